"""Dense sums through the few-image kernels (qcnn_small.hip: k_conv_small, k_fc_lut + k_fc_small) on the shapes at which each of
their sub-space chunks, stage groups and tile edges is live (table_probe.SMALL_REACH; tests/test_small_cases_cpu.py pins the
launchers' tile / chunk choice and shows that the oracle alone meets the bound used here).

A probe output (tests/test_gpu_table_probe.py) is one table entry plus zeros; here the parameters are ordinary random ones
(synth.make_params), so every look-up of every tap and sub-space contributes.  Per output ELEMENT, against the float64 sum of
table_probe.dense_expected and relative to the element's own mag = |bias| + sum |x_j c_j| (no max-norm over a map):

    |y - want64| <= gamma(knl^2 M + CsEff + 1) * mag          (FC: gamma(M + CsEff + 1))

— an entry is a chain of CsEff fused multiply-adds, the output a float32 sum of knl^2 M entries and the bias in ANY order, so
the bound holds for every chunking of the sub-space axis and every slice order; it is derived, not measured.  A look-up that
reads another sub-space's entry is off by one entry's size, about mag / (knl^2 M): some 10^4 bounds for the shapes here.

Beside the bound every case asserts which kernel ran (qcnn_get_layer_split reports (-11, 1) after every forward: a shape that
quietly stops being eligible fails instead of testing the panel kernels), and that the outputs of images 0, 1 and 2 of a batch
of three are bit-equal to each image forwarded alone.  One shape must fall through to the panel kernels (a 17x17 window with
K = 128): it reports another code and meets the same bound."""
import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_gpu_table_probe import BASE, FC_FRONT, OPT

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")

CASES = [(name, 0) for name in sorted(tp.SMALL_REACH)] + [(name, 1) for name in sorted(tp.SMALL_REACH) if tp.SHAPES[name][0] == "fc"]


def model_for(kind, g):
    """(in_chw, layers, layer under test): as in the table probes — a conv shape is the first layer of [conv, relu, fcnt(8), smax],
    an FC shape consumes the 1x1 map of a front conv layer."""
    if kind == "conv":
        return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"]), topo.relu(),
                                            topo.fcnt(8), topo.smax()], 0
    in_chw, front = FC_FRONT[g["D"]]
    return in_chw, [front, topo.fcnt(g["Ct"]), topo.smax()], 1


def forward(eng, kind, l, inp):
    """(pre-ReLU output of layer l, the input it consumed, the family code it reports) of a forward of the images inp."""
    n = inp.shape[0]
    eng.forward_host(inp)
    code = eng.layer_split(l)
    if kind == "conv":
        return eng.layer_output(l + 1, n), None, code
    return eng.layer_output(l + 1, n).reshape(n, -1), eng.layer_output(l, n).reshape(n, -1), code


def run_case(shape, packed, seed, code_ok):
    """The dense-sum check of one shape; code_ok(code) is asserted after every forward.  Returns (family codes, worst err / bound)."""
    kind, g, M, K, Cs, _ = shape
    in_chw, layers, l = model_for(kind, g)
    spec = synth.quant_spec(in_chw, layers)
    spec[l] = dict(spec[l], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=seed, spec=spec)
    eng = pkg("engine").QcnnEngine(0)
    for k, v in dict(BASE, small=1, packed=packed).items():
        eng.set_option(OPT[k], v)
    eng.load_model(in_chw, layers, params, 3)
    x = tp.activations("conv", dict(H=in_chw[1], W=in_chw[2], Cin=in_chw[0]), 3, seed=seed + 1, scaled=False)   # NHWC
    inp = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    y3, xin3, code = forward(eng, kind, l, inp)
    assert code_ok(code), "batch of three: family code %r" % (code,)
    codes = [code]
    want64, mag = tp.dense_expected(kind, g, x if kind == "conv" else xin3, params[l])
    worst = tp.dense_check(y3, want64, mag, tp.dense_count(kind, g, M, Cs), what="batch of three")
    for i in range(3):
        y1, xin1, code = forward(eng, kind, l, inp[i:i + 1])
        assert code_ok(code), "image %d alone: family code %r" % (i, code)
        codes.append(code)
        if kind == "fc":
            assert np.array_equal(xin1[0], xin3[i]), "image %d: the layer's input differs between the batch and the image alone" % i
        assert np.array_equal(y1[0], y3[i]), "image %d alone differs from its output in the batch of three: %d elements" % (
            i, int((y1[0] != y3[i]).sum()))
    eng.close()
    return codes, worst


@pytest.mark.parametrize("name,packed", CASES, ids=["%s%s" % (n, "-packed" if p else "") for n, p in CASES])
def test_dense_sums_through_the_few_image_kernels(name, packed):
    codes, worst = run_case(tp.SHAPES[name], packed, 71, lambda code: code == (-11, 1))
    print("%s%s: codes %r worst err / bound %.3f" % (name, " packed" if packed else "", codes, worst))
    assert worst <= 1.0


def test_a_window_too_large_for_the_few_image_table_falls_through():
    """289 pixels x (128 + 8) floats + 289 x 32 assignment bytes > the kernel's LDS budget at a 1x1 tile: the panel kernel runs
    the layer (and says so), inside the same bound."""
    codes, worst = run_case(tp.SMALL_FALL_THROUGH, 0, 73, lambda code: code[0] != -11)
    print("fall-through: codes %r worst err / bound %.3f" % (codes, worst))
    assert worst <= 1.0
