"""Dense sums through every conv family on maps smaller than the kernel and smaller than a tile (the tg_* shapes of
tests/table_probe.py: 1 x 1, one output row, one output column, windows clipped by the padding on both sides at once, pad = knl - 1,
stride > knl, a tile of eight stages cut into slices of one and two).  tests/test_tiny_cases_cpu.py pins the planner's and the
launchers' choice per shape (table_probe.TINY_REACH), proves from the kernels' tile arithmetic that every workgroup of every launch
here has at least one source row, one column and one stage, shows that the references alone meet the bound and that a missing,
doubled or clamped-instead-of-zero term does not.

Per shape and live family — forced through the option values of the suite's family descriptors, its own code required after EVERY
launch (qcnn_get_layer_split) — run_layer on 131 images (half-panel families also 70 and 5; split forms 125) is held per output
ELEMENT to the float64 sum of table_probe.dense_expected:

    |y - want64| <= gamma(knl^2 M + CsEff + 1) * mag,   mag = |bias| + sum |x_j c_j|

(derived: an entry is a chain of CsEff fused multiply-adds, the output a float32 sum of at most knl^2 M entries and the bias in any
order; a tap in the padding adds nothing).  Beside the bound: the exact builder returns the oracle's bits; the sliding, symmetric and
eight-wave families return the tile kernel's bits; the ragged panel's three images alone return the bits they have in the batch;
the forward's conv map is run_layer's.  The few-image kernel runs every shape at 1 and 3 images through a forward, code (-11, 1);
the decoded panel form runs the Cin = 3 shapes at 131 and 5 images within gamma(Cin knl^2 + 1) * mag.

k_dense (the precise path) runs the same geometries, and tg_1x1 at 3x3 / 2 pad 1, declared dense, 131 images, per element within
gamma(Cin knl^2 + 1) * mag of the float64 restatement of its tap rule (test_tiny_cases_cpu.dense_rule64): a tap whose source row or
column lies outside the map contributes 0.  In a batch of 131 an out-of-map read lands in another image's activations.

A conv layer with padSiz < 0 or padSiz >= knlSiz is refused by qcnn_model_begin, with a message, and the engine stays usable.
NOTHING here launches such a layer: a tile wholly in the padding has no stage, and its first stage's position is a division by
zero into a load address (tests/test_tiny_cases_cpu.py holds the counter-examples on the CPU)."""
import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_gpu_panel_cases import LIKE_TILE, ORACLE_IMAGES, ORDER, make_engine, model_for
from test_gpu_table_probe import BASE, DEC_PANEL, EXACT, OPT, SMALL, TILE, code_ok
from test_panel_cases_cpu import FAMS
from test_table_probe_cpu import oracle_out
from test_tiny_cases_cpu import dense_rule64

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
QcnnError = pkg("engine").QcnnError

N = tp.PANEL_BATCH


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def case(name, seed):
    """(kind, g, M, K, Cs, in_chw, layers, parameters of the whole model, x NHWC [131], the same NCHW)."""
    kind, g, M, K, Cs, _ = tp.TINY_SHAPES[name]
    in_chw, layers = model_for(g)
    spec = synth.quant_spec(in_chw, layers)
    spec[0] = dict(spec[0], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=seed, spec=spec)
    x = tp.activations(kind, g, N, seed=seed + 1, scaled=False)
    return kind, g, M, K, Cs, in_chw, layers, params, x, np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def families(name):
    return [("exact", EXACT), ("tile", TILE)] + [(k, FAMS[k]) for k in ORDER if k != "tile" and k in tp.TINY_REACH[name]["live"]]


def few_images(name, in_chw, layers, params, inp, want64, mag, n_terms):
    """The few-image kernel: forwards of 1 and 3 images, code (-11, 1), the conv map held to the same bound."""
    eng = make_engine(in_chw, layers, params, SMALL["opts"])
    worst = 0.0
    for n in SMALL["n"]:
        eng.forward_host(inp[:n])
        got = eng.layer_split(0)
        assert got == SMALL["code"], "%s / few-image / %d images: family code %r" % (name, n, got)
        y = eng.layer_output(1, n)
        worst = max(worst, tp.dense_check(y, want64[:n], mag[:n], n_terms, what="%s / few-image / %d images" % (name, n)))
        assert same_bits(eng.layer_output(2, n), np.maximum(y, np.float32(0)))
    eng.close()
    return worst


@pytest.mark.parametrize("name", tp.TINY_TABLE)
def test_dense_sums_through_the_table_families(name):
    kind, g, M, K, Cs, in_chw, layers, params, x, inp = case(name, 187)
    want64, mag = tp.dense_expected(kind, g, x, params[0])
    n_terms = tp.dense_count(kind, g, M, Cs)
    sel = list(ORACLE_IMAGES)
    oracle = oracle_out(kind, g, params[0], x[sel])
    tile = None
    worst, differ, codes = {}, {}, {}
    for key, f in families(name):
        eng = make_engine(in_chw, layers, params, f["opts"])
        label = f["label"]
        batches = (tp.PANEL_SPLIT_BATCH,) if key.startswith("split_") else (N,) + (tp.PANEL_HALF_BATCHES if key.startswith("half8") else ())
        assert sorted(batches) == sorted(f["n"])
        for n in batches:
            what = "%s / %s / %d images" % (name, label, n)
            y = eng.run_layer(0, x[:n], n)
            got = eng.layer_split(0)
            assert code_ok(f["code"], got), "%s: family code %r, expected %r" % (what, got, f["code"])
            codes[label] = got
            print("%s: code %r" % (what, got))
            r = tp.dense_check(y, want64[:n], mag[:n], n_terms, what=what)
            worst[label] = max(worst.get(label, 0.0), r)
            if f["exact"]:
                idx = [i for i in sel if i < n]
                assert np.array_equal(y[idx], oracle[:len(idx)]), "%s: %d elements differ from the oracle's" % (
                    what, int((y[idx] != oracle[:len(idx)]).sum()))
            if key == "tile":
                tile = y
            if key in LIKE_TILE:
                assert np.array_equal(y, tile[:n]), "%s: %d elements differ from the tile kernel's" % (what, int((y != tile[:n]).sum()))
            if key.startswith("half8"):
                differ[label] = differ.get(label, 0) + int((y != tile[:n]).sum())
            if n == N:                                                           # the ragged panel's three images alone
                alone = eng.run_layer(0, x[N - 3:], 3)
                assert code_ok(f["code"], eng.layer_split(0)), "%s: the last three images alone ran %r" % (what, eng.layer_split(0))
                assert np.array_equal(alone, y[N - 3:]), "%s: the last three images alone differ in %d elements" % (
                    what, int((alone != y[N - 3:]).sum()))
            if n == batches[0]:                                                  # the forward path: first layer of the model
                eng.forward_host(inp[:n])
                got = eng.layer_split(0)
                assert code_ok(f["code"], got), "%s, forward: family code %r, expected %r" % (what, got, f["code"])
                conv, relu = eng.layer_output(1, n), eng.layer_output(2, n)
                assert np.array_equal(conv, y), "%s: the forward's conv map differs from run_layer's in %d elements" % (what, int((conv != y).sum()))
                assert np.array_equal(relu, np.maximum(y, np.float32(0))), "%s: the ReLU map is not the conv map's clamp" % what
        eng.close()
    worst[SMALL["label"]] = few_images(name, in_chw, layers, params, inp, want64, mag, n_terms)
    for label, v in worst.items():
        extra = ", %d elements differ from the tile kernel's" % differ[label] if label in differ else ""
        print("%s: %s code %r worst err / bound %.3f%s" % (name, label, codes.get(label, SMALL["code"]), v, extra))
    assert all(v <= 1.0 for v in worst.values())


@pytest.mark.parametrize("name", tp.TINY_DEC)
def test_dense_sums_through_the_decoded_panel_form(name):
    """One 3-dim sub-space: the clamped instantiations of k_conv_dec at 131 images (run_layer and forward) and at 5 (a forward, which
    tells the launch how many images its panel holds: the 16-image instantiation), beside the table kernels and the few-image kernel
    on the same layer."""
    kind, g, M, K, Cs, in_chw, layers, params, x, inp = case(name, 189)
    want64, mag = tp.dense_expected(kind, g, x, params[0])
    n_terms = tp.dense_count(kind, g, M, Cs)
    worst = {}
    for f in (EXACT, TILE):
        eng = make_engine(in_chw, layers, params, f["opts"])
        y = eng.run_layer(0, x, N)
        assert code_ok(f["code"], eng.layer_split(0)), "%s / %s: family code %r" % (name, f["label"], eng.layer_split(0))
        worst[f["label"]] = tp.dense_check(y, want64, mag, n_terms, what="%s / %s" % (name, f["label"]))
        if f["exact"]:
            sel = list(ORACLE_IMAGES)
            assert np.array_equal(y[sel], oracle_out(kind, g, params[0], x[sel])), "%s: the exact builder differs from the oracle" % name
        eng.close()
    worst[SMALL["label"]] = few_images(name, in_chw, layers, params, inp, want64, mag, n_terms)
    rel = tp.dec_dense_rel(kind, g)
    eng = make_engine(in_chw, layers, params, DEC_PANEL["opts"])
    y = eng.run_layer(0, x, N)
    assert eng.layer_split(0) == DEC_PANEL["code"], "%s / decoded: family code %r" % (name, eng.layer_split(0))
    worst[DEC_PANEL["label"]] = tp.dense_check_rel(y, want64, mag, rel, what=name + " / decoded, panel form")
    alone = eng.run_layer(0, x[N - 3:], 3)
    assert same_bits(alone, y[N - 3:]), "%s: the ragged panel's three images alone differ" % name
    for n in (N, 5):
        eng.forward_host(inp[:n])
        assert eng.layer_split(0) == DEC_PANEL["code"], "%s / decoded, forward of %d: family code %r" % (name, n, eng.layer_split(0))
        yn = eng.layer_output(1, n)
        tp.dense_check_rel(yn, want64[:n], mag[:n], rel, what="%s / decoded, forward of %d" % (name, n))
        assert same_bits(yn, y[:n]), "%s: a forward of %d images differs from the same images of the batch of %d: %d elements" % (
            name, n, N, int((yn != y[:n]).sum()))
    eng.close()
    for label, v in worst.items():
        print("%s: %s worst err / bound %.3f" % (name, label, v))
    assert all(v <= 1.0 for v in worst.values())


# ---------------------------------------------------------------- the precise path ----
@pytest.mark.parametrize("name", sorted(tp.TINY_DENSE))
def test_dense_kernel_on_tiny_maps(name):
    """k_dense on 131 images: bias plus Cin knl^2 fused multiply-adds in any order, gamma(Cin knl^2 + 1) mag against the float64
    restatement of the tap rule.  tg_1x1_s2: every tap is outside the map or dropped by the reference's rule at output 0 — the output is
    the bias, bit for bit; the unguarded upper bound added the pixel one row behind the map: the next image's."""
    g = tp.TINY_DENSE[name]
    in_chw, layers = model_for(g)
    dense = synth.make_dense_params(in_chw, layers, seed=191)
    x = tp.activations("conv", g, N, seed=192, scaled=False)
    want64, mag = dense_rule64(g, x, dense[0]["bias"], dense[0]["weights"])
    eng = pkg("engine").QcnnEngine(0)
    for k, v in BASE.items():
        eng.set_option(OPT[k], v)
    eng.load_dense_model(in_chw, layers, dense, N)
    y = eng.run_layer(0, x, N)
    worst = tp.dense_check(y, want64, mag, g["Cin"] // g["grp"] * g["knl"] ** 2 + 1, what=name + " / k_dense")
    alone = eng.run_layer(0, x[N - 3:], 3)
    assert same_bits(alone, y[N - 3:]), "%s / k_dense: the ragged panel's three images alone differ" % name
    eng.close()
    if name == "tg_1x1_s2":
        assert np.array_equal(y, np.tile(dense[0]["bias"], (N, 1, 1, 1)))
        # three panels: pixel (1, 1) "of" panel 0's 1 x 1 map is row 2 Cin of the buffer — panel 2's activations, images 256 ..
        n3 = 2 * 128 + 3
        x3 = tp.activations("conv", g, n3, seed=194, scaled=False)
        eng = pkg("engine").QcnnEngine(0)
        for k, v in BASE.items():
            eng.set_option(OPT[k], v)
        eng.load_dense_model(in_chw, layers, dense, n3)
        y3 = eng.run_layer(0, x3, n3)
        eng.close()
        assert np.array_equal(y3, np.tile(dense[0]["bias"], (n3, 1, 1, 1))), "%d outputs are not the bias" % int((y3 != dense[0]["bias"]).sum())
    print("%s: k_dense worst err / bound %.3f" % (name, worst))


# ---------------------------------------------------------------- paddings the tile arithmetic cannot take ----
REFUSED = [(3, 3, "pad = knl"), (1, 1, "a 1x1 layer with pad 1"), (2, 1, "pad > knl"), (5, 3, "pad > knl"), (-1, 3, "a negative padding")]


@pytest.mark.parametrize("pad, knl, why", REFUSED)
def test_a_padding_outside_the_kernel_is_refused_at_load(pad, knl, why):
    """qcnn_model_begin: error code and message (layer, rule), through the quantised and the dense loader; no launch.  The same engine
    then loads and runs a model at pad = knl - 1, the largest admitted."""
    in_chw = (32, 4, 4)
    layers = [topo.conv(1, 3, 32, 1, 1), topo.relu(), topo.conv(pad, knl, 128, 1, 1), topo.relu(), topo.fcnt(8), topo.smax()]
    eng = pkg("engine").QcnnEngine(0)
    for k, v in BASE.items():
        eng.set_option(OPT[k], v)
    arr = (pkg("capi").QcnnLayerDesc * len(layers))(*[pkg("capi").layer_desc(l) for l in layers])
    assert eng.lib.qcnn_model_begin(eng.h, len(layers), arr, *in_chw) != 0
    msg = eng.lib.qcnn_last_error(eng.h).decode()
    assert "layer 2" in msg and "padding %d" % pad in msg and "kernel size %d" % knl in msg, msg
    with pytest.raises(QcnnError, match="layer 2: conv padding"):
        eng.load_dense_model(in_chw, layers, {}, N)
    # the engine is usable afterwards
    kind, g, M, K, Cs, in_chw, layers, params, x, inp = case("tg_pad2", 193)
    eng.load_model(in_chw, layers, params, N)
    y = eng.run_layer(0, x[:5], 5)
    assert eng.layer_split(0) == TILE["code"]
    want64, mag = tp.dense_expected(kind, g, x[:5], params[0])
    tp.dense_check(y, want64, mag, tp.dense_count(kind, g, M, Cs), what="tg_pad2 behind a refused model (%s)" % why)
    eng.close()
