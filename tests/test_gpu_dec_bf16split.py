"""QCNN_OPT_DEC_BF16SPLIT (default on): the decoded first layer read in place computes its products on the bf16 matrix
pipe from exact three-piece splits of the activations and the code words (k_conv_dec_nchw_split).  Against the f32
matrix path (option 0) within 2e-6 of the map's largest value, against the oracle within 1e-4, and with the same
batch-size and permutation invariance as every fast-path kernel."""
import numpy as np
import pytest

import pyoracle as po
from conftest import pkg, rel_err

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")
TOL = 1e-4


def engine(in_chw, layers, params, max_batch, split_bf16, opts=()):
    eng = pkg("engine").QcnnEngine(0)
    eng.set_option(capi.OPT_LUT_MODE, capi.LUT_MFMA)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.set_option(capi.OPT_DEC_BF16SPLIT, split_bf16)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_model(in_chw, layers, params, max_batch)
    return eng


@pytest.mark.parametrize("cin,knl,stride,ct", [(3, 11, 4, 96), (3, 7, 2, 96), (1, 3, 1, 96), (4, 4, 2, 192), (2, 8, 3, 96),
                                                (2, 12, 5, 96), (4, 9, 1, 96)])
def test_split_against_f32_path(cin, knl, stride, ct):
    """Kernel sizes 3 ... 12, 1 - 4 input channels, strides 1 - 5; 1000 / 200 / 70 / 5 images (full and ragged panels,
    one live image tile); host and device input.  The pool map behind the layer within 2e-6 of its largest value of
    the f32 path's, the device-input run bit for bit the host one, the oracle within 1e-4."""
    import torch
    layers = [topo.conv(0, knl, ct, 1, stride), topo.relu(), topo.pool(0, 2, 2), topo.fcnt(40), topo.smax()]
    in_chw = (cin, 29, 31)
    params = synth.make_params(in_chw, layers, seed=290 + cin)
    rng = np.random.default_rng(291)
    imgs = (rng.integers(0, 256, size=(1000,) + in_chw).astype(np.float32) - 120.0)
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    worst = 0.0
    for n in (1000, 200, 70, 5):
        outs = {}
        for sb in (0, 1):
            eng = engine(in_chw, layers, params, 1000, sb)
            prob, top5 = eng.forward_host(imgs[:n])
            assert eng.layer_split(0) == (-3, 2)
            outs[sb] = (eng.layer_output(3, n), prob)
            if sb:
                x = torch.from_numpy(imgs[:n]).to("cuda:0")
                prob_d = torch.empty((n, 40), dtype=torch.float32, device="cuda:0")
                eng.forward_dev(x.data_ptr(), n, prob_d.data_ptr())
                eng.sync()
                assert np.array_equal(prob_d.cpu().numpy(), prob)
                m = min(n, 3)
                orc.forward(imgs[n - m:n])
                for l in (3, 4, 5):
                    e_inf, e_l2 = rel_err(eng.layer_output_range(l, n - m, m), orc.fm(l))
                    assert e_inf <= TOL and e_l2 <= TOL, "n = %d fm[%d] vs oracle: %g %g" % (n, l, e_inf, e_l2)
            eng.close()
        dev = float(np.abs(outs[1][0] - outs[0][0]).max() / np.abs(outs[0][0]).max())
        worst = max(worst, dev)
        assert dev <= 2e-6, "n = %d: %g" % (n, dev)
        assert np.abs(outs[1][1] - outs[0][1]).max() <= 1e-5 * outs[0][1].max()
    print("split-bf16 vs f32 path, cin %d knl %d stride %d ct %d: largest deviation %.3g of the map's largest value"
          % (cin, knl, stride, ct, worst))


def test_alexnet_1000_split_path():
    """AlexNet at 1000 images on the split path: the oracle within 1e-4 on sampled images, the f32 path's top-5 (up to
    scores within 1e-6 of each other), bit-identical results for a 64-image slice and a permuted batch."""
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    params = synth.make_params(in_chw, layers, seed=7)
    imgs = synth.make_images(1000, in_chw, seed=10)
    eng = engine(in_chw, layers, params, 1000, 1, [(capi.OPT_SPLIT, 0)])
    prob, top5 = eng.forward_host(imgs)
    assert eng.layer_split(0) == (-3, 2)
    p64, t64 = eng.forward_host(imgs[936:1000])
    assert np.array_equal(p64, prob[936:1000]) and np.array_equal(t64, top5[936:1000])
    perm = np.random.default_rng(3).permutation(1000)
    pp, tp = eng.forward_host(imgs[perm])
    assert np.array_equal(pp, prob[perm]) and np.array_equal(tp, top5[perm])
    eng.close()
    ref = engine(in_chw, layers, params, 1000, 0, [(capi.OPT_SPLIT, 0)])
    p0, t0 = ref.forward_host(imgs)
    ref.close()
    print("AlexNet 1000 images, split-bf16 vs f32 path: max |d prob| %.3g" % float(np.abs(prob - p0).max()))
    assert np.abs(prob - p0).max() <= 1e-5 * p0.max()
    rows = np.nonzero((top5 != t0).any(axis=1))[0]
    for r in rows:                                        # a top-5 difference only between near-equal scores
        s = np.sort(p0[r])[::-1][:6]
        assert np.diff(s).__abs__().min() <= 1e-6, r
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    pick = [0, 63, 64, 511, 999]
    orc.forward(imgs[pick])
    e_inf, e_l2 = rel_err(prob[pick], orc.fm(len(layers)).reshape(len(pick), -1))
    assert e_inf <= TOL and e_l2 <= TOL, (e_inf, e_l2)


def test_split_input_at_the_very_end_of_an_allocation():
    """The split kernel reads the caller's device buffer in place with the f32 kernel's clamps: batches of 5, 16 and 130
    images ending exactly where their allocation ends, against the oracle."""
    import ctypes as C
    import torch
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    layers = [topo.conv(0, 11, 96, 1, 4), topo.relu(), topo.pool(0, 3, 2), topo.fcnt(40), topo.smax()]
    in_chw = (3, 67, 71)
    params = synth.make_params(in_chw, layers, seed=401)
    rng = np.random.default_rng(402)
    imgs = (rng.integers(0, 256, size=(130,) + in_chw).astype(np.float32) - 120.0)
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    eng = engine(in_chw, layers, params, 130, 1)
    for n in (5, 16, 130):
        nbytes = n * imgs[0].nbytes
        region = (nbytes + (2 << 20) - 1) // (2 << 20) * (2 << 20)
        base = C.c_void_p()
        assert hip.hipMalloc(C.byref(base), region) == 0
        dev = base.value + region - nbytes
        x = np.ascontiguousarray(imgs[:n])
        assert hip.hipMemcpy(C.c_void_p(dev), x.ctypes.data_as(C.c_void_p), nbytes, 1) == 0
        prob_d = torch.empty((n, 40), dtype=torch.float32, device="cuda:0")
        eng.forward_dev(dev, n, prob_d.data_ptr())
        eng.sync()
        assert eng.layer_split(0) == (-3, 2)
        prob = prob_d.cpu().numpy()
        m = min(n, 3)
        orc.forward(imgs[n - m:n])
        e_inf, e_l2 = rel_err(prob[n - m:], orc.fm(len(layers)).reshape(m, -1))
        assert e_inf <= TOL and e_l2 <= TOL, "n = %d: %g %g" % (n, e_inf, e_l2)
        assert hip.hipFree(base) == 0
    eng.close()
