"""The run order of k_conv_dec_nchw_split (16-byte loads of 4 consecutive window columns): window rows of 4 + 3, 4 + 4 + 1
and 4 + 4 + 3 columns (knl 7, 9, 11), and the shapes that keep the flat order (knl 3; Cin 4 with knl 9, whose run-ordered
code words do not fit LDS).  Against the f32 path within 2e-6 of the map's largest value and against the oracle within
1e-4, on ragged batches and on batches that end exactly where their allocation ends."""
import numpy as np
import pytest

import pyoracle as po
from conftest import pkg, rel_err

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")
TOL = 1e-4


def engine(in_chw, layers, params, max_batch, split_bf16):
    eng = pkg("engine").QcnnEngine(0)
    eng.set_option(capi.OPT_LUT_MODE, capi.LUT_MFMA)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.set_option(capi.OPT_DEC_BF16SPLIT, split_bf16)
    eng.load_model(in_chw, layers, params, max_batch)
    return eng


@pytest.mark.parametrize("cin,knl,stride,hw", [(1, 7, 2, (29, 33)), (2, 9, 3, (35, 31)), (3, 11, 4, (39, 43)),
                                              (4, 9, 1, (23, 26)), (2, 3, 2, (21, 24))])
def test_runs_against_f32_path_and_oracle(cin, knl, stride, hw):
    layers = [topo.conv(0, knl, 96, 1, stride), topo.relu(), topo.pool(0, 2, 2), topo.fcnt(24), topo.smax()]
    in_chw = (cin,) + hw
    params = synth.make_params(in_chw, layers, seed=510 + knl)
    rng = np.random.default_rng(511 + cin)
    imgs = (rng.integers(0, 256, size=(1000,) + in_chw).astype(np.float32) - 120.0)
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    engs = {sb: engine(in_chw, layers, params, 1000, sb) for sb in (0, 1)}
    worst = 0.0
    for n in (5, 70, 200, 1000):
        outs = {}
        for sb, eng in engs.items():
            prob, _ = eng.forward_host(imgs[:n])
            assert eng.layer_split(0) == (-3, 2)
            outs[sb] = (eng.layer_output(3, n), prob)
        eng = engs[1]
        m = min(n, 3)
        orc.forward(imgs[n - m:n])
        for l in (3, 4, 5):
            e_inf, e_l2 = rel_err(eng.layer_output_range(l, n - m, m), orc.fm(l))
            assert e_inf <= TOL and e_l2 <= TOL, "n = %d fm[%d] vs oracle: %g %g" % (n, l, e_inf, e_l2)
        dev = float(np.abs(outs[1][0] - outs[0][0]).max() / np.abs(outs[0][0]).max())
        worst = max(worst, dev)
        assert dev <= 2e-6, "n = %d: %g" % (n, dev)
        assert np.abs(outs[1][1] - outs[0][1]).max() <= 1e-5 * outs[0][1].max()
    for eng in engs.values():
        eng.close()
    print("run order, cin %d knl %d stride %d: largest deviation from the f32 path %.3g of the map's largest value"
          % (cin, knl, stride, worst))


@pytest.mark.parametrize("cin,knl,stride,hw", [(2, 9, 2, (37, 41)), (4, 9, 2, (31, 35))])
def test_runs_input_at_the_very_end_of_an_allocation(cin, knl, stride, hw):
    """A batch whose last window row ends at the last byte of its hipMalloc region: the run loads stay inside it."""
    import ctypes as C
    import torch
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    layers = [topo.conv(0, knl, 96, 1, stride), topo.relu(), topo.pool(0, 3, 2), topo.fcnt(24), topo.smax()]
    in_chw = (cin,) + hw
    assert (hw[0] - knl) % stride == 0 and (hw[1] - knl) % stride == 0   # the last window ends at the image's end
    params = synth.make_params(in_chw, layers, seed=520 + cin)
    rng = np.random.default_rng(521)
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
        prob_d = torch.empty((n, 24), dtype=torch.float32, device="cuda:0")
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
