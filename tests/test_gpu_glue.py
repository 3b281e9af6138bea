"""The glue kernels of qcnn_glue.hip element by element (tests/glue_ref.py: float64 references, derived per-element bounds, crafted
inputs; the CPU tier pins all of that to the oracle in tests/test_glue_ref_cpu.py).

Layer tables WITHOUT a conv or FC layer go through qcnn_forward_host, so the network input is the crafted map and the real
forward path — small `live`, streams, the fast path, the fused kernel — carries it into the kernels; the same layers also go
through qcnn_run_layer (which always runs the full-row variants).  Per element, nothing relative to a map's maximum:

  * LRN inside glue_ref.lrn_bound: windows 3 and 5 (k_lrn_stream), 7 and 9 (k_lrn), bet 0.75 (the rsq * sqrt(rsq) form in the
    streaming kernels) and 0.5 / 1.0 (expf / logf), C from 1 (C < n, C <= RAD: the ring prologue) to 256 (channel segments);
  * max-pool bit-identical to glue_ref.pool: pads, clipped and whole ceil-mode windows, negative maps, one peak map per window
    position;
  * the fused LRN + pool inside the interval glue_ref.lrn_pool_interval gives, bit-identical to the separate kernels;
  * soft-max inside glue_ref.softmax_bound, rows summing to 1 within it, C across the 32-class lanes, the four-load seam
    (c + 96 < C) and the 16-value sum seam; a row with a logit of 100 comes out NaN / 0 exactly as the oracle's;
  * top-5 bit-identical to the rule on crafted rows read as they are (one-layer [pool 1x1] and [relu] models);
  * every batch size of glue_ref.BATCHES (qlShift 0 .. 5, a full panel, ragged last panels) returns, image for image, the bits
    of the 300-image batch, and so do the last panel's 44 images run alone;
  * qcnn_run_layer returns the bits of the forward at batch 128; qcnn_fm_dims follows the ceil-mode rule over a grid.

Each test prints the worst err / bound of the kernel variants it ran (-s); k_pool is not among them: qk_pool takes it only
beyond 2^34 rows, which no device holds."""
import numpy as np
import pytest

import glue_ref as gr
import pyoracle as po
from conftest import pkg

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")

N_MAX = 300
TAIL = 256                      # first image of the ragged last panel of the 300-image batch
LDS_TILE_MAX = 1240             # classes whose [C][33] float tile + 32 sums fit 160 KiB: beyond, the one-thread-per-image kernels


def make_engine(in_chw, layers, max_batch=N_MAX, keep_all=1, streams=None, host_chunk=None):
    eng = pkg("engine").QcnnEngine(0)
    eng.set_option(capi.OPT_KEEP_ALL, keep_all)
    if streams is not None:
        eng.set_option(capi.OPT_STREAMS, streams)
    if host_chunk is not None:
        eng.set_option(capi.OPT_HOST_CHUNK, host_chunk)
    eng.load_model(in_chw, layers, {}, max_batch)
    return eng


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def forward_map(eng, x, top5=False):
    """The last feature map (NHWC, the shape of fm[L]) of a forward whose network input is the NHWC map x."""
    prob, t5 = eng.forward_host(gr.nchw(x), want_top5=top5)
    h, w, c = eng.fm_dims(eng.L)
    y = prob.reshape(x.shape[0], h, w, c)
    return (y, t5) if top5 else y


def batches_return_the_same_bits(eng, x, y, what):
    """Every smaller batch, the ragged panel's images alone and qcnn_run_layer (one-layer tables) against the 300-image forward."""
    for nb in gr.BATCHES[:-1]:
        assert bits_equal(forward_map(eng, x[:nb]), y[:nb]), "%s: batch %d differs from the same images in a batch of %d" % (what, nb, N_MAX)
    assert bits_equal(forward_map(eng, x[TAIL:]), y[TAIL:]), "%s: the ragged panel's images alone differ" % what
    if eng.L == 1:
        assert bits_equal(eng.run_layer(0, x[:128], 128), y[:128]), "%s: run_layer differs from forward at batch 128" % what


def report(worst):
    for variant, r in worst.items():
        print("glue variant %s: worst err / bound %s" % (variant, r if isinstance(r, str) else "%.3f" % r))


# ---------------------------------------------------------------------------------------------- LRN
@pytest.mark.parametrize("n", [3, 5, 7, 9])
@pytest.mark.parametrize("bet", [0.75, 0.5, 1.0])
def test_lrn_per_element(n, bet):
    fast = n in (3, 5) and bet == 0.75
    variant = "k_lrn_stream<%d,%s>" % (n, "true" if fast else "false") if n in (3, 5) else "k_lrn (window %d, bet %g)" % (n, bet)
    worst = 0.0
    for i, C in enumerate((1, 2, 3, 5, 7, 16, 96, 256)):
        alp, ini = gr.LRN_SETTINGS[(i + n // 2) % 4]
        what = "%s C=%d alp=%g ini=%g" % (variant, C, alp, ini)
        x = gr.signed_log_uniform((N_MAX, 3, 5, C), seed=1000 + 10 * C + n)
        y64, s = gr.lrn64(x, n, alp, bet, ini)
        eng = make_engine((C, 3, 5), [topo.lorn(n, alp, bet, ini)])
        y = forward_map(eng, x)
        worst = max(worst, gr.check_bound(y, y64, gr.lrn_bound(y64, s, n, bet, not fast), what))
        batches_return_the_same_bits(eng, x, y, what)
        eng.close()
    report({variant: worst})


# ---------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("geo", gr.POOL_GEOMETRIES, ids=lambda g: "k%d_s%d_p%d" % g)
def test_pool_bit_identical(geo):
    knl, stride, pad = geo
    outputs = 0
    for (k, s, p, H, W) in gr.pool_geometries():
        if (k, s, p) != geo:
            continue
        what = "k_pool4 %r on %dx%d" % (geo, H, W)
        x = gr.pool_family(H, W, 5, knl, stride, pad, seed=2000 + H, n=N_MAX)
        want = gr.pool(x, knl, stride, pad)
        eng = make_engine((5, H, W), [topo.pool(pad, knl, stride)])
        assert eng.fm_dims(1) == want.shape[1:]
        y = forward_map(eng, x)
        gr.check_exact(y, want, what, x)
        assert bits_equal(y, want)
        batches_return_the_same_bits(eng, x, y, what)
        eng.close()
        outputs += want.size
    assert outputs
    report({"k_pool4 %r" % (geo,): "0 (bit-identical, %d outputs)" % outputs})


def test_fm_dims_follow_the_ceil_mode_rule():
    """qcnn_fm_dims (pool_out of the engine) over the grid of tests/test_glue_ref_cpu.py::test_output_size_rule_over_a_grid."""
    eng = pkg("engine").QcnnEngine(0)
    cnt = 0
    for H in range(1, 21):
        W = (H * 7) % 19 + 1
        for knl in range(1, 9):
            for stride in range(1, 9):
                for pad in range(0, knl):
                    if not gr.pool_geometry_ok(H, W, knl, stride, pad):
                        continue
                    eng.configure((2, H, W), [topo.pool(pad, knl, stride)], {})
                    assert eng.fm_dims(1) == (gr.pool_out(H, knl, stride, pad), gr.pool_out(W, knl, stride, pad), 2), (H, W, knl, stride, pad)
                    cnt += 1
    assert cnt > 2500
    eng.close()


# ---------------------------------------------------------------------------------------------- fused LRN + pool
@pytest.mark.parametrize("n,bet,C,hw,panels", [(3, 0.75, 2, (22, 13), 8), (3, 0.75, 7, (11, 11), 12), (3, 0.5, 7, (22, 13), 8),
                                               (5, 0.75, 7, (22, 13), 8), (5, 0.75, 3, (11, 11), 12), (5, 1.0, 3, (22, 13), 8)])
def test_lrn_pool_fused_per_element(n, bet, C, hw, panels):
    """22x13 -> 11x6 outputs: partial 4x4 tiles both ways, the last window rows clipped; 11x11 -> 5x5.  `panels` sub-batch panels
    on one stream reach the 192 workgroups the engine wants before it fuses; the last panel holds 77 images."""
    H, W = hw
    fast = bet == 0.75
    variant = "k_lrn_pool<%d,%s>" % (n, "true" if fast else "false")
    alp, ini = gr.LRN_SETTINGS[(n + C) % 4]
    what = "%s C=%d %dx%d alp=%g ini=%g" % (variant, C, H, W, alp, ini)
    N = (panels - 1) * 128 + 77
    layers = [topo.lorn(n, alp, bet, ini), topo.pool(0, 3, 2)]
    x = gr.signed_log_uniform((N, H, W, C), seed=3000 + 10 * C + n)
    y64, s = gr.lrn64(x, n, alp, bet, ini)
    b = gr.lrn_bound(y64, s, n, bet, not fast)
    fus = make_engine((C, H, W), layers, N, keep_all=0, streams=1, host_chunk=0)
    y = forward_map(fus, x)
    with pytest.raises(RuntimeError):
        fus.layer_output_range(1, 0, 1)                    # the normalised map of a fused pair does not exist: the fused kernel ran
    r_fused = gr.check_interval(y, *gr.lrn_pool_interval(y64, b), what)
    sep = make_engine((C, H, W), layers, N, keep_all=1)
    ys = forward_map(sep, x)
    r_sep = gr.check_bound(sep.layer_output(1, N), y64, b, what + " (separate LRN)")
    assert bits_equal(y, ys), what + ": fused and separate kernels differ"
    fus.close(); sep.close()
    report({variant: r_fused, "k_lrn_stream<%d,%s> (%d panels)" % (n, "true" if fast else "false", panels): r_sep})


# ---------------------------------------------------------------------------------------------- soft-max
@pytest.mark.parametrize("C", [3, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 200, 1000, 1400])
def test_softmax_per_element(C):
    variant = "k_softmax_lds" if C <= LDS_TILE_MAX else "k_softmax"
    what = "%s C=%d" % (variant, C)
    x = gr.softmax_logits(N_MAX, C, seed=4000 + C, overflow_at=1)
    eng = make_engine((C, 1, 1), [topo.smax()])
    xm = x.reshape(N_MAX, 1, 1, C)
    y, t5 = forward_map(eng, xm, top5=True)
    y = y.reshape(N_MAX, C)
    keep = np.arange(N_MAX) != 1
    p64 = gr.softmax64(x[keep])
    assert p64.min() >= float(gr.FLT_MIN)
    r = gr.check_bound(y[keep], p64, gr.softmax_bound(p64), what)
    assert abs(y[keep].astype(np.float64).sum(axis=1) - 1.0).max() <= gr.U * (gr.C_EXP + C), what + ": a row does not sum to 1"
    orc = po.COracle((C, 1, 1), [topo.smax()])
    want = orc.run_layer(0, xm[1:2], 1).reshape(C)
    assert np.isnan(want).sum() == 1
    assert np.array_equal(y[1], want, equal_nan=True), what + ": the overflow row is not the oracle's NaN / 0 row"
    assert np.array_equal(t5[keep], gr.top5(y[keep])), what + ": top-5 of the device's own probabilities"
    for nb in gr.BATCHES[:-1]:
        assert np.array_equal(forward_map(eng, xm[:nb]).reshape(nb, C), y[:nb], equal_nan=True), "%s: batch %d" % (what, nb)
    assert np.array_equal(forward_map(eng, xm[1:2]).reshape(C), y[1], equal_nan=True), what + ": the overflow row alone"
    assert bits_equal(forward_map(eng, xm[TAIL:]).reshape(-1, C), y[TAIL:]), what + ": the ragged panel's images alone"
    assert np.array_equal(eng.run_layer(0, xm[:128], 128).reshape(128, C), y[:128], equal_nan=True), what + ": run_layer at batch 128"
    eng.close()
    report({what: r})


# ---------------------------------------------------------------------------------------------- top-5
@pytest.mark.parametrize("C", [3, 5, 33, 200, 1000, 1400])
def test_top5_crafted_rows(C):
    variant = "k_top5_lds" if C <= LDS_TILE_MAX else "k_top5"
    rows = gr.top5_rows(C, seed=5000 + C)
    R = rows.shape[0]
    assert R <= 128
    rng = np.random.default_rng(C)
    idx = np.concatenate([rng.permutation(R) for _ in range(N_MAX // R + 1)])[:N_MAX]           # every row in many image slots
    x = rows[idx]
    orc = po.COracle((C, 1, 1), [topo.relu()])
    for name, layer, rin in (("pool 1x1", topo.pool(0, 1, 1), rows), ("relu", topo.relu(), np.where(np.float32(0.0) < rows, rows, np.float32(0.0)))):
        what = "%s C=%d behind [%s]" % (variant, C, name)
        assert np.array_equal(np.stack([orc.top5(r) for r in rin]), gr.top5(rin)), what + ": the rule differs from the oracle's top-5"
        xin, want = rin[idx], gr.top5(rin)[idx]
        eng = make_engine((C, 1, 1), [layer])
        for lo, hi in [(0, N_MAX), (TAIL, N_MAX)] + [(0, nb) for nb in gr.BATCHES[:-1]]:
            prob, t5 = eng.forward_host(x[lo:hi].reshape(hi - lo, C, 1, 1))
            assert bits_equal(prob, xin[lo:hi]), "%s: images %d..%d do not reach top-5 as they are" % (what, lo, hi)
            bad = np.flatnonzero((t5 != want[lo:hi]).any(axis=1))
            assert bad.size == 0, "%s: images %d..%d: %d rows differ, first %d: got %r, rule %r, row %r" % (
                what, lo, hi, bad.size, bad[0], t5[bad[0]], want[lo + bad[0]], xin[lo + bad[0]])
        eng.close()
    report({"%s C=%d" % (variant, C): "0 (bit-identical, %d crafted rows in %d images)" % (R, N_MAX)})


# ---------------------------------------------------------------------------------------------- a whole glue-only table
def test_glue_only_table_layer_for_layer_and_fast_path():
    """[LRN, padded pool, LRN, soft-max] on a 7-channel 9x11 input: every layer against the float64 reference of ITS OWN input
    (layer-for-layer mode keeps every map), and the fast path with two streams returns the same bits."""
    layers = [topo.lorn(5, 0.01, 0.75, 1.0), topo.pool(1, 3, 2), topo.lorn(3, 0.1, 0.5, 0.5), topo.smax()]
    in_chw = (7, 9, 11)
    x = gr.signed_log_uniform((N_MAX, 9, 11, 7), seed=6000, span=3.0)
    eng = make_engine(in_chw, layers)
    prob, t5 = eng.forward_host(gr.nchw(x))
    fm = [eng.layer_output(l, N_MAX) for l in range(5)]
    assert bits_equal(fm[0], x)
    y64, s = gr.lrn64(fm[0], 5, 0.01, 0.75, 1.0)
    gr.check_bound(fm[1], y64, gr.lrn_bound(y64, s, 5, 0.75, False), "fm[1]")
    gr.check_exact(fm[2], gr.pool(fm[1], 3, 2, 1), "fm[2]", fm[1])
    y64, s = gr.lrn64(fm[2], 3, 0.1, 0.5, 0.5)
    gr.check_bound(fm[3], y64, gr.lrn_bound(y64, s, 3, 0.5, True), "fm[3]")
    p64 = gr.softmax64(fm[3].reshape(N_MAX, -1))
    gr.check_bound(fm[4].reshape(N_MAX, -1), p64, gr.softmax_bound(p64), "fm[4]")
    assert bits_equal(prob, fm[4].reshape(N_MAX, -1)) and np.array_equal(t5, gr.top5(prob))
    fast = make_engine(in_chw, layers, keep_all=0, streams=2)
    prob_f, t5_f = fast.forward_host(gr.nchw(x))
    assert bits_equal(prob_f, prob) and np.array_equal(t5_f, t5)
    for nb in (1, 5, 131):
        p, t = fast.forward_host(gr.nchw(x[:nb]))
        assert bits_equal(p, prob[:nb]) and np.array_equal(t, t5[:nb]), nb
    eng.close(); fast.close()
