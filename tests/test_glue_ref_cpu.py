"""CPU tier of the glue-kernel checks: tests/glue_ref.py against the C oracle (and, where oracle/_ref/libqcnn_ref.so exists, the
compiled reference) on the crafted inputs, the output-size rule over a grid, and a set of deliberately wrong variants of every
operation that the checks of glue_ref must notice on those inputs.  The GPU tier (tests/test_gpu_glue.py) applies the same
references, bounds and inputs to the kernels."""
import numpy as np
import pytest

import glue_ref as gr
import pyoracle as po
from conftest import pkg

topo = pkg("topology")

LRN_C = (1, 2, 3, 5, 7, 16, 96)
SMAX_C = (3, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 200, 1000, 1400)
TOP5_C = (3, 5, 33, 200, 1000, 1400)


def oracle_layer(in_chw, layer, x):
    orc = po.COracle(in_chw, [layer])
    y = orc.run_layer(0, x, x.shape[0])
    orc.close()
    return y


def ref_layer(tmp_path, in_chw, layer, x):
    """The compiled reference, one image at a time (it is a batch-1 program)."""
    ref = po.RefLib()
    ref.load_custom(str(tmp_path), "none", in_chw, [layer])
    return np.concatenate([ref.run_layer(0, x[i:i + 1]) for i in range(x.shape[0])])


# ------------------------------------------------------------------------------ glue_ref against the oracle
def test_glue_only_table_runs_in_the_oracle():
    layers = [topo.lorn(5, 0.01, 0.75, 1.0), topo.pool(1, 3, 2), topo.lorn(3, 0.1, 0.5, 0.5), topo.smax()]
    orc = po.COracle((7, 9, 11), layers)
    x = gr.signed_log_uniform((3, 9, 11, 7), seed=1, span=3.0)
    orc.forward(gr.nchw(x))
    assert np.array_equal(orc.fm(0), x)
    y64, s = gr.lrn64(x, 5, 0.01, 0.75, 1.0)
    gr.check_bound(orc.fm(1), y64, gr.lrn_bound(y64, s, 5, 0.75, True), "fm[1]")
    assert np.array_equal(orc.fm(2), gr.pool(orc.fm(1), 3, 2, 1))
    assert all(np.isfinite(orc.fm(l)).all() for l in range(5))


@pytest.mark.parametrize("n", [3, 5, 7, 9])
@pytest.mark.parametrize("bet", [0.75, 0.5, 1.0])
def test_lrn_oracle_inside_the_libm_bound_every_element(n, bet, tmp_path):
    worst = 0.0
    for i, C in enumerate(LRN_C):
        alp, ini = gr.LRN_SETTINGS[(i + n // 2) % 4]
        x = gr.signed_log_uniform((6, 3, 5, C), seed=100 + C)
        y64, s = gr.lrn64(x, n, alp, bet, ini)
        bound = gr.lrn_bound(y64, s, n, bet, True)
        ly = topo.lorn(n, alp, bet, ini)
        worst = max(worst, gr.check_bound(oracle_layer((C, 3, 5), ly, x), y64, bound, "oracle LRN n=%d bet=%g C=%d" % (n, bet, C)))
        if po.have_ref() and C in (2, 7, 16):
            gr.check_bound(ref_layer(tmp_path, (C, 3, 5), ly, x[:2]), y64[:2], bound[:2], "reference LRN n=%d bet=%g C=%d" % (n, bet, C))
    print("oracle LRN n=%d bet=%g: worst err / bound %.3f" % (n, bet, worst))


def test_lrn_reaches_large_and_small_scales():
    """The crafted maps do what they are for: s from ~ini to the thousands, and an ini below 1."""
    x = gr.signed_log_uniform((6, 3, 5, 16), seed=116)
    s = gr.lrn64(x, 5, 1e-1, 0.75, 0.5)[1]
    assert s.min() < 0.6 and s.max() > 2000.0
    s = gr.lrn64(x, 5, 1e-4, 0.75, 1.0)[1]
    assert s.min() < 1.0001 and s.max() > 2.0
    assert (x < 0).mean() > 0.3 and (x > 0).mean() > 0.3 and np.abs(x).min() < 0.01 and np.abs(x).max() > 100.0


@pytest.mark.parametrize("geo", gr.pool_geometries(), ids=lambda g: "k%d_s%d_p%d_%dx%d" % g)
def test_pool_matches_oracle_bit_for_bit(geo, tmp_path):
    knl, stride, pad, H, W = geo
    x = gr.pool_family(H, W, 3, knl, stride, pad, seed=7)
    want = gr.pool(x, knl, stride, pad)
    assert want.dtype == np.float32
    gr.check_exact(oracle_layer((3, H, W), topo.pool(pad, knl, stride), x), want, "oracle pool %r" % (geo,), x)
    if po.have_ref():
        gr.check_exact(ref_layer(tmp_path, (3, H, W), topo.pool(pad, knl, stride), x[:8]), want[:8], "reference pool %r" % (geo,), x)


def test_pool_geometries_cover_clipped_and_whole_last_windows():
    for k, s, p in gr.POOL_GEOMETRIES:
        sizes = [size for (kk, ss, pp, H, W) in gr.pool_geometries() if (kk, ss, pp) == (k, s, p) for size in (H, W)]
        assert len(sizes) >= 4, (k, s, p)
        clipped = {gr.last_window_clipped(size, k, s, p) for size in sizes}
        # ceil mode makes the last window end at or beyond H + pad: with a pad it is always clipped
        assert clipped == ({True} if p else {True, False}), (k, s, p, clipped)
        assert any(size % 2 for size in sizes) and any(size % 2 == 0 for size in sizes)
    assert any(H != W for (_, _, _, H, W) in gr.pool_geometries())


def test_generator_refuses_empty_windows():
    assert not gr.pool_geometry_ok(8, 8, 3, 3, 1)          # Ho = 4, the last window starts at row 8
    assert not gr.pool_geometry_ok(7, 7, 2, 2, 2)          # pad >= knl: the first window lies in the padding
    assert gr.pool_geometry_ok(7, 7, 3, 3, 1)
    with pytest.raises(ValueError):
        gr.pool(np.ones((1, 8, 8, 1), np.float32), 3, 3, 1)
    for k, s, p, H, W in gr.pool_geometries():
        for size in (H, W):
            assert (gr.pool_out(size, k, s, p) - 1) * s - p < size and p < k


def test_output_size_rule_over_a_grid():
    """topology.fmap_sizes and glue_ref.pool_out against the oracle's fm_dims: ceil mode with pad."""
    cnt = 0
    for H in range(1, 21):
        W = (H * 7) % 19 + 1
        for knl in range(1, 9):
            for stride in range(1, 9):
                for pad in range(0, knl):
                    if not gr.pool_geometry_ok(H, W, knl, stride, pad):
                        continue
                    ly = [topo.pool(pad, knl, stride)]
                    orc = po.COracle((2, H, W), ly)
                    want = orc.fm_dims(1)
                    orc.close()
                    assert topo.fmap_sizes((2, H, W), ly)[1] == want, (H, W, knl, stride, pad)
                    assert (gr.pool_out(H, knl, stride, pad), gr.pool_out(W, knl, stride, pad), 2) == want
                    cnt += 1
    assert cnt > 2500


@pytest.mark.parametrize("C", SMAX_C)
def test_softmax_oracle_inside_the_bound_every_element(C, tmp_path):
    x = gr.softmax_logits(12, C, seed=200 + C, overflow_at=1)
    y = oracle_layer((C, 1, 1), topo.smax(), x.reshape(12, 1, 1, C)).reshape(12, C)
    keep = np.arange(12) != 1
    p64 = gr.softmax64(x[keep])
    assert p64.min() >= float(gr.FLT_MIN)                  # no subnormal output outside the overflow row
    r = gr.check_bound(y[keep], p64, gr.softmax_bound(p64), "oracle soft-max C=%d" % C)
    assert abs(y[keep].astype(np.float64).sum(axis=1) - 1.0).max() <= gr.U * (gr.C_EXP + C)
    want = overflow_row(x[1])
    assert np.isnan(want).sum() == 1 and (want[~np.isnan(want)] == 0.0).all()
    assert np.array_equal(y[1], want, equal_nan=True)
    if po.have_ref():
        yr = ref_layer(tmp_path, (C, 1, 1), topo.smax(), x[:4].reshape(4, 1, 1, C)).reshape(4, C)
        gr.check_bound(yr[[0, 2, 3]], p64[:3], gr.softmax_bound(p64[:3]), "reference soft-max C=%d" % C)
        assert np.array_equal(yr[1], want, equal_nan=True)
    print("oracle soft-max C=%d: worst err / bound %.3f" % (C, r))


def overflow_row(x):
    """The float32 sequence on a row with a logit of 100: expf gives +inf, the sum is +inf, inf / inf = NaN, the rest 0."""
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x.astype(np.float32))
        return e / np.float32(np.inf) if np.isinf(e).any() else e / e.sum(dtype=np.float32)


@pytest.mark.parametrize("C", TOP5_C)
def test_top5_rule_matches_oracle(C):
    rows = gr.top5_rows(C, seed=300 + C)
    orc = po.COracle((C, 1, 1), [topo.relu()])
    want = np.stack([orc.top5(r) for r in rows])
    assert np.array_equal(gr.top5(rows), want)
    if C >= 5:
        assert (want == 0).all(axis=1).sum() >= 4          # rows with nothing above FLT_MIN name class 0 five times
        assert any(len(set(t)) == 5 for t in want.tolist())


def test_top5_rule_matches_the_compiled_reference(tmp_path):
    if not po.have_ref():
        pytest.skip("oracle/_ref/libqcnn_ref.so not built")
    for C in (5, 200):
        rows = gr.top5_rows(C, seed=300 + C)
        ref = po.RefLib()
        ref.load_custom(str(tmp_path), "none", (C, 1, 1), [topo.pool(0, 1, 1)])
        want = gr.top5(rows)
        for i, r in enumerate(rows):
            ref.run_layer(0, r.reshape(1, 1, 1, C))
            assert np.array_equal(ref.top5(), want[i]), (C, i)


# ------------------------------------------------------------------------------ wrong variants must be noticed
def variant_edges(size, knl, stride, pad, low="", high="", floor=False):
    """[(low, high)] of every output along one axis; the keywords switch single mistakes on."""
    cnt = (size + 2 * pad - knl) // stride + 1 if floor else gr.pool_out(size, knl, stride, pad)
    out = []
    for o in range(cnt):
        lo, hi = max(0, o * stride - pad), min(size, o * stride + knl - pad) - 1
        if low == "+1": lo = max(0, o * stride - pad + 1)
        if low == "-1": lo = max(0, o * stride - pad - 1)
        if low == "clip": lo = max(1, o * stride - pad)
        if high == "-1": hi = min(size, o * stride + knl - pad - 1) - 1
        if high == "+1": hi = min(size, o * stride + knl - pad + 1) - 1
        if high == "clip": hi = min(size - 1, o * stride + knl - pad) - 1
        out.append((lo, hi))
    return out


def pool_variant(x, knl, stride, pad, start=None, **mistake):
    """Max-pool as plain loops, independent of glue_ref.pool (an empty window gives NaN)."""
    n, H, W, C = x.shape
    eh, ew = variant_edges(H, knl, stride, pad, **mistake), variant_edges(W, knl, stride, pad, **mistake)
    y = np.full((n, len(eh), len(ew), C), np.nan, np.float32)
    for i, (hl, hu) in enumerate(eh):
        for j, (wl, wu) in enumerate(ew):
            if hl <= hu and wl <= wu:
                y[:, i, j] = x[:, hl:hu + 1, wl:wu + 1].max(axis=(1, 2))
                if start is not None:
                    y[:, i, j] = np.maximum(y[:, i, j], np.float32(start))
    return y


def same_windows(H, W, knl, stride, pad, m):
    """A mistake that changes no window of this geometry (one output per axis whose window is the whole axis) is no mutant."""
    return all(variant_edges(size, knl, stride, pad, **m) == variant_edges(size, knl, stride, pad) for size in (H, W))


def noticed(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


POOL_MUTANTS = [dict(low="+1"), dict(low="-1"), dict(low="clip"), dict(high="-1"), dict(high="+1"), dict(high="clip")]


@pytest.mark.parametrize("geo", gr.pool_geometries(), ids=lambda g: "k%d_s%d_p%d_%dx%d" % g)
def test_pool_mutants_fail(geo):
    knl, stride, pad, H, W = geo
    peaks = gr.pool_peaks(H, W, 3, knl, stride, pad, seed=11)
    assert peaks.shape[0] == knl * knl
    gr.check_exact(pool_variant(peaks, knl, stride, pad), gr.pool(peaks, knl, stride, pad), "plain loops")
    mutants = [m for m in POOL_MUTANTS if not same_windows(H, W, knl, stride, pad, m)]
    assert len(mutants) >= 4
    for m in mutants:
        got = pool_variant(peaks, knl, stride, pad, **m)
        assert noticed(gr.check_exact, got, gr.pool(peaks, knl, stride, pad), "mutant"), "window mutant %r passes on the peak maps of %r" % (m, geo)
    neg = gr.pool_negative(2, H, W, 3, seed=12)
    assert noticed(gr.check_exact, pool_variant(neg, knl, stride, pad, start=0.0), gr.pool(neg, knl, stride, pad), "mutant")
    fam = gr.pool_family(H, W, 3, knl, stride, pad, seed=13)
    for m in mutants + [dict(start=0.0)]:
        assert noticed(gr.check_exact, pool_variant(fam, knl, stride, pad, **m), gr.pool(fam, knl, stride, pad), "mutant"), (m, geo)
    assert (gr.pool(fam, knl, stride, pad) < 0).any()       # windows whose maximum is negative exist


def test_floor_mode_output_size_fails():
    for k, s, p in gr.POOL_GEOMETRIES:
        hit = 0
        for (kk, ss, pp, H, W) in gr.pool_geometries():
            if (kk, ss, pp) != (k, s, p):
                continue
            x = gr.pool_signed(1, H, W, 2, seed=14)
            if (H + 2 * p - k) % s or (W + 2 * p - k) % s:
                assert noticed(gr.check_exact, pool_variant(x, k, s, p, floor=True), gr.pool(x, k, s, p), "floor mode")
                hit += 1
        assert hit or s == 1, (k, s, p)                     # stride 1: floor and ceil agree, nothing to tell apart


def lrn_variant(x, n, alp, bet, ini, centre=True, divide=True, ulps=0):
    """LRN in float64, rounded once to float32; the keywords switch single mistakes on."""
    x64 = x.astype(np.float64)
    C = x.shape[-1]
    rad = (n - 1) // 2 if centre else 0
    sq = np.zeros(x.shape[:-1] + (C + n - 1,))
    sq[..., rad:rad + C] = x64 * x64
    coeff = float(gr.lrn_coeff(alp, n)) if divide else float(np.float32(alp))
    s = float(np.float32(ini)) + coeff * sum(sq[..., j:j + C] for j in range(n))
    scale = (s ** -bet).astype(np.float32)
    scale = (scale.view(np.int32) + ulps).view(np.float32)
    return (x64 * scale.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("n,libm", [(3, False), (5, False), (5, True), (9, True)])
def test_lrn_mutants_fail(n, libm):
    for alp, ini in gr.LRN_SETTINGS:
        for C in (3, 7, 16):
            x = gr.signed_log_uniform((6, 3, 5, C), seed=400 + C)
            y64, s = gr.lrn64(x, n, alp, 0.75, ini)
            bound = gr.lrn_bound(y64, s, n, 0.75, libm)
            what = "n=%d alp=%g ini=%g C=%d" % (n, alp, ini, C)
            assert gr.check_bound(lrn_variant(x, n, alp, 0.75, ini), y64, bound, what) <= 0.6    # float64 rounded twice: well inside
            assert noticed(gr.check_bound, lrn_variant(x, n, alp, 0.5, ini), y64, bound, what), "bet 0.5 passes: " + what
            assert noticed(gr.check_bound, lrn_variant(x, n, alp, 0.75, ini, centre=False), y64, bound, what), "window not centred passes: " + what
            assert noticed(gr.check_bound, lrn_variant(x, n, alp, 0.75, ini, divide=False), y64, bound, what), "alp not divided passes: " + what
            for ulps in (8, -8):
                assert noticed(gr.check_bound, lrn_variant(x, n, alp, 0.75, ini, ulps=ulps), y64, bound, what), "scale %+d ulp passes: %s" % (ulps, what)


@pytest.mark.parametrize("C", SMAX_C)
def test_softmax_mutant_fails(C):
    x = gr.softmax_logits(12, C, seed=200 + C, overflow_at=None)
    p64 = gr.softmax64(x)
    bound = gr.softmax_bound(p64)
    e = np.exp(x.astype(np.float64))
    assert gr.check_bound((e / e.sum(axis=1, keepdims=True)).astype(np.float32), p64, bound, "float64 rounded") <= 0.5
    for left_out in (0, C // 2, C - 1):
        with np.errstate(divide="ignore"):
            got = (e / (e.sum(axis=1, keepdims=True) - e[:, left_out:left_out + 1])).astype(np.float32)
        assert noticed(gr.check_bound, got, p64, bound, "mutant"), "class %d left out of the sum passes at C=%d" % (left_out, C)


def top5_variant(rows, start=gr.FLT_MIN, highest_wins=False):
    out = []
    for row in np.array(rows, np.float32):
        p, picks = row.copy(), []
        for _ in range(5):
            best, bi = np.float32(start), 0
            for c in range(len(p)):
                if best < p[c] or (highest_wins and best == p[c] and best > start):
                    best, bi = p[c], c
            p[bi] = 0.0
            picks.append(bi)
        out.append(picks)
    return np.array(out, np.uint16)


@pytest.mark.parametrize("C", [3, 5, 33, 200])
def test_top5_mutants_fail(C):
    rows = gr.top5_rows(C, seed=300 + C)
    want = gr.top5(rows)
    assert np.array_equal(top5_variant(rows), want)
    assert not np.array_equal(top5_variant(rows, start=0.0), want), "sweeps from 0 pass"
    assert not np.array_equal(top5_variant(rows, highest_wins=True), want), "highest index wins passes"
