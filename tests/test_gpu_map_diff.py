"""qcnn_map_diff on crafted maps (tests/diff_ref.py: the float64 oracle, pinned by tests/test_diff_ref_cpu.py).

Two engines on device 0 each hold a glue-only one-layer table ([pool 1x1 / 1], as tests/test_gpu_glue.py does): the crafted network
input then IS fm[0] and fm[1], bit for bit, and the real forward path — small `live`, streams, chunked uploads — leaves it in
the panels the kernel reads.

  * integer maps: all six fields, per channel and in total, equal the oracle's BITS — one channel, a channel count that divides
    nothing, more channels than a panel has lanes, a map whose rows per channel end one row past two chunks; every n of N_CASES;
    both maps; a [relu] table at fm[1];
  * lanes of images >= n: whatever a larger forward left there changes nothing; n above either context's last batch is refused;
  * NaN / +Inf / -Inf in a, in b, in both, at lane 0 and at the last live lane of a ragged panel: counted per channel, every
    other field the oracle's bits over the remaining pairs;
  * pairs whose difference needs more than fp32: max_abs_d and sum_d exact;
  * real values: count and max_abs_d exact, the sums inside the reordering bound of an fp64 sum (derived, diff_ref.reorder_bounds),
    the same bits from a second call and from engines with one and two streams, total == fold(channels) to the bit;
  * every refusal names its cause and leaves both contexts usable."""
import ctypes as C

import numpy as np
import pytest

import diff_ref as dr
import glue_ref as gr
from conftest import pkg

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
QcnnError = pkg("engine").QcnnError

N_MAX = 300
N_CASES = (1, 3, 4, 127, 128, 129, 300)
SEAM_HW = 2 * capi.DIFF_CHUNK_ROWS + 1         # one panel: two whole chunks and one row
INT_SHAPES = ((1, 1, 1), (7, 3, 5), (130, 1, 1), (3, 37, 41), (2, 1, SEAM_HW))      # (C, H, W)

_engines = {}
_maps = {}


def make_engine(chw, table, streams=None):
    eng = pkg("engine").QcnnEngine(0)
    eng.set_option(capi.OPT_KEEP_ALL, 1)
    if streams is not None:
        eng.set_option(capi.OPT_STREAMS, streams)
    eng.load_model(chw, table, {}, N_MAX)
    return eng


def pair(chw, kind="pool", streams=None):
    """(subject, reference): two engines with the same one-layer table, made once per module."""
    key = (tuple(chw), kind, streams)
    if key not in _engines:
        table = [topo.pool(0, 1, 1)] if kind == "pool" else [topo.relu()]
        _engines[key] = (make_engine(chw, table, streams), make_engine(chw, table, streams))
    return _engines[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for a, b in _engines.values():
        a.close()
        b.close()
    _engines.clear()
    _maps.clear()


def int_maps(chw):
    """Two integer maps [300][H][W][C] of a shape, made once."""
    if chw not in _maps:
        c, h, w = chw
        _maps[chw] = (dr.integer_map((N_MAX, h, w, c), 11 + c), dr.integer_map((N_MAX, h, w, c), 1011 + c))
    return _maps[chw]


def forward(eng, x):
    eng.forward_host(gr.nchw(x), want_prob=False, want_top5=False)


def rows_of(r):
    return np.array([r[f] for f in dr.FIELDS], np.float64)


def check_bits(eng, ref, l, n, a, b, what):
    """map_diff(l, n) of the two engines returns the oracle's bits on the first n images of a and b."""
    want_tot, want_ch = dr.map_diff(a[:n], b[:n])
    got = eng.map_diff(ref, l, n, per_channel=True)
    for c in range(len(want_ch)):
        assert dr.bits_equal(got["channels"][c], want_ch[c]), "%s: channel %d: got %r, want %r (%s)" % (
            what, c, got["channels"][c].tolist(), want_ch[c].tolist(), ", ".join(dr.FIELDS))
    assert dr.bits_equal(rows_of(got), want_tot), "%s: total: got %r, want %r" % (what, rows_of(got).tolist(), want_tot.tolist())
    plain = eng.map_diff(ref, l, n)
    assert "channels" not in plain and dr.bits_equal(rows_of(plain), want_tot), "%s: the call without channels differs" % what
    return got


# ---------------------------------------------------------------------------------------------- 1. integer maps
@pytest.mark.parametrize("n", N_CASES)
@pytest.mark.parametrize("chw", INT_SHAPES, ids=lambda s: "c%d_h%d_w%d" % s)
def test_integer_maps_bit_exact(chw, n):
    eng, ref = pair(chw)
    a, b = int_maps(chw)
    forward(ref, b[:n])
    forward(eng, a[:n])
    for l in (0, 1):
        got = check_bits(eng, ref, l, n, a, b, "%r n=%d l=%d" % (chw, n, l))
        assert got["count"] == n * a[0].size and got["nonfinite"] == 0
        assert got["rel_err"] == np.sqrt(got["sum_d2"] / got["sum_ref2"]) and got["mean_d"] == got["sum_d"] / got["count"]
    if n > 1:                                       # fewer images than the forward ran: a prefix of the same maps
        check_bits(eng, ref, 1, n - 1, a, b, "%r n=%d of a forward of %d" % (chw, n - 1, n))
    # the subject against itself: zeros, and the sum of its squares
    me = eng.map_diff(eng, 1, n)
    sq = (a[:n].astype(np.float64) ** 2).sum()
    assert rows_of(me).tolist() == [n * a[0].size, 0.0, 0.0, 0.0, sq, 0.0]


@pytest.mark.parametrize("n", (3, 129, 300))
def test_integer_maps_behind_a_relu(n):
    chw = (7, 3, 5)
    eng, ref = pair(chw, "relu")
    a, b = int_maps(chw)
    forward(ref, b[:n])
    forward(eng, a[:n])
    zero = np.float32(0)
    check_bits(eng, ref, 1, n, np.where(a > 0, a, zero), np.where(b > 0, b, zero), "relu n=%d" % n)
    check_bits(eng, ref, 0, n, a, b, "relu input n=%d" % n)


# ---------------------------------------------------------------------------------------------- 2. stale lanes
def test_stale_lanes_contribute_nothing():
    chw = (7, 3, 5)
    eng, ref = pair(chw)
    rng = np.random.default_rng(21)
    junk_a = rng.choice(np.float32([-64, 64]), (N_MAX, 3, 5, 7))
    junk_b = rng.choice(np.float32([-64, 64]), (N_MAX, 3, 5, 7))
    a, b = int_maps(chw)
    forward(ref, junk_b)
    forward(eng, junk_a)
    forward(ref, b[:129])
    forward(eng, a[:129])
    for l in (0, 1):
        check_bits(eng, ref, l, 129, a, b, "129 images over 300 of junk, l=%d" % l)
    # the reference still holds 300 images, the subject 129
    forward(ref, junk_b)
    forward(eng, a[100:229])
    for l in (0, 1):
        check_bits(eng, ref, l, 129, a[100:229], junk_b, "subject 129, reference 300, l=%d" % l)
    with pytest.raises(QcnnError, match="exceeds the last forward's batch 129"):
        eng.map_diff(ref, 1, 130)
    with pytest.raises(QcnnError, match="reference context's last forward's batch 129"):
        ref.map_diff(eng, 1, 130)
    check_bits(ref, eng, 1, 129, junk_b, a[100:229], "the other way round after the refusal")


# ---------------------------------------------------------------------------------------------- 3. non-finite plants
def test_nonfinite_plants():
    chw = (7, 3, 5)
    E = 7 * 3 * 5
    eng, ref = pair(chw)
    a, b = int_maps(chw)
    # 300 images: lane 0 of panels 0, 1 and 2, the last lane of a whole panel, the last live lane of the ragged one
    spots = [(0, 0, "a", 0), (0, 8, "b", 1), (0, E - 1, "both", 2), (127, 3, "a", 1), (128, 3, "b", 2), (128, 10, "both", 0),
             (200, 20, "a", 1), (200, 21, "b", 2), (129, 0, "both", 0), (256, 50, "a", 2), (299, 0, "b", 0), (299, 52, "a", 1), (299, E - 1, "both", 1), (298, 7, "a", 0)]
    pa, pb = dr.plant(a, b, spots)
    forward(ref, pb)
    forward(eng, pa)
    for l in (0, 1):
        got = check_bits(eng, ref, l, N_MAX, pa, pb, "plants, 300 images, l=%d" % l)
        assert got["nonfinite"] == len(spots)
        per = np.zeros(7)
        for _, e, _, _ in spots:
            per[e % 7] += 1
        assert got["channels"][:, 1].tolist() == per.tolist()
    # 129 images over those 300: image 128 is the only and last live lane of the ragged panel; the plants of images 256 .. 299
    # and 129 .. 255 lie in dead lanes and dead panels
    spots129 = [(0, 1, "a", 0), (128, 0, "b", 1), (128, E - 1, "a", 2), (128, 9, "both", 0), (64, 33, "b", 2)]
    qa, qb = dr.plant(a[:129], b[:129], spots129)
    forward(ref, qb)
    forward(eng, qa)
    for l in (0, 1):
        got = check_bits(eng, ref, l, 129, qa, qb, "plants, 129 images over 300, l=%d" % l)
        assert got["nonfinite"] == len(spots129)
        check_bits(eng, ref, l, 128, qa, qb, "plants, the first panel alone, l=%d" % l)


# ---------------------------------------------------------------------------------------------- 4. the catchers
@pytest.mark.parametrize("n", (3, 130))
def test_differences_beyond_fp32(n):
    eng, ref = pair((3, 4, 5))
    a, b = dr.catcher_maps(n)
    forward(ref, b)
    forward(eng, a)
    _, want_ch = dr.map_diff(a, b, exact_sums=True)
    for l in (0, 1):
        got = eng.map_diff(ref, l, n, per_channel=True)
        ch = got["channels"]
        assert ch[:, 0].tolist() == [n * 20.0] * 3 and ch[:, 1].tolist() == [0.0] * 3
        assert dr.bits_equal(ch[:, 5], want_ch[:, 5]), "max_abs_d %r, want %r" % (ch[:, 5].tolist(), want_ch[:, 5].tolist())
        assert dr.bits_equal(ch[:, 2], want_ch[:, 2]), "sum_d %r, want %r" % (ch[:, 2].tolist(), want_ch[:, 2].tolist())
        assert ch[2, 5] == 2.0 ** -149
        assert dr.bits_equal(rows_of(got), dr.fold(ch))


# ---------------------------------------------------------------------------------------------- 5. real values
def test_real_values_within_the_reordering_bound():
    chw = (7, 9, 11)
    shape = (N_MAX, 9, 11, 7)
    a = gr.signed_log_uniform(shape, seed=501)
    b = gr.signed_log_uniform(shape, seed=502)
    want_tot, want_ch = dr.map_diff(a, b, exact_sums=True)
    N_ch, absd_ch = dr.reorder_bounds(a, b)
    results = []
    for streams in (1, 2):
        eng, ref = pair(chw, streams=streams)
        forward(ref, b)
        forward(eng, a)
        for l in (0, 1):
            got = eng.map_diff(ref, l, N_MAX, per_channel=True)
            again = eng.map_diff(ref, l, N_MAX, per_channel=True)
            assert dr.bits_equal(got["channels"], again["channels"]) and dr.bits_equal(rows_of(got), rows_of(again))
            results.append(got)
    first = results[0]
    for r in results[1:]:
        assert dr.bits_equal(r["channels"], first["channels"]) and dr.bits_equal(rows_of(r), rows_of(first))
    ch = first["channels"]
    assert dr.bits_equal(rows_of(first), dr.fold(ch))
    assert np.array_equal(ch[:, 0], want_ch[:, 0]) and np.array_equal(ch[:, 1], want_ch[:, 1])
    assert dr.bits_equal(ch[:, 5], want_ch[:, 5]) and first["max_abs_d"] == want_tot[5]
    u = 2.0 ** -52
    worst = 0.0
    for rows, want, N, absd in [(ch, want_ch, N_ch, absd_ch),
                                (rows_of(first)[None], want_tot[None], np.array([N_ch.sum()]), np.array([absd_ch.sum()]))]:
        for j, bound in ((2, N * u * absd), (3, N * u * want[:, 3]), (4, N * u * want[:, 4])):
            err = np.abs(rows[:, j] - want[:, j])
            worst = max(worst, float((err / bound).max()))
            print("map_diff %s over %d rows: worst err / bound %.3g" % (dr.FIELDS[j], len(rows), float((err / bound).max())))
            assert (err <= bound).all(), "%s: err %r beyond %r" % (dr.FIELDS[j], err.tolist(), bound.tolist())
    assert worst < 1.0


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_name_their_cause():
    chw = (7, 3, 5)
    lib = capi.load()
    a, b = int_maps(chw)
    fresh_a, fresh_b = make_engine(chw, [topo.pool(0, 1, 1)]), make_engine(chw, [topo.pool(0, 1, 1)])
    other = make_engine((5, 3, 5), [topo.pool(0, 1, 1)])
    deeper = make_engine(chw, [topo.pool(0, 1, 1), topo.relu()])
    try:
        # no forward yet, on either side
        with pytest.raises(QcnnError, match="feature map 1 is not available"):
            fresh_a.map_diff(fresh_b, 1, 1)
        forward(fresh_a, a[:5])
        with pytest.raises(QcnnError, match="reference context: feature map 1 is not available"):
            fresh_a.map_diff(fresh_b, 1, 1)
        forward(fresh_b, b[:7])
        forward(other, np.zeros((5, 3, 5, 5), np.float32))
        forward(deeper, b[:7])
        tot = capi.QcnnMapDiff()
        assert lib.qcnn_map_diff(None, fresh_b.h, 1, 1, C.byref(tot), None) != 0
        assert b"ctx == NULL" in lib.qcnn_last_error(None)
        with pytest.raises(QcnnError, match="ref == NULL"):
            fresh_a.map_diff(None, 1, 1)
        assert lib.qcnn_map_diff(fresh_a.h, fresh_b.h, 1, 1, None, None) != 0
        assert b"total_host == NULL" in lib.qcnn_last_error(fresh_a.h)
        for l in (-1, 2):
            with pytest.raises(QcnnError, match="feature map %d out of range" % l):
                fresh_a.map_diff(fresh_b, l, 1)
        with pytest.raises(QcnnError, match="out of range of the reference context"):
            deeper.map_diff(fresh_b, 2, 1)
        with pytest.raises(QcnnError, match="different dims in the two contexts: 3 x 5 x 7 against 3 x 5 x 5"):
            fresh_a.map_diff(other, 1, 1)
        for n in (0, -3):
            with pytest.raises(QcnnError, match="n = %d: at least one image" % n):
                fresh_a.map_diff(fresh_b, 1, n)
        with pytest.raises(QcnnError, match="n = 6 exceeds the last forward's batch 5"):
            fresh_a.map_diff(fresh_b, 1, 6)
        with pytest.raises(QcnnError, match="n = 6 exceeds the reference context's last forward's batch 5"):
            fresh_b.map_diff(fresh_a, 1, 6)
        cnt = C.c_int(0)
        assert lib.qcnn_device_count(C.byref(cnt)) == 0
        if cnt.value > 1:
            far = pkg("engine").QcnnEngine(1)
            try:
                with pytest.raises(QcnnError, match="different devices"):
                    fresh_a.map_diff(far, 1, 1)
            finally:
                far.close()
        # both contexts are as usable as before; another model on the other side is fine while the map's dims agree
        check_bits(fresh_a, fresh_b, 1, 5, a, b, "after the refusals")
        check_bits(fresh_a, deeper, 1, 5, a, b, "against a two-layer table")
    finally:
        for e in (fresh_a, fresh_b, other, deeper):
            e.close()
