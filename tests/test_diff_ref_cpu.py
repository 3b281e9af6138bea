"""CPU tier of the response-error report: the float64 oracle of qcnn_map_diff (tests/diff_ref.py) held to its own identities,
the declarations the C-ABI and the Python binding must agree on, and quantize.response_report's host side — its accumulation over
batches and its agreement counts — on two stub engines: no GPU and no library call."""
import ctypes
import re

import numpy as np
import pytest

import diff_ref as dr
from conftest import pkg

capi = pkg("capi")

# the largest integer case of tests/test_gpu_map_diff.py: (C, H, W) = (3, 37, 41) at 300 images
LARGEST_INT_CASE = (300, 37, 41, 3)


# ---------------------------------------------------------------------------------------------- the oracle
def test_total_is_the_fold_of_the_channels():
    a = dr.integer_map((9, 3, 5, 7), 1)
    b = dr.integer_map((9, 3, 5, 7), 2)
    tot, ch = dr.map_diff(a, b)
    assert ch.shape == (7, 6)
    assert dr.bits_equal(tot, dr.fold(ch))
    d = a.astype(np.float64) - b.astype(np.float64)
    assert tot[0] == a.size and tot[1] == 0
    assert tot[2] == d.sum() and tot[3] == (d * d).sum() and tot[4] == (b.astype(np.float64) ** 2).sum()
    assert tot[5] == np.abs(d).max()
    for c in range(7):
        assert ch[c, 2] == d[..., c].sum() and ch[c, 5] == np.abs(d[..., c]).max()


def test_self_diff_is_zero_with_the_sum_of_squares():
    a = dr.integer_map((5, 2, 3, 4), 3)
    tot, ch = dr.map_diff(a, a)
    assert tot[0] == a.size
    assert tot[1] == tot[2] == tot[3] == tot[5] == 0.0
    assert tot[4] == (a.astype(np.float64) ** 2).sum()
    assert np.array_equal(ch[:, 4], (a.astype(np.float64) ** 2).reshape(-1, 4).sum(axis=0))


def test_integer_maps_do_not_depend_on_the_order():
    rng = np.random.default_rng(4)
    a = dr.integer_map((11, 4, 5, 3), 5)
    b = dr.integer_map((11, 4, 5, 3), 6)
    want = dr.map_diff(a, b)
    pi, pp = rng.permutation(11), rng.permutation(20)
    pa = a.reshape(11, 20, 3)[pi][:, pp].reshape(a.shape)
    pb = b.reshape(11, 20, 3)[pi][:, pp].reshape(b.shape)
    got = dr.map_diff(pa, pb)
    assert dr.bits_equal(got[0], want[0]) and dr.bits_equal(got[1], want[1])
    exact = dr.map_diff(a, b, exact_sums=True)
    assert dr.bits_equal(exact[0], want[0]) and dr.bits_equal(exact[1], want[1])


def test_the_largest_integer_case_stays_below_2_53():
    n, H, W, C = LARGEST_INT_CASE
    terms = n * H * W
    assert terms <= dr.INT_MAX_TERMS
    assert dr.integer_bound(dr.INT_MAX_TERMS) < 2 ** 53
    assert dr.integer_bound(terms) * C < 2 ** 53            # the total as well
    a, b = dr.integer_map(LARGEST_INT_CASE, 7), dr.integer_map(LARGEST_INT_CASE, 8)
    tot, ch = dr.map_diff(a, b)
    assert np.abs(ch[:, 2:5]).max() <= dr.integer_bound(terms) and tot[5] <= 2 * dr.INT_MAX_ABS
    assert np.array_equal(ch, np.round(ch))


def test_nonfinite_rule_by_hand():
    # 2 images x 1 x 1 x 3 channels
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    a = np.array([[[[1.0, nan, 3.0]]], [[[-2.0, 5.0, inf]]]], np.float32)
    b = np.array([[[[4.0, 1.0, -inf]]], [[[-2.0, 7.0, inf]]]], np.float32)
    tot, ch = dr.map_diff(a, b)
    #                 count nonfinite sum_d sum_d2 sum_ref2 max_abs_d
    assert ch.tolist() == [[2.0, 0.0, -3.0, 9.0, 20.0, 3.0],       # d = -3, 0;  b = 4, -2
                           [1.0, 1.0, -2.0, 4.0, 49.0, 2.0],       # (nan, 1) not counted: b = 1 adds nothing;  d = -2, b = 7
                           [0.0, 2.0, 0.0, 0.0, 0.0, 0.0]]         # a only / both: nothing counted, max_abs_d = 0
    assert tot.tolist() == [3.0, 3.0, -5.0, 13.0, 69.0, 3.0]


def test_catchers_need_more_than_fp32():
    for x, y in dr.CATCHERS:
        d64 = float(x) - float(y)
        assert d64 != 0.0 and float(np.float32(d64)) != d64 or abs(d64) < 2.0 ** -126
    a, b = dr.catcher_maps(130)
    tot, ch = dr.map_diff(a, b)
    exact = dr.map_diff(a, b, exact_sums=True)
    assert dr.bits_equal(ch[:, 2], exact[1][:, 2])           # sum_d: exact in any order, channel by channel
    assert ch[:, 0].tolist() == [130 * 20.0] * 3
    assert ch[:, 5].tolist() == [abs(float(x) - float(y)) for x, y in dr.CATCHERS]
    assert ch[2, 5] == 2.0 ** -149


def test_plants_count_per_channel():
    a, b = dr.integer_map((4, 2, 2, 3), 9), dr.integer_map((4, 2, 2, 3), 10)
    pa, pb = dr.plant(a, b, [(0, 0, "a", 0), (3, 4, "b", 1), (2, 11, "both", 2), (1, 3, "a", 1)])
    tot, ch = dr.map_diff(pa, pb)
    assert ch[:, 1].tolist() == [2.0, 1.0, 1.0] and tot[1] == 4.0 and tot[0] == a.size - 4
    keep = np.ones(a.shape, bool).reshape(4, -1)
    for i, e in ((0, 0), (3, 4), (2, 11), (1, 3)):
        keep[i, e] = False
    d = np.where(keep.reshape(a.shape), a.astype(np.float64) - b.astype(np.float64), 0.0)
    assert tot[2] == d.sum() and tot[3] == (d * d).sum()


# ---------------------------------------------------------------------------------------------- declarations
def _header():
    return open(capi.HEADER_PATH).read()


def test_header_declares_the_call():
    txt = _header()
    assert "qcnn_map_diff" in capi.declared_symbols()
    assert re.search(r"typedef\s+struct\s*\{\s*double\s+count,\s*nonfinite,\s*sum_d,\s*sum_d2,\s*sum_ref2,\s*max_abs_d;\s*\}\s*QcnnMapDiff;", txt)
    assert re.search(r"int\s+qcnn_map_diff\(QcnnCtx\*\s*ctx,\s*QcnnCtx\*\s*ref,\s*int\s+l,\s*int\s+n,", txt)
    assert re.search(r"#define\s+QCNN_DIFF_CHUNK_ROWS\s+\d+", txt)
    assert re.search(r"#define\s+QCNN_ABI_VERSION\s+5\b", txt)


def test_struct_and_constant_match_the_header():
    assert ctypes.sizeof(capi.QcnnMapDiff) == 48
    assert [f for f, _ in capi.QcnnMapDiff._fields_] == list(dr.FIELDS)
    assert capi.MAP_DIFF_FIELDS == dr.FIELDS
    m = re.search(r"#define\s+QCNN_DIFF_CHUNK_ROWS\s+(\d+)", _header())
    assert capi.DIFF_CHUNK_ROWS == int(m.group(1))
    assert capi.DIFF_CHUNK_ROWS % 8 == 0


def test_python_entry_points_exist():
    assert callable(pkg("engine").QcnnEngine.map_diff)
    assert callable(pkg("quantize").response_report)
    lib = capi.load()
    assert lib.qcnn_map_diff.argtypes is not None and len(lib.qcnn_map_diff.argtypes) == 6


# ---------------------------------------------------------------------------------------------- response_report on stubs
class StubEngine:
    """What response_report touches of an engine: layers, forward_host and map_diff — the maps are the oracle's."""

    def __init__(self, layers, maps_of, top5_of):
        self.layers, self.L = layers, len(layers)
        self.maps_of, self.top5_of = maps_of, top5_of      # batch -> {l: NHWC map}, batch -> top5
        self.last = None
        self.calls = []

    def forward_host(self, x, want_prob=True, want_top5=True):
        self.last = self.maps_of(x)
        self.calls.append(("forward", len(x)))
        return None, self.top5_of(x)

    def map_diff(self, ref, l, n, per_channel=False):
        self.calls.append(("diff", l, n))
        tot, ch = dr.map_diff(self.last[l][:n], ref.last[l][:n])
        out = pkg("engine").map_diff_summary(dr.as_dict(tot))
        if per_channel:
            out["channels"] = ch
        return out


def _stub_pair():
    topo = pkg("topology")
    layers = [topo.conv(0, 1, 4, 1, 1), topo.relu(), topo.fcnt(5), topo.smax()]
    shapes = {1: (2, 2, 4), 3: (1, 1, 5), 4: (1, 1, 5)}

    def maps(seed):
        def f(x):
            s = int(x[0, 0, 0, 0])
            return {l: dr.integer_map((len(x),) + shp, seed + 10 * l + s) for l, shp in shapes.items()}
        return f

    def ref_top5(x):
        return ((np.arange(len(x))[:, None] + np.arange(5)[None, :]) % 7).astype(np.uint16)

    def eng_top5(x):
        t = ref_top5(x)
        t[1::3] = np.roll(t[1::3], 1, axis=1)      # every third image: another first prediction, the reference's still among the five
        t[3::4] += 100                             # every fourth: nothing in common
        return t

    return StubEngine(layers, maps(100), eng_top5), StubEngine(layers, maps(200), ref_top5), shapes


def _batches():
    out = []
    for k, n in enumerate((2, 5, 7)):
        x = np.zeros((n, 1, 1, 1), np.float32)
        x[:] = k
        out.append(x)
    return out


def test_response_report_accumulates_over_batches():
    q = pkg("quantize")
    eng, ref, shapes = _stub_pair()
    assert q.default_report_maps(eng.layers) == [1, 3, 4]
    report, agree = q.response_report(eng, ref, _batches(), per_channel=False)
    assert sorted(report) == [1, 3, 4]
    # the same sums from the maps themselves, batch by batch
    for l in report:
        want = np.zeros(6)
        for x in _batches():
            tot, _ = dr.map_diff(eng.maps_of(x)[l], ref.maps_of(x)[l])
            want[:5] += tot[:5]
            want[5] = max(want[5], tot[5])
        got = report[l]
        assert [got[f] for f in dr.FIELDS] == want.tolist()
        assert got["rel_err"] == np.sqrt(want[3] / want[4]) and got["mean_d"] == want[2] / want[0]
    # ref first, then the subject, then the maps — batch by batch
    assert ref.calls == [("forward", 2), ("forward", 5), ("forward", 7)]
    assert eng.calls[:4] == [("forward", 2), ("diff", 1, 2), ("diff", 3, 2), ("diff", 4, 2)]
    # agreement, counted from the two top-5 arrays
    n = top1 = in5 = 0
    for x in _batches():
        te, tr = eng.top5_of(x), ref.top5_of(x)
        n += len(x)
        top1 += int((te[:, 0] == tr[:, 0]).sum())
        in5 += sum(int(tr[i, 0] in te[i]) for i in range(len(x)))
    assert agree == dict(n=n, top1_equal=top1, ref_top1_in_top5=in5)
    assert 0 < top1 < in5 < n                                   # the stubs disagree in both ways


def test_response_report_per_channel_and_maps():
    q = pkg("quantize")
    eng, ref, shapes = _stub_pair()
    report, _ = q.response_report(eng, ref, _batches(), maps=[3], per_channel=True)
    assert list(report) == [3]
    ch = report[3]["channels"]
    assert ch.shape == (5, 6)
    assert dr.bits_equal(dr.fold(ch), [report[3][f] for f in dr.FIELDS])
    want = np.zeros((5, 6))
    for x in _batches():
        _, c = dr.map_diff(eng.maps_of(x)[3], ref.maps_of(x)[3])
        want[:, :5] += c[:, :5]
        want[:, 5] = np.maximum(want[:, 5], c[:, 5])
    assert np.array_equal(ch, want)


def test_response_report_self_and_derived_values():
    q = pkg("quantize")
    eng, _, _ = _stub_pair()
    report, agree = q.response_report(eng, eng, _batches())
    for r in report.values():
        assert r["sum_d2"] == 0.0 and r["max_abs_d"] == 0.0 and r["rel_err"] == 0.0 and r["mean_d"] == 0.0
    assert agree["top1_equal"] == agree["ref_top1_in_top5"] == agree["n"] == 14
    s = pkg("engine").map_diff_summary
    zero = dict.fromkeys(dr.FIELDS, 0.0)
    assert s(zero)["rel_err"] == 0.0 and s(zero)["mean_d"] == 0.0
    assert s(dict(zero, sum_d2=1.0))["rel_err"] == float("inf")
    assert s(dict(zero, count=4.0, sum_d=2.0, sum_d2=1.0, sum_ref2=4.0)) == dict(
        count=4.0, nonfinite=0.0, sum_d=2.0, sum_d2=1.0, sum_ref2=4.0, max_abs_d=0.0, rel_err=0.5, mean_d=0.5)


def test_response_report_does_not_skip_a_failing_map():
    q = pkg("quantize")
    eng, ref, _ = _stub_pair()

    class Refused(RuntimeError):
        pass

    def refuse(ref_, l, n, per_channel=False):
        raise Refused("feature map %d was fused away" % l)
    eng.map_diff = refuse
    with pytest.raises(Refused):
        q.response_report(eng, ref, _batches())
