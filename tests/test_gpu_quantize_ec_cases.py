"""The error-correction kernels (qcnn_quantize_layer_ec, qcnn_calib_gram through QcnnEngine) on the crafted cases of
tests/ec_cases.py: one sweep of every case is replayed step by step against the fp64 contract (ec_oracle.replay_sweep, which
tests/test_ec_cases_cpu.py shows to reject every single mistake of ec_oracle.WRONG); the sweep loop of the host driver against
chained single sweeps, bit for bit; the gram kernel on small integers, where every sum is exact and the result has one correct
value to the bit."""
import numpy as np
import pytest

import ec_cases as ec
import ec_oracle as eo
from conftest import pkg

pytestmark = pytest.mark.gpu

engine = pkg("engine")


@pytest.fixture(scope="module")
def eng():
    e = engine.QcnnEngine(0)
    yield e
    e.close()


def run(eng, c, sweeps, ridge, ctrd=None, asmt=None):
    return eng.quantize_layer_ec(c["w"], c["M"], c["K"], c["Cs"], c["G"], c["ctrd"] if ctrd is None else ctrd,
                                 c["asmt"] if asmt is None else asmt, grp=c["grp"], sweeps=sweeps, ridge=ridge)


# ---------------------------------------------------------------- 1. one sweep, every step ----
@pytest.mark.parametrize("ridge", ec.RIDGES)
@pytest.mark.parametrize("name", ec.CASES)
def test_one_sweep_replays_step_by_step(eng, name, ridge):
    c = ec.case(name)
    c1, a1, st = run(eng, c, 1, ridge)
    assert c1.dtype == np.float32 and a1.dtype == np.uint8 and a1.shape == c["asmt"].shape
    assert np.isfinite(c1).all() and np.isfinite(st["obj_trace"]).all()
    r = eo.replay_sweep(c["w"], c["ctrd"], c["asmt"], c["G"], c["grp"], ridge, c1, a1)
    print("%s ridge %g: assign worst / tol %.3g, update worst residual / bound %.3g, smallest gap %.3g tol, clear %d, unclear %d, "
          "changed %d, solved %d, kept %d" % (name, ridge, r["assign"], r["update"], r["gap"], r["clear"], r["unclear"], r["changed"],
                                              r["solved"], r["kept"]))
    assert r["unclear"] == 0, "every decision of these cases is clear on the fp64 state (tests/test_ec_cases_cpu.py)"
    for got, want in ((st["obj_trace"][0], eo.objective(c["w"], c["ctrd"], c["asmt"], c["G"], c["grp"])),
                      (st["obj_trace"][1], eo.objective(c["w"], c1, a1, c["G"], c["grp"]))):
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert st["changed"][0] == r["changed"] == int((a1 != c["asmt"]).sum())
    # what the crafted families say of themselves
    if "dup" in c:
        lo, hi = c["dup"]
        assert (a1[c["dup_ct"], 0] == lo).all() and not (a1[:, 0] == hi).any(), "ties among improvements go to the lowest k"
        assert (a1[c["dup_ct"], 1] == hi).all(), "no move at delta = 0"
    if c.get("fixed_point") or c.get("members"):
        assert st["changed"][0] == 0 and a1.tobytes() == c["asmt"].tobytes()
    if c.get("fixed_point"):
        assert c1[:, 0:16].tobytes() == c["ctrd"][:, 0:16].tobytes() and c1[:, 24:].tobytes() == c["ctrd"][:, 24:].tobytes()
    if c.get("members"):
        moved = (c1 != c["ctrd"]).any(axis=2)
        assert moved[0].tolist() == [k == 5 for k in range(32)] and moved[1].all()
    if "dead_m" in c:
        m, dd = c["dead_m"], c["dead_dims"]
        if ridge == 0.0:
            assert c1[m].tobytes() == c["ctrd"][m].tobytes(), "singular A_k: every word of the sub-space keeps its bits"
            assert c1[1 - m].tobytes() != c["ctrd"][1 - m].tobytes()
        else:
            assert c1[m][:, dd].tobytes() == c["ctrd"][m][:, dd].tobytes(), "v_j = 0 on a dead dim: the solve is exactly 0 there"
            assert name == "dead_subspace" or (c1[m] != c["ctrd"][m]).any()


# ---------------------------------------------------------------- 2. the sweep loop of the driver ----
@pytest.mark.parametrize("name", ["rect_grouped", "fc_k130"])
def test_three_sweeps_equal_three_chained_single_sweeps(eng, name):
    """The driver re-derives E and Hm from the book and the assignments between sweeps, so nothing but those two carries over."""
    c = ec.case(name)
    ridge = 1e-6
    c3, a3, st3 = run(eng, c, 3, ridge)
    cc, aa, obj, chg = c["ctrd"], c["asmt"], [], []
    for _ in range(3):
        cc, aa, st = run(eng, c, 1, ridge, cc, aa)
        obj.append(st["obj_trace"][1])
        chg.append(int(st["changed"][0]))
    print("%s: J %r, changed %r" % (name, st3["obj_trace"], st3["changed"]))
    assert c3.tobytes() == cc.tobytes() and a3.tobytes() == aa.tobytes()
    assert st3["obj_trace"][1:].tobytes() == np.array(obj).tobytes() and st3["changed"].tolist() == chg
    assert chg[0] > 0 and chg[1] > 0, "the second sweep is meant to have work to do"


def test_after_a_sweep_that_changes_nothing_the_trace_repeats(eng):
    c = ec.case("copies_below")
    ridge = ec.RIDGES[1]
    cc, aa, quiet = c["ctrd"], c["asmt"], None
    for i in range(4):                                               # the first sweep may move a word by an ulp; then it is still
        c2, a2, st = run(eng, c, 1, ridge, cc, aa)
        if st["changed"][0] == 0 and c2.tobytes() == cc.tobytes():
            quiet = i
            break
        cc, aa = c2, a2
    assert quiet is not None, "no sweep left the book and the assignments as they were"
    n = quiet + 4
    cn, an, stn = run(eng, c, n, ridge)
    print("first quiet sweep %d; J %r, changed %r" % (quiet, stn["obj_trace"], stn["changed"]))
    assert cn.tobytes() == cc.tobytes() and an.tobytes() == aa.tobytes() == c["asmt"].tobytes()
    assert not stn["changed"].any()
    assert (stn["obj_trace"][quiet + 1:] == stn["obj_trace"][quiet + 1]).all()
    assert stn["obj_trace"][quiet + 1] == st["obj_trace"][1]


# ---------------------------------------------------------------- 3. the gram kernel, exact ----
def geom_dict(g):
    return dict(grp=g[4], kh=g[5], kw=g[6], stride=g[7], pad=g[8])


@pytest.mark.parametrize("name", list(ec.GRAM_EXACT))
def test_gram_of_small_integers_is_exact(eng, name):
    g = ec.GRAM_EXACT[name]
    x = ec.gram_input(name)
    want = eo.gram(x, *g[4:])[0]
    if name in ec.GRAM_SPLITS:                                       # (rows per split, splits) of qk_ec_gram_rows_per_split, restated
        assert ec.gram_split(g, engine.EC_GRAM_RUN) == ec.GRAM_SPLITS[name]
    got = eng.calib_gram(x, geom_dict(g))
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = np.argwhere(got != want)
    assert not len(bad), "%d of %d entries differ, first [g, p, q] = %r: got %r, want %r" % (
        len(bad), want.size, bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    if name in ec.GRAM_ACCUMULATE:
        h = g[0] // 2
        two = eng.calib_gram(x[h:], geom_dict(g), eng.calib_gram(x[:h], geom_dict(g)))
        assert np.array_equal(two, want), "the accumulate path is not exact"


@pytest.mark.parametrize("iy,ix", [(3, 4), (6, 9), (0, 0)])
def test_gram_of_a_one_hot_pixel(eng, iy, ix):
    """One image, 1 on every channel of one pixel: G is the 0/1 matrix ec_cases.one_hot_expected derives from the geometry
    (tests/test_ec_cases_cpu.py holds it against the hand-computed taps)."""
    g = ec.GRAM_EXACT["rect_grouped"]
    x = np.zeros((1,) + g[1:4], np.float32)
    x[0, iy, ix] = 1.0
    want = ec.one_hot_expected(g, iy, ix)
    assert want.any() and set(np.unique(want)) == {0.0, 1.0}
    got = eng.calib_gram(x, geom_dict(g))
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    x[0, iy, ix, 1:] = 0.0                                           # one channel of it: a single diagonal entry per tap
    got = eng.calib_gram(x, geom_dict(g))
    want1 = np.zeros_like(want)
    cg = g[3] // g[4]
    for tap in range(g[5] * g[6]):
        want1[0, tap * cg, tap * cg] = want[0, tap * cg, tap * cg]
    assert np.array_equal(got, want1), np.argwhere(got != want1)[:8].tolist()
