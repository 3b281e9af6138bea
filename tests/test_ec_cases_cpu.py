"""CPU tier of the crafted error-correction cases (tests/ec_cases.py): ec_oracle.replay_sweep accepts the oracle's own sweep on
every case and rejects every single mistake of ec_oracle.WRONG on the case named here, so a kernel that made that mistake would
fail tests/test_gpu_quantize_ec_cases.py, which replays the same cases; the cases are what they say they are; and the exact-sum
gram geometries agree with a brute-force patch loop."""
import functools

import numpy as np
import pytest

import ec_cases as ec
import ec_oracle as eo
from test_ec_oracle_cpu import brute_gram

# mutation: (case, ridge) on which replay_sweep has to reject it
REJECTED_BY = dict(taps_reversed=("rect_grouped", 1e-6),
                   no_follow_between_taps=("conv3x3", 1e-6),
                   assign_le=("dup_69_200", 1e-6),
                   move_on_zero=("copies_below", 1e-6),
                   second_best=("rgb_like", 1e-6),
                   wave_low_only=("fc_k130", 1e-6),
                   group0_gram=("rect_grouped", 0.0),
                   update_one_shot=("conv3x3", 0.0),
                   update_stale_E=("k256_cs16", 1e-6),
                   empty_zero=("k256_cs16", 0.0),
                   nonpd_zero=("dead_dim", 0.0),
                   cseff_full=("rgb_like", 0.0),
                   members_last_dropped=("members_all_or_one", 1e-6))
ALSO_REJECTED_BY = dict(assign_le=[("dup_3_7", 0.0), ("dup_5_69", 0.0)], nonpd_zero=[("dead_subspace", 0.0)],
                        wave_low_only=[("k256_cs16", 0.0), ("dup_69_200", 0.0)], group0_gram=[("fc_k130", 1e-6)],
                        update_stale_E=[("fc_k130", 0.0)], cseff_full=[("rect_grouped", 1e-6), ("k256_cs16", 1e-6)])


@functools.lru_cache(maxsize=None)
def swept(name, ridge, wrong=()):
    """(book, assignments, changed) after one sweep of the oracle, with the mistakes ``wrong``."""
    c = ec.case(name)
    st = eo.State(c["w"], c["ctrd"], c["asmt"], c["G"], c["grp"], ridge)
    changed, _ = eo.sweep(st, wrong)
    return st.C, st.A, changed


def replay(name, ridge, wrong=()):
    c = ec.case(name)
    C1, A1, _ = swept(name, ridge, wrong)
    return eo.replay_sweep(c["w"], c["ctrd"], c["asmt"], c["G"], c["grp"], ridge, C1, A1)


@pytest.mark.parametrize("name", ec.CASES)
def test_replay_accepts_the_oracles_own_sweep(name):
    c = ec.case(name)
    assert ec.shape_rules_ok(c), "the case breaks a shape rule of qcnn_quantize_layer_ec"
    for ridge in ec.RIDGES:
        r = replay(name, ridge)
        print("%s ridge %g: %r" % (name, ridge, r))
        assert r["changed"] == swept(name, ridge)[2] and r["assign"] <= 1.0 and r["update"] <= 1.0
        assert r["solved"] > 0 and r["solved"] + r["kept"] == c["M"] * c["K"]
        assert r["unclear"] == 0, "the crafted cases leave nothing to the tolerance rule either"


@pytest.mark.parametrize("name", list(ec.RANDOM))
def test_random_family_reaches_its_paths_and_every_decision_is_clear(name):
    """The cap on what the replay may leave to the tolerance rule is none: a seed that breaks it is replaced, never the cap."""
    c = ec.case(name)
    ct, cin, kh, kw = eo.dims(c["w"])
    for ridge in ec.RIDGES:
        r = replay(name, ridge)
        print("%s ridge %g: smallest gap %.3g tolerances, %d clear, %d unclear" % (name, ridge, r["gap"], r["clear"], r["unclear"]))
        assert r["unclear"] == 0 and r["clear"] == ct * kh * kw * c["M"] and r["changed"] > r["clear"] // 2
    A1 = swept(name, 1e-6)[1]
    if name == "rect_grouped":
        assert kh != kw and c["x"].shape[1] != c["x"].shape[2] and c["grp"] == 2 and cin - c["Cs"] == 2
    if name == "k256_cs16":
        assert c["K"] == 256 and c["Cs"] == 16 and cin - 16 == 4 and ct // c["grp"] > 64
        assert all(len(np.unique(A1[:, :, m])) <= 224 for m in range(2)), "many code words are meant to be without members"
        assert (A1[:, :, 0] == 255).any() or (A1[:, :, 1] == 255).any(), "the last code word needs members: its list ends at off[K]"
    if name == "fc_k130":
        assert kh * kw == 1 and c["K"] > 128 and ct // c["grp"] == 65 and (A1 >= 128).any() and ((A1 >= 64) & (A1 < 128)).any()
    if name == "rgb_like":
        assert cin == 3 and c["M"] == 1


@pytest.mark.parametrize("name", list(ec.DUP_PAIRS))
def test_duplicated_word_is_the_strict_best_and_the_lowest_index_wins(name):
    c = ec.case(name)
    lo, hi = c["dup"]
    assert c["ctrd"][:, lo].tobytes() == c["ctrd"][:, hi].tobytes()
    assert not np.isin(c["asmt"][:, 0], (lo, hi)).any() and (c["asmt"][c["dup_ct"], 1] == hi).all()
    st = eo.State(c["w"], c["ctrd"], c["asmt"], c["G"], 1, 0.0)
    dl = eo.deltas(st, 0, 0)[c["dup_ct"]]
    assert (dl[:, lo] == dl[:, hi]).all() and (dl[:, lo] < 0).all()
    rest = np.delete(dl, [lo, hi], axis=1)
    assert (rest.min(axis=1) > dl[:, lo]).all(), "the duplicated word is not the strict best"
    for ridge in ec.RIDGES:
        A1 = swept(name, ridge)[1]
        assert (A1[c["dup_ct"], 0, 0] == lo).all() and not (A1[:, 0, 0] == hi).any()
        assert (A1[c["dup_ct"], 0, 1] == hi).all(), "a copy at a lower index prices delta = 0: no move"


def test_copies_below_is_a_fixed_point_with_a_zero_delta_at_a_lower_k():
    c = ec.case("copies_below")
    a0 = c["asmt"].reshape(-1, 4, c["M"])
    assert a0.min() >= 16 and c["ctrd"][:, 0:8].tobytes() == c["ctrd"][:, 16:24].tobytes()
    st = eo.State(c["w"], c["ctrd"], c["asmt"], c["G"], 1, 1e-6)
    for m in range(c["M"]):
        for t in range(4):
            dl = eo.deltas(st, m, t)
            rows = np.arange(len(dl))
            assert (dl[rows, a0[:, t, m] - 16] == 0.0).all() and (dl.min(axis=1) == 0.0).all()
    for ridge in ec.RIDGES:
        C1, A1, changed = swept("copies_below", ridge)
        assert changed == 0 and np.array_equal(A1, a0)
        assert C1[:, 0:16].tobytes() == c["ctrd"][:, 0:16].tobytes() and C1[:, 24:].tobytes() == c["ctrd"][:, 24:].tobytes()
    assert swept("copies_below", 1e-6)[0].tobytes() == c["ctrd"].tobytes()                 # built as a fixed point of this ridge


@pytest.mark.parametrize("name", ["dead_subspace", "dead_dim"])
def test_dead_channels_leave_singular_normal_equations(name):
    c = ec.case(name)
    m, dd, Cs = c["dead_m"], c["dead_dims"], c["Cs"]
    cin = eo.dims(c["w"])[1]
    dead_p = [t * cin + m * Cs + j for t in range(4) for j in dd]
    assert not c["G"][0][dead_p].any() and not c["G"][0][:, dead_p].any() and c["G"][0].any()
    C0, A0, _ = swept(name, 0.0)
    assert C0[m].tobytes() == c["ctrd"][m].tobytes() and C0[1 - m].tobytes() != c["ctrd"][1 - m].tobytes()
    assert np.isfinite(C0).all() and np.isfinite(eo.objective(c["w"], C0, A0, c["G"]))
    C1, A1, _ = swept(name, 1e-6)
    assert C1[m][:, dd].tobytes() == c["ctrd"][m][:, dd].tobytes()
    if name == "dead_dim":
        assert (C1[m] != c["ctrd"][m]).any(), "the live dims are meant to move under a ridge"
    assert np.isfinite(C1).all() and np.isfinite(eo.objective(c["w"], C1, A1, c["G"]))


def test_members_case_keeps_its_member_lists_through_the_assign_phase():
    c = ec.case("members_all_or_one")
    a0 = c["asmt"].reshape(-1, 4, 2)
    assert (a0[:, :, 0] == 5).all() and sorted(a0[:, :, 1].reshape(-1)) == list(range(32))
    for ridge in ec.RIDGES:
        C1, A1, changed = swept("members_all_or_one", ridge)
        assert changed == 0 and np.array_equal(A1, a0)
        moved = (C1 != c["ctrd"]).any(axis=2)
        assert moved[0].tolist() == [k == 5 for k in range(32)] and moved[1].all()


@pytest.mark.parametrize("wrong", eo.WRONG)
def test_every_mistake_is_rejected_by_the_replay(wrong):
    for name, ridge in [REJECTED_BY[wrong]] + ALSO_REJECTED_BY.get(wrong, []):
        C1, A1, _ = swept(name, ridge, (wrong,))
        good = swept(name, ridge)
        assert C1.tobytes() != good[0].tobytes() or not np.array_equal(A1, good[1]), "%s changes nothing on %s" % (wrong, name)
        with pytest.raises(eo.ReplayError) as e:
            replay(name, ridge, (wrong,))
        print("%s on %s (ridge %g): rejected at %r" % (wrong, name, ridge, e.value))


def test_every_mistake_has_a_case():
    assert sorted(REJECTED_BY) == sorted(eo.WRONG)
    assert all(n in ec.CASES and r in ec.RIDGES for n, r in list(REJECTED_BY.values()) + sum(ALSO_REJECTED_BY.values(), []))


def test_replay_rejects_a_single_flipped_assignment_and_a_single_moved_word():
    c = ec.case("conv3x3")
    C1, A1, _ = swept("conv3x3", 1e-6)
    args = (c["w"], c["ctrd"], c["asmt"], c["G"], 1, 1e-6)
    A2 = A1.copy()
    A2[7, 4, 1] = (A2[7, 4, 1] + 1) % c["K"]
    with pytest.raises(eo.ReplayError) as e:
        eo.replay_sweep(*args, C1, A2)
    assert e.value.where == (1, 4, 7)
    C2 = C1.copy()
    C2[1, 9] *= np.float32(1.0 + 2.0 ** -18)                        # 64 ulps: the residual bound allows about Cs of them
    with pytest.raises(eo.ReplayError) as e:
        eo.replay_sweep(*args, C2, A1)
    assert e.value.where == (1, 9)


@pytest.mark.parametrize("name", list(ec.GRAM_EXACT))
def test_gram_geometries_are_exact_and_agree_with_a_brute_force_patch_loop(name):
    geom = ec.GRAM_EXACT[name]
    n, H, W, C, grp, kh, kw, stride, pad = geom
    assert C % grp == 0 and H + 2 * pad >= kh and W + 2 * pad >= kw
    x = ec.gram_input(name)
    assert set(np.unique(x)) <= {0.0, 1.0, 2.0, 3.0} and 0.35 < (x == 0).mean() < 0.65
    got = eo.gram(x, grp, kh, kw, stride, pad)[0]
    assert np.array_equal(got, np.rint(got)) and got.max() <= 9.0 * ec.gram_rows(geom) < 2.0 ** 24
    if ec.gram_rows(geom) * (kh * kw * C // grp) ** 2 * grp <= 2e8:         # the brute loop is for the small ones
        assert np.array_equal(got, brute_gram(x.astype(np.float64), grp, kh, kw, stride, pad))
    if name in ec.GRAM_SPLITS:
        import re, os
        from conftest import ROOT
        run = int(re.search(r"#define\s+QCNN_EC_GRAM_RUN\s+(\d+)", open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_kernels.h")).read()).group(1))
        assert ec.gram_split(geom, run) == ec.GRAM_SPLITS[name]
        per, splits = ec.GRAM_SPLITS[name]
        assert (ec.gram_rows(geom) - (splits - 1) * per) % ec.GRAM_CHUNK != 0 or name == "rows264_two_splits"


def test_gram_geometry_table_reaches_what_it_names():
    rows = {k: ec.gram_rows(g) for k, g in ec.GRAM_EXACT.items()}
    assert rows["rows5_p65"] == 5 and rows["rows153"] == 153 and rows["rows264_two_splits"] == 264 and rows["rows300_one_split"] == 300
    assert rows["rows8463_17_splits"] == 8463 and rows["p630_pad2"] == 25
    for k in ("rect_grouped", "rect_1x3", "rect_4x1_stride3"):
        n, H, W, C, grp, kh, kw, stride, pad = ec.GRAM_EXACT[k]
        assert H != W and kh != kw
    assert sum(eo.out_size(g[1], g[5], g[7], g[8]) != eo.out_size(g[2], g[6], g[7], g[8]) for g in ec.GRAM_EXACT.values()) >= 3


def test_one_hot_expectation_is_the_hand_computed_one():
    """(7, 10) map, 3 x 2 window, stride 2, pad 1, Cg = 3.  Pixel (3, 4): rows y = 4 - 2 oy in {0, 2} (oy = 2, 1), column
    x = 5 - 2 ox = 1 (ox = 2): taps 1 and 5, seen by different output pixels.  Corner pixel (6, 9): y = 7 - 2 oy = 1 (oy = 3),
    x = 10 - 2 ox = 0 (ox = 5): tap 2."""
    geom = ec.GRAM_EXACT["rect_grouped"]
    for (iy, ix), taps in (((3, 4), (1, 5)), ((6, 9), (2,))):
        want = np.zeros((2, 18, 18))
        for tap in taps:
            want[:, 3 * tap:3 * tap + 3, 3 * tap:3 * tap + 3] = 1.0
        assert np.array_equal(ec.one_hot_expected(geom, iy, ix), want)
        x = np.zeros((1, 7, 10, 6), np.float32)
        x[0, iy, ix] = 1.0
        assert np.array_equal(eo.gram(x, 2, 3, 2, 2, 1)[0], want)
