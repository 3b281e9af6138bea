"""CPU tier of the crafted quantiser cases (tests/pq_cases.py): the numpy oracle (tests/pq_oracle.py) equals the scalar
restatement of the contract on every case; every family is shown to be potent on the scalar reference alone (ties exist, the
tied seed candidates sit where each level of the block argmax decides, the member sums depend on the order, ...); and every
wrong variant of the scalar reference changes the bytes of at least one case of its family, so a kernel that made that mistake
would fail tests/test_gpu_quantize_cases.py, which runs the same cases against the same oracle."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import pq_cases as pc
import pq_oracle

FAMILY_OF = dict(assign_le="ties_assign",
                 seed_highest="ties_seed", seed_lane_last="ties_seed", seed_wave_highest="ties_seed", seed_block_highest="ties_seed",
                 sum_reversed="sum_order", sum_pairwise="sum_order", sum_interleave4="sum_order", sum_fp32="sum_order",
                 div_float="sum_order", tail_dropped="sum_order",
                 empty_zero="empty_words", pad_keep="empty_words",
                 dist_ftz="range")


@functools.lru_cache(maxsize=None)
def cases(family):
    return pc.FAMILIES[family]()


@functools.lru_cache(maxsize=None)
def ref(family, name):
    """(result, trace) of the scalar reference, computed once per case."""
    trace = {}
    w, M, K, Cs, init, it = cases(family)[name]
    return pc.quantize_layer(w, M, K, Cs, ctrd_init=init, max_iter=it, trace=trace), trace


@functools.lru_cache(maxsize=None)
def oracle(family, name):
    w, M, K, Cs, init, it = cases(family)[name]
    with np.errstate(all="ignore"):
        return pq_oracle.quantize_layer(w, M, K, Cs, ctrd_init=init, max_iter=it)


def same_bytes(got, want):
    return (got[0].tobytes() == want[0].tobytes() and got[1].shape == want[1].shape and got[1].tobytes() == want[1].tobytes()
            and (got[2]["iters"], got[2]["unconverged"]) == (want[2]["iters"], want[2]["unconverged"]))


# ------------------------------------------------------------------------------ the oracle is the contract on every case
@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_oracle_equals_the_scalar_reference(family):
    assert cases(family)
    for name, (w, M, K, Cs, init, it) in cases(family).items():
        got, want = oracle(family, name), ref(family, name)[0]
        what = "%s/%s: %s" % (family, name, pc.describe_diff(got, want, M, K, Cs))
        assert got[0].dtype == want[0].dtype == np.float32 and got[1].dtype == want[1].dtype == np.uint8, what
        assert same_bytes(got, want), what
        for key in ("sse_init", "sse"):
            assert abs(got[2][key] - want[2][key]) <= 1e-9 * max(abs(want[2][key]), 1e-30), what
        assert np.isfinite(got[0]).all() and np.isfinite([got[2]["sse_init"], got[2]["sse"]]).all(), what
        N = want[1].size // M
        assert N <= 8195 and M <= 4 and K <= 256, what


def test_block_argmax_without_a_switch_is_the_first_maximum():
    rng = np.random.default_rng(1)
    for N in (1, 5, 64, 255, 256, 257, 700, 1100):
        d = [np.float32(v) for v in rng.integers(0, 4, N)]
        assert pc.argmax_block(d) == int(np.argmax(np.array(d)))
        assert pc.argmax_block(d, lane_last=True, wave_highest=True, block_highest=True) == N - 1 - int(np.argmax(np.array(d)[::-1]))


# ------------------------------------------------------------------------------ potency, on the scalar reference alone
def test_ties_assign_has_exact_ties_in_every_subspace():
    total = 0
    for name, (w, M, K, Cs, init, it) in cases("ties_assign").items():
        trace = ref("ties_assign", name)[1]
        for m in range(M):
            assert trace["ties"][m][0] > 0, "%s sub-space %d: no point with two nearest code words" % (name, m)
            total += trace["ties"][m][0]
        print("ties_assign/%s: tied points per sub-space in the first assign %r" % (name, [trace["ties"][m][0] for m in range(M)]))
    assert any(M > 1 and w.shape[1] % Cs for (w, M, K, Cs, init, it) in cases("ties_assign").values())
    assert {it for (*_, it) in cases("ties_assign").values()} >= {0, 2}
    print("ties_assign: %d cases, %d tied points" % (len(cases("ties_assign")), total))


def seed_pairings(trace, m):
    """Per round of sub-space m the set of levels at which a tie between the picked point and a different point is
    decided: 'lane' (n and n + 256 j), 'wave' (two lanes of a wave), 'block' (two waves)."""
    out = []
    pts = trace["pts"][m]
    for maxima, pick in trace["rounds"][m]:
        assert pick == maxima[0]
        kinds = set()
        for n in maxima[1:]:
            if pts[n] == pts[pick]:
                continue
            la, lb = pick % pc.SEED_BLOCK, n % pc.SEED_BLOCK
            kinds.add("lane" if la == lb else "wave" if la // pc.WAVE == lb // pc.WAVE else "block")
        out.append(kinds)
    return out


def test_ties_seed_every_pairing_decides_a_round_on_its_own():
    sole = dict(lane=0, wave=0, block=0)
    rounds = 0
    for name, (w, M, K, Cs, init, it) in cases("ties_seed").items():
        assert init is None
        trace = ref("ties_seed", name)[1]
        for m in range(M):
            assert len(trace["rounds"][m]) == K - 1
            for maxima, _ in trace["rounds"][m]:
                assert len(maxima) >= 2, "%s sub-space %d: a round with a single farthest point" % (name, m)
            for kinds in seed_pairings(trace, m):
                rounds += 1
                if len(kinds) == 1:
                    sole[next(iter(kinds))] += 1
    print("ties_seed: %d cases, %d rounds, rounds decided by one level alone: %r" % (len(cases("ties_seed")), rounds, sole))
    assert min(sole.values()) >= 2, sole
    # the all-identical set picks n = 0 in every round; N < K is there
    assert all(pick == 0 for pick in (p for _, p in ref("ties_seed", "identical")[1]["rounds"][0]))
    assert any(np.asarray(w).shape[0] < K for (w, M, K, *_) in cases("ties_seed").values())


def test_sum_order_members_sum_differently_in_another_order():
    seen = set()
    for name, (w, M, K, Cs, init, it) in cases("sum_order").items():
        assert init is not None and it == 1
        N = np.asarray(w).shape[0]
        seen.add((N > pc.CHUNK, N % pc.CHUNK % 4 != 0))
        inexact = 0
        for m, sums in ref("sum_order", name)[1]["sums"].items():
            for step, k, j, vals, s in sums:
                inexact += sum(Fraction(v) for v in vals) != Fraction(s)
        assert (inexact > 0) == (name not in pc.SUM_ORDER_EXACT), name
        print("sum_order/%s: %d member sums differ from the exact rational sum" % (name, inexact))
    assert (True, True) in seen and (False, True) in seen


def test_range_small_scale_is_subnormal_and_still_tells_code_words_apart():
    for name, (w, M, K, Cs, init, it) in cases("range").items():
        (ctrd, asmt, st), trace = ref("range", name)
        dmax = max(trace["dmax"].values())
        if name.startswith("subnormal"):
            assert dmax < pc.FLT_MIN, (name, dmax)
            sub = sum(0.0 < d < pc.FLT_MIN for m in range(M) for d in trace["dm"][m])
            assert sub > 0 and len(np.unique(asmt)) > 1, (name, sub)
            assert np.unique(asmt.reshape(-1, M), axis=0).shape[0] > K, name
            print("range/%s: largest distance %g, %d non-zero subnormal minimum distances" % (name, dmax, sub))
        else:
            assert pc.FLT_MAX / 16.0 <= dmax <= pc.FLT_MAX, (name, dmax)
            print("range/%s: largest distance FLT_MAX / %.3g" % (name, pc.FLT_MAX / dmax))
    assert len(cases("range")) == 4


def test_empty_words_stay_and_padded_dims_are_zeroed():
    for name, (w, M, K, Cs, init, it) in cases("empty_words").items():
        (ctrd, asmt, st), trace = ref("empty_words", name)
        a = asmt.reshape(-1, M)
        empty = [K - len(np.unique(a[:, m])) for m in range(M)]
        assert min(empty) > K // 2, (name, empty)
        cin = np.asarray(w).shape[1]
        cse = cin - (M - 1) * Cs
        assert cse < Cs and (init[M - 1, :, cse:] != 0).all()
        assert ctrd[M - 1, :, cse:].tobytes() == np.zeros((K, Cs - cse), np.float32).tobytes()
        kept = 0
        for m in range(M):
            e = min(cin - m * Cs, Cs)
            for k in (trace["never_member"][m] if it else range(K)):
                assert ctrd[m, k, :e].tobytes() == init[m, k, :e].tobytes(), (name, m, k)
                kept += 1
        assert kept > 0 and np.signbit(ctrd).any()                 # -0.0 is still there
        print("empty_words/%s: empty code words per sub-space %r, %d kept bit for bit" % (name, empty, kept))
    assert any(K == 256 and np.asarray(w).shape[0] == 40 for (w, M, K, *_) in cases("empty_words").values())


def test_active_set_subspaces_converge_at_different_steps():
    (c_all, a_all, st_all), tr_all = ref("active_set", "m4_iter60")
    (c_few, a_few, st_few), tr_few = ref("active_set", "m4_iter2")
    steps = [tr_all["steps"][m] for m in range(4)]
    print("active_set: steps to convergence per sub-space %r" % steps)
    assert steps[0] == 1 and len(set(steps)) >= 3 and max(steps) < 60
    assert st_all["unconverged"] == 0 and st_all["iters"] == max(steps)
    assert st_few["iters"] == 2 and st_few["unconverged"] == sum(s > 2 for s in steps) and 0 < st_few["unconverged"] < 4
    # the fixed point is one from the start: its book is the given one
    assert c_all[0].tobytes() == cases("active_set")["m4_iter60"][4][0].tobytes()


def test_sizes_and_cs_sweep_cover_what_they_name():
    names = cases("sizes")
    for N in pc.SIZES:
        for kind in ("k3_seeded", "k5_given"):
            assert np.asarray(names["n%d_%s" % (N, kind)][0]).shape[0] == N
        assert names["n%d_k256_given" % N][0].shape[0] == N
        assert ("n%d_k256_seeded" % N in names) == (N <= 257 or N == 4097)
    pairs = set()
    for (w, M, K, Cs, init, it) in cases("cs_sweep").values():
        cin = np.asarray(w).shape[1]
        assert M == 2
        pairs.add((Cs, cin - Cs, K, init is None))
    assert pairs == {(Cs, e, K, K == 2) for Cs in range(1, 17) for e in range(1, Cs + 1) for K in (2, 11)}


# ------------------------------------------------------------------------------ wrong variants must change bytes
@pytest.mark.parametrize("variant", pc.WRONG)
def test_wrong_variant_is_noticed_by_its_family(variant):
    family = FAMILY_OF[variant]
    caught = []
    for name, (w, M, K, Cs, init, it) in cases(family).items():
        got = pc.quantize_layer(w, M, K, Cs, ctrd_init=init, max_iter=it, wrong=(variant,))
        if not same_bytes(got, oracle(family, name)):
            caught.append(name)
    print("%s: changes the bytes of %d of %d %s cases: %s" % (variant, len(caught), len(cases(family)), family, ", ".join(caught)))
    assert caught, "%s passes every case of %s" % (variant, family)


def test_every_variant_has_a_family():
    assert sorted(FAMILY_OF) == sorted(pc.WRONG)
