"""CPU tier of the one-hot table probes (tests/table_probe.py): the helper's reading of the file layouts, of groups and of
padding is pinned to the oracle (and, where it is built, to the compiled reference); the checker is shown to fail on
degraded operands that every max-norm bar of the suite lets through; the schedules name what they claim to name."""
import numpy as np
import pytest

import pyoracle as po
import table_probe as tp
from conftest import pkg
from test_bf16split_cpu import bf16_rn, split3

topo = pkg("topology")
synth = pkg("synth")

# what the issue's own CPU experiment used, beside the shapes of the GPU file: grouped and ungrouped conv, a 3-dim single
# sub-space, a partial last sub-space, Cs 8 / 4 / 1, K 128 / 32 / 16, padded and strided windows
EXTRA = {
    "grouped_pad_stride": ("conv", tp.conv_geom(12, 10, 24, 3, 2, 1, 2, 32), 2, 32, 8, None),      # 12 per group: 8 + 4 dims
    "cs1_k16": ("conv", tp.conv_geom(6, 7, 3, 2, 1, 1, 1, 16), 3, 16, 1, None),
    "fc_partial": ("fc", tp.fc_geom(30, 24), 8, 32, 4, None),                                      # last sub-space: 2 of 4 dims
}
ALL = dict(tp.SHAPES, **EXTRA)


def layer_of(kind, g):
    if kind == "conv":
        return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"])]
    return (g["D"], 1, 1), [topo.fcnt(g["Ct"])]


def oracle_out(kind, g, params, x):
    in_chw, layers = layer_of(kind, g)
    orc = po.COracle(in_chw, layers)
    orc.set_params({0: params})
    y = orc.run_layer(0, x, x.shape[0])
    orc.close()
    return y if kind == "conv" else y.reshape(x.shape[0], -1)


@pytest.mark.parametrize("name", sorted(ALL))
def test_helper_equals_the_oracle_bit_for_bit(name):
    """Every round of every shape, both input sets: the oracle's output IS want32_seq (so the helper reads asmt / ctrd /
    groups / padding as the pinned oracle does), lies inside the bound, is exactly zero in the padding; at least half of
    the outputs are informative."""
    kind, g, M, K, Cs, mr = ALL[name]
    n_terms = max(tp.cs_eff(kind, g, M, Cs))
    rounds = tp.schedule(kind, g, M, K, Cs, max_rounds=mr, negate=True)
    worst = 0.0
    for i, rd in enumerate(rounds):
        if i not in (0, len(rounds) // 2 - 1, len(rounds) - 1) and name in tp.SHAPES and len(rounds) > 6:
            continue                                   # long schedules: first, last plain and last negated round
        params = tp.probe_params(kind, g, M, K, Cs, rd, seed=3)
        for scaled in (False, True):
            x = tp.activations(kind, g, 2, seed=4 + i, scaled=scaled)
            want64, mag, seq = tp.expected(kind, g, x, params)
            y = oracle_out(kind, g, params, x)
            assert np.array_equal(y, seq), (name, rd, scaled)
            worst = max(worst, tp.check(y, want64, mag, n_terms, what="%s %r" % (name, rd)))
            assert tp.informative_share(mag) >= 0.5, (name, rd, tp.informative_share(mag))
    print("%s: worst err / bound %.3f" % (name, worst))
    assert worst <= 1.0


@pytest.mark.skipif(not po.have_ref(), reason="oracle/_ref/libqcnn_ref.so not built")
@pytest.mark.parametrize("name", ["grouped_pad_stride", "fc_partial"])
def test_helper_equals_the_compiled_reference(name, tmp_path):
    kind, g, M, K, Cs, mr = ALL[name]
    in_chw, layers = layer_of(kind, g)
    for i, rd in enumerate(tp.schedule(kind, g, M, K, Cs)[:2]):
        params = tp.probe_params(kind, g, M, K, Cs, rd, seed=5)
        d = tmp_path / ("r%d" % i)
        synth.write_param_dir(str(d), "t", {0: {k: params[k] for k in ("bias", "ctrd", "asmt", "bits")}})
        ref = po.RefLib()
        ref.load_custom(str(d), "t", in_chw, layers)
        x = tp.activations(kind, g, 1, seed=6, scaled=bool(i))
        want64, mag, seq = tp.expected(kind, g, x, params)
        y = ref.run_layer(0, x).reshape(seq.shape)
        assert np.array_equal(y, seq), (name, rd)
        tp.check(y, want64, mag, max(tp.cs_eff(kind, g, M, Cs)), what=name)


# ---------------------------------------------------------------- the checker can fail ----
def _conv_case(name, seed=7, scaled=False):
    kind, g, M, K, Cs, mr = ALL[name]
    params = tp.probe_params(kind, g, M, K, Cs, tp.schedule(kind, g, M, K, Cs)[0], seed=seed)
    x = tp.activations(kind, g, 3, seed=seed + 1, scaled=scaled)
    return kind, g, params, x, max(tp.cs_eff(kind, g, M, Cs))


@pytest.mark.parametrize("scaled", [False, True])
def test_checker_trips_on_code_words_kept_as_two_bf16_pieces(scaled):
    """(a) a builder that keeps two bf16 pieces of every code word and drops the third: about 2^-17 per product, invisible to
    the 1e-4 max-norm bar (asserted here), beyond gamma_8 = 2^-21."""
    kind, g, params, x, n = _conv_case("alex_conv2", scaled=scaled)
    want64, mag, seq = tp.expected(kind, g, x, params)
    c1 = bf16_rn(params["ctrd"])
    degraded = dict(params, ctrd=(c1 + bf16_rn(params["ctrd"] - c1)).astype(np.float32))
    _, _, y = tp.expected(kind, g, x, degraded)
    assert np.abs(y - want64).max() <= 1e-4 * np.abs(want64).max()          # the suite's loose bar does not see it
    tp.check(seq, want64, mag, n)                                             # the undegraded sequence passes
    with pytest.raises(AssertionError, match="beyond the bound"):
        tp.check(y, want64, mag, n)


def _six_terms(x, w, drop=None):
    """The split-bf16 product model of tests/test_bf16split_cpu.py in float64, optionally without one 2^-16-order term."""
    x1, x2, x3 = (p.astype(np.float64) for p in split3(x))
    w1, w2, w3 = (p.astype(np.float64) for p in split3(w))
    terms = {"x3w1": x3 * w1, "x2w2": x2 * w2, "x1w3": x1 * w3}
    s = x2 * w1 + x1 * w2 + x1 * w1
    for k, t in terms.items():
        if k != drop:
            s = s + t
    return s


@pytest.mark.parametrize("drop", ["x3w1", "x2w2", "x1w3"])
def test_checker_trips_on_a_dropped_cross_term_of_the_split(drop):
    """(b) the six-term split with one of its three 2^-16-order terms left out, against the split bound
    (2^-22 + gamma_(6 CsEff)) * mag: the complete model passes, the incomplete one does not."""
    kind, g, params, x, n = _conv_case("alex_conv1")
    want64, mag, _ = tp.expected(kind, g, x, params)
    Ho, Wo = tp.out_hw(g)
    s = g["stride"]
    full = np.zeros_like(want64)
    cut = np.zeros_like(want64)
    for ct, (kh, kw, m, k) in enumerate(params["picks"]):
        sl = x[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, :n]
        w = np.broadcast_to(params["ctrd"][m, k, :n], sl.shape)
        full[..., ct] = _six_terms(sl, w).sum(-1)
        cut[..., ct] = _six_terms(sl, w, drop).sum(-1)
    extra = tp.split_extra(n)
    assert tp.check(full.astype(np.float32), want64, mag, n, extra=extra) <= 1.0
    assert np.abs(cut - want64).max() <= 1e-4 * np.abs(want64).max()         # far inside the oracle bar of the decoded layer
    with pytest.raises(AssertionError, match="beyond the bound"):
        tp.check(cut.astype(np.float32), want64, mag, n, extra=extra)


def test_checker_trips_on_a_neighbour_lanes_entry():
    """(c) one entry of one image replaced by its neighbour lane's (the next output channel's)."""
    kind, g, params, x, n = _conv_case("c3_128")
    want64, mag, seq = tp.expected(kind, g, x, params)
    y = seq.copy()
    y[2, 5, 6, 40] = seq[2, 5, 6, 41]
    with pytest.raises(AssertionError, match="beyond the bound"):
        tp.check(y, want64, mag, n)


def test_checker_trips_on_a_non_zero_value_in_the_padding():
    """(d) the tap of channel ct at output (0, 0) lies in the padding for kh* = 0: the output must be exactly 0."""
    kind, g, params, x, n = _conv_case("c3_128")
    want64, mag, seq = tp.expected(kind, g, x, params)
    ct = int(np.flatnonzero(params["picks"][:, 0] == 0)[0])
    assert mag[1, 0, 0, ct] == 0 and seq[1, 0, 0, ct] == 0
    y = seq.copy()
    y[1, 0, 0, ct] = np.float32(1e-30)
    with pytest.raises(AssertionError, match="padding"):
        tp.check(y, want64, mag, n)


def test_relu_form_of_the_checker():
    kind, g, params, x, n = _conv_case("c3_64")
    want64, mag, seq = tp.expected(kind, g, x, params)
    assert (seq < 0).any() and (seq > 0).any()
    tp.check(np.maximum(seq, 0), want64, mag, n, relu=True)
    with pytest.raises(AssertionError):
        tp.check(np.maximum(seq, 0), want64, mag, n)


# ---------------------------------------------------------------- schedule coverage ----
@pytest.mark.parametrize("name", sorted(tp.SHAPES))
def test_schedule_coverage(name):
    """Every (m, k) — k = 0 through the rounds whose silent word is K - 1 — and every tap is named at least once, and every
    (m, k) at least once with a tap that lies inside the map; a thinned schedule (fc6) still names every m and every k."""
    kind, g, M, K, Cs, mr = tp.SHAPES[name]
    rounds = tp.shape_rounds(name)
    pairs, taps, inside = tp.covered(kind, g, M, K, rounds)
    assert taps.all(), np.argwhere(~taps)
    if mr is None:
        assert pairs.all() and inside.all(), (int((~pairs).sum()), int((~inside).sum()))
    else:
        assert pairs.any(axis=1).all() and pairs.any(axis=0).all()
        assert pairs[:, 0].all()                                              # k = 0 in every sub-space
        print("%s: %.1f %% of the (m, k) pairs" % (name, 100.0 * pairs.mean()))
    for rd in rounds:                                                         # a probe is a valid parameter set
        p = tp.probe_params(kind, g, M, K, Cs, rd)
        assert p["asmt"].max() < K and (p["ctrd"][:, rd["silent"]] == 0).all() and np.isfinite(p["ctrd"]).all()
        assert ((p["asmt"] != rd["silent"]).reshape(p["asmt"].shape[0], -1).sum(1) == 1).all()
