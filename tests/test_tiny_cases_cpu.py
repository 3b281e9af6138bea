"""CPU tier of the tiny-map cases (tests/test_gpu_tiny_cases.py, the tg_* shapes of tests/table_probe.py): maps smaller than the
kernel and smaller than a tile — 1 x 1, one row, one column, windows clipped on both sides at once, stride > knl.

  * Live families: through qcnn_plan_conv_query, under the option values the GPU tier forces a family with, every family
    TINY_REACH lists is the planner's choice (the sliding forms on tg_col, the fall-back to the family's tile form on every map
    with fewer than 2 x slots output rows), every family listed as dead has cost 0, split forms are cut as recorded at one panel;
    the few-image launcher's and the decoded panel form's choice are the recorded ones.
  * At least one stage per workgroup: every tile's / strip's hiL, hiU, wiL, wiU and Stot and every slice's [sBeg, sBeg + S) are
    re-derived from the kernels' formulas (k_conv_aprx, k_conv_sym, k_conv_sym8, k_conv_half8), written again below, for every
    shape, live family, tile, segment and slice: rows >= 1, cols >= 1, S >= 1.  tg_1x2's eight stages cut six ways hold one-stage
    slices.  That pad < knl implies rows, cols >= 1 is shown over every (size, knl, stride, pad) with size <= 9, knl <= 5,
    stride <= 4 and EVERY run of consecutive output rows (so every tile size and every segment); the same sweep at pad = knl finds
    tiles of the emitted sizes with no row or no column — the geometry qcnn_model_begin and qcnn_plan_conv_query refuse.
  * The references alone meet the bound of the GPU tier: oracle (exact order) and the float32 MFMA-order emulation against
    table_probe.dense_expected within gamma(knl^2 M + CsEff + 1) * mag.
  * Teeth: one live term removed or doubled, one padding tap replaced by the clamped border pixel's entry (clamp instead of zero),
    on tg_gap an uncovered source pixel's entry added to the nearest window: each leaves the bound.
  * The dense (precise) path: a float64 restatement of its tap rule — the reference's lower-bound quirk as is, a tap whose source
    row or column lies outside the map contributes 0 — holds the oracle's dense path on the tg_* geometries and on tg_1x1 at
    3x3 / 2 pad 1; old and new rule agree wherever pad - kh + H - 1 >= 0."""
import ctypes as C
import itertools

import numpy as np
import pytest

import isolation_cases as ic
import pyoracle as po
import table_probe as tp
from conftest import pkg
from test_decoded_cases_cpu import conv_dec_instance, conv_dec_shape
from test_gpu_table_probe import EXACT, SPLIT_SYM8, SPLIT_TILE, TILE, code_ok
from test_panel_cases_cpu import CONV_TILE, FAMS, HALF8_CASES, derive, mfma_order_out, one_term, plan, slice_starts, tile_of_rank
from test_planner_cpu import COSTS, planner          # (the fixture)
from test_small_cases_cpu import LDS_PER_WORKGROUP, constants, conv_small_plan, stage_group
from test_table_probe_cpu import layer_of, oracle_out

synth = pkg("synth")
build = pkg("build")

TINY = sorted(tp.TINY_SHAPES)
TILE_FAMS = ("tile", "sym16", "sym8", "half8")
SLIDE_FAMS = ("slide16", "sym8_slide", "half8_slide")
SLIDE_TILE = {"slide16": "tile", "sym8_slide": "sym8", "half8_slide": "half8"}     # the tile form a sliding family falls back to
N_REF = 5


# ---------------------------------------------------------------- live families ----
@pytest.mark.parametrize("name", TINY)
def test_every_listed_family_is_live_and_cut_as_recorded(name, planner):
    shape = tp.TINY_SHAPES[name]
    kind, g, M, K, Cs, _ = shape
    reach = tp.TINY_REACH[name]
    assert 0 <= g["pad"] < g["knl"]
    d = derive(shape)
    assert (d["G"], d["last_group"], d["per_pixel"]) == reach["stage"], (name, d)
    whole = [k for k in reach["live"] if not k.startswith("split_")]
    for k in whole:
        assert d.get(k) == reach["live"][k], (name, k, d.get(k))
    assert sorted(k for k in COSTS if k in d) == sorted(whole), (name, sorted(d))
    assert set(reach["dead"]) == set(COSTS) - set(whole)
    Ho, Wo = tp.out_hw(g)
    for panels in (1, 2):                                # 131 images; 125, 70, 5 and 3
        for k in COSTS:
            costs, ch = plan(planner, shape, panels, FAMS[k]["opts"])
            got = (ch["family"], len(ch["segs"]) - 1 if ch["segs"] else ch["Z"])
            if k in whole:
                assert costs[k] > 0.0 and code_ok(FAMS[k]["code"], got), (name, k, panels, ch)
                assert ch["Z"] <= 1                                               # (split = 0: whole tiles)
                if k in SLIDE_FAMS:
                    ns = d[k][1]
                    assert ch["segs"][0] == 0 and ch["segs"][-1] == Ho >= 2 * ns and len(ch["segs"]) >= 3, (name, k, ch)
            else:
                # not eligible: cost 0, and forcing it runs the family's tile form (or the 16-wave tile kernel), whole
                assert costs[k] == 0.0, (name, k, costs)
                fall = SLIDE_TILE.get(k)
                want = FAMS[fall]["code"] if fall in whole else TILE["code"]
                assert code_ok(want, got), (name, k, ch)
        costs, ch0 = plan(planner, shape, panels, EXACT["opts"])
        assert ch0["family"] == -1 and ch0["Z"] <= 1
    for k, f in (("split_tile", SPLIT_TILE), ("split_sym8", SPLIT_SYM8)):          # one panel: the batch of 125 images
        _, ch = plan(planner, shape, 1, f["opts"])
        if k in reach["live"]:
            Z, frm = reach["live"][k]
            assert Z > 1 and (ch["Z"], ch["split_from"]) == (Z, frm), (name, k, ch)
            assert ch["family"] == (-1 if k == "split_tile" else -5)
            assert code_ok(f["code"], (ch["split_from"], ch["Z"]) if k == "split_tile" else (ch["family"], ch["Z"]))
        else:
            assert ch["Z"] <= 1 or ch["family"] != (-1 if k == "split_tile" else -5), (name, k, ch)
    c = constants()
    p = conv_small_plan(g, M, K, Cs, c)
    assert p is not None and (p["TH"], p["TW"], p["MC"], p["CH"], p["chunks"], stage_group(K)) == reach["small"], (name, p)
    assert p["lds"] <= LDS_PER_WORKGROUP and p["TH"] <= Ho and p["TW"] <= Wo
    if name in tp.TINY_DEC:
        kp, s = conv_dec_shape(g, M)
        ns = kp // 4
        many = conv_dec_instance(g, 128, 2)
        assert (s, ns, g["knl"] * ns, many, conv_dec_instance(g, 5, 1), g["Ct"] // (16 * many[0])) == reach["dec"]
        assert many[2] and conv_dec_instance(g, 5, 1)[2]                           # padded layers: the clamped instantiations
    else:
        assert conv_dec_shape(g, M) is None
    if K in (16, 32, 64, 128):                           # a ragged last sub-space / stage: the operand over-read stays inside the slack
        assert ic.over_read(kind, g, M, K, Cs)["bytes"] < ic.K_SLACK


def test_what_each_shape_is_there_for():
    S, R = tp.TINY_SHAPES, tp.TINY_REACH
    assert sorted(S) == sorted(R) and set(tp.TINY_BASE) <= set(S) and len(tp.TINY_BASE) == 10
    hw = {n: (S[n][1]["H"], S[n][1]["W"], tp.out_hw(S[n][1])) for n in tp.TINY_BASE}
    assert hw == {"tg_1x1": (1, 1, (1, 1)), "tg_row": (1, 4, (1, 4)), "tg_col": (7, 1, (7, 1)), "tg_k5": (2, 3, (2, 3)),
                  "tg_pad2": (2, 2, (4, 4)), "tg_s2": (3, 4, (2, 2)), "tg_fit": (3, 3, (1, 1)), "tg_gap": (7, 8, (2, 3)),
                  "tg_s4": (4, 9, (1, 3)), "tg_1x2": (1, 2, (1, 2))}
    for n in tp.TINY_BASE:                               # the base rows: tile, 16-wave symmetric, eight-wave and half-panel all live
        assert set(TILE_FAMS) <= set(R[n]["live"]) and S[n][2:5] == (4, 128, 8)
        c = R[n + "_c512"]["live"]                       # 512 channels: two eight-wave chunks of 1x3 tiles, half panels of 64 channels per wave
        assert c["sym8"][:4] == (32, 1, 3, 2) and c["half8"][:4] == HALF8_CASES[512] and c["tile"][:4] == (24, 1, 1, 2)
    # only tg_col has the 2 x slots output rows a sliding form needs: all three, in two segments, strips as wide as or wider than the map
    assert [n for n in tp.TINY_TABLE if any(k in R[n]["live"] for k in SLIDE_FAMS)] == ["tg_col", "tg_col_c512"]
    assert set(SLIDE_FAMS) <= set(R["tg_col"]["live"]) and R["tg_col"]["live"]["sym8_slide"][2] == 2 and R["tg_col"]["live"]["half8_slide"][2] == 4
    # every tile larger than the whole output map in both axes
    assert all(R["tg_1x1"]["live"][k][-2] == (1, 1) for k in TILE_FAMS)
    assert {R["tg_1x1"]["live"][k][1:3] for k in TILE_FAMS} == {(1, 3), (2, 2), (2, 3), (3, 4)}
    assert R["tg_1x1_c192"]["live"]["sym8"][:3] == (24, 2, 2) and R["tg_1x1_c192"]["live"]["half8"][:4] == HALF8_CASES[192]
    assert R["tg_1x1_c384"]["live"]["sym8"][:3] == (48, 1, 2) and R["tg_1x1_c384"]["live"]["half8"][:4] == HALF8_CASES[384]
    # kernel larger than the map / pad = knl - 1 / stride > knl
    g = S["tg_k5"][1]
    assert g["knl"] > max(g["H"], g["W"])
    assert S["tg_pad2"][1]["pad"] == S["tg_pad2"][1]["knl"] - 1
    assert all(S[n][1]["stride"] > S[n][1]["knl"] for n in ("tg_gap", "tg_s4")) and S["tg_s4"][1]["pad"] and not S["tg_gap"][1]["pad"]
    # a ragged sub-space in two groups on a two-row map; stages of four sub-spaces with a ragged last one
    assert tp.cs_eff(*S["tg_k5_g2"][:2], 3, 8) == [8, 8, 4] and S["tg_k5_g2"][1]["grp"] == 2 and S["tg_k5_g2"][1]["Ct"] == 256
    assert R["tg_pad2_m7"]["stage"] == (4, 3, 2) and tp.cs_eff(*S["tg_pad2_m7"][:2], 7, 4) == [4] * 7
    # tg_1x2: eight stages, cut six ways
    assert R["tg_1x2"]["live"]["sym8"][-1] == 8 and R["tg_1x2"]["live"]["split_sym8"] == (6, 0)
    # both split forms are live somewhere, and so is every family
    assert {k for n in TINY for k in R[n]["live"]} == set(FAMS)
    # the precise path: the tg_* geometries and the one whose upper tap bound truncates to 0 (H = 1, 3x3 / 2, pad 1, kh = 2)
    g = tp.TINY_DENSE["tg_1x1_s2"]
    assert -g["stride"] < g["pad"] - 2 + g["H"] - 1 < 0 and tp.out_hw(g) == (1, 1)


# ---------------------------------------------------------------- at least one stage per workgroup ----
def span_1d(size, knl, stride, pad, o0, oL):
    """(iL, iU) of the source rows (columns) output rows (columns) o0 .. oL look at, as the kernels clip them:
    hiL = max(0, ho0 s - pad), hiU = min(H - 1, hoL s - pad + knl - 1)."""
    return max(0, o0 * stride - pad), min(size - 1, oL * stride - pad + knl - 1)


def workgroups(g, MG, fam, cfg, Z=1, frm=0, segs=None):
    """[(what, rows, cols, [S of every slice])] of a launch of one family: tile kernels — tile (ty, tx) of th x tw outputs, ranks from
    `frm` on cut into Z slices [Stot z / Z, Stot (z + 1) / Z); sliding forms — output rows [segs[i], segs[i + 1]) of a strip of nc
    output columns."""
    Ho, Wo = tp.out_hw(g)
    s, pad, knl = g["stride"], g["pad"], g["knl"]
    out = []
    if fam in SLIDE_FAMS:
        nc = cfg[2]
        for a, b in zip(segs, segs[1:]):
            for tx in range(0, Wo, nc):
                hiL, hiU = span_1d(g["H"], knl, s, pad, a, b - 1)
                wiL, wiU = span_1d(g["W"], knl, s, pad, tx, min(tx + nc, Wo) - 1)
                rows, cols = hiU - hiL + 1, wiU - wiL + 1
                out.append(("rows [%d, %d) x columns from %d" % (a, b, tx), rows, cols, [rows * cols * MG]))
        return out
    th, tw = cfg[1], cfg[2]
    tilesY, tilesX = -(-Ho // th), -(-Wo // tw)
    for r in range(tilesY * tilesX):
        ty, tx = tile_of_rank(r, tilesY, tilesX)
        hiL, hiU = span_1d(g["H"], knl, s, pad, ty * th, min(ty * th + th, Ho) - 1)
        wiL, wiU = span_1d(g["W"], knl, s, pad, tx * tw, min(tx * tw + tw, Wo) - 1)
        rows, cols = hiU - hiL + 1, wiU - wiL + 1
        Stot = rows * cols * MG
        z = Z if r >= frm else 1
        out.append(("tile (%d, %d)" % (ty, tx), rows, cols, [Stot * (i + 1) // z - Stot * i // z for i in range(z)]))
    return out


def launches(name, planner):
    """[(family key, workgroups)] of every live family of a shape, split forms at one panel included."""
    shape = tp.TINY_SHAPES[name]
    g = shape[1]
    reach = tp.TINY_REACH[name]
    MG = reach["stage"][2]
    out = []
    for k, cfg in reach["live"].items():
        if k.startswith("split_"):
            base = reach["live"]["tile" if k == "split_tile" else "sym8"]
            # the ranks are heaviest first; split_from = 0 on every tg_* shape, so every tile is cut whatever the order
            assert cfg[1] == 0
            out.append((k, workgroups(g, MG, "tile", base, Z=cfg[0], frm=0)))
        elif k in SLIDE_FAMS:
            for panels in (1, 2):
                segs = plan(planner, shape, panels, FAMS[k]["opts"])[1]["segs"]
                out.append((k, workgroups(g, MG, k, cfg, segs=segs)))
        else:
            out.append((k, workgroups(g, MG, k, cfg)))
    return out


@pytest.mark.parametrize("name", TINY)
def test_every_workgroup_has_a_row_a_column_and_a_stage(name, planner):
    reach = tp.TINY_REACH[name]
    for k, wgs in launches(name, planner):
        assert wgs
        for what, rows, cols, S in wgs:
            assert rows >= 1 and cols >= 1, (name, k, what, rows, cols)
            assert min(S) >= 1, (name, k, what, S)
        if not k.startswith("split_") and k not in SLIDE_FAMS:      # the recorded "stages of the heaviest tile"
            assert max(sum(S) for _, _, _, S in wgs) == reach["live"][k][-1]


def test_the_one_stage_slice(planner):
    """tg_1x2: one tile of 1 x 2 pixels x 4 sub-spaces = 8 stages, cut into 6 slices by the split eight-wave form: 1, 1, 2, 1, 1, 2.
    A slice of ONE stage rounds up to two stage periods; the surplus one re-fetches the first."""
    wgs = dict(launches("tg_1x2", planner))["split_sym8"]
    assert len(wgs) == 1 and wgs[0][3] == [1, 1, 2, 1, 1, 2]
    assert slice_starts(8, 6) == [1, 2, 4, 5, 6]
    ones = [n for n in TINY for k, w in launches(n, planner) if k.startswith("split_") for _, _, _, S in w if 1 in S]
    assert "tg_1x2" in ones
    print("shapes with a one-stage slice:", sorted(set(ones)))


TILE_SIZES = sorted(set(CONV_TILE.values()) | {(2, 2), (2, 3), (1, 3), (1, 2)} | {v[1:3] for v in HALF8_CASES.values()})
STRIP_COLS = (1, 2, 4)


def sweep_1d(pad_of):
    """{(size, knl, stride, pad, o0, oL): span} over size <= 9, knl <= 5, stride <= 4, pad = pad_of(knl) and EVERY run o0 .. oL of
    consecutive output rows — a superset of every tile row range [ty th, min(ty th + th, Ho)) and every segment [segBeg, segEnd)."""
    out = {}
    for size, knl, stride in itertools.product(range(1, 10), range(1, 6), range(1, 5)):
        for pad in pad_of(knl):
            n_out = (size + 2 * pad - knl) // stride + 1 if size + 2 * pad >= knl else 0
            for o0 in range(n_out):
                for oL in range(o0, n_out):
                    lo, hi = span_1d(size, knl, stride, pad, o0, oL)
                    out[size, knl, stride, pad, o0, oL] = hi - lo + 1
    return out


def test_pad_below_knl_gives_every_tile_a_row_and_a_column():
    """rows and cols are the same one-dimensional expression, so H, W <= 9 is size <= 9 twice.  pad < knl: every window holds a
    pixel of the map, so every run of output rows spans >= 1 source rows — for ANY tile size and segment, the emitted ones
    (TILE_SIZES, STRIP_COLS) among them; with MG >= 1 stages per pixel, Stot = rows cols MG >= 1."""
    spans = sweep_1d(lambda knl: range(knl))
    assert len(spans) > 4000 and min(spans.values()) >= 1
    # the same statement in the kernels' terms, for the tile sizes and strip widths the launchers emit
    n = 0
    for size, knl, stride in itertools.product(range(1, 10), range(1, 6), range(1, 5)):
        for pad in range(knl):
            n_out = (size + 2 * pad - knl) // stride + 1 if size + 2 * pad >= knl else 0
            for t in {th for th, _ in TILE_SIZES} | {tw for _, tw in TILE_SIZES} | set(STRIP_COLS):
                for o0 in range(0, n_out, t):
                    assert spans[size, knl, stride, pad, o0, min(o0 + t, n_out) - 1] >= 1
                    n += 1
    assert n > 3000


def raw_query(geom):
    lib = C.CDLL(build.build_planner_cpu())
    lib.qcnn_plan_conv_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    return lib.qcnn_plan_conv_query((C.c_int * 14)(*geom), (C.c_int * 8)(1, 1, 1, 1, 1, 1, 0, 64), (C.c_double * 7)(), (C.c_int * 13)())


def test_pad_equal_to_knl_leaves_tiles_without_a_row_or_a_column():
    """The counter-examples: at pad = knl the first (and last) window lies wholly in the padding, and tiles of the emitted sizes have
    rows <= 0 (a stage loop that never runs behind a first stage that is still fetched) or cols = 0 (a division by zero in the first
    stage's position).  qcnn_model_begin refuses that geometry (tests/test_gpu_tiny_cases.py); so does qcnn_plan_conv_query."""
    spans = sweep_1d(lambda knl: (knl,))
    bad = {k: v for k, v in spans.items() if v <= 0}
    assert bad and all(v == 0 for v in bad.values())     # pad = knl: exactly no row; one more pixel of padding (the 1x1 pad 2 layer) ...
    assert min(sweep_1d(lambda knl: (knl + 1,)).values()) < 0                              # ... and the count goes negative
    # every (size, knl, stride) has such a tile of ONE output row — the first one
    for size, knl, stride in itertools.product(range(1, 10), range(1, 6), range(1, 5)):
        assert spans[size, knl, stride, knl, 0, 0] <= 0
    # the two layers the planner used to return a plan for: 1x1 pad 2 on 4 x 4 (pad > knl) and 3x3 pad 3 on 2 x 2 — and a 1x1 pad 1 layer
    for H, W, knl, pad in ((4, 4, 1, 2), (2, 2, 3, 3), (4, 4, 1, 1)):
        Ho, Wo = H + 2 * pad - knl + 1, W + 2 * pad - knl + 1
        lo, hi = span_1d(H, knl, 1, pad, 0, 0)
        assert hi - lo + 1 <= 0
        for Ct in (128, 512):
            assert raw_query([H, W, 32, Ho, Wo, Ct, knl, 1, pad, 1, 4, 8, 128, 2]) != 0
    assert raw_query([4, 4, 32, 4, 4, 128, 3, 1, -1, 1, 4, 8, 128, 2]) != 0           # a negative padding
    assert raw_query([4, 4, 32, 6, 6, 128, 3, 1, 2, 1, 4, 8, 128, 2]) == 0            # pad = knl - 1: admitted


# ---------------------------------------------------------------- the references alone stay inside the bound ----
def dense_case(name, seed=181, n=N_REF):
    kind, g, M, K, Cs, _ = tp.TINY_SHAPES[name]
    spec = {0: dict(kind=kind, M=M, K=K, Cs=Cs, Ct=g["Ct"], knl=g["knl"], D=g["Cin"] // g["grp"])}
    params = synth.make_params(None, None, seed=seed, spec=spec)[0]
    x = tp.activations(kind, g, n, seed=seed + 1, scaled=False)
    return g, M, Cs, params, x


@pytest.mark.parametrize("name", TINY)
def test_references_stay_inside_the_dense_sum_bound(name):
    g, M, Cs, params, x = dense_case(name)
    want64, mag = tp.dense_expected("conv", g, x, params)
    n_terms = tp.dense_count("conv", g, M, Cs)
    exact = tp.dense_check(oracle_out("conv", g, params, x), want64, mag, n_terms, what=name + " exact builder")
    mfma = tp.dense_check(mfma_order_out(g, params, x), want64, mag, n_terms, what=name + " MFMA order")
    print("%s: worst err / bound: oracle (exact builder) %.3f, MFMA order %.3f" % (name, exact, mfma))
    assert exact <= 1.0 and mfma <= 1.0


# ---------------------------------------------------------------- the check has teeth ----
def entry64(g, params, x, ct, kh, kw, m, hi, wi):
    """float64 table entry [n] of source pixel (hi, wi), sub-space m, for the code word channel ct's tap (kh, kw) names."""
    M, K, Cs = params["ctrd"].shape
    knl, grp, Ct = g["knl"], g["grp"], g["Ct"]
    cse = tp.cs_eff("conv", g, M, Cs)[m]
    c0 = (ct // (Ct // grp)) * (g["Cin"] // grp) + m * Cs
    k = int(np.asarray(params["asmt"]).reshape(Ct, knl, knl, M)[ct, kh, kw, m])
    word = np.asarray(params["ctrd"], np.float32)[m, k, :cse].astype(np.float64)
    return np.asarray(x, np.float32)[:, hi, wi, c0:c0 + cse].astype(np.float64) @ word


def live_taps(g):
    Ho, Wo = tp.out_hw(g)
    return [(kh, kw) for kh in range(g["knl"]) for kw in range(g["knl"])
            if tp._tap_inside(g, kh, g["H"], Ho) and tp._tap_inside(g, kw, g["W"], Wo)]


def padding_taps(g):
    """[(ho, wo, kh, kw, clamped hi, clamped wi)] of every tap of every window that lies in the padding."""
    Ho, Wo = tp.out_hw(g)
    out = []
    for ho, wo, kh, kw in itertools.product(range(Ho), range(Wo), range(g["knl"]), range(g["knl"])):
        hi, wi = ho * g["stride"] - g["pad"] + kh, wo * g["stride"] - g["pad"] + kw
        if not (0 <= hi < g["H"] and 0 <= wi < g["W"]):
            out.append((ho, wo, kh, kw, min(max(hi, 0), g["H"] - 1), min(max(wi, 0), g["W"] - 1)))
    return out


def must_leave(y, want64, mag, n_terms, ct, what):
    with pytest.raises(AssertionError, match="beyond the bound"):
        tp.dense_check(y.astype(np.float32), want64, mag, n_terms, what=what)
    others = np.arange(y.shape[-1]) != ct                # ... and only through the channel that was touched
    assert tp.dense_check(y.astype(np.float32)[..., others], want64[..., others], mag[..., others], n_terms) <= 1.0


@pytest.mark.parametrize("name", TINY)
def test_a_missing_doubled_or_clamped_term_leaves_the_bound(name):
    g, M, Cs, params, x = dense_case(name)
    want64, mag = tp.dense_expected("conv", g, x, params)
    n_terms = tp.dense_count("conv", g, M, Cs)
    assert tp.dense_check(want64.astype(np.float32), want64, mag, n_terms) <= 1.0
    taps = live_taps(g)
    picks = [taps[0] + (0,), taps[len(taps) // 2] + (M // 2,), taps[-1] + (M - 1,)]
    for i, (kh, kw, m) in enumerate(picks):              # one live (kh, kw, m) term removed or added twice
        ct = (5 + 37 * i) % g["Ct"]
        t = one_term(g, params, x, ct, kh, kw, m)
        assert (t != 0).any()
        for sign, what in ((-1.0, "missing"), (1.0, "doubled")):
            y = want64.copy()
            y[..., ct] += sign * t
            must_leave(y, want64, mag, n_terms, ct, "%s %s term %r" % (name, what, (kh, kw, m)))
    pads = padding_taps(g)
    assert bool(pads) == (g["pad"] > 0)
    if pads:                                             # clamp instead of zero: a padding tap takes the border pixel's entry
        for i, j in enumerate(sorted({0, len(pads) // 2, len(pads) - 1})):
            ho, wo, kh, kw, hc, wc = pads[j]
            ct, m = (11 + 41 * i) % g["Ct"], i % M
            y = want64.copy()
            y[:, ho, wo, ct] += entry64(g, params, x, ct, kh, kw, m, hc, wc)
            must_leave(y, want64, mag, n_terms, ct, "%s padding tap %r of output %r clamped to pixel %r" % (name, (kh, kw), (ho, wo), (hc, wc)))
    if name.startswith("tg_gap"):                        # a source pixel no window holds, added to the nearest window
        hit = tp.window_hit(g, np.ones((1, g["H"], g["W"], 1), bool))
        assert hit.all()
        Ho, Wo = tp.out_hw(g)
        free = [(h, w) for h in range(g["H"]) for w in range(g["W"])
                if not tp.window_hit(g, np.array([[[[hh == h and ww == w] for ww in range(g["W"])] for hh in range(g["H"])]]))[0].any()]
        assert (2, 2) in free and (0, 2) in free and (2, 0) in free and (0, 0) not in free
        for i, (h, w) in enumerate((free[0], free[len(free) // 2], free[-1])):
            ho, wo = min(h // g["stride"], Ho - 1), min(w // g["stride"], Wo - 1)
            kh, kw = min(h - ho * g["stride"], g["knl"] - 1), min(w - wo * g["stride"], g["knl"] - 1)
            ct, m = (17 + 43 * i) % g["Ct"], i % M
            y = want64.copy()
            y[:, ho, wo, ct] += entry64(g, params, x, ct, kh, kw, m, h, w)
            must_leave(y, want64, mag, n_terms, ct, "%s uncovered pixel %r added to output %r" % (name, (h, w), (ho, wo)))


# ---------------------------------------------------------------- the dense (precise) path ----
def tdiv(a, b):
    """C's integer division: truncation towards zero."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def tap_rows(size, n_out, knl, stride, pad, k, guard):
    """Output rows (columns) tap k reaches under the precise path's rule (src/CaffeEva.cc:1219-1226, C division as written):
    oL = max(0, (pad - k - 1) / s + 1) — the documented lower-bound quirk —, oU = min(n_out - 1, (pad - k + size - 1) / s);
    guard: additionally the source row o s - pad + k must lie inside the map."""
    oL, oU = max(0, tdiv(pad - k - 1, stride) + 1), min(n_out - 1, tdiv(pad - k + size - 1, stride))
    rows = [o for o in range(n_out) if oL <= o <= oU]
    return [o for o in rows if 0 <= o * stride - pad + k < size] if guard else rows


def dense_rule64(g, x, bias, weights):
    """(want64, mag) of the precise path as specified: float64, plain loops; a tap contributes where the reference's im2col rule
    fills it AND its source pixel lies inside the map."""
    x = np.asarray(x, np.float32).astype(np.float64)
    b = np.asarray(bias, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    n, H, W, Cin = x.shape
    knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
    Ho, Wo = tp.out_hw(g)
    Cg, Ctg = Cin // grp, Ct // grp
    want, mag = np.tile(b, (n, Ho, Wo, 1)), np.tile(np.abs(b), (n, Ho, Wo, 1))
    for q in range(grp):
        cts, cin = slice(q * Ctg, (q + 1) * Ctg), slice(q * Cg, (q + 1) * Cg)
        for kh in range(knl):
            for ho in tap_rows(H, Ho, knl, s, pad, kh, True):
                for kw in range(knl):
                    for wo in tap_rows(W, Wo, knl, s, pad, kw, True):
                        px = x[:, ho * s - pad + kh, wo * s - pad + kw, cin]
                        want[:, ho, wo, cts] += px @ w[cts, :, kh, kw].T
                        mag[:, ho, wo, cts] += np.abs(px) @ np.abs(w[cts, :, kh, kw]).T
    return want, mag


def oracle_dense_out(g, dense, x):
    in_chw, layers = layer_of("conv", g)
    orc = po.COracle(in_chw, layers)
    orc.set_dense({0: dense})
    y = orc.run_layer(0, x, x.shape[0])
    orc.close()
    return y


@pytest.mark.parametrize("name", sorted(tp.TINY_DENSE))
def test_oracle_dense_path_follows_the_tap_rule(name):
    """The oracle's precise path (the sequence acc = acc + w * x over (channel, kh, kw), one product and one sum rounding per term)
    within gamma(2 Cin knl^2 + 1) mag of the float64 restatement.  An out-of-map read — another image's pixel, or whatever lies
    behind the buffer — is a whole term of the sum: far outside."""
    g = tp.TINY_DENSE[name]
    in_chw, layers = layer_of("conv", g)
    dense = synth.make_dense_params(in_chw, layers, seed=183)[0]
    x = tp.activations("conv", g, N_REF, seed=184, scaled=False)
    want64, mag = dense_rule64(g, x, dense["bias"], dense["weights"])
    y = oracle_dense_out(g, dense, x)
    n_terms = 2 * g["Cin"] // g["grp"] * g["knl"] ** 2 + 1
    worst = tp.dense_check(y, want64, mag, n_terms, what=name + " oracle, dense path")
    print("%s: oracle dense path worst err / bound %.3f" % (name, worst))
    if name == "tg_1x1_s2":
        # tap 0 lies in the padding; tap 1 (the map's one pixel) is dropped at output 0 by the reference's lower-bound quirk
        # ((pad - kh - 1) / s + 1 = -1 / 2 + 1 = 1); tap 2 is the one the old upper bound let through (-1 / 2 = 0) with source
        # row 1 = H.  Under the rule as specified nothing is left: the output is the bias
        assert tap_rows(1, 1, 3, 2, 1, 2, False) == [0] and tap_rows(1, 1, 3, 2, 1, 2, True) == []
        assert tap_rows(1, 1, 3, 2, 1, 1, True) == [] and tap_rows(1, 1, 3, 2, 1, 0, True) == []
        assert np.array_equal(want64[:, 0, 0, :], np.tile(dense["bias"].astype(np.float64), (N_REF, 1)))
        assert np.array_equal(y[:, 0, 0, :], np.tile(dense["bias"], (N_REF, 1)))
    elif g["stride"] == 1:                               # no quirk at stride 1: the rule is the plain zero-padded convolution
        ref64, _ = ic.dense_layer64("conv", g, x, dense["bias"], dense["weights"])
        assert np.array_equal(ref64, want64)


def test_the_guard_changes_nothing_the_reference_defines():
    """Old rule (bounds alone) and new rule (bounds and source pixel inside the map) name the same output rows for every tap wherever
    pad - k + size - 1 >= 0; they differ only for -stride < pad - k + size - 1 < 0, where the old rule's row 0 reads source row
    `size`: one past the map.  Over size <= 9, knl <= 5, stride <= 4, 0 <= pad < knl."""
    differ = []
    for size, knl, stride in itertools.product(range(1, 10), range(1, 6), range(1, 5)):
        for pad in range(knl):
            if size + 2 * pad < knl:
                continue
            n_out = (size + 2 * pad - knl) // stride + 1
            for k in range(knl):
                old, new = tap_rows(size, n_out, knl, stride, pad, k, False), tap_rows(size, n_out, knl, stride, pad, k, True)
                num = pad - k + size - 1
                if num >= 0:
                    assert old == new, (size, knl, stride, pad, k)
                    assert all(0 <= o * stride - pad + k < size for o in old)
                elif old != new:
                    assert -stride < num < 0 and old == [0] and new == [] and -pad + k >= size
                    differ.append((size, knl, stride, pad, k))
                else:
                    assert old == []
    assert (1, 3, 2, 1, 2) in differ and all(s >= 2 for _, _, s, _, _ in differ)
    print("%d (size, knl, stride, pad, tap) combinations read one past the map under the old rule" % len(differ))
