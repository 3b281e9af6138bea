"""CPU tier of the exact-sum cases (tests/exact_cases.py; tests/test_gpu_exact_sums.py sends them through the kernels).

  * The conditions under which every product, table entry and partial sum is exact in every precision the table kernels keep
    them in are asserted on every case, on the very batch the GPU tier runs: |T| <= 2048 units, |bias| + sum |T| <= 2048 units
    where a case runs with packed fp16 sums (<= 2^24 elsewhere), units inside the fp16 normal range, no more than a quarter of
    an element's entries zero (none is: every code word has an odd coordinate sum), unit exponents -8, 0 and +3 among the cases.
  * exact_expected equals the C oracle's layer output bit for bit in fp32 and in both fp16 study modes (fp16 entries; fp16
    entries and fp16 running sums) — all three are exact on this data: the generator is tied to the reference.
  * One term (kh, kw, m) of one channel removed or doubled changes at least one element of the batch: every m, every tap, eight
    channels spread over the waves and both channel halves of a wave.
  * EXACT_REACH is re-derived: the (channels per wave, tile, channel chunks) of the fp16-table and the fp16-sums launch of every conv
    case and which tiles the map clips, from the launch rules restated in test_panel_cases_cpu.py; family, slice count and stages
    per slice of every FC case at each batch used, from qcnn_plan_fc_query.

Seams the planner cannot emit, so that no case exists for them: k_fc_aprx cuts its sub-space axis in whole stages (mBeg = slice x
stages per slice x G), so a seam never falls inside a stage — the cases have seams after an odd and after an even number of stages
and of sub-spaces instead; G = 1 (K = 128) has no ragged last stage (M % 1 == 0)."""
import functools

import numpy as np
import pytest

import exact_cases as ec
import pyoracle as po
import table_probe as tp
from conftest import pkg
from test_gpu_table_probe import BASE
from test_panel_cases_cpu import plan, sym8_config
from test_planner_cpu import fc_planner, planner          # (fixtures: the CPU planner library's two query entries)
from test_table_probe_cpu import layer_of

capi = pkg("capi")

CONV, FCS = sorted(ec.CONV), sorted(ec.FC)
ALL = CONV + FCS
CONFIG16 = {48: (2, 2), 32: (2, 3), 24: (2, 4), 16: (3, 4)}      # qk_conv_sym8_config16: the tiles of k_conv_sym8<.., MODE = 2>


def f16_sums(name):
    """The case also runs with packed fp16 running sums: the conv shapes with an eight-wave form, k_fc_sym8's shapes."""
    return name in ec.FX or (name in ec.CONV and ec.EXACT_REACH[name] is not None)


@functools.lru_cache(maxsize=None)
def data(name):
    kind, g, M, K, Cs, params, x, e = ec.case(name)
    return kind, g, M, K, Cs, params, x, e, ec.exact_stats(kind, g, x, params)


# ---------------------------------------------------------------- the conditions ----
@pytest.mark.parametrize("name", ALL)
def test_every_intermediate_is_exact(name):
    kind, g, M, K, Cs, params, x, e, st = data(name)
    ec.check_conditions(st, e, f16_sums(name))
    amp = ec.shape_of(name)[5]
    ci = params["ctrd"].astype(np.float64) / 2.0 ** params["e_c"]
    assert np.abs(ci).max() == amp and (ci == np.rint(ci)).all()
    for m, c in enumerate(tp.cs_eff(kind, g, M, Cs)):
        assert (ci[m, :, c:] == 0).all() and (ci[m].sum(-1) % 2 == 1).all()
    assert params["asmt"].max() == K - 1 and params["asmt"].min() == 0 and (params["bias"] != 0).all()
    assert set(np.unique(np.abs(x))) == {2.0 ** params["e_x"]}
    want32 = ec.as_float32(st["want"], e)
    assert np.array_equal(want32.astype(np.float64), st["want"] * 2.0 ** e)                 # the cast to float32 loses nothing
    if f16_sums(name):                                                                      # ... nor would one to fp16
        assert np.array_equal(want32.astype(np.float16).astype(np.float64), st["want"] * 2.0 ** e)
    print("%s: unit 2^%d, |T| <= %d, S_abs <= %d units, %d .. %d terms per element, zero entries %d"
          % (name, e, st["t_max"], st["s_abs"].max(), st["terms"].min(), st["terms"].max(), st["zeros"].max()))


def test_unit_exponents_cover_the_fp16_range():
    for names in (CONV, ec.FX, ec.FA):
        assert {-8, 0, 3} <= {sum(ec.shape_of(n)[6:8]) for n in names}, names
    assert ec.shape_of("pn_s2_5x5")[5] == 1                                                # 400 terms: amp = 1


# ---------------------------------------------------------------- tie to the oracle ----
@pytest.mark.parametrize("name", ALL)
def test_expected_is_the_oracles_output_in_all_three_precisions(name):
    kind, g, M, K, Cs, params, x, e, st = data(name)
    sel = [0, 64, ec.BATCH - 1]
    want = ec.as_float32(st["want"][sel], e)
    in_chw, layers = layer_of(kind, g)
    orc = po.COracle(in_chw, layers)
    orc.set_params({0: params})
    try:
        for mode in ((False, False), (True, False), (True, True)):
            orc.study_mode(*mode)
            y = orc.run_layer(0, x[sel], len(sel)).reshape(want.shape)
            assert np.array_equal(y, want), (name, mode, int((y != want).sum()))
    finally:
        orc.study_mode(False, False)
        orc.close()


# ---------------------------------------------------------------- the check has teeth ----
@pytest.mark.parametrize("name", ALL)
def test_one_missing_or_doubled_term_moves_an_element(name):
    """Term (kh, kw, m) of channel ct is T[pixel][m][asmt[ct][kh][kw][m]] over the batch (0 where the tap lies in the padding).
    Removed from, or added once more to, the integer sum it must change the float32 the test compares with in at least one
    element — for every m, every tap, eight channels."""
    kind, g, M, K, Cs, params, x, e, st = data(name)
    n = 3
    xi = x[:n].astype(np.float64) / 2.0 ** params["e_x"]
    ci = params["ctrd"].astype(np.float64) / 2.0 ** params["e_c"]
    Ct = g["Ct"]
    cts = np.unique([min(Ct - 1, i * Ct // 8 + (i % 2) * max(Ct // 16, 1)) for i in range(8)])
    cse = tp.cs_eff(kind, g, M, Cs)
    want = st["want"][:n]
    checked = 0
    if kind == "fc":
        for m in range(M):
            term = (xi[:, m * Cs:m * Cs + cse[m]] @ ci[m, :, :cse[m]].T)[:, params["asmt"][cts, m]]     # [n, 8]
            for sign in (-1, 1):
                moved = ec.as_float32(want[:, cts] + sign * np.rint(term).astype(np.int64), e) != ec.as_float32(want[:, cts], e)
                assert moved.any(0).all(), (name, m, sign)
            checked += len(cts)
        assert checked == M * len(cts)
        return
    knl, s, pad, grp = g["knl"], g["stride"], g["pad"], g["grp"]
    Ho, Wo = tp.out_hw(g)
    Cg, Ctg = g["Cin"] // grp, Ct // grp
    asmt = params["asmt"].reshape(Ct, knl, knl, M)
    xp = np.zeros((n, g["H"] + 2 * pad, g["W"] + 2 * pad, g["Cin"]))
    xp[:, pad:pad + g["H"], pad:pad + g["W"]] = xi
    for ct in cts:
        for m in range(M):
            c0 = (ct // Ctg) * Cg + m * Cs
            T = xp[..., c0:c0 + cse[m]] @ ci[m, :, :cse[m]].T                                       # [n, Hp, Wp, K]; 0 in the padding
            for kh in range(knl):
                for kw in range(knl):
                    term = T[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, asmt[ct, kh, kw, m]]
                    assert term.any(), (name, ct, kh, kw, m)        # (a changed integer below 2^24 is a changed float32)
                    checked += 1
    assert checked == len(cts) * M * knl * knl and len(cts) == 8


# ---------------------------------------------------------------- what each case reaches ----
F16_OPTS = [dict(BASE, lut=capi.LUT_MFMA_F16, sym8=2), dict(BASE, lut=capi.LUT_MFMA_F16ACC, sym8=2)]


@pytest.mark.parametrize("name", CONV)
def test_conv_reach(name, planner):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    reach = ec.EXACT_REACH[name]
    cf = sym8_config(g["Cin"] // g["grp"], g["Ct"] // g["grp"], M, Cs, K)
    if reach is None:
        # no eight-wave form: the engine asks the planner, which keeps the 16-wave tile kernel, whole (code -1, not -7 / -8);
        # qk_conv_aprx then rounds the entries to fp16 (lutF16) and keeps f32 sums in both modes
        assert cf is None
        for opts in F16_OPTS:
            costs, ch = plan(planner, name, 2, opts)
            assert ch["family"] == -1 and ch["Z"] <= 1 and costs["sym8"] == 0.0, (name, ch)
        return
    Ho, Wo = tp.out_hw(g)
    cpw, th, tw, chunks = cf
    th2, tw2 = CONFIG16[cpw]
    assert reach["mode1"] == (cpw, th, tw, chunks) and reach["mode2"] == (cpw, th2, tw2, chunks), (name, cf)
    assert reach["clip1"] == (Ho % th != 0, Wo % tw != 0) and reach["clip2"] == (Ho % th2 != 0, Wo % tw2 != 0), name
    assert tp.PANEL_REACH[name]["live"]["sym8"][:4] == (cpw, th, tw, chunks)


def test_what_the_conv_cases_are_there_for():
    R = {n: ec.EXACT_REACH[n] for n in CONV if ec.EXACT_REACH[n]}
    S = tp.SHAPES
    assert {r["mode2"][1:3] for r in R.values()} == {(3, 4), (2, 4), (2, 3), (2, 2)}           # the tiles no f32 kernel uses
    assert {r["mode1"][0] for r in R.values()} == {16, 24, 32, 48}                             # all eight instantiations of
    assert {r["mode1"][1:3] for r in R.values()} == {(2, 3), (2, 2), (1, 3), (1, 2)}           # qk_conv_sym8's modes 1 and 2
    assert all(all(r["clip2"]) for r in R.values())                                            # every mode-2 tile clipped in both axes
    assert R["pn_deep"]["mode2"] == (16, 3, 4, 1) and tp.out_hw(S["pn_deep"][1]) == (7, 10)
    assert R["pn_c192"]["mode2"][:3] == (24, 2, 4) and R["pn_c384"]["mode2"][:3] == (48, 2, 2)
    assert R["pn_c256_cs4"]["mode1"][0] == 32 and S["pn_c256_cs4"][4] == 4
    assert R["pn_c512"]["mode1"][3] == 2                                                       # two channel chunks
    assert S["pn_grp2_5x5"][1]["grp"] == 2 and S["pn_s2_5x5"][1]["stride"] == 2
    assert {S[n][4] for n in R} == {4, 8}                                                      # KS = 1 and 2
    assert [n for n in CONV if ec.EXACT_REACH[n] is None] == ["pn_k32_m18", "pn_partial"]


def slices_of(stages, z):
    per = -(-stages // z)
    return per, stages - (z - 1) * per


@pytest.mark.parametrize("name", FCS)
def test_fc_reach(name, fc_planner):
    g, M, K, Cs = ec.FC[name][:4]
    reach = ec.EXACT_REACH[name]
    G = 128 // K if K <= 64 else 1
    assert reach["G"] == (4 if name in ec.FX else G)
    stages = M // 4 if name in ec.FX else -(-M // G)
    sym8 = 2 if name in ec.FX else 0
    geom = [g["D"], g["Ct"], M, K, Cs, 1]
    for key, split, batches in (("plain", 0, ((2, 128), (2, 3), (1, 3), (1, 128))), ("split", 1, ((1, ec.SPLIT_BATCH),))):
        fam, z, per, last = reach[key]
        for panels, live in batches:          # 131 images: two panels, by run_layer whole, in a forward one per stream; 3 alone
            for lut, code in ((1, fam), (2, -7 if fam == -5 else fam), (3, -8 if fam == -5 else fam)):
                assert fc_planner(geom + [panels, live], split=split, sym8=sym8, decode=0, lut=lut) == (code, z), (name, key, lut)
        assert slices_of(stages, z) == (per, last) and (z - 1) * per < stages                  # no case has a slice without a stage
        assert fc_planner(geom + [2, 128], split=split, sym8=sym8, decode=0, lut=0) == (-1, 1)  # the exact builder: one slice
    if name in ec.FA:
        assert M % G != 0 or G == 1
        assert fc_planner(geom + [2, 128], split=0, sym8=2, decode=0, lut=1)[0] == -1          # no eight-wave form


def test_what_the_fc_cases_are_there_for():
    R, F = ec.EXACT_REACH, ec.FC
    # k_fc_sym8: one slice of 1, 2 and an odd number of stages (the stageOf clamp, the padded period); slices of an odd stage count
    # with a shorter last one; a per-launch count under QCNN_OPT_SPLIT that differs from the batch-independent one
    assert [R[n]["plain"][1:] for n in ("fx_s1", "fx_s2", "fx_s5")] == [(1, 1, 1), (1, 2, 2), (1, 5, 5)]
    z, per, last = R["fx_slices"]["plain"][1:]
    assert z > 1 and per % 2 == 1 and last < per and R["fx_slices"]["split"][1] not in (1, z)
    cts = {n: F[n][0]["Ct"] for n in ec.FX}
    assert cts["fx_s1"] == 192 == 2 * 96                                   # two live waves of 96 channels
    assert cts["fx_s2"] % 96 == 50 and 48 < cts["fx_s2"] % 96 < 96         # a half-wave of 48 with two live channels
    assert cts["fx_slices"] == 768 + 194                                   # a second chunk
    assert all(F[n][1] % 4 == 0 and F[n][2] == 32 and F[n][3] == 4 and F[n][0]["D"] == 4 * F[n][1] for n in ec.FX)
    # k_fc_aprx: every stage group with a ragged last stage; the three channel configurations, each with gather waves without a
    # channel; seams after an odd and an even number of stages and of sub-spaces; last slices shorter than the others
    assert sorted(R[n]["G"] for n in ec.FA) == [1, 2, 4, 8, 12] and sorted(F[n][2] for n in ec.FA) == [10, 16, 32, 64, 128]
    for n in ec.FA:
        ct = F[n][0]["Ct"]
        cpw = 32 if ct >= 384 else 8 if ct >= 96 else 4
        assert ct % (12 * cpw) and ct % (12 * cpw) <= 11 * cpw, n          # the last workgroup has a gather wave without a channel
    assert {32 if F[n][0]["Ct"] >= 384 else 8 if F[n][0]["Ct"] >= 96 else 4 for n in ec.FA} == {4, 8, 32}
    pers = [R[n][k][2] for n in ec.FA for k in ("plain", "split")]
    assert any(p % 2 for p in pers) and any(p % 2 == 0 for p in pers)
    assert any((R[n][k][2] * R[n]["G"]) % 2 for n in ec.FA for k in ("plain", "split"))       # a seam after an odd sub-space count
    assert any(R[n][k][3] < R[n][k][2] for n in ec.FA for k in ("plain", "split"))
    # a last slice of a single stage: 170 stages in 14 slices of 13
    g, M, K = F["fa_k128"][:3]
    assert (g["Ct"], M, K) == (2, 170, 128) and R["fa_k128"]["plain"][1:] == (14, 13, 1)
