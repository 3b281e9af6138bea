"""CPU tier of the few-image kernel cases (tests/test_gpu_small_cases.py, the sm_* / fc_* shapes of tests/table_probe.py).

  * The tile / chunk choice of the launchers (qk_conv_small, qk_fc_small in quantized-cnn_amd/csrc/qcnn_small.hip) is restated in
    Python, with the LDS budgets read out of the source file, and every shape is held to the branch it is there to reach: a
    changed CONV_LDS / LUT_BYTES fails here instead of letting a GPU case pass vacuously.
  * The reference alone stays inside the dense-sum bound: pyoracle.COracle (the exact sequence acc = acc + x_j * c_j per entry,
    entries added in (kh, kw, m) order) on every shape against table_probe.dense_expected.
  * The dense-sum checker trips on ONE look-up that reads a neighbouring table entry."""
import os
import re

import numpy as np
import pytest

import table_probe as tp
from conftest import ROOT, pkg
from test_table_probe_cpu import layer_of, oracle_out

synth = pkg("synth")

SMALL = sorted(tp.SMALL_REACH)
LDS_PER_WORKGROUP = 160 * 1024          # gfx950


def constants():
    src = open(os.path.join(ROOT, "quantized-cnn_amd", "csrc", "qcnn_small.hip")).read()
    out = {}
    for name in ("NT", "LUT_BYTES", "CONV_LDS"):
        m = re.search(r"constexpr int %s = (\d+)(?: \* (\d+))?;" % name, src)
        assert m, name
        out[name] = int(m.group(1)) * int(m.group(2) or 1)
    return out


def stage_group(K):
    return 128 // K if K <= 64 else 1        # qcnn_stage_group


def conv_small_plan(g, M, K, Cs, c):
    """qk_conv_small's choice: dict(TH, TW, MC, CH, chunks, lds) or None where it returns hipErrorInvalidValue."""
    Ho, Wo = tp.out_hw(g)
    Ctg = g["Ct"] // g["grp"]
    CH = min(128, (Ctg + 31) // 32 * 32)
    slots = c["NT"] // CH
    rf = lambda a: (a - 1) * g["stride"] + g["knl"]
    mc_for = lambda a, b: c["CONV_LDS"] // (rf(a) * rf(b) * (K + Cs) * 4 + g["knl"] ** 2 * CH)
    th, tw = min(2, Ho), min(2, Wo)
    while (mc_for(th, tw) < min(M, 4) or th * tw > 4 * slots) and (th > 1 or tw > 1):
        if tw >= th and tw > 1:
            tw -= 1
        else:
            th -= 1
    if mc_for(th, tw) < 1:
        return None
    MC = min(M, mc_for(th, tw))
    lds = rf(th) * rf(tw) * MC * (K + Cs) * 4 + g["knl"] ** 2 * MC * CH
    return dict(TH=th, TW=tw, MC=MC, CH=CH, chunks=-(-Ctg // CH), lds=lds)


def chunks_of(M, MC):
    return [min(MC, M - m0) for m0 in range(0, M, MC)]


@pytest.mark.parametrize("name", SMALL)
def test_launcher_choice_reaches_the_branch(name):
    c = constants()
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    if kind == "fc":
        MC = min(M, c["LUT_BYTES"] // (K * 4))
        assert K % 4 == 0 and (MC, stage_group(K)) == tp.SMALL_REACH[name]
        assert MC * K * 4 <= c["LUT_BYTES"] <= LDS_PER_WORKGROUP and c["NT"] * 4 <= c["LUT_BYTES"]
        assert len(chunks_of(M, MC)) == (1 if name == "fc_k20" else 2)
        return
    p = conv_small_plan(g, M, K, Cs, c)
    assert p is not None
    assert (p["TH"], p["TW"], p["MC"], p["CH"], p["chunks"], stage_group(K)) == tp.SMALL_REACH[name]
    assert p["lds"] <= LDS_PER_WORKGROUP and c["NT"] // p["CH"] * 4 >= p["TH"] * p["TW"]


def test_what_each_case_is_there_for():
    """The property in words, per shape, from the same rules."""
    c = constants()
    plan = {n: conv_small_plan(*tp.SHAPES[n][1:5], c) for n in SMALL if tp.SHAPES[n][0] == "conv"}
    M = {n: tp.SHAPES[n][2] for n in SMALL}
    K = {n: tp.SHAPES[n][3] for n in SMALL}
    assert chunks_of(M["sm_m18"], plan["sm_m18"]["MC"]) == [17, 1] and tp.cs_eff(*tp.SHAPES["sm_m18"][:2], 18, 4)[-1] == 2
    assert chunks_of(M["sm_5x5_m12"], plan["sm_5x5_m12"]["MC"]) == [7, 5]
    assert tp.out_hw(tp.SHAPES["sm_5x5_m12"][1]) == (9, 9)                          # odd map under 2x2 tiles
    assert chunks_of(M["sm_k32_m24"], plan["sm_k32_m24"]["MC"]) == [19, 5] and 19 % stage_group(32) == 3
    for n, G in (("sm_k40", 3), ("sm_k24", 5), ("sm_k10_m6", 12)):                  # no power of two, and a sub-space whose
        assert stage_group(K[n]) == G and G & (G - 1) and plan[n]["MC"] == M[n] > 1  # m % G differs from m & (G - 1)
        assert any(m % G != m & (G - 1) for m in range(M[n]))
    assert K["sm_k40"] % 16 and M["sm_k40"] * K["sm_k40"] < c["NT"]                 # scalar build, pixels dealt out to thread groups
    assert K["sm_k100_m6"] % 16 and M["sm_k100_m6"] * K["sm_k100_m6"] >= c["NT"] and stage_group(100) == 1
    g = tp.SHAPES["sm_ct400_g2"][1]
    assert g["grp"] == 2 and plan["sm_ct400_g2"]["chunks"] == 2 and g["Ct"] // 2 - plan["sm_ct400_g2"]["CH"] == 72
    assert g["stride"] == 2 and g["H"] != g["W"] and tp.out_hw(g) == (4, 3)
    g = tp.SHAPES["sm_ct24"][1]
    assert plan["sm_ct24"]["CH"] - g["Ct"] == 8 and c["NT"] // plan["sm_ct24"]["CH"] == 16 and g["stride"] > g["knl"] == 1
    for n in ("sm_15_m2", "sm_15_k64"):                                             # one sub-space per chunk with M = 2: the mc == 1
        assert plan[n]["MC"] == 1 and M[n] == 2                                      # gather runs at m0 = 1
    assert 1 % stage_group(K["sm_15_k64"]) == 1
    g = tp.SHAPES["sm_nchw_m2"][1]
    assert g["Cin"] <= 4 and M["sm_nchw_m2"] == 2
    assert chunks_of(900, 896) == [896, 4] and tp.SHAPES["fc_m900"][1]["Ct"] % 16
    assert chunks_of(230, 224) == [224, 6] and chunks_of(1800, 1792) == [1792, 8]


def test_the_fall_through_shape_and_the_15x15_window():
    """17x17 taps with K = 128 do not fit the few-image kernel's LDS table at any tile (the panel kernels take the layer);
    the 15x15 first layer of test_few_image_batches_fall_back_to_the_panel_kernels_where_needed does, at a 2x2 tile."""
    c = constants()
    kind, g, M, K, Cs, _ = tp.SMALL_FALL_THROUGH
    assert conv_small_plan(g, M, K, Cs, c) is None
    assert 289 * (128 + 8) * 4 + 289 * 32 > c["CONV_LDS"]
    p = conv_small_plan(tp.conv_geom(20, 20, 3, 15, 1, 0, 1, 16), 1, 128, 8, c)
    assert p is not None and (p["TH"], p["TW"], p["MC"]) == (2, 2, 1) and p["lds"] == 256 * 136 * 4 + 225 * 32 <= c["CONV_LDS"]


# ---------------------------------------------------------------- the reference alone stays inside the bound ----
def dense_case(name, seed=61, n=3):
    kind, g, M, K, Cs, _ = tp.SMALL_FALL_THROUGH if name == "fall_through" else tp.SHAPES[name]
    in_chw, layers = layer_of(kind, g)
    spec = synth.quant_spec(in_chw, layers)
    spec[0] = dict(spec[0], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=seed, spec=spec)[0]
    x = tp.activations(kind, g, n, seed=seed + 1, scaled=False)
    return kind, g, M, Cs, params, x


@pytest.mark.parametrize("name", SMALL + ["fall_through"])
def test_oracle_stays_inside_the_dense_sum_bound(name):
    kind, g, M, Cs, params, x = dense_case(name)
    want64, mag = tp.dense_expected(kind, g, x, params)
    y = oracle_out(kind, g, params, x)
    worst = tp.dense_check(y, want64, mag, tp.dense_count(kind, g, M, Cs), what=name)
    print("%s: oracle worst err / bound %.3f" % (name, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", ["sm_k40", "sm_k32_m24", "fc_m900"])
def test_dense_sum_checker_trips_on_one_wrong_look_up(name):
    """ONE look-up of one output channel reads the neighbouring code word's entry: every output of that channel the tap reaches
    leaves the bound, every other output stays inside."""
    kind, g, M, Cs, params, x = dense_case(name)
    want64, mag = tp.dense_expected(kind, g, x, params)
    n_terms = tp.dense_count(kind, g, M, Cs)
    asmt = params["asmt"].copy()
    a = asmt.reshape(asmt.shape[0], -1, M)                                          # [Ct][taps][M]
    ct, tap, m = 5, a.shape[1] // 2, M - 1
    a[ct, tap, m] = (int(a[ct, tap, m]) + 1) % params["ctrd"].shape[1]
    y = oracle_out(kind, g, dict(params, asmt=asmt), x)
    with pytest.raises(AssertionError, match="beyond the bound"):
        tp.dense_check(y, want64, mag, n_terms, what=name)
    others = np.arange(y.shape[-1]) != ct
    assert tp.dense_check(y[..., others], want64[..., others], mag[..., others], n_terms) <= 1.0
