"""CPU tier of the panel conv cases (tests/test_gpu_panel_cases.py, the pn_* shapes of tests/table_probe.py).

  * Eligibility and launch cut: through qcnn_plan_conv_query (the planner the engine asks), with the option values the GPU tier
    forces a family with, every family PANEL_REACH lists for a shape is the planner's choice at the panel count the GPU tier
    uses, every family listed as not eligible has zero cost, and the split shapes are cut (split-from rank and Z > 1) at one
    panel.  The quantities PANEL_REACH records — channels per wave, tile / strip, tiles per axis, stages of the heaviest tile,
    stage group and ragged last group, channel chunks — are re-derived from qcnn_kernels.h's and qcnn_planner.hip's plain
    functions written again in Python, and every seam a shape exists for (clipped tiles, tile numbering, ring wrap, slice
    boundaries inside a pixel) is asserted from the same rules: a shape that quietly stops reaching its seam fails here.
  * The reference alone meets the bound: the oracle (exact builder: acc = acc + x_j * c_j, entries added in (kh, kw, m) order)
    and a float32 emulation of the MFMA order (a k-ordered fused multiply-add chain per entry, the same (kh, kw, m) order) on
    the shape's random parameters, against table_probe.dense_expected.
  * The check has teeth: ONE (kh, kw, m) term removed from — or added twice to — the float64 sum of one channel leaves the
    bound; the first term, the last one, and one in the ragged last stage group where the shape has one."""
import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_gpu_table_probe import EXACT, HALF8, HALF8S, SLIDE, SPLIT_SYM8, SPLIT_TILE, SYM, SYM8, SYM8S, TILE, code_ok
from test_planner_cpu import COSTS, planner          # (the fixture: qcnn_plan_conv_query of the CPU planner library)
from test_table_probe_cpu import layer_of, oracle_out

synth = pkg("synth")

PANEL = sorted(tp.PANEL_REACH)
FAMS = {"tile": TILE, "slide16": SLIDE, "sym16": SYM, "sym8": SYM8, "sym8_slide": SYM8S, "half8": HALF8, "half8_slide": HALF8S,
        "split_tile": SPLIT_TILE, "split_sym8": SPLIT_SYM8}
LUT_STAGE_BUFFERS, PROGRAM_ROW_BUFFERS = 2, 3      # the stage ring of every panel conv kernel: stage s in LUT buffer s % 2; its program
                                                   # row in row buffer s % 2 (k_conv_aprx, k_conv_sym) / s % 3 (k_conv_sym8, k_conv_half8)
RING = LUT_STAGE_BUFFERS * PROGRAM_ROW_BUFFERS      # a tile with more stages than this has wrapped every ring of every kernel


def plan(planner, name, panels, opts):
    """(costs by family, choice) of shape `name` (or a shape tuple) at `panels` panels under the option dictionary of a family descriptor."""
    kind, g, M, K, Cs, _ = tp.SHAPES[name] if isinstance(name, str) else name
    Ho, Wo = tp.out_hw(g)
    geom = [g["H"], g["W"], g["Cin"], Ho, Wo, g["Ct"], g["knl"], g["stride"], g["pad"], g["grp"], M, Cs, K, panels]
    return planner(geom, **{k: opts[k] for k in ("split", "slide", "sym", "sym8", "half8", "lut")})


# ---------------------------------------------------------------- qcnn_kernels.h / qcnn_planner.hip, written again ----
def stage_group(K):
    return 128 // K if K <= 64 else 1                   # qcnn_stage_group


def pseudo(K):
    return (K + 126) // 127 if K > 128 else 1           # qcnn_model_set_layer_shape: pseudo sub-spaces per sub-space


def conv_slots(Ctg):
    """qk_conv_slots: (channels per gather wave, channel chunks per group) of the 16-wave tile kernel."""
    chunks = (Ctg + 383) // 384
    per = -(-Ctg // chunks)
    cpw = 4 if per <= 48 else 6 if per <= 72 else 8 if per <= 96 else 12 if per <= 144 else 16 if per <= 192 else 24 if per <= 288 else 32
    return cpw, -(-Ctg // (12 * cpw))


CONV_TILE = {32: (1, 1), 24: (1, 1), 16: (1, 2), 12: (1, 3), 8: (2, 2), 6: (2, 3), 4: (2, 4)}     # qk_conv_tile


def slide_config(Ctg, knl, stride):
    """qk_slide_config: (channels per wave, slots, columns per strip, channel chunks) or None."""
    ns = -(-knl // stride)
    if ns < 2 or ns > 5:
        return None
    for c in (16, 12, 8, 6, 4):
        built = (ns == 2 and c >= 8) or (ns == 3 and c <= 12) or (ns == 4 and c == 8) or (ns == 5 and c <= 6)
        if c <= conv_slots(Ctg)[0] and ns * c <= 36 and built:
            return c, ns, 2 if ns == 3 and c <= 6 else 1, -(-Ctg // (12 * c))
    return None


def complete(Cg, M, Cs, K):
    return K == 128 and Cs in (4, 8) and Cg % Cs == 0 and M == Cg // Cs


def sym8_config(Cg, Ctg, M, Cs, K):
    """qk_conv_sym8_config: (cpw, th, tw, chunks) or None."""
    if not complete(Cg, M, Cs, K):
        return None
    chunks = (Ctg + 383) // 384
    per = -(-Ctg // chunks)
    if per <= 64:
        return None
    cpw, th, tw = (16, 2, 3) if per <= 128 else (24, 2, 2) if per <= 192 else (32, 1, 3) if per <= 256 else (48, 1, 2)
    return None if Ctg % cpw else (cpw, th, tw, -(-Ctg // (8 * cpw)))


def sym8_slide_config(Cg, Ctg, M, Cs, K, knl, stride):
    """qk_conv_sym8_slide_config: (cpw, slots, columns per strip, chunks) or None."""
    if not complete(Cg, M, Cs, K):
        return None
    ns = -(-knl // stride)
    chunks = (Ctg + 255) // 256
    per = -(-Ctg // chunks)
    if ns == 3:
        if per <= 64:
            return None
        cpw, nc = (16, 2) if per <= 128 else (24, 1) if per <= 192 else (32, 1)
    elif ns == 5:
        if per <= 64 or per > 128:
            return None
        cpw, nc = 16, 1
    else:
        return None
    return None if Ctg % cpw else (cpw, ns, nc, -(-Ctg // (8 * cpw)))


HALF8_CASES = {128: (32, 3, 4, 2), 192: (48, 2, 4, 2), 256: (32, 2, 3, 1), 384: (48, 2, 2, 1), 512: (64, 1, 3, 1)}
HALF8_SLIDE_COLS = {128: 4, 192: 2, 256: 2, 384: 1, 512: 1}


def half8_config(Cg, Ctg, M, Cs, K):
    """qk_conv_half8_config: (cpw, th, tw, wave sets, chunks) or None."""
    if not complete(Cg, M, Cs, K):
        return None
    chunks = (Ctg + 511) // 512
    if Ctg % chunks or Ctg // chunks not in HALF8_CASES:
        return None
    return HALF8_CASES[Ctg // chunks] + (chunks,)


def half8_slide_config(Cg, Ctg, M, Cs, K, knl, stride):
    """qk_conv_half8_slide_config: (cpw, slots, columns per strip, wave sets, chunks) or None."""
    cf = half8_config(Cg, Ctg, M, Cs, K)
    if cf is None or -(-knl // stride) != 3:
        return None
    return (cf[0], 3, HALF8_SLIDE_COLS[Ctg // cf[4]], cf[3], cf[4])


def tile_of_rank(r, tilesY, tilesX):
    if tilesY < 3 or tilesX < 3:
        return r // tilesX, r % tilesX
    iy, ix = tilesY - 2, tilesX - 2
    if r < iy * ix:
        return 1 + r // ix, 1 + r % ix
    r -= iy * ix
    if r < ix:
        return 0, 1 + r
    r -= ix
    if r < ix:
        return tilesY - 1, 1 + r
    r -= ix
    if r < iy:
        return 1 + r, 0
    r -= iy
    if r < iy:
        return 1 + r, tilesX - 1
    r -= iy
    return (tilesY - 1 if r >> 1 else 0), (tilesX - 1 if r & 1 else 0)


def span(g, o0, oL, size):
    """Source rows (columns) the output rows (columns) o0 .. oL look at, clipped to the map."""
    return max(min(size - 1, oL * g["stride"] - g["pad"] + g["knl"] - 1) - max(0, o0 * g["stride"] - g["pad"]) + 1, 0)


def tile_pixels(g, r, tilesY, tilesX, th, tw):
    Ho, Wo = tp.out_hw(g)
    ty, tx = tile_of_rank(r, tilesY, tilesX)
    return span(g, ty * th, min(ty * th + th, Ho) - 1, g["H"]) * span(g, tx * tw, min(tx * tw + tw, Wo) - 1, g["W"])


def tile_stages(g, th, tw, per_pixel):
    """(tiles per axis (y, x), stages of every tile in rank order)."""
    Ho, Wo = tp.out_hw(g)
    tilesY, tilesX = -(-Ho // th), -(-Wo // tw)
    return (tilesY, tilesX), [tile_pixels(g, r, tilesY, tilesX, th, tw) * per_pixel for r in range(tilesY * tilesX)]


def derive(name):
    """What the launchers choose for a pn_* shape, family by family, in the layout of table_probe.PANEL_REACH:
       tile / sym16 / sym8 / half8:   (cpw, th, tw[, wave sets], channel chunks per group, (tilesY, tilesX), stages of the heaviest tile)
       slide16 / sym8_slide / half8_slide: (cpw, slots, columns per strip[, wave sets], chunks, strips, stages of a whole-column strip)
    and G, the sub-spaces of a pixel's last stage, the stages per source pixel (pseudo sub-spaces counted).  `name`: a key of
    table_probe.SHAPES or a shape tuple."""
    kind, g, M, K, Cs, _ = tp.SHAPES[name] if isinstance(name, str) else name
    Cg, Ctg = g["Cin"] // g["grp"], g["Ct"] // g["grp"]
    P = pseudo(K)
    Mk, Kk = M * P, (128 if P > 1 else K)               # as the kernels see the layer
    G = stage_group(Kk)
    MG = -(-Mk // G)
    Ho, Wo = tp.out_hw(g)
    out = dict(G=G, last_group=Mk - (MG - 1) * G, per_pixel=MG)
    cpw, chunks = conv_slots(Ctg)
    th, tw = CONV_TILE[cpw]
    tiles, st = tile_stages(g, th, tw, MG)
    out["tile"] = (cpw, th, tw, chunks, tiles, max(st))

    if P == 1 and Kk == 128 and Ho >= 2 * -(-g["knl"] // g["stride"]):
        sc = slide_config(Ctg, g["knl"], g["stride"])
        if sc:
            out["slide16"] = sc + (-(-Wo // sc[2]), g["H"] * max(span(g, c, min(c + sc[2], Wo) - 1, g["W"]) for c in range(0, Wo, sc[2])) * MG)
    if P == 1 and Ctg == 128 and complete(Cg, M, Cs, K):
        tiles, st = tile_stages(g, 2, 2, M)
        out["sym16"] = (8, 2, 2, 1, tiles, max(st))
    if P == 1:
        c8 = sym8_config(Cg, Ctg, M, Cs, K)
        if c8:
            tiles, st = tile_stages(g, c8[1], c8[2], M)
            out["sym8"] = c8 + (tiles, max(st))
        c8s = sym8_slide_config(Cg, Ctg, M, Cs, K, g["knl"], g["stride"])
        if c8s and Ho >= 2 * c8s[1]:
            out["sym8_slide"] = c8s + (-(-Wo // c8s[2]), g["H"] * max(span(g, c, min(c + c8s[2], Wo) - 1, g["W"]) for c in range(0, Wo, c8s[2])) * M)
        ch = half8_config(Cg, Ctg, M, Cs, K)
        if ch:
            tiles, st = tile_stages(g, ch[1], ch[2], M)
            out["half8"] = ch + (tiles, max(st))
        chs = half8_slide_config(Cg, Ctg, M, Cs, K, g["knl"], g["stride"])
        if chs and Ho >= 2 * chs[1]:
            out["half8_slide"] = chs + (-(-Wo // chs[2]), g["H"] * max(span(g, c, min(c + chs[2], Wo) - 1, g["W"]) for c in range(0, Wo, chs[2])) * M)
    return out


def slice_starts(stages, Z):
    return [stages * z // Z for z in range(1, Z)]       # sBeg of slices 1 .. Z - 1 (k_conv_aprx, k_conv_sym8)


# ---------------------------------------------------------------- eligibility and launch cut ----
@pytest.mark.parametrize("name", PANEL)
def test_every_listed_family_is_live_and_cut_as_recorded(name, planner):
    reach = tp.PANEL_REACH[name]
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    assert g["knl"] ** 2 * M <= 1200                                                  # one missing term >= 2^24 / 1200^2 = 11.6 bounds
    d = derive(name)
    assert (d["G"], d["last_group"], d["per_pixel"]) == reach["stage"], (name, d)
    whole = [k for k in reach["live"] if not k.startswith("split_")]
    for k in whole:
        assert d.get(k) == reach["live"][k], (name, k, d.get(k))
    assert sorted(k for k in COSTS if k in d) == sorted(whole), (name, sorted(d))      # ... and no family beyond the listed ones
    assert set(reach["dead"]) == set(COSTS) - set(whole)
    if pseudo(K) > 1:                      # the engine hands pseudo sub-spaces to the exact-builder tile kernel in front of the planner
        assert whole == ["tile"] and not [k for k in reach["live"] if k.startswith("split_")]
        return
    for k in whole:                        # two panels: the batch of 131 images
        costs, ch = plan(planner, name, 2, FAMS[k]["opts"])
        assert costs[k] > 0.0, (name, k, costs)
        assert code_ok(FAMS[k]["code"], (ch["family"], len(ch["segs"]) - 1 if ch["segs"] else ch["Z"])), (name, k, ch)
        assert ch["family"] != -1 or ch["Z"] <= 1                                      # (split = 0: whole tiles)
        if "slide" in k:                   # every segment holds whole slots' worth of rows and wraps the ring
            ns = d[k][1]
            assert len(ch["segs"]) >= 2 and all(b - a >= 1 for a, b in zip(ch["segs"], ch["segs"][1:])), (name, k, ch)
            assert ch["segs"][0] == 0 and ch["segs"][-1] == tp.out_hw(g)[0] >= 2 * ns
    everything_on = dict(TILE["opts"], split=1, slide=1, sym=1, sym8=1, half8=1)
    costs, _ = plan(planner, name, 2, everything_on)
    for k in reach["dead"]:
        assert costs[k] == 0.0, (name, k, costs)
    costs0, ch0 = plan(planner, name, 2, EXACT["opts"])                                       # the exact builder: the tile kernel, whole
    assert ch0["family"] == -1 and ch0["Z"] <= 1
    for k in (k for k in reach["live"] if k.startswith("split_")):                      # one panel: the batch of 125 images
        costs, ch = plan(planner, name, 1, FAMS[k]["opts"])
        Z, frm = reach["live"][k]
        if k == "split_tile":
            assert ch["family"] == -1 and (ch["Z"], ch["split_from"]) == (Z, frm) and Z > 1, (name, ch)
            assert code_ok(SPLIT_TILE["code"], (ch["split_from"], ch["Z"]))
        else:
            assert ch["family"] == -5 and ch["Z"] == Z > 1 and frm == 0, (name, ch)
            assert code_ok(SPLIT_SYM8["code"], (ch["family"], ch["Z"]))


def test_what_each_shape_is_there_for(planner):
    """The seams in words, from the same rules."""
    D = {n: derive(n) for n in PANEL}
    S = tp.SHAPES
    # every family, both split forms, a deep axis of complete 4-dim sub-spaces: 128 channels per group is the only symmetric shape
    assert set(tp.PANEL_REACH["pn_deep"]["live"]) == set(FAMS) and S["pn_deep"][2:5] == (32, 128, 4)
    assert D["pn_deep"]["sym8"][:3] == (16, 2, 3) and D["pn_deep"]["half8"][:4] == (32, 3, 4, 2) and D["pn_deep"]["sym8_slide"][2] == 2
    # every channel configuration of the eight-wave and half-panel kernels: cpw 16 / 24 / 32 / 48, two chunks at 512; cases 128 .. 512
    by_ctg = {S[n][1]["Ct"] // S[n][1]["grp"]: n for n in ("pn_deep", "pn_c192", "pn_c256_cs4", "pn_c384", "pn_c512")}
    assert sorted(by_ctg) == [128, 192, 256, 384, 512]
    assert [D[by_ctg[c]]["sym8"][0] for c in sorted(by_ctg)] == [16, 24, 32, 48, 32] and D["pn_c512"]["sym8"][3] == 2
    assert [D[by_ctg[c]]["half8"][:4] for c in sorted(by_ctg)] == [HALF8_CASES[c] for c in sorted(by_ctg)]
    assert [D[by_ctg[c]]["half8_slide"][2] for c in sorted(by_ctg)] == [4, 2, 2, 1, 1]
    assert [D[by_ctg[c]]["sym8_slide"][0] for c in sorted(by_ctg)] == [16, 24, 32, 24, 32]
    assert {S[n][4] for n in by_ctg.values()} == {4, 8} and all(S[n][2] in (8, 16, 32) for n in by_ctg.values())
    # groups: five slots — the sliding forms of the 16-wave and the eight-wave kernel, no half-panel sliding form
    g = S["pn_grp2_5x5"][1]
    assert g["grp"] == 2 and D["pn_grp2_5x5"]["slide16"][1] == 5 and D["pn_grp2_5x5"]["sym8_slide"][:3] == (16, 5, 1)
    assert "half8_slide" not in D["pn_grp2_5x5"] and "sym16" in D["pn_grp2_5x5"]
    # stride 2 on an odd map: three slots, every sliding form; the last two-column strip of the eight-wave form holds one column
    g = S["pn_s2_5x5"][1]
    assert g["stride"] == 2 and g["H"] % 2 and g["W"] % 2 and tp.out_hw(g) == (7, 5)
    assert all(D["pn_s2_5x5"][k][1] == 3 for k in ("slide16", "sym8_slide", "half8_slide")) and D["pn_s2_5x5"]["sym8_slide"][2] == 2
    # stage groups with a ragged last stage of every pixel; only the 16-wave tile kernel takes K < 128 (no sliding program is built)
    for n, G, last in (("pn_k32_m18", 4, 2), ("pn_k10_m32", 12, 8), ("pn_k64_m9", 2, 1)):
        assert (D[n]["G"], D[n]["last_group"]) == (G, last) and S[n][2] % G == last and set(tp.PANEL_REACH[n]["live"]) == {"tile", "split_tile"}
    # an incomplete last sub-space: no eight-wave / symmetric family
    assert tp.cs_eff(*S["pn_partial"][:2], 9, 8)[-1] == 4 and set(tp.PANEL_REACH["pn_partial"]["live"]) == {"tile", "slide16", "split_tile"}
    assert D["pn_partial"]["slide16"][:3] == (6, 3, 2)                                 # ... and the two-column strips of the 16-wave form
    # more than 128 code words: two and three pseudo sub-spaces per sub-space
    assert (pseudo(200), pseudo(256)) == (2, 3) and D["pn_k200"]["per_pixel"] == 32 and D["pn_k256"]["per_pixel"] == 48
    # tile edges: for every tile family and every tile shape it uses, a clipped last tile along each axis the tile is longer than 1 in
    clipped = {}
    for n in PANEL:
        Ho, Wo = tp.out_hw(S[n][1])
        for k in ("tile", "sym16", "sym8", "half8"):
            if k in D[n]:
                th, tw = D[n][k][1:3]
                c = clipped.setdefault((k, th, tw), [False, False])
                c[0] |= Ho % th != 0
                c[1] |= Wo % tw != 0
        for k in ("slide16", "sym8_slide", "half8_slide"):
            if k in D[n]:
                clipped.setdefault((k, D[n][k][2]), [True, False])[1] |= Wo % D[n][k][2] != 0
    assert {k[1:] for k in clipped if k[0] == "tile"} == set(CONV_TILE.values())          # every tile of k_conv_aprx
    assert {k[1:] for k in clipped if k[0] == "sym8"} == {(2, 3), (2, 2), (1, 3), (1, 2)}    # ... of k_conv_sym8
    assert {k[1:] for k in clipped if k[0] == "half8"} == {v[1:3] for v in HALF8_CASES.values()}
    assert {k[1] for k in clipped if k[0] == "slide16"} == {1, 2} == {k[1] for k in clipped if k[0] == "sym8_slide"}
    assert {k[1] for k in clipped if k[0] == "half8_slide"} == {1, 2, 4}
    for key, (cy, cx) in clipped.items():
        if key[0] in ("tile", "sym16", "sym8", "half8"):
            assert (cy or key[1] == 1) and (cx or key[2] == 1), key
        else:
            assert cx or key[1] == 1, key
    # tile numbering: interior / edge / corner ranks (>= 3 tiles in both axes) and the row-major fall-back, for each tile family
    for k in ("tile", "sym8", "half8"):
        grids = [D[n][k][-2] for n in PANEL if k in D[n]]
        assert any(min(t) >= 3 for t in grids) and any(min(t) < 3 for t in grids), (k, grids)
    assert any(min(D[n]["sym16"][-2]) >= 3 for n in PANEL if "sym16" in D[n])
    # stage ring: every family's heaviest work item, on every shape, has more stages than all rings together
    for n in PANEL:
        for k in COSTS:
            if k in D[n]:
                assert D[n][k][-1] > 4 * RING, (n, k, D[n][k])
    # split seams: a slice boundary strictly inside a pixel's stage sequence, and a slice count that does not divide the stages
    inside = {"split_tile": 0, "split_sym8": 0}
    ragged = {"split_tile": 0, "split_sym8": 0}
    for n in PANEL:
        g = S[n][1]
        for k in ("split_tile", "split_sym8"):
            if k not in tp.PANEL_REACH[n]["live"]:
                continue
            Z, frm = tp.PANEL_REACH[n]["live"][k]
            base = D[n]["tile" if k == "split_tile" else "sym8"]
            per_pixel = D[n]["per_pixel"]
            _, st = tile_stages(g, base[1], base[2], per_pixel)
            assert max(st[frm:]) // Z > RING                                            # the slices of the heaviest tile wrap the rings too
            for s in st[frm:]:
                inside[k] += any(b % per_pixel for b in slice_starts(s, Z))
                ragged[k] += s % Z != 0
    assert min(inside.values()) > 0 and min(ragged.values()) > 0, (inside, ragged)
    # ... and for the stage-group shapes a boundary inside a pixel means: between two stage groups of one pixel
    for n in ("pn_k32_m18", "pn_k10_m32", "pn_k64_m9"):
        Z, frm = tp.PANEL_REACH[n]["live"]["split_tile"]
        _, st = tile_stages(S[n][1], *D[n]["tile"][1:3], D[n]["per_pixel"])
        assert any(b % D[n]["per_pixel"] for s in st[frm:] for b in slice_starts(s, Z)), n


# ---------------------------------------------------------------- the reference alone stays inside the bound ----
def dense_case(name, seed=81, n=3):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    in_chw, layers = layer_of(kind, g)
    spec = synth.quant_spec(in_chw, layers)
    spec[0] = dict(spec[0], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=seed, spec=spec)[0]
    x = tp.activations(kind, g, n, seed=seed + 1, scaled=False)
    return g, M, Cs, params, x


def fma32(acc, a, b):
    """float32 fused multiply-add: the product is exact in float64, the sum rounded to float64 and then to float32 (the second
    rounding differs from a single one only on a float64 tie pattern; either result is inside the bound's one rounding per step
    up to 2^-53)."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def mfma_order_out(g, params, x):
    """The layer as the MFMA builders and the gather waves compute it, in float32: an entry is the chain acc = fma(x_j, c_j, acc)
    from 0 over the dims of its sub-space in ascending order (v_mfma_f32_16x16x4_f32, k-steps chained through the accumulator);
    an output is the bias plus its entries added one by one in (kh, kw, m) order, taps in the padding skipped."""
    x = np.asarray(x, np.float32)
    ctrd, asmt = np.asarray(params["ctrd"], np.float32), np.asarray(params["asmt"]).astype(np.int64)
    M, K, Cs = ctrd.shape
    n, H, W, Cin = x.shape
    knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
    Ho, Wo = tp.out_hw(g)
    Cg, Ctg = Cin // grp, Ct // grp
    cse = tp.cs_eff("conv", g, M, Cs)
    asmt = asmt.reshape(Ct, knl, knl, M)
    y = np.tile(np.asarray(params["bias"], np.float32), (n, Ho, Wo, 1))
    for gi in range(grp):
        cts = slice(gi * Ctg, (gi + 1) * Ctg)
        T = []
        for m in range(M):
            acc = np.zeros((n, H, W, K), np.float32)
            for j in range(cse[m]):
                acc = fma32(acc, x[..., gi * Cg + m * Cs + j, None], ctrd[m, :, j])
            T.append(acc)
        for kh in range(knl):
            ho = [o for o in range(Ho) if 0 <= o * s - pad + kh < H]
            for kw in range(knl):
                wo = [o for o in range(Wo) if 0 <= o * s - pad + kw < W]
                if not ho or not wo:
                    continue
                hi = np.array(ho)[:, None] * s - pad + kh
                wi = np.array(wo)[None, :] * s - pad + kw
                for m in range(M):
                    y[:, ho[0]:ho[-1] + 1, wo[0]:wo[-1] + 1, cts] += T[m][:, hi, wi][..., asmt[cts, kh, kw, m]]
    return y


@pytest.mark.parametrize("name", PANEL)
def test_references_stay_inside_the_dense_sum_bound(name):
    g, M, Cs, params, x = dense_case(name)
    want64, mag = tp.dense_expected("conv", g, x, params)
    n_terms = tp.dense_count("conv", g, M, Cs)
    exact = tp.dense_check(oracle_out("conv", g, params, x), want64, mag, n_terms, what=name + " exact builder")
    mfma = tp.dense_check(mfma_order_out(g, params, x), want64, mag, n_terms, what=name + " MFMA order")
    print("%s: worst err / bound: oracle (exact builder) %.3f, MFMA order %.3f" % (name, exact, mfma))
    assert exact <= 1.0 and mfma <= 1.0


# ---------------------------------------------------------------- the check has teeth ----
def one_term(g, params, x, ct, kh, kw, m):
    """The float64 contribution of term (kh, kw, m) to channel ct: [n, Ho, Wo], 0 where the tap lies in the padding."""
    x = np.asarray(x, np.float32).astype(np.float64)
    M, K, Cs = params["ctrd"].shape
    n, H, W, Cin = x.shape
    knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
    Ho, Wo = tp.out_hw(g)
    cse = tp.cs_eff("conv", g, M, Cs)[m]
    c0 = (ct // (Ct // grp)) * (Cin // grp) + m * Cs
    word = np.asarray(params["ctrd"], np.float32)[m, int(np.asarray(params["asmt"]).reshape(Ct, knl, knl, M)[ct, kh, kw, m]), :cse].astype(np.float64)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    return xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, c0:c0 + cse] @ word


@pytest.mark.parametrize("name", PANEL)
def test_one_missing_or_doubled_term_leaves_the_bound(name):
    """The float64 sum itself, rounded once to float32, with ONE term of one channel removed or added twice: the checker raises;
    untouched it passes.  Terms: the first, the last, and the first sub-space of the ragged last stage group."""
    g, M, Cs, params, x = dense_case(name)
    want64, mag = tp.dense_expected("conv", g, x, params)
    n_terms = tp.dense_count("conv", g, M, Cs)
    assert tp.dense_check(want64.astype(np.float32), want64, mag, n_terms) <= 1.0
    d = derive(name)
    knl = g["knl"]
    terms = [(0, 0, 0), (knl - 1, knl - 1, M - 1)]
    if d["G"] > 1 and d["last_group"] < d["G"]:
        terms.append((knl // 2, knl // 2, (d["per_pixel"] - 1) * d["G"]))
    else:
        terms.append((knl // 2, knl // 2, M // 2))
    for i, (kh, kw, m) in enumerate(terms):
        ct = (5 + 37 * i) % g["Ct"]
        t = one_term(g, params, x, ct, kh, kw, m)
        assert (t != 0).mean() > 0.3
        for sign, what in ((-1.0, "missing"), (1.0, "doubled")):
            y = want64.copy()
            y[..., ct] += sign * t
            with pytest.raises(AssertionError, match="beyond the bound"):
                tp.dense_check(y.astype(np.float32), want64, mag, n_terms, what="%s %s term %r" % (name, what, (kh, kw, m)))
            others = np.arange(g["Ct"]) != ct
            assert tp.dense_check(y.astype(np.float32)[..., others], want64[..., others], mag[..., others], n_terms) <= 1.0
