"""The launch planner on the CPU (quantized-cnn_amd/csrc/qcnn_planner.{h,hip}: host code, built by g++ into
build/libqcnn_planner_cpu.so — the same functions libqcnn_hip.so plans conv and FC launches with).  Which kernel family runs
GetInPdMat + CalcFeatMap_ConvAprx (src/CaffeEva.cc:1261-1296, :760-868) for a launch geometry is a pure function of plain
numbers; these tests pin the decisions the measured profiles are made of and the properties the decision rules promise."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import pkg

topo = pkg("topology")
synth = pkg("synth")
build = pkg("build")
perf = pkg("perfmodel")

TILE, SLIDE16, SYM16, SYM8, SYM8_SLIDE, HALF8, HALF8_SLIDE = -1, -2, -4, -5, -6, -9, -10
COSTS = ("tile", "slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide")


@pytest.fixture(scope="module")
def planner():
    lib = C.CDLL(build.build_planner_cpu())
    lib.qcnn_plan_conv_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]

    def query(geom, split=1, slide=1, sym=1, sym8=1, half8=1, lut=1, nchw=0, scratch_mi=64, concurrent=0):
        g = (C.c_int * 14)(*geom)
        o = (C.c_int * 8)(split, slide, sym, sym8, half8, lut, nchw | (concurrent << 1), scratch_mi)
        costs = (C.c_double * 7)()
        ch = (C.c_int * 13)()
        assert lib.qcnn_plan_conv_query(g, o, costs, ch) == 0
        return dict(zip(COSTS, costs)), dict(family=ch[0], split_from=ch[1], Z=ch[2], segs=[ch[4 + i] for i in range(ch[3] + 1)] if ch[3] else [])
    return query


def conv_geoms(model, panels):
    """{layer index: geom[14]} of a model's quantised conv layers (shipped quantisation shapes) for a launch over `panels` panels."""
    in_chw, layers, _, _ = topo.MODELS[model]
    sizes = topo.fmap_sizes(in_chw, layers)
    spec = synth.quant_spec(in_chw, layers)
    out = {}
    for i, l in enumerate(layers):
        if l["type"] == topo.CONV:
            (h, w, c), (ho, wo, ct) = sizes[i], sizes[i + 1]
            out[i] = [h, w, c, ho, wo, ct, l["knl"], l["stride"], l["pad"], l["grp"], spec[i]["M"], spec[i]["Cs"], spec[i]["K"], panels]
    return out


def test_headline_decisions(planner):
    """AlexNet at 1000 images (8 panels), library defaults — the kernels of profiles/r6_*: conv2 and conv4 eight-wave symmetric,
    conv3 half-panel eight-wave, conv5 16-wave sliding; conv1 (one 3-dim sub-space) has no eight-wave form."""
    g = conv_geoms("AlexNet", 8)
    fam = {i: planner(geom)[1]["family"] for i, geom in g.items()}
    assert fam[4] == SYM8 and fam[8] == HALF8 and fam[10] == SYM8 and fam[12] == SLIDE16, fam
    costs0, ch0 = planner(g[0], nchw=1)
    assert ch0["family"] in (TILE, SLIDE16) and costs0["sym8"] == 0 and costs0["half8"] == 0 and costs0["sym16"] == 0


def test_concurrent_sub_batches_prefer_tiles_over_strips(planner):
    """QCNN_OPT_STREAMS = 2 (the library default): the plan covers the panels of both sub-batches, and coarse strips overlap worse than
    tiles — AlexNet conv5 moves from the 16-wave sliding kernel to the eight-wave tile form (measured 9.45 -> 9.36 ms per 1000
    images); VGG-16's layers, where the sliding forms win by 10 - 25 %, keep them."""
    g = conv_geoms("AlexNet", 8)
    assert planner(g[12])[1]["family"] == SLIDE16 and planner(g[12], concurrent=1)[1]["family"] == SYM8
    assert [planner(g[i], concurrent=1)[1]["family"] for i in (4, 8, 10)] == [SYM8, HALF8, SYM8]
    for i, geom in conv_geoms("VGG16", 8).items():
        if geom[5] in (128, 256):
            assert planner(geom, concurrent=1)[1]["family"] == SYM8_SLIDE, i


def test_vgg16_decisions(planner):
    """VGG-16 at 1000 images: the 128- / 256-channel layers keep the eight-wave sliding form, the 512-channel layers run half
    panels (28 x 28 maps: sliding form; 14 x 14 maps: tile or sliding form) — profiles/r6_vgg16."""
    in_chw, layers, _, _ = topo.MODELS["VGG16"]
    g = conv_geoms("VGG16", 8)
    for i, geom in g.items():
        ct = geom[5]
        fam = planner(geom)[1]["family"]
        if ct in (128, 256):
            assert fam == SYM8_SLIDE, (i, fam)
        elif ct == 512:
            assert fam in (HALF8, HALF8_SLIDE), (i, fam)
            if geom[3] == 28:
                assert fam == HALF8_SLIDE, (i, fam)


def test_forced_options_and_modes(planner):
    g = conv_geoms("AlexNet", 8)
    assert [planner(g[i], half8=2)[1]["family"] for i in (4, 8, 10, 12)] == [HALF8] * 4
    assert [planner(g[i], half8=3)[1]["family"] for i in (4, 8, 10, 12)] == [HALF8, HALF8_SLIDE, HALF8_SLIDE, HALF8_SLIDE]   # conv2 (5x5) cannot slide
    assert [planner(g[i], sym8=2, half8=0)[1]["family"] for i in (4, 8, 10, 12)] == [SYM8] * 4
    assert [planner(g[i], sym8=3, half8=0)[1]["family"] for i in (4, 8, 10, 12)] == [SYM8_SLIDE] * 4
    assert planner(g[4], sym=2, sym8=0, half8=0)[1]["family"] == SYM16
    for i in (4, 8, 10, 12):
        # everything off: the tile kernel, whole tiles at 8 panels
        c, ch = planner(g[i], split=0, slide=0, sym=0, sym8=0, half8=0)
        assert ch["family"] == TILE and ch["Z"] <= 1 and all(c[k] == 0 for k in COSTS[1:])
        # the exact builder (LUT mode 0) and the fp16 study modes never take the f32 eight-wave families
        assert planner(g[i], lut=0)[1]["family"] in (TILE, SLIDE16)


def test_one_panel_shard_splits_tiles(planner):
    """One GPU's share of a batch sharded over 8 GPUs (one panel): the 13 x 13 layers cannot fill 256 CUs with whole tiles — the
    planner cuts them (QCNN_OPT_SPLIT), and never does with the split switched off."""
    g = conv_geoms("AlexNet", 1)
    for i in (8, 10, 12):
        _, ch = planner(g[i])
        assert (ch["family"] == TILE and ch["Z"] >= 2) or (ch["family"] == SYM8 and ch["Z"] >= 2), (i, ch)
        _, ch0 = planner(g[i], split=0)
        assert ch0["Z"] <= 1, (i, ch0)


def test_costs_scale_with_the_work(planner):
    """More panels never cost less; at many panels the cost is linear in the panel count (no tail effects left)."""
    for model in ("AlexNet", "VGG16"):
        for i, geom in conv_geoms(model, 1).items():
            prev = None
            for panels in (1, 2, 4, 8, 16, 32):
                geom[13] = panels
                c, _ = planner(geom, split=0)
                for k in COSTS:
                    if prev and prev[k] > 0:
                        assert c[k] >= prev[k] * 0.999, (model, i, k, panels)
                prev = c
            c16 = planner(geom[:13] + [16], split=0)[0]
            c32 = planner(geom[:13] + [32], split=0)[0]
            for k in COSTS:
                if c16[k] > 0:
                    assert (1.7 if "slide" in k else 1.85) <= c32[k] / c16[k] <= 2.05, (model, i, k, c32[k] / c16[k])   # (sliding forms re-cut their segments)


def test_half_panel_tiles_build_less(planner):
    """What the half-panel kernel is for: twice the tile, fewer table builds per source pixel — the planner's tile tables and
    perfmodel.py's restatement agree on the stage counts' ratio for AlexNet conv2 - conv5."""
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    sizes = topo.fmap_sizes(in_chw, layers)
    spec = synth.quant_spec(in_chw, layers)
    for i in (4, 8, 10, 12):
        w8 = perf.conv_work(sizes[i], sizes[i + 1], layers[i], spec[i]["M"], spec[i]["K"], spec[i]["Cs"], 8)
        wh = perf.conv_work(sizes[i], sizes[i + 1], layers[i], spec[i]["M"], spec[i]["K"], spec[i]["Cs"], "h8")
        assert wh["stages"] / 2 < w8["stages"]            # builds per source pixel and image


def test_malformed_geometry_is_refused(planner):
    lib = C.CDLL(build.build_planner_cpu())
    g = (C.c_int * 14)(13, 13, 256, 13, 13, 385, 3, 1, 1, 2, 32, 8, 128, 8)      # 385 channels in 2 groups
    o = (C.c_int * 8)(1, 1, 1, 1, 1, 1, 0, 64)
    assert lib.qcnn_plan_conv_query(g, o, None, None) != 0


# ----------------------------------------------------------------------------------------------------------------------
# The recorded sweep: every conv geometry of the six models x panel counts x option sets through qcnn_plan_conv_query, against
# tests/golden/planner_sweep.npz (recorded once, from the planner as it stood when this test was added; a rewrite of the planner's
# pricing has to reproduce it.  `python tests/test_planner_cpu.py` rewrites the file from the library at hand: only for a change
# that is MEANT to move a decision).
# ----------------------------------------------------------------------------------------------------------------------
SWEEP_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "planner_sweep.npz")
SWEEP_PANELS = (1, 2, 3, 4, 5, 8, 16)
# (split, slide, sym, sym8, half8, lut, flags, scratch Mi)
SWEEP_OPTIONS = (
    (1, 1, 1, 1, 1, 1, 0, 64),       # library defaults
    (1, 1, 1, 1, 1, 1, 2, 64),       # concurrent sub-batches
    (0, 1, 1, 1, 1, 1, 0, 64),       # no split
    (1, 1, 1, 1, 0, 1, 0, 64),       # no half-panel family
    (1, 1, 1, 0, 0, 1, 0, 64),       # no eight-wave family
    (1, 0, 0, 0, 0, 1, 0, 64),       # everything off but the split
    (1, 1, 1, 1, 1, 0, 0, 64),       # exact builder
    (1, 2, 1, 1, 1, 1, 0, 64),       # forced: 16-wave sliding
    (1, 1, 2, 0, 0, 1, 0, 64),       # 16-wave symmetric
    (1, 1, 1, 2, 0, 1, 0, 64),       # eight-wave tile form
    (1, 1, 1, 3, 0, 1, 0, 64),       # eight-wave sliding form
    (1, 1, 1, 1, 2, 1, 0, 64),       # half-panel tile form
    (1, 1, 1, 1, 3, 1, 0, 64),       # half-panel sliding form
    (1, 1, 1, 1, 1, 1, 0, 0),        # no scratch
    (1, 1, 1, 1, 1, 1, 0, 4),        # 4 Mi floats of scratch
)


def sweep_queries():
    """(geom[14], opts[8]) of the sweep: the distinct conv layers of every model in topology.MODELS x SWEEP_PANELS x SWEEP_OPTIONS."""
    geoms = []
    for model in ("AlexNet", "CaffeNet", "VggCnnS", "VGG16", "CaffeNetFGB", "CaffeNetFGD"):
        for geom in conv_geoms(model, 1).values():
            if geom[:13] not in geoms:
                geoms.append(geom[:13])
    assert set(topo.MODELS) == {"AlexNet", "CaffeNet", "VggCnnS", "VGG16", "CaffeNetFGB", "CaffeNetFGD"}
    return [(g + [panels], list(o)) for g in geoms for panels in SWEEP_PANELS for o in SWEEP_OPTIONS]


def run_sweep(lib):
    """{geom [n][14], opts [n][8], costs [n][7], choice [n][13]} of sweep_queries() through lib.qcnn_plan_conv_query."""
    lib.qcnn_plan_conv_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    queries = sweep_queries()
    costs, choice = np.zeros((len(queries), 7), np.float64), np.zeros((len(queries), 13), np.int32)
    for i, (g, o) in enumerate(queries):
        c, ch = (C.c_double * 7)(), (C.c_int * 13)()
        assert lib.qcnn_plan_conv_query((C.c_int * 14)(*g), (C.c_int * 8)(*o), c, ch) == 0, (g, o)
        costs[i], choice[i] = list(c), list(ch)
    return dict(geom=np.array([g for g, _ in queries], np.int32), opts=np.array([o for _, o in queries], np.int32), costs=costs, choice=choice)


def test_sweep_matches_recorded_plans():
    """Same decisions, same numbers: family, split, Z and every segment boundary identical to the recorded plan, every cost within
    1e-12 relative (zero stays zero).  The bound is derived: the one numeric freedom is the order in which a CU's running sum takes
    an item's fixed part, (top + a) + f against top + (a + f) — one rounding (2^-52 of the sum) per item, and a CU receives fewer
    than 10^3 items in any scheduled branch of this sweep (ny x nSeg x column groups x panels / 256), so 10^3 x 2^-51 = 4.4e-13."""
    rec = np.load(SWEEP_FILE)
    fam, Z = rec["choice"][:, 0], rec["choice"][:, 2]
    # the recorded data itself: every family, both kinds of Z split, every cost slot
    assert set(fam.tolist()) == {TILE, SLIDE16, SYM16, SYM8, SYM8_SLIDE, HALF8, HALF8_SLIDE}
    assert ((fam == TILE) & (Z > 1)).any() and ((fam == SYM8) & (Z > 1)).any()
    assert (rec["costs"] > 0).any(axis=0).all()
    now = run_sweep(C.CDLL(build.build_planner_cpu()))
    assert np.array_equal(now["geom"], rec["geom"]) and np.array_equal(now["opts"], rec["opts"])
    bad = np.nonzero((now["choice"] != rec["choice"]).any(axis=1))[0]
    assert bad.size == 0, [(rec["geom"][i].tolist(), rec["opts"][i].tolist(), rec["choice"][i].tolist(), now["choice"][i].tolist()) for i in bad[:4]]
    zero = rec["costs"] == 0
    assert (now["costs"][zero] == 0).all()
    dev = np.abs(now["costs"] - rec["costs"])[~zero] / rec["costs"][~zero]
    per_slot = [float((np.abs(now["costs"][:, k] - rec["costs"][:, k])[~zero[:, k]] / rec["costs"][:, k][~zero[:, k]]).max()) for k in range(7)]
    print("largest relative cost deviation per slot:", dict(zip(COSTS, per_slot)))
    assert dev.max() <= 1e-12, dict(zip(COSTS, per_slot))

# ----------------------------------------------------------------------------------------------------------------------
# FC layers: qk_choose_fc through qcnn_plan_fc_query.  The oracle below restates the rule as the engine's launch_layer spelt
# it out before it moved into the planner (decoded slices, the two batch-independent picks, the per-launch re-pick under
# QCNN_OPT_SPLIT, the clamp to what qk_fc_sym8 accepts, the scratch-fit fall-back to one pass).
# ----------------------------------------------------------------------------------------------------------------------
FC_WAVE12, FC_DEC, FC_SYM8, FC_SYM8_F16, FC_SYM8_F16SUM = -1, -3, -5, -7, -8
AMPLE = -1
MAX_FC_SPLIT = 32


def _cdiv(a, b):
    return (a + b - 1) // b


def fc_has_forms(D, Ct, M, K, Cs, P, flatten):
    """(decoded form, eight-wave form) as qcnn_model_commit derives them from the layer's shape."""
    s = _cdiv(Ct, 64) * 64
    dec = (not flatten) and Cs == 1 and M == D and D % 64 == 0 and Ct >= 1 and D * 128 * 4 < 2 ** 32 and D * s * 4 < 2 ** 32
    sym8 = P == 1 and K == 32 and Cs == 4 and M % 4 == 0 and D == 4 * M and Ct >= 192 and Ct % 2 == 0
    return dec, sym8


def fc_oracle(geom, split, sym8, decode, lut, small, flatten, scratch):
    D, Ct, M, K, Cs, P, panels, live = geom
    has_dec, has8 = fc_has_forms(D, Ct, M, K, Cs, P, flatten)
    if decode and has_dec and lut == 1:
        z = 1
        if split:
            wgs = _cdiv(Ct, 64) * panels * _cdiv(live, 64)
            while wgs * z < 192 and D % (64 * 2 * z) == 0 and D // (64 * 2 * z) >= 4 and 2 * z <= 32:
                z *= 2
            z = min(z, MAX_FC_SPLIT)
        if not (z > 1 and z * panels * Ct * 128 <= scratch):
            z = 1
        return FC_DEC, z
    if P > 1:
        return FC_WAVE12, 1
    fc8h = bool(has8 and sym8 and lut >= 2 and not small)
    fc8 = fc8h or bool(has8 and sym8 and lut == 1 and not small and (sym8 >= 2 or not split or panels >= 3))
    msplit = 1
    if lut >= 1:
        G = 128 // K if K <= 64 else 1
        stages = _cdiv(M, G)
        cpb = 12 * (32 if Ct >= 384 else (8 if Ct >= 96 else 4))
        chunks = _cdiv(Ct, 8 * 96) if fc8 else _cdiv(Ct, cpb)

        def pick(min_stages):
            best, best_fill = 1, 0.0
            for cand in range(1, MAX_FC_SPLIT + 1):
                if cand > 1 and stages // cand < min_stages:
                    break
                grid = chunks * cand * 8
                fill = grid / (256.0 * _cdiv(grid, 256))
                if fill > best_fill + 1e-9:
                    best_fill, best = fill, cand
            return best
        ms = pick(24)
        if chunks * ms < 64:
            ms = pick(12)
        if split and chunks * ms * panels < 2 * 256:
            best, best_t = ms, 1e30
            for cand in range(1, MAX_FC_SPLIT + 1):
                if cand > 1 and stages // cand < 8:
                    break
                grid = chunks * cand * panels
                t = float(_cdiv(grid, 256)) * (float(_cdiv(stages, cand)) + 10.0) + 0.5 * cand
                if t < best_t - 1e-9:
                    best_t, best = t, cand
            ms = best
        if ms > 1 and ms * panels * Ct * 128 <= scratch:
            msplit = ms
    if not fc8:
        return FC_WAVE12, msplit
    per = _cdiv(M // 4, msplit)
    return (FC_SYM8_F16SUM if lut == 3 else FC_SYM8_F16) if fc8h else FC_SYM8, _cdiv(M // 4, per)


@pytest.fixture(scope="module")
def fc_planner():
    lib = C.CDLL(build.build_planner_cpu())
    lib.qcnn_plan_fc_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def query(geom, split=1, sym8=1, decode=1, lut=1, small=0, flatten=0, scratch=AMPLE):
        ch = (C.c_int * 2)()
        assert lib.qcnn_plan_fc_query((C.c_int * 8)(*geom), (C.c_int * 7)(split, sym8, decode, lut, small, flatten, scratch), ch) == 0
        return ch[0], ch[1]
    return query


def fc_model_shapes(model):
    """[(name, [D, Ct, M, K, Cs, P], flatten)] of a model's FC layers with the shipped quantisation shapes."""
    in_chw, layers, _, _ = topo.MODELS[model]
    sizes = topo.fmap_sizes(in_chw, layers)
    spec = synth.quant_spec(in_chw, layers)
    out = []
    for i, l in enumerate(layers):
        if l["type"] == topo.FCNT:
            h, w, _ = sizes[i]
            out.append(("%s/%d" % (model, i), [spec[i]["D"], spec[i]["Ct"], spec[i]["M"], spec[i]["K"], spec[i]["Cs"], 1], int(h * w > 1)))
    return out


def fc_shapes():
    shapes = fc_model_shapes("AlexNet") + fc_model_shapes("VGG16")
    for ct in (190, 192, 194, 384, 768, 1000, 4096):              # the eight-wave form needs Ct >= 192 and Ct even
        for m4 in (1, 7, 8, 23, 24, 25, 96):
            for k in (16, 32, 64, 128):
                shapes.append(("seam", [16 * m4, ct, 4 * m4, k, 4, 1], 0))
    for d in (64, 512, 4096):                                     # one-dim sub-spaces: the decoded form
        shapes.append(("onedim", [d, 1000, d, 16, 1, 1], 0))
    return shapes


FC_PANELS, FC_LIVE = (1, 2, 3, 8, 32), (1, 64, 65, 128)
FC_OPTIONS = [dict(split=s, sym8=y, lut=m, small=t) for s in (0, 1) for y in (0, 1, 2) for m in (0, 1, 2, 3) for t in (0, 1)]


def fc_grid():
    """(geom[8], options, flatten, scratch) over shapes x panels x live x options x {ample, one float short of the need}."""
    for _, shape, flatten in fc_shapes():
        for panels in FC_PANELS:
            for live in FC_LIVE:
                geom = shape + [panels, live]
                for opt in FC_OPTIONS:
                    _, z = fc_oracle(geom, decode=1, flatten=flatten, scratch=float("inf"), **opt)
                    yield geom, opt, flatten, AMPLE
                    yield geom, opt, flatten, z * panels * shape[1] * 128 - 1


def test_fc_choice_matches_the_engine_rule(fc_planner):
    n = 0
    for geom, opt, flatten, scratch in fc_grid():
        want = fc_oracle(geom, decode=1, flatten=flatten, scratch=float("inf") if scratch == AMPLE else scratch, **opt)
        assert fc_planner(geom, flatten=flatten, scratch=scratch, **opt) == want, (geom, opt, flatten, scratch)
        n += 1
    assert n == len(fc_shapes()) * len(FC_PANELS) * len(FC_LIVE) * len(FC_OPTIONS) * 2
    # QCNN_OPT_DECODE = 0 and pseudo sub-spaces (P > 1) take the table kernels' rule
    for geom, opt in (([4096, 1000, 4096, 16, 1, 1, 1, 128], dict(decode=0)), ([4096, 1000, 2048, 128, 4, 2, 8, 128], {})):
        assert fc_planner(geom, **opt) == fc_oracle(geom, **dict(dict(split=1, sym8=1, decode=1, lut=1, small=0, flatten=0, scratch=float("inf")), **opt))
    assert fc_planner([4096, 1000, 2048, 128, 4, 2, 8, 128]) == (FC_WAVE12, 1)


def test_fc_choice_properties(fc_planner):
    by_key = {}
    for geom, opt, flatten, scratch in fc_grid():
        fam, z = fc_planner(geom, flatten=flatten, scratch=scratch, **opt)
        D, Ct, M, K, Cs, P, panels, live = geom
        ctx = (geom, opt, flatten, scratch)
        assert 1 <= z <= MAX_FC_SPLIT, ctx
        if fam in (FC_SYM8, FC_SYM8_F16, FC_SYM8_F16SUM):       # the condition qk_fc_sym8 enforces
            stages = M // 4
            assert _cdiv(stages, _cdiv(stages, z)) == z, ctx
        # (a single pass writes no partial sums: the scratch only has to hold what a split launch writes)
        assert z == 1 or scratch == AMPLE or z * panels * Ct * 128 <= scratch, ctx
        if opt["lut"] == 0:
            assert (fam, z) == (FC_WAVE12, 1), ctx
        if opt["split"] == 0 and scratch == AMPLE:              # batch-size-invariant bits: the answer must not depend on the panels
            key = (tuple(geom[:6]), live, flatten, tuple(sorted(opt.items())))
            assert by_key.setdefault(key, (fam, z)) == (fam, z), ctx


# (family, splits) of fc6, fc7, fc8 by panels: one or two panels stay with the 12-wave kernel (its split is not what
# qcnn_get_layer_split reports), from three on fc6 / fc7 run eight-wave; fc8 (one-dim sub-spaces) runs decoded, in fewer k slices
# the more panels fill the chip
FC_PINS = {1: [(FC_WAVE12, 23), (FC_WAVE12, 20), (FC_DEC, 8)], 2: [(FC_WAVE12, 11), (FC_WAVE12, 11), (FC_DEC, 4)],
           3: [(FC_SYM8, 14), (FC_SYM8, 14), (FC_DEC, 2)], 8: [(FC_SYM8, 16), (FC_SYM8, 16), (FC_DEC, 1)]}


def test_fc_headline_decisions(fc_planner):
    """AlexNet fc6 / fc7 / fc8 with library defaults at 1, 2, 3 and 8 panels of 128 images."""
    (_, fc6, f6), (_, fc7, f7), (_, fc8, f8) = fc_model_shapes("AlexNet")
    got = {p: [fc_planner(s + [p, 128], flatten=f) for s, f in ((fc6, f6), (fc7, f7), (fc8, f8))] for p in (1, 2, 3, 8)}
    assert got == FC_PINS, got


def test_fc_malformed_geometry_is_refused(fc_planner):
    lib = C.CDLL(build.build_planner_cpu())
    ch = (C.c_int * 2)()
    assert lib.qcnn_plan_fc_query((C.c_int * 8)(4096, 1000, 1024, 0, 4, 1, 8, 128), (C.c_int * 7)(1, 1, 1, 1, 0, 0, -1), ch) != 0   # K = 0
    assert lib.qcnn_plan_fc_query((C.c_int * 8)(4096, 1000, 1024, 32, 4, 1, 8, 129), (C.c_int * 7)(1, 1, 1, 1, 0, 0, -1), ch) != 0  # live > 128


if __name__ == "__main__":      # the recorder: writes the fixture from the planner library as built from this tree
    np.savez_compressed(SWEEP_FILE, **run_sweep(C.CDLL(build.build_planner_cpu())))
