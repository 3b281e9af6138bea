"""TEST HELPER — window isolation under NaN poison for the conv / FC table kernels: shapes, poison plans and the `hit` rule.

Every table kernel loads its operands unconditionally (qcnn_kernels.hip, "LUT stage builders": device buffers carry slack for the
over-read of dims and sub-spaces that do not exist) and zeroes by a select what must not contribute.  On finite data 0 * x = 0, so a
missing select, a padding tap multiplied into a zero entry or a dependence on what the slack holds changes no bit; with a NaN in
the wrong place it turns outputs into NaN where the reference is finite.  The cases here put NaN

  * into ONE input element per image (images are independent, so a forward of 131 images carries up to 124 of them), at every pixel
    of a small map — every tile, strip and segment seam is crossed whatever the cut — and in the channels at which a sub-space, a
    group or the map ends;
  * into whole images on either side of the panel seam (126 and 129), which the lanes of their neighbours must not see;
  * into everything a smaller batch leaves behind (the stale run of tests/test_gpu_isolation.py).

`hit` says which outputs a poisoned element reaches: for a conv layer the outputs of ITS group whose window holds its pixel, for an
FC layer every channel of its image.  tests/test_isolation_cases_cpu.py holds it to np.isnan of table_probe.dense_expected.

New shapes (kept here: existing tests are parametrised over table_probe.SHAPES).  For each one the furthest byte an operand load
can reach past the end of the layer's input buffer is derived below from the operand addressing of mfma_load — dims one past
the highest one a builder lane loads, minus the dims that exist, times the 512-byte row of one dim — and held below the 64 KB of
slack behind every device buffer (qcnn_engine.h: kSlack) on the CPU tier, before anything runs on a GPU.

Plain numpy; no GPU, no oracle."""
from __future__ import annotations

import numpy as np

import exact_cases as ec
import table_probe as tp

ROW_BYTES = 512              # one dim of one pixel: 128 images x 4 bytes (qcnn_kernels.h: image-minor panels)
K_SLACK = 64 * 1024          # qcnn_engine.h: kSlack; tests/test_isolation_cases_cpu.py reads it out of the header
BATCH, SPLIT_BATCH = 131, 125
STALE_BATCHES = (70, 5, 3)   # clean batches on an engine whose buffers an all-NaN forward of 131 images has filled
WHOLE = (126, 129)           # all-NaN images on either side of the panel seam
CLEAN = (0, 1, 127, 128, 130)   # left clean: the first lanes, both sides of the seam, the last image (1 and 127 / 128: the lanes
                                # that share a position with 129 in the next panel / a neighbour with 126)

# ---------------------------------------------------------------- the new shapes ----
# name -> (kind, geometry, M, K, Cs, None), as table_probe.SHAPES
SHAPES = {
    # two groups of 20 input channels in sub-spaces of 8: 8 + 8 + 4.  The last sub-space of group 0 over-reads the first four
    # channels of group 1 at the same pixel — inside the window and finite, which no finite test can see —, the last sub-space of
    # group 1 the first four channels of the NEXT pixel (for the last pixel: the slack).  128 channels per group: the 16-wave tile
    # kernel with 12 channels per wave, its sliding form, split tiles, the few-image kernel
    "ig_grp2_ragged": ("conv", tp.conv_geom(7, 9, 40, 3, 1, 1, 2, 256), 3, 128, 8, None),
    # K = 32: stages of G = 4 sub-spaces.  14 channels per group: 4 + 4 + 4 + 2 in ONE stage per pixel — the builder keeps its
    # code-book operands in registers (k_conv_aprx: reloadA = false) and masks the activations on that path by itself
    "ig_grp2_cs4_k32": ("conv", tp.conv_geom(7, 9, 28, 3, 1, 1, 2, 128), 4, 32, 4, None),
    # 18 channels per group: 4 x 4 + 2, two stages per pixel, the second with ONE sub-space of two dims and three past the end
    "ig_grp2_cs4_m5": ("conv", tp.conv_geom(7, 9, 36, 3, 1, 1, 2, 128), 5, 32, 4, None),
    # FC layers whose last sub-space is incomplete (D % Cs = 2): qcnn_model_set_layer_shape accepts any M Cs >= D > (M - 1) Cs.
    # The over-read lands in rows 0, 1, .. of the NEXT panel — dims 0, 1, .. of the image 128 further on — and in the slack for
    # the last panel.  Each is the nearest exact-sum / few-image shape with two input dims less, so the slice and stage counts are
    # the ones exact_cases.EXACT_REACH / table_probe.SMALL_REACH pin
    "fr_k128": ("fc", tp.fc_geom(678, 2), 170, 128, 4, None),         # fa_k128: 14 slices of 13 stages, the last of one
    "fr_k64": ("fc", tp.fc_geom(474, 100), 119, 64, 4, None),         # fa_k64: G = 2, the last stage holds ONE sub-space of two dims
    "fr_k32": ("fc", tp.fc_geom(1598, 962), 400, 32, 4, None),        # fx_slices: D != 4 M — no eight-wave form; k_fc_aprx, 8 slices
    "fr_small": ("fc", tp.fc_geom(918, 200), 230, 128, 4, None),      # fc_k128: few-image chunks 224 + 6
}
IG = sorted(n for n in SHAPES if n.startswith("ig_"))
# the base rows of table_probe.TINY_SHAPES — maps of a few pixels, where nearly every tap of nearly every window is a clipping select
# (a padding tap, a row or column of a tile larger than the map, a source pixel no window holds): the place a missing select hides.
# Complete sub-spaces (4 x 8 dims for 32 channels): no operand over-read.  Their family reach is table_probe.TINY_REACH
TG = sorted(tp.TINY_BASE)
FR = sorted(n for n in SHAPES if n.startswith("fr_"))
FR_FROM = {"fr_k128": "fa_k128", "fr_k64": "fa_k64", "fr_k32": "fx_slices", "fr_small": "fc_k128"}


def shape_of(name):
    """(kind, geometry, M, K, Cs) of a case: a new shape, a shape of table_probe.SHAPES or an FC case of exact_cases.FC."""
    if name in SHAPES:
        return SHAPES[name][:5]
    if name in tp.TINY_SHAPES:
        return tp.TINY_SHAPES[name][:5]
    if name in ec.FC:
        return ("fc",) + ec.FC[name][:4]
    return tp.SHAPES[name][:5]


# What the planner and the launchers must choose for the new shapes (layout of table_probe.PANEL_REACH / SMALL_REACH and
# exact_cases.EXACT_REACH; tests/test_isolation_cases_cpu.py re-derives every entry).  slide16 also records its row segments;
# split_tile = (slices, first split tile rank) at one panel of 125 images under QCNN_OPT_SPLIT; small = the few-image launcher's
# (TH, TW, MC, CH, channel chunks per group, G) / FC (MC, G)
IG_REACH = {
    "ig_grp2_ragged": dict(stage=(1, 1, 3), live={"tile": (12, 1, 3, 1, (7, 3), 45), "slide16": (12, 3, 1, 1, 9, 63), "split_tile": (3, 0)},
                           segs=[0, 4, 7], small=(2, 2, 3, 128, 1, 1)),
    "ig_grp2_cs4_k32": dict(stage=(4, 4, 1), live={"tile": (6, 2, 3, 1, (4, 3), 20)}, segs=None, small=(2, 2, 4, 64, 1, 4)),
    "ig_grp2_cs4_m5": dict(stage=(4, 1, 2), live={"tile": (6, 2, 3, 1, (4, 3), 40), "split_tile": (2, 0)}, segs=None,
                           small=(2, 2, 5, 64, 1, 4)),
}
# (family, slices, stages per slice, stages of the last slice): plain at any batch with QCNN_OPT_SPLIT = 0, split at one panel of
# 125 images.  QCNN_OPT_SYM8 = 2 changes nothing: qk_fc_sym8_shape refuses D != 4 M, so k_fc_sym8 never sees a ragged layer
FR_REACH = {
    "fr_k128": dict(G=1, plain=(-1, 14, 13, 1), split=(-1, 17, 10, 10), small=(170, 1)),
    "fr_k64": dict(G=2, plain=(-1, 5, 12, 12), split=(-1, 7, 9, 6), small=(119, 2)),
    "fr_k32": dict(G=4, plain=(-1, 8, 13, 9), split=(-1, 10, 10, 10), small=(400, 4)),
    "fr_small": dict(G=1, plain=(-1, 10, 23, 23), split=(-1, 21, 11, 10), small=(224, 1)),
}


# ---------------------------------------------------------------- how far an operand load reaches ----
def over_read(kind, g, M, K, Cs):
    """dict(rows, bytes, into): how far past the END of the layer's input buffer (the last panel's last pixel) a builder's operand
    load can reach, from mfma_load (qcnn_kernels.hip): for the stage that starts at sub-space m0 a lane loads, per k-step ks < KS
    and sub-space slot sub < SUBS, the row of dim (m0 + sub) Cs + 4 ks + (lane >> 4) of the pixel, counted from the group's first
    channel — whether that sub-space or dim exists or not.  SUBS = 128 / K = G sub-spaces per stage, KS = 2 when min(dims per
    group, Cs) > 4.  So the last stage of a pixel (m0 = (ceil(M / G) - 1) G) reads dims up to (m0 + G - 1) Cs + 4 KS - 1 of the
    LAST group, whose first channel is row (grp - 1) Cg of the pixel's Cin rows (FC: one group, one pixel of D rows).
    rows = (dims missing) = that + 1 - Cin, bytes = rows x 512.  The exact builder (LUT_EXACT; K without an MFMA builder; K > 128),
    the few-image kernels and k_dense load under a condition: nothing is over-read.  Inside the buffer the same rows belong to the
    next group at the pixel, the next pixel, or (FC) the next panel: `into` says which."""
    assert K in (16, 32, 64, 128), "no MFMA builder: the exact builder's loads are conditional"
    Cg = g["Cin"] // g["grp"] if kind == "conv" else g["D"]
    grp = g["grp"] if kind == "conv" else 1
    G = 128 // K
    KS = 2 if min(Cg, Cs) > 4 else 1
    m0 = (-(-M // G) - 1) * G
    dims_read = (m0 + G - 1) * Cs + 4 * KS                       # one past the highest dim of the group a lane loads
    rows = max(0, (grp - 1) * Cg + dims_read - grp * Cg)         # past the pixel's (the vector's) last row
    into = ("the next group's channels, the next pixel and, behind the last pixel, the slack" if kind == "conv" and grp > 1 else
            "the next pixel and, behind the last pixel, the slack" if kind == "conv" else
            "dims 0 .. of the image 128 further on (the next panel) and, behind the last panel, the slack")
    return dict(rows=rows, bytes=rows * ROW_BYTES, missing=dims_read - Cg, into=into)


# the furthest byte past the end of the input buffer, per new shape: (dims missing) x row stride, asserted < kSlack on the CPU tier
OVER_READ_BYTES = {
    "ig_grp2_ragged": 4 * ROW_BYTES,       # 3 sub-spaces of 8 = 24 dims for 20
    "ig_grp2_cs4_k32": 2 * ROW_BYTES,      # one stage of 4 x 4 = 16 dims for 14
    "ig_grp2_cs4_m5": 14 * ROW_BYTES,      # the second stage starts at dim 16 and spans 16 dims: 32 for 18
    "fr_k128": 2 * ROW_BYTES,              # 170 x 4 = 680 dims for 678
    "fr_k64": 6 * ROW_BYTES,               # 60 stages of 2 x 4 dims = 480 for 474 (sub-space 119 does not exist)
    "fr_k32": 2 * ROW_BYTES,               # 100 stages of 16 dims = 1600 for 1598
    "fr_small": 2 * ROW_BYTES,             # 230 x 4 = 920 for 918
}


# ---------------------------------------------------------------- which outputs a poison reaches ----
def hit(kind, g, poison):
    """poison: bool [n, H, W, Cin] (conv) / [n, D] (FC) -> bool [n, Ho, Wo, Ct] (FC: [n, Ct]).  A poisoned element in a channel of
    group q reaches exactly the outputs of group q whose window holds its pixel (table_probe.window_hit per group); for an FC layer
    every channel of its image."""
    poison = np.asarray(poison, bool)
    if kind == "fc":
        return np.repeat(poison.any(1)[:, None], g["Ct"], axis=1)
    grp = g["grp"]
    Cg, Ctg = g["Cin"] // grp, g["Ct"] // grp
    Ho, Wo = tp.out_hw(g)
    out = np.zeros((poison.shape[0], Ho, Wo, g["Ct"]), bool)
    for q in range(grp):
        out[..., q * Ctg:(q + 1) * Ctg] = tp.window_hit(g, poison[..., q * Cg:(q + 1) * Cg])[..., None]
    return out


# ---------------------------------------------------------------- poison plans ----
def channels(kind, g, M, Cs):
    """The channels (FC: input dims) a plan cycles through: the first; the last of the last complete run of sub-spaces,
    (M - 1) Cs - 1; the first of the last sub-space, (M - 1) Cs; the last existing channel of group 0; the first channel of group 1
    (one group: the last channel again).  Duplicates are kept out, the order stays."""
    d = g["Cin"] // g["grp"] if kind == "conv" else g["D"]
    cs = [0, (M - 1) * Cs - 1, (M - 1) * Cs, d - 1, d if kind == "conv" and g["grp"] > 1 else d - 1]
    out = []
    for c in cs:
        if 0 <= c and c not in out:
            out.append(c)
    return out


def pixels(g, room):
    """The pixels a plan poisons, at most `room`: every pixel when H W <= 100 (and it fits), else the border and every second
    interior pixel in both axes, thinned evenly to `room` with both far corners kept."""
    H, W = g["H"], g["W"]
    if H * W <= 100 and H * W <= room:
        return [(h, w) for h in range(H) for w in range(W)]
    px = [(h, w) for h in range(H) for w in range(W) if h in (0, H - 1) or w in (0, W - 1) or (h % 2 == 1 and w % 2 == 1)]
    if len(px) > room:
        idx = np.unique(np.round(np.linspace(0, len(px) - 1, room)).astype(int))
        px = [px[i] for i in idx]
    assert px[0] == (0, 0) and px[-1] == (H - 1, W - 1)
    return px


def plan(kind, g, M, Cs, n=BATCH):
    """dict(single = [(image, h, w, c)] with at most one element per image, whole = all-NaN images, clean = images left clean) of a
    forward of n images.  n = 131: whole = 126 and 129, clean = 0, 1, 127, 128 and 130; a smaller batch (the split forms' 125)
    keeps 0 and 1 clean and makes image n - 2 the all-NaN one.  single: both far corners of the map first (first and last
    channel), then one image per pixel of `pixels`, the channel cycling through `channels`; FC: one image per entry of `channels`
    (h = w = 0, c = the input dim)."""
    whole = [i for i in WHOLE if i < n] if n >= BATCH else [n - 2]
    clean = [i for i in CLEAN if i < n]
    free = [i for i in range(n) if i not in whole and i not in clean]
    chs = channels(kind, g, M, Cs)
    if kind == "fc":
        elems = [(0, 0, c) for c in chs]
    else:
        H, W, Cin = g["H"], g["W"], g["Cin"]
        elems = [(0, 0, 0), (H - 1, W - 1, Cin - 1)]
        elems += [(h, w, chs[i % len(chs)]) for i, (h, w) in enumerate(pixels(g, len(free) - 2))]
        # a map with fewer pixels than listed channels (the tg_* shapes): the channels the cycle did not reach, at the last pixel
        elems += [(H - 1, W - 1, c) for c in chs if c not in {e[2] for e in elems}]
    assert len(elems) <= len(free)
    # spread over the free images: the poisons then sit in both halves of the full panel, not in its first lanes alone
    step = len(free) / len(elems)
    single = [(free[int(i * step)],) + e for i, e in enumerate(elems)]
    assert len({s[0] for s in single}) == len(single)
    return dict(single=single, whole=whole, clean=clean)


def few_plans(kind, g, M, Cs):
    """[(what, (h, w, c))] for the few-image kernels: a forward of three images — image 0 clean, image 1 with ONE poisoned element,
    image 2 all NaN — per entry.  Conv: both far corners, the centre tap of the centre output's window in every channel of
    `channels`; FC: every entry of `channels`."""
    chs = channels(kind, g, M, Cs)
    if kind == "fc":
        return [("dim %d" % c, (0, 0, c)) for c in chs]
    H, W, Cin = g["H"], g["W"], g["Cin"]
    out = [("the first pixel", (0, 0, 0)), ("the last pixel", (H - 1, W - 1, Cin - 1))]
    ch, cw = centre(g)
    return out + [("the centre, channel %d" % c, (ch, cw, c)) for c in chs]


def centre(g):
    """The centre tap of the centre output's window (as tests/test_gpu_decoded_cases.py::poisons)."""
    Ho, Wo = tp.out_hw(g)
    return (Ho // 2 * g["stride"] - g["pad"] + g["knl"] // 2, Wo // 2 * g["stride"] - g["pad"] + g["knl"] // 2)


def mask_of(kind, g, n, single=(), whole=()):
    """bool [n, H, W, Cin] (FC: [n, D]) of a plan's elements."""
    if kind == "fc":
        m = np.zeros((n, g["D"]), bool)
        for i, _, _, c in single:
            m[i, c] = True
    else:
        m = np.zeros((n, g["H"], g["W"], g["Cin"]), bool)
        for i, h, w, c in single:
            m[i, h, w, c] = True
    for i in whole:
        m[i] = True
    return m


def plan_mask(kind, g, M, Cs, n=BATCH):
    p = plan(kind, g, M, Cs, n)
    return mask_of(kind, g, n, p["single"], p["whole"]), p


def poisoned(x, mask):
    return np.where(mask, np.float32(np.nan), np.asarray(x, np.float32))


# ---------------------------------------------------------------- what a single poison reaches, where that is not "some, not all" ----
# Every single-element poison reaches at least one output of its image and leaves at least one untouched — except these, stated
# and asserted as such (tests/test_isolation_cases_cpu.py).  FC: every single poison reaches the whole image (no untouched output).
REACHES_NONE = {"sm_ct24": "1x1 / stride 2 on 5 x 6: only even rows and columns are looked at"}
REACHES_ALL = {"sm_15_m2": "15x15 window on 20 x 20: the centre lies in all 36 windows", "sm_15_k64": "as sm_15_m2"}
# positions (of Ho Wo) whose window holds the first pixel / the centre, from table_probe.window_hit itself
POSITIONS = {
    "pn_deep": (4, 9, 70), "pn_c192": (4, 9, 63), "pn_c256_cs4": (4, 9, 70), "pn_c384": (4, 9, 63), "pn_c512": (4, 9, 70),
    "pn_k32_m18": (4, 9, 70), "pn_k10_m32": (4, 9, 70), "pn_k64_m9": (4, 9, 63), "pn_partial": (4, 9, 63), "pn_k200": (4, 9, 70),
    "pn_k256": (4, 9, 70), "pn_grp2_5x5": (9, 25, 77), "pn_s2_5x5": (4, 9, 35),
    "ig_grp2_ragged": (4, 9, 63), "ig_grp2_cs4_k32": (4, 9, 63), "ig_grp2_cs4_m5": (4, 9, 63),
    "tg_1x1": (1, 1, 1), "tg_1x2": (2, 2, 2), "tg_col": (2, 3, 7), "tg_fit": (1, 1, 1), "tg_gap": (1, 1, 6), "tg_k5": (6, 6, 6),
    "tg_pad2": (9, 9, 16), "tg_row": (2, 3, 4), "tg_s2": (4, 4, 4), "tg_s4": (1, 1, 3),
}
# On the tg_* maps "some, not all" cannot hold pixel by pixel: a 1 x 1 map has one output, a 5x5 window holds a whole 2 x 3 map, a
# stride above the kernel size leaves source pixels no window holds.  Stated instead, per shape: (pixels whose poison reaches NO
# output, pixels whose poison reaches EVERY output, pixels of the map); every other pixel reaches some and not all
TG_PIXELS = {
    "tg_1x1": (0, 1, 1), "tg_1x2": (0, 2, 2), "tg_col": (0, 0, 7), "tg_fit": (0, 9, 9), "tg_gap": (32, 0, 56), "tg_k5": (0, 6, 6),
    "tg_pad2": (0, 0, 4), "tg_row": (0, 0, 4), "tg_s2": (0, 9, 12), "tg_s4": (22, 0, 36),
}


# ---------------------------------------------------------------- dense (precise-path) reference ----
def dense_layer64(kind, g, x, bias, weights):
    """(want64, mag) of the precise path (k_dense): conv kernels [Ct][Cin / grp][kh][kw] on NHWC x / FC weights [Ct][D] on [n, D];
    float64 with plain loops over the taps."""
    x = np.asarray(x, np.float32).astype(np.float64)
    b = np.asarray(bias, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    if kind == "fc":
        return b + x @ w.T, np.abs(b) + np.abs(x) @ np.abs(w).T
    n, H, W, Cin = x.shape
    knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
    Ho, Wo = tp.out_hw(g)
    Cg, Ctg = Cin // grp, Ct // grp
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    want, mag = np.tile(b, (n, Ho, Wo, 1)), np.tile(np.abs(b), (n, Ho, Wo, 1))
    for q in range(grp):
        cts, cin = slice(q * Ctg, (q + 1) * Ctg), slice(q * Cg, (q + 1) * Cg)
        for kh in range(knl):
            for kw in range(knl):
                sl = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, cin]
                want[..., cts] += sl @ w[cts, :, kh, kw].T
                mag[..., cts] += np.abs(sl) @ np.abs(w[cts, :, kh, kw]).T
    return want, mag
