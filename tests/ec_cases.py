"""TEST HELPER — crafted layers for qcnn_quantize_layer_ec and exact-sum geometries for qcnn_calib_gram (DESIGN.md
"Error-corrected quantisation").  Importable without a GPU; books and assignments are built with numpy, no k-means.

A case is ``dict(w, G, ctrd, asmt, grp, M, K, Cs, x, geom, **what the family expects)``; ``G`` is the fp64 gram matrix of the
numpy oracle (tests/ec_oracle.py), so the replay of a sweep does not depend on k_ec_gram.  CASES names them all; a case is
built on first use and cached: treat it as read-only.  Both tiers run every case through ``ec_oracle.replay_sweep`` for both
RIDGES: tests/test_ec_cases_cpu.py on the oracle's own sweep and its mutations, tests/test_gpu_quantize_ec_cases.py on the
kernels.

RANDOM: random books and assignments at the smallest shapes that reach a path of the kernels (the table below).
Crafted: bit-equal code words where the tie rules decide bytes, dead input channels where A_k is singular, and the two
extreme member counts.
"""
from __future__ import annotations

import functools

import numpy as np

import ec_oracle as eo

RIDGES = (0.0, 1e-6)

# name: weight shape, grp, M, K, Cs, input (n, H, W), stride, pad, seed                  (Cin per group = shape[1])
RANDOM = {
    "conv3x3": ((32, 16, 3, 3), 1, 2, 32, 8, (4, 8, 8), 1, 1, 910),                       # the baseline conv
    "rect_grouped": ((24, 6, 3, 2), 2, 2, 16, 4, (4, 7, 9), 2, 1, 911),                  # kh != kw, H != W, groups, CsEff = 2
    "k256_cs16": ((66, 20, 2, 3), 1, 2, 256, 16, (4, 6, 5), 1, 1, 912),                  # K = QCNN_PQ_MAX_K, Cs = 16, CsEff = 4, many
                                                                                         # words memberless, two row tiles of k_ec_eg
    "fc_k130": ((130, 40), 2, 10, 130, 4, (64, 1, 1), 1, 0, 913),                        # K across three waves, the one-shot update
    "rgb_like": ((16, 3, 5, 5), 1, 1, 32, 8, (4, 12, 12), 2, 0, 914),                    # CsEff = 3, M = 1
}


def post_relu(rng, shape):
    return np.maximum(rng.standard_normal(shape) + 0.3, 0.0).astype(np.float32)


def _case(w, x, ctrd, asmt, grp, stride, pad, **extra):
    ct, cin, kh, kw = eo.dims(w)
    M, K, Cs = ctrd.shape
    geom = dict(grp=grp, kh=kh, kw=kw, stride=stride, pad=pad)
    G = eo.gram(x, grp, kh, kw, stride, pad)[0]
    asmt = np.ascontiguousarray(asmt, np.uint8).reshape((ct, kh, kw, M) if np.ndim(w) == 4 else (ct, M))
    return dict(w=np.ascontiguousarray(w, np.float32), x=x, G=G, ctrd=np.ascontiguousarray(ctrd, np.float32), asmt=asmt, grp=grp,
                M=M, K=K, Cs=Cs, geom=geom, **extra)


def _zero_pads(book, cin):
    M, K, Cs = book.shape
    for m in range(M):
        book[m, :, max(0, min(cin - m * Cs, Cs)):] = 0.0
    return book


def random_case(name):
    shape, grp, M, K, Cs, (n, H, W), stride, pad, seed = RANDOM[name]
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(shape).astype(np.float32)
    ct, cin, kh, kw = eo.dims(w)
    x = post_relu(rng, (n, H, W, cin * grp))
    book = _zero_pads(rng.standard_normal((M, K, Cs)).astype(np.float32), cin)
    asmt = rng.integers(0, K, (ct, kh * kw, M)).astype(np.uint8)
    return _case(w, x, book, asmt, grp, stride, pad, random=True)


# ------------------------------------------------------------------------------ duplicate code words
DUP_PAIRS = {"dup_3_7": (3, 7, 16), "dup_5_69": (5, 69, 128), "dup_69_200": (69, 200, 256)}        # lo, hi, K


def dup_case(name):
    """FC, M = 2, Cs = 4: word hi of each sub-space is a bit-equal copy of word lo, and the weights of the channels ``dup_ct``
    sit 1e-3 from that word on both sub-spaces.  They start at another word in sub-space 0 and at hi in sub-space 1, so the
    cross terms of the other sub-space are tiny and the duplicated word is the strict best of sub-space 0 (asserted on the
    oracle).  Thread lo and thread hi of k_ec_assign price the same number: (3, 7) meet in the shuffles of one wave, (5, 69)
    and (69, 200) in wBest / wIdx of two waves.  The contract sends every one of those channels to lo in sub-space 0, and
    leaves them at hi in sub-space 1, where the copy at the lower index prices delta = 0."""
    lo, hi, K = DUP_PAIRS[name]
    rng = np.random.default_rng(920 + lo)
    ct, M, Cs = 40, 2, 4
    book = rng.standard_normal((M, K, Cs)).astype(np.float32)
    book[:, hi] = book[:, lo]
    w = rng.standard_normal((ct, M * Cs)).astype(np.float32)
    dup_ct = np.arange(0, ct, 3)
    w[dup_ct] = book[:, lo].reshape(-1)[None, :] + (1e-3 * rng.standard_normal((len(dup_ct), M * Cs))).astype(np.float32)
    others = np.array([k for k in range(K) if k not in (lo, hi)])
    asmt = others[rng.integers(0, len(others), (ct, M))]
    asmt[dup_ct, 1] = hi
    x = post_relu(rng, (48, 1, 1, M * Cs))
    return _case(w, x, book, asmt, 1, 1, 0, dup=(lo, hi), dup_ct=dup_ct)


# ------------------------------------------------------------------------------ a copy of every current word at a lower k
def copies_case():
    """A conv layer at a fixed point of the oracle's sweeps (no assignment changes, no code word moves, ridge RIDGES[1]) with its
    8 code words in slots 16 .. 23; slots 0 .. 7 hold bit-equal copies of them, every other slot a far-away word.  The copy
    prices delta = 0 exactly: nothing may move, the assignments come back byte for byte and the copies keep their bits."""
    rng = np.random.default_rng(930)
    shape, M, Ku, K, Cs = (12, 8, 2, 2), 2, 8, 32, 4
    w = rng.standard_normal(shape).astype(np.float32)
    x = post_relu(rng, (4, 5, 5, 8))
    G = eo.gram(x, 1, 2, 2, 1, 0)[0]
    c = rng.standard_normal((M, Ku, Cs)).astype(np.float32)
    a = rng.integers(0, Ku, (12, 2, 2, M)).astype(np.uint8)
    for _ in range(60):
        c2, a2, _, chg = eo.quantize_layer_ec(w, c, a, G, sweeps=1, ridge=RIDGES[1])
        still = chg[0] == 0 and c2.tobytes() == c.tobytes()
        c, a = c2.copy(), a2.copy()
        if still:
            break
    assert still, "the oracle's sweeps did not reach a fixed point"
    book = (100.0 + 10.0 * rng.standard_normal((M, K, Cs))).astype(np.float32)
    book[:, 16:24] = c
    book[:, 0:8] = c
    return _case(w, x, book, a + 16, 1, 1, 0, fixed_point=True)


# ------------------------------------------------------------------------------ dead input channels
def dead_case(name):
    """A 2 x 2 conv layer, M = 2, Cs = 4, whose calibration images are zero on all channels of sub-space 1 ('dead_subspace') or
    on channel 2 = dim 2 of sub-space 0 ('dead_dim').  The rows and columns of G at the dead patch entries are exactly 0.
    ridge = 0: A_k of every word with members in ``dead_m`` is singular, the words of that sub-space keep their bits.
    ridge > 0: v_j = 0 and the solve is exactly 0 on the dead dims ``dead_dims``; the live dims obey the residual bound."""
    rng = np.random.default_rng(940)
    shape, M, K, Cs = (10, 8, 2, 2), 2, 8, 4
    w = rng.standard_normal(shape).astype(np.float32)
    x = post_relu(rng, (3, 5, 5, 8))
    dead_m, dead_dims = (1, [0, 1, 2, 3]) if name == "dead_subspace" else (0, [2])
    x[..., [dead_m * Cs + j for j in dead_dims]] = 0.0
    book = rng.standard_normal((M, K, Cs)).astype(np.float32)
    asmt = rng.integers(0, K, (10, 2, 2, M)).astype(np.uint8)
    return _case(w, x, book, asmt, 1, 1, 0, dead_m=dead_m, dead_dims=dead_dims)


# ------------------------------------------------------------------------------ one word with every member / one member per word
def members_case():
    """A 2 x 2 conv layer with N = Ct * taps = 32 blocks per sub-space and K = 32.  Sub-space 0: every block names word 5, which
    sits in the middle of the weights while every other word is far away.  Sub-space 1: block n names word perm[n]; the
    weights there are far apart from each other and each 0.05 from its word.  No assign step moves anything (asserted on the
    oracle), so the update meets exactly these member lists: one A_k of 32 members with cross-tap terms, 32 of one member."""
    rng = np.random.default_rng(950)
    ct, M, K, Cs = 8, 2, 32, 4
    perm = rng.permutation(K)
    book = np.empty((M, K, Cs), np.float32)
    book[0] = (50.0 + 10.0 * rng.standard_normal((K, Cs))).astype(np.float32)
    book[0, 5] = 0.1
    book[1] = (8.0 * np.arange(K)[:, None] + rng.standard_normal((K, Cs))).astype(np.float32)
    w = np.empty((ct, 2 * Cs, 2, 2), np.float32)
    w[:, :Cs] = rng.standard_normal((ct, Cs, 2, 2)).astype(np.float32)
    asmt = np.empty((ct, 4, M), np.uint8)
    asmt[:, :, 0] = 5
    asmt[:, :, 1] = perm.reshape(ct, 4)
    w[:, Cs:] = (book[1][asmt[:, :, 1]] + 0.05 * rng.standard_normal((ct, 4, Cs))).transpose(0, 2, 1).reshape(ct, Cs, 2, 2)
    x = post_relu(rng, (4, 5, 5, 2 * Cs))
    return _case(w, x, book, asmt, 1, 1, 0, members=True)


BUILDERS = dict([(n, functools.partial(random_case, n)) for n in RANDOM] + [(n, functools.partial(dup_case, n)) for n in DUP_PAIRS]
                + [("copies_below", copies_case), ("dead_subspace", functools.partial(dead_case, "dead_subspace")),
                   ("dead_dim", functools.partial(dead_case, "dead_dim")), ("members_all_or_one", members_case)])
CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


def shape_rules_ok(c):
    """What the C-ABI of qcnn_quantize_layer_ec asks of a case."""
    ct, cin, kh, kw = eo.dims(c["w"])
    M, K, Cs, grp = c["M"], c["K"], c["Cs"], c["grp"]
    P = kh * kw * cin
    return (ct % grp == 0 and 2 <= K <= 256 and 1 <= Cs <= 16 and (M - 1) * Cs < cin <= M * Cs and c["G"].shape == (grp, P, P)
            and c["ctrd"].shape == (M, K, Cs) and c["ctrd"].dtype == np.float32 and c["asmt"].dtype == np.uint8
            and c["asmt"].size == ct * kh * kw * M and int(c["asmt"].max()) < K and np.isfinite(c["ctrd"]).all()
            and np.isfinite(c["G"]).all() and (np.einsum("gpp->gp", c["G"]) >= 0).all())


# ------------------------------------------------------------------------------ gram geometries with exact sums
GRAM_TILE, GRAM_CHUNK = 64, 16          # k_ec_gram: G tile per workgroup, patches staged per step

# name: (n, H, W, C, grp, kh, kw, stride, pad)
GRAM_EXACT = {
    "rect_grouped": (3, 7, 10, 6, 2, 3, 2, 2, 1),
    "rect_1x3": (2, 5, 9, 4, 1, 1, 3, 1, 1),
    "rect_4x1_stride3": (2, 9, 5, 4, 1, 4, 1, 3, 0),
    "p630_pad2": (1, 3, 3, 70, 1, 3, 3, 1, 2),           # ten tiles, the last one ragged; most taps out of the image
    "rows5_p65": (5, 1, 1, 65, 1, 1, 1, 1, 0),           # fewer rows than one LDS chunk
    "rows153": (17, 4, 4, 8, 1, 2, 2, 1, 0),             # a ragged chunk
    "rows264_two_splits": (22, 5, 4, 6, 1, 2, 2, 1, 0),  # rows straddle one run: a split seam at 256, 8 rows in the last split
    "rows300_one_split": (300, 1, 1, 2817, 1, 1, 1, 1, 0),   # 1035 workgroups: one split, a run seam inside it (256 + 44)
    "rows8463_17_splits": (1, 91, 93, 64, 64, 1, 1, 1, 0),   # 64 groups of P = 1: two runs per split, 271 rows in the last
}
GRAM_SPLITS = {"rows264_two_splits": (256, 2), "rows300_one_split": (512, 1), "rows8463_17_splits": (512, 17)}   # rows per split, splits
GRAM_ACCUMULATE = ("rect_grouped", "rows264_two_splits")


def gram_rows(geom):
    n, H, W, C, grp, kh, kw, stride, pad = geom
    return n * eo.out_size(H, kh, stride, pad) * eo.out_size(W, kw, stride, pad)


def gram_split(geom, run, max_slab_bytes=2 << 30):
    """(rows per split, splits) of qk_ec_gram_rows_per_split (csrc/qcnn_ec.hip), restated: whole runs per split, enough
    workgroups to fill the chip, slabs of at most max_slab_bytes in all."""
    n, H, W, C, grp, kh, kw, stride, pad = geom
    P, rows = kh * kw * (C // grp), gram_rows(geom)
    nt = (P + GRAM_TILE - 1) // GRAM_TILE
    wgs = nt * (nt + 1) // 2 * grp
    runs = (rows + run - 1) // run
    want = max(1, 2048 // wgs)
    want = min(want, max(1, max_slab_bytes // (grp * P * P * 8)))
    want = max(1, min(want, runs, 65535))
    per = (runs + want - 1) // want * run
    return per, max(1, (rows + per - 1) // per)


def gram_input(name):
    """Integers 0 .. 3, about half of them 0: every fp32 product (<= 9) and every sum of a run of 256 patches (<= 2304) is
    exact, and so is the fp64 sum across runs and splits — the result has one correct value, to the bit."""
    n, H, W, C = GRAM_EXACT[name][:4]
    rng = np.random.default_rng(960 + len(name))
    return (rng.integers(1, 4, (n, H, W, C)) * (rng.random((n, H, W, C)) < 0.5)).astype(np.float32)


def one_hot_expected(geom, iy, ix):
    """The gram matrix of one image that is 1 on every channel of pixel (iy, ix) and 0 elsewhere, from the geometry alone: an
    output pixel (oy, ox) sees the pixel through tap (y, x) = (iy + pad - oy * stride, ix + pad - ox * stride) if that is
    inside the window; its patch is 1 on the Cg entries of that tap, so G_g gains a Cg x Cg block of ones there."""
    n, H, W, C, grp, kh, kw, stride, pad = geom
    cg = C // grp
    G = np.zeros((grp, kh * kw * cg, kh * kw * cg))
    for oy in range(eo.out_size(H, kh, stride, pad)):
        for ox in range(eo.out_size(W, kw, stride, pad)):
            y, x = iy + pad - oy * stride, ix + pad - ox * stride
            if 0 <= y < kh and 0 <= x < kw:
                tap = y * kw + x
                G[:, tap * cg:(tap + 1) * cg, tap * cg:(tap + 1) * cg] += 1.0
    return G
