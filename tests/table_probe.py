"""TEST HELPER — one-hot assignment probes: read single look-up-table entries out of a conv / FC layer, exactly.

A conv / FC output is ``bias + sum over (kh, kw, m) of T[pixel][m][asmt[ct][kh][kw][m]]`` (src/CaffeEva.cc:760-868, 968-1025).
With ``bias = 0``, one all-zero code word per sub-space (the *silent* word: its table entry is exactly 0.0f under any builder)
and assignments that name the silent word everywhere except at ONE (kh*, kw*, m*) per output channel, where they name k*,

    out[n, ho, wo, ct] = 0 + ... + T[n, (ho*s - pad + kh*, wo*s - pad + kw*), m*, k*] + ... + 0

and adding 0.0f is exact in any order, grouping or accumulator layout: the output IS the table entry (or exactly 0 where
the tap lies in the padding, which the reference skips).  So an entry can be held to the textbook bound of an fp32 dot
product against a float64 one, per entry and relative to the entry's own magnitude:

    |T - T64| <= gamma_n * sum_j |x_j c_j|,   gamma_n = n u / (1 - n u),   u = 2^-24,   n = CsEff

(n rounded products, n - 1 rounded additions behind the exact 0 + p_0; an f32 MFMA is a k-ordered fmaf chain, one rounding
per step).  The exact builder must moreover return the float32 sequence ``acc = acc + x_j * c_j`` bit for bit.

Plain numpy; no GPU, no oracle.  Layouts are the reference's file layouts, as synth.make_params writes them: ctrd [M][K][Cs]
(dims >= CsEff of a partial last sub-space zero), asmt 0-based uint8 [Ct][kh][kw][M] (conv) / [Ct][M] (FC).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24                     # unit round-off of float32
LO, HI = 2.0 ** -60, 2.0 ** 60     # every |x_j c_j| of a probe stays inside: no subnormals, no overflow


def gamma(n):
    return n * U / (1.0 - n * U)


SPLIT_BF16_PRODUCT = 2.0 ** -22    # three bf16 pieces per operand, six cross terms: each product within 2^-22 (test_bf16split_cpu.py)


def split_extra(cs_eff):
    """What the split-bf16 decoded conv may add to gamma_CsEff: `check(.., n_terms=cs_eff, extra=split_extra(cs_eff))` is the
    bound (2^-22 + gamma_(6 CsEff)) * mag — six cross terms per product, at most 6 CsEff fp32 additions."""
    return SPLIT_BF16_PRODUCT + gamma(6 * cs_eff) - gamma(cs_eff)


# ---------------------------------------------------------------- geometry ----
def conv_geom(H, W, Cin, knl, stride, pad, grp, Ct):
    return dict(H=H, W=W, Cin=Cin, knl=knl, stride=stride, pad=pad, grp=grp, Ct=Ct)


def fc_geom(D, Ct):
    return dict(D=D, Ct=Ct)


def _dims(kind, g):
    """(Ct, taps per side, input dims one group's code book spans)."""
    if kind == "conv":
        return g["Ct"], g["knl"], g["Cin"] // g["grp"]
    return g["Ct"], 1, g["D"]


def cs_eff(kind, g, M, Cs):
    _, _, d = _dims(kind, g)
    assert (M - 1) * Cs < d <= M * Cs, (d, M, Cs)
    return [min(d - m * Cs, Cs) for m in range(M)]


def out_hw(g):
    return ((g["H"] + 2 * g["pad"] - g["knl"]) // g["stride"] + 1, (g["W"] + 2 * g["pad"] - g["knl"]) // g["stride"] + 1)


# ---------------------------------------------------------------- schedule ----
def schedule(kind, g, M, K, Cs, max_rounds=None, negate=False):
    """The rounds of a probe: a list of dict(r, silent, negate).  Round r names, for channel ct, pair number
    q = r * Ct + ct of the (m, k) enumeration below and tap q mod knl^2, so that ceil(M (K - 1) / Ct) rounds name every
    (m, k >= 1) and ceil(knl^2 / Ct) rounds every tap, corners included.  The rounds after those use code word K - 1 as the
    silent one and start the enumeration at k = 0 (ceil(M / Ct) rounds name k = 0 in every sub-space).  max_rounds thins the
    first kind (the caller states the share covered); negate adds every round once more with the code book negated (fused
    ReLU: both signs are seen)."""
    Ct, knl, _ = _dims(kind, g)
    n_main = max(-(-M * (K - 1) // Ct), -(-knl * knl // Ct))
    if max_rounds is not None:
        n_main = min(n_main, max_rounds)
    n_sil = -(-M // Ct)
    rounds = [dict(r=r, silent=0, negate=False) for r in range(n_main)]
    rounds += [dict(r=r, silent=K - 1, negate=False) for r in range(n_sil)]
    if negate:
        rounds += [dict(rd, negate=True) for rd in rounds]
    return rounds


def picks_of_round(kind, g, M, K, rd):
    """Per channel (kh*, kw*, m*, k*) [Ct, 4] of a round.  Pair q -> m = q mod M, k from q div M: neighbouring channels
    (lanes) differ in sub-space and in code word."""
    Ct, knl, _ = _dims(kind, g)
    q = rd["r"] * Ct + np.arange(Ct)
    m = q % M
    if rd["silent"] == 0:                              # silent word 0: k in 1 .. K-1, shifted by m so that one round of a
        k = (q // M + m) % (K - 1) + 1                 # thinned schedule already names every k (a bijection for every m)
    else:                                              # silent word K-1: k in 0 .. K-2, k = 0 first in every sub-space
        k = (q // M) % (K - 1)
    t = q % (knl * knl)
    return np.stack([t // knl, t % knl, m, k], axis=1).astype(np.int64)


def probe_params(kind, g, M, K, Cs, rd, seed=0):
    """dict(bias, ctrd, asmt, bits, picks) of round rd: the file layout of synth.make_params.  Code words: standard normal
    float32 (full mantissas), magnitudes kept >= 2^-6; the silent word and the dims >= CsEff are zero."""
    Ct, knl, _ = _dims(kind, g)
    cse = cs_eff(kind, g, M, Cs)
    rng = np.random.default_rng([seed, 17])            # the same code book in every round of a case
    ctrd = _away_from_zero(rng.standard_normal((M, K, Cs)).astype(np.float32))
    for m in range(M):
        ctrd[m, :, cse[m]:] = 0.0
    ctrd[:, rd["silent"], :] = 0.0
    if rd["negate"]:
        ctrd = -ctrd
    picks = picks_of_round(kind, g, M, K, rd)
    ct = np.arange(Ct)
    if kind == "conv":
        asmt = np.full((Ct, knl, knl, M), rd["silent"], np.uint8)
        asmt[ct, picks[:, 0], picks[:, 1], picks[:, 2]] = picks[:, 3]
    else:
        asmt = np.full((Ct, M), rd["silent"], np.uint8)
        asmt[ct, picks[:, 2]] = picks[:, 3]
    bits = max(1, int(K - 1).bit_length())
    return dict(bias=np.zeros(Ct, np.float32), ctrd=ctrd, asmt=asmt, bits=bits, picks=picks)


def _away_from_zero(v, floor=2.0 ** -6):
    v = np.asarray(v, np.float32)
    return np.where(np.abs(v) < floor, v + np.copysign(np.float32(floor), v), v).astype(np.float32)


def activations(kind, g, n, seed, scaled):
    """Input of the probed layer: NHWC [n, H, W, Cin] (conv) / [n, D] (FC), float32 standard normal with full mantissas
    (magnitudes >= 2^-6); scaled: times 2^e per image and per channel, e uniform in -20 .. 20 (an absolute instead of a
    relative error of a builder shows only there)."""
    rng = np.random.default_rng([seed, 29, int(scaled)])
    shape = (n, g["H"], g["W"], g["Cin"]) if kind == "conv" else (n, g["D"])
    x = _away_from_zero(rng.standard_normal(shape).astype(np.float32))
    if scaled:
        e = rng.integers(-20, 21, size=(n, shape[-1]))
        x = x * np.exp2(e).astype(np.float32).reshape((n,) + (1,) * (len(shape) - 2) + (shape[-1],))
    return np.ascontiguousarray(x, np.float32)


# ---------------------------------------------------------------- expected entries ----
def expected(kind, g, x, params, block=64):
    """(want64, mag, want32_seq) of the probe `params` on input x (layout of `activations`), shaped like the layer's output
    [n, Ho, Wo, Ct] (FC: [n, Ct]): the float64 entry, sum_j |x_j c_j| in float64, and the float32 sequence
    acc = 0; acc = acc + x_j * c_j (j ascending over CsEff).  Where the tap lies in the padding all three are 0.
    Groups: channel ct of group g reads input channels g * Cg + m* Cs + j, the same code book in every group."""
    x = np.asarray(x, np.float32)
    ctrd, picks = params["ctrd"], params["picks"]
    M, K, Cs = ctrd.shape
    Ct = picks.shape[0]
    cse = np.array(cs_eff(kind, g, M, Cs))
    words = ctrd[picks[:, 2], picks[:, 3]]                                     # [Ct, Cs], zero beyond CsEff
    live = np.arange(Cs)[None, :] < cse[picks[:, 2]][:, None]                   # [Ct, Cs]
    if kind == "fc":
        idx = np.minimum(picks[:, 2:3] * Cs + np.arange(Cs)[None, :], g["D"] - 1)
        want64, mag, seq = _dot(np.where(live[None], x[:, idx], np.float32(0)), words[None])
        return want64, mag, seq
    n, H, W, Cin = x.shape
    knl, s, pad, grp = g["knl"], g["stride"], g["pad"], g["grp"]
    Ho, Wo = out_hw(g)
    Cg, Ctg = Cin // grp, Ct // grp
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin), np.float32)               # zero padding: products there are exact zeros
    xp[:, pad:pad + H, pad:pad + W] = x
    want64 = np.zeros((n, Ho, Wo, Ct), np.float64)
    mag = np.zeros((n, Ho, Wo, Ct), np.float64)
    seq = np.zeros((n, Ho, Wo, Ct), np.float32)
    for ct in range(Ct):
        kh, kw, m, _ = picks[ct]
        c0 = (ct // Ctg) * Cg + m * Cs
        sl = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, c0:c0 + cse[m]]
        want64[..., ct], mag[..., ct], seq[..., ct] = _dot(sl, words[ct, :cse[m]])
        inside_h = (np.arange(Ho) * s - pad + kh >= 0) & (np.arange(Ho) * s - pad + kh < H)
        inside_w = (np.arange(Wo) * s - pad + kw >= 0) & (np.arange(Wo) * s - pad + kw < W)
        assert ((mag[0, :, :, ct] > 0) == (inside_h[:, None] & inside_w[None, :])).all()
    return want64, mag, seq


def _dot(xs, cs):
    """xs [..., J] float32, cs broadcastable [..., J] float32 -> float64 dot, float64 sum of |products|, float32 sequence."""
    xs, cs = np.asarray(xs, np.float32), np.asarray(cs, np.float32)
    p64 = xs.astype(np.float64) * cs.astype(np.float64)
    a = np.abs(p64)
    nz = a[a > 0]
    assert nz.size == 0 or (nz.min() >= LO and nz.max() <= HI), "probe products outside [2^-60, 2^60]"
    acc = np.zeros(np.broadcast(xs, cs).shape[:-1], np.float32)
    for j in range(xs.shape[-1]):
        acc = acc + xs[..., j] * cs[..., j]                                     # numpy: one rounding per operation, no FMA
    return p64.sum(-1), a.sum(-1), acc


# ---------------------------------------------------------------- the checker ----
def check(y, want64, mag, n_terms, extra=0.0, relu=False, what=""):
    """Assert |y - want64| <= (gamma_n + extra) * mag for every element (n_terms = 1: one rounding, u * mag), exact zeros
    where mag = 0; relu: y is max(entry, 0) (the clamp does not increase the distance to max(want64, 0)).  Returns the
    worst err / bound over the informative elements (mag > 0)."""
    y = np.asarray(y)
    assert y.shape == want64.shape == mag.shape, (y.shape, want64.shape, mag.shape)
    assert np.isfinite(y).all(), "%s: non-finite output" % what
    w = np.maximum(want64, 0.0) if relu else want64
    err = np.abs(y.astype(np.float64) - w)
    bound = ((U if n_terms == 1 else gamma(n_terms)) + extra) * mag
    dead = mag == 0
    assert not (dead & (y != 0)).any(), "%s: %d non-zero outputs where the tap lies in the padding" % (what, int((dead & (y != 0)).sum()))
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(dead, 0.0, err / np.where(dead, 1.0, bound))), err.shape)
        raise AssertionError("%s: %d of %d entries beyond the bound; worst at %r: got %.9g want %.17g err %.3g bound %.3g"
                             % (what, int(bad.sum()), err.size, i, float(y[i]), float(w[i]), float(err[i]), float(bound[i])))
    return float((err[~dead] / bound[~dead]).max()) if (~dead).any() else 0.0


# ---------------------------------------------------------------- dense sums ----
def dense_count(kind, g, M, Cs):
    """Roundings behind one output element of a layer with ordinary parameters: an entry is a chain of CsEff fused multiply-adds
    (or CsEff products and CsEff - 1 additions), the output a float32 sum of knl^2 M entries and the bias in any order, so
    |y - want64| <= gamma(knl^2 M + CsEff + 1) * mag holds for every summation order, chunking and builder of the library."""
    _, knl, _ = _dims(kind, g)
    return knl * knl * M + max(cs_eff(kind, g, M, Cs)) + 1


def dense_expected(kind, g, x, params):
    """(want64, mag) of a layer with ordinary parameters (synth.make_params: bias, ctrd [M][K][Cs], asmt) on input x (layout of
    `activations`), shaped like the layer's output [n, Ho, Wo, Ct] (FC: [n, Ct]), both float64:
        want64 = bias + sum over the taps inside the map, over m, of <x_m, ctrd[m][asmt]>,   mag = |bias| + sum |x_j c_j|.
    Plain numpy float64 throughout (every product of two float32 values is exact in float64)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    bias = np.asarray(params["bias"], np.float32).astype(np.float64)
    ctrd = np.asarray(params["ctrd"], np.float32).astype(np.float64)
    asmt = np.asarray(params["asmt"]).astype(np.int64)
    M, K, Cs = ctrd.shape
    cse = cs_eff(kind, g, M, Cs)
    Ct = bias.shape[0]
    if kind == "fc":
        n = x.shape[0]
        want = np.tile(bias, (n, 1))
        mag = np.tile(np.abs(bias), (n, 1))
        asmt = asmt.reshape(Ct, M)
        for m in range(M):
            xm, cm = x[:, m * Cs:m * Cs + cse[m]], ctrd[m, :, :cse[m]]
            T, A = xm @ cm.T, np.abs(xm) @ np.abs(cm).T                          # [n, K]
            want += T[:, asmt[:, m]]
            mag += A[:, asmt[:, m]]
        return want, mag
    n, H, W, Cin = x.shape
    knl, s, pad, grp = g["knl"], g["stride"], g["pad"], g["grp"]
    Ho, Wo = out_hw(g)
    Cg, Ctg = Cin // grp, Ct // grp
    asmt = asmt.reshape(Ct, knl, knl, M)
    want = np.tile(bias, (n, Ho, Wo, 1))
    mag = np.tile(np.abs(bias), (n, Ho, Wo, 1))
    for gi in range(grp):
        cts = slice(gi * Ctg, (gi + 1) * Ctg)
        for m in range(M):
            c0 = gi * Cg + m * Cs
            xm, cm = x[..., c0:c0 + cse[m]], ctrd[m, :, :cse[m]]
            T, A = xm @ cm.T, np.abs(xm) @ np.abs(cm).T                          # [n, H, W, K]: the pixel tables of sub-space m
            for kh in range(knl):
                ho = [o for o in range(Ho) if 0 <= o * s - pad + kh < H]
                for kw in range(knl):
                    wo = [o for o in range(Wo) if 0 <= o * s - pad + kw < W]
                    if not ho or not wo:
                        continue
                    hi = np.array(ho)[:, None] * s - pad + kh
                    wi = np.array(wo)[None, :] * s - pad + kw
                    a = asmt[cts, kh, kw, m]
                    want[:, ho[0]:ho[-1] + 1, wo[0]:wo[-1] + 1, cts] += T[:, hi, wi][..., a]
                    mag[:, ho[0]:ho[-1] + 1, wo[0]:wo[-1] + 1, cts] += A[:, hi, wi][..., a]
    return want, mag


def dense_check(y, want64, mag, n_terms, what=""):
    """Assert |y - want64| <= gamma(n_terms) * mag for every element; returns the worst err / bound."""
    y = np.asarray(y)
    assert y.shape == want64.shape == mag.shape, (y.shape, want64.shape, mag.shape)
    assert np.isfinite(y).all(), "%s: non-finite output" % what
    assert (mag > 0).all()
    err = np.abs(y.astype(np.float64) - want64)
    ratio = err / (gamma(n_terms) * mag)
    if (ratio > 1.0).any():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError("%s: %d of %d outputs beyond the bound; worst at %r: got %.9g want %.17g err %.3g bound %.3g"
                             % (what, int((ratio > 1.0).sum()), ratio.size, i, float(y[i]), float(want64[i]), float(err[i]),
                                float(gamma(n_terms) * mag[i])))
    return float(ratio.max())


def informative_share(mag):
    return float((mag > 0).mean())


def covered(kind, g, M, K, rounds):
    """(pairs [M, K] bool: (m, k) named by some round as a non-silent word; taps [knl, knl] bool; pairs_inside [M, K] bool:
    named at least once with a tap that lies inside the map for some output position)."""
    _, knl, _ = _dims(kind, g)
    pairs = np.zeros((M, K), bool)
    inside = np.zeros((M, K), bool)
    taps = np.zeros((knl, knl), bool)
    for rd in rounds:
        p = picks_of_round(kind, g, M, K, rd)
        pairs[p[:, 2], p[:, 3]] = True
        taps[p[:, 0], p[:, 1]] = True
        if kind == "conv":
            Ho, Wo = out_hw(g)
            ok = np.array([_tap_inside(g, kh, g["H"], Ho) and _tap_inside(g, kw, g["W"], Wo) for kh, kw in p[:, :2]])
        else:
            ok = np.ones(len(p), bool)
        inside[p[ok, 2], p[ok, 3]] = True
    return pairs, taps, inside


def _tap_inside(g, k, size, n_out):
    pos = np.arange(n_out) * g["stride"] - g["pad"] + k
    return bool(((pos >= 0) & (pos < size)).any())


# ---------------------------------------------------------------- the shapes the probes run on ----
# name -> (kind, geometry, M, K, Cs, max_rounds).  tests/test_table_probe_cpu.py pins the helper to the oracle on every one of
# them and checks the schedules' coverage; tests/test_gpu_table_probe.py sends them through the kernel families.
SHAPES = {
    # AlexNet conv2: 2 groups x 128 channels, 5x5 / 1, pad 2, six sub-spaces of 8 dims, on a 13x13 map
    "alex_conv2": ("conv", conv_geom(13, 13, 96, 5, 1, 2, 2, 256), 6, 128, 8, None),
    "c3_64": ("conv", conv_geom(13, 13, 16, 3, 1, 1, 1, 64), 2, 128, 8, None),
    "c3_128": ("conv", conv_geom(13, 13, 16, 3, 1, 1, 1, 128), 2, 128, 8, None),
    "partial": ("conv", conv_geom(11, 11, 20, 3, 1, 1, 1, 64), 3, 128, 8, None),          # last sub-space: 4 of 8 dims
    "cs4_2x2": ("conv", conv_geom(11, 11, 16, 2, 1, 0, 1, 128), 4, 128, 4, None),
    "rgb7": ("conv", conv_geom(31, 31, 3, 7, 2, 0, 1, 32), 1, 128, 8, None),              # one 3-dim sub-space
    "s5x5_2": ("conv", conv_geom(21, 21, 16, 5, 2, 2, 1, 96), 2, 128, 8, None),
    "c192": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 192), 2, 128, 8, None),
    "c256": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 256), 2, 128, 8, None),
    "c384": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 384), 2, 128, 8, None),
    "c512": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 512), 2, 128, 8, None),
    "c256_cs4": ("conv", conv_geom(7, 7, 8, 3, 1, 1, 1, 256), 2, 128, 4, None),
    "k10": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 64), 2, 10, 8, None),
    "k64": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 64), 2, 64, 8, None),
    "k200": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 64), 2, 200, 8, None),
    "k256": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 64), 2, 256, 8, None),
    # decoded first layers: AlexNet conv1 on a 67x71 input, four input channels, one input channel
    "alex_conv1": ("conv", conv_geom(67, 71, 3, 11, 4, 0, 1, 96), 1, 128, 8, None),
    "dec4": ("conv", conv_geom(28, 30, 4, 4, 2, 0, 1, 192), 1, 128, 4, None),
    "dec1": ("conv", conv_geom(15, 17, 1, 3, 1, 0, 1, 96), 1, 128, 8, None),
    # FC: 31 x 128 pairs over 768 channels (six rounds); AlexNet fc6 in ONE thinned round (4096 of 2304 x 31 pairs, every m,
    # every k); a 200-channel layer; a classifier with 16 code words of one dim
    "fc512": ("fc", fc_geom(512, 768), 128, 32, 4, None),
    "fc6": ("fc", fc_geom(9216, 4096), 2304, 32, 4, 1),
    "fc200": ("fc", fc_geom(256, 200), 64, 32, 4, None),
    "fc_k16": ("fc", fc_geom(256, 1000), 256, 16, 1, None),
    # the few-image kernels (qcnn_small.hip): the smallest shapes at which each sub-space chunk, stage group and tile edge of
    # k_conv_small / k_fc_small is live.  SMALL_REACH states what each one reaches; tests/test_small_plan_cpu.py re-derives it from
    # the launchers' tile / chunk rules
    "sm_m18": ("conv", conv_geom(7, 7, 70, 3, 1, 1, 1, 64), 18, 128, 4, None),            # last sub-space: 2 of 4 dims
    "sm_5x5_m12": ("conv", conv_geom(9, 9, 96, 5, 1, 2, 1, 128), 12, 128, 8, None),
    "sm_k32_m24": ("conv", conv_geom(7, 7, 96, 5, 1, 2, 1, 128), 24, 32, 4, None),
    "sm_k40": ("conv", conv_geom(7, 7, 16, 3, 1, 1, 1, 64), 4, 40, 4, None),
    "sm_k24": ("conv", conv_geom(7, 7, 32, 3, 1, 1, 1, 64), 8, 24, 4, None),
    "sm_k10_m6": ("conv", conv_geom(7, 7, 48, 3, 1, 1, 1, 64), 6, 10, 8, None),
    "sm_k100_m6": ("conv", conv_geom(7, 7, 48, 3, 1, 1, 1, 64), 6, 100, 8, None),
    "sm_ct400_g2": ("conv", conv_geom(7, 5, 24, 3, 2, 1, 2, 400), 3, 128, 4, None),
    "sm_ct24": ("conv", conv_geom(5, 6, 16, 1, 2, 0, 1, 24), 2, 64, 8, None),
    "sm_15_m2": ("conv", conv_geom(20, 20, 16, 15, 1, 0, 1, 16), 2, 128, 8, None),
    "sm_15_k64": ("conv", conv_geom(20, 20, 16, 15, 1, 0, 1, 128), 2, 64, 8, None),
    "sm_nchw_m2": ("conv", conv_geom(12, 12, 4, 3, 1, 1, 1, 16), 2, 128, 2, None),
    # FC: thinned to the fewest rounds that name every m (ceil(M / Ct); the k shift of picks_of_round then names every k too):
    # 23 of 698 rounds = 3.3 % of fc_m900's pairs, 8 of 147 = 5.5 % of fc_k128's, 57 of 844 = 6.8 % of fc_k16_m1800's
    "fc_m900": ("fc", fc_geom(3600, 40), 900, 32, 4, 23),
    "fc_k128": ("fc", fc_geom(920, 200), 230, 128, 4, 8),
    "fc_k20": ("fc", fc_geom(240, 48), 60, 20, 4, None),
    "fc_k16_m1800": ("fc", fc_geom(1800, 32), 1800, 16, 1, 57),
    # the decoded kernels (qcnn_decoded.hip): the smallest shapes at which each launch variant is live.  DEC_REACH states what
    # each one reaches; tests/test_decoded_cases_cpu.py re-derives it from the launchers' rules.
    # First layers read in place (pad 0, Ct % 96 == 0, one sub-space of Cin <= 4 dims)
    "dn_k5": ("conv", conv_geom(9, 10, 3, 5, 1, 0, 1, 96), 1, 128, 4, None),
    "dn_k5_k10": ("conv", conv_geom(9, 10, 3, 5, 1, 0, 1, 96), 1, 10, 4, None),           # a conv stage row is the code word itself,
    "dn_k5_k100": ("conv", conv_geom(9, 10, 3, 5, 1, 0, 1, 96), 1, 100, 4, None),         # whatever K is
    "dn_k4_s5": ("conv", conv_geom(9, 15, 1, 4, 5, 0, 1, 96), 1, 128, 4, None),
    "dn_k6": ("conv", conv_geom(8, 22, 2, 6, 2, 0, 1, 96), 1, 128, 4, None),
    "dn_k7_ct192": ("conv", conv_geom(9, 13, 3, 7, 2, 0, 1, 192), 1, 128, 4, None),
    "dn_k9": ("conv", conv_geom(9, 9, 1, 9, 1, 0, 1, 96), 1, 128, 4, None),
    "dn_flat_k9": ("conv", conv_geom(10, 11, 4, 9, 1, 0, 1, 96), 1, 128, 4, None),
    "dn_f32_only": ("conv", conv_geom(8, 13, 4, 7, 3, 0, 1, 192), 1, 128, 4, None),
    "dn_1x1": ("conv", conv_geom(2, 5, 1, 1, 1, 0, 1, 96), 1, 128, 4, None),
    "dn_ct288": ("conv", conv_geom(6, 7, 3, 3, 1, 0, 1, 288), 1, 128, 4, None),
    # panel form: 5 x 7 = 35 output positions, so that the position groups of 2, 4 and 6 all have a ragged tail
    "dp_pad_k3": ("conv", conv_geom(5, 7, 3, 3, 1, 1, 1, 64), 1, 128, 4, None),
    "dp_pad_c1": ("conv", conv_geom(5, 7, 1, 3, 1, 1, 1, 96), 1, 128, 4, None),
    "dp_1x1": ("conv", conv_geom(5, 7, 3, 1, 1, 0, 1, 32), 1, 128, 4, None),
    "dp_k7_ct32": ("conv", conv_geom(15, 19, 1, 7, 2, 0, 1, 32), 1, 128, 4, None),
    "dp_k5_ct64": ("conv", conv_geom(9, 11, 2, 5, 1, 0, 1, 64), 1, 128, 4, None),
    "dp_k2_ct96": ("conv", conv_geom(6, 8, 2, 2, 1, 0, 1, 96), 1, 128, 4, None),
    "dp_k4_ct160": ("conv", conv_geom(8, 10, 1, 4, 1, 0, 1, 160), 1, 128, 4, None),
    "dp_half_items": ("conv", conv_geom(48, 48, 2, 3, 1, 0, 1, 96), 1, 128, 4, None),     # (dense sums only, at 128 images)
    # decoded FC (Cs = 1, M = D, D % 64 == 0), thinned to ceil(M / Ct) rounds — every m, and through the k shift every k: with the
    # k = 0 rounds 15.3 % of fcd_d64's pairs, 20.0 % of fcd_d128_k10's, 8.6 / 2.4 % of fcd_d192_k24's / fcd_d320_k100's, 12.5 - 13.0 %
    # of the four long ones'; fcd_d64_k128 (64 sub-spaces for 127 words) needs 43 of its 85 rounds to name every k: 51.6 %
    "fcd_d64": ("fc", fc_geom(64, 40), 64, 16, 1, 2),
    "fcd_d128_k10": ("fc", fc_geom(128, 64), 128, 10, 1, 2),
    "fcd_d192_k24": ("fc", fc_geom(192, 66), 192, 24, 1, 3),             # (an odd channel count is refused at load: two live channels)
    "fcd_d320_k100": ("fc", fc_geom(320, 130), 320, 100, 1, 3),
    "fcd_d64_k128": ("fc", fc_geom(64, 96), 64, 128, 1, 43),
    "fcd_d512": ("fc", fc_geom(512, 40), 512, 16, 1, 13),
    "fcd_d640": ("fc", fc_geom(640, 40), 640, 16, 1, 16),
    "fcd_d768": ("fc", fc_geom(768, 40), 768, 16, 1, 20),
    "fcd_d2048": ("fc", fc_geom(2048, 40), 2048, 16, 1, 52),
    # the panel conv families (k_conv_aprx tile / sliding, k_conv_sym, k_conv_sym8, k_conv_half8, split tiles + k_conv_sum) on DENSE
    # sums: a deep sub-space axis (hundreds of stages per tile) on maps of about 7 x 10, knl^2 M <= 1200 everywhere.  PANEL_REACH
    # states what each one reaches; tests/test_panel_cases_cpu.py re-derives it from the planner's and the launchers' rules
    "pn_deep": ("conv", conv_geom(7, 10, 128, 3, 1, 1, 1, 128), 32, 128, 4, None),          # 288 terms; every family
    "pn_c192": ("conv", conv_geom(7, 9, 64, 3, 1, 1, 1, 192), 8, 128, 8, None),
    "pn_c256_cs4": ("conv", conv_geom(7, 10, 64, 3, 1, 1, 1, 256), 16, 128, 4, None),
    "pn_c384": ("conv", conv_geom(7, 9, 64, 3, 1, 1, 1, 384), 8, 128, 8, None),
    "pn_c512": ("conv", conv_geom(7, 10, 128, 3, 1, 1, 1, 512), 16, 128, 8, None),
    "pn_grp2_5x5": ("conv", conv_geom(11, 7, 128, 5, 1, 2, 2, 256), 8, 128, 8, None),       # alex_conv2 with a deeper axis: 200 terms
    "pn_s2_5x5": ("conv", conv_geom(13, 9, 128, 5, 2, 2, 1, 128), 16, 128, 8, None),        # 400 terms; 7 x 5 outputs
    "pn_k32_m18": ("conv", conv_geom(7, 10, 72, 3, 1, 1, 1, 64), 18, 32, 4, None),          # G = 4, last stage of a pixel: 2 sub-spaces
    "pn_k10_m32": ("conv", conv_geom(7, 10, 128, 3, 1, 1, 1, 32), 32, 10, 4, None),         # G = 12, last stage: 8
    "pn_k64_m9": ("conv", conv_geom(7, 9, 72, 3, 1, 1, 1, 96), 9, 64, 8, None),             # G = 2, last stage: 1
    "pn_partial": ("conv", conv_geom(7, 9, 68, 3, 1, 1, 1, 64), 9, 128, 8, None),           # last sub-space: 4 of 8 dims
    "pn_k200": ("conv", conv_geom(7, 10, 64, 3, 1, 1, 1, 64), 16, 200, 4, None),            # two pseudo sub-spaces per sub-space
    "pn_k256": ("conv", conv_geom(7, 10, 128, 3, 1, 1, 1, 64), 16, 256, 8, None),           # three
}

# What the few-image launchers must choose for each of those shapes (qk_conv_small: output tile, sub-spaces per table chunk,
# channels per workgroup, channel chunks per group; qk_fc_small: sub-spaces per table chunk) for the case to reach the branch it
# is there for: conv (TH, TW, MC, CH, channel chunks per group, G), FC (MC, G).
SMALL_REACH = {
    "sm_m18": (2, 2, 17, 64, 1, 1),           # sub-space chunks 17 + 1: m0 > 0, a ragged last chunk
    "sm_5x5_m12": (2, 2, 7, 128, 1, 1),       # chunks 7 + 5; odd map: ragged 2x2 tiles
    "sm_k32_m24": (2, 2, 19, 128, 1, 4),      # chunks 19 + 5: the second one starts mid-stage (19 mod 4 = 3)
    "sm_k40": (2, 2, 4, 64, 1, 3),            # G = 3: no power of two; scalar build with fewer (m, k) pairs than threads
    "sm_k24": (2, 2, 8, 64, 1, 5),            # G = 5
    "sm_k10_m6": (2, 2, 6, 64, 1, 12),        # G = 12, m >= 4
    "sm_k100_m6": (2, 2, 6, 64, 1, 1),        # scalar build with 600 >= 512 pairs, G = 1, K no multiple of 16
    "sm_ct400_g2": (2, 2, 3, 128, 2, 1),      # 200 channels per group: two channel chunks, the second with 72 live lanes
    "sm_ct24": (2, 2, 2, 32, 1, 2),           # 8 idle lanes, 16 position slots for 4 positions
    "sm_15_m2": (1, 1, 1, 32, 1, 1),          # the mc == 1 gather at m0 = 1
    "sm_15_k64": (1, 1, 1, 128, 1, 2),        # ... with mi = m0 % G = 1
    "sm_nchw_m2": (2, 2, 2, 32, 1, 1),
    "fc_m900": (896, 4), "fc_k128": (224, 1), "fc_k20": (60, 6), "fc_k16_m1800": (1792, 8),
}

# a 17x17 window with K = 128 on a 20x20 map: 289 pixels x (128 + 8) floats + 289 x 32 assignment bytes do not fit the few-image
# kernel's LDS table at any tile, so a forward of one to three images hands this layer to the panel kernels
SMALL_FALL_THROUGH = ("conv", conv_geom(20, 20, 8, 17, 1, 0, 1, 32), 1, 128, 8, None)


# What the decoded launchers must choose for each of those shapes for the case to reach the branch it is there for.
#   dn_*: (in-place order under QCNN_OPT_DEC_BF16SPLIT: "runs" / "flat" / "f32" = no split form, runs per kernel row, padded k of the
#          split kernel (0: none), padded k of the f32 in-place kernel, channel chunks, (Ho, Wo));
#   dp_*: (S, NS, T = knl NS, instantiation <CT, PW, PADDED, R, IT> at more than 16 live images, the one at <= 16, channel chunks);
#         T % R follows from them;
#   fcd_*: (steps of four k per wave with one slice, G, 64-channel blocks, live channels of the last block, k slices under
#          QCNN_OPT_SPLIT at one panel).
DEC_REACH = {
    "dn_k5": ("runs", 2, 128, 80, 1, (5, 6)),            # second run at column 1: three repeated columns; 30 runs in 32 slots
    "dn_k5_k10": ("runs", 2, 128, 80, 1, (5, 6)),
    "dn_k5_k100": ("runs", 2, 128, 80, 1, (5, 6)),
    "dn_k4_s5": ("runs", 1, 32, 16, 1, (2, 3)),          # one run per row; ONE step, four of eight run slots live; column 14 unread
    "dn_k6": ("runs", 2, 96, 80, 1, (2, 9)),             # overlap of two columns; 24 runs = exactly three steps
    "dn_k7_ct192": ("runs", 2, 192, 160, 2, (2, 4)),     # overlap of one column; two channel chunks
    "dn_k9": ("runs", 3, 128, 96, 1, (1, 1)),            # runs at columns 0, 4, 5
    "dn_flat_k9": ("flat", 0, 352, 336, 1, (2, 3)),      # run order does not fit the LDS: Kr = 324 in Kb = 352
    "dn_f32_only": ("f32", 0, 0, 208, 2, (1, 3)),        # neither split order fits: the f32 kernel under both option values
    "dn_1x1": ("flat", 0, 32, 16, 1, (2, 5)),            # Kr = 1: 15 / 31 padded k
    "dn_ct288": ("flat", 0, 32, 32, 3, (4, 5)),          # knl < 4: flat order; three channel chunks
    "dp_pad_k3": (80, 3, 9, (4, 1, True, 2, 4), (2, 4, True, 2, 1), 1),
    "dp_pad_c1": (112, 1, 3, (2, 1, True, 3, 4), (2, 4, True, 2, 1), 3),
    "dp_1x1": (48, 1, 1, (2, 1, True, 3, 4), (2, 4, True, 2, 1), 1),
    "dp_k7_ct32": (48, 2, 14, (2, 2, False, 3, 4), (2, 6, False, 3, 1), 1),
    "dp_k5_ct64": (80, 3, 15, (4, 1, False, 3, 4), (4, 4, False, 3, 1), 1),
    "dp_k2_ct96": (112, 1, 2, (6, 1, False, 2, 4), (6, 2, False, 3, 1), 1),
    "dp_k4_ct160": (176, 1, 4, (2, 2, False, 3, 4), (2, 6, False, 3, 1), 5),
    "dp_half_items": (112, 2, 6, (3, 1, False, 3, 4), (6, 2, False, 3, 1), 2),     # 4232 items at 128 images: half-items of 48 channels
    "fcd_d64": (1, 8, 1, 40, 1), "fcd_d128_k10": (2, 12, 1, 64, 1), "fcd_d192_k24": (3, 5, 2, 2, 1),
    "fcd_d320_k100": (5, 1, 3, 2, 1), "fcd_d64_k128": (1, 1, 2, 32, 1),
    "fcd_d512": (8, 8, 1, 40, 2), "fcd_d640": (10, 8, 1, 40, 2), "fcd_d768": (12, 8, 1, 40, 2), "fcd_d2048": (32, 8, 1, 40, 8),
}
DEC_NCHW_SHAPES = sorted(n for n in DEC_REACH if n.startswith("dn_"))
DEC_PANEL_SHAPES = sorted(n for n in DEC_REACH if n.startswith("dp_"))
DEC_FC_SHAPES = sorted(n for n in DEC_REACH if n.startswith("fcd_"))
DEC_BATCHES = (131, 70, 17, 16, 5)       # two panels with a ragged second one; two image halves; 17 and 16: either side of IT = 4 / 1
DEC_NCHW_FEW = (3, 1)                    # one to three images still take the in-place kernel

# Shapes that must NOT decode: more than 128 code words become pseudo sub-spaces, so the kernels see M = 2 for one sub-space
# (conv) and M = 2 D (FC); the panel table kernel runs and reports its own code
DEC_NOT = {
    "nd_conv_k200": ("conv", conv_geom(9, 10, 3, 5, 1, 0, 1, 96), 1, 200, 4, None),
    "nd_fc_k130": ("fc", fc_geom(64, 40), 64, 130, 1, None),
}


# What the planner and the launchers of the panel conv kernels must choose for each pn_* shape for the case to reach the seam it is
# there for.  stage = (G = sub-spaces per LUT stage, sub-spaces of a pixel's LAST stage, stages per source pixel — pseudo
# sub-spaces counted); live = the families that must run it, by the planner's names, with
#   tile / sym16 / sym8:          (channels per wave, th, tw, channel chunks per group, (tilesY, tilesX), stages of the heaviest tile)
#   half8:                        (channels per wave, th, tw, wave sets, chunks, (tilesY, tilesX), stages of the heaviest tile)
#   slide16 / sym8_slide:         (channels per wave, slots, columns per strip, chunks, strips, stages of the widest whole-column strip)
#   half8_slide:                  (channels per wave, slots, columns per strip, wave sets, chunks, strips, stages of that strip)
#   split_tile / split_sym8:      (slices Z, first split tile rank) at ONE panel under QCNN_OPT_SPLIT (the batch of 125 images)
# dead = the families that must report "not eligible" (cost 0).  Every kernel keeps two LUT stage buffers and two (16-wave) or three
# (eight-wave, half-panel) program-row buffers: each stage count below wraps all of them many times.
PANEL_REACH = {
    # every family and both split forms; 288 terms of 4 dims; 128 channels per group is the one symmetric shape.  Clipped last tiles
    # in both axes for 2x2 (rows), 2x3 and 3x4; 3 x 3 half-panel tiles: interior / edge / corner ranks; Z = 8 cuts 480 stages at
    # 60, 120, ... — inside a pixel's 32 stages; Z = 6 does not divide 640
    "pn_deep": dict(stage=(1, 1, 32),
                    live={"tile": (12, 1, 3, 1, (7, 4), 480), "slide16": (12, 3, 1, 1, 10, 672), "sym16": (8, 2, 2, 1, (4, 5), 512),
                          "sym8": (16, 2, 3, 1, (4, 4), 640), "sym8_slide": (16, 3, 2, 1, 5, 896), "half8": (32, 3, 4, 2, 1, (3, 3), 960),
                          "half8_slide": (32, 3, 4, 2, 1, 3, 1344), "split_tile": (8, 0), "split_sym8": (6, 0)},
                    dead=()),
    # the channel configurations of the eight-wave (24 / 32 / 48 channels per wave, two chunks at 512) and the half-panel kernel
    # (cases 192 / 256 / 384 / 512) and their sliding forms, Cs = 8 and 4; 7 x 9 maps clip the 1x2, 2x2 and 2x4 tiles in both axes
    "pn_c192": dict(stage=(1, 1, 8),
                    live={"tile": (16, 1, 2, 1, (7, 5), 96), "slide16": (12, 3, 1, 2, 9, 168), "sym8": (24, 2, 2, 1, (4, 5), 128),
                          "sym8_slide": (24, 3, 1, 1, 9, 168), "half8": (48, 2, 4, 2, 1, (4, 3), 192),
                          "half8_slide": (48, 3, 2, 2, 1, 5, 224), "split_tile": (5, 0), "split_sym8": (6, 0)},
                    dead=("sym16",)),
    "pn_c256_cs4": dict(stage=(1, 1, 16),
                        live={"tile": (24, 1, 1, 1, (7, 10), 144), "slide16": (12, 3, 1, 2, 10, 336), "sym8": (32, 1, 3, 1, (7, 4), 240),
                              "sym8_slide": (32, 3, 1, 1, 10, 336), "half8": (32, 2, 3, 1, 1, (4, 4), 320),
                              "half8_slide": (32, 3, 2, 1, 1, 5, 448), "split_tile": (3, 0), "split_sym8": (6, 0)},
                        dead=("sym16",)),
    "pn_c384": dict(stage=(1, 1, 8),
                    live={"tile": (32, 1, 1, 1, (7, 9), 72), "slide16": (12, 3, 1, 3, 9, 168), "sym8": (48, 1, 2, 1, (7, 5), 96),
                          "sym8_slide": (24, 3, 1, 2, 9, 168), "half8": (48, 2, 2, 1, 1, (4, 5), 128),
                          "half8_slide": (48, 3, 1, 1, 1, 9, 168), "split_tile": (4, 0), "split_sym8": (5, 0)},
                    dead=("sym16",)),
    "pn_c512": dict(stage=(1, 1, 16),
                    live={"tile": (24, 1, 1, 2, (7, 10), 144), "slide16": (12, 3, 1, 4, 10, 336), "sym8": (32, 1, 3, 2, (7, 4), 240),
                          "sym8_slide": (32, 3, 1, 2, 10, 336), "half8": (64, 1, 3, 1, 1, (7, 4), 240),
                          "half8_slide": (64, 3, 1, 1, 1, 10, 336), "split_tile": (3, 0), "split_sym8": (4, 0)},
                    dead=("sym16",)),
    # two groups, 5x5 / pad 2: five slots — the 16-wave sliding form with 6 channels per wave in two chunks, the eight-wave one with
    # 16; no half-panel sliding form; 4 x 2 half-panel tiles: the row-major tile numbering; 2x2 tiles clipped in both axes
    "pn_grp2_5x5": dict(stage=(1, 1, 8),
                        live={"tile": (12, 1, 3, 1, (11, 3), 240), "slide16": (6, 5, 1, 2, 7, 440), "sym16": (8, 2, 2, 1, (6, 4), 288),
                              "sym8": (16, 2, 3, 1, (6, 3), 288), "sym8_slide": (16, 5, 1, 1, 7, 440),
                              "half8": (32, 3, 4, 2, 1, (4, 2), 336), "split_tile": (4, 0), "split_sym8": (6, 0)},
                        dead=("half8_slide",)),
    # 5x5 / stride 2 / pad 2 on an odd 13 x 9 map: three slots, every sliding form, the last two-column strip one column wide; two
    # tiles per row: the row-major numbering of the 16-wave, eight-wave and half-panel tile kernels
    "pn_s2_5x5": dict(stage=(1, 1, 16),
                      live={"tile": (12, 1, 3, 1, (7, 2), 560), "slide16": (12, 3, 1, 1, 5, 1040), "sym16": (8, 2, 2, 1, (4, 3), 784),
                            "sym8": (16, 2, 3, 1, (4, 2), 784), "sym8_slide": (16, 3, 2, 1, 3, 1456),
                            "half8": (32, 3, 4, 2, 1, (3, 2), 1296), "half8_slide": (32, 3, 4, 2, 1, 2, 1872), "split_tile": (8, 0),
                            "split_sym8": (6, 0)},
                      dead=()),
    # K < 128: G sub-spaces per stage, M % G != 0 — the last stage of every pixel is ragged; Z = 3 cuts between the stage groups of a
    # pixel.  Only the 16-wave tile kernel takes them (the sliding program is built for K = 128 alone); tiles 2x3, 2x4, 2x2
    "pn_k32_m18": dict(stage=(4, 2, 5), live={"tile": (6, 2, 3, 1, (4, 4), 100), "split_tile": (3, 0)},
                       dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide")),
    "pn_k10_m32": dict(stage=(12, 8, 3), live={"tile": (4, 2, 4, 1, (4, 3), 72), "split_tile": (3, 0)},
                       dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide")),
    "pn_k64_m9": dict(stage=(2, 1, 5), live={"tile": (8, 2, 2, 1, (4, 5), 80), "split_tile": (3, 0)},
                      dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide")),
    # 4 of 8 dims in the last sub-space: operand masks; no eight-wave, half-panel or symmetric form; two-column strips of the 16-wave
    # sliding form, the last one a single column
    "pn_partial": dict(stage=(1, 1, 9), live={"tile": (6, 2, 3, 1, (4, 3), 180), "slide16": (6, 3, 2, 1, 5, 252), "split_tile": (8, 0)},
                       dead=("sym16", "sym8", "sym8_slide", "half8", "half8_slide")),
    # K > 128: two / three pseudo sub-spaces per sub-space, the exact-builder tile kernel under every option
    "pn_k200": dict(stage=(1, 1, 32), live={"tile": (6, 2, 3, 1, (4, 4), 640)},
                    dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide")),
    "pn_k256": dict(stage=(1, 1, 48), live={"tile": (6, 2, 3, 1, (4, 4), 960)},
                    dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide")),
}
PANEL_BATCH, PANEL_HALF_BATCHES, PANEL_SPLIT_BATCH = 131, (70, 5), 125     # a full panel + a ragged one of three; half panels; one panel


# ---------------------------------------------------------------- maps smaller than the kernel and the tile ----
# The tg_* shapes: maps of a few pixels — the last layers of a network on a small input — through every conv family (TINY_REACH;
# tests/test_tiny_cases_cpu.py re-derives it and proves every workgroup a stage, tests/test_gpu_tiny_cases.py runs them on dense sums).
# Kept out of SHAPES: the probe tests are parametrised over SHAPES and ask that half of a probe's outputs be informative, which a
# 1 x 1 map under a 3x3 kernel (one live tap of nine) cannot give.  Base quantisation: 32 input channels in four sub-spaces of 8 dims,
# K = 128, one group, 128 channels — the tile, 16-wave symmetric, eight-wave and half-panel families are all eligible.
def _tg(H, W, knl, stride, pad, Cin=32, Ct=128, grp=1, M=4, K=128, Cs=8):
    return ("conv", conv_geom(H, W, Cin, knl, stride, pad, grp, Ct), M, K, Cs, None)


TINY_BASE = {
    "tg_1x1": _tg(1, 1, 3, 1, 1),        # one live tap of nine; every tile larger than the map in both axes
    "tg_row": _tg(1, 4, 3, 1, 1),        # Ho = 1
    "tg_col": _tg(7, 1, 3, 1, 1),        # Wo = 1; the three sliding forms (two segments), their column strip wider than the map
    "tg_k5": _tg(2, 3, 5, 1, 2),         # kernel larger than the map in both axes: every window clipped on both sides
    "tg_pad2": _tg(2, 2, 3, 1, 2),       # pad = knl - 1, the largest admitted: 4 x 4 outputs, the corner windows hold one pixel
    "tg_s2": _tg(3, 4, 5, 2, 2),         # stride 2, clipped at both ends: 2 x 2 outputs
    "tg_fit": _tg(3, 3, 3, 1, 0),        # map = kernel, unpadded: one output
    "tg_gap": _tg(7, 8, 2, 3, 0),        # stride > knl: source rows and columns inside a tile's receptive field that no window holds
    "tg_s4": _tg(4, 9, 3, 4, 1),         # stride > knl with padding: 1 x 3 outputs
    "tg_1x2": _tg(1, 2, 3, 1, 1),        # 8 stages per tile: the split eight-wave form cuts it into slices of one and two stages
}
TINY_SHAPES = dict(TINY_BASE)
# every row with 512 channels: two eight-wave chunks of 1x3 tiles, 1x1 tiles of the 16-wave kernel, half panels of 64 channels per wave
TINY_SHAPES.update({n + "_c512": (k, dict(g, Ct=512), M, K, Cs, mr) for n, (k, g, M, K, Cs, mr) in TINY_BASE.items()})
TINY_SHAPES.update({
    "tg_1x1_c192": _tg(1, 1, 3, 1, 1, Ct=192),                        # 24 / 48 channels per wave, 2x2 / 2x4 tiles on one pixel
    "tg_1x1_c384": _tg(1, 1, 3, 1, 1, Ct=384),                        # 48 channels per wave, 1x2 / 2x2 tiles
    "tg_k5_g2": _tg(2, 3, 5, 1, 2, Cin=40, Ct=256, grp=2, M=3),       # 8 + 8 + 4 dims per group: the ragged sub-space's over-read on a two-row map
    "tg_pad2_m7": _tg(2, 2, 3, 1, 2, Cin=28, M=7, K=32, Cs=4),        # stages of G = 4 sub-spaces, the last of every pixel holds 3
    # one 3-dim sub-space: the decoded panel form (clamped instantiations) and the few-image kernel, as the dp_* shapes
    "tg_1x1_d": _tg(1, 1, 3, 1, 1, Cin=3, Ct=64, M=1, Cs=4),
    "tg_k5_d": _tg(2, 3, 5, 1, 2, Cin=3, Ct=96, M=1, Cs=4),
    "tg_pad2_d": _tg(2, 2, 3, 1, 2, Cin=3, Ct=64, M=1, Cs=8),
})
TINY_DEC = sorted(n for n in TINY_SHAPES if n.endswith("_d"))
TINY_TABLE = sorted(n for n in TINY_SHAPES if not n.endswith("_d"))
# the same geometries for the precise path (k_dense) — and the one at which its upper tap bound used to leave the map:
# H = 1, 3x3 / 2, pad 1: (pad - kh + H - 1) / stride = -1 / 2 truncates to 0 for kh = 2 (qcnn_dense.hip)
TINY_DENSE = dict({n: TINY_BASE[n][1] for n in TINY_BASE}, tg_1x1_s2=conv_geom(1, 1, 32, 3, 2, 1, 1, 128))

# What the planner and the launchers choose for each tg_* shape, in the layout of PANEL_REACH (stage, live families with channels
# per wave, tile / strip, chunks, tiles per axis / strips, stages of the heaviest tile; split forms (Z, first split rank) at ONE
# panel; dead = not eligible, cost 0) plus small = the few-image launcher's (TH, TW, MC, CH, channel chunks per group, G) as
# SMALL_REACH and, for the tg_*_d shapes, dec = the decoded panel form's (S, NS, T, instantiation at > 16 images, at <= 16, channel
# chunks) as DEC_REACH.  A sliding form needs Ho >= 2 x slots output rows: of these maps only tg_col's 7 rows have them, everything
# else falls back to the tile form of its family.  A split form is listed where the planner cuts at one panel (Z > 1).
TINY_REACH = {
    "tg_1x1": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (1, 1), 4), "sym16": (8, 2, 2, 1, (1, 1), 4), "sym8": (16, 2, 3, 1, (1, 1), 4),
              "half8": (32, 3, 4, 2, 1, (1, 1), 4)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(1, 1, 4, 128, 1, 1)),
    "tg_row": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (1, 2), 16), "sym16": (8, 2, 2, 1, (1, 2), 12), "sym8": (16, 2, 3, 1, (1, 2), 16),
              "half8": (32, 3, 4, 2, 1, (1, 1), 16), "split_sym8": (5, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(1, 2, 4, 128, 1, 1)),
    "tg_col": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (7, 1), 12), "slide16": (12, 3, 1, 1, 1, 28), "sym16": (8, 2, 2, 1, (4, 1), 16),
              "sym8": (16, 2, 3, 1, (4, 1), 16), "sym8_slide": (16, 3, 2, 1, 1, 28), "half8": (32, 3, 4, 2, 1, (3, 1), 20),
              "half8_slide": (32, 3, 4, 2, 1, 1, 28), "split_sym8": (4, 0)},
        dead=(), small=(2, 1, 4, 128, 1, 1)),
    "tg_k5": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (2, 1), 24), "sym16": (8, 2, 2, 1, (1, 2), 24), "sym8": (16, 2, 3, 1, (1, 1), 24),
              "half8": (32, 3, 4, 2, 1, (1, 1), 24), "split_tile": (4, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 1, 1)),
    "tg_pad2": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (4, 2), 16), "sym16": (8, 2, 2, 1, (2, 2), 16), "sym8": (16, 2, 3, 1, (2, 2), 16),
              "half8": (32, 3, 4, 2, 1, (2, 1), 16), "split_sym8": (6, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 1, 1)),
    "tg_s2": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (2, 1), 48), "sym16": (8, 2, 2, 1, (1, 1), 48), "sym8": (16, 2, 3, 1, (1, 1), 48),
              "half8": (32, 3, 4, 2, 1, (1, 1), 48), "split_tile": (8, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 1, 1)),
    "tg_fit": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (1, 1), 36), "sym16": (8, 2, 2, 1, (1, 1), 36), "sym8": (16, 2, 3, 1, (1, 1), 36),
              "half8": (32, 3, 4, 2, 1, (1, 1), 36), "split_tile": (6, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(1, 1, 4, 128, 1, 1)),
    "tg_gap": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (2, 1), 64), "sym16": (8, 2, 2, 1, (1, 2), 100), "sym8": (16, 2, 3, 1, (1, 1), 160),
              "half8": (32, 3, 4, 2, 1, (1, 1), 160), "split_tile": (8, 0), "split_sym8": (2, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 1, 1)),
    "tg_s4": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (1, 1), 72), "sym16": (8, 2, 2, 1, (1, 2), 48), "sym8": (16, 2, 3, 1, (1, 1), 72),
              "half8": (32, 3, 4, 2, 1, (1, 1), 72), "split_tile": (8, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(1, 2, 4, 128, 1, 1)),
    "tg_1x2": dict(
        stage=(1, 1, 4),
        live={"tile": (12, 1, 3, 1, (1, 1), 8), "sym16": (8, 2, 2, 1, (1, 1), 8), "sym8": (16, 2, 3, 1, (1, 1), 8),
              "half8": (32, 3, 4, 2, 1, (1, 1), 8), "split_sym8": (6, 0)},
        dead=("slide16", "sym8_slide", "half8_slide"), small=(1, 2, 4, 128, 1, 1)),
    "tg_1x1_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (1, 1), 4), "sym8": (32, 1, 3, 2, (1, 1), 4), "half8": (64, 1, 3, 1, 1, (1, 1), 4)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 1, 4, 128, 4, 1)),
    "tg_row_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (1, 4), 12), "sym8": (32, 1, 3, 2, (1, 2), 16), "half8": (64, 1, 3, 1, 1, (1, 2), 16),
              "split_sym8": (6, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 2, 4, 128, 4, 1)),
    "tg_col_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (7, 1), 12), "slide16": (12, 3, 1, 4, 1, 28), "sym8": (32, 1, 3, 2, (7, 1), 12),
              "sym8_slide": (32, 3, 1, 2, 1, 28), "half8": (64, 1, 3, 1, 1, (7, 1), 12), "half8_slide": (64, 3, 1, 1, 1, 1, 28)},
        dead=("sym16",), small=(2, 1, 4, 128, 4, 1)),
    "tg_k5_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (2, 3), 24), "sym8": (32, 1, 3, 2, (2, 1), 24), "half8": (64, 1, 3, 1, 1, (2, 1), 24),
              "split_tile": (4, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 4, 1)),
    "tg_pad2_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (4, 4), 16), "sym8": (32, 1, 3, 2, (4, 2), 16), "half8": (64, 1, 3, 1, 1, (4, 2), 16),
              "split_sym8": (3, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 4, 1)),
    "tg_s2_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (2, 2), 48), "sym8": (32, 1, 3, 2, (2, 1), 48), "half8": (64, 1, 3, 1, 1, (2, 1), 48),
              "split_tile": (6, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 4, 1)),
    "tg_fit_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (1, 1), 36), "sym8": (32, 1, 3, 2, (1, 1), 36), "half8": (64, 1, 3, 1, 1, (1, 1), 36),
              "split_tile": (6, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 1, 4, 128, 4, 1)),
    "tg_gap_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (2, 3), 16), "sym8": (32, 1, 3, 2, (2, 1), 64), "half8": (64, 1, 3, 1, 1, (2, 1), 64),
              "split_tile": (2, 0), "split_sym8": (2, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(2, 2, 4, 128, 4, 1)),
    "tg_s4_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (1, 3), 24), "sym8": (32, 1, 3, 2, (1, 1), 72), "half8": (64, 1, 3, 1, 1, (1, 1), 72),
              "split_tile": (2, 0), "split_sym8": (6, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 2, 4, 128, 4, 1)),
    "tg_1x2_c512": dict(
        stage=(1, 1, 4),
        live={"tile": (24, 1, 1, 2, (1, 2), 8), "sym8": (32, 1, 3, 2, (1, 1), 8), "half8": (64, 1, 3, 1, 1, (1, 1), 8),
              "split_sym8": (4, 0)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 2, 4, 128, 4, 1)),
    "tg_1x1_c192": dict(
        stage=(1, 1, 4),
        live={"tile": (16, 1, 2, 1, (1, 1), 4), "sym8": (24, 2, 2, 1, (1, 1), 4), "half8": (48, 2, 4, 2, 1, (1, 1), 4)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 1, 4, 128, 2, 1)),
    "tg_1x1_c384": dict(
        stage=(1, 1, 4),
        live={"tile": (32, 1, 1, 1, (1, 1), 4), "sym8": (48, 1, 2, 1, (1, 1), 4), "half8": (48, 2, 2, 1, 1, (1, 1), 4)},
        dead=("slide16", "sym16", "sym8_slide", "half8_slide"), small=(1, 1, 4, 128, 3, 1)),
    "tg_k5_g2": dict(
        stage=(1, 1, 3),
        live={"tile": (12, 1, 3, 1, (2, 1), 18), "split_tile": (3, 0)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 3, 128, 1, 1)),
    "tg_pad2_m7": dict(
        stage=(4, 3, 2),
        live={"tile": (12, 1, 3, 1, (4, 2), 8)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 7, 128, 1, 4)),
    "tg_1x1_d": dict(
        stage=(1, 1, 1),
        live={"tile": (6, 2, 3, 1, (1, 1), 1)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(1, 1, 1, 64, 1, 1), dec=(80, 3, 9, (4, 1, True, 2, 4), (2, 4, True, 2, 1), 1)),
    "tg_k5_d": dict(
        stage=(1, 1, 1),
        live={"tile": (8, 2, 2, 1, (1, 2), 6)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 1, 96, 1, 1), dec=(112, 4, 20, (2, 1, True, 3, 4), (2, 4, True, 2, 1), 3)),
    "tg_pad2_d": dict(
        stage=(1, 1, 1),
        live={"tile": (6, 2, 3, 1, (2, 2), 4)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 1, 64, 1, 1), dec=(80, 3, 9, (4, 1, True, 2, 4), (2, 4, True, 2, 1), 1)),
}


# ---------------------------------------------------------------- maps beyond 2^31 and 2^32 bytes per panel ----
# The lg_* shapes: the large end of the geometry range (tests/test_large_cases_cpu.py does the offset arithmetic and the teeth,
# tests/test_gpu_large_cases.py runs them at THREE images: a panel row is 128 lanes whatever the batch, so the byte offsets inside
# a panel are the large ones while the host arrays stay near 100 MB).  Kept out of SHAPES, as the tg_* shapes are.
LARGE_SHAPES = {
    # input panel 127 x 128 x 512 rows of 512 bytes = 4 261 412 864 bytes: source offsets all through [2^31, 2^32), none beyond
    "lg_in_lo": ("conv", conv_geom(127, 128, 512, 3, 1, 1, 1, 128), 64, 128, 8, None),
    # 132 x 128 x 512 rows = 4 429 185 024 bytes: source rows 128 .. 131 start beyond 2^32
    "lg_in_hi": ("conv", conv_geom(132, 128, 512, 3, 1, 1, 1, 128), 64, 128, 8, None),
    # ... in two groups of 256 channels: the second group's channel offset on top of a pixel offset beyond 2^32
    "lg_in_hi_g2": ("conv", conv_geom(132, 128, 512, 3, 1, 1, 2, 128), 32, 128, 8, None),
    # a small input, an output panel of 66 x 64 x 2048 rows = 4 429 185 024 bytes: conv stores, k_conv_sum, ReLU and unpack beyond 2^32
    "lg_out": ("conv", conv_geom(66, 64, 32, 3, 1, 1, 1, 2048), 4, 128, 8, None),
    # either side of the decoded panel form's 2^31-byte guard: 1182^2 x 3 rows = 2 145 982 464 bytes, 1183^2 x 3 = 2 149 615 104
    "lg_dec_lo": ("conv", conv_geom(1182, 1182, 3, 7, 8, 0, 1, 64), 1, 128, 4, None),
    "lg_dec_hi": ("conv", conv_geom(1183, 1183, 3, 7, 8, 0, 1, 64), 1, 128, 4, None),
}
LARGE_BATCH = 3
LARGE_GLUE_MAP = (132, 128, 512)       # H, W, C of the map the glue kernels (LRN, pool, fused LRN + pool) run on: 4 429 185 024 bytes
# the shapes whose source-pixel byte offsets pass 2^32: the conv table kernels form them in 32 bits (pixel_off, qcnn_dev.h) and read
# the top rows instead — held on the CPU tier only (offsets, reach, teeth); the GPU tier runs them through the kernels that do not
# form that offset (few-image, dense)
LARGE_WRAPPING = ("lg_in_hi", "lg_in_hi_g2")


def panel_bytes(H, W, C):
    """Bytes of one panel of an H x W x C map: a row of the 128 images of one (pixel, channel) is 512 bytes."""
    return H * W * C * 512


# What the planner and the launchers choose for each lg_* shape, in the layout of TINY_REACH (split forms at ONE panel — the three
# images of the GPU tier — listed only where the planner cuts there).  Over lg_in_hi and lg_in_hi_g2 every family that forms a
# source pixel's byte offset (pixel_off, qcnn_dev.h) is live: tile, slide16, sym16, sym8, sym8_slide, half8, half8_slide and the
# exact builder (the tile kernel under QCNN_LUT_EXACT).
LARGE_REACH = {
    # 64 stages per pixel; every family.  The planner cuts nothing at one panel: 5000 tiles and more fill the chip whole
    "lg_in_lo": dict(
        stage=(1, 1, 64),
        live={"tile": (12, 1, 3, 1, (127, 43), 960), "slide16": (12, 3, 1, 1, 128, 24384), "sym16": (8, 2, 2, 1, (64, 64), 1024),
              "sym8": (16, 2, 3, 1, (64, 43), 1280), "sym8_slide": (16, 3, 2, 1, 64, 32512), "half8": (32, 3, 4, 2, 1, (43, 32), 1920),
              "half8_slide": (32, 3, 4, 2, 1, 32, 48768)},
        dead=(), small=(2, 2, 16, 128, 1, 1)),
    "lg_in_hi": dict(
        stage=(1, 1, 64),
        live={"tile": (12, 1, 3, 1, (132, 43), 960), "slide16": (12, 3, 1, 1, 128, 25344), "sym16": (8, 2, 2, 1, (66, 64), 1024),
              "sym8": (16, 2, 3, 1, (66, 43), 1280), "sym8_slide": (16, 3, 2, 1, 64, 33792), "half8": (32, 3, 4, 2, 1, (44, 32), 1920),
              "half8_slide": (32, 3, 4, 2, 1, 32, 50688)},
        dead=(), small=(2, 2, 16, 128, 1, 1)),
    # 64 channels per group: the 16-wave tile and sliding kernels only (the eight-wave forms start at 65 channels per chunk)
    "lg_in_hi_g2": dict(
        stage=(1, 1, 32),
        live={"tile": (6, 2, 3, 1, (66, 43), 640), "slide16": (6, 3, 2, 1, 64, 16896)},
        dead=("sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 17, 64, 1, 1)),
    # 2048 channels: 342 per chunk of the eight-wave tile form, which has no 48-channel split of 2048 — its sliding form does
    "lg_out": dict(
        stage=(1, 1, 4),
        live={"tile": (32, 1, 1, 6, (66, 64), 36), "slide16": (12, 3, 1, 15, 64, 792), "sym8_slide": (32, 3, 1, 8, 64, 792),
              "half8": (64, 1, 3, 1, 4, (66, 22), 60), "half8_slide": (64, 3, 1, 1, 4, 64, 792)},
        dead=("sym16", "sym8"), small=(2, 2, 4, 128, 16, 1)),
    "lg_dec_lo": dict(
        stage=(1, 1, 1), live={"tile": (6, 2, 3, 1, (74, 49), 345)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 1, 64, 1, 1),
        dec=(80, 6, 42, (4, 1, False, 3, 4), (4, 4, False, 3, 1), 1)),
    "lg_dec_hi": dict(
        stage=(1, 1, 1), live={"tile": (6, 2, 3, 1, (74, 50), 345)},
        dead=("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide"), small=(2, 2, 1, 64, 1, 1),
        dec=(80, 6, 42, (4, 1, False, 3, 4), (4, 4, False, 3, 1), 1)),
}


def dense_expected_by_taps(g, x, params, rows=None):
    """dense_expected for a conv layer with any number of sub-spaces and groups, as knl^2 float64 matrix products per group over the
    decoded weights, summed tap by tap (the multi-sub-space, grouped sibling of dense_expected_one_subspace): for maps too large for
    dense_expected's gathers.  Every product of two float32 values is exact in float64; only the summation order differs from
    dense_expected (tests/test_large_cases_cpu.py holds the two together).  rows = (lo, hi): output rows lo .. hi - 1 only."""
    x = np.asarray(x, np.float32)
    n, H, W, Cin = x.shape
    knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
    ctrd = np.asarray(params["ctrd"], np.float32)
    M, K, Cs = ctrd.shape
    Ho, Wo = out_hw(g)
    lo, hi = (0, Ho) if rows is None else rows
    Cg, Ctg = Cin // grp, Ct // grp
    a = np.asarray(params["asmt"]).reshape(Ct, knl, knl, M).astype(np.int64)
    # decoded weights [Ct, kh, kw, Cg]: sub-space m's code word in dims m Cs .. (zero beyond CsEff, cut at Cg)
    w = ctrd[np.arange(M)[None, None, None, :], a].reshape(Ct, knl, knl, M * Cs)[..., :Cg].astype(np.float64)
    bias = np.asarray(params["bias"], np.float32).astype(np.float64)
    want = np.tile(bias, (n, hi - lo, Wo, 1))
    mag = np.tile(np.abs(bias), (n, hi - lo, Wo, 1))
    r0, r1 = lo * s - pad, (hi - 1) * s - pad + knl                                 # source rows [r0, r1) of the padded frame
    xp = np.zeros((n, r1 - r0, W + 2 * pad, Cin))
    a0, a1 = max(r0, 0), min(r1, H)
    xp[:, a0 - r0:a1 - r0, pad:pad + W] = x[:, a0:a1]
    for gi in range(grp):
        cts, cin = slice(gi * Ctg, (gi + 1) * Ctg), slice(gi * Cg, (gi + 1) * Cg)
        for kh in range(knl):
            for kw in range(knl):
                sl = xp[:, kh:kh + (hi - lo - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s, cin]
                wt = w[cts, kh, kw].T
                want[..., cts] += sl @ wt
                mag[..., cts] += np.abs(sl) @ np.abs(wt)
    return want, mag


def dec_dense_rel(kind, g, split_bf16=False):
    """Relative bound of one output of a decoded layer with ordinary parameters, per unit of mag = |bias| + sum |x_j c_j|, valid for
    ANY summation order.  f32 (conv, both forms; FC with any slice count): the output is bias plus n = Cin knl^2 (FC: D) products
    accumulated by fused multiply-adds — one rounding each, and partial chains joined by rounded additions never put more than n
    roundings behind one term: gamma(n + 1).  Split-bf16: every product is six exact bf16 x bf16 terms that miss it by at most
    2^-22 |x c| (test_bf16split_cpu.py), each added with one rounding: 2^-22 + gamma(6 n + 1)."""
    n = g["Cin"] * g["knl"] ** 2 if kind == "conv" else g["D"]
    return SPLIT_BF16_PRODUCT + gamma(6 * n + 1) if split_bf16 else gamma(n + 1)


def dense_check_rel(y, want64, mag, rel, what=""):
    """Assert |y - want64| <= rel * mag for every element; returns the worst err / bound."""
    y = np.asarray(y)
    assert y.shape == want64.shape == mag.shape, (y.shape, want64.shape, mag.shape)
    assert np.isfinite(y).all(), "%s: non-finite output" % what
    assert (mag > 0).all()
    err = np.abs(y.astype(np.float64) - want64)
    ratio = err / (rel * mag)
    if (ratio > 1.0).any():
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError("%s: %d of %d outputs beyond the bound; worst at %r: got %.9g want %.17g err %.3g bound %.3g"
                             % (what, int((ratio > 1.0).sum()), ratio.size, i, float(y[i]), float(want64[i]), float(err[i]),
                                float(rel * mag[i])))
    return float(ratio.max())


def dense_expected_one_subspace(g, x, params):
    """dense_expected for a conv layer with ONE sub-space and one group, as knl^2 float64 matrix products over the decoded weights
    (the same products, summed tap by tap): for maps too large for dense_expected's gathers.  tests/test_decoded_cases_cpu.py holds
    it to dense_expected."""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, H, W, Cin = x.shape
    knl, s, pad, Ct = g["knl"], g["stride"], g["pad"], g["Ct"]
    assert g["grp"] == 1 and params["ctrd"].shape[0] == 1
    Ho, Wo = out_hw(g)
    a = np.asarray(params["asmt"]).reshape(Ct, knl, knl).astype(np.int64)
    w = np.asarray(params["ctrd"], np.float32)[0][a][..., :Cin].astype(np.float64)      # [Ct, kh, kw, Cin]
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin))
    xp[:, pad:pad + H, pad:pad + W] = x
    bias = np.asarray(params["bias"], np.float32).astype(np.float64)
    want = np.tile(bias, (n, Ho, Wo, 1))
    mag = np.tile(np.abs(bias), (n, Ho, Wo, 1))
    for kh in range(knl):
        for kw in range(knl):
            sl = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
            want += sl @ w[:, kh, kw].T
            mag += np.abs(sl) @ np.abs(w[:, kh, kw]).T
    return want, mag


def window_hit(g, poison):
    """poison [n, H, W, Cin] bool -> [n, Ho, Wo] bool: the outputs whose window holds a poisoned input element."""
    n, H, W, _ = poison.shape
    knl, s, pad = g["knl"], g["stride"], g["pad"]
    Ho, Wo = out_hw(g)
    pp = np.zeros((n, H + 2 * pad, W + 2 * pad), bool)
    pp[:, pad:pad + H, pad:pad + W] = poison.any(-1)
    hit = np.zeros((n, Ho, Wo), bool)
    for kh in range(knl):
        for kw in range(knl):
            hit |= pp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
    return hit


def shape_rounds(name, negate=False):
    kind, g, M, K, Cs, mr = SHAPES[name]
    return schedule(kind, g, M, K, Cs, max_rounds=mr, negate=negate)
