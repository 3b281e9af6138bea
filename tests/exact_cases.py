"""TEST HELPER — exact-sum cases: crafted integer data on which every conv / FC table kernel must return ONE number, bit for bit.

Activations are +-2^e_x, code words integers in [-amp, amp] times 2^e_c, the bias a non-zero integer times the unit
u = 2^(e_x + e_c).  Then every product, every table entry T = <x_m, c> and every partial sum of an output

    out = bias + sum over the taps inside the map, over m, of T[pixel][m][asmt]

is an integer multiple of u, and as long as |bias| + sum |T| stays <= 2^24 u (fp32 sums) or <= 2048 u (fp16 entries: |T| <= 2048 u;
packed fp16 sums: the whole of it), every one of them is exactly representable in the precision the kernel keeps it in — f32
MFMA chains, entries rounded to fp16, v_pk_add_f16 sums, f32 sums, the f32 reduction of slices.  Rounding an exact value is a no-op, so
ANY summation order, tiling, stage grouping or slice count gives the same bits and the expected output is an integer sum; one
lost or doubled look-up, a wrong slot, image half or stage buffer, a bias added twice or never shows as a whole unit.  (Whether a
mode rounds at all this data cannot show: that stays with the one-hot probes and the AlexNet fp16 tests.)

A zero entry hides its own loss.  Every code word here has an ODD coordinate sum over its live dims, and x is +-1 per dim, so
T = sum +-c_j has the parity of sum c_j: no entry inside the map is ever 0 (the condition asked for is at most a quarter).

Plain numpy; no GPU, no oracle.  Layouts as table_probe.probe_params / synth.make_params: ctrd [M][K][Cs] (dims >= CsEff zero), asmt
0-based uint8 [Ct][kh][kw][M] (conv) / [Ct][M] (FC).  tests/test_exact_cases_cpu.py asserts the conditions on every case and ties
exact_expected to the oracle; tests/test_gpu_exact_sums.py sends the cases through the kernels."""
from __future__ import annotations

import numpy as np

import table_probe as tp

F16_UNITS = 2048           # integers up to 2^11 are exact in fp16 (11 significand bits); above, the step exceeds 1
F32_UNITS = 2 ** 24        # ... up to 2^24 in fp32
F16_MIN_NORMAL_EXP, F16_MAX = -14, 65504.0


def exact_params(kind, g, M, K, Cs, seed, amp, e_c, e_x=0):
    """dict(bias, ctrd, asmt, bits, e_c, e_x): code words uniform integers in [-amp, amp] times 2^e_c, then one live coordinate of
    every word with an even coordinate sum moved by one (inside the range) so that the sum is odd; dims >= CsEff zero; assignments
    uniform over K; bias a non-zero integer in [-8, 8] times 2^(e_x + e_c)."""
    Ct, knl, _ = tp._dims(kind, g)
    cse = tp.cs_eff(kind, g, M, Cs)
    rng = np.random.default_rng([seed, 41])
    c = rng.integers(-amp, amp + 1, size=(M, K, Cs)).astype(np.int64)
    for m in range(M):
        c[m, :, cse[m]:] = 0
        even = np.flatnonzero(c[m].sum(-1) % 2 == 0)
        j = rng.integers(0, cse[m], size=even.size)
        c[m, even, j] += np.where(c[m, even, j] >= amp, -1, 1)
    assert np.abs(c).max() <= amp and (c.sum(-1) % 2 == 1).all()
    shape = (Ct, knl, knl, M) if kind == "conv" else (Ct, M)
    asmt = rng.integers(0, K, size=shape).astype(np.uint8)
    b = rng.integers(1, 9, size=Ct) * rng.choice([-1, 1], size=Ct)
    return dict(bias=(b * 2.0 ** (e_x + e_c)).astype(np.float32), ctrd=(c * 2.0 ** e_c).astype(np.float32), asmt=asmt,
                bits=max(1, int(K - 1).bit_length()), e_c=e_c, e_x=e_x)


def exact_activations(kind, g, n, seed, e_x):
    """NHWC [n, H, W, Cin] (conv) / [n, D] (FC) float32, every value -2^e_x or +2^e_x."""
    rng = np.random.default_rng([seed, 43])
    shape = (n, g["H"], g["W"], g["Cin"]) if kind == "conv" else (n, g["D"])
    return np.ascontiguousarray(rng.choice([-1.0, 1.0], size=shape) * 2.0 ** e_x, np.float32)


def unit_exp(x, params):
    """e_x + e_c, with x and the parameters checked to be what the generators make."""
    e_x, e_c = params["e_x"], params["e_c"]
    assert (np.abs(np.asarray(x, np.float64)) == 2.0 ** e_x).all()
    ci = np.asarray(params["ctrd"], np.float64) / 2.0 ** e_c
    bi = np.asarray(params["bias"], np.float64) / 2.0 ** (e_x + e_c)
    assert (ci == np.rint(ci)).all() and (bi == np.rint(bi)).all() and (bi != 0).all()
    return e_x + e_c


def exact_stats(kind, g, x, params, full=True):
    """dict(want, s_abs, terms, zeros, t_max), all in units of 2^(e_x + e_c), the first four int64 shaped like the layer's output
    [n, Ho, Wo, Ct] (FC: [n, Ct]): the sum, |bias| + sum |T|, the entries an element names inside the map and how many of them are 0
    (both only with `full`); t_max: the largest |T| of any table.  Padding taps contribute 0 and name nothing; groups as in
    table_probe.dense_expected.  Integer arithmetic carried in float32 matrix products and sums (asserted to stay below 2^24,
    where float32 holds every integer)."""
    e = unit_exp(x, params)
    xi = (np.asarray(x, np.float64) / 2.0 ** params["e_x"]).astype(np.float32)
    ci = (np.asarray(params["ctrd"], np.float64) / 2.0 ** params["e_c"]).astype(np.float32)
    bi = (np.asarray(params["bias"], np.float64) / 2.0 ** e).astype(np.float32)
    asmt = np.asarray(params["asmt"]).astype(np.int64)
    M, K, Cs = ci.shape
    cse = tp.cs_eff(kind, g, M, Cs)
    Ct = bi.shape[0]
    t_max = 0.0
    if kind == "fc":
        shape, boxes = (xi.shape[0], Ct), None
    else:
        n, H, W, Cin = xi.shape
        knl, s, pad, grp = g["knl"], g["stride"], g["pad"], g["grp"]
        Ho, Wo = tp.out_hw(g)
        Cg, Ctg = Cin // grp, Ct // grp
        shape = (n, Ho, Wo, Ct)
        asmt = asmt.reshape(Ct, knl, knl, M)

        def axis(k, size, n_out):                         # outputs o0 .. o1 whose tap k lies inside the map, and the source slice
            o = [i for i in range(n_out) if 0 <= i * s - pad + k < size]
            return (o[0], o[-1] + 1, slice(o[0] * s - pad + k, o[-1] * s - pad + k + 1, s)) if o else None
        boxes = [(kh, kw, axis(kh, H, Ho), axis(kw, W, Wo)) for kh in range(knl) for kw in range(knl)]
        boxes = [b for b in boxes if b[2] and b[3]]
    want, sabs = np.broadcast_to(bi, shape).copy(), np.broadcast_to(np.abs(bi), shape).copy()
    zeros, terms = np.zeros(shape, np.float32), np.zeros(shape, np.float32)

    def add(box, Tm):
        want[box] += Tm
        sabs[box] += np.abs(Tm)
        if full:
            zeros[box] += Tm == 0
            terms[box] += 1
    if kind == "fc":
        asmt = asmt.reshape(Ct, M)
        for m in range(M):
            T = xi[:, m * Cs:m * Cs + cse[m]] @ ci[m, :, :cse[m]].T              # [n, K]
            t_max = max(t_max, float(np.abs(T).max()))
            add((slice(None), slice(None)), T[:, asmt[:, m]])
    else:
        for gi in range(grp):
            cts = slice(gi * Ctg, (gi + 1) * Ctg)
            for m in range(M):
                c0 = gi * Cg + m * Cs
                T = xi[..., c0:c0 + cse[m]] @ ci[m, :, :cse[m]].T                # [n, H, W, K]: the pixel tables of sub-space m
                t_max = max(t_max, float(np.abs(T).max()))
                for kh, kw, (h0, h1, hs), (w0, w1, ws) in boxes:
                    add((slice(None), slice(h0, h1), slice(w0, w1), cts), T[:, hs, ws][..., asmt[cts, kh, kw, m]])
    assert sabs.max() < F32_UNITS and (want == np.rint(want)).all()
    i64 = lambda a: np.rint(a).astype(np.int64)
    return dict(want=i64(want), s_abs=i64(sabs), terms=i64(terms), zeros=i64(zeros), t_max=int(t_max))


def exact_expected(kind, g, x, params):
    """(want, S_abs): the int64 sum in units of 2^(e_x + e_c) and |bias| + sum |T| per output element."""
    st = exact_stats(kind, g, x, params, full=False)
    return st["want"], st["s_abs"]


def as_float32(want, e):
    """The integer sum as the float32 a kernel must return (exact: |want| <= 2^24, 2^e a power of two)."""
    assert np.abs(want).max() <= F32_UNITS
    return (want.astype(np.float64) * 2.0 ** e).astype(np.float32)


def check_conditions(st, e, f16_sums):
    """The conditions under which every intermediate is exact; asserted, not measured.  f16_sums: the case also runs with packed fp16
    running sums."""
    assert st["t_max"] <= F16_UNITS, st["t_max"]
    assert st["s_abs"].max() <= (F16_UNITS if f16_sums else F32_UNITS), int(st["s_abs"].max())
    assert e >= F16_MIN_NORMAL_EXP and F16_UNITS * 2.0 ** e <= F16_MAX          # 1 .. 2048 units lie in the fp16 normal range
    assert (4 * st["zeros"] <= st["terms"]).all(), float((st["zeros"] / np.maximum(st["terms"], 1)).max())
    assert (st["terms"] > 0).all()


# ---------------------------------------------------------------- the cases ----
# conv: geometries of table_probe.SHAPES; name -> (amp, e_x, e_c).  amp per shape so that |bias| + sum |T| <= 2048 units on every
# element (E|T| is about 2.5 for amp = 2, Cs = 4 and 3.2 for Cs = 8; 1.8 for amp = 1, Cs = 8): checked on the CPU tier
CONV = {
    "pn_deep": (2, -3, -5),          # 288 terms of 4 dims; unit 2^-8
    "pn_c192": (2, 0, 0),            # 72 terms of 8 dims; unit 1
    "pn_c256_cs4": (2, 1, 2),        # 144 of 4; unit 8
    "pn_c384": (2, -8, 0),           # 72 of 8; 2^-8
    "pn_c512": (2, 2, 1),            # 144 of 8; 8
    "pn_grp2_5x5": (2, 0, -2),       # 200 of 8; 1/4
    "pn_s2_5x5": (1, -1, 1),         # 400 of 8: amp = 1; unit 1
    "pn_k32_m18": (2, 3, 0),         # 162 of 4 (last sub-space 2 dims); 8
    "pn_partial": (2, -4, -4),       # 81 of 8 (last sub-space 4 dims); 2^-8
}

# FC: name -> (geometry, M, K, Cs, amp, e_x, e_c).  fx_*: k_fc_sym8's shape (K = 32, Cs = 4, M % 4 == 0, D = 4 M, Ct >= 192 and even),
# modes 0, 1 and 2, so S_abs <= 2048 units; fa_*: the 12-wave kernel k_fc_aprx (f32 sums)
FC = {
    "fx_s1": (tp.fc_geom(16, 192), 4, 32, 4, 2, 0, 0),               # one slice of ONE stage; two live waves
    "fx_s2": (tp.fc_geom(32, 242), 8, 32, 4, 2, -3, -5),             # ... of two; the third wave: 48 + 2 channels
    "fx_s5": (tp.fc_geom(80, 192), 20, 32, 4, 2, 1, 2),              # ... of five
    "fx_slices": (tp.fc_geom(1600, 962), 400, 32, 4, 2, -2, -6),     # 100 stages; 768 + 194 channels: a second chunk
    "fa_k128": (tp.fc_geom(680, 2), 170, 128, 4, 2, 0, 0),           # G = 1; Ct < 96: one half-wave with channels
    "fa_k64": (tp.fc_geom(476, 100), 119, 64, 4, 2, -4, -4),         # G = 2, M % G = 1; 96 <= Ct < 384: 96 + 4 channels
    "fa_k32": (tp.fc_geom(812, 400), 203, 32, 4, 2, 1, 2),           # G = 4, M % G = 3; Ct >= 384: 384 + 16
    "fa_k16": (tp.fc_geom(820, 40), 205, 16, 4, 2, -8, 0),           # G = 8, M % G = 5; 40 of 48 channel slots
    "fa_k10": (tp.fc_geom(1240, 200), 310, 10, 4, 2, 3, -3),         # G = 12, M % G = 10: the exact builder's kernel in every mode
}
FX = sorted(n for n in FC if n.startswith("fx_"))
FA = sorted(n for n in FC if n.startswith("fa_"))
BATCH, SPLIT_BATCH = 131, 125        # a full panel and a ragged one of three images; one panel (QCNN_OPT_SPLIT re-picks per launch)

# What the launchers must choose for each case for it to reach the seam it is there for; tests/test_exact_cases_cpu.py re-derives
# every entry from the planner restatements of test_panel_cases_cpu.py and from qcnn_plan_fc_query.
#   conv: mode1 / mode2 = (channels per wave, th, tw, channel chunks per group) of k_conv_sym8<.., MODE = 1 / 2>, clip1 / clip2 =
#         (last tile row clipped, last tile column clipped); None: no eight-wave form — k_conv_aprx with lutF16
#   FC:   plain = (family, slices, stages per slice, stages of the last slice) at 131 images, QCNN_OPT_SPLIT = 0 (the choice does not
#         depend on the batch); split = the same at one panel of 125 images under QCNN_OPT_SPLIT = 1; G = sub-spaces per stage
EXACT_REACH = {
    "pn_deep": dict(mode1=(16, 2, 3, 1), mode2=(16, 3, 4, 1), clip1=(True, True), clip2=(True, True)),
    "pn_c192": dict(mode1=(24, 2, 2, 1), mode2=(24, 2, 4, 1), clip1=(True, True), clip2=(True, True)),
    "pn_c256_cs4": dict(mode1=(32, 1, 3, 1), mode2=(32, 2, 3, 1), clip1=(False, True), clip2=(True, True)),
    "pn_c384": dict(mode1=(48, 1, 2, 1), mode2=(48, 2, 2, 1), clip1=(False, True), clip2=(True, True)),
    "pn_c512": dict(mode1=(32, 1, 3, 2), mode2=(32, 2, 3, 2), clip1=(False, True), clip2=(True, True)),
    "pn_grp2_5x5": dict(mode1=(16, 2, 3, 1), mode2=(16, 3, 4, 1), clip1=(True, True), clip2=(True, True)),
    "pn_s2_5x5": dict(mode1=(16, 2, 3, 1), mode2=(16, 3, 4, 1), clip1=(True, True), clip2=(True, True)),
    "pn_k32_m18": None,
    "pn_partial": None,
    # k_fc_sym8 (QCNN_OPT_SYM8 = 2; codes -5 / -7 / -8 by mode): stages of four sub-spaces
    "fx_s1": dict(G=4, plain=(-5, 1, 1, 1), split=(-5, 1, 1, 1)),
    "fx_s2": dict(G=4, plain=(-5, 1, 2, 2), split=(-5, 1, 2, 2)),
    "fx_s5": dict(G=4, plain=(-5, 1, 5, 5), split=(-5, 1, 5, 5)),
    "fx_slices": dict(G=4, plain=(-5, 8, 13, 9), split=(-5, 10, 10, 10)),      # an odd stage count per slice, a shorter last slice
    # k_fc_aprx (code -1; its slice count is the planner's, not reported by the engine).  fa_k128: a last slice of ONE stage.  (M = 169
    # is NOT a case: the planner asks 14 slices of 13 stages for it, the fourteenth begins at sub-space 169 = M — LABBOOK.md, "Exact sums")
    "fa_k128": dict(G=1, plain=(-1, 14, 13, 1), split=(-1, 17, 10, 10)),
    "fa_k64": dict(G=2, plain=(-1, 5, 12, 12), split=(-1, 7, 9, 6)),            # last slice 23 sub-spaces in 12 stages
    "fa_k32": dict(G=4, plain=(-1, 4, 13, 12), split=(-1, 6, 9, 6)),
    "fa_k16": dict(G=8, plain=(-1, 2, 13, 13), split=(-1, 3, 9, 8)),
    "fa_k10": dict(G=12, plain=(-1, 2, 13, 13), split=(-1, 3, 9, 8)),
}


def shape_of(name):
    """(kind, geometry, M, K, Cs, amp, e_x, e_c) of a case."""
    if name in CONV:
        kind, g, M, K, Cs, _ = tp.SHAPES[name]
        return (kind, g, M, K, Cs) + CONV[name]
    return ("fc",) + FC[name]


def case(name, n=BATCH):
    """(kind, g, M, K, Cs, params, x, unit exponent): the data both tiers use — the CPU tier checks the conditions on exactly the
    batch the GPU tier runs."""
    kind, g, M, K, Cs, amp, e_x, e_c = shape_of(name)
    params = exact_params(kind, g, M, K, Cs, 91, amp, e_c, e_x)
    return kind, g, M, K, Cs, params, exact_activations(kind, g, n, 92, e_x), e_x + e_c
