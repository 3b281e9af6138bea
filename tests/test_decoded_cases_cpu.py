"""CPU tier of the decoded-kernel cases (tests/test_gpu_decoded_cases.py, the dn_* / dp_* / fcd_* shapes of tests/table_probe.py).

  * The launchers' selection rules (quantized-cnn_amd/csrc/qcnn_decoded.hip: qk_conv_dec, qk_conv_dec_shape, qk_conv_dec_nchw_shape,
    nchw_split_runs / nchw_split_kb / nchw_split_lds; qcnn_planner.hip: qk_fc_dec_shape, qk_fc_dec_slices) are restated in plain
    Python and every shape is held to the branch it is there to reach (table_probe.DEC_REACH): a changed rule fails here instead
    of letting a GPU case pass vacuously.  The ten k_conv_dec instantiations are each reached by some (shape, batch) of the GPU
    list, the in-place kernels by all three k orders, and one shape by the f32 in-place kernel alone.
  * The bounds of the GPU test are attainable without the kernels: float32 emulations of the three sums (a k-ordered chain of
    fused multiply-adds; three bf16 pieces and six terms per step of 32 k; sixteen partial chains, a tree and k slices) through
    the restated DECODERS stay inside them on every dense-sum case.
  * A wrong variant is caught: a repeated column not zeroed, k & (G - 1) for k % G, a last run starting at 4 r, an off-by-one
    position group each leave the bound, break window isolation or change probe outputs on at least one shape."""
import ctypes as C

import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_bf16split_cpu import split3
from test_planner_cpu import FC_DEC, fc_oracle

synth = pkg("synth")
build = pkg("build")

LDS = 160 * 1024
PANEL = 128


def geom_of(name):
    kind, g, M, K, Cs, _ = tp.SHAPES[name] if name in tp.SHAPES else tp.DEC_NOT[name]
    return kind, g, M, K, Cs


# ---------------------------------------------------------------- the launchers' rules, restated ----
def seen_M(M, K):
    """Sub-spaces as the kernels see them: more than 128 code words are cut into pseudo sub-spaces (qcnn_model_set_layer_shape)."""
    return M * -(-K // 128)


def conv_dec_shape(g, M):
    """qk_conv_dec_shape: (Kp, S) or None."""
    Cin, Ct, knl = g["Cin"], g["Ct"], g["knl"]
    if g["grp"] != 1 or M != 1 or not 1 <= Cin <= 4 or Ct < 32 or Ct % 32:
        return None
    kp = (knl * Cin + 3) // 4 * 4
    s = Ct
    while s & 63 not in (16, 48):
        s += 16
    if knl * kp * s * 4 > LDS:
        s = Ct
    if knl * kp * s * 4 > LDS:
        return None
    return kp, s


def conv_dec_instance(g, live, panels):
    """qk_conv_dec: the k_conv_dec<CT, PW, PADDED, R, IT> instantiation of a launch."""
    Ct, Kr = g["Ct"], g["knl"] * g["Cin"]
    Ho, Wo = tp.out_hw(g)
    clamped = g["pad"] != 0 or Kr < 4
    if live <= 16:
        if clamped:
            return (2, 4, True, 2, 1)
        return (6, 2, False, 3, 1) if Ct % 96 == 0 else (4, 4, False, 3, 1) if Ct % 64 == 0 else (2, 6, False, 3, 1)
    if clamped:
        return (4, 1, True, 2, 4) if Ct % 64 == 0 else (2, 1, True, 3, 4)
    if Ct % 96 == 0:
        items = panels * Ho * Wo * ((live + 63) // 64) * (Ct // 96)
        return (3, 1, False, 3, 4) if 4096 < items < 8192 else (6, 1, False, 2, 4)
    return (4, 1, False, 3, 4) if Ct % 64 == 0 else (2, 2, False, 3, 4)


def launch_of(n):
    """(panels, live) of a forward of n images (run_layers): one panel holds its images, more panels are launched whole."""
    panels = -(-n // PANEL)
    return panels, (n if panels == 1 else PANEL)


def nchw_shape(g, M):
    """qk_conv_dec_nchw_shape: the padded k of the f32 in-place kernel, or None."""
    Cin, Ct, knl = g["Cin"], g["Ct"], g["knl"]
    if g["grp"] != 1 or M != 1 or not 1 <= Cin <= 4 or g["pad"] != 0 or Ct % 96:
        return None
    kp = (Cin * knl * knl + 15) // 16 * 16
    return None if (kp + 4) * Ct * 4 + (kp // 4 + 4) * 16 > LDS else kp


def split_kb(Cin, knl, nr):                      # nchw_split_kb
    return (Cin * knl * nr + 7) // 8 * 32 if nr else (Cin * knl * knl + 31) // 32 * 32


def split_lds(Kb, Ct, nr):                       # nchw_split_lds
    return Kb * Ct * 4 + (Kb // 4 + 8 if nr else Kb + 32) * 4


def split_runs(Cin, knl, Ct):                    # nchw_split_runs
    if knl < 4:
        return 0
    nr = (knl + 3) // 4
    return nr if split_lds(split_kb(Cin, knl, nr), Ct, nr) <= LDS else 0


def split_shape(g, M):
    """qk_conv_dec_nchw_split_shape: (order, nr, Kb); ("f32", 0, 0) where only the f32 in-place kernel is eligible."""
    if nchw_shape(g, M) is None:
        return None
    nr = split_runs(g["Cin"], g["knl"], g["Ct"])
    kb = split_kb(g["Cin"], g["knl"], nr)
    if split_lds(kb, g["Ct"], nr) > LDS:
        return ("f32", 0, 0)
    return ("runs" if nr else "flat", nr, kb)


def stage_group(K):
    return 128 // K if K <= 64 else 1           # qcnn_stage_group


def fc_dec_shape(D, M, Cs, Ct):
    """qk_fc_dec_shape: S or None."""
    if Cs != 1 or M != D or D % 64 or Ct < 1 or D * PANEL * 4 >= 2 ** 32:
        return None
    S = (Ct + 63) // 64 * 64
    return S if D * S * 4 < 2 ** 32 else None


def fc_dec_slices(D, Ct, panels, live):          # qk_fc_dec_slices
    wgs = ((Ct + 63) // 64) * panels * ((live + 63) // 64)
    z = 1
    while wgs * z < 192 and D % (128 * z) == 0 and D // (128 * z) >= 4 and 2 * z <= 32:
        z *= 2
    return z


# ---------------------------------------------------------------- every listed branch is reached ----
@pytest.mark.parametrize("name", tp.DEC_NCHW_SHAPES)
def test_in_place_shapes_reach_their_order(name):
    kind, g, M, K, Cs = geom_of(name)
    order, nr, kb, kp, chunks, howo = tp.DEC_REACH[name]
    assert conv_dec_shape(g, seen_M(M, K)) is not None             # the engine asks the panel form first
    assert nchw_shape(g, seen_M(M, K)) == kp and kp % 16 == 0 and kp // 4 >= 4
    assert split_shape(g, seen_M(M, K)) == (order, nr, kb)
    assert g["Ct"] // 96 == chunks and tp.out_hw(g) == howo
    assert M == 1 and Cs == 4 and tp.cs_eff(kind, g, M, Cs) == [g["Cin"]]


def test_what_each_in_place_case_is_there_for():
    G = {n: tp.SHAPES[n][1] for n in tp.DEC_NCHW_SHAPES}
    run_start = lambda knl, r: min(4 * r, knl - 4)
    Kr = lambda n: G[n]["Cin"] * G[n]["knl"] ** 2
    assert {tp.DEC_REACH[n][0] for n in tp.DEC_NCHW_SHAPES} == {"runs", "flat", "f32"}
    assert [n for n in tp.DEC_NCHW_SHAPES if tp.DEC_REACH[n][0] == "f32"] == ["dn_f32_only"]
    # dn_k5: second run at column 1 repeats columns 1, 2, 3; 30 runs in 32 slots; the last position group holds two positions
    assert run_start(5, 1) == 1 and 3 * 5 * 2 == 30 and tp.DEC_REACH["dn_k5"][2] // 4 == 32 and tp.out_hw(G["dn_k5"])[1] % 4 == 2
    # dn_k4_s5: one run per row, one step with four of eight run slots, stride > knl, column 14 in no window, Wo < 4
    g = G["dn_k4_s5"]
    cols = {wo * g["stride"] + kw for wo in range(tp.out_hw(g)[1]) for kw in range(g["knl"])}
    assert tp.DEC_REACH["dn_k4_s5"][1:3] == (1, 32) and g["Cin"] * g["knl"] == 4 and 14 not in cols and tp.out_hw(g)[1] == 3
    # dn_k6: overlap of two columns, exactly three steps, Wo % 4 == 1
    assert run_start(6, 1) == 2 and 2 * 6 * 2 * 4 == tp.DEC_REACH["dn_k6"][2] == 96 and tp.out_hw(G["dn_k6"])[1] % 4 == 1
    # dn_k7_ct192: overlap of one column, two chunks, run order fits
    assert run_start(7, 1) == 3 and split_lds(192, 192, 2) <= LDS and tp.out_hw(G["dn_k7_ct192"])[1] % 4 == 0
    assert [run_start(9, r) for r in range(3)] == [0, 4, 5] and tp.out_hw(G["dn_k9"]) == (1, 1)
    # dn_flat_k9: knl >= 4 but the run order does not fit
    assert split_lds(split_kb(4, 9, 3), 96, 3) > LDS >= split_lds(352, 96, 0) and Kr("dn_flat_k9") == 324
    # dn_f32_only: 163 712 of 163 840 bytes for the f32 kernel, neither split order
    g = G["dn_f32_only"]
    assert (208 + 4) * 192 * 4 + (208 // 4 + 4) * 16 == 163712 <= LDS
    assert split_lds(split_kb(4, 7, 2), 192, 2) > LDS and split_lds(split_kb(4, 7, 0), 192, 0) > LDS
    assert Kr("dn_1x1") == 1 and tp.DEC_REACH["dn_1x1"][2:4] == (32, 16)
    assert G["dn_ct288"]["knl"] < 4 and tp.DEC_REACH["dn_ct288"][4] == 3 and tp.out_hw(G["dn_ct288"])[1] == 5


@pytest.mark.parametrize("name", tp.DEC_PANEL_SHAPES)
def test_panel_shapes_reach_their_instantiation(name):
    kind, g, M, K, Cs = geom_of(name)
    S, NS, T, big, small, chunks = tp.DEC_REACH[name]
    kp, s = conv_dec_shape(g, seen_M(M, K))
    assert (s, kp // 4, g["knl"] * kp // 4) == (S, NS, T) and S != g["Ct"] and knl_fits(g, kp, s)
    if name == "dp_half_items":
        assert launch_of(128) == (1, 128) and conv_dec_instance(g, 128, 1) == big
        assert 4096 < 1 * 46 * 46 * 2 * 1 == 4232 < 8192
        assert conv_dec_instance(g, 128, 2) != big                  # (not at two panels: the probes' 131 images would miss it)
    else:
        assert tp.out_hw(g) == (5, 7)
        for n in tp.DEC_BATCHES:
            panels, live = launch_of(n)
            assert conv_dec_instance(g, live, panels) == (small if n <= 16 else big), n
    assert g["Ct"] // (16 * big[0]) == chunks
    assert (g["pad"] != 0 or g["knl"] * g["Cin"] < 4) == big[2] == small[2]


def knl_fits(g, kp, s):
    return g["knl"] * kp * s * 4 <= LDS


def test_every_panel_instantiation_and_ring_tail_is_reached():
    reached = set()
    for name in tp.DEC_PANEL_SHAPES:
        g = tp.SHAPES[name][1]
        for n in ((128,) if name == "dp_half_items" else tp.DEC_BATCHES):
            reached.add(conv_dec_instance(g, *launch_of(n)[::-1]))
    ten = {(2, 4, True, 2, 1), (6, 2, False, 3, 1), (4, 4, False, 3, 1), (2, 6, False, 3, 1), (4, 1, True, 2, 4), (2, 1, True, 3, 4),
           (3, 1, False, 3, 4), (6, 1, False, 2, 4), (4, 1, False, 3, 4), (2, 2, False, 3, 4)}
    assert reached == ten
    tails = {2: set(), 3: set()}
    for name in tp.DEC_PANEL_SHAPES:
        T = tp.DEC_REACH[name][2]
        for inst in tp.DEC_REACH[name][3:5]:
            tails[inst[3]].add(T % inst[3])
    assert tails == {2: {0, 1}, 3: {0, 1, 2}}
    # the dense channel stride stays alex_conv1's case
    assert conv_dec_shape(tp.SHAPES["alex_conv1"][1], 1) == (36, 96)
    # Kr: < 4 padded, < 4 unpadded, a last step that overlaps by one, NS = 1 with Kr >= 4
    Kr = {n: tp.SHAPES[n][1]["knl"] * tp.SHAPES[n][1]["Cin"] for n in tp.DEC_PANEL_SHAPES}
    assert (Kr["dp_pad_c1"], Kr["dp_1x1"], Kr["dp_k7_ct32"], Kr["dp_k2_ct96"], Kr["dp_k4_ct160"]) == (3, 3, 7, 4, 4)


@pytest.fixture(scope="module")
def fc_query():
    lib = C.CDLL(build.build_planner_cpu())
    lib.qcnn_plan_fc_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def query(geom, split):
        ch = (C.c_int * 2)()
        assert lib.qcnn_plan_fc_query((C.c_int * 8)(*geom), (C.c_int * 7)(split, 1, 1, 1, 0, 0, -1), ch) == 0
        return ch[0], ch[1]
    return query


@pytest.mark.parametrize("name", tp.DEC_FC_SHAPES)
def test_fc_shapes_reach_their_steps_and_slices(name, fc_query):
    kind, g, M, K, Cs = geom_of(name)
    D, Ct = g["D"], g["Ct"]
    steps, G, blocks, last, z1 = tp.DEC_REACH[name]
    S = fc_dec_shape(D, seen_M(M, K), Cs, Ct)
    assert S == blocks * 64 and Ct - (blocks - 1) * 64 == last and D // 64 == steps and stage_group(K) == G
    for n in tp.DEC_BATCHES:
        panels, live = launch_of(n)
        z = fc_dec_slices(D, Ct, panels, live)
        geom = (D, Ct, M, K, Cs, 1, panels, live)
        assert fc_query(geom, 1) == (FC_DEC, z) == fc_oracle(geom, 1, 1, 1, 1, 0, 0, 2 ** 40)
        assert fc_query(geom, 0) == (FC_DEC, 1)
        assert D % (64 * z) == 0
        if n <= 128:
            assert z == z1, n
    if z1 > 1:
        assert fc_dec_slices(D, Ct, *launch_of(5)) > 1 and fc_dec_slices(D, Ct, *launch_of(70)) > 1


def test_what_each_fc_case_is_there_for():
    R = tp.DEC_REACH
    assert [R[n][0] for n in ("fcd_d64", "fcd_d128_k10", "fcd_d192_k24", "fcd_d320_k100")] == [1, 2, 3, 5]   # below, at, beyond the ring of three
    assert R["fcd_d128_k10"][1] == 12 and R["fcd_d192_k24"][1] == 5 and R["fcd_d320_k100"][1] == 1 and 100 % 16
    for n in ("fcd_d128_k10", "fcd_d192_k24"):                       # no power of two: k % G differs from k & (G - 1)
        G = R[n][1]
        assert any(k % G != k & (G - 1) for k in range(tp.SHAPES[n][1]["D"]))
    assert R["fcd_d192_k24"][2:4] == (2, 2)                          # a second channel block with TWO live channels (the fewest: Ct is even)
    per_wave = {n: tp.SHAPES[n][1]["D"] // (64 * R[n][4]) for n in ("fcd_d512", "fcd_d640", "fcd_d768", "fcd_d2048")}
    assert per_wave == {"fcd_d512": 4, "fcd_d640": 5, "fcd_d768": 6, "fcd_d2048": 4}
    assert sorted(s % 3 for s in per_wave.values()) == [0, 1, 1, 2] and R["fcd_d2048"][4] == 8


def test_shapes_that_must_not_decode():
    kind, g, M, K, Cs = geom_of("nd_conv_k200")
    assert conv_dec_shape(g, 1) is not None and seen_M(M, K) == 2 and conv_dec_shape(g, seen_M(M, K)) is None
    kind, g, M, K, Cs = geom_of("nd_fc_k130")
    assert fc_dec_shape(g["D"], M, Cs, g["Ct"]) == 64 and seen_M(M, K) == 128 and fc_dec_shape(g["D"], seen_M(M, K), Cs, g["Ct"]) is None


# ---------------------------------------------------------------- the decoders, restated ----
def weights(params, g):
    """w[c][kh][kw][ct] = ctrd[0][asmt[ct][kh][kw][0]][c]: the code word every assignment names."""
    Ct, knl, Cin = g["Ct"], g["knl"], g["Cin"]
    a = np.asarray(params["asmt"]).reshape(Ct, knl, knl).astype(np.int64)
    return np.ascontiguousarray(params["ctrd"][0][a][..., :Cin].transpose(3, 1, 2, 0), np.float32)


def krow(k, Kr, Kp):                             # qk_dec_krow
    last = Kp - 4
    if k < last or Kr < 4:
        return k if k < Kr else -1
    real = Kr - 4 + (k - last)
    return real if real >= last else -1


def order_panel(g):
    """k_decode_weights: the padded k sequence of the panel form, [(c, kh, kw, live)]; a dead k multiplies the operand the kernel
    loads there (inside the window) by a zero code word."""
    Cin, knl = g["Cin"], g["knl"]
    Kr, Kp = knl * Cin, (knl * Cin + 3) // 4 * 4
    out = []
    for kh in range(knl):
        for kp in range(Kp):
            k = krow(kp, Kr, Kp)
            step = kp // 4
            src = (Kr - 4 + kp % 4) if (step == Kp // 4 - 1 and Kr >= 4) else min(kp, Kr - 1)     # load_b: the row it reads
            out.append((src % Cin, kh, src // Cin, k >= 0))
            assert k < 0 or k == src
    return out


def order_flat(g, pad_to):
    """k_decode_weights_nchw (pad_to 16) / k_decode_weights_split with nr = 0 (pad_to 32): k = (c knl + kh) knl + kw; past the
    window the last element again, code word zero."""
    Cin, knl = g["Cin"], g["knl"]
    Kr = Cin * knl * knl
    out = []
    for k in range(-(-Kr // pad_to) * pad_to):
        kk = min(k, Kr - 1)
        out.append((kk // (knl * knl), (kk // knl) % knl, kk % knl, k < Kr))
    return out


def order_runs(g, nr, zero_repeats=True, clamp_last=True):
    """k_decode_weights_split with nr > 0: k = 4 run + e, run r of a row at column min(4 r, knl - 4), the columns a row's last run
    repeats carry a zero code word; run slots past the last repeat it.  (zero_repeats / clamp_last = False: the wrong variants.)"""
    Cin, knl = g["Cin"], g["knl"]
    n_runs = Cin * knl * nr
    out = []
    for k in range(split_kb(Cin, knl, nr)):
        r = min(k >> 2, n_runs - 1)
        ri = r % nr
        c0 = min(4 * ri, knl - 4) if clamp_last else 4 * ri
        kw, kh, c = c0 + (k & 3), (r // nr) % knl, r // (nr * knl)
        live = (k >> 2) < n_runs and (kw >= 4 * ri or not zero_repeats) and kw < knl
        out.append((c, kh, kw, live))
    return out


def fc_weights(params, D, K, wrong_mod=False):
    """k_decode_fc_weights: the slot byte of (k, ch) holds stage row (k % G) K + code word; w[k][ch] = ctrd[k][row - (k % G) K]
    (read flat, as the kernel does: a wrong row reaches into the neighbouring sub-space's words)."""
    G = stage_group(K)
    a = np.asarray(params["asmt"]).astype(np.int64)                     # [Ct][D]
    k = np.arange(D)
    row = (k % G) * K + a
    idx = row - ((k & (G - 1)) if wrong_mod else (k % G)) * K
    flat = np.asarray(params["ctrd"], np.float32).reshape(-1)           # [D][K][1]
    return flat[np.clip(k * K + idx, 0, flat.size - 1)].T.copy()        # [D][Ct]


# ---------------------------------------------------------------- float32 emulations of the three sums ----
def f32(a):
    return a.astype(np.float32).astype(np.float64)


def operand(g, x, c, kh, kw):
    """x [n, H + 2 pad, W + 2 pad, Cin] (zero padded) -> the operand of every output position [n, Ho, Wo, 1]; a column past the
    padded row is the element the flat address reaches (the next row's first columns), as in memory."""
    Ho, Wo = tp.out_hw(g)
    s = g["stride"]
    n, Hp, Wp, Cin = x.shape
    flat = x.reshape(n, Hp * Wp, Cin)
    idx = (np.arange(Ho)[:, None] * s + kh) * Wp + np.arange(Wo)[None, :] * s + kw
    return flat[:, np.minimum(idx, Hp * Wp - 1), c][..., None].astype(np.float64)


def padded(g, x):
    p = g["pad"]
    return np.pad(np.asarray(x, np.float32), ((0, 0), (p, p), (p, p), (0, 0)))


def emulate_chain(g, x, params, order):
    """bias, then one fused multiply-add per k of `order` (exact product and sum in float64, rounded once to float32)."""
    w = weights(params, g).astype(np.float64)
    xp = padded(g, x)
    Ho, Wo = tp.out_hw(g)
    acc = np.tile(params["bias"].astype(np.float64), (x.shape[0], Ho, Wo, 1))
    for c, kh, kw, live in order:
        acc = f32(acc + operand(g, xp, c, kh, kw) * (w[c, kh, kw] if live else 0.0))
    return acc.astype(np.float32)


def emulate_split(g, x, params, order):
    """Three bf16 pieces per operand; per step of 32 k the six terms x3 w1, x2 w2, x1 w3, x2 w1, x1 w2, x1 w1, every product exact
    and added with one float32 rounding."""
    w = weights(params, g)
    wp = [p.astype(np.float64) for p in split3(w)]
    xp = padded(g, x)
    xs = [p.astype(np.float64) for p in split3(xp)]
    Ho, Wo = tp.out_hw(g)
    acc = np.tile(params["bias"].astype(np.float64), (x.shape[0], Ho, Wo, 1))
    for s0 in range(0, len(order), 32):
        for xi, wi in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):
            for c, kh, kw, live in order[s0:s0 + 32]:
                acc = f32(acc + operand(g, xs[xi], c, kh, kw) * (wp[wi][c, kh, kw] if live else 0.0))
    return acc.astype(np.float32)


def emulate_fc(x, w, bias, z):
    """k_fc_dec + k_sum_partials: per slice sixteen waves with a chain each over their D / (16 z) rows, the tree w + (w + 8), + 4,
    + 2, + 1, the bias on slice 0, then the slices in order."""
    D = w.shape[0]
    per = D // (16 * z)
    x64, w64 = np.asarray(x, np.float32).astype(np.float64), w.astype(np.float64)
    total = None
    for zi in range(z):
        part = []
        for wave in range(16):
            acc = np.zeros((x.shape[0], w.shape[1]))
            for k in range((zi * 16 + wave) * per, (zi * 16 + wave + 1) * per):
                acc = f32(acc + x64[:, k:k + 1] * w64[k][None, :])
            part.append(acc)
        for stride in (8, 4, 2, 1):
            part = [f32(part[i] + part[i + stride]) for i in range(stride)]
        sl = f32(part[0] + (bias.astype(np.float64) if zi == 0 else 0.0))
        total = sl if total is None else f32(total + sl)
    return total.astype(np.float32)


def dense_case(name, seed=83, n=2):
    kind, g, M, K, Cs = geom_of(name)
    spec = {0: dict(kind=kind, M=M, K=K, Cs=Cs, Ct=g["Ct"], knl=g["knl"] if kind == "conv" else 1,
                    D=g["Cin"] if kind == "conv" else g["D"])}
    params = synth.make_params(None, None, seed=seed, spec=spec)[0]
    x = tp.activations(kind, g, n, seed=seed + 1, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x, params)
    return kind, g, K, params, x, want64, mag


@pytest.mark.parametrize("name", tp.DEC_NCHW_SHAPES + tp.DEC_PANEL_SHAPES)
def test_conv_emulations_stay_inside_the_bounds(name):
    kind, g, K, params, x, want64, mag = dense_case(name)
    worst = {"panel": tp.dense_check_rel(emulate_chain(g, x, params, order_panel(g)), want64, mag, tp.dec_dense_rel(kind, g), name)}
    if name.startswith("dn_"):
        order, nr, kb = tp.DEC_REACH[name][:3]
        worst["f32 in place"] = tp.dense_check_rel(emulate_chain(g, x, params, order_flat(g, 16)), want64, mag, tp.dec_dense_rel(kind, g), name)
        if order != "f32":
            o = order_runs(g, nr) if nr else order_flat(g, 32)
            assert len(o) == kb
            worst["split " + order] = tp.dense_check_rel(emulate_split(g, x, params, o), want64, mag, tp.dec_dense_rel(kind, g, True), name)
    print("%s: emulation worst err / bound %s" % (name, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values())
    # a misread tap is off by about mag / (Cin knl^2): 50 f32 bounds or more on every shape (25 of the wider split bound)
    taps = g["Cin"] * g["knl"] ** 2
    assert 1.0 / taps / tp.dec_dense_rel(kind, g) >= 50 and 1.0 / taps / tp.dec_dense_rel(kind, g, True) >= 25


@pytest.mark.parametrize("name", tp.DEC_FC_SHAPES)
def test_fc_emulation_stays_inside_the_bound(name):
    kind, g, K, params, x, want64, mag = dense_case(name)
    w = fc_weights(params, g["D"], K)
    worst = {z: tp.dense_check_rel(emulate_fc(x, w, params["bias"], z), want64, mag, tp.dec_dense_rel(kind, g), name)
             for z in sorted({1, tp.DEC_REACH[name][4]})}
    print("%s: emulation worst err / bound %s" % (name, ", ".join("%d slices %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values())


# ---------------------------------------------------------------- the restated decoders on probes; wrong variants are caught ----
@pytest.mark.parametrize("name", ["dn_k5", "dn_k9", "dn_k4_s5", "dp_k7_ct32", "dp_pad_k3"])
def test_restated_decoders_return_the_probe_entries(name):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    rd = tp.shape_rounds(name)[0]
    params = tp.probe_params(kind, g, M, K, Cs, rd, seed=31)
    x = tp.activations(kind, g, 2, seed=32, scaled=False)
    want64, mag, seq = tp.expected(kind, g, x, params)
    orders = [order_panel(g)] + ([order_flat(g, 16), order_runs(g, tp.DEC_REACH[name][1])] if name.startswith("dn_") else [])
    for o in orders:
        tp.check(emulate_chain(g, x, params, o), want64, mag, g["Cin"], what=name)


def test_a_repeated_column_not_zeroed_is_caught():
    for name in ("dn_k5", "dn_k6", "dn_k7_ct192", "dn_k9"):
        kind, g, K, params, x, want64, mag = dense_case(name)
        bad = emulate_split(g, x, params, order_runs(g, tp.DEC_REACH[name][1], zero_repeats=False))
        with pytest.raises(AssertionError, match="beyond the bound"):
            tp.dense_check_rel(bad, want64, mag, tp.dec_dense_rel(kind, g, True), name)
    kind, g, K, params, x, want64, mag = dense_case("dn_k4_s5")      # no overlap: nothing to catch there
    good = order_runs(g, 1)
    assert good == order_runs(g, 1, zero_repeats=False)


def test_k_and_g_minus_1_for_k_mod_g_is_caught():
    caught = []
    for name in tp.DEC_FC_SHAPES:
        kind, g, K, params, x, want64, mag = dense_case(name)
        bad = emulate_fc(x, fc_weights(params, g["D"], K, wrong_mod=True), params["bias"], 1)
        try:
            tp.dense_check_rel(bad, want64, mag, tp.dec_dense_rel(kind, g), name)
        except AssertionError:
            caught.append(name)
    assert caught == ["fcd_d128_k10", "fcd_d192_k24"]                # G = 12 and G = 5; a power of two hides it


def test_a_last_run_starting_at_4r_is_caught_by_window_isolation():
    """Its products are the right ones (the columns past the row carry a zero code word), so no bound sees it: the NaN of a pixel
    right of the window does."""
    kind, g, K, params, x, want64, mag = dense_case("dn_k5")
    good, bad = order_runs(g, 2), order_runs(g, 2, clamp_last=False)
    assert np.array_equal(emulate_chain(g, x, params, good), emulate_chain(g, x, params, bad))
    poison = np.zeros(x.shape, bool)
    poison[0, 4, 6, 1] = True                                        # column 6: right of the windows at columns 0 and 1
    xn = np.where(poison, np.float32(np.nan), x)
    hit = tp.window_hit(g, poison)
    clean = emulate_chain(g, x, params, good)
    y = emulate_chain(g, xn, params, good)
    assert np.isnan(y[hit]).all() and np.array_equal(y[~hit], clean[~hit])
    y = emulate_chain(g, xn, params, bad)
    assert np.isnan(y[~hit]).any()


def test_an_off_by_one_position_group_is_caught():
    """Position groups counted as P // PW: the ragged last group of 35 positions is never written."""
    for name in ("dp_k7_ct32", "dp_k5_ct64", "dp_k2_ct96"):
        kind, g, K, params, x, want64, mag = dense_case(name)
        y = emulate_chain(g, x, params, order_panel(g))
        for inst in tp.DEC_REACH[name][3:5]:
            PW = inst[1]
            if PW == 1:
                continue
            P = y.shape[1] * y.shape[2]
            assert P % PW
            bad = y.reshape(y.shape[0], P, -1).copy()
            bad[:, P // PW * PW:] = 0.0
            with pytest.raises(AssertionError, match="beyond the bound"):
                tp.dense_check_rel(bad.reshape(y.shape), want64, mag, tp.dec_dense_rel(kind, g), name)


def test_window_hit_helper():
    g = tp.SHAPES["dn_k4_s5"][1]
    poison = np.zeros((1, 9, 15, 1), bool)
    poison[0, :, 14] = True                                          # the column no window covers
    assert not tp.window_hit(g, poison).any()
    poison[0, 5, 10] = True
    assert np.argwhere(tp.window_hit(g, poison)).tolist() == [[0, 1, 2]]
    g = tp.SHAPES["dp_pad_k3"][1]
    poison = np.zeros((1, 5, 7, 3), bool)
    poison[0, 0, 0, 2] = True
    assert np.argwhere(tp.window_hit(g, poison)).tolist() == [[0, 0, 0], [0, 0, 1], [0, 1, 0], [0, 1, 1]]


@pytest.mark.parametrize("name", ["dp_pad_k3", "dp_k7_ct32", "dn_k5", "dn_k4_s5"])
def test_the_one_subspace_reference_equals_dense_expected(name):
    kind, g, K, params, x, want64, mag = dense_case(name)
    w2, m2 = tp.dense_expected_one_subspace(g, x, params)
    assert np.abs(w2 - want64).max() <= 1e-13 * mag.max() and np.abs(m2 - mag).max() <= 1e-13 * mag.max()
