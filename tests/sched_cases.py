"""TEST HELPER — the exact network: integer data on which a WHOLE forward has one right answer, bit for bit, in every schedule.

tests/exact_cases.py makes one layer exact: activations, code words and biases integer multiples of a power of two, every partial sum
below 2^24 units, so that every family, tiling, slice count and summation order returns the same bits.  Here the same holds layer
after layer through a small network (NET) in which every layer type that can stay exact appears — a first conv layer that is read
in place from NCHW and decodes, two conv layers with several table families each (one of them grouped), ReLU, two max-pools, an FC
layer behind a map with H, W, C > 1 (the NCHW-flatten map and k_permute_rows), k_fc_sym8's shape, dropout (an alias), a decoded FC
layer, a classifier whose code words and bias carry a negative power of two so that the un-shifted soft-max stays finite — and, for
LRN, which cannot stay integer, through a second, shorter table (LRN_LAYERS).  So whatever run_layers, launch_conv, launch_fc, fc_input
(qcnn_engine_run.hip) and the host schedules (qcnn_engine_host.hip) decide for a batch — streams, chunks, scratch shares, plan
cache, fused ReLU, aliases, in-place input, few-image kernels — the last-FC map must equal the integer result of `reference`.

reference(): integers carried in float64 matrix products (every |partial sum| <= mag < 2^24, asserted: exact in any order), returned as
int64; reference_plain(): the same maps by int64 table look-ups, tap by tap, no float anywhere — tests/test_sched_cases_cpu.py ties
the two and the C oracle together on a few images.  mag = |bias| + sum |x_j c_j| >= |bias| + sum |T| bounds every partial sum of every
builder (an entry is itself a chain over x_j c_j) and of every summation order.

chunks() and sub_batches() restate which launches a forward makes (chunks of QCNN_OPT_HOST_CHUNK panels, sub-batches `panels * k / ns`), launches_of()
what each conv / FC launch looks like to the planner, predict() asks the planner library (no GPU) what runs; SCHED_REACH pins the
answers.  Plain numpy; no GPU."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np

import exact_cases as ec
import table_probe as tp
from conftest import pkg

topo = pkg("topology")
capi = pkg("capi")

PANEL = 128
SMALL_MAX = capi.SMALL_BATCH_MAX
F32_UNITS = ec.F32_UNITS

# ---------------------------------------------------------------------------------------------- the network
IN_CHW = (3, 21, 21)
LAYERS = [topo.conv(0, 3, 96, 1, 1), topo.relu(), topo.pool(0, 2, 2),            # 0 .. 2: 19 x 19 x 96 -> 10 x 10 (last window clipped)
          topo.conv(1, 3, 128, 1, 1), topo.relu(),                               # 3, 4: 10 x 10 x 128: tiles, eight-wave, sliding by panels
          topo.conv(1, 3, 128, 2, 1), topo.relu(), topo.pool(0, 5, 5),           # 5 .. 7: two groups; -> 2 x 2 x 128
          topo.fcnt(192), topo.relu(), topo.drpt(0.5),                           # 8 .. 10: D = 512 = 4 M, K = 32: k_fc_sym8's shape
          topo.fcnt(64), topo.relu(),                                            # 11, 12: Cs = 1, M = D = 192: the decoded FC
          topo.fcnt(10), topo.smax()]                                            # 13, 14
L = len(LAYERS)
SIZES = topo.fmap_sizes(IN_CHW, LAYERS)
# layer -> (M, K, Cs, amp, e_c, bias scale).  conv1: one sub-space of 3 dims (decoded; pad 0 and 96 channels: the NCHW form too)
QUANT = {0: (1, 128, 4, 2, 0, 1), 3: (12, 128, 8, 1, 0, 8), 5: (8, 128, 8, 1, 0, 128), 8: (128, 32, 4, 1, 0, 1024),
         11: (192, 16, 1, 1, 0, 8192), 13: (16, 32, 4, 1, -18, 65536)}
QLAYERS = sorted(QUANT)
RELUS = [l for l in range(L) if LAYERS[l]["type"] == topo.RELU]
LAST_FC = 13                              # its output is fm[14]
FIRST_FC = 8
N_MAX = 1027                              # nine panels, the last one holds three images
SEED = 7
RESEED = {(7, 8): 1400}                               # (seed, layer) -> offset: parameter draws chosen so that the reference meets the visibility conditions

# LRN cannot stay integer: conv -> ReLU -> LRN(5) -> pool 3x3 / 2 / 0 and nothing behind it.  27 x 27 -> 13 x 13 pool outputs = 64
# workgroups of the fused kernel per panel, so the gate 64 * (panels / ns) >= 192 opens at three panels per sub-batch
LRN_IN_CHW = (3, 27, 27)
LRN_LAYERS = [topo.conv(1, 3, 32, 1, 1), topo.relu(), topo.lorn(5, 0.01, 0.75, 2.0), topo.pool(0, 3, 2)]
LRN_QUANT = {0: (1, 128, 4, 2, 0, 1)}
LRN_N = 3 * PANEL + 1
LRN_POOL_BLOCKS = 64                      # qk_lrn_pool_blocks(13, 13) = ceil(13 / 4)^2 * (32 / 8)
LRN_MIN_BLOCKS = 192


def geom_of(layers, sizes, l):
    """(kind, table_probe geometry) of conv / FC layer l."""
    ly, (h, w, c) = layers[l], sizes[l]
    if ly["type"] == topo.CONV:
        return "conv", tp.conv_geom(h, w, c, ly["knl"], ly["stride"], ly["pad"], ly["grp"], ly["cnt"])
    return "fc", tp.fc_geom(h * w * c, ly["nod"])


def _make_params(layers, sizes, quant, seed):
    out = {}
    for l, (M, K, Cs, amp, e_c, bscale) in quant.items():
        kind, g = geom_of(layers, sizes, l)
        p = ec.exact_params(kind, g, M, K, Cs, seed + l + RESEED.get((seed, l), 0), amp, e_c)
        rng = np.random.default_rng([seed, l, 47])
        Ct = p["bias"].shape[0]
        # non-zero integers, seven of eight negative (a ReLU follows every layer but the last), in units of the layer's own scale
        neg = 0.875 if l != max(quant) else 0.5
        b = rng.integers(1, 9, size=Ct) * np.where(rng.random(Ct) < neg, -1, 1) * bscale
        # exact_params turns a zero coordinate sum into +1: negate every other code word so that neither sign leads (sums stay odd)
        p["ctrd"] = (p["ctrd"] * np.where(np.arange(K) % 2, -1.0, 1.0)[None, :, None]).astype(np.float32)
        p["bias"] = (b * 2.0 ** e_c).astype(np.float32)
        out[l] = p
    return out


@functools.lru_cache(maxsize=None)
def params():
    return _make_params(LAYERS, SIZES, QUANT, SEED)


@functools.lru_cache(maxsize=None)
def lrn_params():
    return _make_params(LRN_LAYERS, topo.fmap_sizes(LRN_IN_CHW, LRN_LAYERS), LRN_QUANT, SEED + 100)


def file_params(p):
    return {l: {k: q[k] for k in ("bias", "ctrd", "asmt", "bits")} for l, q in p.items()}


def inputs(n=N_MAX, in_chw=IN_CHW, seed=SEED):
    """NCHW float32 [n, C, H, W], every value -1 or +1."""
    rng = np.random.default_rng([seed, 53])
    return np.ascontiguousarray(rng.choice([-1.0, 1.0], size=(n,) + tuple(in_chw)).astype(np.float32))


# ---------------------------------------------------------------------------------------------- the integer reference
def int_params(p):
    """(bias, ctrd, asmt) as int64, in units of 2^e_c."""
    c = np.asarray(p["ctrd"], np.float64) / 2.0 ** p["e_c"]
    b = np.asarray(p["bias"], np.float64) / 2.0 ** p["e_c"]
    assert (c == np.rint(c)).all() and (b == np.rint(b)).all() and (b != 0).all()
    return b.astype(np.int64), c.astype(np.int64), np.asarray(p["asmt"]).astype(np.int64)


def dense_weights(kind, g, p):
    """int64 weights the code words and assignments spell out: conv [Ct][kh][kw][Cin / grp], FC [Ct][D]."""
    _, c, a = int_params(p)
    M, K, Cs = c.shape
    cse = tp.cs_eff(kind, g, M, Cs)
    Ct = a.shape[0]
    if kind == "fc":
        a = a.reshape(Ct, M)
        return np.concatenate([c[m][a[:, m]][:, :cse[m]] for m in range(M)], axis=1)
    knl = g["knl"]
    a = a.reshape(Ct, knl, knl, M)
    return np.concatenate([c[m][a[..., m]][..., :cse[m]] for m in range(M)], axis=3)


def _patches(x, g):
    """x [n, H, W, Cin] -> [n, Ho, Wo, knl, knl, Cin] with zero padding."""
    n, H, W, Cin = x.shape
    knl, s, pad = g["knl"], g["stride"], g["pad"]
    Ho, Wo = tp.out_hw(g)
    xp = np.zeros((n, H + 2 * pad, W + 2 * pad, Cin), x.dtype)
    xp[:, pad:pad + H, pad:pad + W] = x
    out = np.empty((n, Ho, Wo, knl, knl, Cin), x.dtype)
    for kh in range(knl):
        for kw in range(knl):
            out[:, :, :, kh, kw] = xp[:, kh:kh + (Ho - 1) * s + 1:s, kw:kw + (Wo - 1) * s + 1:s]
    return out


def conv_int(x, g, p, bias=True, with_mag=False):
    """int64 [n, Ho, Wo, Ct] of integer x [n, H, W, Cin]; with_mag: also |bias| + sum |x_j c_j|.  Carried in float64 products."""
    b, _, _ = int_params(p)
    Wd = dense_weights("conv", g, p).astype(np.float64)
    grp, Ct = g["grp"], g["Ct"]
    Cg, Ctg = g["Cin"] // grp, Ct // grp
    n = x.shape[0]
    Ho, Wo = tp.out_hw(g)
    out = np.empty((n, Ho, Wo, Ct))
    mag = np.empty((n, Ho, Wo, Ct)) if with_mag else None
    for i0 in range(0, n, PANEL):                         # a panel of images at a time: the patch matrix stays small
        pt = _patches(np.asarray(x[i0:i0 + PANEL], np.float64), g)
        nb = pt.shape[0]
        for gi in range(grp):
            A = pt[..., gi * Cg:(gi + 1) * Cg].reshape(nb * Ho * Wo, -1)
            Wg = Wd[gi * Ctg:(gi + 1) * Ctg].reshape(Ctg, -1)
            out[i0:i0 + nb, ..., gi * Ctg:(gi + 1) * Ctg] = (A @ Wg.T).reshape(nb, Ho, Wo, Ctg)
            if with_mag:
                mag[i0:i0 + nb, ..., gi * Ctg:(gi + 1) * Ctg] = (np.abs(A) @ np.abs(Wg).T).reshape(nb, Ho, Wo, Ctg)
    if bias:
        out += b
    out = np.rint(out).astype(np.int64)
    if with_mag:
        mag = np.rint(mag + np.abs(b)).astype(np.int64)
        assert mag.max() < 2 ** 53
        return out, mag
    return out


def fc_int(x, g, p, bias=True, with_mag=False):
    """int64 [n, Ct] of integer rows x [n, D] in consumption order."""
    b, _, _ = int_params(p)
    Wd = dense_weights("fc", g, p).astype(np.float64)
    xf = np.asarray(x, np.float64)
    out = xf @ Wd.T + (b if bias else 0)
    out = np.rint(out).astype(np.int64)
    if with_mag:
        return out, np.rint(np.abs(xf) @ np.abs(Wd).T + np.abs(b)).astype(np.int64)
    return out


def pool_int(x, ly):
    import glue_ref as gr
    return gr.pool(np.asarray(x, np.float64), ly["knl"], ly["stride"], ly["pad"]).astype(np.int64)


def flatten_nchw(fm):
    return np.ascontiguousarray(fm.transpose(0, 3, 1, 2)).reshape(fm.shape[0], -1)


def forward_int(fm, first=0, last=LAST_FC, layers=LAYERS, sizes=SIZES, prm=None, variant=None, mags=None, dtype=np.int64):
    """[fm[first], ..., fm[last + 1]] (int64 NHWC, FC maps [n, 1, 1, C]) from the integer map fm[first].  variant: {layer: f(l, x, y)
    -> y'} replaces layer l's output (the teeth); mags: a dict that receives the largest |bias| + sum |x_j c_j| per conv / FC layer."""
    prm = prm or params()
    variant = variant or {}
    out = [np.asarray(fm, dtype)]
    for l in range(first, last + 1):
        ly, x = layers[l], out[-1]
        t = ly["type"]
        if t in (topo.CONV, topo.FCNT):
            kind, g = geom_of(layers, sizes, l)
            fn, xin = (conv_int, x) if kind == "conv" else (fc_int, flatten_nchw(x))
            if mags is not None:                      # (the CPU tier asks for them, on the very batch the GPU tier runs)
                y, mag = fn(xin, g, prm[l], with_mag=True)
                assert mag.max() <= F32_UNITS, (l, int(mag.max()))
                mags[l] = max(mags.get(l, 0), int(mag.max()))
            else:
                y = fn(xin, g, prm[l])
            y = y.reshape(y.shape[0], 1, 1, -1) if kind == "fc" else y
        elif t == topo.RELU:
            y = np.maximum(x, 0)
        elif t == topo.POOL:
            y = pool_int(x, ly)
        elif t == topo.DRPT:
            y = x
        else:
            raise ValueError("layer %d cannot stay integer" % l)
        if l in variant:
            y = variant[l](l, x, y)
        out.append(np.asarray(y, dtype))
    return out


@functools.lru_cache(maxsize=None)
def reference(n=N_MAX, with_mags=False):
    """(x NCHW float32, [fm[0] .. fm[14]] int32, {layer: largest |bias| + sum |x_j c_j|} if asked for) of the first n images of
    THE batch (both tiers use N_MAX)."""
    x = inputs(N_MAX)[:n]
    mags = {} if with_mags else None
    fm = forward_int(np.rint(x.transpose(0, 2, 3, 1)).astype(np.int64), mags=mags, dtype=np.int32)      # (every value is below 2^24)
    for a in fm:
        a.setflags(write=False)
    x.setflags(write=False)
    return x, fm, mags


def unit(l):
    """2^e of feature map l: the last FC layer's output carries its code words' power of two."""
    return 2.0 ** QUANT[LAST_FC][4] if l == LAST_FC + 1 else 1.0


def as_float32(fm_l, l):
    assert np.abs(fm_l).max() <= F32_UNITS
    return (np.asarray(fm_l, np.float64) * unit(l)).astype(np.float32)


def reference_plain(x_nchw, layers=LAYERS, sizes=SIZES, prm=None, last=LAST_FC):
    """The same maps by int64 table look-ups, tap by tap: T[pixel][m] = <x_m, c>, out = bias + sum of T[pixel][m][asmt] over the taps
    inside the map.  No float anywhere; slow — for a few images."""
    prm = prm or params()
    out = [np.rint(np.asarray(x_nchw).transpose(0, 2, 3, 1)).astype(np.int64)]
    for l in range(last + 1):
        ly, x = layers[l], out[-1]
        t = ly["type"]
        if t == topo.CONV:
            _, g = geom_of(layers, sizes, l)
            b, c, a = int_params(prm[l])
            M, K, Cs = c.shape
            cse = tp.cs_eff("conv", g, M, Cs)
            n, H, W, Cin = x.shape
            knl, s, pad, grp, Ct = g["knl"], g["stride"], g["pad"], g["grp"], g["Ct"]
            Ho, Wo = tp.out_hw(g)
            Cg, Ctg = Cin // grp, Ct // grp
            a = a.reshape(Ct, knl, knl, M)
            y = np.broadcast_to(b, (n, Ho, Wo, Ct)).copy()
            for gi in range(grp):
                for m in range(M):
                    c0 = gi * Cg + m * Cs
                    T = np.einsum("nhwj,kj->nhwk", x[..., c0:c0 + cse[m]], c[m, :, :cse[m]])
                    for ho in range(Ho):
                        for wo in range(Wo):
                            for kh in range(knl):
                                for kw in range(knl):
                                    hi, wi = ho * s - pad + kh, wo * s - pad + kw
                                    if 0 <= hi < H and 0 <= wi < W:
                                        y[:, ho, wo, gi * Ctg:(gi + 1) * Ctg] += T[:, hi, wi][:, a[gi * Ctg:(gi + 1) * Ctg, kh, kw, m]]
        elif t == topo.FCNT:
            _, g = geom_of(layers, sizes, l)
            b, c, a = int_params(prm[l])
            M, K, Cs = c.shape
            n, H, W, Ch = x.shape
            rows = np.empty((n, Ch * H * W), np.int64)
            for ch in range(Ch):                              # NCHW flatten: channel-major, then rows, then columns
                for h in range(H):
                    for w in range(W):
                        rows[:, (ch * H + h) * W + w] = x[:, h, w, ch]
            a = a.reshape(g["Ct"], M)
            y = np.broadcast_to(b, (n, g["Ct"])).copy()
            for m in range(M):
                T = np.einsum("nj,kj->nk", rows[:, m * Cs:(m + 1) * Cs], c[m])
                y += T[:, a[:, m]]
            y = y.reshape(n, 1, 1, -1)
        elif t == topo.RELU:
            y = np.where(x > 0, x, 0)
        elif t == topo.POOL:
            y = pool_int(x, ly)
        elif t == topo.DRPT:
            y = x
        else:
            break
        out.append(y)
    return out


@functools.lru_cache(maxsize=None)
def lrn_reference(n=LRN_N):
    """(x NCHW, conv map int64, ReLU map int64) of the LRN table's batch."""
    x = inputs(n, LRN_IN_CHW, SEED + 100)
    sizes = topo.fmap_sizes(LRN_IN_CHW, LRN_LAYERS)
    fm = forward_int(np.rint(x.transpose(0, 2, 3, 1)).astype(np.int64), last=1, layers=LRN_LAYERS, sizes=sizes, prm=lrn_params())
    return x, fm[1], fm[2]


# ---------------------------------------------------------------------------------------------- the schedule, restated
def sub_batches(pa, pb, streams):
    """[(p0, p1)] of run_layers(pa, pb): ns = min(streams, 4, panels) sub-batches, bounds pa + panels * k / ns."""
    panels = pb - pa
    ns = max(1, min(streams, 4, panels))
    return [(pa + panels * k // ns, pa + panels * (k + 1) // ns) for k in range(ns)]


def chunks(n, chunk, host=True):
    """[(pa, pb)] of a forward of n images: qcnn_forward_host cuts a batch of at least two chunks of `chunk` panels; qcnn_forward
    (device input, and every batch of qcnn_forward_host_batches) runs it whole."""
    panels = -(-n // PANEL)
    if not host or chunk <= 0 or n < 2 * chunk * PANEL:
        return [(0, panels)]
    return [(pa, min(panels, pa + chunk)) for pa in range(0, panels, chunk)]


DEFAULTS = dict(streams=2, chunk=2, keep_all=0, split=1, lut=1, bf16split=2, direct=1, decode=1, small=1, packed=0)
OPT = dict(streams=capi.OPT_STREAMS, chunk=capi.OPT_HOST_CHUNK, keep_all=capi.OPT_KEEP_ALL, split=capi.OPT_SPLIT, lut=capi.OPT_LUT_MODE,
           bf16split=capi.OPT_DEC_BF16SPLIT, direct=capi.OPT_DIRECT_DEC, decode=capi.OPT_DECODE, small=capi.OPT_SMALL_BATCH,
           packed=capi.OPT_PACKED_FC)


def config(**kw):
    assert set(kw) <= set(DEFAULTS), kw
    return dict(DEFAULTS, **kw)


def direct_input(n, cfg):
    """qcnn_engine::direct_input for NET: does the first layer read the NCHW input in place?"""
    if cfg["keep_all"]:
        return False
    small = bool(cfg["small"]) and cfg["lut"] == 1 and n <= SMALL_MAX
    if cfg["decode"] and cfg["lut"] == 1 and not small:
        return bool(cfg["direct"])                  # the layer has the NCHW decoded form (pad 0, 96 channels)
    return True                                      # one sub-space, three input channels, K = 128


def launches_of(n, cfg, host=True):
    """[key] of every sub-batch launch of a forward, in issue order (the last one is what qcnn_get_layer_split reports):
    key = (panels, nsub, panels of all sub-batches if they run concurrently else 0, in place, small, live, split, lut, decode, direct)."""
    small = bool(cfg["small"]) and cfg["lut"] == 1 and n <= SMALL_MAX
    live = n if n <= PANEL else PANEL
    inplace = direct_input(n, cfg)
    out = []
    for pa, pb in chunks(n, cfg["chunk"], host):
        subs = sub_batches(pa, pb, cfg["streams"])
        for p0, p1 in subs:
            out.append((p1 - p0, len(subs), (pb - pa) if len(subs) > 1 else 0, int(inplace), int(small), live, cfg["split"], cfg["lut"],
                        cfg["decode"], cfg["direct"]))
    return out


class Planner:
    """qcnn_plan_conv_query / qcnn_plan_fc_query of the CPU planner library (no GPU)."""

    def __init__(self):
        lib = C.CDLL(pkg("build").build_planner_cpu())
        lib.qcnn_plan_conv_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.POINTER(C.c_int)]
        lib.qcnn_plan_fc_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.lib = lib

    def conv(self, l, panels, nsub, concurrent, nchw, split, lut):
        (h, w, c), (ho, wo, ct), ly = SIZES[l], SIZES[l + 1], LAYERS[l]
        M, K, Cs = QUANT[l][:3]
        g = (C.c_int * 14)(h, w, c, ho, wo, ct, ly["knl"], ly["stride"], ly["pad"], ly["grp"], M, Cs, K, panels)
        o = (C.c_int * 8)(split, 1, 1, 1, 1, lut, nchw | (concurrent << 1), 64 // nsub)
        ch = (C.c_int * 13)()
        assert self.lib.qcnn_plan_conv_query(g, o, None, ch) == 0
        fam, frm, Z, nseg = ch[0], ch[1], ch[2], ch[3]
        if fam in (-2, -6, -10):
            return fam, nseg
        if fam == -5:
            return fam, max(Z, 1)
        if fam in (-4, -9):
            return fam, 1
        return (frm, Z) if Z > 1 else (-1, 1)

    def fc(self, l, panels, live, split, lut, decode, small):
        h, w, c = SIZES[l]
        M, K, Cs = QUANT[l][:3]
        g = (C.c_int * 8)(h * w * c, LAYERS[l]["nod"], M, K, Cs, 1, panels, live)
        o = (C.c_int * 7)(split, 1, decode, lut, small, int(l == FIRST_FC and h * w > 1), -1)
        ch = (C.c_int * 2)()
        assert self.lib.qcnn_plan_fc_query(g, o, ch) == 0
        return ch[0], ch[1]


def predict(key, planner):
    """((code, Z) per QLAYERS) of one launch: what launch_conv / launch_fc run and report.  A k_fc_aprx launch is recorded with the
    planner's slice count; the engine reports (-1, 1) for it whatever that is (see reported())."""
    panels, nsub, pall, inplace, small, live, split, lut, decode, direct = key
    out = []
    for l in QLAYERS:
        if LAYERS[l]["type"] == topo.CONV:
            nchw = inplace if l == 0 else 0
            decoded = l == 0 and decode and lut == 1
            if decoded and ((nchw and direct) if small else True):
                out.append((-3, 2 if nchw else 1))
            elif small:
                out.append((-11, 1))
            elif lut == 0:
                out.append((-1, 1))
            else:
                out.append(planner.conv(l, pall if pall else panels, nsub, 1 if pall else 0, nchw, split, lut))
        else:
            fam, z = planner.fc(l, panels, live, split, lut, decode, small)
            if fam != -3 and small and QUANT[l][1] % 4 == 0:
                fam, z = -11, 1
            out.append((fam, z))
    return tuple(out)


def reported(pred):
    """What qcnn_get_layer_split says after a launch predicted as `pred`."""
    return tuple((-1, 1) if (LAYERS[l]["type"] == topo.FCNT and f == -1) else (f, z) for l, (f, z) in zip(QLAYERS, pred))


# ---------------------------------------------------------------------------------------------- the grid
BATCHES = (1, 3, SMALL_MAX, SMALL_MAX + 1, 60, 127, 128, 129, 131, 256, 257, 300, 385, 515, 640, 1027)
BATCHES = tuple(sorted(set(BATCHES)))
STREAMS = (1, 2, 3, 4)
CHUNKS = (0, 1, 2, 3)
CHUNK_BATCHES = (385, 640, 1027)
OPTION_BATCHES = (3, 131, 385, 1027)
OPTION_SETS = (dict(split=0), dict(lut=0), dict(bf16split=0), dict(bf16split=1), dict(direct=0), dict(decode=0), dict(small=0),
               dict(packed=1), dict(small=0, packed=1))
HOST_BATCH_LIST = (131, 3, 300, 1, 128, 640)
SEQUENCE = (1027, 3, 131, 1, 640, 1027)


def grid():
    """[(n, cfg, host)] of every forward the GPU tier makes on NET."""
    out = []
    for n in BATCHES:
        for s in STREAMS:
            out.append((n, config(streams=s), True))
        out.append((n, config(keep_all=1), True))
    for n in CHUNK_BATCHES:
        for keep in (0, 1):
            for s in STREAMS:
                for c in CHUNKS:
                    out.append((n, config(streams=s, chunk=c, keep_all=keep), True))
    for n in OPTION_BATCHES:
        for o in OPTION_SETS:
            out.append((n, config(**o), True))
            out.append((n, config(keep_all=1, **o), True))
    for n in set(HOST_BATCH_LIST) | set(SEQUENCE):
        for keep in (0, 1):
            out.append((n, config(keep_all=keep), False))
    return out


def grid_keys():
    keys = set()
    for n, cfg, host in grid():
        keys.update(launches_of(n, cfg, host))
    return sorted(keys)


# key -> ((code, Z) of conv1, conv2, conv3, fc1, fc2, fc3).  Written by `python tests/sched_cases.py` from the planner library of this tree;
# tests/test_sched_cases_cpu.py re-derives every row and checks that the grid produces exactly these keys.
SCHED_REACH = {
    (1, 1, 0, 0, 0, 3, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 3, 1, 1, 1, 1): ((-3, 1), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 4, 1, 1, 1, 1): ((-3, 1), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 60, 1, 1, 1, 1): ((-3, 1), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 127, 1, 1, 1, 1): ((-3, 1), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 128, 0, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-5, 2), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 128, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 128, 1, 1, 0, 1): ((-1, 1), (0, 6), (0, 6), (-1, 4), (-1, 3), (-1, 1)),
    (1, 1, 0, 0, 0, 128, 1, 1, 1, 0): ((-3, 1), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 0, 1, 1, 1, 1, 1, 1): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 0, 1, 3, 0, 1, 1, 1): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 0, 1, 3, 1, 1, 0, 1): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-11, 1), (-11, 1)),
    (1, 1, 0, 0, 1, 3, 1, 1, 1, 0): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 0, 1, 3, 1, 1, 1, 1): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 1, 0, 3, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 3, 1, 1, 1, 1): ((-3, 2), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 4, 1, 1, 1, 1): ((-3, 2), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 60, 1, 1, 1, 1): ((-3, 2), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 127, 1, 1, 1, 1): ((-3, 2), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 128, 0, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-5, 2), (-3, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 128, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (1, 1, 0, 1, 0, 128, 1, 1, 0, 1): ((-1, 1), (0, 6), (0, 6), (-1, 4), (-1, 3), (-1, 1)),
    (1, 1, 0, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 6), (0, 6), (-1, 4), (-3, 1), (-1, 1)),
    (1, 1, 0, 1, 1, 1, 1, 1, 1, 1): ((-3, 2), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 1, 1, 3, 0, 1, 1, 1): ((-3, 2), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 1, 1, 3, 1, 1, 0, 1): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-11, 1), (-11, 1)),
    (1, 1, 0, 1, 1, 3, 1, 1, 1, 0): ((-11, 1), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 1, 0, 1, 1, 3, 1, 1, 1, 1): ((-3, 2), (-11, 1), (-11, 1), (-11, 1), (-3, 1), (-11, 1)),
    (1, 2, 2, 0, 0, 128, 0, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-5, 2), (-3, 1), (-1, 1)),
    (1, 2, 2, 0, 0, 128, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (1, 2, 2, 0, 0, 128, 1, 1, 0, 1): ((-1, 1), (0, 3), (0, 3), (-1, 4), (-1, 3), (-1, 1)),
    (1, 2, 2, 0, 0, 128, 1, 1, 1, 0): ((-3, 1), (0, 3), (0, 3), (-1, 4), (-3, 1), (-1, 1)),
    (1, 2, 2, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 3), (0, 3), (-1, 4), (-3, 1), (-1, 1)),
    (1, 2, 2, 1, 0, 128, 0, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-5, 2), (-3, 1), (-1, 1)),
    (1, 2, 2, 1, 0, 128, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (1, 2, 2, 1, 0, 128, 1, 1, 0, 1): ((-1, 1), (0, 3), (0, 3), (-1, 4), (-1, 3), (-1, 1)),
    (1, 2, 2, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 3), (0, 3), (-1, 4), (-3, 1), (-1, 1)),
    (1, 2, 3, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 2, 3, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 3, 3, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 3, 3, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 3, 4, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 3, 4, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 3, 5, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (1, 3, 5, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (1, 4, 4, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 4, 4, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (1, 4, 5, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (1, 4, 5, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 1, 0, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 3), (0, 3), (-1, 4), (-3, 1), (-1, 1)),
    (2, 1, 0, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 3), (0, 3), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 3, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 3, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 4, 0, 0, 128, 0, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-5, 2), (-3, 1), (-1, 1)),
    (2, 2, 4, 0, 0, 128, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (2, 2, 4, 0, 0, 128, 1, 1, 0, 1): ((-1, 1), (-5, 3), (0, 2), (-1, 4), (-1, 3), (-1, 1)),
    (2, 2, 4, 0, 0, 128, 1, 1, 1, 0): ((-3, 1), (-5, 3), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 4, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-5, 3), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 4, 1, 0, 128, 0, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-5, 2), (-3, 1), (-1, 1)),
    (2, 2, 4, 1, 0, 128, 1, 0, 1, 1): ((-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1), (-1, 1)),
    (2, 2, 4, 1, 0, 128, 1, 1, 0, 1): ((-1, 1), (-5, 3), (0, 2), (-1, 4), (-1, 3), (-1, 1)),
    (2, 2, 4, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-5, 3), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 5, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-5, 3), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 2, 5, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-5, 3), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 3, 4, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 3, 4, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 3, 5, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 3, 5, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 4, 5, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 4, 5, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-1, 1), (-1, 1), (-1, 4), (-3, 1), (-1, 1)),
    (2, 4, 9, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-2, 2), (-2, 2), (-1, 4), (-3, 1), (-1, 1)),
    (2, 4, 9, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-2, 2), (-2, 2), (-1, 4), (-3, 1), (-1, 1)),
    (3, 1, 0, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (0, 2), (0, 2), (-5, 4), (-3, 1), (-1, 1)),
    (3, 1, 0, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (0, 2), (0, 2), (-5, 4), (-3, 1), (-1, 1)),
    (3, 2, 5, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-5, 3), (-1, 1), (-5, 4), (-3, 1), (-1, 1)),
    (3, 2, 5, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-5, 3), (-1, 1), (-5, 4), (-3, 1), (-1, 1)),
    (3, 3, 9, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (3, 3, 9, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (3, 4, 9, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (3, 4, 9, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (4, 1, 0, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-5, 3), (0, 2), (-5, 4), (-3, 1), (-1, 1)),
    (4, 1, 0, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-5, 3), (0, 2), (-5, 4), (-3, 1), (-1, 1)),
    (4, 2, 9, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (4, 2, 9, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (5, 1, 0, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-5, 3), (-1, 1), (-5, 4), (-3, 1), (-1, 1)),
    (5, 1, 0, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-5, 3), (-1, 1), (-5, 4), (-3, 1), (-1, 1)),
    (5, 2, 9, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (5, 2, 9, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (9, 1, 0, 0, 0, 128, 1, 1, 1, 1): ((-3, 1), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
    (9, 1, 0, 1, 0, 128, 1, 1, 1, 1): ((-3, 2), (-2, 2), (-2, 2), (-5, 4), (-3, 1), (-1, 1)),
}


if __name__ == "__main__":
    pl = Planner()
    for k in grid_keys():
        print("    %r: %r," % (k, predict(k, pl)))
