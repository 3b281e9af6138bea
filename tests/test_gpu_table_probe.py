"""One-hot table probes through every conv / FC kernel family (tests/table_probe.py; the CPU tier pins the helper to the oracle
in tests/test_table_probe_cpu.py).

A probe's parameters make every output ONE look-up-table entry plus exact zeros, so per entry, relative to the entry's own
magnitude sum_j |x_j c_j| (nothing here is a max-norm over a map, and no bar is taken from what a kernel returns):

  * every f32 builder (exact VALU, f32 MFMA = a k-ordered fmaf chain) and the f32 decoded layers stay within
    gamma_CsEff = CsEff u / (1 - CsEff u), u = 2^-24, of the float64 entry; a one-dim sub-space is one rounding: u;
  * the exact builder (and every layer with K > 128, which always runs it) returns the float32 sequence
    acc = acc + x_j * c_j bit for bit;
  * summation order no longer exists, so every f32 table family — sliding, symmetric, eight-wave, half-panel, split tiles,
    few-image kernels, k_fc_sym8 with its split sub-space axis — returns the bits of the tile kernel with the same builder;
  * the split-bf16 first layer stays within (2^-22 + gamma_(6 CsEff)) (six cross terms per product, <= 6 CsEff additions);
  * the fp16 table modes return the f32 entry rounded once to fp16, round to nearest even (v_cvt_pk_f16_f32), bit for bit;
  * a tap in the padding gives exactly 0; an image's entries do not depend on its position in a panel or on the batch.

Every case asserts the family code qcnn_get_layer_split reports (a silent fall-back to another family fails the case; the
few-image kernels report (-11, 1) when they took the launch, and the panel kernel's code when the layer fell through to it)
and prints its worst err / bound.
Layer-for-layer cases go through qcnn_run_layer (any NHWC input, panel kernels, no ReLU); what only a forward reaches (the
few-image kernels, the first layer read in place) goes through qcnn_forward_host, with the code book negated in a second
pass where ReLU is fused.  fc6 (9216 -> 4096) runs ONE thinned round: 5.7 % of its 2304 x 31 (m, k) pairs, every m and every k.
The sm_* / fc_m900 / fc_k128 / fc_k20 / fc_k16_m1800 shapes are the smallest at which each sub-space chunk, stage group and tile
edge of the few-image kernels is live (table_probe.SMALL_REACH; tests/test_small_cases_cpu.py re-derives the launchers' choice);
tests/test_gpu_small_cases.py runs the same shapes on dense sums.
The dn_* / dp_* / fcd_* shapes are the smallest at which each launch variant of the decoded kernels (qcnn_decoded.hip) is live
(table_probe.DEC_REACH; tests/test_decoded_cases_cpu.py re-derives the launchers' choice): dn_* first layers read in place — the
three k orders of the split-bf16 kernel, the f32 kernel, the shape only the f32 kernel takes —, dp_* the ten k_conv_dec
instantiations (the 16-image ones only through a forward, whose launch knows how many images its panel holds), fcd_* k_fc_dec's
ring tails, ragged channel block, stage groups and, under QCNN_OPT_SPLIT, its k slices; every decoded family runs them at 131,
70, 17, 16 and 5 images (in place also at 3 and 1).  tests/test_gpu_decoded_cases.py runs the same shapes on dense sums."""
import numpy as np
import pytest

import table_probe as tp
from conftest import pkg

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")

N_IMG = 131                      # a full panel and a ragged one of three images
BASE = dict(lut=capi.LUT_MFMA, keep_all=1, split=0, decode=0, slide=0, sym=0, sym8=0, half8=0, small=0, packed=0, direct=1, bf16split=1)
OPT = dict(lut=capi.OPT_LUT_MODE, keep_all=capi.OPT_KEEP_ALL, split=capi.OPT_SPLIT, decode=capi.OPT_DECODE, slide=capi.OPT_SLIDE,
           sym=capi.OPT_SYM, sym8=capi.OPT_SYM8, half8=capi.OPT_HALF8, small=capi.OPT_SMALL_BATCH, packed=capi.OPT_PACKED_FC,
           direct=capi.OPT_DIRECT_DEC, bf16split=capi.OPT_DEC_BF16SPLIT)


def fam(label, code, via="layer", n=(N_IMG,), like_tile=True, exact=False, relu=False, split_bf16=False, f16=False, **opts):
    """One kernel family of a case.  code: what layer_split must report — a pair, or (family, None) for 'any slice count',
    or ('split', None) for split tiles (first split tile >= 0, more than one slice)."""
    return dict(label=label, code=code, via=via, n=tuple(n), like_tile=like_tile, exact=exact, relu=relu, split_bf16=split_bf16,
                f16=f16, opts=dict(BASE, **opts))


EXACT = fam("exact builder, tile", (-1, 1), like_tile=False, exact=True, lut=capi.LUT_EXACT)
TILE = fam("MFMA builder, tile", (-1, 1), like_tile=False)
SLIDE = fam("sliding", (-2, None), slide=2)
SYM = fam("symmetric", (-4, 1), sym=2)
SYM8 = fam("eight-wave tile", (-5, 1), sym8=2)
SYM8S = fam("eight-wave sliding", (-6, None), sym8=3)
HALF8 = fam("half-panel tile", (-9, 1), n=(N_IMG, 5, 70), half8=2)
HALF8S = fam("half-panel sliding", (-10, None), n=(N_IMG, 5, 70), half8=3)
SPLIT_TILE = fam("split tiles, tile", ("split", None), n=(125,), split=1)
SPLIT_SYM8 = fam("split tiles, eight-wave", (-5, "cut"), n=(125,), split=1, sym8=2)
SMALL = fam("few-image", (-11, 1), via="forward", n=(1, 3), small=1)
SMALL_PACKED = fam("few-image, packed FC", (-11, 1), via="forward", n=(1, 3), small=1, packed=1)
F16_CONV = [fam("fp16 tables", (-7, 1), like_tile=False, f16=True, lut=capi.LUT_MFMA_F16, sym8=2),
            fam("fp16 tables + sums", (-8, 1), like_tile=False, f16=True, lut=capi.LUT_MFMA_F16ACC, sym8=2)]
F16_FC = [fam("fp16 tables", (-7, None), like_tile=False, f16=True, lut=capi.LUT_MFMA_F16, sym8=1),
          fam("fp16 tables + sums", (-8, None), like_tile=False, f16=True, lut=capi.LUT_MFMA_F16ACC, sym8=1)]
FC_SYM8 = fam("k_fc_sym8", (-5, None), n=(N_IMG, 5, 70), sym8=1)
DEC_PANEL = fam("decoded, panel form", (-3, 1), like_tile=False, decode=1)
DEC_NCHW = fam("decoded in place, f32", (-3, 2), via="forward", like_tile=False, relu=True, decode=1, keep_all=0, bf16split=0)
DEC_SPLIT = fam("decoded in place, split-bf16", (-3, 2), via="forward", like_tile=False, relu=True, split_bf16=True, decode=1,
                keep_all=0, bf16split=1)
DEC_FC = fam("decoded FC", (-3, 1), like_tile=False, decode=1)
DECODED = [EXACT, TILE, DEC_PANEL, DEC_NCHW, DEC_SPLIT]
# the decoded families at every batch size of table_probe.DEC_BATCHES.  A forward tells the launch how many images its one panel
# holds (qcnn_run_layer always launches whole panels): only there do batches of <= 16 images reach the 16-image instantiations of
# k_conv_dec and batches of <= 64 the one-half grid of k_fc_dec
FWD_N = tuple(n for n in tp.DEC_BATCHES if n != N_IMG)
DEC_PANEL_FWD = fam("decoded, panel form, forward", (-3, 1), via="forward", n=FWD_N, like_tile=False, decode=1)
DEC_NCHW_N = dict(DEC_NCHW, n=tp.DEC_BATCHES)
DEC_SPLIT_N = dict(DEC_SPLIT, n=tp.DEC_BATCHES)
DEC_NCHW_FEW = fam("decoded in place, f32, few images", (-3, 2), via="forward", n=tp.DEC_NCHW_FEW, like_tile=False, relu=True, decode=1,
                   keep_all=0, bf16split=0, small=1)
DEC_SPLIT_FEW = fam("decoded in place, split-bf16, few images", (-3, 2), via="forward", n=tp.DEC_NCHW_FEW, like_tile=False, relu=True,
                    split_bf16=True, decode=1, keep_all=0, bf16split=1, small=1)
DEC_FC_FWD = fam("decoded FC, forward", (-3, 1), via="forward", n=FWD_N, like_tile=False, decode=1)
DEC_FC_SLICES = fam("decoded FC, k slices", (-3, "cut"), like_tile=False, decode=1, split=1)
DEC_FC_SLICES_FWD = fam("decoded FC, k slices, forward", (-3, "cut"), via="forward", n=FWD_N, like_tile=False, decode=1, split=1)


def dec_families(name):
    reach = tp.DEC_REACH[name]
    if name.startswith("dp_"):
        return [EXACT, TILE, DEC_PANEL, DEC_PANEL_FWD]
    if name.startswith("fcd_"):
        return [EXACT, TILE, DEC_FC, DEC_FC_FWD] + ([DEC_FC_SLICES, DEC_FC_SLICES_FWD] if reach[4] > 1 else [])
    f32_only = dict(split_bf16=False) if reach[0] == "f32" else {}      # only the f32 kernel is eligible: its bound under both option values
    fams = [EXACT, TILE, DEC_PANEL, DEC_PANEL_FWD, DEC_NCHW_N, dict(DEC_SPLIT_N, **f32_only)]
    if tp.SHAPES[name][3] == 128:
        return fams + [DEC_NCHW_FEW, dict(DEC_SPLIT_FEW, **f32_only)]
    # another K: few images go to the few-image table kernel when it is on, and to the in-place kernel like every batch when it is off
    return fams[:4] + [dict(f, n=tp.DEC_BATCHES + tp.DEC_NCHW_FEW) for f in fams[4:]]


DEC_CASES = [n for n in tp.DEC_NCHW_SHAPES + tp.DEC_PANEL_SHAPES + tp.DEC_FC_SHAPES if n != "dp_half_items"]
WIDE = [EXACT, TILE, SLIDE, SYM8, SYM8S, HALF8, HALF8S]

CASES = [
    ("alex_conv2", [EXACT, TILE, SLIDE, SYM, SYM8, SYM8S, HALF8, SPLIT_TILE, SPLIT_SYM8]),
    ("c3_64", [EXACT, TILE, SLIDE]),
    ("c3_128", [EXACT, TILE, SLIDE, SYM, SYM8, SYM8S, HALF8, HALF8S, SPLIT_SYM8] + F16_CONV),
    ("partial", [EXACT, TILE, SLIDE, SPLIT_TILE]),
    ("cs4_2x2", [EXACT, TILE, SLIDE, SYM, SYM8, HALF8]),
    ("rgb7", [EXACT, TILE, SPLIT_TILE, SMALL]),
    ("s5x5_2", [EXACT, TILE, SLIDE, SYM8, SYM8S]),
    ("c192", WIDE), ("c256", WIDE), ("c384", WIDE), ("c512", WIDE), ("c256_cs4", WIDE),
    ("k10", [EXACT, TILE]), ("k64", [EXACT, TILE]),
    ("k200", [EXACT, dict(TILE, exact=True)]), ("k256", [EXACT, dict(TILE, exact=True)]),   # K > 128: the exact-builder kernels in every mode
    ("alex_conv1", DECODED), ("dec4", DECODED), ("dec1", DECODED),
    ("fc512", [EXACT, TILE, FC_SYM8, SMALL, SMALL_PACKED] + F16_FC),
    ("fc6", [TILE, FC_SYM8]),
    ("fc200", [EXACT, TILE, FC_SYM8]),
    ("fc_k16", [EXACT, TILE, DEC_FC]),
] + [(name, [EXACT, TILE, SMALL] + ([SMALL_PACKED] if tp.SHAPES[name][0] == "fc" else [])) for name in sorted(tp.SMALL_REACH)] + [
    (name, dec_families(name)) for name in DEC_CASES]

FC_FRONT = {512: ((3, 3, 3), topo.conv(0, 3, 512, 1, 1)), 256: ((3, 3, 3), topo.conv(0, 3, 256, 1, 1)),
            9216: ((16, 6, 6), topo.conv(1, 3, 256, 1, 1))}      # a conv layer (no ReLU behind it) whose map has D elements
FC_FRONT.update({d: ((3, 3, 3), topo.conv(0, 3, d, 1, 1)) for d in (3600, 920, 240, 1800)})
FC_FRONT.update({d: ((3, 3, 3), topo.conv(0, 3, d, 1, 1)) for d in (64, 128, 192, 320, 640, 768, 2048)})


def model_of(name):
    """(in_chw, layers, probed layer): a conv shape is the first layer of [conv, relu, fcnt(8), smax]; an FC shape sits behind a
    conv layer whose 1x1 (fc6: 6x6) map it consumes: [conv, fcnt, smax]."""
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    if kind == "conv":
        return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"]), topo.relu(),
                                            topo.fcnt(8), topo.smax()], 0
    in_chw, front = FC_FRONT[g["D"]]
    return in_chw, [front, topo.fcnt(g["Ct"]), topo.smax()], 1


def file_params(p):
    return {k: p[k] for k in ("bias", "ctrd", "asmt", "bits")}


def make_engine(name, opts, params0):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    in_chw, layers, l = model_of(name)
    spec = synth.quant_spec(in_chw, layers)
    spec[l] = dict(spec[l], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=11, spec=spec)
    params[l] = file_params(params0)
    eng = pkg("engine").QcnnEngine(0)
    for k, v in opts.items():
        eng.set_option(OPT[k], v)
    eng.load_model(in_chw, layers, params, N_IMG)
    return eng


def code_ok(code, got):
    if code[0] == "split":
        return got[0] >= 0 and got[1] > 1
    if code[1] == "cut":
        return got[0] == code[0] and got[1] > 1
    return got[0] == code[0] and (code[1] is None or got[1] == code[1])


def run(eng, name, f, x, images):
    """Output of the probed layer for input x: (y, the input the layer consumed)."""
    kind, g = tp.SHAPES[name][:2]
    l = model_of(name)[2]
    n = x.shape[0]
    if f["via"] == "layer":
        y = eng.run_layer(l, x, n)
        return (y if kind == "conv" else y.reshape(n, -1)), x
    if kind == "conv":                                   # the probed layer is the first one: the network input is its input
        eng.forward_host(np.ascontiguousarray(x.transpose(0, 3, 1, 2)))
        return eng.layer_output(2 if f["relu"] else 1, n), x      # fast path: the conv map is fused away, the ReLU map is its clamp
    eng.forward_host(images[:n])                        # FC behind a conv layer: its input is that layer's map (1x1: NHWC = NCHW)
    return eng.layer_output(2, n).reshape(n, -1), eng.layer_output(1, n).reshape(n, -1)


@pytest.mark.parametrize("name,fams", CASES, ids=[c[0] for c in CASES])
def test_table_probe(name, fams):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    l = model_of(name)[2]
    cse = max(tp.cs_eff(kind, g, M, Cs))
    relu = any(f["relu"] for f in fams)
    rounds = tp.shape_rounds(name, negate=relu)
    p0 = tp.probe_params(kind, g, M, K, Cs, rounds[0], seed=31)
    engines = [make_engine(name, f["opts"], p0) for f in fams]
    c, h, w = model_of(name)[0]
    images = tp.activations("conv", dict(H=h, W=w, Cin=c), N_IMG, seed=33, scaled=False).transpose(0, 3, 1, 2)   # (forwards of FC cases)
    labels = [f["label"] for f in fams]
    worst = {f["label"]: 0.0 for f in fams}
    share = 1.0
    for ri, rd in enumerate(rounds):
        params = tp.probe_params(kind, g, M, K, Cs, rd, seed=31)
        for eng in engines:
            eng.upload({l: file_params(params)})
        for scaled in (False, True):
            x = tp.activations(kind, g, N_IMG, seed=32 + ri, scaled=scaled)
            want64, mag, seq = tp.expected(kind, g, x, params)
            share = min(share, tp.informative_share(mag))
            tile = None
            for f, eng in zip(fams, engines):
                if f["f16"] and scaled:                   # 2^-20 .. 2^20 times a normal value leaves the fp16 range
                    continue
                what = "%s / %s / round %d%s" % (name, f["label"], ri, " scaled" if scaled else "")
                for n in f["n"]:
                    y, xin = run(eng, name, f, x[:n], images)
                    xin = x if xin.shape == x[:n].shape and np.array_equal(xin, x[:n]) else xin
                    got = eng.layer_split(l)
                    assert code_ok(f["code"], got), "%s: family code %r, expected %r" % (what, got, f["code"])
                    if xin is x:
                        w64, mg, sq = want64[:n], mag[:n], seq[:n]
                    else:                                 # (few-image FC: the forward's own conv map is the input)
                        w64, mg, sq = tp.expected(kind, g, xin, params)
                        assert tp.informative_share(mg) >= 0.5
                    if f["f16"]:
                        assert tile is not None
                        want = tile[:n].astype(np.float16).astype(np.float32)       # numpy rounds to nearest even
                        assert np.array_equal(y, want), "%s: %d entries are not the f32 entry rounded once to fp16" % (what, int((y != want).sum()))
                        continue
                    extra = tp.split_extra(cse) if f["split_bf16"] else 0.0
                    r = tp.check(y, w64, mg, cse, extra=extra, relu=f["relu"], what=what)
                    worst[f["label"]] = max(worst[f["label"]], r)
                    if f["exact"]:
                        assert np.array_equal(y, sq), "%s: %d entries differ from the float32 sequence" % (what, int((y != sq).sum()))
                    if f["label"] == TILE["label"] and n == N_IMG:
                        tile = y
                    if f["like_tile"]:
                        if f["via"] == "layer":
                            ref = tile[:n]
                        else:                             # the tile kernel on the input this forward consumed
                            ref = run(engines[labels.index(TILE["label"])], name, TILE, xin if xin is not x else x[:n], images)[0]
                        assert np.array_equal(y, ref), "%s: %d entries differ from the tile kernel's" % (what, int((y != ref).sum()))
                    if n == N_IMG:                        # the ragged panel's three images alone: same entries in any panel position
                        alone, _ = run(eng, name, f, x[N_IMG - 3:], images)
                        assert np.array_equal(alone, y[N_IMG - 3:]), "%s: the last three images alone differ" % what
    for eng in engines:
        eng.close()
    assert share >= 0.5, share
    if tp.SHAPES[name][5] is not None:
        print("%s: %.1f %% of the (m, k) pairs" % (name, 100.0 * tp.covered(kind, g, M, K, rounds)[0].mean()))
    for f in fams:
        print("%s: %s code %r worst err / bound %.3f" % (name, f["label"], f["code"], worst[f["label"]]))
    assert all(v <= 1.0 for v in worst.values())
