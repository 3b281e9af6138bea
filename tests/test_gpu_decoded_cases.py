"""Dense sums, batch invariance and window isolation through the decoded kernels (qcnn_decoded.hip: k_conv_dec, k_conv_dec_nchw,
k_conv_dec_nchw_split, k_fc_dec + k_sum_partials) on the shapes at which each of their launch variants is live
(table_probe.DEC_REACH; tests/test_decoded_cases_cpu.py pins the launchers' choice and shows that float32 emulations of the three
sums meet the bounds used here).

A probe output (tests/test_gpu_table_probe.py) is one table entry plus zeros; here the parameters are ordinary random ones
(synth.make_params), so every tap contributes.  Per output ELEMENT, against the float64 sum of table_probe.dense_expected and
relative to the element's own mag = |bias| + sum |x_j c_j| (no max-norm over a map; table_probe.dec_dense_rel):

    f32 decoded conv, both forms      gamma(Cin knl^2 + 1) * mag             a chain of one-rounding multiply-adds onto the bias
    split-bf16 in place               (2^-22 + gamma(6 Cin knl^2 + 1)) * mag  six exact terms per product, one rounding per addition
    decoded FC, any slice count       gamma(D + 1) * mag

— derived, not measured, and valid for any summation order.  A misread tap is off by about mag / (Cin knl^2): 50 or more f32
bounds (25 split bounds) on every shape here.  Where ReLU is fused (the in-place path) the map is the clamp, which does not
increase the distance to max(want, 0); a second pass with bias and code book negated shows the other sign.

Beside the bound every case asserts, after EVERY forward, which kernel ran (qcnn_get_layer_split: (-3, 2) in place, (-3, 1) panel
form and FC, (-3, z) with the planner's own slice count under QCNN_OPT_SPLIT), and with QCNN_OPT_SPLIT = 0 that every image's
outputs are bit-equal across batches of 131, 70, 17, 16 and 5 images (in place also 3 and 1) — for the panel form that crosses
the boundary between the 64- and the 16-image instantiations — and that the three images of a ragged second panel are bit-equal
to the same images alone.  dn_f32_only (eligible for the f32 in-place kernel but for neither split order) returns the same bits
under both values of QCNN_OPT_DEC_BF16SPLIT; dn_k5 must differ somewhere, or the option would be dead.  Two shapes must NOT decode
(K > 128: pseudo sub-spaces): they report another code and meet the same bounds.

Window isolation: ONE input element (or all of image 1) is NaN; every output whose window does not hold it must equal the clean
run bit for bit, every output whose window does must be NaN (fused ReLU: NaN or 0), and a NaN in a column no window covers must
change nothing.  Ordinary arithmetic on NaN inputs: nothing reads outside a buffer."""
import ctypes as C

import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_gpu_table_probe import BASE, FC_FRONT, OPT

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")

N_IMG = tp.DEC_BATCHES[0]
FWD = tp.DEC_BATCHES[1:]


def shape_of(name):
    return tp.SHAPES[name] if name in tp.SHAPES else tp.DEC_NOT[name]


def model_for(kind, g):
    if kind == "conv":
        return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"]), topo.relu(),
                                            topo.fcnt(8), topo.smax()], 0
    in_chw, front = FC_FRONT[g["D"]]
    return in_chw, [front, topo.fcnt(g["Ct"]), topo.smax()], 1


def make(name, seed, max_batch=N_IMG, **opts):
    """(engine, the layer under test, its parameters) of a shape with ordinary random parameters."""
    kind, g, M, K, Cs, _ = shape_of(name)
    in_chw, layers, l = model_for(kind, g)
    spec = synth.quant_spec(in_chw, layers)
    spec[l] = dict(spec[l], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=seed, spec=spec)
    eng = pkg("engine").QcnnEngine(0)
    for k, v in dict(BASE, decode=1, **opts).items():
        eng.set_option(OPT[k], v)
    eng.load_model(in_chw, layers, params, max_batch)
    return eng, l, params[l]


def images(kind, g, n, seed):
    """(NHWC input of the network, the same as the NCHW batch a forward takes)."""
    in_chw = model_for(kind, g)[0]
    x = tp.activations("conv", dict(H=in_chw[1], W=in_chw[2], Cin=in_chw[0]), n, seed=seed, scaled=False)
    return x, np.ascontiguousarray(x.transpose(0, 3, 1, 2))


def negated(p):
    return dict(p, bias=-p["bias"], ctrd=-p["ctrd"])


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------- first layers read in place ----
IN_PLACE = tp.DEC_NCHW_SHAPES


IN_PLACE_BATCHES = tp.DEC_BATCHES + tp.DEC_NCHW_FEW


@pytest.mark.parametrize("name", IN_PLACE)
def test_dense_sums_in_place(name):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    x, inp = images(kind, g, N_IMG, 91)
    out = {}
    worst = {}
    for label, split in (("f32", 0), ("split-bf16", 1)):
        # QCNN_OPT_SMALL_BATCH on: one to three images still take the in-place kernel (K = 128; with another K the few-image table
        # kernel would take them, which reads the input densely: those shapes run with the option off)
        eng, l, p = make(name, 90, keep_all=0, bf16split=split, small=int(K == 128))
        is_split = bool(split) and tp.DEC_REACH[name][0] != "f32"
        rel = tp.dec_dense_rel(kind, g, is_split)
        for sign, params in ((1.0, p), (-1.0, negated(p))):
            eng.upload({l: {k: params[k] for k in ("bias", "ctrd", "asmt", "bits")}})
            want64, mag = tp.dense_expected(kind, g, x, params)
            ys = {}
            for n in IN_PLACE_BATCHES:
                eng.forward_host(inp[:n])
                assert eng.layer_split(l) == (-3, 2), "%s %s at %d images: family code %r" % (name, label, n, eng.layer_split(l))
                ys[n] = eng.layer_output(2, n)
            r = tp.dense_check_rel(ys[N_IMG], np.maximum(want64, 0.0), mag, rel, what="%s %s sign %+d" % (name, label, sign))
            worst[label] = max(worst.get(label, 0.0), r)
            assert (ys[N_IMG] > 0).mean() > 0.2                      # the clamp leaves something to look at
            for n, y in ys.items():
                assert same_bits(y, ys[N_IMG][:n]), "%s %s: %d images differ from the same images in the batch of %d: %d elements" % (
                    name, label, n, N_IMG, int((y != ys[N_IMG][:n]).sum()))
            eng.forward_host(inp[N_IMG - 3:])
            assert eng.layer_split(l) == (-3, 2)
            assert same_bits(eng.layer_output(2, 3), ys[N_IMG][N_IMG - 3:]), "%s %s: the ragged panel's three images alone differ" % (name, label)
            out[label, sign] = ys[N_IMG]
        eng.close()
    print("%s: worst err / bound %s" % (name, ", ".join("%s %.3f" % kv for kv in worst.items())))
    assert all(v <= 1.0 for v in worst.values())
    for sign in (1.0, -1.0):
        if tp.DEC_REACH[name][0] == "f32":
            assert same_bits(out["f32", sign], out["split-bf16", sign]), "only the f32 kernel is eligible: the option must change nothing"
        elif name == "dn_k5":
            assert not same_bits(out["f32", sign], out["split-bf16", sign]), "QCNN_OPT_DEC_BF16SPLIT changes nothing: a dead option"


# ---------------------------------------------------------------- panel form ----
PANEL_FORM = [n for n in tp.DEC_PANEL_SHAPES if n != "dp_half_items"] + ["dn_k5", "dn_ct288"]


def panel_case(name, code_ok, rel_of, seed=92):
    kind, g, M, K, Cs, _ = shape_of(name)
    x, inp = images(kind, g, N_IMG, seed + 1)
    eng, l, p = make(name, seed)
    want64, mag = tp.dense_expected(kind, g, x, p)
    y = eng.run_layer(l, x, N_IMG)
    assert code_ok(eng.layer_split(l)), "%s layer-for-layer: family code %r" % (name, eng.layer_split(l))
    worst = tp.dense_check_rel(y, want64, mag, rel_of(kind, g), what=name)
    alone = eng.run_layer(l, x[N_IMG - 3:], 3)
    assert same_bits(alone, y[N_IMG - 3:]), "%s: the ragged panel's three images alone differ" % name
    for n in tp.DEC_BATCHES:
        eng.forward_host(inp[:n])
        assert code_ok(eng.layer_split(l)), "%s forward of %d: family code %r" % (name, n, eng.layer_split(l))
        yn = eng.layer_output(1, n)
        assert same_bits(yn, y[:n]), "%s: a forward of %d images differs from the same images of the batch of %d: %d elements" % (
            name, n, N_IMG, int((yn != y[:n]).sum()))
    eng.close()
    return worst


@pytest.mark.parametrize("name", PANEL_FORM)
def test_dense_sums_panel_form(name):
    worst = panel_case(name, lambda code: code == (-3, 1), tp.dec_dense_rel)
    print("%s: worst err / bound %.3f" % (name, worst))
    assert worst <= 1.0


def test_dense_sums_half_items():
    """One panel of 128 images on a 46 x 46 map: 4232 items of 96 channels, which run as half-items of 48 (k_conv_dec<3, 1, false, 3, 4>)."""
    name = "dp_half_items"
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    x, _ = images(kind, g, 128, 95)
    eng, l, p = make(name, 94, max_batch=128)
    y = eng.run_layer(l, x, 128)
    assert eng.layer_split(l) == (-3, 1)
    eng.close()
    want64, mag = tp.dense_expected_one_subspace(g, x, p)
    worst = tp.dense_check_rel(y, want64, mag, tp.dec_dense_rel(kind, g), what=name)
    print("%s: worst err / bound %.3f" % (name, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- decoded FC ----
def fc_plan(eng, g, M, K, Cs, n, split):
    """(family, slices) of qcnn_plan_fc_query for a forward of n images."""
    eng.lib.qcnn_plan_fc_query.argtypes = [C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    panels = -(-n // 128)
    ch = (C.c_int * 2)()
    geom = (g["D"], g["Ct"], M, K, Cs, 1, panels, n if panels == 1 else 128)
    assert eng.lib.qcnn_plan_fc_query((C.c_int * 8)(*geom), (C.c_int * 7)(split, 0, 1, 1, 0, 0, -1), ch) == 0
    return ch[0], ch[1]


def fc_case(name, split, seed=96):
    """Forwards of every batch size: dict n -> (input the layer consumed, its output), the worst err / bound, the codes."""
    kind, g, M, K, Cs, _ = shape_of(name)
    _, inp = images(kind, g, N_IMG, seed + 1)
    eng, l, p = make(name, seed, split=split)
    outs, codes, worst = {}, {}, 0.0
    for n in tp.DEC_BATCHES:
        eng.forward_host(inp[:n])
        codes[n] = eng.layer_split(l)
        assert codes[n] == fc_plan(eng, g, M, K, Cs, n, split), "%s at %d images: family code %r, the planner says %r" % (
            name, n, codes[n], fc_plan(eng, g, M, K, Cs, n, split))
        xin, y = eng.layer_output(1, n).reshape(n, -1), eng.layer_output(2, n).reshape(n, -1)
        want64, mag = tp.dense_expected(kind, g, xin, p)
        worst = max(worst, tp.dense_check_rel(y, want64, mag, tp.dec_dense_rel(kind, g), what="%s at %d images" % (name, n)))
        outs[n] = (xin, y)
    xin, y = outs[N_IMG]
    yl = eng.run_layer(l, xin, N_IMG).reshape(N_IMG, -1)             # layer-for-layer: whole panels
    assert eng.layer_split(l)[0] == -3
    worst = max(worst, tp.dense_check_rel(yl, *tp.dense_expected(kind, g, xin, p), tp.dec_dense_rel(kind, g), what=name))
    alone = eng.run_layer(l, xin[N_IMG - 3:], 3).reshape(3, -1)
    eng.close()
    return outs, yl, alone, worst, codes


@pytest.mark.parametrize("name", tp.DEC_FC_SHAPES)
def test_dense_sums_decoded_fc(name):
    outs, yl, alone, worst, codes = fc_case(name, 0)
    assert all(c == (-3, 1) for c in codes.values()), codes
    xin, y = outs[N_IMG]
    assert same_bits(yl, y) and same_bits(alone, y[N_IMG - 3:])
    for n, (xn, yn) in outs.items():
        assert same_bits(xn, xin[:n]), "%s: the layer's input differs between batches of %d and %d" % (name, n, N_IMG)
        assert same_bits(yn, y[:n]), "%s: %d images differ from the same images in the batch of %d: %d elements" % (
            name, n, N_IMG, int((yn != y[:n]).sum()))
    print("%s: codes %r worst err / bound %.3f" % (name, sorted(set(codes.values())), worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name", [n for n in tp.DEC_FC_SHAPES if tp.DEC_REACH[n][4] > 1])
def test_dense_sums_decoded_fc_k_slices(name):
    outs, yl, alone, worst, codes = fc_case(name, 1)
    assert codes[5][1] > 1 and codes[70][1] > 1, codes
    assert codes[5] == codes[70] == (-3, tp.DEC_REACH[name][4])
    print("%s: codes %r worst err / bound %.3f" % (name, codes, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------- shapes that must not decode ----
def test_more_than_128_code_words_do_not_decode_conv():
    worst = panel_case("nd_conv_k200", lambda code: code[0] != -3, tp.dec_dense_rel, seed=98)
    print("nd_conv_k200: worst err / bound %.3f" % worst)
    assert worst <= 1.0


def test_more_than_128_code_words_do_not_decode_fc():
    outs, yl, alone, worst, codes = fc_case_not_decoded("nd_fc_k130")
    print("nd_fc_k130: codes %r worst err / bound %.3f" % (sorted(set(codes.values())), worst))
    assert worst <= 1.0


def fc_case_not_decoded(name, seed=99):
    kind, g, M, K, Cs, _ = shape_of(name)
    _, inp = images(kind, g, N_IMG, seed + 1)
    eng, l, p = make(name, seed)
    outs, codes, worst = {}, {}, 0.0
    for n in tp.DEC_BATCHES:
        eng.forward_host(inp[:n])
        codes[n] = eng.layer_split(l)
        assert codes[n][0] != -3, "%s at %d images: family code %r" % (name, n, codes[n])
        xin, y = eng.layer_output(1, n).reshape(n, -1), eng.layer_output(2, n).reshape(n, -1)
        worst = max(worst, tp.dense_check_rel(y, *tp.dense_expected(kind, g, xin, p), tp.dec_dense_rel(kind, g), what="%s at %d images" % (name, n)))
        outs[n] = (xin, y)
    eng.close()
    return outs, None, None, worst, codes


# ---------------------------------------------------------------- window isolation ----
ISOLATION = ["dn_k5", "dn_k4_s5", "dn_k9", "dp_pad_k3", "dp_k7_ct32", "dp_1x1"]


def poisons(name, g, n):
    """[(what, bool mask [n, H, W, Cin])]: one element each, or all of image 1."""
    H, W, Cin = g["H"], g["W"], g["Cin"]
    out = []

    def one(what, *idx):
        m = np.zeros((n, H, W, Cin), bool)
        m[idx] = True
        out.append((what, m))
    one("the first pixel", 0, 0, 0, 0)
    one("the last pixel of the last image", n - 1, H - 1, W - 1, Cin - 1)
    Ho, Wo = tp.out_hw(g)                                            # the centre tap of the centre output's window
    one("a pixel in the middle of image 0", 0, Ho // 2 * g["stride"] - g["pad"] + g["knl"] // 2,
        Wo // 2 * g["stride"] - g["pad"] + g["knl"] // 2, Cin // 2)
    if name == "dn_k4_s5":
        one("column 14, which no window covers", 0, 2, 14, 0)
    one("all of image 1", 1)
    return out


@pytest.mark.parametrize("name", ISOLATION)
def test_window_isolation(name):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    paths = [("panel form", dict(), 1, False)]
    if name.startswith("dn_"):
        paths += [("in place, f32", dict(keep_all=0, bf16split=0), 2, True), ("in place, split-bf16", dict(keep_all=0, bf16split=1), 2, True)]
    for label, opts, out_layer, relu in paths:
        eng, l, p = make(name, 101, **opts)
        for n in (5, N_IMG):
            x, inp = images(kind, g, n, 102)
            eng.forward_host(inp)
            code = eng.layer_split(l)
            assert code == (-3, 2 if relu else 1), (name, label, code)
            clean = eng.layer_output(out_layer, n)
            assert np.isfinite(clean).all()
            for what, mask in poisons(name, g, n):
                hit = tp.window_hit(g, mask)
                eng.forward_host(np.where(mask, np.float32(np.nan), x).transpose(0, 3, 1, 2))
                assert eng.layer_split(l) == code
                y = eng.layer_output(out_layer, n)
                tag = "%s, %s, %d images, %s" % (name, label, n, what)
                assert same_bits(y[~hit], clean[~hit]), "%s: %d outputs outside every poisoned window changed" % (
                    tag, int((y[~hit].view(np.uint32) != clean[~hit].view(np.uint32)).sum()))
                if relu:
                    assert (np.isnan(y[hit]) | (y[hit] == 0)).all(), "%s: a poisoned window gave a finite non-zero output" % tag
                else:
                    assert np.isnan(y[hit]).all(), "%s: %d outputs of poisoned windows are not NaN" % (tag, int((~np.isnan(y[hit])).sum()))
                if "no window" in what:
                    assert not hit.any() and same_bits(y, clean)
                elif not (name == "dn_k4_s5" and what.startswith("the last pixel")):      # (row 8 is covered, column 14 is not)
                    assert hit.any()
        eng.close()
