"""QCNN_OPT_DEC_BF16SPLIT = 2 (default): the decoded first layer read in place with two fp16 pieces per operand and three
cross terms (k_conv_dec_nchw_f16), its range guard and its scale rule.  Per output element against the float64 dense sum
within f16split_model.output_bound, against the f32 path (option 0) within 2e-6 of the pool map's largest value, against
the oracle within 1e-4; the same batch-size and permutation invariance as every fast-path kernel; inputs outside the
form's range get option 1's bits for the images that hold them and leave every other image alone."""
import numpy as np
import pytest

import f16split_model as fm
import pyoracle as po
import table_probe as tp
from conftest import pkg, rel_err

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")
TOL = 1e-4
IN_HW = (29, 31)
# (cin, knl, stride, ct): flat order with knl < 4; smallest run order (one run per row); AlexNet's (last run overlapping); three
# full runs; flat order because the run order does not fit LDS; two channel chunks
SHAPES = [(1, 3, 1, 96), (3, 4, 2, 96), (3, 11, 4, 96), (2, 12, 5, 96), (4, 9, 1, 96), (4, 4, 2, 192)]
# one partly live image tile; either side of the image-tile seam; a ragged panel; two panels
BATCHES = (130, 70, 17, 16, 5)


def engine(in_chw, layers, params, max_batch, split, opts=()):
    eng = pkg("engine").QcnnEngine(0)
    eng.set_option(capi.OPT_LUT_MODE, capi.LUT_MFMA)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.set_option(capi.OPT_DEC_BF16SPLIT, split)
    for k, v in opts:
        eng.set_option(k, v)
    eng.load_model(in_chw, layers, params, max_batch)
    return eng


def model(cin, knl, stride, ct, seed=None):
    layers = [topo.conv(0, knl, ct, 1, stride), topo.relu(), topo.pool(0, 2, 2), topo.fcnt(40), topo.smax()]
    in_chw = (cin,) + IN_HW
    return in_chw, layers, synth.make_params(in_chw, layers, seed=290 + cin if seed is None else seed)


def pixels(n, in_chw, seed=291):
    return np.random.default_rng(seed).integers(0, 256, size=(n,) + in_chw).astype(np.float32) - 120.0


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def geom(cin, knl, stride, ct):
    return tp.conv_geom(IN_HW[0], IN_HW[1], cin, knl, stride, 0, 1, ct)


def reference(imgs, p, shape, eta=fm.ETA):
    """(float64 dense sums behind the fused ReLU, per-element bound) of the conv map [n, Ho, Wo, Ct], computed once per batch."""
    cin, knl, stride, ct = shape
    x = imgs.transpose(0, 2, 3, 1)
    want, mag = tp.dense_expected_one_subspace(geom(*shape), x, p)
    abs_bias = np.abs(p["bias"].astype(np.float64))
    sw_abs, sx_abs = fm.abs_sums(x, p, knl, stride, cin)
    bound = fm.output_bound(mag - abs_bias, sw_abs, sx_abs[..., None], abs_bias, fm.padded_k(cin, knl, ct), fm.layer_scale(p, cin), eta)
    return np.maximum(want, 0.0), bound


def check_elements(y, ref, what):
    """The fused conv + ReLU map y of the first len(y) images against `reference`; returns the worst err / bound."""
    want, bound = ref
    assert np.isfinite(y).all(), what
    ratio = np.abs(y.astype(np.float64) - want[:len(y)]) / bound[:len(y)]
    assert ratio.max() <= 1.0, "%s: %d outputs beyond the bound, worst err / bound %.3g" % (what, int((ratio > 1).sum()), ratio.max())
    return float(ratio.max())


@pytest.mark.parametrize("cin,knl,stride,ct", SHAPES)
def test_f16_against_f32_path_dense_sums_and_oracle(cin, knl, stride, ct):
    import torch
    shape = (cin, knl, stride, ct)
    in_chw, layers, params = model(*shape)
    imgs = pixels(BATCHES[0], in_chw)
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    assert fm.layer_scale(params[0], cin) > 0
    ref = reference(imgs, params[0], shape)
    e0, e2 = engine(in_chw, layers, params, BATCHES[0], 0), engine(in_chw, layers, params, BATCHES[0], 2)
    worst_dev = worst_el = 0.0
    for n in BATCHES:
        e0.forward_host(imgs[:n])
        prob, _ = e2.forward_host(imgs[:n])
        assert e0.layer_split(0) == (-3, 2) and e0.layer_dec_form(0) == (0, 0)
        assert e2.layer_split(0) == (-3, 2) and e2.layer_dec_form(0) == (2, 0), e2.layer_dec_form(0)
        m0, m2 = e0.layer_output(3, n), e2.layer_output(3, n)
        dev = float(np.abs(m2 - m0).max() / np.abs(m0).max())
        worst_dev = max(worst_dev, dev)
        assert dev <= 2e-6, "n = %d: %g of the pool map's largest value" % (n, dev)
        worst_el = max(worst_el, check_elements(e2.layer_output(2, n), ref, "n = %d" % n))
        x = torch.from_numpy(imgs[:n]).to("cuda:0")
        prob_d = torch.empty((n, 40), dtype=torch.float32, device="cuda:0")
        e2.forward_dev(x.data_ptr(), n, prob_d.data_ptr())
        e2.sync()
        assert np.array_equal(bits(prob_d.cpu().numpy()), bits(prob))
        assert e2.layer_dec_form(0) == (2, 0)
        m = min(n, 3)
        orc.forward(imgs[n - m:n])
        for l in (3, 4, 5):
            e_inf, e_l2 = rel_err(e2.layer_output_range(l, n - m, m), orc.fm(l))
            assert e_inf <= TOL and e_l2 <= TOL, "n = %d fm[%d] vs oracle: %g %g" % (n, l, e_inf, e_l2)
    e0.close()
    e2.close()
    print("fp16 pieces, cin %d knl %d stride %d ct %d: vs f32 path %.3g of the pool map's largest value, worst err / bound %.3g"
          % (cin, knl, stride, ct, worst_dev, worst_el))


def test_invariance_and_live_option():
    """A 64-image slice and a permuted batch reproduce the full batch's bits; option 2 differs from option 1 somewhere."""
    shape = (3, 11, 4, 96)
    in_chw, layers, params = model(*shape)
    imgs = pixels(130, in_chw)
    e2 = engine(in_chw, layers, params, 130, 2)
    prob, top5 = e2.forward_host(imgs)
    y = e2.layer_output(2, 130)
    p64, t64 = e2.forward_host(imgs[66:130])
    assert np.array_equal(bits(p64), bits(prob[66:130])) and np.array_equal(t64, top5[66:130])
    assert np.array_equal(bits(e2.layer_output(2, 64)), bits(y[66:130]))
    perm = np.random.default_rng(3).permutation(130)
    pp, tq = e2.forward_host(imgs[perm])
    assert np.array_equal(bits(pp), bits(prob[perm])) and np.array_equal(tq, top5[perm])
    assert np.array_equal(bits(e2.layer_output(2, 130)), bits(y[perm]))
    e2.close()
    e1 = engine(in_chw, layers, params, 130, 1)
    e1.forward_host(imgs)
    assert e1.layer_dec_form(0) == (1, 0)
    y1 = e1.layer_output(2, 130)
    e1.close()
    assert not np.array_equal(bits(y1), bits(y)), "QCNN_OPT_DEC_BF16SPLIT = 2 changes nothing: a dead option value"
    assert np.abs(y1 - y).max() <= 2e-6 * np.abs(y1).max()


def expected_pairs(hit_img, ct):
    """(work item, image) pairs the guard must flag for ONE image whose outputs hit_img [Ho, Wo] hold the value: an item is four
    consecutive positions of an output row x 96 channels."""
    Ho, Wo = hit_img.shape
    groups = sum(int(hit_img[r, c:c + 4].any()) for r in range(Ho) for c in range(0, Wo, 4))
    return groups * (ct // 96)


@pytest.mark.parametrize("cin,knl,stride,ct", [(3, 11, 4, 96), (4, 4, 2, 192), (1, 3, 1, 96)])
def test_range_guard(cin, knl, stride, ct):
    """One pixel of one image of a 40-image batch outside the form's range.  A: the clean batch, option 2; B: the poisoned batch,
    option 2; C: the poisoned batch, option 1."""
    shape = (cin, knl, stride, ct)
    in_chw, layers, params = model(*shape)
    clean = pixels(40, in_chw)
    img, at = 21, (cin - 1, 13, 14)
    e2, e1 = engine(in_chw, layers, params, 40, 2), engine(in_chw, layers, params, 40, 1)
    e2.forward_host(clean)
    assert e2.layer_dec_form(0) == (2, 0)
    a = e2.layer_output(2, 40)
    others = np.arange(40) != img
    for value in (2 * fm.XMAX, 1e30, np.inf, np.nan, fm.XMAX):
        bad = clean.copy()
        bad[(img,) + at] = value
        e2.forward_host(bad)
        form, pairs = e2.layer_dec_form(0)
        b = e2.layer_output(2, 40)
        assert form == 2
        assert np.array_equal(bits(b[others]), bits(a[others])), "value %r: another image's outputs changed" % value
        if value == fm.XMAX:
            assert pairs == 0
            check_elements(b, reference(bad, params[0], shape), "pixel at X_MAX")
            continue
        e1.forward_host(bad)
        c = e1.layer_output(2, 40)
        poison = np.zeros((40,) + IN_HW + (cin,), bool)
        poison[img, at[1], at[2], at[0]] = True
        hit = tp.window_hit(geom(*shape), poison)
        assert hit[img].any() and not hit[others].any()
        assert ((bits(b) == bits(a)) | (bits(b) == bits(c))).all(), "value %r: an output that is neither A's nor C's" % value
        assert np.array_equal(bits(b[hit]), bits(c[hit])), "value %r: a window with the value does not carry option 1's bits" % value
        assert pairs == expected_pairs(hit[img], ct), (value, pairs, expected_pairs(hit[img], ct))
        e2.forward_host(clean)                                          # the guard leaves nothing behind
        assert e2.layer_dec_form(0) == (2, 0)
        assert np.array_equal(bits(e2.layer_output(2, 40)), bits(a))
    e2.close()
    e1.close()


def scaled(p, f):
    return dict(p, bias=(p["bias"] * np.float32(f)).astype(np.float32), ctrd=(p["ctrd"] * np.float32(f)).astype(np.float32))


def test_scales():
    """Code books and bias scaled by 2^-20 and 2^20: the form the scale rule says, within the bound; all-zero code words: form 1
    and option 1's bits."""
    shape = (3, 11, 4, 96)
    cin = shape[0]
    in_chw, layers, params = model(*shape)
    imgs = pixels(20, in_chw)
    e2 = engine(in_chw, layers, params, 20, 2)
    for f in (2.0 ** -20, 2.0 ** 20):
        p = scaled(params[0], f)
        e2.upload({0: p})
        e2.forward_host(imgs)
        want_form = 2 if fm.layer_scale(p, cin) > 0 else 1
        assert e2.layer_dec_form(0) == (want_form, 0)
        if want_form == 2:
            r = check_elements(e2.layer_output(2, 20), reference(imgs, p, shape), "code book x %g" % f)
            print("code book x 2^%d: form 2, worst err / bound %.3g" % (int(np.log2(f)), r))
    zero = dict(params[0], ctrd=np.zeros_like(params[0]["ctrd"]))
    assert fm.layer_scale(zero, cin) == 0.0
    e2.upload({0: zero})
    e2.forward_host(imgs)
    assert e2.layer_dec_form(0) == (1, 0)
    y2 = e2.layer_output(2, 20)
    e2.close()
    e1 = engine(in_chw, layers, {**params, 0: zero}, 20, 1)
    e1.forward_host(imgs)
    assert np.array_equal(bits(e1.layer_output(2, 20)), bits(y2))
    e1.close()


def test_tiny_inputs():
    """Pieces in fp16's subnormal range: activations of magnitude 1e-3 ... 1e-6 with code words near their maximum, and
    ordinary activations with code words 1e-3 ... 1e-6 of the layer's largest.  The bound holds with f16split_model.ETA —
    2^-25, the matrix instruction keeps subnormal fp16 inputs; flushed inputs would need 2^-14 and miss it by orders of magnitude."""
    shape = (3, 11, 4, 96)
    cin = shape[0]
    in_chw, layers, params = model(*shape)
    rng = np.random.default_rng(77)
    e2 = engine(in_chw, layers, params, 20, 2)
    p = params[0]
    top = np.abs(p["ctrd"]).max()
    near_max = dict(p, ctrd=(np.sign(p["ctrd"]) * top * rng.uniform(0.5, 1.0, p["ctrd"].shape)).astype(np.float32))
    tiny_x = (10.0 ** rng.uniform(-6, -3, (20,) + in_chw) * rng.choice([-1.0, 1.0], (20,) + in_chw)).astype(np.float32)
    small = p["ctrd"] / top * 10.0 ** rng.uniform(-6, -3, p["ctrd"].shape) * top
    small[0, 0, :] = top                                                # one code word sets the scale (every channel names code word 0 somewhere)
    tiny_w = dict(p, ctrd=small.astype(np.float32), asmt=p["asmt"].copy())
    tiny_w["asmt"][:, 0, 0, 0] = 0
    # what settles the subnormal question: every Sx x = h (1 + 2^-12) with h an fp16 number in [2^-6, 2^-3), so every second piece
    # is +h 2^-12, a subnormal fp16 number, and every code word is positive: flushed second pieces would leave every output short
    # by 2^-12 of its sum, four times this bound
    h = rng.uniform(2.0 ** -6, 2.0 ** -3, (20,) + in_chw).astype(np.float16).astype(np.float64)
    coherent_x = (h * (1 + 2.0 ** -12) / fm.SX).astype(np.float32)
    positive = dict(p, ctrd=np.abs(near_max["ctrd"]))
    assert np.array_equal(coherent_x.astype(np.float64) * fm.SX, h * (1 + 2.0 ** -12))
    for what, pp, x in (("tiny activations", near_max, tiny_x), ("tiny code words", tiny_w, pixels(20, in_chw)),
                        ("subnormal second pieces of one sign", positive, coherent_x)):
        e2.upload({0: pp})
        e2.forward_host(x)
        assert e2.layer_dec_form(0) == (2, 0)
        y = e2.layer_output(2, 20)
        r = check_elements(y, reference(x, pp, shape), what)
        flushed = check_elements(y, reference(x, pp, shape, eta=2.0 ** -14), what)
        print("%s: worst err / bound %.3g with eta = 2^-25 (%.3g with 2^-14)" % (what, r, flushed))
    e2.close()


def test_alexnet_200_defaults():
    """AlexNet at 200 images with the option at its default: form 2, no fallback, the oracle within 1e-4 on sampled images,
    option 1's top-5 except between scores within 1e-6 of each other."""
    in_chw, layers, _, _ = topo.MODELS["AlexNet"]
    params = synth.make_params(in_chw, layers, seed=7)
    imgs = synth.make_images(200, in_chw, seed=10)
    eng = pkg("engine").QcnnEngine(0)
    eng.set_option(capi.OPT_LUT_MODE, capi.LUT_MFMA)
    eng.set_option(capi.OPT_KEEP_ALL, 0)
    eng.load_model(in_chw, layers, params, 200)
    prob, top5 = eng.forward_host(imgs)
    assert eng.layer_split(0) == (-3, 2) and eng.layer_dec_form(0) == (2, 0), eng.layer_dec_form(0)
    eng.close()
    e1 = engine(in_chw, layers, params, 200, 1)
    p1, t1 = e1.forward_host(imgs)
    assert e1.layer_dec_form(0) == (1, 0)
    e1.close()
    for r in np.nonzero((top5 != t1).any(axis=1))[0]:
        s = np.sort(p1[r])[::-1][:6]
        assert np.abs(np.diff(s)).min() <= 1e-6, r
    orc = po.COracle(in_chw, layers)
    orc.set_params(params)
    pick = [0, 63, 64, 199]
    orc.forward(imgs[pick])
    e_inf, e_l2 = rel_err(prob[pick], orc.fm(len(layers)).reshape(len(pick), -1))
    assert e_inf <= TOL and e_l2 <= TOL, (e_inf, e_l2)
