"""Window isolation under NaN poison through every conv / FC table family (tests/isolation_cases.py; the CPU tier —
tests/test_isolation_cases_cpu.py — holds the `hit` rule to a float64 restatement, shows that every poison bites on both sides and
bounds the over-read of the new shapes below the buffers' slack).

The table kernels load their operands unconditionally and zero by a select what must not contribute: dims a sub-space does not
have, sub-spaces past the end of a stage, padding taps, clamped rows, the lanes of a ragged panel, dead slots and slices.  With
finite data 0 * x = 0 hides a missing select; with NaN it does not.  Per case and family, each forced by the option values of the
suite's family descriptors and required to report its own code (qcnn_get_layer_split) after EVERY launch:

  * poisoned run — one forward of 131 images (125 for the split forms) that carries one NaN element per image (every pixel of a
    small map, the channels at which a sub-space, a group and the map end), two all-NaN images on either side of the panel seam
    and clean images beside them: every output outside `hit` is bit-equal to the clean value, every output inside it is NaN.  The
    conv map is read before any ReLU (a ReLU turns NaN into 0);
  * stale run — one forward of 131 all-NaN images, then clean batches of 70, 5 and 3 images (125 for the split forms) on the same
    engine: NaN now fills the dead lanes, the untouched second panel, the staging buffer behind an in-place first layer, stale
    partial slabs and the few-image table scratch, and every live output must be finite and bit-equal to the clean value.

The clean value: on the integer data of tests/exact_cases.py the integer sum itself (a reference, not a kernel); elsewhere the same
engine's clean run, which is additionally held per element to the float64 sum of table_probe.dense_expected (bound as in
tests/test_gpu_panel_cases.py; fp16-rounded entries add 2^-11 of mag and 2^-25 per subnormal entry), so a wrong clean run cannot
vouch for itself.  The few-image kernels run three images: one clean, one with one poisoned element, one all NaN.  An FC output
depends on every input dim of its image, so FC cases have image and stale isolation only.  The ten base rows of
table_probe.TINY_SHAPES — maps of a few pixels, where nearly every tap is a clipping select — run the same poisoned and stale runs
through every family table_probe.TINY_REACH lists and through the few-image kernel."""
import numpy as np
import pytest

import exact_cases as ec
import isolation_cases as ic
import table_probe as tp
from conftest import pkg
from test_gpu_exact_sums import F16_APRX, fc_families
from test_gpu_table_probe import BASE, DEC_FC, EXACT, F16_CONV, OPT, SMALL, SMALL_PACKED, TILE, code_ok, fam
from test_panel_cases_cpu import FAMS, pseudo

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")

N = ic.BATCH
ORDER = ("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide", "split_tile", "split_sym8")
NAN = np.float32(np.nan)


def scrub(*arrays):
    """Zero host arrays that hold NaN before they are freed.  Later tests of the tier load the compiled reference into this process,
    and it scales an UNINITIALISED result buffer by beta = 0 before it accumulates (cblas_sgemm_nn: pc[in] *= beta): 0 * NaN is NaN,
    so non-finite garbage left in the heap could surface there as a wrong feature map."""
    for a in arrays:
        if a is not None:
            a.fill(0)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engine_for(opts):
    eng = pkg("engine").QcnnEngine(0)
    for k, v in dict(BASE, **opts).items():
        eng.set_option(OPT[k], v)
    return eng


def file_params(p):
    return {k: p[k] for k in ("bias", "ctrd", "asmt", "bits")}


def layer_params(name, seed):
    """Ordinary random parameters of the case's layer, whatever its D % Cs (synth.quant_spec refuses a ragged FC layer)."""
    kind, g, M, K, Cs = ic.shape_of(name)
    d = g["Cin"] // g["grp"] if kind == "conv" else g["D"]
    spec = {0: dict(kind=kind, M=M, K=K, Cs=Cs, Ct=g["Ct"], knl=g["knl"] if kind == "conv" else 1, D=d)}
    return synth.make_params(None, None, seed=seed, spec=spec)[0]


def model(kind, g, relu=True):
    """(in_chw, layers): the layer under test first — [conv, relu, fcnt(8), smax] (relu = False: no ReLU, so that a fast-path forward
    keeps the conv map), FC: [fcnt, smax] on a D x 1 x 1 input, which a forward feeds the crafted vector."""
    if kind == "conv":
        tail = [topo.relu()] if relu else []
        return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"])] + tail + [topo.fcnt(8), topo.smax()]
    return (g["D"], 1, 1), [topo.fcnt(g["Ct"]), topo.smax()]


def all_params(kind, g, p0, relu=True):
    in_chw, layers = model(kind, g, relu)
    if kind == "fc":
        return {0: file_params(p0)}
    allp = synth.make_params(in_chw, layers, seed=97)
    allp[0] = file_params(p0)
    return allp


def runner(eng, kind, via, out_layer=1):
    """x (NHWC / [n, D]) -> (output of layer 0 before any ReLU, the family code of that launch)."""
    def run(x):
        n = x.shape[0]
        if via == "layer":
            y = eng.run_layer(0, x, n)
        else:
            # a copy in either case: scrub() below zeroes it, and np.ascontiguousarray returns a VIEW of x for a 1 x 1 map (the
            # transposed axes have length 1), which would zero the caller's clean images
            inp = x.transpose(0, 3, 1, 2).copy() if kind == "conv" else x.reshape(n, -1, 1, 1).copy()
            prob, top5 = eng.forward_host(inp)
            scrub(inp, prob)
            y = eng.layer_output(out_layer, n)
        return (y if kind == "conv" else y.reshape(n, -1)), eng.layer_split(0)
    return run


def held(y, want64, mag, n_terms, entries=0, what=""):
    """The clean run against the float64 sum: gamma(n_terms) mag; with fp16-rounded entries (entries > 0) each entry is off by at most
    2^-11 of itself — 2^-25 where it is an fp16 subnormal — before the same float32 sum."""
    assert np.isfinite(y).all(), "%s: the clean run is not finite" % what
    bound = tp.gamma(n_terms) * mag
    if entries:
        bound = bound * (1.0 + 2.0 ** -11) + 2.0 ** -11 * mag + entries * 2.0 ** -25
    err = np.abs(y.astype(np.float64) - want64)
    assert (err <= bound).all(), "%s: %d clean outputs beyond the bound; worst err / bound %.3g" % (what, int((err > bound).sum()), float((err / bound).max()))
    return float((err / bound).max())


def poisoned_run(run, kind, g, M, Cs, x, clean, code, n, what):
    """One forward of n images with the plan's NaNs: un-hit outputs bit-equal to `clean`, hit outputs NaN, the clean run's code."""
    mask, p = ic.plan_mask(kind, g, M, Cs, n)
    h = ic.hit(kind, g, mask)
    xp = ic.poisoned(x[:n], mask)
    y, got = run(xp)
    scrub(xp)
    assert got == code, "%s, poisoned: family code %r, the clean run's was %r" % (what, got, code)
    assert y.shape == h.shape
    bad = bits(y)[~h] != bits(clean[:n])[~h]
    n_bad, n_bad_nan = int(bad.sum()), int(np.isnan(y)[~h].sum())
    first = tuple(np.argwhere((bits(y) != bits(clean[:n])) & ~h)[0]) if n_bad else None
    not_nan = int((~np.isnan(y)[h]).sum())
    scrub(y)
    assert not n_bad, "%s: %d of %d outputs outside every poisoned window changed (%d of the un-hit outputs NaN); first at %r" % (
        what, n_bad, bad.size, n_bad_nan, first)
    assert not not_nan, "%s: %d of %d outputs of poisoned windows are not NaN" % (what, not_nan, int(h.sum()))
    for i in p["clean"]:
        assert not h[i].any()
    return len(p["single"]), int(h.sum()), int((~h).sum())


def stale_run(run, x, clean, code_of, batches, what):
    """An all-NaN forward of 131 images, then clean batches: finite, bit-equal to the clean value, the family's own code."""
    xn = np.full_like(x[:N], NAN)
    y, _ = run(xn)
    finite = int((~np.isnan(y)).sum())
    scrub(xn, y)
    assert not finite, "%s: an all-NaN batch left %d finite outputs" % (what, finite)
    for n in batches:
        y, got = run(x[:n])
        assert code_of(got), "%s, %d clean images behind the NaN batch: family code %r" % (what, n, got)
        assert np.isfinite(y).all(), "%s: %d of %d outputs of %d clean images behind an all-NaN batch are not finite" % (
            what, int((~np.isfinite(y)).sum()), y.size, n)
        assert np.array_equal(bits(y), bits(clean[:n])), "%s: %d clean images behind an all-NaN batch differ in %d elements" % (
            what, n, int((bits(y) != bits(clean[:n])).sum()))


def family_case(name, f, kind, g, M, K, Cs, allp, x, exact_want, want64, mag, relu=True, out_layer=1, f16=False):
    """Clean, poisoned and stale run of one panel family on one engine.  exact_want: the integer sum (float32) or None — then the clean
    value is this engine's clean run, held to (want64, mag).  Returns the row of the result table."""
    in_chw, layers = model(kind, g, relu)
    eng = engine_for(f["opts"])
    eng.load_model(in_chw, layers, allp, N)
    run = runner(eng, kind, f["via"], out_layer)
    what = "%s / %s" % (name, f["label"])
    n = f["n"][0]
    y, code = run(x[:n])
    assert code_ok(f["code"], code), "%s, clean run of %d: family code %r, expected %r" % (what, n, code, f["code"])
    if exact_want is not None:
        assert np.array_equal(bits(y), bits(exact_want[:n])), "%s: the clean run differs from the integer sum in %d elements" % (
            what, int((bits(y) != bits(exact_want[:n])).sum()))
        clean = exact_want
    else:
        n_terms = tp.dense_count(kind, g, M, Cs)
        held(y, want64[:n], mag[:n], n_terms, entries=(g["knl"] ** 2 if kind == "conv" else 1) * M if f16 else 0, what=what)
        clean = y
    row = poisoned_run(run, kind, g, M, Cs, x, clean, code, n, what)
    split = n == ic.SPLIT_BATCH
    stale_run(run, x, clean, (lambda got: got == code) if split else (lambda got: code_ok(f["code"], got)),
              (ic.SPLIT_BATCH,) if split else ic.STALE_BATCHES, what)
    eng.close()
    print("%s: code %r, %d images, %d single poisons + %d NaN images: %d outputs NaN, %d bit-equal to the clean value; stale run clean"
          % (what, code, n, row[0], len(ic.plan(kind, g, M, Cs, n)["whole"]), row[1], row[2]))
    return row


# ---------------------------------------------------------------- conv, panel families ----
def conv_families(name):
    kind, g, M, K, Cs = ic.shape_of(name)
    if name in ic.IG:
        return [EXACT, TILE] + [FAMS[k] for k in ORDER if k in ic.IG_REACH[name]["live"]]
    if name in ic.TG:                                    # maps of a few pixels: every family table_probe.TINY_REACH lists
        return [EXACT, TILE] + [FAMS[k] for k in ORDER if k in tp.TINY_REACH[name]["live"]]
    if pseudo(K) > 1:                                    # K > 128: the exact-builder kernel under every option
        return [EXACT, dict(TILE, exact=True)]
    f16 = [] if name not in ec.CONV else F16_CONV if ec.EXACT_REACH[name] is not None else F16_APRX
    return [EXACT, TILE] + f16 + [FAMS[k] for k in ORDER if k in tp.PANEL_REACH[name]["live"]]


def conv_data(name, relu=True):
    """(kind, g, M, K, Cs, all parameters, x [131], integer sum or None, want64, mag)."""
    if name in ec.CONV:
        kind, g, M, K, Cs, params, x, e = ec.case(name)
        want_i, _ = ec.exact_expected(kind, g, x, params)
        return kind, g, M, K, Cs, all_params(kind, g, params, relu), x, ec.as_float32(want_i, e), None, None
    kind, g, M, K, Cs = ic.shape_of(name)
    p0 = layer_params(name, 87)
    x = tp.activations(kind, g, N, seed=88, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x, p0)
    return kind, g, M, K, Cs, all_params(kind, g, p0, relu), x, None, want64, mag


@pytest.mark.parametrize("name", sorted(tp.PANEL_REACH) + ic.IG + ic.TG)
def test_conv_panel_families(name):
    kind, g, M, K, Cs, allp, x, exact_want, want64, mag = conv_data(name)
    for f in conv_families(name):
        family_case(name, f, kind, g, M, K, Cs, allp, x, exact_want, want64, mag, f16=f["f16"] or f in F16_APRX)


@pytest.mark.parametrize("name", ["rgb7"])
def test_first_layer_read_in_place_by_the_table_kernel(name):
    """QCNN_OPT_DECODE = 0, fast path: k_conv_aprx reads the NCHW batch where the upload left it (one 3-dim sub-space; the dims it
    does not have are the NEXT image's channel planes, for the last image the staging buffer's slack).  No ReLU behind the layer:
    the conv map stays."""
    kind, g, M, K, Cs, allp, x, _, want64, mag = conv_data(name, relu=False)
    for f in (fam("in place, exact builder", (-1, 1), via="forward", lut=capi.LUT_EXACT, keep_all=0),
              fam("in place, MFMA builder", (-1, 1), via="forward", keep_all=0)):
        family_case(name, f, kind, g, M, K, Cs, allp, x, None, want64, mag, relu=False)


# ---------------------------------------------------------------- few-image kernels ----
def few_case(name, f, kind, g, M, K, Cs, allp, x, want64, mag):
    """Three images — clean, one poisoned element, all NaN — per entry of the short list; then three clean images behind an all-NaN
    forward of 131 (the panel kernels' maps and the few-image table scratch full of NaN)."""
    in_chw, layers = model(kind, g)
    eng = engine_for(f["opts"])
    eng.load_model(in_chw, layers, allp, N)
    run = runner(eng, kind, "forward")
    what = "%s / %s" % (name, f["label"])
    clean, code = run(x[:3])
    assert code == f["code"], "%s: family code %r" % (what, code)
    held(clean, want64[:3], mag[:3], tp.dense_count(kind, g, M, Cs), what=what)
    rows = []
    for label, e in ic.few_plans(kind, g, M, Cs):
        mask = ic.mask_of(kind, g, 3, [(1,) + e], whole=[2])
        h = ic.hit(kind, g, mask)
        xp = ic.poisoned(x[:3], mask)
        y, got = run(xp)
        tag = "%s, %s" % (what, label)
        n_bad, not_nan = int((bits(y)[~h] != bits(clean)[~h]).sum()), int((~np.isnan(y)[h]).sum())
        scrub(xp, y)
        assert got == code, "%s: family code %r" % (tag, got)
        assert not n_bad, "%s: %d of %d outputs outside every poisoned window changed" % (tag, n_bad, int((~h).sum()))
        assert not not_nan, "%s: %d outputs of poisoned windows are not NaN" % (tag, not_nan)
        assert not h[0].any() and h[2].all()
        rows.append((int(h[1].sum()), int((~h[1]).sum())))
    xn = np.full_like(x[:N], NAN)
    y, got = run(xn)
    finite = int((~np.isnan(y)).sum())
    scrub(xn, y)
    assert got[0] != -11 and not finite
    y, got = run(x[:3])
    assert got == code, "%s, behind the NaN batch: family code %r" % (what, got)
    assert np.array_equal(bits(y), bits(clean)), "%s: three clean images behind an all-NaN batch differ in %d elements (%d not finite)" % (
        what, int((bits(y) != bits(clean)).sum()), int((~np.isfinite(y)).sum()))
    eng.close()
    print("%s: code %r, %d poisons, (hit, un-hit) outputs of image 1: %r; stale run clean" % (what, code, len(rows), rows))


@pytest.mark.parametrize("name", sorted(n for n in tp.SMALL_REACH if tp.SHAPES[n][0] == "conv") + ic.IG + ic.TG)
def test_few_image_conv(name):
    kind, g, M, K, Cs = ic.shape_of(name)
    p0 = layer_params(name, 71)
    x = tp.activations(kind, g, N, seed=72, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x[:3], p0)
    few_case(name, SMALL, kind, g, M, K, Cs, all_params(kind, g, p0), x, want64, mag)


@pytest.mark.parametrize("name", sorted(n for n in tp.SMALL_REACH if tp.SHAPES[n][0] == "fc") + ["fr_small", "fr_k32"])
def test_few_image_fc(name):
    kind, g, M, K, Cs = ic.shape_of(name)
    p0 = layer_params(name, 73)
    x = tp.activations(kind, g, N, seed=74, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x[:3], p0)
    for f in (SMALL, SMALL_PACKED):                      # on bytes, and on the packed stream read in place
        few_case(name, f, kind, g, M, K, Cs, {0: file_params(p0)}, x, want64, mag)


# ---------------------------------------------------------------- FC, panel families ----
@pytest.mark.parametrize("name", sorted(ec.FC))
def test_fc_panel_families_on_integer_data(name):
    kind, g, M, K, Cs, params, x, e = ec.case(name)
    want_i, _ = ec.exact_expected(kind, g, x, params)
    want = ec.as_float32(want_i, e)
    for f, _ in fc_families(name):
        family_case(name, f, kind, g, M, K, Cs, {0: file_params(params)}, x, want, None, None)


def ragged_fc_families(name):
    r = ic.FR_REACH[name]
    zp, zs = r["plain"][1], r["split"][1]
    return [fam("exact builder, k_fc_aprx, one slice", (-1, 1), lut=capi.LUT_EXACT),
            fam("k_fc_aprx, %d slices" % zp, (-1, 1), lut=capi.LUT_MFMA),
            fam("k_fc_aprx, %d slices, QCNN_OPT_SYM8 = 2 (k_fc_sym8 refuses D != 4 M)" % zp, (-1, 1), lut=capi.LUT_MFMA, sym8=2),
            fam("k_fc_aprx, fp16-rounded entries, %d slices" % zp, (-1, 1), f16=True, lut=capi.LUT_MFMA_F16, sym8=2),
            fam("k_fc_aprx, per-launch %d slices" % zs, (-1, 1), n=(ic.SPLIT_BATCH,), lut=capi.LUT_MFMA, split=1),
            fam("k_fc_aprx, fp16-rounded entries, per-launch %d slices" % zs, (-1, 1), n=(ic.SPLIT_BATCH,), f16=True, lut=capi.LUT_MFMA_F16, split=1)]


@pytest.mark.parametrize("name", ic.FR)
def test_fc_panel_families_on_a_ragged_last_sub_space(name):
    kind, g, M, K, Cs = ic.shape_of(name)
    p0 = layer_params(name, 75)
    x = tp.activations(kind, g, N, seed=76, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x, p0)
    for f in ragged_fc_families(name):
        family_case(name, f, kind, g, M, K, Cs, {0: file_params(p0)}, x, None, want64, mag, f16=f["f16"])


@pytest.mark.parametrize("name", tp.DEC_FC_SHAPES)
def test_decoded_fc(name):
    """k_fc_dec (one-dim sub-spaces through their decoded code words): image and stale isolation."""
    kind, g, M, K, Cs = ic.shape_of(name)
    p0 = layer_params(name, 77)
    x = tp.activations(kind, g, N, seed=78, scaled=False)
    want64, mag = tp.dense_expected(kind, g, x, p0)
    in_chw, layers = model(kind, g)
    eng = engine_for(DEC_FC["opts"])
    eng.load_model(in_chw, layers, {0: file_params(p0)}, N)
    run = runner(eng, kind, "layer")
    clean, code = run(x)
    assert code == (-3, 1), "%s: family code %r" % (name, code)
    tp.dense_check_rel(clean, want64, mag, tp.dec_dense_rel(kind, g), what=name)
    row = poisoned_run(run, kind, g, M, Cs, x, clean, code, N, name)
    stale_run(run, x, clean, lambda got: got == code, ic.STALE_BATCHES, name)
    eng.close()
    print("%s: decoded FC code %r, %d single poisons: %d outputs NaN, %d bit-equal; stale run clean" % ((name, code) + row))


# ---------------------------------------------------------------- the precise path ----
@pytest.mark.parametrize("name", ["ig_grp2_cs4_k32", "fr_k64"])
def test_dense_kernel(name):
    """k_dense, the yardstick of the response report, on one conv geometry (two groups of 14 input channels: a k-step of two live
    dims; stride 1, where the reference's im2col drops no tap) and one FC geometry (D = 474).  It reports no family code.  The clean
    run is held to the float64 sum within gamma(inputs + 1) mag: one fused multiply-add per input, any order."""
    kind, g, _, _, _ = ic.shape_of(name)
    in_chw, layers = model(kind, g)
    dense = synth.make_dense_params(in_chw, layers, seed=79)
    eng = engine_for({})
    eng.load_dense_model(in_chw, layers, dense, N)
    run = runner(eng, kind, "layer")
    x = tp.activations(kind, g, N, seed=80, scaled=False)
    want64, mag = ic.dense_layer64(kind, g, x, dense[0]["bias"], dense[0]["weights"])
    clean, code = run(x)
    inputs = g["knl"] ** 2 * g["Cin"] // g["grp"] if kind == "conv" else g["D"]
    worst = held(clean, want64, mag, inputs + 1, what=name)
    row = poisoned_run(run, kind, g, 1, inputs if kind == "fc" else g["Cin"] // g["grp"], x, clean, code, N, name + " / k_dense")
    stale_run(run, x, clean, lambda got: got == code, ic.STALE_BATCHES, name + " / k_dense")
    eng.close()
    print("%s: k_dense clean worst err / bound %.3f, %d single poisons: %d outputs NaN, %d bit-equal; stale run clean" % ((name, worst) + row))
