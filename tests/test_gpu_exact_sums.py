"""Exact sums through the fp16 table kernels and the FC panel kernels (qcnn_sym8.hip: k_conv_sym8<.., MODE = 1 | 2>, k_fc_sym8<0 | 1 |
2>; qcnn_kernels.hip: k_conv_aprx and k_fc_aprx with lutF16, k_fc_aprx with a split sub-space axis; qcnn_glue.hip: k_sum_partials).

The data of tests/exact_cases.py makes every product, table entry and partial sum an integer multiple of one power of two, small
enough to be exact as an f32 MFMA entry, as an fp16 entry, in a v_pk_add_f16 sum, in an f32 sum and in the f32 reduction of
slices (tests/test_exact_cases_cpu.py asserts the conditions on this very batch and ties the expected sums to the oracle).  So
every summation order, tile, stage grouping and slice count must return the same number, and EVERY assertion here is
np.array_equal against the integer sum cast to float32 — no bound.  One look-up lost or doubled at a clipped tile, a stage-ring
wrap, a channel chunk or a slice seam, a wrong slot, image half or stage buffer, a bias added twice or never moves an element by
a whole unit.  (Whether a mode rounds cannot show on exact values: the probes of test_gpu_table_probe.py hold the entries rounded
once, test_gpu_parity.py the AlexNet bounds.)

Every launch must report its own family code (qcnn_get_layer_split); exact_cases.EXACT_REACH says which instantiation, tile and slice
counts each case reaches, re-derived on the CPU tier.  Conv: the exact builder, the f32 tile kernel, fp16 tables (-7) and fp16
tables + sums (-8) at 131 images, the ragged panel's three images alone, the forward's conv map; then the other f32 families the
shape has, on the same data.  FC: the layer is the first one of [fcnt, smax] on a D x 1 x 1 input, so that a forward feeds it the
crafted input too."""
import numpy as np
import pytest

import exact_cases as ec
import table_probe as tp
from conftest import pkg
from test_gpu_table_probe import BASE, EXACT, F16_CONV, OPT, TILE, code_ok, fam
from test_panel_cases_cpu import FAMS

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")

N = ec.BATCH
OTHER_F32 = ("slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide", "split_tile", "split_sym8")
F16_APRX = [fam("fp16-rounded entries, 16-wave tile", (-1, 1), lut=capi.LUT_MFMA_F16, sym8=2),          # no eight-wave form: k_conv_aprx
            fam("fp16-rounded entries, 16-wave tile (mode 3)", (-1, 1), lut=capi.LUT_MFMA_F16ACC, sym8=2)]   # with lutF16, f32 sums


def make_engine(in_chw, layers, params, opts):
    eng = pkg("engine").QcnnEngine(0)
    for k, v in dict(BASE, **opts).items():
        eng.set_option(OPT[k], v)
    eng.load_model(in_chw, layers, params, N)
    return eng


def file_params(p):
    return {k: p[k] for k in ("bias", "ctrd", "asmt", "bits")}


def equal(y, want, what):
    y = np.asarray(y).reshape(want.shape)
    bad = y != want
    assert not bad.any(), "%s: %d of %d elements are not the integer sum; first at %r: got %r, want %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), float(y[bad][0]), float(want[bad][0]))


def run_family(eng, l, f, x, inp, want, what, full):
    """One family on the case's data: its batches through run_layer; with `full` also the ragged panel's three images alone and the
    forward of the first batch.  Returns the codes seen."""
    seen = []
    for n in f["n"]:
        y = eng.run_layer(l, x[:n], n)
        got = eng.layer_split(l)
        seen.append(got)
        assert code_ok(f["code"], got), "%s / %d images: family code %r, expected %r" % (what, n, got, f["code"])
        equal(y, want[:n], "%s / %d images" % (what, n))
        if full and n == N:
            alone = eng.run_layer(l, x[N - 3:], 3)
            assert code_ok(f["code"], eng.layer_split(l)), "%s: the last three images alone ran %r" % (what, eng.layer_split(l))
            equal(alone, want[N - 3:], "%s / the last three images alone" % what)
        if full and n == f["n"][0]:
            eng.forward_host(inp[:n])
            got = eng.layer_split(l)
            assert code_ok(f["code"], got), "%s, forward of %d: family code %r, expected %r" % (what, n, got, f["code"])
            equal(eng.layer_output(l + 1, n), want[:n], "%s / forward of %d images" % (what, n))
    return seen


@pytest.mark.parametrize("name", sorted(ec.CONV))
def test_conv_exact_sums(name):
    kind, g, M, K, Cs, params, x, e = ec.case(name)
    want_i, s_abs = ec.exact_expected(kind, g, x, params)
    assert s_abs.max() <= ec.F16_UNITS
    want = ec.as_float32(want_i, e)
    in_chw = (g["Cin"], g["H"], g["W"])
    layers = [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"]), topo.relu(), topo.fcnt(8), topo.smax()]
    spec = pkg("synth").quant_spec(in_chw, layers)
    spec[0] = dict(spec[0], M=M, K=K, Cs=Cs)
    allp = pkg("synth").make_params(in_chw, layers, seed=93, spec=spec)
    allp[0] = file_params(params)
    inp = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    reach = ec.EXACT_REACH[name]
    first = [EXACT, TILE] + (F16_CONV if reach is not None else F16_APRX)
    others = [FAMS[k] for k in OTHER_F32 if k in tp.PANEL_REACH[name]["live"]]
    for f, full in [(f, True) for f in first] + [(dict(f, n=f["n"][:1]), False) for f in others]:
        eng = make_engine(in_chw, layers, allp, f["opts"])
        seen = run_family(eng, 0, f, x, inp, want, "%s / %s" % (name, f["label"]), full)
        eng.close()
        print("%s: %s ran %r on %r images: bit-equal to the integer sum (unit 2^%d)" % (name, f["label"], seen, f["n"], e))
    if reach is not None:
        print("%s: k_conv_sym8 MODE 1 <cpw, th, tw, chunks> = %r, MODE 2 = %r" % (name, reach["mode1"], reach["mode2"]))


def fc_families(name):
    """[(family descriptor, run the three images alone and the forward too)] of an FC case: slice counts from EXACT_REACH."""
    r = ec.EXACT_REACH[name]
    if name in ec.FX:
        zp, zs = r["plain"][1], r["split"][1]
        modes = ((capi.LUT_MFMA, -5, "k_fc_sym8<0>"), (capi.LUT_MFMA_F16, -7, "k_fc_sym8<1>"), (capi.LUT_MFMA_F16ACC, -8, "k_fc_sym8<2>"))
        out = [(fam("exact builder, k_fc_aprx", (-1, 1), lut=capi.LUT_EXACT), True)]
        out += [(fam("%s, %d slices" % (lab, zp), (code, zp), lut=lut, sym8=2), True) for lut, code, lab in modes]
        # QCNN_OPT_SPLIT: the slice count of THIS launch — one panel of 125 images
        out += [(fam("%s, per-launch %d slices" % (lab, zs), (code, zs), n=(ec.SPLIT_BATCH,), lut=lut, sym8=2, split=1), True)
                for lut, code, lab in modes]
        return out
    # k_fc_aprx reports (-1, 1) whatever its slice count (the planner's: tests/test_exact_cases_cpu.py::test_fc_reach)
    zp, zs = r["plain"][1], r["split"][1]
    return [(fam("exact builder, k_fc_aprx, one slice", (-1, 1), lut=capi.LUT_EXACT), True),
            (fam("k_fc_aprx, %d slices" % zp, (-1, 1), lut=capi.LUT_MFMA), True),
            (fam("k_fc_aprx, fp16-rounded entries, %d slices" % zp, (-1, 1), lut=capi.LUT_MFMA_F16), True),
            (fam("k_fc_aprx, fp16-rounded entries (mode 3), %d slices" % zp, (-1, 1), lut=capi.LUT_MFMA_F16ACC), False),
            (fam("k_fc_aprx, per-launch %d slices" % zs, (-1, 1), n=(ec.SPLIT_BATCH,), lut=capi.LUT_MFMA, split=1), True),
            (fam("k_fc_aprx, fp16-rounded entries, per-launch %d slices" % zs, (-1, 1), n=(ec.SPLIT_BATCH,), lut=capi.LUT_MFMA_F16, split=1), False)]


@pytest.mark.parametrize("name", sorted(ec.FC))
def test_fc_exact_sums(name):
    kind, g, M, K, Cs, params, x, e = ec.case(name)
    want_i, s_abs = ec.exact_expected(kind, g, x, params)
    assert s_abs.max() <= (ec.F16_UNITS if name in ec.FX else ec.F32_UNITS)
    want = ec.as_float32(want_i, e)
    in_chw, layers = (g["D"], 1, 1), [topo.fcnt(g["Ct"]), topo.smax()]
    inp = x.reshape(N, g["D"], 1, 1)
    for f, full in fc_families(name):
        eng = make_engine(in_chw, layers, {0: file_params(params)}, f["opts"])
        seen = run_family(eng, 0, f, x, inp, want, "%s / %s" % (name, f["label"]), full)
        eng.close()
        print("%s: %s ran %r on %r images: bit-equal to the integer sum (unit 2^%d)" % (name, f["label"], seen, f["n"], e))
