"""Dense sums through every panel conv family (qcnn_kernels.hip: k_conv_aprx tile and sliding form, k_conv_sym; qcnn_sym8.hip:
k_conv_sym8 tile and sliding form; qcnn_half8.hip: k_conv_half8 tile and sliding form; split tiles + k_conv_sum) on the shapes at
which their deep sub-space axis, channel configurations, stage groups, tile edges, stage rings and slice seams are live
(table_probe.PANEL_REACH; tests/test_panel_cases_cpu.py pins the planner's and the launchers' choice per shape, shows that the
references alone meet the bound used here and that one missing or doubled term does not).

A probe output (tests/test_gpu_table_probe.py) is one table entry plus zeros; here the parameters are ordinary random ones
(synth.make_params), so all knl^2 M look-ups of an output accumulate — across the stages of a tile, the wrap-arounds of the stage
ring, the stage groups of a pixel and the slices of a split tile.  Per output ELEMENT, against the float64 sum of
table_probe.dense_expected and relative to the element's own mag = |bias| + sum |x_j c_j| (no max-norm over a map):

    |y - want64| <= gamma(knl^2 M + CsEff + 1) * mag

— an entry is a chain of CsEff fused multiply-adds, the output a float32 sum of knl^2 M entries and the bias in ANY order, so the
bound holds for every tile, strip, slice count and stage grouping; it is derived, not measured.  With knl^2 M <= 1200 on every
shape one dropped or doubled look-up is about mag / (knl^2 M), i.e. 2^24 / (knl^2 M)^2 >= 11 bounds.

Every family is forced through the option values of the probes' family descriptors and must report its own code after every
launch (qcnn_get_layer_split: a silent fall-back fails the case).  Beside the bound:
  * the exact builder (and the K > 128 shapes, which run it under every option) returns the oracle's layer output bit for bit;
  * the families tests/test_gpu_parity.py promises bit-identical to the tile kernels on dense parameters — 16-wave sliding
    (test_sliding_kernels_*), 16-wave symmetric (test_symmetric_workgroups_*), eight-wave tile and sliding form
    (test_sym8_workgroups_*, test_sym8_sliding_form_*) — return the tile kernel's bits; the half-panel families and the split
    forms are held by the bound (for the half-panel families the count of differing elements is printed);
  * the three images of the ragged second panel, run alone, return the bits they have in the batch of 131;
  * the same layer as the first layer of [conv, relu, fcnt(8), smax] through qcnn_forward_host (default streams, every map kept)
    returns run_layer's bits, and the ReLU map is their clamp.
Batches: 131 images (a full panel and a ragged one of three); the half-panel families also 70 and 5; the split forms 125 (one
panel, where the planner cuts the tiles)."""
import numpy as np
import pytest

import table_probe as tp
from conftest import pkg
from test_gpu_table_probe import BASE, EXACT, OPT, TILE, code_ok
from test_panel_cases_cpu import FAMS, pseudo
from test_table_probe_cpu import oracle_out

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")

ORDER = ("tile", "slide16", "sym16", "sym8", "sym8_slide", "half8", "half8_slide", "split_tile", "split_sym8")
LIKE_TILE = ("slide16", "sym16", "sym8", "sym8_slide")     # bit-identical to the tile kernels on dense parameters: tests/test_gpu_parity.py
ORACLE_IMAGES = (0, 1, 63, 64, 127, 128, 129, 130)           # both halves of the full panel, the ragged panel


def families(name):
    """[(planner name or 'exact', family descriptor)] of a shape."""
    if pseudo(tp.SHAPES[name][3]) > 1:       # more than 128 code words: the exact-builder kernels under every lut option
        return [("exact", EXACT), ("tile", dict(TILE, exact=True))]
    return [("exact", EXACT)] + [(k, FAMS[k]) for k in ORDER if k in tp.PANEL_REACH[name]["live"]]


def model_for(g):
    return (g["Cin"], g["H"], g["W"]), [topo.conv(g["pad"], g["knl"], g["Ct"], g["grp"], g["stride"]), topo.relu(), topo.fcnt(8),
                                        topo.smax()]


def make_engine(in_chw, layers, params, opts):
    eng = pkg("engine").QcnnEngine(0)
    for k, v in dict(BASE, **opts).items():
        eng.set_option(OPT[k], v)
    eng.load_model(in_chw, layers, params, tp.PANEL_BATCH)
    return eng


@pytest.mark.parametrize("name", sorted(tp.PANEL_REACH))
def test_dense_sums_through_the_panel_families(name):
    kind, g, M, K, Cs, _ = tp.SHAPES[name]
    in_chw, layers = model_for(g)
    spec = synth.quant_spec(in_chw, layers)
    spec[0] = dict(spec[0], M=M, K=K, Cs=Cs)
    params = synth.make_params(in_chw, layers, seed=87, spec=spec)
    N = tp.PANEL_BATCH
    x = tp.activations(kind, g, N, seed=88, scaled=False)                       # NHWC
    inp = np.ascontiguousarray(x.transpose(0, 3, 1, 2))
    want64, mag = tp.dense_expected(kind, g, x, params[0])
    n_terms = tp.dense_count(kind, g, M, Cs)
    sel = list(ORACLE_IMAGES)
    oracle = oracle_out(kind, g, params[0], x[sel])
    tile = None
    worst, differ = {}, {}
    for key, f in families(name):
        eng = make_engine(in_chw, layers, params, f["opts"])
        label = f["label"]
        batches = (tp.PANEL_SPLIT_BATCH,) if key.startswith("split_") else (N,) + (tp.PANEL_HALF_BATCHES if key.startswith("half8") else ())
        assert sorted(batches) == sorted(f["n"])                                # the image counts of the probes' descriptors
        for n in batches:
            what = "%s / %s / %d images" % (name, label, n)
            y = eng.run_layer(0, x[:n], n)
            got = eng.layer_split(0)
            assert code_ok(f["code"], got), "%s: family code %r, expected %r" % (what, got, f["code"])
            r = tp.dense_check(y, want64[:n], mag[:n], n_terms, what=what)
            worst[label] = max(worst.get(label, 0.0), r)
            if f["exact"]:
                idx = [i for i in sel if i < n]
                assert np.array_equal(y[idx], oracle[:len(idx)]), "%s: %d elements differ from the oracle's" % (
                    what, int((y[idx] != oracle[:len(idx)]).sum()))
            if key == "tile" and not f["exact"]:
                tile = y
            if key in LIKE_TILE:
                assert tile is not None
                assert np.array_equal(y, tile[:n]), "%s: %d elements differ from the tile kernel's" % (what, int((y != tile[:n]).sum()))
            if key.startswith("half8"):
                differ[label] = differ.get(label, 0) + int((y != tile[:n]).sum())
            if n == N:                                                           # the ragged panel's three images alone
                alone = eng.run_layer(0, x[N - 3:], 3)
                assert code_ok(f["code"], eng.layer_split(0)), "%s: the last three images alone ran %r" % (what, eng.layer_split(0))
                assert np.array_equal(alone, y[N - 3:]), "%s: the last three images alone differ in %d elements" % (
                    what, int((alone != y[N - 3:]).sum()))
            if n == batches[0]:                                                  # the forward path: first layer of the model
                eng.forward_host(inp[:n])
                got = eng.layer_split(0)
                assert code_ok(f["code"], got), "%s, forward: family code %r, expected %r" % (what, got, f["code"])
                conv, relu = eng.layer_output(1, n), eng.layer_output(2, n)
                assert np.array_equal(conv, y), "%s: the forward's conv map differs from run_layer's in %d elements" % (what, int((conv != y).sum()))
                assert np.array_equal(relu, np.maximum(y, np.float32(0))), "%s: the ReLU map is not the conv map's clamp" % what
        eng.close()
    for key, f in families(name):
        extra = ", %d elements differ from the tile kernel's" % differ[f["label"]] if f["label"] in differ else ""
        print("%s: %s code %r worst err / bound %.3f%s" % (name, f["label"], f["code"], worst[f["label"]], extra))
    assert all(v <= 1.0 for v in worst.values())
