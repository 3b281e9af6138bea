"""quantize.response_report on a real pair of models: topology.tiny_model() with dense parameters in the reference engine and
their quantisation (quantize.quantize_model) in the subject, both with QCNN_OPT_KEEP_ALL = 1.  Batches of 2, 5 and 130 images:
the few-image kernels, a panel with 123 dead lanes, a panel seam with a ragged second panel.

  1. the report against the same sums taken in numpy float64 from layer_output of both engines, batch by batch — count and
     max_abs_d exact, the sums inside the reordering bound of an fp64 sum (tests/diff_ref.py) — and `agree` against the counts
     taken from the returned top-5 arrays;
  2. a model against itself: zeros on every map, complete agreement;
  3. one bias of the second conv layer raised by 1: every map in front of that layer's output reports exactly zero, that map is
     non-zero in that channel only;
  4. per-channel rows fold to the totals, to the bit;
  5. with QCNN_OPT_KEEP_ALL = 0 on one engine the map between a conv layer and its ReLU raises layer_output's message, and a
     default-maps report raises instead of skipping it."""
import copy
import math

import numpy as np
import pytest

import diff_ref as dr
from conftest import pkg

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
synth = pkg("synth")
quantize = pkg("quantize")
engine = pkg("engine")

BATCHES = (2, 5, 130)
SECOND_CONV = 4                # tiny_model: conv, relu, lorn, pool, CONV, relu, pool, fcnt, relu, drpt, fcnt, smax
BUMPED_CHANNEL = 13


@pytest.fixture(scope="module")
def world():
    in_chw, layers = topo.tiny_model()
    assert layers[SECOND_CONV]["type"] == topo.CONV and [l["type"] for l in layers[:SECOND_CONV]].count(topo.CONV) == 1
    dense = synth.make_dense_params(in_chw, layers, seed=301)
    q = engine.QcnnEngine(0)
    params, _ = quantize.quantize_model(q, in_chw, layers, dense, max_iter=10)
    q.close()
    imgs = synth.make_images(sum(BATCHES), in_chw, seed=302)
    cuts = np.cumsum((0,) + BATCHES)
    batches = [imgs[cuts[k]:cuts[k + 1]] for k in range(len(BATCHES))]
    made = []

    def quantised(p=params, keep_all=1):
        e = engine.QcnnEngine(0)
        e.set_option(capi.OPT_KEEP_ALL, keep_all)
        e.load_model(in_chw, layers, p, max(BATCHES))
        made.append(e)
        return e

    ref = engine.QcnnEngine(0)
    ref.set_option(capi.OPT_KEEP_ALL, 1)
    ref.load_dense_model(in_chw, layers, dense, max(BATCHES))
    made.append(ref)
    w = dict(in_chw=in_chw, layers=layers, params=params, batches=batches, eng=quantised(), ref=ref, quantised=quantised)
    yield w
    for e in made:
        e.close()


def accumulate(rows):
    t = np.zeros(6)
    for r in rows:
        t[:5] += r[:5]
        t[5] = max(t[5], r[5])
    return t


def test_report_against_numpy_on_layer_outputs(world):
    eng, ref, batches = world["eng"], world["ref"], world["batches"]
    maps = quantize.default_report_maps(world["layers"])
    assert maps == [1, 5, 8, 11, 12]
    want = {l: [] for l in maps}
    absd = dict.fromkeys(maps, 0.0)
    n = top1 = in5 = 0
    for x in batches:
        _, t_ref = ref.forward_host(x, want_prob=False)
        _, t_eng = eng.forward_host(x, want_prob=False)
        n += len(x)
        top1 += int((t_eng[:, 0] == t_ref[:, 0]).sum())
        in5 += sum(int(t_ref[i, 0] in t_eng[i]) for i in range(len(x)))
        for l in maps:
            a, b = eng.layer_output(l, len(x)), ref.layer_output(l, len(x))
            want[l].append(dr.map_diff(a, b, exact_sums=True)[0])
            absd[l] += float(dr.reorder_bounds(a, b)[1].sum())
    report, agree = quantize.response_report(eng, ref, batches)
    assert agree == dict(n=n, top1_equal=top1, ref_top1_in_top5=in5) and n == sum(BATCHES)
    assert sorted(report) == maps
    u = 2.0 ** -52
    for l in maps:
        w, r = accumulate(want[l]), report[l]
        N = w[0]
        assert r["count"] == N and r["nonfinite"] == 0 and r["max_abs_d"] == w[5] and w[5] > 0
        errs = (abs(r["sum_d"] - w[2]) / (N * u * absd[l]), abs(r["sum_d2"] - w[3]) / (N * u * w[3]),
                abs(r["sum_ref2"] - w[4]) / (N * u * w[4]))
        print("map %2d: %8d pairs, rel_err %.4f, mean_d %+.3e, err / bound of sum_d, sum_d2, sum_ref2: %.2g %.2g %.2g"
              % ((l, int(N), r["rel_err"], r["mean_d"]) + errs))
        assert max(errs) <= 1.0, "map %d: sums beyond the reordering bound: %r" % (l, errs)
        assert r["rel_err"] == math.sqrt(r["sum_d2"] / r["sum_ref2"]) and r["mean_d"] == r["sum_d"] / r["count"]
        assert 0 < r["rel_err"] < 10


def test_a_model_against_itself(world):
    eng, batches = world["eng"], world["batches"]
    report, agree = quantize.response_report(eng, eng, batches)
    for l, r in report.items():
        assert r["sum_d2"] == 0.0 and r["max_abs_d"] == 0.0 and r["rel_err"] == 0.0 and r["sum_d"] == 0.0, "map %d" % l
        assert r["sum_ref2"] > 0 and r["nonfinite"] == 0
    assert agree["n"] == agree["top1_equal"] == agree["ref_top1_in_top5"] == sum(BATCHES)


def test_one_bias_moves_one_channel_of_one_map(world):
    eng, batches = world["eng"], world["batches"]
    bumped = copy.deepcopy(world["params"])
    bumped[SECOND_CONV]["bias"] = bumped[SECOND_CONV]["bias"].copy()
    bumped[SECOND_CONV]["bias"][BUMPED_CHANNEL] += np.float32(1.0)
    sub = world["quantised"](bumped)
    out = SECOND_CONV + 1
    report, _ = quantize.response_report(sub, eng, batches, maps=list(range(out + 1)), per_channel=True)
    for l in range(out):
        r = report[l]
        assert r["sum_d2"] == 0.0 and r["max_abs_d"] == 0.0 and r["sum_d"] == 0.0 and r["count"] > 0, "map %d in front of the layer" % l
        assert not r["channels"][:, 2:4].any() and not r["channels"][:, 5].any()
    ch = report[out]["channels"]
    others = np.arange(len(ch)) != BUMPED_CHANNEL
    assert not ch[others][:, 2:4].any() and not ch[others, 5].any(), "another channel moved"
    hit = ch[BUMPED_CHANNEL]
    assert hit[0] == ch[0, 0] and hit[1] == 0
    # every response of that channel rose by the bias step, rounded to fp32: by half an ulp of a response below 2^23 at the most
    assert hit[3] > 0 and 0.5 <= hit[2] / hit[0] <= 1.5 and 0.5 <= hit[5] <= 1.5
    assert report[out]["sum_d2"] == hit[3] and report[out]["max_abs_d"] == hit[5]


def test_per_channel_rows_fold_to_the_totals(world):
    report, _ = quantize.response_report(world["eng"], world["ref"], world["batches"], per_channel=True)
    h_w_c = {l: world["eng"].fm_dims(l) for l in report}
    for l, r in report.items():
        assert r["channels"].shape == (h_w_c[l][2], 6)
        assert dr.bits_equal(dr.fold(r["channels"]), [r[f] for f in dr.FIELDS]), "map %d" % l
    # one batch: the device's own total is that fold as well
    x = world["batches"][2]
    world["ref"].forward_host(x, want_prob=False)
    world["eng"].forward_host(x, want_prob=False)
    for l in report:
        r = world["eng"].map_diff(world["ref"], l, len(x), per_channel=True)
        assert dr.bits_equal(dr.fold(r["channels"]), [r[f] for f in dr.FIELDS]), "map %d" % l
        assert r["count"] == len(x) * np.prod(h_w_c[l])


def test_fused_away_maps_raise(world):
    eng, batches = world["eng"], world["batches"]
    fast = world["quantised"](keep_all=0)
    x = batches[1]
    eng.forward_host(x, want_prob=False)
    fast.forward_host(x, want_prob=False)
    msg = r"feature map 1 was fused away \(QCNN_OPT_KEEP_ALL = 0\)"
    with pytest.raises(engine.QcnnError, match=msg):
        fast.layer_output(1, len(x))
    with pytest.raises(engine.QcnnError, match=msg):
        fast.map_diff(eng, 1, len(x))
    with pytest.raises(engine.QcnnError, match="reference context: " + msg):
        eng.map_diff(fast, 1, len(x))
    for sub, ref in ((fast, eng), (eng, fast)):
        with pytest.raises(engine.QcnnError, match=msg):
            quantize.response_report(sub, ref, batches)
    # maps the fast path keeps are compared as ever, and both engines go on (the refused reports left their first batch behind)
    eng.forward_host(x, want_prob=False)
    fast.forward_host(x, want_prob=False)
    r = fast.map_diff(eng, len(world["layers"]), len(x))
    assert r["count"] == len(x) * 24 and r["nonfinite"] == 0 and r["sum_ref2"] > 0
    assert eng.map_diff(eng, 1, len(x))["sum_d2"] == 0.0
