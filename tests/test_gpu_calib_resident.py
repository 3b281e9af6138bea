"""Resident calibration on the GPU (qcnn_calib_begin / _arm / _read / _end, kernel k_ec_gram_panel) against the numpy fp64
reference (tests/calib_ref.py) on the crafted cases of tests/calib_cases.py.  Values are small integers unless said otherwise:
every fp32 run sum is exact, so the resident matrix equals the reference TO THE BIT.  Before each batch an unarmed forward of
max_batch images of value 977.5 leaves junk in the lanes a ragged batch does not fill."""
import functools

import numpy as np
import pytest

import calib_cases as cc
import calib_ref as cr
import ec_oracle as eo
from conftest import pkg

pytestmark = pytest.mark.gpu

topo = pkg("topology")
synth = pkg("synth")
capi = pkg("capi")
engine = pkg("engine")
quantize = pkg("quantize")
JUNK = 977.5
U32 = 2.0 ** -24


def gamma(r, u=U32):
    return r * u / (1.0 - r * u)


def whole_panels(n):
    return (n + cr.PANEL - 1) // cr.PANEL * cr.PANEL


def load(case, max_batch, dense=None):
    e = engine.QcnnEngine(0)
    e.load_dense_model(case.in_chw, case.layers, dense or cc.dense_params(case), max_batch)
    return e


def junk_forward(eng, case, max_batch):
    """Unarmed: adds nothing, and leaves 977.5-derived values in every lane of every map."""
    eng.calib_arm(False)
    eng.forward_host(np.full((max_batch,) + tuple(case.in_chw), JUNK, np.float32), want_prob=False, want_top5=False)
    eng.calib_arm(True)


@functools.lru_cache(maxsize=None)
def reference(name, n, seed=0):
    case = cc.BY_NAME[name]
    geom, flat = cc.geom_of(case)
    panels = cr.to_panels(cc.listed_input(case, cc.images(case, n, seed)), JUNK)
    G, rows = cr.gram_from_panels(panels, n, geom, flat)
    G.setflags(write=False)
    return G, rows


def resident(eng, case, n, max_batch, seed=0):
    junk_forward(eng, case, max_batch)
    eng.forward_host(cc.images(case, n, seed), want_prob=False, want_top5=False)
    return eng.calib_read(case.listed)


RUNS = [(c.name, n) for c in cc.CASES for n in c.ns]


@pytest.mark.parametrize("name,n", RUNS, ids=["%s-n%d" % r for r in RUNS])
def test_crafted_case_to_the_bit(name, n):
    case = cc.BY_NAME[name]
    want, rows = reference(name, n)
    mb = whole_panels(n)
    eng = load(case, mb)
    try:
        eng.calib_begin([case.listed])
        got, got_rows = resident(eng, case, n, mb)
    finally:
        eng.close()
    assert got.dtype == np.float64 and got.shape == want.shape
    assert got_rows == rows
    assert np.array_equal(got, got.transpose(0, 2, 1)), "not symmetric to the bit"
    bad = np.argwhere(got != want)
    assert got.tobytes() == want.tobytes(), "first differing entries (g, p, q): %s" % bad[:8].tolist()


def test_splits_take_the_slab_path_and_repeat_their_bits():
    case, n = cc.BY_NAME[cc.SPLITS_CASE], cc.SPLITS_N
    geom, _ = cc.geom_of(case)
    assert cr.units_per_split(geom, whole_panels(n) // cr.PANEL, engine.EC_GRAM_RUN)[1] >= 2
    want, rows = reference(case.name, n)
    mb = whole_panels(n)
    eng = load(case, mb)
    try:
        runs = []
        for _ in range(2):
            eng.calib_begin([case.listed])
            runs.append(resident(eng, case, n, mb))
            eng.calib_end()
    finally:
        eng.close()
    assert runs[0][1] == runs[1][1] == rows == 4550
    assert runs[0][0].tobytes() == runs[1][0].tobytes() == want.tobytes()


def test_accumulation_over_batches_reads_and_restarts():
    case = cc.BY_NAME["one_tile"]
    geom, flat = cc.geom_of(case)
    parts = [cc.images(case, n, seed) for seed, n in enumerate((130, 5, 1))]
    allx = cc.listed_input(case, np.concatenate(parts))
    want, rows = cr.gram_from_panels(cr.to_panels(allx, JUNK), len(allx), geom, flat)
    mb = 256
    eng = load(case, mb)
    try:
        eng.calib_begin([0])
        for x in parts:
            junk_forward(eng, case, mb)                  # an unarmed forward in between adds nothing
            eng.forward_host(x, want_prob=False, want_top5=False)
        got, got_rows = eng.calib_read(0)
        again, again_rows = eng.calib_read(0)
        eng.calib_end()
        eng.calib_begin([0])
        zero, zero_rows = eng.calib_read(0)
    finally:
        eng.close()
    assert got_rows == again_rows == rows == 136 * 35
    assert got.tobytes() == want.tobytes()
    assert again.tobytes() == got.tobytes()
    assert zero_rows == 0 and not zero.any()


def test_streamed_u8_batches_count_every_slot_once_and_keep_their_outputs():
    case = cc.BY_NAME["one_tile"]
    C, H, W = case.in_chw
    full = (H + 2, W + 2)
    views = [(1, 1, 0), (1, 1, 1)]                                          # the plain crop and its mirror
    rng = np.random.default_rng(11)
    srcs = [rng.integers(0, 4, (C,) + full).astype(np.uint8) for _ in range(173)]
    cut = engine.split_batches(srcs, None, 140, len(views))                 # 70, 70 and 33 images x 2 views
    assert [len(d) for _, d, _ in cut] == [70, 70, 33]
    batches = [(f, d) for f, d, _ in cut]
    dense = cc.dense_params(case)
    dense[0]["weights"] = np.random.default_rng(12).standard_normal(dense[0]["weights"].shape).astype(np.float32)
    crops = np.stack([s[:, 1:1 + H, 1:1 + W] for s in srcs]).astype(np.float32)
    slots = np.concatenate([crops, crops[..., ::-1]])                        # the order of the slots does not matter to a sum
    geom, flat = cc.geom_of(case)
    want, rows = cr.gram_from_panels(cr.to_panels(cc.listed_input(case, slots), JUNK), len(slots), geom, flat)
    mb = 256
    eng = load(case, mb, dense)
    try:
        eng.calib_begin([0])
        junk_forward(eng, case, mb)
        eng.calib_arm(False)
        p0, t0, r0, _ = eng.forward_u8_host_batches(batches, full, None, views, "strict", want=(True, True, True))
        none, none_rows = eng.calib_read(0)
        eng.calib_arm(True)
        p1, t1, r1, _ = eng.forward_u8_host_batches(batches, full, None, views, "strict", want=(True, True, True))
        got, got_rows = eng.calib_read(0)
    finally:
        eng.close()
    assert none_rows == 0 and not none.any()
    assert got_rows == rows == 346 * 35
    assert got.tobytes() == want.tobytes()
    for a, b in zip(p0 + t0 + r0, p1 + t1 + r1):
        assert a.tobytes() == b.tobytes(), "an armed calibration changed a forward's outputs"


def test_ordinary_values_within_the_bound_and_through_quantize():
    """Gaussian images through the tiny dense model, 48 in chunks of 20 (a ragged chunk of 8): per entry within
    gamma_260 * sum |s_p s_q| of the fp64 gram of the float32 maps the engine itself returns (fp32 runs of 256 rows on a
    depth-4 MFMA, fp64 across runs)."""
    in_chw, layers = topo.tiny_model()
    dense = synth.make_dense_params(in_chw, layers, seed=75)
    imgs = synth.make_images(48, in_chw, seed=76)
    ids = sorted(dense)
    eng = engine.QcnnEngine(0)
    try:
        eng.set_option(capi.OPT_KEEP_ALL, 1)
        eng.load_dense_model(in_chw, layers, dense, 20)
        eng.calib_begin(ids)
        want = {i: 0.0 for i in ids}
        scale = {i: 0.0 for i in ids}
        for n0 in range(0, 48, 20):
            part = imgs[n0:n0 + 20]
            eng.forward_host(part, want_prob=False, want_top5=False)
            for i in ids:
                g = quantize.layer_geom(layers, i)
                G, S = eo.gram(quantize.layer_input(layers, i, eng.layer_output(i, len(part))), g["grp"], g["kh"], g["kw"], g["stride"], g["pad"])
                want[i], scale[i] = want[i] + G, scale[i] + S
        got = {i: eng.calib_read(i)[0] for i in ids}
        eng.calib_end()
        res = quantize.calibrate(eng, in_chw, layers, dense, imgs, chunk=20, resident=True)
        old = quantize.calibrate(eng, in_chw, layers, dense, imgs, chunk=20)
    finally:
        eng.close()
    for i in ids:
        bound = gamma(engine.EC_GRAM_RUN + 4) * scale[i]
        err = np.abs(got[i] - want[i])
        err_old = np.abs(old[i] - got[i])
        print("layer %d: worst |G - G64| / bound = %.3g; calibrate() as it is against it: %.3g of twice the bound"
              % (i, float((err / np.maximum(bound, 1e-300)).max()), float((err_old / np.maximum(2 * bound, 1e-300)).max())))
        assert (err <= bound).all()
        assert np.array_equal(got[i], got[i].transpose(0, 2, 1)), "not symmetric to the bit"
        assert res[i].tobytes() == got[i].tobytes(), "calibrate(resident=True) returns other matrices"
        assert (err_old <= 2 * bound).all()


def test_refusals_leave_everything_as_it_was():
    case = cc.BY_NAME["relu_conv"]                      # layer 0 is a ReLU, layer 1 the conv
    n, mb = 5, 128
    x = cc.images(case, n)
    dense = cc.dense_params(case)
    dense[1]["weights"] = np.random.default_rng(13).standard_normal(dense[1]["weights"].shape).astype(np.float32)
    fresh = engine.QcnnEngine(0)
    try:
        with pytest.raises(engine.QcnnError, match="not committed"):
            fresh.calib_begin([0])
    finally:
        fresh.close()
    eng = load(case, mb, dense)
    try:
        before, _ = eng.forward_host(x, want_top5=False)
        for call, msg in ((lambda: eng.calib_read(1), "no calibration"), (lambda: eng.calib_arm(True), "no calibration"),
                          (lambda: eng.calib_end(), "no calibration"), (lambda: eng.calib_begin([0]), "layer 0"),
                          (lambda: eng.calib_begin([1, 1]), "layer 1"), (lambda: eng.calib_begin([7]), "layer 7")):
            with pytest.raises(engine.QcnnError, match=msg):
                call()
        with pytest.raises(engine.QcnnError, match="no calibration"):       # nothing above opened one
            eng.calib_arm(False)
        eng.calib_begin([1])
        eng.forward_host(x, want_prob=False, want_top5=False)
        held, rows = eng.calib_read(1)
        with pytest.raises(engine.QcnnError, match="already open"):
            eng.calib_begin([1])
        with pytest.raises(engine.QcnnError, match="layer 0"):
            eng.calib_read(0)
        again, again_rows = eng.calib_read(1)
        eng.calib_arm(False)
        after, _ = eng.forward_host(x, want_top5=False)
    finally:
        eng.close()
    assert rows == again_rows == n * 35 and held.any()
    assert again.tobytes() == held.tobytes()
    assert after.tobytes() == before.tobytes()


def test_loading_another_model_ends_the_calibration():
    case, other = cc.BY_NAME["one_tile"], cc.BY_NAME["first_fc"]
    eng = load(case, 128)
    try:
        eng.calib_begin([0])
        eng.forward_host(cc.images(case, 5), want_prob=False, want_top5=False)
        assert eng.calib_read(0)[1] == 5 * 35
        eng.load_dense_model(other.in_chw, other.layers, cc.dense_params(other), 128)
        for call in (lambda: eng.calib_read(0), lambda: eng.calib_arm(True), lambda: eng.calib_end()):
            with pytest.raises(engine.QcnnError, match="no calibration"):
                call()
        eng.forward_host(cc.images(other, 5), want_prob=False, want_top5=False)     # unarmed, as if nothing had been begun
        eng.calib_begin([0])
        got, rows = eng.calib_read(0)
        assert rows == 0 and not got.any() and got.shape == (1, 30, 30)
    finally:
        eng.close()
