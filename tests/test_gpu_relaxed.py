"""Device-side Relaxed resize with a crop-sized mean in front of multi-view inference (qcnn_forward_u8_relaxed_views:
k_pack_u8_relaxed, the layers, k_mean_views) bit for bit against tests/relaxed_ref.py — the restatement of the reference's
BmpImgIO::ReszImg (Relaxed) / CropImg / RmMeanImg (Crop) that tests/test_relaxed_cpu.py holds to the host mirror and, where the
modes coincide, to tests/resize_ref.py.

  * the pack kernel per element on a glue-only network (fm[0] read back): nominal full size 12 x 14 with the source sizes of
    relaxed_ref.SOURCES cycled over the images — every image has its own full size, two of them under the nominal one — slots
    across panel seams and a ragged last panel, 1 / 7 / 10 / 32 views on all three anchors of both axes with offsets, mirrors
    and repeats, no mean, a random mean, a mean under which no two positions agree;
  * sources on which Relaxed is Strict: every output equals qcnn_forward_u8_resized_views' under a full-size mean whose window
    is the crop mean;
  * the whole path on the tiny network against qcnn_forward_host of the host-made inputs at the same slot count; three slots on
    the few-image kernels; NULL outputs; the descriptor staging grows; calls back to back without a sync between them;
  * every rejected argument: non-zero with a message, outputs and fm[0] untouched, the next call right."""
import functools
import itertools

import numpy as np
import pytest
import torch

import glue_ref as gr
import relaxed_ref as xr
import views_ref as vr
from conftest import pkg, tiny_params_from_golden
from u8_harness import DEV, Outputs, Source, bits_equal, make_engine, run_sources

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
engine = pkg("engine")


Source = functools.partial(Source, "forward_u8_relaxed_views_dev")
run_relaxed = functools.partial(run_sources, "forward_u8_relaxed_views_dev")


# ---------------------------------------------------------------------------------------------- 1. the pack kernel, per element
PACK_CHW, FULL = (3, 5, 7), xr.FULL_HW            # E = 105: one full 64-element block and a tail of 41; nominal full size 12 x 14
TEN = xr.ten_crop_anchored()
# The smallest full sizes among the sources are 12 rows (12 x 14) and 13 columns (54 x 13, 13 x 13): a 5 x 7 view has 7 rows and
# 6 columns of room there, its centre anchor sits at (3, 3), and the offsets below keep every view inside EVERY image.
ODD = [(2, 2, 0, 0, 0), (0, 1, 1, -3, 1), (1, 0, 3, 1, 0), (0, 1, 1, -3, 1), (2, 2, -1, -2, 1), (0, 0, 0, 0, 1), (1, 2, -2, -5, 0)]
ROOM = {0: (0, 6), 1: (-3, 3), 2: (-6, 0)}        # offsets that are safe under an anchor on both axes


def _many_views(count, seed):
    rng = np.random.default_rng(seed)
    out = [(2, 2, 0, 0, 1), (0, 2, 6, -6, 0)]
    pairs = list(itertools.product(range(3), repeat=2))
    for k in range(count - 2):                    # every pair of anchors, then random ones
        ay, ax = pairs[k] if k < len(pairs) else (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        out.append((ay, ax, int(rng.integers(ROOM[ay][0], ROOM[ay][1] + 1)), int(rng.integers(ROOM[ax][0], ROOM[ax][1] + 1)), int(rng.integers(0, 2))))
    return out


def _mean(kind, rng, chw):
    """'position': no two elements of the crop share a value — 1000 x the element's index (exact in fp32)."""
    return {"none": None, "random": (rng.standard_normal(chw) * 20 + 110).astype(np.float32),
            "position": (np.arange(chw[0] * chw[1] * chw[2], dtype=np.float32) * np.float32(1000)).reshape(chw)}[kind]


PACK_SHAPES = [
    ("ten_crop", 27, TEN),                        # 270 slots = two panels + 14, images 12 and 25 straddle a seam
    ("odd", 27, ODD),                             # 189 slots, image 18 straddles the seam
    ("max_views", 5, _many_views(32, 71)),        # 160 slots
    ("one_view", 131, [(2, 1, -1, 2, 0)]),        # 131 slots: one image per slot, every source size fourteen times
]
PACK_CASES = [(name + "-" + kind, n, views, kind) for name, n, views in PACK_SHAPES for kind in ("none", "random", "position")]


@pytest.fixture(scope="module")
def pack_engine():
    eng = make_engine(PACK_CHW, [topo.relu()], {}, 270)
    yield eng
    eng.close()


def test_the_view_sets_cover_every_anchor():
    assert {v[0] for v in ODD} == {v[1] for v in ODD} == {0, 1, 2} and any(v[2] and v[3] for v in ODD) and any(v[4] for v in ODD)
    many = PACK_SHAPES[2][2]
    assert len(many) == 32 and {(v[0], v[1]) for v in many} == set(itertools.product(range(3), repeat=2))
    for views in (TEN, ODD, many, PACK_SHAPES[3][2]):
        for hf, wf in xr.SIZES:
            assert all(xr.resolve(v, hf, wf, PACK_CHW[1], PACK_CHW[2]) is not None for v in views)


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: c[0])
def test_pack_per_element(pack_engine, case):
    _, n, views, mean_kind = case
    c, h, w = PACK_CHW
    rng = np.random.default_rng(500 + n + len(views))
    images = xr.random_images(rng, n, c)
    assert n < len(xr.SOURCES) or {a.shape[1:] for a in images} == set(xr.SOURCES)
    mean = _mean(mean_kind, rng, PACK_CHW)
    want = vr.nhwc(xr.make_views(images, FULL[0], FULL[1], mean, views, h, w))
    _, _, rows = run_relaxed(pack_engine, images, FULL, mean, views, want=(False, False, True))
    got = pack_engine.layer_output(0, n * len(views))
    if not bits_equal(got, want):
        diff = got.view(np.uint32) != want.view(np.uint32)
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        img = at[0] // len(views)
        raise AssertionError("fm[0] differs in %d of %d elements; first at (slot, y, x, c) = %r (image %d of size %r, view %r): got %r, expected %r"
                             % (int(diff.sum()), got.size, at, img, images[img].shape[1:], views[at[0] % len(views)], got[at], want[at]))
    assert bits_equal(rows, np.maximum(want, np.float32(0)).reshape(n * len(views), -1))     # the ReLU behind it, slot for slot


# ---------------------------------------------------------------------------------------------- 2. where Relaxed is Strict
@pytest.mark.parametrize("mean_kind", ["none", "random"])
def test_same_bits_as_the_resized_call_where_the_modes_coincide(pack_engine, mean_kind):
    """Equal float scales and the nominal size (12 x 14, 23 x 27 and 34 x 40 at 12 x 14: scales 1, 2, 3): one plain view, a
    full-size mean whose window under that view is the crop mean — every output of the two calls has the same bits."""
    n, (c, h, w) = 27, PACK_CHW
    oy, ox = 3, 2
    rng = np.random.default_rng(43)
    images = xr.random_images(rng, n, c, [(12, 14), (23, 27), (34, 40)])
    for a in images[:3]:
        hf, wf, s = xr.full_size(a.shape[1], a.shape[2], *FULL)
        assert (hf, wf) == FULL and float(s) == (a.shape[1] - 1) // 11 == (a.shape[2] - 1) // 13
    full_mean = (rng.standard_normal((c,) + FULL) * 20 + 110).astype(np.float32) if mean_kind == "random" else None
    crop_mean = np.ascontiguousarray(full_mean[:, oy:oy + h, ox:ox + w]) if full_mean is not None else None
    src = Source(images, crop_mean)
    d_full_mean = torch.from_numpy(full_mean).to(DEV) if full_mean is not None else None
    ref = Outputs(pack_engine, n, 1)
    torch.cuda.synchronize()
    pack_engine.forward_u8_resized_views_dev(src.d_flat.data_ptr(), src.flat.size, src.descs, FULL[0], FULL[1],
                                             d_full_mean.data_ptr() if d_full_mean is not None else None, [(oy, ox, 0)], *ref.ptrs())
    pack_engine.sync()
    fm0 = pack_engine.layer_output(0, n)
    want_prob, want_top5, want_rows = ref.host()
    assert np.isfinite(want_rows).all()
    out = Outputs(pack_engine, n, 1)
    src.call(pack_engine, FULL, [(0, 0, oy, ox, 0)], out)
    pack_engine.sync()
    prob, top5, rows = out.host()
    assert bits_equal(pack_engine.layer_output(0, n), fm0)
    assert bits_equal(rows, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


# ---------------------------------------------------------------------------------------------- 3. the whole path, tiny network
TINY_FULL = (40, 45)
TINY_SOURCES = [(40, 45), (14, 54), (30, 8), (37, 53), (100, 75), (6, 9), (500, 375)]      # 6 x 9 comes out 39 x 63: under the nominal 40


class Tiny:
    """The tiny network with the golden parameters, MFMA builder, 130 batch slots; 13 source images of differing sizes under the
    ten anchored views, and the reference forward of their 130 host-made inputs (computed once)."""

    def __init__(self, z):
        self.in_chw, self.layers = topo.tiny_model()
        self.params = tiny_params_from_golden(z, self.layers)
        rng = np.random.default_rng(83)
        self.images = xr.random_images(rng, 13, self.in_chw[0], TINY_SOURCES)
        self.mean = (rng.standard_normal(self.in_chw) * 20 + 110).astype(np.float32)
        self.views = engine.ten_crop_anchored()
        self.eng = self.engine()
        self.rows, self.fm0, self.prob, self.top5 = self.reference(self.images, self.views)

    def engine(self, max_batch=130):
        return make_engine(self.in_chw, self.layers, self.params, max_batch, lut=capi.LUT_MFMA)

    def reference(self, images, views, eng=None):
        """qcnn_forward_host on the host-made inputs, at the slot count of the call under test."""
        eng = eng or self.eng
        _, h, w = self.in_chw
        rows, _ = eng.forward_host(xr.make_views(images, TINY_FULL[0], TINY_FULL[1], self.mean, views, h, w))
        fm0 = eng.layer_output(0, len(images) * len(views))
        prob = vr.mean_views(rows, len(views))
        return rows, fm0, prob, gr.top5(prob)

    def check(self, eng, want=(True, True, True)):
        got = run_relaxed(eng, self.images, TINY_FULL, self.mean, self.views, want)
        assert got[0] is None if not want[0] else bits_equal(got[0], self.prob)
        assert got[1] is None if not want[1] else np.array_equal(got[1], self.top5)
        assert got[2] is None if not want[2] else bits_equal(got[2], self.rows)


@pytest.fixture(scope="module")
def tiny(golden_tiny):
    t = Tiny(golden_tiny)
    yield t
    t.eng.close()


def test_whole_path_ten_anchored_views(tiny):
    assert np.isfinite(tiny.rows).all()
    sizes = {xr.full_size(a.shape[1], a.shape[2], *TINY_FULL)[:2] for a in tiny.images}
    assert len(sizes) >= 6 and any(min(s) < min(TINY_FULL) for s in sizes)      # every image its own size, one under the nominal
    prob, top5, rows = run_relaxed(tiny.eng, tiny.images, TINY_FULL, tiny.mean, tiny.views)
    assert bits_equal(tiny.eng.layer_output(0, 130), tiny.fm0)
    assert bits_equal(rows, tiny.rows)
    assert bits_equal(prob, tiny.prob)
    assert np.array_equal(top5, tiny.top5)


def test_host_convenience_call_is_load_and_forward(tiny):
    """forward_u8_relaxed_host with its default view: resize, centre crop, crop mean (BmpImgIO::Load), then the layers."""
    want_rows, _, want_prob, want_top5 = tiny.reference(tiny.images, [xr.CENTRE])
    prob, top5, rows = tiny.eng.forward_u8_relaxed_host(tiny.images, TINY_FULL, tiny.mean)
    assert rows.shape == (13, 1, want_rows.shape[1])
    assert bits_equal(rows.reshape(13, -1), want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


def test_one_image_three_views_on_the_few_image_kernels(tiny):
    views = [tiny.views[1], tiny.views[9], (0, 1, 3, -2, 0)]
    images = tiny.images[2:3]                                        # the 30 x 8 source
    want_rows, _, want_prob, want_top5 = tiny.reference(images, views)
    conv = [l for l, ly in enumerate(tiny.layers) if ly["type"] == topo.CONV][0]
    family = tiny.eng.layer_split(conv)
    prob, top5, rows = run_relaxed(tiny.eng, images, TINY_FULL, tiny.mean, views)
    print("first conv layer at three slots: family code %r" % (family,))
    assert tiny.eng.layer_split(conv) == family                      # the same kernel family took both launches
    assert bits_equal(rows, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


def test_null_outputs_in_every_combination(tiny):
    for want in itertools.product((True, False), repeat=3):
        tiny.check(tiny.eng, want)
    assert bits_equal(tiny.eng.layer_output(0, 130), tiny.fm0)       # also with no output at all the slots went through


def test_descriptor_staging_grows(tiny):
    """The staging buffers hold 64 descriptors at first: 130 images need larger ones; the small call again afterwards."""
    c, h, w = tiny.in_chw
    eng = tiny.engine()
    tiny.check(eng)
    tiny.check(eng)                                                  # both staging sets in use
    rng = np.random.default_rng(84)
    images = xr.random_images(rng, 130, c, TINY_SOURCES)
    view = [(2, 0, -1, 0, 1)]
    want_rows, _, want_prob, want_top5 = tiny.reference(images, view, eng)
    for _ in range(2):                                               # both sets grow
        prob, top5, rows = run_relaxed(eng, images, TINY_FULL, tiny.mean, view)
        assert bits_equal(rows, want_rows) and bits_equal(prob, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)
    tiny.check(eng)
    eng.close()


def test_calls_back_to_back_keep_their_descriptors(tiny):
    """Three calls with three descriptor lists over the same source buffer and no sync between them: the third takes the
    staging set of the first and must not rewrite it under the first call's pack kernel."""
    order = [list(range(13)), list(range(12, -1, -1)), [(5 * i) % 13 for i in range(13)]]
    refs = [tiny.reference([tiny.images[i] for i in o], tiny.views) for o in order]
    src = Source(tiny.images, tiny.mean)
    outs = [Outputs(tiny.eng, 13, 10) for _ in order]
    for o, out in zip(order, outs):
        src.call(tiny.eng, TINY_FULL, tiny.views, out, descs=[src.descs[i] for i in o])
    tiny.eng.sync()
    for (want_rows, _, want_prob, want_top5), out in zip(refs, outs):
        prob, top5, rows = out.host()
        assert bits_equal(rows, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)
    assert bits_equal(refs[0][0], tiny.rows) and not bits_equal(refs[1][0], tiny.rows)


# ---------------------------------------------------------------------------------------------- 4. rejected arguments
def test_rejections_enqueue_nothing(tiny):
    c, h, w = tiny.in_chw
    fh, fw = TINY_FULL
    eng = tiny.engine()
    tiny.check(eng)
    src = Source(tiny.images, tiny.mean)
    size, one, centre = src.flat.size, src.descs[:1], [xr.CENTRE]
    last_off, last_h, last_w = src.descs[-1]
    with pytest.raises(engine.QcnnError):                             # the size rule refuses it: the call below never launches
        engine.relaxed_full_size(2, 2 ** 20, fh, fw)
    bad = [
        # (descs, full, views, src_bytes, a word of the message)
        ([], TINY_FULL, centre, size, "no image"),                                            # n = 0
        (one, TINY_FULL, [], size, "views"),                                                  # no view
        (one, TINY_FULL, [xr.CENTRE] * 33, size, "views"),                                    # more than QCNN_MAX_VIEWS
        (src.descs * 11, TINY_FULL, centre, size, "batch slots"),                             # 143 slots
        (src.descs + one, TINY_FULL, tiny.views, size, "batch slots"),                        # 140 slots
        (one, (h - 1, fw), centre, size, "smaller than the network input"),
        (one, (fh, w - 1), centre, size, "smaller than the network input"),
        (one, (1, fw), centre, size, "at least 2"),
        (one, (fh, 0), centre, size, "at least 2"),
        (one + [(0, 1, 50)], TINY_FULL, centre, size, "image 1"),                             # a 1-pixel-high source
        (one + [(0, 50, 1)], TINY_FULL, centre, size, "image 1"),                             # a 1-pixel-wide source
        (one + [(0, 0, 5)], TINY_FULL, centre, size, "image 1"),
        (one + [(0, -3, 5)], TINY_FULL, centre, size, "image 1"),
        (one, TINY_FULL, [(3, 1, 0, 0, 0)], size, "outside 0..2"),                            # ay = 3
        (one, TINY_FULL, [xr.CENTRE, (1, -1, 0, 0, 0)], size, "outside 0..2"),
        (one, TINY_FULL, [(0, 0, -1, 0, 0)], size, "leaves"),                                 # above the top edge
        (one, TINY_FULL, [(2, 2, 0, 1, 1)], size, "leaves"),                                  # past the right edge
        (one, TINY_FULL, [(1, 1, 0, 0, 0), (1, 1, 2 ** 31 - 1, 0, 0)], size, "view 1"),
        ([(0, 2, 2 ** 20)], TINY_FULL, centre, 2 ** 40, "2^24"),                              # Wf = 39 * (2^20 - 1) + 1
        ([(0, 46341, 46341)], TINY_FULL, centre, size, "2 GiB"),                              # 3 x 46341^2 bytes > 2^31 - 1
        (src.descs[:-1] + [(last_off + 1, last_h, last_w)], TINY_FULL, centre, size, "leave the source buffer"),   # one byte over
        (src.descs, TINY_FULL, centre, size - 1, "leave the source buffer"),                  # the buffer one byte short
        ([(2 ** 64 - 1, 2, 2)], TINY_FULL, centre, size, "leave the source buffer"),          # offset + bytes wraps around
    ]
    for descs, full, views, src_bytes, word in bad:
        out = Outputs(eng, 13, 10)
        with pytest.raises(engine.QcnnError) as err:
            src.call(eng, full, views, out, descs=descs, src_bytes=src_bytes)
        eng.sync()
        assert word in str(err.value), (word, str(err.value))
        assert out.untouched(), "a rejected call wrote an output (%s)" % word
        assert bits_equal(eng.layer_output(0, 130), tiny.fm0), "a rejected call wrote the input map (%s)" % word
    tiny.check(eng)
    eng.close()
    fresh = engine.QcnnEngine(0)                                      # no model committed
    with pytest.raises(engine.QcnnError) as err:
        fresh.forward_u8_relaxed_views_dev(src.d_flat.data_ptr(), size, one, fh, fw, None, centre)
    assert "not committed" in str(err.value)
    fresh.close()


def test_one_image_too_narrow_refuses_the_whole_call():
    """A network input of width 14 at the nominal full size 12 x 14: it fits 12 x 14, 12 x 16 and 12 x 14 but not the 54 x 13
    the reference's arithmetic gives the 30 x 8 source.  The message names the image and the view."""
    chw = (3, 5, 14)
    eng = make_engine(chw, [topo.relu()], {}, 16)
    rng = np.random.default_rng(45)
    sources = [(12, 14), (37, 53), (30, 8), (24, 27)]
    assert [xr.full_size(h, w, *FULL)[:2] for h, w in sources] == [(12, 14), (12, 16), (54, 13), (12, 14)]
    images = xr.random_images(rng, 4, 3, sources)
    mean = (rng.standard_normal(chw) * 20 + 110).astype(np.float32)
    views = [(0, 0, 0, 0, 0), xr.CENTRE, (2, 2, 0, 0, 1)]
    good = [images[0], images[1], images[3]]
    want = vr.nhwc(xr.make_views(good, FULL[0], FULL[1], mean, views, 5, 14))
    _, _, rows = run_relaxed(eng, good, FULL, mean, views)
    fm0 = eng.layer_output(0, 9)
    assert bits_equal(fm0, want)
    src = Source(images, mean)
    out = Outputs(eng, 4, 3)
    with pytest.raises(engine.QcnnError) as err:
        src.call(eng, FULL, views, out)
    eng.sync()
    assert "image 2, view 0" in str(err.value) and "54x13" in str(err.value), str(err.value)
    assert out.untouched() and bits_equal(eng.layer_output(0, 9), fm0)
    _, _, rows2 = run_relaxed(eng, good, FULL, mean, views)          # the next call is right
    assert bits_equal(rows2, rows) and bits_equal(eng.layer_output(0, 9), fm0)
    eng.close()
