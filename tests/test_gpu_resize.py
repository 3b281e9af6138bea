"""Device-side resize in front of multi-view inference (qcnn_forward_u8_resized_views: k_pack_u8_resized, the layers,
k_mean_views) bit for bit against tests/resize_ref.py — the float32 restatement of the reference's BmpImgIO::ReszImg that
tests/test_resize_cpu.py holds to the compiled reference — and tests/views_ref.py.

  * the pack kernel per element on a glue-only network (fm[0] read back): full image 12 x 14 with the source sizes of
    resize_ref.SOURCES cycled over the images (identity, the rounding seams in both axes, one-pixel / one-row / upscaled / very
    wide sources, offsets beyond 16 bits), slots across panel seams and a ragged last panel, 1 / 7 / 10 / 32 views, no mean, a
    random mean, a mean under which no two positions agree;
  * sources of the full size: every output equals qcnn_forward_u8_views' on the same bytes;
  * the whole path on the tiny network against qcnn_forward_host of the host-made inputs at the same slot count; three slots on
    the few-image kernels; NULL outputs; the descriptor staging grows; calls back to back without a sync between them;
  * every rejected argument: non-zero with a message, outputs and fm[0] untouched, the next call right."""
import functools
import itertools

import numpy as np
import pytest
import torch

import glue_ref as gr
import resize_ref as rr
import views_ref as vr
from conftest import pkg, tiny_params_from_golden
from u8_harness import DEV, Outputs, Source, bits_equal, make_engine, run_sources

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
engine = pkg("engine")


Source = functools.partial(Source, "forward_u8_resized_views_dev")
run_resized = functools.partial(run_sources, "forward_u8_resized_views_dev")


# ---------------------------------------------------------------------------------------------- 1. the pack kernel, per element
PACK_CHW, FULL = (3, 5, 7), rr.FULL_HW            # E = 105: one full 64-element block and a tail of 41; full image 12 x 14
TEN = vr.ten_crop(FULL[0], FULL[1], 5, 7)         # the bottom and right corners reach the seam row 11 and the seam column 13
ODD = [(7, 7, 0), (1, 3, 1), (3, 1, 0), (1, 3, 1), (7, 7, 1), (0, 0, 1), (2, 5, 0)]      # the far corner, odd offsets, mirrors, a repeat


def _many_views(count, seed):
    rng = np.random.default_rng(seed)
    return [(7, 7, 1), (0, 7, 0)] + [(int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 2))) for _ in range(count - 2)]


def _mean(kind, rng, c, full):
    """'position': no two elements of the full image share a value — 1000 x the element's index (exact in fp32)."""
    return {"none": None, "random": (rng.standard_normal((c,) + tuple(full)) * 20 + 110).astype(np.float32),
            "position": (np.arange(c * full[0] * full[1], dtype=np.float32) * np.float32(1000)).reshape((c,) + tuple(full))}[kind]


PACK_SHAPES = [
    ("ten_crop", 27, TEN),                        # 270 slots = two panels + 14, images 12 and 25 straddle a seam
    ("odd", 27, ODD),                             # 189 slots, image 18 straddles the seam
    ("max_views", 5, _many_views(32, 71)),        # 160 slots
    ("one_view", 131, [(7, 7, 0)]),               # 131 slots: one image per slot, every source size fifteen times
]
PACK_CASES = [(name + "-" + kind, n, views, kind) for name, n, views in PACK_SHAPES for kind in ("none", "random", "position")]


@pytest.fixture(scope="module")
def pack_engine():
    eng = make_engine(PACK_CHW, [topo.relu()], {}, 270)
    yield eng
    eng.close()


@pytest.mark.parametrize("case", PACK_CASES, ids=lambda c: c[0])
def test_pack_per_element(pack_engine, case):
    _, n, views, mean_kind = case
    c, h, w = PACK_CHW
    rng = np.random.default_rng(300 + n + len(views))
    images = rr.random_images(rng, n, c)
    assert n < len(rr.SOURCES) or {a.shape[1:] for a in images} == set(rr.SOURCES)
    mean = _mean(mean_kind, rng, c, FULL)
    want = vr.nhwc(rr.make_views(images, FULL[0], FULL[1], mean, views, h, w))
    _, _, rows = run_resized(pack_engine, images, FULL, mean, views, want=(False, False, True))
    got = pack_engine.layer_output(0, n * len(views))
    if not bits_equal(got, want):
        diff = got.view(np.uint32) != want.view(np.uint32)
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        img = at[0] // len(views)
        raise AssertionError("fm[0] differs in %d of %d elements; first at (slot, y, x, c) = %r (image %d of size %r, view %r): got %r, expected %r"
                             % (int(diff.sum()), got.size, at, img, images[img].shape[1:], views[at[0] % len(views)], got[at], want[at]))
    assert bits_equal(rows, np.maximum(want, np.float32(0)).reshape(n * len(views), -1))     # the ReLU behind it, slot for slot


# ---------------------------------------------------------------------------------------------- 2. sources of the full size
@pytest.mark.parametrize("mean_kind", ["none", "random"])
def test_full_size_sources_are_forward_u8_views(pack_engine, mean_kind):
    n, (c, h, w) = 27, PACK_CHW
    rng = np.random.default_rng(41)
    px = rng.integers(0, 256, (n, c) + FULL, dtype=np.uint8)
    mean = _mean(mean_kind, rng, c, FULL)
    d_px = torch.from_numpy(px).to(DEV)
    d_mean = torch.from_numpy(mean).to(DEV) if mean is not None else None
    ref = Outputs(pack_engine, n, len(TEN))
    torch.cuda.synchronize()
    pack_engine.forward_u8_views_dev(d_px.data_ptr(), FULL[0], FULL[1], d_mean.data_ptr() if mean is not None else None, n, TEN, *ref.ptrs())
    pack_engine.sync()
    fm0 = pack_engine.layer_output(0, n * len(TEN))
    want_prob, want_top5, want_rows = ref.host()
    assert bits_equal(fm0, vr.nhwc(vr.make_views(px, mean, TEN, h, w)))
    prob, top5, rows = run_resized(pack_engine, list(px), FULL, mean, TEN)
    assert bits_equal(pack_engine.layer_output(0, n * len(TEN)), fm0)
    assert bits_equal(rows, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


# ---------------------------------------------------------------------------------------------- 3. the whole path, tiny network
TINY_FULL = (40, 45)
TINY_SOURCES = [(40, 45), (14, 54), (30, 8), (1, 1), (37, 53), (100, 75), (2, 2)]


class Tiny:
    """The tiny network with the golden parameters, MFMA builder, 130 batch slots; 13 source images of differing sizes under the
    ten-crop views of the 40 x 45 full image, and the reference forward of their 130 host-made inputs (computed once)."""

    def __init__(self, z):
        self.in_chw, self.layers = topo.tiny_model()
        self.params = tiny_params_from_golden(z, self.layers)
        c, h, w = self.in_chw
        rng = np.random.default_rng(79)
        self.images = rr.random_images(rng, 13, c, TINY_SOURCES)
        self.mean = (rng.standard_normal((c,) + TINY_FULL) * 20 + 110).astype(np.float32)
        self.views = engine.ten_crop_views(TINY_FULL[0], TINY_FULL[1], h, w)
        self.eng = self.engine()
        self.rows, self.fm0, self.prob, self.top5 = self.reference(self.images, self.views)

    def engine(self, max_batch=130):
        return make_engine(self.in_chw, self.layers, self.params, max_batch, lut=capi.LUT_MFMA)

    def reference(self, images, views, eng=None):
        """qcnn_forward_host on the host-made inputs, at the slot count of the call under test."""
        eng = eng or self.eng
        _, h, w = self.in_chw
        rows, _ = eng.forward_host(rr.make_views(images, TINY_FULL[0], TINY_FULL[1], self.mean, views, h, w))
        fm0 = eng.layer_output(0, len(images) * len(views))
        prob = vr.mean_views(rows, len(views))
        return rows, fm0, prob, gr.top5(prob)

    def check(self, eng, want=(True, True, True)):
        got = run_resized(eng, self.images, TINY_FULL, self.mean, self.views, want)
        assert got[0] is None if not want[0] else bits_equal(got[0], self.prob)
        assert got[1] is None if not want[1] else np.array_equal(got[1], self.top5)
        assert got[2] is None if not want[2] else bits_equal(got[2], self.rows)


@pytest.fixture(scope="module")
def tiny(golden_tiny):
    t = Tiny(golden_tiny)
    yield t
    t.eng.close()


def test_whole_path_ten_crop(tiny):
    assert np.isfinite(tiny.rows).all()
    prob, top5, rows = run_resized(tiny.eng, tiny.images, TINY_FULL, tiny.mean, tiny.views)
    assert bits_equal(tiny.eng.layer_output(0, 130), tiny.fm0)
    assert bits_equal(rows, tiny.rows)
    assert bits_equal(prob, tiny.prob)
    assert np.array_equal(top5, tiny.top5)


def test_host_convenience_call_is_load_and_forward(tiny):
    """forward_u8_resized_host with its default view: resize, mean, centre crop (BmpImgIO::Load), then the layers."""
    c, h, w = tiny.in_chw
    centre = [((TINY_FULL[0] - h) // 2, (TINY_FULL[1] - w) // 2, 0)]
    want_rows, _, want_prob, want_top5 = tiny.reference(tiny.images, centre)
    prob, top5, rows = tiny.eng.forward_u8_resized_host(tiny.images, TINY_FULL, tiny.mean)
    assert rows.shape == (13, 1, want_rows.shape[1])
    assert bits_equal(rows.reshape(13, -1), want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


def test_one_image_three_views_on_the_few_image_kernels(tiny):
    views = [tiny.views[1], tiny.views[9], (3, 5, 0)]
    images = tiny.images[2:3]                                        # the 30 x 8 source
    want_rows, _, want_prob, want_top5 = tiny.reference(images, views)
    conv = [l for l, ly in enumerate(tiny.layers) if ly["type"] == topo.CONV][0]
    family = tiny.eng.layer_split(conv)
    prob, top5, rows = run_resized(tiny.eng, images, TINY_FULL, tiny.mean, views)
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
    rng = np.random.default_rng(80)
    images = rr.random_images(rng, 130, c, TINY_SOURCES)
    view = [(9, 0, 1)]
    want_rows, _, want_prob, want_top5 = tiny.reference(images, view, eng)
    for _ in range(2):                                               # both sets grow
        prob, top5, rows = run_resized(eng, images, TINY_FULL, tiny.mean, view)
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
    size, one, centre = src.flat.size, src.descs[:1], [tiny.views[4]]
    last_off, last_h, last_w = src.descs[-1]
    bad = [
        # (descs, full, views, src_bytes, a word of the message)
        ([], TINY_FULL, centre, size, "no image"),                                            # n = 0
        (one, TINY_FULL, [], size, "views"),                                                  # no view
        (one, TINY_FULL, [(0, 0, 0)] * 33, size, "views"),                                    # more than QCNN_MAX_VIEWS
        (src.descs * 11, TINY_FULL, centre, size, "batch slots"),                             # 143 slots
        (src.descs + one, TINY_FULL, tiny.views, size, "batch slots"),                        # 140 slots
        (one, (h - 1, fw), centre, size, "smaller than the network input"),
        (one, (fh, w - 1), centre, size, "smaller than the network input"),
        (one, TINY_FULL, [(fh - h + 1, 0, 0)], size, "leaves"),                               # oy + in_h > full_h
        (one, TINY_FULL, [(0, 0, 0), (0, -1, 0)], size, "leaves"),                            # ox = -1
        (one, TINY_FULL, [(0, fw - w + 1, 1)], size, "leaves"),                               # ox + in_w > full_w
        (one, TINY_FULL, [(-1, 0, 0)], size, "leaves"),
        (one + [(0, 0, 5)], TINY_FULL, centre, size, "image 1"),                              # h = 0
        (one + [(0, 5, 0)], TINY_FULL, centre, size, "image 1"),                              # w = 0
        (one + [(0, -3, 5)], TINY_FULL, centre, size, "image 1"),
        ([(0, 46341, 46341)], TINY_FULL, centre, size, "2 GiB"),                              # 3 x 46341^2 bytes > 2^31 - 1
        ([(0, 2 ** 31 - 1, 2 ** 31 - 1)], TINY_FULL, centre, size, "2 GiB"),                  # ... and a product beyond 64 bits
        (src.descs[:-1] + [(last_off + 1, last_h, last_w)], TINY_FULL, centre, size, "leave the source buffer"),   # one byte over
        (src.descs, TINY_FULL, centre, size - 1, "leave the source buffer"),                  # the buffer one byte short
        ([(size + 1, 1, 1)], TINY_FULL, centre, size, "leave the source buffer"),             # offset behind the end
        ([(2 ** 64 - 1, 1, 1)], TINY_FULL, centre, size, "leave the source buffer"),          # offset + bytes wraps around
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
    # full_h < 2 / full_w < 2 on a network whose 1 x 1 input would fit such a full image: the scale divides by full - 1
    small = make_engine((3, 1, 1), [topo.relu()], {}, 8)
    ssrc = Source([np.full((3, 4, 4), 9, np.uint8)], None)
    for full in ((1, 5), (5, 1), (0, 5), (5, -2)):
        out = Outputs(small, 1, 1, want=(True, False, True))
        with pytest.raises(engine.QcnnError) as err:
            ssrc.call(small, full, [(0, 0, 0)], out)
        small.sync()
        assert "at least 2" in str(err.value) and out.untouched()
    out = Outputs(small, 1, 1, want=(True, False, True))
    ssrc.call(small, (2, 2), [(1, 1, 0)], out)                        # the smallest legal full image
    small.sync()
    assert bits_equal(out.host()[0], np.full((1, 3), 9, np.float32))
    small.close()
    fresh = engine.QcnnEngine(0)                                      # no model committed
    with pytest.raises(engine.QcnnError) as err:
        fresh.forward_u8_resized_views_dev(src.d_flat.data_ptr(), size, one, fh, fw, None, [(0, 0, 0)])
    assert "not committed" in str(err.value)
    fresh.close()
