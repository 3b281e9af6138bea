"""YCbCr frames read in place (qcnn_forward_u8_resized_views_yuv / _relaxed_views_yuv: the QkSrcYuv / QkRelaxedYuv instantiations
of k_pack_u8_resized / k_pack_u8_relaxed) bit for bit against tests/resize_ref.py / relaxed_ref.py on the planar B, G, R images
tests/yuv_ref.to_bgr makes of the frames, and against the existing strided call on those images in the same engine.

  * the pack kernels per element on a glue-only network (fm[0] read back): source sizes cycling over the 9 of the reference
    modules, layouts over the 16 of yuv_ref.KINDS (131 one-view images and 27 ten-crop images meet every pair), the three
    matrices, half the frames made from pictures and half uniformly random (these clamp); ten-crop over two panel seams with a
    ragged tail; 32 views; no mean, a random mean, a mean under which no two positions agree;
  * poison: the same samples in two buffers whose other bytes differ everywhere;
  * full-size 4:4:4 JFIF frames with neutral chroma through the strict call against qcnn_forward_u8_views on the luma plane;
  * NV12 frames end to end on the tiny model against qcnn_forward_host, and streamed from host memory with labels;
  * every refusal: non-zero with a message naming the image and the plane, outputs and fm[0] untouched, the next good call right."""
import functools

import numpy as np
import pytest
import torch

import glue_ref as gr
import relaxed_ref as xr
import resize_ref as rr
import stream_ref as sr
import views_ref as vr
import yuv_ref as yr
from conftest import pkg, tiny_params_from_golden
from test_yuv_cpu import GPU_SEED, GPU_SETS
from u8_harness import DEV, Outputs, bits_equal, make_engine

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
engine = pkg("engine")

PACK_CHW, FULL = (3, 5, 7), rr.FULL_HW            # E = 105: one full 64-element block and a tail of 41; full image 12 x 14
assert xr.FULL_HW == FULL
STRICT, RELAXED = "forward_u8_resized_views_yuv_dev", "forward_u8_relaxed_views_yuv_dev"
STRIDED = {STRICT: "forward_u8_resized_views_strided_dev", RELAXED: "forward_u8_relaxed_views_strided_dev"}
SOURCES = {STRICT: rr.SOURCES, RELAXED: xr.SOURCES}
CENTRE = {STRICT: [((FULL[0] - 5) // 2, (FULL[1] - 7) // 2, 0)], RELAXED: [xr.CENTRE]}
ROOM = {0: (0, 6), 1: (-3, 3), 2: (-6, 0)}        # offsets that keep an anchored 5 x 7 view inside every full size of xr.SIZES


def _many_views(mode, count, seed):
    rng = np.random.default_rng(seed)
    if mode == STRICT:
        return [(7, 7, 1), (0, 7, 0)] + [(int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 2))) for _ in range(count - 2)]
    out = [(2, 2, 0, 0, 1), (0, 2, 6, -6, 0)]
    for _ in range(count - 2):
        ay, ax = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        out.append((ay, ax, int(rng.integers(ROOM[ay][0], ROOM[ay][1] + 1)), int(rng.integers(ROOM[ax][0], ROOM[ax][1] + 1)), int(rng.integers(0, 2))))
    return out


VIEWS = {
    STRICT: {"ten_crop": vr.ten_crop(FULL[0], FULL[1], 5, 7), "max_views": _many_views(STRICT, 32, 71), "one_view": [(7, 7, 0)]},
    RELAXED: {"ten_crop": xr.ten_crop_anchored(), "max_views": _many_views(RELAXED, 32, 71), "one_view": [(2, 1, -1, 2, 0)]},
}
SETS = dict(zip(("one_view", "ten_crop", "max_views"), GPU_SETS))      # 131 slots; 270: two panel seams and a ragged tail; 160


def _mean(mode, kind, rng):
    shape = (3,) + tuple(FULL) if mode == STRICT else PACK_CHW
    return {"none": None, "random": (rng.standard_normal(shape) * 20 + 110).astype(np.float32),
            "position": (np.arange(int(np.prod(shape)), dtype=np.float32) * np.float32(1000)).reshape(shape)}[kind]


def _reference(mode, refs, mean, views):
    make = rr.make_views if mode == STRICT else xr.make_views
    return vr.nhwc(make(refs, FULL[0], FULL[1], mean, views, PACK_CHW[1], PACK_CHW[2]))


class Device:
    """A source buffer and a mean on the device in front of an engine method."""

    def __init__(self, mode, flat, mean):
        self.mode, self.size = mode, int(flat.size)
        self.d_flat = torch.from_numpy(np.ascontiguousarray(flat)).to(DEV)
        self.d_mean = torch.from_numpy(np.ascontiguousarray(mean)).to(DEV) if mean is not None else None
        torch.cuda.synchronize()

    def call(self, eng, descs, views, out, full=FULL, src_bytes=None, method=None):
        getattr(eng, method or self.mode)(self.d_flat.data_ptr(), self.size if src_bytes is None else src_bytes, descs, full[0], full[1],
                                          self.d_mean.data_ptr() if self.d_mean is not None else None, views, *out.ptrs())


def run(mode, eng, flat, descs, mean, views, want=(True, True, True), method=None):
    dev = Device(mode, flat, mean)
    out = Outputs(eng, len(descs), len(views), want)
    dev.call(eng, descs, views, out, method=method)
    eng.sync()
    return out.host()


@functools.lru_cache(maxsize=None)
def laid_out(mode, shape):
    """The frames of one image count in one buffer (made once per mode and count; tests/test_yuv_cpu.py looks at the same)."""
    n, start = SETS[shape]
    frames, kinds, matrices = yr.test_frames(SOURCES[mode], n, start, GPU_SEED + n)
    return yr.Buffer(frames, kinds, matrices, yr.rng_fill(901 + n))


@pytest.fixture(scope="module")
def pack_engine():
    eng = make_engine(PACK_CHW, [topo.relu()], {}, 270)
    yield eng
    eng.close()


def _assert_fm0(eng, want, buf, views):
    got = eng.layer_output(0, want.shape[0])
    if not bits_equal(got, want):
        diff = got.view(np.uint32) != want.view(np.uint32)
        at = tuple(int(v) for v in np.argwhere(diff)[0])
        img = at[0] // len(views)
        raise AssertionError("fm[0] differs in %d of %d elements; first at (slot, y, x, c) = %r (image %d of size %r as %s under %s, view %r): got "
                             "%r, expected %r" % (int(diff.sum()), got.size, at, img, buf.refs[img].shape[1:], buf.kinds[img], buf.matrices[img],
                                                  views[at[0] % len(views)], got[at], want[at]))


# ---------------------------------------------------------------------------------------------- 1. the pack kernels, per element
@pytest.mark.parametrize("mean_kind", ["none", "random", "position"])
@pytest.mark.parametrize("shape", ["ten_crop", "max_views", "one_view"])
@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_pack_per_element(pack_engine, mode, shape, mean_kind):
    views = VIEWS[mode][shape]
    buf = laid_out(mode, shape)
    n = len(buf.descs)
    assert n * len(views) == {"one_view": 131, "ten_crop": 270, "max_views": 160}[shape]
    mean = _mean(mode, mean_kind, np.random.default_rng(902 + n))
    want = _reference(mode, buf.refs, mean, views)
    _, _, rows = run(mode, pack_engine, buf.flat, buf.descs, mean, views, want=(False, False, True))
    _assert_fm0(pack_engine, want, buf, views)
    assert bits_equal(rows, np.maximum(want, np.float32(0)).reshape(n * len(views), -1))     # the ReLU behind it, slot for slot
    # ... and the existing strided call on the converted planar images, in the same engine
    flat, planar = engine.pack_sources(buf.refs)
    prob, top5, rows = run(mode, pack_engine, buf.flat, buf.descs, mean, views)
    got = run(mode, pack_engine, flat, [engine.src_planar(off, h, w, 3) for off, h, w in planar], mean, views, method=STRIDED[mode])
    _assert_fm0(pack_engine, want, buf, views)
    assert bits_equal(got[0], prob) and np.array_equal(got[1], top5) and bits_equal(got[2], rows)


# ---------------------------------------------------------------------------------------------- 2. poison
@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_bytes_that_are_no_sample_are_never_read(pack_engine, mode):
    """Row padding, the unused half of a chroma row's padding, the frame around a region: two buffers that agree in the Y, Cb, Cr
    samples alone."""
    buf = laid_out(mode, "ten_crop")
    other = np.where(buf.sample, buf.flat, buf.flat ^ np.uint8(0xFF))
    assert (other[~buf.sample] != buf.flat[~buf.sample]).all() and (~buf.sample).sum() > 1000
    assert np.array_equal(other[buf.sample], buf.flat[buf.sample])
    views = VIEWS[mode]["ten_crop"]
    mean = _mean(mode, "random", np.random.default_rng(903))
    want = _reference(mode, buf.refs, mean, views)
    a = run(mode, pack_engine, buf.flat, buf.descs, mean, views)
    _assert_fm0(pack_engine, want, buf, views)
    b = run(mode, pack_engine, other, buf.descs, mean, views)
    _assert_fm0(pack_engine, want, buf, views)
    assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and bits_equal(a[2], b[2])
    assert bits_equal(a[2], np.maximum(want, np.float32(0)).reshape(270, -1))


# ---------------------------------------------------------------------------------------------- 3. full-size grey 4:4:4 frames
@pytest.mark.parametrize("mean_kind", ["none", "random"])
def test_full_size_grey_444_frames_are_forward_u8_views_on_the_luma_plane(pack_engine, mean_kind):
    n = 27
    rng = np.random.default_rng(906)
    luma = rng.integers(0, 256, (n,) + FULL, dtype=np.uint8)
    grey = np.full(FULL, 128, np.uint8)
    kinds = [("I444", "I444_pitched")[i % 2] for i in range(n)]
    buf = yr.Buffer([(y, grey, grey) for y in luma], kinds, ["JFIF"] * n, yr.rng_fill(907))
    px = np.ascontiguousarray(np.repeat(luma[:, None], 3, axis=1))   # the luma plane three times
    assert np.array_equal(np.stack(buf.refs), px)
    views = VIEWS[STRICT]["ten_crop"]
    mean = _mean(STRICT, mean_kind, rng)
    d_px = torch.from_numpy(px).to(DEV)
    d_mean = torch.from_numpy(mean).to(DEV) if mean is not None else None
    ref = Outputs(pack_engine, n, len(views))
    torch.cuda.synchronize()
    pack_engine.forward_u8_views_dev(d_px.data_ptr(), FULL[0], FULL[1], d_mean.data_ptr() if mean is not None else None, n, views, *ref.ptrs())
    pack_engine.sync()
    fm0 = pack_engine.layer_output(0, n * len(views))
    want_prob, want_top5, want_rows = ref.host()
    assert bits_equal(fm0, vr.nhwc(vr.make_views(px, mean, views, 5, 7)))
    prob, top5, rows = run(STRICT, pack_engine, buf.flat, buf.descs, mean, views)
    assert bits_equal(pack_engine.layer_output(0, n * len(views)), fm0)
    assert bits_equal(rows, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


# ---------------------------------------------------------------------------------------------- 4. end to end: NV12 frames
TINY_FULL, TINY_SOURCES = 40, [(40, 40), (14, 54), (30, 8), (2, 2), (37, 53), (100, 75), (5, 100)]


@pytest.fixture(scope="module")
def tiny(golden_tiny):
    in_chw, layers = topo.tiny_model()
    eng = make_engine(in_chw, layers, tiny_params_from_golden(golden_tiny, layers), 40, lut=capi.LUT_MFMA)
    yield eng
    eng.close()


def _nv12(rng, n, sizes, matrix):
    """n NV12 frames as a decoder wrote them (bytes), their sizes and the B, G, R images the network sees."""
    frames, refs, hw = [], [], []
    for i in range(n):
        h, w = sizes[i % len(sizes)]
        f = yr.like_image(rng.integers(0, 256, (3, h, w), dtype=np.uint8), matrix, (1, 1)) if i % 2 else yr.random_frame(rng, h, w, (1, 1))
        buf = yr.Buffer([f], ["NV12"], [matrix], yr.rng_fill(int(rng.integers(1 << 30))))
        frames.append(bytes(buf.flat))
        refs.append(buf.refs[0])
        hw.append((h, w))
    return frames, hw, refs


def _float_inputs(refs, relaxed, mean, in_hw):
    """What BmpImgIO::Load makes of the planar images: resize, mean, centre crop (numpy, the reference modules)."""
    if relaxed:
        return xr.make_views(refs, TINY_FULL, TINY_FULL, mean, [xr.CENTRE], in_hw, in_hw)
    o = (TINY_FULL - in_hw) // 2
    return rr.make_views(refs, TINY_FULL, TINY_FULL, mean, [(o, o, 0)], in_hw, in_hw)


@pytest.mark.parametrize("n", [3, 13], ids=["three_slots", "thirteen_slots"])
@pytest.mark.parametrize("relaxed", [0, 1], ids=["strict", "relaxed"])
def test_nv12_frames_and_the_centre_view_are_convert_load_and_forward(tiny, relaxed, n):
    c, h, w = tiny.in_chw
    assert h == w
    rng = np.random.default_rng(908 + n)
    matrix = "BT601" if relaxed else "JFIF"
    frames, hw, refs = _nv12(rng, n, TINY_SOURCES[1:] if relaxed else TINY_SOURCES, matrix)
    mean = (rng.standard_normal((c, h, w) if relaxed else (c, TINY_FULL, TINY_FULL)) * 20 + 110).astype(np.float32)
    inputs = np.ascontiguousarray(_float_inputs(refs, relaxed, mean, h))
    want_prob, want_top5 = tiny.forward_host(inputs)
    want_fm0 = tiny.layer_output(0, n)
    flat, descs = engine.pack_yuv_frames(frames, "NV12", hw, matrix)
    assert bytes(flat) == b"".join(frames)
    call = tiny.forward_u8_relaxed_host if relaxed else tiny.forward_u8_resized_host
    prob, top5, rows = call(None, (TINY_FULL, TINY_FULL), mean, descs=(flat, descs))
    assert bits_equal(tiny.layer_output(0, n), want_fm0)
    assert bits_equal(prob, want_prob) and np.array_equal(top5, want_top5) and bits_equal(rows.reshape(n, -1), want_prob)
    assert np.isfinite(prob).all() and np.array_equal(top5, gr.top5(prob))


@pytest.mark.parametrize("mode", ["strict", "relaxed"])
def test_streamed_nv12_batches_are_the_device_call_and_count_hits(tiny, mode):
    c, h, w = tiny.in_chw
    rng = np.random.default_rng(911)
    relaxed = mode == "relaxed"
    sizes = TINY_SOURCES[1:] if relaxed else TINY_SOURCES
    mean = (rng.standard_normal((c, h, w) if relaxed else (c, TINY_FULL, TINY_FULL)) * 20 + 110).astype(np.float32)
    views = xr.ten_crop_anchored()[3:6] if relaxed else [(0, 0, 0), (TINY_FULL - h, TINY_FULL - w, 1), ((TINY_FULL - h) // 2, (TINY_FULL - w) // 2, 0)]
    batches, want = [], []
    call = tiny.forward_u8_relaxed_host if relaxed else tiny.forward_u8_resized_host
    for n in (13, 5, 9):                                            # three ragged batches of three views: 39, 15, 27 slots
        frames, hw, _ = _nv12(rng, n, sizes, "BT709")
        batches.append(engine.pack_yuv_frames(frames, "NV12", hw, "BT709"))
        want.append(call(None, (TINY_FULL, TINY_FULL), mean, views, descs=batches[-1]))
    classes = want[0][0].shape[1]
    labels = [np.where(rng.random(len(d)) < 0.6, t[:, int(rng.integers(0, 5))], rng.integers(0, classes, len(d))).astype(np.uint16)
              for (_, d), (_, t, _) in zip(batches, want)]
    labels[1] = None                                                # a batch that is not counted
    prob, top5, rows, hits = tiny.forward_u8_host_batches(batches, (TINY_FULL, TINY_FULL), mean, views, mode, labels, want=(True, True, True))
    for b in range(3):
        assert bits_equal(prob[b], want[b][0]) and np.array_equal(top5[b], want[b][1]) and bits_equal(rows[b], want[b][2]), b
    assert np.array_equal(hits, sr.hits5_batches([t for _, t, _ in want], labels)) and int(hits.sum()) > 0
    # evaluate_u8 on the same frames: the same counts
    frames, hw, _ = _nv12(np.random.default_rng(912), 20, sizes, "JFIF")
    flat, descs = engine.pack_yuv_frames(frames, "NV12", hw, "JFIF")
    _, t5, _ = call(None, (TINY_FULL, TINY_FULL), mean, views, descs=(flat[:descs[13].y_offset].copy(), descs[:13]))
    lab = np.concatenate([t5[:, 0], np.zeros(7, np.uint16)]).astype(np.uint16)
    res = tiny.evaluate_u8(frames, lab, (TINY_FULL, TINY_FULL), mean, views, mode, batch_images=13, yuv=("NV12", hw, "JFIF"))
    assert res["n"] == 20 and res["hits"][0] >= 13 and sum(res["hits"]) <= 20 * 5


# ---------------------------------------------------------------------------------------------- 5. refusals
@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_refusals_enqueue_nothing(pack_engine, mode):
    eng = pack_engine
    rng = np.random.default_rng(909)
    sizes = [(37, 53), (12, 14), (30, 8), (24, 27), (14, 54)]
    kinds = ["I420_bottom_up", "NV12", "YUY2_pitched", "NV12_roi", "I444"]
    frames = [yr.random_frame(rng, h, w, yr.sub_of(k)) for (h, w), k in zip(sizes, kinds)]
    buf = yr.Buffer(frames, kinds, ["JFIF", "BT601", "BT709", "JFIF", "BT601"], yr.rng_fill(910))
    views = CENTRE[mode]
    mean = _mean(mode, "random", rng)
    want = _reference(mode, buf.refs, mean, views)
    dev = Device(mode, buf.flat, mean)
    size, D = dev.size, buf.descs
    assert int(D[4].sample_index()[2].max()) == size - 1 and D[0].c_row_stride == -27    # the last Cr sample is the buffer's last byte

    def good(src_bytes=None):
        out = Outputs(eng, 5, 1)
        dev.call(eng, D, views, out, src_bytes=src_bytes)
        eng.sync()
        assert bits_equal(eng.layer_output(0, 5), want) and bits_equal(out.host()[2], np.maximum(want, np.float32(0)).reshape(5, -1))

    good()
    good(src_bytes=size)                                            # exactly fitting ...
    huge = 2 ** 40                                                  # a claimed size: nothing is read on refusal
    i64min, i64max = -2 ** 63, 2 ** 63 - 1
    swap = lambda k, **kw: D[:k] + [D[k]._replace(**kw)] + D[k + 1:]
    i444 = D[4]
    bad = [
        # (descs, views, src_bytes, words of the message)
        (D, views, size - 1, ("image 4", "Cr", "leaves the source buffer")),                             # ... and one byte short
        (swap(4, cb_offset=i444.cr_offset, cr_offset=i444.cb_offset), views, size - 1, ("image 4", "Cb", "leaves the source buffer")),
        (swap(4, y_offset=i444.cr_offset, cr_offset=i444.y_offset), views, size - 1, ("image 4", "luma", "leaves the source buffer")),
        (swap(0, cb_offset=18 * 27 - 1), views, size, ("image 0", "Cb", "below the source buffer")),       # bottom-up: its lowest byte is -1
        (swap(0, cr_offset=0), views, size, ("image 0", "Cr", "below the source buffer")),
        (swap(0, y_offset=35 * 53), views, size, ("image 0", "luma", "below the source buffer")),
        (swap(1, sub_x=2), views, size, ("image 1", "sub_x 2")),
        (swap(1, sub_y=-1), views, size, ("image 1", "sub_y -1")),
        (swap(2, c_pix_stride=0), views, size, ("image 2", "c_pix_stride")),
        (swap(2, y_pix_stride=-2), views, size, ("image 2", "y_pix_stride")),
        (swap(3, matrix=3), views, size, ("image 3", "matrix 3")),
        (swap(3, matrix=-1), views, size, ("image 3", "matrix -1")),
        (swap(1, cr_offset=D[1].y_offset + 2 ** 31 - 1), views, huge, ("image 1", "luma", "Cr", "2^31 - 1")),     # a span of 2^31 - 1 over the planes
        (swap(1, y_row_stride=2 ** 28), views, huge, ("image 1", "luma", "2^31 - 1")),                  # 11 rows of 2^28 bytes
        (swap(2, c_row_stride=-2 ** 27, cb_offset=2 ** 36, cr_offset=2 ** 36), views, huge, ("image 2", "Cb", "2^31 - 1")),
        (swap(1, y_row_stride=i64min), views, huge, ("image 1", "luma", "2^31 - 1")),
        (swap(1, c_row_stride=i64max), views, huge, ("image 1", "Cb", "2^31 - 1")),
        (swap(1, cb_offset=2 ** 64 - 1), views, huge, ("image 1", "Cb", "leaves the source buffer")),   # offset + extent wraps
        (swap(1, y_offset=2 ** 64 - 2 ** 20), views, 2 ** 64 - 1, ("image 1", "luma", "2^31 - 1")),             # inside, and far from its chroma
        (swap(1, h=0), views, size, ("image 1", "size")),
        (swap(1, w=-5), views, size, ("image 1", "size")),
        (D * 55, views, size, ("batch slots",)),                                                        # 275 slots
        ([], views, size, ("no image",)),
        (D[:1], [], size, ("views",)),
        (D[:1], views * 33, size, ("views",)),
    ]
    if mode == STRICT:
        bad += [(D[:1], [(FULL[0] - 4, 0, 0)], size, ("leaves",))]
    else:
        bad += [(swap(1, h=1), views, size, ("image 1", "two pixels")), (D, [(2, 2, 1, 0, 0)], size, ("image 0", "leaves"))]
    for descs, vws, src_bytes, words in bad:
        out = Outputs(eng, 5, 1)
        with pytest.raises(engine.QcnnError) as err:
            dev.call(eng, descs, vws, out, src_bytes=src_bytes)
        eng.sync()
        assert all(word in str(err.value) for word in words), (words, str(err.value))
        assert out.untouched(), "a refused call wrote an output (%r)" % (words,)
        assert bits_equal(eng.layer_output(0, 5), want), "a refused call wrote the input map (%r)" % (words,)
    with pytest.raises(engine.QcnnError) as err:                    # NULL source buffer
        getattr(eng, mode)(None, size, D, FULL[0], FULL[1], None, views)
    assert "NULL" in str(err.value)
    # the Python wrappers: a mixed list of SrcPixels and SrcYuv
    pixels = engine.SrcPixels(0, 14, 12, 14, 1, (0, 168, 336, 0))
    host = eng.forward_u8_relaxed_host if mode == RELAXED else eng.forward_u8_resized_host
    with pytest.raises(ValueError) as err:
        host(None, FULL, mean, views, descs=(buf.flat, [D[1], pixels]))
    assert "not both" in str(err.value)
    with pytest.raises(ValueError) as err:
        eng.forward_u8_host_batches([(buf.flat, D), (buf.flat, [pixels])], FULL, mean, views, "relaxed" if mode == RELAXED else "strict")
    assert "not both" in str(err.value)
    # the streamed call names batch, image and plane, and leaves the host outputs alone
    outs = [(np.full((5, 105), np.nan, np.float32), np.full((5, 5), 0xFFFF, np.uint16), None) for _ in range(2)]
    hits = np.full(5, 77, np.uint64)
    with pytest.raises(engine.QcnnError) as err:
        eng.forward_u8_host_batches_into([(buf.flat, D), (buf.flat[:size - 1], D)], FULL, dev.d_mean.data_ptr(), views,
                                         "relaxed" if mode == RELAXED else "strict", outs, [np.zeros(5, np.uint16)] * 2, hits)
    assert all(word in str(err.value) for word in ("batch 1", "image 4", "Cr")), str(err.value)
    assert all(np.isnan(p).all() and (t == 0xFFFF).all() for p, t, _ in outs) and (hits == 77).all()
    assert bits_equal(eng.layer_output(0, 5), want)
    good()
    # legal oddities: one luma row read 12 times under chroma rows that overlap, a one-pixel frame under any row stride
    one_row = D[1]._replace(y_row_stride=0, c_row_stride=2)
    descs = [one_row] + ([engine.SrcYuv(D[1].y_offset + 7, D[1].cb_offset + 2, D[1].cr_offset + 2, i64max, i64min, 1, 1, 1, 2, 1, 1, 2)] if mode == STRICT else [])
    refs = []
    for d in descs:
        at = d._replace(y_row_stride=0, c_row_stride=0).sample_index() if d.h == 1 else d.sample_index()
        y, cb, cr = buf.flat[at]
        refs.append(yr.to_bgr(y, cb, cr, (0, 0), yr.MATRIX_NAMES[d.matrix]))       # the planes as replicated: 4:4:4 of themselves
    out = Outputs(eng, len(descs), 1)
    dev.call(eng, descs, views, out)
    eng.sync()
    assert bits_equal(eng.layer_output(0, len(descs)), _reference(mode, refs, mean, views))


def test_a_network_of_four_channels_and_an_empty_context_are_refused():
    eng = make_engine((4, 2, 2), [topo.relu()], {}, 8)
    flat = np.arange(200, dtype=np.uint8)
    dev = Device(STRICT, flat, None)
    d = engine.src_yuv_frame("I444", 0, 6, 6)
    for mode, views in ((STRICT, [(1, 1, 0)]), (RELAXED, [xr.CENTRE])):
        out = Outputs(eng, 1, 1)
        with pytest.raises(engine.QcnnError) as err:
            dev.call(eng, [d], views, out, full=(4, 4), method=mode)
        eng.sync()
        assert "image 0" in str(err.value) and "3 channels" in str(err.value), str(err.value)
        assert out.untouched()
    eng.close()
    fresh = engine.QcnnEngine(0)                                    # no model committed
    with pytest.raises(engine.QcnnError) as err:
        fresh.forward_u8_resized_views_yuv_dev(dev.d_flat.data_ptr(), 200, [d], 4, 4, None, [(0, 0, 0)])
    assert "not committed" in str(err.value)
    with pytest.raises(engine.QcnnError) as err:
        fresh.forward_u8_host_batches_into([(flat, [d])], (4, 4), None, [(0, 0, 0)], "strict", [(None, None, None)])
    assert "not committed" in str(err.value)
    fresh.close()
