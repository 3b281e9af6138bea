"""Source images read in place under every layout (qcnn_forward_u8_resized_views_strided / _relaxed_views_strided: the strided
instantiations of k_pack_u8_resized / k_pack_u8_relaxed) bit for bit against tests/resize_ref.py / relaxed_ref.py on the PLANAR
images tests/layout_ref.py laid out.

  * the pack kernels per element on a glue-only network (fm[0] read back): source sizes cycling over the 9 of the reference
    modules, layouts over a list of 10 (every layout, bmp24 twice), so that 131 one-view images meet every (size, layout) pair;
    ten-crop over two panel seams with a ragged tail; 32 views; no mean, a random mean, a mean under which no two positions agree;
  * poison: the same samples in two buffers whose other bytes differ everywhere; aliasing: two regions of one frame;
  * planar descriptors through the strided calls against the planar entry points; full-size sources under every layout against
    qcnn_forward_u8_views;
  * BMP files' bytes on the device + the centre view against qcnn_forward_host of what the host mirror decodes from the files;
  * every refusal: non-zero with a message naming the image, outputs and fm[0] untouched, the next good call right."""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest
import torch

import glue_ref as gr
import layout_ref as lr
import pyoracle as po
import relaxed_ref as xr
import resize_ref as rr
import views_ref as vr
from conftest import ROOT, pkg, tiny_params_from_golden
from u8_harness import DEV, Outputs, bits_equal, make_engine, run_sources

pytestmark = pytest.mark.gpu

topo = pkg("topology")
capi = pkg("capi")
engine = pkg("engine")
fileio = pkg("fileio")

PACK_CHW, FULL = (3, 5, 7), rr.FULL_HW            # E = 105: one full 64-element block and a tail of 41; full image 12 x 14
assert xr.FULL_HW == FULL
CYCLE = lr.LAYOUTS + ["bmp24"]                    # 10 entries against 9 source sizes: coprime, 90 images meet every pair
STRICT, RELAXED = "forward_u8_resized_views_strided_dev", "forward_u8_relaxed_views_strided_dev"
SOURCES = {STRICT: rr.SOURCES, RELAXED: xr.SOURCES}
PLANAR = {STRICT: "forward_u8_resized_views_dev", RELAXED: "forward_u8_relaxed_views_dev"}
CENTRE = {STRICT: [((FULL[0] - 5) // 2, (FULL[1] - 7) // 2, 0)], RELAXED: [xr.CENTRE]}
ROOM = {0: (0, 6), 1: (-3, 3), 2: (-6, 0)}        # offsets that keep an anchored 5 x 7 view inside every full size of xr.SIZES


def _many_views(mode, count, seed):
    rng = np.random.default_rng(seed)
    if mode == STRICT:
        return [(7, 7, 1), (0, 7, 0)] + [(int(rng.integers(0, 8)), int(rng.integers(0, 8)), int(rng.integers(0, 2))) for _ in range(count - 2)]
    out = [(2, 2, 0, 0, 1), (0, 2, 6, -6, 0)]
    pairs = list(itertools.product(range(3), repeat=2))
    for k in range(count - 2):
        ay, ax = pairs[k] if k < len(pairs) else (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
        out.append((ay, ax, int(rng.integers(ROOM[ay][0], ROOM[ay][1] + 1)), int(rng.integers(ROOM[ax][0], ROOM[ax][1] + 1)), int(rng.integers(0, 2))))
    return out


VIEWS = {
    STRICT: {"ten_crop": vr.ten_crop(FULL[0], FULL[1], 5, 7), "max_views": _many_views(STRICT, 32, 71), "one_view": [(7, 7, 0)]},
    RELAXED: {"ten_crop": xr.ten_crop_anchored(), "max_views": _many_views(RELAXED, 32, 71), "one_view": [(2, 1, -1, 2, 0)]},
}
COUNTS = {"ten_crop": 27, "max_views": 5, "one_view": 131}     # 270 slots: two panel seams and a ragged tail; 160; 131


def _mean(mode, kind, rng):
    shape = (3,) + tuple(FULL) if mode == STRICT else PACK_CHW
    return {"none": None, "random": (rng.standard_normal(shape) * 20 + 110).astype(np.float32),
            "position": (np.arange(int(np.prod(shape)), dtype=np.float32) * np.float32(1000)).reshape(shape)}[kind]


def _reference(mode, refs, mean, views):
    make = rr.make_views if mode == STRICT else xr.make_views
    return vr.nhwc(make(refs, FULL[0], FULL[1], mean, views, PACK_CHW[1], PACK_CHW[2]))


class Device:
    """A source buffer and a mean on the device in front of a strided engine method."""

    def __init__(self, mode, flat, mean):
        self.mode, self.size = mode, int(flat.size)
        self.d_flat = torch.from_numpy(np.ascontiguousarray(flat)).to(DEV)
        self.d_mean = torch.from_numpy(np.ascontiguousarray(mean)).to(DEV) if mean is not None else None
        torch.cuda.synchronize()

    def call(self, eng, descs, views, out, full=FULL, src_bytes=None, method=None):
        getattr(eng, method or self.mode)(self.d_flat.data_ptr(), self.size if src_bytes is None else src_bytes, descs, full[0], full[1],
                                          self.d_mean.data_ptr() if self.d_mean is not None else None, views, *out.ptrs())


def run_strided(mode, eng, flat, descs, mean, views, want=(True, True, True), full=FULL):
    dev = Device(mode, flat, mean)
    out = Outputs(eng, len(descs), len(views), want)
    dev.call(eng, descs, views, out, full)
    eng.sync()
    return out.host()


@functools.lru_cache(maxsize=None)
def laid_out(mode, n):
    """n images, sizes cycling over the mode's sources and layouts over CYCLE, in one buffer (made once per mode and count)."""
    rng = np.random.default_rng(700 + n + len(mode))
    images = rr.random_images(rng, n, 3, SOURCES[mode])
    return lr.Buffer(images, CYCLE, lr.rng_fill(701 + n))


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
        raise AssertionError("fm[0] differs in %d of %d elements; first at (slot, y, x, c) = %r (image %d of size %r under %s, view %r): got %r, "
                             "expected %r" % (int(diff.sum()), got.size, at, img, buf.refs[img].shape[1:], buf.layouts[img],
                                              views[at[0] % len(views)], got[at], want[at]))


# ---------------------------------------------------------------------------------------------- 1. the pack kernels, per element
def test_131_images_meet_every_size_under_every_layout():
    assert len(CYCLE) == 10 and set(CYCLE) == set(lr.LAYOUTS) and len(lr.LAYOUTS) == 9
    for mode in (STRICT, RELAXED):
        assert len(SOURCES[mode]) == 9
        met = {(SOURCES[mode][i % 9], CYCLE[i % 10]) for i in range(COUNTS["one_view"])}
        assert met == set(itertools.product(SOURCES[mode], lr.LAYOUTS))
    assert ((700, 900), "bgra_pitched") in {(rr.SOURCES[i % 9], CYCLE[i % 10]) for i in range(131)}
    assert ((1, 1), "bmp24") in {(rr.SOURCES[i % 9], CYCLE[i % 10]) for i in range(131)}
    for hf, wf in xr.SIZES:                                         # every anchored view stays inside every image
        assert all(xr.resolve(v, hf, wf, 5, 7) is not None for views in VIEWS[RELAXED].values() for v in views)


@pytest.mark.parametrize("mean_kind", ["none", "random", "position"])
@pytest.mark.parametrize("shape", ["ten_crop", "max_views", "one_view"])
@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_pack_per_element(pack_engine, mode, shape, mean_kind):
    n, views = COUNTS[shape], VIEWS[mode][shape]
    buf = laid_out(mode, n)
    assert n < 90 or {(r.shape[1:], l) for r, l in zip(buf.refs, buf.layouts)} == set(itertools.product(SOURCES[mode], lr.LAYOUTS))
    mean = _mean(mode, mean_kind, np.random.default_rng(702 + n))
    want = _reference(mode, buf.refs, mean, views)
    _, _, rows = run_strided(mode, pack_engine, buf.flat, buf.descs, mean, views, want=(False, False, True))
    _assert_fm0(pack_engine, want, buf, views)
    assert bits_equal(rows, np.maximum(want, np.float32(0)).reshape(n * len(views), -1))     # the ReLU behind it, slot for slot


# ---------------------------------------------------------------------------------------------- 2. poison and aliasing
@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_bytes_that_are_no_sample_are_never_read(pack_engine, mode):
    """Padding, alpha, gaps, the frame around a region, BMP headers: two buffers that agree in the samples alone."""
    buf = laid_out(mode, 27)
    other = np.where(buf.sample, buf.flat, buf.flat ^ np.uint8(0xFF))
    assert (other[~buf.sample] != buf.flat[~buf.sample]).all() and (~buf.sample).sum() > 1000
    assert np.array_equal(other[buf.sample], buf.flat[buf.sample])
    views = VIEWS[mode]["ten_crop"]
    mean = _mean(mode, "random", np.random.default_rng(703))
    want = _reference(mode, buf.refs, mean, views)
    a = run_strided(mode, pack_engine, buf.flat, buf.descs, mean, views)
    _assert_fm0(pack_engine, want, buf, views)
    b = run_strided(mode, pack_engine, other, buf.descs, mean, views)
    _assert_fm0(pack_engine, want, buf, views)
    assert bits_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and bits_equal(a[2], b[2])
    assert bits_equal(a[2], np.maximum(want, np.float32(0)).reshape(270, -1))


@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_two_regions_of_one_frame_in_one_call(pack_engine, mode):
    """Descriptors may alias: two overlapping rectangles of one interleaved frame, a third naming the first again bottom-up
    (the region flipped), a fourth reading one channel of it three times."""
    rng = np.random.default_rng(704)
    fh, fw = 41, 50
    frame = rng.integers(0, 256, (fh, fw, 3), dtype=np.uint8)
    region = lambda y, x, h, w: engine.SrcPixels(3 * (y * fw + x), 3 * fw, h, w, 3, (0, 1, 2, 0))
    a, b = region(3, 5, 20, 30), region(10, 12, 25, 31)
    c = a._replace(offset=a.offset + 19 * 3 * fw, row_stride=-3 * fw)
    g = b._replace(ch_offset=(1, 1, 1, 0))
    cut = lambda y, x, h, w: np.ascontiguousarray(frame[y:y + h, x:x + w].transpose(2, 0, 1))
    refs = [cut(3, 5, 20, 30), cut(10, 12, 25, 31), cut(3, 5, 20, 30)[:, ::-1], np.repeat(cut(10, 12, 25, 31)[1:2], 3, axis=0)]
    views = VIEWS[mode]["ten_crop"]
    mean = _mean(mode, "random", rng)
    want = _reference(mode, refs, mean, views)
    _, _, rows = run_strided(mode, pack_engine, frame.reshape(-1), [a, b, c, g], mean, views)
    assert bits_equal(pack_engine.layer_output(0, 40), want)
    assert bits_equal(rows, np.maximum(want, np.float32(0)).reshape(40, -1))


# ---------------------------------------------------------------------------------------------- 3. equality with the planar paths
@pytest.mark.parametrize("mean_kind", ["none", "random"])
@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_planar_descriptors_return_the_planar_calls_bits(pack_engine, mode, mean_kind):
    rng = np.random.default_rng(705)
    images = rr.random_images(rng, 27, 3, SOURCES[mode])
    views = VIEWS[mode]["ten_crop"]
    mean = _mean(mode, mean_kind, rng)
    prob, top5, rows = run_sources(PLANAR[mode], pack_engine, images, FULL, mean, views)
    fm0 = pack_engine.layer_output(0, 270)
    flat, descs = engine.pack_sources(images)
    got = run_strided(mode, pack_engine, flat, [engine.src_planar(off, h, w, 3) for off, h, w in descs], mean, views)
    assert bits_equal(pack_engine.layer_output(0, 270), fm0)
    assert bits_equal(got[0], prob) and np.array_equal(got[1], top5) and bits_equal(got[2], rows)


@pytest.mark.parametrize("mean_kind", ["none", "random"])
def test_full_size_sources_under_every_layout_are_forward_u8_views(pack_engine, mean_kind):
    n = 27
    rng = np.random.default_rng(706)
    buf = lr.Buffer(list(rng.integers(0, 256, (n, 3) + FULL, dtype=np.uint8)), CYCLE, lr.rng_fill(707))
    assert set(buf.layouts) == set(lr.LAYOUTS)
    px = np.stack(buf.refs)                                          # the planar bytes (a grey image: its plane three times)
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
    prob, top5, rows = run_strided(STRICT, pack_engine, buf.flat, buf.descs, mean, views)
    assert bits_equal(pack_engine.layer_output(0, n * len(views)), fm0)
    assert bits_equal(rows, want_rows) and bits_equal(prob, want_prob) and np.array_equal(top5, want_top5)


# ---------------------------------------------------------------------------------------------- 4. end to end: BMP files' bytes
TINY_FULL, TINY_SOURCES = 40, [(40, 40), (14, 54), (30, 8), (2, 2), (37, 53), (100, 75), (5, 100)]


@pytest.fixture(scope="module")
def tiny(golden_tiny):
    in_chw, layers = topo.tiny_model()
    eng = make_engine(in_chw, layers, tiny_params_from_golden(golden_tiny, layers), 40, lut=capi.LUT_MFMA)
    yield eng
    eng.close()


@pytest.mark.parametrize("n", [3, 13], ids=["three_slots", "thirteen_slots"])
@pytest.mark.parametrize("relaxed", [0, 1], ids=["strict", "relaxed"])
def test_bmp_bytes_and_the_centre_view_are_load_and_forward(tiny, tmp_path, relaxed, n):
    """The files untouched on the device, described by qcnn_src_bmp, against qcnn_forward_host of the inputs the host mirror's
    BmpImgIO::Load makes from the same files (three slots: the few-image kernels)."""
    c, h, w = tiny.in_chw
    assert h == w
    rng = np.random.default_rng(708 + n)
    images = rr.random_images(rng, n, 3, TINY_SOURCES[1:] if relaxed else TINY_SOURCES)
    files = [lr.bmp24_file(a) if k % 3 else lr.bmp32_topdown_file(a, alpha=200 + k) for k, a in enumerate(images)]
    mean = (rng.standard_normal((c, h, w) if relaxed else (c, TINY_FULL, TINY_FULL)) * 20 + 110).astype(np.float32)
    mean_path = str(tmp_path / "mean.bin")
    fileio.write_bin(mean_path, mean)
    lib = C.CDLL(os.path.join(ROOT, "quantized-cnn_amd", "libqcnn_host.so"))
    lib.qh_bmp_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")]
    inputs = np.full((n, c, h, w), np.nan, np.float32)
    for k, f in enumerate(files):
        p = str(tmp_path / ("%d.bmp" % k))
        open(p, "wb").write(f)
        with po._Quiet():
            assert lib.qh_bmp_load(mean_path.encode(), p.encode(), TINY_FULL, h, relaxed, inputs[k:k + 1]) == 0
    assert np.isfinite(inputs).all()
    want_prob, want_top5 = tiny.forward_host(inputs)
    want_fm0 = tiny.layer_output(0, n)
    flat, descs = engine.pack_bmp_files(files)
    assert bytes(flat) == b"".join(files)
    call = tiny.forward_u8_relaxed_host if relaxed else tiny.forward_u8_resized_host
    prob, top5, rows = call(None, (TINY_FULL, TINY_FULL), mean, descs=(flat, descs))
    assert bits_equal(tiny.layer_output(0, n), want_fm0)
    assert bits_equal(prob, want_prob) and np.array_equal(top5, want_top5) and bits_equal(rows.reshape(n, -1), want_prob)
    assert np.isfinite(prob).all() and np.array_equal(top5, gr.top5(prob))


# ---------------------------------------------------------------------------------------------- 5. refusals
def _highest(descs):
    return max(int(d.sample_index(3).max()) for d in descs)


@pytest.mark.parametrize("mode", [STRICT, RELAXED], ids=["strict", "relaxed"])
def test_refusals_enqueue_nothing(pack_engine, mode):
    eng = pack_engine
    rng = np.random.default_rng(709)
    sizes = [(37, 53), (12, 14), (30, 8), (24, 27), (14, 54)]
    buf = lr.Buffer(rr.random_images(rng, 5, 3, sizes), ["bmp24", "bgr", "bgra_pitched", "roi", "planar"], lr.rng_fill(710))
    views = CENTRE[mode]
    mean = _mean(mode, "random", rng)
    want = _reference(mode, buf.refs, mean, views)
    dev = Device(mode, buf.flat, mean)
    size, D = dev.size, buf.descs
    assert _highest(D) == size - 1 and D[0].row_stride == -160      # the last sample of the planar image is the buffer's last byte

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
    bad = [
        # (descs, views, src_bytes, words of the message)
        (D, views, size - 1, ("image 4", "leave the source buffer")),                                   # ... and one byte short
        (swap(1, pix_stride=0), views, size, ("image 1", "pix_stride")),
        (swap(1, pix_stride=-3), views, size, ("image 1", "pix_stride")),
        (swap(2, ch_offset=(0, -1, 2, 0)), views, size, ("image 2", "ch_offset[1]")),
        (swap(3, ch_offset=(0, 1, -2 ** 31, 0)), views, size, ("image 3", "ch_offset[2]")),
        (swap(0, offset=D[0].offset - 160), views, size, ("image 0", "below the source buffer")),       # bottom-up, one row too small
        (swap(0, offset=35 * 160), views, size, ("image 0", "below the source buffer")),                # the lowest byte is -160
        (swap(0, offset=0), views, size, ("image 0", "below the source buffer")),
        (swap(4, offset=D[4].offset + 1), views, size, ("image 4", "leave the source buffer")),         # one byte over
        (swap(1, offset=size), views, size, ("image 1", "leave the source buffer")),
        (swap(1, offset=2 ** 64 - 1), views, huge, ("image 1", "leave the source buffer")),             # offset + extent wraps
        (swap(1, offset=2 ** 64 - 2 ** 20), views, huge, ("image 1", "leave the source buffer")),
        (swap(2, row_stride=2 ** 30), views, huge, ("image 2", "2^31 - 1")),                            # 29 rows of 2^30 bytes
        (swap(2, row_stride=-2 ** 30, offset=2 ** 36), views, huge, ("image 2", "2^31 - 1")),
        (swap(3, pix_stride=2 ** 27), views, huge, ("image 3", "2^31 - 1")),                            # 26 pixels of 2^27 bytes
        (swap(3, ch_offset=(0, 1, 2 ** 31 - 1, 0)), views, huge, ("image 3", "2^31 - 1")),
        (swap(1, row_stride=i64min), views, huge, ("image 1", "2^31 - 1")),
        (swap(1, row_stride=i64max), views, huge, ("image 1", "2^31 - 1")),
        (swap(1, row_stride=i64min, offset=2 ** 64 - 1), views, 2 ** 64 - 1, ("image 1", "2^31 - 1")),
        (swap(1, h=0), views, size, ("image 1", "size")),
        (swap(1, w=0), views, size, ("image 1", "size")),
        (swap(1, h=-5), views, size, ("image 1", "size")),
        (D * 55, views, size, ("batch slots",)),                                                        # 275 slots
        ([], views, size, ("no image",)),
        (D[:1], [], size, ("views",)),
        (D[:1], views * 33, size, ("views",)),
    ]
    if mode == STRICT:
        bad += [(D[:1], [(FULL[0] - 4, 0, 0)], size, ("leaves",)), (D[:1], [(0, -1, 0)], size, ("leaves",))]
    else:
        bad += [(swap(1, h=1, row_stride=0), views, size, ("image 1", "two pixels")), (D[:1], [(3, 1, 0, 0, 0)], size, ("anchors",)),
                (D, [(2, 2, 1, 0, 0)], size, ("image 0", "leaves"))]
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
    good()
    # legal oddities: one row read 12 times (row_stride 0), rows that overlap, a one-pixel image under any row_stride
    one_row = engine.SrcPixels(D[1].offset, 0, 12, 14, 3, (0, 1, 2, 0))
    overlap = engine.SrcPixels(D[1].offset, 3, 12, 14, 3, (0, 1, 2, 0))
    descs = [one_row, overlap] + ([engine.SrcPixels(D[1].offset + 7, i64max, 1, 1, 3, (0, 1, 2, 0))] if mode == STRICT else [])
    at = [d._replace(row_stride=0) if d.h == 1 else d for d in descs]
    refs = [buf.flat[d.sample_index(3)] for d in at]
    out = Outputs(eng, len(descs), 1)
    dev.call(eng, descs, views, out)
    eng.sync()
    assert bits_equal(eng.layer_output(0, len(descs)), _reference(mode, refs, mean, views))


def test_a_network_of_more_than_four_channels_is_refused():
    eng = make_engine((5, 2, 2), [topo.relu()], {}, 8)
    flat = np.arange(200, dtype=np.uint8)
    dev = Device(STRICT, flat, None)
    planar5 = run_sources("forward_u8_resized_views_dev", eng, [flat[:180].reshape(5, 6, 6)], (4, 4), None, [(1, 1, 0)])
    fm0 = eng.layer_output(0, 1)
    assert np.isfinite(planar5[0]).all()
    for mode, views in ((STRICT, [(1, 1, 0)]), (RELAXED, [xr.CENTRE])):
        out = Outputs(eng, 1, 1)
        with pytest.raises(engine.QcnnError) as err:
            dev.call(eng, [engine.SrcPixels(0, 6, 6, 6, 1, (0, 36, 72, 108))], views, out, full=(4, 4), method=mode)
        eng.sync()
        assert "image 0" in str(err.value) and "4 channels" in str(err.value), str(err.value)
        assert out.untouched() and bits_equal(eng.layer_output(0, 1), fm0)
    eng.close()
    fresh = engine.QcnnEngine(0)                                    # no model committed
    with pytest.raises(engine.QcnnError) as err:
        fresh.forward_u8_resized_views_strided_dev(dev.d_flat.data_ptr(), 200, [engine.SrcPixels(0, 6, 6, 6, 1, (0, 36, 72, 0))], 4, 4, None, [(0, 0, 0)])
    assert "not committed" in str(err.value)
    fresh.close()
