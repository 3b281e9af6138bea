"""CPU tier of the YCbCr source frames (QcnnSrcYuv; qcnn_forward_u8_resized_views_yuv / _relaxed_views_yuv): the integer
conversion of tests/yuv_ref.py against its fixed points and the real-number formula on all 2^24 triples; every layout read back
through its descriptor; qcnn_src_yuv_frame through ctypes against yuv_ref.place; and the inputs of tests/test_gpu_yuv.py
themselves: every mistake of yuv_ref.WRONG shows in what the network sees of them, and they clamp where they should.  No GPU."""
import ctypes as C
import itertools
import re

import numpy as np
import pytest

import relaxed_ref as xr
import resize_ref as rr
import yuv_ref as yr
from conftest import pkg

capi = pkg("capi")
engine = pkg("engine")
SIZES = sorted(set(rr.SOURCES + xr.SOURCES + [(1, 1), (2, 2), (37, 53), (5, 100)]))
# what tests/test_gpu_yuv.py lays out per mode: (count, phase of the kind cycle) — 131 one-view images, 27 ten-crop, 5 x 32 views
GPU_SETS = [(131, 0), (27, 131), (5, 158)]
GPU_SEED = 900


# ---------------------------------------------------------------------------------------------- the conversion
def test_fixed_points_of_the_conversion():
    grey = np.arange(256, dtype=np.uint8).reshape(16, 16)
    mid = np.full((16, 16), 128, np.uint8)
    bgr = yr.to_bgr(grey, mid, mid, (0, 0), "JFIF")
    assert all(np.array_equal(p, grey) for p in bgr)                 # JFIF: Cb = Cr = 128 returns B = G = R = Y
    for m in ("BT601", "BT709"):
        bgr = yr.to_bgr(grey, mid, mid, (0, 0), m).reshape(3, 256)
        assert (bgr[:, :17] == 0).all() and (bgr[:, 235:] == 255).all()          # 16 -> 0, 235 -> 255, beyond: clamped
        assert (bgr[:, 17] == 1).all() and (bgr[:, 234] == 254).all() and (np.diff(bgr.astype(int), axis=1) >= 0).all()
    for m in yr.MATRIX_NAMES:                                        # the extremes clamp, on both sides, in every channel
        lo, hi = np.zeros((1, 1), np.uint8), np.full((1, 1), 255, np.uint8)
        b, g, r = yr.to_bgr(hi, hi, lo, (0, 0), m).reshape(3)
        assert b == 255 and r <= 76
        b, g, r = yr.to_bgr(lo, lo, hi, (0, 0), m).reshape(3)
        assert b == 0 and r >= 178 and g == 0
        b, g, r = yr.to_bgr(lo, lo, lo, (0, 0), m).reshape(3)
        assert b == 0 and r == 0 and g >= 77                        # no blue, no red: green is what is left
        assert not yr.unclamped(hi, hi, lo, (0, 0), m).any() and yr.unclamped(mid[:1, :1], mid[:1, :1], mid[:1, :1], (0, 0), m).all()


@pytest.mark.parametrize("matrix", yr.MATRIX_NAMES)
def test_all_triples_stay_within_one_of_the_real_formula(matrix):
    cb, cr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst, peak = 0.0, 0
    for y in range(256):
        Y = np.full((256, 256), y, np.uint8)
        got = yr.to_bgr(Y, cb, cr, (0, 0), matrix).astype(np.float64)
        want = np.clip(np.rint(yr.real_bgr(Y, cb, cr, matrix)), 0, 255)
        worst = max(worst, float(np.abs(got - want).max()))
        peak = max(peak, int(np.abs(yr._sums(Y, cb, cr, (0, 0), matrix)).max()) + 32768)
    assert worst <= 1.0, worst
    assert peak <= 3.6e7, peak                                       # far inside 32 bits


# ---------------------------------------------------------------------------------------------- the layouts
@pytest.mark.parametrize("kind", yr.KINDS)
def test_every_kind_reads_back_its_frames(kind):
    rng = np.random.default_rng(30)
    sub = yr.sub_of(kind)
    frames = [yr.random_frame(rng, h, w, sub) for h, w in SIZES]
    n = len(frames)
    a = yr.Buffer(frames, [kind] * n, ["BT601"] * n, lambda k: np.full(k, 0x5A, np.uint8))
    b = yr.Buffer(frames, [kind] * n, ["BT601"] * n, yr.rng_fill(31))
    assert a.descs == b.descs and np.array_equal(a.sample, b.sample) and np.array_equal(a.flat[a.sample], b.flat[b.sample])
    assert (a.flat[~a.sample] == 0x5A).all()
    for i, (Y, Cb, Cr) in enumerate(frames):
        h, w = Y.shape
        d = a.descs[i]
        assert (d.h, d.w, d.sub_y, d.sub_x, d.matrix) == (h, w) + sub + (1,)
        cy, cx = np.arange(h)[:, None] >> sub[0], np.arange(w)[None, :] >> sub[1]
        for buf in (a, b):
            got = buf.read_back(i)
            assert np.array_equal(got[0], Y) and np.array_equal(got[1], Cb[cy, cx]) and np.array_equal(got[2], Cr[cy, cx]), (kind, h, w)
        assert np.array_equal(a.refs[i], yr.to_bgr(Y, Cb, Cr, sub, "BT601"))
    # every byte of a tight planar or semi-planar frame of even sides is a sample; a pitch, a region, an odd side leave bytes over
    assert (~a.sample).any() == (kind not in ("I420", "YV12", "I444", "I420_bottom_up")), kind          # tight planes: no byte is left over
    even = yr.Buffer([yr.random_frame(rng, 12, 14, sub)], [kind], ["JFIF"], yr.rng_fill(32))
    assert even.sample.all() == ("_" not in kind or kind == "I420_bottom_up"), kind
    if kind == "I420_bottom_up":
        assert all(d.y_row_stride < 0 and d.c_row_stride < 0 for d in a.descs)


def _frame(fmt, off, h, w, pitch, matrix):
    out = capi.QcnnSrcYuv()
    rc = capi.load().qcnn_src_yuv_frame(capi.YUV_FORMATS.get(fmt, fmt), off, h, w, pitch, capi.YUV_MATRICES.get(matrix, matrix), C.byref(out))
    return rc, engine.SrcYuv(*(int(getattr(out, f)) for f in engine.SrcYuv._fields))


@pytest.mark.parametrize("fmt", yr.FORMATS)
def test_the_constructor_makes_the_descriptors_of_place(fmt):
    rng = np.random.default_rng(33)
    zero = engine.SrcYuv(*([0] * 12))
    for (h, w), matrix in zip(SIZES, itertools.cycle(yr.MATRIX_NAMES)):
        frame = yr.random_frame(rng, h, w, yr.SUB[fmt])
        for kind, off in ((fmt, 0), (fmt, 12345), (fmt + "_pitched", 7)):
            size, want = yr.place(frame, kind, matrix)
            want = want._replace(y_offset=want.y_offset + off, cb_offset=want.cb_offset + off, cr_offset=want.cr_offset + off)
            pitch = want.y_row_stride if kind.endswith("_pitched") else 0
            assert _frame(fmt, off, h, w, pitch, matrix) == (0, want), (kind, h, w)
            assert engine.src_yuv_frame(fmt, off, h, w, pitch, matrix) == want
            assert int(want.sample_index().max()) < off + size
        tight = yr.place(frame, fmt)[1].y_row_stride
        assert tight == 1 or _frame(fmt, 0, h, w, tight - 1, matrix) == (1, zero)   # a pitch smaller than a row (0 means tight)
        assert _frame(fmt, 0, h, w, -tight, matrix) == (1, zero)
    lib = capi.load()
    assert lib.qcnn_src_yuv_frame(capi.YUV_FORMATS[fmt], 0, 4, 4, 0, 0, None) == 1  # NULL out
    for bad in ((fmt, 0, 0, 4, 0, "JFIF"), (fmt, 0, 4, 0, 0, "JFIF"), (fmt, 0, -1, 4, 0, "JFIF"), (fmt, 0, 4, 4, 0, 3), (fmt, 0, 4, 4, 0, -1),
                (7, 0, 4, 4, 0, "JFIF"), (-1, 0, 4, 4, 0, "JFIF"), (fmt, 0, 2, 2, 2 ** 31, "JFIF"), (fmt, 0, 2 ** 16, 2 ** 16, 0, "JFIF"),
                (fmt, 2 ** 64 - 8, 4, 4, 0, "JFIF"), (fmt, 0, 3, 3, 2 ** 62, "JFIF")):
        assert _frame(*bad) == (1, zero), bad
    with pytest.raises(engine.QcnnError):
        engine.src_yuv_frame(fmt, 0, 0, 4)
    with pytest.raises(ValueError):
        engine.src_yuv_frame("RGB", 0, 4, 4)


def test_pack_yuv_frames_leaves_the_bytes_alone():
    rng = np.random.default_rng(34)
    sizes = [(37, 53), (2, 2), (5, 100)]
    bufs = [yr.Buffer([yr.random_frame(rng, h, w, (1, 1))], ["NV12"], ["BT709"], yr.rng_fill(35 + k)) for k, (h, w) in enumerate(sizes)]
    frames = [bytes(b.flat) for b in bufs]
    flat, descs = engine.pack_yuv_frames(frames, "NV12", sizes, "BT709")
    assert bytes(flat) == b"".join(frames) and flat.flags.writeable
    off = 0
    for b, d, f in zip(bufs, descs, frames):
        assert d == b.descs[0]._replace(y_offset=b.descs[0].y_offset + off, cb_offset=b.descs[0].cb_offset + off, cr_offset=b.descs[0].cr_offset + off)
        assert np.array_equal(flat[d.sample_index()], b.read_back(0))
        off += len(f)
    with pytest.raises(engine.QcnnError) as err:
        engine.pack_yuv_frames([frames[0], frames[1][:-1]], "NV12", sizes[:2])
    assert "frame 1" in str(err.value)
    cut = engine.split_batches(frames, [1, 2, 3], 2, 1, yuv=("NV12", sizes, "BT709"))
    assert [len(d) for _, d, _ in cut] == [2, 1] and cut[1][2].tolist() == [3] and bytes(cut[0][0]) == frames[0] + frames[1]
    assert isinstance(cut[0][1][0], engine.SrcYuv) and cut[1][1][0] == descs[2]._replace(
        y_offset=descs[2].y_offset - off + len(frames[2]), cb_offset=descs[2].cb_offset - off + len(frames[2]),
        cr_offset=descs[2].cr_offset - off + len(frames[2]))
    pixels = engine.SrcPixels(0, 3, 1, 1, 3, (0, 1, 2, 0))
    with pytest.raises(ValueError):                                  # one kind per call
        engine._is_yuv([descs[0], pixels])
    assert engine._is_yuv(descs) and not engine._is_yuv([pixels])


def test_struct_and_entry_points_against_the_header():
    text = open(capi.HEADER_PATH).read()
    body = re.search(r"typedef struct \{([^}]*)\} QcnnSrcYuv;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.split(None, 1)[1].split(",")]
    assert names == [f for f, _ in capi.QcnnSrcYuv._fields_] == list(engine.SrcYuv._fields)
    assert C.sizeof(capi.QcnnSrcYuv) == 72 and C.sizeof(capi.QcnnU8YuvBatch) == C.sizeof(capi.QcnnU8Batch)
    for name, value in list(capi.YUV_MATRICES.items()) + list(capi.YUV_FORMATS.items()):
        assert re.search(r"QCNN_YUV_%s = %d\b" % (name, value), text), name
    table = re.findall(r"QCNN_YUV_(\w+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)\s+(\d+)", text)
    assert {n: tuple(int(v) for v in row) for n, *row in table} == yr.MATRICES
    assert text.count("#define QCNN_ABI_VERSION 5") == 1
    lib = capi.load()
    for fn in ("qcnn_src_yuv_frame", "qcnn_forward_u8_resized_views_yuv", "qcnn_forward_u8_relaxed_views_yuv",
               "qcnn_forward_u8_resized_host_batches_yuv", "qcnn_forward_u8_relaxed_host_batches_yuv"):
        assert fn in capi.declared_symbols() and hasattr(lib, fn)


# ---------------------------------------------------------------------------------------------- the inputs of the GPU tests
@pytest.mark.parametrize("mode", ["strict", "relaxed"])
def test_gpu_inputs_meet_every_pair_and_tell_every_mistake_apart(mode):
    sources = rr.SOURCES if mode == "strict" else xr.SOURCES
    resize = (lambda img: rr.resize(img, *rr.FULL_HW)) if mode == "strict" else (lambda img: xr.resize(img, *xr.FULL_HW))
    met, seen = set(), {name: 0 for name in yr.WRONG}
    like, rand = [], []
    for n, start in GPU_SETS:
        frames, kinds, matrices = yr.test_frames(sources, n, start, GPU_SEED + n)
        met |= {(f[0].shape, k) for f, k in zip(frames, kinds)}
        assert n < 6 or set(matrices) == set(yr.MATRIX_NAMES)
        for i, ((Y, Cb, Cr), kind, matrix) in enumerate(zip(frames, kinds, matrices)):
            (rand if i % 2 else like).append((int(yr.unclamped(Y, Cb, Cr, yr.sub_of(kind), matrix).sum()), Y.size))
            if Y.size > 40000 and n > 27:
                continue                                             # the large frames are looked at once, in the small sets
            want = resize(yr.to_bgr(Y, Cb, Cr, yr.sub_of(kind), matrix))
            for name, convert in yr.WRONG.items():                   # network-visible: the resized image differs
                seen[name] += int(not np.array_equal(resize(convert(Y, Cb, Cr, yr.sub_of(kind), matrix)), want))
    assert met == set(itertools.product(sources, yr.KINDS))          # 131 + 27 images meet all 9 x 16 pairs
    assert all(count >= 5 for count in seen.values()), seen
    # of the pixels of the like_image frames at least half convert with no channel clamped, of the random ones at most half
    share = lambda rows: sum(a for a, _ in rows) / sum(b for _, b in rows)
    assert share(like) >= 0.5 and share(rand) <= 0.5, (share(like), share(rand))
    assert min(a / b for a, b in like if b >= 64) >= 0.5 and max(a / b for a, b in rand if b >= 64) <= 0.5      # and frame by frame


@pytest.mark.parametrize("matrix", yr.MATRIX_NAMES)
def test_every_mistake_is_visible_at_37_by_53(matrix):
    rng = np.random.default_rng(36)
    for kind, maker in (("NV12", "like"), ("I420_pitched", "random"), ("YUY2", "like")):
        sub = yr.sub_of(kind)
        frame = yr.like_image(rng.integers(0, 256, (3, 37, 53), dtype=np.uint8), matrix, sub) if maker == "like" else yr.random_frame(rng, 37, 53, sub)
        want = yr.to_bgr(*frame, sub, matrix)
        for name, convert in yr.WRONG.items():
            assert not np.array_equal(convert(*frame, sub, matrix), want), (kind, name)
