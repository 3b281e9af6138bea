"""CPU tier of the strided source images (QcnnSrcPixels; qcnn_forward_u8_resized_views_strided / _relaxed_views_strided):
tests/layout_ref.py reads every layout back through its descriptor; qcnn_src_bmp on the files resize_ref.write_bmp writes and on
every flavour it must refuse; the host mirror decodes the same files to what the descriptor names; struct and entry points
against the header; the host helpers of engine.py leave the bytes alone.  No GPU."""
import ctypes as C
import os
import re
import struct

import numpy as np
import pytest

import layout_ref as lr
import pyoracle as po
import resize_ref as rr
from conftest import ROOT, pkg

capi = pkg("capi")
engine = pkg("engine")
fileio = pkg("fileio")
HOST_SO = os.path.join(ROOT, "quantized-cnn_amd", "libqcnn_host.so")
BMP_SIZES = [(37, 53), (1, 1), (1, 9), (2, 2)]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- layout_ref itself
@pytest.mark.parametrize("layout", lr.LAYOUTS)
def test_every_layout_reads_back_the_planar_image(layout):
    rng = np.random.default_rng(20)
    images = rr.random_images(rng, len(rr.SOURCES))
    assert [a.shape[1:] for a in images] == rr.SOURCES
    a, b = lr.Buffer(images, layout, lr.const_fill(0x5A)), lr.Buffer(images, layout, lr.rng_fill(21), keep_headers=False)
    assert a.descs == b.descs and np.array_equal(a.sample, b.sample)
    for i, img in enumerate(images):
        ref = np.repeat(img[:1], 3, axis=0) if layout == "grey" else img
        assert np.array_equal(a.refs[i], ref)
        assert np.array_equal(a.read_back(i), ref) and np.array_equal(b.read_back(i), ref), (layout, img.shape)
        d = a.descs[i]
        assert (d.h, d.w) == img.shape[1:] and d.pix_stride >= 1 and min(d.ch_offset) >= 0
    # the samples of the two buffers agree; every other byte is the generator's
    assert np.array_equal(a.flat[a.sample], b.flat[b.sample])
    rest = ~a.sample
    if layout in ("bmp24", "bmp32_topdown"):                    # a keeps the 54 header bytes of every file
        for d, img in zip(a.descs, images):
            f = lr.bmp24_file(img) if layout == "bmp24" else lr.bmp32_topdown_file(img)
            start = min(d.offset, d.offset + (d.h - 1) * d.row_stride) - 54
            assert bytes(a.flat[start:start + 54]) == f[:54] and engine.src_bmp(bytes(a.flat[start:start + len(f)]), start) == d
            rest[start:start + 54] = False
    assert (a.flat[rest] == 0x5A).all()
    assert rest.any() == (layout not in ("planar", "bgr", "rgb", "grey"))
    assert (layout != "bmp24") or a.descs[6].row_stride == -160      # 37 x 53: 159 bytes a row, padded to 160, bottom-up


def test_mixed_layouts_in_one_buffer():
    rng = np.random.default_rng(22)
    images = rr.random_images(rng, 20)
    buf = lr.Buffer(images, lr.LAYOUTS, lr.rng_fill(23))
    assert buf.layouts[:9] == lr.LAYOUTS and buf.layouts[9] == "planar"
    for i in range(20):
        assert np.array_equal(buf.read_back(i), buf.refs[i])
    ends = [int(d.sample_index(3).max()) for d in buf.descs]
    assert ends == sorted(ends) and ends[-1] < buf.flat.size     # the chunks follow each other


# ---------------------------------------------------------------------------------------------- qcnn_src_bmp
def _host_lib():
    lib = C.CDLL(HOST_SO)
    lib.qh_bmp_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")]
    return lib


@pytest.mark.parametrize("size", BMP_SIZES, ids=lambda s: "%dx%d" % s)
def test_src_bmp_names_the_planes_and_the_host_mirror_agrees(size, tmp_path):
    rng = np.random.default_rng(24)
    img = rr.random_images(rng, 1, 3, [size])[0]
    h, w = size
    path = str(tmp_path / "a.bmp")
    rr.write_bmp(path, img)
    raw = open(path, "rb").read()
    stride = (3 * w + 3) & ~3
    for at in (0, 1000003):
        d = engine.src_bmp(raw, at)
        assert d == engine.SrcPixels(at + 54 + (h - 1) * stride, -stride, h, w, 3, (0, 1, 2, 0))
    d = engine.src_bmp(raw, 0)
    assert np.array_equal(np.frombuffer(raw, np.uint8)[d.sample_index(3)], img)
    top = lr.bmp32_topdown_file(img, alpha=77)
    dt = engine.src_bmp(top, 5)
    assert dt == engine.SrcPixels(5 + 54, 4 * w, h, w, 4, (0, 1, 2, 0))
    assert np.array_equal(np.frombuffer(b"\0" * 5 + top, np.uint8)[dt.sample_index(3)], img)
    # the host mirror on the same files: its decode + Strict resize is resize_ref on the planes the descriptor names
    full = 12
    mean = str(tmp_path / "mean.bin")
    fileio.write_bin(mean, np.zeros((3, full, full), np.float32))
    tpath = str(tmp_path / "t.bmp")
    open(tpath, "wb").write(top)
    lib = _host_lib()
    for p in (path, tpath):
        got = np.full((3, full, full), np.nan, np.float32)
        with po._Quiet():
            assert lib.qh_bmp_load(mean.encode(), p.encode(), full, full, 0, got) == 0
        assert same_bits(got, rr.resize(img, full, full))


def _header(w=5, h=4, bpp=24, compression=0, data_off=54, sig=b"BM"):
    return struct.pack("<2sIHHI", sig, 0, 0, 0, data_off) + struct.pack("<IiiHHIIiiII", 40, w, h, 1, bpp, compression, 0, 2835, 2835, 0, 0)


def _refused(data, at=0):
    lib = capi.load()
    out = capi.QcnnSrcPixels()
    C.memset(C.byref(out), 0xEE, C.sizeof(out))
    rc = lib.qcnn_src_bmp(data, len(data), at, C.byref(out))
    untouched = bytes(out) == b"\xEE" * C.sizeof(out)
    return rc != 0 and untouched, rc


def test_src_bmp_refuses_what_the_host_mirror_refuses(tmp_path):
    body = bytes(range(256)) * 2                                  # 5 x 4 at 24 bits: 16 bytes a row, 64 bytes
    good = [_header() + body[:64], _header(h=-4) + body[:64], _header(bpp=32) + body[:80], _header(data_off=60) + body[:70],
            _header(w=1, h=1) + body[:4]]
    for g in good:
        ok, rc = _refused(g)
        assert rc == 0 and not ok
    bad = {
        "signature": _header(sig=b"BN") + body[:64],
        "short header": (_header() + body[:64])[:53],
        "empty": b"",
        "8 bits": _header(bpp=8) + body,
        "16 bits": _header(bpp=16) + body,
        "RLE": _header(compression=1) + body,
        "bitfields": _header(bpp=32, compression=3) + body,
        "zero width": _header(w=0) + body,
        "negative width": _header(w=-5) + body,
        "zero height": _header(h=0) + body,
        "INT32_MIN height": _header(h=-2 ** 31) + body,
        "truncated by one byte": _header() + body[:63],
        "truncated top-down": _header(h=-4) + body[:63],
        "dataOff beyond the file": _header(data_off=2 ** 31) + body[:64],
        "dataOff at the end": _header(data_off=54 + 64) + body[:64],
        "dataOff 2^32 - 1": _header(data_off=2 ** 32 - 1) + body[:64],
        "width x bytes near 2^31": _header(w=2 ** 31 - 1, h=2 ** 31 - 1, bpp=32) + body,
        "width near 2^31 / 3": _header(w=715827883, h=1) + body,
    }
    lib = _host_lib()
    mean = str(tmp_path / "mean.bin")
    fileio.write_bin(mean, np.zeros((3, 12, 12), np.float32))
    for name, data in bad.items():
        ok, rc = _refused(data)
        assert ok, "%s: rc %d, or the descriptor was written" % (name, rc)
        if len(data) < 4096:                                      # ... and the host mirror refuses the same file
            p = str(tmp_path / "bad.bmp")
            open(p, "wb").write(data)
            with po._Quiet():
                assert lib.qh_bmp_load(mean.encode(), p.encode(), 12, 12, 0, np.zeros((3, 12, 12), np.float32)) != 0, name
    ok, _ = _refused(good[0], at=2 ** 64 - 10)                    # file_offset + file_bytes beyond 64 bits
    assert ok
    out = capi.QcnnSrcPixels()
    assert capi.load().qcnn_src_bmp(None, 100, 0, C.byref(out)) != 0 and capi.load().qcnn_src_bmp(good[0], len(good[0]), 0, None) != 0
    with pytest.raises(engine.QcnnError):
        engine.src_bmp(bad["RLE"])
    with pytest.raises(engine.QcnnError) as err:
        engine.pack_bmp_files([good[0], bad["16 bits"]])
    assert "file 1" in str(err.value)


# ---------------------------------------------------------------------------------------------- qcnn_src_planar
def test_src_planar_is_pack_sources_layout():
    rng = np.random.default_rng(25)
    imgs = rr.random_images(rng, 4, 3, [(12, 14), (1, 1), (37, 53), (5, 100)])
    flat, descs = engine.pack_sources(imgs)
    for a, (off, h, w) in zip(imgs, descs):
        d = engine.src_planar(off, h, w, 3)
        assert d == engine.SrcPixels(off, w, h, w, 1, (0, h * w, 2 * h * w, 0))
        assert np.array_equal(flat[d.sample_index(3)], a)
    assert engine.src_planar(7, 3, 2, 1).ch_offset == (0, 0, 0, 0) and engine.src_planar(7, 3, 2, 4).ch_offset == (0, 6, 12, 18)
    assert engine.src_planar(2 ** 64 - 1, 1, 1, 3).offset == 2 ** 64 - 1     # the offset is carried, the call checks it
    for h, w, c in ((0, 5, 3), (5, 0, 3), (-1, 5, 3), (5, 5, 0), (5, 5, 5), (46341, 46341, 3), (2 ** 31 - 1, 2 ** 31 - 1, 1), (2 ** 31 - 1, 1, 2)):
        with pytest.raises(engine.QcnnError):
            engine.src_planar(0, h, w, c)
    lib = capi.load()
    out = capi.QcnnSrcPixels()
    assert lib.qcnn_src_planar(None, 3, C.byref(out)) != 0 and lib.qcnn_src_planar(C.byref(capi.QcnnSrcImage(0, 1, 1)), 3, None) != 0


# ---------------------------------------------------------------------------------------------- header and binding
def test_struct_and_entry_points_match_the_header():
    text = open(capi.HEADER_PATH).read()
    m = re.search(r"typedef struct \{([^}]*)\} QcnnSrcPixels;", text)
    assert m, "QcnnSrcPixels is not in the header"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["uint64_t offset", "int64_t row_stride", "int32_t h, w", "int32_t pix_stride", "int32_t ch_offset[4]"]
    S = capi.QcnnSrcPixels
    assert [f[0] for f in S._fields_] == ["offset", "row_stride", "h", "w", "pix_stride", "ch_offset"]
    assert C.sizeof(S) == 48 and C.alignment(S) == 8
    assert [getattr(S, n).offset for n in ("offset", "row_stride", "h", "w", "pix_stride", "ch_offset")] == [0, 8, 16, 20, 24, 28]
    assert S.ch_offset.size == 16
    lib = capi.load()
    declared = capi.declared_symbols()
    for name, nargs in (("qcnn_forward_u8_resized_views_strided", 13), ("qcnn_forward_u8_relaxed_views_strided", 13), ("qcnn_src_planar", 3),
                        ("qcnn_src_bmp", 4)):
        assert name in declared and hasattr(lib, name) and len(getattr(lib, name).argtypes) == nargs
    assert lib.qcnn_abi_version() == 5 and int(re.search(r"#define QCNN_ABI_VERSION (\d+)", text).group(1)) == 5
    # the library reads the struct as the binding writes it: a descriptor goes through qcnn_src_planar field by field
    out = S()
    assert lib.qcnn_src_planar(C.byref(capi.QcnnSrcImage(123456789012, 7, 9)), 3, C.byref(out)) == 0
    assert (out.offset, out.row_stride, out.h, out.w, out.pix_stride, list(out.ch_offset)) == (123456789012, 9, 7, 9, 1, [0, 63, 126, 0])


# ---------------------------------------------------------------------------------------------- the host helpers
def test_pack_bmp_files_and_pack_interleaved_leave_the_bytes_alone():
    rng = np.random.default_rng(26)
    imgs = rr.random_images(rng, 5, 3, [(12, 14), (1, 1), (37, 53), (2, 2), (5, 100)])
    files = [lr.bmp24_file(a) if k % 2 == 0 else lr.bmp32_topdown_file(a, alpha=k) for k, a in enumerate(imgs)]
    flat, descs = engine.pack_bmp_files(files)
    assert flat.dtype == np.uint8 and flat.ndim == 1 and bytes(flat) == b"".join(files) and len(descs) == 5
    start = 0
    for f, d, a in zip(files, descs, imgs):
        assert d == engine.src_bmp(f, start) and np.array_equal(flat[d.sample_index(3)], a)
        start += len(f)
    for order, chans in (("BGR", (0, 1, 2)), ("RGB", (2, 1, 0))):
        hwc = [np.ascontiguousarray(a.transpose(1, 2, 0)[:, :, list(chans)]) for a in imgs]     # the decoder's arrays
        flat, descs = engine.pack_interleaved(hwc, order)
        assert flat.dtype == np.uint8 and bytes(flat) == b"".join(x.tobytes() for x in hwc)
        for d, a in zip(descs, imgs):
            assert d.ch_offset[:3] == chans and d.pix_stride == 3 and d.row_stride == 3 * a.shape[2]
            assert np.array_equal(flat[d.sample_index(3)], a)                                   # network order B, G, R
    for bad in ([], [imgs[0]], [imgs[0].transpose(1, 2, 0).astype(np.float32)]):
        with pytest.raises((ValueError, TypeError)):
            engine.pack_interleaved(bad)
    with pytest.raises(ValueError):
        engine.pack_interleaved([np.zeros((2, 2, 3), np.uint8)], order="GBR")
    with pytest.raises(ValueError):
        engine.pack_bmp_files([])
