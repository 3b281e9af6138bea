"""CPU tier of the device-side resize (qcnn_forward_u8_resized_views): tests/resize_ref.py — the float32 restatement the kernel is
held to — bit for bit against the compiled reference's BmpImgIO::ReszImg (recorded in tests/golden/resize_ref.npz by
scripts/make_resize_golden.py, and directly where oracle/_ref is built) and against the host mirror's BmpImgIO on the same BMP
files; the seams the GPU test's shapes claim; engine.pack_sources; the new entry point in the header and the binding."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import pyoracle as po
import resize_ref as rr
from conftest import GOLDEN, ROOT, pkg

capi = pkg("capi")
fileio = pkg("fileio")
HOST_SO = os.path.join(ROOT, "quantized-cnn_amd", "libqcnn_host.so")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "resize_ref.npz"))
    return [(int(full), z["src_%02d" % k], z["out_%02d" % k]) for k, full in enumerate(z["full"])]


def test_resize_ref_is_the_compiled_reference_golden(golden):
    assert len(golden) >= 12 and {full for full, _, _ in golden} == {12, 14, 30}
    for k, (full, src, want) in enumerate(golden):
        assert src.dtype == np.uint8 and want.dtype == np.float32 and want.shape == (3, full, full)
        got = rr.resize(src, full, full)
        assert same_bits(got, want), "case %d (%r -> %d): %d elements differ" % (
            k, src.shape[1:], full, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    # the golden cases hold the seams too: a full-size source is the pixel values, the division is not a no-op at a clamped row
    full, src, want = golden[0]
    assert src.shape[1:] == (full, full) and np.array_equal(want, src.astype(np.float32))
    assert any("below" in rr.seam_kinds(s.shape[1], f) for f, s, _ in golden) and any("above_clamp" in rr.seam_kinds(s.shape[1], f) for f, s, _ in golden)


def _bmp_case(tmp_path, k, full, src):
    mean, bmp = str(tmp_path / ("mean%d.bin" % full)), str(tmp_path / ("case%d.bmp" % k))
    fileio.write_bin(mean, np.zeros((3, full, full), np.float32))
    rr.write_bmp(bmp, src)
    return mean, bmp


def test_resize_ref_is_the_host_mirror(golden, tmp_path):
    lib = C.CDLL(HOST_SO)
    lib.qh_bmp_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")]
    for k, (full, src, want) in enumerate(golden):
        mean, bmp = _bmp_case(tmp_path, k, full, src)
        got = np.full((3, full, full), np.nan, np.float32)
        with po._Quiet():
            rc = lib.qh_bmp_load(mean.encode(), bmp.encode(), full, full, 0, got)
        assert rc == 0
        assert same_bits(got, rr.resize(src, full, full)) and same_bits(got, want), "case %d" % k


@pytest.mark.skipif(not po.have_ref(), reason="needs the compiled reference (oracle/_ref)")
def test_resize_ref_is_the_compiled_reference(golden, tmp_path):
    ref = po.RefLib()
    rng = np.random.default_rng(12)
    fresh = [(full, rr.random_images(rng, 1, 3, [hw])[0]) for full, hw in ((12, (14, 54)), (14, (30, 8)), (14, (33, 21)), (30, (2, 2)))]
    for k, (full, src) in enumerate([(f, s) for f, s, _ in golden] + fresh):
        mean, bmp = _bmp_case(tmp_path, k, full, src)
        got = ref.load_bmp(mean, bmp, full, crop=full)[0]
        assert same_bits(got, rr.resize(src, full, full)), "case %d (%r -> %d)" % (k, src.shape[1:], full)


def test_the_gpu_shapes_contain_the_seams_they_claim():
    """Destination 12 x 14: the float coordinate sh * y against the exact rational y * (hs - 1) / (hd - 1)."""
    hd, wd = rr.FULL_HW
    assert (hd, wd) == (12, 14)
    rows = {hs: rr.seam_kinds(hs, hd) for hs, _ in rr.SOURCES}
    cols = {ws: rr.seam_kinds(ws, wd) for _, ws in rr.SOURCES}
    assert rows[14][hd - 1] == "below" and rows[30][hd - 1] == "above_clamp"
    assert cols[54][wd - 1] == "below" and cols[8][wd - 1] == "above_clamp"
    assert any(k == "below" for ks in rows.values() for k in ks) and any(k == "above_clamp" for ks in rows.values() for k in ks)
    assert any(k == "below" for ks in cols.values() for k in ks) and any(k in ("above", "above_clamp") for ks in cols.values() for k in ks)
    # what the seams do to the taps, by hand: 14 rows -> 12: the last coordinate is under 13, tap 0 is row 12 and row 13 weighs 1 - eps
    c, y0, y1, wy0, wy1 = rr.axis(14, 12)
    assert Fraction(float(c[11])) < 13 and (y0[11], y1[11]) == (12, 13) and np.float32(0) < wy0[11] < np.float32(1e-6) and wy1[11] < rr.ONE
    # 30 rows -> 12: the last coordinate is over 29, both taps are row 29, the far weight is over 1 and the weights sum to about 2
    c, y0, y1, wy0, wy1 = rr.axis(30, 12)
    assert Fraction(float(c[11])) > 29 and (y0[11], y1[11]) == (29, 29) and wy1[11] > rr.ONE and wy0[11] < rr.ONE
    px = np.full((1, 30, 8), 200, np.uint8)
    assert rr.resize(px, 12, 14)[0, 11, 3] == np.float32(200)            # ... which the division takes out again
    # a one-pixel axis: scale 0, both taps the same pixel
    c, y0, y1, wy0, wy1 = rr.axis(1, 12)
    assert not c.any() and not y0.any() and not y1.any() and (wy0 == 1).all() and (wy1 == 1).all()
    # a full-size source comes out as the pixel values
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (3, hd, wd), dtype=np.uint8)
    assert same_bits(rr.resize(px, hd, wd), px.astype(np.float32))


def test_resize_ref_element_by_element():
    """The vectorised restatement against the rule written out with scalar np.float32 operations."""
    rng = np.random.default_rng(4)
    f = np.float32
    for (hs, ws), (hd, wd) in (((14, 54), (12, 14)), ((30, 8), (12, 14)), ((5, 7), (6, 9)), ((1, 9), (4, 3))):
        px = rng.integers(0, 256, (2, hs, ws), dtype=np.uint8)
        got = rr.resize(px, hd, wd)
        sh, sw = f(hs - 1) / f(hd - 1), f(ws - 1) / f(wd - 1)
        for y in range(hd):
            yc = f(sh * f(y)); y0 = max(0, int(yc)); y1 = min(hs - 1, y0 + 1)
            wy0, wy1 = f(f(1) - f(yc - f(y0))), f(f(1) - f(f(y1) - yc))
            for x in range(wd):
                xc = f(sw * f(x)); x0 = max(0, int(xc)); x1 = min(ws - 1, x0 + 1)
                wx0, wx1 = f(f(1) - f(xc - f(x0))), f(f(1) - f(f(x1) - xc))
                w00, w01, w10, w11 = f(wy0 * wx0), f(wy0 * wx1), f(wy1 * wx0), f(wy1 * wx1)
                den = f(f(f(w00 + w01) + w10) + w11)
                for c in range(2):
                    p = px[c].astype(np.float32)
                    num = f(f(f(f(p[y0, x0] * w00) + f(p[y0, x1] * w01)) + f(p[y1, x0] * w10)) + f(p[y1, x1] * w11))
                    assert got[c, y, x].tobytes() == f(num / den).tobytes(), ((hs, ws), (c, y, x))


def test_make_views_is_views_ref_on_the_resized_image():
    import views_ref as vr
    rng = np.random.default_rng(5)
    imgs = rr.random_images(rng, 4, 3, [(12, 14), (30, 8), (1, 9), (37, 53)])
    mean = (rng.standard_normal((3, 12, 14)) * 20 + 110).astype(np.float32)
    views = vr.ten_crop(12, 14, 5, 7) + [(3, 2, 1)]
    got = rr.make_views(imgs, 12, 14, mean, views, 5, 7)
    assert got.shape == (44, 3, 5, 7) and got.dtype == np.float32
    for i, img in enumerate(imgs):
        full = rr.resize(img, 12, 14) - mean
        for v, (oy, ox, flip) in enumerate(views):
            crop = full[:, oy:oy + 5, ox:ox + 7]
            assert same_bits(got[i * len(views) + v], crop[..., ::-1] if flip else crop)
    # a full-size source: exactly the 8-bit views
    assert same_bits(rr.make_views(imgs[:1], 12, 14, mean, views, 5, 7), vr.make_views(imgs[0][None], mean, views, 5, 7))
    assert same_bits(rr.make_views(imgs[:1], 12, 14, None, views, 5, 7), vr.make_views(imgs[0][None], None, views, 5, 7))


def test_write_bmp_layout(tmp_path):
    px = np.arange(3 * 2 * 3, dtype=np.uint8).reshape(3, 2, 3)           # width 3: 9 bytes a row, padded to 12
    rr.write_bmp(str(tmp_path / "a.bmp"), px)
    raw = open(tmp_path / "a.bmp", "rb").read()
    assert raw[:2] == b"BM" and len(raw) == 54 + 2 * 12 and int.from_bytes(raw[10:14], "little") == 54
    assert int.from_bytes(raw[18:22], "little") == 3 and int.from_bytes(raw[22:26], "little") == 2 and raw[28] == 24
    bottom = raw[54:66]                                                   # bottom-up: the file's first row is image row 1
    assert list(bottom[:9]) == [px[c, 1, x] for x in range(3) for c in range(3)] and bottom[9:] == b"\0\0\0"


def test_pack_sources():
    engine = pkg("engine")
    rng = np.random.default_rng(6)
    imgs = rr.random_images(rng, 5, 3, [(12, 14), (1, 1), (37, 53), (2, 2), (5, 100)])
    flat, descs = engine.pack_sources(imgs)
    assert flat.dtype == np.uint8 and flat.ndim == 1 and flat.flags["C_CONTIGUOUS"]
    assert flat.size == sum(a.size for a in imgs) and len(descs) == 5
    end = 0
    for a, (off, h, w) in zip(imgs, descs):
        assert (h, w) == a.shape[1:] and off == end                      # back to back, in order
        assert np.array_equal(flat[off:off + a.size].reshape(a.shape), a)
        end = off + a.size
    # a strided view is packed by value; anything but uint8 [C][h][w] with one channel count is refused
    flat2, descs2 = engine.pack_sources([imgs[2][:, ::2, 1::3]])
    assert descs2 == [(0, 19, 18)] and np.array_equal(flat2.reshape(3, 19, 18), imgs[2][:, ::2, 1::3])
    for bad in ([imgs[0].astype(np.float32)], [imgs[0][0]], [imgs[0], imgs[1][:2]], []):
        with pytest.raises((ValueError, TypeError)):
            engine.pack_sources(bad)


def test_entry_point_and_struct_match_the_header():
    assert "qcnn_forward_u8_resized_views" in capi.declared_symbols()
    lib = capi.load()
    assert hasattr(lib, "qcnn_forward_u8_resized_views") and lib.qcnn_abi_version() == 5
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"typedef struct \{ uint64_t offset; int32_t h, w; \} QcnnSrcImage;", text)
    assert [f[0] for f in capi.QcnnSrcImage._fields_] == ["offset", "h", "w"] and C.sizeof(capi.QcnnSrcImage) == 16
    assert len(lib.qcnn_forward_u8_resized_views.argtypes) == 13
