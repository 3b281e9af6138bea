"""CPU tier of the device-side Relaxed resize with a crop-sized mean (qcnn_forward_u8_relaxed_views): tests/relaxed_ref.py — the
restatement the kernel is held to — against qcnn_relaxed_full_size over whole ranges of sizes, bit for bit against the host
mirror's BmpImgIO (Relaxed / Crop) on BMP files, bit for bit against tests/resize_ref.py (which the compiled reference's golden
holds) where Relaxed and Strict coincide; the anchors against qcnn_views_ten_crop; the new entry points and struct in the
header and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyoracle as po
import relaxed_ref as xr
import resize_ref as rr
import views_ref as vr
from conftest import ROOT, pkg

capi = pkg("capi")
engine = pkg("engine")
fileio = pkg("fileio")
HOST_SO = os.path.join(ROOT, "quantized-cnn_amd", "libqcnn_host.so")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---------------------------------------------------------------------------------------------- the size rule
def _size_cases():
    for full in ((12, 14), (12, 12), (14, 14)):
        for h in range(2, 61):
            for w in range(2, 61):
                yield h, w, full
    stride = list(range(2, 1201, 37)) + [255, 256, 257, 333, 375, 500, 1200]
    for h in stride:
        for w in stride:
            yield h, w, (256, 256)
    yield 37, 53, (256, 256)
    yield 5, 100, (256, 256)


def test_size_rule_is_qcnn_relaxed_full_size():
    got, differ = {}, 0
    for h, w, full in _size_cases():
        hf, wf, s = engine.relaxed_full_size(h, w, *full)
        want = xr.full_size(h, w, *full)
        assert (hf, wf) == want[:2] and np.float32(s).tobytes() == want[2].tobytes(), ((h, w), full, (hf, wf, s), want)
        got[(h, w, full)] = (hf, wf)
        differ += (hf, wf) != xr.exact_size(h, w, *full)
    # the seams the float quotient makes: the side that sets the scale one pixel UNDER the nominal size
    assert got[(30, 8, (12, 14))] == (54, 13) and xr.exact_size(30, 8, 12, 14) == (54, 14)
    assert got[(2, 2, (12, 14))] == (13, 13)
    assert got[(37, 53, (256, 256))] == (255, 369) and xr.exact_size(37, 53, 256, 256) == (256, 369)
    assert got[(333, 500, (256, 256))] == (255, 384) and got[(2, 2, (256, 256))] == (255, 255) and got[(5, 100, (256, 256))] == (255, 6312)
    assert differ > 0, "no case differs from the exact-fraction size: the test does not see the float arithmetic"
    small = [k for k in got if k[2] == (12, 14) and k[0] <= 60 and k[1] <= 60]
    assert len(small) == 59 * 59 and sum(got[k] != xr.exact_size(*k[:2], 12, 14) for k in small) == 458
    # the sizes the GPU test's shapes claim
    assert [xr.full_size(h, w, *xr.FULL_HW)[:2] for h, w in xr.SOURCES] == xr.SIZES


def test_size_rule_refusals():
    lib = capi.load()
    hf, wf, s = C.c_int(-7), C.c_int(-7), C.c_float(-7)
    for h, w, fh, fw in ((1, 9, 12, 14), (9, 1, 12, 14), (0, 0, 12, 14), (-3, 5, 12, 14), (9, 9, 1, 14), (9, 9, 12, 1), (9, 9, 0, -2),
                         (2, 2 ** 24, 12, 14),                    # s = 1 / 11: Wf = 11 * (2^24 - 1) + 1
                         (2, 2 ** 31 - 1, 2 ** 31 - 1, 2)):
        assert lib.qcnn_relaxed_full_size(h, w, fh, fw, C.byref(hf), C.byref(wf), C.byref(s)) != 0, (h, w, fh, fw)
        assert (hf.value, wf.value, s.value) == (-7, -7, -7.0)
        with pytest.raises(engine.QcnnError):
            engine.relaxed_full_size(h, w, fh, fw)
    assert lib.qcnn_relaxed_full_size(9, 9, 12, 14, None, C.byref(wf), None) != 0
    assert lib.qcnn_relaxed_full_size(30, 8, 12, 14, C.byref(hf), C.byref(wf), None) == 0 and (hf.value, wf.value) == (54, 13)   # scale may be NULL
    # the largest sides still taken: below 2^24
    big = engine.relaxed_full_size(2, 1525202, 12, 14)            # s = 1 / 11
    assert 2 ** 24 - 8 < big[1] < 2 ** 24 and big[:2] == xr.full_size(2, 1525202, 12, 14)[:2]


# ---------------------------------------------------------------------------------------------- the host mirror
MIRROR_SOURCES = [(37, 53), (30, 8), (14, 54), (2, 2), (5, 100), (24, 27)]


def test_relaxed_ref_is_the_host_mirror(tmp_path):
    lib = C.CDLL(HOST_SO)
    lib.qh_bmp_load.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")]
    rng = np.random.default_rng(21)
    under = 0
    for k, (h, w) in enumerate(MIRROR_SOURCES):
        src = rr.random_images(rng, 1, 3, [(h, w)])[0]
        bmp = str(tmp_path / ("case%d.bmp" % k))
        rr.write_bmp(bmp, src)
        for full in (12, 14):
            hf, wf, _ = xr.full_size(h, w, full, full)
            under += min(hf, wf) < full
            for crop in sorted({5, min(hf, wf)}):                 # a small crop, and the whole smaller side
                mean = (rng.standard_normal((3, crop, crop)) * 20 + 110).astype(np.float32)
                path = str(tmp_path / ("mean_%d_%d_%d.bin" % (k, full, crop)))
                fileio.write_bin(path, mean)
                got = np.full((3, crop, crop), np.nan, np.float32)
                with po._Quiet():
                    rc = lib.qh_bmp_load(path.encode(), bmp.encode(), full, crop, 1, got)
                assert rc == 0
                want = xr.make_views([src], full, full, mean, [xr.CENTRE], crop, crop)[0]
                assert same_bits(got, want), "source %r, full %d, crop %d: %d elements differ" % (
                    (h, w), full, crop, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert under >= 2, "no source whose full size falls under the nominal one"


# ---------------------------------------------------------------------------------------------- where Relaxed is Strict
def test_relaxed_is_strict_where_the_scales_agree():
    """Equal float scales and the nominal size: the relaxed resample is resize_ref.resize bit for bit (resize_ref is held to the
    compiled reference by tests/golden/resize_ref.npz)."""
    rng = np.random.default_rng(22)
    for (h, w), full in (((23, 27), (12, 14)), ((12, 14), (12, 14)), ((34, 40), (12, 14)), ((27, 27), (14, 14)), ((29, 29), (30, 30))):
        hf, wf, s = xr.full_size(h, w, *full)
        assert (hf, wf) == full
        assert s.tobytes() == (np.float32(h - 1) / np.float32(full[0] - 1)).tobytes() == (np.float32(w - 1) / np.float32(full[1] - 1)).tobytes()
        src = rr.random_images(rng, 1, 3, [(h, w)])[0]
        assert same_bits(xr.resize(src, *full), rr.resize(src, *full)), ((h, w), full)
        for a, b in zip(xr.axis(h, hf, s), rr.axis(h, full[0])):
            assert np.array_equal(a, b) and a.dtype == b.dtype
    # and a full-size crop mean window: the views of the Strict call from a full mean are the relaxed ones from its window
    src = rr.random_images(rng, 1, 3, [(23, 27)])[0]
    mean = (rng.standard_normal((3, 12, 14)) * 20 + 110).astype(np.float32)
    want = rr.make_views([src], 12, 14, mean, [(3, 2, 0)], 5, 7)
    got = xr.make_views([src], 12, 14, mean[:, 3:8, 2:9], [(0, 0, 3, 2, 0)], 5, 7)
    assert same_bits(got, want)


def test_resample_element_by_element():
    """The vectorised restatement against the rule written out with scalar np.float32 operations."""
    rng = np.random.default_rng(23)
    f = np.float32
    for (h, w), full in (((30, 8), (12, 14)), ((2, 2), (12, 14)), ((14, 54), (12, 14))):
        px = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
        hf, wf, s = xr.full_size(h, w, *full)
        got = xr.resize(px, *full)
        assert got.shape == (2, hf, wf)
        for y in range(hf):
            yc = f(s * f(y)); y0 = max(0, int(yc)); y1 = min(h - 1, y0 + 1)
            wy0, wy1 = f(f(1) - f(yc - f(y0))), f(f(1) - f(f(y1) - yc))
            for x in range(wf):
                xc = f(s * f(x)); x0 = max(0, int(xc)); x1 = min(w - 1, x0 + 1)
                wx0, wx1 = f(f(1) - f(xc - f(x0))), f(f(1) - f(f(x1) - xc))
                w00, w01, w10, w11 = f(wy0 * wx0), f(wy0 * wx1), f(wy1 * wx0), f(wy1 * wx1)
                den = f(f(f(w00 + w01) + w10) + w11)
                for c in range(2):
                    p = px[c].astype(np.float32)
                    num = f(f(f(f(p[y0, x0] * w00) + f(p[y0, x1] * w01)) + f(p[y1, x0] * w10)) + f(p[y1, x1] * w11))
                    assert got[c, y, x].tobytes() == f(num / den).tobytes(), ((h, w), (c, y, x))


# ---------------------------------------------------------------------------------------------- anchors and views
def test_anchors_resolve_to_the_ten_crop_of_each_full_size():
    ten = engine.ten_crop_anchored()
    assert ten == xr.ten_crop_anchored() and len(ten) == 10
    for hf, wf in xr.SIZES + [(255, 369), (256, 256), (5, 7)]:
        want = engine.ten_crop_views(hf, wf, 5, 7)
        assert [xr.resolve(v, hf, wf, 5, 7) for v in ten] == want == vr.ten_crop(hf, wf, 5, 7)
    # offsets add to the anchor; a view that leaves the image resolves to None
    assert xr.resolve((1, 2, -1, -3, 1), 54, 13, 5, 7) == (23, 3, 1) and xr.resolve((0, 0, 2, 1, 0), 12, 14, 5, 7) == (2, 1, 0)
    assert xr.resolve((2, 2, 1, 0, 0), 12, 14, 5, 7) is None and xr.resolve((0, 0, 0, -1, 0), 12, 14, 5, 7) is None
    assert xr.resolve((1, 1, 0, 0, 0), 54, 13, 5, 14) is None and xr.resolve((1, 1, 0, 0, 0), 12, 14, 5, 14) == (3, 0, 0)
    assert capi.load().qcnn_views_ten_crop_anchored(None) != 0


def test_make_views_crop_mean_and_mirrors():
    rng = np.random.default_rng(24)
    imgs = xr.random_images(rng, len(xr.SOURCES), 3)
    mean = (rng.standard_normal((3, 5, 7)) * 20 + 110).astype(np.float32)
    views = xr.ten_crop_anchored() + [(1, 0, -2, 3, 1), (2, 1, -1, 1, 0)]
    got = xr.make_views(imgs, 12, 14, mean, views, 5, 7)
    assert got.shape == (len(imgs) * 12, 3, 5, 7) and got.dtype == np.float32
    for i, img in enumerate(imgs):
        full = xr.resize(img, 12, 14)
        assert full.shape[1:] == xr.SIZES[i]
        for v, view in enumerate(views):
            oy, ox, flip = xr.resolve(view, full.shape[1], full.shape[2], 5, 7)
            plain = full[:, oy:oy + 5, ox:ox + 7] - mean
            assert same_bits(got[i * 12 + v], plain[..., ::-1] if flip else plain)
        for v in range(5):                                        # a mirrored view is the mirror of the plain view
            assert same_bits(got[i * 12 + 5 + v], got[i * 12 + v][..., ::-1])
    none = xr.make_views(imgs[:2], 12, 14, None, views[:3], 5, 7)
    assert same_bits(none[0], xr.resize(imgs[0], 12, 14)[:, :5, :7])
    # the identity source with the centre anchor: the 8-bit centre crop minus the crop mean
    assert same_bits(xr.make_views(imgs[:1], 12, 14, mean, [xr.CENTRE], 5, 7)[0], imgs[0][:, 3:8, 3:10].astype(np.float32) - mean)


# ---------------------------------------------------------------------------------------------- header and binding
def test_entry_points_and_struct_match_the_header():
    names = capi.declared_symbols()
    lib = capi.load()
    for sym in ("qcnn_forward_u8_relaxed_views", "qcnn_relaxed_full_size", "qcnn_views_ten_crop_anchored"):
        assert sym in names and hasattr(lib, sym), sym
    assert lib.qcnn_abi_version() == 5
    text = open(capi.HEADER_PATH).read()
    assert re.search(r"typedef struct \{ int ay, ax, dy, dx, flip; \} QcnnAnchorView;", text)
    assert [f[0] for f in capi.QcnnAnchorView._fields_] == ["ay", "ax", "dy", "dx", "flip"] and C.sizeof(capi.QcnnAnchorView) == 20
    flat = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    args = lambda name: [a.strip() for a in re.search(r"\bint " + name + r"\s*\((.*?)\);", flat, re.S).group(1).split(",")]
    assert len(args("qcnn_forward_u8_relaxed_views")) == len(lib.qcnn_forward_u8_relaxed_views.argtypes) == 13
    assert args("qcnn_forward_u8_relaxed_views")[8].startswith("const QcnnAnchorView*") and lib.qcnn_forward_u8_relaxed_views.argtypes[8] == C.POINTER(capi.QcnnAnchorView)
    assert len(args("qcnn_relaxed_full_size")) == len(lib.qcnn_relaxed_full_size.argtypes) == 7
    assert len(args("qcnn_views_ten_crop_anchored")) == len(lib.qcnn_views_ten_crop_anchored.argtypes) == 1
