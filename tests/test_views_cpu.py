"""CPU tier of multi-view inference: tests/views_ref.py against the definitions written out with explicit loops, and
qcnn_views_ten_crop (host code of libqcnn_hip.so: needs no device) against views_ref.ten_crop."""
import ctypes as C

import numpy as np
import pytest

import views_ref as vr
from conftest import pkg

capi = pkg("capi")

VIEWS = [(0, 0, 0), (2, 2, 0), (1, 1, 1), (2, 0, 1), (0, 2, 1), (1, 1, 1)]      # both far edges of a 6x7 source, mirrors, a repeat


@pytest.mark.parametrize("with_mean", [True, False])
def test_make_views_element_by_element(with_mean):
    n, ch, hs, ws, h, w = 2, 3, 6, 7, 4, 5
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (n, ch, hs, ws), dtype=np.uint8)
    mean = (rng.standard_normal((ch, hs, ws)) * 20 + 110).astype(np.float32) if with_mean else None
    got = vr.make_views(px, mean, VIEWS, h, w)
    assert got.dtype == np.float32 and got.shape == (n * len(VIEWS), ch, h, w)
    for i in range(n):
        for v, (oy, ox, flip) in enumerate(VIEWS):
            for c in range(ch):
                for y in range(h):
                    for x in range(w):
                        xs = ox + (w - 1 - x if flip else x)
                        want = np.float32(px[i, c, oy + y, xs]) - (mean[c, oy + y, xs] if with_mean else np.float32(0))
                        assert got[i * len(VIEWS) + v, c, y, x].tobytes() == np.float32(want).tobytes(), (i, v, c, y, x)
    assert np.array_equal(vr.nhwc(got)[3, 2, 1, :], got[3, :, 2, 1])


def test_make_views_refuses_a_view_outside_the_source():
    px = np.zeros((1, 1, 6, 7), np.uint8)
    for bad in [(3, 0, 0), (0, 3, 0), (-1, 0, 0), (0, -1, 1)]:
        with pytest.raises(AssertionError):
            vr.make_views(px, None, [bad], 4, 5)


def test_mean_views_is_the_fp32_sequence():
    rng = np.random.default_rng(6)
    p = rng.uniform(0.0, 1.0, (12, 7)).astype(np.float32)
    one = vr.mean_views(p, 1)
    assert one.dtype == np.float32 and one.tobytes() == p.tobytes()              # V = 1: the input's bits
    for V in (2, 3, 4):
        got = vr.mean_views(p, V)
        assert got.dtype == np.float32 and got.shape == (12 // V, 7)
        for i in range(12 // V):
            for c in range(7):
                s = np.float32(p[i * V, c])
                for v in range(1, V):
                    s = np.float32(s + p[i * V + v, c])
                assert got[i, c].tobytes() == np.float32(s / np.float32(V)).tobytes(), (V, i, c)
    # the order matters: 2^24 + 1 + 1 stays 2^24 from the left, the other way round it does not
    p = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
    assert vr.mean_views(p, 3)[0, 0] == np.float32(2.0 ** 24) / np.float32(3)
    assert vr.mean_views(p[::-1].copy(), 3)[0, 0] == np.float32(2.0 ** 24 + 2) / np.float32(3)


def test_ten_crop_reference_by_hand():
    assert vr.ten_crop(40, 45, 31, 31) == [(0, 0, 0), (0, 14, 0), (9, 0, 0), (9, 14, 0), (4, 7, 0),
                                           (0, 0, 1), (0, 14, 1), (9, 0, 1), (9, 14, 1), (4, 7, 1)]


def _library():
    try:
        return capi.load()
    except OSError as e:                       # the HIP runtime it links cannot be loaded on this host
        pytest.skip("libqcnn_hip.so does not load here: %s" % e)


@pytest.mark.parametrize("size", [(256, 256, 227, 227), (40, 45, 31, 31), (31, 31, 31, 31)], ids=lambda s: "%dx%d_%dx%d" % s)
def test_library_ten_crop_matches_the_reference(size):
    lib = _library()
    arr = (capi.QcnnView * 10)()
    assert lib.qcnn_views_ten_crop(*size, arr) == 0
    got = [(v.oy, v.ox, v.flip) for v in arr]
    assert got == vr.ten_crop(*size)
    assert pkg("engine").ten_crop_views(*size) == got
    if size[0] == size[2] and size[1] == size[3]:
        assert all((oy, ox) == (0, 0) for oy, ox, _ in got)
    for oy, ox, flip in got:                   # every view inside the source; the centre is qcnn_forward_u8's crop
        assert 0 <= oy <= size[0] - size[2] and 0 <= ox <= size[1] - size[3] and flip in (0, 1)
    assert got[4][:2] == ((size[0] - size[2]) // 2, (size[1] - size[3]) // 2)


@pytest.mark.parametrize("size", [(30, 45, 31, 31), (40, 30, 31, 31), (226, 226, 227, 227)], ids=lambda s: "%dx%d_%dx%d" % s)
def test_library_ten_crop_refuses_a_source_smaller_than_the_input(size):
    lib = _library()
    arr = (capi.QcnnView * 10)()
    assert lib.qcnn_views_ten_crop(*size, arr) != 0
    assert vr.ten_crop(*size) is None
    with pytest.raises(pkg("engine").QcnnError):
        pkg("engine").ten_crop_views(*size)


def test_view_struct_matches_the_header():
    import re
    text = open(capi.HEADER_PATH).read()
    assert capi.MAX_VIEWS == int(re.search(r"#define\s+QCNN_MAX_VIEWS\s+(\d+)", text).group(1))
    assert re.search(r"typedef struct \{ int oy, ox, flip; \} QcnnView;", text)
    assert [f[0] for f in capi.QcnnView._fields_] == ["oy", "ox", "flip"] and C.sizeof(capi.QcnnView) == 12
