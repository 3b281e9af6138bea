"""TEST INFRASTRUCTURE — numpy float32 restatement of the reference's BmpImgIO::ReszImg (src/BmpImgIO.cc:105-178, Strict) for
qcnn_forward_u8_resized_views (k_pack_u8_resized of quantized-cnn_amd/csrc/qcnn_glue.hip).  No GPU here:
tests/test_resize_cpu.py holds this module bit for bit to the compiled reference (tests/golden/resize_ref.npz, written by
scripts/make_resize_golden.py) and to the host mirror; tests/test_gpu_resize.py holds the kernel to it bit for bit.

Every intermediate is an np.float32 (array): one rounding per operation, (float) conversions of ints.

  sh = (float)(hs-1) / (float)(hd-1)                       sw likewise
  yc = sh * (float)y;  y0 = max(0, (int)yc);  y1 = min(hs-1, y0+1)
  wy0 = 1 - (yc - (float)y0);  wy1 = 1 - ((float)y1 - yc)  columns likewise -> x0, x1, wx0, wx1
  w00 = wy0*wx0; w01 = wy0*wx1; w10 = wy1*wx0; w11 = wy1*wx1
  num = ((p(y0,x0)*w00 + p(y0,x1)*w01) + p(y1,x0)*w10) + p(y1,x1)*w11        p = (float)pixel
  den = ((w00 + w01) + w10) + w11
  out = num / den

  slot      i * V + v = view v of image i; element (c, y, x) of it = out_i[c][oy + y][xs] - mean[c][oy + y][xs] with
            xs = ox + (in_w - 1 - x if flip else x): the views of tests/views_ref.py cut from the resized float image
"""
from __future__ import annotations

import struct
from fractions import Fraction

import numpy as np

ONE = np.float32(1)

# The shapes of tests/test_gpu_resize.py: full image 12 x 14 (full - 1 = 11 and 13 give rounding seams at small sources), and
# the source sizes (h, w) cycled over the images of a batch.
FULL_HW = (12, 14)
SOURCES = [
    (12, 14),      # identity
    (14, 54),      # last row / column just below an integer: tap 0 is one pixel early, the last pixel weighs 1 - eps
    (30, 8),       # last row / column just above an integer: clamped, the far weight above 1
    (1, 1),        # one-pixel source
    (2, 2),        # upscale
    (1, 9),        # one-row source
    (37, 53),      # general downscale, odd row padding in a BMP
    (5, 100),      # very wide source
    (700, 900),    # offsets beyond 16 bits, rows skipped
]


def axis(ns: int, nd: int):
    """Source taps and weights of the nd destination indices along an axis of ns source pixels:
    (coordinate float32 [nd], i0 int32, i1 int32, w0 float32, w1 float32)."""
    assert ns >= 1 and nd >= 2
    s = np.float32(ns - 1) / np.float32(nd - 1)
    c = s * np.arange(nd, dtype=np.int32).astype(np.float32)
    i0 = np.maximum(np.int32(0), c.astype(np.int32))               # (int): truncation
    i1 = np.minimum(np.int32(ns - 1), i0 + np.int32(1))
    w0 = ONE - (c - i0.astype(np.float32))
    w1 = ONE - (i1.astype(np.float32) - c)
    assert c.dtype == w0.dtype == w1.dtype == np.float32 and i0.max() <= ns - 1
    return c, i0, i1, w0, w1


def resize(planes, hd: int, wd: int):
    """uint8 [C][hs][ws] -> float32 [C][hd][wd], the reference's Strict bilinear resize."""
    planes = np.asarray(planes)
    assert planes.dtype == np.uint8 and planes.ndim == 3
    p = planes.astype(np.float32)
    _, y0, y1, wy0, wy1 = axis(planes.shape[1], hd)
    _, x0, x1, wx0, wx1 = axis(planes.shape[2], wd)
    w00, w01 = wy0[:, None] * wx0[None, :], wy0[:, None] * wx1[None, :]
    w10, w11 = wy1[:, None] * wx0[None, :], wy1[:, None] * wx1[None, :]
    tap = lambda ys, xs: p[:, ys][:, :, xs]
    num = ((tap(y0, x0) * w00 + tap(y0, x1) * w01) + tap(y1, x0) * w10) + tap(y1, x1) * w11
    den = ((w00 + w01) + w10) + w11
    out = num / den
    assert out.dtype == np.float32
    return out


def seam_kinds(ns: int, nd: int):
    """Per destination index: how the float32 coordinate s * i relates to the exact i * (ns-1) / (nd-1) where that is an integer —
    'below' (the float lies under it: tap 0 is one pixel early with a weight near 0, tap 1 weighs 1 - eps), 'above' (over it), 'above_clamp' (over it at the
    last pixel: both taps clamp to it and the far weight exceeds 1), None otherwise."""
    c, i0, i1, _, w1 = axis(ns, nd)
    kinds = []
    for i in range(nd):
        exact = Fraction(i * (ns - 1), nd - 1)
        got = Fraction(float(c[i]))
        kind = None
        if exact.denominator == 1 and got != exact:
            if got < exact:
                assert int(i0[i]) == int(exact) - 1
                kind = "below"
            else:
                kind = "above_clamp" if int(i1[i]) == int(i0[i]) and w1[i] > ONE else "above"
        kinds.append(kind)
    return kinds


def write_bmp(path: str, planes) -> None:
    """uint8 [3][h][w] in the order BmpImgIO::LoadBmpImg stores them (B, G, R) -> a 24-bit bottom-up BMP, rows padded to 4 bytes."""
    planes = np.asarray(planes)
    assert planes.dtype == np.uint8 and planes.ndim == 3 and planes.shape[0] == 3
    _, h, w = planes.shape
    stride = (3 * w + 3) & ~3
    rows = np.zeros((h, stride), np.uint8)
    rows[:, :3 * w] = planes.transpose(1, 2, 0).reshape(h, 3 * w)      # the file's pixel order is B, G, R
    data = rows[::-1].tobytes()                                         # bottom-up
    with open(path, "wb") as f:
        f.write(struct.pack("<2sIHHI", b"BM", 54 + len(data), 0, 0, 54))
        f.write(struct.pack("<IiiHHIIiiII", 40, w, h, 1, 24, 0, len(data), 2835, 2835, 0, 0))
        f.write(data)


def make_views(images, full_h, full_w, mean, views, in_h, in_w):
    """images: uint8 arrays [C][h_i][w_i] of differing sizes, mean float32 [C][full_h][full_w] or None, views [(oy, ox, flip)]
    -> float32 [n*V][C][in_h][in_w]: every image resized, the mean subtracted at the full-image position (one float32
    subtraction), then the views cut and mirrored as tests/views_ref.make_views does."""
    C = np.asarray(images[0]).shape[0]
    out = np.empty((len(images), len(views), C, in_h, in_w), np.float32)
    for i, img in enumerate(images):
        full = resize(img, full_h, full_w)
        if mean is not None:
            full = full - np.asarray(mean, np.float32)
        for v, (oy, ox, flip) in enumerate(views):
            assert 0 <= oy <= full_h - in_h and 0 <= ox <= full_w - in_w, "view %r leaves the full image" % ((oy, ox, flip),)
            crop = full[:, oy:oy + in_h, ox:ox + in_w]
            out[i, v] = crop[..., ::-1] if flip else crop
    return out.reshape(len(images) * len(views), C, in_h, in_w)


def random_images(rng, n, C=3, sources=SOURCES):
    """n uint8 images [C][h][w], their sizes cycling over `sources`; a few saturated and a few black pixels in each."""
    imgs = []
    for i in range(n):
        h, w = sources[i % len(sources)]
        a = rng.integers(0, 256, (C, h, w), dtype=np.uint8)
        a.reshape(-1)[::7] = 255
        a.reshape(-1)[3::11] = 0
        imgs.append(a)
    return imgs
