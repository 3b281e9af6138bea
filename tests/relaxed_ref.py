"""TEST INFRASTRUCTURE — numpy float32 / float64 restatement of the reference's Relaxed resize with a crop-sized mean
(BmpImgIO::ReszImg's Relaxed branch, CropImg, RmMeanImg: src/BmpImgIO.cc:56-64,105-178) for qcnn_forward_u8_relaxed_views
(k_pack_u8_relaxed of quantized-cnn_amd/csrc/qcnn_glue.hip).  No GPU here.  The compiled reference exposes only Strict through
oracle/, so this module is tied to the reference in two ways (tests/test_relaxed_cpu.py): bit for bit to the host mirror
(qh_bmp_load(..., relaxed = 1, ...), whose source restates src/BmpImgIO.cc:124-131 line by line), and bit for bit to
tests/resize_ref.py — which IS held to the compiled reference — where the two modes coincide.  tests/test_gpu_relaxed.py holds
the kernel to this module bit for bit.

  size      sh = (float)(h-1) / (float)(full_h-1);  sw likewise;  s = min(sh, sw)
            Hf = (int)((double)((float)(h-1) / s) + 1e-7) + 1;    Wf likewise          float quotient, double sum, truncation
  resample  resize_ref's sequence with s given, as both scales: yc = s * (float)Y, taps, four weight products, left-to-right
            sums, one division — every intermediate an np.float32
  anchor    a view (ay, ax, dy, dx, flip) of an image whose full size is Hf x Wf has its corner at (a(ay, Hf - in_h) + dy,
            a(ax, Wf - in_w) + dx), a(0, r) = 0, a(1, r) = r // 2 (CropImg's corner), a(2, r) = r
  slot      i * V + v = view v of image i; element (c, y, x) of it = R_i[c][oy + y][ox + xl] - mean[c][y][xl] with
            xl = in_w - 1 - x if flip else x: the crop, the crop-sized mean at the view-local position, then the mirror
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import resize_ref as rr

ONE = rr.ONE
EPS = np.float64(0.0000001)                       # kEpsilon

# The shapes of tests/test_gpu_relaxed.py: nominal full size 12 x 14, the source sizes (h, w) cycled over the images of a
# batch, and the full size the reference's arithmetic gives each of them.
FULL_HW = (12, 14)
SOURCES = [
    (12, 14),      # identity: scale 1 on both axes
    (30, 8),       # the width sets the scale and comes out UNDER the nominal size: 54 x 13 (exact 54 x 14)
    (2, 2),        # upscale, both sides one over the nominal height: 13 x 13
    (37, 53),      # general downscale
    (14, 54),
    (5, 100),      # very wide
    (700, 900),    # offsets beyond 16 bits, rows skipped
    (500, 375),    # portrait: the width sets the scale
    (24, 27),
]
SIZES = [(12, 14), (54, 13), (13, 13), (12, 16), (12, 45), (12, 273), (12, 15), (18, 14), (12, 14)]


def full_size(h: int, w: int, full_h: int, full_w: int):
    """(Hf, Wf, s) of the reference's Relaxed branch; s an np.float32."""
    assert h >= 2 and w >= 2 and full_h >= 2 and full_w >= 2
    sh = np.float32(h - 1) / np.float32(full_h - 1)
    sw = np.float32(w - 1) / np.float32(full_w - 1)
    s = min(sh, sw)
    qh, qw = np.float32(h - 1) / s, np.float32(w - 1) / s
    assert type(s) is np.float32 and type(qh) is np.float32 and type(qw) is np.float32
    return int(np.float64(qh) + EPS) + 1, int(np.float64(qw) + EPS) + 1, s


def exact_size(h: int, w: int, full_h: int, full_w: int):
    """The size the same rule gives in exact arithmetic (no epsilon, no rounding)."""
    s = min(Fraction(h - 1, full_h - 1), Fraction(w - 1, full_w - 1))
    return int(Fraction(h - 1) / s) + 1, int(Fraction(w - 1) / s) + 1


def axis(ns: int, nd: int, s):
    """resize_ref.axis with the scale GIVEN: taps and weights of the nd destination indices along an axis of ns source pixels.
    The source tap is clamped to the last pixel as the kernel clamps it (it cannot exceed it while the sizes are below 2^23)."""
    assert type(s) is np.float32 and ns >= 1 and nd >= 1
    c = s * np.arange(nd, dtype=np.int32).astype(np.float32)
    i0 = np.maximum(np.int32(0), c.astype(np.int32))               # (int): truncation
    assert i0.max() <= ns - 1
    i1 = np.minimum(np.int32(ns - 1), i0 + np.int32(1))
    w0 = ONE - (c - i0.astype(np.float32))
    w1 = ONE - (i1.astype(np.float32) - c)
    assert c.dtype == w0.dtype == w1.dtype == np.float32
    return c, i0, i1, w0, w1


def resample(planes, s, hd: int, wd: int):
    """uint8 [C][hs][ws] -> float32 [C][hd][wd] by the reference's bilinear sequence with s as the scale of both axes."""
    planes = np.asarray(planes)
    assert planes.dtype == np.uint8 and planes.ndim == 3
    p = planes.astype(np.float32)
    _, y0, y1, wy0, wy1 = axis(planes.shape[1], hd, s)
    _, x0, x1, wx0, wx1 = axis(planes.shape[2], wd, s)
    w00, w01 = wy0[:, None] * wx0[None, :], wy0[:, None] * wx1[None, :]
    w10, w11 = wy1[:, None] * wx0[None, :], wy1[:, None] * wx1[None, :]
    tap = lambda ys, xs: p[:, ys][:, :, xs]
    num = ((tap(y0, x0) * w00 + tap(y0, x1) * w01) + tap(y1, x0) * w10) + tap(y1, x1) * w11
    den = ((w00 + w01) + w10) + w11
    out = num / den
    assert out.dtype == np.float32
    return out


def resize(planes, full_h: int, full_w: int):
    """uint8 [C][h][w] -> float32 [C][Hf][Wf]: the Relaxed resize towards full_h x full_w."""
    planes = np.asarray(planes)
    hf, wf, s = full_size(planes.shape[1], planes.shape[2], full_h, full_w)
    return resample(planes, s, hf, wf)


def anchor(a: int, room: int) -> int:
    assert a in (0, 1, 2) and room >= 0
    return (0, room // 2, room)[a]


def resolve(view, hf: int, wf: int, in_h: int, in_w: int):
    """(ay, ax, dy, dx, flip) on an image of full size hf x wf -> (oy, ox, flip) as tests/views_ref.py takes it; None when the
    view leaves the image."""
    ay, ax, dy, dx, flip = view
    if hf < in_h or wf < in_w:
        return None
    oy, ox = anchor(ay, hf - in_h) + dy, anchor(ax, wf - in_w) + dx
    if oy < 0 or ox < 0 or oy > hf - in_h or ox > wf - in_w:
        return None
    return oy, ox, 1 if flip else 0


def ten_crop_anchored():
    """The order of views_ref.ten_crop: four corners, the centre, then the same five mirrored."""
    plain = [(0, 0, 0, 0, 0), (0, 2, 0, 0, 0), (2, 0, 0, 0, 0), (2, 2, 0, 0, 0), (1, 1, 0, 0, 0)]
    return plain + [v[:4] + (1,) for v in plain]


CENTRE = (1, 1, 0, 0, 0)


def make_views(images, full_h, full_w, mean_crop, views, in_h, in_w):
    """images: uint8 arrays [C][h_i][w_i] of differing sizes, mean_crop float32 [C][in_h][in_w] or None, views
    [(ay, ax, dy, dx, flip)] -> float32 [n*V][C][in_h][in_w]: every image resized by its one scale, each view cropped at the
    corner it resolves to on THAT image, the mean subtracted (one float32 subtraction, view-local position), then mirrored."""
    C = np.asarray(images[0]).shape[0]
    out = np.empty((len(images), len(views), C, in_h, in_w), np.float32)
    for i, img in enumerate(images):
        full = resize(img, full_h, full_w)
        for v, view in enumerate(views):
            at = resolve(view, full.shape[1], full.shape[2], in_h, in_w)
            assert at is not None, "view %r leaves image %d's full size %r" % (view, i, full.shape[1:])
            oy, ox, flip = at
            crop = full[:, oy:oy + in_h, ox:ox + in_w]
            if mean_crop is not None:
                crop = crop - np.asarray(mean_crop, np.float32)
            out[i, v] = crop[..., ::-1] if flip else crop
    return out.reshape(len(images) * len(views), C, in_h, in_w)


def random_images(rng, n, C=3, sources=SOURCES):
    return rr.random_images(rng, n, C, sources)
