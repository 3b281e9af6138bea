"""TEST INFRASTRUCTURE — numpy references for multi-view inference from 8-bit images (qcnn_forward_u8_views; k_pack_u8_views and
k_mean_views of quantized-cnn_amd/csrc/qcnn_glue.hip).  No GPU here: tests/test_views_cpu.py checks this module against the
definitions with explicit loops, tests/test_gpu_views.py holds the kernels to it bit for bit.

  view      (oy, ox, flip): the in_h x in_w crop whose top-left corner is (oy, ox) in the source image, mirrored left-right
            when flip is not 0
  slot      i * V + v = view v of image i (image-major)
  element   (c, y, x) of a slot = float32(px[i][c][oy + y][xs]) - mean[c][oy + y][xs], xs = ox + (in_w - 1 - x if flip else x);
            no mean = 0.  One convert and one float32 subtraction: exact in numpy's float32 as on the device.
  mean      s = p[i*V + 0]; s = s + p[i*V + v] for v = 1 .. V-1; s / float32(V) — float32, one rounding per operation
"""
from __future__ import annotations

import numpy as np


def make_views(px, mean, views, in_h, in_w):
    """px uint8 [n][C][Hs][Ws], mean float32 [C][Hs][Ws] or None, views [(oy, ox, flip)] -> float32 [n*V][C][in_h][in_w]."""
    px = np.asarray(px)
    assert px.dtype == np.uint8 and px.ndim == 4
    full = px.astype(np.float32) - (np.asarray(mean, np.float32)[None] if mean is not None else np.float32(0))
    out = np.empty((px.shape[0], len(views), px.shape[1], in_h, in_w), np.float32)
    for v, (oy, ox, flip) in enumerate(views):
        assert 0 <= oy <= px.shape[2] - in_h and 0 <= ox <= px.shape[3] - in_w, "view %r leaves the source" % ((oy, ox, flip),)
        crop = full[:, :, oy:oy + in_h, ox:ox + in_w]
        out[:, v] = crop[..., ::-1] if flip else crop
    return out.reshape(px.shape[0] * len(views), px.shape[1], in_h, in_w)


def nhwc(slots):
    """[S][C][H][W] -> the NHWC order of a layer dump."""
    return np.ascontiguousarray(np.asarray(slots).transpose(0, 2, 3, 1))


def mean_views(p, V):
    """float32 rows [n*V][C] of the slots -> [n][C]: the sum in view order, then the division, each rounded once."""
    p = np.asarray(p)
    assert p.dtype == np.float32 and p.ndim == 2 and V >= 1 and p.shape[0] % V == 0
    p3 = p.reshape(p.shape[0] // V, V, p.shape[1])
    s = p3[:, 0].copy()
    for v in range(1, V):
        s = s + p3[:, v]
    return s / np.float32(V)


def ten_crop(src_h, src_w, in_h, in_w):
    """The four corners, the centre, then the same five mirrored; None when the source is smaller than the input."""
    if src_h < in_h or src_w < in_w:
        return None
    bottom, right = src_h - in_h, src_w - in_w
    plain = [(0, 0, 0), (0, right, 0), (bottom, 0, 0), (bottom, right, 0), (bottom // 2, right // 2, 0)]
    return plain + [(oy, ox, 1) for (oy, ox, _) in plain]
