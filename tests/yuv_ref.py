"""TEST INFRASTRUCTURE — YCbCr frames in every layout the _yuv 8-bit calls read in place (qcnn_forward_u8_resized_views_yuv /
_relaxed_views_yuv) and the integer conversion that defines what the network sees of them.  numpy only, no GPU:
tests/test_yuv_cpu.py holds this module to the conversion's fixed points, to the real-number formula and to the library's own
constructor; tests/test_gpu_yuv.py hands buffer and descriptors to the device and expects what tests/resize_ref.py /
relaxed_ref.py make of to_bgr of the frames.

A frame is (Y [h][w], Cb [ch][cw], Cr [ch][cw]) uint8 with ch = ((h - 1) >> sub_y) + 1, cw likewise.  A descriptor is an
engine.SrcYuv.  Every byte of a buffer that is no sample — row padding, the unused half of a chroma row's padding, the frame
around a region — comes from the `fill` generator the caller gives (POISON tests).

  NV12 NV21 I420 YV12 I444 YUY2 UYVY     the frame layouts of qcnn_src_yuv_frame, tight
  *_pitched                               the same with a luma pitch beyond the tight one
  NV12_roi                                a pitched NV12 region at an odd-looking corner (6, 10) inside a larger NV12 frame
  I420_bottom_up                          I420 whose three planes are stored last row first: negative row strides
"""
from __future__ import annotations

import numpy as np

from conftest import pkg

engine = pkg("engine")
SrcYuv = engine.SrcYuv

#            y0  ky     crv     cbg    crg    cbu
MATRICES = {"JFIF": (0, 65536, 91881, 22554, 46802, 116130),
            "BT601": (16, 76309, 104597, 25675, 53279, 132201),
            "BT709": (16, 76309, 117489, 13975, 34925, 138438)}
MATRIX_NAMES = ["JFIF", "BT601", "BT709"]
MATRIX_ID = {"JFIF": 0, "BT601": 1, "BT709": 2}
#            Kr      Kb      luma / chroma excursion, luma offset: the real-number transforms the integers approximate
REAL = {"JFIF": (0.299, 0.114, 255.0, 255.0, 0.0), "BT601": (0.299, 0.114, 219.0, 224.0, 16.0), "BT709": (0.2126, 0.0722, 219.0, 224.0, 16.0)}
FORMATS = ["NV12", "NV21", "I420", "YV12", "I444", "YUY2", "UYVY"]
SUB = {"NV12": (1, 1), "NV21": (1, 1), "I420": (1, 1), "YV12": (1, 1), "I444": (0, 0), "YUY2": (0, 1), "UYVY": (0, 1)}
KINDS = FORMATS + [f + "_pitched" for f in FORMATS] + ["NV12_roi", "I420_bottom_up"]      # 16: coprime with the 9 source sizes
ROI_CORNER, ROI_MARGIN = (6, 10), (4, 6)          # even: a region of a 4:2:0 frame starts on a chroma sample


def sub_of(kind):
    return SUB[kind.split("_")[0]]


def chroma_size(h, w, sub):
    return ((h - 1) >> sub[0]) + 1, ((w - 1) >> sub[1]) + 1


def rng_fill(seed):
    rng = np.random.default_rng(seed)
    return lambda n: rng.integers(0, 256, n, dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------ the conversion
def _positions(h, w, sub, ceil=False, x_shift=True):
    """Row and column of the chroma sample of every pixel (replicated: y >> sub_y, x >> sub_x)."""
    ch, cw = chroma_size(h, w, sub)
    y, x = np.arange(h), np.arange(w)
    cy = np.minimum((y + ((1 << sub[0]) - 1 if ceil else 0)) >> sub[0], ch - 1)
    cx = np.minimum((x + ((1 << sub[1]) - 1 if ceil else 0)) >> sub[1], cw - 1) if x_shift else np.minimum(x, cw - 1)
    return cy[:, None], cx[None, :]


def _sums(Y, Cb, Cr, sub, matrix, ceil=False, x_shift=True):
    """int64 [3][h][w]: the accumulators of B, G, R before rounding, shift and clamp."""
    y0, ky, crv, cbg, crg, cbu = MATRICES[matrix]
    Y, Cb, Cr = (np.asarray(a).astype(np.int64) for a in (Y, Cb, Cr))
    h, w = Y.shape
    assert Cb.shape == Cr.shape == chroma_size(h, w, sub), "chroma planes of the wrong size"
    cy, cx = _positions(h, w, sub, ceil, x_shift)
    yy, cb, cr = (Y - y0) * ky, Cb[cy, cx] - 128, Cr[cy, cx] - 128
    return np.stack([yy + cbu * cb, yy - cbg * cb - crg * cr, yy + crv * cr])


def to_bgr(Y, Cb, Cr, sub, matrix):
    """The planar uint8 [3][h][w] image (B, G, R) the network sees of a frame: the table of include/qcnn_hip.h in int64."""
    return np.clip((_sums(Y, Cb, Cr, sub, matrix) + 32768) >> 16, 0, 255).astype(np.uint8)


def unclamped(Y, Cb, Cr, sub, matrix):
    """bool [h][w]: no channel of the pixel is clamped."""
    v = (_sums(Y, Cb, Cr, sub, matrix) + 32768) >> 16
    return ((v >= 0) & (v <= 255)).all(axis=0)


def real_bgr(Y, Cb, Cr, matrix):
    """float64 B, G, R of full-resolution Y, Cb, Cr by the real-number inverse transform, unrounded and unclamped."""
    kr, kb, ey, ec, off = REAL[matrix]
    kg = 1.0 - kr - kb
    y = (np.asarray(Y, np.float64) - off) * (255.0 / ey)
    pb, pr = (np.asarray(Cb, np.float64) - 128.0) * (255.0 / ec), (np.asarray(Cr, np.float64) - 128.0) * (255.0 / ec)
    r, b = y + 2.0 * (1.0 - kr) * pr, y + 2.0 * (1.0 - kb) * pb
    return np.stack([b, (y - kr * r - kb * b) / kg, r])


def like_image(bgr, matrix, sub):
    """A frame made by the forward transform of a uint8 [3][h][w] B, G, R image, chroma averaged over each sub-sampling block:
    what a decoder hands over of a picture."""
    kr, kb, ey, ec, off = REAL[matrix]
    b, g, r = (np.asarray(p, np.float64) for p in bgr)
    y = kr * r + (1.0 - kr - kb) * g + kb * b
    pb, pr = 0.5 * (b - y) / (1.0 - kb), 0.5 * (r - y) / (1.0 - kr)
    h, w = y.shape
    ch, cw = chroma_size(h, w, sub)

    q = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    pad = lambda p: np.pad(p, ((0, (ch << sub[0]) - h), (0, (cw << sub[1]) - w)), mode="edge")     # an odd side: the last block repeats its edge
    down = lambda p: pad(p).reshape(ch, 1 << sub[0], cw, 1 << sub[1]).mean(axis=(1, 3))
    return q(off + y * ey / 255.0), q(128.0 + down(pb) * ec / 255.0), q(128.0 + down(pr) * ec / 255.0)


def random_frame(rng, h, w, sub):
    ch, cw = chroma_size(h, w, sub)
    return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ch, cw), (ch, cw)))


def _wrong(**kw):
    def convert(Y, Cb, Cr, sub, matrix):
        if kw.get("swap"):
            Cb, Cr = Cr, Cb
        if kw.get("matrix"):
            matrix = MATRIX_NAMES[(MATRIX_NAMES.index(matrix) + 1) % 3]
        v = (_sums(Y, Cb, Cr, sub, matrix, kw.get("ceil", False), kw.get("x_shift", True)) + kw.get("rnd", 32768)) >> 16
        return (v & 255).astype(np.uint8) if kw.get("wrap") else np.clip(v, 0, 255).astype(np.uint8)
    return convert


# The mistakes a kernel can make, each a to_bgr gone wrong in one way.
WRONG = {
    "no_rounding_term": _wrong(rnd=0),
    "wrap_instead_of_clamp": _wrong(wrap=True),
    "cb_cr_swapped": _wrong(swap=True),
    "chroma_position_rounded_up": _wrong(ceil=True),
    "another_matrix": _wrong(matrix=True),
    "chroma_shift_on_one_axis_only": _wrong(x_shift=False),
}


# ------------------------------------------------------------------------------------------------------ the layouts
def place(frame, kind, matrix="JFIF"):
    """One frame under one layout -> (size of its chunk in bytes, SrcYuv relative to the chunk).  numpy arithmetic of its own:
    tests/test_yuv_cpu.py holds qcnn_src_yuv_frame to it."""
    Y, Cb, Cr = frame
    h, w = Y.shape
    fmt, sub, m = kind.split("_")[0], sub_of(kind), MATRIX_ID[matrix]
    assert Cb.shape == Cr.shape == chroma_size(h, w, sub)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    if kind == "NV12_roi":                            # the region of an (fh x fw) NV12 frame whose top-left pixel is ROI_CORNER
        fh, fw = ROI_CORNER[0] + h + ROI_MARGIN[0], ROI_CORNER[1] + w + ROI_MARGIN[1]
        pitch = 2 * ((fw + 1) // 2) + 10
        chroma = fh * pitch + (ROI_CORNER[0] // 2) * pitch + ROI_CORNER[1]
        return pitch * (fh + (fh + 1) // 2), SrcYuv(ROI_CORNER[0] * pitch + ROI_CORNER[1], chroma, chroma + 1, pitch, pitch, h, w, 1, 2, 1, 1, m)
    tight = {"NV12": 2 * cw, "NV21": 2 * cw, "I420": w, "YV12": w, "I444": w, "YUY2": 4 * cw, "UYVY": 4 * cw}[fmt]
    pitch = tight + (37 if kind.endswith("_pitched") else 0)
    if fmt in ("NV12", "NV21"):
        d = SrcYuv(0, pitch * h + (fmt == "NV21"), pitch * h + (fmt == "NV12"), pitch, pitch, h, w, 1, 2, 1, 1, m)
        size = pitch * (h + ch)
    elif fmt in ("I420", "YV12"):
        cp = (pitch + 1) // 2
        first, second = pitch * h, pitch * h + cp * ch
        d = SrcYuv(0, first if fmt == "I420" else second, second if fmt == "I420" else first, pitch, cp, h, w, 1, 1, 1, 1, m)
        size = pitch * h + 2 * cp * ch
        if kind == "I420_bottom_up":
            d = d._replace(y_offset=(h - 1) * pitch, cb_offset=first + (ch - 1) * cp, cr_offset=second + (ch - 1) * cp, y_row_stride=-pitch,
                           c_row_stride=-cp)
    elif fmt == "I444":
        d = SrcYuv(0, pitch * h, 2 * pitch * h, pitch, pitch, h, w, 1, 1, 0, 0, m)
        size = 3 * pitch * h
    else:
        d = SrcYuv(0, 1, 3, pitch, pitch, h, w, 2, 4, 0, 1, m) if fmt == "YUY2" else SrcYuv(1, 0, 2, pitch, pitch, h, w, 2, 4, 0, 1, m)
        size = pitch * h
    return size, d


class Buffer:
    """frames[i] under kinds[i] and matrices[i], the chunks back to back: .flat (uint8), .descs ([SrcYuv], offsets into .flat),
    .refs (the planar B, G, R images the network sees: to_bgr), .kinds, .matrices, .frames, .sample (bool per byte of .flat:
    read by a descriptor)."""

    def __init__(self, frames, kinds, matrices, fill):
        self.frames, self.kinds, self.matrices = list(frames), list(kinds), list(matrices)
        placed = [place(f, k, m) for f, k, m in zip(self.frames, self.kinds, self.matrices)]
        starts = np.concatenate([[0], np.cumsum([p[0] for p in placed])]).astype(np.int64)
        self.flat = np.ascontiguousarray(fill(int(starts[-1])), np.uint8)
        self.sample = np.zeros(self.flat.size, bool)
        self.descs, self.refs = [], []
        for (size, d), start, (Y, Cb, Cr), kind, matrix in zip(placed, starts, self.frames, self.kinds, self.matrices):
            start = int(start)
            d = d._replace(y_offset=d.y_offset + start, cb_offset=d.cb_offset + start, cr_offset=d.cr_offset + start)
            at = d.sample_index()
            assert at.min() >= start and at.max() < start + size, "a sample outside its chunk"
            sy, sx = 1 << d.sub_y, 1 << d.sub_x
            self.flat[at[0]] = Y
            self.flat[at[1][::sy, ::sx]] = Cb
            self.flat[at[2][::sy, ::sx]] = Cr
            self.sample[at] = True
            self.descs.append(d)
            self.refs.append(to_bgr(Y, Cb, Cr, sub_of(kind), matrix))

    def read_back(self, i):
        """Frame i through its descriptor and plain numpy indexing: the replicated uint8 [3][h][w] planes Y, Cb, Cr."""
        return self.flat[self.descs[i].sample_index()]

    def wrong_refs(self, name):
        return [WRONG[name](Y, Cb, Cr, sub_of(k), m) for (Y, Cb, Cr), k, m in zip(self.frames, self.kinds, self.matrices)]


def test_frames(sources, n, start, seed):
    """The frames of tests/test_gpu_yuv.py: image i has size sources[(start + i) % len], kind KINDS[(start + i) % 16], matrix
    MATRIX_NAMES[(i // 2) % 3]; even i: like_image of a random B, G, R picture, odd i: uniformly random samples."""
    rng = np.random.default_rng(seed)
    frames, kinds, matrices = [], [], []
    for i in range(n):
        h, w = sources[(start + i) % len(sources)]
        kind, matrix = KINDS[(start + i) % len(KINDS)], MATRIX_NAMES[(i // 2) % 3]
        if i % 2 == 0:
            frames.append(like_image(rng.integers(0, 256, (3, h, w), dtype=np.uint8), matrix, sub_of(kind)))
        else:
            frames.append(random_frame(rng, h, w, sub_of(kind)))
        kinds.append(kind)
        matrices.append(matrix)
    return frames, kinds, matrices


test_frames.__test__ = False                          # a helper, not a test
