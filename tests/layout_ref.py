"""TEST INFRASTRUCTURE — source buffers in every layout the strided 8-bit calls read in place (qcnn_forward_u8_resized_views_strided /
_relaxed_views_strided), made from planar uint8 [C][h][w] images.  numpy only, no GPU: tests/test_layout_cpu.py reads every
layout back through its descriptor; tests/test_gpu_layout.py hands buffer and descriptors to the device and expects what
tests/resize_ref.py / relaxed_ref.py make of the PLANAR images.

A descriptor is an engine.SrcPixels (offset, row_stride, h, w, pix_stride, ch_offset): sample (c, y, x) is byte
offset + y * row_stride + x * pix_stride + ch_offset[c] of the buffer.  Every byte of a buffer that is no sample — padding,
alpha, gaps, the frame around a region, file headers — comes from the `fill` generator the caller gives: two buffers made with
different generators hold the same samples and differ everywhere else (POISON tests).

  planar           the existing layout [C][h][w], as a descriptor
  bgr              interleaved [h][w][3], tight
  rgb              the same with the bytes of a pixel in the order R, G, B: ch_offset = (2, 1, 0)
  bmp24            a whole file from resize_ref.write_bmp (24-bit, bottom-up, rows padded to 4 bytes), described by src_bmp
  bmp32_topdown    a whole 32-bit file with a negative height, written here, described by src_bmp
  bgra_pitched     4 bytes a pixel, row pitch 64 bytes beyond 4 * w
  roi              the image as a rectangle at an odd corner (5, 3) inside a larger interleaved frame
  planar_pitched   planes with rows padded by 13 bytes and a gap of 29 bytes between planes
  grey             ONE plane, all three ch_offset equal: the image the network sees is plane 0 three times
"""
from __future__ import annotations

import os
import struct
import tempfile

import numpy as np

import resize_ref as rr
from conftest import pkg

engine = pkg("engine")
SrcPixels = engine.SrcPixels

LAYOUTS = ["planar", "bgr", "rgb", "bmp24", "bmp32_topdown", "bgra_pitched", "roi", "planar_pitched", "grey"]
ROI_CORNER, ROI_MARGIN = (5, 3), (4, 6)           # rows above / columns left of the region; rows below / columns right of it


def rng_fill(seed):
    """A generator of non-sample bytes: fill(n) -> uint8 [n], random."""
    rng = np.random.default_rng(seed)
    return lambda n: rng.integers(0, 256, n, dtype=np.uint8)


def const_fill(value):
    return lambda n: np.full(n, value, np.uint8)


def bmp24_file(planes) -> bytes:
    """The file resize_ref.write_bmp writes for planes [3][h][w]."""
    fd, path = tempfile.mkstemp(suffix=".bmp")
    os.close(fd)
    try:
        rr.write_bmp(path, planes)
        with open(path, "rb") as f:
            return f.read()
    finally:
        os.unlink(path)


def bmp32_topdown_file(planes, alpha=0) -> bytes:
    """uint8 [3][h][w] (B, G, R) -> a 32-bit BMP with a negative height: rows top-down, 4 bytes a pixel, no padding."""
    planes = np.asarray(planes)
    assert planes.dtype == np.uint8 and planes.ndim == 3 and planes.shape[0] == 3
    _, h, w = planes.shape
    px = np.full((h, w, 4), alpha, np.uint8)
    px[:, :, :3] = planes.transpose(1, 2, 0)
    data = px.tobytes()
    return (struct.pack("<2sIHHI", b"BM", 54 + len(data), 0, 0, 54) +
            struct.pack("<IiiHHIIiiII", 40, w, -h, 1, 32, 0, len(data), 2835, 2835, 0, 0) + data)


def place(img, layout):
    """One image under one layout -> (size of its chunk in bytes, SrcPixels relative to the chunk, the planar image the network
    sees, bytes the chunk must hold besides the samples: {position: bytes} — the headers a BMP parser reads)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[0] == 3, "layout_ref lays out three-channel images"
    C, h, w = img.shape
    if layout == "planar":
        return C * h * w, SrcPixels(0, w, h, w, 1, (0, h * w, 2 * h * w, 0)), img, {}
    if layout == "bgr":
        return 3 * h * w, SrcPixels(0, 3 * w, h, w, 3, (0, 1, 2, 0)), img, {}
    if layout == "rgb":
        return 3 * h * w, SrcPixels(0, 3 * w, h, w, 3, (2, 1, 0, 0)), img, {}
    if layout in ("bmp24", "bmp32_topdown"):
        f = bmp24_file(img) if layout == "bmp24" else bmp32_topdown_file(img)
        return len(f), engine.src_bmp(f, 0), img, {0: f[:54]}
    if layout == "bgra_pitched":
        pitch = 4 * w + 64
        return h * pitch, SrcPixels(0, pitch, h, w, 4, (0, 1, 2, 0)), img, {}
    if layout == "roi":
        fw = ROI_CORNER[1] + w + ROI_MARGIN[1]
        fh = ROI_CORNER[0] + h + ROI_MARGIN[0]
        return 3 * fh * fw, SrcPixels(3 * (ROI_CORNER[0] * fw + ROI_CORNER[1]), 3 * fw, h, w, 3, (0, 1, 2, 0)), img, {}
    if layout == "planar_pitched":
        pitch = w + 13
        plane = h * pitch + 29
        return 3 * plane, SrcPixels(0, pitch, h, w, 1, (0, plane, 2 * plane, 0)), img, {}
    if layout == "grey":
        return h * w, SrcPixels(0, w, h, w, 1, (0, 0, 0, 0)), np.repeat(img[:1], 3, axis=0), {}
    raise ValueError("unknown layout %r" % (layout,))


class Buffer:
    """images[i] under layouts[i % len(layouts)], the chunks back to back: .flat (uint8), .descs ([SrcPixels], offsets into
    .flat), .refs (the planar images the network sees), .layouts (the name per image), .sample (bool per byte of .flat: read
    by a descriptor).  keep_headers = False: the bytes a BMP parser reads come from `fill` too (the descriptors are made before)."""

    def __init__(self, images, layouts, fill, keep_headers=True):
        layouts = [layouts] if isinstance(layouts, str) else list(layouts)
        self.layouts = [layouts[i % len(layouts)] for i in range(len(images))]
        placed = [place(img, lay) for img, lay in zip(images, self.layouts)]
        starts = np.concatenate([[0], np.cumsum([p[0] for p in placed])]).astype(np.int64)
        self.flat = np.ascontiguousarray(fill(int(starts[-1])), np.uint8)
        assert self.flat.shape == (int(starts[-1]),)
        self.sample = np.zeros(self.flat.size, bool)
        self.descs, self.refs = [], []
        for (size, d, ref, keep), start in zip(placed, starts):
            d = d._replace(offset=d.offset + int(start))
            at = d.sample_index(3)
            assert at.min() >= start and at.max() < start + size, "a sample outside its chunk"
            if d.ch_offset[0] == d.ch_offset[1]:      # grey: the three channels alias plane 0
                self.flat[at[0]] = ref[0]
            else:
                self.flat[at] = ref
            self.sample[at] = True
            if keep_headers:
                for pos, b in keep.items():
                    self.flat[start + pos:start + pos + len(b)] = np.frombuffer(b, np.uint8)
            self.descs.append(d)
            self.refs.append(ref)

    def read_back(self, i):
        """Image i through its descriptor and plain numpy indexing: uint8 [3][h][w]."""
        return self.flat[self.descs[i].sample_index(3)]
