"""TEST INFRASTRUCTURE — what the GPU tests of the 8-bit input paths share (tests/test_gpu_views.py, test_gpu_resize.py,
test_gpu_relaxed.py): an engine whose input map stays readable, bit-wise comparison, device outputs that show what a call left
untouched, and source images of differing sizes on the device in front of the engine method under test."""
import numpy as np
import torch

from conftest import pkg

capi = pkg("capi")
engine = pkg("engine")
DEV = torch.device("cuda", 0)


def make_engine(in_chw, layers, params, max_batch, lut=None):
    eng = engine.QcnnEngine(0)
    eng.set_option(capi.OPT_KEEP_ALL, 1)          # fm[0] stays readable; the 8-bit paths pack, so does qcnn_forward then
    if lut is not None:
        eng.set_option(capi.OPT_LUT_MODE, lut)
    eng.load_model(in_chw, layers, params, max_batch)
    return eng


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


class Outputs:
    """Device outputs of one call, pre-filled with NaN / -1: what a call leaves untouched shows."""

    def __init__(self, eng, n, V, want=(True, True, True)):
        h, w, c = eng.fm_dims(eng.L)
        self.classes = h * w * c
        self.prob = torch.full((max(n, 1), self.classes), float("nan"), dtype=torch.float32, device=DEV) if want[0] else None
        self.top5 = torch.full((max(n, 1), 5), -1, dtype=torch.int16, device=DEV) if want[1] else None
        self.rows = torch.full((max(n * V, 1), self.classes), float("nan"), dtype=torch.float32, device=DEV) if want[2] else None

    def ptrs(self):
        return tuple(t.data_ptr() if t is not None else None for t in (self.prob, self.top5, self.rows))

    def host(self):
        return (self.prob.cpu().numpy() if self.prob is not None else None,
                self.top5.cpu().numpy().view(np.uint16) if self.top5 is not None else None,
                self.rows.cpu().numpy() if self.rows is not None else None)

    def untouched(self):
        p, t, r = self.host()
        return ((p is None or np.isnan(p).all()) and (t is None or (t == 0xFFFF).all()) and (r is None or np.isnan(r).all()))


class Source:
    """Images of differing sizes packed into one device buffer (engine.pack_sources) + the mean on the device, for the engine
    method `method` (forward_u8_resized_views_dev, forward_u8_relaxed_views_dev)."""

    def __init__(self, method, images, mean):
        self.method = method
        self.flat, self.descs = engine.pack_sources(images)
        self.d_flat = torch.from_numpy(self.flat).to(DEV)
        self.d_mean = torch.from_numpy(np.ascontiguousarray(mean)).to(DEV) if mean is not None else None
        torch.cuda.synchronize()

    def call(self, eng, full, views, out, descs=None, src_bytes=None):
        getattr(eng, self.method)(self.d_flat.data_ptr(), self.flat.size if src_bytes is None else src_bytes,
                                  self.descs if descs is None else descs, full[0], full[1],
                                  self.d_mean.data_ptr() if self.d_mean is not None else None, views, *out.ptrs())


def run_sources(method, eng, images, full, mean, views, want=(True, True, True)):
    src = Source(method, images, mean)
    out = Outputs(eng, len(images), len(views), want)
    src.call(eng, full, views, out)
    eng.sync()
    return out.host()
