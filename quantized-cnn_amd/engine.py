"""CaffeEva-shaped Python driver over the C-ABI (used by bench.py, the tests and smoke()).

Same life-cycle as the reference's CaffeEva (include/CaffeEva.h:64-85): configure the layer table,
load the per-layer parameters, run forward passes, read per-layer timings — but for a whole batch of
images resident on one MI355X.  All arithmetic happens in libqcnn_hip.so; this file only moves
pointers.  The C++ host mirror (include/CaffeEva.h of this repo) is the same thing for C++ callers.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import capi
from .topology import CONV, FCNT


class QcnnError(RuntimeError):
    pass


DEFAULT_MAX_ITER = 30     # Lloyd steps of quantize_layer / quantize.quantize_model unless the caller says otherwise
DEFAULT_EC_SWEEPS = 4     # sweeps of quantize_layer_ec unless the caller says otherwise
DEFAULT_EC_RIDGE = 1e-6   # its ridge, in units of the mean diagonal of the gram matrix
EC_GRAM_RUN = 256         # QCNN_EC_GRAM_RUN: patches calib_gram sums in fp32 before the sums move to fp64


def _ptr(p):
    """An address as the C-ABI takes it: NULL for None (and 0)."""
    return C.c_void_p(p) if p else None


def _struct_array(ctype, rows):
    """(ctypes array, length) of a sequence of rows of ints — views (oy, ox, flip) / (ay, ax, dy, dx, flip), descriptors
    (offset, h, w); an empty sequence still gives an array the C side may be handed."""
    rs = [tuple(int(x) for x in r) for r in rows]
    return (ctype * max(len(rs), 1))(*[ctype(*r) for r in rs]), len(rs)


def _desc_array(descs):
    if isinstance(descs, C.Array) and descs._type_ is capi.QcnnSrcImage:     # made once by the caller: no per-call conversion
        return descs, len(descs)
    return _struct_array(capi.QcnnSrcImage, descs)


class SrcPixels(collections.namedtuple("SrcPixels", "offset row_stride h w pix_stride ch_offset")):
    """A source image of the strided calls as Python holds it (capi.QcnnSrcPixels): sample (c, y, x) is the byte at offset +
    y * row_stride + x * pix_stride + ch_offset[c] of the source buffer.  ch_offset: up to four ints, network order B, G, R."""
    __slots__ = ()

    def sample_index(self, C):
        """int64 [C][h][w]: the byte of every sample in the source buffer (numpy indexing reads the image through it)."""
        c = np.asarray(self.ch_offset[:C], np.int64)[:, None, None]
        y = np.arange(self.h, dtype=np.int64)[None, :, None]
        x = np.arange(self.w, dtype=np.int64)[None, None, :]
        return int(self.offset) + y * int(self.row_stride) + x * int(self.pix_stride) + c


def _pixels_array(descs):
    """(ctypes array of QcnnSrcPixels, length) of SrcPixels / (offset, row_stride, h, w, pix_stride, ch_offset) rows."""
    if isinstance(descs, C.Array) and descs._type_ is capi.QcnnSrcPixels:    # made once by the caller: no per-call conversion
        return descs, len(descs)
    rows = list(descs)
    arr = (capi.QcnnSrcPixels * max(len(rows), 1))()
    for d, (off, rs, h, w, ps, co) in zip(arr, rows):
        co = tuple(int(v) for v in co) + (0,) * (4 - len(co))
        d.offset, d.row_stride, d.h, d.w, d.pix_stride, d.ch_offset = int(off), int(rs), int(h), int(w), int(ps), (C.c_int32 * 4)(*co)
    return arr, len(rows)


def _from_c(d):
    return SrcPixels(int(d.offset), int(d.row_stride), int(d.h), int(d.w), int(d.pix_stride), tuple(int(v) for v in d.ch_offset))


class SrcYuv(collections.namedtuple("SrcYuv", "y_offset cb_offset cr_offset y_row_stride c_row_stride h w y_pix_stride c_pix_stride "
                                             "sub_y sub_x matrix")):
    """A YCbCr source frame of the _yuv calls as Python holds it (capi.QcnnSrcYuv): pixel (y, x) has Y at y_offset +
    y * y_row_stride + x * y_pix_stride and Cb / Cr at cb_offset / cr_offset + (y >> sub_y) * c_row_stride + (x >> sub_x) *
    c_pix_stride of the source buffer.  matrix: the integer of capi.YUV_MATRICES."""
    __slots__ = ()

    def sample_index(self):
        """int64 [3][h][w]: the bytes of Y, Cb and Cr of every pixel in the source buffer (chroma replicated)."""
        y = np.arange(self.h, dtype=np.int64)[:, None]
        x = np.arange(self.w, dtype=np.int64)[None, :]
        c = (y >> int(self.sub_y)) * int(self.c_row_stride) + (x >> int(self.sub_x)) * int(self.c_pix_stride)
        return np.stack([int(self.y_offset) + y * int(self.y_row_stride) + x * int(self.y_pix_stride), int(self.cb_offset) + c,
                         int(self.cr_offset) + c])


def _yuv_array(descs):
    """(ctypes array of QcnnSrcYuv, length) of SrcYuv rows."""
    if isinstance(descs, C.Array) and descs._type_ is capi.QcnnSrcYuv:       # made once by the caller: no per-call conversion
        return descs, len(descs)
    return _struct_array(capi.QcnnSrcYuv, descs)


def _is_yuv(descs):
    """Are these the descriptors of YCbCr frames (SrcYuv / capi.QcnnSrcYuv) and not of strided pixels?  One kind per call."""
    if isinstance(descs, C.Array):
        return descs._type_ is capi.QcnnSrcYuv
    kinds = {isinstance(d, SrcYuv) for d in descs}
    if len(kinds) > 1:
        raise ValueError("the descriptors of one call are SrcPixels or SrcYuv, not both")
    return kinds == {True}


class QcnnEngine:
    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = capi.load()
        h = C.c_void_p()
        rc = self.lib.qcnn_ctx_create(device, _ptr(stream), C.byref(h))
        if rc:
            raise QcnnError(self.lib.qcnn_last_error(None).decode())
        self.h = h
        self.layers = None
        self.L = 0
        self.max_batch = 0

    # -- plumbing -------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc:
            raise QcnnError(self.lib.qcnn_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.qcnn_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt: int, value: int):
        self._chk(self.lib.qcnn_set_option(self.h, opt, value))

    def sync(self):
        self._chk(self.lib.qcnn_sync(self.h))

    # -- model ----------------------------------------------------------------------------------
    def configure(self, in_chw, layers, shapes):
        """shapes: {layer_idx: (M, K, Cs)} for every conv/FC layer."""
        arr = (capi.QcnnLayerDesc * len(layers))(*[capi.layer_desc(l) for l in layers])
        self._chk(self.lib.qcnn_model_begin(self.h, len(layers), arr, in_chw[0], in_chw[1], in_chw[2]))
        for i, (m, k, cs) in shapes.items():
            self._chk(self.lib.qcnn_model_set_layer_shape(self.h, i, m, k, cs))
        self.layers, self.L, self.in_chw = layers, len(layers), tuple(in_chw)

    def arena_bytes(self) -> int:
        n = C.c_size_t(0)
        self._chk(self.lib.qcnn_model_arena_bytes(self.h, C.byref(n)))
        return n.value

    def commit(self, max_batch: int, arena_ptr: int | None = None):
        self._chk(self.lib.qcnn_model_commit(self.h, max_batch, _ptr(arena_ptr)))
        self.max_batch = max_batch

    def upload(self, params):
        for i, p in params.items():
            bias = np.ascontiguousarray(p["bias"], np.float32)
            ctrd = np.ascontiguousarray(p["ctrd"], np.float32)
            asmt = np.ascontiguousarray(p["asmt"], np.uint8)
            self._chk(self.lib.qcnn_model_set_layer_params(self.h, i, bias.ctypes.data, ctrd.ctypes.data,
                                                           asmt.ctypes.data))

    def upload_cbn(self, params):
        """Same as upload(), but the assignments travel bit-packed (the .cbn payload) and are decoded on the device."""
        from . import fileio
        for i, p in params.items():
            bias = np.ascontiguousarray(p["bias"], np.float32)
            ctrd = np.ascontiguousarray(p["ctrd"], np.float32)
            blocks = fileio.cbn_pack(np.ascontiguousarray(p["asmt"], np.uint8), int(p["bits"]))
            self._chk(self.lib.qcnn_model_set_layer_params_cbn(self.h, i, bias.ctypes.data, ctrd.ctypes.data,
                                                               blocks.ctypes.data, blocks.nbytes, int(p["bits"])))

    def mark_loaded(self):
        self._chk(self.lib.qcnn_model_mark_loaded(self.h))

    def arena_checksum(self):
        """(sum of the arena's 32-bit words, position-weighted sum) as it lies on the device — equal on ranks that hold the same
        parameter bytes (qcnn_model_arena_checksum); blocking."""
        s2 = (C.c_ulonglong * 2)()
        self._chk(self.lib.qcnn_model_arena_checksum(self.h, s2))
        return int(s2[0]), int(s2[1])

    def load_model(self, in_chw, layers, params, max_batch, arena_ptr=None, upload=True):
        shapes = {i: tuple(int(x) for x in p["ctrd"].shape) for i, p in params.items()}   # (M, K, Cs)
        for i, ly in enumerate(layers):
            if ly["type"] in (CONV, FCNT) and i not in shapes:
                raise QcnnError("layer %d has no parameters" % i)
        self.configure(in_chw, layers, shapes)
        self.commit(max_batch, arena_ptr)
        if upload:
            self.upload(params)

    def load_dense_model(self, in_chw, layers, dense, max_batch):
        """The reference's precise path (Init(false)): dense = {layer: dict(bias, weights)} in the convKnl / fcntWei file
        layout (synth.make_dense_params)."""
        arr = (capi.QcnnLayerDesc * len(layers))(*[capi.layer_desc(l) for l in layers])
        self._chk(self.lib.qcnn_model_begin(self.h, len(layers), arr, in_chw[0], in_chw[1], in_chw[2]))
        for i in dense:
            self._chk(self.lib.qcnn_model_set_layer_dense(self.h, i))
        self.layers, self.L, self.in_chw = layers, len(layers), tuple(in_chw)
        self.commit(max_batch)
        for i, p in dense.items():
            bias = np.ascontiguousarray(p["bias"], np.float32)
            w = np.ascontiguousarray(p["weights"], np.float32)
            self._chk(self.lib.qcnn_model_set_layer_weights(self.h, i, bias.ctypes.data, w.ctypes.data))

    def quantize_layer(self, weights, M, K, Cs, ctrd_init=None, max_iter=DEFAULT_MAX_ITER):
        """Product-quantisation k-means of one dense layer on this context's GPU (qcnn_quantize_layer).  weights: conv kernels
        [Ct][Cin][kh][kw] (convKnl layout) or FC weights [Ct][D] (fcntWei).  Returns (ctrd [M][K][Cs] float32, asmt uint8 0-based
        in file order [Ct][kh][kw][M] / [Ct][M], stats dict(sse_init, sse, iters, unconverged)).  Needs no loaded model and leaves
        a loaded one untouched."""
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim == 4:
            ct, cin, kh, kw = w.shape
            ashape = (ct, kh, kw, M)
        elif w.ndim == 2:
            (ct, cin), kh, kw = w.shape, 1, 1
            ashape = (ct, M)
        else:
            raise QcnnError("weights must be [Ct][Cin][kh][kw] or [Ct][D], got shape %r" % (w.shape,))
        init = None
        if ctrd_init is not None:
            init = np.ascontiguousarray(ctrd_init, np.float32)
            if init.shape != (M, K, Cs):
                raise QcnnError("ctrd_init must be [M][K][Cs] = %r, got %r" % ((M, K, Cs), init.shape))
        ctrd = np.empty((max(M, 0), max(K, 0), max(Cs, 0)), np.float32)
        asmt = np.empty(tuple(max(x, 0) for x in ashape), np.uint8)
        sse = (C.c_double * 2)()
        it = (C.c_int * 2)()
        self._chk(self.lib.qcnn_quantize_layer(self.h, ct, cin, kh, kw, M, K, Cs, w.ctypes.data,
                                               init.ctypes.data if init is not None else None, max_iter,
                                               ctrd.ctypes.data, asmt.ctypes.data, sse, it))
        return ctrd, asmt, dict(sse_init=float(sse[0]), sse=float(sse[1]), iters=int(it[0]), unconverged=int(it[1]))

    def calib_gram(self, x_nhwc, geom, gram=None):
        """Second moments of a layer's input windows (qcnn_calib_gram).  x_nhwc: fm[layer] of n images, [n][H][W][C] (FC: anything
        of n rows, taken as [n][1][1][D]); geom: dict(grp, kh, kw, stride, pad) (quantize.layer_geom).  Returns float64
        [grp][P][P], P = kh*kw*C/grp; with ``gram`` (a C-contiguous float64 array of that shape) the sums are added to it in
        place and it is returned."""
        x = np.ascontiguousarray(x_nhwc, np.float32)
        if x.ndim != 4:
            x = x.reshape(x.shape[0], 1, 1, -1)
        n, h, w, ch = x.shape
        grp, kh, kw = int(geom["grp"]), int(geom["kh"]), int(geom["kw"])
        P = kh * kw * (ch // max(grp, 1))
        acc = gram is not None
        if acc:
            if gram.dtype != np.float64 or gram.shape != (grp, P, P) or not gram.flags["C_CONTIGUOUS"]:
                raise QcnnError("gram must be a C-contiguous float64 array of shape %r" % ((grp, P, P),))
        else:
            gram = np.empty((max(grp, 0), P, P), np.float64)
        self._chk(self.lib.qcnn_calib_gram(self.h, h, w, ch, grp, kh, kw, int(geom["stride"]), int(geom["pad"]), x.ctypes.data, n,
                                           gram.ctypes.data, 1 if acc else 0))
        return gram

    def calib_begin(self, layers):
        """Open a resident calibration on the loaded model (qcnn_calib_begin): one zeroed float64 matrix [grp][P][P] per listed
        conv / FC layer on the device, armed.  While armed, every batch of every forward call adds the second moments of those
        layers' input maps, where they lie.  With layer 0 listed, float forwards take the packed input route (qcnn_hip.h)."""
        ls = [int(l) for l in layers]
        arr = (C.c_int * max(len(ls), 1))(*ls)
        self._chk(self.lib.qcnn_calib_begin(self.h, arr, len(ls)))
        self._calib_shapes = {}
        for l in ls:
            ly = self.layers[l]
            h, w, ch = self.fm_dims(l)
            grp, taps, cin = (int(ly["grp"]), int(ly["knl"]) ** 2, ch) if ly["type"] == CONV else (1, 1, h * w * ch)
            self._calib_shapes[l] = (grp, taps * cin // grp, taps * cin // grp)

    def calib_arm(self, on):
        """Arm (True) or disarm (False) the open calibration (qcnn_calib_arm): unarmed forwards add nothing."""
        self._chk(self.lib.qcnn_calib_arm(self.h, 1 if on else 0))

    def calib_read(self, layer):
        """(gram float64 [grp][P][P], patch rows added so far) of a listed layer (qcnn_calib_read); blocking, resets nothing."""
        shape = getattr(self, "_calib_shapes", {}).get(int(layer))
        gram = np.empty(shape, np.float64) if shape else None
        rows = C.c_longlong(0)
        self._chk(self.lib.qcnn_calib_read(self.h, int(layer), gram.ctypes.data if shape else None, C.byref(rows)))
        return gram, int(rows.value)

    def calib_end(self):
        """Free the calibration's matrices (qcnn_calib_end); loading another model does the same."""
        self._calib_shapes = {}
        self._chk(self.lib.qcnn_calib_end(self.h))

    def quantize_layer_ec(self, weights, M, K, Cs, gram, ctrd, asmt, grp=1, sweeps=DEFAULT_EC_SWEEPS, ridge=DEFAULT_EC_RIDGE):
        """Error-corrected refinement of a quantisation of one layer (qcnn_quantize_layer_ec): from the book ``ctrd`` [M][K][Cs]
        and assignments ``asmt`` (file order, quantize_layer's output) minimise the response error e^T G e against ``gram``
        [grp][P][P] (calib_gram; None = identity).  Returns (ctrd, asmt, stats dict(obj_init, obj, obj_trace [sweeps + 1],
        changed [sweeps], sweeps = sweeps that changed something))."""
        w = np.ascontiguousarray(weights, np.float32)
        if w.ndim == 4:
            ct, cin, kh, kw = w.shape
            ashape = (ct, kh, kw, M)
        elif w.ndim == 2:
            (ct, cin), kh, kw = w.shape, 1, 1
            ashape = (ct, M)
        else:
            raise QcnnError("weights must be [Ct][Cin][kh][kw] or [Ct][D], got shape %r" % (w.shape,))
        c0 = np.ascontiguousarray(ctrd, np.float32)
        a0 = np.ascontiguousarray(asmt, np.uint8)
        if c0.shape != (M, K, Cs):
            raise QcnnError("ctrd must be [M][K][Cs] = %r, got %r" % ((M, K, Cs), c0.shape))
        if a0.size != int(np.prod(ashape)):
            raise QcnnError("asmt must have %r entries, got shape %r" % (ashape, a0.shape))
        g = None
        if gram is not None:
            g = np.ascontiguousarray(gram, np.float64)
            P = kh * kw * cin
            if g.shape != (grp, P, P):
                raise QcnnError("gram must be [grp][P][P] = %r, got %r" % ((grp, P, P), g.shape))
        c1 = np.empty_like(c0)
        a1 = np.empty(ashape, np.uint8)
        ns = max(int(sweeps), 0)
        obj = (C.c_double * (ns + 1))()
        chg = (C.c_int * max(ns, 1))()
        self._chk(self.lib.qcnn_quantize_layer_ec(self.h, ct, cin, grp, kh, kw, M, K, Cs, w.ctypes.data,
                                                  g.ctypes.data if g is not None else None, c0.ctypes.data, a0.ctypes.data,
                                                  int(sweeps), float(ridge), c1.ctypes.data, a1.ctypes.data, obj, chg))
        trace, changed = np.array(obj[:], np.float64), np.array(chg[:ns], np.int64)
        return c1, a1, dict(obj_init=float(trace[0]), obj=float(trace[-1]), obj_trace=trace, changed=changed,
                            sweeps=int(np.count_nonzero(changed)) if ns else 0)

    def fm_dims(self, l):
        d = (C.c_int * 3)()
        self._chk(self.lib.qcnn_fm_dims(self.h, l, d))
        return int(d[0]), int(d[1]), int(d[2])

    # -- forward --------------------------------------------------------------------------------
    def forward_dev(self, in_ptr: int, n: int, prob_ptr: int | None = None, top5_ptr: int | None = None):
        """Asynchronous, device pointers (e.g. torch tensors' data_ptr())."""
        self._chk(self.lib.qcnn_forward(self.h, _ptr(in_ptr), n, _ptr(prob_ptr), _ptr(top5_ptr)))

    def forward_u8_dev(self, in_ptr: int, src_h: int, src_w: int, mean_ptr: int | None, n: int,
                       prob_ptr: int | None = None, top5_ptr: int | None = None):
        """Asynchronous, device pointers: 8-bit planar images [n][C][src_h][src_w], mean [C][src_h][src_w] or None;
        mean subtraction + centre crop happen on the device (BmpImgIO::RmMeanImg/CropImg)."""
        self._chk(self.lib.qcnn_forward_u8(self.h, _ptr(in_ptr), src_h, src_w, _ptr(mean_ptr), n, _ptr(prob_ptr), _ptr(top5_ptr)))

    def forward_u8_views_dev(self, in_ptr: int, src_h: int, src_w: int, mean_ptr: int | None, n: int, views,
                             prob_ptr: int | None = None, top5_ptr: int | None = None, prob_views_ptr: int | None = None):
        """Asynchronous, device pointers: multi-view inference from 8-bit planar images (qcnn_forward_u8_views).  views: a
        sequence of (oy, ox, flip) — the top-left corner of a crop of the network's input size inside the source image,
        flip: mirrored left-right (ten_crop_views gives the standard ten).  Batch slot i * len(views) + v is view v of image i;
        prob [n][classes] / top5 [n][5] are those of the probabilities averaged over an image's views, prob_views
        [n][len(views)][classes] the un-averaged rows."""
        varr, V = _struct_array(capi.QcnnView, views)
        self._chk(self.lib.qcnn_forward_u8_views(self.h, _ptr(in_ptr), src_h, src_w, _ptr(mean_ptr), n, varr, V,
                                                 _ptr(prob_ptr), _ptr(top5_ptr), _ptr(prob_views_ptr)))

    def forward_u8_resized_views_dev(self, src_ptr: int, src_bytes: int, descs, full_h: int, full_w: int, mean_ptr: int | None,
                                     views, prob_ptr: int | None = None, top5_ptr: int | None = None,
                                     prob_views_ptr: int | None = None):
        """Asynchronous, device pointers: multi-view inference from 8-bit planar images of ANY size, each resized to
        full_h x full_w on the device (qcnn_forward_u8_resized_views: BmpImgIO::ReszImg, Strict, in front of the mean and the
        views).  descs: a sequence of (offset, h, w) — image i is [C][h][w] at src_ptr + offset (pack_sources makes buffer and
        list); mean [C][full_h][full_w] or None; views as forward_u8_views_dev takes them, cut from the full image.  Neither
        list has to outlive the call."""
        darr, n = _desc_array(descs)
        varr, V = _struct_array(capi.QcnnView, views)
        self._chk(self.lib.qcnn_forward_u8_resized_views(self.h, _ptr(src_ptr), src_bytes, darr, n, full_h, full_w, _ptr(mean_ptr),
                                                         varr, V, _ptr(prob_ptr), _ptr(top5_ptr), _ptr(prob_views_ptr)))

    def forward_u8_resized_views_strided_dev(self, src_ptr: int, src_bytes: int, descs, full_h: int, full_w: int,
                                             mean_ptr: int | None, views, prob_ptr: int | None = None,
                                             top5_ptr: int | None = None, prob_views_ptr: int | None = None):
        """forward_u8_resized_views_dev on source images read in place, whatever their layout
        (qcnn_forward_u8_resized_views_strided).  descs: a sequence of SrcPixels — src_planar, src_bmp, pack_bmp_files and
        pack_interleaved make them — or a ready ctypes array of capi.QcnnSrcPixels."""
        darr, n = _pixels_array(descs)
        varr, V = _struct_array(capi.QcnnView, views)
        self._chk(self.lib.qcnn_forward_u8_resized_views_strided(self.h, _ptr(src_ptr), src_bytes, darr, n, full_h, full_w,
                                                                 _ptr(mean_ptr), varr, V, _ptr(prob_ptr), _ptr(top5_ptr),
                                                                 _ptr(prob_views_ptr)))

    def forward_u8_resized_views_yuv_dev(self, src_ptr: int, src_bytes: int, descs, full_h: int, full_w: int, mean_ptr: int | None,
                                         views, prob_ptr: int | None = None, top5_ptr: int | None = None,
                                         prob_views_ptr: int | None = None):
        """forward_u8_resized_views_strided_dev on YCbCr frames read in place (qcnn_forward_u8_resized_views_yuv): bit for bit
        what it returns on the planar B, G, R images the integer conversion makes of the frames.  descs: a sequence of SrcYuv
        — src_yuv_frame and pack_yuv_frames make them — or a ready ctypes array of capi.QcnnSrcYuv."""
        darr, n = _yuv_array(descs)
        varr, V = _struct_array(capi.QcnnView, views)
        self._chk(self.lib.qcnn_forward_u8_resized_views_yuv(self.h, _ptr(src_ptr), src_bytes, darr, n, full_h, full_w, _ptr(mean_ptr),
                                                             varr, V, _ptr(prob_ptr), _ptr(top5_ptr), _ptr(prob_views_ptr)))

    def forward_u8_relaxed_views_yuv_dev(self, src_ptr: int, src_bytes: int, descs, full_h: int, full_w: int,
                                         mean_crop_ptr: int | None, views, prob_ptr: int | None = None,
                                         top5_ptr: int | None = None, prob_views_ptr: int | None = None):
        """forward_u8_relaxed_views_strided_dev on YCbCr frames read in place (qcnn_forward_u8_relaxed_views_yuv); descs as
        forward_u8_resized_views_yuv_dev takes them."""
        darr, n = _yuv_array(descs)
        varr, V = _struct_array(capi.QcnnAnchorView, views)
        self._chk(self.lib.qcnn_forward_u8_relaxed_views_yuv(self.h, _ptr(src_ptr), src_bytes, darr, n, full_h, full_w,
                                                             _ptr(mean_crop_ptr), varr, V, _ptr(prob_ptr), _ptr(top5_ptr),
                                                             _ptr(prob_views_ptr)))

    def forward_u8_resized_host(self, images, full_hw, mean=None, views=None, descs=None):
        """Blocking convenience: images — a list of uint8 arrays [C][h][w] of differing sizes — are packed, uploaded, resized
        to full_hw = (full_h, full_w) on the device, the float32 mean [C][full_h][full_w] (or None) subtracted, and evaluated on
        `views` (default: the centre crop alone, which makes the call BmpImgIO::Load + the forward pass).  With images = None
        and descs = (flat, descs) — a uint8 buffer and the SrcPixels of the images in it, as pack_bmp_files / pack_interleaved
        give them, or the SrcYuv of YCbCr frames (pack_yuv_frames; one kind per call) — the buffer is uploaded untouched and read
        in place.  Returns (prob [n][classes] averaged over the views,
        top5 [n][5], prob_views [n][len(views)][classes]) as numpy arrays."""
        full_h, full_w = int(full_hw[0]), int(full_hw[1])
        _, in_h, in_w = self.in_chw
        if views is None:
            views = [((full_h - in_h) // 2, (full_w - in_w) // 2, 0)]
        call = (self.forward_u8_resized_views_dev if descs is None else
                self.forward_u8_resized_views_yuv_dev if _is_yuv(list(descs[1])) else self.forward_u8_resized_views_strided_dev)
        return self._u8_host(call, images, full_h, full_w, mean, "mean image", (self.in_chw[0], full_h, full_w), views, descs)

    def forward_u8_relaxed_views_dev(self, src_ptr: int, src_bytes: int, descs, full_h: int, full_w: int, mean_crop_ptr: int | None,
                                     views, prob_ptr: int | None = None, top5_ptr: int | None = None,
                                     prob_views_ptr: int | None = None):
        """Asynchronous, device pointers: multi-view inference from 8-bit planar images of ANY size in the reference's Relaxed /
        Crop mode (qcnn_forward_u8_relaxed_views; VggCnnS): each image resized by one scale towards full_h x full_w — its full
        size is its own, relaxed_full_size gives it — cropped, a mean of the crop's size subtracted.  descs as
        forward_u8_resized_views_dev takes them; mean_crop [C][in_h][in_w] or None; views: a sequence of (ay, ax, dy, dx, flip)
        (ten_crop_anchored gives the standard ten; (1, 1, 0, 0, 0) is BmpImgIO's centre crop).  Neither list has to outlive
        the call."""
        darr, n = _desc_array(descs)
        varr, V = _struct_array(capi.QcnnAnchorView, views)
        self._chk(self.lib.qcnn_forward_u8_relaxed_views(self.h, _ptr(src_ptr), src_bytes, darr, n, full_h, full_w,
                                                         _ptr(mean_crop_ptr), varr, V, _ptr(prob_ptr), _ptr(top5_ptr),
                                                         _ptr(prob_views_ptr)))

    def forward_u8_relaxed_views_strided_dev(self, src_ptr: int, src_bytes: int, descs, full_h: int, full_w: int,
                                             mean_crop_ptr: int | None, views, prob_ptr: int | None = None,
                                             top5_ptr: int | None = None, prob_views_ptr: int | None = None):
        """forward_u8_relaxed_views_dev on source images read in place (qcnn_forward_u8_relaxed_views_strided); descs as
        forward_u8_resized_views_strided_dev takes them."""
        darr, n = _pixels_array(descs)
        varr, V = _struct_array(capi.QcnnAnchorView, views)
        self._chk(self.lib.qcnn_forward_u8_relaxed_views_strided(self.h, _ptr(src_ptr), src_bytes, darr, n, full_h, full_w,
                                                                 _ptr(mean_crop_ptr), varr, V, _ptr(prob_ptr), _ptr(top5_ptr),
                                                                 _ptr(prob_views_ptr)))

    def forward_u8_relaxed_host(self, images, full_hw, mean_crop=None, views=None, descs=None):
        """Blocking convenience: images — a list of uint8 arrays [C][h][w] of differing sizes — are packed, uploaded, resized
        by one scale each towards full_hw = (full_h, full_w) on the device, cropped, the float32 mean_crop [C][in_h][in_w] (or
        None) subtracted, and evaluated on `views` (default: the centre anchor alone, which makes the call BmpImgIO::Load of a
        Relaxed / Crop model + the forward pass).  images = None and descs = (flat, descs): as forward_u8_resized_host.
        Returns (prob [n][classes] averaged over the views, top5 [n][5], prob_views [n][len(views)][classes]) as numpy
        arrays."""
        if views is None:
            views = [(1, 1, 0, 0, 0)]
        call = (self.forward_u8_relaxed_views_dev if descs is None else
                self.forward_u8_relaxed_views_yuv_dev if _is_yuv(list(descs[1])) else self.forward_u8_relaxed_views_strided_dev)
        return self._u8_host(call, images, int(full_hw[0]), int(full_hw[1]), mean_crop, "crop mean", tuple(self.in_chw), views, descs)

    def _u8_host(self, call, images, full_h, full_w, mean, mean_name, mean_shape, views, given=None):
        """The blocking 8-bit calls around their asynchronous one: pack (or take the caller's buffer and descriptors) and
        upload, `call`, wait, download."""
        import torch   # plumbing only: device buffers and copies
        if given is not None and images is not None:
            raise ValueError("images and descs=(flat, descs) exclude each other")
        if given is not None:
            flat, descs = np.asarray(given[0]), list(given[1])
            if flat.dtype != np.uint8 or flat.ndim != 1 or not flat.size or not descs:
                raise ValueError("descs=(flat, descs): a non-empty one-dimensional uint8 buffer and its descriptors")
            flat = np.ascontiguousarray(flat)
        else:
            flat, descs = pack_sources(images)
        n, V = len(descs), len(views)
        fh, fw, fc = self.fm_dims(self.L)
        classes = fh * fw * fc
        dev = torch.device("cuda", self.lib.qcnn_ctx_device(self.h))
        d_src = torch.from_numpy(flat).to(dev)
        d_mean = torch.from_numpy(np.ascontiguousarray(mean, np.float32)).to(dev) if mean is not None else None
        if d_mean is not None and tuple(d_mean.shape) != mean_shape:
            raise QcnnError("%s %r, expected %r" % (mean_name, tuple(d_mean.shape), mean_shape))
        d_prob = torch.empty((n, classes), dtype=torch.float32, device=dev)
        d_top5 = torch.empty((n, 5), dtype=torch.int16, device=dev)
        d_rows = torch.empty((n, max(V, 1), classes), dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        call(d_src.data_ptr(), flat.size, descs, full_h, full_w, d_mean.data_ptr() if d_mean is not None else None, views,
             d_prob.data_ptr(), d_top5.data_ptr(), d_rows.data_ptr())
        self.sync()
        return d_prob.cpu().numpy(), d_top5.cpu().numpy().view(np.uint16), d_rows.cpu().numpy()

    def forward_host(self, imgs_nchw, want_prob=True, want_top5=True):
        imgs = np.ascontiguousarray(imgs_nchw, np.float32)
        n = imgs.shape[0]
        h, w, c = self.fm_dims(self.L)
        prob = np.empty((n, h * w * c), np.float32) if want_prob else None
        top5 = np.empty((n, 5), np.uint16) if want_top5 else None
        self._chk(self.lib.qcnn_forward_host(self.h, imgs.ctypes.data, n,
                                             prob.ctypes.data if want_prob else None,
                                             top5.ctypes.data if want_top5 else None))
        return prob, top5

    def forward_host_batches(self, batches, want_prob=True, want_top5=True):
        """Blocking: a list of [n_b, C, H, W] float32 arrays, one batch after the other with the upload of batch b + 1
        overlapped with the layers of batch b (qcnn_forward_host_batches).  Returns ([prob_b], [top5_b])."""
        return _host_batches(self.lib.qcnn_forward_host_batches, self, batches, self.fm_dims(self.L), want_prob, want_top5)

    def forward_u8_host_batches_into(self, batches, full_hw, mean_ptr, views, mode, outs, labels=None, hits5=None):
        """The streamed 8-bit call on the caller's arrays (qcnn_forward_u8_resized_host_batches for mode "strict",
        qcnn_forward_u8_relaxed_host_batches for "relaxed"); blocking.  batches: [(flat, descs)] — a one-dimensional uint8
        array in host memory of any kind and the SrcPixels of the images in it, or the SrcYuv of YCbCr frames (then the _yuv
        entry points run; one kind per call); mean_ptr: a DEVICE pointer or None; outs: per
        batch (prob, top5, prob_views), each a C-contiguous numpy array that is written or None; labels: per batch a uint16
        array of one class per image or None (batch not counted), or None altogether; hits5: a uint64 array [5] that receives
        the per-rank hit counts, or None (nothing is counted).  A refused call leaves every array as it was."""
        if mode not in ("strict", "relaxed"):
            raise ValueError("mode is 'strict' or 'relaxed'")
        nb = len(batches)
        if len(outs) != nb or (labels is not None and len(labels) != nb):
            raise ValueError("outs and labels hold one entry per batch")
        yuv = {_is_yuv(descs) for _, descs in batches}
        if len(yuv) > 1:
            raise ValueError("the descriptors of one call are SrcPixels or SrcYuv, not both")
        yuv = yuv == {True}
        batch_t, to_array, tag = (capi.QcnnU8YuvBatch, _yuv_array, "_yuv") if yuv else (capi.QcnnU8Batch, _pixels_array, "")
        arr = (batch_t * max(nb, 1))()
        keep = []                                     # the descriptor arrays and label copies live as long as the call
        addr = lambda a: a.ctypes.data if a is not None else None
        for b, ((flat, descs), (prob, top5, rows)) in enumerate(zip(batches, outs)):
            if flat is not None and (not isinstance(flat, np.ndarray) or flat.dtype != np.uint8 or flat.ndim != 1 or not flat.flags["C_CONTIGUOUS"]):
                raise ValueError("batch %d: the source buffer is a C-contiguous one-dimensional uint8 array" % b)
            darr, n = to_array(descs)
            lab = labels[b] if labels is not None else None
            if lab is not None:
                lab = np.ascontiguousarray(lab, np.uint16)
                if lab.shape != (n,):
                    raise ValueError("batch %d: %d labels for %d images" % (b, lab.size, n))
            keep.append((darr, lab))
            arr[b] = batch_t(addr(flat), flat.size if flat is not None else 0, darr, n, addr(lab), addr(prob), addr(top5), addr(rows))
        if hits5 is not None and (hits5.dtype != np.uint64 or hits5.shape != (5,) or not hits5.flags["C_CONTIGUOUS"]):
            raise ValueError("hits5 is a uint64 array [5]")
        hp = hits5.ctypes.data_as(C.POINTER(C.c_ulonglong)) if hits5 is not None else None
        full_h, full_w = int(full_hw[0]), int(full_hw[1])
        if mode == "strict":
            varr, V = _struct_array(capi.QcnnView, views)
            self._chk(getattr(self.lib, "qcnn_forward_u8_resized_host_batches" + tag)(self.h, arr, nb, full_h, full_w, _ptr(mean_ptr), varr, V, hp))
        else:
            varr, V = _struct_array(capi.QcnnAnchorView, views)
            self._chk(getattr(self.lib, "qcnn_forward_u8_relaxed_host_batches" + tag)(self.h, arr, nb, full_h, full_w, _ptr(mean_ptr), varr, V, hp))

    def forward_u8_host_batches(self, batches, full_hw, mean=None, views=None, mode="strict", labels=None, want=(True, True, False)):
        """Blocking: batches of 8-bit source images streamed from host memory, the upload of batch b + 1 under the layers of
        batch b (qcnn_forward_u8_*_host_batches).  batches: [(flat, descs)] as pack_bmp_files / pack_interleaved / pack_sources
        + src_planar or pack_yuv_frames give them; full_hw, views and mean (float32 [C][full_h][full_w], "relaxed": [C][in_h][in_w]; or None) as
        forward_u8_resized_host / forward_u8_relaxed_host take them (default view: the centre); labels: per batch one class per
        image or None.  want = (prob, top5, prob_views).  Returns ([prob_b], [top5_b], [prob_views_b], hits5): per batch prob
        [n][classes] and top5 [n][5] of the view average and prob_views [n][len(views)][classes] — a list that is not wanted is
        None — and hits5, uint64 [5], or None without labels: hits5[r] = labelled images whose r-th prediction is their label,
        every rank by itself (CaffeEva::CalcPredAccu before its running sum; ACCURACY@k is hits5[:k].sum() over the labelled
        images: evaluate_u8).  numpy in, numpy out; torch only holds the mean on the device."""
        full_h, full_w = int(full_hw[0]), int(full_hw[1])
        _, in_h, in_w = self.in_chw
        if views is None:
            views = [((full_h - in_h) // 2, (full_w - in_w) // 2, 0)] if mode == "strict" else [(1, 1, 0, 0, 0)]
        V = len(views)
        fh, fw, fc = self.fm_dims(self.L)
        classes = fh * fw * fc
        d_mean = None
        if mean is not None:
            import torch   # plumbing only: the mean on the device
            shape = (self.in_chw[0], full_h, full_w) if mode == "strict" else tuple(self.in_chw)
            m = np.ascontiguousarray(mean, np.float32)
            if m.shape != shape:
                raise QcnnError("mean %r, expected %r" % (m.shape, shape))
            dev = torch.device("cuda", self.lib.qcnn_ctx_device(self.h))
            d_mean = torch.from_numpy(m).to(dev)
            torch.cuda.synchronize(dev)
        outs = [(np.empty((len(d), classes), np.float32) if want[0] else None, np.empty((len(d), 5), np.uint16) if want[1] else None,
                 np.empty((len(d), V, classes), np.float32) if want[2] else None) for _, d in batches]
        hits5 = np.zeros(5, np.uint64) if labels is not None else None
        self.forward_u8_host_batches_into(batches, full_hw, d_mean.data_ptr() if d_mean is not None else None, views, mode, outs,
                                          labels, hits5)
        col = lambda j: [o[j] for o in outs] if want[j] else None
        return col(0), col(1), col(2), hits5

    def count_top5_hits_dev(self, top5_ptr: int, labels_ptr: int, n: int, hits_ptr: int):
        """Asynchronous, device pointers (qcnn_count_top5_hits): hits[r] += images i < n whose r-th top-5 entry is labels[i],
        every rank by itself — accumulated into the five uint64 counters at hits_ptr, which the caller zeroes."""
        self._chk(self.lib.qcnn_count_top5_hits(self.h, _ptr(top5_ptr), _ptr(labels_ptr), n, _ptr(hits_ptr)))

    def evaluate_u8(self, sources, labels, full_hw, mean, views=None, mode="strict", batch_images=None, yuv=None):
        """Classify a labelled set of source images — what the reference's Main.cc does with its image files: split_batches +
        forward_u8_host_batches.  sources / labels / yuv as split_batches takes them; batch_images: images per batch (default and
        cap: max_batch // len(views)).  Returns dict(n, hits = the five per-rank counts, accuracy = the five CUMULATIVE
        fractions hits[:k + 1].sum() / n: the numbers Main.cc prints as ACCURACY@1..5)."""
        V = 1 if views is None else len(views)
        per = self.max_batch // max(V, 1)
        if batch_images is not None:
            per = min(per, int(batch_images))
        cut = split_batches(sources, labels, per * V, V, yuv)
        _, _, _, hits = self.forward_u8_host_batches([(f, d) for f, d, _ in cut], full_hw, mean, views, mode, [l for _, _, l in cut],
                                                     want=(False, False, False))
        n = sum(len(d) for _, d, _ in cut)
        return dict(n=n, hits=[int(h) for h in hits], accuracy=[float(int(hits[:k + 1].sum()) / n) for k in range(5)])

    def layer_output(self, l: int, n: int):
        h, w, c = self.fm_dims(l)
        out = np.empty((n, h, w, c), np.float32)
        self._chk(self.lib.qcnn_get_layer_output(self.h, l, n, out.ctypes.data))
        return out

    def layer_output_range(self, l: int, first: int, n: int):
        h, w, c = self.fm_dims(l)
        out = np.empty((n, h, w, c), np.float32)
        self._chk(self.lib.qcnn_get_layer_output_range(self.h, l, first, n, out.ctypes.data))
        return out

    def map_diff(self, ref, l: int, n: int, per_channel: bool = False):
        """Feature map l of this engine's last forward against the same map of ``ref``'s, images [0, n), compared on the device
        (qcnn_map_diff; blocking).  With d = (double)a - (double)b over the pairs whose two values are finite, returns
        dict(count, nonfinite, sum_d, sum_d2, sum_ref2, max_abs_d, rel_err = sqrt(sum_d2 / sum_ref2), mean_d = sum_d / count);
        per_channel=True adds ``channels``: float64 [C][6], the same six sums per channel, whose fold is the total to the bit.
        ``ref`` may hold another model: only the map's dims must agree.  Both engines need OPT_KEEP_ALL = 1 for maps the fast
        path fuses away."""
        tot = capi.QcnnMapDiff()
        rows = None
        if per_channel:
            rows = np.empty((self.fm_dims(l)[2], len(capi.MAP_DIFF_FIELDS)), np.float64)
        rc = self.lib.qcnn_map_diff(self.h, getattr(ref, "h", None), int(l), int(n), C.byref(tot),
                                    rows.ctypes.data if rows is not None else None)
        self._chk(rc)
        out = map_diff_summary({f: float(getattr(tot, f)) for f in capi.MAP_DIFF_FIELDS})
        if per_channel:
            out["channels"] = rows
        return out

    def run_layer(self, l: int, x, n: int):
        x = np.ascontiguousarray(x, np.float32)
        h, w, c = self.fm_dims(l + 1)
        out = np.empty((n, h, w, c), np.float32)
        self._chk(self.lib.qcnn_run_layer(self.h, l, x.ctypes.data, n, out.ctypes.data))
        return out

    def layer_split(self, l: int):
        """(tiles run whole, slices per split tile) of the last launch of conv layer l (QCNN_OPT_SPLIT); slices = 1: no split."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.qcnn_get_layer_split(self.h, l, C.byref(a), C.byref(b)))
        return a.value, b.value

    def layer_dec_form(self, l: int):
        """(form, fallback pairs) of the last launch of a first conv layer read in place: form 0 = f32 matrix instructions,
        1 = three bf16 pieces, 2 = two fp16 pieces (OPT_DEC_BF16SPLIT), -1 = another kernel ran; fallback pairs = the (work
        item, image) pairs form 2's fix-up launch recomputed in form 1 for input values outside its range.  Synchronises."""
        form, pairs = C.c_int(0), C.c_longlong(0)
        self._chk(self.lib.qcnn_get_layer_dec_form(self.h, l, C.byref(form), C.byref(pairs)))
        return form.value, pairs.value

    def layer_segments(self, l: int):
        """Row-segment boundaries of the sliding kernel's last launch of conv layer l ([] = the tile kernel ran)."""
        seg = (C.c_int * 9)()
        n = C.c_int(0)
        self._chk(self.lib.qcnn_get_layer_segments(self.h, l, seg, C.byref(n)))
        return [int(seg[i]) for i in range(n.value + 1)] if n.value > 0 else []

    # -- timing ---------------------------------------------------------------------------------
    def layer_ms(self):
        ms = (C.c_float * self.L)()
        cnt = C.c_int(0)
        self._chk(self.lib.qcnn_get_layer_ms(self.h, ms, C.byref(cnt)))
        return np.array(ms[:], np.float64), cnt.value

    def layer_total_ms(self):
        """(ms summed over every recorded launch, launches) per layer, forwards recorded."""
        tot = (C.c_double * self.L)()
        cnt = (C.c_longlong * self.L)()
        fw = C.c_int(0)
        self._chk(self.lib.qcnn_get_layer_total_ms(self.h, tot, cnt, C.byref(fw)))
        return np.array(tot[:], np.float64), np.array(cnt[:], np.int64), fw.value

    def reset_layer_ms(self):
        self._chk(self.lib.qcnn_reset_layer_ms(self.h))


def map_diff_summary(sums):
    """The six sums of a map_diff row (a dict keyed by capi.MAP_DIFF_FIELDS) plus what is derived from them: rel_err =
    sqrt(sum_d2 / sum_ref2) (0.0 when both are 0, inf when only sum_ref2 is) and mean_d = sum_d / count (0.0 without pairs)."""
    out = {f: float(sums[f]) for f in capi.MAP_DIFF_FIELDS}
    d2, r2 = out["sum_d2"], out["sum_ref2"]
    out["rel_err"] = float(np.sqrt(d2 / r2)) if r2 > 0.0 else (0.0 if d2 == 0.0 else float("inf"))
    out["mean_d"] = out["sum_d"] / out["count"] if out["count"] > 0.0 else 0.0
    return out


def _host_batches(fn, obj, batches, out_hwc, want_prob, want_top5):
    imgs = [np.ascontiguousarray(b, np.float32) for b in batches]
    nb = len(imgs)
    classes = out_hwc[0] * out_hwc[1] * out_hwc[2]
    prob = [np.empty((b.shape[0], classes), np.float32) for b in imgs] if want_prob else None
    top5 = [np.empty((b.shape[0], 5), np.uint16) for b in imgs] if want_top5 else None
    vp = C.c_void_p
    a_in = (vp * nb)(*[b.ctypes.data for b in imgs])
    a_n = (C.c_int * nb)(*[b.shape[0] for b in imgs])
    a_p = (vp * nb)(*[p.ctypes.data for p in prob]) if want_prob else None
    a_t = (vp * nb)(*[t.ctypes.data for t in top5]) if want_top5 else None
    obj._chk(fn(obj.h, a_in, a_n, nb, a_p, a_t))
    return prob, top5


def ten_crop_views(src_h: int, src_w: int, in_h: int, in_w: int):
    """The standard ten views [(oy, ox, flip)] of a src_h x src_w image for an in_h x in_w network (qcnn_views_ten_crop): the
    four corner crops and the centre crop, then their left-right mirrors.  Needs no device."""
    lib = capi.load()
    arr = (capi.QcnnView * 10)()
    if lib.qcnn_views_ten_crop(src_h, src_w, in_h, in_w, arr):
        raise QcnnError("ten_crop_views: a %dx%d source holds no %dx%d crop" % (src_h, src_w, in_h, in_w))
    return [(v.oy, v.ox, v.flip) for v in arr]


def ten_crop_anchored():
    """The standard ten views as anchors [(ay, ax, dy, dx, flip)] for forward_u8_relaxed_views_dev (qcnn_views_ten_crop_anchored):
    four corners, centre, then their mirrors, each resolved against every image's own full size.  Needs no device."""
    lib = capi.load()
    arr = (capi.QcnnAnchorView * 10)()
    if lib.qcnn_views_ten_crop_anchored(arr):
        raise QcnnError("ten_crop_anchored failed")
    return [(v.ay, v.ax, v.dy, v.dx, v.flip) for v in arr]


def relaxed_full_size(h: int, w: int, full_h: int, full_w: int):
    """(Hf, Wf, scale) of an h x w source resized towards full_h x full_w by the reference's Relaxed rule
    (qcnn_relaxed_full_size): its float arithmetic, which can land one pixel under the nominal size.  Needs no device."""
    lib = capi.load()
    hf, wf, s = C.c_int(), C.c_int(), C.c_float()
    if lib.qcnn_relaxed_full_size(int(h), int(w), int(full_h), int(full_w), C.byref(hf), C.byref(wf), C.byref(s)):
        raise QcnnError("relaxed_full_size: %dx%d towards %dx%d is refused (a side under 2, or a full size of 2^24 or more)" % (h, w, full_h, full_w))
    return hf.value, wf.value, np.float32(s.value)


def pack_sources(images):
    """A list of uint8 arrays [C][h][w] of differing sizes (one channel count) -> (flat uint8 buffer with the images back to
    back in order, [(offset, h, w)]): what qcnn_forward_u8_resized_views reads once the buffer is on the device.  Needs no
    device."""
    imgs = list(images)
    if not imgs:
        raise ValueError("pack_sources: no image")
    descs, off = [], 0
    for k, a in enumerate(imgs):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.size == 0:
            raise ValueError("pack_sources: image %d is not a uint8 array [C][h][w]" % k)
        if a.shape[0] != imgs[0].shape[0]:
            raise ValueError("pack_sources: image %d has %d channels, image 0 has %d" % (k, a.shape[0], imgs[0].shape[0]))
        descs.append((off, int(a.shape[1]), int(a.shape[2])))
        off += a.size
    flat = np.empty(off, np.uint8)
    for a, (o, _, _) in zip(imgs, descs):
        flat[o:o + a.size] = a.reshape(-1)
    return flat, descs


def src_planar(offset: int, h: int, w: int, C: int) -> SrcPixels:
    """The SrcPixels of a planar [C][h][w] image at `offset` (qcnn_src_planar): what pack_sources' (offset, h, w) means.  Needs
    no device."""
    return _src_planar(int(offset), int(h), int(w), int(C))


def _src_planar(offset, h, w, channels):              # `C` is ctypes here
    out = capi.QcnnSrcPixels()
    if capi.load().qcnn_src_planar(C.byref(capi.QcnnSrcImage(offset, h, w)), channels, C.byref(out)):
        raise QcnnError("src_planar: %d x %dx%d at offset %d is refused (1 to 4 channels, sides of at least 1, under 2 GiB)" % (channels, h, w, offset))
    return _from_c(out)


def src_bmp(file_bytes, file_offset: int = 0) -> SrcPixels:
    """The SrcPixels of the pixel array of a BMP file whose bytes will lie at `file_offset` of the source buffer (qcnn_src_bmp):
    24 or 32 bits per pixel, uncompressed, bottom-up or top-down — the flavours BmpImgIO decodes.  Needs no device."""
    data = bytes(file_bytes)
    out = capi.QcnnSrcPixels()
    if capi.load().qcnn_src_bmp(data, len(data), int(file_offset), C.byref(out)):
        raise QcnnError("src_bmp: not a BMP file this library reads in place (BM, 24 or 32 bits per pixel, uncompressed, complete)")
    return _from_c(out)


def pack_bmp_files(files):
    """A list of BMP files' contents (bytes) -> (flat uint8 buffer with the files back to back, untouched, [SrcPixels]): what
    the strided calls read once the buffer is on the device.  Needs no device."""
    files = [bytes(f) for f in files]
    if not files:
        raise ValueError("pack_bmp_files: no file")
    descs, off = [], 0
    for k, f in enumerate(files):
        try:
            descs.append(src_bmp(f, off))
        except QcnnError as e:
            raise QcnnError("file %d: %s" % (k, e)) from None
        off += len(f)
    return np.frombuffer(bytearray(b"".join(files)), np.uint8), descs      # a bytearray: the array is writable, as torch wants it


def pack_interleaved(images, order="BGR"):
    """A list of uint8 arrays [h][w][3] (a decoder's output; order: "BGR" or "RGB", the order of the three bytes of a pixel) ->
    (flat uint8 buffer with the arrays back to back, untouched, [SrcPixels]).  Needs no device."""
    if order not in ("BGR", "RGB"):
        raise ValueError("pack_interleaved: order is 'BGR' or 'RGB'")
    imgs = list(images)
    if not imgs:
        raise ValueError("pack_interleaved: no image")
    descs, off = [], 0
    for k, a in enumerate(imgs):
        if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.size == 0:
            raise ValueError("pack_interleaved: image %d is not a uint8 array [h][w][3]" % k)
        h, w = int(a.shape[0]), int(a.shape[1])
        descs.append(SrcPixels(off, 3 * w, h, w, 3, (0, 1, 2, 0) if order == "BGR" else (2, 1, 0, 0)))
        off += a.size
    flat = np.empty(off, np.uint8)
    for a, d in zip(imgs, descs):
        flat[d.offset:d.offset + a.size] = a.reshape(-1)
    return flat, descs


def src_yuv_frame(fmt, offset: int, h: int, w: int, pitch: int = 0, matrix="JFIF") -> SrcYuv:
    """The SrcYuv of a frame in one of the common layouts whose first byte will lie at `offset` of the source buffer
    (qcnn_src_yuv_frame).  fmt: "NV12", "NV21", "I420", "YV12", "I444", "YUY2" or "UYVY"; pitch: bytes between luma rows, 0 =
    tight; matrix: "JFIF" (full-range BT.601, JPEG), "BT601" or "BT709" (limited range).  Needs no device."""
    if fmt not in capi.YUV_FORMATS or matrix not in capi.YUV_MATRICES:
        raise ValueError("src_yuv_frame: format %r / matrix %r; formats %s, matrices %s" % (fmt, matrix, sorted(capi.YUV_FORMATS), sorted(capi.YUV_MATRICES)))
    out = capi.QcnnSrcYuv()
    if capi.load().qcnn_src_yuv_frame(capi.YUV_FORMATS[fmt], int(offset), int(h), int(w), int(pitch), capi.YUV_MATRICES[matrix], C.byref(out)):
        raise QcnnError("src_yuv_frame: a %s frame of %dx%d with pitch %d at offset %d is refused (sides of at least 1, a pitch that holds a "
                        "row, under 2 GiB)" % (fmt, h, w, pitch, offset))
    return SrcYuv(*(int(getattr(out, f)) for f in SrcYuv._fields))


def pack_yuv_frames(frames, fmt, sizes, matrix="JFIF"):
    """A list of YCbCr frames (bytes or one-dimensional uint8 arrays, as a decoder wrote them) -> (flat uint8 buffer with the
    frames back to back, untouched, [SrcYuv]): what the _yuv calls read once the buffer is on the device.  fmt and matrix as
    src_yuv_frame takes them; sizes: (h, w) or (h, w, pitch) per frame.  Needs no device."""
    frames = [np.ascontiguousarray(f, np.uint8).tobytes() if isinstance(f, np.ndarray) else bytes(f) for f in frames]
    sizes = list(sizes)
    if not frames or len(sizes) != len(frames):
        raise ValueError("pack_yuv_frames: %d frames, %d sizes" % (len(frames), len(sizes)))
    descs, off = [], 0
    for k, (f, size) in enumerate(zip(frames, sizes)):
        try:
            d = src_yuv_frame(fmt, off, *size, matrix=matrix) if len(size) == 2 else src_yuv_frame(fmt, off, size[0], size[1], size[2], matrix)
        except QcnnError as e:
            raise QcnnError("frame %d: %s" % (k, e)) from None
        last = max(d.y_offset + (d.h - 1) * d.y_row_stride + (d.w - 1) * d.y_pix_stride,
                   max(d.cb_offset, d.cr_offset) + ((d.h - 1) >> d.sub_y) * d.c_row_stride + ((d.w - 1) >> d.sub_x) * d.c_pix_stride)
        if last >= off + len(f):
            raise QcnnError("frame %d: %d bytes hold no %s frame of %dx%d (its last sample is byte %d)" % (k, len(f), fmt, d.h, d.w, last - off))
        descs.append(d)
        off += len(f)
    return np.frombuffer(bytearray(b"".join(frames)), np.uint8), descs      # a bytearray: the array is writable, as torch wants it


def split_batches(sources, labels, max_batch, n_views, yuv=None):
    """Cut a list of per-image sources and their labels into the batches forward_u8_host_batches streams: every batch holds at
    most max_batch // n_views images (n * n_views <= max_batch), the order is kept, the last batch may be ragged.  sources:
    BMP files' contents (bytes: packed by pack_bmp_files and read in place) or uint8 arrays [C][h][w] (pack_sources +
    src_planar), one kind per call — or, with yuv = (fmt, sizes, matrix), YCbCr frames as pack_yuv_frames takes them; labels: one class per image, or None.  Returns [(flat, descs, labels_b)], labels_b a
    uint16 array or None.  Pure Python: needs no device and pins nothing."""
    srcs = list(sources)
    if not srcs:
        raise ValueError("split_batches: no image")
    per = int(max_batch) // int(n_views) if int(n_views) >= 1 else 0
    if per < 1:
        raise ValueError("split_batches: max_batch %d holds no image of %d views" % (max_batch, n_views))
    lab = None
    if labels is not None:
        lab = np.asarray(labels)
        if lab.shape != (len(srcs),) or lab.dtype.kind not in "iu" or (lab.size and (lab.min() < 0 or lab.max() > 0xFFFF)):
            raise ValueError("split_batches: labels are one class in [0, 65535] per image")
        lab = lab.astype(np.uint16)
    if yuv is not None:
        fmt, sizes, matrix = yuv
        sizes = list(sizes)
        if len(sizes) != len(srcs):
            raise ValueError("split_batches: %d sizes for %d frames" % (len(sizes), len(srcs)))
        return [pack_yuv_frames(srcs[a:a + per], fmt, sizes[a:a + per], matrix) + (lab[a:a + per].copy() if lab is not None else None,)
                for a in range(0, len(srcs), per)]
    files = [isinstance(s, (bytes, bytearray, memoryview)) for s in srcs]
    if any(files) and not all(files):
        raise ValueError("split_batches: sources are BMP files' contents or uint8 arrays [C][h][w], not both")
    out = []
    for a in range(0, len(srcs), per):
        part = srcs[a:a + per]
        if files[0]:
            flat, descs = pack_bmp_files(part)
        else:
            flat, planar = pack_sources(part)
            descs = [_src_planar(off, h, w, int(part[0].shape[0])) for off, h, w in planar]
        out.append((flat, descs, lab[a:a + per].copy() if lab is not None else None))
    return out


def host_alloc(nbytes: int):
    """A uint8 array [nbytes] over pinned host memory of the HIP runtime (qcnn_host_alloc): the fastest source of an upload.
    host_free(arr) releases it; the array must not be used afterwards."""
    lib = capi.load()
    p = C.c_void_p()
    if lib.qcnn_host_alloc(int(nbytes), C.byref(p)):
        raise QcnnError(lib.qcnn_last_error(None).decode())
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(int(nbytes),))


def host_free(arr) -> None:
    lib = capi.load()
    if lib.qcnn_host_free(C.c_void_p(arr.ctypes.data)):
        raise QcnnError(lib.qcnn_last_error(None).decode())


def host_register(arr) -> None:
    """Pin a numpy array's storage (hipHostRegister): uploads from it become asynchronous DMA transfers."""
    lib = capi.load()
    if lib.qcnn_host_register(C.c_void_p(arr.ctypes.data), arr.nbytes):
        raise QcnnError(lib.qcnn_last_error(None).decode())


def host_unregister(arr) -> None:
    lib = capi.load()
    if lib.qcnn_host_unregister(C.c_void_p(arr.ctypes.data)):
        raise QcnnError(lib.qcnn_last_error(None).decode())


class QcnnDeviceGroup:
    """One batch sharded over several GPUs of this process (qcnn_group_* of include/qcnn_hip.h): contiguous image
    blocks, parameters uploaded to rank 0 and broadcast to the others with RCCL, one host thread per GPU."""

    def __init__(self, devices=None):
        self.lib = capi.load()
        h = C.c_void_p()
        if devices:
            arr = (C.c_int * len(devices))(*devices)
            rc = self.lib.qcnn_group_create(arr, len(devices), C.byref(h))
        else:
            rc = self.lib.qcnn_group_create(None, 0, C.byref(h))
        if rc:
            raise QcnnError(self.lib.qcnn_group_last_error(None).decode())
        self.h = h
        self.size = self.lib.qcnn_group_size(h)
        self.L = 0
        self.classes = 0
        self.broadcast_ms = None

    def _chk(self, rc):
        if rc:
            raise QcnnError(self.lib.qcnn_group_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.qcnn_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, opt, value):
        self._chk(self.lib.qcnn_group_set_option(self.h, opt, value))

    def shard_bounds(self, n, rank):
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.lib.qcnn_group_shard_bounds(self.h, n, rank, C.byref(a), C.byref(b)))
        return a.value, a.value + b.value

    def load_model(self, in_chw, layers, params, max_batch):
        shapes = {i: tuple(int(x) for x in p["ctrd"].shape) for i, p in params.items()}
        arr = (capi.QcnnLayerDesc * len(layers))(*[capi.layer_desc(l) for l in layers])
        self._chk(self.lib.qcnn_group_model_begin(self.h, len(layers), arr, in_chw[0], in_chw[1], in_chw[2]))
        for i, (m, k, cs) in shapes.items():
            self._chk(self.lib.qcnn_group_model_set_layer_shape(self.h, i, m, k, cs))
        self._chk(self.lib.qcnn_group_model_commit(self.h, max_batch))
        for i, p in params.items():
            bias = np.ascontiguousarray(p["bias"], np.float32)
            ctrd = np.ascontiguousarray(p["ctrd"], np.float32)
            asmt = np.ascontiguousarray(p["asmt"], np.uint8)
            self._chk(self.lib.qcnn_group_model_set_layer_params(self.h, i, bias.ctypes.data, ctrd.ctypes.data,
                                                                 asmt.ctypes.data))
        self.broadcast()
        self.L = len(layers)
        d = (C.c_int * 3)()
        self.lib.qcnn_fm_dims(self.lib.qcnn_group_ctx(self.h, 0), self.L, d)
        self.classes = int(d[0]) * int(d[1]) * int(d[2])

    def upload(self, params):
        """Re-upload layers' parameters to rank 0 ({layer: dict(bias, ctrd, asmt)}); broadcast() must follow."""
        for i, p in params.items():
            bias = np.ascontiguousarray(p["bias"], np.float32)
            ctrd = np.ascontiguousarray(p["ctrd"], np.float32)
            asmt = np.ascontiguousarray(p["asmt"], np.uint8)
            self._chk(self.lib.qcnn_group_model_set_layer_params(self.h, i, bias.ctypes.data, ctrd.ctypes.data, asmt.ctypes.data))

    def broadcast(self):
        """Rank 0's arena to every rank (RCCL), verified by a per-rank device checksum (qcnn_group_model_broadcast)."""
        ms = C.c_float(0.0)
        self._chk(self.lib.qcnn_group_model_broadcast(self.h, C.byref(ms)))
        self.broadcast_ms = ms.value

    def arena_checksum(self):
        s2 = (C.c_ulonglong * 2)()
        self._chk(self.lib.qcnn_group_arena_checksum(self.h, s2))
        return int(s2[0]), int(s2[1])

    def forward_host(self, imgs_nchw):
        imgs = np.ascontiguousarray(imgs_nchw, np.float32)
        n = imgs.shape[0]
        prob = np.empty((n, self.classes), np.float32)
        top5 = np.empty((n, 5), np.uint16)
        self._chk(self.lib.qcnn_group_forward_host(self.h, imgs.ctypes.data, n, prob.ctypes.data, top5.ctypes.data))
        return prob, top5

    def forward_dev(self, in_ptrs, n, prob_ptrs=None, top5_ptrs=None):
        """Asynchronous, device-resident (qcnn_group_forward): per-rank device pointers to each rank's block; sync() waits."""
        vp = C.c_void_p
        arr = lambda ptrs: (vp * self.size)(*[vp(p) if p else None for p in ptrs]) if ptrs is not None else None
        self._chk(self.lib.qcnn_group_forward(self.h, arr(in_ptrs), n, arr(prob_ptrs), arr(top5_ptrs)))

    def sync(self):
        self._chk(self.lib.qcnn_group_sync(self.h))

    def forward_host_batches(self, batches, want_prob=True, want_top5=True):
        d = (C.c_int * 3)()
        self.lib.qcnn_fm_dims(self.lib.qcnn_group_ctx(self.h, 0), self.L, d)
        return _host_batches(self.lib.qcnn_group_forward_host_batches, self, batches, (int(d[0]), int(d[1]), int(d[2])),
                             want_prob, want_top5)
