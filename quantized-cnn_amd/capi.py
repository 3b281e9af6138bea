"""ctypes binding of include/qcnn_hip.h (the C-ABI of libqcnn_hip.so).

Loading the library needs no GPU (symbol checks run on CPU); every compute entry point fails with an
error string when no gfx950 device is present — there is no CPU path behind this module.
"""
from __future__ import annotations

import ctypes as C
import os
import re

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QCNN_HIP_LIB") or os.path.join(PKG, "libqcnn_hip.so")   # QCNN_HIP_LIB: an experimental build of the same library
HEADER_PATH = os.path.join(os.path.dirname(PKG), "include", "qcnn_hip.h")

OPT_LUT_MODE, OPT_KEEP_ALL, OPT_PROFILE, OPT_STREAMS, OPT_SMALL_BATCH, OPT_SPLIT, OPT_HOST_CHUNK, OPT_SLIDE, OPT_DECODE, OPT_SYM, OPT_SYM8, OPT_PACKED_FC, OPT_DIRECT_DEC, OPT_HALF8, OPT_DEC_BF16SPLIT = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14
LUT_EXACT, LUT_MFMA, LUT_MFMA_F16, LUT_MFMA_F16ACC = 0, 1, 2, 3
SMALL_BATCH_MAX = 3        # QCNN_SMALL_BATCH_MAX (include/qcnn_hip.h)
DIFF_CHUNK_ROWS = 64       # QCNN_DIFF_CHUNK_ROWS (include/qcnn_hip.h): rows of one channel a workgroup of qcnn_map_diff folds


class QcnnLayerDesc(C.Structure):
    _fields_ = [("type", C.c_int), ("padSiz", C.c_int), ("knlSiz", C.c_int), ("knlCnt", C.c_int),
                ("grpCnt", C.c_int), ("stride", C.c_int), ("nodCnt", C.c_int), ("lrnSiz", C.c_int),
                ("lrnAlp", C.c_float), ("lrnBet", C.c_float), ("lrnIni", C.c_float), ("drpRat", C.c_float)]


MAX_VIEWS = 32             # QCNN_MAX_VIEWS (include/qcnn_hip.h)


class QcnnView(C.Structure):
    _fields_ = [("oy", C.c_int), ("ox", C.c_int), ("flip", C.c_int)]


class QcnnSrcImage(C.Structure):
    """A source image of qcnn_forward_u8_resized_views: planar [C][h][w] 8-bit at `offset` bytes into the source buffer."""
    _fields_ = [("offset", C.c_uint64), ("h", C.c_int32), ("w", C.c_int32)]


class QcnnSrcPixels(C.Structure):
    """A source image of the strided calls, read in place: sample (c, y, x) is the byte at offset + y * row_stride +
    x * pix_stride + ch_offset[c] of the source buffer ((0, 0): the top-left pixel; c in the network's order B, G, R)."""
    _fields_ = [("offset", C.c_uint64), ("row_stride", C.c_int64), ("h", C.c_int32), ("w", C.c_int32),
                ("pix_stride", C.c_int32), ("ch_offset", C.c_int32 * 4)]


YUV_MATRICES = {"JFIF": 0, "BT601": 1, "BT709": 2}                                                 # QCNN_YUV_JFIF ...
YUV_FORMATS = {"NV12": 0, "NV21": 1, "I420": 2, "YV12": 3, "I444": 4, "YUY2": 5, "UYVY": 6}       # QCNN_YUV_NV12 ...


class QcnnSrcYuv(C.Structure):
    """A YCbCr source frame of the _yuv calls, read in place: pixel (y, x) has Y at y_offset + y * y_row_stride + x * y_pix_stride
    and Cb / Cr at cb_offset / cr_offset + (y >> sub_y) * c_row_stride + (x >> sub_x) * c_pix_stride of the source buffer."""
    _fields_ = [("y_offset", C.c_uint64), ("cb_offset", C.c_uint64), ("cr_offset", C.c_uint64), ("y_row_stride", C.c_int64),
                ("c_row_stride", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("y_pix_stride", C.c_int32),
                ("c_pix_stride", C.c_int32), ("sub_y", C.c_int32), ("sub_x", C.c_int32), ("matrix", C.c_int32)]


class QcnnMapDiff(C.Structure):
    """One row of qcnn_map_diff (a channel, or the total): six doubles, 48 bytes."""
    _fields_ = [("count", C.c_double), ("nonfinite", C.c_double), ("sum_d", C.c_double), ("sum_d2", C.c_double),
                ("sum_ref2", C.c_double), ("max_abs_d", C.c_double)]


MAP_DIFF_FIELDS = tuple(f for f, _ in QcnnMapDiff._fields_)


class QcnnAnchorView(C.Structure):
    """A view of qcnn_forward_u8_relaxed_views, placed relative to each image's own full size: anchor 0 / 1 / 2 = near edge /
    CropImg's centre / far edge on each axis, plus dy / dx pixels; flip: mirrored left-right."""
    _fields_ = [("ay", C.c_int), ("ax", C.c_int), ("dy", C.c_int), ("dx", C.c_int), ("flip", C.c_int)]


class QcnnU8Batch(C.Structure):
    """One batch of qcnn_forward_u8_*_host_batches: its source bytes in host memory as they lie, n descriptors with offsets
    relative to src_host, n labels or NULL (batch not counted), and the three host outputs, each of which may be NULL."""
    _fields_ = [("src_host", C.c_void_p), ("src_bytes", C.c_size_t), ("imgs", C.POINTER(QcnnSrcPixels)), ("n", C.c_int),
                ("labels", C.c_void_p), ("prob_host", C.c_void_p), ("top5_host", C.c_void_p), ("prob_views_host", C.c_void_p)]


class QcnnU8YuvBatch(C.Structure):
    """QcnnU8Batch with YCbCr descriptors (qcnn_forward_u8_*_host_batches_yuv)."""
    _fields_ = [("src_host", C.c_void_p), ("src_bytes", C.c_size_t), ("imgs", C.POINTER(QcnnSrcYuv)), ("n", C.c_int),
                ("labels", C.c_void_p), ("prob_host", C.c_void_p), ("top5_host", C.c_void_p), ("prob_views_host", C.c_void_p)]


def layer_desc(ly: dict) -> QcnnLayerDesc:
    return QcnnLayerDesc(ly["type"], ly.get("pad", 0), ly.get("knl", 0), ly.get("cnt", 0), ly.get("grp", 0),
                         ly.get("stride", 0), ly.get("nod", 0), ly.get("siz", 0), ly.get("alp", 0.0),
                         ly.get("bet", 0.0), ly.get("ini", 0.0), ly.get("rat", 0.0))


def declared_symbols():
    """Entry points declared in include/qcnn_hip.h (parsed from the header text)."""
    txt = open(HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(qcnn_[a-z0-9_]+)\s*\(", txt)))


_lib = None


def load():
    """dlopen libqcnn_hip.so and set prototypes.  Raises a clear error when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(hipcc --offload-arch=gfx950); there is no fallback path" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i, f32p, u8p, u16p = C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p
    lib.qcnn_abi_version.restype = i
    lib.qcnn_device_count.argtypes = [C.POINTER(i)]
    lib.qcnn_last_error.restype = C.c_char_p
    lib.qcnn_last_error.argtypes = [vp]
    lib.qcnn_ctx_create.argtypes = [i, vp, C.POINTER(vp)]
    lib.qcnn_ctx_destroy.argtypes = [vp]
    lib.qcnn_set_option.argtypes = [vp, i, i]
    lib.qcnn_sync.argtypes = [vp]
    lib.qcnn_model_begin.argtypes = [vp, i, C.POINTER(QcnnLayerDesc), i, i, i]
    lib.qcnn_model_set_layer_shape.argtypes = [vp, i, i, i, i]
    lib.qcnn_model_set_layer_dense.argtypes = [vp, i]
    lib.qcnn_model_set_layer_weights.argtypes = [vp, i, f32p, f32p]
    lib.qcnn_group_model_set_layer_dense.argtypes = [vp, i]
    lib.qcnn_group_model_set_layer_weights.argtypes = [vp, i, f32p, f32p]
    lib.qcnn_model_arena_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    lib.qcnn_model_commit.argtypes = [vp, i, vp]
    lib.qcnn_model_set_layer_params.argtypes = [vp, i, f32p, f32p, u8p]
    lib.qcnn_model_set_layer_params_cbn.argtypes = [vp, i, f32p, f32p, u8p, C.c_size_t, i]
    lib.qcnn_model_mark_loaded.argtypes = [vp]
    lib.qcnn_fm_dims.argtypes = [vp, i, C.POINTER(i)]
    lib.qcnn_forward.argtypes = [vp, f32p, i, f32p, u16p]
    lib.qcnn_forward_u8.argtypes = [vp, u8p, i, i, f32p, i, f32p, u16p]
    lib.qcnn_views_ten_crop.argtypes = [i, i, i, i, C.POINTER(QcnnView)]
    lib.qcnn_forward_u8_views.argtypes = [vp, u8p, i, i, f32p, i, C.POINTER(QcnnView), i, f32p, u16p, f32p]
    lib.qcnn_forward_u8_resized_views.argtypes = [vp, u8p, C.c_size_t, C.POINTER(QcnnSrcImage), i, i, i, f32p, C.POINTER(QcnnView), i,
                                                  f32p, u16p, f32p]
    lib.qcnn_views_ten_crop_anchored.argtypes = [C.POINTER(QcnnAnchorView)]
    lib.qcnn_relaxed_full_size.argtypes = [i, i, i, i, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_float)]
    lib.qcnn_forward_u8_relaxed_views.argtypes = [vp, u8p, C.c_size_t, C.POINTER(QcnnSrcImage), i, i, i, f32p, C.POINTER(QcnnAnchorView), i,
                                                  f32p, u16p, f32p]
    lib.qcnn_src_planar.argtypes = [C.POINTER(QcnnSrcImage), i, C.POINTER(QcnnSrcPixels)]
    lib.qcnn_src_bmp.argtypes = [C.c_char_p, C.c_size_t, C.c_uint64, C.POINTER(QcnnSrcPixels)]
    lib.qcnn_forward_u8_resized_views_strided.argtypes = [vp, u8p, C.c_size_t, C.POINTER(QcnnSrcPixels), i, i, i, f32p,
                                                          C.POINTER(QcnnView), i, f32p, u16p, f32p]
    lib.qcnn_forward_u8_relaxed_views_strided.argtypes = [vp, u8p, C.c_size_t, C.POINTER(QcnnSrcPixels), i, i, i, f32p,
                                                          C.POINTER(QcnnAnchorView), i, f32p, u16p, f32p]
    lib.qcnn_src_yuv_frame.argtypes = [i, C.c_uint64, i, i, C.c_int64, i, C.POINTER(QcnnSrcYuv)]
    lib.qcnn_forward_u8_resized_views_yuv.argtypes = [vp, u8p, C.c_size_t, C.POINTER(QcnnSrcYuv), i, i, i, f32p, C.POINTER(QcnnView), i,
                                                      f32p, u16p, f32p]
    lib.qcnn_forward_u8_relaxed_views_yuv.argtypes = [vp, u8p, C.c_size_t, C.POINTER(QcnnSrcYuv), i, i, i, f32p,
                                                      C.POINTER(QcnnAnchorView), i, f32p, u16p, f32p]
    lib.qcnn_forward_host.argtypes = [vp, f32p, i, f32p, u16p]
    lib.qcnn_forward_host_batches.argtypes = [vp, C.POINTER(vp), C.POINTER(i), i, C.POINTER(vp), C.POINTER(vp)]
    lib.qcnn_forward_u8_resized_host_batches.argtypes = [vp, C.POINTER(QcnnU8Batch), i, i, i, f32p, C.POINTER(QcnnView), i,
                                                         C.POINTER(C.c_ulonglong)]
    lib.qcnn_forward_u8_relaxed_host_batches.argtypes = [vp, C.POINTER(QcnnU8Batch), i, i, i, f32p, C.POINTER(QcnnAnchorView), i,
                                                         C.POINTER(C.c_ulonglong)]
    lib.qcnn_forward_u8_resized_host_batches_yuv.argtypes = [vp, C.POINTER(QcnnU8YuvBatch), i, i, i, f32p, C.POINTER(QcnnView), i,
                                                             C.POINTER(C.c_ulonglong)]
    lib.qcnn_forward_u8_relaxed_host_batches_yuv.argtypes = [vp, C.POINTER(QcnnU8YuvBatch), i, i, i, f32p, C.POINTER(QcnnAnchorView), i,
                                                             C.POINTER(C.c_ulonglong)]
    lib.qcnn_count_top5_hits.argtypes = [vp, u16p, u16p, i, vp]
    lib.qcnn_host_register.argtypes = [vp, C.c_size_t]
    lib.qcnn_host_unregister.argtypes = [vp]
    lib.qcnn_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    lib.qcnn_host_free.argtypes = [vp]
    lib.qcnn_get_layer_output.argtypes = [vp, i, i, f32p]
    lib.qcnn_get_layer_output_range.argtypes = [vp, i, i, i, f32p]
    lib.qcnn_map_diff.argtypes = [vp, vp, i, i, C.POINTER(QcnnMapDiff), vp]
    lib.qcnn_run_layer.argtypes = [vp, i, f32p, i, f32p]
    lib.qcnn_get_layer_split.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
    lib.qcnn_get_layer_dec_form.argtypes = [vp, i, C.POINTER(i), C.POINTER(C.c_longlong)]
    lib.qcnn_get_layer_segments.argtypes = [vp, i, C.POINTER(i), C.POINTER(i)]
    lib.qcnn_get_layer_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(i)]
    lib.qcnn_reset_layer_ms.argtypes = [vp]
    lib.qcnn_get_layer_total_ms.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong), C.POINTER(i)]
    lib.qcnn_ctx_device.argtypes = [vp]
    lib.qcnn_ctx_stream.argtypes = [vp]
    lib.qcnn_ctx_stream.restype = vp
    lib.qcnn_model_arena_ptr.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.qcnn_model_arena_checksum.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    lib.qcnn_quantize_layer.argtypes = [vp, i, i, i, i, i, i, i, f32p, f32p, i, f32p, u8p, C.POINTER(C.c_double), C.POINTER(i)]
    lib.qcnn_calib_gram.argtypes = [vp, i, i, i, i, i, i, i, i, f32p, i, vp, i]
    lib.qcnn_calib_begin.argtypes = [vp, C.POINTER(i), i]
    lib.qcnn_calib_arm.argtypes = [vp, i]
    lib.qcnn_calib_read.argtypes = [vp, i, vp, C.POINTER(C.c_longlong)]
    lib.qcnn_calib_end.argtypes = [vp]
    lib.qcnn_quantize_layer_ec.argtypes = [vp, i, i, i, i, i, i, i, i, f32p, vp, f32p, u8p, i, C.c_double, f32p, u8p, C.POINTER(C.c_double),
                                           C.POINTER(i)]
    lib.qcnn_plan_conv_query.argtypes = [C.POINTER(i), C.POINTER(i), C.POINTER(C.c_double), C.POINTER(i)]
    # device group
    lib.qcnn_group_create.argtypes = [C.POINTER(i), i, C.POINTER(vp)]
    lib.qcnn_group_destroy.argtypes = [vp]
    lib.qcnn_group_last_error.restype = C.c_char_p
    lib.qcnn_group_last_error.argtypes = [vp]
    lib.qcnn_group_size.argtypes = [vp]
    lib.qcnn_group_ctx.argtypes = [vp, i]
    lib.qcnn_group_ctx.restype = vp
    lib.qcnn_group_shard_bounds.argtypes = [vp, i, i, C.POINTER(i), C.POINTER(i)]
    lib.qcnn_group_set_option.argtypes = [vp, i, i]
    lib.qcnn_group_model_begin.argtypes = [vp, i, C.POINTER(QcnnLayerDesc), i, i, i]
    lib.qcnn_group_model_set_layer_shape.argtypes = [vp, i, i, i, i]
    lib.qcnn_group_model_commit.argtypes = [vp, i]
    lib.qcnn_group_model_set_layer_params.argtypes = [vp, i, f32p, f32p, u8p]
    lib.qcnn_group_model_broadcast.argtypes = [vp, C.POINTER(C.c_float)]
    lib.qcnn_group_arena_checksum.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    lib.qcnn_group_forward_host.argtypes = [vp, f32p, i, f32p, u16p]
    lib.qcnn_group_forward_host_batches.argtypes = [vp, C.POINTER(vp), C.POINTER(i), i, C.POINTER(vp), C.POINTER(vp)]
    lib.qcnn_group_forward.argtypes = [vp, C.POINTER(vp), i, C.POINTER(vp), C.POINTER(vp)]
    lib.qcnn_group_sync.argtypes = [vp]
    _lib = lib
    return lib
