// Host side of the YCbCr source frames (QcnnSrcYuv, include/qcnn_hip.h): the layout validator of
// qcnn_forward_u8_resized_views_yuv / _relaxed_views_yuv and the descriptor constructor qcnn_src_yuv_frame.  Plain C++, no HIP
// header: the engine includes it, and tests/yuv_layout_sanitize_main.cc compiles it alone under ASan / UBSan.  Every sum and
// product of caller-supplied values is overflow-checked: nothing wraps, nothing is undefined.
#ifndef QCNN_SRC_YUV_H_
#define QCNN_SRC_YUV_H_

#include <stdint.h>
#include <stdio.h>

#include "../../include/qcnn_hip.h"

namespace qcnn_yuv {

// The relative offsets the kernels form — every sample of all three planes against luma sample (0, 0) — stay in signed 32 bits.
const int64_t kMaxSpan = INT32_MAX;

// The six integers of a matrix (include/qcnn_hip.h has the table): y0, ky, crv, cbg, crg, cbu.  nullptr: unknown matrix.
inline const int32_t* matrix_ints(int matrix) {
  static const int32_t table[3][6] = {{0, 65536, 91881, 22554, 46802, 116130},      // QCNN_YUV_JFIF
                                      {16, 76309, 104597, 25675, 53279, 132201},    // QCNN_YUV_BT601
                                      {16, 76309, 117489, 13975, 34925, 138438}};   // QCNN_YUV_BT709
  return matrix >= 0 && matrix < 3 ? table[matrix] : nullptr;
}

// One plane — rows x cols samples from `offset`, strides rs / ps (ps >= 1) — against a buffer of src_bytes bytes: its lowest and
// highest byte.  0 = inside; 1 = it spans 2^31 - 1 bytes or more (or a product left 64 bits); 2 = below the buffer; 3 = beyond it.
inline int plane_span(uint64_t offset, int64_t rows, int64_t cols, int64_t rs, int32_t ps, size_t src_bytes, uint64_t* lowest,
                      uint64_t* highest) {
  int64_t rowSpan = 0, lo = 0, hi = 0, span = 0;
  const int64_t colSpan = (cols - 1) * (int64_t)ps;                        // < 2^62
  if (__builtin_mul_overflow(rows - 1, rs, &rowSpan)) return 1;
  lo = rowSpan < 0 ? rowSpan : 0;
  if (__builtin_add_overflow(rowSpan < 0 ? (int64_t)0 : rowSpan, colSpan, &hi) || __builtin_sub_overflow(hi, lo, &span) || span >= kMaxSpan)
    return 1;
  // from here on -2^31 < lo <= 0 <= hi < 2^31
  const uint64_t below = (uint64_t)(-lo);
  if (offset < below) return 2;
  if (__builtin_add_overflow(offset, (uint64_t)hi, highest) || *highest >= (uint64_t)src_bytes) return 3;
  *lowest = offset - below;
  return 0;
}

// Descriptor `s` against a network of C input channels and a source buffer of src_bytes bytes; minSide = 1 (Strict) or 2
// (Relaxed).  0 = good; non-zero with the reason in msg (no image number: the caller names the image).
inline int check_yuv(const QcnnSrcYuv& s, int C, size_t src_bytes, int minSide, char* msg, size_t msgLen) {
  if (C != 3) {
    snprintf(msg, msgLen, "a YCbCr source makes the 3 channels B, G, R, the network has %d", C);
    return 1;
  }
  if (s.h < minSide || s.w < minSide) {
    if (minSide < 2) snprintf(msg, msgLen, "size %dx%d", s.h, s.w);
    else snprintf(msg, msgLen, "size %dx%d, the one scale of a relaxed resize needs two pixels a side", s.h, s.w);
    return 1;
  }
  if (s.y_pix_stride < 1 || s.c_pix_stride < 1) {
    snprintf(msg, msgLen, "%s %d is below 1", s.y_pix_stride < 1 ? "y_pix_stride" : "c_pix_stride", s.y_pix_stride < 1 ? s.y_pix_stride : s.c_pix_stride);
    return 1;
  }
  if (s.sub_y < 0 || s.sub_y > 1 || s.sub_x < 0 || s.sub_x > 1) {
    snprintf(msg, msgLen, "sub_y %d, sub_x %d: the chroma sub-sampling shifts are 0 or 1", s.sub_y, s.sub_x);
    return 1;
  }
  if (!matrix_ints(s.matrix)) {
    snprintf(msg, msgLen, "matrix %d is none of QCNN_YUV_JFIF, _BT601, _BT709", s.matrix);
    return 1;
  }
  const int64_t ch = ((int64_t)(s.h - 1) >> s.sub_y) + 1, cw = ((int64_t)(s.w - 1) >> s.sub_x) + 1;
  const struct { const char* name; uint64_t off; int64_t rows, cols, rs; int32_t ps; } planes[3] = {
      {"luma", s.y_offset, s.h, s.w, s.y_row_stride, s.y_pix_stride},
      {"Cb", s.cb_offset, ch, cw, s.c_row_stride, s.c_pix_stride},
      {"Cr", s.cr_offset, ch, cw, s.c_row_stride, s.c_pix_stride}};
  uint64_t lowest = 0, highest = 0;
  int atLow = 0, atHigh = 0;
  for (int p = 0; p < 3; ++p) {
    uint64_t lo = 0, hi = 0;
    const int why = plane_span(planes[p].off, planes[p].rows, planes[p].cols, planes[p].rs, planes[p].ps, src_bytes, &lo, &hi);
    if (why == 1)
      snprintf(msg, msgLen, "the %s plane, %lldx%lld samples with row stride %lld, pix stride %d, spans 2^31 - 1 bytes or more (offsets inside a "
               "frame are 32-bit)", planes[p].name, (long long)planes[p].rows, (long long)planes[p].cols, (long long)planes[p].rs, planes[p].ps);
    else if (why == 2)
      snprintf(msg, msgLen, "the lowest byte of the %s plane lies before offset %llu: below the source buffer (row stride %lld)", planes[p].name,
               (unsigned long long)planes[p].off, (long long)planes[p].rs);
    else if (why == 3)
      snprintf(msg, msgLen, "the %s plane at offset %llu (%lldx%lld samples, row stride %lld, pix stride %d) leaves the source buffer of %llu bytes",
               planes[p].name, (unsigned long long)planes[p].off, (long long)planes[p].rows, (long long)planes[p].cols, (long long)planes[p].rs,
               planes[p].ps, (unsigned long long)src_bytes);
    if (why) return 1;
    if (p == 0 || lo < lowest) { lowest = lo; atLow = p; }
    if (p == 0 || hi > highest) { highest = hi; atHigh = p; }
  }
  if (highest - lowest >= (uint64_t)kMaxSpan) {      // both inside the buffer: no wrap
    snprintf(msg, msgLen, "from the lowest byte of the %s plane (%llu) to the highest of the %s plane (%llu) the frame spans 2^31 - 1 bytes or "
             "more (offsets inside a frame are 32-bit)", planes[atLow].name, (unsigned long long)lowest, planes[atHigh].name, (unsigned long long)highest);
    return 1;
  }
  return 0;
}

// qcnn_src_yuv_frame.
inline int yuv_frame(int format, uint64_t frame_offset, int h, int w, int64_t pitch, int matrix, QcnnSrcYuv* out) {
  if (!out || h < 1 || w < 1 || !matrix_ints(matrix) || format < QCNN_YUV_NV12 || format > QCNN_YUV_UYVY) return 1;
  const int64_t ch = ((int64_t)h + 1) / 2, cw = ((int64_t)w + 1) / 2;      // rows and columns of a 2 x 2 sub-sampled plane
  const bool semi = format == QCNN_YUV_NV12 || format == QCNN_YUV_NV21, packed = format == QCNN_YUV_YUY2 || format == QCNN_YUV_UYVY;
  const int64_t row = packed ? 4 * cw : semi ? 2 * cw : (int64_t)w;        // bytes of the longest row stored at `pitch`
  if (pitch == 0) pitch = row;
  if (pitch < row || pitch > kMaxSpan / h) return 1;                       // the luma plane alone stays below 2^31 bytes: no sum below can wrap
  const int64_t cpitch = (pitch + 1) / 2;                                  // I420 / YV12
  int64_t bytes = 0;
  QcnnSrcYuv d = {};
  d.h = h; d.w = w; d.matrix = matrix;
  d.y_row_stride = pitch;
  d.y_pix_stride = 1;
  const uint64_t luma = (uint64_t)(pitch * h);
  if (semi) {
    bytes = pitch * (h + ch);
    d.c_row_stride = pitch; d.c_pix_stride = 2; d.sub_y = 1; d.sub_x = 1;
    d.cb_offset = luma + (format == QCNN_YUV_NV21 ? 1 : 0);
    d.cr_offset = luma + (format == QCNN_YUV_NV21 ? 0 : 1);
  } else if (format == QCNN_YUV_I420 || format == QCNN_YUV_YV12) {
    bytes = pitch * h + 2 * cpitch * ch;
    d.c_row_stride = cpitch; d.c_pix_stride = 1; d.sub_y = 1; d.sub_x = 1;
    const uint64_t first = luma, second = luma + (uint64_t)(cpitch * ch);
    d.cb_offset = format == QCNN_YUV_I420 ? first : second;
    d.cr_offset = format == QCNN_YUV_I420 ? second : first;
  } else if (format == QCNN_YUV_I444) {
    bytes = 3 * pitch * h;
    d.c_row_stride = pitch; d.c_pix_stride = 1;
    d.cb_offset = luma;
    d.cr_offset = 2 * luma;
  } else {                                                                 // Y0 Cb Y1 Cr / Cb Y0 Cr Y1
    bytes = pitch * h;
    d.y_pix_stride = 2;
    d.c_row_stride = pitch; d.c_pix_stride = 4; d.sub_x = 1;
    d.y_offset = format == QCNN_YUV_YUY2 ? 0 : 1;
    d.cb_offset = format == QCNN_YUV_YUY2 ? 1 : 0;
    d.cr_offset = format == QCNN_YUV_YUY2 ? 3 : 2;
  }
  uint64_t end = 0;
  if (bytes >= kMaxSpan || __builtin_add_overflow(frame_offset, (uint64_t)bytes, &end)) return 1;
  d.y_offset += frame_offset;
  d.cb_offset += frame_offset;
  d.cr_offset += frame_offset;
  *out = d;
  return 0;
}

}  // namespace qcnn_yuv

#endif
