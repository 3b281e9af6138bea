// Host side of the strided source images (QcnnSrcPixels, include/qcnn_hip.h): the layout validator of
// qcnn_forward_u8_resized_views_strided / _relaxed_views_strided and the BMP header parser of qcnn_src_bmp.  Plain C++, no HIP
// header: the engine includes it, and tests/src_layout_sanitize_main.cc compiles it alone under ASan / UBSan.  Every sum and
// product of caller-supplied values is overflow-checked: nothing wraps, nothing is undefined.
#ifndef QCNN_SRC_LAYOUT_H_
#define QCNN_SRC_LAYOUT_H_

#include <stdint.h>
#include <stdio.h>

#include "../../include/qcnn_hip.h"

namespace qcnn_src {

// The relative offsets the kernels form — y * row_stride + x * pix_stride + ch_offset[c] — stay in signed 32 bits.
const int64_t kMaxSpan = INT32_MAX;

// Descriptor `s` of a C-channel image against a source buffer of src_bytes bytes; minSide = 1 (Strict) or 2 (Relaxed).  0 = good;
// non-zero with the reason in msg (no image number: the caller names the image).
inline int check_pixels(const QcnnSrcPixels& s, int C, size_t src_bytes, int minSide, char* msg, size_t msgLen) {
  if (C < 1 || C > 4) {
    snprintf(msg, msgLen, "a strided source has at most 4 channels, the network has %d", C);
    return 1;
  }
  if (s.h < minSide || s.w < minSide) {
    if (minSide < 2) snprintf(msg, msgLen, "size %dx%d", s.h, s.w);
    else snprintf(msg, msgLen, "size %dx%d, the one scale of a relaxed resize needs two pixels a side", s.h, s.w);
    return 1;
  }
  if (s.pix_stride < 1) {
    snprintf(msg, msgLen, "pix_stride %d is below 1", s.pix_stride);
    return 1;
  }
  int64_t maxCh = 0;
  for (int c = 0; c < C; ++c) {
    if (s.ch_offset[c] < 0) {
      snprintf(msg, msgLen, "ch_offset[%d] = %d is negative", c, s.ch_offset[c]);
      return 1;
    }
    if (s.ch_offset[c] > maxCh) maxCh = s.ch_offset[c];
  }
  // relative to `offset`: the rows reach rowSpan = (h-1) * row_stride, the last sample of a row (w-1) * pix_stride + maxCh
  int64_t rowSpan = 0, lo = 0, hi = 0, span = 0;
  const int64_t colSpan = (int64_t)(s.w - 1) * s.pix_stride + maxCh;      // < 2^62 + 2^31
  bool wide = __builtin_mul_overflow((int64_t)(s.h - 1), s.row_stride, &rowSpan);
  if (!wide) {
    lo = rowSpan < 0 ? rowSpan : 0;
    wide = __builtin_add_overflow(rowSpan < 0 ? (int64_t)0 : rowSpan, colSpan, &hi) || __builtin_sub_overflow(hi, lo, &span) ||
           span >= kMaxSpan;
  }
  if (wide) {
    snprintf(msg, msgLen, "%dx%d with row_stride %lld, pix_stride %d spans 2^31 - 1 bytes or more (offsets inside an image are 32-bit)",
             s.h, s.w, (long long)s.row_stride, s.pix_stride);
    return 1;
  }
  // from here on -2^31 < lo <= 0 <= hi < 2^31
  const uint64_t below = (uint64_t)(-lo);
  uint64_t last = 0;
  if (s.offset < below) {
    snprintf(msg, msgLen, "its lowest byte lies %llu bytes before offset %llu: below the source buffer (row_stride %lld)",
             (unsigned long long)below, (unsigned long long)s.offset, (long long)s.row_stride);
    return 1;
  }
  if (__builtin_add_overflow(s.offset, (uint64_t)hi, &last) || last >= (uint64_t)src_bytes) {
    snprintf(msg, msgLen, "bytes up to %llu past offset %llu leave the source buffer of %llu bytes", (unsigned long long)hi,
             (unsigned long long)s.offset, (unsigned long long)src_bytes);
    return 1;
  }
  return 0;
}

// qcnn_src_planar.
inline int planar_pixels(const QcnnSrcImage* img, int C, QcnnSrcPixels* out) {
  if (!img || !out || C < 1 || C > 4 || img->h < 1 || img->w < 1) return 1;
  const int64_t plane = (int64_t)img->h * img->w;
  if (plane > INT32_MAX || plane * C > INT32_MAX) return 1;
  QcnnSrcPixels d = {};
  d.offset = img->offset;
  d.row_stride = img->w;
  d.h = img->h;
  d.w = img->w;
  d.pix_stride = 1;
  for (int c = 0; c < C; ++c) d.ch_offset[c] = (int32_t)(plane * c);
  *out = d;
  return 0;
}

inline uint32_t rd16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t rd32(const uint8_t* p) { return rd16(p) | (rd16(p + 2) << 16); }

// qcnn_src_bmp: the flavours BmpImgIO::decode (host/bmp_img_io.cc) accepts, in its order.
inline int bmp_pixels(const uint8_t* file, size_t file_bytes, uint64_t file_offset, QcnnSrcPixels* out) {
  if (!file || !out || file_bytes < 54 || file[0] != 'B' || file[1] != 'M') return 1;
  const uint32_t dataOff = rd32(file + 10);
  const int32_t wid = (int32_t)rd32(file + 18), heiRaw = (int32_t)rd32(file + 22);
  const uint32_t bpp = rd16(file + 28), compression = rd32(file + 30);
  if ((bpp != 24 && bpp != 32) || compression != 0 || wid <= 0 || heiRaw == 0 || heiRaw == INT32_MIN) return 1;
  const int32_t hei = heiRaw < 0 ? -heiRaw : heiRaw;
  const uint64_t stride = ((uint64_t)wid * (bpp / 8) + 3) & ~(uint64_t)3;   // < 2^34
  uint64_t need = 0, end = 0, first = 0;                                     // stride * hei may pass 2^64
  if (__builtin_mul_overflow(stride, (uint64_t)hei, &need) || __builtin_add_overflow(need, (uint64_t)dataOff, &need) ||
      (uint64_t)file_bytes < need)
    return 1;
  if (__builtin_add_overflow(file_offset, (uint64_t)file_bytes, &end)) return 1;
  QcnnSrcPixels d = {};
  d.h = hei;
  d.w = wid;
  d.pix_stride = (int32_t)(bpp / 8);
  d.ch_offset[0] = 0; d.ch_offset[1] = 1; d.ch_offset[2] = 2; d.ch_offset[3] = 0;
  first = file_offset + dataOff;                                             // <= end: no wrap
  if (heiRaw < 0) {
    d.offset = first;
    d.row_stride = (int64_t)stride;
  } else {
    d.offset = first + (uint64_t)(hei - 1) * stride;                         // inside the file
    d.row_stride = -(int64_t)stride;
  }
  *out = d;
  return 0;
}

}  // namespace qcnn_src

#endif
