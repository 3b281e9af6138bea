// The validator and the descriptor constructor of the YCbCr source frames (quantized-cnn_amd/csrc/qcnn_src_yuv.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer: every accepted and every refused case of include/qcnn_hip.h, the extremes of
// every field among them.  Exit status 0 and the OK line: every case answered as expected and no report.
// Built and run by tests/test_yuv_layout_sanitize.py.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../quantized-cnn_amd/csrc/qcnn_src_yuv.h"

namespace {
int failures = 0;
const size_t kHuge = (size_t)1 << 40;               // a claimed size: nothing is read

QcnnSrcYuv yuv(uint64_t y, uint64_t cb, uint64_t cr, int64_t yrs, int64_t crs, int h, int w, int yps, int cps, int sy, int sx, int matrix = 0) {
  QcnnSrcYuv d;
  memset(&d, 0, sizeof(d));
  d.y_offset = y; d.cb_offset = cb; d.cr_offset = cr; d.y_row_stride = yrs; d.c_row_stride = crs; d.h = h; d.w = w;
  d.y_pix_stride = yps; d.c_pix_stride = cps; d.sub_y = sy; d.sub_x = sx; d.matrix = matrix;
  return d;
}

// `word` (or NULL): what a refusal's message must contain — the plane it names
void expect(const char* what, const QcnnSrcYuv& d, int C, size_t bytes, int minSide, bool good, const char* word = nullptr) {
  char msg[320];
  memset(msg, 0, sizeof(msg));
  const int rc = qcnn_yuv::check_yuv(d, C, bytes, minSide, msg, sizeof(msg));
  if ((rc == 0) != good || (!good && !msg[0]) || (!good && word && !strstr(msg, word))) {
    printf("FAIL %s: rc %d (%s), expected %s%s\n", what, rc, msg, good ? "accepted" : "refused with a message naming ", good || !word ? "" : word);
    ++failures;
  }
}

void frame(const char* what, int format, uint64_t off, int h, int w, int64_t pitch, int matrix, bool good) {
  QcnnSrcYuv d, e;
  memset(&d, 0xEE, sizeof(d));
  memset(&e, 0xEE, sizeof(e));
  const int rc = qcnn_yuv::yuv_frame(format, off, h, w, pitch, matrix, &d);
  bool ok = (rc == 0) == good;
  if (ok && !good) ok = memcmp(&d, &e, sizeof(d)) == 0;                 // refused: nothing written
  if (ok && good) {                                                     // made: the validator accepts it in a buffer that just holds it
    char msg[320];
    uint64_t last = 0;
    const uint64_t ch = (uint64_t)((d.h - 1) >> d.sub_y), cw = (uint64_t)((d.w - 1) >> d.sub_x);
    const uint64_t ends[3] = {d.y_offset + (uint64_t)(d.h - 1) * d.y_row_stride + (uint64_t)(d.w - 1) * d.y_pix_stride,
                              d.cb_offset + ch * d.c_row_stride + cw * d.c_pix_stride, d.cr_offset + ch * d.c_row_stride + cw * d.c_pix_stride};
    for (uint64_t v : ends) last = v > last ? v : last;
    ok = qcnn_yuv::check_yuv(d, 3, (size_t)last + 1, 1, msg, sizeof(msg)) == 0 && qcnn_yuv::check_yuv(d, 3, (size_t)last, 1, msg, sizeof(msg)) != 0;
  }
  if (!ok) {
    printf("FAIL frame %s: rc %d, expected %s\n", what, rc, good ? "a descriptor that exactly fits" : "a refusal that writes nothing");
    ++failures;
  }
}
}  // namespace

int main() {
  // a 6 x 8 I420 frame: luma 48 bytes, two chroma planes of 3 x 4 = 12 bytes: 72 bytes
  const QcnnSrcYuv g = yuv(0, 48, 60, 8, 4, 6, 8, 1, 1, 1, 1);
  expect("i420 exactly fitting", g, 3, 72, 1, true);
  expect("i420 relaxed", g, 3, 72, 2, true);
  expect("i420 in a larger buffer", g, 3, kHuge, 1, true);
  // the last byte exactly fitting and one short, per plane
  expect("Cr one byte short", g, 3, 71, 1, false, "Cr");
  { QcnnSrcYuv d = g; d.cb_offset = 60; d.cr_offset = 48; expect("Cb last: fits", d, 3, 72, 1, true); expect("Cb one byte short", d, 3, 71, 1, false, "Cb"); }
  { QcnnSrcYuv d = g; d.y_offset = 24; d.cb_offset = 0; d.cr_offset = 12; expect("luma last: fits", d, 3, 72, 1, true);
    expect("luma one byte short", d, 3, 71, 1, false, "luma"); }
  // offsets 0, src_bytes and 2^64 - 1, per plane
  { QcnnSrcYuv d = g; d.y_offset = 72; expect("luma at src_bytes", d, 3, 72, 1, false, "luma"); }
  { QcnnSrcYuv d = g; d.cb_offset = 72; expect("Cb at src_bytes", d, 3, 72, 1, false, "Cb"); }
  { QcnnSrcYuv d = g; d.cr_offset = 72; expect("Cr at src_bytes", d, 3, 72, 1, false, "Cr"); }
  { QcnnSrcYuv d = g; d.y_offset = UINT64_MAX; expect("luma at 2^64 - 1", d, 3, kHuge, 1, false, "luma"); }
  { QcnnSrcYuv d = g; d.cb_offset = UINT64_MAX; expect("Cb at 2^64 - 1", d, 3, kHuge, 1, false, "Cb"); }
  { QcnnSrcYuv d = g; d.cr_offset = UINT64_MAX; expect("Cr at 2^64 - 1", d, 3, SIZE_MAX, 1, false, "Cr"); }
  { QcnnSrcYuv d = g; d.cr_offset = UINT64_MAX - 10; expect("Cr + extent wraps", d, 3, SIZE_MAX, 1, false, "Cr"); }
  { QcnnSrcYuv d = yuv(0, 0, 0, 0, 0, 6, 8, 1, 1, 1, 1); expect("all planes at 0, strides 0 (aliased)", d, 3, 8, 1, true);
    expect("... one byte short", d, 3, 7, 1, false, "luma"); }
  // strides INT64_MIN, INT64_MAX and 0
  { QcnnSrcYuv d = g; d.y_row_stride = INT64_MIN; expect("luma stride INT64_MIN", d, 3, kHuge, 1, false, "luma"); }
  { QcnnSrcYuv d = g; d.y_row_stride = INT64_MAX; expect("luma stride INT64_MAX", d, 3, kHuge, 1, false, "luma"); }
  { QcnnSrcYuv d = g; d.c_row_stride = INT64_MIN; expect("chroma stride INT64_MIN", d, 3, kHuge, 1, false, "Cb"); }
  { QcnnSrcYuv d = g; d.c_row_stride = INT64_MAX; expect("chroma stride INT64_MAX", d, 3, kHuge, 1, false, "Cb"); }
  { QcnnSrcYuv d = g; d.y_row_stride = INT64_MIN; d.y_offset = UINT64_MAX; expect("stride INT64_MIN at 2^64 - 1", d, 3, SIZE_MAX, 1, false, "luma"); }
  { QcnnSrcYuv d = yuv(0, 1, 2, INT64_MIN, INT64_MAX, 2, 2, 1, 1, 1, 1); expect("two rows of INT64_MIN", d, 3, kHuge, 1, false, "luma"); }
  { QcnnSrcYuv d = yuv(5, 6, 7, INT64_MIN, INT64_MAX, 1, 8, 1, 1, 1, 1); expect("one row: any stride", d, 3, 20, 1, true); }
  { QcnnSrcYuv d = g; d.y_row_stride = 0; d.c_row_stride = 0; expect("strides 0", d, 3, 72, 1, true); }
  // negative strides: bottom-up planes, and a plane below the buffer
  { QcnnSrcYuv d = yuv(40, 56, 68, -8, -4, 6, 8, 1, 1, 1, 1); expect("bottom-up", d, 3, 72, 1, true);
    d.cb_offset = 7; expect("Cb below the buffer", d, 3, 72, 1, false, "Cb"); d.cb_offset = 8; expect("Cb from byte 0", d, 3, 72, 1, true);
    d.cr_offset = 0; expect("Cr below the buffer", d, 3, 72, 1, false, "Cr"); d.cr_offset = 68; d.y_offset = 39;
    expect("luma below the buffer", d, 3, 72, 1, false, "luma"); }
  // a span of exactly 2^31 - 2 (accepted) and of 2^31 - 1 (refused): inside one plane, and over all three
  { const int64_t p = ((int64_t)1 << 31) - 2;      // two rows, one column: span = the stride
    expect("luma spans 2^31 - 2", yuv(0, 0, 0, p, 0, 2, 1, 1, 1, 0, 0), 3, kHuge, 1, true);
    expect("luma spans 2^31 - 1", yuv(0, 0, 0, p + 1, 0, 2, 1, 1, 1, 0, 0), 3, kHuge, 1, false, "luma");
    expect("Cb spans 2^31 - 1", yuv(0, 0, 0, 0, p + 1, 2, 1, 1, 1, 0, 0), 3, kHuge, 1, false, "Cb");
    expect("luma spans 2^31 - 1 bottom-up", yuv((uint64_t)p + 1, 0, 0, -(p + 1), 0, 2, 1, 1, 1, 0, 0), 3, kHuge, 1, false, "luma");
    expect("pix stride spans 2^31 - 1", yuv(0, 0, 0, 0, 0, 1, 3, (int)((p + 1) / 2) + 1, 1, 0, 0), 3, kHuge, 1, false, "luma");
    expect("planes 2^31 - 2 apart", yuv(0, 10, (uint64_t)p, 0, 0, 1, 1, 1, 1, 0, 0), 3, kHuge, 1, true);
    expect("planes 2^31 - 1 apart", yuv(0, 10, (uint64_t)p + 1, 0, 0, 1, 1, 1, 1, 0, 0), 3, kHuge, 1, false, "Cr");
    expect("luma far above the chroma", yuv((uint64_t)p + 100, 99, 100, 0, 0, 1, 1, 1, 1, 0, 0), 3, kHuge, 1, false, "luma");
    expect("Cb 2^40 away", yuv(0, (uint64_t)1 << 39, 5, 0, 0, 1, 1, 1, 1, 0, 0), 3, kHuge, 1, false, "Cb"); }
  // the fields
  expect("four channels", g, 4, 72, 1, false, "3 channels");
  expect("one channel", g, 1, 72, 1, false, "3 channels");
  { QcnnSrcYuv d = g; d.h = 0; expect("h 0", d, 3, 72, 1, false, "size"); d.h = INT_MIN; expect("h INT_MIN", d, 3, 72, 1, false, "size"); }
  { QcnnSrcYuv d = g; d.w = 1; expect("w 1, relaxed", d, 3, 72, 2, false, "two pixels"); expect("w 1, strict", d, 3, 72, 1, true); }
  { QcnnSrcYuv d = g; d.y_pix_stride = 0; expect("y_pix_stride 0", d, 3, 72, 1, false, "y_pix_stride"); }
  { QcnnSrcYuv d = g; d.c_pix_stride = 0; expect("c_pix_stride 0", d, 3, 72, 1, false, "c_pix_stride"); d.c_pix_stride = INT_MIN;
    expect("c_pix_stride INT_MIN", d, 3, 72, 1, false, "c_pix_stride"); }
  { QcnnSrcYuv d = g; d.sub_x = 2; expect("sub_x 2", d, 3, kHuge, 1, false, "sub_x"); d.sub_x = -1; expect("sub_x -1", d, 3, kHuge, 1, false, "sub_x");
    d.sub_x = 1; d.sub_y = 31; expect("sub_y 31", d, 3, kHuge, 1, false, "sub_y"); d.sub_y = INT_MAX; expect("sub_y INT_MAX", d, 3, kHuge, 1, false, "sub_y"); }
  { QcnnSrcYuv d = g; d.matrix = 3; expect("matrix 3", d, 3, 72, 1, false, "matrix"); d.matrix = -1; expect("matrix -1", d, 3, 72, 1, false, "matrix");
    d.matrix = 2; expect("matrix 2", d, 3, 72, 1, true); }
  { QcnnSrcYuv d = yuv(0, 0, 0, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, INT_MAX, 1, 1); expect("every field INT_MAX", d, 3, SIZE_MAX, 1, false, "luma"); }
  // odd sizes: a 5 x 7 NV12 frame has 3 chroma rows of 4 pairs
  expect("nv12 5x7 fits", yuv(0, 40, 41, 8, 8, 5, 7, 1, 2, 1, 1), 3, 64, 1, true);
  expect("nv12 5x7 one short", yuv(0, 40, 41, 8, 8, 5, 7, 1, 2, 1, 1), 3, 63, 1, false, "Cr");
  expect("yuy2 5x7 fits", yuv(0, 1, 3, 16, 16, 5, 7, 2, 4, 0, 1), 3, 80, 1, true);
  expect("yuy2 5x7 one short", yuv(0, 1, 3, 16, 16, 5, 7, 2, 4, 0, 1), 3, 79, 1, false, "Cr");

  // the constructor
  for (int f = QCNN_YUV_NV12; f <= QCNN_YUV_UYVY; ++f)
    for (int m = QCNN_YUV_JFIF; m <= QCNN_YUV_BT709; ++m) {
      const int sizes[][2] = {{1, 1}, {2, 2}, {5, 7}, {6, 8}, {37, 53}, {1, 9}, {1080, 1920}};
      for (const auto& s : sizes) {
        frame("tight", f, 0, s[0], s[1], 0, m, true);
        frame("pitched", f, 12345, s[0], s[1], 4096, m, true);
        frame("far into a buffer", f, (uint64_t)1 << 40, s[0], s[1], 0, m, true);
      }
      frame("h 0", f, 0, 0, 4, 0, m, false);
      frame("w 0", f, 0, 4, 0, 0, m, false);
      frame("h INT_MIN", f, 0, INT_MIN, 4, 0, m, false);
      frame("pitch 3 for 8 columns", f, 0, 4, 8, 3, m, false);
      frame("pitch -8", f, 0, 4, 8, -8, m, false);
      frame("pitch INT64_MIN", f, 0, 4, 8, INT64_MIN, m, false);
      frame("pitch INT64_MAX", f, 0, 4, 8, INT64_MAX, m, false);
      frame("pitch 2^31", f, 0, 2, 8, (int64_t)1 << 31, m, false);
      frame("2^31 bytes of luma", f, 0, 65536, 32768, 0, m, false);
      frame("INT_MAX x INT_MAX", f, 0, INT_MAX, INT_MAX, 0, m, false);
      frame("INT_MAX rows", f, 0, INT_MAX, 1, 0, m, false);
      frame("offset near 2^64", f, UINT64_MAX - 16, 4, 8, 0, m, false);
      frame("offset 2^64 - 1", f, UINT64_MAX, 1, 1, 0, m, false);
    }
  frame("unknown format 7", 7, 0, 4, 4, 0, 0, false);
  frame("unknown format -1", -1, 0, 4, 4, 0, 0, false);
  frame("unknown format INT_MAX", INT_MAX, 0, 4, 4, 0, 0, false);
  frame("unknown matrix 3", QCNN_YUV_NV12, 0, 4, 4, 0, 3, false);
  frame("unknown matrix INT_MIN", QCNN_YUV_NV12, 0, 4, 4, 0, INT_MIN, false);
  if (qcnn_yuv::yuv_frame(QCNN_YUV_NV12, 0, 4, 4, 0, 0, nullptr) == 0) { printf("FAIL NULL out accepted\n"); ++failures; }
  // an I444 frame of 2^31 - 2 bytes is made, one of 2^31 - 1 or more is not
  frame("i444 at the limit", QCNN_YUV_I444, 0, 3, 1, 238609294, 0, true);               // 9 * 238609294 = 2^31 - 2
  frame("i444 over the limit", QCNN_YUV_I444, 0, 3, 1, 238609295, 0, false);

  if (failures) { printf("%d FAILED\n", failures); return 1; }
  printf("YCbCr layouts under ASan/UBSan: OK\n");
  return 0;
}
