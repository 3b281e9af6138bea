// The layout validator and the BMP header parser of the strided source images (quantized-cnn_amd/csrc/qcnn_src_layout.h) under
// AddressSanitizer and UndefinedBehaviorSanitizer: every accepted and every refused case of include/qcnn_hip.h, the extremes
// of every field among them.  Files are handed over in heap blocks of exactly their size, so that a parser reading past the
// end of a truncated file is caught.  Exit status 0 and the OK line: every case answered as expected and no report.
// Built and run by tests/test_src_layout_sanitize.py.
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../quantized-cnn_amd/csrc/qcnn_src_layout.h"

namespace {
int failures = 0;

QcnnSrcPixels px(uint64_t off, int64_t rs, int h, int w, int ps, int c0, int c1, int c2, int c3 = 0) {
  QcnnSrcPixels d;
  memset(&d, 0, sizeof(d));
  d.offset = off; d.row_stride = rs; d.h = h; d.w = w; d.pix_stride = ps;
  d.ch_offset[0] = c0; d.ch_offset[1] = c1; d.ch_offset[2] = c2; d.ch_offset[3] = c3;
  return d;
}

void expect(const char* what, const QcnnSrcPixels& d, int C, size_t bytes, int minSide, bool good) {
  char msg[256];
  memset(msg, 0, sizeof(msg));
  const int rc = qcnn_src::check_pixels(d, C, bytes, minSide, msg, sizeof(msg));
  if ((rc == 0) != good || (!good && !msg[0])) {
    printf("FAIL %s: rc %d (%s), expected %s\n", what, rc, msg, good ? "accepted" : "refused with a message");
    ++failures;
  }
}

std::vector<uint8_t> header(int32_t w, int32_t h, uint16_t bpp, uint32_t compression, uint32_t dataOff, size_t total) {
  std::vector<uint8_t> f(total < 54 ? 54 : total, 0xAB);
  auto w16 = [&](size_t at, uint32_t v) { f[at] = v & 255; f[at + 1] = (v >> 8) & 255; };
  auto w32 = [&](size_t at, uint32_t v) { w16(at, v & 0xFFFF); w16(at + 2, v >> 16); };
  f[0] = 'B'; f[1] = 'M';
  w32(2, (uint32_t)total); w32(6, 0); w32(10, dataOff); w32(14, 40); w32(18, (uint32_t)w); w32(22, (uint32_t)h); w16(26, 1); w16(28, bpp);
  w32(30, compression); w32(34, 0); w32(38, 2835); w32(42, 2835); w32(46, 0); w32(50, 0);
  f.resize(total);
  return f;
}

// the file in a heap block of exactly its size
void bmp(const char* what, const std::vector<uint8_t>& f, uint64_t at, bool good, uint64_t wantOff = 0, int64_t wantStride = 0) {
  uint8_t* block = f.empty() ? nullptr : (uint8_t*)malloc(f.size());
  if (!f.empty()) memcpy(block, f.data(), f.size());
  QcnnSrcPixels d;
  memset(&d, 0xEE, sizeof(d));
  const int rc = qcnn_src::bmp_pixels(block, f.size(), at, &d);
  bool ok = (rc == 0) == good;
  if (ok && !good) {
    QcnnSrcPixels e;
    memset(&e, 0xEE, sizeof(e));
    ok = memcmp(&d, &e, sizeof(d)) == 0;              // refused: nothing written
  }
  if (ok && good) ok = d.offset == wantOff && d.row_stride == wantStride && d.ch_offset[0] == 0 && d.ch_offset[1] == 1 && d.ch_offset[2] == 2;
  if (!ok) {
    printf("FAIL %s: rc %d, offset %llu, row_stride %lld\n", what, rc, (unsigned long long)d.offset, (long long)d.row_stride);
    ++failures;
  }
  free(block);
}
}  // namespace

int main() {
  const size_t big = (size_t)1 << 40;
  // ---- accepted
  expect("planar 3x5x7", px(0, 7, 5, 7, 1, 0, 35, 70), 3, 105, 1, true);
  expect("exactly fitting", px(10, 21, 5, 7, 3, 0, 1, 2), 3, 10 + 4 * 21 + 6 * 3 + 2 + 1, 1, true);
  expect("bottom-up", px(4 * 24, -24, 5, 7, 3, 0, 1, 2), 3, 5 * 24, 1, true);
  expect("bottom-up, first byte 0", px(4 * 24, -24, 5, 7, 3, 0, 1, 2), 3, 4 * 24 + 21, 1, true);
  expect("row_stride 0", px(3, 0, 1000, 7, 1, 0, 0, 0), 3, 10, 1, true);
  expect("rows overlap", px(0, 1, 4, 7, 1, 0, 0, 0), 3, 10, 1, true);
  expect("one pixel, any stride", px(5, INT64_MAX, 1, 1, 1, 0, 0, 0), 3, 6, 1, true);
  expect("one row, INT64_MIN stride", px(5, INT64_MIN, 1, 2, 1, 0, 0, 0), 3, 7, 1, true);
  expect("span 2^31 - 2", px(0, 0, 1, INT32_MAX, 1, 0, 0, 0), 1, big, 1, true);
  expect("four channels", px(0, 8, 2, 2, 4, 0, 1, 2, 3), 4, 16, 1, true);
  expect("ch_offset[3] ignored for C = 3", px(0, 8, 2, 2, 4, 0, 1, 2, -7), 3, 16, 1, true);
  expect("relaxed 2x2", px(0, 2, 2, 2, 1, 0, 4, 8), 3, 12, 2, true);
  expect("offset near 2^63, huge buffer", px(((uint64_t)1 << 63) - 100, 10, 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, true);
  // ---- refused
  expect("one byte short", px(10, 21, 5, 7, 3, 0, 1, 2), 3, 10 + 4 * 21 + 6 * 3 + 2, 1, false);
  expect("bottom-up, offset one row too small", px(3 * 24, -24, 5, 7, 3, 0, 1, 2), 3, 5 * 24, 1, false);
  expect("bottom-up, one byte below 0", px(4 * 24 - 1, -24, 5, 7, 3, 0, 1, 2), 3, 5 * 24, 1, false);
  expect("five channels", px(0, 7, 5, 7, 1, 0, 35, 70), 5, 1000, 1, false);
  expect("no channel", px(0, 7, 5, 7, 1, 0, 35, 70), 0, 1000, 1, false);
  expect("pix_stride 0", px(0, 7, 5, 7, 0, 0, 35, 70), 3, 1000, 1, false);
  expect("pix_stride negative", px(500, 7, 5, 7, -1, 0, 35, 70), 3, 1000, 1, false);
  expect("pix_stride INT32_MIN", px(500, 7, 5, 7, INT32_MIN, 0, 35, 70), 3, 1000, 1, false);
  expect("ch_offset negative", px(500, 7, 5, 7, 1, 0, -1, 70), 3, 1000, 1, false);
  expect("ch_offset INT32_MIN", px(500, 7, 5, 7, 1, 0, 35, INT32_MIN), 3, 1000, 1, false);
  expect("h = 0", px(0, 7, 0, 7, 1, 0, 35, 70), 3, 1000, 1, false);
  expect("w = 0", px(0, 7, 5, 0, 1, 0, 35, 70), 3, 1000, 1, false);
  expect("h INT32_MIN", px(0, 7, INT32_MIN, 7, 1, 0, 35, 70), 3, 1000, 1, false);
  expect("w INT32_MIN", px(0, 7, 5, INT32_MIN, 1, 0, 35, 70), 3, 1000, 1, false);
  expect("relaxed 1x9", px(0, 9, 1, 9, 1, 0, 9, 18), 3, 1000, 2, false);
  expect("INT64_MIN stride", px(big, INT64_MIN, 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("INT64_MAX stride", px(0, INT64_MAX, 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("INT64_MIN stride, INT32_MAX rows", px(big, INT64_MIN, INT32_MAX, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("INT64_MAX stride, INT32_MAX rows", px(0, INT64_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX), 3, SIZE_MAX, 1, false);
  expect("-INT64_MAX stride", px(big, -INT64_MAX, 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("stride 2^31", px(0, (int64_t)1 << 31, 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("stride -2^31", px(big, -((int64_t)1 << 31), 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("span 2^31 - 1", px(0, 0, 1, INT32_MAX, 1, 1, 0, 0), 1, big, 1, false);
  expect("span 2^31 - 1 by a channel offset", px(0, 0, 1, 1, 1, 0, INT32_MAX, 0), 3, big, 1, false);
  expect("span by both signs", px(big, -((int64_t)1 << 30), 2, 1 << 30, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("w x pix_stride near 2^62", px(0, 0, 1, INT32_MAX, INT32_MAX, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("offset 2^64 - 1", px(UINT64_MAX, 1, 2, 2, 1, 0, 0, 0), 3, SIZE_MAX, 1, false);
  expect("offset 2^64 - 1, one pixel", px(UINT64_MAX, 0, 1, 1, 1, 0, 0, 0), 1, SIZE_MAX, 1, false);
  expect("offset 2^64 - 4, wraps to 1", px(UINT64_MAX - 3, 1, 2, 2, 1, 0, 1, 2), 3, 100, 1, false);
  expect("offset behind the end", px(101, 1, 1, 1, 1, 0, 0, 0), 3, 100, 1, false);
  expect("offset at the end", px(100, 1, 1, 1, 1, 0, 0, 0), 3, 100, 1, false);
  expect("empty buffer", px(0, 1, 1, 1, 1, 0, 0, 0), 3, 0, 1, false);

  // ---- qcnn_src_planar
  {
    QcnnSrcImage img = {77, 5, 7};
    QcnnSrcPixels d, e;
    memset(&d, 0xEE, sizeof(d));
    memset(&e, 0xEE, sizeof(e));
    if (qcnn_src::planar_pixels(&img, 3, &d) || d.offset != 77 || d.row_stride != 7 || d.pix_stride != 1 || d.ch_offset[2] != 70) { puts("FAIL planar"); ++failures; }
    expect("planar_pixels' descriptor", d, 3, 77 + 105, 1, true);
    expect("planar_pixels' descriptor, one byte short", d, 3, 77 + 104, 1, false);
    QcnnSrcImage bad[] = {{0, 0, 7}, {0, 5, 0}, {0, INT32_MIN, 7}, {0, 46341, 46341}, {0, INT32_MAX, INT32_MAX}};
    for (const QcnnSrcImage& b : bad) {
      memset(&d, 0xEE, sizeof(d));
      if (!qcnn_src::planar_pixels(&b, 3, &d) || memcmp(&d, &e, sizeof(d))) { printf("FAIL planar %dx%d\n", b.h, b.w); ++failures; }
    }
    if (!qcnn_src::planar_pixels(&img, 5, &d) || !qcnn_src::planar_pixels(&img, 0, &d) || !qcnn_src::planar_pixels(nullptr, 3, &d) ||
        !qcnn_src::planar_pixels(&img, 3, nullptr)) { puts("FAIL planar arguments"); ++failures; }
  }

  // ---- qcnn_src_bmp: 5 x 4 at 24 bits has 16 bytes a row
  bmp("24-bit bottom-up", header(5, 4, 24, 0, 54, 54 + 64), 1000, true, 1000 + 54 + 3 * 16, -16);
  bmp("24-bit top-down", header(5, -4, 24, 0, 54, 54 + 64), 1000, true, 1000 + 54, 16);
  bmp("32-bit bottom-up", header(5, 4, 32, 0, 54, 54 + 80), 0, true, 54 + 3 * 20, -20);
  bmp("dataOff 70, longer file", header(5, 4, 24, 0, 70, 200), 7, true, 7 + 70 + 48, -16);
  bmp("1 x 1", header(1, 1, 24, 0, 54, 58), 0, true, 54, -4);
  bmp("file_offset + file_bytes = 2^64 - 1", header(1, 1, 24, 0, 54, 58), UINT64_MAX - 58, true, UINT64_MAX - 58 + 54, -4);
  bmp("empty", std::vector<uint8_t>(), 0, false);
  bmp("53 bytes", header(5, 4, 24, 0, 54, 53), 0, false);
  bmp("2 bytes", std::vector<uint8_t>{'B', 'M'}, 0, false);
  { std::vector<uint8_t> f = header(5, 4, 24, 0, 54, 54 + 64); f[1] = 'N'; bmp("signature", f, 0, false); }
  bmp("header alone", header(5, 4, 24, 0, 54, 54), 0, false);
  bmp("one byte short", header(5, 4, 24, 0, 54, 54 + 63), 0, false);
  bmp("one byte short, top-down", header(5, -4, 24, 0, 54, 54 + 63), 0, false);
  bmp("one byte short, 32 bits", header(5, 4, 32, 0, 54, 54 + 79), 0, false);
  bmp("dataOff beyond the file", header(5, 4, 24, 0, 1u << 31, 54 + 64), 0, false);
  bmp("dataOff 2^32 - 1", header(5, 4, 24, 0, UINT32_MAX, 54 + 64), 0, false);
  bmp("dataOff one too far", header(5, 4, 24, 0, 55, 54 + 64), 0, false);
  bmp("8 bits", header(5, 4, 8, 0, 54, 200), 0, false);
  bmp("16 bits", header(5, 4, 16, 0, 54, 200), 0, false);
  bmp("1 bit", header(5, 4, 1, 0, 54, 200), 0, false);
  bmp("RLE8", header(5, 4, 24, 1, 54, 200), 0, false);
  bmp("bitfields", header(5, 4, 32, 3, 54, 200), 0, false);
  bmp("width 0", header(0, 4, 24, 0, 54, 200), 0, false);
  bmp("width negative", header(-5, 4, 24, 0, 54, 200), 0, false);
  bmp("width INT32_MIN", header(INT32_MIN, 4, 24, 0, 54, 200), 0, false);
  bmp("height 0", header(5, 0, 24, 0, 54, 200), 0, false);
  bmp("height INT32_MIN", header(5, INT32_MIN, 24, 0, 54, 200), 0, false);
  bmp("width x 4 bytes near 2^31", header(INT32_MAX / 4 + 1, 1, 32, 0, 54, 200), 0, false);
  bmp("width x 3 bytes near 2^31", header(715827883, 1, 24, 0, 54, 200), 0, false);
  bmp("width INT32_MAX at 32 bits, height INT32_MAX", header(INT32_MAX, INT32_MAX, 32, 0, UINT32_MAX, 200), 0, false);
  bmp("width INT32_MAX, top-down INT32_MAX rows", header(INT32_MAX, -INT32_MAX, 24, 0, 54, 200), 0, false);
  bmp("file_offset + file_bytes wraps", header(1, 1, 24, 0, 54, 58), UINT64_MAX - 57, false);
  bmp("file_offset 2^64 - 1", header(1, 1, 24, 0, 54, 58), UINT64_MAX, false);
  {
    QcnnSrcPixels d;
    std::vector<uint8_t> f = header(1, 1, 24, 0, 54, 58);
    if (!qcnn_src::bmp_pixels(nullptr, 58, 0, &d) || !qcnn_src::bmp_pixels(f.data(), f.size(), 0, nullptr)) { puts("FAIL bmp NULL"); ++failures; }
    // what the parser names lies inside the file: check it with the validator against the file's size
    std::vector<uint8_t> g = header(5, 4, 24, 0, 54, 54 + 64);
    if (qcnn_src::bmp_pixels(g.data(), g.size(), 0, &d)) { puts("FAIL bmp"); ++failures; }
    expect("bmp descriptor fits its file", d, 3, g.size() - 1, 1, true);      // the last byte is padding
    expect("bmp descriptor, file two bytes short", d, 3, g.size() - 2, 1, false);
  }
  if (failures) {
    printf("%d case(s) failed\n", failures);
    return 1;
  }
  puts("source layouts under ASan/UBSan: OK");
  return 0;
}
