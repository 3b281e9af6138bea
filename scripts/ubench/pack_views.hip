// pack_views — the two 8-bit input pack kernels alone, timed with HIP events (LABBOOK.md, "Multi-view inference"):
//   k_pack_u8        1000 images, centre crop                       (what qcnn_forward_u8 launches)
//   k_pack_u8_views  100 images x 10 views = 1000 batch slots       (what qcnn_forward_u8_views launches) with
//                    the ten-crop views, the same ten offsets all plain and all mirrored (mirrored reads walk a row
//                    backwards: this is what separates their cost from the per-slot address arithmetic), and ten times
//                    the centre view
// 256 x 256 sources, a 3 x 227 x 227 input (AlexNet), with a mean image.  Every variant writes the same 1000 x 154 587 floats
// of panels (618 MB); the views variants read a tenth of the source bytes.  Variants alternate inside one process, ROUNDS
// rounds after WARM warm-up launches each; median and minimum per variant.  Links the library's own launchers:
//   hipcc --offload-arch=gfx950 -O3 -o pack_views pack_views.hip -L../../quantized-cnn_amd -lqcnn_hip -Wl,-rpath,'$ORIGIN/../../quantized-cnn_amd'
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../quantized-cnn_amd/csrc/qcnn_kernels.h"

#define CHECK(call)                                                                              \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));    \
      return 1;                                                                                  \
    }                                                                                            \
  } while (0)

int main() {
  const int C = 3, H = 227, W = 227, Hs = 256, Ws = 256, N1 = 1000, N10 = 100, V = 10, WARM = 5, ROUNDS = 30;
  const size_t srcImg = (size_t)C * Hs * Ws, E = (size_t)C * H * W;
  std::vector<uint8_t> px(srcImg * N1);
  std::vector<float> mean(srcImg);
  unsigned s = 12345u;
  for (uint8_t& p : px) { s = s * 1664525u + 1013904223u; p = (uint8_t)(s >> 24); }
  for (float& m : mean) { s = s * 1664525u + 1013904223u; m = 90.0f + (float)(s >> 16) / 65536.0f * 40.0f; }
  uint8_t* dPx = nullptr;
  float *dMean = nullptr, *dDst = nullptr;
  const size_t dstBytes = (size_t)((N1 + QCNN_PANEL - 1) / QCNN_PANEL) * E * QCNN_PANEL * sizeof(float);
  CHECK(hipMalloc(&dPx, px.size()));
  CHECK(hipMalloc(&dMean, mean.size() * sizeof(float)));
  CHECK(hipMalloc(&dDst, dstBytes));
  CHECK(hipMemcpy(dPx, px.data(), px.size(), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dMean, mean.data(), mean.size() * sizeof(float), hipMemcpyHostToDevice));
  const int Y = Hs - H, X = Ws - W;
  const int five[5][2] = {{0, 0}, {0, X}, {Y, 0}, {Y, X}, {Y / 2, X / 2}};
  QkViews ten = {}, plain = {}, flipped = {}, centre = {};
  for (int k = 0; k < V; ++k) {
    ten.v[k] = QkView{five[k % 5][0], five[k % 5][1], k / 5};
    plain.v[k] = QkView{five[k % 5][0], five[k % 5][1], 0};
    flipped.v[k] = QkView{five[k % 5][0], five[k % 5][1], 1};
    centre.v[k] = QkView{Y / 2, X / 2, 0};
  }
  const char* names[5] = {"k_pack_u8 1000 images", "k_pack_u8_views 100 x ten-crop", "k_pack_u8_views 100 x 10 plain",
                          "k_pack_u8_views 100 x 10 mirrored", "k_pack_u8_views 100 x 10 centre"};
  const QkViews* sets[5] = {nullptr, &ten, &plain, &flipped, &centre};
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  auto launch = [&](int k) {
    return k == 0 ? qk_pack_u8(dPx, dMean, dDst, N1, C, H, W, Hs, Ws, st)
                  : qk_pack_u8_views(dPx, dMean, dDst, N10, V, *sets[k], C, H, W, Hs, Ws, st);
  };
  std::vector<float> ms[5];
  for (int r = 0; r < WARM + ROUNDS; ++r)
    for (int k = 0; k < 5; ++k) {
      CHECK(hipEventRecord(e0, st));
      CHECK(launch(k));
      CHECK(hipEventRecord(e1, st));
      CHECK(hipEventSynchronize(e1));
      float t = 0.0f;
      CHECK(hipEventElapsedTime(&t, e0, e1));
      if (r >= WARM) ms[k].push_back(t);
    }
  const double bytes = (double)N1 * E * sizeof(float);
  for (int k = 0; k < 5; ++k) {
    std::sort(ms[k].begin(), ms[k].end());
    const double med = ms[k][ms[k].size() / 2];
    printf("%-36s median %.4f ms  min %.4f ms  max %.4f ms  panels written at %.2f TB/s  x %.3f of k_pack_u8\n", names[k], med, ms[k].front(),
           ms[k].back(), bytes / (med * 1e-3) / 1e12, med / ms[0][ms[0].size() / 2]);
  }
  (void)hipFree(dPx); (void)hipFree(dMean); (void)hipFree(dDst);
  return 0;
}
