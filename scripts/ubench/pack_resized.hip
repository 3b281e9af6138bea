// pack_resized — the fused resize + pack kernel alone against the view pack kernel, timed with HIP events (LABBOOK.md, "Resize on
// the device"), 1000 batch slots of a 3 x 227 x 227 input (AlexNet), full image 256 x 256 with a mean image:
//   k_pack_u8_views    256 x 256 sources: 100 images x ten-crop (the yardstick) and 1000 images x the centre view
//   k_pack_u8_resized  the same two slot splits from 256 x 256 sources (the full size: the identity resize) and from 500 x 375
// Every variant writes the same 1000 x 154 587 floats of panels (618 MB).  Variants alternate inside one process, ROUNDS rounds
// after WARM warm-up launches each; median, minimum and maximum per variant.  Links the library's own launchers:
//   hipcc --offload-arch=gfx950 -O3 -o pack_resized pack_resized.hip -L../../quantized-cnn_amd -lqcnn_hip -Wl,-rpath,'$ORIGIN/../../quantized-cnn_amd'
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
  const int C = 3, H = 227, W = 227, Hf = 256, Wf = 256, N = 1000, WARM = 5, ROUNDS = 30;
  const int srcHW[2][2] = {{256, 256}, {500, 375}};
  const size_t E = (size_t)C * H * W;
  unsigned s = 12345u;
  uint8_t* dPx[2] = {nullptr, nullptr};
  QkSrcImage* dDesc[2] = {nullptr, nullptr};
  for (int k = 0; k < 2; ++k) {
    const size_t img = (size_t)C * srcHW[k][0] * srcHW[k][1];
    std::vector<uint8_t> px(img * N);
    for (uint8_t& p : px) { s = s * 1664525u + 1013904223u; p = (uint8_t)(s >> 24); }
    std::vector<QkSrcImage> desc(N);
    for (int i = 0; i < N; ++i)
      desc[i] = QkSrcImage{(unsigned long long)i * img, srcHW[k][0], srcHW[k][1], (float)(srcHW[k][0] - 1) / (float)(Hf - 1),
                           (float)(srcHW[k][1] - 1) / (float)(Wf - 1)};
    CHECK(hipMalloc(&dPx[k], px.size()));
    CHECK(hipMalloc(&dDesc[k], desc.size() * sizeof(QkSrcImage)));
    CHECK(hipMemcpy(dPx[k], px.data(), px.size(), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dDesc[k], desc.data(), desc.size() * sizeof(QkSrcImage), hipMemcpyHostToDevice));
  }
  std::vector<float> mean((size_t)C * Hf * Wf);
  for (float& m : mean) { s = s * 1664525u + 1013904223u; m = 90.0f + (float)(s >> 16) / 65536.0f * 40.0f; }
  float *dMean = nullptr, *dDst = nullptr;
  CHECK(hipMalloc(&dMean, mean.size() * sizeof(float)));
  CHECK(hipMalloc(&dDst, (size_t)((N + QCNN_PANEL - 1) / QCNN_PANEL) * E * QCNN_PANEL * sizeof(float)));
  CHECK(hipMemcpy(dMean, mean.data(), mean.size() * sizeof(float), hipMemcpyHostToDevice));
  const int Y = Hf - H, X = Wf - W;
  const int five[5][2] = {{0, 0}, {0, X}, {Y, 0}, {Y, X}, {Y / 2, X / 2}};
  QkViews ten = {}, centre = {};
  for (int k = 0; k < 10; ++k) ten.v[k] = QkView{five[k % 5][0], five[k % 5][1], k / 5};
  centre.v[0] = QkView{Y / 2, X / 2, 0};
  const char* names[6] = {"k_pack_u8_views   256x256 100 x ten-crop", "k_pack_u8_views   256x256 1000 x centre",
                          "k_pack_u8_resized 256x256 100 x ten-crop", "k_pack_u8_resized 256x256 1000 x centre",
                          "k_pack_u8_resized 500x375 100 x ten-crop", "k_pack_u8_resized 500x375 1000 x centre"};
  hipStream_t st;
  CHECK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  auto launch = [&](int k) {
    const bool tenCrop = k % 2 == 0;
    const int n = tenCrop ? N / 10 : N, V = tenCrop ? 10 : 1;
    const QkViews& views = tenCrop ? ten : centre;
    if (k < 2) return qk_pack_u8_views(dPx[0], dMean, dDst, n, V, views, C, H, W, Hf, Wf, st);
    const int src = (k - 2) / 2;
    return qk_pack_u8_resized(dPx[src], dDesc[src], dMean, dDst, n, V, views, C, H, W, Hf, Wf, st);
  };
  std::vector<float> ms[6];
  for (int r = 0; r < WARM + ROUNDS; ++r)
    for (int k = 0; k < 6; ++k) {
      CHECK(hipEventRecord(e0, st));
      CHECK(launch(k));
      CHECK(hipEventRecord(e1, st));
      CHECK(hipEventSynchronize(e1));
      float t = 0.0f;
      CHECK(hipEventElapsedTime(&t, e0, e1));
      if (r >= WARM) ms[k].push_back(t);
    }
  const double bytes = (double)N * E * sizeof(float);
  for (int k = 0; k < 6; ++k) {
    std::sort(ms[k].begin(), ms[k].end());
    const double med = ms[k][ms[k].size() / 2];
    printf("%-42s median %.4f ms  min %.4f ms  max %.4f ms  panels written at %.2f TB/s  x %.3f of the first\n", names[k], med,
           ms[k].front(), ms[k].back(), bytes / (med * 1e-3) / 1e12, med / ms[0][ms[0].size() / 2]);
  }
  for (int k = 0; k < 2; ++k) { (void)hipFree(dPx[k]); (void)hipFree(dDesc[k]); }
  (void)hipFree(dMean); (void)hipFree(dDst);
  return 0;
}
