// The YCbCr instantiations of the two resizing pack kernels (qcnn_forward_u8_resized_views_yuv / _relaxed_views_yuv):
// k_pack_u8_resized<MEAN, QkSrcYuv> and k_pack_u8_relaxed<MEAN, QkRelaxedYuv> from the templates of qcnn_pack.h, in a code object of
// their own (see there).
#include "qcnn_kernels.h"

#include <limits.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));

namespace {
constexpr int PANEL = QCNN_PANEL;              // images per panel
#include "qcnn_pack.h"
}  // namespace

hipError_t qk_pack_u8_resized_yuv(const uint8_t* in, const QkSrcYuv* desc, const float* mean, float* dst, int n, int V,
                                  const QkViews& views, int C, int H, int W, int Hf, int Wf, hipStream_t st) {
  if (C != 3) return hipErrorInvalidValue;          // a YCbCr frame makes B, G, R
  return launch_pack_resized(in, desc, mean, dst, n, V, views, C, H, W, Hf, Wf, st);
}

hipError_t qk_pack_u8_relaxed_yuv(const uint8_t* in, const QkRelaxedYuv* desc, const float* mean, float* dst, int n, int V,
                                  const QkAnchorViews& views, int C, int H, int W, hipStream_t st) {
  if (C != 3) return hipErrorInvalidValue;
  return launch_pack_relaxed(in, desc, mean, dst, n, V, views, C, H, W, st);
}
