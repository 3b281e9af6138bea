// qcnn_engine_u8.hip — the 8-bit multi-view front end: BmpImgIO::Load's work (resize, crops, mirrors, mean) on the device in
// front of the layers, for one batch whose source bytes lie on the device (qcnn_forward_u8_*_views*) and for batches streamed
// from host memory through host_batch_schedule (qcnn_forward_u8_*_host_batches*); the descriptor constructors.
#include <limits.h>
#include <string.h>

#include <algorithm>

#include "qcnn_engine.h"
#include "qcnn_src_layout.h"
#include "qcnn_src_yuv.h"

using namespace qcnn_engine;

static_assert(QK_MAX_VIEWS == QCNN_MAX_VIEWS, "the kernel-argument view table holds QCNN_MAX_VIEWS entries");

namespace {

// The multi-view calls behind their pack kernel: the layers on the n * n_views slots in fm[0], the un-averaged rows, the mean
// (into the map views_scratch has sized), top-5.
int views_tail(QcnnCtx* c, int n, int n_views, float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  if (forward_tail(c, n * n_views, prob_views_dev, nullptr)) return 1;     // the un-averaged rows: one per slot
  if (!prob_dev && !top5_dev) return 0;
  hipError_t e = qk_mean_views(c->lastFm[c->L], c->viewMean, n, n_views, (int)fm_elems(c, c->L), c->stream);
  if (e != hipSuccess) return fail(c, "view mean launch failed: %s", hipGetErrorString(e));
  return map_outputs(c, c->viewMean, n, prob_dev, top5_dev);
}

// What every multi-view call asks first.  `missing`: what the NULL message names, nullptr when every pointer is there.
int views_open(QcnnCtx* c, const char* fn, const char* missing, int n, int n_views) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (missing) return fail(c, "%s: %s == NULL", fn, missing);
  if (n <= 0) return fail(c, "batch %d: no image", n);
  if (n_views < 1 || n_views > QCNN_MAX_VIEWS) return fail(c, "%d views outside [1, %d]", n_views, QCNN_MAX_VIEWS);
  if ((long long)n * n_views > c->maxBatch)
    return fail(c, "%d images x %d views = %lld batch slots, the model is committed for %d", n, n_views, (long long)n * n_views, c->maxBatch);
  return 0;
}
// The views of a call as the kernels take them, each crop inside the h x w image (`which`: source or full) it is cut from.
int crop_views(QcnnCtx* c, const QcnnView* views_host, int n_views, int h, int w, const char* which, QkViews* views) {
  for (int v = 0; v < n_views; ++v) {
    const QcnnView& q = views_host[v];
    if (q.oy < 0 || q.ox < 0 || q.oy > h - c->inH || q.ox > w - c->inW)
      return fail(c, "view %d: the %dx%d crop at (%d, %d) leaves the %dx%d %s image", v, c->inH, c->inW, q.oy, q.ox, h, w, which);
    views->v[v] = QkView{q.oy, q.ox, q.flip ? 1 : 0};
  }
  return 0;
}
// The full image of a resize: what its scale, the network input and 32-bit offsets need.
int full_image_ok(QcnnCtx* c, int full_h, int full_w) {
  if (full_h < 2 || full_w < 2)
    return fail(c, "full image %dx%d: the resize scale divides by full - 1, both sizes must be at least 2", full_h, full_w);
  if (full_h < c->inH || full_w < c->inW)
    return fail(c, "the full image %dx%d is smaller than the network input %dx%d", full_h, full_w, c->inH, c->inW);
  if ((long long)c->inC * full_h * full_w > INT_MAX) return fail(c, "the full image %dx%dx%d has 2 GiB or more", c->inC, full_h, full_w);
  return 0;
}

// What the planar, the strided and the YCbCr calls differ in, by the type of the caller's descriptor: its check (src_ok), the
// image part of the staged descriptor, the staged descriptor itself and the pack launch.
// Source image i: its sides (at least 1 for a Strict, 2 for a Relaxed resize), its size, its place in the source buffer.
int src_ok(QcnnCtx* c, int i, const QcnnSrcImage& s, size_t src_bytes, int minSide) {
  if (s.h < minSide || s.w < minSide)
    return minSide < 2 ? fail(c, "image %d: size %dx%d", i, s.h, s.w)
                       : fail(c, "image %d: size %dx%d, the one scale of a relaxed resize needs two pixels a side", i, s.h, s.w);
  const unsigned long long rows = (unsigned long long)c->inC * (unsigned long long)s.h, bytes = rows * (unsigned long long)s.w;   // rows <= INT_MAX is asked first: then bytes < 2^62
  if (rows > (unsigned long long)INT_MAX || bytes > (unsigned long long)INT_MAX)
    return fail(c, "image %d: %dx%dx%d has 2 GiB or more (offsets inside an image are 32-bit)", i, c->inC, s.h, s.w);
  if (s.offset > src_bytes || bytes > src_bytes - s.offset)
    return fail(c, "image %d: %llu bytes at offset %llu leave the source buffer of %zu bytes", i, bytes, (unsigned long long)s.offset, src_bytes);
  return 0;
}
// Source image i of a strided call: the same for a layout given by strides (qcnn_src_layout.h holds the rules).
int src_ok(QcnnCtx* c, int i, const QcnnSrcPixels& s, size_t src_bytes, int minSide) {
  char why[256];
  if (qcnn_src::check_pixels(s, c->inC, src_bytes, minSide, why, sizeof(why))) return fail(c, "image %d: %s", i, why);
  return 0;
}
// Source image i of a YCbCr call: the same for three sample planes (qcnn_src_yuv.h holds the rules).
int src_ok(QcnnCtx* c, int i, const QcnnSrcYuv& s, size_t src_bytes, int minSide) {
  char why[320];
  if (qcnn_yuv::check_yuv(s, c->inC, src_bytes, minSide, why, sizeof(why))) return fail(c, "image %d: %s", i, why);
  return 0;
}
// The layout of a checked descriptor as the kernels take it: row_stride's low 32 bits (they differ from it only where h == 1).
QkLayout layout_of(const QcnnSrcPixels& s) {
  return QkLayout{(int)(uint32_t)(uint64_t)s.row_stride, s.pix_stride, s.ch_offset[0], s.ch_offset[1], s.ch_offset[2], s.ch_offset[3]};
}
// The layout of a checked descriptor as the kernels take it: the row strides' low 32 bits (they differ from them only where a
// plane has one row), the chroma bases as deltas from the luma base (32-bit: every sample lies within 2^31 - 1 bytes of every
// other) and the matrix's six integers.
QkYuvLayout yuv_layout_of(const QcnnSrcYuv& s) {
  const int32_t* m = qcnn_yuv::matrix_ints(s.matrix);
  return QkYuvLayout{(int)(uint32_t)(uint64_t)s.y_row_stride, s.y_pix_stride, (int)(uint32_t)(uint64_t)s.c_row_stride, s.c_pix_stride,
                     (int)(uint32_t)(s.cb_offset - s.y_offset), (int)(uint32_t)(s.cr_offset - s.y_offset), s.sub_y, s.sub_x,
                     m[0], m[1], m[2], m[3], m[4], m[5]};
}
uint64_t base_of(const QcnnSrcImage& s) { return s.offset; }       // the byte a staged descriptor's offsets are relative to
uint64_t base_of(const QcnnSrcPixels& s) { return s.offset; }
uint64_t base_of(const QcnnSrcYuv& s) { return s.y_offset; }        // luma sample (0, 0)
QkSrcImage staged(const QcnnSrcImage&, const QkSrcImage& img) { return img; }
QkSrcYuv staged(const QcnnSrcYuv& s, const QkSrcImage& img) { return QkSrcYuv{img, yuv_layout_of(s)}; }
QkRelaxedYuv staged(const QcnnSrcYuv& s, const QkRelaxedImage& img) { return QkRelaxedYuv{img, yuv_layout_of(s)}; }
QkSrcPixels staged(const QcnnSrcPixels& s, const QkSrcImage& img) { return QkSrcPixels{img, layout_of(s)}; }
QkRelaxedImage staged(const QcnnSrcImage&, const QkRelaxedImage& img) { return img; }
QkRelaxedPixels staged(const QcnnSrcPixels& s, const QkRelaxedImage& img) { return QkRelaxedPixels{img, layout_of(s)}; }
hipError_t pack_resized(const uint8_t* in, const QkSrcImage* d, const float* mean, float* dst, int n, int V, const QkViews& views, int C,
                        int H, int W, int Hf, int Wf, hipStream_t st) { return qk_pack_u8_resized(in, d, mean, dst, n, V, views, C, H, W, Hf, Wf, st); }
hipError_t pack_resized(const uint8_t* in, const QkSrcPixels* d, const float* mean, float* dst, int n, int V, const QkViews& views, int C,
                        int H, int W, int Hf, int Wf, hipStream_t st) { return qk_pack_u8_resized_strided(in, d, mean, dst, n, V, views, C, H, W, Hf, Wf, st); }
hipError_t pack_resized(const uint8_t* in, const QkSrcYuv* d, const float* mean, float* dst, int n, int V, const QkViews& views, int C,
                        int H, int W, int Hf, int Wf, hipStream_t st) { return qk_pack_u8_resized_yuv(in, d, mean, dst, n, V, views, C, H, W, Hf, Wf, st); }
hipError_t pack_relaxed(const uint8_t* in, const QkRelaxedYuv* d, const float* mean, float* dst, int n, int V, const QkAnchorViews& views,
                        int C, int H, int W, hipStream_t st) { return qk_pack_u8_relaxed_yuv(in, d, mean, dst, n, V, views, C, H, W, st); }
hipError_t pack_relaxed(const uint8_t* in, const QkRelaxedImage* d, const float* mean, float* dst, int n, int V, const QkAnchorViews& views,
                        int C, int H, int W, hipStream_t st) { return qk_pack_u8_relaxed(in, d, mean, dst, n, V, views, C, H, W, st); }
hipError_t pack_relaxed(const uint8_t* in, const QkRelaxedPixels* d, const float* mean, float* dst, int n, int V, const QkAnchorViews& views,
                        int C, int H, int W, hipStream_t st) { return qk_pack_u8_relaxed_strided(in, d, mean, dst, n, V, views, C, H, W, st); }

// Stage n descriptors D — fill(i) makes image i's — and launch the pack kernel that reads them.  Called when every argument
// is good: nothing is taken or rewritten for a call that is refused.  The set is marked in flight only once nothing of the
// host's can fail any more, and its event is recorded behind its one reader.  afterPack (or nullptr): a second event recorded
// there — the pack kernel is the last reader of the source buffer too (the streamed calls hand the buffer back on it).
template <class D, class Fill, class Pack>
int stage_and_pack(QcnnCtx* c, int n, bool wantMean, hipEvent_t afterPack, Fill fill, Pack launch) {
  QcnnCtx::SrcStage* g = stage_take(c, (size_t)n, sizeof(D));
  if (!g) return 1;
  D* pin = static_cast<D*>(g->pin);
  for (int i = 0; i < n; ++i) pin[i] = fill(i);
  if (views_scratch(c, n, wantMean)) return 1;
  g->used = true;                                     // from here on the set may be in flight
  HIP_TRY(c, hipMemcpyAsync(g->dev, g->pin, (size_t)n * sizeof(D), hipMemcpyHostToDevice, c->stream));
  hipError_t e = launch(static_cast<const D*>(g->dev));
  if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
  HIP_TRY(c, hipEventRecord(g->ev, c->stream));
  if (afterPack) HIP_TRY(c, hipEventRecord(afterPack, c->stream));
  return 0;
}

// What the two pre-processing modes differ in: the caller's view type and its check, the check of one source image, the staged
// descriptor and the pack launch.  Everything around them — one batch on the device (u8_views) and batches streamed from host
// memory (u8_host_batches) — is written once.
// ENUM_ReszType::Strict: every image to full_h x full_w, the views cut from that (qcnn_forward_u8_resized_views*)
struct StrictMode {
  using View = QcnnView;
  using Views = QkViews;
  static int views(QcnnCtx* c, const View* views_host, int n_views, int full_h, int full_w, Views* out) {
    return crop_views(c, views_host, n_views, full_h, full_w, "full", out);
  }
  template <class Src>
  static int image(QcnnCtx* c, int i, const Src& s, size_t src_bytes, int, int, const Views&, int) { return src_ok(c, i, s, src_bytes, 1); }
  template <class Src> static auto desc(const Src& s, int full_h, int full_w) {   // the scales: one IEEE division each, as ReszImg computes them
    return staged(s, QkSrcImage{base_of(s), s.h, s.w, (float)(s.h - 1) / (float)(full_h - 1), (float)(s.w - 1) / (float)(full_w - 1)});
  }
  template <class D>
  static hipError_t pack(QcnnCtx* c, const uint8_t* src_dev, const D* d, const float* mean_dev, int n, int n_views, const Views& views,
                         int full_h, int full_w) {
    return pack_resized(src_dev, d, mean_dev, c->fmBuf[0], n, n_views, views, c->inC, c->inH, c->inW, full_h, full_w, c->stream);
  }
};
// ENUM_ReszType::Relaxed + ENUM_MeanType::Crop: one scale per image, its own full size, anchored views (qcnn_forward_u8_relaxed_views*)
struct RelaxedMode {
  using View = QcnnAnchorView;
  using Views = QkAnchorViews;
  static int views(QcnnCtx* c, const View* views_host, int n_views, int, int, Views* out) {
    for (int v = 0; v < n_views; ++v) {
      const QcnnAnchorView& q = views_host[v];
      if (q.ay < 0 || q.ay > 2 || q.ax < 0 || q.ax > 2) return fail(c, "view %d: anchors (%d, %d) outside 0..2", v, q.ay, q.ax);
      out->v[v] = QkAnchorView{q.ay, q.ax, q.dy, q.dx, q.flip ? 1 : 0};
    }
    return 0;
  }
  template <class Src>
  static int image(QcnnCtx* c, int i, const Src& s, size_t src_bytes, int full_h, int full_w, const Views& views, int n_views) {
    if (src_ok(c, i, s, src_bytes, 2)) return 1;
    int hf = 0, wf = 0;
    if (qcnn_relaxed_full_size(s.h, s.w, full_h, full_w, &hf, &wf, nullptr))
      return fail(c, "image %d: %dx%d resized towards %dx%d has a side of 2^24 pixels or more", i, s.h, s.w, full_h, full_w);
    for (int v = 0; v < n_views; ++v) {               // in 64 bits: d is the caller's
      const QkAnchorView& q = views.v[v];
      const long long oy = (((long long)(hf - c->inH) * q.ay) >> 1) + q.dy, ox = (((long long)(wf - c->inW) * q.ax) >> 1) + q.dx;
      if (hf < c->inH || wf < c->inW || oy < 0 || ox < 0 || oy > hf - c->inH || ox > wf - c->inW)
        return fail(c, "image %d, view %d: the %dx%d crop at (%lld, %lld) leaves the image's %dx%d full size (source %dx%d)", i, v, c->inH,
                    c->inW, oy, ox, hf, wf, s.h, s.w);
    }
    return 0;
  }
  template <class Src> static auto desc(const Src& s, int full_h, int full_w) {   // each image's scale and full size
    QkRelaxedImage d = {base_of(s), s.h, s.w, 0.0f, 0, 0, 0};
    (void)qcnn_relaxed_full_size(s.h, s.w, full_h, full_w, &d.hf, &d.wf, &d.s);     // succeeded in image()
    return staged(s, d);
  }
  template <class D>
  static hipError_t pack(QcnnCtx* c, const uint8_t* src_dev, const D* d, const float* mean_crop_dev, int n, int n_views, const Views& views,
                         int, int) {
    return pack_relaxed(src_dev, d, mean_crop_dev, c->fmBuf[0], n, n_views, views, c->inC, c->inH, c->inW, c->stream);
  }
};

// One checked batch whose source bytes lie on the device: descriptors staged, pack kernel, layers, averaging, outputs — all
// on the context's stream.  afterPack: stage_and_pack's.
template <class Mode, class Src>
int u8_enqueue(QcnnCtx* c, const uint8_t* src_dev, const Src* imgs_host, int n, int full_h, int full_w, const float* mean_dev,
               const typename Mode::Views& views, int n_views, float* prob_dev, uint16_t* top5_dev, float* prob_views_dev,
               hipEvent_t afterPack) {
  using D = decltype(Mode::desc(imgs_host[0], full_h, full_w));
  if (stage_and_pack<D>(
          c, n, prob_dev || top5_dev, afterPack, [&](int i) { return Mode::desc(imgs_host[i], full_h, full_w); },
          [&](const D* d) { return Mode::pack(c, src_dev, d, mean_dev, n, n_views, views, full_h, full_w); }))
    return 1;
  return views_tail(c, n, n_views, prob_dev, top5_dev, prob_views_dev);
}

// qcnn_forward_u8_resized_views[_strided] (Mode = StrictMode) and qcnn_forward_u8_relaxed_views[_strided] (RelaxedMode), for
// planar (Src = QcnnSrcImage), strided (QcnnSrcPixels) and YCbCr (QcnnSrcYuv) descriptors.
template <class Mode, class Src>
int u8_views(QcnnCtx* c, const char* fn, const uint8_t* src_dev, size_t src_bytes, const Src* imgs_host, int n, int full_h, int full_w,
             const float* mean_dev, const typename Mode::View* views_host, int n_views, float* prob_dev, uint16_t* top5_dev,
             float* prob_views_dev) {
  if (views_open(c, fn, src_dev && imgs_host && views_host ? nullptr : "source buffer, images or views", n, n_views) ||
      full_image_ok(c, full_h, full_w))
    return 1;
  typename Mode::Views views = {};
  if (Mode::views(c, views_host, n_views, full_h, full_w, &views)) return 1;
  for (int i = 0; i < n; ++i)
    if (Mode::image(c, i, imgs_host[i], src_bytes, full_h, full_w, views, n_views)) return 1;
  return u8_enqueue<Mode>(c, src_dev, imgs_host, n, full_h, full_w, mean_dev, views, n_views, prob_dev, top5_dev, prob_views_dev, nullptr);
}

// qcnn_forward_u8_resized_host_batches (Mode = StrictMode) and qcnn_forward_u8_relaxed_host_batches (RelaxedMode): the image
// loop of src/CaffeEva.cc:151-211 with BmpImgIO::Load's work on the device and CalcPredAccu's counting (:263-295) behind every
// labelled batch.  The schedule is qcnn_forward_host_batches', with 8-bit source bytes in place of float crops.
template <class Mode, class Batch>                    // Batch: QcnnU8Batch (strided descriptors) or QcnnU8YuvBatch (YCbCr)
int u8_host_batches(QcnnCtx* c, const char* fn, const Batch* batches, int nb, int full_h, int full_w, const float* mean_dev,
                    const typename Mode::View* views_host, int n_views, unsigned long long* hits5) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (nb <= 0 || !batches) return fail(c, "%s: no batches", fn);
  if (!views_host) return fail(c, "%s: views == NULL", fn);
  if (n_views < 1 || n_views > QCNN_MAX_VIEWS) return fail(c, "%d views outside [1, %d]", n_views, QCNN_MAX_VIEWS);
  if (full_image_ok(c, full_h, full_w)) return 1;
  typename Mode::Views views = {};
  if (Mode::views(c, views_host, n_views, full_h, full_w, &views)) return 1;
  // every batch is checked before anything is enqueued or any buffer rewritten
  const unsigned classes = (unsigned)fm_elems(c, c->L);
  size_t maxBytes = 0;
  int maxN = 0;
  bool anyMean = false;
  for (int b = 0; b < nb; ++b) {
    const Batch& q = batches[b];
    if (!q.src_host || !q.imgs) return fail(c, "batch %d: src_host or imgs == NULL", b);
    if (q.n <= 0) return fail(c, "batch %d: no image (n = %d)", b, q.n);
    if ((long long)q.n * n_views > c->maxBatch)
      return fail(c, "batch %d: %d images x %d views = %lld batch slots, the model is committed for %d", b, q.n, n_views,
                  (long long)q.n * n_views, c->maxBatch);
    for (int i = 0; i < q.n; ++i)
      if (Mode::image(c, i, q.imgs[i], q.src_bytes, full_h, full_w, views, n_views)) {
        c->err = "batch " + std::to_string(b) + ": " + c->err;
        return 1;
      }
    for (int i = 0; q.labels && i < q.n; ++i)
      if (q.labels[i] >= classes) return fail(c, "batch %d: image %d: label %u is no class of the model's %u", b, i, (unsigned)q.labels[i], classes);
    maxBytes = std::max(maxBytes, q.src_bytes);
    maxN = std::max(maxN, q.n);
    anyMean = anyMean || q.prob_host || q.top5_host || (q.labels && hits5);
  }
  // everything that grows grows here: source buffers, the view-mean map, both descriptor staging sets (two takes: each set once)
  if (ensure_u8_stream(c, maxBytes) || views_scratch(c, maxN, anyMean)) return 1;
  using D = decltype(Mode::desc(batches[0].imgs[0], full_h, full_w));
  for (int k = 0; k < 2; ++k)
    if (!stage_take(c, (size_t)maxN, sizeof(D))) return 1;
  // the job of the schedule: source bytes and labels go up into the pair the pack kernel of batch b - 2 has handed back; the
  // compute step is u8_enqueue + the hit count of a labelled batch
  QcnnCtx::U8Stream& s = c->u8s;
  bool counted[2] = {false, false};
  auto count = [&](int b) { return batches[b].labels && hits5; };
  HostBatchJob job;
  job.images = [&](int b) { return batches[b].n; };
  job.prologue = [&]() -> int { HIP_TRY(c, hipMemsetAsync(s.hits, 0, 5 * sizeof(unsigned long long), c->stream)); return 0; };
  job.stage = [&](int b, int k) -> int {                // labels pass through the pinned pair: the copy of batch b - 2 out of it has passed
    if (count(b) && b >= 2) HIP_TRY(c, hipEventSynchronize(c->evCopied[k]));
    if (count(b)) memcpy(s.pinLabels[k], batches[b].labels, (size_t)batches[b].n * sizeof(uint16_t));
    return 0;
  };
  job.upload = [&](int b, int k) -> int {
    const Batch& q = batches[b];
    HIP_TRY(c, hipMemcpyAsync(s.src[k], q.src_host, q.src_bytes, hipMemcpyHostToDevice, c->copyStream));
    if (!count(b)) return 0;                            // labels[k]'s last reader is the hit count of batch b - 2, far behind its pack kernel
    if (counted[k]) HIP_TRY(c, hipStreamWaitEvent(c->copyStream, s.evCounted[k], 0));
    HIP_TRY(c, hipMemcpyAsync(s.labels[k], s.pinLabels[k], (size_t)q.n * sizeof(uint16_t), hipMemcpyHostToDevice, c->copyStream));
    return 0;
  };
  job.compute = [&](int b, int k, hipEvent_t freed) -> int {      // the pack kernel is the last reader of src[k]: handed back behind it
    const Batch& q = batches[b];
    if (u8_enqueue<Mode>(c, s.src[k], q.imgs, q.n, full_h, full_w, mean_dev, views, n_views, q.prob_host ? s.prob : nullptr,
                         q.top5_host || count(b) ? s.top5 : nullptr, q.prob_views_host ? s.rows : nullptr, freed))
      return 1;
    if (!count(b)) return 0;                            // on the view-averaged rows: n labels, not n * n_views
    const hipError_t e = qk_top5_hits(s.top5, s.labels[k], q.n, s.hits, c->stream);
    if (e != hipSuccess) return fail(c, "hit count launch failed: %s", hipGetErrorString(e));
    HIP_TRY(c, hipEventRecord(s.evCounted[k], c->stream));
    counted[k] = true;
    return 0;
  };
  job.results = [&](int b, int k) {
    const Batch& q = batches[b];
    const size_t rowBytes = (size_t)q.n * classes * sizeof(float);
    return std::vector<HostResult>{{s.prob, c->pinProb[k], q.prob_host, rowBytes}, {s.top5, c->pinTop5[k], q.top5_host, (size_t)q.n * 5 * sizeof(uint16_t)},
                                   {s.rows, s.pinRows[k], q.prob_views_host, rowBytes * n_views}};
  };
  job.epilogue = [&]() -> int {                         // the five counters: read back once
    if (hits5) HIP_TRY(c, hipMemcpyAsync(s.pinHits, s.hits, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  if (host_batch_schedule(c, nb, job)) return 1;
  if (hits5) memcpy(hits5, c->u8s.pinHits, 5 * sizeof(unsigned long long));
  return 0;
}

}  // namespace

extern "C" {

int qcnn_views_ten_crop(int src_h, int src_w, int in_h, int in_w, QcnnView* views10) {
  if (!views10 || in_h <= 0 || in_w <= 0 || src_h < in_h || src_w < in_w) return 1;
  const int Y = src_h - in_h, X = src_w - in_w;
  const int five[5][2] = {{0, 0}, {0, X}, {Y, 0}, {Y, X}, {Y / 2, X / 2}};
  for (int k = 0; k < 10; ++k) views10[k] = QcnnView{five[k % 5][0], five[k % 5][1], k / 5};
  return 0;
}

int qcnn_forward_u8_views(QcnnCtx* c, const uint8_t* in_u8_dev, int src_h, int src_w, const float* mean_dev, int n,
                          const QcnnView* views_host, int n_views, float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  if (views_open(c, "qcnn_forward_u8_views", in_u8_dev && views_host ? nullptr : "images or views", n, n_views)) return 1;
  QkViews views = {};
  if (crop_views(c, views_host, n_views, src_h, src_w, "source", &views)) return 1;
  if (views_scratch(c, n, prob_dev || top5_dev)) return 1;
  hipError_t e = qk_pack_u8_views(in_u8_dev, mean_dev, c->fmBuf[0], n, n_views, views, c->inC, c->inH, c->inW, src_h, src_w, c->stream);
  if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
  return views_tail(c, n, n_views, prob_dev, top5_dev, prob_views_dev);
}

int qcnn_forward_u8_resized_views(QcnnCtx* c, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcImage* imgs_host, int n,
                                  int full_h, int full_w, const float* mean_dev, const QcnnView* views_host, int n_views,
                                  float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  return u8_views<StrictMode>(c, "qcnn_forward_u8_resized_views", src_dev, src_bytes, imgs_host, n, full_h, full_w, mean_dev, views_host, n_views,
                       prob_dev, top5_dev, prob_views_dev);
}

int qcnn_forward_u8_resized_views_strided(QcnnCtx* c, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcPixels* imgs_host, int n,
                                          int full_h, int full_w, const float* mean_dev, const QcnnView* views_host, int n_views,
                                          float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  return u8_views<StrictMode>(c, "qcnn_forward_u8_resized_views_strided", src_dev, src_bytes, imgs_host, n, full_h, full_w, mean_dev, views_host,
                       n_views, prob_dev, top5_dev, prob_views_dev);
}

int qcnn_forward_u8_resized_views_yuv(QcnnCtx* c, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcYuv* imgs_host, int n, int full_h,
                                      int full_w, const float* mean_dev, const QcnnView* views_host, int n_views, float* prob_dev,
                                      uint16_t* top5_dev, float* prob_views_dev) {
  return u8_views<StrictMode>(c, "qcnn_forward_u8_resized_views_yuv", src_dev, src_bytes, imgs_host, n, full_h, full_w, mean_dev, views_host,
                       n_views, prob_dev, top5_dev, prob_views_dev);
}

int qcnn_src_yuv_frame(int format, uint64_t frame_offset, int h, int w, int64_t pitch, int matrix, QcnnSrcYuv* out) {
  return qcnn_yuv::yuv_frame(format, frame_offset, h, w, pitch, matrix, out);
}

int qcnn_src_planar(const QcnnSrcImage* img, int C, QcnnSrcPixels* out) { return qcnn_src::planar_pixels(img, C, out); }

int qcnn_src_bmp(const uint8_t* file_host, size_t file_bytes, uint64_t file_offset, QcnnSrcPixels* out) {
  return qcnn_src::bmp_pixels(file_host, file_bytes, file_offset, out);
}

int qcnn_views_ten_crop_anchored(QcnnAnchorView* views10) {
  if (!views10) return 1;
  const int five[5][2] = {{0, 0}, {0, 2}, {2, 0}, {2, 2}, {1, 1}};
  for (int k = 0; k < 10; ++k) views10[k] = QcnnAnchorView{five[k % 5][0], five[k % 5][1], 0, 0, k / 5};
  return 0;
}

// BmpImgIO::ReszImg's Relaxed branch (src/BmpImgIO.cc:124-131) operation for operation: every division is a float division
// (int / float converts the int), kEpsilon is a double, the cast truncates.  The quotient is compared in double before the cast.
int qcnn_relaxed_full_size(int h, int w, int full_h, int full_w, int* hf, int* wf, float* scale) {
  if (h < 2 || w < 2 || full_h < 2 || full_w < 2 || !hf || !wf) return 1;
  const float sh = (float)(h - 1) / (float)(full_h - 1), sw = (float)(w - 1) / (float)(full_w - 1);
  const float s = sh < sw ? sh : sw;                  // lines 127-128 leave both scales equal to the smaller
  const double qh = (double)((float)(h - 1) / s) + 0.0000001, qw = (double)((float)(w - 1) / s) + 0.0000001;
  if (!(qh < 16777215.0) || !(qw < 16777215.0)) return 1;     // a full size of 2^24 or more: (float)Y would not be exact
  *hf = (int)qh + 1;
  *wf = (int)qw + 1;
  if (scale) *scale = s;
  return 0;
}

int qcnn_forward_u8_relaxed_views(QcnnCtx* c, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcImage* imgs_host, int n,
                                  int full_h, int full_w, const float* mean_crop_dev, const QcnnAnchorView* views_host, int n_views,
                                  float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  return u8_views<RelaxedMode>(c, "qcnn_forward_u8_relaxed_views", src_dev, src_bytes, imgs_host, n, full_h, full_w, mean_crop_dev, views_host,
                       n_views, prob_dev, top5_dev, prob_views_dev);
}

int qcnn_forward_u8_relaxed_views_strided(QcnnCtx* c, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcPixels* imgs_host, int n,
                                          int full_h, int full_w, const float* mean_crop_dev, const QcnnAnchorView* views_host,
                                          int n_views, float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  return u8_views<RelaxedMode>(c, "qcnn_forward_u8_relaxed_views_strided", src_dev, src_bytes, imgs_host, n, full_h, full_w, mean_crop_dev,
                       views_host, n_views, prob_dev, top5_dev, prob_views_dev);
}

int qcnn_forward_u8_relaxed_views_yuv(QcnnCtx* c, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcYuv* imgs_host, int n, int full_h,
                                      int full_w, const float* mean_crop_dev, const QcnnAnchorView* views_host, int n_views,
                                      float* prob_dev, uint16_t* top5_dev, float* prob_views_dev) {
  return u8_views<RelaxedMode>(c, "qcnn_forward_u8_relaxed_views_yuv", src_dev, src_bytes, imgs_host, n, full_h, full_w, mean_crop_dev,
                       views_host, n_views, prob_dev, top5_dev, prob_views_dev);
}

int qcnn_forward_u8_resized_host_batches(QcnnCtx* c, const QcnnU8Batch* batches, int nb, int full_h, int full_w, const float* mean_dev,
                                         const QcnnView* views_host, int n_views, unsigned long long* hits5) {
  return u8_host_batches<StrictMode>(c, "qcnn_forward_u8_resized_host_batches", batches, nb, full_h, full_w, mean_dev, views_host, n_views,
                                     hits5);
}

int qcnn_forward_u8_relaxed_host_batches(QcnnCtx* c, const QcnnU8Batch* batches, int nb, int full_h, int full_w,
                                         const float* mean_crop_dev, const QcnnAnchorView* views_host, int n_views,
                                         unsigned long long* hits5) {
  return u8_host_batches<RelaxedMode>(c, "qcnn_forward_u8_relaxed_host_batches", batches, nb, full_h, full_w, mean_crop_dev, views_host,
                                      n_views, hits5);
}

int qcnn_forward_u8_resized_host_batches_yuv(QcnnCtx* c, const QcnnU8YuvBatch* batches, int nb, int full_h, int full_w, const float* mean_dev,
                                             const QcnnView* views_host, int n_views, unsigned long long* hits5) {
  return u8_host_batches<StrictMode>(c, "qcnn_forward_u8_resized_host_batches_yuv", batches, nb, full_h, full_w, mean_dev, views_host,
                                     n_views, hits5);
}

int qcnn_forward_u8_relaxed_host_batches_yuv(QcnnCtx* c, const QcnnU8YuvBatch* batches, int nb, int full_h, int full_w,
                                             const float* mean_crop_dev, const QcnnAnchorView* views_host, int n_views,
                                             unsigned long long* hits5) {
  return u8_host_batches<RelaxedMode>(c, "qcnn_forward_u8_relaxed_host_batches_yuv", batches, nb, full_h, full_w, mean_crop_dev, views_host,
                                      n_views, hits5);
}

}  // extern "C"
