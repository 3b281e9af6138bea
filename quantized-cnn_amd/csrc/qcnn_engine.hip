// qcnn_engine.hip — the C-ABI of include/qcnn_hip.h: context, options, model planning, and the owner of the context's buffers.
//
// Mirrors the control flow of the reference's CaffeEva (src/CaffeEva.cc): LoadCaffePara ->
// PrepFeatMap/PrepFeatBuf/PrepCtrdBuf/PrepAsmtBuf (:109-149) becomes qcnn_model_begin / commit /
// set_layer_params (qcnn_engine_params.hip); ExecForwardPass's layer loop (:184-205, :232-254) becomes run_layers()
// (qcnn_engine_run.hip).  Everything the loop touches lives in HBM for the whole batch; the host only enqueues kernels.
// qcnn_engine.h names the other files of the engine and what crosses between them.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "qcnn_engine.h"

using namespace qcnn_engine;

namespace {

std::string g_createError = "";

int plan_arena(QcnnCtx* c) {
  size_t off = 0;
  for (int l = 0; l < c->L; ++l) {
    const QcnnLayerDesc& d = c->layers[l];
    if (d.type != QCNN_CONV && d.type != QCNN_FCNT) continue;
    LayerShape& s = c->shapes[l];
    const int Ct = c->dims[l + 1].c;
    s.hasDmap = (d.type == QCNN_FCNT && l == c->firstFc && c->dims[l].h * c->dims[l].w > 1);
    if (s.dense) {                     // precise path: bias + weights [grp][taps][Cin/grp][Ct/grp]
      s.offBias = off; off = align_up(off + sizeof(float) * Ct, 256);
      const size_t taps = (d.type == QCNN_CONV) ? (size_t)d.knlSiz * d.knlSiz : 1;
      const size_t cin = (d.type == QCNN_CONV) ? (size_t)c->dims[l].c / d.grpCnt : fm_elems(c, l);
      s.denseFloats = taps * cin * Ct;
      s.offDense = off; off = align_up(off + sizeof(float) * s.denseFloats, 256);
      if (s.hasDmap) { s.offDmap = off; off = align_up(off + sizeof(int) * fm_elems(c, l), 256); }
      continue;
    }
    if (s.K <= 0) return fail(c, "layer %d: neither a quantisation shape (qcnn_model_set_layer_shape) nor dense weights (qcnn_model_set_layer_dense) declared", l);
    const size_t bookBytes = sizeof(float) * (size_t)s.M * s.Cs * s.K;
    s.offBias = off; off = align_up(off + sizeof(float) * Ct, 256);
    s.offCtrd = off; off = align_up(off + bookBytes, 256);
    // assignment table: one-byte row slots in the order the gather waves consume them (QkSlots, qcnn_kernels.h)
    const TableGeom g = table_geom(c, l);
    const size_t taps = (d.type == QCNN_CONV) ? (size_t)d.knlSiz * d.knlSiz : 1;
    s.asmtBytes = taps * s.M * g.sl.rowStride;
    s.offAsmt = off; off = align_up(off + s.asmtBytes + QCNN_ROWS_PAD, 256);
    for (bool& has : s.hasBook) has = false;
    for (int k = 0; k < T_COUNT; ++k) {
      s.tab[k] = Span{0, table_desc(k).bytes(g, 0)};
      if (s.tab[k].bytes) { s.tab[k].off = off; off = align_up(off + s.tab[k].bytes + QCNN_ROWS_PAD, 256); }
      const int b = table_desc(k).book;
      if (b == BOOK_NONE) continue;
      s.hasBook[b] = s.hasBook[b] || s.tab[k].bytes;
      if (s.hasBook[b] && (k + 1 == T_COUNT || table_desc(k + 1).book != b)) { s.offBook[b] = off; off = align_up(off + bookBytes, 256); }
    }
    s.cbnBits = s.tab[T_CBN].bytes ? cbn_bits(s.K) : 0;
    s.decKp = 0;
    if (d.type == QCNN_CONV && qk_conv_dec_shape(c->dims[l].c, d.grpCnt, s.M, Ct, d.knlSiz, &s.decKp, &s.decS)) {
      s.offDec = off; off = align_up(off + sizeof(float) * (size_t)d.knlSiz * s.decKp * s.decS, 256);
      s.decNV = 0;
      s.decBK = 0;
      if (l == 0 && qk_conv_dec_nchw_shape(c->dims[l].c, d.grpCnt, s.M, Ct, d.knlSiz, d.padSiz, &s.decNV)) {
        s.offDecN = off; off = align_up(off + sizeof(float) * (size_t)s.decNV * Ct, 256);
        if (qk_conv_dec_nchw_split_shape(c->dims[l].c, d.grpCnt, s.M, Ct, d.knlSiz, d.padSiz, &s.decBK)) {   // derived like the copy above
          s.offDecB = off; off = align_up(off + 6 * (size_t)s.decBK * Ct, 256);                           // w1, w2, w3: 2 bytes each
          s.offDecH = off; off = align_up(off + qk_conv_dec_nchw_f16_bytes(s.decBK, Ct), 256);            // Sw, then w1, w2 as fp16
        }
      }
    } else if (d.type == QCNN_FCNT && !s.hasDmap && qk_fc_dec_shape((int)fm_elems(c, l), s.M, s.Cs, Ct, &s.decS)) {
      s.decKp = -1;                   // FC layer with one-dim sub-spaces: [D][decS] decoded code words
      s.offDec = off; off = align_up(off + sizeof(float) * fm_elems(c, l) * s.decS, 256);
    } else {
      s.decKp = 0;
    }
    if (s.hasDmap) { s.offDmap = off; off = align_up(off + sizeof(int) * fm_elems(c, l), 256); }
  }
  c->arenaBytes = off + kSlack;
  return 0;
}

void free_model(QcnnCtx* c) {
  calib_free(c);                                         // a calibration belongs to the model it was begun on
  for (LayerShape& s : c->shapes) drop_f16_programs(s);
  for (float* p : c->fmBuf) if (p) (void)hipFree(p);
  c->fmBuf.clear();
  if (c->ownArena && c->arena) (void)hipFree(c->arena);
  c->arena = nullptr; c->ownArena = false;
  if (c->stageIn) (void)hipFree(c->stageIn);
  if (c->stageOut) (void)hipFree(c->stageOut);
  if (c->stageTop5) (void)hipFree(c->stageTop5);
  if (c->stageIn1) (void)hipFree(c->stageIn1);
  c->stageIn1 = nullptr;
  for (int k = 0; k < 2; ++k) {
    if (c->pinProb[k]) (void)hipHostFree(c->pinProb[k]);
    if (c->pinTop5[k]) (void)hipHostFree(c->pinTop5[k]);
    c->pinProb[k] = nullptr; c->pinTop5[k] = nullptr; c->freedValid[k] = false;
  }
  {
    QcnnCtx::U8Stream& s = c->u8s;                      // what is sized by the model; the source buffers stay
    for (int k = 0; k < 2; ++k) {
      if (s.labels[k]) (void)hipFree(s.labels[k]);
      if (s.pinLabels[k]) (void)hipHostFree(s.pinLabels[k]);
      if (s.pinRows[k]) (void)hipHostFree(s.pinRows[k]);
      s.labels[k] = nullptr; s.pinLabels[k] = nullptr; s.pinRows[k] = nullptr;
    }
    if (s.prob) (void)hipFree(s.prob);
    if (s.rows) (void)hipFree(s.rows);
    if (s.top5) (void)hipFree(s.top5);
    if (s.hits) (void)hipFree(s.hits);
    if (s.pinHits) (void)hipHostFree(s.pinHits);
    s.prob = s.rows = nullptr; s.top5 = nullptr; s.hits = s.pinHits = nullptr;
  }
  if (c->fcPartial) (void)hipFree(c->fcPartial);
  if (c->convPartial) (void)hipFree(c->convPartial);
  c->convPartial = nullptr; c->noConvPartial = false;
  if (c->fcFlat) (void)hipFree(c->fcFlat);
  c->fcFlat = nullptr;
  if (c->decGuard) (void)hipFree(c->decGuard);
  c->decGuard = nullptr; c->decGuardBytes = 0;
  for (int k = 0; k < kMaxStreams; ++k) { c->decEpoch[k] = 0; c->decGuardItems[k] = 0; }
  c->stageIn = c->stageOut = nullptr; c->stageTop5 = nullptr; c->stageElems = 0;
  c->fcPartial = nullptr; c->fcPartialElems = 0;
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  c->ev.clear();
  c->profCount = 0; c->profPending.clear(); c->profForwards = 0;
  c->lastFm.clear(); c->lastN = 0;       // nothing of the old model can be read back any more
  c->committed = false;
}

// events and pinned result buffers of the pipelined host paths: all the 8-bit stream takes of them
int ensure_pipeline_results(QcnnCtx* c) {
  const size_t classes = fm_elems(c, c->L);
  for (int k = 0; k < 2; ++k) {
    if (!c->evCopied[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->evCopied[k], hipEventDisableTiming));
    if (!c->evFreed[k]) { HIP_TRY(c, hipEventCreateWithFlags(&c->evFreed[k], hipEventDisableTiming)); c->freedValid[k] = false; }
    if (!c->evDone[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->evDone[k], hipEventDisableTiming));
    if (!c->pinProb[k]) HIP_TRY(c, hipHostMalloc(&c->pinProb[k], (size_t)c->maxBatch * classes * sizeof(float), hipHostMallocPortable));
    if (!c->pinTop5[k]) HIP_TRY(c, hipHostMalloc(&c->pinTop5[k], (size_t)c->maxBatch * 5 * sizeof(uint16_t), hipHostMallocPortable));
  }
  return 0;
}

// two 64-bit sums over the arena's 32-bit words: the plain sum and a position-weighted one (a permutation of blocks changes it)
__global__ __launch_bounds__(256) void k_arena_checksum(const uint32_t* __restrict__ w, size_t n, unsigned long long* __restrict__ out) {
  unsigned long long a = 0, b = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const unsigned long long v = w[i];
    a += v;
    b += v * (unsigned long long)(i % 65521u + 1u);
  }
  for (int off = 32; off > 0; off >>= 1) { a += __shfl_down(a, off); b += __shfl_down(b, off); }
  if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], a); atomicAdd(&out[1], b); }
}

}  // namespace

namespace qcnn_engine {

int fail(QcnnCtx* c, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_createError = buf;
  return 1;
}

// Linear staging for host <-> device conversions.  Sized for what the forward paths need — a batch of network inputs, a batch of
// class scores — and grown on demand when a larger feature map is dumped (qcnn_get_layer_output / qcnn_run_layer): sizing it for the
// LARGEST map of the model up front made the first qcnn_forward_host of VGG-16 at batch 1000 allocate 2 x 12.8 GB (0.75 s; AlexNet: 2 x
// 1.2 GB)
int ensure_stage(QcnnCtx* c, size_t elems) {
  const size_t base = std::max(fm_elems(c, 0), fm_elems(c, c->L)) * (size_t)c->maxBatch;
  const size_t need = std::max(base, elems);
  if (c->stageIn && c->stageElems >= need) return 0;
  if (c->stageIn) {                                     // grow: nothing may still be using the old buffers
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->copyStream) HIP_TRY(c, hipStreamSynchronize(c->copyStream));
    (void)hipFree(c->stageIn); (void)hipFree(c->stageOut);
    c->stageIn = c->stageOut = nullptr;
  }
  c->stageElems = 0;                                    // committed only when BOTH buffers exist (a half-grown pair must never be used)
  float *in = nullptr, *out = nullptr;
  HIP_TRY(c, hipMalloc(&in, need * sizeof(float) + kSlack));
  if (hipMalloc(&out, need * sizeof(float) + kSlack) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(in);
    return fail(c, "staging buffers: 2 x %zu bytes do not fit the device", need * sizeof(float) + kSlack);
  }
  c->stageIn = in; c->stageOut = out; c->stageElems = need;
  if (!c->stageTop5) HIP_TRY(c, hipMalloc(&c->stageTop5, (size_t)c->maxBatch * 5 * sizeof(uint16_t)));
  return 0;
}

// buffers, stream and events of the pipelined float path: the results' and the two device input buffers
int ensure_pipeline(QcnnCtx* c) {
  if (ensure_stage(c)) return 1;
  if (c->stageIn1) return 0;
  if (ensure_pipeline_results(c)) return 1;
  HIP_TRY(c, hipMalloc(&c->stageIn1, fm_elems(c, 0) * c->maxBatch * sizeof(float) + kSlack));
  return 0;
}

// what the 8-bit stream owns beside them: two source buffers of at least srcBytes, and per model the label pairs, the device
// results, the pinned pair of the un-averaged rows and the hit counters.  The source buffers grow here, in front of the
// first upload of a call, never inside a stream
int ensure_u8_stream(QcnnCtx* c, size_t srcBytes) {
  if (ensure_pipeline_results(c)) return 1;
  QcnnCtx::U8Stream& s = c->u8s;
  const size_t rowBytes = (size_t)c->maxBatch * fm_elems(c, c->L) * sizeof(float), labelBytes = (size_t)c->maxBatch * sizeof(uint16_t);
  for (int k = 0; k < 2; ++k) {
    if (!s.evCounted[k]) HIP_TRY(c, hipEventCreateWithFlags(&s.evCounted[k], hipEventDisableTiming));
    if (!s.labels[k]) HIP_TRY(c, hipMalloc(&s.labels[k], labelBytes));
    if (!s.pinLabels[k]) HIP_TRY(c, hipHostMalloc(&s.pinLabels[k], labelBytes, hipHostMallocPortable));
    if (!s.pinRows[k]) HIP_TRY(c, hipHostMalloc(&s.pinRows[k], rowBytes, hipHostMallocPortable));
  }
  if (!s.prob) HIP_TRY(c, hipMalloc(&s.prob, rowBytes));
  if (!s.rows) HIP_TRY(c, hipMalloc(&s.rows, rowBytes));
  if (!s.top5) HIP_TRY(c, hipMalloc(&s.top5, (size_t)c->maxBatch * 5 * sizeof(uint16_t)));
  if (!s.hits) HIP_TRY(c, hipMalloc(&s.hits, 5 * sizeof(unsigned long long)));
  if (!s.pinHits) HIP_TRY(c, hipHostMalloc(&s.pinHits, 5 * sizeof(unsigned long long), hipHostMallocPortable));
  if (s.srcCap >= srcBytes && s.src[0] && s.src[1]) return 0;
  HIP_TRY(c, hipStreamSynchronize(c->stream));          // grow: an earlier pack kernel may still be reading the old buffers
  HIP_TRY(c, hipStreamSynchronize(c->copyStream));
  for (int k = 0; k < 2; ++k) {
    if (s.src[k]) (void)hipFree(s.src[k]);
    s.src[k] = nullptr;
  }
  s.srcCap = 0;                                          // committed only when BOTH buffers exist
  for (int k = 0; k < 2; ++k) HIP_TRY(c, hipMalloc(&s.src[k], srcBytes + kSlack));
  s.srcCap = srcBytes;
  return 0;
}

// Partial-sum scratch of split conv tiles: kConvPartialFloats shared by the sub-batches, allocated by the first split launch
// of this context; when the device has no memory left for it (large maps at a large batch) the tiles run whole, which needs
// none — never a failed forward
float* ensure_conv_partial(QcnnCtx* c) {
  if (!c->convPartial && !c->noConvPartial && hipMalloc(&c->convPartial, kConvPartialFloats * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    c->convPartial = nullptr; c->noConvPartial = true;
  }
  return c->convPartial;
}

// Guard regions of the first layer's fp16 form (k_conv_dec_nchw_f16): kMaxStreams regions, each for the items of maxPanels panels,
// zeroed once (word 0 of a region must not hold a launch's number before that launch ran)
uint32_t* ensure_dec_guard(QcnnCtx* c, int sub) {
  if (!c->decGuard) {
    const size_t bytes = align_up(qk_conv_dec_nchw_f16_guard_bytes(c->dims[1].h, c->dims[1].w, c->dims[1].c, c->maxPanels), 256);
    hipError_t e = hipMalloc(&c->decGuard, bytes * kMaxStreams);
    if (e == hipSuccess) e = hipMemset(c->decGuard, 0, bytes * kMaxStreams);
    if (e != hipSuccess) {
      if (c->decGuard) (void)hipFree(c->decGuard);
      c->decGuard = nullptr;
      fail(c, "range-guard regions of the first layer: %s", hipGetErrorString(e));
      return nullptr;
    }
    c->decGuardBytes = bytes;
  }
  return reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(c->decGuard) + c->decGuardBytes * sub);
}

// The multi-view calls, BEFORE their pack kernel is launched: the map of the averaged rows is large enough for n images.
int views_scratch(QcnnCtx* c, int n, bool wantMean) {
  const size_t need = (size_t)((n + QCNN_PANEL - 1) / QCNN_PANEL) * fm_elems(c, c->L) * QCNN_PANEL;
  if (wantMean && c->viewMeanElems < need) {          // grow: an earlier call on the stream may still be reading the old map
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->viewMean) (void)hipFree(c->viewMean);
    c->viewMean = nullptr; c->viewMeanElems = 0;
    HIP_TRY(c, hipMalloc(&c->viewMean, need * sizeof(float) + kSlack));
    c->viewMeanElems = need;
  }
  return 0;
}

// qcnn_map_diff, BEFORE its launches: the scratch of its two passes holds `doubles` doubles.
int diff_scratch(QcnnCtx* c, size_t doubles) {
  if (c->diffScratchDoubles < doubles) {             // grow: the call is blocking, nothing on the stream still reads the old one
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->diffScratch) (void)hipFree(c->diffScratch);
    c->diffScratch = nullptr; c->diffScratchDoubles = 0;
    HIP_TRY(c, hipMalloc(&c->diffScratch, doubles * sizeof(double)));
    c->diffScratchDoubles = doubles;
  }
  return 0;
}

// The next of the two descriptor staging sets, large enough for n descriptors of `each` bytes (at least 64 of them); nullptr
// after fail().  The last reader of the set taken — the pack kernel of the call before the previous one — must have passed
// before its buffers are rewritten or freed.
QcnnCtx::SrcStage* stage_take(QcnnCtx* c, size_t n, size_t each) {
  QcnnCtx::SrcStage& g = c->srcStage[c->srcStageNext];
  c->srcStageNext ^= 1;
  hipError_t e = hipSuccess;
  if (!g.ev) e = hipEventCreateWithFlags(&g.ev, hipEventDisableTiming);
  if (e == hipSuccess && g.used) e = hipEventSynchronize(g.ev);
  if (e == hipSuccess && g.cap < n * each) {
    if (g.pin) (void)hipHostFree(g.pin);
    if (g.dev) (void)hipFree(g.dev);
    g.pin = nullptr; g.dev = nullptr; g.cap = 0; g.used = false;
    const size_t cap = std::max<size_t>(n, 64) * each;
    e = hipHostMalloc(&g.pin, cap, hipHostMallocPortable);
    if (e == hipSuccess) e = hipMalloc(&g.dev, cap);
    if (e == hipSuccess) g.cap = cap;
  }
  if (e != hipSuccess) { fail(c, "descriptor staging: %s", hipGetErrorString(e)); return nullptr; }
  return &g;
}

}  // namespace qcnn_engine

extern "C" {

int qcnn_abi_version(void) { return QCNN_ABI_VERSION; }

int qcnn_device_count(int* count) {
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) { *count = 0; return fail(nullptr, "hipGetDeviceCount -> %s", hipGetErrorString(e)); }
  return 0;
}

const char* qcnn_last_error(const QcnnCtx* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

int qcnn_ctx_create(int device_id, void* stream, QcnnCtx** out) {
  if (!out) return fail(nullptr, "qcnn_ctx_create: out == NULL");
  *out = nullptr;
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0)
    return fail(nullptr, "no HIP device available (%s); this library has no CPU path",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device_id < 0 || device_id >= cnt) return fail(nullptr, "device %d out of range [0, %d)", device_id, cnt);
  e = hipSetDevice(device_id);
  if (e != hipSuccess) return fail(nullptr, "hipSetDevice(%d) -> %s", device_id, hipGetErrorString(e));
  hipDeviceProp_t prop;
  e = hipGetDeviceProperties(&prop, device_id);
  if (e != hipSuccess) return fail(nullptr, "hipGetDeviceProperties -> %s", hipGetErrorString(e));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(nullptr, "device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
  QcnnCtx* c = new QcnnCtx;
  c->device = device_id;
  if (stream) {
    c->stream = static_cast<hipStream_t>(stream);
  } else {
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(nullptr, "hipStreamCreate -> %s", hipGetErrorString(e)); }
    c->ownStream = true;
  }
  // The copy stream is created HERE, second: the runtime spreads a process's streams over a handful of hardware queues
  // (four by default) in creation order, and a copy stream that shares its queue with the compute stream serialises
  // "upload batch b + 1" in front of "layers of batch b" (measured: 25 ms instead of 15 ms per 1000-image batch).  The
  // auxiliary compute streams are created on demand (run_layers), so the default two-stream set-up uses three queues.
  e = hipStreamCreateWithFlags(&c->copyStream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    if (c->ownStream) (void)hipStreamDestroy(c->stream);
    delete c;
    return fail(nullptr, "hipStreamCreate (copy stream) -> %s", hipGetErrorString(e));
  }
  *out = c;
  return 0;
}

int qcnn_ctx_destroy(QcnnCtx* c) {
  if (!c) return 0;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  free_model(c);
  if (c->viewMean) (void)hipFree(c->viewMean);
  if (c->diffScratch) (void)hipFree(c->diffScratch);
  for (int k = 0; k < 2; ++k) {
    if (c->u8s.src[k]) (void)hipFree(c->u8s.src[k]);
    if (c->u8s.evCounted[k]) (void)hipEventDestroy(c->u8s.evCounted[k]);
  }
  for (QcnnCtx::SrcStage& g : c->srcStage) {
    if (g.pin) (void)hipHostFree(g.pin);
    if (g.dev) (void)hipFree(g.dev);
    if (g.ev) (void)hipEventDestroy(g.ev);
  }
  for (int k = 0; k < kMaxStreams - 1; ++k) {
    if (c->aux[k]) (void)hipStreamDestroy(c->aux[k]);
    if (c->evJoin[k]) (void)hipEventDestroy(c->evJoin[k]);
  }
  if (c->evFork) (void)hipEventDestroy(c->evFork);
  for (int k = 0; k < 2; ++k) {
    if (c->evCopied[k]) (void)hipEventDestroy(c->evCopied[k]);
    if (c->evFreed[k]) (void)hipEventDestroy(c->evFreed[k]);
    if (c->evDone[k]) (void)hipEventDestroy(c->evDone[k]);
  }
  for (hipEvent_t e : c->evChunk) (void)hipEventDestroy(e);
  if (c->copyStream) (void)hipStreamDestroy(c->copyStream);
  if (c->ownStream) (void)hipStreamDestroy(c->stream);
  delete c;
  return 0;
}

int qcnn_set_option(QcnnCtx* c, int option, int value) {
  switch (option) {
    case QCNN_OPT_LUT_MODE: if (value < 0 || value > 3) return fail(c, "LUT mode must be 0 (exact), 1 (f32 MFMA), 2 (fp16 table storage) or 3 (fp16 tables and fp16 sums)"); c->lutMode = value; return 0;   // (part of the plan key)
    case QCNN_OPT_KEEP_ALL: c->keepAll = value ? 1 : 0; return 0;
    case QCNN_OPT_PROFILE: c->profile = value ? 1 : 0; return 0;
    case QCNN_OPT_SMALL_BATCH: c->smallBatch = value ? 1 : 0; return 0;
    case QCNN_OPT_SPLIT: c->split = value ? 1 : 0; return 0;
    case QCNN_OPT_DECODE: c->decode = value ? 1 : 0; return 0;
    case QCNN_OPT_HALF8: if (value < 0 || value > 3) return fail(c, "QCNN_OPT_HALF8 must be 0 (off), 1 (planner), 2 (forced tile form) or 3 (forced sliding form)"); c->half8 = value; return 0;
    case QCNN_OPT_SYM8: if (value < 0 || value > 3) return fail(c, "QCNN_OPT_SYM8 must be 0 (off), 1 (planner), 2 (forced tile form) or 3 (forced sliding form)"); c->sym8 = value; return 0;
    case QCNN_OPT_PACKED_FC: c->packedFc = value ? 1 : 0; return 0;
    case QCNN_OPT_DIRECT_DEC: c->directDec = value ? 1 : 0; return 0;
    case QCNN_OPT_DEC_BF16SPLIT: if (value < 0 || value > 2) return fail(c, "QCNN_OPT_DEC_BF16SPLIT must be 0 (f32), 1 (three bf16 pieces) or 2 (two fp16 pieces)"); c->decSplit = value; return 0;
    case QCNN_OPT_SYM: if (value < 0 || value > 2) return fail(c, "QCNN_OPT_SYM must be 0 (off), 1 (planner) or 2 (forced)"); c->sym = value; return 0;
    case QCNN_OPT_SLIDE: if (value < 0 || value > 2) return fail(c, "QCNN_OPT_SLIDE must be 0 (off), 1 (planner) or 2 (forced)"); c->slide = value; return 0;
    case QCNN_OPT_HOST_CHUNK:
      if (value < 0) return fail(c, "host chunk must be >= 0 panels");
      c->hostChunk = value; return 0;
    case QCNN_OPT_STREAMS:
      if (value < 1 || value > kMaxStreams) return fail(c, "streams must be in [1, %d]", kMaxStreams);
      c->nStreams = value; return 0;
    default: return fail(c, "unknown option %d", option);
  }
}

int qcnn_ctx_device(const QcnnCtx* c) { return c->device; }
void* qcnn_ctx_stream(const QcnnCtx* c) { return c->stream; }

int qcnn_sync(QcnnCtx* c) {
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int qcnn_model_begin(QcnnCtx* c, int layer_cnt, const QcnnLayerDesc* layers, int in_c, int in_h, int in_w) {
  HIP_TRY(c, hipSetDevice(c->device));
  free_model(c);
  if (layer_cnt <= 0 || !layers) return fail(c, "qcnn_model_begin: empty layer table");
  c->L = layer_cnt; c->inC = in_c; c->inH = in_h; c->inW = in_w;
  c->layers.assign(layers, layers + layer_cnt);
  c->shapes.assign(layer_cnt, LayerShape());
  c->dims.assign(layer_cnt + 1, FmDims{0, 0, 0});
  c->firstFc = -1;
  int h = in_h, w = in_w, ch = in_c;
  c->dims[0] = FmDims{h, w, ch};
  for (int l = 0; l < layer_cnt; ++l) {           // feature-map size rule, src/CaffeEva.cc:357-391
    const QcnnLayerDesc& d = layers[l];
    switch (d.type) {
      case QCNN_CONV:
        if (d.grpCnt <= 0 || d.stride <= 0 || d.knlSiz <= 0 || ch % d.grpCnt || d.knlCnt % d.grpCnt)
          return fail(c, "layer %d: bad conv geometry", l);
        // a window must touch the map: with padSiz >= knlSiz a tile of the table kernels can lie wholly in the padding (no source
        // row or column at all), which their stage arithmetic does not provide for
        if (d.padSiz < 0 || d.padSiz >= d.knlSiz)
          return fail(c, "layer %d: conv padding %d is outside [0, kernel size %d): every window must hold a pixel of the map", l,
                      d.padSiz, d.knlSiz);
        h = conv_out(h, d.knlSiz, d.stride, d.padSiz); w = conv_out(w, d.knlSiz, d.stride, d.padSiz); ch = d.knlCnt;
        break;
      case QCNN_POOL:
        if (d.stride <= 0 || d.knlSiz <= 0) return fail(c, "layer %d: bad pool geometry", l);
        h = pool_out(h, d.knlSiz, d.stride, d.padSiz); w = pool_out(w, d.knlSiz, d.stride, d.padSiz);
        break;
      case QCNN_FCNT:
        if (c->firstFc < 0) c->firstFc = l;
        h = 1; w = 1; ch = d.nodCnt;
        break;
      case QCNN_RELU: case QCNN_LORN: case QCNN_DRPT: case QCNN_SMAX: break;
      default: return fail(c, "layer %d: invalid layer type %d", l, d.type);
    }
    if (h <= 0 || w <= 0 || ch <= 0) return fail(c, "layer %d: empty feature map", l);
    c->dims[l + 1] = FmDims{h, w, ch};
  }
  return 0;
}

int qcnn_model_set_layer_shape(QcnnCtx* c, int layer, int M, int K, int Cs) {
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const QcnnLayerDesc& d = c->layers[layer];
  if (d.type != QCNN_CONV && d.type != QCNN_FCNT) return fail(c, "layer %d carries no parameters", layer);
  if (M <= 0 || K <= 0 || K > QCNN_MAX_K_FILE || Cs <= 0 || Cs > QCNN_MAX_CS)
    return fail(c, "layer %d: unsupported quantisation shape M=%d K=%d Cs=%d (K <= %d, Cs <= %d)", layer, M, K, Cs,
                QCNN_MAX_K_FILE, QCNN_MAX_CS);
  const int D = (d.type == QCNN_CONV) ? c->dims[layer].c / d.grpCnt : (int)fm_elems(c, layer);
  if ((size_t)M * Cs < (size_t)D) return fail(c, "layer %d: M*Cs = %d does not cover %d input dims", layer, M * Cs, D);
  if ((M - 1) * Cs >= D) return fail(c, "layer %d: sub-space %d starts beyond the %d input dims", layer, M - 1, D);
  const int Ct = c->dims[layer + 1].c;
  const int Ctg = (d.type == QCNN_CONV) ? Ct / d.grpCnt : Ct;
  if (Ctg % 2) return fail(c, "layer %d: %d output channels per group is not even", layer, Ctg);
  LayerShape& s = c->shapes[layer];
  s.Mfile = M; s.Kfile = K; s.Cs = Cs;
  // more code words than a 128-row LDS stage holds (the reference's uint8 assignments allow 256, include/FileIO.h:128-166): P pseudo
  // sub-spaces of <= 127 code words + one all-zero row each over the SAME dims; an assignment names its code word in one of them and
  // the zero row in the others — the same sums (x + 0 = x), through the exact-builder kernels (ConvParams::pd)
  s.P = K > QCNN_MAX_K ? (K + 126) / 127 : 1;
  s.M = M * s.P;
  s.K = s.P > 1 ? QCNN_MAX_K : K;
  return 0;
}

int qcnn_model_set_layer_dense(QcnnCtx* c, int layer) {
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const QcnnLayerDesc& d = c->layers[layer];
  if (d.type != QCNN_CONV && d.type != QCNN_FCNT) return fail(c, "layer %d carries no parameters", layer);
  if (c->committed) return fail(c, "qcnn_model_set_layer_dense must precede qcnn_model_commit");
  c->shapes[layer] = LayerShape();
  c->shapes[layer].dense = true;
  return 0;
}

int qcnn_model_arena_bytes(QcnnCtx* c, size_t* bytes) {
  if (plan_arena(c)) return 1;
  *bytes = c->arenaBytes;
  return 0;
}

int qcnn_model_arena_ptr(QcnnCtx* c, void** dev_ptr, size_t* bytes) {
  if (!c->committed) return fail(c, "model not committed");
  if (dev_ptr) *dev_ptr = c->arena;
  if (bytes) *bytes = c->arenaBytes;
  return 0;
}

/* Checksum of the packed parameter arena as it lies on the device (after uploads / a broadcast): sum2[0] = sum of its 32-bit
 * words, sum2[1] = position-weighted sum.  Ranks whose arenas hold the same bytes report the same pair — what a sharded run
 * compares before it trusts a broadcast.  Blocking. */
int qcnn_model_arena_checksum(QcnnCtx* c, unsigned long long* sum2) {
  if (!c->committed) return fail(c, "model not committed");
  if (!sum2) return fail(c, "qcnn_model_arena_checksum: sum2 == NULL");
  HIP_TRY(c, hipSetDevice(c->device));
  unsigned long long* d = nullptr;
  HIP_TRY(c, hipMalloc(&d, 2 * sizeof(unsigned long long)));
  hipError_t e = hipMemsetAsync(d, 0, 2 * sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_arena_checksum, dim3(1024), dim3(256), 0, c->stream, reinterpret_cast<const uint32_t*>(c->arena),
                       c->arenaBytes / 4, d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(sum2, d, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) return fail(c, "arena checksum -> %s", hipGetErrorString(e));
  return 0;
}

int qcnn_model_commit(QcnnCtx* c, int max_batch, void* dev_arena) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->committed) return fail(c, "model already committed");
  if (max_batch <= 0) return fail(c, "max_batch must be positive");
  if (plan_arena(c)) return 1;
  c->maxBatch = max_batch;
  c->maxPanels = (max_batch + QCNN_PANEL - 1) / QCNN_PANEL;
  if (dev_arena) {
    c->arena = static_cast<char*>(dev_arena);
    c->ownArena = false;
  } else {
    HIP_TRY(c, hipMalloc(&c->arena, c->arenaBytes));   // arenaBytes already includes the slack
    c->ownArena = true;
    HIP_TRY(c, hipMemsetAsync(c->arena, 0, c->arenaBytes, c->stream));
  }
  c->fmBuf.assign(c->L + 1, nullptr);
  for (int l = 0; l <= c->L; ++l) {
    if (l > 0 && c->layers[l - 1].type == QCNN_DRPT) continue;   // always an alias of its input
    const size_t bytes = (size_t)c->maxPanels * fm_elems(c, l) * QCNN_PANEL * sizeof(float) + kSlack;
    HIP_TRY(c, hipMalloc(&c->fmBuf[l], bytes));
  }
  {
    size_t maxCt = 0;
    for (int l = 0; l < c->L; ++l)
      if (c->layers[l].type == QCNN_FCNT) maxCt = std::max<size_t>(maxCt, c->dims[l + 1].c);
    c->fcMaxCt = maxCt;
    c->fcPartialElems = (size_t)QK_MAX_FC_SPLIT * c->maxPanels * maxCt * QCNN_PANEL;
    if (c->fcPartialElems) HIP_TRY(c, hipMalloc(&c->fcPartial, c->fcPartialElems * sizeof(float)));
    if (c->firstFc >= 0 && c->shapes[c->firstFc].hasDmap)
      HIP_TRY(c, hipMalloc(&c->fcFlat, (size_t)c->maxPanels * fm_elems(c, c->firstFc) * QCNN_PANEL * sizeof(float) + kSlack));
  }
  c->ev.resize((size_t)kProfRing * kMaxStreams * c->L * 2);
  for (hipEvent_t& e : c->ev) HIP_TRY(c, hipEventCreate(&e));
  c->profSum.assign(c->L, 0.0);
  c->profLaunches.assign(c->L, 0);
  c->profCount = 0; c->profForwards = 0; c->profPending.clear();
  if (!c->evFork) HIP_TRY(c, hipEventCreateWithFlags(&c->evFork, hipEventDisableTiming));   // aux streams: on demand (run_layers)
  // first-FC flatten map: consumption index d = (ch*H + y)*W + x  ->  NHWC row (y*W + x)*C + ch  (src/CaffeEva.cc:187-189)
  for (int l = 0; l < c->L; ++l) {
    const LayerShape& s = c->shapes[l];
    if (!s.hasDmap) continue;
    const FmDims& a = c->dims[l];
    std::vector<int> map(fm_elems(c, l));
    for (int ch = 0; ch < a.c; ++ch)
      for (int y = 0; y < a.h; ++y)
        for (int x = 0; x < a.w; ++x) map[((size_t)ch * a.h + y) * a.w + x] = (y * a.w + x) * a.c + ch;
    HIP_TRY(c, hipMemcpyAsync(c->arena + s.offDmap, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->committed = true;
  return 0;
}

}  // extern "C"
