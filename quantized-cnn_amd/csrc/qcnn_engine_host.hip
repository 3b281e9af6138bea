// qcnn_engine_host.hip — forwards whose input and results lie in host memory: one batch (qcnn_forward_host), batches streamed
// through the double-buffered schedule (host_batch_schedule: qcnn_forward_host_batches here, the 8-bit streams in
// qcnn_engine_u8.hip), and the pinned / registered memory calls that let their copies run as DMA transfers.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "qcnn_engine.h"

using namespace qcnn_engine;

// the results of a finished forward, from the staging buffers into the caller's memory; blocking
static int download_outputs(QcnnCtx* c, int n, float* prob_host, uint16_t* top5_host) {
  const size_t classes = fm_elems(c, c->L);
  if (prob_host)
    HIP_TRY(c, hipMemcpyAsync(prob_host, c->stageOut, (size_t)n * classes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (top5_host)
    HIP_TRY(c, hipMemcpyAsync(top5_host, c->stageTop5, (size_t)n * 5 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// The reference's image loop (src/CaffeEva.cc:151-211) classifies one batch after the other; here the upload of batch
// b + 1 (copy stream, second input buffer) runs under the compute step of batch b, and the results come back through pinned
// buffers one batch late, so that neither direction of PCIe is ever waited for by the kernels.  The caller has checked every
// batch and grown every buffer (ensure_pipeline / ensure_u8_stream): nothing is allocated inside the schedule.
int qcnn_engine::host_batch_schedule(QcnnCtx* c, int nb, const HostBatchJob& job) {
  // QCNN_DEBUG_PIPELINE=1: time every upload and every batch's kernels with events and print the schedule afterwards
  static const bool dbg = [] { const char* e = getenv("QCNN_DEBUG_PIPELINE"); return e && atoi(e) != 0; }();
  std::vector<hipEvent_t> dbgEv;                        // per batch: upload start, end, compute start, end; the last: time zero
  auto mark = [&](int b, int j, hipStream_t st) -> int {
    if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + j], st));
    return 0;
  };
  auto upload = [&](int b) -> int {
    const int k = b & 1;
    if (job.stage && job.stage(b, k)) return 1;
    HIP_TRY(c, hipStreamWaitEvent(c->copyStream, c->evFreed[k], 0));
    if (mark(b, 0, c->copyStream) || job.upload(b, k) || mark(b, 1, c->copyStream)) return 1;
    HIP_TRY(c, hipEventRecord(c->evCopied[k], c->copyStream));
    return 0;
  };
  auto collect = [&](int b) -> int {
    HIP_TRY(c, hipEventSynchronize(c->evDone[b & 1]));
    for (const HostResult& r : job.results(b, b & 1))
      if (r.host) memcpy(r.host, r.pin, r.bytes);
    return 0;
  };
  auto run = [&]() -> int {
    // the copy stream may not touch an input buffer before everything already enqueued on the compute stream has read it
    for (int k = 0; k < 2; ++k) { HIP_TRY(c, hipEventRecord(c->evFreed[k], c->stream)); c->freedValid[k] = true; }
    if (job.prologue && job.prologue()) return 1;
    if (dbg) {
      dbgEv.resize((size_t)nb * 4 + 1);
      for (hipEvent_t& e : dbgEv) HIP_TRY(c, hipEventCreate(&e));
      HIP_TRY(c, hipEventRecord(dbgEv[(size_t)nb * 4], c->stream));
    }
    if (upload(0)) return 1;
    for (int b = 0; b < nb; ++b) {
      const int k = b & 1;
      if (b + 1 < nb && upload(b + 1)) return 1;
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evCopied[k], 0));
      if (mark(b, 2, c->stream) || job.compute(b, k, c->evFreed[k]) || mark(b, 3, c->stream)) return 1;
      for (const HostResult& r : job.results(b, k))
        if (r.host) HIP_TRY(c, hipMemcpyAsync(r.pin, r.dev, r.bytes, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipEventRecord(c->evDone[k], c->stream));
      if (b >= 1 && collect(b - 1)) return 1;
    }
    if ((job.epilogue && job.epilogue()) || collect(nb - 1)) return 1;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->copyStream));
    return 0;
  };
  if (run()) {                                          // the caller's memory is not read behind a failed call's return
    (void)hipStreamSynchronize(c->copyStream);
    (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : dbgEv) if (e) (void)hipEventDestroy(e);
    return 1;
  }
  for (int b = 0; dbg && b < nb; ++b) {
    float t[4];
    for (int j = 0; j < 4; ++j) HIP_TRY(c, hipEventElapsedTime(&t[j], dbgEv[(size_t)nb * 4], dbgEv[(size_t)b * 4 + j]));
    fprintf(stderr, "[qcnn pipeline] batch %d (%d images): upload %.2f -> %.2f ms, layers %.2f -> %.2f ms\n", b, job.images(b), t[0],
            t[1], t[2], t[3]);
  }
  for (hipEvent_t e : dbgEv) (void)hipEventDestroy(e);
  return 0;
}

extern "C" {

int qcnn_host_register(void* ptr, size_t bytes) {
  if (!ptr || !bytes) return fail(nullptr, "qcnn_host_register: empty range");
  const hipError_t e = hipHostRegister(ptr, bytes, hipHostRegisterPortable);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, "hipHostRegister(%zu bytes) -> %s", bytes, hipGetErrorString(e)); }
  return 0;
}

int qcnn_host_alloc(size_t bytes, void** out) {
  if (!out || !bytes) return fail(nullptr, "qcnn_host_alloc: empty request");
  *out = nullptr;
  const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocPortable);
  if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return fail(nullptr, "hipHostMalloc(%zu bytes) -> %s", bytes, hipGetErrorString(e)); }
  return 0;
}

int qcnn_host_free(void* ptr) {
  if (!ptr) return 0;
  const hipError_t e = hipHostFree(ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, "hipHostFree -> %s", hipGetErrorString(e)); }
  return 0;
}

int qcnn_host_unregister(void* ptr) {
  if (!ptr) return 0;
  const hipError_t e = hipHostUnregister(ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(nullptr, "hipHostUnregister -> %s", hipGetErrorString(e)); }
  return 0;
}

// float crops through stageIn / stageIn1, one qcnn_forward per batch
int qcnn_forward_host_batches(QcnnCtx* c, const float* const* in_host, const int* n, int nb, float* const* prob_host,
                              uint16_t* const* top5_host) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (nb <= 0 || !in_host || !n) return fail(c, "qcnn_forward_host_batches: no batches");
  for (int b = 0; b < nb; ++b)
    if (n[b] <= 0 || n[b] > c->maxBatch || !in_host[b]) return fail(c, "batch %d: %d images outside (0, %d]", b, n[b], c->maxBatch);
  if (ensure_pipeline(c)) return 1;
  const size_t inE = fm_elems(c, 0), classes = fm_elems(c, c->L);
  float* const dIn[2] = {c->stageIn, c->stageIn1};
  auto prob = [&](int b) { return prob_host ? prob_host[b] : nullptr; };
  auto top5 = [&](int b) { return top5_host ? top5_host[b] : nullptr; };
  HostBatchJob job;
  job.images = [&](int b) { return n[b]; };
  job.upload = [&](int b, int k) -> int {
    HIP_TRY(c, hipMemcpyAsync(dIn[k], in_host[b], inE * n[b] * sizeof(float), hipMemcpyHostToDevice, c->copyStream));
    return 0;
  };
  job.compute = [&](int b, int k, hipEvent_t freed) -> int {       // the forward reads its input to the end: handed back behind all of it
    if (qcnn_forward(c, dIn[k], n[b], prob(b) ? c->stageOut : nullptr, top5(b) ? c->stageTop5 : nullptr)) return 1;
    HIP_TRY(c, hipEventRecord(freed, c->stream));
    return 0;
  };
  job.results = [&](int b, int k) {
    return std::vector<HostResult>{{c->stageOut, c->pinProb[k], prob(b), (size_t)n[b] * classes * sizeof(float)},
                                   {c->stageTop5, c->pinTop5[k], top5(b), (size_t)n[b] * 5 * sizeof(uint16_t)}};
  };
  return host_batch_schedule(c, nb, job);
}

int qcnn_count_top5_hits(QcnnCtx* c, const uint16_t* top5_dev, const uint16_t* labels_dev, int n, unsigned long long* hits5_dev) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!top5_dev || !labels_dev || !hits5_dev) return fail(c, "qcnn_count_top5_hits: top5, labels or hits5 == NULL");
  if (n <= 0) return fail(c, "qcnn_count_top5_hits: no image (n = %d)", n);
  const hipError_t e = qk_top5_hits(top5_dev, labels_dev, n, hits5_dev, c->stream);
  if (e != hipSuccess) return fail(c, "hit count launch failed: %s", hipGetErrorString(e));
  return 0;
}

int qcnn_forward_host(QcnnCtx* c, const float* in_nchw_host, int n, float* prob_host, uint16_t* top5_host) {
  if (open_batch(c, n)) return 1;
  const size_t inE = fm_elems(c, 0);
  if (c->hostChunk > 0 && n >= 2 * c->hostChunk * QCNN_PANEL) {
    // A batch of at least two chunks (QCNN_OPT_HOST_CHUNK panels each, default two) goes through chunk by chunk: every chunk is uploaded on the copy stream
    // into its place of the batch's input buffer, and its layers start as soon as it has arrived — the upload of chunk
    // k + 1 (a DMA transfer from pinned / registered memory, a staged copy otherwise) runs under the layers of chunk k.
    // All chunks write into the same whole-batch feature maps, so dumps and results are those of one launch.
    if (ensure_pipeline(c)) return 1;
    const int panelsAll = (n + QCNN_PANEL - 1) / QCNN_PANEL;
    const int chunkPanels = c->hostChunk;
    const int nc = (panelsAll + chunkPanels - 1) / chunkPanels;
    while ((int)c->evChunk.size() < nc) {
      hipEvent_t ev;
      HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      c->evChunk.push_back(ev);
    }
    const bool direct = direct_input(c, n);
    HIP_TRY(c, hipEventRecord(c->evFreed[0], c->stream));            // the buffer may still feed an earlier forward
    HIP_TRY(c, hipStreamWaitEvent(c->copyStream, c->evFreed[0], 0));
    for (int k = 0; k < nc; ++k) {
      const size_t first = (size_t)k * chunkPanels * QCNN_PANEL;
      const size_t cnt = std::min<size_t>((size_t)chunkPanels * QCNN_PANEL, (size_t)n - first);
      HIP_TRY(c, hipMemcpyAsync(c->stageIn + first * inE, in_nchw_host + first * inE, cnt * inE * sizeof(float),
                                hipMemcpyHostToDevice, c->copyStream));
      HIP_TRY(c, hipEventRecord(c->evChunk[k], c->copyStream));
    }
    for (int k = 0; k < nc; ++k) {
      const int pa = k * chunkPanels, pb = std::min(panelsAll, pa + chunkPanels);
      const size_t first = (size_t)pa * QCNN_PANEL;
      const int cnt = (int)std::min<size_t>((size_t)(pb - pa) * QCNN_PANEL, (size_t)n - first);
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evChunk[k], 0));
      if (!direct) {
        const hipError_t e = qk_pack_nchw(c->stageIn + first * inE, c->fmBuf[0] + first * inE, cnt, c->inC, c->inH, c->inW, c->stream);
        if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
      }
      if (run_layers(c, n, direct ? c->stageIn : nullptr, pa, pb)) return 1;
    }
    if (forward_outputs(c, n, prob_host ? c->stageOut : nullptr, top5_host ? c->stageTop5 : nullptr)) return 1;
    return download_outputs(c, n, prob_host, top5_host);
  }
  if (ensure_stage(c)) return 1;
  HIP_TRY(c, hipMemcpyAsync(c->stageIn, in_nchw_host, inE * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (qcnn_forward(c, c->stageIn, n, prob_host ? c->stageOut : nullptr, top5_host ? c->stageTop5 : nullptr)) return 1;
  return download_outputs(c, n, prob_host, top5_host);
}

}  // extern "C"
