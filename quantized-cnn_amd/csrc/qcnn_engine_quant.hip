// qcnn_engine_quant.hip — the quantiser entry points (qcnn_quantize.hip's and qcnn_ec.hip's kernels behind checked C calls) and
// the resident calibration that run_layers feeds (qcnn_calib_begin .. qcnn_calib_end).
#include <limits.h>

#include <algorithm>
#include <cmath>

#include "qcnn_engine.h"

using namespace qcnn_engine;

namespace {

// device scratch of one qcnn_quantize_layer call: freed on every return path
struct PqScratch {
  std::vector<void*> bufs;
  hipError_t alloc(void** p, size_t bytes) {
    *p = nullptr;
    hipError_t e = hipMalloc(p, std::max<size_t>(bytes, 1));
    if (e == hipSuccess) bufs.push_back(*p);
    return e;
  }
  ~PqScratch() { for (void* v : bufs) (void)hipFree(v); }
};

constexpr size_t kCalibSlabBytes = (size_t)128 << 20;   // cap of the resident calibration's split scratch (part of its split rule)

}  // namespace

namespace qcnn_engine {

// the resident calibration matrices (hipFree waits for the launches that still write them)
void calib_free(QcnnCtx* c) {
  for (QcnnCtx::Calib::Layer& q : c->calib.layers)
    if (q.G) (void)hipFree(q.G);
  if (c->calib.slab) (void)hipFree(c->calib.slab);
  c->calib = QcnnCtx::Calib();
}

// Armed calibration: the second moments of the panels [pa, pb) of a batch of n images, added to the resident matrices on the
// context's stream — behind the join of the sub-batch streams, in front of whatever the caller enqueues next (the next batch's
// pack kernel, the event that hands a source buffer back).  fm: the pointer table of this call.
int calib_enqueue(QcnnCtx* c, const std::vector<float*>& fm, int n, int pa, int pb) {
  const int nLive = std::min(n, pb * QCNN_PANEL) - pa * QCNN_PANEL;
  for (QcnnCtx::Calib::Layer& q : c->calib.layers) {
    const int l = q.layer;
    if (!fm[l]) return fail(c, "calibration: the input map of layer %d does not exist as panels in this forward", l);
    int splits = 1;
    const long long per = qk_ec_gram_panel_units_per_split(q.g, pb - pa, kCalibSlabBytes, &splits);
    const int* dmap = c->shapes[l].hasDmap ? arena_at<const int>(c, c->shapes[l].offDmap) : nullptr;
    const hipError_t e = qk_ec_gram_panel(fm[l] + (size_t)pa * fm_elems(c, l) * QCNN_PANEL, dmap, q.g, pb - pa, nLive, per, splits,
                                          c->calib.slab, q.G, c->stream);
    if (e != hipSuccess) return fail(c, "calibration of layer %d: launch failed: %s", l, hipGetErrorString(e));
    q.rows += (long long)nLive * q.g.Ho * q.g.Wo;
  }
  return 0;
}

}  // namespace qcnn_engine

extern "C" {

int qcnn_quantize_layer(QcnnCtx* c, int Ct, int Cin, int kh, int kw, int M, int K, int Cs, const float* weights, const float* ctrd_init,
                        int max_iter, float* ctrd_out, uint8_t* asmt_out, double* sse2, int* iters2) {
  if (!c) return fail(nullptr, "qcnn_quantize_layer: ctx == NULL");
  if (Ct <= 0 || Cin <= 0 || kh <= 0 || kw <= 0) return fail(c, "qcnn_quantize_layer: bad layer shape Ct=%d Cin=%d kh=%d kw=%d", Ct, Cin, kh, kw);
  if (Cs < 1 || Cs > QCNN_PQ_MAX_CS) return fail(c, "qcnn_quantize_layer: Cs=%d outside [1, %d]", Cs, QCNN_PQ_MAX_CS);
  if (K < 2 || K > QCNN_PQ_MAX_K) return fail(c, "qcnn_quantize_layer: K=%d outside [2, %d]", K, QCNN_PQ_MAX_K);
  if (M < 1 || (long long)M * Cs < Cin) return fail(c, "qcnn_quantize_layer: M*Cs = %lld does not cover Cin = %d", (long long)M * Cs, Cin);
  if ((long long)(M - 1) * Cs >= Cin) return fail(c, "qcnn_quantize_layer: sub-space %d starts beyond Cin = %d (M*Cs must be < Cin + Cs)", M - 1, Cin);
  if (max_iter < 0) return fail(c, "qcnn_quantize_layer: max_iter=%d < 0", max_iter);
  if (!weights || !ctrd_out || !asmt_out) return fail(c, "qcnn_quantize_layer: weights, ctrd_out and asmt_out must not be NULL");
  const int taps = kh * kw;
  const long long Nll = (long long)Ct * taps;
  if (Nll * M >= (1LL << 31) || (Nll + 127) / 128 >= 65536) return fail(c, "qcnn_quantize_layer: %lld points x %d sub-spaces is too large", Nll, M);
  const int N = (int)Nll;
  const size_t wElems = (size_t)Nll * Cin;
  for (size_t i = 0; i < wElems; ++i)
    if (!std::isfinite(weights[i])) return fail(c, "qcnn_quantize_layer: weight %zu is not finite", i);
  const size_t cbElems = (size_t)M * K * Cs;
  if (ctrd_init)
    for (size_t i = 0; i < cbElems; ++i)
      if ((int)(i / ((size_t)K * Cs)) * Cs + (int)(i % Cs) < Cin && !std::isfinite(ctrd_init[i]))
        return fail(c, "qcnn_quantize_layer: initial code book entry %zu is not finite", i);
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t MN = (size_t)M * N;
  PqScratch sc;
  float *dW = nullptr, *pts = nullptr, *ctrd = nullptr, *dmin = nullptr;
  uint8_t* asmt = nullptr;
  int* chg = nullptr;
  double* partial = nullptr;
  const int nPart = qk_pq_finalize_blocks(MN);
  HIP_TRY(c, sc.alloc((void**)&pts, MN * Cs * sizeof(float)));
  HIP_TRY(c, sc.alloc((void**)&ctrd, cbElems * sizeof(float)));
  HIP_TRY(c, sc.alloc((void**)&dmin, MN * sizeof(float)));
  HIP_TRY(c, sc.alloc((void**)&asmt, MN));
  HIP_TRY(c, sc.alloc((void**)&chg, 2 * sizeof(int) * M));            // two changed-flag sets: the last step's (= this step's active set) and this step's
  HIP_TRY(c, sc.alloc((void**)&partial, nPart * sizeof(double)));
  {
    PqScratch wsc;                                        // the dense weights live only until they are gathered into points
    HIP_TRY(c, wsc.alloc((void**)&dW, wElems * sizeof(float)));
    HIP_TRY(c, hipMemcpyAsync(dW, weights, wElems * sizeof(float), hipMemcpyHostToDevice, st));
    HIP_TRY(c, qk_pq_gather(dW, pts, N, Cin, taps, M, Cs, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  if (ctrd_init) {
    HIP_TRY(c, hipMemcpyAsync(ctrd, ctrd_init, cbElems * sizeof(float), hipMemcpyHostToDevice, st));
  } else {
    HIP_TRY(c, qk_pq_seed(pts, ctrd, dmin, M, N, K, Cs, st));
  }
  std::vector<double> part(nPart);
  auto sse = [&](double* out) -> int {
    HIP_TRY(c, qk_pq_finalize(dmin, MN, ctrd, M, K, Cs, Cin, partial, st));
    HIP_TRY(c, hipMemcpyAsync(part.data(), partial, nPart * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    double s = 0.0;
    for (double v : part) s += v;
    *out = s;
    return 0;
  };
  double sseInit = 0.0, sseFinal = 0.0;
  HIP_TRY(c, qk_pq_assign(pts, ctrd, asmt, dmin, nullptr, nullptr, M, N, K, Cs, Cin, 1, st));
  if (sse(&sseInit)) return 1;
  // Lloyd steps: update, then re-assign, on the sub-spaces whose assignments changed in the previous step (all at first).  A
  // sub-space whose assignments did not change is a fixed point: leaving it alone gives the bits running it would give.
  std::vector<int> flags(M);
  int steps = 0, changing = 0;
  int* active = nullptr;
  int* cur = chg;
  for (int it = 0; it < max_iter; ++it) {
    HIP_TRY(c, qk_pq_update(pts, ctrd, asmt, active, M, N, K, Cs, Cin, st));
    HIP_TRY(c, hipMemsetAsync(cur, 0, sizeof(int) * M, st));
    HIP_TRY(c, qk_pq_assign(pts, ctrd, asmt, dmin, cur, active, M, N, K, Cs, Cin, 0, st));
    HIP_TRY(c, hipMemcpyAsync(flags.data(), cur, sizeof(int) * M, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    ++steps;
    changing = 0;
    for (int v : flags) changing += v != 0;
    if (!changing) break;
    active = cur;
    cur = (cur == chg) ? chg + M : chg;
  }
  if (sse(&sseFinal)) return 1;
  HIP_TRY(c, hipMemcpyAsync(ctrd_out, ctrd, cbElems * sizeof(float), hipMemcpyDeviceToHost, st));
  // device [M][N] -> file order [Ct][kh][kw][M] = [N][M]
  std::vector<uint8_t> a(MN);
  HIP_TRY(c, hipMemcpyAsync(a.data(), asmt, MN, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < N; ++n) asmt_out[(size_t)n * M + m] = a[(size_t)m * N + n];
  if (sse2) { sse2[0] = sseInit; sse2[1] = sseFinal; }
  if (iters2) { iters2[0] = steps; iters2[1] = changing; }
  return 0;
}

int qcnn_calib_gram(QcnnCtx* c, int H, int W, int Cin_total, int grp, int kh, int kw, int stride, int pad, const float* in_nhwc, int n,
                    double* gram, int accumulate) {
  if (!c) return fail(nullptr, "qcnn_calib_gram: ctx == NULL");
  if (H <= 0 || W <= 0 || Cin_total <= 0 || grp <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || n <= 0)
    return fail(c, "qcnn_calib_gram: bad geometry H=%d W=%d C=%d grp=%d kh=%d kw=%d stride=%d pad=%d n=%d", H, W, Cin_total, grp, kh, kw,
                stride, pad, n);
  if (Cin_total % grp) return fail(c, "qcnn_calib_gram: %d channels do not divide into %d groups", Cin_total, grp);
  if (H + 2 * pad < kh || W + 2 * pad < kw) return fail(c, "qcnn_calib_gram: a %dx%d window does not fit a %dx%d map with pad %d", kh, kw, H, W, pad);
  if (!in_nhwc || !gram) return fail(c, "qcnn_calib_gram: in_nhwc and gram must not be NULL");
  QkGramGeom s;
  s.H = H; s.W = W; s.C = Cin_total; s.grp = grp; s.Cg = Cin_total / grp; s.kh = kh; s.kw = kw; s.stride = stride; s.pad = pad;
  s.Ho = conv_out(H, kh, stride, pad);
  s.Wo = conv_out(W, kw, stride, pad);
  const long long Pll = (long long)kh * kw * s.Cg;
  if (Pll > 46340) return fail(c, "qcnn_calib_gram: patch length %lld is too large", Pll);        // P * P stays below 2^31
  s.P = (int)Pll;
  s.rows = (long long)n * s.Ho * s.Wo;
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  const size_t inElems = (size_t)n * H * W * Cin_total, gElems = (size_t)grp * s.P * s.P;
  int splits = 1;
  const long long per = qk_ec_gram_rows_per_split(s, (size_t)2 << 30, &splits);
  PqScratch sc;
  float* dIn = nullptr;
  double *dG = nullptr, *slab = nullptr;
  HIP_TRY(c, sc.alloc((void**)&dIn, inElems * sizeof(float)));
  HIP_TRY(c, sc.alloc((void**)&dG, gElems * sizeof(double)));
  HIP_TRY(c, sc.alloc((void**)&slab, gElems * sizeof(double) * splits));
  HIP_TRY(c, hipMemcpyAsync(dIn, in_nhwc, inElems * sizeof(float), hipMemcpyHostToDevice, st));
  if (accumulate) HIP_TRY(c, hipMemcpyAsync(dG, gram, gElems * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(c, qk_ec_gram(dIn, s, per, splits, slab, dG, accumulate ? 1 : 0, st));
  HIP_TRY(c, hipMemcpyAsync(gram, dG, gElems * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return 0;
}

int qcnn_quantize_layer_ec(QcnnCtx* c, int Ct, int Cin, int grp, int kh, int kw, int M, int K, int Cs, const float* weights,
                           const double* gram, const float* ctrd_init, const uint8_t* asmt_init, int sweeps, double ridge, float* ctrd_out,
                           uint8_t* asmt_out, double* obj_trace, int* changed_trace) {
  if (!c) return fail(nullptr, "qcnn_quantize_layer_ec: ctx == NULL");
  if (Ct <= 0 || Cin <= 0 || kh <= 0 || kw <= 0) return fail(c, "qcnn_quantize_layer_ec: bad layer shape Ct=%d Cin=%d kh=%d kw=%d", Ct, Cin, kh, kw);
  if (grp <= 0 || Ct % grp) return fail(c, "qcnn_quantize_layer_ec: Ct=%d does not divide into grp=%d groups", Ct, grp);
  if (Cs < 1 || Cs > QCNN_PQ_MAX_CS) return fail(c, "qcnn_quantize_layer_ec: Cs=%d outside [1, %d]", Cs, QCNN_PQ_MAX_CS);
  if (K < 2 || K > QCNN_PQ_MAX_K) return fail(c, "qcnn_quantize_layer_ec: K=%d outside [2, %d]", K, QCNN_PQ_MAX_K);
  if (M < 1 || (long long)M * Cs < Cin) return fail(c, "qcnn_quantize_layer_ec: M*Cs = %lld does not cover Cin = %d", (long long)M * Cs, Cin);
  if ((long long)(M - 1) * Cs >= Cin) return fail(c, "qcnn_quantize_layer_ec: sub-space %d starts beyond Cin = %d (M*Cs must be < Cin + Cs)", M - 1, Cin);
  if (sweeps < 0) return fail(c, "qcnn_quantize_layer_ec: sweeps=%d < 0", sweeps);
  if (!(ridge >= 0.0) || !std::isfinite(ridge)) return fail(c, "qcnn_quantize_layer_ec: ridge=%g must be finite and >= 0", ridge);
  if (!weights || !ctrd_init || !asmt_init || !ctrd_out || !asmt_out)
    return fail(c, "qcnn_quantize_layer_ec: weights, ctrd_init, asmt_init, ctrd_out and asmt_out must not be NULL");
  const int taps = kh * kw;
  const long long Nll = (long long)Ct * taps, Pll = (long long)taps * Cin;
  if (Nll * M >= (1LL << 31) || Pll > 46340) return fail(c, "qcnn_quantize_layer_ec: %lld points x %d sub-spaces x patch length %lld is too large", Nll, M, Pll);
  QkEcShape s;
  s.Ct = Ct; s.Cin = Cin; s.grp = grp; s.taps = taps; s.M = M; s.K = K; s.Cs = Cs; s.P = (int)Pll; s.N = (int)Nll;
  const size_t wElems = (size_t)Nll * Cin, cbElems = (size_t)M * K * Cs, MN = (size_t)M * s.N, pp = (size_t)s.P * s.P, gElems = pp * grp;
  for (size_t i = 0; i < wElems; ++i)
    if (!std::isfinite(weights[i])) return fail(c, "qcnn_quantize_layer_ec: weight %zu is not finite", i);
  std::vector<float> book(ctrd_init, ctrd_init + cbElems);
  for (size_t i = 0; i < cbElems; ++i) {
    if ((int)(i / ((size_t)K * Cs)) * Cs + (int)(i % Cs) >= Cin) book[i] = 0.0f;                // dims >= CsEff stay 0
    else if (!std::isfinite(book[i])) return fail(c, "qcnn_quantize_layer_ec: code book entry %zu is not finite", i);
  }
  std::vector<uint8_t> a(MN);                                                                       // file order [N][M] -> device [M][N]
  for (int n = 0; n < s.N; ++n)
    for (int m = 0; m < M; ++m) {
      const uint8_t v = asmt_init[(size_t)n * M + m];
      if (v >= K) return fail(c, "qcnn_quantize_layer_ec: assignment %zu is %d, the book has %d code words", (size_t)n * M + m, (int)v, K);
      a[(size_t)m * s.N + n] = v;
    }
  double lambda = ridge;                                                                           // identity: trace(G) / P = 1
  if (gram) {
    for (size_t i = 0; i < gElems; ++i)
      if (!std::isfinite(gram[i])) return fail(c, "qcnn_quantize_layer_ec: gram entry %zu is not finite", i);
    double tr = 0.0;
    for (int g = 0; g < grp; ++g)
      for (int p = 0; p < s.P; ++p) {
        const double d = gram[(size_t)g * pp + (size_t)p * s.P + p];
        if (d < 0.0) return fail(c, "qcnn_quantize_layer_ec: gram diagonal entry %d of group %d is negative (%g)", p, g, d);
        tr += d;
      }
    lambda = ridge * tr / ((double)grp * s.P);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  hipStream_t st = c->stream;
  PqScratch sc;
  float *dW = nullptr, *ctrd = nullptr;
  uint8_t* asmt = nullptr;
  double *G = nullptr, *E = nullptr, *Hm = nullptr, *partial = nullptr, *dw = nullptr;
  int *flags = nullptr, *off = nullptr, *list = nullptr;                                           // flags: chg [Ct] + moved [1]
  const int nPart = qk_ec_objective_blocks(s);
  HIP_TRY(c, sc.alloc((void**)&dW, wElems * sizeof(float)));
  HIP_TRY(c, sc.alloc((void**)&ctrd, cbElems * sizeof(float)));
  HIP_TRY(c, sc.alloc((void**)&asmt, MN));
  HIP_TRY(c, sc.alloc((void**)&G, gElems * sizeof(double)));
  HIP_TRY(c, sc.alloc((void**)&E, (size_t)Ct * s.P * sizeof(double)));
  HIP_TRY(c, sc.alloc((void**)&Hm, (size_t)Ct * s.P * sizeof(double)));
  HIP_TRY(c, sc.alloc((void**)&partial, nPart * sizeof(double)));
  HIP_TRY(c, sc.alloc((void**)&dw, (size_t)K * Cs * sizeof(double)));
  HIP_TRY(c, sc.alloc((void**)&flags, (Ct + 1) * sizeof(int)));
  HIP_TRY(c, sc.alloc((void**)&off, (K + 1) * sizeof(int)));
  HIP_TRY(c, sc.alloc((void**)&list, s.N * sizeof(int)));
  HIP_TRY(c, hipMemcpyAsync(dW, weights, wElems * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(ctrd, book.data(), cbElems * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(asmt, a.data(), MN, hipMemcpyHostToDevice, st));
  if (gram) {
    HIP_TRY(c, hipMemcpyAsync(G, gram, gElems * sizeof(double), hipMemcpyHostToDevice, st));
  } else {
    HIP_TRY(c, qk_ec_identity(G, s.P, grp, st));
  }
  std::vector<double> part(nPart);
  std::vector<int> hflags(Ct + 1);
  // J from scratch in fp64; leaves E and Hm = E G of this moment behind, which the next sweep starts from
  auto objective = [&](double* out) -> int {
    HIP_TRY(c, qk_ec_evaluate(dW, ctrd, asmt, G, E, Hm, partial, s, st));
    HIP_TRY(c, hipMemcpyAsync(part.data(), partial, nPart * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    double sum = 0.0;
    for (double v : part) sum += v;
    *out = sum;
    return 0;
  };
  double obj = 0.0;
  if (objective(&obj)) return 1;
  if (obj_trace) obj_trace[0] = obj;
  bool done = false;
  for (int sw = 0; sw < sweeps; ++sw) {
    int changed = 0;
    if (!done) {
      HIP_TRY(c, hipMemsetAsync(flags, 0, (Ct + 1) * sizeof(int), st));
      for (int m = 0; m < M; ++m) {
        for (int t = 0; t < taps; ++t) HIP_TRY(c, qk_ec_assign(ctrd, asmt, G, E, Hm, flags, s, m, t, st));
        HIP_TRY(c, qk_ec_update(ctrd, asmt, off, list, G, E, Hm, dw, flags + Ct, s, m, lambda, st));
      }
      HIP_TRY(c, hipMemcpyAsync(hflags.data(), flags, (Ct + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      for (int i = 0; i < Ct; ++i) changed += hflags[i];
      if (objective(&obj)) return 1;
      done = changed == 0 && hflags[Ct] == 0;
    }
    if (obj_trace) obj_trace[sw + 1] = obj;
    if (changed_trace) changed_trace[sw] = changed;
  }
  HIP_TRY(c, hipMemcpyAsync(ctrd_out, ctrd, cbElems * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(a.data(), asmt, MN, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < s.N; ++n) asmt_out[(size_t)n * M + m] = a[(size_t)m * s.N + n];
  return 0;
}

int qcnn_calib_begin(QcnnCtx* c, const int* layers, int n_layers) {
  if (!c) return fail(nullptr, "qcnn_calib_begin: ctx == NULL");
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "qcnn_calib_begin: model not committed");
  if (c->calib.active) return fail(c, "qcnn_calib_begin: a calibration is already open (qcnn_calib_end closes it)");
  if (!layers || n_layers <= 0) return fail(c, "qcnn_calib_begin: no layers");
  // every layer is checked before anything is allocated
  std::vector<QcnnCtx::Calib::Layer> list;
  size_t slabBytes = 0;
  for (int i = 0; i < n_layers; ++i) {
    const int l = layers[i];
    if (l < 0 || l >= c->L) return fail(c, "qcnn_calib_begin: layer %d out of range", l);
    const QcnnLayerDesc& d = c->layers[l];
    if (d.type != QCNN_CONV && d.type != QCNN_FCNT) return fail(c, "qcnn_calib_begin: layer %d is neither conv nor FC", l);
    for (const QcnnCtx::Calib::Layer& q : list)
      if (q.layer == l) return fail(c, "qcnn_calib_begin: layer %d is listed twice", l);
    // the input map of a conv / FC layer is never fused away: an LRN + pool pair drops the map BETWEEN the two, a fused ReLU
    // aliases a map that holds the rectified values, dropout is a copy.  Only fm[0] can be missing (the NCHW input read in
    // place), and that route is switched off while layer 0 is armed; a map without a buffer would be a planning error
    if (l > 0 && !c->fmBuf[l] && c->layers[l - 1].type != QCNN_DRPT)
      return fail(c, "qcnn_calib_begin: the input map of layer %d never exists as a panel map", l);
    QcnnCtx::Calib::Layer q;
    q.layer = l;
    QkGramGeom& s = q.g;
    const bool conv = d.type == QCNN_CONV;
    const FmDims& a = c->dims[l];
    s.H = conv ? a.h : 1; s.W = conv ? a.w : 1; s.C = conv ? a.c : (int)fm_elems(c, l);
    s.grp = conv ? d.grpCnt : 1; s.Cg = s.C / s.grp;
    s.kh = s.kw = conv ? d.knlSiz : 1; s.stride = conv ? d.stride : 1; s.pad = conv ? d.padSiz : 0;
    s.Ho = conv_out(s.H, s.kh, s.stride, s.pad);
    s.Wo = conv_out(s.W, s.kw, s.stride, s.pad);
    const long long Pll = (long long)s.kh * s.kw * s.Cg;
    if (Pll > 46340) return fail(c, "qcnn_calib_begin: layer %d: patch length %lld is too large", l, Pll);    // P * P stays below 2^31
    s.P = (int)Pll;
    s.rows = 0;
    if ((long long)c->maxPanels * s.Ho * s.Wo > INT_MAX) return fail(c, "qcnn_calib_begin: layer %d: too many output pixels per batch", l);
    int splits = 1;                                      // the most any panel count asks for (rounding: not monotonic)
    for (int p = 1; p <= c->maxPanels; ++p) {
      int z = 1;
      (void)qk_ec_gram_panel_units_per_split(s, p, kCalibSlabBytes, &z);
      splits = std::max(splits, z);
    }
    if (splits > 1) slabBytes = std::max(slabBytes, (size_t)splits * s.grp * s.P * s.P * sizeof(double));
    list.push_back(q);
  }
  for (QcnnCtx::Calib::Layer& q : list) {
    const size_t bytes = (size_t)q.g.grp * q.g.P * q.g.P * sizeof(double);
    hipError_t e = hipMalloc(&q.G, bytes);
    if (e == hipSuccess) e = hipMemsetAsync(q.G, 0, bytes, c->stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      for (QcnnCtx::Calib::Layer& r : list) if (r.G) (void)hipFree(r.G);
      return fail(c, "qcnn_calib_begin: layer %d: %zu bytes for its matrix: %s", q.layer, bytes, hipGetErrorString(e));
    }
  }
  double* slab = nullptr;
  if (slabBytes && hipMalloc(&slab, slabBytes) != hipSuccess) {
    (void)hipGetLastError();
    for (QcnnCtx::Calib::Layer& r : list) (void)hipFree(r.G);
    return fail(c, "qcnn_calib_begin: %zu bytes of split scratch do not fit the device", slabBytes);
  }
  c->calib.layers = list;
  c->calib.slab = slab;
  c->calib.wantsInput = false;
  for (const QcnnCtx::Calib::Layer& q : list) c->calib.wantsInput = c->calib.wantsInput || q.layer == 0;
  c->calib.active = c->calib.armed = true;
  return 0;
}

int qcnn_calib_arm(QcnnCtx* c, int on) {
  if (!c) return fail(nullptr, "qcnn_calib_arm: ctx == NULL");
  if (!c->calib.active) return fail(c, "qcnn_calib_arm: no calibration is open (qcnn_calib_begin)");
  c->calib.armed = on != 0;
  return 0;
}

int qcnn_calib_read(QcnnCtx* c, int layer, double* gram_host, long long* rows) {
  if (!c) return fail(nullptr, "qcnn_calib_read: ctx == NULL");
  if (!c->calib.active) return fail(c, "qcnn_calib_read: no calibration is open (qcnn_calib_begin)");
  for (const QcnnCtx::Calib::Layer& q : c->calib.layers) {
    if (q.layer != layer) continue;
    HIP_TRY(c, hipSetDevice(c->device));
    if (gram_host) {
      HIP_TRY(c, hipMemcpyAsync(gram_host, q.G, (size_t)q.g.grp * q.g.P * q.g.P * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    if (rows) *rows = q.rows;
    return 0;
  }
  return fail(c, "qcnn_calib_read: layer %d is not part of the open calibration", layer);
}

int qcnn_calib_end(QcnnCtx* c) {
  if (!c) return fail(nullptr, "qcnn_calib_end: ctx == NULL");
  if (!c->calib.active) return fail(c, "qcnn_calib_end: no calibration is open (qcnn_calib_begin)");
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  calib_free(c);
  return 0;
}

}  // extern "C"
