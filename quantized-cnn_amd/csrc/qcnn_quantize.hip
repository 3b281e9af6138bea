// qcnn_quantize.hip — product-quantisation k-means (Lloyd's algorithm) of one dense conv / FC layer into the Q-CNN
// parameter form the rest of the library runs: sub-codebooks [M][K][Cs] + one-byte assignments (qcnn_quantize_layer,
// include/qcnn_hip.h).  The reference ships only the result of this step (its parameters came from MATLAB code that
// was not released); the layout it produces is the one src/CaffeEva.cc:1261-1296 (GetInPdMat) consumes.
//
// Every result is specified to the bit (DESIGN.md "Quantising dense weights"), so the kernels keep a fixed order:
//   distance   fp32, one rounding per operation, no contraction: d = 0; for j: t = p_j - c_j; d = d + t * t
//   assign     argmin over k = 0..K-1 with a strict '<' (ties to the lowest k)
//   update     per code word an fp64 sum of its members' coordinates in ascending point order, divided in fp64, rounded to
//              fp32 once; a code word without members keeps its value.  No float atomics anywhere.
//   seeding    farthest-first: c_0 = point 0, then the point farthest from its nearest chosen code word (ties to the lowest n)
//
// Points live on the device as [M][N][Cs] (sub-space major, each point's Cs coordinates contiguous, dims j >= CsEff
// zero).  Kernels (stable names for rocprofv3 --kernel-trace --stats):
//   k_pq_gather    dense file layout [Ct][Cin][kh][kw] -> points                       one thread per (point, sub-space)
//   k_pq_seed      farthest-first code book                                            one workgroup per sub-space
//   k_pq_assign    nearest code word of every point, changed-flag per sub-space        one workgroup per (sub-space, 128 points)
//   k_pq_update    code book from the assignments                                      one workgroup per sub-space, a lane per code word
//   k_pq_finalize  zero the padded dims of the code book; fp64 partial sums of the minimum distances (SSE)
#include <algorithm>

#include "qcnn_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kAssignThreads = 128;
constexpr int kSeedThreads = 256;
constexpr int kUpdateChunk = 4096;     // assignment bytes staged in LDS per pass of k_pq_update
constexpr int kFinalThreads = 256;

__device__ inline int cs_eff(int Cin, int Cs, int m) { return min(Cin - m * Cs, Cs); }

// point n = ct * taps + t of sub-space m; i = n * M + m, so that consecutive lanes read consecutive weights of one row
__global__ __launch_bounds__(256) void k_pq_gather(const float* __restrict__ w, float* __restrict__ pts, int N, int Cin, int taps,
                                                   int M, int Cs) {
  const int total = M * N;     // < 2^31 (checked by the caller)
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int m = i % M, n = i / M;
    const int ct = n / taps, t = n - ct * taps;
    const float* src = w + ((size_t)ct * Cin + m * Cs) * taps + t;
    float* dst = pts + ((size_t)m * N + n) * Cs;
    for (int j = 0; j < Cs; ++j) dst[j] = m * Cs + j < Cin ? src[(size_t)j * taps] : 0.0f;
  }
}

template <int CSM>
__device__ inline float pq_dist(const float (&p)[CSM], const float* c) {
  float d = 0.0f;
#pragma unroll
  for (int j = 0; j < CSM; ++j) {
    const float t = p[j] - c[j];
    d = d + t * t;
  }
  return d;
}

// Farthest-first seeding of sub-space blockIdx.x.  dmin[m][n] holds every point's distance to its nearest chosen code
// word; round i folds in code word i - 1 and picks the farthest point (a block-wide argmax, ties to the lowest n).
// The code word is held with CSM slots whose dims >= Cs are zero, as are the points' dims >= CsEff: a zero dim adds
// (+0) * (+0) = +0 to a sum of squares, which leaves it unchanged, so the distance is exactly the CsEff-dim one.
template <int CSM>
__global__ __launch_bounds__(kSeedThreads) void k_pq_seed(const float* __restrict__ pts, float* __restrict__ ctrd,
                                                          float* __restrict__ dmin, int N, int K, int Cs) {
  __shared__ float cw[CSM];
  __shared__ float wBest[kSeedThreads / 64];
  __shared__ int wIdx[kSeedThreads / 64];
  __shared__ int pick;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* P = pts + (size_t)m * N * Cs;
  float* D = dmin + (size_t)m * N;
  float* C = ctrd + (size_t)m * K * Cs;
  int cur = 0;
  for (int i = 0; i < K; ++i) {
    if (tid < CSM) cw[tid] = tid < Cs ? P[(size_t)cur * Cs + tid] : 0.0f;
    if (tid < Cs) C[(size_t)i * Cs + tid] = P[(size_t)cur * Cs + tid];
    __syncthreads();
    if (i == K - 1) break;
    float c[CSM];
#pragma unroll
    for (int j = 0; j < CSM; ++j) c[j] = cw[j];
    float best = -1.0f;
    int bn = 0;
    for (int n = tid; n < N; n += kSeedThreads) {
      float p[CSM];
#pragma unroll
      for (int j = 0; j < CSM; ++j) p[j] = j < Cs ? P[(size_t)n * Cs + j] : 0.0f;
      float d = pq_dist<CSM>(p, c);
      if (i > 0) {
        const float o = D[n];
        d = d < o ? d : o;
      }
      D[n] = d;
      if (d > best) { best = d; bn = n; }          // ascending n per lane: the first maximum stays
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const float ob = __shfl_xor(best, off);
      const int on = __shfl_xor(bn, off);
      if (ob > best || (ob == best && on < bn)) { best = ob; bn = on; }
    }
    if (lane == 0) { wBest[wave] = best; wIdx[wave] = bn; }
    __syncthreads();
    if (tid == 0) {
      float b = wBest[0];
      int bi = wIdx[0];
      for (int w = 1; w < kSeedThreads / 64; ++w)
        if (wBest[w] > b || (wBest[w] == b && wIdx[w] < bi)) { b = wBest[w]; bi = wIdx[w]; }
      pick = bi;
    }
    __syncthreads();
    cur = pick;
  }
}

// Nearest code word of points [blockIdx.y * 128, +128) of sub-space blockIdx.x.  The code book sits in LDS with CSM
// slots per code word (dims >= CsEff zero, see k_pq_seed): every lane reads the same code word, an LDS broadcast.
// first = 0: a point whose code word changed flags its sub-space in chg[m] (an integer store of 1, never a sum).
template <int CSM>
__global__ __launch_bounds__(kAssignThreads) void k_pq_assign(const float* __restrict__ pts, const float* __restrict__ ctrd,
                                                              uint8_t* __restrict__ asmt, float* __restrict__ dmin,
                                                              int* __restrict__ chg, const int* __restrict__ active, int N, int K,
                                                              int Cs, int Cin, int first) {
  __shared__ float cb[QCNN_PQ_MAX_K * CSM];
  const int m = blockIdx.x;
  if (active && !active[m]) return;
  const int cse = cs_eff(Cin, Cs, m);
  const float* C = ctrd + (size_t)m * K * Cs;
  for (int i = threadIdx.x; i < K * CSM; i += kAssignThreads) {
    const int k = i / CSM, j = i % CSM;
    cb[i] = j < cse ? C[(size_t)k * Cs + j] : 0.0f;
  }
  __syncthreads();
  const int n = blockIdx.y * kAssignThreads + threadIdx.x;
  if (n >= N) return;
  const size_t pn = (size_t)m * N + n;
  float p[CSM];
#pragma unroll
  for (int j = 0; j < CSM; ++j) p[j] = j < Cs ? pts[pn * Cs + j] : 0.0f;
  float best = pq_dist<CSM>(p, cb);
  int bk = 0;
  for (int k = 1; k < K; ++k) {
    const float d = pq_dist<CSM>(p, cb + k * CSM);
    if (d < best) { best = d; bk = k; }
  }
  if (!first && asmt[pn] != (uint8_t)bk) chg[m] = 1;
  asmt[pn] = (uint8_t)bk;
  dmin[pn] = best;
}

// Code book of sub-space blockIdx.x from its assignments: lane k owns code word k and walks the points in ascending n
// (staged through LDS in chunks, four assignments per LDS read), summing its members' coordinates in fp64 in that order.
template <int CSM>
__global__ __launch_bounds__(256) void k_pq_update(const float* __restrict__ pts, float* __restrict__ ctrd,
                                                   const uint8_t* __restrict__ asmt, const int* __restrict__ active, int N, int K,
                                                   int Cs, int Cin) {
  __shared__ uint32_t sa[kUpdateChunk / 4];
  const int m = blockIdx.x;
  if (active && !active[m]) return;
  const int cse = cs_eff(Cin, Cs, m);
  const int k = threadIdx.x;
  const uint8_t* A = asmt + (size_t)m * N;
  const float* P = pts + (size_t)m * N * Cs;
  double s[CSM];
#pragma unroll
  for (int j = 0; j < CSM; ++j) s[j] = 0.0;
  int cnt = 0;
  for (int n0 = 0; n0 < N; n0 += kUpdateChunk) {
    const int len = min(kUpdateChunk, N - n0);
    __syncthreads();
    uint8_t* sb = reinterpret_cast<uint8_t*>(sa);
    for (int i = threadIdx.x; i < len; i += blockDim.x) sb[i] = A[n0 + i];
    __syncthreads();
    if (k >= K) continue;
    const int words = len >> 2;
    for (int wi = 0; wi < words; ++wi) {
      const uint32_t w = sa[wi];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        if ((int)((w >> (8 * b)) & 0xffu) == k) {
          const float* q = P + (size_t)(n0 + wi * 4 + b) * Cs;
          ++cnt;
#pragma unroll
          for (int j = 0; j < CSM; ++j)
            if (j < cse) s[j] += (double)q[j];
        }
      }
    }
    for (int i = words * 4; i < len; ++i) {
      if ((int)sb[i] == k) {
        const float* q = P + (size_t)(n0 + i) * Cs;
        ++cnt;
#pragma unroll
        for (int j = 0; j < CSM; ++j)
          if (j < cse) s[j] += (double)q[j];
      }
    }
  }
  if (k >= K || cnt == 0) return;
  float* c = ctrd + ((size_t)m * K + k) * Cs;
#pragma unroll
  for (int j = 0; j < CSM; ++j)
    if (j < cse) c[j] = (float)(s[j] / (double)cnt);
}

// Zero the code book's dims >= CsEff (only the last sub-space can have any) and sum the minimum distances in fp64:
// one partial per workgroup, added up by the host in workgroup order.
__global__ __launch_bounds__(kFinalThreads) void k_pq_finalize(const float* __restrict__ dmin, size_t total, float* __restrict__ ctrd,
                                                               int M, int K, int Cs, int Cin, double* __restrict__ partial) {
  __shared__ double ws[kFinalThreads / 64];
  const int tid = threadIdx.x;
  const int cse = cs_eff(Cin, Cs, M - 1);
  if (blockIdx.x == 0 && cse < Cs) {
    float* C = ctrd + (size_t)(M - 1) * K * Cs;
    for (int i = tid; i < K * Cs; i += kFinalThreads)
      if (i % Cs >= cse) C[i] = 0.0f;
  }
  double s = 0.0;
  for (size_t i = (size_t)blockIdx.x * kFinalThreads + tid; i < total; i += (size_t)gridDim.x * kFinalThreads) s += (double)dmin[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
  if ((tid & 63) == 0) ws[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int w = 0; w < kFinalThreads / 64; ++w) t += ws[w];
    partial[blockIdx.x] = t;
  }
}

int csm_of(int Cs) { return Cs <= 1 ? 1 : Cs <= 2 ? 2 : Cs <= 4 ? 4 : Cs <= 8 ? 8 : 16; }

#define QK_PQ_DISPATCH(CS, LAUNCH) \
  switch (csm_of(CS)) {            \
    case 1: LAUNCH(1); break;      \
    case 2: LAUNCH(2); break;      \
    case 4: LAUNCH(4); break;      \
    case 8: LAUNCH(8); break;      \
    default: LAUNCH(16); break;    \
  }

}  // namespace

hipError_t qk_pq_gather(const float* w, float* pts, int N, int Cin, int taps, int M, int Cs, hipStream_t st) {
  const int blocks = (int)std::min<long long>(((long long)M * N + 255) / 256, 8192);
  hipLaunchKernelGGL(k_pq_gather, dim3(blocks), dim3(256), 0, st, w, pts, N, Cin, taps, M, Cs);
  return hipGetLastError();
}

hipError_t qk_pq_seed(const float* pts, float* ctrd, float* dmin, int M, int N, int K, int Cs, hipStream_t st) {
#define L_(C) hipLaunchKernelGGL(k_pq_seed<C>, dim3(M), dim3(kSeedThreads), 0, st, pts, ctrd, dmin, N, K, Cs)
  QK_PQ_DISPATCH(Cs, L_)
#undef L_
  return hipGetLastError();
}

hipError_t qk_pq_assign(const float* pts, const float* ctrd, uint8_t* asmt, float* dmin, int* chg, const int* active, int M, int N,
                        int K, int Cs, int Cin, int first, hipStream_t st) {
  const dim3 grid(M, (N + kAssignThreads - 1) / kAssignThreads);   // (N / 128 < 65536: checked by the caller)
#define L_(C) hipLaunchKernelGGL(k_pq_assign<C>, grid, dim3(kAssignThreads), 0, st, pts, ctrd, asmt, dmin, chg, active, N, K, Cs, Cin, first)
  QK_PQ_DISPATCH(Cs, L_)
#undef L_
  return hipGetLastError();
}

hipError_t qk_pq_update(const float* pts, float* ctrd, const uint8_t* asmt, const int* active, int M, int N, int K, int Cs, int Cin,
                        hipStream_t st) {
  const int threads = (K + 63) / 64 * 64;
#define L_(C) hipLaunchKernelGGL(k_pq_update<C>, dim3(M), dim3(threads), 0, st, pts, ctrd, asmt, active, N, K, Cs, Cin)
  QK_PQ_DISPATCH(Cs, L_)
#undef L_
  return hipGetLastError();
}

int qk_pq_finalize_blocks(size_t total) { return (int)std::min<size_t>((total + kFinalThreads - 1) / kFinalThreads, 1024); }

hipError_t qk_pq_finalize(const float* dmin, size_t total, float* ctrd, int M, int K, int Cs, int Cin, double* partial, hipStream_t st) {
  hipLaunchKernelGGL(k_pq_finalize, dim3(qk_pq_finalize_blocks(total)), dim3(kFinalThreads), 0, st, dmin, total, ctrd, M, K, Cs, Cin,
                     partial);
  return hipGetLastError();
}
