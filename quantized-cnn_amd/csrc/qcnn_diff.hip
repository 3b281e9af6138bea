// qcnn_diff.hip — two feature maps compared where they lie (behind qcnn_map_diff; the contract is include/qcnn_hip.h's): per
// channel the counted pairs, the non-finite ones, sum d, sum d^2, sum b^2 and max |d| of d = (double)a - (double)b over the first n
// images of two maps of panels [HW * C][128].  HBM-streaming glue in the style of qcnn_glue.hip: every load is a full 512-byte
// row (32 lanes x float4), the arithmetic is fp64 and far under the loads.  Two passes, no atomics, an order of summation that
// depends on (HW, C, n) alone:
//   k_diff_partial  one workgroup per (channel, chunk of QCNN_DIFF_CHUNK_ROWS rows): a partial row of six doubles
//   k_diff_fold     one wave per channel: its partial rows in a fixed order -> the channel's row
#include "qcnn_kernels.h"

#include "../../include/qcnn_hip.h"

#include <limits.h>

typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PANEL = QCNN_PANEL;                  // images per panel
constexpr int CHUNK = QCNN_DIFF_CHUNK_ROWS;        // rows of one channel per workgroup
constexpr int DIFF_THREADS = 256;                  // 8 rows of 32 float4 lanes per step
constexpr int STEP_ROWS = DIFF_THREADS / 32;
constexpr int FIELDS = 6;                          // doubles of a QcnnMapDiff
static_assert(CHUNK % STEP_ROWS == 0, "a chunk is a whole number of steps");
static_assert(sizeof(QcnnMapDiff) == FIELDS * sizeof(double), "a row of the scratch is a QcnnMapDiff");

inline int panels_of(int n) { return (n + PANEL - 1) / PANEL; }
inline long long chunks_of(int HW, int n) { return ((long long)panels_of(n) * HW + CHUNK - 1) / CHUNK; }

struct Acc {
  unsigned cnt = 0, nf = 0;
  double sd = 0.0, sd2 = 0.0, sr2 = 0.0, mx = 0.0;
};

__device__ inline bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// one pair; live: the image of this slot is one of the first n
__device__ inline void add_pair(Acc& s, float a, float b, bool live) {
  if (!live) return;
  if (!(finite_bits(a) && finite_bits(b))) { s.nf++; return; }
  const double da = (double)a, db = (double)b;
  const double d = da - db;                        // one fp64 operation on the exact values: no rounding at all while the two
  const double ad = d < 0.0 ? -d : d;              // exponents are within 29 of each other (24 + 29 = 53 bits), denormals included
  s.cnt++;
  s.sd += d;
  s.sd2 += d * d;
  s.sr2 += db * db;
  s.mx = ad > s.mx ? ad : s.mx;
}

__device__ inline void add_row(Acc& s, const float* a, const float* b, size_t off, int live) {
  const f32x4 va = *reinterpret_cast<const f32x4*>(a + off);
  const f32x4 vb = *reinterpret_cast<const f32x4*>(b + off);
  add_pair(s, va.x, vb.x, live > 0);
  add_pair(s, va.y, vb.y, live > 1);
  add_pair(s, va.z, vb.z, live > 2);
  add_pair(s, va.w, vb.w, live > 3);
}

// halving tree over the threads of a workgroup (T a power of two); thread 0 ends with the sum
template <int T>
__device__ inline void tree_fold(double (*sh)[T], int tid) {
  for (int s = T / 2; s > 0; s >>= 1) {
    __syncthreads();
    if (tid < s) {
      for (int f = 0; f < FIELDS - 1; ++f) sh[f][tid] += sh[f][tid + s];
      const double m = sh[FIELDS - 1][tid + s];
      if (m > sh[FIELDS - 1][tid]) sh[FIELDS - 1][tid] = m;
    }
  }
}

// Row r of channel c is (panel r / HW, pixel r % HW): the floats at ((panel * HW + pixel) * C + c) * 128.  a and b may alias.
__global__ void __launch_bounds__(DIFF_THREADS)
k_diff_partial(const float* a, const float* b, int HW, int C, int n, long long rows, long long chunks, double* __restrict__ part) {
  __shared__ double sh[FIELDS][DIFF_THREADS];
  const int tid = threadIdx.x, lane = tid & 31, rs = tid >> 5;
  const int c = (int)(blockIdx.x % (unsigned)C);
  const long long chunk = blockIdx.x / (unsigned)C;
  const long long r0 = chunk * CHUNK + rs;
  Acc s;
  auto row = [&](long long r) {                    // r < rows <= INT_MAX (qk_map_diff_doubles): 32-bit division
    const unsigned panel = (unsigned)r / (unsigned)HW;
    const int left = n - (int)panel * PANEL - 4 * lane;                   // images of this float4 among the first n
    const int live = left > 4 ? 4 : (left < 0 ? 0 : left);
    add_row(s, a, b, ((size_t)r * C + c) * PANEL + 4 * lane, live);
  };
  if ((chunk + 1) * CHUNK <= rows) {               // a whole chunk: the loads of all its steps may be in flight together
#pragma unroll
    for (int k = 0; k < CHUNK / STEP_ROWS; ++k) row(r0 + (long long)k * STEP_ROWS);
  } else {                                         // the last, ragged one: same rows per thread in the same order
    for (int k = 0; k < CHUNK / STEP_ROWS; ++k) {
      const long long r = r0 + (long long)k * STEP_ROWS;
      if (r < rows) row(r);
    }
  }
  sh[0][tid] = (double)s.cnt; sh[1][tid] = (double)s.nf; sh[2][tid] = s.sd;
  sh[3][tid] = s.sd2; sh[4][tid] = s.sr2; sh[5][tid] = s.mx;
  tree_fold<DIFF_THREADS>(sh, tid);
  if (tid == 0) {
    double* p = part + ((size_t)c * chunks + chunk) * FIELDS;
    for (int f = 0; f < FIELDS; ++f) p[f] = sh[f][0];
  }
}

// channel c = blockIdx.x: lane j adds its partial rows j, j + 64, ... in ascending order, then the halving tree
__global__ void __launch_bounds__(64)
k_diff_fold(const double* __restrict__ part, long long chunks, double* __restrict__ rows) {
  __shared__ double sh[FIELDS][64];
  const int tid = threadIdx.x;
  const double* p = part + (size_t)blockIdx.x * chunks * FIELDS;
  double v[FIELDS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (long long k = tid; k < chunks; k += 64) {
    for (int f = 0; f < FIELDS - 1; ++f) v[f] += p[k * FIELDS + f];
    const double m = p[k * FIELDS + FIELDS - 1];
    v[FIELDS - 1] = m > v[FIELDS - 1] ? m : v[FIELDS - 1];
  }
  for (int f = 0; f < FIELDS; ++f) sh[f][tid] = v[f];
  tree_fold<64>(sh, tid);
  if (tid == 0)
    for (int f = 0; f < FIELDS; ++f) rows[(size_t)blockIdx.x * FIELDS + f] = sh[f][0];
}

}  // namespace

size_t qk_map_diff_doubles(int HW, int C, int n) {
  if (HW <= 0 || C <= 0 || n <= 0) return 0;
  const long long chunks = chunks_of(HW, n);
  if ((long long)panels_of(n) * HW > INT_MAX || chunks * C > INT_MAX) return 0;
  return ((size_t)C + (size_t)C * chunks) * FIELDS;
}

hipError_t qk_map_diff(const float* a, const float* b, int HW, int C, int n, double* scratch, hipStream_t st) {
  if (!a || !b || !scratch || qk_map_diff_doubles(HW, C, n) == 0) return hipErrorInvalidValue;
  const long long rows = (long long)panels_of(n) * HW, chunks = chunks_of(HW, n);
  double* part = scratch + (size_t)C * FIELDS;
  hipLaunchKernelGGL(k_diff_partial, dim3((unsigned)(chunks * C)), dim3(DIFF_THREADS), 0, st, a, b, HW, C, n, rows, chunks, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_diff_fold, dim3(C), dim3(64), 0, st, part, chunks, scratch);
  return hipGetLastError();
}
