// qcnn_ec.hip — error-corrected quantisation (Wu et al., CVPR'16, sections 3.2 - 3.3): code books and assignments chosen so
// that the error of the layer's RESPONSE on calibration inputs is smallest, not the error of the weights
// (qcnn_calib_gram, qcnn_quantize_layer_ec in include/qcnn_hip.h; DESIGN.md "Error-corrected quantisation").
//
// Patch index p = (y * kw + x) * Cg + c.  J = sum_ct e_ct^T G_g e_ct with E = W - W_hat [Ct][P] in patch order and
// G_g = sum over calibration patches of s s^T; Hm = E G.  Kernels (stable names for rocprofv3 --kernel-trace --stats):
//   k_ec_gram         G_g as a symmetric rank-update, im2col implicit in the loads, v_mfma_f32_16x16x4_f32; fp32 over runs of
//                     kGramRun patches, fp64 across runs; upper-triangle tiles only, one fp64 slab per row split
//   k_ec_gram_panel   the same sums from a layer's input where a forward left it, panels [E][128] (qcnn_calib_begin): a column is
//                     fetched as its 512-byte panel row, 16 bytes a lane, dead lanes zeroed; fp32 over two (panel, pixel) units
//   k_ec_gram_reduce  slabs added in ascending split order (+ the caller's matrix when accumulating), mirrored
//   k_ec_identity     G = I when the caller gives no matrix
//   k_ec_residual     E from the fp32 weights, book and assignments           k_ec_eg         Hm = E G (fp64, LDS tiles)
//   k_ec_objective    fp64 partial sums of E o Hm per workgroup (added by the host in order)
//   k_ec_assign       one workgroup per output channel, thread k prices code word k for block (tap, m); the winner is
//                     taken only if it lowers J; E and the channel's row of Hm follow before the next tap
//   k_ec_members      per code word of a sub-space the blocks that name it, ascending (channel, tap)
//   k_ec_solve        A_k, v_k in fp64 in member order, Cholesky, c_k += delta rounded to fp32 once
//   k_ec_apply_words  E / Hm of the channels that name the moved code words
// No float atomics anywhere: every sum has a fixed order, results are the same bits from run to run.
#include <algorithm>

#include "qcnn_kernels.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kGramTile = 64;                    // G tile per workgroup: 4 waves x (2 x 2) MFMA tiles of 16 x 16
constexpr int kGramChunk = 16;                   // patches staged in LDS per step
constexpr int kGramRun = QCNN_EC_GRAM_RUN;       // patches summed in fp32 before the sums move to fp64
constexpr int kGramLd = kGramTile + 16;          // LDS row stride: the four k rows of an MFMA operand read fall on disjoint banks
static_assert(kGramRun % kGramChunk == 0, "a run is whole chunks");

__device__ inline int cs_eff(int Cin, int Cs, int m) { return min(Cin - m * Cs, Cs); }

// one column (patch index p) of the implicit patch matrix
struct GramCol {
  int y, x, off;        // tap row / column, channel offset g * Cg + c
  bool ok;
};

__device__ inline GramCol gram_col(int p, int g, const QkGramGeom& s) {
  GramCol c;
  c.ok = p < s.P;
  const int tap = c.ok ? p / s.Cg : 0;
  c.y = tap / s.kw;
  c.x = tap - c.y * s.kw;
  c.off = g * s.Cg + (c.ok ? p - tap * s.Cg : 0);
  return c;
}

__device__ inline float gram_load(const float* __restrict__ in, const QkGramGeom& s, const GramCol& c, int img, int oy, int ox,
                                  bool rowOk) {
  const int iy = oy * s.stride - s.pad + c.y, ix = ox * s.stride - s.pad + c.x;
  if (!rowOk || !c.ok || iy < 0 || iy >= s.H || ix < 0 || ix >= s.W) return 0.0f;      // out-of-image taps are zeros
  return in[(((size_t)img * s.H + iy) * s.W + ix) * s.C + c.off];
}

// blockIdx.x = upper-triangle tile pair, .y = group, .z = row split.  slab [split][grp][P][P], tiles ti <= tj only.
__global__ __launch_bounds__(256) void k_ec_gram(const float* __restrict__ in, QkGramGeom s, int nt, long long rowsPerSplit,
                                                 double* __restrict__ slab) {
  __shared__ float As[kGramChunk * kGramLd];
  __shared__ float Bs[kGramChunk * kGramLd];
  int ti = 0, rem = blockIdx.x;
  while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const int g = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int col = tid & 63, r0 = tid >> 6;
  const GramCol ca = gram_col(ti * kGramTile + col, g, s), cb = gram_col(tj * kGramTile + col, g, s);
  const long long rowBeg = (long long)blockIdx.z * rowsPerSplit;
  const long long rowEnd = rowBeg + rowsPerSplit < s.rows ? rowBeg + rowsPerSplit : s.rows;
  const int hw = s.Ho * s.Wo;
  const float* __restrict__ Bp = diag ? As : Bs;
  const int li = lane & 15, lk = lane >> 4;
  f32x4 acc[2][2];
  double dacc[2][2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      acc[a][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < 4; ++r) dacc[a][b][r] = 0.0;
    }
  int inRun = 0;
  for (long long row0 = rowBeg; row0 < rowEnd; row0 += kGramChunk) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kGramChunk / 4; ++i) {
      const int r = r0 + 4 * i;
      const long long R = row0 + r;
      const bool rowOk = R < rowEnd;
      const long long Rc = rowOk ? R : 0;
      const int img = (int)(Rc / hw), pix = (int)(Rc - (long long)img * hw);
      const int oy = pix / s.Wo, ox = pix - oy * s.Wo;
      As[r * kGramLd + col] = gram_load(in, s, ca, img, oy, ox, rowOk);
      if (!diag) Bs[r * kGramLd + col] = gram_load(in, s, cb, img, oy, ox, rowOk);
    }
    __syncthreads();
#pragma unroll
    for (int k0 = 0; k0 < kGramChunk; k0 += 4) {
      float a[2], b[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        a[h] = As[(k0 + lk) * kGramLd + wr * 32 + h * 16 + li];
        b[h] = Bp[(k0 + lk) * kGramLd + wc * 32 + h * 16 + li];
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[x], b[y], acc[x][y], 0, 0, 0);
    }
    inRun += kGramChunk;
    if (inRun == kGramRun || row0 + kGramChunk >= rowEnd) {
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
#pragma unroll
          for (int r = 0; r < 4; ++r) dacc[x][y][r] += (double)acc[x][y][r];
          acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
      inRun = 0;
    }
  }
  // D[(lane >> 4) * 4 + r][lane & 15]
  double* __restrict__ out = slab + ((size_t)blockIdx.z * gridDim.y + g) * s.P * s.P;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = ti * kGramTile + wr * 32 + x * 16 + lk * 4 + r, q = tj * kGramTile + wc * 32 + y * 16 + li;
        if (p < s.P && q < s.P) out[(size_t)p * s.P + q] = dacc[x][y][r];
      }
}

// G[g][p][q] = (accumulate ? G[g][p][q] : 0) + slab[0][g][a][b] + slab[1][g][a][b] + ..., a = min(p, q), b = max(p, q): both
// halves of the matrix read the same slab entries, so the result is symmetric to the bit.
__global__ __launch_bounds__(256) void k_ec_gram_reduce(const double* __restrict__ slab, double* __restrict__ G, int P, int grp,
                                                        int splits, int accumulate) {
  const size_t pp = (size_t)P * P, total = pp * grp;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t g = i / pp, e = i - g * pp;
    const int p = (int)(e / P), q = (int)(e - (size_t)p * P);
    const size_t src = g * pp + (size_t)min(p, q) * P + max(p, q);
    double sum = accumulate ? G[i] : 0.0;
    for (int z = 0; z < splits; ++z) sum += slab[(size_t)z * total + src];
    G[i] = sum;
  }
}

// ---- the same sums from a layer's input where a forward left it: image-minor panels [E][128] (resident calibration) ----
// The summed axis is (image, output pixel) and the 128 images of one element are 512 contiguous bytes, so the k axis of the MFMA
// is the contiguous one.  One UNIT = the 128 patch rows of one (panel, output pixel); a column of a unit is one panel row (an
// element of the map, or zeros for an out-of-map tap).  Two units = one fp32 run of kGramRun rows.
constexpr int kPanelCols = 8;                    // columns a thread fetches per operand and unit: 256 threads x 16 bytes = 8 rows a pass
static_assert(kGramRun == 2 * QCNN_PANEL, "an fp32 run is two (panel, output pixel) units");
static_assert(kGramTile * QCNN_PANEL * sizeof(float) * 2 == 65536, "both operands of a unit fill the static LDS limit exactly");

// Column of tile row `col` in LDS: 128 floats, image k at k ^ swz(col).  A row is 512 bytes = every bank once, so the MFMA
// operand read (16 columns x 4 consecutive k per instruction) would hit four banks sixteen times over; the XOR moves column
// col's group of four k to bank group (k / 4) ^ (col % 16): sixteen columns x four k on 64 distinct banks, and a thread's four
// consecutive images stay one aligned 16-byte store.
__device__ inline int panel_swz(int col) { return (col & 15) << 2; }

struct PanelCols {                               // per thread: its kPanelCols columns of one operand
  int yx[kPanelCols];                            // tap row << 16 | tap column
  int off[kPanelCols];                           // channel offset g * Cg + c (FC: the element itself); -1: past P
};

__device__ inline void panel_cols(PanelCols& pc, int tile, int g, const QkGramGeom& s, const int* __restrict__ dmap, int cs) {
#pragma unroll
  for (int i = 0; i < kPanelCols; ++i) {
    const GramCol c = gram_col(tile * kGramTile + i * 8 + cs, g, s);
    pc.yx[i] = (c.y << 16) | c.x;
    pc.off[i] = !c.ok ? -1 : dmap ? dmap[c.off] : c.off;         // dmap: only with a 1 x 1 window on a map taken as 1 x 1 x D
  }
}

// the thread's 16 bytes (images 4 * seg ..) of its columns of unit (panel, oy, ox); lanes of images >= live are zeroed HERE:
// maps behind the first layer hold bias-derived values in a ragged panel's dead lanes
__device__ inline void panel_fetch(f32x4 (&v)[kPanelCols], const PanelCols& pc, const float* __restrict__ fm, const QkGramGeom& s,
                                   size_t panelBase, int oy, int ox, int seg, int live) {
  const int y0 = oy * s.stride - s.pad, x0 = ox * s.stride - s.pad;
#pragma unroll
  for (int i = 0; i < kPanelCols; ++i) {
    const int iy = y0 + (pc.yx[i] >> 16), ix = x0 + (pc.yx[i] & 0xffff);
    f32x4 t = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (pc.off[i] >= 0 && iy >= 0 && iy < s.H && ix >= 0 && ix < s.W && 4 * seg < live)
      t = *reinterpret_cast<const f32x4*>(fm + (panelBase + ((size_t)iy * s.W + ix) * s.C + pc.off[i]) * QCNN_PANEL + 4 * seg);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * seg + j >= live) t[j] = 0.0f;
    v[i] = t;
  }
}

__device__ inline void panel_stage(float* __restrict__ S, const f32x4 (&v)[kPanelCols], int cs, int seg) {
#pragma unroll
  for (int i = 0; i < kPanelCols; ++i) {
    const int col = i * 8 + cs;
    *reinterpret_cast<f32x4*>(S + col * QCNN_PANEL + ((4 * seg) ^ panel_swz(col))) = v[i];
  }
}

// blockIdx.x = upper-triangle tile pair, .y = group, .z = row split (unitsPerSplit units each).  fm: the first of `panels`
// panels [E][128] that hold nLive images; dmap: the first FC layer's flatten map (column d is element dmap[d]) or nullptr.
// direct != 0 (one split): out = the resident matrix [grp][P][P], the tile is added to its upper entries and mirrored;
// otherwise out = slab [split][grp][P][P] as k_ec_gram writes it (k_ec_gram_reduce adds the slabs in ascending order).
__global__ __launch_bounds__(256) void k_ec_gram_panel(const float* __restrict__ fm, const int* __restrict__ dmap, QkGramGeom s, int nt,
                                                       int panels, int nLive, int unitsPerSplit, double* __restrict__ out, int direct) {
  __shared__ __attribute__((aligned(16))) float As[kGramTile * QCNN_PANEL];
  __shared__ __attribute__((aligned(16))) float Bs[kGramTile * QCNN_PANEL];
  int ti = 0, rem = blockIdx.x;
  while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
  const int tj = ti + rem;
  const bool diag = ti == tj;
  const int g = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  const int seg = tid & 31, cs = tid >> 5;                 // 32 threads x 16 bytes = one 512-byte row; eight rows a pass
  const int li = lane & 15, lk = lane >> 4;
  const int hw = s.Ho * s.Wo;
  const size_t E = (size_t)s.H * s.W * s.C;
  const long long units = (long long)panels * hw;
  const long long uBeg = (long long)blockIdx.z * unitsPerSplit;
  const long long uEnd = uBeg + unitsPerSplit < units ? uBeg + unitsPerSplit : units;
  const float* __restrict__ Bp = diag ? As : Bs;
  PanelCols pa, pb;
  panel_cols(pa, ti, g, s, dmap, cs);
  if (!diag) panel_cols(pb, tj, g, s, dmap, cs);
  f32x4 acc[2][2];
  double dacc[2][2][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      acc[a][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int r = 0; r < 4; ++r) dacc[a][b][r] = 0.0;
    }
  f32x4 va[kPanelCols], vb[kPanelCols];
  auto fetch = [&](long long u) {
    const int panel = (int)(u / hw), pix = (int)(u - (long long)panel * hw);
    const int oy = pix / s.Wo, ox = pix - oy * s.Wo;
    const int live = min(nLive - panel * QCNN_PANEL, QCNN_PANEL);
    panel_fetch(va, pa, fm, s, (size_t)panel * E, oy, ox, seg, live);
    if (!diag) panel_fetch(vb, pb, fm, s, (size_t)panel * E, oy, ox, seg, live);
  };
  if (uBeg < uEnd) fetch(uBeg);
  int inRun = 0;
  for (long long u = uBeg; u < uEnd; ++u) {
    __syncthreads();                                       // the previous unit's operand reads have passed
    panel_stage(As, va, cs, seg);
    if (!diag) panel_stage(Bs, vb, cs, seg);
    __syncthreads();
    if (u + 1 < uEnd) fetch(u + 1);                        // the next unit's rows fly under this unit's MFMAs
    const int sw = li << 2;
#pragma unroll 8
    for (int k0 = 0; k0 < QCNN_PANEL; k0 += 4) {
      float a[2], b[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        a[h] = As[(wr * 32 + h * 16 + li) * QCNN_PANEL + ((k0 + lk) ^ sw)];
        b[h] = Bp[(wc * 32 + h * 16 + li) * QCNN_PANEL + ((k0 + lk) ^ sw)];
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[x], b[y], acc[x][y], 0, 0, 0);
    }
    if (++inRun == kGramRun / QCNN_PANEL || u + 1 == uEnd) {
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) {
#pragma unroll
          for (int r = 0; r < 4; ++r) dacc[x][y][r] += (double)acc[x][y][r];
          acc[x][y] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
      inRun = 0;
    }
  }
  // D[(lane >> 4) * 4 + r][lane & 15]
  const size_t pp = (size_t)s.P * s.P;
  double* __restrict__ dst = out + (direct ? (size_t)g : (size_t)blockIdx.z * gridDim.y + g) * pp;
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = ti * kGramTile + wr * 32 + x * 16 + lk * 4 + r, q = tj * kGramTile + wc * 32 + y * 16 + li;
        if (p >= s.P || q >= s.P) continue;
        if (!direct) { dst[(size_t)p * s.P + q] = dacc[x][y][r]; continue; }
        if (p > q) continue;                               // a diagonal tile's lower half: its mirror image writes it
        const double sum = dst[(size_t)p * s.P + q] + dacc[x][y][r];
        dst[(size_t)p * s.P + q] = sum;
        if (p != q) dst[(size_t)q * s.P + p] = sum;
      }
}

__global__ __launch_bounds__(256) void k_ec_identity(double* __restrict__ G, int P, int grp) {
  const size_t pp = (size_t)P * P, total = pp * grp;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const size_t e = i % pp;
    G[i] = (e / P == e % P) ? 1.0 : 0.0;
  }
}

// E[ct][p] = W[ct][c][tap] - book word of block (tap, m = c / Cs); asmt on the device is [M][N], N = Ct * taps
__global__ __launch_bounds__(256) void k_ec_residual(const float* __restrict__ w, const float* __restrict__ ctrd,
                                                     const uint8_t* __restrict__ asmt, double* __restrict__ E, QkEcShape s) {
  const size_t total = (size_t)s.Ct * s.P;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ct = (int)(i / s.P), p = (int)(i - (size_t)ct * s.P);
    const int tap = p / s.Cin, c = p - tap * s.Cin;
    const int m = c / s.Cs, j = c - m * s.Cs;
    const int k = asmt[(size_t)m * s.N + (size_t)ct * s.taps + tap];
    E[i] = (double)w[((size_t)ct * s.Cin + c) * s.taps + tap] - (double)ctrd[((size_t)m * s.K + k) * s.Cs + j];
  }
}

// Hm = E G_g, fp64: 64 x 64 tile per workgroup (rows of one group), 4 x 4 per thread, 16-deep LDS stages
__global__ __launch_bounds__(256) void k_ec_eg(const double* __restrict__ E, const double* __restrict__ G, double* __restrict__ Hm,
                                               QkEcShape s, int rowTiles) {
  __shared__ double Es[16][64 + 1];
  __shared__ double Gs[16][64];
  const int g = blockIdx.y / rowTiles, rt = blockIdx.y - g * rowTiles;
  const int Ctg = s.Ct / s.grp;
  const int rBase = rt * 64, cBase = blockIdx.x * 64;
  const double* __restrict__ Gg = G + (size_t)g * s.P * s.P;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4] = {};
  for (int k0 = 0; k0 < s.P; k0 += 16) {
    __syncthreads();
    for (int i = tid; i < 16 * 64; i += 256) {
      const int kk = i & 15, r = i >> 4;                      // E: consecutive threads walk a row's k
      const int row = rBase + r;
      Es[kk][r] = (row < Ctg && k0 + kk < s.P) ? E[((size_t)g * Ctg + row) * s.P + k0 + kk] : 0.0;
      const int c = i & 63, k2 = i >> 6;                      // G: consecutive threads walk a row's columns
      Gs[k2][c] = (k0 + k2 < s.P && cBase + c < s.P) ? Gg[(size_t)(k0 + k2) * s.P + cBase + c] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) { a[i] = Es[kk][ty * 4 + i]; b[i] = Gs[kk][tx + 16 * i]; }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += a[i] * b[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = rBase + ty * 4 + i, c = cBase + tx + 16 * j;
      if (row < Ctg && c < s.P) Hm[((size_t)g * Ctg + row) * s.P + c] = acc[i][j];
    }
}

__global__ __launch_bounds__(256) void k_ec_objective(const double* __restrict__ E, const double* __restrict__ Hm, size_t total,
                                                      double* __restrict__ partial) {
  __shared__ double ws[4];
  const int tid = threadIdx.x;
  double sum = 0.0;
  for (size_t i = (size_t)blockIdx.x * 256 + tid; i < total; i += (size_t)gridDim.x * 256) sum += E[i] * Hm[i];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off);
  if ((tid & 63) == 0) ws[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) partial[blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// Assign step of block (tap t, sub-space m) for output channel blockIdx.x.  Thread k prices code word k:
// delta_k = d^T (G_bb d - 2 Hm[ct][b]), d = c_k - c_cur; the lowest k of the smallest delta wins if that delta is < 0.
__global__ __launch_bounds__(256) void k_ec_assign(const float* __restrict__ ctrd, uint8_t* __restrict__ asmt,
                                                   const double* __restrict__ G, double* __restrict__ E, double* __restrict__ Hm,
                                                   int* __restrict__ chg, QkEcShape s, int m, int t) {
  __shared__ double gbb[QCNN_PQ_MAX_CS * QCNN_PQ_MAX_CS];
  __shared__ double h[QCNN_PQ_MAX_CS], ccur[QCNN_PQ_MAX_CS], dsel[QCNN_PQ_MAX_CS];
  __shared__ double wBest[4];
  __shared__ int wIdx[4];
  __shared__ int pick;
  const int ct = blockIdx.x, tid = threadIdx.x;
  const int cse = cs_eff(s.Cin, s.Cs, m);
  const int base = t * s.Cin + m * s.Cs;
  const int g = ct / (s.Ct / s.grp);
  const double* __restrict__ Gg = G + (size_t)g * s.P * s.P;
  uint8_t* a = asmt + (size_t)m * s.N + (size_t)ct * s.taps + t;
  const int cur = *a;
  const float* __restrict__ C = ctrd + (size_t)m * s.K * s.Cs;
  if (tid < cse * cse) gbb[tid] = Gg[(size_t)(base + tid / cse) * s.P + base + tid % cse];
  if (tid < cse) {
    h[tid] = Hm[(size_t)ct * s.P + base + tid];
    ccur[tid] = (double)C[(size_t)cur * s.Cs + tid];
  }
  __syncthreads();
  double best = 0.0;
  int bk = cur;
  if (tid < s.K) {
    double d[QCNN_PQ_MAX_CS];
    for (int j = 0; j < cse; ++j) d[j] = (double)C[(size_t)tid * s.Cs + j] - ccur[j];
    double delta = 0.0;
    for (int i = 0; i < cse; ++i) {
      double u = -2.0 * h[i];
      for (int j = 0; j < cse; ++j) u += gbb[i * cse + j] * d[j];
      delta += d[i] * u;
    }
    if (delta < 0.0) { best = delta; bk = tid; }
  }
  int key = best < 0.0 ? bk : 0x7fffffff;                      // non-improving lanes lose every comparison
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ob = __shfl_xor(best, off);
    const int ok = __shfl_xor(key, off);
    if (ob < best || (ob == best && ok < key)) { best = ob; key = ok; }
  }
  if ((tid & 63) == 0) { wBest[tid >> 6] = best; wIdx[tid >> 6] = key; }
  __syncthreads();
  if (tid == 0) {
    double b = wBest[0];
    int bi = wIdx[0];
    for (int w = 1; w < 4; ++w)
      if (wBest[w] < b || (wBest[w] == b && wIdx[w] < bi)) { b = wBest[w]; bi = wIdx[w]; }
    pick = (b < 0.0 && bi != 0x7fffffff) ? bi : -1;
  }
  __syncthreads();
  const int nk = pick;
  if (nk < 0) return;
  if (tid < cse) dsel[tid] = (double)C[(size_t)nk * s.Cs + tid] - ccur[tid];
  __syncthreads();
  if (tid == 0) { *a = (uint8_t)nk; chg[ct] += 1; }
  if (tid < cse) E[(size_t)ct * s.P + base + tid] -= dsel[tid];
  double* __restrict__ hrow = Hm + (size_t)ct * s.P;
  for (int q = tid; q < s.P; q += 256) {
    double acc = 0.0;
    for (int j = 0; j < cse; ++j) acc += dsel[j] * Gg[(size_t)(base + j) * s.P + q];
    hrow[q] -= acc;
  }
}

// Members of every code word of sub-space m in ascending n = ct * taps + t: off[K + 1], list[N].  One workgroup, thread k.
__global__ __launch_bounds__(256) void k_ec_members(const uint8_t* __restrict__ asmt, int* __restrict__ off, int* __restrict__ list,
                                                    QkEcShape s, int m) {
  __shared__ int so[QCNN_PQ_MAX_K + 1];
  const int k = threadIdx.x;
  const uint8_t* __restrict__ A = asmt + (size_t)m * s.N;
  int cnt = 0;
  if (k < s.K)
    for (int n = 0; n < s.N; ++n) cnt += A[n] == k;
  so[k + 1] = k < s.K ? cnt : 0;
  __syncthreads();
  if (k == 0) {
    so[0] = 0;
    for (int i = 0; i < s.K; ++i) so[i + 1] += so[i];
  }
  __syncthreads();
  if (k <= s.K) off[k] = so[k];
  if (k == 0 && s.K == QCNN_PQ_MAX_K) off[s.K] = so[s.K];
  if (k < s.K) {
    int w = so[k];
    for (int n = 0; n < s.N; ++n)
      if (A[n] == k) list[w++] = n;
  }
}

// Code word k = k0 + blockIdx.x of sub-space m: A_k = sum over channels of sum_{b, b' in L_k(ct)} G_bb' + lambda I,
// v_k = sum of Hm[ct][b]; delta = A_k^-1 v_k by Cholesky; c_k = (float)(c_k + delta); dw[k] = the move as stored.  A code
// word without members, or whose A_k is not positive definite, keeps its value (dw = 0).
__global__ __launch_bounds__(256) void k_ec_solve(float* __restrict__ ctrd, const int* __restrict__ off, const int* __restrict__ list,
                                                  const double* __restrict__ G, const double* __restrict__ Hm, double* __restrict__ dw,
                                                  int* __restrict__ moved, QkEcShape s, int m, int k0, double lambda) {
  __shared__ double A[QCNN_PQ_MAX_CS][QCNN_PQ_MAX_CS + 1];
  __shared__ double v[QCNN_PQ_MAX_CS];
  __shared__ int okFlag;
  const int k = k0 + blockIdx.x, tid = threadIdx.x;
  const int cse = cs_eff(s.Cin, s.Cs, m);
  const int beg = off[k], end = off[k + 1];
  const int Ctg = s.Ct / s.grp;
  const size_t pp = (size_t)s.P * s.P;
  const int sub = m * s.Cs;
  if (tid < cse * cse) {
    const int i = tid / cse, j = tid - i * cse;
    double acc = 0.0;
    int a0 = beg;
    while (a0 < end) {
      const int ct = list[a0] / s.taps;
      int a1 = a0 + 1;
      while (a1 < end && list[a1] / s.taps == ct) ++a1;
      const double* __restrict__ Gg = G + (size_t)(ct / Ctg) * pp;
      for (int x = a0; x < a1; ++x) {
        const double* __restrict__ row = Gg + (size_t)((list[x] - ct * s.taps) * s.Cin + sub + i) * s.P + sub + j;
        for (int y = a0; y < a1; ++y) acc += row[(size_t)(list[y] - ct * s.taps) * s.Cin];
      }
      a0 = a1;
    }
    A[i][j] = acc + (i == j ? lambda : 0.0);
  }
  if (tid < cse) {
    double acc = 0.0;
    for (int x = beg; x < end; ++x) {
      const int ct = list[x] / s.taps, t = list[x] - ct * s.taps;
      acc += Hm[(size_t)ct * s.P + t * s.Cin + sub + tid];
    }
    v[tid] = acc;
  }
  __syncthreads();
  if (tid == 0) {
    bool ok = end > beg;
    for (int j = 0; ok && j < cse; ++j) {                      // A = L L^T in place (lower triangle)
      double d = A[j][j];
      for (int x = 0; x < j; ++x) d -= A[j][x] * A[j][x];
      if (!(d > 0.0)) { ok = false; break; }
      d = sqrt(d);
      A[j][j] = d;
      for (int i = j + 1; i < cse; ++i) {
        double e = A[i][j];
        for (int x = 0; x < j; ++x) e -= A[i][x] * A[j][x];
        A[i][j] = e / d;
      }
    }
    if (ok) {
      for (int i = 0; i < cse; ++i) {                          // L y = v
        double e = v[i];
        for (int x = 0; x < i; ++x) e -= A[i][x] * v[x];
        v[i] = e / A[i][i];
      }
      for (int i = cse - 1; i >= 0; --i) {                     // L^T delta = y
        double e = v[i];
        for (int x = i + 1; x < cse; ++x) e -= A[x][i] * v[x];
        v[i] = e / A[i][i];
      }
    }
    okFlag = ok;
  }
  __syncthreads();
  if (tid < s.Cs) {
    double d = 0.0;
    if (okFlag && tid < cse) {
      float* c = ctrd + ((size_t)m * s.K + k) * s.Cs + tid;
      const float old = *c;
      const float nw = (float)((double)old + v[tid]);
      d = (double)nw - (double)old;
      *c = nw;
      if (nw != old) *moved = 1;
    }
    dw[(size_t)k * s.Cs + tid] = d;
  }
}

// E / Hm of output channel blockIdx.y after the code words of sub-space m moved by dw: every block of the channel that names
// code word ksel (ksel < 0: any code word) moves by -dw.
__global__ __launch_bounds__(256) void k_ec_apply_words(const uint8_t* __restrict__ asmt, const double* __restrict__ dw,
                                                        const double* __restrict__ G, double* __restrict__ E, double* __restrict__ Hm,
                                                        QkEcShape s, int m, int ksel) {
  const int ct = blockIdx.y, tid = threadIdx.x;
  const int cse = cs_eff(s.Cin, s.Cs, m);
  const uint8_t* __restrict__ a = asmt + (size_t)m * s.N + (size_t)ct * s.taps;
  const double* __restrict__ Gg = G + (size_t)(ct / (s.Ct / s.grp)) * s.P * s.P;
  const int q = blockIdx.x * 256 + tid;
  const int sub = m * s.Cs;
  double acc = 0.0;
  bool any = false;
  for (int t = 0; t < s.taps; ++t) {
    const int k = a[t];
    if (ksel >= 0 && k != ksel) continue;
    any = true;
    if (q < s.P)
      for (int j = 0; j < cse; ++j) acc += dw[(size_t)k * s.Cs + j] * Gg[(size_t)(t * s.Cin + sub + j) * s.P + q];
  }
  if (!any) return;
  if (q < s.P) Hm[(size_t)ct * s.P + q] -= acc;
  if (blockIdx.x == 0)
    for (int i = tid; i < s.taps * cse; i += 256) {
      const int t = i / cse, j = i - t * cse;
      const int k = a[t];
      if (ksel < 0 || k == ksel) E[(size_t)ct * s.P + t * s.Cin + sub + j] -= dw[(size_t)k * s.Cs + j];
    }
}

int grid_for(size_t total, int cap) { return (int)std::max<size_t>(1, std::min<size_t>((total + 255) / 256, (size_t)cap)); }

}  // namespace

int qk_ec_gram_tiles(int P) { return (P + kGramTile - 1) / kGramTile; }

// rows of the patch matrix per split: whole runs, enough workgroups to fill the chip, slabs of at most maxSlabBytes in all
long long qk_ec_gram_rows_per_split(const QkGramGeom& s, size_t maxSlabBytes, int* splits) {
  const long long nt = qk_ec_gram_tiles(s.P), wgs = nt * (nt + 1) / 2 * s.grp;
  const long long runs = (s.rows + kGramRun - 1) / kGramRun;
  const size_t one = (size_t)s.grp * s.P * s.P * sizeof(double);
  long long want = std::max<long long>(1, 2048 / wgs);
  want = std::min<long long>(want, std::max<long long>(1, (long long)(maxSlabBytes / one)));
  want = std::max<long long>(1, std::min<long long>(std::min<long long>(want, runs), 65535));
  const long long per = (runs + want - 1) / want * kGramRun;
  *splits = (int)std::max<long long>(1, (s.rows + per - 1) / per);
  return per;
}

hipError_t qk_ec_gram(const float* in, const QkGramGeom& s, long long rowsPerSplit, int splits, double* slab, double* G, int accumulate,
                      hipStream_t st) {
  const int nt = qk_ec_gram_tiles(s.P);
  hipLaunchKernelGGL(k_ec_gram, dim3(nt * (nt + 1) / 2, s.grp, splits), dim3(256), 0, st, in, s, nt, rowsPerSplit, slab);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_ec_gram_reduce, dim3(grid_for((size_t)s.grp * s.P * s.P, 16384)), dim3(256), 0, st, slab, G, s.P, s.grp, splits,
                     accumulate);
  return hipGetLastError();
}

// k_ec_gram_panel's rows are cut in units of one (panel, output pixel) = 128 patch rows; a split is whole fp32 runs of two
// units.  As many splits as fill the chip (2048 workgroups) with the shape's tile pairs, at most one per run, slabs of at most
// maxSlabBytes in all: a function of the shape and the panel count alone.  *splits == 1: no slab, the tiles go straight into
// the resident matrix.
long long qk_ec_gram_panel_units_per_split(const QkGramGeom& s, int panels, size_t maxSlabBytes, int* splits) {
  const long long nt = qk_ec_gram_tiles(s.P), wgs = nt * (nt + 1) / 2 * s.grp;
  const long long units = (long long)panels * s.Ho * s.Wo;
  const long long runs = (units + 1) / 2;
  const size_t one = (size_t)s.grp * s.P * s.P * sizeof(double);
  long long want = std::max<long long>(1, 2048 / wgs);
  want = std::min<long long>(want, std::max<long long>(1, (long long)(maxSlabBytes / one)));
  want = std::max<long long>(1, std::min<long long>(std::min<long long>(want, runs), 65535));
  const long long per = (runs + want - 1) / want * 2;
  *splits = (int)std::max<long long>(1, (units + per - 1) / per);
  return per;
}

// G += the sums over the nLive images of `panels` panels at fm.  splits > 1: through slab (splits * grp * P * P doubles)
hipError_t qk_ec_gram_panel(const float* fm, const int* dmap, const QkGramGeom& s, int panels, int nLive, long long unitsPerSplit,
                            int splits, double* slab, double* G, hipStream_t st) {
  const int nt = qk_ec_gram_tiles(s.P);
  const int direct = splits == 1;
  hipLaunchKernelGGL(k_ec_gram_panel, dim3(nt * (nt + 1) / 2, s.grp, splits), dim3(256), 0, st, fm, dmap, s, nt, panels, nLive,
                     (int)unitsPerSplit, direct ? G : slab, direct);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || direct) return e;
  hipLaunchKernelGGL(k_ec_gram_reduce, dim3(grid_for((size_t)s.grp * s.P * s.P, 16384)), dim3(256), 0, st, slab, G, s.P, s.grp, splits, 1);
  return hipGetLastError();
}

hipError_t qk_ec_identity(double* G, int P, int grp, hipStream_t st) {
  hipLaunchKernelGGL(k_ec_identity, dim3(grid_for((size_t)grp * P * P, 16384)), dim3(256), 0, st, G, P, grp);
  return hipGetLastError();
}

int qk_ec_objective_blocks(const QkEcShape& s) { return grid_for((size_t)s.Ct * s.P, 1024); }

// E and Hm from scratch, and the fp64 partial sums of J (one per workgroup, added by the host in order)
hipError_t qk_ec_evaluate(const float* w, const float* ctrd, const uint8_t* asmt, const double* G, double* E, double* Hm, double* partial,
                          const QkEcShape& s, hipStream_t st) {
  const size_t total = (size_t)s.Ct * s.P;
  hipLaunchKernelGGL(k_ec_residual, dim3(grid_for(total, 16384)), dim3(256), 0, st, w, ctrd, asmt, E, s);
  const int rowTiles = (s.Ct / s.grp + 63) / 64;
  hipLaunchKernelGGL(k_ec_eg, dim3((s.P + 63) / 64, s.grp * rowTiles), dim3(256), 0, st, E, G, Hm, s, rowTiles);
  hipLaunchKernelGGL(k_ec_objective, dim3(qk_ec_objective_blocks(s)), dim3(256), 0, st, E, Hm, total, partial);
  return hipGetLastError();
}

hipError_t qk_ec_assign(const float* ctrd, uint8_t* asmt, const double* G, double* E, double* Hm, int* chg, const QkEcShape& s, int m, int t,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_ec_assign, dim3(s.Ct), dim3(256), 0, st, ctrd, asmt, G, E, Hm, chg, s, m, t);
  return hipGetLastError();
}

// Update step of sub-space m.  kh = kw = 1: no two code words share an output channel, all K are solved from one state;
// otherwise code word by code word in ascending k.
hipError_t qk_ec_update(float* ctrd, const uint8_t* asmt, int* off, int* list, const double* G, double* E, double* Hm, double* dw, int* moved,
                        const QkEcShape& s, int m, double lambda, hipStream_t st) {
  hipLaunchKernelGGL(k_ec_members, dim3(1), dim3(256), 0, st, asmt, off, list, s, m);
  const dim3 grid((s.P + 255) / 256, s.Ct);
  if (s.taps == 1) {
    hipLaunchKernelGGL(k_ec_solve, dim3(s.K), dim3(256), 0, st, ctrd, off, list, G, Hm, dw, moved, s, m, 0, lambda);
    hipLaunchKernelGGL(k_ec_apply_words, grid, dim3(256), 0, st, asmt, dw, G, E, Hm, s, m, -1);
  } else {
    for (int k = 0; k < s.K; ++k) {
      hipLaunchKernelGGL(k_ec_solve, dim3(1), dim3(256), 0, st, ctrd, off, list, G, Hm, dw, moved, s, m, k, lambda);
      hipLaunchKernelGGL(k_ec_apply_words, grid, dim3(256), 0, st, asmt, dw, G, E, Hm, s, m, k);
    }
  }
  return hipGetLastError();
}
