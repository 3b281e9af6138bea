// qcnn_decoded.hip — quantised conv layers with ONE sub-space of <= 4 dims (AlexNet conv1, VGG-16 conv1_1: the RGB input).
//
// For such a layer a table look-up replaces Cin <= 4 multiply-adds and the table of a source pixel (K code words x 128
// images, 64 KB of LDS stores) serves only knl^2 / stride^2 x Ct look-ups: in k_conv_aprx two thirds of a conv1 stage are
// the table build.  The same sum
//
//     dst[pos][c] = bias[c] + sum_taps  LUT[pixel(pos, tap)][asmt[tap][c]],     LUT[p][k] = sum_d x[p][d] * ctrd[d][k]
//                                                                   (src/CaffeEva.cc:816-865 over :1261-1296)
//
// is evaluated here WITHOUT materialising the tables: every assignment is replaced by the code word it names
// (k_decode_weights: w[tap][d][c] = ctrd[d][asmt[tap][c]], once per parameter upload) and the products go to the matrix
// pipe — v_mfma_f32_16x16x4_f32 with A = decoded code words [16 channels x 4 k], B = the panel rows themselves
// [4 k x 16 images]; k runs over the (column, input channel) pairs of ONE kernel row, which are consecutive panel rows,
// so there is no im2col buffer and no address table.  Same quantised parameters, same function; the sum is fused
// multiply-adds in (tap, d) order instead of d-sums rounded into a table first — within the north-star tolerance like
// every MFMA path (the exact builder, QCNN_LUT_EXACT, never takes this path).
//
// Kernels: k_conv_dec (below: persistent waves, all code words of the layer in LDS, wide buffer loads) and, for FC layers
// whose sub-spaces have ONE dim, k_fc_dec (further down).  Both are opt-out (QCNN_OPT_DECODE = 0: table kernels).
#include "qcnn_kernels.h"
#include <algorithm>
#include <type_traits>

typedef float f32x4 __attribute__((ext_vector_type(4)));

#ifndef QCNN_DEC_VAR
#define QCNN_DEC_VAR 0      // timing experiments only (scripts/build_variant.sh, scripts/variants_dec.sh): 1 no B loads, 2 no A reads, 8 no stores
#endif

namespace {

constexpr int PANEL = QCNN_PANEL;

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Product index of padded row k (< Kp) of a kernel row with Kr = knl * Cin real products: the steps (four k each) cover
// [0, 4), [4, 8), ... and the LAST one [Kr - 4, Kr) (Kr >= 4: it overlaps the step before it; an overlapped row carries a
// zero code word in the last step, reported as -1) — every operand row a step loads lies inside the window.  Kr < 4: the
// single step is [0, 4), rows >= Kr are padding (-1; the kernel clamps their loads: PADDED path).
__host__ __device__ __forceinline__ int qk_dec_krow(int k, int Kr, int Kp) {
  const int last = Kp - 4;                                  // first padded row of the last step
  if (k < last || Kr < 4) return k < Kr ? k : -1;
  const int real = Kr - 4 + (k - last);
  return real >= last ? real : -1;
}

// The code word the assignment of tap (kh, kw) names for output channel ch, input channel d of the sub-space.  rows:
// [kh][kw][M = 1][rowStride] slot bytes (QkSlots order); ctrd: [Cs][K]
__device__ __forceinline__ float code_word(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd, const QkSlots& sl, int knl,
                                           int K, int d, int kh, int kw, int ch) {
  const int slot = rows[(size_t)(kh * knl + kw) * sl.rowStride + qk_slot_entry(sl, 0, ch)];
  return ctrd[(size_t)d * K + qcnn_row_slot(slot)];             // qcnn_row_slot is its own inverse; M = 1: stage row = code word
}

// out: [knl][Kp][S]
__global__ void k_decode_weights(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd, float* __restrict__ out,
                                 QkSlots sl, int knl, int Cin, int K, int Ct, int Kp, int S) {
  const int total = knl * Kp * S;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ch = i % S, k = qk_dec_krow((i / S) % Kp, knl * Cin, Kp), kh = i / (S * Kp);
    out[i] = ch < Ct && k >= 0 ? code_word(rows, ctrd, sl, knl, K, k % Cin, kh, k / Cin, ch) : 0.0f;
  }
}

// n16 16-byte words from global memory into LDS, by the THREADS threads of the workgroup
template <int THREADS>
__device__ __forceinline__ void lds_fill(float* lds, const float* __restrict__ src, int n16) {
  const f32x4* __restrict__ src4 = reinterpret_cast<const f32x4*>(src);
  f32x4* lds4 = reinterpret_cast<f32x4*>(lds);
  for (int i = threadIdx.x; i < n16; i += THREADS) lds4[i] = src4[i];
}

// The items of wave `wave` of a persistent workgroup of WAVES: first, first + stride, ... below end.  Workgroups go to the
// eight XCDs round-robin (workgroup i -> XCD i % 8) and every XCD has its own L2: an XCD takes a CONTIGUOUS eighth of the
// item list (whole panels for a 1000-image batch), so that the windows its waves read overlap in ITS L2 instead of every L2
// fetching the whole input.  SPREAD: a launch of less than one item per wave (a few images) spreads its items over the SIMDs
// of ALL workgroups — wave w of workgroup g takes item w wgX + g — instead of filling the waves of a few: an item then has a
// matrix pipe to itself
struct ItemRange { int first, end, stride; };
template <int WAVES, bool SPREAD>
__device__ __forceinline__ ItemRange xcd_items(int nItems, int wave) {
  const int xcd = blockIdx.x & 7, nX = gridDim.x < 8 ? gridDim.x : 8;
  const int wgX = (gridDim.x - xcd + 7) >> 3;                           // workgroups of this XCD
  const int itemBeg = (int)((long long)nItems * xcd / nX), itemEnd = (int)((long long)nItems * (xcd + 1) / nX);
  const bool sparse = SPREAD && itemEnd - itemBeg <= wgX * WAVES;
  return {itemBeg + (sparse ? wave * wgX + (int)(blockIdx.x >> 3) : (int)(blockIdx.x >> 3) * WAVES + wave), itemEnd, wgX * WAVES};
}

// Persistent waves: a workgroup loads ALL decoded code words into LDS once ([knl * Kp][S], <= 152 KB), then every wave
// walks its own list of work items without any workgroup synchronisation: the waves of a SIMD drift apart, so one wave's
// operand loads and result stores sit under the other waves' matrix instructions.
//
// A work item = (panel, PW consecutive output positions, 64 of the panel's images, 16 * CT channels).  Every memory
// instruction between two matrix instructions costs matrix-pipe time (measured: ~20 cycles per load, ~55 per store), so
// the operands come in wide: ONE buffer_load_dwordx4 brings the B operands of FOUR image tiles — a lane (k row kq, li)
// holds images 4 li .. 4 li + 3 of its 64, image tile t = the images with index t modulo 4, any partition of the images
// into sixteens serves —, one ds_read2_b32 the A operands of two channel tiles; the results leave as dwordx4 rows of four
// consecutive images.  B operands run three steps ahead of the products (a ring of three register sets over the flat
// (kernel row, step) sequence), A operands one step ahead.
// IT = image tiles per wave: 4 (64 images, dwordx4 operands and results) or 1 (16 images, dwords: batches of <= 16 images,
// where three quarters of a 64-image item would multiply zeros).
template <int CT, int PW, bool PADDED, int R, int IT>
__global__ __launch_bounds__(1024) void k_conv_dec(DecParams p) {
  extern __shared__ __attribute__((aligned(16))) float ldsW[];          // [knl * Kp][S]
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int P = p.Ho * p.Wo;
  lds_fill<1024>(ldsW, p.wdec, (p.knl * p.Kp * p.S) >> 2);
  __syncthreads();
  const int NS = p.Kp >> 2;                                             // steps (of four k) per kernel row
  const int T = p.knl * NS;                                             // steps per work item
  const int groups = (P + PW - 1) / PW;                                 // position groups per panel
  constexpr int IB = 16 * IT;                                           // images per work item
  const int halves = (p.live + IB - 1) / IB;                            // image blocks a panel has (a small batch: fewer)
  const int chunks = p.Ct / (16 * CT);                                  // channel chunks
  const int nItems = p.panels * groups * halves * chunks;
  const int kClamp = p.Kr - 1;
  const ItemRange ir = xcd_items<16, false>(nItems, wave);
  for (int item = ir.first; item < ir.end; item += ir.stride) {
    // The lane-derived address parts are RE-DERIVED per item from an opaque copy of the lane id: as loop invariants they
    // would have to live through the whole item loop beside 96 accumulator registers, and the compiler spilled two of
    // them to scratch (a handful of vector instructions per ~76 000-cycle item instead).
    int laneI = lane;
    asm volatile("" : "+v"(laneI));
    const int li = laneI & 15, kq = laneI >> 4;
    // channel chunk fastest, then image block: the waves of a workgroup share their B rows through the L1
    const int cc = item % chunks, ib = (item / chunks) % halves, pgi = item / (chunks * halves);
    const int panel = pgi / groups, pos0 = (pgi % groups) * PW;
    int r0[PW], c0[PW];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      const int q = pos0 + j < P ? pos0 + j : P - 1;                    // positions past the map (last group): computed, not stored
      r0[j] = (q / p.Wo) * p.stride - p.pad;
      c0[j] = (q % p.Wo) * p.stride - p.pad;
    }
    // Vector ALU work takes matrix-pipe time on a SIMD (LABBOOK.md), so a B load costs no vector instruction besides
    // itself: a buffer load with the lane's part of the address (k row kq, images 4 li ..) in ONE constant VGPR and
    // everything else — position, kernel row, step — in the scalar offset.  A kernel row of Kr = knl * Cin products is
    // padded to Kp = a multiple of four by letting its LAST step start at k = Kr - 4 (qk_dec_krow): it re-reads rows the
    // step before it already multiplied — their code words are zero in that step (k_decode_weights) — instead of rows of
    // the pixel next to the window: 0 x Inf / NaN of a value outside the window must not reach an output the window does
    // not cover (the table kernels have no such coupling either).  All in the scalar offset: no vector instruction.
    const float* __restrict__ srcU = p.src + (size_t)panel * p.H * p.W * p.Cin * PANEL + ib * IB;
    const size_t left = (size_t)(p.panels - panel) * p.H * p.W * p.Cin * PANEL * sizeof(float) - ib * IB * sizeof(float);
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(srcU), 0, left < 0xffffffffull ? (unsigned)left : 0xffffffffu, 0x00020000);
    const int laneOff = (kq * PANEL + IT * li) * (int)sizeof(float);
    int posOff[PW];                                                     // byte offset of the window's first row, per position
#pragma unroll
    for (int j = 0; j < PW; ++j) posOff[j] = (r0[j] * p.W + c0[j]) * p.Cin * PANEL * (int)sizeof(float);
    const int rowPitch = p.W * p.Cin * PANEL * (int)sizeof(float);
    constexpr int kStep = 4 * PANEL * (int)sizeof(float);                // bytes between two steps' first rows
    // B operands of step `step` of kernel row `kh`: four consecutive panel rows (k) x 64 images, per position
    auto load_b = [&](int kh, int step, int soff, float (&b)[PW][IT]) {
#if QCNN_DEC_VAR & 1
      for (int j = 0; j < PW; ++j) for (int ti = 0; ti < IT; ++ti) b[j][ti] = (float)(kh + step + j + ti);
      return;
#endif
#pragma unroll
      for (int j = 0; j < PW; ++j) {
        if (PADDED) {
          const int row = r0[j] + kh;
          const int k = (step == NS - 1 && p.Kr >= 4) ? p.Kr - 4 + kq : 4 * step + kq;   // the last step ends at the window's last row
          const int kc = k < kClamp ? k : kClamp;                       // k >= Kr (Kr < 4): an operand of the window, its code word is zero
          const int col = c0[j] + kc / p.Cin;
          const bool ok = row >= 0 && row < p.H && col >= 0 && col < p.W;
          const float* __restrict__ px = srcU + (ok ? ((row * p.W + c0[j]) * p.Cin + kc) * PANEL + IT * li : 0);   // a panel map is < 2^31 floats (qk_conv_dec)
          if (IT == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(px);
#pragma unroll
            for (int ti = 0; ti < IT; ++ti) b[j][ti] = ok ? v[ti] : 0.0f;
          } else {
            const float v = *px;
            b[j][0] = ok ? v : 0.0f;
          }
        } else if (IT == 4) {
          const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, laneOff, posOff[j] + soff, 0));
#pragma unroll
          for (int ti = 0; ti < IT; ++ti) b[j][ti] = v[ti];
        } else {
          b[j][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, laneOff, posOff[j] + soff, 0));
        }
      }
    };
    f32x4 acc[PW][CT][IT];                                              // [position][channel tile][image tile]
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(p.bias + (cc * CT + ct) * 16 + 4 * kq);   // D row 4 * kq + r = channel
#pragma unroll
      for (int j = 0; j < PW; ++j)
#pragma unroll
        for (int ti = 0; ti < IT; ++ti) acc[j][ct][ti] = b4;
    }
    // (kernel row, step) of the next B load and its byte offset from the window's first row.  Past the last step the
    // sequence simply runs on (rows below the window, or the buffer's zero): those operands are never multiplied, and
    // loads that are unconditional let the compiler count the ones in flight.
    const int lastOff = NS > 1 ? (p.Kr - 4) * PANEL * (int)sizeof(float) : 0;   // first row of a kernel row's last step
    const int incLast = NS > 1 ? lastOff - (NS - 2) * kStep : 0;        // from the step before the last one to the last one
    const int incWrap = rowPitch - lastOff;                             // from a row's last step to the next row's first
    int khL = 0, stL = 0, soffL = 0;
    float b[R][PW][IT];                                                 // R = operand sets in flight (2 or 3)
    float a[R][CT];
    auto next_b = [&](float (&bb)[PW][IT]) {
      load_b(khL, stL, soffL, bb);
      const int wrap = stL + 1 == NS ? 1 : 0;
      stL = wrap ? 0 : stL + 1;
      khL += wrap;
      soffL += wrap ? incWrap : (stL == NS - 1 ? incLast : kStep);
    };
    // A operands of flat step t: k rows 4 t .. 4 t + 3 (= kh * Kp + 4 * step) of this wave's channels; past the end: LDS zeros
    const float* __restrict__ wl = ldsW + kq * p.S + cc * 16 * CT + li;
    const int aStep = 4 * p.S;
    auto load_a = [&](const float* __restrict__ w, float (&aa)[CT]) {
#if QCNN_DEC_VAR & 2
      for (int ct = 0; ct < CT; ++ct) aa[ct] = (float)ct;
      return;
#endif
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) aa[ct] = w[ct * 16];
    };
    auto products = [&](const float (&aa)[CT], const float (&bb)[PW][IT]) {
#pragma unroll
      for (int j = 0; j < PW; ++j)
#pragma unroll
        for (int ti = 0; ti < IT; ++ti)
#pragma unroll
          for (int ct = 0; ct < CT; ++ct)
            acc[j][ct][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[ct], bb[j][ti], acc[j][ct][ti], 0, 0, 0);
    };
#pragma unroll
    for (int u = 0; u < R; ++u) next_b(b[u]);
    load_a(wl, a[0]);
    int t = 0;
    for (; t + R <= T; t += R) {
#pragma unroll
      for (int u = 0; u < R; ++u) {
        wl += aStep;
        load_a(wl, a[(u + 1) % R]);
        __builtin_amdgcn_sched_barrier(0);
        products(a[u], b[u]);
        __builtin_amdgcn_sched_barrier(0);
        next_b(b[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < R - 1; ++u)                                     // the steps left when T is not a multiple of R
      if (t + u < T) {
        wl += aStep;
        load_a(wl, a[(u + 1) % R]);
        products(a[u], b[u]);
      }
    // D tile ti, element r of lane (li, kq): channel 4 * kq + r of the tile, image IT * li + ti of the block
#pragma unroll
    for (int j = 0; j < PW; ++j) {
      if (pos0 + j >= P) continue;
      float* __restrict__ dst = p.dst + ((size_t)panel * P + pos0 + j) * p.Ct * PANEL + ib * IB + IT * li;
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v[IT];
#pragma unroll
          for (int ti = 0; ti < IT; ++ti) {
            v[ti] = acc[j][ct][ti][r];
            if (p.relu) v[ti] = (0.0f < v[ti]) ? v[ti] : 0.0f;
          }
          float* __restrict__ o = dst + (size_t)((cc * CT + ct) * 16 + 4 * kq + r) * PANEL;
#if QCNN_DEC_VAR & 8
          if (v[0] == 1.2345f)
#endif
          {
            if (IT == 4) *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[IT > 1 ? 1 : 0], v[IT > 2 ? 2 : 0], v[IT > 3 ? 3 : 0]};
            else *o = v[0];
          }
        }
    }
  }
}

// launch with shm bytes of dynamic LDS (above the default limit: raised first)
template <typename Params>
hipError_t launch_lds(void (*kern)(Params), dim3 grid, dim3 block, size_t shm, hipStream_t st, const Params& p) {
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, grid, block, shm, st, p);
  return hipGetLastError();
}

template <int CT, int PW, bool PADDED, int R, int IT>
hipError_t launch_dec(const DecParams& p, hipStream_t st) {
  const int P = p.Ho * p.Wo;
  const long long items = (long long)p.panels * ((P + PW - 1) / PW) * ((p.live + 16 * IT - 1) / (16 * IT)) * (p.Ct / (16 * CT));
  const int blocks = (int)std::min<long long>(256, (items + 15) / 16);    // one persistent workgroup per CU
  return launch_lds(k_conv_dec<CT, PW, PADDED, R, IT>, dim3(blocks), dim3(1024), (size_t)p.knl * p.Kp * p.S * sizeof(float), st, p);
}

// ------------------------------------------------------------------------------------------------------------------
// k_conv_dec_nchw: the same products with the operands taken straight from the NCHW network input — no pack pass (0.24 ms
// per 1000 AlexNet images: 1.24 GB through HBM) in front of the first layer, and k FLAT over the window: k = (c knl + kh) knl
// + kw runs 0 .. Cin knl^2 - 1 in fours whatever the length of a kernel row, so the matrix pipe multiplies 364 (368 with the
// steps padded to a multiple of four; not 11 x 36 = 396) products per output for AlexNet conv1.  Lane (k row kq, li) of step
// s needs element k = 4 s + kq of a window: byte offset c H W 4 + kh W 4 + kw 4 from the window's corner — a table of steps
// x 4 ints the workgroup computes once into LDS — plus the lane's image and position; the item's position group, image tile
// and panel travel in the scalar offset.
// Work item of a wave: 16 images x FOUR NEIGHBOURING POSITIONS of an output row x 96 channels (24 accumulator tiles).  In
// NCHW the images are C H W floats apart, so the 16 rows of a product tile are 2 positions x 8 images: with stride 4 the
// lanes of one image read 4 k x 2 positions = 8 consecutive floats, a dword load touches 8 lines of 32 useful bytes, and the
// four loads of a step and the steps of a kernel row hit the same lines again.  The image values are the A operand (rows of
// the product), the code words B: a lane ends up with FOUR CONSECUTIVE IMAGES of one channel — 24 16-byte stores per item.
// Eight waves of up to 256 registers per CU, a ring of four steps' operands (three in flight, counted s_waitcnt).
// Measured, AlexNet conv1 at 1000 images (scripts/variants_nchw.sh; pack + k_conv_dec: 0.24 + 1.76 ms):
//   tile = 16 images x 1 position, item = 64 images (dword stores)      2.34 ms   (L1: 8 waves x 64 lines per kernel row)
//   tile = 16 images x 1 position, item = 16 images x 4 positions       1.98 ms, 16-byte stores 1.86 ms (loads alone 1.37 ms)
//   tile = 4 images x 4 positions                                       1.96 ms   (loads alone 0.67 ms, 16-byte store fragments)
//   tile = 8 images x 2 positions                                       1.85 ms   (everything but the products 1.10 ms,
//                                                                                  everything but loads or but stores 1.68 ms)
//   one loop body (no peeled tail, no zero-trip path: 225 -> 133 registers), then 5 / 6 positions of 16 images per item
//   1.86 / 2.06 ms, 12 / 16 waves per workgroup 1.86 / 1.88 ms against 1.81 (synthetic parameters): eight waves, four positions;
//   the two 32-byte halves of a row stored back to back 1.79 ms; non-temporal stores 1.86; item = 32 images x 2 positions
//   (whole 128-byte lines per wave) 1.82
// the matrix pipe alone would need 1.42 ms at 2.4 GHz; what is left is the stores and loads of a wave's item boundary that
// its SIMD neighbour's products do not cover.
// The split-bf16 kernel further down has the same tile, items, clamps and stores: the helpers below are both kernels'.
// ------------------------------------------------------------------------------------------------------------------
#ifndef NCHW_WAVES
#define NCHW_WAVES 8
#endif
#ifndef NCHW_VAR
#define NCHW_VAR 0      // timing experiments (scripts/variants_nchw.sh): 1 no operand loads, 2 no products, 4 no stores,
#endif                  // 8 no split (both split kernels), 16 no w3 loads (k_conv_dec_nchw_split only), 32 no fix-up launch
                        // behind k_conv_dec_nchw_f16

typedef int i32x4_t __attribute__((ext_vector_type(4)));

// buffer resource for the inline-assembly loads: base, stride 0, `bytes` (at most 2^32 - 1), raw 32-bit data format
__device__ __forceinline__ i32x4_t raw_rsrc(const void* base, unsigned long long bytes) {
  const unsigned long long a = reinterpret_cast<unsigned long long>(base);
  return i32x4_t{(int)(unsigned)a, (int)((unsigned)(a >> 32) & 0xffffu), (int)(bytes < 0xffffffffull ? (unsigned)bytes : 0xffffffffu),
                 0x00020000};
}

// byte offset of element (c, kh, kw) of a window from the window's corner in an NCHW image
__device__ __forceinline__ int nchw_win_off(const DecParams& p, int c, int kh, int kw) {
  return (int)((uint32_t)c * ((uint32_t)p.H * p.W * 4u) + (uint32_t)kh * ((uint32_t)p.W * 4u) + (uint32_t)kw * 4u);
}

// offset table of k flat over the window, n entries: k = (c knl + kh) knl + kw; past the window the last element again
__device__ __forceinline__ void nchw_flat_offsets(const DecParams& p, int* ldsOff, int n) {
  for (int i = threadIdx.x; i < n; i += 64 * NCHW_WAVES) {
    const int k = min(i, p.Kr - 1);                                     // Kr: Cin knl^2
    ldsOff[i] = nchw_win_off(p, k / (p.knl * p.knl), (k / p.knl) % p.knl, k % p.knl);
  }
}

// The item list of a launch: image tiles of 16 images x channel chunks of 16 CT x position groups of IT consecutive
// positions of an output row x panels
struct NchwGrid {
  uint32_t imgBytes;                                                    // one image, Cin H W floats
  int tiles, chunks, WoG, PG, nItems;
};
template <int CT, int IT>
__device__ __forceinline__ NchwGrid nchw_grid(const DecParams& p) {
  const int tiles = (p.live + 15) / 16;                                 // image tiles a panel has (a small batch: fewer)
  const int chunks = p.Ct / (16 * CT);
  const int WoG = (p.Wo + IT - 1) / IT, PG = p.Ho * WoG;                // position groups: IT consecutive positions of an output row
  return {(uint32_t)p.Cin * p.H * p.W * 4u, tiles, chunks, WoG, PG, p.panels * PG * tiles * chunks};
}

// One work item of a wave, and its lane's place in it
struct NchwItem {
  int laneI, li, kq;                                                    // lane = 16 kq + li; laneI: the same, opaque
  int it, cc, panel, orow, ocol, r0;
  uint32_t img0;                                                        // the tile's first image in the batch
  bool edge;
  int laneOff;                                                          // lane row li of a product tile, from the tile's first row
  uint32_t base0;                                                       // corner of image tile 0's window in the batch
};
template <int IT>
__device__ __forceinline__ NchwItem nchw_item(const DecParams& p, const NchwGrid& g, int item, int lane) {
  int laneI = lane;
  asm volatile("" : "+v"(laneI));                                       // lane-derived constants re-derived per item (registers)
  const int li = laneI & 15, kq = laneI >> 4;
  // image tiles fastest: the eight waves of a workgroup write the 128 images of the same (position, channel) rows at about
  // the same time, so that L2 sees whole lines (position groups fastest: 2.03 against 1.98 ms with dword stores)
  const int it = item % g.tiles, cc = (item / g.tiles) % g.chunks, pg = (item / (g.tiles * g.chunks)) % g.PG, panel = item / (g.chunks * g.tiles * g.PG);
  const int orow = pg / g.WoG, ocol = (pg % g.WoG) * IT;
  const int r0 = orow * p.stride, c0 = ocol * p.stride;                 // unpadded layers
  const uint32_t img0 = (uint32_t)(p.panel0 + panel) * PANEL + (uint32_t)it * 16u;
  // row li of a product tile: image li & 7 of the tile's eight, position li >> 3 of its two.  Positions past the end of the
  // output row read columns of the next image row, of the next plane, of the next image ... finite values, never stored.
  // That stays inside the caller's buffer as long as an image FOLLOWS the tile's sixteen.  An item that holds the batch's
  // last image or images past it (a ragged last panel launches all eight image tiles) takes the `edge` form of the body
  // (nchw_tile_bases).
  const bool edge = img0 + 16u >= (uint32_t)p.nImages;
  const int laneOff = (int)((uint32_t)(li & 7) * g.imgBytes + (uint32_t)((li >> 3) * p.stride) * 4u);
  const uint32_t base0 = img0 * g.imgBytes + (uint32_t)(r0 * p.W + c0) * 4u;
  return {laneI, li, kq, it, cc, panel, orow, ocol, r0, img0, edge, laneOff, base0};
}

// Lane part (vector offset) and scalar base of image tile ti's loads: 8 (ti & 1) images and 2 (ti >> 1) positions on from
// tile 0.  EDGE: every image index is clamped to the last image and every position to the last of its output row — in the
// scalar offset AND per lane —, so that no address leaves the batch whatever the buffer's range check does with the scalar
// offset (the gfx9 raw-buffer check covers the vector offset only), and (last image) x imgBytes cannot wrap 32 bits.  Those
// lanes' results are never stored / never read.
template <bool EDGE, int IT>
__device__ __forceinline__ void nchw_tile_bases(const DecParams& p, const NchwGrid& g, const NchwItem& w, int (&laneOffT)[IT],
                                                uint32_t (&baseT)[IT]) {
#pragma unroll
  for (int ti = 0; ti < IT; ++ti) {
    laneOffT[ti] = w.laneOff;
    baseT[ti] = w.base0 + (uint32_t)(ti & 1) * 8u * g.imgBytes + (uint32_t)((ti >> 1) * 2 * p.stride) * 4u;
  }
  if constexpr (EDGE) {
    const uint32_t lastImg = (uint32_t)p.nImages - 1u, lastPos = (uint32_t)p.Wo - 1u;
#pragma unroll
    for (int ti = 0; ti < IT; ++ti) {
      const uint32_t imgS = min(w.img0 + 8u * (uint32_t)(ti & 1), lastImg), imgL = min(w.img0 + 8u * (uint32_t)(ti & 1) + (uint32_t)(w.li & 7), lastImg);
      const uint32_t posS = min((uint32_t)w.ocol + 2u * (uint32_t)(ti >> 1), lastPos), posL = min((uint32_t)w.ocol + 2u * (uint32_t)(ti >> 1) + (uint32_t)(w.li >> 3), lastPos);
      laneOffT[ti] = (int)((imgL - imgS) * g.imgBytes + (posL - posS) * (uint32_t)p.stride * 4u);
      baseT[ti] = imgS * g.imgBytes + ((uint32_t)(w.r0 * p.W) + posS * (uint32_t)p.stride) * 4u;
    }
  }
}

template <int CT, int IT>
__device__ __forceinline__ void nchw_bias(const DecParams& p, const NchwItem& w, f32x4 (&acc)[CT][IT]) {
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) {
    const float b1 = p.bias[(w.cc * CT + ct) * 16 + w.li];
#pragma unroll
    for (int ti = 0; ti < IT; ++ti) acc[ct][ti] = f32x4{b1, b1, b1, b1};
  }
}

// The image values are the rows of a product (A), the code words its columns (B): lane (li, kq) holds channel li of the tile
// at position kq >> 1 of the tile's two for the FOUR CONSECUTIVE images 4 (kq & 1) .. + 3 of its eight — one 16-byte store
// per tile
// SCALED (k_conv_dec_nchw_f16): the sums are in units of 1 / outScale, an exact power of two
template <int CT, int IT, bool SCALED = false>
__device__ __forceinline__ void nchw_store(const DecParams& p, const NchwItem& w, const f32x4 (&acc)[CT][IT], float outScale = 1.0f) {
  const int nPos = (NCHW_VAR & 4) ? (p.Wo < 0 ? IT : 0) : min(IT, p.Wo - w.ocol);
  float* __restrict__ dst = p.dst + (((size_t)w.panel * (p.Ho * p.Wo) + w.orow * p.Wo + w.ocol + (w.kq >> 1)) * p.Ct + w.li) * PANEL +
                            w.it * 16 + 4 * (w.kq & 1);
  // two copies of the store loop under one uniform branch: a ReLU applied under a branch INSIDE the loop made the compiler
  // keep a second set of result registers (225 instead of 140)
  if (p.relu) {
    // the two halves (images 0-7, 8-15) of a row's 64 bytes leave back to back (1.81 -> 1.79 ms)
#pragma unroll
    for (int tp = 0; tp < IT / 2; ++tp)
      if (tp * 2 + (w.kq >> 1) < nPos) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int ti = tp * 2 + h;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float r = SCALED ? acc[ct][ti][e] * outScale : acc[ct][ti][e];
              v[e] = (0.0f < r) ? r : 0.0f;
            }
            *reinterpret_cast<f32x4*>(dst + ((size_t)tp * 2 * p.Ct + (w.cc * CT + ct) * 16) * PANEL + 8 * h) = v;
            __builtin_amdgcn_sched_barrier(0);
          }
      }
  } else {
#pragma unroll
    for (int ti = 0; ti < IT; ++ti)
      if ((ti >> 1) * 2 + (w.kq >> 1) < nPos) {
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
          *reinterpret_cast<f32x4*>(dst + ((size_t)(ti >> 1) * 2 * p.Ct + (w.cc * CT + ct) * 16) * PANEL + 8 * (ti & 1)) =
              SCALED ? acc[ct][ti] * outScale : acc[ct][ti];
      }
  }
}

// The same rows for the images of `mask` only (bit i: image i of the item's sixteen), one float each: the fix-up launch behind
// k_conv_dec_nchw_f16 leaves every other image's results as they are
template <int CT, int IT>
__device__ __forceinline__ void nchw_store_images(const DecParams& p, const NchwItem& w, const f32x4 (&acc)[CT][IT], unsigned mask) {
  const int nPos = min(IT, p.Wo - w.ocol);
  float* __restrict__ dst = p.dst + (((size_t)w.panel * (p.Ho * p.Wo) + w.orow * p.Wo + w.ocol + (w.kq >> 1)) * p.Ct + w.li) * PANEL +
                            w.it * 16 + 4 * (w.kq & 1);
#pragma unroll
  for (int ti = 0; ti < IT; ++ti)
    if ((ti >> 1) * 2 + (w.kq >> 1) < nPos) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((mask >> (8 * (ti & 1) + 4 * (w.kq & 1) + e)) & 1u) {
            const float r = acc[ct][ti][e];
            dst[((size_t)(ti >> 1) * 2 * p.Ct + (w.cc * CT + ct) * 16) * PANEL + 8 * (ti & 1) + e] = p.relu ? ((0.0f < r) ? r : 0.0f) : r;
          }
    }
}

// s_waitcnt vmcnt(N) that the operands of a step pass through (the compiler must not move their uses above it)
template <int N>
__device__ __forceinline__ void nchw_wait(float (&bb)[4]) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(bb[0]), "+v"(bb[1]), "+v"(bb[2]), "+v"(bb[3]) : "n"(N));
}

template <int CT, int IT>
__global__ __launch_bounds__(64 * NCHW_WAVES) void k_conv_dec_nchw(DecParams p) {
  static_assert(IT == 4, "a product tile is 2 positions x 8 images, an item two pairs of positions x two image halves");
  extern __shared__ __attribute__((aligned(16))) float ldsW[];          // [steps][Ct / 16][4 k][16]: a wave's read of one channel tile is
                                                                        // 64 consecutive floats (no bank conflicts); then int [steps + 4][4]
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int steps = p.Kp >> 2;                                          // Kp: Cin knl^2 padded to a multiple of 16
  // (one step of slack behind the code words: the last step of an item pre-loads "the next step's" code words, which nobody
  // uses — the offset table sits behind that slack, inside the allocation)
  int* ldsOff = reinterpret_cast<int*>(ldsW + (size_t)(steps + 1) * 4 * p.S);
  lds_fill<64 * NCHW_WAVES>(ldsW, p.wdec, steps * p.S);
  nchw_flat_offsets(p, ldsOff, (steps + 4) * 4);
  __syncthreads();
  const NchwGrid g = nchw_grid<CT, IT>(p);
  // No load below depends on the buffer's range check: every address is inside the batch by construction (see `edge`)
  const i32x4_t rsrc4 = raw_rsrc(p.src, (unsigned long long)p.nImages * g.imgBytes);
  const ItemRange ir = xcd_items<NCHW_WAVES, true>(g.nItems, wave);
  for (int item = ir.first; item < ir.end; item += ir.stride) {
    const NchwItem w = nchw_item<IT>(p, g, item, lane);
    const int* __restrict__ offT = ldsOff + w.kq;
   auto body = [&](auto edgeTag) {
    int laneOffT[IT];
    uint32_t baseT[IT];
    nchw_tile_bases<decltype(edgeTag)::value>(p, g, w, laneOffT, baseT);
    // Operand loads as inline assembly with counted waits: the compiler's own vmcnt bookkeeping drains the ring to one
    // step at every loop back edge (s_waitcnt vmcnt(4) in front of the first of four steps).  Loads return in order, so
    // "at most 12 outstanding" = everything but the three newest steps has arrived — whatever else (the previous item's
    // stores) is still in flight only makes the wait stricter.
    auto issue = [&, rsrc4](int s, float (&bb)[IT]) {                  // the operands of step s (explicit capture: asm operand inside a generic lambda)
      const int ot = offT[s * 4];
#pragma unroll
      for (int ti = 0; ti < IT; ++ti)
        if (NCHW_VAR & 1) asm volatile("v_mov_b32 %0, %1" : "=v"(bb[ti]) : "v"(ot + w.laneOff)); else
        asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(bb[ti]) : "v"(ot + laneOffT[ti]), "s"(rsrc4), "s"(baseT[ti]));
    };
    f32x4 acc[CT][IT];
    nchw_bias(p, w, acc);
    const float* __restrict__ wl = ldsW + w.cc * 64 * CT + w.laneI;
    const int aStep = 4 * p.S;
    float a[2][CT], b[4][IT];                                           // b: a ring of four steps' operands, three in flight (a ring
                                                                        // of eight: no faster)
    auto load_a = [&](const float* __restrict__ wp, float (&aa)[CT]) {
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) aa[ct] = wp[ct * 64];
    };
    issue(0, b[0]);
    issue(1, b[1]);
    issue(2, b[2]);
    load_a(wl, a[0]);
#define NCHW_WAIT(n, bb) nchw_wait<n * IT>(bb)
#define NCHW_STEP(u, n) /* step s + u; the loads of at most n steps may still be in flight */                                       \
  {                                                                                                                   \
    wl += aStep;                                                                                                      \
    load_a(wl, a[((u) + 1) & 1]); /* code words of the next step */                                                   \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
    NCHW_WAIT(n, b[u]);                                                                                               \
    _Pragma("unroll") for (int ti = 0; ti < IT; ++ti)                                                                 \
      _Pragma("unroll") for (int ct = 0; ct < CT; ++ct)                                                               \
        if (NCHW_VAR & 2) asm volatile("" : "+v"(acc[ct][ti]) : "v"(a[(u) & 1][ct]), "v"(b[u][ti])); else             \
        acc[ct][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[u][ti], a[(u) & 1][ct], acc[ct][ti], 0, 0, 0);           \
    __builtin_amdgcn_sched_barrier(0);                                                                                \
  }
    // three steps ahead, into the set the step before released.  The last iteration fetches three steps past the end (the
    // offset table repeats the window's last element there): 12 loads of 4 steps x IT per item that nobody reads — the
    // price of ONE loop body: a peeled tail with decreasing wait counts made the compiler keep the accumulators in a
    // second register block (225 registers; 5 positions per item did not fit)
    int s = 0;
    do {                                                                // (at least four steps: no zero-trip copy of the accumulators)
      issue(s + 3, b[3]); NCHW_STEP(0, 3)
      issue(s + 4, b[0]); NCHW_STEP(1, 3)
      issue(s + 5, b[1]); NCHW_STEP(2, 3)
      issue(s + 6, b[2]); NCHW_STEP(3, 3)
    } while ((s += 4) < steps);
    NCHW_WAIT(0, b[0]); NCHW_WAIT(0, b[1]); NCHW_WAIT(0, b[2]);         // nothing in flight into registers the stores may reuse
#undef NCHW_STEP
#undef NCHW_WAIT
    nchw_store(p, w, acc);
   };
    if (w.edge) body(std::true_type{}); else body(std::false_type{});
  }
}

// rows: [kh][kw][1][rowStride] slot bytes; ctrd: [Cs][K]; out: [step][S / 16][4 kq][16]: the code word of window element
// k = 4 step + kq = (c knl + kh) knl + kw, zero past the window
__global__ void k_decode_weights_nchw(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd, float* __restrict__ out,
                                      QkSlots sl, int knl, int Cin, int K, int Ct, int steps, int S) {
  const int total = steps * 4 * S;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int ch = (i % 16) + 16 * ((i / 64) % (S / 16)), kq = (i / 16) % 4, step = i / (4 * S);
    const int k = 4 * step + kq;
    out[i] = ch < Ct && k < Cin * knl * knl ? code_word(rows, ctrd, sl, knl, K, k / (knl * knl), (k / knl) % knl, k % knl, ch) : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// k_conv_dec_nchw_split (QCNN_OPT_DEC_BF16SPLIT = 1; the default, 2, is k_conv_dec_nchw_f16 further down): the same layer at fp32
// accuracy on the BF16 matrix pipe.  The
// f32 kernel above is bound by v_mfma_f32_16x16x4_f32 (32 cycles per 4 k: 1.42 of its 1.85 ms); gfx950 has no xf32, and its
// bf16 rate is 16x the f32 one.  Every fp32 value splits EXACTLY into three bf16 pieces (round to nearest, remainder in
// fp32: 8 + 8 + 8 significant bits), x = x1 + x2 + x3, w = w1 + w2 + w3, and the six cross terms down to order 2^-16,
//     x3 w1, x2 w2, x1 w3, x2 w1, x1 w2, x1 w1      (in that order: small terms first),
// go to v_mfma_f32_16x16x32_bf16 — each bf16 x bf16 product is exact in fp32, the accumulator is fp32 — while the dropped
// x2 w3, x3 w2, x3 w3 are of order 2^-24, one fp32 rounding.  Six 16-cycle MFMAs per 32 k: 3 cycles per k against 8.
// Layout: a lane (li, kq) of a 16x16x32 product holds row li of the product tile (nchw_item) and k = 8 kq .. 8 kq + 7 of the
// step; items, clamps (nchw_tile_bases) and stores (nchw_store) are the shared ones.  k is flat over the window as above,
// padded to a multiple of 32 (the offset table repeats the window's last element, the code words there are zero).  A step:
// 8 dword loads per image tile (same loads per k as the f32 kernel), split once in registers and shared by the six channel
// tiles (36 MFMAs per fragment).  Code words: the decoder writes the pieces once per upload; w1 and w2 stay in LDS (Kb x Ct x
// 4 bytes: 144 KB for AlexNet conv1 — all three planes would be 216 KB), w3 (74 KB) streams from L2 through the buffer loads,
// one dwordx4 per channel tile and step.  Operand loads are inline assembly with counted waits (see the f32 kernel): step s
// splits its raw values, issues step s + 1's loads into the same registers, then runs its channel tiles, each followed by
// the w3 load of step s + 1.  The sum per output — bias, then per step the six terms in fixed order — depends on nothing but
// the output, as before.
// RUNS (the default where it fits, nchw_split_runs): k in RUN ORDER instead.  Every (channel, kernel row) of the window is
// cut into nr = ceil(knl / 4) runs of 4 consecutive columns; run r of a row starts at column min(4 r, knl - 4), so that
// the last run overlaps its predecessor instead of reaching past the row (knl 11: columns 0, 4, 7), and the code words of
// the repeated columns are zero.  k = 4 run + e (e: the column in the run); a lane's 8 k of a step are two runs, each ONE
// buffer_load_dwordx4 (dword aligned: a window row is any number of floats) — 8 loads per step instead of 32.  The LDS
// table holds run offsets; runs past the last repeat it (code words zero).  Every read stays inside its window row.
// Shapes whose run-ordered w1 / w2 do not fit LDS, and kernel rows shorter than 4 columns, keep the flat order.
// ------------------------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// x = x1 + x2 + x3 exactly (finite x; v_cvt_pk_bf16_f32 rounds to nearest even)
__device__ __forceinline__ void split_bf16x8(const f32x4 (&x)[2], bf16x8& h1, bf16x8& h2, bf16x8& h3) {
  u32x4 p1, p2, p3;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float x0 = x[q >> 1][2 * (q & 1)], x1 = x[q >> 1][2 * (q & 1) + 1];
    const unsigned a = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
    const float r0 = x0 - __builtin_bit_cast(float, a << 16), r1 = x1 - __builtin_bit_cast(float, a & 0xffff0000u);
    const unsigned b = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{r0, r1}, bf16x2));
    const float s0 = r0 - __builtin_bit_cast(float, b << 16), s1 = r1 - __builtin_bit_cast(float, b & 0xffff0000u);
    p1[q] = a; p2[q] = b;
    p3[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{s0, s1}, bf16x2));
  }
  h1 = __builtin_bit_cast(bf16x8, p1); h2 = __builtin_bit_cast(bf16x8, p2); h3 = __builtin_bit_cast(bf16x8, p3);
}

template <int N>
__device__ __forceinline__ void split_wait(f32x4 (&x)[4][2]) {
  asm volatile("s_waitcnt vmcnt(%8)" : "+v"(x[0][0]), "+v"(x[0][1]), "+v"(x[1][0]), "+v"(x[1][1]), "+v"(x[2][0]), "+v"(x[2][1]),
               "+v"(x[3][0]), "+v"(x[3][1]) : "n"(N));
}
template <int N>
__device__ __forceinline__ void split_wait(u32x4& w) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(w) : "n"(N)); }

// The per-launch guard region of k_conv_dec_nchw_f16 (p.guard): word 0 = p.epoch when the launch flagged anything (never
// cleared: the next launch has another epoch), then from byte 16 one 16-bit image mask per item
__device__ __forceinline__ uint16_t* nchw_guard_masks(const DecParams& p) { return reinterpret_cast<uint16_t*>(p.guard + 4); }

// runs per kernel row of the run order (k_conv_dec_nchw_split<.., RUNS>), 0: the flat order; Kb of either order
static inline int nchw_split_kb(int Cin, int knl, int nr) { return nr ? (Cin * knl * nr + 7) / 8 * 32 : (Cin * knl * knl + 31) / 32 * 32; }
static inline size_t nchw_split_lds(int Kb, int Ct, int nr) {    // w1 / w2 + the offset table (one step of slack behind it)
  return (size_t)Kb * Ct * 4 + (size_t)(nr ? Kb / 4 + 8 : Kb + 32) * 4;
}
static int nchw_split_runs(int Cin, int knl, int Ct) {
  if (knl < 4) return 0;
  const int nr = (knl + 3) / 4;
  return nchw_split_lds(nchw_split_kb(Cin, knl, nr), Ct, nr) <= 160 * 1024 ? nr : 0;
}

// What the two split kernels (bf16 pieces below, fp16 pieces further down) share: both pieces of every code word in LDS, 4 bytes
// per code word, and behind them the offset table of the k order — RUNS: one entry per run of 4 columns, else one per k
template <bool RUNS>
__device__ __forceinline__ void split_fill_lds(const DecParams& p, float* ldsW, int* ldsOff) {
  lds_fill<64 * NCHW_WAVES>(ldsW, p.wdec, (p.Kp * p.S) >> 2);          // w1, w2: 4 bytes per code word
  if constexpr (RUNS) {
    const int nr = (p.knl + 3) >> 2, nRuns = p.Cin * p.knl * nr;
    for (int i = threadIdx.x; i < (p.Kp >> 2) + 8; i += 64 * NCHW_WAVES) {
      const int r = min(i, nRuns - 1);
      ldsOff[i] = nchw_win_off(p, r / (nr * p.knl), (r / nr) % p.knl, min(4 * (r % nr), p.knl - 4));
    }
  } else {
    nchw_flat_offsets(p, ldsOff, p.Kp + 32);
  }
}

// the operand loads of step s (lane: k = 32 s + 8 kq + j; offT: the lane's part of the offset table).  RUNS: 2 x IT, one
// dwordx4 per run (k = 4 run + e), else 8 x IT dwords
template <int IT, bool RUNS>
__device__ __forceinline__ void split_issue_x(const int* __restrict__ offT, int s, const int (&laneOffT)[IT], const uint32_t (&baseT)[IT],
                                              i32x4_t rsrc4, f32x4 (&xr)[IT][2]) {
  if constexpr (RUNS) {
    typedef int i32x2_t __attribute__((ext_vector_type(2)));
    const i32x2_t o = *reinterpret_cast<const i32x2_t*>(offT + 8 * s);
#pragma unroll
    for (int ti = 0; ti < IT; ++ti)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (NCHW_VAR & 1) {
          float v;
          asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "v"(o[h]));
          xr[ti][h] = f32x4{v, v, v, v};
        } else
        asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(xr[ti][h]) : "v"(o[h] + laneOffT[ti]), "s"(rsrc4), "s"(baseT[ti]));
      }
  } else {
    const i32x4_t o0 = *reinterpret_cast<const i32x4_t*>(offT + 32 * s), o1 = *reinterpret_cast<const i32x4_t*>(offT + 32 * s + 4);
    const int ot[8] = {o0[0], o0[1], o0[2], o0[3], o1[0], o1[1], o1[2], o1[3]};
#pragma unroll
    for (int ti = 0; ti < IT; ++ti)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v;
        if (NCHW_VAR & 1) asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "v"(ot[j]));
        else asm volatile("buffer_load_dword %0, %1, %2, %3 offen" : "=v"(v) : "v"(ot[j] + laneOffT[ti]), "s"(rsrc4), "s"(baseT[ti]));
        xr[ti][j >> 2][j & 3] = v;
      }
  }
}

// FIXUP (k_conv_dec_nchw_fixup): the launch behind k_conv_dec_nchw_f16 (further down).  It leaves at once unless that launch flagged an input value
// outside the fp16 form's range (p.guard[0] == p.epoch); then it computes the flagged items — same items, same sums, same bits
// as this kernel alone — and stores the flagged images' results only.
template <int CT, int IT, bool RUNS, bool FIXUP>
__device__ __forceinline__ void conv_dec_nchw_split(const DecParams& p, float* ldsW) {
  static_assert(IT == 4 && CT == 6, "a product tile is 2 positions x 8 images, an item two pairs of positions x two image halves x 96 channels");
  if constexpr (FIXUP) {
    if (*p.guard != p.epoch) return;                                    // nothing flagged: no LDS fill, no item
  }
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int steps = p.Kp >> 5;                                          // Kp: Cin knl^2 padded to a multiple of 32
  const int CTs = p.S >> 4;                                             // channel tiles of the layer
  int* ldsOff = reinterpret_cast<int*>(ldsW + (size_t)p.Kp * p.S);
  split_fill_lds<RUNS>(p, ldsW, ldsOff);
  __syncthreads();
  const NchwGrid g = nchw_grid<CT, IT>(p);
  const i32x4_t rsrc4 = raw_rsrc(p.src, (unsigned long long)p.nImages * g.imgBytes);
  // w3: [steps][S / 16][64 lanes][8 bf16] behind w1 / w2; the step in the VECTOR offset, so that the range check turns the
  // last step's pre-load of "step `steps`" into zeros
  const uint32_t w3Step = (uint32_t)p.S * 64u;
  const i32x4_t rsrcW = raw_rsrc(p.wdec + (size_t)p.Kp * p.S, (uint32_t)p.Kp * p.S * 2u);
  const ItemRange ir = xcd_items<NCHW_WAVES, true>(g.nItems, wave);
  for (int item = ir.first; item < ir.end; item += ir.stride) {
    unsigned fixMask = 0;
    if constexpr (FIXUP) {
      fixMask = uni(nchw_guard_masks(p)[item]);
      if (!fixMask) continue;
    }
    const NchwItem w = nchw_item<IT>(p, g, item, lane);
   auto body = [&](auto edgeTag) {
    int laneOffT[IT];
    uint32_t baseT[IT];
    nchw_tile_bases<decltype(edgeTag)::value>(p, g, w, laneOffT, baseT);
    const int* __restrict__ offT = ldsOff + (RUNS ? 2 : 8) * w.kq;
    f32x4 xr[IT][2];                                                    // raw operands of the next step
    auto issue_x = [&, rsrc4](int s) { split_issue_x<IT, RUNS>(offT, s, laneOffT, baseT, rsrc4, xr); };
    u32x4 w3[CT];                                                       // w3 of (step, channel tile): one dwordx4 per lane
    const int w3Lane = lane * 16;
    auto issue_w3 = [&, rsrcW, w3Step](int s, int ct) {
      if (NCHW_VAR & 16) asm volatile("v_mov_b32 %0, %1" : "=v"(w3[ct][0]) : "v"(s)); else
      asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(w3[ct]) : "v"(w3Lane + (int)(s * w3Step)), "s"(rsrcW),
                   "s"((uint32_t)((w.cc * CT + ct) * 1024)));
    };
    f32x4 acc[CT][IT];
    nchw_bias(p, w, acc);
    // w1 / w2 of (step, channel tile) in LDS: 1 KB per piece, lane-contiguous 16-byte reads
    const u32x4* __restrict__ wl = reinterpret_cast<const u32x4*>(ldsW) + (size_t)(w.cc * CT) * 128 + lane;
    const int wStep = CTs * 128;                                        // u32x4 per step
    issue_x(0);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) issue_w3(0, ct);
    // Outstanding loads are counted in issue order: at the top of step s the raw values of step s are followed by the six
    // w3 loads of step s (vmcnt 6); before channel tile ct, its w3 load is followed by the w3 loads of tiles ct + 1 .. 5 of
    // step s, the 32 (RUNS: 8) operand loads of step s + 1 and the w3 loads of its tiles 0 .. ct - 1: 37 (13) whatever ct
    constexpr int xLoads = (RUNS ? 2 : 8) * IT;
    int s = 0;
    do {
      u32x4 bw[2][2];
      bw[0][0] = wl[0]; bw[0][1] = wl[64];
      split_wait<CT>(xr);
      bf16x8 a1[IT], a2[IT], a3[IT];
#pragma unroll
      for (int ti = 0; ti < IT; ++ti) {
        if (NCHW_VAR & 8) {
          a1[ti] = __builtin_bit_cast(bf16x8, xr[ti][0]);
          a2[ti] = a1[ti]; a3[ti] = a1[ti];
        } else {
          split_bf16x8(xr[ti], a1[ti], a2[ti], a3[ti]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      issue_x(s + 1);                                                   // (the last step: the window's last element again, never used)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        if (ct + 1 < CT) { bw[(ct + 1) & 1][0] = wl[(ct + 1) * 128]; bw[(ct + 1) & 1][1] = wl[(ct + 1) * 128 + 64]; }
        split_wait<CT - 1 + xLoads>(w3[ct]);
        const bf16x8 b1 = __builtin_bit_cast(bf16x8, bw[ct & 1][0]), b2 = __builtin_bit_cast(bf16x8, bw[ct & 1][1]);
        const bf16x8 b3 = __builtin_bit_cast(bf16x8, w3[ct]);
#define SPLIT_TERM(A, B)                                                                                               \
  _Pragma("unroll") for (int ti = 0; ti < IT; ++ti)                                                                    \
    if (NCHW_VAR & 2) asm volatile("" : "+v"(acc[ct][ti]) : "v"(A[ti]), "v"(B)); else                                  \
    acc[ct][ti] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[ti], B, acc[ct][ti], 0, 0, 0);
        SPLIT_TERM(a3, b1) SPLIT_TERM(a2, b2) SPLIT_TERM(a1, b3) SPLIT_TERM(a2, b1) SPLIT_TERM(a1, b2) SPLIT_TERM(a1, b1)
#undef SPLIT_TERM
        __builtin_amdgcn_sched_barrier(0);
        issue_w3(s + 1, ct);
        __builtin_amdgcn_sched_barrier(0);
      }
      wl += wStep;
    } while (++s < steps);
    split_wait<0>(xr);                                                  // nothing in flight into registers the stores may reuse
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) split_wait<0>(w3[ct]);
    if constexpr (FIXUP) nchw_store_images(p, w, acc, fixMask); else
    nchw_store(p, w, acc);
   };
    if (w.edge) body(std::true_type{}); else body(std::false_type{});
  }
}

// ldsW: [steps][S / 16][piece 2][64 lanes][8 bf16], then int [Kp + 32] (RUNS: int [Kp / 4 + 8], one per run)
template <int CT, int IT, bool RUNS>
__global__ __launch_bounds__(64 * NCHW_WAVES) void k_conv_dec_nchw_split(DecParams p) {
  extern __shared__ __attribute__((aligned(16))) float ldsW[];
  conv_dec_nchw_split<CT, IT, RUNS, false>(p, ldsW);
}
template <int CT, int IT, bool RUNS>
__global__ __launch_bounds__(64 * NCHW_WAVES) void k_conv_dec_nchw_fixup(DecParams p) {
  extern __shared__ __attribute__((aligned(16))) float ldsW[];
  conv_dec_nchw_split<CT, IT, RUNS, true>(p, ldsW);
}

__device__ __forceinline__ float bf16_hi(float x, uint16_t* h) {      // round to nearest even (finite x); returns the piece as fp32
  uint32_t u = __builtin_bit_cast(uint32_t, x);
  u += 0x7fffu + ((u >> 16) & 1u);
  *h = (uint16_t)(u >> 16);
  return __builtin_bit_cast(float, u & 0xffff0000u);
}

// rows: [kh][kw][1][rowStride] slot bytes; ctrd: [Cs][K]; out: w1 / w2 [step][S / 16][piece][64 lanes][8], then
// w3 [step][S / 16][64 lanes][8] (bf16): lane (li, kg), element j = the code word of k = 32 step + 8 kg + j for channel
// 16 tile + li, zero past the window; w = w1 + w2 + w3 exactly.  nr = 0: k flat over the window; nr > 0: run order
// (k_conv_dec_nchw_split<.., true>), k = 4 run + e, zero on the columns a row's last run repeats
__global__ void k_decode_weights_split(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd, uint16_t* __restrict__ out,
                                       QkSlots sl, int knl, int Cin, int K, int Ct, int Kb, int S, int nr) {
  const int total = Kb * S, CTs = S / 16;
  uint16_t* __restrict__ out3 = out + (size_t)2 * total;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int j = i & 7, ln = (i >> 3) & 63, tile = (i >> 9) % CTs, step = (i >> 9) / CTs;
    const int ch = 16 * tile + (ln & 15), k = 32 * step + 8 * (ln >> 4) + j;
    float w = 0.0f;
    int kw = k % knl, kh = (k / knl) % knl, c = k / (knl * knl);
    bool live = k < Cin * knl * knl;
    if (nr) {
      const int r = k >> 2, ri = r % nr;
      kw = min(4 * ri, knl - 4) + (k & 3); kh = (r / nr) % knl; c = r / (nr * knl);
      live = r < Cin * knl * nr && kw >= 4 * ri;
    }
    if (ch < Ct && live) w = code_word(rows, ctrd, sl, knl, K, c, kh, kw, ch);
    uint16_t h1, h2, h3;
    const float r = w - bf16_hi(w, &h1);
    (void)bf16_hi(r - bf16_hi(r, &h2), &h3);
    const size_t blk = (size_t)(step * CTs + tile) * 2 * 512 + ln * 8 + j;
    out[blk] = h1;
    out[blk + 512] = h2;
    out3[i] = h3;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// k_conv_dec_nchw_f16 (QCNN_OPT_DEC_BF16SPLIT = 2, default): the same layer with TWO fp16 pieces per operand and THREE cross
// terms.  An fp16 piece has 11 significant bits: x1 = f16(Sx x), x2 = f16(Sx x - x1) (the remainder is exact in fp32) carry 22
// bits of x, likewise w1, w2 of Sw w, and
//     x2 w1, x1 w2, x1 w1                             (in that order: small terms first)
// on v_mfma_f32_16x16x32_f16 — the bf16 instruction's 16 cycles — reproduce a product to 3 x 2^-22: the two split remainders
// and the dropped x2 w2.  Half the matrix instructions of the bf16 form, no w3 plane (w1 / w2 as fp16 are the 4 bytes per code
// word the LDS holds anyway), one split stage fewer.  fp16 has a narrow range, so both operands are scaled by exact powers
// of two: Sx = QK_F16_SX for |x| <= QK_F16_XMAX, Sw per layer from max |w| (qk_f16_weight_scale; it stands in front of the
// planes); the accumulators start from bias Sx Sw and the store multiplies by 1 / (Sx Sw), both exact.  Items, clamps, edge
// handling, XCD split, LDS layout and k orders are the bf16 kernel's; the sum per output — bias, then per step the three terms
// in fixed order — depends on nothing but the output.
// RANGE GUARD: the API takes any float.  Every loaded value is tested with !(|x| <= QK_F16_XMAX) (NaN too); per product-tile row
// = (position, image) the flags are reduced over k and the steps, rows of positions past the output row (they read another
// image's columns) and of images past the batch are dropped, and the item's 16-bit image mask goes to p.guard (one writer per
// entry, no atomics; word 0 = p.epoch when any mask is non-zero).  The fix-up launch (k_conv_dec_nchw_fixup) behind
// this one recomputes the flagged (item, image) pairs with the bf16 form: their results are option 1's bits, every other
// image's are untouched, and what an image gets never depends on its neighbours in the batch.
// ------------------------------------------------------------------------------------------------------------------
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// Sx x = (x1 + x2) (1 + d), |d| <= 2^-22 (finite |x| <= QK_F16_XMAX; v_cvt_pk_f16_f32 rounds to nearest even)
__device__ __forceinline__ void split_f16x8(const f32x4 (&x)[2], f16x8& h1, f16x8& h2) {
  u32x4 p1, p2;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x2 sx = f32x2{x[q >> 1][2 * (q & 1)], x[q >> 1][2 * (q & 1) + 1]} * QK_F16_SX;
    const f16x2 a = __builtin_convertvector(sx, f16x2);
    const f32x2 r = sx - __builtin_convertvector(a, f32x2);
    p1[q] = __builtin_bit_cast(unsigned, a);
    p2[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
  }
  h1 = __builtin_bit_cast(f16x8, p1); h2 = __builtin_bit_cast(f16x8, p2);
}

template <int CT, int IT, bool RUNS>
__global__ __launch_bounds__(64 * NCHW_WAVES) void k_conv_dec_nchw_f16(DecParams p) {
  static_assert(IT == 4 && CT == 6, "a product tile is 2 positions x 8 images, an item two pairs of positions x two image halves x 96 channels");
  extern __shared__ __attribute__((aligned(16))) float ldsW[];          // [steps][S / 16][piece 2][64 lanes][8 fp16], then the offset table
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int steps = p.Kp >> 5;
  const int CTs = p.S >> 4;
  int* ldsOff = reinterpret_cast<int*>(ldsW + (size_t)p.Kp * p.S);
  split_fill_lds<RUNS>(p, ldsW, ldsOff);
  __syncthreads();
  const NchwGrid g = nchw_grid<CT, IT>(p);
  const i32x4_t rsrc4 = raw_rsrc(p.src, (unsigned long long)p.nImages * g.imgBytes);
  const float accScale = p.accScale, outScale = p.outScale;
  uint32_t* const guard = p.guard;
  uint16_t* const masks = nchw_guard_masks(p);
  const uint32_t epoch = p.epoch;
  const ItemRange ir = xcd_items<NCHW_WAVES, true>(g.nItems, wave);
  for (int item = ir.first; item < ir.end; item += ir.stride) {
    const NchwItem w = nchw_item<IT>(p, g, item, lane);
   auto body = [&](auto edgeTag) {
    unsigned long long bad[IT] = {0, 0, 0, 0};                          // per image tile: the lanes (rows x k quarters) that met a value out of range
    int laneOffT[IT];
    uint32_t baseT[IT];
    nchw_tile_bases<decltype(edgeTag)::value>(p, g, w, laneOffT, baseT);
    const int* __restrict__ offT = ldsOff + (RUNS ? 2 : 8) * w.kq;
    f32x4 xr[IT][2];                                                    // raw operands of the next step
    auto issue_x = [&, rsrc4](int s) { split_issue_x<IT, RUNS>(offT, s, laneOffT, baseT, rsrc4, xr); };
    f32x4 acc[CT][IT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const float b1 = p.bias[(w.cc * CT + ct) * 16 + w.li] * accScale;
#pragma unroll
      for (int ti = 0; ti < IT; ++ti) acc[ct][ti] = f32x4{b1, b1, b1, b1};
    }
    const u32x4* __restrict__ wl = reinterpret_cast<const u32x4*>(ldsW) + (size_t)(w.cc * CT) * 128 + lane;
    const int wStep = CTs * 128;                                        // u32x4 per step
    issue_x(0);
    // The only loads in flight into registers are the operands of ONE step: step s waits for all of them (the previous
    // item's stores may still be on their way, which only makes the first wait stricter), splits them and issues step
    // s + 1's into the same registers, under its 72 matrix instructions
    int s = 0;
    do {
      u32x4 bw[2][2];
      bw[0][0] = wl[0]; bw[0][1] = wl[64];
      split_wait<0>(xr);
      f16x8 a1[IT], a2[IT];
#pragma unroll
      for (int ti = 0; ti < IT; ++ti) {
        if (NCHW_VAR & 8) {
          a1[ti] = __builtin_bit_cast(f16x8, xr[ti][0]);
          a2[ti] = a1[ti];
        } else {
          bool out = false;
#pragma unroll
          for (int j = 0; j < 8; ++j) out |= !(__builtin_fabsf(xr[ti][j >> 2][j & 3]) <= QK_F16_XMAX);
          bad[ti] |= __builtin_amdgcn_ballot_w64(out);
          split_f16x8(xr[ti], a1[ti], a2[ti]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      issue_x(s + 1);                                                   // (the last step: the window's last element again, never used)
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        if (ct + 1 < CT) { bw[(ct + 1) & 1][0] = wl[(ct + 1) * 128]; bw[(ct + 1) & 1][1] = wl[(ct + 1) * 128 + 64]; }
        const f16x8 b1 = __builtin_bit_cast(f16x8, bw[ct & 1][0]), b2 = __builtin_bit_cast(f16x8, bw[ct & 1][1]);
#define SPLIT_TERM(A, B)                                                                                               \
  _Pragma("unroll") for (int ti = 0; ti < IT; ++ti)                                                                    \
    if (NCHW_VAR & 2) asm volatile("" : "+v"(acc[ct][ti]) : "v"(A[ti]), "v"(B)); else                                  \
    acc[ct][ti] = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[ti], B, acc[ct][ti], 0, 0, 0);
        SPLIT_TERM(a2, b1) SPLIT_TERM(a1, b2) SPLIT_TERM(a1, b1)
#undef SPLIT_TERM
        __builtin_amdgcn_sched_barrier(0);
      }
      wl += wStep;
    } while (++s < steps);
    split_wait<0>(xr);                                                  // nothing in flight into registers the stores may reuse
    nchw_store<CT, IT, true>(p, w, acc, outScale);
    // the item's image mask: lane (li, kq) of tile ti is image 8 (ti & 1) + (li & 7) at position 2 (ti >> 1) + (li >> 3)
    unsigned mask = 0;
#pragma unroll
    for (int ti = 0; ti < IT; ++ti) {
      const unsigned long long m = bad[ti] & __builtin_amdgcn_ballot_w64(w.ocol + 2 * (ti >> 1) + (w.li >> 3) < p.Wo);
      unsigned f = (unsigned)m | (unsigned)(m >> 32);
      f |= f >> 16;
      mask |= ((f | (f >> 8)) & 0xffu) << (8 * (ti & 1));
    }
    const int liveImgs = p.nImages - (int)w.img0;                       // a ragged last panel: image tiles past the batch
    mask &= liveImgs >= 16 ? 0xffffu : liveImgs > 0 ? (1u << liveImgs) - 1u : 0u;
    if (lane == 0) {
      masks[item] = (uint16_t)mask;
      if (mask) *guard = epoch;
    }
   };
    if (w.edge) body(std::true_type{}); else body(std::false_type{});
  }
}

// The layer's scale in front of its fp16 planes: out[0] = Sw (qk_f16_weight_scale; 0: the layer keeps the bf16 form), from the
// largest |code word| any assignment of the layer names and the largest |bias|.  One workgroup, a fixed reduction tree.
__global__ __launch_bounds__(1024) void k_f16_weight_scale(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd,
                                                           const float* __restrict__ bias, float* __restrict__ out, QkSlots sl,
                                                           int knl, int Cin, int K, int Ct) {
  __shared__ uint32_t red[2][1024];
  uint32_t mw = 0, mb = 0;
  const int total = Cin * knl * knl * Ct;
  for (int i = threadIdx.x; i < total; i += 1024) {
    const int ch = i % Ct, k = i / Ct;
    mw = max(mw, __builtin_bit_cast(uint32_t, code_word(rows, ctrd, sl, knl, K, k / (knl * knl), (k / knl) % knl, k % knl, ch)) & 0x7fffffffu);
  }
  for (int i = threadIdx.x; i < Ct; i += 1024) mb = max(mb, __builtin_bit_cast(uint32_t, bias[i]) & 0x7fffffffu);
  red[0][threadIdx.x] = mw; red[1][threadIdx.x] = mb;
  __syncthreads();
  for (int n = 512; n > 0; n >>= 1) {
    if ((int)threadIdx.x < n) {
      red[0][threadIdx.x] = max(red[0][threadIdx.x], red[0][threadIdx.x + n]);
      red[1][threadIdx.x] = max(red[1][threadIdx.x], red[1][threadIdx.x + n]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = qk_f16_weight_scale(red[0][0], red[1][0]);
}

// The fp16 planes of k_conv_dec_nchw_f16: w1 = f16(Sw w), w2 = f16(Sw w - w1) in k_decode_weights_split's
// [step][S / 16][piece][64 lanes][8] order (nr as there); scale[0] = Sw, 0: zeros (the layer is not eligible)
__global__ void k_decode_weights_f16(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd, const float* __restrict__ scale,
                                     uint16_t* __restrict__ out, QkSlots sl, int knl, int Cin, int K, int Ct, int Kb, int S, int nr) {
  const int total = Kb * S, CTs = S / 16;
  const float Sw = scale[0];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int j = i & 7, ln = (i >> 3) & 63, tile = (i >> 9) % CTs, step = (i >> 9) / CTs;
    const int ch = 16 * tile + (ln & 15), k = 32 * step + 8 * (ln >> 4) + j;
    float w = 0.0f;
    int kw = k % knl, kh = (k / knl) % knl, c = k / (knl * knl);
    bool live = k < Cin * knl * knl;
    if (nr) {
      const int r = k >> 2, ri = r % nr;
      kw = min(4 * ri, knl - 4) + (k & 3); kh = (r / nr) % knl; c = r / (nr * knl);
      live = r < Cin * knl * nr && kw >= 4 * ri;
    }
    if (ch < Ct && live && Sw != 0.0f) w = code_word(rows, ctrd, sl, knl, K, c, kh, kw, ch) * Sw;
    const _Float16 h1 = (_Float16)w, h2 = (_Float16)(w - (float)h1);
    const size_t blk = (size_t)(step * CTs + tile) * 2 * 512 + ln * 8 + j;
    out[blk] = __builtin_bit_cast(uint16_t, h1);
    out[blk + 512] = __builtin_bit_cast(uint16_t, h2);
  }
}

// ------------------------------------------------------------------------------------------------------------------
// FC layers whose sub-spaces have ONE dim (a 1000-way classifier behind 4096 features: AlexNet / VGG-16 fc8, 16 code
// words of one float each): a look-up there stands for one multiply-add, so the table build — 4096 sub-spaces x 16 code
// words x 128 images per panel — is pure overhead.  out[c] = bias[c] + sum_k x[k] * w[k][c], w[k][c] = ctrd[k][asmt[k][c]].
//
// A workgroup = 64 channels x 64 images of one panel x one slice of the k axis; its 16 waves take 16 sub-slices, each
// with a 4 x 4 block of accumulator tiles fed by ONE dwordx4 of code words (channel tile t = the channels 4 i + t) and
// ONE dwordx4 of activations (image tile t = the images 4 i + t) per four k; the 16 partial blocks are added through LDS
// in a fixed tree (w + (w + 8), then + 4, + 2, + 1).  gridDim.z > 1: k slices over workgroups too, partial sums to
// scratch for k_sum_partials (few panels: one GPU's share of a sharded batch).
__global__ __launch_bounds__(1024) void k_fc_dec(FcDecParams p) {
  extern __shared__ __attribute__((aligned(16))) float ldsR[];          // 8 waves x 16 tiles x 256 floats
  const int lane = threadIdx.x & 63, wave = uni(threadIdx.x >> 6);
  const int li = lane & 15, kq = lane >> 4;
  const int cb = blockIdx.x, half = blockIdx.y % p.halves, panel = blockIdx.y / p.halves, z = blockIdx.z;
  const int steps = p.D / (4 * 16 * (int)gridDim.z);                    // steps of four k per wave
  const int k0 = (z * 16 + wave) * steps * 4;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.wdec), 0, (unsigned)((size_t)p.D * p.S * sizeof(float)), 0x00020000);
  const float* __restrict__ xb = p.src + (size_t)panel * p.D * PANEL;
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(xb), 0, (unsigned)((size_t)p.D * PANEL * sizeof(float)), 0x00020000);
  const int aLane = (kq * p.S + cb * 64 + 4 * li) * (int)sizeof(float);
  const int bLane = (kq * PANEL + half * 64 + 4 * li) * (int)sizeof(float);
  const int aStep = 4 * p.S * (int)sizeof(float), bStep = 4 * PANEL * (int)sizeof(float);
  f32x4 acc[4][4];                                                      // [channel tile][image tile]
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int ti = 0; ti < 4; ++ti) acc[ct][ti] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  constexpr int R = 3;
  f32x4 a[R], b[R];
  int aoff = k0 * p.S * (int)sizeof(float), boff = k0 * PANEL * (int)sizeof(float);
  auto next = [&](f32x4& aa, f32x4& bb) {                               // past the slice: rows of the next slice, never multiplied
    aa = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ra, aLane, aoff, 0));
    bb = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, bLane, boff, 0));
    aoff += aStep; boff += bStep;
  };
  auto products = [&](const f32x4& aa, const f32x4& bb) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int ti = 0; ti < 4; ++ti) acc[ct][ti] = __builtin_amdgcn_mfma_f32_16x16x4f32(aa[ct], bb[ti], acc[ct][ti], 0, 0, 0);
  };
#pragma unroll
  for (int u = 0; u < R; ++u) next(a[u], b[u]);
  int t = 0;
  for (; t + R <= steps; t += R) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      products(a[u], b[u]);
      __builtin_amdgcn_sched_barrier(0);
      next(a[u], b[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < R - 1; ++u)
    if (t + u < steps) products(a[u], b[u]);
  // fixed-order tree over the 16 waves
  f32x4* lds4 = reinterpret_cast<f32x4*>(ldsR);
#pragma unroll
  for (int stride = 8; stride >= 1; stride >>= 1) {
    if (wave >= stride && wave < 2 * stride) {
#pragma unroll
      for (int i = 0; i < 16; ++i) lds4[((wave - stride) * 16 + i) * 64 + lane] = acc[i >> 2][i & 3];
    }
    __syncthreads();
    if (wave < stride) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const f32x4 v = lds4[(wave * 16 + i) * 64 + lane];
        acc[i >> 2][i & 3] += v;
      }
    }
    __syncthreads();
  }
  if (wave != 0) return;
  // tile ct, row 4 kq + r: channel 64 cb + 4 (4 kq + r) + ct; tile ti, column li: image 64 half + 4 li + ti
  float* __restrict__ out = (gridDim.z > 1 ? p.partial + (size_t)z * p.panels * p.Ct * PANEL : p.dst) +
                            (size_t)panel * p.Ct * PANEL + half * 64 + 4 * li;
  const bool first = z == 0;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int ch = cb * 64 + 4 * (4 * kq + r) + ct;
      if (ch < p.Ct) {
        const float bv = first ? p.bias[ch] : 0.0f;
        f32x4 v = {acc[ct][0][r] + bv, acc[ct][1][r] + bv, acc[ct][2][r] + bv, acc[ct][3][r] + bv};
        if (p.relu && gridDim.z == 1) {
          v[0] = (0.0f < v[0]) ? v[0] : 0.0f; v[1] = (0.0f < v[1]) ? v[1] : 0.0f;
          v[2] = (0.0f < v[2]) ? v[2] : 0.0f; v[3] = (0.0f < v[3]) ? v[3] : 0.0f;
        }
        *reinterpret_cast<f32x4*>(out + (size_t)ch * PANEL) = v;
      }
    }
}

// rows: [M = D][rowStride] slot bytes (QkSlots order); ctrd: [M][1][K]; out: [D][S]
__global__ void k_decode_fc_weights(const uint8_t* __restrict__ rows, const float* __restrict__ ctrd, float* __restrict__ out,
                                    QkSlots sl, int D, int K, int Ct, int S) {
  const int G = qcnn_stage_group(K);
  const size_t total = (size_t)D * S;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int ch = (int)(i % S), k = (int)(i / S);
    float w = 0.0f;
    if (ch < Ct) {
      const int slot = rows[(size_t)k * sl.rowStride + qk_slot_entry(sl, 0, ch)];
      w = ctrd[(size_t)k * K + (qcnn_row_slot(slot) - (k % G) * K)];    // stage row = (m % G) * K + code word
    }
    out[i] = w;
  }
}

}  // namespace

bool qk_conv_dec_shape(int Cin, int grp, int M, int Ct, int knl, int* Kp, int* S) {
  if (grp != 1 || M != 1 || Cin < 1 || Cin > 4) return false;
  if (Ct < 32 || Ct % 32) return false;                   // a wave owns 32, 64 or 96 channels
  const int kp = (knl * Cin + 3) / 4 * 4;
  // channel stride: four consecutive k rows of 16 channels on distinct banks (stride = 16 or 48 mod 64) when all code
  // words still fit the LDS that way, else dense rows (AlexNet conv1: 11 x 36 x 96 floats = 152 KB; its A reads then are
  // two-way bank conflicts, 8 instead of 4 LDS cycles per ds_read2_b32 — a sixth of the LDS pipe)
  const size_t lim = 160 * 1024;
  int s = Ct;
  while ((s & 63) != 16 && (s & 63) != 48) s += 16;
  if ((size_t)knl * kp * s * sizeof(float) > lim) s = Ct;
  if ((size_t)knl * kp * s * sizeof(float) > lim) return false;
  *Kp = kp; *S = s;
  return true;
}

hipError_t qk_decode_weights(const uint8_t* rows, const float* ctrd, float* out, const QkSlots& sl, int knl, int Cin, int K,
                             int Ct, int Kp, int S, hipStream_t st) {
  const int total = knl * Kp * S;
  hipLaunchKernelGGL(k_decode_weights, dim3((total + 255) / 256), dim3(256), 0, st, rows, ctrd, out, sl, knl, Cin, K, Ct, Kp, S);
  return hipGetLastError();
}

hipError_t qk_conv_dec(const DecParams& p, hipStream_t st) {
  if ((long long)p.H * p.W * p.Cin * QCNN_PANEL * 4 >= (1ll << 31)) return hipErrorInvalidValue;   // 32-bit BYTE offsets inside a panel
  if (p.Ct % 32) return hipErrorInvalidValue;
  // channels per wave x positions per wave x operand sets in flight x image tiles: as many accumulator tiles as 128
  // registers hold, all channels in one wave where they fit (a chunk of the channels = the B rows loaded once more)
  const bool clamped = p.pad || p.Kr < 4;     // per-lane window clamps: padded layers, and kernel rows of fewer than four products
  if (p.live <= 16) {               // at most one image tile: 16-image items (four positions of 32 channels for padded layers)
    if (clamped) return launch_dec<2, 4, true, 2, 1>(p, st);
    if (p.Ct % 96 == 0) return launch_dec<6, 2, false, 3, 1>(p, st);
    if (p.Ct % 64 == 0) return launch_dec<4, 4, false, 3, 1>(p, st);
    return launch_dec<2, 6, false, 3, 1>(p, st);
  }
  if (clamped) {
    if (p.Ct % 64 == 0) return launch_dec<4, 1, true, 2, 4>(p, st);
    return launch_dec<2, 1, true, 3, 4>(p, st);
  }
  if (p.Ct % 96 == 0) {
    // a launch of a few thousand 96-channel items (one panel: 6050 on 4096 waves = two rounds for 1.5 rounds of work) runs
    // half-items of 48 channels instead (three rounds of half the length; B rows loaded twice)
    const long long items = (long long)p.panels * p.Ho * p.Wo * ((p.live + 63) / 64) * (p.Ct / 96);
    if (items > 4096 && items < 2 * 4096) return launch_dec<3, 1, false, 3, 4>(p, st);
    return launch_dec<6, 1, false, 2, 4>(p, st);
  }
  if (p.Ct % 64 == 0) return launch_dec<4, 1, false, 3, 4>(p, st);
  return launch_dec<2, 2, false, 3, 4>(p, st);
}

hipError_t qk_decode_fc_weights(const uint8_t* rows, const float* ctrd, float* out, const QkSlots& sl, int D, int K, int Ct,
                                int S, hipStream_t st) {
  hipLaunchKernelGGL(k_decode_fc_weights, dim3(2048), dim3(256), 0, st, rows, ctrd, out, sl, D, K, Ct, S);
  return hipGetLastError();
}

hipError_t qk_fc_dec(const FcDecParams& p, int slices, int live, hipStream_t st) {
  if (p.D % (64 * slices)) return hipErrorInvalidValue;
  FcDecParams q = p;
  q.halves = (live + 63) / 64;
  const dim3 grid((unsigned)((p.Ct + 63) / 64), (unsigned)(p.panels * q.halves), (unsigned)slices);
  return launch_lds(k_fc_dec, grid, dim3(1024), 8 * 16 * 256 * sizeof(float), st, q);
}

bool qk_conv_dec_nchw_shape(int Cin, int grp, int M, int Ct, int knl, int pad, int* Kp) {
  if (grp != 1 || M != 1 || Cin < 1 || Cin > 4 || pad != 0 || Ct % 96) return false;
  const int kp = (Cin * knl * knl + 15) / 16 * 16;            // steps in fours
  if ((size_t)(kp + 4) * Ct * sizeof(float) + (kp / 4 + 4) * 16 > 160 * 1024) return false;   // code words + one step of slack + offset table
  *Kp = kp;
  return true;
}

hipError_t qk_decode_weights_nchw(const uint8_t* rows, const float* ctrd, float* out, const QkSlots& sl, int knl, int Cin, int K,
                                  int Ct, int Kp, int S, hipStream_t st) {
  const int total = Kp * S;
  hipLaunchKernelGGL(k_decode_weights_nchw, dim3((total + 255) / 256), dim3(256), 0, st, rows, ctrd, out, sl, knl, Cin, K, Ct, Kp / 4, S);
  return hipGetLastError();
}

// The checks of both NCHW kernels' launches (an NCHW batch whose byte offsets fit 32 bits, an unpadded layer, 96-channel
// chunks, S = Ct) and their grid: one persistent workgroup per CU, fewer for few items (one each, see xcd_items)
static hipError_t launch_nchw(void (*kern)(DecParams), size_t shm, const DecParams& p, hipStream_t st) {
  if (!p.srcNchw || p.pad != 0 || p.Ct % 96 || p.S != p.Ct || (unsigned long long)p.nImages * p.Cin * p.H * p.W * 4ull >= (1ull << 32))
    return hipErrorInvalidValue;
  const long long items = (long long)p.panels * p.Ho * ((p.Wo + 3) / 4) * ((p.live + 15) / 16) * (p.Ct / 96);
  return launch_lds(kern, dim3((int)std::min<long long>(256, items)), dim3(64 * NCHW_WAVES), shm, st, p);
}

// p.Kr = Cin knl^2, p.Kp = qk_conv_dec_nchw_shape's, p.S = Ct
hipError_t qk_conv_dec_nchw(const DecParams& p, hipStream_t st) {
  return launch_nchw(k_conv_dec_nchw<6, 4>, (size_t)(p.Kp + 4) * p.S * sizeof(float) + (size_t)(p.Kp / 4 + 4) * 16, p, st);
}

bool qk_conv_dec_nchw_split_shape(int Cin, int grp, int M, int Ct, int knl, int pad, int* Kb) {
  int kp = 0;
  if (!qk_conv_dec_nchw_shape(Cin, grp, M, Ct, knl, pad, &kp)) return false;
  const int nr = nchw_split_runs(Cin, knl, Ct);               // run order where it fits, else flat
  const int kb = nchw_split_kb(Cin, knl, nr);                 // steps of 32 k
  if (nchw_split_lds(kb, Ct, nr) > 160 * 1024) return false;  // w1 / w2 + offset table
  *Kb = kb;
  return true;
}

hipError_t qk_decode_weights_split(const uint8_t* rows, const float* ctrd, uint16_t* out, const QkSlots& sl, int knl, int Cin, int K,
                                   int Ct, int Kb, hipStream_t st) {
  const int total = Kb * Ct;
  const int nr = nchw_split_runs(Cin, knl, Ct);
  if (Kb != nchw_split_kb(Cin, knl, nr)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_decode_weights_split, dim3((total + 255) / 256), dim3(256), 0, st, rows, ctrd, out, sl, knl, Cin, K, Ct, Kb, Ct, nr);
  return hipGetLastError();
}

// p.Kr = Cin knl^2, p.Kp = qk_conv_dec_nchw_split_shape's Kb, p.S = Ct, p.wdec = qk_decode_weights_split's planes
hipError_t qk_conv_dec_nchw_split(const DecParams& p, hipStream_t st) {
  const int nr = nchw_split_runs(p.Cin, p.knl, p.Ct);         // the order qk_decode_weights_split wrote
  if (p.Kp != nchw_split_kb(p.Cin, p.knl, nr)) return hipErrorInvalidValue;
  return launch_nchw(nr ? k_conv_dec_nchw_split<6, 4, true> : k_conv_dec_nchw_split<6, 4, false>, nchw_split_lds(p.Kp, p.S, nr), p, st);
}

size_t qk_conv_dec_nchw_f16_bytes(int Kb, int Ct) { return QK_F16_PLANES + (size_t)Kb * Ct * 4; }

size_t qk_conv_dec_nchw_f16_guard_bytes(int Ho, int Wo, int Ct, int panels) {   // word + slack, then a mask per item of `panels` full panels
  return 16 + (size_t)panels * Ho * ((Wo + 3) / 4) * (QCNN_PANEL / 16) * (Ct / 96) * sizeof(uint16_t);
}

hipError_t qk_decode_weights_f16(const uint8_t* rows, const float* ctrd, const float* bias, void* out, const QkSlots& sl, int knl,
                                 int Cin, int K, int Ct, int Kb, hipStream_t st) {
  const int total = Kb * Ct;
  const int nr = nchw_split_runs(Cin, knl, Ct);
  if (Kb != nchw_split_kb(Cin, knl, nr)) return hipErrorInvalidValue;
  float* scale = static_cast<float*>(out);
  hipLaunchKernelGGL(k_f16_weight_scale, dim3(1), dim3(1024), 0, st, rows, ctrd, bias, scale, sl, knl, Cin, K, Ct);
  hipLaunchKernelGGL(k_decode_weights_f16, dim3((total + 255) / 256), dim3(256), 0, st, rows, ctrd, scale,
                     reinterpret_cast<uint16_t*>(static_cast<char*>(out) + QK_F16_PLANES), sl, knl, Cin, K, Ct, Kb, Ct, nr);
  return hipGetLastError();
}

// p: as for qk_conv_dec_nchw_split, with p.wdec = the fp16 planes (behind the scale), p.accScale = Sx Sw, p.outScale = its inverse,
// p.guard / p.epoch = this launch's guard region and a number no earlier launch on that region carried; wBf16 = the planes of
// qk_decode_weights_split for the fix-up launch
hipError_t qk_conv_dec_nchw_f16(const DecParams& p, const float* wBf16, hipStream_t st) {
  const int nr = nchw_split_runs(p.Cin, p.knl, p.Ct);
  if (p.Kp != nchw_split_kb(p.Cin, p.knl, nr) || !p.guard || !p.epoch) return hipErrorInvalidValue;
  const size_t shm = nchw_split_lds(p.Kp, p.S, nr);
  const hipError_t e = launch_nchw(nr ? k_conv_dec_nchw_f16<6, 4, true> : k_conv_dec_nchw_f16<6, 4, false>, shm, p, st);
  if (e != hipSuccess || (NCHW_VAR & 32)) return e;
  DecParams q = p;
  q.wdec = wBf16;
  return launch_nchw(nr ? k_conv_dec_nchw_fixup<6, 4, true> : k_conv_dec_nchw_fixup<6, 4, false>, shm, q, st);
}
