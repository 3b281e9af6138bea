// The pack kernels' shared pieces (qcnn_glue.hip has the story): the LDS tile's write-out, the wave-uniform slot walk, the
// reference's bilinear resize as taps + value, the tap loads of every source layout, the two resizing pack kernels as templates
// over the descriptor type, and their launchers.  NO include guard, NO namespace and NO #include of its own: the file is included
// inside the anonymous namespace of a translation unit that has included qcnn_kernels.h and <limits.h> and defined
// the vector type f32x2 and `constexpr int PANEL = QCNN_PANEL;` — qcnn_glue.hip (planar and strided instantiations) and qcnn_glue_yuv.hip (YCbCr).  Two
// units because a code object is loaded whole: the YCbCr kernels are 230 KB that a process which never reads a YCbCr frame then
// never loads, and the code object of qcnn_glue.hip — ReLU, LRN, pool, soft-max, top-5, the pack kernels of the forward pass —
// stays the size it had.
// ---- the pack kernels: rows or 8-bit images -> panels [E][128] through a 128-slot x 64-element LDS tile (both sides
// coalesced).  One block = 64 elements of one panel; wave w fills tile rows w, w + 4, ...; the shared pieces first. ----
// The tile's write-out: element e0 + j of all 128 slots goes to panel row rowOf(e0 + j), two slots a lane.  rowOf is called
// before the tile is read and its result converted to the row behind the reads: what a mapping does where is its own choice.
template <class RowOf>
__device__ __forceinline__ void tile_write_out(const float (&tile)[PANEL][65], float* __restrict__ dst, int panel, int e0, int E,
                                               int lane, int wave, RowOf rowOf) {
  for (int j = wave; j < 64; j += 4) {
    const int e = e0 + j;
    if (e < E) {
      const auto row = rowOf(e);
      *reinterpret_cast<f32x2*>(dst + ((size_t)panel * E + (size_t)row) * PANEL + 2 * lane) =
          f32x2{tile[2 * lane][j], tile[2 * lane + 1][j]};
    }
  }
}

// NCHW: input element e = (c*H + h)*W + w of an image lands in row (h*W + w)*C + c (src/CaffeEva.cc:1146-1160).  The division
// is done at the call, the 64-bit product at the conversion: the tile's reads are issued between the two.
struct NchwRow {
  int C, HW;
  struct Row { int c, hw, C; __device__ __forceinline__ explicit operator size_t() const { return (size_t)hw * C + c; } };
  __device__ __forceinline__ Row operator()(int e) const { return Row{e / HW, e % HW, C}; }
};

// The slots of a multi-view panel as one wave meets them: S = n * V batch slots, slot s = view s % V of image s / V; the wave
// starts at slot `first` = panel * 128 + wave and its next slot is four further: q4 images and r4 views, without a division
// per slot.  Everything here is wave-uniform (`wave` is readfirstlane'd by the kernels): image, view and what is read under
// them — descriptor, view entry — live in scalar registers and come through scalar loads.  vw < V <= QK_MAX_VIEWS also for
// the dead slots of a ragged panel, so the view table is never read outside.  next() wraps by two selects, no branch.
struct SlotWalk {
  int q4, r4, img, vw, V, first, S;
  __device__ __forceinline__ SlotWalk(int panel, int wave, int V_, int S_)       // in this order: q4 and r4 are worked out first
      : q4(4 / V_), r4(4 % V_), img((panel * PANEL + wave) / V_), vw((panel * PANEL + wave) % V_), V(V_), first(panel * PANEL + wave), S(S_) {}
  __device__ __forceinline__ void next() {
    img += q4;
    vw += r4;
    const bool wrap = vw >= V;
    vw -= wrap ? V : 0;
    img += wrap;
  }
  __device__ __forceinline__ bool live(int k) const { return first + 4 * k < S; }     // the wave's k-th slot exists
};

// The reference's bilinear resize (BmpImgIO::ReszImg, src/BmpImgIO.cc:105-178) of one value: pixel (Y, X) of channel ch of the
// resized image from the four 8-bit taps of the h x w source at in + off, in the reference's fp32 sequence with one rounding per
// operation (the build has -ffp-contract=off; the intrinsics say it again):
//   yc = sy * (float)Y;  y0 = max(0, (int)yc);  y1 = min(h - 1, y0 + 1);  wy0 = 1 - (yc - (float)y0);  wy1 = 1 - ((float)y1 - yc)
//   the columns likewise;  w00 = wy0 * wx0 ... w11 = wy1 * wx1
//   (((p00 * w00 + p01 * w01) + p10 * w10) + p11 * w11) / (((w00 + w01) + w10) + w11)
// yc is the float PRODUCT (for some sizes it lands just under or over an integer it equals mathematically: that moves y0 and
// gives weights like 1 - eps or above 1), and the division is no no-op (y1 clamped to y0 at the last row: both row weights
// about 1).  y0 is clamped to h - 1 as well: it cannot exceed it while h - 1 < 2^23, and beyond that the clamp keeps the taps
// inside the image.  Offsets inside an image are 32-bit: C * h * w <= INT_MAX (the engine refuses images of 2 GiB and more).
// bilinear_taps issues the four loads and waits for none (base and offset come apart: the image's 64-bit address is formed
// behind the weights, next to the loads that use it); bilinear_value is the arithmetic on what they brought.
struct BilinearTaps {
  float w00, w01, w10, w11;
  uint8_t p00, p01, p10, p11;
};
// The taps of a YCbCr frame (QkSrcYuv / QkRelaxedYuv) while their loads are in flight: the three bytes of each tap as loaded,
// and what the conversion of the thread's own channel needs besides — v = (Y - y0) * ky + kcb * (Cb - 128) + kcr * (Cr - 128),
// (kcb, kcr) = (cbu, 0) for B, (-cbg, -crg) for G, (0, crv) for R.  converted() is the arithmetic on what the loads brought:
// the 8-bit channel values in a BilinearTaps, which bilinear_value takes as it takes every other source's.
struct YuvTaps {
  float w00, w01, w10, w11;
  uint8_t y00, y01, y10, y11, b00, b01, b10, b11, r00, r01, r10, r11;
  int y0, ky, kcb, kcr;
};
__device__ __forceinline__ uint8_t yuv_channel(const YuvTaps& t, int Y, int Cb, int Cr) {
  const int v = ((Y - t.y0) * t.ky + t.kcb * (Cb - 128) + t.kcr * (Cr - 128) + 32768) >> 16;
  return (uint8_t)min(max(v, 0), 255);
}
__device__ __forceinline__ BilinearTaps converted(const YuvTaps& t) {
  return BilinearTaps{t.w00, t.w01, t.w10, t.w11, yuv_channel(t, t.y00, t.b00, t.r00), yuv_channel(t, t.y01, t.b01, t.r01),
                      yuv_channel(t, t.y10, t.b10, t.r10), yuv_channel(t, t.y11, t.b11, t.r11)};
}
// WHERE the four taps lie is the layout's (tap_loads): planar [C][h][w] for QkSrcImage / QkRelaxedImage, the strides of a
// QkLayout for the strided descriptors.  Either way the image's part — base, sizes, strides, channel offsets — is wave-uniform
// and scalar, the thread's part a 32-bit offset, and the loads are unconditional.
__device__ __forceinline__ void tap_loads(BilinearTaps& t, const uint8_t* px, int h, int w, unsigned ch, int y0, int y1, int x0,
                                          int x1) {
  const unsigned r0 = (ch * h + y0) * w, r1 = (ch * h + y1) * w;
  t.p00 = px[r0 + x0]; t.p01 = px[r0 + x1]; t.p10 = px[r1 + x0]; t.p11 = px[r1 + x1];
}
// QK_STRIDED_VAR (LABBOOK.md, "Source layouts"; timing only, results wrong but for planar descriptors under bit 2): 1 = the
// strided kernels without the channel select, 2 = with the planar address arithmetic on their 48- / 56-byte descriptors.
#ifndef QK_STRIDED_VAR
#define QK_STRIDED_VAR 0
#endif
// Strided: y * rs + x * ps + co[ch] modulo 2^32, read as an int (qcnn_kernels.h, QkLayout: the true sum is one).  ch is the
// thread's own: it picks among the four uniform channel offsets by selects.
__device__ __forceinline__ void tap_loads(BilinearTaps& t, const uint8_t* px, const QkLayout& l, unsigned ch, int y0, int y1,
                                          int x0, int x1) {
  // The four fields are read first, unconditionally, and each select picks between two VALUES: a conditional whose arms read
  // the fields becomes one read at a selected address, and the descriptor is then copied to scratch to be indexed there.
  const unsigned a0 = l.c0, a1 = l.c1, a2 = l.c2, a3 = l.c3;
  unsigned co = a3;
  co = ch == 2 ? a2 : co;
  co = ch == 1 ? a1 : co;
  co = ch == 0 ? a0 : co;
#if QK_STRIDED_VAR & 1
  co = a0;                                          // timing only: no channel select
#endif
  const unsigned r0 = (unsigned)y0 * (unsigned)l.rs + co, r1 = (unsigned)y1 * (unsigned)l.rs + co;
  const unsigned c0 = (unsigned)x0 * (unsigned)l.ps, c1 = (unsigned)x1 * (unsigned)l.ps;
  t.p00 = px[(int)(r0 + c0)]; t.p01 = px[(int)(r0 + c1)]; t.p10 = px[(int)(r1 + c0)]; t.p11 = px[(int)(r1 + c1)];
}
// What a pack kernel asks of its descriptor type D: the image part (offset, sizes, scales) and the taps' loads.
__device__ __forceinline__ const QkSrcImage& image_of(const QkSrcImage& d) { return d; }
__device__ __forceinline__ const QkSrcImage& image_of(const QkSrcPixels& d) { return d.img; }
__device__ __forceinline__ const QkRelaxedImage& image_of(const QkRelaxedImage& d) { return d; }
__device__ __forceinline__ const QkRelaxedImage& image_of(const QkRelaxedPixels& d) { return d.img; }
__device__ __forceinline__ void tap_loads(BilinearTaps& t, const uint8_t* px, const QkSrcImage& d, unsigned ch, int y0, int y1,
                                          int x0, int x1) { tap_loads(t, px, d.h, d.w, ch, y0, y1, x0, x1); }
__device__ __forceinline__ void tap_loads(BilinearTaps& t, const uint8_t* px, const QkRelaxedImage& d, unsigned ch, int y0, int y1,
                                          int x0, int x1) { tap_loads(t, px, d.h, d.w, ch, y0, y1, x0, x1); }
#if QK_STRIDED_VAR & 2
#define QK_STRIDED_TAPS(d) tap_loads(t, px, d.img.h, d.img.w, ch, y0, y1, x0, x1)
#else
#define QK_STRIDED_TAPS(d) tap_loads(t, px, d.lay, ch, y0, y1, x0, x1)
#endif
__device__ __forceinline__ void tap_loads(BilinearTaps& t, const uint8_t* px, const QkSrcPixels& d, unsigned ch, int y0, int y1,
                                          int x0, int x1) { QK_STRIDED_TAPS(d); }
__device__ __forceinline__ void tap_loads(BilinearTaps& t, const uint8_t* px, const QkRelaxedPixels& d, unsigned ch, int y0, int y1,
                                          int x0, int x1) { QK_STRIDED_TAPS(d); }
// YCbCr: three unconditional byte loads a tap — Y at y * yrs + x * yps, Cb and Cr at (y >> sy) * crs + (x >> sx) * cps from their
// bases (chroma replicated) — every sum modulo 2^32, read as an int (qcnn_kernels.h, QkYuvLayout).  The layout is wave-uniform;
// the thread's own channel picks its two chroma coefficients by selects between VALUES, as the strided tap_loads picks its offset.
__device__ __forceinline__ void tap_loads(YuvTaps& t, const uint8_t* px, const QkYuvLayout& l, unsigned ch, int y0, int y1, int x0,
                                          int x1) {
  const int cbu = l.cbu, cbg = l.cbg, crg = l.crg, crv = l.crv;
  t.y0 = l.y0; t.ky = l.ky;
  t.kcb = ch == 0 ? cbu : (ch == 1 ? -cbg : 0);
  t.kcr = ch == 0 ? 0 : (ch == 1 ? -crg : crv);
  const unsigned r0 = (unsigned)y0 * (unsigned)l.yrs, r1 = (unsigned)y1 * (unsigned)l.yrs;
  const unsigned c0 = (unsigned)x0 * (unsigned)l.yps, c1 = (unsigned)x1 * (unsigned)l.yps;
  const unsigned q0 = (unsigned)(y0 >> l.sy) * (unsigned)l.crs, q1 = (unsigned)(y1 >> l.sy) * (unsigned)l.crs;
  const unsigned k0 = (unsigned)(x0 >> l.sx) * (unsigned)l.cps, k1 = (unsigned)(x1 >> l.sx) * (unsigned)l.cps;
  const unsigned cb = (unsigned)l.dcb, cr = (unsigned)l.dcr;
  t.y00 = px[(int)(r0 + c0)]; t.y01 = px[(int)(r0 + c1)]; t.y10 = px[(int)(r1 + c0)]; t.y11 = px[(int)(r1 + c1)];
  t.b00 = px[(int)(cb + q0 + k0)]; t.b01 = px[(int)(cb + q0 + k1)]; t.b10 = px[(int)(cb + q1 + k0)]; t.b11 = px[(int)(cb + q1 + k1)];
  t.r00 = px[(int)(cr + q0 + k0)]; t.r01 = px[(int)(cr + q0 + k1)]; t.r10 = px[(int)(cr + q1 + k0)]; t.r11 = px[(int)(cr + q1 + k1)];
}
__device__ __forceinline__ const QkSrcImage& image_of(const QkSrcYuv& d) { return d.img; }
__device__ __forceinline__ const QkRelaxedImage& image_of(const QkRelaxedYuv& d) { return d.img; }
__device__ __forceinline__ void tap_loads(YuvTaps& t, const uint8_t* px, const QkSrcYuv& d, unsigned ch, int y0, int y1, int x0,
                                          int x1) { tap_loads(t, px, d.lay, ch, y0, y1, x0, x1); }
__device__ __forceinline__ void tap_loads(YuvTaps& t, const uint8_t* px, const QkRelaxedYuv& d, unsigned ch, int y0, int y1, int x0,
                                          int x1) { tap_loads(t, px, d.lay, ch, y0, y1, x0, x1); }
// What a pack kernel holds of a descriptor type's taps between issuing their loads and using them, and how many slots it takes
// a round.  Eight slots of a YCbCr source would have 8 x 13 loads in flight where the vector-memory counter holds 63: four
// slots a round are 52 (48 and the two mean loads in the relaxed kernel), so every load of a round is still issued before the
// first is waited for.
template <class D> struct PackTaps { using Taps = BilinearTaps; static constexpr int R = 8; };
template <> struct PackTaps<QkSrcYuv> { using Taps = YuvTaps; static constexpr int R = 4; };
template <> struct PackTaps<QkRelaxedYuv> { using Taps = YuvTaps; static constexpr int R = 4; };
template <class T, class D>
__device__ __forceinline__ void bilinear_taps(T& t, float sy, float sx, const D& d, unsigned ch, int Y, int X,
                                              const uint8_t* in) {
  const int h = image_of(d).h, w = image_of(d).w;
  const float yc = __fmul_rn(sy, (float)Y), xc = __fmul_rn(sx, (float)X);
  const int y0 = min(max(0, (int)yc), h - 1), x0 = min(max(0, (int)xc), w - 1);
  const int y1 = min(h - 1, y0 + 1), x1 = min(w - 1, x0 + 1);
  const float wy0 = __fsub_rn(1.0f, __fsub_rn(yc, (float)y0)), wy1 = __fsub_rn(1.0f, __fsub_rn((float)y1, yc));
  const float wx0 = __fsub_rn(1.0f, __fsub_rn(xc, (float)x0)), wx1 = __fsub_rn(1.0f, __fsub_rn((float)x1, xc));
  t.w00 = __fmul_rn(wy0, wx0); t.w01 = __fmul_rn(wy0, wx1); t.w10 = __fmul_rn(wy1, wx0); t.w11 = __fmul_rn(wy1, wx1);
  const uint8_t* px = in + image_of(d).off;
  tap_loads(t, px, d, ch, y0, y1, x0, x1);
}
__device__ __forceinline__ float bilinear_value(const BilinearTaps& t) {
  const float num = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn((float)t.p00, t.w00), __fmul_rn((float)t.p01, t.w01)),
                                        __fmul_rn((float)t.p10, t.w10)), __fmul_rn((float)t.p11, t.w11));
  const float den = __fadd_rn(__fadd_rn(__fadd_rn(t.w00, t.w01), t.w10), t.w11);
  return __fdiv_rn(num, den);
}
__device__ __forceinline__ float tap_value(const BilinearTaps& t) { return bilinear_value(t); }
__device__ __forceinline__ float tap_value(const YuvTaps& t) { return bilinear_value(converted(t)); }


// k_pack_u8_views on source images of any size (qcnn_forward_u8_resized_views): each image RESIZED to Hf x Wf — ReszImg's Strict
// mode, bilinear_taps with the two scales of the image's descriptor (QkSrcImage, from the table the engine staged) — fused into
// the pack: the resized float images are never stored (a thousand 256 x 256 x 3 float images are 786 MB; the panels written
// are already the HBM bound).  A (slot, element) is the resized value at (Y, X), the element's position in the full image —
// view corner + (y, x or the mirrored x) — minus mean[c][Y][X].  Unconditional loads as in k_pack_u8_views (a dead slot reads
// image 0 with image 0's own descriptor): the four tap loads and the mean load of the eight slots of a round, forty per
// thread, are in flight together.
template <bool MEAN, class D>                         // D: QkSrcImage (planar), QkSrcPixels (strided) or QkSrcYuv (YCbCr)
__global__ __launch_bounds__(256) void k_pack_u8_resized(const uint8_t* __restrict__ in, const D* __restrict__ desc,
                                                         const float* __restrict__ mean, float* __restrict__ dst, int S, int V,
                                                         const QkViews views, int C, int H, int W, int Hf, int Wf) {
  __shared__ float tile[PANEL][65];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HW = H * W, E = C * HW;
  const int e0 = blockIdx.x * 64;
  const int panel = blockIdx.y;
  const int e = e0 + lane;
  const int el = e < E ? e : 0;                     // the element whose source positions this thread reads
  const int ch = el / HW, ey = (el % HW) / W;       // its channel and its row in a view
  const int ex0 = el % W, ex1 = W - 1 - el % W;     // its column in a plain / a mirrored view
  SlotWalk s(panel, wave, V, S);
  constexpr int R = PackTaps<D>::R;                 // slots a round
#pragma unroll
  for (int b = 0; b < PANEL / 4; b += R) {
    typename PackTaps<D>::Taps t[R];
    float m[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const bool liveSlot = s.live(b + u);
      const D d = desc[liveSlot ? s.img : 0];
      const QkView q = views.v[s.vw];
      const int Y = q.oy + ey, X = q.ox + (q.flip ? ex1 : ex0);         // < Hf, < Wf: the engine checked the views
      bilinear_taps(t[u], image_of(d).sh, image_of(d).sw, d, ch, Y, X, in);
      m[u] = MEAN ? mean[((unsigned)ch * Hf + Y) * Wf + X] : 0.0f;
      s.next();
    }
    __builtin_amdgcn_sched_barrier(0);              // every load of the round is issued before the first value is waited for
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const bool live = s.live(b + u) && e < E;
      const float val = tap_value(t[u]);
      tile[wave + 4 * (b + u)][lane] = live ? (MEAN ? __fsub_rn(val, m[u]) : val) : 0.0f;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  tile_write_out(tile, dst, panel, e0, E, lane, wave, NchwRow{C, HW});
}

// k_pack_u8_resized for the reference's other pre-processing mode (qcnn_forward_u8_relaxed_views): BmpImgIO::ReszImg Relaxed —
// ONE scale s for both axes, so image i has its own full size hf x wf (both computed by the engine on the host with the
// reference's float sequence and staged with the descriptor, QkRelaxedImage) — then CropImg and a mean of the CROP's size
// (ENUM_MeanType::Crop, src/BmpImgIO.cc:56-64,124-131).  A (slot, element) is the resized value at the full-image position
// (Y, X) = (oy + y, ox + xl), xl = x or the mirrored column, minus mean[c][y][xl]; against the resized kernel:
//   * the view corner is resolved per slot from the view's anchor and ITS image's full size, wave-uniformly, in scalar
//     registers: o = (((full - in) * a) >> 1) + d, which is 0, CropImg's (full - in) / 2 and full - in for a = 0, 1, 2 (full >= in:
//     the engine checked every view against every image);
//   * the mean is indexed by the element alone (view-local position BEFORE mirroring), so its loads leave the slot loop: two
//     per thread per block — the plain and the mirrored column, a slot picks by its wave-uniform flip — where the resized
//     kernel issues one per slot: 32 tap loads a round.
// A dead slot reads image 0 under its view, which the engine checked like every other pair.
template <bool MEAN, class D>                         // D: QkRelaxedImage (planar), QkRelaxedPixels (strided) or QkRelaxedYuv (YCbCr)
__global__ __launch_bounds__(256) void k_pack_u8_relaxed(const uint8_t* __restrict__ in, const D* __restrict__ desc,
                                                         const float* __restrict__ mean, float* __restrict__ dst, int S, int V,
                                                         const QkAnchorViews views, int C, int H, int W) {
  __shared__ float tile[PANEL][65];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int HW = H * W, E = C * HW;
  const int e0 = blockIdx.x * 64;
  const int panel = blockIdx.y;
  const int e = e0 + lane;
  const int el = e < E ? e : 0;                     // the element whose source positions this thread reads
  const int ey = (el % HW) / W;                     // its row in a view
  const int ex0 = el % W, ex1 = W - 1 - el % W;     // its column in a plain / a mirrored view
  const unsigned ch = el / HW;                      // its channel
  const float mPlain = MEAN ? mean[el] : 0.0f;      // mean[c][ey][ex0]: el = (c * H + ey) * W + ex0
  const float mFlip = MEAN ? mean[el - ex0 + ex1] : 0.0f;
  SlotWalk s(panel, wave, V, S);
  constexpr int R = PackTaps<D>::R;                 // slots a round
#pragma unroll
  for (int b = 0; b < PANEL / 4; b += R) {
    typename PackTaps<D>::Taps t[R];
    bool flip[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const bool liveSlot = s.live(b + u);
      const D d = desc[liveSlot ? s.img : 0];
      const QkAnchorView q = views.v[s.vw];
      const int oy = (((image_of(d).hf - H) * q.ay) >> 1) + q.dy, ox = (((image_of(d).wf - W) * q.ax) >> 1) + q.dx;
      flip[u] = q.flip != 0;
      const int Y = oy + ey, X = ox + (flip[u] ? ex1 : ex0);            // < hf, < wf: the engine checked view x image
      bilinear_taps(t[u], image_of(d).s, image_of(d).s, d, ch, Y, X, in);
      s.next();
    }
    __builtin_amdgcn_sched_barrier(0);              // every load of the round is issued before the first value is waited for
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const bool live = s.live(b + u) && e < E;
      const float val = tap_value(t[u]);
      tile[wave + 4 * (b + u)][lane] = live ? (MEAN ? __fsub_rn(val, flip[u] ? mFlip : mPlain) : val) : 0.0f;
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  __syncthreads();
  tile_write_out(tile, dst, panel, e0, E, lane, wave, NchwRow{C, HW});
}

inline int panels_of(int n) { return (n + PANEL - 1) / PANEL; }

// The launchers of the two resizing pack kernels, for the planar and the strided descriptor type alike.
template <class D>
hipError_t launch_pack_resized(const uint8_t* in, const D* desc, const float* mean, float* dst, int n, int V, const QkViews& views,
                               int C, int H, int W, int Hf, int Wf, hipStream_t st) {
  if (n <= 0 || V < 1 || V > QK_MAX_VIEWS || !in || !desc || Hf < 2 || Wf < 2) return hipErrorInvalidValue;
  for (int v = 0; v < V; ++v)                       // a view outside the full image must never reach the kernel
    if (views.v[v].oy < 0 || views.v[v].ox < 0 || views.v[v].oy > Hf - H || views.v[v].ox > Wf - W) return hipErrorInvalidValue;
  if ((long long)C * Hf * Wf > INT_MAX) return hipErrorInvalidValue;   // the mean's offsets are 32-bit too
  const int E = C * H * W, S = n * V;
  hipLaunchKernelGGL(mean ? HIP_KERNEL_NAME(k_pack_u8_resized<true, D>) : HIP_KERNEL_NAME(k_pack_u8_resized<false, D>),
                     dim3((E + 63) / 64, panels_of(S)), dim3(256), 0, st, in, desc, mean, dst, S, V, views, C, H, W, Hf, Wf);
  return hipGetLastError();
}
template <class D>
hipError_t launch_pack_relaxed(const uint8_t* in, const D* desc, const float* mean, float* dst, int n, int V,
                               const QkAnchorViews& views, int C, int H, int W, hipStream_t st) {
  if (n <= 0 || V < 1 || V > QK_MAX_VIEWS || !in || !desc || C < 1 || H < 1 || W < 1) return hipErrorInvalidValue;
  for (int v = 0; v < V; ++v)                       // an anchor outside 0..2 must never reach the kernel
    if (views.v[v].ay < 0 || views.v[v].ay > 2 || views.v[v].ax < 0 || views.v[v].ax > 2) return hipErrorInvalidValue;
  const int E = C * H * W, S = n * V;
  hipLaunchKernelGGL(mean ? HIP_KERNEL_NAME(k_pack_u8_relaxed<true, D>) : HIP_KERNEL_NAME(k_pack_u8_relaxed<false, D>),
                     dim3((E + 63) / 64, panels_of(S)), dim3(256), 0, st, in, desc, mean, dst, S, V, views, C, H, W);
  return hipGetLastError();
}
