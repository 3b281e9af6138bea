// qcnn_engine.hip — the C-ABI of include/qcnn_hip.h: context, model planning, layer loop.
//
// Mirrors the control flow of the reference's CaffeEva (src/CaffeEva.cc): LoadCaffePara ->
// PrepFeatMap/PrepFeatBuf/PrepCtrdBuf/PrepAsmtBuf (:109-149) becomes qcnn_model_begin / commit /
// set_layer_params; ExecForwardPass's layer loop (:184-205, :232-254) becomes run_layers().
// Everything the loop touches lives in HBM for the whole batch; the host only enqueues kernels.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/qcnn_hip.h"
#include "qcnn_kernels.h"
#include "qcnn_planner.h"
#include "qcnn_src_layout.h"
#include "qcnn_src_yuv.h"

namespace {

std::string g_createError = "";

// The tables a layer's arena may hold beside bias, code book and the plain assignment rows, in the order plan_arena lays them
// out (kTables, below, says when a layer has which, and how it is built)
enum TableKind { T_PROG16, T_SLIDE16, T_SYM16, T_FC8, T_CBN, T_HALF8, T_HALF8_SLIDE, T_SYM8, T_SYM8_SLIDE, T_COUNT };
enum BookKind { BOOK_NONE = -1, BOOK_FC8, BOOK_CONV8, BOOK_COUNT };    // qk_ctrdf_index / qk_ctrd8_index order
struct Span { size_t off = 0, bytes = 0; };

struct LayerShape {
  int M = 0, K = 0, Cs = 0;                                    // as the kernels see the layer (K <= 128)
  int P = 1, Mfile = 0, Kfile = 0;                             // a parameter set with 128 < K <= 256 code words per sub-space: every sub-space is P =
                                                               // ceil(K / 127) pseudo sub-spaces of <= 127 code words + a zero row (M = P * Mfile, K = 128)
  bool dense = false;                                          // precise path: bias + dense weights instead of a quantisation
  size_t offDense = 0, denseFloats = 0;
  size_t offBias = 0, offCtrd = 0, offAsmt = 0, offDmap = 0;   // byte offsets into the arena
  size_t asmtBytes = 0;
  Span tab[T_COUNT];                                           // the per-family tables (kTables, in arena order); bytes = 0: the layer has none
  size_t offBook[BOOK_COUNT] = {0}; bool hasBook[BOOK_COUNT] = {false};   // the code book in the eight-wave kernels' operand orders
  int cbnBits = 0;                                             // bits per assignment of the T_CBN span
  size_t offDecN = 0; int decNV = 0;                          // first layer: the same code words in k_conv_dec_nchw's order; decNV: its padded k (0: not eligible)
  size_t offDecB = 0; int decBK = 0;                          // ... split into three bf16 pieces for k_conv_dec_nchw_split; decBK: its padded k (0: not eligible)
  size_t offDec = 0; int decKp = 0, decS = 0;                  // decoded code words (qcnn_decoded.hip): conv layer with one sub-space of
                                                               // <= 4 dims (decKp > 0), FC layer with one-dim sub-spaces (decKp = -1); 0: not eligible
  bool hasDmap = false;
  bool loaded = false;
  // QCNN_OPT_LUT_MODE = 2 (fp16 table storage): the eight-wave kernels' program tables with offsets into the fp16 table layout.
  // Own allocations, built from the arena's assignment bytes when the mode first runs the layer (every rank of a group builds
  // its own from the broadcast arena); dropped when the layer's parameters are uploaded again
  uint16_t* progF16[2][T_COUNT] = {{nullptr}};                  // [0]: fp16 tables, [1]: QCNN_OPT_LUT_MODE = 3's twice-as-large tiles (T_SYM8 only)
  // conv: launch plans (qcnn_planner.h) by launch geometry and options (panels, sub-batches, split / slide / sym, LUT mode, input
  // in place): sub-batches of unequal panel counts (3 panels over 2 streams) each keep theirs instead of evicting one another —
  // a plan is dozens of 256-CU list schedules on the host
  std::map<std::array<int, 10>, QkConvPlan> plans;
  int segN = 0, segBeg[9] = {0};                               // segments of the last launch when it slid (qcnn_get_layer_segments)
  int lastFrom = -1, lastZ = 1;                                // how the last launch was actually cut
};

struct FmDims { int h, w, c; };

constexpr int kProfRing = 32;    // forwards whose per-layer events are kept
constexpr int kMaxStreams = 4;   // sub-batches (streams) of one forward
constexpr int kSmallBatchMax = QCNN_SMALL_BATCH_MAX;  // batches up to this size run the few-image kernels (QCNN_OPT_SMALL_BATCH): beyond, a
                                   // 128-image panel is cheaper (measured: 1 / 2 / 3 / 4 images 0.58 / 0.85 / 1.15 / 1.47 ms, a panel 1.50 ms)
constexpr size_t kConvPartialFloats = (size_t)64 << 20;   // 256 MB of partial sums for split conv tiles (all sub-batches), allocated when a plan first splits
constexpr size_t kSlack = 64 * 1024;   // bytes of slack behind every device buffer: the MFMA operand loads are
                                        // unconditional and may read a few rows past the last dim / sub-space

}  // namespace

struct QcnnCtx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool ownStream = false;
  std::string err;
  int lutMode = 1, keepAll = 1, profile = 0;
  int nStreams = 2;                  // QCNN_OPT_STREAMS: sub-batches of whole panels run concurrently
  int smallBatch = 1;                // QCNN_OPT_SMALL_BATCH: few-image kernels for batches <= kSmallBatchMax
  int hostChunk = 2;                 // QCNN_OPT_HOST_CHUNK: panels per chunk of a large qcnn_forward_host batch (0: one launch)
  int directDec = 1;                 // QCNN_OPT_DIRECT_DEC: a decoded first layer reads the NCHW input in place (k_conv_dec_nchw) on the fast path
  int decSplit = 1;                  // QCNN_OPT_DEC_BF16SPLIT: ... with its products as fp32-accurate split-bf16 MFMAs (k_conv_dec_nchw_split)
  int packedFc = 0;                  // QCNN_OPT_PACKED_FC (default off: measured 0.056 against 0.035 ms for AlexNet fc6 at one image): the few-image FC kernel reads the bit-packed assignment stream in place
  int half8 = 1;                     // QCNN_OPT_HALF8: half-panel eight-wave workgroups where predicted faster (2: whenever eligible)
  int sym8 = 1;                      // QCNN_OPT_SYM8: eight-wave symmetric workgroups where predicted faster (2: whenever eligible)
  int sym = 1;                       // QCNN_OPT_SYM: symmetric workgroups for 128-channel layers where predicted faster (2: whenever eligible)
  int decode = 1;                    // QCNN_OPT_DECODE: one-sub-space conv layers through their decoded code words (MFMA builders only)
  int slide = 1;                     // QCNN_OPT_SLIDE: sliding-window conv kernels where they pay (MFMA builders only)
  int split = 1;                     // QCNN_OPT_SPLIT: launches that do not fill the chip split their tail (MFMA builders only)
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};
  hipEvent_t evFork = nullptr, evJoin[3] = {nullptr, nullptr, nullptr};

  int L = 0, inC = 0, inH = 0, inW = 0;
  std::vector<QcnnLayerDesc> layers;
  std::vector<FmDims> dims;          // L + 1
  std::vector<LayerShape> shapes;    // L
  int firstFc = -1;
  bool committed = false;
  int maxBatch = 0, maxPanels = 0;

  char* arena = nullptr;
  bool ownArena = false;
  size_t arenaBytes = 0;
  std::vector<float*> fmBuf;         // L + 1, own allocations (nullptr where aliased)
  float* stageIn = nullptr;          // [maxBatch][maxE] linear staging for host <-> device conversions
  float* stageOut = nullptr;
  size_t stageElems = 0;
  uint16_t* stageTop5 = nullptr;
  // pipelined host path (qcnn_forward_host_batches): the upload of batch b+1 runs on its own stream under the layers of
  // batch b; two device input buffers (stageIn and stageIn1), two pinned host result buffers
  hipStream_t copyStream = nullptr;
  float* stageIn1 = nullptr;         // [maxBatch][inC*inH*inW]
  float* pinProb[2] = {nullptr, nullptr};
  uint16_t* pinTop5[2] = {nullptr, nullptr};
  hipEvent_t evCopied[2] = {nullptr, nullptr}, evFreed[2] = {nullptr, nullptr}, evDone[2] = {nullptr, nullptr};
  bool freedValid[2] = {false, false};
  std::vector<hipEvent_t> evChunk;   // chunked single batch (qcnn_forward_host): "chunk k is on the device"
  float* fcFlat = nullptr;           // first FC layer's input in consumption order
  float* fcPartial = nullptr;        // split-M partial sums of the FC layers
  float* convPartial = nullptr;      // partial sums of split conv tiles (kConvPartialFloats)
  bool noConvPartial = false;        // ... could not be allocated: split plans launch their tiles whole
  size_t fcPartialElems = 0;
  size_t fcMaxCt = 0;
  float* viewMean = nullptr;         // qcnn_forward_u8_views: panels [classes][128] of the probabilities averaged over an image's views —
  size_t viewMeanElems = 0;          // allocated at its first call, grown when one needs more, freed with the context (no part of the plan)
  // qcnn_forward_u8_resized_views: the source-image descriptors of a call travel host -> pinned -> device through one of two
  // staging sets the context owns (first use, grown on demand, freed with the context).  ev is recorded behind the pack kernel
  // that reads the set: the next call that takes the set waits for it before it rewrites (or frees) the buffers.
  // qcnn_forward_u8_relaxed_views stages its QkRelaxedImage table through the same two sets: cap counts bytes.
  struct SrcStage { void* pin = nullptr; void* dev = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
  SrcStage srcStage[2];
  int srcStageNext = 0;
  // qcnn_forward_u8_*_host_batches: source bytes stream host -> device through two buffers the context owns like viewMean
  // (first use, grown when a call needs more, freed with the context); everything sized by max_batch and the classes goes with
  // the model (free_model).  No float input staging: the pack kernel reads the source bytes in place
  struct U8Stream {
    uint8_t* src[2] = {nullptr, nullptr};
    size_t srcCap = 0;
    hipEvent_t evCounted[2] = {nullptr, nullptr};     // "the hit count that read labels[k] has passed"
    uint16_t* labels[2] = {nullptr, nullptr};         // [maxBatch] on the device
    uint16_t* pinLabels[2] = {nullptr, nullptr};
    float* prob = nullptr;                            // [maxBatch][classes]: the view averages
    float* rows = nullptr;                            // [maxBatch][classes]: the un-averaged rows of n * V <= maxBatch slots
    uint16_t* top5 = nullptr;
    float* pinRows[2] = {nullptr, nullptr};
    unsigned long long* hits = nullptr;               // [5] on the device, zeroed at every call's entry
    unsigned long long* pinHits = nullptr;
  } u8s;
  // qcnn_calib_begin .. qcnn_calib_end: one resident fp64 matrix [grp][P][P] per listed layer; while armed, run_layers adds the
  // second moments of every batch's input maps to them (k_ec_gram_panel) behind the layers, on the context's stream
  struct Calib {
    struct Layer { int layer = 0; QkGramGeom g = {}; double* G = nullptr; long long rows = 0; };
    bool active = false, armed = false;
    bool wantsInput = false;         // layer 0 is listed: fm[0] must exist as panels, float entry points take the packed route
    std::vector<Layer> layers;
    double* slab = nullptr;          // scratch of the split launches, sized for maxPanels at begin
  } calib;
  int lastN = 0;
  std::vector<float*> lastFm;        // pointer table of the last forward

  std::vector<hipEvent_t> ev;        // kProfRing * kMaxStreams * L * 2
  int profCount = 0;                 // forwards in the ring, not yet drained
  struct ProfRec { size_t slot; int layer; };
  std::vector<ProfRec> profPending;  // event pairs recorded since the last drain (only layers that were launched)
  std::vector<double> profSum;       // per layer: ms summed over every recorded launch
  std::vector<long long> profLaunches;
  int profForwards = 0;
};

namespace {

int fail(QcnnCtx* c, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_createError = buf;
  return 1;
}

#define HIP_TRY(c, call)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) return fail((c), "%s -> %s", #call, hipGetErrorString(e_));     \
  } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int conv_out(int in, int knl, int stride, int pad) { return (in + 2 * pad - knl) / stride + 1; }
int pool_out(int in, int knl, int stride, int pad) {          // ceil mode, src/CaffeEva.cc:367-370
  const int num = in + 2 * pad - knl;
  return (num + stride - 1) / stride + 1;
}

size_t fm_elems(const QcnnCtx* c, int l) { return (size_t)c->dims[l].h * c->dims[l].w * c->dims[l].c; }

template <class T> T* arena_at(const QcnnCtx* c, size_t off) { return reinterpret_cast<T*>(c->arena + off); }
// a layer's table of one kind; nullptr: it has none
const uint16_t* table(const QcnnCtx* c, const LayerShape& s, int kind) {
  return s.tab[kind].bytes ? arena_at<const uint16_t>(c, s.tab[kind].off) : nullptr;
}

// The reference's .cbn packing of `bits`-bit values (include/FileIO.h:299-341): 4096-byte blocks of floor(32768 / bits) values, MSB
// first, no value across a block; bits <= 8, so a value touches at most two bytes
size_t cbn_size(size_t n, int bits) { const size_t per = 4096 * 8 / (size_t)bits; return (n + per - 1) / per * 4096; }
unsigned cbn_get(const uint8_t* blocks, size_t e, int bits) {
  const size_t per = 4096 * 8 / (size_t)bits, bit0 = (e % per) * bits;
  const uint8_t* b = blocks + (e / per) * 4096 + (bit0 >> 3);
  const unsigned w = ((unsigned)b[0] << 8) | (unsigned)b[(bit0 & 7) + bits > 8 ? 1 : 0];
  return (w >> (16 - (bit0 & 7) - bits)) & ((1u << bits) - 1u);
}
void cbn_put(uint8_t* blocks, size_t e, int bits, unsigned v) {      // into zeroed blocks
  const size_t per = 4096 * 8 / (size_t)bits, bit0 = (e % per) * bits;
  uint8_t* b = blocks + (e / per) * 4096 + (bit0 >> 3);
  const unsigned w = v << (16 - (bit0 & 7) - bits);
  b[0] |= (uint8_t)(w >> 8);
  if (w & 0xffu) b[1] |= (uint8_t)(w & 0xffu);
}
int cbn_bits(int K) {               // the reference's CalcBitCntPerEle for K code words (src/CaffePara.cc:360-380)
  int bits = 1;
  while ((1 << bits) < K) ++bits;
  return bits;
}

// ------------------------------------------------------------------------------------------------------------------
// kTables: the one place that knows, per TableKind, when a layer has the table and how big it is, and how it is built from the
// arena's assignment rows.  (Layers of pseudo sub-spaces — more than 128 code words, P > 1 — always run the exact-builder
// kernels, which read the plain rows: they have none of these.)
// ------------------------------------------------------------------------------------------------------------------
struct TableGeom {
  bool conv;                        // else FC: Cin = its D input dims, grp = knl = stride = 1
  int Cin, Ct, grp, knl, stride;
  int M, Cs, K, P;
  QkSlots sl;                       // of the plain assignment rows (QkSlots, qcnn_kernels.h)
};
TableGeom table_geom(const QcnnCtx* c, int l) {
  const QcnnLayerDesc& d = c->layers[l];
  const LayerShape& s = c->shapes[l];
  const int Ct = c->dims[l + 1].c;
  if (d.type == QCNN_CONV) return {true, c->dims[l].c, Ct, d.grpCnt, d.knlSiz, d.stride, s.M, s.Cs, s.K, s.P, qk_conv_slots(Ct / d.grpCnt, d.grpCnt)};
  return {false, (int)fm_elems(c, l), Ct, 1, 1, 1, s.M, s.Cs, s.K, s.P, qk_fc_slots(Ct)};
}

// 16-wave conv kernels (K = 128): offsets in consumption order (QkProgram) for the tile kernel, its sliding variant where it
// applies, and the symmetric kernel's (8 channels per wave, 2x2 tile) layout.  pg.rfH = 0: the layer has no such table
struct Layout16 { QkSlots dst; QkProgram pg; int slide; };
Layout16 layout16(const TableGeom& g, int kind) {
  Layout16 y = {g.sl, QkProgram{}, 0};
  if (!g.conv || g.P != 1) return y;
  if (kind == T_SYM16) {
    if (!qk_conv_sym_shape(g.Cin, g.grp, g.Ct, g.M, g.Cs, g.K)) return y;
    y.dst = qk_make_slots(g.sl.C, g.sl.groups, 8);
    y.pg = qk_conv_program(y.dst, g.knl, g.stride);
  } else if (g.K == 128 && kind == T_PROG16) {
    y.pg = qk_conv_program(g.sl, g.knl, g.stride);
  } else if (g.K == 128) {
    const QkSlide sc = qk_slide_config(g.sl.C, g.sl.groups, g.knl, g.stride);
    if (sc.ns == 0) return y;
    y.dst = sc.sl; y.slide = 1;
    y.pg = qk_conv_program_slide(sc.sl, sc.ns, sc.nc, g.knl, g.stride);
  }
  return y;
}
template <int KIND> size_t bytes16(const TableGeom& g, int) {
  const QkProgram pg = layout16(g, KIND).pg;
  return (size_t)pg.rfH * pg.rfW * g.M * pg.rowU16 * sizeof(uint16_t);
}
template <int KIND> hipError_t build16(const TableGeom& g, const uint8_t* rows, uint16_t* out, hipStream_t st, int) {
  const Layout16 y = layout16(g, KIND);
  return qk_build_program(rows, out, g.sl, y.dst, y.pg, g.knl, g.stride, g.M, st, y.slide);
}

// eight-wave symmetric kernel (Qk8Config) and its sliding form; v = 2: the twice-as-large tiles of QCNN_OPT_LUT_MODE = 3
Qk8Config cfg_sym8(const TableGeom& g, int v) {
  return v == 2 ? qk_conv_sym8_config16(g.Cin, g.grp, g.Ct, g.M, g.Cs, g.K) : qk_conv_sym8_config(g.Cin, g.grp, g.Ct, g.M, g.Cs, g.K);
}
Qk8Config cfg_sym8_slide(const TableGeom& g, int) { return qk_conv_sym8_slide_config(g.Cin, g.grp, g.Ct, g.M, g.Cs, g.K, g.knl, g.stride); }
template <Qk8Config (*CFG)(const TableGeom&, int)> size_t bytes8(const TableGeom& g, int v) {
  return g.conv && g.P == 1 ? qk_conv_sym8_program_bytes(CFG(g, v), g.grp, g.knl, g.stride, g.M) : 0;
}
template <Qk8Config (*CFG)(const TableGeom&, int)> hipError_t build8(const TableGeom& g, const uint8_t* rows, uint16_t* out, hipStream_t st, int v) {
  return qk_build_program8(rows, out, g.sl, CFG(g, v), g.Ct / g.grp, g.grp, g.knl, g.stride, g.M, st, v ? 1 : 0);
}

// half-panel eight-wave kernel (QkH8Config, qcnn_half8.hip) and its sliding form
QkH8Config cfg_half8(const TableGeom& g) { return qk_conv_half8_config(g.Cin, g.grp, g.Ct, g.M, g.Cs, g.K); }
QkH8Config cfg_half8_slide(const TableGeom& g) { return qk_conv_half8_slide_config(g.Cin, g.grp, g.Ct, g.M, g.Cs, g.K, g.knl, g.stride); }
template <QkH8Config (*CFG)(const TableGeom&)> size_t bytes_h8(const TableGeom& g, int) {
  return g.conv && g.P == 1 ? qk_conv_half8_program_bytes(CFG(g), g.grp, g.knl, g.stride, g.M) : 0;
}
template <QkH8Config (*CFG)(const TableGeom&)> hipError_t build_h8(const TableGeom& g, const uint8_t* rows, uint16_t* out, hipStream_t st, int) {
  return qk_build_program_h8(rows, out, g.sl, CFG(g), g.Ct / g.grp, g.grp, g.knl, g.stride, g.M, st);
}

// FC with 32 code words of 4 dims: the eight-wave kernel's program (k_fc_sym8), uint16 offsets in its channel order
size_t bytes_fc8(const TableGeom& g, int) {
  return !g.conv && g.P == 1 && qk_fc_sym8_shape(g.Cin, g.Ct, g.M, g.Cs, g.K) ? qk_fc_sym8_program_bytes(g.Ct, g.M) : 0;
}
hipError_t build_fc8(const TableGeom& g, const uint8_t* rows, uint16_t* out, hipStream_t st, int v) {
  return qk_build_program_fc8(rows, out, g.sl, g.Ct, g.M, st, v ? 1 : 0);
}
// FC: the assignments bit-packed as the .cbn payload holds them (file order [Ct][M], include/FileIO.h:128-166), read in place
// by the few-image kernel; written by the upload itself (upload_packed_assignments)
size_t bytes_cbn(const TableGeom& g, int) { return !g.conv && g.P == 1 ? cbn_size((size_t)g.Ct * g.M, cbn_bits(g.K)) : 0; }

struct TableDesc {
  size_t (*bytes)(const TableGeom& g, int v);      // 0: the layer has none.  v = 0: the arena's table; 1 / 2: its fp16 forms (ensure_f16_program)
  hipError_t (*build)(const TableGeom& g, const uint8_t* rows, uint16_t* out, hipStream_t st, int v);
  BookKind book;                                   // the code book in the kernel's operand order goes with it: one copy, laid out
};                                                 // behind the last of the (consecutive) kinds that name it
const TableDesc kTables[T_COUNT] = {
    /* T_PROG16      */ {bytes16<T_PROG16>, build16<T_PROG16>, BOOK_NONE},
    /* T_SLIDE16     */ {bytes16<T_SLIDE16>, build16<T_SLIDE16>, BOOK_NONE},
    /* T_SYM16       */ {bytes16<T_SYM16>, build16<T_SYM16>, BOOK_NONE},
    /* T_FC8         */ {bytes_fc8, build_fc8, BOOK_FC8},
    /* T_CBN         */ {bytes_cbn, nullptr, BOOK_NONE},
    /* T_HALF8       */ {bytes_h8<cfg_half8>, build_h8<cfg_half8>, BOOK_CONV8},
    /* T_HALF8_SLIDE */ {bytes_h8<cfg_half8_slide>, build_h8<cfg_half8_slide>, BOOK_CONV8},
    /* T_SYM8        */ {bytes8<cfg_sym8>, build8<cfg_sym8>, BOOK_CONV8},
    /* T_SYM8_SLIDE  */ {bytes8<cfg_sym8_slide>, build8<cfg_sym8_slide>, BOOK_CONV8},
};

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
      s.tab[k] = Span{0, kTables[k].bytes(g, 0)};
      if (s.tab[k].bytes) { s.tab[k].off = off; off = align_up(off + s.tab[k].bytes + QCNN_ROWS_PAD, 256); }
      const int b = kTables[k].book;
      if (b == BOOK_NONE) continue;
      s.hasBook[b] = s.hasBook[b] || s.tab[k].bytes;
      if (s.hasBook[b] && (k + 1 == T_COUNT || kTables[k + 1].book != b)) { s.offBook[b] = off; off = align_up(off + bookBytes, 256); }
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

void drop_f16_programs(LayerShape& s) {
  for (auto& form : s.progF16)
    for (uint16_t*& t : form) {
      if (t) (void)hipFree(t);
      t = nullptr;
    }
}

constexpr size_t kCalibSlabBytes = (size_t)128 << 20;   // cap of the resident calibration's split scratch (part of its split rule)

// the resident calibration matrices (hipFree waits for the launches that still write them)
void calib_free(QcnnCtx* c) {
  for (QcnnCtx::Calib::Layer& q : c->calib.layers)
    if (q.G) (void)hipFree(q.G);
  if (c->calib.slab) (void)hipFree(c->calib.slab);
  c->calib = QcnnCtx::Calib();
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
  c->stageIn = c->stageOut = nullptr; c->stageTop5 = nullptr; c->stageElems = 0;
  c->fcPartial = nullptr; c->fcPartialElems = 0;
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  c->ev.clear();
  c->profCount = 0; c->profPending.clear(); c->profForwards = 0;
  c->lastFm.clear(); c->lastN = 0;       // nothing of the old model can be read back any more
  c->committed = false;
}

// Linear staging for host <-> device conversions.  Sized for what the forward paths need — a batch of network inputs, a batch of
// class scores — and grown on demand when a larger feature map is dumped (qcnn_get_layer_output / qcnn_run_layer): sizing it for the
// LARGEST map of the model up front made the first qcnn_forward_host of VGG-16 at batch 1000 allocate 2 x 12.8 GB (0.75 s; AlexNet: 2 x
// 1.2 GB)
int ensure_stage(QcnnCtx* c, size_t elems = 0) {
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

// Does conv layer l run through its decoded code words (qcnn_decoded.hip)?  The f32 MFMA mode only: the exact
// builder keeps the reference's summation order and the fp16 study is about the tables themselves.
bool decoded_layer(const QcnnCtx* c, int l) {
  const LayerShape& s = c->shapes[l];
  return c->decode && s.decKp > 0 && !s.dense && c->lutMode == 1 && c->layers[l].type == QCNN_CONV;
}

// fp16 table storage (QCNN_OPT_LUT_MODE = 2 / 3): the layer's table of `kind` (T_SYM8, T_FC8) in the fp16 layout's offsets, built by
// the kind's own builder at first use; the build runs on `st`, in front of the launch that reads it.  nullptr: failed (c->err).
// The pointer is published in the LayerShape only once its build has been enqueued without error: on any failure behind the
// hipMalloc the allocation is released, so that a later forward builds again instead of launching with an unbuilt table
const uint16_t* ensure_f16_program(QcnnCtx* c, int l, int kind, hipStream_t st) {
  LayerShape& s = c->shapes[l];
  const int v = (kind == T_SYM8 && c->lutMode == 3) ? 2 : 1;     // fp16 sums too: the program of the twice-as-large tiles
  if (s.progF16[v - 1][kind]) return s.progF16[v - 1][kind];
  const TableGeom g = table_geom(c, l);
  const size_t bytes = kTables[kind].bytes(g, v) + QCNN_ROWS_PAD + (v == 2 ? 4096 : 0);
  uint16_t* t = nullptr;
  hipError_t e = hipMalloc(&t, bytes);
  if (e == hipSuccess) e = hipMemsetAsync(t, 0, bytes, st);
  if (e == hipSuccess) e = kTables[kind].build(g, arena_at<const uint8_t>(c, s.offAsmt), t, st, v);
  if (e == hipSuccess) e = hipStreamSynchronize(st);       // once per layer: the other sub-batch streams of this forward read the table too
  if (e != hipSuccess) {
    (void)hipFree(t);
    fail(c, "layer %d: fp16 program table -> %s", l, hipGetErrorString(e));
    return nullptr;
  }
  return s.progF16[v - 1][kind] = t;
}

// One layer on `panels` panels: the per-launch facts (run_layers and qcnn_run_layer fill them)
struct Launch {
  const float* src; float* dst;    // in panel layout
  int panels, p0;                  // p0: first panel of the sub-batch (offsets into the scratch buffers)
  hipStream_t st;                  // the stream the sub-batch runs on
  const float* inNchw = nullptr;   // the network input, read in place by the first layer (src unused)
  int nImages = 0;                 // ... its images
  int live = QCNN_PANEL;           // images every panel of this launch holds (128, or the batch size of a single-panel forward)
  bool small = false;              // the few-image kernels (qcnn_small.hip) run the conv/FC layers
  int sub = 0, nsub = 1;           // index and number of the sub-batches (streams) of this forward: each has its own share of the scratch
  int panelsAll = 0;               // panels of ALL sub-batches of this forward (they run concurrently on their own streams and share the
                                   // 256 CUs); 0 = this launch is alone
  bool fuseRelu = false;
  bool flatFcInput = false;        // the FC input rows are already in consumption order (qcnn_run_layer): no NCHW-flatten map
};

int launched(QcnnCtx* c, int l, hipError_t e) {
  if (e != hipSuccess) return fail(c, "layer %d (type %d) launch failed: %s", l, c->layers[l].type, hipGetErrorString(e));
  return 0;
}

// Partial-sum scratch.  Split conv tiles: kConvPartialFloats shared by the nsub sub-batches, allocated by the first split launch
// of this context; when the device has no memory left for it (large maps at a large batch) the tiles run whole, which needs
// none — never a failed forward.  FC layers: every sub-batch has its own slab of QK_MAX_FC_SPLIT x (its panels) x (widest layer)
float* conv_partial(QcnnCtx* c, const Launch& L) {
  if (!c->convPartial && !c->noConvPartial && hipMalloc(&c->convPartial, kConvPartialFloats * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    c->convPartial = nullptr; c->noConvPartial = true;
  }
  return c->convPartial ? c->convPartial + kConvPartialFloats / (size_t)L.nsub * L.sub : nullptr;
}
size_t fc_partial_offset(const QcnnCtx* c, const Launch& L) { return (size_t)QK_MAX_FC_SPLIT * L.p0 * c->fcMaxCt * QCNN_PANEL; }
size_t fc_partial_left(const QcnnCtx* c, const Launch& L) {
  const size_t poff = fc_partial_offset(c, L);
  return c->fcPartialElems > poff ? c->fcPartialElems - poff : 0;
}

// what ConvParams and DecParams share: source (a panel map, or the network input read in place), destination, map geometry
template <class P> void conv_geom(P& q, const QcnnCtx* c, int l, const Launch& L) {
  const QcnnLayerDesc& d = c->layers[l];
  const FmDims& a = c->dims[l];
  const FmDims& b = c->dims[l + 1];
  q.src = L.src; q.dst = L.dst;
  q.srcNchw = 0; q.nImages = 0; q.panel0 = 0;
  if (L.inNchw) { q.src = L.inNchw; q.srcNchw = 1; q.nImages = L.nImages; q.panel0 = L.p0; }
  q.bias = arena_at<const float>(c, c->shapes[l].offBias);
  q.H = a.h; q.W = a.w; q.Cin = a.c; q.Ho = b.h; q.Wo = b.w; q.Ct = b.c;
  q.knl = d.knlSiz; q.stride = d.stride; q.pad = d.padSiz;
  q.relu = L.fuseRelu ? 1 : 0; q.panels = L.panels;
}

// precise path (qcnn_dense.hip): a conv layer, or an FC layer as a 1x1 conv on a 1x1 map
int launch_dense(QcnnCtx* c, int l, const Launch& L, const float* src, const FmDims& a, const FmDims& b, int knl, int stride, int pad, int grp) {
  const LayerShape& s = c->shapes[l];
  DenseParams q;
  q.src = src; q.dst = L.dst;
  q.bias = arena_at<const float>(c, s.offBias);
  q.wt = arena_at<const float>(c, s.offDense);
  q.H = a.h; q.W = a.w; q.Cin = a.c; q.Ho = b.h; q.Wo = b.w; q.Ct = b.c;
  q.knl = knl; q.stride = stride; q.pad = pad; q.grp = grp;
  q.relu = L.fuseRelu ? 1 : 0; q.panels = L.panels;
  return launched(c, l, qk_dense(q, L.st));
}

int launch_conv(QcnnCtx* c, int l, const Launch& L) {
  const QcnnLayerDesc& d = c->layers[l];
  const FmDims& a = c->dims[l];
  const FmDims& b = c->dims[l + 1];
  LayerShape& s = c->shapes[l];
  const float* inNchw = L.inNchw;
  hipStream_t st = L.st;
  if (!s.loaded) return fail(c, "layer %d: parameters not uploaded", l);
  // precise path (CalcFeatMap_ConvPrec, src/CaffeEva.cc:681-758)
  if (s.dense) return launch_dense(c, l, L, L.src, a, b, d.knlSiz, d.stride, d.padSiz, d.grpCnt);
  // one sub-space of <= 4 dims: decoded code words on the matrix pipe.  Batches of one to three images too when the layer
  // reads the NCHW input in place: a 16-image tile with one live image still beats the few-image table kernel, whose
  // workgroups rebuild the pixel tables five times (AlexNet conv1 at one image: 0.126 -> 0.0xx ms)
  if (decoded_layer(c, l) && (L.small ? (inNchw && s.decNV && c->directDec) : (!inNchw || s.decNV))) {
    DecParams q;
    conv_geom(q, c, l, L);
    q.wdec = arena_at<const float>(c, inNchw ? s.offDecN : s.offDec);
    q.Kr = d.knlSiz * a.c; q.Kp = s.decKp; q.S = s.decS;
    if (inNchw) { q.Kr = d.knlSiz * d.knlSiz * a.c; q.Kp = s.decNV; q.S = b.c; }
    q.live = L.live;
    s.lastFrom = -3; s.lastZ = inNchw ? 2 : 1;        // reported by qcnn_get_layer_split as (-3, 1), NCHW in place: (-3, 2)
    const bool splitBf16 = inNchw && c->decSplit && s.decBK > 0;   // fp32-accurate split-bf16 products (QCNN_OPT_DEC_BF16SPLIT)
    if (splitBf16) { q.Kp = s.decBK; q.wdec = arena_at<const float>(c, s.offDecB); }
    const hipError_t e = splitBf16 ? qk_conv_dec_nchw_split(q, st) : inNchw ? qk_conv_dec_nchw(q, st) : qk_conv_dec(q, st);
    if (e != hipErrorInvalidValue) return launched(c, l, e);   // (a map beyond the kernel's 32-bit byte offsets: the table kernel below)
  }
  ConvParams p;
  conv_geom(p, c, l, L);
  p.ctrd = arena_at<const float>(c, s.offCtrd);
  p.ctrd8 = s.hasBook[BOOK_CONV8] ? arena_at<const float>(c, s.offBook[BOOK_CONV8]) : nullptr;
  p.rows = arena_at<const uint8_t>(c, s.offAsmt);
  p.prog = table(c, s, T_PROG16);
  p.grp = d.grpCnt;
  p.M = s.M; p.Cs = s.Cs; p.K = s.K; p.pd = s.P;
  p.splitFrom = 0; p.splitZ = 1; p.partial = nullptr;
  p.nSeg = 0; p.progS = table(c, s, T_SLIDE16);
  s.lastFrom = -1; s.lastZ = 1;
  // more than 128 code words per sub-space: pseudo sub-spaces, exact-builder kernel in every mode
  if (s.P > 1) return launched(c, l, qk_conv_aprx(p, 0, st));
  // few-image kernel unless the layer's shape is outside what it covers (a tap window x K that does not fit its LDS
  // table): the panel kernel handles every shape set_layer_shape accepts
  if (L.small) {
    const hipError_t e = qk_conv_small(p, L.live, st);
    if (e != hipErrorInvalidValue) {
      s.lastFrom = -11; s.lastZ = 1;                  // reported by qcnn_get_layer_split as (-11, 1): the few-image kernel took the launch
      return launched(c, l, e);
    }
  }
  // fp16 table storage (QCNN_OPT_LUT_MODE = 2): the eight-wave tile kernel in its fp16 form wherever the layer's shape has one
  // (K = 128, complete 4- / 8-dim sub-spaces, > 64 channels per group); QCNN_OPT_SYM8 = 0 keeps every layer in the 16-wave
  // kernels, which round the same entries and keep them in f32 slots (same sums, same bits: the tests compare the two)
  // QCNN_OPT_LUT_MODE = 3 keeps the running sums as packed fp16 as well (twice the tile per wave); layers without an fp16
  // form round their entries and keep fp32 sums in both modes
  if (c->lutMode >= 2 && c->sym8 && s.tab[T_SYM8].bytes && !inNchw) {
    if (!(p.progS = ensure_f16_program(c, l, T_SYM8, st))) return 1;
    s.lastFrom = c->lutMode == 3 ? -8 : -7; s.lastZ = 1;   // reported by qcnn_get_layer_split as (-7 / -8 fp16 sums, 1)
    return launched(c, l, qk_conv_sym8(p, st, c->lutMode == 3 ? 2 : 1));
  }
  // Which kernel family runs this launch, and how it is cut: the planner (qcnn_planner.h) prices every eligible family for
  // this launch geometry — cached per layer —, its decision rules pick one.  MFMA builders only: the exact builder keeps
  // the tile kernel and the reference's summation order.
  if (c->lutMode >= 1 && (c->split || c->slide || c->sym || c->sym8 || c->half8)) {
    QkPlanOptions o = {};
    o.split = c->split; o.slide = c->slide; o.sym = c->sym; o.sym8 = c->sym8; o.half8 = c->half8;
    o.lutMode = c->lutMode; o.inNchw = inNchw ? 1 : 0; o.scratchFloats = kConvPartialFloats / (size_t)L.nsub;
    o.concurrent = (L.nsub > 1 && L.panelsAll > L.panels) ? 1 : 0;
    o.hasSlide16 = s.tab[T_SLIDE16].bytes != 0; o.hasSym16 = s.tab[T_SYM16].bytes != 0; o.hasSym8 = s.tab[T_SYM8].bytes != 0;
    o.hasSym8Slide = s.tab[T_SYM8_SLIDE].bytes != 0; o.hasHalf8 = s.tab[T_HALF8].bytes != 0; o.hasHalf8Slide = s.tab[T_HALF8_SLIDE].bytes != 0;
    const std::array<int, 10> key = {L.nsub > 1 ? L.panelsAll : 0, L.panels, L.nsub, c->split ? 1 : 0, c->slide, c->sym, c->lutMode, inNchw ? 1 : 0, c->sym8, c->half8};
    auto it = s.plans.find(key);
    if (it == s.plans.end()) {
      // Sub-batches on several streams run CONCURRENTLY: the tail of one sub-batch's launch fills with the other's workgroups
      // (that is what the streams are for), so the family is chosen for the panels of the whole forward — planned per
      // sub-batch, a 1000-image forward on two streams took the kernels of a 500-image one (conv3 / conv4 back on the 16-wave
      // tile kernel) and lost what the overlap gained: 103.8 k images/s against 107 k with the one-stream plan's kernels.
      ConvParams pp = p;
      if (o.concurrent) pp.panels = L.panelsAll;
      it = s.plans.emplace(key, qk_plan_conv(pp, o)).first;
    }
    const QkConvChoice ch = qk_choose_conv(it->second, o);
    auto segments = [&]() {
      p.nSeg = ch.nSeg; s.segN = ch.nSeg; s.lastZ = ch.nSeg;
      for (int i = 0; i <= ch.nSeg; ++i) { p.segBeg[i] = ch.segBeg[i]; s.segBeg[i] = ch.segBeg[i]; }
    };
    s.lastFrom = ch.family; s.lastZ = 1;         // what qcnn_get_layer_split reports: (family code, slices / segments)
    switch (ch.family) {
      case QK_FAM_HALF8_SLIDE:
        p.progS = table(c, s, T_HALF8_SLIDE);
        segments();
        return launched(c, l, qk_conv_half8_slide(p, st));
      case QK_FAM_HALF8:
        p.progS = table(c, s, T_HALF8);
        return launched(c, l, qk_conv_half8(p, st));
      case QK_FAM_SYM8_SLIDE:
        p.progS = table(c, s, T_SYM8_SLIDE);
        segments();
        return launched(c, l, qk_conv_sym8_slide(p, st));
      case QK_FAM_SYM8:
        p.progS = table(c, s, T_SYM8);
        if (ch.Z > 1) {
          if (float* ps = conv_partial(c, L)) { p.splitFrom = 0; p.splitZ = ch.Z; p.partial = ps; s.lastZ = ch.Z; }
        }
        return launched(c, l, qk_conv_sym8(p, st));
      case QK_FAM_SYM16:
        p.progS = table(c, s, T_SYM16);
        return launched(c, l, qk_conv_sym(p, st));
      case QK_FAM_SLIDE16:
        segments();                                // k_conv_aprx<.., SLIDE> below (p.progS = the sliding program)
        break;
      default:                                     // tile kernel, whole or with a split tail
        s.lastFrom = -1;
        if (ch.Z > 1) {
          if (float* ps = conv_partial(c, L)) {
            p.splitFrom = ch.splitFrom; p.splitZ = ch.Z; p.partial = ps;
            s.lastFrom = ch.splitFrom; s.lastZ = ch.Z;
          }
        }
        break;
    }
  }
  return launched(c, l, qk_conv_aprx(p, c->lutMode, st));
}

// NHWC -> consumption order (NCHW flatten) into the scratch map in front of the first FC layer; *src: what the layer then reads
hipError_t fc_input(QcnnCtx* c, int l, const Launch& L, const float** src) {
  const LayerShape& s = c->shapes[l];
  *src = L.src;
  if (!s.hasDmap || L.flatFcInput) return hipSuccess;
  float* flat = c->fcFlat + (size_t)L.p0 * fm_elems(c, l) * QCNN_PANEL;
  *src = flat;
  return qk_permute_rows(L.src, flat, arena_at<const int>(c, s.offDmap), (int)fm_elems(c, l), L.panels, L.live, L.st);
}

int launch_fc(QcnnCtx* c, int l, const Launch& L) {
  LayerShape& s = c->shapes[l];
  const int D = (int)fm_elems(c, l), Ct = c->dims[l + 1].c, panels = L.panels, relu = L.fuseRelu ? 1 : 0;
  hipStream_t st = L.st;
  if (!s.loaded) return fail(c, "layer %d: parameters not uploaded", l);
  hipError_t e;
  const float* src = nullptr;
  if ((e = fc_input(c, l, L, &src)) != hipSuccess) return launched(c, l, e);
  // precise path (CalcFeatMap_FCntPrec, src/CaffeEva.cc:932-966): a 1x1 conv on a 1x1 map
  if (s.dense) return launch_dense(c, l, L, src, FmDims{1, 1, D}, FmDims{1, 1, Ct}, 1, 1, 0, 1);
  // which panel kernel, and over how many workgroups its sub-space axis is split: the planner's rule (qk_choose_fc)
  const QkFcGeom g = {D, Ct, s.M, s.K, s.Cs, s.P, panels, L.live};
  const QkFcOptions o = {c->split, c->sym8, c->decode, c->lutMode, L.small ? 1 : 0, s.decKp < 0, s.tab[T_FC8].bytes != 0, fc_partial_left(c, L)};
  const QkFcChoice ch = qk_choose_fc(g, o);
  float* partial = ch.splits > 1 ? c->fcPartial + fc_partial_offset(c, L) : nullptr;
  const size_t slab = (size_t)panels * Ct * QCNN_PANEL;
  if (ch.family == QK_FC_DEC) {        // one-dim sub-spaces: decoded code words on the matrix pipe (qcnn_decoded.hip)
    FcDecParams q;
    q.src = src; q.dst = L.dst; q.partial = partial;
    q.bias = arena_at<const float>(c, s.offBias);
    q.wdec = arena_at<const float>(c, s.offDec);
    q.D = D; q.Ct = Ct; q.S = s.decS;
    q.relu = relu; q.panels = panels; q.halves = 2;
    s.lastFrom = ch.family; s.lastZ = ch.splits;       // reported by qcnn_get_layer_split as (-3, k slices over workgroups)
    e = qk_fc_dec(q, ch.splits, L.live, st);
    if (e == hipSuccess && ch.splits > 1) e = qk_sum_partials(partial, L.dst, ch.splits, slab, relu, st);
    return launched(c, l, e);
  }
  s.lastFrom = -1; s.lastZ = 1;
  FcParams p;
  p.src = src; p.dst = L.dst;
  p.bias = arena_at<const float>(c, s.offBias);
  p.ctrd = arena_at<const float>(c, s.offCtrd);
  p.rows = arena_at<const uint8_t>(c, s.offAsmt);
  p.cbn = c->packedFc ? reinterpret_cast<const uint8_t*>(table(c, s, T_CBN)) : nullptr;
  p.cbnBits = s.cbnBits;
  p.D = D; p.Ct = Ct; p.M = s.M; p.Cs = s.Cs; p.K = s.K; p.pd = s.P;
  p.relu = relu; p.panels = panels;
  p.msplit = 1; p.partial = nullptr;
  if (s.P > 1) return launched(c, l, qk_fc_aprx(p, 0, st));     // pseudo sub-spaces: one pass of the exact-builder kernel
  if (L.small && s.K % 4 == 0 && (size_t)L.live * s.M * s.K <= c->fcPartialElems) {
    p.partial = c->fcPartial;          // few images: the tables are materialised in the partial-sum scratch
    e = qk_fc_small(p, L.live, st);    // (K not a multiple of 4: the panel kernel below)
    if (e != hipErrorInvalidValue) {
      s.lastFrom = -11; s.lastZ = 1;   // reported by qcnn_get_layer_split as (-11, 1): k_fc_lut + k_fc_small took the launch
      return launched(c, l, e);
    }
  }
  p.msplit = ch.splits; p.partial = partial;
  if (ch.family == QK_FC_WAVE12) {
    e = qk_fc_aprx(p, c->lutMode, st);
  } else {
    s.lastFrom = ch.family; s.lastZ = ch.splits;   // reported by qcnn_get_layer_split as (-5 / -7 fp16 tables / -8 fp16 sums, splits of the sub-space axis)
    const int mode = ch.family == QK_FC_SYM8 ? 0 : ch.family == QK_FC_SYM8_F16 ? 1 : 2;
    const uint16_t* prog = mode ? ensure_f16_program(c, l, T_FC8, st) : table(c, s, T_FC8);
    if (!prog) return 1;
    e = qk_fc_sym8(p, prog, arena_at<const float>(c, s.offBook[BOOK_FC8]), st, mode);
  }
  if (e == hipSuccess && ch.splits > 1) e = qk_sum_partials(partial, L.dst, ch.splits, slab, relu, st);
  return launched(c, l, e);
}

int launch_layer(QcnnCtx* c, int l, const Launch& L) {
  const QcnnLayerDesc& d = c->layers[l];
  const FmDims& a = c->dims[l];
  const FmDims& b = c->dims[l + 1];
  const size_t elems = (size_t)L.panels * fm_elems(c, l) * QCNN_PANEL;
  switch (d.type) {
    case QCNN_CONV: return launch_conv(c, l, L);
    case QCNN_FCNT: return launch_fc(c, l, L);
    case QCNN_POOL: return launched(c, l, qk_pool(L.src, L.dst, L.panels, a.h, a.w, a.c, b.h, b.w, d.knlSiz, d.stride, d.padSiz, L.live, L.st));
    case QCNN_RELU: return launched(c, l, qk_relu(L.src, L.dst, elems, L.st));
    case QCNN_LORN: return launched(c, l, qk_lrn(L.src, L.dst, L.panels, a.h * a.w, a.c, d.lrnSiz, d.lrnAlp, d.lrnBet, d.lrnIni, L.live, L.st));
    case QCNN_DRPT:   // test-time dropout is a copy (src/CaffeEva.cc:1091-1096); only reached by qcnn_run_layer
      return launched(c, l, hipMemcpyAsync(L.dst, L.src, elems * sizeof(float), hipMemcpyDeviceToDevice, L.st));
    case QCNN_SMAX: return launched(c, l, qk_softmax(L.src, L.dst, L.panels, a.h * a.w * a.c, L.live, L.st));
    default: return fail(c, "layer %d: invalid layer type %d", l, d.type);
  }
}

// accumulate the recorded event pairs into the per-layer sums (blocks until the recorded work is done)
int drain_profile(QcnnCtx* c) {
  if (c->profPending.empty()) { c->profForwards += c->profCount; c->profCount = 0; return 0; }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (const QcnnCtx::ProfRec& r : c->profPending) {
    float ms = 0.0f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[r.slot], c->ev[r.slot + 1]));
    c->profSum[r.layer] += ms;
    c->profLaunches[r.layer] += 1;
  }
  c->profForwards += c->profCount;
  c->profCount = 0;
  c->profPending.clear();
  return 0;
}

// workgroups a fused LRN + pool launch must have
// (192: one panel of AlexNet's LRN1 + pool1 — 196 workgroups — fuses: 0.091 against 0.104 ms; LRN2 + pool2 at one / two panels —
// 64 / 128 workgroups — must not: 0.21 against 0.065 ms)
int lrn_pool_min_blocks() {
#ifdef QCNN_EXPERIMENT     // variant builds only (scripts/build_variant.sh -DQCNN_EXPERIMENT)
  static const int v = [] { const char* e = getenv("QCNN_LRNPOOL_MIN"); return (e && atoi(e) > 0) ? atoi(e) : 192; }();
  return v;
#else
  return 192;
#endif
}

// Can the first layer's builders read the NCHW network input in place (no pack kernel, no packed copy of the input)?
// Fast path only (layer-for-layer mode keeps fm[0] for dumps); a conv layer with <= 4 input channels per group (one
// sub-space of <= 4 dims: exactly what the operand loads of one stage touch) and K = 128 or the exact builder.
bool direct_input(const QcnnCtx* c, int n) {
  if (c->keepAll || c->L == 0 || c->layers[0].type != QCNN_CONV) return false;
  if (c->calib.armed && c->calib.wantsInput) return false;     // an armed calibration of layer 0 reads fm[0] as panels
  // the images of THIS forward inside 4 GiB: the in-place kernels keep image offsets in 32 bits
  if ((unsigned long long)n * c->inC * c->inH * c->inW * sizeof(float) >= (1ull << 32)) return false;
  // a first layer that runs through its decoded code words reads packed panels — unless its kernel has the NCHW form
  // (k_conv_dec_nchw); batches of one to three images go to the few-image table kernel below, which reads NCHW densely
  if (decoded_layer(c, 0) && !(c->smallBatch && c->lutMode == 1 && n <= kSmallBatchMax)) return c->directDec && c->shapes[0].decNV > 0;
  const QcnnLayerDesc& d = c->layers[0];
  // table kernels: ONE sub-space (a second one would be fetched from channel planes past the group's own, for the last
  // image past the caller's buffer)
  if (c->shapes[0].dense || c->shapes[0].M != 1) return false;
  return c->inC / d.grpCnt <= 4 && (c->lutMode == 0 || c->shapes[0].K == 128);
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

// The layers of one forward.  The batch is cut into up to nStreams sub-batches of whole panels; sub-batch 0
// runs on the context's stream, the others on auxiliary streams forked from / joined to it with events, so
// that the LDS-bound conv/FC kernels of one sub-batch overlap the HBM-bound glue kernels of another and the
// last dispatch round of one kernel is filled by the next.  Every image still sees exactly the same
// arithmetic (panels are independent), so results do not depend on the number of streams.
// pa / pb: the panels [pa, pb) of the batch this call runs (pb < 0: all of them) — a large host batch goes through in
// chunks whose uploads overlap the previous chunk's layers, all chunks writing into the same whole-batch feature maps
int run_layers(QcnnCtx* c, int n, const float* inNchw = nullptr, int pa = 0, int pb = -1) {
  const int panelsAll = (n + QCNN_PANEL - 1) / QCNN_PANEL;
  if (pb < 0) pb = panelsAll;
  const int panels = pb - pa;
  const int ns = std::max(1, std::min(std::min(c->nStreams, kMaxStreams), panels));
  // A batch of a few images: conv/FC by the channel-lane kernels, glue kernels on the live lanes only.  Only in the
  // default f32 mode: the exact builder's point is the reference's summation order (which only the panel kernels
  // keep), and modes 2 / 3 study properties of the panel kernels' table builders.
  const bool small = c->smallBatch && c->lutMode == 1 && n <= kSmallBatchMax;
  const int live = panelsAll == 1 ? n : QCNN_PANEL;
  if (c->profile && c->profCount == kProfRing && drain_profile(c)) return 1;   // ring full: fold it into the sums
  const bool prof = c->profile != 0;
  // pointer table of THIS call (aliases; nullptr = not materialised by this call: the network input read in place, the
  // normalised map of a fused LRN + pool pair); it becomes / is merged into the context's table at the end
  std::vector<float*> fm(c->L + 1, nullptr);
  fm[0] = inNchw ? nullptr : c->fmBuf[0];
  // LRN + the 3x3 / stride 2 / pad 0 max-pool behind it run as one kernel on the fast path when every sub-batch
  // fills the chip with it; the normalised map is then not materialised (qcnn_get_feature_map reports it missing)
  auto lrn_pool = [&](int l) {
    if (c->keepAll || small || l + 1 >= c->L) return false;
    const QcnnLayerDesc& a = c->layers[l];
    const QcnnLayerDesc& b = c->layers[l + 1];
    if (a.type != QCNN_LORN || b.type != QCNN_POOL || (a.lrnSiz != 5 && a.lrnSiz != 3)) return false;
    if (b.knlSiz != 3 || b.stride != 2 || b.padSiz != 0) return false;
    return (long long)qk_lrn_pool_blocks(c->dims[l + 2].h, c->dims[l + 2].w) * (panels / ns) >= lrn_pool_min_blocks();
  };
  for (int l = 0; l < c->L; ++l) {              // pointer table (aliases) — identical for every sub-batch
    const int type = c->layers[l].type;
    const bool prevFused = l > 0 && !c->keepAll && type == QCNN_RELU &&
                           (c->layers[l - 1].type == QCNN_CONV || c->layers[l - 1].type == QCNN_FCNT);
    fm[l + 1] = (type == QCNN_DRPT || prevFused) ? fm[l] : c->fmBuf[l + 1];
    if (lrn_pool(l)) fm[l + 1] = nullptr;
  }
  for (int k = 0; k < ns - 1; ++k) {                 // auxiliary streams of the sub-batches, created when first needed
    if (!c->aux[k]) HIP_TRY(c, hipStreamCreateWithFlags(&c->aux[k], hipStreamNonBlocking));
    if (!c->evJoin[k]) HIP_TRY(c, hipEventCreateWithFlags(&c->evJoin[k], hipEventDisableTiming));
  }
  if (ns > 1) {
    HIP_TRY(c, hipEventRecord(c->evFork, c->stream));
    for (int k = 1; k < ns; ++k) HIP_TRY(c, hipStreamWaitEvent(c->aux[k - 1], c->evFork, 0));
  }
  for (int l = 0; l < c->L; ++l) {              // layer-major issue order: the streams advance together
    const int type = c->layers[l].type;
    if (fm[l + 1] == fm[l] && fm[l] != nullptr) continue;   // alias: copy semantics, no traffic
    if (fm[l] == nullptr && l > 0) continue;                               // the pool of a fused LRN + pool pair
    const bool lrnPool = fm[l + 1] == nullptr;
    const bool fuse = !c->keepAll && (type == QCNN_CONV || type == QCNN_FCNT) && l + 1 < c->L &&
                      c->layers[l + 1].type == QCNN_RELU;
    for (int k = 0; k < ns; ++k) {
      const int p0 = pa + (int)((long long)panels * k / ns), p1 = pa + (int)((long long)panels * (k + 1) / ns);
      if (p1 <= p0) continue;
      hipStream_t st = k == 0 ? c->stream : c->aux[k - 1];
      const bool direct = l == 0 && inNchw != nullptr;
      const float* src = direct ? nullptr : fm[l] + (size_t)p0 * fm_elems(c, l) * QCNN_PANEL;
      float* dst = lrnPool ? fm[l + 2] + (size_t)p0 * fm_elems(c, l + 2) * QCNN_PANEL
                           : fm[l + 1] + (size_t)p0 * fm_elems(c, l + 1) * QCNN_PANEL;
      hipEvent_t e0 = nullptr, e1 = nullptr;
      if (prof) {
        const size_t slot = (((size_t)c->profCount * kMaxStreams + k) * c->L + l) * 2;
        e0 = c->ev[slot]; e1 = c->ev[slot + 1];
        HIP_TRY(c, hipEventRecord(e0, st));
      }
      if (lrnPool) {
        const QcnnLayerDesc& d = c->layers[l];
        const hipError_t e = qk_lrn_pool(src, dst, p1 - p0, c->dims[l].h, c->dims[l].w, c->dims[l].c, c->dims[l + 2].h,
                                         c->dims[l + 2].w, d.lrnSiz, d.lrnAlp, d.lrnBet, d.lrnIni, live, st);
        if (e != hipSuccess) return fail(c, "layer %d (LRN + pool): %s", l, hipGetErrorString(e));
      } else {
        Launch L = {src, dst, p1 - p0, p0, st};
        L.inNchw = direct ? inNchw : nullptr; L.nImages = n; L.live = live; L.small = small;
        L.sub = k; L.nsub = ns; L.panelsAll = panels; L.fuseRelu = fuse;
        if (launch_layer(c, l, L)) return 1;
      }
      if (prof) {
        HIP_TRY(c, hipEventRecord(e1, st));
        c->profPending.push_back(QcnnCtx::ProfRec{(((size_t)c->profCount * kMaxStreams + k) * c->L + l) * 2, l});
      }
    }
  }
  for (int k = 1; k < ns; ++k) {
    HIP_TRY(c, hipEventRecord(c->evJoin[k - 1], c->aux[k - 1]));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evJoin[k - 1], 0));
  }
  if (c->calib.armed && calib_enqueue(c, fm, n, pa, pb)) return 1;
  if (prof) c->profCount++;
  // what can be read back afterwards: a map exists only if every chunk of the batch materialised it
  if (pa == 0 || (int)c->lastFm.size() != c->L + 1) {
    c->lastFm = fm;
  } else {
    for (int l = 0; l <= c->L; ++l)
      if (fm[l] == nullptr) c->lastFm[l] = nullptr;
  }
  c->lastN = n;
  return 0;
}

}  // namespace

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
    case QCNN_OPT_DEC_BF16SPLIT: c->decSplit = value ? 1 : 0; return 0;
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

int qcnn_model_set_layer_weights(QcnnCtx* c, int layer, const float* bias, const float* weights_file) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "qcnn_model_commit must precede qcnn_model_set_layer_weights");
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const QcnnLayerDesc& d = c->layers[layer];
  LayerShape& s = c->shapes[layer];
  if (!s.dense) return fail(c, "layer %d was not declared dense (qcnn_model_set_layer_dense)", layer);
  const int Ct = c->dims[layer + 1].c;
  const int grp = (d.type == QCNN_CONV) ? d.grpCnt : 1;
  const int taps = (d.type == QCNN_CONV) ? d.knlSiz * d.knlSiz : 1;
  const int Cg = (d.type == QCNN_CONV) ? c->dims[layer].c / grp : (int)fm_elems(c, layer);
  const int Ctg = Ct / grp;
  // file layout [Ct][Cg][kh][kw] (convKnl) / [Ct][D] (fcntWei)  ->  [grp][tap][Cg][Ctg], output channel innermost
  std::vector<float> wt(s.denseFloats);
  for (int g = 0; g < grp; ++g)
    for (int ch = 0; ch < Ctg; ++ch)
      for (int ci = 0; ci < Cg; ++ci)
        for (int t = 0; t < taps; ++t)
          wt[(((size_t)g * taps + t) * Cg + ci) * Ctg + ch] = weights_file[(((size_t)(g * Ctg + ch)) * Cg + ci) * taps + t];
  HIP_TRY(c, hipMemcpyAsync(c->arena + s.offBias, bias, sizeof(float) * Ct, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->arena + s.offDense, wt.data(), sizeof(float) * wt.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  s.loaded = true;
  return 0;
}

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
}  // namespace

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

namespace {
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

namespace {
// bias + code book (PrepCtrdBuf permutation; the eight-wave kernels' operand orders) into the arena
int upload_bias_ctrd(QcnnCtx* c, int layer, const float* bias, const float* ctrd_file) {
  LayerShape& s = c->shapes[layer];
  const int Ct = c->dims[layer + 1].c;
  const int M = s.M, K = s.K, Cs = s.Cs;
  // PrepCtrdBuf: [M][K][Cs] -> [M][Cs][K]  (src/CaffeEva.cc:556-557)
  std::vector<float> ctrd((size_t)M * Cs * K);
  for (int m = 0; m < M; ++m)
    for (int k = 0; k < K; ++k)
      for (int dd = 0; dd < Cs; ++dd) ctrd[((size_t)m * Cs + dd) * K + k] = ctrd_file[((size_t)m * K + k) * Cs + dd];
  // the eight-wave kernels' operand orders: FC (K = 32, Cs = 4) qk_ctrdf_index, conv (K = 128, Cs = 4 or 8) qk_ctrd8_index
  std::vector<float> book[BOOK_COUNT];
  for (int b = 0; b < BOOK_COUNT; ++b) {
    if (!s.hasBook[b]) continue;
    book[b].resize(ctrd.size());
    for (int m = 0; m < M; ++m)
      for (int dd = 0; dd < Cs; ++dd)
        for (int k = 0; k < K; ++k)
          book[b][b == BOOK_FC8 ? qk_ctrdf_index(m, dd, k) : qk_ctrd8_index(m, dd, k, Cs / 4)] = ctrd[((size_t)m * Cs + dd) * K + k];
    HIP_TRY(c, hipMemcpyAsync(c->arena + s.offBook[b], book[b].data(), book[b].size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(c->arena + s.offBias, bias, sizeof(float) * Ct, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->arena + s.offCtrd, ctrd.data(), sizeof(float) * ctrd.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // the host vectors die with this scope
  return 0;
}
}  // namespace

namespace {
// FC layer: the assignments (file order [Ct][M], 0-based code words) bit-packed exactly as a .cbn payload of the layer's own
// width (cbn_put) into the arena: the resident form the few-image kernel reads in place
int upload_packed_assignments(QcnnCtx* c, int layer, const uint8_t* asmt_file) {
  const LayerShape& s = c->shapes[layer];
  if (!s.tab[T_CBN].bytes) return 0;
  const size_t n = (size_t)c->dims[layer + 1].c * s.M;
  std::vector<uint8_t> blocks(s.tab[T_CBN].bytes, 0);
  for (size_t e = 0; e < n; ++e) cbn_put(blocks.data(), e, s.cbnBits, asmt_file[e]);
  HIP_TRY(c, hipMemcpyAsync(c->arena + s.tab[T_CBN].off, blocks.data(), blocks.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

// assignment rows of a layer (already in the arena, same stream) -> its decoded code words and every table of kTables it has
hipError_t build_program(QcnnCtx* c, int layer) {
  const QcnnLayerDesc& d = c->layers[layer];
  const LayerShape& s = c->shapes[layer];
  const TableGeom g = table_geom(c, layer);
  const QkSlots& sl = g.sl;
  const uint8_t* rows = arena_at<const uint8_t>(c, s.offAsmt);
  const float* ctrd = arena_at<const float>(c, s.offCtrd);
  const int Cin = c->dims[layer].c, Ct = c->dims[layer + 1].c;
  hipError_t e = hipSuccess;
  if (s.decKp < 0)                  // FC layer with one-dim sub-spaces
    e = qk_decode_fc_weights(rows, ctrd, arena_at<float>(c, s.offDec), sl, (int)fm_elems(c, layer), s.K, Ct, s.decS, c->stream);
  if (s.decKp > 0)                  // one sub-space of <= 4 dims: the code word every assignment names (qcnn_decoded.hip)
    e = qk_decode_weights(rows, ctrd, arena_at<float>(c, s.offDec), sl, d.knlSiz, Cin, s.K, Ct, s.decKp, s.decS, c->stream);
  if (e == hipSuccess && s.decKp > 0 && s.decNV)
    e = qk_decode_weights_nchw(rows, ctrd, arena_at<float>(c, s.offDecN), sl, d.knlSiz, Cin, s.K, Ct, s.decNV, Ct, c->stream);
  if (e == hipSuccess && s.decKp > 0 && s.decNV && s.decBK)
    e = qk_decode_weights_split(rows, ctrd, arena_at<uint16_t>(c, s.offDecB), sl, d.knlSiz, Cin, s.K, Ct, s.decBK, c->stream);
  for (int k = 0; k < T_COUNT && e == hipSuccess; ++k)
    if (s.tab[k].bytes && kTables[k].build) e = kTables[k].build(g, rows, arena_at<uint16_t>(c, s.tab[k].off), c->stream, 0);
  return e;
}
}  // namespace

int qcnn_model_set_layer_params(QcnnCtx* c, int layer, const float* bias, const float* ctrd_file,
                                const uint8_t* asmt_file) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "qcnn_model_commit must precede qcnn_model_set_layer_params");
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const QcnnLayerDesc& d = c->layers[layer];
  LayerShape& s = c->shapes[layer];
  if (s.K <= 0) return fail(c, "layer %d carries no quantised parameters", layer);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drop_f16_programs(s);
  const int Ct = c->dims[layer + 1].c;
  std::vector<float> ctrdX;
  std::vector<uint8_t> asmtX;
  if (s.P > 1) {
    // file layout (Mfile, Kfile) -> pseudo sub-spaces (M = P * Mfile, K = 128): pseudo sub-space j of m holds code words 127 j .. 127 j +
    // 126 in its rows 0 .. 126 and zeros in row 127; an assignment v becomes row v % 127 of pseudo sub-space v / 127, row 127 elsewhere
    const size_t tapsX = (d.type == QCNN_CONV) ? (size_t)d.knlSiz * d.knlSiz : 1;
    const int P = s.P, Mf = s.Mfile, Kf = s.Kfile, Cs = s.Cs;
    ctrdX.assign((size_t)s.M * 128 * Cs, 0.0f);
    for (int m = 0; m < Mf; ++m)
      for (int k = 0; k < Kf; ++k)
        for (int dd = 0; dd < Cs; ++dd)
          ctrdX[(((size_t)m * P + k / 127) * 128 + k % 127) * Cs + dd] = ctrd_file[((size_t)m * Kf + k) * Cs + dd];
    asmtX.resize((size_t)Ct * tapsX * s.M);
    for (size_t e = 0; e < (size_t)Ct * tapsX * Mf; ++e) {
      const unsigned v = asmt_file[e];
      if ((int)v >= Kf) return fail(c, "layer %d: assignment %u >= K = %d", layer, v, Kf);
      for (int j = 0; j < P; ++j) asmtX[e * P + j] = (uint8_t)((int)(v / 127) == j ? v % 127 : 127);
    }
    ctrd_file = ctrdX.data();
    asmt_file = asmtX.data();
  }
  const int M = s.M, K = s.K;
  // PrepAsmtBuf: conv [Ct][kh][kw][M] -> [kh][kw][M][Ct] (:585-586); FC [Ct][M] -> [M][Ct] (:610-611).  Stored as
  // the one-byte SLOT of the code word's row inside a LUT stage (row = (m % G) * K + index < 128; LDS offset = slot * 64),
  // with the channel axis in the order the gather waves consume it (QkSlots); padding entries point at slot 0.
  const int G = qcnn_stage_group(K);
  const size_t taps = (d.type == QCNN_CONV) ? (size_t)d.knlSiz * d.knlSiz : 1;
  const QkSlots sl = table_geom(c, layer).sl;
  std::vector<uint8_t> asmt(s.asmtBytes + QCNN_ROWS_PAD, 0);
  for (int ch = 0; ch < Ct; ++ch) {
    const int entry = qk_slot_entry(sl, ch / sl.C, ch % sl.C);
    for (size_t t = 0; t < taps; ++t)
      for (int m = 0; m < M; ++m) {
        const uint8_t v = asmt_file[((size_t)ch * taps + t) * M + m];
        if (v >= K) return fail(c, "layer %d: assignment %u >= K = %d", layer, (unsigned)v, K);
        asmt[(t * M + m) * sl.rowStride + entry] = (uint8_t)qcnn_row_slot((m % G) * K + v);
      }
  }
  if (upload_bias_ctrd(c, layer, bias, ctrd_file)) return 1;
  if (upload_packed_assignments(c, layer, asmt_file)) return 1;
  HIP_TRY(c, hipMemcpyAsync(c->arena + s.offAsmt, asmt.data(), asmt.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, build_program(c, layer));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  s.loaded = true;
  return 0;
}

int qcnn_model_set_layer_params_cbn(QcnnCtx* c, int layer, const float* bias, const float* ctrd_file,
                                    const uint8_t* cbn_blocks, size_t cbn_bytes, int bits) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "qcnn_model_commit must precede qcnn_model_set_layer_params_cbn");
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const QcnnLayerDesc& d = c->layers[layer];
  LayerShape& s = c->shapes[layer];
  if (s.K <= 0) return fail(c, "layer %d carries no parameters", layer);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  drop_f16_programs(s);
  if (bits < 1 || bits > 8) return fail(c, "layer %d: %d bits per assignment (1..8 supported)", layer, bits);
  const int Ct = c->dims[layer + 1].c;
  const size_t taps = (d.type == QCNN_CONV) ? (size_t)d.knlSiz * d.knlSiz : 1;
  if (s.P > 1) {                        // more than 128 code words: unpacked here, expanded into pseudo sub-spaces by the byte path
    const size_t nF = (size_t)Ct * taps * s.Mfile;
    if (cbn_bytes < cbn_size(nF, bits)) return fail(c, "layer %d: %zu bytes of packed assignments, %zu needed", layer, cbn_bytes, cbn_size(nF, bits));
    std::vector<uint8_t> vals(nF);
    for (size_t e = 0; e < nF; ++e) vals[e] = (uint8_t)cbn_get(cbn_blocks, e, bits);
    return qcnn_model_set_layer_params(c, layer, bias, ctrd_file, vals.data());
  }
  const QkSlots sl = table_geom(c, layer).sl;
  const size_t n = (size_t)Ct * taps * s.M;
  const size_t need = cbn_size(n, bits);
  if (cbn_bytes < need) return fail(c, "layer %d: %zu bytes of packed assignments, %zu needed", layer, cbn_bytes, need);
  if (upload_bias_ctrd(c, layer, bias, ctrd_file)) return 1;
  if (s.tab[T_CBN].bytes && bits != s.cbnBits) {           // a stream of another width: re-packed at the layer's own width for the resident copy
    std::vector<uint8_t> vals(n);
    bool bad = false;
    for (size_t e = 0; e < n; ++e) {
      vals[e] = (uint8_t)cbn_get(cbn_blocks, e, bits);
      bad = bad || vals[e] >= s.K;
    }
    if (bad) return fail(c, "layer %d: an assignment >= K = %d in the packed stream", layer, s.K);
    if (upload_packed_assignments(c, layer, vals.data())) return 1;
  }
  uint8_t* dev = nullptr;
  int* bad = nullptr;
  HIP_TRY(c, hipMalloc(&dev, need + sizeof(int)));
  bad = reinterpret_cast<int*>(dev + need);
  hipError_t e = hipMemcpyAsync(dev, cbn_blocks, need, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && s.tab[T_CBN].bytes && bits == s.cbnBits)       // the payload itself is the resident packed form
    e = hipMemcpyAsync(c->arena + s.tab[T_CBN].off, dev, std::min(need, s.tab[T_CBN].bytes), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(bad, 0, sizeof(int), c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->arena + s.offAsmt, 0, s.asmtBytes + QCNN_ROWS_PAD, c->stream);   // padding entries -> row 0
  if (e == hipSuccess)
    e = qk_decode_cbn(dev, bits, n, Ct, (int)taps, s.M, s.K, sl, reinterpret_cast<uint8_t*>(c->arena + s.offAsmt), bad, c->stream);
  if (e == hipSuccess) e = build_program(c, layer);
  int flag = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&flag, bad, sizeof(int), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(dev);
  if (e != hipSuccess) return fail(c, "layer %d: device-side assignment decode failed: %s", layer, hipGetErrorString(e));
  if (flag) return fail(c, "layer %d: an assignment >= K = %d in the packed stream", layer, s.K);
  s.loaded = true;
  return 0;
}

/* Mark every conv/FC layer as loaded without uploading: the arena was filled by a broadcast. */
int qcnn_model_mark_loaded(QcnnCtx* c) {
  if (!c->committed) return fail(c, "model not committed");
  // The arena may have been REfilled (a re-upload on rank 0 + a second broadcast, or a caller-owned arena written again): the
  // lazily built fp16 program tables (QCNN_OPT_LUT_MODE = 2 / 3) were derived from the OLD assignment bytes — drop them, they are
  // rebuilt from the arena on the next forward that needs them.  Nothing may still be reading them.
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < kMaxStreams - 1; ++k)
    if (c->aux[k]) HIP_TRY(c, hipStreamSynchronize(c->aux[k]));
  for (int l = 0; l < c->L; ++l) {
    drop_f16_programs(c->shapes[l]);
    if (c->shapes[l].K > 0 || c->shapes[l].dense) c->shapes[l].loaded = true;
  }
  return 0;
}

int qcnn_fm_dims(QcnnCtx* c, int l, int* hwc3) {
  if (l < 0 || l > c->L) return fail(c, "feature map %d out of range", l);
  hwc3[0] = c->dims[l].h; hwc3[1] = c->dims[l].w; hwc3[2] = c->dims[l].c;
  return 0;
}

namespace {
// output conversion of a map of panels [classes][128]: probabilities [n][classes], top-5 [n][5]
int map_outputs(QcnnCtx* c, const float* map, int n, float* prob_dev, uint16_t* top5_dev) {
  const int classes = (int)fm_elems(c, c->L);
  hipError_t e;
  if (prob_dev) {
    e = qk_unpack_rows(map, prob_dev, n, classes, c->stream);
    if (e != hipSuccess) return fail(c, "output unpack launch failed: %s", hipGetErrorString(e));
  }
  if (top5_dev) {
    e = qk_top5(map, top5_dev, n, classes, c->stream);
    if (e != hipSuccess) return fail(c, "top-5 launch failed: %s", hipGetErrorString(e));
  }
  return 0;
}
// output conversion of a finished layer loop
int forward_outputs(QcnnCtx* c, int n, float* prob_dev, uint16_t* top5_dev) {
  return map_outputs(c, c->lastFm[c->L], n, prob_dev, top5_dev);
}
// layers + output conversion of a forward whose input panel (fmBuf[0]) has just been enqueued
int forward_tail(QcnnCtx* c, int n, float* prob_dev, uint16_t* top5_dev, const float* inNchw = nullptr) {
  if (run_layers(c, n, inNchw)) return 1;
  return forward_outputs(c, n, prob_dev, top5_dev);
}
}  // namespace

int qcnn_forward(QcnnCtx* c, const float* in_nchw_dev, int n, float* prob_dev, uint16_t* top5_dev) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (n <= 0 || n > c->maxBatch) return fail(c, "batch %d outside (0, %d]", n, c->maxBatch);
  if (direct_input(c, n)) return forward_tail(c, n, prob_dev, top5_dev, in_nchw_dev);   // conv1's builders read it in place
  hipError_t e = qk_pack_nchw(in_nchw_dev, c->fmBuf[0], n, c->inC, c->inH, c->inW, c->stream);
  if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
  return forward_tail(c, n, prob_dev, top5_dev);
}

int qcnn_forward_u8(QcnnCtx* c, const uint8_t* in_u8_dev, int src_h, int src_w, const float* mean_dev, int n,
                    float* prob_dev, uint16_t* top5_dev) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (n <= 0 || n > c->maxBatch) return fail(c, "batch %d outside (0, %d]", n, c->maxBatch);
  if (src_h < c->inH || src_w < c->inW)
    return fail(c, "source images %dx%d are smaller than the network input %dx%d", src_h, src_w, c->inH, c->inW);
  hipError_t e = qk_pack_u8(in_u8_dev, mean_dev, c->fmBuf[0], n, c->inC, c->inH, c->inW, src_h, src_w, c->stream);
  if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
  return forward_tail(c, n, prob_dev, top5_dev);
}

int qcnn_views_ten_crop(int src_h, int src_w, int in_h, int in_w, QcnnView* views10) {
  if (!views10 || in_h <= 0 || in_w <= 0 || src_h < in_h || src_w < in_w) return 1;
  const int Y = src_h - in_h, X = src_w - in_w;
  const int five[5][2] = {{0, 0}, {0, X}, {Y, 0}, {Y, X}, {Y / 2, X / 2}};
  for (int k = 0; k < 10; ++k) views10[k] = QcnnView{five[k % 5][0], five[k % 5][1], k / 5};
  return 0;
}

static_assert(QK_MAX_VIEWS == QCNN_MAX_VIEWS, "the kernel-argument view table holds QCNN_MAX_VIEWS entries");

namespace {
// The multi-view calls around their pack kernel.  views_scratch (BEFORE the pack is launched): the map of the averaged rows is
// large enough for n images.  views_tail: the layers on the n * n_views slots in fm[0], the un-averaged rows, the mean, top-5.
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
// Source image i: its sides (at least 1 for a Strict, 2 for a Relaxed resize), its size, its place in the source buffer.
int src_image_ok(QcnnCtx* c, int i, const QcnnSrcImage& s, size_t src_bytes, int minSide) {
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
int src_pixels_ok(QcnnCtx* c, int i, const QcnnSrcPixels& s, size_t src_bytes, int minSide) {
  char why[256];
  if (qcnn_src::check_pixels(s, c->inC, src_bytes, minSide, why, sizeof(why))) return fail(c, "image %d: %s", i, why);
  return 0;
}
// The layout of a checked descriptor as the kernels take it: row_stride's low 32 bits (they differ from it only where h == 1).
QkLayout layout_of(const QcnnSrcPixels& s) {
  return QkLayout{(int)(uint32_t)(uint64_t)s.row_stride, s.pix_stride, s.ch_offset[0], s.ch_offset[1], s.ch_offset[2], s.ch_offset[3]};
}
// Source image i of a YCbCr call: the same for three sample planes (qcnn_src_yuv.h holds the rules).
int src_yuv_ok(QcnnCtx* c, int i, const QcnnSrcYuv& s, size_t src_bytes, int minSide) {
  char why[320];
  if (qcnn_yuv::check_yuv(s, c->inC, src_bytes, minSide, why, sizeof(why))) return fail(c, "image %d: %s", i, why);
  return 0;
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
// Stage n descriptors D — fill(i) makes image i's — and launch the pack kernel that reads them.  Called when every argument
// is good: nothing is taken or rewritten for a call that is refused.  The set is marked in flight only once nothing of the
// host's can fail any more, and its event is recorded behind its one reader.  afterPack (or nullptr): a second event recorded
// there — the pack kernel is the last reader of the source buffer too (the streamed calls hand the buffer back on it).
extern "C++" template <class D, class Fill, class Launch>
int stage_and_pack(QcnnCtx* c, int n, bool wantMean, hipEvent_t afterPack, Fill fill, Launch launch) {
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
}  // namespace

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

namespace {
// What the planar, the strided and the YCbCr calls differ in, by the type of the caller's descriptor: its check, the image part of the
// staged descriptor, the staged descriptor itself and the pack launch.
extern "C++" {                                      // overloads
int src_ok(QcnnCtx* c, int i, const QcnnSrcImage& s, size_t src_bytes, int minSide) { return src_image_ok(c, i, s, src_bytes, minSide); }
int src_ok(QcnnCtx* c, int i, const QcnnSrcPixels& s, size_t src_bytes, int minSide) { return src_pixels_ok(c, i, s, src_bytes, minSide); }
int src_ok(QcnnCtx* c, int i, const QcnnSrcYuv& s, size_t src_bytes, int minSide) { return src_yuv_ok(c, i, s, src_bytes, minSide); }
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
}  // extern "C++"

// What the two pre-processing modes differ in: the caller's view type and its check, the check of one source image, the staged
// descriptor and the pack launch.  Everything around them — one batch on the device (u8_views) and batches streamed from host
// memory (u8_host_batches) — is written once.
extern "C++" {
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
}  // extern "C++"
}  // namespace

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

// The reference's image loop (src/CaffeEva.cc:151-211) classifies one batch after the other; here the upload of batch
// b + 1 (copy stream, second input buffer) runs under the layers of batch b, and the results come back through pinned
// buffers one batch late, so that neither direction of PCIe is ever waited for by the kernels.
int qcnn_forward_host_batches(QcnnCtx* c, const float* const* in_host, const int* n, int nb, float* const* prob_host,
                              uint16_t* const* top5_host) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (nb <= 0 || !in_host || !n) return fail(c, "qcnn_forward_host_batches: no batches");
  for (int b = 0; b < nb; ++b)
    if (n[b] <= 0 || n[b] > c->maxBatch || !in_host[b]) return fail(c, "batch %d: %d images outside (0, %d]", b, n[b], c->maxBatch);
  if (ensure_pipeline(c)) return 1;
  const size_t inE = fm_elems(c, 0);
  const size_t classes = fm_elems(c, c->L);
  float* const dIn[2] = {c->stageIn, c->stageIn1};
  // the copy stream may not touch an input buffer before everything already enqueued on the compute stream has read it
  for (int k = 0; k < 2; ++k) { HIP_TRY(c, hipEventRecord(c->evFreed[k], c->stream)); c->freedValid[k] = true; }
  auto upload = [&](int b) -> int {
    const int k = b & 1;
    if (c->freedValid[k]) HIP_TRY(c, hipStreamWaitEvent(c->copyStream, c->evFreed[k], 0));
    HIP_TRY(c, hipMemcpyAsync(dIn[k], in_host[b], inE * n[b] * sizeof(float), hipMemcpyHostToDevice, c->copyStream));
    HIP_TRY(c, hipEventRecord(c->evCopied[k], c->copyStream));
    return 0;
  };
  auto collect = [&](int b) -> int {
    const int k = b & 1;
    HIP_TRY(c, hipEventSynchronize(c->evDone[k]));
    if (prob_host && prob_host[b]) memcpy(prob_host[b], c->pinProb[k], (size_t)n[b] * classes * sizeof(float));
    if (top5_host && top5_host[b]) memcpy(top5_host[b], c->pinTop5[k], (size_t)n[b] * 5 * sizeof(uint16_t));
    return 0;
  };
  // QCNN_DEBUG_PIPELINE=1: time every upload and every batch's kernels with events and print the schedule afterwards
  static const bool dbg = [] { const char* e = getenv("QCNN_DEBUG_PIPELINE"); return e && atoi(e) != 0; }();
  std::vector<hipEvent_t> dbgEv;
  if (dbg) {
    dbgEv.resize((size_t)nb * 4 + 1);
    for (hipEvent_t& e : dbgEv) HIP_TRY(c, hipEventCreate(&e));
    HIP_TRY(c, hipEventRecord(dbgEv[(size_t)nb * 4], c->stream));
  }
  auto uploadT = [&](int b) -> int {
    if (!dbg) return upload(b);
    const int k = b & 1;
    if (c->freedValid[k]) HIP_TRY(c, hipStreamWaitEvent(c->copyStream, c->evFreed[k], 0));
    HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4], c->copyStream));
    HIP_TRY(c, hipMemcpyAsync(dIn[k], in_host[b], inE * n[b] * sizeof(float), hipMemcpyHostToDevice, c->copyStream));
    HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + 1], c->copyStream));
    HIP_TRY(c, hipEventRecord(c->evCopied[k], c->copyStream));
    return 0;
  };
  if (uploadT(0)) return 1;
  for (int b = 0; b < nb; ++b) {
    const int k = b & 1;
    if (b + 1 < nb && uploadT(b + 1)) return 1;
    const bool wantProb = prob_host && prob_host[b], wantTop5 = top5_host && top5_host[b];
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evCopied[k], 0));
    if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + 2], c->stream));
    if (qcnn_forward(c, dIn[k], n[b], wantProb ? c->stageOut : nullptr, wantTop5 ? c->stageTop5 : nullptr)) return 1;
    if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + 3], c->stream));
    HIP_TRY(c, hipEventRecord(c->evFreed[k], c->stream));
    if (wantProb)
      HIP_TRY(c, hipMemcpyAsync(c->pinProb[k], c->stageOut, (size_t)n[b] * classes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (wantTop5)
      HIP_TRY(c, hipMemcpyAsync(c->pinTop5[k], c->stageTop5, (size_t)n[b] * 5 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipEventRecord(c->evDone[k], c->stream));
    if (b >= 1 && collect(b - 1)) return 1;
  }
  if (collect(nb - 1)) return 1;
  HIP_TRY(c, hipStreamSynchronize(c->copyStream));
  if (dbg) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int b = 0; b < nb; ++b) {
      float t[4];
      for (int j = 0; j < 4; ++j) HIP_TRY(c, hipEventElapsedTime(&t[j], dbgEv[(size_t)nb * 4], dbgEv[(size_t)b * 4 + j]));
      fprintf(stderr, "[qcnn pipeline] batch %d (%d images): upload %.2f -> %.2f ms, layers %.2f -> %.2f ms\n", b, n[b], t[0], t[1],
              t[2], t[3]);
    }
    for (hipEvent_t e : dbgEv) (void)hipEventDestroy(e);
  }
  return 0;
}

namespace {
// qcnn_forward_u8_resized_host_batches (Mode = StrictMode) and qcnn_forward_u8_relaxed_host_batches (RelaxedMode): the image
// loop of src/CaffeEva.cc:151-211 with BmpImgIO::Load's work on the device and CalcPredAccu's counting (:263-295) behind every
// labelled batch.  The schedule is qcnn_forward_host_batches', with 8-bit source bytes in place of float crops: the source
// bytes and labels of batch b + 1 go up on the copy stream under the layers of batch b, into the buffer the pack kernel of
// batch b - 1 has handed back; results return through the pinned pairs one batch late.
extern "C++" template <class Mode, class Batch>       // Batch: QcnnU8Batch (strided descriptors) or QcnnU8YuvBatch (YCbCr)
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
  QcnnCtx::U8Stream& s = c->u8s;
  // the copy stream may not touch a source or label buffer before everything already enqueued on the compute stream has read it
  for (int k = 0; k < 2; ++k) { HIP_TRY(c, hipEventRecord(c->evFreed[k], c->stream)); c->freedValid[k] = true; }
  HIP_TRY(c, hipMemsetAsync(s.hits, 0, 5 * sizeof(unsigned long long), c->stream));
  // QCNN_DEBUG_PIPELINE=1: time every upload and every batch's kernels with events and print the schedule afterwards
  static const bool dbg = [] { const char* e = getenv("QCNN_DEBUG_PIPELINE"); return e && atoi(e) != 0; }();
  std::vector<hipEvent_t> dbgEv;
  bool counted[2] = {false, false};
  auto run = [&]() -> int {
    if (dbg) {
      dbgEv.resize((size_t)nb * 4 + 1);
      for (hipEvent_t& e : dbgEv) HIP_TRY(c, hipEventCreate(&e));
      HIP_TRY(c, hipEventRecord(dbgEv[(size_t)nb * 4], c->stream));
    }
    auto upload = [&](int b) -> int {
      const int k = b & 1;
      const Batch& q = batches[b];
      if (q.labels && hits5) {                          // through the pinned pair: the copy of batch b - 2 out of it has passed
        if (b >= 2) HIP_TRY(c, hipEventSynchronize(c->evCopied[k]));
        memcpy(s.pinLabels[k], q.labels, (size_t)q.n * sizeof(uint16_t));
      }
      HIP_TRY(c, hipStreamWaitEvent(c->copyStream, c->evFreed[k], 0));
      if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4], c->copyStream));
      HIP_TRY(c, hipMemcpyAsync(s.src[k], q.src_host, q.src_bytes, hipMemcpyHostToDevice, c->copyStream));
      if (q.labels && hits5) {                          // labels[k]'s last reader is the hit count of batch b - 2, far behind its pack kernel
        if (counted[k]) HIP_TRY(c, hipStreamWaitEvent(c->copyStream, s.evCounted[k], 0));
        HIP_TRY(c, hipMemcpyAsync(s.labels[k], s.pinLabels[k], (size_t)q.n * sizeof(uint16_t), hipMemcpyHostToDevice, c->copyStream));
      }
      if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + 1], c->copyStream));
      HIP_TRY(c, hipEventRecord(c->evCopied[k], c->copyStream));
      return 0;
    };
    auto collect = [&](int b) -> int {
      const int k = b & 1;
      const Batch& q = batches[b];
      HIP_TRY(c, hipEventSynchronize(c->evDone[k]));
      if (q.prob_host) memcpy(q.prob_host, c->pinProb[k], (size_t)q.n * classes * sizeof(float));
      if (q.top5_host) memcpy(q.top5_host, c->pinTop5[k], (size_t)q.n * 5 * sizeof(uint16_t));
      if (q.prob_views_host) memcpy(q.prob_views_host, s.pinRows[k], (size_t)q.n * n_views * classes * sizeof(float));
      return 0;
    };
    if (upload(0)) return 1;
    for (int b = 0; b < nb; ++b) {
      const int k = b & 1;
      const Batch& q = batches[b];
      if (b + 1 < nb && upload(b + 1)) return 1;
      const bool count = q.labels && hits5;
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evCopied[k], 0));
      if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + 2], c->stream));
      if (u8_enqueue<Mode>(c, s.src[k], q.imgs, q.n, full_h, full_w, mean_dev, views, n_views, q.prob_host ? s.prob : nullptr,
                           q.top5_host || count ? s.top5 : nullptr, q.prob_views_host ? s.rows : nullptr, c->evFreed[k]))
        return 1;
      if (count) {                                      // on the view-averaged rows: n labels, not n * n_views
        const hipError_t e = qk_top5_hits(s.top5, s.labels[k], q.n, s.hits, c->stream);
        if (e != hipSuccess) return fail(c, "hit count launch failed: %s", hipGetErrorString(e));
        HIP_TRY(c, hipEventRecord(s.evCounted[k], c->stream));
        counted[k] = true;
      }
      if (dbg) HIP_TRY(c, hipEventRecord(dbgEv[(size_t)b * 4 + 3], c->stream));
      if (q.prob_host)
        HIP_TRY(c, hipMemcpyAsync(c->pinProb[k], s.prob, (size_t)q.n * classes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      if (q.top5_host)
        HIP_TRY(c, hipMemcpyAsync(c->pinTop5[k], s.top5, (size_t)q.n * 5 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
      if (q.prob_views_host)
        HIP_TRY(c, hipMemcpyAsync(s.pinRows[k], s.rows, (size_t)q.n * n_views * classes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipEventRecord(c->evDone[k], c->stream));
      if (b >= 1 && collect(b - 1)) return 1;
    }
    if (hits5) HIP_TRY(c, hipMemcpyAsync(s.pinHits, s.hits, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    if (collect(nb - 1)) return 1;
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // the five counters: read back once
    HIP_TRY(c, hipStreamSynchronize(c->copyStream));
    return 0;
  };
  if (run()) {                                          // the caller's memory is not read behind a failed call's return
    (void)hipStreamSynchronize(c->copyStream);
    (void)hipStreamSynchronize(c->stream);
    for (hipEvent_t e : dbgEv) if (e) (void)hipEventDestroy(e);
    return 1;
  }
  if (hits5) memcpy(hits5, s.pinHits, 5 * sizeof(unsigned long long));
  if (dbg) {
    for (int b = 0; b < nb; ++b) {
      float t[4];
      for (int j = 0; j < 4; ++j) HIP_TRY(c, hipEventElapsedTime(&t[j], dbgEv[(size_t)nb * 4], dbgEv[(size_t)b * 4 + j]));
      fprintf(stderr, "[qcnn pipeline] batch %d (%d images): upload %.2f -> %.2f ms, layers %.2f -> %.2f ms\n", b, batches[b].n, t[0],
              t[1], t[2], t[3]);
    }
    for (hipEvent_t e : dbgEv) (void)hipEventDestroy(e);
  }
  return 0;
}
}  // namespace

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

int qcnn_count_top5_hits(QcnnCtx* c, const uint16_t* top5_dev, const uint16_t* labels_dev, int n, unsigned long long* hits5_dev) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!top5_dev || !labels_dev || !hits5_dev) return fail(c, "qcnn_count_top5_hits: top5, labels or hits5 == NULL");
  if (n <= 0) return fail(c, "qcnn_count_top5_hits: no image (n = %d)", n);
  const hipError_t e = qk_top5_hits(top5_dev, labels_dev, n, hits5_dev, c->stream);
  if (e != hipSuccess) return fail(c, "hit count launch failed: %s", hipGetErrorString(e));
  return 0;
}

int qcnn_forward_host(QcnnCtx* c, const float* in_nchw_host, int n, float* prob_host, uint16_t* top5_host) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (n <= 0 || n > c->maxBatch) return fail(c, "batch %d outside (0, %d]", n, c->maxBatch);
  const size_t inE = fm_elems(c, 0);
  const int classes = (int)fm_elems(c, c->L);
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
    if (prob_host)
      HIP_TRY(c, hipMemcpyAsync(prob_host, c->stageOut, (size_t)n * classes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (top5_host)
      HIP_TRY(c, hipMemcpyAsync(top5_host, c->stageTop5, (size_t)n * 5 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  if (ensure_stage(c)) return 1;
  HIP_TRY(c, hipMemcpyAsync(c->stageIn, in_nchw_host, inE * n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  if (qcnn_forward(c, c->stageIn, n, prob_host ? c->stageOut : nullptr, top5_host ? c->stageTop5 : nullptr)) return 1;
  if (prob_host)
    HIP_TRY(c, hipMemcpyAsync(prob_host, c->stageOut, (size_t)n * classes * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (top5_host)
    HIP_TRY(c, hipMemcpyAsync(top5_host, c->stageTop5, (size_t)n * 5 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int qcnn_get_layer_output(QcnnCtx* c, int l, int n, float* host_out) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (l < 0 || l > c->L) return fail(c, "feature map %d out of range", l);
  if (n <= 0 || n > c->lastN) return fail(c, "n = %d exceeds the last forward's batch %d", n, c->lastN);
  if ((int)c->lastFm.size() != c->L + 1 || !c->lastFm[l]) return fail(c, "feature map %d is not available", l);
  if (!c->keepAll && l > 0 && (c->layers[l - 1].type == QCNN_CONV || c->layers[l - 1].type == QCNN_FCNT) &&
      l < c->L && c->layers[l].type == QCNN_RELU)
    return fail(c, "feature map %d was fused away (QCNN_OPT_KEEP_ALL = 0)", l);
  if (ensure_stage(c, (size_t)n * fm_elems(c, l))) return 1;
  const int E = (int)fm_elems(c, l);
  hipError_t e = qk_unpack_rows(c->lastFm[l], c->stageOut, n, E, c->stream);
  if (e != hipSuccess) return fail(c, "unpack launch failed: %s", hipGetErrorString(e));
  HIP_TRY(c, hipMemcpyAsync(host_out, c->stageOut, (size_t)n * E * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int qcnn_get_layer_output_range(QcnnCtx* c, int l, int first, int n, float* host_out) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (l < 0 || l > c->L) return fail(c, "feature map %d out of range", l);
  if (first < 0 || n <= 0 || first + n > c->lastN)
    return fail(c, "images [%d, %d) are not inside the last forward's batch of %d", first, first + n, c->lastN);
  if ((int)c->lastFm.size() != c->L + 1 || !c->lastFm[l]) return fail(c, "feature map %d is not available", l);
  if (!c->keepAll && l > 0 && (c->layers[l - 1].type == QCNN_CONV || c->layers[l - 1].type == QCNN_FCNT) &&
      l < c->L && c->layers[l].type == QCNN_RELU)
    return fail(c, "feature map %d was fused away (QCNN_OPT_KEEP_ALL = 0)", l);
  if (ensure_stage(c, (size_t)(n + QCNN_PANEL) * fm_elems(c, l))) return 1;
  const size_t E = fm_elems(c, l);
  const int p0 = first / QCNN_PANEL;                       // whole panels from the one that holds `first`
  const int cnt = first + n - p0 * QCNN_PANEL;
  hipError_t e = qk_unpack_rows(c->lastFm[l] + (size_t)p0 * E * QCNN_PANEL, c->stageOut, cnt, (int)E, c->stream);
  if (e != hipSuccess) return fail(c, "unpack launch failed: %s", hipGetErrorString(e));
  HIP_TRY(c, hipMemcpyAsync(host_out, c->stageOut + (size_t)(first - p0 * QCNN_PANEL) * E, (size_t)n * E * sizeof(float),
                            hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int qcnn_run_layer(QcnnCtx* c, int layer, const float* in_host, int n, float* out_host) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  if (n <= 0 || n > c->maxBatch) return fail(c, "batch %d outside (0, %d]", n, c->maxBatch);
  if (ensure_stage(c, (size_t)n * std::max(fm_elems(c, layer), fm_elems(c, layer + 1)))) return 1;
  const int Ein = (int)fm_elems(c, layer), Eout = (int)fm_elems(c, layer + 1);
  const int panels = (n + QCNN_PANEL - 1) / QCNN_PANEL;
  // scratch: reuse the layer's own input/output maps (sized for maxBatch)
  float* src = c->fmBuf[layer] ? c->fmBuf[layer] : c->fmBuf[layer - 1];
  float* dst = c->fmBuf[layer + 1] ? c->fmBuf[layer + 1] : c->stageOut;
  if (c->layers[layer].type == QCNN_DRPT && !c->fmBuf[layer + 1]) {
    // aliased output map: stage through the linear buffer instead
    memcpy(out_host, in_host, (size_t)n * Ein * sizeof(float));
    return 0;
  }
  HIP_TRY(c, hipMemcpyAsync(c->stageIn, in_host, (size_t)n * Ein * sizeof(float), hipMemcpyHostToDevice, c->stream));
  hipError_t e = qk_pack_rows(c->stageIn, src, n, Ein, c->stream);
  if (e != hipSuccess) return fail(c, "pack launch failed: %s", hipGetErrorString(e));
  Launch L = {src, dst, panels, 0, c->stream};
  L.flatFcInput = true;
  if (launch_layer(c, layer, L)) return 1;
  e = qk_unpack_rows(dst, c->stageOut, n, Eout, c->stream);
  if (e != hipSuccess) return fail(c, "unpack launch failed: %s", hipGetErrorString(e));
  HIP_TRY(c, hipMemcpyAsync(out_host, c->stageOut, (size_t)n * Eout * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return 0;
}

int qcnn_get_layer_split(QcnnCtx* c, int layer, int* tiles_unsplit, int* slices) {
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const LayerShape& s = c->shapes[layer];
  if (tiles_unsplit) *tiles_unsplit = s.lastFrom;
  if (slices) *slices = s.lastZ;
  return 0;
}

int qcnn_get_layer_segments(QcnnCtx* c, int layer, int* seg_beg9, int* n_seg) {
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const LayerShape& s = c->shapes[layer];
  const int n = (s.lastFrom == -2 || s.lastFrom == -6 || s.lastFrom == -10) ? s.segN : 0;
  if (n_seg) *n_seg = n;
  if (seg_beg9)
    for (int i = 0; i < 9; ++i) seg_beg9[i] = (i <= n) ? s.segBeg[i] : 0;
  return 0;
}

int qcnn_get_layer_ms(QcnnCtx* c, float* ms, int* forwards_recorded) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (drain_profile(c)) return 1;
  for (int l = 0; l < c->L; ++l) ms[l] = c->profLaunches[l] ? (float)(c->profSum[l] / c->profLaunches[l]) : 0.0f;
  if (forwards_recorded) *forwards_recorded = c->profForwards;
  return 0;
}

int qcnn_get_layer_total_ms(QcnnCtx* c, double* total_ms, long long* launches, int* forwards_recorded) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (drain_profile(c)) return 1;
  for (int l = 0; l < c->L; ++l) {
    total_ms[l] = c->profSum[l];
    if (launches) launches[l] = c->profLaunches[l];
  }
  if (forwards_recorded) *forwards_recorded = c->profForwards;
  return 0;
}

int qcnn_reset_layer_ms(QcnnCtx* c) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (drain_profile(c)) return 1;
  c->profSum.assign(c->L, 0.0);
  c->profLaunches.assign(c->L, 0);
  c->profForwards = 0;
  return 0;
}

}  // extern "C"
