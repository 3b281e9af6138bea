// qcnn_engine.h — what the translation units behind include/qcnn_hip.h share: the context, the per-layer plan, the launch
// descriptor and the handful of functions that cross files.  Internal: never included from include/.
//
//   qcnn_engine.hip         context, options, model begin / commit, arena plan, and the owner of every context buffer
//   qcnn_engine_params.hip  table-layout descriptors (kTables) and the parameter upload
//   qcnn_engine_run.hip     the layer loop, its launchers, the profile ring, device-side forwards and read-backs
//   qcnn_engine_quant.hip   quantiser and calibration entry points
//   qcnn_engine_u8.hip      the 8-bit multi-view front end and its streamed batches
//   qcnn_engine_host.hip    host-memory forwards and the double-buffered batch schedule
//
// Rule of ownership: the file that frees a buffer also allocates it.  Buffers that live as long as the context or the model
// are qcnn_engine.hip's (free_model / qcnn_ctx_destroy and the ensure_* functions below); the other files ask for them.
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "../../include/qcnn_hip.h"
#include "qcnn_kernels.h"
#include "qcnn_planner.h"

#pragma GCC visibility push(hidden)
namespace qcnn_engine {

// The tables a layer's arena may hold beside bias, code book and the plain assignment rows, in the order plan_arena lays them
// out (kTables, qcnn_engine_params.hip, says when a layer has which, and how it is built)
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
  size_t offDecH = 0;                                          // ... as two fp16 pieces behind their scale Sw for k_conv_dec_nchw_f16 (same decBK)
  int decF16 = -1; float decSw = 0.0f;                         // ... that scale as the decoder left it in the arena: -1 not read back yet (an upload, a
                                                               // broadcast arena), 0 the layer keeps the bf16 form (Sw = 0), 1 eligible
  int lastForm = 0;                                            // decoded first layer: the form of the last launch (0 f32, 1 bf16 pieces, 2 fp16 pieces)
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

}  // namespace qcnn_engine
#pragma GCC visibility pop

// The one type of the C-ABI: at global scope, as include/qcnn_hip.h declares it
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
  int decSplit = 2;                  // QCNN_OPT_DEC_BF16SPLIT: ... with its products as fp32-accurate split MFMAs: 1 three bf16 pieces
                                     // (k_conv_dec_nchw_split), 2 two fp16 pieces where the layer's scale allows (k_conv_dec_nchw_f16), else as 1
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
  std::vector<qcnn_engine::FmDims> dims;          // L + 1
  std::vector<qcnn_engine::LayerShape> shapes;    // L
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
  // k_conv_dec_nchw_f16's range guard: one region per sub-batch stream (word + a 16-bit image mask per item, sized for maxPanels),
  // allocated at the first launch, freed with the model; decEpoch: the number the region's last launch carried, decGuardItems: its
  // items (0: the sub-batch did not run the fp16 form in the last forward) — what qcnn_get_layer_dec_form reads back
  uint32_t* decGuard = nullptr;
  size_t decGuardBytes = 0;          // per region
  uint32_t decEpoch[qcnn_engine::kMaxStreams] = {0};
  int decGuardItems[qcnn_engine::kMaxStreams] = {0};
  float* fcFlat = nullptr;           // first FC layer's input in consumption order
  float* fcPartial = nullptr;        // split-M partial sums of the FC layers
  float* convPartial = nullptr;      // partial sums of split conv tiles (kConvPartialFloats)
  bool noConvPartial = false;        // ... could not be allocated: split plans launch their tiles whole
  size_t fcPartialElems = 0;
  size_t fcMaxCt = 0;
  float* viewMean = nullptr;         // qcnn_forward_u8_views: panels [classes][128] of the probabilities averaged over an image's views —
  size_t viewMeanElems = 0;          // allocated at its first call, grown when one needs more, freed with the context (no part of the plan)
  double* diffScratch = nullptr;     // qcnn_map_diff: per-channel rows + partial rows of its two passes, owned like viewMean
  size_t diffScratchDoubles = 0;
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

#pragma GCC visibility push(hidden)
namespace qcnn_engine {

int fail(QcnnCtx* c, const char* fmt, ...);      // c->err (or, c == nullptr, the create error) = the message; returns 1

#define HIP_TRY(c, call)                                                                  \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) return fail((c), "%s -> %s", #call, hipGetErrorString(e_));     \
  } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

inline int conv_out(int in, int knl, int stride, int pad) { return (in + 2 * pad - knl) / stride + 1; }
inline int pool_out(int in, int knl, int stride, int pad) {          // ceil mode, src/CaffeEva.cc:367-370
  const int num = in + 2 * pad - knl;
  return (num + stride - 1) / stride + 1;
}

inline size_t fm_elems(const QcnnCtx* c, int l) { return (size_t)c->dims[l].h * c->dims[l].w * c->dims[l].c; }

template <class T> T* arena_at(const QcnnCtx* c, size_t off) { return reinterpret_cast<T*>(c->arena + off); }
// a layer's table of one kind; nullptr: it has none
inline const uint16_t* table(const QcnnCtx* c, const LayerShape& s, int kind) {
  return s.tab[kind].bytes ? arena_at<const uint16_t>(c, s.tab[kind].off) : nullptr;
}

// What every forward entry point asks first: the context's device, a committed model, a batch it was committed for.
inline int open_batch(QcnnCtx* c, int n) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (!c->committed) return fail(c, "model not committed");
  if (n <= 0 || n > c->maxBatch) return fail(c, "batch %d outside (0, %d]", n, c->maxBatch);
  return 0;
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

// ---- qcnn_engine.hip: the owners of the context's buffers (each allocates at first use and grows on demand) ----
int ensure_stage(QcnnCtx* c, size_t elems = 0);          // stageIn / stageOut / stageTop5
int ensure_pipeline(QcnnCtx* c);                         // ... + events, pinned results and stageIn1 of the pipelined float path
int ensure_u8_stream(QcnnCtx* c, size_t srcBytes);       // ... + what the 8-bit stream owns (QcnnCtx::U8Stream)
float* ensure_conv_partial(QcnnCtx* c);                  // convPartial; nullptr: the device has no room for it (no error)
uint32_t* ensure_dec_guard(QcnnCtx* c, int sub);         // decGuard's region of sub-batch `sub`; nullptr after fail()
int views_scratch(QcnnCtx* c, int n, bool wantMean);     // viewMean for n images
int diff_scratch(QcnnCtx* c, size_t doubles);            // diffScratch of at least that many doubles
QcnnCtx::SrcStage* stage_take(QcnnCtx* c, size_t n, size_t each);   // the next descriptor staging set; nullptr after fail()

// ---- qcnn_engine_params.hip: kTables, the one place that knows, per TableKind, when a layer has the table, how big it is and
// how it is built from the arena's assignment rows ----
struct TableGeom {
  bool conv;                        // else FC: Cin = its D input dims, grp = knl = stride = 1
  int Cin, Ct, grp, knl, stride;
  int M, Cs, K, P;
  QkSlots sl;                       // of the plain assignment rows (QkSlots, qcnn_kernels.h)
};
struct TableDesc {
  size_t (*bytes)(const TableGeom& g, int v);      // 0: the layer has none.  v = 0: the arena's table; 1 / 2: its fp16 forms (ensure_f16_program)
  hipError_t (*build)(const TableGeom& g, const uint8_t* rows, uint16_t* out, hipStream_t st, int v);
  BookKind book;                                   // the code book in the kernel's operand order goes with it: one copy, laid out
};                                                 // behind the last of the (consecutive) kinds that name it
const TableDesc& table_desc(int kind);         // kTables[kind]
TableGeom table_geom(const QcnnCtx* c, int l);
int cbn_bits(int K);
void drop_f16_programs(LayerShape& s);
const uint16_t* ensure_f16_program(QcnnCtx* c, int l, int kind, hipStream_t st);

// ---- qcnn_engine_run.hip ----
bool direct_input(const QcnnCtx* c, int n);
int run_layers(QcnnCtx* c, int n, const float* inNchw = nullptr, int pa = 0, int pb = -1);
int map_outputs(QcnnCtx* c, const float* map, int n, float* prob_dev, uint16_t* top5_dev);
int forward_outputs(QcnnCtx* c, int n, float* prob_dev, uint16_t* top5_dev);
int forward_tail(QcnnCtx* c, int n, float* prob_dev, uint16_t* top5_dev, const float* inNchw = nullptr);

// ---- qcnn_engine_quant.hip: the resident calibration, as the model (free_model) and the layer loop see it ----
void calib_free(QcnnCtx* c);
int calib_enqueue(QcnnCtx* c, const std::vector<float*>& fm, int n, int pa, int pb);

// ---- qcnn_engine_host.hip: the double-buffered batch schedule.  The upload of batch b + 1 runs on the copy stream under the
// compute step of batch b, results come back through the pinned pairs one batch late.  A job supplies what its caller's
// batches differ in; k = b & 1 names the buffer pair of batch b.  A step returns 0 or, after fail(), 1; an empty one is skipped ----
struct HostResult { const void* dev; void* pin; void* host; size_t bytes; };   // device -> pinned pair -> the caller's memory; host == nullptr: not asked for
struct HostBatchJob {
  std::function<int(int b)> images;                      // of batch b (the debug printout names them)
  std::function<int()> prologue;                         // enqueued on the compute stream behind the initial evFreed records
  std::function<int(int b, int k)> stage;                // host work in front of the upload of batch b
  std::function<int(int b, int k)> upload;               // the copies of batch b, enqueued on the copy stream
  std::function<int(int b, int k, hipEvent_t freed)> compute;   // the compute step; records `freed` behind the last reader of input buffer k
  std::function<std::vector<HostResult>(int b, int k)> results;  // what batch b hands back: downloaded behind compute, copied out one batch late
  std::function<int()> epilogue;                         // enqueued behind the last batch, in front of the last collect
};
int host_batch_schedule(QcnnCtx* c, int nb, const HostBatchJob& job);

}  // namespace qcnn_engine
#pragma GCC visibility pop
