// qcnn_engine_run.hip — the layer loop (ExecForwardPass, src/CaffeEva.cc:184-205, :232-254, as run_layers), the launchers
// of every layer type, the profile ring, the forwards whose input lies on the device, and the read-backs of a finished forward.
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "qcnn_engine.h"

using namespace qcnn_engine;

namespace {

// Does conv layer l run through its decoded code words (qcnn_decoded.hip)?  The f32 MFMA mode only: the exact
// builder keeps the reference's summation order and the fp16 study is about the tables themselves.
bool decoded_layer(const QcnnCtx* c, int l) {
  const LayerShape& s = c->shapes[l];
  return c->decode && s.decKp > 0 && !s.dense && c->lutMode == 1 && c->layers[l].type == QCNN_CONV;
}

int launched(QcnnCtx* c, int l, hipError_t e) {
  if (e != hipSuccess) return fail(c, "layer %d (type %d) launch failed: %s", l, c->layers[l].type, hipGetErrorString(e));
  return 0;
}

// Partial-sum scratch.  Split conv tiles: this sub-batch's share of ensure_conv_partial's buffer; nullptr: there is none, the
// tiles run whole.  FC layers: every sub-batch has its own slab of QK_MAX_FC_SPLIT x (its panels) x (widest layer)
float* conv_partial(QcnnCtx* c, const Launch& L) {
  float* all = ensure_conv_partial(c);
  return all ? all + kConvPartialFloats / (size_t)L.nsub * L.sub : nullptr;
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
    q.accScale = q.outScale = 1.0f; q.guard = nullptr; q.epoch = 0;
    s.lastFrom = -3; s.lastZ = inNchw ? 2 : 1;        // reported by qcnn_get_layer_split as (-3, 1), NCHW in place: (-3, 2)
    const bool splitBf16 = inNchw && c->decSplit && s.decBK > 0;   // fp32-accurate split products (QCNN_OPT_DEC_BF16SPLIT)
    if (splitBf16) { q.Kp = s.decBK; q.wdec = arena_at<const float>(c, s.offDecB); }
    // ... as two fp16 pieces (value 2) when the decoder found a scale for the layer: Sw stands in front of the planes, read back
    // once per upload (uploads end with a synchronised stream; the arena does not change between them)
    if (splitBf16 && c->decSplit == 2 && s.decF16 < 0) {
      HIP_TRY(c, hipMemcpy(&s.decSw, arena_at<const float>(c, s.offDecH), sizeof(float), hipMemcpyDeviceToHost));
      s.decF16 = s.decSw > 0.0f ? 1 : 0;
    }
    if (L.sub == 0) for (int& n : c->decGuardItems) n = 0;    // (what qcnn_get_layer_dec_form counts: this forward's launches)
    hipError_t e;
    if (splitBf16 && c->decSplit == 2 && s.decF16 == 1) {
      if (!(q.guard = ensure_dec_guard(c, L.sub))) return 1;
      if (++c->decEpoch[L.sub] == 0) c->decEpoch[L.sub] = 1;   // never 0 (the regions start zeroed); the word is compared, never cleared
      q.epoch = c->decEpoch[L.sub];
      q.accScale = QK_F16_SX * s.decSw; q.outScale = 1.0f / q.accScale;
      q.wdec = reinterpret_cast<const float*>(arena_at<const char>(c, s.offDecH) + QK_F16_PLANES);
      e = qk_conv_dec_nchw_f16(q, arena_at<const float>(c, s.offDecB), st);
      if (e == hipSuccess) c->decGuardItems[L.sub] = q.panels * b.h * ((b.w + 3) / 4) * ((q.live + 15) / 16) * (b.c / 96);
      s.lastForm = 2;
    } else {
      e = splitBf16 ? qk_conv_dec_nchw_split(q, st) : inNchw ? qk_conv_dec_nchw(q, st) : qk_conv_dec(q, st);
      s.lastForm = splitBf16 ? 1 : 0;
    }
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

// what the two read-backs of a finished forward ask first
int layer_output_ok(QcnnCtx* c, int l) {
  if ((int)c->lastFm.size() != c->L + 1 || !c->lastFm[l]) return fail(c, "feature map %d is not available", l);
  if (!c->keepAll && l > 0 && (c->layers[l - 1].type == QCNN_CONV || c->layers[l - 1].type == QCNN_FCNT) &&
      l < c->L && c->layers[l].type == QCNN_RELU)
    return fail(c, "feature map %d was fused away (QCNN_OPT_KEEP_ALL = 0)", l);
  return 0;
}

}  // namespace

namespace qcnn_engine {

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

// The layers of one forward.  The batch is cut into up to nStreams sub-batches of whole panels; sub-batch 0
// runs on the context's stream, the others on auxiliary streams forked from / joined to it with events, so
// that the LDS-bound conv/FC kernels of one sub-batch overlap the HBM-bound glue kernels of another and the
// last dispatch round of one kernel is filled by the next.  Every image still sees exactly the same
// arithmetic (panels are independent), so results do not depend on the number of streams.
// pa / pb: the panels [pa, pb) of the batch this call runs (pb < 0: all of them) — a large host batch goes through in
// chunks whose uploads overlap the previous chunk's layers, all chunks writing into the same whole-batch feature maps
int run_layers(QcnnCtx* c, int n, const float* inNchw, int pa, int pb) {
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
int forward_tail(QcnnCtx* c, int n, float* prob_dev, uint16_t* top5_dev, const float* inNchw) {
  if (run_layers(c, n, inNchw)) return 1;
  return forward_outputs(c, n, prob_dev, top5_dev);
}

}  // namespace qcnn_engine

extern "C" {

int qcnn_fm_dims(QcnnCtx* c, int l, int* hwc3) {
  if (l < 0 || l > c->L) return fail(c, "feature map %d out of range", l);
  hwc3[0] = c->dims[l].h; hwc3[1] = c->dims[l].w; hwc3[2] = c->dims[l].c;
  return 0;
}

int qcnn_forward(QcnnCtx* c, const float* in_nchw_dev, int n, float* prob_dev, uint16_t* top5_dev) {
  if (open_batch(c, n)) return 1;
  if (direct_input(c, n)) return forward_tail(c, n, prob_dev, top5_dev, in_nchw_dev);   // conv1's builders read it in place
  hipError_t e = qk_pack_nchw(in_nchw_dev, c->fmBuf[0], n, c->inC, c->inH, c->inW, c->stream);
  if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
  return forward_tail(c, n, prob_dev, top5_dev);
}

int qcnn_forward_u8(QcnnCtx* c, const uint8_t* in_u8_dev, int src_h, int src_w, const float* mean_dev, int n,
                    float* prob_dev, uint16_t* top5_dev) {
  if (open_batch(c, n)) return 1;
  if (src_h < c->inH || src_w < c->inW)
    return fail(c, "source images %dx%d are smaller than the network input %dx%d", src_h, src_w, c->inH, c->inW);
  hipError_t e = qk_pack_u8(in_u8_dev, mean_dev, c->fmBuf[0], n, c->inC, c->inH, c->inW, src_h, src_w, c->stream);
  if (e != hipSuccess) return fail(c, "input pack launch failed: %s", hipGetErrorString(e));
  return forward_tail(c, n, prob_dev, top5_dev);
}

int qcnn_get_layer_output(QcnnCtx* c, int l, int n, float* host_out) {
  HIP_TRY(c, hipSetDevice(c->device));
  if (l < 0 || l > c->L) return fail(c, "feature map %d out of range", l);
  if (n <= 0 || n > c->lastN) return fail(c, "n = %d exceeds the last forward's batch %d", n, c->lastN);
  if (layer_output_ok(c, l)) return 1;
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
  if (layer_output_ok(c, l)) return 1;
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

// Map l of c's last forward against the same map of ref's (include/qcnn_hip.h): every check first, then two launches on c's
// stream and C rows of six doubles to the host; the total is folded here from the rows the caller receives.
int qcnn_map_diff(QcnnCtx* c, QcnnCtx* ref, int l, int n, QcnnMapDiff* total_host, QcnnMapDiff* per_channel_host) {
  if (!c) return fail(nullptr, "qcnn_map_diff: ctx == NULL");
  if (!ref) return fail(c, "qcnn_map_diff: ref == NULL");
  if (!total_host) return fail(c, "qcnn_map_diff: total_host == NULL");
  if (c->device != ref->device)
    return fail(c, "qcnn_map_diff: the contexts are on different devices (%d and %d)", c->device, ref->device);
  if (l < 0 || l > c->L) return fail(c, "feature map %d out of range", l);
  if (l > ref->L) return fail(c, "feature map %d out of range of the reference context (%d layers)", l, ref->L);
  if ((int)c->dims.size() != c->L + 1 || (int)ref->dims.size() != ref->L + 1) return fail(c, "feature map %d is not available", l);
  const FmDims da = c->dims[l], db = ref->dims[l];
  if (da.h != db.h || da.w != db.w || da.c != db.c)
    return fail(c, "feature map %d has different dims in the two contexts: %d x %d x %d against %d x %d x %d", l, da.h, da.w, da.c,
                db.h, db.w, db.c);
  if (layer_output_ok(c, l)) return 1;
  if (ref != c && layer_output_ok(ref, l)) return fail(c, "reference context: %s", std::string(ref->err).c_str());
  if (n <= 0) return fail(c, "n = %d: at least one image", n);
  if (n > c->lastN) return fail(c, "n = %d exceeds the last forward's batch %d", n, c->lastN);
  if (n > ref->lastN) return fail(c, "n = %d exceeds the reference context's last forward's batch %d", n, ref->lastN);
  const int HW = da.h * da.w, C = da.c;
  const size_t doubles = qk_map_diff_doubles(HW, C, n);
  if (!doubles) return fail(c, "qcnn_map_diff: feature map %d (%d x %d x %d, %d images) is beyond one launch", l, da.h, da.w, C, n);
  HIP_TRY(c, hipSetDevice(c->device));
  if (diff_scratch(c, doubles)) return 1;
  if (ref != c) HIP_TRY(c, hipStreamSynchronize(ref->stream));     // run_layers joined the auxiliary streams into it
  hipError_t e = qk_map_diff(c->lastFm[l], ref->lastFm[l], HW, C, n, c->diffScratch, c->stream);
  if (e != hipSuccess) return fail(c, "map diff launch failed: %s", hipGetErrorString(e));
  std::vector<QcnnMapDiff> own;
  QcnnMapDiff* rows = per_channel_host;
  if (!rows) { own.resize(C); rows = own.data(); }
  HIP_TRY(c, hipMemcpyAsync(rows, c->diffScratch, (size_t)C * sizeof(QcnnMapDiff), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  QcnnMapDiff t = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int ch = 0; ch < C; ++ch) {                   // ascending channel order, fp64
    t.count += rows[ch].count; t.nonfinite += rows[ch].nonfinite;
    t.sum_d += rows[ch].sum_d; t.sum_d2 += rows[ch].sum_d2; t.sum_ref2 += rows[ch].sum_ref2;
    if (rows[ch].max_abs_d > t.max_abs_d) t.max_abs_d = rows[ch].max_abs_d;
  }
  *total_host = t;
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

int qcnn_get_layer_dec_form(QcnnCtx* c, int layer, int* form, long long* fallback_pairs) {
  if (layer < 0 || layer >= c->L) return fail(c, "layer %d out of range", layer);
  const LayerShape& s = c->shapes[layer];
  const bool inPlace = s.lastFrom == -3 && s.lastZ == 2;
  if (form) *form = inPlace ? s.lastForm : -1;
  if (!fallback_pairs) return 0;
  *fallback_pairs = 0;
  if (!inPlace || s.lastForm != 2 || !c->decGuard) return 0;
  HIP_TRY(c, hipSetDevice(c->device));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < kMaxStreams - 1; ++k)
    if (c->aux[k]) HIP_TRY(c, hipStreamSynchronize(c->aux[k]));
  std::vector<uint16_t> host;
  for (int k = 0; k < kMaxStreams; ++k) {
    const int items = c->decGuardItems[k];
    if (!items) continue;
    host.resize(8 + (size_t)items);                       // the word and its slack, then the masks
    HIP_TRY(c, hipMemcpy(host.data(), reinterpret_cast<const char*>(c->decGuard) + c->decGuardBytes * k, host.size() * sizeof(uint16_t), hipMemcpyDeviceToHost));
    uint32_t word = 0;
    memcpy(&word, host.data(), sizeof(word));
    if (word != c->decEpoch[k]) continue;                 // this launch flagged nothing: its fix-up left at once
    for (int i = 0; i < items; ++i) *fallback_pairs += __builtin_popcount(host[8 + (size_t)i]);
  }
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
