// qcnn_engine_params.hip — the table-layout descriptors (kTables) and the parameter upload: PrepCtrdBuf / PrepAsmtBuf of the
// reference's CaffeEva (src/CaffeEva.cc:109-149) as qcnn_model_set_layer_params[_cbn] / qcnn_model_set_layer_weights.
#include <algorithm>

#include "qcnn_engine.h"

using namespace qcnn_engine;

namespace {

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

// ------------------------------------------------------------------------------------------------------------------
// kTables: the one place that knows, per TableKind, when a layer has the table and how big it is, and how it is built from the
// arena's assignment rows.  (Layers of pseudo sub-spaces — more than 128 code words, P > 1 — always run the exact-builder
// kernels, which read the plain rows: they have none of these.)
// ------------------------------------------------------------------------------------------------------------------

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
  LayerShape& s = c->shapes[layer];
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
  if (e == hipSuccess && s.decKp > 0 && s.decNV && s.decBK)      // ... and as two fp16 pieces behind the scale the decoder chooses
    e = qk_decode_weights_f16(rows, ctrd, arena_at<const float>(c, s.offBias), arena_at<void>(c, s.offDecH), sl, d.knlSiz, Cin, s.K, Ct, s.decBK, c->stream);
  s.decF16 = -1;                                                 // read back by the first launch that asks (launch_conv)
  for (int k = 0; k < T_COUNT && e == hipSuccess; ++k)
    if (s.tab[k].bytes && kTables[k].build) e = kTables[k].build(g, rows, arena_at<uint16_t>(c, s.tab[k].off), c->stream, 0);
  return e;
}

}  // namespace

namespace qcnn_engine {

int cbn_bits(int K) {               // the reference's CalcBitCntPerEle for K code words (src/CaffePara.cc:360-380)
  int bits = 1;
  while ((1 << bits) < K) ++bits;
  return bits;
}

TableGeom table_geom(const QcnnCtx* c, int l) {
  const QcnnLayerDesc& d = c->layers[l];
  const LayerShape& s = c->shapes[l];
  const int Ct = c->dims[l + 1].c;
  if (d.type == QCNN_CONV) return {true, c->dims[l].c, Ct, d.grpCnt, d.knlSiz, d.stride, s.M, s.Cs, s.K, s.P, qk_conv_slots(Ct / d.grpCnt, d.grpCnt)};
  return {false, (int)fm_elems(c, l), Ct, 1, 1, 1, s.M, s.Cs, s.K, s.P, qk_fc_slots(Ct)};
}

const TableDesc& table_desc(int kind) { return kTables[kind]; }

void drop_f16_programs(LayerShape& s) {
  for (auto& form : s.progF16)
    for (uint16_t*& t : form) {
      if (t) (void)hipFree(t);
      t = nullptr;
    }
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

}  // namespace qcnn_engine

extern "C" {

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
    c->shapes[l].decF16 = -1;                     // the first layer's fp16 scale: whatever the arena holds now
    if (c->shapes[l].K > 0 || c->shapes[l].dense) c->shapes[l].loaded = true;
  }
  return 0;
}

}  // extern "C"
