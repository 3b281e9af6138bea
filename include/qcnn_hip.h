/* qcnn_hip.h — C-ABI of the MI355X (gfx950) Quantized-CNN approximate forward pass.
 *
 * This is the drop-in boundary: plain C types, caller-owned host/device buffers,
 * library-owned activations, 0 = OK / non-zero = error + qcnn_last_error().  The host side of this
 * repository (include/CaffeEva.h, quantized-cnn_amd/host/caffe_eva.cc) binds exactly these entry
 * points where the reference's CaffeEva calls its CPU routines; INTEGRATION.md shows the same
 * binding applied to the reference tree.  Built by `hipcc --offload-arch=gfx950` into
 * quantized-cnn_amd/libqcnn_hip.so.  There is no CPU fallback: without a HIP device every compute
 * entry point fails with an error string.
 *
 * Reference interface each entry point replaces (file:line in CAS-CLab/quantized-cnn):
 *   qcnn_model_begin            CaffePara::ConfigLayer_* tables            src/CaffePara.cc:20-237
 *                               + CaffeEva::PrepFeatMap size rule          src/CaffeEva.cc:328-411
 *   qcnn_model_set_layer_params CaffePara::LoadLayerPara result ->         src/CaffePara.cc:239-306
 *                               CaffeEva::PrepCtrdBuf / PrepAsmtBuf        src/CaffeEva.cc:534-623
 *   qcnn_model_set_layer_params_cbn  FileIO::ReadCbnFile decode + PrepAsmtBuf   include/FileIO.h:109-178
 *   qcnn_model_commit           CaffeEva::PrepFeatBuf (buffer planning)    src/CaffeEva.cc:413-532
 *   qcnn_forward[_host]         CaffeEva::ExecForwardPass layer loop       src/CaffeEva.cc:151-261
 *                               = CalcFeatMap dispatcher                   src/CaffeEva.cc:625-670
 *                               -> CalcFeatMap_ConvAprx                    src/CaffeEva.cc:760-868
 *                               -> CalcFeatMap_FCntAprx                    src/CaffeEva.cc:968-1025
 *                               -> GetInPdMat (look-up-table build)        src/CaffeEva.cc:1261-1296
 *                               -> _ReLu/_LoRN/_Pool/_Drpt/_SMax           src/CaffeEva.cc:870-921,1027-1116
 *                               + CvtFeatMapToLablVec (top-5)              src/CaffeEva.cc:1162-1190
 *   qcnn_forward_host_batches   the batch loop itself (one batch after the  src/CaffeEva.cc:168-206
 *                               other), uploads overlapped with compute
 *   qcnn_host_register          pins CaffeEva::dataLst (LoadDataset)       src/CaffeEva.cc:95-107
 *   qcnn_forward_u8             BmpImgIO::RmMeanImg + CropImg in front     src/BmpImgIO.cc:180-224
 *   qcnn_forward_u8_views       the same with any crop offsets and mirrors (CropImg takes the centre only), the views'
 *   / qcnn_views_ten_crop       probabilities averaged on the device
 *   qcnn_forward_u8_resized_views  BmpImgIO::ReszImg (Strict) in front of them, sources of any size  src/BmpImgIO.cc:105-178
 *   qcnn_forward_u8_relaxed_views  ReszImg (Relaxed) + CropImg + a crop-sized mean (VggCnnS) in front  src/BmpImgIO.cc:56-64,124-131
 *   qcnn_src_bmp + qcnn_forward_u8_resized_views_strided / _relaxed_views_strided
 *                               BmpImgIO::LoadBmpImg: the de-interleave, the flip and the row re-packing  src/BmpImgIO.cc:73-103
 *                               (the file's pixel array is read where it lies; so is a decoder's HWC output or a region of a frame)
 *   qcnn_src_yuv_frame + qcnn_forward_u8_resized_views_yuv / _relaxed_views_yuv / qcnn_forward_u8_*_host_batches_yuv
 *                               (no counterpart: the reference reads BMP only) YCbCr frames as decoders emit them — NV12, I420,
 *                               4:4:4, YUY2 — converted to B, G, R in the taps of the resize, read where they lie
 *   qcnn_model_set_layer_dense  CaffePara::LoadLayerPara(false, ..) result src/CaffePara.cc:290-302
 *   / _set_layer_weights        -> CalcFeatMap_ConvPrec / _FCntPrec        src/CaffeEva.cc:681-758, 932-966
 *   qcnn_quantize_layer         produces what CaffePara::LoadLayerPara reads src/CaffePara.cc:262-288
 *                               (sub-codebooks + assignments) from the dense weights of :290-302
 *   qcnn_calib_gram             (no counterpart: the reference ships finished parameters) second moments of a layer's
 *   / qcnn_quantize_layer_ec    input windows — the windows CalcFeatMap_ConvAprx walks, src/CaffeEva.cc:787-827 — and the
 *                               error-corrected quantisation of Wu et al., CVPR'16, sections 3.2 - 3.3, on them
 *   qcnn_calib_begin / _arm     (no counterpart) the same second moments accumulated on the device behind every forward, from
 *   / _read / _end              the layers' input maps where they lie: calibration sets of thousands of images
 *   qcnn_run_layer              CaffeEva::CalcFeatMap on one layer         src/CaffeEva.cc:625-670
 *   qcnn_get_layer_output       featMapLst[l] read-back (parity dumps)     include/CaffeEva.h:109
 *   qcnn_map_diff               (no counterpart) featMapLst[l] of two models compared on the device: propagated response error
 *   qcnn_get_layer_ms           swIndvLayerLst / DispElpsTime              src/CaffeEva.cc:297-326
 *   qcnn_group_*                the image loop of ExecForwardPass(void)    src/CaffeEva.cc:151-211
 *                               spread over the GPUs of one node (the reference has one loop on one core)
 *
 * Map sizes — limits the CALLER has to keep; the library does not refuse what exceeds the first two.  A feature map lives on the
 * device as panels of H*W*C rows of 128 images, 512 bytes a row.
 *   - The INPUT map of a quantised conv layer must hold fewer than 2^23 rows (H*W*C < 8388608: 4 GiB per panel).  The conv table
 *     kernels form the byte offset of a source pixel in 32 bits; beyond that size the offset wraps inside the panel and the bottom
 *     output rows are built from the top source rows — no error, no NaN, a wrong map.  Output maps, dense (precise-path) layers
 *     and the ReLU / LRN / pool layers have no such limit.
 *   - A quantised FC layer must have fewer than 2^23 input dims (32-bit byte offsets into its input panel); a dense one may have more.
 *   - A first conv layer whose input panel reaches 2 GiB leaves the decoded kernel for the table kernel by itself (same results;
 *     qcnn_get_layer_split reports -1 instead of -3).
 *   - A first layer reads the NCHW batch in place only while n*C*H*W*4 < 2^32 bytes per forward; a larger batch is packed first.
 * The 8-bit input entry points state their own 2 GiB limits below.
 */
#ifndef QCNN_HIP_H_
#define QCNN_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QCNN_ABI_VERSION 5   /* qcnn_calib_gram / qcnn_quantize_layer_ec / qcnn_calib_begin .. _end are additive: the version stays 5.  5 (round 6): QCNN_OPT_HALF8 (half-panel eight-wave workgroups), qcnn_model_arena_checksum / qcnn_group_arena_checksum,
                              * qcnn_model_mark_loaded drops the lazily built fp16 program tables.  4 (round 5): QCNN_OPT_LUT_MODE 2 = fp16 table storage, 3 = fp16 tables + fp16 sums (the bf16-pair builder
                              * of version 3 is gone); qcnn_set_option rejects out-of-range values of QCNN_OPT_SYM / _SLIDE / _SYM8;
                              * qcnn_model_set_layer_shape accepts up to 256 code words per sub-space; qcnn_group_forward */

#define QCNN_SMALL_BATCH_MAX 3   /* batches up to this size can take the few-image kernels (QCNN_OPT_SMALL_BATCH) */
#define QCNN_DIFF_CHUNK_ROWS 64  /* qcnn_map_diff: 128-image rows of one channel that one workgroup folds into one partial row */

typedef struct QcnnCtx QcnnCtx;

/* layer type codes: the order of ENUM_LyrType (include/CaffePara.h:26) */
enum { QCNN_CONV = 0, QCNN_POOL = 1, QCNN_FCNT = 2, QCNN_RELU = 3, QCNN_LORN = 4, QCNN_DRPT = 5, QCNN_SMAX = 6 };

/* same fields as the reference's LayerInfo (include/CaffePara.h:28-44) */
typedef struct {
  int type;
  int padSiz, knlSiz, knlCnt, grpCnt, stride, nodCnt, lrnSiz;
  float lrnAlp, lrnBet, lrnIni, drpRat;
} QcnnLayerDesc;

/* options for qcnn_set_option */
enum {
  QCNN_OPT_LUT_MODE = 0,   /* 0 = exact (VALU mul+add in the reference's order: conv/FC outputs are
                              bit-identical to the reference's -O2 native build); 1 = MFMA
                              (v_mfma_f32_16x16x4_f32, fused multiply-add chain; default); 2 = fp16 LUT STORAGE
                              (BASELINE.json configs[4], opt-in study: outside the 1e-4 bar): every table entry is
                              rounded to fp16 when it is stored, sums stay fp32 — conv layers with K = 128 and complete
                              4- / 8-dim sub-spaces and FC layers with 32 code words of 4 dims keep half-size tables in
                              LDS (256-byte rows, ds_read_b64 look-ups: k_conv_sym8 / k_fc_sym8 in their fp16 form),
                              every other layer rounds the entries and keeps them in f32 slots (same values); 3 = as 2 with the
                              RUNNING SUMS of those layers in packed fp16 too (rounded after every addition; the accumulate
                              half of the configs[4] study, 1e-2 territory): half the accumulator registers, so a
                              workgroup's tile is twice as large and every source pixel's table is built a third less often */
  QCNN_OPT_KEEP_ALL = 1,   /* 1 = every layer writes its own feature map (layer-for-layer dumps, default);
                              0 = fast path: ReLU fused into the producing conv/FC epilogue, the first conv layer
                              reads the NCHW input in place, and an LRN layer followed by a 3x3 / stride 2 / pad 0
                              max-pool runs as one kernel with it once a sub-batch is large enough to fill the chip
                              (the normalised map then does not exist: qcnn_get_layer_output fails for it) */
  QCNN_OPT_PROFILE = 2,    /* 1 = bracket every layer launch with HIP events (qcnn_get_layer_ms) */
  QCNN_OPT_SMALL_BATCH = 4, /* 1 (default): batches of up to QCNN_SMALL_BATCH_MAX images run the conv/FC layers with the few-image kernels
                              (lanes = output channels; one image no longer costs a 128-image panel).  Their sums
                              run over sub-space chunks first: equal to the panel kernels to rounding (~1e-6), not bit
                              for bit; 0 = panel kernels for every batch size (batch-size-invariant bits).  The exact
                              builder (QCNN_OPT_LUT_MODE = 0) always uses the panel kernels. */
  QCNN_OPT_SPLIT = 5,      /* 1 (default): a conv/FC launch that cannot fill the 256 CUs with whole tiles (a few panels, i.e.
                              one GPU's share of a batch sharded over the GPUs of a node) cuts the look-up sequences of the
                              tail of its tiles into slices run by separate workgroups and adds the partial sums in a
                              fixed order; FC layers pick their sub-space split for the panel count of the launch.  Results
                              then depend on the batch size to rounding (~1e-6).  Never applied with the exact builder
                              (QCNN_OPT_LUT_MODE = 0).  0 = one workgroup per tile, batch-size-invariant bits. */
  QCNN_OPT_SLIDE = 7,      /* 1 (default): conv layers with K = 128 whose windows overlap in at most three output rows
                              (knl <= 3 * stride) and whose channel count leaves room for three accumulator slots may run
                              the SLIDING kernel — a workgroup sweeps the source rows under a segment of one output column
                              and builds every source pixel of the strip once — when the launch planner predicts it to be
                              faster than the tile kernel.  Same summation order as the tile kernels ((kh, kw, m)), MFMA
                              builders only.  0 = tile kernels only; 2 = whenever
                              a layer is eligible, whatever the planner predicts (tests). */
  QCNN_OPT_DECODE = 8,     /* 1 (default): a conv layer with ONE sub-space of <= 4 dims (the RGB input layer: AlexNet conv1,
                              VGG-16 conv1_1) is evaluated through the code words its assignments name — the look-up
                              tables of src/CaffeEva.cc:1261-1296 are not materialised, the same sum goes to the matrix
                              pipe (a look-up there stands for <= 4 multiply-adds and the table of a pixel costs more than
                              the look-ups it serves).  Same parameters, same function, results within the MFMA modes'
                              tolerance; the network input is then packed into panels first.  MFMA modes only
                              (QCNN_OPT_LUT_MODE 1), batches above QCNN_SMALL_BATCH_MAX.  0 = table kernels for every layer */
  QCNN_OPT_SYM = 9,        /* 1 (default): a conv layer with exactly 128 channels per group and K = 128 (AlexNet conv2) that neither
                              slides nor splits may run SYMMETRIC workgroups — all 16 waves build and gather, 8 channels x a
                              2x2 tile per wave: fewer table builds per output position and no idle gather lane — when the
                              launch planner predicts them faster.  Bit-identical to the tile kernels; f32 MFMA mode only.
                              0 = never; 2 = whenever eligible (tests) */
  QCNN_OPT_SYM8 = 10,      /* 1 (default): a conv layer with K = 128, complete 4- or 8-dim sub-spaces and more than 64 channels per
                              group may run EIGHT-wave symmetric workgroups with 256 registers per wave (k_conv_sym8): twice the
                              accumulators of the 16-wave kernels per CU, i.e. larger output tiles (384 channels x 1x2, 256 x 1x3,
                              192 x 2x2, 128 x 2x3) and a third fewer table builds per output position — when the launch planner
                              predicts them faster than the tile / sliding / 16-wave symmetric launch.  Bit-identical to the tile
                              kernels; f32 MFMA mode only.  The same workgroups also SLIDE (segments of strips of one or two output
                              columns with 3 or 5 accumulator slots: 3x3 / 1 and 5x5 / 1 layers of up to 256 channels per workgroup build
                              every source pixel of a strip once: 3 or 2 table builds per output position instead of 4 - 5) where the
                              planner predicts that faster: VGG-16's 256- / 512-channel layers.  0 = never; 2 = tile form whenever
                              eligible, 3 = sliding form whenever eligible (tests); other values are refused.  qcnn_get_layer_split reports
                              (-5, slices per tile: QCNN_OPT_SPLIT cuts its tiles too) for the tile form, (-6, segments per column) for the
                              sliding form.  FC layers with 32 code words of 4 dims
                              (AlexNet / VGG-16 fc6, fc7) run the same eight waves (k_fc_sym8: 96 channels per wave, offsets through
                              LDS-DMA, software-pipelined look-ups) unless the option is 0 */
  QCNN_OPT_PACKED_FC = 11, /* 1: for batches of up to QCNN_SMALL_BATCH_MAX images the FC layers read their assignments from the
                              BIT-PACKED stream the reference's .cbn files hold (4 / 5 bits per assignment, file order [Ct][M], kept
                              resident in the arena beside the one-byte table of the panel kernels) and unpack them in the kernel:
                              AlexNet streams 10.5 MB of FC assignments per image instead of 16.8 MB of bytes (of which the strided
                              byte reads fetched 64-byte lines: 4x).  Same bits as the byte path.  0 (default) = bytes: the unpack arithmetic of the
                              block-structured stream costs more than the traffic it saves (fc6 0.056 against 0.035 ms at one image) */
  QCNN_OPT_DIRECT_DEC = 12, /* 1 (default): on the fast path (QCNN_OPT_KEEP_ALL = 0) an unpadded first conv layer that runs through its
                              decoded code words (QCNN_OPT_DECODE) reads the caller's NCHW batch in place (k_conv_dec_nchw: k over the
                              columns of a kernel row) — no pack pass into panels (AlexNet: 1.24 GB of HBM traffic per 1000 images).
                              0 = pack, then the panel kernel.  qcnn_get_layer_split reports (-3, 2) against (-3, 1) */
  QCNN_OPT_HALF8 = 13,     /* 1 (default): a conv layer with K = 128, complete 4- or 8-dim sub-spaces and 128 / 192 / 256 / 384 / 512
                              output channels per group (or chunks of 512) may run in eight-wave workgroups of HALF a panel (64 images:
                              twice the output tile per workgroup, half the table build per stage — qcnn_half8.hip) where the launch
                              planner predicts them faster than every other form — in their tile form or, for windows that overlap in
                              three output rows, their SLIDING form (segments of strips of output columns, every source pixel built once
                              per segment); 2 = the tile form whenever eligible, 3 = the sliding form whenever eligible (tests); 0 = never.
                              Same table entries in the same order: bit-identical to the other f32 table kernels.
                              qcnn_get_layer_split reports (-9, 1) / (-10, segments per column) */
  QCNN_OPT_DEC_BF16SPLIT = 14, /* A first layer read in place (QCNN_OPT_DIRECT_DEC) whose code words fit the LDS as two 16-bit
                              pieces (Cin knl^2 rounded up to 32, times the channels, times 4 bytes <= 158 KB) computes its products
                              on the 16-bit matrix pipe at fp32 accuracy.  1: activations and code words split exactly into three bf16
                              pieces each, the six cross terms down to order 2^-16 summed in fp32 (k_conv_dec_nchw_split).  2 (default):
                              two fp16 pieces each, scaled by exact powers of two (activations by 64, code words by a per-layer scale
                              that puts the largest into [2^13, 2^14]), the three cross terms x2 w1, x1 w2, x1 w1 summed in fp32
                              (k_conv_dec_nchw_f16: half the matrix instructions; a product is within 3 x 2^-22 of exact).  Input
                              values outside [-1023, 1023], NaN and Inf included, are detected per work item and image, and those
                              images' results of the item are recomputed in form 1 by a second launch: they carry form 1's bits, no
                              other image's result changes.  A layer without such a scale (all code words zero, a largest |code word|
                              that is not a normal float in [2^-107, 2^20), a bias that is not finite or beyond 2^100 / (64 scale)) runs
                              form 1.  Neither is bit-identical to 0 = the f32 matrix instructions (k_conv_dec_nchw); all three are
                              batch-size invariant.  Other values are refused.  qcnn_get_layer_dec_form reports what ran. */
  QCNN_OPT_HOST_CHUNK = 6, /* panels per chunk (default 2) of a qcnn_forward_host batch of at least two chunks: every chunk is
                              uploaded on a copy stream and its layers start when it has arrived, so the upload of chunk
                              k + 1 runs under the layers of chunk k; all chunks fill the same whole-batch feature maps.
                              0 = always one launch per layer for the whole batch */
  QCNN_OPT_STREAMS = 3     /* 1..4 (default 2): a forward is cut into that many sub-batches of whole 128-image
                              panels which run concurrently on separate HIP streams (LDS-bound conv/FC kernels
                              of one overlap HBM-bound glue kernels of another); results do not depend on it */
};

/* ---- context ---- */
/* device_id: HIP device ordinal.  stream: a hipStream_t to enqueue on (e.g. torch's current stream),
 * or NULL to let the library create its own. */
int qcnn_ctx_create(int device_id, void* stream, QcnnCtx** out);
int qcnn_ctx_destroy(QcnnCtx* ctx);
/* last error of ctx (or of ctx creation when ctx == NULL); never NULL */
const char* qcnn_last_error(const QcnnCtx* ctx);
int qcnn_abi_version(void);
int qcnn_device_count(int* count);
int qcnn_set_option(QcnnCtx* ctx, int option, int value);
int qcnn_sync(QcnnCtx* ctx);
int qcnn_ctx_device(const QcnnCtx* ctx);          /* HIP device ordinal of the context */
void* qcnn_ctx_stream(const QcnnCtx* ctx);        /* the hipStream_t the context enqueues on */

/* ---- model ---- */
/* qcnn_model_begin refuses (non-zero, qcnn_last_error names the layer and the rule) a conv layer whose padSiz is negative or >= knlSiz:
 * every window must hold a pixel of the map.  The context stays usable: a later qcnn_model_begin starts over. */
int qcnn_model_begin(QcnnCtx* ctx, int layer_cnt, const QcnnLayerDesc* layers, int in_c, int in_h, int in_w);
/* Declare the quantisation shape of conv/FC layer `layer` (M sub-spaces, K codewords, Cs dims each).
 * Must precede qcnn_model_commit for every conv/FC layer.  K <= 256 — everything the reference's uint8 assignments can
 * name (include/FileIO.h:128-166); Cs <= 8.  No shipped model has more than 128 code words, and a LUT stage in LDS holds 128
 * rows: a layer with 128 < K <= 256 is cut into ceil(K / 127) pseudo sub-spaces of <= 127 code words + one all-zero row over the
 * same dims (an assignment names its code word in one of them and the zero row in the others: the same sums in the same order)
 * and runs the exact-builder kernels whatever QCNN_OPT_LUT_MODE says — correct, about half the speed of a K <= 128 layer. */
int qcnn_model_set_layer_shape(QcnnCtx* ctx, int layer, int M, int K, int Cs);
/* The reference's PRECISE path (CaffeEva::Init(false): CalcFeatMap_ConvPrec src/CaffeEva.cc:681-758, _FCntPrec :932-966) as
 * an on-device exact baseline: declare conv/FC layer `layer` dense (instead of qcnn_model_set_layer_shape, before commit)
 * and upload bias [Ct] + weights in the reference's FILE layout after commit — conv kernels [Ct][Cin/grp][kh][kw]
 * (convKnl.NN.bin), FC weights [Ct][D] (fcntWei.NN.bin).  Dense and quantised layers may be mixed in one model. */
int qcnn_model_set_layer_dense(QcnnCtx* ctx, int layer);
int qcnn_model_set_layer_weights(QcnnCtx* ctx, int layer, const float* bias, const float* weights_file);
/* Quantise one dense conv / FC layer into the parameters qcnn_model_set_layer_params takes: product-quantisation k-means
 * (Lloyd's algorithm), deterministic to the bit (DESIGN.md "Quantising dense weights").  The reference ships only the result
 * of this step; the layout is the one its approximate path reads: sub-codebooks ctrdLst [M][K][Cs] and 0-based assignments
 * asmtLst [Ct][kh][kw][M] (CaffePara::LoadLayerPara src/CaffePara.cc:262-288, consumed by GetInPdMat src/CaffeEva.cc:1261-1296).
 *   weights    the dense layer in the precise path's file layout (src/CaffePara.cc:290-302): conv kernels [Ct][Cin][kh][kw]
 *              (convKnl, Cin = channels per group) or FC weights [Ct][D] with kh = kw = 1, Cin = D (fcntWei)
 *   points     sub-space m holds N = Ct*kh*kw points, point n = (ct*kh + y)*kw + x being W[ct][m*Cs + j][y][x] for
 *              j < CsEff(m) = min(Cin - m*Cs, Cs) (the dims rule of src/CaffeEva.cc:1277)
 *   distance   fp32, d = 0; for j < CsEff: t = p_j - c_j; d = d + t*t (one rounding per operation, no FMA); nearest code
 *              word: the lowest k of the minimum
 *   update     c_k[j] = (float)(fp64 sum of the members' p_j in ascending n / members); a code word without members keeps its value
 *   seeding    ctrd_init ([M][K][Cs]) when given, else farthest-first: c_0 = point 0, then the point farthest from its nearest
 *              chosen code word (ties: lowest n)
 *   loop       a = assign(C); up to max_iter times: C = update(C, a), a' = assign(C), stop when a' == a in every sub-space
 * Outputs: ctrd_out [M][K][Cs] (dims >= CsEff written as 0), asmt_out 0-based [Ct][kh][kw][M] (FC: [Ct][M]); sse2 (may be
 * NULL) = fp64 sums of the minimum distances before the first and after the last step; iters2 (may be NULL) = update steps
 * taken, sub-spaces still changing when max_iter ran out.  Needs 1 <= Cs <= 16, 2 <= K <= 256, (M-1)*Cs < Cin <= M*Cs,
 * max_iter >= 0 and finite weights.  Blocking; device scratch is allocated per call and freed before return; works with or
 * without a model loaded and changes nothing of it. */
int qcnn_quantize_layer(QcnnCtx* ctx, int Ct, int Cin, int kh, int kw, int M, int K, int Cs, const float* weights_host,
                        const float* ctrd_init_host, int max_iter, float* ctrd_out_host, uint8_t* asmt_out_host, double* sse2,
                        int* iters2);
/* Error-corrected quantisation (Wu et al., "Quantized Convolutional Neural Networks for Mobile Devices", CVPR'16, sections
 * 3.2 - 3.3; DESIGN.md "Error-corrected quantisation"): code books and assignments that minimise the error of the layer's
 * RESPONSE on calibration inputs, J = sum_ct e_ct^T G_g(ct) e_ct with e_ct = w_ct - w_hat_ct in patch order
 * p = (y*kw + x)*Cg + c and G_g = sum over calibration patches s of s s^T — instead of the error of the weights.
 *
 * qcnn_calib_gram: the raw fp64 sums G_g[p][q] = sum_images sum_output pixels s_p s_q of a layer's input windows (out-of-image
 * taps are zeros).  in_nhwc_host = fm[layer] of n images, NHWC per image: what qcnn_run_layer takes and qcnn_get_layer_output
 * returns (FC: H = W = 1, Cin_total = D, kh = kw = 1).  gram_inout_host [grp][P][P], P = kh*kw*Cin_total/grp; accumulate != 0
 * adds to what it holds (calibration sets larger than one upload).  Products run on the matrix pipe in fp32 over runs of 256
 * patches and in fp64 across runs: every entry within gamma_260 * sum |s_p s_q| of its exact value however large the set; the
 * result is symmetric to the bit and the same bits from run to run.  Blocking; scratch is allocated per call and freed before
 * return; works with or without a model loaded and changes nothing of it. */
int qcnn_calib_gram(QcnnCtx* ctx, int H, int W, int Cin_total, int grp, int kh, int kw, int stride, int pad,
                    const float* in_nhwc_host, int n, double* gram_inout_host, int accumulate);
/* Refine a quantisation of one layer (the output of qcnn_quantize_layer: ctrd_init [M][K][Cs], asmt_init in file order) against
 * gram_host [grp][P][P] (NULL = identity: J is then the k-means SSE).  Cin = channels per group, output channel ct belongs to
 * group ct / (Ct/grp); one code book for all groups and taps (src/CaffeEva.cc:787,810).  Block (y, x, m) = the index range
 * (y*kw + x)*Cin + m*Cs + [0, CsEff(m)); E = W - W_hat, Hm = E G.  One SWEEP = for m = 0 .. M-1:
 *   assign   for every tap (y, x) in ascending order, all ct at once: code word c_k in place of the current one changes J by
 *            delta_k = -2 d^T Hm[ct][b] + d^T G_bb d, d = c_k - c_cur; the smallest delta_k is taken only if it is < 0 (ties
 *            among improvements: the lowest k); E and Hm follow before the next tap
 *   update   code word by code word in ascending k: A_k = sum_ct sum_{b,b' in L_k(ct)} G_bb' + lambda I, v_k = sum_ct
 *            sum_{b in L_k(ct)} Hm[ct][b] over the blocks L_k(ct) of channel ct that name k, lambda = ridge * trace(G) / P
 *            (mean over groups); c_k = (float)(c_k + A_k^-1 v_k) (fp64 Cholesky); E and Hm follow.  A code word without
 *            members (or with an A_k that is not positive definite) keeps its value.  kh = kw = 1: code words share no
 *            channel, all K are solved from one state.  Dims >= CsEff stay 0.
 * Both steps minimise J over one block of variables: J does not rise.  The search runs in fp64.  obj_trace[i] (may be NULL,
 * [sweeps + 1]) = J after i sweeps, evaluated from scratch in fp64 from the book and assignments of that moment;
 * changed_trace[i] (may be NULL, [sweeps]) = assignments changed in sweep i.  A sweep that changes no assignment and no code
 * word ends the search (the remaining entries repeat the last value and 0).  Needs the shape rules of qcnn_quantize_layer,
 * Ct % grp == 0, sweeps >= 0, ridge >= 0, finite weights / gram / book, assignments < K, a non-negative gram diagonal.
 * Blocking; scratch per call, freed before return; a loaded model is not touched. */
int qcnn_quantize_layer_ec(QcnnCtx* ctx, int Ct, int Cin, int grp, int kh, int kw, int M, int K, int Cs, const float* weights_host,
                           const double* gram_host, const float* ctrd_init_host, const uint8_t* asmt_init_host, int sweeps,
                           double ridge, float* ctrd_out_host, uint8_t* asmt_out_host, double* obj_trace, int* changed_trace);
/* Resident calibration: qcnn_calib_gram's sums, accumulated on the device behind every forward of a committed model (dense or
 * quantised), read from each listed layer's INPUT map where the forward left it (image-minor panels [E][128]; kernel
 * k_ec_gram_panel).  Same conventions (patch index, zeros for out-of-map taps, Ho / Wo) and the same precision contract: fp32
 * over runs of at most 256 patch rows, fp64 across runs, every entry within gamma_260 * sum |s_p s_q| of its exact value however
 * many batches are added; no float atomics, symmetric to the bit, the same bits for the same sequence of batches.  The first FC
 * layer's columns are in the reference's NCHW flatten order d = (c*H + h)*W + w, a later FC layer's are its map's elements.
 *
 * qcnn_calib_begin: one zeroed fp64 matrix [grp][P][P] per listed conv / FC layer on the context's device, and arms.  Refused,
 * with nothing allocated: before commit, a layer that is neither conv nor FC, a layer listed twice, P > 46340, a calibration
 * already open.  (The input map of a conv / FC layer always exists as a panel map — fused ReLUs alias the rectified map, a fused
 * LRN + pool pair drops only the map between the two — with one exception, next paragraph.)
 * LAYER 0 ROUTE: if layer 0 is listed, its input must exist as fm[0] panels while armed.  The float entry points that would
 * feed a first conv layer straight from the NCHW buffer (QCNN_OPT_KEEP_ALL = 0, the in-place first-layer kernels) take the packed
 * route for that time: qk_pack_nchw + the panel kernels, whose results differ from the in-place kernels' in the last bits.  The
 * 8-bit entry points pack anyway.  This is the only way an armed calibration changes a forward's outputs.
 * While armed, every batch that passes the layer loop — any qcnn_forward* entry point, single call or *_host_batches, any
 * QCNN_OPT_STREAMS, batches of one to three images included, every chunk of a chunked host batch once — enqueues one launch per
 * listed layer for its live images (lanes of a ragged panel beyond the batch contribute exactly nothing), on the context's
 * stream behind the join of the sub-batch streams and in front of whatever could overwrite the maps.
 * SPLIT RULE: the rows of a launch are cut in units of one (panel, output pixel) = 128 patch rows.  With T upper-triangle tile
 * pairs (64 x 64) x groups, a launch of `panels` panels runs min(max(1, 2048 / T), 128 MiB / matrix bytes, ceil(units / 2),
 * 65535) splits of whole two-unit runs (at least 1): a function of the shape and the panel count alone.  Several splits write
 * fp64 slabs that are added to the matrix in ascending order; one split adds its tiles to the matrix directly.
 * qcnn_calib_arm(0 / 1): unarmed, nothing is launched and nothing changes.  qcnn_calib_read: blocking; the matrix of a listed
 * layer (gram_host [grp][P][P], may be NULL) and the patch rows added so far (rows, may be NULL); any number of times, resets
 * nothing.  qcnn_calib_end frees the matrices; qcnn_model_begin and qcnn_ctx_destroy end an open calibration implicitly.  Without
 * qcnn_calib_begin no code path differs. */
int qcnn_calib_begin(QcnnCtx* ctx, const int* layers, int n_layers);
int qcnn_calib_arm(QcnnCtx* ctx, int on);
int qcnn_calib_read(QcnnCtx* ctx, int layer, double* gram_host, long long* rows);
int qcnn_calib_end(QcnnCtx* ctx);
/* Size of the packed parameter arena (biases, permuted codebooks, permuted assignments). */
int qcnn_model_arena_bytes(QcnnCtx* ctx, size_t* bytes);
/* Plan buffers for up to max_batch images.  dev_arena: caller-owned device memory of
 * qcnn_model_arena_bytes() bytes (so that a communicator can broadcast it), or NULL to let the
 * library allocate it. */
int qcnn_model_commit(QcnnCtx* ctx, int max_batch, void* dev_arena);
/* Device address and size of the packed parameter arena (after commit): what a communicator broadcasts. */
int qcnn_model_arena_ptr(QcnnCtx* ctx, void** dev_ptr, size_t* bytes);
/* Checksum of the packed parameter arena as it lies on the device: sum2[0] = sum of its 32-bit words, sum2[1] = a
 * position-weighted sum (both modulo 2^64).  Ranks whose arenas hold the same bytes report the same pair: what a sharded run
 * compares before it trusts a broadcast (qcnn_group_model_broadcast does; bench.py --gpus N does across processes).  Blocking. */
int qcnn_model_arena_checksum(QcnnCtx* ctx, unsigned long long* sum2);
/* Upload one conv/FC layer's parameters from host memory in the reference's FILE layout:
 * bias [Ct]; ctrd [M][K][Cs]; asmt 0-based uint8, [Ct][kh][kw][M] (conv) or [Ct][M] (FC).
 * Performs the PrepCtrdBuf / PrepAsmtBuf permutations into the arena.  After commit. */
int qcnn_model_set_layer_params(QcnnCtx* ctx, int layer, const float* bias, const float* ctrd_file,
                                const uint8_t* asmt_file);
/* Same, with the assignments still bit-packed as the .cbn file holds them (include/FileIO.h:128-166): `cbn_blocks` =
 * the file's payload behind its header (4096-byte blocks of floor(32768 / bits) values, MSB first, 0-based indices in
 * file order [Ct][kh][kw][M] / [Ct][M]), `bits` = its bitCntPerEle.  The packed stream is what crosses PCIe (AlexNet fc6:
 * 5.9 MB instead of 9.4 MB); the decode + PrepAsmtBuf permutation run on the device. */
int qcnn_model_set_layer_params_cbn(QcnnCtx* ctx, int layer, const float* bias, const float* ctrd_file,
                                    const uint8_t* cbn_blocks, size_t cbn_bytes, int bits);
/* Declare every conv/FC layer loaded without uploading: the caller filled the arena itself (e.g. the
 * receiving ranks of an RCCL broadcast of rank 0's arena).  After commit. */
int qcnn_model_mark_loaded(QcnnCtx* ctx);
/* (H, W, C) of feature map l in [0, layer_cnt] */
int qcnn_fm_dims(QcnnCtx* ctx, int l, int* hwc3);

/* ---- forward ---- */
/* Device-resident forward of n <= max_batch images, asynchronous on the context's stream.
 * in_nchw_dev [n][C][H][W] fp32; prob_dev [n][classes] fp32 or NULL; top5_dev [n][5] uint16 or NULL. */
int qcnn_forward(QcnnCtx* ctx, const float* in_nchw_dev, int n, float* prob_dev, uint16_t* top5_dev);
/* Same with the reference's image pre-processing done on the device (BmpImgIO::RmMeanImg + CropImg,
 * src/BmpImgIO.cc:180-224): in_u8_dev [n][C][src_h][src_w] planar 8-bit (B, G, R planes, as
 * BmpImgIO::LoadBmpImg :84-96 stores them), mean_dev [C][src_h][src_w] fp32 or NULL; the network input is
 * the centre crop of float(pixel) - mean.  Bit-identical to qcnn_forward on the host-preprocessed image;
 * a quarter of the host-to-device bytes. */
int qcnn_forward_u8(QcnnCtx* ctx, const uint8_t* in_u8_dev, int src_h, int src_w, const float* mean_dev, int n,
                    float* prob_dev, uint16_t* top5_dev);
/* Multi-view inference from the same 8-bit images: every image is evaluated on n_views crops of in_h x in_w pixels (the network
 * input), each optionally mirrored left-right, and the class probabilities of its views are averaged — the ten-crop protocol
 * the shipped networks are reported under, sliding-window and random-crop evaluation.  A view names the top-left corner of its
 * crop inside the source image; flip != 0 mirrors the crop left-right. */
#define QCNN_MAX_VIEWS 32
typedef struct { int oy, ox, flip; } QcnnView;
/* The standard ten views of a src_h x src_w image for an in_h x in_w network, in this order: the corners (0,0), (0,X), (Y,0),
 * (Y,X) with Y = src_h - in_h, X = src_w - in_w, the centre ((src_h - in_h) / 2, (src_w - in_w) / 2) — the offsets
 * qcnn_forward_u8 uses — then the same five with flip = 1.  Needs no device and no context.  Non-zero when the source is
 * smaller than the input (or a size is not positive, or views10 is NULL). */
int qcnn_views_ten_crop(int src_h, int src_w, int in_h, int in_w, QcnnView* views10);
/* in_u8_dev / mean_dev as qcnn_forward_u8; views_host [n_views] in HOST memory, copied into the launch's arguments (nothing
 * has to outlive the call).  Batch slot s = i * n_views + v holds view v of image i: element (c, y, x) of it is
 * float(px[i][c][oy + y][xs]) - mean[c][oy + y][xs] with xs = ox + (flip ? in_w - 1 - x : x) — one convert, one subtract, the
 * mean taken at the SOURCE position, so a mirrored view is the mirror of the plain one bit for bit and the centre view is
 * qcnn_forward_u8's input.  The n * n_views <= max_batch slots run through the layers exactly as a batch of that size given
 * to qcnn_forward_u8 would (same kernels, same bits; qcnn_get_layer_output afterwards addresses slots).
 *   prob_views_dev [n][n_views][classes] or NULL   the rows of the slots, un-averaged
 *   prob_dev [n][classes] or NULL                  fp32, one rounding per operation: s = p[view 0]; s = s + p[view v] for
 *                                                  v = 1 .. n_views - 1 in that order; s / (float)n_views (n_views = 1: the row itself)
 *   top5_dev [n][5] or NULL                        top-5 of the averaged rows, by the rule of every other entry point
 * Every argument is checked before anything is launched: a model that is not committed, n <= 0, n_views outside
 * [1, QCNN_MAX_VIEWS], n * n_views > max_batch and a view that leaves the source (oy < 0, ox < 0, oy + in_h > src_h,
 * ox + in_w > src_w) return non-zero with nothing enqueued, and so does a source image of 2 GiB or more (offsets inside an
 * image are 32-bit).  Asynchronous on the context's stream. */
int qcnn_forward_u8_views(QcnnCtx* ctx, const uint8_t* in_u8_dev, int src_h, int src_w, const float* mean_dev, int n,
                          const QcnnView* views_host, int n_views, float* prob_dev, uint16_t* top5_dev,
                          float* prob_views_dev /* [n][n_views][classes] or NULL */);
/* The same from 8-bit source images of ANY size, each with its own: BmpImgIO::ReszImg (ENUM_ReszType::Strict,
 * src/BmpImgIO.cc:105-178) on the device in front of RmMeanImg (ENUM_MeanType::Full) and the views, so that with the centre view
 * alone the call is BmpImgIO::Load followed by the forward pass.  Image i is the planar [C][h][w] 8-bit image at src_dev +
 * imgs_host[i].offset; it is resized to full_h x full_w in fp32 with one rounding per operation ((float) conversions of ints):
 *   sh = (float)(h-1) / (float)(full_h-1)                          sw likewise
 *   yc = sh * (float)y;  y0 = max(0, (int)yc);  y1 = min(h-1, y0+1)
 *   wy0 = 1.0f - (yc - (float)y0);  wy1 = 1.0f - ((float)y1 - yc)  columns likewise -> x0, x1, wx0, wx1
 *   w00 = wy0*wx0; w01 = wy0*wx1; w10 = wy1*wx0; w11 = wy1*wx1
 *   num = ((p(y0,x0)*w00 + p(y0,x1)*w01) + p(y1,x0)*w10) + p(y1,x1)*w11        p = (float)pixel
 *   out = num / (((w00 + w01) + w10) + w11)                                    IEEE division
 * — the reference's bits (the division is not a no-op: at a clamped last row both row weights are about 1; a source of the full
 * size comes out as its pixel values).  mean_dev [C][full_h][full_w] or NULL is subtracted at the full-image position, one fp32
 * subtraction; the views are then cut from the full_h x full_w image and mirrored exactly as qcnn_forward_u8_views defines them
 * on a source of that size.  The resized images are never stored: every element of a batch slot is computed from the four 8-bit
 * taps of its image.  Slot order, the layers, the averaging, top-5 and the three outputs are those of qcnn_forward_u8_views.
 * h == 1 or w == 1 is legal (the scale is 0 and both taps name the same pixel).
 * imgs_host [n] and views_host [n_views] in HOST memory need not outlive the call: the descriptors are staged in pinned and
 * device memory the context owns (grown on demand; a staging buffer is not rewritten before the call that reads it has passed).
 * Every argument is checked before anything is enqueued — non-zero, a message in qcnn_last_error, outputs untouched: a model that
 * is not committed, n <= 0, n_views outside [1, QCNN_MAX_VIEWS], n * n_views > max_batch, full_h < 2 or full_w < 2 (the scale
 * divides by full - 1), a full image smaller than the network input (or of 2 GiB and more), a view that leaves the full image,
 * h < 1 or w < 1, an image of 2 GiB or more (offsets inside an image are 32-bit), offset + C*h*w > src_bytes.  Asynchronous on
 * the context's stream. */
typedef struct { uint64_t offset; int32_t h, w; } QcnnSrcImage;   /* planar [C][h][w] 8-bit image at src_dev + offset */
int qcnn_forward_u8_resized_views(QcnnCtx* ctx, const uint8_t* src_dev, size_t src_bytes,
                                  const QcnnSrcImage* imgs_host, int n, int full_h, int full_w,
                                  const float* mean_dev /* [C][full_h][full_w] or NULL */,
                                  const QcnnView* views_host, int n_views,
                                  float* prob_dev, uint16_t* top5_dev, float* prob_views_dev);
/* The reference's OTHER pre-processing mode, ENUM_ReszType::Relaxed + ENUM_MeanType::Crop (VggCnnS, src/CaffeEvaWrapper.cc:69-76;
 * src/BmpImgIO.cc:56-64,124-131), on the device: the image is resized by ONE scale for both axes — the aspect ratio is kept, the
 * full size differs per image — then cropped, then a mean of the CROP's size is subtracted.  For a source of h x w pixels and the
 * nominal full size full_h x full_w, in fp32 with one rounding per operation ((float) conversions of ints):
 *   sh = (float)(h-1) / (float)(full_h-1);   sw = (float)(w-1) / (float)(full_w-1)
 *   s  = min(sh, sw)                                        lines 127-128 leave BOTH scales equal to s
 *   Hf = (int)((double)((float)(h-1) / s) + 1e-7) + 1       int / float is a float division, kEpsilon a double, the cast truncates
 *   Wf = (int)((double)((float)(w-1) / s) + 1e-7) + 1
 * and the image is resampled to Hf x Wf by the sequence of qcnn_forward_u8_resized_views with s as both scales: yc = s * (float)Y,
 * the taps, the four weight products, the left-to-right sums, the IEEE division.  The float quotient is NOT the mathematical
 * one: the side that sets the scale may come out one pixel under the nominal size (37 x 53 at 256 x 256 gives 255 x 369, 2 x 2
 * gives 255 x 255; 30 x 8 at 12 x 14 gives 54 x 13), so "the smaller side becomes full" does not hold for the reference's bits
 * and every view is checked against every image's own Hf x Wf.
 * qcnn_relaxed_full_size is that size rule: host only, needs no device and no context; scale may be NULL.  Non-zero (nothing
 * written) for h < 2 or w < 2 (s would be 0 and the reference casts inf / NaN to int: refused, not reproduced), full_h < 2 or
 * full_w < 2, an Hf or Wf of 2^24 or more ((float)Y would not be exact), hf or wf == NULL. */
int qcnn_relaxed_full_size(int h, int w, int full_h, int full_w, int* hf, int* wf, float* scale);
/* a view placed relative to each image's OWN full size: a = 0 near edge, 1 = CropImg's centre (full - in) / 2, 2 = far edge (full - in);
 * d = pixels added to it */
typedef struct { int ay, ax, dy, dx, flip; } QcnnAnchorView;
/* The standard ten views as anchors, in the order of qcnn_views_ten_crop: the corners (0,0), (0,2), (2,0), (2,2), the centre
 * (1,1), all with d = 0, then the same five with flip = 1 — for an image whose full size is Hf x Wf they resolve to
 * qcnn_views_ten_crop(Hf, Wf, in_h, in_w).  Needs no device and no context.  Non-zero when views10 is NULL. */
int qcnn_views_ten_crop_anchored(QcnnAnchorView* views10);
/* Multi-view inference in that mode.  src_dev, src_bytes, imgs_host as qcnn_forward_u8_resized_views takes them.  View v of image
 * i has its corner at oy = a(ay) + dy, ox = a(ax) + dx with a(0) = 0, a(1) = (F - in) / 2 (integer division: CropImg's corner),
 * a(2) = F - in and F that image's Hf resp. Wf.  Element (c, y, x) of batch slot i * n_views + v is
 *   R_i[c][oy + y][ox + xl] - mean_crop[c][y][xl],   xl = flip ? in_w - 1 - x : x
 * with R_i the resampled image (never stored: every element is computed from the four 8-bit taps) and mean_crop_dev
 * [C][in_h][in_w] or NULL: one fp32 subtraction, the mean taken at the view-local position BEFORE mirroring (the reference has no
 * mirrors; the rule is the invariant of qcnn_forward_u8_views), so a mirrored view is the mirror of the plain one bit for bit and
 * the centre anchor alone is BmpImgIO::Load of a Relaxed / Crop model followed by the forward pass.  Slot order, the layers, the
 * averaging, top-5, the three optional outputs and the staging of imgs_host / views_host (neither has to outlive the call) are
 * those of qcnn_forward_u8_resized_views.
 * Every argument is checked before anything is enqueued — non-zero, a message in qcnn_last_error, outputs untouched: everything
 * qcnn_forward_u8_resized_views checks (with h < 2 or w < 2 in place of h < 1 or w < 1), an Hf or Wf of 2^24 or more, ay or ax
 * outside 0..2, and for every image SEPARATELY a resolved view that leaves that image's Hf x Wf: one such image refuses the whole
 * call, the message names the image and the view.  Asynchronous on the context's stream. */
int qcnn_forward_u8_relaxed_views(QcnnCtx* ctx, const uint8_t* src_dev, size_t src_bytes, const QcnnSrcImage* imgs_host, int n,
                                  int full_h, int full_w, const float* mean_crop_dev /* [C][in_h][in_w] or NULL */,
                                  const QcnnAnchorView* views_host, int n_views,
                                  float* prob_dev, uint16_t* top5_dev, float* prob_views_dev);
/* Source images read IN PLACE, whatever their layout: interleaved (a decoder's HWC output, a BMP file's pixel array), pitched
 * (a camera frame, a rectangle inside a larger one), bottom-up (BMP), planar with gaps.  An image is described by strides:
 * sample (c, y, x) of image i — c in the network's channel order B, G, R; (0, 0) the TOP-LEFT pixel as the network sees it — is
 * the byte at
 *   src_dev + offset + y * row_stride + x * pix_stride + ch_offset[c]
 * The planar layout of QcnnSrcImage is row_stride = w, pix_stride = 1, ch_offset[c] = c * h * w (qcnn_src_planar); a bottom-up
 * BMP has offset at its LAST file row and a negative row_stride (qcnn_src_bmp).  Samples may alias (a grey image fed to three
 * channels: all ch_offset equal; row_stride 0; two descriptors naming overlapping regions of one frame): the source is only
 * read.  Bytes that are no sample (padding, alpha, gaps, the frame around a region, file headers) are never read. */
typedef struct {
  uint64_t offset;       /* byte, relative to src_dev, of pixel (0, 0): the TOP-LEFT pixel of the image as the network sees it */
  int64_t  row_stride;   /* bytes from pixel (y, x) to (y + 1, x); negative = rows stored bottom-up */
  int32_t  h, w;
  int32_t  pix_stride;   /* bytes from pixel (y, x) to (y, x + 1); >= 1 */
  int32_t  ch_offset[4]; /* byte of network channel c (c < C, network order B, G, R) relative to its pixel; >= 0; entries c >= C ignored */
} QcnnSrcPixels;         /* 48 bytes with the trailing padding */
/* The descriptor of a planar image (host only: no device, no context).  Non-zero, nothing written: img or out NULL, C outside
 * [1, 4], h < 1 or w < 1, C * h * w > INT32_MAX. */
int qcnn_src_planar(const QcnnSrcImage* img, int C, QcnnSrcPixels* out);
/* The descriptor of the pixel array of a BMP file whose bytes will lie at src_dev + file_offset — the whole file, header
 * included, is uploaded untouched (host only: file_host is read here, no device, no context).  Accepted are exactly the flavours
 * the host mirror's BmpImgIO decodes: the BM signature, a file of at least 54 bytes, 24 or 32 bits per pixel, compression 0,
 * a positive width, a height of either sign (negative = top-down; 0 and INT32_MIN are refused), rows padded to 4 bytes, the file
 * at least dataOff + stride * h bytes long.  Every other file: non-zero, nothing written (so is a NULL pointer or a
 * file_offset + file_bytes beyond 64 bits).  h = |height|, pix_stride = 3 or 4, ch_offset = {0, 1, 2, 0} (the file order is B, G,
 * R); bottom-up: offset = file_offset + dataOff + (h - 1) * stride, row_stride = -stride; top-down: offset = file_offset +
 * dataOff, row_stride = stride. */
int qcnn_src_bmp(const uint8_t* file_host, size_t file_bytes, uint64_t file_offset, QcnnSrcPixels* out);
/* qcnn_forward_u8_resized_views / qcnn_forward_u8_relaxed_views on such images.  Everything but the place of a tap's byte is
 * defined there: scales, taps, weights, the division, the mean's position, mirroring, slot order, averaging, top-5, the three
 * optional outputs, the staging of the host arrays, asynchrony.  Given the planar descriptors the calls return the planar
 * calls' bits; a source of the full size through the resized call returns qcnn_forward_u8_views' bits under every layout.
 * Checked before anything is enqueued (non-zero, a message naming the image, outputs untouched): everything the planar call
 * checks — h, w >= 1 (Strict) or >= 2 (Relaxed) — and, in overflow-checked 64-bit arithmetic (a row_stride of INT64_MIN or an
 * offset near 2^64 is refused, not wrapped):
 *   a network of more than 4 input channels;  pix_stride < 1;  ch_offset[c] < 0 for a c < C;
 *   lowest byte touched   offset + min(0, (h-1) * row_stride)                                            below 0;
 *   highest byte touched  offset + max(0, (h-1) * row_stride) + (w-1) * pix_stride + max_c ch_offset[c]  >= src_bytes
 *                         (a layout whose last sample is byte src_bytes - 1 is accepted);
 *   highest - lowest >= 2^31 - 1  (the kernels keep offsets relative to `offset` in signed 32 bits).
 * row_stride is otherwise free: 0 and values smaller than a row are legal if in bounds. */
int qcnn_forward_u8_resized_views_strided(QcnnCtx* ctx, const uint8_t* src_dev, size_t src_bytes,
                                          const QcnnSrcPixels* imgs_host, int n, int full_h, int full_w,
                                          const float* mean_dev /* [C][full_h][full_w] or NULL */,
                                          const QcnnView* views_host, int n_views,
                                          float* prob_dev, uint16_t* top5_dev, float* prob_views_dev);
int qcnn_forward_u8_relaxed_views_strided(QcnnCtx* ctx, const uint8_t* src_dev, size_t src_bytes,
                                          const QcnnSrcPixels* imgs_host, int n, int full_h, int full_w,
                                          const float* mean_crop_dev /* [C][in_h][in_w] or NULL */,
                                          const QcnnAnchorView* views_host, int n_views,
                                          float* prob_dev, uint16_t* top5_dev, float* prob_views_dev);
/* YCbCr frames read IN PLACE: what JPEG and video decoders emit — NV12 / NV21, I420 / YV12, 4:4:4 planes, packed YUY2 / UYVY —
 * pitched, bottom-up or a region of a larger frame.  A frame is three sample planes over one source buffer; pixel (y, x) of the
 * h x w image the network sees has the three bytes
 *   Y  = src_dev[y_offset  + y * y_row_stride + x * y_pix_stride]
 *   Cb = src_dev[cb_offset + (y >> sub_y) * c_row_stride + (x >> sub_x) * c_pix_stride]
 *   Cr = src_dev[cr_offset + (y >> sub_y) * c_row_stride + (x >> sub_x) * c_pix_stride]
 * Chroma is REPLICATED, never interpolated (the resize that follows is the interpolation); the chroma planes have
 * ((h - 1) >> sub_y) + 1 rows and ((w - 1) >> sub_x) + 1 columns, so odd sizes are legal.  The pixel's network channels (0 = B,
 * 1 = G, 2 = R) are 8-bit values from 32-bit signed integer arithmetic, >> an arithmetic shift (floor):
 *   yy = (Y - y0) * ky;  cb = Cb - 128;  cr = Cr - 128
 *   R = clamp255((yy + crv * cr + 32768) >> 16)
 *   G = clamp255((yy - cbg * cb - crg * cr + 32768) >> 16)
 *   B = clamp255((yy + cbu * cb + 32768) >> 16)
 *   matrix            y0     ky     crv     cbg     crg     cbu
 *   QCNN_YUV_JFIF      0  65536   91881   22554   46802  116130      full-range BT.601 (JPEG): Cb = Cr = 128 gives B = G = R = Y
 *   QCNN_YUV_BT601    16  76309  104597   25675   53279  132201      limited range: 16 -> 0, 235 -> 255
 *   QCNN_YUV_BT709    16  76309  117489   13975   34925  138438      limited range
 * (no accumulator exceeds 3.6e7; every output lies within 1 of the rounded real-number formula).  Bytes that are no sample are
 * never read; planes and frames may alias. */
enum { QCNN_YUV_JFIF = 0, QCNN_YUV_BT601 = 1, QCNN_YUV_BT709 = 2 };   /* full-range BT.601 (JPEG); limited-range BT.601; limited-range BT.709 */
typedef struct {
  uint64_t y_offset, cb_offset, cr_offset;   /* byte, relative to the source buffer, of luma sample (0, 0) and of chroma samples (0, 0) */
  int64_t  y_row_stride, c_row_stride;       /* bytes between rows of the luma plane / of both chroma planes; any sign, 0 legal */
  int32_t  h, w;                             /* luma size = the image's size */
  int32_t  y_pix_stride, c_pix_stride;       /* >= 1.  planar 1 / 1, NV12 1 / 2, YUY2 2 / 4 */
  int32_t  sub_y, sub_x;                     /* 0 or 1: log2 of the chroma sub-sampling (4:4:4 = 0, 0; 4:2:2 = 0, 1; 4:2:0 = 1, 1) */
  int32_t  matrix;                           /* QCNN_YUV_* */
} QcnnSrcYuv;
/* The descriptor of a frame in one of the common layouts whose first byte will lie at src_dev + frame_offset (host only: no
 * device, no context).  pitch: bytes between luma rows, 0 = tight.
 *   QCNN_YUV_NV12 / _NV21   h luma rows of `pitch` bytes, then ceil(h / 2) rows of interleaved Cb Cr / Cr Cb at the same pitch
 *                           (tight: 2 * ceil(w / 2), the chroma row of an odd width is the longer one)
 *   QCNN_YUV_I420 / _YV12   luma, then the Cb and Cr (YV12: Cr and Cb) planes of ceil(h / 2) rows at pitch (pitch + 1) / 2
 *   QCNN_YUV_I444           three planes Y, Cb, Cr of `pitch`
 *   QCNN_YUV_YUY2 / _UYVY   packed 4:2:2, Y0 Cb Y1 Cr / Cb Y0 Cr Y1: y_pix_stride 2, c_pix_stride 4 (tight: 4 * ceil(w / 2))
 * Non-zero, nothing written: out NULL, an unknown format or matrix, h < 1 or w < 1, a pitch smaller than a row, a frame of
 * 2^31 - 1 bytes or more, frame_offset + the frame beyond 64 bits. */
enum { QCNN_YUV_NV12 = 0, QCNN_YUV_NV21 = 1, QCNN_YUV_I420 = 2, QCNN_YUV_YV12 = 3, QCNN_YUV_I444 = 4, QCNN_YUV_YUY2 = 5, QCNN_YUV_UYVY = 6 };
int qcnn_src_yuv_frame(int format, uint64_t frame_offset, int h, int w, int64_t pitch, int matrix, QcnnSrcYuv* out);
/* qcnn_forward_u8_resized_views_strided / qcnn_forward_u8_relaxed_views_strided on such frames: the 8-bit B, G, R values above
 * are the four taps of the bilinear resize, and everything from there on is defined there — scales, weights, the division, the
 * mean's position, mirroring, slot order, averaging, top-5, the three optional outputs, the staging of the host arrays,
 * asynchrony.  A call returns, bit for bit, what the strided call returns on the planar B, G, R image the conversion makes of
 * the frame.
 * Checked before anything is enqueued (non-zero, a message naming the image and the plane — luma, Cb or Cr —, outputs
 * untouched): everything the planar call checks — h, w >= 1 (Strict) or >= 2 (Relaxed) — and
 *   a network whose input has not 3 channels;  y_pix_stride or c_pix_stride < 1;  sub_y or sub_x outside {0, 1};  an unknown matrix;
 *   for each plane, in overflow-checked 64-bit arithmetic (an offset near 2^64 or a stride of INT64_MIN is refused, not wrapped),
 *   with rows x cols = h x w (luma) or the chroma size above:
 *     lowest byte touched   offset + min(0, (rows-1) * row_stride)                             below 0;
 *     highest byte touched  offset + max(0, (rows-1) * row_stride) + (cols-1) * pix_stride     >= src_bytes
 *                           (a layout whose last sample is byte src_bytes - 1 is accepted);
 *   highest - lowest OVER ALL THREE PLANES >= 2^31 - 1  (the kernels keep every offset relative to luma sample (0, 0) in signed
 *   32 bits).
 * The row strides are otherwise free: 0 and values smaller than a row are legal if in bounds. */
int qcnn_forward_u8_resized_views_yuv(QcnnCtx* ctx, const uint8_t* src_dev, size_t src_bytes,
                                      const QcnnSrcYuv* imgs_host, int n, int full_h, int full_w,
                                      const float* mean_dev /* [3][full_h][full_w] or NULL */,
                                      const QcnnView* views_host, int n_views,
                                      float* prob_dev, uint16_t* top5_dev, float* prob_views_dev);
int qcnn_forward_u8_relaxed_views_yuv(QcnnCtx* ctx, const uint8_t* src_dev, size_t src_bytes,
                                      const QcnnSrcYuv* imgs_host, int n, int full_h, int full_w,
                                      const float* mean_crop_dev /* [3][in_h][in_w] or NULL */,
                                      const QcnnAnchorView* views_host, int n_views,
                                      float* prob_dev, uint16_t* top5_dev, float* prob_views_dev);
/* Blocking convenience: host in, host out (H2D + forward + D2H + sync).  A batch of at least two chunks
 * (QCNN_OPT_HOST_CHUNK) goes through chunk by chunk, uploads overlapped with the previous chunk's layers. */
int qcnn_forward_host(QcnnCtx* ctx, const float* in_nchw_host, int n, float* prob_host, uint16_t* top5_host);
/* Blocking: nb batches one after the other — batch b = n[b] <= max_batch images at in_host[b]; prob_host / top5_host
 * (either may be NULL, and so may single entries) receive the results per batch.  The upload of batch b + 1 runs on a
 * copy stream under the layers of batch b (two device input buffers), results return through pinned buffers: with
 * registered (qcnn_host_register) or pinned input memory the kernels never wait for PCIe. */
int qcnn_forward_host_batches(QcnnCtx* ctx, const float* const* in_host, const int* n, int nb, float* const* prob_host,
                              uint16_t* const* top5_host);
/* The same schedule for 8-bit SOURCE images in host memory: what the reference's image loop does with a labelled set of files
 * (src/CaffeEva.cc:151-211: load, pre-process, classify batch after batch; :263-295: count the hits), with BmpImgIO::Load's
 * resize, mean and crop on the device.  A batch is its source bytes as they lie — BMP files, planar or interleaved images,
 * frames — and n descriptors whose offsets are relative to src_host (qcnn_src_planar / qcnn_src_bmp make them).  A 256 x 256
 * x 3 source is 196 608 bytes against the 618 348 of AlexNet's float crop, and with n_views views one source feeds n_views
 * batch slots.
 * Both calls are BLOCKING and mean qcnn_forward_u8_resized_views_strided / qcnn_forward_u8_relaxed_views_strided applied batch
 * after batch: prob_host [n][classes] and top5_host [n][5] are those of the view average, prob_views_host [n][n_views][classes]
 * the un-averaged rows, each bit for bit what the strided call writes for that batch; mean, views, full size as there.
 * Schedule: the source bytes (and labels) of batch b + 1 go up on the copy stream into one of two device buffers the context
 * owns (allocated at first use, grown — before the first upload of a call — when a call's largest src_bytes needs more, freed
 * with the context), under the layers of batch b; a buffer is handed back behind the PACK kernel of its batch, its last
 * reader; results return through pinned buffers one batch late.  No float input is ever staged.  With src_host in pinned
 * (qcnn_host_alloc) or registered memory the kernels never wait for PCIe; pageable memory is correct and slower.
 * labels: n ground-truth classes, or NULL = the batch is not counted.  hits5 (or NULL: nothing is counted) receives
 * CaffeEva::CalcPredAccu's five counters BEFORE its running sum (src/CaffeEva.cc:276-286) over the labelled batches of this
 * call: hits5[r] = #{ i : top5[i][r] == labels[i] } on the view-averaged top-5, one label per IMAGE (not per slot), every rank
 * tested by itself — a row that repeats a class (the reference's rows do, with class 0, once fewer than five probabilities
 * exceed FLT_MIN) counts it at every rank where it stands.  ACCURACY@k as Main.cc prints it is the CALLER's running sum
 * hits5[0] + ... + hits5[k-1] over the number of labelled images.  Counting happens on the device behind each labelled
 * batch's top-5 (qcnn_count_top5_hits into a counter block the context owns, zeroed at entry) with no host round trip per
 * batch; the five numbers are read back once, at the end.
 * Every batch is checked before anything is enqueued or any buffer rewritten — non-zero, a message that names the batch and
 * the image ("batch 3: image 17: ..."), every host output and hits5 untouched: nb <= 0, a NULL batches / views / src_host /
 * imgs, n <= 0, n * n_views > max_batch, every descriptor against its OWN batch's src_bytes and every view as the strided
 * calls check them, a label >= classes.  QCNN_DEBUG_PIPELINE=1 in the environment prints the schedule (upload and layer
 * intervals per batch) to stderr, as for qcnn_forward_host_batches. */
typedef struct QcnnU8Batch {
  const uint8_t* src_host; size_t src_bytes;   /* the batch's source bytes as they lie */
  const QcnnSrcPixels* imgs; int n;            /* n descriptors, offsets relative to src_host */
  const uint16_t* labels;                      /* n ground-truth classes, or NULL: batch not counted */
  float* prob_host; uint16_t* top5_host; float* prob_views_host;   /* each may be NULL */
} QcnnU8Batch;
int qcnn_forward_u8_resized_host_batches(QcnnCtx* ctx, const QcnnU8Batch* batches, int nb, int full_h, int full_w,
                                         const float* mean_dev /* [C][full_h][full_w] or NULL */,
                                         const QcnnView* views_host, int n_views, unsigned long long hits5[5] /* or NULL */);
int qcnn_forward_u8_relaxed_host_batches(QcnnCtx* ctx, const QcnnU8Batch* batches, int nb, int full_h, int full_w,
                                         const float* mean_crop_dev /* [C][in_h][in_w] or NULL */,
                                         const QcnnAnchorView* views_host, int n_views, unsigned long long hits5[5] /* or NULL */);
/* The same two calls for batches of YCbCr frames (qcnn_forward_u8_resized_views_yuv / _relaxed_views_yuv applied batch after
 * batch): a 4:2:0 frame is 1.5 bytes a pixel where B, G, R are 3.  Schedule, buffers, labels, hits5, checks and messages
 * ("batch 3: image 17: ...") are those above. */
typedef struct QcnnU8YuvBatch {
  const uint8_t* src_host; size_t src_bytes;   /* the batch's frames as they lie */
  const QcnnSrcYuv* imgs; int n;               /* n descriptors, offsets relative to src_host */
  const uint16_t* labels;                      /* n ground-truth classes, or NULL: batch not counted */
  float* prob_host; uint16_t* top5_host; float* prob_views_host;   /* each may be NULL */
} QcnnU8YuvBatch;
int qcnn_forward_u8_resized_host_batches_yuv(QcnnCtx* ctx, const QcnnU8YuvBatch* batches, int nb, int full_h, int full_w,
                                             const float* mean_dev /* [3][full_h][full_w] or NULL */,
                                             const QcnnView* views_host, int n_views, unsigned long long hits5[5] /* or NULL */);
int qcnn_forward_u8_relaxed_host_batches_yuv(QcnnCtx* ctx, const QcnnU8YuvBatch* batches, int nb, int full_h, int full_w,
                                             const float* mean_crop_dev /* [3][in_h][in_w] or NULL */,
                                             const QcnnAnchorView* views_host, int n_views, unsigned long long hits5[5] /* or NULL */);
/* The counting alone, asynchronous on the context's stream, DEVICE pointers: hits5_dev[r] += #{ i < n : top5_dev[i * 5 + r] ==
 * labels_dev[i] } for r = 0..4 — accumulated INTO the five counters, which the caller zeroes.  Integer sums: the same from run
 * to run.  Non-zero for a NULL pointer or n <= 0. */
int qcnn_count_top5_hits(QcnnCtx* ctx, const uint16_t* top5_dev, const uint16_t* labels_dev, int n,
                         unsigned long long* hits5_dev /* [5], accumulated into */);
/* Pin / unpin caller memory (hipHostRegister, portable across devices) so that uploads from it are asynchronous DMA
 * transfers.  Errors are reported through qcnn_last_error(NULL). */
int qcnn_host_register(void* ptr, size_t bytes);
int qcnn_host_unregister(void* ptr);
/* Pinned host memory from the HIP runtime (hipHostMalloc, portable): the fastest source / destination of a transfer
 * (measured on MI355X: uploads from it run at about twice the rate of uploads from registered pageable memory). */
int qcnn_host_alloc(size_t bytes, void** out);
int qcnn_host_free(void* ptr);
/* Feature map l of the last forward, images [0, n), NHWC per image, to host (blocking).
 * Requires QCNN_OPT_KEEP_ALL = 1 for maps that the fast path fuses away. */
int qcnn_get_layer_output(QcnnCtx* ctx, int l, int n, float* host_out);
/* Same for images [first, first + n) of the last forward (e.g. one image of the last, ragged panel). */
int qcnn_get_layer_output_range(QcnnCtx* ctx, int l, int first, int n, float* host_out);
/* Response error of one model against another, on the device: feature map l of the LAST forward of ctx (the subject, a) against
 * the same map of the last forward of ref (the reference, b), images [0, n), read where both forwards left them (panels
 * [E][128]) in one streaming pass — nothing but C rows of six doubles crosses PCIe.  (No counterpart in the reference, which
 * ships finished parameters; the quantity is the propagated response error of Wu et al., CVPR'16, section 5.)
 * Element e of an image has channel c = e % C (NHWC element order; behind an FC layer C is the node count and H * W = 1).  A
 * pair (image i < n, element e) is COUNTED when both values are finite; otherwise it adds 1 to `nonfinite` of its channel and
 * contributes to nothing else.  For a counted pair d = (double)a - (double)b — exact: the subtraction is never made in fp32.
 * Per channel, in fp64:
 *   count      counted pairs                     nonfinite  the others
 *   sum_d      sum of d                          sum_d2     sum of d * d (the product rounded once, then added)
 *   sum_ref2   sum of (double)b * (double)b      max_abs_d  largest |d| (0 when nothing is counted)
 * total_host = the per-channel rows added in ascending channel order in fp64 (max for max_abs_d), from the very rows
 * per_channel_host receives: total == fold(per_channel) bit for bit.
 * ORDER OF SUMMATION: a function of (H, W, C, n) alone — no floating-point atomics.  The rows of a channel (one per panel and
 * pixel, in that order) are cut into chunks of QCNN_DIFF_CHUNK_ROWS; a workgroup of 256 threads folds a chunk — thread t takes
 * images 4 (t % 32) .. + 3 of rows t / 32, t / 32 + 8, ... in ascending order, the 256 threads are added by a halving tree —
 * into one partial row of a scratch buffer; one wave per channel adds the partial rows (lane j: chunks j, j + 64, ... ascending,
 * then a halving tree).  Two calls on the same maps return the same bits whatever QCNN_OPT_STREAMS, QCNN_OPT_SMALL_BATCH or
 * the history of the contexts.  Lanes of images >= n contribute nothing, whatever an earlier, larger forward left there; nothing
 * beyond ceil(n / 128) panels of either map is addressed.
 * The two models need not be the same: only fm[l] must have the same (H, W, C).  ctx == ref is allowed (zeros, sum_ref2 =
 * sum of a * a).  Blocking: waits for both contexts' streams, runs on ctx's stream, copies the rows to the host.  The scratch
 * belongs to ctx (first use, grown on demand, freed with the context; no part of the commit plan).
 * Checked before any launch — non-zero, the cause in qcnn_last_error(ctx), both contexts still usable: a NULL context or
 * total_host; contexts on different devices; l outside [0, layer_cnt] of either; fm[l] dims that differ; n <= 0 or above either
 * context's last batch; a map either context cannot read back (the conditions and messages of qcnn_get_layer_output: no forward
 * yet, not materialised, fused away under QCNN_OPT_KEEP_ALL = 0).  With ctx == NULL the message is qcnn_last_error(NULL)'s. */
typedef struct { double count, nonfinite, sum_d, sum_d2, sum_ref2, max_abs_d; } QcnnMapDiff;
int qcnn_map_diff(QcnnCtx* ctx, QcnnCtx* ref, int l, int n,
                  QcnnMapDiff* total_host, QcnnMapDiff* per_channel_host /* [C of fm[l]] or NULL */);
/* Run layer `layer` alone on n images: in_host is fm[layer] NHWC per image (FC layers: the flat
 * vector in the order the reference consumes it), out_host receives fm[layer+1] (blocking). */
int qcnn_run_layer(QcnnCtx* ctx, int layer, const float* in_host, int n, float* out_host);

/* How the last launch of conv layer `layer` was cut (QCNN_OPT_SPLIT): *slices = workgroups per split tile (1 = no tile
 * was split), *tiles_unsplit = tiles of the heaviest-first order that ran whole (-1 when nothing was split); sliding
 * kernel (QCNN_OPT_SLIDE): *tiles_unsplit = -2, *slices = segments per output column; a conv or FC layer that ran through
 * its decoded code words (QCNN_OPT_DECODE): *tiles_unsplit = -3, *slices = 1 (FC: slices of the input axis over workgroups);
 * (a conv layer that read the NCHW batch in place: *slices = 2); symmetric workgroups (QCNN_OPT_SYM): *tiles_unsplit = -4;
 * eight-wave symmetric workgroups (QCNN_OPT_SYM8): -5 (conv tile form, *slices = slices per tile under QCNN_OPT_SPLIT, else 1; FC:
 * *slices = splits of the sub-space axis), -6 in their sliding form (*slices = segments per output column;
 * qcnn_get_layer_segments reports the boundaries); their fp16-storage form (QCNN_OPT_LUT_MODE = 2): -7, with fp16 sums too
 * (QCNN_OPT_LUT_MODE = 3): -8; the few-image kernels (QCNN_OPT_SMALL_BATCH, a forward of up to QCNN_SMALL_BATCH_MAX images, conv
 * and FC layers): -11, *slices = 1 — only when they took the launch: a layer whose shape they do not cover (a tap window x K beyond
 * their LDS table, an FC code book whose K is not a multiple of 4) reports the panel kernel that ran instead. */
int qcnn_get_layer_split(QcnnCtx* ctx, int layer, int* tiles_unsplit, int* slices);
/* A first conv layer that read the NCHW batch in place (qcnn_get_layer_split reports (-3, 2)): *form = the decoded form its last
 * launch ran — 0 f32 matrix instructions, 1 three bf16 pieces, 2 two fp16 pieces (QCNN_OPT_DEC_BF16SPLIT) —, -1 for any other
 * layer or kernel; *fallback_pairs = the (work item, image) pairs whose results the fix-up launch of form 2 recomputed in form 1
 * because the item's windows held a value outside [-1023, 1023] (NaN and Inf included), summed over the sub-batch launches of the
 * last forward (of its last chunk, for a chunked host batch); 0 for the other forms.  Either pointer may be NULL.  Blocking:
 * it waits for the context's streams and reads the guard regions back — for tests and diagnosis. */
int qcnn_get_layer_dec_form(QcnnCtx* ctx, int layer, int* form, long long* fallback_pairs);
/* Sliding kernel: the row segments [seg_beg9[i], seg_beg9[i + 1]) every output column of the last launch of `layer` was
 * cut into (*n_seg of them; 0 when the layer ran the tile kernel). */
int qcnn_get_layer_segments(QcnnCtx* ctx, int layer, int* seg_beg9, int* n_seg);

/* ---- launch planner (diagnostic; quantized-cnn_amd/csrc/qcnn_planner.h) ---- */
/* The plan and the choice for ONE conv launch, from plain numbers (needs no device, no context):
 *   geom[14] = H, W, Cin, Ho, Wo, Ct, knl, stride, pad, grp, M, Cs, K, panels          opts[8] = QCNN_OPT_SPLIT, _SLIDE, _SYM, _SYM8, _HALF8,
 *   QCNN_OPT_LUT_MODE, flags (1: the layer reads the NCHW input in place, 2: the panels are those of concurrent sub-batches —
 *   QCNN_OPT_STREAMS > 1), partial-sum scratch in Mi floats.
 *   costs[7] (predicted stage-times; 0 = not eligible) = tile kernel, 16-wave sliding, 16-wave symmetric, eight-wave tile, eight-wave
 *   sliding, half-panel tile, half-panel sliding.     choice[13] = family code (what qcnn_get_layer_split reports: -1 tile, -2, -4, -5,
 *   -6, -9, -10; never -11: the few-image kernels are the engine's choice, not the planner's), first split tile, slices, segments per column, nine segment boundaries.  Returns non-zero on a malformed geometry, pad < 0 and pad >= knl included (as qcnn_model_begin). */
int qcnn_plan_conv_query(const int* geom, const int* opts, double* costs, int* choice);

/* ---- timing (QCNN_OPT_PROFILE = 1) ---- */
/* Mean milliseconds of one LAUNCH per layer (a forward issues QCNN_OPT_STREAMS launches per layer, each over
 * its share of the panels) over the forwards recorded since the last reset; ms[layer_cnt]. */
int qcnn_get_layer_ms(QcnnCtx* ctx, float* ms, int* forwards_recorded);
/* Per layer: milliseconds SUMMED over every launch recorded since the last reset, and the number of launches
 * (either output may be NULL); nothing is dropped however many forwards were run. */
int qcnn_get_layer_total_ms(QcnnCtx* ctx, double* total_ms, long long* launches, int* forwards_recorded);
int qcnn_reset_layer_ms(QcnnCtx* ctx);

/* ---- device group: one batch sharded over the GPUs of a node ----
 * One context per device + one RCCL communicator over them (single process).  Images are independent: image i of
 * a batch of n goes to rank i * G / n (contiguous blocks); the only collective is the one-time ncclBroadcast of
 * rank 0's parameter arena over xGMI.  Model calls mirror the per-context ones and apply to every rank. */
typedef struct QcnnGroup QcnnGroup;
/* device_ids == NULL or n_dev <= 0: every visible device.  A device may be listed once; with QCNN_GROUP_ALLOW_DUP=1 in
 * the environment (test rigs with fewer GPUs than ranks) it may repeat: such a group has no RCCL communicator — RCCL
 * refuses two ranks on one device — and "broadcasts" rank 0's arena with device-to-device / peer copies instead; the
 * per-rank contexts, host threads and shard arithmetic are the production ones. */
int qcnn_group_create(const int* device_ids, int n_dev, QcnnGroup** out);
int qcnn_group_destroy(QcnnGroup* grp);
const char* qcnn_group_last_error(const QcnnGroup* grp);   /* grp == NULL: error of qcnn_group_create */
int qcnn_group_size(const QcnnGroup* grp);
QcnnCtx* qcnn_group_ctx(QcnnGroup* grp, int rank);         /* per-rank context: options, dumps, timing */
int qcnn_group_shard_bounds(const QcnnGroup* grp, int n, int rank, int* first, int* count);
int qcnn_group_set_option(QcnnGroup* grp, int option, int value);
int qcnn_group_model_begin(QcnnGroup* grp, int layer_cnt, const QcnnLayerDesc* layers, int in_c, int in_h, int in_w);
int qcnn_group_model_set_layer_shape(QcnnGroup* grp, int layer, int M, int K, int Cs);
int qcnn_group_model_set_layer_dense(QcnnGroup* grp, int layer);
int qcnn_group_model_set_layer_weights(QcnnGroup* grp, int layer, const float* bias, const float* weights_file);   /* rank 0 */
/* max_batch: images of one GLOBAL batch; every rank plans the largest block it can be handed */
int qcnn_group_model_commit(QcnnGroup* grp, int max_batch);
/* uploads to rank 0 only; qcnn_group_model_broadcast then ships the packed arena to the other ranks */
int qcnn_group_model_set_layer_params(QcnnGroup* grp, int layer, const float* bias, const float* ctrd_file,
                                      const uint8_t* asmt_file);
/* Ships rank 0's arena to every other rank (RCCL broadcast over xGMI), then compares a device-side checksum of every rank's
 * arena with rank 0's (qcnn_model_arena_checksum): a mismatch is an error, no rank is declared loaded. */
int qcnn_group_model_broadcast(QcnnGroup* grp, float* elapsed_ms);
/* The checksum pair every rank agreed on at the last broadcast. */
int qcnn_group_arena_checksum(QcnnGroup* grp, unsigned long long* sum2);
/* Blocking: host in, host out; one host thread per GPU runs its block on its own context and stream. */
int qcnn_group_forward_host(QcnnGroup* grp, const float* in_nchw_host, int n, float* prob_host, uint16_t* top5_host);
/* Blocking: nb global batches of n[b] images each, every one sharded over the ranks like qcnn_group_forward_host; a
 * rank's uploads overlap its layers as in qcnn_forward_host_batches. */
int qcnn_group_forward_host_batches(QcnnGroup* grp, const float* const* in_host, const int* n, int nb,
                                    float* const* prob_host, uint16_t* const* top5_host);
/* Asynchronous, device-resident: in_dev[r] / prob_dev[r] / top5_dev[r] are pointers ON RANK r's DEVICE to that rank's block of the
 * batch (qcnn_group_shard_bounds; NULL entries for ranks whose block is empty, prob_dev / top5_dev may be NULL altogether).  Every
 * rank's layers are enqueued on its own stream — no host thread, no PCIe: what a caller that already holds the images on the
 * GPUs uses, and what times the sharded batch without the uploads.  qcnn_group_sync waits for all ranks. */
int qcnn_group_forward(QcnnGroup* grp, const float* const* in_dev, int n, float* const* prob_dev, uint16_t* const* top5_dev);
int qcnn_group_sync(QcnnGroup* grp);

#ifdef __cplusplus
}
#endif
#endif /* QCNN_HIP_H_ */
