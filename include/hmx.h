/*
 * hmx.h -- C-ABI of libhmx: the MI355X (gfx950) implementation of the HM block hot path.
 *
 * Drop-in boundary for the reference's block kernels.  The reference (fr34k8/thevc = HM 7.2/8-dev)
 * has no plugin/FFI layer: the boundary is the member-function surface of TComTrQuant,
 * TComPrediction/TComPattern and TComInterpolationFilter, called only from TEncSearch, TEncCu and
 * TDecCu.  Every entry point below names the reference member it replaces (file:line, paths
 * relative to /root/reference/source/Lib/).  Two families:
 *
 *   hmx_<name>        scalar drop-ins: the reference's own argument order, HOST pointers, one block
 *                     per call.  Hidden reference state (bit-depth globals, m_cQP, TComDataCU
 *                     getters) becomes the context handle and explicit scalars.  They run the
 *                     same HIP kernels as the batched path with a batch of one (H2D, launch, D2H);
 *                     there is no CPU arithmetic in this library.
 *   hmx_batch_<name>  the throughput path: DEVICE pointers, descriptor arrays, asynchronous on
 *   hmx_frame_<name>  the context's HIP stream.
 *
 * Types: Pel = int16_t, TCoeff = int32_t (TLibCommon/TypeDef.h:297-298); strides in elements.
 * All functions return 0 on success, a negative hmx_status otherwise (the reference returns Void
 * and asserts; hmx_last_error() gives the text).
 */
#ifndef HMX_H
#define HMX_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef int16_t hmx_pel;
typedef int32_t hmx_coeff;
typedef struct hmx_ctx hmx_ctx;

enum hmx_status {
  HMX_OK = 0,
  HMX_ERR_ARG = -1,     /* unsupported size / null pointer (the reference asserts or falls through) */
  HMX_ERR_DEVICE = -2,  /* HIP runtime error */
  HMX_ERR_NOMEM = -3,
  HMX_ERR_INTERNAL = -4 /* a self-check of the library failed (hmx_aq_thresholds) */
};

#define HMX_REG_DCT 65535u /* TLibCommon/TypeDef.h:239 */
enum hmx_text_type { HMX_TEXT_LUMA = 0, HMX_TEXT_CHROMA = 1, HMX_TEXT_CHROMA_U = 2, HMX_TEXT_CHROMA_V = 3 };
enum hmx_slice_type { HMX_B_SLICE = 0, HMX_P_SLICE = 1, HMX_I_SLICE = 2 };

/* ------------------------------------------------------------------------------------------------
 * Context: replaces the process globals g_uiBitDepth/g_uiBitIncrement/g_uiIBDI_MAX
 * (TLibCommon/TComRom.cpp:445-448) and the scratch members of the three classes.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int bit_depth; /* internal bit depth B = g_uiBitDepth + g_uiBitIncrement (8 or 10 in the cfgs) */
  int device;    /* HIP device ordinal */
  void *stream;  /* hipStream_t to launch on; NULL = the library creates its own */
  int ctu_size;  /* g_uiMaxCUWidth, 64 in every shipped cfg */
} hmx_config;

int hmx_create(const hmx_config *cfg, hmx_ctx **out);
void hmx_destroy(hmx_ctx *ctx);
const char *hmx_last_error(const hmx_ctx *ctx);
int hmx_sync(hmx_ctx *ctx);
/* Tuning knobs (the reference has none: these select between schedules of the SAME arithmetic for A/B runs and
 * cross-checks).  Each is read once from the environment variable of the same name in hmx_create; hmx_set_option
 * changes one afterwards, value NULL restores the default.  HMX_INTRA_SCHEDULE = packed (default) | level | wave,
 * HMX_INTRA_ACROSS, HMX_INTRA_STREAMS, HMX_PIPELINE_CONV, HMX_GRAPH (level schedules), HMX_PACK_SLOTS4 = 16 | 64, HMX_PACK_SLOTS8 = 8 | 16,
 * HMX_PACK_GROUP, HMX_PACK_WAVES, HMX_PACK_SLEEP0, HMX_PACK_SLEEP1 (packed schedule), HMX_RDOQ_LANE (RDOQ: every block
 * through the one-lane-per-block kernel), HMX_PLAN_ROWS (device plan builder: rows of the level table per picture to start with), HMX_PLAN_STREAMS (1: its luma and chroma
 * level walks one after the other instead of side by side on two streams), HMX_TZ_MAX_PASSES = 1 .. 1024 (hmx_batch_tz_search:
 * star-refinement passes of one unit before it is answered with the all-ones cost; a guard, not a tuning knob; default 1024). */
int hmx_set_option(hmx_ctx *ctx, const char *name, const char *value);
/* device memory + timing plumbing so that callers need no HIP headers */
int hmx_malloc(hmx_ctx *ctx, size_t bytes, void **dptr);
int hmx_free(hmx_ctx *ctx, void *dptr);
int hmx_upload(hmx_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int hmx_download(hmx_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int hmx_memset(hmx_ctx *ctx, void *dst_dev, int value, size_t bytes);
int hmx_event_create(hmx_ctx *ctx, void **ev);
int hmx_event_record(hmx_ctx *ctx, void *ev); /* on the context's stream */
int hmx_event_elapsed_ms(hmx_ctx *ctx, void *ev_start, void *ev_stop, float *ms); /* syncs ev_stop */
int hmx_event_destroy(hmx_ctx *ctx, void *ev);

/* ------------------------------------------------------------------------------------------------
 * Quantiser state.  TComTrQuant::setQPforQuant (TLibCommon/TComTrQuant.cpp:192-222) writes the
 * hidden member m_cQP (QpParam, TComTrQuant.h:79-113); here it returns the value.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int qp, per, rem, bits;
} hmx_qp;
hmx_qp hmx_setQPforQuant(int qpy, int text_type, int qp_bd_offset, int chroma_qp_offset);

/* What xQuant reads through TComDataCU / TComSlice / TComPPS (TComTrQuant.cpp:1121-1267) */
typedef struct {
  hmx_qp qp;          /* m_cQP */
  int per_base;       /* cQpBase.m_iPer from getSliceQpBase() (ADAPTIVE_QP_SELECTION); -1 = qp.per */
  int slice_type;     /* hmx_slice_type: rounding 171 (I) / 85 */
  int sign_hide;      /* PPS getSignHideFlag() */
  int is_intra;       /* pcCU->isIntra(uiAbsPartIdx) */
  int dir_mode;       /* luma/chroma intra direction used by getCoefScanIdx (TComDataCU.cpp:4014) */
} hmx_quant_param;

/* ------------------------------------------------------------------------------------------------
 * Scalar drop-ins, TComTrQuant
 * ---------------------------------------------------------------------------------------------- */
/* xT  (TComTrQuant.cpp:1542): strided Pel residual -> Int[w*h]; w == h in {4,8,16,32} */
int hmx_xT(hmx_ctx *ctx, unsigned mode, const hmx_pel *resi, unsigned stride, int32_t *coef, int w, int h);
/* xIT (TComTrQuant.cpp:1583) */
int hmx_xIT(hmx_ctx *ctx, unsigned mode, const int32_t *coef, hmx_pel *resi, unsigned stride, int w, int h);
/* xTransformSkip / xITransformSkip (TComTrQuant.cpp:1622, 1667) */
int hmx_xTransformSkip(hmx_ctx *ctx, const hmx_pel *resi, unsigned stride, int32_t *coef, int w, int h);
int hmx_xITransformSkip(hmx_ctx *ctx, const int32_t *coef, hmx_pel *resi, unsigned stride, int w, int h);
/* xQuant, flat path + signBitHidingHDQ (TComTrQuant.cpp:1102-1270, 977-1100); ac_sum accumulates */
int hmx_xQuant(hmx_ctx *ctx, const int32_t *src, hmx_coeff *dst, int w, int h, uint32_t *ac_sum,
               int text_type, const hmx_quant_param *qp);
/* xDeQuant with a scaling list (TComTrQuant.cpp:1311-1342, getUseScalingList()): dequant_coef[w*h] = the table
 * getDequantCoeff(scalingListType, m_cQP.m_iRem, log2(w) - 2, SCALING_LIST_SQT) that setScalingListDec built from the slice's lists
 * (:2773-2793, 2852-2873: header handling, stays in HM).  Host pointers like the other scalar drop-ins. */
int hmx_xDeQuant_scaled(hmx_ctx *ctx, const hmx_coeff *src, int32_t *dst, int w, int h, const hmx_qp *qp, const int32_t *dequant_coef);
/* The pArlDes output of xQuant (ADAPTIVE_QP_SELECTION, m_bUseAdaptQpSelect): arl[n] = (|src[n]| * quantScale + round) >> (iQBits - 7),
 * what TEncSlice's adaptive QP selection accumulates.  rdoq_form = 0: the flat branch (TComTrQuant.cpp:1229-1249; iQBits from
 * qp->per_base, the slice's base QP); rdoq_form = 1: as xRateDistOptQuant writes it (:1757-1765, 1886-1891; iQBits from qp->qp.per,
 * the product limited to MAX_INT - (1 << (iQBits - 1)) first).  It depends on the coefficients alone: call it beside hmx_xQuant /
 * hmx_xRateDistOptQuant when the encoder runs with AdaptiveQpSelection. */
int hmx_arlCoeff(hmx_ctx *ctx, const int32_t *src, int32_t *arl, int w, int h, int text_type, const hmx_quant_param *qp, int rdoq_form,
                 const int32_t *quant_coef /* getQuantCoeff table of a scaling list, or NULL */);
/* The quantisers with a scaling list (getUseScalingList()): the per-position tables HM's setScalingList built for the block's list
 * type, QP remainder and size are INPUTS (building them from the slice's lists is header handling, TComTrQuant.cpp:2747-2847, 2953-
 * 2977) -- quant_coef = getQuantCoeff(...), err_scale = getErrScaleCoeff(...), w*h entries each, row-major.
 * hmx_xQuant_scaled: xQuant's flat branch (:1215, 1244-1255) + signBitHidingHDQ.
 * hmx_xRateDistOptQuant_scaled: xRateDistOptQuant (:1759-1762, 1882-1883). */
int hmx_xQuant_scaled(hmx_ctx *ctx, const int32_t *src, hmx_coeff *dst, int w, int h, uint32_t *ac_sum, int text_type,
                      const hmx_quant_param *qp, const int32_t *quant_coef);
/* xRateDistOptQuant (TComTrQuant.cpp:1719-2305), the quantiser transformNxN selects when RDOQ is on
 * (:1122-1128; every shipped cfg).  It reads CABAC bit estimates that TEncSbac::estBit leaves in
 * m_pcEstBitsSbac for the block's size and texture type (estBitsSbacStruct, TComTrQuant.h:59-72; same
 * field order here, 1/32768 bit) and the Lagrange multiplier m_dLambda: both are inputs. */
typedef struct hmx_est_bits {
  int32_t significantCoeffGroupBits[2][2];
  int32_t significantBits[42][2];
  int32_t lastXBits[32];
  int32_t lastYBits[32];
  int32_t greaterOneBits[24][2];
  int32_t levelAbsBits[6][2];
  int32_t blockCbpBits[15][2];
  int32_t blockRootCbpBits[4][2];
  int32_t scanZigzag[2];
  int32_t scanNonZigzag[2];
} hmx_est_bits;
typedef struct hmx_rdoq_param {
  hmx_qp qp;       /* m_cQP */
  int sign_hide;   /* PPS getSignHideFlag() */
  int is_intra;    /* pcCU->isIntra(uiAbsPartIdx) */
  int dir_mode;    /* intra direction used by getCoefScanIdx */
  int root_cbf;    /* 1: inter luma block with transform index 0 -> blockRootCbpBits[0] (:2139-2144) */
  int cbf_ctx;     /* otherwise the index into blockCbpBits, texture offset included (:2147-2150) */
  double lambda;   /* m_dLambda */
} hmx_rdoq_param;
int hmx_xRateDistOptQuant(hmx_ctx *ctx, const int32_t *src, hmx_coeff *dst, int w, int h, uint32_t *abs_sum,
                          int text_type, const hmx_rdoq_param *rp, const hmx_est_bits *est);
int hmx_xRateDistOptQuant_scaled(hmx_ctx *ctx, const int32_t *src, hmx_coeff *dst, int w, int h, uint32_t *abs_sum, int text_type,
                                 const hmx_rdoq_param *rp, const hmx_est_bits *est, const int32_t *quant_coef, const double *err_scale);
/* xDeQuant, flat path (TComTrQuant.cpp:1272-1355) */
int hmx_xDeQuant(hmx_ctx *ctx, const hmx_coeff *src, int32_t *dst, int w, int h, const hmx_qp *qp);
/* transformNxN (TComTrQuant.cpp:1373-1426): uiMode is derived as the reference does
 * (luma && intra -> dir_mode, else REG_DCT) */
int hmx_transformNxN(hmx_ctx *ctx, const hmx_pel *resi, unsigned stride, hmx_coeff *level, unsigned w,
                     unsigned h, uint32_t *abs_sum, int text_type, const hmx_quant_param *qp,
                     int use_transform_skip, int trans_quant_bypass);
/* invtransformNxN (TComTrQuant.cpp:1428-1450); scaling lists are off in every shipped cfg */
int hmx_invtransformNxN(hmx_ctx *ctx, int trans_quant_bypass, int text_type, unsigned mode, hmx_pel *resi,
                        unsigned stride, const hmx_coeff *level, unsigned w, unsigned h, const hmx_qp *qp,
                        int use_transform_skip);

/* ------------------------------------------------------------------------------------------------
 * Scalar drop-ins, TComPattern / TComPrediction (intra)
 * ---------------------------------------------------------------------------------------------- */
/* initAdiPattern / initAdiPatternChroma (TLibCommon/TComPattern.cpp:213-366): rec = sample (0,0) of a
 * HOST reconstruction plane; (x,y,n) = block position/size in samples of that plane; neighbour
 * availability is derived geometrically for one slice / one tile / no constrained intra pred
 * (TComDataCU.cpp:1221-1735).  adi receives the reference layout: (2n+1)^2 Int border buffer and,
 * for luma, the [1 2 1]-smoothed copy behind it.  adi must hold 2*(2n+1)^2 ints. */
int hmx_initAdiPattern(hmx_ctx *ctx, const hmx_pel *rec, int stride, int x, int y, int n, int is_chroma,
                       int pic_w_luma, int pic_h_luma, int32_t *adi);
/* Slices, tiles and constrained intra prediction in the availability of intra neighbours.  HM marks a neighbour unit
 * unavailable when it lies in another slice or another tile (TComDataCU.cpp:1221-1735, getPU* with bEnforceSliceRestriction
 * and the getTileIdxMap checks), or, with constrained_intra_pred_flag, when it is not intra-coded (TComPattern.cpp:607-786).
 * A region is one (independent slice, tile) pair: dependent slices do not split regions (TComPattern calls getPU* with
 * bEnforceDependentSliceRestriction = false).  Slices start at CTU boundaries (SliceGranularity 0).  The layout only ever
 * REMOVES units from the geometric availability of hmx_intra_avail_mask.  A NULL layout, or one with both maps NULL, is one
 * region with CIP off and gives exactly what the entry points without a layout give.  A layout whose sizes do not fit the
 * picture, or that turns CIP on without a map, is refused with HMX_ERR_ARG. */
typedef struct {
  const uint32_t *ctu_region; /* region id of every CTU in raster order (n_ctu entries); NULL = one region */
  int n_ctu;                  /* entries of ctu_region: ceil(pic_w / ctu) * ceil(pic_h / ctu) */
  int constrained_intra_pred; /* PPS constrained_intra_pred_flag; 1 needs intra_unit */
  const uint8_t *intra_unit;  /* nonzero = the 4x4 luma unit (ux, uy) is intra-coded: intra_unit[uy * intra_stride + ux] */
  int intra_stride;           /* >= ceil(pic_w / 4) */
  int intra_rows;             /* rows of intra_unit, >= ceil(pic_h / 4) */
} hmx_avail_layout;
/* fillReferenceSamples (TLibCommon/TComPattern.cpp:368-552) in the reference's own argument order: the reference line of an
 * N x N block from HOST samples around rec (= sample (0,0) of the block; rows above and columns left of it are read where
 * flagged), with the caller's bNeighborFlags (4 * N / unit + 1 bytes, below-left bottom first, left, corner, above,
 * above-right), iNumIntraNeighbor = n_avail and iUnitSize = unit (4 luma, 2 chroma; N = 64 with unit 4 is the 64 x 64 luma
 * prediction unit).  adi receives the (2N+1)^2 border buffer (no smoothing: that is initAdiPattern's). */
int hmx_fillReferenceSamples(hmx_ctx *ctx, const hmx_pel *rec, int stride, const uint8_t *flags, int n_avail, int unit, int n,
                             int32_t *adi);
/* hmx_initAdiPattern with the slice / tile / CIP layout of the picture (TComPattern.cpp:213-366 with the availability of
 * :607-786); luma is smoothed as hmx_initAdiPattern smooths it.  layout = NULL: hmx_initAdiPattern. */
int hmx_initAdiPattern_layout(hmx_ctx *ctx, const hmx_pel *rec, int stride, int x, int y, int n, int is_chroma,
                              int pic_w_luma, int pic_h_luma, const hmx_avail_layout *layout, int32_t *adi);
/* predIntraLumaAng / predIntraChromaAng (TLibCommon/TComPrediction.cpp:338-386) */
int hmx_predIntraLumaAng(hmx_ctx *ctx, const int32_t *adi, unsigned dir_mode, hmx_pel *pred, unsigned stride,
                         int w, int h);
int hmx_predIntraChromaAng(hmx_ctx *ctx, const int32_t *adi, unsigned dir_mode, hmx_pel *pred, unsigned stride,
                           int w, int h);
/* The protected building blocks of the two wrappers (TComPrediction.cpp:129-167, 190-336, 689-730), named by
 * the north star.  `adi` is ONE (2w+1) x (2w+1) border buffer (raw or smoothed: the reference's callers choose
 * by passing a pointer; the reference's pSrc is its cell (1,1)).  xPredIntraAng: dir_mode 1 = DC from the
 * sides flagged available (no edge smoothing: xDCPredFiltering is the wrapper's), 2..34 angular, `filter` =
 * bFilter (edge filter of the pure vertical / horizontal modes). */
int hmx_predIntraGetPredValDC(hmx_ctx *ctx, const int32_t *adi, int w, int h, int above, int left, hmx_pel *dc);
int hmx_xPredIntraPlanar(hmx_ctx *ctx, const int32_t *adi, hmx_pel *pred, unsigned stride, int w, int h);
int hmx_xPredIntraAng(hmx_ctx *ctx, const int32_t *adi, hmx_pel *pred, unsigned stride, int w, int h, unsigned dir_mode,
                      int above, int left, int filter);

/* ------------------------------------------------------------------------------------------------
 * Scalar drop-ins, TComRdCost (TLibCommon/TComRdCost.cpp): calcHAD :404-450 (same argument order) and
 * getDistPart(piCur, iCurStride, piOrg, iOrgStride, w, h, false, DF_SSE) :452-478 -> xGetSSE* :1313-1657
 * (the IBDI_DISTORTION 0 variant: per-sample (diff^2) >> 2*bitIncrement).  w, h <= 64.
 * ---------------------------------------------------------------------------------------------- */
int hmx_calcHAD(hmx_ctx *ctx, const hmx_pel *pi0, int stride0, const hmx_pel *pi1, int stride1, int w, int h,
                uint32_t *satd);
int hmx_getSSE(hmx_ctx *ctx, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h,
               uint32_t *sse);
/* TComRdCost::xGetSAD4/8/12/16/24/32/48/64 (TComRdCost.cpp:518-..., dispatch :298-329), bApplyWeight false: the sum of
 * |org - cur| over all w columns of the rows 0, 2^sub_shift, 2 * 2^sub_shift, ... < h; *sad = (sum << sub_shift) >> (bit
 * depth - 8), UInt arithmetic.  w, h from {4, 8, 12, 16, 24, 32, 48, 64}; sub_shift 0, or 1 with h > 8 (what xPatternSearch
 * sets under getUseFastEnc(), TEncSearch.cpp:4245-4251; the reference never sub-samples 8 rows or fewer: HMX_ERR_ARG). */
int hmx_getSAD(hmx_ctx *ctx, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int sub_shift,
               uint32_t *sad);
/* TComRdCostWeightPrediction::xGetSADw (TComRdCostWeightPrediction.cpp:69-104) and xGetHADsw (:490-561), what xGetSAD* / xGetHADs
 * return when DistParam::bApplyWeight is set (TComRdCost.cpp:492 ..., :2188).  Host pointers, sizes as hmx_getSAD.  (weight,
 * offset, log2_denom) = the luma wpScalingParam of the reference searched (ranges as hmx_wp: anything else is HMX_ERR_ARG); with
 * round = log2_denom ? 1 << (log2_denom - 1) : 0 every sample c of cur becomes
 *   pred = (int16_t)(((weight * c + round) >> log2_denom) + offset * 2^(B-8))     -- product in int, wrapped to 16 bits, NOT clipped
 * hmx_getSADw: *sad = (sum of |org - pred| over ALL rows) >> (B - 8); there is no sub_shift: xGetSADw ignores iSubShift.
 * hmx_getHADsw: the Hadamard sum of org - pred over 8x8 sub-blocks when both sides are multiples of 8, else 4x4, each sub-block
 * rounded on its own ((sum + 2) >> 2, (sum + 1) >> 1), the total >> (B - 8).  xCalcHADs4x4w / xCalcHADs8x8w (:204-423) were read
 * against the unweighted functions: the same butterflies and the same roundings, only the difference is formed from pred. */
int hmx_getSADw(hmx_ctx *ctx, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int weight,
                int offset, int log2_denom, uint32_t *sad);
int hmx_getHADsw(hmx_ctx *ctx, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int weight,
                 int offset, int log2_denom, uint32_t *satd);

/* ------------------------------------------------------------------------------------------------
 * Scalar drop-ins, TComInterpolationFilter (TLibCommon/TComInterpolationFilter.cpp:323-415) and
 * TComYuv::addAvg (TLibCommon/TComYuv.cpp:520-581).  src must be readable 3 (luma) / 1 (chroma)
 * samples before and 4 / 2 after the block in the filtered direction, as in the reference.
 * ---------------------------------------------------------------------------------------------- */
int hmx_filterHorLuma(hmx_ctx *ctx, const hmx_pel *src, int src_stride, int16_t *dst, int dst_stride, int w,
                      int h, int frac, int is_last);
int hmx_filterVerLuma(hmx_ctx *ctx, const hmx_pel *src, int src_stride, int16_t *dst, int dst_stride, int w,
                      int h, int frac, int is_first, int is_last);
int hmx_filterHorChroma(hmx_ctx *ctx, const hmx_pel *src, int src_stride, int16_t *dst, int dst_stride, int w,
                        int h, int frac, int is_last);
int hmx_filterVerChroma(hmx_ctx *ctx, const hmx_pel *src, int src_stride, int16_t *dst, int dst_stride, int w,
                        int h, int frac, int is_first, int is_last);
int hmx_addAvg(hmx_ctx *ctx, const hmx_pel *src0, int s0_stride, const hmx_pel *src1, int s1_stride,
               hmx_pel *dst, int dst_stride, int w, int h);
/* TComPrediction::xPredInterLumaBlk / xPredInterChromaBlk (TLibCommon/TComPrediction.cpp:554-585, :599-642) for one block:
 * ref = the reference plane at the block's own position (refPic->getLumaAddr(cuAddr, zorder + partAddr); the reference
 * adds the vector's integer part itself), mv in quarter-pel luma units, bi = the block is one half of a bi-prediction
 * (output = the 14-bit intermediate, not clipped).  w, h: LUMA size of the block (the chroma form halves it, like the
 * reference); dst stride in elements.  The planes must be readable 3 (1) samples before and 4 (2) after the moved block. */
int hmx_xPredInterLumaBlk(hmx_ctx *ctx, const hmx_pel *ref, int ref_stride, int mv_hor, int mv_ver, int w, int h, hmx_pel *dst,
                          int dst_stride, int bi);
int hmx_xPredInterChromaBlk(hmx_ctx *ctx, const hmx_pel *ref, int ref_stride, int mv_hor, int mv_ver, int w, int h, hmx_pel *dst,
                            int dst_stride, int bi);

/* ------------------------------------------------------------------------------------------------
 * Batched device path
 * ---------------------------------------------------------------------------------------------- */
/* One transform / prediction block.  8 bytes, identical on host and device. */
typedef struct {
  uint16_t x, y;  /* position in samples of its plane */
  uint8_t log2n;  /* 2..5; 6 = the 64x64 luma prediction unit of a 64x64 coding unit, prediction entry points only */
  uint8_t plane;  /* 0 Y, 1 Cb, 2 Cr */
  uint8_t mode;   /* intra prediction mode 0..34 (also selects DST for 4x4 luma and the scan) */
  uint8_t flags;  /* HMX_TU_* */
} hmx_tu;
#define HMX_TU_TRANSFORM_SKIP 1u
#define HMX_TU_INTER 2u /* non-intra CU: REG_DCT, diagonal scan, no DST */
#define HMX_TU_CBF_CTX(ctx) (((unsigned)(ctx) & 15u) << 4) /* bits 4..7: context of the coded-block flag (hmx_set_rdoq) */

typedef struct {
  int pic_w, pic_h;      /* luma size of the picture */
  int qp;                /* CU QP (pcCU->getQP(0)); one QP per call -- not used for quantisation while a map is set (hmx_set_qp_map) */
  int chroma_qp_offset;  /* PPS cb/cr offset */
  int slice_type;        /* hmx_slice_type */
  int sign_hide;
} hmx_pic_param;

/* A picture in HBM: three Pel planes; plane[i] points at sample (0,0); stride in elements. */
typedef struct {
  hmx_pel *plane[3];
  int stride[3];
} hmx_pic;
/* Quantised levels.  stride[p] > 0: plane geometry, level of sample (x,y) of plane p at
 * plane[p][y*stride[p]+x].  stride[p] == 0 (whole-picture calls only): the reference's own coefficient
 * layout (TComDataCU::m_pcTrCoeffY/Cb/Cr, TLibCommon/TComDataCU.cpp:117-141): CTU blocks in raster order,
 * C*C ints each (C = CTU size in that plane, planes padded to whole CTUs); inside a CTU the N x N block
 * of the transform block whose first 4x4 unit is (ux,uy) starts at 16 * Zorder(ux,uy), row-major. */
typedef struct {
  hmx_coeff *plane[3];
  int stride[3];
} hmx_levels;

/* A list of blocks resident on the device.  Built once from a HOST array (the library buckets the
 * blocks by size: one launch per size class) and reused by any number of batch calls. */
typedef struct hmx_tu_list hmx_tu_list;
int hmx_tu_list_create(hmx_ctx *ctx, const hmx_tu *tus, int n, hmx_tu_list **list);
void hmx_tu_list_destroy(hmx_ctx *ctx, hmx_tu_list *list);

/* transformNxN over a list of independent blocks (HOT LOOP B' of ENC/TEncSearch.cpp:4784-4990):
 * residual planes -> level planes; d_abs_sum[i] = uiAbsSum of block i in the caller's order
 * (device pointer, may be NULL). */
int hmx_batch_transformNxN(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_pic *resi, const hmx_levels *lev,
                           uint32_t *d_abs_sum, const hmx_pic_param *pp);
/* The inter residual path in one pass (ENC/TEncSearch.cpp:4526-4990): residual = org - pred
 * (TComYuv::subtract, TLibCommon/TComYuv.cpp:461-518) fused into transformNxN. */
int hmx_batch_residual_transformNxN(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_pic *org, const hmx_pic *pred,
                                    const hmx_levels *lev, uint32_t *d_abs_sum, const hmx_pic_param *pp);
/* invtransformNxN over a list of blocks (DEC/TDecCu.cpp:791-831): levels -> residual planes `out`;
 * when pred != NULL the reconstruction Clip(pred + resi) is written instead (TComYuv::addClip). */
int hmx_batch_invtransformNxN(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_levels *lev, const hmx_pic *pred,
                              const hmx_pic *out, const hmx_pic_param *pp);
/* RDOQ over a list of blocks (host list): Int coefficients in `coef` (plane geometry, e.g. the output of the
 * xT drop-in or of a batch transform without quantisation) -> levels in `lev`; d_abs_sum[i] (device, may be
 * NULL) receives block i's absolute sum.  side[i] carries what the reference reads from the CU for block i
 * and which bit-estimate table (est[side[i].est_idx], host array) applies.  8x8 and larger blocks: a wave shares 8 / 4 / 1
 * blocks in LDS, coefficient groups walked in parallel (thevc_amd/csrc/hmx_rdoq_core.h); 4x4 blocks: one lane per block.
 * Coefficients are what xT / xTransformSkip produce: |c| <= 32768.  Levels are Int as in the reference, not clipped: when the
 * QP, bit depth and block sizes of a call allow |level| = (32768 * quantScale) >> qbits > 32767 (e.g. 10 bit, QP < 5 with 32x32
 * blocks), whose levels the wave-cooperative routine would keep in 16 bits, every block of the call runs one lane per block
 * instead (the same holds for hmx_xRateDistOptQuant).  The block list and the tables stay resident on the device while the
 * arguments repeat. */
typedef struct hmx_rdoq_side {
  uint16_t est_idx;
  uint8_t root_cbf, cbf_ctx;
} hmx_rdoq_side;
int hmx_batch_xRateDistOptQuant(hmx_ctx *ctx, const hmx_tu *tus, const hmx_rdoq_side *side, int n, const hmx_levels *coef,
                                const hmx_levels *lev, uint32_t *d_abs_sum, const hmx_pic_param *pp,
                                const hmx_est_bits *est, int n_est, double lambda_luma, double lambda_chroma);
/* Intra prediction of a list of blocks from a reconstructed picture (all neighbours are read
 * from rec as it is: the caller guarantees the dependency order).  Output in plane geometry of
 * `pred`.  HOT LOOP A shape (ENC/TEncSearch.cpp:2534): d_modes != NULL evaluates modes[0..n_modes) for
 * every block from ONE reference gather and writes candidate k at element offset
 * k * mode_plane_elems[plane] of the pred planes. */
int hmx_batch_predIntra(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_pic *rec, const hmx_pic *pred,
                        const hmx_pic_param *pp, const uint8_t *d_modes, int n_modes,
                        const size_t mode_plane_elems[3]);

/* The mode pre-selection of estIntraPredQT (TLibEncoder/TEncSearch.cpp:2509-2540) without writing the
 * candidates: for every block and every mode of d_modes (NULL: the block's own mode, n_modes = 1) predict
 * from `rec` and cost against `org` with TComRdCost::calcHAD (TLibCommon/TComRdCost.cpp:404-450: Hadamard
 * SATD over 8x8 sub-blocks, 4x4 for 4x4 blocks).  d_satd[(block index in the list's creation order) * n_modes
 * + k] (device).  The 35 predictions stay in registers: 35x less write traffic than hmx_batch_predIntra. */
int hmx_batch_predIntra_cost(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_pic *rec, const hmx_pic *org,
                             const hmx_pic_param *pp, const uint8_t *d_modes, int n_modes, uint32_t *d_satd);
/* The two calls above with the slice / tile / CIP layout of the picture (maps in HOST memory; see hmx_avail_layout).
 * layout = NULL: the calls above, unchanged. */
int hmx_batch_predIntra_layout(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_pic *rec, const hmx_pic *pred,
                               const hmx_pic_param *pp, const hmx_avail_layout *layout, const uint8_t *d_modes, int n_modes,
                               const size_t mode_plane_elems[3]);
int hmx_batch_predIntra_cost_layout(hmx_ctx *ctx, const hmx_tu_list *list, const hmx_pic *rec, const hmx_pic *org,
                                    const hmx_pic_param *pp, const hmx_avail_layout *layout, const uint8_t *d_modes, int n_modes,
                                    uint32_t *d_satd);
/* Whole-picture all-intra reconstruction from decisions: for every block, refs <- recon, predict,
 * residual, T, Q, IQ, IT, recon (ENC/TEncSearch.cpp:1006-1165 with RDOQ off; DEC/TDecCu.cpp:469-687 for
 * the decode direction).  Blocks are given per picture in coding order on the HOST; the library
 * derives the dependency schedule (CTU diagonals x in-CTU levels) and launches one kernel per CTU
 * diagonal over all pictures of the batch. */
typedef struct hmx_intra_plan hmx_intra_plan;
/* The neighbour units (bits as in the availability flags of initAdiPattern: below-left bottom first, left, corner, above,
 * above-right; units of 4 luma / 2 chroma samples) whose reconstruction the prediction of a block of n_samples x n_samples
 * with this mode can depend on, given which units are available: what the mode reads (TComPrediction.cpp:179-290, 689-730),
 * one sample wider where the smoothed reference line is used, and the units the padding of unavailable ones copies from.
 * The dependency order of a plan follows these bits, not the availability flags (a horizontal mode does not wait for the
 * block above-right).  Pure host function (no device work); exported for the test that holds it against the oracle. */
unsigned long long hmx_intra_dependency_mask(int n_samples, int is_luma, int mode, unsigned long long avail);
/* 1 when the units the mode reads with every neighbour available are not all available, that is when
 * hmx_intra_dependency_mask(.., avail) differs from hmx_intra_dependency_mask(.., all 4n+1 bits set): the padding of the reference
 * line then changes a sample the prediction looks at.  0: the padding is the identity on every position the mode reads, and the
 * whole-picture chains skip it (the plans carry this bit per block and sort by it).  An empty availability gives 1, and so does a
 * size or mode the function does not know.  Pure host function. */
int hmx_intra_reads_unavailable(int n_samples, int is_luma, int mode, unsigned long long avail);
/* 1 when hmx_intra_reads_unavailable is 1 and no unavailable unit the mode reads lies strictly between the lowest and the highest
 * unit of hmx_intra_dependency_mask(.., avail), or that mask is empty: the unavailable units read are a leading run, a trailing run
 * or both, and the padded reference line is raw[clamp(p, lo, hi)] at every position the mode reads, lo / hi being the first sample
 * of the mask's lowest unit / the last sample of its highest (an empty mask: the mid value everywhere).  0 when a read unit is
 * missing BETWEEN units of the mask (slices, tiles, constrained intra prediction), when nothing is missing, and for a size or mode
 * the function does not know.  The plans carry this bit per block next to the one above.  Pure host function. */
int hmx_intra_pads_simple(int n_samples, int is_luma, int mode, unsigned long long avail);
/* The availability flags of initAdiPattern for a block at luma position (x, y) of luma size size_luma (a chroma block: its
 * luma-scaled position and size), CTU size 64: bit u in the bNeighborFlags order, units of four luma samples.  closed_form 0:
 * the unit-by-unit rule (TComPattern.cpp:607-786); 1: the closed form the device plan builder uses.  Pure host functions,
 * exported for the test that holds one against the other. */
unsigned long long hmx_intra_avail_mask(int x, int y, int size_luma, int pic_w, int pic_h, int closed_form);
/* The same with the slice / tile / CIP layout of the picture (CTU size 64; maps in HOST memory): a subset of
 * hmx_intra_avail_mask(..., 0).  size_luma = 64: the 64 x 64 prediction unit, in units of EIGHT samples (33 bits).  Returns
 * ~0ull for an invalid layout or block. */
unsigned long long hmx_intra_avail_mask_layout(int x, int y, int size_luma, int pic_w, int pic_h, const hmx_avail_layout *layout);
int hmx_intra_plan_create(hmx_ctx *ctx, const hmx_tu *tus, int n_tu, const hmx_pic_param *pp,
                          hmx_intra_plan **plan);
/* The plans of n_pics pictures (picture i: tus[i][0 .. n_tu[i])): the dependency analysis -- host work, about 43 ms per
 * 2160p picture on one core -- runs on as many host threads as the machine has (at most 32), the uploads follow.
 * Same plans as n_pics calls of hmx_intra_plan_create; on an error no plan is left behind. */
int hmx_intra_plan_create_multi(hmx_ctx *ctx, const hmx_tu *const *tus, const int *n_tu, int n_pics, const hmx_pic_param *pp,
                                hmx_intra_plan **plans);
/* The same plans analysed ON THE DEVICE, for pipelines whose every batch brings new decisions (the host analysis above is
 * ~550x a picture's share of a whole-picture call).  d_tus (DEVICE): the decision lists of n_pics pictures back to back,
 * picture i = d_tus[offsets[i] .. offsets[i+1]) (offsets: HOST array of n_pics + 1 entries), each list in coding order --
 * CTUs in raster order, the blocks of a CTU together, in the order the reference codes them (TEncSearch.cpp:1394-1700).
 * The dependency levels are a wavefront over the CTU diagonals with one lane per (picture, CTU, plane) walking its CTU's
 * blocks; the bucket order is a counting sort.  plans[i] equals what hmx_intra_plan_create builds from the same list,
 * entry for entry; such plans serve the packed schedule (default) and the level schedule, not the CTU-wave schedule.
 * The lists may be freed or overwritten when the call returns.  The plans of one call share their device tables: destroy
 * each with hmx_intra_plan_destroy (the memory is kept for the next call of this context). */
int hmx_intra_plan_create_device(hmx_ctx *ctx, const hmx_tu *d_tus, const uint32_t *offsets, int n_pics, const hmx_pic_param *pp,
                                 hmx_intra_plan **plans);
/* The three plan builders with the slice / tile / CIP layout of each picture (see hmx_avail_layout): a block's dependencies
 * follow the availability with the layout, so a block never waits on another region, and the plans serve every schedule
 * as before.  _layout / _multi_layout: maps in HOST memory (layouts[i] for picture i); _device_layout: layouts is a HOST
 * array whose maps are in DEVICE memory.  layouts = NULL (or a NULL entry): the plans of the calls without a layout. */
int hmx_intra_plan_create_layout(hmx_ctx *ctx, const hmx_tu *tus, int n_tu, const hmx_pic_param *pp, const hmx_avail_layout *layout,
                                 hmx_intra_plan **plan);
int hmx_intra_plan_create_multi_layout(hmx_ctx *ctx, const hmx_tu *const *tus, const int *n_tu, int n_pics, const hmx_pic_param *pp,
                                       const hmx_avail_layout *const *layouts, hmx_intra_plan **plans);
int hmx_intra_plan_create_device_layout(hmx_ctx *ctx, const hmx_tu *d_tus, const uint32_t *offsets, int n_pics, const hmx_pic_param *pp,
                                        const hmx_avail_layout *const *layouts, hmx_intra_plan **plans);
void hmx_intra_plan_destroy(hmx_ctx *ctx, hmx_intra_plan *plan);
/* The plans of a batch at once (waits ONCE for the context's stream: hmx_intra_plan_destroy does so per plan). */
void hmx_intra_plan_destroy_many(hmx_ctx *ctx, hmx_intra_plan *const *plans, int n);
/* The two tables of a plan that the packed and the level schedule run on, copied to the HOST (for tests and tools that hold a
 * device-built plan against a host-built one): blocks[n_blocks] = the blocks sorted by (dependency level, size, code path,
 * coding index), 16 bytes each: the hmx_tu followed by a 64-bit mask over the 4n+1 neighbour units in initAdiPattern's order: the
 * units the block's mode READS among the available ones, closed under the padding rule (hmx_intra_dependency_mask of the availability);
 * levels[n_levels] = per dependency level {uint32 start[4], count[4]} by transform size (4, 8, 16, 32), starts into blocks.
 * Either pointer may be NULL. */
int hmx_intra_plan_download(hmx_ctx *ctx, const hmx_intra_plan *plan, void *blocks, void *levels);
/* The two bits a plan keeps per block beside the mask, which hmx_intra_plan_download leaves out: bits[i] for block i of its sorted
 * list, bit 0 = hmx_intra_reads_unavailable, bit 1 = hmx_intra_pads_simple of the block's availability.  For tests that hold a
 * device-built plan against a host-built one. */
int hmx_intra_plan_pad_bits(hmx_ctx *ctx, const hmx_intra_plan *plan, unsigned char *bits);
/* Size of the dependency schedules of a plan: blocks, picture-wide dependency levels (= launches of
 * the level schedule) and CTU diagonals (= launches of the wave schedule). */
int hmx_intra_plan_info(const hmx_intra_plan *plan, int *n_blocks, int *n_levels, int *n_diagonals);
/* One dependency level of the level schedule: its block counts by transform size (4, 8, 16, 32) and
 * the wavefronts one picture contributes to that level's launch. */
int hmx_intra_plan_level(const hmx_intra_plan *plan, int level, uint32_t counts[4], uint32_t *n_waves);
/* How the LAST whole-picture call was issued: schedule 0 = CTU-diagonal waves (k_intra_wave), 1 = levels,
 * one picture per wave (k_intra_level), 2 = levels across pictures (k_intra_level_across); stream_groups =
 * picture groups whose launches ran concurrently on separate streams (launches per level). */
int hmx_last_call_shape(const hmx_ctx *ctx, int *schedule, int *stream_groups);
/* Optional stage timing of whole-picture calls (HIP events on the context's stream): layout conversion
 * in, dependency chain, layout conversion out, of the LAST call issued after hmx_set_timing(ctx, 1).  After
 * hmx_sao_decide_multi the three values are its candidate kernel, its decision kernel and 0. */
int hmx_set_timing(hmx_ctx *ctx, int enable);
int hmx_last_call_timing(hmx_ctx *ctx, float *to_tiled_ms, float *chain_ms, float *from_tiled_ms);
/* Packed schedule: the part of chain_ms the LAST timed call spent building its schedule tables on the device (0 when it re-used
 * the tables of an earlier call with the same pictures and plans). */
int hmx_last_call_tables_ms(hmx_ctx *ctx, float *ms);
/* Packed schedule: the schedule tables of the LAST whole-picture call copied to the HOST, read-only (for the test that holds
 * them against the plans of the call; nothing is rebuilt or invalidated).  The call waits for the context's stream.  Use it
 * twice: with hdr = rows = descs = items = done = NULL it fills *geom only, so that the caller can allocate; any non-NULL
 * pointer then receives its table.  HMX_ERR_ARG when the last whole-picture call did not run the packed schedule or its
 * tables are not valid (the call failed, or a pool it used was destroyed since).
 *   geom   the shape of the tables: pictures form n_groups groups of I (the last one may be ragged), group g belongs to
 *          shard g mod n_shards; a ROW is (dependency level L, group g), index L * n_groups + g, n_rows = max_levels * n_groups.
 *   hdr    12 x uint32: shard_base[9] (the wave-items of shard s are [shard_base[s], shard_base[s + 1]); entries n_shards .. 8
 *          hold the total), total_items, the abort word (non-zero: a dependency wait of the call timed out), 0.
 *   rows   n_rows x 12 x uint32: wave_base (first wave-item), n_waves, item_base[4] (first item per transform size 4, 8, 16,
 *          32), count[4] (blocks per size), 2 words of padding.  Wave-items and items are numbered in TICKET order: shard after
 *          shard, inside a shard level after level, inside a level the shard's groups in ascending order.
 *   descs  n_waves x 4 x uint32, one per wave-item: item_off (first item), n_items | size class << 28, row, dep_target (the
 *          wave-items of row (L - 1, g) that must have completed before this one starts; 0: nothing to wait for).  A row's
 *          wave-items follow each other from wave_base, sizes 32, 16, 8, 4 in that order, at most slots(size) items each
 *          (slots4, slots8, 4 per 16x16, 1 per 32x32).
 *   items  n_items x 16 bytes: a block as hmx_intra_plan_download gives it (hmx_tu + 64-bit mask), with the picture's index
 *          inside its group in bits 2..7 of `plane`.
 *   done   n_rows x uint32: the completion counter of every row as the call left it (= n_waves once the call has finished). */
typedef struct hmx_pack_geom {
  int n_pics, I, n_groups, n_shards, max_levels, slots4, slots8;
  int n_rows, n_waves, n_items;
} hmx_pack_geom;
int hmx_last_call_pack_tables(hmx_ctx *ctx, hmx_pack_geom *geom, void *hdr, void *rows, void *descs, void *items, uint32_t *done);
/* Which schedule a whole-picture call with n_pics pictures uses: 1 = level, 0 = wave. */
int hmx_intra_schedule_for(const hmx_ctx *ctx, int n_pics);
/* n_pics pictures share one plan (same block structure); org/rec/lev are arrays of n_pics entries. */
int hmx_frame_intra_encode(hmx_ctx *ctx, const hmx_intra_plan *plan, int n_pics, const hmx_pic *org,
                           const hmx_pic *rec, const hmx_levels *lev);
int hmx_frame_intra_decode(hmx_ctx *ctx, const hmx_intra_plan *plan, int n_pics, const hmx_pic *rec,
                           const hmx_levels *lev);
/* The general form: picture i follows plans[i] (every picture its own block structure and modes, as in a
 * real stream); all plans of one call share picture size, QP and slice settings (the QP of a block comes from the map instead
 * while hmx_set_qp_map is in force). */
int hmx_frame_intra_encode_multi(hmx_ctx *ctx, const hmx_intra_plan *const *plans, int n_pics, const hmx_pic *org,
                                 const hmx_pic *rec, const hmx_levels *lev);
/* The same for the intra blocks of an INTER picture: the plan lists only the intra-coded blocks, and they are
 * reconstructed ONTO what `rec` already holds -- the inter-coded blocks (motion compensation + residual) of the same
 * picture, which the decoder has reconstructed before any later coding unit predicts from them
 * (DEC/TDecCu.cpp:384-446 xDecompressCU: xReconInter / xReconIntraQT per coding unit; an intra block only ever reads
 * samples of coding units that precede it, so "all inter blocks first, then the intra blocks in dependency order"
 * gives the same picture).  The reconstruction planes are brought into the working pool first. */
int hmx_frame_intra_decode_onto(hmx_ctx *ctx, const hmx_intra_plan *plan, int n_pics, const hmx_pic *rec,
                                const hmx_levels *lev);
/* Encoder side of the same (ENC/TEncSearch.cpp:1006-1390 for the intra coding units the encoder chose inside an inter
 * picture): prediction from what `rec` holds, residual against `org`, T, flat Q + sign hiding -> levels, IQ, IT,
 * reconstruction of the plan's blocks onto `rec`. */
int hmx_frame_intra_encode_onto(hmx_ctx *ctx, const hmx_intra_plan *plan, int n_pics, const hmx_pic *org, const hmx_pic *rec,
                                const hmx_levels *lev);
int hmx_frame_intra_decode_multi(hmx_ctx *ctx, const hmx_intra_plan *const *plans, int n_pics, const hmx_pic *rec,
                                 const hmx_levels *lev);

/* RDOQ as the quantiser of the whole-picture encode calls (the encoder's default: TEncSearch::xIntraCodingLumaBlk /
 * ChromaBlk call transformNxN, which runs xRateDistOptQuant when m_useRDOQ, TComTrQuant.cpp:1395-1404).  What the
 * encoder takes from its live state is an input, per picture: the bit estimates m_pcEstBitsSbac as estBit leaves them
 * for [luma, chroma] x [4x4, 8x8, 16x16, 32x32] (TEncSbac.cpp:1507-1667), and m_dLambda for luma and chroma blocks
 * (setLambda per component, TEncSlice.cpp:380-395).  The context of a block's coded-block flag travels in
 * hmx_tu::flags, bits 4..7 (= getCtxQtCbf: the transform depth for luma, + NUM_QT_CBF_CTX for chroma).
 * n_pics = the pictures of the following calls, or 1 = one set for every picture.  pics = NULL turns RDOQ off again.
 * Transform-skip blocks keep the flat quantiser (TComTrQuant.cpp:1121-1122 with TransformSkipFast, which every shipped
 * cfg that enables transform skip sets); packed schedule only, packing groups of at most 2 pictures (HMX_PACK_GROUP; the
 * tables of a group wait in LDS).  Levels travel as 16-bit words inside the kernel: a call whose QP, bit depth and block sizes allow
 * |level| = (32768 * quantScale) >> qbits > 32767 (e.g. 10-bit, QP < 5 with 32x32 blocks) is refused with HMX_ERR_ARG -- luma
 * blocks judged by the luma QP, chroma blocks by the chroma QP, each by the sizes the plans hold of it. */
typedef struct hmx_rdoq_pic {
  hmx_est_bits est[8]; /* [luma, chroma][log2(size) - 2] */
  double lambda_luma, lambda_chroma;
} hmx_rdoq_pic;
int hmx_set_rdoq(hmx_ctx *ctx, const hmx_rdoq_pic *pics, int n_pics);
/* Distortion next to the chain: the encoder calls TComRdCost::getDistPart(rec, org, DF_SSE) right after every
 * reconstruction (TLibEncoder/TEncSearch.cpp:1163, :1381).  After hmx_set_sse_output(ctx, sse, n) the whole-picture
 * ENCODE calls (any of the hmx_frame_intra_encode* entry points, packed schedule) with at most n pictures also write,
 * for picture i and plane p, xGetSSE(org, rec) of every block -- sum of (org - rec)^2 >> 2 * (B - 8),
 * TLibCommon/TComRdCost.cpp:1313-1657 -- into sse[i].plane[p][u], u = the block's first 4x4 unit in the reference's
 * partition order (CTU blocks in raster order over the CTU-padded plane, Z-order inside a CTU: 1/16 of the block's
 * offset in the stride-0 level layout).  Device arrays of (CTU-padded plane samples / 16) entries; sse == NULL
 * switches the output off.  The sums are formed in the kernel that reconstructs the block. */
typedef struct {
  uint32_t *plane[3];
} hmx_sse;
int hmx_set_sse_output(hmx_ctx *ctx, const hmx_sse *sse, int n_pics);
/* A QP per block (cu_qp_delta: adaptive QP, rate control, MaxDeltaQP > 0).  In the reference the QP of a transform block is its
 * coding unit's, TComDataCU::getQP, applied through TComTrQuant::setQPforQuant; the chroma QP comes from it through
 * g_aucChromaScale and the PPS offset; the encoder sets it per coding unit in TEncCu::xCompressCU / xComputeQP (TEncCu.cpp:1114-1136).
 * hmx_set_qp_map sticks until it is changed, like hmx_set_rdoq and hmx_set_sse_output.  d_qp: DEVICE memory, [n_pics][uh][uw] with
 * uw = ceil(pic_w / 4), uh = ceil(pic_h / 4): one luma QP per 4x4 luma unit in raster order, contiguous per picture -- the layout
 * hmx_deblock_picture_multi reads as d_qp, so a caller keeps ONE map per picture for the transforms and for deblocking.  Values are
 * getQP's, -QpBDOffsetY .. 51.  n_pics == 1: one map for every picture of the following calls; otherwise picture i reads map i and a
 * call with more pictures than maps is HMX_ERR_ARG.  d_qp == NULL switches back to hmx_pic_param.qp, and every call behaves exactly
 * as without this entry.  The memory stays the caller's and must stay valid until the calls that use it have completed.
 *   A transform block takes the QP of the unit at its first sample (a chroma block at (x, y): the unit at luma (2x, 2y));
 * hmx_pic_param.qp is then not used for quantisation; chroma_qp_offset (-12..12), slice_type (rounding 171 / 85) and sign_hide keep
 * their meaning.  The host cannot see the bytes: the kernels clamp what they read to -QpBDOffsetY .. 51 before it indexes their
 * table (built per call on the host, entry [QP + QpBDOffset][luma, chroma], the chroma entry through hmx_setQPforQuant), and the
 * unit to the map.  A bad byte gives a meaningless block, never an access outside a table.
 *   Honoured by: the whole-picture chain on the PACKED schedule -- hmx_frame_intra_encode / _decode, _multi, _onto, _resident, with
 * hmx_set_sse_output beside them -- and the block-list transform entries hmx_batch_transformNxN,
 * hmx_batch_residual_transformNxN[_multi], hmx_batch_residual_transform_recon[_sse]_multi and hmx_batch_invtransformNxN[_multi]
 * (picture i of a _multi call reads map i).  With a map set a whole-picture call that resolves to the level or the wave schedule is
 * HMX_ERR_ARG, and so is one with RDOQ set (lambda and the bit estimates are per picture there, and the reference changes lambda
 * with the QP); both before anything is launched, hmx_last_error says which.  The map kernel has one wave-item shape per size class
 * (64 4x4 blocks, eight 8x8 blocks): HMX_PACK_SLOTS4 / HMX_PACK_SLOTS8 do not apply to it.
 *   NOT covered: hmx_batch_xRateDistOptQuant and the scalar drop-ins (they take their QP per call), RDOQ with a map, the level and
 * wave schedules, and the deblocking QP of coding units without a coded residual in real streams (they carry the PREDICTED QP,
 * which only a parser knows). */
int hmx_set_qp_map(hmx_ctx *ctx, const int8_t *d_qp, int n_pics);
/* The reference ENCODER's flat quantiser (xQuant, built with ADAPTIVE_QP_SELECTION) takes its scale from the block's QP but its right
 * shift iQBits from the SLICE's base QP (TComTrQuant.cpp:1161-1231: cQpBase from getSliceQpBase(); chroma: the base through
 * g_aucChromaScale without the PPS offset, :1175-1190); dequantisation uses the block's QP alone.  With one QP per call the two are
 * the same number.  With a map they are not: hmx_set_qp_map_base(ctx, 1, slice_qp_base) makes the forward quantiser of the calls that
 * honour the map shift by the base QP's period, which reproduces the levels the reference encoder writes under --AdaptiveQP=1;
 * (ctx, 0, 0), the default, shifts by the block's own QP (per of the block's QP: what a quantiser that follows the block QP alone
 * does).  The decoder direction is not affected.  slice_qp_base: -QpBDOffsetY .. 51, else HMX_ERR_ARG.  Sticks like hmx_set_qp_map. */
int hmx_set_qp_map_base(hmx_ctx *ctx, int on, int slice_qp_base);

/* Pictures RESIDENT in the library's working layout: CTU blocks in raster order, 4x4 tiles in
 * Z-order inside a CTU, groups of up to 64 pictures interleaved 8x8 quad by quad.  The whole-picture entry points above
 * take pictures in the reference's plane geometry (TComPicYuv) and convert them into and out of this layout around
 * every call; an application that keeps its pictures here pays that once, or never: hmx_yuv_unpack_resident writes a
 * file's frame straight into a pool picture, hmx_yuv_pack_resident reads one back, hmx_tpool_import / _export convert
 * from / to planes (e.g. a reconstruction that motion compensation needs with the reference's margins).
 * A pool holds n_pics pictures of one size; picture indices are positions in the pool. */
typedef struct hmx_tpool hmx_tpool;
int hmx_tpool_create(hmx_ctx *ctx, int pic_w, int pic_h, int n_pics, hmx_tpool **pool);
void hmx_tpool_destroy(hmx_ctx *ctx, hmx_tpool *pool);
int hmx_tpool_import(hmx_ctx *ctx, hmx_tpool *pool, int first, int n, const hmx_pic *src);       /* planes -> pictures first..first+n-1 */
int hmx_tpool_export(hmx_ctx *ctx, const hmx_tpool *pool, int first, int n, const hmx_pic *dst); /* and back */
/* TVideoIOYuv::read / write (TLibVideoIO/TVideoIOYuv.cpp:226-480) on a pool picture; arguments as hmx_yuv_unpack /
 * hmx_yuv_pack with the picture size taken from the pool (w_full x h_full = the pool's picture size). */
int hmx_yuv_unpack_resident(hmx_ctx *ctx, const void *d_file, int file_bits, hmx_tpool *pool, int index, int pad_x, int pad_y);
int hmx_yuv_pack_resident(hmx_ctx *ctx, const hmx_tpool *pool, int index, int crop_right, int crop_bottom, int file_bits, void *d_file);
/* hmx_frame_intra_encode_multi / _decode_multi on pictures 0..n_pics-1 of resident pools: no layout conversion inside the
 * call.  plan_stride 1: picture i follows plans[i]; 0: every picture follows plans[0].  org and rec must be pools of the
 * plans' picture size and of EQUAL picture count (the count fixes how many pictures form a group of the layout). */
int hmx_frame_intra_encode_resident(hmx_ctx *ctx, const hmx_intra_plan *const *plans, int plan_stride, int n_pics,
                                    const hmx_tpool *org, hmx_tpool *rec, const hmx_levels *lev);
int hmx_frame_intra_decode_resident(hmx_ctx *ctx, const hmx_intra_plan *const *plans, int plan_stride, int n_pics,
                                    hmx_tpool *rec, const hmx_levels *lev);

/* TComPrediction::motionCompensation for one prediction unit (TComPrediction.cpp:410-552 -> xPredInterUni / xPredInterBi
 * -> the two functions above -> TComYuv::addAvg), the call TEncCu.cpp:1299 and TDecCu.cpp:452 make per coding unit.
 * ref0 / ref1: the reference pictures of list 0 / 1 as HOST planes (plane[i] at sample (0,0), margins readable), NULL =
 * list unused; mv0 / mv1: {hor, ver} in quarter-pel, clipped (hmx_clipMv); (x, y, w, h): the unit in luma samples;
 * dst: HOST planes, plane[i] at the unit's first sample of that plane (a TComYuv part address). */
int hmx_motionCompensation(hmx_ctx *ctx, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x, int y,
                           int w, int h, const hmx_pic *dst);

/* Explicit weighted prediction (TLibCommon/TComWeightPrediction.{h,cpp}), the branch TComPrediction::motionCompensation takes when
 * the PPS has getUseWP() (P slices) or getWPBiPred() (B slices), TComPrediction.cpp:421-432 and :516-535.  Every used list is
 * predicted into the 14-bit intermediate (xPredInterUni(..., bi = true)); a unit with one list ends in weightUnidir, a unit with both
 * lists in weightBidir (TComWeightPrediction.h:82-89) -- always, the identical-motion shortcut being off under WPBiPred (:394).
 * Supported ranges (anything else is HMX_ERR_ARG, checked on the host before a launch): weight -128..255, offset -128..127,
 * log2_denom 0..7. */
typedef struct {            /* wpScalingParam of one (list, reference) (TLibCommon/TComSlice.h), per component Y, Cb, Cr */
  int16_t weight[3];        /* iWeight */
  int16_t offset[3];        /* iOffset, 8-bit units */
  uint8_t log2_denom[3];    /* uiLog2WeightDenom */
  uint8_t reserved;
} hmx_wp;
/* TComWeightPrediction::addWeightUni (TComWeightPrediction.cpp:161-237) for one component: src = 14-bit intermediates (host),
 * dst = Clip(((weight * (src + 8192) + round) >> (log2_denom + 14 - B)) + offset * 2^(B-8)); the derived fields are getWpScaling's
 * uni-directional branch (:302-312). */
int hmx_addWeightUni(hmx_ctx *ctx, const hmx_pel *src, int src_stride, hmx_pel *dst, int dst_stride, int w, int h, int weight,
                     int offset, int log2_denom);
/* TComWeightPrediction::addWeightBi (TComWeightPrediction.cpp:61-150, bRound = true) for one component, with getWpScaling's
 * bi-directional branch (:286-301): shift = log2_denom + 1 + 14 - B (list 0's denominator serves both lists), the offsets summed. */
int hmx_addWeightBi(hmx_ctx *ctx, const hmx_pel *src0, int s0_stride, const hmx_pel *src1, int s1_stride, hmx_pel *dst,
                    int dst_stride, int w, int h, int weight0, int weight1, int offset0, int offset1, int log2_denom);
/* hmx_motionCompensation with the weighting of TComPrediction.cpp:421-432 / :516-535 -> xWeightedPredictionUni / xWeightedPredictionBi
 * (TComWeightPrediction.cpp:327-386).  wp0 / wp1: the entries of the two references used (NULL where the list is unused). */
int hmx_motionCompensation_wp(hmx_ctx *ctx, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x, int y,
                              int w, int h, const hmx_pic *dst, const hmx_wp *wp0, const hmx_wp *wp1);

/* Motion compensation of a list of PUs against reference pictures resident in HBM with the
 * reference's margin layout (TLibCommon/TComPicYuv.cpp:82-94): motionCompensation -> xPredInterUni/Bi ->
 * xPredInterLumaBlk/ChromaBlk -> addAvg (TLibCommon/TComPrediction.cpp:410-642). MVs already clipped. */
typedef struct {
  uint16_t x, y;       /* luma position */
  uint8_t w, h;        /* luma size */
  uint8_t ref0, ref1;  /* index into refs[], 255 = list unused */
  int16_t mv0x, mv0y, mv1x, mv1y; /* quarter-pel */
} hmx_pu;
int hmx_batch_motionCompensation(hmx_ctx *ctx, const hmx_pu *d_pus, int n, const hmx_pic *refs, int n_refs,
                                 const hmx_pic *dst);
/* The encoder's sub-pel refinement fan-out (HOT LOOP C): TEncSearch::xPatternSearchFracDIF (TLibEncoder/TEncSearch.cpp:
 * 4480-4514) builds the half- and quarter-sample planes around a unit's integer vector (xExtDIFUpSamplingH / Q, :5982-6165:
 * 2 + 4, then 2 + 8 interpolation calls) and costs nine candidates per stage (xPatternRefinement :711-760) with
 * TComRdCost::xGetHADs (UseHADME, TComRdCost.cpp:2186-2283) or xGetSAD (:488-516).  Here: for every unit i of `pus` (HOST
 * array; ref0 and mv0 = the INTEGER vector in quarter samples, a multiple of 4) and every candidate k the distortion between
 * the original block and the two-stage prediction (filterHorLuma isLast = false, then filterVerLuma isFirst = false, isLast =
 * true -- what the reference's m_filteredBlock planes hold, zero fractions included) at mv0 + offs[k] quarter samples
 * (offs: host array of n_cand {dx, dy} pairs, |dx|, |dy| <= 3; n_cand <= 49: both stages of the reference's search, or the
 * whole 7 x 7 neighbourhood at once): d_cost[i * n_cand + k] (device) = sum over the unit's 8x8 (4x4 when a side is not a
 * multiple of 8) sub-blocks of the Hadamard sum (use_had) or the SAD, >> (bit depth - 8).  The vector-bits term of
 * xPatternRefinement (TComRdCost::getCost(x, y)) and the choice among candidates stay with the caller.
 * refs / org: device pictures; the references with the reference's margins.
 * LIST LENGTH (this entry and the seven others that say "longest list" below).  The host tables of a call travel through the
 * context's argument arena, 8 MiB = 8388608 bytes, each table rounded up to 256 bytes: R(b) = (b + 255) & ~255.  One call takes
 * the lists whose rounded tables fit the arena TOGETHER; a longer list is refused with HMX_ERR_NOMEM ("... list too long: split
 * the call" in hmx_last_error) on the host, before anything is copied, set or launched: the outputs are untouched, the context
 * goes on working, and the caller splits the list.  Lists up to the limit are served from any state of the context.
 * Longest list here: R(16 n) + R(4 (n + 1)) + R(2 n_cand) <= 8388608 -- sizeof(hmx_pu) = 16, a prefix entry per unit, the
 * offsets: n <= 419408. */
int hmx_batch_subpel_cost(hmx_ctx *ctx, const hmx_pu *pus, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                          const int8_t *offs, int n_cand, int use_had, uint32_t *d_cost);
/* The same under weighted distortion (see "Weighted distortion in the motion search" below): unit i is weighted with
 * wp[pus[i].ref0]; wp == NULL is hmx_batch_subpel_cost.  Longest list: as hmx_batch_subpel_cost, n <= 419408. */
int hmx_batch_subpel_cost_wp(hmx_ctx *ctx, const hmx_pu *pus, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                             const int8_t *offs, int n_cand, int use_had, uint32_t *d_cost, const hmx_wp *wp);

/* ------------------------------------------------------------------------------------------------
 * Full-search integer motion estimation: the stage of TEncSearch::xMotionEstimation (TLibEncoder/TEncSearch.cpp:4120-4206)
 * in front of the sub-pel fan-out above.  All arithmetic is uint32_t, wrapping like the reference's UInt.
 * ---------------------------------------------------------------------------------------------- */
/* Host helpers, no context.  TComRdCost::getBits(x, y) (TComRdCost.h:201-211) with xGetComponentBits (TComRdCost.cpp:270-284)
 * in closed form: bits(v) = 2 * floor(log2 t) + 1, t = v <= 0 ? ((-v) << 1) + 1 : v << 1; hmx_mvBits = bits((x << cost_scale)
 * - pred_x) + bits((y << cost_scale) - pred_y), the predictor (setPredictor) in quarter samples. */
uint32_t hmx_mvBits(int x, int y, int pred_x, int pred_y, int cost_scale);
/* TComRdCost::getCost(x, y) (TComRdCost.h:185-193): (lambda * hmx_mvBits(...)) >> 16; lambda = m_uiLambdaMotionSAD =
 * floor(65536 * sqrt(lambda)) (getMotionCost(1, 0), :171).  The integer search runs at cost_scale 2 (TEncSearch.cpp:4172). */
uint32_t hmx_mvCost(uint32_t lambda, int x, int y, int pred_x, int pred_y, int cost_scale);
/* TEncSearch::xSetSearchRange (TEncSearch.cpp:4209-4225) for the unit's CU at (cu_x, cu_y): the predictor (quarter samples)
 * clipped with hmx_clipMv, -/+ (range << 2), both corners clipped with hmx_clipMv, arithmetic >> 2: the inclusive box in
 * integer samples. */
void hmx_setSearchRange(int pred_x, int pred_y, int range, int cu_x, int cu_y, int pic_w, int pic_h, int ctu_size, int *left,
                        int *top, int *right, int *bottom);
typedef struct {
  uint16_t x, y;          /* unit position, luma samples */
  uint8_t  w, h;          /* {4,8,12,16,24,32,48,64} */
  uint8_t  ref;           /* index into refs[] */
  uint8_t  sub_shift;     /* 0 | 1 */
  int16_t  pred_x, pred_y;            /* predictor of the bits term, quarter samples */
  int16_t  left, top, right, bottom;  /* search box, integer samples, inclusive */
} hmx_me_unit;             /* 20 bytes */
typedef struct { int16_t mvx, mvy; uint32_t sad; uint32_t cost; } hmx_me_result; /* 12 bytes */
/* TEncSearch::xPatternSearch (TEncSearch.cpp:4227-4283) for every unit of `units` (HOST array): for y = top..bottom and, inside
 * that, x = left..right, cost = SAD(original block at the unit, reference block displaced by (x, y)) + hmx_mvCost(lambda, x,
 * y, pred_x, pred_y, 2), SAD as hmx_getSAD with the unit's sub_shift; the winner is the first candidate in that raster order
 * with the strictly smallest cost.  d_result[i] (device) = {mv, sad = cost - vector cost (ruiSAD), cost}.  d_cost_map (device,
 * may be NULL) receives the cost of every candidate: unit i's box row by row, box width right - left + 1, starting at the sum
 * of the box areas of units 0..i-1.  refs (n_refs <= 4) / org: device pictures, the references with margins of margin_x /
 * margin_y luma samples and samples in [0, 2^B); org may hold any value in [-2^B, 2^(B+1)) -- bi-prediction refinement
 * searches against 2 * org - other prediction (removeHighFreq, :4147), which the caller passes as org.  Weighted SAD
 * (xGetSADw) is hmx_batch_fullpel_search_wp, xTZSearch is hmx_batch_tz_search, both below; chroma is not covered.
 * n >= 1 and the boxes together hold fewer than 2^32 candidates; anything else is HMX_ERR_ARG.
 * Longest list (see LIST LENGTH at hmx_batch_subpel_cost): R(20 n) + 2 R(4 (n + 1)) <= 8388608 -- sizeof(hmx_me_unit) = 20 and
 * two prefix tables: n <= 299583; a longer one is HMX_ERR_NOMEM before anything is launched.
 * HMX_ERR_ARG, on the host before anything is launched, with the unit named in hmx_last_error: a size outside the set, ref >=
 * n_refs, sub_shift other than 0 or (1 with h > 8), an empty box, a box side above 129 (search range 64), the unit outside the
 * picture, a candidate block reaching outside [-margin, pic + margin) of the reference in either direction. */
int hmx_batch_fullpel_search(hmx_ctx *ctx, const hmx_me_unit *units, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                             int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result,
                             uint32_t *d_cost_map);
/* TEncSearch::xTZSearch (TEncSearch.cpp:4302-4474, through xPatternSearchFast, :4285-4300) for every unit of `units`, as the
 * reference compiles it: TZ_SEARCH_CONFIGURATION (:293-309) with FASTME_SMOOTHER_MV 1.  The walk of one unit:
 *   1. the start point tz[i].start (rcMv after clipMv and >>= 2, :4312-4313: the caller makes it with hmx_clipMv), then the zero
 *      vector (bTestZeroVector), which may lie outside the box;
 *   2. first search: xTZ8PointDiamondSearch (:536-707) around the better of the two with iDist = 1, 2, 4 ... <= tz[i].range,
 *      left as soon as uiBestRound >= 3;
 *   3. xTZ2PointSearch (:351-479) when uiBestDistance == 1;
 *   4. when uiBestDistance > 5: every fifth candidate of the box, rows from top, columns from left (raster search);
 *   5. star refinement while uiBestDistance > 0: the diamonds iDist = 1, 2, 4 ... <= range around the best point with no early
 *      exit, then the 2-point search when uiBestDistance == 1 (and ucPointNr != 0), one PASS each.
 * Every evaluation is xTZSearchHelp (:312-349): cost = SAD + hmx_mvCost(lambda, x, y, pred_x, pred_y, 2), SAD as hmx_getSAD
 * with the unit's sub_shift (FEN: 1 for more than 8 rows), all uint32_t; a candidate replaces the best on a strictly smaller
 * cost only, and then sets uiBestDistance, ucPointNr and uiBestRound = 0.  A pattern point is evaluated when each coordinate
 * that moves away from the pattern's centre stays on the box's side it moves towards: nothing else is tested, so a walk that
 * adopts a zero vector outside the box evaluates points outside the box, all of them inside the bounding rectangle of
 * box U {(0, 0)}.  The other predicted vectors, the zero-vector restart and the raster refinement are compiled off in the
 * reference and absent here; weighted SAD is hmx_batch_tz_search_wp below; chroma is not covered.
 * units: the HOST array hmx_batch_fullpel_search takes (pred_x / pred_y: the unclipped setPredictor values); tz: HOST array
 * parallel to it; range is uiSearchRange = m_iSearchRange (m_aaiAdaptSR: per reference picture, hence per unit).
 * d_result[i] (device) = {iBestX, iBestY, sad = uiBestSad - vector cost (ruiSAD, :4473), cost = uiBestSad}: d_int of
 * hmx_batch_subpel_search.  d_trace / d_trace_count (device, both or neither NULL): d_trace_count[i] = the number of
 * evaluations of unit i, all of them; d_trace[i * trace_cap + k] = the k-th evaluated point and its cost, in the reference's
 * order, for k < min(count, trace_cap); nothing is written beyond.
 * The star refinement ends because every pass that continues has lowered a uint32_t cost.  The kernel still counts passes
 * against a cap: HMX_TZ_MAX_PASSES (hmx_set_option, 1 .. 1024, default 1024).  A unit that asks for another pass after `cap`
 * passes gets {best so far, sad = cost = 0xFFFFFFFF}; its evaluations stay in its trace; other units are unaffected.
 * HMX_ERR_ARG, on the host before anything is launched, with the unit named in hmx_last_error: what hmx_batch_fullpel_search
 * refuses for a unit (size, ref, sub_shift, empty box, side above 129, unit outside the picture); a NULL pointer other than the
 * two trace pointers, exactly one of those NULL, trace_cap < 1 with a trace, n < 1, n_refs outside 1..4, range outside 1..64,
 * reserved != 0, a start point outside the box, and the bounding rectangle of box U {(0, 0)} grown by the block reaching outside
 * [-margin, pic + margin) of the reference in either direction.
 * Longest list (see LIST LENGTH at hmx_batch_subpel_cost): R(20 n) + R(8 n) <= 8388608 -- sizeof(hmx_me_unit) = 20,
 * sizeof(hmx_tz_unit) = 8: n <= 299584; a longer one is HMX_ERR_NOMEM before anything is launched. */
typedef struct { int16_t start_x, start_y; uint16_t range; uint16_t reserved; } hmx_tz_unit; /* 8 bytes */
typedef struct { int16_t x, y; uint32_t cost; } hmx_tz_point; /* 8 bytes */
int hmx_batch_tz_search(hmx_ctx *ctx, const hmx_me_unit *units, const hmx_tz_unit *tz, int n, const hmx_pic *refs, int n_refs,
                        const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda,
                        hmx_me_result *d_result, hmx_tz_point *d_trace, uint32_t *d_trace_count, int trace_cap);
/* TEncSearch::xPatternSearchFracDIF (TEncSearch.cpp:4476-4514) for every unit of `units`, both stages and both decisions of
 * xPatternRefinement (:711-760) in one launch, from the integer winners where hmx_batch_fullpel_search left them.
 * units: the HOST array given to the integer search (position, size, ref, predictor, box; sub_shift is ignored: setDistParam
 * sets iSubShift = 0 for the refinement, TComRdCost.cpp:380).  d_int (DEVICE): d_int[i].mvx / mvy = the integer vector (ix, iy)
 * of unit i, the only fields read; normally the search's own d_result.  lambda: m_uiLambdaMotionSAD, as for the integer stage.
 * D(mv) = the distortion hmx_batch_subpel_cost documents (two-stage prediction, Hadamard sum (use_had = 1) or SAD (0) over
 * 8x8 / 4x4 sub-blocks, >> (bit depth - 8)).  All arithmetic uint32_t.  Nine candidates per stage in table order:
 *   half    (s_acMvRefineH, :47-58)  k = (0,0) (0,-1) (0,1) (-1,0) (1,0) (-1,-1) (1,-1) (-1,1) (1,1)
 *           cost = D(4ix + 2dx, 4iy + 2dy) + hmx_mvCost(lambda, 2ix + dx, 2iy + dy, pred, 1); winner (hx, hy)
 *   quarter (s_acMvRefineQ, :60-71)  k = (0,0) (0,-1) (0,1) (-1,-1) (1,-1) (-1,0) (1,0) (-1,1) (1,1), base = (4ix + 2hx, 4iy + 2hy)
 *           cost = D(base + q) + hmx_mvCost(lambda, base.x + qx, base.y + qy, pred, 0)
 * The winner of a stage is the first candidate in table order with the strictly smallest cost (uiDistBest = MAX_UINT).
 * d_result[i] (device) = {the winning quarter-sample vector, dist = cost - hmx_mvCost(lambda, mvx, mvy, pred, 0), cost = the
 * winning quarter-stage cost}.  d_stage_cost (device, may be NULL): [i * 18 + k] = half-stage cost k, [i * 18 + 9 + k] =
 * quarter-stage cost k.  The tail of xMotionEstimation (:4197-4205: getBits, the fWeight floor) stays with the caller.
 * refs / org as for hmx_batch_fullpel_search (org may be 2 * org - other prediction).  Weighted distortion (bApplyWeight) is
 * hmx_batch_subpel_search_wp below.  Not covered: the non-square Hadamard shapes of NS_HAD with UseNSQT, and chroma.
 * The 18 candidates read the (w + 8) x (h + 8) window from 4 samples left of and above the displaced block.  The integer
 * vectors are device data the host cannot see, so the host checks the box: a unit whose integer vector lies OUTSIDE its own
 * box is not refined and reads no reference sample: its result is {4 * ix, 4 * iy truncated to int16_t, dist = cost =
 * 0xFFFFFFFF} and its 18 stage costs are 0xFFFFFFFF; the other units of the call are unaffected.
 * HMX_ERR_ARG, on the host before anything is launched, with the unit named in hmx_last_error: a NULL pointer other than
 * d_stage_cost, n < 1, n_refs outside 1..4, use_had other than 0 or 1, a size outside the set, ref >= n_refs, an empty box, the
 * unit outside the picture, the box grown by the window (columns x + left - 4 .. x + right + w + 3, rows likewise) reaching
 * outside [-margin, pic + margin) in either direction.
 * Longest list: the unit list is the call's only table, R(20 n) <= 8388608: n <= 419430; a longer one is HMX_ERR_NOMEM before
 * anything is launched. */
typedef struct { int16_t mvx, mvy; uint32_t dist; uint32_t cost; } hmx_subpel_result; /* quarter samples; 12 bytes */
int hmx_batch_subpel_search(hmx_ctx *ctx, const hmx_me_unit *units, int n, const hmx_me_result *d_int, const hmx_pic *refs,
                            int n_refs, const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda,
                            int use_had, hmx_subpel_result *d_result, uint32_t *d_stage_cost);
/* Weighted distortion in the motion search.  In a slice whose PPS has getUseWP() (P) or getWPBiPred() (B),
 * TEncSearch::setWpScalingDistParam (TEncSearch.cpp:6183-6215) sets DistParam::bApplyWeight and wpCur before the integer stage
 * (:4174), and every distortion of xMotionEstimation is then the weighted one: xGetSAD* return xGetSADw (TComRdCost.cpp:492 ...),
 * xGetHADs returns xGetHADsw (:2188) -- TComRdCostWeightPrediction.cpp:69-104, :196-561, as hmx_getSADw / hmx_getHADsw state them.
 * The _wp entries are the four entries above with one more argument:
 *   wp: HOST array parallel to refs[], n_refs entries; wp[k] is the wpScalingParam row of the (list, reference) refs[k] stands for,
 *   of which only component 0 is read.  Unit i is weighted with wp[units[i].ref].  A picture searched under two different
 *   rows (twice in a list, or in both lists of a B slice) is passed twice in refs[].  Only one index is >= 0 in
 *   setWpScalingDistParam, also for bBi calls, so getWpScaling's uni-directional branch (TComWeightPrediction.cpp:302-312) applies.
 * wp == NULL is the unweighted call: the entries without _wp are exactly that.  With a table EVERY unit is weighted, default rows
 * (weight 1 << log2_denom, offset 0) included, as bApplyWeight is per slice.  What changes against the unweighted entry:
 *   integer stages (full search, TZ): SAD = hmx_getSADw.  units[i].sub_shift is validated as in the unweighted call and has NO
 *   effect: xGetSADw ignores the iSubShift that xTZSearchHelp / xPatternSearch set under FEN, reads every row and does not shift;
 *   sub-pel stages and hmx_batch_subpel_cost_wp: the difference is org - pred, pred formed from the final, clipped interpolated
 *   sample; sub-block rule, per-sub-block rounding and >> (B - 8) as unweighted.
 * Vector costs, tie rules, the TZ walk, ruiSAD = best - vector cost and the results' layout do not change.  All sums are uint32_t.
 * HMX_ERR_ARG, on the host before anything is launched, with the entry and the row named in hmx_last_error: everything the
 * unweighted entry refuses, and a row with weight[0] outside -128..255, offset[0] outside -128..127, log2_denom[0] above 7 or
 * reserved != 0.  Not covered: xGetSSEw, chroma, NS_HAD shapes.  The rows themselves: hmx_wp_estimate_slices below.
 * Longest list: that of the unweighted entry (the table of rows travels as a kernel argument): n <= 299583 for
 * hmx_batch_fullpel_search_wp, 299584 for hmx_batch_tz_search_wp, 419430 for hmx_batch_subpel_search_wp; a longer one is
 * HMX_ERR_NOMEM before anything is launched. */
int hmx_batch_fullpel_search_wp(hmx_ctx *ctx, const hmx_me_unit *units, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                                int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result,
                                uint32_t *d_cost_map, const hmx_wp *wp);
int hmx_batch_tz_search_wp(hmx_ctx *ctx, const hmx_me_unit *units, const hmx_tz_unit *tz, int n, const hmx_pic *refs, int n_refs,
                           const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda,
                           hmx_me_result *d_result, hmx_tz_point *d_trace, uint32_t *d_trace_count, int trace_cap, const hmx_wp *wp);
int hmx_batch_subpel_search_wp(hmx_ctx *ctx, const hmx_me_unit *units, int n, const hmx_me_result *d_int, const hmx_pic *refs,
                               int n_refs, const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda,
                               int use_had, hmx_subpel_result *d_result, uint32_t *d_stage_cost, const hmx_wp *wp);

/* ------------------------------------------------------------------------------------------------
 * The encoder's estimation of the rows: WeightPredAnalysis (TLibEncoder/WeightPredAnalysis.cpp), which TEncSlice::compressSlice
 * runs per slice (TEncSlice.cpp:688-711) when the PPS has getUseWP() or getWPBiPred(), as this reference is built
 * (WP_PARAM_RANGE_LIMIT 1).  The reductions over whole pictures are device entries; the arithmetic per (list, reference,
 * component) is host code without a context, because every consumer above takes its hmx_wp tables as host arrays.  B = the
 * context's bit depth; chroma planes are (pic_w >> 1) x (pic_h >> 1).  Picture sizes: any positive even pic_w, pic_h up to 65536.
 * ---------------------------------------------------------------------------------------------- */
/* xCalcACDCParamSlice (WeightPredAnalysis.cpp:71-108 -> xCalcDCValue :451-464, xCalcACValue :474-487) for n_pics (1..65535)
 * ORIGINAL pictures in one launch per pass: per component dc = (sum of x + (n >> 1)) / n and ac = sum of |x - dc|, n = samples of
 * the plane.  The reference computes them for every picture of a sequence with either PPS flag set, intra pictures included
 * (TEncSlice.cpp:689-692).  pics: host array [n_pics] of descriptors of device planes (each picture its own planes and strides;
 * margins and unaligned planes allowed); d_out (device): [n_pics].  The DC of the second pass is formed on the device from the
 * first pass's sums: nothing returns to the host in between.  Samples lie in [0, 2^15).
 * HMX_ERR_ARG, before anything is launched: a null pointer, a null plane, n_pics out of range, an odd or non-positive size. */
typedef struct hmx_wp_acdc_param {
  int64_t ac[3], dc[3]; /* wpACDCParam::iAC, iDC (TLibCommon/TComSlice.h) of Y, Cb, Cr */
} hmx_wp_acdc_param;
int hmx_wp_acdc_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *pics, int pic_w, int pic_h, hmx_wp_acdc_param *d_out);
int hmx_wp_acdc(hmx_ctx *ctx, const hmx_pic *pic, int pic_w, int pic_h, hmx_wp_acdc_param *d_out); /* = _multi with n_pics = 1 */
/* xCalcSADvalueWP (WeightPredAnalysis.cpp:501-517) as xSelectWP calls it (:333-350), for n_jobs (1..65535) pairs of an original
 * and a reference picture's RECONSTRUCTION in one launch.  Job j reads org[jobs[j].org] and rec[jobs[j].rec] ONCE and gives, per
 * component c with (w, o, d) = the job's row and rd = d + B - 8,
 *   d_out[(j * 3 + c) * 2 + 0] = sum of |(org << d) - (rec * w + (o << rd))|      (the row)
 *   d_out[(j * 3 + c) * 2 + 1] = sum of |(org << d) - (rec << d)|                 (the default row of the same denominator)
 * in Int64, BEFORE the division by the sample count of :516 (hmx_wp_select divides).  org / rec: host arrays of descriptors of
 * device planes as for hmx_wp_acdc_multi; jobs may share pictures.  d_out (device): n_jobs * 6 values.  Samples lie in [0, 2^B).
 * Rows: weight -128..255, log2_denom 0..7, chroma offset -128..127 as for the other _wp entries; the LUMA offset may be any
 * int16, because the reference does not clip it (:279).
 * HMX_ERR_ARG, on the host before anything is launched, with the job named in hmx_last_error: a null pointer, a null plane,
 * n_jobs, n_org or n_rec out of range, an odd or non-positive size, an index outside org[] / rec[], a row outside these ranges or
 * with reserved != 0. */
typedef struct hmx_wp_sad_job {
  uint32_t org, rec; /* indices into org[] / rec[] */
  hmx_wp wp;
} hmx_wp_sad_job;    /* 24 bytes */
int hmx_wp_sad_multi(hmx_ctx *ctx, int n_jobs, const hmx_wp_sad_job *jobs, const hmx_pic *org, int n_org, const hmx_pic *rec,
                     int n_rec, int pic_w, int pic_h, int64_t *d_out);
/* Host helpers, no context, no launch; int64_t and double in the reference's order of operations.
 * hmx_wp_update_params: xUpdatingWPParameters under the denominator loop of xEstimateWPParamSlice (WeightPredAnalysis.cpp:176-204,
 * :252-304).  cur: the slice's AC/DC; refs_l0 / refs_l1: those of the ORIGINALS of the reference pictures of the two lists
 * (getRefPic(...)->getSlice(0)->getWpAcDcParam, :265), n_l1 = 0 for a P slice.  One denominator serves the slice: 6, or 7 when
 * n_l0 > 3, lowered by one while any weight w has (1 << d) - w outside -128..127.  Per row: weight = (int)(0.5 + (refAC == 0 ? 1.0 :
 * Clip3(-16.0, 15.0, curAC / refAC)) * (1 << d)), offset = ((curDC << d) - weight * refDC + (1 << (rd - 1))) >> rd, the chroma
 * offset limited as :282-288, the luma offset NOT clipped.  rows_l0 / rows_l1 [n]: the rows; present_l0 / present_l1 [n]: 1
 * (bPresentFlag, one per entry: the reference sets its three components together); *log2_denom: the denominator reached.
 * A weight of 256 at denominator 7 or a luma offset outside -128..127 can come out, as in the reference, whose encoder then
 * writes a stream outside the coded range; the consumers above refuse such a row.  HMX_ERR_ARG: a null pointer for a list that
 * has entries, a negative list size, bit_depth outside 8..12. */
int hmx_wp_update_params(const hmx_wp_acdc_param *cur, const hmx_wp_acdc_param *refs_l0, int n_l0, const hmx_wp_acdc_param *refs_l1,
                         int n_l1, int bit_depth, hmx_wp *rows_l0, hmx_wp *rows_l1, uint8_t *present_l0, uint8_t *present_l1,
                         int *log2_denom);
/* The decision of xSelectWP for one (list, reference) (WeightPredAnalysis.cpp:333-362).  sums: the six values of one job of
 * hmx_wp_sad_multi; n_luma / n_chroma: samples per plane.  SADWP / SADnoWP = the three components' sums, each divided by its
 * sample count first (:516); when (double)SADWP / (double)SADnoWP >= 0.99 the three components of *row become (1 << log2_denom,
 * 0, log2_denom) and *present 0.  0 / 0 is NaN and keeps the row; x / 0 is +inf and resets it. */
int hmx_wp_select(const int64_t *sums, int64_t n_luma, int64_t n_chroma, int log2_denom, hmx_wp *row, uint8_t *present);
/* xCheckWPEnable (WeightPredAnalysis.cpp:135-170) for the tables of one slice: *weighted = some entry is present; if none is,
 * every row becomes (1, 0, 0) (and the reference clears both PPS flags for the slice).  The reference counts the flags of all of
 * m_wp, entries that an earlier slice with longer lists left behind included; this entry sees the slice's own lists only
 * (hmx_hm::WeightPredAnalysis keeps m_wp across slices as the reference does). */
int hmx_wp_check_enable(hmx_wp *rows_l0, uint8_t *present_l0, int n_l0, hmx_wp *rows_l1, uint8_t *present_l1, int n_l1,
                        int *weighted);
/* xEstimateWPParamSlice + xCheckWPEnable (TEncSlice.cpp:706-710) for n_slices P / B slices of one picture size: hmx_wp_update_params
 * per slice, ONE hmx_wp_sad_multi launch and one download for all (list, reference) entries of the call, then hmx_wp_select and
 * hmx_wp_check_enable.  A random-access pipeline calls it once per GOP position over all its segments.  The call synchronises
 * the context's stream.  The rows are reported as the reference computes them (see hmx_wp_update_params for what may leave the
 * consumers' ranges; the call's own SAD step takes the weight 256 that hmx_wp_sad_multi refuses); rows[] / present[] are what
 * hmx_batch_*_wp, hmx_mc_wp and hmx_wp_sad_multi take.
 * HMX_ERR_ARG: what the parts refuse; a slice type other than P or B; list 0 empty, a list above HMX_WP_MAX_REFS, list 1 in a P
 * slice; slices of different sizes; more than 65535 entries in all. */
#define HMX_WP_MAX_REFS 16 /* MAX_NUM_REF (TLibCommon/CommonDef.h) */
typedef struct hmx_wp_slice {
  int slice_type;                          /* HMX_P_SLICE or HMX_B_SLICE */
  int pic_w, pic_h;
  const hmx_pic *org;                      /* the slice's original (device planes) */
  const hmx_wp_acdc_param *acdc, *d_acdc;        /* its AC/DC: a host value, or (acdc NULL) an entry of a device array */
  int n_refs[2];                           /* getNumRefIdx of list 0 / 1 */
  const hmx_pic *rec[2];                   /* host arrays [n_refs[l]]: the reference pictures' reconstructions (device planes) */
  const hmx_wp_acdc_param *ref_acdc[2];          /* host arrays [n_refs[l]] of the AC/DC of their ORIGINALS, or NULL with */
  const hmx_wp_acdc_param *const *d_ref_acdc[2]; /* host arrays [n_refs[l]] of pointers to device entries */
  hmx_wp *rows[2];                         /* out, host arrays [n_refs[l]] */
  uint8_t *present[2];                     /* out, host arrays [n_refs[l]] */
  int log2_denom;                          /* out: the denominator hmx_wp_update_params reached */
  int weighted;                            /* out: 0 = no entry present, the slice is predicted without weights */
} hmx_wp_slice;
int hmx_wp_estimate_slices(hmx_ctx *ctx, int n_slices, hmx_wp_slice *slices);

/* ------------------------------------------------------------------------------------------------
 * Adaptive QP (--AdaptiveQP=1): TEncPreanalyzer::xPreanalyze (TLibEncoder/TEncPreanalyzer.cpp:64-139), which TEncTop::encode
 * runs on every input picture (TEncTop.cpp:383-386), and TEncCu::xComputeQP (TEncCu.cpp:1114-1136), which turns its result into
 * the QP of every coding unit.  The analysis has depths = MaxCuDQPDepth + 1 layers (TEncTop.cpp:440); layer d has units of
 * part[d] = ctu >> d samples, nx[d] = ceil(pic_w / part[d]) by ny[d] = ceil(pic_h / part[d]) of them in raster order
 * (TEncPic.cpp:82-89, :135-138).  Arrays per picture: the layers one after the other, layer d at first[d], units row-major;
 * total units per picture.
 * Size domain of every entry below (anything else is HMX_ERR_ARG, before anything is launched): ctu 16, 32 or 64; depths >= 1
 * with ctu >> (depths - 1) >= 8; pic_w and pic_h positive multiples of 8 (what the encoder's padding to the minimum CU size gives
 * it) up to 16384; n_pics 1..65535; the context's bit depth B 8..12.
 * ---------------------------------------------------------------------------------------------- */
#define HMX_AQ_MAX_DEPTHS 4
typedef struct hmx_aq_geom {
  int pic_w, pic_h, ctu, depths;
  int part[HMX_AQ_MAX_DEPTHS];  /* getAQPartWidth = getAQPartHeight */
  int nx[HMX_AQ_MAX_DEPTHS];    /* getNumAQPartInWidth = getAQPartStride */
  int ny[HMX_AQ_MAX_DEPTHS];    /* getNumAQPartInHeight */
  int first[HMX_AQ_MAX_DEPTHS]; /* index of the layer's first unit in a picture's arrays */
  int total;                    /* units of all layers of one picture */
} hmx_aq_geom;
/* The layout of one picture's arrays (host, no context). */
int hmx_aq_layout(int pic_w, int pic_h, int ctu, int depths, hmx_aq_geom *out);
/* xPreanalyze (TEncPreanalyzer.cpp:64-139) for n_pics ORIGINAL pictures: every luma sample is read once for all layers.  Per
 * unit, cut by the picture edge to cw x ch, the four quadrants split at cw >> 1 and ch >> 1; per quadrant avg = double(sum) / N
 * and var = double(sumsq) / N - avg * avg with N = cw * ch, the samples of the WHOLE unit (:94-126: uiNumPixInAQPart counts every
 * sample of the unit); activity = 1.0 + min(var) (:129); the layer's average = the activities added in raster order, in double,
 * over nx * ny (:131-136).  pics: host array [n_pics] of descriptors of device planes as for hmx_wp_acdc_multi (own strides,
 * margins, unaligned planes); only plane[0] is read.  Samples lie in [0, 2^B).  d_act (device): [n_pics][total] doubles; d_avg
 * (device): [n_pics][depths] doubles; both are the reference's doubles bit for bit.
 * HMX_ERR_ARG: a null pointer, a null luma plane, anything outside the size domain. */
int hmx_aq_activity_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *pics, int pic_w, int pic_h, int ctu, int depths, double *d_act,
                          double *d_avg);
int hmx_aq_activity(hmx_ctx *ctx, const hmx_pic *pic, int pic_w, int pic_h, int ctu, int depths, double *d_act, double *d_avg); /* = _multi with n_pics = 1 */
/* The second half of hmx_aq_activity_multi on its own: the layers' averages (TEncPreanalyzer.cpp:79, :131-137) of activities that
 * lie on the device, the same ordered sums (tools/aq_bench.py times them through this entry).  HMX_ERR_ARG as above. */
int hmx_aq_average_multi(hmx_ctx *ctx, int n_pics, int pic_w, int pic_h, int ctu, int depths, const double *d_act, double *d_avg);
/* xComputeQP (TEncCu.cpp:1114-1136) for every unit of every layer of n_pics pictures: d_qp (device) [n_pics][total], unit u of
 * layer d = Clip3(-qp_bd_offset, 51, slice_qp[pic] + offset) with S = pow(2.0, range / 6.0) (:1128, formed on the host),
 * norm = (S * act + avg) / (act + S * avg) (:1131, on the device, not contracted) and offset = Int(floor(log(norm) / log(2.0) * 6.0
 * + 0.49999)) (:1132-1133).  The logarithm is the HOST's: the device counts the entries of hmx_aq_thresholds(range) that are <=
 * norm.  A CU at depth D reads layer min(D, depths - 1), unit (cuX / part, cuY / part) (:1121-1124).  range =
 * getQPAdaptationRange() 1..64; slice_qp: host array [n_pics], each -qp_bd_offset..51; qp_bd_offset = getQpBDOffsetY() 0..48.
 * HMX_ERR_ARG: a null pointer, anything outside these ranges or the size domain; HMX_ERR_INTERNAL: the threshold table did not
 * verify (hmx_last_error names the offset). */
int hmx_aq_qp_map_multi(hmx_ctx *ctx, int n_pics, int pic_w, int pic_h, int ctu, int depths, const double *d_act, const double *d_avg,
                        const int *slice_qp, int range, int qp_bd_offset, int8_t *d_qp);
/* From the layers to the map hmx_set_qp_map and hmx_deblock_picture_multi read, on the device: d_qp [n_pics][pic_h / 4][pic_w / 4]
 * (device) gets, for every 4x4 luma unit, the QP of the coding unit that covers it -- d_cu_depth [n_pics][pic_h / 4][pic_w / 4]
 * (device) holds that CU's depth D, and the unit reads layer min(D, depths - 1) of d_layer_qp (hmx_aq_qp_map_multi's output), unit
 * (x / part, y / part) (TEncCu.cpp:1121-1124).  A depth byte above the last layer is clamped like any other.  Size domain and
 * refusals as above: HMX_ERR_ARG for a null pointer or anything outside the domain, before anything is launched. */
int hmx_aq_unit_qp_multi(hmx_ctx *ctx, int n_pics, int pic_w, int pic_h, int ctu, int depths, const int8_t *d_layer_qp,
                         const uint8_t *d_cu_depth, int8_t *d_qp);
/* out[k + range], k = -range .. range: the smallest double at which floor(log(n) / log(2.0) * 6.0 + 0.49999), evaluated on the host
 * with libm, reaches k; found by bisection over the doubles and held against the 64 doubles on either side of it (a
 * disagreement is HMX_ERR_INTERNAL).  Built once per range (1..64). */
int hmx_aq_thresholds(int range, double *out);
/* Host scalars, no context.  hmx_aq_offset: iQpOffset of TEncCu.cpp:1128-1133, the literal expression with libm.
 * hmx_aq_compute_qp: xComputeQP on downloaded data (act: one picture's [total], avg: its [depths]) for the CU at luma position
 * (cu_x, cu_y) and depth cu_depth; HMX_AQ_NO_QP for a null pointer or a position outside the picture. */
#define HMX_AQ_NO_QP (-128)
int hmx_aq_offset(double act, double avg_act, int range);
int hmx_aq_compute_qp(const hmx_aq_geom *geom, const double *act, const double *avg, int cu_x, int cu_y, int cu_depth, int slice_qp,
                      int range, int qp_bd_offset);

/* Deblocking filter, the application part (TLibCommon/TComLoopFilter.cpp:571-922: xEdgeFilterLuma, xEdgeFilterChroma,
 * the pel filters, the strong/weak decision), in place on a reconstructed picture whose size
 * is a multiple of 8.  Maps (device) hold one entry per 4x4 luma unit in raster order: d_bs_ver[u] = boundary
 * strength 0..2 of the vertical edge on the unit's LEFT side, d_bs_hor[u] = of the horizontal edge on its TOP side
 * (what xGetBoundaryStrengthSingle :444 leaves in m_aapucBS; 0 on the picture boundary); d_qp[u] = the unit's luma
 * QP (TComDataCU::getQP); d_no_filter[u] != 0 (may be NULL) keeps a unit's samples: IPCM with
 * pcm_loop_filter_disable (:609-614).  (The reference's lossless flags are ORed into variables that stay set for
 * the rest of a CU's edge, :616-617; that CU-shaped stickiness is not reproduced.)  Edges on the 8x8 luma grid
 * are filtered, chroma on its own 8x8 grid for strength 2; all vertical edges, then all horizontal ones. */
/* The boundary strengths of the 8x8-grid edges, xGetBoundaryStrengthSingle (TComLoopFilter.cpp:444-569).  d_units[u]
 * = what the function reads of a 4x4 partition: intra flag, luma cbf of its transform block and, per reference
 * list, a picture id (< 0: list unused; equal ids = same picture) and the motion vector.  d_edge_ver / d_edge_hor[u]:
 * 0 = the unit's left / top side is not a filtered edge (m_aapbEdgeFilter), 1 = filtered edge, 3 = filtered edge
 * that is also a transform-block or coding-block edge (the value xSetEdgefilterTU / xSetEdgefilterMultiple leave
 * in m_aapucBS).  Horizontal edges on a CTU boundary read the P side's motion at the compressed position
 * (g_motionRefer, TComRom.cpp:221-258).  Outputs feed hmx_deblock_picture. */
typedef struct hmx_dbk_unit {
  uint8_t intra, cbf;
  int8_t ref[2];
  int16_t mv[2][2]; /* [list][x, y], quarter-pel */
} hmx_dbk_unit;
int hmx_deblock_strengths(hmx_ctx *ctx, const hmx_dbk_unit *d_units, const uint8_t *d_edge_ver, const uint8_t *d_edge_hor,
                          int pic_w, int pic_h, int is_b_slice, uint8_t *d_bs_ver, uint8_t *d_bs_hor);
int hmx_deblock_picture(hmx_ctx *ctx, const hmx_pic *rec, int pic_w, int pic_h, const uint8_t *d_bs_ver,
                        const uint8_t *d_bs_hor, const int8_t *d_qp, const uint8_t *d_no_filter, int beta_offset_div2,
                        int tc_offset_div2);
/* The same for n_pics (1..65535) pictures of one size in one launch each (loopFilterPic :153-201 per picture; the
 * deblocking filters both directions of a picture in one pass).  Picture i of the batch gets what the single-picture call
 * gives for picture i's arguments; the single-picture calls are these with n_pics = 1.
 * rec: host array [n_pics] of descriptors of device planes (each picture its own planes and strides; margins and unaligned
 * planes allowed).  Two entries of rec must not alias (they are filtered in place, concurrently); this is not checked.
 * Device maps are contiguous per picture, [pic][4x4 unit in raster order]: d_units, d_edge_ver, d_edge_hor, d_bs_ver,
 * d_bs_hor, d_qp, d_no_filter (may be NULL, for all pictures).  is_b_slice, beta_offset_div2, tc_offset_div2: host arrays
 * [n_pics] (slice-level values, slice_deblocking_filter offsets :593-594); the two offset arrays may be NULL = 0.
 * HMX_ERR_ARG, before anything is launched: a null pointer, a null plane, n_pics out of range, pic_w or pic_h not a
 * positive multiple of 8. */
int hmx_deblock_strengths_multi(hmx_ctx *ctx, int n_pics, const hmx_dbk_unit *d_units, const uint8_t *d_edge_ver,
                                const uint8_t *d_edge_hor, int pic_w, int pic_h, const uint8_t *is_b_slice,
                                uint8_t *d_bs_ver, uint8_t *d_bs_hor);
int hmx_deblock_picture_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *rec, int pic_w, int pic_h, const uint8_t *d_bs_ver,
                              const uint8_t *d_bs_hor, const int8_t *d_qp, const uint8_t *d_no_filter,
                              const int8_t *beta_offset_div2, const int8_t *tc_offset_div2);

/* Sample adaptive offset, the application part (TLibCommon/TComSampleAdaptiveOffset.cpp:781-1240: SAOProcess,
 * processSaoUnitAll, processSaoCuOrg), from the deblocked picture `in` to `out` (different
 * buffers: the reference's line buffers exist to keep the unfiltered neighbours an in-place pass destroys).
 * d_params (device): [component][CTU in raster order], merge flags already resolved: type -1 = off, 0..3 = edge
 * offset classes (horizontal, vertical, 135, 45 degrees), 4 = band offset from band `band` of 32; four offsets,
 * scaled by << (bit depth - min(bit depth, 10)).  n_lcu = CTUs of the picture. */
typedef struct hmx_sao_lcu {
  int8_t type;
  uint8_t band;
  int8_t offset[4];
} hmx_sao_lcu;
int hmx_sao_picture(hmx_ctx *ctx, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h, const hmx_sao_lcu *d_params,
                    int n_lcu);
/* The same for n_pics (1..65535) pictures of one size in one launch (SAOProcess :781 per picture); hmx_sao_picture is this
 * with n_pics = 1.  in / out: host arrays [n_pics] of descriptors of device planes (each picture its own planes and strides;
 * margins and unaligned planes allowed).  d_params (device): [pic][component][CTU in raster order].  Two entries of out
 * must not alias, and no entry of out may alias an entry of in; only in[i] against out[i] is checked.
 * HMX_ERR_ARG, before anything is launched: a null pointer, a null plane, n_pics out of range, an odd or non-positive size,
 * n_lcu not the CTU count of a picture, in[i] and out[i] sharing a plane. */
int hmx_sao_picture_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h,
                          const hmx_sao_lcu *d_params, int n_lcu);

/* Which neighbour CTUs the loop filters of a CTU may read: TComDataCU::setNDBFilterBlockBorderAvailability
 * (TLibCommon/TComDataCU.cpp:4212-4634, as compiled with MODIFIED_CROSS_SLICE 1 and REMOVE_FGS 1: one block per CTU), called
 * from TComPic::createNonDBFilterInfo (TComPic.cpp:138-339).  Host only, no context.  avail[CTU in raster order]: bit k set =
 * neighbour k may be read, k as the SGU_* enumeration (TComDataCU.h:64-72): 0 L, 1 R, 2 T, 3 B, 4 TL, 5 TR, 6 BL, 7 BR.
 *   a neighbour outside the picture is unavailable (:4271, :4415 ...);
 *   a neighbour in the same slice is available; one in a LATER slice when that slice's flag is set, one in an EARLIER slice
 *   when this slice's flag is set (:4299); a picture with one slice skips the slice test (onlyOneSliceInPic, :4220);
 *   with lf_cross_tiles == 0 the result is ANDed with "same tile" (:4589-4623).
 * slice_id[CTU in raster order]: index of the CTU's slice in decoding order (slices begin at CTU boundaries; a dependent slice
 * belongs to its independent slice); slice_lf_cross[n_slices]: slice_loop_filter_across_slices_enabled_flag of each slice;
 * tile_id[CTU] (may be NULL: one tile); lf_cross_tiles: loop_filter_across_tiles_enabled_flag of the PPS.  The reference takes
 * the availability path of SAO (m_bUseNIF, TComSampleAdaptiveOffset.cpp:500) as soon as a flag is 0 with more than one slice /
 * tile; with every bit inside the picture set the two paths give the same pictures.  The deblocking filter drops the left /
 * top edges of a CTU whose L / T bit is clear (TComLoopFilter.cpp:411, 432, 458, 462: the left and top neighbours are never in
 * a later slice, so this slice's flag decides there too): clear those entries of d_edge_ver / d_edge_hor or d_bs_ver / d_bs_hor.
 * HMX_ERR_ARG: a null pointer other than tile_id, a non-positive size or n_slices, a slice id >= n_slices. */
int hmx_lf_border_avail(int pic_w, int pic_h, int ctu_size, const uint32_t *slice_id, const uint8_t *slice_lf_cross, int n_slices,
                        const uint32_t *tile_id, int lf_cross_tiles, uint8_t *avail);
/* hmx_sao_picture_multi on the availability path: processSaoCu -> processSaoBlock (TComSampleAdaptiveOffset.cpp:515-776) for
 * every CTU (cut at the picture edge) and component; the chroma planes use the CTU's luma byte.  d_avail (device):
 * [pic][CTU in raster order] bytes of hmx_lf_border_avail.  An edge-offset sample is filtered exactly when each of its two
 * neighbours lies in its own CTU or in a neighbour CTU whose bit is set, and copied otherwise (what the start / end columns
 * and the first-line, last-line and corner branches of :573-759 come to); band offset ignores the bytes (:760-772).  No sample
 * of a CTU whose bit is clear contributes to the output.  A mask with every bit inside the picture set gives what
 * hmx_sao_picture_multi gives.  HMX_ERR_ARG as for hmx_sao_picture_multi, and for a null d_avail. */
int hmx_sao_picture_multi_avail(hmx_ctx *ctx, int n_pics, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h,
                                const hmx_sao_lcu *d_params, int n_lcu, const uint8_t *d_avail);

/* Sample adaptive offset, the encoder's statistics pass: TEncSampleAdaptiveOffset::calcSaoStatsCuOrg
 * (TLibEncoder/TEncSampleAdaptiveOffset.cpp:859-1124 with SAO_SKIP_RIGHT, TLibCommon/TypeDef.h:123), which rdoSaoUnitAll
 * (:1617, via calcSaoStatsCu) runs for every CTU and component between deblocking and the parameter search.  For every CTU
 * and component of n_pics pictures: the sum of org - rec and the sample count of every edge and band class.
 * org / rec: host arrays [n_pics] of descriptors of device planes (each picture its own planes and strides; margins and
 * unaligned planes allowed; org == rec allowed); rec is the deblocked picture, its samples in [0, 2^B).
 * d_out (device): [pic][component][CTU in raster order][HMX_SAO_STAT_BINS]; every bin is written, zeros included.
 * Per CTU of a plane (chroma 4:2:0: sizes and positions >> 1): W x H = the CTU cut at the picture edge; L / T / R / Bt = it
 * touches the left / top / right / bottom picture edge; s = 4 (luma) or 2 (chroma) bottom rows and r = 5 or 3 right
 * columns are skipped, both 0 when lcu_based == 0 (SAOLcuBasedOptimization = 0, :886-896).  CTU-local ranges:
 *   band (type 4)   x in [0, R ? W : W-r)    y in [0, Bt ? H : H-s)      class 1 + (rec >> (B - 5))
 *   EO_0 (type 0)   x in [L, R ? W-1 : W-r)  y in [0, H-s)  (bottom rows skipped even on the picture edge, :971)
 *   EO_1 (type 1)   x in [0, R ? W : W-r)    y in [T, Bt ? H-1 : H-s)
 *   EO_2, EO_3      x in [L, R ? W-1 : W-r)  y in [T, Bt ? H-1 : H-s)
 * Edge class = m_auiEoTable[sign(c - a) + sign(c - b) + 2] (TComSampleAdaptiveOffset.cpp:94; {1, 2, 0, 3, 4}), class 0
 * ("no edge") included; neighbours a, b: (x-1,y),(x+1,y) | (x,y-1),(x,y+1) | (x-1,y-1),(x+1,y+1) | (x+1,y-1),(x-1,y+1), read
 * from the picture across CTU edges.  The NIF path (calcSaoStatsBlock: slice / tile boundaries not crossed,
 * TComSampleAdaptiveOffset.cpp:500) is hmx_sao_stats_multi_avail below.  What follows the statistics with SAOLcuBasedOptimization = 1
 * (offset estimation, estSaoDist, merge, CABAC rates) is hmx_sao_decide_multi further down, which takes d_out as it is.  Not
 * covered: the quadtree part sums of SAOLcuBasedOptimization = 0 (the host sums these per-CTU bins).  |diff| <= 64*64*(2^12 - 1)
 * fits int32.  HMX_ERR_ARG: a null pointer, n_pics < 1, pic_w or pic_h not a positive multiple of 8. */
typedef struct hmx_sao_stat {
  int32_t diff, count;
} hmx_sao_stat;
#define HMX_SAO_STAT_BINS 52 /* bin 5*t + c: edge type t 0..3, class c 0..4 (after m_auiEoTable); bin 20 + k - 1: band class k 1..32 */
int hmx_sao_stats_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h, int lcu_based,
                        hmx_sao_stat *d_out);
int hmx_sao_stats(hmx_ctx *ctx, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h, int lcu_based,
                  hmx_sao_stat *d_out); /* = _multi with n_pics = 1 */
/* The statistics on the availability path: calcSaoStatsCu -> calcSaoStatsBlock (TLibEncoder/TEncSampleAdaptiveOffset.cpp
 * :571-854) for every CTU and component, d_avail (device) as for hmx_sao_picture_multi_avail.  The same 52 bins; no rows or
 * columns are skipped (the block path has no SAO_SKIP_RIGHT).  Band: every sample of the CTU.  Edge type t: the samples whose
 * two neighbours each lie in the CTU or in a neighbour CTU whose bit is set.  A mask with every bit inside the picture set
 * gives what hmx_sao_stats_multi gives with lcu_based = 0.  HMX_ERR_ARG as for hmx_sao_stats_multi, and for a null d_avail. */
int hmx_sao_stats_multi_avail(hmx_ctx *ctx, int n_pics, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h,
                              const uint8_t *d_avail, hmx_sao_stat *d_out);

/* Sample adaptive offset, the encoder's parameter search with SAOLcuBasedOptimization = 1 (the default, TAppEncCfg.cpp:271):
 * TEncSampleAdaptiveOffset::rdoSaoUnitAll (TLibEncoder/TEncSampleAdaptiveOffset.cpp:1466-1799) for n_pics pictures, from the bins
 * of hmx_sao_stats_multi[_avail] to the table hmx_sao_picture_multi[_avail] takes, device to device.  Restated: the constants of
 * SAOProcess (:1253-1263: m_uiSaoBitIncrease = B - min(B, 10), m_iOffsetTh = 1 << min(B - 5, 5), shift = 2 * (B - 8)); the CTU
 * walk with allowMergeLeft / allowMergeUp (:1536-1562) and the choice between new parameters, merge left and merge up
 * (compDistortion[k] + (Double)rate, strict <, in the reference's order, :1663-1748); estSaoTypeDist (:1808-1852: the xRoundIbdi
 * quotient, the clip to +-(m_iOffsetTh - 1), the sign rule of the edge classes), estSaoDist (:1854) and estIterOffset (:1858-1893:
 * the (Int) of the band distortions, the rate decrement at the clip value); saoComponentParamDist (:1897-2062) and
 * sao2ChromaParamDist (:2064-2240): the "off" cost, the band-start search (sums of four doubles in index order, first minimum),
 * Cb and Cr sharing one type with their own band starts, bestDist / lambda, and the merge candidates' distortions from the
 * neighbours' final parameters, whose offsets enter estSaoDist as stored, without << m_uiSaoBitIncrease (:2046-2047, :2224-2225;
 * shows at 12 bit only).  Rates: TEncEntropy::encodeSaoOffset (TEncEntropy.cpp:759-838, with its write to subTypeIdx of edge
 * types of components 0 and 1, :785), TEncSbac::codeSaoTypeIdx / codeSaoMerge / codeSaoMaxUvlc / codeSAOSign / codeSaoUflc
 * (TEncSbac.cpp:1562-1716) under TEncBinCABACCounter (TEncBinCoderCABACCounter.cpp:61-101: fractional bits from
 * ContextModel::getEntropyBits, 32768 per bypass bin, written bits = fracBits >> 15; resetBits keeps the low 15 bits,
 * TEncBinCoderCABAC.cpp:193; load / store copy them, :178), with the loads and stores between CI_CURR_BEST and CI_TEMP_BEST as the
 * reference sequences them.  Macros as the fork sets them (TypeDef.h:87-91, 121-130, 147, 218): SAO_SINGLE_MERGE,
 * SAO_TYPE_SHARING, SAO_TYPE_CODING, SAO_MERGE_ONE_CTX, SAO_ABS_BY_PASS, SAO_ENCODING_CHOICE[_CHROMA], SAO_CHROMA_LAMBDA,
 * FAST_BIT_EST, FULL_NBIT 0.  CTU size and bit depth (8..12) come from the context.
 * Not covered: the quadtree search of SAOLcuBasedOptimization = 0 (rdoSaoOnePart, runQuadTreeDecision), SaoLcuBoundary /
 * interleaved SAO, writing the bitstream.
 * d_stats (device): what hmx_sao_stats_multi[_avail] wrote, [pic][3][CTU][HMX_SAO_STAT_BINS]; count >= 0 and |diff| <= count *
 * (2^B - 1), as every real picture gives.  params: HOST array [n_pics].  d_merge_allow (device, may be NULL): [pic][CTU] bytes,
 * bit 0 = merge left allowed, bit 1 = merge up allowed (hmx_sao_merge_allow); NULL = geometry only.  The first column never
 * merges left and the first row never merges up, whatever the byte says (:1548-1562).
 * d_units (device): [pic][3][CTU], the parameters as rdoSaoUnitAll leaves them in saoLcuParam.  d_apply (device, may be NULL):
 * [pic][3][CTU], the same as hmx_sao_picture_multi takes it: offsets << (B - min(B, 10)), band = sub where type is 4, type -1
 * everywhere for a component whose enable flag is 0.  d_result (device): [pic].
 * HMX_ERR_ARG, before anything is launched: a null pointer other than d_merge_allow and d_apply, n_pics outside 1..65535, a size
 * that is not a positive multiple of 8, a lambda that is not finite and positive, a context state above 127, a fraction
 * above 32767. */
typedef struct hmx_sao_decide_param {
  double lambda_luma, lambda_chroma; /* m_dLambdaLuma / m_dLambdaChroma (SAOProcess :1241-1242) */
  uint8_t enable[2];                 /* bSaoFlag of luma / chroma after :1503-1513 (hmx_sao_rate_flags) */
  uint8_t ctx_state[2];              /* ContextModel::m_ucState of the merge and the type context at the picture's start
                                        (hmx_sao_ctx_init) */
  uint32_t frac;                     /* the fractional bits the coder holds when startSaoEnc runs, below 32768: 0 for a fresh coder.
                                        Inside the reference encoder they are what the picture's last rate estimate left, because
                                        TEncBinCABAC::start (TEncBinCoderCABAC.cpp:69-76) does not clear m_fracBits and resetBits
                                        (:193) keeps its low 15 bits */
} hmx_sao_decide_param; /* 24 bytes */
typedef struct hmx_sao_unit { /* SaoLcuParam as coded: 8 bytes */
  int8_t type;       /* typeIdx: -1 off, 0..3 edge, 4 band */
  uint8_t sub;       /* subTypeIdx: the band start for type 4; for edge types the type (luma, Cb) or 0 (Cr), TEncEntropy.cpp:780-786 */
  int8_t offset[4];  /* unscaled */
  uint8_t merge_left, merge_up;
} hmx_sao_unit;
typedef struct hmx_sao_result {
  uint32_t num_no_sao[2]; /* numNoSao of :1751-1759 (chroma counts 2 per CTU) */
  uint8_t ctx_state[2];   /* the two context states after the last CTU */
  uint8_t reserved[2];
  uint32_t frac;          /* m_fracBits after the last CTU (below 32768) */
} hmx_sao_result; /* 16 bytes */
int hmx_sao_decide_multi(hmx_ctx *ctx, int n_pics, const hmx_sao_stat *d_stats, int pic_w, int pic_h,
                         const hmx_sao_decide_param *params, const uint8_t *d_merge_allow, hmx_sao_unit *d_units,
                         hmx_sao_lcu *d_apply, hmx_sao_result *d_result);
int hmx_sao_decide(hmx_ctx *ctx, const hmx_sao_stat *d_stats, int pic_w, int pic_h, const hmx_sao_decide_param *param,
                   const uint8_t *d_merge_allow, hmx_sao_unit *d_units, hmx_sao_lcu *d_apply,
                   hmx_sao_result *d_result); /* = _multi with n_pics = 1 */
/* Statistics, decision and application of a batch in order on the context's stream, device buffers only: hmx_sao_stats_multi
 * (lcu_based = 1) -> hmx_sao_decide_multi -> hmx_sao_picture_multi from rec to out, or with d_avail (device, [pic][CTU] bytes of
 * hmx_lf_border_avail; NULL = the plain path) the three _avail entries.  d_stats, d_units, d_apply, d_result: device buffers of
 * the sizes above, all required.  HMX_ERR_ARG as for the three entries, before anything is launched. */
int hmx_sao_encode_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *org, const hmx_pic *rec, const hmx_pic *out, int pic_w, int pic_h,
                         const hmx_sao_decide_param *params, const uint8_t *d_merge_allow, const uint8_t *d_avail,
                         hmx_sao_stat *d_stats, hmx_sao_unit *d_units, hmx_sao_lcu *d_apply, hmx_sao_result *d_result);
/* Host helpers, no context.  hmx_sao_ctx_init: the two context states startSaoEnc (:530-546) leaves after resetEntropy
 * (TEncSbac.cpp:112-160): ContextModel::init (ContextModel.cpp:56-65) of INIT_SAO_MERGE_FLAG and INIT_SAO_TYPE_IDX
 * (ContextTables.h:383, 414) for slice_type (the reference's SliceType: 0 B, 1 P, 2 I; with cabac_init_flag the table index
 * resetEntropy substitutes, TEncSbac.cpp:117-121) and the slice QP; state[0] = merge, state[1] = type.  The fraction is hmx_sao_decide_param::frac. */
int hmx_sao_ctx_init(int slice_type, int qp, uint8_t *state);
/* m_depthSaoRate (:1503-1513, :1788-1789): flags gives bSaoFlag of luma and chroma for a picture of hierarchy depth `depth`
 * (off when depth > 0 and the rate of depth - 1 exceeds SAO_ENCODING_RATE 0.75 / SAO_ENCODING_RATE_CHROMA 0.5, TypeDef.h:127-130);
 * update stores num_no_sao / n_ctu and num_no_sao / (2 n_ctu) of a decided picture.  A zeroed state is the encoder's start. */
#define HMX_SAO_RATE_DEPTHS 4
typedef struct hmx_sao_rate_state {
  double rate[2][HMX_SAO_RATE_DEPTHS];
} hmx_sao_rate_state;
int hmx_sao_rate_flags(const hmx_sao_rate_state *state, int depth, uint8_t *enable);
int hmx_sao_rate_update(hmx_sao_rate_state *state, int depth, const uint32_t *num_no_sao, int n_ctu);
/* allowMergeLeft / allowMergeUp of :1536-1562 from the CTU maps hmx_lf_border_avail takes (tile_id may be NULL: one tile):
 * out[CTU] bit 0 = the left CTU exists and shares slice and tile, bit 1 = the same for the CTU above. */
int hmx_sao_merge_allow(int pic_w, int pic_h, int ctu_size, const uint32_t *slice_id, const uint32_t *tile_id, uint8_t *out);

/* Planar 4:2:0 YUV frames, the format either side of the path (TLibVideoIO/TVideoIOYuv.cpp:226-480, SURVEY.md
 * 8f rank 4).  d_file (device) holds one frame as the file does: 8-bit or 16-bit little-endian samples, Y then
 * Cb then Cr.  unpack = TVideoIOYuv::read: the file's (w_full - pad_x) x (h_full - pad_y) samples are padded to
 * the right and below by replication and every sample is scaled from file_bits to the context's bit depth
 * (<< when deeper; (v + half) >> s clipped to [0, 2^bits - 1] when shallower).  pack = TVideoIOYuv::write:
 * scaled the other way, the top-left (w - crop_right) x (h - crop_bottom) samples stored.
 * hmx_yuv_frame_bytes(w, h, file_bits) = size of a frame of w x h samples. */
size_t hmx_yuv_frame_bytes(int w, int h, int file_bits);
int hmx_yuv_unpack(hmx_ctx *ctx, const void *d_file, int file_bits, const hmx_pic *dst, int w_full, int h_full, int pad_x,
                   int pad_y);
int hmx_yuv_pack(hmx_ctx *ctx, const hmx_pic *src, int w, int h, int crop_right, int crop_bottom, int file_bits, void *d_file);

/* One picture's motion compensation in a multi-picture call. */
typedef struct hmx_mc_job {
  const hmx_pu *d_pus; /* device */
  int n_pus;
  const hmx_pic *refs; /* host array [n_refs]; hmx_pu::ref0/ref1 index it */
  int n_refs;
  const hmx_pic *dst;
  int pic_w, pic_h;    /* luma picture size; when > 0 the PUs are scattered into a 4x4-cell map and the
                          prediction runs one lane per cell of the picture (full waves whatever the PU sizes);
                          0: one wave per PU */
} hmx_mc_job;
/* The batch entry points over SEVERAL pictures in one launch each (grid.y = picture): pictures at the
 * same position of different intra-period segments are independent, so a random-access
 * encoder issues one call per GOP position, not one per picture.  The block list (decisions) is shared
 * by the pictures of a call; planes and levels are arrays of n_pics entries.  d_abs_sum, if not NULL,
 * holds n_pics * (blocks of the list) sums, picture-major. */
int hmx_batch_motionCompensation_multi(hmx_ctx *ctx, int n_jobs, const hmx_mc_job *jobs);
/* hmx_batch_motionCompensation_multi under explicit weighted prediction (TComPrediction.cpp:421-432, :516-535 ->
 * TComWeightPrediction.cpp:251-386).  wp: host array [n_jobs], wp[i] = the tables of jobs[i].  Both schedules of hmx_mc_job are
 * supported.  A job whose tables are both NULL is predicted exactly as hmx_batch_motionCompensation_multi predicts it.  A
 * weighted job gives l0 (l0 NULL with l1 set is HMX_ERR_ARG); with l1 NULL a unit that uses list 1 all the same is weighted by 1.
 * The tables are indexed by the same hmx_pu::ref0 / ref1 as hmx_mc_job::refs: a picture that sits in a list twice with different
 * weights (or in both lists of a B slice, where l0[k] and l1[k] belong to the same refs[k]) is entered in refs[] once per
 * distinct weight pair. */
typedef struct {            /* the tables of one hmx_mc_job; both NULL = this job is not weighted */
  const hmx_wp *l0, *l1;    /* host arrays [n_refs], indexed like hmx_mc_job::refs by hmx_pu::ref0 / ref1; l1 may be NULL
                               when no unit of the job uses list 1 (P slice) */
} hmx_mc_wp;
int hmx_batch_motionCompensation_wp_multi(hmx_ctx *ctx, int n_jobs, const hmx_mc_job *jobs, const hmx_mc_wp *wp);

/* ------------------------------------------------------------------------------------------------
 * Prediction error of complete motion candidates: TEncSearch::xGetInterPredictionError (TLibEncoder/TEncSearch.cpp:3059-3081),
 * the call predInterSearch makes per merge candidate (xMergeEstimation, :3096-3149), for the search result the merge winner is
 * compared with (:3771-3796) and -- as xGetTemplateCost (:4057-4118) -- per AMVP candidate (xEstimateMvPredAMVP, :3839-3926).
 * One fused launch: the original block of a unit is read once, every candidate's luma prediction is formed in LDS and never
 * written, costed, and the winner of each group decided on the device.  All arithmetic is uint32_t, wrapping like UInt.
 * ---------------------------------------------------------------------------------------------- */
typedef struct { uint32_t index, dist, cost; } hmx_pred_choice;   /* 12 bytes */
/* cands: HOST array of n candidates (hmx_pu; an unused list has ref0 / ref1 = 255; vectors in quarter samples, clipped with
 * hmx_clipMv).  bits: HOST array parallel to it (uiBitsCand, uiMEBits, m_auiMVPIdxCost[i][n]); NULL = 0 for every candidate.
 * group_first: HOST prefix array of n_groups + 1 entries, group_first[0] = 0, group_first[n_groups] = n; the candidates of a
 * group share x, y, w, h (the kernel stages that original block once).  group_first = NULL with n_groups = 0 and d_best = NULL:
 * costs only.  refs (n_refs <= 4) / org: device pictures, the references with margins of margin_x / margin_y luma samples.
 * Prediction: the luma part of TComPrediction::motionCompensation(..., REF_PIC_LIST_X, iPartIdx) (TLibCommon/TComPrediction.cpp:
 * 410-540): one list = xPredInterLumaBlk with the final rounding; two lists = both into the 14-bit intermediate, then addAvg.
 * The identical-motion shortcut (xCheckIdenticalMotion, :392-407) needs POCs the library does not see: the caller passes such a
 * candidate with one list.  Distortion, always UNWEIGHTED (bApplyWeight = false, TEncSearch.cpp:3070): use_had = 1 xGetHADs
 * (TComRdCost.cpp:2186-2283; 8x8 sub-blocks when both sides are multiples of 8, else 4x4, rounded per sub-block as
 * hmx_batch_subpel_cost documents), use_had = 0 the SAD over every row (iSubShift = 0, :397); both >> (bit depth - 8).
 * d_dist[i] (device) = the distortion; d_cost[i] (device) = d_dist[i] + ((lambda * bits[i]) >> 16) (getCost(UInt), TComRdCost.h:
 * 204); d_best[g] (device) = the first candidate of group g, in array order, whose cost is strictly smaller than a running best
 * that starts at 0xFFFFFFFF (ruiCost = MAX_UINT, :3120, :3139), index counted inside the group; an empty group, or one whose
 * every cost is 0xFFFFFFFF, gives {0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF}.
 * xGetTemplateCost: with ZERO_MVD_EST 0 (TypeDef.h:183) it costs with SAD whatever UseHADME says (:4111-4115) -- call with
 * use_had = 0 -- and adds the bits through calcRdCost(..., DF_SAD) (TComRdCost.cpp:94-98), a double product floored: that equals
 * getCost(UInt) exactly while lambda * bits < 2^31, which the caller must hold.  Its running best starts at MAX_INT with index 0
 * (:3850, :3906), not 0xFFFFFFFF: decide from d_cost.
 * HMX_ERR_ARG, on the host before anything is launched, with the candidate or group named in hmx_last_error: a NULL pointer other
 * than bits, group_first / d_best as allowed above, and wp; n < 1; n_refs outside 1..4; use_had other than 0 or 1; a size outside
 * {4, 8, 12, 16, 24, 32, 48, 64}; a candidate with no list; a used reference index >= n_refs; the unit outside the picture; a
 * prefix array that is not monotonic or does not end at n; a group whose candidates differ in x, y, w, h; for any used list the
 * displaced block grown by the tap window -- columns x + (mvx >> 2) - 3 .. + w + 3, rows likewise, whatever the fraction --
 * reaching outside [-margin, pic + margin) in either direction (conservative; never refuses a vector hmx_clipMv produced for a
 * unit inside a 64x64 CTU with 80-sample margins: the reach is at most 74 samples).  Not covered: chroma, the NS_HAD shapes.
 * Longest list (see LIST LENGTH at hmx_batch_subpel_cost): R(16 n) + R(4 n) + R(4 (n_groups + 1)) <= 8388608 -- sizeof(hmx_pu) =
 * 16; the middle term only with bits; costs only counts as n_groups = n.  With bits: n <= 403280 in groups of five, 349504 in
 * groups of one or costs only; without bits: n <= 419424 costs only.  A longer one is HMX_ERR_NOMEM before anything is launched. */
int hmx_batch_inter_pred_error(hmx_ctx *ctx, const hmx_pu *cands, const uint32_t *bits, int n, const uint32_t *group_first,
                               int n_groups, const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w, int pic_h,
                               int margin_x, int margin_y, uint32_t lambda, int use_had, uint32_t *d_dist, uint32_t *d_cost,
                               hmx_pred_choice *d_best);
/* The same in a weighted slice (TComPrediction.cpp:421-432, :516-535): wp = ONE hmx_mc_wp with the meaning
 * hmx_batch_motionCompensation_wp_multi gives it, luma rows only.  Every used list goes to the 14-bit intermediate; one list is
 * weighted uni-directionally, two lists bi-directionally.  The distortion stays unweighted.  wp == NULL, or both tables NULL, is
 * the unweighted entry.  Also HMX_ERR_ARG: what hmx_batch_motionCompensation_wp_multi refuses for its tables.  Longest list: as
 * hmx_batch_inter_pred_error (the weights travel as a kernel argument). */
int hmx_batch_inter_pred_error_wp(hmx_ctx *ctx, const hmx_pu *cands, const uint32_t *bits, int n, const uint32_t *group_first,
                                  int n_groups, const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w, int pic_h,
                                  int margin_x, int margin_y, uint32_t lambda, int use_had, uint32_t *d_dist, uint32_t *d_cost,
                                  hmx_pred_choice *d_best, const hmx_mc_wp *wp);
/* xGetInterPredictionError for ONE unit with host pointers, as hmx_motionCompensation[_wp] takes them: ref0 / ref1 HOST planes
 * (NULL = list unused), (x, y, w, h) the unit, org the original block at the unit's first sample; wp0 / wp1 both NULL =
 * unweighted, else the entry of every used list.  A batch of one through the same kernel; *err = the distortion. */
int hmx_getInterPredictionError(hmx_ctx *ctx, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x,
                                int y, int w, int h, const hmx_pel *org, int org_stride, int use_had, const hmx_wp *wp0,
                                const hmx_wp *wp1, uint32_t *err);
/* Host helpers, no context.  TEncSearch::xGetMvpIdxBits (TEncSearch.cpp:3928-3952), 0 <= idx < num. */
uint32_t hmx_mvpIdxBits(int idx, int num);
/* uiBitsCand of xMergeEstimation (:3133-3137): cand + 1, less 1 for cand == max_signaled - 1 (MRG_MAX_NUM_CANDS_SIGNALED). */
uint32_t hmx_mergeIdxBits(int cand, int max_signaled);
/* TEncSearch::xCheckBestMVP (:4012-4055): (mvx, mvy) the found vector, mvp_cands the AMVP list as n_cands {hor, ver} pairs
 * (n_cands <= AMVP_MAX_NUM_CANDS = 2), *mvp_idx the predictor the search ran with.  n_cands < 2 changes nothing.  Otherwise the
 * candidate with strictly fewer bits -- hmx_mvBits(mv, candidate, 0) + hmx_mvpIdxBits(i, 2) -- replaces it, first such in order,
 * and *bits / *cost are updated as :4051-4053 (uint32_t, wrapping; getCost(UInt) with lambda).  HMX_ERR_ARG: a NULL pointer,
 * n_cands outside 0..2, *mvp_idx outside the list. */
int hmx_checkBestMVP(uint32_t lambda, int mvx, int mvy, const int16_t *mvp_cands, int n_cands, int *mvp_idx, uint32_t *bits,
                     uint32_t *cost);
int hmx_batch_residual_transformNxN_multi(hmx_ctx *ctx, const hmx_tu_list *list, int n_pics, const hmx_pic *org,
                                          const hmx_pic *pred, const hmx_levels *lev, uint32_t *d_abs_sum,
                                          const hmx_pic_param *pp);
/* The encoder's inter block chain in one pass per block (xEstimateResidualQT's transformNxN followed by
 * invtransformNxN and TComYuv::addClip, TLibEncoder/TEncSearch.cpp:4890-4990): residual org - pred, T, Q
 * (levels out), IQ, IT, rec = Clip(pred + resi).  Same results as hmx_batch_residual_transformNxN_multi
 * followed by hmx_batch_invtransformNxN_multi. */
int hmx_batch_residual_transform_recon_multi(hmx_ctx *ctx, const hmx_tu_list *list, int n_pics, const hmx_pic *org,
                                             const hmx_pic *pred, const hmx_levels *lev, const hmx_pic *rec,
                                             uint32_t *d_abs_sum, const hmx_pic_param *pp);
/* The same with the distortion the encoder takes right behind it (getDistPart(rec, org, DF_SSE), TEncSearch.cpp:4990 ->
 * TComRdCost::xGetSSE*, TComRdCost.cpp:1313-1657): d_sse[picture * blocks + i] = sum of (org - rec)^2 >> 2 * (B - 8) over
 * block i (the caller's order, like d_abs_sum; device, may be NULL), formed in the pass that reconstructs the block. */
int hmx_batch_residual_transform_recon_sse_multi(hmx_ctx *ctx, const hmx_tu_list *list, int n_pics, const hmx_pic *org,
                                                 const hmx_pic *pred, const hmx_levels *lev, const hmx_pic *rec,
                                                 uint32_t *d_abs_sum, uint32_t *d_sse, const hmx_pic_param *pp);
int hmx_batch_invtransformNxN_multi(hmx_ctx *ctx, const hmx_tu_list *list, int n_pics, const hmx_levels *lev,
                                    const hmx_pic *pred, const hmx_pic *out, const hmx_pic_param *pp);
int hmx_pic_extend_border_multi(hmx_ctx *ctx, int n_pics, const hmx_pic *pics, int pic_w, int pic_h, int margin_x,
                                int margin_y);
/* TComPicYuv::extendPicBorder (TLibCommon/TComPicYuv.cpp:248-286); margins in luma samples */
int hmx_pic_extend_border(hmx_ctx *ctx, const hmx_pic *pic, int pic_w, int pic_h, int margin_x, int margin_y);
/* TComDataCU::clipMv (TLibCommon/TComDataCU.cpp:3505-3517), host helper */
void hmx_clipMv(int *mvx, int *mvy, int cu_x, int cu_y, int pic_w, int pic_h, int ctu_size);

#ifdef __cplusplus
}
#endif
#endif
