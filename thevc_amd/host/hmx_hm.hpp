// hmx_hm.hpp -- C++ host mirror of the reference's block-kernel classes over the C-ABI (include/hmx.h).
//
// Same member names, argument order and meaning as the reference (HM: TLibCommon/TComTrQuant.h,
// TComPrediction.h, TComPattern.h, TComInterpolationFilter.h), so TEncSearch / TEncCu / TDecCu call
// sites keep their shape.  What the reference reads through TComDataCU / TComSlice / globals is
// explicit state here (setBlockState(), the context).  Every call goes to libhmx (HIP); nothing is
// computed on the host.  Errors: the reference returns Void and asserts; these wrappers throw.
#pragma once
#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "hmx.h"

namespace hmx_hm {

typedef short Pel;
typedef int TCoeff;
typedef int Int;
typedef unsigned UInt;
typedef bool Bool;
typedef double Double;
enum TextType { TEXT_LUMA = 0, TEXT_CHROMA = 1, TEXT_CHROMA_U = 2, TEXT_CHROMA_V = 3 };
static const UInt REG_DCT = 65535;

class Context { // replaces g_uiBitDepth / g_uiBitIncrement / g_uiIBDI_MAX (TComRom.cpp:445-448)
public:
  explicit Context(int bitDepth, int device = 0, int ctuSize = 64) {
    hmx_config cfg = {bitDepth, device, nullptr, ctuSize};
    if (hmx_create(&cfg, &m_ctx) != HMX_OK) throw std::runtime_error("hmx_create failed (no HIP device or bad config)");
    m_bitDepth = bitDepth;
  }
  ~Context() { hmx_destroy(m_ctx); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  hmx_ctx *get() const { return m_ctx; }
  int bitDepth() const { return m_bitDepth; }
  void check(int rc, const char *what) const {
    if (rc != HMX_OK) throw std::runtime_error(std::string(what) + ": " + hmx_last_error(m_ctx));
  }

private:
  hmx_ctx *m_ctx = nullptr;
  int m_bitDepth = 8;
};

// TComTrQuant (TComTrQuant.h:115-316)
class TComTrQuant {
public:
  explicit TComTrQuant(Context &c) : m_c(c) {
    m_qp.qp = hmx_setQPforQuant(0, HMX_TEXT_LUMA, 0, 0);
    m_qp.per_base = -1;
    m_qp.slice_type = HMX_I_SLICE;
    m_qp.sign_hide = 1;
    m_qp.is_intra = 1;
    m_qp.dir_mode = 1;
  }
  // setQPforQuant (TComTrQuant.cpp:192): same arguments; the result is kept like m_cQP
  void setQPforQuant(Int qpy, TextType eTxtType, Int qpBdOffset, Int chromaQPOffset) {
    m_qp.qp = hmx_setQPforQuant(qpy, eTxtType, qpBdOffset, chromaQPOffset);
  }
  // what xQuant reads through pcCU / the slice / the PPS (TComTrQuant.cpp:1121-1267)
  void setBlockState(Bool isIntra, UInt dirMode, Int sliceType, Bool signHideFlag, Int sliceQpBasePer = -1) {
    m_qp.is_intra = isIntra;
    m_qp.dir_mode = (int)dirMode;
    m_qp.slice_type = sliceType;
    m_qp.sign_hide = signHideFlag;
    m_qp.per_base = sliceQpBasePer;
  }
  // transformNxN (TComTrQuant.cpp:1373); pcCU is replaced by setBlockState()
  void transformNxN(Pel *pcResidual, UInt uiStride, TCoeff *rpcCoeff, UInt uiWidth, UInt uiHeight, UInt &uiAbsSum,
                    TextType eTType, Bool useTransformSkip = false, Bool transQuantBypass = false) {
    uint32_t s = 0;
    m_c.check(hmx_transformNxN(m_c.get(), pcResidual, uiStride, rpcCoeff, uiWidth, uiHeight, &s, eTType, &m_qp,
                               useTransformSkip, transQuantBypass),
              "transformNxN");
    uiAbsSum = s;
  }
  // invtransformNxN (TComTrQuant.cpp:1428); scalingListType is accepted and ignored (lists are off)
  void invtransformNxN(Bool transQuantBypass, TextType eText, UInt uiMode, Pel *rpcResidual, UInt uiStride,
                       TCoeff *pcCoeff, UInt uiWidth, UInt uiHeight, Int /*scalingListType*/,
                       Bool useTransformSkip = false) {
    m_c.check(hmx_invtransformNxN(m_c.get(), transQuantBypass, eText, uiMode, rpcResidual, uiStride, pcCoeff, uiWidth,
                                  uiHeight, &m_qp.qp, useTransformSkip),
              "invtransformNxN");
  }
  // invRecurTransformNxN (TComTrQuant.cpp:1452-1529): the walk over the transform quadtree of an inter CU.
  // What the reference asks pcCU becomes a view over the per-partition arrays TComDataCU stores (one entry per
  // 4x4 luma partition in z-order): transform index, coded-block flags of THIS texture, transform-skip flags.
  struct CuTransformTree {
    const unsigned char *trIdx;         // getTransformIdx
    const unsigned char *cbf;           // getCbf(eTxt): bit d = flag at transform depth d
    const unsigned char *transformSkip; // getTransformSkip(eTxt), may be null
    UInt cuDepth;                       // getDepth
    UInt maxCuWidth;                    // SPS getMaxCUWidth (64)
    UInt numPartInLCU;                  // getPic()->getNumPartInCU() (256 for a 64x64 LCU of 4x4 partitions)
    UInt totalNumPart;                  // getTotalNumPart(): partitions of this CU
    Bool transquantBypass;
  };
  void invRecurTransformNxN(const CuTransformTree &cu, UInt uiAbsPartIdx, TextType eTxt, Pel *rpcResidual, UInt uiAddr,
                            UInt uiStride, UInt uiWidth, UInt uiHeight, UInt uiMaxTrMode, UInt uiTrMode, TCoeff *rpcCoeff) {
    if (!((cu.cbf[uiAbsPartIdx] >> uiTrMode) & 1)) return; // nothing coded below this node
    if (uiTrMode == cu.trIdx[uiAbsPartIdx]) {               // a leaf (convertTransIdx is the identity, TComDataCU.cpp:3520)
      const UInt depth = cu.cuDepth + uiTrMode;
      if (eTxt != TEXT_LUMA && (cu.maxCuWidth >> depth) == 4) {
        // four 4x4 luma leaves share one 4x4 chroma block, carried by the first of them (:1467-1476)
        const UInt quarter = cu.numPartInLCU >> ((depth - 1) << 1);
        if (uiAbsPartIdx % quarter) return;
        uiWidth <<= 1;
        uiHeight <<= 1;
      }
      const Bool ts = cu.transformSkip && cu.transformSkip[uiAbsPartIdx];
      invtransformNxN(cu.transquantBypass, eTxt, HMX_REG_DCT, rpcResidual + uiAddr, uiStride, rpcCoeff, uiWidth, uiHeight, 0, ts);
      return;
    }
    const UInt half_w = uiWidth >> 1, half_h = uiHeight >> 1, parts = cu.totalNumPart >> ((uiTrMode + 1) << 1);
    for (UInt q = 0; q < 4; q++) // z-order: coefficients and partitions advance together
      invRecurTransformNxN(cu, uiAbsPartIdx + q * parts, eTxt, rpcResidual, uiAddr + (q & 1) * half_w + (q >> 1) * half_h * uiStride,
                           uiStride, half_w, half_h, uiMaxTrMode, uiTrMode + 1, rpcCoeff + q * half_w * half_h);
  }
  // private members of the reference, named by the north star
  void xT(UInt uiMode, Pel *piBlkResi, UInt uiStride, Int *psCoeff, Int iWidth, Int iHeight) {
    m_c.check(hmx_xT(m_c.get(), uiMode, piBlkResi, uiStride, psCoeff, iWidth, iHeight), "xT");
  }
  void xIT(UInt uiMode, Int *plCoef, Pel *pResidual, UInt uiStride, Int iWidth, Int iHeight) {
    m_c.check(hmx_xIT(m_c.get(), uiMode, plCoef, pResidual, uiStride, iWidth, iHeight), "xIT");
  }
  void xQuant(Int *pSrc, TCoeff *pDes, Int iWidth, Int iHeight, UInt &uiAcSum, TextType eTType) {
    uint32_t s = uiAcSum;
    m_c.check(hmx_xQuant(m_c.get(), pSrc, pDes, iWidth, iHeight, &s, eTType, &m_qp), "xQuant");
    uiAcSum = s;
  }
  void xDeQuant(const TCoeff *pSrc, Int *pDes, Int iWidth, Int iHeight, Int /*scalingListType*/) {
    m_c.check(hmx_xDeQuant(m_c.get(), pSrc, pDes, iWidth, iHeight, &m_qp.qp), "xDeQuant");
  }
  // xRateDistOptQuant (TComTrQuant.cpp:1719): m_pcEstBitsSbac and m_dLambda are members here too (setLambda,
  // TComTrQuant.h:155; the table is filled by the entropy coder's estBit); transform index and cbf context, which
  // the reference reads from pcCU, come through setRdoqBlockState()
  hmx_est_bits *m_pcEstBitsSbac = &m_estBits;
  void setLambda(Double dLambda) { m_dLambda = dLambda; }
  void setRdoqBlockState(Bool rootCbf, Int cbfCtx) {
    m_rootCbf = rootCbf;
    m_cbfCtx = cbfCtx;
  }
  void xRateDistOptQuant(Int *plSrcCoeff, TCoeff *piDstCoeff, UInt uiWidth, UInt uiHeight, UInt &uiAbsSum, TextType eTType) {
    hmx_rdoq_param rp{m_qp.qp, m_qp.sign_hide, m_qp.is_intra, m_qp.dir_mode, m_rootCbf, m_cbfCtx, m_dLambda};
    uint32_t s = uiAbsSum;
    m_c.check(hmx_xRateDistOptQuant(m_c.get(), plSrcCoeff, piDstCoeff, (int)uiWidth, (int)uiHeight, &s, eTType, &rp, m_pcEstBitsSbac),
              "xRateDistOptQuant");
    uiAbsSum = s;
  }
  const hmx_qp &qp() const { return m_qp.qp; }

private:
  Context &m_c;
  hmx_quant_param m_qp;
  hmx_est_bits m_estBits{};
  Double m_dLambda = 1.0;
  int m_rootCbf = 0, m_cbfCtx = 0;
};

// TComPattern + TComPrediction, intra part (TComPattern.cpp:213-366, TComPrediction.cpp:338-386)
class TComPrediction {
public:
  explicit TComPrediction(Context &c) : m_c(c) {}
  // initAdiPattern: the CU walk is replaced by the block geometry inside the reconstructed plane
  void initAdiPattern(const Pel *recPlane, Int stride, Int x, Int y, Int size, Bool chroma, Int picW, Int picH,
                      Int *piAdiBuf) {
    m_c.check(hmx_initAdiPattern(m_c.get(), recPlane, stride, x, y, size, chroma, picW, picH, piAdiBuf), "initAdiPattern");
  }
  void predIntraLumaAng(const Int *piAdiBuf, UInt uiDirMode, Pel *piPred, UInt uiStride, Int iWidth, Int iHeight) {
    m_c.check(hmx_predIntraLumaAng(m_c.get(), piAdiBuf, uiDirMode, piPred, uiStride, iWidth, iHeight), "predIntraLumaAng");
  }
  void predIntraChromaAng(const Int *piSrc, UInt uiDirMode, Pel *piPred, UInt uiStride, Int iWidth, Int iHeight) {
    m_c.check(hmx_predIntraChromaAng(m_c.get(), piSrc, uiDirMode, piPred, uiStride, iWidth, iHeight), "predIntraChromaAng");
  }
  // xPredInterLumaBlk / xPredInterChromaBlk (TComPrediction.cpp:554-642): refBlock = refPic->getLumaAddr(cuAddr, zorder + partAddr),
  // the TComMv as its two components, dst = dstPic->getLumaAddr(partAddr) with dstPic's stride
  void xPredInterLumaBlk(const Pel *refBlock, Int refStride, Int mvHor, Int mvVer, Int width, Int height, Pel *dst, Int dstStride, Bool bi) {
    m_c.check(hmx_xPredInterLumaBlk(m_c.get(), refBlock, refStride, mvHor, mvVer, width, height, dst, dstStride, bi), "xPredInterLumaBlk");
  }
  void xPredInterChromaBlk(const Pel *refBlock, Int refStride, Int mvHor, Int mvVer, Int width, Int height, Pel *dst, Int dstStride, Bool bi) {
    m_c.check(hmx_xPredInterChromaBlk(m_c.get(), refBlock, refStride, mvHor, mvVer, width, height, dst, dstStride, bi), "xPredInterChromaBlk");
  }
  // motionCompensation (TComPrediction.cpp:410-552) of one prediction unit: the reference pictures of the two lists (NULL = unused),
  // their vectors, the unit's luma rectangle, the prediction planes at the unit's first sample
  void motionCompensation(const hmx_pic *ref0, const Int mv0[2], const hmx_pic *ref1, const Int mv1[2], Int x, Int y, Int width, Int height,
                          const hmx_pic *pred) {
    m_c.check(hmx_motionCompensation(m_c.get(), ref0, mv0, ref1, mv1, x, y, width, height, pred), "motionCompensation");
  }

  // motionCompensation under getUseWP() / getWPBiPred() (TComPrediction.cpp:421-432, :516-535): the same with the table entries of
  // the two references used (what TComSlice::getWpScaling returns for (list, refIdx)); NULL where the list is unused
  void motionCompensation(const hmx_pic *ref0, const Int mv0[2], const hmx_pic *ref1, const Int mv1[2], Int x, Int y, Int width, Int height,
                          const hmx_pic *pred, const hmx_wp *wp0, const hmx_wp *wp1) {
    m_c.check(hmx_motionCompensation_wp(m_c.get(), ref0, mv0, ref1, mv1, x, y, width, height, pred, wp0, wp1), "motionCompensation (weighted)");
  }

private:
  Context &m_c;
};

// wpScalingParam (TComSlice.h): the coded fields, then the ones getWpScaling derives
struct wpScalingParam {
  Bool bPresentFlag;
  UInt uiLog2WeightDenom;
  Int iWeight, iOffset;
  Int w, o, offset, shift, round;
};
// TComWeightPrediction (TComWeightPrediction.h:49-89).  What the reference reads through pcCU->getSlice() is passed in: the
// wpScalingParam[3] rows of the references used.  TComYuv arguments become the three planes of a hmx_pic at the unit's first sample
// (14-bit intermediates in, samples out; host memory).
class TComWeightPrediction {
public:
  explicit TComWeightPrediction(Context &c) : m_c(c) {}
  // getWpScaling (:251-313): wp0 / wp1 = the rows of (list 0, iRefIdx0) / (list 1, iRefIdx1), NULL = list unused; fills w, o, offset,
  // shift, round.  (The reference keeps 1 << log2Denom in `round` for two lists and recomputes it from shift in addWeightBi.)
  void getWpScaling(wpScalingParam *wp0, wpScalingParam *wp1) {
    const int ibdi = m_c.bitDepth();
    if (wp0 && wp1) {
      for (int yuv = 0; yuv < 3; yuv++) {
        wp0[yuv].w = wp0[yuv].iWeight;
        wp0[yuv].o = wp0[yuv].iOffset * (1 << (ibdi - 8));
        wp1[yuv].w = wp1[yuv].iWeight;
        wp1[yuv].o = wp1[yuv].iOffset * (1 << (ibdi - 8));
        wp0[yuv].offset = wp1[yuv].offset = wp0[yuv].o + wp1[yuv].o;
        wp0[yuv].shift = wp1[yuv].shift = (Int)wp0[yuv].uiLog2WeightDenom + 1;
        wp0[yuv].round = wp1[yuv].round = 1 << wp0[yuv].uiLog2WeightDenom;
      }
    } else if (wpScalingParam *pwp = wp0 ? wp0 : wp1) {
      for (int yuv = 0; yuv < 3; yuv++) {
        pwp[yuv].w = pwp[yuv].iWeight;
        pwp[yuv].offset = pwp[yuv].iOffset * (1 << (ibdi - 8));
        pwp[yuv].shift = (Int)pwp[yuv].uiLog2WeightDenom;
        pwp[yuv].round = pwp[yuv].uiLog2WeightDenom >= 1 ? 1 << (pwp[yuv].uiLog2WeightDenom - 1) : 0;
      }
    }
  }
  // addWeightUni (:161-237): iWidth x iHeight luma samples, chroma at half size
  void addWeightUni(const hmx_pic *pcYuvSrc0, UInt iWidth, UInt iHeight, const wpScalingParam *wp0, const hmx_pic *rpcYuvDst) {
    for (int yuv = 0; yuv < 3; yuv++) {
      const int s = yuv ? 1 : 0;
      m_c.check(hmx_addWeightUni(m_c.get(), pcYuvSrc0->plane[yuv], pcYuvSrc0->stride[yuv], rpcYuvDst->plane[yuv], rpcYuvDst->stride[yuv],
                                 (int)iWidth >> s, (int)iHeight >> s, wp0[yuv].iWeight, wp0[yuv].iOffset, (int)wp0[yuv].uiLog2WeightDenom),
                "addWeightUni");
    }
  }
  // addWeightBi (:61-150)
  void addWeightBi(const hmx_pic *pcYuvSrc0, const hmx_pic *pcYuvSrc1, UInt iWidth, UInt iHeight, const wpScalingParam *wp0,
                   const wpScalingParam *wp1, const hmx_pic *rpcYuvDst) {
    for (int yuv = 0; yuv < 3; yuv++) {
      const int s = yuv ? 1 : 0;
      m_c.check(hmx_addWeightBi(m_c.get(), pcYuvSrc0->plane[yuv], pcYuvSrc0->stride[yuv], pcYuvSrc1->plane[yuv], pcYuvSrc1->stride[yuv],
                                rpcYuvDst->plane[yuv], rpcYuvDst->stride[yuv], (int)iWidth >> s, (int)iHeight >> s, wp0[yuv].iWeight,
                                wp1[yuv].iWeight, wp0[yuv].iOffset, wp1[yuv].iOffset, (int)wp0[yuv].uiLog2WeightDenom),
                "addWeightBi");
    }
  }
  // xWeightedPredictionUni (:366-386): pwp = the row of (eRefPicList, iRefIdx)
  void xWeightedPredictionUni(const hmx_pic *pcYuvSrc, Int iWidth, Int iHeight, wpScalingParam *pwp, const hmx_pic *rpcYuvPred) {
    getWpScaling(pwp, nullptr);
    addWeightUni(pcYuvSrc, iWidth, iHeight, pwp, rpcYuvPred);
  }
  // xWeightedPredictionBi (:327-352): a NULL row = that list unused (iRefIdx < 0)
  void xWeightedPredictionBi(const hmx_pic *pcYuvSrc0, const hmx_pic *pcYuvSrc1, wpScalingParam *pwp0, wpScalingParam *pwp1, Int iWidth,
                             Int iHeight, const hmx_pic *rpcYuvDst) {
    if (!pwp0 && !pwp1) throw std::runtime_error("xWeightedPredictionBi: no list");
    getWpScaling(pwp0, pwp1);
    if (pwp0 && pwp1) addWeightBi(pcYuvSrc0, pcYuvSrc1, iWidth, iHeight, pwp0, pwp1, rpcYuvDst);
    else if (pwp0) addWeightUni(pcYuvSrc0, iWidth, iHeight, pwp0, rpcYuvDst);
    else addWeightUni(pcYuvSrc1, iWidth, iHeight, pwp1, rpcYuvDst);
  }
  // the hmx_wp of a row, for TComPrediction::motionCompensation's weighted overload and hmx_mc_wp tables
  static hmx_wp entry(const wpScalingParam *wp) {
    hmx_wp e{};
    for (int yuv = 0; yuv < 3; yuv++) {
      e.weight[yuv] = (int16_t)wp[yuv].iWeight;
      e.offset[yuv] = (int16_t)wp[yuv].iOffset;
      e.log2_denom[yuv] = (uint8_t)wp[yuv].uiLog2WeightDenom;
    }
    return e;
  }

private:
  Context &m_c;
};

// TComRdCost: the two distortion entry points next to the path (TComRdCost.cpp:404-478), SAD, and the motion-vector cost the
// searches add to a distortion (TComRdCost.h:183-211; TComMv is a pair of Int here)
class TComRdCost {
public:
  explicit TComRdCost(Context &c) : m_c(c) {}
  // setLambda (TComRdCost.cpp:167-173), the two integer multipliers only
  void setLambda(Double dLambda) {
    m_uiLambdaMotionSAD = (UInt)std::floor(65536.0 * std::sqrt(dLambda));
    m_uiLambdaMotionSSE = (UInt)std::floor(65536.0 * dLambda);
  }
  void getMotionCost(Bool bSad, Int iAdd) { m_uiCost = (bSad ? m_uiLambdaMotionSAD + iAdd : m_uiLambdaMotionSSE + iAdd); }
  void setPredictor(Int iHor, Int iVer) { m_iPredHor = iHor, m_iPredVer = iVer; } // quarter samples
  void setCostScale(Int iCostScale) { m_iCostScale = iCostScale; }
  UInt getCost(Int x, Int y) const { return hmx_mvCost(m_uiCost, x, y, m_iPredHor, m_iPredVer, m_iCostScale); }
  UInt getCost(UInt b) const { return (m_uiCost * b) >> 16; }
  UInt getBits(Int x, Int y) const { return hmx_mvBits(x, y, m_iPredHor, m_iPredVer, m_iCostScale); }
  UInt motionCostMultiplier() const { return m_uiCost; }
  UInt lambdaMotionSAD() const { return m_uiLambdaMotionSAD; } // what calcRdCost(..., DF_SAD) multiplies with (TComRdCost.cpp:70)
  Int predictorHor() const { return m_iPredHor; }
  Int predictorVer() const { return m_iPredVer; }
  // xGetSAD4..64 with DistParam::iSubShift (TComRdCost.cpp:518-...), bApplyWeight false
  UInt getSAD(Pel *piOrg, Int iStrideOrg, Pel *piCur, Int iStrideCur, Int iCols, Int iRows, Int iSubShift = 0) {
    uint32_t v = 0;
    m_c.check(hmx_getSAD(m_c.get(), piCur, iStrideCur, piOrg, iStrideOrg, iCols, iRows, iSubShift, &v), "xGetSAD");
    return v;
  }
  UInt calcHAD(Pel *pi0, Int iStride0, Pel *pi1, Int iStride1, Int iWidth, Int iHeight) {
    uint32_t v = 0;
    m_c.check(hmx_calcHAD(m_c.get(), pi0, iStride0, pi1, iStride1, iWidth, iHeight, &v), "calcHAD");
    return v;
  }
  // getDistPart(..., bWeighted = false, DF_SSE)
  UInt getDistPart(Pel *piCur, Int iCurStride, Pel *piOrg, Int iOrgStride, UInt uiBlkWidth, UInt uiBlkHeight) {
    uint32_t v = 0;
    m_c.check(hmx_getSSE(m_c.get(), piCur, iCurStride, piOrg, iOrgStride, (int)uiBlkWidth, (int)uiBlkHeight, &v), "getDistPart");
    return v;
  }

private:
  Context &m_c;
  UInt m_uiLambdaMotionSAD = 0, m_uiLambdaMotionSSE = 0, m_uiCost = 0;
  Int m_iPredHor = 0, m_iPredVer = 0, m_iCostScale = 0;
};

// TComRdCostWeightPrediction (TComRdCostWeightPrediction.cpp:69-104, :490-561): the distortions xGetSAD* / xGetHADs return when
// DistParam::bApplyWeight is set.  wpCur: the luma row of the reference searched (what DistParam::wpCur[0] is after
// setWpScalingDistParam); iWeight, iOffset and uiLog2WeightDenom are read, the derived fields are the entry's own.
class TComRdCostWeightPrediction {
public:
  explicit TComRdCostWeightPrediction(Context &c) : m_c(c) {}
  // xGetSADw: every row, whatever DistParam::iSubShift says
  UInt xGetSADw(Pel *piOrg, Int iStrideOrg, Pel *piCur, Int iStrideCur, Int iCols, Int iRows, const wpScalingParam *wpCur) {
    uint32_t v = 0;
    m_c.check(hmx_getSADw(m_c.get(), piCur, iStrideCur, piOrg, iStrideOrg, iCols, iRows, wpCur->iWeight, wpCur->iOffset, (int)wpCur->uiLog2WeightDenom, &v),
              "xGetSADw");
    return v;
  }
  // xGetHADsw with iStep = 1
  UInt xGetHADsw(Pel *piOrg, Int iStrideOrg, Pel *piCur, Int iStrideCur, Int iCols, Int iRows, const wpScalingParam *wpCur) {
    uint32_t v = 0;
    m_c.check(hmx_getHADsw(m_c.get(), piCur, iStrideCur, piOrg, iStrideOrg, iCols, iRows, wpCur->iWeight, wpCur->iOffset, (int)wpCur->uiLog2WeightDenom, &v),
              "xGetHADsw");
    return v;
  }

private:
  Context &m_c;
};

// TComMvField (TComMotionInfo.h): a vector in quarter samples and a reference index, < 0 = the list is unused
struct TComMvField {
  Int mvHor = 0, mvVer = 0, refIdx = -1;
  void setMvField(Int hor, Int ver, Int idx) { mvHor = hor, mvVer = ver, refIdx = idx; }
};

// TEncSearch, xMotionEstimation (TEncSearch.cpp:4120-4514) for ONE unit: the integer stage over hmx_batch_fullpel_search_wp
// (xPatternSearch) or hmx_batch_tz_search_wp (xPatternSearchFast -> xTZSearch, m_iFastSearch = 1), the fractional stage over
// hmx_batch_subpel_search_wp -- each with the table setWpScalingDistParam left, or none: the unweighted call.
// What the reference reads through pcCU, the pattern key and the slice is explicit: the unit's position and size, the
// pictures (DEVICE pictures: the original, and the reference with its margins) and their geometry.
class TEncSearch {
public:
  struct Geometry {
    Int picWidth, picHeight, marginX, marginY, ctuSize;
  };
  TEncSearch(Context &c, TComRdCost &rd, const Geometry &g, Bool useFastEnc = false, Bool useHADME = true, Int iFastSearch = 0)
      : m_c(c), m_rd(rd), m_g(g), m_fastEnc(useFastEnc), m_useHADME(useHADME), m_iFastSearch(iFastSearch) {
    m_c.check(hmx_malloc(m_c.get(), sizeof(hmx_me_result), (void **)&m_dResult), "TEncSearch");
    m_c.check(hmx_malloc(m_c.get(), sizeof(hmx_subpel_result) + 18 * sizeof(uint32_t), (void **)&m_dFrac), "TEncSearch");
    m_c.check(hmx_malloc(m_c.get(), sizeof(PredOut), (void **)&m_dPred), "TEncSearch");
    for (Int iNum = 0; iNum < AMVP_MAX_NUM_CANDS + 1; iNum++) // :219-227
      for (Int iIdx = 0; iIdx < AMVP_MAX_NUM_CANDS; iIdx++) m_auiMVPIdxCost[iIdx][iNum] = iIdx < iNum ? xGetMvpIdxBits(iIdx, iNum) : (UInt)0x7FFFFFFF;
  }
  ~TEncSearch() {
    hmx_free(m_c.get(), m_dPred);
    hmx_free(m_c.get(), m_dResult);
    hmx_free(m_c.get(), m_dFrac);
  }
  TEncSearch(const TEncSearch &) = delete;
  TEncSearch &operator=(const TEncSearch &) = delete;
  // setWpScalingDistParam (:6183-6215), which xMotionEstimation runs before the integer stage (:4174) and whose result stays in
  // m_cDistParam for every distortion of the call.  Here the CALLER runs it before xMotionEstimation, with what the reference reads
  // through pcCU: wp = the wpScalingParam[3] row of (eRefPicListCur, iRefIdx) when the slice is weighted -- a P slice whose PPS has
  // getUseWP(), a B slice whose PPS has getWPBiPred() -- and NULL otherwise, as for iRefIdx < 0: bApplyWeight = false.  Only one
  // index is >= 0 in the reference's call, so the row is used as getWpScaling's uni-directional branch leaves it, also for bBi.
  void setWpScalingDistParam(const wpScalingParam *wp) {
    m_bApplyWeight = wp != nullptr;
    if (wp) m_wpCur = TComWeightPrediction::entry(wp);
  }
  // xSetSearchRange (:4209-4225): cMvPred in quarter samples, the corners in integer samples
  void xSetSearchRange(Int cuX, Int cuY, Int mvPredHor, Int mvPredVer, Int iSrchRng, Int rcMvSrchRngLT[2], Int rcMvSrchRngRB[2]) const {
    hmx_setSearchRange(mvPredHor, mvPredVer, iSrchRng, cuX, cuY, m_g.picWidth, m_g.picHeight, m_g.ctuSize, &rcMvSrchRngLT[0], &rcMvSrchRngLT[1],
                       &rcMvSrchRngRB[0], &rcMvSrchRngRB[1]);
  }
  // xPatternSearch (:4227-4283): the unit (x, y, iRoiWidth, iRoiHeight) of pcOrg against pcRef inside the box; rcMv (integer
  // samples) and ruiSAD as the reference leaves them.  The vector cost is the one m_pcRdCost holds: the caller has run
  // getMotionCost(1, 0), setPredictor and setCostScale(2) as xMotionEstimation does (:4169-4172).
  void xPatternSearch(const hmx_pic *pcOrg, const hmx_pic *pcRef, Int x, Int y, Int iRoiWidth, Int iRoiHeight, const Int pcMvSrchRngLT[2],
                      const Int pcMvSrchRngRB[2], Int rcMv[2], UInt &ruiSAD) {
    hmx_me_unit u{};
    u.x = (uint16_t)x, u.y = (uint16_t)y, u.w = (uint8_t)iRoiWidth, u.h = (uint8_t)iRoiHeight;
    u.ref = 0;
    u.sub_shift = (m_fastEnc && iRoiHeight > 8) ? 1 : 0; // :4245-4251
    u.pred_x = (int16_t)m_rd.predictorHor(), u.pred_y = (int16_t)m_rd.predictorVer();
    u.left = (int16_t)pcMvSrchRngLT[0], u.top = (int16_t)pcMvSrchRngLT[1], u.right = (int16_t)pcMvSrchRngRB[0], u.bottom = (int16_t)pcMvSrchRngRB[1];
    m_c.check(hmx_batch_fullpel_search_wp(m_c.get(), &u, 1, pcRef, 1, pcOrg, m_g.picWidth, m_g.picHeight, m_g.marginX, m_g.marginY,
                                          m_rd.motionCostMultiplier(), m_dResult, nullptr, wpCur()),
              "xPatternSearch");
    hmx_me_result r;
    m_c.check(hmx_download(m_c.get(), &r, m_dResult, sizeof(r)), "xPatternSearch");
    rcMv[0] = r.mvx, rcMv[1] = r.mvy;
    ruiSAD = r.sad;
  }
  // xTZSearch (:4302-4474) through xPatternSearchFast (:4285-4300), whose three neighbour predictors feed only
  // bTestOtherPredictedMV, which is compiled off.  rcMv: in the start vector in quarter samples (xMotionEstimation passes
  // *pcMvPred, :4182), which is clipped for the CU at (x, y) and >>= 2 as the reference does (:4312-4313); out the integer
  // vector.  iSearchRange: m_iSearchRange (m_aaiAdaptSR of the reference picture).  The vector cost is m_pcRdCost's, as for
  // xPatternSearch.  (cuX, cuY): the origin of the unit's CODING UNIT (getCUPelX / Y), which is what clipMv reads; it is the
  // unit's own position only for a first partition.
  void xTZSearch(const hmx_pic *pcOrg, const hmx_pic *pcRef, Int x, Int y, Int iRoiWidth, Int iRoiHeight, const Int pcMvSrchRngLT[2],
                 const Int pcMvSrchRngRB[2], Int iSearchRange, Int rcMv[2], UInt &ruiSAD) {
    xTZSearch(pcOrg, pcRef, x, y, x, y, iRoiWidth, iRoiHeight, pcMvSrchRngLT, pcMvSrchRngRB, iSearchRange, rcMv, ruiSAD);
  }
  void xTZSearch(const hmx_pic *pcOrg, const hmx_pic *pcRef, Int cuX, Int cuY, Int x, Int y, Int iRoiWidth, Int iRoiHeight, const Int pcMvSrchRngLT[2],
                 const Int pcMvSrchRngRB[2], Int iSearchRange, Int rcMv[2], UInt &ruiSAD) {
    hmx_me_unit u{};
    u.x = (uint16_t)x, u.y = (uint16_t)y, u.w = (uint8_t)iRoiWidth, u.h = (uint8_t)iRoiHeight;
    u.ref = 0;
    u.sub_shift = (m_fastEnc && iRoiHeight > 8) ? 1 : 0; // :323-330
    u.pred_x = (int16_t)m_rd.predictorHor(), u.pred_y = (int16_t)m_rd.predictorVer();
    u.left = (int16_t)pcMvSrchRngLT[0], u.top = (int16_t)pcMvSrchRngLT[1], u.right = (int16_t)pcMvSrchRngRB[0], u.bottom = (int16_t)pcMvSrchRngRB[1];
    int sx = rcMv[0], sy = rcMv[1];
    hmx_clipMv(&sx, &sy, cuX, cuY, m_g.picWidth, m_g.picHeight, m_g.ctuSize);
    hmx_tz_unit z{};
    z.start_x = (int16_t)(sx >> 2), z.start_y = (int16_t)(sy >> 2), z.range = (uint16_t)iSearchRange;
    m_c.check(hmx_batch_tz_search_wp(m_c.get(), &u, &z, 1, pcRef, 1, pcOrg, m_g.picWidth, m_g.picHeight, m_g.marginX, m_g.marginY,
                                     m_rd.motionCostMultiplier(), m_dResult, nullptr, nullptr, 0, wpCur()),
              "xTZSearch");
    hmx_me_result r;
    m_c.check(hmx_download(m_c.get(), &r, m_dResult, sizeof(r)), "xTZSearch");
    rcMv[0] = r.mvx, rcMv[1] = r.mvy;
    ruiSAD = r.sad;
  }
  // xPatternSearchFracDIF (:4476-4514): both stages of xPatternRefinement around pcMvInt (integer samples) in one device call
  // (getUseHADME() is the constructor's flag).  ruiCost = the winning quarter-stage cost.  The device returns the refined
  // vector; rcMvHalf and rcMvQter (each component -1..1), which the reference's caller only adds up again (:4198-4200), are
  // split from it with the half-stage costs: the half-sample winner is the first strictly smallest of the nine.  The vector
  // cost is m_pcRdCost's: getMotionCost(1, 0) and setPredictor as xMotionEstimation has left them (:4186); the cost scales
  // 1 and 0 of the two stages are the entry's own.
  void xPatternSearchFracDIF(const hmx_pic *pcOrg, const hmx_pic *pcRef, Int x, Int y, Int iRoiWidth, Int iRoiHeight, const Int pcMvInt[2],
                             Int rcMvHalf[2], Int rcMvQter[2], UInt &ruiCost) {
    hmx_me_unit u{};
    u.x = (uint16_t)x, u.y = (uint16_t)y, u.w = (uint8_t)iRoiWidth, u.h = (uint8_t)iRoiHeight;
    u.pred_x = (int16_t)m_rd.predictorHor(), u.pred_y = (int16_t)m_rd.predictorVer();
    u.left = u.right = (int16_t)pcMvInt[0], u.top = u.bottom = (int16_t)pcMvInt[1]; // the box of one vector: the host checks its window
    hmx_me_result in{};
    in.mvx = (int16_t)pcMvInt[0], in.mvy = (int16_t)pcMvInt[1];
    m_c.check(hmx_upload(m_c.get(), m_dResult, &in, sizeof(in)), "xPatternSearchFracDIF");
    uint32_t *dCosts = reinterpret_cast<uint32_t *>(m_dFrac + 1);
    m_c.check(hmx_batch_subpel_search_wp(m_c.get(), &u, 1, m_dResult, pcRef, 1, pcOrg, m_g.picWidth, m_g.picHeight, m_g.marginX, m_g.marginY,
                                         m_rd.motionCostMultiplier(), m_useHADME ? 1 : 0, m_dFrac, dCosts, wpCur()),
              "xPatternSearchFracDIF");
    struct {
      hmx_subpel_result r;
      uint32_t costs[18];
    } out;
    m_c.check(hmx_download(m_c.get(), &out, m_dFrac, sizeof(out)), "xPatternSearchFracDIF");
    static const Int refineH[9][2] = {{0, 0}, {0, -1}, {0, 1}, {-1, 0}, {1, 0}, {-1, -1}, {1, -1}, {-1, 1}, {1, 1}}; // s_acMvRefineH (:47-58)
    Int best = 0;
    for (Int i = 1; i < 9; i++)
      if (out.costs[i] < out.costs[best]) best = i;
    rcMvHalf[0] = refineH[best][0], rcMvHalf[1] = refineH[best][1];
    rcMvQter[0] = out.r.mvx - 4 * pcMvInt[0] - 2 * rcMvHalf[0], rcMvQter[1] = out.r.mvy - 4 * pcMvInt[1] - 2 * rcMvHalf[1];
    ruiCost = out.r.cost;
  }
  // xMotionEstimation (:4120-4206) against one reference picture: xSetSearchRange (around rcMv when bBi, :4166), the integer
  // stage, the fractional stage, then :4197-4205 on the host.  pcMvPred: the predictor, quarter samples.  rcMv: in (bBi only) the
  // vector the range is centred on, out the refined vector, both in quarter samples.  ruiBits: in the bits before the vector,
  // out with the vector's bits added.  bBi: the caller passes 2 * org - other prediction as pcOrg (removeHighFreq, :4147) and
  // the cost takes fWeight = 0.5 (:4148).  The integer stage is the full search when !m_iFastSearch || bBi, otherwise xTZSearch
  // from rcMv = *pcMvPred with the range iSrchRng (:4176-4184).  (cuX, cuY): the origin of the unit's coding unit, which
  // xSetSearchRange and xTZSearch clip against (pcCU->clipMv); the form without it is for a unit that is its CU's first
  // partition.  A second partition (2NxN, Nx2N, AMP) lies elsewhere, and near the picture border its box differs.
  void xMotionEstimation(const hmx_pic *pcOrg, const hmx_pic *pcRef, Int x, Int y, Int iRoiWidth, Int iRoiHeight, const Int pcMvPred[2], Int iSrchRng,
                         Bool bBi, Int rcMv[2], UInt &ruiBits, UInt &ruiCost) {
    xMotionEstimation(pcOrg, pcRef, x, y, x, y, iRoiWidth, iRoiHeight, pcMvPred, iSrchRng, bBi, rcMv, ruiBits, ruiCost);
  }
  void xMotionEstimation(const hmx_pic *pcOrg, const hmx_pic *pcRef, Int cuX, Int cuY, Int x, Int y, Int iRoiWidth, Int iRoiHeight, const Int pcMvPred[2],
                         Int iSrchRng, Bool bBi, Int rcMv[2], UInt &ruiBits, UInt &ruiCost) {
    const Double fWeight = bBi ? 0.5 : 1.0;
    Int lt[2], rb[2], mvInt[2], mvHalf[2], mvQter[2];
    if (bBi) xSetSearchRange(cuX, cuY, rcMv[0], rcMv[1], iSrchRng, lt, rb);
    else xSetSearchRange(cuX, cuY, pcMvPred[0], pcMvPred[1], iSrchRng, lt, rb);
    m_rd.getMotionCost(true, 0);
    m_rd.setPredictor(pcMvPred[0], pcMvPred[1]);
    m_rd.setCostScale(2);
    if (!m_iFastSearch || bBi) xPatternSearch(pcOrg, pcRef, x, y, iRoiWidth, iRoiHeight, lt, rb, mvInt, ruiCost);
    else {
      mvInt[0] = pcMvPred[0], mvInt[1] = pcMvPred[1];
      xTZSearch(pcOrg, pcRef, cuX, cuY, x, y, iRoiWidth, iRoiHeight, lt, rb, iSrchRng, mvInt, ruiCost);
    }
    m_rd.getMotionCost(true, 0);
    m_rd.setCostScale(1);
    xPatternSearchFracDIF(pcOrg, pcRef, x, y, iRoiWidth, iRoiHeight, mvInt, mvHalf, mvQter, ruiCost);
    m_rd.setCostScale(0);
    for (int k = 0; k < 2; k++) rcMv[k] = (mvInt[k] << 2) + (mvHalf[k] << 1) + mvQter[k];
    const UInt uiMvBits = m_rd.getBits(rcMv[0], rcMv[1]);
    ruiBits += uiMvBits;
    ruiCost = (UInt)(std::floor(fWeight * ((Double)ruiCost - (Double)m_rd.getCost(uiMvBits))) + (Double)m_rd.getCost(ruiBits));
  }

  // ---- complete candidates: xGetInterPredictionError and the loops around it, over hmx_batch_inter_pred_error_wp ----
  static const Int AMVP_MAX_NUM_CANDS = 2, MRG_MAX_NUM_CANDS = 5, MRG_MAX_NUM_CANDS_SIGNALED = 5;
  // What motionCompensation reads through the slice: per list, for every reference index, the picture (an entry of `refs`, DEVICE
  // pictures with margins, at most four) and its POC; whether the slice is B; and the weighted-prediction tables when the PPS has
  // getUseWP() (P slice: wpL0) / getWPBiPred() (B slice: wpL0 and wpL1), indexed like `refs` as hmx_mc_wp documents, else NULL.
  struct RefLists {
    const hmx_pic *refs;
    Int numRefs;
    const Int *entry[2]; // [list][refIdx] -> index into refs
    const Int *poc[2];   // [list][refIdx] -> getRefPic(list, refIdx)->getPOC()
    Bool isInterB;
    const hmx_wp *wpL0, *wpL1;
  };
  void setRefLists(const RefLists &r) { m_refs = r; }
  // xGetMvpIdxBits (:3928-3952)
  static UInt xGetMvpIdxBits(Int iIdx, Int iNum) { return hmx_mvpIdxBits(iIdx, iNum); }
  // xGetInterPredictionError (:3059-3081): motionCompensation(REF_PIC_LIST_X) of the unit with the motion in cMvField[2], then the
  // unweighted Hadamard (bHadamard) or SAD against the original.  (cuX, cuY): the origin of the unit's coding unit, which
  // xPredInterUni clips the vectors against (:487).
  void xGetInterPredictionError(const hmx_pic *pcOrg, Int cuX, Int cuY, Int x, Int y, Int iWidth, Int iHeight, const TComMvField cMvField[2],
                                UInt &ruiErr, Bool bHadamard) {
    hmx_pu u = candidate(cuX, cuY, x, y, iWidth, iHeight, cMvField);
    predError(pcOrg, &u, nullptr, 1, false, 0, bHadamard, sliceWp());
    ruiErr = m_out.dist[0];
  }
  // xRestrictBipredMergeCand (:3159-3172); isBipredRestriction: an 8x4 or 4x8 unit of an 8x8 coding unit
  static void xRestrictBipredMergeCand(Int iWidth, Int iHeight, TComMvField *mvFieldNeighbours, unsigned char *interDirNeighbours, Int numValidMergeCand) {
    if (iWidth + iHeight != 12) return;
    for (Int mergeCand = 0; mergeCand < numValidMergeCand; ++mergeCand)
      if (interDirNeighbours[mergeCand] == 3) {
        interDirNeighbours[mergeCand] = 1;
        mvFieldNeighbours[(mergeCand << 1) + 1].setMvField(0, 0, -1);
      }
  }
  // xMergeEstimation (:3096-3149) behind getInterMergeCandidates, which walks the CU tree and stays with the caller: the candidate
  // list (cMvFieldNeighbours[2 * cand + list], uhInterDirNeighbours, numValidMergeCand) comes in, is restricted for 8x4 / 4x8,
  // and ALL candidates are costed and compared in one device call.  uiInterDir, pacMvField and uiMergeIndex are written only
  // when a candidate's cost gets below MAX_UINT, as in the reference.
  void xMergeEstimation(const hmx_pic *pcOrg, Int cuX, Int cuY, Int x, Int y, Int iWidth, Int iHeight, UInt &uiInterDir, TComMvField pacMvField[2],
                        UInt &uiMergeIndex, UInt &ruiCost, TComMvField *cMvFieldNeighbours, unsigned char *uhInterDirNeighbours, Int numValidMergeCand) {
    xRestrictBipredMergeCand(iWidth, iHeight, cMvFieldNeighbours, uhInterDirNeighbours, numValidMergeCand);
    ruiCost = 0xFFFFFFFFu;
    if (numValidMergeCand <= 0) return;
    if (numValidMergeCand > MRG_MAX_NUM_CANDS) throw std::runtime_error("xMergeEstimation: more than MRG_MAX_NUM_CANDS candidates");
    hmx_pu u[MRG_MAX_NUM_CANDS];
    uint32_t bits[MRG_MAX_NUM_CANDS];
    for (Int c = 0; c < numValidMergeCand; c++) {
      u[c] = candidate(cuX, cuY, x, y, iWidth, iHeight, cMvFieldNeighbours + 2 * c);
      bits[c] = hmx_mergeIdxBits(c, MRG_MAX_NUM_CANDS_SIGNALED);
    }
    m_rd.getMotionCost(true, 0);
    predError(pcOrg, u, bits, numValidMergeCand, true, m_rd.motionCostMultiplier(), m_useHADME, sliceWp());
    if (m_out.best.index == 0xFFFFFFFFu) return;
    ruiCost = m_out.best.cost;
    uiMergeIndex = m_out.best.index;
    pacMvField[0] = cMvFieldNeighbours[0 + 2 * uiMergeIndex];
    pacMvField[1] = cMvFieldNeighbours[1 + 2 * uiMergeIndex];
    uiInterDir = uhInterDirNeighbours[uiMergeIndex];
  }
  // xGetTemplateCost (:4057-4118) as this reference compiles it (ZERO_MVD_EST 0): the candidate vector clipped, the luma
  // prediction from (eRefPicList, iRefIdx) -- weighted uni-directionally only in a P slice with getUseWP() (:4081-4093) --, the
  // SAD whatever UseHADME says (:4111-4115), and the bits through calcRdCost(..., DF_SAD): (Int)(bits * lambdaMotionSAD + .5) >> 16,
  // which is getCost(UInt) while the product stays below 2^31; a larger one is refused.
  UInt xGetTemplateCost(const hmx_pic *pcOrg, Int cuX, Int cuY, Int x, Int y, Int iSizeX, Int iSizeY, Int eRefPicList, Int iRefIdx, const Int cMvCand[2],
                        Int iMVPIdx, Int iMVPNum) {
    TComMvField f[2];
    f[eRefPicList].setMvField(cMvCand[0], cMvCand[1], iRefIdx);
    hmx_pu u = candidate(cuX, cuY, x, y, iSizeX, iSizeY, f);
    const uint32_t bits = templateBits(iMVPIdx, iMVPNum);
    predError(pcOrg, &u, &bits, 1, false, m_rd.lambdaMotionSAD(), false, templateWp());
    return m_out.cost[0];
  }
  // The candidate loop of xEstimateMvPredAMVP (:3893-3924) for AM_EXPL with an unfilled list: every candidate of pcAMVPInfo
  // (iN vectors of m_acMvCand) through xGetTemplateCost in ONE device call, then the reference's own comparison -- uiBestCost
  // starts at MAX_INT with iBestIdx = 0, so it is made here from the costs and not by the library, whose best starts at MAX_UINT.
  // rcMvPred / riMVPIdx: the winner; *puiDistBiP as the reference leaves it (untouched when no cost is below MAX_INT).
  void xEstimateMvPredAMVP(const hmx_pic *pcOrg, Int cuX, Int cuY, Int x, Int y, Int iRoiWidth, Int iRoiHeight, Int eRefPicList, Int iRefIdx,
                           const Int (*m_acMvCand)[2], Int iN, Int rcMvPred[2], Int &riMVPIdx, UInt *puiDistBiP) {
    if (iN < 1 || iN > AMVP_MAX_NUM_CANDS) throw std::runtime_error("xEstimateMvPredAMVP: 1 .. AMVP_MAX_NUM_CANDS candidates");
    hmx_pu u[AMVP_MAX_NUM_CANDS];
    uint32_t bits[AMVP_MAX_NUM_CANDS];
    for (Int i = 0; i < iN; i++) {
      TComMvField f[2];
      f[eRefPicList].setMvField(m_acMvCand[i][0], m_acMvCand[i][1], iRefIdx);
      u[i] = candidate(cuX, cuY, x, y, iRoiWidth, iRoiHeight, f);
      bits[i] = templateBits(i, AMVP_MAX_NUM_CANDS);
    }
    predError(pcOrg, u, bits, iN, false, m_rd.lambdaMotionSAD(), false, templateWp());
    UInt uiBestCost = 0x7FFFFFFF;
    Int iBestIdx = 0;
    for (Int i = 0; i < iN; i++)
      if (uiBestCost > m_out.cost[i]) {
        uiBestCost = m_out.cost[i];
        iBestIdx = i;
        *puiDistBiP = m_out.cost[i];
      }
    rcMvPred[0] = m_acMvCand[iBestIdx][0], rcMvPred[1] = m_acMvCand[iBestIdx][1];
    riMVPIdx = iBestIdx;
  }
  // xCheckBestMVP (:4012-4055): cMv the vector found, the AMVP list, rcMvPred / riMVPIdx the predictor the search ran with
  void xCheckBestMVP(const Int (*m_acMvCand)[2], Int iN, const Int cMv[2], Int rcMvPred[2], Int &riMVPIdx, UInt &ruiBits, UInt &ruiCost) {
    int16_t c[AMVP_MAX_NUM_CANDS][2];
    if (iN < 0 || iN > AMVP_MAX_NUM_CANDS) throw std::runtime_error("xCheckBestMVP: at most AMVP_MAX_NUM_CANDS candidates");
    for (Int i = 0; i < iN; i++) c[i][0] = (int16_t)m_acMvCand[i][0], c[i][1] = (int16_t)m_acMvCand[i][1];
    m_rd.getMotionCost(true, 0);
    m_rd.setCostScale(0);
    uint32_t b = ruiBits, k = ruiCost;
    if (hmx_checkBestMVP(m_rd.motionCostMultiplier(), cMv[0], cMv[1], &c[0][0], iN, &riMVPIdx, &b, &k) != HMX_OK)
      throw std::runtime_error("xCheckBestMVP: the predictor index lies outside the list");
    ruiBits = b, ruiCost = k;
    if (iN >= 2) rcMvPred[0] = m_acMvCand[riMVPIdx][0], rcMvPred[1] = m_acMvCand[riMVPIdx][1];
  }

private:
  const hmx_wp *wpCur() const { return m_bApplyWeight ? &m_wpCur : nullptr; } // the one-entry table of refs[0]
  struct PredOut {
    uint32_t dist[MRG_MAX_NUM_CANDS], cost[MRG_MAX_NUM_CANDS];
    hmx_pred_choice best;
  };
  // the tables motionCompensation(REF_PIC_LIST_X) weights with (TComPrediction.cpp:528-535), and xGetTemplateCost's (:4081-4093)
  hmx_mc_wp sliceWp() const { return hmx_mc_wp{m_refs.wpL0, m_refs.isInterB ? m_refs.wpL1 : nullptr}; }
  hmx_mc_wp templateWp() const { return hmx_mc_wp{m_refs.isInterB ? nullptr : m_refs.wpL0, nullptr}; }
  uint32_t templateBits(Int iMVPIdx, Int iMVPNum) const {
    const uint32_t bits = m_auiMVPIdxCost[iMVPIdx][iMVPNum];
    if ((unsigned long long)bits * m_rd.lambdaMotionSAD() >= (1ull << 31))
      throw std::runtime_error("xGetTemplateCost: lambda * bits reaches 2^31, where calcRdCost(DF_SAD) and getCost(UInt) part");
    return bits;
  }
  // One candidate in the library's form: the vectors clipped for the coding unit (xPredInterUni, :487), the lists mapped to refs[],
  // and the identical-motion shortcut (xCheckIdenticalMotion, :392-407: B slice without WPBiPred, both lists, equal POCs, equal
  // UNCLIPPED vectors) resolved to list 0 alone.
  hmx_pu candidate(Int cuX, Int cuY, Int x, Int y, Int w, Int h, const TComMvField f[2]) const {
    hmx_pu u{};
    u.x = (uint16_t)x, u.y = (uint16_t)y, u.w = (uint8_t)w, u.h = (uint8_t)h, u.ref0 = u.ref1 = 255;
    Bool use[2] = {f[0].refIdx >= 0, f[1].refIdx >= 0};
    if (use[0] && use[1] && m_refs.isInterB && !(m_refs.wpL0 || m_refs.wpL1) && m_refs.poc[0][f[0].refIdx] == m_refs.poc[1][f[1].refIdx] &&
        f[0].mvHor == f[1].mvHor && f[0].mvVer == f[1].mvVer)
      use[1] = false;
    for (Int l = 0; l < 2; l++) {
      if (!use[l]) continue;
      int mx = f[l].mvHor, my = f[l].mvVer;
      hmx_clipMv(&mx, &my, cuX, cuY, m_g.picWidth, m_g.picHeight, m_g.ctuSize);
      (l ? u.ref1 : u.ref0) = (uint8_t)m_refs.entry[l][f[l].refIdx];
      (l ? u.mv1x : u.mv0x) = (int16_t)mx, (l ? u.mv1y : u.mv0y) = (int16_t)my;
    }
    return u;
  }
  void predError(const hmx_pic *pcOrg, const hmx_pu *u, const uint32_t *bits, Int n, Bool decide, UInt lambda, Bool bHadamard, const hmx_mc_wp &wp) {
    const uint32_t first[2] = {0, (uint32_t)n};
    m_c.check(hmx_batch_inter_pred_error_wp(m_c.get(), u, bits, n, decide ? first : nullptr, decide ? 1 : 0, m_refs.refs, m_refs.numRefs, pcOrg,
                                            m_g.picWidth, m_g.picHeight, m_g.marginX, m_g.marginY, lambda, bHadamard ? 1 : 0, m_dPred->dist, m_dPred->cost,
                                            decide ? &m_dPred->best : nullptr, &wp),
              "xGetInterPredictionError");
    m_c.check(hmx_download(m_c.get(), &m_out, m_dPred, sizeof(m_out)), "xGetInterPredictionError");
  }
  RefLists m_refs{};
  UInt m_auiMVPIdxCost[AMVP_MAX_NUM_CANDS][AMVP_MAX_NUM_CANDS + 1];
  PredOut *m_dPred = nullptr;
  PredOut m_out{};
  Context &m_c;
  TComRdCost &m_rd;
  Geometry m_g;
  Bool m_bApplyWeight = false; // DistParam::bApplyWeight / wpCur
  hmx_wp m_wpCur{};
  Bool m_fastEnc, m_useHADME;
  Int m_iFastSearch; // 1: xTZSearch for uni-predictive units
  hmx_me_result *m_dResult = nullptr;
  hmx_subpel_result *m_dFrac = nullptr; // the result, then the 18 stage costs
};

// TComInterpolationFilter (TComInterpolationFilter.cpp:323-415): identical signatures
class TComInterpolationFilter {
public:
  explicit TComInterpolationFilter(Context &c) : m_c(c) {}
  void filterHorLuma(Pel *src, Int srcStride, short *dst, Int dstStride, Int width, Int height, Int frac, Bool isLast) {
    m_c.check(hmx_filterHorLuma(m_c.get(), src, srcStride, dst, dstStride, width, height, frac, isLast), "filterHorLuma");
  }
  void filterVerLuma(Pel *src, Int srcStride, short *dst, Int dstStride, Int width, Int height, Int frac, Bool isFirst,
                     Bool isLast) {
    m_c.check(hmx_filterVerLuma(m_c.get(), src, srcStride, dst, dstStride, width, height, frac, isFirst, isLast), "filterVerLuma");
  }
  void filterHorChroma(Pel *src, Int srcStride, short *dst, Int dstStride, Int width, Int height, Int frac, Bool isLast) {
    m_c.check(hmx_filterHorChroma(m_c.get(), src, srcStride, dst, dstStride, width, height, frac, isLast), "filterHorChroma");
  }
  void filterVerChroma(Pel *src, Int srcStride, short *dst, Int dstStride, Int width, Int height, Int frac, Bool isFirst,
                       Bool isLast) {
    m_c.check(hmx_filterVerChroma(m_c.get(), src, srcStride, dst, dstStride, width, height, frac, isFirst, isLast), "filterVerChroma");
  }

private:
  Context &m_c;
};

// TComSampleAdaptiveOffset, the application (TComSampleAdaptiveOffset.cpp:515-1240): SAOProcess for a whole picture on the
// device.  createPicSaoInfo (:491-505) decides m_bUseNIF per picture; here the caller sets the availability bytes of
// hmx_lf_border_avail (device, one per CTU) for a picture with a slice or tile boundary the filters may not cross, and
// processSaoCu's dispatch (:515-548) follows: with bytes set the block path (processSaoBlock), otherwise processSaoCuOrg.
class TComSampleAdaptiveOffset {
public:
  explicit TComSampleAdaptiveOffset(Context &c) : m_c(c) {}
  void createPicSaoInfo(const uint8_t *d_borderAvail) { m_dAvail = d_borderAvail, m_bUseNIF = d_borderAvail != nullptr; }
  void destroyPicSaoInfo() { m_dAvail = nullptr, m_bUseNIF = false; }
  // in (deblocked), out: device pictures; d_params (device): [component][CTU in raster order], merges resolved
  void SAOProcess(const hmx_pic *in, const hmx_pic *out, Int picWidth, Int picHeight, const hmx_sao_lcu *d_params, Int numLcu) {
    if (!m_bUseNIF) m_c.check(hmx_sao_picture(m_c.get(), in, out, picWidth, picHeight, d_params, numLcu), "SAOProcess");
    else m_c.check(hmx_sao_picture_multi_avail(m_c.get(), 1, in, out, picWidth, picHeight, d_params, numLcu, m_dAvail), "SAOProcess (NIF)");
  }

private:
  Context &m_c;
  const uint8_t *m_dAvail = nullptr;
  Bool m_bUseNIF = false;
};

// TEncSampleAdaptiveOffset, the statistics pass (TEncSampleAdaptiveOffset.cpp:859-1124, calcSaoStatsCuOrg with SAO_SKIP_RIGHT;
// :571-854, calcSaoStatsBlock, when m_bUseNIF): one call for every CTU and component of a picture, on the device; and the
// parameter search with SAOLcuBasedOptimization = 1, rdoSaoUnitAll (:1466-1799), on the bins where they lie.  A caller that
// runs a search of its own (the quadtree of SAOLcuBasedOptimization = 0) reads the downloaded bins through ctuStats.
typedef long long Int64;
class TEncSampleAdaptiveOffset {
public:
  explicit TEncSampleAdaptiveOffset(Context &c) : m_c(c) {}
  // as TComSampleAdaptiveOffset::createPicSaoInfo: the availability bytes of a picture on the NIF path, or nullptr
  void createPicSaoInfo(const uint8_t *d_borderAvail) { m_dAvail = d_borderAvail, m_bUseNIF = d_borderAvail != nullptr; }
  void destroyPicSaoInfo() { m_dAvail = nullptr, m_bUseNIF = false; }
  // org, rec (deblocked): device pictures; d_out (device): [component][CTU in raster order][HMX_SAO_STAT_BINS].  calcSaoStatsCu's
  // dispatch (:816-854): the block path skips no rows or columns, so lcuBasedOptimization plays no part in it
  void calcSaoStatsPicture(const hmx_pic *org, const hmx_pic *rec, Int picWidth, Int picHeight, Bool lcuBasedOptimization,
                           hmx_sao_stat *d_out) {
    if (!m_bUseNIF) m_c.check(hmx_sao_stats(m_c.get(), org, rec, picWidth, picHeight, lcuBasedOptimization ? 1 : 0, d_out), "calcSaoStatsPicture");
    else m_c.check(hmx_sao_stats_multi_avail(m_c.get(), 1, org, rec, picWidth, picHeight, m_dAvail, d_out), "calcSaoStatsPicture (NIF)");
  }
  // adds one CTU's downloaded bins to m_iOffsetOrg / m_iCount [SAO_EO_0..3, SAO_BO][MAX_NUM_SAO_CLASS] of that CTU, which
  // rdoSaoUnitAll clears before each CTU (the reference's calcSaoStatsCu accumulates the same way)
  static inline void ctuStats(const hmx_sao_stat *ctuBins, Int64 stats[5][33], Int64 count[5][33]) {
    for (int t = 0; t < 4; t++)
      for (int c = 0; c < 5; c++) stats[t][c] += ctuBins[5 * t + c].diff, count[t][c] += ctuBins[5 * t + c].count;
    for (int k = 1; k <= 32; k++) stats[4][k] += ctuBins[20 + k - 1].diff, count[4][k] += ctuBins[20 + k - 1].count;
  }
  // What rdoSaoUnitAll reads through m_pcPic and the coder startSaoEnc (:530-546) prepared: the slice type (or the table
  // resetEntropy substitutes, TEncSbac.cpp:117-121) and QP that initialise the two contexts, and the fractional bits the rate
  // coder holds at that moment (0 for a fresh coder).
  void startSaoEnc(Int sliceType, Int sliceQp, UInt fracBits = 0) {
    uint8_t st[2];
    m_c.check(hmx_sao_ctx_init(sliceType, sliceQp, st), "startSaoEnc");
    m_param.ctx_state[0] = st[0], m_param.ctx_state[1] = st[1], m_param.frac = fracBits;
  }
  // rdoSaoUnitAll (:1466-1799) for one picture, device to device: d_stats as calcSaoStatsPicture wrote them, d_units /
  // d_apply (may be nullptr) / d_result as hmx_sao_decide documents them; d_mergeAllow: the bytes of hmx_sao_merge_allow or
  // nullptr.  bSaoFlag comes from m_depthSaoRate (:1503-1513), which is updated from the downloaded counts (:1788-1789);
  // the flags and the result are returned through saoParam.
  struct SAOParam {
    Bool bSaoFlag[2];
    hmx_sao_result result;
  };
  void rdoSaoUnitAll(SAOParam *saoParam, const hmx_sao_stat *d_stats, Int picWidth, Int picHeight, Int numLcu, Double lambda,
                     Double lambdaChroma, Int depth, const uint8_t *d_mergeAllow, hmx_sao_unit *d_units, hmx_sao_lcu *d_apply,
                     hmx_sao_result *d_result) {
    m_c.check(hmx_sao_rate_flags(&m_depthSaoRate, depth, m_param.enable), "rdoSaoUnitAll (rate flags)");
    m_param.lambda_luma = lambda, m_param.lambda_chroma = lambdaChroma;
    m_c.check(hmx_sao_decide(m_c.get(), d_stats, picWidth, picHeight, &m_param, d_mergeAllow, d_units, d_apply, d_result), "rdoSaoUnitAll");
    m_c.check(hmx_download(m_c.get(), &saoParam->result, d_result, sizeof(hmx_sao_result)), "rdoSaoUnitAll (result)");
    saoParam->bSaoFlag[0] = m_param.enable[0] != 0, saoParam->bSaoFlag[1] = m_param.enable[1] != 0;
    m_c.check(hmx_sao_rate_update(&m_depthSaoRate, depth, saoParam->result.num_no_sao, numLcu), "rdoSaoUnitAll (rate update)");
  }

private:
  Context &m_c;
  const uint8_t *m_dAvail = nullptr;
  Bool m_bUseNIF = false;
  hmx_sao_rate_state m_depthSaoRate = {};
  hmx_sao_decide_param m_param = {};
};

// WeightPredAnalysis (TLibEncoder/WeightPredAnalysis.h, .cpp), the estimation of the explicit weights TEncSlice::compressSlice runs
// per slice (TEncSlice.cpp:688-711).  What the reference reads through TComSlice / TComPic is the WpSlice below: the slice's
// original and, per entry of its lists, the reference picture's reconstruction and the wpACDCParam of that picture's original
// (getRefPic(...)->getSlice(0)->getWpAcDcParam).  Pictures are device planes.  The sums over pictures run on the device
// (hmx_wp_acdc, hmx_wp_sad_multi); the arithmetic per row is libhmx's host code (hmx_wp_update_params, hmx_wp_select,
// hmx_wp_check_enable).  m_wp persists from slice to slice as in the reference: xCheckWPEnable counts every entry of it.
static const Int MAX_NUM_REF = 16; // CommonDef.h
struct wpACDCParam { // TComSlice.h
  Int64 iAC, iDC;
};
struct WpSlice {
  Bool isInterP = true;                    // TComSlice::isInterP
  Int numRefIdx[2] = {0, 0};               // getNumRefIdx
  const hmx_pic *picYuvOrg = nullptr;      // getPic()->getPicYuvOrg()
  Int width = 0, height = 0;
  wpACDCParam acdc[3] = {};                // getWpAcDcParam / setWpAcDcParam
  const hmx_pic *refPicYuvRec[2][MAX_NUM_REF] = {};   // getRefPic(list, idx)->getPicYuvRec()
  const wpACDCParam *refAcdc[2][MAX_NUM_REF] = {};    // getRefPic(list, idx)->getSlice(0)->getWpAcDcParam
  Bool useWP = true, wpBiPred = true;      // the PPS flags; xCheckWPEnable clears them
  wpScalingParam wpScaling[2][MAX_NUM_REF][3] = {}; // setWpScaling
};
class WeightPredAnalysis {
public:
  explicit WeightPredAnalysis(Context &c) : m_c(c) { // :47-65
    for (Int iList = 0; iList < 2; iList++)
      for (Int iRefIdx = 0; iRefIdx < MAX_NUM_REF; iRefIdx++)
        for (Int comp = 0; comp < 3; comp++) m_wp[iList][iRefIdx][comp] = wpScalingParam{false, 0, 1, 0, 0, 0, 0, 0, 0};
  }
  // :71-108
  Bool xCalcACDCParamSlice(WpSlice *slice) {
    hmx_wp_acdc_param *d = nullptr, h;
    m_c.check(hmx_malloc(m_c.get(), sizeof(h), (void **)&d), "xCalcACDCParamSlice");
    int rc = hmx_wp_acdc(m_c.get(), slice->picYuvOrg, slice->width, slice->height, d);
    if (rc == HMX_OK) rc = hmx_download(m_c.get(), &h, d, sizeof(h));
    hmx_free(m_c.get(), d);
    m_c.check(rc, "xCalcACDCParamSlice");
    for (Int comp = 0; comp < 3; comp++) slice->acdc[comp] = wpACDCParam{h.ac[comp], h.dc[comp]};
    return true;
  }
  // :176-245 with WP_PARAM_RANGE_LIMIT: the denominator loop over xUpdatingWPParameters, then xSelectWP
  Bool xEstimateWPParamSlice(WpSlice *slice) {
    const Int n[2] = {slice->numRefIdx[0], slice->isInterP ? 0 : slice->numRefIdx[1]};
    hmx_wp_acdc_param cur, refs[2][MAX_NUM_REF];
    hmx_wp rows[2][MAX_NUM_REF];
    uint8_t present[2][MAX_NUM_REF];
    pack(slice->acdc, &cur);
    for (Int l = 0; l < 2; l++)
      for (Int i = 0; i < n[l]; i++) pack(slice->refAcdc[l][i], &refs[l][i]);
    Int iDenom = 0;
    if (hmx_wp_update_params(&cur, refs[0], n[0], refs[1], n[1], m_c.bitDepth(), rows[0], rows[1], present[0], present[1], &iDenom) != HMX_OK)
      throw std::runtime_error("xEstimateWPParamSlice: hmx_wp_update_params refused its arguments");
    for (Int l = 0; l < 2; l++)
      for (Int i = 0; i < n[l]; i++)
        for (Int comp = 0; comp < 3; comp++)
          m_wp[l][i][comp] = wpScalingParam{true, rows[l][i].log2_denom[comp], rows[l][i].weight[comp], rows[l][i].offset[comp], 0, 0, 0, 0, 0};
    xSelectWP(slice, m_wp, iDenom);
    setWpScaling(slice);
    return true;
  }
  // :313-366: one launch for every (list, reference) of the slice.  hmx_wp_sad_multi refuses the weight 256 that :293 lets through
  // at denominator 7: the mirror throws there (hmx_wp_estimate_slices costs such a row).
  Bool xSelectWP(WpSlice *slice, wpScalingParam weightPredTable[2][MAX_NUM_REF][3], Int iDenom) {
    const Int n[2] = {slice->numRefIdx[0], slice->isInterP ? 0 : slice->numRefIdx[1]};
    hmx_wp_sad_job jobs[2 * MAX_NUM_REF];
    hmx_pic recs[2 * MAX_NUM_REF];
    Int nJobs = 0;
    for (Int l = 0; l < 2; l++)
      for (Int i = 0; i < n[l]; i++, nJobs++) {
        recs[nJobs] = *slice->refPicYuvRec[l][i];
        jobs[nJobs] = hmx_wp_sad_job{0u, (uint32_t)nJobs, row(weightPredTable[l][i])};
      }
    if (!nJobs) return true;
    int64_t *d = nullptr, sums[2 * MAX_NUM_REF][6];
    m_c.check(hmx_malloc(m_c.get(), sizeof(int64_t) * 6 * nJobs, (void **)&d), "xSelectWP");
    int rc = hmx_wp_sad_multi(m_c.get(), nJobs, jobs, slice->picYuvOrg, 1, recs, nJobs, slice->width, slice->height, d);
    if (rc == HMX_OK) rc = hmx_download(m_c.get(), sums, d, sizeof(int64_t) * 6 * nJobs);
    hmx_free(m_c.get(), d);
    m_c.check(rc, "xSelectWP");
    const Int64 nLuma = (Int64)slice->width * slice->height, nChroma = (Int64)(slice->width >> 1) * (slice->height >> 1);
    Int j = 0;
    for (Int l = 0; l < 2; l++)
      for (Int i = 0; i < n[l]; i++, j++) {
        hmx_wp r = jobs[j].wp;
        uint8_t present = 1;
        hmx_wp_select(sums[j], nLuma, nChroma, iDenom, &r, &present);
        for (Int comp = 0; comp < 3; comp++)
          weightPredTable[l][i][comp] = wpScalingParam{present != 0, r.log2_denom[comp], r.weight[comp], r.offset[comp], 0, 0, 0, 0, 0};
      }
    return true;
  }
  // :135-170
  void xCheckWPEnable(WpSlice *slice) {
    Int iPresentCnt = 0;
    for (Int iList = 0; iList < 2; iList++)
      for (Int iRefIdx = 0; iRefIdx < MAX_NUM_REF; iRefIdx++)
        for (Int iComp = 0; iComp < 3; iComp++) iPresentCnt += (Int)m_wp[iList][iRefIdx][iComp].bPresentFlag;
    if (iPresentCnt == 0) {
      slice->useWP = false, slice->wpBiPred = false;
      for (Int iList = 0; iList < 2; iList++)
        for (Int iRefIdx = 0; iRefIdx < MAX_NUM_REF; iRefIdx++)
          for (Int iComp = 0; iComp < 3; iComp++) m_wp[iList][iRefIdx][iComp] = wpScalingParam{false, 0, 1, 0, 0, 0, 0, 0, 0};
      setWpScaling(slice);
    }
  }

private:
  static void pack(const wpACDCParam *a, hmx_wp_acdc_param *o) {
    for (Int comp = 0; comp < 3; comp++) o->ac[comp] = a[comp].iAC, o->dc[comp] = a[comp].iDC;
  }
  static hmx_wp row(const wpScalingParam *w) {
    hmx_wp r{};
    for (Int comp = 0; comp < 3; comp++)
      r.weight[comp] = (int16_t)w[comp].iWeight, r.offset[comp] = (int16_t)w[comp].iOffset, r.log2_denom[comp] = (uint8_t)w[comp].uiLog2WeightDenom;
    return r;
  }
  void setWpScaling(WpSlice *slice) {
    for (Int l = 0; l < 2; l++)
      for (Int i = 0; i < MAX_NUM_REF; i++)
        for (Int comp = 0; comp < 3; comp++) slice->wpScaling[l][i][comp] = m_wp[l][i][comp];
  }
  Context &m_c;
  wpScalingParam m_wp[2][MAX_NUM_REF][3];
};

// Adaptive QP: TEncPic's layers (TLibEncoder/TEncPic.h, .cpp), TEncPreanalyzer::xPreanalyze (TEncPreanalyzer.cpp:64-139) and
// TEncCu::xComputeQP (TEncCu.cpp:1114-1136).  The picture is device planes; xPreanalyze is one hmx_aq_activity call and ONE
// download that fills the layers' host arrays, which xComputeQP then reads like the reference's (hmx_aq_compute_qp).
class TEncPicQPAdaptationLayer {
public:
  UInt getAQPartWidth() const { return m_uiAQPartWidth; }
  UInt getAQPartHeight() const { return m_uiAQPartHeight; }
  UInt getNumAQPartInWidth() const { return m_uiNumAQPartInWidth; }
  UInt getNumAQPartInHeight() const { return m_uiNumAQPartInHeight; }
  UInt getAQPartStride() const { return m_uiNumAQPartInWidth; }
  const Double *getQPAdaptationUnit() const { return m_acTEncAQU; } // the units' activities (TEncQPAdaptationUnit::getActivity), row-major
  Double getAvgActivity() const { return m_dAvgActivity; }

private:
  friend class TEncPic;
  friend class TEncPreanalyzer;
  UInt m_uiAQPartWidth = 0, m_uiAQPartHeight = 0, m_uiNumAQPartInWidth = 0, m_uiNumAQPartInHeight = 0;
  const Double *m_acTEncAQU = nullptr;
  Double m_dAvgActivity = 0.0;
};
class TEncPic {
public:
  // TEncPic::create (TEncPic.cpp:128-139); uiMaxAQDepth = MaxCuDQPDepth + 1 (TEncTop.cpp:440)
  void create(const hmx_pic *picYuvOrg, Int iWidth, Int iHeight, UInt uiMaxWidth, UInt uiMaxAQDepth) {
    if (hmx_aq_layout(iWidth, iHeight, (int)uiMaxWidth, (int)uiMaxAQDepth, &m_geom) != HMX_OK)
      throw std::runtime_error("TEncPic::create: picture size, CTU size or AQ depth outside hmx_aq_layout's domain");
    m_picYuvOrg = picYuvOrg;
    m_act.assign((size_t)m_geom.total + (size_t)m_geom.depths, 0.0);
    for (Int d = 0; d < m_geom.depths; d++) {
      TEncPicQPAdaptationLayer &l = m_acAQLayer[d];
      l.m_uiAQPartWidth = l.m_uiAQPartHeight = (UInt)m_geom.part[d];
      l.m_uiNumAQPartInWidth = (UInt)m_geom.nx[d], l.m_uiNumAQPartInHeight = (UInt)m_geom.ny[d];
      l.m_acTEncAQU = m_act.data() + m_geom.first[d];
    }
  }
  const hmx_pic *getPicYuvOrg() const { return m_picYuvOrg; }
  UInt getMaxAQDepth() const { return (UInt)m_geom.depths; }
  TEncPicQPAdaptationLayer *getAQLayer(UInt uiDepth) { return &m_acAQLayer[uiDepth]; }
  const hmx_aq_geom &geom() const { return m_geom; }

private:
  friend class TEncPreanalyzer;
  friend class TEncCu;
  const hmx_pic *m_picYuvOrg = nullptr;
  hmx_aq_geom m_geom = {};
  std::vector<Double> m_act; // the activities of all layers, then the layers' averages: what one download brings
  TEncPicQPAdaptationLayer m_acAQLayer[HMX_AQ_MAX_DEPTHS];
};
class TEncPreanalyzer {
public:
  explicit TEncPreanalyzer(Context &c) : m_c(c) {}
  void xPreanalyze(TEncPic *pcEPic) {
    const hmx_aq_geom &g = pcEPic->m_geom;
    const size_t n = (size_t)g.total + (size_t)g.depths;
    Double *d = nullptr;
    m_c.check(hmx_malloc(m_c.get(), sizeof(Double) * n, (void **)&d), "xPreanalyze");
    int rc = hmx_aq_activity(m_c.get(), pcEPic->m_picYuvOrg, g.pic_w, g.pic_h, g.ctu, g.depths, d, d + g.total);
    if (rc == HMX_OK) rc = hmx_download(m_c.get(), pcEPic->m_act.data(), d, sizeof(Double) * n);
    hmx_free(m_c.get(), d);
    m_c.check(rc, "xPreanalyze");
    for (Int l = 0; l < g.depths; l++) pcEPic->m_acAQLayer[l].m_dAvgActivity = pcEPic->m_act[(size_t)g.total + (size_t)l];
  }

private:
  Context &m_c;
};
class TEncCu {
public:
  // what xComputeQP reads through m_pcEncCfg, the slice and the SPS
  void setAdaptiveQP(Bool bUseAdaptiveQP, Int iQPAdaptationRange) { m_bUseAdaptiveQP = bUseAdaptiveQP, m_iQPAdaptationRange = iQPAdaptationRange; }
  void setSlice(TEncPic *pcPic, Int iSliceQp, Int iQpBDOffsetY) { m_pcPic = pcPic, m_iSliceQp = iSliceQp, m_iQpBDOffsetY = iQpBDOffsetY; }
  // :1114-1136 for the CU at luma position (cuPelX, cuPelY)
  Int xComputeQP(UInt uiCUPelX, UInt uiCUPelY, UInt uiDepth) const {
    if (!m_bUseAdaptiveQP) return std::min(51, std::max(-m_iQpBDOffsetY, m_iSliceQp));
    const hmx_aq_geom &g = m_pcPic->m_geom;
    const Int qp = hmx_aq_compute_qp(&g, m_pcPic->m_act.data(), m_pcPic->m_act.data() + g.total, (int)uiCUPelX, (int)uiCUPelY, (int)uiDepth, m_iSliceQp,
                                     m_iQPAdaptationRange, m_iQpBDOffsetY);
    if (qp == HMX_AQ_NO_QP) throw std::runtime_error("xComputeQP: the CU lies outside the picture");
    return qp;
  }

private:
  TEncPic *m_pcPic = nullptr;
  Bool m_bUseAdaptiveQP = false;
  Int m_iQPAdaptationRange = 6, m_iSliceQp = 0, m_iQpBDOffsetY = 0;
};

} // namespace hmx_hm
