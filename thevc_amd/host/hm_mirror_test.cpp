// hm_mirror_test.cpp -- drives the C++ host mirror (hmx_hm.hpp) the way TEncSearch::xIntraCodingLumaBlk
// does (ENC/TEncSearch.cpp:1006-1165): setQPforQuant, transformNxN, invtransformNxN on one block, and
// prints the results as text so that tests/test_host_mirror.py can compare them with the oracle.
// Usage: hm_mirror_test <bitDepth> <N> <qp> <mode> <seed>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hmx_hm.hpp"

// Usage: hm_mirror_test recur <bitDepth> <qp> <seed>: a 32x32 inter CU whose transform tree splits down to 8x8 in two
// quadrants; prints the coefficient buffer (z-order) and the residual of invRecurTransformNxN.
static int recur_main(int argc, char **argv) {
  if (argc < 5) return 2;
  const int B = atoi(argv[2]), qp = atoi(argv[3]);
  unsigned seed = (unsigned)atoi(argv[4]);
  hmx_hm::Context ctx(B);
  hmx_hm::TComTrQuant tq(ctx);
  tq.setQPforQuant(qp, hmx_hm::TEXT_LUMA, 6 * (B - 8), 0);
  const int W = 32, parts = 64; // 64 partitions of 4x4 in a 32x32 CU (depth 1 of a 64x64 LCU)
  std::vector<unsigned char> trIdx(parts), cbf(parts);
  // quadrant 0: one 16x16 leaf (trIdx 1); quadrant 1: four 8x8 leaves (trIdx 2); quadrant 2: 16x16 not coded; quadrant 3: 8x8 leaves, two coded
  for (int p = 0; p < parts; p++) {
    const int quad = p / 16, sub = (p % 16) / 4;
    trIdx[p] = (quad == 1 || quad == 3) ? 2 : 1;
    unsigned char f = 1; // depth 0: something is coded in the CU
    if (quad != 2) f |= 2;
    if (quad == 1 || (quad == 3 && (sub == 0 || sub == 3))) f |= 4;
    cbf[p] = f;
  }
  std::vector<int> coef(W * W);
  for (auto &v : coef) {
    seed = seed * 1664525u + 1013904223u;
    v = ((seed >> 20) % 7 == 0) ? (int)((seed >> 8) % 41) - 20 : 0;
  }
  std::vector<short> resi(W * W, 0);
  hmx_hm::TComTrQuant::CuTransformTree cu{trIdx.data(), cbf.data(), nullptr, 1, 64, 256, (hmx_hm::UInt)parts, false};
  tq.invRecurTransformNxN(cu, 0, hmx_hm::TEXT_LUMA, resi.data(), 0, W, W, W, 2, 0, coef.data());
  for (int v : coef) printf("%d ", v);
  printf("\n");
  for (int v : resi) printf("%d ", v);
  printf("\n");
  return 0;
}

// Usage: hm_mirror_test wp <bitDepth> <seed>: a 16x8 unit of random 14-bit intermediates of two lists through
// TComWeightPrediction::xWeightedPredictionUni (list 0's row) and xWeightedPredictionBi (both rows).  Prints the two rows
// (weight offset log2Denom per component), the derived offset / shift / round of the bi case, the six source planes and the
// six result planes, one line each.
static int wp_main(int argc, char **argv) {
  if (argc < 4) return 2;
  const int B = atoi(argv[2]), W = 16, H = 8;
  unsigned seed = (unsigned)atoi(argv[3]);
  auto next = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 8; };
  hmx_hm::Context ctx(B);
  hmx_hm::TComWeightPrediction wp(ctx);
  hmx_hm::wpScalingParam row[2][3] = {};
  for (int yuv = 0; yuv < 3; yuv++) {
    const unsigned d = next() % 8; // one denominator per component for both lists, as the slice header codes it
    for (int l = 0; l < 2; l++) {
      row[l][yuv].bPresentFlag = true;
      row[l][yuv].uiLog2WeightDenom = d;
      row[l][yuv].iWeight = (int)(next() % 384) - 128;
      row[l][yuv].iOffset = (int)(next() % 256) - 128;
    }
  }
  std::vector<short> buf[2][3], out[2][3];
  hmx_pic src[2], dst[2];
  for (int l = 0; l < 2; l++)
    for (int yuv = 0; yuv < 3; yuv++) {
      const int w = W >> (yuv ? 1 : 0), h = H >> (yuv ? 1 : 0);
      buf[l][yuv].resize(w * h);
      out[l][yuv].assign(w * h, 0);
      for (auto &v : buf[l][yuv]) v = (short)((int)(next() % 16384) - 8192);
      src[l].plane[yuv] = buf[l][yuv].data(), src[l].stride[yuv] = w;
      dst[l].plane[yuv] = out[l][yuv].data(), dst[l].stride[yuv] = w;
    }
  wp.xWeightedPredictionUni(&src[0], W, H, row[0], &dst[0]);
  wp.xWeightedPredictionBi(&src[0], &src[1], row[0], row[1], W, H, &dst[1]);
  for (int l = 0; l < 2; l++) {
    for (int yuv = 0; yuv < 3; yuv++) printf("%d %d %u ", row[l][yuv].iWeight, row[l][yuv].iOffset, row[l][yuv].uiLog2WeightDenom);
    printf("\n");
  }
  for (int yuv = 0; yuv < 3; yuv++) printf("%d %d %d ", row[0][yuv].offset, row[0][yuv].shift, row[0][yuv].round);
  printf("\n");
  for (auto *set : {buf, out})
    for (int l = 0; l < 2; l++)
      for (int yuv = 0; yuv < 3; yuv++) {
        for (int v : set[l][yuv]) printf("%d ", v);
        printf("\n");
      }
  return 0;
}

// Usage: hm_mirror_test me <bitDepth> <seed>: the integer stage of xMotionEstimation for one 16x16 unit of a 64x64 picture
// (margin 24): setLambda, xSetSearchRange (range 6), getMotionCost(1, 0), setPredictor, setCostScale(2), xPatternSearch.
// Prints the unit as hmx_me_unit fields with the cost multiplier and the geometry, the original plane, the reference plane
// with its margins, and "mvx mvy sad", one line each.
static int me_main(int argc, char **argv) {
  if (argc < 4) return 2;
  const int B = atoi(argv[2]), W = 64, H = 64, M = 24, S = W + 2 * M;
  unsigned seed = (unsigned)atoi(argv[3]);
  const bool fastEnc = (seed & 1) != 0; // getUseFastEnc(): rows > 8 are sub-sampled
  auto next = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 8; };
  hmx_hm::Context ctx(B);
  hmx_hm::TComRdCost rd(ctx);
  hmx_hm::TEncSearch search(ctx, rd, {W, H, M, M, 64}, fastEnc);
  std::vector<short> org(W * H), ref(S * (H + 2 * M));
  for (auto &v : org) v = (short)(next() % (1u << B));
  for (auto &v : ref) v = (short)(next() % (1u << B));
  short *d_org = nullptr, *d_ref = nullptr;
  ctx.check(hmx_malloc(ctx.get(), org.size() * 2, (void **)&d_org), "malloc");
  ctx.check(hmx_malloc(ctx.get(), ref.size() * 2, (void **)&d_ref), "malloc");
  ctx.check(hmx_upload(ctx.get(), d_org, org.data(), org.size() * 2), "upload");
  ctx.check(hmx_upload(ctx.get(), d_ref, ref.data(), ref.size() * 2), "upload");
  hmx_pic po{}, pr{};
  po.plane[0] = d_org, po.stride[0] = W;
  pr.plane[0] = d_ref + M * S + M, pr.stride[0] = S;
  const int x = 24, y = 16, w = 16, h = 16, predHor = (int)(next() % 41) - 20, predVer = (int)(next() % 41) - 20;
  rd.setLambda(20.0 + next() % 40);
  int lt[2], rb[2], mv[2];
  search.xSetSearchRange(x, y, predHor, predVer, 6, lt, rb);
  rd.getMotionCost(true, 0);
  rd.setPredictor(predHor, predVer);
  rd.setCostScale(2);
  hmx_hm::UInt sad = 0;
  search.xPatternSearch(&po, &pr, x, y, w, h, lt, rb, mv, sad);
  printf("%d %d %d %d %d %d %d %d %d %d %d %u %d %d %d\n", x, y, w, h, fastEnc ? 1 : 0, predHor, predVer, lt[0], lt[1], rb[0], rb[1],
         rd.motionCostMultiplier(), W, H, M);
  for (int v : org) printf("%d ", v);
  printf("\n");
  for (int v : ref) printf("%d ", v);
  printf("\n%d %d %u\n", mv[0], mv[1], sad);
  hmx_free(ctx.get(), d_org);
  hmx_free(ctx.get(), d_ref);
  return 0;
}

// Usage: hm_mirror_test frac <bitDepth> <seed>: xMotionEstimation for one 16x8 (odd seed: 8x16) unit of a 64x64 picture
// (margin 24), search range 5, once uni-predicted (fWeight 1.0) and once as the bi-prediction refinement (fWeight 0.5, the
// range centred on a start vector), on a reference that is the original displaced by a fractional vector plus noise.
// Prints "x y w h sub_shift predHor predVer multiplier W H M useHADME range bitsIn startHor startVer", the original plane, the
// reference plane with its margins, and per run "mvHor mvVer bits cost", one line each.
// hm_mirror_test tz <bitDepth> <seed>: the same with m_iFastSearch = 1, margin 40, search range 16 and a predictor up to ten
// samples off: the uni-predicted run takes xTZSearch from the predictor, the bi-prediction refinement still the full search.
static int frac_main(int argc, char **argv) {
  if (argc < 4) return 2;
  const bool tz = std::string(argv[1]) == "tz";
  const int B = atoi(argv[2]), W = 64, H = 64, M = tz ? 40 : 24, S = W + 2 * M, RANGE = tz ? 16 : 5;
  unsigned seed = (unsigned)atoi(argv[3]);
  const bool fastEnc = (seed & 1) != 0, hadME = (seed & 2) == 0;
  auto next = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 8; };
  hmx_hm::Context ctx(B);
  hmx_hm::TComRdCost rd(ctx);
  hmx_hm::TEncSearch search(ctx, rd, {W, H, M, M, 64}, fastEnc, hadME, tz ? 1 : 0);
  std::vector<short> org(W * H), ref(S * (H + 2 * M));
  const int maxv = (1 << B) - 1;
  for (int r = 0; r < H + 2 * M; r++) // a smooth surface plus noise: the costs have a real minimum between samples
    for (int c = 0; c < S; c++) {
      const int v = (maxv / 2) + (int)((maxv / 3) * std::sin(c / 3.7) * std::cos(r / 4.3)) + (int)(next() % 5) - 2;
      ref[r * S + c] = (short)(v < 0 ? 0 : v > maxv ? maxv : v);
    }
  const int sx = (int)(next() % 5) - 2, sy = (int)(next() % 5) - 2;
  for (int r = 0; r < H; r++)
    for (int c = 0; c < W; c++) { // between the sample at (sx, sy) and its right / lower neighbour
      const int a = ref[(M + r + sy) * S + M + c + sx], b = ref[(M + r + sy) * S + M + c + sx + 1], d = ref[(M + r + sy + 1) * S + M + c + sx];
      org[r * W + c] = (short)((2 * a + b + d + 2) >> 2);
    }
  short *d_org = nullptr, *d_ref = nullptr;
  ctx.check(hmx_malloc(ctx.get(), org.size() * 2, (void **)&d_org), "malloc");
  ctx.check(hmx_malloc(ctx.get(), ref.size() * 2, (void **)&d_ref), "malloc");
  ctx.check(hmx_upload(ctx.get(), d_org, org.data(), org.size() * 2), "upload");
  ctx.check(hmx_upload(ctx.get(), d_ref, ref.data(), ref.size() * 2), "upload");
  hmx_pic po{}, pr{};
  po.plane[0] = d_org, po.stride[0] = W;
  pr.plane[0] = d_ref + M * S + M, pr.stride[0] = S;
  const int x = 24, y = 16, w = fastEnc ? 8 : 16, h = fastEnc ? 16 : 8;
  const int ps = tz ? 40 : 12; // the predictor's reach, quarter samples
  const int pred[2] = {(int)(next() % (2 * ps + 1)) - ps, (int)(next() % (2 * ps + 1)) - ps}, start[2] = {4 * sx + (int)(next() % 9) - 4, 4 * sy + (int)(next() % 9) - 4};
  const unsigned bitsIn = next() % 7;
  rd.setLambda(20.0 + next() % 40);
  rd.getMotionCost(true, 0);
  printf("%d %d %d %d %d %d %d %u %d %d %d %d %d %u %d %d\n", x, y, w, h, (fastEnc && h > 8) ? 1 : 0, pred[0], pred[1], rd.motionCostMultiplier(), W, H, M,
         hadME ? 1 : 0, RANGE, bitsIn, start[0], start[1]);
  for (int v : org) printf("%d ", v);
  printf("\n");
  for (int v : ref) printf("%d ", v);
  printf("\n");
  for (int bi = 0; bi < 2; bi++) {
    int mv[2] = {start[0], start[1]};
    hmx_hm::UInt bits = bitsIn, cost = 0;
    search.xMotionEstimation(&po, &pr, x, y, w, h, pred, RANGE, bi != 0, mv, bits, cost);
    printf("%d %d %u %u\n", mv[0], mv[1], bits, cost);
  }
  hmx_free(ctx.get(), d_org);
  hmx_free(ctx.get(), d_ref);
  return 0;
}

// Usage: hm_mirror_test calls <file>: xMotionEstimation for calls somebody else recorded (tests/test_me_enc_tap.py writes the
// file from calls of the reference encoder's own xMotionEstimation).  The file is int32 words {bit depth, picture width,
// height, margin x, margin y, CTU size, FEN, HadamardME, m_iFastSearch, m_uiLambdaMotionSAD, number of calls}, the reference's
// luma plane with its margins as int16, then per call 13 words {CU x, CU y, unit x, y, width, height, bBi, predictor hor, ver,
// rcMv hor, ver as it comes in, search range, ruiBits as it comes in} and the unit's original block as int16 (for bBi it is
// 2 * org - other).  Prints "mvHor mvVer bits cost" per call.
// hm_mirror_test calls_wp <file>: the same for calls recorded in weighted slices (tests/test_me_wp_enc_tap.py).  Per call 17
// words: the 13 above, then {iWeight, iOffset, uiLog2WeightDenom of the luma row of the reference searched, 1 if the slice was
// searched weighted}; the mirror runs setWpScalingDistParam with that row (or none) before xMotionEstimation.  Prints "mvHor
// mvVer bits cost sadw hadsw" per call: the last two are TComRdCostWeightPrediction::xGetSADw / xGetHADsw with the row between
// the original block and the reference block at the integer part of the vector found.
static int calls_main(int argc, char **argv) {
  if (argc < 3) return 2;
  const bool weighted = std::string(argv[1]) == "calls_wp";
  const int words = weighted ? 17 : 13;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  int hd[11];
  if (fread(hd, sizeof(int), 11, f) != 11) return 2;
  const int B = hd[0], W = hd[1], H = hd[2], MX = hd[3], MY = hd[4], S = W + 2 * MX;
  std::vector<short> ref((size_t)S * (H + 2 * MY)), org((size_t)W * H);
  if (fread(ref.data(), sizeof(short), ref.size(), f) != ref.size()) return 2;
  hmx_hm::Context ctx(B);
  hmx_hm::TComRdCost rd(ctx);
  hmx_hm::TEncSearch search(ctx, rd, {W, H, MX, MY, hd[5]}, hd[6] != 0, hd[7] != 0, hd[8]);
  hmx_hm::TComRdCostWeightPrediction rdw(ctx);
  const double root = ((double)(unsigned)hd[9] + 0.5) / 65536.0; // setLambda floors 65536 * sqrt(lambda): aim at the middle of the step
  rd.setLambda(root * root);
  rd.getMotionCost(true, 0);
  if (rd.motionCostMultiplier() != (unsigned)hd[9]) return 3;
  short *d_org = nullptr, *d_ref = nullptr;
  ctx.check(hmx_malloc(ctx.get(), org.size() * 2, (void **)&d_org), "malloc");
  ctx.check(hmx_malloc(ctx.get(), ref.size() * 2, (void **)&d_ref), "malloc");
  ctx.check(hmx_upload(ctx.get(), d_ref, ref.data(), ref.size() * 2), "upload");
  hmx_pic po{}, pr{};
  po.plane[0] = d_org, po.stride[0] = W;
  pr.plane[0] = d_ref + MY * S + MX, pr.stride[0] = S;
  for (int k = 0; k < hd[10]; k++) {
    int c[17];
    if (fread(c, sizeof(int), words, f) != (size_t)words) return 2;
    const int x = c[2], y = c[3], w = c[4], h = c[5];
    if (x < 0 || y < 0 || w <= 0 || h <= 0 || x + w > W || y + h > H) return 2;
    std::vector<short> blk((size_t)w * h);
    if (fread(blk.data(), sizeof(short), blk.size(), f) != blk.size()) return 2;
    std::fill(org.begin(), org.end(), (short)0);
    for (int r = 0; r < h; r++)
      for (int n = 0; n < w; n++) org[(size_t)(y + r) * W + x + n] = blk[(size_t)r * w + n];
    ctx.check(hmx_upload(ctx.get(), d_org, org.data(), org.size() * 2), "upload");
    const int pred[2] = {c[7], c[8]};
    int mv[2] = {c[9], c[10]};
    hmx_hm::UInt bits = (hmx_hm::UInt)c[12], cost = 0;
    hmx_hm::wpScalingParam row[3] = {};
    if (weighted) {
      for (int yuv = 0; yuv < 3; yuv++) row[yuv].bPresentFlag = true, row[yuv].iWeight = 1;
      row[0].iWeight = c[13], row[0].iOffset = c[14], row[0].uiLog2WeightDenom = (hmx_hm::UInt)c[15];
      search.setWpScalingDistParam(c[16] ? row : nullptr);
    }
    search.xMotionEstimation(&po, &pr, c[0], c[1], x, y, w, h, pred, c[11], c[6] != 0, mv, bits, cost);
    if (weighted) {
      short *cur = ref.data() + (size_t)(MY + y + (mv[1] >> 2)) * S + MX + x + (mv[0] >> 2);
      printf("%d %d %u %u %u %u\n", mv[0], mv[1], bits, cost, rdw.xGetSADw(blk.data(), w, cur, S, w, h, row), rdw.xGetHADsw(blk.data(), w, cur, S, w, h, row));
    } else printf("%d %d %u %u\n", mv[0], mv[1], bits, cost);
  }
  fclose(f);
  hmx_free(ctx.get(), d_org);
  hmx_free(ctx.get(), d_ref);
  return 0;
}

// Usage: hm_mirror_test pred <file>: the complete-candidate members of TEncSearch (xGetInterPredictionError, xMergeEstimation,
// xGetTemplateCost, the candidate loop of xEstimateMvPredAMVP, xCheckBestMVP) on inputs somebody else made
// (tests/test_gpu_pred_error.py writes the file and compares with tests/pred_error_oracle.py).  The file is int32 words
// {bit depth, picture width, height, margin x, margin y, CTU size, HadamardME, m_uiLambdaMotionSAD, number of reference
// pictures, 1 for a B slice, 1 for a weighted slice, number of operations}, then 16 words {refs[] entry, POC} of reference
// index 0..3 of list 0, then of list 1, in a weighted slice 3 words {iWeight, iOffset, uiLog2WeightDenom} (luma) per picture for
// list 0, then for list 1, the pictures' luma planes with margins and the original's luma plane as int16, and per operation:
//   1 (merge)  {CU x, CU y, unit x, y, width, height, numValidMergeCand}, 5 x 2 x {mv hor, ver, refIdx}, 5 x interDir
//              prints "M uiInterDir uiMergeIndex ruiCost {mv hor ver refIdx} x 2 err0": uiInterDir and uiMergeIndex start at 99 and
//              the fields at (0, 0, -1); err0 = xGetInterPredictionError of candidate 0 as xMergeEstimation left it (0 without one)
//   2 (AMVP)   {CU x, CU y, unit x, y, width, height, list, refIdx, iN}, 2 x {mv hor, ver}
//              prints "A iBestIdx pred hor ver uiDistBiP cost0": uiDistBiP starts at 4294967295; cost0 = xGetTemplateCost of candidate 0
//   3 (MVP)    {iN}, 2 x {mv hor, ver}, {cMv hor, ver, riMVPIdx, ruiBits, ruiCost}
//              prints "C riMVPIdx pred hor ver ruiBits ruiCost"
static int pred_main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  int hd[12], tab[16];
  if (fread(hd, sizeof(int), 12, f) != 12 || fread(tab, sizeof(int), 16, f) != 16) return 2;
  const int B = hd[0], W = hd[1], H = hd[2], MX = hd[3], MY = hd[4], S = W + 2 * MX, nRefs = hd[8];
  if (nRefs < 1 || nRefs > 4) return 2;
  int entry[2][4], poc[2][4];
  for (int l = 0; l < 2; l++)
    for (int i = 0; i < 4; i++) entry[l][i] = tab[l * 8 + 2 * i], poc[l][i] = tab[l * 8 + 2 * i + 1];
  hmx_wp wp[2][4] = {};
  if (hd[10])
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < nRefs; r++) {
        int e[3];
        if (fread(e, sizeof(int), 3, f) != 3) return 2;
        for (int c = 0; c < 3; c++) wp[l][r].weight[c] = 1;
        wp[l][r].weight[0] = (int16_t)e[0], wp[l][r].offset[0] = (int16_t)e[1], wp[l][r].log2_denom[0] = (uint8_t)e[2];
      }
  hmx_hm::Context ctx(B);
  hmx_hm::TComRdCost rd(ctx);
  hmx_hm::TEncSearch search(ctx, rd, {W, H, MX, MY, hd[5]}, false, hd[6] != 0, 0);
  const double root = ((double)(unsigned)hd[7] + 0.5) / 65536.0; // setLambda floors 65536 * sqrt(lambda): aim at the middle of the step
  rd.setLambda(root * root);
  if (rd.lambdaMotionSAD() != (unsigned)hd[7]) return 3;
  std::vector<short> plane((size_t)S * (H + 2 * MY));
  short *d_ref[4] = {}, *d_org = nullptr;
  hmx_pic refs[4] = {}, po{};
  for (int r = 0; r < nRefs; r++) {
    if (fread(plane.data(), sizeof(short), plane.size(), f) != plane.size()) return 2;
    ctx.check(hmx_malloc(ctx.get(), plane.size() * 2, (void **)&d_ref[r]), "malloc");
    ctx.check(hmx_upload(ctx.get(), d_ref[r], plane.data(), plane.size() * 2), "upload");
    refs[r].plane[0] = d_ref[r] + (size_t)MY * S + MX, refs[r].stride[0] = S;
  }
  if (fread(plane.data(), sizeof(short), (size_t)W * H, f) != (size_t)W * H) return 2;
  ctx.check(hmx_malloc(ctx.get(), (size_t)W * H * 2, (void **)&d_org), "malloc");
  ctx.check(hmx_upload(ctx.get(), d_org, plane.data(), (size_t)W * H * 2), "upload");
  po.plane[0] = d_org, po.stride[0] = W;
  search.setRefLists({refs, nRefs, {entry[0], entry[1]}, {poc[0], poc[1]}, hd[9] != 0, hd[10] ? wp[0] : nullptr, hd[10] ? wp[1] : nullptr});
  for (int k = 0; k < hd[11]; k++) {
    int kind, c[42];
    if (fread(&kind, sizeof(int), 1, f) != 1) return 2;
    if (kind == 1) {
      if (fread(c, sizeof(int), 42, f) != 42) return 2;
      hmx_hm::TComMvField nb[10], out[2];
      unsigned char dir[5];
      for (int i = 0; i < 10; i++) nb[i].setMvField(c[7 + 3 * i], c[8 + 3 * i], c[9 + 3 * i]);
      for (int i = 0; i < 5; i++) dir[i] = (unsigned char)c[37 + i];
      hmx_hm::UInt interDir = 99, mergeIndex = 99, cost = 0, err0 = 0;
      search.xMergeEstimation(&po, c[0], c[1], c[2], c[3], c[4], c[5], interDir, out, mergeIndex, cost, nb, dir, c[6]);
      if (c[6] > 0) search.xGetInterPredictionError(&po, c[0], c[1], c[2], c[3], c[4], c[5], nb, err0, hd[6] != 0);
      printf("M %u %u %u %d %d %d %d %d %d %u\n", interDir, mergeIndex, cost, out[0].mvHor, out[0].mvVer, out[0].refIdx, out[1].mvHor, out[1].mvVer,
             out[1].refIdx, err0);
    } else if (kind == 2) {
      if (fread(c, sizeof(int), 13, f) != 13) return 2;
      const int cand[2][2] = {{c[9], c[10]}, {c[11], c[12]}};
      int pred[2] = {0, 0}, idx = -1;
      hmx_hm::UInt distBiP = 0xFFFFFFFFu;
      search.xEstimateMvPredAMVP(&po, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], cand, c[8], pred, idx, &distBiP);
      const hmx_hm::UInt cost0 = search.xGetTemplateCost(&po, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], cand[0], 0, hmx_hm::TEncSearch::AMVP_MAX_NUM_CANDS);
      printf("A %d %d %d %u %u\n", idx, pred[0], pred[1], distBiP, cost0);
    } else if (kind == 3) {
      if (fread(c, sizeof(int), 10, f) != 10) return 2;
      const int cand[2][2] = {{c[1], c[2]}, {c[3], c[4]}}, mv[2] = {c[5], c[6]};
      int idx = c[7], pred[2] = {c[0] > 0 ? cand[c[7]][0] : 0, c[0] > 0 ? cand[c[7]][1] : 0};
      hmx_hm::UInt bits = (hmx_hm::UInt)c[8], cost = (hmx_hm::UInt)c[9];
      search.xCheckBestMVP(cand, c[0], mv, pred, idx, bits, cost);
      printf("C %d %d %d %u %u\n", idx, pred[0], pred[1], bits, cost);
    } else
      return 2;
  }
  fclose(f);
  for (int r = 0; r < nRefs; r++) hmx_free(ctx.get(), d_ref[r]);
  hmx_free(ctx.get(), d_org);
  return 0;
}

// Usage: hm_mirror_test wpest <file>: WeightPredAnalysis on recorded slices (tests/test_gpu_wp_estimate.py writes the file and
// compares with the tables the reference encoder wrote).  The file is int32 words {bit depth, width, height, number of pictures,
// number of slices}, per picture its original and its reconstruction (three planes each, int16), then per slice {picture, 1 for a
// P slice, entries of list 0, of list 1} and the picture index of every entry.  Every picture's AC/DC comes from
// xCalcACDCParamSlice; the slices run through one WeightPredAnalysis in file order.  Prints per slice "useWP wpBiPred" and one
// line per list with "present weight offset log2denom" of every entry and component.
static int wpest_main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  int hd[5];
  if (fread(hd, sizeof(int), 5, f) != 5) return 2;
  const int B = hd[0], W = hd[1], H = hd[2], nPics = hd[3], nSlices = hd[4];
  if (W <= 0 || H <= 0 || (W | H) & 1 || nPics <= 0 || nPics > 64) return 2;
  hmx_hm::Context ctx(B);
  hmx_hm::WeightPredAnalysis wpa(ctx);
  const size_t elems = (size_t)W * H * 3 / 2;
  std::vector<short> buf(elems);
  std::vector<hmx_pic> org((size_t)nPics), rec((size_t)nPics);
  std::vector<hmx_hm::WpSlice> stat((size_t)nPics);
  std::vector<void *> owned;
  for (int i = 0; i < nPics; i++)
    for (hmx_pic *p : {&org[(size_t)i], &rec[(size_t)i]}) {
      if (fread(buf.data(), sizeof(short), elems, f) != elems) return 2;
      short *d = nullptr;
      ctx.check(hmx_malloc(ctx.get(), elems * 2, (void **)&d), "malloc");
      ctx.check(hmx_upload(ctx.get(), d, buf.data(), elems * 2), "upload");
      owned.push_back(d);
      p->plane[0] = d, p->plane[1] = d + (size_t)W * H, p->plane[2] = d + (size_t)W * H * 5 / 4;
      p->stride[0] = W, p->stride[1] = p->stride[2] = W / 2;
    }
  for (int i = 0; i < nPics; i++) { // TEncSlice.cpp:689-692: every picture of the sequence
    stat[(size_t)i].picYuvOrg = &org[(size_t)i], stat[(size_t)i].width = W, stat[(size_t)i].height = H;
    wpa.xCalcACDCParamSlice(&stat[(size_t)i]);
  }
  for (int s = 0; s < nSlices; s++) {
    int sh[4];
    if (fread(sh, sizeof(int), 4, f) != 4) return 2;
    if (sh[0] < 0 || sh[0] >= nPics || sh[2] < 1 || sh[2] > hmx_hm::MAX_NUM_REF || sh[3] < 0 || sh[3] > hmx_hm::MAX_NUM_REF) return 2;
    hmx_hm::WpSlice slice = stat[(size_t)sh[0]];
    slice.isInterP = sh[1] != 0, slice.numRefIdx[0] = sh[2], slice.numRefIdx[1] = sh[3];
    for (int l = 0; l < 2; l++)
      for (int i = 0; i < sh[2 + l]; i++) {
        int q;
        if (fread(&q, sizeof(int), 1, f) != 1 || q < 0 || q >= nPics) return 2;
        slice.refPicYuvRec[l][i] = &rec[(size_t)q], slice.refAcdc[l][i] = stat[(size_t)q].acdc;
      }
    wpa.xEstimateWPParamSlice(&slice); // TEncSlice.cpp:706-710
    wpa.xCheckWPEnable(&slice);
    printf("%d %d\n", slice.useWP ? 1 : 0, slice.wpBiPred ? 1 : 0);
    for (int l = 0; l < 2; l++) {
      for (int i = 0; i < sh[2 + l]; i++)
        for (int yuv = 0; yuv < 3; yuv++) {
          const hmx_hm::wpScalingParam &w = slice.wpScaling[l][i][yuv];
          printf("%d %d %d %u ", w.bPresentFlag ? 1 : 0, w.iWeight, w.iOffset, w.uiLog2WeightDenom);
        }
      printf("\n");
    }
  }
  fclose(f);
  for (void *d : owned) hmx_free(ctx.get(), d);
  return 0;
}

// Usage: hm_mirror_test aq <file>: TEncPreanalyzer::xPreanalyze and TEncCu::xComputeQP on one picture (tests/test_gpu_aq.py writes the
// file and compares with tests/aq_oracle.py).  The file is int32 words {bit depth, width, height, CTU size, AQ depths, slice QP,
// adaptation range}, then the luma plane (int16).  Prints one line with every layer's average activity as the bits of the double
// (hex), then per CU depth 0..3 one line with the QP of every CU position of that depth (CU size max(ctu >> depth, 8)) in raster
// order.
static int aq_main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  int hd[7];
  if (fread(hd, sizeof(int), 7, f) != 7) return 2;
  const int B = hd[0], W = hd[1], H = hd[2], ctu = hd[3], depths = hd[4], sliceQp = hd[5], range = hd[6];
  if (W <= 0 || H <= 0 || W > 4096 || H > 4096) return 2;
  std::vector<short> luma((size_t)W * H);
  if (fread(luma.data(), sizeof(short), luma.size(), f) != luma.size()) return 2;
  fclose(f);
  hmx_hm::Context ctx(B);
  short *d = nullptr;
  ctx.check(hmx_malloc(ctx.get(), luma.size() * 2, (void **)&d), "malloc");
  ctx.check(hmx_upload(ctx.get(), d, luma.data(), luma.size() * 2), "upload");
  hmx_pic org{};
  org.plane[0] = d, org.stride[0] = W;
  hmx_hm::TEncPic pic;
  pic.create(&org, W, H, (unsigned)ctu, (unsigned)depths);
  hmx_hm::TEncPreanalyzer pre(ctx);
  pre.xPreanalyze(&pic);
  for (unsigned l = 0; l < pic.getMaxAQDepth(); l++) {
    const double a = pic.getAQLayer(l)->getAvgActivity();
    unsigned long long bits;
    memcpy(&bits, &a, 8);
    printf("%016llx ", bits);
  }
  printf("\n");
  hmx_hm::TEncCu cu;
  cu.setAdaptiveQP(true, range);
  cu.setSlice(&pic, sliceQp, 6 * (B - 8));
  for (unsigned depth = 0; depth < 4; depth++) {
    const int size = std::max(ctu >> depth, 8);
    for (int y = 0; y < H; y += size)
      for (int x = 0; x < W; x += size) printf("%d ", cu.xComputeQP((unsigned)x, (unsigned)y, depth));
    printf("\n");
  }
  hmx_free(ctx.get(), d);
  return 0;
}

// Usage: hm_mirror_test sao_decide <file>: TEncSampleAdaptiveOffset::rdoSaoUnitAll on two pictures in a row, the second at
// hierarchy depth 1 under the rate state the first left (tests/test_gpu_sao_decide.py writes the file and compares with
// tests/sao_decision_oracle.py).  The file is int32 words {bit depth, width, height, CTU size, slice type, slice QP, fraction}, two
// doubles {lambda, lambda chroma}, then the bins of the two pictures (int32 [2][3][CTU][52][2]).  Prints per picture one line
// "bSaoFlag bSaoFlag numNoSao numNoSao state state frac" and per component and CTU "type sub o0 o1 o2 o3 left up".
static int sao_decide_main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[2], "rb");
  if (!f) return 2;
  int hd[7];
  double lam[2];
  if (fread(hd, sizeof(int), 7, f) != 7 || fread(lam, sizeof(double), 2, f) != 2) return 2;
  const int B = hd[0], W = hd[1], H = hd[2], ctu = hd[3];
  if (W <= 0 || H <= 0 || W > 4096 || H > 4096 || ctu < 16) return 2;
  const int n = ((W + ctu - 1) / ctu) * ((H + ctu - 1) / ctu);
  std::vector<hmx_sao_stat> bins((size_t)2 * 3 * n * HMX_SAO_STAT_BINS);
  if (fread(bins.data(), sizeof(hmx_sao_stat), bins.size(), f) != bins.size()) return 2;
  fclose(f);
  hmx_hm::Context ctx(B, 0, ctu);
  hmx_sao_stat *d_stats = nullptr;
  hmx_sao_unit *d_units = nullptr;
  hmx_sao_result *d_res = nullptr;
  ctx.check(hmx_malloc(ctx.get(), bins.size() * sizeof(hmx_sao_stat), (void **)&d_stats), "malloc");
  ctx.check(hmx_malloc(ctx.get(), (size_t)3 * n * sizeof(hmx_sao_unit), (void **)&d_units), "malloc");
  ctx.check(hmx_malloc(ctx.get(), sizeof(hmx_sao_result), (void **)&d_res), "malloc");
  ctx.check(hmx_upload(ctx.get(), d_stats, bins.data(), bins.size() * sizeof(hmx_sao_stat)), "upload");
  hmx_hm::TEncSampleAdaptiveOffset sao(ctx);
  std::vector<hmx_sao_unit> units((size_t)3 * n);
  for (int pic = 0; pic < 2; pic++) {
    hmx_hm::TEncSampleAdaptiveOffset::SAOParam sp;
    sao.startSaoEnc(hd[4], hd[5], (unsigned)hd[6]);
    sao.rdoSaoUnitAll(&sp, d_stats + (size_t)pic * 3 * n * HMX_SAO_STAT_BINS, W, H, n, lam[0], lam[1], pic, nullptr, d_units, nullptr, d_res);
    ctx.check(hmx_download(ctx.get(), units.data(), d_units, units.size() * sizeof(hmx_sao_unit)), "download");
    printf("%d %d %u %u %u %u %u\n", (int)sp.bSaoFlag[0], (int)sp.bSaoFlag[1], sp.result.num_no_sao[0], sp.result.num_no_sao[1],
           (unsigned)sp.result.ctx_state[0], (unsigned)sp.result.ctx_state[1], sp.result.frac);
    for (const hmx_sao_unit &u : units)
      printf("%d %d %d %d %d %d %d %d\n", (int)u.type, (int)u.sub, (int)u.offset[0], (int)u.offset[1], (int)u.offset[2], (int)u.offset[3],
             (int)u.merge_left, (int)u.merge_up);
  }
  hmx_free(ctx.get(), d_stats), hmx_free(ctx.get(), d_units), hmx_free(ctx.get(), d_res);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && std::string(argv[1]) == "sao_decide") {
    try {
      return sao_decide_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "hm_mirror_test: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "aq") {
    try {
      return aq_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "hm_mirror_test: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "wpest") {
    try {
      return wpest_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "hm_mirror_test: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "pred") {
    try {
      return pred_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && (std::string(argv[1]) == "calls" || std::string(argv[1]) == "calls_wp")) {
    try {
      return calls_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && (std::string(argv[1]) == "frac" || std::string(argv[1]) == "tz")) {
    try {
      return frac_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "me") {
    try {
      return me_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "wp") {
    try {
      return wp_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
    }
  }
  if (argc >= 2 && std::string(argv[1]) == "recur") {
    try {
      return recur_main(argc, argv);
    } catch (const std::exception &e) {
      fprintf(stderr, "error: %s\n", e.what());
      return 1;
    }
  }
  if (argc < 6) return 2;
  const int B = atoi(argv[1]), N = atoi(argv[2]), qp = atoi(argv[3]), mode = atoi(argv[4]);
  unsigned seed = (unsigned)atoi(argv[5]);
  try {
    hmx_hm::Context ctx(B);
    hmx_hm::TComTrQuant tq(ctx);
    std::vector<short> resi(N * N), rec(N * N);
    std::vector<int> lev(N * N);
    for (auto &v : resi) {
      seed = seed * 1664525u + 1013904223u;
      v = (short)((int)((seed >> 16) % 61) - 30);
    }
    tq.setQPforQuant(qp, hmx_hm::TEXT_LUMA, 6 * (B - 8), 0);
    tq.setBlockState(true, mode, HMX_I_SLICE, true);
    hmx_hm::UInt absSum = 0;
    tq.transformNxN(resi.data(), N, lev.data(), N, N, absSum, hmx_hm::TEXT_LUMA);
    tq.invtransformNxN(false, hmx_hm::TEXT_LUMA, mode, rec.data(), N, lev.data(), N, N, 0);
    printf("%u\n", absSum);
    for (int v : resi) printf("%d ", v);
    printf("\n");
    for (int v : lev) printf("%d ", v);
    printf("\n");
    for (int v : rec) printf("%d ", v);
    printf("\n");
  } catch (const std::exception &e) {
    fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
