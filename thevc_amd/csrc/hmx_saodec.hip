// hmx_saodec.hip -- the encoder's SAO parameter search with SAOLcuBasedOptimization = 1: TEncSampleAdaptiveOffset::rdoSaoUnitAll
// (TLibEncoder/TEncSampleAdaptiveOffset.cpp:1466-1799) over saoComponentParamDist (:1897-2062), sao2ChromaParamDist (:2064-2240),
// estSaoTypeDist / estSaoDist / estIterOffset (:1808-1893) and the rates of TEncEntropy::encodeSaoOffset (TEncEntropy.cpp:759-838)
// under TEncBinCABACCounter (TEncBinCoderCABACCounter.cpp:61-101), between the statistics (hmx_sao_stats*) and the application
// (hmx_sao_picture*).  Macros as the fork sets them (TypeDef.h:87-91, 121-130, 147, 218): SAO_SINGLE_MERGE, SAO_TYPE_SHARING,
// SAO_TYPE_CODING, SAO_MERGE_ONE_CTX, SAO_ABS_BY_PASS, SAO_ENCODING_CHOICE[_CHROMA], SAO_CHROMA_LAMBDA, FAST_BIT_EST, FULL_NBIT 0.
// Out of scope: the quadtree search of SAOLcuBasedOptimization = 0 (rdoSaoOnePart, runQuadTreeDecision), SaoLcuBoundary /
// interleaved SAO, writing the bitstream.
//
// Two kernels.  k_sao_cand, parallel over picture x CTU x component, does everything that does not depend on the coder state:
// the quantised offset of every class walked towards zero (estIterOffset), the distortion of the four edge types, the band
// window search -- and counts the bypass bins of each candidate type.  Every bin of encodeSaoOffset but the first of
// codeSaoTypeIdx is a bypass bin (SAO_ABS_BY_PASS), each worth exactly 32768 fractional bits, so the written bits of a candidate
// are its bypass count plus (fraction + entropy bits of the one context bin) >> 15: the serial part of a rate is one table entry.
// k_sao_decide, one wave per picture, walks the CTUs in raster order with the two context states and the 15 fractional bits that
// survive resetBits (TEncBinCoderCABAC.cpp:193), picks the type per component, the two merge candidates, and writes the tables.
#include "hmx_host.h"

#include <cmath>

// tempDist + lambda * tempRate (:1879), estDist + lambda * estRate (:2000, :2178): one fused multiply-add changes a decision
#pragma clang fp contract(off)

namespace {
typedef unsigned long long u64;

// ContextModel.cpp:106-117 (m_entropyBits, FAST_BIT_EST) ...
__constant__ const unsigned kSaoEntropyBits[128] = {
    0x07b23, 0x085f9, 0x074a0, 0x08cbc, 0x06ee4, 0x09354, 0x067f4, 0x09c1b, 0x060b0, 0x0a62a, 0x05a9c, 0x0af5b, 0x0548d, 0x0b955, 0x04f56, 0x0c2a9,
    0x04a87, 0x0cbf7, 0x045d6, 0x0d5c3, 0x04144, 0x0e01b, 0x03d88, 0x0e937, 0x039e0, 0x0f2cd, 0x03663, 0x0fc9e, 0x03347, 0x10600, 0x03050, 0x10f95,
    0x02d4d, 0x11a02, 0x02ad3, 0x12333, 0x0286e, 0x12cad, 0x02604, 0x136df, 0x02425, 0x13f48, 0x021f4, 0x149c4, 0x0203e, 0x1527b, 0x01e4d, 0x15d00,
    0x01c99, 0x166de, 0x01b18, 0x17017, 0x019a5, 0x17988, 0x01841, 0x18327, 0x016df, 0x18d50, 0x015d9, 0x19547, 0x0147c, 0x1a083, 0x0138e, 0x1a8a3,
    0x01251, 0x1b418, 0x01166, 0x1bd27, 0x01068, 0x1c77b, 0x00f7f, 0x1d18e, 0x00eda, 0x1d91a, 0x00e19, 0x1e254, 0x00d4f, 0x1ec9a, 0x00c90, 0x1f6e0,
    0x00c01, 0x1fef8, 0x00b5f, 0x208b1, 0x00ab6, 0x21362, 0x00a15, 0x21e46, 0x00988, 0x2285d, 0x00934, 0x22ea8, 0x008a8, 0x239b2, 0x0081d, 0x24577,
    0x007c9, 0x24ce6, 0x00763, 0x25663, 0x00710, 0x25e8f, 0x006a0, 0x26a26, 0x00672, 0x26f23, 0x005e8, 0x27ef8, 0x005ba, 0x284b5, 0x0055e, 0x29057,
    0x0050c, 0x29bab, 0x004c1, 0x2a674, 0x004a7, 0x2aa5e, 0x0046f, 0x2b32f, 0x0041f, 0x2c0ad, 0x003e7, 0x2ca8d, 0x003ba, 0x2d323, 0x0010c, 0x3bfbb};
// ... and :79-89 (m_aucNextStateLPS); m_aucNextStateMPS (:67-77) is s + 2 below 124 and s from there
__constant__ const unsigned char kSaoNextLps[128] = {
    1,  0,  0,  1,  2,  3,  4,  5,  4,  5,  8,  9,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 18, 19, 22, 23, 22, 23, 24,  25,
    26, 27, 26, 27, 30, 31, 30, 31, 32, 33, 32, 33, 36, 37, 36, 37, 38, 39, 38, 39, 42, 43, 42, 43, 44, 45, 44, 45, 46, 47, 48,  49,
    48, 49, 50, 51, 52, 53, 52, 53, 54, 55, 54, 55, 56, 57, 58, 59, 58, 59, 60, 61, 60, 61, 60, 61, 62, 63, 64, 65, 64, 65, 66,  67,
    66, 67, 66, 67, 68, 69, 68, 69, 70, 71, 70, 71, 70, 71, 72, 73, 72, 73, 72, 73, 74, 75, 74, 75, 74, 75, 76, 77, 76, 77, 126, 127};
__host__ __device__ inline int sao_next_mps(int s) { return s < 124 ? s + 2 : s; }

// What the candidate stage hands to the decision stage per (picture, component, CTU): the five candidate types SAO_EO_0..3, SAO_BO
struct SaoCand {
  long long dist[5]; // estDist of the type (band: over the best window)
  uint32_t off[5];   // the four offsets, unscaled, one int8 per byte, class order
  uint32_t band;     // bestClassTableBo
  uint8_t nb[8];     // [0..4]: bypass bins encodeSaoOffset codes for the type, as component 0 / 1 (2 codes three fewer: no type bit, :771,
                     // and no edge class, :826, for edge types; one fewer for the band type)
};
static_assert(sizeof(SaoCand) == 72, "nine qwords per record");
constexpr int kCandQ = 9, kBinQ = HMX_SAO_STAT_BINS, kSlotQ = 3 * (kCandQ + kBinQ);

struct SaoConsts {
  int inc, bi, th, shift; // g_uiBitIncrement, m_uiSaoBitIncrease, m_iOffsetTh (SAOProcess :1253-1263), 2 * g_uiBitIncrement (:1903)
};
__host__ __device__ inline SaoConsts sao_consts(int B) {
  return SaoConsts{B - 8, B - (B < 10 ? B : 10), 1 << ((B - 5) < 5 ? (B - 5) : 5), 2 * (B - 8)};
}

__device__ __forceinline__ long long est_sao_dist(long long count, long long offset, long long org, int shift) { // :1854-1857
  return (count * offset * offset - org * offset * 2) >> shift;
}
// bins of codeSaoMaxUvlc (TEncSbac.cpp:1567-1609), maxSymbol = th - 1 > 0
__device__ __forceinline__ int sao_uvlc_bins(int a, int th) { return a == 0 ? 1 : a + (a < th - 1 ? 1 : 0); }

struct SaoCandArgs {
  const hmx_sao_stat *stats;
  const hmx_sao_decide_param *pp;
  SaoCand *cand;
  int n_lcu, B;
};
// One wave per (CTU, component, picture).  Lanes 0..15: edge type lane >> 2, class (lane & 3) + 1; lanes 16..47: band class lane - 15.
// A component the rate state switched off has no statistics (calcSaoStatsCu is skipped, :1611-1620): its bins count as zero.
__global__ __launch_bounds__(64) void k_sao_cand(SaoCandArgs A) {
  const int lane = threadIdx.x, addr = blockIdx.x, comp = blockIdx.y, pic = blockIdx.z;
  const hmx_sao_decide_param P = A.pp[pic];
  const double lam = comp ? P.lambda_chroma : P.lambda_luma;
  const SaoConsts K = sao_consts(A.B);
  const bool band = lane >= 16;
  const int bin = band ? 20 + (lane - 16) : 5 * (lane >> 2) + (lane & 3) + 1;
  const size_t rec = ((size_t)pic * 3 + comp) * A.n_lcu + addr;
  long long org = 0, count = 0;
  if (P.enable[comp ? 1 : 0] && lane < 48) {
    const hmx_sao_stat s = A.stats[rec * HMX_SAO_STAT_BINS + bin];
    org = s.diff, count = s.count;
  }
  // estSaoTypeDist :1808-1852 for this lane's class
  int o = 0, dist_bo = 0;
  double cost_bo = lam;
  if (count) {
    const double x = (double)(org * (1ll << K.inc)) / (double)(count * (1ll << K.bi)); // :1824
    int q;
    if (K.inc > 0) q = x > 0 ? ((int)x + (1 << (K.inc - 1))) / (1 << K.inc) : ((int)x - (1 << (K.inc - 1))) / (1 << K.inc); // xRoundIbdi2 :91
    else q = x >= 0 ? (int)(x + 0.5) : (int)(x - 0.5);                                                                    // xRoundIbdi :103
    q = min(K.th - 1, max(-K.th + 1, q));
    if (!band && ((q < 0 && (lane & 3) < 2) || (q > 0 && (lane & 3) >= 2))) q = 0; // :1827-1837
    // estIterOffset :1858-1893
    double min_cost = lam;
    for (int it = q; it != 0; it = it > 0 ? it - 1 : it + 1) {
      const int a = it < 0 ? -it : it;
      int rate = band ? a + 2 : a + 1;
      if (a == K.th - 1) rate--;
      const long long d = est_sao_dist(count, (long long)it * (1ll << K.bi), org, K.shift);
      const double cost = (double)d + lam * (double)rate;
      if (cost < min_cost) {
        min_cost = cost, o = it;
        if (band) dist_bo = (int)d, cost_bo = cost;
      }
    }
  }
  const long long d_edge = est_sao_dist(count, (long long)o * (1ll << K.bi), org, K.shift); // :1847
  // the band window (:1950-1971): lane 16 + i holds the window that starts at band i, summed in index order from 0.0
  double w = 0.0;
  w += cost_bo;
  w += __shfl(cost_bo, lane + 1);
  w += __shfl(cost_bo, lane + 2);
  w += __shfl(cost_bo, lane + 3);
  double best = 1.7e+308; // MAX_DOUBLE, CommonDef.h:116
  int start = 0;
  for (int i = 0; i < 29; i++) {
    const double v = __shfl(w, 16 + i);
    if (v < best) best = v, start = i;
  }
  SaoCand C{};
  for (int t = 0; t < 5; t++) {
    const int first = t < 4 ? 4 * t : 16 + start;
    int bins = t < 4 ? 3 : 6; // the bypass bit of codeSaoTypeIdx and the 2 bits of the edge class / the 5 of the band position
    long long d = 0;
    for (int c = 0; c < 4; c++) {
      const int oc = __shfl(o, first + c);
      d += t < 4 ? __shfl(d_edge, first + c) : (long long)__shfl(dist_bo, first + c);
      C.off[t] |= (uint32_t)(oc & 255) << (8 * c);
      const int a = oc < 0 ? -oc : oc;
      bins += sao_uvlc_bins(a, K.th) + (t == 4 && oc != 0 ? 1 : 0); // codeSAOSign
    }
    C.dist[t] = d, C.nb[t] = (uint8_t)bins;
  }
  C.band = (uint32_t)start;
  if (lane == 0) A.cand[rec] = C;
}

struct SaoDecArgs {
  const hmx_sao_stat *stats;
  const SaoCand *cand;
  const hmx_sao_decide_param *pp;
  const uint8_t *allow; // may be null
  hmx_sao_unit *units;
  hmx_sao_lcu *apply;   // may be null
  hmx_sao_result *res;
  int n_lcu, cw, B;
};

struct SaoUnitR { // SaoLcuParam in registers; off as in SaoCand
  int type, sub;
  uint32_t off;
  int left, up;
};
__device__ __forceinline__ u64 sao_pack(const SaoUnitR &u) {
  return (u64)(uint8_t)u.type | (u64)(uint8_t)u.sub << 8 | (u64)u.off << 16 | (u64)u.left << 48 | (u64)u.up << 56;
}
__device__ __forceinline__ SaoUnitR sao_unpack(u64 v) {
  return SaoUnitR{(int)(int8_t)(v & 255), (int)((v >> 8) & 255), (uint32_t)(v >> 16), (int)((v >> 48) & 1), (int)((v >> 56) & 1)};
}
// the distortion of taking the neighbour's parameters (:2034-2053, :2212-2231): its offsets enter estSaoDist as stored, without
// << m_uiSaoBitIncrease (:2046-2047, :2224-2225)
__device__ __forceinline__ long long sao_merge_est(const u64 *bins, const SaoUnitR &nb, int shift) {
  if (nb.type < 0) return 0;
  const int base = nb.type == 4 ? 20 + nb.sub : 5 * nb.type + 1;
  long long est = 0;
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const u64 s = bins[base + c];
    const long long org = (int)(unsigned)s, count = (int)(unsigned)(s >> 32), o = (int8_t)(nb.off >> (8 * c));
    est += est_sao_dist(count, o, org, shift);
  }
  return est;
}

// One wave per picture; every lane carries the same state (the serial chain is a handful of dependent table reads and double
// compares: there is nothing to spread), the lanes share the fetching.  The 27 qwords of the CTU's three candidate records and its
// 156 qwords of bins are loaded two CTUs ahead into registers and parked in an LDS slot one CTU ahead, so that no global load
// stands in the chain; the row of decided units above (the merge-up neighbours) stays in LDS.
__global__ __launch_bounds__(64) void k_sao_decide(SaoDecArgs A) {
  extern __shared__ u64 s_row[]; // [3][cw] packed units of the CTU row above (and, left of x, of this row)
  __shared__ unsigned s_eb[128];
  __shared__ unsigned char s_lps[128];
  __shared__ u64 s_ring[2][kSlotQ];
  const int lane = threadIdx.x, pic = blockIdx.x, n = A.n_lcu, cw = A.cw;
  const hmx_sao_decide_param P = A.pp[pic];
  const SaoConsts K = sao_consts(A.B);
  const bool en0 = P.enable[0] != 0, en1 = P.enable[1] != 0;
  const double lamL = P.lambda_luma, lamC = P.lambda_chroma;
  s_eb[lane] = kSaoEntropyBits[lane], s_eb[lane + 64] = kSaoEntropyBits[lane + 64];
  s_lps[lane] = kSaoNextLps[lane], s_lps[lane + 64] = kSaoNextLps[lane + 64];
  hmx_sao_unit *units = A.units + (size_t)pic * 3 * n;
  hmx_sao_lcu *apply = A.apply ? A.apply + (size_t)pic * 3 * n : nullptr;
  int m = P.ctx_state[0], t = P.ctx_state[1];
  unsigned f = P.frac & 32767; // the fractional bits, always below 32768: every rate starts with resetBits
  unsigned no_sao0 = 0, no_sao1 = 0;
  if (!en0 && !en1) { // :1659: nothing is coded, the coder is not touched
    for (int i = lane; i < 3 * n; i += 64) {
      units[i] = hmx_sao_unit{-1, 0, {0, 0, 0, 0}, 0, 0};
      if (apply) apply[i] = hmx_sao_lcu{-1, 0, {0, 0, 0, 0}};
    }
    if (lane == 0) A.res[pic] = hmx_sao_result{{0, 0}, {(uint8_t)m, (uint8_t)t}, {0, 0}, f};
    return;
  }
  const u64 *g_cand = reinterpret_cast<const u64 *>(A.cand) + (size_t)pic * 3 * n * kCandQ;
  const u64 *g_bins = reinterpret_cast<const u64 *>(A.stats) + (size_t)pic * 3 * n * kBinQ;
  const uint8_t *g_allow = A.allow ? A.allow + (size_t)pic * n : nullptr;
  u64 r[4] = {0, 0, 0, 0};
  unsigned ra = 3;
  const auto fetch = [&](int a) { // lane's share of CTU a (clamped: the loads past the end are not used)
    a = min(a, n - 1);
    if (lane < 3 * kCandQ) r[0] = g_cand[((size_t)(lane / kCandQ) * n + a) * kCandQ + lane % kCandQ];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int j = lane + 64 * k;
      if (j < 3 * kBinQ) r[1 + k] = g_bins[((size_t)(j / kBinQ) * n + a) * kBinQ + j % kBinQ];
    }
    ra = g_allow ? g_allow[a] : 3;
  };
  const auto park = [&](int slot) {
    if (lane < 3 * kCandQ) s_ring[slot][lane] = r[0];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const int j = lane + 64 * k;
      if (j < 3 * kBinQ) s_ring[slot][3 * kCandQ + j] = r[1 + k];
    }
  };
  const auto bin_bits = [&](int s, int b) { return s_eb[s ^ b]; };
  const auto bin_next = [&](int s, int b) { return (s & 1) == b ? sao_next_mps(s) : (int)s_lps[s]; };
  fetch(0);
  park(0);
  unsigned allow_cur = ra;
  fetch(1);
  __syncthreads();
  SaoUnitR left[3] = {};
  for (int a = 0, x = 0, y = 0; a < n; a++) {
    const int slot = a & 1;
    park(slot ^ 1); // CTU a + 1
    const unsigned allow_next = ra;
    fetch(a + 2);
    __syncthreads();
    const u64 *S = s_ring[slot];
    const SaoCand *cd = reinterpret_cast<const SaoCand *>(S);
    const bool aL = x > 0 && (allow_cur & 1), aU = y > 0 && (allow_cur & 2); // :1536-1562
    // the merge flags coded as 0 (:1568-1583 and again :1667-1682): from (m, f) to (m0, f0)
    int m0 = m;
    unsigned f0 = f;
    if (aL) f0 += bin_bits(m0, 0), m0 = bin_next(m0, 0);
    if (aU) f0 += bin_bits(m0, 0), m0 = bin_next(m0, 0);
    // saoComponentParamDist: CI_TEMP_BEST holds (m0, t, f0); every rate is taken after resetBits
    SaoUnitR cur[3];
    double dist[3] = {0.0, 0.0, 0.0};
    unsigned tf = f0 & 32767;
    int tt = t;
    {
      const unsigned c0 = (tf + bin_bits(tt, 0)) >> 15, c1 = (tf + bin_bits(tt, 1)) >> 15;
      double cost_best = (double)c0 * lamL; // :1935
      int best = -1;
      long long best_dist = 0;
      for (int k = 0; k < 5; k++) {
        const long long d = cd[0].dist[k];
        const double cost = (double)d + lamL * (double)(c1 + cd[0].nb[k]); // :2000
        if (cost < cost_best) cost_best = cost, best = k, best_dist = d;
      }
      dist[0] += (double)best_dist / lamL; // :2009
      cur[0] = best < 0 ? SaoUnitR{-1, 0, 0, 0, 0} : SaoUnitR{best, best == 4 ? (int)cd[0].band : best, cd[0].off[best], 0, 0}; // sub: TEncEntropy.cpp:785
      const int b = best < 0 ? 0 : 1; // :2010-2016: the chosen unit coded onto CI_TEMP_BEST
      tf = (tf + bin_bits(tt, b)) & 32767, tt = bin_next(tt, b);
    }
    { // sao2ChromaParamDist
      const unsigned c0 = (tf + bin_bits(tt, 0)) >> 15, c1 = (tf + bin_bits(tt, 1)) >> 15;
      double cost_best = (double)c0 * lamC; // :2107
      int best = -1;
      long long best_dist = 0;
      for (int k = 0; k < 5; k++) {
        const long long d = cd[1].dist[k] + cd[2].dist[k];
        const unsigned bins = (unsigned)cd[1].nb[k] + cd[2].nb[k] - (k < 4 ? 3 : 1); // Cr: no type bits, no edge class
        const double cost = (double)d + lamC * (double)(c1 + bins);                   // :2178
        if (cost < cost_best) cost_best = cost, best = k, best_dist = d;
      }
      dist[0] += (double)best_dist / lamC; // :2189
      cur[1] = best < 0 ? SaoUnitR{-1, 0, 0, 0, 0} : SaoUnitR{best, best == 4 ? (int)cd[1].band : best, cd[1].off[best], 0, 0};
      cur[2] = best < 0 ? SaoUnitR{-1, 0, 0, 0, 0} : SaoUnitR{best, best == 4 ? (int)cd[2].band : 0, cd[2].off[best], 0, 0}; // :780: Cr keeps 0
    }
    // the merge candidates (:2021-2061, :2197-2239): luma, Cb, Cr into dist[1] (left) and dist[2] (up)
    SaoUnitR up[3];
#pragma unroll
    for (int c = 0; c < 3; c++) up[c] = sao_unpack(s_row[c * cw + x]);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const u64 *bins = S + 3 * kCandQ + c * kBinQ;
      const double lam = c ? lamC : lamL;
      const bool on = c ? en1 : en0; // a component without statistics: every bin zero, every distortion 0
      if (aL) dist[1] += (double)(on ? sao_merge_est(bins, left[c], K.shift) : 0ll) / lam;
      if (aU) dist[2] += (double)(on ? sao_merge_est(bins, up[c], K.shift) : 0ll) / lam;
    }
    // the cost of new parameters (:1664-1701): the merge flags as 0, then the enabled components
    int bm = m0, bt = t;
    unsigned bf = f0; // resetBits (:1666) came before the merge flags: their bits count
    {
      unsigned g = bf;
      if (en0) {
        const int b = cur[0].type < 0 ? 0 : 1;
        g += bin_bits(bt, b) + (b ? 32768u * cd[0].nb[cur[0].type < 0 ? 0 : cur[0].type] : 0u), bt = bin_next(bt, b);
      }
      if (en1) {
        const int b = cur[1].type < 0 ? 0 : 1, k = b ? cur[1].type : 0;
        g += bin_bits(bt, b) + (b ? 32768u * ((unsigned)cd[1].nb[k] + cd[2].nb[k] - (k < 4 ? 3 : 1)) : 0u), bt = bin_next(bt, b);
      }
      bf = g;
    }
    double best_cost = dist[0] + (double)(bf >> 15); // :1700
    // the cost of the merges (:1704-1748), strict <, left first
    if (aL) {
      const unsigned g = (f & 32767) + bin_bits(m, 1);
      const double cost = dist[1] + (double)(g >> 15);
      if (cost < best_cost) {
        best_cost = cost, bm = bin_next(m, 1), bt = t, bf = g;
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c ? en1 : en0) cur[c] = left[c], cur[c].left = 1, cur[c].up = 0;
      }
    }
    if (aU) {
      const int mm = aL ? bin_next(m, 0) : m;
      const unsigned g = (f & 32767) + (aL ? bin_bits(m, 0) : 0u) + bin_bits(mm, 1);
      const double cost = dist[2] + (double)(g >> 15);
      if (cost < best_cost) {
        best_cost = cost, bm = bin_next(mm, 1), bt = t, bf = g;
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c ? en1 : en0) cur[c] = up[c], cur[c].left = 0, cur[c].up = 1;
      }
    }
    no_sao0 += cur[0].type < 0 ? 1 : 0; // :1751-1759
    no_sao1 += cur[1].type < 0 ? 2 : 0;
    m = bm, t = bt, f = bf & 32767; // :1780-1781
#pragma unroll
    for (int c = 0; c < 3; c++) {
      left[c] = cur[c];
      if (lane == c) { // three lanes, one component each
        s_row[c * cw + x] = sao_pack(cur[c]);
        hmx_sao_unit u;
        u.type = (int8_t)cur[c].type, u.sub = (uint8_t)cur[c].sub, u.merge_left = (uint8_t)cur[c].left, u.merge_up = (uint8_t)cur[c].up;
        hmx_sao_lcu l;
        const bool on = c ? en1 : en0;
        l.type = on ? u.type : (int8_t)-1, l.band = on && cur[c].type == 4 ? u.sub : (uint8_t)0;
        for (int k = 0; k < 4; k++) {
          u.offset[k] = (int8_t)(cur[c].off >> (8 * k));
          l.offset[k] = on ? (int8_t)(u.offset[k] * (1 << K.bi)) : (int8_t)0;
        }
        units[(size_t)c * n + a] = u;
        if (apply) apply[(size_t)c * n + a] = l;
      }
    }
    allow_cur = allow_next;
    if (++x == cw) x = 0, y++;
    __syncthreads(); // the row entry and this slot are rewritten after every lane has read them
  }
  if (lane == 0) A.res[pic] = hmx_sao_result{{no_sao0, no_sao1}, {(uint8_t)m, (uint8_t)t}, {0, 0}, f};
}
} // namespace

// ---- host ----
static int sao_decide_check(hmx_ctx *c, const char *fn, int n_pics, int pic_w, int pic_h, const hmx_sao_decide_param *params) {
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, std::string(fn) + ": n_pics must be 1..65535");
  if (pic_w <= 0 || pic_h <= 0 || pic_w % 8 || pic_h % 8) return fail(c, HMX_ERR_ARG, std::string(fn) + ": picture size must be a positive multiple of 8");
  if (c->cfg.bit_depth < 8 || c->cfg.bit_depth > 12) return fail(c, HMX_ERR_ARG, std::string(fn) + ": the context's bit depth must be 8..12");
  for (int i = 0; i < n_pics; i++) {
    const hmx_sao_decide_param &p = params[i];
    if (!(std::isfinite(p.lambda_luma) && p.lambda_luma > 0 && std::isfinite(p.lambda_chroma) && p.lambda_chroma > 0))
      return fail(c, HMX_ERR_ARG, std::string(fn) + ": params[" + std::to_string(i) + "]: a lambda is not finite and positive");
    if (p.ctx_state[0] > 127 || p.ctx_state[1] > 127)
      return fail(c, HMX_ERR_ARG, std::string(fn) + ": params[" + std::to_string(i) + "]: a context state above 127");
    if (p.frac > 32767) return fail(c, HMX_ERR_ARG, std::string(fn) + ": params[" + std::to_string(i) + "]: a fraction above 32767");
  }
  return HMX_OK;
}

extern "C" int hmx_sao_decide_multi(hmx_ctx *c, int n_pics, const hmx_sao_stat *d_stats, int pic_w, int pic_h, const hmx_sao_decide_param *params,
                                    const uint8_t *d_merge_allow, hmx_sao_unit *d_units, hmx_sao_lcu *d_apply, hmx_sao_result *d_result) {
  if (!c || !d_stats || !params || !d_units || !d_result) return fail(c, HMX_ERR_ARG, "hmx_sao_decide_multi: null argument");
  if (int r = sao_decide_check(c, "hmx_sao_decide_multi", n_pics, pic_w, pic_h, params)) return r;
  const int ctu = c->cfg.ctu_size, cw = (pic_w + ctu - 1) / ctu, n_lcu = cw * ((pic_h + ctu - 1) / ctu);
  if (int r = grow_dev(c, &c->d_saodec, &c->saodec_cap, sizeof(SaoCand) * 3 * (size_t)n_lcu * (size_t)n_pics, "SAO candidate records")) return r;
  const hmx_sao_decide_param *d_pp =
      static_cast<const hmx_sao_decide_param *>(arena_push(c, params, sizeof(hmx_sao_decide_param) * (size_t)n_pics));
  if (!d_pp) return fail(c, HMX_ERR_NOMEM, "argument arena");
  SaoCand *cand = static_cast<SaoCand *>(c->d_saodec);
  const bool tm = c->timing && c->tev[0]; // hmx_set_timing: the two kernels apart (hmx_last_call_timing: candidates, decision, 0)
  if (tm) HIPCHK(c, hipEventRecord(c->tev[0], c->stream));
  hipLaunchKernelGGL(k_sao_cand, dim3((unsigned)n_lcu, 3, (unsigned)n_pics), dim3(64), 0, c->stream,
                     SaoCandArgs{d_stats, d_pp, cand, n_lcu, c->cfg.bit_depth});
  if (tm) HIPCHK(c, hipEventRecord(c->tev[1], c->stream));
  hipLaunchKernelGGL(k_sao_decide, dim3((unsigned)n_pics), dim3(64), sizeof(u64) * 3 * (size_t)cw, c->stream,
                     SaoDecArgs{d_stats, cand, d_pp, d_merge_allow, d_units, d_apply, d_result, n_lcu, cw, c->cfg.bit_depth});
  if (tm) {
    HIPCHK(c, hipEventRecord(c->tev[2], c->stream));
    HIPCHK(c, hipEventRecord(c->tev[3], c->stream));
    c->tev_valid = true, c->tev_prep_valid = false;
  }
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_sao_decide(hmx_ctx *c, const hmx_sao_stat *d_stats, int pic_w, int pic_h, const hmx_sao_decide_param *param,
                              const uint8_t *d_merge_allow, hmx_sao_unit *d_units, hmx_sao_lcu *d_apply, hmx_sao_result *d_result) {
  return hmx_sao_decide_multi(c, 1, d_stats, pic_w, pic_h, param, d_merge_allow, d_units, d_apply, d_result);
}

extern "C" int hmx_sao_encode_multi(hmx_ctx *c, int n_pics, const hmx_pic *org, const hmx_pic *rec, const hmx_pic *out, int pic_w, int pic_h,
                                    const hmx_sao_decide_param *params, const uint8_t *d_merge_allow, const uint8_t *d_avail,
                                    hmx_sao_stat *d_stats, hmx_sao_unit *d_units, hmx_sao_lcu *d_apply, hmx_sao_result *d_result) {
  if (!c || !org || !rec || !out || !params || !d_stats || !d_units || !d_apply || !d_result)
    return fail(c, HMX_ERR_ARG, "hmx_sao_encode_multi: null argument");
  if (int r = sao_decide_check(c, "hmx_sao_encode_multi", n_pics, pic_w, pic_h, params)) return r;
  for (int i = 0; i < n_pics; i++)
    for (int p = 0; p < 3; p++) {
      if (!org[i].plane[p] || !rec[i].plane[p] || !out[i].plane[p]) return fail(c, HMX_ERR_ARG, "hmx_sao_encode_multi: null plane");
      if (rec[i].plane[p] == out[i].plane[p]) return fail(c, HMX_ERR_ARG, "hmx_sao_encode_multi: rec and out must be different pictures");
    }
  const int ctu = c->cfg.ctu_size, n_lcu = ((pic_w + ctu - 1) / ctu) * ((pic_h + ctu - 1) / ctu);
  if (int r = d_avail ? hmx_sao_stats_multi_avail(c, n_pics, org, rec, pic_w, pic_h, d_avail, d_stats)
                      : hmx_sao_stats_multi(c, n_pics, org, rec, pic_w, pic_h, 1, d_stats))
    return r;
  if (int r = hmx_sao_decide_multi(c, n_pics, d_stats, pic_w, pic_h, params, d_merge_allow, d_units, d_apply, d_result)) return r;
  return d_avail ? hmx_sao_picture_multi_avail(c, n_pics, rec, out, pic_w, pic_h, d_apply, n_lcu, d_avail)
                 : hmx_sao_picture_multi(c, n_pics, rec, out, pic_w, pic_h, d_apply, n_lcu);
}

// ---- host helpers, no context ----
extern "C" int hmx_sao_ctx_init(int slice_type, int qp, uint8_t *state) {
  static const int kInitMerge[3] = {153, 153, 153}, kInitType[3] = {200, 185, 160}; // ContextTables.h:383-388, :414-419; rows B, P, I
  if (!state || slice_type < 0 || slice_type > 2) return HMX_ERR_ARG;
  qp = std::min(51, std::max(0, qp)); // ContextModel::init, ContextModel.cpp:56-65
  const int init[2] = {kInitMerge[slice_type], kInitType[slice_type]};
  for (int i = 0; i < 2; i++) {
    const int slope = (init[i] >> 4) * 5 - 45, offset = ((init[i] & 15) << 3) - 16;
    const int s = std::min(std::max(1, ((slope * qp) >> 4) + offset), 126), mps = s >= 64;
    state[i] = (uint8_t)(((mps ? s - 64 : 63 - s) << 1) + mps);
  }
  return HMX_OK;
}
extern "C" int hmx_sao_rate_flags(const hmx_sao_rate_state *state, int depth, uint8_t *enable) {
  if (!state || !enable || depth < 0 || depth >= HMX_SAO_RATE_DEPTHS) return HMX_ERR_ARG;
  enable[0] = !(depth > 0 && state->rate[0][depth - 1] > 0.75); // SAO_ENCODING_RATE, :1503-1506
  enable[1] = !(depth > 0 && state->rate[1][depth - 1] > 0.5);  // SAO_ENCODING_RATE_CHROMA, :1507-1513
  return HMX_OK;
}
extern "C" int hmx_sao_rate_update(hmx_sao_rate_state *state, int depth, const uint32_t *num_no_sao, int n_ctu) {
  if (!state || !num_no_sao || depth < 0 || depth >= HMX_SAO_RATE_DEPTHS || n_ctu < 1) return HMX_ERR_ARG;
  state->rate[0][depth] = num_no_sao[0] / ((double)n_ctu);     // :1788
  state->rate[1][depth] = num_no_sao[1] / ((double)n_ctu * 2); // :1789
  return HMX_OK;
}
extern "C" int hmx_sao_merge_allow(int pic_w, int pic_h, int ctu, const uint32_t *slice_id, const uint32_t *tile_id, uint8_t *out) {
  if (!slice_id || !out || pic_w <= 0 || pic_h <= 0 || ctu <= 0) return HMX_ERR_ARG;
  const int cw = (pic_w + ctu - 1) / ctu, ch = (pic_h + ctu - 1) / ctu;
  for (int a = 0; a < cw * ch; a++) { // :1536-1562
    const auto same = [&](int b) { return slice_id[a] == slice_id[b] && (!tile_id || tile_id[a] == tile_id[b]); };
    out[a] = (uint8_t)((a % cw && same(a - 1) ? 1 : 0) | (a >= cw && same(a - cw) ? 2 : 0));
  }
  return HMX_OK;
}
