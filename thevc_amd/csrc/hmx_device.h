// hmx_device.h -- device-side building blocks of libhmx (gfx950).
//
// Work decomposition used by every block kernel: a block (TU) of N x N samples is owned by a group
// of N consecutive lanes of one wavefront; lane r keeps one row (or one column) of the block in
// registers.  The two 1-D passes of a separable transform run entirely in registers, the N x N
// transposition between them goes through a padded LDS tile.  64/N blocks share a wavefront
// (16 4x4, 8 8x8, 4 16x16, 2 32x32), so all cross-lane traffic of a block stays inside a wave.
//
// Arithmetic contract (bit-exact with the reference, see include/hmx.h for file:line):
//   forward pass  y[k] = wrap16((sum_n M[k][n] x[n] + rnd) >> shift)      TComTrQuant.cpp:417-795
//   inverse pass  y[n] = clip16((sum_k M[k][n] c[k] + rnd) >> shift)
// The even/odd recursion (hmx_transform.h) is an exact integer factorisation of those sums (no overflow:
// |sum| < 2^27), so the result equals the reference's partial butterflies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hmx_sbh.h"
#include "hmx_transform.h"

namespace hmx {

__device__ __forceinline__ int clip3(int lo, int hi, int v) { return min(max(v, lo), hi); }
// The median of three in one instruction (v_med3_i32): with lo <= hi it is clip3(lo, hi, v).  The compiler forms it from min(max())
// only when both bounds are constants.  med3k: v is a constant the instruction takes inline (-16 .. 64).
__device__ __forceinline__ int med3i(int v, int lo, int hi) {
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v), "v"(lo), "v"(hi));
  return r;
}
template <int K>
__device__ __forceinline__ int med3k(int lo, int hi) {
  static_assert(K >= -16 && K <= 64, "an inline constant");
  int r;
  asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "n"(K), "v"(lo), "v"(hi));
  return r;
}
// Full-rate integer multiplies (v_mul_i32_i24 / v_mad_i32_i24 / v_mul_u32_u24; the plain 32-bit multiply
// v_mul_lo_u32 is a quarter-rate instruction).  Both operands must fit 24 bits; the result is the
// exact low 32 bits of the product.  Every use states why its operands fit.
__device__ __forceinline__ int mul24(int a, int b) { return __mul24(a, b); }
__device__ __forceinline__ unsigned umul24(unsigned a, unsigned b) { return __umul24(a, b); }
__device__ __forceinline__ int wrap16(int v) { return (int)(short)v; }
// a - b as its low 17 bits, sign-extended (one v_bfe_i32): the difference itself for int16 a and b, and a value the instruction
// selector knows to fit 24 bits, whatever the words hold
__device__ __forceinline__ int diff17(int a, int b) { return (int)(((unsigned)a - (unsigned)b) << 15) >> 15; }

// The 1-D transforms on register arrays (dct_coef, dst_coef, fwd_pass, inv_pass): hmx_transform.h, shared with the host.

// ---------------------------------------------------------------------------------------------
// Quantiser parameters (host-prepared, one set per plane type) and scan tables
// ---------------------------------------------------------------------------------------------
struct QuantDev {
  int q;          // g_quantScales[rem]
  int per_qbits;  // per used for iQBits (slice base QP)
  int iq_scale;   // g_invQuantScales[rem] << per
  int rnd_factor; // 171 (I) or 85
};

struct PicDev { // parameters shared by the block kernels
  int pic_w, pic_h; // luma
  int ctu;          // 64
  int bit_depth;
  int sign_hide;
  QuantDev qd[2];   // [0] luma, [1] chroma
};

// P.qd[luma ? 0 : 1] by value.  The parameters live in the kernel-argument segment; a select between two
// references makes the compiler select the ADDRESS and fetch every field with a per-lane load from that
// segment.  Here both sets arrive as scalars (v_readfirstlane pins them) and the lane selects values.
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <typename T>
__device__ __forceinline__ T *wave_uniform(T *p) {
  const unsigned long long u = (unsigned long long)p;
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32));
  return (T *)((unsigned long long)lo | ((unsigned long long)hi << 32));
}
__device__ __forceinline__ QuantDev pick_qd(const PicDev &P, bool luma) {
  const int a0 = wave_uniform(P.qd[0].q), a1 = wave_uniform(P.qd[0].per_qbits), a2 = wave_uniform(P.qd[0].iq_scale),
            a3 = wave_uniform(P.qd[0].rnd_factor);
  const int b0 = wave_uniform(P.qd[1].q), b1 = wave_uniform(P.qd[1].per_qbits), b2 = wave_uniform(P.qd[1].iq_scale),
            b3 = wave_uniform(P.qd[1].rnd_factor);
  return QuantDev{luma ? a0 : b0, luma ? a1 : b1, luma ? a2 : b2, luma ? a3 : b3};
}

// A QP per block (hmx_set_qp_map): the caller's map holds one luma QP per 4x4 luma unit, a block takes the unit at its first sample
// (TComDataCU::getQP of its coding unit).  The host builds tab[qp + off][0 luma, 1 chroma] for every legal QP of the call, the chroma
// entry through hmx_setQPforQuant, and a block reads its map byte and its table entry ONCE, next to its descriptor.  The byte is
// clamped to -off .. 51 before it indexes the table, and the unit to the map: device memory the host cannot validate.
// The block routines are templates over the type of their picture parameters.  PicDev: the constants are wave-uniform (pick_qd
// above), the form every call without a map instantiates.  PicDevLane: a copy whose qd[0] holds the constants of this lane's block.
struct QuantPk { // a table entry, and what a lane of the persistent kernel keeps beside its item: two registers
  int q_per; // g_quantScales[rem] | per << 16
  int iq_scale;
};
struct QpMapDev {
  const signed char *map; // [n][uh][uw]
  const QuantPk *tab;     // [52 + off][2]; the rounding factor is the slice's, PicDev::qd[0].rnd_factor
  long long pic_elems;    // uh * uw, or 0: one map for every picture
  int uw, uh, off;        // units per row and column, QpBDOffset
};
struct PicDevLane : PicDev {};
__device__ __forceinline__ QuantDev pick_qd(const PicDevLane &P, bool) { return P.qd[0]; }
// (lx, ly): the block's first sample in luma coordinates
__device__ __forceinline__ QuantPk qp_map_qd(const QpMapDev &M, int pic, int lx, int ly, bool luma) {
  typedef __attribute__((address_space(1))) const signed char gbyte;
  typedef int i2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(1))) const i2 gq;
  const int ux = min(max(lx >> 2, 0), M.uw - 1), uy = min(max(ly >> 2, 0), M.uh - 1);
  const int qp = ((gbyte *)M.map)[(long long)pic * M.pic_elems + uy * M.uw + ux];
  const int e = (min(max(qp, -M.off), 51) + M.off) * 2 + (luma ? 0 : 1);
  const i2 v = ((gq *)M.tab)[e];
  return QuantPk{v[0], v[1]};
}
// the parameters a kernel hands its block routines: the call's own (no map), or the lane's copy
template <bool QMAP>
__device__ __forceinline__ const auto &pick_pd(const PicDev &call, const PicDevLane &lane) {
  if constexpr (QMAP) return lane;
  else return call;
}
__device__ __forceinline__ PicDevLane lane_picdev(const PicDev &P, const QuantPk &k) {
  PicDevLane L;
  L.pic_w = P.pic_w, L.pic_h = P.pic_h, L.ctu = P.ctu, L.bit_depth = P.bit_depth, L.sign_hide = P.sign_hide; // (field by field: a struct copy leaves a stack object behind)
  L.qd[0] = L.qd[1] = QuantDev{k.q_per & 0xffff, k.q_per >> 16, k.iq_scale, wave_uniform(P.qd[0].rnd_factor)};
  return L;
}

// Scan tables g_auiSigLastScan (TComRom.cpp:564-698 with REMOVAL_8x2_2x8_CG): coefficient groups
// of 4x4, groups ordered like the samples inside a group.  Index 0 = diagonal (also used for the
// reference's "zigzag" index, TComTrQuant.cpp:1135), 1 = horizontal, 2 = vertical.  Entry = raster
// position inside the N x N block.  Built at compile time, kept in constant memory.
__host__ __device__ constexpr int diag_xy(int W, int i) { // i-th position of the up-right diagonal scan of a WxW grid -> y*W+x
  int c = 0;
  for (int d = 0; d <= 2 * W - 2; d++)
    for (int x = (d < W ? 0 : d - W + 1); x <= d && x < W; x++) {
      if (c == i) return (d - x) * W + x;
      c++;
    }
  return 0;
}
template <int N, typename T>
struct ScanTab {
  T t[3][N * N];
  constexpr ScanTab() : t{} {
    constexpr int G = N / 4;
    for (int sc = 0; sc < 3; sc++)
      for (int g = 0; g < G * G; g++)
        for (int i = 0; i < 16; i++) {
          int gy = 0, gx = 0, y = 0, x = 0;
          if (sc == 1) {
            gy = g / G, gx = g % G, y = i >> 2, x = i & 3;
          } else if (sc == 2) {
            gx = g / G, gy = g % G, x = i >> 2, y = i & 3;
          } else {
            int gp = diag_xy(G, g), ip = diag_xy(4, i);
            gy = gp / G, gx = gp % G, y = ip >> 2, x = ip & 3;
          }
          t[sc][g * 16 + i] = (T)((gy * 4 + y) * N + gx * 4 + x);
        }
  }
};
static __constant__ ScanTab<4, unsigned char> kScan4 = ScanTab<4, unsigned char>();
static __constant__ ScanTab<8, unsigned char> kScan8 = ScanTab<8, unsigned char>();
static __constant__ ScanTab<16, unsigned char> kScan16 = ScanTab<16, unsigned char>();
static __constant__ ScanTab<32, unsigned short> kScan32 = ScanTab<32, unsigned short>();

// the 16 raster positions of coefficient group g in scan order, kept PACKED as loaded (one or two
// 16-byte loads: 4 dwords of bytes, or 8 dwords of halfwords for 32x32) -- they stay live across the
// sign-hiding decision, so their register footprint matters
template <int N>
struct ScanPos {
  static constexpr int W = N == 32 ? 8 : 4;
  unsigned pk[W];
  __device__ __forceinline__ void load(int scan_idx, int g) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    if constexpr (N == 32) {
      const u4 *p = reinterpret_cast<const u4 *>(&kScan32.t[scan_idx][g * 16]);
      const u4 a = p[0], b = p[1];
#pragma unroll
      for (int q = 0; q < 4; q++) pk[q] = a[q], pk[4 + q] = b[q];
    } else {
      const unsigned char *base = N == 4 ? &kScan4.t[scan_idx][g * 16] : N == 8 ? &kScan8.t[scan_idx][g * 16] : &kScan16.t[scan_idx][g * 16];
      const u4 a = *reinterpret_cast<const u4 *>(base);
#pragma unroll
      for (int q = 0; q < 4; q++) pk[q] = a[q];
    }
  }
  __device__ __forceinline__ int at(int i) const { // i: compile-time constant after unrolling
    if constexpr (N == 32) return (pk[i >> 1] >> (16 * (i & 1))) & 0xffff;
    else return (pk[i >> 2] >> (8 * (i & 3))) & 255;
  }
  __device__ __forceinline__ int at_dyn(int i) const { // i: run-time index
    unsigned d = 0;
    if constexpr (N == 32) {
#pragma unroll
      for (int q = 0; q < 8; q++) d = (i >> 1) == q ? pk[q] : d;
      return (d >> (16 * (i & 1))) & 0xffff;
    } else {
#pragma unroll
      for (int q = 0; q < 4; q++) d = (i >> 2) == q ? pk[q] : d;
      return (d >> (8 * (i & 3))) & 255;
    }
  }
};

// getCoefScanIdx (TComDataCU.cpp:4014-4063); 0 (zigzag) is used as diagonal by xQuant
__device__ __forceinline__ int coef_scan_idx(int N, bool luma, bool intra, int mode) {
  if (!intra) return 0;
  bool multi = luma ? (N == 4 || N == 8) : (N == 4);
  if (!multi) return 0;
  if (abs(mode - 26) < 5) return 1;
  if (abs(mode - 10) < 5) return 2;
  return 0;
}

// The 16 words of a 4x4 group in raster order (k = 4 y + x) -> scan order (0 diagonal, 1 horizontal, 2 vertical).  The scan differs
// per lane, but there are only three of them: scan entry k of each is a compile-time register, so the reorder is two selects per entry.
__device__ __forceinline__ void scan4_order(const int *w, int scan_idx, int *ws) {
  constexpr int dg[16] = {0, 4, 1, 8, 5, 2, 12, 9, 6, 3, 13, 10, 7, 14, 11, 15};
  const bool hor = scan_idx == 1, ver = scan_idx == 2;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int d = w[dg[k]], hv = w[k], vv = w[((k & 3) << 2) | (k >> 2)];
    ws[k] = hor ? hv : (ver ? vv : d);
  }
}
// raster position of scan entry i (run-time i)
__device__ __forceinline__ int scan4_raster(int scan_idx, int i) {
  const int bd = (int)((0xfbe7ad369c258140ull >> (4 * i)) & 15); // dg[i], one nibble per entry
  return scan_idx == 1 ? i : (scan_idx == 2 ? (((i & 3) << 2) | (i >> 2)) : bd);
}

// LDS scratch of one block.  tile: transposition buffer, then the quantiser's packed words
//   bits 0..15  level (signed)      bits 16..31  (deltaU << 1) | (unquantised coefficient < 0)
// i.e. everything sign-bit hiding reads about a coefficient in one word.
template <int N>
struct TuLds {
  int tile[N][N + 1];
  int me[3 * N + 2]; // extended main reference of the angular modes, me[N + k] = refMain[k], k = -N..2N
  int line[4 * N + 2];
  int fline[4 * N + 2];
  unsigned nzmask[2]; // bit g: coefficient group g (scan order) holds a non-zero level
};

// The scratch of an 8x8 block worked by FOUR lanes, sixteen blocks per wave (wave_chain_8x2): the extended main reference is
// spent when the prediction is formed and the tile is first written behind it, so they share memory -- 568 bytes per block, 9 KB
// per wave (sixteen TuLds<8> would be 10.5 KB, and sixteen waves per CU have 10 KB each).
struct TuLds8x2 {
  union {
    int tile[8][9];
    int me[3 * 8 + 2];
  };
  int line[4 * 8 + 2];
  int fline[4 * 8 + 2];
  unsigned nzmask[2];
};

__device__ __forceinline__ int level_of(int word) { return (int)(short)word; }

// Flat quantisation of one coefficient (TComTrQuant.cpp:1241-1259) -> packed word.  WIDE = false is
// for coefficients known to lie in [-32768, 32768] (anything that went through a forward pass or
// transform skip): |c| * q < 2^30 and every intermediate fits 32 bits, identical results.
template <bool WIDE>
__device__ __forceinline__ int quant_one(int c, int q, int qbits, int rnd_factor, int &abs_level) {
  int l, du;
  if (WIDE) {
    const long long t = (long long)abs(c) * q, add = (long long)rnd_factor << (qbits - 9);
    l = (int)((t + add) >> qbits);
    du = (int)((t - ((long long)l << qbits)) >> (qbits - 8));
  } else {
    const unsigned t = umul24((unsigned)abs(c), (unsigned)q), add = (unsigned)rnd_factor << (qbits - 9); // |c| <= 2^15, q < 2^15
    l = (int)((t + add) >> qbits);
    du = ((int)t - (l << qbits)) >> (qbits - 8);
  }
  abs_level = l;
  const int level = clip3(-32768, 32767, c < 0 ? -l : l);
  return (level & 0xffff) | ((du << 1 | (c < 0 ? 1 : 0)) << 16);
}

// Sign-bit hiding of one coefficient group (select16, sbh_pick, sbh_apply): hmx_sbh.h, shared with the host.

// ---------------------------------------------------------------------------------------------
// Intra reference samples and prediction
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned zorder4(unsigned cx, unsigned cy) { // 4-bit coordinates
  unsigned z = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) z |= ((cx >> b) & 1u) << (2 * b) | ((cy >> b) & 1u) << (2 * b + 1);
  return z;
}

// Availability mask of the 4n+1 neighbour units of a block at luma (x,y), luma size `size`
// (TComPattern.cpp:607-786 + TComDataCU.cpp:1221-1735; one slice, one tile, no constrained intra):
// bit u follows the bNeighborFlags order: below-left (bottom first), left, corner, above, above-right.
__host__ __device__ __forceinline__ unsigned long long intra_avail_mask(int x, int y, int size, const PicDev &P) {
  int n = size >> 2, U = P.ctu >> 2;
  int cx = (x & (P.ctu - 1)) >> 2, cy = (y & (P.ctu - 1)) >> 2;
  unsigned long long m = 0;
  if (x > 0 && y > 0) m |= 1ull << (2 * n);
  if (y > 0) m |= ((1ull << n) - 1) << (2 * n + 1);
  if (x > 0) m |= ((1ull << n) - 1) << n;
  int rx = cx + n - 1, by = cy + n - 1;
  int ctu_col = x / P.ctu, ctu_cols = (P.pic_w + P.ctu - 1) / P.ctu;
  for (int o = 1; o <= n; o++) {
    bool a;
    if (x + size - 4 + 4 * o >= P.pic_w)
      a = false;
    else if (rx + o < U)
      a = cy > 0 ? (zorder4(rx, cy) > zorder4(rx + o, cy - 1)) : (y > 0);
    else
      a = (cy == 0) && y > 0 && ctu_col < ctu_cols - 1;
    if (a) m |= 1ull << (3 * n + o);
    bool b;
    if (y + size - 4 + 4 * o >= P.pic_h)
      b = false;
    else if (by + o < U)
      b = cx > 0 ? (zorder4(cx, by) > zorder4(cx - 1, by + o)) : (x > 0);
    else
      b = false;
    if (b) m |= 1ull << (n - o);
  }
  return m;
}

// The same mask in closed form (no loop over the units; the plan kernels form it for every block of every picture).  The n
// above-right units of an n-aligned block lie in ONE n-aligned neighbour position (a + 1, b - 1) in units of n, so inside the
// CTU they share one answer: is that position earlier in Z-order?  The most significant differing Morton bit decides: the y bit
// at ctz(b) (set in b, clear in b - 1) against the x bit at cto(a) = trailing ones of a (clear in a, set in a + 1); y bits
// outrank x bits of the same position, so the neighbour precedes iff ctz(b) >= cto(a).  Below-left, (a - 1, b + 1): the y bit at
// cto(b) (clear in b) against the x bit at ctz(a) (set in a): the neighbour precedes iff cto(b) < ctz(a).  The picture's right and
// lower edges then cut the runs.  CTU size 64; held against intra_avail_mask at every position by tests/test_intra_dependencies.py.
__host__ __device__ __forceinline__ unsigned long long intra_avail_mask_fast(int x, int y, int size, const PicDev &P) {
  const int n = size >> 2, lgn = n == 1 ? 0 : n == 2 ? 1 : n == 4 ? 2 : 3;
  const int cx = (x & 63) >> 2, cy = (y & 63) >> 2;
  const unsigned a = (unsigned)cx >> lgn, b = (unsigned)cy >> lgn;
  const unsigned long long run = (1ull << n) - 1;
  unsigned long long m = 0;
  if (x > 0 && y > 0) m |= 1ull << (2 * n);
  if (y > 0) m |= run << (2 * n + 1);
  if (x > 0) m |= run << n;
#if defined(__HIP_DEVICE_COMPILE__)
  const int ctz_a = __ffs((int)(a | 16u)) - 1, ctz_b = __ffs((int)(b | 16u)) - 1, cto_a = __ffs((int)(~a)) - 1, cto_b = __ffs((int)(~b)) - 1;
#else
  const int ctz_a = __builtin_ctz(a | 16u), ctz_b = __builtin_ctz(b | 16u), cto_a = __builtin_ctz(~a), cto_b = __builtin_ctz(~b);
#endif
  bool ar;
  if (cx + n < 16) ar = cy > 0 ? ctz_b >= cto_a : y > 0;
  else ar = cy == 0 && y > 0 && (x >> 6) < ((P.pic_w + 63) >> 6) - 1;
  if (ar) {
    int k = (P.pic_w - x - size + 3) >> 2; // units of the run that start inside the picture
    k = k < 0 ? 0 : k > n ? n : k;
    m |= ((1ull << k) - 1) << (3 * n + 1);
  }
  const bool bl = cy + n < 16 && (cx > 0 ? cto_b < ctz_a : x > 0);
  if (bl) {
    int k = (P.pic_h - y - size + 3) >> 2;
    k = k < 0 ? 0 : k > n ? n : k;
    m |= ((1ull << k) - 1) << (n - k); // below-left counts upwards from the bottom: the k units nearest the block
  }
  return m;
}

// The same for a 64 x 64 LUMA block = a whole CTU (the prediction unit of a 64 x 64 coding unit, TEncSearch.cpp:2509-2540:
// initAdiPattern and the 35 modes run at the PU size; no transform of that size exists).  4n + 1 = 65 units of four samples
// do not fit the 64-bit mask, and need not: below-left of a CTU is never coded before it, left / above are all-or-nothing,
// and the picture's right edge cuts the above-right CTU at a multiple of the minimum CU size (8).  So the mask is kept in
// units of EIGHT samples (n = 8, 33 bits, same bit order); build_ref_line takes the unit size as an argument.
__host__ __device__ __forceinline__ unsigned long long intra_avail_mask_ctu(int x, int y, const PicDev &P) {
  unsigned long long m = 0;
  if (x > 0 && y > 0) m |= 1ull << 16;
  if (x > 0) m |= 0xffull << 8;
  if (y > 0) {
    m |= 0xffull << 17;
    for (int o = 0; o < 8; o++)
      if (x + 64 + 8 * o < P.pic_w) m |= 1ull << (25 + o);
  }
  return m;
}

// Slices, tiles and constrained intra prediction (hmx_avail_layout, packed by the host entry points).  A region is one
// (independent slice, tile) pair; CTUs see each other only inside their region (TComDataCU.cpp:1221-1735: getPU* with
// bEnforceSliceRestriction / the getTileIdxMap checks; TComPattern calls them with bEnforceDependentSliceRestriction = false,
// so dependent slices do not split regions).  With constrained_intra_pred_flag a neighbour unit that is not intra-coded is
// unavailable (TComPattern.cpp:607-786, isAbove/Left/AboveLeft...Available).  The intra flags are kept twice, bit-packed along
// unit rows (the above run of a block is one 64-bit window) and along unit columns (the left run likewise).
struct AvailDev {
  const uint32_t *region; // region id per CTU, raster order; NULL = one region
  const uint32_t *rows;   // intra flag of 4x4 luma unit (ux, uy): bit ux & 31 of rows[uy * row_words + (ux >> 5)]; NULL = CIP off
  const uint32_t *cols;   // the same transposed: bit uy & 31 of cols[ux * col_words + (uy >> 5)]
  int row_words, col_words;
  int cw, ctu_log2; // CTUs per row, log2 of the CTU size
};
// 64 bits of a packed line from bit `pos` on (at least 33 of them; bits past the line's end read as 0)
__host__ __device__ __forceinline__ unsigned long long avail_bits64(const uint32_t *line, int words, int pos) {
  const int w = pos >> 5, s = pos & 31;
  unsigned long long v = w < words ? line[w] : 0u;
  if (w + 1 < words) v |= (unsigned long long)line[w + 1] << 32;
  return v >> s;
}
__host__ __device__ __forceinline__ unsigned avail_even_bits(unsigned long long v) { // bits 0, 2, 4, .. 62 -> 0 .. 31
  v &= 0x5555555555555555ull;
  v = (v | (v >> 1)) & 0x3333333333333333ull;
  v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0full;
  v = (v | (v >> 4)) & 0x00ff00ff00ff00ffull;
  v = (v | (v >> 8)) & 0x0000ffff0000ffffull;
  return (unsigned)(v | (v >> 16));
}
__host__ __device__ __forceinline__ unsigned avail_rev32(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __brev(v);
#else
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  return (v >> 16) | (v << 16);
#endif
}
// The geometric mask m of a block at luma (x, y), luma size `size`, in units of 1 << ulog2 luma samples (2: the 4n + 1 units of
// intra_avail_mask, 3: the 64 x 64 prediction unit of intra_avail_mask_ctu), cut down to the layout: a subset of m, never more
// (a unit that geometry says is not yet coded stays unavailable, so every schedule built on m stays valid).  At most four region
// lookups (left, above-left, above, above-right CTU) and three windows of the intra bitmaps.
__host__ __device__ __forceinline__ unsigned long long intra_avail_mask_layout(unsigned long long m, int x, int y, int size, int ulog2,
                                                                              const AvailDev &L) {
  const int n = size >> ulog2, cl = L.ctu_log2;
  const unsigned long long left_run = (1ull << (2 * n)) - 1, corner = 1ull << (2 * n), above_run = ((1ull << (2 * n)) - 1) << (2 * n + 1);
  if (L.region && m) {
    const int cx = x >> cl, cy = y >> cl;
    const uint32_t r = L.region[cy * L.cw + cx];
    // left and below-left: the available ones lie in the CTU row of the block, in CTU ((x - 1) >> cl)
    if ((m & left_run) && ((x - 1) >> cl) != cx && L.region[cy * L.cw + cx - 1] != r) m &= ~left_run;
    if (m & corner) {
      const int ax = (x - 1) >> cl, ay = (y - 1) >> cl;
      if ((ax != cx || ay != cy) && L.region[ay * L.cw + ax] != r) m &= ~corner;
    }
    if ((m & above_run) && ((y - 1) >> cl) != cy) { // the above run in the CTU row above: CTU cx, then cx + 1 (above-right)
      const int ay = (y - 1) >> cl, k = (((cx + 1) << cl) - x) >> ulog2; // units of the run above CTU cx
      const unsigned long long own = k >= 2 * n ? above_run : (((1ull << k) - 1) << (2 * n + 1));
      if ((m & own) && L.region[ay * L.cw + cx] != r) m &= ~own;
      if ((m & above_run & ~own) && L.region[ay * L.cw + cx + 1] != r) m &= ~(above_run & ~own);
    }
  }
  if (L.rows && m) {
    const int ux = x >> 2, uy = y >> 2, run = 2 * n;
    unsigned long long keep = 0;
    if (y > 0) { // above and above-right: unit row uy - 1 from column ux
      const unsigned long long a = avail_bits64(L.rows + (size_t)(uy - 1) * L.row_words, L.row_words, ux);
      keep |= ((ulog2 == 3 ? (unsigned long long)avail_even_bits(a) : a) & left_run) << (2 * n + 1);
    }
    if (x > 0) { // left and below-left: unit column ux - 1 from row uy; the mask counts from the bottom
      const unsigned long long l = avail_bits64(L.cols + (size_t)(ux - 1) * L.col_words, L.col_words, uy);
      const unsigned v = (unsigned)((ulog2 == 3 ? (unsigned long long)avail_even_bits(l) : l) & left_run);
      keep |= (unsigned long long)(avail_rev32(v) >> (32 - run));
      if (y > 0 && ((L.rows[(size_t)(uy - 1) * L.row_words + ((ux - 1) >> 5)] >> ((ux - 1) & 31)) & 1u)) keep |= corner;
    }
    m &= keep;
  }
  return m;
}

// Reference line of a block: L[0..4N], L[0] = lowest below-left sample, L[2N] = corner,
// L[4N] = right-most above-right sample (fillReferenceSamples, TComPattern.cpp:368-552).
// Every sample is one independent load: an unavailable sample copies the nearest available
// sample before it (or the first available one for a leading run), which is what the reference's
// sequential padding loop produces.  fetch(dx, dy) returns the reconstructed sample at offset
// (dx, dy) from the block origin (plane or tiled addressing is the caller's business).
template <int N, int NL, typename Fetch>
__device__ __forceinline__ void build_ref_line(Fetch fetch, unsigned long long avail, int unit_log2, int bit_depth, int gl,
                                               int *L) {
  const int unit = 1 << unit_log2, n = N >> unit_log2;
  constexpr int IT = (4 * N + 1 + NL - 1) / NL;
  // two phases, fully unrolled: every load of this lane is issued before the first one is consumed,
  // so the gather costs ONE memory round trip instead of one per sample
  int v[IT];
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int p = gl + it * NL;
    v[it] = 1 << (bit_depth - 1);
    if (p <= 4 * N && avail != 0) {
      int u = p < 2 * N ? (p >> unit_log2) : (p == 2 * N ? 2 * n : 2 * n + 1 + ((p - 2 * N - 1) >> unit_log2));
      int q = p;
      if (!((avail >> u) & 1)) {
        unsigned long long lower = avail & ((1ull << u) - 1);
        if (lower) {
          int u2 = 63 - __clzll((long long)lower); // last sample of the nearest available unit below
          q = u2 < 2 * n ? (u2 << unit_log2) + unit - 1 : (u2 == 2 * n ? 2 * N : 2 * N + ((u2 - 2 * n) << unit_log2));
        } else {
          int u2 = __ffsll((long long)avail) - 1; // first sample of the first available unit
          q = u2 < 2 * n ? (u2 << unit_log2) : (u2 == 2 * n ? 2 * N : 2 * N + 1 + ((u2 - 2 * n - 1) << unit_log2));
        }
      }
      // one address, one load (q always names an available sample)
      const int dx = q < 2 * N ? -1 : (q == 2 * N ? -1 : q - 2 * N - 1);
      const int dy = q < 2 * N ? 2 * N - 1 - q : -1;
      v[it] = fetch(dx, dy);
    }
  }
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int p = gl + it * NL;
    if (p <= 4 * N) L[p] = v[it];
  }
}

template <int N, int NL>
__device__ __forceinline__ void smooth_ref_line(const int *L, int *F, int gl) { // [1 2 1], :265-306
  for (int p = gl; p <= 4 * N; p += NL)
    F[p] = (p == 0 || p == 4 * N) ? L[p] : (L[p - 1] + 2 * L[p] + L[p + 1] + 2) >> 2;
}

__device__ __forceinline__ bool use_filtered_refs(int mode, int log2n) { // TComPattern.cpp:49-56,577-605
  const int thr = log2n == 2 ? 10 : log2n == 3 ? 7 : log2n == 4 ? 1 : log2n == 5 ? 0 : 10; // m_aucIntraFilter: {10, 7, 1, 0, 10 (64x64)}
  if (mode == 1) return false;
  return min(abs(mode - 10), abs(mode - 26)) > thr;
}

// An empty instruction that reads and "rewrites" K values (addresses, or the destinations of loads) held in vector registers:
// every one of them is complete in a register of its own at this point, and nothing that uses one can move above it.
template <int K, typename V>
__device__ __forceinline__ void pin_regs(V *v) {
  if constexpr (K == 1) asm volatile("" : "+v"(v[0]));
  else if constexpr (K == 2) asm volatile("" : "+v"(v[0]), "+v"(v[1]));
  else if constexpr (K == 3) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
  else if constexpr (K == 4) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
  else if constexpr (K == 5) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]));
  else if constexpr (K == 6) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]));
  else {
    pin_regs<6>(v);
    pin_regs<K - 6>(v + 6);
  }
}
// K words of an LDS array at run-time indices, read back to back between two pins: every index is complete before the first
// read, every read has a register of its own, and ONE wait stands behind the last (LDS returns in order; the waits the compiler
// puts in front of the second pin's pieces have no read between them).  Left to itself the compiler waits behind every read.
template <int K>
__device__ __forceinline__ void lds_gather(const int *base, int *idx, int *v) {
  pin_regs<K>(idx);
#pragma unroll
  for (int k = 0; k < K; k++) v[k] = base[idx[k]];
  pin_regs<K>(v);
}
// The same for K adjacent pairs base[idx], base[idx + 1]: one two-word read each
template <int K>
__device__ __forceinline__ void lds_gather_pairs(const int *base, int *idx, int *v0, int *v1) {
  pin_regs<K>(idx);
#pragma unroll
  for (int k = 0; k < K; k++) v0[k] = base[idx[k]], v1[k] = base[idx[k] + 1];
  pin_regs<K>(v0);
  pin_regs<K>(v1);
}

// Angular parameters of a mode (TComPrediction.cpp:196-210)
struct AngParam {
  bool ver;
  int angle, inv_angle;
};
__device__ __forceinline__ AngParam ang_param(int mode) {
  AngParam a;
  a.ver = mode >= 18;
  const int idx = a.ver ? mode - 26 : 10 - mode, aidx = abs(idx);
  constexpr int ang_tab[9] = {0, 2, 5, 9, 13, 17, 21, 26, 32};
  constexpr int inv_tab[9] = {0, 4096, 1638, 910, 630, 482, 390, 315, 256};
  int angle = 0, inv = 0;
#pragma unroll
  for (int i = 0; i < 9; i++)
    if (i == aidx) {
      angle = ang_tab[i];
      inv = inv_tab[i];
    }
  a.angle = idx < 0 ? -angle : angle;
  a.inv_angle = inv;
  return a;
}

// Extended main reference of an angular mode (TComPrediction.cpp:227-258): ME[N + k] = refMain[k].
// k >= 0: the main reference (above for vertical modes, left for horizontal ones); k < 0 (negative
// angles only, down to (N*angle)>>5): the side reference projected with the inverse angle.
// NL lanes of the block fill it together.  R = reference line (top(k) = R[2N+k], left(k) = R[2N-k]).
// OPT (what a caller asks of the prediction, a mask; 0 = the forms every kernel but the packed chain's uses):
//   kPredPairs    the general angular path reads all its tap pairs in one batch (intra_pred_samples)
//   kPredMainRef  this routine fully unrolled in three phases, as the padding pass of refs_gather_pad: every source index without a
//                 branch, all the reads back to back (lds_gather), then the writes, predicated for the entries outside (lim, last];
//                 an entry that is not written reads the corner, R[2N].  As a run-time loop every entry is a read, a wait and a write.
//   kLdsBatch     (the chains themselves, hmx_chain_dev.h) the LDS reads of the level read-back, the level store and the inverse
//                 passes back to back with one wait per batch (pin_regs), where the compiler waits for every word or pair
constexpr int kPredPairs = 1, kPredMainRef = 2, kLdsBatch = 4;
template <int N, int NL, int OPT = 0>
__device__ __forceinline__ void build_main_ref(const int *R, int *ME, int mode, int gl) {
  if (mode < 2) return;
  const AngParam a = ang_param(mode);
  const int lim = a.angle < 0 ? (N * a.angle) >> 5 : 0, last = a.angle < 0 ? N : 2 * N;
  if constexpr (!(OPT & kPredMainRef)) {
    for (int e = gl; e <= 3 * N; e += NL) {
      const int k = e - N;
      if (k > last || (k < 0 && k <= lim)) continue;
      int v;
      if (k >= 0)
        v = a.ver ? R[2 * N + k] : R[2 * N - k];
      else {
        const int j = (128 + mul24(-k, a.inv_angle)) >> 8; // k >= -32, inv_angle <= 4096
        v = a.ver ? R[2 * N - j] : R[2 * N + j];
      }
      ME[e] = (short)v;
    }
    return;
  }
  constexpr int IT = (3 * N + 1 + NL - 1) / NL;
  int q[IT], v[IT];
  bool on[IT];
  // inv_angle <= 4096 and 0 < -k <= N where j is used: the masks change nothing and show the instruction selector a 24-bit
  // product (the table value reaches it through a register whose range it does not know: the half-rate v_mad_u64_u32 otherwise)
  int inv = a.inv_angle;
  asm("" : "+v"(inv));
  inv &= 0x1fff;
#pragma unroll
  for (int it = 0; it < IT; it++) {
    const int e = gl + it * NL, k = e - N;
    // gl < NL: the sign of k is a compile-time fact for most trips (all of them where NL divides N)
    const bool neg = (it + 1) * NL <= N ? true : it * NL >= N ? false : k < 0;
    on[it] = ((it + 1) * NL <= 3 * N + 1 || e <= 3 * N) && (neg ? k > lim : k <= last);
    const int j = (128 + mul24(-k & (2 * N - 1), inv)) >> 8;
    const int off = neg ? -j : k; // projected onto the side reference, or along the main one
    q[it] = on[it] ? (a.ver ? 2 * N + off : 2 * N - off) : 2 * N;
  }
  lds_gather<IT>(R, q, v);
#pragma unroll
  for (int it = 0; it < IT; it++)
    if (on[it]) ME[gl + it * NL] = (short)v[it];
}

// NS samples of the N x N prediction (TComPrediction.cpp:129-386, 689-730, 1010-1029):
// p[s] = pred(row(s), col(s)).  R = reference line (raw or smoothed), ME = extended main reference
// built from the same line (angular modes), dc_sum = sum of the N above and N left neighbours.
// Words of a block's extended main reference that the prediction may READ: ME[0 .. 3N + 1] (the general path reads one past the
// 3N + 1 entries build_main_ref can write, see there)
constexpr int main_ref_words(int n) { return 3 * n + 2; }
template <int N, int NS, int OPT = 0, typename RowFn, typename ColFn>
__device__ __forceinline__ void intra_pred_samples(const int *R, const int *ME, int mode, bool luma, int bit_depth, int dc_sum,
                                                   RowFn row, ColFn col, int *p) {
  constexpr int LOG2N = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : N == 32 ? 5 : 6;
  const int *top = R + 2 * N; // top[k]; left(k) = R[2N - k]
  if (mode == 0) { // planar, closed form of the accumulators
    const int tr = top[N + 1], bl = R[2 * N - (N + 1)];
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int r = row(s), c = col(s), t = top[c + 1], left = R[2 * N - (r + 1)];
      int hor = (left << LOG2N) + N + mul24(c + 1, tr - left); // samples: at most 12 bits
      int ver = (t << LOG2N) + mul24(r + 1, bl - t);
      p[s] = (short)((hor + ver) >> (LOG2N + 1));
    }
    return;
  }
  if (mode == 1) { // DC (+ edge smoothing for luma, any size)
    const int dc = (dc_sum + N) >> (LOG2N + 1);
    // (the edge smoothing stays a branch per sample, here and in the pure path below: formed for every sample from batched reads
    // and taken with a select, the two measured 0.6 % SLOWER on the mixed workload -- DESIGN.md section 5)
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int r = row(s), c = col(s);
      int v = dc;
      if (luma) {
        if (r == 0) v = c == 0 ? (top[1] + R[2 * N - 1] + 2 * dc + 2) >> 2 : (top[c + 1] + 3 * dc + 2) >> 2;
        else if (c == 0) v = (R[2 * N - (r + 1)] + 3 * dc + 2) >> 2;
      }
      p[s] = (short)v;
    }
    return;
  }
  const AngParam a = ang_param(mode);
  const int max_v = (1 << bit_depth) - 1;
  const int *M0 = ME + N; // M0[k] = refMain[k]
  if (a.angle == 0) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int r = row(s), c = col(s);
      // main-frame coordinates: k = distance from the main reference, l = position along it
      const int k = a.ver ? r : c, l = a.ver ? c : r;
      int v = M0[l + 1];
      if (luma && l == 0) { // edge filter on the first column of the main frame (:280-286)
        const int side_k1 = a.ver ? R[2 * N - (k + 1)] : top[k + 1];
        v = clip3(0, max_v, v + (((short)side_k1 - (short)top[0]) >> 1));
      }
      p[s] = v;
    }
    return;
  }
  if constexpr (!(OPT & kPredPairs)) {
#pragma unroll
    for (int s = 0; s < NS; s++) {
      const int r = row(s), c = col(s);
      const int k = a.ver ? r : c, l = a.ver ? c : r;
      const int pos = mul24(k + 1, a.angle), di = pos >> 5, df = pos & 31; // k < 32, |angle| <= 32
      const int i = l + di + 1;
      const int m0 = M0[i];
      p[s] = df ? (short)((mul24(32 - df, m0) + mul24(df, M0[i + 1]) + 16) >> 5) : m0; // samples: at most 12 bits
    }
    return;
  }
  // The general path in three phases: (a) every sample's index and weight, (b) the pairs M0[i], M0[i + 1] of all NS samples read
  // back to back with one wait behind them (lds_gather_pairs), (c) the two-tap form for every sample, with no select on df.  It is
  // exact: with df = 0 it gives (32 * m0 + 16) >> 5 = m0 for every int16 m0, whatever M0[i + 1] holds.  That read is one the
  // reference does not make; it reaches M0[2N + 1] = ME[3N + 1] (modes 2 and 34, last row: di = N), which the callers keep inside
  // the wave's scratch.  The operands are 24-bit by construction (diff17, df < 32): v_mul_i32_i24 / v_mad_i32_i24, where
  // operands without a known range took the half-rate v_mad_u64_u32.
  int idx[NS], df[NS], m0[NS], m1[NS];
#pragma unroll
  for (int s = 0; s < NS; s++) {
    const int r = row(s), c = col(s);
    const int k = a.ver ? r : c, l = a.ver ? c : r;
    const int pos = mul24(k + 1, a.angle); // k < 32, |angle| <= 32
    idx[s] = l + (pos >> 5) + 1;
    df[s] = pos & 31;
  }
  lds_gather_pairs<NS>(M0, idx, m0, m1);
#pragma unroll
  for (int s = 0; s < NS; s++) {
    // (32 - df) * m0 + df * m1 = 32 * m0 + df * (m1 - m0); the result lies between m0 and m1: no wrap to 16 bits to apply.
    // m0 and m1 are int16 (build_main_ref), their difference has 17 bits; a word m1 that is no sample meets df = 0
    p[s] = ((m0[s] << 5) + 16 + mul24(df[s], diff17(m1[s], m0[s]))) >> 5;
  }
}

} // namespace hmx
