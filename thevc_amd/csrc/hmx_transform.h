// hmx_transform.h -- the 1-D integer transforms of the reference (partialButterfly4/8/16/32 and their inverses, fastForwardDst /
// fastInverseDst, TComTrQuant.cpp:417-795) on register arrays, one pass with its rounding.  No HIP dependency: HMX_HD is
// __host__ __device__ under hipcc and nothing under g++ (as in hmx_sbh.h), so tests/native/transform_host.cpp holds every pass
// against the plain matrix product on the CPU.
//
// Arithmetic contract (bit-exact with the reference, see include/hmx.h for file:line):
//   forward pass  y[k] = wrap16((sum_n M[k][n] x[n] + rnd) >> shift)
//   inverse pass  y[n] = clip16((sum_k M[k][n] c[k] + rnd) >> shift)
// The even/odd recursion and the DST butterflies below are exact integer factorisations of those sums (no overflow:
// |sum| < 2^27), so the result equals the matrix product, and the reference's partial butterflies, bit for bit.
//
// Forms (a mask, the template argument F of the passes; kTrDefault is what every kernel uses but the packed intra kernels, whose
// 16-point forward pass keeps the loops: PackedSrc::kTrForms in hmx_chain_dev.h):
//   kTrMadChains  every odd-part sum of the DCT is ONE chain of v_mad_i32_i24, a product and an add per instruction, with the
//                 coefficient as an inline constant (-16 .. 64) or in an SGPR holding the signed value.  Written as inline asm: from
//                 `acc += mul24(k, o[n])` the compiler forms multiply, multiply, three-way add (a VOP3 instruction takes no
//                 literal: 1.5 instructions per product), and where the wrap to 16 bits bounds the demanded bits it shrinks a
//                 negative coefficient to a constant of more than 24 bits (-43 -> 0x3ffffd5), i.e. a sign extension and a
//                 quarter-rate v_mul_lo_u32.  The rounding constant seeds the chains of a forward pass and enters the even part
//                 at the bottom of the recursion, so no add stands behind a sum; the wrap and the shift are one bit-field extract.
//   kTrFastDst    the 4-point DST as the reference's own butterflies: 9 products per vector where the matrix form has 16 (the
//                 reference's 8, and 74 x2 once more with the other sign: both signs of it come with the seed in them).
// Without a bit the pass keeps the form it had before (the loops over the matrix): for a kernel that would spill with the new one.
#pragma once

#include "hmx_sbh.h" // HMX_HD

namespace hmx {

// The chains are chosen per direction and size: tr_fwd_bit(N) / tr_inv_bit(N), N = 4, 8, 16, 32; kTrMadFwd / kTrMadInv are all sizes of
// a direction.  (The DST follows the 4-point bits: its products are multiply-adds where the 4-point DCT's are.)
HMX_HD constexpr int tr_fwd_bit(int N) { return N; }
HMX_HD constexpr int tr_inv_bit(int N) { return N << 4; }
constexpr int kTrFastDst = 2;
constexpr int kTrMadFwd16 = tr_fwd_bit(16);
constexpr int kTrMadFwd = tr_fwd_bit(4) | tr_fwd_bit(8) | tr_fwd_bit(16) | tr_fwd_bit(32);
constexpr int kTrMadInv = tr_inv_bit(4) | tr_inv_bit(8) | tr_inv_bit(16) | tr_inv_bit(32);
constexpr int kTrMadChains = kTrMadFwd | kTrMadInv;
static_assert(!(kTrFastDst & kTrMadChains) && !(kTrMadFwd & kTrMadInv), "one bit per form");
#ifndef HMX_X_TRANSFORM_FORMS /* A/B builds of the forms (profiles/mad_chains_bench_ab.txt): -DHMX_X_TRANSFORM_FORMS=0 the matrix loops, =kTrFastDst the DST butterflies alone, =kTrMadChains the chains alone */
#define HMX_X_TRANSFORM_FORMS (kTrMadChains | kTrFastDst)
#endif
constexpr int kTrDefault = HMX_X_TRANSFORM_FORMS;

// ---------------------------------------------------------------------------------------------
// Tables
// ---------------------------------------------------------------------------------------------
// integer chosen by HEVC for cos(p*pi/64), p = 0..32 (first column of the 32-point matrix)
HMX_HD constexpr int cos64(int p) {
  constexpr int t[33] = {64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64,
                         61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9,  4,  0};
  return t[p];
}
// M_N[k][n]: fold the angle (2n+1)k*(32/N)*pi/64 into the first quadrant
HMX_HD constexpr int dct_coef(int N, int k, int n) {
  int p = ((2 * n + 1) * k * (32 / N)) & 127;
  int s = 1;
  if (p > 64) p = 128 - p;
  if (p > 32) {
    p = 64 - p;
    s = -1;
  }
  return s * cos64(p);
}
HMX_HD constexpr int dst_coef(int k, int n) {
  constexpr int t[4][4] = {{29, 55, 74, 84}, {74, 74, 0, -74}, {84, -29, -74, 55}, {55, -84, 74, -29}};
  return t[k][n];
}

// ---------------------------------------------------------------------------------------------
// Arithmetic helpers: one instruction each on the device, plain C++ on the host
// ---------------------------------------------------------------------------------------------
// a * b for operands that fit 24 bits (v_mul_i32_i24)
HMX_HD int tr_mul24(int a, int b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __mul24(a, b);
#else
  return a * b;
#endif
}
// acc + K * x for x that fits 24 bits.  MAD: v_mad_i32_i24 by hand, K an inline constant where the instruction takes it and an
// SGPR with the signed value otherwise (the instruction reads its low 24 bits as a signed number: no constant is widened).
template <int K, bool MAD>
HMX_HD int tr_mad(int x, int acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (MAD) {
    int r;
    if constexpr (K >= -16 && K <= 64) asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "n"(K), "v"(x), "v"(acc));
    else asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "s"(K), "v"(x), "v"(acc));
    return r;
  } else {
    return acc + __mul24(K, x);
  }
#else
  return acc + K * x;
#endif
}
HMX_HD int tr_clip16(int v) { // Clip3(-32768, 32767, v): v_med3_i32
#if defined(__HIP_DEVICE_COMPILE__)
  return min(max(v, -32768), 32767);
#else
  return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
#endif
}
// The rounding constant of a pass as the addend of its chains, made where the pass stands.  It is the same in every trip of a
// persistent kernel's loop: left as a plain value, its copy in a vector register is hoisted out of that loop and lives through the
// whole kernel, one register per pass and size (the packed encoder kernels spilled two to four registers for it).
HMX_HD int tr_seed(int rnd) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(rnd));
#endif
  return rnd;
}
// wrap16(v >> shift): bits shift .. shift + 15 of v, sign-extended (one v_bfe_i32); shift <= 16
HMX_HD int tr_shift_wrap16(int v, int shift) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sbfe(v, (unsigned)shift, 16u);
#else
  return (int)(short)(v >> shift);
#endif
}

// ---------------------------------------------------------------------------------------------
// 1-D DCT on register arrays, the loops over the matrix (raw sums, no rounding)
// ---------------------------------------------------------------------------------------------
template <int N>
HMX_HD void dct_fwd_raw(const int *x, int *y) {
  if constexpr (N == 2) {
    y[0] = 64 * (x[0] + x[1]);
    y[1] = 64 * (x[0] - x[1]);
  } else {
    int e[N / 2], o[N / 2], ye[N / 2];
#pragma unroll
    for (int n = 0; n < N / 2; n++) {
      e[n] = x[n] + x[N - 1 - n];
      o[n] = x[n] - x[N - 1 - n];
    }
    dct_fwd_raw<N / 2>(e, ye);
#pragma unroll
    for (int m = 0; m < N / 2; m++) {
      y[2 * m] = ye[m];
      int acc = 0;
#pragma unroll
      for (int n = 0; n < N / 2; n++) acc += tr_mul24(dct_coef(N, 2 * m + 1, n), o[n]); // |o| < 2^21: sums of int16 inputs
      y[2 * m + 1] = acc;
    }
  }
}

template <int N>
HMX_HD void dct_inv_raw(const int *c, int *out) {
  if constexpr (N == 2) {
    out[0] = 64 * (c[0] + c[1]);
    out[1] = 64 * (c[0] - c[1]);
  } else {
    int ce[N / 2], ee[N / 2];
#pragma unroll
    for (int m = 0; m < N / 2; m++) ce[m] = c[2 * m];
    dct_inv_raw<N / 2>(ce, ee);
#pragma unroll
    for (int n = 0; n < N / 2; n++) {
      int acc = 0;
#pragma unroll
      for (int m = 0; m < N / 2; m++) acc += tr_mul24(dct_coef(N, 2 * m + 1, n), c[2 * m + 1]); // c: int16 inputs
      out[n] = ee[n] + acc;
      out[N - 1 - n] = ee[n] - acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The same sums as multiply-add chains.  `seed` (the rounding constant of the pass) is part of every output.
// ---------------------------------------------------------------------------------------------
// seed + sum_{n >= I} M_N[ROW][n] o[n]: the coefficients are template arguments, so each is a constant of its instruction
template <int N, int ROW, int I = 0>
HMX_HD int dct_fwd_chain(const int *o, int acc) {
  if constexpr (I == N / 2) return acc;
  else return dct_fwd_chain<N, ROW, I + 1>(o, tr_mad<dct_coef(N, ROW, I), true>(o[I], acc)); // |o| < 2^21: sums of int16 inputs
}
template <int N, int M = 0>
HMX_HD void dct_fwd_odd(const int *o, int *y, int seed) {
  if constexpr (M < N / 2) {
    y[2 * M + 1] = dct_fwd_chain<N, 2 * M + 1>(o, seed);
    dct_fwd_odd<N, M + 1>(o, y, seed);
  }
}
template <int N>
HMX_HD void dct_fwd_mad(const int *x, int *y, int seed) {
  if constexpr (N == 2) {
    y[0] = 64 * (x[0] + x[1]) + seed;
    y[1] = 64 * (x[0] - x[1]) + seed;
  } else {
    int e[N / 2], o[N / 2], ye[N / 2];
#pragma unroll
    for (int n = 0; n < N / 2; n++) {
      e[n] = x[n] + x[N - 1 - n];
      o[n] = x[n] - x[N - 1 - n];
    }
    dct_fwd_mad<N / 2>(e, ye, seed);
#pragma unroll
    for (int m = 0; m < N / 2; m++) y[2 * m] = ye[m];
    dct_fwd_odd<N>(o, y, seed);
  }
}

// sum_m M_N[2m + 1][COL] c[2m + 1]: the first product a plain multiply (it takes a literal), the rest of the chain behind it
template <int N, int COL, int I = 1>
HMX_HD int dct_inv_chain(const int *c, int acc) {
  if constexpr (I == N / 2) return acc;
  else return dct_inv_chain<N, COL, I + 1>(c, tr_mad<dct_coef(N, 2 * I + 1, COL), true>(c[2 * I + 1], acc)); // c: int16 inputs
}
template <int N, int COL = 0>
HMX_HD void dct_inv_odd(const int *c, const int *ee, int *out) {
  if constexpr (COL < N / 2) {
    const int acc = dct_inv_chain<N, COL>(c, tr_mul24(dct_coef(N, 1, COL), c[1]));
    out[COL] = ee[COL] + acc;
    out[N - 1 - COL] = ee[COL] - acc;
    dct_inv_odd<N, COL + 1>(c, ee, out);
  }
}
template <int N>
HMX_HD void dct_inv_mad(const int *c, int *out, int seed) {
  if constexpr (N == 2) {
    out[0] = 64 * (c[0] + c[1]) + seed;
    out[1] = 64 * (c[0] - c[1]) + seed;
  } else {
    int ce[N / 2], ee[N / 2];
#pragma unroll
    for (int m = 0; m < N / 2; m++) ce[m] = c[2 * m];
    dct_inv_mad<N / 2>(ce, ee, seed);
    dct_inv_odd<N>(c, ee, out);
  }
}

// ---------------------------------------------------------------------------------------------
// 4-point DST (4x4 luma intra), the reference's butterflies: raw sums with the seed in them.  Inputs of the int16 range: the
// sums of two and three of them fit 24 bits.
// ---------------------------------------------------------------------------------------------
template <bool MAD>
HMX_HD void dst_fwd_fast(const int *x, int *y, int seed) {
  const int c0 = x[0] + x[3], c1 = x[1] + x[3], c2 = x[0] - x[1];
  const int p = tr_mad<74, MAD>(x[2], seed), m = tr_mad<-74, MAD>(x[2], seed); // seed + 74 x2, seed - 74 x2
  y[0] = tr_mad<55, MAD>(c1, tr_mad<29, MAD>(c0, p));
  y[1] = tr_mad<74, MAD>(x[0] + x[1] - x[3], seed);
  y[2] = tr_mad<55, MAD>(c0, tr_mad<29, MAD>(c2, m));
  y[3] = tr_mad<-29, MAD>(c1, tr_mad<55, MAD>(c2, p));
}
template <bool MAD>
HMX_HD void dst_inv_fast(const int *t, int *y, int seed) {
  const int c0 = t[0] + t[2], c1 = t[2] + t[3], c2 = t[0] - t[3];
  const int p = tr_mad<74, MAD>(t[1], seed), m = tr_mad<-74, MAD>(t[1], seed);
  y[0] = tr_mad<55, MAD>(c1, tr_mad<29, MAD>(c0, p));
  y[1] = tr_mad<-29, MAD>(c1, tr_mad<55, MAD>(c2, p));
  y[2] = tr_mad<74, MAD>(t[0] - t[2] + t[3], seed);
  y[3] = tr_mad<29, MAD>(c2, tr_mad<55, MAD>(c0, m));
}

// ---------------------------------------------------------------------------------------------
// One pass with its rounding
// ---------------------------------------------------------------------------------------------
// forward pass with the reference's rounding and implicit store-to-short wrap
template <int N, int F = kTrDefault>
HMX_HD void fwd_pass(const int *x, int *y, int shift, bool use_dst) {
  const int rnd = 1 << (shift - 1);
  if (N == 4 && use_dst) {
    if constexpr (F & kTrFastDst) {
      int raw[4];
      dst_fwd_fast<(F & tr_fwd_bit(N)) != 0>(x, raw, (F & tr_fwd_bit(N)) ? tr_seed(rnd) : rnd);
#pragma unroll
      for (int k = 0; k < 4; k++) y[k] = tr_shift_wrap16(raw[k], shift);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        int acc = 0;
#pragma unroll
        for (int n = 0; n < 4; n++) acc += tr_mul24(dst_coef(k, n), x[n]); // x: int16-range residuals
        y[k] = (int)(short)((acc + rnd) >> shift);
      }
    }
  } else {
    int raw[N];
    if constexpr (F & tr_fwd_bit(N)) {
      dct_fwd_mad<N>(x, raw, tr_seed(rnd));
#pragma unroll
      for (int k = 0; k < N; k++) y[k] = tr_shift_wrap16(raw[k], shift);
    } else {
      dct_fwd_raw<N>(x, raw);
#pragma unroll
      for (int k = 0; k < N; k++) y[k] = (int)(short)((raw[k] + rnd) >> shift);
    }
  }
}

// inverse pass with Clip3(-32768, 32767)
template <int N, int F = kTrDefault>
HMX_HD void inv_pass(const int *c, int *y, int shift, bool use_dst) {
  const int rnd = 1 << (shift - 1);
  if (N == 4 && use_dst) {
    if constexpr (F & kTrFastDst) {
      int raw[4];
      dst_inv_fast<(F & tr_inv_bit(N)) != 0>(c, raw, (F & tr_inv_bit(N)) ? tr_seed(rnd) : rnd);
#pragma unroll
      for (int n = 0; n < 4; n++) y[n] = tr_clip16(raw[n] >> shift);
    } else {
#pragma unroll
      for (int n = 0; n < 4; n++) {
        int acc = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) acc += tr_mul24(dst_coef(k, n), c[k]); // c: int16 coefficients
        y[n] = tr_clip16((acc + rnd) >> shift);
      }
    }
  } else {
    int raw[N];
    if constexpr (F & tr_inv_bit(N)) {
      dct_inv_mad<N>(c, raw, tr_seed(rnd));
#pragma unroll
      for (int n = 0; n < N; n++) y[n] = tr_clip16(raw[n] >> shift);
    } else {
      dct_inv_raw<N>(c, raw);
#pragma unroll
      for (int n = 0; n < N; n++) y[n] = tr_clip16((raw[n] + rnd) >> shift);
    }
  }
}

} // namespace hmx
