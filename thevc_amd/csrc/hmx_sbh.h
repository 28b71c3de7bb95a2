// hmx_sbh.h -- signBitHidingHDQ (TComTrQuant.cpp:977-1100) for ONE 16-coefficient group, the decision every flat quantiser of the
// device shares (quant_sbh_block, quant_sbh_diag, the 8x8 in-register path of wave_chain_8x2, lane4_forward).  No HIP dependency:
// HMX_HD is __host__ __device__ under hipcc and nothing under g++, so tests/test_sbh_core.py holds it against the oracle's xQuant
// on the CPU.
//
// A group arrives as 16 packed words (bits 0..15 level, bit 16 coefficient < 0, bits 17..31 deltaU, as quant_one leaves them) in
// any order: word k sits at position sc.pos(k) of the group's scan, and sc.word(s) is the word at scan position s.  The callers
// hold the words in scan order and pass ScanOrder (both compile-time identities).  (A raster-order group with the scan as a
// per-lane nibble table of positions was tried for the 4x4 and 8x8 shapes: the run-time shifts cost more than the two selects per
// word of the reorder.)
//
// Branch-free where lanes differ:
//  * one pass gathers the parity and two 16-bit masks in scan order (non-zero, negative) -> first / last / the hidden sign;
//  * the reference scans n = 15..0 keeping the strictly smaller cost, i.e. the lowest cost and, among equal costs, the highest n.
//    The cost of every candidate is -|deltaU|: a non-zero level costs -deltaU or deltaU by the sign of deltaU (:1031-1047), a
//    zero level -deltaU (:1050-1069), and a zero level's deltaU is never negative.  So the choice is the maximum of one key
//    valid << 16 | |deltaU| << 8 | n << 4 | k  (|deltaU| <= 255, see below), with "valid" the reference's candidate rules:
//      not a zero level below the first non-zero whose sign differs from the hidden sign   (:1055-1060)
//      not the first non-zero itself when |level| = 1 and deltaU <= 0                      (:1040-1043)
//      not above the last non-zero in the last group                                        (:1017, lastCG)
//    The last non-zero is always valid (it is not the first: last - first >= 4), so the maximum is a valid key.
// deltaU = (|c| q - |l| << qbits) >> (qbits - 8) lies in [-rnd/2, (512 - rnd)/2) for the rounding offset rnd << (qbits - 9)
// (rnd = 171 intra, 85 inter): |deltaU| <= 255 at any bit depth and QP.
#pragma once

#ifndef HMX_HD
#if defined(__HIPCC__)
#define HMX_HD __host__ __device__ __forceinline__
#else
#define HMX_HD inline
#endif
#endif

namespace hmx {

// w[idx] for a run-time idx: a four-level tree of 15 bit-field inserts (v_bfi_b32 with an all-ones / all-zeros mask per index
// bit).  Written with masks on purpose: a tree of ?: selects is turned into an indexed private array by the compiler, i.e.
// scratch memory.
HMX_HD int sbh_blend(int m, int t, int f) { return (t & m) | (f & ~m); }
HMX_HD int select16(const int *w, int idx) {
  int a[8], b[4], c[2];
  const int m0 = -(idx & 1), m1 = -((idx >> 1) & 1), m2 = -((idx >> 2) & 1), m3 = -((idx >> 3) & 1);
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = sbh_blend(m0, w[2 * k + 1], w[2 * k]);
#pragma unroll
  for (int k = 0; k < 4; k++) b[k] = sbh_blend(m1, a[2 * k + 1], a[2 * k]);
#pragma unroll
  for (int k = 0; k < 2; k++) c[k] = sbh_blend(m2, b[2 * k + 1], b[2 * k]);
  return sbh_blend(m3, c[1], c[0]);
}

struct ScanOrder { // the words are in scan order
  HMX_HD int pos(int k) const { return k; }
  HMX_HD int word(int s) const { return s; }
};

// The level change at the chosen word (:1086-1096): +1 in magnitude unless a non-zero level has deltaU <= 0 or sits at the clip.
HMX_HD int sbh_apply(int wsel) {
  const int q = (int)(short)wsel, neg = (wsel >> 16) & 1;
  int chg = (q != 0 && (wsel >> 17) <= 0) ? -1 : 1;
  if (q == 32767 || q == -32768) chg = -1;
  const int nq = neg ? q - chg : q + chg;
  return (int)(((unsigned)wsel & 0xffff0000u) | ((unsigned)nq & 0xffffu));
}

// The word index k whose level changes, or -1.  last_group: no later group of the block holds a non-zero level (the reference's
// lastCG).  fetch(k) returns word k for a run-time k (select16 on registers, or a load where the words lie in memory).
template <typename SC, typename FETCH>
HMX_HD int sbh_pick(const int *w, const SC &sc, bool last_group, FETCH fetch) {
  unsigned nzm = 0, ngm = 0, par = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int s = sc.pos(k);
    par ^= (unsigned)w[k];
    nzm |= ((unsigned)w[k] << 16 != 0 ? 1u : 0u) << s;
    ngm |= (((unsigned)w[k] >> 16) & 1u) << s;
  }
  if (nzm == 0) return -1;
  const int first = __builtin_ctz(nzm), last = 31 - __builtin_clz(nzm);
  const unsigned signbit = (ngm >> first) & 1u;
  if (last - first < 4 || signbit == (par & 1u)) return -1;
  const int wf = fetch(sc.word(first));
  const int qf = (int)(short)wf;
  const bool first_unit_down = (qf == 1 || qf == -1) && (wf >> 17) <= 0;
  unsigned valid = last_group ? (2u << last) - 1u : 0xffffu;
  valid &= ~(((1u << first) - 1u) & (ngm ^ (0u - signbit))); // below the first non-zero every level is zero
  valid &= ~((first_unit_down ? 1u : 0u) << first);
  const unsigned v16 = valid << 16;
  unsigned best = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int s = sc.pos(k), du = w[k] >> 17, adu = du < 0 ? -du : du;
    const unsigned key = ((v16 >> s) & 0x10000u) | ((unsigned)adu << 8) | ((unsigned)s << 4) | (unsigned)k;
    best = best > key ? best : key;
  }
  return (int)(best & 15u);
}

template <typename SC>
HMX_HD int sbh_pick(const int *w, const SC &sc, bool last_group) {
  return sbh_pick(w, sc, last_group, [&](int k) { return select16(w, k); });
}

} // namespace hmx
