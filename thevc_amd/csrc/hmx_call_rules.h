// hmx_call_rules.h -- what a whole-picture call DECIDES on the host before it touches the device: packing group, shape and limits
// of the packed tables, persistent waves, the schedule, RDOQ's per-call constants.  Pure host arithmetic, no HIP, every tuning rule
// beside the measurement that set it: hmx_chain.hip, hmx_plan.hip and hmx_scalar.hip call it around their device work,
// tests/native/call_rules_host.cpp runs it on the CPU.  HMX_HD (as in hmx_sbh.h): a function the kernels need too (pack_slots).
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>

#ifndef HMX_HD
#if defined(__HIPCC__)
#define HMX_HD __host__ __device__ __forceinline__
#else
#define HMX_HD inline
#endif
#endif

namespace hmx {
constexpr int kRdoqMaxGroup = 2; // pictures per packing group with RDOQ: 2 x 2 tables of 1016 bytes in LDS
}
constexpr int kMaxSideStreams = 8; // side streams of a context: the picture groups of the level schedule (hmx_ctx::kMaxSide)

struct PackGeom {
  int n_pics, I, n_groups, n_shards, max_levels, slots4, slots8;
};
HMX_HD uint32_t pack_slots(int s, int slots4, int slots8) { return s == 0 ? (uint32_t)slots4 : s == 1 ? (uint32_t)slots8 : s == 2 ? 4u : 1u; }

// Pictures per group of the packed schedule.  A group is an interleave domain of the pool and the unit that advances level
// by level: its pictures move in lockstep, and a row is complete only when its slowest wave-item is.  Small groups keep
// that coupling small (measured at 2048 pictures of 2160p, 64 distinct plans: 70 / 79 / 86 / 93 / 94 / 93 Gpx/s with groups
// of 64 / 32 / 16 / 8 / 4 / 2); what is left of "packing across pictures" at 4 is enough to fill the waves of the large
// batches, and small batches are latency-bound whatever the packing (256 pictures: 29 / 32 Gpx/s with 4 / 2; 64
// pictures: 9.5 / 9.9 with 2 / 1).  Groups are dealt to the 8 XCDs round-robin.
// knob_group: HMX_PACK_GROUP (0: by batch size)
inline int pack_group_rule(int knob_group, bool rdoq, int n_pics) {
  if (knob_group > 0) return std::min(knob_group, n_pics);
  if (rdoq) return n_pics >= 512 ? hmx::kRdoqMaxGroup : 1; // RDOQ on (hmx_set_rdoq): the tables of a group wait in LDS
  return n_pics >= 1536 ? 4 : n_pics >= 512 ? 2 : 1;
}

struct PackShape {
  PackGeom G;
  uint64_t items, n_rows, waves_bound; // blocks and rows of the call; an upper bound on its wave-items (sizes the descriptor table)
  bool too_large;                      // the tables of one call index with 32 bits: the batch has to be split
};
// knob4 / knob8: HMX_PACK_SLOTS4 / 8 (0: by batch size); rdoq / qmap: the call quantises with RDOQ / with a QP per block; max_levels,
// sz[], items: the most dependency levels of any plan of the call, its blocks per size class and in all
inline PackShape pack_shape(int n_pics, int I, int knob4, int knob8, bool rdoq, bool qmap, int max_levels, const uint64_t sz[4], uint64_t items) {
  PackShape S{};
  PackGeom &G = S.G;
  G.n_pics = n_pics, G.I = I, G.max_levels = max_levels;
  G.n_groups = (n_pics + I - 1) / I;
  G.n_shards = std::min(8, G.n_groups);
  // one lane per 4x4 block is the throughput shape, four lanes per block make more, shorter waves (small batches)
  // (measured with the mode-aware dependency order, 2160p mix: 64 lanes/wave-item ahead at 8..128 and from 384 pictures,
  // 16 ahead at 192 and 256)
  G.slots4 = knob4 ? knob4 : ((n_pics >= 160 && n_pics < 320) ? 16 : 64);
  if (qmap) G.slots4 = 64; // the kernel with a QP per block has one wave-item shape per size class (HMX_PACK_SLOTS4 / 8 do not apply)
  if (rdoq) G.slots4 = 64; // a 4x4 block's RDOQ runs inside one lane
  // 8x8 blocks: sixteen per wave-item on four lanes each (wave_chain_8x2) where throughput counts, eight on eight lanes where a
  // wave-item's latency does (and under RDOQ, whose rounds are laid out for eight)
  G.slots8 = rdoq || qmap || G.slots4 != 64 ? 8 : knob8 ? knob8 : (n_pics >= 640 ? 16 : 8); // measured, 2160p mix: 512 pictures -3 %, 768 +4 %, 1024 +8 %, 2048 +11 %
  S.items = items;
  S.n_rows = (uint64_t)G.max_levels * G.n_groups;
  S.waves_bound = 4 * S.n_rows + 4;
  for (int s = 0; s < 4; s++) S.waves_bound += sz[s] / pack_slots(s, G.slots4, G.slots8);
  S.too_large = items >= 0xffffffffull || S.waves_bound >= 0x0fffffffull || S.n_rows >= 0x7fffffffull / 4;
  return S;
}

// Persistent waves of the packed launch: enough to hold about two levels' worth of wave-items (the waves of the next row load
// their descriptors and originals while the current row finishes), never more than the device keeps resident.
// knob_waves: HMX_PACK_WAVES (0: by batch size); resident: resident waves of the kernel variant the call launches
inline int pack_wave_count(int knob_waves, int resident, uint64_t waves_bound, int max_levels) {
  const uint64_t wpl = waves_bound / (uint64_t)std::max(1, max_levels); // wave-items per dependency level, all groups
  const uint64_t want = std::max<uint64_t>(256, 2 * wpl);
  return knob_waves ? std::min(knob_waves, resident) : (int)std::min<uint64_t>((uint64_t)resident, want);
}

struct CallSchedule {
  int schedule;       // 3 packed, 2 level across pictures, 1 level per picture, 0 wave (hmx_last_call_shape)
  bool across;        // level schedule: SIMD across pictures
  int groups;         // stream groups of the level schedule
  bool pipeline_conv; // its conversions pipelined by CTU row
};
// Schedules.  "packed" (default): ONE persistent launch, blocks of equal size and dependency level
// packed into waves across pictures, each picture following its own plan, the dependency order kept by counters in
// memory.  The level-synchronous schedules stay as cross-checks and for A/B runs (HMX_INTRA_SCHEDULE=level|wave):
// "level" = one launch per picture-wide dependency level (pictures that share ONE plan run it across pictures on a
// pool interleaved per stream group), "wave" = one launch per CTU diagonal with autonomous waves.
// resident: the pictures stay in the caller's pools (packed only); plan_stride 0: one plan for all pictures; onto: the call
// reconstructs onto what the reconstruction planes already hold; kn: hmx_ctx::Knobs (schedule, across, streams, pipeline_conv, graph)
template <class Knobs>
inline CallSchedule resolve_schedule(bool resident, int plan_stride, int n_pics, bool onto, const Knobs &kn) {
  CallSchedule s{};
  const int base = resident ? 3 : kn.schedule >= 0 ? kn.schedule : 3;
  const bool packed = base == 3, use_level = base == 1;
  s.across = use_level && plan_stride == 0 && kn.across != 0;
  s.schedule = packed ? 3 : !use_level ? 0 : (s.across ? 2 : 1);
  // Picture groups of the across schedule on separate streams: measured at 1024 pictures 64.8 / 73.6 / 76.1 / 51.8 Gpx/s
  // with 1 / 2 / 3 / 4 groups.
  s.groups = !s.across ? 1 : n_pics >= 640 ? 3 : n_pics >= 384 ? 2 : 1;
  if (use_level && kn.streams > 0) s.groups = std::min(std::max(kn.streams, 1), std::min(n_pics, kMaxSideStreams));
  // Conversions pipelined with the chain, CTU row by CTU row (issue_across_pipelined): opt-in, across schedule only.
  s.pipeline_conv = kn.pipeline_conv && s.across && !kn.graph && !onto;
  return s;
}

// RDOQ's two quotients that the host forms, each in the reference's operation order (one reordered division changes levels) and
// without fused multiply-add.  The error scale of a 2^log2n block at bit depth B with quantiser scale q (setErrScaleCoeff,
// TComTrQuant.cpp:2794-2818, flat quantiser coefficients)
inline double rdoq_err_scale(int B, int q, int log2n) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const int tshift = 15 - B - log2n;
  double e = (double)(1 << 15);
  e = e * ldexp(1.0, -2 * tshift);
  e = e / (double)q / (double)q / (double)(1 << (2 * (B - 8)));
  return e;
}
// The Int64 factor of sign hiding's rate-distortion cost (TComTrQuant.cpp:2205): inv_scale = g_invQuantScales[rem], lambda > 0
inline long long rdoq_rd_factor(int inv_scale, int per, double lambda, int B) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return (long long)((double)inv_scale * (double)inv_scale * (double)(1 << (2 * per)) / lambda / 16 / (double)(1 << (2 * (B - 8))) + 0.5);
}
// The wave-cooperative RDOQ keeps levels as 16-bit words; the reference keeps TCoeff = Int.  A level can reach (32768 * q) >> qbits:
// at the lowest QPs of deep bit depths that exceeds 32767 for the large transforms (10 bit, per = 0, 32x32: ~52000) and would wrap
// silently.  false: a 2^log2n block at (q, per, B) can exceed 16 bits -- the whole-picture chain refuses such a call, the block
// list sends it through the one-lane-per-block kernel, whose levels are 32-bit.  A negative shift does not fit.
inline bool rdoq_levels_fit16(int q, int per, int B, int log2n) {
  const int qbits = 14 + per + (15 - B - log2n);
  return qbits >= 0 && ((32768ll * q) >> qbits) <= 32767;
}
