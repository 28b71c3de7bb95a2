// hmx_inter.hip: interpolation filters, motion compensation, sub-pel cost fan-out, border extension -- part of libhmx (include/hmx.h), gfx950.  See hmx_host.h for how the library is cut into translation units.
#include "hmx_host.h"

// =============================================================================================
// Interpolation (TComInterpolationFilter.cpp), addAvg, motion compensation, border extension
// =============================================================================================
// filterCopy (:91-145) of one sample, the reference's three cases as it writes them
__device__ __forceinline__ int interp_copy(int v, bool first, bool last, int B) {
  const int head = 14 - B;
  if (first == last) return v;
  if (first) return wrap16(wrap16(v << head) - 8192);
  int off = wrap16(8192 + (head ? (1 << (head - 1)) : 0));
  return clip3(0, (1 << B) - 1, wrap16((v + off) >> head));
}
// One output sample of filterHor*/filterVer* incl. the frac == 0 filterCopy cases (:91-244): the drop-in for the reference's
// function, first == last included.  src points at the sample co-located with the output; step = 1 (horizontal) or the stride.
template <int NTAP>
__device__ __forceinline__ int interp_sample(const short *src, int step, int frac, bool first, bool last, int B) {
  if (frac == 0) return interp_copy(src[0], first, last, B);
  const InterpStage st = interp_stage(first, last, B);
  int acc = st.offset;
#pragma unroll
  for (int t = 0; t < NTAP; t++) acc += src[(t - (NTAP / 2 - 1)) * step] * (NTAP == 8 ? luma_tap(frac, t) : chroma_tap(frac, t));
  return interp_end(st, acc);
}

__global__ void k_filter(const short *src, int ss, short *dst, int ds, int w, int h, int frac, int chroma, int vertical,
                         int first, int last, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  int r = i / w, col = i % w;
  const short *p = src + (size_t)r * ss + col;
  int step = vertical ? ss : 1;
  dst[(size_t)r * ds + col] =
      (short)(chroma ? interp_sample<4>(p, step, frac, first, last, B) : interp_sample<8>(p, step, frac, first, last, B));
}

static int filter_scalar(hmx_ctx *c, const hmx_pel *src, int ss, int16_t *dst, int ds, int w, int h, int frac, int chroma,
                         int vertical, int first, int last) {
  if (!c || !src || !dst || w <= 0 || h <= 0 || w > 128 || h > 128 || frac < 0 || frac >= (chroma ? 8 : 4))
    return fail(c, HMX_ERR_ARG, "filter: bad argument");
  const int before = frac ? (chroma ? 1 : 3) : 0, after = frac ? (chroma ? 2 : 4) : 0;
  const int ww = w + (vertical ? 0 : before + after), wh = h + (vertical ? before + after : 0);
  Scratch s{c};
  short *d_in = s.up(src - (vertical ? (ptrdiff_t)before * ss : before), ww, wh, ss), *d_out = s.take<short>((size_t)w * h);
  if (s.r) return s.r;
  const short *d_org = d_in + (vertical ? before * ww : before);
  hipLaunchKernelGGL(k_filter, dim3((w * h + 255) / 256), dim3(256), 0, c->stream, d_org, ww, d_out, w, w, h, frac, chroma,
                     vertical, first, last, c->cfg.bit_depth);
  HIPCHK(c, hipGetLastError());
  return down2d(c, dst, ds, d_out, 2, w, h);
}
extern "C" int hmx_filterHorLuma(hmx_ctx *c, const hmx_pel *src, int ss, int16_t *dst, int ds, int w, int h, int frac,
                                 int is_last) {
  return filter_scalar(c, src, ss, dst, ds, w, h, frac, 0, 0, 1, is_last);
}
extern "C" int hmx_filterVerLuma(hmx_ctx *c, const hmx_pel *src, int ss, int16_t *dst, int ds, int w, int h, int frac,
                                 int is_first, int is_last) {
  return filter_scalar(c, src, ss, dst, ds, w, h, frac, 0, 1, is_first, is_last);
}
extern "C" int hmx_filterHorChroma(hmx_ctx *c, const hmx_pel *src, int ss, int16_t *dst, int ds, int w, int h, int frac,
                                   int is_last) {
  return filter_scalar(c, src, ss, dst, ds, w, h, frac, 1, 0, 1, is_last);
}
extern "C" int hmx_filterVerChroma(hmx_ctx *c, const hmx_pel *src, int ss, int16_t *dst, int ds, int w, int h, int frac,
                                   int is_first, int is_last) {
  return filter_scalar(c, src, ss, dst, ds, w, h, frac, 1, 1, is_first, is_last);
}

// ---- scalar drop-ins of the inter prediction of ONE block (host pointers) ----
// xPredInterLumaBlk / xPredInterChromaBlk (TComPrediction.cpp:554-642): the window the filters reach goes up once, the
// one or two filter stages run on the device (the reference's three cases: horizontal only, vertical only, horizontal
// into the 14-bit intermediate then vertical), the block comes back.  w, h: the block IN ITS PLANE.
// s: the caller's scratch, whose front this block re-uses; d_keep: the block stays on the device, there (a tail buffer of s)
static int pred_inter_blk(hmx_ctx *c, Scratch &s, const hmx_pel *ref, int ref_stride, int mvx, int mvy, int w, int h, hmx_pel *dst, int dst_stride,
                          int bi, int chroma, short *d_keep = nullptr) {
  if (!c || !ref || (!dst && !d_keep) || w <= 0 || h <= 0 || w > 64 || h > 64) return fail(c, HMX_ERR_ARG, "xPredInterBlk: bad argument");
  const int fb = chroma ? 3 : 2, fm = (1 << fb) - 1, xf = mvx & fm, yf = mvy & fm;
  const int before = chroma ? 1 : 3, after = chroma ? 2 : 4, ww = w + before + after, wh = h + before + after;
  s.rewind();
  short *d_in = s.up(ref + (ptrdiff_t)((mvy >> fb) - before) * ref_stride + ((mvx >> fb) - before), ww, wh, ref_stride);
  short *d_tmp = s.take<short>((size_t)w * wh), *d_out = d_keep ? d_keep : s.take<short>((size_t)w * h);
  if (s.r) return s.r;
  const short *d_blk = d_in + before * ww + before; // the block's first sample inside the window
  const int B = c->cfg.bit_depth, last = !bi;
  const dim3 g1((w * h + 255) / 256), g2((w * wh + 255) / 256), blk(256);
  if (yf == 0) {
    hipLaunchKernelGGL(k_filter, g1, blk, 0, c->stream, d_blk, ww, d_out, w, w, h, xf, chroma, 0, 1, last, B);
  } else if (xf == 0) {
    hipLaunchKernelGGL(k_filter, g1, blk, 0, c->stream, d_blk, ww, d_out, w, w, h, yf, chroma, 1, 1, last, B);
  } else { // rows -before .. h+after-1 through the horizontal stage (isLast = false), then the vertical one (isFirst = false)
    hipLaunchKernelGGL(k_filter, g2, blk, 0, c->stream, d_in + before, ww, d_tmp, w, w, wh, xf, chroma, 0, 1, 0, B);
    hipLaunchKernelGGL(k_filter, g1, blk, 0, c->stream, d_tmp + before * w, w, d_out, w, w, h, yf, chroma, 1, 0, last, B);
  }
  HIPCHK(c, hipGetLastError());
  return d_keep ? HMX_OK : down2d(c, dst, dst_stride, d_out, 2, w, h);
}
extern "C" int hmx_xPredInterLumaBlk(hmx_ctx *c, const hmx_pel *ref, int ref_stride, int mv_hor, int mv_ver, int w, int h, hmx_pel *dst,
                                     int dst_stride, int bi) {
  Scratch s{c};
  return pred_inter_blk(c, s, ref, ref_stride, mv_hor, mv_ver, w, h, dst, dst_stride, bi, 0);
}
extern "C" int hmx_xPredInterChromaBlk(hmx_ctx *c, const hmx_pel *ref, int ref_stride, int mv_hor, int mv_ver, int w, int h, hmx_pel *dst,
                                       int dst_stride, int bi) {
  if ((w & 1) || (h & 1)) return fail(c, HMX_ERR_ARG, "hmx_xPredInterChromaBlk: odd luma size");
  Scratch s{c};
  return pred_inter_blk(c, s, ref, ref_stride, mv_hor, mv_ver, w >> 1, h >> 1, dst, dst_stride, bi, 1);
}
// TComYuv::addAvg and TComWeightPrediction::addWeightUni / addWeightBi (TComWeightPrediction.cpp:61-237) of n 14-bit intermediates
__global__ void k_addavg(const short *a, const short *b, short *d, int n, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = (short)add_avg(a[i], b[i], B);
}
__global__ void k_weight_uni(const short *a, short *d, int n, WpPair q, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = (short)weight_uni(a[i], q, B);
}
__global__ void k_weight_bi(const short *a, const short *b, short *d, int n, WpPair q, int B) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) d[i] = (short)weight_bi(a[i], b[i], q, B);
}
// motionCompensation of ONE prediction unit (TComPrediction.cpp:410-552): xPredInterUni per used list (isLast = uni-prediction),
// TComYuv::addAvg when both lists are used.  ref0 / ref1: planes of the reference pictures (plane[i] at sample (0,0), margins
// readable), NULL = list unused; (x, y, w, h): the unit in luma samples; dst: plane[i] at the unit's first sample.
// weighted (:421-432, :516-535): every list makes 14-bit samples, addWeightUni / addWeightBi with the entries wp0 / wp1 end it.
static int mc_one(hmx_ctx *c, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x, int y, int w, int h,
                  const hmx_pic *dst, bool weighted, const hmx_wp *wp0, const hmx_wp *wp1) {
  const bool bi = ref0 && ref1, mid = bi || weighted; // mid: the lists' predictions stay 14-bit on the device
  const int B = c->cfg.bit_depth, head = 14 - B;
  for (int p = 0; p < 3; p++) {
    const int ch = p ? 1 : 0, pw = w >> ch, ph = h >> ch;
    Scratch s{c};
    short *d_pred[2] = {nullptr, nullptr};
    if (mid) { // both 14-bit intermediates stay on the device (the tail of the scratch area), addAvg there
      d_pred[0] = s.take_tail<short>(2 * 64 * 64);
      d_pred[1] = d_pred[0] + 64 * 64;
    }
    for (int l = 0; l < 2; l++) {
      const hmx_pic *rp = l ? ref1 : ref0;
      const int *mv = l ? mv1 : mv0;
      if (!rp) continue;
      const hmx_pel *r0 = rp->plane[p] + (ptrdiff_t)(y >> ch) * rp->stride[p] + (x >> ch);
      int r = pred_inter_blk(c, s, r0, rp->stride[p], mv[0], mv[1], pw, ph, dst->plane[p], dst->stride[p], mid, ch, mid ? d_pred[l] : nullptr);
      if (r) return r;
    }
    if (mid) {
      s.rewind();
      short *d_out = s.take<short>((size_t)pw * ph);
      if (s.r) return s.r;
      const dim3 grid((pw * ph + 255) / 256), blk(256);
      if (!weighted) {
        hipLaunchKernelGGL(k_addavg, grid, blk, 0, c->stream, d_pred[0], d_pred[1], d_out, pw * ph, B);
      } else {
        const auto at = [&](const hmx_wp &e) { return wp_entry_make(e.weight[p], e.offset[p], e.log2_denom[p], B); };
        const WpEntry e0 = at(ref0 ? *wp0 : *wp1), e1 = bi ? at(*wp1) : e0;
        const WpPair q = wp_pair(e0, e1, bi, head);
        if (bi) hipLaunchKernelGGL(k_weight_bi, grid, blk, 0, c->stream, d_pred[0], d_pred[1], d_out, pw * ph, q, B);
        else hipLaunchKernelGGL(k_weight_uni, grid, blk, 0, c->stream, d_pred[ref0 ? 0 : 1], d_out, pw * ph, q, B);
      }
      HIPCHK(c, hipGetLastError());
      int r = down2d(c, dst->plane[p], dst->stride[p], d_out, 2, pw, ph);
      if (r) return r;
    }
  }
  return HMX_OK;
}
static bool mc_one_args_ok(hmx_ctx *c, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int w, int h, const hmx_pic *dst) {
  return c && dst && (ref0 || ref1) && (!ref0 || mv0) && (!ref1 || mv1) && w > 0 && h > 0 && w <= 64 && h <= 64 && !(w & 1) && !(h & 1);
}
extern "C" int hmx_motionCompensation(hmx_ctx *c, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x, int y, int w,
                                      int h, const hmx_pic *dst) {
  if (!mc_one_args_ok(c, ref0, mv0, ref1, mv1, w, h, dst)) return fail(c, HMX_ERR_ARG, "hmx_motionCompensation: bad argument");
  return mc_one(c, ref0, mv0, ref1, mv1, x, y, w, h, dst, false, nullptr, nullptr);
}
extern "C" int hmx_motionCompensation_wp(hmx_ctx *c, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x, int y,
                                         int w, int h, const hmx_pic *dst, const hmx_wp *wp0, const hmx_wp *wp1) {
  if (!mc_one_args_ok(c, ref0, mv0, ref1, mv1, w, h, dst) || (ref0 && !wp0) || (ref1 && !wp1))
    return fail(c, HMX_ERR_ARG, "hmx_motionCompensation_wp: bad argument");
  for (int l = 0; l < 2; l++)
    for (int p = 0; p < 3; p++) {
      const hmx_wp *e = l ? wp1 : wp0;
      if ((l ? ref1 : ref0) && !wp_range_ok(e->weight[p], e->offset[p], e->log2_denom[p]))
        return fail(c, HMX_ERR_ARG, "hmx_motionCompensation_wp: weight outside -128..255, offset outside -128..127 or log2_denom > 7");
    }
  return mc_one(c, ref0, mv0, ref1, mv1, x, y, w, h, dst, true, wp0, wp1);
}

// ---- the encoder's sub-pel refinement fan-out (HOT LOOP C) ----
// xPatternSearchFracDIF (TEncSearch.cpp:4480-4514) makes the half- and quarter-sample planes of a prediction unit
// (xExtDIFUpSamplingH / Q, :5982-6165: filterHorLuma(frac x, isLast = false) into the 14-bit intermediate, then
// filterVerLuma(frac y, isFirst = false, isLast = true), zero fractions included) and costs nine candidates per stage
// (xPatternRefinement, :711-760) with xGetHADs / xGetSAD (TComRdCost.cpp:2186-2283, :488-516).  The sample a plane holds
// at a candidate's position depends on the position alone, so the fan-out is: for every unit and every candidate
// displacement (integer vector + up to 3 quarter samples either way) the distortion of the displaced two-stage
// prediction against the original.  One thread = one 8x8 (4x4) sub-block of one unit at one candidate: column by column
// the horizontal stage of the 15 (11) rows it needs, the vertical stage, the difference; then the Hadamard sum of the
// sub-block (rounded per sub-block as the reference does) or its SAD, added to the unit's candidate.
struct SubpelArgs {
  const hmx_pu *pus;
  const uint32_t *first; // [n + 1] prefix of sub-blocks per unit
  int n;
  PlanesDev refs[4];
  PlanesDev org;
  const signed char *offs; // [n_cand][2]
  int n_cand, use_had, B;
  uint32_t *cost; // [n][n_cand]
  static constexpr bool weighted = false;
};
struct SubpelArgsWp : SubpelArgs { // the weighted launch's arguments (as MeArgsWp in hmx_me.hip): the unweighted kernel keeps its argument block
  MeWp wp[4];                      // the luma entry of refs[k]
  static constexpr bool weighted = true;
};
// ARGS::weighted (SubpelArgsWp, uniform over a launch): the weighted distortion of TComRdCostWeightPrediction.cpp (xGetSADw :69-104, xGetHADsw :490-561):
// the difference is org - me_wp_pel(entry of the unit's reference, the final clipped sample); nothing else changes.
template <class ARGS>
__global__ __launch_bounds__(64) void k_subpel_cost(ARGS A) {
  const uint32_t sb = blockIdx.x * blockDim.x + threadIdx.x;
  const int cand = blockIdx.y;
  if (sb >= A.first[A.n]) return;
  int lo = 0, hi = A.n; // the unit this sub-block belongs to
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (A.first[mid] <= sb) lo = mid;
    else hi = mid;
  }
  const hmx_pu pu = A.pus[lo];
  const int w = pu.w, h = pu.h, n = (w % 8 == 0 && h % 8 == 0) ? 8 : 4, bw = w / n, k = (int)(sb - A.first[lo]);
  const int bx = pu.x + (k % bw) * n, by = pu.y + (k / bw) * n;
  const int mvx = pu.mv0x + A.offs[2 * cand], mvy = pu.mv0y + A.offs[2 * cand + 1];
  const int xf = mvx & 3, yf = mvy & 3, B = A.B;
  const InterpStage st2 = interp_stage(false, true, B); // filterVerLuma(isFirst = false, isLast = true)
  const PlanesDev &R = A.refs[pu.ref0 < 4 ? pu.ref0 : 0];
  const short *ref = R.p[0] + (ptrdiff_t)(by + (mvy >> 2)) * R.s[0] + bx + (mvx >> 2);
  const short *org = A.org.p[0] + (size_t)by * A.org.s[0] + bx;
  int d[64];
  for (int c = 0; c < n; c++) {
    int t[15]; // horizontal stage of rows -3 .. n+3 of this column (isFirst = true, isLast = false)
    for (int r = 0; r < n + 7; r++) t[r] = interp_sample<8>(ref + (ptrdiff_t)(r - 3) * R.s[0] + c, 1, xf, true, false, B);
    for (int r = 0; r < n; r++) {
      int v;
      if (yf == 0) { // filterCopy, last only (:124-145)
        v = interp_copy(t[r + 3], false, true, B);
      } else {
        int sum = 0;
        for (int q = 0; q < 8; q++) sum += t[r + q] * luma_tap(yf, q);
        v = clip3(st2.lo, st2.hi, wrap16((sum + st2.offset) >> st2.shift));
      }
      if constexpr (ARGS::weighted) d[r * 8 + c] = org[(size_t)r * A.org.s[0] + c] - me_wp_pel(A.wp[pu.ref0 < 4 ? pu.ref0 : 0], v);
      else d[r * 8 + c] = org[(size_t)r * A.org.s[0] + c] - v;
    }
  }
  atomicAdd(&A.cost[(size_t)lo * A.n_cand + cand], (unsigned)subblock_dist(d, n, A.use_had != 0));
}
__global__ void k_shift_u32(uint32_t *v, size_t n, int sh) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] >>= sh;
}
static int subpel_cost(hmx_ctx *c, const char *name, const hmx_pu *pus, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org, const int8_t *offs,
                       int n_cand, int use_had, uint32_t *d_cost, const hmx_wp *wp) {
  if (!c || !pus || n <= 0 || !refs || n_refs <= 0 || n_refs > 4 || !org || !offs || n_cand <= 0 || n_cand > 49 || !d_cost)
    return fail(c, HMX_ERR_ARG, std::string(name) + ": bad argument");
  MeWp wpt[4] = {};
  if (wp)
    if (const int r = me_wp_table(c, name, wp, n_refs, wpt)) return r;
  std::vector<uint32_t> first((size_t)n + 1, 0);
  for (int i = 0; i < n; i++) {
    const int w = pus[i].w, h = pus[i].h;
    if (w <= 0 || h <= 0 || w > 64 || h > 64 || ((w | h) & 3) || pus[i].ref0 >= n_refs || ((pus[i].mv0x | pus[i].mv0y) & 3))
      return fail(c, HMX_ERR_ARG, std::string(name) + ": unit size not a multiple of 4, reference index, or a vector that is not integer");
    const int nb = (w % 8 == 0 && h % 8 == 0) ? 8 : 4;
    first[i + 1] = first[i] + (uint32_t)((w / nb) * (h / nb));
  }
  for (int k = 0; k < 2 * n_cand; k++)
    if (offs[k] < -3 || offs[k] > 3) return fail(c, HMX_ERR_ARG, std::string(name) + ": candidate further than 3 quarter samples");
  SubpelArgsWp A{};
  const size_t pu_bytes = sizeof(hmx_pu) * (size_t)n, first_bytes = sizeof(uint32_t) * ((size_t)n + 1);
  // unit list, prefix and offsets through the argument arena (the caller's host arrays, and a table made from them), reserved together
  if (const int r = arena_reserve(c, {pu_bytes, first_bytes, (size_t)2 * n_cand}, "argument arena (unit list too long: split the call)")) return r;
  A.pus = static_cast<const hmx_pu *>(arena_place(c, pus, pu_bytes));
  A.first = static_cast<const uint32_t *>(arena_place(c, first.data(), first_bytes));
  A.offs = static_cast<const signed char *>(arena_place(c, offs, (size_t)2 * n_cand));
  if (!A.pus || !A.first || !A.offs) return fail(c, HMX_ERR_INTERNAL, kArenaOutside);
  A.n = n;
  A.n_cand = n_cand;
  A.use_had = use_had;
  A.cost = d_cost;
  HIPCHK(c, hipMemsetAsync(d_cost, 0, sizeof(uint32_t) * (size_t)n * n_cand, c->stream));
  me_launch<SubpelArgs>(c, A, refs, n_refs, org, wp != nullptr, wpt, [&](const auto &a) {
    hipLaunchKernelGGL(k_subpel_cost<std::decay_t<decltype(a)>>, dim3((first[n] + 63) / 64, (unsigned)n_cand), dim3(64), 0, c->stream, a);
  });
  if (c->cfg.bit_depth > 8) // xGetHADs / xGetSAD return uiSum >> g_uiBitIncrement
    hipLaunchKernelGGL(k_shift_u32, dim3((unsigned)(((size_t)n * n_cand + 255) / 256)), dim3(256), 0, c->stream, d_cost, (size_t)n * n_cand, c->cfg.bit_depth - 8);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_batch_subpel_cost(hmx_ctx *c, const hmx_pu *pus, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                                     const int8_t *offs, int n_cand, int use_had, uint32_t *d_cost) {
  return subpel_cost(c, "hmx_batch_subpel_cost", pus, n, refs, n_refs, org, offs, n_cand, use_had, d_cost, nullptr);
}
extern "C" int hmx_batch_subpel_cost_wp(hmx_ctx *c, const hmx_pu *pus, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                                        const int8_t *offs, int n_cand, int use_had, uint32_t *d_cost, const hmx_wp *wp) {
  return subpel_cost(c, "hmx_batch_subpel_cost_wp", pus, n, refs, n_refs, org, offs, n_cand, use_had, d_cost, wp);
}

extern "C" int hmx_addAvg(hmx_ctx *c, const hmx_pel *s0, int s0s, const hmx_pel *s1, int s1s, hmx_pel *dst, int ds, int w,
                          int h) {
  if (!c || !s0 || !s1 || !dst || w <= 0 || h <= 0 || w > 128 || h > 128) return fail(c, HMX_ERR_ARG, "hmx_addAvg: bad argument");
  Scratch s{c};
  short *da = s.up(s0, w, h, s0s), *db = s.up(s1, w, h, s1s), *dd = s.take<short>((size_t)w * h);
  if (s.r) return s.r;
  hipLaunchKernelGGL(k_addavg, dim3((w * h + 255) / 256), dim3(256), 0, c->stream, da, db, dd, w * h, c->cfg.bit_depth);
  HIPCHK(c, hipGetLastError());
  return down2d(c, dst, ds, dd, 2, w, h);
}

// The scalar entries of one component: src = 14-bit intermediates, weight / offset / log2_denom = iWeight / iOffset (8-bit units) /
// uiLog2WeightDenom of the entries getWpScaling derives from
extern "C" int hmx_addWeightUni(hmx_ctx *c, const hmx_pel *src, int ss, hmx_pel *dst, int ds, int w, int h, int weight, int offset,
                                int log2_denom) {
  if (!c || !src || !dst || w <= 0 || h <= 0 || w > 128 || h > 128) return fail(c, HMX_ERR_ARG, "hmx_addWeightUni: bad argument");
  if (!wp_range_ok(weight, offset, log2_denom))
    return fail(c, HMX_ERR_ARG, "hmx_addWeightUni: weight outside -128..255, offset outside -128..127 or log2_denom > 7");
  const int B = c->cfg.bit_depth;
  Scratch s{c};
  short *da = s.up(src, w, h, ss), *dd = s.take<short>((size_t)w * h);
  if (s.r) return s.r;
  hipLaunchKernelGGL(k_weight_uni, dim3((w * h + 255) / 256), dim3(256), 0, c->stream, da, dd, w * h,
                     wp_pair(wp_entry_make(weight, offset, log2_denom, B), WpEntry{}, false, 14 - B), B);
  HIPCHK(c, hipGetLastError());
  return down2d(c, dst, ds, dd, 2, w, h);
}
extern "C" int hmx_addWeightBi(hmx_ctx *c, const hmx_pel *s0, int s0s, const hmx_pel *s1, int s1s, hmx_pel *dst, int ds, int w, int h,
                               int weight0, int weight1, int offset0, int offset1, int log2_denom) {
  if (!c || !s0 || !s1 || !dst || w <= 0 || h <= 0 || w > 128 || h > 128) return fail(c, HMX_ERR_ARG, "hmx_addWeightBi: bad argument");
  if (!wp_range_ok(weight0, offset0, log2_denom) || !wp_range_ok(weight1, offset1, log2_denom))
    return fail(c, HMX_ERR_ARG, "hmx_addWeightBi: weight outside -128..255, offset outside -128..127 or log2_denom > 7");
  const int B = c->cfg.bit_depth;
  Scratch s{c};
  short *da = s.up(s0, w, h, s0s), *db = s.up(s1, w, h, s1s), *dd = s.take<short>((size_t)w * h);
  if (s.r) return s.r;
  hipLaunchKernelGGL(k_weight_bi, dim3((w * h + 255) / 256), dim3(256), 0, c->stream, da, db, dd, w * h,
                     wp_pair(wp_entry_make(weight0, offset0, log2_denom, B), wp_entry_make(weight1, offset1, log2_denom, B), true, 14 - B), B);
  HIPCHK(c, hipGetLastError());
  return down2d(c, dst, ds, dd, 2, w, h);
}

// ---- motionCompensation over PU lists ----
struct McJob { // one picture: its prediction units, its reference pictures, its destination planes
  const hmx_pu *pus;
  int n, ref_off; // refs of this job start at McArgs::refs[ref_off]
  PlanesDev dst;
  int *map;       // cell -> PU index (-1: none), cw x ch cells of 4x4 luma samples; NULL: one wave per PU
  int cw, ch;
};
struct McArgs {
  const McJob *jobs;     // [grid.y]
  const PlanesDev *refs; // all jobs' reference tables, back to back
  int B;
};
// Explicit weighted prediction (TComWeightPrediction.cpp:61-313): one entry per (reference, list), next to McArgs::refs
// and indexed like it, [2 * (J.ref_off + ref) + list]; o is iOffset already scaled to the bit depth.
struct alignas(16) WpDev { // one 16-byte load
  short w[3], o[3];
  unsigned char d[3], pad;
  __host__ __device__ WpEntry at(int pl) const { return WpEntry{w[pl], o[pl], d[pl]}; }
};
struct McArgsWp : McArgs {
  const WpDev *wp;
};
template <bool WP>
using McArgsOf = std::conditional_t<WP, McArgsWp, McArgs>;
// ---- the prediction of one cell, on packed 16-bit pairs ----
// A cell is 4x4 luma samples (2x2 chroma) of one PU.  Its reference window is read row by row with
// DWORD-ALIGNED wide loads (x4 + x2 / x3 per row: tools/loadshape_probe.hip measures 41 cycles per wave-row
// against 105 for the same loads at a 2-byte-aligned address and 194 for twelve 16-bit loads), the samples stay
// packed two per register as they lie in memory, and both filter stages run on v_dot2_i32_i16 (two taps per
// instruction, full rate).  With p = 1 when the window starts on the odd half of a dword, output c of a
// row starts at sample p + c of the loaded registers d[]:
//   p + c even:  pairs d[(p+c)/2 + j] with tap pairs (t0,t1)(t2,t3)...                 NTAP/2 products
//   p + c odd:   pairs d[(p+c-1)/2 + j] with the taps moved up by one, (0,t0)(t1,t2)...(t7,0)   NTAP/2+1
// Both cases are written as NTAP/2+1 products on d[c/2 + j] with a tap set chosen by (fraction, p) -- T0 for
// even c, T1 for odd c, one of them padded with a zero pair -- so no lane ever re-aligns samples and the
// lanes of a wave (different PUs, fractions and parities) run the same instructions.  Every cell takes the
// two-stage route (horizontal into the 14-bit intermediate, then vertical), a zero fraction being the filter
// {0,..,64,..,0}: bit-identical to the reference's one-stage and copy cases (interp_stage, hmx_kernels.h).
template <int NTAP>
__device__ __forceinline__ int tap_pair(int frac, int k) { // the pair (t[k], t[k+1]); taps outside 0..NTAP-1 are 0
  auto tap = [&](int t) { return (t < 0 || t >= NTAP) ? 0 : (NTAP == 8 ? luma_tap(frac, t) : chroma_tap(frac, t)); };
  return (tap(k) & 0xffff) | (tap(k + 1) << 16);
}
// table[frac][p][set][j]: set 0 = T0 (even c), set 1 = T1 (odd c); rows padded to 12 / 8 registers
constexpr int kLumaRow = 12, kChromaRow = 8;
constexpr int kTapTable = 4 * 2 * kLumaRow + 8 * 2 * kChromaRow;
template <int NTAP>
__device__ __forceinline__ int tap_table_entry(int frac, int p, int i) {
  constexpr int NO = NTAP / 2 + 1;
  if (i >= 2 * NO) return 0;
  const int set = i / NO, j = i % NO;
  // p + c even (set == p): even pairs from register 0 when c is even, from register 1 when c is odd
  if (set == p) return set == 0 ? tap_pair<NTAP>(frac, 2 * j) : tap_pair<NTAP>(frac, 2 * j - 2);
  return tap_pair<NTAP>(frac, 2 * j - 1);
}
__device__ __forceinline__ void fill_tap_table(int *lds, int tid, int nthreads) {
  for (int i = tid; i < kTapTable; i += nthreads) {
    if (i < 8 * kLumaRow) lds[i] = tap_table_entry<8>(i / (2 * kLumaRow), (i / kLumaRow) & 1, i % kLumaRow);
    else {
      const int k = i - 8 * kLumaRow;
      lds[i] = tap_table_entry<4>(k / (2 * kChromaRow), (k / kChromaRow) & 1, k % kChromaRow);
    }
  }
  __syncthreads();
}
typedef short s2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int dot2(int pair, int taps, int acc) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s2v, pair), __builtin_bit_cast(s2v, taps), acc, false);
}

// Prediction of one list for a W x H cell whose first sample is `ref` in the reference plane:
// xPredInterLumaBlk / ChromaBlk (:554-642) restricted to the cell.  The reference's two-stage
// filtering is position-wise (every output is the vertical filter of horizontally filtered rows), so
// cutting a PU into cells gives the same samples.  Rows go to emit(r, v[W]) as they are finished.
template <int NTAP, int W, int H, typename Emit>
__device__ __forceinline__ void mc_cell(const int *lds_taps, const short *ref, int rs, int mvx, int mvy, bool bi, int B, Emit emit) {
  constexpr int SH = NTAP == 8 ? 2 : 3, MASK = (1 << SH) - 1, HALF = NTAP / 2, R = H + NTAP - 1;
  constexpr int ND = (W + NTAP + 1) / 2;        // registers per window row: 12 / 6 samples, W + NTAP of them used
  constexpr int NE = NTAP / 2, NO = NTAP / 2 + 1, NP = (R + 1) / 2, ROW = NTAP == 8 ? kLumaRow : kChromaRow;
  typedef __attribute__((address_space(1))) const short gpel; // the table pointer is generic to the compiler: no FLAT loads
  typedef __attribute__((address_space(1))) const int gword;
  const gpel *win = (const gpel *)ref + (mvx >> SH) - (HALF - 1) + (ptrdiff_t)((mvy >> SH) - (HALF - 1)) * rs;
  const int p = (int)(((uintptr_t)win >> 1) & 1); // window starts on the odd half of a dword: start one sample earlier
  win -= p; // (with an odd stride every other row is still 2-byte aligned: the same samples, merely slower loads)
  const int *base = lds_taps + (NTAP == 8 ? 0 : 8 * kLumaRow);
  const int *tx = base + ((mvx & MASK) * 2 + p) * ROW, *ty = base + (mvy & MASK) * 2 * ROW;
  int t0[NO], t1[NO], ey[NE], oy[NO];
#pragma unroll
  for (int j = 0; j < NO; j++) t0[j] = tx[j], t1[j] = tx[NO + j], oy[j] = ty[NO + j];
#pragma unroll
  for (int j = 0; j < NE; j++) ey[j] = ty[j];
  // stage 1, first and not last; narrowed to 16 bits by the packing below.  Stage 2, not first: the last stage of a lane with one
  // list, clipped; else the 14-bit sample addAvg or the weighting takes
  const InterpStage st1 = interp_stage(true, false, B), st2 = interp_stage(false, !bi, B);
  int P[NP][W]; // the intermediate, rows 2k and 2k+1 packed per column
  int lo[W];
  // The rows are fetched four at a time, one chunk ahead of the arithmetic: a wave spends its life waiting for
  // window rows (25 us per wave against 2 us of VALU issue when every row was loaded where it is used), so the
  // loads of the next chunk are in flight while this one is filtered.
  constexpr int CH = 4, NCH = (R + CH - 1) / CH;
  int buf[2][CH][ND];
  auto fetch = [&](int k, int (&dst)[CH][ND]) {
#pragma unroll
    for (int i = 0; i < CH; i++)
      if (k * CH + i < R) __builtin_memcpy(dst[i], (gword *)(win + (ptrdiff_t)(k * CH + i) * rs), ND * 4);
  };
  fetch(0, buf[0]);
#pragma unroll
  for (int k = 0; k < NCH; k++) {
    if (k + 1 < NCH) fetch(k + 1, buf[(k + 1) & 1]);
#pragma unroll
    for (int i = 0; i < CH; i++) {
      const int r = k * CH + i;
      if (r < R) {
        const int *d = buf[k & 1][i];
#pragma unroll
        for (int c = 0; c < W; c++) {
          int s = st1.offset;
#pragma unroll
          for (int j = 0; j < NO; j++) s = dot2(d[c / 2 + j], c % 2 ? t1[j] : t0[j], s);
          s >>= st1.shift;
          if (r % 2 == 0) lo[c] = s;
          else P[r / 2][c] = (int)__builtin_amdgcn_perm((unsigned)s, (unsigned)lo[c], 0x05040100u);
        }
      }
    }
  }
  if (R % 2)
#pragma unroll
    for (int c = 0; c < W; c++) P[NP - 1][c] = lo[c] & 0xffff;
#pragma unroll
  for (int r = 0; r < H; r++) {
    int v[W];
#pragma unroll
    for (int c = 0; c < W; c++) {
      int s = st2.offset;
      if (r % 2 == 0) {
#pragma unroll
        for (int j = 0; j < NE; j++) s = dot2(P[r / 2 + j][c], ey[j], s);
      } else {
#pragma unroll
        for (int j = 0; j < NO; j++) s = dot2(P[r / 2 + j][c], oy[j], s);
      }
      v[c] = interp_end(st2, s);
    }
    emit(r, v);
  }
}

// Prediction of one plane's W x H cell from both lists (+ addAvg) into dst.  Pass one runs for every lane: the
// only list of a uni-predicted PU (final samples, stored) or list 0 of a bi-predicted one (14-bit samples, kept
// packed two per register); pass two runs list 1 for the bi-predicted lanes and stores addAvg rows.
// WP (explicit weighted prediction, TComPrediction.cpp:421-432, :516-535): pass one makes 14-bit samples for every lane
// (xPredInterUni(..., bi = true)); a uni-predicted lane stores weight_uni of them, pass two stores weight_bi instead of addAvg.
template <int NTAP, int W, int H, bool WP = false>
__device__ __forceinline__ void mc_cell_plane(const int *lds_taps, const McArgsOf<WP> &A, const McJob &J, const hmx_pu &u, int pl, int x, int y) {
  typedef __attribute__((address_space(1))) short gpel;
  const bool bi = u.ref0 != 255 && u.ref1 != 255, first1 = u.ref0 == 255;
  gpel *d = (gpel *)J.dst.p[pl] + (size_t)y * J.dst.s[pl] + x;
  const int ds = J.dst.s[pl];
  unsigned keep[H * W / 2];
  WpPair wq{}; // this plane's weights (WP only)
  if constexpr (WP) {
    typedef int i4v __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(1))) const i4v gwp;
    const gwp *tab = (const gwp *)A.wp + 2 * J.ref_off;
    const auto entry = [&](int k) { return __builtin_bit_cast(WpDev, (i4v)tab[k]).at(pl); }; // one 16-byte load
    const WpEntry e0 = entry(first1 ? 2 * u.ref1 + 1 : 2 * u.ref0), e1 = bi ? entry(2 * u.ref1 + 1) : e0;
    wq = wp_pair(e0, e1, bi, 14 - A.B);
  }
  {
    const PlanesDev &R = A.refs[J.ref_off + (first1 ? u.ref1 : u.ref0)];
    mc_cell<NTAP, W, H>(lds_taps, R.p[pl] + (ptrdiff_t)y * R.s[pl] + x, R.s[pl], first1 ? u.mv1x : u.mv0x, first1 ? u.mv1y : u.mv0y,
                        WP || bi, A.B, [&](int r, const int *v) {
                          short row[W];
#pragma unroll
                          for (int c = 0; c < W; c++) row[c] = (short)v[c];
#pragma unroll
                          for (int c = 0; c < W; c += 2) keep[(r * W + c) / 2] = (unsigned)(unsigned short)row[c] | ((unsigned)(unsigned short)row[c + 1] << 16);
                          if constexpr (WP) {
                            if (!bi) {
#pragma unroll
                              for (int c = 0; c < W; c++) row[c] = (short)weight_uni(v[c], wq, A.B);
                            }
                          }
                          if (!bi) __builtin_memcpy(d + (size_t)r * ds, row, W * 2); // one 8-byte (4-byte) store per row
                        });
  }
  if (bi) {
    const PlanesDev &R = A.refs[J.ref_off + u.ref1];
    mc_cell<NTAP, W, H>(lds_taps, R.p[pl] + (ptrdiff_t)y * R.s[pl] + x, R.s[pl], u.mv1x, u.mv1y, true, A.B, [&](int r, const int *v) {
      short row[W];
#pragma unroll
      for (int c = 0; c < W; c += 2) {
        const unsigned k = keep[(r * W + c) / 2];
        if constexpr (WP) {
          row[c] = (short)weight_bi((int)(short)(k & 0xffff), v[c], wq, A.B);
          row[c + 1] = (short)weight_bi((int)(short)(k >> 16), v[c + 1], wq, A.B);
        } else {
          row[c] = (short)add_avg((int)(short)(k & 0xffff), v[c], A.B);
          row[c + 1] = (short)add_avg((int)(short)(k >> 16), v[c + 1], A.B);
        }
      }
      __builtin_memcpy(d + (size_t)r * ds, row, W * 2);
    });
  }
}

// Two ways to hand cells to lanes.  With the picture size known (hmx_mc_job::pic_w/pic_h) a scatter pass
// writes each PU's index into a cell map and the prediction kernel runs one lane per cell of the PICTURE:
// every wave is full whatever the PU sizes.  Without it, one wave per PU, its lanes looping over the
// PU's cells (an 8x4 PU keeps 2 of 64 lanes busy).  A cell reads its (W+7) / (W+3) window rows straight
// from the margin-extended reference planes (the caches absorb the overlap between neighbouring
// cells); nothing is staged, nothing synchronises after the tap table is in LDS.
__global__ __launch_bounds__(256) void k_mc_map(McArgs A) { // 16 threads per PU, one per row of its cells (PUs are <= 64 high)
  const McJob J = A.jobs[blockIdx.y];
  const int pi = blockIdx.x * 16 + (threadIdx.x >> 4), r = threadIdx.x & 15;
  if (pi >= J.n) return;
  const hmx_pu u = J.pus[pi];
  if (u.ref0 == 255 && u.ref1 == 255) return;
  const int cw = u.w >> 2, rows = u.h >> 2;
  for (int rr = r; rr < rows; rr += 16) { // one pass for every legal PU
    const int cy = (u.y >> 2) + rr;
    if (cy >= J.ch) break;
    for (int i = 0; i < cw; i++)
      if ((u.x >> 2) + i < J.cw) J.map[(size_t)cy * J.cw + (u.x >> 2) + i] = pi;
  }
}
template <bool WP>
__global__ __launch_bounds__(256) void k_mc_cells(McArgsOf<WP> A) {
  __shared__ int taps[kTapTable];
  fill_tap_table(taps, threadIdx.x, 256);
  const McJob J = A.jobs[blockIdx.y];
  // A lane owns two vertically adjacent cells (4 x 8 luma samples); a wave 8 x 8 such pairs = 32 x 64 samples, a
  // workgroup 64 x 128: the window rows of the cells of one PU fall into the same cache lines of the same load
  // instruction, and rows shared by vertical neighbours are fetched by the same wave.  When both cells belong to
  // ONE PU (every PU at least 8 high does that) they are predicted as one 4 x 8 cell -- 15 window rows instead of
  // 2 x 11, one horizontal pass over them; otherwise each cell on its own.
  const int tiles_x = (J.cw + 15) >> 4, tile = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int cx = (tile % tiles_x) * 16 + (wave & 1) * 8 + (lane & 7), cy = (tile / tiles_x) * 32 + (wave >> 1) * 16 + (lane >> 3) * 2;
  if (cx >= J.cw || cy >= J.ch) return;
  const int pi0 = J.map[cy * J.cw + cx], pi1 = cy + 1 < J.ch ? J.map[(cy + 1) * J.cw + cx] : -1;
  const int x = cx << 2, y = cy << 2;
  if (pi0 >= 0 && pi0 == pi1) {
    const hmx_pu u = J.pus[pi0];
    mc_cell_plane<8, 4, 8, WP>(taps, A, J, u, 0, x, y);
    mc_cell_plane<4, 2, 4, WP>(taps, A, J, u, 1, x >> 1, y >> 1);
    mc_cell_plane<4, 2, 4, WP>(taps, A, J, u, 2, x >> 1, y >> 1);
  } else {
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
      const int pi = k ? pi1 : pi0;
      if (pi < 0) continue;
      const hmx_pu u = J.pus[pi];
      mc_cell_plane<8, 4, 4, WP>(taps, A, J, u, 0, x, y + 4 * k);
      mc_cell_plane<4, 2, 2, WP>(taps, A, J, u, 1, x >> 1, (y >> 1) + 2 * k);
      mc_cell_plane<4, 2, 2, WP>(taps, A, J, u, 2, x >> 1, (y >> 1) + 2 * k);
    }
  }
}
template <bool WP>
__global__ __launch_bounds__(64) void k_mc(McArgsOf<WP> A) {
  __shared__ int taps[kTapTable];
  fill_tap_table(taps, threadIdx.x, 64);
  const McJob J = A.jobs[blockIdx.y];
  if ((int)blockIdx.x >= J.n) return; // jobs of one call may differ in length
  const hmx_pu u = J.pus[blockIdx.x];
  if (u.ref0 == 255 && u.ref1 == 255) return;
  const int cw = u.w >> 2, cells = cw * (u.h >> 2);
  for (int i = threadIdx.x; i < cells; i += 64) {
    const int x = u.x + ((i % cw) << 2), y = u.y + ((i / cw) << 2);
    mc_cell_plane<8, 4, 4, WP>(taps, A, J, u, 0, x, y);
    mc_cell_plane<4, 2, 2, WP>(taps, A, J, u, 1, x >> 1, y >> 1);
    mc_cell_plane<4, 2, 2, WP>(taps, A, J, u, 2, x >> 1, y >> 1);
  }
}

// One table entry checked and brought to the device form (getWpScaling :286-312: o = iOffset * (1 << (B - 8))).
static bool wp_entry(const hmx_wp &e, int B, WpDev *out) {
  for (int k = 0; k < 3; k++) {
    if (!wp_range_ok(e.weight[k], e.offset[k], e.log2_denom[k])) return false;
    out->w[k] = e.weight[k];
    out->o[k] = (short)(e.offset[k] * (1 << (B - 8)));
    out->d[k] = e.log2_denom[k];
  }
  out->pad = 0;
  return true;
}
// The jobs of one call, weighted ones (wp && wp[i].l0) first: the two kinds go to their own instantiations of the
// prediction kernel, so an unweighted job of a weighted call runs the very code of the unweighted call.
static int mc_multi(hmx_ctx *c, int n_jobs, const hmx_mc_job *jobs, const hmx_mc_wp *wp) {
  std::vector<McJob> hj(n_jobs);
  std::vector<PlanesDev> hr;
  std::vector<WpDev> hw;
  int n_kind[2] = {0, 0}, max_n[2] = {0, 0}; // [1] = weighted
  size_t map_cells = 0, max_tiles[2] = {0, 0};
  bool mapped = true;
  if (wp)
    for (int i = 0; i < n_jobs; i++) {
      if (!wp[i].l0 && wp[i].l1) return fail(c, HMX_ERR_ARG, "hmx_batch_motionCompensation_wp_multi: a weighted job needs the list 0 table (l0 NULL, l1 not)");
      n_kind[1] += wp[i].l0 != nullptr;
    }
  n_kind[0] = n_jobs - n_kind[1];
  int next[2] = {n_kind[1], 0}; // weighted jobs take the front of hj
  for (int i = 0; i < n_jobs; i++) {
    const hmx_mc_job &j = jobs[i];
    if (j.n_pus < 0 || (j.n_pus > 0 && !j.d_pus) || !j.refs || j.n_refs <= 0 || j.n_refs > 16 || !j.dst || j.pic_w < 0 || j.pic_h < 0)
      return fail(c, HMX_ERR_ARG, "hmx_batch_motionCompensation_multi: bad job");
    const int kind = wp && wp[i].l0;
    McJob &h = hj[next[kind]++];
    h = McJob{j.d_pus, j.n_pus, (int)hr.size(), to_dev(j.dst), nullptr, (j.pic_w + 3) / 4, (j.pic_h + 3) / 4};
    for (int k = 0; k < j.n_refs; k++) hr.push_back(to_dev(&j.refs[k]));
    if (wp) { // entries of unweighted jobs are never read; a missing list 1 table holds the unit weight
      const hmx_wp unit = {{1, 1, 1}, {0, 0, 0}, {0, 0, 0}, 0};
      for (int k = 0; k < j.n_refs; k++)
        for (int l = 0; l < 2; l++) {
          const hmx_wp *t = l ? wp[i].l1 : wp[i].l0;
          WpDev e;
          if (!wp_entry(kind && t ? t[k] : unit, c->cfg.bit_depth, &e))
            return fail(c, HMX_ERR_ARG, "hmx_batch_motionCompensation_wp_multi: weight outside -128..255, offset outside -128..127 or log2_denom > 7");
          hw.push_back(e);
        }
    }
    max_n[kind] = std::max(max_n[kind], j.n_pus);
    const size_t cells = (size_t)h.cw * h.ch;
    mapped = mapped && cells > 0;
    map_cells += cells;
    max_tiles[kind] = std::max(max_tiles[kind], (size_t)((h.cw + 15) / 16) * ((h.ch + 31) / 32)); // 64 x 128 luma samples
  }
  if (!max_n[0] && !max_n[1]) return HMX_OK;
  if (mapped) { // cell maps of all jobs, back to back, in a grow-only scratch buffer
    if (int r = grow_dev(c, (void **)&c->d_mcmap, &c->mcmap_cap, map_cells * sizeof(int), "cell map")) return r;
    HIPCHK(c, hipMemsetAsync(c->d_mcmap, 0xff, map_cells * sizeof(int), c->stream));
    size_t off = 0;
    for (int i = 0; i < n_jobs; i++) {
      hj[i].map = c->d_mcmap + off;
      off += (size_t)hj[i].cw * hj[i].ch;
    }
  }
  // all tables in one copy
  const size_t jb = (sizeof(McJob) * hj.size() + 255) & ~(size_t)255, rb = (sizeof(PlanesDev) * hr.size() + 15) & ~(size_t)15;
  std::vector<char> blob(jb + rb + sizeof(WpDev) * hw.size());
  memcpy(blob.data(), hj.data(), sizeof(McJob) * hj.size());
  memcpy(blob.data() + jb, hr.data(), sizeof(PlanesDev) * hr.size());
  if (!hw.empty()) memcpy(blob.data() + jb + rb, hw.data(), sizeof(WpDev) * hw.size());
  char *d = static_cast<char *>(arena_push(c, blob.data(), blob.size()));
  if (!d) return fail(c, HMX_ERR_NOMEM, "argument arena");
  McArgsWp A;
  A.jobs = reinterpret_cast<const McJob *>(d);
  A.refs = reinterpret_cast<const PlanesDev *>(d + jb);
  A.B = c->cfg.bit_depth;
  A.wp = reinterpret_cast<const WpDev *>(d + jb + rb);
  McArgs U = A; // the unweighted jobs: the tail of the job table
  U.jobs = A.jobs + n_kind[1];
  if (mapped) {
    hipLaunchKernelGGL(k_mc_map, dim3((unsigned)((std::max(max_n[0], max_n[1]) + 15) / 16), (unsigned)n_jobs), dim3(256), 0, c->stream, static_cast<McArgs>(A));
    if (max_n[1]) hipLaunchKernelGGL(k_mc_cells<true>, dim3((unsigned)max_tiles[1], (unsigned)n_kind[1]), dim3(256), 0, c->stream, A);
    if (max_n[0]) hipLaunchKernelGGL(k_mc_cells<false>, dim3((unsigned)max_tiles[0], (unsigned)n_kind[0]), dim3(256), 0, c->stream, U);
  } else {
    if (max_n[1]) hipLaunchKernelGGL(k_mc<true>, dim3((unsigned)max_n[1], (unsigned)n_kind[1]), dim3(64), 0, c->stream, A);
    if (max_n[0]) hipLaunchKernelGGL(k_mc<false>, dim3((unsigned)max_n[0], (unsigned)n_kind[0]), dim3(64), 0, c->stream, U);
  }
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_batch_motionCompensation_multi(hmx_ctx *c, int n_jobs, const hmx_mc_job *jobs) {
  if (!c || !jobs || n_jobs <= 0 || n_jobs > 65535) return fail(c, HMX_ERR_ARG, "hmx_batch_motionCompensation_multi: bad argument");
  return mc_multi(c, n_jobs, jobs, nullptr);
}
// motionCompensation with TComWeightPrediction (TComPrediction.cpp:421-432, :516-535) over PU lists: wp[i] = the tables of jobs[i]
extern "C" int hmx_batch_motionCompensation_wp_multi(hmx_ctx *c, int n_jobs, const hmx_mc_job *jobs, const hmx_mc_wp *wp) {
  if (!c || !jobs || !wp || n_jobs <= 0 || n_jobs > 65535) return fail(c, HMX_ERR_ARG, "hmx_batch_motionCompensation_wp_multi: bad argument");
  return mc_multi(c, n_jobs, jobs, wp);
}

extern "C" int hmx_batch_motionCompensation(hmx_ctx *c, const hmx_pu *d_pus, int n, const hmx_pic *refs, int n_refs,
                                            const hmx_pic *dst) {
  if (!c || !d_pus || !refs || !dst || n_refs <= 0 || n_refs > 16) return fail(c, HMX_ERR_ARG, "hmx_batch_motionCompensation: bad argument");
  if (n <= 0) return HMX_OK;
  const hmx_mc_job j{d_pus, n, refs, n_refs, dst, 0, 0}; // picture size unknown here: one wave per PU
  return hmx_batch_motionCompensation_multi(c, 1, &j);
}

// ---- extendPicBorder (TComPicYuv.cpp:248-286): every margin sample is the nearest picture sample, so
// one launch covers all margins of all planes of all pictures (no left/right-then-up/down ordering) ----
__global__ __launch_bounds__(256) void k_border1(const PlanesDev *pics, int pic_w, int pic_h, int mx, int my) {
  const int pl = blockIdx.y % 3;
  const PlanesDev &D = pics[blockIdx.y / 3];
  const int sh = pl ? 1 : 0, w = pic_w >> sh, h = pic_h >> sh, bx = mx >> sh, by = my >> sh;
  const int ww = w + 2 * bx, band = ww * by, side = h * bx;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int x, y;
  if (i < band) { // above
    y = -1 - i / ww, x = i % ww - bx;
  } else if ((i -= band) < band) { // below
    y = h + i / ww, x = i % ww - bx;
  } else if ((i -= band) < side) { // left
    y = i / bx, x = -1 - i % bx;
  } else if ((i -= side) < side) { // right
    y = i / bx, x = w + i % bx;
  } else
    return;
  short *p = D.p[pl];
  const int s = D.s[pl];
  p[(ptrdiff_t)y * s + x] = p[(ptrdiff_t)min(max(y, 0), h - 1) * s + min(max(x, 0), w - 1)];
}
// The same with four samples per thread (one 8-byte store): for plane widths and margins that are multiples of
// four samples a group never straddles the picture edge, so it is either a copy of four picture samples
// (above / below the picture) or one edge sample four times.
__global__ __launch_bounds__(256) void k_border(const PlanesDev *pics, int pic_w, int pic_h, int mx, int my) {
  typedef __attribute__((address_space(1))) short gpel;
  const int pl = blockIdx.y % 3;
  const PlanesDev &D = pics[blockIdx.y / 3];
  const int sh = pl ? 1 : 0, w = pic_w >> sh, h = pic_h >> sh, bx = mx >> sh, by = my >> sh;
  const int gw = (w + 2 * bx) >> 2, gb = bx >> 2, band = gw * by, side = h * gb;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  int x, y;
  if (i < band) { // above
    y = -1 - i / gw, x = ((i % gw) << 2) - bx;
  } else if ((i -= band) < band) { // below
    y = h + i / gw, x = ((i % gw) << 2) - bx;
  } else if ((i -= band) < side) { // left
    y = i / gb, x = ((i % gb) << 2) - bx;
  } else if ((i -= side) < side) { // right
    y = i / gb, x = w + ((i % gb) << 2);
  } else
    return;
  gpel *p = (gpel *)wave_uniform(D.p[pl]);
  const int s = wave_uniform(D.s[pl]);
  gpel *src = p + (ptrdiff_t)min(max(y, 0), h - 1) * s;
  short v[4];
  if (x >= 0 && x < w) {
    __builtin_memcpy(v, src + x, 8);
  } else {
    v[0] = v[1] = v[2] = v[3] = src[x < 0 ? 0 : w - 1];
  }
  __builtin_memcpy(p + (ptrdiff_t)y * s + x, v, 8);
}
extern "C" int hmx_pic_extend_border_multi(hmx_ctx *c, int n_pics, const hmx_pic *pics, int pic_w, int pic_h, int mx, int my) {
  if (!c || !pics || n_pics <= 0 || n_pics > 21845 || mx < 0 || my < 0) return fail(c, HMX_ERR_ARG, "hmx_pic_extend_border_multi: bad argument");
  if (!mx && !my) return HMX_OK;
  std::vector<PlanesDev> t(n_pics);
  for (int i = 0; i < n_pics; i++) t[i] = to_dev(&pics[i]);
  const PlanesDev *d = static_cast<const PlanesDev *>(arena_push(c, t.data(), sizeof(PlanesDev) * n_pics));
  if (!d) return fail(c, HMX_ERR_NOMEM, "argument arena");
  const long long total = 2LL * (pic_w + 2 * mx) * my + 2LL * pic_h * mx; // luma margin samples (chroma has fewer)
  if (pic_w % 8 == 0 && mx % 8 == 0) // chroma width and margin are then multiples of four as well
    hipLaunchKernelGGL(k_border, dim3((unsigned)((total / 4 + 255) / 256), (unsigned)n_pics * 3), dim3(256), 0, c->stream, d, pic_w, pic_h, mx, my);
  else
    hipLaunchKernelGGL(k_border1, dim3((unsigned)((total + 255) / 256), (unsigned)n_pics * 3), dim3(256), 0, c->stream, d, pic_w, pic_h, mx, my);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_pic_extend_border(hmx_ctx *c, const hmx_pic *pic, int pic_w, int pic_h, int mx, int my) {
  if (!c || !pic) return fail(c, HMX_ERR_ARG, "hmx_pic_extend_border: bad argument");
  return hmx_pic_extend_border_multi(c, 1, pic, pic_w, pic_h, mx, my);
}


// =============================================================================================
// Prediction error of complete motion candidates: TEncSearch::xGetInterPredictionError (TEncSearch.cpp:3059-3081), fused
// =============================================================================================
// predInterSearch compares complete candidates -- the merge candidates of xMergeEstimation (:3096-3149), the search result the
// merge winner meets (:3771-3796), the AMVP candidates of xGetTemplateCost (:4057-4118) -- and each comparison is the luma part
// of motionCompensation (TComPrediction.cpp:410-540) followed by xGetHADs / xGetSAD against the original, UNWEIGHTED
// (bApplyWeight = false, :3070) also in a weighted slice.  One workgroup owns one GROUP of candidates of one unit: the original
// block goes to LDS once; per candidate and used list the (w + 7) x (h + 7) reference window is staged with coalesced row loads,
// xPredInterLumaBlk's three cases run on it (horizontal only, vertical only, horizontal into a 14-bit LDS intermediate then
// vertical), the second pass hands each finished sample straight to the combination (final sample; addAvg with the first list's
// 14-bit block, which waits in LDS; weightUnidir / weightBidir) and the difference, and S lanes (S = 8, or 4 when a side is no
// multiple of 8) form one sub-block: Hadamard down the lane's column in registers and across the lanes by shuffles, or the SAD.
// No prediction sample leaves the workgroup.  Thread 0 adds the bits term and keeps the running best of the group (:3139).
// LDS rows are padded to an odd number of dwords (pe_pitch): the sub-blocks of a wave that lie below each other start 8 (4)
// rows apart, and with an even pitch their columns would walk the same banks.
constexpr int kPeThreads = 256;
struct PeArgs {
  const hmx_pu *cands;
  const uint32_t *bits;  // NULL: 0 for every candidate
  const uint32_t *first; // [n_groups + 1]
  PlanesDev refs[4];
  PlanesDev org;
  int B, use_had;
  uint32_t lambda;
  uint32_t *dist, *cost;
  hmx_pred_choice *best; // NULL: costs only
  static constexpr bool weighted = false;
};
struct PeArgsWp : PeArgs { // as SubpelArgsWp: the unweighted kernel keeps its argument block
  WpEntry wp[4][2];        // the luma entry of [reference][list]
  static constexpr bool weighted = true;
};
__host__ __device__ constexpr int pe_pitch(int n) { return (((n + 1) >> 1) | 1) << 1; } // >= n samples, an odd number of dwords
static size_t pe_lds_bytes(int w, int h) { // original, window, intermediate, the first list's 14-bit block
  return sizeof(short) * (size_t)(w * h + pe_pitch(w + 7) * (h + 7) + pe_pitch(w) * (h + 7) + w * h);
}
enum PeMode { PE_FINAL, PE_KEEP, PE_AVG, PE_WUNI, PE_WBI };
// Every pass is a LumaFilter (hmx_kernels.h), a zero fraction included (interp_stage: the filter {.., 64, ..}), so a pass has no
// branch per sample and no table load per tap.
// k = tid, tid + nt, ... as (row, column) of a `cols`-wide block without a division per element
struct PeWalk {
  int r, c, dr, dc, cols;
  __device__ __forceinline__ PeWalk(int tid, int nt, int cols_) : r(tid / cols_), c(tid - (tid / cols_) * cols_), dr(nt / cols_), dc(nt - (nt / cols_) * cols_), cols(cols_) {}
  __device__ __forceinline__ void next() {
    r += dr, c += dc;
    if (c >= cols) c -= cols, r++;
  }
};
// The last filter pass of one list over the whole block, and what follows it.  src: the block's first sample in the window
// (first) or in the intermediate (!first), rows `pitch` apart; ver: the taps run down the column.  PE_KEEP stores the 14-bit
// samples in p0 and costs nothing; every other mode adds the block's distortion to *s_sum.
template <int S>
__device__ __forceinline__ void pe_cost_pass(const short *src, int pitch, bool ver, int frac, bool first, int mode, short *p0, const short *org, int w,
                                             int h, int B, int use_had, const WpPair &wq, unsigned *s_sum, int tid, int nthreads) {
  const int bw = w / S, lane = tid & (S - 1);
  const LumaFilter f = luma_filter(frac, first, mode == PE_FINAL, B);
  subblock_walk<S>(bw * (h / S), tid, nthreads, [&](int g, bool act) {
    const int sby = g / bw, sx = (g - sby * bw) * S + lane, sy = sby * S;
    const short *s = src + sy * pitch + sx;
    int d[S];
    if (ver) { // the column this lane filters, read once
      int col[S + 7];
#pragma unroll
      for (int q = 0; q < S + 7; q++) col[q] = s[(q - 3) * pitch];
      luma_column<S>(f, col, d);
    } else {
#pragma unroll
      for (int r = 0; r < S; r++) {
        int row[8];
#pragma unroll
        for (int q = 0; q < 8; q++) row[q] = s[r * pitch + q - 3];
        d[r] = luma_sample(f, row);
      }
    }
    short *k0 = p0 + sy * w + sx;
    if (mode == PE_KEEP) {
#pragma unroll
      for (int r = 0; r < S; r++) k0[r * w] = (short)d[r];
      return;
    }
    if (mode == PE_AVG) {
#pragma unroll
      for (int r = 0; r < S; r++) d[r] = add_avg(k0[r * w], d[r], B);
    } else if (mode == PE_WUNI) {
#pragma unroll
      for (int r = 0; r < S; r++) d[r] = weight_uni(d[r], wq, B);
    } else if (mode == PE_WBI) {
#pragma unroll
      for (int r = 0; r < S; r++) d[r] = weight_bi(k0[r * w], d[r], wq, B);
    }
    column_cost<S>(d, org + sy * w + sx, w, lane, use_had, act, s_sum);
  });
}
template <class ARGS>
__global__ __launch_bounds__(kPeThreads) void k_pred_error(ARGS A) {
  constexpr bool WP = ARGS::weighted;
  extern __shared__ __attribute__((aligned(16))) short s_pe[];
  __shared__ unsigned s_sum;
  typedef __attribute__((address_space(1))) const short gpel;
  const int grp = blockIdx.x, tid = threadIdx.x, nt = blockDim.x, B = A.B;
  const uint32_t c0 = A.first[grp], c1 = A.first[grp + 1];
  hmx_pred_choice best{0xffffffffu, 0xffffffffu, 0xffffffffu};
  if (c0 == c1) { // uniform over the workgroup
    if (tid == 0 && A.best) A.best[grp] = best;
    return;
  }
  const hmx_pu u0 = A.cands[c0];
  const int x = u0.x, y = u0.y, w = u0.w, h = u0.h, wp = pe_pitch(w + 7), tp = pe_pitch(w), ww = w + 7, rows = h + 7;
  short *org = s_pe, *win = org + w * h, *tmp = win + wp * rows, *p0 = tmp + tp * rows;
  const PeWalk walk_w(tid, nt, w), walk_ww(tid, nt, ww);
  {
    const gpel *so = (const gpel *)A.org.p[0] + (size_t)y * A.org.s[0] + x;
    PeWalk k = walk_w;
    for (int i = tid; i < w * h; i += nt, k.next()) org[i] = so[(size_t)k.r * A.org.s[0] + k.c];
  }
  if (tid == 0) s_sum = 0;
  const bool s8 = (w % 8 == 0) && (h % 8 == 0);
  for (uint32_t i = c0; i < c1; i++) {
    const hmx_pu u = A.cands[i];
    const bool bi = u.ref0 != 255 && u.ref1 != 255, mid = WP || bi; // mid: the lists' predictions are 14-bit samples
    WpPair wq{};
    if constexpr (WP) wq = wp_pair(u.ref0 != 255 ? A.wp[u.ref0 & 3][0] : A.wp[u.ref1 & 3][1], A.wp[u.ref1 & 3][1], bi, 14 - B);
    for (int l = 0; l < 2; l++) {
      const int ref = l ? u.ref1 : u.ref0;
      if (ref == 255) continue;
      const int mvx = l ? u.mv1x : u.mv0x, mvy = l ? u.mv1y : u.mv0y, xf = mvx & 3, yf = mvy & 3;
      const PlanesDev &R = A.refs[ref & 3];
      const gpel *sr = (const gpel *)R.p[0] + (ptrdiff_t)(y + (mvy >> 2) - 3) * R.s[0] + (x + (mvx >> 2) - 3);
      __syncthreads(); // the previous pass has read the window and the intermediate (the first time: the original is staged)
      {
        PeWalk k = walk_ww;
        for (int j = tid; j < ww * rows; j += nt, k.next()) win[k.r * wp + k.c] = sr[(ptrdiff_t)k.r * R.s[0] + k.c];
      }
      __syncthreads();
      const short *src = win + 3 * wp + 3;
      int pitch = wp, frac = xf;
      bool first = true, ver = false;
      if (xf && yf) { // filterHorLuma(isLast = false) of rows -3 .. h + 3, then filterVerLuma(isFirst = false) (TComPrediction.cpp:583-600)
        const LumaFilter f = luma_filter(xf, true, false, B);
        PeWalk k = walk_w;
        for (int j = tid; j < w * rows; j += nt, k.next()) {
          const short *s = win + k.r * wp + k.c;
          int row[8];
#pragma unroll
          for (int q = 0; q < 8; q++) row[q] = s[q];
          tmp[k.r * tp + k.c] = (short)luma_sample(f, row);
        }
        __syncthreads();
        src = tmp + 3 * tp, pitch = tp, frac = yf, first = false, ver = true;
      } else if (yf) {
        frac = yf, ver = true;
      }
      const int mode = !mid ? PE_FINAL : (bi && l == 0) ? PE_KEEP : bi ? (WP ? PE_WBI : PE_AVG) : PE_WUNI;
      if (s8) pe_cost_pass<8>(src, pitch, ver, frac, first, mode, p0, org, w, h, B, A.use_had, wq, &s_sum, tid, nt);
      else pe_cost_pass<4>(src, pitch, ver, frac, first, mode, p0, org, w, h, B, A.use_had, wq, &s_sum, tid, nt);
    }
    __syncthreads();
    if (tid == 0) { // getCost(UInt) (TComRdCost.h:204), all of it uint32_t; the next sum starts two barriers from here
      const uint32_t dist = s_sum >> (B - 8), cost = dist + ((A.lambda * (A.bits ? A.bits[i] : 0u)) >> 16);
      s_sum = 0;
      A.dist[i] = dist, A.cost[i] = cost;
      if (cost < best.cost) best = hmx_pred_choice{i - c0, dist, cost};
    }
  }
  if (tid == 0 && A.best) A.best[grp] = best;
}

// the launch: every argument has been checked; first (host): n_groups + 1 prefix entries
static int pe_launch(hmx_ctx *c, const hmx_pu *cands, const uint32_t *bits, int n, const uint32_t *first, int n_groups, const PlanesDev *refs, int n_refs,
                     const PlanesDev &org, uint32_t lambda, int use_had, uint32_t *d_dist, uint32_t *d_cost, hmx_pred_choice *d_best, const WpEntry (*wp)[2]) {
  size_t lds = 0;
  int threads = 64;
  for (int i = 0; i < n; i++) {
    const int w = cands[i].w, h = cands[i].h, s = (w % 8 == 0 && h % 8 == 0) ? 8 : 4;
    lds = std::max(lds, pe_lds_bytes(w, h));
    threads = std::max(threads, std::min(kPeThreads, (w * h / s + 63) & ~63)); // one lane per sub-block column
  }
  PeArgsWp A{};
  // the caller's host arrays, reserved together (no bits: no table)
  const size_t cand_bytes = sizeof(hmx_pu) * (size_t)n, bits_bytes = bits ? sizeof(uint32_t) * (size_t)n : 0, first_bytes = sizeof(uint32_t) * ((size_t)n_groups + 1);
  if (const int r = arena_reserve(c, {cand_bytes, bits_bytes, first_bytes}, "argument arena (candidate list too long: split the call)")) return r;
  A.cands = static_cast<const hmx_pu *>(arena_place(c, cands, cand_bytes));
  A.bits = bits ? static_cast<const uint32_t *>(arena_place(c, bits, bits_bytes)) : nullptr;
  A.first = static_cast<const uint32_t *>(arena_place(c, first, first_bytes));
  if (!A.cands || (bits && !A.bits) || !A.first) return fail(c, HMX_ERR_INTERNAL, kArenaOutside);
  for (int r = 0; r < n_refs; r++) A.refs[r] = refs[r];
  A.org = org;
  A.B = c->cfg.bit_depth, A.use_had = use_had, A.lambda = lambda;
  A.dist = d_dist, A.cost = d_cost, A.best = d_best;
  if (wp) memcpy(A.wp, wp, sizeof(A.wp));
  launch_plain_or_wp<PeArgs>(wp != nullptr, A, [&](const auto &a) {
    hipLaunchKernelGGL(k_pred_error<std::decay_t<decltype(a)>>, dim3((unsigned)n_groups), dim3(threads), lds, c->stream, a);
  });
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
static int pred_error(hmx_ctx *c, const char *name, const hmx_pu *cands, const uint32_t *bits, int n, const uint32_t *group_first, int n_groups,
                      const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, int use_had,
                      uint32_t *d_dist, uint32_t *d_cost, hmx_pred_choice *d_best, const hmx_mc_wp *wp) {
  // the tables of this entry are per list (hmx_mc_wp) and go through wp_entry below, not through the searches' table
  if (const int r = me_call_check(c, name, !c || !cands || !refs || !org || !d_dist || !d_cost, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, nullptr,
                                  nullptr))
    return r;
  const auto nm = [name] { return std::string(name); }; // refusals only
  if (use_had != 0 && use_had != 1) return fail(c, HMX_ERR_ARG, nm() + ": use_had is 0 or 1");
  if (n_groups < 0 || (n_groups == 0) != (group_first == nullptr) || (n_groups == 0) != (d_best == nullptr))
    return fail(c, HMX_ERR_ARG, nm() + ": group_first, n_groups and d_best are given together (groups) or NULL, 0, NULL (costs only)");
  const bool weighted = wp && (wp->l0 || wp->l1);
  WpEntry wpt[4][2] = {};
  if (weighted) {
    if (!wp->l0) return fail(c, HMX_ERR_ARG, nm() + ": a weighted call needs the list 0 table (l0 NULL, l1 not)");
    const hmx_wp unit = {{1, 1, 1}, {0, 0, 0}, {0, 0, 0}, 0}; // a missing list 1 table holds the unit weight
    for (int r = 0; r < n_refs; r++)
      for (int l = 0; l < 2; l++) {
        const hmx_wp *t = l ? wp->l1 : wp->l0;
        WpDev e;
        if (!wp_entry(t ? t[r] : unit, c->cfg.bit_depth, &e))
          return fail(c, HMX_ERR_ARG, nm() + ": wp list " + std::to_string(l) + " row " + std::to_string(r) +
                                          ": weight outside -128..255, offset outside -128..127 or log2_denom > 7");
        wpt[r][l] = e.at(0);
      }
  }
  for (int i = 0; i < n; i++) {
    const hmx_pu &u = cands[i];
    auto refuse = [&](const std::string &why) { return fail(c, HMX_ERR_ARG, nm() + ": candidate " + std::to_string(i) + ": " + why); }; // text only when refused
    if (!me_size_ok(u.w) || !me_size_ok(u.h)) return refuse("width and height come from {4, 8, 12, 16, 24, 32, 48, 64}");
    if (u.ref0 == 255 && u.ref1 == 255) return refuse("no list is used");
    if (u.x + u.w > pic_w || u.y + u.h > pic_h) return refuse("the unit lies outside the picture");
    for (int l = 0; l < 2; l++) {
      const int ref = l ? u.ref1 : u.ref0, ix = (l ? u.mv1x : u.mv0x) >> 2, iy = (l ? u.mv1y : u.mv0y) >> 2;
      if (ref == 255) continue;
      if (ref >= n_refs) return refuse("reference index of list " + std::to_string(l) + " outside refs[]");
      // the tap window, whatever the fraction: columns x + ix - 3 .. x + ix + w + 3, rows likewise
      if (u.x + ix - 3 < -margin_x || u.x + ix + u.w + 4 > pic_w + margin_x || u.y + iy - 3 < -margin_y || u.y + iy + u.h + 4 > pic_h + margin_y)
        return refuse("the interpolation window of list " + std::to_string(l) + " reaches outside the reference's margins");
    }
  }
  std::vector<uint32_t> ones;
  if (!n_groups) { // costs only: groups of one
    ones.resize((size_t)n + 1);
    for (int i = 0; i <= n; i++) ones[i] = (uint32_t)i;
    group_first = ones.data();
  } else {
    if (group_first[0] != 0) return fail(c, HMX_ERR_ARG, nm() + ": group 0: group_first[0] must be 0");
    for (int g = 0; g < n_groups; g++) // the prefix first: the geometry pass below indexes cands[] with it
      if (group_first[g + 1] < group_first[g] || group_first[g + 1] > (uint32_t)n)
        return fail(c, HMX_ERR_ARG, nm() + ": group " + std::to_string(g) + ": group_first is not monotonic or passes n");
    if (group_first[n_groups] != (uint32_t)n) return fail(c, HMX_ERR_ARG, nm() + ": group " + std::to_string(n_groups - 1) + ": group_first does not end at n");
    for (int g = 0; g < n_groups; g++)
      for (uint32_t i = group_first[g] + 1; i < group_first[g + 1]; i++) {
        const hmx_pu &a = cands[group_first[g]], &b = cands[i];
        if (a.x != b.x || a.y != b.y || a.w != b.w || a.h != b.h)
          return fail(c, HMX_ERR_ARG, nm() + ": group " + std::to_string(g) + ": its candidates differ in x, y, w or h");
      }
  }
  PlanesDev dr[4] = {};
  for (int r = 0; r < n_refs; r++) dr[r] = to_dev(&refs[r]);
  return pe_launch(c, cands, bits, n, group_first, n_groups ? n_groups : n, dr, n_refs, to_dev(org), lambda, use_had, d_dist, d_cost, d_best,
                   weighted ? wpt : nullptr);
}
extern "C" int hmx_batch_inter_pred_error(hmx_ctx *c, const hmx_pu *cands, const uint32_t *bits, int n, const uint32_t *group_first, int n_groups,
                                          const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y,
                                          uint32_t lambda, int use_had, uint32_t *d_dist, uint32_t *d_cost, hmx_pred_choice *d_best) {
  return pred_error(c, "hmx_batch_inter_pred_error", cands, bits, n, group_first, n_groups, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda,
                    use_had, d_dist, d_cost, d_best, nullptr);
}
extern "C" int hmx_batch_inter_pred_error_wp(hmx_ctx *c, const hmx_pu *cands, const uint32_t *bits, int n, const uint32_t *group_first, int n_groups,
                                             const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y,
                                             uint32_t lambda, int use_had, uint32_t *d_dist, uint32_t *d_cost, hmx_pred_choice *d_best,
                                             const hmx_mc_wp *wp) {
  return pred_error(c, "hmx_batch_inter_pred_error_wp", cands, bits, n, group_first, n_groups, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda,
                    use_had, d_dist, d_cost, d_best, wp);
}
// The scalar drop-in: the tap windows of the used lists and the original go up into the context scratch, the candidate is
// re-based on them (unit at (3, 3) of each window, the vectors' fractions kept) and runs through k_pred_error as a batch of one.
extern "C" int hmx_getInterPredictionError(hmx_ctx *c, const hmx_pic *ref0, const int *mv0, const hmx_pic *ref1, const int *mv1, int x, int y, int w, int h,
                                           const hmx_pel *org, int org_stride, int use_had, const hmx_wp *wp0, const hmx_wp *wp1, uint32_t *err) {
  const std::string nm = "hmx_getInterPredictionError";
  if (!c || !org || !err || (!ref0 && !ref1) || (ref0 && !mv0) || (ref1 && !mv1)) return fail(c, HMX_ERR_ARG, nm + ": null argument, or no list is used");
  if ((ref0 && !ref0->plane[0]) || (ref1 && !ref1->plane[0])) return fail(c, HMX_ERR_ARG, nm + ": a reference has no luma plane");
  if (use_had != 0 && use_had != 1) return fail(c, HMX_ERR_ARG, nm + ": use_had is 0 or 1");
  if (!me_size_ok(w) || !me_size_ok(h)) return fail(c, HMX_ERR_ARG, nm + ": width and height come from {4, 8, 12, 16, 24, 32, 48, 64}");
  const bool weighted = wp0 || wp1;
  if (weighted && ((ref0 && !wp0) || (ref1 && !wp1))) return fail(c, HMX_ERR_ARG, nm + ": a weighted call needs the entry of every used list");
  WpEntry wpt[4][2] = {};
  for (int l = 0; l < 2 && weighted; l++) {
    WpDev e;
    if (!(l ? ref1 : ref0)) continue;
    if (!wp_entry(l ? *wp1 : *wp0, c->cfg.bit_depth, &e))
      return fail(c, HMX_ERR_ARG, nm + ": wp" + std::to_string(l) + ": weight outside -128..255, offset outside -128..127 or log2_denom > 7");
    wpt[l][l] = e.at(0);
  }
  const int ww = w + 7, wh = h + 7;
  Scratch s{c};
  uint32_t *d_out = s.take_tail<uint32_t>(2);
  short *d_org = s.take<short>((size_t)ww * wh); // the original at (3, 3) of a buffer shaped like the windows
  if (s.r) return s.r;
  HIPCHK(c, hipMemcpy2DAsync(d_org + 3 * ww + 3, ww * sizeof(short), org, (size_t)org_stride * sizeof(short), w * sizeof(short), h, hipMemcpyHostToDevice,
                             c->stream));
  hmx_pu u{};
  u.x = u.y = 3, u.w = (uint8_t)w, u.h = (uint8_t)h, u.ref0 = u.ref1 = 255;
  PlanesDev dr[4] = {}, dorg{};
  dorg.p[0] = d_org, dorg.s[0] = ww;
  for (int l = 0; l < 2; l++) {
    const hmx_pic *rp = l ? ref1 : ref0;
    const int *mv = l ? mv1 : mv0;
    if (!rp) continue;
    dr[l].p[0] = s.up(rp->plane[0] + (ptrdiff_t)(y + (mv[1] >> 2) - 3) * rp->stride[0] + (x + (mv[0] >> 2) - 3), ww, wh, rp->stride[0]);
    dr[l].s[0] = ww;
    if (s.r) return s.r;
    (l ? u.ref1 : u.ref0) = (uint8_t)l;
    (l ? u.mv1x : u.mv0x) = (int16_t)(mv[0] & 3), (l ? u.mv1y : u.mv0y) = (int16_t)(mv[1] & 3);
  }
  const uint32_t first[2] = {0, 1};
  const int r = pe_launch(c, &u, nullptr, 1, first, 1, dr, 2, dorg, 0, use_had, d_out, d_out + 1, nullptr, weighted ? wpt : nullptr);
  if (r) return r;
  HIPCHK(c, hipMemcpyAsync(err, d_out, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HMX_OK;
}
// xGetMvpIdxBits (TEncSearch.cpp:3928-3952); the reference asserts 0 <= idx < num
extern "C" uint32_t hmx_mvpIdxBits(int idx, int num) {
  if (num == 1 || idx == 0) return num == 1 ? 0 : 1;
  return 1 + (uint32_t)(idx - 1) + (num - 1 > idx ? 1 : 0);
}
// uiBitsCand of xMergeEstimation (:3133-3137)
extern "C" uint32_t hmx_mergeIdxBits(int cand, int max_signaled) { return (uint32_t)cand + 1 - (cand == max_signaled - 1 ? 1 : 0); }
// xCheckBestMVP (:4012-4055): vector bits at cost scale 0 plus m_auiMVPIdxCost[idx][AMVP_MAX_NUM_CANDS] (= xGetMvpIdxBits(idx, 2), :219-227)
extern "C" int hmx_checkBestMVP(uint32_t lambda, int mvx, int mvy, const int16_t *mvp_cands, int n_cands, int *mvp_idx, uint32_t *bits, uint32_t *cost) {
  if (!mvp_cands || !mvp_idx || !bits || !cost || n_cands < 0 || n_cands > 2 || *mvp_idx < 0 || (n_cands && *mvp_idx >= n_cands)) return HMX_ERR_ARG;
  if (n_cands < 2) return HMX_OK;
  const int cur = *mvp_idx;
  const int org_bits = (int)(hmx_mvBits(mvx, mvy, mvp_cands[2 * cur], mvp_cands[2 * cur + 1], 0) + hmx_mvpIdxBits(cur, 2));
  int best_bits = org_bits, best = cur;
  for (int i = 0; i < n_cands; i++) {
    if (i == cur) continue;
    const int b = (int)(hmx_mvBits(mvx, mvy, mvp_cands[2 * i], mvp_cands[2 * i + 1], 0) + hmx_mvpIdxBits(i, 2));
    if (b < best_bits) best_bits = b, best = i;
  }
  if (best != cur) { // UInt arithmetic, wrapping (:4051-4053)
    const uint32_t org = *bits;
    *mvp_idx = best;
    *bits = org - (uint32_t)org_bits + (uint32_t)best_bits;
    *cost = (*cost - ((lambda * org) >> 16)) + ((lambda * *bits) >> 16);
  }
  return HMX_OK;
}
