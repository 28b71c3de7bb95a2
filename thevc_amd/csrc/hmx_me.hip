// hmx_me.hip: full-search integer motion estimation (TEncSearch::xPatternSearch), SAD, vector-bits cost, search box, and the fused
// half- and quarter-sample refinement behind it (TEncSearch::xPatternSearchFracDIF) -- part of libhmx
// (include/hmx.h), gfx950.  See hmx_host.h for how the library is cut into translation units.
#include "hmx_host.h"

// =============================================================================================
// Vector cost (TComRdCost.h:185-211, TComRdCost.cpp:270-284) and search box (TEncSearch.cpp:4209-4225): host helpers
// =============================================================================================
// xGetComponentBits in closed form: the halving loop adds 2 per bit of uiTemp above the lowest
__host__ __device__ __forceinline__ uint32_t me_comp_bits(int v) {
  const uint32_t t = v <= 0 ? ((uint32_t)(-v) << 1) + 1 : (uint32_t)v << 1;
#ifdef __HIP_DEVICE_COMPILE__
  return 2u * (31u - (uint32_t)__clz((int)t)) + 1u;
#else
  return 2u * (31u - (uint32_t)__builtin_clz(t)) + 1u;
#endif
}
__host__ __device__ __forceinline__ uint32_t me_mv_bits(int x, int y, int px, int py, int sc) {
  return me_comp_bits(x * (1 << sc) - px) + me_comp_bits(y * (1 << sc) - py);
}
__host__ __device__ __forceinline__ uint32_t me_mv_cost(uint32_t lambda, int x, int y, int px, int py, int sc) {
  return (lambda * me_mv_bits(x, y, px, py, sc)) >> 16; // UInt product, wraps as the reference's
}
extern "C" uint32_t hmx_mvBits(int x, int y, int pred_x, int pred_y, int cost_scale) { return me_mv_bits(x, y, pred_x, pred_y, cost_scale); }
extern "C" uint32_t hmx_mvCost(uint32_t lambda, int x, int y, int pred_x, int pred_y, int cost_scale) {
  return me_mv_cost(lambda, x, y, pred_x, pred_y, cost_scale);
}
extern "C" void hmx_setSearchRange(int pred_x, int pred_y, int range, int cu_x, int cu_y, int pic_w, int pic_h, int ctu, int *left, int *top,
                                   int *right, int *bottom) {
  hmx_clipMv(&pred_x, &pred_y, cu_x, cu_y, pic_w, pic_h, ctu);
  int lx = pred_x - (range << 2), ty = pred_y - (range << 2), rx = pred_x + (range << 2), by = pred_y + (range << 2);
  hmx_clipMv(&lx, &ty, cu_x, cu_y, pic_w, pic_h, ctu);
  hmx_clipMv(&rx, &by, cu_x, cu_y, pic_w, pic_h, ctu);
  *left = lx >> 2, *top = ty >> 2, *right = rx >> 2, *bottom = by >> 2;
}

// =============================================================================================
// xGetSAD4 .. xGetSAD64 (TComRdCost.cpp:518-..., dispatch :298-329) of ONE block, host pointers
// =============================================================================================
__global__ void k_sad(const short *org, const short *cur, int w, int h, int step, unsigned *out) {
  const int r = (blockIdx.x * blockDim.x + threadIdx.x) * step; // one thread per row that is summed
  if (r >= h) return;
  unsigned sum = 0;
  for (int k = 0; k < w; k++) sum += (unsigned)abs(org[r * w + k] - cur[r * w + k]);
  atomicAdd(out, sum);
}
extern "C" int hmx_getSAD(hmx_ctx *c, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int sub_shift,
                          uint32_t *sad) {
  if (!c || !cur || !org || !sad) return fail(c, HMX_ERR_ARG, "hmx_getSAD: null argument");
  if (!me_size_ok(w) || !me_size_ok(h)) return fail(c, HMX_ERR_ARG, "hmx_getSAD: width and height come from {4, 8, 12, 16, 24, 32, 48, 64}");
  if (sub_shift < 0 || sub_shift > 1 || (sub_shift && h <= 8)) return fail(c, HMX_ERR_ARG, "hmx_getSAD: sub_shift is 0, or 1 with more than 8 rows");
  Scratch s{c};
  short *d_o = s.up(org, w, h, org_stride), *d_c = s.up(cur, w, h, cur_stride);
  unsigned *d_out = s.take<unsigned>(1);
  if (s.r) return s.r;
  HIPCHK(c, hipMemsetAsync(d_out, 0, 4, c->stream));
  hipLaunchKernelGGL(k_sad, dim3(1), dim3(64), 0, c->stream, d_o, d_c, w, h, 1 << sub_shift, d_out);
  HIPCHK(c, hipGetLastError());
  unsigned v = 0;
  const int r = hmx_download(c, &v, d_out, 4);
  *sad = (v << sub_shift) >> (c->cfg.bit_depth - 8);
  return r;
}

// =============================================================================================
// TComRdCostWeightPrediction::xGetSADw (TComRdCostWeightPrediction.cpp:69-104) and xGetHADsw (:490-561) of ONE block, host pointers
// =============================================================================================
// xGetHADsw read against subblock_dist (hmx_kernels.h): xCalcHADs4x4w (:204-302) and xCalcHADs8x8w (:311-423) form diff = org - pred
// with pred a Pel (the weighted sample wrapped to 16 bits), then run the butterflies of xCalcHADs4x4 / xCalcHADs8x8 unchanged and
// round per sub-block with (satd + 1) >> 1 and (sad + 2) >> 2, as the unweighted functions do; xGetHADsw picks 8x8 when both sides
// are multiples of 8, else 4x4 (:516-545), and returns uiSum >> g_uiBitIncrement (:560).  Only the difference changes.
__global__ void k_dist_w(const short *org, const short *cur, int w, int h, MeWp p, int hads, unsigned *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (!hads) { // one thread per row: every row, whatever iSubShift says
    if (i >= h) return;
    unsigned sum = 0;
    for (int k = 0; k < w; k++) sum += (unsigned)abs(org[i * w + k] - me_wp_pel(p, cur[i * w + k]));
    atomicAdd(out, sum);
    return;
  }
  const int n = (w % 8 == 0 && h % 8 == 0) ? 8 : 4, bw = w / n, nb = bw * (h / n);
  if (i >= nb) return;
  const short *o = org + (i / bw) * n * w + (i % bw) * n, *c = cur + (i / bw) * n * w + (i % bw) * n;
  int d[64];
  for (int r = 0; r < n; r++)
    for (int k = 0; k < n; k++) d[r * 8 + k] = o[r * w + k] - me_wp_pel(p, c[r * w + k]);
  atomicAdd(out, (unsigned)subblock_dist(d, n, true));
}
static int dist_w(hmx_ctx *c, const char *name, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int weight,
                  int offset, int log2_denom, int hads, uint32_t *out) {
  if (!c || !cur || !org || !out) return fail(c, HMX_ERR_ARG, std::string(name) + ": null argument");
  if (!me_size_ok(w) || !me_size_ok(h)) return fail(c, HMX_ERR_ARG, std::string(name) + ": width and height come from {4, 8, 12, 16, 24, 32, 48, 64}");
  MeWp p;
  if (!me_wp_make(weight, offset, log2_denom, 0, c->cfg.bit_depth, &p))
    return fail(c, HMX_ERR_ARG, std::string(name) + ": weight outside -128..255, offset outside -128..127 or log2_denom outside 0..7");
  Scratch s{c};
  short *d_o = s.up(org, w, h, org_stride), *d_c = s.up(cur, w, h, cur_stride);
  unsigned *d_out = s.take<unsigned>(1);
  if (s.r) return s.r;
  HIPCHK(c, hipMemsetAsync(d_out, 0, 4, c->stream));
  const int items = hads ? (w / 4) * (h / 4) : h;
  hipLaunchKernelGGL(k_dist_w, dim3((items + 63) / 64), dim3(64), 0, c->stream, d_o, d_c, w, h, p, hads, d_out);
  HIPCHK(c, hipGetLastError());
  unsigned v = 0;
  const int r = hmx_download(c, &v, d_out, 4);
  *out = v >> (c->cfg.bit_depth - 8);
  return r;
}
extern "C" int hmx_getSADw(hmx_ctx *c, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int weight,
                           int offset, int log2_denom, uint32_t *sad) {
  return dist_w(c, "hmx_getSADw", cur, cur_stride, org, org_stride, w, h, weight, offset, log2_denom, 0, sad);
}
extern "C" int hmx_getHADsw(hmx_ctx *c, const hmx_pel *cur, int cur_stride, const hmx_pel *org, int org_stride, int w, int h, int weight,
                            int offset, int log2_denom, uint32_t *satd) {
  return dist_w(c, "hmx_getHADsw", cur, cur_stride, org, org_stride, w, h, weight, offset, log2_denom, 1, satd);
}

// =============================================================================================
// xPatternSearch (TEncSearch.cpp:4227-4283) over unit lists
// =============================================================================================
// One workgroup (two waves) = one unit and one tile of 32 x 32 candidates of its box.  The unit's original block and the
// (w + 31) x (h + 31) reference window of the tile are staged in LDS once, both with 2^B added, so that the original --
// which may be 2 * org - other prediction, negative or above the sample range -- and the reference are unsigned 16-bit values
// with the differences unchanged: v_sad_u16 then sums two absolute differences and the accumulator per instruction.
// A lane owns EIGHT candidates of one candidate row: x = 16 * half + p + 2 * j, j = 0..7 (p: parity, half: left or right 16
// candidates; four lanes a row, sixteen rows a wave).  Per original row it reads its stretch of the window row once with
// 16-byte LDS reads -- the stretch starts on a dword for every lane -- and brings it to its parity with one v_alignbit per
// dword (shift 0 or 16), so all eight candidates, whose first samples are whole dwords apart, read their sample pairs from
// registers: per eight samples one window read, one (broadcast) read of the original and 4 alignbit feed 32 v_sad_u16.
// Window rows are kMeWinPitch samples = 12 sixteen-byte slots apart: the sixteen lanes of a 16-byte read's lane group
// (MI355X: four groups of sixteen) then fall on different slots.
// ARGS::weighted (MeArgsWp, uniform over a launch): weighted distortion, xGetSADw (TComRdCostWeightPrediction.cpp:69-104).  The window is weighted ONCE
// while it is staged -- pred = me_wp_pel(entry of the unit's reference, sample) -- and the loop over rows is the unweighted one.
// The bias: pred is any int16, [-2^15, 2^15), and the original lies in [-2^B, 2^(B+1)); with 2^15 added both are in [0, 2^16) as
// long as 2^(B+1) + 2^15 <= 2^16, i.e. B <= 14, so they stay unsigned 16-bit values with the differences unchanged (2^B, the
// unweighted bias, would leave a negative pred negative).  xGetSADw ignores iSubShift: every row is read, nothing is shifted left.
constexpr int kMeTile = 32, kMeWinPitch = 96, kMeWinRows = 64 + kMeTile - 1, kMeThreads = 128;
struct MeArgs {
  const hmx_me_unit *units;
  const uint32_t *tile_first; // [n + 1] prefix of tiles per unit
  const uint32_t *map_first;  // [n + 1] prefix of box areas (the host refuses a call whose sum does not fit 32 bits)
  int n;
  PlanesDev refs[4];
  PlanesDev org;
  int B;
  uint32_t lambda;
  unsigned long long *keys; // [n]: (cost << 32) | raster index in the box, all ones before the launch
  uint32_t *cost_map;       // NULL = none
  static constexpr bool weighted = false;
};
// The weighted launch's arguments.  The kernels below are templates over their argument type, so that the unweighted
// instantiation has the argument block, and with it the code, it had before the weighted one existed.
struct MeArgsWp : MeArgs {
  MeWp wp[4]; // the luma entry of refs[k]
  static constexpr bool weighted = true;
};
typedef unsigned u4v __attribute__((ext_vector_type(4)));

template <int W>
__device__ __forceinline__ void me_rows(const u4v *win, const u4v *org, int h, int step, unsigned sh, unsigned (&acc)[8]) {
  constexpr int ND = (W / 2 + 8 + 3) / 4 * 4, OD = (W / 2 + 3) / 4 * 4; // dwords read per window row / original row
  for (int r = 0; r < h; r += step) {
    unsigned d[ND], o[OD];
#pragma unroll
    for (int k = 0; k < ND / 4; k++) {
      const u4v v = win[r * (kMeWinPitch / 8) + k];
      d[4 * k] = v.x, d[4 * k + 1] = v.y, d[4 * k + 2] = v.z, d[4 * k + 3] = v.w;
    }
#pragma unroll
    for (int k = 0; k < OD / 4; k++) {
      const u4v v = org[r * (OD / 4) + k];
      o[4 * k] = v.x, o[4 * k + 1] = v.y, o[4 * k + 2] = v.z, o[4 * k + 3] = v.w;
    }
    unsigned e[W / 2 + 7];
#pragma unroll
    for (int i = 0; i < W / 2 + 7; i++) e[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], sh);
#pragma unroll
    for (int i = 0; i < W / 2; i++)
#pragma unroll
      for (int j = 0; j < 8; j++) acc[j] = __builtin_amdgcn_sad_u16(e[i + j], o[i], acc[j]);
  }
}

template <class ARGS>
__global__ __launch_bounds__(kMeThreads) void k_me_search(ARGS A) {
  __shared__ __attribute__((aligned(16))) unsigned short s_win[kMeWinRows * kMeWinPitch];
  __shared__ __attribute__((aligned(16))) unsigned short s_org[64 * 64];
  __shared__ unsigned long long s_key[kMeThreads / 64];
  const uint32_t wg = blockIdx.x;
  int lo = 0, hi = A.n; // the unit this tile belongs to
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (A.tile_first[mid] <= wg) lo = mid;
    else hi = mid;
  }
  const hmx_me_unit u = A.units[lo];
  const int w = u.w, h = u.h, bw = u.right - u.left + 1, bh = u.bottom - u.top + 1, tiles_x = (bw + kMeTile - 1) / kMeTile;
  const int t = (int)(wg - A.tile_first[lo]), tx0 = (t % tiles_x) * kMeTile, ty0 = (t / tiles_x) * kMeTile;
  const int nx = min(kMeTile, bw - tx0), ny = min(kMeTile, bh - ty0); // candidates of this tile
  const int tid = threadIdx.x, bias = ARGS::weighted ? 32768 : 1 << A.B;
  typedef __attribute__((address_space(1))) const short gpel;
  { // the window: rows and columns no candidate of the tile reaches are zero and never read from memory
    const PlanesDev &R = A.refs[u.ref < 4 ? u.ref : 0];
    const gpel *src = (const gpel *)R.p[0] + (ptrdiff_t)(u.y + u.top + ty0) * R.s[0] + (u.x + u.left + tx0);
    const int vx = nx + w - 1, vy = ny + h - 1, cols = min(kMeWinPitch, w + 40), rows = h + kMeTile - 1;
    for (int wy = tid >> 5; wy < rows; wy += kMeThreads / 32)
      for (int wx = tid & 31; wx < cols; wx += 32)
        if constexpr (ARGS::weighted)
          s_win[wy * kMeWinPitch + wx] =
              (wx < vx && wy < vy) ? (unsigned short)(me_wp_pel(A.wp[u.ref < 4 ? u.ref : 0], src[(ptrdiff_t)wy * R.s[0] + wx]) + bias) : (unsigned short)0;
        else s_win[wy * kMeWinPitch + wx] = (wx < vx && wy < vy) ? (unsigned short)(src[(ptrdiff_t)wy * R.s[0] + wx] + bias) : (unsigned short)0;
  }
  const int op = ((w / 2 + 3) / 4 * 4) * 2; // samples per staged original row
  {
    const gpel *src = (const gpel *)A.org.p[0] + (size_t)u.y * A.org.s[0] + u.x;
    for (int ry = tid >> 5; ry < h; ry += kMeThreads / 32)
      for (int rx = tid & 31; rx < op; rx += 32) s_org[ry * op + rx] = rx < w ? (unsigned short)(src[(size_t)ry * A.org.s[0] + rx] + bias) : (unsigned short)0;
  }
  __syncthreads();
  const int row = tid >> 2, half = (tid >> 1) & 1, p = tid & 1;
  unsigned acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const u4v *win = reinterpret_cast<const u4v *>(s_win + row * kMeWinPitch + 16 * half), *org = reinterpret_cast<const u4v *>(s_org);
  const int step = 1 << (ARGS::weighted ? 0 : u.sub_shift);
  const unsigned sh = p ? 16u : 0u;
  // a wave holds sixteen candidate rows: one whose rows all lie below the tile's last candidate row (the fifth tile row of a 129-high
  // box has one, a +-1 box three) sums nothing -- uniform over the wave; its lanes keep acc = 0 and are masked out below
  if ((tid >> 6) * 16 < ny) {
    switch (w) { // uniform over the workgroup
    case 4: me_rows<4>(win, org, h, step, sh, acc); break;
    case 8: me_rows<8>(win, org, h, step, sh, acc); break;
    case 12: me_rows<12>(win, org, h, step, sh, acc); break;
    case 16: me_rows<16>(win, org, h, step, sh, acc); break;
    case 24: me_rows<24>(win, org, h, step, sh, acc); break;
    case 32: me_rows<32>(win, org, h, step, sh, acc); break;
    case 48: me_rows<48>(win, org, h, step, sh, acc); break;
    default: me_rows<64>(win, org, h, step, sh, acc); break;
    }
  }
  // cost = SAD + getCost(x, y) at cost scale 2 (TEncSearch.cpp:4172, :4268); first minimum in raster order = minimum of
  // (cost, raster index)
  unsigned long long best = ~0ull;
  typedef __attribute__((address_space(1))) uint32_t gu32;
  gu32 *map = A.cost_map ? (gu32 *)A.cost_map + A.map_first[lo] : nullptr;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int cx = 16 * half + p + 2 * j;
    if (cx < nx && row < ny) {
      const int bx = tx0 + cx, by = ty0 + row;
      const uint32_t sad = (acc[j] << (ARGS::weighted ? 0 : u.sub_shift)) >> (A.B - 8);
      const uint32_t cost = sad + me_mv_cost(A.lambda, u.left + bx, u.top + by, u.pred_x, u.pred_y, 2);
      const uint32_t idx = (uint32_t)(by * bw + bx);
      if (map) map[idx] = cost;
      const unsigned long long key = ((unsigned long long)cost << 32) | idx;
      best = key < best ? key : best;
    }
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long other = __shfl_xor(best, m, 64);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) s_key[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) atomicMin(&A.keys[lo], s_key[1] < s_key[0] ? s_key[1] : s_key[0]);
}

__global__ void k_me_unpack(const hmx_me_unit *units, const unsigned long long *keys, int n, uint32_t lambda, hmx_me_result *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const hmx_me_unit u = units[i];
  const unsigned long long key = keys[i];
  const int bw = u.right - u.left + 1, idx = (int)(uint32_t)key;
  const int x = u.left + idx % bw, y = u.top + idx / bw;
  const uint32_t cost = (uint32_t)(key >> 32);
  hmx_me_result r;
  r.mvx = (int16_t)x, r.mvy = (int16_t)y;
  r.cost = cost;
  r.sad = cost - me_mv_cost(lambda, x, y, u.pred_x, u.pred_y, 2); // ruiSAD (:4281)
  out[i] = r;
}

// the four searches' entries: `name` is the entry the caller used (refusals are made under it), wp == NULL the unweighted call
static int me_fullpel(hmx_ctx *c, const char *name, const hmx_me_unit *units, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w,
                      int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result, uint32_t *d_cost_map, const hmx_wp *wp) {
  MeWp wpt[4] = {};
  if (const int r = me_call_check(c, name, !c || !units || !refs || !org || !d_result, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, wp, wpt)) return r;
  std::vector<uint32_t> tile_first((size_t)n + 1, 0), map_first((size_t)n + 1, 0);
  uint64_t area = 0; // the kernel's offsets into the cost map are 32-bit
  for (int i = 0; i < n; i++) {
    const hmx_me_unit &u = units[i];
    const char *why = me_unit_check(u, n_refs, pic_w, pic_h, true);
    if (!why && !me_reach_ok(u, u.left, u.top, u.right, u.bottom, pic_w, pic_h, margin_x, margin_y))
      why = "a candidate block reaches outside the reference's margins";
    if (why) return me_unit_refuse(c, name, i, why);
    const int bw = u.right - u.left + 1, bh = u.bottom - u.top + 1;
    tile_first[i + 1] = tile_first[i] + (uint32_t)(((bw + kMeTile - 1) / kMeTile) * ((bh + kMeTile - 1) / kMeTile));
    map_first[i + 1] = map_first[i] + (uint32_t)(bw * bh);
    area += (uint64_t)(bw * bh);
  }
  if (area > 0xffffffffull) return fail(c, HMX_ERR_ARG, std::string(name) + ": the boxes hold more than 2^32 - 1 candidates: split the call");
  // unit list and prefixes through the argument arena (the caller's host array, and tables made from it): the three are reserved
  // together, so a list they do not fit is refused here, before the key buffer grows and before anything is copied
  const size_t unit_bytes = sizeof(hmx_me_unit) * (size_t)n, prefix_bytes = sizeof(uint32_t) * ((size_t)n + 1);
  if (const int r = arena_reserve(c, {unit_bytes, prefix_bytes, prefix_bytes}, "argument arena (unit list too long: split the call)")) return r;
  void *keys = c->d_me_keys;
  const int gr = grow_dev(c, &keys, &c->me_keys_cap, sizeof(unsigned long long) * (size_t)n, "motion search keys");
  c->d_me_keys = static_cast<unsigned long long *>(keys);
  if (gr) return gr;
  MeArgsWp A{};
  A.units = static_cast<const hmx_me_unit *>(arena_place(c, units, unit_bytes));
  A.tile_first = static_cast<const uint32_t *>(arena_place(c, tile_first.data(), prefix_bytes));
  A.map_first = static_cast<const uint32_t *>(arena_place(c, map_first.data(), prefix_bytes));
  if (!A.units || !A.tile_first || !A.map_first) return fail(c, HMX_ERR_INTERNAL, kArenaOutside);
  A.n = n;
  A.lambda = lambda;
  A.keys = c->d_me_keys;
  A.cost_map = d_cost_map;
  HIPCHK(c, hipMemsetAsync(c->d_me_keys, 0xff, sizeof(unsigned long long) * (size_t)n, c->stream));
  me_launch<MeArgs>(c, A, refs, n_refs, org, wp != nullptr, wpt, [&](const auto &a) {
    hipLaunchKernelGGL(k_me_search<std::decay_t<decltype(a)>>, dim3(tile_first[n]), dim3(kMeThreads), 0, c->stream, a);
  });
  hipLaunchKernelGGL(k_me_unpack, dim3((n + 255) / 256), dim3(256), 0, c->stream, A.units, (const unsigned long long *)c->d_me_keys, n, lambda, d_result);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_batch_fullpel_search(hmx_ctx *c, const hmx_me_unit *units, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w,
                                        int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result, uint32_t *d_cost_map) {
  return me_fullpel(c, "hmx_batch_fullpel_search", units, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda, d_result, d_cost_map, nullptr);
}
extern "C" int hmx_batch_fullpel_search_wp(hmx_ctx *c, const hmx_me_unit *units, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org,
                                           int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result,
                                           uint32_t *d_cost_map, const hmx_wp *wp) {
  return me_fullpel(c, "hmx_batch_fullpel_search_wp", units, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda, d_result, d_cost_map, wp);
}

// =============================================================================================
// xPatternSearchFracDIF (TEncSearch.cpp:4476-4514) over unit lists: both stages and both decisions in one launch
// =============================================================================================
// One workgroup (four waves) = one unit.  The (w + 8) x (h + 8) reference window around the integer-displaced block and the
// original block are staged in LDS once; the integer vector is device data, so a unit whose vector lies outside the box the
// host checked is answered with the all-ones sentinel before any reference sample is read.  The horizontal 8-tap stage
// (filterHorLuma, isLast = false) is run once per phase into a 14-bit plane in LDS and shared by every candidate that uses it:
// phase 2 for the half stage (columns -1 .. w - 1, all h + 8 rows), phases 1 and 3 once the half-sample winner (hx, hy) is
// known (w columns from the one column offset and only the rows the nine quarter candidates reach); phase 0 is a shift of the
// window and has no plane.  A candidate's distortion is then vertical taps over a plane: S lanes (S = 8, or 4 when a side is
// not a multiple of 8) share one S x S sub-block of one candidate, a lane owning a column -- S + 7 intermediates, S
// differences; the Hadamard sum runs down the column in registers and across the S lanes by lane exchange -- and the
// sub-block sums meet in LDS counters (integer adds: the order does not matter).  Wave 0 adds the vector cost and takes the
// minimum of (cost, table index) -- the tables of the two stages differ, so the index is the table's, never a raster
// position -- and writes costs and result with plain stores.  The zero-fraction vertical step (filterCopy, isLast) runs as the
// general step with the taps {0, 0, 0, 64, 0, 0, 0, 0} (interp_stage, hmx_kernels.h).
// LDS (dynamic, sized for the largest unit of the call): window, original, planes 2, 1, 3 = 46352 bytes at 64 x 64: three
// workgroups = twelve waves per CU (160 KB); 1440 bytes at 8 x 8, where the registers (eight workgroups per CU) bind first.
// WP (uniform over a launch): weighted distortion, xGetSADw / xGetHADsw (TComRdCostWeightPrediction.cpp:69-104, :490-561): the
// difference is org - me_wp_pel(entry, final clipped sample), what the reference forms from its m_filteredBlock planes; the
// interpolation, the sub-block rule and the per-sub-block rounding do not change.
constexpr int kSpThreads = 256;
struct SpArgs {
  const hmx_me_unit *units;
  const hmx_me_result *ints; // device: the integer vectors
  PlanesDev refs[4];
  PlanesDev org;
  int B, use_had;
  uint32_t lambda;
  hmx_subpel_result *result;
  uint32_t *stage_cost; // [n][18], NULL = none
  static constexpr bool weighted = false;
};
struct SpArgsWp : SpArgs { // as MeArgsWp
  MeWp wp[4];
  static constexpr bool weighted = true;
};
static size_t sp_lds_bytes(int w, int h) { return sizeof(short) * (size_t)((w + 8) * (h + 8) + w * h + (w + 1) * (h + 8) + 2 * w * (h + 8)); }
struct SpDiv { // n / d for n < 4096 * d and n * d < 2^20, by one multiplication
  unsigned d, m;
  __device__ __forceinline__ explicit SpDiv(int dd) : d((unsigned)dd), m(((1u << 20) + (unsigned)dd - 1) / (unsigned)dd) {}
  __device__ __forceinline__ int div(int n) const { return (int)(((unsigned)n * m) >> 20); }
};
__host__ __device__ constexpr unsigned sp_tap_word(int frac, int half) { // four taps as signed bytes
  return ((unsigned)luma_tap(frac, 4 * half) & 255u) | (((unsigned)luma_tap(frac, 4 * half + 1) & 255u) << 8) |
         (((unsigned)luma_tap(frac, 4 * half + 2) & 255u) << 16) | (((unsigned)luma_tap(frac, 4 * half + 3) & 255u) << 24);
}
// s_acMvRefineH / s_acMvRefineQ (TEncSearch.cpp:47-71), component + 1 in two bits per entry; the x components agree
__host__ __device__ constexpr unsigned sp_pack9(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7, int a8) {
  return (unsigned)(a0 + 1) | (unsigned)(a1 + 1) << 2 | (unsigned)(a2 + 1) << 4 | (unsigned)(a3 + 1) << 6 | (unsigned)(a4 + 1) << 8 |
         (unsigned)(a5 + 1) << 10 | (unsigned)(a6 + 1) << 12 | (unsigned)(a7 + 1) << 14 | (unsigned)(a8 + 1) << 16;
}
constexpr unsigned kSpCandX = sp_pack9(0, 0, 0, -1, 1, -1, 1, -1, 1);
constexpr unsigned kSpCandYH = sp_pack9(0, -1, 1, 0, 0, -1, -1, 1, 1), kSpCandYQ = sp_pack9(0, -1, 1, -1, -1, 0, 0, 1, 1);
__device__ __forceinline__ void sp_cand(int stage, int k, int &dx, int &dy) {
  dx = (int)((kSpCandX >> (2 * k)) & 3u) - 1;
  dy = (int)(((stage ? kSpCandYQ : kSpCandYH) >> (2 * k)) & 3u) - 1;
}

// filterHorLuma(frac, isLast = false) of plane rows r0 .. r1 - 1 (row r = window row r) and `cols` columns, column c at window
// column wc0 + c, into dst (pitch dp)
template <int FRAC>
__device__ __forceinline__ void sp_hor_plane(const short *win, int wp, short *dst, int dp, int cols, int wc0, int r0, int r1, int B, int tid) {
  const LumaFilter f = luma_filter(FRAC, true, false, B); // the taps fold to constants
  const int n = (r1 - r0) * cols;
  const SpDiv dc(cols);
  for (int i = tid; i < n; i += kSpThreads) {
    const int r = dc.div(i), c = i - r * cols;
    const short *s = win + (r0 + r) * wp + wc0 + c - 3;
    int row[8];
#pragma unroll
    for (int q = 0; q < 8; q++) row[q] = s[q];
    dst[(r0 + r) * dp + c] = (short)luma_sample(f, row);
  }
}

struct SpLds {
  const short *win, *org, *p1, *p2, *p3;
  int w, h;
};
// the nine candidates of one stage: s_cost[k] += the sub-block sums of candidate k
template <int S, bool WP>
__device__ __forceinline__ void sp_stage(const SpLds &L, int stage, int hx, int hy, int c1, int c3, int B, int use_had, const MeWp *wp, unsigned *s_cost,
                                         int tid) {
  const int w = L.w, bw = w / S, nsb = bw * (L.h / S), lane = tid & (S - 1);
  const SpDiv dn(nsb), db(bw);
  const int head = 14 - B;
  LumaFilter f{{}, interp_stage(false, true, B)}; // filterVerLuma(isFirst = false, isLast = true); the taps are the item's
  subblock_walk<S>(9 * nsb, tid, kSpThreads, [&](int g, bool act) { // an item: one sub-block of one candidate
    const int k = dn.div(g), sb = g - k * nsb, sby = db.div(sb), sx = (sb - sby * bw) * S, sy = sby * S;
    int dx, dy;
    sp_cand(stage, k, dx, dy);
    const int ox = stage ? 2 * hx + dx : 2 * dx, oy = stage ? 2 * hy + dy : 2 * dy; // quarter samples from the integer vector
    const int xf = ox & 3, cx = ox >> 2, yf = oy & 3, iy = oy >> 2;
    const int rb = sy + iy + 1, col = sx + lane + cx; // plane row of the first intermediate: sample row sy + iy - 3
    const short *src;
    int pitch;
    if (xf == 0) src = L.win + rb * (w + 8) + col + 4, pitch = w + 8;
    else if (xf == 2) src = L.p2 + rb * (w + 1) + col + 1, pitch = w + 1;
    else if (xf == 1) src = L.p1 + rb * w + col - c1, pitch = w;
    else src = L.p3 + rb * w + col - c3, pitch = w;
    int t[S + 7];
#pragma unroll
    for (int q = 0; q < S + 7; q++) {
      const int v = src[q * pitch];
      t[q] = xf == 0 ? (v << head) - 8192 : v; // filterCopy, isFirst (:112-122)
    }
    unsigned tw[2];
    tw[0] = yf == 0 ? sp_tap_word(0, 0) : yf == 1 ? sp_tap_word(1, 0) : yf == 2 ? sp_tap_word(2, 0) : sp_tap_word(3, 0);
    tw[1] = yf == 0 ? sp_tap_word(0, 1) : yf == 1 ? sp_tap_word(1, 1) : yf == 2 ? sp_tap_word(2, 1) : sp_tap_word(3, 1);
#pragma unroll
    for (int q = 0; q < 8; q++) f.tap[q] = (int)(signed char)(tw[q >> 2] >> (8 * (q & 3)));
    int d[S];
    luma_column<S>(f, t, d);
    if constexpr (WP) {
#pragma unroll
      for (int r = 0; r < S; r++) d[r] = me_wp_pel(*wp, d[r]);
    }
    column_cost<S>(d, L.org + sy * w + sx + lane, w, lane, use_had, act, &s_cost[k]);
  });
}

// xPatternRefinement's loop (:725-757) over the nine costs of a stage, by the first 16 lanes of wave 0: the costs to the
// caller's array, and the winner's table index with its cost (every lane of the 16 returns them)
__device__ __forceinline__ unsigned long long sp_decide(const unsigned *s_cost, int stage, int bx, int by, const hmx_me_unit &u, const SpArgs &A,
                                                        uint32_t *costs, int tid) {
  unsigned long long key = ~0ull;
  if (tid < 9) {
    int dx, dy;
    sp_cand(stage, tid, dx, dy);
    const uint32_t cost = (s_cost[tid] >> (A.B - 8)) + me_mv_cost(A.lambda, bx + dx, by + dy, u.pred_x, u.pred_y, stage ? 0 : 1);
    if (costs) costs[tid] = cost;
    key = ((unsigned long long)cost << 32) | (unsigned)tid;
  }
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) {
    const unsigned long long other = __shfl_xor(key, m, 64);
    key = other < key ? other : key;
  }
  return key;
}

template <class ARGS>
__global__ __launch_bounds__(kSpThreads) void k_subpel_search(ARGS A) {
  constexpr bool WP = ARGS::weighted;
  extern __shared__ __attribute__((aligned(16))) short s_sp[];
  __shared__ unsigned s_cost[18];
  __shared__ int s_half;
  const int i = blockIdx.x, tid = threadIdx.x;
  const hmx_me_unit u = A.units[i];
  const int ix = A.ints[i].mvx, iy = A.ints[i].mvy, w = u.w, h = u.h, B = A.B;
  typedef __attribute__((address_space(1))) uint32_t gu32;
  gu32 *costs = A.stage_cost ? (gu32 *)A.stage_cost + (size_t)i * 18 : nullptr;
  if (ix < u.left || ix > u.right || iy < u.top || iy > u.bottom) { // uniform over the workgroup: nothing was checked for this vector
    if (tid < 18 && costs) costs[tid] = 0xffffffffu;
    if (tid == 0) {
      hmx_subpel_result r;
      r.mvx = (int16_t)(4 * ix), r.mvy = (int16_t)(4 * iy), r.dist = r.cost = 0xffffffffu;
      A.result[i] = r;
    }
    return;
  }
  const int wp = w + 8, rows = h + 8;
  short *win = s_sp, *org = win + wp * rows, *p2 = org + w * h, *p1 = p2 + (w + 1) * rows, *p3 = p1 + w * rows;
  typedef __attribute__((address_space(1))) const short gpel;
  {
    const PlanesDev &R = A.refs[u.ref < 4 ? u.ref : 0];
    const gpel *src = (const gpel *)R.p[0] + (ptrdiff_t)(u.y + iy - 4) * R.s[0] + (u.x + ix - 4);
    const SpDiv dc(wp);
    for (int k = tid; k < wp * rows; k += kSpThreads) {
      const int r = dc.div(k), c = k - r * wp;
      win[k] = src[(ptrdiff_t)r * R.s[0] + c];
    }
    const gpel *so = (const gpel *)A.org.p[0] + (size_t)u.y * A.org.s[0] + u.x;
    const SpDiv dw(w);
    for (int k = tid; k < w * h; k += kSpThreads) {
      const int r = dw.div(k), c = k - r * w;
      org[k] = so[(size_t)r * A.org.s[0] + c];
    }
  }
  if (tid < 18) s_cost[tid] = 0;
  __syncthreads();
  sp_hor_plane<2>(win, wp, p2, w + 1, w + 1, 3, 0, rows, B, tid); // column c = sample column c - 1
  __syncthreads();
  const bool s8 = (w % 8 == 0) && (h % 8 == 0);
  SpLds L{win, org, p1, p2, p3, w, h};
  const MeWp *wpe = nullptr; // the unit's entry, WP only
  if constexpr (WP) wpe = &A.wp[u.ref < 4 ? u.ref : 0];
  if (s8) sp_stage<8, WP>(L, 0, 0, 0, 0, 0, B, A.use_had, wpe, s_cost, tid);
  else sp_stage<4, WP>(L, 0, 0, 0, 0, 0, B, A.use_had, wpe, s_cost, tid);
  __syncthreads();
  if (tid < 16) {
    const int kb = (int)(uint32_t)sp_decide(s_cost, 0, 2 * ix, 2 * iy, u, A, (uint32_t *)costs, tid);
    if (tid == 0) s_half = kb;
  }
  __syncthreads();
  int hx, hy;
  sp_cand(0, s_half, hx, hy);
  // the quarter stage's columns: phase 1 is reached at +1 (hx = 0, 1: sample column 0) or -3 (hx = -1: column -1), phase 3 at
  // -1 (hx = 0, -1: column -1) or +3 (hx = 1: column 0); its rows: all but the last below hy = -1, all but the first above hy = 1
  const int c1 = hx < 0 ? -1 : 0, c3 = hx > 0 ? 0 : -1, r0 = hy > 0 ? 1 : 0, r1 = hy < 0 ? rows - 1 : rows;
  sp_hor_plane<1>(win, wp, p1, w, w, 4 + c1, r0, r1, B, tid);
  sp_hor_plane<3>(win, wp, p3, w, w, 4 + c3, r0, r1, B, tid);
  __syncthreads();
  if (s8) sp_stage<8, WP>(L, 1, hx, hy, c1, c3, B, A.use_had, wpe, s_cost + 9, tid);
  else sp_stage<4, WP>(L, 1, hx, hy, c1, c3, B, A.use_had, wpe, s_cost + 9, tid);
  __syncthreads();
  if (tid < 16) {
    const int bx = 4 * ix + 2 * hx, by = 4 * iy + 2 * hy;
    const unsigned long long key = sp_decide(s_cost + 9, 1, bx, by, u, A, costs ? (uint32_t *)(costs + 9) : nullptr, tid);
    if (tid == 0) {
      int qx, qy;
      sp_cand(1, (int)(uint32_t)key, qx, qy);
      hmx_subpel_result r;
      r.mvx = (int16_t)(bx + qx), r.mvy = (int16_t)(by + qy);
      r.cost = (uint32_t)(key >> 32);
      r.dist = r.cost - me_mv_cost(A.lambda, bx + qx, by + qy, u.pred_x, u.pred_y, 0);
      A.result[i] = r;
    }
  }
}

static int me_subpel(hmx_ctx *c, const char *name, const hmx_me_unit *units, int n, const hmx_me_result *d_int, const hmx_pic *refs, int n_refs,
                     const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, int use_had,
                     hmx_subpel_result *d_result, uint32_t *d_stage_cost, const hmx_wp *wp) {
  MeWp wpt[4] = {};
  if (const int r = me_call_check(c, name, !c || !units || !d_int || !refs || !org || !d_result, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, wp, wpt))
    return r;
  if (use_had != 0 && use_had != 1) return fail(c, HMX_ERR_ARG, std::string(name) + ": use_had is 0 or 1");
  size_t lds = 0;
  for (int i = 0; i < n; i++) {
    const hmx_me_unit &u = units[i];
    const char *why = me_unit_check(u, n_refs, pic_w, pic_h, false);
    // the window of every integer vector of the box: columns x + left - 4 .. x + right + w + 3, rows likewise
    if (!why && !me_reach_ok(u, u.left - 4, u.top - 4, u.right + 4, u.bottom + 4, pic_w, pic_h, margin_x, margin_y))
      why = "the interpolation window of a vector of the box reaches outside the reference's margins";
    if (why) return me_unit_refuse(c, name, i, why);
    lds = std::max(lds, sp_lds_bytes(u.w, u.h));
  }
  SpArgsWp A{};
  A.units = static_cast<const hmx_me_unit *>(arena_push(c, units, sizeof(hmx_me_unit) * (size_t)n)); // the caller's host array
  if (!A.units) return fail(c, HMX_ERR_NOMEM, "argument arena (unit list too long: split the call)");
  A.ints = d_int;
  A.use_had = use_had;
  A.lambda = lambda;
  A.result = d_result;
  A.stage_cost = d_stage_cost;
  me_launch<SpArgs>(c, A, refs, n_refs, org, wp != nullptr, wpt, [&](const auto &a) {
    hipLaunchKernelGGL(k_subpel_search<std::decay_t<decltype(a)>>, dim3((unsigned)n), dim3(kSpThreads), lds, c->stream, a);
  });
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_batch_subpel_search(hmx_ctx *c, const hmx_me_unit *units, int n, const hmx_me_result *d_int, const hmx_pic *refs, int n_refs,
                                       const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, int use_had,
                                       hmx_subpel_result *d_result, uint32_t *d_stage_cost) {
  return me_subpel(c, "hmx_batch_subpel_search", units, n, d_int, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda, use_had, d_result,
                   d_stage_cost, nullptr);
}
extern "C" int hmx_batch_subpel_search_wp(hmx_ctx *c, const hmx_me_unit *units, int n, const hmx_me_result *d_int, const hmx_pic *refs, int n_refs,
                                          const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, int use_had,
                                          hmx_subpel_result *d_result, uint32_t *d_stage_cost, const hmx_wp *wp) {
  return me_subpel(c, "hmx_batch_subpel_search_wp", units, n, d_int, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda, use_had, d_result,
                   d_stage_cost, wp);
}

// =============================================================================================
// xTZSearch (TEncSearch.cpp:4302-4474) over unit lists: one wave owns one unit from its start point to its result
// =============================================================================================
// One workgroup = one wave = one unit, so the walk's state (uiBestSad, iBestX / iBestY, uiBestDistance, uiBestRound, ucPointNr,
// the evaluation count) is the same in all 64 lanes by construction and lives in scalar registers; there is no barrier between
// waves and nothing shared between units.  The original block is staged in LDS once with 2^B added (as k_me_search stages it:
// v_sad_u16 then serves originals in [-2^B, 2^(B+1))).  The candidates of one pattern are independent of the state -- their
// centre is fixed before the pattern starts -- so they are costed side by side: a pattern of P points gives each point 64 / P'
// lanes (P' = 2, 4, 8 or 16: start point + zero vector and the 2-point search, the 4-, 8- and 16-point diamonds; the raster grid
// goes through in chunks of 16), which share the block's (row, four-sample segment) items, sum with v_sad_u16 and meet by lane
// exchange.  The costs are then folded into the state in the reference's order with its strict <: the minimum of (cost, lane)
// over the evaluated points IS that fold, since the points sit in the lanes in evaluation order.  The reference is read
// straight from global memory in aligned 32-bit words brought to the candidate's parity with v_alignbit; every word read holds
// at least one sample of the candidate block, so nothing outside the rectangle the host checked (rounded to words) is touched.
// xTZ8PointDiamondSearch's "whole pattern inside" fast paths and its border paths evaluate the surviving points in the same
// order, and every border test of the diamonds and of xTZ2PointSearch is one rule: a coordinate that moves away from the centre
// is tested against the side it moves towards.  So a pattern here is a table of (offset, point number, distance) and that rule.
// Every loop is bounded in sight: iDist doubles up to range <= 64, the raster grid has at most 26 x 26 points, passes <= cap.
// WP (uniform over a launch): weighted distortion, xGetSADw.  Each sample pair is weighted after the load (me_wp_pel) and both the
// prediction and the original carry a bias of 2^15, not 2^B: pred is any int16 and the original lies in [-2^B, 2^(B+1)), so for
// B <= 14 both are unsigned 16-bit values with the differences unchanged (see k_me_search).  xGetSADw ignores the iSubShift that
// xTZSearchHelp sets under FEN (TEncSearch.cpp:324-330): every row is read and the sum is not shifted left.
struct TzArgs {
  const hmx_me_unit *units;
  const hmx_tz_unit *tz;
  PlanesDev refs[4];
  PlanesDev org;
  int B, max_passes;
  uint32_t lambda;
  hmx_me_result *result;
  hmx_tz_point *trace; // NULL = none
  uint32_t *trace_count;
  int trace_cap;
  static constexpr bool weighted = false;
};
struct TzArgsWp : TzArgs { // as MeArgsWp
  MeWp wp[4];
  static constexpr bool weighted = true;
};
struct TzState {
  uint32_t best;                // uiBestSad
  int bx, by, dist, round, nr;  // iBestX, iBestY, uiBestDistance, uiBestRound, ucPointNr
  uint32_t count;               // xTZSearchHelp calls so far
};
struct TzUnit {
  const __attribute__((address_space(1))) short *ref; // the sample the zero vector points at
  ptrdiff_t stride;
  const unsigned short *org; // LDS, w samples a row, biased
  int w, h, sub_shift, B, left, top, right, bottom, pred_x, pred_y;
  uint32_t lambda;
  __attribute__((address_space(1))) uint32_t *trace; // this unit's slice of hmx_tz_point as word pairs {x | y << 16, cost}, or NULL
  uint32_t trace_cap;
};
struct TzUnitWp : TzUnit {
  MeWp wp; // the unit's entry
};
// 16 entries of 2 bits: component + 1
__host__ __device__ constexpr unsigned tz_pack(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7, int a8 = 0, int a9 = 0, int a10 = 0,
                                               int a11 = 0, int a12 = 0, int a13 = 0, int a14 = 0, int a15 = 0) {
  return (unsigned)(a0 + 1) | (unsigned)(a1 + 1) << 2 | (unsigned)(a2 + 1) << 4 | (unsigned)(a3 + 1) << 6 | (unsigned)(a4 + 1) << 8 |
         (unsigned)(a5 + 1) << 10 | (unsigned)(a6 + 1) << 12 | (unsigned)(a7 + 1) << 14 | (unsigned)(a8 + 1) << 16 | (unsigned)(a9 + 1) << 18 |
         (unsigned)(a10 + 1) << 20 | (unsigned)(a11 + 1) << 22 | (unsigned)(a12 + 1) << 24 | (unsigned)(a13 + 1) << 26 | (unsigned)(a14 + 1) << 28 |
         (unsigned)(a15 + 1) << 30;
}
__device__ __forceinline__ int tz_sign(unsigned table, int k) { return (int)((table >> (2 * k)) & 3u) - 1; }
// the 4-point diamond (:553-571): top, left, right, bottom = point numbers 2, 4, 5, 7; also the first four of the 16-point one
constexpr unsigned kTz4X = tz_pack(0, -1, 1, 0, 0, 0, 0, 0), kTz4Y = tz_pack(-1, 0, 0, 1, 0, 0, 0, 0);
// the 8-point diamond (:574-634) in evaluation order: point numbers 2 1 3 4 5 6 8 7, the diagonal ones at iDist >> 1
constexpr unsigned kTz8X = tz_pack(0, -1, 1, -1, 1, -1, 1, 0), kTz8Y = tz_pack(-1, -1, -1, 0, 0, 1, 1, 1);
constexpr unsigned kTz8Nr = 2u | 1u << 4 | 3u << 8 | 4u << 12 | 5u << 16 | 6u << 20 | 8u << 24 | 7u << 28;
// xTZ2PointSearch (:351-479): entry 2 * (ucPointNr - 1) + p = the p-th point of the case
constexpr unsigned kTz2X = tz_pack(-1, 0, -1, 1, 0, 1, -1, -1, 1, 1, -1, 0, -1, 1, 1, 0);
constexpr unsigned kTz2Y = tz_pack(0, -1, -1, -1, -1, 0, 1, -1, -1, 1, 0, 1, 1, 1, 0, 1);

// One batch of xTZSearchHelp calls: the lanes [c * L, (c + 1) * L) hold candidate c = (cx, cy) of the batch, evaluated when
// `valid`; candidates are in evaluation order.  L is a power of two, the same in all lanes.
template <bool WP, class UNIT>
__device__ __forceinline__ void tz_eval(const UNIT &U, TzState &S, int L, int cx, int cy, bool valid, int nr, int dist) {
  const int lane = threadIdx.x, sub = lane & (L - 1);
  unsigned acc = 0;
  if (valid) {
    const int segs = U.w >> 2, items = (U.h >> U.sub_shift) * segs;
    const unsigned inv = 65536u / (unsigned)segs + 1u; // it / segs for it < 1024
    const unsigned bias2 = WP ? 0x80008000u : (1u << U.B) * 0x00010001u;
    const __attribute__((address_space(1))) short *base = U.ref + (ptrdiff_t)cy * U.stride + cx;
    for (int it = sub; it < items; it += L) { // at most 64 rows x 16 segments
      const int row = (int)(((unsigned)it * inv) >> 16), seg = it - row * segs, r = row << U.sub_shift;
      const uintptr_t a = (uintptr_t)(base + (ptrdiff_t)r * U.stride + 4 * seg);
      const unsigned sh = (a & 2) ? 16u : 0u;
      const __attribute__((address_space(1))) unsigned *q = (const __attribute__((address_space(1))) unsigned *)(a & ~(uintptr_t)3);
      const unsigned d0 = q[0], d1 = q[1], d2 = sh ? q[2] : 0u; // the third word holds a sample of the segment only at odd parity
      unsigned e0 = __builtin_amdgcn_alignbit(d1, d0, sh), e1 = __builtin_amdgcn_alignbit(d2, d1, sh);
      if constexpr (WP) { // the two samples of a word weighted on their own; each result is an int16, so + 2^15 per half cannot carry across
        e0 = ((unsigned)me_wp_pel(U.wp, (short)e0) & 0xffffu) | ((unsigned)me_wp_pel(U.wp, (short)(e0 >> 16)) << 16);
        e1 = ((unsigned)me_wp_pel(U.wp, (short)e1) & 0xffffu) | ((unsigned)me_wp_pel(U.wp, (short)(e1 >> 16)) << 16);
        e0 ^= bias2, e1 ^= bias2; // int16 + 2^15 as an unsigned 16-bit value = the sign bit flipped
      } else e0 += bias2, e1 += bias2;
      const uint2 o = *reinterpret_cast<const uint2 *>(U.org + r * U.w + 4 * seg);
      acc = __builtin_amdgcn_sad_u16(e0, o.x, acc);
      acc = __builtin_amdgcn_sad_u16(e1, o.y, acc);
    }
  }
  for (int m = 1; m < L; m <<= 1) acc += (unsigned)__shfl_xor((int)acc, m, 64);
  const uint32_t cost = ((acc << U.sub_shift) >> (U.B - 8)) + me_mv_cost(U.lambda, cx, cy, U.pred_x, U.pred_y, 2);
  const bool own = valid && sub == 0;
  const unsigned long long mask = __ballot(own);
  if (mask == 0) return; // uniform: nothing evaluated
  if (U.trace && own) {
    const uint32_t k = S.count + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    if (k < U.trace_cap) U.trace[2 * k] = ((uint32_t)cx & 0xffffu) | ((uint32_t)cy << 16), U.trace[2 * k + 1] = cost;
  }
  S.count += (uint32_t)__popcll(mask);
  unsigned long long key = own ? ((unsigned long long)cost << 32) | (unsigned)lane : ~0ull;
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned long long other = __shfl_xor(key, m, 64);
    key = other < key ? other : key;
  }
  const uint32_t wcost = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32));
  if (wcost < S.best) { // uniform.  wcost = 0xFFFFFFFF never passes, and the sentinel key carries that cost
    const int wl = __builtin_amdgcn_readfirstlane((int)((uint32_t)key & 63u));
    S.best = wcost;
    S.bx = __builtin_amdgcn_readfirstlane(__shfl(cx, wl, 64));
    S.by = __builtin_amdgcn_readfirstlane(__shfl(cy, wl, 64));
    S.dist = __builtin_amdgcn_readfirstlane(__shfl(dist, wl, 64));
    S.nr = __builtin_amdgcn_readfirstlane(__shfl(nr, wl, 64));
    S.round = 0;
  }
}
// the border rule: a coordinate that has moved by d is tested against the side it moved towards
__device__ __forceinline__ bool tz_inside(const TzUnit &U, int x, int y, int dx, int dy) {
  return (dx >= 0 || x >= U.left) && (dx <= 0 || x <= U.right) && (dy >= 0 || y >= U.top) && (dy <= 0 || y <= U.bottom);
}
// xTZ8PointDiamondSearch (:536-707) around (sx, sy)
template <bool WP, class UNIT>
__device__ __forceinline__ void tz_diamond(const UNIT &U, TzState &S, int sx, int sy, int d) {
  const int lane = threadIdx.x;
  S.round += 1;
  int L, dx, dy, nr, dist = d;
  if (d == 1) {
    const int k = lane >> 4;
    L = 16, dx = tz_sign(kTz4X, k), dy = tz_sign(kTz4Y, k), nr = (int)((0x7542u >> (4 * k)) & 15u);
  } else if (d <= 8) {
    const int k = lane >> 3;
    const bool diag = ((0x66u >> k) & 1u) != 0;
    dist = diag ? d >> 1 : d;
    L = 8, dx = tz_sign(kTz8X, k) * dist, dy = tz_sign(kTz8Y, k) * dist, nr = (int)((kTz8Nr >> (4 * k)) & 15u);
  } else {
    const int k = lane >> 2;
    L = 4, nr = 0;
    if (k < 4) dx = tz_sign(kTz4X, k) * d, dy = tz_sign(kTz4Y, k) * d; // top, left, right, bottom
    else { // index 1 .. 3 (:644-654): (XL, YT) (XR, YT) (XL, YB) (XR, YB)
      const int i = ((k - 4) >> 2) + 1, j = (k - 4) & 3, q = (d >> 2) * i;
      dx = (j & 1) ? q : -q, dy = (j & 2) ? d - q : q - d;
    }
  }
  const int cx = sx + dx, cy = sy + dy;
  tz_eval<WP>(U, S, L, cx, cy, tz_inside(U, cx, cy, dx, dy), nr, dist);
}
// xTZ2PointSearch (:351-479) around the best point; ucPointNr = 0 evaluates nothing (the reference asserts: it is unreachable,
// because uiBestDistance == 1 is only ever set together with a point number of 1 .. 8)
template <bool WP, class UNIT>
__device__ __forceinline__ void tz_two_point(const UNIT &U, TzState &S) {
  const int p = (int)threadIdx.x >> 5, e = S.nr > 0 ? 2 * (S.nr - 1) + p : 0;
  const int dx = tz_sign(kTz2X, e), dy = tz_sign(kTz2Y, e), cx = S.bx + dx, cy = S.by + dy;
  tz_eval<WP>(U, S, 32, cx, cy, S.nr > 0 && tz_inside(U, cx, cy, dx, dy), 0, 2);
}

constexpr int kTzThreads = 64, kTzRaster = 5, kTzPassCap = 1024;
template <class ARGS>
__global__ __launch_bounds__(kTzThreads) void k_tz_search(ARGS A) {
  constexpr bool WP = ARGS::weighted;
  extern __shared__ __attribute__((aligned(16))) unsigned short s_tz_org[];
  const int i = blockIdx.x, lane = threadIdx.x;
  const hmx_me_unit u = A.units[i];
  const hmx_tz_unit z = A.tz[i];
  typedef __attribute__((address_space(1))) const short gpel;
  {
    const int bias = WP ? 32768 : 1 << A.B;
    const gpel *src = (const gpel *)A.org.p[0] + (size_t)u.y * A.org.s[0] + u.x;
    const int lw = u.w == 4 ? 2 : u.w == 8 ? 3 : u.w == 16 ? 4 : u.w == 32 ? 5 : u.w == 64 ? 6 : -1;
    for (int k = lane; k < u.w * u.h; k += kTzThreads) { // at most 64 rounds
      const int r = lw >= 0 ? k >> lw : k / u.w, c = k - r * u.w;
      s_tz_org[k] = (unsigned short)(src[(size_t)r * A.org.s[0] + c] + bias);
    }
  }
  __syncthreads();
  typename std::conditional<WP, TzUnitWp, TzUnit>::type U;
  const PlanesDev &R = A.refs[u.ref < 4 ? u.ref : 0];
  U.stride = R.s[0];
  U.ref = (gpel *)R.p[0] + (ptrdiff_t)u.y * R.s[0] + u.x;
  U.org = s_tz_org;
  U.w = u.w, U.h = u.h, U.sub_shift = WP ? 0 : u.sub_shift, U.B = A.B;
  if constexpr (WP) U.wp = A.wp[u.ref < 4 ? u.ref : 0];
  U.left = u.left, U.top = u.top, U.right = u.right, U.bottom = u.bottom, U.pred_x = u.pred_x, U.pred_y = u.pred_y;
  U.lambda = A.lambda;
  U.trace = A.trace ? (__attribute__((address_space(1))) uint32_t *)A.trace + 2 * (size_t)i * (size_t)A.trace_cap : nullptr;
  U.trace_cap = (uint32_t)A.trace_cap;
  TzState S{0xffffffffu, 0, 0, 0, 0, 0, 0u};
  const int range = z.range;
  // the start point, then the zero vector (:4321, :4338): neither is tested against the box
  tz_eval<WP>(U, S, 32, lane < 32 ? z.start_x : 0, lane < 32 ? z.start_y : 0, true, 0, 0);
  int sx = S.bx, sy = S.by;
  for (int d = 1; d <= range; d *= 2) { // first search (:4347-4362)
    tz_diamond<WP>(U, S, sx, sy, d);
    if (S.round >= 3) break;
  }
  if (S.dist == 1) { // :4383-4387, no test of ucPointNr
    S.dist = 0;
    tz_two_point<WP>(U, S);
  }
  if (S.dist > kTzRaster) { // :4390-4400
    S.dist = kTzRaster;
    const int nx = (U.right - U.left) / kTzRaster + 1, ny = (U.bottom - U.top) / kTzRaster + 1, total = nx * ny; // at most 26 x 26
    for (int c0 = 0; c0 < total; c0 += 16) {
      const int c = c0 + (lane >> 2), ry = c / nx, rx = c - ry * nx;
      tz_eval<WP>(U, S, 4, U.left + kTzRaster * rx, U.top + kTzRaster * ry, c < total, 0, kTzRaster);
    }
  }
  int passes = 0;
  bool capped = false;
  while (S.dist > 0) { // star refinement (:4435-4469)
    if (passes >= A.max_passes || passes >= kTzPassCap) {
      capped = true;
      break;
    }
    passes++;
    sx = S.bx, sy = S.by;
    S.dist = 0, S.nr = 0;
    for (int d = 1; d <= range; d *= 2) tz_diamond<WP>(U, S, sx, sy, d);
    if (S.dist == 1) {
      S.dist = 0;
      if (S.nr != 0) tz_two_point<WP>(U, S);
    }
  }
  if (lane == 0) {
    hmx_me_result r;
    r.mvx = (int16_t)S.bx, r.mvy = (int16_t)S.by;
    r.cost = capped ? 0xffffffffu : S.best;
    r.sad = capped ? 0xffffffffu : S.best - me_mv_cost(A.lambda, S.bx, S.by, U.pred_x, U.pred_y, 2); // ruiSAD (:4473)
    A.result[i] = r;
    if (A.trace_count) A.trace_count[i] = S.count;
  }
}

static int me_tz(hmx_ctx *c, const char *name, const hmx_me_unit *units, const hmx_tz_unit *tz, int n, const hmx_pic *refs, int n_refs,
                 const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result,
                 hmx_tz_point *d_trace, uint32_t *d_trace_count, int trace_cap, const hmx_wp *wp) {
  MeWp wpt[4] = {};
  if (const int r = me_call_check(c, name, !c || !units || !tz || !refs || !org || !d_result, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, wp, wpt))
    return r;
  if ((d_trace == nullptr) != (d_trace_count == nullptr)) return fail(c, HMX_ERR_ARG, std::string(name) + ": d_trace and d_trace_count go together");
  if (d_trace && trace_cap < 1) return fail(c, HMX_ERR_ARG, std::string(name) + ": trace_cap must be at least 1");
  size_t lds = 0;
  for (int i = 0; i < n; i++) {
    const hmx_me_unit &u = units[i];
    const hmx_tz_unit &z = tz[i];
    const char *why = me_unit_check(u, n_refs, pic_w, pic_h, true);
    // every evaluated point lies in the bounding rectangle of box U {(0, 0)}: the zero vector is evaluated unconditionally
    const int rl = std::min<int>(u.left, 0), rr = std::max<int>(u.right, 0), rt = std::min<int>(u.top, 0), rb = std::max<int>(u.bottom, 0);
    if (!why)
      why = z.range < 1 || z.range > 64 ? "range must be 1 .. 64"
            : z.reserved != 0           ? "reserved must be 0"
            : z.start_x < u.left || z.start_x > u.right || z.start_y < u.top || z.start_y > u.bottom ? "the start point lies outside the search box"
            : !me_reach_ok(u, rl, rt, rr, rb, pic_w, pic_h, margin_x, margin_y)
                ? "a block of the box or the zero vector's rectangle reaches outside the reference's margins"
                : nullptr;
    if (why) return me_unit_refuse(c, name, i, why);
    lds = std::max(lds, sizeof(short) * (size_t)u.w * (size_t)u.h);
  }
  TzArgsWp A{};
  const size_t unit_bytes = sizeof(hmx_me_unit) * (size_t)n, tz_bytes = sizeof(hmx_tz_unit) * (size_t)n; // the caller's host arrays
  if (const int r = arena_reserve(c, {unit_bytes, tz_bytes}, "argument arena (unit list too long: split the call)")) return r;
  A.units = static_cast<const hmx_me_unit *>(arena_place(c, units, unit_bytes));
  A.tz = static_cast<const hmx_tz_unit *>(arena_place(c, tz, tz_bytes));
  if (!A.units || !A.tz) return fail(c, HMX_ERR_INTERNAL, kArenaOutside);
  A.max_passes = std::min(kTzPassCap, std::max(1, c->knob.tz_max_passes));
  A.lambda = lambda;
  A.result = d_result;
  A.trace = d_trace;
  A.trace_count = d_trace_count;
  A.trace_cap = d_trace ? trace_cap : 0;
  me_launch<TzArgs>(c, A, refs, n_refs, org, wp != nullptr, wpt, [&](const auto &a) {
    hipLaunchKernelGGL(k_tz_search<std::decay_t<decltype(a)>>, dim3((unsigned)n), dim3(kTzThreads), lds, c->stream, a);
  });
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_batch_tz_search(hmx_ctx *c, const hmx_me_unit *units, const hmx_tz_unit *tz, int n, const hmx_pic *refs, int n_refs,
                                   const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result,
                                   hmx_tz_point *d_trace, uint32_t *d_trace_count, int trace_cap) {
  return me_tz(c, "hmx_batch_tz_search", units, tz, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda, d_result, d_trace, d_trace_count,
               trace_cap, nullptr);
}
extern "C" int hmx_batch_tz_search_wp(hmx_ctx *c, const hmx_me_unit *units, const hmx_tz_unit *tz, int n, const hmx_pic *refs, int n_refs,
                                      const hmx_pic *org, int pic_w, int pic_h, int margin_x, int margin_y, uint32_t lambda, hmx_me_result *d_result,
                                      hmx_tz_point *d_trace, uint32_t *d_trace_count, int trace_cap, const hmx_wp *wp) {
  return me_tz(c, "hmx_batch_tz_search_wp", units, tz, n, refs, n_refs, org, pic_w, pic_h, margin_x, margin_y, lambda, d_result, d_trace,
               d_trace_count, trace_cap, wp);
}
