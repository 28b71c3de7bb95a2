// hmx_aq.hip -- the encoder's adaptive QP (--AdaptiveQP=1): TEncPreanalyzer::xPreanalyze (TLibEncoder/TEncPreanalyzer.cpp:64-139),
// which TEncTop::encode runs on every input picture (TEncTop.cpp:383-386), and TEncCu::xComputeQP (TEncCu.cpp:1114-1136), which
// turns its activities into the QP of every coding unit.  The walk over the luma plane is one kernel that reads every sample once
// for all AQ layers (k_aq_activity); the layer averages are ordered double sums (k_aq_avg); the QP of every unit of every layer is
// a third small kernel (k_aq_qp).  The scalar forms of the same arithmetic are host code without a context.
#include "hmx_host.h"

#include <cmath>
#include <mutex>

// Every double expression below is the reference's, operation by operation: a fused x / N - avg * avg or S * a + A rounds once
// where the host rounds twice.
#pragma clang fp contract(off)

namespace {
typedef short aqs8v __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int kAqTile = 64;             // one wave takes a 64 x 64 tile: one CTU of 64, four of 32, sixteen of 16
constexpr int kAqCells = kAqTile / 4;   // 4 x 4 cells across a tile
constexpr int kAqSat = kAqCells + 1;    // summed-area tables carry a zero row and column in front

struct AqArgs {
  const PlanesDev *pics; // [n_pics]
  double *act;           // [n_pics][G.total]
  hmx_aq_geom G;
};

// min over the four lanes of a quad, in every lane of it: the halves of the double travel through the VALU's lane crossbar like
// group_sum's terms (quad_perm [1,0,3,2], then [2,3,0,1]).  Every lane of the wave runs it (the callers stand in wave-uniform
// control flow), so no partner lies outside EXEC.
template <int CTRL>
__device__ __forceinline__ double dpp_min_f64(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, true);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)((u64)b >> 32), CTRL, 0xf, 0xf, true);
  const double o = __longlong_as_double((long long)((u64)lo | ((u64)hi << 32)));
  return o < v ? o : v;
}
__device__ __forceinline__ double quad_min_f64(double v) { return dpp_min_f64<0x4E>(dpp_min_f64<0xB1>(v)); }

// One wave per (tile, picture).  Lane l owns the 8 x 8 strip (l & 7, l >> 3) of the tile: eight 16-byte row loads (one load per
// sample where the strip's rows do not start on 16-byte boundaries), four 4 x 4 cells of sum and sum of squares.  Picture sizes
// are multiples of 8, so a strip lies inside the picture or outside it, and every quadrant of every unit of every layer -- a unit
// cut by the picture edge splits at cw >> 1, a multiple of 4 -- is a rectangle of cells.  The cells become two summed-area tables
// in LDS; the samples are not visited again.
// Widening: a cell's 16 samples below 2^12 sum to less than 2^16 and their squares to less than 2^28 (u32); the table of sums
// ends below 2^24 (u32), the table of squares below 2^36 (u64).
__global__ __launch_bounds__(64) void k_aq_activity(AqArgs A) {
  __shared__ unsigned s1[kAqSat][kAqSat];
  __shared__ u64 s2[kAqSat][kAqSat];
  const int lane = threadIdx.x, tx = blockIdx.x * kAqTile, ty = blockIdx.y * kAqTile, pic = blockIdx.z;
  const int w = A.G.pic_w, h = A.G.pic_h;
  const PlanesDev *P = A.pics + pic;
  const int sx = lane & 7, sy = lane >> 3, x0 = tx + 8 * sx, y0 = ty + 8 * sy;
  unsigned c1[2][2] = {{0, 0}, {0, 0}}, c2[2][2] = {{0, 0}, {0, 0}};
  if (x0 < w && y0 < h) {
    const int stride = P->s[0];
    const short *p = P->p[0] + (ptrdiff_t)y0 * stride + x0;
    int v[8][8];
    if ((((uintptr_t)p | (uintptr_t)((ptrdiff_t)stride * 2)) & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 8; r++) {
        const aqs8v t = *reinterpret_cast<const aqs8v *>(p + (ptrdiff_t)r * stride);
#pragma unroll
        for (int j = 0; j < 8; j++) v[r][j] = t[j];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 8; r++)
#pragma unroll
        for (int j = 0; j < 8; j++) v[r][j] = p[(ptrdiff_t)r * stride + j];
    }
#pragma unroll
    for (int r = 0; r < 8; r++)
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const unsigned s = (unsigned)v[r][j];
        c1[r >> 2][j >> 2] += s;
        c2[r >> 2][j >> 2] += s * s;
      }
  }
  if (lane < kAqSat) s1[0][lane] = 0, s2[0][lane] = 0, s1[lane][0] = 0, s2[lane][0] = 0;
#pragma unroll
  for (int j = 0; j < 2; j++)
#pragma unroll
    for (int i = 0; i < 2; i++) s1[2 * sy + j + 1][2 * sx + i + 1] = c1[j][i], s2[2 * sy + j + 1][2 * sx + i + 1] = c2[j][i];
  __syncthreads();
  if (lane < kAqCells) { // prefix along every row, then along every column
    unsigned a = 0;
    u64 b = 0;
    for (int c = 1; c < kAqSat; c++) {
      a += s1[lane + 1][c], b += s2[lane + 1][c];
      s1[lane + 1][c] = a, s2[lane + 1][c] = b;
    }
  }
  __syncthreads();
  if (lane < kAqCells) {
    unsigned a = 0;
    u64 b = 0;
    for (int r = 1; r < kAqSat; r++) {
      a += s1[r][lane + 1], b += s2[r][lane + 1];
      s1[r][lane + 1] = a, s2[r][lane + 1] = b;
    }
  }
  __syncthreads();
  // One lane per (unit of the tile, quadrant), the quadrant in the lane's low two bits; the unit's minimum over its quad on DPP.
  double *act = A.act + (size_t)pic * A.G.total;
  for (int d = 0; d < A.G.depths; d++) {
    const int part = A.G.part[d], lp = 31 - __builtin_clz(part), ul = 6 - lp; // 1 << ul units across the tile
    const int items = 4 << (2 * ul);
    for (int base = 0; base < items; base += 64) {
      const int i = base + lane, q = i & 3, u = i >> 2;
      const int x = tx + ((u & ((1 << ul) - 1)) << lp), y = ty + ((u >> ul) << lp);
      const bool valid = i < items && x < w && y < h;
      double var = __longlong_as_double(0x7ff0000000000000ll);
      if (valid) {
        const int cw = min(part, w - x), ch = min(part, h - y);
        const int xa = (q & 1) ? cw >> 1 : 0, xb = (q & 1) ? cw : cw >> 1, ya = (q & 2) ? ch >> 1 : 0, yb = (q & 2) ? ch : ch >> 1;
        const int ca = (x - tx + xa) >> 2, cb = (x - tx + xb) >> 2, ra = (y - ty + ya) >> 2, rb = (y - ty + yb) >> 2;
        const unsigned sum = s1[rb][cb] - s1[ra][cb] - s1[rb][ca] + s1[ra][ca];
        const u64 sumsq = s2[rb][cb] - s2[ra][cb] - s2[rb][ca] + s2[ra][ca];
        const double n = (double)(unsigned)(cw * ch); // the samples of the WHOLE unit, as the reference counts them (:94-114)
        const double avg = (double)sum / n;
        var = (double)sumsq / n - avg * avg;
      }
      var = quad_min_f64(var);
      if (valid && q == 0) act[A.G.first[d] + (y >> lp) * A.G.nx[d] + (x >> lp)] = 1.0 + var;
    }
  }
}

struct AqAvgArgs {
  const double *act;
  double *avg; // [n_pics][G.depths]
  hmx_aq_geom G;
};
__device__ __forceinline__ double readlane_f64(double v, int j) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, j), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((u64)b >> 32), j);
  return __longlong_as_double((long long)((u64)lo | ((u64)hi << 32)));
}
// dSumAct (:79, :131) is an ORDERED sum: one wave per (layer, picture) fetches 64 units at a time, the next two batches in flight
// while this one is added lane by lane in raster order.  A unit past the end is +0.0, which leaves a sum of activities (>= 1.0) as
// it is; its load is clamped to the last unit and not branched around, so that no wait for a load stands in front of the adds.
__global__ __launch_bounds__(64) void k_aq_avg(AqAvgArgs A) {
  const int d = blockIdx.x, pic = blockIdx.y, lane = threadIdx.x;
  const int n = A.G.nx[d] * A.G.ny[d];
  const double *a = A.act + (size_t)pic * A.G.total + A.G.first[d];
  const auto fetch = [&](int i) {
    const double v = a[min(i, n - 1)];
    return i < n ? v : 0.0;
  };
  double s = 0.0, cur = fetch(lane), nxt = fetch(64 + lane);
  for (int base = 0; base < n; base += 64) {
    const double far = fetch(base + 128 + lane);
#pragma unroll
    for (int j = 0; j < 64; j++) s += readlane_f64(cur, j);
    cur = nxt, nxt = far;
  }
  if (lane == 0) A.avg[(size_t)pic * A.G.depths + d] = s / (double)(unsigned)n;
}

struct AqQpArgs {
  const double *act, *avg, *thr; // thr[n_thr]: hmx_aq_thresholds
  const int *slice_qp;           // [n_pics]
  int8_t *qp;                    // [n_pics][G.total]
  hmx_aq_geom G;
  double scale;                  // pow(2.0, range / 6.0), formed on the host
  int n_thr, range, qp_min;
};
// xComputeQP for every unit of every layer: dNormAct in the reference's operations, the offset as the count of thresholds it has
// reached (the logarithm is the host's, see aq_thresholds).
__global__ __launch_bounds__(256) void k_aq_qp(AqQpArgs A) {
  const int u = blockIdx.x * 256 + threadIdx.x, pic = blockIdx.y;
  if (u >= A.G.total) return;
  int d = 0;
  for (int k = 1; k < A.G.depths; k++) d += u >= A.G.first[k];
  const double a = A.act[(size_t)pic * A.G.total + u], avg = A.avg[(size_t)pic * A.G.depths + d];
  const double norm = (A.scale * a + avg) / (a + A.scale * avg);
  int cnt = 0;
  for (int k = 0; k < A.n_thr; k++) cnt += A.thr[k] <= norm;
  const int qp = A.slice_qp[pic] + cnt - A.range - 1;
  A.qp[(size_t)pic * A.G.total + u] = (int8_t)min(51, max(A.qp_min, qp));
}

struct AqUnitArgs {
  const int8_t *layer_qp;  // [n_pics][G.total]: hmx_aq_qp_map_multi
  const uint8_t *cu_depth; // [n_pics][uh][uw]
  int8_t *qp;              // [n_pics][uh][uw]
  hmx_aq_geom G;
  int uw, uh;
};
// The QP of every 4x4 luma unit: its CU at depth D reads layer min(D, depths - 1), unit (x / part, y / part) (TEncCu.cpp:1121-1124).
// The depth byte is clamped before it picks a layer, so whatever it holds the read stays inside the picture's layer array.
__global__ __launch_bounds__(256) void k_aq_unit_qp(AqUnitArgs A) {
  const int u = blockIdx.x * 256 + threadIdx.x, pic = blockIdx.y, n = A.uw * A.uh;
  if (u >= n) return;
  const int uy = u / A.uw, ux = u - uy * A.uw;
  const int D = min((int)A.cu_depth[(size_t)pic * n + u], A.G.depths - 1);
  int first = A.G.first[0], nx = A.G.nx[0], part = A.G.part[0];
#pragma unroll
  for (int k = 1; k < HMX_AQ_MAX_DEPTHS; k++)
    if (k == D) first = A.G.first[k], nx = A.G.nx[k], part = A.G.part[k];
  const int lp = 31 - __builtin_clz(part);
  A.qp[(size_t)pic * n + u] = A.layer_qp[(size_t)pic * A.G.total + first + ((4 * uy) >> lp) * nx + ((4 * ux) >> lp)];
}

// ---- host ----
const char *const kAqDomain = "ctu must be 16, 32 or 64, depths at least 1 with ctu >> (depths - 1) >= 8, the picture size positive multiples of 8 up to 16384";
bool aq_domain_ok(int pic_w, int pic_h, int ctu, int depths) {
  return (ctu == 16 || ctu == 32 || ctu == 64) && depths >= 1 && depths <= HMX_AQ_MAX_DEPTHS && (ctu >> (depths - 1)) >= 8 && pic_w > 0 && pic_h > 0 &&
         pic_w % 8 == 0 && pic_h % 8 == 0 && pic_w <= 16384 && pic_h <= 16384;
}

// the reference's expression (TEncCu.cpp:1132-1133) with libm's log
double aq_offset_of_norm(double norm) { return floor(log(norm) / log(2.0) * 6.0 + 0.49999); }
uint64_t aq_bits(double v) {
  uint64_t b;
  memcpy(&b, &v, 8);
  return b;
}
double aq_double(uint64_t b) {
  double v;
  memcpy(&v, &b, 8);
  return v;
}
// T[k + range], k = -range .. range: the smallest double at which aq_offset_of_norm reaches k, by bisection over the doubles
// (positive doubles order like their bit patterns), then held against the 64 doubles on either side.  Built once per range.
struct AqTable {
  bool built = false;
  std::vector<double> t;
  std::string why; // not empty: the verification failed
};
const AqTable &aq_thresholds(int range) {
  static std::mutex mu;
  static AqTable tabs[65];
  std::lock_guard<std::mutex> lock(mu);
  AqTable &T = tabs[range];
  if (T.built) return T;
  T.built = true;
  for (int k = -range; k <= range; k++) {
    uint64_t lo = aq_bits(ldexp(1.0, -13)), hi = aq_bits(ldexp(1.0, 13)); // offsets -78 and +78: outside every range
    while (hi - lo > 1) {
      const uint64_t mid = lo + (hi - lo) / 2;
      if (aq_offset_of_norm(aq_double(mid)) >= (double)k) hi = mid;
      else lo = mid;
    }
    bool ok = aq_offset_of_norm(aq_double(hi)) == (double)k;
    for (uint64_t j = 1; j <= 64 && ok; j++)
      ok = aq_offset_of_norm(aq_double(hi - j)) == (double)(k - 1) && aq_offset_of_norm(aq_double(hi + j)) == (double)k;
    if (!ok && T.why.empty())
      T.why = "the offset expression is not monotonic within 64 doubles of its threshold for offset " + std::to_string(k) + " (range " + std::to_string(range) + ")";
    T.t.push_back(aq_double(hi));
  }
  return T;
}
} // namespace

extern "C" int hmx_aq_layout(int pic_w, int pic_h, int ctu, int depths, hmx_aq_geom *out) {
  if (!out || !aq_domain_ok(pic_w, pic_h, ctu, depths)) return HMX_ERR_ARG;
  hmx_aq_geom g{};
  g.pic_w = pic_w, g.pic_h = pic_h, g.ctu = ctu, g.depths = depths;
  for (int d = 0; d < depths; d++) { // TEncPic.cpp:82-89, :135-138
    g.part[d] = ctu >> d;
    g.nx[d] = (pic_w + g.part[d] - 1) / g.part[d], g.ny[d] = (pic_h + g.part[d] - 1) / g.part[d];
    g.first[d] = g.total;
    g.total += g.nx[d] * g.ny[d];
  }
  *out = g;
  return HMX_OK;
}

extern "C" int hmx_aq_activity_multi(hmx_ctx *c, int n_pics, const hmx_pic *pics, int pic_w, int pic_h, int ctu, int depths, double *d_act,
                                     double *d_avg) {
  if (!c || !pics || !d_act || !d_avg) return fail(c, HMX_ERR_ARG, "hmx_aq_activity_multi: null argument");
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, "hmx_aq_activity_multi: n_pics must be 1..65535");
  hmx_aq_geom G;
  if (hmx_aq_layout(pic_w, pic_h, ctu, depths, &G)) return fail(c, HMX_ERR_ARG, std::string("hmx_aq_activity_multi: ") + kAqDomain);
  if (c->cfg.bit_depth < 8 || c->cfg.bit_depth > 12) return fail(c, HMX_ERR_ARG, "hmx_aq_activity_multi: the context's bit depth must be 8..12");
  std::vector<PlanesDev> t((size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    if (!pics[i].plane[0]) return fail(c, HMX_ERR_ARG, "hmx_aq_activity_multi: null luma plane");
    t[i] = to_dev(&pics[i]);
  }
  const PlanesDev *d_pics = static_cast<const PlanesDev *>(arena_push(c, t.data(), sizeof(PlanesDev) * t.size()));
  if (!d_pics) return fail(c, HMX_ERR_NOMEM, "argument arena");
  const dim3 tiles((unsigned)((pic_w + kAqTile - 1) / kAqTile), (unsigned)((pic_h + kAqTile - 1) / kAqTile), (unsigned)n_pics);
  hipLaunchKernelGGL(k_aq_activity, tiles, dim3(64), 0, c->stream, AqArgs{d_pics, d_act, G});
  hipLaunchKernelGGL(k_aq_avg, dim3((unsigned)depths, (unsigned)n_pics), dim3(64), 0, c->stream, AqAvgArgs{d_act, d_avg, G});
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_aq_average_multi(hmx_ctx *c, int n_pics, int pic_w, int pic_h, int ctu, int depths, const double *d_act, double *d_avg) {
  if (!c || !d_act || !d_avg) return fail(c, HMX_ERR_ARG, "hmx_aq_average_multi: null argument");
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, "hmx_aq_average_multi: n_pics must be 1..65535");
  hmx_aq_geom G;
  if (hmx_aq_layout(pic_w, pic_h, ctu, depths, &G)) return fail(c, HMX_ERR_ARG, std::string("hmx_aq_average_multi: ") + kAqDomain);
  hipLaunchKernelGGL(k_aq_avg, dim3((unsigned)depths, (unsigned)n_pics), dim3(64), 0, c->stream, AqAvgArgs{d_act, d_avg, G});
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_aq_activity(hmx_ctx *c, const hmx_pic *pic, int pic_w, int pic_h, int ctu, int depths, double *d_act, double *d_avg) {
  return hmx_aq_activity_multi(c, 1, pic, pic_w, pic_h, ctu, depths, d_act, d_avg);
}

extern "C" int hmx_aq_thresholds(int range, double *out) {
  if (!out || range < 1 || range > 64) return HMX_ERR_ARG;
  const AqTable &T = aq_thresholds(range);
  if (!T.why.empty()) return HMX_ERR_INTERNAL;
  std::copy(T.t.begin(), T.t.end(), out);
  return HMX_OK;
}

extern "C" int hmx_aq_qp_map_multi(hmx_ctx *c, int n_pics, int pic_w, int pic_h, int ctu, int depths, const double *d_act, const double *d_avg,
                                   const int *slice_qp, int range, int qp_bd_offset, int8_t *d_qp) {
  if (!c || !d_act || !d_avg || !slice_qp || !d_qp) return fail(c, HMX_ERR_ARG, "hmx_aq_qp_map_multi: null argument");
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, "hmx_aq_qp_map_multi: n_pics must be 1..65535");
  hmx_aq_geom G;
  if (hmx_aq_layout(pic_w, pic_h, ctu, depths, &G)) return fail(c, HMX_ERR_ARG, std::string("hmx_aq_qp_map_multi: ") + kAqDomain);
  if (range < 1 || range > 64) return fail(c, HMX_ERR_ARG, "hmx_aq_qp_map_multi: range must be 1..64");
  if (qp_bd_offset < 0 || qp_bd_offset > 48) return fail(c, HMX_ERR_ARG, "hmx_aq_qp_map_multi: qp_bd_offset must be 0..48");
  for (int i = 0; i < n_pics; i++)
    if (slice_qp[i] < -qp_bd_offset || slice_qp[i] > 51)
      return fail(c, HMX_ERR_ARG, "hmx_aq_qp_map_multi: slice_qp[" + std::to_string(i) + "] outside -qp_bd_offset..51");
  const AqTable &T = aq_thresholds(range);
  if (!T.why.empty()) return fail(c, HMX_ERR_INTERNAL, "hmx_aq_qp_map_multi: " + T.why);
  const size_t thr_bytes = sizeof(double) * T.t.size(), sqp_bytes = sizeof(int) * (size_t)n_pics; // two tables, one launch: reserved together
  if (const int r = arena_reserve(c, {thr_bytes, sqp_bytes}, "argument arena")) return r;
  const double *d_thr = static_cast<const double *>(arena_place(c, T.t.data(), thr_bytes));
  const int *d_sqp = static_cast<const int *>(arena_place(c, slice_qp, sqp_bytes));
  if (!d_thr || !d_sqp) return fail(c, HMX_ERR_INTERNAL, kArenaOutside);
  const AqQpArgs A{d_act, d_avg, d_thr, d_sqp, d_qp, G, pow(2.0, range / 6.0), (int)T.t.size(), range, -qp_bd_offset};
  hipLaunchKernelGGL(k_aq_qp, dim3((unsigned)((G.total + 255) / 256), (unsigned)n_pics), dim3(256), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

extern "C" int hmx_aq_unit_qp_multi(hmx_ctx *c, int n_pics, int pic_w, int pic_h, int ctu, int depths, const int8_t *d_layer_qp,
                                    const uint8_t *d_cu_depth, int8_t *d_qp) {
  if (!c || !d_layer_qp || !d_cu_depth || !d_qp) return fail(c, HMX_ERR_ARG, "hmx_aq_unit_qp_multi: null argument");
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, "hmx_aq_unit_qp_multi: n_pics must be 1..65535");
  hmx_aq_geom G;
  if (hmx_aq_layout(pic_w, pic_h, ctu, depths, &G)) return fail(c, HMX_ERR_ARG, std::string("hmx_aq_unit_qp_multi: ") + kAqDomain);
  const int uw = pic_w / 4, uh = pic_h / 4; // multiples of 8
  const AqUnitArgs A{d_layer_qp, d_cu_depth, d_qp, G, uw, uh};
  hipLaunchKernelGGL(k_aq_unit_qp, dim3((unsigned)((uw * uh + 255) / 256), (unsigned)n_pics), dim3(256), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

// ---- host scalars ----
extern "C" int hmx_aq_offset(double act, double avg_act, int range) {
  const double scale = pow(2.0, range / 6.0);
  const double norm = (scale * act + avg_act) / (act + scale * avg_act);
  return (int)aq_offset_of_norm(norm);
}
extern "C" int hmx_aq_compute_qp(const hmx_aq_geom *g, const double *act, const double *avg, int cu_x, int cu_y, int cu_depth, int slice_qp, int range,
                                 int qp_bd_offset) {
  if (!g || !act || !avg || g->depths < 1 || g->depths > HMX_AQ_MAX_DEPTHS || cu_x < 0 || cu_y < 0 || cu_x >= g->pic_w || cu_y >= g->pic_h ||
      cu_depth < 0)
    return HMX_AQ_NO_QP;
  const int d = std::min(cu_depth, g->depths - 1); // :1121
  const int u = g->first[d] + (cu_y / g->part[d]) * g->nx[d] + cu_x / g->part[d];
  const int qp = slice_qp + hmx_aq_offset(act[u], avg[d], range);
  return std::min(51, std::max(-qp_bd_offset, qp)); // MAX_QP = 51
}
