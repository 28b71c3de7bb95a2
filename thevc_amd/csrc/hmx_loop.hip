// hmx_loop.hip: deblocking and SAO (application), YUV file formats -- part of libhmx (include/hmx.h), gfx950.  See hmx_host.h for how the library is cut into translation units.
#include "hmx_host.h"

// ---- deblocking filter, application part (TLibCommon/TComLoopFilter.cpp:571-922) ----
// One launch per direction over the whole picture (loopFilterPic :153-201 filters every vertical edge of the
// picture before the first horizontal one).  Work item = one 4x4 luma unit whose left (top) side is an edge of
// the 8x8 grid with a non-zero strength: the thread filters the unit's four luma lines and, on the chroma grid
// with strength 2, two lines of Cb and Cr.  Edges are 8 samples apart and a filter reads 4 and writes 3 samples
// per side, so the work items of one launch touch disjoint samples.
static __constant__ unsigned char kDbkTc[54] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                         2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24};
static __constant__ unsigned char kDbkBeta[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15,
                                           16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64};
static __constant__ unsigned char kChromaScale[58] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
                                               20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 33, 33, 34, 34, 35, 35,
                                               36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51};
struct DbkArgs {
  PlanesDev rec;
  const unsigned char *bs; // of this direction
  const signed char *qp;
  const unsigned char *no_filter;
  int uw, uh, dir, B, boff, toff;
};
__global__ __launch_bounds__(256) void k_deblock(DbkArgs A) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= A.uw * A.uh) return;
  const int ux = u % A.uw, uy = u / A.uw, dir = A.dir;
  const int b = A.bs[u];
  if (!b || ((dir ? uy : ux) & 1)) return;
  const int up = dir ? u - A.uw : u - 1;
  const bool pn = A.no_filter && A.no_filter[up], qn = A.no_filter && A.no_filter[u];
  const int q_avg = ((int)A.qp[up] + (int)A.qp[u] + 1) >> 1;
  const int B = A.B, scale = 1 << (B - 8), maxv = (1 << B) - 1;
  {
    const int tc = kDbkTc[clip3(0, 53, q_avg + 2 * (b - 1) + (A.toff << 1))] * scale;
    const int beta = kDbkBeta[clip3(0, 51, q_avg + (A.boff << 1))] * scale;
    const int side = (beta + (beta >> 1)) >> 3, cut = tc * 10;
    const int st = A.rec.s[0], across = dir ? st : 1, along = dir ? 1 : st;
    short *s = A.rec.p[0] + (size_t)(4 * uy) * st + 4 * ux;
    int m[4][8];
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
      for (int k = 0; k < 8; k++) m[l][k] = s[(ptrdiff_t)l * along + (ptrdiff_t)(k - 4) * across];
    const int dp0 = abs(m[0][1] - 2 * m[0][2] + m[0][3]), dq0 = abs(m[0][4] - 2 * m[0][5] + m[0][6]);
    const int dp3 = abs(m[3][1] - 2 * m[3][2] + m[3][3]), dq3 = abs(m[3][4] - 2 * m[3][5] + m[3][6]);
    const int d0 = dp0 + dq0, d3 = dp3 + dq3, dp = dp0 + dp3, dq = dq0 + dq3, d = d0 + d3;
    if (d < beta) {
      const bool fp = dp < side, fq = dq < side;
      const bool s0 = (abs(m[0][0] - m[0][3]) + abs(m[0][7] - m[0][4]) < (beta >> 3)) && (2 * d0 < (beta >> 2)) &&
                      (abs(m[0][3] - m[0][4]) < ((tc * 5 + 1) >> 1));
      const bool s3 = (abs(m[3][0] - m[3][3]) + abs(m[3][7] - m[3][4]) < (beta >> 3)) && (2 * d3 < (beta >> 2)) &&
                      (abs(m[3][3] - m[3][4]) < ((tc * 5 + 1) >> 1));
      const bool strong = s0 && s3;
#pragma unroll
      for (int l = 0; l < 4; l++) {
        const int m0 = m[l][0], m1 = m[l][1], m2 = m[l][2], m3 = m[l][3], m4 = m[l][4], m5 = m[l][5], m6 = m[l][6], m7 = m[l][7];
        int n1 = m1, n2 = m2, n3 = m3, n4 = m4, n5 = m5, n6 = m6;
        if (strong) {
          n3 = clip3(m3 - 2 * tc, m3 + 2 * tc, (m1 + 2 * m2 + 2 * m3 + 2 * m4 + m5 + 4) >> 3);
          n4 = clip3(m4 - 2 * tc, m4 + 2 * tc, (m2 + 2 * m3 + 2 * m4 + 2 * m5 + m6 + 4) >> 3);
          n2 = clip3(m2 - 2 * tc, m2 + 2 * tc, (m1 + m2 + m3 + m4 + 2) >> 2);
          n5 = clip3(m5 - 2 * tc, m5 + 2 * tc, (m3 + m4 + m5 + m6 + 2) >> 2);
          n1 = clip3(m1 - 2 * tc, m1 + 2 * tc, (2 * m0 + 3 * m1 + m2 + m3 + m4 + 4) >> 3);
          n6 = clip3(m6 - 2 * tc, m6 + 2 * tc, (m3 + m4 + m5 + 3 * m6 + 2 * m7 + 4) >> 3);
        } else {
          int delta = (9 * (m4 - m3) - 3 * (m5 - m2) + 8) >> 4;
          if (abs(delta) < cut) {
            delta = clip3(-tc, tc, delta);
            n3 = clip3(0, maxv, m3 + delta);
            n4 = clip3(0, maxv, m4 - delta);
            const int tc2 = tc >> 1;
            if (fp) n2 = clip3(0, maxv, m2 + clip3(-tc2, tc2, ((((m1 + m3 + 1) >> 1) - m2 + delta) >> 1)));
            if (fq) n5 = clip3(0, maxv, m5 + clip3(-tc2, tc2, ((((m6 + m4 + 1) >> 1) - m5 - delta) >> 1)));
          }
        }
        short *pl = s + (ptrdiff_t)l * along;
        if (!pn) pl[-across] = (short)n3, pl[-2 * across] = (short)n2, pl[-3 * across] = (short)n1;
        if (!qn) pl[0] = (short)n4, pl[across] = (short)n5, pl[2 * across] = (short)n6;
      }
    }
  }
  if (b > 1 && !((dir ? uy : ux) & 3)) { // chroma: its own 8x8 grid, strength 2 only (:709-712, :740)
    const int qc = kChromaScale[clip3(0, 51, q_avg)];
    const int tc = kDbkTc[clip3(0, 53, qc + 2 * (b - 1) + (A.toff << 1))] * scale;
#pragma unroll
    for (int p = 1; p < 3; p++) {
      const int st = A.rec.s[p], across = dir ? st : 1, along = dir ? 1 : st;
      short *c0 = A.rec.p[p] + (size_t)(2 * uy) * st + 2 * ux;
#pragma unroll
      for (int k = 0; k < 2; k++) {
        short *s = c0 + (ptrdiff_t)k * along;
        const int m2 = s[-2 * across], m3 = s[-across], m4 = s[0], m5 = s[across];
        const int delta = clip3(-tc, tc, ((((m4 - m3) << 2) + m2 - m5 + 4) >> 3));
        if (!pn) s[-across] = (short)clip3(0, maxv, m3 + delta);
        if (!qn) s[0] = (short)clip3(0, maxv, m4 - delta);
      }
    }
  }
}
// boundary strengths (xGetBoundaryStrengthSingle :444-569): one thread per 4x4 unit, both directions
__device__ __forceinline__ bool dbk_mv_far(const short *a, const short *b) { return abs(a[0] - b[0]) >= 4 || abs(a[1] - b[1]) >= 4; }
__device__ __forceinline__ int dbk_strength(const hmx_dbk_unit &P, const hmx_dbk_unit &Pm, const hmx_dbk_unit &Q, bool tu_edge, bool is_b) {
  if (P.intra || Q.intra) return 2;
  if (tu_edge && (Q.cbf || P.cbf)) return 1;
  if (!is_b) return (Pm.ref[0] != Q.ref[0]) || dbk_mv_far(Pm.mv[0], Q.mv[0]);
  const int p0 = Pm.ref[0] < 0 ? -1 : Pm.ref[0], p1 = Pm.ref[1] < 0 ? -1 : Pm.ref[1];
  const int q0 = Q.ref[0] < 0 ? -1 : Q.ref[0], q1 = Q.ref[1] < 0 ? -1 : Q.ref[1];
  if (!((p0 == q0 && p1 == q1) || (p0 == q1 && p1 == q0))) return 1;
  if (p0 != p1) {
    if (p0 == q0) return dbk_mv_far(Pm.mv[0], Q.mv[0]) || dbk_mv_far(Pm.mv[1], Q.mv[1]);
    return dbk_mv_far(Pm.mv[0], Q.mv[1]) || dbk_mv_far(Pm.mv[1], Q.mv[0]);
  }
  return (dbk_mv_far(Pm.mv[0], Q.mv[1]) || dbk_mv_far(Pm.mv[1], Q.mv[0])) && (dbk_mv_far(Pm.mv[0], Q.mv[0]) || dbk_mv_far(Pm.mv[1], Q.mv[1]));
}
__global__ __launch_bounds__(256) void k_dbk_strengths(const hmx_dbk_unit *units, const unsigned char *edge_ver, const unsigned char *edge_hor,
                                                       int uw, int uh, int ctu, int is_b, unsigned char *bs_ver, unsigned char *bs_hor) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= uw * uh) return;
  const int ux = u % uw, uy = u / uw;
  const hmx_dbk_unit Q = units[u];
  int bv = 0, bh = 0;
  if ((edge_ver[u] & 1) && !(ux & 1) && ux) {
    const hmx_dbk_unit P = units[u - 1];
    bv = dbk_strength(P, P, Q, (edge_ver[u] >> 1) & 1, is_b);
  }
  if ((edge_hor[u] & 1) && !(uy & 1) && uy) {
    const int up = u - uw;
    int um = up;
    if ((4 * uy) % ctu == 0) um = up - ux + (ux & ~3) + ((ux & 3) < 2 ? 0 : 3); // compressed motion of the CTU row above: [0 0 3 3]
    bh = dbk_strength(units[up], units[um], Q, (edge_hor[u] >> 1) & 1, is_b);
  }
  bs_ver[u] = (unsigned char)bv;
  bs_hor[u] = (unsigned char)bh;
}
extern "C" int hmx_deblock_strengths(hmx_ctx *c, const hmx_dbk_unit *d_units, const uint8_t *d_edge_ver, const uint8_t *d_edge_hor, int pic_w,
                                     int pic_h, int is_b_slice, uint8_t *d_bs_ver, uint8_t *d_bs_hor) {
  if (!c || !d_units || !d_edge_ver || !d_edge_hor || !d_bs_ver || !d_bs_hor || pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7))
    return fail(c, HMX_ERR_ARG, "hmx_deblock_strengths: null argument or picture size not a multiple of 8");
  const int uw = pic_w / 4, uh = pic_h / 4;
  hipLaunchKernelGGL(k_dbk_strengths, dim3((unsigned)(((size_t)uw * uh + 255) / 256)), dim3(256), 0, c->stream, d_units, d_edge_ver, d_edge_hor,
                     uw, uh, c->cfg.ctu_size, is_b_slice, d_bs_ver, d_bs_hor);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

extern "C" int hmx_deblock_picture(hmx_ctx *c, const hmx_pic *rec, int pic_w, int pic_h, const uint8_t *d_bs_ver, const uint8_t *d_bs_hor,
                                   const int8_t *d_qp, const uint8_t *d_no_filter, int beta_offset_div2, int tc_offset_div2) {
  if (!c || !rec || !d_bs_ver || !d_bs_hor || !d_qp || pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7))
    return fail(c, HMX_ERR_ARG, "hmx_deblock_picture: null argument or picture size not a multiple of 8");
  DbkArgs A{to_dev(rec), nullptr, d_qp, d_no_filter, pic_w / 4, pic_h / 4, 0, c->cfg.bit_depth, beta_offset_div2, tc_offset_div2};
  const unsigned blocks = (unsigned)(((size_t)A.uw * A.uh + 255) / 256);
  for (int dir = 0; dir < 2; dir++) {
    A.dir = dir;
    A.bs = dir ? d_bs_hor : d_bs_ver;
    hipLaunchKernelGGL(k_deblock, dim3(blocks), dim3(256), 0, c->stream, A);
  }
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

// ---- sample adaptive offset, application (TLibCommon/TComSampleAdaptiveOffset.cpp:781-1240) ----
// The reference filters in place, CTU by CTU, with line buffers that keep the unfiltered neighbours: the same as one
// pass from `in` to `out`, a thread per sample.
// A thread filters 8 consecutive samples of a row (a CTU is a multiple of 8 wide in both planes, so they share their
// parameters): three 16-byte loads (the row, the rows above and below) and the six samples just outside, one 16-byte store.
typedef short s8v __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void k_sao(PlanesDev in, PlanesDev out, int pic_w, int pic_h, int B, int ctu, const hmx_sao_lcu *prm, int n_lcu) {
  const int p = blockIdx.y, sh = p ? 1 : 0, w = pic_w >> sh, h = pic_h >> sh, cs = ctu >> sh, w8 = (w + 7) >> 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w8 * h) return;
  const int x0 = (i % w8) << 3, y = i / w8, cw = (pic_w + ctu - 1) / ctu;
  const hmx_sao_lcu q = prm[(size_t)p * n_lcu + (y / cs) * cw + x0 / cs];
  // the four offsets in one register, picked by shifts (an indexed copy of the struct would live in scratch)
  const unsigned offs = (unsigned)(unsigned char)q.offset[0] | (unsigned)(unsigned char)q.offset[1] << 8 | (unsigned)(unsigned char)q.offset[2] << 16 |
                        (unsigned)(unsigned char)q.offset[3] << 24;
  const short *s = in.p[p];
  const int st = in.s[p], maxv = (1 << B) - 1, up = B - min(B, 10), n = min(8, w - x0);
  short *d = out.p[p] + (size_t)y * out.s[p] + x0;
  // rows y-1, y, y+1 at x0-1 .. x0+8 (clamped addresses; out-of-picture neighbours are excluded by the tests below)
  int r[3][10];
  const bool vec = n == 8 && (((uintptr_t)(s + (size_t)y * st + x0) | (uintptr_t)(2 * st)) & 15) == 0;
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int yy = min(max(y + j - 1, 0), h - 1);
    const short *row = s + (size_t)yy * st;
    if (vec) {
      const s8v v = *reinterpret_cast<const s8v *>(row + x0);
#pragma unroll
      for (int k = 0; k < 8; k++) r[j][k + 1] = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) r[j][k + 1] = row[min(x0 + k, w - 1)];
    }
    r[j][0] = row[max(x0 - 1, 0)];
    r[j][9] = row[min(x0 + 8, w - 1)];
  }
  int v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int x = x0 + k, c = r[1][k + 1];
    int o = c;
    if (q.type >= 0 && q.type < 4) {
      const int dx = q.type == 1 ? 0 : (q.type == 3 ? -1 : 1), dy = q.type == 0 ? 0 : 1; // b = c + d, a = c - d
      if (x - dx >= 0 && x - dx < w && y - dy >= 0 && x + dx >= 0 && x + dx < w && y + dy < h) {
        // select the neighbours from the register rows (dx, dy are uniform over the thread's samples)
        const int a = dy ? (dx == 0 ? r[0][k + 1] : (dx > 0 ? r[0][k] : r[0][k + 2])) : r[1][k];
        const int bb = dy ? (dx == 0 ? r[2][k + 1] : (dx > 0 ? r[2][k + 2] : r[2][k])) : r[1][k + 2];
        const int e = ((c > a) - (c < a)) + ((c > bb) - (c < bb)) + 2; // 0..4; m_auiEoTable {1, 2, 0, 3, 4} picks the offset
        const int slot = e == 2 ? 0 : (e < 2 ? e + 1 : e);
        if (slot) o = clip3(0, maxv, c + ((int)(signed char)(offs >> (8 * (slot - 1))) << up));
      }
    } else if (q.type == 4) {
      const int kk = ((c >> (B - 5)) - q.band) & 31;
      if (kk < 4) o = clip3(0, maxv, c + ((int)(signed char)(offs >> (8 * kk)) << up));
    }
    v[k] = o;
  }
  if (n == 8 && (((uintptr_t)d) & 15) == 0) {
    s8v ov;
#pragma unroll
    for (int k = 0; k < 8; k++) ov[k] = (short)v[k];
    *reinterpret_cast<s8v *>(d) = ov;
  } else {
    for (int k = 0; k < n; k++) d[k] = (short)v[k];
  }
}
extern "C" int hmx_sao_picture(hmx_ctx *c, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h, const hmx_sao_lcu *d_params, int n_lcu) {
  const int ctu = c ? c->cfg.ctu_size : 64;
  if (!c || !in || !out || !d_params || pic_w <= 0 || pic_h <= 0 || (pic_w & 1) || (pic_h & 1) ||
      n_lcu != ((pic_w + ctu - 1) / ctu) * ((pic_h + ctu - 1) / ctu))
    return fail(c, HMX_ERR_ARG, "hmx_sao_picture: bad argument (n_lcu must be the CTU count of the picture)");
  for (int p = 0; p < 3; p++)
    if (in->plane[p] == out->plane[p]) return fail(c, HMX_ERR_ARG, "hmx_sao_picture: in and out must be different pictures");
  hipLaunchKernelGGL(k_sao, dim3((unsigned)(((size_t)((pic_w + 7) / 8) * pic_h + 255) / 256), 3), dim3(256), 0, c->stream, to_dev(in), to_dev(out), pic_w, pic_h,
                     c->cfg.bit_depth, ctu, d_params, n_lcu);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

// ---- SAO statistics of the encoder (TLibEncoder/TEncSampleAdaptiveOffset.cpp:859-1124, calcSaoStatsCuOrg, SAO_SKIP_RIGHT) ----
// One workgroup per (CTU, component, picture), ending in plain stores of its 52 bins.  A thread owns a strip of 8 columns
// and `rows` rows of the CTU and walks it downwards with the rows above and below in registers: every sign of a neighbour
// difference is formed once and serves the samples on both sides of it (what the reference's m_iUpBuff1 does incrementally).
// Edge classes, per type: s = sign(c - a) + sign(c - b) in -2..2.  Counts go to 6-bit fields of one register (field s + 2; a
// sample outside the type's range goes to bits 30-31, never read; a thread sees at most 32 samples).  Diffs go to the five
// moments M_j = sum(diff * s^j), j = 0..4, from which the five class sums follow exactly at the end (sao_stats_solve).
// Band classes: a per-wave LDS histogram of (count << 40) + diff in 64 bits.
constexpr int kSaoStatThreads = 128;
struct SaoStatArgs {
  const PlanesDev *pics; // [n_pics] originals, then [n_pics] reconstructions
  hmx_sao_stat *out;
  int n_pics, pic_w, pic_h, ctu, B, lcu_based, n_lcu, cw;
};
__device__ __forceinline__ int sao_sign(int a, int b) { return min(max(a - b, -1), 1); }
// samples x0-1 .. x0+8 of a row into r[0..9] (addresses clamped to the plane; what lies outside is masked off by the ranges)
__device__ __forceinline__ void sao_row(const short *row, int x0, int w, bool vec, int r[10]) {
  if (vec) {
    const s8v v = *reinterpret_cast<const s8v *>(row + x0);
#pragma unroll
    for (int k = 0; k < 8; k++) r[k + 1] = v[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) r[k + 1] = row[min(x0 + k, w - 1)];
  }
  r[0] = row[max(x0 - 1, 0)];
  r[9] = row[min(x0 + 8, w - 1)];
}
// signs of a row against the row below: d1[i] = sign(c_i - below_i) (i = 1..8), d2[i] = sign(c_i - below_{i+1}) (0..8),
// d3[i] = sign(c_i - below_{i-1}) (1..9); i indexes r[] (i = 1 is column x0)
__device__ __forceinline__ void sao_vsigns(const int u[10], const int l[10], int d1[10], int d2[10], int d3[10]) {
#pragma unroll
  for (int i = 0; i < 10; i++) {
    d1[i] = i >= 1 && i <= 8 ? sao_sign(u[i], l[i]) : 0;
    d2[i] = i <= 8 ? sao_sign(u[i], l[i + 1]) : 0;
    d3[i] = i >= 1 ? sao_sign(u[i], l[i - 1]) : 0;
  }
}
// bits k of the 8 columns x0 + k that lie in [lo, hi)
__device__ __forceinline__ unsigned sao_xmask(int lo, int hi, int x0) {
  lo = min(max(lo - x0, 0), 8), hi = min(max(hi - x0, 0), 8);
  return ((1u << hi) - 1) & ~((1u << lo) - 1);
}
__device__ __forceinline__ void sao_acc(int m[5], unsigned &cnt, bool ok, int s, int diff) {
  const int dm = ok ? diff : 0, s2 = __mul24(s, s);
  cnt += 1u << (ok ? __mul24(s + 2, 6) : 30);
  m[0] += dm;
  m[1] += __mul24(dm, s);
  m[2] += __mul24(dm, s2);
  m[3] += __mul24(dm, __mul24(s2, s));
  m[4] += __mul24(dm, __mul24(s2, s2));
}
// class sums D_s (s = -2..2) from M_j = sum_s D_s s^j: with P_k = D_k + D_-k, Q_k = D_k - D_-k, M2 = P1 + 4 P2, M4 = P1 + 16 P2,
// M1 = Q1 + 2 Q2, M3 = Q1 + 8 Q2, M0 = D0 + P1 + P2 (every division is exact)
__device__ __forceinline__ void sao_stats_solve(const int M[5], int D[5]) {
  const int P2 = (M[4] - M[2]) / 12, P1 = M[2] - 4 * P2, Q2 = (M[3] - M[1]) / 6, Q1 = M[1] - 2 * Q2;
  D[0] = (P2 - Q2) / 2, D[1] = (P1 - Q1) / 2, D[2] = M[0] - P1 - P2, D[3] = (P1 + Q1) / 2, D[4] = (P2 + Q2) / 2;
}
__global__ __launch_bounds__(kSaoStatThreads) void k_sao_stats(SaoStatArgs A) {
  constexpr int kWaves = kSaoStatThreads / 64;
  __shared__ unsigned long long hist[kWaves][32];
  __shared__ int part[kWaves][40];
  const int lcu = blockIdx.x, p = blockIdx.y, pic = blockIdx.z, t = threadIdx.x, wave = t >> 6;
  for (int i = t; i < kWaves * 32; i += kSaoStatThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
  // the CTU in this plane (:898-909) and the ranges of the five passes (CTU-local, end exclusive; include/hmx.h)
  const int sh = p ? 1 : 0, w = A.pic_w >> sh, h = A.pic_h >> sh, cs = A.ctu >> sh;
  const int lx = (lcu % A.cw) * cs, ty = (lcu / A.cw) * cs, W = min(cs, w - lx), H = min(cs, h - ty);
  const bool isL = lx == 0, isT = ty == 0, isR = lx + W == w, isB = ty + H == h;
  const int skip_b = A.lcu_based ? (p ? 2 : 4) : 0, skip_r = A.lcu_based ? (p ? 3 : 5) : 0;
  const int xe_full = isR ? W : W - skip_r, xe_in = isR ? W - 1 : W - skip_r, xs = isL ? 1 : 0;
  const int ye_bo = isB ? H : H - skip_b, ye_eo0 = H - skip_b, ys = isT ? 1 : 0, ye_v = isB ? H - 1 : H - skip_b;
  const int strips = cs >> 3, rows = max(1, cs * strips / kSaoStatThreads);
  const int x0 = (t % strips) * 8, y0 = (t / strips) * rows;
  int mom[4][5] = {};
  unsigned cnt[4] = {0, 0, 0, 0};
  if (x0 < W && y0 < H) {
    const PlanesDev *O = A.pics + pic, *R = A.pics + A.n_pics + pic; // indexed in memory: a copy indexed by p would live in scratch
    const int gx = lx + x0, so = O->s[p], sr = R->s[p], bshift = A.B - 5;
    const short *po = O->p[p] + gx, *pr = R->p[p]; // pr: column 0 of the plane (sao_row indexes it with gx)
    const bool vo = gx + 8 <= w && (((uintptr_t)po | (uintptr_t)(2 * so)) & 15) == 0;
    const bool vr = gx + 8 <= w && (((uintptr_t)(pr + gx) | (uintptr_t)(2 * sr)) & 15) == 0;
    const unsigned m_full = sao_xmask(0, xe_full, x0), m_in = sao_xmask(xs, xe_in, x0);
    int up[10], cur[10], dn[10], u1[10], u2[10], u3[10];
    sao_row(pr + (size_t)max(ty + y0 - 1, 0) * sr, gx, w, vr, up);
    sao_row(pr + (size_t)(ty + y0) * sr, gx, w, vr, cur);
    sao_vsigns(up, cur, u1, u2, u3); // signs of the row above against this one: negated, they are this row's "up" signs
#pragma unroll 1
    for (int j = 0; j < rows; j++) {
      const int y = y0 + j, gy = ty + y;
      if (y >= H) break;
      sao_row(pr + (size_t)min(gy + 1, h - 1) * sr, gx, w, vr, dn);
      int org[8];
      const short *orow = po + (size_t)gy * so;
      if (vo) {
        const s8v v = *reinterpret_cast<const s8v *>(orow);
#pragma unroll
        for (int k = 0; k < 8; k++) org[k] = v[k];
      } else {
#pragma unroll
        for (int k = 0; k < 8; k++) org[k] = orow[min(k, w - 1 - gx)];
      }
      int d1[10], d2[10], d3[10], g[10];
      sao_vsigns(cur, dn, d1, d2, d3);
#pragma unroll
      for (int i = 0; i < 9; i++) g[i] = sao_sign(cur[i], cur[i + 1]); // sign(c_i - right)
      const bool vrow = y >= ys && y < ye_v;
      const unsigned mb = y < ye_bo ? m_full : 0, m0 = y < ye_eo0 ? m_in : 0, m1 = vrow ? m_full : 0, m23 = vrow ? m_in : 0;
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = k + 1, c = cur[i], diff = org[k] - c;
        sao_acc(mom[0], cnt[0], (m0 >> k) & 1, g[i] - g[i - 1], diff);
        sao_acc(mom[1], cnt[1], (m1 >> k) & 1, d1[i] - u1[i], diff);
        sao_acc(mom[2], cnt[2], (m23 >> k) & 1, d2[i] - u2[i - 1], diff);
        sao_acc(mom[3], cnt[3], (m23 >> k) & 1, d3[i] - u3[i + 1], diff);
        if ((mb >> k) & 1) atomicAdd(&hist[wave][(c >> bshift) & 31], (1ull << 40) + (unsigned long long)(long long)diff);
      }
#pragma unroll
      for (int i = 0; i < 10; i++) cur[i] = dn[i], u1[i] = d1[i], u2[i] = d2[i], u3[i] = d3[i];
    }
  }
  // moments and counts summed over the wave, then over the waves
#pragma unroll
  for (int ty4 = 0; ty4 < 4; ty4++) {
#pragma unroll
    for (int j = 0; j < 5; j++) {
      const int m = group_sum(mom[ty4][j], 64), n = group_sum((int)((cnt[ty4] >> (6 * j)) & 63), 64);
      if ((t & 63) == 0) part[wave][10 * ty4 + j] = m, part[wave][10 * ty4 + 5 + j] = n;
    }
  }
  __syncthreads();
  hmx_sao_stat *out = A.out + (((size_t)pic * 3 + p) * A.n_lcu + lcu) * HMX_SAO_STAT_BINS;
  if (t < 32) { // band class t + 1
    unsigned long long v = 0;
#pragma unroll
    for (int q = 0; q < kWaves; q++) v += hist[q][t];
    const long long n = (long long)((v + (1ull << 39)) >> 40);
    out[20 + t] = hmx_sao_stat{(int32_t)((long long)v - (n << 40)), (int32_t)n};
  } else if (t >= 64 && t < 68) { // edge type t - 64: raw class s + 2 -> m_auiEoTable {1, 2, 0, 3, 4}
    const int ty4 = t - 64;
    int M[5], N[5], D[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
      M[j] = 0, N[j] = 0;
#pragma unroll
      for (int q = 0; q < kWaves; q++) M[j] += part[q][10 * ty4 + j], N[j] += part[q][10 * ty4 + 5 + j];
    }
    sao_stats_solve(M, D);
    const int cls[5] = {1, 2, 0, 3, 4};
#pragma unroll
    for (int e = 0; e < 5; e++) out[5 * ty4 + cls[e]] = hmx_sao_stat{D[e], N[e]};
  }
}
extern "C" int hmx_sao_stats_multi(hmx_ctx *c, int n_pics, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h, int lcu_based,
                                   hmx_sao_stat *d_out) {
  if (!c || !org || !rec || !d_out) return fail(c, HMX_ERR_ARG, "hmx_sao_stats_multi: null argument");
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, "hmx_sao_stats_multi: n_pics must be 1..65535");
  if (pic_w <= 0 || pic_h <= 0 || (pic_w & 7) || (pic_h & 7))
    return fail(c, HMX_ERR_ARG, "hmx_sao_stats_multi: picture size must be a positive multiple of 8");
  std::vector<PlanesDev> t(2 * (size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    for (int p = 0; p < 3; p++)
      if (!org[i].plane[p] || !rec[i].plane[p]) return fail(c, HMX_ERR_ARG, "hmx_sao_stats_multi: null plane");
    t[i] = to_dev(&org[i]), t[n_pics + i] = to_dev(&rec[i]);
  }
  const PlanesDev *d = static_cast<const PlanesDev *>(arena_push(c, t.data(), sizeof(PlanesDev) * t.size()));
  if (!d) return fail(c, HMX_ERR_NOMEM, "argument arena");
  const int ctu = c->cfg.ctu_size, cw = (pic_w + ctu - 1) / ctu, n_lcu = cw * ((pic_h + ctu - 1) / ctu);
  SaoStatArgs A{d, d_out, n_pics, pic_w, pic_h, ctu, c->cfg.bit_depth, lcu_based ? 1 : 0, n_lcu, cw};
  hipLaunchKernelGGL(k_sao_stats, dim3((unsigned)n_lcu, 3, (unsigned)n_pics), dim3(kSaoStatThreads), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_sao_stats(hmx_ctx *c, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h, int lcu_based, hmx_sao_stat *d_out) {
  return hmx_sao_stats_multi(c, 1, org, rec, pic_w, pic_h, lcu_based, d_out);
}

// ---- planar 4:2:0 YUV frames (TLibVideoIO/TVideoIOYuv.cpp:226-480) ----
// A frame travels as the bytes of the file (1 or 2 bytes per sample, Y then Cb then Cr): half or a quarter of
// the PCIe traffic of int16 planes; widening, bit-depth scaling and the right/bottom padding happen in HBM.
__device__ __forceinline__ short yuv_rescale(short v, int shift, int bits) { // scalePlane :62-127
  if (shift == 0) return v;
  if (shift > 0) return (short)(v << shift);
  const short r = (short)((v + (short)(1 << (-shift - 1))) >> -shift);
  return (short)min(max((int)r, 0), (1 << bits) - 1);
}
// 8 consecutive samples of a row per thread (16-byte plane accesses when aligned)
struct TiledPic { // the three planes of one resident picture
  TiledPlane T[3];
};
template <bool TILED>
__global__ __launch_bounds__(256) void k_yuv_unpack(const unsigned char *file, int wide, int shift, int bits, int w_full, int h_full,
                                                    int pad_x, int pad_y, PlanesDev D, TiledPic TP) {
  const int p = blockIdx.y, c = p ? 1 : 0;
  const int wf = w_full >> c, hf = h_full >> c, w = wf - (pad_x >> c), h = hf - (pad_y >> c), w8 = (wf + 7) >> 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w8 * hf) return;
  const int x0 = (i % w8) << 3, y = i / w8, sy = min(y, h - 1), n = min(8, wf - x0); // readPlane :226-275: replicate right, then down
  const size_t luma = (size_t)(w_full - pad_x) * (h_full - pad_y), chroma = (size_t)w * h;
  const size_t plane_off = (p == 0 ? 0 : luma + (p == 2 ? chroma : 0)) * (wide ? 2 : 1);
  const unsigned char *row = file + plane_off + (size_t)sy * w * (wide ? 2 : 1);
  short v[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int sx = min(x0 + k, w - 1);
    const short t = wide ? (short)((row[2 * sx + 1] << 8) | row[2 * sx]) : (short)row[sx];
    v[k] = yuv_rescale(t, shift, bits);
  }
  if constexpr (TILED) { // eight samples of a row = one row of two neighbouring tiles (widths are even: n is 2, 4, 6 or 8)
    const TiledPlane T = p == 0 ? TP.T[0] : p == 1 ? TP.T[1] : TP.T[2];
#pragma unroll
    for (int k = 0; k < 8; k += 4) {
      if (k + 4 <= n) {
        s4v o = {v[k], v[k + 1], v[k + 2], v[k + 3]};
        *reinterpret_cast<s4v *>(T.p + taddr(T, x0 + k, y)) = o;
      } else {
        for (int q = k; q < n; q++) T.p[taddr(T, x0 + q, y)] = v[q];
      }
    }
    return;
  }
  short *d = D.p[p] + (size_t)y * D.s[p] + x0;
  if (n == 8 && (((uintptr_t)d) & 15) == 0) {
    s8v ov;
#pragma unroll
    for (int k = 0; k < 8; k++) ov[k] = v[k];
    *reinterpret_cast<s8v *>(d) = ov;
  } else {
    for (int k = 0; k < n; k++) d[k] = v[k];
  }
}
template <bool TILED>
__global__ __launch_bounds__(256) void k_yuv_pack(PlanesDev S, TiledPic TP, int wide, int shift, int bits, int ww, int hh, unsigned char *file) {
  const int p = blockIdx.y, c = p ? 1 : 0, w = ww >> c, h = hh >> c, w8 = (w + 7) >> 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w8 * h) return;
  const int x0 = (i % w8) << 3, y = i / w8, n = min(8, w - x0);
  const size_t luma = (size_t)ww * hh, chroma = (size_t)w * h;
  unsigned char *d = file + ((p == 0 ? 0 : luma + (p == 2 ? chroma : 0)) + (size_t)y * w + x0) * (wide ? 2 : 1);
  const short *s = TILED ? nullptr : S.p[p] + (size_t)y * S.s[p] + x0;
  short v[8];
  if constexpr (TILED) {
    const TiledPlane T = p == 0 ? TP.T[0] : p == 1 ? TP.T[1] : TP.T[2];
#pragma unroll
    for (int k = 0; k < 8; k += 4) {
      if (k + 4 <= n) {
        const s4v iv = *reinterpret_cast<const s4v *>(T.p + taddr(T, x0 + k, y));
        v[k] = iv[0], v[k + 1] = iv[1], v[k + 2] = iv[2], v[k + 3] = iv[3];
      } else {
        for (int q = k; q < k + 4; q++) v[q] = T.p[taddr(T, x0 + min(q, n - 1), y)];
      }
    }
  } else if (n == 8 && (((uintptr_t)s) & 15) == 0) {
    const s8v iv = *reinterpret_cast<const s8v *>(s);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = iv[k];
  } else {
    for (int k = 0; k < 8; k++) v[k] = s[min(k, n - 1)];
  }
#pragma unroll
  for (int k = 0; k < 8; k++) v[k] = yuv_rescale(v[k], shift, bits);
  if (wide) {
    if (n == 8 && (((uintptr_t)d) & 15) == 0) {
      s8v ov;
#pragma unroll
      for (int k = 0; k < 8; k++) ov[k] = v[k]; // little-endian 16-bit samples are the register layout
      *reinterpret_cast<s8v *>(d) = ov;
    } else {
      for (int k = 0; k < n; k++) d[2 * k] = (unsigned char)(v[k] & 0xff), d[2 * k + 1] = (unsigned char)((v[k] >> 8) & 0xff);
    }
  } else {
    if (n == 8 && (((uintptr_t)d) & 7) == 0) {
      unsigned long long o = 0;
#pragma unroll
      for (int k = 0; k < 8; k++) o |= (unsigned long long)(unsigned char)v[k] << (8 * k);
      *reinterpret_cast<unsigned long long *>(d) = o;
    } else {
      for (int k = 0; k < n; k++) d[k] = (unsigned char)v[k];
    }
  }
}
extern "C" size_t hmx_yuv_frame_bytes(int w, int h, int file_bits) { return (size_t)w * h * 3 / 2 * (file_bits > 8 ? 2 : 1); }
extern "C" int hmx_yuv_unpack(hmx_ctx *c, const void *d_file, int file_bits, const hmx_pic *dst, int w_full, int h_full, int pad_x,
                              int pad_y) {
  if (!c || !d_file || !dst || file_bits < 8 || file_bits > 16 || w_full <= 0 || h_full <= 0 || (w_full & 1) || (h_full & 1) ||
      pad_x < 0 || pad_y < 0 || (pad_x & 1) || (pad_y & 1) || pad_x >= w_full || pad_y >= h_full)
    return fail(c, HMX_ERR_ARG, "hmx_yuv_unpack: bad argument");
  hipLaunchKernelGGL(k_yuv_unpack<false>, dim3((unsigned)(((size_t)((w_full + 7) / 8) * h_full + 255) / 256), 3), dim3(256), 0, c->stream,
                     static_cast<const unsigned char *>(d_file), file_bits > 8 ? 1 : 0, c->cfg.bit_depth - file_bits, c->cfg.bit_depth,
                     w_full, h_full, pad_x, pad_y, to_dev(dst), TiledPic{});
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_yuv_pack(hmx_ctx *c, const hmx_pic *src, int w, int h, int crop_right, int crop_bottom, int file_bits, void *d_file) {
  if (!c || !d_file || !src || file_bits < 8 || file_bits > 16 || crop_right < 0 || crop_bottom < 0 || crop_right >= w ||
      crop_bottom >= h || ((w - crop_right) & 1) || ((h - crop_bottom) & 1))
    return fail(c, HMX_ERR_ARG, "hmx_yuv_pack: bad argument");
  const int ww = w - crop_right, hh = h - crop_bottom;
  hipLaunchKernelGGL(k_yuv_pack<false>, dim3((unsigned)(((size_t)((ww + 7) / 8) * hh + 255) / 256), 3), dim3(256), 0, c->stream, to_dev(src),
                     TiledPic{}, file_bits > 8 ? 1 : 0, file_bits - c->cfg.bit_depth, file_bits, ww, hh, static_cast<unsigned char *>(d_file));
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
// The same straight into / out of a resident picture: the frame crosses PCIe as file bytes and is widened, scaled, padded and
// laid out for the block kernels in ONE pass over it; no plane-geometry copy exists on the device.
extern "C" int hmx_yuv_unpack_resident(hmx_ctx *c, const void *d_file, int file_bits, hmx_tpool *t, int index, int pad_x, int pad_y) {
  if (!c || !d_file || !t || index < 0 || index >= t->n_pics || file_bits < 8 || file_bits > 16 || (t->pic_w & 1) || (t->pic_h & 1) || pad_x < 0 ||
      pad_y < 0 || (pad_x & 1) || (pad_y & 1) || pad_x >= t->pic_w || pad_y >= t->pic_h)
    return fail(c, HMX_ERR_ARG, "hmx_yuv_unpack_resident: bad argument");
  TiledPic TP;
  for (int p = 0; p < 3; p++) TP.T[p] = tpool_plane(t, index, p);
  hipLaunchKernelGGL(k_yuv_unpack<true>, dim3((unsigned)(((size_t)((t->pic_w + 7) / 8) * t->pic_h + 255) / 256), 3), dim3(256), 0, c->stream,
                     static_cast<const unsigned char *>(d_file), file_bits > 8 ? 1 : 0, c->cfg.bit_depth - file_bits, c->cfg.bit_depth,
                     t->pic_w, t->pic_h, pad_x, pad_y, PlanesDev{}, TP);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_yuv_pack_resident(hmx_ctx *c, const hmx_tpool *t, int index, int crop_right, int crop_bottom, int file_bits, void *d_file) {
  if (!c || !d_file || !t || index < 0 || index >= t->n_pics || file_bits < 8 || file_bits > 16 || crop_right < 0 || crop_bottom < 0 ||
      crop_right >= t->pic_w || crop_bottom >= t->pic_h || ((t->pic_w - crop_right) & 1) || ((t->pic_h - crop_bottom) & 1))
    return fail(c, HMX_ERR_ARG, "hmx_yuv_pack_resident: bad argument");
  const int ww = t->pic_w - crop_right, hh = t->pic_h - crop_bottom;
  TiledPic TP;
  for (int p = 0; p < 3; p++) TP.T[p] = tpool_plane(t, index, p);
  hipLaunchKernelGGL(k_yuv_pack<true>, dim3((unsigned)(((size_t)((ww + 7) / 8) * hh + 255) / 256), 3), dim3(256), 0, c->stream, PlanesDev{}, TP,
                     file_bits > 8 ? 1 : 0, file_bits - c->cfg.bit_depth, file_bits, ww, hh, static_cast<unsigned char *>(d_file));
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

extern "C" void hmx_clipMv(int *mvx, int *mvy, int cu_x, int cu_y, int pic_w, int pic_h, int ctu) {
  const int hmax = (pic_w + 8 - cu_x - 1) << 2, hmin = (-ctu - 8 - cu_x + 1) * 4; // TComDataCU.cpp:3505-3517
  const int vmax = (pic_h + 8 - cu_y - 1) << 2, vmin = (-ctu - 8 - cu_y + 1) * 4;
  *mvx = std::min(hmax, std::max(hmin, *mvx));
  *mvy = std::min(vmax, std::max(vmin, *mvy));
}

