// hmx_loop.hip: deblocking and SAO (application), YUV file formats -- part of libhmx (include/hmx.h), gfx950.  See hmx_host.h for how the library is cut into translation units.
#include "hmx_host.h"

// ---- deblocking filter, application part (TLibCommon/TComLoopFilter.cpp:571-922) ----
// One launch per batch, grid = (windows of a picture, pictures); both directions in one pass through LDS (loopFilterPic
// :153-201 filters every vertical edge of the picture before the first horizontal one).  A workgroup owns the 64x64 luma
// window [x0-4, x0+60) x [y0-4, y0+60) clipped to the picture and the 32x32 windows of Cb and Cr at (x0/2-2, y0/2-2).  Edges
// are 8 samples apart and a luma filter reads 4 and writes 3 samples per side (chroma: reads 2, writes 1), so with that shift
// every edge of the 8x8 grid inside a window has its whole support inside it, and a horizontal edge reads only samples whose
// vertical-edge filtering (decided per 4 lines, and the window starts on a multiple of 4) happened in the same window.  The
// windows of a picture are disjoint and cover it: the picture is read once and written once, in place, with no halo.
//   load -> vertical edges in LDS -> barrier -> horizontal edges -> barrier -> store
// Work item of a direction = one 4x4 luma unit whose left (top) side is an edge of the 8x8 grid with a non-zero strength:
// its four luma lines (threads 0..127: 8 edges x 16 segments of a window) or, on the chroma grid with strength 2, its two lines
// of Cb or Cr (threads 128..255: 2 planes x 4 edges x 16 segments).
// LDS rows: luma pitch 72 shorts (144 B), chroma 40 (80 B).  Vertical luma edges are read with one 16-byte access per line at
// row * 144 + 16 * edge: four lines are 576 = 64 mod 256 bytes apart, and with edge = lane & 3 (+ 4 * wave), segment =
// lane >> 2 each of the hardware's 16-lane groups of that access covers all 64 banks once.  Horizontal luma edges read 8 bytes
// per row at row * 144 + 8 * segment: two edges (8 rows = 1152 = 128 mod 256 bytes apart) x 16 segments fill the banks of a
// 32-lane group once.  (A pitch of 64 shorts puts every row of a column on one bank.)  Chroma: the vertical pass is
// conflict-free at pitch 40 (2 rows = 160 B, 4 edges x 16 B); its horizontal pass reads dwords 2-way (8 rows = 640 B = 0 mod 128).
typedef short s8v __attribute__((ext_vector_type(8)));
static __constant__ unsigned char kDbkTc[54] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                         2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24};
static __constant__ unsigned char kDbkBeta[52] = {0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  0,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15,
                                           16, 17, 18, 20, 22, 24, 26, 28, 30, 32, 34, 36, 38, 40, 42, 44, 46, 48, 50, 52, 54, 56, 58, 60, 62, 64};
static __constant__ unsigned char kChromaScale[58] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18, 19,
                                               20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32, 33, 33, 34, 34, 35, 35,
                                               36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51};
constexpr int kDbkLumaPitch = 72, kDbkChromaPitch = 40; // shorts
constexpr int kDbkLumaChunks = 9, kDbkChromaChunks = 5; // aligned 8-sample runs of the picture that a window row touches
struct DbkPic { // one picture of the batch (in the argument arena)
  PlanesDev rec;
  int boff, toff;
};
struct DbkArgs {
  const DbkPic *pics;                   // [n_pics]
  const unsigned char *bs_ver, *bs_hor; // [pic][unit]
  const signed char *qp;
  const unsigned char *no_filter; // or null
  int w, h, uw, uh, tiles_x, B;
};
struct DbkUnit { // what an edge segment takes from the maps
  int b, q_avg;
  bool pn, qn;
};
__device__ __forceinline__ DbkUnit dbk_unit(const DbkArgs &A, const unsigned char *bs, size_t base, int u, int up) {
  DbkUnit e;
  e.b = bs[base + u];
  e.pn = A.no_filter && A.no_filter[base + up], e.qn = A.no_filter && A.no_filter[base + u];
  e.q_avg = ((int)A.qp[base + up] + (int)A.qp[base + u] + 1) >> 1;
  return e;
}
// four lines across a luma edge, m[l][0..3] the P side and m[l][4..7] the Q side (xEdgeFilterLuma :626-700, xPelFilterLuma
// :780-850), filtered in the registers; false = the edge stays as it is
__device__ __forceinline__ bool dbk_luma(int m[4][8], const DbkUnit &e, int boff, int toff, int B) {
  const int scale = 1 << (B - 8), maxv = (1 << B) - 1;
  const int tc = kDbkTc[clip3(0, 53, e.q_avg + 2 * (e.b - 1) + (toff << 1))] * scale;
  const int beta = kDbkBeta[clip3(0, 51, e.q_avg + (boff << 1))] * scale;
  const int side = (beta + (beta >> 1)) >> 3, cut = tc * 10;
  const int dp0 = abs(m[0][1] - 2 * m[0][2] + m[0][3]), dq0 = abs(m[0][4] - 2 * m[0][5] + m[0][6]);
  const int dp3 = abs(m[3][1] - 2 * m[3][2] + m[3][3]), dq3 = abs(m[3][4] - 2 * m[3][5] + m[3][6]);
  const int d0 = dp0 + dq0, d3 = dp3 + dq3, dp = dp0 + dp3, dq = dq0 + dq3, d = d0 + d3;
  if (d >= beta) return false;
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
    if (!e.pn) m[l][3] = n3, m[l][2] = n2, m[l][1] = n1;
    if (!e.qn) m[l][4] = n4, m[l][5] = n5, m[l][6] = n6;
  }
  return true;
}
// tc of a chroma edge: its own 8x8 grid, strength 2 only (:709-712, :740); one line m2 m3 | m4 m5 (xPelFilterChroma :861-878)
__device__ __forceinline__ int dbk_chroma_tc(const DbkUnit &e, int toff, int B) {
  const int qc = kChromaScale[clip3(0, 51, e.q_avg)];
  return kDbkTc[clip3(0, 53, qc + 2 * (e.b - 1) + (toff << 1))] * (1 << (B - 8));
}
__device__ __forceinline__ void dbk_chroma(int m2, int &m3, int &m4, int m5, const DbkUnit &e, int tc, int B) {
  const int maxv = (1 << B) - 1;
  const int delta = clip3(-tc, tc, ((((m4 - m3) << 2) + m2 - m5 + 4) >> 3));
  const int n3 = clip3(0, maxv, m3 + delta), n4 = clip3(0, maxv, m4 - delta);
  if (!e.pn) m3 = n3;
  if (!e.qn) m4 = n4;
}
// The run of 8 samples number i of a workgroup's three windows: luma 64 rows x 9 runs, then Cb and Cr 32 rows x 5 runs each.
// A run starts on a multiple of 8 of the plane (16-byte accesses on aligned planes); the window starts 4 (chroma: 6) samples
// into the first run and ends 4 (6) samples into the last.
constexpr int kDbkRuns = 64 * kDbkLumaChunks + 2 * 32 * kDbkChromaChunks;
struct DbkRun {
  short *g;   // the run in the plane, or null when no sample of it is in the window
  short *lds; // where sample 0 of the run would go (it may lie before the row: lo says where the window begins)
  int lo, hi; // samples [lo, hi) of the run are in the window and the plane (even)
  bool vec;   // the whole run is in the plane and 16-byte aligned
};
__device__ __forceinline__ DbkRun dbk_run(const DbkArgs &A, const PlanesDev *R, int i, int x0, int y0, short *sy, short *sc) {
  int p = 0, r, j;
  if (i < 64 * kDbkLumaChunks) {
    r = i / kDbkLumaChunks, j = i - r * kDbkLumaChunks;
  } else {
    int k = i - 64 * kDbkLumaChunks;
    p = 1 + k / (32 * kDbkChromaChunks), k -= (p - 1) * (32 * kDbkChromaChunks);
    r = k / kDbkChromaChunks, j = k - r * kDbkChromaChunks;
  }
  const int sh = p ? 1 : 0, off = 4 >> sh, ws = 64 >> sh, w = A.w >> sh, h = A.h >> sh;
  const int y = (y0 >> sh) - off + r, xa = (x0 >> sh) - 8 + 8 * j, col0 = 8 * j - 8 + off; // window column of sample 0
  DbkRun q;
  q.g = nullptr;
  q.lo = max(0, -col0), q.hi = min(min(8, ws - col0), w - xa);
  if (y < 0 || y >= h || xa < 0 || q.lo >= q.hi) return q;
  const int st = R->s[p]; // indexed in memory: a copy indexed by p would live in scratch
  q.g = R->p[p] + (size_t)y * st + xa;
  q.lds = (p == 0 ? sy + r * kDbkLumaPitch : sc + ((p - 1) * 32 + r) * kDbkChromaPitch) + col0;
  q.vec = xa + 8 <= w && (((uintptr_t)q.g | (uintptr_t)(2 * st)) & 15) == 0;
  return q;
}
__global__ __launch_bounds__(256) void k_deblock(DbkArgs A) {
  __shared__ __attribute__((aligned(16))) short sy[64 * kDbkLumaPitch];
  __shared__ __attribute__((aligned(16))) short sc[2 * 32 * kDbkChromaPitch];
  const int t = threadIdx.x, pic = blockIdx.y;
  const int x0 = (blockIdx.x % A.tiles_x) * 64, y0 = (blockIdx.x / A.tiles_x) * 64;
  const DbkPic *P = A.pics + pic;
  const PlanesDev *R = &P->rec;
  const int boff = P->boff, toff = P->toff, B = A.B, uw = A.uw;
  const size_t base = (size_t)pic * uw * A.uh;
  for (int i = t; i < kDbkRuns; i += 256) { // the windows into LDS
    const DbkRun q = dbk_run(A, R, i, x0, y0, sy, sc);
    if (!q.g) continue;
    short v[8];
    if (q.vec) {
      const s8v iv = *reinterpret_cast<const s8v *>(q.g);
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = iv[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; k++) v[k] = q.g[min(k, q.hi - 1)];
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2)
      if (k >= q.lo && k < q.hi) *reinterpret_cast<unsigned *>(q.lds + k) = (unsigned)(unsigned short)v[k] | (unsigned)(unsigned short)v[k + 1] << 16;
  }
  __syncthreads();
#pragma unroll 1
  for (int dir = 0; dir < 2; dir++) {
    const unsigned char *bs = dir ? A.bs_hor : A.bs_ver;
    if (t < 128) {
      // vertical: edge column x0 + 8e = window column 4 + 8e, lines 4 seg ..; horizontal: edge row y0 + 8e, columns 4 seg ..
      const int e = dir ? t >> 4 : (t & 3) | ((t >> 6) << 2), seg = dir ? t & 15 : (t >> 2) & 15;
      const int x = dir ? x0 - 4 + 4 * seg : x0 + 8 * e, y = dir ? y0 + 8 * e : y0 - 4 + 4 * seg;
      if (x >= 0 && x < A.w && y >= 0 && y < A.h && (dir ? y : x) > 0) {
        const int u = (y >> 2) * uw + (x >> 2);
        const DbkUnit E = dbk_unit(A, bs, base, u, dir ? u - uw : u - 1);
        if (E.b) {
          int m[4][8];
          if (!dir) {
            short *s = sy + (4 * seg) * kDbkLumaPitch + 8 * e;
#pragma unroll
            for (int l = 0; l < 4; l++) {
              const s8v v = *reinterpret_cast<const s8v *>(s + l * kDbkLumaPitch);
#pragma unroll
              for (int k = 0; k < 8; k++) m[l][k] = v[k];
            }
            if (dbk_luma(m, E, boff, toff, B)) {
#pragma unroll
              for (int l = 0; l < 4; l++) {
                s8v v;
#pragma unroll
                for (int k = 0; k < 8; k++) v[k] = (short)m[l][k];
                *reinterpret_cast<s8v *>(s + l * kDbkLumaPitch) = v;
              }
            }
          } else {
            short *s = sy + (8 * e) * kDbkLumaPitch + 4 * seg;
#pragma unroll
            for (int k = 0; k < 8; k++) {
              const s4v v = *reinterpret_cast<const s4v *>(s + k * kDbkLumaPitch);
#pragma unroll
              for (int l = 0; l < 4; l++) m[l][k] = v[l];
            }
            if (dbk_luma(m, E, boff, toff, B)) {
#pragma unroll
              for (int k = 1; k < 7; k++) {
                s4v v;
#pragma unroll
                for (int l = 0; l < 4; l++) v[l] = (short)m[l][k];
                *reinterpret_cast<s4v *>(s + k * kDbkLumaPitch) = v;
              }
            }
          }
        }
      }
    } else {
      // chroma, in chroma samples: vertical edge column x0/2 + 8e = window column 2 + 8e, lines 2 seg, 2 seg + 1; horizontal
      // edge row y0/2 + 8e, columns 2 seg, 2 seg + 1
      const int c = t - 128, i = c & 63;
      short *pl = sc + (c >> 6) * 32 * kDbkChromaPitch;
      const int e = dir ? i >> 4 : i & 3, seg = dir ? i & 15 : i >> 2;
      const int x = dir ? (x0 >> 1) - 2 + 2 * seg : (x0 >> 1) + 8 * e, y = dir ? (y0 >> 1) + 8 * e : (y0 >> 1) - 2 + 2 * seg;
      if (x >= 0 && x < (A.w >> 1) && y >= 0 && y < (A.h >> 1) && (dir ? y : x) > 0) {
        const int u = (y >> 1) * uw + (x >> 1);
        const DbkUnit E = dbk_unit(A, bs, base, u, dir ? u - uw : u - 1);
        if (E.b > 1) {
          const int tc = dbk_chroma_tc(E, toff, B);
          if (!dir) {
            short *s = pl + (2 * seg) * kDbkChromaPitch + 8 * e;
#pragma unroll
            for (int k = 0; k < 2; k++) {
              s4v v = *reinterpret_cast<const s4v *>(s + k * kDbkChromaPitch);
              int m3 = v[1], m4 = v[2];
              dbk_chroma(v[0], m3, m4, v[3], E, tc, B);
              v[1] = (short)m3, v[2] = (short)m4;
              *reinterpret_cast<s4v *>(s + k * kDbkChromaPitch) = v;
            }
          } else {
            short *s = pl + (8 * e) * kDbkChromaPitch + 2 * seg;
            unsigned r[4];
#pragma unroll
            for (int j = 0; j < 4; j++) r[j] = *reinterpret_cast<const unsigned *>(s + j * kDbkChromaPitch);
            unsigned o3 = 0, o4 = 0;
#pragma unroll
            for (int k = 0; k < 2; k++) {
              int m3 = (short)(r[1] >> (16 * k)), m4 = (short)(r[2] >> (16 * k));
              dbk_chroma((short)(r[0] >> (16 * k)), m3, m4, (short)(r[3] >> (16 * k)), E, tc, B);
              o3 |= (unsigned)(unsigned short)m3 << (16 * k), o4 |= (unsigned)(unsigned short)m4 << (16 * k);
            }
            *reinterpret_cast<unsigned *>(s + kDbkChromaPitch) = o3;
            *reinterpret_cast<unsigned *>(s + 2 * kDbkChromaPitch) = o4;
          }
        }
      }
    }
    __syncthreads();
  }
  for (int i = t; i < kDbkRuns; i += 256) { // and back: whole runs with one 16-byte store, the cut ones by dwords or samples
    const DbkRun q = dbk_run(A, R, i, x0, y0, sy, sc);
    if (!q.g) continue;
    unsigned v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = (2 * k >= q.lo && 2 * k < q.hi) ? *reinterpret_cast<const unsigned *>(q.lds + 2 * k) : 0;
    if (q.vec && q.lo == 0 && q.hi == 8) {
      typedef unsigned u4v __attribute__((ext_vector_type(4)));
      const u4v ov = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<u4v *>(q.g) = ov;
    } else if ((((uintptr_t)q.g) & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (2 * k >= q.lo && 2 * k < q.hi) *reinterpret_cast<unsigned *>(q.g + 2 * k) = v[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (2 * k >= q.lo && 2 * k < q.hi) q.g[2 * k] = (short)(v[k] & 0xffff), q.g[2 * k + 1] = (short)(v[k] >> 16);
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
                                                       int uw, int uh, int ctu, const unsigned char *is_b_pic, unsigned char *bs_ver,
                                                       unsigned char *bs_hor) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x, pic = blockIdx.y;
  if (u >= uw * uh) return;
  const size_t base = (size_t)pic * uw * uh; // the maps of this picture
  units += base, edge_ver += base, edge_hor += base;
  const bool is_b = is_b_pic[pic] != 0;
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
  bs_ver[base + u] = (unsigned char)bv;
  bs_hor[base + u] = (unsigned char)bh;
}
// What the _multi entry points share, with the messages of `fn`, the entry point: the range of n_pics (grid.y or grid.z), the
// picture size (dims_ok, what it has to be in size_rule) ...
static int multi_shape(hmx_ctx *c, const char *fn, int n_pics, bool dims_ok, const char *size_rule) {
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, std::string(fn) + ": n_pics must be 1..65535");
  if (!dims_ok) return fail(c, HMX_ERR_ARG, std::string(fn) + ": " + size_rule);
  return HMX_OK;
}
// ... and the pictures: no null plane in a[] (nor in b[], when there is one; with `distinct` a rule that a[i] and b[i] share none), then
// the table in the argument arena, make(a[i], i) for every picture and behind them make(b[i], i)
template <typename T, typename Make>
static int multi_pics(hmx_ctx *c, const char *fn, int n_pics, bool dims_ok, const char *size_rule, const hmx_pic *a, const hmx_pic *b,
                      const char *distinct, Make make, const T **d) {
  if (int r = multi_shape(c, fn, n_pics, dims_ok, size_rule)) return r;
  std::vector<T> t((b ? 2 : 1) * (size_t)n_pics);
  for (int i = 0; i < n_pics; i++) {
    for (int p = 0; p < 3; p++) {
      if (!a[i].plane[p] || (b && !b[i].plane[p])) return fail(c, HMX_ERR_ARG, std::string(fn) + ": null plane");
      if (b && distinct && a[i].plane[p] == b[i].plane[p]) return fail(c, HMX_ERR_ARG, std::string(fn) + ": " + distinct);
    }
    t[i] = make(a[i], i);
    if (b) t[n_pics + i] = make(b[i], i);
  }
  *d = static_cast<const T *>(arena_push(c, t.data(), sizeof(T) * t.size()));
  return *d ? HMX_OK : fail(c, HMX_ERR_NOMEM, "argument arena");
}
static bool multiple_of(int pic_w, int pic_h, int m) { return pic_w > 0 && pic_h > 0 && pic_w % m == 0 && pic_h % m == 0; }
static const char *const kMultipleOf8 = "picture size must be a positive multiple of 8";
static PlanesDev planes_of(const hmx_pic &p, int) { return to_dev(&p); }

extern "C" int hmx_deblock_strengths_multi(hmx_ctx *c, int n_pics, const hmx_dbk_unit *d_units, const uint8_t *d_edge_ver,
                                           const uint8_t *d_edge_hor, int pic_w, int pic_h, const uint8_t *is_b_slice, uint8_t *d_bs_ver,
                                           uint8_t *d_bs_hor) {
  if (!c || !d_units || !d_edge_ver || !d_edge_hor || !is_b_slice || !d_bs_ver || !d_bs_hor)
    return fail(c, HMX_ERR_ARG, "hmx_deblock_strengths_multi: null argument");
  if (int r = multi_shape(c, "hmx_deblock_strengths_multi", n_pics, multiple_of(pic_w, pic_h, 8), kMultipleOf8)) return r;
  const unsigned char *d_b = static_cast<const unsigned char *>(arena_push(c, is_b_slice, (size_t)n_pics));
  if (!d_b) return fail(c, HMX_ERR_NOMEM, "argument arena");
  const int uw = pic_w / 4, uh = pic_h / 4;
  hipLaunchKernelGGL(k_dbk_strengths, dim3((unsigned)(((size_t)uw * uh + 255) / 256), (unsigned)n_pics), dim3(256), 0, c->stream, d_units,
                     d_edge_ver, d_edge_hor, uw, uh, c->cfg.ctu_size, d_b, d_bs_ver, d_bs_hor);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_deblock_strengths(hmx_ctx *c, const hmx_dbk_unit *d_units, const uint8_t *d_edge_ver, const uint8_t *d_edge_hor, int pic_w,
                                     int pic_h, int is_b_slice, uint8_t *d_bs_ver, uint8_t *d_bs_hor) {
  const uint8_t is_b = is_b_slice ? 1 : 0;
  return hmx_deblock_strengths_multi(c, 1, d_units, d_edge_ver, d_edge_hor, pic_w, pic_h, &is_b, d_bs_ver, d_bs_hor);
}

extern "C" int hmx_deblock_picture_multi(hmx_ctx *c, int n_pics, const hmx_pic *rec, int pic_w, int pic_h, const uint8_t *d_bs_ver,
                                         const uint8_t *d_bs_hor, const int8_t *d_qp, const uint8_t *d_no_filter, const int8_t *beta_offset_div2,
                                         const int8_t *tc_offset_div2) {
  if (!c || !rec || !d_bs_ver || !d_bs_hor || !d_qp) return fail(c, HMX_ERR_ARG, "hmx_deblock_picture_multi: null argument");
  const DbkPic *d;
  const auto entry = [&](const hmx_pic &p, int i) { return DbkPic{to_dev(&p), beta_offset_div2 ? beta_offset_div2[i] : 0, tc_offset_div2 ? tc_offset_div2[i] : 0}; };
  if (int r = multi_pics(c, "hmx_deblock_picture_multi", n_pics, multiple_of(pic_w, pic_h, 8), kMultipleOf8, rec, nullptr, nullptr, entry, &d)) return r;
  const int tiles_x = (pic_w + 4 + 63) / 64, tiles_y = (pic_h + 4 + 63) / 64; // windows start at 64 k - 4
  DbkArgs A{d, d_bs_ver, d_bs_hor, d_qp, d_no_filter, pic_w, pic_h, pic_w / 4, pic_h / 4, tiles_x, c->cfg.bit_depth};
  hipLaunchKernelGGL(k_deblock, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_pics), dim3(256), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_deblock_picture(hmx_ctx *c, const hmx_pic *rec, int pic_w, int pic_h, const uint8_t *d_bs_ver, const uint8_t *d_bs_hor,
                                   const int8_t *d_qp, const uint8_t *d_no_filter, int beta_offset_div2, int tc_offset_div2) {
  const int8_t boff = (int8_t)beta_offset_div2, toff = (int8_t)tc_offset_div2;
  return hmx_deblock_picture_multi(c, 1, rec, pic_w, pic_h, d_bs_ver, d_bs_hor, d_qp, d_no_filter, &boff, &toff);
}

// ---- sample adaptive offset, application (TLibCommon/TComSampleAdaptiveOffset.cpp:781-1240) ----
// The reference filters in place, CTU by CTU, with line buffers that keep the unfiltered neighbours: the same as one
// pass from `in` to `out`, a thread per sample.
// A thread filters 8 consecutive samples of a row (a CTU is a multiple of 8 wide in both planes, so they share their
// parameters): three 16-byte loads (the row, the rows above and below) and the six samples just outside, one 16-byte store.
// pics: [n_pics] inputs, then [n_pics] outputs (in the argument arena); the picture is blockIdx.z
// an availability byte (hmx_lf_border_avail) as the 3x3 CTU neighbourhood in 9 bits, bit (sx + 1) + 3 * (sy + 1) for the CTU at (sx, sy) from this one (the centre is set)
__device__ __forceinline__ unsigned sao_avail9(unsigned m) {
  return ((m >> 4) & 1) | ((m >> 2) & 1) << 1 | ((m >> 5) & 1) << 2 | (m & 1) << 3 | 1u << 4 | ((m >> 1) & 1) << 5 | ((m >> 6) & 1) << 6 |
         ((m >> 3) & 1) << 7 | ((m >> 7) & 1) << 8;
}
// may the sample at CTU-local (x, y) be read from a CTU of W x H samples with the neighbourhood a9?
__device__ __forceinline__ bool sao_may_read(unsigned a9, int x, int y, int W, int H) {
  const int sx = x < 0 ? 0 : (x >= W ? 2 : 1), sy = y < 0 ? 0 : (y >= H ? 2 : 1);
  return (a9 >> (sx + 3 * sy)) & 1;
}
// AVAIL (processSaoBlock :561-776, the path of m_bUseNIF): avail[pic][CTU] says which of the eight neighbour CTUs may be read
// (bit k = SGU_L, R, T, B, TL, TR, BL, BR); an edge-offset sample is filtered when each of its two neighbours lies in its own
// CTU or in a CTU whose bit is set, which takes the place of the in-picture test (a CTU outside the picture has no bit).
template <bool AVAIL>
__global__ __launch_bounds__(256) void k_sao(const PlanesDev *pics, int n_pics, int pic_w, int pic_h, int B, int ctu, const hmx_sao_lcu *prm, int n_lcu,
                                             const uint8_t *avail) {
  const int pic = blockIdx.z;
  const PlanesDev &in = pics[pic], &out = pics[n_pics + pic];
  prm += (size_t)pic * 3 * n_lcu;
  const int p = blockIdx.y, sh = p ? 1 : 0, w = pic_w >> sh, h = pic_h >> sh, cs = ctu >> sh, w8 = (w + 7) >> 3;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w8 * h) return;
  const int x0 = (i % w8) << 3, y = i / w8, cw = (pic_w + ctu - 1) / ctu;
  const hmx_sao_lcu q = prm[(size_t)p * n_lcu + (y / cs) * cw + x0 / cs];
  unsigned a9 = 0;
  int lx0 = 0, ly = 0, W = 0, H = 0; // the thread's first sample in its CTU, and the CTU cut at the picture edge
  if constexpr (AVAIL) {
    a9 = sao_avail9(avail[(size_t)pic * n_lcu + (y / cs) * cw + x0 / cs]);
    lx0 = x0 % cs, ly = y % cs, W = min(cs, w - (x0 - lx0)), H = min(cs, h - (y - ly));
  }
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
      bool both;
      if constexpr (AVAIL) both = sao_may_read(a9, lx0 + k - dx, ly - dy, W, H) && sao_may_read(a9, lx0 + k + dx, ly + dy, W, H);
      else both = x - dx >= 0 && x - dx < w && y - dy >= 0 && x + dx >= 0 && x + dx < w && y + dy < h;
      if (both) {
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
// d_avail: null = the in-picture test (processSaoCuOrg), else the availability path
static int sao_picture_multi(hmx_ctx *c, const char *fn, int n_pics, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h,
                             const hmx_sao_lcu *d_params, int n_lcu, const uint8_t *d_avail) {
  if (!c || !in || !out || !d_params) return fail(c, HMX_ERR_ARG, std::string(fn) + ": null argument");
  const int ctu = c->cfg.ctu_size;
  const bool dims_ok = multiple_of(pic_w, pic_h, 2) && n_lcu == ((pic_w + ctu - 1) / ctu) * ((pic_h + ctu - 1) / ctu);
  const PlanesDev *d;
  if (int r = multi_pics(c, fn, n_pics, dims_ok, "bad size (even, and n_lcu must be the CTU count of the picture)", in, out,
                         "in and out must be different pictures", planes_of, &d))
    return r;
  const dim3 grid((unsigned)(((size_t)((pic_w + 7) / 8) * pic_h + 255) / 256), 3, (unsigned)n_pics);
  if (d_avail) hipLaunchKernelGGL(k_sao<true>, grid, dim3(256), 0, c->stream, d, n_pics, pic_w, pic_h, c->cfg.bit_depth, ctu, d_params, n_lcu, d_avail);
  else hipLaunchKernelGGL(k_sao<false>, grid, dim3(256), 0, c->stream, d, n_pics, pic_w, pic_h, c->cfg.bit_depth, ctu, d_params, n_lcu, d_avail);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_sao_picture_multi(hmx_ctx *c, int n_pics, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h,
                                     const hmx_sao_lcu *d_params, int n_lcu) {
  return sao_picture_multi(c, "hmx_sao_picture_multi", n_pics, in, out, pic_w, pic_h, d_params, n_lcu, nullptr);
}
extern "C" int hmx_sao_picture_multi_avail(hmx_ctx *c, int n_pics, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h,
                                           const hmx_sao_lcu *d_params, int n_lcu, const uint8_t *d_avail) {
  if (!d_avail) return fail(c, HMX_ERR_ARG, "hmx_sao_picture_multi_avail: null argument");
  return sao_picture_multi(c, "hmx_sao_picture_multi_avail", n_pics, in, out, pic_w, pic_h, d_params, n_lcu, d_avail);
}
extern "C" int hmx_sao_picture(hmx_ctx *c, const hmx_pic *in, const hmx_pic *out, int pic_w, int pic_h, const hmx_sao_lcu *d_params, int n_lcu) {
  return hmx_sao_picture_multi(c, 1, in, out, pic_w, pic_h, d_params, n_lcu);
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
  const uint8_t *avail; // [n_pics][n_lcu] for the availability path (calcSaoStatsBlock), unused otherwise
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
// bits k of the 8 columns x0 + k of a CTU row y whose two neighbours at -+(dx, dy) may both be read (calcSaoStatsBlock :571-815)
__device__ __forceinline__ unsigned sao_pair_mask(unsigned a9, int x0, int y, int dx, int dy, int W, int H) {
  unsigned m = 0;
#pragma unroll
  for (int k = 0; k < 8; k++)
    m |= (unsigned)(x0 + k < W && sao_may_read(a9, x0 + k - dx, y - dy, W, H) && sao_may_read(a9, x0 + k + dx, y + dy, W, H)) << k;
  return m;
}
template <bool AVAIL>
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
  unsigned a9 = 0;
  if constexpr (AVAIL) a9 = sao_avail9(A.avail[(size_t)pic * A.n_lcu + lcu]);
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
      unsigned mb = y < ye_bo ? m_full : 0, m0 = y < ye_eo0 ? m_in : 0, m1 = vrow ? m_full : 0, m2 = vrow ? m_in : 0, m3 = m2;
      if constexpr (AVAIL) { // no rows or columns skipped; the four edge masks from the neighbourhood
        mb = sao_xmask(0, W, x0);
        m0 = sao_pair_mask(a9, x0, y, 1, 0, W, H), m1 = sao_pair_mask(a9, x0, y, 0, 1, W, H);
        m2 = sao_pair_mask(a9, x0, y, 1, 1, W, H), m3 = sao_pair_mask(a9, x0, y, -1, 1, W, H);
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int i = k + 1, c = cur[i], diff = org[k] - c;
        sao_acc(mom[0], cnt[0], (m0 >> k) & 1, g[i] - g[i - 1], diff);
        sao_acc(mom[1], cnt[1], (m1 >> k) & 1, d1[i] - u1[i], diff);
        sao_acc(mom[2], cnt[2], (m2 >> k) & 1, d2[i] - u2[i - 1], diff);
        sao_acc(mom[3], cnt[3], (m3 >> k) & 1, d3[i] - u3[i + 1], diff);
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
// d_avail: null = calcSaoStatsCuOrg, else calcSaoStatsBlock with these availabilities (lcu_based is then 0: nothing is skipped)
static int sao_stats_multi(hmx_ctx *c, const char *fn, int n_pics, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h, int lcu_based,
                           const uint8_t *d_avail, hmx_sao_stat *d_out) {
  if (!c || !org || !rec || !d_out) return fail(c, HMX_ERR_ARG, std::string(fn) + ": null argument");
  const PlanesDev *d;
  if (int r = multi_pics(c, fn, n_pics, multiple_of(pic_w, pic_h, 8), kMultipleOf8, org, rec, nullptr, planes_of, &d)) return r;
  const int ctu = c->cfg.ctu_size, cw = (pic_w + ctu - 1) / ctu, n_lcu = cw * ((pic_h + ctu - 1) / ctu);
  SaoStatArgs A{d, d_out, n_pics, pic_w, pic_h, ctu, c->cfg.bit_depth, lcu_based ? 1 : 0, n_lcu, cw, d_avail};
  const dim3 grid((unsigned)n_lcu, 3, (unsigned)n_pics);
  if (d_avail) hipLaunchKernelGGL(k_sao_stats<true>, grid, dim3(kSaoStatThreads), 0, c->stream, A);
  else hipLaunchKernelGGL(k_sao_stats<false>, grid, dim3(kSaoStatThreads), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_sao_stats_multi(hmx_ctx *c, int n_pics, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h, int lcu_based,
                                   hmx_sao_stat *d_out) {
  return sao_stats_multi(c, "hmx_sao_stats_multi", n_pics, org, rec, pic_w, pic_h, lcu_based, nullptr, d_out);
}
extern "C" int hmx_sao_stats_multi_avail(hmx_ctx *c, int n_pics, const hmx_pic *org, const hmx_pic *rec, int pic_w, int pic_h,
                                         const uint8_t *d_avail, hmx_sao_stat *d_out) {
  if (!d_avail) return fail(c, HMX_ERR_ARG, "hmx_sao_stats_multi_avail: null argument");
  return sao_stats_multi(c, "hmx_sao_stats_multi_avail", n_pics, org, rec, pic_w, pic_h, 0, d_avail, d_out);
}

// ---- border availability of the loop filters (TComDataCU::setNDBFilterBlockBorderAvailability, TComDataCU.cpp:4212-4634, with
// MODIFIED_CROSS_SLICE and REMOVE_FGS: one block per CTU).  Host only; no context.
extern "C" int hmx_lf_border_avail(int pic_w, int pic_h, int ctu, const uint32_t *slice_id, const uint8_t *slice_lf_cross, int n_slices,
                                   const uint32_t *tile_id, int lf_cross_tiles, uint8_t *avail) {
  if (!slice_id || !slice_lf_cross || !avail || pic_w <= 0 || pic_h <= 0 || ctu <= 0 || n_slices <= 0) return HMX_ERR_ARG;
  const int cw = (pic_w + ctu - 1) / ctu, ch = (pic_h + ctu - 1) / ctu;
  for (int a = 0; a < cw * ch; a++)
    if (slice_id[a] >= (uint32_t)n_slices) return HMX_ERR_ARG;
  static const int kDx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, kDy[8] = {0, 0, -1, 1, -1, -1, 1, 1}; // SGU_L, R, T, B, TL, TR, BL, BR
  for (int y = 0; y < ch; y++)
    for (int x = 0; x < cw; x++) {
      const int a = y * cw + x;
      const uint32_t s = slice_id[a];
      unsigned m = 0;
      for (int k = 0; k < 8; k++) {
        const int nx = x + kDx[k], ny = y + kDy[k];
        if (nx < 0 || nx >= cw || ny < 0 || ny >= ch) continue; // bPic?Boundary
        const int n = ny * cw + nx;
        const uint32_t r = slice_id[n];
        bool ok = n_slices == 1 || r == s || slice_lf_cross[r > s ? r : s]; // onlyOneSliceInPic; the later slice's flag (:4299)
        if (!lf_cross_tiles && tile_id && tile_id[n] != tile_id[a]) ok = false; // :4589-4623
        m |= (unsigned)ok << k;
      }
      avail[a] = (uint8_t)m;
    }
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
  if (!c || !d_file || !t || index < 0 || index >= t->n_pics || file_bits < 8 || file_bits > 16 || (t->geom.pic_w & 1) || (t->geom.pic_h & 1) || pad_x < 0 ||
      pad_y < 0 || (pad_x & 1) || (pad_y & 1) || pad_x >= t->geom.pic_w || pad_y >= t->geom.pic_h)
    return fail(c, HMX_ERR_ARG, "hmx_yuv_unpack_resident: bad argument");
  TiledPic TP;
  for (int p = 0; p < 3; p++) TP.T[p] = tpool_plane(t, index, p);
  hipLaunchKernelGGL(k_yuv_unpack<true>, dim3((unsigned)(((size_t)((t->geom.pic_w + 7) / 8) * t->geom.pic_h + 255) / 256), 3), dim3(256), 0, c->stream,
                     static_cast<const unsigned char *>(d_file), file_bits > 8 ? 1 : 0, c->cfg.bit_depth - file_bits, c->cfg.bit_depth,
                     t->geom.pic_w, t->geom.pic_h, pad_x, pad_y, PlanesDev{}, TP);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_yuv_pack_resident(hmx_ctx *c, const hmx_tpool *t, int index, int crop_right, int crop_bottom, int file_bits, void *d_file) {
  if (!c || !d_file || !t || index < 0 || index >= t->n_pics || file_bits < 8 || file_bits > 16 || crop_right < 0 || crop_bottom < 0 ||
      crop_right >= t->geom.pic_w || crop_bottom >= t->geom.pic_h || ((t->geom.pic_w - crop_right) & 1) || ((t->geom.pic_h - crop_bottom) & 1))
    return fail(c, HMX_ERR_ARG, "hmx_yuv_pack_resident: bad argument");
  const int ww = t->geom.pic_w - crop_right, hh = t->geom.pic_h - crop_bottom;
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

