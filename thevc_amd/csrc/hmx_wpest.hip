// hmx_wpest.hip -- the encoder's estimation of explicit weighted-prediction parameters: WeightPredAnalysis
// (TLibEncoder/WeightPredAnalysis.cpp), called per slice from TEncSlice.cpp:688-711.  The whole-picture reductions are kernels
// (xCalcDCValue / xCalcACValue :451-487, xCalcSADvalueWP :501-517); the scalar arithmetic per (list, reference, component)
// (xUpdatingWPParameters :252-304, the decision of xSelectWP :352-362, xCheckWPEnable :135-170) runs on the host, because every
// consumer of a hmx_wp row takes its tables as host arrays.
#include "hmx_host.h"

#include <cassert>

namespace {
typedef short wps8v __attribute__((ext_vector_type(8)));
typedef unsigned long long u64;

constexpr int kWpThreads = 256, kWpWaves = kWpThreads / 64;
constexpr int kWpRowsPerWave = 4; // rows of a plane one wave walks (a 2160p luma plane: 135 workgroups)

// Samples [x0, x0 + 8) of a row of w samples, x0 = 8 k - lead with lead = the samples between the 16-byte boundary below the row's
// first sample and that sample: every chunk starts on a 16-byte boundary.  A chunk that lies inside the row is ONE 16-byte load;
// the first and the last chunk of a row are cut by it and take one predicated load per sample, so nothing outside the row is ever
// read.  Returns the mask of samples that exist; the others are 0.
__device__ __forceinline__ unsigned wp_chunk(const short *row, int x0, int w, int v[8]) {
  if (x0 >= 0 && x0 + 8 <= w) {
    const wps8v t = *reinterpret_cast<const wps8v *>(row + x0);
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = t[j];
    return 0xffu;
  }
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const bool in = x0 + j >= 0 && x0 + j < w;
    v[j] = in ? row[x0 + j] : 0;
    m |= (unsigned)in << j;
  }
  return m;
}
// The same for a row whose chunks follow ANOTHER row's boundaries (the reconstruction against the original): one 16-byte load
// where this row's address happens to be aligned too (aligned: of row + x0 for every chunk, as chunks are 16 bytes apart), one
// load per sample otherwise.
__device__ __forceinline__ void wp_chunk_beside(const short *row, int x0, int w, bool aligned, int v[8]) {
  if (aligned && x0 >= 0 && x0 + 8 <= w) {
    const wps8v t = *reinterpret_cast<const wps8v *>(row + x0);
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = t[j];
    return;
  }
#pragma unroll
  for (int j = 0; j < 8; j++) v[j] = x0 + j >= 0 && x0 + j < w ? row[x0 + j] : 0;
}
__device__ __forceinline__ int wp_lead(const short *row) { return (int)(((uintptr_t)row & 15) >> 1); }

// Sum of a non-negative 64-bit value over the wave, in every lane: three limbs of 24, 24 and 16 bits through group_sum (64 limbs
// of 24 bits stay below 2^30).
__device__ __forceinline__ u64 wp_wave_sum(u64 v) {
  const unsigned a = (unsigned)group_sum((int)(v & 0xffffffu), 64), b = (unsigned)group_sum((int)((v >> 24) & 0xffffffu), 64),
                 c = (unsigned)group_sum((int)(v >> 48), 64);
  return (u64)a + ((u64)b << 24) + ((u64)c << 48);
}
// The workgroup's total of N values per lane added to dst[0..N): wave sums on DPP, the waves through LDS, one 64-bit vector
// atomic per value.  Integer addition commutes, so the result does not depend on the order the workgroups arrive in.
template <int N>
__device__ __forceinline__ void wp_block_add(const u64 (&v)[N], u64 *dst) {
  __shared__ u64 part[kWpWaves][N];
  const int t = threadIdx.x, wave = t >> 6;
#pragma unroll
  for (int i = 0; i < N; i++) {
    const u64 s = wp_wave_sum(v[i]);
    if ((t & 63) == 0) part[wave][i] = s;
  }
  __syncthreads();
  if (t < N) {
    u64 s = 0;
#pragma unroll
    for (int q = 0; q < kWpWaves; q++) s += part[q][t];
    if (s) atomicAdd(dst + t, s);
  }
}

struct WpAcdcArgs {
  const PlanesDev *pics; // [n_pics]
  u64 *sums;             // [n_pics][3]: the sample sums between the passes
  hmx_wp_acdc_param *out;
  int pic_w, pic_h;
};
// PASS 0: the sums of xCalcDCValue into A.sums (zeroed by the host); PASS 1: iDC = (sum + (n >> 1)) / n from those sums -- formed
// here, in every workgroup, so that no value travels to the host between the passes -- and the sums of xCalcACValue into
// A.out[pic].ac (zeroed by pass 0, which precedes this launch on the stream).
// Widening: a sample is below 2^15 (Pel) and a DC lies in the samples' range, so a chunk's eight terms sum to less than 2^19 in
// 32 bits; every chunk's sum is added to the lane's 64-bit total at once.
template <int PASS>
__global__ __launch_bounds__(kWpThreads) void k_wp_acdc(WpAcdcArgs A) {
  const int p = blockIdx.y, pic = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const int w = A.pic_w >> (p ? 1 : 0), h = A.pic_h >> (p ? 1 : 0);
  const PlanesDev *P = A.pics + pic;
  const short *plane = P->p[p];
  const int stride = P->s[p];
  unsigned dc = 0;
  if (PASS == 1) {
    const u64 n = (u64)w * (u64)h;
    dc = (unsigned)((A.sums[pic * 3 + p] + (n >> 1)) / n);
    if (blockIdx.x == 0 && t == 0) A.out[pic].dc[p] = (int64_t)dc;
  } else if (blockIdx.x == 0 && t == 0) {
    A.out[pic].ac[p] = 0;
  }
  u64 acc[1] = {0};
  const int y0 = (blockIdx.x * kWpWaves + (t >> 6)) * kWpRowsPerWave;
  for (int y = y0; y < min(y0 + kWpRowsPerWave, h); y++) {
    const short *row = plane + (size_t)y * stride;
    const int lead = wp_lead(row), chunks = (lead + w + 7) >> 3;
    for (int k = lane; k < chunks; k += 64) {
      int v[8];
      const unsigned m = wp_chunk(row, 8 * k - lead, w, v);
      unsigned s = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (PASS == 0) s += (unsigned)v[j];
        else s += ((m >> j) & 1) ? __usad((unsigned)v[j], dc, 0u) : 0u;
      }
      acc[0] += s;
    }
  }
  wp_block_add<1>(acc, PASS == 0 ? A.sums + pic * 3 + p : reinterpret_cast<u64 *>(&A.out[pic].ac[p]));
}

struct WpSadJob { // one hmx_wp_sad_job for the device: per component the weight, -(offset << (denominator + B - 8)) and the denominator
  int org, rec;
  int w[3], c[3], d[3];
};
struct WpSadArgs {
  const WpSadJob *jobs;
  const PlanesDev *org, *rec;
  u64 *out; // [n_jobs][3][2], zeroed by the host
  int pic_w, pic_h;
};
// xCalcSADvalueWP for the job's row and for the default row of the same denominator, from one read of the two pictures:
//   |(org << d) - (rec * w + (o << rd))| and |(org << d) - (rec << d)| = |org - rec| << d (shifted once, at the end).
// Widening, with B <= 12, d <= 7, -128 <= w <= 256 and o any int16: org << d < 2^19, |rec * w| < 2^20, |o << rd| <= 2^26, so a term
// is below 2^27 and fits int; a chunk's eight terms sum to less than 2^30 in 32 bits (the default row's: 8 * 2^12), and every
// chunk's sums are added to the lane's 64-bit totals at once.
__global__ __launch_bounds__(kWpThreads) void k_wp_sad(WpSadArgs A) {
  const int p = blockIdx.y, job = blockIdx.z, t = threadIdx.x, lane = t & 63;
  const int w = A.pic_w >> (p ? 1 : 0), h = A.pic_h >> (p ? 1 : 0);
  const WpSadJob *J = A.jobs + job;
  const PlanesDev *O = A.org + J->org, *R = A.rec + J->rec;
  const short *po = O->p[p], *pr = R->p[p];
  const int so = O->s[p], sr = R->s[p];
  const int nw = -J->w[p], c = J->c[p], d = J->d[p];
  u64 acc[2] = {0, 0};
  const int y0 = (blockIdx.x * kWpWaves + (t >> 6)) * kWpRowsPerWave;
  for (int y = y0; y < min(y0 + kWpRowsPerWave, h); y++) {
    const short *ro = po + (size_t)y * so, *rr = pr + (size_t)y * sr;
    const int lead = wp_lead(ro), chunks = (lead + w + 7) >> 3;
    const bool beside = wp_lead(rr) == lead; // the reconstruction's chunks start on 16-byte boundaries too
    for (int k = lane; k < chunks; k += 64) {
      int a[8], b[8];
      const unsigned m = wp_chunk(ro, 8 * k - lead, w, a);
      wp_chunk_beside(rr, 8 * k - lead, w, beside, b);
      unsigned s_wp = 0, s_no = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int e = (a[j] << d) + c + b[j] * nw;
        s_wp += ((m >> j) & 1) ? (unsigned)abs(e) : 0u; // a sample outside the row is 0 in both pictures: only this sum sees the offset
        s_no = __usad((unsigned)a[j], (unsigned)b[j], s_no);
      }
      acc[0] += s_wp;
      acc[1] += s_no;
    }
  }
  acc[1] <<= d;
  wp_block_add<2>(acc, A.out + ((size_t)job * 3 + p) * 2);
}

// ---- what the entries share on the host ----
const char *const kWpSizeRule = "picture size must be positive and even, at most 65536";
bool wp_size_ok(int pic_w, int pic_h) { return pic_w > 0 && pic_h > 0 && pic_w % 2 == 0 && pic_h % 2 == 0 && pic_w <= 65536 && pic_h <= 65536; }
// a table of n pictures in the argument arena; every plane must be there.  reserved: the caller puts further tables before its
// launch and has reserved this one with them (arena_reserve)
int wp_pics(hmx_ctx *c, const char *fn, const hmx_pic *pics, int n, const PlanesDev **d, bool reserved = false) {
  std::vector<PlanesDev> t((size_t)n);
  for (int i = 0; i < n; i++) {
    for (int p = 0; p < 3; p++)
      if (!pics[i].plane[p]) return fail(c, HMX_ERR_ARG, std::string(fn) + ": null plane");
    t[i] = to_dev(&pics[i]);
  }
  const size_t bytes = sizeof(PlanesDev) * t.size();
  *d = static_cast<const PlanesDev *>(reserved ? arena_place(c, t.data(), bytes) : arena_push(c, t.data(), bytes));
  if (*d) return HMX_OK;
  return reserved ? fail(c, HMX_ERR_INTERNAL, kArenaOutside) : fail(c, HMX_ERR_NOMEM, "argument arena");
}
unsigned wp_grid_x(int pic_h) { return (unsigned)((pic_h + kWpWaves * kWpRowsPerWave - 1) / (kWpWaves * kWpRowsPerWave)); }
// the rows hmx_wp_sad_multi takes: those of the other _wp entries, but any int16 as the luma offset (WeightPredAnalysis.cpp:279
// does not clip it)
bool wp_sad_row_ok(const hmx_wp &r, int max_weight) {
  if (r.reserved != 0) return false;
  for (int k = 0; k < 3; k++)
    if (!wp_range_ok(std::min<int>(r.weight[k], 255), k ? r.offset[k] : 0, r.log2_denom[k]) || r.weight[k] > max_weight) return false;
  return true;
}
template <typename T>
T wp_clip3(T lo, T hi, T v) { return v < lo ? lo : v > hi ? hi : v; }
} // namespace

extern "C" int hmx_wp_acdc_multi(hmx_ctx *c, int n_pics, const hmx_pic *pics, int pic_w, int pic_h, hmx_wp_acdc_param *d_out) {
  if (!c || !pics || !d_out) return fail(c, HMX_ERR_ARG, "hmx_wp_acdc_multi: null argument");
  if (n_pics < 1 || n_pics > 65535) return fail(c, HMX_ERR_ARG, "hmx_wp_acdc_multi: n_pics must be 1..65535");
  if (!wp_size_ok(pic_w, pic_h)) return fail(c, HMX_ERR_ARG, std::string("hmx_wp_acdc_multi: ") + kWpSizeRule);
  const PlanesDev *d;
  if (int r = wp_pics(c, "hmx_wp_acdc_multi", pics, n_pics, &d)) return r;
  const size_t sums_bytes = sizeof(u64) * 3 * (size_t)n_pics;
  if (int r = grow_dev(c, &c->d_wpest, &c->wpest_cap, sums_bytes, "weight estimation sums")) return r;
  HIPCHK(c, hipMemsetAsync(c->d_wpest, 0, sums_bytes, c->stream));
  const WpAcdcArgs A{d, static_cast<u64 *>(c->d_wpest), d_out, pic_w, pic_h};
  const dim3 grid(wp_grid_x(pic_h), 3, (unsigned)n_pics);
  hipLaunchKernelGGL(k_wp_acdc<0>, grid, dim3(kWpThreads), 0, c->stream, A);
  hipLaunchKernelGGL(k_wp_acdc<1>, grid, dim3(kWpThreads), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_wp_acdc(hmx_ctx *c, const hmx_pic *pic, int pic_w, int pic_h, hmx_wp_acdc_param *d_out) {
  return hmx_wp_acdc_multi(c, 1, pic, pic_w, pic_h, d_out);
}

// hmx_wp_sad_multi under the name of the entry that runs it.  max_weight: 255 for the public entry; 256 for hmx_wp_estimate_slices,
// whose rows are the reference's own, and xUpdatingWPParameters lets 256 through at denominator 7 (128 - 256 = -128, :293).  The
// kernel's bounds hold for it: 4095 * 256 < 2^20.
static int wp_sad_run(hmx_ctx *c, const char *entry, int max_weight, int n_jobs, const hmx_wp_sad_job *jobs, const hmx_pic *org, int n_org,
                      const hmx_pic *rec, int n_rec, int pic_w, int pic_h, int64_t *d_out) {
  const std::string fn = entry;
  if (!c || !jobs || !org || !rec || !d_out) return fail(c, HMX_ERR_ARG, fn + ": null argument");
  if (n_jobs < 1 || n_jobs > 65535) return fail(c, HMX_ERR_ARG, fn + ": n_jobs must be 1..65535");
  if (n_org < 1 || n_rec < 1) return fail(c, HMX_ERR_ARG, fn + ": n_org and n_rec must be at least 1");
  if (!wp_size_ok(pic_w, pic_h)) return fail(c, HMX_ERR_ARG, fn + ": " + kWpSizeRule);
  const int B = c->cfg.bit_depth;
  std::vector<WpSadJob> t((size_t)n_jobs);
  for (int i = 0; i < n_jobs; i++) {
    const hmx_wp_sad_job &j = jobs[i];
    if (j.org >= (uint32_t)n_org || j.rec >= (uint32_t)n_rec)
      return fail(c, HMX_ERR_ARG, fn + ": job " + std::to_string(i) + ": picture index outside org[] / rec[]");
    if (!wp_sad_row_ok(j.wp, max_weight))
      return fail(c, HMX_ERR_ARG, fn + ": job " + std::to_string(i) +
                                      ": weight outside -128..255, chroma offset outside -128..127, log2_denom above 7 or reserved not 0");
    t[i].org = (int)j.org, t[i].rec = (int)j.rec;
    for (int k = 0; k < 3; k++)
      t[i].w[k] = j.wp.weight[k], t[i].d[k] = j.wp.log2_denom[k], t[i].c[k] = -(j.wp.offset[k] * (1 << (j.wp.log2_denom[k] + B - 8)));
  }
  const PlanesDev *d_org, *d_rec;
  const size_t job_bytes = sizeof(WpSadJob) * t.size(); // three tables, one launch: reserved together
  if (int r = arena_reserve(c, {sizeof(PlanesDev) * (size_t)n_org, sizeof(PlanesDev) * (size_t)n_rec, job_bytes}, "argument arena")) return r;
  if (int r = wp_pics(c, entry, org, n_org, &d_org, true)) return r;
  if (int r = wp_pics(c, entry, rec, n_rec, &d_rec, true)) return r;
  const WpSadJob *d_jobs = static_cast<const WpSadJob *>(arena_place(c, t.data(), job_bytes));
  if (!d_jobs) return fail(c, HMX_ERR_INTERNAL, kArenaOutside);
  HIPCHK(c, hipMemsetAsync(d_out, 0, sizeof(int64_t) * 6 * (size_t)n_jobs, c->stream));
  const WpSadArgs A{d_jobs, d_org, d_rec, reinterpret_cast<u64 *>(d_out), pic_w, pic_h};
  hipLaunchKernelGGL(k_wp_sad, dim3(wp_grid_x(pic_h), 3, (unsigned)n_jobs), dim3(kWpThreads), 0, c->stream, A);
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_wp_sad_multi(hmx_ctx *c, int n_jobs, const hmx_wp_sad_job *jobs, const hmx_pic *org, int n_org, const hmx_pic *rec,
                                int n_rec, int pic_w, int pic_h, int64_t *d_out) {
  return wp_sad_run(c, "hmx_wp_sad_multi", 255, n_jobs, jobs, org, n_org, rec, n_rec, pic_w, pic_h, d_out);
}

// ---- host arithmetic: int64_t / double in the reference's order of operations ----
// xUpdatingWPParameters (:252-304) for the rows of one list at denominator d; false = a weight left the coded range (:293)
static bool wp_update_list(const hmx_wp_acdc_param *cur, const hmx_wp_acdc_param *refs, int n, int B, int d, hmx_wp *rows) {
  const int rd = d + B - 8, real_offset = 1 << (rd - 1);
  for (int r = 0; r < n; r++) {
    rows[r].reserved = 0;
    for (int comp = 0; comp < 3; comp++) {
      const int64_t cur_dc = cur->dc[comp], cur_ac = cur->ac[comp], ref_dc = refs[r].dc[comp], ref_ac = refs[r].ac[comp];
      const double d_weight = ref_ac == 0 ? 1.0 : wp_clip3(-16.0, 15.0, (double)cur_ac / (double)ref_ac);
      const int weight = (int)(0.5 + d_weight * (double)(1 << d));
      int offset = (int)(((cur_dc << d) - ((int64_t)weight * ref_dc) + (int64_t)real_offset) >> rd);
      if (comp) { // chroma offset range limitation (:282-288)
        const int shift = 1 << (B - 1), pred = shift - ((shift * weight) >> d);
        const int delta = wp_clip3(-512, 511, offset - pred);
        offset = wp_clip3(-128, 127, delta + pred);
      }
      const int delta_weight = (1 << d) - weight;
      if (delta_weight > 127 || delta_weight < -128) return false;
      // the luma offset is not clipped (:279); with both DCs below 2^B and the weight at most 15 * 2^d it stays inside +-2^12
      rows[r].weight[comp] = (int16_t)weight, rows[r].offset[comp] = (int16_t)offset, rows[r].log2_denom[comp] = (uint8_t)d;
    }
  }
  return true;
}
extern "C" int hmx_wp_update_params(const hmx_wp_acdc_param *cur, const hmx_wp_acdc_param *refs_l0, int n_l0, const hmx_wp_acdc_param *refs_l1, int n_l1,
                                    int bit_depth, hmx_wp *rows_l0, hmx_wp *rows_l1, uint8_t *present_l0, uint8_t *present_l1,
                                    int *log2_denom) {
  if (!cur || !log2_denom || n_l0 < 0 || n_l1 < 0 || (n_l0 && (!refs_l0 || !rows_l0 || !present_l0)) ||
      (n_l1 && (!refs_l1 || !rows_l1 || !present_l1)) || bit_depth < 8 || bit_depth > 12)
    return HMX_ERR_ARG;
  int d = n_l0 > 3 ? 7 : 6; // xEstimateWPParamSlice :178-194
  while (!(wp_update_list(cur, refs_l0, n_l0, bit_depth, d, rows_l0) && wp_update_list(cur, refs_l1, n_l1, bit_depth, d, rows_l1))) {
    d--; // :197-204.  AC >= 0 bounds the weight by 15 * 2^d, which is inside the range from d = 3 down
    assert(d >= 3);
  }
  for (int r = 0; r < n_l0; r++) present_l0[r] = 1;
  for (int r = 0; r < n_l1; r++) present_l1[r] = 1;
  *log2_denom = d;
  return HMX_OK;
}
extern "C" int hmx_wp_select(const int64_t *sums, int64_t n_luma, int64_t n_chroma, int log2_denom, hmx_wp *row, uint8_t *present) {
  if (!sums || !row || !present || n_luma <= 0 || n_chroma <= 0 || log2_denom < 0 || log2_denom > 7) return HMX_ERR_ARG;
  int64_t sad_wp = 0, sad_no = 0; // every component divided by its own size before the sum (:516, :333-350)
  for (int comp = 0; comp < 3; comp++) {
    const int64_t n = comp ? n_chroma : n_luma;
    sad_wp += sums[2 * comp] / n, sad_no += sums[2 * comp + 1] / n;
  }
  const double ratio = (double)sad_wp / (double)sad_no; // 0 / 0 is NaN and keeps the rows, x / 0 is +inf and resets them (:352-353)
  if (ratio >= 0.99) {
    for (int comp = 0; comp < 3; comp++) row->weight[comp] = (int16_t)(1 << log2_denom), row->offset[comp] = 0, row->log2_denom[comp] = (uint8_t)log2_denom;
    *present = 0;
  }
  return HMX_OK;
}
extern "C" int hmx_wp_check_enable(hmx_wp *rows_l0, uint8_t *present_l0, int n_l0, hmx_wp *rows_l1, uint8_t *present_l1, int n_l1,
                                   int *weighted) {
  if (!weighted || n_l0 < 0 || n_l1 < 0 || (n_l0 && (!rows_l0 || !present_l0)) || (n_l1 && (!rows_l1 || !present_l1))) return HMX_ERR_ARG;
  int cnt = 0;
  for (int r = 0; r < n_l0; r++) cnt += present_l0[r] != 0;
  for (int r = 0; r < n_l1; r++) cnt += present_l1[r] != 0;
  *weighted = cnt != 0;
  if (cnt) return HMX_OK;
  const auto clear = [](hmx_wp *rows, int n) {
    for (int r = 0; r < n; r++)
      for (int comp = 0; comp < 3; comp++) rows[r].weight[comp] = 1, rows[r].offset[comp] = 0, rows[r].log2_denom[comp] = 0;
  };
  clear(rows_l0, n_l0), clear(rows_l1, n_l1);
  return HMX_OK;
}

// xEstimateWPParamSlice + xCheckWPEnable for n_slices slices: steps 2 to 4 with one hmx_wp_sad_multi launch and one download
extern "C" int hmx_wp_estimate_slices(hmx_ctx *c, int n_slices, hmx_wp_slice *slices) {
  if (!c || !slices) return fail(c, HMX_ERR_ARG, "hmx_wp_estimate_slices: null argument");
  if (n_slices < 1) return fail(c, HMX_ERR_ARG, "hmx_wp_estimate_slices: n_slices must be at least 1");
  const int pic_w = slices[0].pic_w, pic_h = slices[0].pic_h; // one launch: one size
  if (!wp_size_ok(pic_w, pic_h)) return fail(c, HMX_ERR_ARG, std::string("hmx_wp_estimate_slices: ") + kWpSizeRule);
  // the AC/DC values that live on the device: one download for all of them
  struct Fetch { const hmx_wp_acdc_param *src; hmx_wp_acdc_param v; };
  std::vector<Fetch> fetch;
  const auto want = [&](const hmx_wp_acdc_param *d_ptr, const hmx_wp_acdc_param *h_ptr) -> int { // index into fetch, -1 = host value
    if (h_ptr) return -1;
    fetch.push_back(Fetch{d_ptr, {}});
    return (int)fetch.size() - 1;
  };
  size_t n_jobs = 0;
  for (int s = 0; s < n_slices; s++) {
    hmx_wp_slice &S = slices[s];
    const std::string who = "hmx_wp_estimate_slices: slice " + std::to_string(s);
    if (S.slice_type != HMX_P_SLICE && S.slice_type != HMX_B_SLICE) return fail(c, HMX_ERR_ARG, who + ": slice_type must be HMX_P_SLICE or HMX_B_SLICE");
    if (S.pic_w != pic_w || S.pic_h != pic_h) return fail(c, HMX_ERR_ARG, who + ": the slices of a call share one picture size");
    if (!S.org || (!S.acdc && !S.d_acdc)) return fail(c, HMX_ERR_ARG, who + ": no original or no AC/DC values");
    if (S.slice_type == HMX_P_SLICE && S.n_refs[1] != 0) return fail(c, HMX_ERR_ARG, who + ": a P slice has no list 1");
    for (int l = 0; l < 2; l++) {
      if (S.n_refs[l] < 0 || S.n_refs[l] > HMX_WP_MAX_REFS || (l == 0 && S.n_refs[l] < 1)) return fail(c, HMX_ERR_ARG, who + ": list size outside 1..16 (list 1: 0..16)");
      if (S.n_refs[l] && (!S.rec[l] || (!S.ref_acdc[l] && !S.d_ref_acdc[l]) || !S.rows[l] || !S.present[l])) return fail(c, HMX_ERR_ARG, who + ": null list argument");
      n_jobs += (size_t)S.n_refs[l];
    }
  }
  if (n_jobs > 65535) return fail(c, HMX_ERR_ARG, "hmx_wp_estimate_slices: more than 65535 (list, reference) entries");
  std::vector<int> at;
  for (int s = 0; s < n_slices; s++) {
    const hmx_wp_slice &S = slices[s];
    at.push_back(want(S.d_acdc, S.acdc));
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < S.n_refs[l]; r++) {
        if (!S.ref_acdc[l] && !S.d_ref_acdc[l][r]) return fail(c, HMX_ERR_ARG, "hmx_wp_estimate_slices: slice " + std::to_string(s) + ": null AC/DC pointer");
        at.push_back(want(S.ref_acdc[l] ? nullptr : S.d_ref_acdc[l][r], S.ref_acdc[l] ? &S.ref_acdc[l][r] : nullptr));
      }
  }
  for (Fetch &f : fetch) HIPCHK(c, hipMemcpyAsync(&f.v, f.src, sizeof(hmx_wp_acdc_param), hipMemcpyDeviceToHost, c->stream));
  if (!fetch.empty()) HIPCHK(c, hipStreamSynchronize(c->stream));
  // step 2 per slice, and the jobs of step 3
  std::vector<hmx_wp_sad_job> jobs;
  std::vector<hmx_pic> orgs, recs;
  size_t a = 0;
  for (int s = 0; s < n_slices; s++) {
    hmx_wp_slice &S = slices[s];
    const int i_cur = at[a++];
    const hmx_wp_acdc_param cur = i_cur < 0 ? *S.acdc : fetch[(size_t)i_cur].v;
    std::vector<hmx_wp_acdc_param> ref[2];
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < S.n_refs[l]; r++) {
        const int i = at[a++];
        ref[l].push_back(i < 0 ? S.ref_acdc[l][r] : fetch[(size_t)i].v);
      }
    if (hmx_wp_update_params(&cur, ref[0].data(), S.n_refs[0], ref[1].data(), S.n_refs[1], c->cfg.bit_depth, S.rows[0], S.rows[1], S.present[0],
                             S.present[1], &S.log2_denom))
      return fail(c, HMX_ERR_ARG, "hmx_wp_estimate_slices: hmx_wp_update_params refused slice " + std::to_string(s));
    orgs.push_back(*S.org);
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < S.n_refs[l]; r++) {
        jobs.push_back(hmx_wp_sad_job{(uint32_t)s, (uint32_t)recs.size(), S.rows[l][r]});
        recs.push_back(S.rec[l][r]);
      }
  }
  // step 3: one launch, one download
  const size_t out_bytes = sizeof(int64_t) * 6 * jobs.size();
  if (int r = grow_dev(c, &c->d_wpest, &c->wpest_cap, out_bytes, "weight estimation sums")) return r;
  if (int r = wp_sad_run(c, "hmx_wp_estimate_slices", 256, (int)jobs.size(), jobs.data(), orgs.data(), (int)orgs.size(), recs.data(), (int)recs.size(),
                         pic_w, pic_h, static_cast<int64_t *>(c->d_wpest)))
    return r;
  std::vector<int64_t> sums(6 * jobs.size());
  HIPCHK(c, hipMemcpyAsync(sums.data(), c->d_wpest, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t n_luma = (int64_t)pic_w * pic_h, n_chroma = (int64_t)(pic_w >> 1) * (pic_h >> 1);
  size_t j = 0;
  for (int s = 0; s < n_slices; s++) {
    hmx_wp_slice &S = slices[s];
    for (int l = 0; l < 2; l++)
      for (int r = 0; r < S.n_refs[l]; r++, j++) hmx_wp_select(&sums[6 * j], n_luma, n_chroma, S.log2_denom, &S.rows[l][r], &S.present[l][r]);
    hmx_wp_check_enable(S.rows[0], S.present[0], S.n_refs[0], S.rows[1], S.present[1], S.n_refs[1], &S.weighted); // step 4
  }
  return HMX_OK;
}
