// hmx_host.h -- what the translation units of libhmx share: the structures that travel between host and device, the
// context, and the prototypes of the host helpers that cross files.  The library is cut into
//   hmx_core.hip        context, device-memory plumbing, quantiser parameters, argument arena
//   hmx_list.hip        block-list kernels (k_list, k_inter4, k_inter32) and the hmx_batch_* entry points over lists
//   hmx_scalar.hip      scalar drop-ins of TComTrQuant / TComPattern / TComPrediction / TComRdCost, RDOQ block list
//   hmx_plan.hip        intra plans: dependency analysis on the host and on the device
//   hmx_chain.hip       whole-picture all-intra chain: level / wave / packed schedules, resident pools
//   hmx_chain_rdoq.hip  the packed schedule's kernel with xRateDistOptQuant as its quantiser (a translation unit of its own:
//                       its instantiations take as long to compile as everything else together)
//   hmx_chain_qmap.hip  the packed schedule's kernel with a QP per block (hmx_set_qp_map), likewise a unit of its own
//   hmx_inter.hip       interpolation filters, motion compensation, sub-pel cost fan-out, border extension, prediction error of
//                       complete motion candidates (k_pred_error)
//   hmx_me.hip          full-search integer motion estimation (SAD, vector-bits cost, search box)
//   hmx_loop.hip        deblocking, SAO, YUV file formats
//   hmx_wpest.hip       the encoder's weight estimation (WeightPredAnalysis): AC/DC and weighted SAD reductions, host arithmetic
//   hmx_aq.hip          adaptive QP (TEncPreanalyzer, TEncCu::xComputeQP): block activities of all layers, layer averages, QP maps
//   hmx_saodec.hip      the encoder's SAO parameter search (rdoSaoUnitAll, LCU-based): candidates per CTU, the serial decision per picture
// Beside them stand three headers of host arithmetic with no HIP in them, which the library uses and tests/native/*.cpp runs on the CPU:
//   hmx_arena.h         where a call's tables go in the argument arena
//   hmx_rdoq_core.h     xRateDistOptQuant decomposed for the lanes of a wave (host and device)
//   hmx_call_rules.h    what a whole-picture call decides before it touches the device: packing group, shape and limits of the packed
//                       tables, persistent waves, the schedule it resolves to, RDOQ's per-call constants
// and hmx_lib.hip includes all of them for a single-translation-unit build (-DHMX_PACK_PROFILE builds read device
// symbols of several parts).  Build: __graft_entry__.build() compiles the parts in parallel and links libhmx.so.
//
// Staging of the scalar drop-ins (host pointers in and out): a drop-in carves the context's device scratch (hmx_ctx::d_scratch, 1 MiB)
// with Scratch -- take / up from the front, take_tail from the end for buffers that outlive one staging round -- runs one block through
// the batch kernels (run_one for the list kernels, launch_sized / with_size for the size-templated ones) and brings the block back
// with down2d.  The budget is enforced: a carve that does not fit, like a failed upload, sticks in Scratch::r, which is tested once
// before the launch, so an overflow is HMX_ERR_NOMEM and never a launch.  The largest drop-in is the 64x64 initAdiPattern, a 129 x 129
// window of samples (33 KB) and two 129 x 129 border buffers of Int (133 KB); motion compensation adds a tail of 2 x 64 x 64 shorts.
// A static_assert beside Scratch holds the worst case of every family against the allocation.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "hmx_arena.h"
#include "hmx_call_rules.h"
#include "hmx_kernels.h"
#include "hmx_rdoq.h"

using namespace hmx;

struct DTu { // device descriptor of the list kernels: hmx_tu + index in the caller's order
  hmx_tu t;
  uint32_t idx;
};
__device__ __forceinline__ DTu load_dtu(const DTu *p) { // one 12-byte load instead of one per field read
  typedef __attribute__((address_space(1))) const int gint;
  int w[3];
  __builtin_memcpy(w, (gint *)p, 12);
  DTu d;
  __builtin_memcpy(&d, w, 12);
  return d;
}

// list kernels: 256-thread workgroups = four autonomous waves; blocks per workgroup
template <int N>
struct Slots {
  static constexpr int v = N == 64 ? 1 : N == 32 ? 4 : 256 / N; // 32x32 scratch (9.5 KB) is kept to four blocks; 64x64 (prediction only, 19.5 KB): one
};
#define HMX_SMEM_BYTES (16 * (int)sizeof(TuLds<16>)) /* largest of Slots<N> * sizeof(TuLds<N>) */
static_assert(64 * sizeof(TuLds<4>) <= HMX_SMEM_BYTES && 32 * sizeof(TuLds<8>) <= HMX_SMEM_BYTES &&
                  4 * sizeof(TuLds<32>) <= HMX_SMEM_BYTES && sizeof(TuLds<64>) <= HMX_SMEM_BYTES,
              "LDS scratch");

enum ListOp { OP_TRANSFORM_NXN, OP_INVTRANSFORM_NXN, OP_XT, OP_XIT, OP_XQUANT, OP_XDEQUANT, OP_PRED, OP_TRANSFORM_RECON, OP_PRED_LAYOUT };

struct ListPic { // planes of one picture of a multi-picture list call
  PlanesDev a, b;
  LevelsDev lev;
  PlanesDev rec; // OP_TRANSFORM_RECON: reconstruction out
};
struct ListArgs {
  const DTu *tus;
  int n;
  const ListPic *pics; // != NULL: grid.y pictures, planes from this table instead of a / b / lev
  int n_pics, abs_stride;
  PlanesDev a;   // residual in (transform) / prediction in (inverse with recon) / recon (pred)
  PlanesDev b;   // output planes
  LevelsDev lev; // levels / coefficients (Int)
  LevelsDev lev2;
  uint32_t *abs_sum;
  uint32_t *sse; // OP_TRANSFORM_RECON: xGetSSE(org, rec) per block, indexed like abs_sum (NULL = none)
  int have_pred;
  PlanesDev org;        // OP_PRED with cost: the original the predictions are costed against
  uint32_t *cost;       // OP_PRED: calcHAD of every (block, mode), [block idx][n_modes]; NULL = none
  const uint8_t *modes; // OP_PRED fan-out
  int n_modes;
  size_t mode_elems[3];
  PicDev P;
  AvailDev lay; // OP_PRED_LAYOUT: the slice / tile / CIP layout of the picture
};

template <typename T>
__device__ __forceinline__ T pick3(const T (&a)[3], int i) { // a[i] without a run-time index (see k_list)
  T r = a[0];
  r = i == 1 ? a[1] : r;
  return i == 2 ? a[2] : r;
}
// The same for a table entry that is uniform over the wave: the three values are pinned as wave-uniform (scalar
// loads), or the compiler turns the select of loads back into one per-lane load from a selected address.
template <typename T>
__device__ __forceinline__ T uniform3v(T a0, T a1, T a2, int i) {
  const T v0 = wave_uniform(a0), v1 = wave_uniform(a1), v2 = wave_uniform(a2);
  T r = v0;
  r = i == 1 ? v1 : r;
  return i == 2 ? v2 : r;
}
#define uniform3(arr, i) uniform3v((arr)[0], (arr)[1], (arr)[2], (i))

// ---- whole-picture all-intra reconstruction: one launch per CTU diagonal ----
// Work item = (picture, CTU of the diagonal, plane), owned by ONE autonomous wave (64-thread
// workgroup): no workgroup barrier anywhere.  The host plan lists the item's blocks as segments of
// equal size and equal dependency level; a wave walks its segments, 64/N blocks at a time on the
// VALU path (N <= 16), one 32x32 block at a time on the matrix cores.
struct Seg { // a run of same-size blocks of one dependency level of one (CTU, plane)
  uint32_t start;
  uint16_t count;
  uint8_t log2n;
  uint8_t new_level; // 1: first segment of a dependency level (needs the previous level's recon)
};
struct FTu { // block descriptor of the frame path: geometry + precomputed neighbour availability
  hmx_tu t;
  uint32_t avail_lo, avail_hi; // the mask has at most 33 bits; bits 31 / 30 of avail_hi are kFtuPads / kFtuPadsSimple
};
// FTu::avail_hi: the block's mode reads a unit that is not available (hmx_intra_reads_unavailable), so its reference line needs
// the padding pass.  Without the bit every position the mode reads holds a gathered sample and the chains skip the pass.
constexpr uint32_t kFtuPads = 1u << 31;
// FTu::avail_hi, only with kFtuPads: no unavailable unit the mode reads lies strictly between the lowest and the highest unit of the
// mask (or the mask is empty), so the padding rule is line[p] = raw[clamp(p, lo, hi)] with lo / hi the first sample of the lowest /
// the last sample of the highest unit of the mask (hmx_intra_pads_simple).  Holes between available units --
// slices, tiles, constrained intra prediction -- clear it, and the block takes the general pass.
constexpr uint32_t kFtuPadsSimple = 1u << 30;
constexpr uint32_t kFtuFlagBits = kFtuPads | kFtuPadsSimple; // what is not mask in avail_hi
struct LevelRow { // blocks of one picture-wide dependency level, bucketed by size (log2n - 2)
  uint32_t start[4];
  uint32_t count[4];
};
struct PicWork { // per picture: working planes + the plan it follows
  TiledPlane org[3], rec[3]; // tiled working copies (see TiledPlane)
  int *lev[3];
  int lev_stride[3];         // > 0: plane geometry; 0: the reference's Z-order coefficient layout
  const FTu *tus;
  const Seg *segs;
  const uint32_t *seg_range; // [(ctu*3+plane)*2 + {0,1}] -> begin,end in segs
  const FTu *ltus;           // level schedule: blocks sorted by (level, size)
  const LevelRow *ltab;      // [n_levels]
  int n_levels;
};
struct FrameArgs {
  const PicWork *pics;
  const uint32_t *wave_ctus; // CTU ids of this diagonal
  int n_wave_ctus;
  PicDev P;
};
// plane <-> tiled conversion: one thread per tile row (4 samples), a 256-thread workgroup = 64 tiles
// = a 32x32 region in Z-order: tiled side fully coalesced, plane side whole 64-byte sectors.
struct ConvJob { // one plane of one picture
  short *plane;
  int stride, w, h;
  TiledPlane T;
};
struct PackRow { // one (level, group)
  uint32_t wave_base;    // index of its first wave-item in the call's descriptor array
  uint32_t n_waves;
  uint32_t item_base[4]; // first entry of each size class in the call's item array
  uint32_t count[4];     // blocks per size class
  uint32_t pad[2];
};
struct PackDesc { // one wave-item
  uint32_t item_off;   // first item
  uint32_t n_s;        // items | size class << 28
  uint32_t row;
  uint32_t dep_target; // wave-items of the previous row of the group (0: nothing to wait for)
};
struct PackHdr {
  uint32_t shard_base[9]; // wave-items of shard s: [shard_base[s], shard_base[s+1])
  uint32_t total_items;
  uint32_t pad0[22];
  uint32_t abort;         // set by a wave whose wait timed out
  uint32_t pad1[31];
  uint32_t ticket[8][32]; // one 128-byte line per shard
  uint32_t owner[8][32];  // 0: unclaimed, x + 1: claimed by XCD x
  // -DHMX_PACK_PROFILE builds only: phases of a wave-item in ticks of the 100 MHz wall clock, summed over all wave-items
  // [0] draw a ticket [1] descriptor [2] item loads issued up to the wait [3] wait for the previous row [4] references +
  // arithmetic + stores issued [5] drain of the stores [6] count; [7] wave-items; [8] polls; [9] waves' lifetimes
  unsigned long long prof[16];
};
struct PackPic { // per picture: where its levels go, and the plan it follows
  int *lev[3];
  int lev_stride[3];
  int n_levels;
  const LevelRow *ltab;
  const FTu *ltus;
  uint32_t *sse[3]; // distortion output per plane (hmx_set_sse_output), NULL = none
};
// (PackGeom and pack_slots: hmx_call_rules.h)

struct hmx_ctx {
  hmx_config cfg;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string err;
  // scratch for the scalar drop-ins (one block): device staging
  char *d_scratch = nullptr;
  size_t scratch_bytes = 0;
  // working pictures of the whole-picture path in tiled layout (TiledGeom): grow-only pools behind the plane-geometry entry
  // points, ONE allocation per direction.  What a single call decides travels in its IntraCall (hmx_chain.hip), not here.
  short *own_pool_org = nullptr, *own_pool_rec = nullptr;
  int pool_pics = 0;
  int own_cw = 0, own_ch = 0;     // CTU grid the pools were sized for
  ConvJob *d_jobs = nullptr;      // [2][n_pics*3]: to-tiled jobs, then from-tiled jobs
  size_t jobs_cap = 0;            // bytes
  // whole-picture calls recorded as HIP graphs (run_graph, hmx_chain.hip)
  struct GraphEntry {
    uint64_t key;
    int n_pics;
    hipGraphExec_t exec;
    PicWork *d_work;
    uint64_t stamp;
  };
  std::vector<GraphEntry> graphs;
  uint64_t graph_clock = 0;
  int last_schedule = 0, last_groups = 1; // of the last whole-picture call (hmx_last_call_shape)
  // optional timing of the last whole-picture call: events around the layout conversions and the chain
  bool timing = false;
  hipEvent_t tev[4] = {};
  hipEvent_t tev_prep = nullptr; // packed schedule: behind the tables' prep kernels, when the timed call rebuilt them
  bool tev_prep_valid = false;
  bool tev_valid = false;
  // level schedule: picture groups run on side streams so that launches of different groups overlap
  static const int kMaxSide = kMaxSideStreams;
  hipStream_t side[kMaxSide] = {};
  // layout conversions pipelined with the chain (across schedule): one stream for the conversions, one event per CTU row
  // and direction, one per (group, CTU row) for "this row is final"
  hipStream_t conv_stream = nullptr;
  std::vector<hipEvent_t> ev_rows; // [ch] converted in, [ch] converted out marker unused, then [groups][ch] row final
  hipEvent_t ev_conv_join = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join[kMaxSide] = {};
  int n_side = 0;
  // Argument arena: small per-call tables (picture planes, job lists) travel through a pinned host ring
  // and a device ring by asynchronous copies; the stream is synchronised only when the ring wraps.
  double *rdoq_wd = nullptr; // RDOQ per-lane records (hmx_rdoq.h), sized for rdoq_T lanes
  int *rdoq_wi = nullptr;
  RdoqBlock *rdoq_blocks = nullptr;
  EstBitsDev *rdoq_est = nullptr;
  int rdoq_T = 0;
  size_t rdoq_est_cap = 0, rdoq_blocks_cap = 0; // bytes
  uint64_t rdoq_key = 0;      // of the block list and tables resident on the device
  bool rdoq_resident = false;
  size_t rdoq_class_n[4] = {0, 0, 0, 0}; // blocks of 32, 16, 8, 4 in the resident list
  uint64_t rdoq_in_key = 0;              // of the caller's arguments that produced the resident list (hmx_batch_xRateDistOptQuant)
  bool rdoq_join[2] = {false, false}; // side streams of the current RDOQ call still to be joined
  double rdoq_consts_h[4] = {};
  bool rdoq_consts_valid = false;
  double *rdoq_consts = nullptr; // k_rdoq_tiles: lambda [luma, chroma], then the Int64 factors of sign hiding
  int *d_mcmap = nullptr; // cell -> PU maps of the last motion-compensation call
  size_t mcmap_cap = 0; // bytes
  unsigned long long *d_me_keys = nullptr; // hmx_batch_fullpel_search: one (cost, raster index) word per unit
  size_t me_keys_cap = 0;
  void *d_wpest = nullptr; // hmx_wp_acdc_multi: the sample sums between its passes; hmx_wp_estimate_slices: the sums it downloads
  size_t wpest_cap = 0;
  void *d_saodec = nullptr; // hmx_sao_decide_multi: the candidate records between its two kernels
  size_t saodec_cap = 0;
  char *arena_h = nullptr, *arena_d = nullptr;
  ArenaCursor arena; // where the next table goes (hmx_arena.h)
  // packed schedule (k_intra_packed): tables of the last call; rebuilt on the device when the pictures / plans change
  struct Packed {
    PackPic *d_pics = nullptr;
    PackRow *d_rows = nullptr;
    PackDesc *d_descs = nullptr;
    FTu *d_items = nullptr;
    uint32_t *d_done = nullptr;
    PackHdr *d_hdr = nullptr;
    size_t cap_pics = 0, cap_rows = 0, cap_descs = 0, cap_items = 0, cap_done = 0;
    uint64_t key = 0;
    bool valid = false;
    PackGeom G{};
    int n_wg = 0;
    uint64_t waves_bound = 0;
  } pk;
  int pk_resident[3] = {0, 0, 0}; // resident waves of the packed kernel's variants on this device, by PackVariant (0: not asked yet)
  bool pk_pending = false;    // a packed launch was issued since the last check of its abort word
  // hmx_set_rdoq: xRateDistOptQuant as the quantiser of the next whole-picture encode calls
  struct ChainRdoq {
    int n = 0;                    // pictures described (1: one set for all pictures of a call); 0 = off
    EstBitsDev *d_est = nullptr;  // [n][2][4]
    size_t cap_est = 0;
    std::vector<double> lambda;   // [n][2]
    double *d_lambda = nullptr;   // [n][2], then the Int64 factors [n][2]
    size_t cap_lambda = 0;
    uint64_t serial = 0;          // counts hmx_set_rdoq calls (part of the schedule key)
    uint64_t lambda_key = 0;      // of the multiplier table resident in d_lambda (serial + quantiser parameters)
    bool lambda_valid = false;
  } crq;
  // hmx_intra_plan_create_device: work buffers (grow-only) and a cache of freed slabs (a pipeline that rebuilds its plans every
  // batch gets the previous batch's memory back instead of a hipMalloc / hipFree pair per call)
  struct PlanDev {
    void *buf[12] = {};
    size_t cap[12] = {};
    unsigned long long *d_need = nullptr; // what a mode reads: [4 sizes][chroma, luma][35 modes] unit masks
    std::vector<std::pair<void *, size_t>> slabs;
  } pd;
  std::vector<hmx_sse> sse_out; // hmx_set_sse_output: per-picture distortion arrays of the next whole-picture encode calls
  // hmx_set_qp_map: a QP per 4x4 luma unit for the whole-picture chain (packed schedule) and the block-list transform entries
  struct QpMap {
    const int8_t *d = nullptr; // the caller's device memory, [n][uh][uw]; NULL = off (hmx_pic_param::qp)
    int n = 0;                 // maps (1: one for every picture of a call)
    uint64_t serial = 0;       // counts hmx_set_qp_map calls (part of the packed schedule's key)
    QuantPk *d_tab = nullptr;  // [52 + QpBDOffset][luma, chroma], built for tab_key
    int tab_key = -1;          // the chroma_qp_offset and the base QP the table was built for
    bool base_on = false;      // hmx_set_qp_map_base: the forward quantiser's right shift follows the slice's base QP
    int base_qp = 0;
  } qm;
  uint64_t table_key = 0;     // of the picture table resident in d_jobs (whole-picture calls)
  bool table_valid = false;
  std::vector<unsigned char> table_bytes; // what table_key was hashed from (the table is re-used only when these bytes are equal)
  uint64_t table_salt = 0;
  // knobs, read once from the environment in hmx_create (A/B runs and the cross-checks of the tests)
  struct Knobs {
    int schedule = -1;     // HMX_INTRA_SCHEDULE: wave / level / packed (default: packed)
    int across = -1;       // HMX_INTRA_ACROSS: 0 keeps shared-plan batches of the level schedule per picture
    int streams = 0;       // HMX_INTRA_STREAMS: picture groups of the across schedule
    bool pipeline_conv = false, graph = false;
    int slots8 = 0;        // HMX_PACK_SLOTS8: 8 or 16 8x8 blocks per wave-item of the packed schedule: eight or four lanes per block (0: by batch size)
    int slots4 = 0;        // HMX_PACK_SLOTS4: 16 or 64 4x4 blocks per wave-item (0: by batch size)
    int pack_group = 0;    // HMX_PACK_GROUP: pictures per group, 1..64 (0: by batch size, see pack_group_size)
    int pack_waves = 0;    // HMX_PACK_WAVES: persistent waves (0: by batch size)
    int pack_sleep0 = -1, pack_sleep1 = -1; // HMX_PACK_SLEEP0 / 1: poll back-off, units of 64 clocks (-1: default)
    bool plan_one_stream = false; // HMX_PLAN_STREAMS=1: the luma and chroma level walks of the device plan builder one after the other (A/B)
    int plan_rows = 0;     // HMX_PLAN_ROWS: rows of the level table per picture the device plan builder starts with (0: from the picture size)
    bool rdoq_lane_only = false; // HMX_RDOQ_LANE: every block through the one-lane-per-block kernel (round 1's, A/B and cross-check)
    int tz_max_passes = 1024;    // HMX_TZ_MAX_PASSES: star-refinement passes of a unit of hmx_batch_tz_search before the all-ones answer, 1..1024
  } knob;
};

// The tables of plans built on the device (hmx_intra_plan_create_device): ONE slab each for the sorted block lists and the
// level tables of all pictures of a call; the plans of the call point into them and share ownership.
struct PlanSet {
  FTu *d_ltus = nullptr;
  LevelRow *d_ltab = nullptr;
  size_t ltus_bytes = 0, ltab_bytes = 0;
  int refs = 0;
};
struct hmx_intra_plan {
  int n_levels = 0;            // picture-wide dependency levels (= level_chunks.size() for plans analysed on the host)
  PlanSet *set = nullptr;      // != NULL: built on the device; d_ltus / d_ltab point into the set's slabs, the other tables do not exist
  int n_diagonals = 0;
  FTu *d_tus = nullptr;
  Seg *d_segs = nullptr;
  uint32_t *d_seg_range = nullptr;
  uint32_t *d_wave_ctus = nullptr;
  std::vector<std::pair<uint32_t, uint32_t>> waves; // offset,count into d_wave_ctus
  FTu *d_ltus = nullptr;       // level schedule
  LevelRow *d_ltab = nullptr;
  std::vector<uint32_t> level_chunks; // waves needed per level
  std::vector<LevelRow> h_ltab;       // host copy of the level table
  uint64_t size_total[4] = {0, 0, 0, 0}; // blocks per transform size
  uint32_t tex_sizes = 0;                 // bit 4 * t + log2n - 2: the plan holds a block of that size in luma (t = 0) / chroma (t = 1)
  uint64_t serial = 0;                    // unique per plan: a freed plan's address may be handed out again
  // per CTU row: the first and the last dependency level that touches it (the layout conversions are pipelined by CTU
  // row: a row is converted in before its first level and out after its last one)
  std::vector<int> row_first_level, row_last_level;
  PicDev P;
  int n_tu = 0;
  int qp = 0, chroma_qp_offset = 0, slice_type = 0;
};

// 4x4 blocks per wave in the across-pictures level schedule: 16 = four lanes per block (one row each, through LDS like the 8x8 and
// 16x16 blocks), 64 = one lane per block (wave_chain_4_lane).  Measured at 1024 pictures of the 2160p mix: four lanes
// +3 % encoder direction, +16 % decoder direction (more, shorter waves); the one-lane form stays for A/B builds.
#ifndef HMX_SLOTS4
#define HMX_SLOTS4 16
#endif
constexpr int kSlots4 = HMX_SLOTS4; // across pictures
constexpr int kSlots4Own = 64;       // per-picture level kernel: one lane per block (four lanes: 51.5 vs 54.5 Gpx/s at 1024 pictures)
int fail(hmx_ctx *c, int code, const char *what, hipError_t e = hipSuccess);
inline int fail(hmx_ctx *c, int code, const std::string &what) { return fail(c, code, what.c_str()); } // messages that name their caller
static const int kQuantScales[6] = {26214, 23302, 20560, 18396, 16384, 14564}; // TComRom.cpp:293
static const int kInvQuantScales[6] = {40, 45, 51, 57, 64, 72};                // TComRom.cpp:298
#define HIPCHK(ctx, call)                                                   \
  do {                                                                      \
    hipError_t e_ = (call);                                                 \
    if (e_ != hipSuccess) return fail(ctx, HMX_ERR_DEVICE, #call, e_);      \
  } while (0)

static inline int ilog2i(int n) {
  int l = 0;
  while ((1 << l) < n) l++;
  return l;
}
// A block list resident on the device, bucketed by block size.
struct hmx_tu_list {
  DTu *d = nullptr;
  int off[5] = {0, 0, 0, 0, 0}, cnt[5] = {0, 0, 0, 0, 0}; // size classes 4 .. 64 (64: luma prediction units, hmx_batch_predIntra[_cost] only)
  int n = 0;
};
// The tiled working layout of the whole-picture path (TiledPlane): planes padded to whole CTUs, ONE allocation per pool, picture i
// at element offset i * pic_elems, its planes at plane_off[]: a wave that works across pictures reaches any picture with a
// multiply-add.  Pictures of one interleave domain [g0, g1) of a pool lie quad by quad beside each other.
struct TiledGeom {
  int ctu = 64, cw = 0, ch = 0, pic_w = 0, pic_h = 0;
  uint32_t plane_off[3] = {0, 0, 0};
  size_t pic_elems = 0;
};
inline TiledGeom tiled_geom(int pic_w, int pic_h, int ctu) {
  TiledGeom g;
  g.ctu = ctu, g.pic_w = pic_w, g.pic_h = pic_h;
  g.cw = (pic_w + ctu - 1) / ctu, g.ch = (pic_h + ctu - 1) / ctu;
  for (int p = 0; p < 3; p++) {
    g.plane_off[p] = (uint32_t)g.pic_elems;
    g.pic_elems += (size_t)g.cw * g.ch * ((size_t)ctu * ctu >> (p ? 2 : 0));
  }
  return g;
}
inline bool operator==(const TiledGeom &a, const TiledGeom &b) { return a.ctu == b.ctu && a.pic_w == b.pic_w && a.pic_h == b.pic_h; } // the rest follows
// plane p of picture i, a member of the interleave domain [g0, g1) of the pool at `pool` (NULL: a pool the call does not have)
inline TiledPlane tiled_plane(const TiledGeom &g, short *pool, int i, int p, int g0, int g1) {
  const int clog = ilog2i(g.ctu);
  const size_t base = (size_t)g0 * g.pic_elems + (size_t)g.plane_off[p] * (g1 - g0) + (size_t)(i - g0) * 64;
  return TiledPlane{pool ? pool + base : nullptr, g.cw, p ? clog - 1 : clog, 64u * (unsigned)(g1 - g0)};
}
// 64 x 64 regions of `rows` sample rows of the padded luma plane (the chroma planes need a quarter of them; the rest exit): the
// grid of k_convert_tiled over n_pics pictures
inline dim3 convert_grid(const TiledGeom &g, int n_pics, int rows) { return dim3((unsigned)n_pics, (unsigned)(g.cw * g.ctu + 63) / 64 * ((unsigned)(rows + 63) / 64), 3); }
struct hmx_tpool {
  short *base = nullptr;
  int n_pics = 0, I = 1;   // groups of I pictures are interleaved quad by quad
  TiledGeom geom;
};
inline TiledPlane tpool_plane(const hmx_tpool *t, int i, int p) { return tiled_plane(t->geom, t->base, i, p, i / t->I * t->I, i / t->I * t->I + t->I); }

// ---- host helpers that cross translation units ----
QuantDev make_qd(const hmx_qp &qp, int per_base, int slice_type);                 // hmx_core.hip
PicDev make_picdev(const hmx_ctx *c, const hmx_pic_param *pp);
PlanesDev to_dev(const hmx_pic *p);
LevelsDev to_dev(const hmx_levels *p);
// The argument arena (placement rule: hmx_arena.h).  A call that puts ONE table before its launch uses arena_push.  A call that puts
// several reserves all of them first -- sizes: the byte counts of its tables, 0 for one it leaves out -- and then places each:
// arena_reserve refuses a call whose tables do not fit the arena together with HMX_ERR_NOMEM and `too_long` as the text, before
// anything is copied; arena_place returns NULL for a table the reservation does not cover, which the entry reports as
// HMX_ERR_INTERNAL (kArenaOutside) -- it is never served by wrapping onto the call's own tables.
int arena_reserve(hmx_ctx *c, std::initializer_list<size_t> sizes, const char *too_long);
void *arena_place(hmx_ctx *c, const void *src, size_t bytes);
void *arena_push(hmx_ctx *c, const void *src, size_t bytes); // NULL: the table alone exceeds the arena, or the copy failed
constexpr const char *kArenaOutside = "argument arena: a table outside what the call reserved";
void drop_graphs(hmx_ctx *c); // destroy every recorded whole-picture graph (the stream is idle)
// a grow-only device buffer of the context: at least `need` bytes behind *p.  Growing waits for the stream, frees the old buffer and
// allocates with some headroom; `what` names the buffer in the HMX_ERR_NOMEM text ("hipMalloc <what>"), *grew (if given) is set when
// the buffer moved, so that the caller drops whatever it believed to be resident in it
int grow_dev(hmx_ctx *c, void **p, size_t *cap, size_t need, const char *what, bool *grew = nullptr);
// the device form of the map set by hmx_set_qp_map for a call over n_pics pictures of pic_w x pic_h: refuses a call with more pictures
// than maps, (re)builds the quantiser table when the chroma offset or the slice type changed                    // hmx_core.hip
int qp_map_for_call(hmx_ctx *c, int n_pics, int pic_w, int pic_h, int chroma_qp_offset, int slice_type, QpMapDev &M);
int check_packed_abort(hmx_ctx *c);                                               // hmx_chain.hip
int pack_group_size(const hmx_ctx *c, int n_pics);
int launch_op(hmx_ctx *c, int op, int log2n, const ListArgs &A);                  // hmx_list.hip
unsigned long long intra_dependency_mask(int n_s, bool luma, int mode, unsigned long long avail); // hmx_plan.hip
bool intra_reads_unavailable(int n_s, bool luma, int mode, unsigned long long avail);             // hmx_plan.hip
bool intra_pads_simple(int n_s, bool luma, int mode, unsigned long long avail);                  // hmx_plan.hip
int plan_host_tables(hmx_ctx *c, const hmx_intra_plan *pl); // device-built plan: fetch the level table for the level schedule / queries
// a slice / tile / CIP layout (hmx_avail_layout) checked against the picture and packed for intra_avail_mask_layout; H.D points
// into H's vectors (host use), layout_to_device puts a copy of the maps in the argument arena (device use)   // hmx_plan.hip
struct LayoutHost {
  std::vector<uint32_t> region, rows, cols;
  AvailDev D{};
};
const char *layout_pack(const hmx_avail_layout *L, int pic_w, int pic_h, int ctu, LayoutHost &H, bool maps_on_device = false);
int layout_to_device(hmx_ctx *c, const LayoutHost &H, AvailDev &D);
// the packed schedule's kernel with RDOQ as the quantiser lives in hmx_chain_rdoq.hip
struct PackArgs;
int packed_rdoq_max_blocks(int *nb);
void launch_packed_rdoq(const PackArgs &A, bool sse, unsigned n_wg, hipStream_t st);
// and the one with a QP per block (hmx_set_qp_map) in hmx_chain_qmap.hip
struct PackArgsQ;
int packed_qmap_max_blocks(int *nb);
void launch_packed_qmap(const PackArgsQ &A, bool enc, bool sse, unsigned n_wg, hipStream_t st);

// the ranges hmx_wp documents for one component of an entry, whichever way it arrives
inline bool wp_range_ok(int weight, int offset, int log2_denom) {
  return weight >= -128 && weight <= 255 && offset >= -128 && offset <= 127 && log2_denom >= 0 && log2_denom <= 7;
}
// one component in the form the prediction weights take (WpEntry, hmx_kernels.h): the offset goes to the bit depth (getWpScaling :286-312)
inline WpEntry wp_entry_make(int weight, int offset, int log2_denom, int B) { return WpEntry{(short)weight, (short)(offset * (1 << (B - 8))), log2_denom}; }// the luma entry of one hmx_wp in the searches' device form (setWpScalingDistParam, TEncSearch.cpp:6183-6215 -> getWpScaling's
// uni-directional branch): false = outside the ranges hmx_wp documents
inline bool me_wp_make(int weight, int offset, int log2_denom, int reserved, int B, MeWp *out) {
  if (!wp_range_ok(weight, offset, log2_denom) || reserved != 0) return false;
  out->w0 = weight, out->shift = log2_denom, out->round = log2_denom ? 1 << (log2_denom - 1) : 0, out->offset = offset * (1 << (B - 8));
  return true;
}
// the table of a _wp search entry (host array parallel to refs[]), refused under the entry's name
inline int me_wp_table(hmx_ctx *c, const char *entry, const hmx_wp *wp, int n_refs, MeWp *out) {
  for (int r = 0; r < n_refs; r++)
    if (!me_wp_make(wp[r].weight[0], wp[r].offset[0], wp[r].log2_denom[0], wp[r].reserved, c->cfg.bit_depth, &out[r]))
      return fail(c, HMX_ERR_ARG, std::string(entry) + ": wp[" + std::to_string(r) +
                                      "]: weight outside -128..255, offset outside -128..127, log2_denom above 7 or reserved not 0");
  return HMX_OK;
}
// ---- what the entries over unit and candidate lists share: the three searches, the sub-pel fan-out, the prediction error ----
inline bool me_size_ok(int v) { return v == 4 || v == 8 || v == 12 || v == 16 || v == 24 || v == 32 || v == 48 || v == 64; }
// The call-level checks, refused under the entry's name: null_arg is the entry's own pointer test (it is reported first, and
// nothing is dereferenced before it), then n, n_refs, the picture, the luma planes and, for wp != NULL, the table of a _wp entry
// into out[] (me_wp_table).
inline int me_call_check(hmx_ctx *c, const char *entry, bool null_arg, int n, const hmx_pic *refs, int n_refs, const hmx_pic *org, int pic_w, int pic_h,
                         int margin_x, int margin_y, const hmx_wp *wp, MeWp *out) {
  const char *why = nullptr;
  if (null_arg) why = ": null argument";
  else if (n <= 0) why = ": n must be at least 1";
  else if (n_refs <= 0 || n_refs > 4) why = ": n_refs must be 1 .. 4";
  else if (pic_w <= 0 || pic_h <= 0 || margin_x < 0 || margin_y < 0) why = ": picture size must be positive and margins not negative";
  else if (!org->plane[0]) why = ": the original has no luma plane";
  else
    for (int r = 0; r < n_refs; r++)
      if (!refs[r].plane[0]) why = ": a reference has no luma plane";
  if (why) return fail(c, HMX_ERR_ARG, std::string(entry) + why);
  return wp ? me_wp_table(c, entry, wp, n_refs, out) : HMX_OK;
}
// One hmx_me_unit against the call: the tail of the refusal, or NULL.  boxed: the search walks the box (sub_shift is honoured, and
// a side is at most 129 = search range 64); the sub-pel refinement only needs the box to hold the integer vector.
inline const char *me_unit_check(const hmx_me_unit &u, int n_refs, int pic_w, int pic_h, bool boxed) {
  if (!me_size_ok(u.w) || !me_size_ok(u.h)) return "width and height come from {4, 8, 12, 16, 24, 32, 48, 64}";
  if (u.ref >= n_refs) return "reference index outside refs[]";
  if (boxed && (u.sub_shift > 1 || (u.sub_shift && u.h <= 8))) return "sub_shift is 0, or 1 with more than 8 rows";
  if (u.right < u.left || u.bottom < u.top) return "empty search box";
  if (boxed && (u.right - u.left + 1 > 129 || u.bottom - u.top + 1 > 129)) return "search box side above 129 (search range 64)";
  if (u.x + u.w > pic_w || u.y + u.h > pic_h) return "the unit lies outside the picture";
  return nullptr;
}
// the margin test, a unit's last: the unit's block displaced by every vector of [l, r] x [t, b] lies inside the reference's margins
inline bool me_reach_ok(const hmx_me_unit &u, int l, int t, int r, int b, int pic_w, int pic_h, int margin_x, int margin_y) {
  return u.x + l >= -margin_x && u.x + r + u.w <= pic_w + margin_x && u.y + t >= -margin_y && u.y + b + u.h <= pic_h + margin_y;
}
inline int me_unit_refuse(hmx_ctx *c, const char *entry, int i, const char *why) { // the text is built only here
  return fail(c, HMX_ERR_ARG, std::string(entry) + ": unit " + std::to_string(i) + ": " + why);
}
// The launch tail.  The kernels are templates over their argument type and the weighted struct derives from the plain one, so that
// the unweighted instantiation keeps the argument block it had before the weighted one existed: launch(A) as ARGSWP or as PLAIN.
template <class PLAIN, class ARGSWP, typename F>
inline void launch_plain_or_wp(bool weighted, const ARGSWP &A, F &&launch) {
  if (weighted) launch(A);
  else launch(static_cast<const PLAIN &>(A));
}
// the same for the searches' structs, with the fields they share filled first: refs[], org, B and the table me_call_check made
template <class PLAIN, class ARGSWP, typename F>
inline void me_launch(const hmx_ctx *c, ARGSWP &A, const hmx_pic *refs, int n_refs, const hmx_pic *org, bool weighted, const MeWp *wpt, F &&launch) {
  for (int r = 0; r < n_refs; r++) A.refs[r] = to_dev(&refs[r]);
  A.org = to_dev(org);
  A.B = c->cfg.bit_depth;
  for (int r = 0; r < 4; r++) A.wp[r] = wpt[r];
  launch_plain_or_wp<PLAIN>(weighted, A, launch);
}

// ---- scalar drop-ins: one block through the batch kernels (host pointers in and out) ----
struct Scratch { // carve the context's device scratch (the budget: head of this file); the first failure sticks in r
  hmx_ctx *c;
  size_t off = 0, tail = 0;
  int r = HMX_OK;
  void claim(size_t front, size_t back) {
    if (front + back > c->scratch_bytes) r = r ? r : fail(c, HMX_ERR_NOMEM, "device scratch: the block does not fit");
    else off = front, tail = back;
  }
  template <typename T>
  T *take(size_t n) {
    const size_t at = (off + 255) & ~(size_t)255;
    claim(at + n * sizeof(T), tail);
    return r ? nullptr : reinterpret_cast<T *>(c->d_scratch + at);
  }
  template <typename T>
  T *take_tail(size_t n) { // from the end of the scratch: stays claimed across rewind()
    claim(off, (tail + n * sizeof(T) + 255) & ~(size_t)255);
    return r ? nullptr : reinterpret_cast<T *>(c->d_scratch + c->scratch_bytes - tail);
  }
  void rewind() { off = 0; } // the next staging round of the same call re-uses the front
  template <typename T>
  T *up(const T *src, int w, int h, size_t src_stride_elems); // take w x h and fill it from a host block
  template <typename T>
  T *up(const T *src, size_t n);                              // the same for n contiguous elements
};
constexpr size_t scratch_need(std::initializer_list<size_t> carves) { // the front after these carves, in bytes
  size_t off = 0;
  for (size_t b : carves) off = ((off + 255) & ~(size_t)255) + b;
  return off;
}
constexpr size_t kScratchBytes = 1 << 20, kMcTail = 2 * 64 * 64 * sizeof(short); // what hmx_create allocates; hmx_motionCompensation's tail
static_assert(scratch_need({129 * 129 * 2, 2 * 129 * 129 * 4}) <= kScratchBytes &&                        // initAdiPattern, 64x64
                  scratch_need({135 * 128 * 2, 128 * 128 * 2}) <= kScratchBytes &&                          // filters, 128x128
                  scratch_need({128 * 128 * 2, 128 * 128 * 2, 128 * 128 * 2}) <= kScratchBytes &&           // addAvg, 128x128
                  scratch_need({32 * 32 * 4, 32 * 32 * 4, 32 * 32 * 4, 32 * 32 * 8, 4}) <= kScratchBytes && // RDOQ with tables, 32x32
                  scratch_need({71 * 71 * 2, 64 * 71 * 2, 64 * 64 * 2}) + kMcTail <= kScratchBytes,         // motion compensation
              "the worst-case carve of every scalar drop-in fits the device scratch");

inline int up2d(hmx_ctx *c, void *dst, const void *src, size_t elem, int w, int h, size_t src_stride_elems) {
  HIPCHK(c, hipMemcpy2DAsync(dst, w * elem, src, src_stride_elems * elem, w * elem, h, hipMemcpyHostToDevice, c->stream));
  return HMX_OK;
}
inline int down2d(hmx_ctx *c, void *dst, size_t dst_stride_elems, const void *src, size_t elem, int w, int h) {
  HIPCHK(c, hipMemcpy2DAsync(dst, dst_stride_elems * elem, src, w * elem, w * elem, h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HMX_OK;
}
template <typename T>
T *Scratch::up(const T *src, int w, int h, size_t src_stride_elems) {
  T *d = take<T>((size_t)w * h);
  if (!r) r = up2d(c, d, src, sizeof(T), w, h, src_stride_elems);
  return d;
}
template <typename T>
T *Scratch::up(const T *src, size_t n) {
  T *d = take<T>(n);
  if (!r) r = hmx_upload(c, d, src, n * sizeof(T));
  return d;
}

// One n x n block through a list kernel: its descriptor goes up behind the staged buffers, and the dense buffers (NULL = unused)
// sit at the origin of `plane` in the four plane slots of the launch.
inline int run_one(hmx_ctx *c, Scratch &s, int op, int n, int plane, unsigned mode, unsigned flags, const PicDev &P, short *a, short *b,
                   int *lev, int *lev2, uint32_t *abs_sum = nullptr) {
  DTu h{};
  h.t.x = h.t.y = 0;
  h.t.log2n = (uint8_t)ilog2i(n);
  h.t.plane = (uint8_t)plane;
  h.t.mode = (uint8_t)(mode > 255 ? 255 : mode);
  h.t.flags = (uint8_t)flags;
  h.idx = 0;
  ListArgs A{};
  A.tus = s.up(&h, 1); // synchronises: h is a stack object
  if (s.r) return s.r;
  A.n = 1;
  A.P = P;
  A.a.p[plane] = a, A.b.p[plane] = b, A.lev.p[plane] = lev, A.lev2.p[plane] = lev2;
  A.a.s[plane] = a ? n : 0, A.b.s[plane] = b ? n : 0, A.lev.s[plane] = lev ? n : 0, A.lev2.s[plane] = lev2 ? n : 0;
  A.abs_sum = abs_sum;
  return launch_op(c, op, ilog2i(n), A);
}

// f(std::integral_constant<int, N>{}) for the block size N of 4, 8, 16, 32 and (Max = 64) 64 that equals n; false, and no call, for
// any other n.  The size-templated kernels are launched through it: one argument list per kernel family.
template <int Max, typename F>
inline bool with_size(int n, F &&f) {
  static_assert(Max == 32 || Max == 64, "block sizes end at 32 or at 64");
  switch (n) {
  case 4: f(std::integral_constant<int, 4>{}); return true;
  case 8: f(std::integral_constant<int, 8>{}); return true;
  case 16: f(std::integral_constant<int, 16>{}); return true;
  case 32: f(std::integral_constant<int, 32>{}); return true;
  case 64:
    if constexpr (Max == 64) {
      f(std::integral_constant<int, 64>{});
      return true;
    }
  }
  return false;
}
// f(std::true_type{}) or f(std::false_type{}): a kernel with a bool template parameter (encoder / decoder direction) launched from a
// run-time flag, one argument list for both
template <typename F>
inline void with_bool(bool b, F &&f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// the launch of one kernel family for an n x n block (a size the caller has checked), and its launch error
template <int Max, typename F>
inline int launch_sized(hmx_ctx *c, int n, F &&launch) {
  if (!with_size<Max>(n, launch)) return fail(c, HMX_ERR_ARG, "unsupported block size");
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
inline bool size_ok(int w, int h) { return w == h && (w == 4 || w == 8 || w == 16 || w == 32); }
// intra prediction also runs at 64 x 64, the prediction unit of a 64 x 64 coding unit (TComPrediction.cpp:343-345 asserts 4..128)
inline bool size_ok_intra(int w, int h) { return size_ok(w, h) || (w == 64 && h == 64); }

inline PicDev scalar_picdev(hmx_ctx *c, const hmx_qp *qp, int per_base, int slice_type, int sign_hide) {
  PicDev P{};
  P.pic_w = P.pic_h = 1 << 14;
  P.ctu = c->cfg.ctu_size;
  P.bit_depth = c->cfg.bit_depth;
  P.sign_hide = sign_hide;
  hmx_qp q = qp ? *qp : hmx_qp{0, 0, 0, 15};
  P.qd[0] = P.qd[1] = make_qd(q, per_base, slice_type);
  return P;
}
