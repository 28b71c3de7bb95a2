// hmx_chain.hip: whole-picture all-intra chain -- schedules, resident pools, entry points -- part of libhmx (include/hmx.h), gfx950.  See hmx_host.h for how the library is cut into translation units.
#define HMX_CHAIN_MAIN 1
#include "hmx_chain_dev.h"

// =============================================================================================
// Packed schedule: ONE persistent launch per whole-picture call.
//
// The level schedules pay one kernel launch per picture-wide dependency level (4844 at 2160p) and every launch lasts at
// least one block-chain latency however little work it carries.  Here the dependency order lives in memory instead:
//   * pictures form GROUPS of I <= 64 (the interleave domain of the working pool); a ROW = (dependency level, group)
//     holds every block of that level of the group's pictures -- each picture following ITS OWN plan -- bucketed by
//     transform size.  A WAVE-ITEM is one wave's worth of a bucket: 64/N blocks (one 32x32 block) taken from whichever
//     pictures have them, so waves are full whether the pictures share a plan or not (per item: picture + descriptor);
//   * groups are dealt to SHARDS (group mod n_shards, at most 8); the wave-items of a shard are numbered row after row,
//     level-major (tickets).  A persistent wave draws the next ticket of its shard with an atomic add, WAITS until the
//     previous row of the same group is complete (one counter per row, polled with an L1-bypassing load), runs the
//     block chain, drains its stores and adds 1 to its row's counter.
// A shard belongs to ONE XCD: the first wave that touches it claims it for the XCD it runs on (compare-and-swap on the
// shard's owner word with the hardware's XCC id; a wave starts at the shard with its XCD's number, moves on to shards its
// XCD already owns or that nobody owns when those are drained, and never works on another XCD's).  So every producer and
// every consumer of a group's reconstruction runs on the same XCD BY CONSTRUCTION -- read from the hardware, not assumed
// from the dispatch order -- and the hand-off stays inside that XCD's L2: plain stores (the vector L1 is write-through;
// a store whose vmcnt has drained is in the L2), loads that bypass the L1 (sc1), no write-through to HBM and no round
// trip to it on the dependency path.  An XCD is a 32-CU machine with its own L2; this schedule runs eight of them side
// by side on independent pictures.
// Forward progress: a wave waits only for wave-items with SMALLER tickets of the same shard, and a ticket is drawn by a
// wave that is already running, in ticket order.  So the unfinished wave-item with the smallest ticket of a shard is always
// held by a running wave whose own dependencies are complete: it finishes, and by induction all do, whatever the number of
// resident waves, the dispatch order or the placement (an XCD that gets no wave of the launch owns nothing: its shards
// are claimed by the waves of another XCD once those have drained their own).  There is no barrier between workgroups.
// (A spin that exceeds ~2^22 polls -- seconds -- raises the abort word and every wave leaves: a bug fails loudly.)
// Rows of different groups are independent, so while one group waits for its row's last wave-item the others compute.
// Latency hiding inside a wave: the ticket, the descriptor and the items of the NEXT wave-item are fetched while the current
// one runs (ticket drawn before the chain, descriptor loaded behind the dependency poll, items loaded behind the chain's
// stores), so that a wave-item starts with its block descriptors in registers.
// Reference for the dependency a row encodes: TLibCommon/TComPattern.cpp:389-425 (which neighbours a block reads).
// =============================================================================================
// after a synchronisation: did a wave of the packed schedule give up waiting (its bounded spin ran out)?
int check_packed_abort(hmx_ctx *c) {
  if (!c->pk_pending || !c->pk.d_hdr) return HMX_OK;
  c->pk_pending = false;
#ifdef HMX_PACK_PROFILE
  {
    unsigned long long pr[16];
    HIPCHK(c, hipMemcpy(pr, c->pk.d_hdr->prof, sizeof(pr), hipMemcpyDeviceToHost));
    const double n = pr[7] ? (double)pr[7] : 1.0;
    fprintf(stderr, "[pack profile] last call: %llu wave-items, per item (us): ticket %.2f desc %.2f pre-wait %.2f wait %.2f (%.1f polls) chain %.2f drain %.2f count %.2f; "
                    "wave lifetime %.1f us avg over %d waves\n", pr[7], pr[0] / n / 100, pr[1] / n / 100, pr[2] / n / 100, pr[3] / n / 100, pr[8] / n, pr[4] / n / 100,
            pr[5] / n / 100, pr[6] / n / 100, c->pk.n_wg ? pr[9] / 100.0 / c->pk.n_wg : 0.0, c->pk.n_wg);
    unsigned long long rq[40], zero[40] = {};
    HIPCHK(c, hipMemcpyFromSymbol(rq, HIP_SYMBOL(g_rdoq_prof), sizeof(rq)));
    HIPCHK(c, hipMemcpyToSymbol(HIP_SYMBOL(g_rdoq_prof), zero, sizeof(zero)));
    if (rq[9]) fprintf(stderr, "[rdoq profile] 4x4 in a lane: %llu blocks, %.2f us each\n", rq[9], rq[0] / (double)rq[9] / 100);
    for (int g = 1; g < 4; g++)
      if (rq[g * 10 + 9]) {
        const double m = (double)rq[g * 10 + 9] * 100;
        fprintf(stderr, "[rdoq profile] %dx%d: %llu wave calls, us per call: prep %.2f walk8 %.2f resolve %.2f walk %.2f lastpos %.2f levels %.2f signhide %.2f store %.2f\n",
                4 << g, 4 << g, rq[g * 10 + 9], rq[g * 10] / m, rq[g * 10 + 1] / m, rq[g * 10 + 2] / m, rq[g * 10 + 3] / m, rq[g * 10 + 4] / m, rq[g * 10 + 5] / m,
                rq[g * 10 + 6] / m, rq[g * 10 + 7] / m);
      }
  }
#endif
  uint32_t ab = 0;
  HIPCHK(c, hipMemcpy(&ab, &c->pk.d_hdr->abort, sizeof(ab), hipMemcpyDeviceToHost));
  if (!ab) return HMX_OK;
  HIPCHK(c, hipMemset(&c->pk.d_hdr->abort, 0, sizeof(ab))); // read and reported: the next call starts clean
  return fail(c, HMX_ERR_DEVICE, "packed schedule: a dependency wait timed out, the outputs of every call since the last hmx_sync are invalid");
}
// Everything frame_intra decides for ONE whole-picture call: what the caller passed, the schedule it resolved to, the pools it
// works on and, once uploaded, its tables on the device.  The issue_* functions read it and nothing else about the call; the
// context keeps only what outlives a call (what it owns, what it caches, what reports on the last call).
struct IntraCall {
  bool enc, onto, resident;
  const hmx_intra_plan *const *plans; // picture i follows plans[i * plan_stride] (stride 0: one plan for all)
  int plan_stride, n_pics;
  const hmx_levels *lev;              // the caller's array, valid while the call is issued
  int schedule;                       // 3 packed, 2 level across pictures, 1 level per picture, 0 wave (hmx_last_call_shape)
  bool across, pipeline_conv;         // level schedule: SIMD across pictures; its conversions pipelined by CTU row
  int groups, I;                      // stream groups of the level schedule; pictures per group of the packed one
  TiledGeom geom;
  short *pool_org, *pool_rec;         // the context's own pools or the caller's (hmx_tpool)
  const PicWork *d_work;
  const ConvJob *d_jobs;              // [2][n_pics * 3]: to-tiled jobs, then from-tiled jobs
  bool qmap;                          // a QP per block (hmx_set_qp_map): qm is the map in its device form
  QpMapDev qm;
  bool packed() const { return schedule == 3; }
  bool use_level() const { return schedule == 1 || schedule == 2; }
  const hmx_intra_plan *plan(int i) const { return plans[i * plan_stride]; }
  // the interleave domain of the pool is a group of I pictures (packed), a stream group (across), one picture
  int group_first(int g) const { return (int)((long long)n_pics * g / groups); }           // stream group g = [first(g), first(g + 1))
  int group_of(int i) const { return (int)(((long long)(i + 1) * groups - 1) / n_pics); } // the g with first(g) <= i < first(g + 1)
};
// Issue the launches of one whole-picture call on `main` (and the side streams).  Also used under
// stream capture to record the call as a HIP graph.
static int issue_chain_launches(hmx_ctx *c, const IntraCall &k, hipStream_t main);

// ---- packed schedule, host side: the steps of one call around the rules of hmx_call_rules.h (issue_packed puts them together) ----
enum PackVariant { kPackPlain = 0, kPackRdoq = 1, kPackQmap = 2 }; // which instantiation family of k_intra_packed the call launches
struct PackedCall { // what the packed call decides
  PackVariant variant;
  PackShape S;        // pack_shape over the totals of the call's plans
  uint32_t tex_sizes; // hmx_intra_plan::tex_sizes of all plans, or-ed
  bool want_sse;      // the distortion output (hmx_set_sse_output) covers this call
};
static PackedCall packed_shape(const hmx_ctx *c, const IntraCall &k) {
  PackedCall pc{};
  pc.variant = k.enc && c->crq.n > 0 ? kPackRdoq : k.qmap ? kPackQmap : kPackPlain;
  pc.want_sse = k.enc && (int)c->sse_out.size() >= k.n_pics;
  uint64_t items = 0, sz[4] = {0, 0, 0, 0};
  int max_levels = 0;
  for (int i = 0; i < k.n_pics; i++) {
    const hmx_intra_plan *pl = k.plan(i);
    max_levels = std::max(max_levels, pl->n_levels);
    items += (uint64_t)pl->n_tu;
    for (int s = 0; s < 4; s++) sz[s] += pl->size_total[s];
    pc.tex_sizes |= pl->tex_sizes;
  }
  pc.S = pack_shape(k.n_pics, k.I, c->knob.slots4, c->knob.slots8, pc.variant == kPackRdoq, k.qmap, max_levels, sz, items);
  return pc;
}
// RDOQ as the quantiser: what hmx_set_rdoq described fits the call, and no level can leave the 16-bit words it travels in
static int packed_rdoq_checks(hmx_ctx *c, const IntraCall &k, const PackedCall &pc) {
  const PicDev &P = k.plans[0]->P;
  if (c->crq.n != 1 && c->crq.n != k.n_pics) return fail(c, HMX_ERR_ARG, "frame_intra: hmx_set_rdoq described another number of pictures");
  if (pc.S.G.I > kRdoqMaxGroup) return fail(c, HMX_ERR_ARG, "frame_intra: RDOQ keeps the bit-estimate tables of a packing group in LDS: at most 2 pictures per group (HMX_PACK_GROUP)");
  // Inside the kernel RDOQ's levels travel as 16-bit words (hmx_rdoq.h): a call in which one can exceed them (rdoq_levels_fit16) is
  // refused (the scalar and block-list entries send such calls through the one-lane-per-block kernel, whose levels are 32-bit:
  // include/hmx.h).  Luma and chroma have QPs of their own: a size counts for the texture type that holds a block of it (32x32
  // luma beside a lower chroma QP does not make a 32x32 chroma block).  The plans of a call share the picture parameters (the
  // kernel takes them from the first): so does this check, over the sizes of all of them.
  for (int t = 0; t < 2; t++)
    for (int lg = 2; lg <= 5; lg++)
      if (((pc.tex_sizes >> (4 * t + lg - 2)) & 1) && !rdoq_levels_fit16(P.qd[t].q, P.qd[t].per_qbits, P.bit_depth, lg))
        return fail(c, HMX_ERR_ARG, "frame_intra: RDOQ in the chain keeps levels in 16 bits; this QP / bit depth / block size can exceed them (raise the QP or use the flat quantiser)");
  return HMX_OK;
}
// The per-picture table of the prep kernels and of the chain: where a picture's levels and distortions go, the plan it follows
static int upload_pack_pics(hmx_ctx *c, const IntraCall &k, const PackedCall &pc, hipStream_t st) {
  std::vector<PackPic> hp(k.n_pics);
  for (int i = 0; i < k.n_pics; i++) {
    const hmx_intra_plan *pl = k.plan(i);
    for (int p = 0; p < 3; p++) hp[i].lev[p] = k.lev[i].plane[p], hp[i].lev_stride[p] = k.lev[i].stride[p];
    hp[i].n_levels = pl->n_levels;
    hp[i].ltab = pl->d_ltab;
    hp[i].ltus = pl->d_ltus;
    for (int p = 0; p < 3; p++) hp[i].sse[p] = pc.want_sse ? c->sse_out[i].plane[p] : nullptr;
  }
  HIPCHK(c, hipMemcpyAsync(c->pk.d_pics, hp.data(), sizeof(PackPic) * k.n_pics, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st)); // hp goes out of scope
  return HMX_OK;
}
// The tables: kept while the call's pictures, plans and shape are the last call's, else sized and rebuilt on the device
static int packed_tables(hmx_ctx *c, const IntraCall &k, const PackedCall &pc, hipStream_t st) {
  auto &pk = c->pk;
  const PackGeom &G = pc.S.G;
  const uint64_t n_rows = pc.S.n_rows;
  c->tev_prep_valid = false;
  if (pk.valid && pk.key == c->table_key && pk.G.n_pics == G.n_pics && pk.G.I == G.I && pk.G.slots4 == G.slots4 && pk.G.slots8 == G.slots8 &&
      pk.G.max_levels == G.max_levels)
    return HMX_OK;
  pk.valid = false;
  const char *what = "packed schedule tables";
  int r = grow_dev(c, (void **)&pk.d_pics, &pk.cap_pics, sizeof(PackPic) * k.n_pics, what);
  if (!r) r = grow_dev(c, (void **)&pk.d_descs, &pk.cap_descs, sizeof(PackDesc) * pc.S.waves_bound, what);
  if (!r) r = grow_dev(c, (void **)&pk.d_items, &pk.cap_items, sizeof(FTu) * pc.S.items, what);
  if (!r) r = grow_dev(c, (void **)&pk.d_rows, &pk.cap_rows, sizeof(PackRow) * n_rows, what);
  if (!r) r = grow_dev(c, (void **)&pk.d_done, &pk.cap_done, std::max<size_t>(sizeof(uint32_t) * kDoneStride * n_rows, sizeof(uint32_t) * 2 * kPackScanWgs), what); // (also k_pack_scan's scratch)
  if (!r && !pk.d_hdr) {
    if (hipMalloc((void **)&pk.d_hdr, sizeof(PackHdr)) != hipSuccess) r = fail(c, HMX_ERR_NOMEM, "hipMalloc packed header");
    else if (hipMemsetAsync(pk.d_hdr, 0, sizeof(PackHdr), st) != hipSuccess) r = fail(c, HMX_ERR_DEVICE, "hipMemsetAsync packed header");
  }
  if (r) return r;
  if (int e = upload_pack_pics(c, k, pc, st)) return e;
  HIPCHK(c, hipMemsetAsync(pk.d_hdr, 0, offsetof(PackHdr, abort), st)); // everything but the sticky abort word (packed_clear)
  const unsigned prep_waves = (unsigned)((n_rows + (uint64_t)(64 / G.I) - 1) / (uint64_t)(64 / G.I));
  hipLaunchKernelGGL(k_pack_count, dim3(prep_waves), dim3(64), 0, st, pk.d_pics, pk.d_rows, G, (int)n_rows);
  // (the completion counters are cleared behind the prep kernels: their array doubles as the scan's scratch)
  hipLaunchKernelGGL(k_pack_scan<false>, dim3(kPackScanWgs), dim3(1024), 0, st, pk.d_rows, pk.d_hdr, G, pk.d_done);
  hipLaunchKernelGGL(k_pack_scan<true>, dim3(kPackScanWgs), dim3(1024), 0, st, pk.d_rows, pk.d_hdr, G, pk.d_done);
  hipLaunchKernelGGL(k_pack_fill, dim3((unsigned)((G.max_levels + kPackFillLevels - 1) / kPackFillLevels), (unsigned)G.n_groups), dim3(256), 0, st, pk.d_pics, pk.d_rows, pk.d_descs, pk.d_items, G);
  HIPCHK(c, hipGetLastError());
  if (c->timing && c->tev_prep) {
    HIPCHK(c, hipEventRecord(c->tev_prep, st));
    c->tev_prep_valid = true;
  }
  pk.key = c->table_key;
  pk.G = G;
  pk.waves_bound = pc.S.waves_bound;
  pk.valid = true;
  return HMX_OK;
}
// What starts from zero every call: the completion counters and the ticket and owner words
static int packed_clear(hmx_ctx *c, const PackedCall &pc, hipStream_t st) {
  HIPCHK(c, hipMemsetAsync(c->pk.d_done, 0, sizeof(uint32_t) * kDoneStride * pc.S.n_rows, st));
  // The abort word is STICKY: it is cleared only by check_packed_abort after the host has read it (hmx_sync / hmx_download).
  // Calls queued behind a call whose dependency wait timed out see it set, leave at once and the next hmx_sync reports it --
  // a per-call clear would let call k+1 erase the failure of call k.
  HIPCHK(c, hipMemsetAsync(c->pk.d_hdr->ticket, 0, sizeof(PackHdr) - offsetof(PackHdr, ticket), st));
  return HMX_OK;
}
// Resident waves of a variant of the packed kernel on this device: the runtime is asked once per context and variant.  (The RDOQ and
// QP-map instantiations live in units of their own, which answer for them.)
static int resident_waves(hmx_ctx *c, PackVariant v, int &resident) {
  if (!c->pk_resident[v]) {
    int nb = 0;
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->cfg.device));
    if (v == kPackPlain) HIPCHK(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_intra_packed<true, 64>, 64, 0));
    if (v == kPackRdoq && packed_rdoq_max_blocks(&nb)) return fail(c, HMX_ERR_DEVICE, "hipOccupancyMaxActiveBlocksPerMultiprocessor(k_intra_packed, RDOQ)");
    if (v == kPackQmap && packed_qmap_max_blocks(&nb)) return fail(c, HMX_ERR_DEVICE, "hipOccupancyMaxActiveBlocksPerMultiprocessor(k_intra_packed_qmap)");
    c->pk_resident[v] = std::max(64, nb * prop.multiProcessorCount);
  }
  resident = c->pk_resident[v];
  return HMX_OK;
}
// The kernel's arguments but for RDOQ's.  The level planes of the call are addressed as ONE slab when they lie at equal distances
// with equal strides (a picture's planes then come from a multiply-add instead of the picture table)
static PackArgs packed_args(const hmx_ctx *c, const IntraCall &k, const PackedCall &pc) {
  const auto &pk = c->pk;
  PackArgs A{};
  A.pics = pk.d_pics, A.rows = pk.d_rows, A.descs = pk.d_descs, A.items = pk.d_items, A.done = pk.d_done, A.hdr = pk.d_hdr;
  A.pool_org = k.pool_org, A.pool_rec = k.pool_rec;
  A.pic_elems = k.geom.pic_elems;
  for (int p = 0; p < 3; p++) A.plane_off[p] = k.geom.plane_off[p];
  A.ctu_w = k.geom.cw;
  A.clog = ilog2i(k.geom.ctu);
  A.n_groups = pc.S.G.n_groups, A.n_shards = pc.S.G.n_shards, A.I = pc.S.G.I;
  A.want_sse = pc.want_sse;
  const hmx_levels *lv = k.lev;
  bool slab = true;
  for (int p = 0; p < 3 && slab; p++) {
    const ptrdiff_t d = k.n_pics > 1 ? (const char *)lv[1].plane[p] - (const char *)lv[0].plane[p] : 0;
    slab = d >= 0 && d % (ptrdiff_t)sizeof(int) == 0;
    for (int i = 0; i < k.n_pics && slab; i++)
      slab = (const char *)lv[i].plane[p] == (const char *)lv[0].plane[p] + (ptrdiff_t)i * d && lv[i].stride[p] == lv[0].stride[p];
    A.lev_base[p] = lv[0].plane[p];
    A.lev_pic_elems[p] = d / (ptrdiff_t)sizeof(int);
    A.lev_stride[p] = lv[0].stride[p];
  }
  A.lev_slab = slab ? 1 : 0;
  A.sleep0 = c->knob.pack_sleep0 >= 0 ? c->knob.pack_sleep0 : 16;
  A.sleep1 = c->knob.pack_sleep1 >= 0 ? c->knob.pack_sleep1 : 2;
  A.P = k.plans[0]->P;
  return A;
}
// RDOQ's arguments: the error scale per size, and per picture lambda and the factor of the sign-hiding cost (rdoq_err_scale,
// rdoq_rd_factor: the quotients in the reference's operation order)
static int packed_rdoq_args(hmx_ctx *c, const IntraCall &k, PackArgs &A, hipStream_t st) {
  auto &q = c->crq;
  const int B = A.P.bit_depth;
  std::vector<double> up((size_t)q.n * 4);
  for (int t = 0; t < 2; t++) {
    const int per = A.P.qd[t].per_qbits, iq = A.P.qd[t].iq_scale >> per;
    for (int lg = 2; lg <= 5; lg++) A.rq.err_scale[t][lg - 2] = rdoq_err_scale(B, A.P.qd[t].q, lg);
    for (int i = 0; i < q.n; i++) {
      const double lam = q.lambda[(size_t)i * 2 + t];
      up[(size_t)i * 2 + t] = lam;
      const long long f = rdoq_rd_factor(iq, per, lam, B);
      memcpy(&up[(size_t)q.n * 2 + (size_t)i * 2 + t], &f, sizeof(f));
    }
  }
  // The table depends on hmx_set_rdoq's multipliers and the call's quantiser parameters only: it goes up when one of them changed
  // (the first call after hmx_set_rdoq, or another QP), so that steady-state calls queue behind each other without a host wait.
  uint64_t lkey = 1469598103934665603ull ^ q.serial;
  for (int t = 0; t < 2; t++)
    for (int v : {A.P.qd[t].q, A.P.qd[t].per_qbits, A.P.qd[t].iq_scale, B, q.n}) lkey = (lkey ^ (uint64_t)(uint32_t)v) * 1099511628211ull;
  if (!q.lambda_valid || q.lambda_key != lkey) {
    HIPCHK(c, hipMemcpyAsync(q.d_lambda, up.data(), up.size() * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st)); // `up` goes out of scope
    q.lambda_key = lkey, q.lambda_valid = true;
  }
  A.rq.est = q.d_est;
  A.rq.lambda = q.d_lambda;
  A.rq.rd_factor = reinterpret_cast<const long long *>(q.d_lambda + (size_t)q.n * 2);
  A.rq.pic_mul = q.n == 1 ? 0 : 1;
  A.rq.n_pics = k.n_pics;
  return HMX_OK;
}
// The launch: n_wg persistent waves of the call's variant
static int packed_launch(hmx_ctx *c, const IntraCall &k, const PackedCall &pc, const PackArgs &A, hipStream_t st) {
  const PackGeom &G = pc.S.G;
  const dim3 grid((unsigned)c->pk.n_wg), blk(64);
  if (pc.variant == kPackRdoq) {
    launch_packed_rdoq(A, A.want_sse != 0, grid.x, st); // hmx_chain_rdoq.hip
  } else if (pc.variant == kPackQmap) {
    PackArgsQ AQ{};
    static_cast<PackArgs &>(AQ) = A;
    AQ.qm = k.qm;
    launch_packed_qmap(AQ, k.enc, A.want_sse != 0, grid.x, st); // hmx_chain_qmap.hip
  } else {
    with_bool(k.enc, [&](auto enc_t) {
      with_bool(A.want_sse != 0, [&](auto sse_t) {
        constexpr bool E = decltype(enc_t)::value, S = decltype(sse_t)::value;
        if constexpr (E || !S) { // the distortion output exists in the encoder direction only
          if (G.slots8 == 16) hipLaunchKernelGGL((k_intra_packed<E, 64, S, false, 16>), grid, blk, 0, st, A); // (then slots4 is 64)
          else if (G.slots4 == 64) hipLaunchKernelGGL((k_intra_packed<E, 64, S>), grid, blk, 0, st, A);
          else hipLaunchKernelGGL((k_intra_packed<E, 16, S>), grid, blk, 0, st, A);
        }
      });
    });
  }
  HIPCHK(c, hipGetLastError());
  c->pk_pending = true;
  return HMX_OK;
}
static int issue_packed(hmx_ctx *c, const IntraCall &k, hipStream_t st) {
  const PackedCall pc = packed_shape(c, k);
  if (pc.variant == kPackRdoq)
    if (int r = packed_rdoq_checks(c, k, pc)) return r;
  if (pc.S.too_large) return fail(c, HMX_ERR_ARG, "frame_intra: batch too large for one packed call (split it)");
  if (int r = packed_tables(c, k, pc, st)) return r;
  if (int r = packed_clear(c, pc, st)) return r;
  int resident = 0;
  if (int r = resident_waves(c, pc.variant, resident)) return r;
  c->pk.n_wg = pack_wave_count(c->knob.pack_waves, resident, pc.S.waves_bound, pc.S.G.max_levels);
  PackArgs A = packed_args(c, k, pc);
  if (pc.variant == kPackRdoq)
    if (int r = packed_rdoq_args(c, k, A, st)) return r;
  return packed_launch(c, k, pc, A, st);
}
// The packed schedule's tables of the last call, copied out for the test that checks them against the plans (include/hmx.h has
// the record layouts).  Reads only: neither the tables nor the cache key nor the sticky abort word change.
extern "C" int hmx_last_call_pack_tables(hmx_ctx *c, hmx_pack_geom *geom, void *hdr, void *rows, void *descs, void *items, uint32_t *done) {
  if (!c || !geom) return fail(c, HMX_ERR_ARG, "hmx_last_call_pack_tables: bad argument");
  const auto &pk = c->pk;
  if (c->last_schedule != 3 || !pk.valid || !pk.d_hdr)
    return fail(c, HMX_ERR_ARG, "hmx_last_call_pack_tables: the last whole-picture call did not run the packed schedule, or its tables are not valid");
  static_assert(sizeof(PackRow) == 48 && sizeof(PackDesc) == 16 && sizeof(FTu) == 16 && offsetof(PackHdr, total_items) == 36, "record layouts documented in include/hmx.h");
  HIPCHK(c, hipStreamSynchronize(c->stream));
  uint32_t h[12] = {};
  HIPCHK(c, hipMemcpy(h, pk.d_hdr, 10 * sizeof(uint32_t), hipMemcpyDeviceToHost)); // shard_base[9], total_items
  HIPCHK(c, hipMemcpy(&h[10], &pk.d_hdr->abort, sizeof(uint32_t), hipMemcpyDeviceToHost));
  const size_t n_rows = (size_t)pk.G.max_levels * pk.G.n_groups;
  if (h[8] > pk.waves_bound || (size_t)h[8] * sizeof(PackDesc) > pk.cap_descs || (size_t)h[9] * sizeof(FTu) > pk.cap_items || n_rows * sizeof(PackRow) > pk.cap_rows)
    return fail(c, HMX_ERR_DEVICE, "hmx_last_call_pack_tables: the header's totals exceed the tables");
  geom->n_pics = pk.G.n_pics, geom->I = pk.G.I, geom->n_groups = pk.G.n_groups, geom->n_shards = pk.G.n_shards;
  geom->max_levels = pk.G.max_levels, geom->slots4 = pk.G.slots4, geom->slots8 = pk.G.slots8;
  geom->n_rows = (int)n_rows, geom->n_waves = (int)h[8], geom->n_items = (int)h[9];
  if (hdr) memcpy(hdr, h, sizeof(h));
  if (rows && n_rows) HIPCHK(c, hipMemcpy(rows, pk.d_rows, sizeof(PackRow) * n_rows, hipMemcpyDeviceToHost));
  if (descs && h[8]) HIPCHK(c, hipMemcpy(descs, pk.d_descs, sizeof(PackDesc) * h[8], hipMemcpyDeviceToHost));
  if (items && h[9]) {
    HIPCHK(c, hipMemcpy(items, pk.d_items, sizeof(FTu) * h[9], hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < h[9]; i++) static_cast<FTu *>(items)[i].avail_hi &= ~kFtuFlagBits; // the caller gets the mask alone
  }
  if (done && n_rows) // word 0 of every row's 128-byte counter line
    HIPCHK(c, hipMemcpy2D(done, sizeof(uint32_t), pk.d_done, sizeof(uint32_t) * kDoneStride, sizeof(uint32_t), n_rows, hipMemcpyDeviceToHost));
  return HMX_OK;
}

// ---- level schedules: picture groups on side streams, forked from and joined into `main` through events ----
static int fork_groups(hmx_ctx *c, int groups, hipStream_t main) { // the groups start after what is already on main
  HIPCHK(c, hipEventRecord(c->ev_fork, main));
  for (int g = 0; g < groups; g++) HIPCHK(c, hipStreamWaitEvent(c->side[g], c->ev_fork, 0));
  return HMX_OK;
}
static int join_groups(hmx_ctx *c, int groups, hipStream_t main) {
  for (int g = 0; g < groups; g++) {
    HIPCHK(c, hipEventRecord(c->ev_join[g], c->side[g]));
    HIPCHK(c, hipStreamWaitEvent(main, c->ev_join[g], 0));
  }
  return HMX_OK;
}
// One plan for every picture: SIMD across pictures (k_intra_level_across); every group of pictures is its own interleave
// domain of the pool (see build_tables) and walks the levels on its own stream.  What the launches of a call share ...
static AcrossArgs across_args(const IntraCall &k) {
  AcrossArgs AA{};
  AA.ltus = k.plans[0]->d_ltus;
  AA.pic_elems = k.geom.pic_elems;
  for (int p = 0; p < 3; p++) AA.plane_off[p] = k.geom.plane_off[p];
  AA.ctu_w = k.geom.cw;
  AA.clog = ilog2i(k.geom.ctu);
  AA.P = k.plans[0]->P;
  return AA;
}
// ... and the launch of dependency level l for picture group g on `st`
static int launch_across_level(hmx_ctx *c, const IntraCall &k, AcrossArgs AA, size_t l, int g, hipStream_t st) {
  const int first = k.group_first(g), np = k.group_first(g + 1) - first;
  if (np <= 0) return HMX_OK;
  AA.row = k.plans[0]->h_ltab[l];
  AA.pics = k.d_work + first;
  AA.n_pics = np;
  AA.pool_org = k.pool_org + (size_t)first * k.geom.pic_elems;
  AA.pool_rec = k.pool_rec + (size_t)first * k.geom.pic_elems;
  uint64_t waves = 0;
  for (int s = 0; s < 4; s++) {
    const int slots = s == 0 ? kSlots4 : s == 1 ? 8 : s == 2 ? 4 : 1;
    AA.cpb[s] = (uint32_t)((np + slots - 1) / slots);
    waves += (uint64_t)AA.row.count[s] * AA.cpb[s];
  }
  if (!waves) return HMX_OK;
  if (waves > 0x7fffffffull) return fail(c, HMX_ERR_ARG, "frame_intra: level too large for one launch");
  with_bool(k.enc, [&](auto E) { hipLaunchKernelGGL(k_intra_level_across<E>, dim3((unsigned)waves), dim3(64), 0, st, AA); });
  return HMX_OK;
}

// The across schedule with the layout conversions pipelined by CTU row.  The chain is latency-bound and leaves the
// memory system idle; the conversions are pure traffic.  CTU row r is converted in (stream `conv`) before the first
// dependency level that touches it and converted out after the last one, so both conversions hide behind the chain:
//   conv:   in(0) in(1) ... in(R-1)            wait(final 0) out(0)  wait(final 1) out(1) ...
//   group:  wait(in 0) level 0 ... wait(in r) level first[r] ... level last[r] record(final r) ...
static int issue_across_pipelined(hmx_ctx *c, const IntraCall &k, hipStream_t main) {
  const hmx_intra_plan *p0 = k.plans[0];
  const int ctu = k.geom.ctu, ch = k.geom.ch, groups = k.groups;
  int prio_lo = 0, prio_hi = 0; // the conversions are background traffic: lowest priority, the chain highest
  hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
  if (!c->conv_stream) HIPCHK(c, hipStreamCreateWithPriority(&c->conv_stream, hipStreamNonBlocking, prio_lo));
  if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  if (!c->ev_conv_join) HIPCHK(c, hipEventCreateWithFlags(&c->ev_conv_join, hipEventDisableTiming));
  for (int g = c->n_side; g < groups; g++) {
    HIPCHK(c, hipStreamCreateWithPriority(&c->side[g], hipStreamNonBlocking, prio_hi));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[g], hipEventDisableTiming));
    c->n_side = g + 1;
  }
  const size_t need = (size_t)ch * (1 + groups);
  while (c->ev_rows.size() < need) {
    hipEvent_t e;
    HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->ev_rows.push_back(e);
  }
  hipEvent_t *ev_in = c->ev_rows.data(), *ev_final = c->ev_rows.data() + ch; // ev_final[g * ch + r]
  hipStream_t conv = c->conv_stream;
  const dim3 cgrid = convert_grid(k.geom, k.n_pics, ctu); // one CTU row
  if (int r = fork_groups(c, groups, main)) return r;
  HIPCHK(c, hipStreamWaitEvent(conv, c->ev_fork, 0)); // the conversions too start after what is already on main
  if (c->timing) HIPCHK(c, hipEventRecord(c->tev[1], main)); // conversion-in is not a separate phase any more
  if (k.enc)
    for (int r = 0; r < ch; r++) {
      hipLaunchKernelGGL(k_convert_tiled<true>, cgrid, dim3(256), 0, conv, k.d_jobs, r * ctu, (r + 1) * ctu);
      HIPCHK(c, hipEventRecord(ev_in[r], conv));
    }
  const AcrossArgs AA = across_args(k);
  // rows in the order their first level comes up / their last level passes
  std::vector<int> by_first(ch), by_last(ch);
  for (int r = 0; r < ch; r++) by_first[r] = by_last[r] = r;
  std::stable_sort(by_first.begin(), by_first.end(), [&](int a, int b) { return p0->row_first_level[a] < p0->row_first_level[b]; });
  std::stable_sort(by_last.begin(), by_last.end(), [&](int a, int b) { return p0->row_last_level[a] < p0->row_last_level[b]; });
  int nf = 0, nl = 0;
  const size_t n_levels = p0->h_ltab.size();
  for (size_t l = 0; l < n_levels; l++) {
    if (k.enc)
      for (; nf < ch && p0->row_first_level[by_first[nf]] <= (int)l; nf++)
        for (int g = 0; g < groups; g++) HIPCHK(c, hipStreamWaitEvent(c->side[g], ev_in[by_first[nf]], 0));
    for (int g = 0; g < groups; g++)
      if (int r = launch_across_level(c, k, AA, l, g, c->side[g])) return r;
    for (; nl < ch && p0->row_last_level[by_last[nl]] <= (int)l; nl++) { // these rows are final: convert them out
      const int r = by_last[nl];
      for (int g = 0; g < groups; g++) {
        HIPCHK(c, hipEventRecord(ev_final[g * ch + r], c->side[g]));
        HIPCHK(c, hipStreamWaitEvent(conv, ev_final[g * ch + r], 0));
      }
      hipLaunchKernelGGL(k_convert_tiled<false>, cgrid, dim3(256), 0, conv, k.d_jobs + (size_t)k.n_pics * 3, r * ctu, (r + 1) * ctu);
    }
  }
  if (int r = join_groups(c, groups, main)) return r;
  if (c->timing) HIPCHK(c, hipEventRecord(c->tev[2], main)); // the chain is done
  HIPCHK(c, hipEventRecord(c->ev_conv_join, conv));
  HIPCHK(c, hipStreamWaitEvent(main, c->ev_conv_join, 0));
  return HMX_OK;
}

static int issue_intra_launches(hmx_ctx *c, const IntraCall &k, hipStream_t main) {
  // original planes -> tiled working copies (encode), chain, tiled reconstruction -> caller's planes
  const dim3 cgrid = convert_grid(k.geom, k.n_pics, k.geom.ch * k.geom.ctu);
  const ConvJob *jobs_rec = k.d_jobs + (size_t)k.n_pics * 3;
  const bool tm = c->timing;
  if (tm) HIPCHK(c, hipEventRecord(c->tev[0], main));
  if (k.across && k.pipeline_conv) {
    if (int r = issue_across_pipelined(c, k, main)) return r;
  } else {
    const bool conv = !k.resident;
    if (conv && k.enc) hipLaunchKernelGGL(k_convert_tiled<true>, cgrid, dim3(256), 0, main, k.d_jobs, 0, 1 << 30);
    if (conv && k.onto) // the pool starts from the caller's reconstruction (the inter-coded parts of the picture)
      hipLaunchKernelGGL(k_convert_tiled<true>, cgrid, dim3(256), 0, main, jobs_rec, 0, 1 << 30);
    if (tm) HIPCHK(c, hipEventRecord(c->tev[1], main));
    if (int r = k.packed() ? issue_packed(c, k, main) : issue_chain_launches(c, k, main)) return r;
    if (tm) HIPCHK(c, hipEventRecord(c->tev[2], main));
    if (conv) hipLaunchKernelGGL(k_convert_tiled<false>, cgrid, dim3(256), 0, main, jobs_rec, 0, 1 << 30);
  }
  if (tm) {
    HIPCHK(c, hipEventRecord(c->tev[3], main));
    c->tev_valid = true;
  }
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

static int issue_chain_launches(hmx_ctx *c, const IntraCall &k, hipStream_t main) {
  const hmx_intra_plan *p0 = k.plans[0];
  const int groups = k.groups;
  if (!k.use_level()) { // one launch per CTU diagonal, autonomous waves
    FrameArgs A;
    A.pics = k.d_work;
    A.P = p0->P;
    for (auto &w : p0->waves) {
      if (!w.second) continue;
      A.wave_ctus = p0->d_wave_ctus + w.first;
      A.n_wave_ctus = (int)w.second;
      const dim3 grid((unsigned)(w.second * k.n_pics * 3));
      with_bool(k.enc, [&](auto E) { hipLaunchKernelGGL(k_intra_wave<E>, grid, dim3(64), 0, main, A); });
    }
    HIPCHK(c, hipGetLastError());
    return HMX_OK;
  }
  // Pictures are split into groups; each group walks its levels on its own stream.  A launch
  // of one group fills only part of the chip (its duration is one block-chain latency), so
  // launches of different groups overlap.
  if (groups > 1)
    if (int r = fork_groups(c, groups, main)) return r;
  auto stream_of = [&](int g) { return groups > 1 ? c->side[g] : main; };
  std::vector<size_t> glevels(groups, 0);
  size_t n_levels = 0;
  for (int g = 0; g < groups; g++) {
    for (int i = k.group_first(g); i < k.group_first(g + 1); i++) glevels[g] = std::max(glevels[g], (size_t)k.plan(i)->n_levels);
    n_levels = std::max(n_levels, glevels[g]);
  }
  if (k.across) {
    const AcrossArgs AA = across_args(k);
    for (size_t l = 0; l < n_levels; l++)
      for (int g = 0; g < groups; g++)
        if (int r = launch_across_level(c, k, AA, l, g, stream_of(g))) return r;
  } else {
    LevelArgs LA{};
    LA.P = p0->P;
    for (size_t l = 0; l < n_levels; l++)
      for (int g = 0; g < groups; g++) {
        if (l >= glevels[g]) continue;
        const int first = k.group_first(g), end = k.group_first(g + 1);
        uint32_t chunks = 0;
        if (k.plan_stride == 0)
          chunks = p0->level_chunks[l];
        else
          for (int i = first; i < end; i++) {
            const auto &lc = k.plan(i)->level_chunks;
            if (l < lc.size()) chunks = std::max(chunks, lc[l]);
          }
        if (!chunks) continue;
        LA.pics = k.d_work + first;
        LA.level = (int)l;
        LA.shared = k.plan_stride == 0;
        if (LA.shared) {
          LA.row = p0->h_ltab[l];
          LA.ltus = p0->d_ltus;
        }
        const dim3 grid(chunks, (unsigned)(end - first));
        with_bool(k.enc, [&](auto E) { hipLaunchKernelGGL(k_intra_level<E>, grid, dim3(64), 0, stream_of(g), LA); });
      }
  }
  if (groups > 1)
    if (int r = join_groups(c, groups, main)) return r;
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}

// Pictures per group of the packed schedule for this context's knob and RDOQ setting (the rule: pack_group_rule, hmx_call_rules.h)
int pack_group_size(const hmx_ctx *c, int n_pics) { return pack_group_rule(c ? c->knob.pack_group : 0, c && c->crq.n > 0, n_pics); }
// ---- pictures resident in the working layout (include/hmx.h: hmx_tpool) ----
extern "C" int hmx_tpool_create(hmx_ctx *c, int pic_w, int pic_h, int n_pics, hmx_tpool **out) {
  if (!c || !out || pic_w <= 0 || pic_h <= 0 || n_pics <= 0) return fail(c, HMX_ERR_ARG, "hmx_tpool_create: bad argument");
  hmx_tpool *t = new hmx_tpool;
  t->geom = tiled_geom(pic_w, pic_h, c->cfg.ctu_size);
  t->n_pics = n_pics;
  t->I = pack_group_size(c, n_pics);
  const size_t slots = (size_t)(n_pics + t->I - 1) / t->I * t->I;
  if (hipMalloc((void **)&t->base, t->geom.pic_elems * 2 * slots) != hipSuccess) {
    delete t;
    return fail(c, HMX_ERR_NOMEM, "hipMalloc resident pictures");
  }
  *out = t;
  return HMX_OK;
}
extern "C" void hmx_tpool_destroy(hmx_ctx *c, hmx_tpool *t) {
  if (!t) return;
  if (c) {
    hipStreamSynchronize(c->stream);
    c->table_valid = false; // a later pool may get the same address
    c->pk.valid = false;
  }
  hipFree(t->base);
  delete t;
}
static int tpool_convert(hmx_ctx *c, const hmx_tpool *t, int first, int n, const hmx_pic *planes, bool to_tiled) {
  if (!c || !t || !planes || first < 0 || n <= 0 || first + n > t->n_pics) return fail(c, HMX_ERR_ARG, "hmx_tpool import/export: bad argument");
  std::vector<ConvJob> jobs((size_t)n * 3);
  for (int i = 0; i < n; i++)
    for (int p = 0; p < 3; p++)
      jobs[(size_t)i * 3 + p] = ConvJob{planes[i].plane[p], planes[i].stride[p], t->geom.pic_w >> (p ? 1 : 0), t->geom.pic_h >> (p ? 1 : 0), tpool_plane(t, first + i, p)};
  // through the argument arena, a few thousand jobs at a time.  Each part is launched before the next is pushed, so arena_push's
  // own one-table reservation is enough: a part that wraps waits for the launches of the parts before it (hmx_arena.h)
  for (size_t done = 0; done < jobs.size();) {
    const size_t part = std::min(jobs.size() - done, (size_t)3 * 8192);
    const ConvJob *d = static_cast<const ConvJob *>(arena_push(c, jobs.data() + done, sizeof(ConvJob) * part));
    if (!d) return fail(c, HMX_ERR_NOMEM, "argument arena");
    const dim3 grid = convert_grid(t->geom, (int)(part / 3), t->geom.ch * t->geom.ctu);
    with_bool(to_tiled, [&](auto T) { hipLaunchKernelGGL(k_convert_tiled<T>, grid, dim3(256), 0, c->stream, d, 0, 1 << 30); });
    done += part;
  }
  HIPCHK(c, hipGetLastError());
  return HMX_OK;
}
extern "C" int hmx_tpool_import(hmx_ctx *c, hmx_tpool *t, int first, int n, const hmx_pic *src) { return tpool_convert(c, t, first, n, src, true); }
extern "C" int hmx_tpool_export(hmx_ctx *c, const hmx_tpool *t, int first, int n, const hmx_pic *dst) { return tpool_convert(c, t, first, n, dst, false); }

// ---- one whole-picture call, step by step (frame_intra below puts the steps together) ----
// What the call resolves to -- schedule, groups, group size, geometry -- and whether its pools and plans fit that.
static int resolve_call(hmx_ctx *c, IntraCall &k, const hmx_tpool *torg, const hmx_tpool *trec) {
  const hmx_intra_plan *p0 = k.plans[0];
  const CallSchedule s = resolve_schedule(k.resident, k.plan_stride, k.n_pics, k.onto, c->knob); // the rule: hmx_call_rules.h
  const bool packed = s.schedule == 3, use_level = s.schedule == 1 || s.schedule == 2;
  k.schedule = s.schedule, k.across = s.across, k.groups = s.groups, k.pipeline_conv = s.pipeline_conv;
  // packed: groups of I pictures are the interleave domains of the pool and the lanes of the tables' prep kernels
  k.I = k.resident ? trec->I : packed ? pack_group_size(c, k.n_pics) : 1;
  k.geom = tiled_geom(p0->P.pic_w, p0->P.pic_h, p0->P.ctu);
  if (k.resident) // the caller's pools: same geometry as the plans, at least n_pics pictures, one interleave
    for (const hmx_tpool *t : {trec, k.enc ? torg : trec})
      if (!(t->geom == k.geom) || t->n_pics < k.n_pics || t->I != k.I)
        return fail(c, HMX_ERR_ARG, "frame_intra: resident pool does not match the call (picture size, CTU size, pictures, group size)");
  c->last_schedule = k.schedule;
  c->last_groups = k.groups;
  for (int i = 0; i < k.n_pics; i++) {
    const hmx_intra_plan *pl = k.plan(i);
    if (!pl || pl->P.pic_w != p0->P.pic_w || pl->P.pic_h != p0->P.pic_h || pl->qp != p0->qp ||
        pl->chroma_qp_offset != p0->chroma_qp_offset || pl->slice_type != p0->slice_type ||
        pl->P.sign_hide != p0->P.sign_hide)
      return fail(c, HMX_ERR_ARG, "frame_intra: plans of one call must share picture size and quantiser settings");
    if (pl->set && !packed) { // built on the device: the packed schedule's tables only
      if (!use_level) return fail(c, HMX_ERR_ARG, "frame_intra: a plan built on the device has no tables for the wave schedule (HMX_INTRA_SCHEDULE=packed|level)");
      if (int r = plan_host_tables(c, pl)) return r; // the level schedule walks the level table on the host
      k.pipeline_conv = false;                       // (no per-CTU-row level ranges either)
    }
  }
  return HMX_OK;
}
// The pools the call works on: the caller's resident ones, or the context's own (one slot per picture, grown when the call needs more)
static int ensure_pools(hmx_ctx *c, IntraCall &k, const hmx_tpool *torg, const hmx_tpool *trec) {
  if (k.resident) {
    k.pool_org = k.enc ? torg->base : nullptr;
    k.pool_rec = trec->base;
    return HMX_OK;
  }
  const int pool_need = k.packed() ? (k.n_pics + k.I - 1) / k.I * k.I : k.n_pics;
  if (c->own_cw != k.geom.cw || c->own_ch != k.geom.ch || c->pool_pics < pool_need) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipFree(c->own_pool_org);
    hipFree(c->own_pool_rec);
    c->own_pool_org = c->own_pool_rec = nullptr;
    c->pool_pics = 0;
    c->own_cw = k.geom.cw, c->own_ch = k.geom.ch;
    c->table_valid = false;
    c->pk.valid = false;
    if (hipMalloc((void **)&c->own_pool_org, k.geom.pic_elems * 2 * pool_need) != hipSuccess ||
        hipMalloc((void **)&c->own_pool_rec, k.geom.pic_elems * 2 * pool_need) != hipSuccess) {
      hipFree(c->own_pool_org);
      c->own_pool_org = nullptr;
      return fail(c, HMX_ERR_NOMEM, "hipMalloc tiled working pictures");
    }
    c->pool_pics = pool_need;
  }
  k.pool_org = c->own_pool_org, k.pool_rec = c->own_pool_rec;
  return HMX_OK;
}
// The side streams and events of the level schedule's picture groups
static int ensure_side_streams(hmx_ctx *c, const IntraCall &k) {
  if (!k.use_level() || k.groups <= 1 || c->n_side >= k.groups) return HMX_OK;
  if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
  for (int g = c->n_side; g < k.groups; g++) {
    HIPCHK(c, hipStreamCreateWithFlags(&c->side[g], hipStreamNonBlocking));
    HIPCHK(c, hipEventCreateWithFlags(&c->ev_join[g], hipEventDisableTiming));
  }
  c->n_side = k.groups;
  return HMX_OK;
}
// The picture table (hw) and the conversion jobs of the call: to-tiled jobs of the originals, then the jobs of the reconstruction
static void build_tables(const IntraCall &k, const hmx_pic *org, const hmx_pic *rec, std::vector<PicWork> &hw, std::vector<ConvJob> &jobs) {
  hw.resize(k.n_pics);
  jobs.resize((size_t)k.n_pics * 6);
  for (int i = 0; i < k.n_pics; i++) {
    const hmx_intra_plan *pl = k.plan(i);
    // interleave domain [g0, g1) of picture i: a stream group (across), a group of I pictures (packed), itself
    int g0 = i, g1 = i + 1;
    if (k.packed()) g0 = i / k.I * k.I, g1 = g0 + k.I;
    else if (k.across) g0 = k.group_first(k.group_of(i)), g1 = k.group_first(k.group_of(i) + 1);
    memset(&hw[i], 0, sizeof(PicWork));
    for (int p = 0; p < 3; p++) {
      const int pw = k.geom.pic_w >> (p ? 1 : 0), ph = k.geom.pic_h >> (p ? 1 : 0);
      hw[i].org[p] = tiled_plane(k.geom, k.pool_org, i, p, g0, g1);
      hw[i].rec[p] = tiled_plane(k.geom, k.pool_rec, i, p, g0, g1);
      hw[i].lev[p] = k.lev[i].plane[p];
      hw[i].lev_stride[p] = k.lev[i].stride[p];
      if (!k.resident) {
        if (k.enc) jobs[(size_t)i * 3 + p] = ConvJob{org[i].plane[p], org[i].stride[p], pw, ph, hw[i].org[p]};
        jobs[(size_t)(k.n_pics + i) * 3 + p] = ConvJob{rec[i].plane[p], rec[i].stride[p], pw, ph, hw[i].rec[p]};
      }
    }
    hw[i].tus = pl->d_tus;
    hw[i].segs = pl->d_segs;
    hw[i].seg_range = pl->d_seg_range;
    hw[i].ltus = pl->d_ltus;
    hw[i].ltab = pl->d_ltab;
    hw[i].n_levels = pl->n_levels;
  }
}
// Key of the call = the picture table itself (planes, level buffers, plans, schedule).  A steady-state pipeline
// re-uses its picture pools: the device copy of the table (and the packed schedule's tables) is then kept as it is,
// and the call is queued behind the previous one without any synchronisation.
// kb: the bytes the key is formed from: two calls are "the same" when these are, not when a hash says so
static int table_key_of(hmx_ctx *c, const IntraCall &k, const std::vector<PicWork> &hw, const std::vector<ConvJob> &jobs, uint64_t &key,
                        std::vector<unsigned char> &kb) {
  key = 1469598103934665603ull;
  kb.reserve(sizeof(PicWork) * k.n_pics + sizeof(ConvJob) * jobs.size() + 24 * (size_t)k.n_pics + 64);
  auto mix = [&](const void *p, size_t n) { // FNV-1a over 8-byte words (the table of a 2048-picture call is ~1 MB, hashed on every call)
    const unsigned char *b = (const unsigned char *)p;
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
      uint64_t w8;
      memcpy(&w8, b + i, 8);
      key = (key ^ w8) * 1099511628211ull;
    }
    for (; i < n; i++) key = (key ^ b[i]) * 1099511628211ull;
    kb.insert(kb.end(), b, b + n);
  };
  mix(hw.data(), sizeof(PicWork) * k.n_pics);
  mix(jobs.data(), sizeof(ConvJob) * jobs.size());
  const int flags[6] = {k.enc, k.schedule, k.groups, k.n_pics, k.across, k.I};
  mix(flags, sizeof(flags));
  if (k.enc && c->crq.n > 0) {
    if (!k.packed()) return fail(c, HMX_ERR_ARG, "frame_intra: RDOQ as the quantiser (hmx_set_rdoq) needs the packed schedule");
    mix(&c->crq.serial, sizeof(c->crq.serial)); // 4x4 blocks then always go one per lane: another table
  }
  if (k.qmap) { // another wave-item shape, another kernel: never the tables of a call without a map by accident
    const int on = 1;
    mix(&on, sizeof(on));
  }
  if (k.enc && (int)c->sse_out.size() >= k.n_pics) {
    if (!k.packed()) return fail(c, HMX_ERR_ARG, "frame_intra: the distortion output (hmx_set_sse_output) needs the packed schedule");
    mix(c->sse_out.data(), sizeof(hmx_sse) * k.n_pics);
  }
  for (int i = 0; i < k.n_pics; i++) {
    const hmx_intra_plan *pp = k.plan(i);
    mix(&pp, sizeof(pp));
    mix(&pp->serial, sizeof(pp->serial)); // a destroyed plan's address may come back
  }
  if (c->table_valid && c->table_key == key && c->table_bytes != kb) // two different calls, one hash: never mistake one for the other
    key = key * 1099511628211ull + ++c->table_salt;
  return HMX_OK;
}
// Eager path: the tables go into ONE grow-only allocation of the context, and only when they are not the ones already there
static int upload_table(hmx_ctx *c, IntraCall &k, const std::vector<PicWork> &hw, const std::vector<ConvJob> &jobs, uint64_t key,
                        std::vector<unsigned char> &kb) {
  const size_t work_bytes = sizeof(PicWork) * k.n_pics, table_bytes = work_bytes + sizeof(ConvJob) * jobs.size();
  bool grew = false;
  const int r = grow_dev(c, (void **)&c->d_jobs, &c->jobs_cap, table_bytes, "picture table", &grew);
  if (grew) c->table_valid = false;
  if (r) return r;
  char *base = reinterpret_cast<char *>(c->d_jobs);
  if (!c->table_valid || c->table_key != key) {
    // earlier calls may still read the table: the copies are ordered behind them on the stream; the host vectors go
    // out of scope, hence the synchronisation -- on this path only
    HIPCHK(c, hipMemcpyAsync(base, hw.data(), work_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + work_bytes, jobs.data(), sizeof(ConvJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->table_key = key;
    c->table_bytes.swap(kb);
    c->table_valid = true;
  }
  k.d_work = reinterpret_cast<const PicWork *>(base);
  k.d_jobs = reinterpret_cast<const ConvJob *>(base + work_bytes);
  return HMX_OK;
}
// HMX_GRAPH (level and wave schedules; measured: replay is not faster than eager launches here): the call is recorded as a HIP
// graph with a table of its own and replayed when the same call comes again; the six most recently used graphs are kept
static int run_graph(hmx_ctx *c, IntraCall &k, const std::vector<PicWork> &hw, const std::vector<ConvJob> &jobs, uint64_t key) {
  for (auto &e : c->graphs)
    if (e.key == key && e.n_pics == k.n_pics) {
      e.stamp = ++c->graph_clock;
      HIPCHK(c, hipGraphLaunch(e.exec, c->stream));
      return HMX_OK;
    }
  PicWork *d_work = nullptr;
  const size_t work_bytes = sizeof(PicWork) * k.n_pics, table_bytes = work_bytes + sizeof(ConvJob) * jobs.size();
  if (hipMalloc((void **)&d_work, table_bytes) != hipSuccess) return fail(c, HMX_ERR_NOMEM, "hipMalloc picture table");
  HIPCHK(c, hipMemcpyAsync(d_work, hw.data(), work_bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(reinterpret_cast<char *>(d_work) + work_bytes, jobs.data(), sizeof(ConvJob) * jobs.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream)); // hw / jobs go out of scope
  k.d_work = d_work;
  k.d_jobs = reinterpret_cast<const ConvJob *>(reinterpret_cast<char *>(d_work) + work_bytes);
  hipGraph_t graph = nullptr;
  HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
  int r = issue_intra_launches(c, k, c->stream);
  hipError_t ce = hipStreamEndCapture(c->stream, &graph);
  if (r != HMX_OK || ce != hipSuccess) {
    if (graph) hipGraphDestroy(graph);
    hipFree(d_work);
    return r != HMX_OK ? r : fail(c, HMX_ERR_DEVICE, "hipStreamEndCapture", ce);
  }
  hipGraphExec_t exec = nullptr;
  ce = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  hipGraphDestroy(graph);
  if (ce != hipSuccess) {
    hipFree(d_work);
    return fail(c, HMX_ERR_DEVICE, "hipGraphInstantiate", ce);
  }
  if (c->graphs.size() >= 6) { // evict the least recently used entry
    size_t v = 0;
    for (size_t i = 1; i < c->graphs.size(); i++)
      if (c->graphs[i].stamp < c->graphs[v].stamp) v = i;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hipGraphExecDestroy(c->graphs[v].exec);
    hipFree(c->graphs[v].d_work);
    c->graphs.erase(c->graphs.begin() + v);
  }
  c->graphs.push_back(hmx_ctx::GraphEntry{key, k.n_pics, exec, d_work, ++c->graph_clock});
  HIPCHK(c, hipGraphLaunch(exec, c->stream));
  return HMX_OK;
}

// org / rec: pictures in plane geometry (converted into / out of the context's own working pools around the chain), or
// NULL with torg / trec: pictures resident in the working layout (no conversion; packed schedule only).
// onto: the call reconstructs onto what the reconstruction planes already hold
static int frame_intra(hmx_ctx *c, const hmx_intra_plan *const *plans, int plan_stride, int n_pics, const hmx_pic *org,
                       const hmx_pic *rec, const hmx_levels *lev, bool enc, bool onto = false, const hmx_tpool *torg = nullptr,
                       const hmx_tpool *trec = nullptr) {
  const bool resident = trec != nullptr;
  if (!c || !plans || !plans[0] || n_pics <= 0 || !lev || (!resident && (!rec || (enc && !org))) || (resident && enc && !torg))
    return fail(c, HMX_ERR_ARG, "frame_intra: null argument");
  IntraCall k{};
  k.enc = enc, k.onto = onto, k.resident = resident;
  k.plans = plans, k.plan_stride = plan_stride, k.n_pics = n_pics, k.lev = lev;
  if (int r = resolve_call(c, k, torg, trec)) return r;
  if (c->qm.d) { // a QP per block (hmx_set_qp_map): refused here, before anything is launched, where the call cannot honour the map
    if (enc && c->crq.n > 0)
      return fail(c, HMX_ERR_ARG, "frame_intra: a QP map (hmx_set_qp_map) with RDOQ (hmx_set_rdoq): lambda and the bit estimates are per picture, the reference changes lambda with the QP");
    if (!k.packed())
      return fail(c, HMX_ERR_ARG, k.use_level() ? "frame_intra: a QP map (hmx_set_qp_map) needs the packed schedule; this call resolved to the level schedule, which takes one QP per call"
                                                : "frame_intra: a QP map (hmx_set_qp_map) needs the packed schedule; this call resolved to the wave schedule, which takes one QP per call");
    const hmx_intra_plan *p0 = plans[0];
    if (int r = qp_map_for_call(c, n_pics, p0->P.pic_w, p0->P.pic_h, p0->chroma_qp_offset, p0->slice_type, k.qm)) return r;
    k.qmap = true;
  }
  if (int r = ensure_pools(c, k, torg, trec)) return r;
  std::vector<PicWork> hw;
  std::vector<ConvJob> jobs;
  build_tables(k, org, rec, hw, jobs);
  if (int r = ensure_side_streams(c, k)) return r;
  uint64_t key = 0;
  std::vector<unsigned char> kb;
  if (int r = table_key_of(c, k, hw, jobs, key, kb)) return r;
  if (c->knob.graph && !k.packed()) return run_graph(c, k, hw, jobs, key);
  if (int r = upload_table(c, k, hw, jobs, key, kb)) return r;
  return issue_intra_launches(c, k, c->stream);
}

extern "C" int hmx_frame_intra_encode(hmx_ctx *c, const hmx_intra_plan *pl, int n_pics, const hmx_pic *org,
                                      const hmx_pic *rec, const hmx_levels *lev) {
  return frame_intra(c, &pl, 0, n_pics, org, rec, lev, true);
}
extern "C" int hmx_frame_intra_decode(hmx_ctx *c, const hmx_intra_plan *pl, int n_pics, const hmx_pic *rec,
                                      const hmx_levels *lev) {
  return frame_intra(c, &pl, 0, n_pics, nullptr, rec, lev, false);
}
extern "C" int hmx_frame_intra_decode_onto(hmx_ctx *c, const hmx_intra_plan *pl, int n_pics, const hmx_pic *rec,
                                           const hmx_levels *lev) {
  if (!c) return HMX_ERR_ARG;
  if (c->knob.graph) return fail(c, HMX_ERR_ARG, "hmx_frame_intra_decode_onto: not available with HMX_GRAPH");
  return frame_intra(c, &pl, 0, n_pics, nullptr, rec, lev, false, true);
}
extern "C" int hmx_frame_intra_encode_onto(hmx_ctx *c, const hmx_intra_plan *pl, int n_pics, const hmx_pic *org, const hmx_pic *rec,
                                           const hmx_levels *lev) {
  if (!c) return HMX_ERR_ARG;
  if (c->knob.graph) return fail(c, HMX_ERR_ARG, "hmx_frame_intra_encode_onto: not available with HMX_GRAPH");
  return frame_intra(c, &pl, 0, n_pics, org, rec, lev, true, true);
}
extern "C" int hmx_frame_intra_encode_multi(hmx_ctx *c, const hmx_intra_plan *const *plans, int n_pics, const hmx_pic *org,
                                            const hmx_pic *rec, const hmx_levels *lev) {
  return frame_intra(c, plans, 1, n_pics, org, rec, lev, true);
}
extern "C" int hmx_frame_intra_decode_multi(hmx_ctx *c, const hmx_intra_plan *const *plans, int n_pics, const hmx_pic *rec,
                                            const hmx_levels *lev) {
  return frame_intra(c, plans, 1, n_pics, nullptr, rec, lev, false);
}
extern "C" int hmx_set_rdoq(hmx_ctx *c, const hmx_rdoq_pic *pics, int n_pics) {
  if (!c || (pics && n_pics <= 0)) return HMX_ERR_ARG;
  auto &q = c->crq;
  // every input is checked BEFORE the context's state moves: a rejected call leaves the previous setting as it was
  if (pics)
    for (int i = 0; i < n_pics; i++)
      if (!(pics[i].lambda_luma > 0) || !(pics[i].lambda_chroma > 0)) return fail(c, HMX_ERR_ARG, "hmx_set_rdoq: lambda must be positive");
  q.serial++;
  q.lambda_valid = false;
  if (!pics) {
    q.n = 0;
    return HMX_OK;
  }
  static_assert(sizeof(hmx_rdoq_pic) == 8 * sizeof(EstBitsDev) + 2 * sizeof(double), "hmx_rdoq_pic: eight tables and two multipliers");
  q.n = 0; // from here on a failure (device memory, copy) leaves RDOQ OFF, never a half-written table set
  HIPCHK(c, hipStreamSynchronize(c->stream)); // a queued call may still read the previous tables
  int r = grow_dev(c, (void **)&q.d_est, &q.cap_est, sizeof(EstBitsDev) * 8 * (size_t)n_pics, "RDOQ bit-estimate tables of the chain");
  if (!r) r = grow_dev(c, (void **)&q.d_lambda, &q.cap_lambda, sizeof(double) * 4 * (size_t)n_pics, "RDOQ multipliers of the chain");
  if (r) return r;
  q.lambda.resize((size_t)n_pics * 2);
  for (int i = 0; i < n_pics; i++) {
    q.lambda[(size_t)i * 2] = pics[i].lambda_luma, q.lambda[(size_t)i * 2 + 1] = pics[i].lambda_chroma;
    HIPCHK(c, hipMemcpyAsync(q.d_est + (size_t)i * 8, pics[i].est, sizeof(EstBitsDev) * 8, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  q.n = n_pics;
  return HMX_OK;
}
extern "C" int hmx_set_sse_output(hmx_ctx *c, const hmx_sse *sse, int n_pics) {
  if (!c || (sse && n_pics <= 0)) return HMX_ERR_ARG;
  c->sse_out.clear();
  if (sse) c->sse_out.assign(sse, sse + n_pics);
  return HMX_OK;
}
extern "C" int hmx_frame_intra_encode_resident(hmx_ctx *c, const hmx_intra_plan *const *plans, int plan_stride, int n_pics,
                                               const hmx_tpool *org, hmx_tpool *rec, const hmx_levels *lev) {
  if (!org || !rec || (plan_stride != 0 && plan_stride != 1)) return fail(c, HMX_ERR_ARG, "hmx_frame_intra_encode_resident: bad argument");
  return frame_intra(c, plans, plan_stride, n_pics, nullptr, nullptr, lev, true, false, org, rec);
}
extern "C" int hmx_frame_intra_decode_resident(hmx_ctx *c, const hmx_intra_plan *const *plans, int plan_stride, int n_pics,
                                               hmx_tpool *rec, const hmx_levels *lev) {
  if (!rec || (plan_stride != 0 && plan_stride != 1)) return fail(c, HMX_ERR_ARG, "hmx_frame_intra_decode_resident: bad argument");
  return frame_intra(c, plans, plan_stride, n_pics, nullptr, nullptr, lev, false, false, nullptr, rec);
}

