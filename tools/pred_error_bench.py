"""hmx_batch_inter_pred_error against the cheapest route a caller had before it, on one 1920 x 1080 10-bit picture tiled into
16 x 16 units with five candidates each (a mix of uni- and bi-predicted, two references, Hadamard):
  (a) the fused call: one launch, every candidate predicted in LDS, costed, the winner of each unit decided on the device;
  (b) five hmx_batch_motionCompensation_multi calls over the same units, one per candidate rank, into a scratch picture.  That
      route only PREDICTS (luma and chroma, written to HBM); any costing would come on top.
Median of --repeats timings after one warm-up, the two paths alternated, time between two events on the context's stream
around the call.  The events also see what the host does before it launches (the argument checks and the copy of the candidate
list into the argument arena), so each path is timed a second way: two calls between the events, minus one call -- the second
call's host work overlaps the first call's kernel, which leaves the larger of the two parts.
Prints microseconds per call, candidates per second, and the algorithmic bytes of (a) -- the original once per unit plus the
(w + 7) x (h + 7) window per candidate and list -- against 6.3 TB/s."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thevc_amd import capi, workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--size", type=int, default=16, help="unit size (square)")
ap.add_argument("--sad", action="store_true", help="SAD instead of the Hadamard sum")
args = ap.parse_args()
B, w, h, M, LAM, NC, S = 10, 1920, 1080, 80, 2000000, 5, args.size
ctx = capi.Context(bit_depth=B)
L = capi.lib()
refs = [capi.DevPicture(ctx, w, h, M, M).upload(workload.make_planes(3 + i, w, h, B, "texture")) for i in range(2)]
for r in refs:
    ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(r.as_pic()), w, h, M, M))
org = capi.DevPicture(ctx, w, h).upload(workload.make_planes(9, w, h, B, "texture"))
dst = capi.DevPicture(ctx, w, h).zero()
rng = np.random.default_rng(11)
units = [(x, y) for y in range(0, h - S + 1, S) for x in range(0, w - S + 1, S)]
n_units, n = len(units), len(units) * NC
cands = np.zeros(n, capi.PU_DTYPE)
for i, (x, y) in enumerate(units):
    for k in range(NC):
        kind = (i + k) % 3  # list 0, list 1, both
        mv = [capi.clip_mv(int(rng.integers(-64, 65)), int(rng.integers(-64, 65)), x & ~63, y & ~63, w, h) for _ in range(2)]
        cands[i * NC + k] = (x, y, S, S, 255 if kind == 1 else int(rng.integers(0, 2)), 255 if kind == 0 else int(rng.integers(0, 2)), mv[0][0], mv[0][1],
                             mv[1][0], mv[1][1])
bits = np.tile(np.array([capi.merge_idx_bits(k) for k in range(NC)], np.uint32), n_units)
first = np.arange(0, n + 1, NC).astype(np.uint32)
n_lists = int((cands["ref0"] != 255).sum() + (cands["ref1"] != 255).sum())
alg_bytes = 2 * (n_units * S * S + n_lists * (S + 7) * (S + 7)) + 8 * n + 12 * n_units
ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in refs])
o, d = org.as_pic(), dst.as_pic()
d_dist, d_cost, d_best = ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(12 * n_units)
d_rank = [ctx.to_device(np.ascontiguousarray(cands[k::NC])) for k in range(NC)]
jobs = [(capi.McJob * 1)() for _ in range(NC)]
for k in range(NC):
    jobs[k][0].d_pus, jobs[k][0].n_pus, jobs[k][0].refs, jobs[k][0].n_refs = d_rank[k].ptr, n_units, ref_arr, 2
    jobs[k][0].dst, jobs[k][0].pic_w, jobs[k][0].pic_h = C.pointer(d), w, h
e0, e1 = ctx.event(), ctx.event()
use_had = 0 if args.sad else 1


def path_a():
    ctx._chk(L.hmx_batch_inter_pred_error(ctx.h, cands.ctypes.data, bits.ctypes.data, n, first.ctypes.data, n_units, ref_arr, 2, C.byref(o), w, h, M, M, LAM,
                                          use_had, d_dist.ptr, d_cost.ptr, d_best.ptr))


def path_b():
    for k in range(NC):
        ctx._chk(L.hmx_batch_motionCompensation_multi(ctx.h, 1, jobs[k]))


def timed(fn):
    ctx.record(e0)
    fn()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1)


def stats(ts):
    return f"{np.median(ts) * 1e3:9.1f} us (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f})"


def twice(fn):
    return lambda: (fn(), fn())


timed(path_a), timed(path_b)  # warm-up
ta, tb, ta2, tb2 = [], [], [], []
for _ in range(args.repeats):
    ta.append(timed(path_a))
    tb.append(timed(path_b))
    ta2.append(timed(twice(path_a)) - ta[-1])
    tb2.append(timed(twice(path_b)) - tb[-1])
best = d_best.download(capi.PRED_CHOICE_DTYPE, n_units)
ma, mb = float(np.median(ta)), float(np.median(tb))
print(f"1920x1080 {B} bit, {n_units} units of {S}x{S}, {NC} candidates each ({n_lists} list predictions), {'SAD' if args.sad else 'Hadamard'}, "
      f"{args.repeats} repeats, alternated", flush=True)
print(f"(a) hmx_batch_inter_pred_error, one call     GPU {stats(ta)}  {n / ma / 1e3:8.2f} M candidates/s  "
      f"algorithmic {alg_bytes / 1e6:.1f} MB = {alg_bytes / (ma * 1e-3) / 1e12:.3f} TB/s of 6.3", flush=True)
print(f"(b) 5 x hmx_batch_motionCompensation_multi   GPU {stats(tb)}  {n / mb / 1e3:8.2f} M candidates/s  (prediction only, luma + chroma to HBM)", flush=True)
print(f"second of two back-to-back calls: (a) {stats(ta2)}   (b) {stats(tb2)}", flush=True)
print(f"GPU time (b) / (a) = {mb / ma:.2f}; ranges {'do not overlap' if max(ta) < min(tb) or max(tb) < min(ta) else 'OVERLAP'}; "
      f"winners: index histogram {np.bincount(best['index'], minlength=NC).tolist()}", flush=True)
ctx.close()
