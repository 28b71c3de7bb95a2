"""hmx_batch_subpel_search against what a caller had to do before it, on one 1920 x 1080 10-bit picture with two references:
units from workload.make_me_units, integer winners from hmx_batch_fullpel_search (left on the device).  Two paths on the same
units and winners, alternated, --repeats timings each after one warm-up:
  (a) the new call: both stages and both decisions in one launch, 18 candidates per unit;
  (b) one hmx_batch_subpel_cost call over the 49-offset neighbourhood (the quarter stage depends on each unit's own
      half-sample winner, so one call for all units has to cost the whole 7 x 7), the download of its costs and the pick on
      the host (numpy, the vector bits through capi.mv_cost).
Per path: the device time between two events on the context's stream (the kernels alone) and the wall time of the whole path,
as median with min..max.  Then (a) per size class (units up to 8 x 8, 16 to 32, 48 to 64), so that a weak small-unit shape
shows.  The two paths' results are compared before anything is timed.
--wp: hmx_batch_subpel_search_wp with a non-default table (weights 45 and 90, offsets -20 and 33, denominators 2^5 and 2^6) is
timed on the same units and winners, alternated with (a), and gets a line of its own."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thevc_amd import capi, workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--range", type=int, default=16, help="search range of the integer stage that supplies the winners")
ap.add_argument("--sad", action="store_true", help="SAD instead of the Hadamard sum")
ap.add_argument("--wp", action="store_true", help="also time the weighted entry on the same units, alternated with (a)")
args = ap.parse_args()
B, w, h, M, LAM = 10, 1920, 1080, 80, 2000000
use_had = 0 if args.sad else 1
ctx = capi.Context(bit_depth=B)
L = capi.lib()
refs = [capi.DevPicture(ctx, w, h, M, M).upload(workload.make_planes(3 + i, w, h, B, "texture")) for i in range(2)]
for r in refs:
    ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(r.as_pic()), w, h, M, M))
org = capi.DevPicture(ctx, w, h).upload(workload.make_planes(9, w, h, B, "texture"))
units = workload.make_me_units(5, w, h, 2, args.range)
ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in refs])
o = org.as_pic()
REFINE_H = ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))
REFINE_Q = ((0, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1))
OFFS = [(dx, dy) for dy in range(-3, 4) for dx in range(-3, 4)]
WP = capi.me_wp_table([45, 90], [-20, 33], [5, 6])
offs = np.array(OFFS, np.int8)
IDX_H = [OFFS.index((2 * dx, 2 * dy)) for dx, dy in REFINE_H]


def timed(fn, e0, e1):
    t0 = time.perf_counter()
    ctx.record(e0)
    out = fn()
    return out, ctx.elapsed_ms(e0, e1), (time.perf_counter() - t0) * 1e3


def stats(ts):
    return f"{np.median(ts):8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


def run(u, label):
    n = len(u)
    d_int = ctx.batch_fullpel_search_device(u, refs, org, w, h, M, M, LAM)
    ctx.sync()
    ints = d_int.download(capi.ME_RESULT_DTYPE, n)
    d_res, d_cost = ctx.alloc(n * capi.SUBPEL_RESULT_DTYPE.itemsize), ctx.alloc(n * 49 * 4)
    pus = np.zeros(n, capi.PU_DTYPE)
    for k in ("x", "y", "w", "h"):
        pus[k] = u[k]
    pus["ref0"], pus["ref1"], pus["mv0x"], pus["mv0y"] = u["ref"], 255, 4 * ints["mvx"].astype(np.int32), 4 * ints["mvy"].astype(np.int32)
    e0, e1 = ctx.event(), ctx.event()

    def path_a():
        ctx._chk(L.hmx_batch_subpel_search(ctx.h, u.ctypes.data, n, d_int.ptr, ref_arr, 2, C.byref(o), w, h, M, M, LAM, use_had, d_res.ptr, None))
        ctx.record(e1)
        ctx.sync()
        return d_res.download(capi.SUBPEL_RESULT_DTYPE, n)

    def path_w():
        ctx._chk(L.hmx_batch_subpel_search_wp(ctx.h, u.ctypes.data, n, d_int.ptr, ref_arr, 2, C.byref(o), w, h, M, M, LAM, use_had, d_res.ptr, None,
                                              WP.ctypes.data))
        ctx.record(e1)
        ctx.sync()
        return d_res.download(capi.SUBPEL_RESULT_DTYPE, n)

    def path_b():
        ctx._chk(L.hmx_batch_subpel_cost(ctx.h, pus.ctypes.data, n, ref_arr, 2, C.byref(o), offs.ctypes.data, 49, use_had, d_cost.ptr))
        ctx.record(e1)
        ctx.sync()
        d = d_cost.download(np.uint32, n * 49).reshape(n, 49)
        out = np.zeros(n, capi.SUBPEL_RESULT_DTYPE)
        for i in range(n):
            ix, iy, px, py = int(ints[i]["mvx"]), int(ints[i]["mvy"]), int(u[i]["pred_x"]), int(u[i]["pred_y"])
            ch = [(int(d[i][IDX_H[k]]) + capi.mv_cost(LAM, 2 * ix + dx, 2 * iy + dy, px, py, 1)) & 0xFFFFFFFF for k, (dx, dy) in enumerate(REFINE_H)]
            hx, hy = REFINE_H[int(np.argmin(ch))]
            bx, by = 4 * ix + 2 * hx, 4 * iy + 2 * hy
            cq = [(int(d[i][OFFS.index((2 * hx + qx, 2 * hy + qy))]) + capi.mv_cost(LAM, bx + qx, by + qy, px, py, 0)) & 0xFFFFFFFF for qx, qy in REFINE_Q]
            k = int(np.argmin(cq))
            mvx, mvy = bx + REFINE_Q[k][0], by + REFINE_Q[k][1]
            out[i] = (mvx, mvy, (cq[k] - capi.mv_cost(LAM, mvx, mvy, px, py, 0)) & 0xFFFFFFFF, cq[k])
        return out

    ra, rb = path_a(), (path_b() if label == "all units" else None)  # warm-up, and the two paths agree
    if rb is not None and not np.array_equal(ra, rb):
        raise SystemExit(f"{label}: the two paths disagree on {int((ra != rb).sum())} units")
    ta, tb, tw = [], [], []
    if args.wp:
        path_w()  # warm-up
    for _ in range(args.repeats):
        ta.append(timed(path_a, e0, e1)[1:])
        if args.wp:
            tw.append(timed(path_w, e0, e1)[1:])
        if rb is not None:
            tb.append(timed(path_b, e0, e1)[1:])
    ga = [t[0] for t in ta]
    print(f"{label:14s} {n:6d} units  (a) hmx_batch_subpel_search   GPU {stats(ga)}  whole {stats([t[1] for t in ta])}  "
          f"{n / np.median(ga) / 1e3:7.2f} M units/s", flush=True)
    if args.wp:
        gw = [t[0] for t in tw]
        print(f"{label:14s} {n:6d} units  (w) hmx_batch_subpel_search_wp GPU {stats(gw)}  whole {stats([t[1] for t in tw])}  "
              f"{n / np.median(gw) / 1e3:7.2f} M units/s", flush=True)
    if rb is not None:
        gb = [t[0] for t in tb]
        print(f"{label:14s} {n:6d} units  (b) subpel_cost x 49 + host   GPU {stats(gb)}  whole {stats([t[1] for t in tb])}", flush=True)
        print(f"{label:14s} GPU time (b) / (a) = {np.median(gb) / np.median(ga):.2f}; ranges {'do not overlap' if max(ga) < min(gb) else 'OVERLAP'}; "
              f"{args.repeats} repeats, alternated; {'SAD' if args.sad else 'Hadamard'}; results of (a) and (b) identical", flush=True)
    for d in (d_int, d_res, d_cost):
        d.free()


print(f"1920x1080 {B} bit, 2 references, make_me_units(range {args.range})", flush=True)
run(units, "all units")
side = np.maximum(units["w"], units["h"])
for lo, hi, name in ((4, 8, "up to 8x8"), (12, 32, "12 to 32"), (48, 64, "48 to 64")):
    sel = units[(side >= lo) & (side <= hi)]
    if len(sel):
        run(sel, name)
ctx.close()
