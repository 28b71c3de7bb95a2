"""Throughput of hmx_batch_fullpel_search on one 3840 x 2160 10-bit picture tiled into 16 x 16 units and into 64 x 64 units,
+-64 boxes (xSetSearchRange around random predictors), sub_shift 0 and 1, and on the mixed unit list of workload.make_me_units.  Every line is the median of --repeats timings
(device time between two events on the context's stream, after one warm-up call) with their min..max, the absolute differences
per second, and that figure as a fraction of the VALU issue bound of v_sad_u16: two differences per lane and instruction, one
wave64 instruction per --sad-cycles cycles per SIMD, 4 SIMDs x 256 CUs at --ghz.  Both figures are arguments without a default:
they come from a run of tools/bin/issue_probe on the same device (ISSUE_FROM=60 prints the clock and the v_sad_u16 lines).
--wp: every case is also timed through hmx_batch_fullpel_search_wp with a non-default table (weight 45, offset -20, denominator
2^5), the two calls alternated on the same units; the weighted line follows the unweighted one.  The weighted call reads every
row whatever sub_shift says, and its line counts the differences it forms."""
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
ap.add_argument("--sad-cycles", type=float, required=True, help="measured SIMD cycles per v_sad_u16 wave instruction (tools/issue_probe)")
ap.add_argument("--ghz", type=float, required=True, help="the device clock tools/issue_probe prints")
ap.add_argument("--once", action="store_true", help="one call per case and no timing lines (for profiler runs)")
ap.add_argument("--wp", action="store_true", help="also time the weighted entry on the same units, alternated with the unweighted call")
args = ap.parse_args()
B, w, h, M, RANGE = 10, 3840, 2160, 80, 64
ctx = capi.Context(bit_depth=B)
L = capi.lib()
rng = np.random.default_rng(1)
refs = [capi.DevPicture(ctx, w, h, M, M).upload(workload.make_planes(3, w, h, B, "texture"))]
ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(refs[0].as_pic()), w, h, M, M))
org = capi.DevPicture(ctx, w, h).upload(workload.make_planes(4, w, h, B, "texture"))
bound = 2 * 64 / args.sad_cycles * 4 * 256 * args.ghz * 1e9  # absolute differences per second
WP = capi.me_wp_table([45], [-20], [5])


def units_of(size, sub_shift):
    xs, ys = np.meshgrid(np.arange(0, w - size + 1, size), np.arange(0, h - size + 1, size))
    u = np.zeros(xs.size, capi.ME_UNIT_DTYPE)
    u["x"], u["y"], u["w"], u["h"], u["sub_shift"] = xs.reshape(-1), ys.reshape(-1), size, size, sub_shift
    u["pred_x"], u["pred_y"] = rng.integers(-4 * 16, 4 * 16 + 1, (2, u.size))
    for r in u:
        r["left"], r["top"], r["right"], r["bottom"] = capi.set_search_range(int(r["pred_x"]), int(r["pred_y"]), RANGE, int(r["x"]), int(r["y"]), w, h, 64)
    return u


for size in (16, 64, 0):  # 0: mixed sizes, sub_shift drawn per unit
    for sub_shift in (0, 1) if size else ("mixed",):
        u = units_of(size, sub_shift) if size else workload.make_me_units(5, w, h, 1, RANGE)
        per_unit = (u["right"].astype(np.int64) - u["left"] + 1) * (u["bottom"].astype(np.int64) - u["top"] + 1)
        cands = int(per_unit.sum())
        diffs = int((per_unit * u["w"] * (u["h"].astype(np.int64) >> u["sub_shift"])).sum())
        name = f"{size:2d}x{size:<2d} units sub_shift {sub_shift}" if size else "make_me_units (mixed sizes) "
        ref_arr = (capi.Pic * 1)(refs[0].as_pic())
        d_res = ctx.alloc(len(u) * capi.ME_RESULT_DTYPE.itemsize)
        o = org.as_pic()
        call = lambda: ctx._chk(L.hmx_batch_fullpel_search(ctx.h, u.ctypes.data, len(u), ref_arr, 1, C.byref(o), w, h, M, M, 2000000, d_res.ptr, None))
        call_wp = lambda: ctx._chk(L.hmx_batch_fullpel_search_wp(ctx.h, u.ctypes.data, len(u), ref_arr, 1, C.byref(o), w, h, M, M, 2000000, d_res.ptr,
                                                                 None, WP.ctypes.data))
        calls = [(call, name, diffs)] + ([(call_wp, name.rstrip() + " WEIGHTED", int((per_unit * u["w"] * u["h"].astype(np.int64)).sum()))] if args.wp else [])
        for fn, _, _ in calls:
            fn()
        ctx.sync()
        if not args.once:
            e0, e1 = ctx.event(), ctx.event()
            ts = [[] for _ in calls]
            for _ in range(args.repeats):
                for k, (fn, _, _) in enumerate(calls):  # alternated
                    ctx.record(e0)
                    fn()
                    ctx.record(e1)
                    ctx.sync()
                    ts[k].append(ctx.elapsed_ms(e0, e1))
            for (_, label, nd), tk in zip(calls, ts):
                t = float(np.median(tk))
                rate = nd / (t * 1e-3)
                print(f"{label}: {len(u):6d} units, {cands / 1e6:7.1f} M candidates  {t:8.2f} ms/picture (min {min(tk):.2f}, max {max(tk):.2f}; "
                      f"{len(tk)} repeats)  {rate / 1e12:6.2f} T absolute differences/s = {100 * rate / bound:5.1f} % of the v_sad_u16 issue bound "
                      f"({bound / 1e12:.1f} T/s at {args.sad_cycles} cycles and {args.ghz} GHz)", flush=True)
        d_res.free()
