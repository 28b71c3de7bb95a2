"""hmx_batch_tz_search against hmx_batch_fullpel_search (unchanged code: the yardstick) on one 3840 x 2160 10-bit picture with two
references: the units of workload.make_me_units at +-64, start points from hmx_clipMv (capi.tz_units).  The two calls are
alternated on the same units, --repeats timings each after one warm-up; per call the device time between two events on the
context's stream, as median with min..max.  Then the evaluations per unit from d_trace_count (mean, max) and the share of
units that ran the raster stage -- read off the trace: the raster stage is the one place where (left, top) is followed by the
point five to its right (or, in a box narrower than six, five below).  The TZ vectors are checked against the full search's
before anything is timed: a TZ cost is never below the box minimum unless its vector lies outside the box.
--wp: hmx_batch_tz_search_wp with a non-default table (weights 45 and 90, offsets -20 and 33, denominators 2^5 and 2^6) is timed
on the same units, alternated with the two calls above, and gets a line of its own."""
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
ap.add_argument("--range", type=int, default=64)
ap.add_argument("--wp", action="store_true", help="also time the weighted entry on the same units, alternated with the unweighted calls")
args = ap.parse_args()
B, w, h, M, LAM, CAP = 10, 3840, 2160, 80, 2000000, 128
ctx = capi.Context(bit_depth=B)
L = capi.lib()
refs = [capi.DevPicture(ctx, w, h, M, M).upload(workload.make_planes(3 + i, w, h, B, "texture")) for i in range(2)]
for r in refs:
    ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(r.as_pic()), w, h, M, M))
org = capi.DevPicture(ctx, w, h).upload(workload.make_planes(9, w, h, B, "texture"))
units = workload.make_me_units(5, w, h, 2, args.range)
tz = capi.tz_units(units, args.range, w, h)
n = len(units)
ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in refs])
o = org.as_pic()
d_tz, d_full = ctx.alloc(n * capi.ME_RESULT_DTYPE.itemsize), ctx.alloc(n * capi.ME_RESULT_DTYPE.itemsize)
e0, e1 = ctx.event(), ctx.event()


def tz_call():
    ctx._chk(L.hmx_batch_tz_search(ctx.h, units.ctypes.data, tz.ctypes.data, n, ref_arr, 2, C.byref(o), w, h, M, M, LAM, d_tz.ptr, None, None, 0))


WP = capi.me_wp_table([45, 90], [-20, 33], [5, 6])


def tz_wp_call():
    ctx._chk(L.hmx_batch_tz_search_wp(ctx.h, units.ctypes.data, tz.ctypes.data, n, ref_arr, 2, C.byref(o), w, h, M, M, LAM, d_tz.ptr, None, None, 0,
                                      WP.ctypes.data))


def full_call():
    ctx._chk(L.hmx_batch_fullpel_search(ctx.h, units.ctypes.data, n, ref_arr, 2, C.byref(o), w, h, M, M, LAM, d_full.ptr, None))


def timed(fn):
    ctx.record(e0)
    fn()
    ctx.record(e1)
    ctx.sync()
    return ctx.elapsed_ms(e0, e1)


def stats(ts):
    return f"{np.median(ts):8.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"


timed(tz_call), timed(full_call)  # warm-up
rt, rf = d_tz.download(capi.ME_RESULT_DTYPE, n), d_full.download(capi.ME_RESULT_DTYPE, n)
inside = (rt["mvx"] >= units["left"]) & (rt["mvx"] <= units["right"]) & (rt["mvy"] >= units["top"]) & (rt["mvy"] <= units["bottom"])
if np.any(rt["cost"][inside] < rf["cost"][inside]):
    raise SystemExit("a TZ cost lies below the full search's minimum of the same box")
tt, tf, tw = [], [], []
if args.wp:
    timed(tz_wp_call)  # warm-up
for _ in range(args.repeats):
    tt.append(timed(tz_call))
    tf.append(timed(full_call))
    if args.wp:
        tw.append(timed(tz_wp_call))
res, counts, trace = ctx.batch_tz_search(units, tz, refs, org, w, h, M, M, LAM, want_trace=True, trace_cap=CAP)
if res.tobytes() != rt.tobytes():
    raise SystemExit("the call with a trace gives other results than the call without")
raster = 0
for i in range(n):
    l, t = int(units[i]["left"]), int(units[i]["top"])
    nxt = (l + 5, t) if int(units[i]["right"]) - l >= 5 else (l, t + 5)
    k = min(int(counts[i]), CAP)
    tx, ty = trace[i]["x"][:k], trace[i]["y"][:k]
    raster += bool(np.any((tx[:-1] == l) & (ty[:-1] == t) & (tx[1:] == nxt[0]) & (ty[1:] == nxt[1])))
cand = int(((units["right"].astype(np.int64) - units["left"] + 1) * (units["bottom"].astype(np.int64) - units["top"] + 1)).sum())
print(f"{w}x{h} {B} bit, 2 references, make_me_units(range {args.range}): {n} units, {cand / 1e6:.1f} M candidates in the boxes", flush=True)
print(f"hmx_batch_tz_search       GPU {stats(tt)}  {n / np.median(tt) / 1e3:7.2f} M units/s", flush=True)
if args.wp:
    print(f"hmx_batch_tz_search_wp    GPU {stats(tw)}  {n / np.median(tw) / 1e3:7.2f} M units/s  (its own walks: the weighted costs lead elsewhere)", flush=True)
print(f"hmx_batch_fullpel_search  GPU {stats(tf)}", flush=True)
print(f"GPU time full / TZ = {np.median(tf) / np.median(tt):.2f}; ranges {'do not overlap' if max(tt) < min(tf) else 'OVERLAP'}; "
      f"{args.repeats} repeats, alternated", flush=True)
print(f"evaluations per unit: mean {counts.mean():.1f}, max {int(counts.max())}; raster stage in {raster} of {n} units ({100.0 * raster / n:.1f} %); "
      f"TZ vector = full-search vector in {int(((rt['mvx'] == rf['mvx']) & (rt['mvy'] == rf['mvy'])).sum())} units, "
      f"TZ cost = box minimum in {int((rt['cost'] == rf['cost']).sum())}", flush=True)
ctx.close()
