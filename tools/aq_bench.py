"""Throughput of the adaptive-QP entries (include/hmx.h) over N distinct 3840x2160 10-bit originals at AQ depths 1 and 4 (CTU 64),
timed with events on the context's stream: hmx_aq_activity_multi (activity kernel + ordered layer sums), hmx_aq_average_multi (the
ordered sums alone; the activity kernel's time is the difference, the two run back to back on one stream) and hmx_aq_qp_map_multi.
Prints one JSON line per measurement.  For the activity kernel: the algorithmic traffic -- every luma sample once, 2 bytes -- in
GB/s, beside what a device-to-device copy of the same bytes reaches in the same run (bytes read plus bytes written over its time,
the way the 6.3 TB/s of tools/wp_estimate_bench.py is counted).  The copy is the yardstick, as for the weight estimation.  For
context tests/aq_oracle.py is timed on one host core on one picture.  Numbers go to DESIGN.md, the README and
profiles/aq_activity_bench.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from thevc_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=64)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=int, default=80, help="luma margin of every picture (the reference's layout)")
    ap.add_argument("--host", type=int, default=1, help="0: skip the host timing of tests/aq_oracle.py")
    a = ap.parse_args()
    ctx = capi.Context(bit_depth=a.bits)
    L = capi.lib()
    rng = np.random.default_rng(2026)
    mx = (1 << a.bits) - 1
    # seeded content, every picture distinct: one noisy field, shifted and faded per picture
    yy, xx = np.mgrid[0:a.h, 0:a.w]
    base = ((mx / 2) * (1 + 0.8 * np.sin(xx / 23.0) * np.cos(yy / 31.0)) + rng.integers(-6, 7, (a.h, a.w)) * (1 + (xx // 64 + yy // 64) % 5)).astype(np.int32)
    chroma = np.zeros((a.h // 2, a.w // 2), np.int16)
    lumas, pics = [], []
    for i in range(a.pics):
        y = np.clip(np.roll(base, (3 * i, 5 * i), (0, 1)) * (1.0 - 0.004 * i) + i, 0, mx).astype(np.int16)
        if i == 0:
            lumas.append(y)
        pics.append(capi.DevPicture(ctx, a.w, a.h, a.margin, a.margin).upload([y, chroma, chroma]))
    po = (capi.Pic * a.pics)(*[p.as_pic() for p in pics])
    luma_bytes = a.pics * a.w * a.h * 2

    def measure(call):
        for _ in range(a.warmup):
            call()
        ctx.sync()
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        for _ in range(a.calls):
            call()
        ctx.record(e1)
        ms = ctx.elapsed_ms(e0, e1) / a.calls
        ctx.sync()
        return ms

    def report(**kw):
        print(json.dumps(dict(pics=a.pics, w=a.w, h=a.h, bits=a.bits, calls=a.calls, **kw)), flush=True)

    # the yardstick: a device-to-device copy of the same bytes, in this run
    import torch
    src, dst = torch.zeros(luma_bytes, dtype=torch.uint8, device="cuda"), torch.empty(luma_bytes, dtype=torch.uint8, device="cuda")
    for _ in range(a.warmup):
        dst.copy_(src)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.calls):
        dst.copy_(src)
    t1.record()
    torch.cuda.synchronize()
    copy_ms = t0.elapsed_time(t1) / a.calls
    copy_gbs = 2 * luma_bytes / (copy_ms * 1e-3) / 1e9
    report(kernel="device copy of the luma bytes", ms_per_call=round(copy_ms, 4), read_plus_write_gb_s=round(copy_gbs, 1))
    del src, dst
    for depths in (1, 4):
        g = capi.aq_layout(a.w, a.h, 64, depths)
        d_act, d_avg, d_qp = ctx.alloc(8 * a.pics * g.total), ctx.alloc(8 * a.pics * depths), ctx.alloc(a.pics * g.total)
        sq = (np.arange(a.pics) % 20 + 22).astype(np.int32)
        both = measure(lambda: ctx._chk(L.hmx_aq_activity_multi(ctx.h, a.pics, po, a.w, a.h, 64, depths, d_act.ptr, d_avg.ptr)))
        sums = measure(lambda: ctx._chk(L.hmx_aq_average_multi(ctx.h, a.pics, a.w, a.h, 64, depths, d_act.ptr, d_avg.ptr)))
        qpm = measure(lambda: ctx._chk(L.hmx_aq_qp_map_multi(ctx.h, a.pics, a.w, a.h, 64, depths, d_act.ptr, d_avg.ptr, sq.ctypes.data, 6, 6 * (a.bits - 8), d_qp.ptr)))
        act_ms = both - sums
        gbs = luma_bytes / (act_ms * 1e-3) / 1e9
        report(kernel="hmx_aq_activity_multi", depths=depths, units_per_pic=g.total, ms_per_call=round(both, 4))
        report(kernel="  ordered layer sums (hmx_aq_average_multi)", depths=depths, ms_per_call=round(sums, 4), dependent_adds_finest_layer=g.nx[depths - 1] * g.ny[depths - 1])
        report(kernel="  activity kernel (difference)", depths=depths, ms_per_call=round(act_ms, 4), gpx_s=round(a.pics * a.w * a.h / (act_ms * 1e-3) / 1e9, 2),
               alg_gb_s=round(gbs, 1), frac_of_copy=round(gbs / copy_gbs, 3))
        report(kernel="hmx_aq_qp_map_multi range 6", depths=depths, ms_per_call=round(qpm, 4))
        if a.host:
            import aq_oracle as ao
            t0 = time.perf_counter()
            ao.preanalyze(lumas[0], 64, depths)
            report(kernel="tests/aq_oracle.py preanalyze, one picture on one host core", depths=depths, ms_per_picture=round((time.perf_counter() - t0) * 1e3, 1))
        for b in (d_act, d_avg, d_qp):
            b.free()
    ctx.close()


if __name__ == "__main__":
    main()
