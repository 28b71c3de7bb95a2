"""Throughput of hmx_sao_stats_multi (the encoder's SAO statistics, include/hmx.h): N distinct 3840x2160 10-bit
picture pairs (org, deblocked rec) in one call, timed with events on the context's stream.  Prints one JSON line: ms per
call, Gpx/s (luma positions), and the algorithmic traffic -- both pictures read once, 6 bytes per luma position at 4:2:0,
plus the bins written -- in GB/s and as a fraction of 6.3 TB/s achievable HBM bandwidth; then the same for lcu_based = 0 and
for hmx_sao_stats_multi_avail with the mask of 4 x 4 tiles.  Numbers go to DESIGN.md 7."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thevc_amd import capi  # noqa: E402

HBM = 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=64)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    ctx = capi.Context(bit_depth=a.bits)
    L = capi.lib()
    rng = np.random.default_rng(2026)
    mx = (1 << a.bits) - 1
    orgs, recs = [], []
    for i in range(a.pics):  # seeded content, every picture distinct: a smooth field plus noise, rec = org + small error
        planes_o, planes_r = [], []
        for pw, ph in ((a.w, a.h), (a.w // 2, a.h // 2), (a.w // 2, a.h // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            base = (mx / 2) * (1 + np.sin((xx + 37 * i) / (23 + i % 7)) * np.cos((yy - 11 * i) / (31 + i % 5)))
            o = np.clip(base + rng.integers(-6, 7, (ph, pw)), 0, mx).astype(np.int16)
            r = np.clip(o.astype(np.int32) + rng.integers(-3, 4, (ph, pw)), 0, mx).astype(np.int16)
            planes_o.append(o), planes_r.append(r)
        orgs.append(capi.DevPicture(ctx, a.w, a.h).upload(planes_o))
        recs.append(capi.DevPicture(ctx, a.w, a.h).upload(planes_r))
    n_lcu = -(-a.w // 64) * -(-a.h // 64)
    out = ctx.alloc(a.pics * 3 * n_lcu * capi.SAO_STAT_BINS * 8)
    po = (capi.Pic * a.pics)(*[p.as_pic() for p in orgs])
    pr = (capi.Pic * a.pics)(*[p.as_pic() for p in recs])

    def measure(kernel, call):
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
        px = a.w * a.h * a.pics
        nbytes = px * 6 + a.pics * 3 * n_lcu * capi.SAO_STAT_BINS * 8
        gbs = nbytes / (ms * 1e-3) / 1e9
        print(json.dumps(dict(kernel=kernel, pics=a.pics, w=a.w, h=a.h, bits=a.bits, calls=a.calls, ms_per_call=round(ms, 4),
                              gpx_s=round(px / (ms * 1e-3) / 1e9, 2), alg_gb_s=round(gbs, 1), frac_of_6p3_tb_s=round(gbs * 1e9 / HBM, 3))))

    measure("hmx_sao_stats_multi", lambda: ctx._chk(L.hmx_sao_stats_multi(ctx.h, a.pics, po, pr, a.w, a.h, 1, out.ptr)))
    if hasattr(L, "hmx_sao_stats_multi_avail"):  # (absent from an older build loaded through HMX_LIB_PATH)
        # the availability path with the mask of 4 x 4 tiles that the filters may not cross, next to the entry it is compared
        # with: nothing skipped (lcu_based = 0)
        from thevc_amd import decisions
        cw, ch = -(-a.w // 64), -(-a.h // 64)
        _, tile_id = decisions.slice_tile_maps(a.w, a.h, 64, (0,), decisions.uniform_bounds(cw, 4), decisions.uniform_bounds(ch, 4))
        avail = decisions.lf_border_avail(a.w, a.h, 64, tile_id=tile_id, lf_cross_tiles=False)
        d_av = ctx.to_device(np.ascontiguousarray(np.broadcast_to(avail, (a.pics, n_lcu))))
        measure("hmx_sao_stats_multi lcu_based=0", lambda: ctx._chk(L.hmx_sao_stats_multi(ctx.h, a.pics, po, pr, a.w, a.h, 0, out.ptr)))
        measure("hmx_sao_stats_multi_avail", lambda: ctx._chk(L.hmx_sao_stats_multi_avail(ctx.h, a.pics, po, pr, a.w, a.h, d_av.ptr, out.ptr)))
    ctx.close()


if __name__ == "__main__":
    main()
