"""Throughput of the weight-estimation reductions (include/hmx.h): hmx_wp_acdc_multi over N distinct 3840x2160 10-bit originals and
hmx_wp_sad_multi over (original, reconstruction) jobs, one reference per picture and four, each in one call, timed with events on
the context's stream; hmx_sao_stats_multi on the same pictures beside them (the project's other whole-picture statistic).  Prints
one JSON line per entry: ms per call, Gpx/s (luma positions read), the algorithmic traffic -- hmx_wp_acdc_multi reads every plane
once per pass (two passes), hmx_wp_sad_multi reads the original and the reconstruction once per job, 3 bytes per luma position
and picture at 4:2:0 -- in GB/s and as a fraction of the 8.0 TB/s HBM peak and of the 6.3 TB/s a copy achieves.  Numbers go to
DESIGN.md and profiles/wp_estimate_bench.txt."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thevc_amd import capi  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, default=64)
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--margin", type=int, default=80, help="luma margin of every picture (the reference's layout)")
    a = ap.parse_args()
    ctx = capi.Context(bit_depth=a.bits)
    L = capi.lib()
    rng = np.random.default_rng(2026)
    mx = (1 << a.bits) - 1
    # seeded content, every picture distinct: one noisy field, shifted and faded per picture; rec = org + small error
    base = []
    for pw, ph in ((a.w, a.h), (a.w // 2, a.h // 2), (a.w // 2, a.h // 2)):
        yy, xx = np.mgrid[0:ph, 0:pw]
        base.append(((mx / 2) * (1 + 0.8 * np.sin(xx / 23.0) * np.cos(yy / 31.0)) + rng.integers(-6, 7, (ph, pw))).astype(np.int32))
    err = [rng.integers(-3, 4, b.shape).astype(np.int32) for b in base]
    orgs, recs = [], []
    for i in range(a.pics):
        o = [np.clip(np.roll(b, (3 * i, 5 * i), (0, 1)) * (1.0 - 0.004 * i) + i, 0, mx).astype(np.int16) for b in base]
        r = [np.clip(p.astype(np.int32) + np.roll(e, i, 1), 0, mx).astype(np.int16) for p, e in zip(o, err)]
        orgs.append(capi.DevPicture(ctx, a.w, a.h, a.margin, a.margin).upload(o))
        recs.append(capi.DevPicture(ctx, a.w, a.h, a.margin, a.margin).upload(r))
    po = (capi.Pic * a.pics)(*[p.as_pic() for p in orgs])
    pr = (capi.Pic * a.pics)(*[p.as_pic() for p in recs])
    pic_bytes = a.w * a.h * 3  # one 4:2:0 picture of 16-bit samples

    def measure(kernel, call, pictures_read, out_bytes):
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
        nbytes = pictures_read * pic_bytes + out_bytes
        gbs = nbytes / (ms * 1e-3) / 1e9
        print(json.dumps(dict(kernel=kernel, pics=a.pics, w=a.w, h=a.h, bits=a.bits, calls=a.calls, ms_per_call=round(ms, 4),
                              gpx_s=round(pictures_read * a.w * a.h / (ms * 1e-3) / 1e9, 2), alg_gb_s=round(gbs, 1),
                              frac_of_8p0_tb_s=round(gbs * 1e9 / HBM_PEAK, 3), frac_of_6p3_tb_s=round(gbs * 1e9 / HBM_COPY, 3))), flush=True)

    d_acdc = ctx.alloc(48 * a.pics)
    measure("hmx_wp_acdc_multi", lambda: ctx._chk(L.hmx_wp_acdc_multi(ctx.h, a.pics, po, a.w, a.h, d_acdc.ptr)), 2 * a.pics, 48 * a.pics)
    for per_pic in (1, 4):
        jobs = np.zeros(a.pics * per_pic, capi.WP_SAD_JOB_DTYPE)
        for i in range(a.pics):
            for k in range(per_pic):
                jobs[i * per_pic + k] = (i, (i + k) % a.pics, ((60 + k, 66, 62), (3 - k, -2, 1), (6, 6, 6), 0))
        d_out = ctx.alloc(48 * len(jobs))
        measure(f"hmx_wp_sad_multi {per_pic} ref/pic", lambda: ctx._chk(L.hmx_wp_sad_multi(ctx.h, len(jobs), jobs.ctypes.data, po, a.pics, pr, a.pics, a.w, a.h, d_out.ptr)),
                2 * len(jobs), 48 * len(jobs))
        d_out.free()
    n_lcu = -(-a.w // 64) * -(-a.h // 64)
    d_sao = ctx.alloc(a.pics * 3 * n_lcu * capi.SAO_STAT_BINS * 8)
    measure("hmx_sao_stats_multi", lambda: ctx._chk(L.hmx_sao_stats_multi(ctx.h, a.pics, po, pr, a.w, a.h, 1, d_sao.ptr)), 2 * a.pics,
            a.pics * 3 * n_lcu * capi.SAO_STAT_BINS * 8)
    ctx.close()


if __name__ == "__main__":
    main()
