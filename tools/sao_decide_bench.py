"""What the SAO parameter search costs on the device (hmx_sao_decide_multi, include/hmx.h) next to what it replaces: N distinct
3840x2160 10-bit picture pairs (org, deblocked rec) at CTU 64, timed with events on the context's stream, warm, median of
repeated calls.  Per batch size one JSON line each for: the statistics kernel, the candidate kernel, the decision kernel (with
its time per CTU step: the kernel's time over the CTUs of ONE picture, since every picture is a chain of its own walked by its
own wave -- the latency of one step of the serial chain), hmx_sao_encode_multi as a whole (statistics, decision, application)
and a device-to-host copy of the statistics array, the download the decision makes unnecessary.  Numbers go to README and
DESIGN.md 4."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thevc_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pics", type=int, nargs="+", default=[64, 8, 512])
    ap.add_argument("--distinct", type=int, default=16, help="distinct picture pairs on the device; a batch cycles through them")
    ap.add_argument("--w", type=int, default=3840)
    ap.add_argument("--h", type=int, default=2160)
    ap.add_argument("--bits", type=int, default=10)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    ctx = capi.Context(bit_depth=a.bits)
    L = capi.lib()
    rng = np.random.default_rng(2026)
    mx = (1 << a.bits) - 1
    orgs, recs, outs = [], [], []
    for i in range(min(a.distinct, max(a.pics))):  # seeded content, as tools/sao_stats_bench.py makes it
        planes_o, planes_r = [], []
        for pw, ph in ((a.w, a.h), (a.w // 2, a.h // 2), (a.w // 2, a.h // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            base = (mx / 2) * (1 + np.sin((xx + 37 * i) / (23 + i % 7)) * np.cos((yy - 11 * i) / (31 + i % 5)))
            o = np.clip(base + rng.integers(-6, 7, (ph, pw)), 0, mx).astype(np.int16)
            r = np.clip(o.astype(np.int32) + rng.integers(-3, 4, (ph, pw)), 0, mx).astype(np.int16)
            planes_o.append(o), planes_r.append(r)
        orgs.append(capi.DevPicture(ctx, a.w, a.h).upload(planes_o))
        recs.append(capi.DevPicture(ctx, a.w, a.h).upload(planes_r))
        outs.append(capi.DevPicture(ctx, a.w, a.h).zero())
    n_lcu = -(-a.w // 64) * -(-a.h // 64)

    def timed(call):
        ms = []
        for k in range(a.warmup + a.calls):
            e0, e1 = ctx.event(), ctx.event()
            ctx.record(e0)
            call()
            ctx.record(e1)
            ctx.sync()
            if k >= a.warmup:
                ms.append(ctx.elapsed_ms(e0, e1))
        return statistics.median(ms)

    for n in a.pics:
        pick = lambda ps: (capi.Pic * n)(*[ps[i % len(ps)].as_pic() for i in range(n)])  # noqa: E731
        po, pr, pt = pick(orgs), pick(recs), pick(outs)  # (the outputs of pictures that share a buffer are the same picture's)
        stat_bytes = n * 3 * n_lcu * capi.SAO_STAT_BINS * 8
        d_stats, d_units = ctx.alloc(stat_bytes), ctx.alloc(n * 3 * n_lcu * 8)
        d_apply, d_res = ctx.alloc(n * 3 * n_lcu * 6), ctx.alloc(n * 16)
        lam = 0.57 * 2.0 ** ((32 - 12) / 3.0) / 16.0  # an intra picture at QP 32, on the scale of 10-bit distortions >> 4
        params = capi.sao_decide_params([(lam, lam / 2.0 ** (1 / 3.0))] * n, [(1, 1)] * n, [capi.sao_ctx_init(2, 32)] * n)
        hp = C.c_void_p(params.ctypes.data)
        base = dict(pics=n, w=a.w, h=a.h, bits=a.bits, calls=a.calls)
        ms = timed(lambda: ctx._chk(L.hmx_sao_stats_multi(ctx.h, n, po, pr, a.w, a.h, 1, d_stats.ptr)))
        print(json.dumps(dict(base, what="statistics kernel (hmx_sao_stats_multi)", ms=round(ms, 4))), flush=True)
        ctx._chk(L.hmx_set_timing(ctx.h, 1))
        cand, dec = [], []
        for k in range(a.warmup + a.calls):
            ctx._chk(L.hmx_sao_decide_multi(ctx.h, n, d_stats.ptr, a.w, a.h, hp, None, d_units.ptr, d_apply.ptr, d_res.ptr))
            t = [C.c_float(), C.c_float(), C.c_float()]
            ctx._chk(L.hmx_last_call_timing(ctx.h, *[C.byref(v) for v in t]))
            if k >= a.warmup:
                cand.append(t[0].value), dec.append(t[1].value)
        ctx._chk(L.hmx_set_timing(ctx.h, 0))
        ms_c, ms_d = statistics.median(cand), statistics.median(dec)
        print(json.dumps(dict(base, what="candidate kernel (k_sao_cand)", ms=round(ms_c, 4))), flush=True)
        print(json.dumps(dict(base, what="decision kernel (k_sao_decide)", ms=round(ms_d, 4), ctus_per_picture=n_lcu,
                              us_per_ctu_step=round(ms_d * 1e3 / n_lcu, 4))), flush=True)
        res = d_res.download(capi.SAO_RESULT_DTYPE)
        ms = timed(lambda: ctx._chk(L.hmx_sao_encode_multi(ctx.h, n, po, pr, pt, a.w, a.h, hp, None, None, d_stats.ptr, d_units.ptr,
                                                            d_apply.ptr, d_res.ptr)))
        print(json.dumps(dict(base, what="hmx_sao_encode_multi (statistics + decision + application)", ms=round(ms, 4),
                              ctus_without_sao_luma=int(res["num_no_sao"][:, 0].sum()), ctus=n * n_lcu)), flush=True)
        host = np.empty(stat_bytes, np.uint8)
        ms = timed(lambda: ctx._chk(L.hmx_download(ctx.h, C.c_void_p(host.ctypes.data), d_stats.ptr, stat_bytes)))
        print(json.dumps(dict(base, what="download of the statistics array (pageable host memory)", mbytes=round(stat_bytes / 1e6, 1), ms=round(ms, 4))), flush=True)
        for b in (d_stats, d_units, d_apply, d_res):
            b.free()
    ctx.close()


if __name__ == "__main__":
    main()
