#!/usr/bin/env python3
"""tools/qp_map_bench.py -- what a QP per block costs in the whole-picture encoder (hmx_set_qp_map), on the shape of bench.py's
headline (ai2160p10: 3840x2160, 10 bit, QP 32, pictures resident in the working layout, every picture its own plan out of --plans
distinct ones).  Four legs over the SAME blocks, one JSON line each:

  map13     a map per picture with 13 distinct QPs (slice QP - 6 .. + 6, drawn per 16x16 luma area)
  uniform   a map that holds the slice QP everywhere (the map kernel, no variation)
  nomap     no map (the single-QP kernel: the headline's call)
  calls13   what a caller could do before the map existed: 13 calls, one per QP value, each over the blocks of that QP (plans of the
            sub-lists).  TIMING ONLY: blocks of different QPs predict from each other, so 13 calls in QP order do not code the picture
            -- a caller would need one call per run of equal QPs in coding order, which is far more calls; this is the floor.

  python tools/qp_map_bench.py [--frames F] [--plans P] [--steps K] [--warmup W]

The batch is --frames pictures, or the largest multiple of 64 that fits the free memory."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thevc_amd import capi, workload  # noqa: E402

W, H, B, QP, SPREAD = 3840, 2160, 10, 32, 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--plans", type=int, default=64)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="map13,uniform,nomap,calls13")
    args = ap.parse_args()
    import torch
    free_b, _ = torch.cuda.mem_get_info()
    uw, uh = W // 4, H // 4
    F = args.frames
    per_pic = int(12.3 * W * H) + uw * uh + 18 * 140000
    if F * per_pic > 0.9 * free_b:
        F = max(64, int(0.9 * free_b / per_pic) // 64 * 64)
    n_plans = min(args.plans, F)
    ctx, L = capi.Context(bit_depth=B), capi.lib()
    tus_list = [workload.make_tus(1 + j, W, H, "mix") for j in range(n_plans)]
    pp = capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1)
    plans = ctx.intra_plans(tus_list, pp)
    # the maps: one per plan (a picture's QPs belong to its block structure), QP - 6 .. QP + 6 per 16x16 luma area
    maps = []
    for j in range(n_plans):
        rng = np.random.default_rng(5000 + j)
        a = QP + rng.integers(-SPREAD, SPREAD + 1, ((uh + 3) // 4, (uw + 3) // 4))
        maps.append(np.ascontiguousarray(np.repeat(np.repeat(a, 4, 0), 4, 1)[:uh, :uw].astype(np.int8)))
    assert all(len(np.unique(m)) == 2 * SPREAD + 1 for m in maps)
    d_map, d_uni = ctx.alloc(F * uw * uh), ctx.to_device(np.full((uh, uw), QP, np.int8))
    for i in range(F):
        ctx._chk(L.hmx_upload(ctx.h, d_map.ptr + i * uw * uh, maps[i % n_plans].ctypes.data_as(C.c_void_p), uw * uh))
    # pictures resident in the working layout, as in bench.py
    src = [workload.make_planes(1000 + k, W, H, B, "texture") for k in range(min(F, 16))]
    p_org, p_rec = capi.ResidentPool(ctx, W, H, F), capi.ResidentPool(ctx, W, H, F)
    stage = [capi.DevPicture(ctx, W, H).upload(s) for s in src]
    for i0 in range(0, F, len(stage)):
        p_org.import_planes(i0, stage[:min(len(stage), F - i0)])
    ctx.sync()
    lev_slab = capi.DevLevelsZSlab(ctx, W, H, F).zero()
    lev_arr = (capi.Levels * F)(*[lev_slab.as_pic(i) for i in range(F)])
    plan_arr = (C.c_void_p * F)(*[plans[i % n_plans].value for i in range(F)])

    def encode(parr):
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, 1, F, p_org.h_, p_rec.h_, lev_arr))

    def timed(step):
        for _ in range(args.warmup):
            step()
        ctx.sync()
        e0, e1 = ctx.event(), ctx.event()
        ctx.record(e0)
        for _ in range(args.steps):
            step()
        ctx.record(e1)
        ctx.sync()
        return ctx.elapsed_ms(e0, e1) / args.steps

    results = {}
    for leg in args.legs.split(","):
        t0 = time.perf_counter()
        if leg == "map13":
            ctx.set_qp_map(d_map, F)
            ms = timed(lambda: encode(plan_arr))
        elif leg == "uniform":
            ctx.set_qp_map(d_uni, 1)
            ms = timed(lambda: encode(plan_arr))
        elif leg == "nomap":
            ctx.set_qp_map(None)
            ms = timed(lambda: encode(plan_arr))
        elif leg == "calls13":
            ctx.set_qp_map(None)
            subs = []  # per QP value: the plans of the blocks that hold it, one per structure
            for v in range(QP - SPREAD, QP + SPREAD + 1):
                lists = []
                for j, t in enumerate(tus_list):
                    sh = (t["plane"] != 0).astype(np.int64)
                    q = maps[j][(t["y"].astype(np.int64) << sh) >> 2, (t["x"].astype(np.int64) << sh) >> 2]
                    lists.append(np.ascontiguousarray(t[q == v]))
                ppv = capi.PicParam(W, H, v, 0, capi.I_SLICE, 1)
                pl = ctx.intra_plans(lists, ppv)
                subs.append((pl, (C.c_void_p * F)(*[pl[i % n_plans].value for i in range(F)])))

            def step13():
                for _, parr in subs:
                    encode(parr)
            ms = timed(step13)
            for pl, _ in subs:
                for x in pl:
                    L.hmx_intra_plan_destroy(ctx.h, x)
        else:
            raise SystemExit(f"unknown leg {leg}")
        ctx.set_qp_map(None)
        results[leg] = ms
        print(json.dumps({"leg": leg, "ms_per_step": round(ms, 3), "pictures": F, "plans": n_plans, "gpx_per_s": round(F * W * H / ms / 1e6, 2),
                          "wall_s": round(time.perf_counter() - t0, 1)}), flush=True)
    if "nomap" in results:
        print(json.dumps({"ratios_to_nomap": {k: round(v / results["nomap"], 4) for k, v in results.items()}}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
