"""Dependency levels of a workload picture with one region and with uniform tiles: the picture-wide level walk of the plan
builder (plan_build_host: level = 1 + the highest level among the units a block depends on), from the host functions
hmx_intra_avail_mask_layout and hmx_intra_dependency_mask.  No GPU; --gpu prints hmx_intra_plan_info of real plans too.

  python3 tools/layout_levels.py [--w 1920 --h 1080 --tiles 2x2 --seed 7 --tiling mix] [--gpu]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from thevc_amd import capi  # noqa: E402
from thevc_amd import decisions as D  # noqa: E402
from thevc_amd.workload import make_tus  # noqa: E402


def walk_levels(tus, w, h, layout):
    L = capi.lib()
    uw, uh = (w + 63) // 64 * 16, (h + 63) // 64 * 16
    g = [np.zeros((uh, uw), np.int32) for _ in range(3)]
    top = 0
    lay = None if layout is None else layout.ref()
    for t in tus:
        pl = int(t["plane"])
        sh = 1 if pl else 0
        N = 1 << int(t["log2n"])
        lx, ly, ls = int(t["x"]) << sh, int(t["y"]) << sh, N << sh
        n, ux, uy = ls // 4, lx // 4, ly // 4
        m = L.hmx_intra_dependency_mask(N, int(pl == 0), int(t["mode"]), L.hmx_intra_avail_mask_layout(lx, ly, ls, w, h, lay))
        lv = 0
        while m:
            u = (m & -m).bit_length() - 1
            m &= m - 1
            qx, qy = (ux - 1, uy + 2 * n - 1 - u) if u < 2 * n else ((ux - 1, uy - 1) if u == 2 * n else (ux + (u - 2 * n - 1), uy - 1))
            lv = max(lv, int(g[pl][qy, qx]))
        g[pl][uy:uy + n, ux:ux + n] = lv + 1
        top = max(top, lv + 1)
    return top


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=1920)
    ap.add_argument("--h", type=int, default=1080)
    ap.add_argument("--tiles", default="2x2")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--tiling", default="mix")
    ap.add_argument("--gpu", action="store_true", help="also build the plans (hmx_intra_plan_create[_layout]) and print hmx_intra_plan_info")
    a = ap.parse_args()
    w, h = a.w, a.h
    tc, tr = (int(v) for v in a.tiles.split("x"))
    cw, ch = -(-w // 64), -(-h // 64)
    tus = np.ascontiguousarray(make_tus(a.seed, w, h, a.tiling), capi.TU_DTYPE)
    region = D.region_map(w, h, 64, [0], D.uniform_bounds(cw, tc), D.uniform_bounds(ch, tr))
    layouts = {"one region": None, f"{tc}x{tr} tiles": capi.Layout(region)}
    print(f"{w}x{h}, {len(tus)} blocks (workload seed {a.seed}, tiling {a.tiling})")
    for name, lay in layouts.items():
        print(f"  {name:>12}: {walk_levels(tus, w, h, lay)} dependency levels (host walk)")
    if a.gpu:
        import ctypes as C
        ctx = capi.Context(bit_depth=8, ctu_size=64)
        try:
            pp = capi.PicParam(w, h, 32, 0, capi.I_SLICE, 1)
            for name, lay in layouts.items():
                plan = ctx.intra_plan(tus, pp, layout=lay)
                nb, nl, nd = C.c_int(), C.c_int(), C.c_int()
                capi.lib().hmx_intra_plan_info(plan, C.byref(nb), C.byref(nl), C.byref(nd))
                print(f"  {name:>12}: hmx_intra_plan_info: {nb.value} blocks, {nl.value} levels, {nd.value} CTU diagonals")
                capi.lib().hmx_intra_plan_destroy(ctx.h, plan)
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
