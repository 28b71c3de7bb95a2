#!/usr/bin/env python3
"""tools/ref_skip_shares.py [--pictures 64] [--size 3840x2160] [--tiling mix] [--group 64] [--slots8 16] -- the share of the packed
schedule's wave-items, per size class, that take each wave-uniform skip of the reference line (hmx_kernels.h, intra_refs_tiled): no
padding pass (no block of the wave-item reads an unavailable unit), no smoothed line (none predicts from it), no DC sum (none is
DC), and, of those that run the padding pass, the share on its index-clamp path against the general rule; then the share that hold
each mode class (planar, DC, pure vertical / horizontal, angular) and a transform-skip block -- a wave runs every prediction and transform
arm one of its lanes takes -- and the share that hold more than one code-path class (k_pack_fill orders a bucket by that class).  Counted on the host from the tables of one real call (hmx_last_call_pack_tables) with the bench's plans (seeds 1.., one plan
per picture), in the shape the bench's 2048 pictures run in: packing groups of 64, sixteen 8x8 blocks per wave-item (a call of 64
pictures would choose groups of one by itself).  Needs a GPU."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from thevc_amd import capi, workload  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--pictures", type=int, default=64)
ap.add_argument("--size", default="3840x2160")
ap.add_argument("--tiling", default="mix")
ap.add_argument("--group", default="64", help="HMX_PACK_GROUP")
ap.add_argument("--slots8", default="16", help="HMX_PACK_SLOTS8")
a = ap.parse_args()
w, h = (int(v) for v in a.size.split("x"))
h = (h + 7) // 8 * 8
tiling = a.tiling if a.tiling == "mix" else int(a.tiling)
n, B, qp = a.pictures, 10, 32
L = capi.lib()
ctx = capi.Context(bit_depth=B)
ctx.set_option("HMX_INTRA_SCHEDULE", "packed")
ctx.set_option("HMX_PACK_GROUP", a.group)
ctx.set_option("HMX_PACK_SLOTS8", a.slots8)
pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
tus = [workload.make_tus(1 + i, w, h, tiling) for i in range(n)]
plans = ctx.intra_plans(tus, pp)
org = capi.DevPicture(ctx, w, h).upload(workload.make_planes(1, w, h, B, "texture"))
rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
lev = [capi.DevPicture(ctx, w, h, dtype=np.int32).zero() for _ in range(n)]
arr = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
ctx._chk(L.hmx_frame_intra_encode_multi(ctx.h, (C.c_void_p * n)(*[p.value for p in plans]), n, arr([org] * n, capi.Pic), arr(rec, capi.Pic),
                                        arr(lev, capi.Levels)))
g, _, _, descs, items, _ = ctx.pack_tables()
ctx.sync()
# per item: reach[size][luma][mode] = the dependency mask with every unit available; an item pads when its mask lacks a unit of it
reach = np.zeros((4, 2, 35), np.uint64)
for lg in range(4):
    for lu in range(2):
        if lg == 3 and lu == 0:
            continue  # no 32x32 chroma
        units = (4 << lg) // (4 if lu else 2) * 4 + 1
        for m in range(35):
            reach[lg, lu, m] = L.hmx_intra_dependency_mask(4 << lg, lu, m, (1 << units) - 1)
lg, luma, mode = items["log2n"].astype(np.int64) - 2, ((items["plane"] & 3) == 0).astype(np.int64), items["mode"].astype(np.int64)
pads = (reach[lg, luma, mode] & ~items["avail"]) != 0
thr = np.array([10, 7, 1, 0])[lg]
smooth = (luma == 1) & (lg > 0) & (mode != 1) & (np.minimum(np.abs(mode - 10), np.abs(mode - 26)) > thr)  # use_filtered_refs
dc = mode == 1
off, cnt, cls = descs["item_off"].astype(np.int64), (descs["n_s"] & 0x0fffffff).astype(np.int64), (descs["n_s"] >> 28).astype(np.int64)
order = np.argsort(off)  # the items of the wave-items tile the item array
off, cnt, cls = off[order], cnt[order], cls[order]
assert (off[1:] == off[:-1] + cnt[:-1]).all() and off[0] == 0 and off[-1] + cnt[-1] == len(items)
print(f"{n} pictures {w}x{h}, tiling {tiling}, groups of {g.I}, slots {g.slots4}/{g.slots8}: {len(items)} blocks in {len(descs)} wave-items")
for name, flag in (("pads", pads), ("smoothed", smooth), ("DC", dc)):
    some = np.add.reduceat(flag.astype(np.int64), off) > 0
    for s in range(4):
        k = cls == s
        if k.any():
            blocks = np.concatenate([[0], np.cumsum(flag)])  # share of BLOCKS with the property, for comparison
            nb = (blocks[off[k] + cnt[k]] - blocks[off[k]]).sum()
            print(f"  {name:8s} {4 << s:2d}x{4 << s:<2d}: blocks {nb / cnt[k].sum():.3f}, wave-items with one {some[k].mean():.3f} -> skip taken by {1 - some[k].mean():.3f} of {k.sum()}")
# the padding pass has three paths: none (above), the index clamp while every padding block of the wave-item is simple
# (hmx_intra_pads_simple: no unit read and missing between units of the mask), the general rule otherwise
simple = np.zeros(len(items), bool)
if hasattr(L, "hmx_intra_pads_simple"):  # (absent from an older build loaded through HMX_LIB_PATH); one call per distinct (size, type, mode, mask)
    key = np.stack([lg.astype(np.uint64), luma.astype(np.uint64), mode.astype(np.uint64), items["avail"].astype(np.uint64)], axis=1)
    uniq, inv = np.unique(key, axis=0, return_inverse=True)
    simple = np.array([L.hmx_intra_pads_simple(4 << int(u[0]), int(u[1]), int(u[2]), int(u[3])) != 0 for u in uniq])[inv.reshape(-1)]
wave_of = np.repeat(np.arange(len(off)), cnt)  # the wave-item of every item
any_pad = np.add.reduceat(pads.astype(np.int64), off) > 0
any_general = np.add.reduceat((pads & ~simple).astype(np.int64), off) > 0
for s in range(4):
    k = cls == s
    if k.any():
        print(f"  paths    {4 << s:2d}x{4 << s:<2d}: no padding {(~any_pad[k]).mean():.3f}, clamp {(any_pad[k] & ~any_general[k]).mean():.3f}, general {any_general[k].mean():.3f} of {k.sum()} wave-items"
              f" (blocks that pad: {pads[k[wave_of]].mean():.3f}, of them simple {simple[pads & k[wave_of]].mean():.3f})")
# the arms of intra_pred_samples and of the 4x4 chain's transform: per lane by mode class and transform skip, so a wave-item runs every
# one that occurs in it; and the code-path class k_pack_fill orders a bucket by (plane class, transform skip, pads, mode class)
mc = np.where(mode == 0, 0, np.where(mode == 1, 1, np.where((mode == 10) | (mode == 26), 2, 3)))
ts = (items["flags"] & 1).astype(np.int64)
path = ((1 - luma) << 4) | (ts << 3) | (pads.astype(np.int64) << 2) | mc
for name, flag in (("planar", mc == 0), ("DC", mc == 1), ("pure V/H", mc == 2), ("angular", mc == 3), ("tr. skip", ts == 1)):
    some = np.add.reduceat(flag.astype(np.int64), off) > 0
    for s in range(4):
        k = cls == s
        if k.any():
            print(f"  {name:8s} {4 << s:2d}x{4 << s:<2d}: blocks {flag[k[wave_of]].mean():.3f}, wave-items with one {some[k].mean():.3f}")
arms = sum((np.add.reduceat((mc == v).astype(np.int64), off) > 0).astype(np.int64) for v in range(4))
lo, hi = np.minimum.reduceat(path, off), np.maximum.reduceat(path, off)
for s in range(4):
    k = cls == s
    if k.any():
        print(f"  classes  {4 << s:2d}x{4 << s:<2d}: wave-items with more than one code-path class {(lo[k] != hi[k]).mean():.3f}, prediction arms per wave-item {arms[k].mean():.2f} of {k.sum()}")
