"""Throughput of the picture-level kernels either side of the chain on one 2160p picture set: deblocking (strengths +
application), SAO, YUV unpack / pack: picture by picture and, for the loop filters, the whole set in one call.  Every line is
the median of --repeats timings with their min..max; the last line is SAO on the availability path (hmx_sao_picture_multi_avail)
with the mask of 4 x 4 tiles that the filters may not cross.  With HMX_LIB_PATH naming an older build of the library the batched
lines are left out: its per-picture lines are the baseline of DESIGN.md section 5."""
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
ap.add_argument("--repeats", type=int, default=5)
REPEATS = ap.parse_args().repeats
B, w, h, NP = 10, 3840, 2160, 16
ctx = capi.Context(bit_depth=B)
L = capi.lib()
rng = np.random.default_rng(1)
pics = [capi.DevPicture(ctx, w, h).upload(workload.make_planes(i, w, h, B, "texture")) for i in range(2)]
pics += [capi.DevPicture(ctx, w, h).zero() for _ in range(NP - 2)]
outs = [capi.DevPicture(ctx, w, h).zero() for _ in range(NP)]
uw, uh = w // 4, h // 4
units = np.zeros(uw * uh, np.dtype([("intra", "u1"), ("cbf", "u1"), ("ref", "i1", 2), ("mv", "<i2", (2, 2))]))
units["intra"] = rng.random(uw * uh) < 0.2
units["cbf"] = rng.random(uw * uh) < 0.4
units["mv"] = rng.integers(-8, 9, (uw * uh, 2, 2))
edge = ((np.arange(uw)[None, :] % 2 == 0) * 3).astype(np.uint8).repeat(uh, 0).copy()
d_units, d_ev, d_eh = ctx.to_device(units), ctx.to_device(edge), ctx.to_device(edge)
d_bv, d_bh = ctx.alloc(uw * uh), ctx.alloc(uw * uh)
d_qp = ctx.to_device(np.full(uw * uh, 32, np.int8))
n_lcu = 60 * 34
sao = np.zeros((3, n_lcu), np.dtype([("type", "i1"), ("band", "u1"), ("offset", "i1", 4)]))
sao["type"] = rng.integers(-1, 5, (3, n_lcu))
sao["offset"] = rng.integers(-3, 4, (3, n_lcu, 4))
d_sao = ctx.to_device(np.ascontiguousarray(sao))
nbytes = L.hmx_yuv_frame_bytes(w, h, 10)
d_file = ctx.alloc(nbytes)


def timed(fn, reps=3):
    """seconds per picture: REPEATS timings of `reps` passes over the NP pictures, after one pass to warm up"""
    fn()
    ctx.sync()
    out = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) / reps / NP)
    return out


def line(name, ts, note=""):
    t = float(np.median(ts))
    print(f"{name:<27s} {t * 1e6:8.1f} us/picture (min {min(ts) * 1e6:.1f}, max {max(ts) * 1e6:.1f}; {len(ts)} repeats)  {px / t / 1e9:6.1f} Gpx/s{note}")


def per_pic(f):
    def g():
        for i in range(NP):
            f(i)
    return g


px = w * h
t = timed(per_pic(lambda i: ctx._chk(L.hmx_deblock_strengths(ctx.h, d_units.ptr, d_ev.ptr, d_eh.ptr, w, h, 1, d_bv.ptr, d_bh.ptr))))
line("deblock strengths", t)
t = timed(per_pic(lambda i: ctx._chk(L.hmx_deblock_picture(ctx.h, C.byref(pics[i].as_pic()), w, h, d_bv.ptr, d_bh.ptr, d_qp.ptr, None, 0, 0))))
line("deblock picture", t, f"  ({6 * px / np.median(t) / 1e9:.0f} GB/s of 2 B read + 2 B written per sample)")
t = timed(per_pic(lambda i: ctx._chk(L.hmx_sao_picture(ctx.h, C.byref(pics[i].as_pic()), C.byref(outs[i].as_pic()), w, h, d_sao.ptr, n_lcu))))
line("SAO", t, f"  ({6 * px / np.median(t) / 1e9:.0f} GB/s of 2 B read + 2 B written per sample)")
t = timed(per_pic(lambda i: ctx._chk(L.hmx_yuv_pack(ctx.h, C.byref(pics[i].as_pic()), w, h, 0, 0, 10, d_file.ptr))))
line("YUV pack (10-bit)", t)
t = timed(per_pic(lambda i: ctx._chk(L.hmx_yuv_unpack(ctx.h, d_file.ptr, 10, C.byref(outs[i].as_pic()), w, h, 0, 0))))
line("YUV unpack (10-bit)", t)
# one picture alone, as a caller without a batch sees it (launch and synchronisation included)
t = [x * NP for x in timed(lambda: ctx._chk(L.hmx_deblock_picture(ctx.h, C.byref(pics[0].as_pic()), w, h, d_bv.ptr, d_bh.ptr, d_qp.ptr, None, 0, 0)), reps=20)]
line("deblock picture, 1 alone", t)
if hasattr(L, "hmx_deblock_picture_multi"):  # the NP pictures in one call each, every picture with its own maps
    rep = lambda a: ctx.to_device(np.ascontiguousarray(np.broadcast_to(a, (NP,) + a.shape)))
    m_units, m_ev, m_eh, m_qp, m_sao = rep(units), rep(edge), rep(edge), rep(np.full(uw * uh, 32, np.int8)), rep(sao)
    m_bv, m_bh = ctx.alloc(NP * uw * uh), ctx.alloc(NP * uw * uh)
    is_b = np.ones(NP, np.uint8)
    t = timed(lambda: ctx.deblock_strengths(NP, m_units, m_ev, m_eh, w, h, is_b, m_bv, m_bh))
    line(f"deblock strengths, {NP} a call", t)
    t = timed(lambda: ctx.deblock_pictures(pics, w, h, m_bv, m_bh, m_qp))
    line(f"deblock picture, {NP} a call", t, f"  ({6 * px / np.median(t) / 1e9:.0f} GB/s of 2 B read + 2 B written per sample)")
    t = timed(lambda: ctx.sao_pictures(pics, outs, w, h, m_sao))
    line(f"SAO, {NP} a call", t, f"  ({6 * px / np.median(t) / 1e9:.0f} GB/s of 2 B read + 2 B written per sample)")
if hasattr(L, "hmx_sao_picture_multi_avail"):  # the same with loop filters that stop at the boundaries of 4 x 4 tiles
    from thevc_amd import decisions
    _, tile_id = decisions.slice_tile_maps(w, h, 64, (0,), decisions.uniform_bounds(60, 4), decisions.uniform_bounds(34, 4))
    avail = decisions.lf_border_avail(w, h, 64, tile_id=tile_id, lf_cross_tiles=False)
    m_avail = ctx.to_device(np.ascontiguousarray(np.broadcast_to(avail, (NP, n_lcu))))
    t = timed(lambda: ctx.sao_pictures_avail(pics, outs, w, h, m_sao, m_avail))
    line(f"SAO avail, {NP} a call", t, f"  ({6 * px / np.median(t) / 1e9:.0f} GB/s of 2 B read + 2 B written per sample)")
