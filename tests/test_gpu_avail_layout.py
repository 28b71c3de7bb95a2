"""Intra availability with slices, tiles and constrained intra prediction on the GPU: stream fixtures of the reference
encoder decoded through libhmx, the encoder direction, whole-picture calls with random layouts under every schedule,
device-built plans, the block-list calls and the scalar drop-ins, each against the CPU oracle (tests/layout_oracle.py)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import layout_oracle as LO
import oracle_lib as ol
from test_avail_layout import random_layout
from thevc_amd import decisions as D
from thevc_amd.workload import make_planes, make_tus

HERE = os.path.dirname(os.path.abspath(__file__))
LAYOUT_FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "layout_*.npz")))
pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", LAYOUT_FIXTURES, ids=[os.path.basename(f)[:-4] for f in LAYOUT_FIXTURES])
def test_gpu_decodes_layout_streams(path):
    pics = list(D.load_pictures(path))
    for p, got in zip(pics, D.decode_sequence(pics)):
        for k in range(3):
            bad = np.argwhere(got[k] != p["rec"][k])
            assert not len(bad), (os.path.basename(path), p["poc"], k, bad[0].tolist(), len(bad))


@pytest.mark.parametrize("path", [f for f in LAYOUT_FIXTURES if "intra" in os.path.basename(f) and "rdoq0" in f])
def test_gpu_encodes_layout_streams_like_the_reference_encoder(path):
    from thevc_amd import capi
    L = capi.lib()
    pics = list(D.load_pictures(path))
    ctx = capi.Context(bit_depth=pics[0]["B"], ctu_size=pics[0]["ctu"])
    try:
        for p in pics:
            w, h = p["w"], p["h"]
            plan = ctx.intra_plan(p["tus"], capi.PicParam(w, h, p["qp"], 0, capi.I_SLICE, 1), layout=D.layout_of(p))
            d_org, d_rec = capi.DevPicture(ctx, w, h).upload(p["org"]), capi.DevPicture(ctx, w, h).zero()
            d_lev = capi.DevLevelsZ(ctx, w, h, p["ctu"]).zero()
            ctx._chk(L.hmx_frame_intra_encode(ctx.h, plan, 1, (capi.Pic * 1)(d_org.as_pic()), (capi.Pic * 1)(d_rec.as_pic()),
                                              (capi.Levels * 1)(d_lev.as_pic())))
            ctx.sync()
            got = d_rec.download()
            for k in range(3):
                assert np.array_equal(d_lev.bufs[k].download(np.int32), p["lev"][k]), (p["poc"], "levels", k)
                assert np.array_equal(got[k], p["rec"][k]), (p["poc"], "reconstruction", k)
            L.hmx_intra_plan_destroy(ctx.h, plan)
    finally:
        ctx.close()


def _levels(rng, tus, w, h):
    """Sparse random levels in plane geometry (small values: the reconstruction stays inside the sample range often
    enough to carry neighbour differences)."""
    lev = [np.zeros((h, w), np.int32), np.zeros((h // 2, w // 2), np.int32), np.zeros((h // 2, w // 2), np.int32)]
    for t in tus:
        n, k, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        blk = rng.integers(-12, 13, (n, n)) * (rng.random((n, n)) < 0.15)
        lev[k][y:y + n, x:x + n] = blk
    return lev


@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("schedule", ["packed", "level", "wave"])
def test_gpu_random_layouts_every_schedule(B, schedule):
    """Workload pictures with random slice / tile / CIP layouts through hmx_frame_intra_decode_multi: the oracle
    composition, with host plans and (packed / level) device-built plans whose tables equal the host plans'."""
    from thevc_amd import capi
    L = capi.lib()
    w, h, qp = 416, 240, 30
    rng = np.random.default_rng(B * 10 + len(schedule))
    ctx = capi.Context(bit_depth=B, ctu_size=64)
    try:
        ctx._chk(L.hmx_set_option(ctx.h, b"HMX_INTRA_SCHEDULE", schedule.encode()))
        pics, lays = [], []
        for i in range(3):
            tus = np.ascontiguousarray(make_tus(100 + i + B, w, h), ol.TU_DTYPE)
            region, intra = random_layout(rng, w, h)
            pics.append((tus, _levels(rng, tus, w, h), region, intra))
            lays.append(capi.Layout(region, intra))
        pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
        plans = ctx.intra_plans([t for t, _, _, _ in pics], pp, lays)
        variants = [plans]
        if schedule != "wave":
            offs = np.cumsum([0] + [len(t) for t, _, _, _ in pics])
            d_tus = ctx.to_device(np.concatenate([t for t, _, _, _ in pics]))
            dplans = ctx.intra_plans_device_layout(d_tus.ptr, offs, pp, lays)
            for a, b in zip(plans, dplans):
                ba, la = ctx.plan_tables(a)
                bb, lb = ctx.plan_tables(b)
                assert np.array_equal(ba, bb) and np.array_equal(la, lb)
            variants.append(dplans)
        want = []
        for tus, lev, region, intra in pics:
            rec = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
            LO.intra_blocks(tus, rec, lev, w, h, B, qp, LO.Region(region, w), intra)
            want.append(rec)
        for pl in variants:
            d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in pics]
            d_lev = [capi.DevPicture(ctx, w, h, dtype=np.int32).upload(lev) for _, lev, _, _ in pics]
            arr = (C.c_void_p * len(pl))(*[q.value for q in pl])
            ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, arr, len(pl), (capi.Pic * len(pics))(*[d.as_pic() for d in d_rec]),
                                                    (capi.Levels * len(pics))(*[d.as_pic() for d in d_lev])))
            ctx.sync()
            for i, d in enumerate(d_rec):
                got = d.download()
                for k in range(3):
                    assert np.array_equal(got[k], want[i][k]), (schedule, i, k, int((got[k] != want[i][k]).sum()))
        geo = []  # the layouts matter for these pictures
        for tus, lev, _, _ in pics[:1]:
            rec = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
            LO.intra_blocks(tus, rec, lev, w, h, B, qp, None, None)
            geo.append(rec)
        assert any((geo[0][k] != want[0][k]).any() for k in range(3))
        for q in plans + (variants[1] if len(variants) > 1 else []):
            L.hmx_intra_plan_destroy(ctx.h, q)
    finally:
        ctx.close()


def test_gpu_plans_null_layout_and_tiles_and_bad_layouts():
    """A NULL layout gives the tables of hmx_intra_plan_create; 2 x 2 tiles on a 1080p workload picture give strictly fewer
    dependency levels; a malformed layout is refused with HMX_ERR_ARG; a 1080p picture with tiles decodes like the oracle."""
    from thevc_amd import capi
    L = capi.lib()
    ctx = capi.Context(bit_depth=8, ctu_size=64)
    try:
        for path in LAYOUT_FIXTURES[:2]:
            p = next(D.load_pictures(path))
            pp = capi.PicParam(p["w"], p["h"], p["qp"], 0, capi.I_SLICE, 1)
            a, b = ctx.intra_plan(p["tus"], pp), ctx.intra_plan(p["tus"], pp, layout=capi.Layout())
            ta, tb = ctx.plan_tables(a), ctx.plan_tables(b)
            assert np.array_equal(ta[0], tb[0]) and np.array_equal(ta[1], tb[1])
            L.hmx_intra_plan_destroy(ctx.h, a), L.hmx_intra_plan_destroy(ctx.h, b)
        w, h, qp = 1920, 1080, 32
        tus = np.ascontiguousarray(make_tus(7, w, h), ol.TU_DTYPE)
        pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
        region = D.region_map(w, h, 64, [0], D.uniform_bounds(30, 2), D.uniform_bounds(17, 2))
        one, tiled = ctx.intra_plan(tus, pp), ctx.intra_plan(tus, pp, layout=capi.Layout(region))
        nl = []
        for q in (one, tiled):
            n = C.c_int()
            L.hmx_intra_plan_info(q, None, C.byref(n), None)
            nl.append(n.value)
        assert nl[1] < nl[0], nl
        rng = np.random.default_rng(1)
        lev = _levels(rng, tus, w, h)
        want = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        LO.intra_blocks(tus, want, lev, w, h, 8, qp, LO.Region(region, w), None)
        d_rec, d_lev = capi.DevPicture(ctx, w, h).zero(), capi.DevPicture(ctx, w, h, dtype=np.int32).upload(lev)
        ctx._chk(L.hmx_frame_intra_decode(ctx.h, tiled, 1, (capi.Pic * 1)(d_rec.as_pic()), (capi.Levels * 1)(d_lev.as_pic())))
        ctx.sync()
        got = d_rec.download()
        for k in range(3):
            assert np.array_equal(got[k], want[k]), k
        L.hmx_intra_plan_destroy(ctx.h, one), L.hmx_intra_plan_destroy(ctx.h, tiled)
        h_out = C.c_void_p()
        bad = capi.AvailLayout()
        bad.constrained_intra_pred = 1
        assert L.hmx_intra_plan_create_layout(ctx.h, tus.ctypes.data, len(tus), C.byref(pp), C.byref(bad), C.byref(h_out)) == -1
        short = capi.Layout(region[:-1])
        assert L.hmx_intra_plan_create_layout(ctx.h, tus.ctypes.data, len(tus), C.byref(pp), short.ref(), C.byref(h_out)) == -1
    finally:
        ctx.close()


@pytest.mark.parametrize("B", [8, 10])
def test_gpu_batch_pred_layout(B):
    """hmx_batch_predIntra_layout and _cost_layout (35 modes, 64x64 prediction units included) against the oracle's
    prediction from the layout's flags, on a random reconstruction."""
    from thevc_amd import capi
    L = capi.lib()
    O = ol.oracle()
    w, h = 416, 240
    rng = np.random.default_rng(40 + B)
    ctx = capi.Context(bit_depth=B, ctu_size=64)
    try:
        rec = make_planes(5 + B, w, h, B)
        region, intra = random_layout(rng, w, h, cip=True)
        lay = capi.Layout(region, intra)
        tus = np.ascontiguousarray(make_tus(9 + B, w, h), ol.TU_DTYPE)
        extra = np.zeros(6, ol.TU_DTYPE)  # 64x64 luma prediction units
        for i, (x, y) in enumerate([(0, 0), (64, 0), (128, 64), (320, 64), (64, 128), (256, 128)]):
            extra[i] = (x, y, 6, 0, int(rng.integers(0, 35)), 0)
        pp = capi.PicParam(w, h, 30, 0, capi.I_SLICE, 1)
        d_rec = capi.DevPicture(ctx, w, h).upload(rec)
        reg = LO.Region(region, w)
        n_diff = 0
        for blocks in (tus, extra):  # the 64x64 units cover blocks of the first list: a prediction picture of their own
            tl = ctx.tu_list(blocks)
            d_pred = capi.DevPicture(ctx, w, h).zero()
            ctx._chk(L.hmx_batch_predIntra_layout(ctx.h, tl, C.byref(d_rec.as_pic()), C.byref(d_pred.as_pic()), C.byref(pp), lay.ref(), None, 0, None))
            ctx.sync()
            got = d_pred.download()
            L.hmx_tu_list_destroy(ctx.h, tl)
            for t in blocks:
                k, N, x, y, mode = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["mode"])
                sh = 1 if k else 0
                ulog2 = 3 if N == 64 else 2
                geo_bits = L.hmx_intra_avail_mask_layout(x << sh, y << sh, N << sh, w, h, None)
                n = (N << sh) >> ulog2
                geo = np.array([(geo_bits >> u) & 1 for u in range(4 * n + 1)], np.uint8)
                f = LO.layout_flags(geo, x << sh, y << sh, N << sh, ulog2, reg, intra)
                n_diff += int((f != geo).any())
                if N == 64:  # the oracle fills in units of 4: every 8-sample unit twice
                    f4 = np.zeros(65, np.uint8)
                    f4[0:32] = np.repeat(f[0:16], 2)
                    f4[32] = f[16]
                    f4[33:65] = np.repeat(f[17:33], 2)
                    f = f4
                flags = np.zeros(65, np.uint8)
                flags[:f.size] = f
                plane = np.ascontiguousarray(rec[k]).reshape(-1)
                W = 2 * N + 1
                adi = np.zeros(2 * W * W, np.int32)
                O.hmo_fillReferenceSamples(ol.ptr(plane, y * rec[k].shape[1] + x), rec[k].shape[1], flags, int(f.sum()), 2 if k else 4, N, B, adi)
                pred = np.zeros((N, N), np.int16)
                if k:
                    O.hmo_predIntraChromaAng(adi, mode, pred.reshape(-1), N, N, B)
                else:
                    O.hmo_filterAdi(adi, N)
                    O.hmo_predIntraLumaAng(adi, mode, pred.reshape(-1), N, N, B)
                assert np.array_equal(got[k][y:y + N, x:x + N], pred), (k, N, x, y, mode)
        assert n_diff > 50, n_diff
        # the cost form (35 modes from one gather, 64x64 units included): without a layout it is hmx_batch_predIntra_cost, with
        # one it follows the predictions above (the same gather feeds both)
        tl = ctx.tu_list(np.concatenate([tus, extra]))
        org = make_planes(77 + B, w, h, B)
        d_org = capi.DevPicture(ctx, w, h).upload(org)
        modes = ctx.to_device(np.arange(35, dtype=np.uint8))
        n_all = len(tus) + len(extra)
        d_a, d_b, d_c = (ctx.to_device(np.zeros(n_all * 35, np.uint32)) for _ in range(3))
        ctx._chk(L.hmx_batch_predIntra_cost_layout(ctx.h, tl, C.byref(d_rec.as_pic()), C.byref(d_org.as_pic()), C.byref(pp), lay.ref(), modes.ptr, 35, d_a.ptr))
        ctx._chk(L.hmx_batch_predIntra_cost_layout(ctx.h, tl, C.byref(d_rec.as_pic()), C.byref(d_org.as_pic()), C.byref(pp), None, modes.ptr, 35, d_b.ptr))
        ctx._chk(L.hmx_batch_predIntra_cost(ctx.h, tl, C.byref(d_rec.as_pic()), C.byref(d_org.as_pic()), C.byref(pp), modes.ptr, 35, d_c.ptr))
        ctx.sync()
        a, b, c = d_a.download(np.uint32), d_b.download(np.uint32), d_c.download(np.uint32)
        assert np.array_equal(b, c) and not np.array_equal(a, b)
        L.hmx_tu_list_destroy(ctx.h, tl)
    finally:
        ctx.close()


@pytest.mark.parametrize("B", [8, 10])
def test_gpu_scalar_layout_dropins(B):
    """hmx_fillReferenceSamples against hmo_fillReferenceSamples (which tests/test_oracle_vs_ref.py pins to the reference) for
    random flag patterns, and hmx_initAdiPattern_layout against the oracle's fill + smoothing with the layout's flags."""
    from thevc_amd import capi
    O = ol.oracle()
    rng = np.random.default_rng(60 + B)
    ctx = capi.Context(bit_depth=B, ctu_size=64)
    try:
        for N, unit in [(4, 4), (8, 4), (16, 4), (32, 4), (4, 2), (8, 2), (16, 2)]:
            stride = 3 * N + 7
            plane = rng.integers(0, 1 << B, (3 * N + 3) * stride).astype(np.int16)
            org = (N + 1) * stride + N + 1
            W = 2 * N + 1
            for it in range(30):
                total = 4 * (N // unit) + 1
                f = np.zeros(total, np.uint8) if it % 5 == 0 else (rng.random(total) < rng.choice([0.2, 0.5, 0.8])).astype(np.uint8)
                flags = np.zeros(65, np.uint8)
                flags[:total] = f
                want = np.full(2 * W * W, -1, np.int32)
                O.hmo_fillReferenceSamples(ol.ptr(plane, org), stride, flags, int(f.sum()), unit, N, B, want)
                got = ctx.fillReferenceSamples(plane, org, stride, flags, int(f.sum()), unit, N, np.full(2 * W * W, -1, np.int32))
                assert np.array_equal(got, want), (N, unit, it)
        w, h = 416, 240
        rec = make_planes(3, w, h, B)
        region, intra = random_layout(rng, w, h, cip=True)
        lay, reg = capi.Layout(region, intra), LO.Region(region, w)
        for _ in range(80):
            k = int(rng.integers(0, 3))
            N = int(rng.choice([4, 8, 16] if k else [4, 8, 16, 32]))
            pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
            x, y = int(rng.integers(0, pw // N)) * N, int(rng.integers(0, ph // N)) * N
            sh = 1 if k else 0
            geo = LO.geometric_flags(x << sh, y << sh, N << sh, w, h)
            f = LO.layout_flags(geo, x << sh, y << sh, N << sh, 2, reg, intra)
            flags = np.zeros(65, np.uint8)
            flags[:f.size] = f
            W = 2 * N + 1
            want = np.zeros(2 * W * W, np.int32)
            p = np.ascontiguousarray(rec[k]).reshape(-1)
            O.hmo_fillReferenceSamples(ol.ptr(p, y * pw + x), pw, flags, int(f.sum()), 2 if k else 4, N, B, want)
            if not k:
                O.hmo_filterAdi(want, N)
            got = ctx.initAdiPattern_layout(p, pw, x, y, N, int(k != 0), w, h, lay)
            n = W * W if k else 2 * W * W
            assert np.array_equal(got[:n], want[:n]), (k, N, x, y)
    finally:
        ctx.close()
