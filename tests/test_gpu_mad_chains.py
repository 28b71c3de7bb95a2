"""The transform passes as multiply-add chains and the 4-point DST as butterflies (thevc_amd/csrc/hmx_transform.h) cannot change a
result: whole-picture parity against the CPU oracle, levels and reconstruction, through the packed whole-picture entry in both
directions.

  * one 64x64 picture per case: uniform tilings 4, 8, 16, 32 and the mix, at 8, 10 and 12 bit;
  * originals at the range ends (all 0, all 2^B - 1: extreme_inputs.opposite_ends), checkerboards of the two extremes with squares of
    one and of four samples, every sample one of the extremes at random (extreme_inputs.extreme_plane "binary"), and one noise picture:
    the residuals reach +-(2^B - 1) and the first-pass outputs their bounds, where a product or a sum that lost a bit would show;
  * both wave-item shapes of the 8x8 blocks (eight and sixteen per wave-item: different kernels);
  * the 4x4 tiling holds luma blocks (DST), chroma blocks (DCT) and transform-skip blocks: checked in the set-up;
  * one case through the block-list kernels at 16 and 32 (hmx_batch_residual_transform_recon_multi: forward, quantiser, inverse and
    reconstruction) against the oracle's transformNxN / invtransformNxN block by block."""
import ctypes as C
import functools

import numpy as np
import pytest

import extreme_inputs as xi
import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

W = H = 64
QP = 22
TILINGS = [4, 8, 16, 32, "mix"]
KINDS = ["min", "max", "checker1", "checker4", "binary", "noise"]


@pytest.fixture(scope="module")
def ctxs():
    c = {B: capi.Context(bit_depth=B) for B in (8, 10, 12)}
    yield c
    for v in c.values():
        v.close()


def _checker(w, h, B, cell, phase):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // cell) + (xx // cell) + phase) & 1) * ((1 << B) - 1)).astype(np.int16)


def _planes(kind, B):
    shapes = [(W, H), (W // 2, H // 2), (W // 2, H // 2)]
    if kind in ("min", "max"):
        hi, lo = xi.opposite_ends(W, H, B)
        return hi if kind == "max" else lo
    if kind.startswith("checker"):
        return [_checker(w, h, B, int(kind[7:]), p) for p, (w, h) in enumerate(shapes)]
    if kind == "binary":
        rng = np.random.default_rng(9100 + B)
        return [xi.extreme_plane(rng, w, h, B, "binary") for w, h in shapes]
    return workload.make_planes(9200 + B, W, H, B, "noise")


@functools.lru_cache(maxsize=None)
def _case(tiling, B, kind):
    """(decisions, originals, the oracle's (reconstruction, levels)); computed once, never modified"""
    tus = workload.make_tus(9300 + TILINGS.index(tiling), W, H, tiling, ts_prob=0.25)
    if tiling == 4:
        luma, ts = tus["plane"] == 0, (tus["flags"] & capi.TU_TRANSFORM_SKIP) != 0
        assert (tus["log2n"] == 2).all() and (luma & ~ts).any() and (~luma & ~ts).any() and (luma & ts).any() and (~luma & ts).any()
    org = _planes(kind, B)
    return tus, org, ol.o_intra_frame_encode(tus, W, H, B, QP, org)


def _call(ctx, plan, org, want, decode):
    L = capi.lib()
    d_org, d_rec = capi.DevPicture(ctx, W, H).upload(org), capi.DevPicture(ctx, W, H).zero()
    d_lev = capi.DevPicture(ctx, W, H, dtype=np.int32)
    d_lev.upload(want[1]) if decode else d_lev.zero()
    parr = (C.c_void_p * 1)(plan.value)
    try:
        if decode:
            ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, parr, 1, C.byref(d_rec.as_pic()), C.byref(d_lev.as_pic())))
        else:
            ctx._chk(L.hmx_frame_intra_encode_multi(ctx.h, parr, 1, C.byref(d_org.as_pic()), C.byref(d_rec.as_pic()), C.byref(d_lev.as_pic())))
        ctx.sync()
        sched = C.c_int()
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3, sched.value  # the packed schedule
        return d_rec.download(), d_lev.download()
    finally:
        for d in (d_org, d_rec, d_lev):
            d.free()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("tiling", TILINGS)
def test_packed_picture_vs_oracle(ctxs, hmx_opts, tiling, B, kind):
    ctx, L = ctxs[B], capi.lib()
    tus, org, want = _case(tiling, B, kind)
    pp = capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1)
    plans = ctx.intra_plans([tus], pp, None)
    try:
        for slots8 in ("16", "8"):
            hmx_opts(ctx, HMX_INTRA_SCHEDULE="p", HMX_PACK_SLOTS4="64", HMX_PACK_SLOTS8=slots8)
            for decode in (False, True):
                rec, lev = _call(ctx, plans[0], org, want, decode)
                for p in range(3):
                    assert np.array_equal(lev[p], want[1][p]), ("levels", slots8, decode, p)
                    assert np.array_equal(rec[p], want[0][p]), ("reconstruction", slots8, decode, p)
    finally:
        L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * 1)(plans[0].value), 1)


@pytest.mark.parametrize("B", [8, 10, 12])
def test_block_lists_16_and_32(ctxs, B):
    """the list kernels' forward and inverse passes at 16 and 32 on residuals of +-(2^B - 1) (a checkerboard original on the opposite
    checkerboard as the prediction) and of noise"""
    ctx, L, O = ctxs[B], capi.lib(), ol.oracle()
    mx = (1 << B) - 1
    pp = capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1)
    for tiling in (16, 32):
        tus = workload.make_tus(9400 + tiling, W, H, tiling, ts_prob=0.0)
        assert ((1 << tus["log2n"][tus["plane"] == 0]) == tiling).all()
        for kind in ("checker1", "noise"):
            org = _planes(kind, B)
            pred = [(mx - o).astype(np.int16) for o in org] if kind == "checker1" else _planes("binary", B)
            lst = ctx.tu_list(tus)
            d_org, d_pred = capi.DevPicture(ctx, W, H).upload(org), capi.DevPicture(ctx, W, H).upload(pred)
            d_lev, d_rec = capi.DevPicture(ctx, W, H, dtype=np.int32).zero(), capi.DevPicture(ctx, W, H).zero()
            try:
                ctx._chk(L.hmx_batch_residual_transform_recon_multi(ctx.h, lst, 1, C.byref(d_org.as_pic()), C.byref(d_pred.as_pic()),
                                                                    C.byref(d_lev.as_pic()), C.byref(d_rec.as_pic()), None, C.byref(pp)))
                ctx.sync()
                lev, rec = d_lev.download(), d_rec.download()
            finally:
                L.hmx_tu_list_destroy(ctx.h, lst)
                for d in (d_org, d_pred, d_lev, d_rec):
                    d.free()
            for i, t in enumerate(tus):
                N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
                q = O.hmo_setQPforQuant(QP, int(p != 0), 6 * (B - 8), 0)
                cfg = ol.quant_cfg(q.per, q.rem, intra_slice=1, sign_hide=1, scan_idx=O.hmo_coef_scan_idx(N, int(p == 0), 1, int(t["mode"])))
                tmode = int(t["mode"]) if p == 0 else capi.REG_DCT
                resi = (org[p][y:y + N, x:x + N].astype(np.int32) - pred[p][y:y + N, x:x + N]).astype(np.int16)
                ref, _ = ol.o_transformNxN(np.ascontiguousarray(resi), N, B, tmode, 0, cfg)
                assert np.array_equal(lev[p][y:y + N, x:x + N], ref), ("levels", tiling, kind, i)
                r = ol.o_invtransformNxN(ref, N, B, tmode, q.per, q.rem, 0)
                want = np.clip(pred[p][y:y + N, x:x + N].astype(np.int32) + r, 0, mx)
                assert np.array_equal(rec[p][y:y + N, x:x + N], want), ("reconstruction", tiling, kind, i)
