"""Uniform 4x4 and 8x8 tilings through the resident packed path in the shapes of the default bench (64 lanes of 4x4 blocks per
wave, lane4_forward; 8x8 blocks on four lanes, the in-register path of wave_chain_8x2), held against the CPU oracle: both call
the shared sign-bit hiding decision of thevc_amd/csrc/hmx_sbh.h on words they reorder into the block's scan.  Random intra modes
cover the three 4x4 / 8x8 scans, and 4x4 blocks include transform skip.  8- and 10-bit, QP 4 (large levels) / 22 / 32 / 37,
sign hiding on and off; levels, reconstruction and the decoder direction of every picture.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tiling", ["4", "8"])
@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("qp", [4, 22, 32, 37])
@pytest.mark.parametrize("sign_hide", [1, 0])
def test_uniform_tiling_vs_oracle(tiling, B, qp, sign_hide):
    w, h, F, n_src = 640, 384, 6, 3
    ctx = capi.Context(bit_depth=B)
    try:
        L = capi.lib()
        # the slot counts of the default bench: small batches would otherwise take eight 8x8 slots per wave
        ctx.set_option("HMX_PACK_SLOTS4", 64)
        ctx.set_option("HMX_PACK_SLOTS8", 16)
        pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, sign_hide)
        tus = workload.make_tus(800 + int(tiling) + B + qp, w, h, tiling, ts_prob=0.3)
        assert (tus["log2n"][tus["plane"] == 0] == (2 if tiling == "4" else 3)).all()  # chroma: 4x4 (under 8x8 luma as well)
        assert (tus["flags"] & workload.TU_TRANSFORM_SKIP).any() and len(set(tus["mode"][tus["plane"] == 0])) > 20
        plan = ctx.intra_plan(tus, pp)
        # one smooth source (long runs of small levels: first and last non-zero 3 or 4 apart) and two of noise (dense groups)
        src = [workload.make_planes(900 + j, w, h, B, "texture" if j == 0 else "noise") for j in range(n_src)]
        p_org, p_rec, p_dec = (capi.ResidentPool(ctx, w, h, F) for _ in range(3))
        stage = [capi.DevPicture(ctx, w, h) for _ in range(n_src)]
        for k, d in enumerate(stage):
            d.upload(src[k])
        for i0 in range(0, F, n_src):
            p_org.import_planes(i0, stage[:min(n_src, F - i0)])
        lev = capi.DevLevelsZSlab(ctx, w, h, F).zero()
        lev_arr = (capi.Levels * F)(*[lev.as_pic(i) for i in range(F)])
        parr = (C.c_void_p * F)(*[plan.value] * F)
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, 1, F, p_org.h_, p_rec.h_, lev_arr))
        ctx._chk(L.hmx_frame_intra_decode_resident(ctx.h, parr, 1, F, p_dec.h_, lev_arr))
        ctx.sync()
        want = [ol.o_intra_frame_encode(tus, w, h, B, qp, src[j], sign_hide) for j in range(n_src)]
        for i in range(F):
            rr, lr = want[i % n_src]
            p_rec.export_planes(i, stage[:1])
            rec = stage[0].download()
            p_dec.export_planes(i, stage[:1])
            dec = stage[0].download()
            got_lev = lev.picture(i).to_planes(tus)
            for p in range(3):
                assert np.array_equal(got_lev[p], lr[p]), ("levels", i, p)
                assert np.array_equal(rec[p], rr[p]), ("reconstruction", i, p)
                assert np.array_equal(dec[p], rr[p]), ("decoder direction", i, p)
        for x in (p_org, p_rec, p_dec):
            x.free()
        lev.free()
        for d in stage:
            d.free()
        L.hmx_intra_plan_destroy(ctx.h, plan)
    finally:
        ctx.close()
