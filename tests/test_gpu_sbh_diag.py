"""Uniform 16x16 and 32x32 tilings through the resident packed path, held against the CPU oracle: the two shapes whose
quantiser decides sign-bit hiding in the lane that holds the coefficient group (quant_sbh_diag in
thevc_amd/csrc/hmx_kernels.h).  8- and 10-bit, QP 22/32/37, sign hiding on and off; levels, reconstruction and the
decoder direction of every picture.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tiling", ["16", "32"])
@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("qp", [22, 32, 37])
@pytest.mark.parametrize("sign_hide", [1, 0])
def test_uniform_tiling_vs_oracle(tiling, B, qp, sign_hide):
    w, h, F, n_src = 640, 384, 6, 3
    ctx = capi.Context(bit_depth=B)
    try:
        L = capi.lib()
        pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, sign_hide)
        tus = workload.make_tus(700 + int(tiling) + B, w, h, tiling)
        assert (tus["log2n"][tus["plane"] == 0] == (4 if tiling == "16" else 5)).all()  # chroma: 8x8, or 16x16 under 32x32
        plan = ctx.intra_plan(tus, pp)
        # one smooth source (long runs of small levels: the "first and last non-zero" corners) and two of noise (dense groups)
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
