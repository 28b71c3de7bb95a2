"""The packed chain issues the global loads of a wave-item in batches: the original rows before the dependency poll (raw, unpacked
where the residual is formed), and the units of a reference gather back to back, a unit outside the mask or past the line, and
every unit of a lane without a block, reading one stand-in address.  None of that may change a sample.  A gather load that moved
above the poll reads a neighbour before it is written; a stand-in value that leaks into a position a mode reads changes a
prediction; both show as a difference from the CPU oracle.

70 pictures of 200x136 at 10 bit with 70 distinct decision structures, resident in the working layout, packing groups of 64: one
full group and one of 6 pictures, whose wave-items have lanes without a block.  The pictures cut the last CTU column and row (8
samples of each), so picture edges and CTU corners give every shape of availability mask.  Uniform tilings 4, 8, 16, 32 and the
mix, in the slot counts of the default bench (64 4x4 blocks, sixteen 8x8 blocks per wave-item); once at 416x240, 8 bit, mix.
Levels and reconstruction of EVERY picture against oracle_lib.o_intra_frame_encode, encoder and decoder direction, exactly; and
the same encode call a second time into other buffers gives the same bytes.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

F, N_SRC, QP = 70, 5, 32


def _run(w, h, B, tiling, seed):
    ctx = capi.Context(bit_depth=B)
    L = capi.lib()
    try:
        ctx.set_option("HMX_PACK_GROUP", 64)
        ctx.set_option("HMX_PACK_SLOTS4", 64)
        ctx.set_option("HMX_PACK_SLOTS8", 16)
        pp = capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1)
        tus = [workload.make_tus(seed + i, w, h, tiling) for i in range(F)]
        assert len({t.tobytes() for t in tus}) == F  # 70 distinct plans
        plans = ctx.intra_plans(tus, pp)
        src = [workload.make_planes(seed + 500 + j, w, h, B, "texture" if j % 2 == 0 else "noise") for j in range(N_SRC)]
        p_org, p_rec, p_rec2, p_dec = (capi.ResidentPool(ctx, w, h, F) for _ in range(4))
        stage = [capi.DevPicture(ctx, w, h) for _ in range(N_SRC)]
        for k, d in enumerate(stage):
            d.upload(src[k])
        for i0 in range(0, F, N_SRC):  # picture i holds source i mod N_SRC
            p_org.import_planes(i0, stage[:min(N_SRC, F - i0)])
        lev, lev2 = capi.DevLevelsZSlab(ctx, w, h, F).zero(), capi.DevLevelsZSlab(ctx, w, h, F).zero()
        arr = lambda lv: (capi.Levels * F)(*[lv.as_pic(i) for i in range(F)])
        parr = (C.c_void_p * F)(*[p.value for p in plans])
        sched = C.c_int()
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, 1, F, p_org.h_, p_rec.h_, arr(lev)))
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3, sched.value  # the packed schedule
        ctx._chk(L.hmx_frame_intra_decode_resident(ctx.h, parr, 1, F, p_dec.h_, arr(lev)))
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3, sched.value
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, 1, F, p_org.h_, p_rec2.h_, arr(lev2)))
        ctx.sync()
        for i in range(F):
            rr, lr = ol.o_intra_frame_encode(tus[i], w, h, B, QP, src[i % N_SRC])
            got = []
            for pool in (p_rec, p_dec, p_rec2):
                pool.export_planes(i, stage[:1])
                got.append(stage[0].download())
            got_lev, got_lev2 = lev.picture(i).to_planes(tus[i]), lev2.picture(i).to_planes(tus[i])
            for p in range(3):
                assert np.array_equal(got_lev[p], lr[p]), ("levels", tiling, i, p)
                assert np.array_equal(got[0][p], rr[p]), ("reconstruction", tiling, i, p)
                assert np.array_equal(got[1][p], rr[p]), ("decoder direction", tiling, i, p)
                assert got[2][p].tobytes() == got[0][p].tobytes(), ("second call, reconstruction", tiling, i, p)
                assert got_lev2[p].tobytes() == got_lev[p].tobytes(), ("second call, levels", tiling, i, p)
        for x in (p_org, p_rec, p_rec2, p_dec, lev, lev2, *stage):
            x.free()
        L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * F)(*[p.value for p in plans]), F)
    finally:
        ctx.close()


@pytest.mark.parametrize("tiling", ["mix", 4, 8, 16, 32])
def test_70_pictures_200x136_10bit(tiling):
    _run(200, 136, 10, tiling, 4100 + 100 * ["mix", 4, 8, 16, 32].index(tiling))


def test_70_pictures_416x240_8bit_mix():
    _run(416, 240, 8, "mix", 5100)
