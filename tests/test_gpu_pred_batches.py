"""Intra prediction reads its LDS operands in batches: the extended main reference is built from sources read together and
written under a predicate, the general angular path reads both taps of all its samples back to back and always interpolates (a
weight of zero where the reference takes the sample itself -- with one read the reference does not make, one word past the main
reference).  That is the form of the 8x8, 16x16 and 32x32 chains of the packed schedule's plain encoder and decoder kernels,
which is what this test runs; the 4x4 lane chain and the distortion and RDOQ variants keep the plain forms.  None of that may
change a sample.  A stale LDS word that leaked into a sample differs between two calls or from the CPU oracle.

70 pictures of 200x136 with 70 distinct decision structures, resident in the working layout, packing groups of 64 (one full group
and one of 6 pictures, whose wave-items have lanes without a block) in the slot counts of the default bench (64 4x4 blocks,
sixteen 8x8 blocks per wave-item): every wave mixes planar, DC, pure-angle and general blocks.  The pictures cut the last CTU
column and row, which gives every availability shape.  Sources alternate "texture" and "noise"; noise puts samples at 0 and at the
maximum into the references.  Uniform tilings 4, 8, 16, 32 and the mix, at 8 and at 10 bit.

Uniform-mode cases: all pictures follow ONE plan whose luma modes are all set to one value, so the mode branches of luma waves
are wave-uniform and a path runs with every lane active.  Modes 2 and 34 are the two ends with di = N, df = 0 (the extra read),
18 has the longest projected side reference, 26 and 10 run the edge filter, 0 and 1 planar and DC.

Levels and reconstruction of EVERY picture against oracle_lib.o_intra_frame_encode, encoder and decoder direction, exactly; and
the same encode call a second time into other buffers gives the same bytes.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

F, N_SRC, QP, W, H = 70, 5, 32, 200, 136
TILINGS = ["mix", 4, 8, 16, 32]
UNIFORM_MODES = [0, 1, 2, 10, 18, 26, 34]


def sources(seed, B):
    return [workload.make_planes(seed + 500 + j, W, H, B, "texture" if j % 2 == 0 else "noise") for j in range(N_SRC)]


def distinct_tus(seed, tiling):
    tus = [workload.make_tus(seed + i, W, H, tiling) for i in range(F)]
    assert len({t.tobytes() for t in tus}) == F  # 70 distinct plans
    return tus


def uniform_mode_tus(seed, mode):
    tus = workload.make_tus(seed, W, H, "mix")
    tus["mode"][tus["plane"] == 0] = mode
    return tus


def _run(B, tus, src):
    """tus: one TU list per picture, or ONE list that every picture follows"""
    shared = not isinstance(tus, list)
    ctx = capi.Context(bit_depth=B)
    L = capi.lib()
    try:
        ctx.set_option("HMX_PACK_GROUP", 64)
        ctx.set_option("HMX_PACK_SLOTS4", 64)
        ctx.set_option("HMX_PACK_SLOTS8", 16)
        pp = capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1)
        plans = ctx.intra_plans([tus] if shared else tus, pp)
        tu_of = (lambda i: tus) if shared else (lambda i: tus[i])
        p_org, p_rec, p_rec2, p_dec = (capi.ResidentPool(ctx, W, H, F) for _ in range(4))
        stage = [capi.DevPicture(ctx, W, H) for _ in range(N_SRC)]
        for k, d in enumerate(stage):
            d.upload(src[k])
        for i0 in range(0, F, N_SRC):  # picture i holds source i mod N_SRC
            p_org.import_planes(i0, stage[:min(N_SRC, F - i0)])
        lev, lev2 = capi.DevLevelsZSlab(ctx, W, H, F).zero(), capi.DevLevelsZSlab(ctx, W, H, F).zero()
        arr = lambda lv: (capi.Levels * F)(*[lv.as_pic(i) for i in range(F)])
        parr = (C.c_void_p * len(plans))(*[p.value for p in plans])
        stride = 0 if shared else 1
        sched = C.c_int()
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, stride, F, p_org.h_, p_rec.h_, arr(lev)))
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3, sched.value  # the packed schedule
        ctx._chk(L.hmx_frame_intra_decode_resident(ctx.h, parr, stride, F, p_dec.h_, arr(lev)))
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3, sched.value
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, stride, F, p_org.h_, p_rec2.h_, arr(lev2)))
        ctx.sync()
        want = {}  # the oracle once per (decision structure, source)
        for i in range(F):
            key = (0 if shared else i, i % N_SRC)
            if key not in want:
                want[key] = ol.o_intra_frame_encode(tu_of(i), W, H, B, QP, src[i % N_SRC])
                assert all(np.any(l) for l in want[key][1]), ("the oracle's levels are all zero in a plane", key)
            rr, lr = want[key]
            got = []
            for pool in (p_rec, p_dec, p_rec2):
                pool.export_planes(i, stage[:1])
                got.append(stage[0].download())
            got_lev, got_lev2 = lev.picture(i).to_planes(tu_of(i)), lev2.picture(i).to_planes(tu_of(i))
            for p in range(3):
                assert np.array_equal(got_lev[p], lr[p]), ("levels", i, p)
                assert np.array_equal(got[0][p], rr[p]), ("reconstruction", i, p)
                assert np.array_equal(got[1][p], rr[p]), ("decoder direction", i, p)
                assert got[2][p].tobytes() == got[0][p].tobytes(), ("second call, reconstruction", i, p)
                assert got_lev2[p].tobytes() == got_lev[p].tobytes(), ("second call, levels", i, p)
        for x in (p_org, p_rec, p_rec2, p_dec, lev, lev2, *stage):
            x.free()
        L.hmx_intra_plan_destroy_many(ctx.h, parr, len(plans))
    finally:
        ctx.close()


@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("tiling", TILINGS)
def test_70_pictures_every_mode(tiling, B):
    seed = 6100 + 100 * TILINGS.index(tiling) + 1000 * (B == 8)
    _run(B, distinct_tus(seed, tiling), sources(seed, B))


@pytest.mark.parametrize("mode", UNIFORM_MODES)
def test_one_plan_one_luma_mode(mode):
    seed = 8100 + mode
    _run(10, uniform_mode_tus(seed, mode), sources(seed, 10))
