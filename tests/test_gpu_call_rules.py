"""The host rules of a whole-picture call as the library applies them (thevc_amd/csrc/hmx_call_rules.h through issue_packed and
hmx_tpool_create), at the picture counts on both sides of every threshold: after each packed encode call the geometry of the call's
tables (hmx_last_call_pack_tables) is the one tests/call_rules_model.py -- the restatement tests/test_call_rules.py holds the header
against on the CPU -- gives for that batch size, and the first and the last picture of the batch are the oracle's, bit for bit.

One 64x64 8-bit picture (one CTU whose `mix` tiling holds all four size classes), one shared plan, resident pools and one slab of
levels per call, the pictures alternating between two sources; with hmx_set_rdoq (one table set) 511 and 512 pictures fall on the
two sides of RDOQ's group rule.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import call_rules_model as M
import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

W = H = 64
B, QP = 8, 30
N_PICS = (1, 159, 160, 319, 320, 511, 512, 639, 640, 1535, 1536)


@pytest.fixture(scope="module")
def setup():
    """The context, the plan, two staged sources and their oracle results: shared by every case, not modified."""
    tus = workload.with_cbf_ctx(workload.make_tus(3, W, H, "mix"))
    sz = np.bincount(tus["log2n"], minlength=6)[2:6]
    assert (sz > 0).all() and set(tus["log2n"][tus["plane"] == 0]) == {2, 3, 4, 5}
    ctx = capi.Context(bit_depth=B)
    L = capi.lib()
    plan = ctx.intra_plan(tus, capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1))
    src = [workload.make_planes(4100 + j, W, H, B, "texture" if j else "noise") for j in range(2)]
    stage = [capi.DevPicture(ctx, W, H).upload(s) for s in src]
    out = capi.DevPicture(ctx, W, H)
    ests = [workload.make_est_bits(4200 + k) for k in range(8)]
    lams = workload.rdoq_lambdas(QP)
    want = {False: [ol.o_intra_frame_encode(tus, W, H, B, QP, s, 1) for s in src],
            True: [ol.o_intra_frame_encode_rdoq(tus, W, H, B, QP, s, ests, lams, 1) for s in src]}
    assert any(not np.array_equal(a, b) for j in range(2) for a, b in zip(want[False][j][1], want[True][j][1]))  # RDOQ decides something
    yield dict(ctx=ctx, L=L, plan=plan, tus=tus, sz=[int(v) for v in sz], stage=stage, out=out, ests=ests, lams=lams, want=want)
    ctx.set_rdoq(None)
    L.hmx_intra_plan_destroy(ctx.h, plan)
    for d in stage + [out]:
        d.free()
    ctx.close()


def encode_and_check(s, n, rdoq):
    ctx, L, tus = s["ctx"], s["L"], s["tus"]
    # the pools take their group size when they are created: RDOQ is set first
    ctx.set_rdoq([(s["ests"], s["lams"][0], s["lams"][1])] if rdoq else None)
    p_org, p_rec = capi.ResidentPool(ctx, W, H, n), capi.ResidentPool(ctx, W, H, n)
    lev = capi.DevLevelsZSlab(ctx, W, H, n).zero()
    try:
        pics = (capi.Pic * n)(*[s["stage"][i % 2].as_pic() for i in range(n)])
        ctx._chk(L.hmx_tpool_import(ctx.h, p_org.h_, 0, n, pics))
        lev_arr = (capi.Levels * n)(*[lev.as_pic(i) for i in range(n)])
        parr = (C.c_void_p * 1)(s["plan"].value)
        ctx._chk(L.hmx_frame_intra_encode_resident(ctx.h, parr, 0, n, p_org.h_, p_rec.h_, lev_arr))
        ctx.sync()
        g = capi.PackGeom()
        ctx._chk(L.hmx_last_call_pack_tables(ctx.h, C.byref(g), None, None, None, None, None))
        I = M.pack_group(0, rdoq, n)
        m = M.pack_shape(n, I, 0, 0, rdoq, False, g.max_levels, [v * n for v in s["sz"]], len(tus) * n)
        print(f"n_pics {n} rdoq {int(rdoq)}: I {g.I} groups {g.n_groups} shards {g.n_shards} slots4 {g.slots4} slots8 {g.slots8} "
              f"rows {g.n_rows} waves {g.n_waves} (bound {m['waves_bound']}) items {g.n_items}")
        assert (g.n_pics, g.I, g.n_groups, g.n_shards, g.slots4, g.slots8) == (n, I, m["n_groups"], m["n_shards"], m["slots4"], m["slots8"])
        assert g.n_rows == m["n_rows"] and g.n_items == len(tus) * n and 0 < g.n_waves <= m["waves_bound"] and not m["too_large"]
        for i in sorted({0, n - 1}):
            rr, lr = s["want"][rdoq][i % 2]
            p_rec.export_planes(i, [s["out"]])
            rec, got_lev = s["out"].download(), lev.picture(i).to_planes(tus)
            for p in range(3):
                assert np.array_equal(got_lev[p], lr[p]), ("levels", n, i, p)
                assert np.array_equal(rec[p], rr[p]), ("reconstruction", n, i, p)
        return g
    finally:
        p_org.free()
        p_rec.free()
        lev.free()


@pytest.mark.parametrize("n", N_PICS)
def test_geometry_and_pictures_at_the_thresholds(setup, n):
    g = encode_and_check(setup, n, False)
    # the rules spelled out: groups of 2 from 512 and 4 from 1536 pictures, 16 4x4 blocks per wave-item from 160 to 319, sixteen 8x8 from 640
    assert g.I == (4 if n >= 1536 else 2 if n >= 512 else 1)
    assert g.slots4 == (16 if 160 <= n < 320 else 64) and g.slots8 == (16 if n >= 640 else 8)


@pytest.mark.parametrize("n,group", [(511, 1), (512, M.RDOQ_MAX_GROUP)])
def test_rdoq_group_at_its_threshold(setup, n, group):
    g = encode_and_check(setup, n, True)
    assert (g.I, g.slots4, g.slots8) == (group, 64, 8)
