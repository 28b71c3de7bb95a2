"""GPU vs oracle, bit for bit, at the 16-bit edges of the quantisers and the inverse transform (tests/extreme_inputs.py):
QP_Y at per 0 and 1 on saturating pictures (flat level clip, uiAcSum of the unclipped magnitudes, sign hiding on a clipped
level, RDOQ's Int levels), and the decoder direction on synthetic levels (levels outside int16, the 12-bit de-quantiser wrap,
the clip after the first inverse stage).  The oracle is pinned to the reference at the same edges by
tests/test_oracle_vs_ref_edges.py.  Every case asserts that it reached its edge.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import extreme_inputs as xi
import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu
REG_DCT = 65535
HMX_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(B):
        if B not in made:
            made[B] = capi.Context(bit_depth=B)
        return made[B]

    yield get
    for c in made.values():
        c.close()


def _at_clip(planes):
    """Levels sitting at the flat quantiser's clip bound."""
    return sum(int(np.count_nonzero((p == xi.INT16_MAX) | (p == xi.INT16_MIN))) for p in planes)


def _synthetic_planes(rng, tus, w, h, kinds=xi.LEVEL_KINDS):
    lev = [np.zeros((h, w), np.int32), np.zeros((h // 2, w // 2), np.int32), np.zeros((h // 2, w // 2), np.int32)]
    for t in tus:
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        lev[p][y:y + N, x:x + N] = xi.synthetic_levels(rng, N, kinds[int(rng.integers(0, len(kinds)))])
    return lev


def _decode_counters(tus, lev, B, qp, cqo=0):
    """(de-quantiser wraps, first-stage clips) over the blocks of a level picture, from the oracle's xDeQuant."""
    O = ol.oracle()
    bd = xi.qp_bd_offset(B)
    wraps = first = 0
    for t in tus:
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        q = O.hmo_setQPforQuant(qp, int(p != 0), bd, cqo if p else 0)
        blk = np.ascontiguousarray(lev[p][y:y + N, x:x + N], np.int32).reshape(-1)
        wraps += xi.count_dequant_wrap(blk, N, B, q.per, q.rem)
        if not (int(t["flags"]) & capi.TU_TRANSFORM_SKIP):
            d = np.zeros(N * N, np.int32)
            O.hmo_xDeQuant(blk, d, N, B, q.per, q.rem)
            first += xi.count_first_stage_clip(d, N, dst=(N == 4 and p == 0))
    return wraps, first


def _oracle_decode(tus, w, h, B, qp, lev, cqo=0):
    cfg = ol.frame_cfg(w, h, B, qp, 1, cqo)
    rec = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
    P3, I3 = C.c_void_p * 3, C.c_int * 3
    st = I3(w, w // 2, w // 2)
    t = np.ascontiguousarray(tus, ol.TU_DTYPE)
    lv = [np.ascontiguousarray(p, np.int32) for p in lev]
    ol.oracle().hmo_intra_frame_decode(C.byref(cfg), t.ctypes.data, len(t), P3(*[p.ctypes.data for p in rec]), st,
                                       P3(*[p.ctypes.data for p in lv]))
    return rec


# ---- a. the encoder chain at per 0 and 1 ---------------------------------------------------------------------------------------

CHAIN_CASES = [  # (B, QP_Y, sign hiding, tiling, knobs | "sse")
    (10, -12, 1, "mix", {}),
    (10, -9, 0, 32, {}),
    (10, -12, 1, 32, {"HMX_INTRA_SCHEDULE": "level"}),
    (12, -24, 1, 8, {"HMX_PACK_SLOTS8": "16"}),
    (12, -24, 0, 8, {"HMX_PACK_SLOTS8": "8"}),
    (12, -21, 1, 16, {"HMX_INTRA_SCHEDULE": "wave"}),
    (12, -15, 1, "mix", {"HMX_PACK_SLOTS4": "16"}),
    (12, -24, 1, "mix", {"HMX_PACK_SLOTS4": "64"}),
    (12, -21, 0, "mix", {"HMX_INTRA_SCHEDULE": "level"}),
    (12, -24, 1, "mix", "sse"),
]


@pytest.mark.parametrize("B,qp,sbh,tiling,knobs", CHAIN_CASES)
def test_chain_at_lowest_qp(ctxs, B, qp, sbh, tiling, knobs, hmx_opts):
    """hmx_frame_intra_encode on saturating pictures at per 0 / 1: levels, reconstruction (and the per-block SSE of its own
    kernel instantiation) vs the oracle; then hmx_frame_intra_decode from those levels reproduces the reconstruction."""
    ctx, L, O = ctxs(B), capi.lib(), ol.oracle()
    if isinstance(knobs, dict):
        hmx_opts(ctx, **knobs)
    w, h, n = 128, 128, 2
    tus = workload.make_tus(40 + B, w, h, tiling)
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, sbh)
    plan = ctx.intra_plan(tus, pp)
    rng = np.random.default_rng(900 + B - qp)
    scale = tiling if tiling != "mix" else (32 if B == 10 else 16)  # at 10 bit only 32x32 blocks clip
    orgs = [xi.saturating_picture(rng, w, h, B, scale=scale) for _ in range(n)]
    d_org = [capi.DevPicture(ctx, w, h).upload(o) for o in orgs]
    d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
    zorder = knobs == "sse"  # this case also keeps its levels in the reference's Z-order layout
    d_lev = [(capi.DevLevelsZ(ctx, w, h) if zorder else capi.DevPicture(ctx, w, h, dtype=np.int32)).zero() for _ in range(n)]
    A = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
    d_sse = []
    if knobs == "sse":
        units = [4 * 256, 4 * 64, 4 * 64]  # 2 x 2 CTUs
        d_sse = [[ctx.alloc(4 * u).zero() for u in units] for _ in range(n)]
        sse_arr = (capi.Sse * n)()
        for i in range(n):
            for p in range(3):
                sse_arr[i].plane[p] = d_sse[i][p].ptr
        ctx._chk(L.hmx_set_sse_output(ctx.h, sse_arr, n))
    try:
        ctx._chk(L.hmx_frame_intra_encode(ctx.h, plan, n, A(d_org, capi.Pic), A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        ctx.sync()
    finally:
        if d_sse:
            ctx._chk(L.hmx_set_sse_output(ctx.h, None, 0))
    n_clip = n_sbh_changed = 0
    for i in range(n):
        rr, lr = ol.o_intra_frame_encode(tus, w, h, B, qp, orgs[i], sign_hide=sbh)
        rec, lev = d_rec[i].download(), (d_lev[i].to_planes(tus) if zorder else d_lev[i].download())
        for p in range(3):
            assert np.array_equal(lev[p], lr[p]), ("levels", i, p)
            assert np.array_equal(rec[p], rr[p]), ("recon", i, p)
        n_clip += _at_clip(lr)
        if sbh:
            _, l0 = ol.o_intra_frame_encode(tus, w, h, B, qp, orgs[i], sign_hide=0)
            n_sbh_changed += sum(int(not np.array_equal(a, b)) for a, b in zip(lr, l0))
        if d_sse:
            O.hmo_getSSE.restype = C.c_uint32
            got = [d_sse[i][p].download(np.uint32) for p in range(3)]
            for t in tus:
                N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
                o = np.ascontiguousarray(orgs[i][p][y:y + N, x:x + N])
                r = np.ascontiguousarray(rr[p][y:y + N, x:x + N])
                want = O.hmo_getSSE(o.ctypes.data_as(C.c_void_p), N, r.ctypes.data_as(C.c_void_p), N, N, N, B)
                assert int(got[p][d_lev[i].block_offset(p, x, y) // 16]) == want, ("sse", i, p, x, y, N)
    assert n_clip > 0, "no level at the clip bound"
    if sbh:
        assert n_sbh_changed > 0
    # decoder direction from the levels just produced
    d_rec2 = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
    ctx._chk(L.hmx_frame_intra_decode(ctx.h, plan, n, A(d_rec2, capi.Pic), A(d_lev, capi.Levels)))
    ctx.sync()
    for i in range(n):
        a, b = d_rec2[i].download(), d_rec[i].download()
        assert all(np.array_equal(a[p], b[p]) for p in range(3)), ("decode", i)
    L.hmx_intra_plan_destroy(ctx.h, plan)
    for d in d_org + d_rec + d_rec2 + d_lev + [b for row in d_sse for b in row]:
        d.free()


# ---- b. the decoder direction on synthetic levels ------------------------------------------------------------------------------

DECODE_CASES = [  # (B, QP_Y, chroma QP offset): every remainder at per 0, the 12-bit wrap QPs, 51 with chroma offsets
    (8, 0, 0), (8, 3, 0), (8, 51, -12),
    (10, -12, 0), (10, -10, 0), (10, -7, 0), (10, 51, 12),
    (12, -24, 0), (12, -23, 0), (12, -20, 0), (12, 41, 0), (12, 46, -5), (12, 51, 12),
]


@pytest.mark.parametrize("B,qp,cqo", DECODE_CASES)
def test_decode_synthetic_levels(ctxs, B, qp, cqo):
    """hmx_frame_intra_decode (plane and Z-order levels), _multi, _onto and _resident on levels of every synthetic kind
    (all four block sizes, 4x4 DST and transform skip) vs the oracle's decoder."""
    ctx, L = ctxs(B), capi.lib()
    w, h, n = 128, 64, 2
    tus = [workload.make_tus(60 + i + B, w, h, "mix", ts_prob=0.3) for i in range(n)]
    pp = capi.PicParam(w, h, qp, cqo, capi.I_SLICE, 1)
    plans = [ctx.intra_plan(t, pp) for t in tus]
    rng = np.random.default_rng(3000 + 64 * B + qp)
    levs = [_synthetic_planes(rng, t, w, h) for t in tus]
    want = [_oracle_decode(tus[i], w, h, B, qp, levs[i], cqo) for i in range(n)]
    wraps = first = 0
    for i in range(n):
        a, b = _decode_counters(tus[i], levs[i], B, qp, cqo)
        wraps, first = wraps + a, first + b
    assert first > 0, "no first-stage clip"
    if B == 12 and qp >= 41:
        assert wraps > 0, "no de-quantiser wrap"
    d_lev = [capi.DevPicture(ctx, w, h, dtype=np.int32).upload(lv) for lv in levs]
    d_levz = [capi.DevLevelsZ(ctx, w, h).zero() for _ in range(n)]
    for i in range(n):
        d_levz[i].from_planes(levs[i], tus[i])
    A = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
    parr = (C.c_void_p * n)(*[p.value for p in plans])

    def check(d_rec, what):
        ctx.sync()
        for i in range(n):
            got = d_rec[i].download()
            for p in range(3):
                assert np.array_equal(got[p], want[i][p]), (what, i, p)

    for what, lev in (("plane", d_lev), ("zorder", d_levz)):
        d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
        ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, parr, n, A(d_rec, capi.Pic), A(lev, capi.Levels)))
        check(d_rec, "multi " + what)
        d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
        ctx._chk(L.hmx_frame_intra_decode_onto(ctx.h, plans[0], 1, (capi.Pic * 1)(d_rec[0].as_pic()), (capi.Levels * 1)(lev[0].as_pic())))
        ctx._chk(L.hmx_frame_intra_decode(ctx.h, plans[1], 1, (capi.Pic * 1)(d_rec[1].as_pic()), (capi.Levels * 1)(lev[1].as_pic())))
        check(d_rec, "single/onto " + what)
    # resident pictures
    pool = capi.ResidentPool(ctx, w, h, n)
    d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
    pool.import_planes(0, d_rec)
    ctx._chk(L.hmx_frame_intra_decode_resident(ctx.h, parr, 1, n, pool.h_, A(d_lev, capi.Levels)))
    pool.export_planes(0, d_rec)
    check(d_rec, "resident")
    pool.free()
    for pl in plans:
        L.hmx_intra_plan_destroy(ctx.h, pl)
    for d in d_lev + d_levz:
        d.free()


# ---- c. block lists ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,qp", [(10, -12), (12, -24), (12, -21)])
def test_block_lists_at_edges(ctxs, B, qp):
    """hmx_batch_transformNxN on saturating residuals at per 0 / 1 (levels, d_abs_sum = HM's unclipped uiAcSum), the fused
    hmx_batch_residual_transform_recon_multi, and hmx_batch_invtransformNxN (+ _multi) on synthetic levels with and without a
    prediction; intra, inter and transform-skip blocks."""
    ctx, L, O = ctxs(B), capi.lib(), ol.oracle()
    w, h = 128, 64
    mx = (1 << B) - 1
    rng = np.random.default_rng(4000 + B - qp)
    tus = workload.make_tus(80 + B, w, h, "mix", ts_prob=0.25)
    inter = rng.random(len(tus)) < 0.3
    tus["flags"] = np.where(inter, tus["flags"] | capi.TU_INTER, tus["flags"]).astype(np.uint8)
    lst = ctx.tu_list(tus)
    pp = capi.PicParam(w, h, qp, 0, capi.P_SLICE, 1)
    resi = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
    for t in tus:
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        resi[p][y:y + N, x:x + N] = xi.saturating_residual(rng, N, B, xi.RESIDUAL_KINDS[int(rng.integers(0, 6))])
    pred = [np.where(r > 0, 0, mx).astype(np.int16) for r in resi]
    org = [(pr.astype(np.int32) + r).clip(0, mx).astype(np.int16) for pr, r in zip(pred, resi)]
    d_resi, d_pred, d_org = (capi.DevPicture(ctx, w, h).upload(a) for a in (resi, pred, org))
    d_lev = capi.DevPicture(ctx, w, h, dtype=np.int32).zero()
    d_sum = ctx.alloc(4 * len(tus))
    ctx._chk(L.hmx_batch_transformNxN(ctx.h, lst, C.byref(d_resi.as_pic()), C.byref(d_lev.as_pic()), d_sum.ptr, C.byref(pp)))
    d_lev2, d_rec2 = capi.DevPicture(ctx, w, h, dtype=np.int32).zero(), capi.DevPicture(ctx, w, h).zero()
    ctx._chk(L.hmx_batch_residual_transform_recon_multi(ctx.h, lst, 1, C.byref(d_org.as_pic()), C.byref(d_pred.as_pic()),
                                                        C.byref(d_lev2.as_pic()), C.byref(d_rec2.as_pic()), None, C.byref(pp)))
    ctx.sync()
    lev, lev2, rec2, sums = d_lev.download(), d_lev2.download(), d_rec2.download(), d_sum.download(np.uint32)
    n_clip = 0
    res2 = [(o.astype(np.int32) - pr).astype(np.int16) for o, pr in zip(org, pred)]
    for i, t in enumerate(tus):
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        is_inter, ts = bool(t["flags"] & capi.TU_INTER), int(t["flags"] & capi.TU_TRANSFORM_SKIP)
        q = O.hmo_setQPforQuant(qp, int(p != 0), 6 * (B - 8), 0)
        cfg = ol.quant_cfg(q.per, q.rem, intra_slice=0, sign_hide=1,
                           scan_idx=O.hmo_coef_scan_idx(N, int(p == 0), int(not is_inter), int(t["mode"])))
        tmode = int(t["mode"]) if (p == 0 and not is_inter) else REG_DCT
        ref, s = ol.o_transformNxN(np.ascontiguousarray(resi[p][y:y + N, x:x + N]), N, B, tmode, ts, cfg)
        assert np.array_equal(lev[p][y:y + N, x:x + N], ref), ("levels", i)
        assert int(sums[i]) == s, ("abs_sum", i)
        n_clip += _at_clip([ref])
        ref2, _ = ol.o_transformNxN(np.ascontiguousarray(res2[p][y:y + N, x:x + N]), N, B, tmode, ts, cfg)
        assert np.array_equal(lev2[p][y:y + N, x:x + N], ref2), ("fused levels", i)
        r = ol.o_invtransformNxN(ref2, N, B, tmode, q.per, q.rem, ts)
        want = np.clip(pred[p][y:y + N, x:x + N].astype(np.int32) + r, 0, mx)
        assert np.array_equal(rec2[p][y:y + N, x:x + N], want), ("fused recon", i)
    assert n_clip > 0
    # the inverse direction on synthetic levels, with and without a prediction, one picture and the _multi form
    levs = _synthetic_planes(rng, tus, w, h)
    d_sl = capi.DevPicture(ctx, w, h, dtype=np.int32).upload(levs)
    d_out, d_rc, d_rcm = (capi.DevPicture(ctx, w, h).zero() for _ in range(3))
    ctx._chk(L.hmx_batch_invtransformNxN(ctx.h, lst, C.byref(d_sl.as_pic()), None, C.byref(d_out.as_pic()), C.byref(pp)))
    ctx._chk(L.hmx_batch_invtransformNxN(ctx.h, lst, C.byref(d_sl.as_pic()), C.byref(d_pred.as_pic()), C.byref(d_rc.as_pic()),
                                         C.byref(pp)))
    ctx._chk(L.hmx_batch_invtransformNxN_multi(ctx.h, lst, 1, C.byref(d_sl.as_pic()), C.byref(d_pred.as_pic()),
                                               C.byref(d_rcm.as_pic()), C.byref(pp)))
    ctx.sync()
    out, rc, rcm = d_out.download(), d_rc.download(), d_rcm.download()
    first = 0
    for i, t in enumerate(tus):
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        is_inter, ts = bool(t["flags"] & capi.TU_INTER), int(t["flags"] & capi.TU_TRANSFORM_SKIP)
        q = O.hmo_setQPforQuant(qp, int(p != 0), 6 * (B - 8), 0)
        tmode = int(t["mode"]) if (p == 0 and not is_inter) else REG_DCT
        r = ol.o_invtransformNxN(levs[p][y:y + N, x:x + N], N, B, tmode, q.per, q.rem, ts)
        assert np.array_equal(out[p][y:y + N, x:x + N], r), ("residual", i)
        want = np.clip(pred[p][y:y + N, x:x + N].astype(np.int32) + r, 0, mx)
        assert np.array_equal(rc[p][y:y + N, x:x + N], want), ("recon", i)
        assert np.array_equal(rcm[p][y:y + N, x:x + N], want), ("recon multi", i)
        if not ts:
            d = np.zeros(N * N, np.int32)
            O.hmo_xDeQuant(np.ascontiguousarray(levs[p][y:y + N, x:x + N], np.int32).reshape(-1), d, N, B, q.per, q.rem)
            first += xi.count_first_stage_clip(d, N, dst=(N == 4 and tmode != REG_DCT))
    assert first > 0
    L.hmx_tu_list_destroy(ctx.h, lst)
    for d in (d_resi, d_pred, d_org, d_lev, d_sum, d_lev2, d_rec2, d_sl, d_out, d_rc, d_rcm):
        d.free()


# ---- d. scalar drop-ins --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("N", [4, 8, 16, 32])
def test_scalar_dropins_at_edges(ctxs, B, N):
    """hmx_transformNxN / hmx_xQuant (levels, abs_sum / ac_sum) on saturating residuals at per 0 and 1, including blocks where
    sign hiding lands on a clipped level, and hmx_xDeQuant / hmx_invtransformNxN on synthetic levels at every remainder and the
    wrap QPs."""
    ctx, O = ctxs(B), ol.oracle()
    rng = np.random.default_rng(7000 + 8 * N + B)
    bd = xi.qp_bd_offset(B)
    cases = []
    for it in range(12):
        resi = xi.saturating_residual(rng, N, B, xi.RESIDUAL_KINDS[it % len(xi.RESIDUAL_KINDS)])
        cases.append((resi, -bd + int(rng.integers(0, 12)), int(rng.integers(0, 35)), it % 3))
    cases += [(r, q, m, 0) for r, q, m in (xi.search_sbh_on_clip(rng, N, B, n_want=2) if N > 4 else [])]
    n_clip = n_sbh_clip = 0
    for resi, qpy, mode, ttype_i in cases:
        tt = (capi.TEXT_LUMA, capi.TEXT_CHROMA_U, capi.TEXT_CHROMA_V)[ttype_i if N < 32 else 0]
        qp = capi.qp_for(qpy, tt, B)
        tmode = mode if tt == capi.TEXT_LUMA else REG_DCT
        scan = O.hmo_coef_scan_idx(N, int(tt == capi.TEXT_LUMA), 1, mode)
        per, rem = qp.per, qp.rem
        ts = int(N == 4 and mode % 4 == 0)
        for sbh in (1, 0):
            qparam = capi.QuantParam(qp, -1, capi.I_SLICE, sbh, 1, mode)
            got, gs = ctx.transformNxN(resi, N, N, tt, qparam, ts=ts)
            ref, rs = ol.o_transformNxN(resi, N, B, tmode, ts, ol.quant_cfg(per, rem, 1, sbh, scan))
            assert np.array_equal(got.reshape(N, N), ref) and gs == rs, ("transformNxN", qpy, mode, sbh)
            coef = np.zeros(N * N, np.int32)
            O.hmo_xT(tmode, resi.reshape(-1), N, coef, N, B)
            gq, ga = ctx.xQuant(coef, N, tt, qparam, ac_sum=5)
            rq, ra = np.zeros(N * N, np.int32), C.c_uint32(5)
            O.hmo_xQuant(coef, rq, N, B, C.byref(ol.quant_cfg(per, rem, 1, sbh, scan)), C.byref(ra))
            assert np.array_equal(gq, rq) and ga == ra.value, ("xQuant", qpy, mode, sbh)
            if sbh:
                on = ref
            else:
                n_sbh_clip += xi.count_sbh_on_clipped(on, ref)
        n_clip += xi.count_flat_clip(coef, N, B, per, rem)
    if (B, N) in ((10, 32), (12, 8), (12, 16), (12, 32)):
        assert n_clip > 0 and n_sbh_clip > 0, (n_clip, n_sbh_clip)
    # the inverse direction
    n_wrap = n_first = 0
    qps = [-bd + k for k in range(6)] + ([41, 46, 51] if B == 12 else [51])
    for it, qpy in enumerate(qps * 2):
        kind = xi.LEVEL_KINDS[(it + 1) % len(xi.LEVEL_KINDS)] if it % 2 else ("column", "one_min", "dense")[it % 3]
        lv = xi.synthetic_levels(rng, N, kind).reshape(-1)
        qp = capi.qp_for(qpy, capi.TEXT_LUMA, B)
        d = np.zeros(N * N, np.int32)
        O.hmo_xDeQuant(lv, d, N, B, qp.per, qp.rem)
        assert np.array_equal(ctx.xDeQuant(lv, N, qp), d), ("xDeQuant", qpy, kind)
        n_wrap += xi.count_dequant_wrap(lv, N, B, qp.per, qp.rem)
        for tmode, ts in ((REG_DCT, 0), (int(rng.integers(0, 35)), 0), (REG_DCT, 1)):
            if ts and N != 4:
                continue
            got = ctx.invtransformNxN(lv, N, N, capi.TEXT_LUMA, tmode, qp, ts=ts)
            ref = ol.o_invtransformNxN(lv, N, B, tmode, qp.per, qp.rem, ts)
            assert np.array_equal(got.reshape(N, N), ref), ("invtransformNxN", qpy, kind, tmode, ts)
            if not ts:
                n_first += xi.count_first_stage_clip(d, N, dst=(N == 4 and tmode != REG_DCT))
    assert n_first > 0
    if B == 12:
        assert n_wrap > 0


# ---- e. RDOQ at per 0 ----------------------------------------------------------------------------------------------------------

def _rdoq_or_refused(call, want, what):
    """The library either matches the oracle or refuses with HMX_ERR_ARG (the bound of include/hmx.h); never other levels."""
    try:
        got = call()
    except capi.HmxError as e:
        assert f"error {HMX_ERR_ARG}:" in str(e), (what, str(e))
        return False
    assert np.array_equal(got[0].reshape(want[0].shape), want[0]), (what, np.argwhere(got[0].reshape(want[0].shape) != want[0])[:4])
    assert got[1] == want[1], (what, "abs_sum")
    return True


@pytest.mark.parametrize("B,qps", [(10, (-12, -10, -9)), (12, (-24, -22, -15))])
def test_rdoq_at_lowest_qp(ctxs, B, qps):
    """hmx_xRateDistOptQuant (+ _scaled with flat tables) and hmx_batch_xRateDistOptQuant on coefficients up to +-32768 at per 0
    and 1: the levels are Int as in the reference (above 32767 where the QP allows) -- or the call is refused."""
    ctx, L, O = ctxs(B), capi.lib(), ol.oracle()
    rng = np.random.default_rng(8000 + B)
    bd = xi.qp_bd_offset(B)
    n_wide = 0
    for N in (4, 8, 16, 32):
        for it in range(4):
            qpy = qps[it % len(qps)]
            tt = capi.TEXT_LUMA if (N == 32 or it % 2 == 0) else capi.TEXT_CHROMA_U
            mode = int(rng.integers(0, 35))
            resi = xi.saturating_residual(rng, N, B, ("dc", "dc_neg", "basis", "checker")[it])
            coef = np.zeros(N * N, np.int32)
            O.hmo_xT(mode if tt == capi.TEXT_LUMA else REG_DCT, resi.reshape(-1), N, coef, N, B)
            if it == 3:
                coef[0] = -32768 if coef[0] <= 0 else 32767  # the extremes of a transform coefficient
            qp = capi.qp_for(qpy, tt, B)
            est = ol.make_est_bits(rng)
            lam = float(rng.choice([0.5, 4.0, 30.0]))
            luma = tt == capi.TEXT_LUMA
            scan = O.hmo_coef_scan_idx(N, int(luma), 1, mode)
            cbf_ctx = int(rng.integers(0, 5)) + (0 if luma else 5)
            cfg = ol.RdoqCfg(qp.per, qp.rem, int(luma), 1, scan, 0, cbf_ctx, 1, lam)
            want = ol.o_rdoq(coef, N, B, cfg, est)
            n_wide += int(np.count_nonzero(np.abs(want[0].astype(np.int64)) > xi.INT16_MAX))
            rp = capi.RdoqParam(qp, 1, 1, mode, 0, cbf_ctx, lam)
            e = capi.EstBits.from_buffer_copy(bytes(est))
            _rdoq_or_refused(lambda: ctx.xRateDistOptQuant(coef, N, tt, rp, e), want, ("scalar", N, qpy))
            qtab, estab, _ = ol.scaling_tables(rng, N, B, qp.rem, flat=True)
            want_s = ol.o_rdoq_scaled(coef, N, B, cfg, est, qtab, estab)
            _rdoq_or_refused(lambda: ctx.xRateDistOptQuant_scaled(coef, N, tt, rp, e, qtab, estab), want_s, ("scaled", N, qpy))
    assert n_wide > 0, "no RDOQ level above 16 bits"
    # the block list: saturating coefficients in plane geometry, per 0
    w, h, qpy = 128, 64, qps[0]
    tus = workload.make_tus(90 + B, w, h, "mix")
    n = len(tus)
    ests = [ol.make_est_bits(rng) for _ in range(3)]
    est_arr = (capi.EstBits * 3)(*[capi.EstBits.from_buffer_copy(bytes(e)) for e in ests])
    side = (capi.RdoqSide * n)()
    coef = [np.zeros((h, w), np.int32), np.zeros((h // 2, w // 2), np.int32), np.zeros((h // 2, w // 2), np.int32)]
    for i, t in enumerate(tus):
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        c = np.zeros(N * N, np.int32)
        O.hmo_xT(int(t["mode"]) if p == 0 else REG_DCT, xi.saturating_residual(rng, N, B, ("dc", "dc_neg", "basis")[i % 3]).reshape(-1),
                 N, c, N, B)
        coef[p][y:y + N, x:x + N] = c.reshape(N, N)
        side[i].est_idx, side[i].root_cbf, side[i].cbf_ctx = i % 3, 0, int(rng.integers(0, 5)) + (5 if p else 0)
    lam = (2.5, 1.75)
    d_coef = capi.DevPicture(ctx, w, h, dtype=np.int32).upload(coef)
    d_lev = capi.DevPicture(ctx, w, h, dtype=np.int32).zero()
    d_sum = ctx.alloc(4 * n)
    pp = capi.PicParam(w, h, qpy, 0, capi.I_SLICE, 1)
    t_c = np.ascontiguousarray(tus, capi.TU_DTYPE)
    rc = L.hmx_batch_xRateDistOptQuant(ctx.h, t_c.ctypes.data, side, n, C.byref(d_coef.as_pic()), C.byref(d_lev.as_pic()), d_sum.ptr,
                                       C.byref(pp), est_arr, 3, lam[0], lam[1])
    assert rc in (0, HMX_ERR_ARG), rc
    if rc == 0:
        ctx.sync()
        lev, sums = d_lev.download(), d_sum.download(np.uint32, n)
        n_wide = 0
        for i, t in enumerate(tus):
            N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
            q = O.hmo_setQPforQuant(qpy, int(p != 0), bd, 0)
            cfg = ol.RdoqCfg(q.per, q.rem, int(p == 0), 1, O.hmo_coef_scan_idx(N, int(p == 0), 1, int(t["mode"])), 0, side[i].cbf_ctx, 1,
                             lam[1 if p else 0])
            lo, so = ol.o_rdoq(coef[p][y:y + N, x:x + N], N, B, cfg, ests[i % 3])
            assert np.array_equal(lev[p][y:y + N, x:x + N], lo), ("batch levels", i, N, p)
            assert int(sums[i]) == so, ("batch abs_sum", i)
            n_wide += int(np.count_nonzero(np.abs(lo.astype(np.int64)) > xi.INT16_MAX))
        assert n_wide > 0
    d_coef.free(), d_lev.free(), d_sum.free()
