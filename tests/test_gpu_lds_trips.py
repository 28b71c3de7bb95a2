"""The lane sums on DPP (group_sum) and the batched LDS reads of the packed intra chain (level read-back and store, inverse passes)
cannot change a result: whole-picture parity against the CPU oracle, levels and reconstruction, encoder and decoder direction, in
the shapes the bench runs (packed schedule, 64 4x4 blocks and 16 8x8 blocks per wave-item).

  * pictures of 64x64 and 128x64, uniform tilings 8, 16, 32 and the mix, 1, 3 and 5 pictures per call, 8 and 10 bit: wave-items with
    idle lanes and idle blocks -- a reduction that picks up an idle lane's value shows as a flipped sign-bit-hiding decision
    (uiAbsSum), a wrong DC value or a wrong level;
  * plans whose luma modes are all DC and all planar: the sums of dc_sum_block at every size, the planar products;
  * uiAbsSum at its threshold: originals built block by block from the oracle's own prediction plus one or two changed samples, the
    amplitude raised until the block's uiAbsSum reaches 1 (even blocks: no hiding) or 2 (odd blocks: hiding), so that both kinds sit
    side by side in the wave-items; the set-up checks that the oracle's blocks contain both;
  * one 12-bit case and one with sign_hide = 0;
  * a unit test of the sums themselves through an entry that returns one per block: hmx_batch_predIntra_cost (satd_block: a sum over
    the 4 or 8 lanes of a sub-block, then over the block's 4, 8, 16 or 32 lanes) against the oracle's calcHAD.  The sum over 64 lanes
    is the uiAbsSum of the 32x32 blocks above."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

PICS = [(64, 64), (128, 64)]
TILINGS = [8, 16, 32, "mix"]
COUNTS = [1, 3, 5]
QP = 30


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


def _tus(w, h, tiling, pic, luma_mode=None):
    tus = workload.make_tus(8800 + 10 * pic + w + (TILINGS.index(tiling) if tiling in TILINGS else 7), w, h, tiling)
    if luma_mode is not None:
        tus = tus.copy()
        tus["mode"][tus["plane"] == 0] = luma_mode
    return tus


@functools.lru_cache(maxsize=None)
def _case(w, h, tiling, B, pic, luma_mode=None, sign_hide=1, qp=QP):
    """(decisions, originals, the oracle's (reconstruction, levels)) of picture `pic`; computed once, never modified"""
    tus = _tus(w, h, tiling, pic, luma_mode)
    org = workload.make_planes(8900 + pic, w, h, B, "texture" if pic % 2 else "noise")
    return tus, org, ol.o_intra_frame_encode(tus, w, h, B, qp, org, sign_hide=sign_hide)


def _oracle_pred(O, rec, t, w, h, B):
    """the oracle's prediction of block t from the reconstruction so far (no slices, tiles or constrained intra prediction)"""
    k, N, x, y, mode = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["mode"])
    plane = rec[k].reshape(-1)
    return ol.o_intra_pred(plane, rec[k].shape[1], x, y, N, mode, B, w, h, k != 0)


@functools.lru_cache(maxsize=None)
def _threshold_case(w, h, tiling, B, pic, qp):
    """Originals whose residual is one (even blocks) or two (odd blocks) changed samples on the oracle's own prediction, the
    amplitude the smallest at which the block's uiAbsSum reaches 1 (even) or 2 (odd).  Returns (decisions, originals, the oracle's
    (reconstruction, levels) from hmo_intra_frame_encode on those originals, uiAbsSum per block)."""
    O = ol.oracle()
    tus = _tus(w, h, tiling, pic)
    mx = (1 << B) - 1
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    org = [np.zeros(s, np.int16) for s in shapes]
    rec = [np.zeros(s, np.int16) for s in shapes]
    sums, seen = [], {}
    for i, t in enumerate(tus):
        k, N, x, y, mode, ts = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["mode"]), int(t["flags"]) & 1
        pred = np.asarray(_oracle_pred(O, rec, t, w, h, B)).reshape(N, N).astype(np.int32)
        q = O.hmo_setQPforQuant(qp, int(k != 0), 6 * (B - 8), 0)
        cfg = ol.quant_cfg(q.per, q.rem, 1, 1, O.hmo_coef_scan_idx(N, int(k == 0), 1, mode))
        tmode = mode if k == 0 else 65535
        target = 1 + (seen.get((k, N), 0) & 1)  # alternating among the blocks of one size and plane: what a wave-item is filled from
        seen[(k, N)] = seen.get((k, N), 0) + 1
        # a changed sample spreads over every coefficient; where several share the largest magnitude (a corner sample of a large
        # block) the sum jumps over the target: the next position is tried, then (None: 32x32, whose first pass rounds a lone sample
        # into many equal coefficients) the same step on every sample, a lone DC level; the last form stands whatever it gives
        lvl, abs_sum, resi = None, 0, None
        for first in ((N - 1, N - 1), (1, 2), (N // 4, N // 2 + 1), None):
            spots = [first, (0, N // 2)][:target] if first else [(r, c) for r in range(N) for c in range(N)]
            sign = 1 if int(pred.max()) + 8 <= mx else -1
            for a in range(1, mx + 1):
                resi = np.zeros((N, N), np.int32)
                for (r, c) in spots:
                    resi[r, c] = (a if pred[r, c] + a <= mx else -a) if first else sign * min(a, 8)
                lvl, abs_sum = ol.o_transformNxN(resi.astype(np.int16), N, B, tmode, ts, cfg)
                if abs_sum >= target:
                    break
            if abs_sum == target:
                break
        org[k][y:y + N, x:x + N] = pred + resi
        r = ol.o_invtransformNxN(lvl, N, B, tmode, q.per, q.rem, ts) if abs_sum else np.zeros((N, N), np.int16)
        rec[k][y:y + N, x:x + N] = np.clip(pred + r, 0, mx)
        sums.append(int(abs_sum))
    want = ol.o_intra_frame_encode(tus, w, h, B, qp, org)
    for p in range(3):  # the block-by-block composition is the frame oracle
        assert np.array_equal(want[0][p], rec[p])
    return tus, org, want, np.array(sums)


def _call(ctx, w, h, plans, orgs, want, decode):
    L, n = capi.lib(), len(orgs)
    d_org = [capi.DevPicture(ctx, w, h).upload(o) for o in orgs]
    d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
    d_lev = [capi.DevPicture(ctx, w, h, dtype=np.int32) for _ in range(n)]
    for i, d in enumerate(d_lev):
        d.upload(want[i][1]) if decode else d.zero()
    A = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
    parr = (C.c_void_p * n)(*[p.value for p in plans])
    try:
        if decode:
            ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, parr, n, A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        else:
            ctx._chk(L.hmx_frame_intra_encode_multi(ctx.h, parr, n, A(d_org, capi.Pic), A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        ctx.sync()
        sched = C.c_int()
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3, sched.value  # the packed schedule
        return [(d_rec[i].download(), d_lev[i].download()) for i in range(n)]
    finally:
        for d in d_org + d_rec + d_lev:
            d.free()


def _run(ctx, hmx_opts, w, h, cases, what, sign_hide=1, qp=QP):
    """encode and decode the pictures of `cases` (a list of (decisions, originals, oracle result)) in one call each; both must be
    the oracle's"""
    L = capi.lib()
    hmx_opts(ctx, HMX_INTRA_SCHEDULE="p", HMX_PACK_SLOTS4="64", HMX_PACK_SLOTS8="16")
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, sign_hide)
    tus, orgs, want = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    plans = ctx.intra_plans(tus, pp, None)
    try:
        for decode in (False, True):
            got = _call(ctx, w, h, plans, orgs, want, decode)
            for i in range(len(cases)):
                for p in range(3):
                    assert np.array_equal(got[i][1][p], want[i][1][p]), ("levels", decode) + what + (i, p)
                    assert np.array_equal(got[i][0][p], want[i][0][p]), ("reconstruction", decode) + what + (i, p)
    finally:
        L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * len(plans))(*[p.value for p in plans]), len(plans))


@pytest.mark.parametrize("tiling", TILINGS)
@pytest.mark.parametrize("pic", PICS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_packed_parity(ctx, hmx_opts, pic, tiling):
    w, h = pic
    for n in COUNTS:
        _run(ctx, hmx_opts, w, h, [_case(w, h, tiling, ctx.bit_depth, i)[:3] for i in range(n)], (w, h, tiling, n))


@pytest.mark.parametrize("luma_mode", [1, 0], ids=["dc", "planar"])
@pytest.mark.parametrize("tiling", [4] + TILINGS)
def test_all_dc_all_planar(ctx, hmx_opts, tiling, luma_mode):
    for w, h in PICS:
        _run(ctx, hmx_opts, w, h, [_case(w, h, tiling, ctx.bit_depth, i, luma_mode) for i in range(3)], (w, h, tiling, luma_mode))


@pytest.mark.parametrize("tiling", [4] + TILINGS)
def test_abs_sum_threshold(ctx, hmx_opts, tiling):
    w, h, B = 128, 64, ctx.bit_depth
    cases = [_threshold_case(w, h, tiling, B, i, QP) for i in range(3)]
    for tus, _, want, sums in cases:
        assert (sums == 1).any() and (sums == 2).any(), np.bincount(sums)  # no hiding beside hiding
        # neighbours in the order the wave-items are filled from: blocks of one size and plane, a sum of 1 right beside a sum of 2
        key = tus["log2n"].astype(int) * 4 + tus["plane"]
        for k in np.unique(key):
            s = sums[key == k]
            if len(s) < 4:  # (a size the mix holds a block or two of)
                continue
            assert ((s[:-1] == 1) & (s[1:] == 2)).any() or ((s[:-1] == 2) & (s[1:] == 1)).any(), (tiling, k, s[:16])
    _run(ctx, hmx_opts, w, h, [c[:3] for c in cases], (w, h, tiling, "threshold"))


def test_twelve_bit(hmx_opts):
    c = capi.Context(bit_depth=12)
    try:
        _run(c, hmx_opts, 128, 64, [_case(128, 64, "mix", 12, i) for i in range(3)], ("12 bit",))
    finally:
        c.close()


def test_no_sign_hiding(ctx, hmx_opts):
    w, h = 128, 64
    _run(ctx, hmx_opts, w, h, [_case(w, h, "mix", ctx.bit_depth, i, None, 0) for i in range(3)], ("sign_hide 0",), sign_hide=0)


@pytest.mark.parametrize("tiling", [4] + TILINGS)
def test_lane_sums_of_satd(ctx, tiling):
    """satd_block's two sums (sub-block, then block) for every block of a picture, chroma included, against the oracle's calcHAD"""
    O, L, B = ol.oracle(), capi.lib(), ctx.bit_depth
    O.hmo_calcHAD.restype = C.c_uint32
    w, h = 64, 64
    tus = _tus(w, h, tiling, 0)
    rec = workload.make_planes(8700, w, h, B, "noise")
    org = workload.make_planes(8701, w, h, B, "texture")
    pp = capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1)
    lst = ctx.tu_list(tus)
    d_rec, d_org = capi.DevPicture(ctx, w, h).upload(rec), capi.DevPicture(ctx, w, h).upload(org)
    d_cost = ctx.alloc(4 * len(tus))
    try:
        ctx._chk(L.hmx_batch_predIntra_cost(ctx.h, lst, C.byref(d_rec.as_pic()), C.byref(d_org.as_pic()), C.byref(pp), None, 0, d_cost.ptr))
        ctx.sync()
        cost = d_cost.download(np.uint32)
    finally:
        L.hmx_tu_list_destroy(ctx.h, lst)
        d_rec.free(), d_org.free(), d_cost.free()
    flat = [p.reshape(-1).copy() for p in rec]
    for i, t in enumerate(tus):
        N, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        ob = np.ascontiguousarray(org[p][y:y + N, x:x + N])
        pb = np.ascontiguousarray(ol.o_intra_pred(flat[p], rec[p].shape[1], x, y, N, int(t["mode"]), B, w, h, p != 0))
        want = O.hmo_calcHAD(ob.ctypes.data_as(C.c_void_p), N, pb.ctypes.data_as(C.c_void_p), N, N, N, B)
        assert cost[i] == want, ("satd", tiling, i, N, p)
