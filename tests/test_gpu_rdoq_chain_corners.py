"""RDOQ as the quantiser of the whole-picture chain (hmx_set_rdoq + hmx_frame_intra_encode*) at the corners of its parameter
space and at the top of its 16-bit level words, GPU vs oracle bit for bit -- levels and reconstruction of every picture and
plane, then hmx_frame_intra_decode* on the produced levels:
  a. the parameter corners of the flat chain's test (12 bit, QP 0 and 51, CTU 16 / 32, chroma QP offsets through the table's
     clip) plus sign hiding off, with multipliers from 0.036 to 4669, both level layouts, packing groups of one and two;
  b. the lowest QP_Y the 16-bit check lets through for each largest block size, on saturating pictures (levels up to ~28000),
     and the refusal one QP_Y below;
  c. the refusal is exact: refused when extreme_inputs.rdoq_chain_must_refuse says so and only then, for plans analysed on
     the host and plans built on the device, and when one picture of a call alone holds the offending size;
  d. multipliers that quantise whole pictures to zero, and ones at which rate hardly counts.
The oracle's sign_hide == 0 branch and the level bound are pinned on the CPU by tests/test_rdoq_chain_corners.py.  Every case
asserts that it reached its edge.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import extreme_inputs as xi
import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu
HMX_ERR_ARG = -1


@pytest.fixture(scope="module")
def ctxs():
    made = {}

    def get(B, ctu=64):
        if (B, ctu) not in made:
            made[(B, ctu)] = capi.Context(bit_depth=B, ctu_size=ctu)
        return made[(B, ctu)]

    yield get
    for c in made.values():
        c.close()


class _Run:
    """One whole-picture encode call on zeroed outputs: plans = one plan for the call or a list with one per picture."""

    def __init__(self, ctx, plans, w, h, orgs, zorder=False):
        self.ctx, self.plans, self.w, self.h, self.n, self.zorder = ctx, plans, w, h, len(orgs), zorder
        n, L = self.n, capi.lib()
        self.d_org = [capi.DevPicture(ctx, w, h).upload(o) for o in orgs]
        self.d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
        self.d_lev = [(capi.DevLevelsZ(ctx, w, h, ctx.ctu_size) if zorder else capi.DevPicture(ctx, w, h, dtype=np.int32)).zero() for _ in range(n)]
        if isinstance(plans, list):
            self.rc = L.hmx_frame_intra_encode_multi(ctx.h, self._parr(), n, self._A(self.d_org, capi.Pic), self._A(self.d_rec, capi.Pic),
                                                     self._A(self.d_lev, capi.Levels))
        else:
            self.rc = L.hmx_frame_intra_encode(ctx.h, plans, n, self._A(self.d_org, capi.Pic), self._A(self.d_rec, capi.Pic),
                                               self._A(self.d_lev, capi.Levels))
        self.error = L.hmx_last_error(ctx.h) if self.rc else b""
        ctx.sync()

    def _A(self, lst, T):
        return (T * self.n)(*[x.as_pic() for x in lst])

    def _parr(self):
        return (C.c_void_p * self.n)(*[p.value for p in self.plans])

    def check(self, tus, want, what):
        """levels and reconstruction vs want = [(rec planes, level planes)]; then the decoder direction on these levels.
        tus = the block list of every picture (one list when the call had one plan)."""
        ctx, L, n = self.ctx, capi.lib(), self.n
        assert self.rc == 0, (what, self.rc, self.error)
        for i in range(n):
            t = tus[i] if isinstance(self.plans, list) else tus
            rec, lev = self.d_rec[i].download(), (self.d_lev[i].to_planes(t) if self.zorder else self.d_lev[i].download())
            for p in range(3):
                assert np.array_equal(lev[p], want[i][1][p]), (what, "levels", i, p, np.argwhere(lev[p] != want[i][1][p])[:4])
                assert np.array_equal(rec[p], want[i][0][p]), (what, "recon", i, p)
        d_dec = [capi.DevPicture(ctx, self.w, self.h).zero() for _ in range(n)]
        if isinstance(self.plans, list):
            ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, self._parr(), n, self._A(d_dec, capi.Pic), self._A(self.d_lev, capi.Levels)))
        else:
            ctx._chk(L.hmx_frame_intra_decode(ctx.h, self.plans, n, self._A(d_dec, capi.Pic), self._A(self.d_lev, capi.Levels)))
        ctx.sync()
        for i in range(n):
            dec = d_dec[i].download()
            assert all(np.array_equal(dec[p], want[i][0][p]) for p in range(3)), (what, "decode", i)
        for d in d_dec:
            d.free()

    def check_refused(self, what):
        """HMX_ERR_ARG with the 16-bit message, and nothing written."""
        assert self.rc == HMX_ERR_ARG and b"16 bits" in self.error, (what, self.rc, self.error)
        for i in range(self.n):
            assert not any(p.any() for p in self.d_rec[i].download()), (what, "rec written", i)
            assert not any(p.any() for p in self.d_lev[i].download()), (what, "levels written", i)

    def free(self):
        for d in self.d_org + self.d_rec + self.d_lev:
            d.free()


def _differs(a, b):
    """positions at which two pictures' level planes differ"""
    return sum(int((x != y).sum()) for x, y in zip(a, b))


# ---- a. parameter corners ------------------------------------------------------------------------------------------------------

CORNERS = [(12, 51, 64, 1, 0), (8, 0, 64, 1, 0), (10, 51, 32, 0, 0), (8, 22, 16, 1, 3), (12, 4, 64, 0, -5), (10, 37, 32, 1, 12),
           (8, 51, 64, 1, -12), (10, 27, 64, 0, 0)]


def corner_inputs(B, qp, ctu, n=5, w=152, h=88):
    tus = [workload.with_cbf_ctx(workload.make_tus(3100 + 10 * qp + i, w, h, "mix", ctu=ctu)) for i in range(n)]
    orgs = [workload.make_planes(200 + i, w, h, B, "texture" if i % 2 else "noise") for i in range(n)]
    ests = [[workload.make_est_bits(6000 + 8 * i + k) for k in range(8)] for i in range(n)]
    lam = workload.rdoq_lambdas(qp)
    lams = [(lam[0] * (1 + 0.01 * (i % 7)), lam[1] * (1 + 0.02 * (i % 5))) for i in range(n)]
    return tus, orgs, ests, lams


@pytest.mark.parametrize("B,qp,ctu,sign_hide,cqo", CORNERS)
def test_rdoq_chain_parameter_corners(ctxs, B, qp, ctu, sign_hide, cqo, hmx_opts):
    """The flat chain's corner list (tests/test_gpu_parity.py::test_frame_intra_parameter_corners) and one case that isolates
    sign hiding off, with RDOQ: five pictures with plans, tables and multipliers of their own (about 0.036 at QP 0, 4669 / 1167 at
    QP 51); packing groups of one with plane levels, then of two (a ragged last group) with levels in the reference's layout."""
    ctx = ctxs(B, ctu)
    w, h, n = 152, 88, 5
    tus, orgs, ests, lams = corner_inputs(B, qp, ctu)
    assert any((t["flags"] & capi.TU_TRANSFORM_SKIP).any() for t in tus)
    want, n_not_flat, n_flag = [], 0, 0
    for i in range(n):
        want.append(ol.o_intra_frame_encode_rdoq(tus[i], w, h, B, qp, orgs[i], ests[i], lams[i], sign_hide, cqo, ctu))
        n_not_flat += _differs(want[i][1], ol.o_intra_frame_encode(tus[i], w, h, B, qp, orgs[i], sign_hide, cqo, ctu)[1])
        if sign_hide:
            n_flag += _differs(want[i][1], ol.o_intra_frame_encode_rdoq(tus[i], w, h, B, qp, orgs[i], ests[i], lams[i], 0, cqo, ctu)[1])
    assert n_not_flat > 0, "RDOQ decided nothing the flat quantiser does not"
    assert n_flag > 0 or not sign_hide, "sign hiding changed nothing"
    L = capi.lib()
    plans = [ctx.intra_plan(t, capi.PicParam(w, h, qp, cqo, capi.I_SLICE, sign_hide)) for t in tus]
    try:
        for group, zorder in ((1, False), (2, True)):
            hmx_opts(ctx, HMX_PACK_GROUP=str(group))
            ctx.set_rdoq([(ests[i], lams[i][0], lams[i][1]) for i in range(n)])
            run = _Run(ctx, plans, w, h, orgs, zorder)
            run.check(tus, want, ("group", group))
            run.free()
    finally:
        ctx.set_rdoq(None)
        for pl in plans:
            L.hmx_intra_plan_destroy(ctx.h, pl)


# ---- b. the 16-bit boundary ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sign_hide", [1, 0])
@pytest.mark.parametrize("B,qp,N", xi.RDOQ_BOUNDARY_CASES)
def test_rdoq_chain_at_16_bit_boundary(ctxs, B, qp, N, sign_hide):
    """The lowest QP_Y at which a plan of N x N blocks is accepted (the inputs of tests/test_rdoq_chain_corners.py, where the
    oracle's levels are held to the bound): exact, with luma levels above 16383.  One QP_Y lower -- where the bit depth has one:
    -12 at 10 bit and -24 at 12 bit are the lowest QPs there are -- rem 4 meets qbits 14, a level can be 32768, and the call is
    refused with nothing written."""
    ctx, L = ctxs(B), capi.lib()
    w = h = 128
    tus, orgs, ests, lams = xi.rdoq_boundary_case(B, qp, N)
    want = [ol.o_intra_frame_encode_rdoq(tus, w, h, B, qp, o, ests, lams, sign_hide) for o in orgs]
    assert sum(int(np.count_nonzero(np.abs(wl[0].astype(np.int64)) > 16383)) for _, wl in want) > 0, "no luma level above 16383"
    plan = ctx.intra_plan(tus, capi.PicParam(w, h, qp, 0, capi.I_SLICE, sign_hide))
    lower = ctx.intra_plan(tus, capi.PicParam(w, h, qp - 1, 0, capi.I_SLICE, sign_hide)) if qp - 1 >= -xi.qp_bd_offset(B) else None
    assert (lower is None) == ((B, qp, N) in ((10, -12, 16), (12, -24, 4)))
    try:
        ctx.set_rdoq([(ests, lams[0], lams[1])])
        run = _Run(ctx, plan, w, h, orgs)
        run.check(tus, want, "boundary")
        run.free()
        if lower is not None:
            assert xi.rdoq_chain_must_refuse(tus, B, qp - 1, 0)
            run = _Run(ctx, lower, w, h, orgs)
            run.check_refused("one below the boundary")
            run.free()
    finally:
        ctx.set_rdoq(None)
        for pl in (plan, lower):
            if pl is not None:
                L.hmx_intra_plan_destroy(ctx.h, pl)


# ---- c. the refusal is exact ---------------------------------------------------------------------------------------------------

# QP_Y: the six values around each boundary of the bit depth that a tiling of the grid can meet (32x32: -7 at both depths;
# 16x16: -13 at 12 bit, none at 10 bit, whose lowest QP_Y is -12)
REFUSAL_QPS = {10: tuple(range(-10, -4)), 12: tuple(range(-16, -10)) + tuple(range(-10, -4))}


def _make_plans(ctx, tus_list, pp, builder):
    """One plan per block list from the host analysis or from the device builder (one call for all pictures): the two record
    the sizes a plan holds per texture type, which the 16-bit check reads, in code of their own."""
    if builder == "host":
        return [ctx.intra_plan(t, pp) for t in tus_list]
    d_cat = ctx.to_device(np.ascontiguousarray(np.concatenate(tus_list), capi.TU_DTYPE))
    try:
        return ctx.intra_plans_device(d_cat.ptr, np.concatenate([[0], np.cumsum([len(t) for t in tus_list])]), pp)
    finally:
        d_cat.free()


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("tiling", [32, 16, "mix"])
@pytest.mark.parametrize("B", [10, 12])
def test_rdoq_chain_refuses_exactly(ctxs, B, tiling, builder):
    """QP_Y around the boundaries x chroma QP offsets x tilings: refused exactly when a block, by ITS plane and size, can exceed
    16 bits -- a luma size does not stand for a chroma block (10 bit, QP_Y -6, offset -2, 32x32 luma: chroma index 4 is fine for
    the 16x16 chroma blocks there are), a low chroma QP alone does refuse (12 bit, QP_Y -7, offset -12: chroma index 5 on 16x16)
    -- and exact where accepted.  With plans analysed on the host and plans built on the device."""
    ctx, L = ctxs(B), capi.lib()
    w = h = 64
    rng = np.random.default_rng(5100 + B)
    tus = workload.with_cbf_ctx(workload.make_tus(60 + 2 * B, w, h, tiling, ts_prob=0.0))
    if tiling == "mix":
        assert {int(x) for x in tus["log2n"][tus["plane"] == 0]} == {2, 3, 4, 5}
    orgs = [xi.saturating_picture(rng, w, h, B, scale=tiling if tiling != "mix" else 16)]
    ests = [workload.make_est_bits(9200 + k) for k in range(8)]
    bd = xi.qp_bd_offset(B)
    top_luma = int(tus["log2n"][tus["plane"] == 0].max())
    n_refused = n_accepted = n_luma_size_would_refuse = 0
    for qp in REFUSAL_QPS[B]:
        for cqo in (-12, -2, 0, 6):
            lams = workload.rdoq_lambdas(qp)
            plans = _make_plans(ctx, [tus], capi.PicParam(w, h, qp, cqo, capi.I_SLICE, 1), builder)
            plan = plans[0] if builder == "host" else plans  # the one-plan entry / the plan-per-picture entry
            try:
                ctx.set_rdoq([(ests, lams[0], lams[1])])
                run = _Run(ctx, plan, w, h, orgs)
                if xi.rdoq_chain_must_refuse(tus, B, qp, cqo):
                    run.check_refused((qp, cqo))
                    n_refused += 1
                else:
                    run.check(tus if builder == "host" else [tus], [ol.o_intra_frame_encode_rdoq(tus, w, h, B, qp, orgs[0], ests, lams, 1, cqo)],
                              (qp, cqo))
                    n_accepted += 1
                    qc = ol.oracle().hmo_setQPforQuant(qp, 1, bd, cqo)
                    n_luma_size_would_refuse += int(xi.rdoq_max_level(B, qc.per, qc.rem, top_luma) > xi.INT16_MAX)
                run.free()
            finally:
                ctx.set_rdoq(None)
                L.hmx_intra_plan_destroy(ctx.h, plans[0])
    # at 10 bit 16x16 (qbits 15 at per 0) and smaller blocks stay within 16 bits at every QP
    assert n_accepted > 0 and (n_refused > 0) == ((B, tiling) != (10, 16)), (n_refused, n_accepted)
    if (B, tiling) != (10, 16):  # accepted although chroma at the largest LUMA size would exceed 16 bits
        assert n_luma_size_would_refuse > 0


# (B, QP_Y, chroma QP offset): 16x16 tilings are fine, a 32x32 tiling is not -- by its 32x32 luma blocks at 10 bit, QP_Y -8
# (index 4, qbits 14), by its 16x16 chroma blocks alone at 12 bit, QP_Y -7, offset -12 (index 5, qbits 13)
ONE_PICTURE_CASES = [(10, -8, 0), (12, -7, -12)]


@pytest.mark.parametrize("builder", ["host", "device"])
@pytest.mark.parametrize("B,qp,cqo", ONE_PICTURE_CASES)
def test_rdoq_chain_refuses_for_one_picture_of_a_call(ctxs, B, qp, cqo, builder):
    """Calls of three pictures with plans of their own: one picture alone holding the offending size -- the last, the middle or the
    first of the call -- has the whole call refused with nothing written; the same call without it is accepted and exact."""
    ctx, L = ctxs(B), capi.lib()
    w = h = 64
    rng = np.random.default_rng(5300 + B)
    fine = [workload.with_cbf_ctx(workload.make_tus(90 + i, w, h, 16, ts_prob=0.0)) for i in range(3)]
    bad = workload.with_cbf_ctx(workload.make_tus(95, w, h, 32, ts_prob=0.0))
    assert xi.rdoq_chain_must_refuse(bad, B, qp, cqo) and not any(xi.rdoq_chain_must_refuse(t, B, qp, cqo) for t in fine)
    if cqo:  # luma alone would pass: the chroma blocks of the one picture decide
        assert not xi.rdoq_chain_must_refuse(bad[bad["plane"] == 0], B, qp, cqo)
    orgs = [xi.saturating_picture(rng, w, h, B, scale=16) for _ in range(3)]
    ests = [workload.make_est_bits(9300 + k) for k in range(8)]
    lams = workload.rdoq_lambdas(qp)
    pp = capi.PicParam(w, h, qp, cqo, capi.I_SLICE, 1)
    for at in (2, 1, 0, None):
        tus = [bad if i == at else fine[i] for i in range(3)]
        plans = _make_plans(ctx, tus, pp, builder)
        try:
            ctx.set_rdoq([(ests, lams[0], lams[1])])
            run = _Run(ctx, plans, w, h, orgs)
            if at is None:
                run.check(tus, [ol.o_intra_frame_encode_rdoq(tus[i], w, h, B, qp, orgs[i], ests, lams, 1, cqo) for i in range(3)], "all fine")
            else:
                run.check_refused(("offending picture", at))
            run.free()
        finally:
            ctx.set_rdoq(None)
            for pl in plans:
                L.hmx_intra_plan_destroy(ctx.h, pl)


# ---- d. multiplier extremes ----------------------------------------------------------------------------------------------------

def test_rdoq_chain_multiplier_extremes(ctxs):
    """10 bit, QP 30, three pictures.  Multipliers of 1e7: whole pictures quantise to zero (every block takes the abs_sum == 0
    path: reconstruction = prediction); the plans hold no transform-skip block, which the flat quantiser would code.  Multipliers of
    1e-4: rate hardly counts, and the result still is not the flat quantiser's."""
    B, qp, w, h, n = 10, 30, 152, 88, 3
    ctx, L = ctxs(B), capi.lib()
    tus = [workload.with_cbf_ctx(workload.make_tus(3500 + i, w, h, "mix", ts_prob=0.0)) for i in range(n)]
    orgs = [workload.make_planes(260 + i, w, h, B, "texture" if i % 2 else "noise") for i in range(n)]
    ests = [workload.make_est_bits(6100 + k) for k in range(8)]
    plans = [ctx.intra_plan(t, capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)) for t in tus]
    try:
        for lam in (1e7, 1e-4):
            want = [ol.o_intra_frame_encode_rdoq(tus[i], w, h, B, qp, orgs[i], ests, (lam, lam)) for i in range(n)]
            if lam > 1:
                assert not any(p.any() for _, wl in want for p in wl), "a level survived"
            else:
                assert all(_differs(want[i][1], ol.o_intra_frame_encode(tus[i], w, h, B, qp, orgs[i])[1]) > 0 for i in range(n))
            ctx.set_rdoq([(ests, lam, lam)])
            run = _Run(ctx, plans, w, h, orgs)
            run.check(tus, want, lam)
            run.free()
    finally:
        ctx.set_rdoq(None)
        for pl in plans:
            L.hmx_intra_plan_destroy(ctx.h, pl)
