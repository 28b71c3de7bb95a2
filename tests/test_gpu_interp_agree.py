"""Every entry that interpolates luma returns the same prediction for the same block and the same quarter-sample vector: the
stage parameters (shift, offset, clip) are one function (interp_stage: thevc_amd/csrc/hmx_kernels.h) that six kernels share, and
the weights of one or two lists one function (wp_pair).  The sibling of test_gpu_dist_agree.py, which holds the vector at (0, 0)
and so never enters a filter.  The expected samples are subpel_oracle.predict -- the project's C oracle, horizontal stage into the
14-bit intermediate and then vertical -- and the expected distortions subpel_oracle.measure of them; the oracle's one-stage route
(hmo_predInterLumaBlk, as tests/test_gpu_parity.py::test_scalar_motion_compensation_dropins uses it) is held against them on the
CPU first, on the very inputs used (test_two_constructions_agree: it needs no GPU).

A 64 x 64 picture with margin 16.  Five units, one per shape, side by side in the picture so that one batch call can hold them all;
the shapes are the smallest at which the shared code can go wrong: one sub-block of each side, the side falling to 4 by the height
alone, several 4x4 sub-blocks, and 24x32: twelve 8x8 sub-blocks = 96 lanes, a half-busy second wave in the lane form.  All sixteen
phases, each with the integer vectors (-3, 2) and (1, -2) in the fan-out and with one of them (by parity) in the entries that take
one vector per call.  Contents: a seeded texture, and extreme_inputs.overshoot_plane of the half-sample taps with either sign,
where the 16-bit narrowing between the stages and the final clip are reached.  Two weighted cases, one list and two lists, with
every field of the tables at an end of its range, against wp_oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

import extreme_inputs as xi
import oracle_lib as ol
import subpel_oracle as so
import wp_oracle as wo
from thevc_amd import capi

W = H = 64
M = 16
ST = W + 2 * M
UNITS = ((0, 0, 24, 32), (24, 0, 12, 16), (36, 0, 8, 8), (44, 0, 8, 4), (52, 0, 4, 4))  # (x, y, w, h): the shapes the issue names
INTS = ((-3, 2), (1, -2))                                                              # integer vectors, both signs in both components
PHASES = tuple((fx, fy) for fy in range(4) for fx in range(4))
MVS = tuple((4 * INTS[(fx + fy) & 1][0] + fx, 4 * INTS[(fx + fy) & 1][1] + fy) for (fx, fy) in PHASES)  # one vector per phase
BITS = (8, 10, 12)
CONTENTS = ("texture", "overshoot+", "overshoot-")
SCENES = [(B, content) for B in BITS for content in CONTENTS]
# the weighted cases: (weight, offset, log2_denom) per component Y, Cb, Cr, every value at an end of its range.  Two lists use list
# 0's denominators; the luma offsets of the two lists sum to 254, those of Cr to -256.
WP_UNI = ([255, -128, 255], [-128, 127, 127], [7, 0, 0])
WP_BI = (([-128, 255, -128], [127, -128, -128], [7, 0, 7]), ([255, -128, 255], [127, 127, -128], [0, 7, 0]))
WP_MVS = ((MVS[0], MVS[6]), (MVS[6], MVS[11]), (MVS[11], MVS[13]), (MVS[13], MVS[0]))  # (list 0, list 1): phases (0,0) (2,1) (3,2) (1,3)


class Expect:
    """The inputs of one (bit depth, content) and what the oracle makes of them; CPU only, made once and not changed."""

    def __init__(self, B, content):
        self.B = B
        rng = np.random.default_rng(1700 + 16 * B + CONTENTS.index(content))
        half = xi.LUMA_TAPS[2]

        def luma(sign):
            if content == "texture":
                return rng.integers(0, 1 << B, (H + 2 * M, ST)).astype(np.int16)
            return np.ascontiguousarray(xi.overshoot_plane(rng, ST, H + 2 * M, B, half, half, sign)[0], np.int16)

        def chroma():
            return rng.integers(0, 1 << B, (H // 2 + M, W // 2 + M)).astype(np.int16)

        sign = -1 if content == "overshoot-" else 1
        self.refs = [[luma(sign), chroma(), chroma()], [luma(-sign), chroma(), chroma()]]  # planes WITH margins; list 1 reads the second
        self.org = rng.integers(0, 1 << B, (H, W)).astype(np.int16)
        for a in [self.org] + [p for r in self.refs for p in r]:
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def pred(self, unit, mv):
        """the two-stage prediction of the unit from reference 0"""
        x, y, w, h = unit
        return so.predict(self.refs[0][0], M + x, M + y, w, h, mv[0], mv[1], self.B)

    def one_stage(self, unit, mv):
        """xPredInterLumaBlk's own route: one stage, or copy, where a fraction is zero"""
        x, y, w, h = unit
        out = np.zeros((h, w), np.int16)
        ol.oracle().hmo_predInterLumaBlk(ol.ptr(self.refs[0][0].reshape(-1), (M + y) * ST + M + x), ST, mv[0], mv[1], w, h, out.reshape(-1), w, 0, self.B)
        return out

    def org_block(self, unit):
        x, y, w, h = unit
        return np.ascontiguousarray(self.org[y:y + h, x:x + w])

    def dist(self, unit, mv, use_had):
        return so.measure(self.org_block(unit), self.pred(unit, mv), self.B, use_had)

    @functools.lru_cache(maxsize=None)
    def weighted(self, bi, k):
        """wp_oracle's picture (three planes) of the five units under weighted case `bi` at the vectors WP_MVS[k]"""
        pus = np.zeros(len(UNITS), ol.PU_DTYPE)
        for i, (x, y, w, h) in enumerate(UNITS):
            (m0, m1) = WP_MVS[k]
            pus[i] = (x, y, w, h, 0, 1 if bi else 255, m0[0], m0[1], m1[0] if bi else 0, m1[1] if bi else 0)
        l0, l1 = (WP_BI[0], WP_BI[1]) if bi else (WP_UNI, WP_UNI)
        return pus, wo.mc_frame_wp(pus, [(self.refs[0], M), (self.refs[1], M)], ([l0, l0], [l1, l1]), self.B)


@functools.lru_cache(maxsize=None)
def expect(B, content):
    return Expect(B, content)


class Scene:
    """The inputs of an Expect on the device."""

    def __init__(self, E):
        self.E, self.ctx = E, capi.Context(bit_depth=E.B)
        self.refs = []
        for planes in E.refs:
            d = capi.DevPicture(self.ctx, W, H, M, M)
            for p in range(3):
                d.bufs[p].upload(planes[p].reshape(-1))
            self.refs.append(d)
        z = np.zeros((H // 2, W // 2), np.int16)
        self.dorg = capi.DevPicture(self.ctx, W, H).upload([E.org, z, z])
        self.dst = capi.DevPicture(self.ctx, W, H).zero()

    def host_pic(self, r):
        p = capi.Pic()
        for k, a in enumerate(self.E.refs[r]):
            m = M >> (1 if k else 0)
            p.plane[k], p.stride[k] = a.ctypes.data + 2 * (m * a.shape[1] + m), a.shape[1]
        return p

    def free(self):
        for d in self.refs + [self.dorg, self.dst]:
            d.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(B, content):
        if (B, content) not in made:
            made[(B, content)] = Scene(expect(B, content))
        return made[(B, content)]

    yield get
    for s in made.values():
        s.free()


@pytest.mark.parametrize("B,content", SCENES)
def test_two_constructions_agree(B, content):
    """CPU: the two-stage route equals xPredInterLumaBlk's one-stage and copy cases on every input the GPU tests use, and the
    overshoot planes do reach the final clip."""
    E = expect(B, content)
    for unit in UNITS:
        for mv in MVS:
            assert np.array_equal(E.pred(unit, mv), E.one_stage(unit, mv)), (unit, mv)
    if content != "texture":
        p = E.pred(UNITS[0], MVS[10])  # phase (2, 2)
        assert p.min() == 0 and p.max() == (1 << B) - 1
    assert len({E.dist(u, MVS[5], 1) for u in UNITS}) == len(UNITS)  # the expected values are no constants


@pytest.mark.gpu
@pytest.mark.parametrize("B,content", SCENES)
def test_scalar_luma_block(scenes, B, content):
    s, L = scenes(B, content), capi.lib()
    full = s.E.refs[0][0]
    for unit in UNITS:
        x, y, w, h = unit
        for mv in MVS:
            got = np.zeros((h, w), np.int16)
            s.ctx._chk(L.hmx_xPredInterLumaBlk(s.ctx.h, full.ctypes.data + 2 * ((M + y) * ST + M + x), ST, mv[0], mv[1], w, h, got.ctypes.data, w, 0))
            assert np.array_equal(got, s.E.pred(unit, mv)), ("hmx_xPredInterLumaBlk", unit, mv)


@pytest.mark.gpu
@pytest.mark.parametrize("B,content", SCENES)
def test_batch_motion_compensation_luma(scenes, B, content):
    s, L = scenes(B, content), capi.lib()
    ref_arr = (capi.Pic * 1)(s.refs[0].as_pic())
    for mv in MVS:
        pus = np.zeros(len(UNITS), capi.PU_DTYPE)
        for i, (x, y, w, h) in enumerate(UNITS):
            pus[i] = (x, y, w, h, 0, 255, mv[0], mv[1], 0, 0)
        d_pus = s.ctx.to_device(pus)
        s.ctx._chk(L.hmx_batch_motionCompensation(s.ctx.h, d_pus.ptr, len(pus), ref_arr, 1, C.byref(s.dst.as_pic())))
        s.ctx.sync()
        got = s.dst.download()[0]
        d_pus.free()
        for unit in UNITS:
            x, y, w, h = unit
            assert np.array_equal(got[y:y + h, x:x + w], s.E.pred(unit, mv)), ("hmx_batch_motionCompensation", unit, mv)


@pytest.mark.gpu
@pytest.mark.parametrize("B,content", SCENES)
def test_subpel_cost(scenes, B, content):
    s = scenes(B, content)
    items = [(unit, iv) for unit in UNITS for iv in INTS]
    pus = np.zeros(len(items), capi.PU_DTYPE)
    for i, ((x, y, w, h), (ix, iy)) in enumerate(items):
        pus[i] = (x, y, w, h, 0, 255, 4 * ix, 4 * iy, 0, 0)
    offs = np.array(PHASES, np.int8)
    for use_had in (0, 1):
        got = s.ctx.batch_subpel_cost(pus, [s.refs[0]], s.dorg, offs, use_had)
        want = [[s.E.dist(unit, (4 * ix + fx, 4 * iy + fy), use_had) for (fx, fy) in PHASES] for (unit, (ix, iy)) in items]
        assert got.tolist() == want, ("hmx_batch_subpel_cost", use_had)


@pytest.mark.gpu
@pytest.mark.parametrize("B,content", SCENES)
def test_subpel_search_stage_costs(scenes, B, content):
    """The eighteen costs of the two stages with lambda 0 are the distortions at the eighteen vectors the refinement visits."""
    s = scenes(B, content)
    items = [(unit, iv) for unit in UNITS for iv in INTS]
    units, ints = np.zeros(len(items), capi.ME_UNIT_DTYPE), np.zeros(len(items), capi.ME_RESULT_DTYPE)
    for i, ((x, y, w, h), (ix, iy)) in enumerate(items):
        units[i] = (x, y, w, h, 0, 0, 0, 0, ix, iy, ix, iy)  # the box is the integer vector alone
        ints[i] = (ix, iy, 0, 0)
    for use_had in (0, 1):
        res, costs = s.ctx.batch_subpel_search(units, ints, [s.refs[0]], s.dorg, W, H, M, M, 0, use_had, want_stage_costs=True)
        for i, (unit, (ix, iy)) in enumerate(items):
            x, y, w, h = unit
            (mvx, mvy, dist, cost), want, (half, q) = so.refine(s.E.org_block(unit), s.E.refs[0][0], M + x + ix, M + y + iy, B, use_had, 0, (0, 0), ix, iy)
            assert costs[i].tolist() == want, ("hmx_batch_subpel_search", unit, (ix, iy), use_had)
            assert (int(res[i]["mvx"]), int(res[i]["mvy"]), int(res[i]["dist"])) == (mvx, mvy, dist)
            # and the winner's distortion is the fan-out's and the scalar entries' number at that vector
            assert dist == s.E.dist(unit, (mvx, mvy), use_had)


@pytest.mark.gpu
@pytest.mark.parametrize("B,content", SCENES)
def test_prediction_error(scenes, B, content):
    s = scenes(B, content)
    ref0 = s.host_pic(0)
    items = [(unit, mv) for unit in UNITS for mv in MVS]
    cands = np.zeros(len(items), capi.PU_DTYPE)
    for i, ((x, y, w, h), mv) in enumerate(items):
        cands[i] = (x, y, w, h, 0, 255, mv[0], mv[1], 0, 0)
    for use_had in (0, 1):
        want = [s.E.dist(unit, mv, use_had) for (unit, mv) in items]
        got = [s.ctx.getInterPredictionError(ref0, mv, None, None, unit[0], unit[1], unit[2], unit[3], s.E.org_block(unit), unit[2], use_had)
               for (unit, mv) in items]
        assert got == want, ("hmx_getInterPredictionError", use_had)
        dist, _, _ = s.ctx.batch_inter_pred_error(cands, None, None, [s.refs[0]], s.dorg, W, H, M, M, 0, use_had)
        assert dist.tolist() == want, ("hmx_batch_inter_pred_error", use_had)


@pytest.mark.gpu
@pytest.mark.parametrize("bi", [0, 1], ids=["uni", "bi"])
@pytest.mark.parametrize("B,content", SCENES)
def test_weighted(scenes, B, content, bi):
    """One list and two lists with the tables at their range ends: the scalar entry, the batch entry (cell map) and the fused
    prediction error, whose distortion is the plain one of the weighted prediction (bApplyWeight = false)."""
    s, L = scenes(B, content), capi.lib()
    e0, e1 = (WP_BI[0], WP_BI[1]) if bi else (WP_UNI, None)
    tab = lambda e: np.array([(e[0], e[1], e[2], 0)] * 2, capi.WP_DTYPE)  # one row per reference
    tables = (tab(e0), tab(e1) if bi else None)
    ref_arr = (capi.Pic * 2)(s.refs[0].as_pic(), s.refs[1].as_pic())
    r0, r1 = s.host_pic(0), s.host_pic(1)
    for k, (m0, m1) in enumerate(WP_MVS):
        pus, want = s.E.weighted(bi, k)
        # hmx_motionCompensation_wp, unit by unit
        for (x, y, w, h) in UNITS:
            dst = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
            dp = capi.Pic()
            for p in range(3):
                dp.plane[p], dp.stride[p] = dst[p].ctypes.data, dst[p].shape[1]
            s.ctx.motion_compensation_wp(r0, m0, r1 if bi else None, m1, x, y, w, h, dp, capi.wp_entry(*e0), capi.wp_entry(*e1) if bi else None)
            for p in range(3):
                ch = 1 if p else 0
                assert np.array_equal(dst[p], want[p][y >> ch:(y + h) >> ch, x >> ch:(x + w) >> ch]), ("hmx_motionCompensation_wp", (x, y, w, h), k, p)
        # hmx_batch_motionCompensation_wp_multi, the five units in one job
        d_pus = s.ctx.to_device(pus)
        dst_pic = s.dst.as_pic()
        job = (capi.McJob * 1)()
        job[0].d_pus, job[0].n_pus, job[0].refs, job[0].n_refs = d_pus.ptr, len(pus), ref_arr, 2
        job[0].dst, job[0].pic_w, job[0].pic_h = C.pointer(dst_pic), W, H
        s.ctx.batch_motion_compensation_wp(job, [tables])
        s.ctx.sync()
        got = s.dst.download()
        d_pus.free()
        for (x, y, w, h) in UNITS:
            for p in range(3):
                ch = 1 if p else 0
                sl = (slice(y >> ch, (y + h) >> ch), slice(x >> ch, (x + w) >> ch))
                assert np.array_equal(got[p][sl], want[p][sl]), ("hmx_batch_motionCompensation_wp_multi", (x, y, w, h), k, p)
        # hmx_batch_inter_pred_error_wp
        for use_had in (0, 1):
            dist, _, _ = s.ctx.batch_inter_pred_error(pus, None, None, s.refs, s.dorg, W, H, M, M, 0, use_had, wp=tables)
            exp = [so.measure(s.E.org_block(u), want[0][u[1]:u[1] + u[3], u[0]:u[0] + u[2]], B, use_had) for u in UNITS]
            assert dist.tolist() == exp, ("hmx_batch_inter_pred_error_wp", k, use_had)
