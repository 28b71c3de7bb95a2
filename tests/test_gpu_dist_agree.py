"""Every entry that measures one block against its prediction returns the same number for the same block: the sub-block rule
(8x8 Hadamard sub-blocks, 4x4 when a side is no multiple of 8, each rounded on its own; or the SAD) lives in two device helpers
(subblock_dist, subblock_dist_lanes: thevc_amd/csrc/hmx_kernels.h) that five kernels share.  The expected value is
subpel_oracle.measure -- the project's C oracle -- of the original block against the reference block at the integer position,
which is what each entry predicts here: unit weights, vector (0, 0), lambda 0.

A 64 x 64 picture with margin 8, the unit at its origin.  The shapes are the smallest at which the shared code can go wrong: one
sub-block of each side, the side falling to 4 by the height alone, several 4x4 and 8x8 sub-blocks a row and a column (24x32:
twelve sub-blocks = 96 lanes, so one wave of the lane form is half busy, and nine candidates of twelve leave a partial last
pass in the fused search), and 64x64, more sub-blocks than one pass of a workgroup holds.  Contents: a seeded random texture,
and the original at 2^B - 1 against a reference of 0, the largest differences there are."""
import ctypes as C

import numpy as np
import pytest

import subpel_oracle as so
from thevc_amd import capi

pytestmark = pytest.mark.gpu

W = H = 64
M = 8
SHAPES = ((4, 4), (8, 8), (8, 4), (12, 16), (16, 12), (24, 32), (64, 64))  # (w, h)
CASES = [(w, h, use_had) for (w, h) in SHAPES for use_had in (0, 1)]
CONTENTS = ("texture", "extremes")
UNIT_WP = capi.me_wp_table([1], [0], [0])


class Scene:
    def __init__(self, B, content):
        self.B, self.ctx = B, capi.Context(bit_depth=B)
        if content == "texture":
            rng = np.random.default_rng(1300 + B)
            self.org = rng.integers(0, 1 << B, (H, W)).astype(np.int16)
            self.full = rng.integers(0, 1 << B, (H + 2 * M, W + 2 * M)).astype(np.int16)
        else:
            self.org = np.full((H, W), (1 << B) - 1, np.int16)
            self.full = np.zeros((H + 2 * M, W + 2 * M), np.int16)
        self.ref = capi.DevPicture(self.ctx, W, H, M, M)
        self.ref.bufs[0].upload(self.full.reshape(-1))
        z = np.zeros((H // 2, W // 2), np.int16)
        self.dorg = capi.DevPicture(self.ctx, W, H).upload([self.org, z, z])
        # the oracle, once: the reference block at the integer position is the prediction of every entry below
        self.want = {(w, h, use_had): so.measure(self.org[:h, :w], self.full[M:M + h, M:M + w], B, use_had) for (w, h, use_had) in CASES}

    def blocks(self, w, h):
        """the original and the reference block, contiguous"""
        return np.ascontiguousarray(self.org[:h, :w]), np.ascontiguousarray(self.full[M:M + h, M:M + w])

    def free(self):
        self.ref.free()
        self.dorg.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def scenes():
    made = {}

    def get(B, content):
        if (B, content) not in made:
            made[(B, content)] = Scene(B, content)
        return made[(B, content)]

    yield get
    for s in made.values():
        s.free()


def test_oracle_values_are_not_constants(scenes):
    s = scenes(8, "texture")
    assert len(set(s.want.values())) == len(CASES)
    e = scenes(10, "extremes")
    assert e.want[(64, 64, 0)] == (64 * 64 * 1023) >> 2 and e.want[(4, 4, 0)] == (16 * 1023) >> 2


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("B", [8, 10])
def test_scalar_entries(scenes, B, content):
    s = scenes(B, content)
    L = capi.lib()
    for (w, h, use_had) in CASES:
        org, ref = s.blocks(w, h)
        want = s.want[(w, h, use_had)]
        if use_had:
            v = C.c_uint32()
            s.ctx._chk(L.hmx_calcHAD(s.ctx.h, org.ctypes.data, w, ref.ctypes.data, w, w, h, C.byref(v)))
            assert v.value == want, ("hmx_calcHAD", w, h)
            assert s.ctx.getHADsw(ref, w, org, w, w, h, 1, 0, 0) == want, ("hmx_getHADsw", w, h)
        else:
            assert s.ctx.getSADw(ref, w, org, w, w, h, 1, 0, 0) == want, ("hmx_getSADw", w, h)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("B", [8, 10])
def test_subpel_cost(scenes, B, content):
    s = scenes(B, content)
    pus = np.zeros(len(SHAPES), capi.PU_DTYPE)
    for i, (w, h) in enumerate(SHAPES):
        pus[i] = (0, 0, w, h, 0, 255, 0, 0, 0, 0)
    offs = np.zeros((1, 2), np.int8)
    for use_had in (0, 1):
        want = [s.want[(w, h, use_had)] for (w, h) in SHAPES]
        for wp in (None, UNIT_WP):
            got = s.ctx.batch_subpel_cost(pus, [s.ref], s.dorg, offs, use_had, wp=wp)
            assert [int(v) for v in got[:, 0]] == want, ("hmx_batch_subpel_cost", use_had, wp is not None)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("B", [8, 10])
def test_subpel_search(scenes, B, content):
    s = scenes(B, content)
    units = np.zeros(len(SHAPES), capi.ME_UNIT_DTYPE)
    for i, (w, h) in enumerate(SHAPES):
        units[i] = (0, 0, w, h, 0, 0, 0, 0, 0, 0, 0, 0)  # the box is the zero vector alone
    ints = np.zeros(len(SHAPES), capi.ME_RESULT_DTYPE)
    for use_had in (0, 1):
        want = [s.want[(w, h, use_had)] for (w, h) in SHAPES]
        for wp in (None, UNIT_WP):
            _, costs = s.ctx.batch_subpel_search(units, ints, [s.ref], s.dorg, W, H, M, M, 0, use_had, want_stage_costs=True, wp=wp)
            # entry 0: the half stage's centre candidate; with lambda 0 the vector term (lambda * bits) >> 16 is 0
            assert [int(v) for v in costs[:, 0]] == want, ("hmx_batch_subpel_search", use_had, wp is not None)


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("B", [8, 10, 12])
def test_pred_error_entries(scenes, B, content):
    s = scenes(B, content)
    cands = np.zeros(len(SHAPES), capi.PU_DTYPE)
    for i, (w, h) in enumerate(SHAPES):
        cands[i] = (0, 0, w, h, 0, 255, 0, 0, 0, 0)
    ref0 = capi.Pic()
    ref0.plane[0] = s.full.ctypes.data + (M * s.full.shape[1] + M) * 2
    ref0.stride[0] = s.full.shape[1]
    for use_had in (0, 1):
        want = [s.want[(w, h, use_had)] for (w, h) in SHAPES]
        dist, _, _ = s.ctx.batch_inter_pred_error(cands, None, None, [s.ref], s.dorg, W, H, M, M, 0, use_had)
        assert [int(v) for v in dist] == want, ("hmx_batch_inter_pred_error", use_had)
        got = [s.ctx.getInterPredictionError(ref0, (0, 0), None, None, 0, 0, w, h, s.org, W, use_had) for (w, h) in SHAPES]
        assert got == want, ("hmx_getInterPredictionError", use_had)
