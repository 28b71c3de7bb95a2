"""A QP per block on the device (hmx_set_qp_map, hmx_aq_unit_qp_multi) against the yardstick of tests/qp_map_oracle.py: the
whole-picture chain on the packed schedule in both directions, the block-list transform entries, every refusal, the clamp, and the
bridge from the AQ layer QPs to the unit map.  The picture is 128 x 64, two CTUs of 64, with every transform size that exists."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol
import qp_map_oracle as qo
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

W, H, N_PICS = 128, 64, 3
UH, UW = qo.unit_dims(W, H)
# (bit depth, chroma_qp_offset, slice QP): at 10 bit the negative offset takes the units near -QpBDOffset to a chroma QP below 0
CASES = {8: (2, 33), 10: (-9, 5)}


@pytest.fixture(scope="module")
def ctxs():
    c = {B: capi.Context(bit_depth=B) for B in CASES}
    yield c
    for v in c.values():
        v.close()


def planted(B, cqo):
    off = 6 * (B - 8)
    plant = [51, -off, 30, 33, 36, 40, 43]  # the range ends; 30..43: g_aucChromaScale is not linear there
    if cqo < 0:
        plant += [-off + 1, -off + 4]  # luma QP + offset < -QpBDOffset: the chroma QP of these units is below 0
    return plant


class Scene:
    """Three pictures with plans, originals and maps of their own, and the yardstick's answers (computed once per bit depth)."""
    cache = {}

    def __init__(self, B):
        self.B = B
        self.cqo, self.slice_qp = CASES[B]
        self.tus = [qo.all_sizes_tus(40 + i) for i in range(N_PICS)]
        self.org = [workload.make_planes(500 + 10 * B + i, W, H, B, "texture" if i != 1 else "noise") for i in range(N_PICS)]
        self.maps = np.stack([qo.varied_map(60 + B + i, W, H, B, self.slice_qp, planted(B, self.cqo)) for i in range(N_PICS)])
        self.want = [qo.encode(self.tus[i], W, H, B, self.org[i], self.maps[i], 1, self.cqo) for i in range(N_PICS)]

    @classmethod
    def get(cls, B):
        if B not in cls.cache:
            cls.cache[B] = cls(B)
        return cls.cache[B]


def test_scene_covers_what_the_issue_asks():
    for B, (cqo, slice_qp) in CASES.items():
        s, off = Scene.get(B), 6 * (B - 8)
        for i in range(N_PICS):
            q = qo.block_qps(s.tus[i], s.maps[i])
            cq = q[s.tus[i]["plane"] != 0] + cqo
            assert 51 in s.maps[i] and -off in s.maps[i] and ((s.maps[i] >= 30) & (s.maps[i] <= 43)).any()
            assert len(set(q.tolist())) >= 8
            if cqo < 0:
                assert (np.maximum(cq, -off) < 0).any(), "no chroma block below QP 0"
        assert not np.array_equal(s.maps[0], s.maps[1]) and not np.array_equal(s.maps[1], s.maps[2])


class Chain:
    """The device side of one whole-picture call over the scene's three pictures"""

    def __init__(self, ctx, s, pp_qp):
        self.ctx, self.s, self.L = ctx, s, capi.lib()
        self.pp = capi.PicParam(W, H, pp_qp, s.cqo, capi.I_SLICE, 1)
        self.plans = [ctx.intra_plan(t, self.pp) for t in s.tus]
        self.d_org = [capi.DevPicture(ctx, W, H).upload(o) for o in s.org]
        self.d_rec = [capi.DevPicture(ctx, W, H).zero() for _ in range(N_PICS)]
        self.d_lev = [capi.DevLevelsZ(ctx, W, H) for _ in range(N_PICS)]
        self.units = [2 * 256, 2 * 64, 2 * 64]
        self.d_sse = [[ctx.alloc(4 * u).zero() for u in self.units] for _ in range(N_PICS)]
        self.parr = (C.c_void_p * N_PICS)(*[p.value for p in self.plans])

    def arr(self, lst, T):
        return (T * N_PICS)(*[x.as_pic() for x in lst])

    def encode(self, sse=False):
        ctx, L = self.ctx, self.L
        if sse:
            sa = (capi.Sse * N_PICS)()
            for i in range(N_PICS):
                for p in range(3):
                    sa[i].plane[p] = self.d_sse[i][p].ptr
            ctx._chk(L.hmx_set_sse_output(ctx.h, sa, N_PICS))
        try:
            rc = L.hmx_frame_intra_encode_multi(ctx.h, self.parr, N_PICS, self.arr(self.d_org, capi.Pic), self.arr(self.d_rec, capi.Pic), self.arr(self.d_lev, capi.Levels))
        finally:
            if sse:
                ctx._chk(L.hmx_set_sse_output(ctx.h, None, 0))
        return rc

    def decode(self):
        return self.L.hmx_frame_intra_decode_multi(self.ctx.h, self.parr, N_PICS, self.arr(self.d_rec, capi.Pic), self.arr(self.d_lev, capi.Levels))

    def results(self):
        self.ctx.sync()
        return [d.download() for d in self.d_rec], [self.d_lev[i].to_planes(self.s.tus[i]) for i in range(N_PICS)]

    def raw(self):
        """every output byte of the call: reconstruction planes and the level buffers as they lie"""
        self.ctx.sync()
        return [np.concatenate([np.asarray(p).reshape(-1) for p in d.download()]) for d in self.d_rec], \
               [np.concatenate([b.download(np.int32) for b in d.bufs]) for d in self.d_lev]

    def close(self):
        for pl in self.plans:
            self.L.hmx_intra_plan_destroy(self.ctx.h, pl)
        for d in self.d_org + self.d_rec + self.d_lev:
            d.free()
        for t in self.d_sse:
            for b in t:
                b.free()


@pytest.mark.parametrize("B", sorted(CASES))
def test_chain_encode_decode_three_maps(ctxs, B, hmx_opts):
    """(a) levels, reconstruction and the distortion sums of the encoder, and the decoder's reconstruction from the yardstick's
    levels, equal the yardstick exactly; three pictures, three maps, groups of two pictures: the picture's index inside its group
    must select the right map.  PicParam.qp is a value no unit holds: it must not be used."""
    ctx, s = ctxs[B], Scene.get(B)
    hmx_opts(ctx, HMX_PACK_GROUP="2")
    ch = Chain(ctx, s, pp_qp=22)
    d_map = ctx.to_device(s.maps)
    try:
        ctx.set_qp_map(d_map, N_PICS)
        ctx._chk(ch.encode(sse=True))
        rec, lev = ch.results()
        for i in range(N_PICS):
            got = [ch.d_sse[i][p].download(np.uint32) for p in range(3)]
            for p in range(3):
                assert np.array_equal(lev[i][p], s.want[i][1][p]), ("levels", i, p)
                assert np.array_equal(rec[i][p], s.want[i][0][p]), ("reconstruction", i, p)
            for t in s.tus[i]:
                u = ch.d_lev[i].block_offset(int(t["plane"]), int(t["x"]), int(t["y"])) // 16
                assert int(got[int(t["plane"])][u]) == qo.block_sse(t, B, s.org[i], s.want[i][0]), ("sse", i, tuple(t))
        # the decoder direction, from the yardstick's levels
        for i in range(N_PICS):
            ch.d_lev[i].from_planes(s.want[i][1], s.tus[i])
            ch.d_rec[i].zero()
        ctx._chk(ch.decode())
        rec, _ = ch.results()
        for i in range(N_PICS):
            want = qo.decode(s.tus[i], W, H, B, s.want[i][1], s.maps[i], 1, s.cqo)
            for p in range(3):
                assert np.array_equal(want[p], s.want[i][0][p])
                assert np.array_equal(rec[i][p], want[p]), ("decode", i, p)
    finally:
        ctx.set_qp_map(None)
        ctx.sync()
        d_map.free()
        ch.close()


@pytest.mark.parametrize("B", sorted(CASES))
def test_uniform_map_switching_and_one_map_for_all(ctxs, B):
    """(b) a uniform map gives byte for byte what the call gives without a map; after hmx_set_qp_map(NULL) it gives that again; n_pics
    = 1 applies the one map to all three pictures."""
    ctx, s = ctxs[B], Scene.get(B)
    qp = s.slice_qp
    ch = Chain(ctx, s, pp_qp=qp)
    d_uni = ctx.to_device(np.full((UH, UW), qp, np.int8))
    d_one = ctx.to_device(s.maps[1])
    try:
        ctx._chk(ch.encode())
        plain = ch.raw()
        for d in ch.d_rec + ch.d_lev:
            d.zero()
        ctx.set_qp_map(d_uni, 1)
        ctx._chk(ch.encode())
        uni = ch.raw()
        for d in ch.d_rec + ch.d_lev:
            d.zero()
        ctx.set_qp_map(None)
        ctx._chk(ch.encode())
        again = ch.raw()
        for i in range(N_PICS):
            for k in range(2):
                assert np.array_equal(uni[k][i], plain[k][i]), ("uniform map", i, k)
                assert np.array_equal(again[k][i], plain[k][i]), ("map off", i, k)
        ctx.set_qp_map(d_one, 1)
        ctx._chk(ch.encode())
        rec, lev = ch.results()
        for i in range(N_PICS):
            wr, wl = qo.encode(s.tus[i], W, H, B, s.org[i], s.maps[1], 1, s.cqo)
            for p in range(3):
                assert np.array_equal(lev[i][p], wl[p]) and np.array_equal(rec[i][p], wr[p]), ("one map for all", i, p)
    finally:
        ctx.set_qp_map(None)
        ctx.sync()
        d_uni.free(), d_one.free()
        ch.close()


@pytest.mark.parametrize("B", sorted(CASES))
def test_block_list_entries(ctxs, B):
    """(c) the same blocks as blocks of inter coding units, two pictures with two maps, through
    hmx_batch_residual_transform_recon_sse_multi and hmx_batch_invtransformNxN_multi: levels, uiAbsSum, reconstruction and distortion
    of every block against the yardstick's per-block results."""
    ctx, s, L, n = ctxs[B], Scene.get(B), capi.lib(), 2
    tus = s.tus[0].copy()
    tus["flags"] |= capi.TU_INTER
    org = s.org[:n]
    pred = [workload.make_planes(900 + B + i, W, H, B, "texture") for i in range(n)]
    pp = capi.PicParam(W, H, 22, s.cqo, capi.B_SLICE, 1)
    tl = ctx.tu_list(tus)
    d_org = [capi.DevPicture(ctx, W, H).upload(o) for o in org]
    d_pred = [capi.DevPicture(ctx, W, H).upload(o) for o in pred]
    d_rec = [capi.DevPicture(ctx, W, H).zero() for _ in range(n)]
    d_out = [capi.DevPicture(ctx, W, H).zero() for _ in range(n)]
    d_lev = [capi.DevPicture(ctx, W, H, dtype=np.int32).zero() for _ in range(n)]
    d_abs, d_sse = ctx.alloc(4 * n * len(tus)).zero(), ctx.alloc(4 * n * len(tus)).zero()
    d_map = ctx.to_device(s.maps[:n])
    A = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
    try:
        ctx.set_qp_map(d_map, n)
        ctx._chk(L.hmx_batch_residual_transform_recon_sse_multi(ctx.h, tl, n, A(d_org, capi.Pic), A(d_pred, capi.Pic), A(d_lev, capi.Levels),
                                                                A(d_rec, capi.Pic), d_abs.ptr, d_sse.ptr, C.byref(pp)))
        ctx._chk(L.hmx_batch_invtransformNxN_multi(ctx.h, tl, n, A(d_lev, capi.Levels), A(d_pred, capi.Pic), A(d_out, capi.Pic), C.byref(pp)))
        ctx.sync()
        abs_sum, sse = d_abs.download(np.uint32).reshape(n, -1), d_sse.download(np.uint32).reshape(n, -1)
        for i in range(n):
            lev, rec, out = d_lev[i].download(), d_rec[i].download(), d_out[i].download()
            for k, t in enumerate(tus):
                p, N, x, y = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"])
                wl, wa, wr, ws = qo.inter_block(t, qo.block_qp(t, s.maps[i]), B, org[i][p][y:y + N, x:x + N], pred[i][p][y:y + N, x:x + N],
                                                1, s.cqo, 0)
                where = (i, k, p, x, y, N)
                assert np.array_equal(lev[p][y:y + N, x:x + N], wl), ("levels",) + where
                assert int(abs_sum[i, k]) == wa, ("abs sum",) + where
                assert np.array_equal(rec[p][y:y + N, x:x + N], wr), ("reconstruction",) + where
                assert int(sse[i, k]) == ws, ("sse",) + where
                assert np.array_equal(out[p][y:y + N, x:x + N], wr), ("inverse",) + where
    finally:
        ctx.set_qp_map(None)
        ctx.sync()
        L.hmx_tu_list_destroy(ctx.h, tl)
        for d in d_org + d_pred + d_rec + d_out + d_lev + [d_abs, d_sse, d_map]:
            d.free()


def test_refusals_leave_the_outputs_untouched(ctxs, hmx_opts):
    """(d) with a map set: RDOQ, the level schedule and the wave schedule are HMX_ERR_ARG before anything is launched, and the text says
    which; more pictures than maps likewise.  hmx_aq_unit_qp_multi refuses null pointers and a size outside the AQ domain."""
    B = 8
    ctx, s, L = ctxs[B], Scene.get(B), capi.lib()
    ch = Chain(ctx, s, pp_qp=30)
    d_map = ctx.to_device(s.maps)
    fill = [np.full(p.shape, 77, np.int16) for p in s.org[0]]

    def refused(call, word):
        for d in ch.d_rec:
            d.upload(fill)
        for d in ch.d_lev:
            for b in d.bufs:
                ctx._chk(L.hmx_memset(ctx.h, b.ptr, 0x5a, b.nbytes))
        rc = call()
        assert rc == -1, rc  # HMX_ERR_ARG
        msg = L.hmx_last_error(ctx.h).decode()
        assert word in msg and "hmx_set_qp_map" in msg, msg
        rec, lev = ch.raw()
        for i in range(N_PICS):
            assert (rec[i] == 77).all() and (lev[i] == 0x5a5a5a5a).all(), (word, i)

    try:
        ctx.set_qp_map(d_map, N_PICS)
        ests = [workload.make_est_bits(7000 + k) for k in range(8)]
        ctx.set_rdoq([(ests, 40.0, 35.0)])
        try:
            refused(ch.encode, "RDOQ")
        finally:
            ctx.set_rdoq(None)
        hmx_opts(ctx, HMX_INTRA_SCHEDULE="level")
        refused(ch.encode, "level schedule")
        refused(ch.decode, "level schedule")
        hmx_opts(ctx, HMX_INTRA_SCHEDULE="wave")
        refused(ch.encode, "wave schedule")
        ctx.set_option("HMX_INTRA_SCHEDULE", None)
        ctx.set_qp_map(d_map, 2)  # three pictures, two maps
        refused(ch.encode, "fewer pictures")
        # the AQ bridge
        d_a, d_b, d_c = ctx.alloc(4096).zero(), ctx.alloc(4096).zero(), ctx.alloc(4096).zero()
        for args in ((None, d_b.ptr, d_c.ptr), (d_a.ptr, None, d_c.ptr), (d_a.ptr, d_b.ptr, None)):
            assert L.hmx_aq_unit_qp_multi(ctx.h, 1, 64, 64, 64, 1, *args) != 0
        for bad in ((1, 60, 64, 64, 1), (1, 64, 64, 48, 1), (1, 64, 64, 16, 3), (0, 64, 64, 64, 1), (1, 64, 64, 64, 5), (1, 16392, 64, 64, 1)):
            assert L.hmx_aq_unit_qp_multi(ctx.h, bad[0], bad[1], bad[2], bad[3], bad[4], d_a.ptr, d_b.ptr, d_c.ptr) != 0, bad
        ctx.sync()
        assert not d_c.download(np.uint8).any()
        for d in (d_a, d_b, d_c):
            d.free()
    finally:
        ctx.set_option("HMX_INTRA_SCHEDULE", None)
        ctx.set_rdoq(None)
        ctx.set_qp_map(None)
        ctx.sync()
        d_map.free()
        ch.close()


def test_bytes_outside_the_legal_range_run_to_completion(ctxs):
    """(d) a map that holds 127 and -128: the kernels clamp what they read before they index their table.  Only completion is
    asserted (and that the clamp is the one documented: 127 acts as 51, -128 as -QpBDOffset)."""
    B = 10
    ctx, s = ctxs[B], Scene.get(B)
    ch = Chain(ctx, s, pp_qp=30)
    wild = s.maps.copy()
    wild[:, ::3, ::5], wild[:, 1::4, 2::3] = 127, -128
    d_map = ctx.to_device(wild)
    try:
        ctx.set_qp_map(d_map, N_PICS)
        ctx._chk(ch.encode())
        rec, lev = ch.results()
        clamped = np.clip(wild, -12, 51)
        wr, wl = qo.encode(s.tus[0], W, H, B, s.org[0], clamped[0], 1, s.cqo)
        for p in range(3):
            assert np.array_equal(lev[0][p], wl[p]) and np.array_equal(rec[0][p], wr[p])
    finally:
        ctx.set_qp_map(None)
        ctx.sync()
        d_map.free()
        ch.close()


@pytest.mark.parametrize("ctu,depths", [(16, 1), (16, 2), (32, 1), (32, 3), (64, 2), (64, 4)])
def test_aq_unit_qp_against_numpy(ctxs, ctu, depths):
    """(e) the unit map from the layer QPs: a unit inside a CU at depth D reads layer min(D, depths - 1), unit (x / part, y / part).
    The picture's right and lower edges cut a CTU; depths beyond the last layer are clamped."""
    ctx = ctxs[8]
    w, h, n = 152, 88, 2
    g = capi.aq_layout(w, h, ctu, depths)
    rng = np.random.default_rng(ctu * 10 + depths)
    layer = rng.integers(-12, 52, (n, g.total)).astype(np.int8)
    depth = rng.integers(0, 5, (n, h // 4, w // 4)).astype(np.uint8)
    want = np.zeros((n, h // 4, w // 4), np.int8)
    for i in range(n):
        for uy in range(h // 4):
            for ux in range(w // 4):
                d = min(int(depth[i, uy, ux]), depths - 1)
                part = ctu >> d
                want[i, uy, ux] = layer[i, g.first[d] + (4 * uy // part) * g.nx[d] + 4 * ux // part]
    d_layer, d_depth, d_qp = ctx.to_device(layer), ctx.to_device(depth), ctx.alloc(want.size).zero()
    try:
        ctx.aq_unit_qp(n, w, h, ctu, depths, d_layer, d_depth, d_qp)
        ctx.sync()
        assert np.array_equal(d_qp.download(np.int8).reshape(want.shape), want)
    finally:
        for d in (d_layer, d_depth, d_qp):
            d.free()
