"""tests/golden/aq_intra_stream.npz on the device: all-intra pictures the reference encoder coded under --AdaptiveQP=1.  The
whole-picture chain with the fixture's unit map decodes the reference decoder's pictures and encodes the levels the reference
encoder wrote; and the map itself comes out of the device path originals -> hmx_aq_activity_multi -> hmx_aq_qp_map_multi ->
hmx_aq_unit_qp_multi with nothing downloaded in between."""
import ctypes as C
import os

import numpy as np
import pytest

import qp_map_oracle as qo
from thevc_amd import capi

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aq_intra_stream.npz")
CLIPS = qo.load_aq_intra_stream(FIXTURE)


class Clip:
    """One clip on the device: plans, level buffers in the reference's layout, reconstruction planes"""

    def __init__(self, cfg, pics):
        self.cfg, self.pics, self.n = cfg, pics, len(pics)
        p0 = pics[0]
        self.w, self.h, self.B, self.ctu = p0["w"], p0["h"], p0["B"], p0["ctu"]
        assert all(p["qp"] == p0["qp"] for p in pics)
        self.ctx = ctx = capi.Context(bit_depth=self.B, ctu_size=self.ctu)
        self.pp = capi.PicParam(self.w, self.h, p0["qp"], 0, capi.I_SLICE, 1)
        self.plans = [ctx.intra_plan(np.ascontiguousarray(p["tus"], capi.TU_DTYPE), self.pp) for p in pics]
        self.parr = (C.c_void_p * self.n)(*[p.value for p in self.plans])
        self.d_rec = [capi.DevPicture(ctx, self.w, self.h).zero() for _ in pics]
        self.d_org = [capi.DevPicture(ctx, self.w, self.h).upload(p["org"]) for p in pics]
        self.d_lev = [capi.DevLevelsZ(ctx, self.w, self.h, self.ctu) for _ in pics]
        for d, p in zip(self.d_lev, pics):
            for k in range(3):
                assert d.elems[k] == len(p["lev"][k])
        self.maps = np.stack([p["qp_map"] for p in pics])

    def arr(self, lst, T):
        return (T * self.n)(*[x.as_pic() for x in lst])

    def close(self):
        L = capi.lib()
        self.ctx.set_qp_map(None)
        self.ctx.sync()
        for pl in self.plans:
            L.hmx_intra_plan_destroy(self.ctx.h, pl)
        self.ctx.close()


@pytest.fixture(scope="module", params=range(len(CLIPS)), ids=[f"{c['B']}bit_ctu{c['ctu']}" for c, _ in CLIPS])
def clip(request):
    c = Clip(*CLIPS[request.param])
    yield c
    c.close()


def test_decode_with_the_map_gives_the_reference_decoders_pictures(clip):
    ctx, L = clip.ctx, capi.lib()
    d_map = ctx.to_device(clip.maps)
    for d, p in zip(clip.d_lev, clip.pics):
        for k in range(3):
            d.bufs[k].upload(np.ascontiguousarray(p["lev"][k], np.int32))
    for d in clip.d_rec:
        d.zero()
    ctx.set_qp_map(d_map, clip.n)
    ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, clip.parr, clip.n, clip.arr(clip.d_rec, capi.Pic), clip.arr(clip.d_lev, capi.Levels)))
    ctx.sync()
    for d, p in zip(clip.d_rec, clip.pics):
        got = d.download()
        for k in range(3):
            assert np.array_equal(got[k], p["rec"][k]), (p["poc"], k)
    # without the map the call decodes another picture: the fixture needs the feature
    ctx.set_qp_map(None)
    ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, clip.parr, clip.n, clip.arr(clip.d_rec, capi.Pic), clip.arr(clip.d_lev, capi.Levels)))
    ctx.sync()
    for d, p in zip(clip.d_rec, clip.pics):
        got = d.download()
        assert any(not np.array_equal(got[k], p["rec"][k]) for k in range(3)), p["poc"]
    d_map.free()


def test_encode_with_the_map_gives_the_levels_the_reference_encoder_wrote(clip):
    """The reference's xQuant shifts by the slice's base QP (hmx_set_qp_map_base) and scales by the block's: both are needed"""
    ctx, L = clip.ctx, capi.lib()
    d_map = ctx.to_device(clip.maps)
    for d in clip.d_rec + clip.d_lev:
        d.zero()
    ctx.set_qp_map(d_map, clip.n)
    ctx.set_qp_map_base(clip.pics[0]["qp"])
    try:
        ctx._chk(L.hmx_frame_intra_encode_multi(ctx.h, clip.parr, clip.n, clip.arr(clip.d_org, capi.Pic), clip.arr(clip.d_rec, capi.Pic),
                                                clip.arr(clip.d_lev, capi.Levels)))
        ctx.sync()
    finally:
        ctx.set_qp_map_base(None)
        ctx.set_qp_map(None)
    for dl, dr, p in zip(clip.d_lev, clip.d_rec, clip.pics):
        rec = dr.download()
        for k in range(3):
            assert np.array_equal(dl.bufs[k].download(np.int32), p["lev"][k]), ("levels", p["poc"], k)
            assert np.array_equal(rec[k], p["rec"][k]), ("reconstruction", p["poc"], k)
    d_map.free()


def test_originals_to_pictures_on_the_device(clip):
    """originals -> activities -> layer QPs -> unit map (with the fixture's CU depths) -> decode, no download in between; then the
    unit map is the fixture's and the pictures are the reference decoder's"""
    ctx, L, cfg = clip.ctx, capi.lib(), clip.cfg
    w, h, n, ctu, depths = clip.w, clip.h, clip.n, clip.ctu, cfg["k"] + 1
    g = capi.aq_layout(w, h, ctu, depths)
    d_act, d_avg, d_layer = ctx.alloc(8 * n * g.total), ctx.alloc(8 * n * depths), ctx.alloc(n * g.total)
    d_depth = ctx.to_device(np.stack([p["cu_depth"] for p in clip.pics]))
    d_map = ctx.alloc(n * (h // 4) * (w // 4)).zero()
    for d, p in zip(clip.d_lev, clip.pics):
        for k in range(3):
            d.bufs[k].upload(np.ascontiguousarray(p["lev"][k], np.int32))
    for d in clip.d_rec:
        d.zero()
    ctx._chk(L.hmx_aq_activity_multi(ctx.h, n, clip.arr(clip.d_org, capi.Pic), w, h, ctu, depths, d_act.ptr, d_avg.ptr))
    ctx.aq_qp_map(n, w, h, ctu, depths, d_act, d_avg, [p["qp"] for p in clip.pics], cfg["range"], 6 * (clip.B - 8), out=d_layer)
    ctx.aq_unit_qp(n, w, h, ctu, depths, d_layer, d_depth, d_map)
    ctx.set_qp_map(d_map, n)
    ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, clip.parr, n, clip.arr(clip.d_rec, capi.Pic), clip.arr(clip.d_lev, capi.Levels)))
    ctx.sync()
    ctx.set_qp_map(None)
    assert np.array_equal(d_map.download(np.int8).reshape(clip.maps.shape), clip.maps)
    for d, p in zip(clip.d_rec, clip.pics):
        got = d.download()
        for k in range(3):
            assert np.array_equal(got[k], p["rec"][k]), (p["poc"], k)
    for d in (d_act, d_avg, d_layer, d_depth, d_map):
        d.free()
