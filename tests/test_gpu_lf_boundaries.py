"""Loop filters that stop at slice and tile boundaries, on the device: hmx_sao_picture_multi_avail and
hmx_sao_stats_multi_avail against the per-sample rule of tests/sao_block_oracle.py (which tests/test_sao_block_oracle.py holds
against the literal restatement of processSaoBlock / calcSaoStatsBlock), and the lfx_* streams through
thevc_amd.decisions.decode_sequence against the reference decoder's pictures."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import sao_block_oracle as SB
from thevc_amd import decisions as D

HERE = os.path.dirname(os.path.abspath(__file__))
LFX = sorted(glob.glob(os.path.join(HERE, "golden", "lfx_*.npz")))
CONTROL = [f for f in LFX if f.endswith("_cross.npz")]
CLOSED = [f for f in LFX if f not in CONTROL]
ids = lambda fs: [os.path.basename(f)[:-4] for f in fs]


@pytest.fixture(scope="module", params=[8, 12])
def ctx16(request):
    from thevc_amd import capi
    c = capi.Context(bit_depth=request.param, ctu_size=16)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx8():
    from thevc_amd import capi
    c = capi.Context(bit_depth=8, ctu_size=16)
    yield c
    c.close()


def dev(ctx, planes, w, h, **kw):
    from thevc_amd import capi
    return capi.DevPicture(ctx, w, h, **kw).upload(planes)


def sao_avail(ctx, ins, prms, avails, w, h, out_kw=None):
    """ins: DevPictures; prms: one [3, n_lcu] record array per picture; avails: one byte array per picture -> host pictures"""
    from thevc_amd import capi
    n = len(ins)
    outs = [capi.DevPicture(ctx, w, h, **((out_kw or [{}] * n)[i])).zero() for i in range(n)]
    d_prm, d_av = ctx.to_device(np.stack(prms)), ctx.to_device(np.ascontiguousarray(np.stack(avails), np.uint8))
    try:
        ctx.sao_pictures_avail(ins, outs, w, h, d_prm, d_av)
        ctx.sync()
        return [o.download() for o in outs]
    finally:
        for o in outs:
            o.free()
        d_prm.free(), d_av.free()


def same(got, want):
    return all(np.array_equal(a, b) for a, b in zip(got, want))


# ---- application ---------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_sao_every_mask(ctx16):
    """3 x 3 CTUs of 16, samples at the range ends: every byte value on the centre CTU, every edge type on luma and chroma"""
    B = ctx16.bit_depth
    c = SB.all_masks_case(B)
    w, h = c["w"], c["h"]
    d_in = dev(ctx16, c["rec"], w, h)
    for j in range(4):
        sl = slice(256 * j, 256 * (j + 1))
        got = sao_avail(ctx16, [d_in] * 256, c["prm"][sl], c["avail"][sl], w, h)
        for m in range(256):
            want = SB.apply_rule(c["rec"], c["prm"][256 * j + m], w, h, B, c["ctu"], c["avail"][256 * j + m])
            assert same(got[m], want), (j, m)
    d_in.free()


@pytest.mark.gpu
def test_sao_cut_ctus_unaligned_three_pictures(ctx8):
    """40x24 with CTU 16 (cut CTUs on both edges), three pictures in one call, each with its own parameters and bytes, on
    planes with margins, odd strides and addresses that are not dword-aligned"""
    c = SB.odd_case()
    w, h = c["w"], c["h"]
    shapes = [dict(mx=16, my=8), dict(pad=1), dict(skew=1, pad=1, mx=8, my=8)]
    ins = [dev(ctx8, p["rec"], w, h, **kw) for p, kw in zip(c["pics"], shapes)]
    got = sao_avail(ctx8, ins, [p["prm"] for p in c["pics"]], [p["avail"] for p in c["pics"]], w, h, out_kw=shapes[::-1])
    for i, p in enumerate(c["pics"]):
        assert same(got[i], SB.apply_rule(p["rec"], p["prm"], w, h, c["B"], c["ctu"], p["avail"])), i
    assert not same(got[0], SB.apply_rule(c["pics"][0]["rec"], c["pics"][0]["prm"], w, h, c["B"], c["ctu"], D.lf_border_avail(w, h, 16)))
    for d in ins:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(48, 48), (40, 24)])
def test_sao_geometry_mask_is_the_existing_entry(ctx16, w, h):
    """a mask built from the picture's geometry alone: bit for bit what hmx_sao_picture_multi gives"""
    from extreme_inputs import sao_edge_content
    from thevc_amd import capi
    B = ctx16.bit_depth
    rng = np.random.default_rng(w + B)
    n_lcu = -(-w // 16) * -(-h // 16)
    pics = [sao_edge_content(rng, w, h, B) for _ in range(3)]
    prms = [SB.random_params(rng, n_lcu) for _ in range(3)]
    ins = [dev(ctx16, p, w, h) for p in pics]
    outs = [capi.DevPicture(ctx16, w, h).zero() for _ in range(3)]
    d_prm = ctx16.to_device(np.stack(prms))
    ctx16.sao_pictures(ins, outs, w, h, d_prm)
    ctx16.sync()
    want = [o.download() for o in outs]
    got = sao_avail(ctx16, ins, prms, [D.lf_border_avail(w, h, 16)] * 3, w, h)
    for i in range(3):
        assert same(got[i], want[i]), i
        assert same(got[i], SB.apply_rule(pics[i], prms[i], w, h, B, 16, D.lf_border_avail(w, h, 16))), i
    for d in ins + outs:
        d.free()
    d_prm.free()


# ---- statistics ----------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_stats_every_mask(ctx16):
    B = ctx16.bit_depth
    c = SB.all_masks_case(B)
    w, h = c["w"], c["h"]
    d_org, d_rec = dev(ctx16, c["org"], w, h), dev(ctx16, c["rec"], w, h)
    got = ctx16.sao_stats([d_org] * 256, [d_rec] * 256, w, h, avail=c["avail"][:256]).astype(np.int64)
    for m in range(256):
        assert np.array_equal(got[m], SB.stats_rule(c["org"], c["rec"], w, h, c["ctu"], B, c["avail"][m])), m
    d_org.free(), d_rec.free()


@pytest.mark.gpu
def test_stats_cut_ctus_unaligned_three_pictures(ctx8):
    c = SB.odd_case()
    w, h = c["w"], c["h"]
    shapes = [dict(mx=16, my=8), dict(pad=1), dict(skew=1, pad=1, mx=8, my=8)]
    do = [dev(ctx8, p["org"], w, h, **kw) for p, kw in zip(c["pics"], shapes)]
    dr = [dev(ctx8, p["rec"], w, h, **kw) for p, kw in zip(c["pics"], shapes[::-1])]
    got = ctx8.sao_stats(do, dr, w, h, avail=np.stack([p["avail"] for p in c["pics"]])).astype(np.int64)
    for i, p in enumerate(c["pics"]):
        assert np.array_equal(got[i], SB.stats_rule(p["org"], p["rec"], w, h, c["ctu"], c["B"], p["avail"])), i
    for d in do + dr:
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(48, 48), (40, 24)])
def test_stats_geometry_mask_is_the_existing_entry(ctx16, w, h):
    from extreme_inputs import sao_edge_content
    B = ctx16.bit_depth
    rng = np.random.default_rng(w + 2 * B)
    org, rec = sao_edge_content(rng, w, h, B), sao_edge_content(rng, w, h, B)
    do, dr = dev(ctx16, org, w, h), dev(ctx16, rec, w, h)
    geo = D.lf_border_avail(w, h, 16)
    got = ctx16.sao_stats([do], [dr], w, h, avail=geo[None, :])
    assert np.array_equal(got, ctx16.sao_stats([do], [dr], w, h, lcu_based=False))
    assert np.array_equal(got[0].astype(np.int64), SB.stats_rule(org, rec, w, h, 16, B, geo))
    do.free(), dr.free()


@pytest.mark.gpu
def test_stats_ctu64_two_waves(ctx16):
    """CTU 64 (a thread walks 16 rows of a strip, two waves per workgroup): 136x72, a random byte on every CTU"""
    from extreme_inputs import sao_edge_content
    from thevc_amd import capi
    B, w, h = ctx16.bit_depth, 136, 72
    rng = np.random.default_rng(64 + B)
    org, rec = sao_edge_content(rng, w, h, B), sao_edge_content(rng, w, h, B)
    avail = rng.integers(0, 256, (1, 6)).astype(np.uint8)
    prm = SB.random_params(rng, 6, (0, 1, 2, 3, 4))
    c = capi.Context(bit_depth=B, ctu_size=64)
    try:
        do, dr = dev(c, org, w, h), dev(c, rec, w, h)
        got = c.sao_stats([do], [dr], w, h, avail=avail).astype(np.int64)
        assert np.array_equal(got[0], SB.stats_rule(org, rec, w, h, 64, B, avail[0]))
        assert same(sao_avail(c, [dr], [prm], [avail[0]], w, h)[0], SB.apply_rule(rec, prm, w, h, B, 64, avail[0]))
    finally:
        c.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals(ctx8):
    """each HMX_ERR_ARG of the two entries, with nothing launched: the outputs keep their sentinel"""
    from thevc_amd import capi
    L, w, h = capi.lib(), 40, 24
    c = SB.odd_case()
    p = c["pics"][0]
    din, dorg = dev(ctx8, p["rec"], w, h), dev(ctx8, p["org"], w, h)
    sentinel = [np.full_like(a, 0x5A5) for a in p["rec"]]
    dout = dev(ctx8, sentinel, w, h)
    d_prm, d_av = ctx8.to_device(p["prm"]), ctx8.to_device(p["avail"])
    stat = ctx8.to_device(np.full(3 * 6 * SB.BINS * 2, -0x5A5A5A5A, np.int32))
    pi, po, pg, bad_plane = din.as_pic(), dout.as_pic(), dorg.as_pic(), capi.Pic()
    R = C.byref
    good = (ctx8.h, 1, R(pi), R(po), w, h, d_prm.ptr, 6, d_av.ptr)
    cases = [(None,) + good[1:], good[:2] + (None,) + good[3:], good[:3] + (None,) + good[4:], good[:6] + (None,) + good[7:], good[:8] + (None,),
             good[:2] + (R(bad_plane),) + good[3:], good[:3] + (R(bad_plane),) + good[4:], good[:1] + (0,) + good[2:], good[:1] + (-1,) + good[2:],
             good[:1] + (65536,) + good[2:], good[:4] + (0,) + good[5:], good[:4] + (41,) + good[5:], good[:5] + (-24,) + good[6:], good[:5] + (23,) + good[6:],
             good[:7] + (5,) + good[8:], good[:7] + (9,) + good[8:], good[:3] + (R(pi),) + good[4:]]
    for args in cases:
        assert L.hmx_sao_picture_multi_avail(*args) == -1, args[1:]
        if args[0] is not None:
            assert L.hmx_last_error(ctx8.h).decode()
    sgood = (ctx8.h, 1, R(pg), R(pi), w, h, d_av.ptr, stat.ptr)
    scases = [(None,) + sgood[1:], sgood[:2] + (None,) + sgood[3:], sgood[:3] + (None,) + sgood[4:], sgood[:6] + (None,) + sgood[7:], sgood[:7] + (None,),
              sgood[:2] + (R(bad_plane),) + sgood[3:], sgood[:1] + (0,) + sgood[2:], sgood[:1] + (-1,) + sgood[2:], sgood[:4] + (0,) + sgood[5:],
              sgood[:4] + (36,) + sgood[5:], sgood[:5] + (-8,) + sgood[6:], sgood[:5] + (20,) + sgood[6:]]
    for args in scases:
        assert L.hmx_sao_stats_multi_avail(*args) == -1, args[1:]
    ctx8.sync()
    assert same(dout.download(), sentinel), "a refused call wrote to the output picture"
    assert (stat.download(np.int32) == -0x5A5A5A5A).all(), "a refused call wrote statistics"
    assert L.hmx_sao_picture_multi_avail(*good) == 0 and L.hmx_sao_stats_multi_avail(*sgood) == 0
    ctx8.sync()
    assert same(dout.download(), SB.apply_rule(p["rec"], p["prm"], w, h, 8, 16, p["avail"]))
    assert np.array_equal(stat.download(np.int32).reshape(3, 6, SB.BINS, 2), SB.stats_rule(p["org"], p["rec"], w, h, 16, 8, p["avail"]))
    for d in (din, dorg, dout, d_prm, d_av, stat):
        d.free()


# ---- streams -------------------------------------------------------------------------------------------------------------------

def _decode(path, forget=False):
    pics = list(D.load_pictures(path))
    if forget:  # the loop filters of a decoder without the feature: the mask of the geometry, every edge (the block path keeps its layout)
        pics = [dict(p, slice_id=None, tile_id=None, lf_cross_slice=None, lf_cross_tile=True) for p in pics]
    return pics, D.decode_sequence(pics)


@pytest.mark.gpu
@pytest.mark.parametrize("path", CLOSED, ids=ids(CLOSED))
def test_streams_with_closed_boundaries(path):
    pics, out = _decode(path)
    for p, got in zip(pics, out):
        for k in range(3):
            bad = np.argwhere(got[k] != p["rec"][k])
            assert not len(bad), (os.path.basename(path), "poc", p["poc"], "plane", k, "first mismatch (y, x)", bad[0].tolist(), len(bad))


@pytest.mark.gpu
def test_control_stream_takes_the_existing_entries(monkeypatch):
    """fixture (e): several slices, both flags 1 -- every bit inside the picture is set and the driver must not need the new entry"""
    from thevc_amd import capi

    def refuse(*a, **k):
        raise AssertionError("the availability entry was called for a picture whose boundaries are all open")

    monkeypatch.setattr(capi.Context, "sao_pictures_avail", refuse)
    pics, out = _decode(CONTROL[0])
    for p, got in zip(pics, out):
        assert same(got, p["rec"]), p["poc"]


@pytest.mark.gpu
def test_fixture_power_on_the_device():
    """a fixture with closed boundaries, decoded with the mask of the geometry and the unmasked edges, is NOT the reference"""
    pics, out = _decode(CLOSED[0], forget=True)
    assert any(not same(got, p["rec"]) for p, got in zip(pics, out))
