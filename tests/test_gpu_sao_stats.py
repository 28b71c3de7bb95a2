"""hmx_sao_stats / hmx_sao_stats_multi (the encoder's SAO statistics, include/hmx.h) against the restatement in
tests/sao_stats_oracle.py, bin for bin."""
import ctypes as C
import os

import numpy as np
import pytest

from sao_stats_oracle import BINS, stats_vec
from test_sao_stats import SIZES, random_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module", params=[8, 10])
def sctx(request):
    from thevc_amd import capi
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sctx32():
    from thevc_amd import capi
    c = capi.Context(bit_depth=10, ctu_size=32)
    yield c
    c.close()


def upload(ctx, planes, w, h, **kw):
    from thevc_amd import capi
    return capi.DevPicture(ctx, w, h, **kw).upload(planes)


def gpu_stats(ctx, orgs, recs, w, h, lcu_based, **kw):
    """orgs / recs: lists of host pictures (three planes); returns int64 [n, 3, n_lcu, 52, 2]"""
    do = [upload(ctx, o, w, h, **kw) for o in orgs]
    dr = [upload(ctx, r, w, h, **kw) for r in recs]
    try:
        return ctx.sao_stats(do, dr, w, h, lcu_based).astype(np.int64)
    finally:
        for p in do + dr:
            p.free()


@pytest.mark.gpu
@pytest.mark.parametrize("lcu_based", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_random(sctx, w, h, lcu_based):
    B = sctx.bit_depth
    org, rec = random_pair(np.random.default_rng(w + h + B + lcu_based), w, h, B)
    got = gpu_stats(sctx, [org], [rec], w, h, lcu_based)
    assert np.array_equal(got[0], stats_vec(org, rec, w, h, 64, B, lcu_based))


@pytest.mark.gpu
@pytest.mark.parametrize("lcu_based", [0, 1])
@pytest.mark.parametrize("w,h", SIZES)
def test_random_ctu32(sctx32, w, h, lcu_based):
    org, rec = random_pair(np.random.default_rng(w * h + lcu_based), w, h, 10)
    got = gpu_stats(sctx32, [org], [rec], w, h, lcu_based)
    assert np.array_equal(got[0], stats_vec(org, rec, w, h, 32, 10, lcu_based))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stream_intra_main_q29_rdoq0.npz", "stream_lowdelay_P_main_q28_rdoq0.npz", "stream_intra_he10_q35_rdoq0.npz"])
def test_encoder_pictures(sctx, name):
    """the reference encoder's own input and reconstruction pairs"""
    from thevc_amd.decisions import load_pictures
    pics = [p for p in load_pictures(os.path.join(GOLDEN, name)) if p["org"] is not None]
    assert pics
    if pics[0]["B"] != sctx.bit_depth:
        return  # the fixture's other context runs it
    for p in pics:
        w, h = p["w"], p["h"]
        for lcu_based in (0, 1):
            got = gpu_stats(sctx, [p["org"]], [p["rec"]], w, h, lcu_based)
            assert np.array_equal(got[0], stats_vec(p["org"], p["rec"], w, h, p["ctu"], p["B"], lcu_based)), (name, p["poc"])


@pytest.mark.gpu
def test_multi_margins_pad_skew(sctx):
    """distinct pictures in one call, each with its own planes: margins, odd strides, planes that are not dword-aligned"""
    B, w, h = sctx.bit_depth, 200, 136
    rng = np.random.default_rng(7 + B)
    pairs = [random_pair(rng, w, h, B) for _ in range(3)]
    shapes = [dict(mx=32, my=16), dict(pad=1), dict(skew=1, pad=1, mx=8, my=8)]
    do = [upload(sctx, o, w, h, **kw) for (o, _), kw in zip(pairs, shapes)]
    dr = [upload(sctx, r, w, h, **kw) for (_, r), kw in zip(pairs, shapes[::-1])]
    got = sctx.sao_stats(do, dr, w, h, True).astype(np.int64)
    for i, (o, r) in enumerate(pairs):
        assert np.array_equal(got[i], stats_vec(o, r, w, h, 64, B, 1)), i
    for p in do + dr:
        p.free()


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n", [(1920, 1080, 3), (3840, 2160, 2)])
def test_full_size(sctx, w, h, n):
    B = sctx.bit_depth
    rng = np.random.default_rng(w + n + B)
    pairs = [random_pair(rng, w, h, B) for _ in range(n)]
    got = gpu_stats(sctx, [o for o, _ in pairs], [r for _, r in pairs], w, h, True)
    for i, (o, r) in enumerate(pairs):
        assert np.array_equal(got[i], stats_vec(o, r, w, h, 64, B, 1)), i


@pytest.mark.gpu
@pytest.mark.parametrize("lcu_based", [0, 1])
def test_extreme_values(sctx, lcu_based):
    """rec = 0 and org = 2^B - 1, and the other way round: every sum at its largest magnitude"""
    B, w, h = sctx.bit_depth, 136, 72
    mx = (1 << B) - 1
    zero = [np.zeros((ph, pw), np.int16) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
    full = [np.full_like(z, mx) for z in zero]
    got = gpu_stats(sctx, [full, zero], [zero, full], w, h, lcu_based)
    assert np.array_equal(got[0], stats_vec(full, zero, w, h, 64, B, lcu_based))
    assert np.array_equal(got[1], stats_vec(zero, full, w, h, 64, B, lcu_based))
    assert got[0][..., 0].max() == (64 * 64 if not lcu_based else 59 * 60) * mx  # the whole first luma CTU in band 1


@pytest.mark.gpu
def test_org_is_rec_and_repeatable(sctx):
    from thevc_amd import capi
    B, w, h = sctx.bit_depth, 200, 136
    org, rec = random_pair(np.random.default_rng(3), w, h, B)
    d = upload(sctx, rec, w, h)
    same = sctx.sao_stats([d], [d], w, h, True).astype(np.int64)
    assert not same[..., 0].any()
    assert np.array_equal(same[0], stats_vec(rec, rec, w, h, 64, B, 1))
    do = upload(sctx, org, w, h)
    runs = [sctx.sao_stats([do], [d], w, h, True) for _ in range(3)]
    assert all(np.array_equal(runs[0], r) for r in runs[1:])
    d.free(), do.free()
    assert capi.SAO_STAT_BINS == BINS


@pytest.mark.gpu
def test_every_bin_written(sctx):
    """a d_out full of a sentinel comes back with no sentinel left (bins that stay zero are written too)"""
    from thevc_amd import capi
    L, B, w, h = capi.lib(), sctx.bit_depth, 136, 72
    org, rec = random_pair(np.random.default_rng(5), w, h, B)
    do, dr = upload(sctx, org, w, h), upload(sctx, rec, w, h)
    n_lcu = 3 * 2
    out = sctx.to_device(np.full(2 * 3 * n_lcu * BINS * 2, -0x5A5A5A5A, np.int32))
    o, r = (capi.Pic * 2)(do.as_pic(), do.as_pic()), (capi.Pic * 2)(dr.as_pic(), dr.as_pic())
    sctx._chk(L.hmx_sao_stats_multi(sctx.h, 2, o, r, w, h, 1, out.ptr))
    sctx.sync()
    got = out.download(np.int32).reshape(2, 3, n_lcu, BINS, 2).astype(np.int64)
    want = stats_vec(org, rec, w, h, 64, B, 1)
    assert np.array_equal(got[0], want) and np.array_equal(got[1], want)
    out.free(), do.free(), dr.free()


@pytest.mark.gpu
def test_arguments(sctx):
    from thevc_amd import capi
    L, w, h = capi.lib(), 136, 72
    org, rec = random_pair(np.random.default_rng(9), w, h, sctx.bit_depth)
    do, dr = upload(sctx, org, w, h), upload(sctx, rec, w, h)
    out = sctx.alloc(3 * 6 * BINS * 8)
    po, pr = do.as_pic(), dr.as_pic()
    bad_plane = capi.Pic()
    cases = [
        (None, 1, C.byref(po), C.byref(pr), w, h, 1, out.ptr),
        (sctx.h, 1, None, C.byref(pr), w, h, 1, out.ptr),
        (sctx.h, 1, C.byref(po), None, w, h, 1, out.ptr),
        (sctx.h, 1, C.byref(po), C.byref(pr), w, h, 1, None),
        (sctx.h, 1, C.byref(bad_plane), C.byref(pr), w, h, 1, out.ptr),
        (sctx.h, 0, C.byref(po), C.byref(pr), w, h, 1, out.ptr),
        (sctx.h, -1, C.byref(po), C.byref(pr), w, h, 1, out.ptr),
        (sctx.h, 1, C.byref(po), C.byref(pr), 0, h, 1, out.ptr),
        (sctx.h, 1, C.byref(po), C.byref(pr), w, -8, 1, out.ptr),
        (sctx.h, 1, C.byref(po), C.byref(pr), 132, h, 1, out.ptr),
        (sctx.h, 1, C.byref(po), C.byref(pr), w, 68, 1, out.ptr),
    ]
    for args in cases:
        assert L.hmx_sao_stats_multi(*args) == -1, args[1:]
        if args[0] is not None:
            assert lib_error(sctx)
    assert L.hmx_sao_stats(sctx.h, None, C.byref(pr), w, h, 1, out.ptr) == -1
    assert L.hmx_sao_stats(sctx.h, C.byref(po), C.byref(pr), w, 68, 1, out.ptr) == -1
    assert L.hmx_sao_stats(sctx.h, C.byref(po), C.byref(pr), w, h, 1, out.ptr) == 0
    sctx.sync()
    got = out.download(np.int32).reshape(3, 6, BINS, 2).astype(np.int64)
    assert np.array_equal(got, stats_vec(org, rec, w, h, 64, sctx.bit_depth, 1))
    out.free(), do.free(), dr.free()


def lib_error(ctx):
    from thevc_amd import capi
    return capi.lib().hmx_last_error(ctx.h).decode()
