"""Adaptive QP on the GPU (hmx_aq_activity_multi, hmx_aq_qp_map_multi, the C++ mirror) through the C-ABI: activities and layer
averages bit for bit against tests/aq_oracle.py (compared as uint64), QP maps against it, the device's threshold count against the
host's logarithm on the thresholds' neighbours, and the QPs against the streams the reference encoder wrote
(tests/golden/aq_stream.npz).

Device double division is the compiler's full sequence (v_div_scale, v_rcp, v_fma, v_div_fmas, v_div_fixup); that it is correctly
rounded on the chip is what the bit comparisons here measure."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import aq_oracle as ao
from test_aq_oracle import CTUS, GOLDEN, KINDS, RANGES, SIZES, offset_pairs, picture
from thevc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (luma margin x, y, extra samples per row, samples the plane starts after its allocation).  The first two keep every row of
# every 8-sample strip on a 16-byte boundary (the vector loads); the others do not (odd strides, odd addresses).
LAYOUTS = [(0, 0, 0, 0), (16, 8, 0, 0), (16, 8, 0, 1), (6, 2, 3, 1), (0, 0, 1, 1), (10, 4, 8, 0), (2, 2, 5, 1)]


@pytest.fixture(scope="module")
def ctxs():
    c = {B: capi.Context(bit_depth=B) for B in (8, 10, 12)}
    yield c
    for v in c.values():
        v.close()


def device_picture(ctx, luma, layout, rng):
    """The luma plane inside margins full of other samples: a read outside the picture changes a sum"""
    h, w = luma.shape
    mx, my, pad, skew = layout
    d = capi.DevPicture(ctx, w, h, mx, my, pad=pad, skew=skew)
    flat = rng.integers(0, 1 << ctx.bit_depth, d.elems[0]).astype(np.int16)
    full = flat[skew:].reshape(h + 2 * my, d.strides[0])
    full[my:my + h, mx:mx + w] = luma
    d.bufs[0].upload(flat)
    return d


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def check_bits(got, want, what):
    got, want = bits(got), bits(want)
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (what, bad[:8].tolist(), got.ravel()[bad[:8]].tolist(), want.ravel()[bad[:8]].tolist())


@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("w,h", SIZES)
def test_activities_bit_exact(ctxs, B, w, h):
    """Every kind of content, one picture each, as ONE batch per (CTU size, depths); every picture its own layout"""
    ctx = ctxs[B]
    rng = np.random.default_rng(9000 + 7 * w + h + B)
    for ctu in CTUS:
        pics = [picture(w, h, B, kind, rng, part=ctu) for kind in KINDS]
        dev = [device_picture(ctx, p, LAYOUTS[(i + ctu // 16) % len(LAYOUTS)], rng) for i, p in enumerate(pics)]
        full = ao.legal_depths(ctu)[-1]
        want = [ao.preanalyze(p, ctu, full) for p in pics]
        for depths in ao.legal_depths(ctu):
            g = ao.Geom(w, h, ctu, depths)
            act, avg = ctx.aq_activity(dev, w, h, ctu, depths)
            check_bits(act, np.stack([a[:g.total] for a, _ in want]), (ctu, depths, "activities"))
            check_bits(avg, np.stack([v[:depths] for _, v in want]), (ctu, depths, "averages"))
        flat = KINDS.index("flat")
        assert (act[flat] == 1.0).all() and (avg[flat] == 1.0).all()
        for d in dev:
            d.free()


@pytest.mark.parametrize("n", [1, 3, 65])
def test_batches_of_distinct_pictures(ctxs, n):
    ctx, B, w, h = ctxs[10], 10, 72, 56
    rng = np.random.default_rng(9100 + n)
    pics = [picture(w, h, B, "texture" if i % 2 else "noise", rng) for i in range(n)]
    dev = [device_picture(ctx, p, LAYOUTS[i % len(LAYOUTS)], rng) for i, p in enumerate(pics)]
    for ctu, depths in ((64, 4), (32, 2), (16, 2)):
        want = [ao.preanalyze(p, ctu, depths) for p in pics]
        act, avg = ctx.aq_activity(dev, w, h, ctu, depths)
        check_bits(act, np.stack([a for a, _ in want]), (ctu, "activities"))
        check_bits(avg, np.stack([v for _, v in want]), (ctu, "averages"))
    # the scalar companion on the last picture
    g = ao.Geom(w, h, 16, 2)
    d_act, d_avg = ctx.alloc(8 * g.total), ctx.alloc(16)
    ctx._chk(capi.lib().hmx_aq_activity(ctx.h, C.byref(dev[-1].as_pic()), w, h, 16, 2, d_act.ptr, d_avg.ptr))
    ctx.sync()
    check_bits(d_act.download(np.float64), want[-1][0], "hmx_aq_activity")
    check_bits(d_avg.download(np.float64), want[-1][1], "hmx_aq_activity")
    # the ordered sums on their own, over activities that lie on the device
    d_avg.zero()
    ctx._chk(capi.lib().hmx_aq_average_multi(ctx.h, 1, w, h, 16, 2, d_act.ptr, d_avg.ptr))
    ctx.sync()
    check_bits(d_avg.download(np.float64), want[-1][1], "hmx_aq_average_multi")
    for d in dev + [d_act, d_avg]:
        d.free()


@pytest.mark.parametrize("qp_range", RANGES)
def test_qp_maps_vs_oracle(ctxs, qp_range):
    """Slice QP 0 and 51, and -10 at 10 bit (QpBDOffsetY 12), where the offsets of the larger ranges meet the lower clip"""
    rng = np.random.default_rng(9200 + qp_range)
    w, h = 136, 72
    clipped_low = clipped_high = 0
    for B, ctu, depths in ((8, 64, 4), (10, 32, 3), (10, 16, 1)):
        ctx, bd = ctxs[B], 6 * (B - 8)
        slice_qps = [0, 51, -10 if B == 10 else 30]
        pics = [picture(w, h, B, kind, rng) for kind in ("texture", "patch", "texture")]  # patch: offsets up to +range on slice QP 51
        dev = [device_picture(ctx, p, LAYOUTS[i + 1], rng) for i, p in enumerate(pics)]
        g = ao.Geom(w, h, ctu, depths)
        d_act, d_avg = ctx.alloc(8 * len(pics) * g.total), ctx.alloc(8 * len(pics) * depths)
        act, avg = ctx.aq_activity(dev, w, h, ctu, depths, d_act, d_avg)
        got = ctx.aq_qp_map(len(pics), w, h, ctu, depths, d_act, d_avg, slice_qps, qp_range, bd)
        for i, qp in enumerate(slice_qps):
            want = ao.qp_map(g, act[i], avg[i], qp, qp_range, bd)
            assert np.array_equal(got[i], want), (B, ctu, qp)
            raw = np.array([qp + ao.offset(act[i][u], avg[i][d], qp_range) for d in range(depths) for u in range(g.first[d], g.first[d] + g.nx[d] * g.ny[d])])
            clipped_low += int((raw < -bd).sum())
            clipped_high += int((raw > 51).sum())
        for d in dev + [d_act, d_avg]:
            d.free()
    assert clipped_high > 0 and clipped_low > 0  # both clips of Clip3 are reached in every range


@pytest.mark.parametrize("qp_range", RANGES)
def test_threshold_count_on_the_device(ctxs, qp_range):
    """10^5 random (activity, average) pairs and the pairs whose norm is a threshold or the double below it: one 8x8 picture
    per pair (one unit, one layer, so that every pair has its own average), the device's count against the host's logarithm"""
    ctx, L = ctxs[8], capi.lib()
    pairs, hit = offset_pairs(qp_range, np.random.default_rng(8300 + qp_range))
    assert hit >= qp_range
    want = np.array([ao.offset(a, v, qp_range) for a, v in pairs])
    assert want.min() < 0 < want.max()
    arr = np.array(pairs, np.float64)
    for lo in range(0, len(arr), 65535):
        part = arr[lo:lo + 65535]
        d_act, d_avg = ctx.to_device(part[:, 0]), ctx.to_device(part[:, 1])
        # QPs span -48 .. 51: from slice QP 51 every offset down to -99 is told apart, from -48 every offset up to 99
        for slice_qp in (51, -48):
            got = ctx.aq_qp_map(len(part), 8, 8, 16, 1, d_act, d_avg, [slice_qp] * len(part), qp_range, 48)
            ref = np.clip(slice_qp + want[lo:lo + 65535], -48, 51)
            assert np.array_equal(got[:, 0], ref), (slice_qp, np.flatnonzero(got[:, 0] != ref)[:8])
        d_act.free(), d_avg.free()


def test_recorded_streams(ctxs):
    """Every block of every recorded run: the set of QPs that reproduce the reference decoder's reconstruction contains the QP
    the library computes from the original"""
    z = np.load(GOLDEN)
    checked = 0
    for run in range(int(z["n_runs"])):
        B, k, r, ctu, slice_qp = [int(v) for v in z[f"run{run}_config"]]
        ctx, bd, depths = ctxs[B], 6 * (B - 8), k + 1
        org, blocks = z[f"run{run}_org"], z[f"run{run}_blocks"]
        n, h, w = org.shape
        rng = np.random.default_rng(9300 + run)
        dev = [device_picture(ctx, org[i], LAYOUTS[i % len(LAYOUTS)], rng) for i in range(n)]
        g = ao.Geom(w, h, ctu, depths)
        d_act, d_avg = ctx.alloc(8 * n * g.total), ctx.alloc(8 * n * depths)
        ctx.aq_activity(dev, w, h, ctu, depths, d_act, d_avg)
        slice_qps = [int(q) for q in z[f"run{run}_slice_qp"]]
        qp = ctx.aq_qp_map(n, w, h, ctu, depths, d_act, d_avg, slice_qps, r, bd)
        for pic, x, y, plane, cu_size, lo, mask in blocks.tolist():
            d = min(ctu.bit_length() - cu_size.bit_length(), depths - 1)
            u = g.first[d] + (y // g.part[d]) * g.nx[d] + x // g.part[d]
            got = int(qp[pic][u])
            assert lo <= got < lo + 64 and (mask >> (got - lo)) & 1, (run, pic, x, y, plane, cu_size, got)
            checked += 1
        for d in dev + [d_act, d_avg]:
            d.free()
    assert checked == int(z["n_blocks"])


def test_cpp_mirror(tmp_path):
    """hmx_hm::TEncPreanalyzer::xPreanalyze + TEncCu::xComputeQP (thevc_amd/host/hmx_hm.hpp) for every CU position and depth of one
    208x120 picture"""
    exe = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
    B, w, h, ctu, depths, slice_qp, qp_range = 10, 208, 120, 64, 3, 27, 6
    luma = picture(w, h, B, "texture", np.random.default_rng(9400))
    path = tmp_path / "aq.bin"
    with open(path, "wb") as f:
        f.write(np.array([B, w, h, ctu, depths, slice_qp, qp_range], np.int32).tobytes())
        f.write(np.ascontiguousarray(luma, np.int16).tobytes())
    lines = subprocess.run([exe, "aq", str(path)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(lines) == 5
    act, avg = ao.preanalyze(luma, ctu, depths)
    assert [int(v, 16) for v in lines[0].split()] == bits(avg).tolist()
    g = ao.Geom(w, h, ctu, depths)
    offsets = set()
    for depth in range(4):
        size = max(ctu >> depth, 8)
        want = [ao.compute_qp(g, act, avg, x, y, depth, slice_qp, qp_range, 6 * (B - 8)) for y in range(0, h, size) for x in range(0, w, size)]
        assert [int(v) for v in lines[1 + depth].split()] == want, depth
        offsets |= {q - slice_qp for q in want}
    assert len(offsets) >= 5  # the picture exercises the offsets, not one QP


def test_refusals(ctxs):
    ctx, L = ctxs[8], capi.lib()
    rng = np.random.default_rng(9500)
    w, h = 64, 64
    luma = picture(w, h, 8, "noise", rng)
    d = device_picture(ctx, luma, LAYOUTS[1], rng)
    pic = (capi.Pic * 1)(d.as_pic())
    bad = (capi.Pic * 1)(d.as_pic())
    bad[0].plane[0] = None
    g = ao.Geom(w, h, 64, 4)
    d_act, d_avg, d_qp = ctx.alloc(8 * g.total), ctx.alloc(8 * 4), ctx.alloc(g.total)
    sq = (C.c_int * 1)(30)
    want = ao.preanalyze(luma, 64, 4)
    before = d_act.zero().download(np.float64)

    def refused(rc, word):
        assert rc == -1 and word in L.hmx_last_error(ctx.h).decode(), (rc, L.hmx_last_error(ctx.h))

    def act(n=1, pics=pic, ww=w, hh=h, ctu=64, depths=4, a=d_act.ptr, v=d_avg.ptr):
        return L.hmx_aq_activity_multi(ctx.h, n, pics, ww, hh, ctu, depths, a, v)

    def qp(n=1, ww=w, hh=h, ctu=64, depths=4, a=d_act.ptr, v=d_avg.ptr, s=sq, r=6, bd=0, out=d_qp.ptr):
        return L.hmx_aq_qp_map_multi(ctx.h, n, ww, hh, ctu, depths, a, v, s, r, bd, out)

    def mean(n=1, ww=w, hh=h, ctu=64, depths=4, a=d_act.ptr, v=d_avg.ptr):
        return L.hmx_aq_average_multi(ctx.h, n, ww, hh, ctu, depths, a, v)

    refused(mean(a=None), "null")
    refused(mean(v=None), "null")
    refused(mean(n=0), "n_pics")
    refused(mean(ctu=48), "multiples of 8")
    refused(mean(ww=60), "multiples of 8")
    refused(act(pics=None), "null")
    refused(act(a=None), "null")
    refused(act(v=None), "null")
    refused(act(pics=bad), "null luma plane")
    refused(L.hmx_aq_activity(ctx.h, None, w, h, 64, 4, d_act.ptr, d_avg.ptr), "null")
    refused(qp(a=None), "null")
    refused(qp(v=None), "null")
    refused(qp(s=None), "null")
    refused(qp(out=None), "null")
    for n in (0, -1, 65536):
        refused(act(n=n), "n_pics")
        refused(qp(n=n), "n_pics")
    for kw in (dict(ctu=8), dict(ctu=48), dict(ctu=128), dict(depths=0), dict(depths=5), dict(ctu=32, depths=4), dict(ctu=16, depths=3), dict(ww=0), dict(hh=0),
               dict(ww=-64), dict(ww=60), dict(hh=68), dict(ww=16392), dict(hh=16392)):
        refused(act(**kw), "multiples of 8")
        refused(qp(**kw), "multiples of 8")
    for r in (0, -1, 65):
        refused(qp(r=r), "range")
    for bd in (-1, 49):
        refused(qp(bd=bd), "qp_bd_offset")
    for s, bd in ((52, 0), (-1, 0), (-13, 12)):
        refused(qp(s=(C.c_int * 1)(s), bd=bd), "slice_qp[0]")
    out = np.zeros(13, np.float64)
    assert L.hmx_aq_thresholds(0, out.ctypes.data) == -1 and L.hmx_aq_thresholds(65, out.ctypes.data) == -1 and L.hmx_aq_thresholds(6, None) == -1
    # nothing was launched, and the context still works
    ctx.sync()
    assert np.array_equal(d_act.download(np.float64), before)
    ctx._chk(act())
    ctx._chk(qp())
    ctx.sync()
    check_bits(d_act.download(np.float64), want[0], "after the refusals")
    assert np.array_equal(d_qp.download(np.int8), ao.qp_map(g, want[0], want[1], 30, 6, 0))
    for b in (d, d_act, d_avg, d_qp):
        b.free()
