"""hmx_batch_tz_search on the GPU against tests/tz_oracle.py, everything compared for equality: results, evaluation counts and
whole traces of the fixture set (tests/tz_fixture.py, which tests/test_tz_oracle.py proves to reach every branch), the trace
against the full search's cost map and against the pinned hmx_batch_subpel_cost, originals outside the sample range, 12 bit at
the range ends, the chain into hmx_batch_subpel_search without a download, a trace capacity below the count with guard words,
the pass cap, every refusal of the host, determinism, and xMotionEstimation with m_iFastSearch = 1 through the C++ host
mirror.  A 192 x 128 picture with margin 80 (the pictures of tests/test_gpu_me.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import me_oracle as mo
import test_gpu_me as tgm
import tz_fixture as tf
import tz_oracle as tzo
from thevc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
W, H, M = tf.W, tf.H, tf.M
assert (W, H, M) == (tgm.W, tgm.H, tgm.M)
ONES = 0xFFFFFFFF
CAP = 1024  # above every count of the fixture set (tests/test_tz_oracle.py asserts it)


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


_expected = {}


def expected(B, sc, max_passes=tzo.PASS_CAP):
    """The oracle's (result, trace, passes, labels) of every unit of a scene, computed once."""
    key = (B, sc.name, max_passes)
    if key not in _expected:
        _expected[key] = [tzo.search(sc.org, sc.refs[int(u["ref"])], (M, M), u, z, sc.lam, B, max_passes) for u, z in zip(sc.units, sc.tz)]
    return _expected[key]


@pytest.fixture(scope="module")
def staged(ctx):
    """The scenes' pictures on the device."""
    out = [(sc, tgm.Pictures(ctx, sc.refs, sc.org)) for sc in tf.scenes(ctx.bit_depth)]
    yield out
    for _, p in out:
        p.free()


def run(ctx, p, units, tz, lam, cap=CAP):
    return ctx.batch_tz_search(units, tz, p.refs, p.org, W, H, M, M, lam, want_trace=True, trace_cap=cap)


def rows(a):
    return [tuple(int(v) for v in r) for r in a]


def compare(got, want, label):
    res, counts, trace = got
    for i, (wres, wtrace, _, _) in enumerate(want):
        assert int(counts[i]) == len(wtrace), (label, i, int(counts[i]), len(wtrace))
        assert rows(trace[i][:len(wtrace)]) == wtrace, (label, i)
        assert rows(res[i:i + 1])[0] == wres, (label, i, res[i], wres)


# ---- 1. the fixture set: result, count and whole trace; the same results without a trace ----
def test_fixture_vs_oracle(ctx, staged):
    B = ctx.bit_depth
    t = tgm.make_textured(ctx)  # the textured scene is what test_gpu_me makes
    sc = tf.scenes(B)[0]
    assert sc.name == "textured" and np.array_equal(t.org_h, sc.org) and all(np.array_equal(a, b) for a, b in zip(t.full, sc.refs))
    t.free()
    for sc, p in staged:
        got = run(ctx, p, sc.units, sc.tz, sc.lam)
        compare(got, expected(B, sc), sc.name)
        plain = ctx.batch_tz_search(sc.units, sc.tz, p.refs, p.org, W, H, M, M, sc.lam)  # d_trace = d_trace_count = NULL
        assert plain.tobytes() == got[0].tobytes(), sc.name


# ---- 2. the trace against the full search's cost map and against the pinned hmx_batch_subpel_cost ----
def test_trace_vs_full_search(ctx, staged):
    B = ctx.bit_depth
    at_min = above = 0
    for sc, p in staged:
        res, counts, trace = run(ctx, p, sc.units, sc.tz, sc.lam)
        full, cmap, first = ctx.batch_fullpel_search(sc.units, p.refs, p.org, W, H, M, M, sc.lam, want_map=True)
        inside = 0
        for i, u in enumerate(sc.units):
            l, t, r, b = (int(u[k]) for k in ("left", "top", "right", "bottom"))
            m = cmap[first[i]:first[i + 1]].reshape(b - t + 1, r - l + 1)
            for (x, y, c) in rows(trace[i][:int(counts[i])]):
                if l <= x <= r and t <= y <= b:
                    assert c == int(m[y - t, x - l]), (sc.name, i, x, y)
                    inside += 1
            want = expected(B, sc)[i][0]
            if l <= want[0] <= r and t <= want[1] <= b:
                # TZ is greedy: a vector of the box never costs less than the box minimum.  (A vector OUTSIDE the box -- a zero
                # vector the walk adopted, or a point reached from it -- is no candidate of the full search and may cost less.)
                assert want[3] >= int(full[i]["cost"]), (sc.name, i)
                assert (int(res[i]["cost"]) == int(full[i]["cost"])) == (want[3] == int(full[i]["cost"]))
                at_min += want[3] == int(full[i]["cost"])
                above += want[3] > int(full[i]["cost"])
            else:
                assert "zero_outside_adopted" in expected(B, sc)[i][3], (sc.name, i)
        assert inside > 20 * len(sc.units) // 2
    assert at_min >= 1 and above >= 1  # it reaches the minimum somewhere (the smooth scene's units near the truth) and misses it elsewhere


def test_trace_vs_pinned_sad(ctx, staged):
    """lambda = 0 and sub_shift = 0: a trace cost is the SAD, which hmx_batch_subpel_cost (pinned on the compiled reference)
    gives for the integer vector -- also for the evaluated points outside the box."""
    for sc, p in staged[:2]:
        keep = np.flatnonzero(sc.units["sub_shift"] == 0)[:10]
        units, tz = sc.units[keep], sc.tz[keep]
        res, counts, trace = run(ctx, p, units, tz, 0)
        pts = [(i, x, y, c) for i in range(len(units)) for (x, y, c) in rows(trace[i][:int(counts[i])])[:40]]
        pus = np.zeros(len(pts), capi.PU_DTYPE)
        for k, (i, x, y, _) in enumerate(pts):
            u = units[i]
            pus[k] = (u["x"], u["y"], u["w"], u["h"], u["ref"], 255, 4 * x, 4 * y, 0, 0)
        offs = np.zeros((1, 2), np.int8)
        d_cost = ctx.alloc(4 * len(pus))
        ref_arr = (capi.Pic * len(p.refs))(*[r.as_pic() for r in p.refs])
        ctx._chk(capi.lib().hmx_batch_subpel_cost(ctx.h, pus.ctypes.data, len(pus), ref_arr, len(p.refs), C.byref(p.org.as_pic()), offs.ctypes.data, 1,
                                                 0, d_cost.ptr))
        ctx.sync()
        want = d_cost.download(np.uint32)
        d_cost.free()
        assert [c for (_, _, _, c) in pts] == [int(v) for v in want], sc.name
        assert len(pts) > 150 and len({c for (_, _, _, c) in pts}) > 50


# ---- 3. originals outside the sample range ----
def signed_case(ctx, refs, org, lam):
    B = ctx.bit_depth
    p = tgm.Pictures(ctx, refs, org)
    pairs = [tf.boxed(0, 0, 64, 64, 1, 0, 0, 0, 4), tf.boxed(0, 64, 64, 64, 0, 0, 3, 3, 64), tf.boxed(64, 0, 64, 64, 0, 0, -9, 2, 4),
             tf.boxed(64, 64, 64, 64, 1, 1, 0, 0, 64), tf.boxed(128, 32, 64, 64, 1, 0, 50, 50, 16), tf.boxed(0, 64, 64, 64, 0, 1, -77, 30, 64),
             tf.boxed(100, 20, 12, 24, 0, 0, 20, -20, 64), tf.boxed(20, 100, 4, 4, 1, 0, -40, 40, 32)]
    units, tz = np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs])
    want = [tzo.search(org, refs[int(u["ref"])], (M, M), u, z, lam, B) for u, z in zip(units, tz)]
    got = run(ctx, p, units, tz, lam)
    compare(got, want, "signed originals")
    p.free()
    return got[0]


def test_signed_originals(ctx):
    B = ctx.bit_depth
    rng = np.random.default_rng(1740 + B)
    org = rng.integers(-(1 << B), 1 << (B + 1), (H, W)).astype(np.int16)
    org[0:64, 0:64] = -(1 << B)               # the extremes, whole 64 x 64 blocks of them
    org[64:128, 0:64] = (1 << (B + 1)) - 1
    refs = [np.zeros((H + 2 * M, W + 2 * M), np.int16), np.full((H + 2 * M, W + 2 * M), (1 << B) - 1, np.int16)]
    res = signed_case(ctx, refs, org, 500000)
    assert int(res[0]["sad"]) == (64 * 64 * ((1 << B) + (1 << B) - 1)) >> (B - 8)  # |-2^B - (2^B - 1)| on every sample
    assert int(res[1]["sad"]) == (64 * 64 * ((1 << (B + 1)) - 1)) >> (B - 8)


def test_range_ends_12_bit():
    c = capi.Context(bit_depth=12)
    try:
        rng = np.random.default_rng(1752)
        org = rng.choice(np.array([-4096, 8191], np.int16), (H, W))  # both ends of [-2^B, 2^(B+1))
        refs = [rng.choice(np.array([0, 4095], np.int16), (H + 2 * M, W + 2 * M)) for _ in range(2)]
        res = signed_case(c, refs, org, 700000)
        assert len({int(r["sad"]) for r in res}) > 4
    finally:
        c.close()


# ---- 4. the chain into the sub-pel refinement, no download in between ----
def test_chain_into_subpel(ctx, staged):
    import subpel_oracle as so
    B = ctx.bit_depth
    outside = 0
    for sc, p in staged[:2]:
        units, tz = sc.units[:21], sc.tz[:21]
        d_int = ctx.batch_tz_search(units, tz, p.refs, p.org, W, H, M, M, sc.lam, keep_on_device=True)
        assert isinstance(d_int, capi.DevBuf)
        res = ctx.batch_subpel_search(units, d_int, p.refs, p.org, W, H, M, M, sc.lam, 1)
        d_int.free()
        for i, u in enumerate(units):
            ix, iy = expected(B, sc)[i][0][:2]
            if int(u["left"]) <= ix <= int(u["right"]) and int(u["top"]) <= iy <= int(u["bottom"]):
                want = so.refine_unit(sc.org, sc.refs[int(u["ref"])], (M, M), u, ix, iy, sc.lam, B, 1)[0]
            else:  # a zero vector adopted outside the box: the refinement's documented answer for a vector outside the box
                want = (4 * ix, 4 * iy, ONES, ONES)
                outside += 1
            assert rows(res[i:i + 1])[0] == want, (sc.name, i)
    assert outside >= 1


# ---- 5. a trace capacity below the count: full counts, the first entries, guard words untouched ----
def test_small_trace_cap(ctx, staged):
    B, cap, guard = ctx.bit_depth, 20, 0x5A5AA5A5
    sc, p = staged[1]
    n = len(sc.units)
    want = expected(B, sc)
    assert any(len(w[1]) < cap for w in want) and any(len(w[1]) > cap for w in want)
    d_trace = ctx.to_device(np.full(2 * (n * cap + 16), guard, np.uint32))  # every slice and 16 entries behind the last
    d_cnt = ctx.to_device(np.full(n + 4, guard, np.uint32))
    d_res = ctx.alloc(n * capi.ME_RESULT_DTYPE.itemsize)
    ref_arr = (capi.Pic * len(p.refs))(*[r.as_pic() for r in p.refs])
    ctx._chk(capi.lib().hmx_batch_tz_search(ctx.h, sc.units.ctypes.data, sc.tz.ctypes.data, n, ref_arr, len(p.refs), C.byref(p.org.as_pic()), W, H, M, M,
                                            sc.lam, d_res.ptr, d_trace.ptr, d_cnt.ptr, cap))
    ctx.sync()
    counts, raw = d_cnt.download(np.uint32), d_trace.download(np.uint32).reshape(-1, 2)
    res = d_res.download(capi.ME_RESULT_DTYPE, n)
    for d in (d_trace, d_cnt, d_res):
        d.free()
    assert [int(v) for v in counts[:n]] == [len(w[1]) for w in want] and all(int(v) == guard for v in counts[n:])
    trace = raw[:n * cap].copy().view(capi.TZ_POINT_DTYPE).reshape(n, cap)
    for i, w in enumerate(want):
        k = min(len(w[1]), cap)
        assert rows(trace[i][:k]) == w[1][:k], i
        assert np.all(raw[i * cap + k:(i + 1) * cap] == guard), i  # behind the unit's entries, inside its slice
        assert rows(res[i:i + 1])[0] == w[0], i
    assert np.all(raw[n * cap:] == guard)


# ---- 6. the pass cap ----
def test_pass_cap(ctx, staged):
    B = ctx.bit_depth
    sc, p = staged[1]
    full, one = expected(B, sc), expected(B, sc, 1)
    hit = [i for i, w in enumerate(full) if w[2] >= 2]
    assert hit and any(w[2] <= 1 for w in full)
    ctx.set_option("HMX_TZ_MAX_PASSES", 1)
    try:
        got = run(ctx, p, sc.units, sc.tz, sc.lam)
    finally:
        ctx.set_option("HMX_TZ_MAX_PASSES", None)
    compare(got, one, "one pass")  # the neighbours of the capped units are the full walk's
    for i, w in enumerate(full):
        if i in hit:
            assert rows(got[0][i:i + 1])[0][2:] == (ONES, ONES) and one[i][1] == w[1][:len(one[i][1])] and len(one[i][1]) < len(w[1])
        else:
            assert one[i] == w
    compare(run(ctx, p, sc.units, sc.tz, sc.lam), full, "cap restored")


# ---- 7. refusals ----
def test_host_validation(ctx, staged):
    sc, p = staged[0]
    L = capi.lib()
    good_u, good_z = tf.boxed(64, 32, 16, 16, 0, 0, 0, 0, 4)
    units0 = np.concatenate([good_u, good_u])
    tz0 = np.concatenate([good_z, good_z])
    sentinel = np.full(6, 0x5A5A5A5A, np.uint32)
    ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in p.refs])
    d_trace, d_cnt = ctx.alloc(2 * 8 * 8), ctx.alloc(8)

    def call(msg, units=units0, tz=tz0, n=2, refs=ref_arr, n_refs=2, org=C.byref(p.org.as_pic()), res=True, trace=None, cnt=None, cap=0, named=True):
        d_res = ctx.to_device(sentinel)
        rc = L.hmx_batch_tz_search(ctx.h, units.ctypes.data if units is not None else None, tz.ctypes.data if tz is not None else None, n, refs,
                                   n_refs, org, W, H, M, M, 0, d_res.ptr if res else None, trace, cnt, cap)
        err = L.hmx_last_error(ctx.h).decode()
        assert rc == -1, (msg, rc)  # HMX_ERR_ARG
        assert msg in err and (not named or "unit 1" in err), (msg, err)
        ctx.sync()
        assert np.array_equal(d_res.download(np.uint32), sentinel), msg  # nothing was launched
        d_res.free()

    def bad(msg, **kw):
        u, z = units0.copy(), tz0.copy()
        for k, v in kw.items():
            (u if k in u.dtype.names else z)[1][k] = v
        call(msg, units=u, tz=z)

    bad("width and height", w=20)
    bad("width and height", h=6)
    bad("reference index", ref=2)
    bad("sub_shift", sub_shift=2)
    bad("sub_shift", sub_shift=1, h=8)
    bad("empty search box", left=5)
    bad("empty search box", bottom=-5)
    bad("above 129", left=-65, right=64)
    bad("above 129", top=-64, bottom=65)
    bad("outside the picture", x=W - 8)
    bad("outside the picture", y=H - 12)
    bad("range must be", range=0)
    bad("range must be", range=65)
    bad("reserved", reserved=1)
    bad("start point", start_x=5)
    bad("start point", start_y=-5)
    bad("outside the reference's margins", x=0, left=-M - 1, start_x=-M - 1)
    bad("outside the reference's margins", x=W - 16, right=M + 1)
    bad("outside the reference's margins", y=0, top=-M - 1)
    bad("outside the reference's margins", y=H - 16, bottom=M + 1)
    u3, z3 = np.concatenate([good_u] * 3), np.concatenate([good_z] * 3)  # only the last of three is bad: the prefix names it
    u3[2]["w"] = 20
    call("width and height", units=u3, tz=z3, n=3, named=False)
    assert "unit 2: " in L.hmx_last_error(ctx.h).decode()
    call("null argument", units=None, named=False)
    call("null argument", tz=None, named=False)
    call("null argument", refs=None, named=False)
    call("null argument", org=None, named=False)
    call("null argument", res=False, named=False)
    call("go together", trace=d_trace.ptr, cnt=None, cap=8, named=False)
    call("go together", trace=None, cnt=d_cnt.ptr, cap=8, named=False)
    call("trace_cap", trace=d_trace.ptr, cnt=d_cnt.ptr, cap=0, named=False)
    call("n must be", n=0, named=False)
    call("n_refs", n_refs=0, named=False)
    call("n_refs", n_refs=5, named=False)
    d_trace.free()
    d_cnt.free()
    # the margins themselves are legal, and the context still works
    edge_u = np.concatenate([tf.unit(0, 0, 16, 16, 0, 0, -4 * M, -4 * M, (-M, -M, -M + 3, -M + 3)), tf.unit(W - 16, H - 16, 16, 16, 1, 1, 4 * M, 4 * M, (M - 2, M - 2, M, M)),
                             good_u[:1]])
    edge_z = np.zeros(3, capi.TZ_UNIT_DTYPE)
    edge_z[0], edge_z[1], edge_z[2] = (-M + 1, -M, 64, 0), (M, M - 1, 64, 0), tuple(good_z[0])
    want = [tzo.search(sc.org, sc.refs[int(u["ref"])], (M, M), u, z, 99999, ctx.bit_depth) for u, z in zip(edge_u, edge_z)]
    compare(run(ctx, p, edge_u, edge_z, 99999), want, "after refused calls")


# ---- 8. determinism ----
def test_two_calls_same_bytes(ctx, staged):
    for sc, p in staged:
        a, b = run(ctx, p, sc.units, sc.tz, sc.lam), run(ctx, p, sc.units, sc.tz, sc.lam)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), sc.name


# ---- 9. xMotionEstimation with m_iFastSearch = 1 through the C++ host mirror ----
def check_mirror_output(out, B):
    import subpel_oracle as so
    lines = out.strip().split("\n")
    assert len(lines) == 5
    q = [int(v) for v in lines[0].split()]
    u = dict(zip(("x", "y", "w", "h", "sub_shift", "pred_x", "pred_y"), q[:7]))
    lam, w, h, m, use_had, rng_, bits_in, start_x, start_y = q[7:]
    u["ref"] = 0
    org = np.array(lines[1].split(), np.int64).reshape(h, w).astype(np.int16)
    ref = np.array(lines[2].split(), np.int64).reshape(h + 2 * m, w + 2 * m).astype(np.int16)
    assert lam > 65536 and rng_ == 16
    for line, (bi, weight) in zip(lines[3:], ((0, 1.0), (1, 0.5))):
        got = [int(v) for v in line.split()]
        centre = (start_x, start_y) if bi else (u["pred_x"], u["pred_y"])  # xSetSearchRange around rcMv when bBi (:4166)
        u["left"], u["top"], u["right"], u["bottom"] = mo.set_search_range(centre[0], centre[1], rng_, u["x"], u["y"], w, h)
        if bi:  # still the full search
            (ix, iy, _, _), _ = mo.search(org, ref, (m, m), u, lam, B)
        else:   # rcMv = *pcMvPred, clipMv, >>= 2 (:4182, :4312-4313)
            cx, cy = mo.clip_mv(u["pred_x"], u["pred_y"], u["x"], u["y"], w, h, 64)
            z = {"start_x": cx >> 2, "start_y": cy >> 2, "range": rng_}
            (ix, iy, _, _), trace, _, _ = tzo.search(org, ref, (m, m), u, z, lam, B)
            assert len(trace) > 20
        (mvx, mvy, _, cost), _, _ = so.refine_unit(org, ref, (m, m), u, ix, iy, lam, B, use_had)
        bits, total = so.me_tail(lam, (u["pred_x"], u["pred_y"]), mvx, mvy, cost, bits_in, weight)
        assert got == [mvx, mvy, bits, total], (bi, got, [mvx, mvy, bits, total])


@pytest.mark.parametrize("B,seed", [(8, 4), (10, 7)])
def test_mirror_motion_estimation_tz(B, seed):
    import __graft_entry__ as g
    g.build()
    out = subprocess.run([EXE, "tz", str(B), str(seed)], capture_output=True, text=True, check=True).stdout
    check_mirror_output(out, B)
