"""Weighted distortion in the motion search on the GPU (hmx_getSADw, hmx_getHADsw and the four _wp entries) against
tests/me_wp_oracle.py, everything compared for equality: every width of the size set with the cost map, the entry corners at
8, 10 and 12 bit (identity against the unweighted entries bit for bit, weight -128, 255 / 2^7, 128 / 2^0 with its int16 wrap,
offsets -128 and 127, references at the range ends, originals outside the sample range), two references with different entries
and the same picture twice in one call, the TZ fixture set with the whole trace, every size of the sub-pel refinement with
Hadamard and with SAD, the chain behind the weighted integer search, hmx_batch_subpel_cost_wp on the 7 x 7 neighbourhood, the
scalars, every refusal, and the unweighted entries after weighted calls on the same context.  A 192 x 128 picture with margin
80 (the pictures of tests/test_gpu_me.py)."""
import ctypes as C

import numpy as np
import pytest

import extreme_inputs as ei
import me_oracle as mo
import me_wp_oracle as wo
import subpel_oracle as so
import test_gpu_me as tgm
import test_gpu_subpel_search as tgs
import tz_fixture as tf
import tz_oracle as tzo
from thevc_amd import capi

pytestmark = pytest.mark.gpu

W, H, M = tgm.W, tgm.H, tgm.M
CAP = 1024
OFFS49 = tgs.OFFS49
# (weight, offset, log2_denom)
FADE_A, FADE_B, FADE_C = (45, -20, 5), (90, 33, 6), (-7, 100, 2)
CORNERS = {"weight_min": (-128, 0, 0), "weight_max_denom_max": (255, 0, 7), "wraps_int16": (128, 0, 0), "offset_min": (37, -128, 5),
           "offset_max": (29, 127, 5)}


@pytest.fixture(scope="module", params=[8, 10, 12])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def textured(ctx):
    p = tgm.make_textured(ctx)
    yield p
    p.free()


def table(ents):
    return capi.me_wp_table([e[0] for e in ents], [e[1] for e in ents], [e[2] for e in ents])


def rows(a):
    return [tuple(int(v) for v in r) for r in a]


def check_full(p, refs, full, units, ents, lam, label):
    """hmx_batch_fullpel_search_wp with the map: every result and every map entry against the oracle."""
    B = p.ctx.bit_depth
    res, cmap, first = p.ctx.batch_fullpel_search(units, refs, p.org, W, H, M, M, lam, want_map=True, wp=table(ents))
    for i, u in enumerate(units):
        k = int(u["ref"])
        want_res, want = wo.search(p.org_h, full[k], (M, M), u, lam, B, wo.entry(*ents[k], B))
        got = cmap[first[i]:first[i + 1]].reshape(want.shape)
        assert np.array_equal(got, want), (label, i, u, np.argwhere(got != want)[:4])
        assert rows(res[i:i + 1])[0] == want_res, (label, i, u)
    plain = p.ctx.batch_fullpel_search(units, refs, p.org, W, H, M, M, lam, wp=table(ents))  # d_cost_map = NULL
    assert plain.tobytes() == res.tobytes(), label
    return res, cmap


def check_tz(p, refs, full, units, tz, ents, lam, label):
    """hmx_batch_tz_search_wp: result, count and whole trace against the oracle."""
    B = p.ctx.bit_depth
    res, counts, trace = p.ctx.batch_tz_search(units, tz, refs, p.org, W, H, M, M, lam, want_trace=True, trace_cap=CAP, wp=table(ents))
    labels = set()
    for i, (u, z) in enumerate(zip(units, tz)):
        k = int(u["ref"])
        wres, wtrace, _, lab = wo.tz_search(p.org_h, full[k], (M, M), u, z, lam, B, wo.entry(*ents[k], B))
        assert int(counts[i]) == len(wtrace) <= CAP, (label, i, int(counts[i]), len(wtrace))
        assert rows(trace[i][:len(wtrace)]) == wtrace, (label, i)
        assert rows(res[i:i + 1])[0] == wres, (label, i)
        labels |= lab
    return res, counts, trace, labels


def check_sub(p, refs, full, units, ints, ents, lam, use_had, label):
    """hmx_batch_subpel_search_wp: the result and all 18 stage costs against the oracle."""
    B = p.ctx.bit_depth
    res, costs = p.ctx.batch_subpel_search(units, ints, refs, p.org, W, H, M, M, lam, use_had, want_stage_costs=True, wp=table(ents))
    for i, (u, v) in enumerate(zip(units, ints)):
        k = int(u["ref"])
        want = wo.refine_unit(p.org_h, full[k], (M, M), u, int(v["mvx"]), int(v["mvy"]), lam, B, use_had, wo.entry(*ents[k], B))
        assert [int(c) for c in costs[i]] == want[1], (label, i, u, v)
        assert rows(res[i:i + 1])[0] == want[0], (label, i, u, v)
    return res, costs


# ---- 1. the scalars ----
def test_scalars_vs_oracle(ctx):
    B = ctx.bit_depth
    rng = np.random.default_rng(2700 + B)
    ents = [FADE_A, FADE_B, FADE_C] + list(CORNERS.values())
    n = 0
    for w in mo.SIZES:
        for h in (4, 8, 12, 32, 64) if w % 8 else (4, 16, 24, 48, 64):
            so_, sc = w + 5, w + 11  # strides larger than the width
            org = rng.integers(-(1 << B), 1 << (B + 1), (h, so_)).astype(np.int16)
            cur = rng.integers(0, 1 << B, (h, sc)).astype(np.int16)
            if n % 4 == 0:
                cur = ei.extreme_plane(rng, sc, h, B, "binary")
            for ent in (ents[n % len(ents)], ents[(n + 3) % len(ents)]):
                e = wo.entry(*ent, B)
                assert ctx.getSADw(cur, sc, org, so_, w, h, *ent) == wo.sad_w(org[:, :w], cur[:, :w], e, B), (w, h, ent)
                assert ctx.getHADsw(cur, sc, org, so_, w, h, *ent) == wo.hads_w(org[:, :w], cur[:, :w], e, B), (w, h, ent)
            n += 1
    assert n >= 40
    # the identity entry on samples of the range: the unweighted drop-ins
    org, cur = rng.integers(0, 1 << B, (16, 16)).astype(np.int16), rng.integers(0, 1 << B, (16, 16)).astype(np.int16)
    assert ctx.getSADw(cur, 16, org, 16, 16, 16, 64, 0, 6) == ctx.getSAD(cur, 16, org, 16, 16, 16, 0)
    assert ctx.getHADsw(cur, 16, org, 16, 16, 16, 1, 0, 0) == so.measure(org, cur, B, 1)


# ---- 2. every width of the size set, two references with different entries, the same picture twice ----
def width_units(rng):
    shapes = [(4, 4), (4, 16), (8, 8), (8, 64), (12, 16), (12, 12), (16, 4), (16, 16), (24, 12), (24, 32), (32, 8), (32, 64), (48, 16), (48, 4),
              (64, 64), (64, 12)]
    assert {s[0] for s in shapes} == set(mo.SIZES) and {4, 8, 12, 16, 64} <= {s[1] for s in shapes}
    units = []
    for k, (w, h) in enumerate(shapes):
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        units.append(tgm.boxed(x, y, w, h, k % 3, int(h > 8 and k % 2 == 0), int(rng.integers(-30, 31)), int(rng.integers(-30, 31)), (1, 3, 2)[k % 3]))
    units += [tgm.unit(60, 40, 16, 16, 2, 1, 3, -5, -16, -1, 16, 1),   # 33 wide: two tiles
              tgm.unit(100, 20, 8, 12, 1, 1, 0, 0, -1, -1, 1, 1),      # a +-1 box
              tgm.unit(20, 60, 64, 64, 0, 1, -9, 2, -1, -1, 1, 1),
              tgm.unit(40, 8, 4, 8, 2, 0, 7, 7, -20, 0, 13, 0)]        # 34 wide, one row
    units = np.concatenate(units)
    assert set(units["ref"]) == {0, 1, 2} and any(int(u["sub_shift"]) and int(u["h"]) > 8 for u in units)
    return units


def test_fullpel_widths_two_references(ctx, textured):
    units = width_units(np.random.default_rng(2710 + ctx.bit_depth))
    refs, full = textured.refs + [textured.refs[0]], textured.full + [textured.full[0]]  # reference 0 twice, under two entries
    ents = [FADE_A, FADE_B, FADE_C]
    res, cmap = check_full(textured, refs, full, units, ents, 1234567, "widths")
    # not the unweighted call
    plain, pmap, _ = ctx.batch_fullpel_search(units, refs, textured.org, W, H, M, M, 1234567, want_map=True)
    assert np.count_nonzero(cmap != pmap) > cmap.size // 2


# ---- 3. the entry corners ----
def corner_units():
    full = np.concatenate([tgm.boxed(64, 32, 16, 16, 0, 1, 3, -5, 2), tgm.boxed(8, 8, 8, 8, 1, 0, -6, 4, 2), tgm.unit(96, 48, 64, 64, 1, 1, 0, 0, -1, -1, 1, 1),
                           tgm.boxed(32, 96, 4, 4, 0, 0, 9, 9, 2), tgm.boxed(128, 16, 32, 12, 0, 1, -2, -2, 1), tgm.boxed(0, 64, 12, 48, 1, 1, 5, 0, 1)])
    pairs = [tf.boxed(64, 32, 16, 16, 0, 1, 3, -5, 16), tf.boxed(8, 8, 8, 8, 1, 0, -26, 14, 8), tf.boxed(96, 48, 64, 64, 1, 1, 0, 0, 8),
             tf.boxed(100, 20, 12, 24, 0, 1, 20, -20, 64), tf.boxed(20, 100, 4, 4, 1, 0, -40, 40, 32)]
    return full, np.concatenate([a for a, _ in pairs]), np.concatenate([b for _, b in pairs])


def corner_scenes(B):
    """(name, references with margins, original): the textured pictures; references at the range ends with an original outside
    the sample range (what a bBi call passes: 2 * org - other prediction)."""
    rng = np.random.default_rng(2720 + B)
    tr, to = tf.textured_host(B)
    ends = [ei.extreme_plane(rng, W + 2 * M, H + 2 * M, B, "binary"), ei.extreme_plane(rng, W + 2 * M, H + 2 * M, B, "border")]
    org = rng.integers(-(1 << B), 1 << (B + 1), (H, W)).astype(np.int16)
    org[0:64, 0:64] = -(1 << B)
    org[64:128, 0:64] = (1 << (B + 1)) - 1
    return [("textured", tr, to), ("range ends, signed original", ends, org)]


@pytest.mark.parametrize("name", sorted(CORNERS))
def test_entry_corners(ctx, name):
    B = ctx.bit_depth
    ent = CORNERS[name]
    ufull, utz, ztz = corner_units()
    for sname, full, org in corner_scenes(B):
        p = tgm.Pictures(ctx, full, org)
        try:
            ents = [ent, FADE_A if name != "wraps_int16" else ent]
            label = (name, sname)
            check_full(p, p.refs, full, ufull, ents, 500000, label)
            res, _, _, _ = check_tz(p, p.refs, full, utz, ztz, ents, 500000, label)
            inside = [i for i, (u, r) in enumerate(zip(utz, res))
                      if int(u["left"]) <= int(r["mvx"]) <= int(u["right"]) and int(u["top"]) <= int(r["mvy"]) <= int(u["bottom"])]
            assert len(inside) >= 3
            for use_had in (1, 0):
                check_sub(p, p.refs, full, utz[inside], res[inside], ents, 500000, use_had, label)
        finally:
            p.free()
    if name == "wraps_int16":  # 128 * (2^B - 1) leaves int16 exactly when B >= 10
        top = np.array([(1 << B) - 1])
        assert (int(wo.weigh(top, wo.entry(*ent, B))[0]) != 128 * int(top[0])) == (B >= 10)


def test_identity_equals_unweighted(ctx, textured):
    """weight 1 << d, offset 0 leaves every sample unchanged: with sub_shift = 0 units the _wp entries give the unweighted
    entries' bytes (results, cost map, TZ trace, stage costs); with sub_shift = 1 units, those of the unweighted entries called
    with sub_shift forced to 0."""
    p = textured
    ufull, utz, ztz = corner_units()
    sc = tf.scenes(ctx.bit_depth)[0]
    utz, ztz = np.concatenate([utz, sc.units[:12]]), np.concatenate([ztz, sc.tz[:12]])
    assert set(ufull["sub_shift"]) == {0, 1} == set(utz["sub_shift"])
    lam = 777777
    for d in (0, 3, 7):
        wp = table([(1 << d, 0, d), (1 << d, 0, d)])
        for keep in (0, 1):
            uf, ut, zt = ufull[ufull["sub_shift"] == keep], utz[utz["sub_shift"] == keep], ztz[utz["sub_shift"] == keep]
            uf0, ut0 = uf.copy(), ut.copy()
            uf0["sub_shift"], ut0["sub_shift"] = 0, 0
            a = ctx.batch_fullpel_search(uf, p.refs, p.org, W, H, M, M, lam, want_map=True, wp=wp)
            b = ctx.batch_fullpel_search(uf0, p.refs, p.org, W, H, M, M, lam, want_map=True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (d, keep, "full")
            a = ctx.batch_tz_search(ut, zt, p.refs, p.org, W, H, M, M, lam, want_trace=True, trace_cap=CAP, wp=wp)
            b = ctx.batch_tz_search(ut0, zt, p.refs, p.org, W, H, M, M, lam, want_trace=True, trace_cap=CAP)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), (d, keep, "tz")
            if keep:  # sub_shift = 1 does change the unweighted walk: the comparison above is not between equal inputs
                c = ctx.batch_tz_search(ut, zt, p.refs, p.org, W, H, M, M, lam, want_trace=True, trace_cap=CAP)
                assert c[2].tobytes() != b[2].tobytes()
            ints = b[0]
            ok = (ints["mvx"] >= ut["left"]) & (ints["mvx"] <= ut["right"]) & (ints["mvy"] >= ut["top"]) & (ints["mvy"] <= ut["bottom"])
            for use_had in (1, 0):
                a = ctx.batch_subpel_search(ut[ok], ints[ok], p.refs, p.org, W, H, M, M, lam, use_had, want_stage_costs=True, wp=wp)
                b2 = ctx.batch_subpel_search(ut[ok], ints[ok], p.refs, p.org, W, H, M, M, lam, use_had, want_stage_costs=True)
                assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b2)), (d, keep, "subpel", use_had)


# ---- 4. TZ: the fixture set with a non-default entry, whole traces ----
def test_tz_fixture_set(ctx):
    B = ctx.bit_depth
    labels = set()
    for sc in tf.scenes(B):
        p = tgm.Pictures(ctx, sc.refs, sc.org)
        try:
            ents = [FADE_A, FADE_B][:len(sc.refs)]
            res, counts, trace, lab = check_tz(p, p.refs, sc.refs, sc.units, sc.tz, ents, sc.lam, sc.name)
            labels |= lab
            plain = ctx.batch_tz_search(sc.units, sc.tz, p.refs, p.org, W, H, M, M, sc.lam, wp=table(ents))  # no trace
            assert plain.tobytes() == res.tobytes(), sc.name
            if sc.name != "constant":
                unw = ctx.batch_tz_search(sc.units, sc.tz, p.refs, p.org, W, H, M, M, sc.lam, want_trace=True, trace_cap=CAP)
                assert unw[2].tobytes() != trace.tobytes(), sc.name
        finally:
            p.free()
    assert {"raster", "no_raster", "star_2_passes", "diamond_gt8_border", "diamond_2_8_inside"} <= labels and any(l.startswith("two_point_") for l in labels)


# ---- 5. sub-pel: every size, with Hadamard and with SAD; the chain; hmx_batch_subpel_cost_wp ----
@pytest.mark.parametrize("use_had", [1, 0])
def test_subpel_sizes(ctx, textured, use_had):
    units, ints = tgs.size_units(np.random.default_rng(2730 + ctx.bit_depth))
    ents = [FADE_A, FADE_B]
    _, costs = check_sub(textured, textured.refs, textured.full, units, ints, ents, 1234567, use_had, "sizes")
    _, plain = ctx.batch_subpel_search(units, ints, textured.refs, textured.org, W, H, M, M, 1234567, use_had, want_stage_costs=True)
    assert np.count_nonzero(costs != plain) > costs.size // 2


def test_chain_behind_weighted_search(ctx, textured):
    from thevc_amd import workload
    p = textured
    units = workload.make_me_units(2740 + ctx.bit_depth, W, H, 2, 4)
    assert len(units) >= 6
    ents, lam = [FADE_B, FADE_C], 2222222
    d_int = ctx.batch_fullpel_search_device(units, p.refs, p.org, W, H, M, M, lam, wp=table(ents))
    try:
        res, costs = ctx.batch_subpel_search(units, d_int, p.refs, p.org, W, H, M, M, lam, 1, want_stage_costs=True, wp=table(ents))
        ints = d_int.download(capi.ME_RESULT_DTYPE, len(units))
    finally:
        d_int.free()
    B = ctx.bit_depth
    for i, u in enumerate(units):
        k = int(u["ref"])
        e = wo.entry(*ents[k], B)
        want_int, _ = wo.search(p.org_h, p.full[k], (M, M), u, lam, B, e)
        assert rows(ints[i:i + 1])[0] == want_int, i
        want = wo.refine_unit(p.org_h, p.full[k], (M, M), u, want_int[0], want_int[1], lam, B, 1, e)
        assert [int(c) for c in costs[i]] == want[1] and rows(res[i:i + 1])[0] == want[0], i


@pytest.mark.parametrize("use_had", [1, 0])
def test_subpel_cost_7x7(ctx, textured, use_had):
    B = ctx.bit_depth
    p = textured
    shapes = [(8, 8), (16, 12), (4, 4), (32, 16), (12, 24), (64, 8)]
    pus = np.zeros(len(shapes), capi.PU_DTYPE)
    for i, (w, h) in enumerate(shapes):
        pus[i] = (8 + 16 * i, 8 + 12 * i, w, h, i % 2, 255, 4 * (i - 2), 4 * (3 - i), 0, 0)
    ents = [FADE_A, CORNERS["wraps_int16"]]
    got = ctx.batch_subpel_cost(pus, p.refs, p.org, OFFS49, use_had, wp=table(ents))
    for i, u in enumerate(pus):
        x, y, w, h, k = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"]), int(u["ref0"])
        ix, iy = int(u["mv0x"]) >> 2, int(u["mv0y"]) >> 2
        want = [wo.dist(p.org_h[y:y + h, x:x + w], p.full[k], M + x + ix, M + y + iy, dx, dy, B, use_had, wo.entry(*ents[k], B)) for (dx, dy) in OFFS49]
        assert [int(v) for v in got[i]] == want, (i, u)
    assert not np.array_equal(got, ctx.batch_subpel_cost(pus, p.refs, p.org, OFFS49, use_had))


# ---- 6. refusals ----
BAD_ROWS = (("weight", 256), ("weight", -129), ("offset", 128), ("offset", -129), ("log2_denom", 8), ("reserved", 1))


def test_refusals(ctx, textured):
    p = textured
    L = capi.lib()
    ufull, utz, ztz = corner_units()
    ints = tgs.ints_of([(0, 0)] * len(ufull))
    good = table([FADE_A, FADE_B])
    ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in p.refs])
    org = C.byref(p.org.as_pic())
    pus = np.zeros(1, capi.PU_DTYPE)
    pus[0] = (16, 16, 8, 8, 1, 255, 0, 0, 0, 0)
    offs = np.zeros((1, 2), np.int8)
    sentinel = np.full(64, 0x5A5A5A5A, np.uint32)

    d = ctx.to_device(sentinel)

    def calls(units, tz, wp):
        u = units.ctypes.data
        return [("hmx_batch_fullpel_search_wp", lambda: L.hmx_batch_fullpel_search_wp(ctx.h, u, 2, ref_arr, 2, org, W, H, M, M, 0, d.ptr, None, wp.ctypes.data)),
                ("hmx_batch_tz_search_wp", lambda: L.hmx_batch_tz_search_wp(ctx.h, utz.ctypes.data if tz else u, ztz.ctypes.data, 2, ref_arr, 2, org, W, H, M, M,
                                                                            0, d.ptr, None, None, 0, wp.ctypes.data)),
                ("hmx_batch_subpel_search_wp", lambda: L.hmx_batch_subpel_search_wp(ctx.h, u, 2, ctx_ints.ptr, ref_arr, 2, org, W, H, M, M, 0, 1, d.ptr, None,
                                                                                    wp.ctypes.data)),
                ("hmx_batch_subpel_cost_wp", lambda: L.hmx_batch_subpel_cost_wp(ctx.h, pus.ctypes.data, 1, ref_arr, 2, org, offs.ctypes.data, 1, 1, d.ptr,
                                                                                wp.ctypes.data))]

    ctx_ints = ctx.to_device(ints)
    try:
        for field, value in BAD_ROWS:
            wp = good.copy()
            if field == "reserved":
                wp[1]["reserved"] = value
            else:
                wp[1][field][0] = value
            for name, fn in calls(ufull, True, wp):
                rc = fn()
                err = L.hmx_last_error(ctx.h).decode()
                assert rc == -1 and name + ":" in err and "wp[1]" in err, (field, value, name, rc, err)  # HMX_ERR_ARG, the entry and the row named
                ctx.sync()
                assert np.array_equal(d.download(np.uint32), sentinel), (field, name)  # nothing was launched
        # chroma components are not read
        wp = good.copy()
        wp["weight"][:, 1:], wp["offset"][:, 1:], wp["log2_denom"][:, 1:] = 999, -999, 99
        a = ctx.batch_fullpel_search(ufull, p.refs, p.org, W, H, M, M, 0, wp=wp)
        assert a.tobytes() == ctx.batch_fullpel_search(ufull, p.refs, p.org, W, H, M, M, 0, wp=good).tobytes()
        # the unweighted entry's refusals stay, under the _wp entry's name
        bad = ufull.copy()
        bad[1]["sub_shift"] = 2
        for name, fn in calls(bad, False, good)[:2]:
            rc = fn()
            err = L.hmx_last_error(ctx.h).decode()
            assert rc == -1 and err.startswith(name + ": unit 1") and "sub_shift" in err, (name, rc, err)
        bad = ufull.copy()
        bad[1]["w"] = 20
        for name, fn in calls(bad, False, good)[:3]:
            rc = fn()
            err = L.hmx_last_error(ctx.h).decode()
            assert rc == -1 and err.startswith(name + ": unit 1") and "width and height" in err, (name, rc, err)
        ctx.sync()
        assert np.array_equal(d.download(np.uint32), sentinel)
    finally:
        ctx_ints.free()
        d.free()
    for fn, nm in ((ctx.getSADw, "hmx_getSADw"), (ctx.getHADsw, "hmx_getHADsw")):
        z = np.zeros(64, np.int16)
        for ent in ((256, 0, 0), (-129, 0, 0), (1, 128, 0), (1, -129, 0), (1, 0, 8), (1, 0, -1)):
            with pytest.raises(capi.HmxError, match=nm):
                fn(z, 8, z, 8, 8, 8, *ent)
        with pytest.raises(capi.HmxError, match="width and height"):
            fn(np.zeros(400, np.int16), 20, np.zeros(400, np.int16), 20, 20, 16, 1, 0, 0)
    # the range ends themselves are legal, and the context still works
    ends = [(-128, -128, 7), (255, 127, 0)]
    check_full(p, p.refs, p.full, ufull, ends, 99999, "after refused calls")
    check_tz(p, p.refs, p.full, utz, ztz, ends, 99999, "after refused calls")


# ---- 7. the unweighted entries after weighted calls on the same context ----
def test_unweighted_after_weighted(ctx, textured):
    p = textured
    B = ctx.bit_depth
    ufull, utz, ztz = corner_units()
    ents, lam = [CORNERS["wraps_int16"], FADE_C], 1234567
    res_w = check_tz(p, p.refs, p.full, utz, ztz, ents, lam, "weighted first")[0]
    check_full(p, p.refs, p.full, ufull, ents, lam, "weighted first")
    p.check(ufull, lam, "unweighted after weighted")  # against me_oracle, with the map
    res, counts, trace = ctx.batch_tz_search(utz, ztz, p.refs, p.org, W, H, M, M, lam, want_trace=True, trace_cap=CAP)
    for i, (u, z) in enumerate(zip(utz, ztz)):
        wres, wtrace, _, _ = tzo.search(p.org_h, p.full[int(u["ref"])], (M, M), u, z, lam, B)
        assert int(counts[i]) == len(wtrace) and rows(trace[i][:len(wtrace)]) == wtrace and rows(res[i:i + 1])[0] == wres, i
    assert res.tobytes() != res_w.tobytes()
    ok = (res["mvx"] >= utz["left"]) & (res["mvx"] <= utz["right"]) & (res["mvy"] >= utz["top"]) & (res["mvy"] <= utz["bottom"])
    check_sub(p, p.refs, p.full, utz[ok], res[ok], ents, lam, 1, "weighted sub-pel")
    tgs.check(p, utz[ok], res[ok], lam, 1, "unweighted after weighted")
    tgs.check(p, utz[ok], res[ok], lam, 0, "unweighted after weighted")
