"""hmx_batch_inter_pred_error[_wp] and hmx_getInterPredictionError on the GPU against tests/pred_error_oracle.py, everything
compared for equality: every unit size x {list 0, list 1, both} x SAD / Hadamard, the vectors of the compiled reference
(tests/golden/pred_error_b*.npz), the decisions with ties and empty groups, the uint32 wrap of the cost, 12 bit at the range
ends, units whose windows reach the outermost margin samples, weighted candidates, the scalar entry, every refusal of the host,
and xMergeEstimation / the AMVP loop / xCheckBestMVP through the C++ host mirror.  128 x 96 pictures with 80-sample margins
made by hmx_pic_extend_border, three references.  No candidate is skipped: the generators clip vectors with clip_mv, so every
case is valid, and the tests assert the case counts."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extreme_inputs as ei
import me_oracle as mo
import pred_error_cases as pc
import pred_error_oracle as po
import wp_cases
import wp_oracle as wo
from thevc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
W, H, M = 128, 96, 80
N = 255
M32 = 0xFFFFFFFF
FILL = 0xA5A5A5A5


class Scene:
    """Device pictures from host luma planes without margins: the references get their margins from hmx_pic_extend_border, `full`
    holds the same planes extended on the host (the nearest picture sample)."""

    def __init__(self, ctx, planes, org, w=W, h=H):
        self.ctx, self.w, self.h, self.org_h = ctx, w, h, np.ascontiguousarray(org, np.int16)
        z = np.zeros((h // 2, w // 2), np.int16)
        self.refs = []
        for p in planes:
            d = capi.DevPicture(ctx, w, h, M, M).upload([p, z, z])
            ctx._chk(capi.lib().hmx_pic_extend_border(ctx.h, C.byref(d.as_pic()), w, h, M, M))
            self.refs.append(d)
        self.full = [np.ascontiguousarray(np.pad(np.asarray(p, np.int16), M, mode="edge")) for p in planes]
        self.org = capi.DevPicture(ctx, w, h).upload([self.org_h, z, z])
        ctx.sync()

    def free(self):
        for d in self.refs + [self.org]:
            d.free()

    def run(self, cands, bits, first, lam, use_had, wp=None):
        return self.ctx.batch_inter_pred_error(cands, bits, first, self.refs, self.org, self.w, self.h, M, M, lam, use_had, wp=wp_tables(wp))

    def want(self, cands, bits, lam, use_had, wp=None):
        return po.errors(cands, bits, self.full, (M, M), self.org_h, lam, self.ctx.bit_depth, use_had, wp)

    def check(self, cands, bits, first, lam, use_had, label, wp=None):
        dist, cost, best = self.run(cands, bits, first, lam, use_had, wp)
        wd, wc = self.want(cands, bits, lam, use_had, wp)
        bad = np.flatnonzero((dist != wd) | (cost != wc))
        assert len(bad) == 0, (label, len(bad), [(int(i), cands[i], int(dist[i]), int(wd[i])) for i in bad[:4]])
        if first is not None:
            wb = po.decide(wd, wc, first)
            assert np.array_equal(best, wb), (label, np.flatnonzero(best != wb)[:4])
        return dist, cost, best


def wp_tables(wp):
    """(l0, l1) of wp_oracle entries -> WP_DTYPE tables for capi"""
    if wp is None:
        return None
    out = []
    for t in wp:
        if t is None:
            out.append(None)
            continue
        a = np.zeros(len(t), capi.WP_DTYPE)
        for r, e in enumerate(t):
            a[r] = (e[0], e[1], e[2], 0)
        out.append(a)
    return tuple(out)


def textured_planes(B, w=W, h=H, n=3, seed=0):
    rng = np.random.default_rng(7600 + B + seed)
    yy, xx = np.mgrid[0:h, 0:w]
    planes = []
    for k in range(n):
        base = (np.sin(xx / (5.0 + k)) + np.cos(yy / (7.0 - k))) * (1 << (B - 3)) + (1 << (B - 1))
        planes.append(np.clip(base + rng.integers(-(1 << (B - 4)), 1 << (B - 4), base.shape), 0, (1 << B) - 1).astype(np.int16))
    org = np.clip(np.roll(planes[0], (3, -2), (0, 1)).astype(np.int32) + rng.integers(-6, 7, (h, w)), 0, (1 << B) - 1).astype(np.int16)
    return planes, org


def cand(x, y, w, h, r0, r1, mv0=(0, 0), mv1=(0, 0), cu=None):
    """One PU record, its vectors clipped for the CU at `cu` (default: the unit's own position)."""
    cx, cy = (x, y) if cu is None else cu
    a, b = mo.clip_mv(int(mv0[0]), int(mv0[1]), cx, cy, W, H, 64), mo.clip_mv(int(mv1[0]), int(mv1[1]), cx, cy, W, H, 64)
    u = np.zeros(1, capi.PU_DTYPE)
    u[0] = (x, y, w, h, r0, r1, a[0], a[1], b[0], b[1])
    return u


def place(rng, w, h):
    return int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4


def kind_refs(rng, kind, n_refs=3):
    r0, r1 = int(rng.integers(0, n_refs)), int(rng.integers(0, n_refs))
    return (N if kind == 1 else r0), (N if kind == 0 else r1)


def grouped_candidates(rng, shapes, per_group):
    """One group per shape at a random place: per_group candidates that walk list 0, list 1, both.  -> (cands, group_first)"""
    out = []
    for (w, h) in shapes:
        x, y = place(rng, w, h)
        out += [cand(x, y, w, h, *kind_refs(rng, k % 3), rng.integers(-200, 201, 2), rng.integers(-200, 201, 2)) for k in range(per_group)]
    return np.concatenate(out), np.arange(0, len(out) + 1, per_group).astype(np.uint32)


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def scene(ctx):
    planes, org = textured_planes(ctx.bit_depth)
    s = Scene(ctx, planes, org)
    yield s
    s.free()


@pytest.fixture(scope="module")
def ctx12():
    c = capi.Context(bit_depth=12)
    yield c
    c.close()


# ---- 1. every size x kind x measure ----
def size_candidates(rng):
    """Every (width, height) of the set x {list 0, list 1, both}, twice, with random vectors; every sixteenth both vectors integer."""
    out = []
    for rep in range(2):
        for w in mo.SIZES:
            for h in mo.SIZES:
                for kind in range(3):
                    x, y = place(rng, w, h)
                    mv = [rng.integers(-330, 331, 2) for _ in range(2)]
                    if len(out) % 16 == 5:
                        mv = [(v // 4) * 4 for v in mv]
                    r0, r1 = kind_refs(rng, kind)
                    out.append(cand(x, y, w, h, r0, r1, mv[0], mv[1]))
    return np.concatenate(out)


@pytest.mark.parametrize("use_had", [1, 0])
def test_sizes_kinds_vs_oracle(ctx, scene, use_had):
    rng = np.random.default_rng(7610 + ctx.bit_depth)
    cands = size_candidates(rng)
    assert len(cands) == 2 * 64 * 3
    phases, integer_bi = [set(), set()], 0
    for u in cands:
        use = po.lists(u)
        for lst, _, mvx, mvy in use:
            phases[lst].add((mvx & 3, mvy & 3))
        integer_bi += len(use) == 2 and all((mvx & 3) == 0 and (mvy & 3) == 0 for _, _, mvx, mvy in use)
    assert len(phases[0]) == 16 and len(phases[1]) == 16 and integer_bi >= 4  # the 14-bit copy path on both lists
    assert {(int(u["w"]), int(u["h"]), int(u["ref0"] != N) + 2 * int(u["ref1"] != N)) for u in cands} == {(w, h, k) for w in mo.SIZES for h in mo.SIZES for k in (1, 2, 3)}
    bits = rng.integers(0, 40, len(cands)).astype(np.uint32)
    dist, cost, _ = scene.check(cands, bits, None, 1234567, use_had, "sizes")
    assert len(set(dist.tolist())) > 200 and (cost != dist).any()  # not a comparison of constants
    d0, c0, _ = scene.run(cands, None, None, 1234567, use_had)  # bits == NULL: 0 for every candidate
    assert np.array_equal(d0, dist) and np.array_equal(c0, dist)


# ---- 2. the vectors of the compiled reference ----
@pytest.mark.parametrize("B", [8, 10, 12])
def test_golden_vectors(B):
    S = pc.load_vectors(B)
    count = pc.check_scene(S)
    c = capi.Context(bit_depth=B)
    try:
        sc = Scene(c, [p[0] for p in S["pics"]], S["org"], pc.PIC_W, pc.PIC_H)
        n = 0
        for flag in (0, 1):
            sel = np.flatnonzero(S["weighted"] == flag)
            wp = wp_tables((S["l0"], S["l1"])) if flag else None
            dist, cost, _ = c.batch_inter_pred_error(S["cands"][sel], None, None, sc.refs, sc.org, pc.PIC_W, pc.PIC_H, M, M, 0, 1, wp=wp)
            assert np.array_equal(dist, S["had"][sel]) and np.array_equal(cost, S["had"][sel]), (B, flag, np.flatnonzero(dist != S["had"][sel])[:4])
            n += len(sel)
        assert n == len(S["cands"]) == sum(count.values()) >= 60
        sc.free()
    finally:
        c.close()


# ---- 3. decisions ----
def test_decisions(ctx, scene):
    rng = np.random.default_rng(7630 + ctx.bit_depth)
    shapes = [(8, 8), (16, 16), (8, 4), (4, 8), (16, 8), (32, 32), (12, 16), (64, 64), (24, 8), (4, 4), (48, 16), (16, 64)]
    cands, bits, first = [], [], [0]
    for g in range(300):
        n = int(rng.integers(0, 8)) if g % 9 else 0
        w, h = shapes[g % len(shapes)] if g % 50 else (64, 64)
        x, y = place(rng, w, h)
        group = []
        for k in range(n):
            if k and rng.integers(0, 3) == 0:  # a duplicate of an earlier candidate with its bits: a tie
                j = int(rng.integers(0, k))
                group.append((group[j][0].copy(), group[j][1]))
                continue
            r0, r1 = kind_refs(rng, int(rng.integers(0, 3)))
            group.append((cand(x, y, w, h, r0, r1, rng.integers(-60, 61, 2), rng.integers(-60, 61, 2)), int(rng.integers(0, 4))))
        if n > 1 and g % 4 == 0:  # the last one repeats the first one: were the best a later duplicate, it would show
            group[-1] = (group[0][0].copy(), group[0][1])
        cands += [c for c, _ in group]
        bits += [b for _, b in group]
        first.append(first[-1] + n)
    cands, bits, first = np.concatenate(cands), np.array(bits, np.uint32), np.array(first, np.uint32)
    assert len(first) == 301 and first[-1] == len(cands) > 700
    lam = 5 << 16
    dist, cost, best = scene.check(cands, bits, first, lam, 1, "decisions")
    empty = tied = 0
    for g in range(300):
        a, b = int(first[g]), int(first[g + 1])
        if a == b:
            assert tuple(int(v) for v in best[g]) == (po.NONE, po.NONE, po.NONE)
            empty += 1
            continue
        lo = int(cost[a:b].min())
        where = np.flatnonzero(cost[a:b] == lo)
        assert int(best[g]["index"]) == int(where[0]) and int(best[g]["cost"]) == lo and int(best[g]["dist"]) == int(dist[a + where[0]])
        tied += len(where) > 1  # the oracle's costs hold a tie at the minimum, and the first one won
    assert empty >= 30 and tied >= 10, (empty, tied)
    d1, c1, b1 = scene.run(cands, bits, None, lam, 1)  # costs only: groups of one inside
    assert b1 is None and np.array_equal(c1, cost) and np.array_equal(d1, dist)


# ---- 4. the cost wraps ----
def test_cost_wraps(ctx, scene):
    """uint32 throughout: the product lambda * bits wraps before the shift, so the cost term stays below 2^16 and the 32-bit sum
    itself cannot pass 2^32; what is asserted is that the restatement in wide arithmetic passes 2^32 in both places -- the
    product, and dist + (product >> 16) -- on cases where the library gives the wrapped value."""
    rng = np.random.default_rng(7640 + ctx.bit_depth)
    cands, first = grouped_candidates(rng, [(16, 16)] * 24, 4)
    assert len(cands) == 96
    bits = np.concatenate([rng.integers(0, 1 << 32, 48), rng.integers(1 << 16, 1 << 20, 48)]).astype(np.uint32)
    n_prod = n_sum = 0
    for lam in (0xFFFFFFFF, 0xFFFF0001, 0x80000000, 65536 * 3 + 1):
        dist, cost, _ = scene.check(cands, bits, first, lam, 0, "wrap")
        wide = [int(lam) * int(b) for b in bits]
        n_prod += sum(p >= 1 << 32 for p in wide)
        n_sum += sum(int(d) + (p >> 16) >= 1 << 32 for d, p in zip(dist, wide))
        assert all(int(c) == (int(d) + ((p & M32) >> 16)) & M32 for c, d, p in zip(cost, dist, wide))
    assert n_prod > 100 and n_sum > 50, (n_prod, n_sum)


# ---- 5. 12 bit at the range ends ----
def mid14(full, x, y, w, h, mvx, mvy, B):
    """The 14-bit two-stage sample (not last) in int64, no narrowing."""
    tx, ty = np.asarray(ei.LUMA_TAPS[mvx & 3], np.int64), np.asarray(ei.LUMA_TAPS[mvy & 3], np.int64)
    X, Y = M + x + (mvx >> 2) - 3, M + y + (mvy >> 2) - 3
    win = np.asarray(full, np.int64)[Y:Y + h + 7, X:X + w + 7]
    mid = (sum(int(tx[i]) * win[:, i:i + w] for i in range(8)) >> (B - 8)) - 8192
    return sum(int(ty[j]) * mid[j:j + h, :] for j in range(8)) >> 6


def test_range_ends_12bit(ctx12):
    B, mx = 12, 4095
    rng = np.random.default_rng(7650)
    half = ei.LUMA_TAPS[2]
    planes = [ei.overshoot_plane(rng, W, H, B, half, half, 1)[0], ei.overshoot_plane(rng, W, H, B, half, half, -1)[0], ei.extreme_plane(rng, W, H, B, "border")]
    org = ei.extreme_plane(rng, W, H, B, "binary")
    sc = Scene(ctx12, planes, org)
    cands = []
    for y in range(0, H, 16):
        for x in range(0, W, 16):
            cands += [cand(x, y, 16, 16, 0, N, (2, 2)), cand(x, y, 16, 16, N, 1, (0, 0), (2, 2)), cand(x, y, 16, 16, 0, 0, (2, 2), (2, 2)),
                      cand(x, y, 16, 16, 1, 1, (2, 2), (2, 2)), cand(x, y, 16, 16, 2, N, rng.integers(-300, 301, 2)),
                      cand(x, y, 16, 16, 2, int(rng.integers(0, 2)), rng.integers(-300, 301, 2), rng.integers(-9, 10, 2))]
    cands = np.concatenate(cands)
    assert len(cands) == 6 * 48
    below, above, at_zero, at_max = [0, 0], [0, 0], [0, 0], [0, 0]
    for u in cands:
        use = po.lists(u)
        x, y, w, h = (int(u[k]) for k in "xywh")
        if len(use) == 1:
            _, r, mvx, mvy = use[0]
            v = ei.interp_unclipped(sc.full[r], mvx, mvy, w, h, B, False, M + x, M + y)[0]
        else:
            a, b = (mid14(sc.full[r], x, y, w, h, mvx, mvy, B) for _, r, mvx, mvy in use)
            v = (a + b + (1 << (14 - B)) + 16384) >> (15 - B)
        lo, hi = ei.count_outside(v, B)
        k = len(use) - 1
        below[k] += lo
        above[k] += hi
        p = po.predict(u, sc.full, (M, M), B)
        assert np.array_equal(p, np.clip(v, 0, mx))  # the restatement is the prediction but for the clip
        at_zero[k] += int((p == 0).sum())
        at_max[k] += int((p == mx).sum())
    assert min(below) > 100 and min(above) > 100 and min(at_zero) > 100 and min(at_max) > 100, (below, above, at_zero, at_max)  # uni and bi: the clip was needed
    for use_had in (1, 0):
        sc.check(cands, None, None, 0, use_had, "range ends")
    sc.free()


# ---- 6. the picture corners ----
def test_corners_reach_the_margins(ctx, scene):
    """Units in the four corners with vectors far outside, clipped as for a 64 x 64 coding unit that ends at the unit's outer
    edge: the tap windows run from column -74 to column W + 74, rows likewise (the margins hold 80 samples)."""
    cands, reach = [], set()
    for (w, h) in ((64, 64), (16, 16), (4, 4), (8, 32), (32, 8)):
        for sx, sy in ((-1, -1), (1, -1), (-1, 1), (1, 1)):
            x, y = (0 if sx < 0 else W - w), (0 if sy < 0 else H - h)
            cu = (x if sx < 0 else x + w - 64, y if sy < 0 else y + h - 64)
            far = (sx * 4000 + 1, sy * 4000 + 3)
            for kind in range(3):
                c = cand(x, y, w, h, N if kind == 1 else 0, N if kind == 0 else 2, far, (far[0] + 1, far[1] - 1), cu=cu)
                cands.append(c)
                for _, _, mvx, mvy in po.lists(c[0]):
                    x0, y0 = x + (mvx >> 2), y + (mvy >> 2)
                    reach |= {("left", -(x0 - 3))} if sx < 0 else {("right", x0 + w + 3 - W)}  # the window is columns x0 - 3 .. x0 + w + 3
                    reach |= {("top", -(y0 - 3))} if sy < 0 else {("bottom", y0 + h + 3 - H)}
    assert reach == {("left", 74), ("right", 74), ("top", 74), ("bottom", 74)}
    cands = np.concatenate(cands)
    assert len(cands) == 60
    for use_had in (1, 0):
        scene.check(cands, None, None, 0, use_had, "corners")


# ---- 7. weighted candidates ----
CORNER_L0 = [([-128, 1, 1], [127, 0, 0], [0, 0, 0]), ([255, 1, 1], [-128, 0, 0], [7, 0, 0]), ([37, 1, 1], [-9, 0, 0], [5, 0, 0])]
CORNER_L1 = [([-1, 1, 1], [-128, 0, 0], [7, 0, 0]), ([128, 1, 1], [127, 0, 0], [0, 0, 0]), ([-64, 1, 1], [5, 0, 0], [6, 0, 0])]


def weighted_candidates(rng, kinds):
    out = []
    for (w, h) in wp_cases.SHAPES + [(32, 32), (48, 8), (8, 48), (16, 16)]:
        for kind in kinds:
            for _ in range(2):
                x, y = place(rng, w, h)
                r0, r1 = kind_refs(rng, kind)
                out.append(cand(x, y, w, h, r0, r1, rng.integers(-200, 201, 2), rng.integers(-200, 201, 2)))
    return out


def test_weighted(ctx, scene):
    B = ctx.bit_depth
    rng = np.random.default_rng(7670 + B)
    random_tables = [[wo.random_entry(rng) for _ in range(3)] for _ in range(2)]
    fades = list(zip(*[wp_cases.entry_pair(rng, False) for _ in range(3)]))
    n = 0
    for l0, l1 in ((CORNER_L0, CORNER_L1), tuple(random_tables), (list(fades[0]), list(fades[1]))):  # B style: both tables
        cands = weighted_candidates(rng, (0, 1, 2))
        cands += [cand(*place(rng, 16, 16), 16, 16, r, r, mv, mv) for r in range(3) for mv in ((9, -7), (0, 0), (-3, 2))]  # one picture, one vector: the bi formula
        cands = np.concatenate(cands)
        for use_had in (1, 0):
            d, _, _ = scene.check(cands, None, None, 0, use_had, "weighted B", (l0, l1))
            plain, _ = scene.want(cands, None, 0, use_had)
            assert (d != plain).sum() > len(cands) // 2  # the weights act
        same = [u for u in cands[-9:]]
        assert all(u["ref0"] == u["ref1"] and u["mv0x"] == u["mv1x"] and u["mv0y"] == u["mv1y"] for u in same)
        n += len(cands)
    for l0 in (CORNER_L0, random_tables[0]):  # P style: list 0 only, no list 1 table
        cands = np.concatenate(weighted_candidates(rng, (0,)))
        scene.check(cands, None, None, 0, 1, "weighted P", (l0, None))
        n += len(cands)
    cands = np.concatenate(weighted_candidates(rng, (1, 2)))  # a list 1 unit under a call without the list 1 table: the unit weight
    scene.check(cands, None, None, 0, 1, "no list 1 table", (CORNER_L0, None))
    assert n >= 3 * 75 + 2 * 22
    # tables that are NULL: the unweighted entry bit for bit
    cands, first = grouped_candidates(rng, wp_cases.SHAPES + [(32, 32), (48, 8), (8, 48), (16, 16)], 3)
    bits = rng.integers(0, 9, len(cands)).astype(np.uint32)
    a = scene.run(cands, bits, first, 77777, 1)
    b = scene.run(cands, bits, first, 77777, 1, (None, None))
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    scene.check(cands, bits, first, 77777, 1, "null tables")


# ---- 8. the scalar entry ----
def host_pic(full):
    p = capi.Pic()
    p.plane[0] = full.ctypes.data + (M * full.shape[1] + M) * 2
    p.stride[0] = full.shape[1]
    return p


def test_scalar_entry(ctx, scene):
    B = ctx.bit_depth
    rng = np.random.default_rng(7680 + B)
    pics = [host_pic(f) for f in scene.full]
    shapes = [(4, 4), (8, 4), (4, 8), (16, 16), (12, 16), (64, 64), (24, 32), (48, 8), (8, 8), (32, 32), (16, 64), (64, 48)]
    n = 0
    for k, (w, h) in enumerate(shapes):
        x, y = place(rng, w, h)
        r0, r1 = kind_refs(rng, k % 3)
        one = cand(x, y, w, h, r0, r1, rng.integers(-300, 301, 2), rng.integers(-300, 301, 2))
        u = one[0]
        ob = np.ascontiguousarray(scene.org_h[y:y + h, x:x + w])
        for weighted in (False, True):
            e0, e1 = wo.random_entry(rng), wo.random_entry(rng)
            tab0, tab1 = [e0] * 3, [e1] * 3
            for use_had in (1, 0):
                got = ctx.getInterPredictionError(None if r0 == N else pics[r0], None if r0 == N else (int(u["mv0x"]), int(u["mv0y"])),
                                                  None if r1 == N else pics[r1], None if r1 == N else (int(u["mv1x"]), int(u["mv1y"])), x, y, w, h, ob, w,
                                                  use_had, capi.wp_entry(*e0) if weighted and r0 != N else None,
                                                  capi.wp_entry(*e1) if weighted and r1 != N else None)
                want, _ = scene.want(one, None, 0, use_had, (tab0, tab1) if weighted else None)
                assert got == int(want[0]), (w, h, k % 3, weighted, use_had)
                n += 1
    assert n == 12 * 4
    with pytest.raises(capi.HmxError, match="every used list"):
        ctx.getInterPredictionError(pics[0], (1, 1), pics[1], (2, 2), 0, 0, 8, 8, scene.org_h[:8, :8].copy(), 8, 1, capi.wp_entry(*wo.random_entry(rng)), None)
    with pytest.raises(capi.HmxError, match="width and height"):
        ctx.getInterPredictionError(pics[0], (1, 1), None, None, 0, 0, 20, 8, scene.org_h[:8, :20].copy(), 20, 1)


# ---- 9. every refusal ----
def test_refusals(ctx, scene):
    n = 6
    d_dist, d_cost, d_best = ctx.alloc(4 * n), ctx.alloc(4 * n), ctx.alloc(12 * 3)
    fill = np.full(3 * n, FILL, np.uint32)
    for d in (d_dist, d_cost, d_best):
        d.upload(fill[:d.nbytes // 4])
    base = np.concatenate([cand(16, 8, 16, 16, 0, N, (5, -3)), cand(16, 8, 16, 16, N, 1, (0, 0), (-6, 2)), cand(16, 8, 16, 16, 2, 0, (1, 1), (2, 2)),
                           cand(64, 32, 8, 8, 1, N, (4, 4)), cand(64, 32, 8, 8, 0, 2, (3, 0), (0, 3)), cand(0, 0, 64, 64, 1, 1, (-7, 9), (9, -7))])
    first = np.array([0, 3, 5, 6], np.uint32)
    ref_arr = (capi.Pic * 3)(*[r.as_pic() for r in scene.refs])
    org = scene.org.as_pic()

    def call(cands=base, bits=None, nn=None, gf=first, ng=None, refs=ref_arr, n_refs=3, org_=org, pic=(W, H), margin=(M, M), use_had=1, dist=d_dist.ptr,
             cost=d_cost.ptr, best=d_best.ptr, wp=None):
        cands = None if cands is None else np.ascontiguousarray(cands, capi.PU_DTYPE)
        args = (ctx.h, None if cands is None else cands.ctypes.data, None if bits is None else bits.ctypes.data, len(base) if nn is None else nn,
                None if gf is None else gf.ctypes.data, (0 if gf is None else len(gf) - 1) if ng is None else ng, refs, n_refs,
                None if org_ is None else C.byref(org_), pic[0], pic[1], margin[0], margin[1], 1000, use_had, dist, cost, best)
        if wp is None:
            return capi.lib().hmx_batch_inter_pred_error(*args)
        arr, keep = capi.mc_wp_array([wp])
        return capi.lib().hmx_batch_inter_pred_error_wp(*args, arr)

    def refused(what, **kw):
        assert call(**kw) == -1, what  # HMX_ERR_ARG
        msg = capi.lib().hmx_last_error(ctx.h).decode()
        assert what in msg, (what, msg)
        ctx.sync()
        for d in (d_dist, d_cost, d_best):  # nothing was launched
            assert (d.download(np.uint32) == FILL).all(), what
        return msg

    def with_(i, **fields):
        c = base.copy()
        for k, v in fields.items():
            c[i][k] = v
        return c

    assert call() == 0  # the base call is valid ...
    ctx.sync()
    assert (d_cost.download(np.uint32) != FILL).all()
    for d in (d_dist, d_cost, d_best):  # ... and the sentinel is back
        d.upload(fill[:d.nbytes // 4])
    k = 0
    for kw in (dict(cands=None), dict(refs=None), dict(org_=None), dict(dist=None), dict(cost=None)):
        refused("null argument", **kw)
        k += 1
    for kw in (dict(best=None), dict(gf=None, ng=0), dict(gf=None, ng=3), dict(gf=first, ng=0)):  # groups and d_best come together
        refused("given together", **kw)
        k += 1
    refused("n must be at least 1", nn=0)
    refused("n_refs must be 1 .. 4", n_refs=0)
    refused("n_refs must be 1 .. 4", n_refs=5)
    refused("use_had is 0 or 1", use_had=2)
    refused("use_had is 0 or 1", use_had=-1)
    k += 5
    assert "candidate 3" in refused("width and height come from", cands=with_(3, w=20))
    assert "candidate 5" in refused("width and height come from", cands=with_(5, h=2))
    assert "candidate 1" in refused("no list is used", cands=with_(1, ref1=N))
    assert "candidate 2" in refused("reference index of list 0 outside refs[]", cands=with_(2, ref0=3))
    assert "candidate 4" in refused("reference index of list 1 outside refs[]", cands=with_(4, ref1=3))
    assert "candidate 5" in refused("the unit lies outside the picture", cands=with_(5, x=W - 60))
    assert "candidate 3" in refused("the unit lies outside the picture", cands=with_(3, y=H - 4))
    k += 7
    assert "group 1" in refused("not monotonic", gf=np.array([0, 4, 3, 6], np.uint32))
    assert "group 2" in refused("not monotonic", gf=np.array([0, 3, 5, 7], np.uint32))  # passes n
    assert "group 2" in refused("does not end at n", gf=np.array([0, 3, 5, 5], np.uint32))
    assert "group 0" in refused("group_first[0] must be 0", gf=np.array([1, 3, 5, 6], np.uint32))
    assert "group 0" in refused("differ in x, y, w or h", gf=np.array([0, 4, 5, 6], np.uint32))
    assert "group 1" in refused("differ in x, y, w or h", cands=with_(4, w=16))
    k += 6
    # the tap window one sample past the margin, in each direction (the last legal vector is accepted by the base geometry)
    for i, fields in ((0, dict(mv0x=4 * (-M - 16 + 3) - 4)), (3, dict(mv0x=4 * (W + M - 64 - 8 - 4) + 4)), (1, dict(mv1y=4 * (-M - 8 + 3) - 1)),
                      (4, dict(mv1y=4 * (H + M - 32 - 8 - 4) + 4))):
        lst = 0 if "mv0x" in fields or "mv0y" in fields else 1
        assert f"candidate {i}" in refused(f"window of list {lst} reaches outside", cands=with_(i, **fields))
        k += 1
    ok = with_(0, mv0x=4 * (-M - 16 + 3))  # exactly at the margin's end: accepted
    ok = np.concatenate([ok[:1], base[1:]])
    assert call(cands=ok) == 0
    ctx.sync()
    for d in (d_dist, d_cost, d_best):
        d.upload(fill[:d.nbytes // 4])
    good = np.zeros(3, capi.WP_DTYPE)
    good["weight"], good["log2_denom"] = 1, 0
    for field, v in (("weight", 256), ("weight", -129), ("offset", 128), ("offset", -129), ("log2_denom", 8)):
        bad = good.copy()
        bad[field][1, 0] = v
        assert "row 1" in refused("weight outside -128..255", wp=(good, bad))
        assert "list 0 row 1" in refused("weight outside -128..255", wp=(bad, None))
        k += 2
    refused("needs the list 0 table", wp=(None, good))
    k += 1
    assert k >= 40
    assert call(wp=(None, None)) == 0  # both tables NULL: the unweighted entry
    ctx.sync()
    for d in (d_dist, d_cost, d_best):
        d.free()


# ---- 10. the host mirror ----
def mirror_pu(f, cu, x, y, w, h, entry, poc, is_b, weighted):
    """One candidate as the mirror must hand it to the library: identical motion resolved, vectors clipped for the CU."""
    use = [f[0][2] >= 0, f[1][2] >= 0]
    if all(use) and is_b and not weighted and poc[0][f[0][2]] == poc[1][f[1][2]] and f[0][:2] == f[1][:2]:
        use[1] = False
    r = [entry[l][f[l][2]] if use[l] else N for l in range(2)]
    mv = [mo.clip_mv(f[l][0], f[l][1], cu[0], cu[1], W, H, 64) if use[l] else (0, 0) for l in range(2)]
    u = np.zeros(1, capi.PU_DTYPE)
    u[0] = (x, y, w, h, r[0], r[1], mv[0][0], mv[0][1], mv[1][0], mv[1][1])
    return u[0]


@pytest.mark.parametrize("slice_kind", ["B", "B weighted", "P weighted"])
def test_host_mirror(ctx, scene, slice_kind, tmp_path):
    B = ctx.bit_depth
    rng = np.random.default_rng(7690 + B + len(slice_kind))
    is_b, weighted = slice_kind[0] == "B", "weighted" in slice_kind
    lam, had_me = 65536 * 4 + 321, 1
    entry, poc = [[0, 1, 2, 0], [2, 1, 0, 1]], [[8, 4, 0, 8], [0, 4, 8, 4]]  # list 0 index 3 and list 1 index 2 are picture 0 again: POC 8
    l0, l1 = [wo.random_entry(rng) for _ in range(3)], [wo.random_entry(rng) for _ in range(3)]
    wp = None if not weighted else (l0, l1) if is_b else (l0, None)
    words, ops = [], []
    units = [(8, 4), (4, 8), (8, 8), (16, 16), (16, 8), (8, 16), (32, 32), (64, 64), (32, 16), (24, 32), (12, 16), (64, 32)]
    n_ident = n_restricted = 0
    for k in range(40):  # merge
        w, h = units[k % len(units)]
        x, y = place(rng, w, h)
        cu = (x & ~7, y & ~7) if w + h == 12 else (x, y)
        nv = 1 + k % 5
        fields, dirs = [], []
        for c in range(5):
            d = int(rng.integers(1, 4)) if is_b else 1
            f = [(int(rng.integers(-90, 91)), int(rng.integers(-90, 91)), int(rng.integers(0, 4))) if d & (l + 1) else (0, 0, -1) for l in range(2)]
            if is_b and d == 3 and (k + c) % 3 == 0:  # an identical-motion pair: the same picture through both lists, one vector
                i0 = int(rng.integers(0, 4))
                f[1] = (f[0][0], f[0][1], poc[1].index(poc[0][i0]))
                f[0] = (f[0][0], f[0][1], i0)
                n_ident += c < nv and w + h != 12
            fields.append(f)
            dirs.append(d)
        words += [1, cu[0], cu[1], x, y, w, h, nv] + [v for f in fields for l in range(2) for v in f[l]] + dirs
        ops.append(("M", cu, x, y, w, h, nv, fields, dirs))
    for k in range(24):  # AMVP
        w, h = units[(k + 3) % len(units)]
        x, y = place(rng, w, h)
        lst = int(rng.integers(0, 2)) if is_b else 0
        idx, n_c = int(rng.integers(0, 4)), 1 + k % 2
        mvs = [(int(rng.integers(-400, 401)), int(rng.integers(-400, 401))) for _ in range(2)]
        if k % 6 == 1:
            mvs[1] = mvs[0]  # equal costs but for the index bits: the first stays
        words += [2, x, y, x, y, w, h, lst, idx, n_c, mvs[0][0], mvs[0][1], mvs[1][0], mvs[1][1]]
        ops.append(("A", x, y, w, h, lst, idx, n_c, mvs))
    for k in range(40):  # xCheckBestMVP
        n_c = 2 if k % 5 else k % 2
        mvs = [(int(rng.integers(-60, 61)), int(rng.integers(-60, 61))) for _ in range(2)]
        mv = (int(rng.integers(-60, 61)), int(rng.integers(-60, 61)))
        idx, bits, cost = int(rng.integers(0, max(n_c, 1))), int(rng.integers(0, 64)), int(rng.integers(0, 1 << 31))
        words += [3, n_c, mvs[0][0], mvs[0][1], mvs[1][0], mvs[1][1], mv[0], mv[1], idx, bits, cost]
        ops.append(("C", n_c, mvs, mv, idx, bits, cost))
    path = tmp_path / "pred.bin"
    with open(path, "wb") as f:
        np.array([B, W, H, M, M, 64, had_me, lam, 3, int(is_b), int(weighted), len(ops)], np.int32).tofile(f)
        np.array([v for l in range(2) for i in range(4) for v in (entry[l][i], poc[l][i])], np.int32).tofile(f)
        if weighted:
            np.array([[e[0][0], e[1][0], e[2][0]] for t in (l0, l1) for e in t], np.int32).tofile(f)
        for p in scene.full:
            p.tofile(f)
        scene.org_h.tofile(f)
        np.array(words, np.int32).tofile(f)
    out = subprocess.run([EXE, "pred", str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(ops) == 104
    refs, org = scene.full, scene.org_h
    for line, op in zip(lines, ops):
        got = line.split()
        assert got[0] == op[0]
        got = [int(v) for v in got[1:]]
        if op[0] == "M":
            _, cu, x, y, w, h, nv, fields, dirs = op
            fields, dirs = [list(f) for f in fields], list(dirs)
            if w + h == 12:  # xRestrictBipredMergeCand
                for c in range(nv):
                    if dirs[c] == 3:
                        dirs[c], fields[c][1] = 1, (0, 0, -1)
                        n_restricted += 1
            pus = np.array([mirror_pu(fields[c], cu, x, y, w, h, entry, poc, is_b, weighted) for c in range(nv)], capi.PU_DTYPE)
            bits = [po.merge_idx_bits(c) for c in range(nv)]
            d, c_ = po.errors(pus, bits, refs, (M, M), org, lam, B, had_me, wp)
            best = po.decide(d, c_, [0, nv])[0]
            i = int(best["index"])
            assert i != po.NONE
            want = [dirs[i], i, int(best["cost"])] + list(fields[i][0]) + list(fields[i][1]) + [int(d[0])]
            assert got == want, (line, op)
        elif op[0] == "A":
            _, x, y, w, h, lst, idx, n_c, mvs = op
            tw = wp if (weighted and not is_b) else None  # xGetTemplateCost weights in a P slice only
            pus = np.array([mirror_pu([(mvs[i][0], mvs[i][1], idx) if l == lst else (0, 0, -1) for l in range(2)], (x, y), x, y, w, h, entry, poc, is_b, True)
                            for i in range(n_c)], capi.PU_DTYPE)
            bits = [po.mvp_idx_bits(i, 2) for i in range(n_c)]
            assert all(lam * b < 1 << 31 for b in bits)
            _, cost = po.errors(pus, bits, refs, (M, M), org, lam, B, 0, tw)
            best_cost, best_idx, dist_bip = 0x7FFFFFFF, 0, M32  # uiBestCost = MAX_INT, iBestIdx = 0 (:3850, :3906)
            for i in range(n_c):
                if best_cost > int(cost[i]):
                    best_cost, best_idx, dist_bip = int(cost[i]), i, int(cost[i])
            assert got == [best_idx, mvs[best_idx][0], mvs[best_idx][1], dist_bip, int(cost[0])], (line, op)
        else:
            _, n_c, mvs, mv, idx, bits, cost = op
            wi, wb, wc = po.check_best_mvp(lam, mv[0], mv[1], mvs[:n_c], idx, bits, cost)
            pred = mvs[wi] if n_c >= 2 else (mvs[idx] if n_c > 0 else (0, 0))
            assert got == [wi, pred[0], pred[1], wb, wc], (line, op)
    if is_b and not weighted:
        assert n_ident >= 3
    if is_b:
        assert n_restricted >= 2
