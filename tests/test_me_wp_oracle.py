"""tests/me_wp_oracle.py held by a second, literal construction (CPU only): the weighted sample map with plain Python integers and
an explicit 16-bit wrap, xGetSADw and xGetHADsw as double loops over samples and sub-blocks with the Hadamard transform as a
matrix product, xPatternSearch as y-outside / x-inside loops with strict <, and the TZ walk and the sub-pel stages over the
literal distortions.  The int16 wrap and the ignored sub_shift are required explicitly."""
import numpy as np
import pytest

import me_oracle as mo
import me_wp_oracle as wo
import subpel_oracle as so
import tz_fixture as tf
import tz_oracle as tzo

M32 = mo.M32
W, H, M = tf.W, tf.H, tf.M
# (weight, offset, log2_denom): identity forms, the corners of the ranges, a typical fade
ENTRIES = [(1, 0, 0), (64, 0, 6), (-128, 0, 0), (255, 0, 7), (128, 0, 0), (37, -128, 5), (90, 127, 6), (-3, 5, 1), (255, 127, 0), (-128, -128, 7)]


def wrap16(v):
    v &= 0xFFFF
    return v - 65536 if v >= 32768 else v


def pel(c, weight, offset, log2_denom, B):
    rnd = (1 << (log2_denom - 1)) if log2_denom else 0
    return wrap16(((weight * int(c) + rnd) >> log2_denom) + offset * (1 << (B - 8)))


def sad_loop(org, cur, ent, B):
    s = 0
    for r in range(org.shape[0]):
        for n in range(org.shape[1]):
            s = (s + abs(int(org[r, n]) - pel(cur[r, n], *ent, B))) & M32
    return s >> (B - 8)


def hadamard(n):
    h = np.array([[1]], np.int64)
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def hads_loop(org, cur, ent, B):
    h, w = org.shape
    n = 8 if (h % 8 == 0 and w % 8 == 0) else 4
    Hn = hadamard(n)
    total = 0
    for y in range(0, h, n):
        for x in range(0, w, n):
            d = np.array([[int(org[y + r, x + c]) - pel(cur[y + r, x + c], *ent, B) for c in range(n)] for r in range(n)], np.int64)
            s = int(np.abs(Hn @ d @ Hn).sum())
            total = (total + ((s + 2) >> 2 if n == 8 else (s + 1) >> 1)) & M32
    return total >> (B - 8)


@pytest.mark.parametrize("B", [8, 10, 12])
def test_sample_map_and_wrap(B):
    samples = np.array([0, 1, 2, (1 << B) // 2, (1 << B) - 2, (1 << B) - 1, -5, -(1 << B)], np.int64)
    for ent in ENTRIES:
        got = wo.weigh(samples, wo.entry(*ent, B))
        assert got.dtype == np.int16 and [int(v) for v in got] == [pel(c, *ent, B) for c in samples], ent
    top = (1 << B) - 1
    # weight 128 with denominator 0: 128 * (2^B - 1) leaves int16 at 10 and 12 bit and the assignment to Pel wraps
    raw = 128 * top
    assert int(wo.weigh(np.array([top]), wo.entry(128, 0, 0, B))[0]) == wrap16(raw)
    assert (wrap16(raw) != raw) == (B >= 10)
    assert [int(v) for v in wo.weigh(samples[:6], wo.entry(*wo.default_entry(3), B))] == [int(v) for v in samples[:6]]  # identity
    assert wo.entry(5, -3, 0, B) == (5, 0, 0, -3 * (1 << (B - 8))) and wo.entry(5, 7, 4, B) == (5, 8, 4, 7 * (1 << (B - 8)))


@pytest.mark.parametrize("B", [8, 10, 12])
def test_sad_and_hads_vs_loops(B):
    rng = np.random.default_rng(2600 + B)
    n = 0
    for k, (w, h) in enumerate([(4, 4), (8, 4), (4, 8), (8, 8), (12, 16), (16, 12), (24, 8), (32, 16), (16, 64), (48, 24), (64, 32)]):
        org = rng.integers(-(1 << B), 1 << (B + 1), (h, w)).astype(np.int16)  # bBi originals lie outside the sample range
        cur = rng.choice(np.array([0, (1 << B) - 1]), (h, w)).astype(np.int16) if k % 3 == 0 else rng.integers(0, 1 << B, (h, w)).astype(np.int16)
        for ent in ENTRIES[k % 2::2] + ENTRIES[4:5]:
            e = wo.entry(*ent, B)
            assert wo.sad_w(org, cur, e, B) == sad_loop(org, cur, ent, B), (w, h, ent)
            assert wo.hads_w(org, cur, e, B) == hads_loop(org, cur, ent, B), (w, h, ent)
            if h > 8:  # iSubShift = 1 is ignored: every row is read and nothing is shifted left
                assert wo.sad_w(org, cur, e, B, sub_shift=1) == sad_loop(org, cur, ent, B)
            n += 1
    assert n >= 60
    # the identity entry on samples of the range is the unweighted distortion with iSubShift = 0 -- and NOT the sub-sampled one
    org, cur = rng.integers(0, 1 << B, (16, 16)).astype(np.int16), rng.integers(0, 1 << B, (16, 16)).astype(np.int16)
    e = wo.entry(*wo.default_entry(6), B)
    assert wo.sad_w(org, cur, e, B, sub_shift=1) == mo.sad(org, cur, 0, B) != mo.sad(org, cur, 1, B)
    assert wo.hads_w(org, cur, e, B) == so.measure(org, cur, B, 1)


def search_loop(org, ref, margin, u, lam, B, ent):
    """xPatternSearch as written, with the weighted SAD: the unit's sub_shift is not read."""
    x0, y0, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
    px, py = int(u["pred_x"]), int(u["pred_y"])
    best, bx, by, costs = M32, 0, 0, []
    for y in range(int(u["top"]), int(u["bottom"]) + 1):
        for x in range(int(u["left"]), int(u["right"]) + 1):
            cur = ref[margin[1] + y0 + y:margin[1] + y0 + y + h, margin[0] + x0 + x:margin[0] + x0 + x + w]
            sm = sad_loop(org[y0:y0 + h, x0:x0 + w], cur, ent, B)
            bits = mo.comp_bits_loop((x << 2) - px) + mo.comp_bits_loop((y << 2) - py)
            sm = (sm + (((lam * bits) & M32) >> 16)) & M32
            costs.append(sm)
            if sm < best:
                best, bx, by = sm, x, y
    bits = mo.comp_bits_loop((bx << 2) - px) + mo.comp_bits_loop((by << 2) - py)
    return (bx, by, (best - (((lam * bits) & M32) >> 16)) & M32, best), costs


@pytest.mark.parametrize("B", [8, 10])
def test_search_vs_loop(B):
    refs, org = tf.textured_host(B)
    org = org.copy()
    org[0:32, 0:64] = 2 * org[0:32, 0:64] - refs[1][M:M + 32, M:M + 64]  # a bBi original: 2 * org - other prediction
    units = np.concatenate([tf.unit(8, 4, 8, 8, 0, 0, 5, -3, (-3, -2, 2, 3)), tf.unit(40, 40, 16, 16, 1, 1, -9, 6, (-2, -2, 2, 1)),
                            tf.unit(100, 60, 12, 16, 0, 1, 0, 0, (0, -1, 3, 1)), tf.unit(16, 8, 4, 4, 1, 0, 11, 11, (-1, -1, 1, 1))])
    differs = 0
    for k, u in enumerate(units):
        for ent in (ENTRIES[1 + k], ENTRIES[6]):
            (res, m), (lres, lcosts) = wo.search(org, refs[int(u["ref"])], (M, M), u, 345678, B, wo.entry(*ent, B)), \
                search_loop(org, refs[int(u["ref"])], (M, M), u, 345678, B, ent)
            assert res == lres and [int(v) for v in m.reshape(-1)] == lcosts, (k, ent)
            differs += not np.array_equal(m, mo.cost_map(org, refs[int(u["ref"])], (M, M), u, 345678, B))
    assert differs >= 6  # the weights matter
    # identity entry, sub_shift = 1: the unweighted map of the same unit with sub_shift forced to 0
    u = units[1].copy()
    m = wo.cost_map(org, refs[1], (M, M), u, 345678, B, wo.entry(*wo.default_entry(5), B))
    u0 = u.copy()
    u0["sub_shift"] = 0
    assert np.array_equal(m, mo.cost_map(org, refs[1], (M, M), u0, 345678, B)) and not np.array_equal(m, mo.cost_map(org, refs[1], (M, M), u, 345678, B))


def test_tz_vs_walk_over_literal_cost():
    B = 8
    sc = tf.scenes(B)[1]
    ent = (45, -20, 5)
    e = wo.entry(*ent, B)
    for i in (0, 9, 17):
        u, z = sc.units[i], sc.tz[i]
        ref = sc.refs[int(u["ref"])]
        x0, y0, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])

        def cost(x, y):
            cur = ref[M + y0 + y:M + y0 + y + h, M + x0 + x:M + x0 + x + w]
            return (sad_loop(sc.org[y0:y0 + h, x0:x0 + w], cur, ent, B) + mo.mv_cost(sc.lam, x, y, int(u["pred_x"]), int(u["pred_y"]), 2)) & M32
        wk = tzo.walk(cost, tuple(int(u[k]) for k in ("left", "top", "right", "bottom")), (int(z["start_x"]), int(z["start_y"])), int(z["range"]))
        res, trace, passes, _ = wo.tz_search(sc.org, ref, (M, M), u, z, sc.lam, B, e)
        assert trace == wk.trace and res[:2] == (wk.bx, wk.by) and res[3] == wk.best and passes == wk.passes
        assert res[2] == (wk.best - mo.mv_cost(sc.lam, wk.bx, wk.by, int(u["pred_x"]), int(u["pred_y"]), 2)) & M32
        assert trace != tzo.search(sc.org, ref, (M, M), u, z, sc.lam, B)[1]  # not the unweighted walk


@pytest.mark.parametrize("use_had", [1, 0])
def test_refine_vs_literal_stages(use_had):
    B = 10
    refs, org = tf.textured_host(B)
    lam = 777777
    for k, (w, h, ent) in enumerate(((8, 8, (50, 30, 5)), (12, 16, (-128, 0, 0)), (16, 4, (128, 0, 0)), (4, 8, (255, -128, 7)))):
        x, y, ix, iy, pred = 16 + 24 * k, 20 + 8 * k, k - 2, 1 - k, (3 * k - 4, 7 - 5 * k)
        ob = org[y:y + h, x:x + w]
        X, Y = M + x + ix, M + y + iy
        got = wo.refine(ob, refs[k % 2], X, Y, B, use_had, lam, pred, ix, iy, wo.entry(*ent, B))
        costs, base = [], (0, 0)
        for stage, table in enumerate((so.REFINE_H, so.REFINE_Q)):  # xPatternRefinement candidate by candidate, uiDistBest = MAX_UINT, strict <
            best, direc = M32, 0
            for i, (dx, dy) in enumerate(table):
                ox, oy = (2 * dx, 2 * dy) if stage == 0 else (2 * base[0] + dx, 2 * base[1] + dy)
                p = so.predict(refs[k % 2], X, Y, w, h, ox, oy, B)
                d = hads_loop(ob, p, ent, B) if use_had else sad_loop(ob, p, ent, B)
                c = (d + (mo.mv_cost(lam, 2 * ix + dx, 2 * iy + dy, *pred, 1) if stage == 0 else mo.mv_cost(lam, 4 * ix + ox, 4 * iy + oy, *pred, 0))) & M32
                costs.append(c)
                if c < best:
                    best, direc = c, i
            if stage == 0:
                base = table[direc]
        q = so.REFINE_Q[direc]
        mvx, mvy = 4 * ix + 2 * base[0] + q[0], 4 * iy + 2 * base[1] + q[1]
        assert got[1] == costs and got[2] == (base, q), (k, ent)
        assert got[0] == (mvx, mvy, (best - mo.mv_cost(lam, mvx, mvy, *pred, 0)) & M32, best)
        assert got[1] != so.refine(ob, refs[k % 2], X, Y, B, use_had, lam, pred, ix, iy)[1]
