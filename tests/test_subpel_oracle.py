"""tests/subpel_oracle.py against itself, no GPU: the planes of xExtDIFUpSamplingH / Q read with xPatternRefinement's pointer
adjustments hold at every candidate what the position alone gives (`planes` against `dist`), the vectorised two stages equal
the literal loop, and the tie cases the GPU test uses give the winners the table order dictates."""
import numpy as np
import pytest

import me_oracle as mo
import subpel_oracle as so

SHAPES = [(4, 4), (8, 4), (12, 16), (16, 16), (24, 32), (64, 64)]  # (w, h)


def pictures(w, h, B, seed):
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 1 << B, (h + 24, w + 24)).astype(np.int16)
    org = rng.integers(0, 1 << B, (h, w)).astype(np.int16)
    return org, ref


@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("w,h", SHAPES)
def test_planes_hold_what_the_position_gives(w, h, B):
    org, ref = pictures(w, h, B, 100 * w + h + B)
    X = Y = 12
    fb = so.planes(ref, X, Y, w, h, B)
    for (dx, dy) in so.REFINE_H:
        got = so.plane_block(fb, w, h, 2 * dx, 2 * dy)
        assert np.array_equal(got, so.predict(ref, X, Y, w, h, 2 * dx, 2 * dy, B)), ("half", dx, dy)
    n = 0
    for half in so.REFINE_H:
        fb = so.planes(ref, X, Y, w, h, B, half)
        for (qx, qy) in so.REFINE_Q:
            hv, vv = 2 * half[0] + qx, 2 * half[1] + qy
            got = so.plane_block(fb, w, h, hv, vv)
            assert got.shape == (h, w)
            assert np.array_equal(got, so.predict(ref, X, Y, w, h, hv, vv, B)), ("quarter", half, qx, qy)
            for use_had in (0, 1):
                assert so.measure(org, got, B, use_had) == so.dist(org, ref, X, Y, hv, vv, B, use_had)
            n += 1
    assert n == 81


@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("use_had", [0, 1])
def test_refine_equals_loop(B, use_had):
    for k, (w, h) in enumerate(SHAPES):
        org, ref = pictures(w, h, B, 7 * w + h + B + use_had)
        # a smooth original near a shifted reference, so that the stages have real minima away from the centre
        org = np.clip(so.predict(ref, 12, 12, w, h, (-3, 2, 5, -1, 1, 6)[k], (2, -3, 1, 3, -2, -1)[k], B).astype(np.int32) +
                      np.random.default_rng(k).integers(-2, 3, (h, w)), 0, (1 << B) - 1).astype(np.int16)
        for (ix, iy, pred, lam) in ((0, 0, (0, 0), 0), (3, -2, (9, -11), 123456), (-7, 5, (-30, 22), 0xFFFFFFFF)):
            a = so.refine(org, ref, 12, 12, B, use_had, lam, pred, ix, iy)
            assert a == so.refine_loop(org, ref, 12, 12, B, use_had, lam, pred, ix, iy), (w, h, ix, iy)
            if k in (1, 3):
                assert a == so.refine_loop(org, ref, 12, 12, B, use_had, lam, pred, ix, iy, use_planes=True), (w, h, ix, iy)


TIES = {  # predictor - 4 * integer vector (quarter samples) -> (tied half candidates, half winner, tied quarter candidates, quarter winner, final offset)
    (-4, -7): ([3, 5], 3, [3, 5], 3, (-3, -1)),
    (-4, -8): ([5], 5, [3, 5, 7], 3, (-3, -3)),
    (-8, -6): ([3, 5], 3, list(range(9)), 0, (-2, 0)),
    (0, 0): ([0], 0, [0], 0, (0, 0)),
}


def minima(c):
    return [k for k in range(9) if c[k] == min(c)]


@pytest.mark.parametrize("rel", sorted(TIES))
@pytest.mark.parametrize("use_had", [0, 1])
def test_ties_follow_the_table_order(rel, use_had):
    B, w, h, lam = 8, 16, 16, 65536
    ref = np.full((h + 24, w + 24), 100, np.int16)
    org = np.full((h, w), 90, np.int16)
    th, wh, tq, wq, off = TIES[rel]
    for (ix, iy) in ((0, 0), (5, -3)):
        pred = (rel[0] + 4 * ix, rel[1] + 4 * iy)
        (mvx, mvy, d, cost), costs, (half, q) = so.refine(org, ref, 12, 12, B, use_had, lam, pred, ix, iy)
        assert minima(costs[:9]) == th and so.REFINE_H.index(half) == wh
        assert minima(costs[9:]) == tq and so.REFINE_Q.index(q) == wq
        assert (mvx - 4 * ix, mvy - 4 * iy) == off
        assert d == so.dist(org, ref, 12, 12, 0, 0, B, use_had) and cost == d + mo.mv_bits(mvx, mvy, pred[0], pred[1], 0)
    # the first case is the one a raster-ordered minimum gets wrong: the quarter table's entry 5 is (-1, 0), entry 3 (-1, -1)
    assert so.REFINE_Q[3] == (-1, -1) and so.REFINE_Q[5] == (-1, 0) and so.REFINE_H[3] == (-1, 0)


def test_lambda_zero_centre_wins():
    ref = np.full((64 + 24, 64 + 24), 7, np.int16)
    for n in (8, 64):
        org = np.full((n, n), 9, np.int16)
        (mvx, mvy, d, cost), costs, _ = so.refine(org, ref, 12, 12, 8, 1, 0, (5, -9), 2, 3)
        assert (mvx, mvy) == (8, 12) and len(set(costs)) == 1 and cost == d


def test_me_tail():
    lam, pred = 300000, (3, -6)
    for w in (1.0, 0.5):
        bits, cost = so.me_tail(lam, pred, 13, -9, 5000, 4, w)
        mvb = mo.mv_bits(13, -9, 3, -6, 0)
        assert bits == 4 + mvb
        assert cost == int(np.floor(w * (5000 - ((lam * mvb) >> 16)))) + ((lam * bits) >> 16)
