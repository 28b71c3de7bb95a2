"""tests/me_oracle.py against itself: the vectorised search against the literal loop-for-loop restatement of xPatternSearch on
small cases, and the closed form of the vector bits against the reference's halving loop.  No GPU needed."""
import numpy as np
import pytest

import me_oracle as mo


def test_comp_bits_closed_form_vs_halving_loop():
    for v in range(-600, 601):
        assert mo.comp_bits(v) == mo.comp_bits_loop(v), v
    assert [mo.comp_bits(v) for v in (0, 1, -1, 2, -2, 3, 4, -4)] == [1, 3, 3, 5, 5, 5, 7, 7]  # by hand: t = 1, 2, 3, 4, 5, 6, 8, 9


def unit(x, y, w, h, s, px, py, l, t, r, b):
    return dict(x=x, y=y, w=w, h=h, ref=0, sub_shift=s, pred_x=px, pred_y=py, left=l, top=t, right=r, bottom=b)


CASES = [(8, unit(8, 8, 4, 4, 0, 0, 0, -2, -2, 2, 2), 0), (8, unit(4, 12, 8, 4, 0, 5, -3, -3, 0, 1, 0), 30000),
         (10, unit(0, 0, 4, 16, 1, -9, 14, -1, -2, 3, 2), 0xFFFFFFF3), (10, unit(12, 4, 12, 16, 1, 2, 2, 0, 0, 0, 0), 77777),
         (8, unit(16, 16, 16, 12, 1, 0, 0, -3, -1, 2, 3), 65536), (10, unit(8, 8, 8, 8, 0, 1, 1, -4, -4, 4, 4), 1 << 20)]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_vector_search_vs_literal_loop(k):
    B, u, lam = CASES[k]
    rng = np.random.default_rng(40 + k)
    m = (8, 6)
    org = rng.integers(-(1 << B), 1 << (B + 1), (32, 32)).astype(np.int16)  # the range hmx_batch_fullpel_search takes
    ref = rng.integers(0, 1 << B, (32 + 2 * m[1], 32 + 2 * m[0])).astype(np.int16)
    (win, costs) = mo.search(org, ref, m, u, lam, B)
    (win_l, costs_l) = mo.search_loop(org, ref, m, u, lam, B)
    assert win == win_l
    assert costs.reshape(-1).tolist() == costs_l


def test_first_minimum_on_ties():
    u = unit(8, 8, 8, 8, 0, 0, 0, -3, -2, 3, 2)
    org = np.full((32, 32), 7, np.int16)
    ref = np.full((48, 48), 9, np.int16)  # every SAD is 128
    for lam, want in ((0, (-3, -2)), (65536, (0, 0))):
        w1, _ = mo.search(org, ref, (8, 8), u, lam, 8)
        w2, _ = mo.search_loop(org, ref, (8, 8), u, lam, 8)
        assert w1 == w2 and w1[:2] == want and w1[2] == 128
    u = unit(8, 8, 8, 8, 0, 0, 0, -3, -2, 3, -1)  # (0, 0) is outside: the minima are (0, -1) alone, then raster order
    assert mo.search(org, ref, (8, 8), u, 65536, 8)[0][:2] == (0, -1)


def test_sad_and_range_by_hand():
    o = np.arange(64, dtype=np.int16).reshape(16, 4)
    c = np.zeros((16, 4), np.int16)
    assert mo.sad(o, c, 0, 8) == 63 * 64 // 2
    assert mo.sad(o, c, 1, 8) == 2 * sum(sum(range(8 * r, 8 * r + 4)) for r in range(8))
    assert mo.sad(o, c, 0, 10) == (63 * 64 // 2) >> 2
    # a CU at the origin of a 192 x 128 picture: the clip at -(64 + 8 - 1) on the left / top, the range elsewhere
    assert mo.set_search_range(0, 0, 64, 0, 0, 192, 128) == (-64, -64, 64, 64)
    assert mo.set_search_range(-100, 0, 64, 0, 0, 192, 128) == (-71, -64, 39, 64)
    assert mo.set_search_range(0, 0, 64, 128, 64, 192, 128) == (-64, -64, 64, 64)
    assert mo.set_search_range(40, 40, 64, 128, 64, 192, 128) == (-54, -54, 71, 71)
    assert mo.set_search_range(5, -7, 4, 64, 64, 192, 128) == (-3, -6, 5, 2)  # arithmetic >> 2 of 5 - 16, -7 - 16, 5 + 16, -7 + 16
