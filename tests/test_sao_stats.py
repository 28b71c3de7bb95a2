"""The yardstick of the encoder's SAO statistics (tests/sao_stats_oracle.py) pinned three ways -- the line-for-line
restatement against the vectorised one, the position counts against the range table of include/hmx.h, hand cases with
known answers -- and capi.sao_stats_to_hm against the reference's [type][class] indexing.  No GPU needed."""
import numpy as np
import pytest

from sao_stats_oracle import BINS, stats_loop, stats_vec

SIZES = [(136, 72), (200, 136), (72, 40)]


def random_pair(rng, w, h, B):
    """org and a reconstruction close to it (small differences, so every edge class occurs), three planes each"""
    mx = (1 << B) - 1
    org, rec = [], []
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        base = rng.integers(0, mx + 1, (ph, pw))
        smooth = (base + np.roll(base, 1, 0) + np.roll(base, 1, 1) + np.roll(base, (1, 1), (0, 1))) // 4
        r = np.clip(smooth + rng.integers(-2, 3, (ph, pw)), 0, mx)
        o = np.clip(r + rng.integers(-9, 10, (ph, pw)), 0, mx)
        org.append(o.astype(np.int16))
        rec.append(r.astype(np.int16))
    return org, rec


@pytest.mark.parametrize("lcu_based", [0, 1])
@pytest.mark.parametrize("ctu", [64, 32, 16])
@pytest.mark.parametrize("B", [8, 10])
@pytest.mark.parametrize("w,h", SIZES)
def test_loop_equals_vec(w, h, B, ctu, lcu_based):
    rng = np.random.default_rng(w * 7 + h * 3 + B + ctu + lcu_based)
    org, rec = random_pair(rng, w, h, B)
    a = stats_loop(org, rec, w, h, ctu, B, lcu_based)
    b = stats_vec(org, rec, w, h, ctu, B, lcu_based)
    assert np.array_equal(a, b)


def table_counts(comp, w, h, ctu, lcu_based):
    """[CTU, 5 types (EO_0..3, BO)] positions each pass visits: the product of the ranges of the table in include/hmx.h,
    written out per CTU without the restatements' helpers."""
    sh = 1 if comp else 0
    pw, ph, cs = w >> sh, h >> sh, ctu >> sh
    s, r = ((2, 3) if comp else (4, 5)) if lcu_based else (0, 0)
    cw, ch = -(-w // ctu), -(-h // ctu)
    out = np.zeros((cw * ch, 5), np.int64)
    for addr in range(cw * ch):
        x0, y0 = (addr % cw) * cs, (addr // cw) * cs
        W, H = min(cs, pw - x0), min(cs, ph - y0)
        L, T, R, Bt = x0 == 0, y0 == 0, x0 + W == pw, y0 + H == ph
        n_full = (W if R else W - r) - 0
        n_in = (W - 1 if R else W - r) - (1 if L else 0)
        n_v = (H - 1 if Bt else H - s) - (1 if T else 0)
        out[addr] = [(H - s) * n_in, n_v * n_full, n_v * n_in, n_v * n_in, (H if Bt else H - s) * n_full]
    return out


@pytest.mark.parametrize("lcu_based", [0, 1])
@pytest.mark.parametrize("ctu", [64, 32, 16])
@pytest.mark.parametrize("w,h", SIZES + [(1920, 1080)])
def test_position_counts(w, h, ctu, lcu_based):
    rng = np.random.default_rng(1)
    org, rec = random_pair(rng, w, h, 8)
    st = stats_vec(org, rec, w, h, ctu, 8, lcu_based)
    small = w * h <= 200 * 136
    lp = stats_loop(org, rec, w, h, ctu, 8, lcu_based) if small else None
    for comp in range(3):
        want = table_counts(comp, w, h, ctu, lcu_based)
        for s in (st, lp) if small else (st,):
            c = s[comp, :, :, 1]
            got = np.stack([c[:, 5 * t:5 * t + 5].sum(1) for t in range(4)] + [c[:, 20:].sum(1)], 1)
            assert np.array_equal(got, want), comp


def planes(w, h, fn):
    return [fn(pw, ph).astype(np.int16) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]


@pytest.mark.parametrize("B", [8, 10])
def test_constant_picture(B):
    w, h, ctu, v = 136, 72, 64, 100 << (B - 8)
    rec = planes(w, h, lambda pw, ph: np.full((ph, pw), v))
    org = planes(w, h, lambda pw, ph: np.full((ph, pw), v + 3))
    for f in (stats_loop, stats_vec):
        s = f(org, rec, w, h, ctu, B, 1)
        for t in range(4):
            cls = s[:, :, 5 * t:5 * t + 5, :]
            assert not cls[:, :, [1, 2, 3, 4], :].any()  # no edges: every sample in class 0
            assert np.array_equal(cls[:, :, 0, 0], 3 * cls[:, :, 0, 1])
        band = 1 + (v >> (B - 5))
        bo = s[:, :, 20:, :]
        assert bo[:, :, band - 1, 1].sum() == bo[:, :, :, 1].sum() > 0
        assert np.array_equal(bo[:, :, band - 1, 0], 3 * bo[:, :, band - 1, 1])


def test_checkerboard():
    """rec = 512 +- 1 in a checkerboard: every horizontal and vertical position is a local extremum (class 1 for a
    minimum, class 4 for a maximum); org - rec = +1 at minima, -1 at maxima"""
    w, h, ctu, B = 200, 136, 32, 10
    cb = lambda pw, ph: (np.indices((ph, pw)).sum(0) & 1)  # noqa: E731
    rec = planes(w, h, lambda pw, ph: 511 + 2 * cb(pw, ph))
    org = planes(w, h, lambda pw, ph: np.full((ph, pw), 512))
    for f in (stats_loop, stats_vec):
        s = f(org, rec, w, h, ctu, B, 1)
        for t in (0, 1):
            c = s[:, :, 5 * t:5 * t + 5, :]
            assert not c[:, :, [0, 2, 3], 1].any()
            assert np.array_equal(c[:, :, 1, 0], c[:, :, 1, 1]) and np.array_equal(c[:, :, 4, 0], -c[:, :, 4, 1])
            assert c[:, :, 1, 1].sum() > 0 and c[:, :, 4, 1].sum() > 0


@pytest.mark.parametrize("lcu_based", [0, 1])
def test_extreme_values(lcu_based):
    """rec = 0, org = 2^B - 1 (B = 10): all samples in class 0 / band 1, every diff at its largest"""
    w, h, ctu, B = 136, 72, 64, 10
    mx = (1 << B) - 1
    rec = planes(w, h, lambda pw, ph: np.zeros((ph, pw)))
    org = planes(w, h, lambda pw, ph: np.full((ph, pw), mx))
    s = stats_vec(org, rec, w, h, ctu, B, lcu_based)
    assert np.array_equal(s[..., 0], mx * s[..., 1])
    assert s[:, :, 20, 1].sum() == s[:, :, 20:, 1].sum()
    assert np.array_equal(s, stats_loop(org, rec, w, h, ctu, B, lcu_based))


def test_sao_stats_to_hm():
    from thevc_amd.capi import sao_stats_to_hm
    a = np.zeros((2, 3, 4, BINS, 2), np.int32)
    a[..., 0] = np.arange(BINS) + 1
    a[..., 1] = 1000 + np.arange(BINS)
    stats, count = sao_stats_to_hm(a)
    assert stats.shape == count.shape == (2, 3, 4, 5, 33) and stats.dtype == np.int64
    for t in range(4):  # SAO_EO_0..3, classes 0..4
        for c in range(5):
            assert (stats[..., t, c] == 5 * t + c + 1).all() and (count[..., t, c] == 1000 + 5 * t + c).all()
        assert not stats[..., t, 5:].any() and not count[..., t, 5:].any()
    for k in range(1, 33):  # SAO_BO, classes 1..32
        assert (stats[..., 4, k] == 20 + k).all() and (count[..., 4, k] == 1000 + 19 + k).all()
    assert not stats[..., 4, 0].any() and not count[..., 4, 0].any()
