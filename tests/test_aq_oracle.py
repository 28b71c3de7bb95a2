"""tests/aq_oracle.py held on the CPU: against a second construction of TEncPreanalyzer::xPreanalyze (quadrant sums from integral
images, the quadrant a sample belongs to derived from the reference's loop bounds sample by sample), against the QPs the reference
encoder coded into the streams of tests/golden/aq_stream.npz, and the library's host scalars (hmx_aq_layout, hmx_aq_thresholds,
hmx_aq_offset, hmx_aq_compute_qp) against both."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import aq_oracle as ao
from thevc_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aq_stream.npz")
SIZES = [(8, 8), (64, 64), (72, 56), (136, 72), (208, 120)]
CTUS = [16, 32, 64]
RANGES = [1, 6, 12, 64]
KINDS = ["noise", "texture", "flat", "grey", "patch", "max", "checker", "quadmin"]


def picture(w, h, B, kind, rng, part=64):
    """One luma plane, int16 (h, w)"""
    mx = (1 << B) - 1
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "noise":
        p = rng.integers(0, mx + 1, (h, w))
    elif kind == "texture":  # smooth field + noise whose strength varies over the picture: activities from 1 to thousands
        amp = (1 + ((xx // 16 + 2 * (yy // 16)) % 7)) ** 2
        p = np.clip(mx / 2 * (1 + 0.7 * np.sin(xx / 9.0) * np.cos(yy / 13.0)) + rng.integers(-64, 65, (h, w)) * amp // 49, 0, mx)
    elif kind == "flat":  # all zero: the only flat picture whose activities are exactly 1.0 (see test_the_quirk_and_the_quadrants)
        p = np.zeros((h, w))
    elif kind == "grey":
        p = np.full((h, w), int(rng.integers(1, mx + 1)))
    elif kind == "patch":  # one noisy region in a zero picture (activity 1.0): a few activities far above the layer's average
        p = np.zeros((h, w), np.int64)
        p[h // 4:h // 4 + 24, w // 4:w // 4 + 24] = rng.integers(0, mx + 1, p[h // 4:h // 4 + 24, w // 4:w // 4 + 24].shape)
    elif kind == "max":
        p = np.full((h, w), mx)
    elif kind == "checker":
        p = ((xx + yy) & 1) * mx
    elif kind == "quadmin":  # noise, but in every unit of `part` one quadrant (its number walks with the unit) is flat
        p = rng.integers(0, mx + 1, (h, w))
        for y in range(0, h, part):
            for x in range(0, w, part):
                cw, ch = min(part, w - x), min(part, h - y)
                q = (x // part + y // part) % 4
                xa, xb = (cw >> 1, cw) if q & 1 else (0, cw >> 1)
                ya, yb = (ch >> 1, ch) if q & 2 else (0, ch >> 1)
                p[y + ya:y + yb, x + xa:x + xb] = mx // 3
    else:
        raise ValueError(kind)
    return np.asarray(p).astype(np.int16)


# ---- the second construction ---------------------------------------------------------------------------------------------------------
def quadrant_of(bx, by, cw, ch):
    """The arrays a sample of the unit is added to: rows below ch >> 1 feed [0] / [1], the others [2] / [3] (:91, :106); in a row the
    samples below cw >> 1 feed the even one (:94, :99)."""
    return (0 if by < (ch >> 1) else 2) + (0 if bx < (cw >> 1) else 1)


def second_preanalyze(luma, ctu, depths, want_argmin=False):
    luma = [[int(v) for v in row] for row in np.asarray(luma)]
    h, w = len(luma), len(luma[0])
    i1 = [[0] * (w + 1) for _ in range(h + 1)]
    i2 = [[0] * (w + 1) for _ in range(h + 1)]
    for y in range(h):
        r1 = r2 = 0
        for x in range(w):
            r1 += luma[y][x]
            r2 += luma[y][x] * luma[y][x]
            i1[y + 1][x + 1] = i1[y][x + 1] + r1
            i2[y + 1][x + 1] = i2[y][x + 1] + r2

    def rect(t, x0, y0, x1, y1):
        return t[y1][x1] - t[y0][x1] - t[y1][x0] + t[y0][x0]

    acts, avgs, argmins = [], [], []
    for d in range(depths):
        part = ctu >> d
        layer = []
        for y in range(0, h, part):
            for x in range(0, w, part):
                cw, ch = min(part, w - x), min(part, h - y)
                # the quadrants' extents, from the membership rule: the first column / row that belongs to the odd / lower ones
                split_x = next(bx for bx in range(cw) if quadrant_of(bx, 0, cw, ch) & 1)
                split_y = next(by for by in range(ch) if quadrant_of(0, by, cw, ch) & 2)
                boxes = [(0, 0, split_x, split_y), (split_x, 0, cw, split_y), (0, split_y, split_x, ch), (split_x, split_y, cw, ch)]
                n = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in boxes)
                var = []
                for x0, y0, x1, y1 in boxes:
                    s, ss = rect(i1, x + x0, y + y0, x + x1, y + y1), rect(i2, x + x0, y + y0, x + x1, y + y1)
                    a = s / n  # int / int of Python is the correctly rounded quotient: equal to double(s) / n while s < 2^53
                    var.append(ss / n - a * a)
                layer.append(1.0 + min(var))
                argmins.append(var.index(min(var)))
        total = 0.0
        for a in layer:
            total += a
        acts += layer
        avgs.append(total / len(layer))
    out = (np.array(acts, np.float64), np.array(avgs, np.float64))
    return out + (argmins,) if want_argmin else out


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))


@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("w,h", SIZES)
def test_oracle_vs_second_construction(B, w, h):
    rng = np.random.default_rng(8100 + 7 * w + h + B)
    for ctu in CTUS:
        depths = ao.legal_depths(ctu)[-1]
        for kind in KINDS:
            p = picture(w, h, B, kind, rng, part=ctu)
            act, avg = ao.preanalyze(p, ctu, depths)
            act2, avg2 = second_preanalyze(p, ctu, depths)
            assert same_bits(act, act2) and same_bits(avg, avg2), (ctu, kind)
            for k in ao.legal_depths(ctu)[:-1]:  # fewer depths: a prefix of the layers
                a, v = ao.preanalyze(p, ctu, k)
                assert same_bits(a, act[:len(a)]) and same_bits(v, avg[:k])
            if kind == "flat":
                assert (act == 1.0).all() and (avg == 1.0).all()


def test_the_quirk_and_the_quadrants():
    """A flat picture of value v: every quadrant's 'variance' is v^2 / 4 - (v / 4)^2 for a full unit, because N counts the whole
    unit -- zero, and the activity exactly 1.0, only for v = 0; all samples 4095 give the largest such value.  And the quadmin
    pictures make each quadrant the minimum somewhere."""
    rng = np.random.default_rng(8200)
    act, _ = ao.preanalyze(picture(64, 64, 12, "max", rng), 64, 1)
    assert act[0] == 1.0 + (4095.0 * 4095.0 / 4.0 - (4095.0 / 4.0) * (4095.0 / 4.0))
    grey = picture(64, 64, 10, "grey", rng)
    v = float(grey[0, 0])
    assert (ao.preanalyze(grey, 16, 2)[0] == 1.0 + (v * v / 4.0 - (v / 4.0) * (v / 4.0))).all()
    seen = set()
    for w, h in ((72, 56), (208, 120)):
        seen |= set(second_preanalyze(picture(w, h, 10, "quadmin", rng, part=16), 16, 1, want_argmin=True)[2])
    assert seen == {0, 1, 2, 3}


# ---- on the reference: the QPs its encoder coded --------------------------------------------------------------------------------
def test_oracle_vs_recorded_streams():
    """tests/golden/aq_stream.npz (make_aq_stream.py): for every inter transform block with a level, the set of QPs that reproduce the
    reference decoder's reconstruction contains the QP restated from the original -- by the oracle and by hmx_aq_compute_qp.  All
    blocks are checked.  The generator's conditions on the fixture's sharpness are re-asserted on what is stored."""
    L, z = capi.lib(), np.load(GOLDEN)
    assert int(z["n_runs"]) == 6
    checked, offsets = 0, set()
    for run in range(int(z["n_runs"])):
        B, k, r, ctu, _ = [int(v) for v in z[f"run{run}_config"]]
        org, blocks, slice_qp = z[f"run{run}_org"], z[f"run{run}_blocks"], z[f"run{run}_slice_qp"]
        n, h, w = org.shape
        o, g = ao.Geom(w, h, ctu, k + 1), capi.aq_layout(w, h, ctu, k + 1)
        stats = [ao.preanalyze(org[i], ctu, k + 1) for i in range(n)]
        unique = moved = 0
        for pic, x, y, plane, cu_size, lo, mask in blocks.tolist():
            act, avg = stats[pic]
            depth, sq = ctu.bit_length() - cu_size.bit_length(), int(slice_qp[pic])
            want = ao.compute_qp(o, act, avg, x, y, depth, sq, r, 6 * (B - 8))
            assert L.hmx_aq_compute_qp(C.byref(g), act.ctypes.data, avg.ctypes.data, x, y, depth, sq, r, 6 * (B - 8)) == want
            assert lo <= want <= lo + 2 * r and (mask >> (want - lo)) & 1, (run, pic, x, y, plane, cu_size, want)
            unique += mask == 1 << (want - lo)
            moved += want != sq and not (mask >> (sq - lo)) & 1
            offsets.add(want - sq)
        assert unique >= 0.7 * len(blocks) and moved >= 100, (run, len(blocks), unique, moved)
        checked += len(blocks)
    assert checked == int(z["n_blocks"]) and min(offsets) <= -6 and max(offsets) >= 5


# ---- the library's host scalars ------------------------------------------------------------------------------------------------------
def test_layout():
    L = capi.lib()
    for w, h in SIZES + [(3840, 2160), (16384, 16384)]:
        for ctu in CTUS:
            for depths in ao.legal_depths(ctu):
                g, o = capi.aq_layout(w, h, ctu, depths), ao.Geom(w, h, ctu, depths)
                assert (g.pic_w, g.pic_h, g.ctu, g.depths, g.total) == (w, h, ctu, depths, o.total)
                assert list(g.part)[:depths] == o.part and list(g.nx)[:depths] == o.nx and list(g.ny)[:depths] == o.ny and list(g.first)[:depths] == o.first
    g = capi.AqGeom()
    for w, h, ctu, depths in ((0, 8, 64, 1), (8, -8, 64, 1), (12, 8, 64, 1), (8, 20, 64, 1), (16392, 8, 64, 1), (8, 16392, 64, 1), (64, 64, 8, 1), (64, 64, 128, 1),
                              (64, 64, 48, 1), (64, 64, 64, 0), (64, 64, 64, 5), (64, 64, 32, 4), (64, 64, 16, 3)):
        assert L.hmx_aq_layout(w, h, ctu, depths, C.byref(g)) == -1, (w, h, ctu, depths)
    assert L.hmx_aq_layout(64, 64, 64, 1, None) == -1


def neighbours(t):
    return float(np.nextafter(t, 0.0)), float(t)


@pytest.mark.parametrize("qp_range", RANGES)
def test_thresholds(qp_range):
    T = capi.aq_thresholds(qp_range)
    assert len(T) == 2 * qp_range + 1 and (np.diff(T) > 0).all()
    for i, t in enumerate(T):
        k = i - qp_range
        below, at = neighbours(t)
        assert ao.offset_of_norm(at) == k and ao.offset_of_norm(below) == k - 1, k
    # every norm lies inside the table: 1 / S < norm < S
    s = math.pow(2.0, qp_range / 6.0)
    assert T[0] < 1.0 / s and T[-1] < s


def offset_pairs(qp_range, rng, n=100000):
    """(act, avg) pairs: random ones, and pairs whose norm IS a threshold or the double below it.  A wanted norm n >= 1 is sought as
    (x, 1): n = (S x + 1) / (x + S), x = (S n - 1) / (S - n); one below 1 as (1, x): n = (S + x) / (1 + S x), x = (S - n) / (S n - 1);
    the doubles around that solution are walked until the oracle's own expression gives n (not every double is a value of it).
    Returns the pairs and how many thresholds got at least one constructed pair."""
    act = np.exp(rng.uniform(0.0, math.log(4.0e6), n))
    avg = np.exp(rng.uniform(0.0, math.log(4.0e6), n))
    act[:n // 10] = 1.0 + rng.integers(0, 50, n // 10) / 16.0  # flat regions
    pairs = list(zip(act.tolist(), avg.tolist()))
    s = math.pow(2.0, qp_range / 6.0)
    hit = 0
    for t in capi.aq_thresholds(qp_range)[1:]:
        got = 0
        for want in neighbours(t):
            if want >= 1.0:
                x, f, up = (s * want - 1.0) / (s - want), (lambda x: (s * x + 1.0) / (x + s * 1.0)), True
            else:
                x, f, up = (s - want) / (s * want - 1.0), (lambda x: (s * 1.0 + x) / (1.0 + s * x)), False
            for _ in range(256):
                if f(x) == want:
                    pairs.append((x, 1.0) if up else (1.0, x))
                    got += 1
                    break
                x = float(np.nextafter(x, math.inf if (f(x) < want) == up else 0.0))
        hit += got > 0
    return pairs, hit


@pytest.mark.parametrize("qp_range", RANGES)
def test_offset_vs_oracle(qp_range):
    L = capi.lib()
    pairs, hit = offset_pairs(qp_range, np.random.default_rng(8300 + qp_range))
    print(f"range {qp_range}: {hit} of {2 * qp_range} thresholds have a constructed pair")
    assert hit >= qp_range  # at least half of the thresholds are landed on
    for a, v in pairs:
        assert L.hmx_aq_offset(a, v, qp_range) == ao.offset(a, v, qp_range), (a, v)


def test_compute_qp_vs_oracle():
    L = capi.lib()
    rng = np.random.default_rng(8400)
    w, h = 208, 120
    for B, ctu, depths, slice_qp, qp_range in ((8, 64, 4, 30, 6), (10, 32, 2, -10, 12), (12, 16, 1, 51, 64), (10, 64, 3, 0, 1)):
        p = picture(w, h, B, "texture", rng)
        act, avg = ao.preanalyze(p, ctu, depths)
        g, o = capi.aq_layout(w, h, ctu, depths), ao.Geom(w, h, ctu, depths)
        bd = 6 * (B - 8)
        for depth in range(4):
            size = max(ctu >> depth, 8)
            for y in range(0, h, size):
                for x in range(0, w, size):
                    got = L.hmx_aq_compute_qp(C.byref(g), act.ctypes.data, avg.ctypes.data, x, y, depth, slice_qp, qp_range, bd)
                    assert got == ao.compute_qp(o, act, avg, x, y, depth, slice_qp, qp_range, bd), (x, y, depth)
        assert L.hmx_aq_compute_qp(C.byref(g), act.ctypes.data, avg.ctypes.data, w, 0, 0, slice_qp, qp_range, bd) == -128
        assert L.hmx_aq_compute_qp(None, act.ctypes.data, avg.ctypes.data, 0, 0, 0, slice_qp, qp_range, bd) == -128
