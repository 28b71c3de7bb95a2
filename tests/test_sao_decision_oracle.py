"""The yardstick of the SAO parameter search (tests/sao_decision_oracle.py) pinned on the reference encoder's own decisions
(tests/golden/saodec_*.npz, made by tests/golden/make_sao_decision.py), on a second construction of its candidate stage, and on
hand cases with known answers; the host helpers of include/hmx.h against it.  No GPU needed."""
import glob
import importlib.util
import os

import numpy as np
import pytest

import sao_decision_oracle as sd

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(glob.glob(os.path.join(HERE, "golden", "saodec_*.npz")))


def generator():
    spec = importlib.util.spec_from_file_location("make_sao_decision", os.path.join(HERE, "golden", "make_sao_decision.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixtures_present():
    names = " ".join(os.path.basename(f) for f in FIXTURES)
    assert len(FIXTURES) >= 4 and "intra_main" in names and "intra_he10" in names and "lowdelay_P" in names and "randomaccess" in names


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(f)[:-4] for f in FIXTURES])
def test_oracle_decides_like_the_reference_encoder(path):
    """every picture, in coding order with the rate state carried: type and offsets always, band start where the type is 4"""
    assert generator().compare(path) == []


def test_fixture_coverage():
    """what the generator asserts when it makes the set, held again on the committed files"""
    g = generator()
    counts = g.new_counts()
    for path in FIXTURES:
        assert g.compare(path, counts) == []
    for key in ("luma", "chroma"):
        assert all(counts[key].get(t, 0) > 0 for t in (-1, 0, 1, 2, 3, 4)), (key, counts[key])
    assert counts["merge_left"] > 0 and counts["merge_up"] > 0 and counts["band_pos"] > 0 and counts["band_neg"] > 0, counts
    assert counts["switched_off"] > 0, counts


@pytest.mark.skipif(not os.path.isdir("/root/reference/source/Lib/TLibEncoder"), reason="needs the reference sources (not on the GPU box)")
def test_fixture_comes_from_the_reference(tmp_path):
    """Provenance: re-make one fixture with the reference encoder + decoder tap and compare it with the committed file."""
    g = generator()
    case = [c for c in g.CASES if c[0] == "intra_main_q26_ctu16"][0]
    name, seed, w, h, n, B, qp, cfg, ctu, kw = case
    g.make(name, seed, w, h, n, B, qp, cfg, ctu, out_dir=str(tmp_path), **kw)
    new, old = np.load(tmp_path / f"saodec_{name}.npz"), np.load(os.path.join(HERE, "golden", f"saodec_{name}.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in new.files:
        assert np.array_equal(new[k], old[k]), k


def random_bins(rng, n, B, spread=1.5):
    """n records of 52 bins: counts up to a CTU's worth, a fifth of them empty, mean differences of a few quantiser steps"""
    cnt = rng.integers(0, 400, (n, 52))
    cnt[rng.random((n, 52)) < 0.2] = 0
    org = (cnt * rng.normal(0, spread * (1 << (B - 8)), (n, 52))).astype(np.int64)
    return np.stack([org, cnt], -1)


@pytest.mark.parametrize("B", [8, 10, 12])
def test_second_construction_of_the_candidate_stage(B):
    rng = np.random.default_rng(B)
    bins = random_bins(rng, 150, B)
    for lam in (2.5, 37.9, 640.0):
        offs, dist, start = sd.candidates_vec(bins, lam, B)
        for i in range(len(bins)):
            out, st = sd.candidates_loop(bins[i].tolist(), lam, B)
            assert st == start[i], (B, lam, i)
            for t in range(5):
                assert out[t][0] == offs[i, t].tolist() and out[t][1] == dist[i, t], (B, lam, i, t)
    assert np.abs(offs).max() > 0


def zeros(n):
    return np.zeros((3, n, 52, 2), np.int64)


def test_all_counts_zero_is_all_off():
    res = sd.decide(zeros(6).tolist(), 3, 2, 8, 30.0, 24.0, (1, 1), sd.ctx_init(2, 30))
    assert (res["units"]["type"] == -1).all() and not res["units"]["off"].any()
    assert res["num_no_sao"] == [6, 12]


@pytest.mark.parametrize("B,clip", [(8, 7), (10, 31), (12, 31)])
def test_offset_is_the_mean_difference_up_to_the_clip(B, clip):
    """one class with diff = count * k (in units of the coded offset) and a lambda too small to matter: offset k, clipped"""
    unit = 1 << (B - min(B, 10))
    for k in (1, 3, clip - 1, clip, clip + 5):
        bins = np.zeros((52, 2), np.int64)
        bins[1] = 200 * k * unit, 200      # EO_0 class 1: positive offsets only
        bins[5 + 4] = -200 * k * unit, 200  # EO_1 class 4: negative offsets only
        bins[20 + 7] = -200 * k * unit, 200  # band 7
        out, start = sd.candidates_loop(bins.tolist(), 1e-9, B)
        assert out[0][0] == [min(k, clip), 0, 0, 0] and out[1][0] == [0, 0, 0, -min(k, clip)]
        want = [0, 0, 0, 0]
        want[7 - start] = -min(k, clip)  # a window that holds band 7 (which of the four: the rounding of their sums decides)
        assert 4 <= start <= 7 and out[4][0] == want


def test_edge_sign_rule():
    bins = np.zeros((52, 2), np.int64)
    for c in (1, 2, 3, 4):
        bins[c] = (-300 if c < 3 else 300), 100  # the wrong sign for every class
    out, _ = sd.candidates_loop(bins.tolist(), 1e-9, 8)
    assert out[0] == ([0, 0, 0, 0], 0)


def test_huge_and_tiny_lambda():
    rng = np.random.default_rng(5)
    stats = np.stack([random_bins(rng, 6, 8) for _ in range(3)])
    res = sd.decide(stats.tolist(), 3, 2, 8, 1e12, 1e12, (1, 1), sd.ctx_init(2, 30))
    assert (res["units"]["type"] == -1).all()
    # a tiny lambda: the walk stops at its first step, the clip value, whose rate is one less (:1872-1875)
    dist_bo, cost_bo = [0] * 33, [0.0] * 33
    lam = 1e-6
    o = sd.est_iter_offset(4, 3, lam, 7, 100, 100 * 90, 0, 0, 8, dist_bo, cost_bo)
    d = sd.est_sao_dist(100, 7, 100 * 90, 0)
    assert o == 7 and dist_bo[2] == d and cost_bo[2] == float(d) + lam * float(7 + 2 - 1)
    o = sd.est_iter_offset(0, 1, lam, 6, 100, 100 * 6, 0, 0, 8, dist_bo, cost_bo)
    assert o == 6  # below the clip: rate 6 + 1, no decrement, and still the best


@pytest.mark.parametrize("B", [8, 10, 12])
def test_band_distortion_is_cast_to_32_bits(B):
    """(Int) tempDist, :1886.  A recorded distortion is negative, so |dist| <= 2 |diff| (offset << bitIncrease) >> shift: with int32
    bins that passes 2^31 at 8 bit (offset 7, shift 0) and at 10 bit (31, 4), and cannot at 12 bit (124, 8)"""
    bins = np.zeros((52, 2), np.int64)
    bins[20 + 9] = (1 << 31) - 1, 1 << 26
    out, start = sd.candidates_loop(bins.tolist(), 2.0, B)
    bi, _, shift = sd.sao_consts(B)
    full = sd.est_sao_dist(1 << 26, max(out[4][0]) << bi, (1 << 31) - 1, shift)
    assert out[4][1] == sd._int32(full) and (out[4][1] != full) == (B < 12)
    offs, dist, st = sd.candidates_vec(bins[None], 2.0, B)
    assert st[0] == start and offs[0, 4].tolist() == out[4][0] and dist[0, 4] == out[4][1]


def test_first_of_two_equal_band_windows_wins():
    bins = np.zeros((52, 2), np.int64)
    bins[20 + 5] = bins[20 + 15] = 64 * 3, 64  # bands 5 and 15 alike; lambda a power of two, so every window sum is exact
    out, start = sd.candidates_loop(bins.tolist(), 4.0, 8)
    assert start == 2 and out[4][0] == [0, 0, 0, 3]  # windows 2..5 hold band 5, windows 12..15 band 15: the first one wins


def test_new_parameters_win_a_tie_against_merge():
    """two CTUs without statistics: everything is off and every distortion 0, so the costs are the rates.  With the merge context
    at state 0 (MPS 0) a merge flag of 1 costs 0x85f9 and the new parameters 0x7b23 + two type bins of a saturated context: both
    one bit, and new parameters stay (:1729 is a strict <).  At state 21 (MPS 1) the flag costs 0x4144, under a bit, against
    0xe01b for the 0 in front of new parameters: the merge wins."""
    for m_state, want_left in ((0, 0), (21, 1)):
        res = sd.decide(zeros(2).tolist(), 2, 1, 8, 30.0, 24.0, (1, 1), (m_state, 124))
        assert res["units"]["left"][:, 1].tolist() == [want_left] * 3, m_state
        assert (res["units"]["type"] == -1).all()


def test_rate_state_thresholds():
    s = sd.RateState()
    assert s.flags(0) == [1, 1] and s.flags(1) == [1, 1]
    s.update(0, [75, 100], 100)  # exactly 0.75 and 0.5: not exceeded
    assert s.rate[0][0] == 0.75 and s.rate[1][0] == 0.5 and s.flags(1) == [1, 1]
    s.update(0, [76, 101], 100)
    assert s.flags(1) == [0, 0] and s.flags(0) == [1, 1] and s.flags(2) == [1, 1]
    s.update(1, [76, 100], 100)  # depth 2 looks at depth 1 only
    assert s.flags(2) == [0, 1]
    s.update(2, [0, 200], 100)
    assert s.flags(3) == [1, 0]


def test_disabled_components():
    rng = np.random.default_rng(9)
    stats = np.stack([random_bins(rng, 6, 8, 3.0) for _ in range(3)])
    both = sd.decide(stats.tolist(), 3, 2, 8, 8.0, 6.0, (1, 1), sd.ctx_init(2, 30))
    assert (both["units"]["type"] >= 0).any()
    luma = sd.decide(stats.tolist(), 3, 2, 8, 8.0, 6.0, (1, 0), sd.ctx_init(2, 30))
    assert (luma["apply"]["type"][1:] == -1).all() and (luma["apply"]["type"][0] >= 0).any() and luma["num_no_sao"][1] == 12
    none = sd.decide(stats.tolist(), 3, 2, 8, 8.0, 6.0, (0, 0), sd.ctx_init(2, 30), None, 77)
    assert (none["units"]["type"] == -1).all() and none["num_no_sao"] == [0, 0]
    assert none["ctx_state"] == sd.ctx_init(2, 30) and none["frac"] == 77  # :1659: the coder is not touched


# ---- the host helpers of include/hmx.h ----
def test_ctx_init_helper():
    from thevc_amd import capi
    for slice_type in (0, 1, 2):
        for qp in range(-3, 56):
            assert capi.sao_ctx_init(slice_type, qp).tolist() == sd.ctx_init(slice_type, qp), (slice_type, qp)
    with pytest.raises(capi.HmxError):
        capi.sao_ctx_init(3, 30)


def test_rate_state_helper():
    from thevc_amd import capi
    rng = np.random.default_rng(2)
    a, b = capi.SaoRateState(), sd.RateState()
    for _ in range(200):
        depth, n_ctu = int(rng.integers(0, 4)), int(rng.integers(1, 200))
        assert a.flags(depth).tolist() == b.flags(depth)
        nn = [int(rng.integers(0, n_ctu + 1)), 2 * int(rng.integers(0, n_ctu + 1))]
        a.update(depth, nn, n_ctu), b.update(depth, nn, n_ctu)
        assert a.rate.tolist() == b.rate
    a.update(0, [75, 100], 100)
    assert a.flags(1).tolist() == [1, 1]
    a.update(0, [76, 101], 100)
    assert a.flags(1).tolist() == [0, 0]
    with pytest.raises(capi.HmxError):
        a.flags(4)


def test_merge_allow_helper():
    from thevc_amd import capi
    from thevc_amd.decisions import slice_tile_maps
    w, h, ctu = 200, 136, 16
    cw, ch = 13, 9
    for kw in (dict(), dict(slice_starts=(0, 40)), dict(col_bounds=(0, 6)), dict(slice_starts=(0, 30, 77), col_bounds=(0, 6), row_bounds=(0, 4))):
        slice_id, tile_id = slice_tile_maps(w, h, ctu, **kw)
        got = capi.sao_merge_allow(w, h, ctu, slice_id, tile_id)
        assert got.tolist() == sd.merge_allow_bytes(cw, ch, slice_id, tile_id).tolist()
        assert not (got[:cw] & 2).any() and not (got[::cw] & 1).any()
    one = capi.sao_merge_allow(w, h, ctu, np.zeros(cw * ch, np.uint32))
    assert (one[cw + 1:cw + cw] == 3).all()
    assert len(set(capi.sao_merge_allow(w, h, ctu, *slice_tile_maps(w, h, ctu, slice_starts=(0, 30, 77), col_bounds=(0, 6))).tolist())) == 4
