"""Pins tests/wp_oracle.py, the yardstick of explicit weighted prediction, on the compiled reference's own members:
xWeightedPredictionUni / xWeightedPredictionBi / getWpScaling of TComWeightPrediction, run by oracle/ref_tap.cpp with the rows in the
slice's m_weightPredTable and both PPS flags set, and one prediction-unit list composed from xPredInter*Blk (bi = true) and those
members as TComPrediction::xPredInterBi composes them (TComPrediction.cpp:497-535).  Bit depths 8, 10, 12; rows over the whole legal
range with each component its own; a list-1 denominator that differs from list 0's in every bi case; sources over all of int16 and
over -8192..8191; the three index patterns of xWeightedPredictionBi."""
import numpy as np
import pytest

import oracle_lib as ol
import wp_cases as wc
import wp_oracle as wo

pytestmark = pytest.mark.ref


def _same(a, b, what):
    for c in range(3):
        assert np.array_equal(a[c], b[c]), (what, c, np.argwhere(a[c] != b[c])[:3])


@pytest.mark.parametrize("B", [8, 10, 12])
def test_members_vs_loop_restatement(B):
    ol.ref().ref_init(B, 64, 64, 1)
    cases = wc.block_cases(B, every_combination=True)
    assert {(c["w"], c["h"]) for c in cases} == set(wc.SHAPES) and {c["pattern"] for c in cases} == {wc.BI, wc.L0_ONLY, wc.L1_ONLY}
    n_denoms_differ = 0
    for k, c in enumerate(cases):
        e0, e1, s0, s1 = c["e0"], c["e1"], c["src0"], c["src1"]
        if c["pattern"] == wc.BI:
            assert all(a != b for a, b in zip(e0[2], e1[2]))
            n_denoms_differ += 1
            _same(ol.r_wp_bi(s0, s1, e0, e1, k % 4, (k // 4) % 4), wo.add_weight_bi_loop(s0, s1, e0, e1, B), ("bi", k, e0, e1))
            _same(ol.r_wp_bi(s0, s1, e0, e1), wo.add_weight_bi_vec(s0, s1, e0, e1, B), ("bi vec", k, e0, e1))
        elif c["pattern"] == wc.L0_ONLY:  # xWeightedPredictionBi's branch with iRefIdx1 < 0, and the uni member itself
            _same(ol.r_wp_bi(s0, None, e0, None, k % 4), wo.add_weight_uni_loop(s0, e0, B), ("bi entry, list 0 only", k, e0))
            _same(ol.r_wp_uni(s0, e0, 0, k % 4), wo.add_weight_uni_loop(s0, e0, B), ("uni, list 0", k, e0))
            _same(ol.r_wp_uni(s0, e0, 0), wo.add_weight_uni_vec(s0, e0, B), ("uni vec", k, e0))
        else:  # iRefIdx0 < 0: the row and the source of list 1
            _same(ol.r_wp_bi(None, s1, None, e1, 0, k % 4), wo.add_weight_uni_loop(s1, e1, B), ("bi entry, list 1 only", k, e1))
            _same(ol.r_wp_uni(s1, e1, 1, k % 4), wo.add_weight_uni_loop(s1, e1, B), ("uni, list 1", k, e1))
    assert n_denoms_differ >= 2 * len(wc.SHAPES)


@pytest.mark.parametrize("B", [8, 10, 12])
def test_get_wp_scaling(B):
    """w / offset / shift / round as getWpScaling leaves them, one list and two; in the bi case list 1's copy equals list 0's."""
    ol.ref().ref_init(B, 64, 64, 1)
    rng = np.random.default_rng(6300 + B)
    for it in range(200):
        e0, e1 = wc.entry_pair(rng, True)
        for a, b in ((e0, e1), (e0, None), (None, e1)):
            got, raw = ol.r_wp_scaling(a, b)
            assert got == wo.get_wp_scaling(a, b, B), (it, a, b)
            if a is not None and b is not None:
                assert np.array_equal(raw[0][:, 2:], raw[1][:, 2:])  # offset, shift, round are shared
                assert [int(v) for v in raw[1][:, 1]] == [o * (1 << (B - 8)) for o in b[1]]


@pytest.mark.parametrize("B,kind,args,want", wo.CLIP_CASES)
def test_hand_computed_clips_are_the_reference_s(B, kind, args, want):
    ol.ref().ref_init(B, 64, 64, 1)
    if kind == "uni":
        p, w, o, d = args
        e = ([w] * 3, [o] * 3, [d] * 3)
        src = [np.full((4 >> s, 4 >> s), p, np.int16) for s in (0, 1, 1)]
        got = ol.r_wp_uni(src, e, 0) + ol.r_wp_uni(src, e, 1) + ol.r_wp_bi(src, None, e, None) + ol.r_wp_bi(None, src, None, e)
    else:
        p0, p1, w0, w1, o0, o1, d = args
        e0, e1 = ([w0] * 3, [o0] * 3, [d] * 3), ([w1] * 3, [o1] * 3, [(d + 3) % 8] * 3)  # list 1's denominator is not read
        s0, s1 = ([np.full((4 >> s, 4 >> s), p, np.int16) for s in (0, 1, 1)] for p in (p0, p1))
        got = ol.r_wp_bi(s0, s1, e0, e1)
    assert all((g == want).all() for g in got), (kind, args, want, [int(g[0, 0]) for g in got])


@pytest.mark.parametrize("B", [8, 10, 12])
def test_prediction_units_end_to_end(B):
    """The reference composition of a whole unit list against wp_oracle.mc_frame_wp (the pinned oracle's interpolation plus the vector
    formulas), B slice; and its list-0 units as a P slice, where xWeightedPredictionUni is the member called."""
    S = wc.pu_scene(B)
    wc.check_pu_scene(S)
    m = wc.MARGIN
    ext = [([np.pad(p, m >> (1 if k else 0), mode="edge") for k, p in enumerate(S["pics"][i])], m) for i in S["order"]]
    want = ol.r_mc_frame_wp(S["pus"], S["pics"], S["order"], (S["l0"], S["l1"]), B)
    _same(wo.mc_frame_wp(S["pus"], ext, (S["l0"], S["l1"]), B), want, "B slice")
    assert all(w.any() for w in want)
    uni = S["pus"][S["pus"]["ref1"] == wc.N]
    want = ol.r_mc_frame_wp(uni, S["pics"], S["order"], (S["l0"], None), B, b_slice=False)
    _same(wo.mc_frame_wp(uni, ext, (S["l0"], None), B), want, "P slice")
