"""tests/wp_oracle.py, the yardstick of explicit weighted prediction, checked on the CPU for its own consistency: its two
restatements agree, unit weights give the pinned oracle's unweighted prediction / addAvg, and it gives the hand-computed samples at
the clips.  What ties it to the reference is tests/test_oracle_vs_ref_wp.py (the compiled reference's own members) and, where the
reference is absent, the reference's recorded results in tests/golden/wp_b*.npz (tests/test_golden.py::test_oracle_wp).  No GPU."""
import numpy as np
import pytest

import oracle_lib as ol
import wp_oracle as wo


def _planes(rng, w, h, lo=-32768, hi=32768):
    return [rng.integers(lo, hi, (h >> (1 if c else 0), w >> (1 if c else 0))).astype(np.int16) for c in range(3)]


@pytest.mark.parametrize("B", [8, 10, 12])
def test_loop_equals_vec(B):
    rng = np.random.default_rng(4100 + B)
    for it in range(24):
        w, h = [(4, 4), (8, 4), (4, 8), (16, 12)][it % 4]
        a, b = _planes(rng, w, h), _planes(rng, w, h)  # any int16, as the library must be exact over
        e0, e1 = wo.random_entry(rng), wo.random_entry(rng)
        for c, (l, v) in enumerate(zip(wo.add_weight_uni_loop(a, e0, B), wo.add_weight_uni_vec(a, e0, B))):
            assert np.array_equal(l, v), ("uni", it, c, e0)
        for c, (l, v) in enumerate(zip(wo.add_weight_bi_loop(a, b, e0, e1, B), wo.add_weight_bi_vec(a, b, e0, e1, B))):
            assert np.array_equal(l, v), ("bi", it, c, e0, e1)


def test_derived_fields():
    """getWpScaling's fields for one and for two lists (:286-312)."""
    e0, e1 = ([3, -5, 255], [7, -128, 127], [0, 1, 7]), ([9, 1, -128], [-2, 4, 1], [5, 5, 5])
    uni = wo.get_wp_scaling(None, e1, 10)
    assert [(d["w0"], d["offset"], d["shift"], d["round"]) for d in uni] == [(9, -8, 5, 16), (1, 16, 5, 16), (-128, 4, 5, 16)]
    assert wo.get_wp_scaling(e0, None, 8)[0] == dict(w0=3, w1=None, offset=7, shift=0, round=0)
    bi = wo.get_wp_scaling(e0, e1, 8)
    assert [(d["w0"], d["w1"], d["offset"], d["shift"], d["round"]) for d in bi] == [(3, 9, 5, 1, 1), (-5, 1, -124, 2, 2), (255, -128, 128, 8, 128)]


@pytest.mark.parametrize("B,kind,args,want", wo.CLIP_CASES)
def test_hand_computed_clips(B, kind, args, want):
    if kind == "uni":
        p, w, o, d = args
        e = ([w] * 3, [o] * 3, [d] * 3)
        src = [np.full((2, 2), p, np.int16)] * 3
        got = [wo.weight_uni_vec(np.int16(p), w, o, d, B)] + [x[0, 0] for x in wo.add_weight_uni_loop(src, e, B)]
    else:
        p0, p1, w0, w1, o0, o1, d = args
        e0, e1 = ([w0] * 3, [o0] * 3, [d] * 3), ([w1] * 3, [o1] * 3, [d] * 3)
        s0, s1 = [np.full((2, 2), p0, np.int16)] * 3, [np.full((2, 2), p1, np.int16)] * 3
        got = [wo.weight_bi_vec(np.int16(p0), np.int16(p1), w0, w1, o0, o1, d, B)] + [x[0, 0] for x in wo.add_weight_bi_loop(s0, s1, e0, e1, B)]
    assert [int(g) for g in got] == [want] * 4


def _ext_ref(rng, w, h, m, B):
    """A reference picture with margins, random samples of bit depth B everywhere (margins included)."""
    return [rng.integers(0, 1 << B, ((h >> ch) + 2 * (m >> ch), (w >> ch) + 2 * (m >> ch))).astype(np.int16) for ch in (0, 1, 1)]


def _pred(O, planes, m, x, y, w, h, mvx, mvy, bi, B):
    out = []
    for c in range(3):
        ch = 1 if c else 0
        st, mc = planes[c].shape[1], m >> ch
        t = np.zeros((h >> ch, w >> ch), np.int16)
        f = O.hmo_predInterChromaBlk if c else O.hmo_predInterLumaBlk
        f(ol.ptr(planes[c].reshape(-1), (mc + (y >> ch)) * st + mc + (x >> ch)), st, mvx, mvy, w, h, t.reshape(-1), w >> ch, bi, B)
        out.append(t)
    return out


@pytest.mark.parametrize("B", [8, 10, 12])
def test_unit_weights_are_the_unweighted_prediction(B):
    """Uni with weight = 1 << d, offset 0 is the oracle's own bi = 0 prediction (its last-stage rounding), d = 0..7;
    bi with both weights 1 << d, offsets 0 is hmo_addAvg."""
    O = ol.oracle()
    rng = np.random.default_rng(4200 + B)
    W, H, m = 32, 16, 16
    refs = [_ext_ref(rng, W, H, m, B) for _ in range(2)]
    mvs = [(0, 0), (5, 0), (0, -6), (-7, 9), (18, 3), (2, 2), (-13, -1), (4, 8)]  # every kind of fraction pair, luma and chroma
    for d in range(8):
        e = ([1 << d] * 3, [0] * 3, [d] * 3)
        for k, (mvx, mvy) in enumerate(mvs):
            w, h, x, y = [(8, 8, 4, 0), (16, 4, 8, 8), (4, 8, 20, 4), (32, 16, 0, 0)][k % 4]
            p0 = _pred(O, refs[0], m, x, y, w, h, mvx, mvy, 1, B)
            final = _pred(O, refs[0], m, x, y, w, h, mvx, mvy, 0, B)
            for c, (a, b) in enumerate(zip(wo.add_weight_uni_vec(p0, e, B), final)):
                assert np.array_equal(a, b), ("uni identity", d, k, c)
            mv1 = mvs[(k + 3) % len(mvs)]
            p1 = _pred(O, refs[1], m, x, y, w, h, mv1[0], mv1[1], 1, B)
            for c, got in enumerate(wo.add_weight_bi_vec(p0, p1, e, e, B)):
                avg = np.zeros_like(got)
                O.hmo_addAvg(p0[c].reshape(-1), p0[c].shape[1], p1[c].reshape(-1), p0[c].shape[1], avg.reshape(-1), p0[c].shape[1],
                             p0[c].shape[1], p0[c].shape[0], B)
                assert np.array_equal(got, avg), ("bi identity", d, k, c)


def test_mc_frame_wp_is_the_block_functions_plus_weights():
    """mc_frame_wp on two units (one list, two lists, one of them cut by the picture edge) equals the block-wise construction."""
    O, B = ol.oracle(), 8
    rng = np.random.default_rng(4300)
    W, H, m = 24, 16, 16
    refs = [(_ext_ref(rng, W, H, m, B), m) for _ in range(2)]
    l0, l1 = [wo.random_entry(rng) for _ in range(2)], [wo.random_entry(rng) for _ in range(2)]
    pus = np.zeros(2, ol.PU_DTYPE)
    pus[0] = (0, 0, 8, 8, 255, 1, 0, 0, -5, 3)
    pus[1] = (16, 8, 16, 8, 0, 1, 6, -2, 1, 0)  # 8 of its 16 columns lie outside the picture
    got = wo.mc_frame_wp(pus, refs, (l0, l1), B)
    a = wo.add_weight_uni_loop(_pred(O, refs[1][0], m, 0, 0, 8, 8, -5, 3, 1, B), l1[1], B)
    b = wo.add_weight_bi_loop(_pred(O, refs[0][0], m, 16, 8, 16, 8, 6, -2, 1, B), _pred(O, refs[1][0], m, 16, 8, 16, 8, 1, 0, 1, B), l0[0], l1[1], B)
    for c in range(3):
        s = 1 if c else 0
        want = np.zeros((H >> s, W >> s), np.int16)
        want[:8 >> s, :8 >> s] = a[c]
        want[8 >> s:, 16 >> s:] = b[c][:, :8 >> s]
        assert np.array_equal(got[c], want), c
