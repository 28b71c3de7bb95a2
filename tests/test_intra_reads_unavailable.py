"""hmx_intra_reads_unavailable: the bit a plan stores per block to say whether the reference line needs the padding pass.

Definition: the units the mode reads with every neighbour available are not all available, i.e.
hmx_intra_dependency_mask(n, luma, mode, avail) != hmx_intra_dependency_mask(n, luma, mode, all 4n+1 bits set).

Where the function returns 0 the whole-picture chains skip the padding rule and leave, in the positions of unavailable units,
whatever their stand-in load returned.  That is sound when the oracle's prediction (fillReferenceSamples -> smoothing ->
predIntra*Ang) does not look at those positions: predicting with the true flags must equal predicting with EVERY flag set on a
plane whose unavailable units hold arbitrary samples.  Where it returns 1 the two must be able to differ, or the bit says nothing.

Cases: N = 4, 8, 16, 32 luma and N = 4, 8, 16 chroma (a 32x32 chroma block does not occur in 4:2:0 with 32x32 luma transforms, and
its 65 units do not fit the 64-bit mask -- test_intra_dependencies.py leaves it out for the same reason), all 35 modes, the 13
availability patterns of test_intra_dependencies.py.  No GPU: the function is host code of the library."""
import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi

def _predict(O, plane, x0, y0, N, luma, mode, flags, B):
    """the oracle's prediction of the block at (x0, y0) of `plane` under the availability `flags` (test_intra_dependencies.py)"""
    W = 2 * N + 1
    adi = np.zeros(2 * W * W, np.int32)
    fl = np.ascontiguousarray(flags, np.uint8)
    flat = plane.reshape(-1)
    O.hmo_fillReferenceSamples(ol.ptr(flat, y0 * plane.shape[1] + x0), plane.shape[1], fl, int(fl.sum()), 4 if luma else 2, N, B, adi)
    pred = np.zeros(N * N, np.int16)
    if luma:
        O.hmo_filterAdi(adi, N)
        O.hmo_predIntraLumaAng(adi, mode, pred, N, N, B)
    else:
        O.hmo_predIntraChromaAng(adi, mode, pred, N, N, B)
    return pred.reshape(N, N)


CASES = [(4, True), (8, True), (16, True), (32, True), (4, False), (8, False), (16, False)]
B = 10


def _patterns(N, luma):
    """the seven fixed and six random availability patterns of test_dependency_mask_covers_what_the_prediction_reads"""
    n = N // (4 if luma else 2)
    rng = np.random.default_rng(N * 2 + luma)
    pats = [[1] * (4 * n + 1), [0] * n + [1] * (3 * n + 1), [1] * (3 * n + 1) + [0] * n, [0] * n + [1] * (2 * n + 1) + [0] * n,
            [0] * (2 * n + 1) + [1] * (2 * n), [1] * (2 * n) + [0] * (2 * n + 1), [0] * (2 * n) + [1] + [0] * (2 * n)]
    pats += [[int(b) for b in rng.integers(0, 2, 4 * n + 1)] for _ in range(6)]
    assert len(pats) == 13
    return n, pats


@pytest.mark.parametrize("N,luma", CASES)
def test_reads_unavailable_is_the_definition(N, luma):
    L = capi.lib()
    n, pats = _patterns(N, luma)
    full = (1 << (4 * n + 1)) - 1
    ones = 0
    for flags in pats:
        avail = sum(b << u for u, b in enumerate(flags))
        for mode in range(35):
            want = L.hmx_intra_dependency_mask(N, int(luma), mode, avail) != L.hmx_intra_dependency_mask(N, int(luma), mode, full)
            got = L.hmx_intra_reads_unavailable(N, int(luma), mode, avail)
            assert got == int(want), (N, luma, mode, flags)
            ones += got
            # a plan stores the dependency mask in the availability's place: the bit read off that mask is the same bit
            dep = L.hmx_intra_dependency_mask(N, int(luma), mode, avail)
            assert L.hmx_intra_reads_unavailable(N, int(luma), mode, dep) == got, (N, luma, mode, flags, hex(dep))
    assert 0 < ones < 13 * 35  # both values occur
    for mode in range(35):
        assert L.hmx_intra_reads_unavailable(N, int(luma), mode, 0) == 1  # an empty availability pads


@pytest.mark.parametrize("N,luma", CASES)
def test_padding_is_invisible_without_the_bit_and_visible_with_it(N, luma):
    O, L = ol.oracle(), capi.lib()
    n, pats = _patterns(N, luma)
    rng = np.random.default_rng(1000 + N * 2 + luma)
    x0 = y0 = 2 * N + 8
    side = 4 * N + 32
    every = [1] * (4 * n + 1)
    # every sample of the plane distinct from every neighbour sample the block can read: 4N+1 <= 129 < 2^B neighbours get the
    # values of a permutation, so a padded position (a copy of ANOTHER sample) never equals the sample under it by accident
    plane = rng.integers(0, 1 << B, (side, side)).astype(np.int16)
    perm = rng.permutation(1 << B)[:4 * N + 1].astype(np.int16)
    for p in range(4 * N + 1):
        xx, yy = (-1, 2 * N - 1 - p) if p < 2 * N else ((-1, -1) if p == 2 * N else (p - 2 * N - 1, -1))
        plane[y0 + yy, x0 + xx] = perm[p]
    zeros = differ = 0
    for flags in pats:
        avail = sum(b << u for u, b in enumerate(flags))
        for mode in range(35):
            bit = L.hmx_intra_reads_unavailable(N, int(luma), mode, avail)
            padded = _predict(O, plane, x0, y0, N, luma, mode, flags, B)
            as_is = _predict(O, plane, x0, y0, N, luma, mode, every, B)
            if bit == 0:
                zeros += 1
                assert np.array_equal(padded, as_is), (N, luma, mode, flags)
            else:
                differ += not np.array_equal(padded, as_is)
    print(f"N={N} luma={luma}: bit 0 in {zeros} of {13 * 35} cases; with the bit the padding changed the prediction in {differ}")
    assert zeros > 0 and differ > 0
