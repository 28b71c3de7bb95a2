"""hmx_intra_pads_simple: the bit a plan stores per block to say that the padding of its reference line is an index clamp.

Definition.  A = hmx_intra_dependency_mask(n, luma, mode, avail), the mask a plan stores: the units the mode reads among the
available ones, closed under the padding rule.  U = the units the mode reads that are not available (the reach -- the dependency mask
with every unit available -- without the availability).  The bit is 1 exactly when U is not empty (hmx_intra_reads_unavailable) and
no unit of U lies strictly between the lowest and the highest unit of A, or A is empty.

Where the bit is 1 the whole-picture chains replace the padding rule by line[p] = raw[clamp(p, lo, hi)], lo = the first sample of
A's lowest unit, hi = the last sample of A's highest unit (1 << (B - 1) everywhere when A is empty).  raw holds the plane's samples in
the units of A and ANYTHING elsewhere (those units are not loaded).  That is sound when the oracle's line (fillReferenceSamples with
the true flags) equals the clamped one at every position of every unit the mode reads.  Where the bit is 0 although the block pads,
the two must be able to differ, or the general pass kept for those blocks would be dead weight.

Cases as in test_intra_reads_unavailable.py: N = 4, 8, 16, 32 luma and N = 4, 8, 16 chroma, all 35 modes; its 13 availability patterns
plus 40 random masks of several densities, most of them with holes.  No GPU: the function is host code of the library."""
import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi

CASES = [(4, True), (8, True), (16, True), (32, True), (4, False), (8, False), (16, False)]
B = 10


def _patterns(N, luma):
    n = N // (4 if luma else 2)
    rng = np.random.default_rng(N * 2 + luma)
    pats = [[1] * (4 * n + 1), [0] * n + [1] * (3 * n + 1), [1] * (3 * n + 1) + [0] * n, [0] * n + [1] * (2 * n + 1) + [0] * n,
            [0] * (2 * n + 1) + [1] * (2 * n), [1] * (2 * n) + [0] * (2 * n + 1), [0] * (2 * n) + [1] + [0] * (2 * n)]
    pats += [[int(b) for b in rng.integers(0, 2, 4 * n + 1)] for _ in range(6)]
    for k in range(40):  # sparse, even and dense masks: holes of every width
        dens = (0.15, 0.5, 0.85, 0.95)[k % 4]
        pats.append([int(b) for b in (rng.random(4 * n + 1) < dens)])
    return n, pats


def _unit_range(u, n, N, unit):
    """first and last position of unit u in the line (p = 0 lowest below-left sample .. 2N corner .. 4N last above-right sample)"""
    if u < 2 * n:
        return u * unit, u * unit + unit - 1
    if u == 2 * n:
        return 2 * N, 2 * N
    return 2 * N + 1 + (u - 2 * n - 1) * unit, 2 * N + (u - 2 * n) * unit


def _definition(L, N, luma, mode, avail, n):
    full = (1 << (4 * n + 1)) - 1
    A = L.hmx_intra_dependency_mask(N, int(luma), mode, avail)
    U = L.hmx_intra_dependency_mask(N, int(luma), mode, full) & ~avail
    if not U:
        return 0, A, U
    if not A:
        return 1, A, U
    lo_u, hi_u = (A & -A).bit_length() - 1, A.bit_length() - 1
    between = U & ((1 << hi_u) - 1) & ~((2 << lo_u) - 1)
    return int(between == 0), A, U


@pytest.mark.parametrize("N,luma", CASES)
def test_pads_simple_is_the_definition(N, luma):
    L = capi.lib()
    n, pats = _patterns(N, luma)
    count = {(0, 0): 0, (1, 0): 0, (1, 1): 0}
    for flags in pats:
        avail = sum(b << u for u, b in enumerate(flags))
        for mode in range(35):
            want, A, U = _definition(L, N, luma, mode, avail, n)
            got = L.hmx_intra_pads_simple(N, int(luma), mode, avail)
            assert got == want, (N, luma, mode, flags, hex(A), hex(U))
            pads = L.hmx_intra_reads_unavailable(N, int(luma), mode, avail)
            assert pads == int(U != 0)
            count[(pads, got)] += 1  # the bit is never set without the padding bit: (0, 1) is a KeyError
            # a plan stores A in the availability's place: the bit read off that mask is the same bit
            assert L.hmx_intra_pads_simple(N, int(luma), mode, A) == got, (N, luma, mode, flags, hex(A))
    assert all(v > 0 for v in count.values()), count  # no padding, general padding and simple padding all occur
    for mode in range(35):
        assert L.hmx_intra_pads_simple(N, int(luma), mode, 0) == 1  # an empty availability: the mid value, no search
    assert L.hmx_intra_pads_simple(N, int(luma), 35, 0) == 0 and L.hmx_intra_pads_simple(5, int(luma), 0, 0) == 0  # not known: general


@pytest.mark.parametrize("N,luma", CASES)
def test_clamp_is_the_padding_rule_with_the_bit_and_not_without(N, luma):
    O, L = ol.oracle(), capi.lib()
    n, pats = _patterns(N, luma)
    unit = 4 if luma else 2
    rng = np.random.default_rng(2000 + N * 2 + luma)
    x0 = y0 = 2 * N + 8
    side = 4 * N + 32
    full = (1 << (4 * n + 1)) - 1
    W = 2 * N + 1
    # the 4N+1 neighbour samples distinct (a permutation): a position that copies ANOTHER sample never matches by accident
    plane = rng.integers(0, 1 << B, (side, side)).astype(np.int16)
    true_line = rng.permutation(1 << B)[:4 * N + 1].astype(np.int32)
    for p in range(4 * N + 1):
        xx, yy = (-1, 2 * N - 1 - p) if p < 2 * N else ((-1, -1) if p == 2 * N else (p - 2 * N - 1, -1))
        plane[y0 + yy, x0 + xx] = true_line[p]
    flat = plane.reshape(-1)
    simple_checked = general_differs = 0
    for flags in pats:
        avail = sum(b << u for u, b in enumerate(flags))
        fl = np.ascontiguousarray(flags, np.uint8)
        adi = np.zeros(2 * W * W, np.int32)
        O.hmo_fillReferenceSamples(ol.ptr(flat, y0 * side + x0), side, fl, int(fl.sum()), unit, N, B, adi)
        want = np.empty(4 * N + 1, np.int32)  # the oracle's line, out of its (2N+1)^2 layout
        want[2 * N:] = adi[:2 * N + 1]
        want[:2 * N] = adi[W:(2 * N + 1) * W:W][::-1]
        for mode in range(35):
            if not L.hmx_intra_reads_unavailable(N, int(luma), mode, avail):
                continue
            bit = L.hmx_intra_pads_simple(N, int(luma), mode, avail)
            A = L.hmx_intra_dependency_mask(N, int(luma), mode, avail)
            reach = L.hmx_intra_dependency_mask(N, int(luma), mode, full)
            # raw: the plane's samples in the units of A, arbitrary values (what a stand-in load returned) in every other unit
            raw = rng.integers(0, 1 << B, 4 * N + 1).astype(np.int32)
            for u in range(4 * n + 1):
                if (A >> u) & 1:
                    a, b = _unit_range(u, n, N, unit)
                    raw[a:b + 1] = true_line[a:b + 1]
            if A:
                lo = _unit_range((A & -A).bit_length() - 1, n, N, unit)[0]
                hi = _unit_range(A.bit_length() - 1, n, N, unit)[1]
                got = raw[np.clip(np.arange(4 * N + 1), lo, hi)]
            else:
                got = np.full(4 * N + 1, 1 << (B - 1), np.int32)
            read = np.zeros(4 * N + 1, bool)
            for u in range(4 * n + 1):
                if (reach >> u) & 1:
                    a, b = _unit_range(u, n, N, unit)
                    read[a:b + 1] = True
            if bit:
                simple_checked += 1
                assert np.array_equal(got[read], want[read]), (N, luma, mode, flags, hex(A))
            else:
                general_differs += not np.array_equal(got[read], want[read])
    print(f"N={N} luma={luma}: clamp checked on {simple_checked} simple cases; it differs from the oracle in {general_differs} cases without the bit")
    assert simple_checked > 0 and general_differs > 0
