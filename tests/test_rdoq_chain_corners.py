"""RDOQ at the corners the GPU suite holds the whole-picture chain to (tests/test_gpu_rdoq_chain_corners.py), on the CPU:
  * xRateDistOptQuant with sign hiding OFF, the oracle against the compiled reference -- every other RDOQ test of the suite
    runs with the flag on, so the oracle's own sign_hide == 0 branch was pinned nowhere;
  * the level bound the chain's 16-bit words rest on (extreme_inputs.rdoq_max_level), against the oracle's chain at the
    lowest QP each largest block size allows."""
import numpy as np
import pytest

import extreme_inputs as xi
import oracle_lib as ol

REG_DCT = 65535


@pytest.mark.ref
@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("N", [4, 8, 16, 32])
def test_rdoq_sign_hiding_off_vs_reference(B, N):
    """xRateDistOptQuant with SignHideFlag = 0 (TComTrQuant.cpp:2189): luma and chroma, intra and inter scans, both cbf branches,
    random residuals at ordinary QPs and saturating ones at per 0 and 1; levels and absolute sums.  With the flag on the same
    calls give other levels for some blocks."""
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 0)
    try:
        rng = np.random.default_rng(7400 + 7 * N + B)
        bd, mx = xi.qp_bd_offset(B), (1 << B) - 1
        n_nonzero = n_flag_matters = 0
        for it in range(64):
            ttype = (0, 2, 3)[it % 3] if N < 32 else 0
            is_intra = it % 4 != 3
            mode = int(rng.integers(0, 35))
            tr_idx = int(rng.integers(0, 2))
            slice_type = 2 if is_intra else (1, 0)[it % 2]
            if it % 2:  # the lowest QPs (per 0 and 1) on saturating residuals
                qpy = int(rng.choice([-bd, -bd + 3, -bd + 6, -bd + 9]))
                lam = float(rng.choice([0.05, 0.5, 3.0, 17.5]))
                resi = xi.saturating_residual(rng, N, B, xi.RESIDUAL_KINDS[(it // 2) % len(xi.RESIDUAL_KINDS)]).reshape(-1)
            else:
                qpy = int(rng.choice([10, 22, 27, 32, 37, 45, 51]))
                lam = float(rng.choice([3.0, 17.5, 58.0, 140.25, 900.0]))
                amp = int(rng.choice([4, 20, 60, 200, mx, mx]))
                resi = rng.integers(-amp, amp + 1, N * N).astype(np.int16)
            coef = np.zeros(N * N, np.int32)
            tmode = mode if (ttype == 0 and is_intra) else REG_DCT
            O.hmo_xT(tmode, resi, N, coef, N, B)
            est = ol.make_est_bits(rng)
            la, sa = ol.r_rdoq(coef, N, qpy, slice_type, ttype, int(is_intra), mode, tr_idx, lam, est)
            q = O.hmo_setQPforQuant(qpy, int(ttype != 0), bd, 0)
            scan = O.hmo_coef_scan_idx(N, int(ttype == 0), int(is_intra), mode)
            root = int((not is_intra) and ttype == 0 and tr_idx == 0)
            cbf_ctx = R.ref_cbf_ctx(ttype, tr_idx)
            lb, sb = ol.o_rdoq(coef, N, B, ol.RdoqCfg(q.per, q.rem, int(ttype == 0), int(is_intra), scan, root, cbf_ctx, 0, lam), est)
            assert np.array_equal(la, lb), (it, qpy, np.argwhere(la != lb)[:4])
            assert sa == sb, (it, qpy)
            n_nonzero += int(sa > 0)
            lc, _ = ol.o_rdoq(coef, N, B, ol.RdoqCfg(q.per, q.rem, int(ttype == 0), int(is_intra), scan, root, cbf_ctx, 1, lam), est)
            n_flag_matters += int(not np.array_equal(lb, lc))
        assert n_nonzero >= 16, n_nonzero
        assert n_flag_matters > 0, "sign hiding changed no block of the set: the flag was not shown to matter"
    finally:
        R.ref_init(B, 416, 240, 1)  # the state every other test of the reference expects


@pytest.mark.parametrize("sign_hide", [1, 0])
@pytest.mark.parametrize("B,qp,N", xi.RDOQ_BOUNDARY_CASES)
def test_rdoq_chain_levels_within_bound(B, qp, N, sign_hide):
    """The oracle's chain with RDOQ at the lowest QP_Y at which no block of the plan can exceed 16 bits: every level stays within
    rdoq_max_level of its block, the bound of every block is within int16 -- and luma levels above
    16383 do occur, so the GPU test of the same cases (same inputs) rides in the top bit of the chain's 16-bit words."""
    tus, orgs, ests, lams = xi.rdoq_boundary_case(B, qp, N)
    assert not xi.rdoq_chain_must_refuse(tus, B, qp, 0)
    O = ol.oracle()
    bd = xi.qp_bd_offset(B)
    n_high = 0
    for org in orgs:
        _, lev = ol.o_intra_frame_encode_rdoq(tus, 128, 128, B, qp, org, ests, lams, sign_hide=sign_hide)
        for t in tus:
            n, p, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
            q = O.hmo_setQPforQuant(qp, int(p != 0), bd, 0)
            bound = xi.rdoq_max_level(B, q.per, q.rem, int(t["log2n"]))
            assert bound <= xi.INT16_MAX
            top = int(np.abs(lev[p][y:y + n, x:x + n].astype(np.int64)).max())
            assert top <= bound, (p, x, y, top, bound)
        n_high += int(np.count_nonzero(np.abs(lev[0].astype(np.int64)) > 16383))
    assert n_high > 0, "no luma level above 16383"
