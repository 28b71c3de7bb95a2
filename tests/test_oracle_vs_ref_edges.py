"""Pins the CPU oracle against the compiled reference at the 16-bit edges of the quantisers and the inverse transform:
QP_Y down to -QpBdOffset (per = 0), saturating residuals, 8, 10 and 12 bit.  Every case also counts, with the int64
restatements of tests/extreme_inputs.py, that it reached the edge it is about:
  * the flat level clip to [-32768, 32767] with uiAcSum over the unclipped magnitudes (TComTrQuant.cpp:1250-1258);
  * sign hiding on a clipped level (finalChange = -1, :1076-1081);
  * RDOQ's Int levels above 32767 (:1893-1898, 1945, 2167-2169);
  * the 32-bit wrap of the de-quantiser product at 12 bit (:1346-1353);
  * the normative 16-bit clip after the first inverse stage (:378, 474-499)."""
import ctypes as C

import numpy as np
import pytest

import extreme_inputs as xi
import oracle_lib as ol

pytestmark = pytest.mark.ref
REG_DCT = 65535
# (bit depth, block size) where (32767 * quantScale) >> qbits exceeds 32767 at per 0: qbits = 14 + per + 15 - B - log2 N
CLIP_SHAPES = ((10, 32), (12, 8), (12, 16), (12, 32))


def _qps(B):
    """QP_Y at per 0 and 1 (-QpBdOffset upwards) and a few above."""
    bd = xi.qp_bd_offset(B)
    return [-bd, -bd + 3, -bd + 6, -bd + 9, min(51, -bd + 15)]


@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("N", [4, 8, 16, 32])
def test_flat_quant_clip_and_sbh_at_lowest_qp(B, N):
    """transformNxN (flat xQuant + signBitHidingHDQ, uiAcSum) and invtransformNxN on saturating residuals at per 0 and 1."""
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 1)
    rng = np.random.default_rng(4100 + 7 * N + B)
    bd = xi.qp_bd_offset(B)
    n_clip = n_sbh_clip = n_sbh = 0
    for it in range(60):
        ttype = (0, 2, 3)[it % 3] if N < 32 else 0
        is_intra = it % 5 != 4
        mode = int(rng.integers(0, 35))
        ts = int(N == 4 and it % 6 == 5)
        qpy = int(rng.choice(_qps(B)))
        slice_type = 2 if is_intra else (1, 0)[it % 2]
        kind = xi.RESIDUAL_KINDS[it % len(xi.RESIDUAL_KINDS)]
        resi = xi.saturating_residual(rng, N, B, kind)
        stride = N
        la, sa = np.zeros(N * N, np.int32), C.c_uint32(0)
        R.ref_transformNxN(qpy, slice_type, ttype, int(is_intra), mode, ts, 0, resi.reshape(-1).copy(), stride, la, N, C.byref(sa))
        q = O.hmo_setQPforQuant(qpy, int(ttype != 0), bd, 0)
        scan = O.hmo_coef_scan_idx(N, int(ttype == 0), int(is_intra), mode)
        tmode = mode if (ttype == 0 and is_intra) else REG_DCT
        cfg = ol.quant_cfg(q.per, q.rem, intra_slice=int(slice_type == 2), sign_hide=1, scan_idx=scan)
        lb, sb = ol.o_transformNxN(resi, N, B, tmode, ts, cfg)
        assert np.array_equal(la.reshape(N, N), lb), (it, kind, qpy)
        assert sa.value == sb, (it, kind, qpy)  # uiAcSum of the unclipped magnitudes
        # the edges this case reached
        coef = np.zeros(N * N, np.int32)
        if ts:
            O.hmo_xTransformSkip(resi.reshape(-1), N, coef, N, B)
        else:
            O.hmo_xT(tmode, resi.reshape(-1), N, coef, N, B)
        unclipped = xi.flat_levels_unclipped(coef, N, B, q.per, q.rem, slice_type == 2)
        n_clip += xi.count_flat_clip(coef, N, B, q.per, q.rem, slice_type == 2)
        cfg0 = ol.quant_cfg(q.per, q.rem, intra_slice=int(slice_type == 2), sign_hide=0, scan_idx=scan)
        lc, sc = ol.o_transformNxN(resi, N, B, tmode, ts, cfg0)
        assert sc == sb == int(np.abs(unclipped).sum())
        n_sbh += int(not np.array_equal(lb, lc))
        n_sbh_clip += xi.count_sbh_on_clipped(lb, lc)
        # the inverse of the clipped levels
        ra, rb = np.zeros(N * N, np.int16), np.zeros(N * N, np.int16)
        R.ref_invtransformNxN(qpy, ttype, 0, tmode, ra, N, la.copy(), N, ts)
        rb = ol.o_invtransformNxN(lb, N, B, tmode, q.per, q.rem, ts)
        assert np.array_equal(ra.reshape(N, N), rb), (it, kind, qpy)
    # blocks where sign hiding lands on a clipped level are rare in random draws: add the ones a search over the oracle finds
    for resi, qpy, mode in xi.search_sbh_on_clip(rng, N, B) if (B, N) in CLIP_SHAPES else []:
        la, sa = np.zeros(N * N, np.int32), C.c_uint32(0)
        R.ref_transformNxN(qpy, 2, 0, 1, mode, 0, 0, resi.reshape(-1).copy(), N, la, N, C.byref(sa))
        q = O.hmo_setQPforQuant(qpy, 0, bd, 0)
        scan = O.hmo_coef_scan_idx(N, 1, 1, mode)
        lb, sb = ol.o_transformNxN(resi, N, B, mode, 0, ol.quant_cfg(q.per, q.rem, 1, 1, scan))
        lc, _ = ol.o_transformNxN(resi, N, B, mode, 0, ol.quant_cfg(q.per, q.rem, 1, 0, scan))
        assert np.array_equal(la.reshape(N, N), lb) and sa.value == sb, (qpy, mode)
        n_sbh_clip += xi.count_sbh_on_clipped(lb, lc)
    assert n_sbh > 0
    if (B, N) in CLIP_SHAPES:
        assert n_clip > 0, "no level reached the clip"
        assert n_sbh_clip > 0, "sign hiding never landed on a clipped level"


@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("N", [4, 8, 16, 32])
def test_dequant_and_inverse_on_synthetic_levels(B, N):
    """xDeQuant on every QP remainder and the wrap QPs, and invtransformNxN (DCT, 4x4 DST, transform skip) on synthetic levels:
    extreme single levels, dense full-range int16, columns that overflow the first inverse stage, values outside int16."""
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 1)
    rng = np.random.default_rng(5200 + 7 * N + B)
    bd = xi.qp_bd_offset(B)
    qps = sorted(set([-bd + k for k in range(6)] + [40, 45, 46, 51]))
    n_wrap = n_first = 0
    for it in range(len(qps) * len(xi.LEVEL_KINDS)):
        qpy = qps[it % len(qps)]
        kind = xi.LEVEL_KINDS[(it // len(qps)) % len(xi.LEVEL_KINDS)]
        lv = xi.synthetic_levels(rng, N, kind).reshape(-1)
        out = np.zeros(3, np.int32)
        R.ref_setQPforQuant(qpy, 0, bd, 0, out)
        per, rem = int(out[1]), int(out[2])
        a, b = np.zeros(N * N, np.int32), np.zeros(N * N, np.int32)
        R.ref_xDeQuant(qpy, 0, bd, 0, lv.copy(), a, N)
        O.hmo_xDeQuant(lv, b, N, B, per, rem)
        assert np.array_equal(a, b), (qpy, kind)
        nw = xi.count_dequant_wrap(lv, N, B, per, rem)
        n_wrap += nw
        if nw == 0:  # without a wrap the de-quantiser is the int64 formula
            assert np.array_equal(b, xi.dequant_int64(lv, N, B, per, rem))
        for tmode, ts in ((REG_DCT, 0), (int(rng.integers(0, 35)), 0), (REG_DCT, 1)):
            if ts and N != 4:
                continue
            use_dst = N == 4 and tmode != REG_DCT and not ts
            if not ts:
                n_first += xi.count_first_stage_clip(b, N, use_dst)
            ra = np.zeros(N * N, np.int16)
            R.ref_invtransformNxN(qpy, 0, 0, tmode, ra, N, lv.copy(), N, ts)
            rb = ol.o_invtransformNxN(lv, N, B, tmode, per, rem, ts)
            assert np.array_equal(ra.reshape(N, N), rb), (qpy, kind, tmode, ts)
    assert n_first > 0, "no block clipped after the first inverse stage"
    if B == 12:
        assert n_wrap > 0, "no de-quantiser product wrapped"


@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("N", [4, 8, 16, 32])
def test_rdoq_levels_above_int16(B, N):
    """xRateDistOptQuant at per 0 and 1 on saturating residuals: Int levels, not clipped, and the absolute sum."""
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 1)
    rng = np.random.default_rng(6300 + 7 * N + B)
    bd = xi.qp_bd_offset(B)
    n_wide = 0
    for it in range(24):
        ttype = (0, 2, 3)[it % 3] if N < 32 else 0
        is_intra = it % 4 != 3
        mode = int(rng.integers(0, 35))
        tr_idx = int(rng.integers(0, 2))
        qpy = int(rng.choice(_qps(B)[:3]))
        slice_type = 2 if is_intra else (1, 0)[it % 2]
        lam = float(rng.choice([0.5, 3.0, 17.5, 140.25]))
        resi = xi.saturating_residual(rng, N, B, xi.RESIDUAL_KINDS[it % len(xi.RESIDUAL_KINDS)])
        coef = np.zeros(N * N, np.int32)
        tmode = mode if (ttype == 0 and is_intra) else REG_DCT
        O.hmo_xT(tmode, resi.reshape(-1), N, coef, N, B)
        est = ol.make_est_bits(rng)
        la, sa = ol.r_rdoq(coef, N, qpy, slice_type, ttype, int(is_intra), mode, tr_idx, lam, est)
        q = O.hmo_setQPforQuant(qpy, int(ttype != 0), bd, 0)
        scan = O.hmo_coef_scan_idx(N, int(ttype == 0), int(is_intra), mode)
        root = int((not is_intra) and ttype == 0 and tr_idx == 0)
        cfg = ol.RdoqCfg(q.per, q.rem, int(ttype == 0), int(is_intra), scan, root, R.ref_cbf_ctx(ttype, tr_idx), 1, lam)
        lb, sb = ol.o_rdoq(coef, N, B, cfg, est)
        assert np.array_equal(la, lb), (it, qpy, np.argwhere(la != lb)[:4])
        assert sa == sb
        n_wide += int(np.count_nonzero(np.abs(la.astype(np.int64)) > xi.INT16_MAX))
    if (B, N) in CLIP_SHAPES:
        assert n_wide > 0, "no RDOQ level exceeded 16 bits"
