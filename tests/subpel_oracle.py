"""Numpy restatement of the fractional motion refinement of the reference encoder, for the tests of hmx_batch_subpel_search:

  dist         the distortion of one candidate: filterHorLuma(isLast = false) over height + 7 rows, filterVerLuma(isFirst =
               false, isLast = true), then calcHAD or the SAD -- made with the pinned CPU oracle (oracle/hmx_oracle.c) exactly
               as tests/test_gpu_parity.py::test_batch_subpel_cost makes it; a function of the candidate's position alone
  planes       a second construction: the sixteen m_filteredBlock planes as xExtDIFUpSamplingH / Q (TEncSearch.cpp:5982-6175)
               build them, with their source offsets for the half-sample winner; plane_block reads a candidate with
               xPatternRefinement's pointer adjustments (:734-740)
  refine       xPatternSearchFracDIF (:4476-4514): the two stages of xPatternRefinement (:711-760) with me_oracle.mv_cost
  refine_loop  the same candidate by candidate: uiDistBest = MAX_UINT, strict <, the halving loop of the bits
  me_tail      the tail of xMotionEstimation (:4197-4205)

tests/test_me_enc_tap.py pins stage_costs, refine and me_tail on the reference encoder's own calls (tests/golden/me_enc_tap.npz:
all eighteen uiDist of the two xPatternRefinement calls, rcMvHalf, rcMvQter, ruiBits and ruiCost).

Everything is UInt arithmetic modulo 2^32.  Positions: `ref` is a luma plane WITH its margins, (X, Y) the position in it of
the block displaced by the integer vector."""
import ctypes as C
import math

import numpy as np

import me_oracle as mo
import oracle_lib as ol

M32 = mo.M32
REFINE_H = ((0, 0), (0, -1), (0, 1), (-1, 0), (1, 0), (-1, -1), (1, -1), (-1, 1), (1, 1))  # s_acMvRefineH (:47-58)
REFINE_Q = ((0, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (1, 1))  # s_acMvRefineQ (:60-71)


def _oracle():
    O = ol.oracle()
    O.hmo_calcHAD.restype = C.c_uint32
    return O


def _hor(src, y0, x0, w, h, frac, B):
    """filterHorLuma(isLast = false) of h rows and w columns of the 2-D int16 array src from (y0, x0)."""
    assert y0 >= 0 and x0 - 3 >= 0 and y0 + h <= src.shape[0] and x0 + w + 4 <= src.shape[1]
    out = np.zeros((h, w), np.int16)
    _oracle().hmo_filterHorLuma(ol.ptr(src.reshape(-1), y0 * src.shape[1] + x0), src.shape[1], ol.ptr(out.reshape(-1)), w, w, h, frac, 0, B)
    return out


def _ver(tmp, r0, c0, w, h, frac, B):
    """filterVerLuma(isFirst = false, isLast = true) of h rows and w columns of the intermediate tmp from (r0, c0)."""
    lo, hi = (3, 4) if frac else (0, 0)
    assert r0 - lo >= 0 and r0 + h + hi <= tmp.shape[0] and c0 >= 0 and c0 + w <= tmp.shape[1], (r0, c0, w, h, frac, tmp.shape)
    out = np.zeros((h, w), np.int16)
    _oracle().hmo_filterVerLuma(ol.ptr(tmp.reshape(-1), r0 * tmp.shape[1] + c0), tmp.shape[1], ol.ptr(out.reshape(-1)), w, w, h, frac, 0, 1, B)
    return out


def measure(org_block, pred, B, use_had):
    """xGetHADs (8x8 sub-blocks, 4x4 when a side is no multiple of 8) or xGetSAD, iSubShift = 0, >> (B - 8)."""
    h, w = org_block.shape
    ob, pr = np.ascontiguousarray(org_block, np.int16), np.ascontiguousarray(pred, np.int16)
    if use_had:
        return int(_oracle().hmo_calcHAD(ob.ctypes.data_as(C.c_void_p), w, pr.ctypes.data_as(C.c_void_p), w, w, h, B))
    return (int(np.abs(ob.astype(np.int64) - pr).sum()) & M32) >> (B - 8)


def predict(ref, X, Y, w, h, mvx, mvy, B):
    """The two-stage prediction at (mvx, mvy) quarter samples from (X, Y)."""
    ref = np.ascontiguousarray(ref, np.int16)
    tmp = _hor(ref, Y + (mvy >> 2) - 3, X + (mvx >> 2), w, h + 7, mvx & 3, B)
    return _ver(tmp, 3, 0, w, h, mvy & 3, B)


def dist(org_block, ref, X, Y, mvx, mvy, B, use_had):
    h, w = org_block.shape
    return measure(org_block, predict(ref, X, Y, w, h, mvx, mvy, B), B, use_had)


def planes(ref, X, Y, w, h, B, half=None):
    """m_filteredBlock[ver & 3][hor & 3] as a dict {(v, h): 2-D array}: after xExtDIFUpSamplingH, and with half = (hx, hy), the
    half-sample winner, also after xExtDIFUpSamplingQ.  Planes the reference leaves stale are absent."""
    ref = np.ascontiguousarray(ref, np.int16)
    t0 = _hor(ref, Y - 4, X - 1, w + 1, h + 8, 0, B)  # m_filteredBlockTmp[0], srcPtr = ROIY - 4 * stride - 1
    t2 = _hor(ref, Y - 4, X - 1, w + 1, h + 8, 2, B)
    fb = {(0, 0): _ver(t0, 4, 1, w, h, 0, B), (2, 0): _ver(t0, 3, 1, w, h + 1, 2, B),
          (0, 2): _ver(t2, 4, 0, w + 1, h, 0, B), (2, 2): _ver(t2, 3, 0, w + 1, h + 1, 2, B)}
    if half is None:
        return fb
    hx, hy = half
    ext = h + 8 if hy == 0 else h + 7
    t1 = _hor(ref, Y - 4 + (hy > 0), X - 1 + (hx >= 0), w, ext, 1, B)
    t3 = _hor(ref, Y - 4 + (hy > 0), X - 1 + (hx > 0), w, ext, 3, B)
    fb[(1, 1)] = _ver(t1, 3 + (hy == 0), 0, w, h, 1, B)
    fb[(3, 1)] = _ver(t1, 3, 0, w, h, 3, B)
    if hy != 0:
        fb[(2, 1)] = _ver(t1, 3, 0, w, h, 2, B)  # the reference's "if (ver == 0) intPtr += stride" is dead here
        fb[(2, 3)] = _ver(t3, 3, 0, w, h, 2, B)
    else:
        fb[(0, 1)] = _ver(t1, 4, 0, w, h, 0, B)
        fb[(0, 3)] = _ver(t3, 4, 0, w, h, 0, B)
    if hx != 0:
        fb[(1, 2)] = _ver(t2, 3 + (hy >= 0), int(hx > 0), w, h, 1, B)
        fb[(3, 2)] = _ver(t2, 3 + (hy > 0), int(hx > 0), w, h, 3, B)
    else:
        fb[(1, 0)] = _ver(t0, 3 + (hy >= 0), 1, w, h, 1, B)
        fb[(3, 0)] = _ver(t0, 3 + (hy > 0), 1, w, h, 3, B)
    fb[(1, 3)] = _ver(t3, 3 + (hy == 0), 0, w, h, 1, B)
    fb[(3, 3)] = _ver(t3, 3, 0, w, h, 3, B)
    return fb


def plane_block(fb, w, h, hor_val, ver_val):
    """What xPatternRefinement reads for a candidate (:734-740): horVal, verVal = (table entry + baseRefMv) * iFrac."""
    p = fb[(ver_val & 3, hor_val & 3)]
    c = 1 if (hor_val == 2 and (ver_val & 1) == 0) else 0
    r = 1 if ((hor_val & 1) == 0 and ver_val == 2) else 0
    return p[r:r + h, c:c + w]


def stage_costs(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, half=None):
    """The nine costs of the half stage (half = None) or of the quarter stage around the half-sample winner."""
    out = []
    for (dx, dy) in (REFINE_H if half is None else REFINE_Q):
        if half is None:
            d = dist(org_block, ref, X, Y, 2 * dx, 2 * dy, B, use_had)
            out.append((d + mo.mv_cost(lam, 2 * ix + dx, 2 * iy + dy, pred[0], pred[1], 1)) & M32)
        else:
            bx, by = 2 * half[0], 2 * half[1]
            d = dist(org_block, ref, X, Y, bx + dx, by + dy, B, use_had)
            out.append((d + mo.mv_cost(lam, 4 * ix + bx + dx, 4 * iy + by + dy, pred[0], pred[1], 0)) & M32)
    return out


def refine(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy):
    """((mvx, mvy, dist, cost), the 18 stage costs, (half winner, quarter winner))."""
    ch = stage_costs(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy)
    half = REFINE_H[int(np.argmin(ch))]  # numpy returns the first occurrence of the minimum
    cq = stage_costs(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, half)
    k = int(np.argmin(cq))
    q = REFINE_Q[k]
    mvx, mvy = 4 * ix + 2 * half[0] + q[0], 4 * iy + 2 * half[1] + q[1]
    return (mvx, mvy, (cq[k] - mo.mv_cost(lam, mvx, mvy, pred[0], pred[1], 0)) & M32, cq[k]), ch + cq, (half, q)


def refine_loop(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, use_planes=False):
    """xPatternSearchFracDIF as written; use_planes reads the candidates from `planes` instead of `dist`."""
    h, w = org_block.shape
    costs, frac_mv = [], []
    base = (0, 0)
    for i_frac, table, scale in ((2, REFINE_H, 1), (1, REFINE_Q, 0)):
        mv = (2 * ix, 2 * iy) if i_frac == 2 else (2 * (2 * ix + frac_mv[0][0]), 2 * (2 * iy + frac_mv[0][1]))  # rcMvHalf / rcMvQter going in
        fb = planes(ref, X, Y, w, h, B, None if i_frac == 2 else frac_mv[0]) if use_planes else None
        best, direc = M32, 0
        for i in range(9):
            hv, vv = (table[i][0] + base[0]) * i_frac, (table[i][1] + base[1]) * i_frac
            if use_planes:
                d = measure(org_block, plane_block(fb, w, h, hv, vv), B, use_had)
            else:
                d = dist(org_block, ref, X, Y, hv, vv, B, use_had)
            bits = mo.comp_bits_loop(((table[i][0] + mv[0]) << scale) - pred[0]) + mo.comp_bits_loop(((table[i][1] + mv[1]) << scale) - pred[1])
            d = (d + (((lam * bits) & M32) >> 16)) & M32
            costs.append(d)
            if d < best:
                best, direc = d, i
        frac_mv.append(table[direc])
        base = (frac_mv[0][0] * 2, frac_mv[0][1] * 2)  # baseRefMv = rcMvHalf << 1
    half, q = frac_mv
    mvx, mvy = (ix << 2) + (half[0] << 1) + q[0], (iy << 2) + (half[1] << 1) + q[1]
    bits = mo.comp_bits_loop(mvx - pred[0]) + mo.comp_bits_loop(mvy - pred[1])
    return (mvx, mvy, (best - (((lam * bits) & M32) >> 16)) & M32, best), costs, (half, q)


def refine_unit(org, ref, margin, u, ix, iy, lam, B, use_had):
    """refine for a unit given as hmx_me_unit fields: org the original luma plane, ref the reference's with margins."""
    x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
    return refine(org[y:y + h, x:x + w], ref, margin[0] + x + ix, margin[1] + y + iy, B, use_had, lam, (int(u["pred_x"]), int(u["pred_y"])), ix, iy)


def me_tail(lam, pred, mvx, mvy, cost, bits_in, weight):
    """xMotionEstimation :4197-4205 at cost scale 0: (ruiBits, ruiCost) from the quarter-stage cost."""
    mv_bits = mo.mv_bits(mvx, mvy, pred[0], pred[1], 0)
    bits = (bits_in + mv_bits) & M32
    get_cost = lambda b: ((lam * b) & M32) >> 16
    return bits, int(math.floor(weight * (float(cost) - float(get_cost(mv_bits)))) + float(get_cost(bits))) & M32
