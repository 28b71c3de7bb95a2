"""Numpy restatement of the WEIGHTED distortions of the reference encoder's motion search, for the tests of hmx_getSADw,
hmx_getHADsw and the four _wp search entries.  In a slice whose PPS has getUseWP() (P) or getWPBiPred() (B),
TEncSearch::setWpScalingDistParam (TEncSearch.cpp:6183-6215) sets DistParam::bApplyWeight before the integer stage, and every
xGetSAD* then returns xGetSADw, xGetHADs returns xGetHADsw (TComRdCostWeightPrediction.cpp:69-104, :196-561).

  entry        (w0, round, shift, offset) of a luma wpScalingParam: getWpScaling's uni-directional branch
               (TComWeightPrediction.cpp:302-312) -- only one index is >= 0 in setWpScalingDistParam, also for bBi calls
  weigh        the sample map pred = (Pel)(((w0 * c + round) >> shift) + offset): the product in Int, the assignment wraps to
               16 bits, no clip
  sad_w        xGetSADw: every row, whatever iSubShift says, >> (B - 8)
  hads_w       xGetHADsw: subpel_oracle.measure (the pinned calcHAD: same sub-block rule, butterflies and per-sub-block rounding
               as xCalcHADs4x4w / 8x8w) on the weighted prediction
  cost_map / search        xPatternSearch with sad_w, winner by me_oracle.winner
  tz_search                xTZSearch: tz_oracle.walk over the weighted cost
  stage_costs / refine     xPatternSearchFracDIF: subpel_oracle.measure on weigh(subpel_oracle.predict(...))

Everything is UInt arithmetic modulo 2^32.  The vector-cost terms, the tie rules, the TZ walk and ruiSAD = best - vector cost are
those of the unweighted oracles and are taken from them.  tests/test_me_wp_oracle.py holds the second, literal construction;
tests/test_me_wp_enc_tap.py pins this module on calls recorded inside the reference encoder."""
import numpy as np

import me_oracle as mo
import subpel_oracle as so
import tz_oracle as tzo

M32 = mo.M32


def entry(weight, offset, log2_denom, B):
    """(w0, round, shift, offset) from (iWeight, iOffset, uiLog2WeightDenom)."""
    d = int(log2_denom)
    return int(weight), (1 << (d - 1)) if d else 0, d, int(offset) * (1 << (B - 8))


def default_entry(log2_denom=0):
    """(weight, offset, log2_denom) that leaves every sample in [0, 2^B) unchanged."""
    return 1 << log2_denom, 0, log2_denom


def weigh(cur, e):
    """The weighted samples of an integer array, as int16 (the wrap of the assignment to Pel)."""
    w0, rnd, shift, off = e
    v = ((w0 * np.asarray(cur).astype(np.int64) + rnd) >> shift) + off
    return ((v + 32768) % 65536 - 32768).astype(np.int16)


def sad_w(org, cur, e, B, sub_shift=0):
    """xGetSADw of one block; sub_shift is accepted and ignored, as the reference ignores iSubShift."""
    s = int(np.abs(np.asarray(org).astype(np.int64) - weigh(cur, e)).sum()) & M32
    return s >> (B - 8)


def hads_w(org, cur, e, B):
    """xGetHADsw of one block (cur: the final, clipped prediction samples)."""
    return so.measure(np.asarray(org), weigh(cur, e), B, 1)


def measure_w(org_block, pred, e, B, use_had):
    return hads_w(org_block, pred, e, B) if use_had else sad_w(org_block, pred, e, B)


def cost_map(org, ref, margin, u, lam, B, e):
    """me_oracle.cost_map under weighting: (bottom - top + 1, right - left + 1) uint32; u["sub_shift"] has no effect."""
    x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
    l, t, r, b = int(u["left"]), int(u["top"]), int(u["right"]), int(u["bottom"])
    px, py = int(u["pred_x"]), int(u["pred_y"])
    ob = np.asarray(org)[y:y + h, x:x + w].astype(np.int64)
    X0, Y0 = margin[0] + x, margin[1] + y
    win = weigh(ref[Y0 + t:Y0 + b + h, X0 + l:X0 + r + w], e).astype(np.int64)  # a sample's weight does not depend on the candidate
    out = np.zeros((b - t + 1, r - l + 1), np.uint32)
    for j in range(b - t + 1):
        rows = win[j:j + h]
        for i in range(r - l + 1):
            sd = (int(np.abs(ob - rows[:, i:i + w]).sum()) & M32) >> (B - 8)
            out[j, i] = (sd + mo.mv_cost(lam, l + i, t + j, px, py, 2)) & M32
    return out


def search(org, ref, margin, u, lam, B, e):
    """((mvx, mvy, sad, cost), cost map) of xPatternSearch under weighting."""
    m = cost_map(org, ref, margin, u, lam, B, e)
    return mo.winner(m, u, lam), m


def cost_fn(org, ref, margin, u, lam, B, e):
    """cost(x, y) of xTZSearchHelp under weighting, memoised: xGetSADw reads every row although iSubShift may be 1."""
    x0, y0, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
    px, py = int(u["pred_x"]), int(u["pred_y"])
    ob = np.asarray(org)[y0:y0 + h, x0:x0 + w]
    X0, Y0 = margin[0] + x0, margin[1] + y0
    memo = {}

    def cost(x, y):
        if (x, y) not in memo:
            assert Y0 + y >= 0 and X0 + x >= 0 and Y0 + y + h <= ref.shape[0] and X0 + x + w <= ref.shape[1]
            memo[(x, y)] = (sad_w(ob, ref[Y0 + y:Y0 + y + h, X0 + x:X0 + x + w], e, B) + mo.mv_cost(lam, x, y, px, py, 2)) & M32
        return memo[(x, y)]
    return cost


def tz_search(org, ref, margin, u, z, lam, B, e, max_passes=tzo.PASS_CAP):
    """tz_oracle.search under weighting: ((mvx, mvy, sad, cost), trace, passes, labels)."""
    box = (int(u["left"]), int(u["top"]), int(u["right"]), int(u["bottom"]))
    w = tzo.walk(cost_fn(org, ref, margin, u, lam, B, e), box, (int(z["start_x"]), int(z["start_y"])), int(z["range"]), max_passes)
    if w.capped:
        res = (w.bx, w.by, M32, M32)
    else:
        res = (w.bx, w.by, (w.best - mo.mv_cost(lam, w.bx, w.by, int(u["pred_x"]), int(u["pred_y"]), 2)) & M32, w.best)
    return res, w.trace, w.passes, w.labels


def dist(org_block, ref, X, Y, mvx, mvy, B, use_had, e):
    """The weighted distortion of the candidate at (mvx, mvy) quarter samples from (X, Y) (positions as in subpel_oracle)."""
    h, w = org_block.shape
    return measure_w(org_block, so.predict(ref, X, Y, w, h, mvx, mvy, B), e, B, use_had)


def stage_costs(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, e, half=None):
    """subpel_oracle.stage_costs under weighting."""
    out = []
    for (dx, dy) in (so.REFINE_H if half is None else so.REFINE_Q):
        if half is None:
            d = dist(org_block, ref, X, Y, 2 * dx, 2 * dy, B, use_had, e)
            out.append((d + mo.mv_cost(lam, 2 * ix + dx, 2 * iy + dy, pred[0], pred[1], 1)) & M32)
        else:
            bx, by = 2 * half[0], 2 * half[1]
            d = dist(org_block, ref, X, Y, bx + dx, by + dy, B, use_had, e)
            out.append((d + mo.mv_cost(lam, 4 * ix + bx + dx, 4 * iy + by + dy, pred[0], pred[1], 0)) & M32)
    return out


def refine(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, e):
    """subpel_oracle.refine under weighting: ((mvx, mvy, dist, cost), the 18 stage costs, (half winner, quarter winner))."""
    ch = stage_costs(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, e)
    half = so.REFINE_H[int(np.argmin(ch))]
    cq = stage_costs(org_block, ref, X, Y, B, use_had, lam, pred, ix, iy, e, half)
    k = int(np.argmin(cq))
    q = so.REFINE_Q[k]
    mvx, mvy = 4 * ix + 2 * half[0] + q[0], 4 * iy + 2 * half[1] + q[1]
    return (mvx, mvy, (cq[k] - mo.mv_cost(lam, mvx, mvy, pred[0], pred[1], 0)) & M32, cq[k]), ch + cq, (half, q)


def refine_unit(org, ref, margin, u, ix, iy, lam, B, use_had, e):
    x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
    return refine(np.asarray(org)[y:y + h, x:x + w], ref, margin[0] + x + ix, margin[1] + y + iy, B, use_had, lam,
                  (int(u["pred_x"]), int(u["pred_y"])), ix, iy, e)
