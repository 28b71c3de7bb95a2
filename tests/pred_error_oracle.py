"""The yardstick of hmx_batch_inter_pred_error[_wp], hmx_getInterPredictionError, hmx_mvpIdxBits, hmx_mergeIdxBits and
hmx_checkBestMVP: TEncSearch::xGetInterPredictionError (TLibEncoder/TEncSearch.cpp:3059-3081) and the loops around it, composed
only of pieces that are already held on the reference:

  predict        the luma part of motionCompensation (TComPrediction.cpp:410-540): hmo_predInterLumaBlk of the pinned CPU oracle
                 (final samples for one list, 14-bit for two lists or any weighted candidate), the oracle's addAvg,
                 wp_oracle.weight_uni_vec / weight_bi_vec -- the luma rows of add_weight_uni_vec / add_weight_bi_vec
  distortion     subpel_oracle.measure: hmo_calcHAD (xGetHADs) or the SAD over every row, >> (B - 8), always unweighted
  cost           getCost(UInt) (TComRdCost.h:204): dist + ((lambda * bits) >> 16), UInt arithmetic modulo 2^32
  decide         ruiCost = MAX_UINT, strict < in array order (TEncSearch.cpp:3120, :3139)
  mvp_idx_bits   xGetMvpIdxBits (:3928-3952), merge_idx_bits (:3133-3137), check_best_mvp (xCheckBestMVP, :4012-4055)

No recorder inside the reference encoder exists for these calls, so the yardstick is pinned through the taps the compiled
reference already has (tests/test_pred_error_oracle.py: ref_predInterBlk, ref_addAvg, ref_xWeightedPredictionUni / Bi,
ref_getDistPart with DF_HADS) and carried to the GPU by tests/golden/pred_error_b*.npz.  The SAD has no tap: it rests on
me_oracle.sad and subpel_oracle.measure, which the recorded encoder calls (tests/test_me_enc_tap.py) already pin.

A candidate is a record of capi.PU_DTYPE / oracle_lib.PU_DTYPE fields; `refs` is a list of 2-D int16 luma planes WITH their
margins (mx, my); `org` the original luma plane without margins; wp = None or (l0, l1), per list one wp_oracle entry
(weight[3], offset[3], log2_denom[3]) per reference, l1 possibly None (the unit weight, as hmx_mc_wp documents)."""
import numpy as np

import me_oracle as mo
import oracle_lib as ol
import subpel_oracle as so
import wp_oracle as wo

M32 = mo.M32
SIZES = mo.SIZES
NONE = 0xFFFFFFFF
UNIT_ENTRY = ([1, 1, 1], [0, 0, 0], [0, 0, 0])
AMVP_MAX_NUM_CANDS = 2
MRG_MAX_NUM_CANDS_SIGNALED = 5
CHOICE_DTYPE = np.dtype([("index", "<u4"), ("dist", "<u4"), ("cost", "<u4")])


def lists(u):
    """The used lists of a candidate as (list, reference, mvx, mvy)."""
    use = [(0, int(u["ref0"]), int(u["mv0x"]), int(u["mv0y"])), (1, int(u["ref1"]), int(u["mv1x"]), int(u["mv1y"]))]
    return [t for t in use if t[1] != 255]


def pred_list(ref, margin, x, y, w, h, mvx, mvy, bi, B):
    """xPredInterLumaBlk of one list: final samples (bi = 0) or the 14-bit intermediate (bi = 1)."""
    ref = np.ascontiguousarray(ref, np.int16)
    out = np.zeros((h, w), np.int16)
    st = ref.shape[1]
    ol.oracle().hmo_predInterLumaBlk(ol.ptr(ref.reshape(-1), (margin[1] + y) * st + margin[0] + x), st, mvx, mvy, w, h, out.reshape(-1), w, bi, B)
    return out


def add_avg(a, b, B):
    h, w = a.shape
    out = np.zeros((h, w), np.int16)
    ol.oracle().hmo_addAvg(np.ascontiguousarray(a).reshape(-1), w, np.ascontiguousarray(b).reshape(-1), w, out.reshape(-1), w, w, h, B)
    return out


def wp_entry_of(wp, lst, ref):
    t = wp[lst]
    return UNIT_ENTRY if t is None else t[ref]


def predict(u, refs, margin, B, wp=None):
    """The luma prediction of one candidate."""
    x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
    use = lists(u)
    assert use
    mid = wp is not None or len(use) == 2
    p = [pred_list(refs[r], margin, x, y, w, h, mvx, mvy, int(mid), B) for (_, r, mvx, mvy) in use]
    if wp is None:
        return p[0] if len(use) == 1 else add_avg(p[0], p[1], B)
    e = [wp_entry_of(wp, lst, r) for (lst, r, _, _) in use]
    if len(use) == 1:
        return wo.weight_uni_vec(p[0], e[0][0][0], e[0][1][0], e[0][2][0], B)
    return wo.weight_bi_vec(p[0], p[1], e[0][0][0], e[1][0][0], e[0][1][0], e[1][1][0], e[0][2][0], B)


def get_cost(lam, bits):
    return ((int(lam) * int(bits)) & M32) >> 16


def errors(cands, bits, refs, margin, org, lam, B, use_had, wp=None):
    """(dist, cost) of every candidate, uint32 arrays."""
    n = len(cands)
    dist, cost = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i, u in enumerate(cands):
        x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
        d = so.measure(org[y:y + h, x:x + w], predict(u, refs, margin, B, wp), B, use_had)
        dist[i] = d
        cost[i] = (d + get_cost(lam, 0 if bits is None else bits[i])) & M32
    return dist, cost


def decide(dist, cost, group_first):
    """hmx_pred_choice per group: the first strictly smaller than a running best that starts at MAX_UINT."""
    out = np.zeros(len(group_first) - 1, CHOICE_DTYPE)
    for g in range(len(out)):
        best = (NONE, NONE, NONE)
        for k, i in enumerate(range(int(group_first[g]), int(group_first[g + 1]))):
            if int(cost[i]) < best[2]:
                best = (k, int(dist[i]), int(cost[i]))
        out[g] = best
    return out


def mvp_idx_bits(idx, num):
    assert 0 <= idx < num
    if num == 1:
        return 0
    if idx == 0:
        return 1
    return idx + (1 if num - 1 > idx else 0)


def merge_idx_bits(cand, max_signaled=MRG_MAX_NUM_CANDS_SIGNALED):
    return cand + 1 - (1 if cand == max_signaled - 1 else 0)


def check_best_mvp(lam, mvx, mvy, mvp_cands, mvp_idx, bits, cost):
    """xCheckBestMVP: returns (mvp_idx, bits, cost); the index bits are m_auiMVPIdxCost[i][AMVP_MAX_NUM_CANDS]."""
    n = len(mvp_cands)
    if n < 2:
        return mvp_idx, bits & M32, cost & M32
    total = [mo.mv_bits(mvx, mvy, int(c[0]), int(c[1]), 0) + mvp_idx_bits(i, AMVP_MAX_NUM_CANDS) for i, c in enumerate(mvp_cands)]
    best = mvp_idx
    for i in range(n):
        if i != mvp_idx and total[i] < total[best]:
            best = i
    if best == mvp_idx:
        return mvp_idx, bits & M32, cost & M32
    new_bits = (bits - total[mvp_idx] + total[best]) & M32
    return best, new_bits, (((cost - get_cost(lam, bits)) & M32) + get_cost(lam, new_bits)) & M32
