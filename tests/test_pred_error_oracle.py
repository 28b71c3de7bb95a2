"""tests/pred_error_oracle.py held from two sides (CPU).

1. A literal second construction: the two-stage interpolation sample by sample as TComInterpolationFilter::filter / filterCopy
   and xPredInterLumaBlk's three cases write it (TComInterpolationFilter.cpp:91-244, TComPrediction.cpp:554-601), addAvg and the
   inline weightUnidir / weightBidir per sample, the sub-block Hadamard as a matrix product, and the loops of xMergeEstimation,
   xCheckBestMVP and xGetMvpIdxBits in the reference's statement order.  It must equal the oracle on every size, all 16 phases per
   list, 8 / 10 / 12 bit.
2. The compiled reference (`ref`): ref_set_recon + ref_predInterBlk (bi 0 and 1, once per reference picture), ref_addAvg,
   ref_xWeightedPredictionUni / Bi and ref_getDistPart(hads = 1), which reaches xGetHADs through DF_HADS, give the oracle's
   predictions and Hadamard distortions for uni, bi and weighted candidates -- and they are what the committed vectors hold.
3. The committed vectors (tests/golden/pred_error_b*.npz) against the oracle, on machines without the reference.

The SAD has no tap in the compiled reference: it rests on me_oracle.sad and subpel_oracle.measure, which the recorded encoder calls
(tests/test_me_enc_tap.py) already pin; here it is restated as a plain double loop."""
import numpy as np
import pytest

import me_oracle as mo
import oracle_lib as ol
import pred_error_cases as pc
import pred_error_oracle as po
import wp_oracle as wo

M32 = 0xFFFFFFFF
TAPS = ((0, 0, 0, 64, 0, 0, 0, 0), (-1, 4, -10, 58, 17, -5, 1, 0), (-1, 4, -11, 40, 40, -11, 4, -1), (0, 1, -5, 17, 58, -10, 4, -1))  # m_lumaFilter
OFFS = 8192  # IF_INTERNAL_OFFS
SHAPES = [(4, 8), (8, 4), (12, 16), (16, 12), (24, 32), (32, 24), (48, 64), (64, 48)]


def short(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def clip(v, B):
    return min(max(v, 0), (1 << B) - 1)


def lit_filter(src, y0, x0, step, w, h, frac, first, last, B):
    """filter<8> / filterCopy over w x h outputs; src: 2-D array of Python-readable ints, (y0, x0) the first output's sample,
    step = (dy, dx) of the tap direction.  Returns a list of rows."""
    head = 14 - B
    out = [[0] * w for _ in range(h)]
    if frac == 0:  # filterCopy (:91-145)
        for r in range(h):
            for c in range(w):
                v = int(src[y0 + r][x0 + c])
                if first == last:
                    out[r][c] = v
                elif first:
                    out[r][c] = short((v << head) - OFFS)
                else:
                    out[r][c] = clip(short((v + OFFS + ((1 << (head - 1)) if head else 0)) >> head), B)
        return out
    shift = 6  # filter (:160-244)
    if last:
        shift += 0 if first else head
        offset = (1 << (shift - 1)) + (0 if first else OFFS << 6)
    else:
        shift -= head if first else 0
        offset = -(OFFS << shift) if first else 0
    taps = np.array(TAPS[frac], np.int64)
    arr = np.asarray(src, np.int64)
    for r in range(h):
        for c in range(w):
            yy, xx = y0 + r - 3 * step[0], x0 + c - 3 * step[1]
            col = arr[yy:yy + 8, xx] if step[0] else arr[yy, xx:xx + 8]
            v = short((int(col @ taps) + offset) >> shift)
            out[r][c] = clip(v, B) if last else v
    return out


def lit_pred_list(ref, margin, x, y, w, h, mvx, mvy, bi, B):
    """xPredInterLumaBlk (TComPrediction.cpp:554-601)."""
    xf, yf, X, Y = mvx & 3, mvy & 3, margin[0] + x + (mvx >> 2), margin[1] + y + (mvy >> 2)
    if yf == 0:
        return lit_filter(ref, Y, X, (0, 1), w, h, xf, True, not bi, B)
    if xf == 0:
        return lit_filter(ref, Y, X, (1, 0), w, h, yf, True, not bi, B)
    tmp = lit_filter(ref, Y - 3, X, (0, 1), w, h + 7, xf, True, False, B)
    return lit_filter(tmp, 3, 0, (1, 0), w, h, yf, False, not bi, B)


def lit_predict(u, refs, margin, B, wp=None):
    x, y, w, h = (int(u[k]) for k in "xywh")
    use = po.lists(u)
    mid = wp is not None or len(use) == 2
    p = [lit_pred_list(refs[r], margin, x, y, w, h, mvx, mvy, mid, B) for (_, r, mvx, mvy) in use]
    out = np.zeros((h, w), np.int16)
    if wp is not None:
        e = {lst: po.wp_entry_of(wp, lst, r) for (lst, r, _, _) in use}
        s = wo.get_wp_scaling(e.get(0), e.get(1), B)[0]  # getWpScaling: list 0's denominator and the summed offsets for two lists
        shift = s["shift"] + 14 - B
        rnd = (1 << (shift - 1)) if shift else 0
    for r in range(h):
        for c in range(w):
            if wp is None and len(use) == 1:
                out[r, c] = p[0][r][c]
            elif wp is None:  # TComYuv::addAvg (:539-540)
                out[r, c] = clip((p[0][r][c] + p[1][r][c] + (1 << (14 - B)) + 2 * OFFS) >> (15 - B), B)
            elif len(use) == 1:
                out[r, c] = wo.weight_unidir(s["w0"], p[0][r][c], rnd, shift, s["offset"], B)
            else:
                out[r, c] = wo.weight_bidir(s["w0"], p[0][r][c], s["w1"], p[1][r][c], rnd, shift, s["offset"], B)
    return out


def hadamard(n):
    m = np.array([[1]], np.int64)
    while len(m) < n:
        m = np.block([[m, m], [m, -m]])
    return m


def lit_measure(org, pred, B, use_had):
    """xGetHADs (TComRdCost.cpp:2186-2283): 8x8 sub-blocks when both sides are multiples of 8, else 4x4; xCalcHADs8x8 returns
    (sad + 2) >> 2 (:2083), xCalcHADs4x4 (satd + 1) >> 1 (:1991); xGetSAD: every row.  Both >> g_uiBitIncrement."""
    h, w = org.shape
    d = org.astype(np.int64) - pred.astype(np.int64)
    if not use_had:
        s = 0
        for r in range(h):
            for c in range(w):
                s += abs(int(d[r, c]))
        return (s & M32) >> (B - 8)
    n = 8 if (w % 8 == 0 and h % 8 == 0) else 4
    H = hadamard(n)
    s = 0
    for y in range(0, h, n):
        for x in range(0, w, n):
            t = int(np.abs(H @ d[y:y + n, x:x + n] @ H.T).sum())
            s += (t + 2) >> 2 if n == 8 else (t + 1) >> 1
    return (s & M32) >> (B - 8)


def lit_mvp_idx_bits(idx, num):  # xGetMvpIdxBits (:3928-3952), statement by statement
    assert idx >= 0 and num >= 0 and idx < num
    if num == 1:
        return 0
    length = 1
    temp = idx
    if temp == 0:
        return length
    code_last = num - 1 > temp
    length += temp - 1
    if code_last:
        length += 1
    return length


def lit_merge_estimation(errs, lam, n_valid):
    """The loop of xMergeEstimation (:3120-3148) over the candidates' errors: (merge index, cost) -- (None, MAX_UINT) when no
    candidate gets below MAX_UINT."""
    cost, index = M32, None
    for cand in range(n_valid):
        cost_cand = errs[cand]
        bits_cand = cand + 1
        if cand == po.MRG_MAX_NUM_CANDS_SIGNALED - 1:
            bits_cand -= 1
        cost_cand = (cost_cand + (((lam * bits_cand) & M32) >> 16)) & M32
        if cost_cand < cost:
            cost, index = cost_cand, cand
    return index, cost


def lit_check_best_mvp(lam, mv, cands, idx, bits, cost):  # xCheckBestMVP (:4012-4055)
    if len(cands) < 2:
        return idx, bits, cost
    idx_cost = [[lit_mvp_idx_bits(i, n) if i < n else 0x7FFFFFFF for n in range(3)] for i in range(2)]  # m_auiMVPIdxCost (:219-227)
    best = idx
    org_bits = mo.comp_bits_loop(mv[0] - cands[idx][0]) + mo.comp_bits_loop(mv[1] - cands[idx][1]) + idx_cost[idx][2]
    best_bits = org_bits
    for i in range(len(cands)):
        if i == idx:
            continue
        b = mo.comp_bits_loop(mv[0] - cands[i][0]) + mo.comp_bits_loop(mv[1] - cands[i][1]) + idx_cost[i][2]
        if b < best_bits:
            best_bits, best = b, i
    if best != idx:
        org = bits
        bits = (org - org_bits + best_bits) & M32
        cost = (((cost - (((lam * org) & M32) >> 16)) & M32) + (((lam * bits) & M32) >> 16)) & M32
    return best, bits, cost


def make_pictures(rng, B, w=96, h=80, m=80):
    refs = [rng.integers(0, 1 << B, (h + 2 * m, w + 2 * m)).astype(np.int16) for _ in range(2)]
    org = rng.integers(0, 1 << B, (h, w)).astype(np.int16)
    return refs, org, (m, m)


@pytest.mark.parametrize("B", [8, 10, 12])
def test_literal_equals_oracle(B):
    rng = np.random.default_rng(7400 + B)
    refs, org, margin = make_pictures(rng, B)
    l0, l1 = [wo.random_entry(rng) for _ in range(2)], [wo.random_entry(rng) for _ in range(2)]
    phases = [set(), set()]
    n = 0
    for (w, h) in SHAPES:
        x, y = int(rng.integers(0, (96 - w) // 4 + 1)) * 4, int(rng.integers(0, (80 - h) // 4 + 1)) * 4
        for k in range(16):
            ph = (k, (5 * k + 3) % 16)  # both lists walk all 16 phases
            mv = [mo.clip_mv(4 * int(rng.integers(-90, 91)) + (p & 3), 4 * int(rng.integers(-90, 91)) + (p >> 2), x, y, 96, 80, 64) for p in ph]
            kind = ("bi", "l0", "l1", "bi")[k % 4] if w * h > 1024 else "all"
            for use in (("l0", "l1", "bi") if kind == "all" else (kind,)):
                u = np.zeros(1, ol.PU_DTYPE)[0]
                u["x"], u["y"], u["w"], u["h"] = x, y, w, h
                u["ref0"], u["ref1"] = (255 if use == "l1" else k % 2), (255 if use == "l0" else (k // 2) % 2)
                u["mv0x"], u["mv0y"], u["mv1x"], u["mv1y"] = mv[0][0], mv[0][1], mv[1][0], mv[1][1]
                for lst, _, mvx, mvy in po.lists(u):
                    phases[lst].add((mvx & 3, mvy & 3))
                for wp in (None, (l0, l1), (l0, None)) if (k % 4 == 1 or w * h <= 64) else (None,):
                    want = po.predict(u, refs, margin, B, wp)
                    got = lit_predict(u, refs, margin, B, wp)
                    assert np.array_equal(got, want), (B, w, h, k, use, wp is not None)
                    ob = org[y:y + h, x:x + w]
                    for use_had in (1, 0):
                        assert lit_measure(ob, got, B, use_had) == po.so.measure(ob, want, B, use_had), (B, w, h, k, use, use_had)
                    n += 1
    assert len(phases[0]) == 16 and len(phases[1]) == 16
    assert {s[0] for s in SHAPES} == set(mo.SIZES) == {s[1] for s in SHAPES}
    assert n >= 8 * 16


def test_helpers_literal():
    for num in (1, 2, 3):
        for idx in range(num):
            assert po.mvp_idx_bits(idx, num) == lit_mvp_idx_bits(idx, num)
    assert [po.merge_idx_bits(i) for i in range(5)] == [1, 2, 3, 4, 4]
    assert [po.merge_idx_bits(i, 3) for i in range(3)] == [1, 2, 2]
    rng = np.random.default_rng(7410)
    changed = wrapped = 0
    for k in range(2000):
        n = int(rng.integers(0, 3))
        cands = [(int(rng.integers(-300, 301)), int(rng.integers(-300, 301))) for _ in range(n)]
        if n == 2 and k % 5 == 0:
            cands[1] = cands[0]  # equal bits: the later candidate must not win
        idx = int(rng.integers(0, max(n, 1)))
        mv = (int(rng.integers(-300, 301)), int(rng.integers(-300, 301)))
        lam = int(rng.integers(0, 1 << 32)) if k % 2 else int(rng.integers(0, 1 << 20))
        bits, cost = int(rng.integers(0, 1 << 12)), int(rng.integers(0, 1 << 32)) if k % 3 == 0 else int(rng.integers(0, 1 << 16))
        got = po.check_best_mvp(lam, mv[0], mv[1], cands, idx, bits, cost)
        assert got == lit_check_best_mvp(lam, mv, cands, idx, bits, cost), k
        changed += n == 2 and got[0] != idx
        wrapped += n == 2 and got[0] != idx and cost - (((lam * bits) & M32) >> 16) < 0
    assert changed > 100 and wrapped > 10


def test_merge_loop_literal():
    """decide over one group with the merge bits equals the reference's loop, ties and MAX_UINT included."""
    rng = np.random.default_rng(7420)
    ties = none = 0
    for k in range(500):
        n = int(rng.integers(0, 6))
        errs = [int(v) for v in rng.integers(0, 50, n)] if k % 3 else [M32 - int(v) for v in rng.integers(0, 3, n)]
        lam = (1 << 16) * int(rng.integers(0, 3)) if k % 2 else int(rng.integers(0, 1 << 32))
        bits = [po.merge_idx_bits(i) for i in range(n)]
        cost = np.array([(e + po.get_cost(lam, b)) & M32 for e, b in zip(errs, bits)], np.uint32)
        best = po.decide(np.array(errs, np.uint32), cost, [0, n])[0]
        index, c = lit_merge_estimation(errs, lam, n)
        assert (None if int(best["index"]) == po.NONE else int(best["index"]), int(best["cost"])) == (index, c), k
        ties += n > 1 and len(set(cost.tolist())) < n
        none += index is None
    assert ties > 20 and none > 5


@pytest.mark.ref
@pytest.mark.parametrize("B", [8, 10, 12])
def test_oracle_on_compiled_reference(B):
    """The oracle's predictions and Hadamard distortions are the compiled reference's, for uni, bi and weighted candidates; and
    the committed vectors are what the reference gives today."""
    S = pc.scene(B)
    count = pc.check_scene(S)
    preds, hads = pc.ref_results(S, B)
    ext, margin = pc.extended(S), (pc.MARGIN, pc.MARGIN)
    for i, u in enumerate(S["cands"]):
        wp = (S["l0"], S["l1"]) if S["weighted"][i] else None
        assert np.array_equal(po.predict(u, ext, margin, B, wp), preds[i]), (B, i, u)
    for flag in (0, 1):  # one call per kind of table: a call is weighted or not as a whole
        sel = np.flatnonzero(S["weighted"] == flag)
        d, _ = po.errors(S["cands"][sel], None, ext, margin, S["org"], 0, B, 1, (S["l0"], S["l1"]) if flag else None)
        assert np.array_equal(d, hads[sel]), (B, flag)
    G = pc.load_vectors(B)
    assert np.array_equal(G["cands"], S["cands"]) and np.array_equal(G["had"], hads) and all(np.array_equal(a, b) for a, b in zip(G["pred"], preds))
    assert sum(count.values()) == len(S["cands"])


@pytest.mark.parametrize("B", [8, 10, 12])
def test_oracle_on_committed_vectors(B):
    S = pc.load_vectors(B)
    pc.check_scene(S)
    ext, margin = pc.extended(S), (pc.MARGIN, pc.MARGIN)
    for i, u in enumerate(S["cands"]):
        wp = (S["l0"], S["l1"]) if S["weighted"][i] else None
        p = po.predict(u, ext, margin, B, wp)
        assert np.array_equal(p, S["pred"][i]), (B, i)
        x, y, w, h = (int(u[k]) for k in "xywh")
        assert po.so.measure(S["org"][y:y + h, x:x + w], p, B, 1) == int(S["had"][i]), (B, i)
