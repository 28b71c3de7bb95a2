"""Oracle of the encoder's weight estimation (TLibEncoder/WeightPredAnalysis.cpp, WP_PARAM_RANGE_LIMIT 1), numpy int64 and Python
floats: what hmx_wp_acdc_multi, hmx_wp_sad_multi, the host helpers and hmx_wp_estimate_slices must give.  It is held by a literal
second construction in tests/test_wp_estimate_oracle.py and by the tables the reference encoder wrote (tests/golden/wp_estimate.npz).

A row is (weight, offset, log2_denom); a table is an int array [entry][component][3] like the wptab* arrays of the stream
fixtures.  An AC/DC value is (ac[3], dc[3]) as Python ints."""
import numpy as np

P_SLICE, B_SLICE = 1, 0  # hmx_slice_type


def acdc(planes):
    """xCalcACDCParamSlice (:71-108): per component dc = (sum + (n >> 1)) / n, ac = sum |x - dc|."""
    ac, dc = [], []
    for p in planes:
        p = np.asarray(p).astype(np.int64)
        n = p.size
        d = (int(p.sum()) + (n >> 1)) // n
        ac.append(int(np.abs(p - d).sum()))
        dc.append(d)
    return ac, dc


def sad_sums(org, rec, row, B):
    """The raw sums of xCalcSADvalueWP (:501-517, before the division by the size) of three planes under `row` ([component][3]) and
    under the default row of the same denominator: int [3][2]."""
    out = []
    for c in range(3):
        w, o, d = (int(v) for v in row[c])
        rd = d + B - 8
        a, b = np.asarray(org[c]).astype(np.int64), np.asarray(rec[c]).astype(np.int64)
        out.append([int(np.abs((a << d) - (b * w + (o << rd))).sum()), int(np.abs((a << d) - (b * (1 << d))).sum())])
    return out


def _clip3(lo, hi, v):
    return lo if v < lo else hi if v > hi else v


def _update(cur, refs, d, B):
    """xUpdatingWPParameters (:252-304) for one list; None = a weight outside the coded range"""
    rd = d + B - 8
    real_offset = 1 << (rd - 1)
    tab = []
    for ref in refs:
        rows = []
        for c in range(3):
            cur_ac, cur_dc, ref_ac, ref_dc = cur[0][c], cur[1][c], ref[0][c], ref[1][c]
            d_weight = 1.0 if ref_ac == 0 else _clip3(-16.0, 15.0, float(cur_ac) / float(ref_ac))
            weight = int(0.5 + d_weight * float(1 << d))
            offset = ((cur_dc << d) - weight * ref_dc + real_offset) >> rd
            if c:
                shift = 1 << (B - 1)
                pred = shift - ((shift * weight) >> d)
                offset = _clip3(-128, 127, _clip3(-512, 511, offset - pred) + pred)
            if not -128 <= (1 << d) - weight <= 127:
                return None
            rows.append([weight, offset, d])
        tab.append(rows)
    return tab


def update_params(cur, refs_l0, refs_l1, B):
    """The denominator loop of xEstimateWPParamSlice (:176-204): (tables of the two lists, denominator reached)."""
    d = 7 if len(refs_l0) > 3 else 6
    while True:
        tabs = [_update(cur, refs, d, B) for refs in (refs_l0, refs_l1)]
        if tabs[0] is not None and tabs[1] is not None:
            return tabs, d
        d -= 1
        assert d >= 3


def select(sums, n_luma, n_chroma, d, rows):
    """The decision of xSelectWP (:333-362) for one entry: (rows, present)."""
    sad_wp = sum(sums[c][0] // (n_chroma if c else n_luma) for c in range(3))
    sad_no = sum(sums[c][1] // (n_chroma if c else n_luma) for c in range(3))
    with np.errstate(all="ignore"):
        ratio = np.float64(sad_wp) / np.float64(sad_no)
    if ratio >= 0.99:  # NaN compares false
        return [[1 << d, 0, d]] * 3, False
    return rows, True


def check_enable(tabs, present):
    """xCheckWPEnable (:135-170): (tables, weighted)."""
    if any(any(p) for p in present):
        return tabs, True
    return [[[[1, 0, 0]] * 3 for _ in t] for t in tabs], False


def estimate_slice(org, cur, refs_acdc, refs_rec, B):
    """One P / B slice: org = three planes, cur = its AC/DC, refs_acdc / refs_rec = per list (one list for P, two for B) the AC/DC
    of the reference pictures' originals and their reconstructions.  Returns (tables [list] int16 [n][3][3], present [list][n],
    denominator, weighted)."""
    lists = list(refs_acdc) + [[]] * (2 - len(refs_acdc))
    tabs, d = update_params(cur, lists[0], lists[1], B)
    n_luma, n_chroma = np.asarray(org[0]).size, np.asarray(org[1]).size
    present = []
    for l, t in enumerate(tabs):
        present.append([])
        for i in range(len(t)):
            t[i], keep = select(sad_sums(org, refs_rec[l][i], t[i], B), n_luma, n_chroma, d, t[i])
            present[l].append(keep)
    tabs, weighted = check_enable(tabs, present)
    return [np.array(t, np.int16).reshape(len(t), 3, 3) for t in tabs], present, d, weighted
