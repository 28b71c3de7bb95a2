"""The yardstick of explicit weighted prediction (hmx_addWeightUni / hmx_addWeightBi / hmx_motionCompensation_wp /
hmx_batch_motionCompensation_wp_multi): TComWeightPrediction (TLibCommon/TComWeightPrediction.cpp:61-313, .h:75-89) restated twice.

*_loop   member by member: get_wp_scaling derives w / o / offset / shift / round as getWpScaling does (:286-312), then
         add_weight_uni_loop / add_weight_bi_loop walk the three components sample by sample, chroma at half size, with the
         inline weightUnidir / weightBidir; slow.
*_vec    numpy on whole planes, written from the formulas and not from the loop.

An entry is (weight[3], offset[3], log2_denom[3]) per component Y, Cb, Cr: iWeight, iOffset (8-bit units), uiLog2WeightDenom.
Sources are 14-bit intermediates (int16), results are samples of bit depth B.  The reference's `offset << (shift - 1)` on a
negative offset is written as a product.

mc_frame_wp builds a whole picture's weighted prediction from the pinned CPU oracle's own 14-bit intermediates
(hmo_predInterLumaBlk / hmo_predInterChromaBlk with bi = 1) and the vector form.
"""
import numpy as np

IF_INTERNAL_PREC, IF_INTERNAL_OFFS = 14, 8192


def get_wp_scaling(e0, e1, B):
    """getWpScaling (:251-313): e0 / e1 = the entries of list 0 / list 1, None = list unused.  Returns per component a dict
    with the derived fields the add* members read: w0, w1 (None where unused), offset, shift, round."""
    out = []
    for c in range(3):
        if e0 is not None and e1 is not None:  # :286-301, list 0's denominator for both lists
            o0 = e0[1][c] * (1 << (B - 8))
            o1 = e1[1][c] * (1 << (B - 8))
            out.append(dict(w0=e0[0][c], w1=e1[0][c], offset=o0 + o1, shift=e0[2][c] + 1, round=1 << e0[2][c]))
        else:  # :302-312
            e = e0 if e0 is not None else e1
            d = e[2][c]
            out.append(dict(w0=e[0][c], w1=None, offset=e[1][c] * (1 << (B - 8)), shift=d, round=(1 << (d - 1)) if d >= 1 else 0))
    return out


def _clip(x, B):
    return 0 if x < 0 else ((1 << B) - 1 if x > (1 << B) - 1 else x)


def weight_unidir(w0, p0, rnd, shift, offset, B):  # TComWeightPrediction.h:86-89
    return _clip(((w0 * (p0 + IF_INTERNAL_OFFS) + rnd) >> shift) + offset, B)


def weight_bidir(w0, p0, w1, p1, rnd, shift, offset, B):  # :82-85
    return _clip((w0 * (p0 + IF_INTERNAL_OFFS) + w1 * (p1 + IF_INTERNAL_OFFS) + rnd + offset * (1 << (shift - 1))) >> shift, B)


def add_weight_uni_loop(src, e, B):
    """addWeightUni (:161-237) after getWpScaling: src = [Y, Cb, Cr] 2-D int16 planes (chroma at half size)."""
    wp = get_wp_scaling(e, None, B)
    shift_num = IF_INTERNAL_PREC - B
    out = []
    for c in range(3):
        shift = wp[c]["shift"] + shift_num
        rnd = (1 << (shift - 1)) if shift else 0  # the member recomputes the rounding from the full shift
        h, w = src[c].shape
        d = np.zeros((h, w), np.int16)
        for y in range(h - 1, -1, -1):
            for x in range(w - 1, -1, -1):
                d[y, x] = weight_unidir(wp[c]["w0"], int(src[c][y, x]), rnd, shift, wp[c]["offset"], B)
        out.append(d)
    return out


def add_weight_bi_loop(src0, src1, e0, e1, B):
    """addWeightBi (:61-150, bRound = true) after getWpScaling."""
    wp = get_wp_scaling(e0, e1, B)
    shift_num = IF_INTERNAL_PREC - B
    out = []
    for c in range(3):
        shift = wp[c]["shift"] + shift_num
        rnd = (1 << (shift - 1)) if shift else 0
        h, w = src0[c].shape
        d = np.zeros((h, w), np.int16)
        for y in range(h - 1, -1, -1):
            for x in range(w - 1, -1, -1):
                d[y, x] = weight_bidir(wp[c]["w0"], int(src0[c][y, x]), wp[c]["w1"], int(src1[c][y, x]), rnd, shift, wp[c]["offset"], B)
        out.append(d)
    return out


def weight_uni_vec(p, weight, offset, log2_denom, B):
    """One component: Clip_B(((w * (P + 8192) + round) >> shift) + o), shift = denom + 14 - B, o = offset * 2^(B-8)."""
    shift = int(log2_denom) + 14 - B
    rnd = (1 << (shift - 1)) if shift > 0 else 0
    v = ((int(weight) * (np.asarray(p, np.int64) + 8192) + rnd) >> shift) + int(offset) * (1 << (B - 8))
    return np.clip(v, 0, (1 << B) - 1).astype(np.int16)


def weight_bi_vec(p0, p1, weight0, weight1, offset0, offset1, log2_denom, B):
    """One component: Clip_B((w0 (P0 + 8192) + w1 (P1 + 8192) + round + (o0 + o1) * 2^(shift-1)) >> shift), shift = denom0 + 1 + 14 - B."""
    shift = int(log2_denom) + 1 + 14 - B
    half = 1 << (shift - 1)
    off = (int(offset0) + int(offset1)) * (1 << (B - 8))
    v = (int(weight0) * (np.asarray(p0, np.int64) + 8192) + int(weight1) * (np.asarray(p1, np.int64) + 8192) + half + off * half) >> shift
    return np.clip(v, 0, (1 << B) - 1).astype(np.int16)


def add_weight_uni_vec(src, e, B):
    return [weight_uni_vec(src[c], e[0][c], e[1][c], e[2][c], B) for c in range(3)]


def add_weight_bi_vec(src0, src1, e0, e1, B):
    return [weight_bi_vec(src0[c], src1[c], e0[0][c], e1[0][c], e0[1][c], e1[1][c], e0[2][c], B) for c in range(3)]


def random_entry(rng):
    """An entry over the full supported ranges: weight -128..255, offset -128..127, log2_denom 0..7."""
    return ([int(v) for v in rng.integers(-128, 256, 3)], [int(v) for v in rng.integers(-128, 128, 3)], [int(v) for v in rng.integers(0, 8, 3)])


# Hand-computed samples at the clips (B, kind, arguments, expected):
#   uni: (P, weight, offset, log2_denom)          bi: (P0, P1, weight0, weight1, offset0, offset1, log2_denom)
CLIP_CASES = [
    # B = 8: head = 6
    (8, "uni", (8191, -128, 0, 0), 0),        # (-128 * 16383 + 32) >> 6 = -32766: below 0; negative weight, denom 0, P = 8191
    (8, "uni", (8191, 255, 127, 0), 255),     # (255 * 16383 + 32) >> 6 = 65276, + 127: above 255
    (8, "uni", (4608, 128, -128, 7), 72),     # (128 * 12800 + 4096) >> 13 = 200, - 128; denom 7, offset -128
    (8, "uni", (-8192, 255, 127, 7), 127),    # P = -8192: 4096 >> 13 = 0, + 127; offset +127
    (8, "uni", (-1792, 64, 127, 6), 227),     # (64 * 6400 + 2048) >> 12 = 100, + 127
    (8, "uni", (-4992, -1, 127, 0), 77),      # (-3200 + 32) >> 6 = -50 (arithmetic shift), + 127
    # B = 10: head = 4, offsets times 4
    (10, "uni", (8191, 1, -128, 0), 512),     # (16383 + 8) >> 4 = 1024, - 512
    (10, "uni", (8191, 255, 127, 7), 1023),   # (255 * 16383 + 1024) >> 11 = 2040, + 508: above 1023
    (8, "bi", (-7552, -6848, 1, 1, 0, 0, 0), 16),           # (640 + 1344 + 64) >> 7; denom 0
    (8, "bi", (8191, 8191, -128, -128, -128, -128, 0), 0),  # (-4194048 - 255 * 64) >> 7 < 0
    (8, "bi", (8191, 8191, 255, 255, 127, 127, 0), 255),
    (8, "bi", (-1792, -1728, 128, 128, 127, -128, 7), 100),   # offsets sum to -1: (1646592 + 0) >> 14 = 100; denom 7
    (8, "bi", (-8192, -8192, 255, 255, 127, 127, 7), 127),    # P = -8192: 255 * 8192 >> 14
    (8, "bi", (-5632, -3072, -64, 192, -128, 0, 6), 36),      # (-163840 + 983040 - 127 * 4096) >> 13
    (10, "bi", (-8192, -8192, 1, 1, 127, 127, 0), 508),       # (1 + 1016) * 16 >> 5
    # B = 12: head = 2, offsets times 16
    (12, "uni", (8191, -128, 0, 0), 0),       # (-128 * 16383 + 2) >> 2 < 0
    (12, "uni", (8191, 255, 127, 0), 4095),   # (255 * 16383 + 2) >> 2 = 1044416, + 2032: above 4095
    (12, "uni", (8191, 1, -128, 0), 2048),    # (16383 + 2) >> 2 = 4096, - 2048
    (12, "uni", (-8192, 255, 127, 7), 2032),  # P = -8192: 256 >> 9 = 0, + 127 * 16
    (12, "uni", (-1792, 64, 127, 6), 3632),   # (64 * 6400 + 128) >> 8 = 1600, + 2032
    (12, "uni", (4608, 128, -128, 7), 1152),  # (128 * 12800 + 256) >> 9 = 3200, - 2048
    (12, "bi", (8191, 8191, -128, -128, -128, -128, 0), 0),   # (-4194048 + 4 - 4096 * 4) >> 3 < 0
    (12, "bi", (8191, 8191, 255, 255, 127, 127, 7), 4095),    # (8355330 + 512 + 4064 * 512) >> 10 = 10191: above 4095
    (12, "bi", (-8192, -8192, 1, 1, 127, 127, 0), 2032),      # (4 + 4064 * 4) >> 3
    (12, "bi", (-1792, -1728, 128, 128, 127, -128, 7), 1600), # offsets sum to -1: (1646592 + 512 - 16 * 512) >> 10 = 1600
]


def mc_frame_wp(pus, refs, wp, B):
    """The weighted prediction of one picture.  pus: PU records (oracle_lib.PU_DTYPE fields); refs: one item per reference,
    ([Y, Cb, Cr] 2-D int16 planes INCLUDING margins, luma margin m) -- chroma planes carry m / 2; wp = (l0, l1): per list one
    entry per reference (l1 may be None when no unit uses list 1).  Every used list is predicted into the 14-bit intermediate by
    the pinned oracle (bi = 1), then weighted: one list -> uni formula, two lists -> bi formula (always).  Returns the
    three planes of the picture (picture size = the references' size without margins); units are cropped at the picture edge."""
    import ctypes as C

    import oracle_lib as ol
    O = ol.oracle()
    planes0, m0 = refs[0]
    H, W = planes0[0].shape[0] - 2 * m0, planes0[0].shape[1] - 2 * m0
    out = [np.zeros((H, W), np.int16), np.zeros((H // 2, W // 2), np.int16), np.zeros((H // 2, W // 2), np.int16)]
    flat = [[np.ascontiguousarray(p).reshape(-1) for p in planes] for planes, _ in refs]
    for u in pus:
        x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
        use = [(int(u["ref0"]), int(u["mv0x"]), int(u["mv0y"]), 0), (int(u["ref1"]), int(u["mv1x"]), int(u["mv1y"]), 1)]
        use = [t for t in use if t[0] != 255]
        if not use:
            continue
        inter, entries = [], []
        for r, mvx, mvy, lst in use:
            planes, m = refs[r]
            pred = []
            for c in range(3):
                ch = 1 if c else 0
                st, mc = planes[c].shape[1], m >> ch
                o = (mc + (y >> ch)) * st + mc + (x >> ch)
                t = np.zeros((h >> ch, w >> ch), np.int16)
                (O.hmo_predInterChromaBlk if c else O.hmo_predInterLumaBlk)(ol.ptr(flat[r][c], o), st, mvx, mvy, w, h, t.reshape(-1), w >> ch, 1, B)
                pred.append(t)
            inter.append(pred)
            entries.append(wp[lst][r])
        got = add_weight_bi_vec(inter[0], inter[1], entries[0], entries[1], B) if len(use) == 2 else add_weight_uni_vec(inter[0], entries[0], B)
        for c in range(3):
            ch = 1 if c else 0
            ph, pw = out[c].shape
            y0, x0 = y >> ch, x >> ch
            hh, ww = min(h >> ch, ph - y0), min(w >> ch, pw - x0)
            if hh > 0 and ww > 0:
                out[c][y0:y0 + hh, x0:x0 + ww] = got[c][:hh, :ww]
    return out
