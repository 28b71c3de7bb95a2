"""The yardstick of hmx_sao_stats*: TEncSampleAdaptiveOffset::calcSaoStatsCuOrg (TLibEncoder/TEncSampleAdaptiveOffset.cpp
:859-1124, SAO_SKIP_RIGHT = 1, TLibCommon/TypeDef.h:123) restated twice.

stats_loop  line for line, with the reference's running sign buffers (m_iUpBuff1 / m_iUpBufft) and loop bounds; slow.
stats_vec   numpy, every sign compared directly with the neighbour, ranges as masks; fast enough for 2160p.

Both take org / rec as three 2-D planes (4:2:0) and return int64 [3 components, CTUs in raster order, 52 bins, 2]
([..., 0] = sum of org - rec, [..., 1] = count), the layout of hmx_sao_stats (include/hmx.h): bin 5 * t + c for edge
type t (SAO_EO_0..3) and class c 0..4, bin 20 + k - 1 for band class k 1..32.
"""
import numpy as np

BINS = 52
EO_TABLE = (1, 2, 0, 3, 4)  # m_auiEoTable, TLibCommon/TComSampleAdaptiveOffset.cpp:94


def _sign(v):
    return (v > 0) - (v < 0)


def skips(comp, lcu_based):
    """(bottom rows, right columns) skipped by a CTU that does not touch the picture edge (:884-896)."""
    if not lcu_based:
        return 0, 0
    return (2, 3) if comp else (4, 5)


def _cu_org(O, R, B, pic_w, pic_h, lpx, tpy, lcu, skip_b, skip_r, st, cn):
    """One CTU of one component; O / R = the plane as lists of rows, (lpx, tpy) = the CTU's first sample in this plane,
    st / cn = m_iOffsetOrg / m_iCount [5 types][33 classes] of the CTU."""
    rpx, bpy = min(lpx + lcu, pic_w), min(tpy + lcu, pic_h)  # :898-909
    W, H = rpx - lpx, bpy - tpy
    shift = B - 5

    # band offset :914-943 (m_lumaTableBo[k] = 1 + (k >> (B - SAO_BO_BITS)), TComSampleAdaptiveOffset.cpp:176-181)
    end_x = W if rpx == pic_w else W - skip_r
    end_y = H if bpy == pic_h else H - skip_b
    for y in range(end_y):
        o, r = O[tpy + y], R[tpy + y]
        for x in range(lpx, lpx + end_x):
            k = 1 + (r[x] >> shift)
            if k:
                st[4][k] += o[x] - r[x]
                cn[4][k] += 1

    # SAO_EO_0 :953-977 (the rows run to H - numSkipLine even on the picture's bottom edge, :971)
    start_x = 1 if lpx == 0 else 0
    end_x = W - 1 if rpx == pic_w else W - skip_r
    for y in range(H - skip_b):
        o, r = O[tpy + y], R[tpy + y]
        assert lpx + start_x - 1 >= 0
        sign_left = _sign(r[lpx + start_x] - r[lpx + start_x - 1])
        for x in range(lpx + start_x, lpx + end_x):
            sign_right = _sign(r[x] - r[x + 1])
            e = EO_TABLE[sign_right + sign_left + 2]
            sign_left = -sign_right
            st[0][e] += o[x] - r[x]
            cn[0][e] += 1

    # SAO_EO_1 :979-1015
    start_y = 1 if tpy == 0 else 0
    end_x = W if rpx == pic_w else W - skip_r
    end_y = H - 1 if bpy == pic_h else H - skip_b
    row = tpy + start_y
    up = [_sign(R[row][lpx + x] - R[row - 1][lpx + x]) for x in range(W)]  # m_iUpBuff1
    for y in range(start_y, end_y):
        o, r, rn = O[row], R[row], R[row + 1]
        for x in range(end_x):
            sign_down = _sign(r[lpx + x] - rn[lpx + x])
            e = EO_TABLE[sign_down + up[x] + 2]
            up[x] = -sign_down
            st[1][e] += o[lpx + x] - r[lpx + x]
            cn[1][e] += 1
        row += 1

    # SAO_EO_2 :1016-1062; the buffers are indexed x + 1 (the reference's m_iUpBuff1++)
    start_x = 1 if lpx == 0 else 0
    end_x = W - 1 if rpx == pic_w else W - skip_r
    start_y = 1 if tpy == 0 else 0
    end_y = H - 1 if bpy == pic_h else H - skip_b
    row = tpy + start_y
    buf1, buft = [0] * (W + 2), [0] * (W + 2)
    for x in range(start_x, end_x):
        assert lpx + x - 1 >= 0
        buf1[x + 1] = _sign(R[row][lpx + x] - R[row - 1][lpx + x - 1])
    for y in range(start_y, end_y):
        o, r, rn = O[row], R[row], R[row + 1]
        sign_down2 = _sign(rn[lpx + start_x] - r[lpx + start_x - 1])
        for x in range(start_x, end_x):
            sign_down1 = _sign(r[lpx + x] - rn[lpx + x + 1])
            e = EO_TABLE[sign_down1 + buf1[x + 1] + 2]
            buft[x + 2] = -sign_down1
            st[2][e] += o[lpx + x] - r[lpx + x]
            cn[2][e] += 1
        buft[start_x + 1] = sign_down2
        buf1, buft = buft, buf1
        row += 1

    # SAO_EO_3 :1063-1120
    row = tpy + start_y
    buf1 = [0] * (W + 2)
    for x in range(start_x - 1, end_x):
        assert lpx + x >= 0
        buf1[x + 1] = _sign(R[row][lpx + x] - R[row - 1][lpx + x + 1])
    for y in range(start_y, end_y):
        o, r, rn = O[row], R[row], R[row + 1]
        for x in range(start_x, end_x):
            sign_down1 = _sign(r[lpx + x] - rn[lpx + x - 1])
            e = EO_TABLE[sign_down1 + buf1[x + 1] + 2]
            buf1[x] = -sign_down1  # m_iUpBuff1[x - 1]
            st[3][e] += o[lpx + x] - r[lpx + x]
            cn[3][e] += 1
        buf1[end_x] = _sign(rn[lpx + end_x - 1] - r[lpx + end_x])  # m_iUpBuff1[iEndX - 1]
        row += 1


def _to_bins(st, cn, out):
    for t in range(4):
        for c in range(5):
            out[5 * t + c] = st[t][c], cn[t][c]
    for k in range(1, 33):
        out[20 + k - 1] = st[4][k], cn[4][k]


def stats_loop(org, rec, w, h, ctu, B, lcu_based):
    cw, ch = -(-w // ctu), -(-h // ctu)
    out = np.zeros((3, cw * ch, BINS, 2), np.int64)
    for comp in range(3):
        sh = 1 if comp else 0
        O = np.asarray(org[comp], np.int64).tolist()
        R = np.asarray(rec[comp], np.int64).tolist()
        skip_b, skip_r = skips(comp, lcu_based)
        for addr in range(cw * ch):
            st, cn = [[0] * 33 for _ in range(5)], [[0] * 33 for _ in range(5)]
            _cu_org(O, R, B, w >> sh, h >> sh, ((addr % cw) * ctu) >> sh, ((addr // cw) * ctu) >> sh, ctu >> sh, skip_b, skip_r,
                    st, cn)
            _to_bins(st, cn, out[comp, addr])
    return out


# (type, neighbour a, neighbour b) as (dx, dy)
EO_NEIGHBOURS = ((0, (-1, 0), (1, 0)), (1, (0, -1), (0, 1)), (2, (-1, -1), (1, 1)), (3, (1, -1), (-1, 1)))


def ranges(comp, pw, ph, cs, lcu_based):
    """Per column and per row of the plane: CTU-local position, CTU index, and the end-exclusive range bounds of the
    table in include/hmx.h.  Returns (cx, lx, x bounds dict), (cy, ly, y bounds dict)."""
    skip_b, skip_r = skips(comp, lcu_based)
    X, Y = np.arange(pw), np.arange(ph)
    cx, cy = X // cs, Y // cs
    lx, ly = X - cx * cs, Y - cy * cs
    W, H = np.minimum(cs, pw - cx * cs), np.minimum(cs, ph - cy * cs)
    isL, isT, isR, isB = cx == 0, cy == 0, cx * cs + W == pw, cy * cs + H == ph
    xb = dict(full=np.where(isR, W, W - skip_r), inner=np.where(isR, W - 1, W - skip_r), start=isL.astype(np.int64))
    yb = dict(bo=np.where(isB, H, H - skip_b), eo0=H - skip_b, start=isT.astype(np.int64), v=np.where(isB, H - 1, H - skip_b))
    return (cx, lx, xb), (cy, ly, yb)


def stats_vec(org, rec, w, h, ctu, B, lcu_based):
    cw, ch = -(-w // ctu), -(-h // ctu)
    n_lcu = cw * ch
    out = np.zeros((3, n_lcu, BINS, 2), np.int64)
    table = np.array(EO_TABLE)
    for comp in range(3):
        sh = 1 if comp else 0
        pw, ph, cs = w >> sh, h >> sh, ctu >> sh
        r = np.asarray(rec[comp], np.int64)
        d = np.asarray(org[comp], np.int64) - r
        (cx, lx, xb), (cy, ly, yb) = ranges(comp, pw, ph, cs, lcu_based)
        lcu = (cy * cw)[:, None] + cx[None, :]
        x_full, x_in = lx < xb["full"], (lx >= xb["start"]) & (lx < xb["inner"])
        y_v = (ly >= yb["start"]) & (ly < yb["v"])
        pad = np.pad(r, 1, mode="edge")  # out-of-picture neighbours are never inside a range

        def nb(dx, dy):
            return pad[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw]

        def add(mask, bins):
            idx = lcu[mask] * BINS + bins[mask]
            for j, wt in ((0, d[mask]), (1, None)):
                v = np.bincount(idx, weights=wt, minlength=n_lcu * BINS)
                out[comp, :, :, j] += np.rint(v).astype(np.int64).reshape(n_lcu, BINS)

        masks = {0: x_in[None, :] & (ly < yb["eo0"])[:, None], 1: x_full[None, :] & y_v[:, None], 2: x_in[None, :] & y_v[:, None]}
        masks[3] = masks[2]
        for t, a, b in EO_NEIGHBOURS:
            e = np.sign(r - nb(*a)) + np.sign(r - nb(*b)) + 2
            add(masks[t], 5 * t + table[e])
        add(x_full[None, :] & (ly < yb["bo"])[:, None], 20 + (r >> (B - 5)))
    return out

