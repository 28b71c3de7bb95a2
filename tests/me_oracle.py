"""Numpy restatement of the integer motion search of the reference encoder, for the tests of hmx_getSAD, hmx_mvBits,
hmx_mvCost, hmx_setSearchRange and hmx_batch_fullpel_search:

  sad             TComRdCost::xGetSAD4..64 (TComRdCost.cpp:518-...): rows 0, 2^s, ... of |org - cur|, (sum << s) >> (B - 8)
  comp_bits       TComRdCost::xGetComponentBits (:270-284) in closed form; comp_bits_loop is its halving loop
  mv_bits/mv_cost TComRdCost::getBits(x, y) / getCost(x, y) (TComRdCost.h:185-211)
  set_search_range TEncSearch::xSetSearchRange (TEncSearch.cpp:4209-4225) over clip_mv (TComDataCU.cpp:3505-3517)
  search          TEncSearch::xPatternSearch (:4227-4283), vectorised over the box; search_loop is the loop-for-loop form

Everything is UInt arithmetic modulo 2^32.  The oracle is pinned on the compiled reference by recorded calls:
oracle/_ref/TAppEncoder_metap is the reference encoder with a recorder inside its own TEncSearch (oracle/ref_me_tap.h), and
tests/test_me_enc_tap.py requires of sad, mv_cost, set_search_range and search what its xMotionEstimation did in the calls of
tests/golden/me_enc_tap.npz: the box, the vector term of the costs, the winning vector and ruiSAD.  The second, literal
restatement (tests/test_me_oracle.py) and, on the GPU, the cross-check of the cost map against hmx_batch_subpel_cost
(tests/test_gpu_me.py) cover the sizes and edges the encoder's calls do not reach."""
import numpy as np

M32 = 0xFFFFFFFF
SIZES = (4, 8, 12, 16, 24, 32, 48, 64)


def sad(org, cur, sub_shift, B):
    """org, cur: 2-D integer arrays of one block."""
    step = 1 << sub_shift
    s = int(np.abs(org[::step].astype(np.int64) - cur[::step].astype(np.int64)).sum()) & M32
    return ((s << sub_shift) & M32) >> (B - 8)


def comp_bits(v):
    t = ((-v) << 1) + 1 if v <= 0 else v << 1
    return 2 * (t.bit_length() - 1) + 1


def comp_bits_loop(v):
    """The reference's loop, statement by statement."""
    length = 1
    temp = ((-v) << 1) + 1 if v <= 0 else (v << 1)
    assert temp
    while temp != 1:
        temp >>= 1
        length += 2
    return length


def mv_bits(x, y, pred_x, pred_y, cost_scale):
    return comp_bits((x << cost_scale) - pred_x) + comp_bits((y << cost_scale) - pred_y)


def mv_cost(lam, x, y, pred_x, pred_y, cost_scale):
    return ((lam * mv_bits(x, y, pred_x, pred_y, cost_scale)) & M32) >> 16


def clip_mv(mvx, mvy, cu_x, cu_y, pic_w, pic_h, ctu):
    hmax, hmin = (pic_w + 8 - cu_x - 1) << 2, (-ctu - 8 - cu_x + 1) << 2
    vmax, vmin = (pic_h + 8 - cu_y - 1) << 2, (-ctu - 8 - cu_y + 1) << 2
    return min(hmax, max(hmin, mvx)), min(vmax, max(vmin, mvy))


def set_search_range(pred_x, pred_y, range_, cu_x, cu_y, pic_w, pic_h, ctu=64):
    """(left, top, right, bottom), integer samples, inclusive."""
    px, py = clip_mv(pred_x, pred_y, cu_x, cu_y, pic_w, pic_h, ctu)
    lx, ty = clip_mv(px - (range_ << 2), py - (range_ << 2), cu_x, cu_y, pic_w, pic_h, ctu)
    rx, by = clip_mv(px + (range_ << 2), py + (range_ << 2), cu_x, cu_y, pic_w, pic_h, ctu)
    return lx >> 2, ty >> 2, rx >> 2, by >> 2


def cost_map(org, ref, margin, u, lam, B):
    """The cost of every candidate of one unit, (bottom - top + 1, right - left + 1) uint32.  org: the original luma plane;
    ref: the reference's luma plane WITH its margins (margin = (mx, my)); u: a mapping with the hmx_me_unit fields."""
    x, y, w, h, s = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"]), int(u["sub_shift"])
    l, t, r, b = int(u["left"]), int(u["top"]), int(u["right"]), int(u["bottom"])
    px, py = int(u["pred_x"]), int(u["pred_y"])
    step = 1 << s
    ob = org[y:y + h:step, x:x + w].astype(np.int64)
    out = np.zeros((b - t + 1, r - l + 1), np.uint32)
    X0, Y0 = margin[0] + x, margin[1] + y
    win = ref[Y0 + t:Y0 + b + h, X0 + l:X0 + r + w].astype(np.int64)
    for j in range(b - t + 1):
        rows = win[j:j + h:step]
        for i in range(r - l + 1):
            sm = int(np.abs(ob - rows[:, i:i + w]).sum()) & M32
            sd = ((sm << s) & M32) >> (B - 8)
            out[j, i] = (sd + mv_cost(lam, l + i, t + j, px, py, 2)) & M32
    return out


def winner(costs, u, lam):
    """(mvx, mvy, sad, cost) of a cost map: the first strictly smallest cost in raster order."""
    k = int(np.argmin(costs.reshape(-1)))  # numpy returns the first occurrence of the minimum
    bw = costs.shape[1]
    mx, my = int(u["left"]) + k % bw, int(u["top"]) + k // bw
    c = int(costs.reshape(-1)[k])
    return mx, my, (c - mv_cost(lam, mx, my, int(u["pred_x"]), int(u["pred_y"]), 2)) & M32, c


def search(org, ref, margin, u, lam, B):
    m = cost_map(org, ref, margin, u, lam, B)
    return winner(m, u, lam), m


def search_loop(org, ref, margin, u, lam, B):
    """xPatternSearch as written: y outside, x inside, strict <, uiSadBest = MAX_UINT; plain Python integers."""
    x0, y0, w, h, s = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"]), int(u["sub_shift"])
    px, py = int(u["pred_x"]), int(u["pred_y"])
    best, bx, by = M32, 0, 0
    costs = []
    for y in range(int(u["top"]), int(u["bottom"]) + 1):
        for x in range(int(u["left"]), int(u["right"]) + 1):
            sm, rows = 0, h
            r = 0
            while rows != 0:
                for n in range(w):
                    sm = (sm + abs(int(org[y0 + r, x0 + n]) - int(ref[margin[1] + y0 + y + r, margin[0] + x0 + x + n]))) & M32
                r += 1 << s
                rows -= 1 << s
            sm = ((sm << s) & M32) >> (B - 8)
            bits = comp_bits_loop((x << 2) - px) + comp_bits_loop((y << 2) - py)
            sm = (sm + (((lam * bits) & M32) >> 16)) & M32
            costs.append(sm)
            if sm < best:
                best, bx, by = sm, x, y
    bits = comp_bits_loop((bx << 2) - px) + comp_bits_loop((by << 2) - py)
    return (bx, by, (best - (((lam * bits) & M32) >> 16)) & M32, best), costs
