"""Adaptive QP restated from the reference's text: TEncPreanalyzer::xPreanalyze (TLibEncoder/TEncPreanalyzer.cpp:64-139) and
TEncCu::xComputeQP (TEncCu.cpp:1114-1136).  Python floats are IEEE doubles and every operation below is one operation of the
reference, in its order; the sums are Python ints; the logarithm is math.log (libm's).  tests/test_aq_oracle.py holds this file
against a second construction and against QPs the reference encoder coded."""
import math

import numpy as np

MAX_QP = 51


class Geom:
    """The layers of TEncPic::create (TEncPic.cpp:128-139): layer d has parts of ctu >> d, ceil(w / part) x ceil(h / part) of them
    (:82-89).  A picture's arrays hold the layers one after the other, units row-major."""

    def __init__(self, w, h, ctu, depths):
        self.w, self.h, self.ctu, self.depths = w, h, ctu, depths
        self.part = [ctu >> d for d in range(depths)]
        self.nx = [(w + p - 1) // p for p in self.part]
        self.ny = [(h + p - 1) // p for p in self.part]
        self.first, self.total = [], 0
        for d in range(depths):
            self.first.append(self.total)
            self.total += self.nx[d] * self.ny[d]


def legal_depths(ctu):
    return [k for k in range(1, 5) if ctu >> (k - 1) >= 8]


def preanalyze(luma, ctu, depths):
    """xPreanalyze of one luma plane (2-D integer array): (activities float64 [total], layer averages float64 [depths])"""
    luma = np.asarray(luma).astype(np.int64)
    h, w = luma.shape
    g = Geom(w, h, ctu, depths)
    act, avg = np.zeros(g.total, np.float64), np.zeros(depths, np.float64)
    for d in range(depths):
        part, u = g.part[d], g.first[d]
        sum_act = 0.0
        for y in range(0, h, part):
            ch = min(part, h - y)
            for x in range(0, w, part):
                cw = min(part, w - x)
                blk = luma[y:y + ch, x:x + cw]
                quads = (blk[:ch >> 1, :cw >> 1], blk[:ch >> 1, cw >> 1:], blk[ch >> 1:, :cw >> 1], blk[ch >> 1:, cw >> 1:])
                n = cw * ch  # uiNumPixInAQPart counts the samples of all four quadrants (:94-114)
                min_var = 1.7976931348623157e308  # DBL_MAX
                for q in quads:
                    s, ss = int(q.sum()), int((q * q).sum())
                    average = float(s) / n
                    variance = float(ss) / n - average * average
                    min_var = min(min_var, variance)
                activity = 1.0 + min_var
                act[u] = activity
                sum_act += activity
                u += 1
        avg[d] = sum_act / (g.nx[d] * g.ny[d])
    return act, avg


def offset_of_norm(norm):
    return int(math.floor(math.log(norm) / math.log(2.0) * 6.0 + 0.49999))


def offset(act, avg_act, qp_range):
    """iQpOffset of xComputeQP (:1128-1133)"""
    act, avg_act = float(act), float(avg_act)
    scale = math.pow(2.0, qp_range / 6.0)
    norm = (scale * act + avg_act) / (act + scale * avg_act)
    return offset_of_norm(norm)


def clip_qp(qp, qp_bd_offset):
    return min(MAX_QP, max(-qp_bd_offset, qp))


def compute_qp(g, act, avg, cu_x, cu_y, cu_depth, slice_qp, qp_range, qp_bd_offset):
    """xComputeQP for the CU at luma position (cu_x, cu_y) and depth cu_depth"""
    d = min(cu_depth, g.depths - 1)
    u = g.first[d] + (cu_y // g.part[d]) * g.nx[d] + cu_x // g.part[d]
    return clip_qp(slice_qp + offset(act[u], avg[d], qp_range), qp_bd_offset)


def qp_map(g, act, avg, slice_qp, qp_range, qp_bd_offset):
    """The xComputeQP result of every unit of every layer, int8 [total]"""
    out = np.zeros(g.total, np.int8)
    for d in range(g.depths):
        for u in range(g.first[d], g.first[d] + g.nx[d] * g.ny[d]):
            out[u] = clip_qp(slice_qp + offset(act[u], avg[d], qp_range), qp_bd_offset)
    return out
