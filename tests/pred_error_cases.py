"""The inputs of the prediction-error vectors (tests/golden/pred_error_b*.npz) and of tests/test_pred_error_oracle.py: two small
reference pictures, an original and about 60 complete motion candidates over every unit size and kind (list 0, list 1, both;
plain and weighted).  Inputs only: expected values come from the compiled reference (ref_results: ref_set_recon + ref_predInterBlk
once per reference picture, ref_addAvg, ref_xWeightedPredictionUni / Bi, ref_getDistPart with DF_HADS), never from here."""
import ctypes as C
import functools
import os

import numpy as np

import me_oracle as mo
import oracle_lib as ol
import wp_cases

PIC_W, PIC_H, MARGIN = 128, 64, 80
N = 255
# every width and every height of the set, small partners so that the stored predictions stay small; 64x64 once per kind
SHAPES = [(4, 4), (8, 4), (4, 8), (8, 8), (12, 16), (16, 12), (16, 16), (24, 8), (8, 24), (32, 8), (8, 32), (48, 4), (4, 48), (64, 8), (16, 64),
          (32, 32), (64, 64), (24, 32), (16, 4), (4, 16)]
KINDS = ("l0", "l1", "bi")


def scene(B):
    """pictures (luma, chroma at half size; without margins), the original, the candidates, per candidate whether it is
    weighted, and the tables l0 / l1 (one wp_oracle entry per reference)."""
    rng = np.random.default_rng(7300 + B)
    yy, xx = np.mgrid[0:PIC_H, 0:PIC_W]
    pics = []
    for k in range(2):  # texture plus noise: distortions with structure
        base = (np.sin(xx / (5.0 + k)) + np.cos(yy / (7.0 - k))) * (1 << (B - 3)) + (1 << (B - 1))
        y = np.clip(base + rng.integers(-(1 << (B - 4)), 1 << (B - 4), base.shape), 0, (1 << B) - 1).astype(np.int16)
        pics.append([y] + [rng.integers(0, 1 << B, (PIC_H // 2, PIC_W // 2)).astype(np.int16) for _ in range(2)])
    org = np.clip(np.roll(pics[0][0], (2, -3), (0, 1)).astype(np.int32) + rng.integers(-(1 << (B - 5)), (1 << (B - 5)) + 1, (PIC_H, PIC_W)), 0,
                  (1 << B) - 1).astype(np.int16)
    cands, weighted = np.zeros(3 * len(SHAPES), ol.PU_DTYPE), np.zeros(3 * len(SHAPES), np.uint8)
    for i in range(len(cands)):
        w, h = SHAPES[i % len(SHAPES)]
        kind = KINDS[(i + i // len(SHAPES)) % 3]
        x, y = int(rng.integers(0, (PIC_W - w) // 4 + 1)) * 4, int(rng.integers(0, (PIC_H - h) // 4 + 1)) * 4
        mv = []
        for lst in range(2):
            far = i % 7 == lst  # some vectors far outside, which the clip brings back to the margin's reach
            v = rng.integers(-400, 401, 2) if far else rng.integers(-40, 41, 2)
            if i % 11 == 3 + lst:
                v = (v // 4) * 4  # integer vectors: the copy cases
            mv.append(mo.clip_mv(int(v[0]), int(v[1]), x, y, PIC_W, PIC_H, 64))
        r0, r1 = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        cands[i] = (x, y, w, h, N if kind == "l1" else r0, N if kind == "l0" else r1, mv[0][0], mv[0][1], mv[1][0], mv[1][1])
        weighted[i] = i % 3 == 1 or i >= 2 * len(SHAPES) + 10
    l0, l1 = [], []
    for r in range(2):  # one row pair over the legal ranges, one fade
        e0, e1 = wp_cases.entry_pair(rng, r == 0)
        l0.append(e0), l1.append(e1)
    return dict(pics=pics, org=org, cands=cands, weighted=weighted, l0=l0, l1=l1)


def check_scene(S):
    """what the list must contain; returns the counts"""
    c, wt = S["cands"], S["weighted"]
    assert {int(u["w"]) for u in c} == set(mo.SIZES) == {int(u["h"]) for u in c}
    count = {}
    for u, f in zip(c, wt):
        kind = "l0" if u["ref1"] == N else "l1" if u["ref0"] == N else "bi"
        count[(kind, bool(f))] = count.get((kind, bool(f)), 0) + 1
        for lst in range(2):
            if u[f"ref{lst}"] == N:
                continue
            x0, y0 = int(u["x"]) + (int(u[f"mv{lst}x"]) >> 2), int(u["y"]) + (int(u[f"mv{lst}y"]) >> 2)
            assert -MARGIN <= x0 - 3 and x0 + int(u["w"]) + 4 <= PIC_W + MARGIN and -MARGIN <= y0 - 3 and y0 + int(u["h"]) + 4 <= PIC_H + MARGIN
    assert len(count) == 6 and min(count.values()) >= 4, count
    assert len(c) >= 60
    return count


def ref_results(S, B):
    """(predictions, Hadamard distortions) of every candidate of a scene from the compiled reference alone, composed as
    xGetInterPredictionError composes them: motionCompensation's luma (TComPrediction.cpp:410-540) and xGetHADs through
    getDistPart(DF_HADS).  One ref_set_recon per reference picture."""
    R = ol.ref()
    R.ref_init(B, PIC_W, PIC_H, 1)
    R.ref_getDistPart.restype = C.c_uint
    c, wt = S["cands"], S["weighted"]
    inter = [[None, None] for _ in c]
    for r in range(2):
        p = [np.ascontiguousarray(a, np.int16).reshape(-1) for a in S["pics"][r]]
        R.ref_set_recon(p[0], p[1], p[2])
        for i, u in enumerate(c):
            w, h = int(u["w"]), int(u["h"])
            both = u["ref0"] != N and u["ref1"] != N
            for lst in range(2):
                if int(u[f"ref{lst}"]) != r:
                    continue
                t = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
                R.ref_predInterBlk(int(u["x"]), int(u["y"]), w, h, int(u[f"mv{lst}x"]), int(u[f"mv{lst}y"]), int(both or bool(wt[i])), t[0].reshape(-1),
                                   t[1].reshape(-1), t[2].reshape(-1), 0)
                inter[i][lst] = t
    preds, hads = [], np.zeros(len(c), np.uint32)
    P3 = C.c_void_p * 3
    for i, u in enumerate(c):
        a, b = inter[i]
        w, h = int(u["w"]), int(u["h"])
        if wt[i]:
            e0 = None if a is None else S["l0"][int(u["ref0"])]
            e1 = None if b is None else S["l1"][int(u["ref1"])]
            if b is None and i % 2:  # P style: xWeightedPredictionUni on list 0
                p = ol.r_wp_uni(a, e0, 0, int(u["ref0"]))[0]
            else:
                p = ol.r_wp_bi(a, b, e0, e1, 0 if a is None else int(u["ref0"]), 0 if b is None else int(u["ref1"]))[0]
        elif a is not None and b is not None:
            o = [np.zeros_like(q) for q in a]
            R.ref_addAvg(P3(*[q.ctypes.data for q in a]), P3(*[q.ctypes.data for q in b]), P3(*[q.ctypes.data for q in o]), w, h)
            p = o[0]
        else:
            p = (a if a is not None else b)[0]
        p = np.ascontiguousarray(p, np.int16)
        ob = np.ascontiguousarray(S["org"][int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w], np.int16)
        hads[i] = R.ref_getDistPart(p.ctypes.data_as(C.c_void_p), w, ob.ctypes.data_as(C.c_void_p), w, w, h, 1)
        preds.append(p)
    R.ref_init(B, 416, 240, 1)  # the state every other test of the reference expects
    return preds, hads


def extended(S):
    """The luma planes of the scene's references with their margins (extendPicBorder: the nearest picture sample)."""
    return [np.pad(p[0], MARGIN, mode="edge") for p in S["pics"]]


@functools.lru_cache(maxsize=None)
def load_vectors(B):
    """The committed scene of bit depth B as `scene` returns it, with the reference's results under "pred" (list of 2-D arrays)
    and "had".  Read once per bit depth and shared read-only."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"pred_error_b{B}.npz"))
    S = dict(pics=[[np.ascontiguousarray(g[f"pic{i}_{k}"]) for k in ("y", "cb", "cr")] for i in range(2)], org=np.ascontiguousarray(g["org"]),
             cands=g["cands"], weighted=g["weighted"], l0=[tuple(e) for e in g["l0"].tolist()], l1=[tuple(e) for e in g["l1"].tolist()], had=g["had"])
    S["pred"], at = [], 0
    for u in S["cands"]:
        w, h = int(u["w"]), int(u["h"])
        S["pred"].append(np.ascontiguousarray(g["pred"][at:at + w * h].reshape(h, w)))
        at += w * h
    for a in [p for pic in S["pics"] for p in pic] + [S["org"], S["cands"], S["weighted"], S["had"]] + S["pred"]:
        a.setflags(write=False)
    return S
