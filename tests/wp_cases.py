"""The inputs of the weighted-prediction vectors (tests/golden/wp_b*.npz) and of tests/test_oracle_vs_ref_wp.py: block cases for the
members and one prediction-unit list on a 136x72 picture.  Inputs only: expected values come from the compiled reference
(oracle_lib.r_wp_uni / r_wp_bi / r_mc_frame_wp), never from here."""
import functools
import os

import numpy as np

import oracle_lib as ol
import wp_oracle as wo

SHAPES = [(4, 4), (8, 4), (4, 8), (16, 12), (12, 16), (24, 32), (64, 64)]
BI, L0_ONLY, L1_ONLY = 0, 1, 2  # the three index patterns of xWeightedPredictionBi


def planes(rng, w, h, B, full):
    """[Y, Cb, Cr] sources: any int16 (full) or -8192..8191 (what the interpolation gives)"""
    lo, hi = (-32768, 32768) if full else (-8192, 8192)
    return [rng.integers(lo, hi, (h >> s, w >> s)).astype(np.int16) for s in (0, 1, 1)]


def fade_entry(rng, denoms, denom_field=None):
    """Weights around 1 << denoms[c], small offsets, so that results stay off the clips; denom_field: the coded denominators, when
    they are to differ from the scale of the weights (a list-1 row, whose denominator the bi case must not read)."""
    w = [int((1 << d) + rng.integers(-(1 << d) // 2, (1 << d) // 2 + 1)) for d in denoms]
    return (w, [int(v) for v in rng.integers(-20, 21, 3)], list(denoms if denom_field is None else denom_field))


def entry_pair(rng, legal_range):
    """(e0, e1) with list 1's denominator different from list 0's in every component"""
    if legal_range:  # weight -128..255, offset -128..127, denominator 0..7, each component its own
        e0, e1 = wo.random_entry(rng), wo.random_entry(rng)
        e1 = (e1[0], e1[1], [d1 if d1 != d0 else (d0 + 1) % 8 for d0, d1 in zip(e0[2], e1[2])])
        return e0, e1
    d0 = [int(v) for v in rng.integers(0, 7, 3)]
    return fade_entry(rng, d0), fade_entry(rng, d0, [d + 1 for d in d0])


def block_cases(B, every_combination):
    """dicts w, h, pattern, e0, e1, src0, src1.  every_combination: per shape the three patterns x the two source ranges x the two kinds
    of rows; otherwise the four per shape that the committed vectors hold, and the rows of wp_oracle.CLIP_CASES as constant 4x4 blocks."""
    rng = np.random.default_rng(6100 + B)
    out = []
    for k, (w, h) in enumerate(SHAPES):
        combos = [(p, f, r) for p in (BI, L0_ONLY, L1_ONLY) for f in (True, False) for r in (True, False)] if every_combination else \
            [(BI, True, True), (BI, False, False), (L0_ONLY, False, k % 2 == 0), (L1_ONLY, True, k % 2 == 1)]
        for pattern, full, legal in combos:
            e0, e1 = entry_pair(rng, legal)
            out.append(dict(w=w, h=h, pattern=pattern, e0=e0, e1=e1, src0=planes(rng, w, h, B, full), src1=planes(rng, w, h, B, full)))
    if not every_combination:
        for cb, kind, args, _ in wo.CLIP_CASES:
            if cb != B:
                continue
            if kind == "uni":
                p, wt, o, d = args
                e0 = e1 = ([wt] * 3, [o] * 3, [d] * 3)
                p0 = p1 = p
                pattern = L0_ONLY
            else:
                p0, p1, w0, w1, o0, o1, d = args
                e0, e1, pattern = ([w0] * 3, [o0] * 3, [d] * 3), ([w1] * 3, [o1] * 3, [d] * 3), BI
            out.append(dict(w=4, h=4, pattern=pattern, e0=e0, e1=e1, src0=[np.full((4 >> s, 4 >> s), p0, np.int16) for s in (0, 1, 1)],
                            src1=[np.full((4 >> s, 4 >> s), p1, np.int16) for s in (0, 1, 1)]))
    return out


# ---- the prediction-unit list: 136x72 = 34 x 18 cells of 4x4, partial 64-wide tiles in both directions ----
PIC_W, PIC_H, MARGIN = 136, 72, 80
ORDER = [0, 1, 0, 1]  # refs[] entry -> picture: both pictures are entered twice, with different rows
N = 255
#        x    y   w   h  ref0 ref1 mv0x  mv0y  mv1x  mv1y
PUS = [(0, 0, 64, 64, 0, 1, -289, -279, 242, 0),        # 64x64, both lists; quarter fractions into the top-left margin, half / zero
       (64, 0, 32, 8, 2, N, 6, -24, 0, 0),              # 2NxnU of a 32x32 unit: 32x8 over 32x24
       (64, 8, 32, 24, 1, 3, -9, 2, 15, -7),
       (96, 0, 8, 32, N, 0, 0, 0, 0, 5),                # nLx2N: 8x32 beside 24x32; list 1 only
       (104, 0, 24, 32, 2, 1, 3, 3, -2, 8),
       (64, 32, 8, 4, 0, N, 4, 0, 0, 0),                # two 8x4 above each other on ONE picture with different rows (entries 0 and 2):
       (64, 36, 8, 4, 2, N, 4, 0, 0, 0),                # the 4x8 cell pairing must split
       (72, 32, 8, 4, N, 1, 0, 0, -6, 1),
       (72, 36, 8, 4, 0, 0, 7, -2, 1, 2),               # both lists on refs[] entry 0: l0[0] and l1[0]
       (64, 40, 4, 8, 1, N, 2, 2, 0, 0),
       (68, 40, 4, 8, N, 3, 0, 0, -5, 6),
       (72, 40, 4, 8, 3, 2, 1, 0, 0, 3),
       (76, 40, 4, 8, 0, 1, -3, -3, 2, -1),
       (80, 32, 16, 4, 1, N, 0, 9, 0, 0),               # 2NxnU of a 16x16 unit: 16x4 over 16x12
       (80, 36, 16, 12, 0, 3, -1, -1, 10, 4),
       (96, 32, 4, 16, N, 2, 0, 0, 11, -6),             # nLx2N of a 16x16 unit: 4x16 beside 12x16
       (100, 32, 12, 16, 3, N, -14, 5, 0, 0),
       (112, 32, 16, 16, 2, 2, 9, -7, 9, -7),           # both lists, one picture, one vector: no identical-motion shortcut under WP
       (64, 48, 16, 16, N, 1, 0, 0, 0, -8),
       (80, 48, 16, 16, 3, 0, 18, 3, -13, -1),
       (96, 48, 32, 16, 0, N, 8, 8, 0, 0),              # integer vector
       (128, 0, 8, 8, 1, N, 281, -2, 0, 0),             # the 8 columns beyond the last whole tile; into the right margin
       (128, 8, 8, 8, N, 2, 0, 0, 276, 3),
       (128, 16, 8, 16, 0, 3, 5, 0, -6, 2),
       (128, 32, 8, 32, 2, N, -1, 2, 0, 0),
       (128, 64, 8, 8, 3, 1, 270, 275, 3, 284),         # bottom-right corner, into both margins
       (0, 64, 8, 8, N, 0, 0, 0, -282, 278),            # the 8 rows below the last whole tile; bottom-left margin
       (8, 64, 8, 4, 1, N, -6, 273, 0, 0),
       (8, 68, 8, 4, N, 1, 0, 0, -6, 273),              # height 4 under height 4: list 0 row above, list 1 row below
       (16, 64, 16, 8, 2, 3, 2, 0, 0, 2),
       (32, 64, 32, 8, 0, 2, -7, 1, 7, -1),
       (64, 64, 64, 8, N, 3, 0, 0, 1, 1)]


def pu_scene(B):
    """pictures (without margins), the unit list and the two tables l0 / l1 indexed like refs[]"""
    rng = np.random.default_rng(6200 + B)
    pics = [[rng.integers(0, 1 << B, (PIC_H >> s, PIC_W >> s)).astype(np.int16) for s in (0, 1, 1)] for _ in range(2)]
    pus = np.zeros(len(PUS), ol.PU_DTYPE)
    for i, t in enumerate(PUS):
        pus[i] = t
    d0 = [[int(v) for v in rng.integers(3, 6, 3)] for _ in range(4)]
    l0 = [fade_entry(rng, d) for d in d0]
    # list 1: weights on list 0's scale (a bi unit of entries (r0, r1) shifts by l0[r0]'s denominator), coded denominators that differ
    l1 = [fade_entry(rng, d0[(r + 1) % 4], [d - 1 if k % 2 else d + 1 for k, d in enumerate(d0[(r + 1) % 4])]) for r in range(4)]
    return dict(pics=pics, pus=pus, order=ORDER, l0=l0, l1=l1)


def check_pu_scene(S):
    """what the list must contain; returns the counts"""
    pus, l0, l1, order = S["pus"], S["l0"], S["l1"], S["order"]
    shapes = {(int(u["w"]), int(u["h"])) for u in pus}
    assert {(8, 4), (4, 8), (64, 64)} <= shapes
    assert {(32, 8), (32, 24), (16, 4), (16, 12)} <= shapes and {(8, 32), (24, 32), (4, 16), (12, 16)} <= shapes  # AMP, both orientations
    cover = np.zeros((PIC_H // 4, PIC_W // 4), np.int32)
    for u in pus:
        x, y, w, h = (int(u[k]) for k in "xywh")
        assert x + w <= PIC_W and y + h <= PIC_H
        cover[y // 4:(y + h) // 4, x // 4:(x + w) // 4] += 1
    assert (cover <= 1).all()  # no overlap: the order of the list does not matter
    by_pos = {(int(u["x"]), int(u["y"])): u for u in pus}

    def rows(u):
        return (None if u["ref0"] == N else l0[u["ref0"]], None if u["ref1"] == N else l1[u["ref1"]])

    n_split = 0
    for u in pus:
        v = by_pos.get((int(u["x"]), int(u["y"]) + 4))
        if u["h"] == 4 and u["y"] % 8 == 0 and v is not None and v["h"] == 4 and rows(u) != rows(v):
            n_split += 1
    assert n_split >= 2
    n_l0 = sum(1 for u in pus if u["ref0"] != N and u["ref1"] == N)
    n_l1 = sum(1 for u in pus if u["ref0"] == N and u["ref1"] != N)
    n_bi = 0
    for u in pus:
        if u["ref0"] != N and u["ref1"] != N:
            a, b = rows(u)
            if all(a[f][c] != b[f][c] for f in range(3) for c in range(3)):
                n_bi += 1
    assert n_l0 >= 4 and n_l1 >= 4 and n_bi >= 4, (n_l0, n_l1, n_bi)
    # a picture entered twice with different rows, and both entries used in each list
    twice = [(a, b) for a in range(4) for b in range(a + 1, 4) if order[a] == order[b]]
    assert twice and all(l0[a] != l0[b] and l1[a] != l1[b] for a, b in twice)
    assert {int(u["ref0"]) for u in pus} >= {0, 1, 2, 3} and {int(u["ref1"]) for u in pus} >= {0, 1, 2, 3}
    frac = [set(), set()]
    reach = set()
    for u in pus:
        for lst, r in ((0, "ref0"), (1, "ref1")):
            if u[r] == N:
                continue
            mvx, mvy = int(u[f"mv{lst}x"]), int(u[f"mv{lst}y"])
            frac[0].add(mvx & 3), frac[1].add(mvy & 3)
            x0, y0, w, h = int(u["x"]) + (mvx >> 2), int(u["y"]) + (mvy >> 2), int(u["w"]), int(u["h"])
            # the 8-tap window stays inside the margin
            assert -MARGIN <= x0 - 3 and x0 + w + 4 <= PIC_W + MARGIN and -MARGIN <= y0 - 3 and y0 + h + 4 <= PIC_H + MARGIN, tuple(u)
            reach |= {s for s, c in (("left", x0 < 0), ("top", y0 < 0), ("right", x0 + w > PIC_W), ("bottom", y0 + h > PIC_H)) if c}
    assert frac[0] == {0, 1, 2, 3} and frac[1] == {0, 1, 2, 3}  # zero, half and both quarter fractions in each direction
    assert reach == {"left", "top", "right", "bottom"}
    return dict(split_pairs=n_split, uni_l0=n_l0, uni_l1=n_l1, bi_all_fields_differ=n_bi)


# ---- reading the committed vectors back (tests/golden/wp_b*.npz, written by tests/golden/make_golden.py wp) ----
def _split(flat, start, w, h):
    out = []
    for s in (0, 1, 1):
        n = (w >> s) * (h >> s)
        out.append(np.ascontiguousarray(flat[start:start + n].reshape(h >> s, w >> s)))
        start += n
    return out


@functools.lru_cache(maxsize=None)
def load_vectors(B):
    """(block cases, unit-list scene): the inputs as block_cases / pu_scene return them, each with the reference's result under
    "out" / "want".  Read once per bit depth and shared read-only."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"wp_b{B}.npz"))
    blocks = []
    for (w, h, pattern, a0, a1, ao), e in zip(g["blk_par"].tolist(), g["blk_e"].tolist()):
        blocks.append(dict(w=w, h=h, pattern=pattern, e0=tuple(e[0]), e1=tuple(e[1]), out=_split(g["blk_out"], ao, w, h),
                           src0=_split(g["blk_s0"], a0, w, h) if pattern != L1_ONLY else None,
                           src1=_split(g["blk_s1"], a1, w, h) if pattern != L0_ONLY else None))
    S = dict(pics=[[np.ascontiguousarray(g[f"pic{i}_{k}"]) for k in ("y", "cb", "cr")] for i in range(2)], pus=g["pu"], order=g["pu_order"].tolist(),
             l0=[tuple(e) for e in g["pu_l0"].tolist()], l1=[tuple(e) for e in g["pu_l1"].tolist()], want=[g["pu_oy"], g["pu_ocb"], g["pu_ocr"]])
    S["ext"] = [([np.pad(p, MARGIN >> (1 if k else 0), mode="edge") for k, p in enumerate(S["pics"][i])], MARGIN) for i in S["order"]]
    for a in [p for b in blocks for key in ("src0", "src1", "out") if b[key] is not None for p in b[key]] + [p for pic in S["pics"] for p in pic] + \
            S["want"] + [p for e, _ in S["ext"] for p in e]:
        a.setflags(write=False)
    return blocks, S
