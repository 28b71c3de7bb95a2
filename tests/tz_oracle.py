"""Numpy / Python restatement of TEncSearch::xTZSearch (TEncSearch.cpp:4302-4474) as the reference compiles it
(TZ_SEARCH_CONFIGURATION, :293-309, with FASTME_SMOOTHER_MV 1), for the tests of hmx_batch_tz_search.

The walk is TABLE-DRIVEN here: a pattern is a list of (dx, dy, point number, distance) in evaluation order, and a point is
evaluated when every coordinate that moves away from the pattern's centre stays on the side of the box it moves towards.  That
one rule covers the "whole pattern inside" fast paths and the border paths of xTZ8PointDiamondSearch (:536-707) and the eight
cases of xTZ2PointSearch (:351-479).  tests/test_tz_oracle.py holds the second construction, written call site by call site
from the reference, and compares the two traces.

  walk(cost, box, start, range_)   over any cost function cost(x, y) -> UInt
  search(org, ref, margin, u, z, lam, B)   cost = me_oracle.sad + me_oracle.mv_cost at cost scale 2 (xTZSearchHelp, :312-349)

Like tests/me_oracle.py this is pinned on the compiled reference by recorded calls: tests/test_me_enc_tap.py requires `search`
to give, entry for entry, every xTZSearchHelp evaluation (point and cost) that the reference encoder's own xTZSearch made in the
TZ calls of tests/golden/me_enc_tap.npz (oracle/ref_me_tap.h records them) -- walks that adopt the zero vector, run the raster
search, two and more star passes and the 2-point search among them -- and its result.  On the GPU every trace entry inside the
box is also held against hmx_batch_fullpel_search's cost map, which is cross-checked against the pinned hmx_batch_subpel_cost
(tests/test_gpu_tz_search.py).

The zero vector is evaluated unconditionally and may lie outside the box; the border rule tests only the moving coordinate,
so a walk that adopts it evaluates points outside the box.  Every evaluated point lies inside the bounding rectangle of
box U {(0, 0)}: `Walk.help` asserts it at every evaluation."""
import numpy as np

import me_oracle as mo

M32 = mo.M32
RASTER = 5
FIRST_SEARCH_ROUNDS = 3
PASS_CAP = 1024

# xTZ2PointSearch: ucPointNr -> the two points in evaluation order
TWO_POINT = {1: ((-1, 0), (0, -1)), 2: ((-1, -1), (1, -1)), 3: ((0, -1), (1, 0)), 4: ((-1, 1), (-1, -1)),
             5: ((1, -1), (1, 1)), 6: ((-1, 0), (0, 1)), 7: ((-1, 1), (1, 1)), 8: ((1, 0), (0, 1))}


def diamond(d):
    """The pattern of xTZ8PointDiamondSearch at iDist = d: [(dx, dy, ucPointNr, uiDistance)] in evaluation order."""
    if d == 1:
        return [(0, -1, 2, 1), (-1, 0, 4, 1), (1, 0, 5, 1), (0, 1, 7, 1)]
    if d <= 8:
        e = d >> 1
        return [(0, -d, 2, d), (-e, -e, 1, e), (e, -e, 3, e), (-d, 0, 4, d), (d, 0, 5, d), (-e, e, 6, e), (e, e, 8, e), (0, d, 7, d)]
    pts = [(0, -d, 0, d), (-d, 0, 0, d), (d, 0, 0, d), (0, d, 0, d)]
    for i in (1, 2, 3):
        q = (d >> 2) * i
        pts += [(-q, q - d, 0, d), (q, q - d, 0, d), (-q, d - q, 0, d), (q, d - q, 0, d)]
    return pts


class Walk:
    def __init__(self, cost, box, max_passes=PASS_CAP):
        self.cost, self.box, self.max_passes = cost, box, max_passes
        self.best, self.bx, self.by, self.dist, self.round, self.nr = M32, 0, 0, 0, 0, 0
        self.trace, self.labels, self.passes, self.capped = [], set(), 0, False
        l, t, r, b = box
        self.rect = (min(l, 0), min(t, 0), max(r, 0), max(b, 0))

    def in_box(self, x, y):
        l, t, r, b = self.box
        return l <= x <= r and t <= y <= b

    def help(self, x, y, nr, dist):
        """xTZSearchHelp: strict <."""
        rl, rt, rr, rb = self.rect
        assert rl <= x <= rr and rt <= y <= rb, ("evaluated point outside box U {(0, 0)}", (x, y), self.box)
        c = self.cost(x, y) & M32
        self.trace.append((x, y, c))
        if c < self.best:
            self.best, self.bx, self.by, self.dist, self.round, self.nr = c, x, y, dist, 0, nr

    def pattern(self, sx, sy, pts):
        l, t, r, b = self.box
        for (dx, dy, nr, dist) in pts:
            x, y = sx + dx, sy + dy
            if (dx >= 0 or x >= l) and (dx <= 0 or x <= r) and (dy >= 0 or y >= t) and (dy <= 0 or y <= b):
                self.help(x, y, nr, dist)

    def diamond(self, sx, sy, d):
        l, t, r, b = self.box
        self.round += 1
        whole = sy - d >= t and sx - d >= l and sx + d <= r and sy + d <= b
        self.labels.add("diamond_1" if d == 1 else ("diamond_2_8_" if d <= 8 else "diamond_gt8_") + ("inside" if whole else "border"))
        self.pattern(sx, sy, diamond(d))

    def two_point(self):
        if self.nr == 0:
            self.labels.add("two_point_0")  # the reference asserts here
            return
        self.labels.add("two_point_%d" % self.nr)
        self.pattern(self.bx, self.by, [(dx, dy, 0, 2) for (dx, dy) in TWO_POINT[self.nr]])

    def run(self, start, range_):
        l, t, r, b = self.box
        self.help(start[0], start[1], 0, 0)
        self.help(0, 0, 0, 0)
        zero_out = (self.bx, self.by) == (0, 0) and not self.in_box(0, 0)
        sx, sy = self.bx, self.by
        d = 1
        while d <= range_:  # first search
            self.diamond(sx, sy, d)
            if self.round >= FIRST_SEARCH_ROUNDS:
                if (self.bx, self.by) == tuple(start) and self.dist == 0:
                    self.labels.add("start_wins_round3")
                break
            d *= 2
        if self.dist == 1:
            self.dist = 0
            self.two_point()
        if self.dist > RASTER:
            self.labels.add("raster")
            self.dist = RASTER
            for y in range(t, b + 1, RASTER):
                for x in range(l, r + 1, RASTER):
                    self.help(x, y, 0, RASTER)
        else:
            self.labels.add("no_raster")
        while self.dist > 0:  # star refinement
            if self.passes >= self.max_passes:
                self.capped = True
                break
            self.passes += 1
            sx, sy = self.bx, self.by
            self.dist, self.nr = 0, 0
            d = 1
            while d <= range_:
                self.diamond(sx, sy, d)
                d *= 2
            if self.dist == 1:
                self.dist = 0
                if self.nr != 0:
                    self.two_point()
        if self.passes >= 2:
            self.labels.add("star_2_passes")
        if zero_out and any(not self.in_box(x, y) for (x, y, _) in self.trace[2:]):
            self.labels.add("zero_outside_adopted")
        return self


def walk(cost, box, start, range_, max_passes=PASS_CAP):
    """box = (left, top, right, bottom) inclusive; returns the Walk: .bx .by .best .trace .passes .labels .capped."""
    return Walk(cost, box, max_passes).run(start, range_)


def cost_fn(org, ref, margin, u, lam, B):
    """cost(x, y) of xTZSearchHelp for one unit (fields of hmx_me_unit), memoised."""
    x0, y0, w, h, s = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"]), int(u["sub_shift"])
    px, py = int(u["pred_x"]), int(u["pred_y"])
    ob = np.asarray(org)[y0:y0 + h, x0:x0 + w]
    X0, Y0 = margin[0] + x0, margin[1] + y0
    memo = {}

    def cost(x, y):
        if (x, y) not in memo:
            assert Y0 + y >= 0 and X0 + x >= 0 and Y0 + y + h <= ref.shape[0] and X0 + x + w <= ref.shape[1]
            memo[(x, y)] = (mo.sad(ob, ref[Y0 + y:Y0 + y + h, X0 + x:X0 + x + w], s, B) + mo.mv_cost(lam, x, y, px, py, 2)) & M32
        return memo[(x, y)]
    return cost


def search(org, ref, margin, u, z, lam, B, max_passes=PASS_CAP):
    """((mvx, mvy, sad, cost), trace, passes, labels) of one unit; z: fields of hmx_tz_unit.  A capped walk answers with the
    best so far and sad = cost = 0xFFFFFFFF."""
    box = (int(u["left"]), int(u["top"]), int(u["right"]), int(u["bottom"]))
    w = walk(cost_fn(org, ref, margin, u, lam, B), box, (int(z["start_x"]), int(z["start_y"])), int(z["range"]), max_passes)
    if w.capped:
        res = (w.bx, w.by, M32, M32)
    else:
        res = (w.bx, w.by, (w.best - mo.mv_cost(lam, w.bx, w.by, int(u["pred_x"]), int(u["pred_y"]), 2)) & M32, w.best)
    return res, w.trace, w.passes, w.labels
