"""tests/tz_oracle.py (table-driven) against a second construction of xTZSearch written here call site by call site from the
reference (TEncSearch.cpp:312-349, :351-479, :536-707, :4302-4474, with the switches of TZ_SEARCH_CONFIGURATION that are off
left out): identical traces on a few thousand random units over synthetic cost functions and on every unit of the GPU fixture
set (tests/tz_fixture.py); the rectangle assertion; and the proof that the fixture set reaches every branch the GPU test is
meant to cover.  No GPU needed."""
import numpy as np
import pytest

import me_oracle as mo
import tz_fixture as tf
import tz_oracle as tzo

M32 = mo.M32


class Struct:  # IntTZSearchStruct
    pass


class Literal:
    """The reference's member functions, statement by statement; iSrchRng* are the four sides of the box."""

    def __init__(self, cost, box):
        self.cost = cost
        self.iSrchRngHorLeft, self.iSrchRngVerTop, self.iSrchRngHorRight, self.iSrchRngVerBottom = box
        self.trace = []

    def xTZSearchHelp(self, rcStruct, iSearchX, iSearchY, ucPointNr, uiDistance):
        uiSad = self.cost(iSearchX, iSearchY) & M32
        self.trace.append((iSearchX, iSearchY, uiSad))
        if uiSad < rcStruct.uiBestSad:
            rcStruct.uiBestSad = uiSad
            rcStruct.iBestX = iSearchX
            rcStruct.iBestY = iSearchY
            rcStruct.uiBestDistance = uiDistance
            rcStruct.uiBestRound = 0
            rcStruct.ucPointNr = ucPointNr

    def xTZ2PointSearch(self, rcStruct):
        L, R, T, B = self.iSrchRngHorLeft, self.iSrchRngHorRight, self.iSrchRngVerTop, self.iSrchRngVerBottom
        iStartX, iStartY = rcStruct.iBestX, rcStruct.iBestY
        h = lambda x, y: self.xTZSearchHelp(rcStruct, x, y, 0, 2)
        nr = rcStruct.ucPointNr
        if nr == 1:
            if (iStartX - 1) >= L:
                h(iStartX - 1, iStartY)
            if (iStartY - 1) >= T:
                h(iStartX, iStartY - 1)
        elif nr == 2:
            if (iStartY - 1) >= T:
                if (iStartX - 1) >= L:
                    h(iStartX - 1, iStartY - 1)
                if (iStartX + 1) <= R:
                    h(iStartX + 1, iStartY - 1)
        elif nr == 3:
            if (iStartY - 1) >= T:
                h(iStartX, iStartY - 1)
            if (iStartX + 1) <= R:
                h(iStartX + 1, iStartY)
        elif nr == 4:
            if (iStartX - 1) >= L:
                if (iStartY + 1) <= B:
                    h(iStartX - 1, iStartY + 1)
                if (iStartY - 1) >= T:
                    h(iStartX - 1, iStartY - 1)
        elif nr == 5:
            if (iStartX + 1) <= R:
                if (iStartY - 1) >= T:
                    h(iStartX + 1, iStartY - 1)
                if (iStartY + 1) <= B:
                    h(iStartX + 1, iStartY + 1)
        elif nr == 6:
            if (iStartX - 1) >= L:
                h(iStartX - 1, iStartY)
            if (iStartY + 1) <= B:
                h(iStartX, iStartY + 1)
        elif nr == 7:
            if (iStartY + 1) <= B:
                if (iStartX - 1) >= L:
                    h(iStartX - 1, iStartY + 1)
                if (iStartX + 1) <= R:
                    h(iStartX + 1, iStartY + 1)
        elif nr == 8:
            if (iStartX + 1) <= R:
                h(iStartX + 1, iStartY)
            if (iStartY + 1) <= B:
                h(iStartX, iStartY + 1)
        else:
            assert False, "xTZ2PointSearch with ucPointNr 0"

    def xTZ8PointDiamondSearch(self, rcStruct, iStartX, iStartY, iDist):
        L, R, T, B = self.iSrchRngHorLeft, self.iSrchRngHorRight, self.iSrchRngVerTop, self.iSrchRngVerBottom
        h = lambda x, y, nr, d: self.xTZSearchHelp(rcStruct, x, y, nr, d)
        assert iDist != 0
        iTop, iBottom, iLeft, iRight = iStartY - iDist, iStartY + iDist, iStartX - iDist, iStartX + iDist
        rcStruct.uiBestRound += 1
        if iDist == 1:
            if iTop >= T:
                h(iStartX, iTop, 2, iDist)
            if iLeft >= L:
                h(iLeft, iStartY, 4, iDist)
            if iRight <= R:
                h(iRight, iStartY, 5, iDist)
            if iBottom <= B:
                h(iStartX, iBottom, 7, iDist)
        elif iDist <= 8:
            iTop_2, iBottom_2 = iStartY - (iDist >> 1), iStartY + (iDist >> 1)
            iLeft_2, iRight_2 = iStartX - (iDist >> 1), iStartX + (iDist >> 1)
            if iTop >= T and iLeft >= L and iRight <= R and iBottom <= B:
                h(iStartX, iTop, 2, iDist)
                h(iLeft_2, iTop_2, 1, iDist >> 1)
                h(iRight_2, iTop_2, 3, iDist >> 1)
                h(iLeft, iStartY, 4, iDist)
                h(iRight, iStartY, 5, iDist)
                h(iLeft_2, iBottom_2, 6, iDist >> 1)
                h(iRight_2, iBottom_2, 8, iDist >> 1)
                h(iStartX, iBottom, 7, iDist)
            else:
                if iTop >= T:
                    h(iStartX, iTop, 2, iDist)
                if iTop_2 >= T:
                    if iLeft_2 >= L:
                        h(iLeft_2, iTop_2, 1, iDist >> 1)
                    if iRight_2 <= R:
                        h(iRight_2, iTop_2, 3, iDist >> 1)
                if iLeft >= L:
                    h(iLeft, iStartY, 4, iDist)
                if iRight <= R:
                    h(iRight, iStartY, 5, iDist)
                if iBottom_2 <= B:
                    if iLeft_2 >= L:
                        h(iLeft_2, iBottom_2, 6, iDist >> 1)
                    if iRight_2 <= R:
                        h(iRight_2, iBottom_2, 8, iDist >> 1)
                if iBottom <= B:
                    h(iStartX, iBottom, 7, iDist)
        else:
            if iTop >= T and iLeft >= L and iRight <= R and iBottom <= B:
                h(iStartX, iTop, 0, iDist)
                h(iLeft, iStartY, 0, iDist)
                h(iRight, iStartY, 0, iDist)
                h(iStartX, iBottom, 0, iDist)
                for index in range(1, 4):
                    iPosYT = iTop + ((iDist >> 2) * index)
                    iPosYB = iBottom - ((iDist >> 2) * index)
                    iPosXL = iStartX - ((iDist >> 2) * index)
                    iPosXR = iStartX + ((iDist >> 2) * index)
                    h(iPosXL, iPosYT, 0, iDist)
                    h(iPosXR, iPosYT, 0, iDist)
                    h(iPosXL, iPosYB, 0, iDist)
                    h(iPosXR, iPosYB, 0, iDist)
            else:
                if iTop >= T:
                    h(iStartX, iTop, 0, iDist)
                if iLeft >= L:
                    h(iLeft, iStartY, 0, iDist)
                if iRight <= R:
                    h(iRight, iStartY, 0, iDist)
                if iBottom <= B:
                    h(iStartX, iBottom, 0, iDist)
                for index in range(1, 4):
                    iPosYT = iTop + ((iDist >> 2) * index)
                    iPosYB = iBottom - ((iDist >> 2) * index)
                    iPosXL = iStartX - ((iDist >> 2) * index)
                    iPosXR = iStartX + ((iDist >> 2) * index)
                    if iPosYT >= T:
                        if iPosXL >= L:
                            h(iPosXL, iPosYT, 0, iDist)
                        if iPosXR <= R:
                            h(iPosXR, iPosYT, 0, iDist)
                    if iPosYB <= B:
                        if iPosXL >= L:
                            h(iPosXL, iPosYB, 0, iDist)
                        if iPosXR <= R:
                            h(iPosXR, iPosYB, 0, iDist)

    def xTZSearch(self, rcMv, uiSearchRange, max_passes=tzo.PASS_CAP):
        """rcMv: after clipMv and >>= 2.  Returns (iBestX, iBestY, uiBestSad or all ones when the pass cap is reached, passes)."""
        iRaster, uiFirstSearchRounds = 5, 3
        cStruct = Struct()
        cStruct.uiBestSad = M32
        self.xTZSearchHelp(cStruct, rcMv[0], rcMv[1], 0, 0)
        self.xTZSearchHelp(cStruct, 0, 0, 0, 0)  # bTestZeroVector
        iStartX, iStartY = cStruct.iBestX, cStruct.iBestY
        iDist = 1
        while iDist <= uiSearchRange:
            self.xTZ8PointDiamondSearch(cStruct, iStartX, iStartY, iDist)
            if cStruct.uiBestRound >= uiFirstSearchRounds:  # bFirstSearchStop
                break
            iDist *= 2
        if cStruct.uiBestDistance == 1:
            cStruct.uiBestDistance = 0
            self.xTZ2PointSearch(cStruct)
        if cStruct.uiBestDistance > iRaster:
            cStruct.uiBestDistance = iRaster
            iStartY = self.iSrchRngVerTop
            while iStartY <= self.iSrchRngVerBottom:
                iStartX = self.iSrchRngHorLeft
                while iStartX <= self.iSrchRngHorRight:
                    self.xTZSearchHelp(cStruct, iStartX, iStartY, 0, iRaster)
                    iStartX += iRaster
                iStartY += iRaster
        passes = 0
        if cStruct.uiBestDistance > 0:  # bStarRefinementEnable
            while cStruct.uiBestDistance > 0:
                if passes >= max_passes:  # the library's guard, not the reference's
                    return cStruct.iBestX, cStruct.iBestY, M32, passes
                passes += 1
                iStartX, iStartY = cStruct.iBestX, cStruct.iBestY
                cStruct.uiBestDistance = 0
                cStruct.ucPointNr = 0
                iDist = 1
                while iDist < uiSearchRange + 1:
                    self.xTZ8PointDiamondSearch(cStruct, iStartX, iStartY, iDist)
                    iDist *= 2
                if cStruct.uiBestDistance == 1:
                    cStruct.uiBestDistance = 0
                    if cStruct.ucPointNr != 0:
                        self.xTZ2PointSearch(cStruct)
        return cStruct.iBestX, cStruct.iBestY, cStruct.uiBestSad, passes


def both(cost, box, start, range_, max_passes=tzo.PASS_CAP):
    w = tzo.walk(cost, box, start, range_, max_passes)
    lit = Literal(cost, box)
    bx, by, best, passes = lit.xTZSearch(start, range_, max_passes)
    assert w.trace == lit.trace, (box, start, range_)
    assert (w.bx, w.by, M32 if w.capped else w.best, w.passes) == (bx, by, best, passes), (box, start, range_)
    return w


def synthetic_cost(rng, kind):
    """A cost function on the plane: a bowl around a random target plus noise, pure noise, few distinct values (ties), constant."""
    tx, ty = int(rng.integers(-70, 71)), int(rng.integers(-70, 71))
    a, b, salt = int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 1 << 30))

    def noise(x, y, m):
        return ((x * 73856093) ^ (y * 19349663) ^ salt) % m
    if kind == 0:
        return lambda x, y: a * abs(x - tx) + b * abs(y - ty) + noise(x, y, 2 * (a + b))
    if kind == 1:
        return lambda x, y: (a * (x - tx) ** 2 + b * (y - ty) ** 2) // 8 + noise(x, y, 7)
    if kind == 2:
        return lambda x, y: noise(x, y, 100000)
    if kind == 3:
        return lambda x, y: noise(x, y, 3)
    return lambda x, y: 1000


def random_case(rng):
    range_ = int(rng.choice([1, 2, 3, 5, 8, 16, 31, 64]))
    cx, cy = int(rng.integers(-70, 71)), int(rng.integers(-70, 71))
    l, t = cx - int(rng.integers(0, range_ + 1)), cy - int(rng.integers(0, range_ + 1))
    r, b = cx + int(rng.integers(0, range_ + 1)), cy + int(rng.integers(0, range_ + 1))
    start = (int(rng.integers(l, r + 1)), int(rng.integers(t, b + 1)))
    return (l, t, r, b), start, range_


def test_constructions_agree_on_random_units():
    rng = np.random.default_rng(4242)
    labels, n = set(), 0
    for k in range(3000):
        box, start, range_ = random_case(rng)
        w = both(synthetic_cost(rng, k % 5), box, start, range_)  # the rectangle assertion runs inside tzo.walk
        labels |= w.labels
        n += len(w.trace)
    assert "two_point_0" not in labels
    assert {"two_point_%d" % k for k in range(1, 9)} <= labels and {"raster", "star_2_passes", "zero_outside_adopted", "diamond_gt8_border"} <= labels
    assert n > 100000


def test_pass_cap_agrees():
    rng = np.random.default_rng(4243)
    capped = 0
    for k in range(400):
        box, start, range_ = random_case(rng)
        cost = synthetic_cost(rng, k % 2)
        full = both(cost, box, start, range_)
        for cap in (1, 2):
            w = both(cost, box, start, range_, cap)
            assert w.capped == (full.passes > cap)
            assert w.trace == full.trace[:len(w.trace)]
            capped += w.capped
    assert capped > 50


def test_rectangle_assertion_fires():
    """The assertion is live: a cost function that lures the walk is not enough to leave the rectangle, a wrong rule is."""
    w = tzo.Walk(lambda x, y: 0, (10, 10, 20, 20))
    with pytest.raises(AssertionError, match="outside box"):
        w.help(21, 21, 0, 0)
    w.help(0, 0, 0, 0)
    w.help(20, 0, 0, 0)  # inside the rectangle of box U {(0, 0)}, outside the box


def fixture_walks(B):
    out = []
    for sc in tf.scenes(B):
        for u, z in zip(sc.units, sc.tz):
            cost = tzo.cost_fn(sc.org, sc.refs[int(u["ref"])], (tf.M, tf.M), u, sc.lam, B)
            box = (int(u["left"]), int(u["top"]), int(u["right"]), int(u["bottom"]))
            out.append((sc, u, z, both(cost, box, (int(z["start_x"]), int(z["start_y"])), int(z["range"]))))
    return out


# two_point_0 (the first 2-point call with ucPointNr == 0) is not in the list: it is unreachable.  uiBestDistance == 1 is only
# ever assigned by an xTZSearchHelp call that passes distance 1, and every such call site (the 4-point diamond, the diagonal
# points of the iDist = 2 diamond) passes a point number of 1 .. 8 in the same call; both fields are written together.  The
# walks below and the 3000 random ones above never reach it, and the literal construction asserts if they did.
LABELS = {"start_wins_round3", "zero_outside_adopted", "diamond_1", "diamond_2_8_inside", "diamond_2_8_border", "diamond_gt8_inside",
          "diamond_gt8_border", "raster", "no_raster", "star_2_passes"} | {"two_point_%d" % k for k in range(1, 9)}


@pytest.mark.parametrize("B", [8, 10])
def test_fixture_set_reaches_every_branch(B):
    walks = fixture_walks(B)  # the two constructions agree on every fixture unit
    seen = set()
    for _, _, _, w in walks:
        seen |= w.labels
    assert seen == LABELS, (LABELS - seen, seen - LABELS)
    # diamond > 8 on the border path at a picture corner, where hmx_setSearchRange cut the box
    assert any("diamond_gt8_border" in w.labels and (int(u["x"]), int(u["y"])) in ((0, 0), (tf.W - 16, 0), (0, tf.H - 16), (tf.W - 16, tf.H - 16))
               and int(u["right"]) - int(u["left"]) < 128 for _, u, _, w in walks)
    # a tie resolved by evaluation order: constant pictures, lambda 0, the first evaluated point wins
    ties = [(u, z, w) for sc, u, z, w in walks if sc.name == "constant"]
    assert ties and all(sc.lam == 0 for sc in tf.scenes(B) if sc.name == "constant")
    for u, z, w in ties:
        assert len({c for (_, _, c) in w.trace}) == 1 and (w.bx, w.by) == (int(z["start_x"]), int(z["start_y"])) == w.trace[0][:2]
    units = np.concatenate([sc.units for sc in tf.scenes(B)])
    assert set(units["sub_shift"]) == {0, 1}
    assert set(units["w"]) == set(mo.SIZES) == set(units["h"]) and any(u["w"] != u["h"] for u in units)
    # the GPU test's other needs: a unit of at least two passes with a neighbour, TZ ending above the box minimum and at it
    assert max(w.passes for _, _, _, w in walks) >= 2
    assert max(len(w.trace) for _, _, _, w in walks) < 1024  # the trace capacity of the GPU test


def test_fixture_dtypes_equal_capi():
    from thevc_amd import capi
    assert tf.ME_UNIT_DTYPE == capi.ME_UNIT_DTYPE and tf.TZ_UNIT_DTYPE == capi.TZ_UNIT_DTYPE
    assert capi.TZ_POINT_DTYPE.itemsize == 8 and capi.TZ_UNIT_DTYPE.itemsize == 8
