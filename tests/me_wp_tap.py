"""The calls of TEncSearch::xMotionEstimation that the REFERENCE ENCODER made in WEIGHTED slices (tests/golden/me_wp_enc_tap.npz),
for tests/test_me_wp_enc_tap.py and the maker tests/golden/make_me_wp_enc_tap.py.  The call data is tests/me_tap.py's format,
unchanged; beside it the file holds, per call,
  wp        int16 (n, 3): (iWeight, iOffset, uiLog2WeightDenom) of the luma wpScalingParam of the (POC, list, reference index) searched,
            recovered by decoding the run's stream;
  applied   uint8 (n): 1 = the recorded costs reproduce with the weighted distortion, 0 = they reproduce only unweighted (the encoder
            may clear the slice's flag when every weight is the default); nothing is assumed about which of the two a slice got.
`classes` names what a call proves about the weighted search; a call counts only when its entry is not the default, it was
weighted, and its recorded costs differ from what the unweighted oracles give for the same call."""
import os

import numpy as np

import me_oracle as mo
import me_tap as mt
import me_wp_oracle as wo
import subpel_oracle as so

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "me_wp_enc_tap.npz")
REQUIRED = ("P_uni", "B_list0", "B_list1", "bBi", "tz", "full", "had_0", "had_1", "fen_rows_gt_8", "bits_8", "bits_10", "offset_nonzero")


def load(path=FIXTURE):
    """me_tap.load's Fixture with .wp = [(weight, offset, log2_denom)] and .applied = [bool], parallel to .calls."""
    fx = mt.load(path)
    z = np.load(path)
    fx.wp = [tuple(int(v) for v in r) for r in z["wp"]]
    fx.applied = [bool(v) for v in z["applied"]]
    assert len(fx.wp) == len(fx.applied) == len(fx.calls)
    return fx


def save(path, runs, calls, pics, wp, applied):
    mt.save(path, runs, calls, pics)
    z = dict(np.load(path))
    z["wp"], z["applied"] = np.array(wp, np.int16).reshape(len(calls), 3), np.array(applied, np.uint8)
    np.savez_compressed(path, **z)


def is_default(wp):
    return wp[0] == (1 << wp[2]) and wp[1] == 0


def recorded(c):
    """The costs of a call the maker requires an oracle to reproduce: the first TZ evaluation, ruiSAD, the 18 fractional costs."""
    return (c.trace[0][2] if c.tz else None, c["int_sad"], list(c.frac))


def expected(c, pic, wp):
    """`recorded` from the oracles at the recorded vectors (integer vector, half-sample winner): weighted with the entry wp, or
    unweighted for wp = None."""
    (mx, my), ref = pic
    lam, B = c["lam"], c["bits"]
    e = wo.entry(*wp, B) if wp is not None else None

    def sad(x, y):
        blk = ref[my + c["y"] + y:my + c["y"] + y + c["h"], mx + c["x"] + x:mx + c["x"] + x + c["w"]]
        return wo.sad_w(c.org, blk, e, B, c.sub_shift) if e else mo.sad(c.org, blk, c.sub_shift, B)
    first = None
    if c.tz:
        x, y, _ = c.trace[0]
        first = (sad(x, y) + mo.mv_cost(lam, x, y, c["pred_x"], c["pred_y"], 2)) & mo.M32
    ix, iy = c["int_x"], c["int_y"]
    args = (c.org, ref, mx + c["x"] + ix, my + c["y"] + iy, B, c["had_me"], lam, c.pred, ix, iy)
    half = (c["half_x"], c["half_y"])
    frac = wo.stage_costs(*args, e) + wo.stage_costs(*args, e, half) if e else so.stage_costs(*args) + so.stage_costs(*args, half)
    return (first, sad(ix, iy), frac)


def tail_holds(c):
    """The tail of xMotionEstimation (:4197-4205) on the recorded quarter-stage cost, and the vector assembled from the stages."""
    bits, cost = so.me_tail(c["lam"], c.pred, c["mv_out_x"], c["mv_out_y"], c["frac_cost"], c["bits_in"], 0.5 if c["bi"] else 1.0)
    k = so.REFINE_Q.index((c["qter_x"], c["qter_y"]))
    return ((bits, cost) == (c["bits_out"], c["cost_out"]) and c.frac[9 + k] == c["frac_cost"] == min(c.frac[9:]) and
            (c["mv_out_x"], c["mv_out_y"]) == (4 * c["int_x"] + 2 * c["half_x"] + c["qter_x"], 4 * c["int_y"] + 2 * c["half_y"] + c["qter_y"]))


def classes(c, wp, applied, differs):
    """The REQUIRED classes a call stands for; none unless it was weighted with a non-default entry and shows it."""
    if not applied or is_default(wp) or not differs:
        return set()
    out = {"bits_%d" % c["bits"], "had_%d" % c["had_me"]}
    if c["bi"]:
        out.add("bBi")
    else:
        out.add("tz" if c.tz else "full")
        out.add("P_uni" if c.run_name.startswith("P_") else "B_list%d" % c["list"])  # the run's name says what its inter pictures are
    if c["fen"] and c["h"] > 8:
        out.add("fen_rows_gt_8")  # xTZSearchHelp / xPatternSearch set iSubShift = 1 and xGetSADw ignores it
    if wp[1] != 0:
        out.add("offset_nonzero")
    return out
