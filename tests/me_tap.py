"""The calls of TEncSearch::xMotionEstimation that the REFERENCE ENCODER itself made (tests/golden/me_enc_tap.npz, recorded by
oracle/_ref/TAppEncoder_metap: oracle/ref_me_tap.h names every field), for tests/test_me_enc_tap.py and the fixture maker
tests/golden/make_me_enc_tap.py: the file layout, a call as hmx_me_unit / hmx_tz_unit fields, and the classes of calls the
fixture must contain (`classes`, `REQUIRED`)."""
import os

import numpy as np

import me_oracle as mo

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "me_enc_tap.npz")

# the recorder's header words in its order (the H_* enum of oracle/ref_me_tap.h)
FIELDS = ("magic", "poc", "list", "ref_idx", "ref_poc", "cu_x", "cu_y", "x", "y", "w", "h", "bi", "fast_search", "fen", "had_me", "pred_x", "pred_y",
          "mv_in_x", "mv_in_y", "range", "adapt_range", "lam", "bits_in", "bits_out", "cost_out", "left", "top", "right", "bottom", "int_x", "int_y",
          "int_sad", "half_x", "half_y", "qter_x", "qter_y", "frac_cost", "mv_out_x", "mv_out_y", "n_tz", "n_frac", "bits", "pic_w", "pic_h", "ctu")
UNSIGNED = ("lam", "bits_in", "bits_out", "cost_out", "int_sad", "frac_cost")
CALL_MAGIC, PIC_MAGIC = 0x4D454341, 0x4D455049


class Call(dict):
    """The header words by name (costs as unsigned), plus run, org (h, w) int16, trace [(x, y, cost)], frac [18 costs]."""

    @property
    def tz(self):
        return bool(self["fast_search"]) and not self["bi"]  # :4176

    @property
    def sub_shift(self):
        return 1 if self["fen"] and self["h"] > 8 else 0  # :323-330, :4245-4251

    @property
    def pred(self):
        return self["pred_x"], self["pred_y"]

    @property
    def box(self):
        return self["left"], self["top"], self["right"], self["bottom"]

    def unit(self, ref=0):
        """The fields of hmx_me_unit with the recorded box."""
        return {"x": self["x"], "y": self["y"], "w": self["w"], "h": self["h"], "ref": ref, "sub_shift": self.sub_shift, "pred_x": self["pred_x"],
                "pred_y": self["pred_y"], "left": self["left"], "top": self["top"], "right": self["right"], "bottom": self["bottom"]}

    def tz_unit(self):
        """The fields of hmx_tz_unit as xTZSearch makes its start point: rcMv = *pcMvPred (:4182), clipMv, >>= 2 (:4312-4313);
        the range is m_iSearchRange (:4311)."""
        cx, cy = mo.clip_mv(self["pred_x"], self["pred_y"], self["cu_x"], self["cu_y"], self["pic_w"], self["pic_h"], self["ctu"])
        return {"start_x": cx >> 2, "start_y": cy >> 2, "range": self["adapt_range"]}


def make_call(run, run_name, head, org, trace, frac):
    c = Call(zip(FIELDS, (int(v) for v in head)))
    for k in UNSIGNED:
        c[k] &= mo.M32
    c["run"], c.run_name = int(run), str(run_name)
    c.org = np.asarray(org, np.int16).reshape(c["h"], c["w"])
    c.trace = [(int(x), int(y), int(v) & mo.M32) for (x, y, v) in np.asarray(trace).reshape(-1, 3)]
    c.frac = [int(v) & mo.M32 for v in frac]
    return c


class Fixture:
    def __init__(self, runs, calls, pics):
        self.runs, self.calls, self.pics = runs, calls, pics  # pics: {(run, poc): ((mx, my), plane with margins)}

    def ref(self, c):
        return self.pics[(c["run"], c["ref_poc"])]


def save(path, runs, calls, pics):
    org_off = np.concatenate([[0], np.cumsum([c.org.size for c in calls])]).astype(np.int64)
    tz_off = np.concatenate([[0], np.cumsum([len(c.trace) for c in calls])]).astype(np.int64)
    keys = sorted(pics)
    pic_off = np.concatenate([[0], np.cumsum([pics[k][1].size for k in keys])]).astype(np.int64)
    np.savez_compressed(
        path, runs=np.array(runs), run=np.array([c["run"] for c in calls], np.int32),
        head=np.array([[c[k] for k in FIELDS] for c in calls], np.int64).astype(np.uint32).view(np.int32),
        org_off=org_off, org=np.concatenate([c.org.reshape(-1) for c in calls]).astype(np.int16),
        tz_off=tz_off, tz=np.array([p for c in calls for p in c.trace], np.int64).reshape(-1, 3).astype(np.uint32).view(np.int32),
        frac=np.array([c.frac for c in calls], np.uint32),
        pic_head=np.array([[k[0], k[1], pics[k][1].shape[1] - 2 * pics[k][0][0], pics[k][1].shape[0] - 2 * pics[k][0][1], pics[k][0][0], pics[k][0][1]]
                           for k in keys], np.int32),
        pic_off=pic_off, pic=np.concatenate([pics[k][1].reshape(-1) for k in keys]).astype(np.int16))


def load(path=FIXTURE):
    z = np.load(path)
    calls = [make_call(z["run"][i], z["runs"][z["run"][i]], z["head"][i], z["org"][z["org_off"][i]:z["org_off"][i + 1]], z["tz"][z["tz_off"][i]:z["tz_off"][i + 1]], z["frac"][i])
             for i in range(len(z["head"]))]
    pics = {}
    for i, (run, poc, w, h, mx, my) in enumerate(z["pic_head"]):
        pics[(int(run), int(poc))] = ((int(mx), int(my)), z["pic"][z["pic_off"][i]:z["pic_off"][i + 1]].reshape(h + 2 * my, w + 2 * mx))
    return Fixture([str(r) for r in z["runs"]], calls, pics)


def raster_points(box):
    l, t, r, b = box
    return [(x, y) for y in range(t, b + 1, 5) for x in range(l, r + 1, 5)]


def padded_org(c):
    """A picture that holds the recorded block at the unit's position: what the oracles' `org` plane is read at."""
    org = np.zeros((c["pic_h"], c["pic_w"]), np.int16)
    org[c["y"]:c["y"] + c["h"], c["x"]:c["x"] + c["w"]] = c.org
    return org


def cu_origin_decides(c, pic):
    """True when the integer stage answers differently if clipMv is given the UNIT's position where the reference gives it the
    coding unit's (getCUPelX / Y): a second partition whose box or start point the picture border cuts, and whose search goes
    there.  pic = (margin, plane) of the call's reference picture."""
    import tz_oracle as tzo
    if (c["cu_x"], c["cu_y"]) == (c["x"], c["y"]):
        return False
    centre = (c["mv_in_x"], c["mv_in_y"]) if c["bi"] else c.pred
    box = mo.set_search_range(centre[0], centre[1], c["range"], c["x"], c["y"], c["pic_w"], c["pic_h"], c["ctu"])
    cx, cy = mo.clip_mv(c["pred_x"], c["pred_y"], c["x"], c["y"], c["pic_w"], c["pic_h"], c["ctu"])
    z = {"start_x": cx >> 2, "start_y": cy >> 2, "range": c["adapt_range"]}
    if box == c.box and (not c.tz or z == c.tz_unit()):
        return False
    u = c.unit()
    u["left"], u["top"], u["right"], u["bottom"] = box
    margin, ref = pic
    if c.tz:
        res = tzo.search(padded_org(c), ref, margin, u, z, c["lam"], c["bits"])[0]
    else:
        res = mo.search(padded_org(c), ref, margin, u, c["lam"], c["bits"])[0]
    return res[:3] != (c["int_x"], c["int_y"], c["int_sad"])


def classes(c, walk=None, pic=None):
    """The classes a recorded call belongs to, read from the recording alone; `walk` = (passes, labels) of tests/tz_oracle.py for
    a call whose recorded evaluations it reproduced entry for entry adds the two classes that need the walk's state, `pic` (the
    reference picture) the class cu_origin_decides."""
    B = c["bits"]
    out = {"bits_%d" % B, "had_%d" % c["had_me"], "fen_%d" % c["fen"], "sub_shift_%d" % c.sub_shift, "rows_le_8" if c["h"] <= 8 else "rows_gt_8",
           "bi" if c["bi"] else ("tz" if c.tz else "full")}
    if not c["bi"] and c.run_name.startswith("P_"):  # the run's name says what its inter pictures are
        out.add("P_tz" if c.tz else "P_full")
    for k in ("w", "h"):
        if c[k] in (12, 24, 48):
            out.add("%s_%d" % (k, c[k]))
    if c["bi"] and (int(c.org.min()) < 0 or int(c.org.max()) >= (1 << B)):
        out.add("bi_outside_sample_range")
    if pic is not None and cu_origin_decides(c, pic):
        out.add("cu_origin_decides")
    if (c["half_x"], c["half_y"]) != (0, 0):
        out.add("half_winner_not_0")
    if (c["qter_x"], c["qter_y"]) != (0, 0):
        out.add("qter_winner_not_0")
    if c.tz:
        pts = [(x, y) for (x, y, _) in c.trace]
        if pts[0] != (0, 0) and pts[1] == (0, 0) and c.trace[1][2] < c.trace[0][2]:
            out.add("tz_zero_adopted")  # strict < of xTZSearchHelp: the first search starts from the zero vector
        rp = raster_points(c.box)
        if any(pts[i:i + len(rp)] == rp for i in range(2, len(pts) - len(rp) + 1)):
            out.add("tz_raster")
        if walk is not None:
            passes, labels = walk
            if passes >= 2:
                out.add("tz_star_2_passes")
            if any(k.startswith("two_point_") and k != "two_point_0" for k in labels):
                out.add("tz_two_point")
    return out


# Widths and heights of 48 are not in the list: the reference encoder never searches them.  They are the AMP partitions of a
# 64 x 64 coding unit, for which deriveTestModeAMP switches the searched AMP modes off (TEncCu.cpp:352-356) and leaves only the
# merge candidates, which run no motion search.  `classes` still names them should a recording hold one.
REQUIRED = ("P_tz", "P_full", "tz", "full", "bi", "bits_8", "bits_10", "had_0", "had_1", "fen_0", "fen_1", "sub_shift_0", "sub_shift_1", "rows_le_8", "rows_gt_8",
            "w_12", "w_24", "h_12", "h_24", "bi_outside_sample_range", "half_winner_not_0", "qter_winner_not_0",
            "tz_zero_adopted", "tz_raster", "tz_star_2_passes", "tz_two_point", "cu_origin_decides")
