"""tests/golden/me_wp_enc_tap.npz: calls of TEncSearch::xMotionEstimation the REFERENCE ENCODER made in slices under explicit
weighted prediction (-wpP 1 / -wpB 1), where setWpScalingDistParam switches every distortion of the search to the weighted one
(xGetSADw, xGetHADsw).  The recorder is the one of tests/golden/make_me_enc_tap.py (oracle/_ref/TAppEncoder_metap) on fading
clips with motion; per run the maker
  checks that the unmodified TAppEncoder writes the same stream;
  decodes that stream with the decision tap (oracle/_ref/hm_decision_tap) to recover every slice's weight tables, and keys each
  recorded call to its luma entry by (POC, list, reference index), the entry's POC checked against the recorded reference POC;
  keeps a few calls per class of call, and of each call decides from its recorded costs alone -- the first TZ evaluation, ruiSAD,
  all 18 fractional costs -- whether the slice was searched weighted or not (tests/me_wp_tap.py: `applied`); a call that
  reproduces neither way stops the maker, and so does a wrong tail.
It FAILS unless every class of me_wp_tap.REQUIRED is present among kept calls that were weighted with a non-default entry and
whose recorded costs differ from the unweighted oracles'.  Needs oracle/_ref (build container).

  python tests/golden/make_me_wp_enc_tap.py
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import me_wp_tap as wt  # noqa: E402
from make_me_enc_tap import ENC, LIMIT, P_FRAME, PLAIN, records, run_options  # noqa: E402
from make_stream_golden import fading_clip, parse_hmxd  # noqa: E402

TAP = os.path.join(ROOT, "oracle", "_ref", "hm_decision_tap")
OUT = os.path.join(HERE, "me_wp_enc_tap.npz")
PER_CLASS = 2  # calls kept per (run, POC, kind, list, reference index, width, height)
WP_P, WP_B = ["--weighted_pred_flag=1"], ["--weighted_bipred_flag=1"]
# make_me_enc_tap's B_FRAME holds the same two pictures in both lists, and the uni-predictive search then runs on list 0 alone: a
# list-1 entry whose picture is also in list 0 takes list 0's result (TEncSearch.cpp:3341-3356).  Here a GOP of two with one
# active reference per list: POC 2 from POC 0, then POC 1 between them with list 0 = (POC 0) and list 1 = (POC 2), so that both
# lists are searched, each picture under its own entry.
B_GOP = ["--GOPSize=2", "--Frame1=B 2 0 0.5 0 1 1 1 -2 0", "--Frame2=B 1 0 0.5 0 1 0 2 -1 1 0"]
RUNS = [
    # name (P_ / B_ says what the inter pictures are), clip (make_stream_golden.fading_clip), switches on top of enc_shim_cases.options
    {"name": "P_tz_fen_had_b8", "seed": 81, "w": 128, "h": 128, "frames": 3, "bits": 8, "qp": 30,
     "extra": [P_FRAME, "--FastSearch=1", "--FEN=1", "--HadamardME=1", "--SearchRange=16"] + WP_P},
    {"name": "P_full_b8", "seed": 82, "w": 128, "h": 128, "frames": 2, "bits": 8, "qp": 32,
     "extra": [P_FRAME, "--FastSearch=0", "--FEN=0", "--HadamardME=0", "--SearchRange=8"] + WP_P},
    {"name": "P_tz_b10", "seed": 83, "w": 128, "h": 128, "frames": 3, "bits": 10, "qp": 28,
     "extra": [P_FRAME, "--FastSearch=1", "--FEN=0", "--HadamardME=0", "--SearchRange=16"] + WP_P},
    {"name": "B_tz_fen_had_b10", "seed": 84, "w": 128, "h": 128, "frames": 3, "bits": 10, "qp": 30,
     "extra": B_GOP + ["--FastSearch=1", "--FEN=1", "--HadamardME=1", "--SearchRange=16", "--BipredSearchRange=4"] + WP_B},
    {"name": "B_full_fen_b8", "seed": 85, "w": 128, "h": 128, "frames": 3, "bits": 8, "qp": 34,
     "extra": B_GOP + ["--FastSearch=0", "--FEN=1", "--HadamardME=0", "--SearchRange=8", "--BipredSearchRange=4"] + WP_B},
    {"name": "P_full_fen_had_b10", "seed": 86, "w": 128, "h": 128, "frames": 2, "bits": 10, "qp": 33,
     "extra": [P_FRAME, "--FastSearch=0", "--FEN=1", "--HadamardME=1", "--SearchRange=8"] + WP_P},
]


def write_clip(run, path):
    with open(path, "wb") as f:
        for planes in fading_clip(run["seed"], run["w"], run["h"], run["frames"], run["bits"]):
            for p in planes:
                f.write(p.astype(np.uint8 if run["bits"] == 8 else "<u2").tobytes())
    return path


def entry_of(c, slices):
    """(iWeight, iOffset, uiLog2WeightDenom) of the luma row the call's (POC, list, reference index) names in the decoded tables."""
    s = slices[c["poc"]]["wp"]
    assert int(s["poc"][c["list"]][c["ref_idx"]]) == c["ref_poc"], ("the decoded list does not hold the recorded reference", c)
    return tuple(int(v) for v in s["tab"][c["list"]][c["ref_idx"]][0])


def judge(c, pic, wp):
    """(applied, differs) from the recorded costs alone."""
    rec = wt.recorded(c)
    as_w, as_u = wt.expected(c, pic, wp) == rec, wt.expected(c, pic, None) == rec
    if not (as_w or as_u):
        raise SystemExit("make_me_wp_enc_tap: a call reproduces neither weighted nor unweighted: %r entry %r" % (dict(c), wp))
    if not wt.tail_holds(c):
        raise SystemExit("make_me_wp_enc_tap: the tail of a call does not reproduce: %r" % dict(c))
    return as_w, not as_u


def main():
    runs, keep, pics, wps, applied = [r["name"] for r in RUNS], [], {}, [], []
    total = {}
    for ri, run in enumerate(RUNS):
        with tempfile.TemporaryDirectory() as d:
            yuv = write_clip(run, os.path.join(d, "in.yuv"))
            tap = os.path.join(d, "tap.bin")
            subprocess.run([ENC] + run_options(run, yuv, os.path.join(d, "s.bin"), os.path.join(d, "rec.yuv")), check=True, stdout=subprocess.DEVNULL,
                           env=dict(os.environ, HMX_ME_TAP=tap))
            calls, rp = records(tap, ri, run["name"])
            # the recorder only reads: the unmodified encoder writes the same bitstream
            subprocess.run([PLAIN] + run_options(run, yuv, os.path.join(d, "p.bin"), os.path.join(d, "rec.yuv")), check=True, stdout=subprocess.DEVNULL)
            assert open(os.path.join(d, "s.bin"), "rb").read() == open(os.path.join(d, "p.bin"), "rb").read(), run["name"]
            subprocess.run([TAP, os.path.join(d, "p.bin"), os.path.join(d, "out.hmxd")], check=True, stdout=subprocess.DEVNULL)
            slices = {p["poc"]: p for p in parse_hmxd(os.path.join(d, "out.hmxd"))}
        flags = {poc: p["wp"]["flags"] for poc, p in sorted(slices.items()) if p["slice_type"] != 2}
        by_class = {}
        for k, c in enumerate(calls):
            assert c["bits"] == run["bits"]
            by_class.setdefault((c["poc"], "bi" if c["bi"] else "tz" if c.tz else "full", c["list"], c["ref_idx"], c["w"], c["h"]), []).append(k)
        chosen = set()
        for key, idx in sorted(by_class.items()):
            chosen.update(idx[int(j)] for j in np.linspace(0, len(idx) - 1, min(PER_CLASS, len(idx))))
        count, n_applied = {}, 0
        for k in sorted(chosen):
            c = calls[k]
            pic = rp[(ri, c["ref_poc"])]
            wp = entry_of(c, slices)
            a, differs = judge(c, pic, wp)
            keep.append(c)
            wps.append(wp)
            applied.append(a)
            pics[(ri, c["ref_poc"])] = pic
            n_applied += a
            for name in wt.classes(c, wp, a, differs):
                count[name] = count.get(name, 0) + 1
                total[name] = total.get(name, 0) + 1
        entries = sorted({(c["poc"], c["list"], c["ref_idx"]) + entry_of(c, slices) for c in calls})
        print(run["name"], len(calls), "calls,", len(chosen), "kept,", n_applied, "searched weighted; PPS flags (use_wp, wp_bipred) by POC:", flags)
        print("   luma entries (POC, list, reference index, weight, offset, log2 denominator):", entries)
        print("   classes:", dict(sorted(count.items())))
    wt.save(OUT, runs, keep, pics, wps, applied)
    fx = wt.load(OUT)
    assert len(fx.calls) == len(keep) and fx.wp == wps and fx.applied == applied
    size = os.path.getsize(OUT)
    print("kept", len(fx.calls), "calls,", sum(applied), "searched weighted,", len(fx.pics), "reference pictures; class counts:", dict(sorted(total.items())))
    print(OUT, size, "bytes")
    missing = [name for name in wt.REQUIRED if not total.get(name)]
    if missing:
        raise SystemExit("make_me_wp_enc_tap: classes missing from the kept calls: " + ", ".join(missing))
    if size > LIMIT:
        raise SystemExit(f"make_me_wp_enc_tap: {size} bytes, above the {LIMIT} of rdoq_enc_tap.npz")


if __name__ == "__main__":
    main()
