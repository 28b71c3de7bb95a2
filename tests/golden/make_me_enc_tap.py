"""tests/golden/me_enc_tap.npz: the calls of TEncSearch::xMotionEstimation the REFERENCE ENCODER itself made -- per call what the
function was given (the unit, the predictor, the search box xSetSearchRange left, the cost multiplier, the pattern key's luma
block, which for bi-prediction is 2 * org - other), every xTZSearchHelp evaluation in order, the integer stage's answer, all
eighteen costs of the two xPatternRefinement calls, the half- and quarter-sample winners and the bits and cost returned --
and the luma plane of every reference picture with its margins.  Recorded by oracle/_ref/TAppEncoder_metap (the reference
encoder with recorder statements between the statements of its own motion search: oracle/ref_me_tap.h,
oracle/ref_shim_edit.py TEncSearch metap, oracle/build_ref_enc_shim.sh) on the RUNS below; per run and class of call (kind,
reference index, width, height) a few calls spread over the run are kept, and every call of the rarer classes tests/me_tap.py names until each
has its share.  The maker checks that the recording encoder wrote the bitstream of the unmodified one, that the recorded costs reproduce
with the recovered cost multiplier, and FAILS if a required class is missing from the kept calls.  Needs oracle/_ref (build container).

  python tests/golden/make_me_enc_tap.py
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
import me_oracle as mo  # noqa: E402
import me_tap as mt  # noqa: E402
import subpel_oracle as so  # noqa: E402
import tz_oracle as tzo  # noqa: E402
from enc_shim_cases import options  # noqa: E402
from make_stream_golden import synthetic_clip  # noqa: E402

ENC = os.path.join(ROOT, "oracle", "_ref", "TAppEncoder_metap")
PLAIN = os.path.join(ROOT, "oracle", "_ref", "TAppEncoder")
OUT = os.path.join(HERE, "me_enc_tap.npz")
LIMIT = os.path.getsize(os.path.join(HERE, "rdoq_enc_tap.npz"))
PER_CLASS = 2   # calls kept per (run, kind, reference index, width, height)
PER_RARE = 4    # calls kept per run of each class of RARE
RARE = ("cu_origin_decides", "tz_zero_adopted", "tz_raster", "tz_star_2_passes", "tz_two_point", "bi_outside_sample_range", "w_24", "h_24", "w_12", "h_12")

P_FRAME = "--Frame1=P 1 0 0.5 0 1 1 1 -1 0"          # one reference: the previous picture
B_FRAME = "--Frame1=B 1 0 0.5 0 2 1 2 -1 -2 0"       # both lists hold the two previous pictures: uni-predictive and bBi calls
RUNS = [
    # name (P_ / B_ says what the inter pictures are), clip, switches on top of enc_shim_cases.options
    {"name": "P_tz_fen_had_b8", "seed": 71, "w": 192, "h": 128, "frames": 3, "bits": 8, "qp": 30, "pan": (11, 7),
     "extra": [P_FRAME, "--FastSearch=1", "--FEN=1", "--HadamardME=1", "--SearchRange=16"]},
    {"name": "P_full_b8", "seed": 72, "w": 128, "h": 128, "frames": 2, "bits": 8, "qp": 32, "pan": (5, 3),
     "extra": [P_FRAME, "--FastSearch=0", "--FEN=0", "--HadamardME=0", "--SearchRange=8"]},
    {"name": "P_tz_b10", "seed": 73, "w": 128, "h": 128, "frames": 3, "bits": 10, "qp": 28, "pan": (9, 12),
     "extra": [P_FRAME, "--FastSearch=1", "--FEN=0", "--HadamardME=0", "--SearchRange=16"]},
    {"name": "B_tz_fen_had_b10", "seed": 74, "w": 128, "h": 128, "frames": 3, "bits": 10, "qp": 30, "pan": (6, 4),
     "extra": [B_FRAME, "--FastSearch=1", "--FEN=1", "--HadamardME=1", "--SearchRange=16", "--BipredSearchRange=4"]},
    {"name": "B_full_fen_b8", "seed": 75, "w": 128, "h": 128, "frames": 3, "bits": 8, "qp": 34, "pan": (3, 5),
     "extra": [B_FRAME, "--FastSearch=0", "--FEN=1", "--HadamardME=0", "--SearchRange=8", "--BipredSearchRange=4"]},
    {"name": "P_full_fen_had_b10", "seed": 76, "w": 128, "h": 128, "frames": 2, "bits": 10, "qp": 33, "pan": (4, 6),
     "extra": [P_FRAME, "--FastSearch=0", "--FEN=1", "--HadamardME=1", "--SearchRange=8"]},
]


def fast_clip(run):
    """synthetic_clip's still picture as a canvas seen through a window that pans `pan` luma samples per picture -- further than
    synthetic_clip's own 4 x 2, so that walks leave the first diamonds and reach the raster search -- with one object moving
    against the pan and one that stands still on the screen, and a little fresh noise per picture."""
    w, h, n, B = run["w"], run["h"], run["frames"], run["bits"]
    rng = np.random.default_rng(run["seed"])
    mx = (1 << B) - 1
    px, py = run["pan"]
    canvas = synthetic_clip(run["seed"] + 1000, w + 2 * px * n + 16, h + 2 * py * n + 16, 1, B, smooth=True)[0]
    out = []
    for i in range(n):
        planes = []
        for k, c in enumerate(canvas):
            s = 1 if k else 0
            ox, oy = (8 + 2 * (px // 2) * i) >> s, (8 + 2 * (py // 2) * i) >> s
            p = c[oy:oy + (h >> s), ox:ox + (w >> s)].astype(np.float64)
            bx, by = (w - 40 - 2 * (px // 2) * i) >> s, (24 + 4 * i) >> s  # against the pan
            yy, xx = np.mgrid[0:(24 >> s), 0:(32 >> s)]
            p[by:by + (24 >> s), bx:bx + (32 >> s)] = (0.25 + 0.5 * ((xx // (4 >> s) + yy // (4 >> s)) % 2)) * mx
            p[(h - 32) >> s:(h - 8) >> s, 8 >> s:40 >> s] = (0.6 if k == 0 else 0.4) * mx  # stands still: the zero vector
            p += rng.normal(0, 0.003 * mx, p.shape)
            planes.append(np.clip(np.rint(p), 0, mx).astype(np.uint16))
        out.append(planes)
    return out


def write_clip(run, path):
    with open(path, "wb") as f:
        for planes in fast_clip(run):
            for p in planes:
                f.write(p.astype(np.uint8 if run["bits"] == 8 else "<u2").tobytes())
    return path


def run_options(run, yuv, stream, recon):
    case = dict(run, inter=True)
    mine = {e.split("=")[0] for e in run["extra"]} | {"--NSQT"}
    base = [o for o in options(case, yuv, stream, recon) if o.split("=")[0] not in mine]
    # the non-square Hadamard shapes are not covered by the library (a reference built with REMOVE_NSQT has none and answers
    # that it does not know the switch); weighted prediction stays off
    return base + run["extra"] + ["--NSQT=0"]


def records(path, run, name):
    """(calls, pics) of one recorder file."""
    data = open(path, "rb").read()
    off, calls, pics = 0, [], {}
    nw = len(mt.FIELDS)
    while off < len(data):
        magic = int(np.frombuffer(data, "<i4", 1, off)[0])
        if magic == mt.PIC_MAGIC:
            _, poc, w, h, mx, my = (int(v) for v in np.frombuffer(data, "<i4", 6, off))
            off += 24
            n = (h + 2 * my) * (w + 2 * mx)
            pics[(run, poc)] = ((mx, my), np.frombuffer(data, "<i2", n, off).reshape(h + 2 * my, w + 2 * mx).copy())
            off += 2 * n
            continue
        assert magic == mt.CALL_MAGIC, hex(magic)
        head = np.frombuffer(data, "<i4", nw, off)
        off += 4 * nw
        c = dict(zip(mt.FIELDS, (int(v) for v in head)))
        org = np.frombuffer(data, "<i2", c["w"] * c["h"], off)
        off += 2 * c["w"] * c["h"]
        tz = np.frombuffer(data, "<i4", 3 * c["n_tz"], off)
        off += 12 * c["n_tz"]
        frac = np.frombuffer(data, "<u4", 18, off)
        off += 72
        assert c["n_frac"] == 18, c["n_frac"]
        calls.append(mt.make_call(run, name, head, org, tz, frac))
    return calls, pics


def check_costs(c, pic):
    """The recorded costs reproduce with the recovered cost multiplier (m_uiLambdaMotionSAD)."""
    (mx, my), ref = pic
    lam, B = c["lam"], c["bits"]
    assert 0 < lam < (1 << 32)
    # the vector term of the integer stage: the first evaluation of a TZ walk is SAD + getCost at cost scale 2
    if c.tz:
        x, y, cost = c.trace[0]
        blk = ref[my + c["y"] + y:my + c["y"] + y + c["h"], mx + c["x"] + x:mx + c["x"] + x + c["w"]]
        assert cost == (mo.sad(c.org, blk, c.sub_shift, B) + mo.mv_cost(lam, x, y, c["pred_x"], c["pred_y"], 2)) & mo.M32, ("trace[0]", c)
    blk = ref[my + c["y"] + c["int_y"]:my + c["y"] + c["int_y"] + c["h"], mx + c["x"] + c["int_x"]:mx + c["x"] + c["int_x"] + c["w"]]
    assert c["int_sad"] == mo.sad(c.org, blk, c.sub_shift, B), ("ruiSAD", c)
    # candidate 0 of the half-sample stage is the integer position: its distortion needs no interpolation when it is a SAD
    if not c["had_me"]:
        d = (int(np.abs(c.org.astype(np.int64) - blk).sum()) & mo.M32) >> (B - 8)
        assert c.frac[0] == (d + mo.mv_cost(lam, 2 * c["int_x"], 2 * c["int_y"], c["pred_x"], c["pred_y"], 1)) & mo.M32, ("frac[0]", c)
    # the tail: ruiBits and ruiCost
    bits, cost = so.me_tail(lam, c.pred, c["mv_out_x"], c["mv_out_y"], c["frac_cost"], c["bits_in"], 0.5 if c["bi"] else 1.0)
    assert (bits, cost) == (c["bits_out"], c["cost_out"]), ("tail", c, bits, cost)
    assert (c["mv_out_x"], c["mv_out_y"]) == (4 * c["int_x"] + 2 * c["half_x"] + c["qter_x"], 4 * c["int_y"] + 2 * c["half_y"] + c["qter_y"])


def walk_of(c, pic):
    """(passes, labels) of tests/tz_oracle.py when it reproduces the recorded evaluations, else None."""
    (mx, my), ref = pic
    _, trace, passes, labels = tzo.search(mt.padded_org(c), ref, (mx, my), c.unit(), c.tz_unit(), c["lam"], c["bits"])
    return (passes, labels) if trace == c.trace else None


def main():
    runs, keep, pics = [r["name"] for r in RUNS], [], {}
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
        # a unit is searched many times over (every partition of every CU size, every reference): a call is worth keeping once
        cls = []
        for c in calls:
            assert c["bits"] == run["bits"]
            cls.append(mt.classes(c, walk_of(c, rp[(ri, c["ref_poc"])]) if c.tz else None, rp[(ri, c["ref_poc"])]))
        chosen = set()
        by_class = {}
        for k, c in enumerate(calls):
            by_class.setdefault(("bi" if c["bi"] else "tz" if c.tz else "full", c["ref_idx"], c["w"], c["h"]), []).append(k)
        for key, idx in sorted(by_class.items()):
            chosen.update(idx[int(j)] for j in np.linspace(0, len(idx) - 1, min(PER_CLASS, len(idx))))
        for name in RARE:
            idx = [k for k in range(len(calls)) if name in cls[k]]
            idx.sort(key=lambda k: calls[k].org.size + 6 * len(calls[k].trace))  # the small ones: the fixture has a size limit
            have = sum(name in cls[k] for k in chosen)
            chosen.update(idx[:max(0, PER_RARE - have)])
        count = {}
        for k in sorted(chosen):
            check_costs(calls[k], rp[(ri, calls[k]["ref_poc"])])
            keep.append(calls[k])
            pics[(ri, calls[k]["ref_poc"])] = rp[(ri, calls[k]["ref_poc"])]
            for name in cls[k]:
                count[name] = count.get(name, 0) + 1
        print(run["name"], len(calls), "calls,", len(chosen), "kept:", dict(sorted(count.items())))
    mt.save(OUT, runs, keep, pics)
    fx = mt.load(OUT)
    total = {}
    for c in fx.calls:
        for name in mt.classes(c, walk_of(c, fx.ref(c)) if c.tz else None, fx.ref(c)):
            total[name] = total.get(name, 0) + 1
    print("kept", len(fx.calls), "calls,", len(fx.pics), "reference pictures:", dict(sorted(total.items())))
    size = os.path.getsize(OUT)
    print(OUT, size, "bytes")
    missing = [name for name in mt.REQUIRED if not total.get(name)]
    if missing:
        raise SystemExit("make_me_enc_tap: classes missing from the kept calls: " + ", ".join(missing))
    if size > LIMIT:
        raise SystemExit(f"make_me_enc_tap: {size} bytes, above the {LIMIT} of rdoq_enc_tap.npz")


if __name__ == "__main__":
    main()
