"""tests/golden/wp_estimate.npz: what the reference ENCODER decided in WeightPredAnalysis (TLibEncoder/WeightPredAnalysis.cpp), held
against everything it decided from.  Fading clips are encoded by oracle/_ref/TAppEncoder with weighted prediction on, the streams
are read back by oracle/_ref/hm_decision_tap (both built by oracle/build_ref_apps.sh), and per run the fixture stores, picture
by picture in coding order: the ORIGINAL the encoder read, the reconstruction, and the weight tables of the slice header with the
POC of every entry.  tests/wp_estimate_oracle.py and hmx_wp_estimate_slices must reproduce every table from the pictures.

  python tests/golden/make_wp_estimate.py            # writes tests/golden/wp_estimate.npz

Arrays, r = run, i = picture in coding order, k = component, l = list:
  runs                     the runs' names;   r{r}_n  pictures;   r{r}_command  the encoder's arguments
  r{r}_hdr{i}              [poc, w, h, B, slice_type (0 B, 1 P, 2 I), weighted]
  r{r}_org{i}_{k}          the encoder's input picture of that POC;   r{r}_rec{i}_{k}  the reconstruction
  r{r}_wppoc{i}_{l}        the POC of every entry of list l (inter slices, weighted or not)
  r{r}_wptab{i}_{l}        [entry][component][weight, offset, log2 denominator], weighted slices only
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import wp_estimate_oracle as wo  # noqa: E402
from make_stream_golden import PURE, REFBIN, parse_hmxd, synthetic_clip, weighted  # noqa: E402


def fading_clip(seed, w, h, n, B, stop=None):
    """make_stream_golden.fading_clip (the same pictures for stop = None); from picture `stop` on the gain and the step stay what
    they were there, so that a later picture and a reference from that stretch differ by motion only"""
    mx = (1 << B) - 1
    mid, unit = (mx + 1) / 2, 1 << (B - 8)
    out = []
    for i, planes in enumerate(synthetic_clip(seed, w, h, n, B, False, True)):
        f = i if stop is None else min(i, stop)
        fade = []
        for k, p in enumerate(planes):
            gain, step = (1.0 - 0.08 * f, 5 * f * unit) if k == 0 else (1.0 - 0.06 * f, (-4 if k == 1 else 3) * f * unit)
            fade.append(np.clip(np.rint((p.astype(np.float64) - mid) * gain + mid + step), 0, mx).astype(np.uint16))
        out.append(fade)
    return out


def encode(clip, w, h, B, qp, cfg, extra):
    enc, tap = os.path.join(REFBIN, "TAppEncoder"), os.path.join(REFBIN, "hm_decision_tap")
    if not (os.path.exists(enc) and os.path.exists(tap)):
        subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref_apps.sh")])
    with tempfile.TemporaryDirectory() as d:
        yuv, bit, out = (os.path.join(d, f) for f in ("in.yuv", "str.bin", "out.hmxd"))
        with open(yuv, "wb") as f:
            for planes in clip:
                for p in planes:
                    f.write(p.astype(np.uint8 if B == 8 else "<u2").tobytes())
        cmd = [enc, "-c", os.path.join("/root/reference/cfg", cfg), "-i", yuv, "-wdt", str(w), "-hgt", str(h), "-fr", "30",
               "-f", str(len(clip)), "-q", str(qp), "-b", bit, "-o", os.path.join(d, "rec.yuv"), "--SEIpictureDigest=1", f"--InputBitDepth={B}",
               f"--InternalBitDepth={B}"] + list(extra)
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        subprocess.run([tap, bit, out], check=True, stdout=subprocess.DEVNULL)
        return parse_hmxd(out), " ".join(c for c in cmd[1:] if not c.startswith(d))


def slices_of(run):
    """The inter slices of a run as the oracle takes them: (picture index, org, AC/DC, per list the AC/DC of the entries' originals
    and their reconstructions, recorded tables or None)."""
    by_poc = {p["poc"]: p for p in run["pics"]}
    stats = {poc: wo.acdc(run["clip"][poc]) for poc in by_poc}
    for i, p in enumerate(run["pics"]):
        if p["slice_type"] == 2:
            continue
        pocs = [[int(q) for q in p["wp"]["poc"][l]] for l in (0, 1) if len(p["wp"]["poc"][l])]
        yield (i, run["clip"][p["poc"]], stats[p["poc"]], [[stats[q] for q in l] for l in pocs], [[by_poc[q]["rec"] for q in l] for l in pocs],
               [np.asarray(t) for t in p["wp"]["tab"]] if weighted(p) else None)


def census(run, cnt):
    """Run the oracle over every slice of the run against the recording and count the branches reached."""
    B = run["B"]
    for i, org, cur, racdc, rrec, want in slices_of(run):
        tabs, present, d, is_w = wo.estimate_slice(org, cur, racdc, rrec, B)
        cnt["slices"] += 1
        if want is None:
            assert not is_w, (run["name"], i)
            cnt["slices_unweighted"] += 1
            continue
        # a slice whose entries xSelectWP all rejected is written with the rows xCheckWPEnable leaves, (1, 0, 0): the stream's PPS
        # keeps its flag, so the tap still shows tables, and they are compared like any others
        assert is_w == any((np.asarray(t)[:, :, 2] != 0).any() for t in want), (run["name"], i)
        cnt["slices_all_rejected"] += int(not is_w)
        for l in range(len(racdc)):
            assert np.array_equal(tabs[l], want[l]), (run["name"], i, l, tabs[l].tolist(), want[l].tolist())
            cnt["lists"] += 1
            cnt["entries"] += len(tabs[l])
            cnt["entries_rejected"] += sum(not k for k in present[l])
        if is_w:
            cnt[f"slices_denom{d}"] = cnt.get(f"slices_denom{d}", 0) + 1
        cnt["slices_kept_beside_rejected"] += int(any(not k for l in present for k in l) and any(k for l in present for k in l))
        raw, _ = wo.update_params(cur, racdc[0], racdc[1] if len(racdc) > 1 else [], B)
        for l, t in enumerate(raw):
            for e, rows in enumerate(t):
                for c in (1, 2):
                    cnt["chroma_offsets_at_a_clip"] += int(rows[c][1] in (-128, 127) and present[l][e])
                cnt["luma_offsets_outside_int8"] += int(not -128 <= rows[0][1] <= 127)
        start = 7 if len(racdc[0]) > 3 else 6
        cnt["slices_denominator_lowered"] += int(d < start)


def main():
    runs = []
    for name, seed, w, h, n, B, qp, cfg, extra, stop in (
            # the two clips of the stream fixtures (make_stream_golden.py), with the same arguments
            ("lowdelay_P_wp_q30", 25, 192, 128, 4, 8, 30, "encoder_lowdelay_P_main.cfg", PURE + ["-wpP", "1"], None),
            ("randomaccess_wp_q32", 26, 192, 128, 5, 8, 32, "encoder_randomaccess_main.cfg", ["-wpP", "1", "-wpB", "1"], None),
            # 10 bit, B slices
            ("randomaccess_he10_wp_q32", 27, 128, 64, 5, 10, 32, "encoder_randomaccess_he10.cfg", ["-wpP", "1", "-wpB", "1"], None),
            # seven pictures of low delay P: list 0 reaches four entries and the denominator starts at 7
            ("lowdelay_P_wp7_q30", 28, 128, 64, 7, 8, 30, "encoder_lowdelay_P_main.cfg", PURE + ["-wpP", "1"], None),
            # the fade stops at picture 1: later pictures see references of their own level (rejected) beside faded ones (kept), the last only such
            ("lowdelay_P_wpstop_q30", 29, 128, 64, 6, 8, 30, "encoder_lowdelay_P_main.cfg", PURE + ["-wpP", "1"], 1)):
        clip = fading_clip(seed, w, h, n, B, stop)
        pics, command = encode(clip, w, h, B, qp, cfg, extra)
        runs.append(dict(name=name, B=B, clip=clip, pics=pics, command=command))
    cnt = dict(slices=0, slices_unweighted=0, slices_all_rejected=0, lists=0, entries=0, entries_rejected=0, slices_kept_beside_rejected=0, chroma_offsets_at_a_clip=0,
               luma_offsets_outside_int8=0, slices_denominator_lowered=0)
    arrays = {"runs": np.array([r["name"] for r in runs])}
    for r, run in enumerate(runs):
        census(run, cnt)
        arrays[f"r{r}_n"], arrays[f"r{r}_command"] = np.int32(len(run["pics"])), np.array(run["command"])
        small = np.uint8 if run["B"] == 8 else np.int16
        for i, p in enumerate(run["pics"]):
            arrays[f"r{r}_hdr{i}"] = np.array([p["poc"], p["w"], p["h"], p["B"], p["slice_type"], int(weighted(p))], np.int32)
            for k in range(3):
                arrays[f"r{r}_org{i}_{k}"] = run["clip"][p["poc"]][k].astype(small)
                arrays[f"r{r}_rec{i}_{k}"] = p["rec"][k].astype(small)
            if p["slice_type"] != 2:
                for l in (0, 1):
                    arrays[f"r{r}_wppoc{i}_{l}"] = p["wp"]["poc"][l]
                    if weighted(p):
                        arrays[f"r{r}_wptab{i}_{l}"] = p["wp"]["tab"][l]
    print("wp_estimate:", cnt)
    assert cnt.get("slices_denom7", 0) > 0, "no slice at denominator 7"
    assert cnt["slices_kept_beside_rejected"] > 0, "no rejected entry beside a kept one"
    assert cnt["slices_all_rejected"] > 0, "no slice that xCheckWPEnable turned off"
    path = os.path.join(HERE, "wp_estimate.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(runs)} runs, {sum(len(r['pics']) for r in runs)} pictures, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
