"""tests/golden/aq_stream.npz: the QPs the reference ENCODER coded under --AdaptiveQP=1, held against tests/aq_oracle.py.  The
decision tap does not record CU QPs, so the pin goes through what was coded: oracle/_ref/TAppEncoder (built by
oracle/build_ref_apps.sh) encodes synthetic_clip(..., motion=True), 208x120, 4 pictures, under encoder_lowdelay_P_main.cfg with
--AdaptiveQP=1 --MaxDeltaQP=0 --MaxCuDQPDepth=k --MaxQPAdaptationRange=r and the loop filters off; oracle/_ref/hm_decision_tap reads
the stream back.  For every transform block of an inter coding unit with a non-zero level, the fixture records the set of QPs in
sliceQP +- r for which Clip(motion-compensated prediction + invtransformNxN(levels, QP)) equals the reference decoder's
reconstruction (the recorded reconstructions serve as reference pictures).  With MaxDeltaQP = 0 the coded QP of such a block is
xComputeQP of its coding unit at layer min(depth, k) (TEncCu.cpp:1114-1136), so the QP restated from the ORIGINAL must lie in the
set.  This pins the integer QPs; the bits of the activities rest on the two constructions of tests/test_aq_oracle.py.

  python tests/golden/make_aq_stream.py            # writes tests/golden/aq_stream.npz

Arrays, r = run: n_runs; n_blocks (all runs); run{r}_config [bit depth, k, adaptation range, CTU size, -q]; run{r}_command the
encoder's arguments; run{r}_org [picture in coding order][h][w] the luma originals; run{r}_hdr [picture][poc, slice type];
run{r}_slice_qp [picture]; run{r}_blocks [block][picture, x, y (luma samples of the block's origin), plane, CU size, lo, mask]:
bit j of mask = QP lo + j reproduces the reconstruction.  Data only."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import aq_oracle as ao  # noqa: E402
import oracle_lib as ol  # noqa: E402
from make_stream_golden import PURE, REFBIN, parse_hmxd, synthetic_clip  # noqa: E402
from thevc_amd.decisions import MARGIN, TU_INTER, levels_to_planes, prediction_units, reference_pocs  # noqa: E402

W, H, N_PICS = 208, 120, 4
RUNS = [(8, 2, 6, 64, 30), (10, 3, 6, 64, 30), (8, 0, 6, 64, 30), (8, 1, 10, 32, 30), (10, 1, 3, 16, 30), (8, 2, 12, 64, 22)]  # (bit depth, k, r, CTU, slice QP)
# The clips' seeds.  Every block of every clip tried fitted the restated QP; what varies with the clip is how SHARP the fixture is:
# with seeds 43 / 44 the runs (8, 1, 10, 32, 30) and (10, 1, 3, 16, 30) fell short of the two conditions main() asserts (62 % of the
# blocks identified their QP; 93 blocks moved off the slice QP), so these two runs take the next seeds that meet them.
SEEDS = [40, 41, 42, 53, 64, 45]


def encode(clip, B, k, r, ctu, qp):
    enc, tap = os.path.join(REFBIN, "TAppEncoder"), os.path.join(REFBIN, "hm_decision_tap")
    if not (os.path.exists(enc) and os.path.exists(tap)):
        subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref_apps.sh")])
    with tempfile.TemporaryDirectory() as d:
        yuv, bit, out = (os.path.join(d, f) for f in ("in.yuv", "str.bin", "out.hmxd"))
        with open(yuv, "wb") as f:
            for planes in clip:
                for p in planes:
                    f.write(p.astype(np.uint8 if B == 8 else "<u2").tobytes())
        log2ctu = ctu.bit_length() - 1
        cmd = [enc, "-c", os.path.join("/root/reference/cfg", "encoder_lowdelay_P_main.cfg"), "-i", yuv, "-wdt", str(W), "-hgt", str(H), "-fr", "30",
               "-f", str(len(clip)), "-q", str(qp), "-b", bit, "-o", os.path.join(d, "rec.yuv"), "--SEIpictureDigest=1", f"--InputBitDepth={B}",
               f"--InternalBitDepth={B}", f"--MaxCUSize={ctu}", f"--MaxPartitionDepth={log2ctu - 2}", f"--QuadtreeTULog2MaxSize={min(5, log2ctu)}",
               "--AdaptiveQP=1", "--MaxDeltaQP=0", f"--MaxCuDQPDepth={k}", f"--MaxQPAdaptationRange={r}"] + PURE
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        subprocess.run([tap, bit, out], check=True, stdout=subprocess.DEVNULL)
        return parse_hmxd(out), " ".join(c for c in cmd[1:] if not c.startswith(d))


def extend(rec):
    O, planes = ol.oracle(), []
    for k, a in enumerate(rec):
        pm = MARGIN if k == 0 else MARGIN // 2
        ph, pw = a.shape
        e = np.zeros((ph + 2 * pm, pw + 2 * pm), np.int16)
        e[pm:pm + ph, pm:pm + pw] = a
        flat = e.reshape(-1)
        O.hmo_extendPicBorder(ol.ptr(flat, pm * (pw + 2 * pm) + pm), pw + 2 * pm, pw, ph, pm, pm)
        planes.append(flat)
    return planes


def blocks_of(pics, r):
    """Per picture in coding order: (picture, x, y, plane, CU size, lo, mask) of every inter transform block with a level"""
    O = ol.oracle()
    P3, I3 = C.c_void_p * 3, C.c_int * 3
    ext, out = {}, []
    for i, p in enumerate(pics):
        w, h, B, m = p["w"], p["h"], p["B"], MARGIN
        if len(p["pus"]):
            pred = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
            pocs = reference_pocs(p)
            pus = prediction_units(p, {poc: j for j, poc in enumerate(pocs)})
            ptrs = (C.c_void_p * (3 * len(pocs)))()
            for j, poc in enumerate(pocs):
                for k in range(3):
                    pm, pw = (m, w) if k == 0 else (m // 2, w // 2)
                    ptrs[j * 3 + k] = ext[poc][k].ctypes.data + 2 * (pm * (pw + 2 * pm) + pm)
            O.hmo_mc_frame(pus.ctypes.data, len(pus), B, ptrs, I3(w + 2 * m, w // 2 + m, w // 2 + m), P3(*[a.ctypes.data for a in pred]), I3(w, w // 2, w // 2))
            lev, mx = levels_to_planes(p), (1 << B) - 1
            cu_size = np.zeros((h // 8, w // 8), np.int32)  # the size of the coding unit that covers each 8x8
            for c in p["cus"]:
                s = 1 << int(c["log2size"])
                cu_size[int(c["y"]) // 8:(int(c["y"]) + s) // 8, int(c["x"]) // 8:(int(c["x"]) + s) // 8] = s
            for t in p["tus"]:
                if not int(t["flags"]) & TU_INTER:
                    continue
                n, k, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
                if not lev[k][y:y + n, x:x + n].any():
                    continue
                lo, mask = p["qp"] - r, 0
                for j in range(2 * r + 1):
                    q = O.hmo_setQPforQuant(lo + j, int(k != 0), 6 * (B - 8), 0)
                    res = ol.o_invtransformNxN(lev[k][y:y + n, x:x + n], n, B, 65535, q.per, q.rem, int(t["flags"]) & 1)
                    if np.array_equal(np.clip(pred[k][y:y + n, x:x + n].astype(np.int32) + res, 0, mx), p["rec"][k][y:y + n, x:x + n]):
                        mask |= 1 << j
                lx, ly = (x, y) if k == 0 else (2 * x, 2 * y)
                out.append((i, lx, ly, k, int(cu_size[ly // 8, lx // 8]), lo, mask))
        ext[p["poc"]] = extend(p["rec"])
    return out


def main():
    arrays, total = {"n_runs": np.int32(len(RUNS))}, 0
    for run, (B, k, r, ctu, qp) in enumerate(RUNS):
        clip = synthetic_clip(SEEDS[run], W, H, N_PICS, B, motion=True)
        pics, command = encode(clip, B, k, r, ctu, qp)
        assert all(p["ctu"] == ctu and p["B"] == B for p in pics)
        blocks = blocks_of(pics, r)
        g = ao.Geom(W, H, ctu, k + 1)
        stats = [ao.preanalyze(clip[p["poc"]][0], ctu, k + 1) for p in pics]
        unique = moved = 0
        offsets = set()
        for i, x, y, plane, cu, lo, mask in blocks:
            act, avg = stats[i]
            want = ao.compute_qp(g, act, avg, x, y, ctu.bit_length() - cu.bit_length(), pics[i]["qp"], r, 6 * (B - 8))
            assert lo <= want <= lo + 2 * r and (mask >> (want - lo)) & 1, (run, i, x, y, plane, cu, want, bin(mask))
            unique += mask == 1 << (want - lo)
            moved += want != pics[i]["qp"] and not (mask >> r) & 1
            offsets.add(want - pics[i]["qp"])
        print(f"run {run} {(B, k, r, ctu, qp)}: {len(blocks)} blocks, {unique} identify their QP, {moved} moved off a slice QP that does not fit, "
              f"offsets {min(offsets)}..{max(offsets)}, slice QPs {[p['qp'] for p in pics]}")
        assert unique >= 0.7 * len(blocks), "fewer than 70 % of the blocks identify their QP"
        assert moved >= 100, "fewer than 100 blocks with a non-zero offset that the slice QP does not fit"
        arrays[f"run{run}_config"] = np.array([B, k, r, ctu, qp], np.int32)
        arrays[f"run{run}_command"] = np.array(command)
        arrays[f"run{run}_org"] = np.stack([clip[p["poc"]][0] for p in pics]).astype(np.uint8 if B == 8 else np.int16)
        arrays[f"run{run}_hdr"] = np.array([[p["poc"], p["slice_type"]] for p in pics], np.int32)
        arrays[f"run{run}_slice_qp"] = np.array([p["qp"] for p in pics], np.int32)
        arrays[f"run{run}_blocks"] = np.array(blocks, np.int64).reshape(-1, 7)
        total += len(blocks)
    arrays["n_blocks"] = np.int32(total)
    path = os.path.join(HERE, "aq_stream.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(RUNS)} runs, {total} blocks, {os.path.getsize(path)} bytes")
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
