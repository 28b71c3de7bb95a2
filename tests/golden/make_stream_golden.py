"""Fixtures from REAL reference streams: a synthetic clip is encoded by the reference's own
encoder (oracle/_ref/TAppEncoder, built by oracle/build_ref_apps.sh), the stream is decoded by the reference's decoder
library under oracle/ref_decision_tap.cpp, and every picture's decision list (transform blocks, levels) is stored
with the reference decoder's reconstruction.  Needs /root/reference (not on the GPU box); the .npz travels.

  python tests/golden/make_stream_golden.py            # writes tests/golden/stream_*.npz
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REFBIN = os.path.join(ROOT, "oracle", "_ref")
TU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("log2n", "u1"), ("plane", "u1"), ("mode", "u1"), ("flags", "u1")])
SAO_DTYPE = np.dtype([("type", "i1"), ("band", "u1"), ("offset", "i1", 4)])
CU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("log2size", "u1"), ("intra", "u1"), ("skipped", "u1"), ("pad", "u1")])
PU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("cu_x", "<u2"), ("cu_y", "<u2"), ("w", "u1"), ("h", "u1"), ("poc0", "<i2"), ("poc1", "<i2"),
                     ("mv0x", "<i2"), ("mv0y", "<i2"), ("mv1x", "<i2"), ("mv1y", "<i2")])


def synthetic_clip(seed, w, h, n, B, smooth=False, motion=False):
    """Pictures with flat areas, ramps, sharp rectangles, fine noise and text-like 1-sample detail, so that the
    encoder's search picks every block size, many directions and transform skip."""
    rng = np.random.default_rng(seed)
    mx = (1 << B) - 1
    out = []
    if motion:
        # one larger canvas seen through a window that pans 4 x 2 luma samples per picture, an object that moves
        # against the pan, fresh noise every picture and a new rectangle in every picture (uncovered content: the
        # encoder codes it intra inside inter pictures)
        canvas = synthetic_clip(seed + 1000, w + 64, h + 64, 1, B)[0]
        for i in range(n):
            planes = []
            for k, c in enumerate(canvas):
                s = 1 if k else 0
                ox, oy = (8 + 4 * i) >> s, (8 + 2 * i) >> s
                p = c[oy:oy + (h >> s), ox:ox + (w >> s)].astype(np.float64)
                bx, by = (100 - 6 * i) >> s, (40 + 4 * i) >> s
                p[by:by + (24 >> s), bx:bx + (32 >> s)] = (0.8 if k == 0 else 0.3) * mx
                nx, ny = int(rng.integers(0, (w >> s) - 24)), int(rng.integers(0, (h >> s) - 24))
                p[ny:ny + (20 >> s), nx:nx + (20 >> s)] = rng.integers(0, mx + 1, ((20 >> s), (20 >> s)))
                p += rng.normal(0, 0.004 * mx, p.shape)
                planes.append(np.clip(np.rint(p), 0, mx).astype(np.uint16))
            out.append(planes)
        return out
    for i in range(n):
        planes = []
        for (pw, ph) in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = 0.5 * mx * (1 + 0.5 * np.sin(xx / 19.0 + seed + i) * np.cos(yy / 13.0))
            p[:, : pw // 3] = 0.3 * mx + 0.4 * mx * xx[:, : pw // 3] / pw                   # ramp
            for _ in range(3 if smooth else 12):                                            # sharp rectangles
                x0, y0 = int(rng.integers(0, pw - 8)), int(rng.integers(0, ph - 8))
                p[y0:y0 + int(rng.integers(3, 24)), x0:x0 + int(rng.integers(3, 40))] = rng.integers(0, mx + 1)
            noisy = ((xx // 16 + yy // 16) % 3 == 0) & ((not smooth) | (xx > 0.7 * pw))
            p = np.where(noisy, p + rng.normal(0, 0.08 * mx, (ph, pw)), p + rng.normal(0, 0.004 * mx, (ph, pw)))
            p[ph // 2: ph // 2 + 12, ::2] = mx * (rng.random((12, (pw + 1) // 2)) < 0.5)   # 1-sample detail
            planes.append(np.clip(np.rint(p), 0, mx).astype(np.uint16))
        out.append(planes)
    return out


def fading_clip(seed, w, h, n, B):
    """synthetic_clip's panning clip under a fade: picture i has its contrast about mid-grey scaled by a gain and its brightness moved
    by a step, luma and chroma each their own, so that an encoder with weighted prediction on codes non-default weights and offsets.
    The slopes keep the reference encoder's estimates inside the coded range: it does not clip its luma offset to -128..127
    (WeightPredAnalysis.cpp:228-232), and a steeper fade over four pictures made it write -129 and -136."""
    mx = (1 << B) - 1
    mid, unit = (mx + 1) / 2, 1 << (B - 8)
    out = []
    for i, planes in enumerate(synthetic_clip(seed, w, h, n, B, False, True)):
        fade = []
        for k, p in enumerate(planes):
            gain, step = (1.0 - 0.08 * i, 5 * i * unit) if k == 0 else (1.0 - 0.06 * i, (-4 if k == 1 else 3) * i * unit)
            fade.append(np.clip(np.rint((p.astype(np.float64) - mid) * gain + mid + step), 0, mx).astype(np.uint16))
        out.append(fade)
    return out


def parse_hmxd(path):
    b = open(path, "rb").read()
    assert b[:4] == b"HMXD"
    ver, n = np.frombuffer(b, "<i4", 2, 4)
    assert ver in (4, 5)  # 5 adds the weighted-prediction records behind every picture
    off, pics = 12, []
    for _ in range(n):
        poc, w, h, B, qp, ctu, slice_type, n_tu, n_pu, n_cu = (int(v) for v in np.frombuffer(b, "<i4", 10, off))
        off += 40
        tus = np.frombuffer(b, TU_DTYPE, n_tu, off).copy()
        off += 8 * n_tu
        pus = np.frombuffer(b, PU_DTYPE, n_pu, off).copy()
        off += PU_DTYPE.itemsize * n_pu
        cus = np.frombuffer(b, CU_DTYPE, n_cu, off).copy()
        off += 8 * n_cu
        n_ctu = -(-w // ctu) * -(-h // ctu)
        lev = []
        for p in range(3):
            e = n_ctu * ctu * ctu >> (2 if p else 0)
            lev.append(np.frombuffer(b, "<i4", e, off).copy())
            off += 4 * e
        sao = np.frombuffer(b, SAO_DTYPE, 3 * n_ctu, off).reshape(3, n_ctu).copy()
        off += 6 * 3 * n_ctu
        dbk = np.frombuffer(b, "<i4", 3, off).copy()  # disabled, beta_offset_div2, tc_offset_div2
        off += 12
        rec = []
        for p in range(3):
            pw, ph = w >> (1 if p else 0), h >> (1 if p else 0)
            rec.append(np.frombuffer(b, "<i2", pw * ph, off).reshape(ph, pw).copy())
            off += 2 * pw * ph
        # explicit weighted prediction: PPS flags, entries per list, per entry its POC and the rows [component][weight, offset, log2 denominator],
        # the two reference indices of every prediction unit
        wp = dict(flags=(0, 0), poc=[], tab=[], ridx=None)
        if ver >= 5:
            use_wp, wp_bipred, n0, n1 = (int(v) for v in np.frombuffer(b, "<i4", 4, off))
            off += 16
            wp_poc, wp_tab = [], []
            for cnt in (n0, n1):
                a = np.frombuffer(b, "<i4", 10 * cnt, off).reshape(cnt, 10)
                off += 40 * cnt
                wp_poc.append(a[:, 0].astype(np.int16))
                wp_tab.append(a[:, 1:].reshape(cnt, 3, 3).astype(np.int16))
            ridx = np.frombuffer(b, "i1", 2 * n_pu, off).reshape(n_pu, 2).copy()
            off += 2 * n_pu
            wp = dict(flags=(use_wp, wp_bipred), poc=wp_poc, tab=wp_tab, ridx=ridx)
        pics.append(dict(wp=wp, poc=poc, w=w, h=h, B=B, qp=qp, ctu=ctu, tus=tus, pus=pus, cus=cus, slice_type=slice_type, lev=lev, rec=rec, sao=sao, dbk=dbk))
    assert off == len(b)
    return pics


def weighted(p):
    """the slice is predicted with explicit weights (TComSlice::applyWP): P with the PPS's use-WP flag, B with its WP bi-pred flag"""
    return bool((p["slice_type"] == 1 and p["wp"]["flags"][0]) or (p["slice_type"] == 0 and p["wp"]["flags"][1]))


def check_weighted(pics):
    """What a weighted fixture must hold, on what the tap recorded: a P slice and a B slice with a luma row and a chroma row that
    are not the default, a bi-predicted unit on two rows that differ, a uni-predicted unit of a B slice on list 1; every row inside
    the coded ranges.  Returns the counts."""
    cnt = dict(rows_P=[0, 0], rows_B=[0, 0], bi_rows_differ=0, uni_list1_in_B=0)
    for p in pics:
        if not weighted(p):
            continue
        tab, ridx = p["wp"]["tab"], p["wp"]["ridx"]
        for t in tab:
            assert ((t[:, :, 0] >= -128) & (t[:, :, 0] <= 255) & (t[:, :, 1] >= -128) & (t[:, :, 1] <= 127) & (t[:, :, 2] >= 0) & (t[:, :, 2] <= 7)).all(), t
        used = {(l, int(r[l])) for r in ridx for l in (0, 1) if r[l] >= 0}
        for l, i in used:
            off_default = (tab[l][i][:, 0] != (1 << tab[l][i][:, 2])) | (tab[l][i][:, 1] != 0)
            key = "rows_P" if p["slice_type"] == 1 else "rows_B"
            cnt[key][0] += int(off_default[0])
            cnt[key][1] += int(off_default[1:].any())
        if p["slice_type"] == 0:
            for r in ridx:
                if r[0] >= 0 and r[1] >= 0:
                    cnt["bi_rows_differ"] += int(not np.array_equal(tab[0][r[0]], tab[1][r[1]]))
                elif r[1] >= 0:
                    cnt["uni_list1_in_B"] += int(((tab[1][r[1]][:, 0] != (1 << tab[1][r[1]][:, 2])) | (tab[1][r[1]][:, 1] != 0)).any())
    return cnt


def make(name, seed, w, h, n, B, qp, cfg, extra=(), smooth=False, motion=False, keep_org=False, out_dir=HERE, fade=False, need=("P",)):
    enc, tap = os.path.join(REFBIN, "TAppEncoder"), os.path.join(REFBIN, "hm_decision_tap")
    if not (os.path.exists(enc) and os.path.exists(tap)):
        subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref_apps.sh")])
    with tempfile.TemporaryDirectory() as d:
        yuv, bit, out = (os.path.join(d, f) for f in ("in.yuv", "str.bin", "out.hmxd"))
        clip = fading_clip(seed, w, h, n, B) if fade else synthetic_clip(seed, w, h, n, B, smooth, motion)
        with open(yuv, "wb") as f:
            for planes in clip:
                for p in planes:
                    f.write(p.astype(np.uint8 if B == 8 else "<u2").tobytes())
        cmd = [enc, "-c", os.path.join("/root/reference/cfg", cfg), "-i", yuv, "-wdt", str(w), "-hgt", str(h), "-fr", "30",
               "-f", str(n), "-q", str(qp), "-b", bit, "-o", os.path.join(d, "rec.yuv"), "--SEIpictureDigest=1", f"--InputBitDepth={B}",
               f"--InternalBitDepth={B}"] + list(extra)
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
        subprocess.run([tap, bit, out], check=True, stdout=subprocess.DEVNULL)
        pics = parse_hmxd(out)
        nbytes = os.path.getsize(bit)
    arrays = {"n": np.int32(len(pics)), "stream_bytes": np.int32(nbytes), "command": np.array(" ".join(c for c in cmd[1:] if not c.startswith(d)))}  # without the temporary paths
    for i, p in enumerate(pics):
        arrays[f"hdr{i}"] = np.array([p["poc"], p["w"], p["h"], p["B"], p["qp"], p["ctu"], p["slice_type"]], np.int32)
        arrays[f"pus{i}"] = p["pus"]
        arrays[f"cus{i}"] = p["cus"]
        if keep_org:  # the encoder's input picture (all-intra: coding order = input order)
            for k in range(3):
                arrays[f"org{i}_{k}"] = clip[p["poc"]][k].astype(np.int16)
        if weighted(p):  # the slice's tables: per list the POC of every entry and its rows [entry][component][weight, offset, log2 denominator]; ridx: the units' reference indices
            arrays[f"wpflags{i}"] = np.array(p["wp"]["flags"], np.int32)
            for l in (0, 1):
                arrays[f"wppoc{i}_{l}"], arrays[f"wptab{i}_{l}"] = p["wp"]["poc"][l], p["wp"]["tab"][l]
            arrays[f"ridx{i}"] = p["wp"]["ridx"]
        arrays[f"tus{i}"] = p["tus"]
        arrays[f"sao{i}"] = p["sao"]
        arrays[f"dbk{i}"] = p["dbk"]
        for k in range(3):
            arrays[f"lev{i}_{k}"] = p["lev"][k]
            arrays[f"rec{i}_{k}"] = p["rec"][k]
    if fade:
        cnt = check_weighted(pics)
        assert "P" not in need or min(cnt["rows_P"]) > 0, cnt
        assert "B" not in need or (min(cnt["rows_B"]) > 0 and cnt["bi_rows_differ"] > 0 and cnt["uni_list1_in_B"] > 0), cnt
        print(f"stream_{name}: non-default (luma, chroma) rows in use, P slices {cnt['rows_P']}, B slices {cnt['rows_B']}; bi units on two differing rows "
              f"{cnt['bi_rows_differ']}; list-1 uni units of B slices on a non-default row {cnt['uni_list1_in_B']}")
    path = os.path.join(out_dir, f"stream_{name}.npz")
    np.savez_compressed(path, **arrays)
    sizes = np.bincount(np.concatenate([p["tus"]["log2n"][p["tus"]["plane"] == 0] for p in pics]), minlength=6)[2:]
    ts = sum(int((p["tus"]["flags"] & 1).sum()) for p in pics)
    sao_on = sum(int((p["sao"]["type"] >= 0).sum()) for p in pics)
    n_pu = sum(len(p["pus"]) for p in pics)
    n_bi = sum(int(((p["pus"]["poc0"] > -32768) & (p["pus"]["poc1"] > -32768)).sum()) for p in pics)
    intra_in_inter = sum(int(((p["tus"]["flags"] & 2) == 0).sum()) for p in pics if p["slice_type"] != 2)
    print(f"{path}: {len(pics)} picture(s), {nbytes} stream bytes, luma blocks 4/8/16/32 = {sizes.tolist()}, transform-skip blocks {ts}, SAO CTU-components on {sao_on}, PUs {n_pu} ({n_bi} bi), intra blocks in inter pictures {intra_in_inter}, "
          f"{os.path.getsize(path)} bytes")


# loop filters off (the slice-level disable is only signalled with the control-present flag)
PURE = ["--DeblockingFilterControlPresent=1", "--LoopFilterDisable=1", "--SAO=0"]

if __name__ == "__main__":
    only = sys.argv[1:]
    if only:
        _make = make
        make = lambda name, *a, **k: _make(name, *a, **k) if name in only else None  # noqa: E731
    # pure reconstruction: loop filters off, so the decoder's output IS prediction + residual of the block path
    make("intra_main_q27", 11, 192, 128, 2, 8, 27, "encoder_intra_main.cfg", PURE)
    make("intra_he10_q32", 12, 128, 128, 1, 10, 32, "encoder_intra_he10.cfg", PURE)
    # deblocking as the configuration ships it (all-intra: every filtered edge has strength 2), SAO off: the decoder's
    # output is the block path followed by the deblocking filter
    make("intra_main_q34_dbk", 13, 192, 128, 1, 8, 34, "encoder_intra_main.cfg", ["--SAO=0"])
    # 416x240: 6.5 x 3.75 CTUs (coding units cut by the picture boundary), smoother content for 32x32 blocks, deblocked
    make("intra_main_q37_416x240_dbk", 14, 416, 240, 1, 8, 37, "encoder_intra_main.cfg", ["--SAO=0"], smooth=True)
    # the shipped configurations as they are: deblocking and SAO on (the decoder's output = block path, deblocking, SAO)
    make("intra_main_q32_full", 15, 256, 192, 2, 8, 32, "encoder_intra_main.cfg")
    make("intra_he10_q30_416x240_full", 16, 416, 240, 1, 10, 30, "encoder_intra_he10.cfg")
    # encoder direction: with the flat quantiser (RDOQ off; sign-bit hiding stays on) the levels in the stream are a
    # function of the decisions and the input picture alone, so the encoder-side chain can be held against them
    make("intra_main_q29_rdoq0", 22, 192, 128, 2, 8, 29, "encoder_intra_main.cfg", PURE + ["--RDOQ=0"], keep_org=True)
    make("intra_he10_q35_rdoq0", 23, 128, 128, 1, 10, 35, "encoder_intra_he10.cfg", PURE + ["--RDOQ=0"], keep_org=True)
    # the same for inter residuals (rounding offset of inter slices): wherever the encoder kept a transform block's
    # residual, its levels are the flat quantiser's of (input - prediction)
    make("lowdelay_P_main_q28_rdoq0", 24, 192, 128, 3, 8, 28, "encoder_lowdelay_P_main.cfg", PURE + ["--RDOQ=0"], motion=True, keep_org=True)
    # inter pictures (low delay P, random access), loop filters off: motion compensation + inter residual + the intra
    # blocks the encoder chose inside inter pictures
    make("lowdelay_P_main_q30", 17, 192, 128, 4, 8, 30, "encoder_lowdelay_P_main.cfg", PURE, motion=True)
    make("randomaccess_main_q32", 18, 192, 128, 9, 8, 32, "encoder_randomaccess_main.cfg", PURE, motion=True)
    # the same two structures with the loop filters of the shipped configurations (boundary strengths from motion)
    make("lowdelay_P_main_q32_full", 19, 192, 128, 4, 8, 32, "encoder_lowdelay_P_main.cfg", motion=True)
    make("randomaccess_main_q34_full", 20, 256, 192, 9, 8, 34, "encoder_randomaccess_main.cfg", motion=True)
    # 10-bit low-delay B, 416x240 (coding units cut by the picture boundary, vectors that leave the picture), filters on
    make("lowdelay_he10_q33_416x240_full", 21, 416, 240, 3, 10, 33, "encoder_lowdelay_he10.cfg", motion=True)
    # explicit weighted prediction on a fading clip: P slices (loop filters off), B slices with both flags (filters as shipped)
    make("lowdelay_P_wp_q30", 25, 192, 128, 4, 8, 30, "encoder_lowdelay_P_main.cfg", PURE + ["-wpP", "1"], fade=True, need=("P",))
    make("randomaccess_wp_q32", 26, 192, 128, 5, 8, 32, "encoder_randomaccess_main.cfg", ["-wpP", "1", "-wpB", "1"], fade=True, need=("B",))
