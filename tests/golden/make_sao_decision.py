"""Fixtures that pin the SAO parameter search (tests/sao_decision_oracle.py, hmx_sao_decide_multi) on the reference ENCODER: a
synthetic clip is encoded by oracle/_ref/TAppEncoder under a shipped configuration with SAO on (make_stream_golden.make), the
stream goes through oracle/_ref/hm_decision_tap, and for every picture the deblocked, pre-SAO reconstruction is rebuilt on the
CPU with the decode loop of tests/test_stream_golden.py (the picture in hand decoded with its SAO table set to off).  The
generator asserts that hmo_sao_picture of that reconstruction with the tap's table gives the tap's final picture, so the stored
pair (input picture, pre-SAO picture) is what TEncSampleAdaptiveOffset::SAOProcess saw, and the tap's table is what it decided.

One input of the search is not visible from outside the encoder: the fractional bits its rate coder holds when startSaoEnc runs.
The reference never clears them (TEncBinCABAC::start, TEncBinCoderCABAC.cpp:69-76, leaves m_fracBits alone; resetBits, :193, keeps
the low 15 bits), so they are what the picture's last rate estimate left behind.  The generator scans the 32768 values coarse to
fine with the oracle and stores the first one under which the oracle's table IS the encoder's (frac{i}); a picture for which no
scanned value does that fails the generator.  With 0 in its place a few CTUs per picture sit on the other side of a cost tie.
The same holds for the context table of an inter picture: resetEntropy initialises from the table the PPS's encCABACTableIdx names
(TEncSbac.cpp:117-121), which determineCabacInitIdx chose after the previous picture (TEncSlice.cpp:1392-1394) and which is B or
P whatever the slice's own type; both are tried and the one that reproduces the encoder is stored as the last entry of hdr{i}.

Stored per picture i: hdr{i} = [poc, w, h, B, slice qp, ctu, slice type, hierarchy depth, context table] in coding order, lambda{i} = the two
lambdas, frac{i}, org{i}_{k} the input planes, dpre{i}_{k} = pre-SAO - input, drec{i}_{k} = final - pre-SAO (small differences pack
well), sao{i} the tap's table.  Needs /root/reference; the .npz travels.

  python tests/golden/make_sao_decision.py            # writes tests/golden/saodec_*.npz and prints the coverage counts
"""
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

# g_aucChromaScale, TLibCommon/TComRom.cpp:380-386 (the table of CHROMA_QP_EXTENSION, which the fork sets)
CHROMA_SCALE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 29, 30, 31, 32,
                33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51]
# the coding structures of the shipped configurations (cfg/encoder_*.cfg: GOPSize, HadamardME, Frame<k>: POC -> QPfactor)
STRUCTURES = {
    "encoder_intra_main.cfg": dict(gop=1, hadamard=1, factor={1: 1.0}),
    "encoder_intra_he10.cfg": dict(gop=1, hadamard=1, factor={1: 1.0}),
    "encoder_lowdelay_P_main.cfg": dict(gop=4, hadamard=1, factor={1: 0.4624, 2: 0.4624, 3: 0.4624, 4: 0.578}),
    "encoder_randomaccess_main.cfg": dict(gop=8, hadamard=1, factor={8: 0.442, 4: 0.3536, 2: 0.3536, 1: 0.68, 3: 0.68, 6: 0.3536, 5: 0.68, 7: 0.68}),
}


def depth_of(poc, gop):
    """TEncSlice::initEncSlice, TEncSlice.cpp:179-206"""
    p = poc % gop
    if p == 0:
        return 0
    step, depth, i = gop, 0, gop >> 1
    while i >= 1:
        found = False
        for j in range(i, gop, step):
            if j == p:
                found = True
                break
        step >>= 1
        depth += 1
        if found:
            break
        i >>= 1
    return depth


def lambdas(cfg, poc, qp, is_intra):
    """TEncSlice.cpp:264-342 for DeltaQpRD = 0; qp = the slice QP (dQP is an integer under the shipped configurations)"""
    s = STRUCTURES[cfg]
    number_b_frames = s["gop"] - 1                                            # :266
    lambda_scale = 1.0 - min(0.5, max(0.0, 0.05 * float(number_b_frames)))    # :268
    qp_temp = float(qp) + 0 - 12                                              # :272-274 (FULL_NBIT 0, SHIFT_QP 12)
    factor = s["factor"][(poc - 1) % s["gop"] + 1] if poc else 1.0            # :279 dQPFactor of the GOP entry
    if is_intra:
        factor = 0.57 * lambda_scale                                          # :280-283
    lam = factor * pow(2.0, qp_temp / 3.0)                                    # :284
    depth = depth_of(poc, s["gop"])
    if depth > 0:
        lam *= min(4.0, max(2.0, qp_temp / 6.0))                              # :286-293 the depth clip
    if not s["hadamard"]:
        lam *= 0.95                                                           # :296-299
    # :313-316 LambdaModifier is 1.0 under the shipped configurations
    weight = 1.0
    if qp >= 0:
        weight = pow(2.0, (qp - CHROMA_SCALE[qp]) / 3.0)                      # :326
    return lam, lam / weight, depth                                           # :340 setLambda(dLambda, dLambda / weight)


def pre_sao_pictures(pics):
    """the deblocked picture of every picture of the stream: the sequence decoded up to it, the last picture's SAO table off"""
    from test_stream_golden import oracle_decode_sequence
    out = []
    for i, p in enumerate(pics):
        q = dict(p)
        q["sao"] = p["sao"].copy()
        q["sao"]["type"] = -1
        out.append(oracle_decode_sequence(pics[:i] + [q])[-1])
    return out


def sao_picture(pre, p):
    import oracle_lib as ol
    O = ol.oracle()
    P3, I3 = C.c_void_p * 3, C.c_int * 3
    w, h = p["w"], p["h"]
    src = [np.ascontiguousarray(a, np.int16) for a in pre]
    flt = [np.zeros_like(a) for a in src]
    prm = np.ascontiguousarray(p["sao"])
    O.hmo_sao_picture(P3(*[a.ctypes.data for a in src]), P3(*[a.ctypes.data for a in flt]), I3(w, w // 2, w // 2), w, h, p["B"], p["ctu"],
                      P3(prm[0].ctypes.data, prm[1].ctypes.data, prm[2].ctypes.data))
    return flt


def make(name, seed, w, h, n, B, qp, cfg, ctu, out_dir=HERE, **kw):
    import make_stream_golden as msg
    from thevc_amd.decisions import has_sao, load_pictures
    depth = {32: 3, 16: 2}[ctu]
    extra = [f"--MaxCUWidth={ctu}", f"--MaxCUHeight={ctu}", f"--MaxPartitionDepth={depth}", f"--QuadtreeTULog2MaxSize={min(5, ctu.bit_length() - 1)}"]
    with tempfile.TemporaryDirectory() as d:
        msg.make("tmp", seed, w, h, n, B, qp, cfg, extra, keep_org=True, out_dir=d, **kw)
        pics = list(load_pictures(os.path.join(d, "stream_tmp.npz")))
    pre = pre_sao_pictures(pics)
    arrays = {"n": np.int32(len(pics)), "cfg": np.array(cfg)}
    import sao_decision_oracle as sd
    state = sd.RateState()
    for i, p in enumerate(pics):
        assert p["ctu"] == ctu and p["B"] == B
        flt = sao_picture(pre[i], p) if has_sao(p) else pre[i]
        for k in range(3):
            assert np.array_equal(flt[k], p["rec"][k]), (name, p["poc"], k, "SAO of the rebuilt pre-SAO picture is not the reference decoder's output")
        lam, lam_c, dep = lambdas(cfg, p["poc"], p["qp"], p["slice_type"] == 2)
        arrays[f"lambda{i}"] = np.array([lam, lam_c], np.float64)
        tried, found = set(), None
        tables = [2] if p["slice_type"] == 2 else [p["slice_type"], 1 - p["slice_type"]]
        for step in (2048, 256, 32, 4):  # coarse to fine: the values that reproduce the encoder form intervals
            for f0 in range(0, 32768, step):
                for table in tables:
                    if (f0, table) not in tried and found is None:
                        tried.add((f0, table))
                        res, ok = decide_picture(dict(p, depth=dep, lambdas=(lam, lam_c), pre=pre[i], table=table), state, f0)
                        if ok:
                            found = (f0, res, table)
        assert found, (name, p["poc"], "no starting fraction and table among", len(tried), "reproduces the encoder's table")
        arrays[f"frac{i}"] = np.int32(found[0])
        arrays[f"hdr{i}"] = np.array([p["poc"], p["w"], p["h"], B, p["qp"], ctu, p["slice_type"], dep, found[2]], np.int32)
        state.update(dep, found[1]["num_no_sao"], len(p["sao"][0]))
        arrays[f"sao{i}"] = p["sao"]
        for k in range(3):
            arrays[f"org{i}_{k}"] = np.asarray(p["org"][k], np.int16)
            arrays[f"dpre{i}_{k}"] = (np.asarray(pre[i][k], np.int16) - arrays[f"org{i}_{k}"]).astype(np.int16)
            arrays[f"drec{i}_{k}"] = (np.asarray(p["rec"][k], np.int16) - np.asarray(pre[i][k], np.int16)).astype(np.int16)
    path = os.path.join(out_dir, f"saodec_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(pics)} picture(s), {os.path.getsize(path)} bytes")
    return path


def load(path):
    """the pictures of a saodec_* fixture in coding order"""
    d = np.load(path)
    for i in range(int(d["n"])):
        poc, w, h, B, qp, ctu, slice_type, depth, table = (int(v) for v in d[f"hdr{i}"])
        org = [d[f"org{i}_{k}"] for k in range(3)]
        pre = [(org[k] + d[f"dpre{i}_{k}"]).astype(np.int16) for k in range(3)]
        rec = [(pre[k] + d[f"drec{i}_{k}"]).astype(np.int16) for k in range(3)]
        yield dict(poc=poc, w=w, h=h, B=B, qp=qp, ctu=ctu, slice_type=slice_type, depth=depth, lambdas=tuple(float(v) for v in d[f"lambda{i}"]),
                   frac=int(d[f"frac{i}"]), table=table,
                   org=org, pre=pre, rec=rec, sao=np.ascontiguousarray(d[f"sao{i}"]))


def expected_table(res, flags):
    """What the decoder sees of a decision: the slice's SAO flag is bSaoFlag[0] (TEncGOP.cpp:1083) and the chroma flag is only
    written behind it (TEncCavlc.cpp:691-700), so a picture whose luma is switched off carries no SAO at all."""
    t, band, off = (res["apply"][k].copy() for k in ("type", "band", "off"))
    if not flags[0]:
        t[:], band[:], off[:] = -1, 0, 0
    return t, band, off


_STATS = {}


def decide_picture(p, state, frac):
    """the oracle on one picture (p: org, pre, lambdas, depth, ...) under the rate state; (result, equals the tap's table)"""
    import sao_decision_oracle as sd
    from sao_stats_oracle import stats_vec
    cw, ch = -(-p["w"] // p["ctu"]), -(-p["h"] // p["ctu"])
    key = (id(p["pre"]), p["poc"])
    if key not in _STATS:
        _STATS.clear()
        _STATS[key] = stats_vec(p["org"], p["pre"], p["w"], p["h"], p["ctu"], p["B"], 1).tolist()
    flags = state.flags(p["depth"])
    res = sd.decide(_STATS[key], cw, ch, p["B"], p["lambdas"][0], p["lambdas"][1], flags, sd.ctx_init(p["table"], p["qp"]), None, frac)
    t, band, off = expected_table(res, flags)
    ok = np.array_equal(t, p["sao"]["type"]) and np.array_equal(off, p["sao"]["offset"]) and np.array_equal(band[t == 4], p["sao"]["band"][t == 4])
    return res, ok


def compare(path, counts=None):
    """Every picture of a fixture, in coding order with the rate state carried, against the tap's table.  Returns the mismatches."""
    import sao_decision_oracle as sd
    state, bad = sd.RateState(), []
    for p in load(path):
        cw, ch = -(-p["w"] // p["ctu"]), -(-p["h"] // p["ctu"])
        flags = state.flags(p["depth"])
        res, ok = decide_picture(p, state, p["frac"])
        state.update(p["depth"], res["num_no_sao"], cw * ch)
        t, band, off = expected_table(res, flags)
        if not ok:
            bad.append((os.path.basename(path), p["poc"], int((t != p["sao"]["type"]).sum()), int((off != p["sao"]["offset"]).any(-1).sum())))
        elif counts is not None:
            u = res["units"]
            for c, key in ((0, "luma"), (1, "chroma")):
                if flags[c] and flags[0]:
                    for v in u["type"][c]:
                        counts[key][int(v)] = counts[key].get(int(v), 0) + 1
            on = [c for c in range(3) if flags[1 if c else 0]]
            counts["merge_left"] += int(max(u["left"][c].sum() for c in on)) if on else 0
            counts["merge_up"] += int(max(u["up"][c].sum() for c in on)) if on else 0
            bo = u["off"][u["type"] == 4]
            counts["band_pos"] += int((bo > 0).sum())
            counts["band_neg"] += int((bo < 0).sum())
            counts["switched_off"] += int(not flags[0]) + int(not flags[1])
            counts["pictures"] += 1
    return bad


def new_counts():
    return dict(luma={}, chroma={}, merge_left=0, merge_up=0, band_pos=0, band_neg=0, switched_off=0, pictures=0)


CASES = [
    # name, seed, w, h, pictures, bit depth, QP, configuration, CTU size, clip options
    ("intra_main_q30", 31, 192, 128, 2, 8, 30, "encoder_intra_main.cfg", 32, {}),
    ("intra_main_q26_ctu16", 41, 192, 128, 1, 8, 26, "encoder_intra_main.cfg", 16, {}),
    ("intra_he10_q24", 46, 192, 128, 1, 10, 24, "encoder_intra_he10.cfg", 16, {}),
    ("lowdelay_P_main_q35", 33, 192, 128, 5, 8, 35, "encoder_lowdelay_P_main.cfg", 32, dict(motion=True)),
    ("randomaccess_main_q33", 34, 192, 128, 9, 8, 33, "encoder_randomaccess_main.cfg", 32, dict(motion=True)),
]

if __name__ == "__main__":
    only = sys.argv[1:]
    counts = new_counts()
    for name, seed, w, h, n, B, qp, cfg, ctu, kw in CASES:
        if only and name not in only:
            continue
        path = make(name, seed, w, h, n, B, qp, cfg, ctu, **kw)
        bad = compare(path, counts)
        assert not bad, bad
    print("coverage over the fixture set:", counts)
    if not only:
        for key in ("luma", "chroma"):
            assert all(counts[key].get(t, 0) > 0 for t in (-1, 0, 1, 2, 3, 4)), (key, counts[key])
        assert counts["merge_left"] > 0 and counts["merge_up"] > 0 and counts["band_pos"] > 0 and counts["band_neg"] > 0, counts
        if not counts["switched_off"]:
            print("no picture of these encodes has a component the rate state switched off: that case is left to the second-construction "
                  "and hand-case tests of tests/test_sao_decision_oracle.py")
