"""The yardstick for a QP per block (hmx_set_qp_map): a picture whose transform blocks take the QP of the 4x4 luma unit at their first
sample (TComDataCU::getQP of the coding unit, applied through TComTrQuant::setQPforQuant; a chroma block at (x, y) reads the unit at
luma (2x, 2y)) is the CPU oracle called once per maximal run of blocks in coding order that share a QP, with cfg.qp = that run's QP:
hmo_intra_frame_encode / _decode work on the reconstruction in place and in list order, so the runs chain exactly as one call would.

encode() / decode() are that construction; encode_blockwise() / decode_blockwise() are a second one, block by block through
hmo_predIntra*, hmo_transformNxN / hmo_invtransformNxN and hmo_setQPforQuant, which tests/test_qp_map_oracle.py holds against the
first.  inter_block() is the per-block form for blocks of inter coding units (prediction given, no neighbours)."""
import ctypes as C

import numpy as np

import oracle_lib as ol

TU_TRANSFORM_SKIP, TU_INTER = 1, 2
REG_DCT = 65535


def unit_dims(w, h):
    return -(-h // 4), -(-w // 4)


def block_qp(t, qp_map):
    """The QP of one block: the map's unit at the block's first sample, in luma coordinates."""
    c = 1 if int(t["plane"]) else 0
    return int(qp_map[(int(t["y"]) << c) >> 2, (int(t["x"]) << c) >> 2])


def block_qps(tus, qp_map):
    return np.array([block_qp(t, qp_map) for t in tus], np.int32)


def runs(tus, qp_map):
    """[(first, end, qp)]: the maximal runs of blocks in list order that share a QP."""
    q = block_qps(tus, qp_map)
    out, a = [], 0
    for i in range(1, len(q) + 1):
        if i == len(q) or q[i] != q[a]:
            out.append((a, i, int(q[a])))
            a = i
    return out


def _p3(planes):
    return (C.c_void_p * 3)(*[p.ctypes.data for p in planes])


def encode(tus, w, h, B, org, qp_map, sign_hide=1, chroma_qp_offset=0, ctu=64, inter_slice=0):
    """-> (reconstruction planes, level planes in plane geometry)"""
    t = np.ascontiguousarray(tus, ol.TU_DTYPE)
    rec = [np.zeros_like(p) for p in org]
    lev = [np.zeros(p.shape, np.int32) for p in org]
    st = (C.c_int * 3)(w, w // 2, w // 2)
    for a, b, qp in runs(t, qp_map):
        cfg = ol.frame_cfg(w, h, B, qp, sign_hide, chroma_qp_offset, ctu, inter_slice)
        ol.oracle().hmo_intra_frame_encode(C.byref(cfg), t[a:b].ctypes.data, b - a, _p3(org), st, _p3(rec), st, _p3(lev))
    return rec, lev


def decode(tus, w, h, B, lev, qp_map, sign_hide=1, chroma_qp_offset=0, ctu=64, inter_slice=0):
    t = np.ascontiguousarray(tus, ol.TU_DTYPE)
    lev = [np.ascontiguousarray(p, np.int32) for p in lev]
    rec = [np.zeros(p.shape, np.int16) for p in lev]
    st = (C.c_int * 3)(w, w // 2, w // 2)
    for a, b, qp in runs(t, qp_map):
        cfg = ol.frame_cfg(w, h, B, qp, sign_hide, chroma_qp_offset, ctu, inter_slice)
        ol.oracle().hmo_intra_frame_decode(C.byref(cfg), t[a:b].ctypes.data, b - a, _p3(rec), st, _p3(lev))
    return rec


def _quant(t, qp, B, chroma_qp_offset, sign_hide, intra_slice, is_intra, base_qp=None):
    """(hmo_qp, quantiser settings) of one block under luma QP qp.  base_qp: the slice's base QP, from which the reference encoder's
    xQuant takes its right shift (TComTrQuant.cpp:1161-1231, ADAPTIVE_QP_SELECTION; chroma: the base through the chroma table
    without the PPS offset); None: the shift follows the block's QP, as in the oracle's frame drivers."""
    chroma, N = 1 if int(t["plane"]) else 0, 1 << int(t["log2n"])
    q = ol.oracle().hmo_setQPforQuant(qp, chroma, 6 * (B - 8), chroma_qp_offset if chroma else 0)
    scan = ol.oracle().hmo_coef_scan_idx(N, 0 if chroma else 1, 1 if is_intra else 0, int(t["mode"]))
    per_qbits = None if base_qp is None else ol.oracle().hmo_setQPforQuant(base_qp, chroma, 6 * (B - 8), 0).per
    return q, ol.quant_cfg(q.per, q.rem, intra_slice, sign_hide, scan, per_qbits)


def encode_blockwise(tus, w, h, B, org, qp_map, sign_hide=1, chroma_qp_offset=0, ctu=64, inter_slice=0, base_qp=None):
    rec = [np.zeros_like(p) for p in org]
    lev = [np.zeros(p.shape, np.int32) for p in org]
    for t in tus:
        p, N, x, y, ts = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["flags"]) & TU_TRANSFORM_SKIP
        q, qc = _quant(t, block_qp(t, qp_map), B, chroma_qp_offset, sign_hide, 0 if inter_slice else 1, True, base_qp)
        pw = w >> (1 if p else 0)
        pred = ol.o_intra_pred(rec[p].reshape(-1), pw, x, y, N, int(t["mode"]), B, w, h, p != 0, ctu)
        resi = (org[p][y:y + N, x:x + N].astype(np.int32) - pred).astype(np.int16)
        mode = REG_DCT if p else int(t["mode"])
        lv, abs_sum = ol.o_transformNxN(resi, N, B, mode, ts, qc)
        r = ol.o_invtransformNxN(lv, N, B, mode, q.per, q.rem, ts) if abs_sum else np.zeros((N, N), np.int16)
        rec[p][y:y + N, x:x + N] = np.clip(pred.astype(np.int32) + r, 0, (1 << B) - 1)
        lev[p][y:y + N, x:x + N] = lv
    return rec, lev


def decode_blockwise(tus, w, h, B, lev, qp_map, sign_hide=1, chroma_qp_offset=0, ctu=64):
    rec = [np.zeros(p.shape, np.int16) for p in lev]
    for t in tus:
        p, N, x, y, ts = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["flags"]) & TU_TRANSFORM_SKIP
        q, _ = _quant(t, block_qp(t, qp_map), B, chroma_qp_offset, sign_hide, 1, True)
        pw = w >> (1 if p else 0)
        pred = ol.o_intra_pred(rec[p].reshape(-1), pw, x, y, N, int(t["mode"]), B, w, h, p != 0, ctu)
        r = ol.o_invtransformNxN(lev[p][y:y + N, x:x + N], N, B, REG_DCT if p else int(t["mode"]), q.per, q.rem, ts)
        rec[p][y:y + N, x:x + N] = np.clip(pred.astype(np.int32) + r, 0, (1 << B) - 1)
    return rec


def inter_block(t, qp, B, org_blk, pred_blk, sign_hide=1, chroma_qp_offset=0, intra_slice=0):
    """A block of an inter coding unit under luma QP qp: (levels, uiAbsSum, reconstruction, xGetSSE(org, rec)).  The reconstruction
    is the one hmx_batch_residual_transform_recon makes: the inverse of the levels whatever uiAbsSum (all-zero levels give zero)."""
    N, ts = 1 << int(t["log2n"]), int(t["flags"]) & TU_TRANSFORM_SKIP
    q, qc = _quant(t, qp, B, chroma_qp_offset, sign_hide, intra_slice, False)
    resi = (org_blk.astype(np.int32) - pred_blk).astype(np.int16)
    lv, abs_sum = ol.o_transformNxN(resi, N, B, REG_DCT, ts, qc)
    r = ol.o_invtransformNxN(lv, N, B, REG_DCT, q.per, q.rem, ts)
    rec = np.clip(pred_blk.astype(np.int32) + r, 0, (1 << B) - 1).astype(np.int16)
    O = ol.oracle()
    O.hmo_getSSE.restype = C.c_uint32
    o, rr = np.ascontiguousarray(org_blk, np.int16), np.ascontiguousarray(rec)
    sse = O.hmo_getSSE(o.ctypes.data_as(C.c_void_p), N, rr.ctypes.data_as(C.c_void_p), N, N, N, B)
    return lv, abs_sum, rec, int(sse)


def block_sse(t, B, org, rec):
    """xGetSSE(org, rec) of one block of two pictures (three planes each)"""
    O = ol.oracle()
    O.hmo_getSSE.restype = C.c_uint32
    p, N, x, y = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"])
    o, r = np.ascontiguousarray(org[p][y:y + N, x:x + N]), np.ascontiguousarray(rec[p][y:y + N, x:x + N])
    return int(O.hmo_getSSE(o.ctypes.data_as(C.c_void_p), N, r.ctypes.data_as(C.c_void_p), N, N, N, B))


# ---- the pictures the tests share ----
def all_sizes_tus(seed, ts_prob=0.3):
    """A 128 x 64 picture, two CTUs of 64, in coding order, with every transform size that exists: 4..32 in luma and 4..16 in chroma
    (4:2:0 with 32x32 as the largest transform: a 32x32 chroma block would belong to a 64x64 transform unit), some 4x4 blocks with
    transform skip.  CTU 0: one 64x64 CU of 32x32 luma and 16x16 chroma blocks.  CTU 1: a 32x32 CU of 16x16 blocks (8x8 chroma), a
    32x32 CU of 8x8 blocks (4x4 chroma), four 16x16 CUs of 8x8 or 4x4 blocks, and sixteen 8x8 CUs of 4x4 luma blocks with one 4x4
    block per chroma plane."""
    from thevc_amd import workload
    rng = np.random.default_rng(seed)
    o = []
    workload._cu_blocks(0, 0, 64, 32, o)
    workload._cu_blocks(64, 0, 32, 16, o)
    workload._cu_blocks(96, 0, 32, 8, o)
    for k, (dx, dy) in enumerate(((0, 0), (16, 0), (0, 16), (16, 16))):
        workload._cu_blocks(64 + dx, 32 + dy, 16, 8 if k % 2 else 4, o)
    for (j, i) in workload._zorder(4):
        workload._cu_blocks(96 + 8 * i, 32 + 8 * j, 8, 4, o)
    a = np.array(o, np.int32)
    tus = np.zeros(len(a), ol.TU_DTYPE)
    tus["x"], tus["y"], tus["log2n"], tus["plane"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    luma = tus["plane"] == 0
    modes = rng.integers(0, 35, len(a)).astype(np.uint8)
    cm = np.array(workload.CHROMA_MODES + (34,), np.uint8)[rng.integers(0, 5, len(a))]
    tus["mode"] = np.where(luma, modes, cm)
    ts = (tus["log2n"] == 2) & (rng.random(len(a)) < ts_prob)
    tus["flags"] = np.where(ts, TU_TRANSFORM_SKIP, 0).astype(np.uint8)
    return tus


def varied_map(seed, w, h, B, slice_qp, plant=()):
    """A map that varies per 8 x 8 luma area: values drawn from slice_qp +- 7 (so qp / 6 and qp % 6 both change between neighbours),
    clipped to the legal range -QpBDOffset .. 51; plant = QPs written over as many areas picked by the seed, one each (51,
    -QpBDOffset, the range where the chroma table is not linear, ...)."""
    rng = np.random.default_rng(seed)
    off = 6 * (B - 8)
    uh, uw = unit_dims(w, h)
    areas = np.clip(slice_qp + rng.integers(-7, 8, ((uh + 1) // 2, (uw + 1) // 2)), -off, 51)
    where = rng.permutation(areas.size)[:len(plant)]
    for k, v in zip(where, plant):
        areas.flat[k] = v
    return np.ascontiguousarray(np.repeat(np.repeat(areas, 2, 0), 2, 1)[:uh, :uw].astype(np.int8))


def load_aq_intra_stream(path):
    """tests/golden/aq_intra_stream.npz (make_aq_intra_stream.py) -> per clip (config dict, [picture dicts as thevc_amd.decisions has them,
    with qp_map and cu_depth])"""
    d, clips = np.load(path), []
    for c in range(int(d["n_clips"])):
        B, ctu, k, rng_, q, seed = (int(v) for v in d[f"c{c}_config"])
        pics = []
        for i in range(int(d[f"c{c}_n"])):
            poc, w, h, b, qp, cs, st = (int(v) for v in d[f"c{c}_hdr{i}"])
            pics.append(dict(poc=poc, w=w, h=h, B=b, qp=qp, ctu=cs, slice_type=st, tus=d[f"c{c}_tus{i}"], cus=d[f"c{c}_cus{i}"], pus=np.zeros(0),
                             lev=[d[f"c{c}_lev{i}_{j}"] for j in range(3)], rec=[d[f"c{c}_rec{i}_{j}"] for j in range(3)],
                             org=[d[f"c{c}_org{i}_{j}"] for j in range(3)], qp_map=d[f"c{c}_qp_map{i}"], cu_depth=d[f"c{c}_cu_depth{i}"]))
        clips.append((dict(B=B, ctu=ctu, k=k, range=rng_, q=q, seed=seed), pics))
    return clips
