"""Decision lists of real streams -> pictures: the host-side driver that turns what a decoder has PARSED (the
reference's, via oracle/ref_decision_tap.cpp) into libhmx calls, picture by picture in decoding
order, with libhmx's own earlier outputs as reference pictures:

    inter coding units   hmx_batch_motionCompensation_multi (hmx_batch_motionCompensation_wp_multi for a slice under explicit
                         weighted prediction), hmx_batch_invtransformNxN_multi
    intra coding units   hmx_frame_intra_decode (intra pictures) / hmx_frame_intra_decode_onto (inside inter pictures)
    loop filters         hmx_deblock_strengths_multi (inter pictures; intra pictures have strength 2 on every edge),
                         hmx_deblock_picture_multi, hmx_sao_picture_multi (a decoder holds one picture at a time: batches of 1);
                         with slice / tile boundaries the filters may not cross, the edges on them are dropped and SAO is
                         hmx_sao_picture_multi_avail
    reference pictures   hmx_pic_extend_border

A picture is a dict: poc, w, h, B, qp, ctu, slice_type (0 B, 1 P, 2 I), tus (hmx_tu records; flags bit 1 = block of
an inter coding unit, bit 7 = luma coded-block flag), pus / cus (records of the tap), lev (three arrays in the
reference's per-CTU coefficient layout), sao ([3][n_ctu] hmx_sao_lcu records), dbk ([disabled, beta_offset_div2,
tc_offset_div2]), and the layout of its slices, tiles and constrained intra prediction: region (region id per CTU in
raster order, or None: one region) and cip (constrained_intra_pred_flag).  For the loop filters: slice_id / tile_id (slice
index in decoding order / tile index per CTU in raster order, or None: one slice / tile), lf_cross_slice (one
slice_loop_filter_across_slices_enabled_flag per slice) and lf_cross_tile (loop_filter_across_tiles_enabled_flag); from these
lf_border_avail() makes the byte per CTU that says which neighbour CTUs deblocking and SAO may read.  qp_map (optional): int8
[ceil(h / 4)][ceil(w / 4)], the luma QP of every 4x4 luma unit (TComDataCU::getQP; a stream with cu_qp_delta, adaptive QP) -- when
present, decode_sequence() sets it (hmx_set_qp_map) for the whole-picture and block-list calls of the picture, which then do not
quantise with qp, and deblock_maps() returns it as the deblocking QP map; when absent nothing changes.  wp: None, or the slice's
explicit weighted prediction: flags (the PPS's use WP, WP bi-pred), poc / tab (per list: the POC of every entry, its rows
[entry][component][weight, offset, log2 denominator]) and ridx (the two reference indices of every prediction unit).  load_pictures() reads
the .npz fixtures of tests/golden/make_stream_golden.py, make_stream_layout_golden.py and make_stream_lf_golden.py.  The
numpy helpers import nothing of the GPU side; decode_sequence() needs libhmx."""
import ctypes as C

import numpy as np

MARGIN = 80  # luma margin of reference pictures (TComPicYuv: g_uiMaxCUWidth + 16)
TU_INTER = 2
TU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("log2n", "u1"), ("plane", "u1"), ("mode", "u1"), ("flags", "u1")])
PU_DTYPE = np.dtype([("x", "<u2"), ("y", "<u2"), ("w", "u1"), ("h", "u1"), ("ref0", "u1"), ("ref1", "u1"), ("mv0x", "<i2"),
                     ("mv0y", "<i2"), ("mv1x", "<i2"), ("mv1y", "<i2")])  # hmx_pu


def _spread4(v):
    v = (v | (v << 2)) & 0x33
    return (v | (v << 1)) & 0x55


def z_offset(plane, x, y, w, ctu):
    """Offset of a block in the reference's coefficient layout: CTUs in raster order, 16 ints per 4x4 unit in Z order."""
    c = ctu >> (1 if plane else 0)
    cw = -(-(w >> (1 if plane else 0)) // c)
    z = _spread4((x & (c - 1)) >> 2) | (_spread4((y & (c - 1)) >> 2) << 1)
    return ((y // c) * cw + (x // c)) * c * c + z * 16


def load_pictures(path):
    d = np.load(path)
    for i in range(int(d["n"])):
        poc, w, h, B, qp, ctu, slice_type = (int(v) for v in d[f"hdr{i}"])
        yield dict(poc=poc, w=w, h=h, B=B, qp=qp, ctu=ctu, slice_type=slice_type, pus=d[f"pus{i}"], cus=d[f"cus{i}"], tus=d[f"tus{i}"], lev=[d[f"lev{i}_{k}"] for k in range(3)],
                   rec=[d[f"rec{i}_{k}"] for k in range(3)], org=[d[f"org{i}_{k}"] for k in range(3)] if f"org{i}_0" in d else None, sao=np.ascontiguousarray(d[f"sao{i}"]), dbk=[int(v) for v in d[f"dbk{i}"]],
                   region=np.ascontiguousarray(d[f"region{i}"], np.uint32) if f"region{i}" in d else None, cip=bool(int(d[f"cip{i}"])) if f"cip{i}" in d else False,
                   slice_id=np.ascontiguousarray(d[f"slice_id{i}"], np.uint32) if f"slice_id{i}" in d else None,
                   tile_id=np.ascontiguousarray(d[f"tile_id{i}"], np.uint32) if f"tile_id{i}" in d else None,
                   lf_cross_slice=np.ascontiguousarray(d[f"lf_cross_slice{i}"], np.uint8) if f"lf_cross_slice{i}" in d else None,
                   lf_cross_tile=bool(int(d[f"lf_cross_tile{i}"])) if f"lf_cross_tile{i}" in d else True,
                   wp=dict(flags=tuple(int(v) for v in d[f"wpflags{i}"]), poc=[d[f"wppoc{i}_{l}"] for l in (0, 1)], tab=[d[f"wptab{i}_{l}"] for l in (0, 1)],
                           ridx=d[f"ridx{i}"]) if f"wpflags{i}" in d else None)


def tile_scan(cw, ch, col_bounds, row_bounds):
    """CtbAddrTsToRs (H.265 6.5.1): CTU raster addresses in tile-scan order, with the tile index of each.  col_bounds /
    row_bounds = the CTU columns / rows where tiles start, 0 first (e.g. [0, 3, 5] for three tile columns)."""
    cb, rb = list(col_bounds) + [cw], list(row_bounds) + [ch]
    order, tile = [], []
    for j in range(len(rb) - 1):
        for i in range(len(cb) - 1):
            for y in range(rb[j], rb[j + 1]):
                for x in range(cb[i], cb[i + 1]):
                    order.append(y * cw + x)
                    tile.append(j * (len(cb) - 1) + i)
    return np.array(order, np.int64), np.array(tile, np.int64)


def uniform_bounds(n_ctu, n_tiles):
    """Tile boundaries with uniform spacing (H.265 6.5.1, uniform_spacing_flag = 1)."""
    return [(i * n_ctu) // n_tiles for i in range(n_tiles)]


def region_map(w, h, ctu, slice_starts=(0,), col_bounds=(0,), row_bounds=(0,)):
    """Region id of every CTU in raster order: one region per (independent slice, tile) pair.  slice_starts = tile-scan CTU
    addresses where independent slices begin (slices start at CTU boundaries; dependent slices are not listed: they do
    not split regions)."""
    cw, ch = -(-w // ctu), -(-h // ctu)
    order, tile = tile_scan(cw, ch, col_bounds, row_bounds)
    starts = np.array(sorted(set(int(s) for s in slice_starts) | {0}), np.int64)
    sl = np.searchsorted(starts, np.arange(cw * ch), side="right") - 1  # slice of each tile-scan address
    n_tiles = int(tile.max()) + 1
    region = np.zeros(cw * ch, np.uint32)
    region[order] = (sl * n_tiles + tile).astype(np.uint32)
    return region


def slice_tile_maps(w, h, ctu, slice_starts=(0,), col_bounds=(0,), row_bounds=(0,)):
    """(slice index, tile index) of every CTU in raster order; arguments as for region_map."""
    cw, ch = -(-w // ctu), -(-h // ctu)
    order, tile = tile_scan(cw, ch, col_bounds, row_bounds)
    starts = np.array(sorted(set(int(s) for s in slice_starts) | {0}), np.int64)
    sl = np.searchsorted(starts, np.arange(cw * ch), side="right") - 1
    slice_id, tile_id = np.zeros(cw * ch, np.uint32), np.zeros(cw * ch, np.uint32)
    slice_id[order], tile_id[order] = sl.astype(np.uint32), tile.astype(np.uint32)
    return slice_id, tile_id


# neighbour CTU k of the availability byte, (dx, dy): the SGU_* enumeration (COM/TComDataCU.h:64-72)
SGU_L, SGU_R, SGU_T, SGU_B, SGU_TL, SGU_TR, SGU_BL, SGU_BR = range(8)
SGU_OFFSETS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (-1, 1), (1, 1))


def lf_border_avail(w, h, ctu, slice_id=None, slice_lf_cross=None, tile_id=None, lf_cross_tiles=True):
    """The numpy twin of hmx_lf_border_avail (TComDataCU::setNDBFilterBlockBorderAvailability, COM/TComDataCU.cpp:4212-4634
    with MODIFIED_CROSS_SLICE): one byte per CTU in raster order, bit k set = neighbour CTU k may be read.  A neighbour
    outside the picture: no.  Same slice: yes; a later slice: that slice's flag; an earlier slice: this slice's flag; one
    slice in the picture: no slice test.  Then ANDed with "same tile" when lf_cross_tiles is false.  slice_id None = one
    slice: the mask of the picture's geometry alone."""
    cw, ch = -(-w // ctu), -(-h // ctu)
    sid = np.zeros((ch, cw), np.int64) if slice_id is None else np.asarray(slice_id, np.int64).reshape(ch, cw)
    flags = np.ones(1, bool) if slice_lf_cross is None else np.asarray(slice_lf_cross).astype(bool).reshape(-1)
    if sid.min() < 0 or sid.max() >= len(flags):
        raise ValueError("lf_border_avail: slice id without a flag")
    tid = None if tile_id is None else np.asarray(tile_id, np.int64).reshape(ch, cw)
    out = np.zeros((ch, cw), np.uint8)
    ys, xs = np.mgrid[0:ch, 0:cw]
    for k, (dx, dy) in enumerate(SGU_OFFSETS):
        ny, nx = ys + dy, xs + dx
        inside = (ny >= 0) & (ny < ch) & (nx >= 0) & (nx < cw)
        ny, nx = np.clip(ny, 0, ch - 1), np.clip(nx, 0, cw - 1)
        other = sid[ny, nx]
        ok = inside & ((len(flags) == 1) | (other == sid) | flags[np.maximum(other, sid)])
        if tid is not None and not lf_cross_tiles:
            ok &= tid[ny, nx] == tid
        out |= (ok.astype(np.uint8) << k).astype(np.uint8)
    return out.reshape(-1)


def picture_avail(p):
    """The availability bytes of a picture dict (the geometry's alone without slice / tile maps)."""
    return lf_border_avail(p["w"], p["h"], p["ctu"], p.get("slice_id"), p.get("lf_cross_slice"), p.get("tile_id"), p.get("lf_cross_tile", True))


def avail_is_geometry(p, avail):
    """True when every bit of a neighbour inside the picture is set: the loop filters cross every CTU boundary."""
    return np.array_equal(avail, lf_border_avail(p["w"], p["h"], p["ctu"]))


def _drop_closed_edges(p, ver, hor):
    """Clears the vertical-edge entries in the first unit column of a CTU whose L bit is clear and the horizontal-edge
    entries in the first unit row of a CTU whose T bit is clear (COM/TComLoopFilter.cpp:411, 432: getPULeft / getPUAbove
    return no unit across a slice or tile boundary the filter may not cross; the left and top neighbours are never in a
    later slice, so the SAO byte serves).  ver / hor: [4x4 unit row][4x4 unit column], modified in place."""
    avail = picture_avail(p)
    n, cw = p["ctu"] // 4, -(-p["w"] // p["ctu"])
    for a, m in enumerate(avail):
        cy, cx = divmod(a, cw)
        if cx and not (m >> SGU_L) & 1:
            ver[cy * n:(cy + 1) * n, cx * n] = 0
        if cy and not (m >> SGU_T) & 1:
            hor[cy * n, cx * n:(cx + 1) * n] = 0


def intra_unit_map(p):
    """The intra flag of every 4x4 luma unit of a picture, from its coding units (constrained intra prediction)."""
    uw, uh = -(-p["w"] // 4), -(-p["h"] // 4)
    m = np.zeros((uh, uw), np.uint8)
    for c in p["cus"]:
        n, x, y = (1 << int(c["log2size"])) // 4, int(c["x"]) // 4, int(c["y"]) // 4
        m[y:y + n, x:x + n] = 1 if c["intra"] else 0
    return m


def layout_of(p):
    """The capi.Layout of a picture, or None for one region without constrained intra prediction."""
    region, cip = p.get("region"), p.get("cip", False)
    if region is None and not cip:
        return None
    from thevc_amd import capi
    return capi.Layout(region, intra_unit_map(p) if cip else None)


def deblock_maps(p):
    """Boundary strengths of an all-intra picture (xGetBoundaryStrengthSingle :444-470: 2 wherever an edge is
    filtered): the left / top sides of the luma transform blocks that lie on the 8x8 grid, not on the picture boundary
    (xSetEdgefilterTU, xSetEdgefilterPU :264-330; every coding-unit edge is also a transform-block edge)."""
    uw, uh = p["w"] // 4, p["h"] // 4
    bsv, bsh = np.zeros((uh, uw), np.uint8), np.zeros((uh, uw), np.uint8)
    for t in p["tus"]:
        if t["plane"]:
            continue
        n, x, y = (1 << int(t["log2n"])) // 4, int(t["x"]) // 4, int(t["y"]) // 4
        if x and x % 2 == 0:
            bsv[y:y + n, x] = 2
        if y and y % 2 == 0:
            bsh[y, x:x + n] = 2
    _drop_closed_edges(p, bsv, bsh)
    return bsv, bsh, qp_unit_map(p)[:uh, :uw]


def qp_unit_map(p):
    """The luma QP of every 4x4 luma unit, int8 [ceil(h / 4)][ceil(w / 4)]: the picture's qp_map, or its one QP everywhere."""
    uw, uh = -(-p["w"] // 4), -(-p["h"] // 4)
    if p.get("qp_map") is None:
        return np.full((uh, uw), p["qp"], np.int8)
    m = np.ascontiguousarray(p["qp_map"], np.int8)
    if m.shape != (uh, uw):
        raise ValueError(f"qp_map: shape {m.shape}, the picture has {(uh, uw)} units")
    return m


DBK_UNIT = np.dtype([("intra", "u1"), ("cbf", "u1"), ("ref", "i1", 2), ("mv", "<i2", (2, 2))])


def strength_inputs(p):
    """What xGetBoundaryStrengthSingle reads, per 4x4 unit, and the edge maps (hmx_deblock_strengths): intra flag from the
    coding units, luma coded-block flag from the transform blocks, reference picture (its POC; -1 = list unused) and
    vector from the prediction units; edges: coding-unit and transform-block sides = 3, prediction-unit sides inside
    a coding unit = 1 (xSetEdgefilterTU / xSetEdgefilterPU, COM/TComLoopFilter.cpp:264-330)."""
    uw, uh = p["w"] // 4, p["h"] // 4
    units = np.zeros((uh, uw), DBK_UNIT)
    units["ref"][:] = -1
    ev, eh = np.zeros((uh, uw), np.uint8), np.zeros((uh, uw), np.uint8)

    def sides(x, y, wd, ht, v):
        if x:
            ev[y:y + ht, x] |= v
        if y:
            eh[y, x:x + wd] |= v

    for c in p["cus"]:
        n, x, y = (1 << int(c["log2size"])) // 4, int(c["x"]) // 4, int(c["y"]) // 4
        units["intra"][y:y + n, x:x + n] = c["intra"]
        sides(x, y, n, n, 3)
    for t in p["tus"]:
        if t["plane"] == 0:
            n, x, y = (1 << int(t["log2n"])) // 4, int(t["x"]) // 4, int(t["y"]) // 4
            units["cbf"][y:y + n, x:x + n] = 1 if int(t["flags"]) & 0x80 else 0
            sides(x, y, n, n, 3)
    for u in p["pus"]:
        x, y, wd, ht = int(u["x"]) // 4, int(u["y"]) // 4, int(u["w"]) // 4, int(u["h"]) // 4
        for l in (0, 1):
            if u[f"poc{l}"] > -32768:
                units["ref"][y:y + ht, x:x + wd, l] = int(u[f"poc{l}"])
                units["mv"][y:y + ht, x:x + wd, l, 0] = int(u[f"mv{l}x"])
                units["mv"][y:y + ht, x:x + wd, l, 1] = int(u[f"mv{l}y"])
        sides(x, y, wd, ht, 1)
    _drop_closed_edges(p, ev, eh)
    return np.ascontiguousarray(units), ev, eh


def is_deblocked(p):
    return not p["dbk"][0]


def has_sao(p):
    return bool((p["sao"]["type"] >= 0).any())


def levels_to_planes(p):
    """The picture's levels from the reference's per-CTU layout into plane geometry, following the block list."""
    w, h = p["w"], p["h"]
    lev = [np.zeros((h, w), np.int32), np.zeros((h // 2, w // 2), np.int32), np.zeros((h // 2, w // 2), np.int32)]
    for t in p["tus"]:
        n, pl, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
        o = z_offset(pl, x, y, w, p["ctu"])
        lev[pl][y:y + n, x:x + n] = p["lev"][pl][o:o + n * n].reshape(n, n)
    return lev


def prediction_units(p, slot):
    """The tap's prediction units as hmx_pu / hmo_pu records: reference POC -> slot of the reference table, vectors
    clipped as motion compensation clips them (TComDataCU::clipMv, COM/TComDataCU.cpp:3505-3517: relative to the
    coding unit's origin, 8 samples + one CTU beyond the picture)."""
    src, ctu = p["pus"], p["ctu"]
    out = np.zeros(len(src), PU_DTYPE)
    for k in ("x", "y", "w", "h"):
        out[k] = src[k]
    cx, cy = src["cu_x"].astype(np.int64), src["cu_y"].astype(np.int64)
    for l in (0, 1):
        used = src[f"poc{l}"] > -32768
        out[f"ref{l}"] = [slot[int(v)] if u else 255 for v, u in zip(src[f"poc{l}"], used)]
        out[f"mv{l}x"] = np.clip(src[f"mv{l}x"].astype(np.int64), (-ctu - 8 - cx + 1) * 4, (p["w"] + 8 - cx - 1) * 4)
        out[f"mv{l}y"] = np.clip(src[f"mv{l}y"].astype(np.int64), (-ctu - 8 - cy + 1) * 4, (p["h"] + 8 - cy - 1) * 4)
    return out


def weighted(p):
    """The slice is predicted with explicit weights: a P slice under the PPS's use-WP flag, a B slice under its WP bi-pred flag
    (TComPrediction.cpp:516-535; a B slice with use WP alone is NOT weighted)."""
    wp = p.get("wp")
    return bool(wp and ((p["slice_type"] == 1 and wp["flags"][0]) or (p["slice_type"] == 0 and wp["flags"][1])))


def weighted_prediction_units(p):
    """A weighted slice's units for hmx_batch_motionCompensation_wp_multi: (hmx_pu records, the POC of every refs[] entry, l0, l1).
    refs[] gets one entry per distinct (picture, list-0 row, list-1 row), as include/hmx.h prescribes: the (list, refIdx) pairs
    the units use, list 0's first; a pair of list 1 joins an entry of the same picture whose list-1 row is free or equal.  A
    picture that sits in a list twice with different rows therefore has two entries.  l0 / l1: tables of capi.WP_DTYPE indexed
    like refs[]; a row no unit addresses holds the default weight 1 << denominator, offset 0."""
    from thevc_amd import capi
    wp = p["wp"]
    used = {}
    for u, r in zip(p["pus"], wp["ridx"]):
        for l in (0, 1):
            if r[l] >= 0:
                assert int(u[f"poc{l}"]) == int(wp["poc"][l][r[l]])
                used[(l, int(r[l]))] = int(u[f"poc{l}"])
    entries, index = [], {}  # [poc, row of list 0 or None, row of list 1 or None]
    for (l, i), poc in sorted(used.items()):
        row = tuple(int(v) for v in np.asarray(wp["tab"][l][i]).reshape(-1))
        for k, e in enumerate(entries):
            if e[0] == poc and e[1 + l] in (None, row) and (l == 1 or e[1] == row):
                e[1 + l], index[(l, i)] = row, k
                break
        else:
            index[(l, i)] = len(entries)
            entries.append([poc, row if l == 0 else None, row if l == 1 else None])
    denom = [int(v) for v in np.asarray(wp["tab"][0][0])[:, 2]]
    default = tuple(v for d in denom for v in (1 << d, 0, d))
    tabs = [np.zeros(len(entries), capi.WP_DTYPE), np.zeros(len(entries), capi.WP_DTYPE)]
    for k, e in enumerate(entries):
        for l in (0, 1):
            row = np.array(e[1 + l] or default).reshape(3, 3)
            tabs[l][k]["weight"], tabs[l][k]["offset"], tabs[l][k]["log2_denom"] = row[:, 0], row[:, 1], row[:, 2]
    slot = [{poc: 0 for poc in used.values()}] * 2  # placeholders: the slots of a weighted slice come from the reference indices
    out = prediction_units(p, slot[0])
    for l in (0, 1):
        out[f"ref{l}"] = [index[(l, int(r[l]))] if r[l] >= 0 else 255 for r in wp["ridx"]]
    return out, [e[0] for e in entries], tabs[0], tabs[1]


def reference_pocs(p):
    return sorted({int(v) for l in (0, 1) for v in p["pus"][f"poc{l}"] if v > -32768})


def split_blocks(p):
    inter = (p["tus"]["flags"] & TU_INTER) != 0
    return np.ascontiguousarray(p["tus"][~inter], TU_DTYPE), np.ascontiguousarray(p["tus"][inter], TU_DTYPE)


def decode_sequence(pics):
    """Every picture of the stream through libhmx, in decoding order; returns the output pictures (three planes each)."""
    from thevc_amd import capi
    L = capi.lib()
    pics = list(pics)
    ctx = capi.Context(bit_depth=pics[0]["B"], ctu_size=pics[0]["ctu"])
    out = []
    refs, m = {}, MARGIN
    try:
        for p in pics:
            w, h = p["w"], p["h"]
            intra_tus, inter_tus = split_blocks(p)
            d_rec = capi.DevPicture(ctx, w, h, m, m).zero()
            rec_arr = (capi.Pic * 1)(d_rec.as_pic())
            keep = []
            if p.get("qp_map") is not None:  # a QP per block for this picture's transform calls (synchronised before it is freed)
                d_qm = ctx.to_device(qp_unit_map(p))
                ctx.set_qp_map(d_qm, 1)
                keep += [d_qm]
            else:
                ctx.set_qp_map(None)
            if len(p["pus"]):
                # Without weighting a unit whose two lists name one picture and one vector is predicted from list 0 alone
                # (xCheckIdenticalMotion, TComPrediction.cpp:392-407); the average of a 14-bit intermediate with itself rounds to the
                # same sample, so the unweighted entry needs no such case.  Under WP bi-pred the shortcut is off (:394) and the weighted
                # entry always takes the bi formula.
                if weighted(p):
                    pus, pocs, l0, l1 = weighted_prediction_units(p)
                else:
                    pocs = reference_pocs(p)
                    pus = prediction_units(p, {poc: i for i, poc in enumerate(pocs)})
                d_pus = ctx.to_device(pus)
                ref_arr = (capi.Pic * len(pocs))(*[refs[poc].as_pic() for poc in pocs])
                d_pred = capi.DevPicture(ctx, w, h).zero()
                pred_arr = (capi.Pic * 1)(d_pred.as_pic())
                for dst in (pred_arr, rec_arr):  # the prediction, and the reconstruction of units without residual
                    job = (capi.McJob * 1)()
                    job[0].d_pus, job[0].n_pus, job[0].refs, job[0].n_refs = d_pus.ptr, len(pus), ref_arr, len(pocs)
                    job[0].dst, job[0].pic_w, job[0].pic_h = C.pointer(dst[0]), w, h
                    if weighted(p):
                        ctx.batch_motion_compensation_wp(job, [(l0, l1 if p["slice_type"] == 0 else None)])
                    else:
                        ctx._chk(L.hmx_batch_motionCompensation_multi(ctx.h, 1, job))
                if len(inter_tus):
                    tl = ctx.tu_list(inter_tus)
                    d_lp = capi.DevPicture(ctx, w, h, dtype=np.int32).upload(levels_to_planes(p))
                    lp_arr = (capi.Levels * 1)(d_lp.as_pic())
                    pp = capi.PicParam(w, h, p["qp"], 0, capi.B_SLICE, 1)
                    ctx._chk(L.hmx_batch_invtransformNxN_multi(ctx.h, tl, 1, lp_arr, pred_arr, rec_arr, C.byref(pp)))
                    keep += [d_lp]
                keep += [d_pred, d_pus]
            if len(intra_tus):
                plan = ctx.intra_plan(intra_tus, capi.PicParam(w, h, p["qp"], 0, capi.I_SLICE, 1), layout=layout_of(p))
                d_lev = capi.DevLevelsZ(ctx, w, h, p["ctu"])
                for k in range(3):
                    assert d_lev.elems[k] == len(p["lev"][k]), "levels are not in the per-CTU layout of this picture size"
                    d_lev.bufs[k].upload(np.ascontiguousarray(p["lev"][k], np.int32))
                lev_arr = (capi.Levels * 1)(d_lev.as_pic())
                fn = L.hmx_frame_intra_decode_onto if len(p["pus"]) else L.hmx_frame_intra_decode
                ctx._chk(fn(ctx.h, plan, 1, rec_arr, lev_arr))
                ctx.sync()
                L.hmx_intra_plan_destroy(ctx.h, plan)
                d_lev.free()
            if is_deblocked(p):
                bsv, bsh, qpm = deblock_maps(p)
                d_bv, d_bh, d_qp = ctx.to_device(bsv), ctx.to_device(bsh), ctx.to_device(np.ascontiguousarray(qpm))
                if len(p["pus"]):
                    units, ev, eh = strength_inputs(p)
                    d_u, d_ev, d_eh = ctx.to_device(units), ctx.to_device(ev), ctx.to_device(eh)
                    ctx.deblock_strengths(1, d_u, d_ev, d_eh, w, h, [int(p["slice_type"] == 0)], d_bv, d_bh)
                ctx.deblock_pictures([d_rec], w, h, d_bv, d_bh, d_qp, None, [p["dbk"][1]], [p["dbk"][2]])
            d_out = d_rec
            if has_sao(p):
                d_out = capi.DevPicture(ctx, w, h, m, m).zero()
                d_prm = ctx.to_device(p["sao"])
                assert p["sao"].shape[1] == -(-w // p["ctu"]) * -(-h // p["ctu"])
                avail = picture_avail(p)
                if avail_is_geometry(p, avail):
                    ctx.sao_pictures([d_rec], [d_out], w, h, d_prm)
                else:  # a slice or tile boundary the filter may not cross: processSaoBlock
                    d_av = ctx.to_device(avail)
                    ctx.sao_pictures_avail([d_rec], [d_out], w, h, d_prm, d_av)
                    keep += [d_av]
            ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(d_out.as_pic()), w, h, m, m))
            ctx.sync()
            refs[p["poc"]] = d_out
            out.append(d_out.download())
            for d in keep:
                d.free()
    finally:
        ctx.close()
    return out
