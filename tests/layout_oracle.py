"""The CPU oracle of intra availability with slices, tiles and constrained intra prediction, and the decode composed from
it: per block in coding order, hmo_fillReferenceSamples with the layout's flags, then smoothing, prediction, inverse
transform and reconstruction (TComPattern.cpp:213-786, TComPrediction.cpp:338-386, DEC/TDecCu.cpp:469-687).  The rule is
modelled unit by unit here, independently of libhmx: a neighbour unit is available when geometry says so
(hmo_intra_avail), it lies in the block's region, and, with constrained intra pred, it is intra-coded."""
import ctypes as C

import numpy as np

import oracle_lib as ol
from thevc_amd.decisions import (MARGIN, intra_unit_map, is_deblocked, has_sao, levels_to_planes, prediction_units, reference_pocs,
                                 split_blocks)


def unit_positions(x, y, size, ulog2):
    """Luma sample of each of the 4n + 1 neighbour units (bNeighborFlags order), units of 1 << ulog2 samples."""
    n, us = size >> ulog2, 1 << ulog2
    pos = [(x - 1, y + (2 * n - 1 - u) * us) for u in range(2 * n)] + [(x - 1, y - 1)]
    return pos + [(x + k * us, y - 1) for k in range(2 * n)]


def layout_flags(geo, x, y, size, ulog2, region=None, intra=None, ctu=64):
    """geo (4n + 1 flags) cut down to the layout: same region as the block (region: a Region), and intra-coded where intra
    (per-4x4-unit flags) is given."""
    f = np.array(geo, np.uint8).copy()
    for u, (sx, sy) in enumerate(unit_positions(x, y, size, ulog2)):
        if not f[u]:
            continue
        if region is not None and region[(sy // ctu) * region.cols + sx // ctu] != region[(y // ctu) * region.cols + x // ctu]:
            f[u] = 0
        if intra is not None and not intra[sy >> 2, sx >> 2]:
            f[u] = 0
    return f


class Region(np.ndarray):
    """A region map (region id per CTU, raster order) that knows its CTUs per row."""

    def __new__(cls, arr, w, ctu=64):
        obj = np.asarray(arr, np.uint32).view(cls)
        obj.cols = -(-w // ctu)
        return obj

    def __array_finalize__(self, obj):
        self.cols = getattr(obj, "cols", None)


def geometric_flags(x, y, size, w, h, ctu=64):
    O = ol.oracle()
    f = np.zeros(65, np.uint8)
    O.hmo_intra_avail(x, y, size, w, h, ctu, f)
    return f[:4 * (size // 4) + 1]


def block_flags(t, w, h, region, intra, geometric=False):
    sh = 1 if t["plane"] else 0
    x, y, s = int(t["x"]) << sh, int(t["y"]) << sh, (1 << int(t["log2n"])) << sh
    geo = geometric_flags(x, y, s, w, h)
    return geo if geometric else layout_flags(geo, x, y, s, 2, region, intra)


def intra_blocks(tus, rec, lev, w, h, B, qp, region, intra, geometric=False):
    """The intra blocks of a picture in list (coding) order onto rec (three int16 planes), levels in plane geometry."""
    O = ol.oracle()
    mx = (1 << B) - 1
    for t in tus:
        k, N, x, y, mode = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["mode"])
        f = block_flags(t, w, h, region, intra, geometric)
        flags = np.zeros(65, np.uint8)
        flags[:f.size] = f
        plane = rec[k].reshape(-1)
        stride = rec[k].shape[1]
        W = 2 * N + 1
        adi = np.zeros(2 * W * W, np.int32)
        O.hmo_fillReferenceSamples(ol.ptr(plane, y * stride + x), stride, flags, int(f.sum()), 2 if k else 4, N, B, adi)
        pred = np.zeros((N, N), np.int16)
        if k:
            O.hmo_predIntraChromaAng(adi, mode, pred.reshape(-1), N, N, B)
        else:
            O.hmo_filterAdi(adi, N)
            O.hmo_predIntraLumaAng(adi, mode, pred.reshape(-1), N, N, B)
        q = O.hmo_setQPforQuant(qp, int(k != 0), 6 * (B - 8), 0)
        tmode = mode if k == 0 else 65535
        r = ol.o_invtransformNxN(lev[k][y:y + N, x:x + N], N, B, tmode, q.per, q.rem, int(t["flags"]) & 1)
        rec[k][y:y + N, x:x + N] = np.clip(pred.astype(np.int32) + r, 0, mx)


def picture_layout(p):
    region = None if p.get("region") is None else Region(p["region"], p["w"], p["ctu"])
    intra = intra_unit_map(p) if p.get("cip") else None
    return region, intra


def decode(pics, geometric=False):
    """Every picture of a layout fixture (loop filters off), in decoding order; references are this function's outputs.
    geometric=True ignores the layout (what a decoder without the rule computes)."""
    O = ol.oracle()
    P3, I3 = C.c_void_p * 3, C.c_int * 3
    ext, out = {}, []
    for p in pics:
        assert not is_deblocked(p) and not has_sao(p), "layout fixtures are coded without loop filters"
        w, h, B, m = p["w"], p["h"], p["B"], MARGIN
        st = I3(w, w // 2, w // 2)
        lev = levels_to_planes(p)
        rec = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        intra_tus, inter_tus = split_blocks(p)
        if len(p["pus"]):
            pocs = reference_pocs(p)
            pus = prediction_units(p, {poc: i for i, poc in enumerate(pocs)})
            ptrs = (C.c_void_p * (3 * len(pocs)))()
            for i, poc in enumerate(pocs):
                for k in range(3):
                    pm, pw = (m, w) if k == 0 else (m // 2, w // 2)
                    ptrs[i * 3 + k] = ext[poc][k].ctypes.data + 2 * (pm * (pw + 2 * pm) + pm)
            O.hmo_mc_frame(pus.ctypes.data, len(pus), B, ptrs, I3(w + 2 * m, w // 2 + m, w // 2 + m), P3(*[a.ctypes.data for a in rec]), st)
            mx = (1 << B) - 1
            for t in inter_tus:
                n, k, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
                q = O.hmo_setQPforQuant(p["qp"], int(k != 0), 6 * (B - 8), 0)
                r = ol.o_invtransformNxN(lev[k][y:y + n, x:x + n], n, B, 65535, q.per, q.rem, int(t["flags"]) & 1)
                rec[k][y:y + n, x:x + n] = np.clip(rec[k][y:y + n, x:x + n].astype(np.int32) + r, 0, mx)
        region, intra = picture_layout(p)
        intra_blocks(intra_tus, rec, lev, w, h, B, p["qp"], region, intra, geometric)
        planes = []
        for k, a in enumerate(rec):
            pm = m if k == 0 else m // 2
            ph, pw = a.shape
            e = np.zeros((ph + 2 * pm, pw + 2 * pm), np.int16)
            e[pm:pm + ph, pm:pm + pw] = a
            flat = e.reshape(-1)
            O.hmo_extendPicBorder(ol.ptr(flat, pm * (pw + 2 * pm) + pm), pw + 2 * pm, pw, ph, pm, pm)
            planes.append(flat)
        ext[p["poc"]] = planes
        out.append(rec)
    return out
