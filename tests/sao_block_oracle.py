"""The yardstick of the loop filters at slice and tile boundaries they may not cross: the reference's block path of SAO,
TComSampleAdaptiveOffset::processSaoBlock (TLibCommon/TComSampleAdaptiveOffset.cpp:561-776) and
TEncSampleAdaptiveOffset::calcSaoStatsBlock (TLibEncoder/TEncSampleAdaptiveOffset.cpp:571-811), restated twice.

apply_literal / stats_literal   branch by branch from the source, with its start / end columns, its first-line, last-line and
                                corner branches and its running sign buffers (m_iUpBuff1 / m_iUpBufft); slow.  The two source
                                functions walk a block in the same way (same bounds, same branches, same buffers) and differ
                                in what they do with a visited sample, so one walker, _visits, restates both.
apply_rule / stats_rule         numpy, the per-sample rule of include/hmx.h: an edge-offset sample counts exactly when each of
                                its two neighbours lies in its own CTU or in a neighbour CTU whose availability bit is set.

avail: one byte per CTU in raster order, bit k = neighbour CTU k may be read, k = SGU_L, R, T, B, TL, TR, BL, BR
(thevc_amd.decisions.lf_border_avail).  Pictures are three 2-D planes (4:2:0); the chroma planes use the CTU's byte.
cpu_decode() is the stream direction on the CPU: block path with the layout rule, the oracle's deblocking with the closed
edges dropped, then apply_literal.
"""
import ctypes as C

import numpy as np

BINS = 52
EO_TABLE = (1, 2, 0, 3, 4)  # m_auiEoTable, TLibCommon/TComSampleAdaptiveOffset.cpp:94
L, R, T, B_, TL, TR, BL, BR = range(8)  # SGU_*, TLibCommon/TComDataCU.h:64-72


def _sign(v):
    return (v > 0) - (v < 0)


def _visits(D, width, height, sao_type, av):
    """(x, y, edgeType) of every sample an edge-offset type visits in one block, in the source's order.  D(x, y) = the
    unfiltered sample at block-local (x, y) (pDec / pRec of the source; neighbours outside the block are read through it)."""
    if sao_type == 0:  # SAO_EO_0 :570-590
        start_x = 0 if av[L] else 1
        end_x = width if av[R] else width - 1
        for y in range(height):
            sign_left = _sign(D(start_x, y) - D(start_x - 1, y))
            for x in range(start_x, end_x):
                sign_right = _sign(D(x, y) - D(x + 1, y))
                e = sign_right + sign_left + 2
                sign_left = -sign_right
                yield x, y, e
    elif sao_type == 1:  # SAO_EO_1 :591-618
        start_y = 0 if av[T] else 1
        end_y = height if av[B_] else height - 1
        up = [_sign(D(x, start_y) - D(x, start_y - 1)) for x in range(width)]
        for y in range(start_y, end_y):
            for x in range(width):
                sign_down = _sign(D(x, y) - D(x, y + 1))
                e = sign_down + up[x] + 2
                up[x] = -sign_down
                yield x, y, e
    elif sao_type == 2:  # SAO_EO_2 :619-691 (posShift = stride + 1)
        start_x = 0 if av[L] else 1
        end_x = width if av[R] else width - 1
        up1, upt = [None] * (width + 2), [None] * (width + 2)
        for x in range(start_x, end_x + 1):  # prepare 2nd line upper sign
            up1[x] = _sign(D(x, 1) - D(x - 1, 0))
        if av[TL]:  # 1st line
            yield 0, 0, _sign(D(0, 0) - D(-1, -1)) - up1[1] + 2
        if av[T]:
            for x in range(1, end_x):
                yield x, 0, _sign(D(x, 0) - D(x - 1, -1)) - up1[x + 1] + 2
        for y in range(1, height - 1):  # middle lines
            for x in range(start_x, end_x):
                sign_down1 = _sign(D(x, y) - D(x + 1, y + 1))
                yield x, y, sign_down1 + up1[x] + 2
                upt[x + 1] = -sign_down1
            upt[start_x] = _sign(D(start_x, y + 1) - D(start_x - 1, y))
            up1, upt = upt, up1
        y = height - 1  # last line
        if av[B_]:
            for x in range(start_x, width - 1):
                yield x, y, _sign(D(x, y) - D(x + 1, y + 1)) + up1[x] + 2
        if av[BR]:
            x = width - 1
            yield x, y, _sign(D(x, y) - D(x + 1, y + 1)) + up1[x] + 2
    elif sao_type == 3:  # SAO_EO_3 :692-759 (posShift = stride - 1); the buffer is indexed x + 1 (the source reaches index -1)
        start_x = 0 if av[L] else 1
        end_x = width if av[R] else width - 1
        up1 = [None] * (width + 2)
        for x in range(start_x - 1, end_x):  # prepare 2nd line upper sign
            up1[x + 1] = _sign(D(x, 1) - D(x + 1, 0))
        if av[T]:  # first line
            for x in range(start_x, width - 1):
                yield x, 0, _sign(D(x, 0) - D(x + 1, -1)) - up1[x - 1 + 1] + 2
        if av[TR]:
            x = width - 1
            yield x, 0, _sign(D(x, 0) - D(x + 1, -1)) - up1[x - 1 + 1] + 2
        for y in range(1, height - 1):  # middle lines
            for x in range(start_x, end_x):
                sign_down1 = _sign(D(x, y) - D(x - 1, y + 1))
                yield x, y, sign_down1 + up1[x + 1] + 2
                up1[x - 1 + 1] = -sign_down1
            up1[end_x - 1 + 1] = _sign(D(end_x - 1, y + 1) - D(end_x, y))
        y = height - 1  # last line
        if av[BL]:
            yield 0, y, _sign(D(0, y) - D(-1, y + 1)) + up1[0 + 1] + 2
        if av[B_]:
            for x in range(1, end_x):
                yield x, y, _sign(D(x, y) - D(x - 1, y + 1)) + up1[x + 1] + 2


def _blocks(w, h, ctu, comp):
    """(CTU address, x, y, width, height) of every CTU in a plane: the NDBFBlockInfo of a CTU, >> 1 for chroma (:537-540)."""
    sh = 1 if comp else 0
    pw, ph, cs = w >> sh, h >> sh, ctu >> sh
    cw, ch = -(-w // ctu), -(-h // ctu)
    for a in range(cw * ch):
        x, y = (a % cw) * cs, (a // cw) * cs
        yield a, x, y, min(cs, pw - x), min(cs, ph - y)


def _reader(plane):
    """D(x, y) factory on a plane padded by one sample (an unavailable neighbour outside the picture is never USED; the
    source forms a few signs next to the block that it then drops)."""
    rows = np.pad(np.asarray(plane, np.int64), 1, mode="edge").tolist()
    return lambda x0, y0: (lambda x, y: rows[y0 + y + 1][x0 + x + 1])


def _bits(m):
    return [bool((int(m) >> k) & 1) for k in range(8)]


def apply_literal(planes, prm, w, h, B, ctu, avail, only=None):
    """processSaoCu -> processSaoBlock for every CTU and component.  prm: [3, CTUs] records (type -1..4, band, offset[4]);
    offsets << (B - min(B, 10)) (m_uiSaoBitIncrease :1010).  only: CTU addresses to process (the others are copied)."""
    mx, up = (1 << B) - 1, B - min(B, 10)
    out = []
    for comp, plane in enumerate(planes):
        at = _reader(plane)
        rest = np.array(plane, np.int64)
        for a, x0, y0, width, height in _blocks(w, h, ctu, comp):
            q = prm[comp][a]
            t = int(q["type"])
            if t < 0 or (only is not None and a not in only):
                continue
            offs = [0] + [int(v) << up for v in q["offset"]]
            D = at(x0, y0)
            if t == 4:  # SAO_BO :760-772; m_iOffsetBo :1170-1187
                table = [0] * 33
                for i in range(4):
                    table[(int(q["band"]) + i) % 32 + 1] = offs[i + 1]
                for y in range(height):
                    for x in range(width):
                        v = D(x, y)
                        rest[y0 + y, x0 + x] = min(mx, max(0, v + table[1 + (v >> (B - 5))]))
                continue
            off_eo = [offs[EO_TABLE[e]] for e in range(5)]  # m_iOffsetEo :1198
            for x, y, e in _visits(D, width, height, t, _bits(avail[a])):
                rest[y0 + y, x0 + x] = min(mx, max(0, D(x, y) + off_eo[e]))
        out.append(rest.astype(np.int16))
    return out


def stats_literal(org, rec, w, h, ctu, B, avail, only=None):
    """calcSaoStatsCu -> calcSaoStatsBlock for every CTU and component: int64 [3, CTUs, 52, 2] in the layout of hmx_sao_stats."""
    cw, ch = -(-w // ctu), -(-h // ctu)
    out = np.zeros((3, cw * ch, BINS, 2), np.int64)
    for comp in range(3):
        at = _reader(rec[comp])
        O = np.asarray(org[comp], np.int64).tolist()
        for a, x0, y0, width, height in _blocks(w, h, ctu, comp):
            if only is not None and a not in only:
                continue
            D = at(x0, y0)
            for y in range(height):  # band offset :579-597
                for x in range(width):
                    v = D(x, y)
                    k = 1 + (v >> (B - 5))
                    if k:
                        out[comp, a, 20 + k - 1] += (O[y0 + y][x0 + x] - v, 1)
            for t in range(4):
                for x, y, e in _visits(D, width, height, t, _bits(avail[a])):
                    out[comp, a, 5 * t + EO_TABLE[e]] += (O[y0 + y][x0 + x] - D(x, y), 1)
    return out


# ---- the per-sample rule -------------------------------------------------------------------------------------------------------

EO_NEIGHBOURS = ((-1, 0), (0, -1), (-1, -1), (1, -1))  # neighbour a of type 0..3 as (dx, dy); b is opposite


def _avail9(avail):
    """The byte as 9 bits, bit (sx + 1) + 3 * (sy + 1) for the CTU at (sx, sy) from this one; the centre is set."""
    m = np.asarray(avail, np.int64)
    bit = lambda k: (m >> k) & 1
    return bit(TL) | bit(T) << 1 | bit(TR) << 2 | bit(L) << 3 | 1 << 4 | bit(R) << 5 | bit(BL) << 6 | bit(B_) << 7 | bit(BR) << 8


def _plane_geometry(w, h, ctu, comp):
    sh = 1 if comp else 0
    pw, ph, cs = w >> sh, h >> sh, ctu >> sh
    cw = -(-w // ctu)
    X, Y = np.arange(pw), np.arange(ph)
    cx, cy = X // cs, Y // cs
    lx, ly = X - cx * cs, Y - cy * cs
    W, H = np.minimum(cs, pw - cx * cs), np.minimum(cs, ph - cy * cs)
    lcu = (cy * cw)[:, None] + cx[None, :]
    return lcu, (lx, W), (ly, H)


def _both_readable(a9, lcu, xs, ys, dx, dy):
    """Per sample (x, y): may both (x + dx, y + dy) and (x - dx, y - dy) be read?"""
    (lx, W), (ly, H) = xs, ys
    ok = np.ones(lcu.shape, bool)
    for s in (1, -1):
        nx, ny = lx + s * dx, ly + s * dy
        sx = np.where(nx < 0, 0, np.where(nx >= W, 2, 1))
        sy = np.where(ny < 0, 0, np.where(ny >= H, 2, 1))
        ok &= ((a9[lcu] >> (sx[None, :] + 3 * sy[:, None])) & 1).astype(bool)
    return ok


def apply_rule(planes, prm, w, h, B, ctu, avail):
    mx, up = (1 << B) - 1, B - min(B, 10)
    a9, eo, out = _avail9(avail), np.array(EO_TABLE), []
    for comp, plane in enumerate(planes):
        c = np.asarray(plane, np.int64)
        ph, pw = c.shape
        lcu, xs, ys = _plane_geometry(w, h, ctu, comp)
        q = prm[comp][lcu]
        typ, band, offs = q["type"].astype(np.int64), q["band"].astype(np.int64), q["offset"].astype(np.int64)
        pad = np.pad(c, 1, mode="edge")
        add = np.zeros_like(c)
        for t, (dx, dy) in enumerate(EO_NEIGHBOURS):
            a, b = pad[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw], pad[1 - dy:1 - dy + ph, 1 - dx:1 - dx + pw]
            slot = eo[np.sign(c - a) + np.sign(c - b) + 2]
            use = (typ == t) & _both_readable(a9, lcu, xs, ys, dx, dy) & (slot > 0)
            add = np.where(use, np.take_along_axis(offs, np.maximum(slot - 1, 0)[..., None], -1)[..., 0], add)
        k = ((c >> (B - 5)) - band) & 31
        add = np.where((typ == 4) & (k < 4), np.take_along_axis(offs, np.minimum(k, 3)[..., None], -1)[..., 0], add)
        out.append(np.clip(c + (add << up), 0, mx).astype(np.int16))
    return out


def stats_rule(org, rec, w, h, ctu, B, avail):
    cw, ch = -(-w // ctu), -(-h // ctu)
    n_lcu = cw * ch
    a9, table = _avail9(avail), np.array(EO_TABLE)
    out = np.zeros((3, n_lcu, BINS, 2), np.int64)
    for comp in range(3):
        r = np.asarray(rec[comp], np.int64)
        d = np.asarray(org[comp], np.int64) - r
        ph, pw = r.shape
        lcu, xs, ys = _plane_geometry(w, h, ctu, comp)
        pad = np.pad(r, 1, mode="edge")

        def add(mask, bins):
            idx = lcu[mask] * BINS + bins[mask]
            for j, wt in ((0, d[mask]), (1, None)):
                v = np.bincount(idx, weights=wt, minlength=n_lcu * BINS)
                out[comp, :, :, j] += np.rint(v).astype(np.int64).reshape(n_lcu, BINS)

        for t, (dx, dy) in enumerate(EO_NEIGHBOURS):
            a, b = pad[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw], pad[1 - dy:1 - dy + ph, 1 - dx:1 - dx + pw]
            add(_both_readable(a9, lcu, xs, ys, dx, dy), 5 * t + table[np.sign(r - a) + np.sign(r - b) + 2])
        add(np.ones(r.shape, bool), 20 + (r >> (B - 5)))
    return out


# ---- inputs shared by the CPU and the GPU tests --------------------------------------------------------------------------------

SAO_DTYPE = np.dtype([("type", "i1"), ("band", "u1"), ("offset", "i1", 4)])
_cache = {}


def random_params(rng, n_lcu, types=(-1, 0, 1, 2, 3, 4)):
    prm = np.zeros((3, n_lcu), SAO_DTYPE)
    prm["type"] = rng.choice(types, (3, n_lcu))
    prm["band"] = rng.integers(0, 32, (3, n_lcu))
    prm["offset"] = rng.integers(-7, 8, (3, n_lcu, 4))
    return prm


def all_masks_case(B):
    """48x48, CTU 16 (3 x 3 CTUs; chroma CTUs of 8, one strip of a thread): samples at the range ends, and 4 x 256 (parameters,
    mask) pairs: pair 256 * j + m gives the centre CTU mask m and the edge types (j, j + 1, j + 2) mod 4 on its three
    components, so that every type meets every mask on luma and on chroma; the other CTUs carry random types and the mask
    of the geometry.  -> dict(w, h, ctu, B, org, rec, prm [1024], avail [1024, 9]); shared, do not modify."""
    if B not in _cache:
        from extreme_inputs import sao_edge_content
        from thevc_amd.decisions import lf_border_avail
        rng = np.random.default_rng(480 + B)
        w = h = 48
        rec, org = sao_edge_content(rng, w, h, B), sao_edge_content(rng, w, h, B)
        geo = lf_border_avail(w, h, 16)
        prm, avail = [], []
        for j in range(4):
            base = random_params(rng, 9)
            for comp in range(3):
                base["type"][comp, 4] = (j + comp) % 4
            for m in range(256):
                a = geo.copy()
                a[4] = m
                prm.append(base)
                avail.append(a)
        _cache[B] = dict(w=w, h=h, ctu=16, B=B, org=org, rec=rec, prm=prm, avail=np.array(avail, np.uint8))
    return _cache[B]


def odd_case(B=8, n=3):
    """40x24, CTU 16: cut CTUs on the right (8 wide) and at the bottom (8 high); n pictures, each with its own parameters and
    its own random bytes on every CTU (bits towards the outside of the picture included: a mask need not be consistent)."""
    key = ("odd", B, n)
    if key not in _cache:
        from extreme_inputs import sao_edge_content
        rng = np.random.default_rng(40 + B)
        w, h = 40, 24
        pics = []
        for _ in range(n):
            pics.append(dict(rec=sao_edge_content(rng, w, h, B), org=sao_edge_content(rng, w, h, B), prm=random_params(rng, 6, (0, 1, 2, 3, 0, 1, 2, 3, 4, -1)),
                             avail=rng.integers(0, 256, 6).astype(np.uint8)))
        _cache[key] = dict(w=w, h=h, ctu=16, B=B, pics=pics)
    return _cache[key]


# ---- the stream direction on the CPU -------------------------------------------------------------------------------------------

def cpu_decode(pics, with_boundaries=True, literal=True):
    """Every picture of an lfx_* fixture in decoding order on the CPU: the block path under the layout rule (layout_oracle),
    the oracle's deblocking on the edge maps of thevc_amd.decisions (closed edges dropped), SAO by apply_literal (or
    apply_rule).  with_boundaries=False forgets the slice / tile maps in the LOOP FILTERS only: the mask of the geometry and
    every edge, which is what a decoder without the feature computes.  -> (outputs, deblocked pictures)."""
    import layout_oracle as LO
    import oracle_lib as ol
    from thevc_amd import decisions as D
    O = ol.oracle()
    P3, I3 = C.c_void_p * 3, C.c_int * 3
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    ext, out, dbk = {}, [], []
    for p in pics:
        w, h, Bd, m = p["w"], p["h"], p["B"], D.MARGIN
        st = I3(w, w // 2, w // 2)
        lev = D.levels_to_planes(p)
        rec = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        intra_tus, inter_tus = D.split_blocks(p)
        if len(p["pus"]):
            pocs = D.reference_pocs(p)
            pus = D.prediction_units(p, {poc: i for i, poc in enumerate(pocs)})
            ptrs = (C.c_void_p * (3 * len(pocs)))()
            for i, poc in enumerate(pocs):
                for k in range(3):
                    pm, pw = (m, w) if k == 0 else (m // 2, w // 2)
                    ptrs[i * 3 + k] = ext[poc][k].ctypes.data + 2 * (pm * (pw + 2 * pm) + pm)
            O.hmo_mc_frame(pus.ctypes.data, len(pus), Bd, ptrs, I3(w + 2 * m, w // 2 + m, w // 2 + m), P3(*[a.ctypes.data for a in rec]), st)
            mx = (1 << Bd) - 1
            for t in inter_tus:
                n, k, x, y = 1 << int(t["log2n"]), int(t["plane"]), int(t["x"]), int(t["y"])
                q = O.hmo_setQPforQuant(p["qp"], int(k != 0), 6 * (Bd - 8), 0)
                r = ol.o_invtransformNxN(lev[k][y:y + n, x:x + n], n, Bd, 65535, q.per, q.rem, int(t["flags"]) & 1)
                rec[k][y:y + n, x:x + n] = np.clip(rec[k][y:y + n, x:x + n].astype(np.int32) + r, 0, mx)
        region, intra = LO.picture_layout(p)
        LO.intra_blocks(intra_tus, rec, lev, w, h, Bd, p["qp"], region, intra)
        lf = p if with_boundaries else dict(p, slice_id=None, tile_id=None, lf_cross_slice=None, lf_cross_tile=True)
        if D.is_deblocked(p):
            bsv, bsh, qpm = D.deblock_maps(lf)
            if len(p["pus"]):
                units, ev, eh = D.strength_inputs(lf)
                O.hmo_deblock_strengths(vp(units), vp(ev), vp(eh), w, h, p["ctu"], int(p["slice_type"] == 0), vp(bsv), vp(bsh))
            O.hmo_deblock_picture(P3(*[a.ctypes.data for a in rec]), st, w, h, Bd, vp(bsv), vp(bsh), vp(qpm), None, p["dbk"][1], p["dbk"][2])
        dbk.append([a.copy() for a in rec])
        if D.has_sao(p):
            fn = apply_literal if literal else apply_rule
            rec = [np.ascontiguousarray(a) for a in fn(rec, p["sao"], w, h, Bd, p["ctu"], D.picture_avail(lf))]
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
    return out, dbk
