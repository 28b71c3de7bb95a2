"""Pins the CPU oracle against the compiled reference in the sample domain -- the interpolation filters, block prediction with
border extension and clipMv, addAvg, SAD / HAD / SSE, deblocking and SAO -- at 12 bit on the usual random content, and at 8, 10
and 12 bit on the range-end content of tests/extreme_inputs.py.  tests/test_gpu_inter_loop_edges.py compares libhmx with the
oracle on the same content.  Every case on extreme content counts, with the int64 restatements of extreme_inputs, that it reached
the edge it is about (> 0):
  * filter outputs beyond 0..maxv before the final clip, at both ends, and first-stage intermediates at their closed-form extremes
    ((sum of positive taps * maxv) >> (B - 8)) - 8192 and the same over the negative taps;
  * lines of the weak luma and of the chroma deblocking filter whose unclipped result leaves the range, at both ends;
  * SAO results beyond the range before the clip, at both ends, and at 12 bit offsets applied as 4 * offset;
  * |org - cur| = maxv on every sample of a block.
The weighted prediction's yardstick is held by tests/test_wp_oracle.py (12 bit included).  The tap of the compiled reference has
neither TEncSearch / xGetSAD* nor calcSaoStatsCuOrg: tests/me_oracle.py and tests/sao_stats_oracle.py are held at 12 bit and at
the opposite range ends by their second, literal restatements here."""
import ctypes as C

import numpy as np
import pytest

import extreme_inputs as xi
import me_oracle as mo
import oracle_lib as ol
import sao_stats_oracle as so
import test_oracle_vs_ref as T

pytestmark = pytest.mark.ref
P3, I3 = C.c_void_p * 3, C.c_int * 3
vp = lambda a: a.ctypes.data_as(C.c_void_p)


# ---- 12 bit on the random content of tests/test_oracle_vs_ref.py ----
def test_interpolation_filters_12bit():
    ol.ref().ref_init(12, 416, 240, 1)
    T.test_interpolation_filters(12)


def test_pred_inter_blocks_and_border_12bit():
    T._pred_inter_blocks_and_border((12,))


def test_add_avg_and_distortion_12bit():
    ol.ref().ref_init(12, 416, 240, 1)
    T.test_add_avg(12)
    T.test_distortion(12)


def test_deblock_application_12bit():
    T._deblock_application((12,))


def test_sao_application_12bit():
    T._sao_application((12,))


# ---- extreme content ----
@pytest.mark.parametrize("B", [8, 10, 12])
def test_filters_on_overshoot_planes(B):
    """The four filters, every fraction, both signs: isLast = 1 must clip at both ends, isLast = 0 must hold the closed-form extremes."""
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 1)
    rng = np.random.default_rng(8100 + B)
    W = H = 40
    for chroma in (0, 1):
        taps, sfx = (xi.CHROMA_TAPS, "Chroma") if chroma else (xi.LUMA_TAPS, "Luma")
        n = len(taps[0])
        w, h, org = W - n, H - n, (n // 2 - 1) * W + n // 2 - 1
        below = above = at_min = at_max = 0
        for frac in range(len(taps)):
            lo, hi = xi.mid_extremes(taps[frac], B)
            for sign in (1, -1):
                for hor in (1, 0):
                    zero = taps[0]
                    plane, _ = xi.overshoot_plane(rng, W, H, B, taps[frac] if hor else zero, zero if hor else taps[frac], sign)
                    src = np.ascontiguousarray(plane).reshape(-1)
                    final, mid = xi.interp_unclipped(plane, frac if hor else 0, 0 if hor else frac, w, h, B, chroma, n // 2 - 1, n // 2 - 1)
                    for last in (0, 1):
                        a, b = np.zeros(h * w, np.int16), np.zeros(h * w, np.int16)
                        if hor:
                            getattr(R, "ref_filterHor" + sfx)(ol.ptr(src, org), W, ol.ptr(a), w, w, h, frac, last)
                            getattr(O, "hmo_filterHor" + sfx)(ol.ptr(src, org), W, ol.ptr(b), w, w, h, frac, last, B)
                        else:
                            getattr(R, "ref_filterVer" + sfx)(ol.ptr(src, org), W, ol.ptr(a), w, w, h, frac, 1, last)
                            getattr(O, "hmo_filterVer" + sfx)(ol.ptr(src, org), W, ol.ptr(b), w, w, h, frac, 1, last, B)
                        assert np.array_equal(a, b), (sfx, "hor" if hor else "ver", frac, sign, last)
                        if last:
                            assert np.array_equal(b.reshape(h, w), np.clip(final, 0, (1 << B) - 1))
                            lo_n, hi_n = xi.count_outside(final, B)
                            below, above = below + lo_n, above + hi_n
                        elif frac:
                            at_min, at_max = at_min + int((b == lo).sum()), at_max + int((b == hi).sum())
                    if hor:  # the second stage on these intermediates: (hor, frac) then (ver, every fraction)
                        m16 = np.ascontiguousarray(mid.astype(np.int16)).reshape(-1)
                        assert np.array_equal(m16.astype(np.int64), mid.reshape(-1))  # the 14-bit intermediate fits 16 bits
                        for f2 in range(len(taps)):
                            for last in (0, 1):
                                a, b = np.zeros(h * w, np.int16), np.zeros(h * w, np.int16)
                                getattr(R, "ref_filterVer" + sfx)(ol.ptr(m16, (n // 2 - 1) * w), w, ol.ptr(a), w, w, h, f2, 0, last)
                                getattr(O, "hmo_filterVer" + sfx)(ol.ptr(m16, (n // 2 - 1) * w), w, ol.ptr(b), w, w, h, f2, 0, last, B)
                                assert np.array_equal(a, b), (sfx, "second stage", frac, f2, sign, last)
        print("filters", B, sfx, dict(below=below, above=above, at_min=at_min, at_max=at_max))
        assert below > 0 and above > 0 and at_min > 0 and at_max > 0, (sfx, below, above, at_min, at_max)


def _extend(O, planes, w, h, m):
    out = []
    for k, pl in enumerate(planes):
        pw, ph, pm = (w, h, m) if k == 0 else (w // 2, h // 2, m // 2)
        st = pw + 2 * pm
        e = np.zeros((ph + 2 * pm) * st, np.int16)
        e.reshape(ph + 2 * pm, st)[pm:pm + ph, pm:pm + pw] = pl
        O.hmo_extendPicBorder(ol.ptr(e, pm * st + pm), st, pw, ph, pm, pm)
        out.append((e, st, pm))
    return out


@pytest.mark.parametrize("kind", xi.PLANE_KINDS)
@pytest.mark.parametrize("B", [8, 10, 12])
def test_pred_inter_blocks_on_extreme_planes(B, kind):
    """predInterLumaBlk / predInterChromaBlk with border extension and clipMv on constant, binary and border-line planes: every
    luma and chroma phase, vectors far outside the picture (whole windows in the margins), bi = 0 and 1."""
    R, O = ol.ref(), ol.oracle()
    w, h, m = 136, 72, 80
    R.ref_init(B, w, h, 1)
    rng = np.random.default_rng(8200 + B + len(kind))
    pl = [xi.extreme_plane(rng, pw, ph, B, kind) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))]
    R.ref_set_recon(*[np.ascontiguousarray(p).reshape(-1) for p in pl])
    planes = _extend(O, pl, w, h, m)
    ext = np.zeros((h + 2 * m) * (w + 2 * m), np.int16)
    R.ref_extended_luma(ext)
    assert np.array_equal(planes[0][0], ext)
    shapes = [(8, 4), (4, 8), (12, 16), (16, 12), (64, 64), (8, 8), (16, 4), (32, 24)]
    out = np.zeros((3, 2), np.int64)
    for it in range(96):
        pw_, ph_ = shapes[it % len(shapes)]
        px, py = int(rng.integers(0, (w - pw_) // 4 + 1)) * 4, int(rng.integers(0, (h - ph_) // 4 + 1)) * 4
        mvx, mvy = (int(v) for v in (rng.integers(-2000, 2000, 2) if it % 4 == 3 else rng.integers(-48, 48, 2)))
        if it < 64:
            mvx, mvy = (mvx & ~7) | (it & 7), (mvy & ~7) | (it >> 3)  # every chroma phase (and so every luma phase) once
        bi = it % 2
        cx, cy, rx, ry = C.c_int(mvx), C.c_int(mvy), C.c_int(mvx), C.c_int(mvy)
        O.hmo_clipMv(C.byref(cx), C.byref(cy), px, py, w, h, 64)
        R.ref_clipMv(px, py, C.byref(rx), C.byref(ry))
        assert (cx.value, cy.value) == (rx.value, ry.value)
        ref_out = [np.zeros(pw_ * ph_, np.int16), np.zeros(pw_ * ph_ // 4, np.int16), np.zeros(pw_ * ph_ // 4, np.int16)]
        R.ref_predInterBlk(px, py, pw_, ph_, mvx, mvy, bi, ref_out[0], ref_out[1], ref_out[2], 1)
        for k in range(3):
            ch = 1 if k else 0
            e, st, pm = planes[k]
            got = np.zeros((pw_ >> ch) * (ph_ >> ch), np.int16)
            (O.hmo_predInterChromaBlk if k else O.hmo_predInterLumaBlk)(ol.ptr(e, (pm + (py >> ch)) * st + pm + (px >> ch)), st, cx.value, cy.value,
                                                                        pw_, ph_, got, pw_ >> ch, bi, B)
            assert np.array_equal(ref_out[k], got), (kind, it, k, (px, py, pw_, ph_), (mvx, mvy), bi)
            final, _ = xi.interp_unclipped(e.reshape(-1, st), cx.value, cy.value, pw_ >> ch, ph_ >> ch, B, ch, pm + (px >> ch), pm + (py >> ch))
            if not bi:
                assert np.array_equal(got.reshape(final.shape), np.clip(final, 0, (1 << B) - 1))
            out[k] += xi.count_outside(final, B)
    print("pred inter", B, kind, out.tolist())
    if kind in ("binary", "border"):
        assert (out > 0).all(), out
    else:  # a constant plane: every output equals the constant, at the range end itself
        assert not out.any()


@pytest.mark.parametrize("B", [8, 10, 12])
def test_add_avg_at_the_intermediate_extremes(B):
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 1)
    rng = np.random.default_rng(8300 + B)
    lo, hi = xi.mid_extremes(xi.LUMA_TAPS[2], B)
    w, h = 16, 8
    a = [rng.choice([lo, hi, -8192, (((1 << B) - 1) << (14 - B)) - 8192], n).astype(np.int16) for n in (w * h, w * h // 4, w * h // 4)]
    b = [rng.choice([lo, hi, -8192, (((1 << B) - 1) << (14 - B)) - 8192], n).astype(np.int16) for n in (w * h, w * h // 4, w * h // 4)]
    o = [np.zeros(n, np.int16) for n in (w * h, w * h // 4, w * h // 4)]
    R.ref_addAvg(P3(*[x.ctypes.data for x in a]), P3(*[x.ctypes.data for x in b]), P3(*[x.ctypes.data for x in o]), w, h)
    below = above = 0
    for k in range(3):
        ww, hh = (w, h) if k == 0 else (w // 2, h // 2)
        ob = np.zeros(ww * hh, np.int16)
        O.hmo_addAvg(a[k], ww, b[k], ww, ob, ww, ww, hh, B)
        assert np.array_equal(o[k], ob), k
        un = (a[k].astype(np.int64) + b[k] + (1 << (14 - B)) + 2 * 8192) >> (15 - B)
        below, above = below + xi.count_outside(un, B)[0], above + xi.count_outside(un, B)[1]
    assert below > 0 and above > 0


@pytest.mark.parametrize("B", [8, 10, 12])
def test_distortion_at_opposite_ends(B):
    """calcHAD and getDistPart (SSE, HADS) with |org - cur| = maxv on every sample, both signs; me_oracle.sad on the same blocks
    against the closed form (the tap has no xGetSAD*)."""
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, 416, 240, 1)
    O.hmo_calcHAD.restype = O.hmo_getSSE.restype = C.c_uint32
    R.ref_calcHAD.restype = R.ref_getDistPart.restype = C.c_uint
    mx = (1 << B) - 1
    for (w, h) in ((4, 4), (8, 8), (64, 64), (8, 4), (4, 8), (12, 16), (16, 12), (64, 32)):
        for flip in (0, 1):
            org, cur = np.full((h, w), mx if flip else 0, np.int16), np.full((h, w), 0 if flip else mx, np.int16)
            assert int(np.abs(org.astype(np.int64) - cur).min()) == mx
            po, pc = vp(org), vp(cur)
            assert R.ref_calcHAD(po, w, pc, w, w, h) == O.hmo_calcHAD(po, w, pc, w, w, h, B), ("calcHAD", w, h)
            sse = O.hmo_getSSE(po, w, pc, w, w, h, B)
            assert R.ref_getDistPart(pc, w, po, w, w, h, 0) == sse, ("SSE", w, h)
            assert sse == ((mx * mx) >> (2 * (B - 8))) * w * h  # per sample (diff * diff) >> shift
            if w == h or (w % 8 == 0 and h % 8 == 0):
                assert R.ref_getDistPart(pc, w, po, w, w, h, 1) == O.hmo_calcHAD(po, w, pc, w, w, h, B), ("HADS", w, h)
            for s in (0, 1) if h > 8 else (0,):
                assert mo.sad(org, cur, s, B) == (((w * (h >> s) * mx) << s) & mo.M32) >> (B - 8)
    assert mo.sad(np.zeros((64, 64)), np.full((64, 64), 4095), 0, 12) == (64 * 64 * 4095) >> 4


@pytest.mark.parametrize("w,h", [(128, 64), (192, 128)])  # whole CTUs: the tap drives the reference's edge filters CTU by CTU
@pytest.mark.parametrize("B", [8, 10, 12])
def test_deblock_on_edge_content(B, w, h):
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, w, h, 1)
    rng = np.random.default_rng(8400 + B + w)
    total = np.zeros((2, 2), np.int64)
    for use_nof, boff, toff in ((True, 0, 0), (False, -6, 6), (True, 6, -6)):
        d = xi.dbk_edge_content(rng, w, h, B)
        y, cb, cr = d["planes"]
        R.ref_set_recon(y.reshape(-1), cb.reshape(-1), cr.reshape(-1))
        ry, rcb, rcr = np.zeros_like(y), np.zeros_like(cb), np.zeros_like(cr)
        R.ref_deblock_picture(vp(d["bsv"]), vp(d["bsh"]), vp(d["qp"]), vp(d["nof"]) if use_nof else None, boff, toff, vp(ry), vp(rcb), vp(rcr))
        out = [p.copy() for p in d["planes"]]
        O.hmo_deblock_picture(P3(*[p.ctypes.data for p in out]), I3(w, w // 2, w // 2), w, h, B, vp(d["bsv"]), vp(d["bsh"]), vp(d["qp"]),
                              vp(d["nof"]) if use_nof else None, boff, toff)
        for k, (a, b) in enumerate(zip((ry, rcb, rcr), out)):
            assert np.array_equal(a, b), (k, boff, toff, np.argwhere(a != b)[:3])
        assert (out[0] != y).sum() > 200 and (out[1] != cb).sum() > 50
        cnt = xi.dbk_count_outside(d, w, h, B, use_nof, boff, toff)
        total += np.array([cnt["luma"], cnt["chroma"]])
    print("deblock edge content", B, (w, h), "luma (below, above), chroma (below, above):", total.tolist())
    assert (total > 0).all(), total


@pytest.mark.parametrize("w,h", [(136, 72), (200, 136)])
@pytest.mark.parametrize("B", [8, 10, 12])
def test_sao_on_edge_content(B, w, h):
    R, O = ol.ref(), ol.oracle()
    R.ref_init(B, w, h, 1)
    rng = np.random.default_rng(8500 + B + w)
    n_lcu = -(-w // 64) * -(-h // 64)
    pl = xi.sao_edge_content(rng, w, h, B)
    prm = T._sao_params(rng, n_lcu)
    for c in range(3):
        prm["type"][c, rng.permutation(n_lcu)[:6]] = np.arange(-1, 5)
    R.ref_set_recon(*[p.reshape(-1) for p in pl])
    r = [np.zeros_like(p) for p in pl]
    R.ref_sao_picture(vp(prm), n_lcu, vp(r[0]), vp(r[1]), vp(r[2]))
    o = [np.zeros_like(p) for p in pl]
    O.hmo_sao_picture(P3(*[p.ctypes.data for p in pl]), P3(*[p.ctypes.data for p in o]), I3(w, w // 2, w // 2), w, h, B, 64,
                      P3(prm[0].ctypes.data, prm[1].ctypes.data, prm[2].ctypes.data))
    unc, add = xi.sao_unclipped(pl, prm, w, h, B)
    for k in range(3):
        assert np.array_equal(r[k], o[k]), (k, np.argwhere(r[k] != o[k])[:3])
        below, above = xi.count_outside(unc[k], B)
        print("sao edge content", B, (w, h), k, dict(below=below, above=above))
        assert below > 0 and above > 0, (k, below, above)
        if B == 12:  # the offsets are scaled by 1 << (B - 10)
            inside = (unc[k] >= 0) & (unc[k] < (1 << B)) & (add[k] != 0)
            assert inside.any() and np.array_equal((o[k].astype(np.int64) - pl[k])[inside], 4 * add[k][inside])


def test_me_and_sao_stats_oracles_at_12bit_opposite_ends():
    """No tap of the reference for these: the vectorised yardsticks against their literal restatements at 12 bit, with original
    and reference (org and rec) at opposite range ends, and the closed forms."""
    B, mx = 12, 4095
    full, zero = xi.opposite_ends(72, 40, B)
    for lcu_based in (0, 1):
        a, b = so.stats_vec(full, zero, 72, 40, 32, B, lcu_based), so.stats_loop(full, zero, 72, 40, 32, B, lcu_based)
        assert np.array_equal(a, b)
        assert (a[..., 0] == a[..., 1] * mx).all() and a[..., 0].max() == (32 * 32 if not lcu_based else 27 * 28) * mx
        assert np.array_equal(so.stats_vec(zero, full, 72, 40, 32, B, lcu_based), so.stats_loop(zero, full, 72, 40, 32, B, lcu_based))
    M = 8
    ref = np.zeros((64 + 2 * M, 64 + 2 * M), np.int16)
    org = np.full((64, 64), mx, np.int16)
    for (w, h, s) in ((64, 64, 0), (64, 64, 1), (4, 4, 0)):
        u = dict(x=0, y=0, w=w, h=h, sub_shift=s, pred_x=3, pred_y=-2, left=-2, top=-1, right=1, bottom=2)
        (mvx, mvy, sad, cost), cmap = mo.search(org, ref, (M, M), u, 70000, B)
        loop, costs = mo.search_loop(org, ref, (M, M), u, 70000, B)
        assert (mvx, mvy, sad, cost) == loop and cmap.reshape(-1).tolist() == costs
        assert sad == (w * h * mx) >> 4
