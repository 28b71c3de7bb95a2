"""libhmx against the CPU oracle on the inter path and the loop filters at 12 bit and at the range ends (8, 10 and 12 bit):
the scalar interpolation filters and block prediction, hmx_motionCompensation, hmx_batch_motionCompensation[_multi] in both
schedules, weighted prediction, the costs and the integer motion search, deblocking, SAO and the SAO statistics.  The content
comes from tests/extreme_inputs.py; tests/test_oracle_vs_ref_sample_edges.py pins the oracle to the compiled reference on the
same content.  Every comparison is for equality, and every case on extreme content asserts (> 0), with the int64 restatements
of extreme_inputs, that the edge it is about was reached.  The bit-depth-generic cases of test_gpu_wp, test_gpu_me,
test_gpu_loop_multi and test_gpu_sao_stats run here on a 12-bit context (their full-size cases stay at 8 and 10 bit); the 12-bit
vectors of the compiled reference are tests/test_golden.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

import extreme_inputs as xi
import me_oracle as mo
import oracle_lib as ol
import test_gpu_loop_multi as tl
import test_gpu_me as tm
import test_gpu_sao_stats as ts
import test_gpu_wp as tw
import wp_oracle as wo
from sao_stats_oracle import stats_vec
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu
P3, I3 = C.c_void_p * 3, C.c_int * 3
SIZES = [(136, 72), (200, 136)]  # cut CTUs, plane widths that are no multiple of 8, a cell map that is no multiple of 16 cells wide
MARGIN = 80


@pytest.fixture(scope="module", params=[8, 10, 12])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx12():
    c = capi.Context(bit_depth=12)
    yield c
    c.close()


# ---- a. scalar filters and block prediction -------------------------------------------------------------------------------------
def test_scalar_filters_on_overshoot_planes(ctx):
    O, B = ol.oracle(), ctx.bit_depth
    rng = np.random.default_rng(9100 + B)
    W = H = 40
    for chroma in (0, 1):
        taps, sfx = (xi.CHROMA_TAPS, "Chroma") if chroma else (xi.LUMA_TAPS, "Luma")
        n = len(taps[0])
        w, h, org = W - n, H - n, (n // 2 - 1) * W + n // 2 - 1
        at_zero = at_max = at_lo = at_hi = 0
        for frac in range(len(taps)):
            lo, hi = xi.mid_extremes(taps[frac], B)
            for sign in (1, -1):
                for hor in (1, 0):
                    plane, _ = xi.overshoot_plane(rng, W, H, B, taps[frac] if hor else taps[0], taps[0] if hor else taps[frac], sign)
                    src = np.ascontiguousarray(plane).reshape(-1)
                    final, mid = xi.interp_unclipped(plane, frac if hor else 0, 0 if hor else frac, w, h, B, chroma, n // 2 - 1, n // 2 - 1)
                    name = ("filterHor" if hor else "filterVer") + sfx
                    for last in (0, 1):
                        want = np.zeros(h * w, np.int16)
                        if hor:
                            getattr(O, "hmo_" + name)(ol.ptr(src, org), W, ol.ptr(want), w, w, h, frac, last, B)
                            got = ctx.filter(name, src, org, W, w, w, h, frac, is_last=last)
                        else:
                            getattr(O, "hmo_" + name)(ol.ptr(src, org), W, ol.ptr(want), w, w, h, frac, 1, last, B)
                            got = ctx.filter(name, src, org, W, w, w, h, frac, is_first=1, is_last=last)
                        assert np.array_equal(got.reshape(-1)[:h * w], want), (name, frac, sign, last, np.argwhere(got.reshape(-1)[:h * w] != want)[:3])
                        if last:
                            out = (final < 0) | (final > (1 << B) - 1)
                            at_zero += int(((want.reshape(h, w) == 0) & out).sum())
                            at_max += int(((want.reshape(h, w) == (1 << B) - 1) & out).sum())
                        elif frac:
                            at_lo, at_hi = at_lo + int((got.reshape(-1)[:h * w] == lo).sum()), at_hi + int((got.reshape(-1)[:h * w] == hi).sum())
                    if hor:  # the second stage on the first stage's intermediates, every fraction, isLast 0 and 1
                        m16 = np.ascontiguousarray(mid.astype(np.int16)).reshape(-1)
                        for f2 in range(len(taps)):
                            for last in (0, 1):
                                want = np.zeros(h * w, np.int16)
                                getattr(O, "hmo_filterVer" + sfx)(ol.ptr(m16, (n // 2 - 1) * w), w, ol.ptr(want), w, w, h, f2, 0, last, B)
                                got = ctx.filter("filterVer" + sfx, m16, (n // 2 - 1) * w, w, w, w, h, f2, is_first=0, is_last=last)
                                assert np.array_equal(got.reshape(-1)[:h * w], want), ("second stage", sfx, frac, f2, sign, last)
        print("scalar filters", B, sfx, dict(clipped_at_0=at_zero, clipped_at_max=at_max, mid_at_min=at_lo, mid_at_max=at_hi))
        assert at_zero > 0 and at_max > 0 and at_lo > 0 and at_hi > 0


def host_pic(planes, m):
    """a capi.Pic over host planes that include margins (luma margin m, chroma m / 2)"""
    p = capi.Pic()
    for k, a in enumerate(planes):
        mk = m >> (1 if k else 0)
        p.plane[k], p.stride[k] = a.ctypes.data + 2 * (mk * a.shape[1] + mk), a.shape[1]
    return p


@functools.lru_cache(maxsize=None)
def host_refs(B):
    """Two reference pictures 96 x 80 with margin 24 whose every sample, margins included, is 0 or 2^B - 1."""
    rng = np.random.default_rng(9200 + B)
    W, H, M = 96, 80, 24
    refs = [[np.ascontiguousarray(xi.extreme_plane(rng, (W >> ch) + 2 * (M >> ch), (H >> ch) + 2 * (M >> ch), B, "binary")) for ch in (0, 1, 1)] for _ in range(2)]
    for r in refs:
        for p in r:
            p.setflags(write=False)
    return refs, W, H, M


def oracle_blk(O, plane, st, m, x, y, w, h, mvx, mvy, bi, B, ch):
    t = np.zeros((h >> ch, w >> ch), np.int16)
    (O.hmo_predInterChromaBlk if ch else O.hmo_predInterLumaBlk)(ol.ptr(plane.reshape(-1), (m + (y >> ch)) * st + m + (x >> ch)), st, mvx, mvy, w, h,
                                                                 t.reshape(-1), w >> ch, bi, B)
    return t


AMP = [(8, 4), (4, 8), (12, 16), (16, 12), (64, 64)]


def test_block_prediction_and_one_unit(ctx):
    """hmx_xPredInterLumaBlk / ChromaBlk (bi 0 and 1) and hmx_motionCompensation (uni, list 1 only, bi): all 16 luma phases (and 16
    of the chroma phases through them, the others through odd vectors), AMP shapes, on binary planes."""
    O, B, L = ol.oracle(), ctx.bit_depth, capi.lib()
    refs, W, H, M = host_refs(B)
    rng = np.random.default_rng(9210 + B)
    mx = (1 << B) - 1
    clipped = np.zeros((2, 2), np.int64)  # [luma, chroma][at 0, at maxv]
    for it in range(40):
        w, h = AMP[it % len(AMP)]
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mv = [[int(v) for v in rng.integers(-4 * (M - 8), 4 * (M - 8) + 1, 2)] for _ in range(2)]
        if it < 32:
            mv[0] = [(mv[0][0] & ~3) | (it & 3), (mv[0][1] & ~3) | ((it >> 2) & 3)]  # every luma phase, twice
        use = [(1, 0), (0, 1), (1, 1)][it % 3]
        for bi in (0, 1):
            for k in (0, 1):
                pl, st, mk = refs[0][k], refs[0][k].shape[1], M >> k
                want = oracle_blk(O, pl, st, mk, x, y, w, h, mv[0][0], mv[0][1], bi, B, k)
                got = np.zeros((h >> k, (w >> k) + 3), np.int16)
                fn = L.hmx_xPredInterChromaBlk if k else L.hmx_xPredInterLumaBlk
                ctx._chk(fn(ctx.h, pl.ctypes.data + 2 * ((mk + (y >> k)) * st + mk + (x >> k)), st, mv[0][0], mv[0][1], w, h, got.ctypes.data, (w >> k) + 3, bi))
                assert np.array_equal(got[:, :w >> k], want), ("blk", "chroma" if k else "luma", it, (x, y, w, h), mv[0], bi, np.argwhere(got[:, :w >> k] != want)[:3])
                final, mid = xi.interp_unclipped(pl, mv[0][0], mv[0][1], w >> k, h >> k, B, k, mk + (x >> k), mk + (y >> k))
                if not bi:
                    clipped[k] += (int(((want == 0) & (final < 0)).sum()), int(((want == mx) & (final > mx)).sum()))
        dst = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        dp = capi.Pic()
        for k in range(3):
            dp.plane[k], dp.stride[k] = dst[k].ctypes.data, dst[k].shape[1]
        r0, r1 = host_pic(refs[0], M), host_pic(refs[1], M)
        m0, m1 = (C.c_int * 2)(*mv[0]), (C.c_int * 2)(*mv[1])
        ctx._chk(L.hmx_motionCompensation(ctx.h, C.byref(r0) if use[0] else None, m0 if use[0] else None, C.byref(r1) if use[1] else None,
                                          m1 if use[1] else None, x, y, w, h, C.byref(dp)))
        both = int(use[0] and use[1])
        for k in range(3):
            ch = 1 if k else 0
            parts = [oracle_blk(O, refs[l][k], refs[l][k].shape[1], M >> ch, x, y, w, h, mv[l][0], mv[l][1], both, B, ch) for l in range(2) if use[l]]
            want = parts[0]
            if both:
                want = np.zeros_like(parts[0])
                O.hmo_addAvg(parts[0].reshape(-1), w >> ch, parts[1].reshape(-1), w >> ch, want.reshape(-1), w >> ch, w >> ch, h >> ch, B)
            assert np.array_equal(dst[k], want), ("motionCompensation", it, k, use, (x, y, w, h), mv)
    print("block prediction", B, "clipped [luma, chroma][at 0, at maxv]", clipped.tolist())
    assert (clipped > 0).all()
    # bi = 1 on a horizontal half-sample vector over an overshoot plane: the intermediate at its closed-form extremes
    lo, hi = xi.mid_extremes(xi.LUMA_TAPS[2], B)
    assert hi == ((88 * mx) >> (B - 8)) - 8192 and lo == ((-24 * mx) >> (B - 8)) - 8192
    for sign, value in ((1, hi), (-1, lo)):
        plane, pos = xi.overshoot_plane(rng, 48, 40, B, xi.LUMA_TAPS[2], xi.LUMA_TAPS[0], sign)
        plane = np.ascontiguousarray(plane)
        got = np.zeros((16, 32), np.int16)
        ctx._chk(L.hmx_xPredInterLumaBlk(ctx.h, plane.ctypes.data + 2 * (8 * 48 + 8), 48, 2, 0, 32, 16, got.ctypes.data, 32, 1))
        assert np.array_equal(got, oracle_blk(O, plane, 48, 8, 0, 0, 32, 16, 2, 0, 1, B, 0))
        assert (got.min() if sign < 0 else got.max()) == value and any(got[y - 8, x - 8] == value for x, y in pos if 8 <= x < 40 and 8 <= y < 24)


# ---- c. batch motion compensation -----------------------------------------------------------------------------------------------
def pu_list(w, h, seed, n_refs, bi_mode="mixed"):
    """Units that tile the picture, built so that every path of the cell kernel occurs: heights 4 and 12 (4x4 cells whose lane
    partner belongs to another unit) beside heights >= 8 (merged 4x8 cells), widths 4 and 12, integer displacements of both parities
    in x (the window starts on either half of a dword, luma and chroma), every chroma phase and with them every luma phase ((0, 0),
    (f, 0) and (0, f) included), vectors at the clipMv limits (whole windows in the margins).  bi_mode: "uni" = no unit uses both lists (3 of 5 list 0 only, 2 of 5 list 1 only), "mixed" =
    list 0 only, list 1 only and both (2 : 1 : 2), "bi" = every unit uses both."""
    O = ol.oracle()
    rng = np.random.default_rng(seed)
    parts = [[(0, 0, 16, 16)], [(0, 0, 16, 8), (0, 8, 16, 8)], [(0, 0, 8, 16), (8, 0, 8, 16)], [(0, 0, 8, 8), (8, 0, 8, 8), (0, 8, 8, 8), (8, 8, 8, 8)],
             [(0, 0, 16, 12), (0, 12, 16, 4)], [(0, 0, 16, 4), (0, 4, 16, 12)], [(0, 0, 12, 16), (12, 0, 4, 16)], [(0, 0, 4, 16), (4, 0, 12, 16)],
             [(0, 0, 8, 4), (0, 4, 8, 4), (8, 0, 4, 8), (12, 0, 4, 8), (0, 8, 8, 8), (8, 8, 8, 4), (8, 12, 8, 4)]]
    rects = []
    for by in range(0, h, 16):
        for bx in range(0, w, 16):
            if bx + 16 <= w and by + 16 <= h:
                rects += [(bx + x, by + y, pw, ph) for x, y, pw, ph in parts[(bx // 16 + 3 * (by // 16)) % len(parts)]]
            else:  # the cut column and row: 8x8, 8x4 and 4x8
                for y in range(by, min(by + 16, h), 8):
                    for x in range(bx, min(bx + 16, w), 8):
                        k = (x // 8 + y // 8) % 3
                        rects += [(x, y, 8, 8)] if k == 0 else [(x, y, 8, 4), (x, y + 4, 8, 4)] if k == 1 else [(x, y, 4, 8), (x + 4, y, 4, 8)]
    pus = np.zeros(len(rects), ol.PU_DTYPE)
    for i, (x, y, pw, ph) in enumerate(rects):
        mv = []
        for l in range(2):
            ph8 = (i * 5 + 29 * l) % 64  # every chroma phase within 64 consecutive units, both lists
            ix, iy = int(rng.integers(-9, 10)), int(rng.integers(-9, 10))
            mvx, mvy = (ix << 3) | (ph8 & 7), (iy << 3) | (ph8 >> 3)  # luma: integer part 2 * ix + (phase >> 2), both parities; chroma: ix
            if i % 11 == 5 + l:  # far outside: clipMv brings it to its limit, the window lies in the margin
                cx, cy = C.c_int(int(rng.choice([-4000, 4000])) + (ph8 & 3)), C.c_int(int(rng.choice([-4000, 4000, 0])) + (ph8 >> 3 & 3))
                O.hmo_clipMv(C.byref(cx), C.byref(cy), x, y, w, h, 64)
                mvx, mvy = cx.value, cy.value
            mv.append((mvx, mvy))
        kind = i % 5  # 0, 1: list 0; 2: list 1 only; 3, 4: both
        kind = 3 if bi_mode == "bi" else (kind, 2, 0)[kind - 2] if bi_mode == "uni" and kind > 2 else kind
        r0, r1 = (255 if kind == 2 else i % n_refs), (255 if kind < 2 else (i + 1) % n_refs)
        pus[i] = (x, y, pw, ph, r0, r1, mv[0][0], mv[0][1], mv[1][0], mv[1][1])
    return pus


def ext_planes(O, planes, w, h, m):
    """what hmx_pic_extend_border makes of a picture, from the oracle: flat arrays with margins"""
    out = []
    for k, pl in enumerate(planes):
        pw, ph, pm = (w, h, m) if k == 0 else (w // 2, h // 2, m // 2)
        e = np.zeros((ph + 2 * pm, pw + 2 * pm), np.int16)
        e[pm:pm + ph, pm:pm + pw] = pl
        O.hmo_extendPicBorder(ol.ptr(e.reshape(-1), pm * (pw + 2 * pm) + pm), pw + 2 * pm, pw, ph, pm, pm)
        out.append(e)
    return out


def oracle_mc(O, pus, ext, w, h, m, B):
    dst = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
    ptrs = (C.c_void_p * (3 * len(ext)))()
    for i, e in enumerate(ext):
        for p in range(3):
            pm = m >> (1 if p else 0)
            ptrs[i * 3 + p] = e[p].ctypes.data + 2 * (pm * e[p].shape[1] + pm)
    t = np.ascontiguousarray(pus, ol.PU_DTYPE)
    O.hmo_mc_frame(t.ctypes.data, len(t), B, ptrs, I3(w + 2 * m, w // 2 + m, w // 2 + m), P3(*[d.ctypes.data for d in dst]), I3(w, w // 2, w // 2))
    return dst


def count_mc_clips(pus, ext, m, B):
    """[luma, chroma][below 0, above maxv]: unclipped outputs of the units that use one list"""
    n = np.zeros((2, 2), np.int64)
    for u in pus:
        for r, mvx, mvy in ((int(u["ref0"]), int(u["mv0x"]), int(u["mv0y"])), (int(u["ref1"]), int(u["mv1x"]), int(u["mv1y"]))):
            if r == 255 or (u["ref0"] != 255 and u["ref1"] != 255):
                continue
            for k in range(3):
                ch = 1 if k else 0
                final, _ = xi.interp_unclipped(ext[r][k], mvx, mvy, int(u["w"]) >> ch, int(u["h"]) >> ch, B, ch, (m >> ch) + (int(u["x"]) >> ch), (m >> ch) + (int(u["y"]) >> ch))
                n[ch] += xi.count_outside(final, B)
    return n


def window_in_margin(u, l, w, h):
    """whether list l's luma window of unit u, its 8 filter taps included, lies wholly outside the picture"""
    X, Y = int(u["x"]) + (int(u[f"mv{l}x"]) >> 2), int(u["y"]) + (int(u[f"mv{l}y"]) >> 2)
    return int(u[f"ref{l}"]) != 255 and (X + int(u["w"]) + 4 <= 0 or X - 3 >= w or Y + int(u["h"]) + 4 <= 0 or Y - 3 >= h)


def mc_scene(B, w, h, kind, bi_mode="mixed"):
    O = ol.oracle()
    rng = np.random.default_rng(9300 + B + w)
    if kind == "texture":
        pics = [workload.make_planes(60 + i, w, h, B) for i in range(2)]
    else:
        pics = [[xi.extreme_plane(rng, pw, ph, B, ("binary", "border")[i]) for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2))] for i in range(2)]
    ext = [ext_planes(O, p, w, h, MARGIN) for p in pics]
    pus = pu_list(w, h, 9310 + w, 2, bi_mode)
    return pics, ext, pus


@pytest.mark.parametrize("bi_mode", ["uni", "mixed", "bi"])
@pytest.mark.parametrize("w,h", SIZES)
def test_batch_motion_compensation(ctx, w, h, bi_mode):
    """binary and border-line references; no, some and all units bi-predicted"""
    batch_mc(ctx, w, h, "extreme", bi_mode)


@pytest.mark.parametrize("w,h", SIZES)
def test_batch_motion_compensation_texture_12bit(ctx12, w, h):
    """workload.make_planes at 12 bit (random content at 8 and 10 bit is tests/test_gpu_parity.py's)"""
    batch_mc(ctx12, w, h, "texture", "mixed")


def batch_mc(ctx, w, h, kind, bi_mode):
    O, B, L = ol.oracle(), ctx.bit_depth, capi.lib()
    pics, ext, pus = mc_scene(B, w, h, kind, bi_mode)
    assert {4, 8, 12, 16} <= set(pus["h"]) and {4, 8, 12, 16} <= set(pus["w"])
    assert {(int(u["mv0x"]) & 7, int(u["mv0y"]) & 7) for u in pus} | {(int(u["mv1x"]) & 7, int(u["mv1y"]) & 7) for u in pus} == {(a, b) for a in range(8) for b in range(8)}
    assert {(int(u["mv0x"]) >> 2) & 1 for u in pus} == {0, 1} and {(int(u["mv0x"]) >> 3) & 1 for u in pus} == {0, 1}
    l1_only, both = (pus["ref0"] == 255) & (pus["ref1"] != 255), (pus["ref0"] != 255) & (pus["ref1"] != 255)
    assert (l1_only.any(), both.any(), both.all()) == dict(uni=(True, False, False), mixed=(True, True, False), bi=(False, True, True))[bi_mode]
    n_margin = sum(window_in_margin(u, l, w, h) for u in pus for l in (0, 1))
    assert n_margin > 0  # vectors at the clipMv limits: whole windows in the margins
    counts = [len(pus), 2 * len(pus) // 3]  # two jobs of unequal length
    want = [oracle_mc(O, pus[:n], ext, w, h, MARGIN, B) for n in counts]
    if kind == "extreme":
        mx = (1 << B) - 1
        if bi_mode != "bi":  # the counter restates the uni-predicted output
            n_clip = count_mc_clips(pus, ext, MARGIN, B)
            print("batch mc", B, (w, h), bi_mode, "windows in the margin", n_margin, "unclipped outputs outside [luma, chroma][below, above]", n_clip.tolist())
            assert (n_clip > 0).all()
        assert all((want[0][p] == 0).any() and (want[0][p] == mx).any() for p in range(3))
    d_refs = [capi.DevPicture(ctx, w, h, MARGIN, MARGIN).upload(p) for p in pics]
    for d in d_refs:
        ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(d.as_pic()), w, h, MARGIN, MARGIN))
    ctx.sync()
    for i, d in enumerate(d_refs):
        for p, a in enumerate(d.download(with_margins=True)):
            assert np.array_equal(a, ext[i][p]), ("border", i, p)
    ref_arr = (capi.Pic * 2)(*[d.as_pic() for d in d_refs])
    d_pus = ctx.to_device(pus)
    for mapped in (True, False):
        dst = [capi.DevPicture(ctx, w, h).zero() for _ in counts]
        dst_pics = (capi.Pic * 2)(*[d.as_pic() for d in dst])
        jobs = (capi.McJob * 2)()
        for q, n in enumerate(counts):
            jobs[q].d_pus, jobs[q].n_pus, jobs[q].refs, jobs[q].n_refs = d_pus.ptr, n, ref_arr, 2
            jobs[q].dst, jobs[q].pic_w, jobs[q].pic_h = C.pointer(dst_pics[q]), (w if mapped else 0), (h if mapped else 0)
        ctx._chk(L.hmx_batch_motionCompensation_multi(ctx.h, 2, jobs))
        ctx.sync()
        for q in range(2):
            got = dst[q].download()
            for p in range(3):
                if not np.array_equal(got[p], want[q][p]):
                    yx = np.argwhere(got[p] != want[q][p])[0]
                    sh = 1 if p else 0
                    u = [t for t in pus[:counts[q]] if t["x"] >> sh <= yx[1] < (t["x"] + t["w"]) >> sh and t["y"] >> sh <= yx[0] < (t["y"] + t["h"]) >> sh]
                    pytest.fail(f"{'cell map' if mapped else 'wave per PU'}, job {q}, plane {p}, (y, x) = {yx.tolist()}: got {got[p][tuple(yx)]}, want "
                                f"{want[q][p][tuple(yx)]}; unit {u}; luma phases {[(int(t['mv0x']) & 3, int(t['mv0y']) & 3) for t in u]}, window parity "
                                f"{[((int(t['x']) >> sh) + (int(t['mv0x']) >> (2 + sh))) & 1 for t in u]}")
        for d in dst:
            d.free()
    one = capi.DevPicture(ctx, w, h).zero()  # the single-job entry: one wave per PU
    ctx._chk(L.hmx_batch_motionCompensation(ctx.h, d_pus.ptr, len(pus), ref_arr, 2, C.byref(one.as_pic())))
    ctx.sync()
    assert all(np.array_equal(a, b) for a, b in zip(one.download(), want[0]))
    for d in d_refs + [one, d_pus]:
        d.free()


# ---- d. weighted prediction -----------------------------------------------------------------------------------------------------
def test_weighted_scalar_entries_at_the_extremes(ctx):
    """hmx_addWeightUni / Bi over weights {-128, -1, 0, 1, 255}, offsets {-128, 127}, log2_denom {0, 7} on intermediates at the
    extremes of the half-sample filter and of the copy."""
    B = ctx.bit_depth
    mx = (1 << B) - 1
    lo, hi = xi.mid_extremes(xi.LUMA_TAPS[2], B)
    vals = np.array([lo, hi, -8192, (mx << (14 - B)) - 8192, 0, -1], np.int16)
    a = np.ascontiguousarray(np.resize(vals, 64).reshape(8, 8))  # 8 x 8 of the six values; b: every pair of them
    b = np.ascontiguousarray(a.T)
    at = np.zeros((2, 2), np.int64)
    for w0 in (-128, -1, 0, 1, 255):
        for o0 in (-128, 127):
            for d in (0, 7):
                want = wo.weight_uni_vec(a, w0, o0, d, B)
                assert np.array_equal(ctx.addWeightUni(a, 8, 8, w0, o0, d).reshape(8, 8), want), ("uni", w0, o0, d)
                at[0] += ((want == 0).sum(), (want == mx).sum())
                for w1, o1 in ((-128, -128), (255, 127), (1, -128), (-1, 127), (0, 127)):
                    want = wo.weight_bi_vec(a, b, w0, w1, o0, o1, d, B)
                    assert np.array_equal(ctx.addWeightBi(a, b, 8, 8, w0, w1, o0, o1, d).reshape(8, 8), want), ("bi", w0, w1, o0, o1, d)
                    at[1] += ((want == 0).sum(), (want == mx).sum())
    assert (at > 0).all(), at


def test_weighted_one_unit_on_binary_planes(ctx):
    """hmx_motionCompensation_wp, one and two lists, extreme weights, references of 0 and 2^B - 1."""
    B = ctx.bit_depth
    refs, W, H, M = host_refs(B)
    rng = np.random.default_rng(9400 + B)
    mx = (1 << B) - 1
    ends = np.zeros(2, np.int64)
    for it in range(15):
        w, h = AMP[it % len(AMP)]
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mv = [[int(v) for v in rng.integers(-4 * (M - 8), 4 * (M - 8) + 1, 2)] for _ in range(2)]
        use = [(1, 0), (0, 1), (1, 1)][it % 3]
        den = [(0, 7)[it & 1]] * 3
        e = [([int(rng.choice([-128, -1, 0, 1, 255])) for _ in range(3)], [int(rng.choice([-128, 127])) for _ in range(3)], den) for _ in range(2)]
        pus = np.zeros(1, ol.PU_DTYPE)
        pus[0] = (x, y, w, h, 0 if use[0] else 255, 1 if use[1] else 255, mv[0][0], mv[0][1], mv[1][0], mv[1][1])
        want = wo.mc_frame_wp(pus, [(refs[0], M), (refs[1], M)], ([e[0], e[0]], [e[1], e[1]]), B)
        dst = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        dp = capi.Pic()
        for k in range(3):
            dp.plane[k], dp.stride[k] = dst[k].ctypes.data, dst[k].shape[1]
        ctx.motion_compensation_wp(host_pic(refs[0], M) if use[0] else None, mv[0], host_pic(refs[1], M) if use[1] else None, mv[1], x, y, w, h, dp,
                                   capi.wp_entry(*e[0]) if use[0] else None, capi.wp_entry(*e[1]) if use[1] else None)
        for k in range(3):
            ch = 1 if k else 0
            blk = want[k][y >> ch:(y + h) >> ch, x >> ch:(x + w) >> ch]
            assert np.array_equal(dst[k], blk), ("motionCompensation_wp", it, k, use, e, (x, y, w, h), mv)
            ends += ((blk == 0).sum(), (blk == mx).sum())
    assert (ends > 0).all()


WP_WEIGHTS, WP_OFFSETS = (-128, -1, 0, 1, 255), (-128, 127)


def wp_extreme_tables():
    """Two table sets (list 0, list 1) x two references: over the eight entries every weight of WP_WEIGHTS and both offsets occur in
    every component, next to each other within a set; one denominator per component and set (the bi formula reads list 0's)."""
    tabs = []
    for t, denoms in enumerate(([0, 7, 0], [7, 0, 7])):
        tabs.append(tuple([([WP_WEIGHTS[(3 * (4 * t + 2 * l + r) + c + 4) % 5] for c in range(3)], [WP_OFFSETS[(t + l + r + c) & 1] for c in range(3)], denoms)
                           for r in range(2)] for l in range(2)))
    for c in range(3):
        assert {e[0][c] for t in tabs for l in t for e in l} == set(WP_WEIGHTS) and {e[1][c] for t in tabs for l in t for e in l} == set(WP_OFFSETS)
    return tabs


@pytest.mark.parametrize("w,h", SIZES)
def test_weighted_batch_on_extreme_planes(ctx, w, h):
    """hmx_batch_motionCompensation_wp_multi, both schedules, on binary and border-line references with the unit lists of the
    unweighted test: per reference and list a table entry drawn from weights {-128, -1, 0, 1, 255}, offsets {-128, 127} and
    log2_denom {0, 7}; three jobs of unequal length in one call, the middle one with NULL tables."""
    O, B, L = ol.oracle(), ctx.bit_depth, capi.lib()
    mx = (1 << B) - 1
    pics, ext, pus = mc_scene(B, w, h, "extreme")
    tabs = wp_extreme_tables()
    counts = [len(pus), 2 * len(pus) // 3, len(pus) // 2]
    refs_m = [(e, MARGIN) for e in ext]
    want = [wo.mc_frame_wp(pus[:counts[0]], refs_m, tabs[0], B), oracle_mc(O, pus[:counts[1]], ext, w, h, MARGIN, B), wo.mc_frame_wp(pus[:counts[2]], refs_m, tabs[1], B)]
    ends = [int((want[0][p] == e).sum() + (want[2][p] == e).sum()) for p in range(3) for e in (0, mx)]
    print("batch wp", B, (w, h), "outputs of the weighted jobs at [Y 0, Y maxv, Cb 0, Cb maxv, Cr 0, Cr maxv]", ends)
    assert min(ends) > 0
    assert all(0 < int(((want[q][p] > 0) & (want[q][p] < mx)).sum()) for q in (0, 2) for p in range(3))  # and not every output is a clip
    d_refs = [capi.DevPicture(ctx, w, h, MARGIN, MARGIN).upload(p) for p in pics]
    for d in d_refs:
        ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(d.as_pic()), w, h, MARGIN, MARGIN))
    ref_arr = (capi.Pic * 2)(*[d.as_pic() for d in d_refs])
    d_pus = ctx.to_device(pus)
    for mapped in (True, False):
        dst = [capi.DevPicture(ctx, w, h).zero() for _ in counts]
        dst_pics = (capi.Pic * 3)(*[d.as_pic() for d in dst])
        jobs = (capi.McJob * 3)()
        for q, n in enumerate(counts):
            jobs[q].d_pus, jobs[q].n_pus, jobs[q].refs, jobs[q].n_refs = d_pus.ptr, n, ref_arr, 2
            jobs[q].dst, jobs[q].pic_w, jobs[q].pic_h = C.pointer(dst_pics[q]), (w if mapped else 0), (h if mapped else 0)
        ctx.batch_motion_compensation_wp(jobs, [tuple(tw.table(t) for t in tabs[0]), None, tuple(tw.table(t) for t in tabs[1])])
        ctx.sync()
        for q in range(3):
            got = dst[q].download()
            for p in range(3):
                if not np.array_equal(got[p], want[q][p]):
                    yx = np.argwhere(got[p] != want[q][p])[0]
                    sh = 1 if p else 0
                    u = [t for t in pus[:counts[q]] if t["x"] >> sh <= yx[1] < (t["x"] + t["w"]) >> sh and t["y"] >> sh <= yx[0] < (t["y"] + t["h"]) >> sh]
                    pytest.fail(f"{'cell map' if mapped else 'wave per PU'}, job {q} ({'unweighted' if q == 1 else tabs[q // 2]}), plane {p}, (y, x) = {yx.tolist()}: "
                                f"got {got[p][tuple(yx)]}, want {want[q][p][tuple(yx)]}; unit {u}")
        for d in dst:
            d.free()
    for d in d_refs + [d_pus]:
        d.free()


def test_weighted_12bit(ctx12):
    """tests/test_gpu_wp.py at 12 bit: the scalar entries (the hand-computed 12-bit clip cases of wp_oracle.CLIP_CASES among them),
    one unit, and the batch entry on both schedules with the mixed weighted / unweighted call."""
    for w, h in [(4, 4), (8, 4), (4, 8), (16, 12), (32, 32), (64, 64)]:
        tw.test_scalar_entries_vs_oracle(ctx12, w, h)
    assert sum(c[0] == 12 for c in wo.CLIP_CASES) >= 8
    tw.test_scalar_entries_at_the_clips(ctx12)
    tw.test_motion_compensation_wp_one_unit(ctx12)
    for mapped in (True, False):
        tw.test_batch_vs_oracle(ctx12, mapped)
        tw.test_mixed_call(ctx12, mapped)


# ---- e. costs and the integer search --------------------------------------------------------------------------------------------
def test_costs_at_opposite_ends(ctx):
    """hmx_getSAD / hmx_getSSE / hmx_calcHAD with |org - cur| = 2^B - 1 on every sample, 64x64 and 4x4 among the shapes; then
    hmx_batch_subpel_cost (SAD and HAD) and hmx_batch_fullpel_search with its cost map, original and reference at opposite ends."""
    O, B, L = ol.oracle(), ctx.bit_depth, capi.lib()
    O.hmo_calcHAD.restype = O.hmo_getSSE.restype = C.c_uint32
    mx = (1 << B) - 1
    for (w, h) in ((4, 4), (8, 8), (64, 64), (8, 4), (12, 16), (64, 32)):
        for flip in (0, 1):
            org, cur = np.full((h, w), mx * flip, np.int16), np.full((h, w), mx * (1 - flip), np.int16)
            po, pc, v = org.ctypes.data_as(C.c_void_p), cur.ctypes.data_as(C.c_void_p), C.c_uint32(0)
            ctx._chk(L.hmx_calcHAD(ctx.h, po, w, pc, w, w, h, C.byref(v)))
            assert v.value == O.hmo_calcHAD(po, w, pc, w, w, h, B), ("calcHAD", w, h, flip)
            ctx._chk(L.hmx_getSSE(ctx.h, pc, w, po, w, w, h, C.byref(v)))
            assert v.value == O.hmo_getSSE(po, w, pc, w, w, h, B) == ((mx * mx) >> (2 * (B - 8))) * w * h, ("SSE", w, h, flip)
            for s in (0, 1) if h > 8 else (0,):
                assert ctx.getSAD(cur, w, org, w, w, h, s) == mo.sad(org, cur, s, B) == ((w * (h >> s) * mx) << s) >> (B - 8), ("SAD", w, h, s, flip)
    # the batch entries: W x H = 192 x 128 as tests/test_gpu_me.py; reference 0 all zero, reference 1 all maxv; the original's left half
    # maxv, its right half 0
    W, H, M = tm.W, tm.H, tm.M
    refs = [np.zeros((H + 2 * M, W + 2 * M), np.int16), np.full((H + 2 * M, W + 2 * M), mx, np.int16)]
    org = np.zeros((H, W), np.int16)
    org[:, :W // 2] = mx
    p = tm.Pictures(ctx, refs, org)
    units = np.concatenate([tm.boxed(0, 0, 64, 64, 0, 0, 0, 0, 3), tm.boxed(0, 64, 64, 64, 0, 1, 2, -3, 3), tm.boxed(128, 0, 64, 64, 1, 0, -5, 1, 3),
                            tm.boxed(128, 64, 64, 64, 1, 1, 0, 0, 3), tm.boxed(8, 8, 4, 4, 0, 0, 1, 1, 3), tm.boxed(120, 100, 4, 4, 1, 0, 0, 0, 3),
                            tm.boxed(32, 32, 64, 64, 0, 0, 0, 0, 2), tm.boxed(16, 16, 12, 16, 0, 1, 0, 0, 2)])
    res, cmap, first = p.check(units, 400000, "opposite ends")
    assert int(res[0]["sad"]) == int(res[2]["sad"]) == (64 * 64 * mx) >> (B - 8)  # at 12 bit 64 * 64 * 4095 >> 4
    assert int(res[1]["sad"]) == int(res[3]["sad"]) == ((32 * 64 * mx) << 1) >> (B - 8)
    assert int(res[4]["sad"]) == int(res[5]["sad"]) == (16 * mx) >> (B - 8)
    assert int(res[6]["sad"]) == (64 * 64 * mx) >> (B - 8)
    pus = np.zeros(6, capi.PU_DTYPE)
    for i, (x, y, w, h, r) in enumerate(((0, 0, 64, 64, 0), (128, 0, 64, 64, 1), (8, 8, 4, 4, 0), (120, 100, 4, 4, 1), (64, 64, 8, 8, 0), (16, 16, 12, 16, 0))):
        pus[i] = (x, y, w, h, r, 255, 4 * (i - 2), 4 * (2 - i), 0, 0)
    offs = np.array([(0, 0), (2, 0), (0, 2), (-2, -2), (1, 3), (-3, 1)], np.int8)
    ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in p.refs])
    for use_had in (0, 1):
        d_cost = ctx.alloc(4 * len(pus) * len(offs))
        ctx._chk(L.hmx_batch_subpel_cost(ctx.h, pus.ctypes.data, len(pus), ref_arr, 2, C.byref(p.org.as_pic()), offs.ctypes.data, len(offs), use_had, d_cost.ptr))
        got = d_cost.download(np.uint32).reshape(len(pus), len(offs))
        d_cost.free()
        for i, u in enumerate(pus):  # a constant reference interpolates to itself at every phase
            w, h = int(u["w"]), int(u["h"])
            ob = np.ascontiguousarray(org[int(u["y"]):int(u["y"]) + h, int(u["x"]):int(u["x"]) + w])
            pred = np.full((h, w), mx * int(u["ref0"]), np.int16)
            want = O.hmo_calcHAD(ob.ctypes.data_as(C.c_void_p), w, pred.ctypes.data_as(C.c_void_p), w, w, h, B) if use_had else (w * h * mx) >> (B - 8)
            assert [int(v) for v in got[i]] == [want] * len(offs), ("subpel cost", use_had, i, u)
    p.free()


def test_motion_search_12bit(ctx12):
    """tests/test_gpu_me.py at 12 bit, test_signed_originals among them."""
    tm.test_get_sad_vs_oracle(ctx12)
    tm.test_signed_originals(ctx12)
    tm.test_ties(ctx12)
    tex = tm.make_textured(ctx12)
    try:
        tm.test_batch_vs_oracle_with_map(ctx12, tex)
        tm.test_full_range_boxes(ctx12, tex)
        tm.test_map_vs_subpel_cost(ctx12, tex)
        tm.test_workload_units(ctx12, tex)
    finally:
        tex.free()


# ---- f. deblocking --------------------------------------------------------------------------------------------------------------
DBK_PARAMS = [(True, -6, 6), (False, 0, 0), (True, 6, -6)]  # per picture of a batch: no-filter map in use, beta offset, tc offset


@pytest.mark.parametrize("w,h", SIZES)
def test_deblock_on_edge_content(ctx, w, h):
    B = ctx.bit_depth
    rng = np.random.default_rng(10500 + B + w)  # seeds at which every case below reaches both ends (checked with the oracle alone)
    for use_nof in (True, False):
        pics = [xi.dbk_edge_content(rng, w, h, B) for _ in range(3)]
        boffs, toffs = [p[1] for p in DBK_PARAMS], [p[2] for p in DBK_PARAMS]
        assert all({0, 1, 2} <= set(d["bsv"].reshape(-1)) and d["qp"].min() < 16 and d["qp"].max() > 45 for d in pics)  # tc = beta = 0 next to active edges
        want = [tl.oracle_deblock(d, w, h, B, use_nof, boffs[i], toffs[i]) for i, d in enumerate(pics)]
        total = np.zeros((2, 2), np.int64)
        for i, (d, o) in enumerate(zip(pics, want)):
            changed = [int((a != b).sum()) for a, b in zip(d["planes"], o)]
            assert changed[0] > 1000 and changed[1] > 100, changed  # a filter that does nothing must not pass
            cnt = xi.dbk_count_outside(d, w, h, B, use_nof, boffs[i], toffs[i])
            total += np.array([cnt["luma"], cnt["chroma"]])
        print("deblock", B, (w, h), "no-filter map" if use_nof else "no map", "lines outside [luma, chroma][below, above]", total.tolist())
        assert (total > 0).all(), total
        for single in (False, True):
            got, intact = tl.gpu_deblock(ctx, pics, w, h, use_nof, boffs, toffs, single=single)
            for i in range(3):
                for p in range(3):
                    assert np.array_equal(got[i][p], want[i][p]), ("single" if single else "multi", use_nof, i, p, np.argwhere(got[i][p] != want[i][p])[:4])
            assert intact


def test_deblock_12bit(ctx12):
    for n, w, h in [(1, 8, 8), (3, 64, 64), (3, 72, 72), (5, 200, 136), (1, 416, 240)]:
        tl.test_deblock_batch(ctx12, n, w, h)
    tl.test_deblock_order(ctx12)


# ---- g. SAO and the SAO statistics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES)
def test_sao_on_edge_content(ctx, w, h):
    import test_oracle_vs_ref as T
    L, B, n = capi.lib(), ctx.bit_depth, 3
    mx, up = (1 << B) - 1, B - min(B, 10)
    n_lcu = -(-w // 64) * -(-h // 64)
    rng = np.random.default_rng(9600 + B + w)
    ins = []
    for _ in range(n):
        prm = T._sao_params(rng, n_lcu)
        for c in range(3):  # every type in every component, and the largest offsets of both signs
            prm["type"][c, rng.permutation(n_lcu)[:6]] = np.arange(-1, 5)
            prm["offset"][c, :, 0], prm["offset"][c, :, 3] = 7, -7
        ins.append((xi.sao_edge_content(rng, w, h, B), prm))
    want = [tl.oracle_sao(pl, prm, w, h, B) for pl, prm in ins]
    for (pl, prm), o in zip(ins, want):
        unc, add = xi.sao_unclipped(pl, prm, w, h, B)
        for k in range(3):
            below, above = xi.count_outside(unc[k], B)
            assert below > 0 and above > 0, (k, below, above)
            assert np.array_equal(np.clip(unc[k], 0, mx), o[k])
            inside = (unc[k] >= 0) & (unc[k] <= mx) & (add[k] != 0)  # the offsets as applied: scaled by 1 << (B - 10) at 12 bit
            assert inside.any() and np.array_equal((o[k].astype(np.int64) - pl[k])[inside], (add[k] << up)[inside])
            assert (np.abs(o[k].astype(np.int64) - pl[k]) == 7 << up).any()
    src = [tl.upload(ctx, pl, w, h, **tl.shape_of(i)) for i, (pl, _) in enumerate(ins)]
    zero = [np.zeros_like(p) for p in ins[0][0]]
    d_prm = ctx.to_device(np.ascontiguousarray(np.stack([prm for _, prm in ins])))
    for single in (False, True):
        dst = [tl.upload(ctx, zero, w, h, **tl.shape_of(i + 1)) for i in range(n)]
        if single:
            for i in range(n):
                a, b = src[i].as_pic(), dst[i].as_pic()
                ctx._chk(L.hmx_sao_picture(ctx.h, C.byref(a), C.byref(b), w, h, d_prm.ptr + i * 3 * n_lcu * 6, n_lcu))
        else:
            ctx.sao_pictures(src, dst, w, h, d_prm)
        ctx.sync()
        for i in range(n):
            got = dst[i].download()
            for p in range(3):
                assert np.array_equal(got[p], want[i][p]), ("single" if single else "multi", i, p, np.argwhere(got[p] != want[i][p])[:4])
            assert tl.surroundings_intact(dst[i])
            dst[i].free()
    for x in src + [d_prm]:
        x.free()


def test_sao_12bit(ctx12):
    for n in (1, 4):
        for w, h in [(416, 240), (200, 136), (136, 72)]:
            tl.test_sao_batch(ctx12, n, w, h)


@pytest.mark.parametrize("ctu", [64, 32])
def test_sao_stats_at_opposite_ends(ctx, ctu):
    """org and rec at opposite range ends over whole pictures, both ways round, in one call: every sum is count * (2^B - 1)."""
    B = ctx.bit_depth
    mx = (1 << B) - 1
    c = ctx if ctu == 64 else capi.Context(bit_depth=B, ctu_size=32)
    try:
        for w, h in SIZES:
            full, zero = xi.opposite_ends(w, h, B)
            for lcu_based in (0, 1):
                got = ts.gpu_stats(c, [full, zero], [zero, full], w, h, lcu_based)
                for i, (o, r) in enumerate(((full, zero), (zero, full))):
                    want = stats_vec(o, r, w, h, ctu, B, lcu_based)
                    assert np.array_equal(got[i], want), (ctu, (w, h), lcu_based, i, np.argwhere(got[i] != want)[:4])
                    assert (np.abs(want[..., 0]) == want[..., 1] * mx).all() and want[..., 1].max() > 0
                    assert np.abs(got[i][..., 0]).max() == want[..., 1].max() * mx  # the fullest bin: count * maxv
                assert got[0][..., 0].max() == (ctu * ctu if not lcu_based else (ctu - 5) * (ctu - 4)) * mx  # a whole luma CTU in one band
    finally:
        if c is not ctx:
            c.close()


def test_sao_stats_12bit(ctx12):
    for w, h in ts.SIZES:
        if w * h <= 416 * 240:
            for lcu_based in (0, 1):
                ts.test_random(ctx12, w, h, lcu_based)
    ts.test_multi_margins_pad_skew(ctx12)
    ts.test_every_bin_written(ctx12)
    for lcu_based in (0, 1):
        ts.test_extreme_values(ctx12, lcu_based)
