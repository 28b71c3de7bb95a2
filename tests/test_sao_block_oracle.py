"""CPU side of the loop filters at slice and tile boundaries they may not cross: the literal restatement of the reference's
block path of SAO (tests/sao_block_oracle.py) against the reference decoder's pictures of the lfx_* fixtures, the per-sample
rule that the device implements against the literal restatement, and hmx_lf_border_avail against its numpy twin."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import sao_block_oracle as SB
from sao_stats_oracle import stats_vec
from thevc_amd import capi
from thevc_amd import decisions as D

HERE = os.path.dirname(os.path.abspath(__file__))
LFX = sorted(glob.glob(os.path.join(HERE, "golden", "lfx_*.npz")))
CONTROL = [f for f in LFX if f.endswith("_cross.npz")]
CLOSED = [f for f in LFX if f not in CONTROL]
ids = lambda fs: [os.path.basename(f)[:-4] for f in fs]


def test_fixtures_present():
    assert len(CLOSED) == 4 and len(CONTROL) == 1
    union = set()
    for f in CLOSED:
        pics = list(D.load_pictures(f))
        assert all(D.is_deblocked(p) for p in pics) and D.has_sao(pics[0]), f  # (the encoder may leave a P picture without an SAO CTU)
        for p in pics:
            avail = D.picture_avail(p)
            closed = avail != D.lf_border_avail(p["w"], p["h"], p["ctu"])
            assert closed.any(), f
            union |= {int(t) for t in p["sao"]["type"][:, closed].reshape(-1)}
    assert {0, 1, 2, 3, 4} <= union
    assert any(len(p["pus"]) for f in CLOSED for p in D.load_pictures(f)), "no inter picture with a closed boundary"
    assert any(p["B"] == 10 for f in CLOSED for p in D.load_pictures(f))
    for p in D.load_pictures(CONTROL[0]):
        assert int(p["slice_id"].max()) > 0 and D.avail_is_geometry(p, D.picture_avail(p))


def test_slices_of_nine_close_a_corner_only():
    """fixture (a): CTUs whose left and top neighbours may be read while the top-left one may not"""
    p = next(iter(D.load_pictures([f for f in CLOSED if "slices9" in f][0])))
    a = D.picture_avail(p)
    corner_only = ((a >> D.SGU_L) & 1) & ((a >> D.SGU_T) & 1) & ~((a >> D.SGU_TL) & 1) & 1
    cw = -(-p["w"] // p["ctu"])
    inside = (np.arange(len(a)) % cw > 0) & (np.arange(len(a)) // cw > 0)
    assert (corner_only.astype(bool) & inside).any()


@pytest.mark.parametrize("path", LFX, ids=ids(LFX))
def test_literal_oracle_reproduces_reference_streams(path):
    """block path + the oracle's deblocking (closed edges dropped) + processSaoBlock restated literally == the reference
    decoder's pictures; the per-sample rule on the same deblocked pictures gives the same"""
    pics = list(D.load_pictures(path))
    out, dbk = SB.cpu_decode(pics, True)
    for p, got, d in zip(pics, out, dbk):
        rule = SB.apply_rule(d, p["sao"], p["w"], p["h"], p["B"], p["ctu"], D.picture_avail(p))
        for k in range(3):
            bad = np.argwhere(got[k] != p["rec"][k])
            assert not len(bad), (os.path.basename(path), "poc", p["poc"], "plane", k, "first mismatch (y, x)", bad[0].tolist(), len(bad))
            assert np.array_equal(rule[k], p["rec"][k]), (os.path.basename(path), "rule", p["poc"], k)


@pytest.mark.parametrize("path", CLOSED, ids=ids(CLOSED))
def test_fixtures_tell_the_boundaries(path):
    """without the boundaries in the loop filters (the mask of the geometry, every edge) the pictures are NOT the reference's"""
    pics = list(D.load_pictures(path))
    out, _ = SB.cpu_decode(pics, False, literal=False)
    for p, got in zip(pics, out):
        assert any(not np.array_equal(got[k], p["rec"][k]) for k in range(3)), (os.path.basename(path), p["poc"])


@pytest.mark.parametrize("B", [8, 12])
def test_rule_is_the_literal_application(B):
    """every mask value on the centre CTU of 3 x 3, every edge type on luma and chroma, samples at the range ends"""
    c = SB.all_masks_case(B)
    w, h, ctu = c["w"], c["h"], c["ctu"]
    for i in range(len(c["prm"])):
        lit = SB.apply_literal(c["rec"], c["prm"][i], w, h, B, ctu, c["avail"][i], only={4})
        rule = SB.apply_rule(c["rec"], c["prm"][i], w, h, B, ctu, c["avail"][i])
        for k in range(3):
            cs = ctu >> (1 if k else 0)
            assert np.array_equal(lit[k][cs:2 * cs, cs:2 * cs], rule[k][cs:2 * cs, cs:2 * cs]), (i, int(c["avail"][i][4]), k)
    changed = SB.apply_rule(c["rec"], c["prm"][255], w, h, B, ctu, c["avail"][255])
    assert any(not np.array_equal(a, b) for a, b in zip(changed, c["rec"]))


@pytest.mark.parametrize("B", [8, 12])
def test_rule_is_the_literal_statistics(B):
    c = SB.all_masks_case(B)
    w, h, ctu = c["w"], c["h"], c["ctu"]
    for m in range(256):
        lit = SB.stats_literal(c["org"], c["rec"], w, h, ctu, B, c["avail"][m], only={4})
        rule = SB.stats_rule(c["org"], c["rec"], w, h, ctu, B, c["avail"][m])
        assert np.array_equal(lit[:, 4], rule[:, 4]), m


def test_rule_is_literal_on_cut_ctus():
    """40x24 with CTU 16: whole pictures, a random byte on every CTU"""
    c = SB.odd_case()
    for p in c["pics"]:
        lit = SB.apply_literal(p["rec"], p["prm"], c["w"], c["h"], c["B"], c["ctu"], p["avail"])
        rule = SB.apply_rule(p["rec"], p["prm"], c["w"], c["h"], c["B"], c["ctu"], p["avail"])
        assert all(np.array_equal(a, b) for a, b in zip(lit, rule))
        assert np.array_equal(SB.stats_literal(p["org"], p["rec"], c["w"], c["h"], c["ctu"], c["B"], p["avail"]),
                              SB.stats_rule(p["org"], p["rec"], c["w"], c["h"], c["ctu"], c["B"], p["avail"]))


@pytest.mark.parametrize("w,h,ctu,B", [(48, 48, 16, 8), (48, 48, 16, 12), (40, 24, 16, 8), (200, 136, 64, 10)])
def test_geometry_mask_is_the_pinned_statistics(w, h, ctu, B):
    """with the mask of the geometry, the block statistics are calcSaoStatsCuOrg's without skipped rows and columns"""
    from extreme_inputs import sao_edge_content
    rng = np.random.default_rng(w + h + B)
    org, rec = sao_edge_content(rng, w, h, B), sao_edge_content(rng, w, h, B)
    geo = D.lf_border_avail(w, h, ctu)
    want = stats_vec(org, rec, w, h, ctu, B, 0)
    assert np.array_equal(SB.stats_rule(org, rec, w, h, ctu, B, geo), want)
    if w <= 48:
        assert np.array_equal(SB.stats_literal(org, rec, w, h, ctu, B, geo), want)


# ---- hmx_lf_border_avail -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", LFX, ids=ids(LFX))
def test_border_avail_on_fixtures(path):
    for p in D.load_pictures(path):
        want = D.picture_avail(p)
        got = capi.lf_border_avail(p["w"], p["h"], p["ctu"], p["slice_id"], p["lf_cross_slice"], p["tile_id"], p["lf_cross_tile"])
        assert np.array_equal(got, want)
        assert np.array_equal(capi.lf_border_avail(p["w"], p["h"], p["ctu"], np.zeros_like(p["slice_id"]), [0]), D.lf_border_avail(p["w"], p["h"], p["ctu"]))


def _model(w, h, ctu, sid, flags, tid, cross_tiles):
    """the bullets of the rule, CTU by CTU"""
    cw, ch = -(-w // ctu), -(-h // ctu)
    out = np.zeros(cw * ch, np.uint8)
    for a in range(cw * ch):
        for k, (dx, dy) in enumerate(D.SGU_OFFSETS):
            x, y = a % cw + dx, a // cw + dy
            if not (0 <= x < cw and 0 <= y < ch):
                continue
            n = y * cw + x
            if len(flags) == 1 or sid[n] == sid[a]:
                ok = True
            elif sid[n] > sid[a]:
                ok = bool(flags[sid[n]])
            else:
                ok = bool(flags[sid[a]])
            if not cross_tiles and tid is not None and tid[n] != tid[a]:
                ok = False
            out[a] |= int(ok) << k
    return out


@pytest.mark.parametrize("pic", [(416, 240, 64), (200, 136, 64), (48, 48, 16), (64, 64, 64), (136, 72, 32)])
def test_border_avail_random_layouts_and_mixed_flags(pic):
    """Random slice / tile layouts with a flag of its own per slice.  Mixed flags cannot come from a stream of the reference
    encoder: its application sets one LFCrossSliceBoundaryFlag for all slices (TEncGOP.cpp:240), so they are only tested here."""
    w, h, ctu = pic
    cw, ch = -(-w // ctu), -(-h // ctu)
    rng = np.random.default_rng(w * h)
    for trial in range(40):
        ncol, nrow = int(rng.integers(1, min(cw, 3) + 1)), int(rng.integers(1, min(ch, 3) + 1))
        cb, rb = D.uniform_bounds(cw, ncol), D.uniform_bounds(ch, nrow)
        n_starts = int(rng.integers(0, min(6, cw * ch)))
        starts = [0] + sorted(int(v) for v in rng.choice(np.arange(1, max(2, cw * ch)), size=min(n_starts, cw * ch - 1), replace=False)) if cw * ch > 1 else [0]
        sid, tid = D.slice_tile_maps(w, h, ctu, starts, cb, rb)
        flags = rng.integers(0, 2, int(sid.max()) + 1).astype(np.uint8)
        for cross_tiles in (False, True):
            for t in (tid, None):
                want = _model(w, h, ctu, sid, flags, t, cross_tiles)
                assert np.array_equal(D.lf_border_avail(w, h, ctu, sid, flags, t, cross_tiles), want), (trial, cross_tiles)
                assert np.array_equal(capi.lf_border_avail(w, h, ctu, sid, flags, t, cross_tiles), want), (trial, cross_tiles)


def test_border_avail_refusals():
    L = capi.lib()
    sid, fl, tid, out = np.zeros(28, np.uint32), np.ones(2, np.uint8), np.zeros(28, np.uint32), np.full(28, 0x5A, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [416, 240, 64, vp(sid), vp(fl), 2, vp(tid), 0, vp(out)]
    assert L.hmx_lf_border_avail(*good) == 0 and (out != 0x5A).all()
    out[:] = 0x5A
    for i, bad in ((0, 0), (0, -416), (1, 0), (1, -8), (2, 0), (2, -64), (3, None), (4, None), (5, 0), (5, -1), (8, None)):
        args = list(good)
        args[i] = bad
        assert L.hmx_lf_border_avail(*args) == -1, (i, bad)
    sid[27] = 2  # a slice id without a flag
    assert L.hmx_lf_border_avail(*good) == -1
    sid[27] = 1
    assert (out == 0x5A).all(), "a refused call wrote"
    args = list(good)
    args[6] = None  # one tile
    assert L.hmx_lf_border_avail(*args) == 0
    with pytest.raises(ValueError):
        D.lf_border_avail(416, 240, 64, np.full(28, 2), [1, 1])


# ---- edges of the deblocking filter ------------------------------------------------------------------------------------------

def test_closed_edges_are_dropped_and_nothing_else():
    for f in CLOSED:
        for p in D.load_pictures(f):
            open_p = dict(p, slice_id=None, tile_id=None, lf_cross_slice=None, lf_cross_tile=True)
            avail, n, cw = D.picture_avail(p), p["ctu"] // 4, -(-p["w"] // p["ctu"])
            pairs = [(D.deblock_maps(p)[:2], D.deblock_maps(open_p)[:2])]
            if len(p["pus"]):
                pairs.append((D.strength_inputs(p)[1:], D.strength_inputs(open_p)[1:]))
            for (ver, hor), (ver0, hor0) in pairs:
                keep_v, keep_h = np.ones(ver.shape, bool), np.ones(hor.shape, bool)
                for a, m in enumerate(avail):
                    cy, cx = divmod(a, cw)
                    if cx and not (m >> D.SGU_L) & 1:
                        keep_v[cy * n:(cy + 1) * n, cx * n] = False
                    if cy and not (m >> D.SGU_T) & 1:
                        keep_h[cy * n, cx * n:(cx + 1) * n] = False
                assert not keep_v.all() or not keep_h.all()
                assert np.array_equal(ver, np.where(keep_v, ver0, 0)) and np.array_equal(hor, np.where(keep_h, hor0, 0))
                assert (ver0[~keep_v] != 0).any() or (hor0[~keep_h] != 0).any()
    p = next(iter(D.load_pictures(CONTROL[0])))
    open_p = dict(p, slice_id=None, tile_id=None, lf_cross_slice=None, lf_cross_tile=True)
    assert all(np.array_equal(a, b) for a, b in zip(D.deblock_maps(p), D.deblock_maps(open_p)))
