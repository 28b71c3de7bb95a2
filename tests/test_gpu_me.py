"""Full-search integer motion estimation on the GPU against tests/me_oracle.py, everything compared for equality: the scalar
hmx_getSAD, hmx_batch_fullpel_search with its cost map (every candidate of every unit), ties, originals outside the sample
range, the cross-check of the map against hmx_batch_subpel_cost (which is pinned on the compiled reference), the host-side
argument checks, and xPatternSearch through the C++ host mirror.  A 192 x 128 picture with margin 80, bit depths 8 and 10."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import me_oracle as mo
from thevc_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
W, H, M = 192, 128, 80


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


class Pictures:
    """Device pictures from host luma planes: refs (H + 2M, W + 2M) with margins, org (H, W)."""

    def __init__(self, ctx, refs_full, org):
        self.ctx, self.full, self.org_h = ctx, refs_full, org
        self.refs = []
        for f in refs_full:
            d = capi.DevPicture(ctx, W, H, M, M)
            flat = np.zeros(d.elems[0], np.int16)
            flat[:] = np.ascontiguousarray(f, np.int16).reshape(-1)
            d.bufs[0].upload(flat)
            self.refs.append(d)
        z = np.zeros((H // 2, W // 2), np.int16)
        self.org = capi.DevPicture(ctx, W, H).upload([org, z, z])

    def free(self):
        for d in self.refs + [self.org]:
            d.free()

    def check(self, units, lam, label):
        """Run the batch entry with the map and compare every result and every map entry with the oracle."""
        B = self.ctx.bit_depth
        res, cmap, first = self.ctx.batch_fullpel_search(units, self.refs, self.org, W, H, M, M, lam, want_map=True)
        for i, u in enumerate(units):
            (mx, my, sad, cost), want = mo.search(self.org_h, self.full[int(u["ref"])], (M, M), u, lam, B)
            got = cmap[first[i]:first[i + 1]].reshape(want.shape)
            assert np.array_equal(got, want), (label, i, u, np.argwhere(got != want)[:4])
            assert (int(res[i]["mvx"]), int(res[i]["mvy"]), int(res[i]["sad"]), int(res[i]["cost"])) == (mx, my, sad, cost), (label, i, u)
        plain = self.ctx.batch_fullpel_search(units, self.refs, self.org, W, H, M, M, lam)  # d_cost_map = NULL
        assert np.array_equal(plain, res), label
        return res, cmap, first


def unit(x, y, w, h, ref, s, px, py, l, t, r, b):
    u = np.zeros(1, capi.ME_UNIT_DTYPE)
    u[0] = (x, y, w, h, ref, s, px, py, l, t, r, b)
    return u


def boxed(x, y, w, h, ref, s, px, py, rng_):
    return unit(x, y, w, h, ref, s, px, py, *capi.set_search_range(px, py, rng_, x, y, W, H, 64))


def make_textured(ctx):
    """The textured pictures on the device (the caller frees them); tests/test_gpu_inter_loop_edges.py makes them at 12 bit."""
    B = ctx.bit_depth
    rng = np.random.default_rng(800 + B)
    # smooth texture plus noise, so that costs have structure and a real minimum; margins hold samples of their own
    refs = []
    for k in range(2):
        yy, xx = np.mgrid[0:H + 2 * M, 0:W + 2 * M]
        base = (np.sin(xx / (5.0 + k)) + np.cos(yy / (7.0 - k))) * (1 << (B - 3)) + (1 << (B - 1))
        refs.append(np.clip(base + rng.integers(-(1 << (B - 4)), 1 << (B - 4), base.shape), 0, (1 << B) - 1).astype(np.int16))
    org = np.clip(refs[0][M + 3:M + 3 + H, M - 2:M - 2 + W].astype(np.int32) + rng.integers(-6, 7, (H, W)), 0, (1 << B) - 1).astype(np.int16)
    return Pictures(ctx, refs, org)


@pytest.fixture(scope="module")
def textured(ctx):
    p = make_textured(ctx)
    yield p
    p.free()


# ---- 1. hmx_getSAD ----
def test_get_sad_vs_oracle(ctx):
    B = ctx.bit_depth
    rng = np.random.default_rng(810 + B)
    n = 0
    for w in mo.SIZES:
        for h in (4, 8, 12, 32, 64) if w % 8 else (4, 16, 24, 48, 64):
            so, sc = w + 5, w + 11  # strides larger than the width
            org = rng.integers(-(1 << B), 1 << (B + 1), (h, so)).astype(np.int16)
            cur = rng.integers(0, 1 << B, (h, sc)).astype(np.int16)
            for s in (0, 1):
                if s and h <= 8:
                    with pytest.raises(capi.HmxError, match="sub_shift"):
                        ctx.getSAD(cur, sc, org, so, w, h, s)
                    continue
                assert ctx.getSAD(cur, sc, org, so, w, h, s) == mo.sad(org[:, :w], cur[:, :w], s, B), (w, h, s)
                n += 1
    assert n >= 60
    with pytest.raises(capi.HmxError, match="width and height"):
        ctx.getSAD(np.zeros(400, np.int16), 20, np.zeros(400, np.int16), 20, 20, 16, 0)


# ---- 2. the batch entry against the oracle, with the cost map ----
def test_batch_vs_oracle_with_map(ctx, textured):
    rng = np.random.default_rng(820 + ctx.bit_depth)
    # every width and every height of the set, the shapes the issue names among them
    shapes = [(8, 4), (4, 8), (12, 16), (16, 4), (24, 32), (64, 48), (64, 64), (4, 4), (8, 8), (16, 12), (32, 24), (48, 64), (32, 32), (16, 16),
              (48, 16), (16, 64), (24, 8), (12, 48)]
    assert {s[0] for s in shapes} == set(mo.SIZES) == {s[1] for s in shapes}
    units = []
    for k, (w, h) in enumerate(shapes * 2):
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        s = int(h > 8 and k % 2 == 0)
        px, py = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
        units.append(boxed(x, y, w, h, k % 2, s, px, py, (1, 4, 9)[k % 3]))
    units += [unit(40, 40, 16, 16, 1, 1, 3, -5, 2, -3, 2, -3),       # a single candidate
              unit(64, 32, 8, 8, 0, 0, -7, 9, -11, 0, 2, 1),         # asymmetric boxes
              unit(96, 64, 32, 16, 1, 0, 0, 0, 3, -20, 5, 13),
              unit(20, 12, 4, 16, 0, 1, 100, -100, -33, -2, 0, 0)]   # 34 wide: the box crosses one tile by two candidates
    for (x, y) in ((0, 0), (W - 16, 0), (0, H - 16), (W - 16, H - 16)):  # the corners, predictors that xSetSearchRange clips
        px, py = (-300 if x == 0 else 300), (-300 if y == 0 else 300)
        units.append(boxed(x, y, 16, 16, (x + y) % 2, 1, px, py, 9))
    units = np.concatenate(units)
    assert len(units) >= 40 and set(units["sub_shift"]) == {0, 1} and set(units["ref"]) == {0, 1}
    textured.check(units, 1234567, "mixed")


def test_full_range_boxes(ctx, textured):
    """Two units at the full +-64: 5 x 5 tiles each and the minimum across workgroups."""
    units = np.concatenate([boxed(64, 32, 64, 64, 0, 1, 2, -3, 64), boxed(96, 64, 8, 8, 1, 0, -5, 6, 64)])
    assert all(int(u["right"]) - int(u["left"]) == 128 and int(u["bottom"]) - int(u["top"]) == 128 for u in units)
    textured.check(units, 3000000, "full range")


# ---- 3. ties ----
def test_ties(ctx):
    B = ctx.bit_depth
    const = [np.full((H + 2 * M, W + 2 * M), (1 << B) - 3, np.int16)]
    rng = np.random.default_rng(830 + B)
    org = rng.integers(0, 1 << B, (H, W)).astype(np.int16)
    p = Pictures(ctx, const, org)
    u = np.concatenate([unit(64, 32, 16, 16, 0, 0, 0, 0, -40, -20, 40, 37), unit(32, 64, 8, 8, 0, 0, 0, 0, -40, 3, 40, 37)])  # 81 wide: three tiles
    res, _, _ = p.check(u, 0, "constant reference, lambda 0")
    assert [(int(r["mvx"]), int(r["mvy"])) for r in res] == [(-40, -20), (-40, 3)]  # (left, top)
    res, _, _ = p.check(u, 65536 * 4, "constant reference, lambda > 0")
    # predictor (0, 0): (0, 0) costs two bits and wins alone in the first box; the second box starts at y = 3, and (0, 3) wins alone
    assert [(int(r["mvx"]), int(r["mvy"])) for r in res] == [(0, 0), (0, 3)]
    # symmetric minima, bits(+v) = bits(-v): with the predictor half a sample left of 0, x = -1 (v = -2) and x = 0 (v = +2) tie; the
    # box starts at -32, so they are the last candidate of one tile and the first of the next, and the raster-first, x = -1, wins.
    # The same vertically; and with both, four candidates of four workgroups tie.
    u = np.concatenate([unit(64, 32, 16, 16, 0, 0, -2, 0, -32, -3, 40, -3), unit(64, 32, 16, 16, 0, 0, 0, -2, 5, -32, 7, 20),
                        unit(64, 32, 8, 8, 0, 0, -2, -2, -32, -32, 31, 31)])
    res, _, _ = p.check(u, 65536 * 4, "constant reference, symmetric minima across tiles")
    assert [(int(r["mvx"]), int(r["mvy"])) for r in res] == [(-1, -3), (5, -1), (-1, -1)]
    p.free()
    # a periodic texture, period 8 in x and 4 in y, box 33 x 9 around the unit: equal SADs 8 and 32 candidates apart
    yy, xx = np.mgrid[0:H + 2 * M, 0:W + 2 * M]
    tex = (((xx % 8) * 5 + (yy % 4) * 11) % (1 << B)).astype(np.int16)
    org = tex[M:M + H, M:M + W].copy()
    p = Pictures(ctx, [tex], org)
    u = np.concatenate([unit(64, 32, 16, 16, 0, 0, 0, 0, -20, -6, 20, 6), unit(32, 32, 32, 32, 0, 1, 0, 0, -36, -8, 36, 8)])
    res, _, _ = p.check(u, 0, "periodic, lambda 0")
    assert [(int(r["mvx"]), int(r["mvy"]), int(r["sad"])) for r in res] == [(-16, -4, 0), (-32, -8, 0)]  # the first zero in raster order
    res, _, _ = p.check(u, 70000, "periodic, lambda > 0")
    assert [(int(r["mvx"]), int(r["mvy"])) for r in res] == [(0, 0), (0, 0)]
    p.free()


# ---- 4. originals outside the sample range ----
def test_signed_originals(ctx):
    B = ctx.bit_depth
    rng = np.random.default_rng(840 + B)
    org = rng.integers(-(1 << B), 1 << (B + 1), (H, W)).astype(np.int16)
    org[0:64, 0:64] = -(1 << B)               # the extremes, whole 64 x 64 blocks of them
    org[64:128, 0:64] = (1 << (B + 1)) - 1
    refs = [np.zeros((H + 2 * M, W + 2 * M), np.int16), np.full((H + 2 * M, W + 2 * M), (1 << B) - 1, np.int16)]
    p = Pictures(ctx, refs, org)
    units = np.concatenate([boxed(0, 0, 64, 64, 1, 0, 0, 0, 4), boxed(0, 64, 64, 64, 0, 0, 3, 3, 4), boxed(64, 0, 64, 64, 0, 0, -9, 2, 4),
                            boxed(64, 64, 64, 64, 1, 1, 0, 0, 4), boxed(128, 32, 64, 64, 1, 0, 5, 5, 1), boxed(0, 64, 64, 64, 0, 1, 0, 0, 1)])
    res, _, _ = p.check(units, 500000, "signed originals")
    assert int(res[0]["sad"]) == (64 * 64 * ((1 << B) + (1 << B) - 1)) >> (B - 8)  # |-2^B - (2^B - 1)| on every sample
    assert int(res[1]["sad"]) == (64 * 64 * ((1 << (B + 1)) - 1)) >> (B - 8)
    p.free()


# ---- 5. the map against hmx_batch_subpel_cost, which is pinned on the compiled reference ----
def test_map_vs_subpel_cost(ctx, textured):
    L = capi.lib()
    rng = np.random.default_rng(850 + ctx.bit_depth)
    shapes = [(8, 8), (16, 16), (32, 32), (64, 64), (16, 8), (8, 16), (32, 16), (64, 32), (24, 32), (12, 16), (4, 8), (48, 64)]
    units = np.concatenate([boxed(int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4, w, h, k % 2, 0,
                                  int(rng.integers(-30, 31)), int(rng.integers(-30, 31)), 4) for k, (w, h) in enumerate(shapes)])
    res, cmap, first = ctx.batch_fullpel_search(units, textured.refs, textured.org, W, H, M, M, 0, want_map=True)
    K = 12  # candidates per unit, all in one call
    pus = np.zeros(len(units) * K, capi.PU_DTYPE)
    cand = []
    for i, u in enumerate(units):
        bw, bh = int(u["right"]) - int(u["left"]) + 1, int(u["bottom"]) - int(u["top"]) + 1
        picks = [0, bw * bh - 1] + [int(v) for v in rng.choice(np.arange(1, bw * bh - 1), K - 2, replace=False)]  # the corners and ten others
        for k, idx in enumerate(picks):
            cand.append(int(first[i]) + idx)
            pus[i * K + k] = (u["x"], u["y"], u["w"], u["h"], u["ref"], 255, 4 * (int(u["left"]) + idx % bw), 4 * (int(u["top"]) + idx // bw), 0, 0)
    offs = np.zeros((1, 2), np.int8)
    d_cost = ctx.alloc(4 * len(pus))
    ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in textured.refs])
    ctx._chk(L.hmx_batch_subpel_cost(ctx.h, pus.ctypes.data, len(pus), ref_arr, 2, C.byref(textured.org.as_pic()), offs.ctypes.data, 1, 0, d_cost.ptr))
    want = d_cost.download(np.uint32)
    d_cost.free()
    got = [int(cmap[c]) for c in cand]
    assert got == [int(v) for v in want]
    assert len(set(got)) > 6 * K  # not a comparison of constants


# ---- 5b. the unit lists of workload.make_me_units ----
def test_workload_units(ctx, textured):
    from thevc_amd import workload
    units = workload.make_me_units(860 + ctx.bit_depth, W, H, 2, 4)
    assert len(units) >= 6 and len(set(zip(units["w"], units["h"]))) > 2
    textured.check(units, 2222222, "make_me_units")


# ---- 6. host validation ----
def test_host_validation(ctx, textured):
    good = unit(64, 32, 16, 16, 0, 0, 0, 0, -4, -4, 4, 4)

    def bad(msg, n=1, **kw):
        u = np.concatenate([good] * n)  # the last of n units is the bad one
        for k, v in kw.items():
            u[n - 1][k] = v
        sentinel = np.full(3, 0x5A5A5A5A, np.uint32)
        d_res = ctx.to_device(sentinel)
        ref_arr = (capi.Pic * 2)(*[r.as_pic() for r in textured.refs])
        rc = capi.lib().hmx_batch_fullpel_search(ctx.h, u.ctypes.data, n, ref_arr, 2, C.byref(textured.org.as_pic()), W, H, M, M, 0,
                                                 d_res.ptr, None)
        assert rc == -1, (msg, rc)  # HMX_ERR_ARG
        assert msg in capi.lib().hmx_last_error(ctx.h).decode(), (msg, capi.lib().hmx_last_error(ctx.h).decode())
        assert f"unit {n - 1}: " in capi.lib().hmx_last_error(ctx.h).decode()  # the unit is named
        ctx.sync()
        assert np.array_equal(d_res.download(np.uint32), sentinel), msg  # nothing was launched
        d_res.free()

    bad("width and height", w=20)
    bad("width and height", h=6)
    bad("reference index", ref=2)
    bad("sub_shift", sub_shift=2)
    bad("sub_shift", sub_shift=1, h=8)
    bad("empty search box", left=5)
    bad("empty search box", bottom=-5)
    bad("above 129", left=-65, right=64)
    bad("above 129", top=-64, bottom=65)
    bad("outside the picture", x=W - 8)
    bad("outside the picture", y=H - 12)
    bad("outside the reference's margins", x=0, left=-M - 1)
    bad("outside the reference's margins", x=W - 16, right=M + 1)
    bad("outside the reference's margins", y=0, top=-M - 1)
    bad("outside the reference's margins", y=H - 16, bottom=M + 1)
    bad("sub_shift", n=3, sub_shift=2)  # only unit 2 of three is bad: the prefix names it
    # the margins themselves are legal, and the context still works
    edge = np.concatenate([unit(0, 0, 16, 16, 0, 0, 0, 0, -M, -M, -M + 3, -M + 3), unit(W - 16, H - 16, 16, 16, 1, 1, 0, 0, M - 2, M - 2, M, M), good])
    textured.check(edge, 99999, "after refused calls")


# ---- 7. the C++ host mirror ----
def check_mirror_output(out, B):
    lines = out.strip().split("\n")
    assert len(lines) == 4
    p = [int(v) for v in lines[0].split()]
    u = dict(zip(("x", "y", "w", "h", "sub_shift", "pred_x", "pred_y", "left", "top", "right", "bottom"), p[:11]))
    lam, w, h, m = p[11:]
    org = np.array(lines[1].split(), np.int64).reshape(h, w)
    ref = np.array(lines[2].split(), np.int64).reshape(h + 2 * m, w + 2 * m)
    assert (u["left"], u["top"], u["right"], u["bottom"]) == mo.set_search_range(u["pred_x"], u["pred_y"], 6, u["x"], u["y"], w, h)
    assert u["sub_shift"] in (0, 1) and lam > 65536
    (mx, my, sad, _), _ = mo.search(org, ref, (m, m), u, lam, B)
    assert [int(v) for v in lines[3].split()] == [mx, my, sad]


@pytest.mark.parametrize("B,seed", [(8, 4), (10, 7)])
def test_mirror_pattern_search(B, seed):
    import __graft_entry__ as g
    g.build()
    out = subprocess.run([EXE, "me", str(B), str(seed)], capture_output=True, text=True, check=True).stdout
    check_mirror_output(out, B)
