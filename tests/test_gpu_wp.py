"""Explicit weighted prediction on the GPU against tests/wp_oracle.py: the scalar drop-ins (hmx_addWeightUni / hmx_addWeightBi),
one prediction unit (hmx_motionCompensation_wp), the batch entry in both schedules (cell map, one wave per PU), a call that
mixes weighted and unweighted jobs, and the host-side argument checks.  The batch entry is also held directly on the reference's own
results (tests/golden/wp_b*.npz, at 8, 10 and 12 bit); the scalar entries and the single unit on them: tests/test_golden.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import wp_cases as wc
import wp_oracle as wo
from thevc_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


def fade_entry(rng, denoms):
    """An entry as an encoder would code it for a fade: weights around 1 << denom, small offsets (results stay off the clips)."""
    return ([int((1 << d) + rng.integers(-(1 << d) // 2, (1 << d) // 2 + 1)) for d in denoms], [int(v) for v in rng.integers(-20, 21, 3)], list(denoms))


def table(entries):
    t = np.zeros(len(entries), capi.WP_DTYPE)
    for i, (w, o, d) in enumerate(entries):
        t[i]["weight"], t[i]["offset"], t[i]["log2_denom"] = w, o, d
    return t


# ---- 1. the scalar entries ----
@pytest.mark.parametrize("w,h", [(4, 4), (8, 4), (4, 8), (16, 12), (32, 32), (64, 64)])
def test_scalar_entries_vs_oracle(ctx, w, h):
    B = ctx.bit_depth
    rng = np.random.default_rng(5100 + 64 * w + h + B)
    full = rng.integers(-32768, 32768, (2, h, w)).astype(np.int16)  # any int16
    mid = ((rng.integers(0, 1 << B, (2, h, w)) << (14 - B)) - 8192).astype(np.int16)  # what the interpolation makes of samples
    for it in range(12):
        a, b = (full, mid)[it % 2]
        if it % 2 == 0:  # the full parameter ranges
            (w0, w1), (o0, o1), d = rng.integers(-128, 256, 2), rng.integers(-128, 128, 2), int(rng.integers(0, 8))
        else:
            d = int(rng.integers(0, 8))
            (w0, w1), (o0, o1) = (1 << d) + rng.integers(-(1 << d) // 2, (1 << d) // 2 + 1, 2), rng.integers(-20, 21, 2)
        w0, w1, o0, o1 = int(w0), int(w1), int(o0), int(o1)
        got = ctx.addWeightUni(a, w, h, w0, o0, d).reshape(h, w)
        assert np.array_equal(got, wo.weight_uni_vec(a, w0, o0, d, B)), ("uni", it, w0, o0, d)
        got = ctx.addWeightBi(a, b, w, h, w0, w1, o0, o1, d).reshape(h, w)
        assert np.array_equal(got, wo.weight_bi_vec(a, b, w0, w1, o0, o1, d, B)), ("bi", it, w0, w1, o0, o1, d)
    e = wo.random_entry(rng)  # and against the member-by-member form, once per size
    got = ctx.addWeightBi(full[0], full[1], w, h, e[0][0], e[0][1], e[1][0], e[1][1], e[2][0]).reshape(h, w)
    want = wo.add_weight_bi_loop([full[0][:8, :8]] * 3, [full[1][:8, :8]] * 3, ([e[0][0]] * 3, [e[1][0]] * 3, [e[2][0]] * 3),
                                 ([e[0][1]] * 3, [e[1][1]] * 3, [e[2][0]] * 3), B)[0]
    assert np.array_equal(got[:8, :8], want)


def test_scalar_entries_at_the_clips(ctx):
    B, n = ctx.bit_depth, 0
    for cb, kind, args, want in wo.CLIP_CASES:
        if cb != B:
            continue
        if kind == "uni":
            got = ctx.addWeightUni(np.full(16, args[0], np.int16), 4, 4, *args[1:])
        else:
            got = ctx.addWeightBi(np.full(16, args[0], np.int16), np.full(16, args[1], np.int16), 4, 4, *args[2:])
        assert (got == want).all(), (kind, args, want, got[0])
        n += 1
    assert n == sum(c[0] == B for c in wo.CLIP_CASES) > 0
    # strided source and destination: the rows beside the block stay untouched
    rng = np.random.default_rng(5150 + B)
    a = rng.integers(-8192, 8192, (6, 11)).astype(np.int16)
    d = np.full((6, 13), -7, np.int16)
    ctx._chk(capi.lib().hmx_addWeightUni(ctx.h, a.ctypes.data, 11, d.ctypes.data, 13, 8, 6, 37, -9, 5))
    assert np.array_equal(d[:, :8], wo.weight_uni_vec(a[:, :8], 37, -9, 5, B)) and (d[:, 8:] == -7).all()


# ---- 2. one prediction unit per call ----
def test_motion_compensation_wp_one_unit(ctx):
    B = ctx.bit_depth
    rng = np.random.default_rng(5200 + B)
    W, H, M = 96, 80, 24
    refs = [[rng.integers(0, 1 << B, ((H >> ch) + 2 * (M >> ch), (W >> ch) + 2 * (M >> ch))).astype(np.int16) for ch in (0, 1, 1)] for _ in range(2)]

    def pic_of(planes):
        p = capi.Pic()
        for k, a in enumerate(planes):
            m = M >> (1 if k else 0)
            p.plane[k], p.stride[k] = a.ctypes.data + 2 * (m * a.shape[1] + m), a.shape[1]
        return p

    shapes = [(8, 8), (16, 4), (4, 16), (32, 24), (64, 16), (8, 4)]
    n = 0
    for it in range(20):
        w, h = shapes[it % len(shapes)]
        x, y = int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4
        mv = [[int(rng.integers(-4 * (M - 8), 4 * (M - 8) + 1)) for _ in range(2)] for _ in range(2)]
        if it < 16:
            mv[0] = [(mv[0][0] & ~3) | (it & 3), (mv[0][1] & ~3) | (it >> 2)]  # every luma phase once
        use = [(1, 0), (0, 1), (1, 1)][it % 3]
        same = it >= 18  # both lists on the SAME picture with EQUAL vectors: still the bi formula, no identical-motion shortcut
        if same:
            use, mv[1] = (1, 1), list(mv[0])
        denoms = [int(v) for v in rng.integers(0, 8, 3)]
        e = [fade_entry(rng, denoms), fade_entry(rng, denoms)] if it % 2 else [wo.random_entry(rng), wo.random_entry(rng)]
        if same:
            e[1] = (e[1][0], [o + 3 for o in e[1][1]], e[1][2])
        r = [refs[0], refs[0] if same else refs[1]]
        pus = np.zeros(1, ol.PU_DTYPE)
        pus[0] = (x, y, w, h, 0 if use[0] else 255, 1 if use[1] else 255, mv[0][0], mv[0][1], mv[1][0], mv[1][1])
        want = wo.mc_frame_wp(pus, [(r[0], M), (r[1], M)], ([e[0], e[0]], [e[1], e[1]]), B)
        dst = [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
        dp = capi.Pic()
        for k in range(3):
            dp.plane[k], dp.stride[k] = dst[k].ctypes.data, dst[k].shape[1]
        ctx.motion_compensation_wp(pic_of(r[0]) if use[0] else None, mv[0], pic_of(r[1]) if use[1] else None, mv[1], x, y, w, h, dp,
                                   capi.wp_entry(*e[0]) if use[0] else None, capi.wp_entry(*e[1]) if use[1] else None)
        for k in range(3):
            ch = 1 if k else 0
            assert np.array_equal(dst[k], want[k][y >> ch:(y + h) >> ch, x >> ch:(x + w) >> ch]), ("motionCompensation_wp", it, k, use, e)
        n += 1
    assert n == 20


# ---- 3. and 4. the batch entry ----
PIC_W, PIC_H, MARGIN = 72, 40, 80  # 72: not a multiple of the 64-wide workgroup tile; margins as tests/test_gpu_parity.py
#        x   y   w   h  ref0 ref1 mv0x mv0y mv1x mv1y
PUS = [(0, 0, 16, 16, 0, 255, 0, 0, 0, 0),          # list 0, integer vector
       (16, 0, 8, 8, 255, 1, 0, 0, 5, 0),           # list 1 only, horizontal fraction only; one merged 4x8 cell pair per column
       (24, 0, 8, 4, 1, 255, 0, -6, 0, 0),          # two 8x4 stacked in one cell pair with different references: the split path
       (24, 4, 8, 4, 3, 255, 7, 9, 0, 0),           # reference 3 = the picture of reference 1 with other weights
       (32, 0, 4, 8, 0, 2, -13, 3, 18, -1),         # 4x8, both lists
       (36, 0, 4, 8, 2, 255, 2, 2, 0, 0),
       (40, 0, 16, 16, 1, 3, 21, -10, -4, 0),       # both lists on one picture entered twice
       (56, 0, 16, 16, 2, 2, 9, -7, 9, -7),         # both lists, same picture, same vector: the bi formula all the same
       (16, 8, 8, 8, 255, 2, 0, 0, -3, -64),
       (24, 8, 8, 4, 0, 1, 8, 4, 0, 7),             # the cell below it is not covered: pi1 = -1
       (32, 8, 8, 8, 255, 3, 0, 0, 31, 30),
       (0, 16, 16, 16, 255, 0, 0, 0, -22, 0),
       (16, 16, 16, 16, 3, 1, 1, 0, 0, 1),
       (32, 16, 64, 32, 0, 1, -17, 6, 12, -9),      # 64x32 cut by the right and the bottom picture edge
       (0, 32, 8, 8, 2, 255, 6, 5, 0, 0),
       (8, 36, 8, 4, 1, 0, -1, -1, 3, 3),           # the cell above it is not covered: pi0 = -1
       (16, 32, 16, 8, 0, 255, 64, -64, 0, 0)]


@functools.lru_cache(maxsize=None)
def scene(B):
    """Reference pictures (three pictures, the second entered twice), margin-extended planes for the oracle, two sets of tables and
    the oracle's pictures for them; computed once per bit depth and shared (read-only) by the batch tests."""
    rng = np.random.default_rng(5300 + B)
    w, h, m = PIC_W, PIC_H, MARGIN
    pics = [[rng.integers(0, 1 << B, (h >> ch, w >> ch)).astype(np.int16) for ch in (0, 1, 1)] for _ in range(3)]
    order = [0, 1, 2, 1]
    ext = [([np.pad(p, m >> (1 if k else 0), mode="edge") for k, p in enumerate(pics[i])], m) for i in order]
    pus = np.zeros(len(PUS), ol.PU_DTYPE)
    for i, t in enumerate(PUS):
        pus[i] = t
    tabs = []
    for k in range(2):
        denoms = [int(v) for v in rng.integers(1, 8, 3)]
        l0 = [fade_entry(rng, denoms) for _ in range(3)] + [wo.random_entry(rng)]
        l1 = [fade_entry(rng, denoms), wo.random_entry(rng), fade_entry(rng, [int(v) for v in rng.integers(0, 8, 3)]), fade_entry(rng, denoms)]
        tabs.append((l0, l1))
    want = [wo.mc_frame_wp(pus, ext, t, B) for t in tabs]
    want_sub = wo.mc_frame_wp(pus[:9], ext, tabs[1], B)
    for a in [p for pl in pics for p in pl] + [p for e, _ in ext for p in e] + [p for ws in want + [want_sub] for p in ws]:
        a.setflags(write=False)
    return dict(pics=pics, order=order, ext=ext, pus=pus, tabs=tabs, want=want, want_sub=want_sub)


class Device:
    """The scene on the device: references with extended borders; destinations WITH margins, so that the part of a unit
    beyond the picture edge, which the one-wave-per-PU schedule writes, lands in allocated memory."""

    def __init__(self, ctx, S, size=(PIC_W, PIC_H, MARGIN)):
        L, (w, h, m) = capi.lib(), size
        self.ctx, self.size = ctx, size
        self.pics = [capi.DevPicture(ctx, w, h, m, m).upload(p) for p in S["pics"]]
        for d in self.pics:
            ctx._chk(L.hmx_pic_extend_border(ctx.h, C.byref(d.as_pic()), w, h, m, m))
        self.refs = (capi.Pic * 4)(*[self.pics[i].as_pic() for i in S["order"]])
        self.d_pus = ctx.to_device(S["pus"])
        self.dst, self.keep = [], []

    def jobs(self, counts, mapped):
        arr = (capi.McJob * len(counts))()
        self.dst_pics = (capi.Pic * len(counts))()
        self.keep.append(self.dst_pics)
        w, h, m = self.size
        for q, n in enumerate(counts):
            d = capi.DevPicture(self.ctx, w, h, m, m).zero()
            self.dst.append(d)
            self.dst_pics[q] = d.as_pic()
            arr[q].d_pus, arr[q].n_pus, arr[q].refs, arr[q].n_refs = self.d_pus.ptr, n, self.refs, 4
            arr[q].dst, arr[q].pic_w, arr[q].pic_h = C.pointer(self.dst_pics[q]), (w if mapped else 0), (h if mapped else 0)
        return arr, self.dst[-len(counts):]

    def free(self):
        self.ctx.sync()
        for d in self.pics + self.dst:
            d.free()
        self.d_pus.free()


@pytest.mark.parametrize("mapped", [True, False], ids=["cell_map", "wave_per_pu"])
def test_batch_vs_oracle(ctx, mapped):
    B = ctx.bit_depth
    S = scene(B)
    dev = Device(ctx, S)
    l0, l1 = S["tabs"][0]
    jobs, dst = dev.jobs([len(S["pus"])], mapped)
    ctx.batch_motion_compensation_wp(jobs, [(table(l0), table(l1))])
    ctx.sync()
    got = dst[0].download()
    for p in range(3):
        assert np.array_equal(got[p], S["want"][0][p]), ("plane", p, np.argwhere(got[p] != S["want"][0][p])[:4])
    dev.free()


@pytest.mark.parametrize("mapped", [True, False], ids=["cell_map", "wave_per_pu"])
def test_mixed_call(ctx, mapped):
    """Three jobs of different length in one call, the middle one with NULL tables: the weighted jobs equal the oracle, the
    unweighted one what hmx_batch_motionCompensation_multi writes for it."""
    B, L = ctx.bit_depth, capi.lib()
    S = scene(B)
    dev = Device(ctx, S)
    counts = [len(S["pus"]), 13, 9]
    jobs, dst = dev.jobs(counts, mapped)
    ctx.batch_motion_compensation_wp(jobs, [tuple(table(t) for t in S["tabs"][0]), None, tuple(table(t) for t in S["tabs"][1])])
    plain_jobs, plain_dst = dev.jobs([13], mapped)
    ctx._chk(L.hmx_batch_motionCompensation_multi(ctx.h, 1, plain_jobs))
    ctx.sync()
    for q, want in ((0, S["want"][0]), (2, S["want_sub"])):
        got = dst[q].download()
        for p in range(3):
            assert np.array_equal(got[p], want[p]), ("weighted job", q, p)
    a, b = dst[1].download(with_margins=True), plain_dst[0].download(with_margins=True)
    for p in range(3):
        assert np.array_equal(a[p], b[p]), ("unweighted job", p)
    assert any(a[p].any() for p in range(3))
    # P slice: no list 1 table, no unit on list 1
    uni = S["pus"][[0, 2, 3, 5, 14, 16]]
    d_uni = ctx.to_device(uni)
    jobs1, dst1 = dev.jobs([len(uni)], mapped)
    jobs1[0].d_pus = d_uni.ptr
    ctx.batch_motion_compensation_wp(jobs1, [(table(S["tabs"][0][0]), None)])
    ctx.sync()
    want = wo.mc_frame_wp(uni, S["ext"], (S["tabs"][0][0], None), B)
    got = dst1[0].download()
    for p in range(3):
        assert np.array_equal(got[p], want[p]), ("P slice", p)
    dev.free()
    d_uni.free()


# ---- the batch entry on the reference's results ----
@pytest.mark.parametrize("mapped", [True, False], ids=["cell_map", "wave_per_pu"])
@pytest.mark.parametrize("B", [8, 10, 12])
def test_batch_vs_reference_vectors(B, mapped):
    """The unit list of wp_b*.npz (136x72: partial tiles in both directions, AMP shapes, 64x64, height-4 pairs with different rows,
    a picture entered in refs[] twice) with pic_w = 0 and with the picture size, and the same weighted job beside an unweighted job
    of the same list in one call."""
    _, S = wc.load_vectors(B)
    L = capi.lib()
    c = capi.Context(bit_depth=B)
    try:
        dev = Device(c, S, (wc.PIC_W, wc.PIC_H, wc.MARGIN))
        tabs = (table(S["l0"]), table(S["l1"]))
        n = len(S["pus"])
        jobs, dst = dev.jobs([n], mapped)
        c.batch_motion_compensation_wp(jobs, [tabs])
        jobs3, dst3 = dev.jobs([n, n, n], mapped)
        c.batch_motion_compensation_wp(jobs3, [None, tabs, None])
        plain_jobs, plain_dst = dev.jobs([n], mapped)
        c._chk(L.hmx_batch_motionCompensation_multi(c.h, 1, plain_jobs))
        c.sync()
        for what, d in (("alone", dst[0]), ("between unweighted jobs", dst3[1])):
            got = d.download()
            for p in range(3):
                assert np.array_equal(got[p], S["want"][p]), (what, p, np.argwhere(got[p] != S["want"][p])[:4])
        plain = plain_dst[0].download(with_margins=True)
        assert any((a != b).any() for a, b in zip(plain_dst[0].download(), S["want"]))  # the weights matter on this list
        for q in (0, 2):
            got = dst3[q].download(with_margins=True)
            for p in range(3):
                assert np.array_equal(got[p], plain[p]), ("unweighted job", q, p)
        dev.free()
    finally:
        c.close()


# ---- 5. host validation ----
def test_host_validation(ctx):
    L = capi.lib()
    S = scene(ctx.bit_depth)
    dev = Device(ctx, S)
    jobs, dst = dev.jobs([len(S["pus"])], True)
    good = [([64, 64, 64], [0, 0, 0], [6, 6, 6])] * 4

    def rc_of(tables):
        arr, keep = capi.mc_wp_array(tables)
        rc = L.hmx_batch_motionCompensation_wp_multi(ctx.h, 1, jobs, arr)
        return rc, L.hmx_last_error(ctx.h).decode()

    for bad in (([64, 64, 64], [0, 0, 0], [6, 8, 6]), ([64, 256, 64], [0, 0, 0], [6, 6, 6]), ([-129, 64, 64], [0, 0, 0], [6, 6, 6]),
                ([64, 64, 64], [0, 0, 128], [6, 6, 6]), ([64, 64, 64], [-129, 0, 0], [6, 6, 6])):
        for lst in (0, 1):
            t = [table(good), table(good)]
            t[lst] = table(good[:2] + [bad] + good[3:])
            rc, msg = rc_of([tuple(t)])
            assert rc == -1 and "hmx_batch_motionCompensation_wp_multi" in msg, (bad, lst, rc, msg)
    rc, msg = rc_of([(None, table(good))])  # units use list 0, its table is missing
    assert rc == -1 and "l0" in msg
    assert L.hmx_batch_motionCompensation_wp_multi(ctx.h, 1, jobs, None) == -1
    ctx.sync()
    assert not any(p.any() for p in dst[0].download(with_margins=True))  # refused before any launch
    # the scalar entries and the single unit
    a, d = np.zeros(16, np.int16), np.zeros(16, np.int16)
    for args in ((256, 0, 0), (-129, 0, 0), (1, 128, 0), (1, -129, 0), (1, 0, 8), (1, 0, -1)):
        assert L.hmx_addWeightUni(ctx.h, a.ctypes.data, 4, d.ctypes.data, 4, 4, 4, *args) == -1, args
        assert "hmx_addWeightUni" in L.hmx_last_error(ctx.h).decode()
    for args in ((256, 1, 0, 0, 0), (1, -129, 0, 0, 0), (1, 1, 128, 0, 0), (1, 1, 0, -129, 0), (1, 1, 0, 0, 8)):
        assert L.hmx_addWeightBi(ctx.h, a.ctypes.data, 4, a.ctypes.data, 4, d.ctypes.data, 4, 4, 4, *args) == -1, args
    assert L.hmx_addWeightUni(ctx.h, None, 4, d.ctypes.data, 4, 4, 4, 1, 0, 0) == -1
    pic, mv = capi.Pic(), (C.c_int * 2)(0, 0)
    for k in range(3):
        pic.plane[k], pic.stride[k] = a.ctypes.data, 4
    ok, bad = capi.wp_entry([1, 1, 1], [0, 0, 0], [0, 0, 0]), capi.wp_entry([1, 1, 1], [0, 0, 0], [0, 0, 8])
    assert L.hmx_motionCompensation_wp(ctx.h, C.byref(pic), mv, None, None, 0, 0, 4, 4, C.byref(pic), None, None) == -1  # entry missing
    assert L.hmx_motionCompensation_wp(ctx.h, C.byref(pic), mv, None, None, 0, 0, 4, 4, C.byref(pic), C.byref(bad), None) == -1
    assert L.hmx_motionCompensation_wp(ctx.h, C.byref(pic), mv, C.byref(pic), mv, 0, 0, 4, 4, C.byref(pic), C.byref(ok), C.byref(bad)) == -1
    dev.free()
