"""The batched loop filters (hmx_deblock_strengths_multi, hmx_deblock_picture_multi, hmx_sao_picture_multi; include/hmx.h)
against the oracle (hmo_deblock_strengths, hmo_deblock_picture, hmo_sao_picture, which tests/test_oracle_vs_ref.py pins to the
compiled reference), sample for sample, and against the single-picture entries."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as ol

P3, I3 = C.c_void_p * 3, C.c_int * 3
vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
SENTINEL = 0x1234  # what lies around a picture in its allocation: margins, row padding, the skew elements
# plane layouts (capi.DevPicture): the reference's margins, an odd stride, planes that start on an odd element, 16-byte aligned
SHAPES = [dict(), dict(mx=32, my=16), dict(pad=1), dict(skew=1, pad=1, mx=8, my=8), dict(skew=1)]
shape_of = lambda i: SHAPES[(2 * i + 3) % 5]


@pytest.fixture(scope="module", params=[8, 10])
def lctx(request):
    from thevc_amd import capi
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


def upload(ctx, planes, w, h, **kw):
    """a DevPicture whose allocation holds SENTINEL everywhere outside the picture"""
    from thevc_amd import capi
    pic = capi.DevPicture(ctx, w, h, **kw)
    for p in range(3):
        pw, ph, pmx, pmy = pic.dims[p]
        flat = np.full(pic.elems[p], SENTINEL, np.int16)
        full = flat[pic.skew:].reshape(ph + 2 * pmy, pic.strides[p])
        full[pmy:pmy + ph, pmx:pmx + pw] = planes[p]
        pic.bufs[p].upload(flat)
    return pic


def surroundings_intact(pic):
    for p in range(3):
        pw, ph, pmx, pmy = pic.dims[p]
        flat = pic.bufs[p].download(np.int16)[:pic.elems[p]].copy()
        flat[pic.skew:].reshape(ph + 2 * pmy, pic.strides[p])[pmy:pmy + ph, pmx:pmx + pw] = SENTINEL
        if not (flat == SENTINEL).all():
            return False
    return True


# ---- deblocking ----

def dbk_inputs(rng, w, h, B, every_edge=False):
    """content and maps as tests/test_gpu_parity.py::test_deblock_picture_vs_oracle makes them (blocks of 8x8 with steps, a ramp
    and noise; random strengths, per-8x8 QPs, no-filter units).  every_edge: strength 2 on every edge, QP 45..51.
    A picture below 128 samples has few edges (64x64: 7 + 7 luma and 3 + 3 chroma edges per plane, at most 384 chroma samples
    that can change), so there two strengths in three are 2, QPs start at 30 and the noise is +-1: the guard of test_deblock_batch
    (1000 luma and 100 chroma samples changed) then holds with the beta and tc offsets at -6 too."""
    small = min(w, h) < 128
    mx = (1 << B) - 1
    uw, uh = w // 4, h // 4
    c8 = lambda n: -(-n // 8)
    ramp = (np.arange(w)[None, :] // 8 + np.arange(h)[:, None] // 8) * (1 << (B - 8))
    y = np.clip(rng.integers(0, 30 << (B - 8), (h // 8, w // 8)).repeat(8, 0).repeat(8, 1) + rng.integers(-1, 2, (h, w)) * (1 if small else 2) + (60 << (B - 8)) + ramp, 0, mx).astype(np.int16)
    chroma = lambda: np.clip(rng.integers(0, mx // 3, (c8(h // 2), c8(w // 2))).repeat(8, 0).repeat(8, 1)[:h // 2, :w // 2] + rng.integers(0, 6, (h // 2, w // 2)), 0, mx).astype(np.int16)
    cb, cr = chroma(), chroma()
    if every_edge:
        bsv, bsh = np.full((uh, uw), 2, np.uint8), np.full((uh, uw), 2, np.uint8)
        qp = rng.integers(45, 52, (uh // 2, uw // 2)).repeat(2, 0).repeat(2, 1).astype(np.int8)
    else:
        strength = lambda: (np.minimum(rng.integers(0, 6, (uh, uw)), 2) if small else rng.integers(0, 3, (uh, uw))).astype(np.uint8)
        bsv, bsh = strength(), strength()
        qp = rng.integers(30 if small else 10, 52, (uh // 2, uw // 2)).repeat(2, 0).repeat(2, 1).astype(np.int8)
    bsv[:, 0] = 0
    bsh[0, :] = 0
    nof = (rng.random((uh // 2, uw // 2)) < (0.05 if small else 0.15)).repeat(2, 0).repeat(2, 1).astype(np.uint8)
    return dict(planes=[y, cb, cr], bsv=bsv, bsh=bsh, qp=qp, nof=nof)


def oracle_deblock(d, w, h, B, use_nof, boff, toff):
    out = [p.copy() for p in d["planes"]]
    ol.oracle().hmo_deblock_picture(P3(*[p.ctypes.data for p in out]), I3(w, w // 2, w // 2), w, h, B, vp(d["bsv"]), vp(d["bsh"]), vp(d["qp"]),
                                    vp(d["nof"]) if use_nof else None, int(boff), int(toff))
    return out


def stack(ctx, pics, key):
    return ctx.to_device(np.ascontiguousarray(np.stack([d[key] for d in pics])))


def gpu_deblock(ctx, pics, w, h, use_nof, boffs, toffs, single=False):
    """the batch through hmx_deblock_picture_multi (or picture by picture through hmx_deblock_picture); returns the planes and
    whether every allocation is intact outside its picture"""
    from thevc_amd import capi
    L, n = capi.lib(), len(pics)
    dev = [upload(ctx, d["planes"], w, h, **shape_of(i)) for i, d in enumerate(pics)]
    maps = [stack(ctx, pics, k) for k in ("bsv", "bsh", "qp", "nof")]
    if single:
        u = (w // 4) * (h // 4)
        for i in range(n):
            p = dev[i].as_pic()
            ctx._chk(L.hmx_deblock_picture(ctx.h, C.byref(p), w, h, maps[0].ptr + i * u, maps[1].ptr + i * u, maps[2].ptr + i * u,
                                           maps[3].ptr + i * u if use_nof else None, 0 if boffs is None else int(boffs[i]),
                                           0 if toffs is None else int(toffs[i])))
    else:
        ctx.deblock_pictures(dev, w, h, maps[0], maps[1], maps[2], maps[3] if use_nof else None, boffs, toffs)
    ctx.sync()
    got, intact = [p.download() for p in dev], all(surroundings_intact(p) for p in dev)
    for x in dev + maps:
        x.free()
    return got, intact


# per batch size: no-filter map or NULL, beta offsets, tc offsets (None = the NULL array); -6 and +6 are the extremes
DBK_BATCH = {1: (False, None, None), 2: (False, None, [6, -6]), 3: (True, [-6, 6, 2], [6, -6, -1]), 5: (True, [0, -6, 6, 3, -4], None)}
DBK_CASES = [(n, w, h) for n in (1, 3, 5) for (w, h) in ((8, 8), (64, 64), (72, 72), (200, 136), (416, 240))] + [(2, 3840, 2160)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,w,h", DBK_CASES)
def test_deblock_batch(lctx, n, w, h):
    B = lctx.bit_depth
    rng = np.random.default_rng(1000 * n + w + h + B)
    use_nof, boffs, toffs = DBK_BATCH[n]
    pics = [dbk_inputs(rng, w, h, B) for _ in range(n)]
    want = [oracle_deblock(d, w, h, B, use_nof, 0 if boffs is None else boffs[i], 0 if toffs is None else toffs[i]) for i, d in enumerate(pics)]
    if w >= 64 and h >= 64:  # a filter that does nothing must not pass
        for d, o in zip(pics, want):
            changed = [int((a != b).sum()) for a, b in zip(d["planes"], o)]
            print("changed samples", (n, w, h), changed)
            assert changed[0] > 1000 and changed[1] > 100, changed
    got, intact = gpu_deblock(lctx, pics, w, h, use_nof, boffs, toffs)
    for i in range(n):
        for p in range(3):
            assert np.array_equal(got[i][p], want[i][p]), (i, p, np.argwhere(got[i][p] != want[i][p])[:4])
    assert intact
    one, intact = gpu_deblock(lctx, pics, w, h, use_nof, boffs, toffs, single=True)
    assert intact and all(np.array_equal(a, b) for x, y in zip(one, got) for a, b in zip(x, y))


@pytest.mark.gpu
def test_deblock_order(lctx):
    """Strength 2 on every edge and a high QP: the horizontal edges are filtered on what the vertical edges left.  The other
    order (the oracle on the transposed picture with the maps swapped, transposed back) gives a different picture."""
    B, w, h = lctx.bit_depth, 136, 72
    rng = np.random.default_rng(77 + B)
    pics = [dbk_inputs(rng, w, h, B, every_edge=True) for _ in range(2)]
    want = [oracle_deblock(d, w, h, B, False, 0, 0) for d in pics]
    for d, o in zip(pics, want):
        tr = dict(planes=[np.ascontiguousarray(p.T) for p in d["planes"]], bsv=np.ascontiguousarray(d["bsh"].T),
                  bsh=np.ascontiguousarray(d["bsv"].T), qp=np.ascontiguousarray(d["qp"].T), nof=None)
        swapped = [np.ascontiguousarray(p.T) for p in oracle_deblock(tr, h, w, B, False, 0, 0)]
        assert (swapped[0] != o[0]).sum() > 100 and (swapped[1] != o[1]).sum() > 10
    got, intact = gpu_deblock(lctx, pics, w, h, False, None, None)
    assert intact
    for i in range(2):
        for p in range(3):
            assert np.array_equal(got[i][p], want[i][p]), (i, p)


# ---- boundary strengths ----

@pytest.mark.gpu
@pytest.mark.parametrize("w,h,is_b", [(256, 192, [0, 1, 1, 0]), (200, 136, [1, 0, 1]), (64, 64, [1]), (72, 264, [0, 1])])
def test_strengths_batch(lctx, w, h, is_b):
    """P and B pictures in one batch; the heights cross CTU rows (compressed motion above a horizontal CTU boundary)"""
    import test_oracle_vs_ref as T
    from thevc_amd import capi
    L, O, n = capi.lib(), ol.oracle(), len(is_b)
    uw, uh = w // 4, h // 4
    rng = np.random.default_rng(w + h + lctx.bit_depth)
    ins = [T._dbk_units(rng, uw, uh, b) for b in is_b]
    want_v, want_h = np.zeros((n, uh, uw), np.uint8), np.zeros((n, uh, uw), np.uint8)
    for i, (units, ev, eh) in enumerate(ins):
        O.hmo_deblock_strengths(vp(units), vp(ev), vp(eh), w, h, 64, is_b[i], vp(want_v[i]), vp(want_h[i]))
    assert (want_v == 1).any() and (want_v == 2).any() and (want_h == 1).any() and (want_h == 2).any()
    d_in = [lctx.to_device(np.ascontiguousarray(np.stack([x[k] for x in ins]))) for k in range(3)]
    d_v, d_h = lctx.to_device(np.full(n * uw * uh, 9, np.uint8)), lctx.to_device(np.full(n * uw * uh, 9, np.uint8))
    lctx.deblock_strengths(n, d_in[0], d_in[1], d_in[2], w, h, is_b, d_v, d_h)
    lctx.sync()
    got_v, got_h = d_v.download(np.uint8, n * uw * uh).reshape(n, uh, uw), d_h.download(np.uint8, n * uw * uh).reshape(n, uh, uw)
    assert np.array_equal(got_v, want_v) and np.array_equal(got_h, want_h)
    u = uw * uh
    for i in range(n):  # the single-picture entry, picture by picture
        lctx._chk(L.hmx_deblock_strengths(lctx.h, d_in[0].ptr + i * u * 12, d_in[1].ptr + i * u, d_in[2].ptr + i * u, w, h, is_b[i],
                                          d_v.ptr + i * u, d_h.ptr + i * u))
    lctx.sync()
    assert np.array_equal(d_v.download(np.uint8, n * u).reshape(n, uh, uw), want_v)
    assert np.array_equal(d_h.download(np.uint8, n * u).reshape(n, uh, uw), want_h)
    for d in d_in + [d_v, d_h]:
        d.free()


# ---- SAO ----

def sao_inputs(rng, w, h, B, n_lcu):
    import test_oracle_vs_ref as T
    mx = (1 << B) - 1
    y = np.clip(rng.integers(0, mx + 1, (h // 4 + 1, w // 4 + 1)).repeat(4, 0).repeat(4, 1)[:h, :w] // 2 + rng.integers(0, 6, (h, w)), 0, mx).astype(np.int16)
    cb = rng.integers(0, mx + 1, (h // 2, w // 2)).astype(np.int16)
    cr = np.clip(rng.integers(0, 40, (h // 2, w // 2)) + mx - 30, 0, mx).astype(np.int16)
    prm = T._sao_params(rng, n_lcu)
    for c in range(3):  # every type in every component
        prm["type"][c, rng.permutation(n_lcu)[:6]] = np.arange(-1, 5)
    return [y, cb, cr], prm


def oracle_sao(planes, prm, w, h, B):
    out = [np.zeros_like(p) for p in planes]
    ol.oracle().hmo_sao_picture(P3(*[p.ctypes.data for p in planes]), P3(*[p.ctypes.data for p in out]), I3(w, w // 2, w // 2), w, h, B, 64,
                                P3(prm[0].ctypes.data, prm[1].ctypes.data, prm[2].ctypes.data))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("w,h", [(416, 240), (200, 136), (136, 72)])
def test_sao_batch(lctx, n, w, h):
    """cut CTUs at the right and bottom; chroma widths (100, 68) that are not a multiple of 8; unaligned planes"""
    from thevc_amd import capi
    L, B = capi.lib(), lctx.bit_depth
    n_lcu = -(-w // 64) * -(-h // 64)
    rng = np.random.default_rng(n + w + B)
    ins = [sao_inputs(rng, w, h, B, n_lcu) for _ in range(n)]
    for _, prm in ins:
        assert all(set(prm["type"][c]) == set(range(-1, 5)) for c in range(3))
    want = [oracle_sao(pl, prm, w, h, B) for pl, prm in ins]
    assert all((o[0] != pl[0]).sum() > 500 for o, (pl, _) in zip(want, ins))
    src = [upload(lctx, pl, w, h, **shape_of(i)) for i, (pl, _) in enumerate(ins)]
    zero = [np.zeros_like(p) for p in ins[0][0]]
    d_prm = lctx.to_device(np.ascontiguousarray(np.stack([prm for _, prm in ins])))
    for single in (False, True):
        dst = [upload(lctx, zero, w, h, **shape_of(i + 1)) for i in range(n)]
        if single:
            for i in range(n):
                a, b = src[i].as_pic(), dst[i].as_pic()
                lctx._chk(L.hmx_sao_picture(lctx.h, C.byref(a), C.byref(b), w, h, d_prm.ptr + i * 3 * n_lcu * 6, n_lcu))
        else:
            lctx.sao_pictures(src, dst, w, h, d_prm)
        lctx.sync()
        for i in range(n):
            got = dst[i].download()
            for p in range(3):
                assert np.array_equal(got[p], want[i][p]), (single, i, p, np.argwhere(got[p] != want[i][p])[:4])
            assert surroundings_intact(dst[i])
            dst[i].free()
    for x in src + [d_prm]:
        x.free()


# ---- arguments ----

def lib_error(ctx):
    from thevc_amd import capi
    return capi.lib().hmx_last_error(ctx.h).decode()


@pytest.mark.gpu
def test_arguments(lctx):
    """every HMX_ERR_ARG condition returns -1 and launches nothing; a valid call afterwards works"""
    import test_oracle_vs_ref as T
    from thevc_amd import capi
    L, B, w, h, n = capi.lib(), lctx.bit_depth, 136, 72, 2
    uw, uh, n_lcu = w // 4, h // 4, 3 * 2
    rng = np.random.default_rng(5 + B)
    pics = [dbk_inputs(rng, w, h, B) for _ in range(n)]
    dev = [upload(lctx, d["planes"], w, h, **shape_of(i)) for i, d in enumerate(pics)]
    out = [upload(lctx, [np.zeros_like(p) for p in d["planes"]], w, h) for d in pics]
    bsv, bsh, qp, nof = [stack(lctx, pics, k) for k in ("bsv", "bsh", "qp", "nof")]
    rec, dst = (capi.Pic * n)(*[p.as_pic() for p in dev]), (capi.Pic * n)(*[p.as_pic() for p in out])
    hole = (capi.Pic * n)(*[p.as_pic() for p in dev])
    hole[1].plane[2] = None
    off = (C.c_int8 * n)(2, -2)
    isb = (C.c_uint8 * n)(0, 1)
    units = [T._dbk_units(rng, uw, uh, b) for b in (0, 1)]
    d_u, d_ev, d_eh = [lctx.to_device(np.ascontiguousarray(np.stack([x[k] for x in units]))) for k in range(3)]
    d_v, d_h = lctx.to_device(np.full(n * uw * uh, 9, np.uint8)), lctx.to_device(np.full(n * uw * uh, 9, np.uint8))
    prm = np.stack([sao_inputs(rng, w, h, B, n_lcu)[1] for _ in range(n)])
    d_prm = lctx.to_device(np.ascontiguousarray(prm))

    def rejected(fn, good, bad):
        """good: a valid argument list; bad: {position: value} variants, each of which must be refused"""
        for k, vals in bad.items():
            for v in vals:
                args = list(good)
                args[k] = v
                assert fn(*args) == -1, (fn.__name__, k, v)
                if args[0] is not None:
                    assert lib_error(lctx)

    sizes = lambda iw, ih: {iw: [0, -8, 132], ih: [0, -8, 68]}
    good_d = [lctx.h, n, rec, w, h, bsv.ptr, bsh.ptr, qp.ptr, nof.ptr, off, off]
    rejected(L.hmx_deblock_picture_multi, good_d, {0: [None], 1: [0, -1, 65536], 2: [None, hole], 5: [None], 6: [None], 7: [None], **sizes(3, 4)})
    good_s = [lctx.h, n, d_u.ptr, d_ev.ptr, d_eh.ptr, w, h, isb, d_v.ptr, d_h.ptr]
    rejected(L.hmx_deblock_strengths_multi, good_s, {0: [None], 1: [0, -1, 65536], 2: [None], 3: [None], 4: [None], 7: [None], 8: [None], 9: [None],
                                                     **sizes(5, 6)})
    same = (capi.Pic * n)(dst[0], rec[1])  # in[1] and out[1] are one picture
    part = (capi.Pic * n)(dst[0], dst[1])
    part[1].plane[1] = rec[1].plane[1]  # ... share one plane
    good_a = [lctx.h, n, rec, dst, w, h, d_prm.ptr, n_lcu]
    rejected(L.hmx_sao_picture_multi, good_a, {0: [None], 1: [0, -1, 65536], 2: [None, hole], 3: [None, hole, same, part], 4: [0, -8, 135], 5: [0, -8, 71],
                                               6: [None], 7: [0, n_lcu - 1, n_lcu + 1]})
    a, b = dev[0].as_pic(), out[0].as_pic()
    assert L.hmx_sao_picture(lctx.h, C.byref(a), C.byref(a), w, h, d_prm.ptr, n_lcu) == -1
    assert L.hmx_deblock_picture(lctx.h, None, w, h, bsv.ptr, bsh.ptr, qp.ptr, None, 0, 0) == -1
    assert L.hmx_deblock_strengths(lctx.h, d_u.ptr, d_ev.ptr, d_eh.ptr, w, 68, 0, d_v.ptr, d_h.ptr) == -1
    # nothing ran: pictures, outputs and strength maps are as they were uploaded
    lctx.sync()
    for d, p, o in zip(pics, dev, out):
        assert all(np.array_equal(x, y) for x, y in zip(p.download(), d["planes"])) and surroundings_intact(p)
        assert not any(x.any() for x in o.download())
    assert (d_v.download(np.uint8, n * uw * uh) == 9).all() and (d_h.download(np.uint8, n * uw * uh) == 9).all()
    # and the valid calls, NULL no-filter map and NULL offsets included
    assert L.hmx_deblock_strengths_multi(*good_s) == 0
    assert L.hmx_sao_picture_multi(*good_a) == 0
    lctx.sync()
    for i in range(n):
        want = oracle_sao(pics[i]["planes"], prm[i], w, h, B)
        assert all(np.array_equal(x, y) for x, y in zip(out[i].download(), want))
    good_d[8:] = [None, None, None]
    assert L.hmx_deblock_picture_multi(*good_d) == 0
    lctx.sync()
    for i in range(n):
        want = oracle_deblock(pics[i], w, h, B, False, 0, 0)
        assert all(np.array_equal(x, y) for x, y in zip(dev[i].download(), want))
    for x in dev + out + [bsv, bsh, qp, nof, d_u, d_ev, d_eh, d_v, d_h, d_prm]:
        x.free()
