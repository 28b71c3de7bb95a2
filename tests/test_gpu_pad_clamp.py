"""The index-clamp form of the reference-line padding (kFtuPadsSimple: refs_gather_pad and the 4x4 lane chain) cannot change a
result: whole-picture parity against the oracle, levels and reconstruction, encoder and decoder direction.

Pictures of 128x64 (two CTUs) and 64x64 (one), three per call in ONE packing group, 8 and 10 bit, uniform tilings 4, 8, 16, 32 and
the mix.  A wave-item takes one of three paths -- no block pads, every padding block is simple (the clamp), some padding block is not
(the general pass) -- so the decisions are chosen to give wave-items of each kind:
  p  every block gets a mode whose padding is simple where one exists: wave-items of simple padders only
  q  the generator's random modes: simple padders beside blocks that do not pad
  r  the modes of q under constrained intra prediction on a random 8x8 intra map (and, 128 wide, two tiles): units missing BETWEEN
     available ones, the only way to a block that is not simple
The first block of a picture has no neighbour at all (the empty mask).  Every packed call's items are downloaded and
hmx_intra_reads_unavailable / hmx_intra_pads_simple evaluated per item: over a tiling's calls all four kinds must have occurred.

The oracle: hmo_intra_frame_encode for p and q; for r the same chain composed block by block from the oracle's pieces with the
layout's flags (tests/layout_oracle.py gives them; _oracle_encode below, held against hmo_intra_frame_encode on a case without a
layout).  Every call runs over a zeroed and over a pseudo-random reconstruction, as tests/test_gpu_ref_skips.py does: a position
the clamp left stale and a prediction read shows in one of the two.  Host-built and device-built plans must carry the same two
bits per block (hmx_intra_plan_pad_bits) and give the same pictures on r."""
import ctypes as C
import functools

import numpy as np
import pytest

import layout_oracle as LO
import oracle_lib as ol
from thevc_amd import capi, workload
from thevc_amd import decisions as D

pytestmark = pytest.mark.gpu

PICS = [(128, 64), (64, 64)]
QP, N_PICS = 30, 3
TILINGS = [4, 8, 16, 32, "mix"]
SHAPES = [(16, 8), (64, 16)]  # 4x4 and 8x8 blocks per wave-item of the packed schedule
PAD_MODES = [2, 34, 18, 10, 26, 0, 1]  # below-left first, above-right next: the units most often missing


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _bits(n, luma, mode, mask):
    L = capi.lib()
    return L.hmx_intra_reads_unavailable(n, luma, mode, mask), L.hmx_intra_pads_simple(n, luma, mode, mask)


@functools.lru_cache(maxsize=None)
def _layout(w, h, pic):
    """(region, intra) of decision r: a random intra map on the 8x8 grid; two tiles where the picture has two CTUs"""
    rng = np.random.default_rng(7700 + w + pic)
    g = (rng.random((h // 8, w // 8)) < 0.6).astype(np.uint8)
    intra = np.ascontiguousarray(np.kron(g, np.ones((2, 2), np.uint8)))
    region = D.region_map(w, h, 64, [0], [0, 1], [0]) if w > 64 else None
    return region, intra


def _decisions(w, h, tiling, decision, pic):
    tus = workload.make_tus(9500 + 10 * pic + TILINGS.index(tiling) + w, w, h, tiling)
    if decision != "p":
        return tus
    L = capi.lib()
    t = tus.copy()
    for b in t:
        sh = 1 if b["plane"] else 0
        n = 1 << int(b["log2n"])
        avail = L.hmx_intra_avail_mask_layout(int(b["x"]) << sh, int(b["y"]) << sh, n << sh, w, h, None)
        for mode in PAD_MODES:
            if _bits(n, int(b["plane"] == 0), mode, avail) == (1, 1):
                b["mode"] = mode
                break
    return t


def _oracle_encode(tus, org, w, h, B, region, intra):
    """hmo_intra_frame_encode's chain, block by block, with the availability flags of a layout"""
    O = ol.oracle()
    rec = [np.zeros_like(p) for p in org]
    lev = [np.zeros(p.shape, np.int32) for p in org]
    reg = None if region is None else LO.Region(region, w)
    mx = (1 << B) - 1
    for t in tus:
        k, N, x, y, mode, ts = int(t["plane"]), 1 << int(t["log2n"]), int(t["x"]), int(t["y"]), int(t["mode"]), int(t["flags"]) & 1
        f = LO.block_flags(t, w, h, reg, intra)
        flags = np.zeros(65, np.uint8)
        flags[:f.size] = f
        plane, stride = rec[k].reshape(-1), rec[k].shape[1]
        W = 2 * N + 1
        adi = np.zeros(2 * W * W, np.int32)
        O.hmo_fillReferenceSamples(ol.ptr(plane, y * stride + x), stride, flags, int(f.sum()), 2 if k else 4, N, B, adi)
        pred = np.zeros((N, N), np.int16)
        if k:
            O.hmo_predIntraChromaAng(adi, mode, pred.reshape(-1), N, N, B)
        else:
            O.hmo_filterAdi(adi, N)
            O.hmo_predIntraLumaAng(adi, mode, pred.reshape(-1), N, N, B)
        q = O.hmo_setQPforQuant(QP, int(k != 0), 6 * (B - 8), 0)
        cfg = ol.quant_cfg(q.per, q.rem, 1, 1, O.hmo_coef_scan_idx(N, int(k == 0), 1, mode))
        tmode = mode if k == 0 else 65535
        resi = (org[k][y:y + N, x:x + N].astype(np.int32) - pred).astype(np.int16)
        lvl, abs_sum = ol.o_transformNxN(resi, N, B, tmode, ts, cfg)
        r = ol.o_invtransformNxN(lvl, N, B, tmode, q.per, q.rem, ts) if abs_sum else np.zeros((N, N), np.int16)
        rec[k][y:y + N, x:x + N] = np.clip(pred.astype(np.int32) + r, 0, mx)
        lev[k][y:y + N, x:x + N] = lvl
    return rec, lev


@functools.lru_cache(maxsize=None)
def _case(w, h, tiling, decision, B):
    """(decisions, layouts, originals, the oracle's (reconstruction, levels)) of the three pictures; computed once, never modified"""
    tus = [_decisions(w, h, tiling, decision, i) for i in range(N_PICS)]
    orgs = [workload.make_planes(9600 + i, w, h, B, "texture" if i % 2 else "noise") for i in range(N_PICS)]
    if decision == "r":
        lays = [_layout(w, h, i) for i in range(N_PICS)]
        want = [_oracle_encode(tus[i], orgs[i], w, h, B, *lays[i]) for i in range(N_PICS)]
    else:
        lays = None
        want = [ol.o_intra_frame_encode(tus[i], w, h, B, QP, orgs[i]) for i in range(N_PICS)]
    return tus, lays, orgs, want


@functools.lru_cache(maxsize=None)
def _prefill(w, h, B, kind):
    if kind == 0:
        return [np.zeros((h, w), np.int16), np.zeros((h // 2, w // 2), np.int16), np.zeros((h // 2, w // 2), np.int16)]
    return workload.make_planes(9700, w, h, B, "noise")


def _call(ctx, w, h, plans, orgs, want, prefill, decode):
    L, n = capi.lib(), len(orgs)
    d_org = [capi.DevPicture(ctx, w, h).upload(o) for o in orgs]
    d_rec = [capi.DevPicture(ctx, w, h).upload(prefill) for _ in range(n)]
    d_lev = [capi.DevPicture(ctx, w, h, dtype=np.int32) for _ in range(n)]
    for i, d in enumerate(d_lev):
        d.upload(want[i][1]) if decode else d.zero()
    A = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
    parr = (C.c_void_p * n)(*[p.value for p in plans])
    try:
        if decode:
            ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, parr, n, A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        else:
            ctx._chk(L.hmx_frame_intra_encode_multi(ctx.h, parr, n, A(d_org, capi.Pic), A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        ctx.sync()
        return [(d_rec[i].download(), d_lev[i].download()) for i in range(n)]
    finally:
        for d in d_org + d_rec + d_lev:
            d.free()


def _check(got, want, what):
    for i in range(len(want)):
        for p in range(3):
            assert np.array_equal(got[i][1][p], want[i][1][p]), ("levels",) + what + (i, p)
            assert np.array_equal(got[i][0][p], want[i][0][p]), ("reconstruction",) + what + (i, p)


KINDS = ("simple padders only", "simple padders beside blocks that do not pad", "a block that is not simple", "an empty mask")


def _wave_item_kinds(tables):
    """how many wave-items of a packed call are of each of KINDS.  An item carries the dependency mask, for which the two functions
    give the bits of the availability (tests/test_intra_pads_simple.py)."""
    _, _, _, descs, items, _ = tables
    out = [0, 0, 0, 0]
    for d in descs:
        n, off = int(d["n_s"]) & 0x0fffffff, int(d["item_off"])
        blk = items[off:off + n]
        bits = [_bits(1 << int(b["log2n"]), int((int(b["plane"]) & 3) == 0), int(b["mode"]), int(b["avail"])) for b in blk]
        pads, simple = [p for p, _ in bits], [s for p, s in bits if p]
        if any(pads) and all(simple):
            out[0 if all(pads) else 1] += 1
        if not all(simple):
            out[2] += 1
        out[3] += any(int(b["avail"]) == 0 for b in blk)
    return out


def _set_shape(ctx, hmx_opts, shape):
    hmx_opts(ctx, HMX_INTRA_SCHEDULE=None, HMX_PACK_GROUP="3", HMX_PACK_SLOTS4=str(shape[0]), HMX_PACK_SLOTS8=str(shape[1]))


def test_block_by_block_oracle_is_the_frame_oracle():
    """_oracle_encode without a layout is hmo_intra_frame_encode (the composition used for decision r adds the flags only)"""
    w, h, B = 64, 64, 10
    tus, _, orgs, want = _case(w, h, "mix", "q", B)
    rec, lev = _oracle_encode(tus[0], orgs[0], w, h, B, None, None)
    for p in range(3):
        assert np.array_equal(rec[p], want[0][0][p]) and np.array_equal(lev[p], want[0][1][p])


@pytest.mark.parametrize("tiling", TILINGS)
def test_pad_clamp_parity(ctx, hmx_opts, tiling):
    L, B = capi.lib(), ctx.bit_depth
    kinds = [0, 0, 0, 0]  # over both picture sizes
    for w, h in PICS:
        pp = capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1)
        for decision in "pqr":
            tus, lays, orgs, want = _case(w, h, tiling, decision, B)
            plans = ctx.intra_plans(tus, pp, None if lays is None else [capi.Layout(*l) for l in lays])
            try:
                for shape in SHAPES:
                    _set_shape(ctx, hmx_opts, shape)
                    for fill in (0, 1):
                        got = _call(ctx, w, h, plans, orgs, want, _prefill(w, h, B, fill), decode=False)
                        sched = C.c_int()
                        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
                        assert sched.value == 3, (shape, sched.value)  # the packed schedule
                        if fill == 0:
                            k = _wave_item_kinds(ctx.pack_tables())
                            print(f"{w}x{h} tiling {tiling} {B} bit, {decision}, slots {shape}: wave-items {dict(zip(KINDS, k))}")
                            kinds = [a + b for a, b in zip(kinds, k)]
                        _check(got, want, (w, h, tiling, B, decision, shape, fill, "encode"))
                        got = _call(ctx, w, h, plans, orgs, want, _prefill(w, h, B, fill), decode=True)
                        _check(got, want, (w, h, tiling, B, decision, shape, fill, "decode"))
            finally:
                L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * N_PICS)(*[p.value for p in plans]), N_PICS)
    for name, k in zip(KINDS, kinds):
        assert k > 0, f"tiling {tiling}: no wave-item with {name}"


@pytest.mark.parametrize("pic", PICS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_pad_clamp_device_built_plans(ctx, hmx_opts, pic):
    """device-built plans set the two bits as host-built ones do -- with and without a layout -- and give the same pictures on r"""
    L, B = capi.lib(), ctx.bit_depth
    w, h = pic
    pp = capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1)
    _set_shape(ctx, hmx_opts, SHAPES[1])
    for decision in "qr":
        tus, lays, orgs, want = _case(w, h, "mix", decision, B)
        layouts = None if lays is None else [capi.Layout(*l) for l in lays]
        host = ctx.intra_plans(tus, pp, layouts)
        cat = np.ascontiguousarray(np.concatenate(tus), capi.TU_DTYPE)
        offs = np.concatenate([[0], np.cumsum([len(t) for t in tus])])
        d = ctx.to_device(cat)
        dev = ctx.intra_plans_device(d.ptr, offs, pp) if layouts is None else ctx.intra_plans_device_layout(d.ptr, offs, pp, layouts)
        d.free()
        try:
            seen = set()
            for a, b in zip(host, dev):
                assert np.array_equal(ctx.plan_tables(a)[0], ctx.plan_tables(b)[0])
                ba, bb = ctx.plan_pad_bits(a), ctx.plan_pad_bits(b)
                assert np.array_equal(ba, bb), (decision, np.flatnonzero(ba != bb)[:8])
                blocks = ctx.plan_tables(a)[0]
                for blk, bit in zip(blocks, ba):  # and they are the exported predicates of the stored mask
                    p, s = _bits(1 << int(blk["log2n"]), int(blk["plane"] == 0), int(blk["mode"]), int(blk["avail"]))
                    assert int(bit) == p | (s << 1), (decision, blk, bit)
                seen |= set(int(v) for v in ba)
            assert seen == ({0, 1, 3} if decision == "r" else {0, 3}), (decision, seen)  # r: blocks that pad and are not simple
            for fill in (0, 1):
                got = _call(ctx, w, h, dev, orgs, want, _prefill(w, h, B, fill), decode=False)
                _check(got, want, (pic, B, decision, "device", fill, "encode"))
                got = _call(ctx, w, h, dev, orgs, want, _prefill(w, h, B, fill), decode=True)
                _check(got, want, (pic, B, decision, "device", fill, "decode"))
        finally:
            for p in list(host) + list(dev):
                L.hmx_intra_plan_destroy(ctx.h, p)
