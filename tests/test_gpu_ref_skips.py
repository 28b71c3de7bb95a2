"""The wave-uniform skips of the reference line in the whole-picture chains (no padding pass when no block of the wave reads an
unavailable unit, no smoothed line when none predicts from it, no DC sum when none is DC) cannot change a result: whole-picture
parity against the oracle, levels and reconstruction, encoder and decoder direction, over decisions chosen so that wave-items
with and without padded blocks, with and without smoothed lines and with and without DC blocks all occur -- and mix.

Pictures: 128x128 (four CTUs), 8 and 10 bit, three pictures with their own decisions in ONE packing group; uniform tilings 4, 8, 16,
32 and the mix.  Decisions (the generator's blocks with `mode` overwritten):
  a  every block vertical (26): interior blocks read nothing unavailable
  b  luma alternating 2 and 34: below-left and above-right, many padded
  c  all DC            d  all planar            e  the generator's random modes
  f  one picture of a beside one of b and one of c in the same group: wave-items mix them
Shapes: 16 or 64 4x4 blocks and 8 or 16 8x8 blocks per wave-item of the packed schedule, and the level schedule.
Every call runs twice, the reconstruction pictures pre-filled with zeros and then with a fixed pseudo-random pattern: a skipped
pass that let a stale sample reach a prediction shows as a difference from the oracle in one of the two.
The packed calls' items are downloaded and hmx_intra_reads_unavailable is evaluated per item: over the calls of (a) and (b) every
size class must have a wave-item without a padded block and one with some, or the test says nothing about the skip."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu

W, H, QP, N_PICS = 128, 128, 30, 3
TILINGS = [4, 8, 16, 32, "mix"]
DECISIONS = "abcdef"
SHAPES = [("packed", 16, 8), ("packed", 16, 16), ("packed", 64, 8), ("packed", 64, 16), ("level", 0, 0)]


@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


def _with_modes(tus, decision, pic):
    t = tus.copy()
    d = "abc"[pic] if decision == "f" else decision
    luma = t["plane"] == 0
    if d == "a":
        t["mode"] = 26
    elif d == "b":
        t["mode"][luma] = np.where(np.arange(int(luma.sum())) % 2 == 0, 2, 34)
    elif d == "c":
        t["mode"] = 1
    elif d == "d":
        t["mode"] = 0
    return t


@functools.lru_cache(maxsize=None)
def _case(tiling, decision, B):
    """(decisions, originals, the oracle's (reconstruction, levels)) of the three pictures; computed once, never modified"""
    tus = [_with_modes(workload.make_tus(9100 + 10 * i + TILINGS.index(tiling), W, H, tiling), decision, i) for i in range(N_PICS)]
    orgs = [workload.make_planes(9200 + i, W, H, B, "texture" if i % 2 else "noise") for i in range(N_PICS)]
    want = [ol.o_intra_frame_encode(tus[i], W, H, B, QP, orgs[i]) for i in range(N_PICS)]
    return tus, orgs, want


@functools.lru_cache(maxsize=None)
def _prefill(B, kind):
    """what the reconstruction pictures hold before a call: zeros, or one fixed pseudo-random pattern in the legal range"""
    if kind == 0:
        return [np.zeros((H, W), np.int16), np.zeros((H // 2, W // 2), np.int16), np.zeros((H // 2, W // 2), np.int16)]
    return workload.make_planes(9300, W, H, B, "noise")


@functools.lru_cache(maxsize=None)
def _pads(n, luma, mode, mask):
    return capi.lib().hmx_intra_reads_unavailable(n, luma, mode, mask)


def _wave_item_kinds(tables):
    """{size class: [wave-items without a padded block, wave-items with one]} of a packed call.  An item carries the dependency
    mask; the function gives the same bit for it as for the availability (tests/test_intra_reads_unavailable.py)."""
    _, _, _, descs, items, _ = tables
    out = {}
    for d in descs:
        s, n, off = int(d["n_s"]) >> 28, int(d["n_s"]) & 0x0fffffff, int(d["item_off"])
        some = any(_pads(1 << int(b["log2n"]), int((int(b["plane"]) & 3) == 0), int(b["mode"]), int(b["avail"])) for b in items[off:off + n])
        out.setdefault(s, [0, 0])[1 if some else 0] += 1
    return out


def _call(ctx, plans, orgs, want, prefill, decode):
    """one whole-picture call of the three pictures; returns (reconstruction, levels) per picture"""
    L, n = capi.lib(), len(orgs)
    d_org = [capi.DevPicture(ctx, W, H).upload(o) for o in orgs]
    d_rec = [capi.DevPicture(ctx, W, H).upload(prefill) for _ in range(n)]
    d_lev = [capi.DevPicture(ctx, W, H, dtype=np.int32) for _ in range(n)]
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


def _set_shape(ctx, hmx_opts, shape):
    kind, s4, s8 = shape
    if kind == "level":
        hmx_opts(ctx, HMX_INTRA_SCHEDULE="level")
    else:
        hmx_opts(ctx, HMX_INTRA_SCHEDULE=None, HMX_PACK_GROUP="3", HMX_PACK_SLOTS4=str(s4), HMX_PACK_SLOTS8=str(s8))


@pytest.mark.parametrize("tiling", TILINGS)
def test_ref_skips_parity(ctx, hmx_opts, tiling):
    L, B = capi.lib(), ctx.bit_depth
    pp = capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1)
    kinds = {}  # (shape, size class) -> [wave-items without a padded block, with one] over the calls of (a) and (b)
    for decision in DECISIONS:
        tus, orgs, want = _case(tiling, decision, B)
        plans = ctx.intra_plans(tus, pp)
        try:
            for shape in SHAPES:
                _set_shape(ctx, hmx_opts, shape)
                for fill in (0, 1):
                    got = _call(ctx, plans, orgs, want, _prefill(B, fill), decode=False)
                    sched = C.c_int()
                    L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
                    assert (sched.value == 3) == (shape[0] == "packed"), (shape, sched.value)
                    if shape[0] == "packed" and fill == 0:
                        k = _wave_item_kinds(ctx.pack_tables())
                        print(f"tiling {tiling} {B} bit, {decision}, slots {shape[1:]}: wave-items [none padded, some padded] by size class {k}")
                        if decision in "ab":
                            for s, (a, b) in k.items():
                                acc = kinds.setdefault((shape, s), [0, 0])
                                acc[0] += a
                                acc[1] += b
                    _check(got, want, (tiling, B, decision, shape, fill, "encode"))
                    got = _call(ctx, plans, orgs, want, _prefill(B, fill), decode=True)
                    _check(got, want, (tiling, B, decision, shape, fill, "decode"))
        finally:
            L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * N_PICS)(*[p.value for p in plans]), N_PICS)
    present = {3: {32, "mix"}, 2: {16, 32, "mix"}, 1: {8, 16, "mix"}, 0: {4, 8, "mix"}}  # luma size, or the chroma of the next one up
    for shape in SHAPES[:4]:
        for s in range(4):
            if tiling in present[s]:
                assert (shape, s) in kinds, (tiling, shape, s)
    for (shape, s), (a, b) in kinds.items():
        assert a > 0 and b > 0, f"tiling {tiling}, slots {shape[1:]}, size class {s}: {a} wave-items without a padded block, {b} with one"


def test_ref_skips_device_built_plans(ctx, hmx_opts):
    """device-built plans carry the same bit: the plans of (f) on the mix from hmx_intra_plan_create_device give the pictures and
    levels of the host-built plans' run"""
    L, B = capi.lib(), ctx.bit_depth
    pp = capi.PicParam(W, H, QP, 0, capi.I_SLICE, 1)
    tus, orgs, want = _case("mix", "f", B)
    _set_shape(ctx, hmx_opts, SHAPES[3])
    host = ctx.intra_plans(tus, pp)
    cat = np.ascontiguousarray(np.concatenate(tus), capi.TU_DTYPE)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tus])])
    d = ctx.to_device(cat)
    dev = ctx.intra_plans_device(d.ptr, offs, pp)
    d.free()
    try:
        for fill in (0, 1):
            a = _call(ctx, host, orgs, want, _prefill(B, fill), decode=False)
            b = _call(ctx, dev, orgs, want, _prefill(B, fill), decode=False)
            _check(b, a, ("mix", B, "f", "device against host", fill, "encode"))
            _check(b, want, ("mix", B, "f", "device", fill, "encode"))
            b = _call(ctx, dev, orgs, want, _prefill(B, fill), decode=True)
            _check(b, want, ("mix", B, "f", "device", fill, "decode"))
    finally:
        for p in list(host) + list(dev):
            L.hmx_intra_plan_destroy(ctx.h, p)
