"""The order of the items inside a (row, size) bucket of the packed schedule: by code-path class, then by rank inside the picture's
run of that class, then by picture (thevc_amd/csrc/hmx_chain_dev.h, k_pack_fill).

Blocks of a bucket are independent, so the order cannot change a picture; it decides which blocks share a wave-item, and a wave runs
every arm one of its lanes takes.  The class is the part of the plans' sort key above the mode -- plane class, transform skip,
padding pass, mode class with the two angular classes as one -- so a class is one contiguous run of a picture's bucket.  Item
(picture k of the group, class c, rank r' in k's run of c) goes to

    item_base + sum_{c'' < c} sum_t n[t][c''] + sum_t min(n[t][c], r') + #{t < k : n[t][c] > r'}          n[t][c]: class-c items of picture t

Checked here: that formula against a stable sort (no device); the exported items of real calls against a Python mirror of the class
and the formula, entry for entry -- ragged groups, pictures with fewer levels, buckets of more than 64 items whose runs cross rank 64,
wave-items that straddle two classes; a shared plan keeps rank * I + k; at most (classes present - 1) wave-items of a bucket hold
more than one class; tables rebuilt and reused; and whole-picture parity against the oracle, 8 and 10 bit, both directions."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as ol
import plan_check as PC
from thevc_amd import capi, workload

N_CLASSES = 32
QP = 30
FIELDS = ("x", "y", "log2n", "mode", "flags", "avail")


# ---- the mirror ----
def class_code(plane, flags, pads, mode):
    mc = 0 if mode == 0 else 1 if mode == 1 else 2 if mode in (10, 26) else 3
    return (int(plane != 0) << 4) | ((int(flags) & 1) << 3) | (int(bool(pads)) << 2) | mc


def bucket_positions(n):
    """n[t][c] -> pos[t][c]: the places, relative to the bucket's first, of picture t's class-c items by rank; the formula above"""
    n = np.asarray(n, np.int64)
    I, nc = n.shape
    before = np.concatenate([[0], np.cumsum(n.sum(axis=0))])  # items of lower classes
    pos = [[None] * nc for _ in range(I)]
    for c in range(nc):
        col = n[:, c]
        for k in range(I):
            r = np.arange(col[k])
            pos[k][c] = before[c] + np.minimum(col[:, None], r[None, :]).sum(axis=0) + (col[:k, None] > r[None, :]).sum(axis=0)
    return pos


def test_formula_is_the_stable_sort_by_class_rank_picture():
    """no device: the closed form places every item where sorting (class, rank in the run, picture) puts it -- empty classes,
    pictures without items, runs longer than a round of 64"""
    rng = np.random.default_rng(31)
    for I in (1, 2, 3, 5, 64):
        for trial in range(6):
            n = rng.integers(0, [3, 9, 80, 200][trial % 4], (I, N_CLASSES))
            n[rng.random((I, N_CLASSES)) < 0.5] = 0
            if trial == 5:
                n[I // 2] = 0
            keys = sorted((c, r, k) for k in range(I) for c in range(N_CLASSES) for r in range(n[k, c]))
            want = {key: i for i, key in enumerate(keys)}
            pos = bucket_positions(n)
            for k in range(I):
                for c in range(N_CLASSES):
                    assert [want[(c, r, k)] for r in range(n[k, c])] == pos[k][c].tolist(), (I, trial, k, c)


def _plan_classes(ctx, plan):
    blocks, levels = ctx.plan_tables(plan)
    pads = ctx.plan_pad_bits(plan) & 1
    cls = np.array([class_code(b["plane"], b["flags"], p, b["mode"]) for b, p in zip(blocks, pads)], np.int64)
    return blocks, levels.astype(np.int64), cls


def mirror_items(ctx, plans, tables):
    """the item array of a call as the formula orders it, and per (row, size) the classes of its entries.  plans: one per picture."""
    geom, _, rows, _, items, _ = tables
    per_plan = {}
    for p in plans:
        if p.value not in per_plan:
            per_plan[p.value] = _plan_classes(ctx, p)
    want = np.zeros(len(items), items.dtype)
    cls_of = np.full(len(items), -1, np.int64)
    for L in range(geom.max_levels):
        for g in range(geom.n_groups):
            row = rows[L * geom.n_groups + g]
            members = range(g * geom.I, min((g + 1) * geom.I, geom.n_pics))
            for s in range(4):
                n = np.zeros((len(members), N_CLASSES), np.int64)
                runs = []
                for k, p in enumerate(members):
                    blocks, levels, cls = per_plan[plans[p].value]
                    st, ct = (int(levels[L, s]), int(levels[L, 4 + s])) if L < len(levels) else (0, 0)
                    c = cls[st:st + ct]
                    assert (np.diff(c) >= 0).all(), "a plan's bucket is sorted by class"
                    n[k] = np.bincount(c, minlength=N_CLASSES)
                    runs.append((blocks[st:st + ct], c))
                assert n.sum() == int(row["count"][s])
                pos = bucket_positions(n)
                for k, (blk, c) in enumerate(runs):
                    for cc in np.unique(c):
                        at = int(row["item_base"][s]) + pos[k][cc]
                        src = blk[c == cc]
                        for f in FIELDS:
                            want[f][at] = src[f]
                        want["plane"][at] = src["plane"] | (k << 2)
                        cls_of[at] = cc
    assert (cls_of >= 0).all()
    return want, cls_of


def assert_items_follow_the_formula(ctx, plans, tables):
    want, cls_of = mirror_items(ctx, plans, tables)
    items = tables[4]
    for f in FIELDS + ("plane",):
        bad = np.flatnonzero(items[f] != want[f])
        assert bad.size == 0, (f, bad[:8], items[bad[:4]], want[bad[:4]])
    return cls_of


# ---- calls ----
@pytest.fixture(scope="module", params=[8, 10])
def ctx(request):
    c = capi.Context(bit_depth=request.param)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _mix_case(w, h, B, seed, n):
    """(decisions, originals, the oracle's (reconstruction, levels)) of n pictures with plans and textures of their own"""
    tus = [workload.make_tus(seed + i, w, h, "mix") for i in range(n)]
    orgs = [workload.make_planes(seed + 50 + i, w, h, B, "texture" if i % 2 else "noise") for i in range(n)]
    want = [ol.o_intra_frame_encode(tus[i], w, h, B, QP, orgs[i]) for i in range(n)]
    return tus, orgs, want


def _call(ctx, w, h, plans, orgs, want, decode=False, shared=False):
    """one whole-picture call on the packed schedule: its pictures and levels against the oracle's, its tables checked"""
    L, n = capi.lib(), len(orgs)
    d_org = [capi.DevPicture(ctx, w, h).upload(o) for o in orgs]
    d_rec = [capi.DevPicture(ctx, w, h).zero() for _ in range(n)]
    d_lev = [capi.DevPicture(ctx, w, h, dtype=np.int32) for _ in range(n)]
    for i, d in enumerate(d_lev):
        d.upload(want[i][1]) if decode else d.zero()
    A = lambda lst, T: (T * n)(*[x.as_pic() for x in lst])
    parr = (C.c_void_p * len(plans))(*[p.value for p in plans])
    try:
        if decode:
            ctx._chk(L.hmx_frame_intra_decode_multi(ctx.h, parr, n, A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        elif shared:
            ctx._chk(L.hmx_frame_intra_encode(ctx.h, plans[0], n, A(d_org, capi.Pic), A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        else:
            ctx._chk(L.hmx_frame_intra_encode_multi(ctx.h, parr, n, A(d_org, capi.Pic), A(d_rec, capi.Pic), A(d_lev, capi.Levels)))
        sched = C.c_int()
        L.hmx_last_call_shape(ctx.h, C.byref(sched), None)
        assert sched.value == 3  # the packed schedule
        tables = ctx.pack_tables()
        ctx.sync()
        each = [plans[0 if shared else i] for i in range(n)]
        PC.check_pack_tables([ctx.plan_tables(p) for p in each], *tables)
        for i in range(n):
            rec, lev = d_rec[i].download(), d_lev[i].download()
            for p in range(3):
                assert np.array_equal(lev[p], want[i][1][p]), ("levels", i, p)
                assert np.array_equal(rec[p], want[i][0][p]), ("reconstruction", i, p)
        return tables, each
    finally:
        for d in d_org + d_rec + d_lev:
            d.free()


def _destroy(ctx, plans):
    capi.lib().hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * len(plans))(*[p.value for p in plans]), len(plans))


def _mixed_wave_items(tables, cls_of):
    """per (row, size) bucket with items: (wave-items that hold more than one class, classes present)"""
    geom, _, rows, descs, _, _ = tables
    slots = [PC.pack_slots(s, geom.slots4, geom.slots8) for s in range(4)]
    out = []
    for row in rows:
        for s in range(4):
            lo, total = int(row["item_base"][s]), int(row["count"][s])
            if total:
                mixed = sum(len(set(cls_of[a:min(a + slots[s], lo + total)].tolist())) > 1 for a in range(lo, lo + total, slots[s]))
                out.append((mixed, len(set(cls_of[lo:lo + total].tolist()))))
    assert sum(-(-int(r["count"][s]) // slots[s]) for r in rows for s in range(4)) == len(descs)  # (those ranges are the wave-items)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [(64, 16), (16, 8)], ids=lambda s: f"slots{s[0]}_{s[1]}")
@pytest.mark.parametrize("group", [3, 64])
def test_parity_order_and_homogeneity(ctx, hmx_opts, group, slots):
    """five pictures of 128x64 with plans of their own, encode and decode against the oracle; the items follow the formula; a bucket
    has at most (classes present - 1) wave-items with more than one class -- a bound of the construction: a wave-item is a range of
    the class-major order, and only a range that contains a class boundary holds two classes"""
    w, h, n = 128, 64, 5
    hmx_opts(ctx, HMX_INTRA_SCHEDULE=None, HMX_PACK_GROUP=str(group), HMX_PACK_SLOTS4=str(slots[0]), HMX_PACK_SLOTS8=str(slots[1]))
    tus, orgs, want = _mix_case(w, h, ctx.bit_depth, 4100, n)
    plans = ctx.intra_plans(list(tus), capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1))
    try:
        for decode in (False, True):
            tables, each = _call(ctx, w, h, plans, orgs, want, decode=decode)
            g = tables[0]
            assert (g.I, g.n_groups, g.slots4) == (min(group, n), -(-n // min(group, n)), slots[0])
            cls_of = assert_items_follow_the_formula(ctx, each, tables)
            stats = _mixed_wave_items(tables, cls_of)
            for mixed, present in stats:
                assert mixed <= present - 1, (mixed, present)
            if group == 64 and slots[0] == 16:
                assert any(m > 0 for m, _ in stats), "no wave-item straddles two classes: the case is too small"
    finally:
        _destroy(ctx, plans)


def _diagonals_of_4x4(w, h, seed, mode):
    """a uniform 4x4 tiling whose blocks all take `mode`, a third of the blocks of every diagonal on transform skip"""
    t = workload.make_tus(seed, w, h, 4)
    t["mode"] = mode
    t["flags"] = np.where((t["x"] // 4 + 2 * (t["y"] // 4)) % 3 == 0, capi.TU_TRANSFORM_SKIP, 0)
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("group", [2, 64])
def test_order_with_long_buckets_and_short_plans(ctx, hmx_opts, group):
    """400x400: a picture of 4x4 blocks, every block pure vertical.  Such a block reads the units above it and, luma, the one to its
    left (a row of the picture alone does not make a level: the first row pads from the left), so a level is a diagonal of the
    picture: up to 100 luma blocks, 67 of them without transform skip and without padding -- a 4x4 bucket of two rounds of 64 ranks
    in k_pack_fill whose first class run crosses rank 64.  Beside it a picture of 32x32 blocks with fewer levels, and a mix.  Groups
    of two leave a ragged last group."""
    w, h, B = 400, 400, ctx.bit_depth
    hmx_opts(ctx, HMX_INTRA_SCHEDULE=None, HMX_PACK_GROUP=str(group))
    tus = [_diagonals_of_4x4(w, h, 4200, 26), workload.make_tus(4201, w, h, 32), workload.make_tus(4202, w, h, "mix")]
    orgs = [workload.make_planes(4250 + i, w, h, B, "texture") for i in range(3)]
    want = [ol.o_intra_frame_encode(tus[i], w, h, B, QP, orgs[i]) for i in range(3)]
    plans = ctx.intra_plans(tus, capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1))
    try:
        _, levels, cls = _plan_classes(ctx, plans[0])
        crossing = False
        for L in range(len(levels)):
            st, ct = int(levels[L, 0]), int(levels[L, 4])
            c = cls[st:st + ct]
            crossing |= ct > 64 and c[63] == c[64]
        assert crossing, "the case: no 4x4 bucket of more than 64 blocks with a class run across rank 64"
        depth = [len(ctx.plan_tables(p)[1]) for p in plans]
        assert depth[1] < depth[0], depth
        tables, each = _call(ctx, w, h, plans, orgs, want)
        assert tables[0].I == min(group, 3) and tables[0].max_levels == max(depth)
        assert_items_follow_the_formula(ctx, each, tables)
    finally:
        _destroy(ctx, plans)


@pytest.mark.gpu
@pytest.mark.parametrize("group", [3, 64])
def test_shared_plan_keeps_rank_times_pictures_plus_picture(ctx, hmx_opts, group):
    """six pictures that follow ONE plan: item r of a picture's bucket, picture k of a group of I, sits at r * I + k"""
    w, h, n, B = 128, 64, 6, ctx.bit_depth
    hmx_opts(ctx, HMX_INTRA_SCHEDULE=None, HMX_PACK_GROUP=str(group))
    tus = workload.make_tus(4300, w, h, "mix")
    orgs = [workload.make_planes(4350 + i, w, h, B, "texture" if i % 2 else "noise") for i in range(n)]
    want = [ol.o_intra_frame_encode(tus, w, h, B, QP, o) for o in orgs]
    plan = ctx.intra_plan(tus, capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1))
    try:
        tables, each = _call(ctx, w, h, [plan], orgs, want, shared=True)
        geom, _, rows, _, items, _ = tables
        blocks, levels = ctx.plan_tables(plan)
        for L in range(geom.max_levels):
            for g in range(geom.n_groups):
                I = min(geom.I, n - g * geom.I)
                for s in range(4):
                    st, ct, lo = int(levels[L, s]), int(levels[L, 4 + s]), int(rows[L * geom.n_groups + g]["item_base"][s])
                    got = items[lo:lo + ct * I].reshape(ct, I)
                    for k in range(I):
                        for f in FIELDS:
                            assert np.array_equal(got[f][:, k], blocks[f][st:st + ct]), (L, g, s, k, f)
                        assert np.array_equal(got["plane"][:, k], blocks["plane"][st:st + ct] | (k << 2)), (L, g, s, k)
        assert_items_follow_the_formula(ctx, each, tables)  # (the formula says the same)
    finally:
        _destroy(ctx, [plan])


@pytest.mark.gpu
def test_tables_rebuilt_and_reused(ctx, hmx_opts):
    """plans A, A again (the tables of the call before are reused), plans B (rebuilt), A (rebuilt): tables and pictures right each time"""
    w, h, n, B = 128, 64, 5, ctx.bit_depth
    hmx_opts(ctx, HMX_INTRA_SCHEDULE=None, HMX_PACK_GROUP="3")
    pp = capi.PicParam(w, h, QP, 0, capi.I_SLICE, 1)
    cases = {"A": _mix_case(w, h, B, 4100, n), "B": _mix_case(w, h, B, 4400, n)}
    plans = {name: ctx.intra_plans(list(case[0]), pp) for name, case in cases.items()}
    try:
        for name in "AABA":
            tus, orgs, want = cases[name]
            tables, each = _call(ctx, w, h, plans[name], orgs, want)
            assert_items_follow_the_formula(ctx, each, tables)
    finally:
        for p in plans.values():
            _destroy(ctx, p)
