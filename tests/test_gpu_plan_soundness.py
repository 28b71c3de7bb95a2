"""The intra schedules checked STRUCTURALLY (plan_check.py), not through the pictures they produce: a block one dependency
level too early, or a wave-item that waits for one wave-item too few, is a race that gives the right picture almost always.
 * plans, host-built and device-built separately: permutation of the input, level table, stored masks (from the ORACLE's
   availability), order (every block a mask names sits at a strictly lower level) and tightness (no level deeper than needed);
 * the packed schedule's tables of real calls (hmx_last_call_pack_tables) re-derived from the plans of the call: rows, ticket
   order, wave-items, dependency targets, the forward-progress induction, items, completion counters.
Run with -m gpu (plans and calls need a context; the checks themselves are host arithmetic)."""
import ctypes as C
import functools

import numpy as np
import pytest

import layout_oracle as LO
import oracle_lib as ol
import plan_check as PC
from test_avail_layout import random_layout
from thevc_amd import capi, workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(bit_depth=8)
    yield c
    c.close()


def _cached(f):
    memo = {}

    def g(t):
        k = tuple(int(t[n]) for n in ("x", "y", "log2n", "plane"))
        if k not in memo:
            memo[k] = f(t)
        return memo[k]

    return g


def _geometric_flags(w, h, ctu=64):
    """flags_of for check_plan: the oracle's hmo_intra_avail"""
    O = ol.oracle()

    def f(t):
        sh = 1 if t["plane"] else 0
        x, y, s = int(t["x"]) << sh, int(t["y"]) << sh, (1 << int(t["log2n"])) << sh
        flags = np.zeros(65, np.uint8)
        O.hmo_intra_avail(x, y, s, w, h, ctu, flags)
        return flags[:4 * (s // 4) + 1]

    return _cached(f)


def _layout_flags(w, h, region, intra):
    """flags_of for check_plan: the oracle's unit-by-unit layout rule"""
    reg = LO.Region(region, w)
    return _cached(lambda t: LO.block_flags(t, w, h, reg, intra))


def _device_plans(ctx, tus_list, pp, layouts=None):
    cat = np.ascontiguousarray(np.concatenate(tus_list), capi.TU_DTYPE)
    offs = np.concatenate([[0], np.cumsum([len(t) for t in tus_list])])
    d = ctx.to_device(cat)
    plans = ctx.intra_plans_device(d.ptr, offs, pp) if layouts is None else ctx.intra_plans_device_layout(d.ptr, offs, pp, layouts)
    d.free()
    return plans


def _sparse(tus, seed=5):
    """whole 16x16 luma areas (and their chroma) kept at random, one CTU without any block (test_device_plan_sparse_and_errors)"""
    rng = np.random.default_rng(seed)
    sh = (tus["plane"] != 0).astype(np.int32)
    key = ((tus["y"].astype(np.int32) << sh) // 16) * 64 + (tus["x"].astype(np.int32) << sh) // 16
    keep_area = rng.random(64 * 64) < 0.35
    keep_area[((np.arange(64 * 64) // 64) // 4 == 1) & ((np.arange(64 * 64) % 64) // 4 == 2)] = False
    sparse = tus[keep_area[key]]
    assert 0 < len(sparse) < len(tus)
    return sparse


PICTURE_NAMES = ["layout200x136", "layout416x240", "mix200x136", "mix416x240", "sparse", "uniform32", "uniform4"]


@functools.lru_cache(maxsize=None)
def _pictures():
    """name -> (w, h, tus, slice type, (region, intra) or None)"""
    out = {}
    for w, h in ((416, 240), (200, 136)):
        t = workload.make_tus(7000 + w, w, h, "mix", ts_prob=0.15)
        assert (t["flags"] & 1).any() and len(set(t["mode"][t["plane"] == 0].tolist())) == 35
        out[f"mix{w}x{h}"] = (w, h, t, capi.I_SLICE, None)
    out["uniform4"] = (128, 128, workload.make_tus(7101, 128, 128, 4), capi.I_SLICE, None)
    out["uniform32"] = (128, 128, workload.make_tus(7102, 128, 128, 32), capi.I_SLICE, None)
    out["sparse"] = (416, 240, _sparse(workload.make_tus(77, 416, 240, "mix")), capi.P_SLICE, None)
    rng = np.random.default_rng(7200)
    out["layout416x240"] = (416, 240, workload.make_tus(7201, 416, 240, "mix"), capi.I_SLICE, random_layout(rng, 416, 240, cip=True))
    out["layout200x136"] = (200, 136, workload.make_tus(7202, 200, 136, "mix"), capi.I_SLICE, random_layout(rng, 200, 136, cip=False))
    assert sorted(out) == PICTURE_NAMES
    return out


@pytest.mark.parametrize("name", PICTURE_NAMES)
def test_plan_is_sound_and_tight(ctx, name):
    """check_plan on the host-built and on the device-built plan of the same decisions, each on its own."""
    L = capi.lib()
    w, h, tus, slice_type, lay = _pictures()[name]
    pp = capi.PicParam(w, h, 30, 0, slice_type, 1)
    if lay is None:
        flags_of = _geometric_flags(w, h)
        host = ctx.intra_plan(tus, pp)
        (dev,) = _device_plans(ctx, [tus], pp)
    else:
        flags_of = _layout_flags(w, h, *lay)
        layout = capi.Layout(*lay)
        host = ctx.intra_plan(tus, pp, layout)  # hmx_intra_plan_create_layout
        (dev,) = _device_plans(ctx, [tus], pp, [layout])
        geo = _geometric_flags(w, h)
        assert any(PC.flags_to_mask(flags_of(t)) != PC.flags_to_mask(geo(t)) for t in tus), "the layout cuts nothing"
    try:
        for what, plan in (("host", host), ("device", dev)):
            blocks, levels = ctx.plan_tables(plan)
            nl = C.c_int()
            L.hmx_intra_plan_info(plan, None, C.byref(nl), None)
            assert nl.value == len(levels), what
            try:
                PC.check_plan(tus, blocks, levels, w, h, flags_of)
            except AssertionError as e:
                raise AssertionError(f"{name}, {what}-built plan: {e}") from None
    finally:
        L.hmx_intra_plan_destroy(ctx.h, host)
        L.hmx_intra_plan_destroy(ctx.h, dev)


@pytest.mark.parametrize("ctu", [16, 32])
def test_plan_is_sound_and_tight_small_ctu(ctu):
    """CTU sizes 16 and 32 (hmx_config): the availability changes with the CTU grid, the host analysis follows it.  (The
    device builder is for CTU size 64 and says so.)"""
    L = capi.lib()
    w, h = 200, 136
    c = capi.Context(bit_depth=8, ctu_size=ctu)
    try:
        pp = capi.PicParam(w, h, 30, 0, capi.I_SLICE, 1)
        for seed, tiling in ((7300, "mix"), (7301, 4)):
            tus = workload.make_tus(seed + ctu, w, h, tiling, ctu=ctu)
            flags_of = _geometric_flags(w, h, ctu)
            geo64 = _geometric_flags(w, h, 64)
            assert any(PC.flags_to_mask(flags_of(t)) != PC.flags_to_mask(geo64(t)) for t in tus)
            plan = c.intra_plan(tus, pp)
            blocks, levels = c.plan_tables(plan)
            PC.check_plan(tus, blocks, levels, w, h, flags_of)
            L.hmx_intra_plan_destroy(c.h, plan)
        d = c.to_device(tus)
        out = (C.c_void_p * 1)()
        assert L.hmx_intra_plan_create_device(c.h, d.ptr, (C.c_uint32 * 2)(0, len(tus)), 1, C.byref(pp), out) == -1 and not out[0]
        d.free()
    finally:
        c.close()


def test_checker_rejects_a_block_moved_up(ctx):
    """The checker can fail: in a downloaded table (numpy copies only) one block with dependencies is moved into the level
    of a block it reads from -- check_plan must name the order; the untouched table passes."""
    L = capi.lib()
    w, h, tus, slice_type, _ = _pictures()["mix200x136"]
    plan = ctx.intra_plan(tus, capi.PicParam(w, h, 30, 0, slice_type, 1))
    blocks, levels = ctx.plan_tables(plan)
    L.hmx_intra_plan_destroy(ctx.h, plan)
    flags_of = _geometric_flags(w, h)
    PC.check_plan(tus, blocks, levels, w, h, flags_of)
    lv_of = PC.table_levels(blocks, levels)
    where = {}
    for i, t in enumerate(blocks):
        pl, ux, uy, n = PC.block_units(t)
        for y in range(uy, uy + n):
            for x in range(ux, ux + n):
                where[(pl, x, y)] = i
    moved = None
    for i, t in enumerate(blocks):
        pl, ux, uy, n = PC.block_units(t)
        s = int(t["log2n"]) - 2
        if lv_of[i] == 0 or not int(t["avail"]) or levels[lv_of[i], 4:].sum() < 2:
            continue  # (the level it leaves must not become empty: the ORDER check is the one to fire)
        u = int(t["avail"]).bit_length() - 1
        j = where[(pl,) + PC.neighbour_unit(ux, uy, n, u)]
        moved = (i, j, s)
        break
    assert moved
    i, j, s = moved
    src, dst = int(lv_of[i]), int(lv_of[j])
    assert dst < src
    lv2 = levels.copy()
    lv2[src, 4 + s] -= 1
    lv2[dst, 4 + s] += 1
    lv2[:, :4] = (np.cumsum(lv2[:, 4:].reshape(-1)) - lv2[:, 4:].reshape(-1)).reshape(-1, 4)
    at = int(lv2[dst, s] + lv2[dst, 4 + s] - 1)  # the last slot of its new bucket
    order = [k for k in range(len(blocks)) if k != i]
    order.insert(at, i)
    b2 = blocks[order]
    assert PC.table_levels(b2, lv2)[at] == dst  # the edited table is a well-formed table
    with pytest.raises(AssertionError, match="order: block"):
        PC.check_plan(tus, b2, lv2, w, h, flags_of)


# ---- the packed schedule's tables ----
def _closed_sparse(tus, w, h, holes):
    """A sparse plan whose pictures the oracle can predict: the blocks inside `holes` (luma rectangles x0, y0, x1, y1) go, and
    so does every block whose mode reads -- directly or through other dropped blocks -- a unit of a dropped block.  What is
    left never looks at a sample this call does not write."""
    flags_of = _geometric_flags(w, h)
    bad = np.zeros((3, (h + 3) // 4, (w + 3) // 4), bool)
    keep = []
    for i, t in enumerate(tus):
        pl, ux, uy, n = PC.block_units(t)
        drop = any(x0 <= ux * 4 < x1 and y0 <= uy * 4 < y1 for x0, y0, x1, y1 in holes)
        if not drop:
            m = PC.dependency_mask(t, flags_of(t))
            drop = any((m >> u) & 1 and bad[(pl,) + PC.neighbour_unit(ux, uy, n, u)[::-1]] for u in range(4 * n + 1))
        if drop:
            bad[pl, uy:uy + n, ux:ux + n] = True
        else:
            keep.append(i)
    return tus[keep]


def _covered(tus, w, h):
    m = [np.zeros((h, w), bool), np.zeros((h // 2, w // 2), bool), np.zeros((h // 2, w // 2), bool)]
    for t in tus:
        N, x, y = 1 << int(t["log2n"]), int(t["x"]), int(t["y"])
        m[int(t["plane"])][y:y + N, x:x + N] = True
    return m


def _packed_call(ctx, tus, plans, w, h, qp, orgs, shared=False, decode=False, oracle=None):
    """One whole-picture call on the packed schedule; returns its tables (ctx.pack_tables) after checking them against the
    plans (check_pack_tables) and the pictures and levels against the oracle, on the samples the plans' blocks cover."""
    B, L, n = ctx.bit_depth, capi.lib(), len(orgs)
    want = [(oracle or ol.o_intra_frame_encode)(tus[0 if shared else i], w, h, B, qp, orgs[i]) for i in range(n)]  # (rec, levels)
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
        assert sched.value == 3
        tables = ctx.pack_tables()  # (waits for the call; the abort word is read before hmx_sync reports and clears it)
        ctx.sync()
        tabs = [ctx.plan_tables(plans[0 if shared else i]) for i in range(n)]
        PC.check_pack_tables(tabs, *tables)
        for i in range(n):
            cov = _covered(tus[0 if shared else i], w, h)
            rec, lev = d_rec[i].download(), d_lev[i].download()
            for p in range(3):
                assert np.array_equal(rec[p][cov[p]], want[i][0][p][cov[p]]), ("reconstruction", i, p)
                assert np.array_equal(lev[p][cov[p]], want[i][1][p][cov[p]]), ("levels", i, p)
        return tables
    finally:
        for d in d_org + d_rec + d_lev:
            d.free()


def test_pack_tables_own_plans_of_different_depth(ctx, hmx_opts):
    """(a) five pictures, every one its own plan -- two mix tilings, a uniform 32 tiling, a sparse plan (whole CTUs and parts
    of CTUs missing), a uniform 8 tiling -- in groups of four: a ragged last group, pictures that run out of levels inside
    their group.  Then the export's error path: after a call on the level schedule there are no packed tables to give."""
    L = capi.lib()
    hmx_opts(ctx, HMX_PACK_GROUP="4")
    w, h, qp = 200, 136, 30
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
    sparse = _closed_sparse(workload.make_tus(8003, w, h, "mix"), w, h, [(128, 0, 192, 64), (32, 80, 64, 112)])
    ctus = {(int(t["y"]) << (1 if t["plane"] else 0)) // 64 * 4 + (int(t["x"]) << (1 if t["plane"] else 0)) // 64 for t in sparse}
    assert 2 not in ctus and max(ctus) > 2 and len(sparse) > 200, "the sparse plan: a CTU without blocks before CTUs with blocks"
    tus = [workload.make_tus(8001, w, h, "mix"), workload.make_tus(8002, w, h, 32), sparse, workload.make_tus(8004, w, h, "mix"),
           workload.make_tus(8005, w, h, 8)]
    plans = ctx.intra_plans(tus, pp)
    orgs = [workload.make_planes(8100 + i, w, h, ctx.bit_depth, "texture" if i % 2 else "noise") for i in range(5)]
    try:
        g = _packed_call(ctx, tus, plans, w, h, qp, orgs)[0]
        assert (g.n_pics, g.I, g.n_groups, g.n_shards) == (5, 4, 2, 2)
        depth = [len(ctx.plan_tables(p)[1]) for p in plans]
        assert len(set(depth[:4])) >= 3 and g.max_levels == max(depth), depth
        # no packed call, no tables
        hmx_opts(ctx, HMX_INTRA_SCHEDULE="level")
        d = [capi.DevPicture(ctx, w, h).upload(orgs[0]), capi.DevPicture(ctx, w, h).zero(), capi.DevPicture(ctx, w, h, dtype=np.int32).zero()]
        ctx._chk(L.hmx_frame_intra_encode(ctx.h, plans[0], 1, C.byref(d[0].as_pic()), C.byref(d[1].as_pic()), C.byref(d[2].as_pic())))
        ctx.sync()
        geom = capi.PackGeom()
        assert L.hmx_last_call_pack_tables(ctx.h, C.byref(geom), None, None, None, None, None) == -1
        assert L.hmx_last_call_pack_tables(ctx.h, None, None, None, None, None, None) == -1
        for x in d:
            x.free()
    finally:
        L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * 5)(*[p.value for p in plans]), 5)


def test_pack_tables_more_groups_than_shards(ctx, hmx_opts):
    """(b) twenty pictures in groups of two: ten groups on eight shards, so shards 0 and 1 hold two groups and the others one."""
    L = capi.lib()
    hmx_opts(ctx, HMX_PACK_GROUP="2")
    w, h, qp, n = 136, 72, 28, 20
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
    tilings = ["mix", "mix", 4, "mix", 16, 8, "mix", 32]
    tus = [workload.make_tus(8200 + i, w, h, tilings[i % len(tilings)]) for i in range(n)]
    plans = ctx.intra_plans(tus, pp)
    orgs = [workload.make_planes(8300 + i, w, h, ctx.bit_depth, "texture" if i % 2 else "noise") for i in range(n)]
    try:
        g = _packed_call(ctx, tus, plans, w, h, qp, orgs)[0]
        assert (g.n_pics, g.I, g.n_groups, g.n_shards) == (n, 2, 10, 8)
    finally:
        L.hmx_intra_plan_destroy_many(ctx.h, (C.c_void_p * n)(*[p.value for p in plans]), n)


@pytest.mark.parametrize("slots4,slots8", [(16, 8), (16, 16), (64, 8), (64, 16)])
def test_pack_tables_slots(ctx, hmx_opts, slots4, slots8):
    """(c) 16 or 64 4x4 blocks and 8 or 16 8x8 blocks per wave-item (sixteen 8x8 blocks go with one lane per 4x4 block only:
    with HMX_PACK_SLOTS4=16 the 8x8 blocks stay at eight).  Device-built plans, three pictures in one group."""
    L = capi.lib()
    hmx_opts(ctx, HMX_PACK_SLOTS4=str(slots4), HMX_PACK_SLOTS8=str(slots8), HMX_PACK_GROUP="3")
    w, h, qp = 200, 136, 31
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
    tus = [workload.make_tus(8400 + i, w, h, t) for i, t in enumerate(["mix", 4, 8])]
    plans = _device_plans(ctx, tus, pp)
    orgs = [workload.make_planes(8500 + i, w, h, ctx.bit_depth, "texture") for i in range(3)]
    try:
        g, _, rows, descs, _, _ = _packed_call(ctx, tus, plans, w, h, qp, orgs)
        assert (g.slots4, g.slots8) == (slots4, 8 if slots4 == 16 else slots8)
        # the knob shows in the tables: some wave-item of each class is full, none is fuller
        for s, want in ((0, g.slots4), (1, g.slots8)):
            cnt = (descs["n_s"] & 0x0fffffff)[descs["n_s"] >> 28 == s]
            assert len(cnt) and cnt.max() == want, (s, want)
    finally:
        for p in plans:
            L.hmx_intra_plan_destroy(ctx.h, p)


def test_pack_tables_shared_plan(ctx, hmx_opts):
    """(d) nine pictures that share ONE plan (hmx_frame_intra_encode), groups of four."""
    L = capi.lib()
    hmx_opts(ctx, HMX_PACK_GROUP="4")
    w, h, qp, n = 136, 72, 29, 9
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
    tus = workload.make_tus(8600, w, h, "mix")
    plan = ctx.intra_plan(tus, pp)
    orgs = [workload.make_planes(8700 + i, w, h, ctx.bit_depth, "texture" if i % 2 else "noise") for i in range(n)]
    try:
        g = _packed_call(ctx, [tus], [plan], w, h, qp, orgs, shared=True)[0]
        assert (g.n_pics, g.I, g.n_groups, g.n_shards) == (n, 4, 3, 3)
    finally:
        L.hmx_intra_plan_destroy(ctx.h, plan)


def test_pack_tables_decoder_direction(ctx, hmx_opts):
    """(e) the decoder direction builds its tables the same way: three pictures from the oracle's levels, groups of two."""
    L = capi.lib()
    hmx_opts(ctx, HMX_PACK_GROUP="2")
    w, h, qp = 200, 136, 27
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
    tus = [workload.make_tus(8800 + i, w, h, t) for i, t in enumerate(["mix", 16, "mix"])]
    plans = ctx.intra_plans(tus, pp)
    orgs = [workload.make_planes(8900 + i, w, h, ctx.bit_depth, "texture") for i in range(3)]
    try:
        g = _packed_call(ctx, tus, plans, w, h, qp, orgs, decode=True)[0]
        assert (g.n_pics, g.I, g.n_groups, g.n_shards) == (3, 2, 2, 2)
    finally:
        for p in plans:
            L.hmx_intra_plan_destroy(ctx.h, p)


def test_pack_tables_rdoq_call(ctx, hmx_opts):
    """(f) RDOQ as the quantiser of the chain (the pictures of test_frame_intra_rdoq_in_chain): whatever the knobs ask for, such
    a call runs one lane per 4x4 block, eight 8x8 blocks per wave-item and groups of at most two pictures."""
    L = capi.lib()
    hmx_opts(ctx, HMX_PACK_SLOTS4="16", HMX_PACK_SLOTS8="16", HMX_PACK_GROUP="2")
    w, h, n, qp = 200, 136, 4, 27
    rng = np.random.default_rng(77)
    pp = capi.PicParam(w, h, qp, 0, capi.I_SLICE, 1)
    tus = []
    for i in range(n):
        t = workload.make_tus(2300 + i, w, h, "mix")
        depth = rng.integers(0, 3, len(t))
        t["flags"] = (t["flags"] & 1) | (np.where(t["plane"] == 0, np.minimum(depth, 1), 5 + depth).astype(np.uint8) << 4)
        tus.append(t)
    plans = [ctx.intra_plan(t, pp) for t in tus]
    orgs = [workload.make_planes(2400 + i, w, h, ctx.bit_depth, "texture" if i % 2 else "noise") for i in range(n)]
    ests = [[ol.make_est_bits(rng) for _ in range(8)] for _ in range(n)]
    lams = [(float(rng.uniform(20, 120)), float(rng.uniform(15, 90))) for _ in range(n)]
    by_org = {id(o): i for i, o in enumerate(orgs)}
    oracle = lambda t, w_, h_, B, qp_, org: ol.o_intra_frame_encode_rdoq(t, w_, h_, B, qp_, org, ests[by_org[id(org)]], lams[by_org[id(org)]])
    ctx.set_rdoq([(ests[i], lams[i][0], lams[i][1]) for i in range(n)])
    try:
        g = _packed_call(ctx, tus, plans, w, h, qp, orgs, oracle=oracle)[0]
        assert (g.slots4, g.slots8, g.I, g.n_groups) == (64, 8, 2, 2)
    finally:
        ctx.set_rdoq(None)
        for p in plans:
            L.hmx_intra_plan_destroy(ctx.h, p)
