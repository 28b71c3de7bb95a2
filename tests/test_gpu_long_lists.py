"""Unit and candidate lists of hundreds of thousands of entries through the batch entries that put two or three host tables into
the argument arena before one launch: hmx_batch_fullpel_search, hmx_batch_tz_search, hmx_batch_subpel_cost,
hmx_batch_inter_pred_error and their _wp forms (and hmx_batch_subpel_search's single table at its limit).

A list is periodic: K = 509 distinct units (a prime, coprime to every wave and tile size) drawn with a seed -- positions over the
picture, sizes from {4, 8, 16}, no two alike -- repeated to length n.  The project's Python oracles (tests/me_oracle.py,
tests/tz_oracle.py, tests/subpel_oracle.py, tests/pred_error_oracle.py and, weighted, tests/me_wp_oracle.py) compute the K results
once; ALL n device results must equal them tiled, bit for bit.  A table of the call that is overwritten by another table of the
same call -- at any of its n entries -- changes results, or positions the host never checked.

What the sizes aim at is shown on the CPU by tests/test_arena_placement.py over the same tests/long_list_cases.py: the (small call,
large call) pairs and the over-long lists are exactly what the placement rule before reserve-then-place got wrong.

Every case runs on a fresh Context, whose arena head is 0; the pictures (64 x 64 luma, 80-sample margins made by
hmx_pic_extend_border, a random original) belong to a context of their own, so making them moves no case's head.  Per-unit work is
minimal: 1 x 1 and 3 x 3 full-search boxes, TZ range 4, two sub-pel candidates, prediction-error groups of 5 with bits and best."""
import ctypes as C

import numpy as np
import pytest

import long_list_cases as ll
import me_oracle as mo
import me_wp_oracle as mwo
import pred_error_oracle as po
import subpel_oracle as so
import tz_oracle as tzo
from thevc_amd import capi

pytestmark = pytest.mark.gpu

W, H, M = 64, 64, 80
K = 509
SIZES = (4, 8, 16)
LAMBDA = 70000
USE_HAD = 1
OFFS = np.array([[1, -2], [-3, 2]], np.int8)  # ll.N_CAND sub-pel candidates, quarter samples
WP_ROW = (37, -5, 5)                            # weight, offset, log2_denom of the one non-trivial row
WP_ROW_L1 = (20, 3, 5)                          # the prediction error's list 1 (the lists of a slice share the denominator)
NOMEM = -3                                      # HMX_ERR_NOMEM
FILL = 0x5A
assert len(OFFS) == ll.N_CAND


class Scene:
    """The pictures of one bit depth on the device, and the K results of every entry from the oracles (made on first use)."""

    def __init__(self, B):
        self.B, self.ctx = B, capi.Context(bit_depth=B)
        rng = np.random.default_rng(9100 + B)
        yy, xx = np.mgrid[0:H, 0:W]
        base = (np.sin(xx / 5.0) + np.cos(yy / 7.0)) * (1 << (B - 3)) + (1 << (B - 1))
        plane = np.clip(base + rng.integers(-(1 << (B - 4)), 1 << (B - 4), base.shape), 0, (1 << B) - 1).astype(np.int16)
        self.org_h = rng.integers(0, 1 << B, (H, W)).astype(np.int16)
        z = np.zeros((H // 2, W // 2), np.int16)
        self.ref = capi.DevPicture(self.ctx, W, H, M, M).upload([plane, z, z])
        self.ctx._chk(capi.lib().hmx_pic_extend_border(self.ctx.h, C.byref(self.ref.as_pic()), W, H, M, M))
        self.org = capi.DevPicture(self.ctx, W, H).upload([self.org_h, z, z])
        self.ctx.sync()
        self.full = np.ascontiguousarray(np.pad(plane, M, mode="edge"))  # what hmx_pic_extend_border makes (tests/test_gpu_parity.py)
        self.refs_arr, self.org_pic = (capi.Pic * 1)(self.ref.as_pic()), self.org.as_pic()
        self.lists, self.wants = {}, {}

    def free(self):
        self.ref.free()
        self.org.free()
        self.ctx.close()

    # ---- the K units of an entry ----
    def units(self, entry):
        if entry not in self.lists:
            self.lists[entry] = getattr(self, "_draw_" + entry)(np.random.default_rng(9200 + self.B + 10 * ll.ENTRIES.index(entry)))
        return self.lists[entry]

    @staticmethod
    def _geometry(rng):
        w, h = (int(v) for v in rng.choice(SIZES, 2))
        return int(rng.integers(0, (W - w) // 4 + 1)) * 4, int(rng.integers(0, (H - h) // 4 + 1)) * 4, w, h

    @staticmethod
    def _distinct(draw, dtype):
        """K draws, no two alike (so neighbours differ, also across the seam of the period), as records of dtype; a draw is one
        record or a tuple of them."""
        seen = {}
        while len(seen) < K:
            seen.setdefault(draw())
        recs = list(seen)
        return np.array(recs if np.isscalar(recs[0][0]) else [r for g in recs for r in g], dtype)

    def _draw_fullpel(self, rng):
        def draw():
            x, y, w, h = self._geometry(rng)
            cx, cy, k = int(rng.integers(-8, 9)), int(rng.integers(-8, 9)), int(rng.integers(0, 2))  # a 1 x 1 or a 3 x 3 box
            return (x, y, w, h, 0, int(h > 8 and rng.integers(0, 2)), int(rng.integers(-32, 33)), int(rng.integers(-32, 33)), cx - k, cy - k, cx + k, cy + k)
        u = self._distinct(draw, capi.ME_UNIT_DTYPE)
        assert {int(v) for v in u["right"] - u["left"]} == {0, 2} and set(u["w"]) == set(SIZES) == set(u["h"])
        return (u,)

    def _draw_tz(self, rng):
        def draw():
            x, y, w, h = self._geometry(rng)
            px, py = int(rng.integers(-32, 33)), int(rng.integers(-32, 33))
            return (x, y, w, h, 0, int(h > 8 and rng.integers(0, 2)), px, py, *mo.set_search_range(px, py, 4, x, y, W, H))
        u = self._distinct(draw, capi.ME_UNIT_DTYPE)
        tz = np.zeros(K, capi.TZ_UNIT_DTYPE)
        for i, r in enumerate(u):  # the start point as xTZSearch makes it: the clipped predictor >> 2
            sx, sy = mo.clip_mv(int(r["pred_x"]), int(r["pred_y"]), int(r["x"]), int(r["y"]), W, H, 64)
            tz[i] = (sx >> 2, sy >> 2, 4, 0)
        return u, tz

    def _draw_subpel_cost(self, rng):
        def draw():
            return (*self._geometry(rng), 0, 255, 4 * int(rng.integers(-8, 9)), 4 * int(rng.integers(-8, 9)), 0, 0)
        return (self._distinct(draw, capi.PU_DTYPE),)

    def _draw_pred_error(self, rng):
        """K groups of ll.GROUP candidates: list 0, list 1 or both of the one reference, quarter-sample vectors, and their bits."""
        def draw():
            g, out = self._geometry(rng), []
            for _ in range(ll.GROUP):
                kind = int(rng.integers(0, 3))
                out.append((*g, 255 if kind == 1 else 0, 255 if kind == 0 else 0, *(int(v) for v in rng.integers(-40, 41, 4))))
            return tuple(out)
        cands = self._distinct(draw, capi.PU_DTYPE)
        assert len(cands) == K * ll.GROUP
        return cands, rng.integers(0, 64, K * ll.GROUP).astype(np.uint32)

    # ---- the K results of an entry, from the oracles ----
    def want(self, entry, wp):
        if (entry, wp) not in self.wants:
            self.wants[(entry, wp)] = getattr(self, "_want_" + entry)(wp)
        return self.wants[(entry, wp)]

    def _entry(self):
        return mwo.entry(*WP_ROW, self.B)

    def _want_fullpel(self, wp):
        out = np.zeros(K, capi.ME_RESULT_DTYPE)
        for i, u in enumerate(self.units("fullpel")[0]):
            (mx, my, sad, cost), _ = mwo.search(self.org_h, self.full, (M, M), u, LAMBDA, self.B, self._entry()) if wp else mo.search(self.org_h, self.full, (M, M), u, LAMBDA, self.B)
            out[i] = (mx, my, sad, cost)
        return {"result": out}

    def _want_tz(self, wp):
        out = np.zeros(K, capi.ME_RESULT_DTYPE)
        units, tz = self.units("tz")
        for i, (u, z) in enumerate(zip(units, tz)):
            res = mwo.tz_search(self.org_h, self.full, (M, M), u, z, LAMBDA, self.B, self._entry())[0] if wp else tzo.search(self.org_h, self.full, (M, M), u, z, LAMBDA, self.B)[0]
            out[i] = res
        return {"result": out}

    def _want_subpel_cost(self, wp):
        out = np.zeros((K, ll.N_CAND), np.uint32)
        for i, u in enumerate(self.units("subpel_cost")[0]):
            x, y, w, h = int(u["x"]), int(u["y"]), int(u["w"]), int(u["h"])
            ob, X, Y = self.org_h[y:y + h, x:x + w], M + x + (int(u["mv0x"]) >> 2), M + y + (int(u["mv0y"]) >> 2)
            for k, (dx, dy) in enumerate(OFFS):
                out[i, k] = mwo.dist(ob, self.full, X, Y, int(dx), int(dy), self.B, USE_HAD, self._entry()) if wp else so.dist(ob, self.full, X, Y, int(dx), int(dy), self.B, USE_HAD)
        return {"cost": out}

    def _want_pred_error(self, wp):
        cands, bits = self.units("pred_error")
        table = tuple([([r[0], 1, 1], [r[1], 0, 0], [r[2], 0, 0])] for r in (WP_ROW, WP_ROW_L1)) if wp else None
        dist, cost = po.errors(cands, bits, [self.full], (M, M), self.org_h, LAMBDA, self.B, USE_HAD, table)
        best = po.decide(dist, cost, np.arange(0, K * ll.GROUP + 1, ll.GROUP))
        return {"dist": dist, "cost": cost, "best": best.astype(capi.PRED_CHOICE_DTYPE)}


@pytest.fixture(scope="module")
def scene():
    """scene(B): the Scene of a bit depth, made once."""
    made = {}

    def get(B):
        if B not in made:
            made[B] = Scene(B)
        return made[B]
    yield get
    for s in made.values():
        s.free()


def test_the_weighted_oracle_results_differ(scene):
    """The weight row is not trivial: the _wp cases below are not the unweighted cases again."""
    s = scene(8)
    for e in ll.ENTRIES:
        a, b = s.want(e, False), s.want(e, True)
        assert any(not np.array_equal(a[k], b[k]) for k in a), e


# ---- one call: buffers, issue, compare ----
OUTPUTS = {"fullpel": lambda n: {"result": (n, capi.ME_RESULT_DTYPE)}, "tz": lambda n: {"result": (n, capi.ME_RESULT_DTYPE)},
           "subpel_cost": lambda n: {"cost": (n * ll.N_CAND, np.dtype(np.uint32))},
           "pred_error": lambda n: {"dist": (n, np.dtype(np.uint32)), "cost": (n, np.dtype(np.uint32)), "best": (ll.n_groups(n), capi.PRED_CHOICE_DTYPE)}}


class Call:
    """One call of `entry` over the period repeated to n, on `ctx`: issue() returns the entry's code and waits for nothing."""

    def __init__(self, ctx, s, entry, n, wp=False):
        self.ctx, self.s, self.entry, self.n, self.wp = ctx, s, entry, n, wp
        self.host = [np.resize(a, n) for a in s.units(entry)]  # the period, cyclically; kept alive here
        if entry == "pred_error":
            self.host.append(np.append(np.arange(0, n, ll.GROUP), n).astype(np.uint32))  # the last group may be short
        self.out = {k: ctx.alloc(cnt * dt.itemsize) for k, (cnt, dt) in OUTPUTS[entry](n).items()}
        for d in self.out.values():
            ctx._chk(capi.lib().hmx_memset(ctx.h, d.ptr, FILL, d.nbytes))

    def issue(self):
        L, c, s, h, n = capi.lib(), self.ctx, self.s, self.host, self.n
        pics = (s.refs_arr, 1, C.byref(s.org_pic))
        geom = (W, H, M, M)
        wp = capi.me_wp_table([WP_ROW[0]], [WP_ROW[1]], [WP_ROW[2]]) if self.wp else None
        tail = (wp.ctypes.data,) if self.wp else ()
        if self.entry == "fullpel":
            f = L.hmx_batch_fullpel_search_wp if self.wp else L.hmx_batch_fullpel_search
            return f(c.h, h[0].ctypes.data, n, *pics, *geom, LAMBDA, self.out["result"].ptr, None, *tail)
        if self.entry == "tz":
            f = L.hmx_batch_tz_search_wp if self.wp else L.hmx_batch_tz_search
            return f(c.h, h[0].ctypes.data, h[1].ctypes.data, n, *pics, *geom, LAMBDA, self.out["result"].ptr, None, None, 0, *tail)
        if self.entry == "subpel_cost":
            f = L.hmx_batch_subpel_cost_wp if self.wp else L.hmx_batch_subpel_cost
            return f(c.h, h[0].ctypes.data, n, *pics, OFFS.ctypes.data, ll.N_CAND, USE_HAD, self.out["cost"].ptr, *tail)
        args = (c.h, h[0].ctypes.data, h[1].ctypes.data, n, h[2].ctypes.data, len(h[2]) - 1, *pics, *geom, LAMBDA, USE_HAD, self.out["dist"].ptr,
                self.out["cost"].ptr, self.out["best"].ptr)
        if not self.wp:
            return L.hmx_batch_inter_pred_error(*args)
        arr, keep = capi.mc_wp_array([tuple(capi.me_wp_table([r[0]], [r[1]], [r[2]]) for r in (WP_ROW, WP_ROW_L1))])
        return L.hmx_batch_inter_pred_error_wp(*args, arr)  # the call copies the tables before it returns

    def accepted(self):
        rc = self.issue()
        assert rc == 0, (self.entry, self.n, rc, capi.lib().hmx_last_error(self.ctx.h).decode())  # a refusal here is a failure, not a skip
        return self

    def check(self):
        """Every one of the n results against the K of the oracle (after a sync)."""
        want = self.s.want(self.entry, self.wp)
        for k, (cnt, dt) in OUTPUTS[self.entry](self.n).items():
            got = self.out[k].download(dt, cnt)
            if k == "best":  # per group; a short last group is decided by the oracle on its own
                w = np.resize(want["best"], cnt)
                if self.n % ll.GROUP:
                    lo = (cnt - 1) * ll.GROUP
                    idx = np.arange(lo, self.n) % (K * ll.GROUP)
                    w[-1] = po.decide(want["dist"][idx], want["cost"][idx], [0, len(idx)])[0]
            else:
                w = np.resize(want[k].reshape(-1), cnt)
            bad = np.flatnonzero(got != w)
            assert bad.size == 0, (self.entry, self.n, self.wp, k, int(bad.size), bad[:6].tolist(), got[bad[:3]].tolist(), w[bad[:3]].tolist())

    def untouched(self):
        for k, d in self.out.items():
            assert np.all(d.download(np.uint8) == FILL), (self.entry, self.n, k)

    def free(self):
        for d in self.out.values():
            d.free()


class Fresh:
    """A context of its own for one case (its arena head starts at 0), and the calls made on it."""

    def __init__(self, s):
        self.s, self.ctx, self.calls = s, capi.Context(bit_depth=s.B), []

    def call(self, entry, n, wp=False):
        self.calls.append(Call(self.ctx, self.s, entry, n, wp))
        return self.calls[-1]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                self.ctx.sync()
        finally:
            for c in self.calls:
                c.free()
            self.ctx.close()


def pairs():
    return [(e, m) for e in ll.ENTRIES for m in ll.SMALL[e]]


# ---- fits, head low ----
@pytest.mark.parametrize("entry,small", pairs(), ids=[f"{e}-{m}" for e, m in pairs()])
def test_large_call_behind_a_small_one(scene, entry, small):
    """The large call's tables fit the arena, but not behind the head the small call leaves: no wait in between."""
    with Fresh(scene(8)) as f:
        a, b = f.call(entry, small), f.call(entry, ll.LARGE[entry])
        a.accepted()
        b.accepted()
        f.ctx.sync()
        a.check()
        b.check()


@pytest.mark.parametrize("entry", ll.ENTRIES)
def test_large_call_first_on_a_context(scene, entry):
    with Fresh(scene(8)) as f:
        a = f.call(entry, ll.LARGE[entry]).accepted()
        f.ctx.sync()
        a.check()


@pytest.mark.parametrize("entry", ll.ENTRIES)
def test_large_call_twice_back_to_back(scene, entry):
    with Fresh(scene(8)) as f:
        a, b = f.call(entry, ll.LARGE[entry]), f.call(entry, ll.LARGE[entry])
        a.accepted()
        b.accepted()
        f.ctx.sync()
        a.check()
        b.check()


def test_ten_bit(scene):
    """The pair of the full search at bit depth 10."""
    with Fresh(scene(10)) as f:
        a, b = f.call("fullpel", ll.SMALL["fullpel"][2]), f.call("fullpel", ll.LARGE["fullpel"])
        a.accepted()
        b.accepted()
        f.ctx.sync()
        a.check()
        b.check()


# ---- weighted forms ----
@pytest.mark.parametrize("entry", ll.ENTRIES)
def test_weighted_large_call_behind_a_small_one(scene, entry):
    with Fresh(scene(8)) as f:
        a, b = f.call(entry, ll.SMALL[entry][3], wp=True), f.call(entry, ll.LARGE[entry], wp=True)
        a.accepted()
        b.accepted()
        f.ctx.sync()
        a.check()
        b.check()


# ---- does not fit ----
def refused(f, c):
    rc = c.issue()
    err = capi.lib().hmx_last_error(f.ctx.h).decode()
    assert rc == NOMEM and "split the call" in err, (c.entry, c.n, rc, err)
    f.ctx.sync()
    c.untouched()  # nothing was copied over, set or launched


def too_long():
    return [(e, n) for e in ll.ENTRIES for n in ll.TOO_LONG[e]]


@pytest.mark.parametrize("entry,n", too_long(), ids=[f"{e}-{n}" for e, n in too_long()])
def test_too_long_is_refused(scene, entry, n):
    """Every table fits the arena alone, together they do not: HMX_ERR_NOMEM, nothing touched, and the context goes on working."""
    assert ll.total(entry, n) > ll.CAP and all(ll.rounded(b) <= ll.CAP for b in ll.tables(entry, n))
    with Fresh(scene(8)) as f:
        refused(f, f.call(entry, n))
        a = f.call(entry, ll.AFTER_REFUSAL).accepted()
        f.ctx.sync()
        a.check()


def test_subpel_search_too_long_stays_refused(scene):
    """One table that alone exceeds the arena: hmx_batch_subpel_search refused it before reserve-then-place and still does."""
    s, n = scene(8), ll.TOO_LONG_SUBPEL_SEARCH
    with Fresh(s) as f:
        units = np.resize(s.units("fullpel")[0], n)
        d_int, d_res = f.ctx.alloc(n * capi.ME_RESULT_DTYPE.itemsize).zero(), f.ctx.alloc(n * capi.SUBPEL_RESULT_DTYPE.itemsize)
        try:
            f.ctx._chk(capi.lib().hmx_memset(f.ctx.h, d_res.ptr, FILL, d_res.nbytes))
            rc = capi.lib().hmx_batch_subpel_search(f.ctx.h, units.ctypes.data, n, d_int.ptr, s.refs_arr, 1, C.byref(s.org_pic), W, H, M, M, LAMBDA, USE_HAD,
                                                    d_res.ptr, None)
            err = capi.lib().hmx_last_error(f.ctx.h).decode()
            assert rc == NOMEM and "split the call" in err, (rc, err)
            f.ctx.sync()
            assert np.all(d_res.download(np.uint8) == FILL)
        finally:
            d_int.free()
            d_res.free()


# ---- the longest list ----
@pytest.mark.parametrize("entry", ["fullpel", "pred_error"])
def test_longest_list(scene, entry):
    """The largest n whose rounded tables fit 8 MiB together is accepted and right; one more is refused."""
    n = ll.largest(entry)
    assert ll.total(entry, n) <= ll.CAP < ll.total(entry, n + 1)
    with Fresh(scene(8)) as f:
        a = f.call(entry, n).accepted()
        f.ctx.sync()
        a.check()
        refused(f, f.call(entry, n + 1))
