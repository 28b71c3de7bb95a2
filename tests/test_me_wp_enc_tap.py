"""The WEIGHTED motion search held against what the REFERENCE ENCODER itself did: tests/golden/me_wp_enc_tap.npz holds calls of
the reference's TEncSearch::xMotionEstimation recorded inside its encoder in slices under explicit weighted prediction
(tests/golden/make_me_wp_enc_tap.py, tests/me_wp_tap.py) -- P slices, B slices on list 0 and on list 1, the bi-prediction
refinement, TZ and full search, SAD and Hadamard, FEN's ignored row sub-sampling, 8 and 10 bit -- with the luma weight entry
of the (POC, list, reference index) each call searched, recovered from the coded stream.  Everything is compared for equality.

On the CPU tests/me_wp_oracle.py must reproduce the recording, evaluation by evaluation; on the GPU
hmx_batch_fullpel_search_wp, hmx_batch_tz_search_wp (whole trace and count), hmx_batch_subpel_search_wp (all 18 stage costs, fed
from the device results and from the recorded vectors) and xMotionEstimation of the C++ host mirror must.  No call is skipped.
The fixture alone suffices: nothing under oracle/_ref is read."""
import os
import subprocess

import numpy as np
import pytest

import me_oracle as mo
import me_tap as mt
import me_wp_oracle as wo
import me_wp_tap as wt
import subpel_oracle as so
import test_me_enc_tap as tme

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
ONES = 0xFFFFFFFF

_fx = []


def fixture():
    if not _fx:
        _fx.append(wt.load())
    return _fx[0]


def entry(fx, i):
    """The oracle's entry of call i, or None when the slice was searched unweighted."""
    return wo.entry(*fx.wp[i], fx.calls[i]["bits"]) if fx.applied[i] else None


_judged = {}


def judged(i):
    """(weighted oracles reproduce the recorded costs, unweighted oracles do), computed once per call."""
    if i not in _judged:
        fx = fixture()
        c = fx.calls[i]
        rec = wt.recorded(c)
        _judged[i] = (wt.expected(c, fx.ref(c), fx.wp[i]) == rec, wt.expected(c, fx.ref(c), None) == rec)
    return _judged[i]


# ---- the fixture itself ----
def test_fixture_holds_every_class():
    """The class table the maker requires, counted again on the file that is loaded; `applied` is what the costs say."""
    fx = fixture()
    assert len(fx.runs) == 6 and len(fx.calls) >= 300 and len(fx.pics) >= len(fx.runs)
    count = {}
    for i, c in enumerate(fx.calls):
        assert c["magic"] == mt.CALL_MAGIC and c["n_frac"] == 18 and c["n_tz"] == len(c.trace) and (c["n_tz"] > 0) == c.tz
        assert c["ctu"] == 64 and c.org.shape == (c["h"], c["w"]) and (c["run"], c["ref_poc"]) in fx.pics
        w, o, d = fx.wp[i]
        assert -128 <= w <= 255 and -128 <= o <= 127 and 0 <= d <= 7
        as_w, as_u = judged(i)
        assert as_w or as_u, i
        assert fx.applied[i] == as_w, i
        assert wt.tail_holds(c), i
        for name in wt.classes(c, fx.wp[i], fx.applied[i], not as_u):
            count[name] = count.get(name, 0) + 1
    missing = [name for name in wt.REQUIRED if not count.get(name)]
    assert not missing, (missing, count)
    # one picture under two different entries, in one slice's two lists or in two slices
    seen = {}
    for i, c in enumerate(fx.calls):
        seen.setdefault((c["run"], c["ref_poc"]), set()).add(fx.wp[i])
    assert any(len(v) >= 2 for v in seen.values())
    bi = [c for c in fx.calls if c["bi"]]
    assert any(int(c.org.min()) < 0 for c in bi) or any(int(c.org.max()) >= (1 << c["bits"]) for c in bi)  # 2 * org - other leaves the range


def test_unweighted_recordings_are_told_apart():
    """Every call of this fixture was searched weighted, so the other answer of the maker's decision is shown on the calls of
    tests/golden/me_enc_tap.npz, recorded with weighted prediction off: they reproduce unweighted, do not reproduce under a
    non-default entry, and stand for no class; under the default entry only a call whose rows FEN sub-samples tells the two apart."""
    ufx = mt.load()
    sel = [int(j) for j in np.linspace(0, len(ufx.calls) - 1, 24)]
    told = 0
    for i in sel:
        c = ufx.calls[i]
        rec = wt.recorded(c)
        assert wt.expected(c, ufx.ref(c), None) == rec, i
        assert wt.expected(c, ufx.ref(c), (58, 17, 6)) != rec, i
        assert wt.classes(c, (58, 17, 6), False, True) == set() == wt.classes(c, (64, 0, 6), True, True)
        same = wt.expected(c, ufx.ref(c), (64, 0, 6)) == rec  # the identity entry: weighted = unweighted unless rows are skipped
        assert same == (c.sub_shift == 0), (i, c.sub_shift)
        told += not same
    assert told >= 3 and any(ufx.calls[i].sub_shift == 0 for i in sel)


# ---- xPatternSearch ----
def test_full_search_oracle():
    fx, n = fixture(), 0
    for i, c in enumerate(fx.calls):
        if c.tz:
            continue
        margin, ref = fx.ref(c)
        e = entry(fx, i)
        if e:
            (ix, iy, sad, cost), _ = wo.search(mt.padded_org(c), ref, margin, c.unit(), c["lam"], c["bits"], e)
        else:
            (ix, iy, sad, cost), _ = mo.search(mt.padded_org(c), ref, margin, c.unit(), c["lam"], c["bits"])
        assert (ix, iy, sad) == (c["int_x"], c["int_y"], c["int_sad"]), (i, (ix, iy, sad))
        assert cost == (c["int_sad"] + mo.mv_cost(c["lam"], ix, iy, c["pred_x"], c["pred_y"], 2)) & ONES, i
        n += 1
    assert n == sum(not c.tz for c in fx.calls) >= 150


# ---- xTZSearch ----
def test_tz_oracle_entry_for_entry():
    import tz_oracle as tzo
    fx = fixture()
    n = entries = 0
    for i, c in enumerate(fx.calls):
        if not c.tz:
            continue
        margin, ref = fx.ref(c)
        e = entry(fx, i)
        if e:
            (ix, iy, sad, cost), trace, _, _ = wo.tz_search(mt.padded_org(c), ref, margin, c.unit(), c.tz_unit(), c["lam"], c["bits"], e)
        else:
            (ix, iy, sad, cost), trace, _, _ = tzo.search(mt.padded_org(c), ref, margin, c.unit(), c.tz_unit(), c["lam"], c["bits"])
        assert len(trace) == len(c.trace), (i, len(trace), len(c.trace))
        for k, (got, want) in enumerate(zip(trace, c.trace)):
            assert got == want, (i, k, got, want)
        assert (ix, iy, sad) == (c["int_x"], c["int_y"], c["int_sad"]), (i, (ix, iy, sad))
        assert cost == min(v for (_, _, v) in c.trace), i
        n += 1
        entries += len(trace)
    assert n == sum(c.tz for c in fx.calls) >= 100 and entries > 20 * n


# ---- xPatternSearchFracDIF and the tail ----
def test_fractional_stage_oracle():
    fx = fixture()
    for i, c in enumerate(fx.calls):
        (mx, my), ref = fx.ref(c)
        args = (c.org, ref, mx + c["x"] + c["int_x"], my + c["y"] + c["int_y"], c["bits"], c["had_me"], c["lam"], c.pred, c["int_x"], c["int_y"])
        e = entry(fx, i)
        (mvx, mvy, _, cost), costs, (half, q) = wo.refine(*args, e) if e else so.refine(*args)
        assert costs == c.frac, (i, costs, c.frac)
        assert half == (c["half_x"], c["half_y"]) and q == (c["qter_x"], c["qter_y"]), (i, half, q)
        assert cost == c["frac_cost"] and (mvx, mvy) == (c["mv_out_x"], c["mv_out_y"]), i
        bits, total = so.me_tail(c["lam"], c.pred, c["mv_out_x"], c["mv_out_y"], c["frac_cost"], c["bits_in"], 0.5 if c["bi"] else 1.0)
        assert (bits, total) == (c["bits_out"], c["cost_out"]), (i, bits, total)


# ================================ GPU ================================
# Calls grouped by (run, POC, reference picture, cost multiplier, Hadamard flag, entry, weighted or not): one reference picture and
# one table row per group; test_me_enc_tap's Group and Layer stage them (a layer = units whose pasted originals do not overlap).
@pytest.fixture(scope="module")
def staged():
    from thevc_amd import capi
    fx = fixture()
    ctxs = {B: capi.Context(bit_depth=B) for B in (8, 10)}
    keys = {}
    for i, c in enumerate(fx.calls):
        keys.setdefault((c["run"], c["poc"], c["ref_poc"], c["lam"], c["had_me"], fx.wp[i], fx.applied[i]), []).append(i)
    groups = []
    for key, idx in sorted(keys.items()):
        g = tme.Group(capi, ctxs[fx.calls[idx[0]]["bits"]], fx, idx)
        g.wp = capi.me_wp_table(*[[v] for v in key[5]]) if key[6] else None
        groups.append(g)
    assert len(groups) >= 10 and sum(len(lay.full) + len(lay.tz) for g in groups for lay in g.layers) == len(fx.calls)
    assert sum(g.wp is not None for g in groups) >= 10
    yield groups
    for g in groups:
        g.free()
    for c in ctxs.values():
        c.close()


row, want_int, want_frac, check_frac = tme.row, tme.want_int, tme.want_frac, tme.check_frac


@pytest.mark.gpu
def test_gpu_full_search(staged):
    fx, n = fixture(), 0
    for g in staged:
        for lay in g.layers:
            if lay.full:
                res = g.ctx.batch_fullpel_search(lay.units["full"], [g.ref], lay.org, *g.geometry(), wp=g.wp)
                for k, i in enumerate(lay.full):
                    assert row(res[k]) == want_int(fx.calls[i]), (i, row(res[k]), want_int(fx.calls[i]))
                    n += 1
    assert n == sum(not c.tz for c in fx.calls) >= 150


@pytest.mark.gpu
def test_gpu_tz_search_entry_for_entry(staged):
    fx, n, cap = fixture(), 0, 256
    assert max(len(c.trace) for c in fx.calls) <= cap
    for g in staged:
        for lay in g.layers:
            if lay.tz:
                res, counts, trace = g.ctx.batch_tz_search(lay.units["tz"], lay.z, [g.ref], lay.org, *g.geometry(), want_trace=True, trace_cap=cap, wp=g.wp)
                for k, i in enumerate(lay.tz):
                    c = fx.calls[i]
                    assert int(counts[k]) == len(c.trace), (i, int(counts[k]), len(c.trace))
                    got = [row(r) for r in trace[k][:len(c.trace)]]
                    assert got == c.trace, (i, [(j, a, b) for j, (a, b) in enumerate(zip(got, c.trace)) if a != b][:3])
                    assert row(res[k]) == want_int(c), (i, row(res[k]), want_int(c))
                    n += 1
    assert n == sum(c.tz for c in fx.calls) >= 100


@pytest.mark.gpu
def test_gpu_subpel_search_fed_from_the_device(staged):
    """Each weighted integer search leaves its results on the device and hmx_batch_subpel_search_wp reads them there."""
    from thevc_amd import capi
    fx, n = fixture(), 0
    for g in staged:
        for lay in g.layers:
            for kind, sel in (("full", lay.full), ("tz", lay.tz)):
                if not sel:
                    continue
                if kind == "full":
                    d_int = g.ctx.batch_fullpel_search_device(lay.units[kind], [g.ref], lay.org, *g.geometry(), wp=g.wp)
                else:
                    d_int = g.ctx.batch_tz_search(lay.units[kind], lay.z, [g.ref], lay.org, *g.geometry(), keep_on_device=True, wp=g.wp)
                try:
                    res, costs = g.ctx.batch_subpel_search(lay.units[kind], d_int, [g.ref], lay.org, *g.geometry(), g.had, want_stage_costs=True, wp=g.wp)
                    ints = d_int.download(capi.ME_RESULT_DTYPE, len(sel))
                finally:
                    d_int.free()
                assert [row(r) for r in ints] == [want_int(fx.calls[i]) for i in sel], kind
                check_frac(fx, sel, res, costs, kind + " chained")
                n += len(sel)
    assert n == len(fx.calls)


@pytest.mark.gpu
def test_gpu_subpel_search_from_recorded_vectors(staged):
    """d_int uploaded from the recording: a wrong integer stage cannot mask a wrong refinement."""
    from thevc_amd import capi
    fx, n = fixture(), 0
    for g in staged:
        for lay in g.layers:
            for kind, sel in (("full", lay.full), ("tz", lay.tz)):
                if not sel:
                    continue
                ints = np.array([want_int(fx.calls[i]) for i in sel], capi.ME_RESULT_DTYPE)
                res, costs = g.ctx.batch_subpel_search(lay.units[kind], ints, [g.ref], lay.org, *g.geometry(), g.had, want_stage_costs=True, wp=g.wp)
                check_frac(fx, sel, res, costs, kind + " recorded")
                n += len(sel)
    assert n == len(fx.calls)


# ---- xMotionEstimation of the C++ host mirror, setWpScalingDistParam in front of it ----
@pytest.mark.gpu
def test_gpu_mirror_motion_estimation(tmp_path):
    """EVERY call of the fixture through the mirror, one unit at a time; no call is skipped."""
    import __graft_entry__ as g
    g.build()
    fx = fixture()
    picked = 0
    # one file per (run, reference picture, cost multiplier): in the B runs a picture is the reference of two pictures with their own
    # lambda; FEN, HadamardME and FastSearch are a run's switches
    files = {}
    for i, c in enumerate(fx.calls):
        files.setdefault((c["run"], c["ref_poc"], c["lam"]), []).append(i)
    for (run, ref_poc, lam), sel in sorted(files.items()):
        c0 = fx.calls[sel[0]]
        (mx, my), plane = fx.ref(c0)
        assert all(tuple(fx.calls[i][k] for k in ("lam", "fen", "had_me", "fast_search", "bits")) == tuple(c0[k] for k in ("lam", "fen", "had_me", "fast_search", "bits"))
                   for i in sel)
        path = tmp_path / ("calls_%d_%d_%d.bin" % (run, ref_poc, lam))
        with open(path, "wb") as f:
            f.write(np.array([c0["bits"], c0["pic_w"], c0["pic_h"], mx, my, c0["ctu"], c0["fen"], c0["had_me"], c0["fast_search"], c0["lam"], len(sel)],
                             np.uint32).tobytes())
            f.write(np.ascontiguousarray(plane, "<i2").tobytes())
            for i in sel:
                c = fx.calls[i]
                words = [c[k] for k in ("cu_x", "cu_y", "x", "y", "w", "h", "bi", "pred_x", "pred_y", "mv_in_x", "mv_in_y", "range", "bits_in")]
                f.write(np.array(words + list(fx.wp[i]) + [int(fx.applied[i])], np.int64).astype(np.uint32).tobytes())
                f.write(np.ascontiguousarray(c.org, "<i2").tobytes())
        out = subprocess.run([EXE, "calls_wp", str(path)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == len(sel)
        for line, i in zip(out, sel):
            c = fx.calls[i]
            e = wo.entry(*fx.wp[i], c["bits"])
            blk = plane[my + c["y"] + (c["mv_out_y"] >> 2):my + c["y"] + (c["mv_out_y"] >> 2) + c["h"],
                        mx + c["x"] + (c["mv_out_x"] >> 2):mx + c["x"] + (c["mv_out_x"] >> 2) + c["w"]]
            want = [c["mv_out_x"], c["mv_out_y"], c["bits_out"], c["cost_out"], wo.sad_w(c.org, blk, e, c["bits"]), wo.hads_w(c.org, blk, e, c["bits"])]
            assert [int(v) for v in line.split()] == want, (i, line, want)
            picked += 1
    assert picked == len(fx.calls) >= 300
