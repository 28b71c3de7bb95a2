"""The motion search held against what the REFERENCE ENCODER itself did: tests/golden/me_enc_tap.npz holds calls of the
reference's TEncSearch::xMotionEstimation recorded inside its encoder (tests/golden/make_me_enc_tap.py, tests/me_tap.py) --
P and B pictures, TZ and full search, the bi-prediction refinement on 2 * org - other, 8 and 10 bit, SAD and Hadamard, with
and without the row sub-sampling of FEN, the AMP widths and heights 12 and 24 -- with every xTZSearchHelp evaluation and all
eighteen xPatternRefinement costs.  Everything is compared for equality.

On the CPU the Python restatements (tests/me_oracle.py, tests/tz_oracle.py, tests/subpel_oracle.py) and the host helpers of
libhmx must reproduce the recording, evaluation by evaluation; on the GPU hmx_batch_fullpel_search, hmx_batch_tz_search (with
its whole trace), hmx_batch_subpel_search (fed from the device results and from the recorded vectors) and xMotionEstimation of
the C++ host mirror must.  The fixture alone suffices: nothing under oracle/_ref is read."""
import os
import subprocess

import numpy as np
import pytest

import me_oracle as mo
import me_tap as mt
import subpel_oracle as so
import tz_oracle as tzo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
ONES = 0xFFFFFFFF

_fx = []


def fixture():
    if not _fx:
        _fx.append(mt.load())
    return _fx[0]


padded_org = mt.padded_org


_walks = {}


def tz_walk(i):
    """tz_oracle.search of recorded call i: (result, trace, passes, labels), computed once."""
    if i not in _walks:
        fx = fixture()
        c = fx.calls[i]
        margin, ref = fx.ref(c)
        _walks[i] = tzo.search(padded_org(c), ref, margin, c.unit(), c.tz_unit(), c["lam"], c["bits"])
    return _walks[i]


# ---- the fixture itself ----
def test_fixture_holds_every_class():
    """The classes the maker requires, counted again on the file that is loaded: a regenerated, thinner fixture fails here."""
    fx = fixture()
    assert fx.runs and len(fx.calls) >= 300 and len(fx.pics) >= len(fx.runs)
    count = {}
    for i, c in enumerate(fx.calls):
        assert c["magic"] == mt.CALL_MAGIC and c["n_frac"] == 18 and c["n_tz"] == len(c.trace) and (c["n_tz"] > 0) == c.tz
        assert c["ctu"] == 64 and c.org.shape == (c["h"], c["w"]) and (c["run"], c["ref_poc"]) in fx.pics
        (mx, my), ref = fx.ref(c)
        assert ref.shape == (c["pic_h"] + 2 * my, c["pic_w"] + 2 * mx) and mx >= 64 + 8 and my >= 64 + 8
        walk = None
        if c.tz:
            _, trace, passes, labels = tz_walk(i)
            walk = (passes, labels) if trace == c.trace else None
        for name in mt.classes(c, walk, fx.ref(c)):
            count[name] = count.get(name, 0) + 1
    missing = [name for name in mt.REQUIRED if not count.get(name)]
    assert not missing, (missing, count)
    # the bi-prediction originals leave the sample range on both sides somewhere
    bi = [c for c in fx.calls if c["bi"]]
    assert any(int(c.org.min()) < 0 for c in bi) and any(int(c.org.max()) >= (1 << c["bits"]) for c in bi)
    # the margins are the picture's border samples repeated (TComPicYuv::extendPicBorder): the recording is a real reference picture
    for (mx, my), ref in fx.pics.values():
        assert np.all(ref[:my, mx:-mx] == ref[my, mx:-mx]) and np.all(ref[my:-my, :mx] == ref[my:-my, mx:mx + 1])


# ---- xSetSearchRange ----
def test_search_box():
    from thevc_amd import capi
    fx = fixture()
    clipped = 0
    for i, c in enumerate(fx.calls):
        centre = (c["mv_in_x"], c["mv_in_y"]) if c["bi"] else c.pred  # :4166-4167
        args = (centre[0], centre[1], c["range"], c["cu_x"], c["cu_y"], c["pic_w"], c["pic_h"], c["ctu"])
        assert mo.set_search_range(*args) == c.box, (i, "oracle", args)
        assert capi.set_search_range(*args) == c.box, (i, "hmx_setSearchRange", args)
        clipped += (c["right"] - c["left"], c["bottom"] - c["top"]) != (2 * c["range"], 2 * c["range"])
        if c.tz:  # the walk's start point: the predictor clipped for the CU, >> 2 (:4312-4313)
            z = c.tz_unit()
            assert (z["start_x"], z["start_y"]) == c.trace[0][:2], i
            assert tuple(v >> 2 for v in capi.clip_mv(c["pred_x"], c["pred_y"], c["cu_x"], c["cu_y"], c["pic_w"], c["pic_h"], c["ctu"])) == c.trace[0][:2], i
            assert c["adapt_range"] == c["range"]
    assert clipped >= 10  # boxes the picture border cuts
    assert any((c["cu_x"], c["cu_y"]) != (c["x"], c["y"]) for c in fx.calls)  # second partitions: the CU origin is not the unit's


# ---- the vector term ----
def test_vector_term():
    """me_oracle.mv_cost and hmx_mvCost with the recorded multiplier give the vector term of recorded costs at all three cost
    scales: recorded cost minus the SAD of the samples (no interpolation is involved at an integer position)."""
    from thevc_amd import capi
    fx = fixture()
    n = [0, 0, 0]
    for i, c in enumerate(fx.calls):
        (mx, my), ref = fx.ref(c)
        lam, B = c["lam"], c["bits"]

        def block(x, y):
            return ref[my + c["y"] + y:my + c["y"] + y + c["h"], mx + c["x"] + x:mx + c["x"] + x + c["w"]]

        def both(x, y, scale):
            v = mo.mv_cost(lam, x, y, c["pred_x"], c["pred_y"], scale)
            assert v == capi.mv_cost(lam, x, y, c["pred_x"], c["pred_y"], scale)
            n[scale] += 1
            return v
        for (x, y, cost) in c.trace[:12]:  # cost scale 2, the sub-sampled SAD of the integer stage
            assert (cost - mo.sad(c.org, block(x, y), c.sub_shift, B)) & ONES == both(x, y, 2), (i, x, y)
        if not c["had_me"]:  # candidate 0 of a stage at an integer position, the full SAD
            ix, iy = c["int_x"], c["int_y"]
            d = mo.sad(c.org, block(ix, iy), 0, B)
            assert (c.frac[0] - d) & ONES == both(2 * ix, 2 * iy, 1), i
            if (c["half_x"], c["half_y"]) == (0, 0):
                assert (c.frac[9] - d) & ONES == both(4 * ix, 4 * iy, 0), i
    assert min(n) > 40, n


# ---- xPatternSearch ----
def test_full_search_oracle():
    fx = fixture()
    n = 0
    for i, c in enumerate(fx.calls):
        if c.tz:
            continue
        margin, ref = fx.ref(c)
        (ix, iy, sad, cost), _ = mo.search(padded_org(c), ref, margin, c.unit(), c["lam"], c["bits"])
        assert (ix, iy, sad) == (c["int_x"], c["int_y"], c["int_sad"]), (i, (ix, iy, sad))
        assert cost == (c["int_sad"] + mo.mv_cost(c["lam"], ix, iy, c["pred_x"], c["pred_y"], 2)) & ONES, i
        n += 1
    assert n >= 150


# ---- xTZSearch ----
def test_tz_oracle_entry_for_entry():
    fx = fixture()
    n = entries = 0
    for i, c in enumerate(fx.calls):
        if not c.tz:
            continue
        (ix, iy, sad, cost), trace, _, _ = tz_walk(i)
        assert len(trace) == len(c.trace), (i, len(trace), len(c.trace))
        for k, (got, want) in enumerate(zip(trace, c.trace)):
            assert got == want, (i, k, got, want)
        assert (ix, iy, sad) == (c["int_x"], c["int_y"], c["int_sad"]), (i, (ix, iy, sad))
        assert cost == min(v for (_, _, v) in c.trace), i
        n += 1
        entries += len(trace)
    assert n >= 100 and entries > 40 * n


# ---- xPatternSearchFracDIF and the tail ----
def frac_expected(c, fx):
    (mx, my), ref = fx.ref(c)
    return so.refine(c.org, ref, mx + c["x"] + c["int_x"], my + c["y"] + c["int_y"], c["bits"], c["had_me"], c["lam"], c.pred, c["int_x"], c["int_y"])


def test_fractional_stage_oracle():
    fx = fixture()
    for i, c in enumerate(fx.calls):
        (mvx, mvy, _, cost), costs, (half, q) = frac_expected(c, fx)
        assert costs == c.frac, (i, costs, c.frac)
        assert half == (c["half_x"], c["half_y"]) and q == (c["qter_x"], c["qter_y"]), (i, half, q)
        assert cost == c["frac_cost"] and (mvx, mvy) == (c["mv_out_x"], c["mv_out_y"]), i
        (mx, my), ref = fx.ref(c)
        X, Y = mx + c["x"] + c["int_x"], my + c["y"] + c["int_y"]
        if i % 8 == 0:  # stage_costs on its own, the quarter stage around the RECORDED half-sample winner
            assert so.stage_costs(c.org, ref, X, Y, c["bits"], c["had_me"], c["lam"], c.pred, c["int_x"], c["int_y"]) == c.frac[:9], i
            assert so.stage_costs(c.org, ref, X, Y, c["bits"], c["had_me"], c["lam"], c.pred, c["int_x"], c["int_y"],
                                  (c["half_x"], c["half_y"])) == c.frac[9:], i
        bits, total = so.me_tail(c["lam"], c.pred, c["mv_out_x"], c["mv_out_y"], c["frac_cost"], c["bits_in"], 0.5 if c["bi"] else 1.0)
        assert (bits, total) == (c["bits_out"], c["cost_out"]), (i, bits, total)
    odd = [c for c in fx.calls if c["bi"] and (c["frac_cost"] - mo.mv_cost(c["lam"], c["mv_out_x"], c["mv_out_y"], c["pred_x"], c["pred_y"], 0)) & 1]
    assert len(odd) >= 5  # the floor of fWeight = 0.5 rounds somewhere


# ================================ GPU ================================
# Recorded calls grouped by (run, POC, reference picture, cost multiplier): one call per entry point and layer.  The original
# picture of a layer is assembled by pasting the recorded blocks at their positions, so units whose blocks overlap (the
# partitions of one CU, the CU sizes above it, a bBi block over the plain one) go to different layers.
def layers_of(calls, idx):
    layers = []
    for i in idx:
        c = calls[i]
        for lay in layers:
            if all(c["x"] + c["w"] <= calls[j]["x"] or calls[j]["x"] + calls[j]["w"] <= c["x"] or c["y"] + c["h"] <= calls[j]["y"]
                   or calls[j]["y"] + calls[j]["h"] <= c["y"] for j in lay):
                lay.append(i)
                break
        else:
            layers.append([i])
    return layers


class Layer:
    """The calls of one layer on the device: `full` and `tz` index lists with their unit arrays, and the pasted original."""

    def __init__(self, capi, ctx, fx, idx):
        c0 = fx.calls[idx[0]]
        self.w, self.h = c0["pic_w"], c0["pic_h"]
        org = np.zeros((self.h, self.w), np.int16)
        for i in idx:
            c = fx.calls[i]
            assert not org[c["y"]:c["y"] + c["h"], c["x"]:c["x"] + c["w"]].any()
            org[c["y"]:c["y"] + c["h"], c["x"]:c["x"] + c["w"]] = c.org
        z = np.zeros((self.h // 2, self.w // 2), np.int16)
        self.org = capi.DevPicture(ctx, self.w, self.h).upload([org, z, z])
        self.full = [i for i in idx if not fx.calls[i].tz]
        self.tz = [i for i in idx if fx.calls[i].tz]
        self.units, self.z = {}, None
        for kind, sel in (("full", self.full), ("tz", self.tz)):
            u = np.zeros(len(sel), capi.ME_UNIT_DTYPE)
            for k, i in enumerate(sel):
                for name, v in fx.calls[i].unit(0).items():
                    u[k][name] = v
            self.units[kind] = u
        self.z = np.zeros(len(self.tz), capi.TZ_UNIT_DTYPE)
        for k, i in enumerate(self.tz):
            t = fx.calls[i].tz_unit()
            self.z[k] = (t["start_x"], t["start_y"], t["range"], 0)


class Group:
    def __init__(self, capi, ctx, fx, idx):
        c0 = fx.calls[idx[0]]
        self.ctx, self.lam, self.had, self.B = ctx, c0["lam"], c0["had_me"], c0["bits"]
        (self.mx, self.my), plane = fx.ref(c0)
        self.w, self.h = c0["pic_w"], c0["pic_h"]
        d = capi.DevPicture(ctx, self.w, self.h, self.mx, self.my)
        flat = np.zeros(d.elems[0], np.int16)
        flat[:] = np.ascontiguousarray(plane, np.int16).reshape(-1)
        d.bufs[0].upload(flat)
        self.ref = d
        self.layers = [Layer(capi, ctx, fx, lay) for lay in layers_of(fx.calls, idx)]

    def geometry(self):
        return self.w, self.h, self.mx, self.my, self.lam

    def free(self):
        for d in [self.ref] + [lay.org for lay in self.layers]:
            d.free()


@pytest.fixture(scope="module")
def staged():
    from thevc_amd import capi
    fx = fixture()
    ctxs = {B: capi.Context(bit_depth=B) for B in (8, 10)}
    keys = {}
    for i, c in enumerate(fx.calls):
        keys.setdefault((c["run"], c["poc"], c["ref_poc"], c["lam"], c["had_me"]), []).append(i)
    groups = [Group(capi, ctxs[fx.calls[idx[0]]["bits"]], fx, idx) for _, idx in sorted(keys.items())]
    assert len(groups) >= 10 and sum(len(lay.full) + len(lay.tz) for g in groups for lay in g.layers) == len(fx.calls)
    yield groups
    for g in groups:
        g.free()
    for c in ctxs.values():
        c.close()


def row(r):
    return tuple(int(v) for v in r)


def want_int(c):
    return (c["int_x"], c["int_y"], c["int_sad"], (c["int_sad"] + mo.mv_cost(c["lam"], c["int_x"], c["int_y"], c["pred_x"], c["pred_y"], 2)) & ONES)


def want_frac(c):
    return (c["mv_out_x"], c["mv_out_y"], (c["frac_cost"] - mo.mv_cost(c["lam"], c["mv_out_x"], c["mv_out_y"], c["pred_x"], c["pred_y"], 0)) & ONES, c["frac_cost"])


@pytest.mark.gpu
def test_gpu_full_search(staged):
    fx, n = fixture(), 0
    for g in staged:
        for lay in g.layers:
            if lay.full:
                res = g.ctx.batch_fullpel_search(lay.units["full"], [g.ref], lay.org, *g.geometry())
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
                res, counts, trace = g.ctx.batch_tz_search(lay.units["tz"], lay.z, [g.ref], lay.org, *g.geometry(), want_trace=True, trace_cap=cap)
                for k, i in enumerate(lay.tz):
                    c = fx.calls[i]
                    assert int(counts[k]) == len(c.trace), (i, int(counts[k]), len(c.trace))
                    got = [row(r) for r in trace[k][:len(c.trace)]]
                    assert got == c.trace, (i, [(j, a, b) for j, (a, b) in enumerate(zip(got, c.trace)) if a != b][:3])
                    assert row(res[k]) == want_int(c), (i, row(res[k]), want_int(c))
                    n += 1
    assert n == sum(c.tz for c in fx.calls) >= 100


def check_frac(fx, sel, res, costs, label):
    for k, i in enumerate(sel):
        c = fx.calls[i]
        assert [int(v) for v in costs[k]] == c.frac, (label, i, [int(v) for v in costs[k]], c.frac)
        assert row(res[k]) == want_frac(c), (label, i, row(res[k]), want_frac(c))


@pytest.mark.gpu
def test_gpu_subpel_search_fed_from_the_device(staged):
    """Each integer search leaves its results on the device and hmx_batch_subpel_search reads them there; they are downloaded
    only afterwards, to show that the chain started from the recorded vectors."""
    from thevc_amd import capi
    fx, n = fixture(), 0
    for g in staged:
        for lay in g.layers:
            for kind, sel in (("full", lay.full), ("tz", lay.tz)):
                if not sel:
                    continue
                if kind == "full":
                    d_int = g.ctx.batch_fullpel_search_device(lay.units[kind], [g.ref], lay.org, *g.geometry())
                else:
                    d_int = g.ctx.batch_tz_search(lay.units[kind], lay.z, [g.ref], lay.org, *g.geometry(), keep_on_device=True)
                try:
                    res, costs = g.ctx.batch_subpel_search(lay.units[kind], d_int, [g.ref], lay.org, *g.geometry(), g.had, want_stage_costs=True)
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
                res, costs = g.ctx.batch_subpel_search(lay.units[kind], ints, [g.ref], lay.org, *g.geometry(), g.had, want_stage_costs=True)
                check_frac(fx, sel, res, costs, kind + " recorded")
                plain = g.ctx.batch_subpel_search(lay.units[kind], ints, [g.ref], lay.org, *g.geometry(), g.had)  # d_stage_costs = NULL
                assert plain.tobytes() == res.tobytes(), kind
                n += len(sel)
    assert n == len(fx.calls)


# ---- xMotionEstimation of the C++ host mirror ----
MIRROR_PER_KIND = 5


def mirror_calls(fx, run):
    """Per reference picture of a run and kind of call up to MIRROR_PER_KIND calls: first those whose integer stage answers
    differently when clipMv is given the unit's position for the CU origin (second partitions next to the picture border:
    me_tap.cu_origin_decides), then a spread of the rest."""
    out = {}
    for kind in ("tz", "full", "bi"):
        sel = [i for i, c in enumerate(fx.calls) if c["run"] == run and ("bi" if c["bi"] else "tz" if c.tz else "full") == kind]
        first = [i for i in sel if mt.cu_origin_decides(fx.calls[i], fx.ref(fx.calls[i]))][:3]
        rest = [i for i in sel if i not in first]
        pick = first + [rest[int(j)] for j in np.linspace(0, len(rest) - 1, min(MIRROR_PER_KIND - len(first), len(rest)))]
        for i in sorted(set(pick)):
            out.setdefault(fx.calls[i]["ref_poc"], []).append(i)
    return out


def test_mirror_selection_covers_every_kind():
    fx = fixture()
    kinds, cu, decides = {}, 0, 0
    for run in range(len(fx.runs)):
        for sel in mirror_calls(fx, run).values():
            for i in sel:
                c = fx.calls[i]
                k = "bi" if c["bi"] else "tz" if c.tz else "full"
                kinds[k] = kinds.get(k, 0) + 1
                cu += (c["cu_x"], c["cu_y"]) != (c["x"], c["y"])
                decides += mt.cu_origin_decides(c, fx.ref(c))
    assert all(kinds.get(k, 0) >= 8 for k in ("tz", "full", "bi")) and cu >= 8 and decides >= 4, (kinds, cu, decides)


@pytest.mark.gpu
@pytest.mark.parametrize("run", range(6))
def test_gpu_mirror_motion_estimation(run, tmp_path):
    import __graft_entry__ as g
    g.build()
    fx = fixture()
    assert len(fx.runs) == 6
    for ref_poc, sel in sorted(mirror_calls(fx, run).items()):
        c0 = fx.calls[sel[0]]
        (mx, my), plane = fx.ref(c0)
        assert all(fx.calls[i]["lam"] == c0["lam"] for i in sel)
        path = tmp_path / ("calls_%d.bin" % ref_poc)
        with open(path, "wb") as f:
            f.write(np.array([c0["bits"], c0["pic_w"], c0["pic_h"], mx, my, c0["ctu"], c0["fen"], c0["had_me"], c0["fast_search"], c0["lam"], len(sel)],
                             np.uint32).tobytes())
            f.write(np.ascontiguousarray(plane, "<i2").tobytes())
            for i in sel:
                c = fx.calls[i]
                f.write(np.array([c[k] for k in ("cu_x", "cu_y", "x", "y", "w", "h", "bi", "pred_x", "pred_y", "mv_in_x", "mv_in_y", "range", "bits_in")],
                                 np.int64).astype(np.uint32).tobytes())
                f.write(np.ascontiguousarray(c.org, "<i2").tobytes())
        out = subprocess.run([EXE, "calls", str(path)], capture_output=True, text=True, check=True).stdout.strip().split("\n")
        assert len(out) == len(sel)
        for line, i in zip(out, sel):
            c = fx.calls[i]
            assert [int(v) for v in line.split()] == [c["mv_out_x"], c["mv_out_y"], c["bits_out"], c["cost_out"]], (i, line)
