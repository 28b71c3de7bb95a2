"""The encoder's weight estimation on the GPU (hmx_wp_acdc_multi, hmx_wp_sad_multi, hmx_wp_estimate_slices, the C++ mirror), bit-exact
against tests/wp_estimate_oracle.py and against the tables the reference encoder wrote (tests/golden/wp_estimate.npz)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import wp_estimate_oracle as wo
from test_wp_estimate_oracle import expect_weighted, golden_slices, pictures
from thevc_amd import capi, decisions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(2, 2), (8, 8), (24, 16), (70, 34), (200, 136), (416, 240)]
# (luma margin x, y, extra samples per row, samples the planes start after their allocation): every picture its own strides, an odd
# element offset in all but one
LAYOUTS = [(16, 8, 0, 1), (6, 2, 3, 1), (0, 0, 1, 1), (10, 4, 8, 0), (2, 2, 5, 1)]


@pytest.fixture(scope="module")
def ctxs():
    c = {B: capi.Context(bit_depth=B) for B in (8, 10, 12)}
    yield c
    for v in c.values():
        v.close()


def device_picture(ctx, planes, w, h, layout, rng):
    """The planes inside margins full of other samples: a read outside a row changes a sum"""
    mx, my, pad, skew = layout
    d = capi.DevPicture(ctx, w, h, mx, my, pad=pad, skew=skew)
    for p in range(3):
        pw, ph, pmx, pmy = d.dims[p]
        flat = rng.integers(0, 1 << ctx.bit_depth, d.elems[p]).astype(np.int16)
        full = flat[skew:].reshape(ph + 2 * pmy, d.strides[p])
        full[pmy:pmy + ph, pmx:pmx + pw] = planes[p]
        d.bufs[p].upload(flat)
    return d


def acdc_array(values):
    return np.array([tuple(v) for v in values], capi.WP_ACDC_DTYPE)


def check_acdc(got, planes_list):
    want = acdc_array([wo.acdc(p) for p in planes_list])
    assert np.array_equal(got["ac"], want["ac"]) and np.array_equal(got["dc"], want["dc"]), (got, want)


def wp_row(rows):
    r = np.zeros((), capi.WP_DTYPE)
    r["weight"], r["offset"], r["log2_denom"] = [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows]
    return r


def random_row(rng):
    d = int(rng.integers(0, 8))
    return [[int(rng.integers(-128, 256)), int(rng.integers(-2000, 2001)) if c == 0 else int(rng.integers(-128, 128)), d if c == 0 else int(rng.integers(0, 8))]
            for c in range(3)]


def check_sad(ctx, jobs, orgs, recs, d_orgs, d_recs, w, h):
    got = ctx.wp_sad([(o, r, wp_row(row)) for o, r, row in jobs], d_orgs, d_recs, w, h)
    for j, (o, r, row) in enumerate(jobs):
        assert got[j].tolist() == wo.sad_sums(orgs[o], recs[r], row, ctx.bit_depth), (j, row)


@pytest.mark.parametrize("B", [8, 10, 12])
@pytest.mark.parametrize("w,h", SIZES)
def test_sums_vs_oracle(ctxs, B, w, h):
    ctx = ctxs[B]
    rng = np.random.default_rng(7000 + 13 * w + h + B)
    orgs = [pictures(w, h, B, "random", rng) for _ in range(5)]
    recs = [pictures(w, h, B, "random", rng) for _ in range(5)]
    d_orgs = [device_picture(ctx, p, w, h, LAYOUTS[i], rng) for i, p in enumerate(orgs)]
    d_recs = [device_picture(ctx, p, w, h, LAYOUTS[(i + 2) % 5], rng) for i, p in enumerate(recs)]  # rows of a pair differ in alignment
    check_acdc(ctx.wp_acdc(d_orgs[:1], w, h), orgs[:1])
    check_acdc(ctx.wp_acdc(d_orgs, w, h), orgs)
    one = capi.DevBuf(ctx, 48)  # the scalar companion
    ctx._chk(capi.lib().hmx_wp_acdc(ctx.h, C.byref(d_orgs[3].as_pic()), w, h, one.ptr))
    ctx.sync()
    check_acdc(one.download(capi.WP_ACDC_DTYPE, 1), orgs[3:4])
    check_sad(ctx, [(2, 4, random_row(rng))], orgs, recs, d_orgs, d_recs, w, h)
    check_sad(ctx, [(i, (i + 1) % 5, random_row(rng)) for i in range(5)], orgs, recs, d_orgs, d_recs, w, h)
    same = capi.DevPicture(ctx, w, h).upload(recs[0])  # both rows on 16-byte boundaries: the vector path of the pair
    plain = capi.DevPicture(ctx, w, h).upload(orgs[0])
    check_sad(ctx, [(0, 0, random_row(rng))], orgs, recs, [plain], [same], w, h)
    for d in d_orgs + d_recs + [same, plain]:
        d.free()
    one.free()


@pytest.mark.parametrize("B", [8, 10, 12])
def test_range_ends(ctxs, B):
    ctx = ctxs[B]
    rng = np.random.default_rng(7100 + B)
    for w, h in ((8, 8), (70, 34)):
        pics = [pictures(w, h, B, k, rng) for k in ("zero", "max", "checker")]
        dev = [device_picture(ctx, p, w, h, LAYOUTS[i], rng) for i, p in enumerate(pics)]
        check_acdc(ctx.wp_acdc(dev, w, h), pics)
        rows = [[[255, 2000, 7], [-128, 127, 7], [255, -128, 0]], [[-128, -2000, 0], [255, -128, 7], [-128, 127, 3]]]
        check_sad(ctx, [(o, r, rows[(o + r) % 2]) for o in range(3) for r in range(3)], pics, pics, dev, dev, w, h)
        for d in dev:
            d.free()


def test_sums_that_leave_32_bits(ctxs):
    ctx, B = ctxs[12], 12
    rng = np.random.default_rng(7200)
    w, h = 1056, 1024
    big = pictures(w, h, B, "max", rng)
    assert int(big[0].astype(np.int64).sum()) > 1 << 32
    d = device_picture(ctx, big, w, h, LAYOUTS[1], rng)
    check_acdc(ctx.wp_acdc([d], w, h), [big])
    d.free()
    w = h = 64
    z, m = pictures(w, h, B, "zero", rng), pictures(w, h, B, "max", rng)
    dz, dm = device_picture(ctx, z, w, h, LAYOUTS[0], rng), device_picture(ctx, m, w, h, LAYOUTS[4], rng)
    # weight 255 at denominator 7, original 0 against reference maximum and the other way round: 4095 * 255 * 4096 stops 0.4 % short
    # of 2^32, so the same pair also runs under a luma offset, which takes the sum to 4.5 * 2^32
    row, far = [[255, 0, 7]] * 3, [[-128, -2000, 7], [-128, -128, 7], [-128, -128, 7]]
    assert wo.sad_sums(z, m, row, B)[0][0] > 0.995 * (1 << 32) and wo.sad_sums(m, z, far, B)[0][0] > 4 << 32
    check_sad(ctx, [(0, 1, row), (1, 0, row), (1, 0, far), (0, 1, far)], [z, m], [z, m], [dz, dm], [dz, dm], w, h)
    dz.free(), dm.free()


@pytest.mark.parametrize("B", [8, 10, 12])
def test_rows_at_the_limits(ctxs, B):
    """Weights -128 and 255, luma offsets +-2000, denominators 0 and 7; jobs that share an original; one reconstruction under two rows"""
    ctx = ctxs[B]
    rng = np.random.default_rng(7300 + B)
    w, h = 24, 16
    orgs = [pictures(w, h, B, "random", rng) for _ in range(2)]
    recs = [pictures(w, h, B, "random", rng) for _ in range(3)]
    d_orgs = [device_picture(ctx, p, w, h, LAYOUTS[i], rng) for i, p in enumerate(orgs)]
    d_recs = [device_picture(ctx, p, w, h, LAYOUTS[i + 2], rng) for i, p in enumerate(recs)]
    rows = [[[-128, 2000, 0], [255, 127, 7], [-128, -128, 0]], [[255, -2000, 7], [-128, -128, 0], [255, 127, 7]], [[1, 0, 0]] * 3, [[128, 0, 7]] * 3,
            [[-128, -2000, 7], [37, 5, 3], [64, 0, 6]], [[255, 2000, 0], [64, 0, 6], [90, -7, 5]]]
    jobs = [(0, 0, rows[0]), (0, 1, rows[1]), (0, 1, rows[4]), (0, 2, rows[2]), (1, 2, rows[3]), (1, 2, rows[5]), (1, 0, rows[1])]
    check_sad(ctx, jobs, orgs, recs, d_orgs, d_recs, w, h)
    for d in d_orgs + d_recs:
        d.free()


def test_estimate_slices_on_the_recordings(ctxs):
    """Every slice of every recorded stream.  One call takes one picture size at the context's bit depth, so the five streams go
    in three calls; inside a call the slices of all its streams share one launch.  AC/DC values come from hmx_wp_acdc_multi and
    stay on the device for every other slice."""
    slices = golden_slices()
    done = 0
    for key in sorted({(s["B"], s["w"], s["h"]) for s in slices}):
        B, w, h = key
        ctx = ctxs[B]
        group = [s for s in slices if (s["B"], s["w"], s["h"]) == key]
        dev, planes = [], []

        def put(p):
            dev.append(capi.DevPicture(ctx, w, h, 16, 16).upload(p))
            planes.append(p)
            return len(dev) - 1

        items = []
        for s in group:
            items.append(dict(org=put(s["org"]), ref_org=[[put(p) for p in l] for l in s["ref_org"]], ref_rec=[[put(p) for p in l] for l in s["ref_rec"]]))
        d_acdc = ctx.alloc(48 * len(dev))
        stats = ctx.wp_acdc(dev, w, h, out=d_acdc)
        check_acdc(stats, planes)
        calls = []
        for k, (s, it) in enumerate(zip(group, items)):
            val = (lambda i: d_acdc.ptr + 48 * i) if k % 2 == 0 else (lambda i: stats[i])
            calls.append(dict(slice_type=s["slice_type"], org=dev[it["org"]], acdc=val(it["org"]),
                              refs=[[(dev[r], val(o)) for o, r in zip(lo, lr)] for lo, lr in zip(it["ref_org"], it["ref_rec"])]))
        outs = ctx.wp_estimate_slices(calls, w, h)
        for s, out in zip(group, outs):
            assert bool(out["weighted"]) == expect_weighted(s["want"]), (s["run"], s["pic"])
            for l, want in enumerate(s["want"] or []):
                rows = out["rows"][l]
                got = np.stack([rows["weight"], rows["offset"], rows["log2_denom"]], axis=-1)
                assert np.array_equal(got, want), (s["run"], s["pic"], l, got.tolist(), want.tolist())
                done += len(want)
        for d in dev:
            d.free()
        d_acdc.free()
    assert done == 66


def test_estimate_reports_a_weight_of_256(ctxs):
    """Four entries in list 0 (denominator 7) of a reference with half the slice's contrast: the reference's rule lets the weight
    256 through (128 - 256 = -128), the composite reports it as computed and costs it; hmx_wp_sad_multi itself refuses such a row."""
    ctx, B, w, h = ctxs[8], 8, 24, 16
    rng = np.random.default_rng(7500)
    ref = [rng.integers(96, 161, (h >> (1 if k else 0), w >> (1 if k else 0))).astype(np.int16) for k in range(3)]
    org = [(128 + 2 * (p.astype(np.int32) - 128)).astype(np.int16) for p in ref]
    cur, racdc = wo.acdc(org), [[wo.acdc(ref)] * 4]
    want = wo.estimate_slice(org, cur, racdc, [[ref] * 4], B)
    assert want[2] == 7 and (want[0][0][:, :, 0] == 256).any() and want[3]
    d_org, d_ref = device_picture(ctx, org, w, h, LAYOUTS[0], rng), device_picture(ctx, ref, w, h, LAYOUTS[1], rng)
    stats = ctx.wp_acdc([d_org, d_ref], w, h)
    out = ctx.wp_estimate_slices([dict(slice_type=capi.P_SLICE, org=d_org, acdc=stats[0], refs=[[(d_ref, stats[1])] * 4])], w, h)[0]
    rows = out["rows"][0]
    assert np.array_equal(np.stack([rows["weight"], rows["offset"], rows["log2_denom"]], axis=-1), want[0][0])
    assert out["present"][0].tolist() == [int(k) for k in want[1][0]] and out["log2_denom"] == 7 and out["weighted"] == 1
    with pytest.raises(capi.HmxError, match="job 0: weight"):
        ctx.wp_sad([(0, 0, rows[0])], [d_org], [d_ref], w, h)
    d_org.free(), d_ref.free()


def test_estimated_rows_drive_motion_compensation(ctxs):
    """The last P slice of stream_lowdelay_P_wp_q30: its units predicted under the rows hmx_wp_estimate_slices returns, as they come,
    equal the prediction under the rows of the stream."""
    ctx = ctxs[8]
    pics = list(decisions.load_pictures(os.path.join(ROOT, "tests", "golden", "stream_lowdelay_P_wp_q30.npz")))
    p = pics[3]
    s = [g for g in golden_slices() if g["run"] == "lowdelay_P_wp_q30" and g["pic"] == 3][0]
    w, h, m = p["w"], p["h"], decisions.MARGIN
    assert p["slice_type"] == capi.P_SLICE and [int(q) for q in p["wp"]["poc"][0]] == [2, 1, 0]
    d_org = capi.DevPicture(ctx, w, h).upload(s["org"])
    d_ref_org = [capi.DevPicture(ctx, w, h).upload(q) for q in s["ref_org"][0]]
    d_ref_rec = [capi.DevPicture(ctx, w, h, m, m).upload(q) for q in s["ref_rec"][0]]
    for d in d_ref_rec:
        ctx._chk(capi.lib().hmx_pic_extend_border(ctx.h, C.byref(d.as_pic()), w, h, m, m))
    stats = ctx.wp_acdc([d_org] + d_ref_org, w, h)
    out = ctx.wp_estimate_slices([dict(slice_type=capi.P_SLICE, org=d_org, acdc=stats[0], refs=[[(r, stats[1 + i]) for i, r in enumerate(d_ref_rec)]])], w, h)[0]
    rows = out["rows"][0]
    mine = dict(p, wp=dict(p["wp"], tab=[np.stack([rows["weight"], rows["offset"], rows["log2_denom"]], axis=-1), p["wp"]["tab"][1]]))
    results = []
    for q in (mine, p):
        pus, pocs, l0, _ = decisions.weighted_prediction_units(q)
        by_poc = {2: d_ref_rec[0], 1: d_ref_rec[1], 0: d_ref_rec[2]}
        d_pus = ctx.to_device(pus)
        ref_arr = (capi.Pic * len(pocs))(*[by_poc[poc].as_pic() for poc in pocs])
        d_pred = capi.DevPicture(ctx, w, h).zero()
        pred_arr = (capi.Pic * 1)(d_pred.as_pic())
        job = (capi.McJob * 1)()
        job[0].d_pus, job[0].n_pus, job[0].refs, job[0].n_refs = d_pus.ptr, len(pus), ref_arr, len(pocs)
        job[0].dst, job[0].pic_w, job[0].pic_h = C.pointer(pred_arr[0]), w, h
        ctx.batch_motion_compensation_wp(job, [(l0, None)])
        ctx.sync()
        results.append(d_pred.download())
        d_pred.free(), d_pus.free()
    assert any(a.any() for a in results[0])
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    for d in [d_org] + d_ref_org + d_ref_rec:
        d.free()


def test_cpp_mirror(tmp_path):
    """hmx_hm::WeightPredAnalysis (thevc_amd/host/hmx_hm.hpp) on one P and one B slice of the 192x128 recordings"""
    exe = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")
    slices = golden_slices()
    p_slice = [s for s in slices if s["run"] == "lowdelay_P_wp_q30" and s["pic"] == 3][0]
    b_slice = [s for s in slices if s["run"] == "randomaccess_wp_q32" and s["slice_type"] == capi.B_SLICE and len(s["ref_org"]) == 2 and len(s["ref_org"][0]) == 2][0]
    pics, body = [], []

    def put(org, rec):
        pics.append((org, rec))
        return len(pics) - 1

    for s in (p_slice, b_slice):
        cur = put(s["org"], s["org"])
        lists = [[put(o, r) for o, r in zip(lo, lr)] for lo, lr in zip(s["ref_org"], s["ref_rec"])] + [[]] * (2 - len(s["ref_org"]))
        body.append(np.array([cur, int(s["slice_type"] == capi.P_SLICE), len(lists[0]), len(lists[1])] + lists[0] + lists[1], np.int32))
    path = tmp_path / "wpest.bin"
    with open(path, "wb") as f:
        f.write(np.array([8, 192, 128, len(pics), 2], np.int32).tobytes())
        for org, rec in pics:
            for planes in (org, rec):
                for k in range(3):
                    f.write(np.ascontiguousarray(planes[k], np.int16).tobytes())
        for b in body:
            f.write(b.tobytes())
    lines = subprocess.run([exe, "wpest", str(path)], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert len(lines) == 6
    for k, s in enumerate((p_slice, b_slice)):
        assert lines[3 * k] == "1 1"
        present = wo.estimate_slice(s["org"], wo.acdc(s["org"]), [[wo.acdc(q) for q in l] for l in s["ref_org"]], s["ref_rec"], 8)[1]
        for l in range(2):
            v = np.array(lines[3 * k + 1 + l].split(), np.int64).reshape(-1, 3, 4)
            if l >= len(s["want"]):
                assert v.size == 0
                continue
            assert np.array_equal(v[:, :, 1:], s["want"][l]), (k, l)
            assert (v[:, :, 0] != 0).tolist() == [[k] * 3 for k in present[l]]


def test_refusals(ctxs):
    ctx, L = ctxs[8], capi.lib()
    rng = np.random.default_rng(7400)
    w, h = 8, 8
    d = device_picture(ctx, pictures(w, h, 8, "random", rng), w, h, LAYOUTS[0], rng)
    pic = (capi.Pic * 1)(d.as_pic())
    out = ctx.alloc(96)
    bad = (capi.Pic * 1)(d.as_pic())
    bad[0].plane[1] = None
    job = np.zeros(1, capi.WP_SAD_JOB_DTYPE)
    job["wp"]["weight"], job["wp"]["log2_denom"] = 64, 6
    jp = job.ctypes.data

    def refused(rc, word):
        assert rc == -1 and word in L.hmx_last_error(ctx.h).decode(), (rc, L.hmx_last_error(ctx.h))

    refused(L.hmx_wp_acdc_multi(ctx.h, 1, None, w, h, out.ptr), "null")
    refused(L.hmx_wp_acdc_multi(ctx.h, 1, pic, w, h, None), "null")
    refused(L.hmx_wp_acdc_multi(ctx.h, 1, bad, w, h, out.ptr), "null plane")
    refused(L.hmx_wp_acdc_multi(ctx.h, 0, pic, w, h, out.ptr), "n_pics")
    refused(L.hmx_wp_acdc(ctx.h, None, w, h, out.ptr), "null")
    for ww, hh in ((7, 8), (8, 7), (0, 8), (8, -2)):
        refused(L.hmx_wp_acdc_multi(ctx.h, 1, pic, ww, hh, out.ptr), "even")
        refused(L.hmx_wp_sad_multi(ctx.h, 1, jp, pic, 1, pic, 1, ww, hh, out.ptr), "even")
    for args in ((None, pic, 1, pic, 1), (jp, None, 1, pic, 1), (jp, pic, 1, None, 1)):
        refused(L.hmx_wp_sad_multi(ctx.h, 1, *args, w, h, out.ptr), "null")
    refused(L.hmx_wp_sad_multi(ctx.h, 1, jp, pic, 1, pic, 1, w, h, None), "null")
    refused(L.hmx_wp_sad_multi(ctx.h, 1, jp, pic, 1, bad, 1, w, h, out.ptr), "null plane")
    refused(L.hmx_wp_sad_multi(ctx.h, 0, jp, pic, 1, pic, 1, w, h, out.ptr), "n_jobs")
    refused(L.hmx_wp_sad_multi(ctx.h, 1, jp, pic, 0, pic, 1, w, h, out.ptr), "n_org")
    for field, value in (("org", 1), ("rec", 1)):
        j = job.copy()
        j[field] = value
        refused(L.hmx_wp_sad_multi(ctx.h, 1, j.ctypes.data, pic, 1, pic, 1, w, h, out.ptr), "job 0: picture index")
    two = np.concatenate([job, job])
    for field, comp, value in (("weight", 0, 256), ("weight", 2, -129), ("offset", 1, 128), ("offset", 2, -129), ("log2_denom", 0, 8), ("log2_denom", 1, 8)):
        j = two.copy()
        j["wp"][field][1, comp] = value
        refused(L.hmx_wp_sad_multi(ctx.h, 2, j.ctypes.data, pic, 1, pic, 1, w, h, out.ptr), "job 1: weight")
    j = two.copy()
    j["wp"]["reserved"][1] = 1
    refused(L.hmx_wp_sad_multi(ctx.h, 2, j.ctypes.data, pic, 1, pic, 1, w, h, out.ptr), "job 1")
    j = job.copy()
    j["wp"]["offset"][0, 0] = -32768  # any int16 as the luma offset
    ctx._chk(L.hmx_wp_sad_multi(ctx.h, 1, j.ctypes.data, pic, 1, pic, 1, w, h, out.ptr))
    ctx.sync()
    # the composite: what its parts refuse, and its own rules
    stats = ctx.wp_acdc([d], w, h)
    ok = dict(slice_type=capi.P_SLICE, org=d, acdc=stats[0], refs=[[(d, stats[0])]])
    assert ctx.wp_estimate_slices([ok], w, h)[0]["weighted"] == 1  # a picture against itself: both sums 0, 0 / 0 keeps the (default-valued) row
    for change, word in ((dict(slice_type=capi.I_SLICE), "slice_type"), (dict(refs=[[]]), "list size"), (dict(refs=[[(d, stats[0])], [(d, stats[0])]]), "P slice"),
                         (dict(refs=[[(d, stats[0])] * 17]), "list size")):
        with pytest.raises(capi.HmxError, match=word):
            ctx.wp_estimate_slices([dict(ok, **change)], w, h)
    with pytest.raises(capi.HmxError, match="even"):
        ctx.wp_estimate_slices([ok], 7, 8)
    refused(L.hmx_wp_estimate_slices(ctx.h, 1, None), "null")
    refused(L.hmx_wp_estimate_slices(ctx.h, 0, (capi.WpSlice * 1)()), "n_slices")
    assert L.hmx_wp_update_params(None, None, 0, None, 0, 8, None, None, None, None, None) == -1
    assert L.hmx_wp_select(None, 1, 1, 6, None, None) == -1 and L.hmx_wp_check_enable(None, None, 1, None, None, 0, None) == -1
    d.free(), out.free()
