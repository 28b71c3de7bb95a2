"""tests/wp_estimate_oracle.py held three ways, all on the CPU: against a literal second construction of WeightPredAnalysis.cpp
(plain loops over samples, the reference's statement order); against every weight table the reference encoder wrote into the
streams of tests/golden/wp_estimate.npz; and the library's host helpers (hmx_wp_update_params, hmx_wp_select,
hmx_wp_check_enable) against both."""
import math
import os

import numpy as np
import pytest

import wp_estimate_oracle as wo
from thevc_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wp_estimate.npz")
MAX_NUM_REF = 16


# ---- the second construction: WeightPredAnalysis.cpp, statement by statement -----------------------------------------------------
def _c_div(a, b):
    """Int64 division of C: towards zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def _c_ratio(a, b):
    """(Double)a / (Double)b of C, division by zero included"""
    a, b = float(a), float(b)
    if b != 0.0:
        return a / b
    return math.nan if a == 0.0 else math.copysign(math.inf, a)


def ref_calc_dc(pel, width, height):  # xCalcDCValue :451-464
    dc = 0
    for y in range(height):
        for x in range(width):
            dc += int(pel[y][x])
    return dc


def ref_calc_ac(pel, width, height, dc):  # xCalcACValue :474-487
    ac = 0
    for y in range(height):
        for x in range(width):
            ac += abs(int(pel[y][x]) - dc)
    return ac


def ref_acdc(planes, width, height):  # xCalcACDCParamSlice :71-108
    ac, dc = [], []
    for comp in range(3):
        w, h = (width, height) if comp == 0 else (width >> 1, height >> 1)
        sample = w * h
        org_dc = ref_calc_dc(planes[comp], w, h)
        norm_dc = _c_div(org_dc + (sample >> 1), sample)
        ac.append(ref_calc_ac(planes[comp], w, h, norm_dc))
        dc.append(norm_dc)
    return ac, dc


def ref_sad(org, ref, width, height, denom, weight, offset, B):  # xCalcSADvalueWP :501-517
    sad = 0
    size = width * height
    real_denom = denom + B - 8
    for y in range(height):
        for x in range(width):
            v = (int(org[y][x]) << denom) - (int(ref[y][x]) * weight + (offset << real_denom))
            sad += -v if v < 0 else v
    return _c_div(sad, size)


class RefAnalysis:
    """m_wp and the members that work on it; rows are dicts like wpScalingParam"""

    def __init__(self):  # :47-65
        self.wp = [[[dict(present=False, denom=0, weight=1, offset=0) for _ in range(3)] for _ in range(MAX_NUM_REF)] for _ in range(2)]

    def updating(self, cur, refs, is_p, log2_denom, B):  # xUpdatingWPParameters :252-304
        real_log2_denom = log2_denom + B - 8
        real_offset = 1 << (real_log2_denom - 1)
        for ref_list in range(1 if is_p else 2):
            for ref_idx in range(len(refs[ref_list])):
                for comp in range(3):
                    cur_dc, cur_ac = cur[1][comp], cur[0][comp]
                    ref_dc, ref_ac = refs[ref_list][ref_idx][1][comp], refs[ref_list][ref_idx][0][comp]
                    d_weight = 1.0 if ref_ac == 0 else min(max(-16.0, float(cur_ac) / float(ref_ac)), 15.0)
                    weight = int(0.5 + d_weight * float(1 << log2_denom))
                    offset = ((cur_dc << log2_denom) - weight * ref_dc + real_offset) >> real_log2_denom
                    if comp:
                        shift = 1 << (B - 1)
                        pred = shift - ((shift * weight) >> log2_denom)
                        delta_offset = min(max(-512, offset - pred), 511)
                        offset = min(max(-128, delta_offset + pred), 127)
                    default_weight = 1 << log2_denom
                    delta_weight = default_weight - weight
                    if delta_weight > 127 or delta_weight < -128:
                        return False
                    self.wp[ref_list][ref_idx][comp] = dict(present=True, weight=weight, offset=offset, denom=log2_denom)
        return True

    def select(self, org, recs, is_p, width, height, denom, B):  # xSelectWP :313-366
        default_weight = 1 << denom
        for ref_list in range(1 if is_p else 2):
            for ref_idx in range(len(recs[ref_list])):
                ref, t = recs[ref_list][ref_idx], self.wp[ref_list][ref_idx]
                sad_wp = ref_sad(org[0], ref[0], width, height, denom, t[0]["weight"], t[0]["offset"], B)
                sad_no = ref_sad(org[0], ref[0], width, height, denom, default_weight, 0, B)
                for comp in (1, 2):
                    sad_wp += ref_sad(org[comp], ref[comp], width >> 1, height >> 1, denom, t[comp]["weight"], t[comp]["offset"], B)
                    sad_no += ref_sad(org[comp], ref[comp], width >> 1, height >> 1, denom, default_weight, 0, B)
                ratio = _c_ratio(sad_wp, sad_no)
                if ratio >= 0.99:
                    for comp in range(3):
                        t[comp] = dict(present=False, offset=0, weight=default_weight, denom=denom)

    def estimate(self, org, cur, refs, recs, is_p, width, height, B):  # xEstimateWPParamSlice :176-245
        denom = 6
        if len(refs[0]) > 3:
            denom = 7
        while True:
            valid = self.updating(cur, refs, is_p, denom, B)
            if valid:
                break
            denom -= 1
        self.select(org, recs, is_p, width, height, denom, B)
        return denom

    def check_enable(self):  # xCheckWPEnable :135-170
        present_cnt = 0
        for lst in range(2):
            for ref_idx in range(MAX_NUM_REF):
                for comp in range(3):
                    present_cnt += int(self.wp[lst][ref_idx][comp]["present"])
        if present_cnt == 0:
            for lst in range(2):
                for ref_idx in range(MAX_NUM_REF):
                    for comp in range(3):
                        self.wp[lst][ref_idx][comp] = dict(present=False, denom=0, weight=1, offset=0)
            return False
        return True

    def table(self, lst, n):
        return np.array([[[c["weight"], c["offset"], c["denom"]] for c in self.wp[lst][i]] for i in range(n)], np.int16).reshape(n, 3, 3)


def ref_slice(org, cur, refs, recs, width, height, B):
    lists = list(refs) + [[]] * (2 - len(refs))
    rlists = list(recs) + [[]] * (2 - len(recs))
    a = RefAnalysis()
    d = a.estimate(org, cur, lists, rlists, len(refs) == 1, width, height, B)
    weighted = a.check_enable()
    return ([a.table(l, len(lists[l])) for l in range(2)], [[a.wp[l][i][0]["present"] for i in range(len(lists[l]))] for l in range(2)], d, weighted)


# ---- pictures -----------------------------------------------------------------------------------------------------------------------
def pictures(w, h, B, kind, rng):
    mx = (1 << B) - 1
    out = []
    for pw, ph in ((w, h), (w >> 1, h >> 1), (w >> 1, h >> 1)):
        if kind == "random":
            p = rng.integers(0, mx + 1, (ph, pw))
        elif kind == "zero":
            p = np.zeros((ph, pw), np.int64)
        elif kind == "max":
            p = np.full((ph, pw), mx)
        else:  # checkerboard of both range ends
            yy, xx = np.mgrid[0:ph, 0:pw]
            p = ((xx + yy) & 1) * mx
        out.append(p.astype(np.int16))
    return out


def faded(planes, B, gain, step, rng, noise=2):
    mx = (1 << B) - 1
    mid = (mx + 1) // 2
    return [np.clip(np.rint((p.astype(np.float64) - mid) * gain + mid + step * (1 << (B - 8))) + rng.integers(-noise, noise + 1, p.shape), 0, mx).astype(np.int16)
            for p in planes]


def same_slice(a, b):
    for l in range(2):
        if not np.array_equal(a[0][l], b[0][l]) or list(a[1][l]) != list(b[1][l]):
            return False
    return a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("B", [8, 10, 12])
def test_acdc_and_sad_against_the_loops(B):
    rng = np.random.default_rng(100 + B)
    for w, h, kind in ((6, 4, "random"), (24, 16, "random"), (8, 8, "zero"), (8, 8, "max"), (10, 6, "checker")):
        a, b = pictures(w, h, B, kind, rng), pictures(w, h, B, "random", rng)
        assert wo.acdc(a) == ref_acdc(a, w, h), (w, h, kind)
        for row in ([[64, 0, 6]] * 3, [[-128, 2000, 7], [255, -128, 7], [1, 127, 0]], [[255, -2000, 0], [-128, 127, 3], [37, -5, 5]]):
            got = wo.sad_sums(a, b, row, B)
            for c in range(3):
                pw, ph = (w, h) if c == 0 else (w >> 1, h >> 1)
                wgt, off, d = row[c]
                assert got[c][0] // (pw * ph) == ref_sad(a[c], b[c], pw, ph, d, wgt, off, B), (kind, row, c)
                assert got[c][1] // (pw * ph) == ref_sad(a[c], b[c], pw, ph, d, 1 << d, 0, B), (kind, row, c)


@pytest.mark.parametrize("B", [8, 10, 12])
def test_slices_against_the_loops(B):
    """P and B slices over faded, partly faded and range-end pictures: the tables, the present flags, the denominator and the
    weighted flag of the oracle equal those of the loops."""
    rng = np.random.default_rng(200 + B)
    w, h = 16, 8
    base = pictures(w, h, B, "random", rng)
    seen = set()
    for trial in range(12):
        n0, n1 = int(rng.integers(1, 6)), int(rng.integers(0, 3))
        org = faded(base, B, 1.0 - 0.05 * trial, 3 * trial, rng)
        lists_org, lists_rec = [], []
        for n in (n0, n1):
            # every other entry sits at the slice's own level: xSelectWP rejects it
            o = [faded(base, B, 1.0 - 0.05 * trial - (0.07 * (k + 1) if k % 2 else 0), 3 * trial + (4 * k if k % 2 else 0), rng) for k in range(n)]
            lists_org.append(o)
            lists_rec.append([faded(p, B, 1.0, 0, rng, noise=1) for p in o])
        if n1 == 0:
            lists_org, lists_rec = lists_org[:1], lists_rec[:1]
        if trial == 10:  # range ends as references
            lists_org[0][0] = lists_rec[0][0] = pictures(w, h, B, "max", rng)
        if trial == 11:
            lists_org[0][0] = lists_rec[0][0] = pictures(w, h, B, "checker", rng)
        cur, racdc = wo.acdc(org), [[wo.acdc(p) for p in l] for l in lists_org]
        got = wo.estimate_slice(org, cur, racdc, lists_rec, B)
        want = ref_slice(org, cur, racdc, lists_rec, w, h, B)
        got = (got[0] + [np.zeros((0, 3, 3), np.int16)] * (2 - len(got[0])), got[1] + [[]] * (2 - len(got[1])), got[2], got[3])
        assert same_slice(got, want), (trial, got, want)
        seen.add((got[2], got[3], any(not k for l in got[1] for k in l)))
    assert any(d == 7 for d, _, _ in seen) and any(d == 6 for d, _, _ in seen) and any(r for _, _, r in seen)


def _acdc_of(ac, dc):
    return ([ac] * 3, [dc] * 3)


def test_corners_against_the_loops():
    """refAC == 0; the ratio clipped at 15; the denominator falling to 3; both zero-denominator ratios of xSelectWP; the ratio at
    the 0.99 boundary from both sides."""
    B = 8
    # refAC == 0 -> weight 1.0; clipped at 15 -> 15 << d leaves the range at d = 6, 5, 4 and fits at 3 (8 - 120 = -112)
    for cur, ref, want_d, want_w in ((_acdc_of(500, 100), _acdc_of(0, 90), 6, 64), (_acdc_of(16000, 100), _acdc_of(10, 100), 3, 120),
                                     (_acdc_of(310, 100), _acdc_of(100, 100), 5, 99), (_acdc_of(300, 100), _acdc_of(100, 100), 6, 192)):
        tabs, d = wo.update_params(cur, [ref], [], B)
        a = RefAnalysis()
        dd = 6
        while not a.updating(cur, [[ref], []], True, dd, B):
            dd -= 1
        assert (d, tabs[0][0][0][0]) == (want_d, want_w) and dd == d
        assert np.array_equal(np.array(tabs[0], np.int16), a.table(0, 1))
    # xSelectWP on sums: 0 / 0 keeps, x / 0 resets, 98 / 100 keeps, 99 / 100 resets
    rows = [[70, 3, 6]] * 3
    for sums, keep in (([[0, 0]] * 3, True), ([[5, 0], [0, 0], [0, 0]], False), ([[98, 100], [0, 0], [0, 0]], True), ([[99, 100], [0, 0], [0, 0]], False),
                       ([[33, 34], [33, 33], [33, 33]], False), ([[32, 34], [33, 33], [33, 33]], True)):
        got, present = wo.select(sums, 1, 1, 6, rows)
        assert present == keep and got == (rows if keep else [[64, 0, 6]] * 3), sums
        assert keep == (not (_c_ratio(sum(s[0] for s in sums), sum(s[1] for s in sums)) >= 0.99))
    # the same through whole slices of the loops: identical pictures (0 / 0) and a zero original against a flat offset reference
    z, m = pictures(8, 8, B, "zero", None), pictures(8, 8, B, "max", None)
    for org, rec in ((z, z), (m, m), (z, m)):
        cur, racdc = wo.acdc(org), [[wo.acdc(rec)]]
        got = wo.estimate_slice(org, cur, racdc, [[rec]], B)
        want = ref_slice(org, cur, racdc, [[rec]], 8, 8, B)
        assert same_slice((got[0] + [np.zeros((0, 3, 3), np.int16)], got[1] + [[]], got[2], got[3]), want)


# ---- the recordings -------------------------------------------------------------------------------------------------------------------
def golden_slices():
    """Every inter slice of every run: (run, picture, B, w, h, org, per list the originals and reconstructions of its entries,
    recorded tables or None)."""
    z = np.load(GOLDEN)
    out = []
    for r, name in enumerate(z["runs"]):
        n = int(z[f"r{r}_n"])
        hdr = [z[f"r{r}_hdr{i}"] for i in range(n)]
        at = {int(hd[0]): i for i, hd in enumerate(hdr)}
        planes = lambda kind, i: [z[f"r{r}_{kind}{i}_{k}"].astype(np.int16) for k in range(3)]
        for i, hd in enumerate(hdr):
            if hd[4] == 2:
                continue
            pocs = [[int(q) for q in z[f"r{r}_wppoc{i}_{l}"]] for l in (0, 1)]
            pocs = [p for p in pocs if p]
            want = [z[f"r{r}_wptab{i}_{l}"] for l in range(len(pocs))] if hd[5] else None
            out.append(dict(run=str(name), pic=i, B=int(hd[3]), w=int(hd[1]), h=int(hd[2]), slice_type=int(hd[4]), org=planes("org", i),
                            ref_org=[[planes("org", at[q]) for q in l] for l in pocs], ref_rec=[[planes("rec", at[q]) for q in l] for l in pocs], want=want))
    return out


def expect_weighted(want):
    """A recorded slice whose every entry xSelectWP rejected carries the rows xCheckWPEnable leaves, (1, 0, 0): denominator 0 is
    reached no other way (the loop stops at 3)."""
    return want is not None and any((t[:, :, 2] != 0).any() for t in want)


def test_recorded_tables():
    """Every list of every P and B slice of every recorded stream; the 20 (list, reference) entries of the two stream fixtures' clips
    among them."""
    slices = golden_slices()
    lists = entries = 0
    per_run = {}
    for s in slices:
        cur, racdc = wo.acdc(s["org"]), [[wo.acdc(p) for p in l] for l in s["ref_org"]]
        tabs, present, d, weighted = wo.estimate_slice(s["org"], cur, racdc, s["ref_rec"], s["B"])
        assert weighted == expect_weighted(s["want"]), (s["run"], s["pic"])
        if s["want"] is None:
            continue
        for l, want in enumerate(s["want"]):
            assert np.array_equal(tabs[l], want), (s["run"], s["pic"], l, tabs[l].tolist(), want.tolist())
            lists += 1
            entries += len(want)
            per_run[s["run"]] = per_run.get(s["run"], 0) + len(want)
    assert len(slices) == 22 and lists == 30 and entries == 66
    assert per_run["lowdelay_P_wp_q30"] == 6 and per_run["randomaccess_wp_q32"] == 14


def test_host_helpers_on_the_recordings():
    """hmx_wp_update_params, hmx_wp_select and hmx_wp_check_enable chained over the oracle's sums give the recorded tables."""
    for s in golden_slices():
        cur, racdc = wo.acdc(s["org"]), [[wo.acdc(p) for p in l] for l in s["ref_org"]]
        as_arr = lambda v: np.array([tuple(v)], capi.WP_ACDC_DTYPE)[0]
        refs = [np.array([tuple(a) for a in l], capi.WP_ACDC_DTYPE) for l in racdc] + [np.zeros(0, capi.WP_ACDC_DTYPE)] * (2 - len(racdc))
        r0, r1, p0, p1, d = capi.wp_update_params(as_arr(cur), refs[0], refs[1], s["B"])
        want_tabs, want_d = wo.update_params(cur, racdc[0], racdc[1] if len(racdc) > 1 else [], s["B"])
        assert d == want_d and p0.all() and p1.all()
        rows, present = [r0, r1], [p0, p1]
        for l in range(len(racdc)):
            got = np.stack([rows[l]["weight"], rows[l]["offset"], rows[l]["log2_denom"]], axis=-1)
            assert np.array_equal(got, np.array(want_tabs[l])), (s["run"], s["pic"], l)
            for e in range(len(racdc[l])):
                sums = wo.sad_sums(s["org"], s["ref_rec"][l][e], want_tabs[l][e], s["B"])
                rows[l][e], present[l][e] = capi.wp_select(sums, s["w"] * s["h"], (s["w"] >> 1) * (s["h"] >> 1), d, rows[l][e])
        r0, r1, weighted = capi.wp_check_enable(rows[0], present[0], rows[1], present[1])
        assert bool(weighted) == expect_weighted(s["want"])
        if s["want"] is not None:
            for l, (got, want) in enumerate(zip((r0, r1), s["want"])):
                assert np.array_equal(np.stack([got["weight"], got["offset"], got["log2_denom"]], axis=-1), want), (s["run"], s["pic"], l)


def test_host_helpers_at_the_corners():
    as_arr = lambda v: np.array([tuple(v)], capi.WP_ACDC_DTYPE)[0]
    for cur, ref in ((_acdc_of(500, 100), _acdc_of(0, 90)), (_acdc_of(16000, 100), _acdc_of(10, 100)), (_acdc_of(300, 100), _acdc_of(100, 100)),
                     (_acdc_of(0, 0), _acdc_of(0, 0)), (_acdc_of(123456789012, 4095), _acdc_of(7, 1))):
        for B in (8, 10, 12):
            for n0 in (1, 4):
                tabs, d = wo.update_params(cur, [ref] * n0, [ref], B)
                r0, r1, p0, p1, got_d = capi.wp_update_params(as_arr(cur), np.array([tuple(ref)] * n0, capi.WP_ACDC_DTYPE), np.array([tuple(ref)], capi.WP_ACDC_DTYPE), B)
                assert got_d == d and len(r0) == n0
                for rows, want in ((r0, tabs[0]), (r1, tabs[1])):
                    assert np.array_equal(np.stack([rows["weight"], rows["offset"], rows["log2_denom"]], axis=-1), np.array(want)), (cur, ref, B, n0)
    row = np.array([((70, 70, 70), (3, 3, 3), (6, 6, 6), 0)], capi.WP_DTYPE)[0]
    for sums, keep in (([[0, 0]] * 3, True), ([[5, 0], [0, 0], [0, 0]], False), ([[98, 100], [0, 0], [0, 0]], True), ([[99, 100], [0, 0], [0, 0]], False),
                       ([[33, 34], [33, 33], [33, 33]], False), ([[32, 34], [33, 33], [33, 33]], True), ([[991, 1000], [7, 4], [3, 4]], False)):
        got, present = capi.wp_select(sums, 1 if sums[0][1] != 1000 else 10, 4 if sums[0][1] == 1000 else 1, 6, row)
        want, wkeep = wo.select(sums, 1 if sums[0][1] != 1000 else 10, 4 if sums[0][1] == 1000 else 1, 6, [[70, 3, 6]] * 3)
        assert bool(present) == wkeep and (sums[0][1] == 1000 or wkeep == keep), sums
        assert [[int(got["weight"][c]), int(got["offset"][c]), int(got["log2_denom"][c])] for c in range(3)] == want
    rows = np.array([((64, 64, 64), (0, 0, 0), (6, 6, 6), 0)] * 2, capi.WP_DTYPE)
    r0, r1, weighted = capi.wp_check_enable(rows, [0, 0], rows[:1], [0])
    assert weighted == 0 and (r0["weight"] == 1).all() and (r0["log2_denom"] == 0).all() and (r1["weight"] == 1).all()
    r0, r1, weighted = capi.wp_check_enable(rows, [0, 0], rows[:1], [1])
    assert weighted == 1 and (r0["weight"] == 64).all() and (r1["log2_denom"] == 6).all()


def test_recordings_are_the_stream_fixtures():
    """The first two runs are the clips of stream_lowdelay_P_wp_q30 / stream_randomaccess_wp_q32: the same tables and reconstructions."""
    z = np.load(GOLDEN)
    for r, name in enumerate(z["runs"][:2]):
        s = np.load(os.path.join(os.path.dirname(GOLDEN), f"stream_{name}.npz"))
        assert int(s["n"]) == int(z[f"r{r}_n"])
        for i in range(int(s["n"])):
            assert np.array_equal(s[f"hdr{i}"][[0, 1, 2, 3, 6]], z[f"r{r}_hdr{i}"][:5])
            for k in range(3):
                assert np.array_equal(s[f"rec{i}_{k}"], z[f"r{r}_rec{i}_{k}"])
            for l in (0, 1):
                if f"wptab{i}_{l}" in s.files:
                    assert np.array_equal(s[f"wptab{i}_{l}"], z[f"r{r}_wptab{i}_{l}"]) and np.array_equal(s[f"wppoc{i}_{l}"], z[f"r{r}_wppoc{i}_{l}"])


def test_weight_256_and_a_chroma_clip_against_the_loops():
    """Twice the contrast of the reference under four entries: weight 256 at denominator 7 passes the range rule (128 - 256 = -128)
    and the chroma offset lands on its clip at -128."""
    rng = np.random.default_rng(7500)
    w, h, B = 24, 16, 8
    ref = [rng.integers(96, 161, (h >> (1 if k else 0), w >> (1 if k else 0))).astype(np.int16) for k in range(3)]
    org = [(128 + 2 * (p.astype(np.int32) - 128)).astype(np.int16) for p in ref]
    cur, racdc = wo.acdc(org), [[wo.acdc(ref)] * 4]
    got = wo.estimate_slice(org, cur, racdc, [[ref] * 4], B)
    assert got[2] == 7 and (got[0][0][:, :, 0] == 256).all() and (got[0][0][:, 1:, 1] == -128).any() and all(got[1][0])
    assert same_slice((got[0] + [np.zeros((0, 3, 3), np.int16)], got[1] + [[]], got[2], got[3]), ref_slice(org, cur, racdc, [[ref] * 4], w, h, B))
