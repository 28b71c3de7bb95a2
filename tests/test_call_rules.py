"""The host rules of a whole-picture call (thevc_amd/csrc/hmx_call_rules.h) on the CPU: tests/native/call_rules_host.cpp runs the
library's own header, and every answer is held against tests/call_rules_model.py, the rules restated in Python from the source as
it stood before they moved into the header -- never against the header itself.

  RDOQ constants   the error scale and the Int64 factor of sign hiding, bit for bit against IEEE double arithmetic in the
                   reference's operation order, over every bit depth, QP remainder, size, QP period and the multipliers the
                   chain's RDOQ tests use; the 16-bit level bound against extreme_inputs.rdoq_max_level (the form with the
                   rounding term) and at the six boundary QPs of RDOQ_BOUNDARY_CASES
  shape rules      the picture counts on both sides of every threshold (159/160, 319/320, 511/512, 639/640, 1535/1536), each knob
                   set and unset, RDOQ and QP map on and off; the size limits at the last accepted and the first refused value,
                   which no call on a GPU can reach; the persistent-wave rule below, at and above what is resident
  schedule         every combination of the knobs that decide it
No GPU is needed."""
import itertools
import os
import struct
import subprocess

import pytest

import call_rules_model as M
import extreme_inputs as xi
from thevc_amd import workload

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
THRESHOLDS = (159, 160, 319, 320, 511, 512, 639, 640, 1535, 1536)
# QP_Y of tests/test_gpu_rdoq_chain_corners.py's CORNERS; its five pictures scale the two multipliers by 1 + 0.01 (i % 7) / 1 + 0.02 (i % 5)
CORNER_QPS = (51, 0, 22, 4, 37, 27)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("call_rules") / "call_rules_host")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "thevc_amd", "csrc"),
                           os.path.join(HERE, "native", "call_rules_host.cpp"), "-o", out])

    def run(queries):
        r = subprocess.run([out], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.returncode, r.stderr[-500:])
        lines = r.stdout.split("\n")[:-1]
        assert len(lines) == len(queries)
        return lines

    return run


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def lambdas():
    out = set()
    for qp in CORNER_QPS:
        lam = workload.rdoq_lambdas(qp)
        out |= {v for i in range(5) for v in (lam[0] * (1 + 0.01 * (i % 7)), lam[1] * (1 + 0.02 * (i % 5)))}
    for qp in range(52):
        out |= set(workload.rdoq_lambdas(qp))
    assert min(out) < 0.037 and max(out) > 4669  # the range the corner test names
    return sorted(out)


# ---- RDOQ's per-call constants ----
def test_err_scale_bit_for_bit(ask):
    grid = list(itertools.product(range(8, 13), range(6), range(2, 6)))
    got = ask([f"E {B} {M.QUANT_SCALES[rem]} {lg}" for B, rem, lg in grid])
    for (B, rem, lg), g in zip(grid, got):
        assert int(g, 16) == bits(M.err_scale(B, M.QUANT_SCALES[rem], lg)), (B, rem, lg)


def test_rd_factor(ask):
    grid = list(itertools.product(range(8, 13), range(6), range(13), lambdas()))
    assert len(grid) > 40000
    got = ask([f"F {M.INV_QUANT_SCALES[rem]} {per} {B} {bits(lam):016x}" for B, rem, per, lam in grid])
    for (B, rem, per, lam), g in zip(grid, got):
        assert int(g) == M.rd_factor(M.INV_QUANT_SCALES[rem], per, lam, B), (B, rem, per, lam)
    assert len(set(got)) > 1000 and min(int(g) for g in got) == 0 and max(int(g) for g in got) > 1 << 30  # the grid spans the factor's range


def test_levels_fit16_against_the_rounded_bound(ask):
    grid = list(itertools.product(range(8, 13), range(13), range(6), range(2, 6)))
    got = ask([f"L {M.QUANT_SCALES[rem]} {per} {B} {lg}" for B, per, rem, lg in grid])
    n_wide = 0
    for (B, per, rem, lg), g in zip(grid, got):
        wide = xi.rdoq_max_level(B, per, rem, lg) > xi.INT16_MAX
        assert (g == "0") == wide, (B, per, rem, lg)
        n_wide += wide
    assert 0 < n_wide < len(grid) // 4
    assert ask([f"L 26214 0 16 5", "L 14564 0 16 5"]) == ["0", "0"]  # a negative shift (qbits = -2) does not fit


@pytest.mark.parametrize("B,qp,N", xi.RDOQ_BOUNDARY_CASES)
def test_levels_fit16_at_the_boundary_qps(ask, B, qp, N):
    """(B, QP_Y, N): the lowest QP_Y at which every luma block up to N x N fits; one lower, where the bit depth has one, N x N does not."""
    top, bd = N.bit_length() - 1, 6 * (B - 8)
    per, rem = divmod(qp + bd, 6)
    assert ask([f"L {M.QUANT_SCALES[rem]} {per} {B} {lg}" for lg in range(2, top + 1)]) == ["1"] * (top - 1)
    if qp - 1 >= -bd:
        per, rem = divmod(qp - 1 + bd, 6)
        assert ask([f"L {M.QUANT_SCALES[rem]} {per} {B} {top}"]) == ["0"]
    else:
        assert (B, qp, N) in ((10, -12, 16), (12, -24, 4))  # the lowest QP there is


# ---- the packed shape ----
def shape_query(n, I, k4, k8, rdoq, qmap, levels, sz, items):
    return f"S {n} {I} {k4} {k8} {int(rdoq)} {int(qmap)} {levels} {sz[0]} {sz[1]} {sz[2]} {sz[3]} {items}"


def shape_answer(line):
    v = [int(x) for x in line.split()]
    return dict(n_groups=v[0], n_shards=v[1], slots4=v[2], slots8=v[3], n_rows=v[4], waves_bound=v[5], too_large=bool(v[6]))


def test_pack_group(ask):
    grid = list(itertools.product((0, 1, 2, 3, 64), (0, 1), (1, 2, 3, 63, 64, 65, 2048) + THRESHOLDS))
    got = ask([f"G {k} {r} {n}" for k, r, n in grid])
    for (k, r, n), g in zip(grid, got):
        assert int(g) == M.pack_group(k, bool(r), n), (k, r, n)
    assert [M.pack_group(0, False, n) for n in (511, 512, 1535, 1536)] == [1, 2, 2, 4]
    assert [M.pack_group(0, True, n) for n in (511, 512, 1536)] == [1, M.RDOQ_MAX_GROUP, M.RDOQ_MAX_GROUP]


def test_pack_shape_over_thresholds_and_knobs(ask):
    cases = []
    for n, k4, k8, rdoq, qmap, kg in itertools.product((1, 7, 2048) + THRESHOLDS, (0, 16, 64), (0, 8, 16), (False, True), (False, True), (0, 1, 3, 64)):
        I = M.pack_group(kg, rdoq, n)
        sz = (1021 * n, 257 * n, 61 * n, 13 * n)  # blocks per size class: no multiple of any wave-item shape
        cases.append((n, I, k4, k8, rdoq, qmap, 37, sz, sum(sz)))
    got = ask([shape_query(*c) for c in cases])
    seen = set()
    for c, g in zip(cases, got):
        want = M.pack_shape(*c)
        assert shape_answer(g) == want, (c, g)
        seen.add((want["slots4"], want["slots8"]))
    assert seen == {(64, 8), (64, 16), (16, 8)}
    for s, s4, s8 in itertools.product(range(4), (16, 64), (8, 16)):
        assert int(ask([f"P {s} {s4} {s8}"])[0]) == M.pack_slots(s, s4, s8)
    # the defaults by batch size, spelled out once: 16 lanes-per-item shape from 160 to 319 pictures, sixteen 8x8 blocks from 640
    d = {n: M.pack_shape(n, 1, 0, 0, False, False, 1, (0, 0, 0, 0), 0) for n in THRESHOLDS}
    assert [(d[n]["slots4"], d[n]["slots8"]) for n in THRESHOLDS] == [(64, 8), (16, 8), (16, 8), (64, 8), (64, 8), (64, 8), (64, 8), (64, 16), (64, 16), (64, 16)]


def test_pack_size_limits(ask):
    """The refusals no GPU test can reach, each at its last accepted and its first refused value.  The row limit (0x7fffffff / 4 rows)
    lies behind the wave-item limit -- a row costs four of the 0x0fffffff wave-items the bound allows -- so the largest number of rows
    a call can have is 67108862; the row limit's own boundary is refused on both sides."""
    def one(n, levels, sz, items):
        c = (n, 1, 0, 0, False, False, levels, sz, items)
        got, want = shape_answer(ask([shape_query(*c)])[0]), M.pack_shape(*c)
        assert got == want, (c, got)
        return got

    assert not one(1, 1, (0, 0, 0, 8), 0xfffffffe)["too_large"] and one(1, 1, (0, 0, 0, 8), 0xffffffff)["too_large"]  # items
    fill = 0x0fffffff - 8  # one picture, one level: the bound is 8 + the 32x32 blocks
    a, b = one(1, 1, (0, 0, 0, fill - 1), fill - 1), one(1, 1, (0, 0, 0, fill), fill)
    assert (a["waves_bound"], a["too_large"], b["waves_bound"], b["too_large"]) == (0x0ffffffe, False, 0x0fffffff, True)  # wave-items
    a, b = one(2, 33554431, (0, 0, 0, 0), 0), one(3, 22369621, (0, 0, 0, 0), 0)
    assert (a["n_rows"], a["too_large"], b["n_rows"], b["too_large"]) == (67108862, False, 67108863, True)  # rows, through the wave-items
    lim = 0x7fffffff // 4
    assert lim == 536870911 == 1 * lim and lim - 1 == 2 * 268435455
    a, b = one(2, 268435455, (0, 0, 0, 0), 0), one(1, lim, (0, 0, 0, 0), 0)
    assert (a["n_rows"], a["too_large"], b["n_rows"], b["too_large"]) == (lim - 1, True, lim, True)


def test_pack_wave_count(ask):
    resident = 4096
    cases = [(0, resident, 10, 1),  # a small call: the floor of 256
             (0, resident, 2047 * 50 + 49, 50),  # want = 2 * 2047 = 4094, below what is resident
             (0, resident, 2048 * 50, 50),  # want = resident
             (0, resident, 2049 * 50, 50),  # above: capped
             (0, 64, 10, 1),  # fewer resident waves than the floor
             (0, resident, 1000, 0),  # no levels: divided by one
             (3, resident, 2049 * 50, 50), (5000, resident, 10, 1), (resident, resident, 10, 1)]  # the knob: below, above and at resident
    got = [int(g) for g in ask([f"W {k} {r} {b} {l}" for k, r, b, l in cases])]
    assert got == [M.pack_wave_count(*c) for c in cases]
    assert got == [256, 4094, 4096, 4096, 64, 2000, 3, 4096, 4096]


# ---- the schedule ----
def test_resolve_schedule(ask):
    grid = list(itertools.product((0, 1), (0, 1), (1, 2, 383, 384, 639, 640), (0, 1), (-1, 0, 1, 3), (-1, 0, 1), (0, 1, 2, 9), (0, 1), (0, 1)))
    got = ask(["R " + " ".join(str(v) for v in g) for g in grid])
    seen = set()
    for (res, stride, n, onto, sched, across, streams, pipe, graph), g in zip(grid, got):
        want = M.resolve_schedule(bool(res), stride, n, bool(onto), sched, across, streams, bool(pipe), bool(graph))
        assert tuple(int(v) for v in g.split()) == tuple(int(v) for v in want), (res, stride, n, onto, sched, across, streams, pipe, graph)
        seen.add(want)
    assert {s[0] for s in seen} == {0, 1, 2, 3} and {s[2] for s in seen} == {1, 2, 3, 8} and {s[3] for s in seen} == {False, True}
    # the table of tests/test_gpu_parity.py's schedule walk (three pictures, one shared plan)
    assert M.resolve_schedule(False, 0, 3, False, schedule=1)[:3] == (2, True, 1)
    assert M.resolve_schedule(False, 0, 3, False, schedule=1, streams=2)[:3] == (2, True, 2)
    assert M.resolve_schedule(False, 0, 3, False, schedule=1, across=0)[:3] == (1, False, 1)
    assert M.resolve_schedule(False, 0, 3, False, schedule=0)[:3] == (0, False, 1)
    assert M.resolve_schedule(True, 0, 3, False, schedule=1)[0] == 3  # resident pools: packed whatever the knob says
