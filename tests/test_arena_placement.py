"""Where the tables of a call go in the argument arena (thevc_amd/csrc/hmx_arena.h), on the CPU: tests/native/arena_host.cpp runs
the library's own header beside a model of the rule it replaced -- every push on its own, wrapping to offset 0 whenever it does not
fit, also in the middle of a call whose kernel is not launched yet.

  property    random calls from heads across the ring, and every list length around the sizes at which a table count times a
              struct size crosses the arena: tables of a call are disjoint, in range and consecutive, a call wraps at most once
              and only in front of its first table, it is refused exactly when its rounded tables exceed the arena together, and
              then nothing moves; a table outside the reservation is never served
  aim         the (small call, large call) pairs and the over-long calls of tests/test_gpu_long_lists.py (tests/long_list_cases.py)
              are cases the OLD rule got wrong -- it put a later table of the call over an earlier one -- and the new rule places
              or refuses.  That is the evidence that the GPU tests cover the hazard; they are never run against the old rule.
No GPU is needed."""
import os
import subprocess

import numpy as np
import pytest

import long_list_cases as ll

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CAP = ll.CAP
rounded = ll.rounded


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("arena") / "arena_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "thevc_amd", "csrc"),
                           os.path.join(HERE, "native", "arena_host.cpp"), "-o", out])
    return out


def run(exe, scenarios):
    """scenarios: [(cap, head, [(sizes, reserved), ...])] -> per scenario, per call: (new, old) with new = (status, head, offsets)
    and old = (head, offsets)."""
    text = "\n".join(f"{cap} {head} " + " ".join(f"{len(s)} {r} " + " ".join(str(v) for v in s) for s, r in calls) for cap, head, calls in scenarios)
    r = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(scenarios)
    out = []
    for line, (_, _, calls) in zip(lines, scenarios):
        t, at, res = line.split(), 0, []
        for s, _ in calls:
            k = len(s)
            assert t[at] == "N" and int(t[at + 3]) == k
            new = (int(t[at + 1]), int(t[at + 2]), [int(v) for v in t[at + 4:at + 4 + k]])
            at += 4 + k
            assert t[at] == "O" and int(t[at + 2]) == k
            old = (int(t[at + 1]), [int(v) for v in t[at + 3:at + 3 + k]])
            at += 3 + k
            res.append((new, old))
        assert at == len(t)
        out.append(res)
    return out


def full(sizes):
    """A call that reserves all its tables, as the library's entries do."""
    return sizes, len(sizes)


def overlaps(sizes, offs):
    """The pairs of tables of one call that share bytes (a table of no bytes takes no room)."""
    iv = [(o, o + rounded(s), i) for i, (s, o) in enumerate(zip(sizes, offs)) if s > 0 and o >= 0]
    return [(a[2], b[2]) for i, a in enumerate(iv) for b in iv[i + 1:] if a[0] < b[1] and b[0] < a[1]]


def check_new(cap, head, sizes, new, what):
    """The contract of reserve-then-place for one fully reserved call that started at `head`; returns the head it leaves."""
    status, head_after, offs = new
    tot = sum(rounded(s) for s in sizes)
    if tot > cap:  # refused, and nothing moved
        assert status == -1 and head_after == head and all(o == -1 for o in offs), (what, new)
        return head
    wrap = head + tot > cap
    assert status == (1 if wrap else 0), (what, new)
    at = 0 if wrap else head  # at most one wrap, in front of the first table ...
    for s, o in zip(sizes, offs):
        assert o == at and o + rounded(s) <= cap, (what, new)  # ... then side by side, inside [0, cap)
        at += rounded(s)
    assert head_after == at and not overlaps(sizes, offs), (what, new)
    return at


# ---- property ----
def test_random_calls(exe):
    rng = np.random.default_rng(20240)
    scen = []
    for _ in range(4000):
        cap = int(rng.choice([CAP, CAP, 1 << 16, 4096]))
        head = int(rng.integers(0, cap // 256 + 1)) * 256
        calls = []
        for _ in range(int(rng.integers(1, 4))):
            k = int(rng.integers(1, 5))
            kind = rng.integers(0, 4, k)  # nothing, a few bytes, a share of the ring, about the ring
            sizes = [int(0 if t == 0 else rng.integers(1, 600) if t == 1 else rng.integers(1, cap // 2) if t == 2 else rng.integers(cap - 600, cap + 600))
                     for t in kind]
            calls.append((sizes, k))
        scen.append((cap, head, calls))
    seen = {-1: 0, 0: 0, 1: 0}
    for (cap, head, calls), res in zip(scen, run(exe, scen)):
        for (sizes, _), (new, _) in zip(calls, res):
            head = check_new(cap, head, sizes, new, (cap, head, sizes))
            seen[new[0]] += 1
    assert min(seen.values()) > 300, seen  # refusals, wraps and plain placements all occurred


def test_a_table_outside_the_reservation_is_not_served(exe):
    rng = np.random.default_rng(20241)
    scen = []
    for _ in range(1000):
        head = int(rng.integers(0, CAP // 256 + 1)) * 256
        k = int(rng.integers(2, 5))
        sizes = [int(rng.integers(1, CAP // 4)) for _ in range(k)]
        scen.append((CAP, head, [(sizes, int(rng.integers(0, k)))]))  # only the first r < k tables are reserved
    for (cap, head, [(sizes, r)]), [(new, _)] in zip(scen, run(exe, scen)):
        status, head_after, offs = new
        assert status != -1
        check_new(cap, head, sizes[:r], (status, head_after, offs[:r]), (head, sizes, r))  # the reserved tables, as ever
        # nothing is left of the reservation, so every later table is turned away -- never wrapped onto the first ones
        assert offs[r:] == [-1] * (len(sizes) - r), (head, sizes, r, new)


def boundary_lengths():
    """List lengths at which a table count times a struct size crosses the arena, +-2, per entry: 262144 (28n + 4n), 299593 (28n),
    349525 (24n), 419430 (20n), 524288 (16n) for today's structs, and the longest list of each entry."""
    marks = {CAP // (ll.ME_UNIT + 12), CAP // (ll.ME_UNIT + 8), CAP // (ll.ME_UNIT + 4), CAP // ll.ME_UNIT, CAP // (ll.PU + 4), CAP // ll.PU}
    assert marks == {262144, 299593, 349525, 419430, 524288}  # the structs have not changed size
    return {e: sorted({m + d for m in marks | {ll.largest(e)} for d in (-2, -1, 0, 1, 2)}) for e in ll.ENTRIES}


def test_list_lengths_at_the_arena_boundaries(exe):
    scen = []
    for e, lengths in boundary_lengths().items():
        for n in lengths:
            sizes = ll.tables(e, n)
            tot = sum(rounded(s) for s in sizes)
            # heads: a coarse walk over the ring, and every step around the places where the old rule changed its mind
            marks = [0, rounded(4 * n), 2 * rounded(4 * n), rounded(8 * n), CAP - tot, CAP - rounded(sizes[0]), CAP - rounded(sizes[0]) - rounded(sizes[1]), CAP]
            heads = set(range(0, CAP + 1, 1 << 16)) | {m + 256 * d for m in marks for d in range(-4, 5)}
            scen += [(CAP, h, [full(sizes)]) for h in sorted(heads) if 0 <= h <= CAP]
    assert len(scen) > 10000
    for (cap, head, [(sizes, _)]), [(new, _)] in zip(scen, run(exe, scen)):
        check_new(cap, head, sizes, new, (head, sizes))
    for e in ll.ENTRIES:  # the longest list is accepted from every head, one more unit is refused
        assert ll.total(e, ll.largest(e)) <= CAP < ll.total(e, ll.largest(e) + 1)


# ---- aim ----
@pytest.mark.parametrize("entry", ll.ENTRIES)
def test_gpu_pairs_hit_what_the_old_rule_got_wrong(exe, entry):
    big = ll.tables(entry, ll.LARGE[entry])
    assert sum(rounded(s) for s in big) <= CAP  # "fits": the large call is one the contract accepts
    scen = [(CAP, 0, [full(ll.tables(entry, m)), full(big)]) for m in ll.SMALL[entry]]
    heads = []
    for (cap, _, calls), res in zip(scen, run(exe, scen)):
        (new_s, old_s), (new_l, old_l) = res
        head = check_new(cap, 0, calls[0][0], new_s, "small call")
        assert old_s == (new_s[1], new_s[2]) and not overlaps(calls[0][0], old_s[1])  # from a fresh context the small call was fine
        heads.append(head)
        check_new(cap, head, big, new_l, "large call")
        assert new_l[0] == 1  # it wraps, once, in front
        assert -1 not in old_l[1] and overlaps(big, old_l[1]), (entry, head, old_l)  # the old rule served it, tables on top of each other
    assert len(set(heads)) == len(heads) >= 6


@pytest.mark.parametrize("entry", ll.ENTRIES)
def test_gpu_refusals_hit_what_the_old_rule_served(exe, entry):
    scen = [(CAP, 0, [full(ll.tables(entry, n)), full(ll.tables(entry, ll.AFTER_REFUSAL))]) for n in ll.TOO_LONG[entry]]
    for (cap, _, calls), res in zip(scen, run(exe, scen)):
        (new, old), (new_after, _) = res
        assert all(rounded(s) <= CAP for s in calls[0][0])  # every table fits alone: the old check passed
        assert -1 not in old[1] and overlaps(calls[0][0], old[1]), (entry, old)
        assert new == (-1, 0, [-1] * len(calls[0][0]))  # refused, head still 0
        assert check_new(cap, 0, calls[1][0], new_after, "after a refusal") == ll.total(entry, ll.AFTER_REFUSAL)


def test_gpu_controls(exe):
    """The remaining calls of the GPU tests: the large call first on a context and twice in a row, the longest list and one more,
    the sub-pel search's single table.  No rule overlaps here; the new one must place, wrap in front, or refuse."""
    for e in ll.ENTRIES:
        big = ll.tables(e, ll.LARGE[e])
        [[(a, _), (b, _)]] = run(exe, [(CAP, 0, [full(big), full(big)])])
        assert a[0] == 0 and b[0] == 1 and check_new(CAP, check_new(CAP, 0, big, a, e), big, b, e) == ll.total(e, ll.LARGE[e])
    for e in ("fullpel", "pred_error"):
        n = ll.largest(e)
        [[(a, _)], [(b, _)]] = run(exe, [(CAP, 0, [full(ll.tables(e, n))]), (CAP, 0, [full(ll.tables(e, n + 1))])])
        assert a[0] == 0 and a[1] == ll.total(e, n) <= CAP and b[0] == -1
    [[(new, old)]] = run(exe, [(CAP, 0, [full(ll.tables("subpel_search", ll.TOO_LONG_SUBPEL_SEARCH))])])
    assert new == (-1, 0, [-1]) and old == (0, [-1])
    assert ll.total("subpel_search", ll.TOO_LONG_SUBPEL_SEARCH - 1) == CAP
