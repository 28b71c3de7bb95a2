"""The calls of tests/test_gpu_long_lists.py as table sizes, shared with tests/test_arena_placement.py, which shows on the CPU that
the pairs the GPU tests issue are pairs the old placement rule got wrong.

The argument arena (thevc_amd/csrc/hmx_arena.h) is a ring of CAP bytes with 256-byte steps.  An entry over a unit or candidate
list puts two or three host tables there before its one launch; `tables` gives their byte sizes in the order the entry puts them
(thevc_amd/csrc/hmx_me.hip, hmx_inter.hip), from the struct sizes capi declares."""
from thevc_amd import capi

CAP = 8 << 20
ALIGN = 256
ME_UNIT, PU, TZ_UNIT = capi.ME_UNIT_DTYPE.itemsize, capi.PU_DTYPE.itemsize, capi.TZ_UNIT_DTYPE.itemsize
N_CAND = 2   # hmx_batch_subpel_cost: candidates per unit
GROUP = 5    # hmx_batch_inter_pred_error: candidates per group, bits given
ENTRIES = ("fullpel", "tz", "subpel_cost", "pred_error")


def rounded(b):
    return (b + ALIGN - 1) // ALIGN * ALIGN


def n_groups(n):
    return (n + GROUP - 1) // GROUP


def tables(entry, n):
    if entry == "fullpel":       # units, tile_first, map_first
        return [ME_UNIT * n, 4 * (n + 1), 4 * (n + 1)]
    if entry == "tz":            # units, tz
        return [ME_UNIT * n, TZ_UNIT * n]
    if entry == "subpel_cost":   # pus, first, offs
        return [PU * n, 4 * (n + 1), 2 * N_CAND]
    if entry == "pred_error":    # cands, bits, group_first
        return [PU * n, 4 * n, 4 * (n_groups(n) + 1)]
    if entry == "subpel_search":  # units
        return [ME_UNIT * n]
    raise KeyError(entry)


def total(entry, n):
    return sum(rounded(b) for b in tables(entry, n))


def largest(entry):
    """The longest list one call of `entry` takes: the largest n whose rounded tables fit CAP together (total is monotonic in n)."""
    lo, hi = 1, CAP
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if total(entry, mid) <= CAP:
            lo = mid
        else:
            hi = mid - 1
    return lo


# ---- what the GPU tests issue ----
# "fits, head low": a small call, then without a wait the large one.  The large call's tables fit the arena together, but from the
# head the small call leaves the old rule wrapped in the middle of the large call and put a later table over its first one.
LARGE = {"fullpel": 280000, "tz": 280000, "subpel_cost": 400000, "pred_error": 400000}
SMALL = {"fullpel": (20000, 24000, 28000, 32000, 39000, 65000),      # heads in (cap - 28n, 4n); 65000: tile_first wraps, map_first lands on the units
         "tz": (20000, 30000, 40000, 50000, 65000, 79000),           # heads in (cap - 28n, 8n)
         "subpel_cost": (20000, 30000, 40000, 50000, 65000, 79000),  # heads in (cap - 20n, 4n)
         "pred_error": (5000, 10000, 20000, 50000, 70000, 90000)}    # 5000, 10000 and 90000: only group_first lands on the candidates
# "does not fit": every table fits alone, the tables together do not -- the old rule served these from head 0 by overwriting
TOO_LONG = {"fullpel": (300000, 419430), "tz": (300000, 419430), "subpel_cost": (420000, 524288), "pred_error": (420000, 524288)}
TOO_LONG_SUBPEL_SEARCH = 419431  # one table that alone exceeds the arena: refused before and after
AFTER_REFUSAL = 1000             # the small call that follows a refusal on the same context
