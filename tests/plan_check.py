"""Structural checks of the intra schedules, in plain Python: the dependency levels of a decision list (the one derivation
tools/level_counts.py prints and the tests assert), check_plan for the two tables of a plan (hmx_intra_plan_download) and
check_pack_tables for the packed schedule's tables of a call (hmx_last_call_pack_tables).  Nothing here looks at a picture:
a block scheduled too early is found in the tables, whether or not the race it causes would have shown.

Geometry (TComPattern.cpp:389-425 initAdiPattern): a block of n x n units (4 luma / 2 chroma samples each) at unit position
(ux, uy) of its plane has 4n + 1 neighbour units, bit u of a mask: u < 2n the left column from below-left bottom upwards,
u = 2n the corner, u > 2n the row above from left to above-right."""
import numpy as np

from thevc_amd import capi

KEY_FIELDS = ("x", "y", "log2n", "plane", "mode", "flags")


def block_units(t):
    """(plane, ux, uy, n) of a block: its position and size in units of its plane."""
    pl = int(t["plane"])
    U = 2 if pl else 4
    return pl, int(t["x"]) // U, int(t["y"]) // U, (1 << int(t["log2n"])) // U


def neighbour_unit(ux, uy, n, u):
    if u < 2 * n:
        return ux - 1, uy + 2 * n - 1 - u
    if u == 2 * n:
        return ux - 1, uy - 1
    return ux + (u - 2 * n - 1), uy - 1


def flags_to_mask(flags):
    return sum(int(b) << u for u, b in enumerate(flags))


def dependency_mask(t, flags):
    """hmx_intra_dependency_mask of a block, given its availability flags (any source)."""
    return int(capi.lib().hmx_intra_dependency_mask(1 << int(t["log2n"]), int(int(t["plane"]) == 0), int(t["mode"]), flags_to_mask(flags)))


def _grid_shape(w, h):
    return (h + 3) // 4, (w + 3) // 4  # units per plane: 4 luma samples, or 2 chroma samples of a plane half as large


def plan_levels(tus, w, h, mask_of):
    """Zero-based dependency level of every block of tus (coding order): 1 + the highest level among the blocks that cover
    the units of mask_of(t), 0 when there are none.  A block only depends on blocks before it in coding order."""
    uh, uw = _grid_shape(w, h)
    g = np.zeros((3, uh, uw), np.int32)  # level + 1 of the block that covers a unit; 0: none (yet)
    out = []
    for t in tus:
        pl, ux, uy, n = block_units(t)
        m, lv = mask_of(t), 0
        for u in range(4 * n + 1):
            if (m >> u) & 1:
                qx, qy = neighbour_unit(ux, uy, n, u)
                assert 0 <= qx < uw and 0 <= qy < uh, ("a dependency outside the picture", t, u)
                lv = max(lv, int(g[pl, qy, qx]))
        g[pl, uy:uy + n, ux:ux + n] = lv + 1
        out.append(lv)
    return out


def _key(a):
    return sorted(zip(*[a[f].tolist() for f in KEY_FIELDS]))


def table_levels(blocks, levels):
    """The level of every entry of `blocks` according to the level table, after checking the table: counts per size class,
    starts as the running sum in (level, size) order, every block covered once, no empty level."""
    levels = np.asarray(levels).reshape(-1, 8).astype(np.int64)
    start, count = levels[:, :4], levels[:, 4:]
    assert len(levels) > 0, "level table: no level"
    lv_of = np.full(len(blocks), -1, np.int64)
    off = 0
    for l in range(len(levels)):
        assert count[l].sum() > 0, f"level table: level {l} is empty"
        lo = off
        for s in range(4):
            assert start[l, s] == off, f"level table: start[{l}][{s}] = {start[l, s]}, running sum {off}"
            off += int(count[l, s])
            assert off <= len(blocks), f"level table: level {l} runs past the block list"
            cls = blocks["log2n"][start[l, s]:off].astype(np.int64) - 2
            assert (cls == s).all(), f"level table: bucket ({l}, {s}) holds blocks of other sizes"
        for s in range(4):  # (as the issue words it: per size class over the level's whole slice)
            assert int((blocks["log2n"][lo:off] == s + 2).sum()) == count[l, s], f"level table: count[{l}][{s}]"
        lv_of[lo:off] = l
    assert off == len(blocks), f"level table: counts sum to {off}, the plan has {len(blocks)} blocks"
    return lv_of


def check_plan(tus, blocks, levels, w, h, flags_of):
    """The tables of one plan against the decision list it was built from.  flags_of(t): the availability flags of a block
    from a source that is NOT the library.  Raises AssertionError naming the first violated property."""
    assert len(blocks) == len(tus) and _key(blocks) == _key(tus), "permutation: the plan's blocks are not the input blocks"
    lv_of = table_levels(blocks, levels)
    uh, uw = _grid_shape(w, h)
    cover = np.full((3, uh, uw), -1, np.int64)  # index into blocks of the block that covers a unit
    for i, t in enumerate(blocks):
        pl, ux, uy, n = block_units(t)
        want = dependency_mask(t, flags_of(t))
        assert int(t["avail"]) == want, f"stored mask: block {i} {t} holds {int(t['avail']):#x}, dependency mask of the oracle's availability {want:#x}"
        assert (cover[pl, uy:uy + n, ux:ux + n] == -1).all(), f"blocks overlap at {t}"
        cover[pl, uy:uy + n, ux:ux + n] = i
    for i, t in enumerate(blocks):
        pl, ux, uy, n = block_units(t)
        m, need = int(t["avail"]), 0
        for u in range(4 * n + 1):
            if not (m >> u) & 1:
                continue
            qx, qy = neighbour_unit(ux, uy, n, u)
            assert 0 <= qx < uw and 0 <= qy < uh, f"order: block {i} {t} depends on unit {u} outside the picture"
            j = int(cover[pl, qy, qx])
            if j < 0:
                continue  # a sparse plan: nobody writes that unit in this call
            assert lv_of[j] < lv_of[i], f"order: block {i} {t} at level {lv_of[i]} reads unit {u} of block {j} {blocks[j]} at level {lv_of[j]}"
            need = max(need, int(lv_of[j]) + 1)
        assert lv_of[i] == need, f"tightness: block {i} {t} sits at level {lv_of[i]}, its dependencies allow {need}"
    masks = {tuple(int(t[f]) for f in KEY_FIELDS[:4]): int(t["avail"]) for t in blocks}
    top = 1 + max(plan_levels(tus, w, h, lambda t: masks[tuple(int(t[f]) for f in KEY_FIELDS[:4])]))
    n_levels = len(np.asarray(levels).reshape(-1, 8))
    assert n_levels == top, f"n_levels: the plan has {n_levels} levels, the coding-order derivation {top}"


# ---- the packed schedule's tables ----
def pack_slots(s, slots4, slots8):
    return (slots4, slots8, 4, 1)[s]


def ticket_order(n_groups, n_shards, max_levels):
    """[(shard, level, group)] in ticket order: shard-major, then level, then the shard's groups ascending."""
    return [(sh, L, g) for sh in range(n_shards) for L in range(max_levels) for g in range(sh, n_groups, n_shards)]


def check_pack_tables(plans, geom, hdr, rows, descs, items, done):
    """The packed schedule's tables of a call (capi.Context.pack_tables) against the plans the call was given: plans =
    [(blocks, levels)] per picture in call order (capi.Context.plan_tables).  Everything is re-derived from the plans and
    the geometry; raises AssertionError naming the first violated property."""
    n_pics, I, n_groups, n_shards, max_levels = geom.n_pics, geom.I, geom.n_groups, geom.n_shards, geom.max_levels
    assert n_pics == len(plans) and 1 <= I <= 64
    assert n_groups == -(-n_pics // I) and n_shards == min(8, n_groups), "geometry: groups / shards"
    tabs = [np.asarray(lv).reshape(-1, 8).astype(np.int64) for _, lv in plans]
    assert max_levels == max(len(t) for t in tabs), "geometry: max_levels"
    assert geom.n_rows == max_levels * n_groups == len(rows) == len(done)
    slots = [pack_slots(s, geom.slots4, geom.slots8) for s in range(4)]
    members = lambda g: range(g * I, min((g + 1) * I, n_pics))
    # rows: counts and wave-items
    want_count = np.zeros((max_levels, n_groups, 4), np.int64)
    for L in range(max_levels):
        for g in range(n_groups):
            for p in members(g):
                if L < len(tabs[p]):
                    want_count[L, g] += tabs[p][L, 4:]
    want_waves = (-(-want_count // np.array(slots))).sum(axis=2)
    R = lambda L, g: rows[L * n_groups + g]
    for L in range(max_levels):
        for g in range(n_groups):
            r = R(L, g)
            assert r["count"].tolist() == want_count[L, g].tolist(), f"row ({L}, {g}): count {r['count']}, plans {want_count[L, g]}"
            assert int(r["n_waves"]) == want_waves[L, g], f"row ({L}, {g}): n_waves {r['n_waves']}, expected {want_waves[L, g]}"
    # ticket order: the exclusive prefix, the shards' ranges, the totals
    wb = ib = 0
    shard_first = {}
    for sh, L, g in ticket_order(n_groups, n_shards, max_levels):
        shard_first.setdefault(sh, wb)
        r = R(L, g)
        assert int(r["wave_base"]) == wb, f"row ({L}, {g}): wave_base {r['wave_base']}, prefix {wb}"
        for s in range(4):
            assert int(r["item_base"][s]) == ib, f"row ({L}, {g}): item_base[{s}] {r['item_base'][s]}, prefix {ib}"
            ib += int(want_count[L, g, s])
        wb += int(want_waves[L, g])
    assert wb == geom.n_waves == len(descs) and ib == geom.n_items == len(items)
    assert ib == sum(len(b) for b, _ in plans) == int(hdr["total_items"]), "total_items is not the sum of the plans' blocks"
    for sh in range(9):
        want = shard_first[sh] if sh < n_shards else wb
        assert int(hdr["shard_base"][sh]) == want, f"shard_base[{sh}] = {hdr['shard_base'][sh]}, expected {want}"
    # wave-items
    seen = np.zeros(len(descs), bool)
    for L in range(max_levels):
        for g in range(n_groups):
            r, row = R(L, g), L * n_groups + g
            dep = int(R(L - 1, g)["n_waves"]) if L else 0
            if L and int(r["n_waves"]):
                assert dep > 0, f"forward progress: row ({L}, {g}) has wave-items, row ({L - 1}, {g}) has none"
            w = int(r["wave_base"])
            for s in (3, 2, 1, 0):
                lo, total = int(r["item_base"][s]), int(r["count"][s])
                at = lo
                for _ in range(-(-total // slots[s])):
                    d = descs[w]
                    assert not seen[w], f"wave-item {w} belongs to two rows"
                    seen[w] = True
                    cnt = int(d["n_s"]) & 0x0fffffff
                    assert int(d["row"]) == row and int(d["n_s"]) >> 28 == s, f"wave-item {w} of row ({L}, {g}): row {d['row']}, class {int(d['n_s']) >> 28}, expected {row}, {s}"
                    # (n_waves = the ceilings above leaves no room for a wave-item that is not full, the class's last one apart)
                    assert int(d["item_off"]) == at and cnt == min(slots[s], lo + total - at), f"wave-item {w} of row ({L}, {g}): items [{d['item_off']}, +{cnt}) do not tile [{lo}, +{total}) {slots[s]} at a time"
                    assert int(d["dep_target"]) == dep, f"wave-item {w} of row ({L}, {g}): dep_target {d['dep_target']}, wave-items of the previous row {dep}"
                    assert (int(d["dep_target"]) == 0) == (L == 0)
                    at += cnt
                    w += 1
                assert at == lo + total, f"row ({L}, {g}) class {s}: the wave-items cover {at - lo} of {total} items"
            assert w == int(r["wave_base"]) + int(r["n_waves"])
    assert seen.all()
    # forward progress: what a wave-item waits for has smaller tickets, in the same shard
    sb = [int(v) for v in hdr["shard_base"]]
    for L in range(max_levels):
        for g in range(n_groups):
            r, sh = R(L, g), g % n_shards
            lo, hi = int(r["wave_base"]), int(r["wave_base"]) + int(r["n_waves"])
            assert sb[sh] <= lo <= hi <= sb[sh + 1], f"row ({L}, {g}) lies outside its shard's tickets"
            if L:
                p = R(L - 1, g)
                assert int(p["wave_base"]) + int(p["n_waves"]) <= lo, f"forward progress: row ({L}, {g}) draws tickets before row ({L - 1}, {g}) has drawn all of its own"
    # items: the blocks of level L, class s, of the group's pictures, each once, mask unchanged
    rec = lambda k, b: (k, int(b["x"]), int(b["y"]), int(b["log2n"]), int(b["plane"]) & 3, int(b["mode"]), int(b["flags"]), int(b["avail"]))
    for L in range(max_levels):
        for g in range(n_groups):
            r = R(L, g)
            for s in range(4):
                lo, total = int(r["item_base"][s]), int(r["count"][s])
                got = sorted(rec(int(b["plane"]) >> 2, b) for b in items[lo:lo + total])
                want = []
                for k, p in enumerate(members(g)):
                    if L < len(tabs[p]):
                        st, ct = int(tabs[p][L, s]), int(tabs[p][L, 4 + s])
                        want += [rec(k, b) for b in plans[p][0][st:st + ct]]
                assert got == sorted(want), f"items of row ({L}, {g}) class {s} are not the plans' blocks of that level and size"
    # counters
    assert done.tolist() == rows["n_waves"].tolist(), "completion counters: a row did not see all its wave-items"
    assert int(hdr["abort"]) == 0, "the abort word is set"
