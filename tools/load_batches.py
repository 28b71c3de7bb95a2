#!/usr/bin/env python3
"""tools/load_batches.py FILE.s [KERNEL-SUBSTRING] -- how the vector-memory loads of a kernel are batched, per marked section.
Build the ISA as for tools/section_mix.py (-DHMX_MARKS -S --cuda-device-only).  For every section (the instructions behind a
"; HMXMARK n id" comment, in layout order: an approximation where the compiler moved code across a mark) it prints

  * the sequence of vector-memory events:  L load, S store, A atomic (global / flat / buffer),  l / s scratch load / store,
    wN = s_waitcnt with vmcnt(N); a load or store with the non-temporal hint carries an n (Ln: the originals, Sn: the levels),
    one that bypasses the vector L1 (sc1) a c (Lc: the dependency poll and the reference gather);
  * serial round trips: the waits that have a load (L, l or A) between them and the previous wait -- each is one trip to the L2 or
    to HBM that the wave sits out; loads that are issued back to back and waited for once count as one;
  * the scratch accesses of the section;

and for the kernel its vgpr_count, vgpr_spill_count and LDS size from the code object's metadata.  It looks at loads, stores and
wait counts only: what an instruction computes, and every other instruction, is none of its business."""
import re
import sys

path, want = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "k_intra_packedILb1ELi64ELb0ELb0ELi16")
MEM = re.compile(r"^(global|flat|buffer|scratch)_(load|store|atomic)")


def events(path, want):
    """[(section, [event, ...])] of the first kernel whose name contains `want`, and that name"""
    name, cur, out = None, None, []
    for ln in open(path):
        s = ln.strip()
        m = re.match(r"^(_Z\w+):", s)
        if m:
            if name is None and want in m.group(1):
                name, cur = m.group(1), []
                out.append(("entry", cur))
            elif cur is not None:
                break
            continue
        if cur is None or not s:
            continue
        if s.startswith((".end_amdhsa_kernel", ".Lfunc_end")):
            break
        m = re.search(r"; HMXMARK (0x[0-9a-f]+|\d+) (\d+)", s)
        if m:
            cur = []
            out.append((f"N={int(m.group(1), 0)} s{m.group(2)}", cur))
            continue
        if s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        op = s.split()[0]
        m = MEM.match(op)
        if m:
            ev = {"load": "L", "store": "S", "atomic": "A"}[m.group(2)]
            mods = s.split(";")[0].split()
            cur.append(ev.lower() if m.group(1) == "scratch" else ev + ("n" if "nt" in mods else "") + ("c" if "sc1" in mods and ev != "A" else ""))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                cur.append("w" + m.group(1))
    return name, out


def metadata(path, name):
    """vgpr_count, vgpr_spill_count, LDS bytes of kernel `name` (the amdhsa.kernels list at the end of the file)"""
    entry, found = {}, None
    for ln in open(path):
        if re.match(r"^  - \.", ln):  # a new entry of amdhsa.kernels
            if entry.get(".name") == name:
                found = entry
            entry = {}
            ln = "    " + ln[4:]
        m = re.match(r"^    (\.\w+):\s*(\S+)\s*$", ln)
        if m:
            entry[m.group(1)] = m.group(2)
    if entry.get(".name") == name:
        found = entry
    return found or {}


name, secs = events(path, want)
if name is None:
    raise SystemExit(f"no kernel matching {want!r} in {path}")
print(f"kernel {name}")
md = metadata(path, name)
print(f"vgpr_count {md.get('.vgpr_count', '?')}  vgpr_spill_count {md.get('.vgpr_spill_count', '?')}  sgpr_spill_count {md.get('.sgpr_spill_count', '?')}  "
      f"lds_bytes {md.get('.group_segment_fixed_size', '?')}")
tot_trips = tot_scratch = 0
merged, order = {}, []
for sec, ev in secs:  # a section the compiler laid out in several pieces: the pieces in layout order
    if sec not in merged:
        merged[sec] = []
        order.append(sec)
    merged[sec] += ev
for sec in order:
    ev = merged[sec]
    if not ev:
        continue
    trips, pending = 0, False
    for e in ev:
        if e[0] in "LlA":
            pending = True
        elif e[0] == "w" and pending:
            trips, pending = trips + 1, False
    scratch = sum(e in ("l", "s") for e in ev)
    tot_trips += trips
    tot_scratch += scratch
    print(f"{sec:10s} round trips {trips:2d}  scratch {scratch:2d}  | {' '.join(ev)}")
print(f"{'total':10s} round trips {tot_trips:2d}  scratch {tot_scratch:2d}")
