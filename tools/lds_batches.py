#!/usr/bin/env python3
"""tools/lds_batches.py FILE.s [KERNEL-SUBSTRING] -- how the LDS reads of a kernel are batched, per marked section: the LDS twin of
tools/load_batches.py.  Build the ISA as for tools/section_mix.py (-DHMX_MARKS -S --cuda-device-only).  For every section (the
instructions behind a "; HMXMARK n id" comment, in layout order: an approximation where the compiler moved code across a mark) it
prints

  * the sequence of LDS events:  R = ds_read* (R2 = a ds_read2* pair, one instruction), W = ds_write*, P = a lane exchange through
    the LDS crossbar (ds_bpermute / ds_permute / ds_swizzle: no memory, the same counter),  wN = s_waitcnt with lgkmcnt(N),
    B = s_cbranch*.  Runs of one event are folded: "R2x8" is eight ds_read2 back to back;
  * serial round trips: the waits that have a read (R or P) between them and the previous wait -- each is one trip to the LDS that
    the wave sits out; reads that are issued back to back and waited for once count as one.  (lgkmcnt also counts scalar loads;
    a wait for one of those alone has no R in front of it and is not counted);
  * the counts of reads, writes, waits and branches, and of v_mad_u64_u32 (the one multiply that issues at half rate: what the
    compiler makes of a product whose operands it cannot bound);

and for the kernel its vgpr_count, vgpr_spill_count and LDS size from the code object's metadata.  It looks at LDS instructions,
wait counts and branches only: what an instruction computes is none of its business."""
import re
import sys

path, want = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "k_intra_packedILb1ELi64ELb0ELb0ELi16")


def events(path, want):
    """[(section, [event, ...], n_mad64)] of the first kernel whose name contains `want`, and that name"""
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
        if op.startswith("ds_read"):
            cur.append("R2" if op.startswith("ds_read2") else "R")
        elif op.startswith("ds_write"):
            cur.append("W")
        elif op.startswith(("ds_bpermute", "ds_permute", "ds_swizzle")):
            cur.append("P")
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", s)
            if m:
                cur.append("w" + m.group(1))
        elif op.startswith("s_cbranch"):
            cur.append("B")
        elif op == "v_mad_u64_u32":
            cur.append("M")
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


def fold(ev):
    out, i = [], 0
    while i < len(ev):
        j = i
        while j < len(ev) and ev[j] == ev[i]:
            j += 1
        out.append(ev[i] if j - i == 1 else f"{ev[i]}x{j - i}")
        i = j
    return " ".join(out)


name, secs = events(path, want)
if name is None:
    raise SystemExit(f"no kernel matching {want!r} in {path}")
print(f"kernel {name}")
md = metadata(path, name)
print(f"vgpr_count {md.get('.vgpr_count', '?')}  vgpr_spill_count {md.get('.vgpr_spill_count', '?')}  sgpr_spill_count {md.get('.sgpr_spill_count', '?')}  "
      f"lds_bytes {md.get('.group_segment_fixed_size', '?')}")
tot = [0] * 6
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
        if e[0] in "RP":
            pending = True
        elif e[0] == "w" and pending:
            trips, pending = trips + 1, False
    row = [trips, sum(e[0] == "R" for e in ev), sum(e == "W" for e in ev), sum(e[0] == "w" for e in ev), sum(e == "B" for e in ev),
           sum(e == "M" for e in ev)]
    tot = [a + b for a, b in zip(tot, row)]
    print(f"{sec:10s} round trips {row[0]:3d}  reads {row[1]:3d}  writes {row[2]:3d}  waits {row[3]:3d}  branches {row[4]:3d}  mad_u64 {row[5]:2d}  | "
          f"{fold([e for e in ev if e != 'M'])}")
print(f"{'total':10s} round trips {tot[0]:3d}  reads {tot[1]:3d}  writes {tot[2]:3d}  waits {tot[3]:3d}  branches {tot[4]:3d}  mad_u64 {tot[5]:2d}")
