#!/usr/bin/env python3
"""tools/kernel_resources.py FILE.s [FILE.s ...] -- registers, spills, LDS and scratch of every kernel in an ISA listing
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only UNIT.hip), one line per kernel: the amdhsa metadata at the end
of the file and a count of the scratch_ instructions in the kernel's body.  Diff the outputs of two builds."""
import re
import sys

FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size")
for path in sys.argv[1:]:
    scratch, cur, kernels, rec, in_meta = {}, None, {}, None, False
    for ln in open(path):
        s = ln.rstrip()
        if s.startswith("amdhsa.kernels:"):
            in_meta = True
            continue
        if in_meta:
            if s.startswith("  - "):  # the next kernel's record; its own fields are indented by four
                rec = {}
                s = "    " + s[4:]
            m = re.match(r"^    \.(\w+):\s*(\S+)", s)
            if m and rec is not None:
                rec[m.group(1)] = m.group(2)
                if m.group(1) == "name":
                    kernels[m.group(2)] = rec
            continue
        t = s.strip()
        m = re.match(r"^(_Z\w+):", t)
        if m:
            cur = m.group(1)
            scratch[cur] = 0
        elif t.startswith((".end_amdhsa_kernel", ".Lfunc_end")):
            cur = None
        elif cur and t.startswith("scratch_"):
            scratch[cur] += 1
    print(f"# {path}")
    for name in sorted(kernels):
        r = kernels[name]
        print(name + "  " + "  ".join(f"{f} {r.get(f)}" for f in FIELDS) + f"  scratch_insts {scratch.get(name, 0)}")
