#!/usr/bin/env python3
"""tools/kernel_usage.py FILE.s [FILE.s ...] -- what the compiler reports at the end of every kernel of an ISA listing
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only UNIT.hip): code bytes, SGPRs, VGPRs, AGPRs, scratch bytes per
lane, LDS bytes and occupancy, one line per kernel.  tools/kernel_resources.py reads the metadata records (spill counts); this one
adds the code size and the scalar registers.  Diff the outputs of two builds: a kernel a change must not touch has the same line."""
import re
import subprocess
import sys

KEYS = ("codeLenInByte", "TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "LDSByteSize", "Occupancy")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


for path in sys.argv[1:]:
    rows, cur, vals = [], None, {}
    for ln in open(path):
        t = ln.strip()
        m = re.match(r"^(_Z\w+):", t)
        if m:
            cur, vals = m.group(1), {}
            continue
        m = re.match(r"^; (\w+)\s*[:=]\s*(\d+)", t)
        if m and cur and m.group(1) in KEYS and m.group(1) not in vals:
            vals[m.group(1)] = m.group(2)
            if len(vals) == len(KEYS):
                rows.append((cur, vals))
                cur = None
    names = demangle([r[0] for r in rows])
    print(f"# {path}")
    for name, v in sorted(rows, key=lambda r: names[r[0]]):
        print(names[name] + "  " + "  ".join(f"{k} {v[k]}" for k in KEYS))
