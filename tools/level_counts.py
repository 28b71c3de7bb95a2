"""Dependency levels of the first picture of the REAL reference streams under tests/golden (decisions of the reference encoder):
with every available neighbour as a dependency (round 1) and with what the block's mode reads (hmx_intra_dependency_mask).
No GPU.  python3 tools/level_counts.py"""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as ol  # noqa: E402
from thevc_amd.decisions import load_pictures, split_blocks  # noqa: E402

import plan_check  # noqa: E402

O = ol.oracle()


def levels(tus, w, h, by_mode):
    """Number of dependency levels (plan_check.plan_levels: the derivation the tests hold the plans against)."""
    def mask_of(t):
        sh = 1 if t["plane"] else 0
        lx, ly, ls = int(t["x"]) << sh, int(t["y"]) << sh, (1 << int(t["log2n"])) << sh
        flags = np.zeros(4 * (ls // 4) + 1, np.uint8)
        O.hmo_intra_avail(lx, ly, ls, w, h, 64, flags)
        return plan_check.dependency_mask(t, flags) if by_mode else plan_check.flags_to_mask(flags)

    return 1 + max(plan_check.plan_levels(tus, w, h, mask_of))


for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "stream_intra*.npz"))):
    p = next(iter(load_pictures(path)))
    tus, _ = split_blocks(p)
    a, b = levels(tus, p["w"], p["h"], False), levels(tus, p["w"], p["h"], True)
    print(f"{os.path.basename(path)}: {p['w']}x{p['h']}, {len(tus)} blocks: {a} -> {b} levels ({a / b:.2f}x)")
