"""The C++ host mirror's TComWeightPrediction (thevc_amd/host/hmx_hm.hpp) through the mirror's own test program:
getWpScaling's derived fields, xWeightedPredictionUni and xWeightedPredictionBi on one unit, against tests/wp_oracle.py."""
import os
import subprocess

import numpy as np
import pytest

import wp_oracle as wo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "thevc_amd", "host", "hm_mirror_test")


@pytest.mark.gpu
@pytest.mark.parametrize("B,seed", [(8, 3), (10, 11)])
def test_mirror_weighted_prediction(B, seed):
    import __graft_entry__ as g
    g.build()
    out = subprocess.run([EXE, "wp", str(B), str(seed)], capture_output=True, text=True, check=True).stdout
    lines = [np.array(l.split(), np.int64) for l in out.strip().split("\n")]
    assert len(lines) == 15
    rows = [tuple([int(v) for v in lines[l][k::3]] for k in range(3)) for l in range(2)]  # (weight[3], offset[3], log2_denom[3])
    derived = wo.get_wp_scaling(rows[0], rows[1], B)
    assert [int(v) for v in lines[2]] == [v for d in derived for v in (d["offset"], d["shift"], d["round"])]
    W, H = 16, 8
    planes = [[lines[3 + 3 * s + c].astype(np.int16).reshape(H >> (1 if c else 0), W >> (1 if c else 0)) for c in range(3)] for s in range(4)]
    src0, src1, uni, bi = planes
    for c, (a, b) in enumerate(zip(uni, wo.add_weight_uni_loop(src0, rows[0], B))):
        assert np.array_equal(a, b), ("xWeightedPredictionUni", c)
    for c, (a, b) in enumerate(zip(bi, wo.add_weight_bi_loop(src0, src1, rows[0], rows[1], B))):
        assert np.array_equal(a, b), ("xWeightedPredictionBi", c)
