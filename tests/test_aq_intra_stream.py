"""tests/golden/aq_intra_stream.npz (make_aq_intra_stream.py: the reference encoder under --AdaptiveQP=1, all-intra) held against the
per-block-QP yardstick on the CPU: the fixture's internal consistency.  No GPU."""
import os

import numpy as np
import pytest

import aq_oracle as ao
import qp_map_oracle as qo
from thevc_amd.decisions import levels_to_planes

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aq_intra_stream.npz")


@pytest.fixture(scope="module")
def clips():
    return qo.load_aq_intra_stream(FIXTURE)


def test_shape_of_the_fixture(clips):
    assert [(c["B"], c["ctu"], c["k"]) for c, _ in clips] == [(8, 64, 2), (10, 32, 1)]
    for cfg, pics in clips:
        assert len(pics) == 2
        for p in pics:
            assert (p["w"], p["h"], p["B"], p["ctu"], p["slice_type"]) == (208, 120, cfg["B"], cfg["ctu"], 2)
            assert p["qp_map"].shape == (30, 52) and p["qp_map"].dtype == np.int8 and p["cu_depth"].shape == (30, 52)
            assert abs(p["qp_map"].astype(int) - p["qp"]).max() <= cfg["range"]
    assert os.path.getsize(FIXTURE) < (1 << 20)


def test_decode_with_the_map_is_the_reference_decoder(clips):
    for cfg, pics in clips:
        for p in pics:
            lev = levels_to_planes(p)
            got = qo.decode(p["tus"], p["w"], p["h"], p["B"], lev, p["qp_map"], 1, 0, p["ctu"])
            flat = qo.decode(p["tus"], p["w"], p["h"], p["B"], lev, np.full_like(p["qp_map"], p["qp"]), 1, 0, p["ctu"])
            for k in range(3):
                assert np.array_equal(got[k], p["rec"][k]), (cfg, p["poc"], k)
            assert any(not np.array_equal(flat[k], p["rec"][k]) for k in range(3)), "the slice QP alone reproduces the picture"


def test_encode_with_the_map_gives_the_streams_levels(clips):
    """RDOQ was off: with the decisions and the QPs the flat quantiser's levels are the ones the encoder wrote -- the reference's xQuant,
    which takes its right shift from the slice's base QP (qp_map_oracle._quant) while the scale follows the block's QP; with the shift
    from the block's own QP the levels differ."""
    for cfg, pics in clips:
        for p in pics:
            rec, lev = qo.encode_blockwise(p["tus"], p["w"], p["h"], p["B"], p["org"], p["qp_map"], 1, 0, p["ctu"], 0, p["qp"])
            _, own = qo.encode(p["tus"], p["w"], p["h"], p["B"], p["org"], p["qp_map"], 1, 0, p["ctu"])
            assert any(not np.array_equal(own[k], lev[k]) for k in range(3))
            want = levels_to_planes(p)
            for k in range(3):
                assert np.array_equal(lev[k], want[k]) and np.array_equal(rec[k], p["rec"][k]), (cfg, p["poc"], k)


def test_maps_are_the_aq_oracles(clips):
    """The unit map restated: every coding unit's QP is xComputeQP of the ORIGINAL at layer min(depth, k), the depth map is the
    coding units'; the coded blocks of every picture use at least four QPs."""
    for cfg, pics in clips:
        for p in pics:
            ctu, k, B = p["ctu"], cfg["k"], p["B"]
            g = ao.Geom(p["w"], p["h"], ctu, k + 1)
            act, avg = ao.preanalyze(p["org"][0], ctu, k + 1)
            for c in p["cus"]:
                s, x, y = 1 << int(c["log2size"]), int(c["x"]), int(c["y"])
                depth = (ctu.bit_length() - 1) - int(c["log2size"])
                want = ao.compute_qp(g, act, avg, x, y, depth, p["qp"], cfg["range"], 6 * (B - 8))
                assert (p["qp_map"][y // 4:(y + s) // 4, x // 4:(x + s) // 4] == want).all(), (p["poc"], x, y, s)
                assert (p["cu_depth"][y // 4:(y + s) // 4, x // 4:(x + s) // 4] == depth).all()
            lev = levels_to_planes(p)
            coded = {qo.block_qp(t, p["qp_map"]) for t in p["tus"]
                     if lev[int(t["plane"])][int(t["y"]):int(t["y"]) + (1 << int(t["log2n"])), int(t["x"]):int(t["x"]) + (1 << int(t["log2n"]))].any()}
            assert len(coded) >= 4, coded
