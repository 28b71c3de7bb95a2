"""Fixtures from REAL reference streams with several slices, several tiles and constrained intra prediction: the clips of
make_stream_golden.py encoded with SliceMode / tiles / ConstrainedIntraPred, decoded by the reference under
oracle/ref_decision_tap.cpp, plus the layout the availability rule needs, per picture:

  region{i}  region id of every CTU in raster order (one per (independent slice, tile) pair; thevc_amd.decisions.region_map
             from the encoder's own slice and tile settings)
  cip{i}     constrained_intra_pred_flag (the intra flags come from the picture's coding units)

Loop filters off (PURE), so the decoder's output is the block path alone.  Needs /root/reference (not on the GPU box); the
.npz travels.

  python tests/golden/make_stream_layout_golden.py      # writes tests/golden/layout_*.npz (not stream_*: those are held to the geometric rule)
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_stream_golden import PURE, make  # noqa: E402

from thevc_amd import decisions as D  # noqa: E402


def make_layout(name, seed, w, h, n, B, qp, cfg, slice_ctus=0, tiles=(1, 1), cip=False, extra=(), **kw):
    args = list(PURE) + list(extra)
    if slice_ctus:
        args += ["--SliceMode=1", f"--SliceArgument={slice_ctus}"]
    if tiles != (1, 1):
        args += ["--UniformSpacingIdc=1", f"--NumTileColumnsMinus1={tiles[0] - 1}", f"--NumTileRowsMinus1={tiles[1] - 1}"]
    if cip:
        args += ["--ConstrainedIntraPred=1"]
    ctu = 64
    cw, ch = -(-w // ctu), -(-h // ctu)
    cb, rb = D.uniform_bounds(cw, tiles[0]), D.uniform_bounds(ch, tiles[1])
    # the reference encoder counts SliceArgument CTUs from the start of each tile (a slice ends where its tile ends)
    _, tile = D.tile_scan(cw, ch, cb, rb)
    starts = [0]
    if slice_ctus:
        first = [int(np.argmax(tile == t)) for t in range(int(tile.max()) + 1)]
        starts = [s for t, f in enumerate(first) for s in range(f, f + int((tile == t).sum()), slice_ctus)]
    region = D.region_map(w, h, ctu, starts, cb, rb)
    with tempfile.TemporaryDirectory() as d:
        make(name, seed, w, h, n, B, qp, cfg, args, out_dir=d, **kw)
        src = np.load(os.path.join(d, f"stream_{name}.npz"))
        arrays = {k: src[k] for k in src.files}
    for i in range(int(arrays["n"])):
        arrays[f"region{i}"] = region
        arrays[f"cip{i}"] = np.int32(1 if cip else 0)
    path = os.path.join(HERE, f"layout_{name}.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {len(set(region.tolist()))} regions, cip {int(cip)}")


if __name__ == "__main__":
    only = sys.argv[1:]
    run = (lambda name: not only or name in only)
    # slices of 5 CTUs in 7-CTU rows: slices start in the middle of CTU rows
    if run("intra_main_q30_slices"):
        make_layout("intra_main_q30_slices", 31, 416, 240, 2, 8, 30, "encoder_intra_main.cfg", slice_ctus=5)
    # uniform 3 x 2 tiles
    if run("intra_main_q32_tiles3x2"):
        make_layout("intra_main_q32_tiles3x2", 32, 416, 240, 1, 8, 32, "encoder_intra_main.cfg", tiles=(3, 2))
    # 2 x 2 tiles with slices of 3 CTUs (several slices per tile), 10 bit
    if run("intra_he10_q32_tiles_slices"):
        make_layout("intra_he10_q32_tiles_slices", 33, 416, 240, 1, 10, 32, "encoder_intra_he10.cfg", slice_ctus=3, tiles=(2, 2))
    # low-delay P with constrained intra prediction: intra coding units inside P pictures see only intra neighbours
    if run("lowdelay_P_main_q30_cip"):
        make_layout("lowdelay_P_main_q30_cip", 34, 192, 128, 4, 8, 30, "encoder_lowdelay_P_main.cfg", cip=True, motion=True)
    # encoder direction (flat quantiser): tiles and slices in an intra clip, and constrained intra prediction in P pictures
    if run("intra_main_q29_tiles_slices_rdoq0"):
        make_layout("intra_main_q29_tiles_slices_rdoq0", 35, 256, 192, 2, 8, 29, "encoder_intra_main.cfg", slice_ctus=4, tiles=(2, 2),
                    extra=["--RDOQ=0"], keep_org=True)
    if run("lowdelay_P_main_q28_cip_rdoq0"):
        make_layout("lowdelay_P_main_q28_cip_rdoq0", 36, 192, 128, 3, 8, 28, "encoder_lowdelay_P_main.cfg", cip=True, extra=["--RDOQ=0"],
                    motion=True, keep_org=True)
