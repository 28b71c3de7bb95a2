"""Fixtures from REAL reference streams whose loop filters stop at slice or tile boundaries: the clips of
make_stream_golden.py encoded with SliceMode / tiles and LFCrossSliceBoundaryFlag=0 / LFCrossTileBoundaryFlag=0, deblocking and
SAO ON, decoded by the reference under oracle/ref_decision_tap.cpp, plus what the loop filters need to know, per picture,
from the encoder's own settings (as make_stream_layout_golden.py does for region):

  slice_id{i}        index of the slice (decoding order) of every CTU in raster order
  tile_id{i}         index of the tile of every CTU in raster order
  lf_cross_slice{i}  slice_loop_filter_across_slices_enabled_flag of every slice (the encoder sets one value for all)
  lf_cross_tile{i}   loop_filter_across_tiles_enabled_flag
  region{i}, cip{i}  as in the layout fixtures (the block path needs them)

For every picture the generator checks on the CPU, and prints, what gives the fixtures their power:
  * at least one CTU-component of each edge class 0..3 is ON in a CTU with a clear availability bit inside the picture
    (case (d): over its pictures together, see below);
  * the CPU restatement with the boundaries (tests/sao_block_oracle.py: cpu_decode) IS the reference decoder's picture, and
    the restatement without them (the mask of the geometry, every edge filtered) is NOT.
A case that misses a condition is not written.  Needs /root/reference (not on the GPU box); the .npz travels.

  python tests/golden/make_stream_lf_golden.py [name ...]     # writes tests/golden/lfx_*.npz
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_stream_golden import make  # noqa: E402

import sao_block_oracle as SB  # noqa: E402
from thevc_amd import decisions as D  # noqa: E402


def check(path, control, classes_per_picture=True):
    pics = list(D.load_pictures(path))
    union = set()
    with_b, _ = SB.cpu_decode(pics, True)
    without, _ = SB.cpu_decode(pics, False)
    ok = True
    for i, p in enumerate(pics):
        avail = D.picture_avail(p)
        closed = avail != D.lf_border_avail(p["w"], p["h"], p["ctu"])
        types = p["sao"]["type"]
        classes = sorted({int(t) for t in types[:, closed].reshape(-1) if 0 <= t < 4})
        same = all(np.array_equal(with_b[i][k], p["rec"][k]) for k in range(3))
        differs = sum(int((without[i][k] != p["rec"][k]).sum()) for k in range(3))
        print(f"  poc {p['poc']}: CTUs with a closed side {int(closed.sum())}, edge classes ON there {classes}, CPU restatement "
              f"{'==' if same else '!='} reference, samples that differ without the boundaries {differs}")
        ok &= same
        if control:
            ok &= not closed.any() and differs == 0
        else:
            union |= set(classes)
            ok &= differs > 0 and (classes == [0, 1, 2, 3] or not classes_per_picture)
    return ok and (control or union == {0, 1, 2, 3})


def make_lf(name, seed, w, h, n, B, qp, cfg, slice_ctus=0, tiles=(1, 1), cross_slice=True, cross_tile=True, control=False,
            classes_per_picture=True, **kw):
    args = [f"--LFCrossSliceBoundaryFlag={int(cross_slice)}", f"--LFCrossTileBoundaryFlag={int(cross_tile)}"]
    if slice_ctus:
        args += ["--SliceMode=1", f"--SliceArgument={slice_ctus}"]
    if tiles != (1, 1):
        args += ["--UniformSpacingIdc=1", f"--NumTileColumnsMinus1={tiles[0] - 1}", f"--NumTileRowsMinus1={tiles[1] - 1}"]
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
    slice_id, tile_id = D.slice_tile_maps(w, h, ctu, starts, cb, rb)
    n_slices = int(slice_id.max()) + 1
    with tempfile.TemporaryDirectory() as d:
        make(name, seed, w, h, n, B, qp, cfg, args, out_dir=d, **kw)
        src = np.load(os.path.join(d, f"stream_{name}.npz"))
        arrays = {k: src[k] for k in src.files}
        for i in range(int(arrays["n"])):
            arrays[f"region{i}"] = region
            arrays[f"cip{i}"] = np.int32(0)
            arrays[f"slice_id{i}"] = slice_id
            arrays[f"tile_id{i}"] = tile_id
            arrays[f"lf_cross_slice{i}"] = np.full(n_slices, int(cross_slice), np.uint8)
            arrays[f"lf_cross_tile{i}"] = np.int32(int(cross_tile))
        tmp = os.path.join(d, "candidate.npz")
        np.savez_compressed(tmp, **arrays)
        print(f"lfx_{name}: {n_slices} slice(s), {int(tile_id.max()) + 1} tile(s), {os.path.getsize(tmp)} bytes")
        if not check(tmp, control, classes_per_picture):
            print(f"lfx_{name}: a condition does not hold; NOT written (choose another QP or seed)")
            return False
        np.savez_compressed(os.path.join(HERE, f"lfx_{name}.npz"), **arrays)
    return True


if __name__ == "__main__":
    only = sys.argv[1:]
    run = (lambda name: not only or name in only)
    results = []
    # (a) slices of 9 CTUs in 7-CTU rows: CTUs whose left and top neighbours are available while the top-left one is not
    if run("intra_main_q27_slices9"):
        results.append(make_lf("intra_main_q27_slices9", 41, 416, 240, 1, 8, 27, "encoder_intra_main.cfg", slice_ctus=9, cross_slice=False))
    # (b) uniform 3 x 2 tiles
    if run("intra_main_q32_tiles3x2"):
        results.append(make_lf("intra_main_q32_tiles3x2", 42, 416, 240, 1, 8, 32, "encoder_intra_main.cfg", tiles=(3, 2), cross_tile=False))
    # (c) 10 bit, 2 x 2 tiles with slices of 3 CTUs, neither crossed
    if run("intra_he10_q37_tiles_slices"):
        results.append(make_lf("intra_he10_q37_tiles_slices", 44, 416, 240, 1, 10, 37, "encoder_intra_he10.cfg", slice_ctus=3, tiles=(2, 2),
                               cross_slice=False, cross_tile=False))
    # (d) low-delay P, 2 x 1 tiles: boundary strengths from motion across a tile edge.  Four CTUs of a picture touch the tile
    # boundary and the encoder switches SAO on in few CTUs of a P picture: about 700 encodes (seeds 44..131, QP 20..40, two or
    # three pictures, moving and still content, both SAO optimisations) gave no stream with all four edge classes there in
    # EVERY picture, so this case asks for the four classes over its pictures together (each picture must still differ)
    if run("lowdelay_P_main_q38_tiles2x1"):
        results.append(make_lf("lowdelay_P_main_q38_tiles2x1", 62, 192, 128, 3, 8, 38, "encoder_lowdelay_P_main.cfg", tiles=(2, 1), cross_tile=False,
                               motion=True, classes_per_picture=False))
    # (e) the control: (a) with both flags 1 -- every bit inside the picture set, the existing path
    if run("intra_main_q27_slices9_cross"):
        results.append(make_lf("intra_main_q27_slices9_cross", 41, 416, 240, 1, 8, 27, "encoder_intra_main.cfg", slice_ctus=9, control=True))
    sys.exit(0 if all(results) else 1)
