"""Writes tests/golden/pred_error_b{8,10,12}.npz: the scene of tests/pred_error_cases.py with the compiled reference's luma
predictions and Hadamard distortions of every candidate (pred_error_cases.ref_results: ref_set_recon + ref_predInterBlk once per
reference picture, ref_addAvg, ref_xWeightedPredictionUni / Bi, ref_getDistPart with DF_HADS).  The files carry the reference's
results to machines that do not have it.  Needs oracle/_ref/libhmref.so.  Usage: python tests/golden/make_pred_error.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import pred_error_cases as pc  # noqa: E402


def main():
    for B in (8, 10, 12):
        S = pc.scene(B)
        count = pc.check_scene(S)
        preds, hads = pc.ref_results(S, B)
        arrays = dict(org=S["org"], cands=S["cands"], weighted=S["weighted"], l0=np.array(S["l0"], np.int32), l1=np.array(S["l1"], np.int32),
                      pred=np.concatenate([p.reshape(-1) for p in preds]).astype(np.int16), had=hads)
        for i, pic in enumerate(S["pics"]):
            for k, p in zip(("y", "cb", "cr"), pic):
                arrays[f"pic{i}_{k}"] = p
        out = os.path.join(HERE, f"pred_error_b{B}.npz")
        np.savez_compressed(out, **arrays)
        print(f"{out}: {len(S['cands'])} candidates {count}, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
