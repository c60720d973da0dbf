"""Geometrically verified matches for a pair list (the reference's
match_features + geometric_verification of evaluations/aachen/reconstruct_pipeline.py,
on the GPU and without the COLMAP database):
``python verify_pairs.py --features DIR --pairs image_pairs_to_match.txt --postfix NAME
--out verified.npz [--matcher mnn|ratio|mnn_ratio] [--ratio R] [--model fundamental|homography]
[--ransac_iters N] [--ransac_thr T] [--seed S] [--chunk PAIRS]``.
DIR holds ``<image name>.<postfix>`` as extract.py wrote them.  Writes the .npz
posfeat_amd.evaluation.verification.verify_pair_list describes (pair names,
inlier matches with per-pair offsets, the model and the RANSAC info per pair)
and prints one summary line."""
import argparse

import numpy as np

from posfeat_amd.evaluation import verification

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--features", type=str, required=True)
    parser.add_argument("--pairs", type=str, required=True)
    parser.add_argument("--postfix", type=str, required=True)
    parser.add_argument("--out", type=str, required=True)
    parser.add_argument("--matcher", type=str, default="mnn")
    parser.add_argument("--ratio", type=float, default=0.95)
    parser.add_argument("--model", type=str, default="fundamental")
    parser.add_argument("--ransac_iters", type=int, default=None)
    parser.add_argument("--ransac_thr", type=float, default=None)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--chunk", type=int, default=1024)
    args = parser.parse_args()
    res = verification.verify_pair_list(
        args.features, args.pairs, args.postfix, matcher=args.matcher, ratio=args.ratio,
        model=args.model, chunk=args.chunk, iters=args.ransac_iters, thr=args.ransac_thr,
        seed=args.seed, output=args.out)
    info = res["info"]
    n = info.shape[0]
    print("# Pairs: {:d}, with a model: {:d}; matches {:d}, verified {:d} ({:.3f})".format(
        n, int(np.sum(info[:, 0] == 0)), int(res["n_matches"].sum()), int(res["matches"].shape[0]),
        res["matches"].shape[0] / max(1, int(res["n_matches"].sum()))))
