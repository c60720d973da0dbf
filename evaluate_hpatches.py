"""HPatches MMA of extracted features (the reference's
evaluations/hpatches/evaluation.py for one method, on the GPU):
``python evaluate_hpatches.py --features ckpts/hpatches/<name>/desc
--dataset <hpatches-sequences-release> --postfix <name> [--top_k K] [--out PREFIX]``.
Prints the summary lines and the table row; writes PREFIX.npy (the object
array the reference caches: i_err, v_err, [seq_type, n_feats, n_matches]) and
PREFIX.txt (the row).  ``--homography [--ransac_iters N] [--ransac_thr T] [--seed S]``
also estimates a homography per pair (RANSAC on the same matches, on the GPU)
and prints the homography accuracy at 1 / 3 / 5 px after the row; with --out
the per-pair corner errors go to PREFIX.homography.npy."""
import argparse

import numpy as np

from posfeat_amd.evaluation import hpatches

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--features", type=str, required=True)
    parser.add_argument("--dataset", type=str, required=True)
    parser.add_argument("--postfix", type=str, required=True)
    parser.add_argument("--extension", type=str, default="ppm")
    parser.add_argument("--top_k", type=int, default=None)
    parser.add_argument("--out", type=str, default=None)
    parser.add_argument("--homography", action="store_true")
    parser.add_argument("--ransac_iters", type=int, default=1024)
    parser.add_argument("--ransac_thr", type=float, default=3.0)
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args()
    out = args.out or "hpatches_" + args.postfix
    errors = hpatches.benchmark_features(args.features, args.dataset, args.postfix,
                                         extension=args.extension, top_k=args.top_k)
    np.save(out + ".npy", np.array(errors, dtype=object))
    i_err, v_err, stats = errors
    for line in hpatches.summary_lines(stats):
        print(line)
    n_i, n_v = hpatches.seq_counts(stats)
    row = hpatches.format_row(args.postfix, stats, hpatches.mma_score(i_err, v_err, n_i, n_v))
    print(row, end="")
    with open(out + ".txt", "w") as f:
        f.write(row)
    if args.homography:
        corner_err, acc, _ = hpatches.benchmark_homography(
            args.features, args.dataset, args.postfix, extension=args.extension, top_k=args.top_k,
            iters=args.ransac_iters, thr=args.ransac_thr, seed=args.seed)
        for line in hpatches.homography_lines(acc):
            print(line)
        if args.out:
            np.save(args.out + ".homography.npy", corner_err)
