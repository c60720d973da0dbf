"""Geometrically verified matches for a pair list (the reference's
match_features + geometric_verification of evaluations/aachen/reconstruct_pipeline.py,
on the GPU and without the COLMAP database):
``python verify_pairs.py --features DIR --pairs image_pairs_to_match.txt --postfix NAME
--out verified.npz [--matcher mnn|ratio|mnn_ratio] [--ratio R] [--model fundamental|homography]
[--ransac_iters N] [--ransac_thr T] [--seed S] [--chunk PAIRS] [--guided]``.
``--guided`` matches every pair again under the model RANSAC found, each
descriptor competing only against the keypoints that model admits within the
RANSAC threshold (COLMAP's guided matching): ``matches`` then holds the guided
matches and the .npz gains ``n_verified``, the inlier counts they replace.
``--model essential --intrinsics database_intrinsics.txt`` fits five-point
essential matrices and relative poses between the calibrated cameras instead
(the .npz gains ``pose`` and ``cheir``); with ``--nvm MODEL.nvm`` it also prints
the relative-pose AUC at 5, 10 and 20 degrees against the ground-truth poses,
over the pairs whose two images are both in that file.
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
    parser.add_argument("--intrinsics", type=str, default=None)
    parser.add_argument("--nvm", type=str, default=None)
    parser.add_argument("--guided", action="store_true")
    args = parser.parse_args()
    if args.model == "essential" and args.intrinsics is None:
        parser.error("--model essential requires --intrinsics FILE")
    if args.nvm is not None and args.model != "essential":
        parser.error("--nvm goes with --model essential")
    extra = {} if args.intrinsics is None else {"intrinsics": args.intrinsics}
    if args.guided:
        extra["guided"] = True
    res = verification.verify_pair_list(
        args.features, args.pairs, args.postfix, matcher=args.matcher, ratio=args.ratio,
        model=args.model, chunk=args.chunk, iters=args.ransac_iters, thr=args.ransac_thr,
        seed=args.seed, output=args.out, **extra)
    info = res["info"]
    n = info.shape[0]
    verified = int(res["n_verified"].sum()) if args.guided else int(res["matches"].shape[0])
    print("# Pairs: {:d}, with a model: {:d}; matches {:d}, verified {:d} ({:.3f})".format(
        n, int(np.sum(info[:, 0] == 0)), int(res["n_matches"].sum()), verified,
        verified / max(1, int(res["n_matches"].sum()))))
    if args.guided:
        print("# Guided matches: {:d} ({:.3f} of the verified)".format(
            int(res["matches"].shape[0]), res["matches"].shape[0] / max(1, verified)))
    if args.nvm is not None:
        from posfeat_amd.evaluation import reconstruction, relative_pose
        gt = {n: np.concatenate([reconstruction.quat_to_rot(q), t[:, None]], 1)
              for n, (q, t) in reconstruction.read_nvm_poses(args.nvm).items()}
        rows = [p for p, (a, b) in enumerate(res["pairs"]) if a in gt and b in gt]
        world = np.asarray([gt[n] for p in rows for n in res["pairs"][p]]).reshape(-1, 3, 4)
        rel = relative_pose.relative_poses(world, [(2 * k, 2 * k + 1) for k in range(len(rows))])
        rot, trans = relative_pose.relative_pose_errors(res["pose"][rows], rel)
        auc = relative_pose.pose_auc(np.maximum(rot, trans))
        print("# Relative pose over {:d} pairs: AUC@5 {:.4f}, AUC@10 {:.4f}, AUC@20 {:.4f}".format(
            len(rows), *auc))
