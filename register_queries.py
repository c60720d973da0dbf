"""Query poses from verified matches and a sparse model (the reference's
``colmap image_registrator`` and ``recover_query_poses`` steps of
evaluations/aachen/reconstruct_pipeline.py, on the GPU and without COLMAP):
``python register_queries.py --verified verified.npz --features DIR --postfix NAME
--model MODEL_DIR --queries night_time_queries_with_intrinsics.txt --out FILE
[--thr T] [--iters N] [--min_inliers K] [--min_ratio R] [--seed S]``.
verified.npz is what verify_pairs.py wrote, MODEL_DIR what triangulate_pairs.py
wrote; DIR holds ``<image name>.<postfix>`` as extract.py wrote them.  Writes
the Aachen prediction file (``basename qw qx qy qz tx ty tz`` per registered
query) and prints what posfeat_amd.evaluation.localization.register_query_list
found."""
import argparse

import numpy as np

from posfeat_amd.evaluation import localization

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--verified", type=str, required=True)
    parser.add_argument("--features", type=str, required=True)
    parser.add_argument("--postfix", type=str, required=True)
    parser.add_argument("--model", type=str, required=True)
    parser.add_argument("--queries", type=str, required=True)
    parser.add_argument("--out", type=str, required=True)
    parser.add_argument("--thr", type=float, default=12.0)
    parser.add_argument("--iters", type=int, default=1024)
    parser.add_argument("--min_inliers", type=int, default=30)
    parser.add_argument("--min_ratio", type=float, default=0.25)
    parser.add_argument("--seed", type=int, default=0)
    args = parser.parse_args()
    res = localization.register_query_list(
        args.verified, args.features, args.postfix, args.model, args.queries, thr=args.thr,
        iters=args.iters, min_inliers=args.min_inliers, min_ratio=args.min_ratio, seed=args.seed)
    localization.write_predictions(res, args.out)
    reg = res["registered"]
    print("# Registered: {:d} / {:d}, skipped pairs: {:d}".format(
        int(reg.sum()), len(res["queries"]), res["skipped_pairs"]))
    print("# Median inliers of the registered queries: {:.1f}".format(
        float(np.median(res["info"][reg, 1])) if reg.any() else 0.0))
