"""A sparse model from verified matches and known database poses (the
reference's ``colmap point_triangulator`` step of
evaluations/aachen/reconstruct_pipeline.py, on the GPU and without COLMAP):
``python triangulate_pairs.py --verified verified.npz --features DIR --postfix NAME
--intrinsics database_intrinsics.txt --nvm MODEL.nvm --out MODEL_DIR [--thr T]
[--min_angle DEG] [--iters N] [--max_track M] [--seed S] [--refine K]
[--split K]``.
verified.npz is what verify_pairs.py wrote; DIR holds ``<image name>.<postfix>``
as extract.py wrote them.  Writes COLMAP's text model (cameras.txt, images.txt,
points3D.txt) to MODEL_DIR and prints the summary
posfeat_amd.evaluation.reconstruction.triangulate_pair_list describes.  With
--refine K (K > 0) the points are refined by K rounds of points-only bundle
adjustment on the GPU first (COLMAP's step after the triangulation); without
it the output is the triangulated points as before.  With --split K (K > 0)
the members each track's RANSAC left out are triangulated again, K generations
at the most, before any refinement: a track tied to another by a wrong match
gives both points.  Without it the output is as before."""
import argparse

from posfeat_amd.evaluation import reconstruction

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--verified", type=str, required=True)
    parser.add_argument("--features", type=str, required=True)
    parser.add_argument("--postfix", type=str, required=True)
    parser.add_argument("--intrinsics", type=str, required=True)
    parser.add_argument("--nvm", type=str, required=True)
    parser.add_argument("--out", type=str, required=True)
    parser.add_argument("--thr", type=float, default=4.0)
    parser.add_argument("--min_angle", type=float, default=1.5)
    parser.add_argument("--iters", type=int, default=64)
    parser.add_argument("--max_track", type=int, default=256)
    parser.add_argument("--seed", type=int, default=0)
    parser.add_argument("--refine", type=int, default=0)
    parser.add_argument("--split", type=int, default=0)
    args = parser.parse_args()
    res = reconstruction.triangulate_pair_list(
        args.verified, args.features, args.postfix, args.intrinsics, args.nvm, thr=args.thr,
        min_angle=args.min_angle, iters=args.iters, max_track=args.max_track, seed=args.seed,
        refine=args.refine, split=args.split)
    reconstruction.write_model(res, args.out)
    s = res["summary"]
    c = res.get("counts_unsplit", res.get("counts_unrefined", res["counts"]))
    print("# Images: {:d}, skipped pairs: {:d}, tracks: {:d} (dropped {:d}, ignored edges {:d})".format(
        len(res["images"]), res["skipped_pairs"], int(c[0]), int(c[4]), int(c[5])))
    print("# Points: {:d}\n# Observations: {:d}\n# Mean track length: {:.6f}\n"
          "# Mean reprojection error: {:.6f}px".format(
              s["points"], s["observations"], s["mean_track_length"],
              s["mean_reprojection_error"]))
    if args.split > 0:
        k = res.get("counts_unrefined", res["counts"])
        u = res["summary_unsplit"]
        print("# Split: {:d} generations at the most, {:d} parents split into {:d} more tracks\n"
              "# Before the split: {:d} points, {:d} observations".format(
                  args.split, int(k[7]), int(k[6]), u["points"], u["observations"]))
    if args.refine > 0:
        r, u = res["counts"], res["summary_unrefined"]
        print("# Refined: {:d} rounds at the most, {:d} tracks changed their inliers, {:d} fell below "
              "two inliers, {:d} failed the angle filter\n# Before refinement: {:d} points, "
              "{:.6f}px".format(args.refine, int(r[6]), int(r[3]), int(r[4]), u["points"],
                               u["mean_reprojection_error"]))
