"""Times the batched RANSAC fundamental-matrix stage
(geometry.ransac_fundamental_pairs, fundamental.hip) on the HPatches-shaped
pair list of tools/bench_ransac_pairs.py (100 pairs of 8192 x 128 sets, 30 %
planted correspondences), alternating in one process with the homography
stage and with the matcher that feeds both.  The planted keypoints of that
list follow homographies, which is degenerate for a fundamental matrix: the
inlier counts reported here say nothing about accuracy, the list is used
because it is the one the other two numbers were measured on.

Every call gets device tensors and ends in its device-to-host read (RANSAC:
``info``; matcher: counts and matches).  Per call: the wall time (host clock,
device idle before) and the HIP-event time; median, min and max over --reps
runs after --warmup untimed ones.  Also: (candidate x match) Sampson tests per
second -- a lane tests its three candidate slots against every match, whether
its cubic had one real root or three, so that is 3 x iters x matches per call;
(sample x match) per second is given next to it -- and the ratios to the
homography call (as measured, and per iteration) and to match_pairs.  One JSON
document on stdout and in --out.

  python tools/bench_fundamental_pairs.py [--reps 7] [--warmup 2] [--iters 2048] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from posfeat_amd import geometry, matchers as M  # noqa: E402
from bench_ransac_pairs import layout, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=2048)
    ap.add_argument("--thr", type=float, default=4.0)
    ap.add_argument("--homography_iters", type=int, default=1024)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "fundamental_pairs",
                                                            "bench.json"))
    args = ap.parse_args()
    torch.manual_seed(1)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    pool, kp_pool, set_off, pairs = layout(dev)

    def match():
        batch = M.match_pairs_device(pool, set_off, pairs, "mnn")
        batch.read()
        return batch

    batch = match()

    def fundamental():
        _, info, _ = geometry.ransac_fundamental_pairs(kp_pool, batch, args.iters, args.thr, 0)
        return info.cpu().numpy()

    def homography():
        _, info, _ = geometry.ransac_homography_pairs(kp_pool, batch, args.homography_iters, 3.0, 0)
        return info.cpu().numpy()

    info = fundamental()
    assert np.array_equal(info, fundamental()), "two calls on the same inputs differ"
    counts = batch.read()[0].astype(np.int64)
    calls = (("match_pairs", match), ("homography", homography), ("fundamental", fundamental))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    t = {key: ([], []) for key, _ in calls}
    for _ in range(args.reps):                          # alternate the calls
        for key, fn in calls:
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per pair list", "pairs": int(pairs.shape[0]), "iters": args.iters,
           "thr": args.thr, "homography_iters": args.homography_iters,
           "matches": int(counts.sum()), "matches_per_pair": stats(counts),
           "pairs_with_model": int(np.sum(info[:, 0] == 0)),
           "inliers_per_pair": stats(info[:, 1]), "refit_kept": int((info[:, 3] & 1).sum())}
    for key in t:
        res[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    ev = res["fundamental"]["event_ms"]["median"]
    per_sample = float(args.iters) * float(counts.sum()) / (ev * 1e-3)
    res["sample_matches_per_s"] = per_sample
    res["candidate_matches_per_s"] = 3.0 * per_sample        # three slots per lane
    res["ratio_to_homography_event"] = ev / res["homography"]["event_ms"]["median"]
    res["ratio_to_homography_per_iteration"] = (
        res["ratio_to_homography_event"] * args.homography_iters / args.iters)
    res["ratio_to_match_pairs_event"] = ev / res["match_pairs"]["event_ms"]["median"]
    res["ratio_to_match_pairs_wall"] = (res["fundamental"]["wall_ms"]["median"] /
                                        res["match_pairs"]["wall_ms"]["median"])
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
