"""Times guided matching (matchers.match_pairs_guided_device,
posfeat_match_pairs_guided in matchpairs.hip) on the HPatches-shaped pair list
of tools/bench_ransac_pairs.py (100 pairs of 8192 x 128 sets, 30 % planted
correspondences with keypoints), alternating in one process with the unguided
matcher and with the RANSAC fundamental call whose F it matches under.  As in
tools/bench_fundamental_pairs.py the planted keypoints follow homographies, so
F is one member of a degenerate family: the counts reported here say nothing
about accuracy; the list is the one the other numbers were measured on.  The
guided call is also timed under the RANSAC homographies of the same list.

Every call gets device tensors and ends in its device-to-host read (matchers:
counts and matches; RANSAC: ``info``).  Per call: the wall time (host clock,
device idle before) and the HIP-event time; median, min and max over --reps
runs after --warmup untimed ones, and the guided / unguided ratios.  One JSON
document on stdout and in --out.

  python tools/bench_guided_pairs.py [--reps 7] [--warmup 2] [--iters 2048] [--out FILE]
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
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "guided_pairs",
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
    F, info, _ = geometry.ransac_fundamental_pairs(kp_pool, batch, args.iters, args.thr, 0)
    H, hinfo, _ = geometry.ransac_homography_pairs(kp_pool, batch, 1024, 3.0, 0)

    def fundamental():
        _, i, _ = geometry.ransac_fundamental_pairs(kp_pool, batch, args.iters, args.thr, 0)
        return i.cpu().numpy()

    def guided_f():
        return geometry.guided_pairs(kp_pool, batch, "fundamental", F, args.thr, "mnn").read()

    def guided_h():
        return geometry.guided_pairs(kp_pool, batch, "homography", H, args.thr, "mnn").read()

    gf = [x.copy() for x in guided_f()]
    again = guided_f()
    assert np.array_equal(gf[0], again[0]), "two guided calls on the same inputs differ"
    gh = guided_h()[0].astype(np.int64)
    counts = batch.read()[0].astype(np.int64)
    calls = (("match_pairs", match), ("fundamental", fundamental), ("guided_fundamental", guided_f),
             ("guided_homography", guided_h))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    t = {key: ([], []) for key, _ in calls}
    for _ in range(args.reps):                          # alternate the calls
        for key, fn in calls:
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    info = info.cpu().numpy()
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per pair list", "pairs": int(pairs.shape[0]), "iters": args.iters,
           "thr": args.thr, "matches": int(counts.sum()), "matches_per_pair": stats(counts),
           "verified_per_pair": stats(info[:, 1]),
           "guided_fundamental_matches_per_pair": stats(gf[0].astype(np.int64)),
           "guided_homography_matches_per_pair": stats(gh)}
    for key in t:
        res[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    for key in ("guided_fundamental", "guided_homography"):
        res["ratio_%s_to_match_pairs_event" % key] = (
            res[key]["event_ms"]["median"] / res["match_pairs"]["event_ms"]["median"])
        res["ratio_%s_to_match_pairs_wall" % key] = (
            res[key]["wall_ms"]["median"] / res["match_pairs"]["wall_ms"]["median"])
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
