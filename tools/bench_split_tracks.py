"""Times the split-track stage (geometry.split_tracks, posfeat_split_tracks in
triangulate.hip) on the scene of tools/bench_triangulate.py, alternating in one
process with the triangulate call whose result it splits.

The scene knows its planting (one junk edge in fifty ties two planted tracks
together), so besides the time the document says what the split recovered:
children created, inlier observations before and after, and the share of
children whose inliers all come from one planted track.

Every call gets device tensors and ends in its device-to-host read of
``counts``.  Per call: the wall time (host clock, device idle before) and the
HIP-event time; median, min and max over --reps runs after --warmup untimed
ones.  One JSON document on stdout and in --out.

  python tools/bench_split_tracks.py [--reps 7] [--warmup 2] [--cameras 256] [--rounds 2] [--out FILE]
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

from posfeat_amd import geometry  # noqa: E402
from bench_ransac_pairs import stats, timed  # noqa: E402
from bench_triangulate import scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cameras", type=int, default=256)
    ap.add_argument("--fill", type=float, default=0.4)
    ap.add_argument("--iters", type=int, default=64)
    ap.add_argument("--thr", type=float, default=4.0)
    ap.add_argument("--min_angle", type=float, default=1.5)
    ap.add_argument("--max_track", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "split_tracks",
                                                            "bench.json"))
    args = ap.parse_args()
    torch.manual_seed(1)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    planting = {}
    kp, set_off, cams, poses, edges, planted = scene(args.cameras, args.fill,
                                                     np.random.RandomState(1), planting)
    kp_d, cams_d, poses_d, edges_d = (torch.from_numpy(a).to(dev) for a in (kp, cams, poses, edges))

    def triangulate():
        res = geometry.triangulate_tracks(kp_d, set_off, cams_d, poses_d, edges_d, args.iters,
                                          args.thr, args.min_angle, args.max_track, 0)
        return res.counts.cpu().numpy(), res

    counts_in, tracks = triangulate()

    def split():
        res = geometry.split_tracks(kp_d, set_off, cams_d, poses_d, tracks, args.iters, args.thr,
                                    args.min_angle, args.rounds, 0)
        return res.counts.cpu().numpy(), res

    counts, res = split()
    again = split()[1]
    T, M = int(counts[0]), int(counts[1])
    for k in ("points", "err", "tinfo", "track_off", "parent_of", "generation"):
        assert torch.equal(getattr(res, k)[:T].view(torch.uint8),
                           getattr(again, k)[:T].view(torch.uint8)), "two calls differ in %s" % k
    for k in ("track_rows", "obs_inlier"):
        assert torch.equal(getattr(res, k)[:M], getattr(again, k)[:M]), "two calls differ in %s" % k
    assert torch.equal(res.point_of_row, again.point_of_row), "two calls differ in point_of_row"
    host = res.host()
    del res, again
    # every row is in exactly one output track, the parents are the input's
    assert np.array_equal(np.sort(host["track_rows"]), np.sort(tracks.track_rows[:M].cpu().numpy()))
    kid = host["generation"] > 0
    sizes = np.diff(host["track_off"])
    assert sizes.min() >= 2 and np.array_equal(sizes[kid], host["tinfo"][kid, 1])
    origin = planting["track_of_row"][host["track_rows"]]
    lo = np.minimum.reduceat(origin, host["track_off"][:-1])
    hi = np.maximum.reduceat(origin, host["track_off"][:-1])
    pure = kid & (lo == hi) & (lo >= 0)

    calls = (("triangulate", lambda: triangulate()[0]), ("split", lambda: split()[0]))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    t = {key: ([], []) for key, _ in calls}
    for _ in range(args.reps):                          # alternate the calls
        for key, fn in calls:
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    doc = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per call", "cameras": args.cameras, "rows": int(set_off[-1]),
           "edges": int(edges.shape[0]), "planted_tracks": planted, "iters": args.iters,
           "thr": args.thr, "min_angle": args.min_angle, "max_track": args.max_track,
           "rounds": args.rounds, "counts_in": [int(v) for v in counts_in],
           "counts": [int(v) for v in counts],
           "children_created": int(counts[6]), "parents_split": int(counts[7]),
           "children_not_fitting": int(counts[4]),
           "points_before": int(counts_in[2]), "points_after": int(counts[2]),
           "inlier_observations_before": int(counts_in[3]),
           "inlier_observations_after": int(counts[3]),
           "children_by_generation": [int((host["generation"] == g).sum())
                                      for g in range(1, args.rounds + 1)],
           "child_length": stats(sizes[kid]) if kid.any() else None,
           "children_from_one_planted_track": int(pure.sum()),
           "share_of_children_from_one_planted_track": (float(pure.sum()) / int(kid.sum())
                                                        if kid.any() else None)}
    for key in t:
        doc[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    doc["ratio_to_triangulate_event"] = (doc["split"]["event_ms"]["median"] /
                                         doc["triangulate"]["event_ms"]["median"])
    doc["ratio_to_triangulate_wall"] = (doc["split"]["wall_ms"]["median"] /
                                        doc["triangulate"]["wall_ms"]["median"])
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
