"""Times the point-refinement stage (geometry.refine_tracks, refine.hip) on the
scene of tools/bench_triangulate.py with the depths and focal lengths spread,
alternating in one process with the triangulate call it follows.

The scene: --cameras (256) cameras 0.45 apart on a line, every second one
SIMPLE_RADIAL, focal lengths log-uniform in 400..1600 (principal point 0.64 f,
0.48 f), 8192 keypoints each; planted 3-D points at depths log-uniform in 3..30
seen by 2..10 consecutive cameras (0.5 px noise) until --fill (0.4) of the
keypoints are used; edges and junk edges as in tools/bench_triangulate.py.

Every call gets device tensors and ends in the device-to-host read of its
``counts``.  Per call: the wall time (host clock, device idle before) and the
HIP-event time; median, min and max over --reps runs after --warmup untimed
ones.  Also tracks and residual evaluations per second (an evaluation is one
observation's residual and Jacobian at one trial point: per round the set's
members times the taken steps plus one at the least, so the figure is a lower
bound), the ratio to the triangulate call, the share of tracks that took more
than one round, the counts, and the mean reprojection error before and after.
One JSON document on stdout and in --out.

  python tools/bench_refine_points.py [--reps 7] [--warmup 2] [--cameras 256] [--out FILE]
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
from posfeat_amd.evaluation.reconstruction import summary  # noqa: E402
from bench_ransac_pairs import stats, timed  # noqa: E402

NKP, STEP, YAW, K1 = 8192, 0.45, 2.0, -0.06


def scene(ncam, fill, rs):
    """(kp [N, 2] fp32, set_off, cams, poses, edges [E, 2] int32, planted tracks):
    tools/bench_triangulate.py's construction with spread focal lengths and depths"""
    cams, poses = np.zeros((ncam, 8)), np.zeros((ncam, 12))
    foc = np.exp(rs.uniform(np.log(400.0), np.log(1600.0), ncam))
    for i in range(ncam):
        a = np.deg2rad(YAW if i % 2 else -YAW)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        cams[i, :5] = (foc[i], foc[i], 0.64 * foc[i], 0.48 * foc[i], K1 if i % 2 else 0.0)
        poses[i] = np.concatenate([R, (-R @ [STEP * i, 0.0, 0.0])[:, None]], 1).reshape(-1)
    N = ncam * NKP
    kp = np.stack([rs.uniform(0, 1.28, N), rs.uniform(0, 0.96, N)], 1) * np.repeat(foc, NKP)[:, None]
    target = int(fill * N)
    lengths = np.minimum(2 + rs.geometric(0.3, size=target) % 9, ncam)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), target))]
    T = len(lengths)
    start = (rs.uniform(0, 1, T) * (ncam - lengths + 1)).astype(np.int64)
    z = np.exp(rs.uniform(np.log(3.0), np.log(30.0), T))
    mid = STEP * (start + (lengths - 1) / 2.0)
    X = np.stack([mid + rs.uniform(-0.2, 0.2, T) * z / 3, rs.uniform(-0.2, 0.2, T) * z / 3, z], 1)
    tid = np.repeat(np.arange(T), lengths)
    first = np.concatenate([[0], np.cumsum(lengths)])[:-1]
    view = np.arange(len(tid)) - first[tid]
    cam = start[tid] + view
    P, c = poses[cam].reshape(-1, 3, 4), cams[cam]
    xc = np.einsum("nij,nj->ni", P[:, :, :3], X[tid]) + P[:, :, 3]
    xn, yn = xc[:, 0] / xc[:, 2], xc[:, 1] / xc[:, 2]
    f = 1.0 + c[:, 4] * (xn * xn + yn * yn)
    xy = np.stack([c[:, 0] * f * xn + c[:, 2], c[:, 1] * f * yn + c[:, 3]], 1)
    xy += rs.normal(0, 0.5, xy.shape)
    order = np.argsort(cam, kind="stable")
    cs = cam[order]
    rank = np.arange(len(cs)) - np.searchsorted(cs, cs, side="left")
    keep = rank < NKP
    slot = np.argsort(rs.uniform(size=(ncam, NKP)), 1)
    row = np.full(len(tid), -1, np.int64)
    row[order[keep]] = cs[keep] * NKP + slot[cs[keep], rank[keep]]
    kp[row[row >= 0]] = xy[row >= 0]
    edges = []
    for gap in (1, 2):
        a = np.flatnonzero(view + gap < lengths[tid])
        ok = (row[a] >= 0) & (row[a + gap] >= 0)
        edges.append(np.stack([row[a[ok]], row[a[ok] + gap]], 1))
    edges = np.concatenate(edges, 0)
    used = np.zeros(N, bool)
    used[row[row >= 0]] = True
    unused, members = np.flatnonzero(~used), row[row >= 0]
    njunk = int(0.3 * len(edges))
    nmerge = njunk // 50
    junk = np.concatenate([
        np.stack([rs.choice(members, njunk - nmerge), rs.choice(unused, njunk - nmerge)], 1),
        np.stack([rs.choice(members, nmerge), rs.choice(members, nmerge)], 1)], 0)
    edges = np.concatenate([edges, junk], 0)
    flip = rs.uniform(size=len(edges)) < 0.5
    edges[flip] = edges[flip][:, ::-1]
    edges = edges[rs.permutation(len(edges))]
    set_off = (np.arange(ncam + 1) * NKP).astype(np.int32)
    return kp.astype(np.float32), set_off, cams, poses, edges.astype(np.int32), T


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "refine_points",
                                                            "bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    kp, set_off, cams, poses, edges, planted = scene(args.cameras, args.fill,
                                                     np.random.RandomState(1))
    kp_d, cams_d, poses_d, edges_d = (torch.from_numpy(a).to(dev) for a in (kp, cams, poses, edges))

    def triangulate():
        res = geometry.triangulate_tracks(kp_d, set_off, cams_d, poses_d, edges_d, args.iters,
                                          args.thr, args.min_angle, args.max_track, 0)
        return res.counts.cpu().numpy(), res

    tri_counts, tri = triangulate()

    def refine():
        res = geometry.refine_tracks(kp_d, set_off, cams_d, poses_d, tri, args.thr, args.min_angle,
                                     args.rounds, args.steps)
        return res.counts.cpu().numpy(), res

    counts, res = refine()
    again = refine()[1]
    T = int(counts[0])
    for k in ("points", "err", "tinfo", "rinfo"):
        assert torch.equal(getattr(res, k)[:T].view(torch.uint8),
                           getattr(again, k)[:T].view(torch.uint8)), "two calls differ in %s" % k
    host = res.host()
    before = host.pop("unrefined")
    sizes = np.diff(host["track_off"])
    del res, again

    calls = (("triangulate", lambda: triangulate()[0]), ("refine", lambda: refine()[0]))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    t = {key: ([], []) for key, _ in calls}
    for _ in range(args.reps):                          # alternate the calls
        for key, fn in calls:
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    rinfo, tinfo = host["rinfo"], host["tinfo"]
    # per round the members of the set at every trial point and at the start;
    # the set's size is known at the end only: the final inlier count stands in
    evals = int(((rinfo[:, 1] + rinfo[:, 0]).astype(np.int64) *
                 np.maximum(tinfo[:, 1], before["tinfo"][:, 1]).astype(np.int64)).sum())
    same = (tinfo[:, 0] == 0) & (before["tinfo"][:, 0] == 0) & (rinfo[:, 3] == 0)
    w = tinfo[same, 1].astype(np.float64)
    doc = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per call", "cameras": args.cameras, "keypoints_per_camera": NKP,
           "rows": int(set_off[-1]), "edges": int(edges.shape[0]), "planted_tracks": planted,
           "thr": args.thr, "min_angle": args.min_angle, "rounds": args.rounds, "steps": args.steps,
           "triangulate_counts": [int(v) for v in tri_counts], "counts": [int(v) for v in counts],
           "track_length": stats(sizes) if len(sizes) else None,
           "tracks_longer_than_lane_kernel": int((sizes > 16).sum()),
           "share_more_than_one_round": float((rinfo[:, 0] > 1).mean()) if T else 0.0,
           "mean_taken_steps": float(rinfo[:, 1].mean()) if T else 0.0,
           "max_taken_steps": int(rinfo[:, 1].max()) if T else 0,
           "summary_before": summary(before), "summary_after": summary(host),
           "unchanged_sets": {"points": int(same.sum()),
                              "mean_reprojection_error_before":
                                  float((before["err"][same] * w).sum() / max(w.sum(), 1.0)),
                              "mean_reprojection_error_after":
                                  float((host["err"][same] * w).sum() / max(w.sum(), 1.0))},
           "residual_evaluations_lower_bound": evals}
    for key in t:
        doc[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    ev, tev = doc["refine"]["event_ms"]["median"], doc["triangulate"]["event_ms"]["median"]
    doc["tracks_per_s"] = float(T) / (ev * 1e-3)
    doc["residual_evaluations_per_s"] = float(evals) / (ev * 1e-3)
    doc["ratio_to_triangulate_event"] = ev / tev
    doc["ratio_to_triangulate_wall"] = (doc["refine"]["wall_ms"]["median"] /
                                        doc["triangulate"]["wall_ms"]["median"])
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
