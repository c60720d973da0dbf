"""Times the track-building and triangulation stage (geometry.triangulate_tracks,
triangulate.hip) on a synthetic scene shaped like an Aachen chunk, alternating
in one process with the batched RANSAC fundamental-matrix stage
(geometry.ransac_fundamental_pairs) on the pair list of
tools/bench_ransac_pairs.py, whose match rows are of the same order as the
edges here.

The scene: --cameras (256) cameras 0.45 apart on a line, every second one
SIMPLE_RADIAL, 8192 keypoints each; planted 3-D points seen by 2..10
consecutive cameras (0.5 px noise) until --fill (0.4) of the keypoints are
used; per track the edges (k, k + 1) and (k, k + 2) of its views; then 30 % junk
edges on top: most tie an unused keypoint to a track (an outlier observation),
one in fifty ties two tracks together.  Edges are shuffled.

Every call gets device tensors and ends in its device-to-host read
(triangulation: ``counts``; RANSAC: ``info``).  Per call: the wall time (host
clock, device idle before) and the HIP-event time; median, min and max over
--reps runs after --warmup untimed ones.  Also edges and tracks per second and
the ratio to the fundamental call, as measured and per edge / match row.  The
share of time per launch is not collected (it would take a profiler run).  One
JSON document on stdout and in --out.

  python tools/bench_triangulate.py [--reps 7] [--warmup 2] [--cameras 256] [--out FILE]
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

NKP, STEP, YAW, K1 = 8192, 0.45, 2.0, -0.06


def cameras(n):
    cams, poses = np.zeros((n, 8)), np.zeros((n, 12))
    for i in range(n):
        a = np.deg2rad(YAW if i % 2 else -YAW)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        cams[i, :5] = (500.0, 500.0, 320.0, 240.0, K1 if i % 2 else 0.0)
        poses[i] = np.concatenate([R, (-R @ [STEP * i, 0.0, 0.0])[:, None]], 1).reshape(-1)
    return cams, poses


def scene(ncam, fill, rs, planting=None):
    """(kp [N, 2] fp32, set_off, cams, poses, edges [E, 2] int32, number of planted tracks);
    a dict ``planting`` gets 'track_of_row' [N]: the planted track of a row, -1 for none"""
    cams, poses = cameras(ncam)
    N = ncam * NKP
    kp = np.stack([rs.uniform(0, 640, N), rs.uniform(0, 480, N)], 1)
    target = int(fill * N)
    # 2..10 views, short tracks most often
    lengths = np.minimum(2 + rs.geometric(0.3, size=target) % 9, ncam)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), target))]
    T = len(lengths)
    start = (rs.uniform(0, 1, T) * (ncam - lengths + 1)).astype(np.int64)
    z = rs.uniform(4, 9, T)
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
    # the next free row of its camera for every observation, rows in random order
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
    if planting is not None:
        planting["track_of_row"] = np.full(N, -1, np.int64)
        planting["track_of_row"][row[row >= 0]] = tid[row >= 0]
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
    ap.add_argument("--fundamental_iters", type=int, default=2048)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "triangulate",
                                                            "bench.json"))
    args = ap.parse_args()
    torch.manual_seed(1)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    kp, set_off, cams, poses, edges, planted = scene(args.cameras, args.fill,
                                                     np.random.RandomState(1))
    kp_d, cams_d, poses_d, edges_d = (torch.from_numpy(a).to(dev) for a in (kp, cams, poses, edges))

    def triangulate():
        res = geometry.triangulate_tracks(kp_d, set_off, cams_d, poses_d, edges_d, args.iters,
                                          args.thr, args.min_angle, args.max_track, 0)
        return res.counts.cpu().numpy(), res

    counts, res = triangulate()
    again = triangulate()[1]
    T = int(counts[0])
    for k in ("points", "err", "tinfo"):
        assert torch.equal(getattr(res, k)[:T].view(torch.uint8),
                           getattr(again, k)[:T].view(torch.uint8)), "two calls differ in %s" % k
    host = res.host()
    sizes = np.diff(host["track_off"])
    del res, again

    pool, kp_pool, f_set_off, pairs = layout(dev)
    batch = M.match_pairs_device(pool, f_set_off, pairs, "mnn")
    match_rows = int(batch.read()[0].astype(np.int64).sum())

    def fundamental():
        _, info, _ = geometry.ransac_fundamental_pairs(kp_pool, batch, args.fundamental_iters,
                                                       4.0, 0)
        return info.cpu().numpy()

    calls = (("fundamental", fundamental), ("triangulate", lambda: triangulate()[0]))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    t = {key: ([], []) for key, _ in calls}
    for _ in range(args.reps):                          # alternate the calls
        for key, fn in calls:
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    ok = host["tinfo"][:, 0] == 0
    doc = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per call", "cameras": args.cameras, "keypoints_per_camera": NKP,
           "rows": int(set_off[-1]), "edges": int(edges.shape[0]), "planted_tracks": planted,
           "iters": args.iters, "thr": args.thr, "min_angle": args.min_angle,
           "max_track": args.max_track, "counts": [int(v) for v in counts],
           "track_length": stats(sizes) if len(sizes) else None,
           "tracks_longer_than_lane_kernel": int((sizes > 6).sum()),
           "mean_inliers_per_point": float(host["tinfo"][ok, 1].mean()) if ok.any() else 0.0,
           "mean_reprojection_error_px": float(host["err"][ok].mean()) if ok.any() else 0.0,
           "refit_kept": int(host["tinfo"][:, 3].sum()),
           "fundamental_pairs": int(pairs.shape[0]), "fundamental_iters": args.fundamental_iters,
           "fundamental_match_rows": match_rows}
    for key in t:
        doc[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    ev = doc["triangulate"]["event_ms"]["median"]
    fev = doc["fundamental"]["event_ms"]["median"]
    doc["edges_per_s"] = float(edges.shape[0]) / (ev * 1e-3)
    doc["tracks_per_s"] = float(T) / (ev * 1e-3)
    doc["ratio_to_fundamental_event"] = ev / fev
    doc["ratio_to_fundamental_wall"] = (doc["triangulate"]["wall_ms"]["median"] /
                                        doc["fundamental"]["wall_ms"]["median"])
    doc["ratio_to_fundamental_per_edge_and_match_row"] = (ev / edges.shape[0]) / (fev / match_rows)
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
