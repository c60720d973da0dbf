"""Times the query registration stage (geometry.ransac_pose_queries, pose.hip) on
a synthetic list shaped like Aachen's night queries, alternating in one process
with the batched RANSAC fundamental-matrix stage
(geometry.ransac_fundamental_pairs) on the pair list of
tools/bench_ransac_pairs.py.

The list: --queries (191) queries x --corr (8192) correspondences each; every
query has its own planted pose (K = 500 / 320 / 240, every second one
SIMPLE_RADIAL) and its own world points; --planted (0.3) of a query's
correspondences are projections of their points with 0.5 px noise, the rest
random pixels.  --iters (1024) iterations, thr = 12.

Every call gets device tensors and ends in its device-to-host read (``info``).
Per call: the wall time (host clock, device idle before) and the HIP-event
time; median, min and max over --reps runs after --warmup untimed ones.  Also
hypothesis-correspondence scores per second (iterations x the mean number of
candidates is not known on the host, so per sample: queries x iters x corr) and
the ratio to the fundamental call.  One JSON document on stdout and in --out.

  python tools/bench_pose_queries.py [--reps 7] [--warmup 2] [--queries 191] [--out FILE]
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


def random_rotations(rs, n):
    q = rs.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)],
                    1).reshape(n, 3, 3)


def scene(nq, ncorr, planted, rs):
    """(kp [nq ncorr, 2] fp32, cams, points, corr int32, q_off, planted poses [nq, 3, 4])"""
    cams = np.zeros((nq, 8))
    cams[:, :4] = (500.0, 500.0, 320.0, 240.0)
    cams[1::2, 4] = -0.06
    R, C = random_rotations(rs, nq), rs.uniform(-1, 1, (nq, 3))
    t = -np.einsum("qij,qj->qi", R, C)
    Xc = np.stack([rs.uniform(-0.6, 0.6, (nq, ncorr)), rs.uniform(-0.45, 0.45, (nq, ncorr)),
                   np.ones((nq, ncorr))], 2) * rs.uniform(3, 9, (nq, ncorr, 1))
    X = np.einsum("qji,qnj->qni", R, Xc - t[:, None, :])        # R^T (Xc - t)
    xn, yn = Xc[:, :, 0] / Xc[:, :, 2], Xc[:, :, 1] / Xc[:, :, 2]
    f = 1.0 + cams[:, None, 4] * (xn * xn + yn * yn)
    xy = np.stack([500.0 * f * xn + 320.0, 500.0 * f * yn + 240.0], 2)
    xy += rs.normal(0, 0.5, xy.shape)
    junk = rs.uniform(size=(nq, ncorr)) >= planted
    xy[junk] = np.stack([rs.uniform(0, 640, junk.sum()), rs.uniform(0, 480, junk.sum())], 1)
    n = nq * ncorr
    corr = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    q_off = (np.arange(nq + 1) * ncorr).astype(np.int32)
    return (xy.reshape(n, 2).astype(np.float32), cams, X.reshape(n, 3), corr, q_off,
            np.concatenate([R, t[:, :, None]], 2), ~junk)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--queries", type=int, default=191)
    ap.add_argument("--corr", type=int, default=8192)
    ap.add_argument("--planted", type=float, default=0.3)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--thr", type=float, default=12.0)
    ap.add_argument("--fundamental_iters", type=int, default=2048)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "pose_queries",
                                                            "bench.json"))
    args = ap.parse_args()
    torch.manual_seed(1)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    kp, cams, points, corr, q_off, planted, good = scene(args.queries, args.corr, args.planted,
                                                          np.random.RandomState(1))
    kp_d, cams_d, points_d, corr_d = (torch.from_numpy(a).to(dev) for a in (kp, cams, points, corr))

    def pose():
        res = geometry.ransac_pose_queries(kp_d, cams_d, points_d, corr_d, q_off, args.iters,
                                           args.thr, 0)
        return res[1].cpu().numpy(), res

    info, res = pose()
    again = pose()[1]
    for a, b in zip(res, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "two calls differ"
    poses = res[0].cpu().numpy().reshape(-1, 3, 4)
    mask = res[2].cpu().numpy().reshape(args.queries, args.corr) != 0
    rot_err = np.abs(poses[:, :, :3] - planted[:, :, :3]).max((1, 2))
    del res, again

    pool, kp_pool, f_set_off, pairs = layout(dev)
    batch = M.match_pairs_device(pool, f_set_off, pairs, "mnn")
    match_rows = int(batch.read()[0].astype(np.int64).sum())

    def fundamental():
        _, finfo, _ = geometry.ransac_fundamental_pairs(kp_pool, batch, args.fundamental_iters,
                                                        4.0, 0)
        return finfo.cpu().numpy()

    calls = (("fundamental", fundamental), ("pose", lambda: pose()[0]))
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
           "unit": "ms per call", "queries": args.queries, "correspondences_per_query": args.corr,
           "planted_share": args.planted, "iters": args.iters, "thr": args.thr,
           "solved": int((info[:, 0] == 0).sum()), "refit_kept": int((info[:, 3] & 1).sum()),
           "inliers": stats(info[:, 1]),
           "planted_recovered_share": float((mask & good).sum() / max(good.sum(), 1)),
           "junk_inlier_share": float((mask & ~good).sum() / max((~good).sum(), 1)),
           "rotation_error_max": float(rot_err.max()),
           "winning_root_histogram": np.bincount(info[:, 3] >> 8, minlength=4).tolist(),
           "fundamental_pairs": int(pairs.shape[0]), "fundamental_iters": args.fundamental_iters,
           "fundamental_match_rows": match_rows}
    for key in t:
        doc[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    ev = doc["pose"]["event_ms"]["median"]
    fev = doc["fundamental"]["event_ms"]["median"]
    doc["queries_per_s"] = float(args.queries) / (ev * 1e-3)
    doc["sample_correspondence_pairs_per_s"] = (float(args.queries) * args.iters * args.corr /
                                                (ev * 1e-3))
    doc["ratio_to_fundamental_event"] = ev / fev
    doc["ratio_to_fundamental_wall"] = (doc["pose"]["wall_ms"]["median"] /
                                        doc["fundamental"]["wall_ms"]["median"])
    text = json.dumps(doc, indent=1)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
