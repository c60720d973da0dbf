"""Times the batched five-point RANSAC essential-matrix stage
(geometry.ransac_essential_pairs, essential.hip) on the HPatches-shaped pair
list of tools/bench_ransac_pairs.py (100 pairs of 8192 x 128 sets, 30 % planted
correspondences) with one synthetic camera per set (f = 500, centre (320, 240),
no distortion), alternating in one process with the fundamental-matrix call.
The planted keypoints of that list follow homographies, so the inlier counts
say nothing about pose accuracy: the list is used because it is the one the
other geometry numbers were measured on.

Both calls get device tensors and end in the device-to-host read of ``info``.
Per call: the wall time (host clock, device idle before) and the HIP-event
time; median, min and max over --reps runs after --warmup untimed ones.  Also
the mean number of candidates per sample -- counted with the host solver
(geometry.solve5, the text the kernel compiles) on the first --probe samples of
the first --probe_pairs pairs, since the call does not return its record counts
-- and from it (candidate x match) Sampson tests per second = candidates per
sample x iters x matches / time, and the ratio to the fundamental call.  One
JSON document on stdout and in --out.

  python tools/bench_essential_pairs.py [--reps 7] [--warmup 2] [--iters 1024] [--out FILE]
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

CAM = (500.0, 500.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0)


def candidates_per_sample(kp, batch, set_off, pairs, npairs, nsamples):
    """the host solver on the samples the kernel draws (seed 0)"""
    counts, matches = batch.read()
    total, n = 0, 0
    for p in range(min(npairs, pairs.shape[0])):
        m = matches[batch.moff[p]:batch.moff[p] + counts[p]]
        if len(m) < 5:
            continue
        a, b = pairs[p]
        rows = np.concatenate([kp[set_off[a] + m[:, 0]], kp[set_off[b] + m[:, 1]]], 1).astype(np.float64)
        rows = (rows - [CAM[2], CAM[3], CAM[2], CAM[3]]) / CAM[0]
        for it in range(nsamples):
            idx = geometry.sample_indices(0, p, it, len(m), k=5)
            total += geometry.solve5(rows[idx]).shape[0]
            n += 1
    return total / max(n, 1), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--thr", type=float, default=4.0)
    ap.add_argument("--fundamental_iters", type=int, default=2048)
    ap.add_argument("--probe", type=int, default=256)
    ap.add_argument("--probe_pairs", type=int, default=8)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "essential_pairs",
                                                            "bench.json"))
    args = ap.parse_args()
    torch.manual_seed(1)
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    pool, kp_pool, set_off, pairs = layout(dev)
    batch = M.match_pairs_device(pool, set_off, pairs, "mnn")
    batch.read()
    nsets = set_off.shape[0] - 1
    cams = torch.tensor([CAM] * nsets, dtype=torch.float64, device=dev)

    def essential():
        _, _, info, _, _ = geometry.ransac_essential_pairs(kp_pool, cams, batch, args.iters,
                                                           args.thr, 0)
        return info.cpu().numpy()

    def fundamental():
        _, info, _ = geometry.ransac_fundamental_pairs(kp_pool, batch, args.fundamental_iters,
                                                       args.thr, 0)
        return info.cpu().numpy()

    info = essential()
    assert np.array_equal(info, essential()), "two calls on the same inputs differ"
    counts = batch.read()[0].astype(np.int64)
    calls = (("fundamental", fundamental), ("essential", essential))
    for _ in range(args.warmup):
        for _, fn in calls:
            fn()
    t = {key: ([], []) for key, _ in calls}
    for _ in range(args.reps):                          # alternate the calls
        for key, fn in calls:
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    cands, probed = candidates_per_sample(kp_pool.cpu().numpy(), batch, set_off, pairs,
                                          args.probe_pairs, args.probe)
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per pair list", "pairs": int(pairs.shape[0]), "iters": args.iters,
           "thr": args.thr, "fundamental_iters": args.fundamental_iters,
           "matches": int(counts.sum()), "matches_per_pair": stats(counts),
           "pairs_with_model": int(np.sum(info[:, 0] == 0)),
           "inliers_per_pair": stats(info[:, 1]), "refit_kept": int((info[:, 3] & 1).sum()),
           "candidates_per_sample": cands, "candidates_probed_samples": probed}
    for key in t:
        res[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    ev = res["essential"]["event_ms"]["median"]
    per_sample = float(args.iters) * float(counts.sum()) / (ev * 1e-3)
    res["sample_matches_per_s"] = per_sample
    res["candidate_matches_per_s"] = cands * per_sample
    res["ratio_to_fundamental_event"] = ev / res["fundamental"]["event_ms"]["median"]
    res["ratio_to_fundamental_per_iteration"] = (
        res["ratio_to_fundamental_event"] * args.fundamental_iters / args.iters)
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
