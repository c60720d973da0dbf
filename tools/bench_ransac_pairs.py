"""Times the batched RANSAC homography stage (geometry.ransac_homography_pairs,
ransac.hip) on the HPatches-shaped pair list of tools/bench_match_pairs.py,
and the matcher that feeds it (matchers.match_pairs_device) in the same
process:

  hpatches  20 sequences x 6 sets of 8192 x 128, image 1 against images 2..6:
            100 pairs; 30 % of the rows of images 2..6 are noisy copies of
            rows of image 1 whose keypoints follow a homography (the planted
            true correspondences), the rest is random.  The matches are
            whatever the mutual-nearest-neighbour matcher yields on them.

Both calls get device tensors and end in their device-to-host read (RANSAC:
``info``; matcher: counts and matches), so a timed call leaves its result on
the host.  Per call: the wall time (host clock, device idle before) and the
HIP-event time; median, min and max over --reps runs after --warmup untimed
ones, the two calls alternating.  Also: (hypotheses x matches) scored per
second and the ratio RANSAC / matcher.  One JSON document on stdout and in
--out.

  python tools/bench_ransac_pairs.py [--reps 7] [--warmup 2] [--iters 1024] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from posfeat_amd import geometry, matchers as M  # noqa: E402

N, SEQS, PLANTED = 8192, 20, 0.3
W, H = 640, 480


def _unit(d):
    return d / d.norm(dim=1, keepdim=True)


def layout(dev):
    """(descriptor pool, keypoint pool, set_off, pairs) of the list"""
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    size = torch.tensor([W, H], device=dev, dtype=torch.float32)
    descs, kps = [], []
    m = int(PLANTED * N)
    for s in range(SEQS):
        d1 = _unit(torch.randn(N, 128, device=dev, generator=g))
        k1 = torch.rand(N, 2, device=dev, generator=g) * size
        descs.append(d1)
        kps.append(k1)
        for k in range(1, 6):
            Hm = torch.eye(3, dtype=torch.float64)
            Hm += (torch.rand(3, 3, dtype=torch.float64) * 2 - 1) * torch.tensor(
                [[.05, .05, 20], [.05, .05, 20], [1e-4, 1e-4, 0]], dtype=torch.float64)
            Hm = Hm.to(dev)
            d = torch.randn(N, 128, device=dev, generator=g)
            kp = torch.rand(N, 2, device=dev, generator=g) * size
            src = torch.randperm(N, device=dev, generator=g)[:m]
            dst = torch.randperm(N, device=dev, generator=g)[:m]
            d[dst] = d1[src] + 0.05 * torch.randn(m, 128, device=dev, generator=g)
            ph = torch.cat([k1[src].double(), torch.ones(m, 1, device=dev, dtype=torch.float64)],
                           1) @ Hm.T
            kp[dst] = (ph[:, :2] / ph[:, 2:]).float() + 0.5 * torch.randn(m, 2, device=dev,
                                                                          generator=g)
            descs.append(_unit(d))
            kps.append(kp)
    set_off = (np.arange(6 * SEQS + 1) * N).astype(np.int32)
    pairs = np.asarray([(6 * s, 6 * s + k) for s in range(SEQS) for k in range(1, 6)], np.int32)
    return torch.cat(descs, 0), torch.cat(kps, 0).contiguous(), set_off, pairs


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1), out


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=1024)
    ap.add_argument("--thr", type=float, default=3.0)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "ransac_pairs",
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

    def ransac():
        _, info, _ = geometry.ransac_homography_pairs(kp_pool, batch, args.iters, args.thr, 0)
        return info.cpu().numpy()

    info = ransac()
    assert np.array_equal(info, ransac()), "two calls on the same inputs differ"
    counts = batch.read()[0].astype(np.int64)
    for _ in range(args.warmup):
        match()
        ransac()
    t = {"match_pairs": ([], []), "ransac": ([], [])}
    for _ in range(args.reps):                          # alternate the two calls
        for key, fn in (("match_pairs", match), ("ransac", ransac)):
            w, d, _ = timed(fn)
            t[key][0].append(w)
            t[key][1].append(d)
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per pair list", "pairs": int(pairs.shape[0]), "iters": args.iters,
           "thr": args.thr, "matches": int(counts.sum()),
           "matches_per_pair": stats(counts), "pairs_with_model": int(np.sum(info[:, 0] == 0)),
           "inliers_per_pair": stats(info[:, 1]), "refit_kept": int(info[:, 3].sum())}
    for key in t:
        res[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
    ev = res["ransac"]["event_ms"]["median"]
    res["hypothesis_matches_per_s"] = float(args.iters) * float(counts.sum()) / (ev * 1e-3)
    res["ratio_event"] = ev / res["match_pairs"]["event_ms"]["median"]
    res["ratio_wall"] = res["ransac"]["wall_ms"]["median"] / res["match_pairs"]["wall_ms"]["median"]
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")


if __name__ == "__main__":
    main()
