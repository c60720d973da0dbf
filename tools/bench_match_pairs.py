"""Times the batched pair-list matcher (matchers.match_pairs, matchpairs.hip)
against a loop over the per-pair mnn_matcher (match.hip) on two pair lists:

  hpatches  20 sequences x 6 sets of 8192 x 128, image 1 against images 2..6:
            100 pairs (configs/extract_hpatches.yaml num_pts)
  aachen    50 pairs of 20480 x 7000 over 10 + 10 sets (the ragged Aachen shape
            of tests/test_gpu_matchers.py)

Both paths get the same device tensors and return host arrays, so each timed
call ends in its device-to-host read.  Per layout and path: the wall time of
one whole list (host clock, device idle before, the result on the host after)
and the HIP-event time between the first and the last device operation of the
call; median, min and max over --reps runs after --warmup untimed ones, the two
paths alternating.  The outputs are compared (they must be identical) before
anything is timed.  One JSON document on stdout and in --out.

  python tools/bench_match_pairs.py [--reps 7] [--warmup 2] [--out FILE]
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

from posfeat_amd import matchers as M  # noqa: E402


def _sets(sizes, seed, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    out = []
    for n in sizes:
        d = torch.randn(n, 128, device=dev, generator=g)
        out.append(d / d.norm(dim=1, keepdim=True))
    # every other set holds noisy copies of rows of the set before it
    for k in range(1, len(out)):
        m = min(out[k].shape[0], out[k - 1].shape[0]) // 2
        d = out[k].clone()
        d[:m] = out[k - 1][:m] + 0.05 * torch.randn(m, 128, device=dev, generator=g)
        out[k] = d / d.norm(dim=1, keepdim=True)
    return out


def layouts(dev):
    hp_sets = _sets([8192] * 120, 1, dev)
    hp_pairs = [(6 * s, 6 * s + k) for s in range(20) for k in range(1, 6)]
    aa_sets = _sets([20480] * 10 + [7000] * 10, 2, dev)
    aa_pairs = [(p % 10, 10 + (p // 10 + p) % 10) for p in range(50)]
    return {"hpatches": (hp_sets, hp_pairs), "aachen": (aa_sets, aa_pairs)}


def per_pair(sets, pairs):
    return [M.mnn_matcher(sets[i], sets[j]) for i, j in pairs]


def batched(sets, pairs):
    return M.match_pairs(sets, pairs)


def timed(fn, sets, pairs):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn(sets, pairs)
    e1.record()
    e1.synchronize()
    return (time.perf_counter() - t0) * 1e3, e0.elapsed_time(e1)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "match_pairs",
                                                            "bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"device": torch.cuda.get_device_name(dev), "reps": args.reps, "warmup": args.warmup,
           "unit": "ms per pair list", "layouts": {}}
    for name, (sets, pairs) in layouts(dev).items():
        a, b = per_pair(sets, pairs), batched(sets, pairs)
        same = all(np.array_equal(x, y) for x, y in zip(a, b))
        for _ in range(args.warmup):
            per_pair(sets, pairs)
            batched(sets, pairs)
        t = {"per_pair": ([], []), "batched": ([], [])}
        for _ in range(args.reps):                      # alternate the two paths
            for key, fn in (("per_pair", per_pair), ("batched", batched)):
                w, d = timed(fn, sets, pairs)
                t[key][0].append(w)
                t[key][1].append(d)
        n1 = [sets[i].shape[0] for i, _ in pairs]
        n2 = [sets[j].shape[0] for _, j in pairs]
        flop = float(sum(2 * 2 * 128 * a_ * b_ for a_, b_ in zip(n1, n2)))   # both sides
        r = {"pairs": len(pairs), "matches": int(sum(len(x) for x in b)),
             "outputs_identical": bool(same), "mfma_gflop": flop / 1e9}
        for key in t:
            r[key] = {"wall_ms": stats(t[key][0]), "event_ms": stats(t[key][1])}
        r["wall_speedup"] = r["per_pair"]["wall_ms"]["median"] / r["batched"]["wall_ms"]["median"]
        r["event_speedup"] = (r["per_pair"]["event_ms"]["median"] /
                              r["batched"]["event_ms"]["median"])
        r["batched_tflops_event"] = flop / (r["batched"]["event_ms"]["median"] * 1e-3) / 1e12
        res["layouts"][name] = r
        del sets
        torch.cuda.empty_cache()
    doc = json.dumps(res, indent=1)
    print(doc)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(doc + "\n")
    if not all(r["outputs_identical"] for r in res["layouts"].values()):
        sys.exit("batched and per-pair outputs differ")


if __name__ == "__main__":
    main()
