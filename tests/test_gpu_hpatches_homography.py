"""evaluation.hpatches.benchmark_homography and ``evaluate_hpatches.py
--homography`` on a tiny synthetic HPatches tree (2 sequences of six 160 x 120
PPM images, planted matches) against the numpy restatement
(tests/ransac_ref.py) driven over the same matches."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ransac_ref as R
from oracle import match_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSTFIX = "synth"
W, HT = 160, 120
ITERS, THR, SEED = 128, 3.0, 5
H_SCALE = np.array([[.04, .04, 6], [.04, .04, 6], [1e-4, 1e-4, 0]])


def _kp(rs, n):
    return (rs.uniform(0, 1, (n, 2)) * [W - 1, HT - 1]).astype(np.float32)


def _write_tree(root):
    """sequences i_synth and v_synth; returns (feats, data, {seq: (kps, descs, Hs)}).
    Image k of a sequence holds, for the matches the numpy matcher finds against
    image 1, the projection of the image-1 keypoint plus noise (a share of
    them displaced instead); image 4 of v_synth has 3 keypoints only."""
    feats, data = os.path.join(root, "feats"), os.path.join(root, "data")
    tree = {}
    for s, seq in enumerate(("i_synth", "v_synth")):
        rs = np.random.RandomState(160 + s)
        os.makedirs(os.path.join(feats, seq))
        os.makedirs(os.path.join(data, seq))
        n = [int(v) for v in rs.randint(150, 260, 6)]
        if seq == "v_synth":
            n[3] = 3
        kps, descs, Hs = [_kp(rs, n[0])], [None], []
        for k in range(1, 6):
            d1, d2 = mr.seeded_descriptors(170 + s, n[0], n[k])   # d1: the same rows for every k
            descs[0] = d1
            descs.append(d2)
            H = np.eye(3) + rs.uniform(-1, 1, (3, 3)) * H_SCALE
            kb = _kp(rs, n[k])
            m = mr.mnn_matcher(d1, d2)
            sigma = (0.3, 0.3, 1.5, 0.3, 3.0)[k - 1]
            tgt = R.warp(H, kps[0][m[:, 0]].astype(np.float64)) + sigma * rs.randn(len(m), 2)
            out = rs.uniform(0, 1, len(m)) < 0.3
            tgt[out] += rs.uniform(10, 60, (int(out.sum()), 2))
            kb[m[:, 1]] = tgt.astype(np.float32)
            kps.append(kb)
            np.savetxt(os.path.join(data, seq, "H_1_%d" % (k + 1)), H)
        for k in range(6):
            kp3 = np.concatenate([kps[k], np.ones((n[k], 1), np.float32)], 1)   # (x, y, scale)
            with open(os.path.join(feats, seq, "%d.ppm.%s" % (k + 1, POSTFIX)), "wb") as f:
                np.savez(f, keypoints=kp3, scores=rs.uniform(0, 1, n[k]).astype(np.float32),
                         descriptors=descs[k])
            with open(os.path.join(data, seq, "%d.ppm" % (k + 1)), "wb") as f:
                f.write(b"P6\n# synthetic\n%d %d\n255\n" % (W, HT))
                f.write(rs.randint(0, 256, (HT, W, 3)).astype(np.uint8).tobytes())
        Hs = [np.loadtxt(os.path.join(data, seq, "H_1_%d" % (k + 1))) for k in range(1, 6)]
        tree[seq] = (kps, descs, Hs)
    return feats, data, tree


def _restated(tree):
    """per pair, in the chunk's pair order: the restatement on the GPU matcher's
    matches, its corner error against H_1_k, and the closest residual to thr"""
    from posfeat_amd import matchers as M
    errs, types, margin = [], [], np.inf
    p = 0
    for seq in sorted(tree):
        kps, descs, Hs = tree[seq]
        for k in range(1, 6):
            m = M.mnn_matcher(descs[0], descs[k])
            rows = np.concatenate([kps[0][m[:, 0]], kps[k][m[:, 1]]], 1)
            r = R.ransac(rows, p, ITERS, THR, SEED)
            margin = min(margin, r["margin"])
            errs.append(R.corner_error(r["H"], Hs[k - 1], W, HT) if r["status"] == 0
                        else float("inf"))
            types.append(seq[0])
            p += 1
    return np.asarray(errs), np.asarray(types), margin


def _acc(errs, types, eps=(1, 3, 5)):
    out = {}
    for key, sel in (("all", np.ones(len(errs), bool)), ("i", types == "i"), ("v", types == "v")):
        out[key] = {e: float(np.mean(errs[sel] <= e)) for e in eps}
    return out


def _cli(args, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_hpatches.py")] + args,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_benchmark_homography_and_cli(gpu, tmp_path):
    from posfeat_amd.evaluation import hpatches as hp
    feats, data, tree = _write_tree(str(tmp_path))
    ref_err, ref_types, margin = _restated(tree)
    print("closest residual to thr in the restatement: %.3g px" % margin)
    assert margin > 1e-6
    errs, acc, types = hp.benchmark_homography(feats, data, POSTFIX, iters=ITERS, thr=THR,
                                               seed=SEED)
    print("corner errors (px):", np.array2string(errs, precision=4))
    assert errs.dtype == np.float64 and errs.shape == (10,)
    assert types.tolist() == ["i"] * 5 + ["v"] * 5 == ref_types.tolist()
    assert np.array_equal(np.isinf(errs), np.isinf(ref_err))
    fin = np.isfinite(ref_err)
    assert np.abs(errs[fin] - ref_err[fin]).max() <= 1e-6
    assert np.isinf(errs[5 + 2]) and fin.sum() == 9        # v_synth image 4: 3 keypoints, no model
    assert acc == _acc(ref_err, ref_types)
    assert acc["v"][5] <= 0.8 and acc["all"][5] > 0.0      # not vacuous
    assert acc["all"][1] <= acc["all"][3] <= acc["all"][5]
    # the command-line entry point: with the flag the rows follow the existing output ...
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    got = hp.benchmark_features(feats, data, POSTFIX)
    row = hp.format_row(POSTFIX, got[2], hp.mma_score(got[0], got[1], 1, 1))
    existing = "\n".join(hp.summary_lines(got[2])) + "\n" + row
    os.makedirs(str(tmp_path / "a"))
    os.makedirs(str(tmp_path / "b"))
    base = ["--features", feats, "--dataset", data, "--postfix", POSTFIX]
    out_h = _cli(base + ["--out", str(tmp_path / "a" / "synth"), "--homography", "--ransac_iters",
                         str(ITERS), "--ransac_thr", str(THR), "--seed", str(SEED)], env)
    assert out_h == existing + "\n".join(hp.homography_lines(acc)) + "\n"
    assert len(hp.homography_lines(acc)) == 3
    saved = np.load(str(tmp_path / "a" / "synth.homography.npy"))
    assert saved.tobytes() == errs.tobytes()               # deterministic
    # ... and without it stdout and files are what the existing code path gives
    out_0 = _cli(base + ["--out", str(tmp_path / "b" / "synth")], env)
    assert out_0 == existing
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["synth.npy", "synth.txt"]
    assert sorted(os.listdir(str(tmp_path / "a"))) == ["synth.homography.npy", "synth.npy",
                                                       "synth.txt"]
    with open(str(tmp_path / "a" / "synth.txt")) as fa, open(str(tmp_path / "b" / "synth.txt")) as fb:
        assert fa.read() == fb.read() == row
