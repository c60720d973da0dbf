"""posfeat_reproj_hist and posfeat_amd.evaluation.hpatches on the GPU against a
float64 numpy restatement of evaluations/hpatches/evaluation.py:71-90, and
evaluate_hpatches.py end to end on a synthetic tree."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import match_ref as mr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NTHR = 15
H_SCALE = np.array([[.05, .05, 20], [.05, .05, 20], [1e-4, 1e-4, 0]])


def _homography(rs):
    return np.eye(3) + rs.uniform(-1, 1, (3, 3)) * H_SCALE


def _proj(H, xy):
    """evaluation.py:71-74"""
    pos_a_h = np.concatenate([xy, np.ones([xy.shape[0], 1])], axis=1)
    pos_b_proj_h = np.transpose(np.dot(H, np.transpose(pos_a_h)))
    return pos_b_proj_h[:, :2] / pos_b_proj_h[:, 2:]


def _dist(H, kp_a, kp_b, matches):
    """evaluation.py:71-78 (fp32 keypoints, fp64 arithmetic)"""
    pos_b_proj = _proj(H, kp_a[matches[:, 0], :2])
    pos_b = kp_b[matches[:, 1], :2]
    return np.sqrt(np.sum((pos_b - pos_b_proj) ** 2, axis=1))


def _keypoints(rs, n):
    return (rs.uniform(0, 1, (n, 2)) * [640, 480]).astype(np.float32)


def _noisy_targets(rs, H, ka, kb, ia, ib):
    """kb[ib] = proj(ka[ia]) + sigma N(0, 1), sigma ~ U(0, 8) per match"""
    sigma = rs.uniform(0, 8, (len(ia), 1))
    kb[ib] = (_proj(H, ka[ia]) + sigma * rs.randn(len(ia), 2)).astype(np.float32)


REPROJ_CASES = [(31, 300, 257, 200), (32, 1000, 1200, 700), (33, 2049, 64, 33),
                (34, 5000, 5000, 4096)]


def test_reproj_hist_vs_numpy(gpu):
    from posfeat_amd import matchers as M
    from posfeat_amd.evaluation import hpatches as hp
    kps, Hs, ms, pairs = [], [], [], []
    for seed, n_a, n_b, m in REPROJ_CASES:
        rs = np.random.RandomState(seed)
        ka, kb = _keypoints(rs, n_a), _keypoints(rs, n_b)
        H = _homography(rs)
        ia, ib = rs.permutation(n_a)[:m], rs.permutation(n_b)[:m]   # m random index pairs
        _noisy_targets(rs, H, ka, kb, ia, ib)
        pairs.append((len(kps), len(kps) + 1))
        kps += [ka, kb]
        Hs.append(H)
        ms.append(np.stack([ia, ib], 1))
    # a pair without matches (counts = 0) between the others; its rows hold garbage
    pairs.insert(2, (0, 3))
    Hs.insert(2, _homography(np.random.RandomState(35)))
    ms.insert(2, np.zeros((0, 2), np.int64))
    # the reference histograms, and the margin that makes exact equality fair:
    # no distance within 1e-9 of an integer threshold
    ref = np.zeros((len(pairs), NTHR), np.int64)
    margin = np.inf
    for p, ((a, b), H, m) in enumerate(zip(pairs, Hs, ms)):
        dist = _dist(H, kps[a], kps[b], m)
        if dist.shape[0] == 0:
            dist = np.array([float("inf")])
        for thr in range(1, NTHR + 1):
            ref[p, thr - 1] = np.sum(dist <= thr)
            margin = min(margin, np.min(np.abs(dist - thr)))
    print("closest distance to a threshold: %.3g" % margin)
    assert margin > 1e-9
    # the device buffers as posfeat_match_pairs leaves them: pair p's rows at moff[p]
    sizes = [k.shape[0] for k in kps]
    set_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pairs_np = np.asarray(pairs, np.int32)
    n1 = np.asarray([sizes[a] for a, _ in pairs])
    moff = np.concatenate([[0], np.cumsum(n1)])
    matches = np.full((moff[-1], 2), -1, np.int32)
    counts = np.zeros(len(pairs), np.int32)
    for p, m in enumerate(ms):
        matches[moff[p]:moff[p] + len(m)] = m
        counts[p] = len(m)
    buf = torch.from_numpy(np.concatenate([counts, matches.reshape(-1)])).to(gpu)
    batch = M.PairBatch(None, set_off, pairs_np, moff, buf)
    kp_pool = torch.from_numpy(np.concatenate(kps, 0)).to(gpu)
    Hd = torch.from_numpy(np.stack([h.reshape(9) for h in Hs])).to(gpu)
    assert Hd.dtype == torch.float64
    hist = hp.reproj_hist(kp_pool, batch, Hd, NTHR).cpu().numpy()
    assert hist.dtype == np.int32 and hist.shape == (len(pairs), NTHR)
    np.testing.assert_array_equal(hist, ref)
    assert not hist[2].any()                               # the empty pair
    frac = ref[[0, 1, 3, 4]].sum(0) / counts.sum()
    assert frac[0] < 0.2 and frac[-1] > 0.9                # the thresholds discriminate
    # other threshold counts are prefixes / extensions of the same cumulative counts
    h32 = hp.reproj_hist(kp_pool, batch, Hd, 32).cpu().numpy()
    np.testing.assert_array_equal(h32[:, :NTHR], ref)
    np.testing.assert_array_equal(hp.reproj_hist(kp_pool, batch, Hd, 1).cpu().numpy(), ref[:, :1])
    # a non-finite projection counts nowhere
    Hbad = Hd.clone()
    Hbad[0] = 0.0                                          # 0 / 0 for every match of pair 0
    hb = hp.reproj_hist(kp_pool, batch, Hbad, NTHR).cpu().numpy()
    assert not hb[0].any()
    np.testing.assert_array_equal(hb[1:], ref[1:])


# ---- benchmark_features / evaluate_hpatches.py on a synthetic tree -----------

POSTFIX = "synth"


def _write_tree(root):
    """sequences i_synth and v_synth: six npz files each (200..700 keypoints)
    and the H_1_k files; returns {seq: ([kp], [desc], [scores], [H])}"""
    feats, data = os.path.join(root, "feats"), os.path.join(root, "data")
    tree = {}
    for s, seq in enumerate(("i_synth", "v_synth")):
        rs = np.random.RandomState(60 + s)
        os.makedirs(os.path.join(feats, seq))
        os.makedirs(os.path.join(data, seq))
        n = [int(v) for v in rs.randint(200, 701, 6)]
        kps, descs, scores, Hs = [_keypoints(rs, n[0])], [None], [], []
        for k in range(1, 6):
            d1, d2 = mr.seeded_descriptors(70 + s, n[0], n[k])   # d1: the same rows for every k
            descs[0] = d1
            descs.append(d2)
            H = _homography(rs)
            kb = _keypoints(rs, n[k])
            m = mr.mnn_matcher(d1, d2)                           # the numpy oracle's matches
            _noisy_targets(rs, H, kps[0], kb, m[:, 0], m[:, 1])
            kps.append(kb)
            Hs.append(H)
            np.savetxt(os.path.join(data, seq, "H_1_%d" % (k + 1)), H)
        for k in range(6):
            scores.append(rs.uniform(0, 1, n[k]).astype(np.float32))
            kp3 = np.concatenate([kps[k], np.ones((n[k], 1), np.float32)], 1)   # (x, y, scale)
            with open(os.path.join(feats, seq, "%d.ppm.%s" % (k + 1, POSTFIX)), "wb") as f:
                np.savez(f, keypoints=kp3, scores=scores[k], descriptors=descs[k])
        # loadtxt reads back what savetxt wrote (%.18e: exact for fp64)
        Hs = [np.loadtxt(os.path.join(data, seq, "H_1_%d" % (k + 1))) for k in range(1, 6)]
        tree[seq] = (kps, descs, scores, Hs)
    return feats, data, tree


def _restated(tree, top_k=None, max_kp=60000):
    """evaluation.py:40-96 with the per-pair GPU matcher and numpy reprojection"""
    from posfeat_amd import matchers as M
    rng = np.arange(1, 16)
    i_err = {thr: 0 for thr in rng}
    v_err = {thr: 0 for thr in rng}
    n_feats, n_matches, seq_type = [], [], []

    def read(seq, k):
        kps, descs, scores, _ = tree[seq]
        kp, d = kps[k], descs[k]
        if top_k is not None:
            ids = np.argsort(scores[k])[-top_k:]
            kp, d = kp[ids, :], d[ids, :]
        return kp[:max_kp], d[:max_kp]

    for seq in sorted(tree):
        keypoints_a, descriptors_a = read(seq, 0)
        n_feats.append(keypoints_a.shape[0])
        for k in range(1, 6):
            keypoints_b, descriptors_b = read(seq, k)
            n_feats.append(keypoints_b.shape[0])
            matches = M.mnn_matcher(descriptors_a, descriptors_b)
            dist = _dist(tree[seq][3][k - 1], keypoints_a, keypoints_b, matches)
            n_matches.append(matches.shape[0])
            seq_type.append(seq[0])
            if dist.shape[0] == 0:
                dist = np.array([float("inf")])
            for thr in rng:
                if seq[0] == "i":
                    i_err[thr] += np.mean(dist <= thr)
                else:
                    v_err[thr] += np.mean(dist <= thr)
    return i_err, v_err, [np.array(seq_type), np.array(n_feats), np.array(n_matches)]


def _assert_same(got, ref):
    for g, r in zip(got[:2], ref[:2]):
        assert sorted(g) == list(range(1, 16))
        for thr in range(1, 16):
            assert abs(g[thr] - r[thr]) <= 1e-12, (thr, g[thr], r[thr])
    for g, r in zip(got[2], ref[2]):
        assert np.array_equal(g, r)


def test_benchmark_features_and_cli(gpu, tmp_path):
    from posfeat_amd.evaluation import hpatches as hp
    feats, data, tree = _write_tree(str(tmp_path))
    got = hp.benchmark_features(feats, data, POSTFIX)                  # both sequences: one chunk
    ref = _restated(tree)
    _assert_same(got, ref)
    assert got[2][0].tolist() == ["i"] * 5 + ["v"] * 5 and len(got[2][1]) == 12
    assert 1.0 < got[0][10] <= 5.0 and 1.0 < got[1][10] <= 5.0        # not vacuous
    assert got[0][1] < got[0][15]
    # top_k = 150, one sequence per chunk
    got_k = hp.benchmark_features(feats, data, POSTFIX, top_k=150, pool_bytes=1)
    _assert_same(got_k, _restated(tree, top_k=150))
    assert set(got_k[2][1].tolist()) == {150}
    # the row cut (the reference's 60000) at a size the tree reaches
    _assert_same(hp.benchmark_features(feats, data, POSTFIX, max_kp=230),
                 _restated(tree, max_kp=230))
    # the command-line entry point on the same tree
    prefix = str(tmp_path / "out" / "synth")
    os.makedirs(os.path.dirname(prefix))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate_hpatches.py"), "--features",
                        feats, "--dataset", data, "--postfix", POSTFIX, "--out", prefix],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    saved = np.load(prefix + ".npy", allow_pickle=True)
    assert saved.shape == (3,)
    _assert_same((saved[0], saved[1], saved[2]), got)
    for thr in range(1, 16):                                           # deterministic
        assert saved[0][thr] == got[0][thr] and saved[1][thr] == got[1][thr]
    row = hp.format_row(POSTFIX, got[2], hp.mma_score(got[0], got[1], 1, 1))
    lines = r.stdout.splitlines()
    assert lines[-3:-1] == hp.summary_lines(got[2])
    assert lines[-1] + "\n" == row
    with open(prefix + ".txt") as f:
        assert f.read() == row
    assert row.startswith(POSTFIX.ljust(25) + " & ") and row.count("&") == 5
