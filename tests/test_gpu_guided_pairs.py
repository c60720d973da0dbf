"""posfeat_amd.matchers.match_pairs_guided_device (posfeat_match_pairs_guided,
matchpairs.hip) against its numpy restatement (tests/guided_ref.py).

The sets have the sizes [0, 1, 2, 31, 64, 65, 129, 300]: below, at and above
the 32-row MFMA block, the 64-row LDS step and the 128-column tile.  With 20
pairs the plan (match_plan.h, reused as is) cuts the streamed rows into ranges
of 64: every side that streams 129 or 300 rows is split (3 and 5 ranges), and
so is one that streams 65 rows (2 ranges: one full step and one row); the sides
over 0..64 rows are not.  test_plan_splits asserts this through
posfeat_match_pairs_splits.  The list shares sets, has a set on both sides, one
pair in both orders, the empty set on either side and a pair whose model is
zero.

Exact test: descriptor entries are k / 32 with integer |k| <= 3, so every
partial sum of a similarity is a multiple of 2^-10 below 2 and exact in fp32 in
any order: the restatement's float32 similarities are the kernel's, and the
records and the predicate are rounded once per operation on both sides, so
counts and matches must be equal with no tolerance."""
import ctypes
import os

import numpy as np
import pytest
import torch

import guided_ref as GR
from oracle import match_ref as mr

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 31, 64, 65, 129, 300]
PAIRS = ([(1, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 1)] +     # every size on each side
         [(7, 3), (7, 4), (7, 5), (7, 6)] +                            # set 7 shared; (6, 7) reversed
         [(7, 7), (6, 6), (4, 4), (1, 1)] +                            # a set on both sides
         [(0, 7), (7, 0), (0, 0)] +                                    # the empty set
         [(5, 7), (3, 6)])
ZERO = PAIRS.index((5, 7))                                             # this pair's model is zero
THR = 4.0
NG = 200
CASES = [("mnn", 0.95), ("ratio", 0.95), ("mnn_ratio", 0.95), ("ratio", 0.8), ("mnn_ratio", 0.8)]
_CACHE = {}


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


def _scene():
    """The exact fixture: per set keypoints [n, 2] float32 and descriptors
    [n, 128] float32 with entries k / 32, per pair F and H.  One plane of NG
    3-D points seen by a camera per set (so a homography and a fundamental
    matrix both hold).  A set of n rows holds, in shuffled order: ceil(0.55 n)
    projections (+- 0.5 px) of points 0.. whose descriptors are the point's
    base descriptor with three entries redrawn; n // 8 twins (a second
    detection of a point, same descriptor: arg-max ties); n // 8 decoys (the
    base descriptor itself, more similar than any true partner, at a random
    place: the unguided nearest neighbour, inadmissible); junk."""
    if "scene" in _CACHE:
        return _CACHE["scene"]
    rs = np.random.RandomState(2024)
    K, Ki = GR.K_CAM, np.linalg.inv(GR.K_CAM)
    nw, dw = np.array([-0.15, 0.1, 1.0]), 8.0            # the plane nw . X = dw
    xy = np.stack([rs.uniform(-3, 3, NG), rs.uniform(-2.2, 2.2, NG)], 1)
    X = np.concatenate([xy, (dw + 0.15 * xy[:, :1] - 0.1 * xy[:, 1:])], 1)
    vals = np.arange(-3, 4)
    prob = np.array([0.3, 0.15, 0.05, 0.0, 0.05, 0.15, 0.3])

    def draw(*shape):
        return (rs.choice(vals, size=shape, p=prob) / 32.0).astype(np.float32)

    base = draw(NG, 128)
    poses, kps, descs = [], [], []
    for n in SIZES:
        R = GR.rot(rs.uniform(-0.06, 0.06, 3))
        t = rs.uniform(-0.6, 0.6, 3) * [1, 1, 0.3]
        poses.append((R, t))
        ntrue, ntwin, ndec = int(np.ceil(0.55 * n)), n // 8, n // 8
        q = (K @ (R @ X.T + t[:, None])).T
        proj = q[:, :2] / q[:, 2:3]
        kp = np.stack([rs.uniform(0, GR.W, n), rs.uniform(0, GR.HGT, n)], 1)
        d = draw(n, 128)
        for g in range(ntrue):
            kp[g] = proj[g] + rs.uniform(-0.5, 0.5, 2)
            d[g] = base[g]
            d[g, rs.choice(128, 3, replace=False)] = draw(3)
        for k in range(ntwin):
            kp[ntrue + k] = proj[k] + rs.uniform(-0.5, 0.5, 2)
            d[ntrue + k] = d[k]
        for k in range(ndec):
            d[ntrue + ntwin + k] = base[ntwin + k]
        perm = rs.permutation(n)
        kps.append(kp[perm].astype(np.float32))
        descs.append(np.ascontiguousarray(d[perm]))
    Fs, Hs = np.zeros((len(PAIRS), 3, 3)), np.zeros((len(PAIRS), 3, 3))
    for p, (a, b) in enumerate(PAIRS):
        if p == ZERO:
            continue
        (Ra, ta), (Rb, tb) = poses[a], poses[b]
        R = Rb @ Ra.T
        t = tb - R @ ta
        if a == b:                       # F of a fake sideways motion: x^T [t]x x = 0, so
            t = np.array([1.0, 0.2, 0.1])    # a point is admissible for itself
        F = Ki.T @ _skew(t) @ R @ Ki
        Fs[p] = F / np.sqrt((F ** 2).sum())
        na = Ra @ nw
        Hs[p] = np.eye(3) if a == b else K @ (R + np.outer(tb - R @ ta, na) / (dw + na @ ta)) @ Ki
    _CACHE["scene"] = (kps, descs, Fs, Hs)
    return _CACHE["scene"]


def _reference(model):
    """per pair the masks and the masked top-2 of both sides, computed once"""
    key = ("ref", model)
    if key not in _CACHE:
        kps, descs, Fs, Hs = _scene()
        Ms = Fs if model == 1 else Hs
        out = []
        for p, (a, b) in enumerate(PAIRS):
            if SIZES[a] == 0 or SIZES[b] == 0:
                out.append(None)
                continue
            sim = descs[a] @ descs[b].T
            assert sim.dtype == np.float32
            okr, okc = GR.pair_masks(model, Ms[p], kps[a], kps[b], THR)
            out.append((sim, okr, okc, GR.masked_top2(sim.T, okr), GR.masked_top2(sim, okc)))
        _CACHE[key] = out
    return _CACHE[key]


def _expected(model, matcher, ratio):
    out = []
    for r in _reference(model):
        if r is None:
            out.append(np.zeros((0, 2), np.int64))
        else:
            out.append(GR.select(*r[3], *r[4], GR.MODES[matcher], ratio))
    return out


def _device(gpu, sets, kps):
    from posfeat_amd import matchers
    pool, set_off = matchers._pool(sets)
    kp_pool = torch.from_numpy(np.concatenate(kps, 0).astype(np.float32)).to(gpu)
    return pool, kp_pool, set_off


def _run(gpu, sets, kps, pairs, model, Ms, thr, matcher, ratio):
    from posfeat_amd import matchers
    pool, kp_pool, set_off = _device(gpu, sets, kps)
    M = torch.from_numpy(np.ascontiguousarray(Ms, dtype=np.float64)).to(gpu)
    batch = matchers.match_pairs_guided_device(pool, kp_pool, set_off,
                                               np.asarray(pairs, np.int32), model, M, thr, matcher,
                                               ratio)
    counts, matches = batch.read()
    return [matches[batch.moff[p]:batch.moff[p] + counts[p]].astype(np.int64)
            for p in range(len(pairs))]


def test_plan_splits_and_fixture():
    """CPU only: the plan the list gets, and what the exact fixture exercises"""
    from posfeat_amd import _lib
    set_off = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    pairs = np.asarray(PAIRS, np.int32)
    ns = np.zeros(2 * len(PAIRS), np.int32)
    assert _lib.lib().posfeat_match_pairs_splits(
        ctypes.c_void_p(set_off.ctypes.data), len(SIZES), ctypes.c_void_p(pairs.ctypes.data),
        len(PAIRS), ctypes.c_void_p(ns.ctypes.data)) == 0
    want = {1: 1, 2: 1, 31: 1, 64: 1, 65: 2, 129: 3, 300: 5}
    for p, (i, j) in enumerate(PAIRS):
        if SIZES[i] == 0 or SIZES[j] == 0:
            assert (ns[2 * p], ns[2 * p + 1]) == (0, 0)
        else:   # side 2p streams the rows of set j, side 2p + 1 those of set i
            assert (ns[2 * p], ns[2 * p + 1]) == (want[SIZES[j]], want[SIZES[i]]), (p, i, j)
    streamed = np.asarray([[SIZES[j], SIZES[i]] for i, j in PAIRS]).reshape(-1)
    live = np.repeat([SIZES[i] > 0 and SIZES[j] > 0 for i, j in PAIRS], 2)
    assert (ns[live & (streamed >= 129)] > 1).all() and (ns[live & (streamed <= 64)] == 1).all()
    kps, descs, Fs, Hs = _scene()
    assert max(float((d.astype(np.float64) ** 2).sum(1).max()) for d in descs if len(d)) <= 1.0
    for model in (0, 1):
        ref = _reference(model)
        rows = ties = none = one = rescued = 0
        for r in ref:
            if r is None:
                continue
            sim, okr, okc = r[:3]
            for s, ok, (nn, v1, v2) in ((sim.T, okr, r[3]), (sim, okc, r[4])):
                rows += len(nn)
                ties += int(((v1 == v2) & (v1 > -np.inf)).sum())
                nadm = ok.sum(0)
                none += int((nadm == 0).sum())
                one += int((nadm == 1).sum())
                unguided = np.argmax(s, 0)
                rescued += int(((nadm > 0) & ~ok[unguided, np.arange(len(nn))]).sum())
            assert (sim <= 1).all()
        print("model %d: %d rows, %d top-2 ties, %d without and %d with one admissible "
              "candidate, %d whose unguided neighbour is inadmissible" %
              (model, rows, ties, none, one, rescued))
        assert ties > 0 and none > 0 and one > 0 and rescued > 0
        assert ref[ZERO] is not None and not ref[ZERO][1].any() and not ref[ZERO][2].any()
        for matcher, ratio in CASES:
            exp = _expected(model, matcher, ratio)
            assert sum(len(m) for m in exp) > 50 and len(exp[ZERO]) == 0, (model, matcher, ratio)
            # not "match, then filter": some expected match is not the unguided neighbour's
            if matcher == "mnn":
                diff = 0
                for r, m in zip(ref, exp):
                    if r is not None and len(m):
                        diff += int((np.argmax(r[0], 1)[m[:, 0]] != m[:, 1]).sum())
                assert diff > 0


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("matcher,ratio", CASES)
def test_exact_descriptors_equal_restatement(gpu, model, matcher, ratio):
    kps, descs, Fs, Hs = _scene()
    got = _run(gpu, descs, kps, PAIRS, model, Fs if model == 1 else Hs, THR, matcher, ratio)
    exp = _expected(model, matcher, ratio)
    for p, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape and np.array_equal(g, e), (p, PAIRS[p], len(g), len(e))


def _seeded_sets():
    if "seeded" not in _CACHE:
        sets = [np.zeros((0, 128), np.float32)]
        sets += list(mr.seeded_descriptors(50, 1, 2))
        sets += list(mr.seeded_descriptors(51, 31, 64))
        sets += list(mr.seeded_descriptors(52, 65, 129))
        sets.append(mr.seeded_descriptors(53, 300, 300)[0])
        assert [len(s) for s in sets] == SIZES
        _CACHE["seeded"] = sets
    return _CACHE["seeded"]


@pytest.mark.parametrize("matcher", ["mnn", "ratio", "mnn_ratio"])
def test_huge_threshold_equals_unguided(gpu, matcher):
    """thr = 1e15 admits every candidate of a non-zero model, so the output is
    match_pairs_device's bit for bit (counts and every written row)"""
    from posfeat_amd import matchers
    kps, _, Fs, _ = _scene()
    sets = _seeded_sets()
    Fn = Fs.copy()
    Fn[ZERO] = Fs[0]
    pool, kp_pool, set_off = _device(gpu, sets, kps)
    pairs = np.asarray(PAIRS, np.int32)
    base = matchers.match_pairs_device(pool, set_off, pairs, matcher, 0.95)
    bc, bm = (x.copy() for x in base.read())
    assert bc.sum() > 100
    for model, Ms in ((1, Fn), (0, np.tile(np.eye(3), (len(PAIRS), 1, 1)))):
        M = torch.from_numpy(Ms).to(gpu)
        g = matchers.match_pairs_guided_device(pool, kp_pool, set_off, pairs, model, M, 1e15,
                                               matcher, 0.95)
        gc, gm = g.read()
        assert np.array_equal(gc, bc), model
        for p in range(len(PAIRS)):
            rows = slice(int(base.moff[p]), int(base.moff[p]) + int(bc[p]))
            assert gm[rows].tobytes() == bm[rows].tobytes(), (model, p)


def _random_scene():
    """random unit descriptors with planted partners on real geometry: sets
    (2049, 1000) and (300, 129) under F, (300, 300) under H"""
    if "random" in _CACHE:
        return _CACHE["random"]
    rs = np.random.RandomState(77)

    def unit(n):
        d = rs.randn(n, 128)
        return d / np.linalg.norm(d, axis=1, keepdims=True)

    def planted(n1, n2, k, view):
        a, b, M = view(rs, k)
        kp1 = np.stack([rs.uniform(0, GR.W, n1), rs.uniform(0, GR.HGT, n1)], 1).astype(np.float32)
        kp2 = np.stack([rs.uniform(0, GR.W, n2), rs.uniform(0, GR.HGT, n2)], 1).astype(np.float32)
        d1, d2 = unit(n1), unit(n2)
        src, dst = rs.permutation(n1)[:k], rs.permutation(n2)[:k]
        kp1[src], kp2[dst] = a, b
        d2[dst] = d1[src] + 0.05 * rs.randn(k, 128)
        d2 /= np.linalg.norm(d2, axis=1, keepdims=True)
        return (d1.astype(np.float32), d2.astype(np.float32)), (kp1, kp2), M

    (s0, s1), (k0, k1), F01 = planted(2049, 1000, 600, GR.two_view)
    (s2, s3), (k2, k3), F23 = planted(300, 129, 80, GR.two_view)
    (s4, s5), (k4, k5), H45 = planted(300, 300, 150, GR.plane_view)
    sets, kps = [s0, s1, s2, s3, s4, s5], [k0, k1, k2, k3, k4, k5]
    lists = {1: ([(0, 1), (1, 0), (2, 3)], np.stack([F01, F01.T, F23])),
             0: ([(4, 5), (5, 4)], np.stack([H45, np.linalg.inv(H45)]))}
    _CACHE["random"] = (sets, kps, lists)
    return _CACHE["random"]


@pytest.mark.parametrize("model", [0, 1])
def test_random_descriptors_against_fp64(gpu, model):
    """value check: margin m = 2 * 128 * 2^-24 on a similarity of unit vectors
    (a K = 128 fp32 chain of products below 1 is within 128 * 2^-24 of the fp64
    value; two such values are compared)"""
    m = 2 * 128 * 2.0 ** -24
    sets, kps, lists = _random_scene()
    pairs, Ms = lists[model]
    got = _run(gpu, sets, kps, pairs, model, Ms, THR, "mnn", 0.95)
    nrows = undecided = 0
    for p, (a, b) in enumerate(pairs):
        sim = sets[a].astype(np.float64) @ sets[b].astype(np.float64).T
        okr, okc = GR.pair_masks(model, Ms[p], kps[a], kps[b], THR)
        nn12, r1a, r1b = GR.masked_top2(sim.T, okr)
        nn21, r2a, r2b = GR.masked_top2(sim, okc)
        for v1, v2 in ((r1a, r1b), (r2a, r2b)):
            nrows += len(v1)
            has = v1 > -np.inf
            undecided += int((v1[has] - v2[has] <= m).sum())
        g = got[p]
        assert len(g) > 40, p
        i, j = g[:, 0], g[:, 1]
        assert okr[j, i].all() and okc[i, j].all(), p              # admissible, exactly
        assert (sim[i, j] >= r1a[i] - m).all() and (sim[i, j] >= r2a[j] - m).all(), p
        # every mutual admissible arg-max that is clear of the margin on both sides is output
        rows = np.nonzero(r1a > -np.inf)[0]
        jj = nn12[rows]
        clear = (nn21[jj] == rows) & (r1a[rows] - r1b[rows] > m) & (r2a[jj] - r2b[jj] > m)
        want = set(zip(rows[clear].tolist(), jj[clear].tolist()))
        assert want <= set(map(tuple, g.tolist())), p
        assert len(want) > 0.4 * len(g)
    print("model %d: %d of %d rows undecided within %.3g" % (model, undecided, nrows, m))
    assert undecided <= 0.02 * nrows


def test_sub_list_gives_the_same_rows(gpu):
    kps, descs, Fs, _ = _scene()
    full = _run(gpu, descs, kps, PAIRS, 1, Fs, THR, "mnn_ratio", 0.95)
    sub = [1, 5, 11, ZERO, 19, 15, 8]
    part = _run(gpu, descs, kps, [PAIRS[p] for p in sub], 1, Fs[sub], THR, "mnn_ratio", 0.95)
    assert sum(len(x) for x in part) > 20
    for k, p in enumerate(sub):
        assert np.array_equal(part[k], full[p]), p


# ---- end to end: verify_pair_list(guided=True) -------------------------------

E2E_THR, E2E_ITERS, E2E_SEED = 3.0, 256, 7
SLACK = 10 * GR.MEASURED_DEV
K_SMALL = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])


def _feature_files(root):
    """three images of one 3-D scene of 240 points; points 2k and 2k + 1 (k <
    40) look alike (descriptors closer to each other than the image-to-image
    noise), so the global nearest neighbour is often the wrong one of the two
    while the epipolar line tells them apart.  Returns the per-image features
    and the true F of every listed pair."""
    rs = np.random.RandomState(5)
    n = 240
    base = rs.randn(n, 128)
    base[1:80:2] = base[0:80:2] + 0.02 * rs.randn(40, 128)
    z = rs.uniform(3, 9, n)
    X = np.stack([rs.uniform(-0.5, 0.5, n) * z, rs.uniform(-0.4, 0.4, n) * z, z], 1)
    motions = [(np.eye(3), np.zeros(3)), (GR.rot([0.02, -0.1, 0.03]), np.array([0.8, 0.1, 0.1])),
               (GR.rot([-0.05, 0.08, -0.02]), np.array([-0.6, 0.3, 0.2]))]
    names, feats = ["a.jpg", "b.jpg", "c.jpg"], []
    for name, (R, t) in zip(names, motions):
        q = (X @ R.T + t) @ K_SMALL.T
        kp = np.zeros((n, 3), np.float32)
        perm = rs.permutation(n)
        kp[perm, :2] = (q[:, :2] / q[:, 2:] + rs.uniform(-0.3, 0.3, (n, 2))).astype(np.float32)
        d = base + 0.05 * rs.randn(n, 128)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        desc = np.zeros((n, 128), np.float32)
        desc[perm] = d.astype(np.float32)
        with open(os.path.join(root, name + ".test"), "wb") as f:
            np.savez(f, keypoints=kp, descriptors=desc, scores=np.ones(n, np.float32))
        feats.append((kp[:, :2].copy(), desc))
    with open(os.path.join(root, "pairs.txt"), "w") as f:
        f.write("a.jpg b.jpg\nb.jpg c.jpg\na.jpg c.jpg\n")
    pairs = [(0, 1), (1, 2), (0, 2)]
    Ki = np.linalg.inv(K_SMALL)
    Fs = []
    for a, b in pairs:
        (Ra, ta), (Rb, tb) = motions[a], motions[b]
        R = Rb @ Ra.T
        F = Ki.T @ _skew(tb - R @ ta) @ R @ Ki
        Fs.append(F / np.sqrt((F ** 2).sum()))
    return feats, pairs, np.stack(Fs)


def test_verify_pair_list_guided(gpu, tmp_path):
    from posfeat_amd import geometry, matchers
    from posfeat_amd.evaluation import verification
    root = str(tmp_path)
    feats, pairs, Ftrue = _feature_files(root)
    kps, descs = [k for k, _ in feats], [d for _, d in feats]
    # beforehand, in numpy: under the true F guided matching finds more than
    # mutual nearest neighbours offer RANSAC (n_verified cannot exceed those)
    for p, (a, b) in enumerate(pairs):
        sim = descs[a].astype(np.float64) @ descs[b].astype(np.float64).T
        nn12, nn21 = np.argmax(sim, 1), np.argmax(sim, 0)
        n_mnn = int((nn21[nn12] == np.arange(len(nn12))).sum())
        okr, okc = GR.pair_masks(1, Ftrue[p], kps[a], kps[b], E2E_THR)
        n_guided = len(GR.guided_pair(sim, okr, okc, 0, 0.95))
        assert n_guided >= n_mnn + 10, (p, n_guided, n_mnn)
    pairs_file = os.path.join(root, "pairs.txt")
    out_g, out_p = os.path.join(root, "guided.npz"), os.path.join(root, "plain.npz")
    res = verification.verify_pair_list(root, pairs_file, "test", iters=E2E_ITERS, thr=E2E_THR,
                                        seed=E2E_SEED, output=out_g, guided=True)
    plain = verification.verify_pair_list(root, pairs_file, "test", iters=E2E_ITERS, thr=E2E_THR,
                                          seed=E2E_SEED, output=out_p)
    today = ["pairs", "match_offsets", "matches", "model", "info", "n_matches"]
    saved_g, saved_p = np.load(out_g), np.load(out_p)
    assert list(saved_p.keys()) == today and list(saved_g.keys()) == today + ["n_verified"]
    # without the flag: what the direct calls give, array by array
    pool, set_off = matchers._pool(descs)
    kp_pool = torch.from_numpy(np.concatenate(kps, 0)).to(gpu)
    batch = matchers.match_pairs_device(pool, set_off, np.asarray(pairs, np.int32), "mnn", 0.95)
    counts, matches = (x.copy() for x in batch.read())
    M, info, inl = geometry.ransac_fundamental_pairs(kp_pool, batch, iters=E2E_ITERS, thr=E2E_THR,
                                                     seed=E2E_SEED)
    M, info, inl = M.cpu().numpy(), info.cpu().numpy(), inl.cpu().numpy().astype(bool)
    inliers = []
    for p in range(3):
        rows = slice(int(batch.moff[p]), int(batch.moff[p]) + int(counts[p]))
        inliers.append(matches[rows][inl[rows]])
    direct = dict(pairs=np.asarray([("a.jpg", "b.jpg"), ("b.jpg", "c.jpg"), ("a.jpg", "c.jpg")]),
                  match_offsets=np.concatenate([[0], np.cumsum([len(x) for x in inliers])]),
                  matches=np.concatenate(inliers, 0).astype(np.int32), model=M, info=info,
                  n_matches=counts)
    for key in today:
        assert saved_p[key].dtype == plain[key].dtype == direct[key].dtype, key
        assert saved_p[key].tobytes() == np.ascontiguousarray(direct[key]).tobytes(), key
        assert np.array_equal(saved_p[key], plain[key]), key
    # with it: the same model, info and raw counts; guided matches in place of the inliers
    for key in ("pairs", "model", "info", "n_matches"):
        assert np.array_equal(saved_g[key], saved_p[key]), key
    assert np.array_equal(saved_g["n_verified"], info[:, 1]) and saved_g["n_verified"].dtype == np.int32
    off = saved_g["match_offsets"]
    assert off.shape == (4,) and off[0] == 0 and off[-1] == saved_g["matches"].shape[0]
    assert saved_g["matches"].dtype == np.int32 and np.array_equal(res["matches"], saved_g["matches"])
    for p, (a, b) in enumerate(pairs):
        g = saved_g["matches"][off[p]:off[p + 1]]
        assert info[p, 0] == 0
        d = GR.sampson(M[p], kps[a], kps[b])
        assert (d[g[:, 0], g[:, 1]] <= E2E_THR + SLACK).all(), p
        assert (np.diff(g[:, 0]) > 0).all()
        inside = inliers[p][d[inliers[p][:, 0], inliers[p][:, 1]] <= E2E_THR - SLACK]
        assert len(inside) > 100 and set(map(tuple, inside.tolist())) <= set(map(tuple, g.tolist())), p
        print("pair %d: %d mutual NN, %d verified, %d guided" % (p, counts[p], info[p, 1], len(g)))
        assert len(g) > info[p, 1], p


def test_verify_pair_list_guided_other_models(gpu, tmp_path):
    """the homography and the essential model: the guided matches lie within
    thr of the written model (for E through F = K2^-T E K1^-1); a camera with
    distortion is refused"""
    from posfeat_amd.evaluation import verification
    root = str(tmp_path)
    feats, pairs, _ = _feature_files(root)
    kps = [k for k, _ in feats]
    pairs_file = os.path.join(root, "pairs.txt")
    intr = os.path.join(root, "intrinsics.txt")
    with open(intr, "w") as f:
        for nm in ("a.jpg", "b.jpg", "c.jpg"):
            f.write("%s PINHOLE 640 480 500 500 320 240\n" % nm)
    res = verification.verify_pair_list(root, pairs_file, "test", model="essential", iters=E2E_ITERS,
                                        thr=E2E_THR, seed=E2E_SEED, intrinsics=intr, guided=True)
    assert sorted(res) == ["cheir", "info", "match_offsets", "matches", "model", "n_matches",
                           "n_verified", "pairs", "pose"]
    Ki = np.linalg.inv(K_SMALL)
    off = res["match_offsets"]
    for p, (a, b) in enumerate(pairs):
        g = res["matches"][off[p]:off[p + 1]]
        F = Ki.T @ res["model"][p] @ Ki
        d = GR.sampson(F, kps[a], kps[b])
        assert res["info"][p, 0] == 0 and len(g) > res["n_verified"][p] > 150, p
        assert (d[g[:, 0], g[:, 1]] <= E2E_THR + SLACK).all(), p
    with open(intr, "w") as f:
        for nm in ("a.jpg", "b.jpg", "c.jpg"):
            f.write("%s SIMPLE_RADIAL 640 480 500 320 240 0.01\n" % nm)
    with pytest.raises(ValueError):
        verification.verify_pair_list(root, pairs_file, "test", model="essential", iters=E2E_ITERS,
                                      thr=E2E_THR, seed=E2E_SEED, intrinsics=intr, guided=True)
    # a general scene has no homography: whatever H RANSAC settles on, the
    # guided matches are the pairs within thr of it
    res = verification.verify_pair_list(root, pairs_file, "test", model="homography",
                                        iters=E2E_ITERS, thr=E2E_THR, seed=E2E_SEED, guided=True)
    off = res["match_offsets"]
    for p, (a, b) in enumerate(pairs):
        g = res["matches"][off[p]:off[p + 1]]
        if res["info"][p, 0] != 0:
            assert len(g) == 0
            continue
        d = GR.transfer(res["model"][p], kps[a], kps[b])
        assert (d[g[:, 0], g[:, 1]] <= E2E_THR + SLACK).all(), p
