"""posfeat_ransac_fundamental on the GPU against the numpy restatement of its
definitions (tests/fundamental_ref.py): one pair list, one call.  Synthetic
matches of 3-D points seen by two cameras (K = [500 0 320; 0 500 240; 0 0 1],
small rotation, sideways + forward baseline, depths 3..9), fp32 keypoints,
iters = 512 (two hypothesis blocks per pair), thr = 3, seed = 2024.  The
fixture comes from fixed numpy seeds; its preconditions -- (a) every good pair
has an all-inlier, non-rejected sample, (b) no Sampson distance of any scored
candidate or of the refit lies within 1e-6 px of thr, (c) every scored cubic
has relative root separation > 1e-6, (d) the refit's normal matrix has second
smallest / largest eigenvalue >= 1e-8 on good pairs -- are asserted on the
restatement before the device result is looked at, so counts, winners and masks
are compared exactly."""
import ctypes
import os

import numpy as np
import pytest
import torch

import fundamental_ref as FR

pytestmark = pytest.mark.gpu

W, HT = 640, 480
ITERS, THR, SEED = 512, 3.0, 2024
K_CAM = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])
GUARD = 64
FIXTURE_SEED = 22                                          # chosen so that the preconditions hold

# pair positions in the list
(EXACT, NOISY, BIG, FORWARD, SEVEN, SIX, EMPTY, COINCIDENT, DUP, SHARE1, SHARE2,
 BORDER) = range(12)
NPAIRS = 12
FAILING = (SIX, EMPTY, COINCIDENT)
GOOD = (EXACT, NOISY, BIG, FORWARD, DUP, SHARE1, SHARE2, BORDER)   # SEVEN: no refit, no outliers
SIZES = [300, 300, 2049, 300, 7, 6, 0, 40, 300, 120, 120, 200]


def _rot(ax):
    th = np.linalg.norm(ax)
    if th == 0:
        return np.eye(3)
    k = np.asarray(ax) / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


MOTION_A = (_rot([0.03, -0.05, 0.02]), np.array([0.6, 0.1, 0.4]))
MOTION_B = (_rot([-0.04, 0.03, -0.03]), np.array([-0.5, 0.15, 0.3]))
MOTION_FWD = (np.eye(3), np.array([0.0, 0.0, 0.8]))


def _f_gt(motion):
    R, t = motion
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K_CAM)
    return Ki.T @ tx @ R @ Ki


def _views(rs, motion, n):
    """n 3-D points in front of both cameras, inside both images: (p1, p2) [n, 2]"""
    R, t = motion
    e1, e2 = K_CAM @ (-R.T @ t), K_CAM @ t                 # the epipoles (pure forward motion:
    e1, e2 = e1[:2] / e1[2], e2[:2] / e2[2]                # the image centre); no point within 40 px
    out1, out2 = [], []
    while len(out1) < n:
        z = rs.uniform(3, 9)
        X = np.array([rs.uniform(-0.6, 0.6) * z, rs.uniform(-0.45, 0.45) * z, z])
        a, b = K_CAM @ X, K_CAM @ (R @ X + t)
        a, b = a[:2] / a[2], b[:2] / b[2]
        if np.linalg.norm(a - e1) < 40 or np.linalg.norm(b - e2) < 40:
            continue
        if 5 <= a[0] <= W - 5 and 5 <= a[1] <= HT - 5 and 5 <= b[0] <= W - 5 and 5 <= b[1] <= HT - 5:
            out1.append(a)
            out2.append(b)
    return np.asarray(out1), np.asarray(out2)


def _kp(rs, n):
    return (rs.uniform(0, 1, (n, 2)) * [W - 40, HT - 40] + 20).astype(np.float32)


def _fixture():
    """sets (keypoint arrays), pairs, per-pair matches [m, 2], planted masks,
    per-pair ground-truth F"""
    rs = np.random.RandomState(FIXTURE_SEED)
    sets, pairs, ms, planted, fgt = [], [], [], [], []

    def add(kp1, kp2, ia, ib, pl, motion, s1=None):
        if s1 is None:
            sets.append(kp1)
            s1 = len(sets) - 1
        sets.append(kp2)
        pairs.append((s1, len(sets) - 1))
        ms.append(np.stack([ia, ib], 1).astype(np.int32).reshape(-1, 2))
        planted.append(pl)
        fgt.append(None if motion is None else _f_gt(motion))
        return s1

    def scene(n, n_in, sigma, motion, extra=13, kp1=None, s1=None, ia=None):
        """n matches, n_in of them projections of one 3-D point (noise sigma in
        image 2), the rest between unrelated points"""
        p1, p2 = _views(rs, motion, n)
        if kp1 is None:
            kp1 = _kp(rs, n + extra)
            ia = np.sort(rs.permutation(n + extra)[:n])
            kp1[ia] = p1.astype(np.float32)
        else:                                              # a shared image-1 set: its own points
            R, t = motion
            p1 = kp1[ia].astype(np.float64)
            z = rs.uniform(3, 9, n)
            X = np.concatenate([(p1 - K_CAM[:2, 2]) / 500.0, np.ones((n, 1))], 1) * z[:, None]
            b = (X @ R.T + t) @ K_CAM.T
            p2 = b[:, :2] / b[:, 2:]
        pl = np.zeros(n, bool)
        pl[rs.permutation(n)[:n_in]] = True
        tgt = p2 + sigma * rs.randn(n, 2) * pl[:, None]
        tgt[~pl] = _kp(rs, int((~pl).sum()))
        if sigma == 0.0:                                   # the exact pairs: no outlier within 10 px
            F = _f_gt(motion)                              # of its epipolar line, so the planted
            while True:                                    # matches are the inliers of the truth
                near = ~pl & (FR.sampson(F, np.concatenate([p1, tgt], 1)) < 10.0)
                if not near.any():
                    break
                tgt[near] = _kp(rs, int(near.sum()))
        kp2 = _kp(rs, n + extra + 5)
        ib = rs.permutation(n + extra + 5)[:n]
        kp2[ib] = tgt.astype(np.float32)
        return add(kp1, kp2, ia, ib, pl, motion, s1), kp1, ia

    scene(300, 180, 0.0, MOTION_A)                         # EXACT
    scene(300, 180, 0.5, MOTION_A)                         # NOISY
    scene(2049, 1230, 0.5, MOTION_A)                       # BIG: 8 tiles and a remainder of 1
    scene(300, 180, 0.0, MOTION_FWD)                       # FORWARD
    scene(7, 7, 0.0, MOTION_A, extra=2)                    # SEVEN
    scene(6, 6, 0.0, MOTION_A, extra=2)                    # SIX
    sets += [_kp(rs, 50), _kp(rs, 40)]                     # EMPTY: 50 rows, no match
    pairs.append((len(sets) - 2, len(sets) - 1))
    ms.append(np.zeros((0, 2), np.int32))
    planted.append(np.zeros(0, bool))
    fgt.append(None)
    kc1, kc2 = _kp(rs, 45), _kp(rs, 50)                    # COINCIDENT: 40 matches of one point
    ia, ib = np.sort(rs.permutation(45)[:40]), rs.permutation(50)[:40]
    kc1[ia], kc2[ib] = kc1[ia[0]], kc2[ib[0]]
    add(kc1, kc2, ia, ib, np.ones(40, bool), None)
    p1, p2 = _views(rs, MOTION_A, 150)                     # DUP: 150 matches, each twice
    pl = np.zeros(150, bool)
    pl[rs.permutation(150)[:90]] = True
    p2 = p2 + 0.5 * rs.randn(150, 2) * pl[:, None]
    p2[~pl] = _kp(rs, 60)
    kd1, kd2 = _kp(rs, 320), _kp(rs, 200)
    ia, ib = np.sort(rs.permutation(320)[:150]), rs.permutation(200)[:150]
    kd1[ia], kd2[ib] = p1.astype(np.float32), p2.astype(np.float32)
    add(kd1, kd2, np.repeat(ia, 2), np.repeat(ib, 2), np.repeat(pl, 2), MOTION_A)
    s1, kps, ia = scene(120, 72, 0.5, MOTION_A, extra=20)  # SHARE1 / SHARE2: one image-1 set
    scene(120, 72, 0.5, MOTION_B, kp1=kps, s1=s1, ia=ia)
    # BORDER: 80 exact inliers, 20 more at a Sampson distance of 2.98 px from the
    # truth (inliers of the exact F that a least-squares refit pushes past thr),
    # 100 outliers: the pair whose refit is NOT kept
    rs = np.random.RandomState(701)
    F = _f_gt(MOTION_A)
    p1, p2 = _views(rs, MOTION_A, 200)
    pl = np.zeros(200, bool)
    pl[rs.permutation(200)[:100]] = True
    edge = np.flatnonzero(pl)[:20]
    for i in edge:
        line = F @ np.append(p1[i], 1.0)
        nrm = line[:2] / np.linalg.norm(line[:2]) * rs.choice([-1.0, 1.0])
        d = 2.98 * np.sqrt(2.0)
        for _ in range(6):                                 # the offset whose Sampson distance is 2.98
            s = FR.sampson(F, np.concatenate([p1[i], p2[i] + d * nrm])[None])[0]
            d *= 2.98 / s
        p2[i] = p2[i] + d * nrm
    p2[~pl] = _kp(rs, 100)
    kb1, kb2 = _kp(rs, 213), _kp(rs, 218)
    ia, ib = np.sort(rs.permutation(213)[:200]), rs.permutation(218)[:200]
    kb1[ia], kb2[ib] = p1.astype(np.float32), p2.astype(np.float32)
    add(kb1, kb2, ia, ib, pl, MOTION_A)
    return sets, np.asarray(pairs, np.int32), ms, planted, fgt


def _rows(sets, pairs, ms, p):
    """the (x1 y1 x2 y2) rows of pair p, as the device gathers them"""
    a, b = pairs[p]
    return np.concatenate([sets[a][ms[p][:, 0]], sets[b][ms[p][:, 1]]], 1)


_CACHE = {}


def _reference():
    """fixture + restatement (512 iterations per pair, finished at 512 and at
    100), computed once for the module"""
    if not _CACHE:
        sets, pairs, ms, planted, fgt = _fixture()
        ref = {ITERS: [], 100: []}
        samples, rows = [], []
        for p in range(len(pairs)):
            m = _rows(sets, pairs, ms, p)
            rows.append(m.astype(np.float64))
            nm, Fs, smp, sep = FR.hypotheses(m, p, ITERS, SEED)
            samples.append((Fs, smp, sep))
            for iters in ref:
                ref[iters].append(FR.finish(m, nm, Fs[:iters], THR))
        _CACHE.update(sets=sets, pairs=pairs, ms=ms, planted=planted, fgt=fgt, ref=ref,
                      samples=samples, rows=rows)
    return _CACHE


def _device_inputs(c, dev):
    sizes = [k.shape[0] for k in c["sets"]]
    set_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n1 = np.asarray([sizes[a] for a, _ in c["pairs"]])
    moff = np.concatenate([[0], np.cumsum(n1)])
    matches = np.full((moff[-1], 2), -1, np.int32)         # rows past a pair's count: garbage
    counts = np.zeros(len(c["pairs"]), np.int32)
    for p, m in enumerate(c["ms"]):
        matches[moff[p]:moff[p] + len(m)] = m
        counts[p] = len(m)
    kp_pool = torch.from_numpy(np.concatenate(c["sets"], 0)).to(dev)
    return set_off, moff, matches, counts, kp_pool


def _call(dev, kp_pool, set_off, pairs, matches, counts, iters, npairs=None):
    """the C ABI on the first npairs pairs with guarded inputs and outputs:
    asserts the guards, matches and counts are untouched; returns host (F, info,
    inlier)"""
    from posfeat_amd._lib import check, lib, ptr, stream_ptr
    npairs = len(pairs) if npairs is None else npairs
    pairs = np.ascontiguousarray(pairs[:npairs])
    n1 = (set_off[1:] - set_off[:-1])[pairs[:, 0]]
    total = int(n1.sum())
    so, pp = ctypes.c_void_p(set_off.ctypes.data), ctypes.c_void_p(pairs.ctypes.data)
    need = lib().posfeat_ransac_fundamental_workspace(so, len(set_off) - 1, pp, npairs, iters)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    md, cd = torch.from_numpy(matches).to(dev), torch.from_numpy(counts).to(dev)
    F = torch.full((npairs * 9 + GUARD,), 7.5, dtype=torch.float64, device=dev)
    info = torch.full((npairs * 4 + GUARD,), -77, dtype=torch.int32, device=dev)
    inl = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    kp_before = kp_pool.clone()
    check(lib().posfeat_ransac_fundamental(ptr(kp_pool), so, len(set_off) - 1, pp, npairs, ptr(md),
                                           ptr(cd), iters, THR, SEED, ptr(F), ptr(info), ptr(inl),
                                           ptr(ws), need, stream_ptr(dev)))
    torch.cuda.synchronize()
    F, info, inl = F.cpu().numpy(), info.cpu().numpy(), inl.cpu().numpy()
    assert (F[npairs * 9:] == 7.5).all() and (info[npairs * 4:] == -77).all()
    assert (inl[total:] == 0xAB).all(), "inlier rows beyond sum n1 were written"
    assert np.array_equal(md.cpu().numpy(), matches) and np.array_equal(cd.cpu().numpy(), counts)
    assert torch.equal(kp_pool, kp_before)
    return F[:npairs * 9].reshape(npairs, 3, 3), info[:npairs * 4].reshape(npairs, 4), inl[:total]


def _preconditions(c):
    """asserted on the restatement before any device result is looked at"""
    assert len(c["pairs"]) == NPAIRS
    assert [len(m) for m in c["ms"]] == SIZES
    assert c["pairs"][SHARE1][0] == c["pairs"][SHARE2][0]
    for p in GOOD + (SEVEN,):
        Fs, smp, sep = c["samples"][p]
        pl = c["planted"][p]
        clean = [it for it in range(ITERS) if Fs[it] and pl[smp[it]].all()]
        clean100 = [it for it in clean if it < 100]
        r = c["ref"][ITERS][p]
        print("pair %d: %d all-inlier non-rejected samples (%d below 100), margin %.3g px (512) "
              "%.3g px (100), root separation %.3g"
              % (p, len(clean), len(clean100), r["margin"], c["ref"][100][p]["margin"], sep))
        assert clean, "precondition (a) fails for pair %d" % p
        assert sep > 1e-6, "precondition (c) fails for pair %d" % p
    for iters in (ITERS, 100):
        for p in range(NPAIRS):
            assert c["ref"][iters][p]["margin"] > 1e-6, "precondition (b) fails for pair %d" % p
        for p in GOOD:
            eig = c["ref"][iters][p]["eig"]
            print("iters %d pair %d: second smallest / largest eigenvalue %.3g"
                  % (iters, p, eig[1] / eig[-1]))
            assert eig[1] / eig[-1] >= 1e-8, "precondition (d) fails for pair %d" % p
    for p in FAILING:
        assert c["ref"][ITERS][p]["status"] == 1
    for p in GOOD:                                         # planted inliers are found
        r = c["ref"][ITERS][p]
        assert r["status"] == 0 and r["mask"][c["planted"][p]].all(), p
        # an outlier lands within thr of its epipolar line with probability about
        # 2 thr / image height = 1.25 %: at most 5 % of the outliers, plus 5
        n_out = int((~c["planted"][p]).sum())
        assert r["n_inliers"] <= c["planted"][p].sum() + 0.05 * n_out + 5, p
    b = c["ref"][ITERS][BORDER]                            # both outcomes of the refit occur
    assert b["refit_kept"] == 0 and b["n_refit"] < b["n_min"]
    assert sum(c["ref"][ITERS][p]["refit_kept"] for p in GOOD) >= 4
    s = c["ref"][ITERS][SEVEN]                             # every root fits all seven: the tie rule
    assert (s["n_inliers"], s["best_iter"], s["root"], s["refit_kept"]) == (7, 0, 0, 0)
    assert len(c["samples"][SEVEN][0][0]) == 3, "SEVEN needs three real roots at iteration 0"
    # the restatement's F against the truth on the exact pairs (fp32 keypoints)
    for p in (EXACT, FORWARD):
        m = c["rows"][p][c["planted"][p]]
        err = FR.sampson(c["ref"][ITERS][p]["F"], m).max()
        print("restatement on the planted points of pair %d: %.3g px (truth: %.3g px)"
              % (p, err, FR.sampson(c["fgt"][p], m).max()))
        assert err <= 1e-3
        assert np.array_equal(c["ref"][ITERS][p]["mask"], c["planted"][p])


def test_fixture_preconditions():
    _preconditions(_reference())


def _check_unit_and_sign(F):
    f = F.reshape(-1)
    assert abs(np.sqrt((f ** 2).sum()) - 1.0) <= 1e-14
    assert f[int(np.argmax(np.abs(f)))] > 0


def _compare(c, F, info, inl, moff, iters, npairs):
    ref = c["ref"][iters]
    for p in range(npairs):
        r, n = ref[p], len(c["ms"][p])
        n1 = moff[p + 1] - moff[p]
        rows = inl[moff[p]:moff[p] + n1]
        got = (info[p, 0], info[p, 1], info[p, 2], info[p, 3] >> 8, info[p, 3] & 255)
        want = (r["status"], r["n_inliers"], r["best_iter"], r["root"], r["refit_kept"])
        assert got == want, (p, got, want)
        assert np.array_equal(rows[:n], r["mask"].astype(np.uint8)), p
        assert not rows[n:].any(), "rows past counts[p] must be 0 (pair %d)" % p
        if r["status"] == 1:
            assert not F[p].any() and not rows.any() and info[p].tolist() == [1, 0, -1, 0]
            continue
        _check_unit_and_sign(F[p])
        m = c["rows"][p][c["planted"][p]]
        err = float(np.abs(FR.sampson(F[p], m) - FR.sampson(r["F"], m)).max())
        ratio = r["eig"][1] / r["eig"][-1]
        print("iters %d pair %d: eigenvalue ratio %.3g, device vs restatement %.3g px, inliers %d "
              "(minimal %d, refit %d, kept %d, root %d)"
              % (iters, p, ratio, err, r["n_inliers"], r["n_min"], r["n_refit"], r["refit_kept"],
                 r["root"]))
        assert err <= 1e-6, (p, err)
        assert info[p, 1] == (r["n_refit"] if r["refit_kept"] else r["n_min"])


def test_fundamental_pairs_vs_restatement(gpu):
    c = _reference()
    _preconditions(c)
    set_off, moff, matches, counts, kp_pool = _device_inputs(c, gpu)
    F, info, inl = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, ITERS)
    _compare(c, F, info, inl, moff, ITERS, NPAIRS)
    for p in GOOD:                                         # planted is a subset of the mask
        mask = inl[moff[p]:moff[p] + SIZES[p]].astype(bool)
        assert mask[c["planted"][p]].all(), p
    for p in (EXACT, FORWARD):                             # fp32 keypoint rounding
        err = FR.sampson(F[p], c["rows"][p][c["planted"][p]]).max()
        print("device F on the planted points of pair %d: %.3g px" % (p, err))
        assert err <= 1e-3
    assert info[BORDER, 3] & 255 == 0 and info[SEVEN].tolist() == [0, 7, 0, 0]
    for p in FAILING:
        assert info[p].tolist() == [1, 0, -1, 0] and not F[p].any()
        assert not inl[moff[p]:moff[p + 1]].any()
    # determinism: a second call, and the list truncated after a pair
    F2, info2, inl2 = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, ITERS)
    assert F.tobytes() == F2.tobytes() and np.array_equal(info, info2)
    assert np.array_equal(inl, inl2)
    for k in (BIG + 1, DUP + 1):
        Fk, infok, inlk = _call(gpu, kp_pool, set_off, c["pairs"], matches[:moff[k]], counts[:k],
                                ITERS, npairs=k)
        assert Fk.tobytes() == F[:k].tobytes() and np.array_equal(infok, info[:k])
        assert np.array_equal(inlk, inl[:moff[k]])


def test_fundamental_pairs_partial_block(gpu):
    c = _reference()
    _preconditions(c)
    set_off, moff, matches, counts, kp_pool = _device_inputs(c, gpu)
    F, info, inl = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, 100)
    _compare(c, F, info, inl, moff, 100, NPAIRS)
    assert info[:, 2].max() < 100


def test_python_entry_points(gpu):
    """geometry.ransac_fundamental_pairs on a PairBatch, and find_fundamental"""
    from posfeat_amd import geometry, matchers
    c = _reference()
    set_off, moff, matches, counts, kp_pool = _device_inputs(c, gpu)
    buf = torch.from_numpy(np.concatenate([counts, matches.reshape(-1)])).to(gpu)
    batch = matchers.PairBatch(None, set_off, c["pairs"], moff, buf)
    F, info, inl = geometry.ransac_fundamental_pairs(kp_pool, batch, iters=ITERS, thr=THR,
                                                     seed=SEED)
    assert F.dtype == torch.float64 and tuple(F.shape) == (NPAIRS, 3, 3)
    assert info.dtype == torch.int32 and tuple(info.shape) == (NPAIRS, 4)
    assert inl.dtype == torch.uint8 and inl.shape[0] == moff[-1]
    Fc, infoc, inlc = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, ITERS)
    assert F.cpu().numpy().tobytes() == Fc.tobytes()
    assert np.array_equal(info.cpu().numpy(), infoc) and np.array_equal(inl.cpu().numpy(), inlc)
    # one pair, numpy in and out: pair position 0, so the EXACT pair's own result
    a, b = c["pairs"][EXACT]
    F1, mask, inf1 = geometry.find_fundamental(c["sets"][a], c["sets"][b], c["ms"][EXACT],
                                               iters=ITERS, thr=THR, seed=SEED)
    assert F1.tobytes() == Fc[EXACT].tobytes() and np.array_equal(inf1, infoc[EXACT])
    assert mask.dtype == bool and np.array_equal(mask, inlc[:SIZES[EXACT]].astype(bool))
    with pytest.raises(ValueError):
        geometry.ransac_fundamental_pairs(kp_pool, batch, iters=0)


def _feature_files(tmp_path):
    """four tiny feature files whose mutual-NN matches are known: every image
    holds the same 200 random unit descriptors in its own row order, so row
    perm_a[i] of image a matches row perm_b[i] of image b; a, b and c see one
    3-D scene, d's keypoints are unrelated"""
    rs = np.random.RandomState(99)
    n = 200
    base = rs.randn(n, 128).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    z = rs.uniform(3, 9, n)                                # one scene seen by a, b and c
    X = np.stack([rs.uniform(-0.5, 0.5, n) * z, rs.uniform(-0.4, 0.4, n) * z, z], 1)
    views = []
    for R, t in ((np.eye(3), np.zeros(3)), MOTION_A, MOTION_B):
        q = (X @ R.T + t) @ K_CAM.T
        views.append(q[:, :2] / q[:, 2:])
    names, perms = ["a.jpg", "b.jpg", "c.jpg", "d.jpg"], []
    kps = views + [_kp(rs, n).astype(np.float64)]
    for k, name in enumerate(names):
        perm = rs.permutation(n)
        perms.append(perm)
        kp = np.zeros((n, 3), np.float32)
        kp[perm, :2] = kps[k].astype(np.float32)           # row perm[i] holds point i
        desc = np.zeros((n, 128), np.float32)
        desc[perm] = base
        with open(os.path.join(str(tmp_path), name + ".test"), "wb") as f:   # as extract.py writes
            np.savez(f, keypoints=kp, descriptors=desc, scores=np.ones(n, np.float32))
    with open(os.path.join(str(tmp_path), "pairs.txt"), "w") as f:
        f.write("a.jpg b.jpg\nb.jpg c.jpg\n\na.jpg d.jpg\n")
    return names, perms


def test_verify_pair_list(gpu, tmp_path):
    """the consumer: .npz features + a pair list -> verified matches, equal to a
    direct match_pairs_device + ransac_*_pairs on the same data"""
    from posfeat_amd import geometry, matchers
    from posfeat_amd.evaluation import verification
    names, perms = _feature_files(tmp_path)
    pairs_file = os.path.join(str(tmp_path), "pairs.txt")
    feats = [np.load(os.path.join(str(tmp_path), nm + ".test")) for nm in names]
    descs = [f["descriptors"] for f in feats]
    pool, set_off = matchers._pool(descs)
    kp_pool = torch.from_numpy(np.concatenate([f["keypoints"][:, :2] for f in feats], 0)).to(gpu)
    pairs = np.asarray([[0, 1], [1, 2], [0, 3]], np.int32)
    batch = matchers.match_pairs_device(pool, set_off, pairs, "mnn", 0.95)
    counts, matches = batch.read()
    counts, matches = counts.copy(), matches.copy()
    # the mutual-NN matches are the known ones: row perm_a[i] <-> row perm_b[i]
    for p, (a, b) in enumerate(pairs):
        m = matches[batch.moff[p]:batch.moff[p] + counts[p]]
        want = np.stack([perms[a], perms[b]], 1)
        assert counts[p] == 200 and np.array_equal(m, want[np.argsort(want[:, 0])])
    for model, fn in (("fundamental", geometry.ransac_fundamental_pairs),
                      ("homography", geometry.ransac_homography_pairs)):
        out = os.path.join(str(tmp_path), "verified_%s.npz" % model)
        res = verification.verify_pair_list(str(tmp_path), pairs_file, "test", model=model,
                                            iters=256, thr=3.0, seed=7, output=out)
        M, info, inl = fn(kp_pool, batch, iters=256, thr=3.0, seed=7)
        M, info, inl = M.cpu().numpy(), info.cpu().numpy(), inl.cpu().numpy().astype(bool)
        saved = np.load(out)
        assert [tuple(x) for x in saved["pairs"]] == [("a.jpg", "b.jpg"), ("b.jpg", "c.jpg"),
                                                      ("a.jpg", "d.jpg")]
        assert saved["model"].tobytes() == M.tobytes() and np.array_equal(saved["info"], info)
        assert np.array_equal(saved["model"], res["model"])
        off = saved["match_offsets"]
        assert off.shape == (4,) and off[0] == 0
        for p in range(3):
            m = matches[batch.moff[p]:batch.moff[p] + counts[p]]
            keep = inl[batch.moff[p]:batch.moff[p] + counts[p]]
            assert np.array_equal(saved["matches"][off[p]:off[p + 1]], m[keep]), (model, p)
            assert off[p + 1] - off[p] == info[p, 1]
        if model == "fundamental":                         # two true motions, one unrelated image
            assert info[0, 1] == 200 and info[1, 1] == 200 and info[2, 1] < 30
            # two chunks: the third pair is pair 0 of its own chunk (another sample stream)
            two = verification.verify_pair_list(str(tmp_path), pairs_file, "test", iters=256,
                                                thr=3.0, seed=7, chunk=2)
            assert np.array_equal(two["n_matches"], counts) and two["info"][0, 1] == 200
            assert two["model"][:2].tobytes() == M[:2].tobytes()
            assert two["match_offsets"][-1] == two["matches"].shape[0]
