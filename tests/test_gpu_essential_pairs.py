"""posfeat_ransac_essential on the GPU against the numpy restatement of its
definitions (tests/essential_ref.py): one pair list, one call.  Synthetic
matches of 3-D points seen by two calibrated cameras (f = 500, centre (320,
240) unless the pair says otherwise), fp32 keypoints, iters = 512 (two
hypothesis blocks per pair) and 100 (a partial block), thr = 3, seed = 2024.
The fixture comes from fixed numpy seeds; its preconditions -- (a) every good
pair has an all-inlier, non-rejected sample, (b) no Sampson distance of any
scored candidate or of the refit lies within 1e-6 relative of thr_n, (c) every
scored degree-10 polynomial has relative real-root separation > 1e-6 and no
root's |Im| within a factor 100 of the real / complex tolerance, (d) the
refit's normal matrix has second smallest / largest eigenvalue >= 1e-8 on good
pairs -- are asserted on the restatement before the device result is looked at,
so counts, winners, masks and cheirality indices are compared exactly.

Bounds.  The device and the restatement run the same operations with another
rounding (fma in the score, another order inside a product), and the
five-point solve amplifies rounding by the conditioning of the winning sample,
which differs from pair to pair by orders of magnitude.  So the restatement
measures its own rounding noise per pair: the winner's sample is solved again
with its five rows in reverse order, the refit again with the inlier rows in
reverse order -- the same problem, other roundings.  The device may differ from
the restatement by 100 times that (the project's rule in
test_solve7_against_an_independent_method), plus a floor of 1e-9 px and 1e-12
on a pose entry for a pair whose two restatement runs happen to agree to the
last bit (2^-52 * 500 px, or * 1, times a few hundred operations).  Poses are
compared entry by entry: an angle through arccos resolves only 1e-8 near 0.  Device pose against the planted
pose on the exact pairs: fp32 keypoints move a point by up to 2^-24 * 640 =
4e-5 px = 8e-8 in normalised coordinates; with baselines of 0.7 against depths
of 3..9 a least-squares fit over 180 points moves the pose by at most a few
hundred times that: 1e-3 degrees is asserted, the measured values are
printed."""
import ctypes

import numpy as np
import pytest
import torch

import essential_ref as ER

pytestmark = pytest.mark.gpu

W, HT = 640, 480
ITERS, THR, SEED = 512, 3.0, 2024
CAM = np.array([500.0, 500.0, 320.0, 240.0, 0.0, 0.0, 0.0, 0.0])
CAM_D1 = np.array([400.0, 400.0, 320.0, 240.0, -0.1, 0.0, 0.0, 0.0])
CAM_D2 = np.array([900.0, 900.0, 320.0, 240.0, 0.05, 0.0, 0.0, 0.0])
GUARD = 64
# one numpy seed per scene of the list (EMPTY and DUP draw nothing of their own),
# chosen so that the preconditions hold
SCENE_SEEDS = {"EXACT": 0, "NOISY": 0, "BIG": 2, "FORWARD": 0, "PLANAR": 2, "DISTORTED": 0,
               "FIVE": 0, "FOUR": 0, "COINCIDENT": 0, "SHARE": 0}

# pair positions in the list
(EXACT, NOISY, BIG, FORWARD, PLANAR, DISTORTED, FIVE, FOUR, EMPTY, COINCIDENT, DUP, SHARE1,
 SHARE2, BORDER) = range(14)
NPAIRS = 14
FAILING = (FOUR, EMPTY, COINCIDENT)
GOOD = (EXACT, NOISY, BIG, FORWARD, PLANAR, DISTORTED, DUP, SHARE1, SHARE2, BORDER)
SIZES = [300, 300, 2049, 300, 300, 300, 5, 4, 0, 40, 300, 120, 120, 200]


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


def _e_gt(motion):
    R, t = motion
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    return tx @ R


def _pose_gt(motion):
    R, t = motion
    return np.concatenate([R, (t / np.linalg.norm(t))[:, None]], 1)


def _project(cam, xn):
    """normalised points [n, 2] -> pixels under the SIMPLE_RADIAL model"""
    f = 1.0 + cam[4] * (xn ** 2).sum(1, keepdims=True)
    return xn * f * cam[:2] + cam[2:4]


def _views(rs, motion, n, cam1, cam2, planar=False):
    """n 3-D points in front of both cameras: normalised (x1, x2) [n, 2]"""
    R, t = motion
    z = rs.uniform(3, 9, n)
    X = np.stack([rs.uniform(-0.45, 0.45, n) * z, rs.uniform(-0.35, 0.35, n) * z, z], 1)
    if planar:                                             # the plane z = 6 + 0.5 x - 0.3 y
        X[:, 2] = 6.0 + 0.5 * X[:, 0] - 0.3 * X[:, 1]
    Y = X @ R.T + t
    assert (X[:, 2] > 1).all() and (Y[:, 2] > 1).all()
    return X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]


def _kp(rs, n):
    return (rs.uniform(0, 1, (n, 2)) * [W - 40, HT - 40] + 20).astype(np.float32)


def _fixture():
    """sets (keypoint arrays), their cameras, pairs, per-pair matches [m, 2],
    planted masks, per-pair motion"""
    rs = np.random.RandomState(0)
    sets, cams, pairs, ms, planted, motions = [], [], [], [], [], []

    def add(kp1, kp2, cam1, cam2, ia, ib, pl, motion, s1=None):
        if s1 is None:
            sets.append(kp1)
            cams.append(cam1)
            s1 = len(sets) - 1
        sets.append(kp2)
        cams.append(cam2)
        pairs.append((s1, len(sets) - 1))
        ms.append(np.stack([ia, ib], 1).astype(np.int32).reshape(-1, 2))
        planted.append(pl)
        motions.append(motion)
        return s1

    def scene(n, n_in, sigma, motion, extra=13, cam1=CAM, cam2=CAM, planar=False, kp1=None,
              s1=None, ia=None):
        """n matches, n_in of them views of one 3-D point (pixel noise sigma in
        image 2), the rest between unrelated points"""
        x1, x2 = _views(rs, motion, n, cam1, cam2, planar)
        if kp1 is None:
            kp1 = _kp(rs, n + extra)
            ia = np.sort(rs.permutation(n + extra)[:n])
            kp1[ia] = _project(cam1, x1).astype(np.float32)
        else:                                              # a shared image-1 set: its own points
            R, t = motion
            x1 = ER.undistort(cam1, kp1[ia].astype(np.float64))
            z = rs.uniform(3, 9, n)
            Y = (np.concatenate([x1, np.ones((n, 1))], 1) * z[:, None]) @ R.T + t
            x2 = Y[:, :2] / Y[:, 2:]
        pl = np.zeros(n, bool)
        pl[rs.permutation(n)[:n_in]] = True
        tgt = _project(cam2, x2) + sigma * rs.randn(n, 2) * pl[:, None]
        tgt[~pl] = _kp(rs, int((~pl).sum()))
        if sigma == 0.0:                                   # the exact pairs: no outlier within 10 px
            E = _e_gt(motion)                              # of its epipolar line, so the planted
            for _ in range(200):                           # matches are the inliers of the truth
                d = ER.sampson(E, np.concatenate([x1, ER.undistort(cam2, tgt)], 1))
                near = ~pl & ~(d >= ER.thr_norm(cam1, cam2, 10.0))
                if not near.any():
                    break
                tgt[near] = _kp(rs, int(near.sum()))
            assert not near.any()
        kp2 = _kp(rs, n + extra + 5)
        ib = rs.permutation(n + extra + 5)[:n]
        kp2[ib] = tgt.astype(np.float32)
        return add(kp1, kp2, cam1, cam2, ia, ib, pl, motion, s1), kp1, ia

    rs.seed(SCENE_SEEDS["EXACT"])
    scene(300, 180, 0.0, MOTION_A)                         # EXACT
    rs.seed(SCENE_SEEDS["NOISY"])
    scene(300, 210, 0.5, MOTION_A)                         # NOISY: 30 % outliers
    rs.seed(SCENE_SEEDS["BIG"])
    scene(2049, 1230, 0.5, MOTION_A)                       # BIG: 8 tiles and a remainder of 1
    rs.seed(SCENE_SEEDS["FORWARD"])
    scene(300, 180, 0.0, MOTION_FWD)                       # FORWARD
    rs.seed(SCENE_SEEDS["PLANAR"])
    scene(300, 180, 0.5, MOTION_A, planar=True)            # PLANAR: degenerate for F, not for E
    rs.seed(SCENE_SEEDS["DISTORTED"])
    scene(300, 180, 0.0, MOTION_A, cam1=CAM_D1, cam2=CAM_D2)   # DISTORTED
    rs.seed(SCENE_SEEDS["FIVE"])
    scene(5, 5, 0.0, MOTION_A, extra=2)                    # FIVE
    rs.seed(SCENE_SEEDS["FOUR"])
    scene(4, 4, 0.0, MOTION_A, extra=2)                    # FOUR
    sets += [_kp(rs, 50), _kp(rs, 40)]                     # EMPTY: 50 rows, no match
    cams += [CAM, CAM]
    pairs.append((len(sets) - 2, len(sets) - 1))
    ms.append(np.zeros((0, 2), np.int32))
    planted.append(np.zeros(0, bool))
    motions.append(None)
    rs.seed(SCENE_SEEDS["COINCIDENT"])
    kc1, kc2 = _kp(rs, 45), _kp(rs, 50)                    # COINCIDENT: 40 matches of one point
    ia, ib = np.sort(rs.permutation(45)[:40]), rs.permutation(50)[:40]
    kc1[ia], kc2[ib] = kc1[ia[0]], kc2[ib[0]]
    add(kc1, kc2, CAM, CAM, ia, ib, np.ones(40, bool), None)
    pairs.append(pairs[EXACT])                             # DUP: EXACT's sets and matches again
    ms.append(ms[EXACT])
    planted.append(planted[EXACT])
    motions.append(MOTION_A)
    rs.seed(SCENE_SEEDS["SHARE"])
    s1, kps, ia = scene(120, 72, 0.5, MOTION_A, extra=20)  # SHARE1 / SHARE2: one image-1 set
    scene(120, 72, 0.5, MOTION_B, kp1=kps, s1=s1, ia=ia)
    # BORDER: 80 exact inliers, 20 more at a Sampson distance of 2.98 px (in
    # units of thr_n / thr) from the truth, inliers of the exact E that a
    # least-squares refit pushes past thr, 100 outliers: the refit is NOT kept
    rs = np.random.RandomState(701)
    E = _e_gt(MOTION_A)
    x1, x2 = _views(rs, MOTION_A, 200, CAM, CAM)
    pl = np.zeros(200, bool)
    pl[rs.permutation(200)[:100]] = True
    unit_px = ER.thr_norm(CAM, CAM, 1.0)
    for i in np.flatnonzero(pl)[:20]:
        line = E @ np.append(x1[i], 1.0)
        nrm = line[:2] / np.linalg.norm(line[:2]) * rs.choice([-1.0, 1.0])
        d = 2.98 * unit_px * np.sqrt(2.0)
        for _ in range(6):                                 # the offset whose Sampson distance is 2.98
            s = ER.sampson(E, np.concatenate([x1[i], x2[i] + d * nrm])[None])[0]
            d *= 2.98 * unit_px / s
        x2[i] = x2[i] + d * nrm
    p1, p2 = _project(CAM, x1), _project(CAM, x2)
    p2[~pl] = _kp(rs, 100)
    kb1, kb2 = _kp(rs, 213), _kp(rs, 218)
    ia, ib = np.sort(rs.permutation(213)[:200]), rs.permutation(218)[:200]
    kb1[ia], kb2[ib] = p1.astype(np.float32), p2.astype(np.float32)
    add(kb1, kb2, CAM, CAM, ia, ib, pl, MOTION_A)
    return sets, np.asarray(cams), np.asarray(pairs, np.int32), ms, planted, motions


_CACHE = {}


def _reference():
    """fixture + restatement (512 iterations per pair, finished at 512 and at
    100), computed once for the module"""
    if not _CACHE:
        sets, cams, pairs, ms, planted, motions = _fixture()
        ref = {ITERS: [], 100: []}
        samples, rows, thr_n = [], [], []
        for p, (a, b) in enumerate(pairs):
            m = ER.rows(sets[a][ms[p][:, 0]], sets[b][ms[p][:, 1]], cams[a], cams[b])
            rows.append(m)
            thr_n.append(ER.thr_norm(cams[a], cams[b], THR))
            Es, smp, sep, fac = ER.hypotheses(m, p, ITERS, SEED)
            samples.append((Es, smp, sep, fac))
            for iters in ref:
                ref[iters].append(ER.finish(m, Es[:iters], thr_n[p]))
        _CACHE.update(sets=sets, cams=cams, pairs=pairs, ms=ms, planted=planted, motions=motions,
                      ref=ref, samples=samples, rows=rows, thr_n=thr_n)
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
    cams = torch.from_numpy(np.ascontiguousarray(c["cams"], np.float64)).to(dev)
    return set_off, moff, matches, counts, kp_pool, cams


def _call(dev, kp_pool, cams, set_off, pairs, matches, counts, iters, npairs=None):
    """the C ABI on the first npairs pairs with guarded outputs: asserts the
    guards and the inputs are untouched; returns host (E, pose, info, cheir,
    inlier)"""
    from posfeat_amd._lib import check, lib, ptr, stream_ptr
    npairs = len(pairs) if npairs is None else npairs
    pairs = np.ascontiguousarray(pairs[:npairs])
    n1 = (set_off[1:] - set_off[:-1])[pairs[:, 0]]
    total = int(n1.sum())
    so, pp = ctypes.c_void_p(set_off.ctypes.data), ctypes.c_void_p(pairs.ctypes.data)
    need = lib().posfeat_ransac_essential_workspace(so, len(set_off) - 1, pp, npairs, iters)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    md, cd = torch.from_numpy(matches).to(dev), torch.from_numpy(counts).to(dev)
    E = torch.full((npairs * 9 + GUARD,), 7.5, dtype=torch.float64, device=dev)
    pose = torch.full((npairs * 12 + GUARD,), 7.5, dtype=torch.float64, device=dev)
    info = torch.full((npairs * 4 + GUARD,), -77, dtype=torch.int32, device=dev)
    cheir = torch.full((npairs * 2 + GUARD,), -77, dtype=torch.int32, device=dev)
    inl = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    kp_before, cams_before = kp_pool.clone(), cams.clone()
    check(lib().posfeat_ransac_essential(ptr(kp_pool), ptr(cams), so, len(set_off) - 1, pp, npairs,
                                         ptr(md), ptr(cd), iters, THR, SEED, ptr(E), ptr(pose),
                                         ptr(info), ptr(cheir), ptr(inl), ptr(ws), need,
                                         stream_ptr(dev)))
    torch.cuda.synchronize()
    E, pose, info, cheir, inl = (t.cpu().numpy() for t in (E, pose, info, cheir, inl))
    assert (E[npairs * 9:] == 7.5).all() and (pose[npairs * 12:] == 7.5).all()
    assert (info[npairs * 4:] == -77).all() and (cheir[npairs * 2:] == -77).all()
    assert (inl[total:] == 0xAB).all(), "inlier rows beyond sum n1 were written"
    assert np.array_equal(md.cpu().numpy(), matches) and np.array_equal(cd.cpu().numpy(), counts)
    assert torch.equal(kp_pool, kp_before) and torch.equal(cams, cams_before)
    return (E[:npairs * 9].reshape(npairs, 3, 3), pose[:npairs * 12].reshape(npairs, 3, 4),
            info[:npairs * 4].reshape(npairs, 4), cheir[:npairs * 2].reshape(npairs, 2),
            inl[:total])


def _pose_error(P, Q):
    """(rotation, translation direction) difference in degrees"""
    from posfeat_amd.evaluation.relative_pose import relative_pose_errors
    r, t = relative_pose_errors(P, Q)
    return float(r), float(t)


def _preconditions(c):
    """asserted on the restatement before any device result is looked at"""
    assert len(c["pairs"]) == NPAIRS
    assert [len(m) for m in c["ms"]] == SIZES
    assert c["pairs"][SHARE1][0] == c["pairs"][SHARE2][0]
    assert tuple(c["pairs"][DUP]) == tuple(c["pairs"][EXACT])
    for p in GOOD + (FIVE,):
        Es, smp, sep, fac = c["samples"][p]
        pl = c["planted"][p]
        clean = [it for it in range(ITERS) if Es[it] and pl[smp[it]].all()]
        clean100 = [it for it in clean if it < 100]
        r = c["ref"][ITERS][p]
        print("pair %d: %d all-inlier non-rejected samples (%d below 100), margin %.3g (512) "
              "%.3g (100) of thr_n, root separation %.3g, |Im| / tolerance factor %.3g, "
              "%.2f candidates per sample"
              % (p, len(clean), len(clean100), r["margin"], c["ref"][100][p]["margin"], sep, fac,
                 np.mean([len(e) for e in Es])))
        assert clean100, "precondition (a) fails for pair %d" % p
        assert sep > 1e-6 and fac > 100.0, "precondition (c) fails for pair %d" % p
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
        assert r["cheir"][1] >= c["planted"][p].sum(), p   # every planted match is in front
    b = c["ref"][ITERS][BORDER]                            # both outcomes of the refit occur
    assert b["refit_kept"] == 0 and b["n_refit"] < b["n_min"]
    assert sum(c["ref"][ITERS][p]["refit_kept"] for p in GOOD) >= 4
    s = c["ref"][ITERS][FIVE]                              # every root fits all five: the tie rule
    assert (s["n_inliers"], s["best_iter"], s["root"], s["refit_kept"]) == (5, 0, 0, 0)
    assert len(c["samples"][FIVE][0][0]) >= 2, "FIVE needs several real roots at iteration 0"
    # the restatement's pose against the truth on the exact pairs (fp32 keypoints)
    for p in (EXACT, DISTORTED):
        r = c["ref"][ITERS][p]
        er, et = _pose_error(r["pose"], _pose_gt(c["motions"][p]))
        print("restatement pose of pair %d: rotation %.3g deg, translation %.3g deg" % (p, er, et))
        assert er <= 1e-3 and et <= 1e-3
        assert np.array_equal(r["mask"], c["planted"][p])
    # 0.5 px noise, or (FORWARD) outliers near the epipole that fit every E: a loose sanity bound
    for p in (NOISY, BIG, PLANAR, FORWARD):
        er, et = _pose_error(c["ref"][ITERS][p]["pose"], _pose_gt(c["motions"][p]))
        print("restatement pose of noisy pair %d: rotation %.3g deg, translation %.3g deg"
              % (p, er, et))
        assert er <= 1.0 and et <= 10.0


def test_fixture_preconditions():
    _preconditions(_reference())


def _check_unit_and_sign(E):
    e = E.reshape(-1)
    assert abs(np.sqrt((e ** 2).sum()) - 1.0) <= 1e-14
    assert e[int(np.argmax(np.abs(e)))] > 0


def _self_noise(c, p, iters):
    """the restatement against itself on pair p with other roundings: (Sampson
    difference on the planted points in px, largest difference of a pose entry)"""
    key = ("noise", p, iters)
    if key not in c:
        r, m = c["ref"][iters][p], c["rows"][p]
        Es, smp = c["samples"][p][0], c["samples"][p][1]
        E0 = Es[r["best_iter"]][r["root"]].reshape(-1)
        again = np.array(ER.solve5(m[smp[r["best_iter"]][::-1]])).reshape(-1, 9)
        d = np.minimum(np.abs(again - E0).max(1), np.abs(again + E0).max(1))
        E2 = ER.unit(again[int(np.argmin(d))].reshape(3, 3))
        if r["refit_kept"]:
            E2 = ER.unit(ER.refit(m[r["mask_min"]][::-1])[0])
        pl = m[c["planted"][p]]
        scale = THR / c["thr_n"][p]
        e = float(np.abs(ER.sampson(E2, pl) - ER.sampson(r["E"], pl)).max()) * scale
        c[key] = (e, min(float(np.abs(P - r["pose"]).max()) for P in ER.decompositions(E2)))
    return c[key]


def _compare(c, E, pose, info, cheir, inl, moff, iters, npairs):
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
            assert not E[p].any() and not pose[p].any() and not rows.any()
            assert info[p].tolist() == [1, 0, -1, 0] and cheir[p].tolist() == [-1, 0]
            continue
        _check_unit_and_sign(E[p])
        m = c["rows"][p][c["planted"][p]]
        scale = THR / c["thr_n"][p]                        # normalised units -> pixels
        err = float(np.abs(ER.sampson(E[p], m) - ER.sampson(r["E"], m)).max()) * scale
        dp = float(np.abs(pose[p] - r["pose"]).max())       # entries, not angles: arccos near 1
        print("iters %d pair %d: device vs restatement %.3g px, pose entries %.3g, inliers %d "
              "(minimal %d, refit %d, kept %d, root %d), cheirality %s"   # resolves only 1e-8
              % (iters, p, err, dp, r["n_inliers"], r["n_min"], r["n_refit"], r["refit_kept"],
                 r["root"], r["cheir"]))
        ne, npose = _self_noise(c, p, iters)
        print("    the restatement against itself: %.3g px, pose entries %.3g" % (ne, npose))
        assert err <= 100 * ne + 1e-9, (p, err, ne)
        assert cheir[p].tolist() == list(r["cheir"]), (p, cheir[p], r["cheir"])
        assert dp <= 100 * npose + 1e-12, (p, dp, npose)
        R = pose[p][:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
        assert abs(np.linalg.norm(pose[p][:, 3]) - 1.0) <= 1e-14
        assert info[p, 1] == (r["n_refit"] if r["refit_kept"] else r["n_min"])


def test_essential_pairs_vs_restatement(gpu):
    c = _reference()
    _preconditions(c)
    set_off, moff, matches, counts, kp_pool, cams = _device_inputs(c, gpu)
    E, pose, info, cheir, inl = _call(gpu, kp_pool, cams, set_off, c["pairs"], matches, counts,
                                      ITERS)
    _compare(c, E, pose, info, cheir, inl, moff, ITERS, NPAIRS)
    for p in GOOD:                                         # planted is a subset of the mask
        mask = inl[moff[p]:moff[p] + SIZES[p]].astype(bool)
        assert mask[c["planted"][p]].all(), p
    for p in (EXACT, DISTORTED):                           # fp32 keypoint rounding
        er, et = _pose_error(pose[p], _pose_gt(c["motions"][p]))
        print("device pose of pair %d: rotation %.3g deg, translation %.3g deg" % (p, er, et))
        assert er <= 1e-3 and et <= 1e-3
    assert info[BORDER, 3] & 255 == 0 and info[FIVE].tolist() == [0, 5, 0, 0]
    for p in FAILING:
        assert info[p].tolist() == [1, 0, -1, 0] and not E[p].any()
        assert not inl[moff[p]:moff[p + 1]].any()
    # determinism: a second call, and the list truncated after a pair
    again = _call(gpu, kp_pool, cams, set_off, c["pairs"], matches, counts, ITERS)
    for x, y in zip((E, pose, info, cheir, inl), again):
        assert x.tobytes() == y.tobytes()
    for k in (BIG + 1, DUP + 1):
        Ek, posek, infok, cheirk, inlk = _call(gpu, kp_pool, cams, set_off, c["pairs"],
                                               matches[:moff[k]], counts[:k], ITERS, npairs=k)
        assert Ek.tobytes() == E[:k].tobytes() and posek.tobytes() == pose[:k].tobytes()
        assert np.array_equal(infok, info[:k]) and np.array_equal(cheirk, cheir[:k])
        assert np.array_equal(inlk, inl[:moff[k]])


def test_essential_pairs_partial_block(gpu):
    c = _reference()
    _preconditions(c)
    set_off, moff, matches, counts, kp_pool, cams = _device_inputs(c, gpu)
    E, pose, info, cheir, inl = _call(gpu, kp_pool, cams, set_off, c["pairs"], matches, counts, 100)
    _compare(c, E, pose, info, cheir, inl, moff, 100, NPAIRS)
    assert info[:, 2].max() < 100


def test_python_entry_points(gpu):
    """geometry.ransac_essential_pairs on a PairBatch, and find_essential"""
    from posfeat_amd import geometry, matchers
    c = _reference()
    set_off, moff, matches, counts, kp_pool, cams = _device_inputs(c, gpu)
    buf = torch.from_numpy(np.concatenate([counts, matches.reshape(-1)])).to(gpu)
    batch = matchers.PairBatch(None, set_off, c["pairs"], moff, buf)
    E, pose, info, cheir, inl = geometry.ransac_essential_pairs(kp_pool, cams, batch, iters=ITERS,
                                                                thr=THR, seed=SEED)
    assert E.dtype == torch.float64 and tuple(E.shape) == (NPAIRS, 3, 3)
    assert pose.dtype == torch.float64 and tuple(pose.shape) == (NPAIRS, 3, 4)
    assert info.dtype == torch.int32 and tuple(info.shape) == (NPAIRS, 4)
    assert cheir.dtype == torch.int32 and tuple(cheir.shape) == (NPAIRS, 2)
    assert inl.dtype == torch.uint8 and inl.shape[0] == moff[-1]
    Ec, posec, infoc, cheirc, inlc = _call(gpu, kp_pool, cams, set_off, c["pairs"], matches, counts,
                                           ITERS)
    assert E.cpu().numpy().tobytes() == Ec.tobytes() and pose.cpu().numpy().tobytes() == posec.tobytes()
    assert np.array_equal(info.cpu().numpy(), infoc) and np.array_equal(inl.cpu().numpy(), inlc)
    assert np.array_equal(cheir.cpu().numpy(), cheirc)
    # one pair, numpy in and out: pair position 0, so the EXACT pair's own result
    a, b = c["pairs"][EXACT]
    E1, pose1, mask, inf1 = geometry.find_essential(c["sets"][a], c["sets"][b], c["cams"][a],
                                                    c["cams"][b], c["ms"][EXACT], iters=ITERS,
                                                    thr=THR, seed=SEED)
    assert E1.tobytes() == Ec[EXACT].tobytes() and np.array_equal(inf1, infoc[EXACT])
    assert pose1.tobytes() == posec[EXACT].tobytes()
    assert mask.dtype == bool and np.array_equal(mask, inlc[:SIZES[EXACT]].astype(bool))
    with pytest.raises(ValueError):
        geometry.ransac_essential_pairs(kp_pool, cams, batch, iters=0)
    with pytest.raises(ValueError):
        geometry.ransac_essential_pairs(kp_pool, cams[:-1], batch)
    with pytest.raises(ValueError):
        geometry.ransac_essential_pairs(kp_pool, cams.float(), batch)


def test_verify_pair_list_essential(gpu, tmp_path):
    """the consumer: .npz features + a pair list + an intrinsics file -> verified
    matches and relative poses, equal to a direct match_pairs_device +
    ransac_essential_pairs on the same data; the other models' dict is as it was"""
    import os
    from posfeat_amd import geometry, matchers
    from posfeat_amd.evaluation import relative_pose, verification
    from test_gpu_fundamental_pairs import _feature_files
    names, _ = _feature_files(tmp_path)                    # a, b, c see one scene; d is unrelated
    pairs_file = os.path.join(str(tmp_path), "pairs.txt")
    intr = os.path.join(str(tmp_path), "intrinsics.txt")
    with open(intr, "w") as f:
        for nm in names:
            f.write("%s PINHOLE 640 480 500 500 320 240\n" % nm)
    out = os.path.join(str(tmp_path), "verified_essential.npz")
    res = verification.verify_pair_list(str(tmp_path), pairs_file, "test", model="essential",
                                        iters=256, thr=3.0, seed=7, output=out, intrinsics=intr)
    feats = [np.load(os.path.join(str(tmp_path), nm + ".test")) for nm in names]
    pool, set_off = matchers._pool([f["descriptors"] for f in feats])
    kp_pool = torch.from_numpy(np.concatenate([f["keypoints"][:, :2] for f in feats], 0)).to(gpu)
    pairs = np.asarray([[0, 1], [1, 2], [0, 3]], np.int32)
    batch = matchers.match_pairs_device(pool, set_off, pairs, "mnn", 0.95)
    cams = torch.from_numpy(np.tile(CAM, (4, 1))).to(gpu)
    E, pose, info, cheir, inl = geometry.ransac_essential_pairs(kp_pool, cams, batch, iters=256,
                                                                thr=3.0, seed=7)
    saved = np.load(out)
    assert saved["model"].tobytes() == E.cpu().numpy().tobytes()
    assert saved["pose"].tobytes() == pose.cpu().numpy().tobytes()
    assert np.array_equal(saved["info"], info.cpu().numpy())
    assert np.array_equal(saved["cheir"], cheir.cpu().numpy())
    assert np.array_equal(saved["pose"], res["pose"]) and res["pose"].shape == (3, 3, 4)
    counts, matches = batch.read()
    inl, off = inl.cpu().numpy().astype(bool), saved["match_offsets"]
    for p in range(3):
        rows = slice(int(batch.moff[p]), int(batch.moff[p]) + int(counts[p]))
        assert np.array_equal(saved["matches"][off[p]:off[p + 1]], matches[rows][inl[rows]]), p
    assert res["info"][0, 1] == 200 and res["info"][1, 1] == 200 and res["info"][2, 1] < 30
    # the planted motions: a -> b is MOTION_A, b -> c is MOTION_B after MOTION_A's inverse
    world = np.stack([np.concatenate([np.eye(3), np.zeros((3, 1))], 1),
                      np.concatenate([MOTION_A[0], MOTION_A[1][:, None]], 1),
                      np.concatenate([MOTION_B[0], MOTION_B[1][:, None]], 1)])
    rot, trans = relative_pose.relative_pose_errors(res["pose"][:2],
                                                    relative_pose.relative_poses(world, [(0, 1), (1, 2)]))
    print("verified poses: rotation", rot, "translation", trans, "degrees")
    assert rot.max() <= 1e-3 and trans.max() <= 1e-3      # fp32 keypoints, as above
    with pytest.raises(ValueError):
        verification.verify_pair_list(str(tmp_path), pairs_file, "test", model="essential")
    with pytest.raises(ValueError):
        verification.verify_pair_list(str(tmp_path), pairs_file, "test", intrinsics=intr)
    plain = verification.verify_pair_list(str(tmp_path), pairs_file, "test", iters=256, thr=3.0,
                                          seed=7)
    assert sorted(plain) == ["info", "match_offsets", "matches", "model", "n_matches", "pairs"]
