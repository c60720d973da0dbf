"""posfeat_ransac_homography on the GPU against the numpy restatement of its
definitions (tests/ransac_ref.py): one pair list, one call.  Synthetic matches
under known homographies with a mild perspective at 640 x 480, iters = 256,
thr = 3.  The fixture comes from fixed numpy seeds; its preconditions -- (a)
every non-degenerate pair has an all-inlier, non-rejected sample among the 256,
(b) no residual of any match under any non-rejected hypothesis (or the refit)
of the restatement lies within 1e-6 px of thr -- are asserted on the
restatement before the device result is looked at, so counts and masks are
compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

import ransac_ref as R

pytestmark = pytest.mark.gpu

W, HT = 640, 480
ITERS, THR, SEED = 256, 3.0, 2024
H_GT = np.array([[1.05, 0.04, 12.0], [-0.03, 0.97, 8.0], [4e-5, -3e-5, 1.0]])
H_B = np.array([[0.95, -0.05, 30.0], [0.04, 1.03, -10.0], [-3e-5, 5e-5, 1.0]])
GUARD = 64

# pair positions in the list
EXACT, NOISY, BIG, FOUR, THREE, EMPTY, LINE, DUP, SHARE1, SHARE2, BORDER = range(11)
GOOD = (EXACT, NOISY, BIG, FOUR, DUP, SHARE1, SHARE2, BORDER)
NPAIRS = 11
FAILING = (THREE, EMPTY, LINE)


def _kp(rs, n):
    return (rs.uniform(0, 1, (n, 2)) * [W - 40, HT - 40] + 20).astype(np.float32)


def _targets(rs, H, src, n_in, sigma):
    """targets of src [n, 2] under H: n_in planted inliers (Gaussian noise
    sigma), the rest displaced by 30..300 px; returns (targets fp32, planted)"""
    n = src.shape[0]
    planted = np.zeros(n, bool)
    planted[rs.permutation(n)[:n_in]] = True
    t = R.warp(H, src.astype(np.float64))
    t[planted] += sigma * rs.randn(n_in, 2)
    ang, mag = rs.uniform(0, 2 * np.pi, n - n_in), rs.uniform(30, 300, n - n_in)
    t[~planted] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
    return t.astype(np.float32), planted


def _fixture():
    """sets (keypoint arrays), pairs, per-pair matches [m, 2], planted masks"""
    rs = np.random.RandomState(11)
    sets, pairs, ms, planted = [], [], [], []

    def add(kp1, n2, ia, tgt, pl, s1=None):
        kp2 = _kp(rs, n2)
        ib = rs.permutation(n2)[:len(ia)]
        kp2[ib] = tgt
        if s1 is None:
            sets.append(kp1)
            s1 = len(sets) - 1
        sets.append(kp2)
        pairs.append((s1, len(sets) - 1))
        ms.append(np.stack([ia, ib], 1).astype(np.int32).reshape(-1, 2))
        planted.append(pl)
        return s1

    def plain(n, n_in, sigma, H=H_GT, extra=13, kp1=None, s1=None):
        kp1 = _kp(rs, n + extra) if kp1 is None else kp1
        ia = np.sort(rs.permutation(kp1.shape[0])[:n])
        tgt, pl = _targets(rs, H, kp1[ia], n_in, sigma)
        return add(kp1, n + extra + 5, ia, tgt, pl, s1)

    plain(300, 150, 0.0)                                   # EXACT
    plain(300, 150, 0.5)                                   # NOISY
    plain(2049, 615, 0.5)                                  # BIG: 30 % of 2049
    kp4 = np.array([[100, 100], [500, 120], [480, 400], [120, 380], [7, 9]], np.float32)
    add(kp4, 9, np.arange(4), R.warp(H_GT, kp4[:4].astype(np.float64)).astype(np.float32),
        np.ones(4, bool))                                  # FOUR
    plain(3, 3, 0.0)                                       # THREE
    sets += [_kp(rs, 50), _kp(rs, 40)]                     # EMPTY: 50 rows, no match
    pairs.append((len(sets) - 2, len(sets) - 1))
    ms.append(np.zeros((0, 2), np.int32))
    planted.append(np.zeros(0, bool))
    kpl = _kp(rs, 230)                                     # LINE: image-1 points on y = 100
    kpl[:, 1] = 100.0
    ia = np.sort(rs.permutation(230)[:200])
    add(kpl, 240, ia, R.warp(H_GT, kpl[ia].astype(np.float64)).astype(np.float32),
        np.ones(200, bool))
    kpd = _kp(rs, 320)                                     # DUP: 150 matches, each twice
    ia = np.sort(rs.permutation(320)[:150])
    tgt, pl = _targets(rs, H_GT, kpd[ia], 75, 0.5)
    kp2 = _kp(rs, 200)
    ib = rs.permutation(200)[:150]
    kp2[ib] = tgt
    sets += [kpd, kp2]
    pairs.append((len(sets) - 2, len(sets) - 1))
    ms.append(np.repeat(np.stack([ia, ib], 1).astype(np.int32), 2, axis=0))
    planted.append(np.repeat(pl, 2))
    kps = _kp(rs, 140)                                     # SHARE1 / SHARE2: one image-1 set
    s1 = plain(120, 60, 0.5, kp1=kps)
    plain(120, 60, 0.5, H=H_B, kp1=kps, s1=s1)
    # BORDER: 80 exact inliers, 20 more 2.98 px off the truth in random directions
    # (inliers of the exact H that a least-squares refit pushes past thr), 100
    # outliers: the pair whose refit is NOT kept
    rs = np.random.RandomState(701)
    kpb = _kp(rs, 213)
    ia = np.sort(rs.permutation(213)[:200])
    tgt, pl = _targets(rs, H_GT, kpb[ia], 100, 0.0)
    edge = np.flatnonzero(pl)[:20]
    ang = rs.uniform(0, 2 * np.pi, 20)
    tgt[edge] = (R.warp(H_GT, kpb[ia][edge].astype(np.float64)) +
                 2.98 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(np.float32)
    add(kpb, 218, ia, tgt, pl)
    return sets, np.asarray(pairs, np.int32), ms, planted


def _rows(sets, pairs, ms, p):
    """the (x1 y1 x2 y2) rows of pair p, as the device gathers them"""
    a, b = pairs[p]
    return np.concatenate([sets[a][ms[p][:, 0]], sets[b][ms[p][:, 1]]], 1)


_CACHE = {}


def _reference():
    """fixture + restatement (256 hypotheses per pair, finished at 256 and at
    100 iterations), computed once for the module"""
    if not _CACHE:
        sets, pairs, ms, planted = _fixture()
        ref = {ITERS: [], 100: []}
        samples = []
        for p in range(len(pairs)):
            m = _rows(sets, pairs, ms, p)
            nm, Hs, smp = R.hypotheses(m, p, ITERS, SEED)
            samples.append((Hs, smp))
            for iters in ref:
                ref[iters].append(R.finish(m, nm, Hs[:iters], THR))
        _CACHE.update(sets=sets, pairs=pairs, ms=ms, planted=planted, ref=ref, samples=samples)
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
    """the C ABI on the first npairs pairs with guarded outputs: asserts the
    guards, matches and counts are untouched; returns host (H, info, inlier)"""
    from posfeat_amd._lib import check, lib, ptr, stream_ptr
    npairs = len(pairs) if npairs is None else npairs
    pairs = np.ascontiguousarray(pairs[:npairs])
    n1 = (set_off[1:] - set_off[:-1])[pairs[:, 0]]
    total = int(n1.sum())
    so, pp = ctypes.c_void_p(set_off.ctypes.data), ctypes.c_void_p(pairs.ctypes.data)
    need = lib().posfeat_ransac_homography_workspace(so, len(set_off) - 1, pp, npairs, iters)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    md, cd = torch.from_numpy(matches).to(dev), torch.from_numpy(counts).to(dev)
    H = torch.full((npairs * 9 + GUARD,), 7.5, dtype=torch.float64, device=dev)
    info = torch.full((npairs * 4 + GUARD,), -77, dtype=torch.int32, device=dev)
    inl = torch.full((total + GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    check(lib().posfeat_ransac_homography(ptr(kp_pool), so, len(set_off) - 1, pp, npairs, ptr(md),
                                          ptr(cd), iters, THR, SEED, ptr(H), ptr(info), ptr(inl),
                                          ptr(ws), need, stream_ptr(dev)))
    torch.cuda.synchronize()
    H, info, inl = H.cpu().numpy(), info.cpu().numpy(), inl.cpu().numpy()
    assert (H[npairs * 9:] == 7.5).all() and (info[npairs * 4:] == -77).all()
    assert (inl[total:] == 0xAB).all(), "inlier rows beyond sum n1 were written"
    assert np.array_equal(md.cpu().numpy(), matches) and np.array_equal(cd.cpu().numpy(), counts)
    return H[:npairs * 9].reshape(npairs, 3, 3), info[:npairs * 4].reshape(npairs, 4), inl[:total]


def _preconditions(c):
    """asserted on the restatement before any device result is looked at"""
    assert len(c["pairs"]) == NPAIRS
    assert [len(m) for m in c["ms"]] == [300, 300, 2049, 4, 3, 0, 200, 300, 120, 120, 200]
    assert c["pairs"][SHARE1][0] == c["pairs"][SHARE2][0]
    for p in GOOD:
        Hs, smp = c["samples"][p]
        pl = c["planted"][p]
        clean = [it for it in range(ITERS) if Hs[it] is not None and pl[smp[it]].all()]
        print("pair %d: %d all-inlier non-rejected samples, margin %.3g px (256) %.3g px (100)"
              % (p, len(clean), c["ref"][ITERS][p]["margin"], c["ref"][100][p]["margin"]))
        assert clean, "precondition (a) fails for pair %d" % p
    for iters in (ITERS, 100):
        for p in range(NPAIRS):
            assert c["ref"][iters][p]["margin"] > 1e-6, "precondition (b) fails for pair %d" % p
    for p in FAILING:
        assert c["ref"][ITERS][p]["status"] == 1
    b = c["ref"][ITERS][BORDER]                            # both outcomes of the refit occur
    assert b["refit_kept"] == 0 and b["n_refit"] < b["n_min"] == 100
    assert all(c["ref"][ITERS][p]["refit_kept"] == 1 for p in GOOD if p != BORDER)
    # the restatement's H against the truth on the exact pair (fp32 keypoints)
    e = c["ref"][ITERS][EXACT]
    err = R.corner_error(e["H"], H_GT, W, HT)
    print("restatement vs H_gt on the exact pair: %.3g px" % err)
    assert err <= 1e-3
    assert e["n_inliers"] == 150 and np.array_equal(e["mask"], c["planted"][EXACT])


def test_fixture_preconditions():
    _preconditions(_reference())


def _compare(c, H, info, inl, moff, iters, npairs):
    ref = c["ref"][iters]
    for p in range(npairs):
        r, n = ref[p], len(c["ms"][p])
        n1 = moff[p + 1] - moff[p]
        rows = inl[moff[p]:moff[p] + n1]
        assert info[p, 0] == r["status"] and info[p, 1] == r["n_inliers"], (p, info[p], r)
        assert info[p, 2] == r["best_iter"] and info[p, 3] == r["refit_kept"], (p, info[p], r)
        assert np.array_equal(rows[:n], r["mask"].astype(np.uint8)), p
        assert not rows[n:].any(), "rows past counts[p] must be 0 (pair %d)" % p
        if r["status"] == 1:
            assert not H[p].any() and not rows.any() and info[p].tolist() == [1, 0, -1, 0]
            continue
        assert abs(np.sqrt((H[p] ** 2).sum()) - 1.0) <= 1e-14 and H[p, 2, 2] >= 0
        err = R.corner_error(H[p], r["H"], W, HT)
        print("iters %d pair %d: cond(normal equations) %.3g, device vs restatement %.3g px, "
              "inliers %d (minimal %d, refit %d, kept %d)"
              % (iters, p, r["cond"], err, r["n_inliers"], r["n_min"], r["n_refit"],
                 r["refit_kept"]))
        assert err <= 1e-6, (p, err)
        if info[p, 3] == 1:
            assert r["n_refit"] >= r["n_min"] and info[p, 1] == r["n_refit"]
        else:
            assert info[p, 1] == r["n_min"]


def test_ransac_pairs_vs_restatement(gpu):
    c = _reference()
    _preconditions(c)
    set_off, moff, matches, counts, kp_pool = _device_inputs(c, gpu)
    H, info, inl = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, ITERS)
    _compare(c, H, info, inl, moff, ITERS, NPAIRS)
    # the exact pair: the planted mask
    assert info[EXACT, 1] == 150
    assert info[BORDER].tolist()[1:] == [100, c["ref"][ITERS][BORDER]["best_iter"], 0]
    assert np.array_equal(inl[moff[EXACT]:moff[EXACT] + 300].astype(bool), c["planted"][EXACT])
    for p in FAILING:
        assert info[p].tolist() == [1, 0, -1, 0] and not H[p].any()
        assert not inl[moff[p]:moff[p + 1]].any()
    # determinism: a second call, and the list truncated after a pair
    H2, info2, inl2 = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, ITERS)
    assert H.tobytes() == H2.tobytes() and np.array_equal(info, info2)
    assert np.array_equal(inl, inl2)
    for k in (BIG + 1, DUP + 1):
        Hk, infok, inlk = _call(gpu, kp_pool, set_off, c["pairs"], matches[:moff[k]], counts[:k],
                                ITERS, npairs=k)
        assert Hk.tobytes() == H[:k].tobytes() and np.array_equal(infok, info[:k])
        assert np.array_equal(inlk, inl[:moff[k]])


def test_ransac_pairs_iters_not_a_multiple_of_the_wave(gpu):
    c = _reference()
    _preconditions(c)
    set_off, moff, matches, counts, kp_pool = _device_inputs(c, gpu)
    H, info, inl = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, 100)
    _compare(c, H, info, inl, moff, 100, NPAIRS)
    assert info[:, 2].max() < 100


def test_python_entry_points(gpu):
    """geometry.ransac_homography_pairs on a PairBatch, and find_homography"""
    from posfeat_amd import geometry, matchers
    c = _reference()
    set_off, moff, matches, counts, kp_pool = _device_inputs(c, gpu)
    buf = torch.from_numpy(np.concatenate([counts, matches.reshape(-1)])).to(gpu)
    batch = matchers.PairBatch(None, set_off, c["pairs"], moff, buf)
    H, info, inl = geometry.ransac_homography_pairs(kp_pool, batch, iters=ITERS, thr=THR,
                                                    seed=SEED)
    assert H.dtype == torch.float64 and tuple(H.shape) == (NPAIRS, 3, 3)
    assert info.dtype == torch.int32 and tuple(info.shape) == (NPAIRS, 4)
    assert inl.dtype == torch.uint8 and inl.shape[0] == moff[-1]
    Hc, infoc, inlc = _call(gpu, kp_pool, set_off, c["pairs"], matches, counts, ITERS)
    assert H.cpu().numpy().tobytes() == Hc.tobytes()
    assert np.array_equal(info.cpu().numpy(), infoc) and np.array_equal(inl.cpu().numpy(), inlc)
    # one pair, numpy in and out: pair position 0, so the EXACT pair's own result
    a, b = c["pairs"][EXACT]
    H1, mask, inf1 = geometry.find_homography(c["sets"][a], c["sets"][b], c["ms"][EXACT],
                                              iters=ITERS, thr=THR, seed=SEED)
    assert H1.tobytes() == Hc[EXACT].tobytes() and np.array_equal(inf1, infoc[EXACT])
    assert mask.dtype == bool and np.array_equal(mask, c["planted"][EXACT])
    with pytest.raises(ValueError):
        geometry.ransac_homography_pairs(kp_pool, batch, iters=0)
