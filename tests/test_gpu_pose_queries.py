"""posfeat_ransac_pose on the GPU against the numpy restatement of its
definitions (tests/pose_ref.py): one planted list of nine queries
(tests/pose_fixture.py), one call, iters = 512 (two hypothesis blocks per
query), thr = 12.  The preconditions -- no reprojection error of a scored
candidate or refit within 1e-6 px of thr, no scored depth within 1e-9 of 0, the
smallest / largest eigenvalue of the final 6x6 normal matrix >= 1e-4 on every
kept refit -- are asserted on the restatement before the device result is
looked at, so info, the mask and the statuses are compared exactly and the kept
poses to 1e3 eps / 1e-4 = 2.2e-12 (largest entry difference of R and of t /
max(1, |t|)).  A pose that was not kept is the P3P candidate itself and is held
to ten times the deviation of posfeat_pose_solve3 on the host from the
restatement on the winning sample (with a floor of 64 eps, since on an easy
sample that deviation can be exactly 0).  Measured on an MI355X: kept poses
3.3e-14 on the main list and 3.7e-13 on the permuted one (the 4-row query, whose
normal matrix has the smallest eigenvalue ratio, 7e-4); the one pose that is
not kept (query 8, three inliers) 2.8e-15, against a bound of 1.4e-13."""
import numpy as np
import pytest
import torch

import pose_fixture as fx
import pose_ref as pr
from ransac_ref import sample as sample4

pytestmark = pytest.mark.gpu

EIG_BOUND = 1e-4
KEPT_TOL = 1e3 * np.finfo(np.float64).eps / EIG_BOUND


def _run(f, iters=fx.ITERS, thr=fx.THR, seed=fx.SEED):
    from posfeat_amd import geometry
    dev = torch.device("cuda:0")
    poses, info, inlier = geometry.ransac_pose_queries(
        torch.from_numpy(f["kp"]).to(dev), torch.from_numpy(f["cams"]).to(dev),
        torch.from_numpy(f["points"]).to(dev), torch.from_numpy(f["corr"]).to(dev), f["q_off"],
        iters=iters, thr=thr, seed=seed)
    return dict(poses=poses.cpu().numpy(), info=info.cpu().numpy(), inlier=inlier.cpu().numpy())


def _ref(f, iters=fx.ITERS, thr=fx.THR, seed=fx.SEED):
    return pr.ransac_pose(f["kp"], f["cams"], f["points"], f["corr"], f["q_off"], iters, thr, seed)


def _check_preconditions(ref):
    mg = ref["margins"]
    print("margins", mg, "eig ratios", ref["eig_ratio"])
    assert mg.get("err", np.inf) > 1e-6 and mg.get("depth", np.inf) > 1e-9
    kept = (ref["info"][:, 0] == 0) & ((ref["info"][:, 3] & 1) == 1)
    assert np.all(ref["eig_ratio"][kept] >= EIG_BOUND)


def _host_deviation(f, ref, q, seed):
    """|posfeat_pose_solve3 - restatement| on the winning sample of query q"""
    from posfeat_amd import geometry
    rows = slice(int(f["q_off"][q]), int(f["q_off"][q + 1]))
    xy, und, X = pr.gather(f["kp"], f["cams"][q], f["points"], f["corr"][rows])
    idx = sample4(seed, q, int(ref["info"][q, 2]), rows.stop - rows.start)[:3]
    m = np.concatenate([und[idx], X[idx]], 1)
    a, b = geometry.solve_p3p(m), pr.p3p(m)
    assert len(a) == len(b)
    return max(pr.pose_error(x, y) for x, y in zip(a, b))


def _compare(f, ref, got, seed=fx.SEED):
    """-> (largest deviation of a kept pose, of a pose not kept)"""
    assert np.array_equal(got["info"], ref["info"])
    assert np.array_equal(got["inlier"], ref["inlier"])
    kept_dev, other_dev = 0.0, 0.0
    for q in range(len(f["q_off"]) - 1):
        if ref["info"][q, 0] != 0:
            assert np.all(got["poses"][q] == 0.0)
            continue
        d = pr.pose_error(got["poses"][q], ref["poses"][q])
        if ref["info"][q, 3] & 1:
            kept_dev = max(kept_dev, d)
            assert d <= KEPT_TOL, (q, d)
        else:
            other_dev = max(other_dev, d)
            tol = 10.0 * max(_host_deviation(f, ref, q, seed), 64 * np.finfo(np.float64).eps)
            assert d <= tol, (q, d, tol)
    print("device deviation: kept poses %.3g, poses not kept %.3g" % (kept_dev, other_dev))
    return kept_dev, other_dev


@pytest.fixture(scope="module")
def scene():
    f = fx.build(fx.FIXTURE_SEED)
    ref = _ref(f)
    _check_preconditions(ref)
    got = _run(f)
    return f, ref, got


def test_fixture_is_what_it_is_meant_to_be(scene):
    f, ref, _ = scene
    assert [int(s) for s in ref["info"][:, 0]] == [0, 0, 0, 1, 1, 0, 1, 0, 0]
    assert tuple(ref["info"][8, [1, 3]]) == (3, 0)             # too few inliers for a refit
    for q in (3, 4, 6):
        assert tuple(ref["info"][q]) == (1, 0, -1, 0) and np.all(ref["poses"][q] == 0)
    assert (fx.ITERS + 255) // 256 == 2 and fx.SIZES[0] > 256
    assert ref["info"][0, 1] == 300 and ref["info"][2, 1] == 4 and ref["info"][7, 1] == 34
    at = int(f["q_off"][7])
    assert not ref["inlier"][at + 34:at + 40].any()            # invalid rows are never inliers


def test_outputs_against_the_restatement(scene):
    f, ref, got = scene
    _compare(f, ref, got)


def test_ground_truth(scene):
    """The exact queries recover the planted pose within what the fp32 rounding
    of their pixels allows; the noisy query's inliers are its planted half."""
    f, _, got = scene
    # An fp32 pixel below 1024 is off by at most 2^-15 = 3.1e-5 px per coordinate,
    # so the residual vector r of the planted pose has |r| <= sqrt(2 n) 3.1e-5.
    # To first order the Gauss-Newton minimum sits at delta = -(J^T J)^-1 J^T r
    # from the planted pose, |delta| <= |r| / sigma_min(J) = |r| / sqrt(lambda_min
    # (N)); delta = (omega, tau) moves an entry of R by at most |omega| and one
    # of t by at most |tau| + |omega| |t|.  A factor 2 covers the second order
    # and the distance between the minimum and where the refit stops.
    for q in (0, 2, 5, 7):
        rows = slice(int(f["q_off"][q]), int(f["q_off"][q + 1]))
        keep = f["planted"][q]
        xy, _, X = pr.gather(f["kp"], f["cams"][q], f["points"], f["corr"][rows])
        N = pr.gn_normal(f["cams"][q], f["poses"][q], X[keep], xy[keep])[0]
        delta = np.sqrt(2 * keep.sum()) * 2.0 ** -15 / np.sqrt(np.linalg.eigvalsh(N)[0])
        P, G = f["poses"][q], got["poses"][q].reshape(3, 4)
        bound = 2.0 * delta * (1.0 + np.abs(P[:, 3]).max())
        print("query", q, "pose error", pr.pose_error(G, P), "bound", bound)
        assert got["info"][q, 0] == 0 and got["info"][q, 1] == keep.sum()
        assert np.abs(G[:, :3] - P[:, :3]).max() <= bound and np.abs(G[:, 3] - P[:, 3]).max() <= bound
        assert np.array_equal(got["inlier"][rows] != 0, keep)
    # query 1: sigma = 0.5 px, so every planted row is far inside thr = 12; a
    # random pixel is an inlier only where it fell next to its point's image:
    # within thr + 1 of the planted projection (the pose moved the projections
    # by far less than a pixel), and never beyond it
    q = 1
    rows = slice(int(f["q_off"][q]), int(f["q_off"][q + 1]))
    xy, _, X = pr.gather(f["kp"], f["cams"][q], f["points"], f["corr"][rows])
    e2, z = pr.reproj(f["cams"][q], f["poses"][q], X, xy)
    flags, planted = got["inlier"][rows] != 0, f["planted"][q]
    assert flags[planted].all() and planted.sum() == 350
    assert not flags[~planted & (np.sqrt(e2) > fx.THR + 1.0)].any()
    assert flags[~planted & (np.sqrt(e2) < fx.THR - 1.0)].all()
    assert pr.pose_error(got["poses"][q], f["poses"][q]) <= 5e-3   # 0.5 px / 500 over 350 rows


def test_a_query_does_not_depend_on_the_others(scene):
    """Query 1 at index 1 of a three-query list (behind an empty query, so its
    rows start elsewhere) gives the bits it gave in the full list; a permuted
    list gives what the restatement gives for each query at its new index."""
    f, _, got = scene
    short = fx.sublist(f, [None, 1, 7])
    res = _run(short)
    rows = slice(int(f["q_off"][1]), int(f["q_off"][2]))
    assert np.array_equal(res["poses"][1].view(np.int64), got["poses"][1].view(np.int64))
    assert np.array_equal(res["info"][1], got["info"][1])
    assert np.array_equal(res["inlier"][:700], got["inlier"][rows])
    assert tuple(res["info"][0]) == (1, 0, -1, 0)
    perm = fx.sublist(f, [7, 5, 2, 3, 0])
    ref = _ref(perm)
    _check_preconditions(ref)
    _compare(perm, ref, _run(perm))
    # the same query at the same index: the same bits whatever surrounds it
    again = _run(fx.sublist(f, [0, 5, 2]))
    assert np.array_equal(again["poses"][2].view(np.int64), _run(perm)["poses"][2].view(np.int64))


@pytest.mark.parametrize("iters", [1, 65536])
def test_slot_table_extremes(scene, iters):
    """one slot and 256 slots per query, on the 4-row query"""
    f, _, _ = scene
    one = fx.sublist(f, [2])
    ref = _ref(one, iters=iters)
    _check_preconditions(ref)
    got = _run(one, iters=iters)
    _compare(one, ref, got)
    assert got["info"][0, 0] == 0 and got["info"][0, 1] == 4
