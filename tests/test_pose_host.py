"""CPU checks of the absolute-pose stage (pose.hip / pose_solve.h,
posfeat_amd/evaluation/localization.py): the P3P solver on planted poses and
against an independent root finder, its rejections, the sampler, the ABI's
argument validation (no device work), the quaternion / prediction-file /
acceptance helpers, and the pure header under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import pose_fixture as fx
import pose_ref as pr
from ransac_ref import sample as sample4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planted():
    """20000 planted samples and what posfeat_pose_solve3 makes of them"""
    from posfeat_amd import geometry
    rs = np.random.RandomState(11)
    cases = [pr.planted_sample(rs) for _ in range(20000)]
    return cases, [geometry.solve_p3p(m) for m, _ in cases]


def test_p3p_recovers_planted_poses(planted):
    """Every case has 1..4 candidates, each a rotation; the planted pose is
    among them to 1e-6 in at least 99.5 % of the cases.  Measured for the
    header (Ferrari through the closed-form cubic, two Newton steps): 99.935 %
    (13 misses of 20000, all with two quartic roots within 1e-3 of each other,
    where the depth u divides by cg - v ca near 0), median error 7.9e-14."""
    cases, got = planted
    errs = []
    for (m, P), cand in zip(cases, got):
        assert 1 <= len(cand) <= 4
        for G in cand:
            R = G[:, :3]
            assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
        errs.append(min(pr.pose_error(G, P) for G in cand))
    errs = np.asarray(errs)
    share = float((errs <= 1e-6).mean())
    print("share %.5f, median error %.3g, misses %d" % (share, np.median(errs), (errs > 1e-6).sum()))
    assert share >= 0.995


def test_p3p_against_numpy_roots(planted):
    """The header's candidates against the same formulas with np.roots (the
    companion matrix's eigenvalues) as the root finder, on the first 4000 cases
    whose quartic roots (complex ones included) are at least 1e-6 apart,
    relatively: the counts agree, and the poses agree to ten times the largest
    deviation of the restatement (tests/pose_ref.py, the header's steps in
    numpy) from that np.roots version on the same cases.  Measured: restatement
    6.1e-6 (so the tolerance is 6.1e-5), header 5.3e-5; both maxima sit on
    cases whose closest roots are about 1e-6 apart, where the root itself is
    only good to the square root of the rounding error."""
    cases, got = planted
    dev_ref, dev_hdr, n = 0.0, 0.0, 0
    for (m, _), cand in list(zip(cases, got))[:4000]:
        A, _ = pr.quartic(m)
        if pr.root_separation(A) < 1e-6:
            continue
        n += 1
        want, ref = pr.p3p(m, pr.quartic_roots_numpy), pr.p3p(m)
        assert len(cand) == len(want) == len(ref)
        dev_ref = max([dev_ref] + [pr.pose_error(a, b) for a, b in zip(ref, want)])
        dev_hdr = max([dev_hdr] + [pr.pose_error(a, b) for a, b in zip(cand, want)])
    print("cases %d, restatement vs np.roots %.3g, header vs np.roots %.3g" % (n, dev_ref, dev_hdr))
    assert n >= 3900 and dev_hdr <= 10.0 * dev_ref


def test_p3p_equals_restatement(planted):
    """The header and its numpy restatement (the same steps, numpy's acos / cos
    / cbrt), case by case: the same number of candidates in the same order,
    which is what lets the GPU tests compare the winning root index exactly;
    the median difference of the poses is at rounding level.  (The largest is
    not: where two roots meet, or cg - v ca comes close to 0 and the depth u is
    a quotient of two small numbers, the two differ by up to 5.9e-5.)"""
    cases, got = planted
    diffs = []
    for (m, _), cand in list(zip(cases, got))[:1500]:
        ref = pr.p3p(m)
        assert len(ref) == len(cand)
        diffs += [pr.pose_error(a, b) for a, b in zip(cand, ref)]
    print("median difference %.3g, largest %.3g" % (np.median(diffs), np.max(diffs)))
    assert np.median(diffs) <= 1e-12


def test_p3p_rejections():
    from posfeat_amd import geometry
    rs = np.random.RandomState(5)
    m, _ = pr.planted_sample(rs)
    assert len(geometry.solve_p3p(m)) >= 1
    bad = m.copy()                                             # collinear world points
    bad[2, 2:] = bad[0, 2:] + 2.5 * (bad[1, 2:] - bad[0, 2:])
    assert len(geometry.solve_p3p(bad)) == 0 and len(pr.p3p(bad)) == 0
    bad[2, 2:] += 1e-3 * np.cross(bad[1, 2:] - bad[0, 2:], [0.3, -0.2, 0.9])   # off the line: solvable
    assert pr.rejected(bad) is False
    bad = m.copy()                                             # coincident bearings
    bad[1, :2] = bad[0, :2]
    assert len(geometry.solve_p3p(bad)) == 0 and len(pr.p3p(bad)) == 0
    bad = m.copy()                                             # one world point twice
    bad[1, 2:] = bad[0, 2:]
    assert len(geometry.solve_p3p(bad)) == 0 and len(pr.p3p(bad)) == 0
    for r, c, v in ((2, 3, np.nan), (0, 0, np.inf), (1, 4, -np.inf)):   # a non-finite entry
        bad = m.copy()
        bad[r, c] = v
        assert len(geometry.solve_p3p(bad)) == 0 and len(pr.p3p(bad)) == 0
    # a sample whose every real root has a non-positive depth: bearings and
    # points that belong to no common pose; the first such among random draws
    found = None
    for _ in range(400):
        m, _ = pr.planted_sample(rs)
        m[:, :2] = rs.uniform(-0.6, 0.6, (3, 2))               # bearings of their own
        A, (k, cb, cg, ca, b2) = pr.quartic(m)
        roots = pr.quartic_roots_numpy(A)
        if roots and pr.root_separation(A) > 1e-3 and not pr.rejected(m) and all(
                v <= 0 or ((k - 1) * v * v - 2 * k * cb * v + 1 + k) / (2 * (cg - v * ca)) <= 0
                for v in roots):
            found = m
            break
    assert found is not None
    assert len(geometry.solve_p3p(found)) == 0 and len(pr.p3p(found)) == 0
    with pytest.raises(ValueError):
        geometry.solve_p3p(np.zeros((3, 4)))


def test_sampler_first_three_draws():
    """the restatement samples with the first three draws of sample_indices,
    as drawn"""
    from posfeat_amd import geometry
    for seed, q, it, n in ((0, 0, 0, 4), (3, 1, 511, 700), (2 ** 63 + 5, 190, 65535, 8192),
                           (7, 7, 12, 5), (1, 2, 3, 2 ** 31 - 1)):
        got = geometry.sample_indices(seed, q, it, n)
        assert list(got[:3]) == sample4(seed, q, it, n)[:3]
        assert len(set(got[:3])) == 3 and all(0 <= i < n for i in got[:3])


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_argument_validation_without_a_device():
    from posfeat_amd import _lib
    L = _lib.lib()
    q_off, qo = _i32([0, 300, 300, 1000, 1004])                # query 1 is empty
    need = L.posfeat_ransac_pose_workspace(qo, 4, 512)
    assert need >= 5 * 4 + 1004 * 64 + 4 * 2 * 8
    p = ctypes.c_void_p(4096)                                  # dummy, non-null, 256-B aligned

    def call(kp=p, nkp=5000, cams=p, points=p, npoints=900, corr=p, qo=qo, nq=4, iters=512,
             thr=12.0, poses=p, info=p, inlier=p, ws=p, ws_bytes=need):
        return L.posfeat_ransac_pose(kp, nkp, cams, points, npoints, corr, qo, nq, iters, thr, 0,
                                     poses, info, inlier, ws, ws_bytes, None)

    for name in ("kp", "cams", "points", "corr", "qo", "poses", "info", "inlier", "ws"):
        assert call(**{name: None}) == -1, name                # a null pointer
    _, dec = _i32([0, 300, 299, 1000, 1004])
    _, neg = _i32([-1, 300, 300, 1000, 1004])
    _, off = _i32([1, 300, 300, 1000, 1004])
    for bad in (dec, neg, off):
        assert call(qo=bad) == -1
        assert L.posfeat_ransac_pose_workspace(bad, 4, 512) == 0
    assert call(nq=-1) == -1 and call(nkp=-1) == -1 and call(npoints=-1) == -1
    for iters in (0, -1, 65537):
        assert call(iters=iters) == -1
        assert L.posfeat_ransac_pose_workspace(qo, 4, iters) == 0
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    assert call(ws=ctypes.c_void_p(4096 + 64)) == -1           # ws not 256-B aligned
    assert call(poses=ctypes.c_void_p(4100)) == -1             # poses not 8-B aligned
    assert call(points=ctypes.c_void_p(4100)) == -1 and call(info=ctypes.c_void_p(4098)) == -1
    assert L.posfeat_ransac_pose_workspace(None, 4, 512) == 0
    # legal extremes: only the workspace is short
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert call(iters=1, ws_bytes=0) == -3 and call(iters=65536, ws_bytes=0) == -3
    assert call(thr=1e-300, ws_bytes=0) == -3 and call(thr=1e300, ws_bytes=0) == -3
    assert L.posfeat_ransac_pose_workspace(qo, 4, 65536) > L.posfeat_ransac_pose_workspace(qo, 4, 1)
    _, none = _i32([0])
    assert L.posfeat_ransac_pose_workspace(none, 0, 8) >= 256 and call(qo=none, nq=0) == 0
    assert L.posfeat_pose_solve3(None, p) == -1 and L.posfeat_pose_solve3(p, None) == -1


def test_rot_to_quat_round_trip():
    from posfeat_amd.evaluation import reconstruction as rc
    rs = np.random.RandomState(2)
    for k in range(20):
        q = rs.normal(size=4)
        if k % 5 == 0:
            q[0] = 0.0 if k % 10 == 0 else 1e-9                # half turns: qw = 0 (nearly)
        q /= np.linalg.norm(q)
        got = rc.rot_to_quat(rc.quat_to_rot(q))
        want = q if q[0] > 0 or (q[0] == 0 and got @ q > 0) else -q
        assert got[0] >= 0 and abs(np.linalg.norm(got) - 1) <= 1e-15
        assert np.abs(got - want).max() <= 1e-14, (k, got, want)
        assert np.abs(rc.quat_to_rot(got) - rc.quat_to_rot(q)).max() <= 1e-14


def test_acceptance_rule_and_prediction_file(tmp_path):
    from posfeat_amd.evaluation import localization as loc, reconstruction as rc
    info = np.array([[0, 30, 5, 1], [0, 29, 0, 1], [1, 0, -1, 0], [0, 100, 7, 257], [0, 100, 7, 0],
                     [0, 25, 1, 1]], np.int32)
    n = np.array([120, 40, 0, 400, 401, 100])
    # 30 of 120 = 0.25 passes; 29 fails the count; status 1; 100 of 400 passes, of 401 fails
    assert loc.registered_mask(info, n).tolist() == [True, False, False, True, False, False]
    assert loc.registered_mask(info, n, min_inliers=25, min_ratio=0.3).tolist() == \
        [False, True, False, False, False, False]
    q = np.array([[0.5, -0.5, 0.5, 0.5], [1, 0, 0, 0], [1, 0, 0, 0], [0.1, 0.7, -0.7, 0.1]])
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = np.array([[1.5, -2.25, 1e-17], [0, 0, 0], [0, 0, 0], [-123.456789012345, 0.1, 3e5]])
    res = dict(queries=["query/night/a.jpg", "b.jpg", "c.jpg", "query/d.jpg"],
               registered=np.array([True, False, False, True]), qvecs=q, tvecs=t)
    path = str(tmp_path / "pred.txt")
    assert loc.write_predictions(res, path) == 2
    lines = open(path).read().splitlines()
    assert [ln.split()[0] for ln in lines] == ["a.jpg", "d.jpg"]
    for ln, k in zip(lines, (0, 3)):
        v = [float(x) for x in ln.split()[1:]]
        assert len(v) == 7 and v[:4] == q[k].tolist() and v[4:] == t[k].tolist()   # repr round-trips
    # the model's pool as the registration reads it
    images = {2: dict(name="b", point3D_ids=np.array([-1, 7, 3])),
              1: dict(name="a", point3D_ids=np.array([3, -1, 9, 5]))}
    points = {3: dict(xyz=np.array([1.0, 2, 3]), track=[(1, 0), (2, 2)]),
              7: dict(xyz=np.array([4.0, 5, 6]), track=[(2, 1), (1, 1)]),
              9: dict(xyz=np.array([7.0, 8, 9]), track=[(1, 2), (2, 0), (1, 3)])}
    ids, set_off, por, pids, xyz, tinfo = loc.model_points(images, points)
    assert ids == [1, 2] and set_off.tolist() == [0, 4, 7] and pids.tolist() == [3, 7, 9]
    assert por.tolist() == [0, -1, 2, -1, -1, 1, 0]            # id 5 is not a point of the model
    assert xyz[1].tolist() == [4.0, 5, 6] and tinfo[:, 1].tolist() == [2, 2, 3]


def test_fixture_restatement():
    """the restatement itself (no device) on the planted list: statuses, counts
    and the planted poses"""
    f = fx.build(fx.FIXTURE_SEED)
    ref = pr.ransac_pose(f["kp"], f["cams"], f["points"], f["corr"], f["q_off"], fx.ITERS, fx.THR,
                         fx.SEED)
    assert ref["info"][:, 0].tolist() == [0, 0, 0, 1, 1, 0, 1, 0, 0]
    assert ref["info"][8].tolist() == [0, 3, 0, 0]
    assert ref["info"][[0, 2, 5, 7], 1].tolist() == [300, 4, 120, 34]
    for q in fx.SOLVED:
        assert pr.pose_error(ref["poses"][q], f["poses"][q]) <= (5e-3 if q == 1 else 1e-6)


def test_pose_solve_under_host_sanitizers(tmp_path):
    """tests/host/pose_solve_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "pose_solve_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "pose_solve_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "pose_solve ok" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]
