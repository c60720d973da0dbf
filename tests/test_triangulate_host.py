"""CPU checks of the triangulation stage (triangulate.hip / triangulate_solve.h,
posfeat_amd/evaluation/reconstruction.py): the DLT against the numpy
restatement (tests/triangulate_ref.py) and against an independent SVD null
space, the camera model's round trip, the ABI's argument validation (no device
work), the camera / pose helpers, the file readers and the COLMAP text model's
round trip, the pure header under the host sanitizers, and the restatement
itself on the planted scene."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import triangulate_fixture as fx
import triangulate_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def _system(rs, nviews, X):
    cams, poses = tr.line_cameras(8)
    views = rs.choice(8, nviews, replace=False)
    obs = []
    for v in views:
        px, py, _ = tr.project(cams[v], poses[v], X)
        obs.append(np.concatenate([tr.undistort(cams[v], px, py), poses[v]]))
    return np.asarray(obs)


def test_dlt_equals_restatement_and_svd():
    from posfeat_amd import geometry
    rs = np.random.RandomState(3)
    for k in range(200):
        X = np.array([rs.uniform(0.5, 2.5), rs.uniform(-0.5, 0.5), rs.uniform(3, 9)])
        obs = _system(rs, 2 + k % 7, X)
        if k % 2:                                            # a noisy system: a real least squares
            obs[:, :2] += rs.normal(0, 1e-3, obs[:, :2].shape)
        got = geometry.triangulate_dlt(obs)
        want, eig = tr.dlt(obs)
        eig = np.sort(eig)
        assert got is not None and want is not None
        # fp64 eps over the eigenvalue gap, with margin for the rotations' order
        tol = 1e3 * np.finfo(np.float64).eps * eig[-1] / (eig[1] - eig[0])
        assert np.abs(got - want).max() <= tol * np.abs(want).max(), (k, tol)
        # independent: the right singular vector of the stacked 2n x 4 system
        A = []
        for o in obs:
            P = o[2:].reshape(3, 4)
            A += [o[0] * P[2] - P[0], o[1] * P[2] - P[1]]
        v = np.linalg.svd(np.asarray(A))[2][-1]
        assert np.abs(got - v[:3] / v[3]).max() <= 1e-9 * np.abs(got).max(), k
        if k % 2 == 0:
            assert np.abs(got - X).max() <= 1e-9 * 9.0


def test_dlt_rejects_a_point_at_infinity():
    from posfeat_amd import geometry
    _, poses = tr.line_cameras(8, yaw=0.0)
    obs = np.asarray([np.concatenate([[0.1, -0.05], poses[0]]),
                      np.concatenate([[0.1, -0.05], poses[3]])])    # parallel rays
    assert geometry.triangulate_dlt(obs) is None and tr.dlt(obs)[0] is None
    obs[1, 0] = np.nan
    assert geometry.triangulate_dlt(obs) is None
    with pytest.raises(ValueError):
        geometry.triangulate_dlt(np.zeros((0, 14)))
    with pytest.raises(ValueError):
        geometry.triangulate_dlt(np.zeros((2, 13)))


@pytest.mark.parametrize("k1", [0.0, -0.06, 0.05])
def test_undistort_project_round_trip(k1):
    rs = np.random.RandomState(7)
    cam = np.array([500.0, 500.0, 320.0, 240.0, k1, 0, 0, 0])
    _, poses = tr.line_cameras(3)
    for _ in range(300):
        x, y = rs.uniform(0, 640), rs.uniform(0, 480)
        xu, yu = tr.undistort(cam, x, y)
        f = 1.0 + k1 * (xu * xu + yu * yu)
        assert abs(f * xu - (x - 320.0) / 500.0) <= 1e-12       # distorting again gives the pixel
        assert abs(f * yu - (y - 240.0) / 500.0) <= 1e-12
        # a point on that ray reprojects onto the pixel (the kernels' own camera
        # code makes the same round trip in tests/host/triangulate_check.cpp)
        d = rs.uniform(3, 9)
        P = poses[1].reshape(3, 4)
        X = P[:, :3].T @ (np.array([xu * d, yu * d, d]) - P[:, 3])
        e2, z = tr.reproj2(cam, poses[1], X, (x, y))
        assert abs(z - d) <= 1e-12 * d and np.sqrt(e2) <= 500.0 * 4e-12


def test_argument_validation_without_a_device():
    from posfeat_amd import _lib
    L = _lib.lib()
    set_off, so = _i32([0, 300, 300, 2349, 2400])              # set 1 is empty
    need = L.posfeat_triangulate_workspace(so, 4, 1000, 256)
    assert need >= 2400 * (5 * 4 + 16)
    p = ctypes.c_void_p(4096)                                  # dummy, non-null, 256-B aligned

    def call(kp=p, so=so, nsets=4, cams=p, poses=p, edges=p, nedges=1000, iters=64, thr=4.0,
             min_angle=1.5, max_track=256, points=p, err=p, tinfo=p, track_off=p, track_rows=p,
             obs_inlier=p, point_of_row=p, counts=p, ws=p, ws_bytes=need):
        return L.posfeat_triangulate(kp, so, nsets, cams, poses, edges, nedges, iters, thr,
                                     min_angle, max_track, 0, points, err, tinfo, track_off,
                                     track_rows, obs_inlier, point_of_row, counts, ws, ws_bytes,
                                     None)

    for name in ("kp", "so", "cams", "poses", "edges", "points", "err", "tinfo", "track_off",
                 "track_rows", "obs_inlier", "point_of_row", "counts", "ws"):
        assert call(**{name: None}) == -1, name                # a null pointer
    _, dec = _i32([0, 300, 299, 2349, 2400])
    _, neg = _i32([-1, 300, 300, 2349, 2400])
    _, off = _i32([1, 300, 300, 2349, 2400])
    for bad in (dec, neg, off):
        assert call(so=bad) == -1
        assert L.posfeat_triangulate_workspace(bad, 4, 1000, 256) == 0
    assert call(nsets=-1) == -1
    for iters in (7, 0, -1, 1025):
        assert call(iters=iters) == -1
    for mt in (1, 0, -5, 1025):
        assert call(max_track=mt) == -1
        assert L.posfeat_triangulate_workspace(so, 4, 1000, mt) == 0
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    for ang in (-0.1, 90.0, 180.0, float("nan"), float("inf")):
        assert call(min_angle=ang) == -1
    assert call(nedges=-1) == -1 and L.posfeat_triangulate_workspace(so, 4, -1, 256) == 0
    assert call(ws=ctypes.c_void_p(4096 + 64)) == -1           # ws not 256-B aligned
    assert L.posfeat_triangulate_workspace(None, 4, 1000, 256) == 0
    # legal extremes: only the workspace is short
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert call(iters=8, max_track=2, min_angle=0.0, ws_bytes=0) == -3
    assert call(iters=1024, max_track=1024, min_angle=89.9, ws_bytes=0) == -3
    assert L.posfeat_triangulate_dlt(None, 2, p) == -1 and L.posfeat_triangulate_dlt(p, 0, p) == -1
    assert call(points=ctypes.c_void_p(4100)) == -1 and call(err=ctypes.c_void_p(4100)) == -1


def test_camera_and_pose_helpers():
    from posfeat_amd.evaluation import reconstruction as rc
    assert rc.camera_row("SIMPLE_PINHOLE", [500, 320, 240]).tolist() == [500, 500, 320, 240, 0, 0, 0, 0]
    assert rc.camera_row("PINHOLE", [500, 510, 320, 240]).tolist() == [500, 510, 320, 240, 0, 0, 0, 0]
    assert rc.camera_row("SIMPLE_RADIAL", [500, 320, 240, -0.06]).tolist() == \
        [500, 500, 320, 240, -0.06, 0, 0, 0]
    for model, params in (("RADIAL", [500, 320, 240, 0.1, 0.0]), ("OPENCV", [1] * 8),
                          ("PINHOLE", [500, 320, 240])):
        with pytest.raises(NotImplementedError):
            rc.camera_row(model, params)
    # a quarter turn about z: x -> y
    q = [np.cos(np.pi / 4), 0.0, 0.0, np.sin(np.pi / 4)]
    P = rc.pose_row(q, [1.0, 2.0, 3.0]).reshape(3, 4)
    assert np.allclose(P[:, :3] @ [1.0, 0, 0], [0, 1.0, 0], atol=1e-15)
    assert P[:, 3].tolist() == [1.0, 2.0, 3.0]
    rs = np.random.RandomState(1)
    for _ in range(20):
        q = rs.normal(size=4)
        R = rc.quat_to_rot(3.0 * q)                            # normalised inside
        assert np.allclose(R @ R.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R) - 1) < 1e-14
        v = q[1:] / np.linalg.norm(q[1:])                      # the axis is fixed by R
        assert np.allclose(R @ v, v, atol=1e-14)


def test_readers(tmp_path):
    from posfeat_amd.evaluation import reconstruction as rc
    intr = tmp_path / "database_intrinsics.txt"
    intr.write_text("db/1.jpg SIMPLE_RADIAL 1600 1200 1469.2 800 600 -0.0353\n"
                    "db/2.jpg PINHOLE 640 480 500.0 505.0 320 240\n\n")
    got = rc.read_intrinsics(str(intr))
    assert got["db/1.jpg"] == ("SIMPLE_RADIAL", 1600, 1200, [1469.2, 800.0, 600.0, -0.0353])
    assert got["db/2.jpg"] == ("PINHOLE", 640, 480, [500.0, 505.0, 320.0, 240.0])
    q = np.array([0.9, 0.1, -0.3, 0.2])
    nvm = tmp_path / "model.nvm"
    nvm.write_text("NVM_V3\n\n2\n"
                   "db/1.jpg 1469.2 %r %r %r %r 1.5 -2.0 0.25 -0.0353 0\n"
                   "db/2.jpg 500 1 0 0 0 0.45 0 0 0 0\n\n0\n" % tuple(float(v) for v in q))
    poses = rc.read_nvm_poses(str(nvm))
    assert sorted(poses) == ["db/1.jpg", "db/2.jpg"]
    qv, t = poses["db/1.jpg"]
    R = rc.quat_to_rot(q)
    assert np.array_equal(qv, q) and np.allclose(t, -R @ [1.5, -2.0, 0.25], atol=1e-15)
    assert np.allclose(-R.T @ t, [1.5, -2.0, 0.25], atol=1e-14)    # the centre comes back
    assert poses["db/2.jpg"][1].tolist() == [-0.45, 0.0, 0.0]


def test_pair_list_edges():
    from posfeat_amd.evaluation import reconstruction as rc
    set_off = np.asarray([0, 5, 9], np.int32)
    index = {"a": 0, "b": 1}
    pairs = [("a", "b"), ("a", "q"), ("b", "a")]
    moff = [0, 2, 3, 4]
    matches = np.asarray([[0, 3], [4, 0], [1, 1], [3, 4]], np.int32)
    edges, skipped = rc.pair_list_edges(pairs, moff, matches, index, set_off)
    assert skipped == 1 and edges.dtype == np.int32
    assert edges.tolist() == [[0, 8], [4, 5], [8, 4]]
    for bad in ([[0, 4]], [[5, 0]], [[-1, 0]]):                # b has 4 keypoints, a has 5
        with pytest.raises(ValueError):
            rc.pair_list_edges([("a", "b")], [0, 1], np.asarray(bad, np.int32), index, set_off)
    edges, skipped = rc.pair_list_edges([("q", "a")], [0, 1], [[99, 99]], index, set_off)
    assert edges.shape == (0, 2) and skipped == 1              # a skipped pair is not looked at


def test_text_model_round_trip(tmp_path):
    from posfeat_amd.evaluation import reconstruction as rc
    f = fx.build(fx.FIXTURE_SEED)
    ref = tr.triangulate(f["kp"], f["set_off"], f["cams"], f["poses"], f["edges"], fx.ITERS, fx.THR,
                         fx.MIN_ANGLE, fx.MAX_TRACK, fx.SEED)
    n = len(f["set_off"]) - 1
    res = dict(ref, images=["db/%02d.jpg" % i for i in range(n)], set_off=f["set_off"],
               keypoints=f["kp"],
               models=[("SIMPLE_RADIAL", 640, 480, [500.0, 320.0, 240.0, float(c[4])]) if c[4] else
                       ("SIMPLE_PINHOLE", 640, 480, [500.0, 320.0, 240.0]) for c in f["cams"]],
               qvecs=[np.array([1.0, 0, 0, 0])] * n, tvecs=[p.reshape(3, 4)[:, 3] for p in f["poses"]])
    rc.write_model(res, str(tmp_path / "model"))
    cameras, images, points = rc.read_model(str(tmp_path / "model"))
    assert len(cameras) == n and len(images) == n
    good = np.flatnonzero((ref["tinfo"][:, 0] == 0) & (ref["tinfo"][:, 1] >= 2))
    assert sorted(points) == [int(t) + 1 for t in good]
    for i in range(n):
        im = images[i + 1]
        rows = slice(int(f["set_off"][i]), int(f["set_off"][i + 1]))
        assert im["name"] == res["images"][i] and im["camera_id"] == i + 1
        assert np.array_equal(im["xys"].astype(np.float32), f["kp"][rows])     # repr round-trips
        assert np.array_equal(im["tvec"], res["tvecs"][i])
        want = ref["point_of_row"][rows].astype(np.int64)
        want = np.where((want >= 0) & np.isin(want, good), want + 1, -1)
        assert np.array_equal(im["point3D_ids"], want)
        assert cameras[i + 1] == res["models"][i]
    for t in good:
        pt = points[int(t) + 1]
        assert np.array_equal(pt["xyz"], ref["points"][t]) and pt["error"] == ref["err"][t]
        assert len(pt["track"]) == ref["tinfo"][t, 1]
        for image_id, idx in pt["track"]:
            assert images[image_id]["point3D_ids"][idx] == t + 1


def test_triangulate_solve_under_host_sanitizers(tmp_path):
    """tests/host/triangulate_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "triangulate_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "triangulate_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "triangulate_solve ok" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]


def test_restatement_on_the_planted_scene():
    """the restatement itself (no device): exact observations recover the
    points, the 5 + 3 component keeps the 5 and flags the 3, the 0.002-baseline
    pair is rejected"""
    f = fx.build(fx.FIXTURE_SEED)
    ref = tr.triangulate(f["kp"], f["set_off"], f["cams"], f["poses"], f["edges"], fx.ITERS, fx.THR,
                         fx.MIN_ANGLE, fx.MAX_TRACK, fx.SEED)
    root = {int(ref["track_rows"][ref["track_off"][t]]): t for t in range(int(ref["counts"][0]))}
    c = f["cases"]
    # fp32 pixels are off by up to 640 x 2^-24 = 3.8e-5 px; at depth z with
    # baseline b and focal length 500 the depth moves by z^2 / (500 b) per pixel
    # of disparity: 81 / 225 x 3.8e-5 x sqrt 2 = 2e-5 at the most, 2.2e-6 of z = 9
    for case in c["two_view"] + c["chain8"]:
        t = root[min(case["rows"])]
        assert ref["tinfo"][t, 0] == 0 and ref["tinfo"][t, 1] == len(case["rows"])
        assert np.abs(ref["points"][t] - case["X"]).max() <= 2.2e-6 * np.abs(case["X"]).max()
        assert ref["err"][t] <= 1e-4
    for case in c["noisy"]:                                    # sigma = 0.5 px: all inliers
        t = root[min(case["rows"])]
        assert ref["tinfo"][t, 1] == len(case["rows"]) and 0.0 < ref["err"][t] < 2.0
    t = root[min(c["merge5"][0]["rows"] + c["merge3"][0]["rows"])]
    sl = slice(int(ref["track_off"][t]), int(ref["track_off"][t + 1]))
    rows, flags = ref["track_rows"][sl], ref["obs_inlier"][sl]
    assert set(rows[flags == 1]) == set(c["merge5"][0]["rows"])
    assert set(rows[flags == 0]) == set(c["merge3"][0]["rows"])
    assert all(ref["point_of_row"][r] == t for r in c["merge5"][0]["rows"])
    assert all(ref["point_of_row"][r] == -1 for r in c["merge3"][0]["rows"])
    t = root[min(c["low_parallax"][0]["rows"])]
    assert tuple(ref["tinfo"][t]) == (1, 0, -1, 0) and np.all(ref["points"][t] == 0)
    s = tr.summary(ref)
    assert s["points"] == ref["counts"][2] and s["observations"] == ref["counts"][3]
    assert 2.0 <= s["mean_track_length"] <= 8.0 and 0.0 < s["mean_reprojection_error"] < 1.0
    # adjacent cameras subtend 2.9 degrees at depth 9: above min_angle
    assert np.degrees(2 * np.arctan(0.225 / 9.0)) > 2.8 > fx.MIN_ANGLE
