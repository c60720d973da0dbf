"""The consumer of posfeat_ransac_pose end to end on the GPU: a tiny feature
directory, a pair list, the two intrinsics files and an .nvm written here ->
evaluation.verification.verify_pair_list -> evaluation.reconstruction
.triangulate_pair_list -> write_model -> evaluation.localization
.register_query_list -> write_predictions.  Eight images: five posed database
cameras 0.45 apart on a line and two queries with planted poses hold the same
300 random unit 128-d descriptors in their own row order (so the mutual-NN
matches are the planted ones; keypoints with 0.3 px noise); a third query has
its own random descriptors and random keypoints, so its matches are junk."""
import os

import numpy as np
import pytest

import pose_ref as pr
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

N_PTS, YAW = 300, 2.0
DB = ["db/a.jpg", "db/b.jpg", "db/c.jpg", "db/d.jpg", "db/e.jpg"]
QUERIES = ["query/night/q1.jpg", "query/night/q2.jpg", "query/night/q3.jpg"]
NAMES = DB + QUERIES
PAIRS = [(0, 1), (1, 2), (2, 3), (0, 2), (3, 4), (1, 3),
         (5, 0), (5, 2), (3, 5), (6, 1), (6, 4), (7, 0), (7, 2)]
ITERS, THR, SEED = 256, 12.0, 5


def _query_cameras():
    cams = np.array([[500.0, 500.0, 320.0, 240.0, 0.0, 0, 0, 0],
                     [500.0, 500.0, 320.0, 240.0, -0.01, 0, 0, 0]])
    poses = []
    for yaw, C in ((3.0, [0.7, 0.1, -0.3]), (-4.0, [1.2, -0.15, 0.2])):
        R = tr.rot_y(yaw)
        poses.append(np.concatenate([R, (-R @ np.asarray(C))[:, None]], 1).reshape(-1))
    return cams, np.asarray(poses)


def _write_scene(root):
    rs = np.random.RandomState(23)
    for d in ("db", "query/night"):
        os.makedirs(os.path.join(root, d))
    base = rs.randn(N_PTS, 128).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    cams, poses = tr.line_cameras(5, k1=-0.01, yaw=YAW)
    qcams, qposes = _query_cameras()
    cams, poses = np.concatenate([cams, qcams]), np.concatenate([poses, qposes])
    z = rs.uniform(4, 9, N_PTS)
    X = np.stack([0.9 + rs.uniform(-0.25, 0.25, N_PTS) * z, rs.uniform(-0.2, 0.2, N_PTS) * z, z], 1)
    for k, name in enumerate(NAMES):
        perm = rs.permutation(N_PTS)
        kp = np.zeros((N_PTS, 3), np.float32)
        desc = np.zeros((N_PTS, 128), np.float32)
        if k < 7:
            xy = np.array([tr.project(cams[k], poses[k], p)[:2] for p in X])
            kp[perm, :2] = (xy + rs.normal(0, 0.3, xy.shape)).astype(np.float32)
            desc[perm] = base
        else:
            kp[:, :2] = rs.uniform(20, 460, (N_PTS, 2)).astype(np.float32)
            desc = rs.randn(N_PTS, 128).astype(np.float32)
            desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        with open(os.path.join(root, name + ".test"), "wb") as f:       # as extract.py writes
            np.savez(f, keypoints=kp, descriptors=desc, scores=np.ones(N_PTS, np.float32))
    with open(os.path.join(root, "pairs.txt"), "w") as f:
        f.write("".join("%s %s\n" % (NAMES[a], NAMES[b]) for a, b in PAIRS))

    def intrinsics_line(name, cam):
        if cam[4]:
            return "%s SIMPLE_RADIAL 640 480 500.0 320.0 240.0 %r\n" % (name, float(cam[4]))
        return "%s SIMPLE_PINHOLE 640 480 500.0 320.0 240.0\n" % name
    with open(os.path.join(root, "database_intrinsics.txt"), "w") as f:
        f.write("".join(intrinsics_line(NAMES[k], cams[k]) for k in range(5)))
    with open(os.path.join(root, "queries_with_intrinsics.txt"), "w") as f:
        f.write("".join(intrinsics_line(NAMES[k], cams[min(k, 6)]) for k in (6, 5, 7)))
    with open(os.path.join(root, "model.nvm"), "w") as f:
        f.write("NVM_V3\n\n5\n")
        for k in range(5):
            a = np.deg2rad(YAW if k % 2 else -YAW)          # rot_y(a) as a quaternion
            f.write("%s 500.0 %r 0.0 %r 0.0 %r 0.0 0.0 0 0\n"
                    % (NAMES[k], float(np.cos(a / 2)), float(np.sin(a / 2)), 0.45 * k))
        f.write("\n0\n")
    return cams, poses, X


def test_pair_list_to_query_poses(gpu, tmp_path):
    from posfeat_amd.evaluation import localization as loc, reconstruction as rc, verification
    root = str(tmp_path)
    cams, poses, X = _write_scene(root)
    out = os.path.join(root, "verified.npz")
    ver = verification.verify_pair_list(root, os.path.join(root, "pairs.txt"), "test", seed=7,
                                        output=out)
    assert np.all(ver["info"][:11, 1] >= 250)                  # the true motions verify
    res3d = rc.triangulate_pair_list(out, root, "test", os.path.join(root, "database_intrinsics.txt"),
                                     os.path.join(root, "model.nvm"), seed=3)
    assert res3d["images"] == DB and res3d["skipped_pairs"] == 7 and res3d["summary"]["points"] >= 280
    rc.write_model(res3d, os.path.join(root, "sparse"))
    res = loc.register_query_list(out, root, "test", os.path.join(root, "sparse"),
                                  os.path.join(root, "queries_with_intrinsics.txt"), thr=THR,
                                  iters=ITERS, seed=SEED)
    assert res["queries"] == QUERIES and res["skipped_pairs"] == 6
    print("info", res["info"].tolist(), "n_corr", res["n_corr"].tolist())
    assert res["registered"].tolist() == [True, True, False]
    assert np.all(res["n_corr"][:2] >= 280) and np.all(res["info"][:2, 1] >= 270)
    assert res["info"][2, 1] < 30                              # junk matches do not make a pose

    # the restatement on the same correspondences
    ref = pr.ransac_pose(res["keypoints"], res["cams"], res["points"], res["corr"], res["q_off"],
                         ITERS, THR, SEED)
    print("margins", ref["margins"], "eig ratios", ref["eig_ratio"])
    assert ref["margins"]["err"] > 1e-6 and ref["margins"]["depth"] > 1e-9
    assert np.array_equal(res["info"], ref["info"]) and np.array_equal(res["inlier"], ref["inlier"])

    # The planted poses.  A residual at the planted pose is the query's pixel
    # noise (0.3 px per coordinate) plus the image of the point's triangulation
    # error: across the rays that is the same 0.3 px; along them a point seen by
    # two views b >= 0.45 apart is off by z^2 / (500 b) times the disparity noise
    # 0.3 sqrt 2, which a query at most 1 from those views sees as (1 / b) 0.42
    # <= 0.95 px.  So sigma_r <= 1 px per coordinate, independent between points,
    # and the least-squares pose delta = (omega, tau) has covariance <= sigma_r^2
    # N^-1, N the 6x6 normal matrix at the planted pose: |delta| stays below 4
    # sigma_r sqrt(trace N^-1) (4 sigma).  An entry of R moves by at most
    # |omega|, the centre C = -R^T t by at most |tau| + |omega| |t|.
    for q in (0, 1):
        P = poses[5 + q].reshape(3, 4)
        rows = slice(int(res["q_off"][q]), int(res["q_off"][q + 1]))
        xy, _, Xq = pr.gather(res["keypoints"], res["cams"][q], res["points"], res["corr"][rows])
        N = pr.gn_normal(cams[5 + q], P, Xq, xy)[0]
        bound = 4.0 * 1.0 * np.sqrt(np.trace(np.linalg.inv(N)))
        G = res["poses"][q].reshape(3, 4)
        C, Cp = -G[:, :3].T @ G[:, 3], -P[:, :3].T @ P[:, 3]
        print("query", q, "rotation", np.abs(G[:, :3] - P[:, :3]).max(), "centre",
              np.abs(C - Cp).max(), "bound", bound)
        assert bound < 0.05
        assert np.abs(G[:, :3] - P[:, :3]).max() <= bound
        assert np.abs(C - Cp).max() <= bound * (1.0 + np.abs(P[:, 3]).max())
        assert np.allclose(rc.quat_to_rot(res["qvecs"][q]), G[:, :3], atol=1e-14)
        assert res["qvecs"][q][0] >= 0 and np.array_equal(res["tvecs"][q], G[:, 3])

    # the prediction file: one line per registered query, parsing back exactly
    path = os.path.join(root, "predictions.txt")
    assert loc.write_predictions(res, path) == 2
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines()]
    assert [ln[0] for ln in lines] == ["q1.jpg", "q2.jpg"] and all(len(ln) == 8 for ln in lines)
    for q, ln in enumerate(lines):
        v = np.array([float(x) for x in ln[1:]])
        assert np.array_equal(v[:4], res["qvecs"][q]) and np.array_equal(v[4:], res["tvecs"][q])
