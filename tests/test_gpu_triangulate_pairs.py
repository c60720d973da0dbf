"""The consumer of posfeat_triangulate end to end on the GPU: a tiny feature
directory, a pair list, an intrinsics file and an .nvm written here ->
evaluation.verification.verify_pair_list -> evaluation.reconstruction
.triangulate_pair_list -> COLMAP's text model.  Six images hold the same 300
random unit 128-d descriptors in their own row order, so the mutual-NN matches
are the planted ones; five are cameras 0.45 apart on a line looking at one
scene (keypoints with 0.3 px noise), the sixth has features but no pose."""
import os

import numpy as np
import pytest

import triangulate_ref as tr

pytestmark = pytest.mark.gpu

N_PTS, NAMES = 300, ["db/a.jpg", "db/b.jpg", "db/c.jpg", "db/d.jpg", "db/e.jpg", "db/f.jpg"]
PAIRS = [(0, 1), (1, 2), (2, 3), (0, 2), (3, 4), (0, 5), (1, 3)]
ITERS, THR, MIN_ANGLE, MAX_TRACK, SEED = 64, 4.0, 1.5, 256, 3
YAW = 2.0


def _write_scene(root):
    rs = np.random.RandomState(17)
    os.makedirs(os.path.join(root, "db"))
    base = rs.randn(N_PTS, 128).astype(np.float32)
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    cams, poses = tr.line_cameras(5, k1=-0.01, yaw=YAW)
    z = rs.uniform(4, 9, N_PTS)
    X = np.stack([0.9 + rs.uniform(-0.25, 0.25, N_PTS) * z, rs.uniform(-0.2, 0.2, N_PTS) * z, z], 1)
    perms = []
    for k, name in enumerate(NAMES):
        perm = rs.permutation(N_PTS)
        perms.append(perm)
        kp = np.zeros((N_PTS, 3), np.float32)
        if k < 5:
            xy = np.array([tr.project(cams[k], poses[k], p)[:2] for p in X])
            kp[perm, :2] = (xy + rs.normal(0, 0.3, xy.shape)).astype(np.float32)
        else:
            kp[:, :2] = rs.uniform(20, 460, (N_PTS, 2)).astype(np.float32)
        desc = np.zeros((N_PTS, 128), np.float32)
        desc[perm] = base
        with open(os.path.join(root, name + ".test"), "wb") as f:       # as extract.py writes
            np.savez(f, keypoints=kp, descriptors=desc, scores=np.ones(N_PTS, np.float32))
    with open(os.path.join(root, "pairs.txt"), "w") as f:
        f.write("".join("%s %s\n" % (NAMES[a], NAMES[b]) for a, b in PAIRS))
    with open(os.path.join(root, "database_intrinsics.txt"), "w") as f:
        for k in range(5):
            if cams[k, 4]:
                f.write("%s SIMPLE_RADIAL 640 480 500.0 320.0 240.0 %r\n"
                        % (NAMES[k], float(cams[k, 4])))
            else:
                f.write("%s SIMPLE_PINHOLE 640 480 500.0 320.0 240.0\n" % NAMES[k])
        f.write("%s SIMPLE_PINHOLE 640 480 500.0 320.0 240.0\n" % NAMES[5])   # intrinsics, no pose
    with open(os.path.join(root, "model.nvm"), "w") as f:
        f.write("NVM_V3\n\n5\n")
        for k in range(5):
            a = np.deg2rad(YAW if k % 2 else -YAW)          # rot_y(a) as a quaternion
            f.write("%s 500.0 %r 0.0 %r 0.0 %r 0.0 0.0 0 0\n"
                    % (NAMES[k], float(np.cos(a / 2)), float(np.sin(a / 2)), 0.45 * k))
        f.write("\n0\n")
    return cams, poses, X, perms


def test_pair_list_to_sparse_model(gpu, tmp_path):
    from posfeat_amd.evaluation import reconstruction as rc, verification
    root = str(tmp_path)
    cams, poses, X, perms = _write_scene(root)
    out = os.path.join(root, "verified.npz")
    ver = verification.verify_pair_list(root, os.path.join(root, "pairs.txt"), "test", seed=7,
                                        output=out)
    assert np.all(ver["info"][[0, 1, 2, 3, 4, 6], 1] >= 250)  # the true motions verify
    res = rc.triangulate_pair_list(out, root, "test", os.path.join(root, "database_intrinsics.txt"),
                                   os.path.join(root, "model.nvm"), thr=THR, min_angle=MIN_ANGLE,
                                   iters=ITERS, max_track=MAX_TRACK, seed=SEED)
    assert res["images"] == NAMES[:5] and res["skipped_pairs"] == 1
    assert np.allclose(res["poses"], poses, atol=1e-15) and np.array_equal(res["cams"], cams)

    # the restatement on the same verified matches
    set_off = np.arange(6, dtype=np.int32) * N_PTS
    edges = []
    for p, (a, b) in enumerate(PAIRS):
        if a < 5 and b < 5:
            m = ver["matches"][ver["match_offsets"][p]:ver["match_offsets"][p + 1]]
            edges.append(np.stack([set_off[a] + m[:, 0], set_off[b] + m[:, 1]], 1))
    edges = np.concatenate(edges, 0)
    ref = tr.triangulate(res["keypoints"], set_off, res["cams"], res["poses"], edges, ITERS, THR,
                         MIN_ANGLE, MAX_TRACK, SEED)
    mg = ref["margins"]
    print("margins", mg, "summary", res["summary"])
    assert mg["err"] > 1e-6 and mg["depth"] > 1e-9 and mg["cos"] > 1e-9
    want, got = tr.summary(ref), res["summary"]
    assert got["points"] == want["points"] >= 280
    assert got["observations"] == want["observations"] >= 5 * 250
    assert got["mean_track_length"] == want["mean_track_length"]
    assert abs(got["mean_reprojection_error"] - want["mean_reprojection_error"]) <= \
        1e-9 * want["mean_reprojection_error"]
    assert 0.1 < got["mean_reprojection_error"] < 1.0          # 0.3 px noise per coordinate
    for k in ("counts", "track_rows", "obs_inlier", "tinfo", "point_of_row"):
        assert np.array_equal(res[k], ref[k]), k

    # the written model, read back: every point reprojects within thr in every
    # image of its track, and is the planted point
    rc.write_model(res, os.path.join(root, "sparse"))
    cameras, images, points = rc.read_model(os.path.join(root, "sparse"))
    assert len(points) == got["points"] and len(images) == 5 and len(cameras) == 5
    assert sum(len(p["track"]) for p in points.values()) == got["observations"]
    inv = [np.argsort(p) for p in perms]                       # row -> planted point
    worst = 0.0
    for pid, pt in points.items():
        assert len(pt["track"]) >= 2
        planted = set()
        for image_id, idx in pt["track"]:
            im = images[image_id]
            cam = rc.camera_row(*[cameras[im["camera_id"]][i] for i in (0, 3)])
            e2, zd = tr.reproj2(cam, rc.pose_row(im["qvec"], im["tvec"]), pt["xyz"], im["xys"][idx])
            assert zd > 0 and np.sqrt(e2) <= THR
            assert im["point3D_ids"][idx] == pid
            worst = max(worst, float(np.sqrt(e2)))
            planted.add(int(inv[NAMES.index(im["name"])][idx]))
        assert len(planted) == 1                               # one planted point per track
        Xp = X[planted.pop()]
        # two views 0.45 apart at depth 9 with 3 sigma sqrt 2 = 1.3 px of disparity
        # noise: 81 / (500 x 0.45) x 1.3 = 0.47, 5 % of the depth; longer tracks do better
        assert np.abs(pt["xyz"] - Xp).max() <= 0.05 * Xp[2]
    print("largest reprojection error in the written model %.3f px" % worst)
