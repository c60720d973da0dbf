"""posfeat_split_tracks through its consumer on the GPU: a tiny feature
directory, verified matches with one planted wrong match that ties two tracks,
an intrinsics file and an .nvm written here -> evaluation.reconstruction
.triangulate_pair_list(split=2) -> COLMAP's text model.  Six cameras 0.45 apart
on a line; point 0 is seen in images a, b, c only and point 1 in d, e, f only;
the wrong match joins point 0's keypoint in c with point 1's in d, so the two
tracks are one component of six rows.  posfeat_triangulate keeps one of the
two points; with the split both are in the written model.  Keypoints are exact
projections rounded to fp32."""
import os

import numpy as np
import pytest

import triangulate_ref as tr

pytestmark = pytest.mark.gpu

N_PTS, NAMES = 40, ["db/a.jpg", "db/b.jpg", "db/c.jpg", "db/d.jpg", "db/e.jpg", "db/f.jpg"]
ITERS, THR, MIN_ANGLE, MAX_TRACK, SEED = 64, 4.0, 1.5, 256, 3
YAW = 2.0


def _write_scene(root):
    rs = np.random.RandomState(23)
    os.makedirs(os.path.join(root, "db"))
    cams, poses = tr.line_cameras(6, k1=-0.01, yaw=YAW)
    z = rs.uniform(4, 9, N_PTS)
    X = np.stack([1.1 + rs.uniform(-0.2, 0.2, N_PTS) * z, rs.uniform(-0.2, 0.2, N_PTS) * z, z], 1)
    X[0], X[1] = (0.5, 0.3, 6.0), (1.8, -0.4, 5.0)
    seen = np.ones((6, N_PTS), bool)
    seen[3:, 0] = False                                        # point 0: a, b, c
    seen[:3, 1] = False                                        # point 1: d, e, f
    for k, name in enumerate(NAMES):
        kp = np.zeros((N_PTS, 3), np.float32)
        kp[:, :2] = rs.uniform(20, 460, (N_PTS, 2))
        for i in np.flatnonzero(seen[k]):
            kp[i, :2] = tr.observe(cams[k], poses[k], X[i])
        with open(os.path.join(root, name + ".test"), "wb") as f:       # as extract.py writes
            np.savez(f, keypoints=kp, descriptors=np.zeros((N_PTS, 128), np.float32),
                     scores=np.ones(N_PTS, np.float32))
    pairs, matches, moff = [], [], [0]
    for k in range(5):
        m = [(i, i) for i in range(N_PTS) if seen[k, i] and seen[k + 1, i]]
        if k == 2:
            m.append((0, 1))                                   # the wrong match
        pairs.append((NAMES[k], NAMES[k + 1]))
        matches += m
        moff.append(len(matches))
    out = os.path.join(root, "verified.npz")
    np.savez(out, pairs=np.asarray(pairs), match_offsets=np.asarray(moff, np.int64),
             matches=np.asarray(matches, np.int32))
    with open(os.path.join(root, "database_intrinsics.txt"), "w") as f:
        for k in range(6):
            if cams[k, 4]:
                f.write("%s SIMPLE_RADIAL 640 480 500.0 320.0 240.0 %r\n"
                        % (NAMES[k], float(cams[k, 4])))
            else:
                f.write("%s SIMPLE_PINHOLE 640 480 500.0 320.0 240.0\n" % NAMES[k])
    with open(os.path.join(root, "model.nvm"), "w") as f:
        f.write("NVM_V3\n\n6\n")
        for k in range(6):
            a = np.deg2rad(YAW if k % 2 else -YAW)          # rot_y(a) as a quaternion
            f.write("%s 500.0 %r 0.0 %r 0.0 %r 0.0 0.0 0 0\n"
                    % (NAMES[k], float(np.cos(a / 2)), float(np.sin(a / 2)), 0.45 * k))
        f.write("\n0\n")
    return out, cams, poses, X


def _near(points, X):
    return [pid for pid, p in points.items() if np.abs(p["xyz"] - X).max() <= 1e-4 * np.abs(X).max()]


def _files(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in ("cameras.txt", "images.txt",
                                                               "points3D.txt")}


def test_split_pair_list_to_sparse_model(gpu, tmp_path):
    from posfeat_amd.evaluation import reconstruction as rc
    root = str(tmp_path)
    ver, cams, poses, X = _write_scene(root)
    args = (ver, root, "test", os.path.join(root, "database_intrinsics.txt"),
            os.path.join(root, "model.nvm"))
    kw = dict(thr=THR, min_angle=MIN_ANGLE, iters=ITERS, max_track=MAX_TRACK, seed=SEED)
    plain = rc.triangulate_pair_list(*args, **kw)
    zero = rc.triangulate_pair_list(*args, split=0, **kw)
    res = rc.triangulate_pair_list(*args, split=2, **kw)
    for name, r in (("plain", plain), ("zero", zero), ("split", res)):
        rc.write_model(r, os.path.join(root, name))

    # split = 0 is the call as it was
    assert list(zero.keys()) == list(plain.keys())
    assert "summary_unsplit" not in plain and "parent_of" not in plain
    assert _files(os.path.join(root, "zero")) == _files(os.path.join(root, "plain"))

    # without the split one of the two tied points is lost, with it both are there
    _, _, pts0 = rc.read_model(os.path.join(root, "plain"))
    cameras, images, pts = rc.read_model(os.path.join(root, "split"))
    assert len(_near(pts0, X[0])) + len(_near(pts0, X[1])) == 1
    a, b = _near(pts, X[0]), _near(pts, X[1])
    assert len(a) == 1 and len(b) == 1 and a != b
    name_id = {im["name"]: i for i, im in images.items()}
    assert sorted(i for i, _ in pts[a[0]]["track"]) == [name_id[n] for n in NAMES[:3]]
    assert sorted(i for i, _ in pts[b[0]]["track"]) == [name_id[n] for n in NAMES[3:]]
    assert len(pts) == N_PTS and len(pts0) == N_PTS - 1
    for i in range(2, N_PTS):
        assert len(_near(pts, X[i])) == 1

    # every written point reprojects within thr into every image of its track
    worst = 0.0
    for pid, p in pts.items():
        assert len(p["track"]) >= 2
        for image_id, idx in p["track"]:
            k = NAMES.index(images[image_id]["name"])
            assert images[image_id]["point3D_ids"][idx] == pid
            e2, zc = tr.reproj2(cams[k], poses[k], p["xyz"], images[image_id]["xys"][idx])
            assert zc > 0 and e2 <= THR ** 2
            worst = max(worst, float(np.sqrt(e2)))
    print("largest reprojection error of a written observation %.3g px" % worst)

    # the summary says what the split added
    s, u = res["summary"], res["summary_unsplit"]
    assert (u["points"], u["observations"]) == (N_PTS - 1, 6 * (N_PTS - 2) + 3)
    assert (s["points"], s["observations"]) == (N_PTS, 6 * (N_PTS - 2) + 6)
    assert res["counts_unsplit"][0] == N_PTS - 1 and res["counts"][0] == N_PTS
    assert tuple(res["counts"][[4, 6, 7]]) == (0, 1, 1)
    assert sorted(res["generation"].tolist()) == [0] * (N_PTS - 1) + [1]

    # split then refine: the result goes through the refinement as it is
    both = rc.triangulate_pair_list(*args, split=2, refine=3, **kw)
    assert both["summary"]["points"] == N_PTS and both["summary_unsplit"]["points"] == N_PTS - 1
    assert both["counts_unrefined"][6] == 1 and both["counts_unsplit"][0] == N_PTS - 1
