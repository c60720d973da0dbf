"""The planted query list of the absolute-pose tests: nine queries over one
keypoint pool and one point array, each with its own planted pose (K = 500 /
320 / 240), holding every case posfeat_ransac_pose distinguishes.  Built from
fixed numpy seeds; nothing here touches the GPU.

  0  300 exact correspondences (crosses the 256-row tile)
  1  700: 350 planted with 0.5 px noise, 350 uniform-random pixels
  2  4 exact
  3  3 (too few)
  4  0
  5  150 exact through a SIMPLE_RADIAL camera, k1 = -0.06, 30 of them moved
  6  50 whose world points lie on one line
  7  40: 34 exact, 2 with a keypoint row out of range, 2 with a point index out
     of range, 2 on a NaN point
  8  6 random pixels against 6 points: the best sample has its own three rows
     for inliers, too few for a refit, so the pose is the P3P candidate itself
"""
import numpy as np

import pose_ref as pr
import triangulate_ref as tr

ITERS, THR = 512, 12.0
# Picked together so that the preconditions of the device comparison hold
# (tests/test_gpu_pose_queries.py asserts them on the restatement).
FIXTURE_SEED, SEED = 5, 3
SIZES = [300, 700, 4, 3, 0, 150, 50, 40, 6]
SOLVED = [0, 1, 2, 5, 7]


def plant(rs, n, k1=0.0, line=False):
    """a pose and n points in front of it -> (cam [8], pose [3, 4], X [n, 3],
    exact pixels [n, 2] fp64)"""
    cam = np.array([500.0, 500.0, 320.0, 240.0, k1, 0, 0, 0])
    R, C = pr.random_rotation(rs), rs.uniform(-1, 1, 3)
    t = -R @ C
    if line:                                                   # between two points of the view
        a = np.array([-0.5, -0.3, 1.0]) * 4.0
        b = np.array([0.5, 0.35, 1.0]) * 8.0
        Xc = a + rs.uniform(0, 1, n)[:, None] * (b - a)
    else:
        Xc = np.stack([rs.uniform(-0.6, 0.6, n), rs.uniform(-0.45, 0.45, n), np.ones(n)], 1) * \
            rs.uniform(3, 9, n)[:, None]
    X = (Xc - t) @ R
    pose = np.concatenate([R, t[:, None]], 1)
    px = np.array([tr.project(cam, pose.reshape(-1), x)[:2] for x in X]).reshape(-1, 2)
    return cam, pose, X, px


def build(seed=FIXTURE_SEED):
    rs = np.random.RandomState(seed)
    cams, poses, kps, pts, corr, q_off, planted = [], [], [], [], [], [0], []
    nkp = npt = 0
    for q, n in enumerate(SIZES):
        cam, pose, X, px = plant(rs, n, k1=-0.06 if q == 5 else 0.0, line=q == 6)
        good = np.ones(n, bool)
        if q == 1:
            px[:350] += rs.normal(0, 0.5, (350, 2))
            px[350:] = np.stack([rs.uniform(0, 640, 350), rs.uniform(0, 480, 350)], 1)
            good[350:] = False
        if q == 8:
            px = np.stack([rs.uniform(0, 640, n), rs.uniform(0, 480, n)], 1)
            good[:] = False
        if q == 5:
            px[120:] += rs.uniform(40, 90, (30, 2)) * rs.choice([-1, 1], (30, 2))
            good[120:] = False
        rows, pidx = nkp + np.arange(n), npt + np.arange(n)
        if q in (1, 5):                                        # the correspondences in mixed order
            order = rs.permutation(n)
            rows, pidx, good = rows[order], pidx[order], good[order]
        kps.append(px.astype(np.float32))
        pts.append(X)
        corr.append(np.stack([rows, pidx], 1))
        cams.append(cam)
        poses.append(pose)
        planted.append(good)
        nkp, npt = nkp + n, npt + n
        q_off.append(q_off[-1] + n)
    kp = np.concatenate(kps, 0)
    points = np.concatenate(pts, 0)
    corr = np.concatenate(corr, 0).astype(np.int64)
    # query 7: rows 34..39 are invalid in the three ways
    at = q_off[7]
    corr[at + 34, 0], corr[at + 35, 0] = -1, nkp
    corr[at + 36, 1], corr[at + 37, 1] = -1, npt
    points[corr[at + 38, 1]] = np.nan
    corr[at + 39, 1] = corr[at + 38, 1]
    planted[7][34:] = False
    return dict(kp=kp, cams=np.stack(cams), points=points, corr=corr.astype(np.int32),
                q_off=np.asarray(q_off, np.int32), poses=poses, planted=planted)


def sublist(f, queries):
    """the list made of the given queries of ``f``, in that order (None: an
    empty query), over the same pool and points"""
    cams, corr, q_off = [], [], [0]
    for q in queries:
        rows = slice(0, 0) if q is None else slice(int(f["q_off"][q]), int(f["q_off"][q + 1]))
        cams.append(f["cams"][0 if q is None else q])
        corr.append(f["corr"][rows])
        q_off.append(q_off[-1] + corr[-1].shape[0])
    return dict(kp=f["kp"], cams=np.stack(cams), points=f["points"],
                corr=np.concatenate(corr, 0).astype(np.int32), q_off=np.asarray(q_off, np.int32))
