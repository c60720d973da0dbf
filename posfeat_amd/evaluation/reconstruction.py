"""A sparse model from verified matches and known database poses, on the GPU:
what the reference's Aachen pipeline asks of ``colmap point_triangulator``
after ``geometric_verification`` (evaluations/aachen/reconstruct_pipeline.py),
without COLMAP.

  triangulate_pair_list(verified_npz, feature_dir, postfix, intrinsics, nvm,
                        thr=4.0, min_angle=1.5, iters=64, max_track=256, seed=0,
                        refine=0, split=0) -> dict

``verified_npz`` is what evaluation.verification.verify_pair_list wrote (pairs,
match_offsets, matches); ``intrinsics`` and ``nvm`` are the two files the
reference's preprocess_reference_model reads (database_intrinsics.txt: ``name
MODEL w h params...``; the .nvm camera block: ``name f qw qx qy qz cx cy cz
...``, t = -R c).  The images that have a pose, in sorted name order, form one
keypoint pool (a posed image without intrinsics raises); the verified matches
of the pairs between them become edges (a match index outside its image's
keypoints raises); pairs that name an image without a pose are skipped and
counted.  geometry.triangulate_tracks runs once.  With ``split`` = k > 0,
geometry.split_tracks (sequential RANSAC over each track's left-over members,
rounds = k, the same iters, thr, min_angle and seed) runs on its result on the
device, before any refinement: a track may become several, and every array
below is the split result's.  With ``refine`` = k > 0,
geometry.refine_tracks (points-only bundle adjustment, rounds = k, the same thr
and min_angle) runs on its result on the device before the one read-back, and
points, err, tinfo, obs_inlier, point_of_row and counts are the refined ones
(counts then as posfeat_refine_points defines it).  The returned dict:
  images         [n] names; image i is set i of the pool
  set_off        [n + 1] int32
  cams, poses    [n, 8], [n, 12] fp64 as posfeat_triangulate takes them
  models         [n] (MODEL, w, h, params) as read
  keypoints      [N, 2] fp32 the pool
  points, err, tinfo, track_off, track_rows, obs_inlier, point_of_row, counts
                 as TrackResult.host() gives them
  skipped_pairs  pairs naming an image without a pose
  summary        points, observations, mean_track_length,
                 mean_reprojection_error (what the reference's ETH script
                 reads from ``colmap model_analyzer``), over the points with at
                 least two inlier observations
  with refine > 0 also:
  rinfo          [T, 4] (rounds used, taken steps, converged, flags changed)
  summary_unrefined   the summary of the triangulated points before refinement
  counts_unrefined    posfeat_triangulate's counts (posfeat_split_tracks' with split > 0)
  with split > 0 also:
  parent_of, generation   [T] the track of the triangulate call a track comes
                 from, and 0 for that track itself, g for its g-th child
                 (without refine; the refined result keeps the split's order)
  summary_unsplit     the summary of the triangulated points before the split
  counts_unsplit      posfeat_triangulate's counts
write_model / read_model: COLMAP's text model (cameras.txt, images.txt,
points3D.txt).
"""
import os

import numpy as np
import torch

from .. import _lib, geometry

MODELS = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL")


def camera_row(model, params):
    """(fx, fy, cx, cy, k1, 0, 0, 0) of a COLMAP camera model and its params"""
    p = [float(v) for v in params]
    if model == "SIMPLE_PINHOLE" and len(p) == 3:
        return np.array([p[0], p[0], p[1], p[2], 0.0, 0, 0, 0])
    if model == "PINHOLE" and len(p) == 4:
        return np.array([p[0], p[1], p[2], p[3], 0.0, 0, 0, 0])
    if model == "SIMPLE_RADIAL" and len(p) == 4:
        return np.array([p[0], p[0], p[1], p[2], p[3], 0, 0, 0])
    raise NotImplementedError("camera model %s with %d parameters (supported: %s)"
                              % (model, len(p), ", ".join(MODELS)))


def quat_to_rot(qvec):
    """COLMAP's (qw, qx, qy, qz) -> R; the quaternion is normalised first"""
    q = np.asarray(qvec, np.float64)
    w, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def rot_to_quat(R):
    """R -> COLMAP's (qw, qx, qy, qz), unit norm, qw >= 0 (quat_to_rot's
    inverse): the component of largest magnitude from the diagonal, the others
    from the off-diagonal sums and differences"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    d = [R[0, 0] + R[1, 1] + R[2, 2], R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2],
         R[2, 2] - R[0, 0] - R[1, 1]]
    k = int(np.argmax(d))
    s = 2.0 * np.sqrt(max(1.0 + d[k], 0.0))                    # 4 |q_k|
    if k == 0:
        q = [0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]
    elif k == 1:
        q = [(R[2, 1] - R[1, 2]) / s, 0.25 * s, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]
    elif k == 2:
        q = [(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, 0.25 * s, (R[1, 2] + R[2, 1]) / s]
    else:
        q = [(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, 0.25 * s]
    q = np.asarray(q) / np.sqrt(np.sum(np.square(q)))
    return -q if q[0] < 0 else q


def pose_row(qvec, t):
    """[R | t] row-major [12] of a COLMAP pose (world to camera)"""
    return np.concatenate([quat_to_rot(qvec), np.asarray(t, np.float64).reshape(3, 1)],
                          1).reshape(-1)


def read_intrinsics(path):
    """database_intrinsics.txt -> {name: (MODEL, w, h, [params])}"""
    out = {}
    with open(path) as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if len(parts) < 5:
                raise ValueError("expected 'name MODEL w h params...', got %r" % line.rstrip("\n"))
            out[parts[0]] = (parts[1], int(float(parts[2])), int(float(parts[3])),
                             [float(v) for v in parts[4:]])
    return out


def read_nvm_poses(path):
    """the camera block of an .nvm -> {name: (qvec [4], t [3])}, t = -R c"""
    with open(path) as f:
        lines = f.readlines()
    n = int(lines[2])
    out = {}
    for line in lines[3:3 + n]:
        parts = line.split()
        if len(parts) < 9:
            raise ValueError("expected 'name f qw qx qy qz cx cy cz ...', got %r" % line.rstrip("\n"))
        qvec = np.array([float(v) for v in parts[2:6]])
        c = np.array([float(v) for v in parts[6:9]])
        out[parts[0]] = (qvec, -quat_to_rot(qvec) @ c)
    return out


def summary(res):
    """points, observations, mean track length and mean reprojection error
    (over the observations) of the points with at least two inliers"""
    ok = (res["tinfo"][:, 0] == 0) & (res["tinfo"][:, 1] >= 2)
    n, obs = int(ok.sum()), int(res["tinfo"][ok, 1].sum())
    w = res["tinfo"][ok, 1].astype(np.float64)
    return dict(points=n, observations=obs, mean_track_length=(obs / n if n else 0.0),
                mean_reprojection_error=(float((res["err"][ok] * w).sum() / obs) if obs else 0.0))


def pair_list_edges(pairs, match_offsets, matches, index, set_off):
    """The verified matches as global pool rows: pairs [(name1, name2)],
    ``index`` {name: set} over the images of the pool.  Returns (edges [E, 2]
    int32, number of pairs skipped because they name an image outside the
    pool).  A match index outside its image's keypoints raises: it would land
    on a row of another image."""
    moff, matches = np.asarray(match_offsets), np.asarray(matches).reshape(-1, 2)
    sizes = np.diff(np.asarray(set_off, np.int64))
    edges, skipped = [], 0
    for p, (a, b) in enumerate(pairs):
        if a not in index or b not in index:
            skipped += 1
            continue
        m = matches[int(moff[p]):int(moff[p + 1])].astype(np.int64)
        for col, name in ((0, a), (1, b)):
            if m.shape[0] and (m[:, col].min() < 0 or m[:, col].max() >= sizes[index[name]]):
                raise ValueError("pair %d (%s %s): a match index outside the %d keypoints of %s"
                                 % (p, a, b, sizes[index[name]], name))
        edges.append(np.stack([set_off[index[a]] + m[:, 0], set_off[index[b]] + m[:, 1]], 1))
    edges = (np.concatenate(edges, 0) if edges else np.zeros((0, 2))).astype(np.int32)
    return edges, skipped


def triangulate_pair_list(verified_npz, feature_dir, postfix, intrinsics, nvm, thr=4.0,
                          min_angle=1.5, iters=64, max_track=256, seed=0, refine=0, split=0):
    _lib.require_device()
    device = torch.device("cuda", torch.cuda.current_device())
    ver = np.load(verified_npz) if isinstance(verified_npz, (str, os.PathLike)) else verified_npz
    intr, nvm_poses = read_intrinsics(intrinsics), read_nvm_poses(nvm)
    pairs = [(str(a), str(b)) for a, b in np.asarray(ver["pairs"]).reshape(-1, 2)]
    images = sorted({n for pair in pairs for n in pair if n in nvm_poses})
    missing = [n for n in images if n not in intr]
    if missing:
        raise ValueError("images with a pose but no intrinsics: %s" % ", ".join(missing[:5]))
    index = {n: i for i, n in enumerate(images)}
    kps = [np.ascontiguousarray(np.load(os.path.join(feature_dir, "%s.%s" % (n, postfix)))
                                ["keypoints"][:, :2], dtype=np.float32) for n in images]
    set_off = np.concatenate([[0], np.cumsum([k.shape[0] for k in kps])]).astype(np.int32)
    cams = np.stack([camera_row(intr[n][0], intr[n][3]) for n in images]) if images else \
        np.zeros((0, 8))
    poses = np.stack([pose_row(*nvm_poses[n]) for n in images]) if images else np.zeros((0, 12))
    edges, skipped = pair_list_edges(pairs, ver["match_offsets"], ver["matches"], index, set_off)
    kp_pool = np.concatenate(kps, 0) if kps else np.zeros((0, 2), np.float32)
    kp_d, cams_d, poses_d = (torch.from_numpy(a).to(device) for a in (kp_pool, cams, poses))
    res = geometry.triangulate_tracks(kp_d, set_off, cams_d, poses_d,
                                      torch.from_numpy(edges).to(device), iters=iters, thr=thr,
                                      min_angle=min_angle, max_track=max_track, seed=seed)
    unsplit = None
    if int(split) > 0:
        unsplit = res
        res = geometry.split_tracks(kp_d, set_off, cams_d, poses_d, res, iters=iters, thr=thr,
                                    min_angle=min_angle, rounds=int(split), seed=seed)
    if int(refine) > 0:
        res = geometry.refine_tracks(kp_d, set_off, cams_d, poses_d, res, thr=thr,
                                     min_angle=min_angle, rounds=int(refine))
    res = res.host()
    if unsplit is not None:
        res.pop("counts_unsplit", None)
        raw = geometry._read_back(dict(err=unsplit.err, tinfo=unsplit.tinfo, counts=unsplit.counts))
        c0 = raw["counts"].view(np.int32).copy()
        res.update(counts_unsplit=c0, summary_unsplit=summary(dict(
            err=raw["err"].view(np.float64)[:int(c0[0])],
            tinfo=raw["tinfo"].view(np.int32).reshape(-1, 4)[:int(c0[0])])))
    unrefined = res.pop("unrefined", None)
    if unrefined is not None:
        res.update(summary_unrefined=summary(unrefined), counts_unrefined=unrefined["counts"])
    res.update(images=images, set_off=set_off, cams=cams, poses=poses, keypoints=kp_pool,
               models=[(intr[n][0], intr[n][1], intr[n][2], intr[n][3]) for n in images],
               qvecs=[nvm_poses[n][0] for n in images], tvecs=[nvm_poses[n][1] for n in images],
               skipped_pairs=skipped)
    res["summary"] = summary(res)
    return res


def write_model(res, out_dir):
    """COLMAP's text model of a triangulate_pair_list result: cameras.txt (one
    camera per image, ids from 1), images.txt (``X Y POINT3D_ID`` per keypoint,
    -1 where it has no point) and points3D.txt (``ID X Y Z R G B ERROR`` and
    the track as ``IMAGE_ID POINT2D_IDX`` pairs) with the points that have at
    least two inlier observations; point ids are track ids + 1."""
    os.makedirs(out_dir, exist_ok=True)
    set_off, tinfo = res["set_off"], res["tinfo"]
    good = (tinfo[:, 0] == 0) & (tinfo[:, 1] >= 2)
    with open(os.path.join(out_dir, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n"
                "#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for i, (model, w, h, params) in enumerate(res["models"]):
            f.write("%d %s %d %d %s\n" % (i + 1, model, w, h, " ".join(repr(float(v)) for v in params)))
    with open(os.path.join(out_dir, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n"
                "#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for i, name in enumerate(res["images"]):
            f.write("%d %s %s %d %s\n" % (i + 1, " ".join(repr(float(v)) for v in res["qvecs"][i]),
                                          " ".join(repr(float(v)) for v in res["tvecs"][i]), i + 1,
                                          name))
            rows = range(int(set_off[i]), int(set_off[i + 1]))
            trip = []
            for r in rows:
                t = int(res["point_of_row"][r])
                pid = t + 1 if t >= 0 and good[t] else -1
                trip.append("%s %s %d" % (repr(float(res["keypoints"][r, 0])),
                                          repr(float(res["keypoints"][r, 1])), pid))
            f.write(" ".join(trip) + "\n")
    image_of = np.repeat(np.arange(len(res["images"])), np.diff(set_off))
    with open(os.path.join(out_dir, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for t in np.flatnonzero(good):
            sl = slice(int(res["track_off"][t]), int(res["track_off"][t + 1]))
            rows = res["track_rows"][sl][res["obs_inlier"][sl] != 0]
            track = " ".join("%d %d" % (image_of[r] + 1, r - set_off[image_of[r]]) for r in rows)
            f.write("%d %s 0 0 0 %s %s\n" % (t + 1, " ".join(repr(float(v)) for v in res["points"][t]),
                                             repr(float(res["err"][t])), track))


def _data_lines(path):
    with open(path) as f:
        return [ln.rstrip("\n") for ln in f if not ln.startswith("#")]


def read_model(model_dir):
    """the text model back: (cameras {id: (MODEL, w, h, [params])}, images {id:
    dict(qvec, tvec, camera_id, name, xys [n, 2], point3D_ids [n])}, points {id:
    dict(xyz, error, track [(image_id, point2D_idx)])})"""
    cameras, images, points = {}, {}, {}
    for ln in _data_lines(os.path.join(model_dir, "cameras.txt")):
        p = ln.split()
        if p:
            cameras[int(p[0])] = (p[1], int(p[2]), int(p[3]), [float(v) for v in p[4:]])
    lines = _data_lines(os.path.join(model_dir, "images.txt"))
    for head, pts in zip(lines[0::2], lines[1::2]):
        p, q = head.split(), pts.split()
        images[int(p[0])] = dict(
            qvec=np.array([float(v) for v in p[1:5]]), tvec=np.array([float(v) for v in p[5:8]]),
            camera_id=int(p[8]), name=p[9],
            xys=np.array([float(v) for v in q]).reshape(-1, 3)[:, :2] if q else np.zeros((0, 2)),
            point3D_ids=np.array([int(v) for v in q[2::3]], dtype=np.int64))
    for ln in _data_lines(os.path.join(model_dir, "points3D.txt")):
        p = ln.split()
        if p:
            tr = [int(v) for v in p[8:]]
            points[int(p[0])] = dict(xyz=np.array([float(v) for v in p[1:4]]), error=float(p[7]),
                                     track=list(zip(tr[0::2], tr[1::2])))
    return cameras, images, points
