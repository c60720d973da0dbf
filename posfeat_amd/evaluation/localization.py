"""Query poses from verified query-database matches and a sparse model, on the
GPU: what the reference's Aachen pipeline asks of ``colmap image_registrator``
and its ``recover_query_poses`` (evaluations/aachen/reconstruct_pipeline.py),
without COLMAP.

  register_query_list(verified_npz, feature_dir, postfix, model_dir,
                      query_intrinsics, thr=12.0, iters=1024, min_inliers=30,
                      min_ratio=0.25, seed=0) -> dict
  write_predictions(res, path)

``verified_npz`` is what evaluation.verification.verify_pair_list wrote (pairs,
match_offsets, matches); ``model_dir`` holds the text model
evaluation.reconstruction.write_model wrote; ``query_intrinsics`` is the
dataset's ``night_time_queries_with_intrinsics*.txt`` (``name MODEL w h
params...``).  The queries are the names of that file, in sorted order; the
keypoints of those that occur in a pair with a model image form one pool (the
others have no correspondence and stay unregistered).  A verified match between
a query keypoint and a model image's keypoint that carries a 3-D point is a
2D-3D correspondence (geometry.pose_correspondences keeps each (keypoint,
point) once); geometry.ransac_pose_queries runs once over all queries, and
poses, info and masks come back in one copy with one synchronisation.  Query q
of the sorted list samples as query q.

A query is registered iff its status is 0, n_inliers >= min_inliers and
n_inliers / n >= min_ratio (n its correspondences).  thr = 12 px, 30 and 0.25
are meant to be COLMAP's abs_pose_max_error, abs_pose_min_num_inliers and
abs_pose_min_inlier_ratio defaults; they are written from memory and have not
been checked against COLMAP's sources.

The returned dict:
  queries      [nq] names
  registered   [nq] bool
  poses        [nq, 12] fp64 [R | t] world to camera (zeros where none was found)
  qvecs, tvecs [nq, 4] (qw >= 0), [nq, 3]
  info         [nq, 4] int32 as posfeat_ransac_pose gives it
  n_corr       [nq] correspondences per query
  corr, q_off, inlier   the correspondences (query pool row, point index), the
               queries' table and the inlier mask
  point_ids    [P] the model's POINT3D_ID of point index i
  keypoints, cams, points   what the call ran on: the query pool [N, 2] fp32,
               the camera rows [nq, 8] and the points [P, 3] in index order
  skipped_pairs  pairs that do not join a query and a model image
"""
import os

import numpy as np
import torch

from .. import _lib, geometry
from . import reconstruction as rc


def registered_mask(info, n_corr, min_inliers=30, min_ratio=0.25):
    """the acceptance rule on info [nq, 4] and the correspondence counts [nq]"""
    info, n = np.asarray(info).reshape(-1, 4), np.asarray(n_corr, np.float64).reshape(-1)
    nin = info[:, 1].astype(np.float64)
    return (info[:, 0] == 0) & (nin >= min_inliers) & (nin >= min_ratio * n) & (n > 0)


def model_points(images, points):
    """The pool of a read_model result: (image ids in ascending order, set_off
    [n + 1], point_of_row [N] the point index of a keypoint or -1, point_ids
    [P] ascending, xyz [P, 3], tinfo [P, 4] = (0, track length, 0, 0))"""
    ids = sorted(images)
    point_ids = np.asarray(sorted(points), dtype=np.int64)
    xyz = np.asarray([points[int(p)]["xyz"] for p in point_ids], np.float64).reshape(-1, 3)
    tinfo = np.zeros((len(point_ids), 4), np.int32)
    tinfo[:, 1] = [len(points[int(p)]["track"]) for p in point_ids]
    set_off = np.concatenate([[0], np.cumsum([len(images[i]["point3D_ids"]) for i in ids])])
    por = np.concatenate([images[i]["point3D_ids"] for i in ids] or [np.zeros(0, np.int64)])
    at = np.searchsorted(point_ids, por)
    at = np.minimum(at, max(len(point_ids) - 1, 0))
    hit = (por >= 0) & (len(point_ids) > 0)
    if len(point_ids):
        hit &= point_ids[at] == por
    return ids, set_off.astype(np.int64), np.where(hit, at, -1).astype(np.int32), point_ids, xyz, tinfo


def register_query_list(verified_npz, feature_dir, postfix, model_dir, query_intrinsics, thr=12.0,
                        iters=1024, min_inliers=30, min_ratio=0.25, seed=0):
    _lib.require_device()
    device = torch.device("cuda", torch.cuda.current_device())
    ver = np.load(verified_npz) if isinstance(verified_npz, (str, os.PathLike)) else verified_npz
    _, images, points = rc.read_model(model_dir)
    intr = rc.read_intrinsics(query_intrinsics)
    ids, db_off, point_of_row, point_ids, xyz, tinfo = model_points(images, points)
    db_index = {images[i]["name"]: k for k, i in enumerate(ids)}
    queries = sorted(n for n in intr if n not in db_index)
    q_index = {n: k for k, n in enumerate(queries)}
    pairs = [(str(a), str(b)) for a, b in np.asarray(ver["pairs"]).reshape(-1, 2)]
    moff, matches = np.asarray(ver["match_offsets"]), np.asarray(ver["matches"]).reshape(-1, 2)
    used, skipped = set(), 0
    for a, b in pairs:
        if a in q_index and b in db_index:
            used.add(a)
        elif b in q_index and a in db_index:
            used.add(b)
        else:
            skipped += 1
    kps = [np.ascontiguousarray(np.load(os.path.join(feature_dir, "%s.%s" % (n, postfix)))
                                ["keypoints"][:, :2], dtype=np.float32) if n in used else
           np.zeros((0, 2), np.float32) for n in queries]
    q_set_off = np.concatenate([[0], np.cumsum([k.shape[0] for k in kps])]).astype(np.int64)
    q_rows, db_rows = [], []
    for p, (a, b) in enumerate(pairs):
        m = matches[int(moff[p]):int(moff[p + 1])].astype(np.int64)
        if a in q_index and b in db_index:
            qn, dn, mq, md = a, b, m[:, 0], m[:, 1]
        elif b in q_index and a in db_index:
            qn, dn, mq, md = b, a, m[:, 1], m[:, 0]
        else:
            continue
        nq_kp = q_set_off[q_index[qn] + 1] - q_set_off[q_index[qn]]
        nd_kp = db_off[db_index[dn] + 1] - db_off[db_index[dn]]
        if m.shape[0] and (mq.min() < 0 or mq.max() >= nq_kp or md.min() < 0 or md.max() >= nd_kp):
            raise ValueError("pair %d (%s %s): a match index outside the keypoints of its image"
                             % (p, a, b))
        q_rows.append(q_set_off[q_index[qn]] + mq)
        db_rows.append(db_off[db_index[dn]] + md)
    q_rows = np.concatenate(q_rows or [np.zeros(0, np.int64)])
    db_rows = np.concatenate(db_rows or [np.zeros(0, np.int64)])
    nq = len(queries)
    cams = np.stack([rc.camera_row(intr[n][0], intr[n][3]) for n in queries]) if nq else \
        np.zeros((0, 8))
    kp_pool = np.concatenate(kps, 0) if kps else np.zeros((0, 2), np.float32)
    corr, q_off = geometry.pose_correspondences(
        torch.from_numpy(q_rows).to(device), torch.from_numpy(db_rows).to(device),
        torch.from_numpy(point_of_row).to(device), torch.from_numpy(tinfo).to(device), q_set_off)
    poses, info, inlier = geometry.ransac_pose_queries(
        torch.from_numpy(kp_pool).to(device), torch.from_numpy(cams).to(device),
        torch.from_numpy(xyz).to(device), corr, q_off, iters=iters, thr=thr, seed=seed)
    # one synchronisation: everything into one pinned byte buffer
    parts = [poses.reshape(-1).view(torch.uint8), info.reshape(-1).view(torch.uint8), inlier,
             corr.reshape(-1).view(torch.uint8)]
    sizes = [int(p.numel()) for p in parts]
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    at = 0
    for p, s in zip(parts, sizes):
        host[at:at + s].copy_(p, non_blocking=True)
        at += s
    torch.cuda.current_stream(device).synchronize()
    h, cuts = host.numpy(), np.cumsum([0] + sizes)
    poses = h[cuts[0]:cuts[1]].view(np.float64).reshape(nq, 12).copy()
    info = h[cuts[1]:cuts[2]].view(np.int32).reshape(nq, 4).copy()
    n_corr = np.diff(q_off).astype(np.int64)
    reg = registered_mask(info, n_corr, min_inliers, min_ratio)
    return dict(queries=queries, registered=reg, poses=poses, info=info, n_corr=n_corr,
                qvecs=np.asarray([rc.rot_to_quat(P.reshape(3, 4)[:, :3]) if ok else [1.0, 0, 0, 0]
                                  for P, ok in zip(poses, info[:, 0] == 0)]).reshape(nq, 4),
                tvecs=poses.reshape(nq, 3, 4)[:, :, 3].copy(),
                corr=h[cuts[3]:cuts[4]].view(np.int32).reshape(-1, 2).copy(), q_off=q_off,
                inlier=h[cuts[2]:cuts[3]].copy(), point_ids=point_ids, skipped_pairs=skipped,
                keypoints=kp_pool, cams=cams, points=xyz)


def write_predictions(res, path):
    """One line per registered query, ``basename qw qx qy qz tx ty tz`` (what
    the reference's recover_query_poses writes): the file the Aachen benchmark
    scores.  Returns the number of lines."""
    n = 0
    with open(path, "w") as f:
        for name, ok, q, t in zip(res["queries"], res["registered"], res["qvecs"], res["tvecs"]):
            if not ok:
                continue
            f.write("%s %s\n" % (name.split("/")[-1],
                                 " ".join(repr(float(v)) for v in list(q) + list(t))))
            n += 1
    return n
