"""Relative-pose accuracy as descriptor papers report it: the rotation and
translation-direction errors of estimated two-view poses against ground truth,
and the area under the recall curve of their maximum (pose AUC at 5, 10 and 20
degrees).  Pure numpy; nothing here touches the device.

  relative_pose_errors(pose_est, pose_gt) -> (rot_deg, trans_deg)
        poses are [..., 3, 4] = [R | t] with x2 ~ R x1 + t.  The rotation error
        is the angle of R_est^T R_gt; the translation error the angle between
        the two t, sign-insensitive (t and -t give 0), as the usual protocol
        has it, since an essential matrix fixes t only up to sign before the
        cheirality test.  A zero or non-finite pose (no model) gives 180 / 90.
  pose_auc(errors, thresholds=(5, 10, 20)) -> [len(thresholds)]
        errors: per pair max(rot_deg, trans_deg).  The recall curve steps at
        the sorted errors (recall (i + 1) / n at the i-th); its area up to each
        threshold by the trapezoid rule, divided by the threshold.
  relative_poses(poses, pairs) -> [npairs, 3, 4]
        ground-truth relative poses of image pairs from world-to-camera [R | t]
        rows: R = R2 R1^T, t = t2 - R t1, t scaled to length 1.
"""
import numpy as np


def relative_pose_errors(pose_est, pose_gt):
    pe = np.asarray(pose_est, np.float64)
    pg = np.asarray(pose_gt, np.float64)
    if pe.shape[-2:] != (3, 4) or pe.shape != pg.shape:
        raise ValueError("poses must be [..., 3, 4] of one shape")
    Re, te, Rg, tg = pe[..., :3], pe[..., 3], pg[..., :3], pg[..., 3]
    with np.errstate(all="ignore"):
        c = (np.einsum("...ij,...ij->...", Re, Rg) - 1.0) / 2.0     # tr(Re^T Rg)
        rot = np.degrees(np.arccos(np.clip(c, -1.0, 1.0)))
        ct = np.abs(np.einsum("...i,...i->...", te, tg)) / (
            np.linalg.norm(te, axis=-1) * np.linalg.norm(tg, axis=-1))
        trans = np.degrees(np.arccos(np.clip(ct, 0.0, 1.0)))
    bad = ~np.isfinite(pe).all((-1, -2)) | ~np.any(Re != 0, axis=(-1, -2))
    rot = np.where(bad | ~np.isfinite(rot), 180.0, rot)
    trans = np.where(bad | ~np.isfinite(trans), 90.0, trans)
    return rot, trans


def pose_auc(errors, thresholds=(5, 10, 20)):
    e = np.sort(np.asarray(errors, np.float64).reshape(-1))
    n = e.shape[0]
    if n == 0:
        return np.zeros(len(thresholds))
    recall = np.concatenate([[0.0], (np.arange(n) + 1.0) / n])
    e = np.concatenate([[0.0], e])
    out = []
    for t in thresholds:
        last = int(np.searchsorted(e, t))                  # the errors below t
        x = np.concatenate([e[:last], [float(t)]])
        y = np.concatenate([recall[:last], [recall[last - 1]]])
        out.append(float(np.sum((x[1:] - x[:-1]) * (y[1:] + y[:-1]) / 2.0) / t))
    return np.asarray(out)


def relative_poses(poses, pairs):
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    out = np.zeros((len(pairs), 3, 4))
    for k, (a, b) in enumerate(pairs):
        R = poses[b][:, :3] @ poses[a][:, :3].T
        t = poses[b][:, 3] - R @ poses[a][:, 3]
        nt = np.linalg.norm(t)
        out[k, :, :3] = R
        out[k, :, 3] = t / nt if nt > 0 else t
    return out
