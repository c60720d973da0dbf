"""Numpy restatement of the triangulation definitions of include/posfeat_hip.h
(posfeat_triangulate): camera model, tracks from edges, the DLT with the Jacobi
of the fundamental refit, hypotheses, score, selection, refit, outputs.
Written from those definitions in plain loops; float64 throughout.  Shared by
the triangulation tests; nothing here touches the GPU."""
import numpy as np

from fundamental_ref import jacobi
from ransac_ref import sample as sample4

W_REL = 1e-12


def undistort(cam, x, y):
    fx, fy, cx, cy, k1 = (float(v) for v in cam[:5])
    with np.errstate(all="ignore"):
        xd, yd = (x - cx) / fx, (y - cy) / fy
        rd = float(np.hypot(xd, yd))
        if k1 == 0.0 or rd == 0.0:
            return xd, yd
        ru = rd
        for _ in range(8):
            g = ru * (1.0 + k1 * (ru * ru)) - rd
            d = 1.0 + 3.0 * k1 * (ru * ru)
            if d > 0.0 and np.isfinite(d):
                ru = ru - g / d
        return (ru / rd) * xd, (ru / rd) * yd


def project(cam, pose, X):
    """(pixel x, pixel y, depth)"""
    fx, fy, cx, cy, k1 = (float(v) for v in cam[:5])
    P = np.asarray(pose, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        xc, yc, z = P[:, :3] @ np.asarray(X, np.float64) + P[:, 3]
        xn, yn = xc / z, yc / z
        f = 1.0 + k1 * (xn * xn + yn * yn)
        return fx * f * xn + cx, fy * f * yn + cy, z


def reproj2(cam, pose, X, xy):
    """(squared reprojection error, depth)"""
    with np.errstate(all="ignore"):
        px, py, z = project(cam, pose, X)
        return (px - xy[0]) ** 2 + (py - xy[1]) ** 2, z


def centre(pose):
    P = np.asarray(pose, np.float64).reshape(3, 4)
    return -P[:, :3].T @ P[:, 3]


def dlt_matrix(obs):
    """obs: rows (xu, yu, pose[12]) in order -> N4"""
    N = np.zeros((4, 4))
    for o in obs:
        P = np.asarray(o[2:14], np.float64).reshape(3, 4)
        a, b = o[0] * P[2] - P[0], o[1] * P[2] - P[1]
        N = (N + np.outer(a, a)) + np.outer(b, b)
    return N


def dlt(obs):
    """X [3] or None when rejected; also the eigenvalues (diagonal after Jacobi)"""
    with np.errstate(all="ignore"):
        d, V = jacobi(dlt_matrix(obs))
        v = V[:, int(np.argmin(d))]
        if not np.all(np.isfinite(v)) or not abs(v[3]) > W_REL * np.abs(v).max():
            return None, d
        X = v[:3] / v[3]
        return (X if np.all(np.isfinite(X)) else None), d


def set_of_rows(set_off):
    set_off = np.asarray(set_off, np.int64)
    return np.repeat(np.arange(len(set_off) - 1), np.diff(set_off))


def components(edges, set_off, max_track):
    """-> (tracks: list of ascending row lists in ascending root order, dropped,
    ignored)"""
    N = int(set_off[-1])
    sid = set_of_rows(set_off)
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    ignored = 0
    for a, b in np.asarray(edges, np.int64).reshape(-1, 2):
        if a < 0 or b < 0 or a >= N or b >= N or a == b or sid[a] == sid[b]:
            ignored += 1
            continue
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    comp = {}
    for r in range(N):
        comp.setdefault(find(r), []).append(r)
    tracks, dropped = [], 0
    for root in sorted(comp):
        rows = comp[root]
        if len(rows) > max_track:
            dropped += 1
        elif len(rows) >= 2:
            tracks.append(rows)
    return tracks, dropped, ignored


def hyp_pairs(m, root, iters, seed):
    H = m * (m - 1) // 2
    if H <= iters:
        return [(i, j) for i in range(m) for j in range(i + 1, m)]
    return [tuple(sample4(seed, root, h, m)[:2]) for h in range(iters)]


def angle_cos(X, Ci, Cj):
    a, b = X - Ci, X - Cj
    na, nb = np.sqrt(a @ a), np.sqrt(b @ b)
    if not (na > 0.0 and nb > 0.0):
        return None
    return float((a @ b) / (na * nb))


class Scene:
    def __init__(self, kp, set_off, cams, poses):
        self.kp = np.asarray(kp, np.float32).astype(np.float64)
        self.sid = set_of_rows(set_off)
        self.cams = np.asarray(cams, np.float64).reshape(-1, 8)
        self.poses = np.asarray(poses, np.float64).reshape(-1, 12)
        self.und = np.array([undistort(self.cams[s], x, y)
                             for (x, y), s in zip(self.kp, self.sid)]).reshape(-1, 2)

    def obs(self, r):
        return np.concatenate([self.und[r], self.poses[self.sid[r]]])

    def reproj2(self, r, X):
        s = self.sid[r]
        return reproj2(self.cams[s], self.poses[s], X, self.kp[r])

    def reproj2_rows(self, rows, X):
        """reproj2 for many rows at once: the same operations, elementwise"""
        s = self.sid[rows]
        P, c, xy = self.poses[s], self.cams[s], self.kp[rows]
        with np.errstate(all="ignore"):
            xc = ((P[:, 0] * X[0] + P[:, 1] * X[1]) + P[:, 2] * X[2]) + P[:, 3]
            yc = ((P[:, 4] * X[0] + P[:, 5] * X[1]) + P[:, 6] * X[2]) + P[:, 7]
            z = ((P[:, 8] * X[0] + P[:, 9] * X[1]) + P[:, 10] * X[2]) + P[:, 11]
            xn, yn = xc / z, yc / z
            f = 1.0 + c[:, 4] * (xn * xn + yn * yn)
            dx, dy = (c[:, 0] * f * xn + c[:, 2]) - xy[:, 0], (c[:, 1] * f * yn + c[:, 3]) - xy[:, 1]
            return dx * dx + dy * dy, z


def triangulate_track(sc, rows, iters, thr, min_angle_deg, seed, margins=None):
    """One track (ascending rows) -> dict(status, X, err, n_inliers, best_h,
    refit_kept, flags, eig).  ``margins`` (a dict) collects the closest
    distances to the decision thresholds: 'err' (|e - thr| over everything
    scored), 'depth' (|z|), 'cos' (|cos - cosmin|)."""
    m, thr2, cosmin = len(rows), thr * thr, np.cos(np.deg2rad(min_angle_deg))
    mg = margins if margins is not None else {}
    for k in ("err", "depth", "cos"):
        mg.setdefault(k, np.inf)

    rows_a = np.asarray(rows, np.int64)

    def flags_of(X):
        with np.errstate(all="ignore"):
            e2, z = sc.reproj2_rows(rows_a, X)
            if np.isfinite(z).any():
                mg["depth"] = min(mg["depth"], float(np.abs(z[np.isfinite(z)]).min()))
            scored = np.isfinite(e2) & (z > 0)
            if scored.any():
                mg["err"] = min(mg["err"], float(np.abs(np.sqrt(e2[scored]) - thr).min()))
            return (z > 0.0) & np.isfinite(e2) & (e2 <= thr2)

    def pair_ok(i, j, X):
        Pi, Pj = sc.poses[sc.sid[rows[i]]], sc.poses[sc.sid[rows[j]]]
        zi = Pi.reshape(3, 4)[2] @ np.append(X, 1.0)
        zj = Pj.reshape(3, 4)[2] @ np.append(X, 1.0)
        mg["depth"] = min(mg["depth"], abs(zi), abs(zj))
        if not (zi > 0.0 and zj > 0.0):
            return False
        c = angle_cos(X, centre(Pi), centre(Pj))
        if c is None:
            return False
        mg["cos"] = min(mg["cos"], abs(c - cosmin))
        return c < cosmin

    out = dict(status=1, X=np.zeros(3), err=0.0, n_inliers=0, best_h=-1, refit_kept=0,
               flags=np.zeros(m, bool), eig=None)
    best = (-1, -1, None, None)
    for h, (i, j) in enumerate(hyp_pairs(m, rows[0], iters, seed)):
        X, _ = dlt([sc.obs(rows[i]), sc.obs(rows[j])])
        if X is None or not pair_ok(i, j, X):
            continue
        cnt = int(flags_of(X).sum())
        if cnt > best[0]:
            best = (cnt, h, X, (i, j))
    if best[0] < 0:
        return out
    c0, h0, X0, (i0, j0) = best
    f0 = flags_of(X0)
    X, flags, keep = X0, f0, 0
    if f0.any():
        X1, eig = dlt([sc.obs(r) for r, f in zip(rows, f0) if f])
        out["eig"] = np.sort(eig)
        if X1 is not None:
            f1 = flags_of(X1)
            if int(f1.sum()) >= c0 and pair_ok(i0, j0, X1):
                X, flags, keep = X1, f1, 1
    errs = [np.sqrt(sc.reproj2(r, X)[0]) for r, f in zip(rows, flags) if f]
    s = 0.0
    for e in errs:
        s = s + e
    out.update(status=0, X=X, err=(s / len(errs) if errs else 0.0), n_inliers=int(flags.sum()),
               best_h=h0, refit_kept=keep, flags=flags)
    return out


def triangulate(kp, set_off, cams, poses, edges, iters, thr, min_angle_deg, max_track, seed):
    """The whole call -> dict of the outputs of posfeat_triangulate, trimmed,
    plus 'margins' and 'eig_ratio' (per track: second-smallest over largest
    eigenvalue of the refit matrix, nan where there was no refit)."""
    sc = Scene(kp, set_off, cams, poses)
    N = int(set_off[-1])
    tracks, dropped, ignored = components(edges, set_off, max_track)
    T = len(tracks)
    margins = {}
    points, err, tinfo = np.zeros((T, 3)), np.zeros(T), np.zeros((T, 4), np.int32)
    track_off, rows_all, flags_all = [0], [], []
    point_of_row = np.full(N, -1, np.int32)
    eig_ratio = np.full(T, np.nan)
    for t, rows in enumerate(tracks):
        r = triangulate_track(sc, rows, iters, thr, min_angle_deg, seed, margins)
        points[t], err[t] = r["X"], r["err"]
        tinfo[t] = (r["status"], r["n_inliers"], r["best_h"], r["refit_kept"])
        rows_all += rows
        flags_all += list(r["flags"])
        track_off.append(len(rows_all))
        if r["status"] == 0:
            for row, f in zip(rows, r["flags"]):
                if f:
                    point_of_row[row] = t
        if r["eig"] is not None and r["eig"][-1] > 0:
            eig_ratio[t] = r["eig"][1] / r["eig"][-1]
    flags_all = np.asarray(flags_all, np.uint8)
    ok = tinfo[:, 0] == 0
    counts = np.array([T, len(rows_all), int(ok.sum()), int(tinfo[ok, 1].sum()), dropped, ignored,
                       0, 0], np.int32)
    return dict(points=points, err=err, tinfo=tinfo, track_off=np.asarray(track_off, np.int32),
                track_rows=np.asarray(rows_all, np.int32), obs_inlier=flags_all,
                point_of_row=point_of_row, counts=counts, margins=margins, eig_ratio=eig_ratio)


def summary(res):
    """points, observations, mean track length, mean reprojection error of a
    result (host dict), counted track by track: a point is a status-0 track
    with at least two inlier observations; the error is averaged over the
    observations"""
    points, obs, err_sum = 0, 0, 0.0
    for t in range(len(res["tinfo"])):
        status, n_in = int(res["tinfo"][t][0]), int(res["tinfo"][t][1])
        if status != 0 or n_in < 2:
            continue
        points += 1
        obs += n_in
        err_sum += float(res["err"][t]) * n_in
    return dict(points=points, observations=obs,
                mean_track_length=(obs / points if points else 0.0),
                mean_reprojection_error=(err_sum / obs if obs else 0.0))


# ---- the planted scene the tests share -----------------------------------

def rot_y(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def line_cameras(n, step=0.45, k1=-0.06, yaw=2.0):
    """n cameras ``step`` apart on the x axis looking down +z (camera i turned
    by +-yaw degrees about y), K = 500 / 320 / 240, every second one
    SIMPLE_RADIAL with k1 -> (cams [n, 8], poses [n, 12])"""
    cams, poses = np.zeros((n, 8)), np.zeros((n, 12))
    for i in range(n):
        cams[i, :5] = (500.0, 500.0, 320.0, 240.0, k1 if i % 2 else 0.0)
        R = rot_y(yaw if i % 2 else -yaw)
        C = np.array([step * i, 0.0, 0.0])
        poses[i] = np.concatenate([R, (-R @ C)[:, None]], 1).reshape(-1)
    return cams, poses


def observe(cam, pose, X, rng=None, sigma=0.0):
    """the pixel of X as fp32, with Gaussian noise of ``sigma`` px"""
    px, py, _ = project(cam, pose, X)
    xy = np.array([px, py])
    if sigma > 0.0:
        xy = xy + rng.normal(0.0, sigma, 2)
    return xy.astype(np.float32)
