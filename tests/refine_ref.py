"""Numpy restatement of the point-refinement definitions of
include/posfeat_hip.h (posfeat_refine_points, posfeat_refine_point): residual
and Jacobian, the sums in their fixed order, the damped solve with the pose
refit's pivot rule, the Levenberg-Marquardt round, the rounds with the inlier
test in between, the angle filter, the outputs.  Written from those
definitions in plain loops; float64 throughout.  Shared by the refinement
tests; nothing here touches the GPU."""
import numpy as np

import triangulate_ref as tr

LANE_TRACK, WAVE, MAX_TRACK = 16, 64, 1024
LAMBDA0, LAMBDA_MAX, STEP_STOP, PIVOT_REL = 1e-4, 1e8, 1e-10, 1e-12


def row_terms(cam, pose, xy, X):
    """(r [2], J [2, 3], usable) of one observation at X"""
    fx, fy, cx, cy, k1 = (float(v) for v in cam[:5])
    P = np.asarray(pose, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        xc = ((P[0, 0] * X[0] + P[0, 1] * X[1]) + P[0, 2] * X[2]) + P[0, 3]
        yc = ((P[1, 0] * X[0] + P[1, 1] * X[1]) + P[1, 2] * X[2]) + P[1, 3]
        z = ((P[2, 0] * X[0] + P[2, 1] * X[1]) + P[2, 2] * X[2]) + P[2, 3]
        xn, yn = xc / z, yc / z
        f = 1.0 + k1 * (xn * xn + yn * yn)
        r = np.array([(fx * f * xn + cx) - xy[0], (fy * f * yn + cy) - xy[1]])
        axx, axy = fx * (f + 2.0 * k1 * (xn * xn)), fx * (2.0 * k1 * (xn * yn))
        ayx, ayy = fy * (2.0 * k1 * (xn * yn)), fy * (f + 2.0 * k1 * (yn * yn))
        iz = 1.0 / z
        jx = np.array([axx * iz, axy * iz, -(axx * xn + axy * yn) * iz])
        jy = np.array([ayx * iz, ayy * iz, -(ayx * xn + ayy * yn) * iz])
        R = P[:, :3]
        J = np.stack([(jx[0] * R[0] + jx[1] * R[1]) + jx[2] * R[2],
                      (jy[0] * R[0] + jy[1] * R[1]) + jy[2] * R[2]])
        e2 = r[0] * r[0] + r[1] * r[1]
        return r, J, bool(z > 0.0 and np.isfinite(e2))


def add_row(acc, r, J):
    """acc [10] += (J^T J upper triangle row-major, J^T r, r . r): first the x
    row's product, then the y row's"""
    with np.errstate(all="ignore"):
        k = 0
        for a in range(3):
            for b in range(a, 3):
                acc[k] = (acc[k] + J[0, a] * J[0, b]) + J[1, a] * J[1, b]
                k += 1
        for a in range(3):
            acc[6 + a] = (acc[6 + a] + J[0, a] * r[0]) + J[1, a] * r[1]
        acc[9] = acc[9] + (r[0] * r[0] + r[1] * r[1])


def sums(obs, member_index, m, X):
    """The sums over the observations ``obs`` (rows (xy, cam, pose)) that are
    members ``member_index`` of a track of m members, in the order of the
    definition -> (acc [10], usable)"""
    ok = True
    if m <= LANE_TRACK:
        acc = np.zeros(10)
        for o in obs:
            r, J, u = row_terms(o[1], o[2], o[0], X)
            add_row(acc, r, J)
            ok = ok and u
        return acc, ok
    part = np.zeros((WAVE, 10))
    for o, k in zip(obs, member_index):
        r, J, u = row_terms(o[1], o[2], o[0], X)
        add_row(part[k % WAVE], r, J)
        ok = ok and u
    o_ = WAVE // 2
    with np.errstate(all="ignore"):
        while o_ > 0:
            part = part + part[np.arange(WAVE) ^ o_]
            o_ >>= 1
    return part[0].copy(), ok


def pivot_solve(A, b):
    """A delta = b by Gaussian elimination with partial pivoting (the first
    largest entry of the column) -> delta or None"""
    n = len(b)
    a = np.concatenate([np.asarray(A, np.float64), np.asarray(b, np.float64)[:, None]], 1)
    with np.errstate(all="ignore"):
        cmax = np.abs(a[:, :n]).max(0)
        ok = True
        for c in range(n):
            piv, best = c, abs(a[c, c])
            for r in range(c + 1, n):
                if abs(a[r, c]) > best:
                    best, piv = abs(a[r, c]), r
            if piv != c:
                a[[c, piv]] = a[[piv, c]]
            ok = ok and bool(best >= PIVOT_REL * cmax[c] and best > 0.0)
            for r in range(c + 1, n):
                f = a[r, c] / a[c, c]
                a[r, c + 1:] = a[r, c + 1:] - f * a[c, c + 1:]
        d = np.zeros(n)
        for c in range(n - 1, -1, -1):
            s = a[c, n]
            for j in range(c + 1, n):
                s = s - a[c, j] * d[j]
            d[c] = s / a[c, c]
        return d if ok and np.isfinite(d.sum()) else None


def lm_solve(acc, lam):
    N = np.array([[acc[0], acc[1], acc[2]], [acc[1], acc[3], acc[4]], [acc[2], acc[4], acc[5]]])
    with np.errstate(all="ignore"):
        for i in range(3):
            N[i, i] = N[i, i] + lam * N[i, i]
        return pivot_solve(N, -acc[6:9])


def lm_round(obs, member_index, m, X0, steps):
    """One round on a fixed set -> (X, cost, taken); cost is NaN when the set is
    not usable at X0"""
    X = np.array(X0, np.float64)
    acc, ok = sums(obs, member_index, m, X)
    if not ok:
        return X, np.nan, 0
    lam, taken, evals = LAMBDA0, 0, 0
    while evals < steps and lam <= LAMBDA_MAX:
        d = lm_solve(acc, lam)
        take = False
        if d is not None:
            Xn = X + d
            accn, okn = sums(obs, member_index, m, Xn)
            evals += 1
            take = bool(okn and accn[9] < acc[9])
        if not take:
            lam = lam * 10.0
            continue
        X, acc = Xn, accn
        lam = lam / 10.0
        taken += 1
        if np.abs(d).max() <= STEP_STOP * max(1.0, np.abs(X).max()):
            break
    return X, float(acc[9]), taken


def refine_point(obs22, X0, steps):
    """posfeat_refine_point on obs [n, 22] rows"""
    obs = [(o[0:2], o[2:10], o[10:22]) for o in np.asarray(obs22, np.float64)]
    return lm_round(obs, list(range(len(obs))), len(obs), X0, steps)


def cost_of(obs22, X):
    c = 0.0
    for o in np.asarray(obs22, np.float64):
        e2, _ = tr.reproj2(o[2:10], o[10:22], X, o[0:2])
        c += e2
    return c


def gradient_of(obs22, X):
    """(g = sum J^T r, sum over rows of |J| |r|) at X"""
    g, scale = np.zeros(3), 0.0
    for o in np.asarray(obs22, np.float64):
        r, J, _ = row_terms(o[2:10], o[10:22], o[0:2], X)
        g += J.T @ r
        scale += np.linalg.norm(J) * np.linalg.norm(r)
    return g, scale


def refine_track(sc, rows, flags_in, X0, status_in, thr, min_angle_deg, rounds, steps,
                 margins=None):
    """One track -> dict(status, X, err, n_inliers, flags, rinfo).  ``margins``
    collects the closest relative distance of a tested squared error to thr^2
    ('err2') and of a tested cosine to the threshold ('cos')."""
    m, thr2, cosmin = len(rows), thr * thr, np.cos(np.deg2rad(min_angle_deg))
    mg = margins if margins is not None else {}
    for k in ("err2", "cos"):
        mg.setdefault(k, np.inf)
    N = len(sc.kp)
    out = dict(status=1, X=np.zeros(3), err=0.0, n_inliers=0, flags=np.zeros(m, bool),
               rinfo=(0, 0, 0, 0), cost_in=np.nan, cost_out=np.nan)
    if status_in != 0:
        return out
    valid = np.array([0 <= r < N for r in rows], bool)
    given = np.asarray(flags_in) != 0
    S = given & valid
    X = np.array(X0, np.float64)

    def obs_of(idx):
        return [(sc.kp[rows[k]], sc.cams[sc.sid[rows[k]]], sc.poses[sc.sid[rows[k]]]) for k in idx]

    used = taken = converged = 0
    status, errs = 0, np.zeros(m)
    for _ in range(rounds):
        used += 1
        idx = list(np.flatnonzero(S))
        if len(idx) >= 2:
            X, _, tk = lm_round(obs_of(idx), idx, m, X, steps)
            taken += tk
        F = np.zeros(m, bool)
        for k in range(m):
            if not valid[k]:
                continue
            with np.errstate(all="ignore"):
                e2, z = sc.reproj2(rows[k], X)
                if z > 0.0 and np.isfinite(e2):
                    mg["err2"] = min(mg["err2"], abs(e2 - thr2) / thr2)
                F[k] = bool(z > 0.0 and np.isfinite(e2) and e2 <= thr2)
                errs[k] = np.sqrt(e2) if F[k] else 0.0
        same = bool(np.array_equal(F, S))
        S = F
        if S.sum() < 2:
            status = 2
            break
        if same:
            converged = 1
            break
    if status == 0:
        found = False
        idx = list(np.flatnonzero(S))
        for a in range(len(idx)):
            for b in range(a + 1, len(idx)):
                c = tr.angle_cos(X, tr.centre(sc.poses[sc.sid[rows[idx[a]]]]),
                                 tr.centre(sc.poses[sc.sid[rows[idx[b]]]]))
                if c is None:
                    continue
                mg["cos"] = min(mg["cos"], abs(c - cosmin))
                found = found or c < cosmin
        status = 0 if found else 3
    changed = int(not np.array_equal(S, given))
    out["rinfo"] = (used, taken, converged, changed)
    out["status"] = status
    if status == 0:
        s = 0.0
        for k in np.flatnonzero(S):
            s = s + errs[k]
        final = obs_of(list(np.flatnonzero(S)))
        out.update(X=X, err=s / int(S.sum()), n_inliers=int(S.sum()), flags=S,
                   cost_in=sum(tr.reproj2(o[1], o[2], X0, o[0])[0] for o in final),
                   cost_out=sum(tr.reproj2(o[1], o[2], X, o[0])[0] for o in final))
    return out


def refine(kp, set_off, cams, poses, tracks, thr, min_angle_deg, rounds, steps):
    """The whole call on a host dict ``tracks`` (points, tinfo, track_off,
    track_rows, obs_inlier, counts[0] = T) -> dict of the outputs of
    posfeat_refine_points, trimmed, plus 'margins', 'cost_in', 'cost_out'."""
    sc = tr.Scene(kp, set_off, cams, poses)
    N, T = int(set_off[-1]), int(tracks["counts"][0])
    off = np.asarray(tracks["track_off"], np.int64)
    M = int(off[T]) if T else 0
    margins = {}
    points, err = np.zeros((T, 3)), np.zeros(T)
    tinfo, rinfo = np.zeros((T, 4), np.int32), np.zeros((T, 4), np.int32)
    flags = np.zeros(M, np.uint8)
    point_of_row = np.full(N, -1, np.int32)
    cost_in, cost_out = np.full(T, np.nan), np.full(T, np.nan)
    for t in range(T):
        sl = slice(int(off[t]), int(off[t + 1]))
        rows = [int(r) for r in tracks["track_rows"][sl]]
        r = refine_track(sc, rows, tracks["obs_inlier"][sl], tracks["points"][t],
                         int(tracks["tinfo"][t][0]), thr, min_angle_deg, rounds, steps, margins)
        points[t], err[t] = r["X"], r["err"]
        tinfo[t] = (r["status"], r["n_inliers"], tracks["tinfo"][t][2], tracks["tinfo"][t][3])
        rinfo[t] = r["rinfo"]
        flags[sl] = r["flags"]
        cost_in[t], cost_out[t] = r["cost_in"], r["cost_out"]
        if r["status"] == 0:
            for row, f in zip(rows, r["flags"]):
                if f:
                    point_of_row[row] = t
    st = tinfo[:, 0]
    counts = np.array([T, int((st == 0).sum()), int(tinfo[st == 0, 1].sum()), int((st == 2).sum()),
                       int((st == 3).sum()), int((st == 1).sum()), int(rinfo[:, 3].sum()), 0],
                      np.int32)
    return dict(points=points, err=err, tinfo=tinfo, rinfo=rinfo, obs_inlier=flags,
                point_of_row=point_of_row, counts=counts,
                track_off=np.asarray(tracks["track_off"][:T + 1], np.int32),
                track_rows=np.asarray(tracks["track_rows"][:M], np.int32), margins=margins,
                cost_in=cost_in, cost_out=cost_out)
