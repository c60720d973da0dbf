"""Numpy restatement of the absolute-pose definitions of include/posfeat_hip.h
(posfeat_ransac_pose): the sample, its rejections, Grunert's quartic and its
closed-form roots, the candidate poses, the score, the selection, the
Gauss-Newton refit and the outputs.  Written from those definitions in plain
loops; float64 throughout.  The camera model is triangulate_ref's.  Shared by
the pose tests; nothing here touches the GPU.

Where a decision has a threshold the functions collect the closest distance to
it in a ``margins`` dict: 'err' (|e - thr| in pixels over everything scored),
'depth' (|z| over every finite depth scored)."""
import numpy as np

import triangulate_ref as tr
from fundamental_ref import cubic_roots
from ransac_ref import sample as sample4

COLLINEAR_REL, BEARING_COS, LEAD_REL, ROOT_GAP = 1e-6, 1.0 - 1e-12, 1e-12, 1e-9
GN_STEPS, GN_MIN_INLIERS, GN_PIVOT_REL, GN_STOP = 10, 4, 1e-12, 1e-12
MIN_CORR = 4


# ---- the minimal solve ------------------------------------------------------------

def bearings(m):
    f = np.concatenate([m[:, :2], np.ones((3, 1))], 1)
    return f / np.sqrt((f * f).sum(1))[:, None]


def rejected(m):
    """the sample-level rejections: non-finite, collinear points, coincident bearings"""
    m = np.asarray(m, np.float64)
    if not np.all(np.isfinite(m)):
        return True
    P, f = m[:, 2:5], bearings(m)
    d12, d13 = P[1] - P[0], P[2] - P[0]
    if not np.linalg.norm(np.cross(d12, d13)) > COLLINEAR_REL * (np.linalg.norm(d12) * np.linalg.norm(d13)):
        return True
    return bool(f[1] @ f[2] >= BEARING_COS or f[0] @ f[2] >= BEARING_COS or f[0] @ f[1] >= BEARING_COS)


def quartic(m):
    """Grunert's quartic in v = s3 / s1: (A[0..4] ascending powers, the
    constants k, cb, cg, ca, b2 the depths need)"""
    m = np.asarray(m, np.float64)
    P, f = m[:, 2:5], bearings(m)
    a2, b2, c2 = ((P[1] - P[2]) ** 2).sum(), ((P[0] - P[2]) ** 2).sum(), ((P[0] - P[1]) ** 2).sum()
    ca, cb, cg = f[1] @ f[2], f[0] @ f[2], f[0] @ f[1]
    k, mm = (a2 - c2) / b2, (a2 + c2) / b2
    A4 = (k - 1) ** 2 - 4 * (c2 / b2) * ca ** 2
    A3 = 4 * (k * (1 - k) * cb - (1 - mm) * ca * cg + 2 * (c2 / b2) * ca ** 2 * cb)
    A2 = 2 * (k * k - 1 + 2 * k * k * cb ** 2 + 2 * ((b2 - c2) / b2) * ca ** 2 - 4 * mm * ca * cb * cg +
              2 * ((b2 - a2) / b2) * cg ** 2)
    A1 = 4 * (-k * (1 + k) * cb + 2 * (a2 / b2) * cg ** 2 * cb - (1 - mm) * ca * cg)
    A0 = (1 + k) ** 2 - 4 * (a2 / b2) * cg ** 2
    return np.array([A0, A1, A2, A3, A4]), (k, cb, cg, ca, b2)


def _polish_sort(A, roots):
    out = []
    for x in roots:
        for _ in range(2):
            f = (((A[4] * x + A[3]) * x + A[2]) * x + A[1]) * x + A[0]
            df = ((4 * A[4] * x + 3 * A[3]) * x + 2 * A[2]) * x + A[1]
            if df != 0.0 and np.isfinite(x - f / df):
                x = x - f / df
        out.append(float(x))
    out.sort()
    kept = []
    for x in out:
        if kept and x - kept[-1] <= ROOT_GAP * max(1.0, abs(x)):
            continue
        kept.append(x)
    return kept


def quartic_roots(A):
    """the real roots, ascending, as the header finds them: Ferrari through the
    resolvent cubic, two Newton steps, duplicates dropped"""
    A = np.asarray(A, np.float64)
    cm = np.abs(A).max()
    if not (cm > 0.0) or not np.all(np.isfinite(A)):
        return []
    with np.errstate(all="ignore"):
        if abs(A[4]) > LEAD_REL * cm:
            rev = abs(A[0]) > abs(A[4])                        # the larger end leads
            B = A[::-1] if rev else A
            a, b, c, d = B[3] / B[4], B[2] / B[4], B[1] / B[4], B[0] / B[4]
            p = b - 0.375 * a * a
            q = c - 0.5 * a * b + 0.125 * a ** 3
            r = d - 0.25 * a * c + 0.0625 * a * a * b - (3.0 / 256.0) * a ** 4
            lam = cubic_roots(np.array([-(q * q), 2 * p * p - 8 * r, 8 * p, 8.0]))
            m = lam[-1] if lam else np.inf
            ys = []
            if m > 0.0 and np.isfinite(m):
                s, h, w = np.sqrt(2 * m), 0.5 * p + m, q / (2 * np.sqrt(2 * m))
                for B, C in ((s, h - w), (-s, h + w)):
                    disc = s * s - 4 * C
                    if disc >= 0.0:
                        t = -0.5 * (B + np.sign(B) * np.sqrt(disc))
                        ys += [t, C / t]
            else:
                disc = p * p - 4 * r
                if disc >= 0.0:
                    sd = np.sqrt(disc)
                    t = -0.5 * (p + (sd if p >= 0.0 else -sd))
                    for z in (t, (r / t if t != 0.0 else 0.0)):
                        if z >= 0.0:
                            ys += [np.sqrt(z), -np.sqrt(z)]
            roots = [y - 0.25 * a for y in ys]
            if rev:
                roots = [1.0 / x for x in roots if x != 0.0]
        else:
            roots = cubic_roots(A[:4])
        return _polish_sort(A, [x for x in roots if np.isfinite(x)])


def quartic_roots_numpy(A):
    """the independent route: np.roots (companion-matrix eigenvalues), the
    real ones by |imag| <= 1e-9 max(1, |root|), then the same polish"""
    r = np.roots(np.asarray(A, np.float64)[::-1])
    real = [float(z.real) for z in r if abs(z.imag) <= 1e-9 * max(1.0, abs(z))]
    return _polish_sort(A, real)


def root_separation(A):
    """smallest distance between two roots of the quartic (complex ones
    included) relative to max(1, the larger magnitude)"""
    r = np.roots(np.asarray(A, np.float64)[::-1])
    if len(r) < 2:
        return np.inf
    return float(min(abs(r[i] - r[j]) / max(1.0, abs(r[i]), abs(r[j]))
                     for i in range(len(r)) for j in range(i)))


def triad(A, B, C):
    e1 = (B - A) / np.linalg.norm(B - A)
    e3 = np.cross(e1, C - A)
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3], 1)             # columns


def p3p(m, roots=quartic_roots):
    """m [3, 5] = (xu, yu, X, Y, Z) -> the candidate poses [c, 3, 4] in
    ascending root order (c = 0: rejected)"""
    m = np.asarray(m, np.float64)
    if rejected(m):
        return np.zeros((0, 3, 4))
    P, f = m[:, 2:5], bearings(m)
    A, (k, cb, cg, ca, b2) = quartic(m)
    out = []
    Tw = triad(P[0], P[1], P[2])
    with np.errstate(all="ignore"):
        for v in roots(A):
            u = ((k - 1) * v * v - 2 * k * cb * v + 1 + k) / (2 * (cg - v * ca))
            s1 = np.sqrt(b2 / (1 + v * v - 2 * v * cb))
            if not (v > 0 and u > 0 and np.isfinite(u) and s1 > 0 and np.isfinite(s1)):
                continue
            Q = np.stack([s1 * f[0], u * s1 * f[1], v * s1 * f[2]])
            R = triad(Q[0], Q[1], Q[2]) @ Tw.T
            pose = np.concatenate([R, (Q[0] - R @ P[0])[:, None]], 1)
            if np.all(np.isfinite(pose)):
                out.append(pose)
    return np.asarray(out).reshape(-1, 3, 4)


# ---- score ----------------------------------------------------------------------------

def reproj(cam, pose, X, xy):
    """(squared pixel errors [n], depths [n]) of the points X [n, 3] against the
    pixels xy [n, 2]: triangulate_ref.project, elementwise"""
    fx, fy, cx, cy, k1 = (float(v) for v in cam[:5])
    P = np.asarray(pose, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        Xc = X @ P[:, :3].T + P[:, 3]
        z = Xc[:, 2]
        xn, yn = Xc[:, 0] / z, Xc[:, 1] / z
        f = 1.0 + k1 * (xn * xn + yn * yn)
        dx, dy = (fx * f * xn + cx) - xy[:, 0], (fy * f * yn + cy) - xy[:, 1]
        return dx * dx + dy * dy, z


def flags_of(cam, pose, X, xy, thr, mg=None):
    with np.errstate(all="ignore"):
        e2, z = reproj(cam, pose, X, xy)
        if mg is not None:
            fin = np.isfinite(z)
            if fin.any():
                mg["depth"] = min(mg.get("depth", np.inf), float(np.abs(z[fin]).min()))
            scored = np.isfinite(e2) & (z > 0)
            if scored.any():
                mg["err"] = min(mg.get("err", np.inf), float(np.abs(np.sqrt(e2[scored]) - thr).min()))
        return (z > 0.0) & np.isfinite(e2) & (e2 <= thr * thr)


# ---- the refit ------------------------------------------------------------------------

def gn_normal(cam, pose, X, xy):
    """(N [6, 6], g [6], cost, bad rows) over the rows given"""
    fx, fy, cx, cy, k1 = (float(v) for v in cam[:5])
    P = np.asarray(pose, np.float64).reshape(3, 4)
    with np.errstate(all="ignore"):
        Xc = X @ P[:, :3].T + P[:, 3]
        xc, yc, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        xn, yn = xc / z, yc / z
        f = 1.0 + k1 * (xn * xn + yn * yn)
        rx, ry = (fx * f * xn + cx) - xy[:, 0], (fy * f * yn + cy) - xy[:, 1]
        axx, axy = fx * (f + 2 * k1 * xn * xn), fx * 2 * k1 * xn * yn
        ayx, ayy = fy * 2 * k1 * xn * yn, fy * (f + 2 * k1 * yn * yn)
        jx = np.stack([axx / z, axy / z, -(axx * xn + axy * yn) / z], 1)
        jy = np.stack([ayx / z, ayy / z, -(ayx * xn + ayy * yn) / z], 1)
        Ja = np.concatenate([np.cross(Xc, jx), jx], 1)         # jx . (omega x Xc) = omega . (Xc x jx)
        Jb = np.concatenate([np.cross(Xc, jy), jy], 1)
        N = Ja.T @ Ja + Jb.T @ Jb
        g = Ja.T @ rx + Jb.T @ ry
        e2 = rx * rx + ry * ry
        bad = int((~((z > 0) & np.isfinite(e2))).sum())
        return N, g, float(e2.sum()), bad


def gn_solve(N, g):
    a = np.concatenate([N, -g[:, None]], 1).astype(np.float64)
    cmax = np.abs(N).max(0)
    ok = True
    with np.errstate(all="ignore"):
        for c in range(6):
            piv = c + int(np.argmax(np.abs(a[c:, c])))
            best = abs(a[piv, c])
            if piv != c:
                a[[c, piv]] = a[[piv, c]]
            ok = ok and bool(best >= GN_PIVOT_REL * cmax[c]) and bool(best > 0.0)
            fac = a[c + 1:, c] / a[c, c]
            a[c + 1:, c + 1:] = a[c + 1:, c + 1:] - fac[:, None] * a[c, c + 1:][None, :]
        x = np.zeros(6)
        for c in range(5, -1, -1):
            x[c] = (a[c, 6] - a[c, c + 1:6] @ x[c + 1:]) / a[c, c]
    return x if ok and np.all(np.isfinite(x)) else None


def rodrigues(w):
    th = float(np.sqrt(w @ w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    A = np.sin(th) / th if th > 0 else 1.0
    B = 2 * np.sin(0.5 * th) ** 2 / (th * th) if th > 0 else 0.5
    return np.eye(3) + A * K + B * (K @ K)


def refit(cam, pose, X, xy):
    """Gauss-Newton over the rows given from ``pose`` -> (pose, accepted steps,
    the final normal matrix)"""
    P = np.asarray(pose, np.float64).reshape(3, 4).copy()
    N, g, cost, _ = gn_normal(cam, P, X, xy)
    taken = 0
    for _ in range(GN_STEPS):
        d = gn_solve(N, g)
        if d is None:
            break
        E = rodrigues(d[:3])
        Q = np.concatenate([E @ P[:, :3], (E @ P[:, 3] + d[3:])[:, None]], 1)
        N1, g1, cost1, bad1 = gn_normal(cam, Q, X, xy)
        if not (bad1 == 0 and cost1 < cost):
            break
        P, N, g, cost = Q, N1, g1, cost1
        taken += 1
        if np.abs(d).max() <= GN_STOP:
            break
    return P, taken, N


# ---- the call -------------------------------------------------------------------------

def gather(kp, cam, points, corr):
    """the rows of one query: (xy [n, 2], und [n, 2], X [n, 3]); a
    correspondence out of range or not finite is all NaN"""
    kp = np.asarray(kp, np.float32).astype(np.float64)
    n = len(corr)
    xy, und, X = np.full((n, 2), np.nan), np.full((n, 2), np.nan), np.full((n, 3), np.nan)
    for i, (r, pt) in enumerate(np.asarray(corr, np.int64).reshape(-1, 2)):
        if not (0 <= r < len(kp) and 0 <= pt < len(points)):
            continue
        u = tr.undistort(cam, kp[r, 0], kp[r, 1])
        if np.all(np.isfinite(kp[r])) and np.all(np.isfinite(u)) and np.all(np.isfinite(points[pt])):
            xy[i], und[i], X[i] = kp[r], u, points[pt]
    return xy, und, X


def ransac_query(cam, xy, und, X, q, iters, thr, seed, margins=None):
    """One query -> dict(status, pose [12], info [4], flags [n], eig_ratio,
    steps, winner [3, 4])"""
    n = len(xy)
    mg = margins if margins is not None else {}
    out = dict(status=1, pose=np.zeros(12), info=np.array([1, 0, -1, 0], np.int32),
               flags=np.zeros(n, np.uint8), eig_ratio=np.nan, steps=0, winner=None)
    if n < MIN_CORR:
        return out
    best, cache = (-1, -1, -1, None), {}
    for it in range(iters):
        idx = tuple(sample4(seed, q, it, n)[:3])
        if idx not in cache:                                   # the solve depends on the rows alone
            m = np.concatenate([und[list(idx)], X[list(idx)]], 1)
            cache[idx] = [(P, int(flags_of(cam, P, X, xy, thr, mg).sum())) for P in p3p(m)]
        for root, (P, cnt) in enumerate(cache[idx]):
            if cnt > best[0]:
                best = (cnt, it, root, P)
    if best[0] < 0:
        return out
    c0, it0, root0, P0 = best
    f0 = flags_of(cam, P0, X, xy, thr)
    pose, flags, keep, cnt = P0, f0, 0, c0
    if c0 >= GN_MIN_INLIERS:
        P1, steps, N = refit(cam, P0, X[f0], xy[f0])
        ev = np.linalg.eigvalsh(N)
        out.update(steps=steps)
        f1 = flags_of(cam, P1, X, xy, thr, mg)
        if np.all(np.isfinite(P1)) and int(f1.sum()) >= c0:
            pose, flags, keep, cnt = P1, f1, 1, int(f1.sum())
            out.update(eig_ratio=float(ev[0] / ev[-1]))
    out.update(status=0, pose=pose.reshape(-1), flags=flags.astype(np.uint8), winner=P0,
               info=np.array([0, cnt, it0, keep | (root0 << 8)], np.int32))
    return out


def ransac_pose(kp, cams, points, corr, q_off, iters, thr, seed):
    """The whole call -> dict(poses [nq, 12], info [nq, 4], inlier [C],
    margins, eig_ratio [nq] (nan where no refit was kept), winners)"""
    nq = len(q_off) - 1
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    poses, info = np.zeros((nq, 12)), np.zeros((nq, 4), np.int32)
    inlier, margins = np.zeros(int(q_off[-1]), np.uint8), {}
    eig, winners = np.full(nq, np.nan), []
    for q in range(nq):
        rows = slice(int(q_off[q]), int(q_off[q + 1]))
        xy, und, X = gather(kp, cams[q], np.asarray(points, np.float64), corr[rows])
        r = ransac_query(cams[q], xy, und, X, q, iters, thr, seed, margins)
        poses[q], info[q], inlier[rows], eig[q] = r["pose"], r["info"], r["flags"], r["eig_ratio"]
        winners.append(r["winner"])
    return dict(poses=poses, info=info, inlier=inlier, margins=margins, eig_ratio=eig,
                winners=winners)


# ---- planting -------------------------------------------------------------------------

def random_rotation(rs):
    q = rs.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def planted_sample(rs):
    """a random pose and three points in front of it: (m [3, 5] with exact fp64
    bearings, pose [3, 4])"""
    R, C = random_rotation(rs), rs.uniform(-1, 1, 3)
    Xc = np.stack([rs.uniform(-0.6, 0.6, 3), rs.uniform(-0.45, 0.45, 3), np.ones(3)], 1) * \
        rs.uniform(3, 9, 3)[:, None]
    t = -R @ C
    Xw = (Xc - t) @ R                                          # R^T (Xc - t)
    m = np.concatenate([Xc[:, :2] / Xc[:, 2:], Xw], 1)
    return m, np.concatenate([R, t[:, None]], 1)


def pose_error(P, Q):
    """largest entry difference of R and of t / max(1, |t|_inf)"""
    P, Q = np.asarray(P).reshape(3, 4), np.asarray(Q).reshape(3, 4)
    return max(np.abs(P[:, :3] - Q[:, :3]).max(),
               np.abs(P[:, 3] - Q[:, 3]).max() / max(1.0, np.abs(Q[:, 3]).max()))
