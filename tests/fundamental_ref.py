"""Numpy restatement of the RANSAC fundamental-matrix definitions of
include/posfeat_hip.h (posfeat_ransac_fundamental): sampler, normalisation,
the 7x9 elimination with full pivoting, the cubic and its roots, the Sampson
score, selection, the Jacobi 8-point refit with its rank-2 projection and the
output scaling.  Written from those definitions; float64 throughout.  Shared by
the fundamental-matrix tests; nothing here touches the GPU."""
import numpy as np

from ransac_ref import M64, mix, normalisation

PIVOT_REL = 1e-12
LEAD_REL = 1e-12


def sample(seed, pair, it, n, k=7):
    """the first k distinct indices in [0, n) of iteration ``it`` of pair ``pair``"""
    base = mix(mix((seed & M64) ^ mix(pair)) ^ it)
    out = []
    for i in range(k):
        r = mix(base ^ i)
        j = ((r >> 32) * (n - i)) >> 32
        for prev in sorted(out):
            if j >= prev:
                j += 1
        out.append(j)
    return out


def system(m):
    """m [k, 4] rows (x, y, u, v) -> the k x 9 rows of x2^T F x1 = 0"""
    x, y, u, v = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
    return np.stack([u * x, u * y, u, v * x, v * y, v, x, y, np.ones_like(x)], 1)


def null2(A):
    """the defined elimination on a 7x9 system: (f1, f2) or None when rejected"""
    a = np.array(A, np.float64)
    amax = np.abs(a).max()
    if not np.isfinite(amax):
        return None
    perm = list(range(9))
    for s in range(7):
        sub = np.abs(a[s:, s:])
        r, c = np.unravel_index(int(np.argmax(sub)), sub.shape)    # the first largest, row-major
        best = sub[r, c]
        r, c = r + s, c + s
        a[[s, r]] = a[[r, s]]
        a[:, [s, c]] = a[:, [c, s]]
        perm[s], perm[c] = perm[c], perm[s]
        if not (best >= PIVOT_REL * amax and best > 0.0):
            return None
        for r in range(s + 1, 7):
            f = a[r, s] / a[s, s]
            a[r, s + 1:] = a[r, s + 1:] - f * a[s, s + 1:]
    out = []
    for free, val in ((7, 1.0), (8, -1.0)):
        z = np.zeros(9)
        z[free] = val
        for c in range(6, -1, -1):
            t = -a[c, free] * val
            for k in range(c + 1, 7):
                t = t - a[c, k] * z[k]
            z[c] = t / a[c, c]
        f = np.zeros(9)
        f[perm] = z
        out.append(f)
    return out[0], out[1]


def _triple(a, b, c):
    return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) +
            a[2] * (b[0] * c[1] - b[1] * c[0]))


def cubic_coeffs(f1, f2):
    """c0..c3 of det(l f1 + (1 - l) f2)"""
    B, D = f2.reshape(3, 3), (f1 - f2).reshape(3, 3)
    return np.array([
        _triple(B[0], B[1], B[2]),
        _triple(D[0], B[1], B[2]) + _triple(B[0], D[1], B[2]) + _triple(B[0], B[1], D[2]),
        _triple(D[0], D[1], B[2]) + _triple(D[0], B[1], D[2]) + _triple(B[0], D[1], D[2]),
        _triple(D[0], D[1], D[2])])


def cubic_roots(co):
    """the real roots, ascending, as the header finds them"""
    cm = np.abs(co).max()
    if not (cm > 0.0) or not np.all(np.isfinite(co)):
        return []
    if abs(co[3]) > LEAD_REL * cm:
        a, b, d = co[2] / co[3], co[1] / co[3], co[0] / co[3]
        Q = (a * a - 3.0 * b) / 9.0
        R = ((2.0 * (a * a) - 9.0 * b) * a + 27.0 * d) / 54.0
        Q3 = Q * Q * Q
        if R * R < Q3:
            t = np.arccos(min(1.0, max(-1.0, R / np.sqrt(Q3))))
            sq = -2.0 * np.sqrt(Q)
            roots = [sq * np.cos((t + 2.0 * np.pi * k) / 3.0) - a / 3.0 for k in (0, 1, -1)]
        else:
            A = -np.sign(R) * np.cbrt(abs(R) + np.sqrt(R * R - Q3)) if R != 0 else \
                -np.cbrt(np.sqrt(R * R - Q3))
            roots = [A + (Q / A if A != 0.0 else 0.0) - a / 3.0]
        out = []
        for x in roots:
            for _ in range(2):
                p = ((x + a) * x + b) * x + d
                dp = (3.0 * x + 2.0 * a) * x + b
                if dp != 0.0 and np.isfinite(x - p / dp):
                    x = x - p / dp
            out.append(float(x))
        return sorted(out)
    if abs(co[2]) > LEAD_REL * cm:
        disc = co[1] * co[1] - 4.0 * co[2] * co[0]
        if disc < 0.0:
            return []
        sd = np.sqrt(disc)
        q = -(co[1] + (sd if co[1] >= 0.0 else -sd)) / 2.0
        return sorted([q / co[2], co[0] / q] if q != 0.0 else [0.0, 0.0])
    if abs(co[1]) > LEAD_REL * cm:
        return [-co[0] / co[1]]
    return []


def root_separation(co):
    """smallest distance between two roots (complex ones included) of the
    cubic, relative to the largest root magnitude (at least 1)"""
    r = np.roots(co[::-1])
    if len(r) < 2:
        return np.inf
    d = min(abs(r[i] - r[j]) for i in range(len(r)) for j in range(i))
    return float(d / max(1.0, np.abs(r).max()))


def solve7(m):
    """m [7, 4] normalised rows -> ([Fn [3, 3]] per real root ascending, cubic
    coefficients); ([], None) for a rejected sample"""
    with np.errstate(all="ignore"):
        ns = null2(system(np.asarray(m, np.float64)))
        if ns is None:
            return [], None
        f1, f2 = ns
        co = cubic_coeffs(f1, f2)
        return [(l * f1 + (1.0 - l) * f2).reshape(3, 3) for l in cubic_roots(co)], co


def transforms(nm):
    (c1, s1), (c2, s2) = nm
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]])
    T2 = np.array([[s2, 0, -s2 * c2[0]], [0, s2, -s2 * c2[1]], [0, 0, 1]])
    return T1, T2


def normalise(m, nm):
    (c1, s1), (c2, s2) = nm
    with np.errstate(all="ignore"):                        # coincident points: s = inf, rows NaN
        return np.concatenate([(m[:, :2] - c1) * s1, (m[:, 2:4] - c2) * s2], 1)


def sampson(F, m):
    """Sampson distances in pixels (not squared): m [n, 4] -> [n]"""
    with np.errstate(all="ignore"):
        x1 = np.concatenate([m[:, :2], np.ones((m.shape[0], 1))], 1)
        x2 = np.concatenate([m[:, 2:4], np.ones((m.shape[0], 1))], 1)
        a, b = x1 @ F.T, x2 @ F
        e = (x2 * a).sum(1)
        den = a[:, 0] ** 2 + a[:, 1] ** 2 + b[:, 0] ** 2 + b[:, 1] ** 2
        return np.sqrt(e * e / den)


def unit(F):
    """Frobenius norm 1, the first entry of largest magnitude positive"""
    F = F / np.sqrt((F ** 2).sum())
    return -F if F.reshape(-1)[int(np.argmax(np.abs(F)))] < 0 else F


def jacobi(A, sweeps=16, tol=1e-32):
    """cyclic Jacobi as the header states it: (diagonal, V) with eigenvector j
    the column V[:, j]"""
    a = np.array(A, np.float64)
    n = a.shape[0]
    V = np.eye(n)
    for _ in range(sweeps):
        off = sum(a[p, q] ** 2 for p in range(n) for q in range(p + 1, n))
        if not (off > tol * (np.diag(a) ** 2).sum()):
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = a[p, q]
                if apq == 0.0:
                    continue
                with np.errstate(all="ignore"):
                    theta = (a[q, q] - a[p, p]) / (2.0 * apq)
                    t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                J = np.eye(n)
                J[p, p] = J[q, q] = c
                J[p, q], J[q, p] = s, -s
                a = J.T @ a @ J
                a[p, q] = a[q, p] = 0.0
                V = V @ J
    return np.diag(a).copy(), V


def rank2(Fn):
    d, W = jacobi(Fn.T @ Fn)
    w = W[:, int(np.argmin(d))]
    return Fn - np.outer(Fn @ w, w)


def refit(mn):
    """mn [k, 4] normalised inlier rows -> (Fn [3, 3] of rank 2, eigenvalues of
    the normal matrix ascending)"""
    A = system(mn)
    d, V = jacobi(A.T @ A)
    Fn = V[:, int(np.argmin(d))].reshape(3, 3)
    return rank2(Fn), np.sort(d)


def hypotheses(m, pair, iters, seed):
    """m [n, 4] match rows -> (nm, per iteration the list of candidate F
    (pixels; [] for a rejected sample), samples, smallest root separation over
    the scored cubics)"""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    if n < 7:
        return None, [[] for _ in range(iters)], [None] * iters, np.inf
    nm = (normalisation(m[:, :2]), normalisation(m[:, 2:4]))
    T1, T2 = transforms(nm)
    mn = normalise(m, nm)
    Fs, samples, sep = [], [], np.inf
    for it in range(iters):
        idx = sample(seed, pair, it, n, 7)
        samples.append(idx)
        cands, co = solve7(mn[idx])
        if cands:
            sep = min(sep, root_separation(co))
        Fs.append([T2.T @ Fn @ T1 for Fn in cands])
    return nm, Fs, samples, sep


def finish(m, nm, Fs, thr):
    """selection, refit and output over the candidates Fs (a prefix of what
    ``hypotheses`` gave is the run with that many iterations).  Returns a dict:
    status, n_inliers, best_iter, root, refit_kept, F, mask, margin (closest
    Sampson distance to thr over everything scored), eig (of the refit's normal
    matrix, ascending), n_min / n_refit."""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    out = dict(status=1, n_inliers=0, best_iter=-1, root=0, refit_kept=0, F=np.zeros((3, 3)),
               mask=np.zeros(n, bool), margin=np.inf, eig=None, n_min=0, n_refit=0)
    best = (-1, -1, -1)
    for it, cands in enumerate(Fs):
        for r, F in enumerate(cands):
            d = sampson(F, m)
            ok = np.isfinite(d)
            cnt = int(np.sum(ok & (d <= thr)))
            if ok.any():
                out["margin"] = min(out["margin"], float(np.min(np.abs(d[ok] - thr))))
            if cnt > best[0]:                              # the first of the largest
                best = (cnt, it, r)
    if best[0] < 0:
        return out
    _, it, r = best
    F0 = Fs[it][r]
    d = sampson(F0, m)
    mask0 = np.isfinite(d) & (d <= thr)
    T1, T2 = transforms(nm)
    Fn, eig = refit(normalise(m[mask0], nm))
    F1 = T2.T @ Fn @ T1
    d = sampson(F1, m)
    ok = np.isfinite(d)
    if ok.any():
        out["margin"] = min(out["margin"], float(np.min(np.abs(d[ok] - thr))))
    mask1 = ok & (d <= thr)
    keep = bool(mask0.sum() >= 8 and np.all(np.isfinite(F1)) and np.any(F1 != 0) and
                mask1.sum() >= mask0.sum())
    F, mask = (F1, mask1) if keep else (F0, mask0)
    out.update(status=0, n_inliers=int(mask.sum()), best_iter=it, root=r, refit_kept=int(keep),
               F=unit(F), mask=mask, eig=eig, n_min=int(mask0.sum()), n_refit=int(mask1.sum()))
    return out


def ransac(m, pair, iters, thr, seed):
    nm, Fs, _, _ = hypotheses(m, pair, iters, seed)
    return finish(m, nm, Fs, thr)
