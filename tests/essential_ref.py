"""Numpy restatement of the five-point RANSAC essential-matrix definitions of
include/posfeat_hip.h (posfeat_ransac_essential): sampler, undistortion, the
5x9 elimination with full pivoting, the ten cubic constraints, the Gauss-Jordan
step, the degree-10 polynomial and its Aberth-Ehrlich roots, the Sampson score
in normalised coordinates, selection, the linear refit with its projection onto
the essential manifold, the four decompositions and the cheirality count.
Written from those definitions; float64 throughout.  Shared by the essential
tests; nothing here touches the GPU."""
import numpy as np

import fundamental_ref as FR
from fundamental_ref import sample, sampson, system, unit, jacobi  # noqa: F401  (re-exported)

PIVOT_REL = 1e-12          # of the 5x9 elimination (null2's rule)
GJ_PIVOT_REL = 1e-12       # of the Gauss-Jordan step on the 10x20 matrix
LEAD_REL = 1e-12           # |c10| <= this max |ck|: rejected
ABERTH_SWEEPS = 40
ROOT_IM_TOL = 1e-8         # a root is real iff |Im| <= this max(1, |z|)
NEWTON_STEPS = 2
POLISH_STEPS = 3           # Gauss-Newton steps on the ten cubics per candidate
UNDISTORT_STEPS = 8

# the fixed orthogonal mixing of the eliminated basis (a Householder matrix whose
# last row is (2, 4, 5, 6) / 9): the gauge vector takes part of every free column
_W = np.array([-2.0, -4.0, -5.0, 3.0])
MIX = np.eye(4) - np.outer(_W, _W) / 27.0

# monomials as exponent triples of (x, y, z)
LIN = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
QUAD = [tuple(a + b for a, b in zip(LIN[i], LIN[j])) for i in range(4) for j in range(i, 4)]
CUBIC = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0),
         (1, 1, 1), (1, 1, 0), (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0),
         (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
QI = [[QUAD.index(tuple(a + b for a, b in zip(LIN[i], LIN[j]))) for j in range(4)]
      for i in range(4)]
CI = [[CUBIC.index(tuple(a + b for a, b in zip(QUAD[k], LIN[j]))) for j in range(4)]
      for k in range(10)]
# the fixed starting directions of the root finder: angle 2 pi k / 10 + 0.7
START = [(np.cos(2.0 * np.pi * k / 10.0 + 0.7), np.sin(2.0 * np.pi * k / 10.0 + 0.7))
         for k in range(10)]


def undistort(cam, p):
    """p [n, 2] pixels -> normalised undistorted points [n, 2] (SIMPLE_RADIAL,
    8 Newton steps, as posfeat_triangulate)"""
    p = np.asarray(p, np.float64)
    out = np.zeros_like(p)
    fx, fy, cx, cy, k1 = [float(v) for v in cam[:5]]
    for i in range(p.shape[0]):
        xd, yd = (p[i, 0] - cx) / fx, (p[i, 1] - cy) / fy
        rd = np.hypot(xd, yd)
        if k1 == 0.0 or rd == 0.0:
            out[i] = xd, yd
            continue
        ru = rd
        for _ in range(UNDISTORT_STEPS):
            g = ru * (1.0 + k1 * (ru * ru)) - rd
            d = 1.0 + 3.0 * k1 * (ru * ru)
            if d > 0.0 and np.isfinite(d):
                ru = ru - g / d
        out[i] = (ru / rd) * xd, (ru / rd) * yd
    return out


def rows(kp1, kp2, cam1, cam2):
    """matched pixel rows -> [n, 4] normalised (x, y, u, v); a non-finite point
    makes its whole row NaN"""
    with np.errstate(all="ignore"):
        m = np.concatenate([undistort(cam1, kp1), undistort(cam2, kp2)], 1)
    m[~np.isfinite(m).all(1)] = np.nan
    return m


def thr_norm(cam1, cam2, thr):
    f1, f2 = (cam1[0] + cam1[1]) / 2.0, (cam2[0] + cam2[1]) / 2.0
    return (thr / f1 + thr / f2) / 2.0


def null4(A):
    """the defined elimination on a 5x9 system: the basis [4, 9] (MIX times the
    vectors e_j with 1 at free column 5 + j, 0 at the other free columns) or
    None when rejected"""
    a = np.array(A, np.float64)
    amax = np.abs(a).max()
    if not np.isfinite(amax):
        return None
    perm = list(range(9))
    for s in range(5):
        sub = np.abs(a[s:, s:])
        r, c = np.unravel_index(int(np.argmax(sub)), sub.shape)
        best = sub[r, c]
        r, c = r + s, c + s
        a[[s, r]] = a[[r, s]]
        a[:, [s, c]] = a[:, [c, s]]
        perm[s], perm[c] = perm[c], perm[s]
        if not (best >= PIVOT_REL * amax and best > 0.0):
            return None
        for r in range(s + 1, 5):
            f = a[r, s] / a[s, s]
            a[r, s + 1:] = a[r, s + 1:] - f * a[s, s + 1:]
    out = np.zeros((4, 9))
    for j in range(4):
        z = np.zeros(9)
        z[5 + j] = 1.0
        for c in range(4, -1, -1):
            t = -a[c, 5 + j]
            for k in range(c + 1, 5):
                t = t - a[c, k] * z[k]
            z[c] = t / a[c, c]
        out[j, perm] = z
    return MIX @ out


def _qmul(a, b):
    """a, b [4, ...] -> [10, ...] (any trailing batch axes)"""
    out = np.zeros((10,) + a.shape[1:])
    for i in range(4):
        for j in range(4):
            out[QI[i][j]] += a[i] * b[j]
    return out


def _cacc(out, q, l, s):
    for k in range(10):
        for j in range(4):
            out[CI[k][j]] += s * (q[k] * l[j])


def constraints(Eb):
    """Eb [4, 9] or [4, 9, S] (E = x Eb[0] + y Eb[1] + z Eb[2] + Eb[3]) -> the
    10x20 matrix [10, 20(, S)]: row 0 det E, rows 1 + 3 i + j the entries of 2 E
    E^T E - tr(E E^T) E, over CUBIC"""
    L = [Eb[:, e] for e in range(9)]
    A = np.zeros((10, 20) + Eb.shape[2:])
    m0 = _qmul(L[4], L[8]) - _qmul(L[5], L[7])
    m1 = _qmul(L[3], L[8]) - _qmul(L[5], L[6])
    m2 = _qmul(L[3], L[7]) - _qmul(L[4], L[6])
    _cacc(A[0], m0, L[0], 1.0)
    _cacc(A[0], m1, L[1], -1.0)
    _cacc(A[0], m2, L[2], 1.0)
    G = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            G[i][j] = (_qmul(L[3 * i], L[3 * j]) + _qmul(L[3 * i + 1], L[3 * j + 1])) + \
                _qmul(L[3 * i + 2], L[3 * j + 2])
            G[j][i] = G[i][j]
    tr = (G[0][0] + G[1][1]) + G[2][2]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                _cacc(A[1 + 3 * i + j], G[i][k], L[3 * k + j], 2.0)
            _cacc(A[1 + 3 * i + j], tr, L[3 * i + j], -1.0)
    return A


def gauss_jordan(A):
    """Gauss-Jordan on the first ten columns with partial pivoting; None when a
    pivot is below GJ_PIVOT_REL times the largest entry of A as given"""
    a = np.array(A, np.float64)
    amax = np.abs(a).max()
    if not np.isfinite(amax):
        return None
    for s in range(10):
        r = s + int(np.argmax(np.abs(a[s:, s])))
        best = abs(a[r, s])
        a[[s, r]] = a[[r, s]]
        if not (best >= GJ_PIVOT_REL * amax and best > 0.0):
            return None
        a[s, s:] = a[s, s:] / a[s, s]
        f = a[:, s].copy()
        f[s] = 0.0
        a[:, s + 1:] = a[:, s + 1:] - f[:, None] * a[s, s + 1:][None, :]
        a[:, s] = 0.0
        a[s, s] = 1.0
    return a


def bmatrix(a):
    """rows k = e - z f, l = g - z h, m = i - z j of the reduced matrix [10,
    20(, S)] as polynomials in z (ascending): B[r] = (bx [4], by [4], b1 [5])"""
    B = []
    for p, q in ((4, 5), (6, 7), (8, 9)):
        P, Q = a[p], a[q]
        bx = np.array([P[12], P[11] - Q[12], P[10] - Q[11], -Q[10]])
        by = np.array([P[15], P[14] - Q[15], P[13] - Q[14], -Q[13]])
        b1 = np.array([P[19], P[18] - Q[19], P[17] - Q[18], P[16] - Q[17], -Q[16]])
        B.append((bx, by, b1))
    return B


def _pmul(a, b):
    out = np.zeros((len(a) + len(b) - 1,) + a.shape[1:])
    for i in range(len(a)):
        for j in range(len(b)):
            out[i + j] += a[i] * b[j]
    return out


def poly10(B):
    """det B(z), ascending coefficients [11(, S)]"""
    (b00, b01, b02), (b10, b11, b12), (b20, b21, b22) = B
    return (_pmul(b00, _pmul(b11, b22) - _pmul(b12, b21)) -
            _pmul(b01, _pmul(b10, b22) - _pmul(b12, b20))) + \
        _pmul(b02, _pmul(b10, b21) - _pmul(b11, b20))


def aberth(co):
    """co [11, S] (ascending, degree 10) -> (ok [S], a [10, S] the monic
    coefficients, z [10, S] the complex roots after ABERTH_SWEEPS Gauss-Seidel
    sweeps from the fixed starting points); ok is False where a coefficient is
    not finite or the leading one is too small"""
    co = np.asarray(co, np.float64)
    with np.errstate(all="ignore"):
        cm = np.abs(co).max(0)
        ok = (cm > 0.0) & np.isfinite(co).all(0) & (np.abs(co[10]) > LEAD_REL * cm)
        a = np.where(ok, co[:10] / co[10], 0.0)
        r0 = np.zeros(co.shape[1])
        for k in range(1, 11):
            r0 = np.maximum(r0, np.abs(a[10 - k]) ** (1.0 / k))
        r0 = np.where(r0 > 0.0, r0, 1.0)
        z = [r0 * complex(c, s) for c, s in START]
        for _ in range(ABERTH_SWEEPS):
            for i in range(10):
                p = np.ones_like(z[i])
                dp = np.zeros_like(z[i])
                for k in range(9, -1, -1):
                    dp = dp * z[i] + p
                    p = p * z[i] + a[k]
                w = p / dp
                s = sum(1.0 / (z[i] - z[j]) for j in range(10) if j != i)
                corr = w / (1.0 - w * s)
                go = (p != 0) & np.isfinite(corr.real) & np.isfinite(corr.imag)
                z[i] = np.where(go, z[i] - corr, z[i])
    return ok, a, np.array(z)


def real_roots(a, z):
    """the real roots of one monic polynomial a [10] among its complex roots z
    [10], ascending, after NEWTON_STEPS Newton steps"""
    out = []
    for zi in z:
        if abs(zi.imag) <= ROOT_IM_TOL * max(1.0, abs(zi)):
            x = zi.real
            for _ in range(NEWTON_STEPS):
                p, dp = 1.0, 0.0
                for k in range(9, -1, -1):
                    dp = dp * x + p
                    p = p * x + a[k]
                with np.errstate(all="ignore"):
                    xn = x - p / dp if dp != 0.0 else x
                if dp != 0.0 and np.isfinite(xn):
                    x = xn
            out.append(float(x))
    return sorted(out)


def _peval(c, z):
    v = c[-1]
    for k in range(len(c) - 2, -1, -1):
        v = v * z + c[k]
    return v


def polish(A, x, y, z):
    """POLISH_STEPS Gauss-Newton steps on the ten cubics A mon(x, y, z) = 0 (A the
    10x20 matrix before the elimination): r = A mon, J = A (dmon / dx, dy, dz),
    N = J^T J, g = J^T r, delta = adj(N) g / det N by cofactors; a step with a
    zero determinant or a non-finite result is skipped"""
    for _ in range(POLISH_STEPS):
        px, py, pz = ([1.0, v, v * v, (v * v) * v] for v in (x, y, z))
        mon = np.array([(px[a] * py[b]) * pz[c] for a, b, c in CUBIC])
        d = np.zeros((20, 3))
        for k, (a, b, c) in enumerate(CUBIC):
            d[k, 0] = a * ((px[a - 1] * py[b]) * pz[c]) if a else 0.0
            d[k, 1] = b * ((px[a] * py[b - 1]) * pz[c]) if b else 0.0
            d[k, 2] = c * ((px[a] * py[b]) * pz[c - 1]) if c else 0.0
        r, J = A @ mon, A @ d
        N, g = J.T @ J, J.T @ r
        c0 = np.array([N[1, 1] * N[2, 2] - N[1, 2] * N[1, 2], N[0, 2] * N[1, 2] - N[0, 1] * N[2, 2],
                       N[0, 1] * N[1, 2] - N[0, 2] * N[1, 1]])
        det = (N[0, 0] * c0[0] + N[0, 1] * c0[1]) + N[0, 2] * c0[2]
        c11 = N[0, 0] * N[2, 2] - N[0, 2] * N[0, 2]
        c12 = N[0, 1] * N[0, 2] - N[0, 0] * N[1, 2]
        c22 = N[0, 0] * N[1, 1] - N[0, 1] * N[0, 1]
        dx = ((c0[0] * g[0] + c0[1] * g[1]) + c0[2] * g[2]) / det
        dy = ((c0[1] * g[0] + c11 * g[1]) + c12 * g[2]) / det
        dz = ((c0[2] * g[0] + c12 * g[1]) + c22 * g[2]) / det
        if det != 0.0 and np.isfinite(dx) and np.isfinite(dy) and np.isfinite(dz):
            x, y, z = x - dx, y - dy, z - dz
    return x, y, z


def solve5_batch(ms):
    """ms: a list of [5, 4] normalised row sets -> per set (candidates, the
    polynomial [11], its complex roots [10]); ([], None, None) for a rejected
    sample.  The constraints and the root finder run over all sets at once; the
    arithmetic per set is that of the definition."""
    out = [([], None, None)] * len(ms)
    with np.errstate(all="ignore"):
        live, Ebs = [], []
        for k, m in enumerate(ms):
            m = np.asarray(m, np.float64)
            if not np.isfinite(m).all():
                continue
            Eb = null4(system(m))
            if Eb is not None:
                live.append(k)
                Ebs.append(Eb)
        if not live:
            return out
        A = constraints(np.stack(Ebs, 2))
        red = np.full(A.shape, np.nan)
        for j in range(len(live)):
            a = gauss_jordan(A[:, :, j])
            if a is not None:
                red[:, :, j] = a
        B = bmatrix(red)
        co = poly10(B)
        ok, mono, zc = aberth(co)
        for j, k in enumerate(live):
            if not ok[j]:
                continue
            Eb = Ebs[j]
            cands = []
            for z in real_roots(mono[:, j], zc[:, j]):
                Bz = np.array([[_peval(c[:, j], z) for c in row] for row in B])
                cr = [np.cross(Bz[0], Bz[1]), np.cross(Bz[0], Bz[2]), np.cross(Bz[1], Bz[2])]
                best = 0
                for i in (1, 2):
                    if abs(cr[i][2]) > abs(cr[best][2]):
                        best = i
                x, y = cr[best][0] / cr[best][2], cr[best][1] / cr[best][2]
                x, y, z = polish(A[:, :, j], x, y, z)
                E = ((x * Eb[0] + y * Eb[1]) + z * Eb[2]) + Eb[3]
                ss = (E ** 2).sum()
                if np.isfinite(E).all() and ss > 0.0 and np.isfinite(ss):
                    cands.append(unit(E.reshape(3, 3)))
            if cands:
                out[k] = (cands, co[:, j], zc[:, j])
    return out


def solve5(m, detail=False):
    """m [5, 4] normalised rows -> the candidates [c] of [3, 3] (unit norm,
    largest entry positive) for the real roots ascending; [] for a rejected
    sample.  With detail: (candidates, polynomial, complex roots)."""
    got = solve5_batch([m])[0]
    return got if detail else got[0]


def project(E):
    """onto the essential manifold: (E', U, V) with E' = u1 v1^T + u2 v2^T, V the
    eigenvectors of E^T E by descending eigenvalue (v3 = v1 x v2), u_i = E v_i /
    |E v_i|, u3 = u1 x u2"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    d, W = jacobi(E.T @ E)
    order = sorted(range(3), key=lambda i: -d[i])         # stable: the first of equals first
    v1, v2 = W[:, order[0]], W[:, order[1]]
    v3 = np.cross(v1, v2)
    with np.errstate(all="ignore"):
        u1 = E @ v1
        u1 = u1 / np.sqrt((u1 ** 2).sum())
        u2 = E @ v2
        u2 = u2 / np.sqrt((u2 ** 2).sum())
    u3 = np.cross(u1, u2)
    if u3[int(np.argmax(np.abs(u3)))] < 0:                 # the order that makes u3's first largest
        u1, u2, u3, v1, v2, v3 = u2, u1, -u3, v2, v1, -v3  # entry positive
    return np.outer(u1, v1) + np.outer(u2, v2), np.stack([u1, u2, u3], 1), np.stack([v1, v2, v3], 1)


def refit(mi):
    """mi [k, 4] inlier rows -> (E [3, 3] on the essential manifold, eigenvalues
    of the normal matrix ascending)"""
    A = system(mi)
    d, V = jacobi(A.T @ A)
    Fn = FR.rank2(V[:, int(np.argmin(d))].reshape(3, 3))   # refit_from_normal as it stands
    with np.errstate(all="ignore"):
        E = project(Fn)[0]
    return E, np.sort(d)


W_MAT = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])


def decompositions(E):
    """the four [R | t] in the defined order"""
    _, U, V = project(E)
    Ra, Rb, t = U @ W_MAT @ V.T, U @ W_MAT.T @ V.T, U[:, 2]
    return [np.concatenate([R, s * t[:, None]], 1) for R in (Ra, Rb) for s in (1.0, -1.0)]


def depths(P, m):
    """the two depths of every match between [I | 0] and P"""
    R, t = P[:, :3], P[:, 3]
    x1 = np.concatenate([m[:, :2], np.ones((m.shape[0], 1))], 1)
    a = x1 @ R.T
    u, v = m[:, 2], m[:, 3]
    with np.errstate(all="ignore"):
        p0, p1 = a[:, 0] - u * a[:, 2], a[:, 1] - v * a[:, 2]
        q0, q1 = u * t[2] - t[0], v * t[2] - t[1]
        d1 = (p0 * q0 + p1 * q1) / (p0 * p0 + p1 * p1)
        d2 = d1 * a[:, 2] + t[2]
    return d1, d2


def cheirality(E, m):
    """(pose [3, 4], decomposition index, n_front) over the matches m [k, 4]"""
    with np.errstate(all="ignore"):
        Ps = decompositions(E)
        cnt = []
        for P in Ps:
            d1, d2 = depths(P, m)
            cnt.append(int(np.sum(np.isfinite(d1) & np.isfinite(d2) & (d1 > 0) & (d2 > 0))))
    k = int(np.argmax(cnt))                                # the first of the largest
    return Ps[k], k, cnt[k]


decompose = cheirality


def root_margins(co, zc):
    """(relative separation of the real roots, closest |Im| / tolerance ratio
    as max(r, 1 / r) distance from 1 expressed as a factor) of a scored
    polynomial"""
    sep, factor = np.inf, np.inf
    zc = np.asarray(zc)
    tol = ROOT_IM_TOL * np.maximum(1.0, np.abs(zc))
    real = np.sort(zc[np.abs(zc.imag) <= tol].real)
    if len(real) > 1:
        sep = float(np.min(np.diff(real)) / max(1.0, np.abs(real).max()))
    for im, t in zip(np.abs(zc.imag), tol):
        if im > 0:
            with np.errstate(over="ignore"):
                factor = min(factor, t / im if im <= t else im / t)
    return sep, float(factor)


def hypotheses(m, pair, iters, seed):
    """m [n, 4] normalised rows -> per iteration the list of candidate E,
    samples, smallest real-root separation, smallest |Im| / tolerance factor"""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    if n < 5:
        return [[] for _ in range(iters)], [None] * iters, np.inf, np.inf
    samples = [sample(seed, pair, it, n, 5) for it in range(iters)]
    Es, sep, fac = [], np.inf, np.inf
    for cands, co, zc in solve5_batch([m[idx] for idx in samples]):
        if cands:
            s, f = root_margins(co, zc)
            sep, fac = min(sep, s), min(fac, f)
        Es.append(cands)
    return Es, samples, sep, fac


def finish(m, Es, thr_n):
    """selection, refit, pose and output over the candidates Es (a prefix is the
    run with that many iterations).  m: normalised rows, thr_n: the normalised
    threshold.  margin is relative to thr_n."""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    out = dict(status=1, n_inliers=0, best_iter=-1, root=0, refit_kept=0, E=np.zeros((3, 3)),
               pose=np.zeros((3, 4)), cheir=(-1, 0), mask=np.zeros(n, bool), margin=np.inf,
               eig=None, n_min=0, n_refit=0, mask_min=np.zeros(n, bool))
    best = (-1, -1, -1)

    def score(E):
        d = sampson(E, m)
        ok = np.isfinite(d)
        if ok.any():
            out["margin"] = min(out["margin"], float(np.min(np.abs(d[ok] - thr_n)) / thr_n))
        return ok & (d <= thr_n)

    for it, cands in enumerate(Es):
        for r, E in enumerate(cands):
            cnt = int(score(E).sum())
            if cnt > best[0]:
                best = (cnt, it, r)
    if best[0] < 0:
        return out
    _, it, r = best
    E0 = Es[it][r]
    mask0 = score(E0)
    E1, eig = refit(m[mask0])
    ok1 = bool(mask0.sum() >= 8 and np.all(np.isfinite(E1)) and np.any(E1 != 0))
    mask1 = score(E1) if np.all(np.isfinite(E1)) else np.zeros(n, bool)
    keep = bool(ok1 and mask1.sum() >= mask0.sum())
    E, mask = (unit(E1), mask1) if keep else (E0, mask0)
    pose, k, nf = cheirality(E, m[mask])
    out.update(status=0, n_inliers=int(mask.sum()), best_iter=it, root=r, refit_kept=int(keep),
               E=E, pose=pose, cheir=(k, nf), mask=mask, eig=eig, n_min=int(mask0.sum()),
               n_refit=int(mask1.sum()), mask_min=mask0)
    return out


def ransac(kp1, kp2, cam1, cam2, pair, iters, thr, seed):
    """matched pixel rows kp1, kp2 [n, 2] -> the dict of ``finish``"""
    m = rows(kp1, kp2, cam1, cam2)
    Es, _, _, _ = hypotheses(m, pair, iters, seed)
    return finish(m, Es, thr_norm(cam1, cam2, thr))
