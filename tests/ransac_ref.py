"""Numpy restatement of the RANSAC homography definitions of
include/posfeat_hip.h (posfeat_ransac_homography): sampler, normalisation,
degeneracy test, minimal solve, score, selection, refit, output scaling.
Written from those definitions; float64 throughout, Python integers for the
uint64 sampler.  Shared by the RANSAC tests; nothing here touches the GPU."""
import numpy as np

M64 = (1 << 64) - 1


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample(seed, pair, it, n):
    """the four distinct indices in [0, n) of iteration ``it`` of pair ``pair``"""
    base = mix(mix((seed & M64) ^ mix(pair)) ^ it)
    out = []
    for k in range(4):
        r = mix(base ^ k)
        j = ((r >> 32) * (n - k)) >> 32
        for prev in sorted(out):
            if j >= prev:
                j += 1
        out.append(j)
    return out


def normalisation(xy):
    """(centroid [2], scale): mean distance to the centroid becomes sqrt 2"""
    c = xy.mean(0)
    d = np.sqrt(((xy - c) ** 2).sum(1)).mean()
    with np.errstate(divide="ignore"):
        return c, np.sqrt(2.0) / d


def solve8(A, b):
    """Gaussian elimination with partial pivoting (first largest entry); None
    when a pivot is below 1e-12 times the largest entry of its column of A"""
    a = np.concatenate([A, b[:, None]], 1).astype(np.float64)
    cmax = np.abs(A).max(0)
    ok = True
    with np.errstate(all="ignore"):
        for c in range(8):
            piv = c + int(np.argmax(np.abs(a[c:, c])))
            best = abs(a[piv, c])
            if piv != c:
                a[[c, piv]] = a[[piv, c]]
            ok = ok and bool(best >= 1e-12 * cmax[c]) and bool(best > 0.0)
            f = a[c + 1:, c] / a[c, c]
            a[c + 1:, c + 1:] = a[c + 1:, c + 1:] - f[:, None] * a[c, c + 1:][None, :]
        x = np.zeros(8)
        for c in range(7, -1, -1):
            s = a[c, 8]
            for k in range(c + 1, 8):
                s = s - a[c, k] * x[k]
            x[c] = s / a[c, c]
    return x if ok and np.all(np.isfinite(x)) else None


def dlt_system(m, nm):
    """the 2 k x 8 system and right-hand side of matches m [k, 4] (x1 y1 x2 y2)"""
    (c1, s1), (c2, s2) = nm
    x, y = (m[:, 0] - c1[0]) * s1, (m[:, 1] - c1[1]) * s1
    u, v = (m[:, 2] - c2[0]) * s2, (m[:, 3] - c2[1]) * s2
    k = m.shape[0]
    A = np.zeros((2 * k, 8))
    A[0::2, 0], A[0::2, 1], A[0::2, 2] = x, y, 1.0
    A[0::2, 6], A[0::2, 7] = -(u * x), -(u * y)
    A[1::2, 3], A[1::2, 4], A[1::2, 5] = x, y, 1.0
    A[1::2, 6], A[1::2, 7] = -(v * x), -(v * y)
    b = np.zeros(2 * k)
    b[0::2], b[1::2] = u, v
    return A, b


def denormalise(x, nm):
    (c1, s1), (c2, s2) = nm
    Hn = np.append(x, 1.0).reshape(3, 3)
    T1 = np.array([[s1, 0, -s1 * c1[0]], [0, s1, -s1 * c1[1]], [0, 0, 1]])
    T2i = np.array([[1 / s2, 0, c2[0]], [0, 1 / s2, c2[1]], [0, 0, 1]])
    return T2i @ Hn @ T1


def degenerate(m):
    """m [4, 4]: any of the four triples collinear in an image, or turning the
    other way round in the other image"""
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        cr = []
        for o in (0, 2):
            a, b = m[j, o:o + 2] - m[i, o:o + 2], m[k, o:o + 2] - m[i, o:o + 2]
            c = a[0] * b[1] - a[1] * b[0]
            if abs(c) <= 1e-6 * np.sqrt(a @ a) * np.sqrt(b @ b):
                return True
            cr.append(c)
        if (cr[0] > 0) != (cr[1] > 0):
            return True
    return False


def residuals(H, m):
    """the distances of posfeat_reproj_hist: m [n, 4] -> [n]"""
    with np.errstate(all="ignore"):
        p = np.concatenate([m[:, :2], np.ones((m.shape[0], 1))], 1) @ H.T
        d = m[:, 2:4] - p[:, :2] / p[:, 2:]
        return np.sqrt((d ** 2).sum(1))


def inliers(H, m, thr):
    r = residuals(H, m)
    return np.isfinite(r) & (r <= thr)


def hypotheses(m, pair, iters, seed):
    """m [n, 4] float32/64 match rows -> (nm, [H or None] * iters, samples)"""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    if n < 4:
        return None, [None] * iters, [None] * iters
    nm = (normalisation(m[:, :2]), normalisation(m[:, 2:4]))
    Hs, samples = [], []
    for it in range(iters):
        idx = sample(seed, pair, it, n)
        samples.append(idx)
        s = m[idx]
        if degenerate(s):
            Hs.append(None)
            continue
        x = solve8(*dlt_system(s, nm))
        Hs.append(None if x is None else denormalise(x, nm))
    return nm, Hs, samples


def unit(H):
    H = H / np.sqrt((H ** 2).sum())
    return -H if H[2, 2] < 0 else H


def finish(m, nm, Hs, thr):
    """selection, refit and output over the hypotheses Hs (a prefix of what
    ``hypotheses`` gave is the run with that many iterations).  Returns a dict:
    status, n_inliers, best_iter, refit_kept, H, mask, counts (per hypothesis,
    -1 rejected), margin (closest residual to thr over everything scored),
    cond (of the refit's normal equations), n_min / n_refit."""
    m = np.asarray(m, np.float64)
    n = m.shape[0]
    out = dict(status=1, n_inliers=0, best_iter=-1, refit_kept=0, H=np.zeros((3, 3)),
               mask=np.zeros(n, bool), counts=np.full(len(Hs), -1), margin=np.inf, cond=np.nan,
               n_min=0, n_refit=0)
    for it, H in enumerate(Hs):
        if H is None:
            continue
        r = residuals(H, m)
        out["counts"][it] = int(np.sum(np.isfinite(r) & (r <= thr)))
        out["margin"] = min(out["margin"], float(np.min(np.abs(r[np.isfinite(r)] - thr))))
    if out["counts"].max(initial=-1) < 0:
        return out
    best = int(np.argmax(out["counts"]))                   # the first of the largest
    H0 = Hs[best]
    mask0 = inliers(H0, m, thr)
    A, b = dlt_system(m[mask0], nm)
    N, rhs = A.T @ A, A.T @ b
    out["cond"] = float(np.linalg.cond(N))
    x = solve8(N, rhs)
    keep, H, mask = False, H0, mask0
    out["n_min"] = int(mask0.sum())
    if x is not None:
        H1 = denormalise(x, nm)
        r = residuals(H1, m)
        out["margin"] = min(out["margin"], float(np.min(np.abs(r[np.isfinite(r)] - thr))))
        mask1 = np.isfinite(r) & (r <= thr)
        out["n_refit"] = int(mask1.sum())
        if mask1.sum() >= mask0.sum():
            keep, H, mask = True, H1, mask1
    out.update(status=0, n_inliers=int(mask.sum()), best_iter=best, refit_kept=int(keep),
               H=unit(H), mask=mask)
    return out


def ransac(m, pair, iters, thr, seed):
    nm, Hs, _ = hypotheses(m, pair, iters, seed)
    return finish(m, nm, Hs, thr)


def warp(H, pts):
    p = np.concatenate([pts, np.ones((pts.shape[0], 1))], 1) @ np.asarray(H, np.float64).T
    return p[:, :2] / p[:, 2:]


def corner_error(H_a, H_b, w, h):
    """mean distance between the four corners of a w x h image warped by the
    two homographies"""
    c = np.array([[0, 0], [w - 1, 0], [w - 1, h - 1], [0, h - 1]], np.float64)
    with np.errstate(all="ignore"):
        return float(np.mean(np.sqrt(((warp(H_a, c) - warp(H_b, c)) ** 2).sum(1))))
