"""Robust two-view model fitting on the GPU (ransac.hip, fundamental.hip,
essential.hip): RANSAC homographies, fundamental matrices or five-point
essential matrices with relative poses for every pair of a pair list in a fixed
number of launches, on the matches matchers.match_pairs_device left on the device;
tracks with one triangulated point each from the verified matches
(triangulate.hip); those points refined by points-only bundle adjustment
(refine.hip); absolute poses of queries against them (pose.hip).  The
definitions (sampler, degeneracy test, minimal solve,
score, selection, refit) are in include/posfeat_hip.h; no CPU path.

  ransac_homography_pairs(kp_pool, batch, iters=1024, thr=3.0, seed=0)
        -> (H [npairs, 3, 3] fp64, info [npairs, 4] int32, inlier [sum n1] uint8)
        device tensors, stream-ordered, nothing read back.  info[p] =
        (status, n_inliers, best_iter, refit_kept); pair p's rows of ``inlier``
        start at ``batch.moff[p]``.
  find_homography(kp1, kp2, matches, iters=1024, thr=3.0, seed=0)
        one pair, numpy in and out: (H [3, 3], mask [m] bool, info [4]).
  ransac_fundamental_pairs(kp_pool, batch, iters=2048, thr=4.0, seed=0)
        -> (F [npairs, 3, 3] fp64, info, inlier), as above; thr is a Sampson
        distance in pixels and info[p, 3] = refit_kept | root << 8.
  find_fundamental(kp1, kp2, matches, iters=2048, thr=4.0, seed=0)
        one pair, numpy in and out: (F [3, 3], mask [m] bool, info [4]).
  guided_pairs(kp_pool, batch, model, M, thr, matcher="mnn", ratio=0.95)
        -> PairBatch: posfeat_match_pairs_guided (matchpairs.hip) on the tables
        of ``batch``: the matchers again, each descriptor competing only against
        the keypoints the pair's verified H or F admits within thr pixels.
        guided_record / guided_admissible are its host-only record and predicate.
  ransac_essential_pairs(kp_pool, cams, batch, iters=1024, thr=4.0, seed=0)
        -> (E [npairs, 3, 3] fp64, pose [npairs, 3, 4] fp64, info [npairs, 4],
        cheir [npairs, 2] int32, inlier): posfeat_ransac_essential
        (essential.hip) between calibrated cameras, cams [nsets, 8] fp64 device
        rows (fx, fy, cx, cy, k1, 0, 0, 0); device tensors, nothing read back.
        pose[p] = [R | t] with x2 ~ R x1 + t, |t| = 1; cheir[p] = (decomposition
        index, matches in front of both cameras).
  find_essential(kp1, kp2, cam1, cam2, matches, iters=1024, thr=4.0, seed=0)
        one pair, numpy in and out: (E [3, 3], pose [3, 4], mask [m] bool,
        info [4]).
  solve5(m)
        the five-point candidates [c, 3, 3] (c = 0..10) of five matches m [5, 4]
        in normalised camera coordinates (host only, needs no device).
  decompose_essential(E, m)
        (pose [3, 4], decomposition index, n_front) of E over the matches m
        [n, 4] in normalised camera coordinates (host only, needs no device).
  sample_indices(seed, pair, it, n, k=4)
        the first k match indices (4 for a homography, 5 for an essential, 7
        for a fundamental matrix) iteration ``it`` of pair ``pair`` draws from ``n`` matches (host
        only, needs no device).
  solve7(m)
        the 7-point candidates [c, 3, 3] (c = 0..3) of seven matches m [7, 4] in
        normalised coordinates (host only, needs no device).
  triangulate_tracks(kp_pool, set_off, cams, poses, edges, iters=64, thr=4.0,
                     min_angle=1.5, max_track=256, seed=0) -> TrackResult
        posfeat_triangulate (triangulate.hip): feature tracks from match edges
        and one RANSAC-triangulated point per track, device tensors in and out,
        nothing read back; ``.host()`` brings everything back in one copy.
  track_edges(batch, inlier)
        the global-row edges [sum n1, 2] int32 of a PairBatch and its RANSAC
        mask (device, torch ops only; -1 rows where there is no inlier match).
  triangulate_dlt(obs)
        the DLT of obs [n, 14] = (xu, yu, pose) rows (host only, needs no
        device): X [3], or None for a rejected system.
  refine_tracks(kp_pool, set_off, cams, poses, tracks, thr=4.0, min_angle=1.5,
                rounds=3, steps=10) -> RefinedTrackResult
        posfeat_refine_points (refine.hip): Levenberg-Marquardt on the pixel
        reprojection error of every track's point over its inliers, the inlier
        test again, up to ``rounds`` times, then COLMAP's angle filter; device
        tensors in and out, nothing read back.  A TrackResult with ``rinfo``
        that shares track_off and track_rows with ``tracks``.
  refine_point(obs, X0, steps=10)
        one Levenberg-Marquardt round over obs [n, 22] = (x, y, cam, pose) rows
        from X0 (host only, needs no device): (X [3], cost, taken steps).
  ransac_pose_queries(kp_pool, cams, points, corr, q_off, iters=1024, thr=12.0,
                      seed=0) -> (poses [nq, 12] fp64, info [nq, 4] int32,
                      inlier [C] uint8)
        posfeat_ransac_pose (pose.hip): a RANSAC absolute pose (P3P, Gauss-Newton
        refit) for every query of a list from its 2D-3D correspondences, device
        tensors in and out, nothing read back.
  pose_correspondences(q_rows, db_rows, point_of_row, tinfo, q_set_off)
        the unique (query pool row, point) rows [C, 2] int32 of verified
        query-database matches and the queries' table q_off (device, torch ops
        only; one small read-back for the host table).
  solve_p3p(m)
        the P3P candidates [c, 3, 4] (c = 0..4) of three correspondences m [3, 5]
        = (xu, yu, X, Y, Z) (host only, needs no device).
"""
import ctypes

import numpy as np
import torch

from . import _lib, matchers
from ._lib import check, lib, ptr, stream_ptr


def sample_indices(seed, pair, it, n, k=4):
    k = int(k)
    out = np.zeros(max(k, 4), dtype=np.int32)
    if k == 4:
        r = lib().posfeat_ransac_sample(int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair), int(it), int(n),
                                        ctypes.c_void_p(out.ctypes.data))
    else:
        r = lib().posfeat_ransac_sample_k(int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair), int(it),
                                          int(n), k, ctypes.c_void_p(out.ctypes.data))
    if r != 0:
        raise ValueError("sample_indices needs 4 <= k <= 8, n >= k and non-negative pair and "
                         "iteration (got n = %d, pair = %d, it = %d, k = %d)" % (n, pair, it, k))
    return out[:k]


def solve7(m):
    """posfeat_fundamental_solve7: m [7, 4] rows (x, y, u, v) in normalised
    coordinates -> the candidates [c, 3, 3], unit norm, largest entry positive;
    c = 0 for a rejected sample."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (7, 4):
        raise ValueError("solve7 takes seven (x, y, u, v) rows")
    out = np.zeros((3, 3, 3), dtype=np.float64)
    c = lib().posfeat_fundamental_solve7(ctypes.c_void_p(m.ctypes.data),
                                         ctypes.c_void_p(out.ctypes.data))
    if c < 0:
        raise ValueError("posfeat_fundamental_solve7 failed (%d)" % c)
    return out[:c]


def solve5(m):
    """posfeat_essential_solve5: m [5, 4] rows (x, y, u, v) in normalised camera
    coordinates -> the candidates [c, 3, 3], unit norm, largest entry positive;
    c = 0 for a rejected sample."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (5, 4):
        raise ValueError("solve5 takes five (x, y, u, v) rows")
    out = np.zeros((10, 3, 3), dtype=np.float64)
    c = lib().posfeat_essential_solve5(ctypes.c_void_p(m.ctypes.data),
                                       ctypes.c_void_p(out.ctypes.data))
    if c < 0:
        raise ValueError("posfeat_essential_solve5 failed (%d)" % c)
    return out[:c]


def decompose_essential(E, m):
    """posfeat_essential_decompose: E [3, 3] and the matches m [n, 4] in
    normalised camera coordinates -> (pose [3, 4] = [R | t], the index of the
    chosen decomposition, the matches in front of both cameras)."""
    E = np.ascontiguousarray(E, dtype=np.float64)
    m = np.ascontiguousarray(m, dtype=np.float64)
    if E.shape != (3, 3) or m.ndim != 2 or m.shape[1] != 4:
        raise ValueError("decompose_essential takes E [3, 3] and (x, y, u, v) rows")
    pose = np.zeros((3, 4), dtype=np.float64)
    front = np.zeros(2, dtype=np.int32)
    r = lib().posfeat_essential_decompose(ctypes.c_void_p(E.ctypes.data),
                                          ctypes.c_void_p(m.ctypes.data) if m.shape[0] else None,
                                          int(m.shape[0]), ctypes.c_void_p(pose.ctypes.data),
                                          ctypes.c_void_p(front.ctypes.data))
    if r != 0:
        raise ValueError("E has no finite decomposition")
    return pose, int(front[0]), int(front[1])


def _ransac_pairs(model, kp_pool, batch, iters, thr, seed):
    """the one call shape both models share"""
    _lib.require_device(kp_pool)
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    kp_pool = kp_pool.contiguous()
    set_off, pairs = batch.set_off, batch.pairs
    npairs, nsets = pairs.shape[0], set_off.shape[0] - 1
    if kp_pool.shape[0] < int(set_off[-1]):
        raise ValueError("kp_pool has fewer rows than the sets of the batch")
    so, pp = ctypes.c_void_p(set_off.ctypes.data), ctypes.c_void_p(pairs.ctypes.data)
    need = getattr(lib(), "posfeat_ransac_%s_workspace" % model)(so, nsets, pp, npairs, int(iters))
    if need == 0:
        raise ValueError("invalid pair tables, or iters outside 1..65536")
    dev = kp_pool.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    M = torch.empty(npairs, 3, 3, dtype=torch.float64, device=dev)
    info = torch.empty(npairs, 4, dtype=torch.int32, device=dev)
    inlier = torch.empty(int(batch.moff[-1]), dtype=torch.uint8, device=dev)
    check(getattr(lib(), "posfeat_ransac_%s" % model)(
        ptr(kp_pool), so, nsets, pp, npairs, ptr(batch.matches), ptr(batch.counts), int(iters),
        float(thr), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(M), ptr(info), ptr(inlier), ptr(ws), need,
        stream_ptr(dev)))
    return M, info, inlier


def ransac_homography_pairs(kp_pool, batch, iters=1024, thr=3.0, seed=0):
    """posfeat_ransac_homography on what ``batch`` (matchers.PairBatch) holds;
    kp_pool: [N, 2] fp32 device tensor with the row numbering of the descriptor
    pool the batch was matched from."""
    return _ransac_pairs("homography", kp_pool, batch, iters, thr, seed)


def ransac_fundamental_pairs(kp_pool, batch, iters=2048, thr=4.0, seed=0):
    """posfeat_ransac_fundamental on what ``batch`` (matchers.PairBatch) holds;
    the arguments of ransac_homography_pairs.  thr = 4 px is COLMAP's two-view
    max_error default."""
    return _ransac_pairs("fundamental", kp_pool, batch, iters, thr, seed)


def guided_pairs(kp_pool, batch, model, M, thr, matcher="mnn", ratio=0.95):
    """posfeat_match_pairs_guided on the tables of an existing PairBatch: the
    pairs of ``batch`` matched again with the candidates restricted to those
    the verified model M[p] ("homography" or "fundamental", [npairs, 3, 3] fp64
    on the device, as ransac_*_pairs return it) admits within ``thr`` pixels.
    Returns a new PairBatch with the layout of ``batch``."""
    return matchers.match_pairs_guided_device(batch.pool, kp_pool, batch.set_off, batch.pairs,
                                              model, M, thr, matcher, ratio)


def guided_record(model, side, M, pt):
    """posfeat_guided_record (host only, needs no device): the fp32 x 4 record
    of the point ``pt`` (x, y) under M [3, 3]; side 0 an image-1 point, side 1
    an image-2 point; model 0 homography, 1 fundamental matrix."""
    M = np.ascontiguousarray(M, dtype=np.float64).reshape(9)
    pt = np.ascontiguousarray(pt, dtype=np.float32).reshape(2)
    out = np.zeros(4, dtype=np.float32)
    r = lib().posfeat_guided_record(int(model), int(side), ctypes.c_void_p(M.ctypes.data),
                                    ctypes.c_void_p(pt.ctypes.data),
                                    ctypes.c_void_p(out.ctypes.data))
    if r != 0:
        raise ValueError("posfeat_guided_record failed (%d)" % r)
    return out


def guided_admissible(model, ra, col, thr):
    """posfeat_guided_admissible (host only, needs no device): the fp32
    predicate of the guided fold for a streamed record ra [4] and the column's
    data col [3] (fundamental: its keypoint and the w of its record;
    homography: its record's x, y)."""
    ra = np.ascontiguousarray(ra, dtype=np.float32).reshape(4)
    col = np.ascontiguousarray(col, dtype=np.float32).reshape(3)
    r = lib().posfeat_guided_admissible(int(model), ctypes.c_void_p(ra.ctypes.data),
                                        ctypes.c_void_p(col.ctypes.data), float(thr))
    if r < 0:
        raise ValueError("posfeat_guided_admissible failed (%d)" % r)
    return bool(r)


def ransac_essential_pairs(kp_pool, cams, batch, iters=1024, thr=4.0, seed=0):
    """posfeat_ransac_essential on what ``batch`` (matchers.PairBatch) holds;
    kp_pool as for ransac_homography_pairs, cams [nsets, 8] fp64 device tensor,
    one camera row per set.  thr is in pixels (COLMAP's two-view default)."""
    _lib.require_device(kp_pool)
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    kp_pool = kp_pool.contiguous()
    set_off, pairs = batch.set_off, batch.pairs
    npairs, nsets = pairs.shape[0], set_off.shape[0] - 1
    if kp_pool.shape[0] < int(set_off[-1]):
        raise ValueError("kp_pool has fewer rows than the sets of the batch")
    if (not torch.is_tensor(cams) or cams.dtype != torch.float64 or cams.dim() != 2 or
            tuple(cams.shape) != (nsets, 8) or cams.device != kp_pool.device):
        raise ValueError("cams must be a [nsets, 8] float64 tensor on kp_pool's device")
    cams = cams.contiguous()
    so, pp = ctypes.c_void_p(set_off.ctypes.data), ctypes.c_void_p(pairs.ctypes.data)
    need = lib().posfeat_ransac_essential_workspace(so, nsets, pp, npairs, int(iters))
    if need == 0:
        raise ValueError("invalid pair tables, or iters outside 1..65536")
    dev = kp_pool.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    E = torch.empty(npairs, 3, 3, dtype=torch.float64, device=dev)
    pose = torch.empty(npairs, 3, 4, dtype=torch.float64, device=dev)
    info = torch.empty(npairs, 4, dtype=torch.int32, device=dev)
    cheir = torch.empty(npairs, 2, dtype=torch.int32, device=dev)
    inlier = torch.empty(int(batch.moff[-1]), dtype=torch.uint8, device=dev)
    check(lib().posfeat_ransac_essential(
        ptr(kp_pool), ptr(cams), so, nsets, pp, npairs, ptr(batch.matches), ptr(batch.counts),
        int(iters), float(thr), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(E), ptr(pose), ptr(info),
        ptr(cheir), ptr(inlier), ptr(ws), need, stream_ptr(dev)))
    return E, pose, info, cheir, inlier


def _one_pair(kp1, kp2, matches, dev):
    """the two-set pool and the one-pair batch of find_*: (kp_pool, batch, m),
    or None when the first set is empty"""
    kp1 = np.ascontiguousarray(np.asarray(kp1)[:, :2], dtype=np.float32)
    kp2 = np.ascontiguousarray(np.asarray(kp2)[:, :2], dtype=np.float32)
    matches = np.asarray(matches, dtype=np.int32).reshape(-1, 2)
    n1, m = kp1.shape[0], matches.shape[0]
    if m > n1:
        raise ValueError("more matches (%d) than keypoints in the first set (%d)" % (m, n1))
    if n1 == 0:
        return None
    set_off = np.asarray([0, n1, n1 + kp2.shape[0]], dtype=np.int32)
    pairs = np.asarray([[0, 1]], dtype=np.int32)
    rows = np.full((n1, 2), -1, np.int32)
    rows[:m] = matches
    buf = torch.from_numpy(np.concatenate([[m], rows.reshape(-1)]).astype(np.int32)).to(dev)
    batch = matchers.PairBatch(None, set_off, pairs, np.asarray([0, n1]), buf)
    return torch.from_numpy(np.concatenate([kp1, kp2], 0)).to(dev), batch, m


def find_essential(kp1, kp2, cam1, cam2, matches, iters=1024, thr=4.0, seed=0):
    """find_fundamental's counterpart between two calibrated cameras: cam1, cam2
    are camera rows (fx, fy, cx, cy, k1, 0, 0, 0).  Returns (E [3, 3] fp64 with
    Frobenius norm 1, pose [3, 4] = [R | t], mask [m] bool, info [4] int32); E
    and pose are all zeros and info[0] = 1 when no model was found."""
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    cams = np.zeros((2, 8), np.float64)
    for row, cam in zip(cams, (cam1, cam2)):
        cam = np.asarray(cam, np.float64).reshape(-1)
        if cam.shape[0] < 4 or cam.shape[0] > 8:
            raise ValueError("a camera row is (fx, fy, cx, cy[, k1, 0, 0, 0])")
        row[:cam.shape[0]] = cam
    one = _one_pair(kp1, kp2, matches, dev)
    if one is None:
        return (np.zeros((3, 3)), np.zeros((3, 4)), np.zeros(0, bool),
                np.asarray([1, 0, -1, 0], np.int32))
    kp_pool, batch, m = one
    E, pose, info, _, inlier = ransac_essential_pairs(kp_pool, torch.from_numpy(cams).to(dev),
                                                      batch, iters, thr, seed)
    return (E[0].cpu().numpy(), pose[0].cpu().numpy(), inlier[:m].cpu().numpy().astype(bool),
            info[0].cpu().numpy())


def _find(model, kp1, kp2, matches, iters, thr, seed):
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    kp1 = np.ascontiguousarray(np.asarray(kp1)[:, :2], dtype=np.float32)
    kp2 = np.ascontiguousarray(np.asarray(kp2)[:, :2], dtype=np.float32)
    matches = np.asarray(matches, dtype=np.int32).reshape(-1, 2)
    n1, m = kp1.shape[0], matches.shape[0]
    if m > n1:
        raise ValueError("more matches (%d) than keypoints in the first set (%d)" % (m, n1))
    if n1 == 0:
        return np.zeros((3, 3)), np.zeros(0, bool), np.asarray([1, 0, -1, 0], np.int32)
    set_off = np.asarray([0, n1, n1 + kp2.shape[0]], dtype=np.int32)
    pairs = np.asarray([[0, 1]], dtype=np.int32)
    rows = np.full((n1, 2), -1, np.int32)
    rows[:m] = matches
    buf = torch.from_numpy(np.concatenate([[m], rows.reshape(-1)]).astype(np.int32)).to(dev)
    batch = matchers.PairBatch(None, set_off, pairs, np.asarray([0, n1]), buf)
    kp_pool = torch.from_numpy(np.concatenate([kp1, kp2], 0)).to(dev)
    M, info, inlier = _ransac_pairs(model, kp_pool, batch, iters, thr, seed)
    return M[0].cpu().numpy(), inlier[:m].cpu().numpy().astype(bool), info[0].cpu().numpy()


def find_homography(kp1, kp2, matches, iters=1024, thr=3.0, seed=0):
    """One pair through the same call: kp1 [n1, >=2], kp2 [n2, >=2] keypoints
    (x, y), matches [m, 2] (index in 1, index in 2), m <= n1.  Returns (H [3, 3]
    fp64 with Frobenius norm 1, mask [m] bool, info [4] int32); H is all zeros
    and info[0] = 1 when no model was found."""
    return _find("homography", kp1, kp2, matches, iters, thr, seed)


def find_fundamental(kp1, kp2, matches, iters=2048, thr=4.0, seed=0):
    """find_homography's counterpart for a fundamental matrix: (F [3, 3] fp64
    with Frobenius norm 1, mask [m] bool, info [4] int32)."""
    return _find("fundamental", kp1, kp2, matches, iters, thr, seed)


def triangulate_dlt(obs):
    """posfeat_triangulate_dlt: obs [n, 14] rows (xu, yu, the 12 entries of [R |
    t] row-major) -> X [3], or None when the system is rejected."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    if obs.ndim != 2 or obs.shape[1] != 14 or obs.shape[0] < 1:
        raise ValueError("triangulate_dlt takes [n >= 1, 14] rows (xu, yu, pose)")
    X = np.zeros(3, dtype=np.float64)
    r = lib().posfeat_triangulate_dlt(ctypes.c_void_p(obs.ctypes.data), obs.shape[0],
                                      ctypes.c_void_p(X.ctypes.data))
    if r < 0:
        raise ValueError("posfeat_triangulate_dlt failed (%d)" % r)
    return X if r == 0 else None


def _read_back(parts):
    """{name: device tensor} -> {name: its bytes on the host (a uint8 numpy view)}:
    one pinned buffer, one synchronisation"""
    flat = [p.reshape(-1).view(torch.uint8) for p in parts.values()]
    sizes = [int(f.numel()) for f in flat]
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    at = 0
    for f, n in zip(flat, sizes):
        host[at:at + n].copy_(f, non_blocking=True)
        at += n
    torch.cuda.current_stream(flat[0].device).synchronize()
    h, cuts = host.numpy(), np.cumsum([0] + sizes)
    return {k: h[cuts[i]:cuts[i + 1]] for i, k in enumerate(parts)}


class TrackResult:
    """What one posfeat_triangulate call left on the device, cut to the worst
    case (Tmax = min(nedges, N // 2) tracks, Mmax = min(2 nedges, N) members):
    ``points`` [Tmax, 3] fp64, ``err`` [Tmax] fp64, ``tinfo`` [Tmax, 4] int32,
    ``track_off`` [Tmax + 1] int32, ``track_rows`` [Mmax] int32, ``obs_inlier``
    [Mmax] uint8, ``point_of_row`` [N] int32, ``counts`` [8] int32.  Rows past
    counts[0] tracks / counts[1] members are not written."""

    FIELDS = ("points", "err", "tinfo", "track_off", "track_rows", "obs_inlier", "point_of_row",
              "counts")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])

    def host(self):
        """Everything on the host as numpy arrays trimmed by ``counts``: one
        pinned copy, one synchronisation."""
        raw = _read_back({k: getattr(self, k) for k in self.FIELDS})
        counts = raw["counts"].view(np.int32).copy()
        T, M = int(counts[0]), int(counts[1])
        return dict(
            points=raw["points"].view(np.float64).reshape(-1, 3)[:T].copy(),
            err=raw["err"].view(np.float64)[:T].copy(),
            tinfo=raw["tinfo"].view(np.int32).reshape(-1, 4)[:T].copy(),
            track_off=raw["track_off"].view(np.int32)[:T + 1].copy(),
            track_rows=raw["track_rows"].view(np.int32)[:M].copy(),
            obs_inlier=raw["obs_inlier"][:M].copy(),
            point_of_row=raw["point_of_row"].view(np.int32)[:self.point_of_row.shape[0]].copy(),
            counts=counts)


def triangulate_tracks(kp_pool, set_off, cams, poses, edges, iters=64, thr=4.0, min_angle=1.5,
                       max_track=256, seed=0):
    """posfeat_triangulate: kp_pool [N, 2] fp32, cams [nsets, 8] fp64, poses
    [nsets, 12] fp64 (or [nsets, 3, 4]), edges [E, 2] int32 device tensors;
    set_off [nsets + 1] a host int32 table.  thr = 4 px and min_angle = 1.5
    degrees are COLMAP's filter_max_reproj_error and filter_min_tri_angle."""
    _lib.require_device(kp_pool)
    dev = kp_pool.device
    set_off = np.ascontiguousarray(set_off, dtype=np.int32)
    nsets = set_off.shape[0] - 1
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    if nsets < 0 or kp_pool.shape[0] != int(set_off[-1]):
        raise ValueError("kp_pool must have set_off[-1] rows")
    poses = poses.reshape(-1, 12)
    for name, t, shape, dt in (("cams", cams, (nsets, 8), torch.float64),
                               ("poses", poses, (nsets, 12), torch.float64)):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s %s tensor on the keypoints' device" % (name, shape, dt))
    if edges.device != dev or edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 2:
        raise ValueError("edges must be a [E, 2] int32 tensor on the keypoints' device")
    kp_pool, cams, poses, edges = (t.contiguous() for t in (kp_pool, cams, poses, edges))
    N, E = int(set_off[-1]), int(edges.shape[0])
    so = ctypes.c_void_p(set_off.ctypes.data)
    need = lib().posfeat_triangulate_workspace(so, nsets, E, int(max_track))
    if need == 0:
        raise ValueError("invalid set table, or max_track outside 2..1024")
    tmax, mmax = min(E, N // 2), min(2 * E, N)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = TrackResult(
        points=torch.empty(max(tmax, 1), 3, dtype=torch.float64, device=dev),
        err=torch.empty(max(tmax, 1), dtype=torch.float64, device=dev),
        tinfo=torch.empty(max(tmax, 1), 4, dtype=torch.int32, device=dev),
        track_off=torch.empty(tmax + 1, dtype=torch.int32, device=dev),
        track_rows=torch.empty(max(mmax, 1), dtype=torch.int32, device=dev),
        obs_inlier=torch.empty(max(mmax, 1), dtype=torch.uint8, device=dev),
        point_of_row=torch.empty(max(N, 1), dtype=torch.int32, device=dev),
        counts=torch.empty(8, dtype=torch.int32, device=dev))
    check(lib().posfeat_triangulate(
        ptr(kp_pool), so, nsets, ptr(cams), ptr(poses), ptr(edges), E, int(iters), float(thr),
        float(min_angle), int(max_track), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(out.points),
        ptr(out.err), ptr(out.tinfo), ptr(out.track_off), ptr(out.track_rows), ptr(out.obs_inlier),
        ptr(out.point_of_row), ptr(out.counts), ptr(ws), need, stream_ptr(dev)))
    out.point_of_row = out.point_of_row[:N]
    return out


class RefinedTrackResult(TrackResult):
    """What one posfeat_refine_points call left on the device: a TrackResult
    (``track_off`` and ``track_rows`` are the input's own tensors) plus
    ``rinfo`` [Tmax, 4] int32 = (rounds used, taken steps, converged, flags
    changed).  ``counts`` is posfeat_refine_points' (T, status-0 points, inlier
    observations, status-2, status-3, carried status-1, tracks whose flags
    changed, 0); the member count is track_off[T]."""

    FIELDS = TrackResult.FIELDS + ("rinfo",)
    source = None        # the TrackResult that was refined (refine_tracks sets it)

    def host(self):
        """TrackResult.host() plus ``rinfo`` and, where the refined TrackResult
        is attached, ``unrefined`` = dict(err, tinfo, counts) of it: one pinned
        copy, one synchronisation."""
        parts = {k: getattr(self, k) for k in self.FIELDS}
        if self.source is not None:
            parts.update(err0=self.source.err, tinfo0=self.source.tinfo, counts0=self.source.counts)
        raw = _read_back(parts)
        counts = raw["counts"].view(np.int32).copy()
        T = int(counts[0])
        track_off = raw["track_off"].view(np.int32)[:T + 1].copy()
        M = int(track_off[T]) if T > 0 else 0
        out = dict(
            points=raw["points"].view(np.float64).reshape(-1, 3)[:T].copy(),
            err=raw["err"].view(np.float64)[:T].copy(),
            tinfo=raw["tinfo"].view(np.int32).reshape(-1, 4)[:T].copy(),
            track_off=track_off,
            track_rows=raw["track_rows"].view(np.int32)[:M].copy(),
            obs_inlier=raw["obs_inlier"][:M].copy(),
            point_of_row=raw["point_of_row"].view(np.int32)[:self.point_of_row.shape[0]].copy(),
            counts=counts,
            rinfo=raw["rinfo"].view(np.int32).reshape(-1, 4)[:T].copy())
        if self.source is not None:
            out["unrefined"] = dict(err=raw["err0"].view(np.float64)[:T].copy(),
                                    tinfo=raw["tinfo0"].view(np.int32).reshape(-1, 4)[:T].copy(),
                                    counts=raw["counts0"].view(np.int32).copy())
        return out


def refine_tracks(kp_pool, set_off, cams, poses, tracks, thr=4.0, min_angle=1.5, rounds=3, steps=10):
    """posfeat_refine_points on what ``tracks`` (a TrackResult of
    triangulate_tracks on the same kp_pool, set_off, cams and poses) holds on the
    device.  thr and min_angle as in triangulate_tracks; ``rounds`` in 1..8
    alternations of refinement and inlier test, ``steps`` in 1..32 trial points
    per round."""
    _lib.require_device(kp_pool)
    dev = kp_pool.device
    set_off = np.ascontiguousarray(set_off, dtype=np.int32)
    nsets = set_off.shape[0] - 1
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    if nsets < 0 or kp_pool.shape[0] != int(set_off[-1]):
        raise ValueError("kp_pool must have set_off[-1] rows")
    poses = poses.reshape(-1, 12)
    for name, t, shape, dt in (("cams", cams, (nsets, 8), torch.float64),
                               ("poses", poses, (nsets, 12), torch.float64)):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s %s tensor on the keypoints' device" % (name, shape, dt))
    N = int(set_off[-1])
    tmax, mmax = int(tracks.track_off.shape[0]) - 1, int(tracks.track_rows.shape[0])
    for name, dt, shape in (("points", torch.float64, (tracks.points.shape[0], 3)),
                            ("tinfo", torch.int32, (tracks.points.shape[0], 4)),
                            ("track_off", torch.int32, (tmax + 1,)),
                            ("track_rows", torch.int32, (mmax,)),
                            ("obs_inlier", torch.uint8, (mmax,)), ("counts", torch.int32, (8,))):
        t = getattr(tracks, name)
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("tracks.%s must be a contiguous %s %s tensor on the keypoints' device"
                             % (name, shape, dt))
    if tmax < 0 or tracks.points.shape[0] < max(tmax, 1) or tuple(tracks.point_of_row.shape) != (N,):
        raise ValueError("tracks does not belong to this keypoint pool")
    kp_pool, cams, poses = (t.contiguous() for t in (kp_pool, cams, poses))
    so = ctypes.c_void_p(set_off.ctypes.data)
    need = lib().posfeat_refine_points_workspace(so, nsets, tmax, mmax)
    if need == 0:
        raise ValueError("invalid set table")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = RefinedTrackResult(
        points=torch.empty(max(tmax, 1), 3, dtype=torch.float64, device=dev),
        err=torch.empty(max(tmax, 1), dtype=torch.float64, device=dev),
        tinfo=torch.empty(max(tmax, 1), 4, dtype=torch.int32, device=dev),
        track_off=tracks.track_off, track_rows=tracks.track_rows,
        obs_inlier=torch.empty(max(mmax, 1), dtype=torch.uint8, device=dev),
        point_of_row=torch.empty(max(N, 1), dtype=torch.int32, device=dev),
        counts=torch.empty(8, dtype=torch.int32, device=dev),
        rinfo=torch.empty(max(tmax, 1), 4, dtype=torch.int32, device=dev))
    check(lib().posfeat_refine_points(
        ptr(kp_pool), so, nsets, ptr(cams), ptr(poses), ptr(tracks.points), ptr(tracks.tinfo),
        ptr(tracks.track_off), ptr(tracks.track_rows), ptr(tracks.obs_inlier), ptr(tracks.counts),
        tmax, mmax, float(thr), float(min_angle), int(rounds), int(steps), ptr(out.points),
        ptr(out.err), ptr(out.tinfo), ptr(out.obs_inlier), ptr(out.point_of_row), ptr(out.rinfo),
        ptr(out.counts), ptr(ws), need, stream_ptr(dev)))
    out.point_of_row = out.point_of_row[:N]
    out.source = tracks
    return out


class SplitTrackResult(TrackResult):
    """What one posfeat_split_tracks call left on the device: a TrackResult of
    its own buffers (capacity Tmax' = Mmax // 2 tracks) in which a track of the
    input may have become several, plus ``parent_of`` [Tmax'] int32 (the input
    track id) and ``generation`` [Tmax'] int32 (0 for the parent itself, g for
    its g-th child).  ``counts`` = (T', members, status-0 points, inlier
    observations, children that did not fit, 0, children created, parents that
    split)."""

    FIELDS = TrackResult.FIELDS + ("parent_of", "generation")
    source = None        # the TrackResult that was split (split_tracks sets it)

    def host(self):
        """TrackResult.host() plus ``parent_of`` and ``generation`` and, where the
        split TrackResult is attached, ``counts_unsplit``: one pinned copy, one
        synchronisation."""
        parts = {k: getattr(self, k) for k in self.FIELDS}
        if self.source is not None:
            parts.update(counts0=self.source.counts)
        raw = _read_back(parts)
        counts = raw["counts"].view(np.int32).copy()
        T, M = int(counts[0]), int(counts[1])
        out = dict(
            points=raw["points"].view(np.float64).reshape(-1, 3)[:T].copy(),
            err=raw["err"].view(np.float64)[:T].copy(),
            tinfo=raw["tinfo"].view(np.int32).reshape(-1, 4)[:T].copy(),
            track_off=raw["track_off"].view(np.int32)[:T + 1].copy(),
            track_rows=raw["track_rows"].view(np.int32)[:M].copy(),
            obs_inlier=raw["obs_inlier"][:M].copy(),
            point_of_row=raw["point_of_row"].view(np.int32)[:self.point_of_row.shape[0]].copy(),
            counts=counts,
            parent_of=raw["parent_of"].view(np.int32)[:T].copy(),
            generation=raw["generation"].view(np.int32)[:T].copy())
        if self.source is not None:
            out["counts_unsplit"] = raw["counts0"].view(np.int32).copy()
        return out


def split_tracks(kp_pool, set_off, cams, poses, tracks, iters=64, thr=4.0, min_angle=1.5, rounds=2,
                 seed=0, tmax_out=None):
    """posfeat_split_tracks on what ``tracks`` (a TrackResult of
    triangulate_tracks on the same kp_pool, set_off, cams and poses) holds on the
    device: sequential RANSAC, ``rounds`` in 1..4 generations, over the members
    each track's own RANSAC left out.  iters, thr, min_angle and seed as in
    triangulate_tracks.  ``tmax_out`` (default Mmax // 2, which disjoint tracks
    of two members cannot exceed, and never below the input's capacity) is the
    track capacity of the result.  The result can be passed to refine_tracks
    and pose_correspondences as it is."""
    _lib.require_device(kp_pool)
    dev = kp_pool.device
    set_off = np.ascontiguousarray(set_off, dtype=np.int32)
    nsets = set_off.shape[0] - 1
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    if nsets < 0 or kp_pool.shape[0] != int(set_off[-1]):
        raise ValueError("kp_pool must have set_off[-1] rows")
    poses = poses.reshape(-1, 12)
    for name, t, shape, dt in (("cams", cams, (nsets, 8), torch.float64),
                               ("poses", poses, (nsets, 12), torch.float64)):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s %s tensor on the keypoints' device" % (name, shape, dt))
    N = int(set_off[-1])
    tmax, mmax = int(tracks.track_off.shape[0]) - 1, int(tracks.track_rows.shape[0])
    for name, dt, shape in (("points", torch.float64, (tracks.points.shape[0], 3)),
                            ("err", torch.float64, (tracks.points.shape[0],)),
                            ("tinfo", torch.int32, (tracks.points.shape[0], 4)),
                            ("track_off", torch.int32, (tmax + 1,)),
                            ("track_rows", torch.int32, (mmax,)),
                            ("obs_inlier", torch.uint8, (mmax,)), ("counts", torch.int32, (8,))):
        t = getattr(tracks, name)
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("tracks.%s must be a contiguous %s %s tensor on the keypoints' device"
                             % (name, shape, dt))
    if tmax < 0 or tracks.points.shape[0] < max(tmax, 1) or tuple(tracks.point_of_row.shape) != (N,):
        raise ValueError("tracks does not belong to this keypoint pool")
    tout = max(tmax, mmax // 2) if tmax_out is None else int(tmax_out)
    kp_pool, cams, poses = (t.contiguous() for t in (kp_pool, cams, poses))
    so = ctypes.c_void_p(set_off.ctypes.data)
    need = lib().posfeat_split_tracks_workspace(so, nsets, tmax, mmax, tout)
    if need == 0:
        raise ValueError("invalid set table, or tmax_out below the input's track capacity")
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = SplitTrackResult(
        points=torch.empty(max(tout, 1), 3, dtype=torch.float64, device=dev),
        err=torch.empty(max(tout, 1), dtype=torch.float64, device=dev),
        tinfo=torch.empty(max(tout, 1), 4, dtype=torch.int32, device=dev),
        track_off=torch.empty(tout + 1, dtype=torch.int32, device=dev),
        track_rows=torch.empty(max(mmax, 1), dtype=torch.int32, device=dev),
        obs_inlier=torch.empty(max(mmax, 1), dtype=torch.uint8, device=dev),
        point_of_row=torch.empty(max(N, 1), dtype=torch.int32, device=dev),
        counts=torch.empty(8, dtype=torch.int32, device=dev),
        parent_of=torch.empty(max(tout, 1), dtype=torch.int32, device=dev),
        generation=torch.empty(max(tout, 1), dtype=torch.int32, device=dev))
    check(lib().posfeat_split_tracks(
        ptr(kp_pool), so, nsets, ptr(cams), ptr(poses), ptr(tracks.points), ptr(tracks.err),
        ptr(tracks.tinfo), ptr(tracks.track_off), ptr(tracks.track_rows), ptr(tracks.obs_inlier),
        ptr(tracks.counts), tmax, mmax, int(iters), float(thr), float(min_angle),
        int(seed) & 0xFFFFFFFFFFFFFFFF, int(rounds), tout, ptr(out.points), ptr(out.err),
        ptr(out.tinfo), ptr(out.track_off), ptr(out.track_rows), ptr(out.obs_inlier),
        ptr(out.point_of_row), ptr(out.parent_of), ptr(out.generation), ptr(out.counts), ptr(ws),
        need, stream_ptr(dev)))
    out.point_of_row = out.point_of_row[:N]
    out.source = tracks
    return out


def refine_point(obs, X0, steps=10):
    """posfeat_refine_point: obs [n >= 2, 22] rows (x, y, the 8 camera entries,
    the 12 entries of [R | t] row-major), X0 [3] -> (X [3], the cost sum |r|^2 at
    X, the number of taken steps) after one Levenberg-Marquardt round over all
    rows; the cost is NaN (and X = X0) when a row has no positive depth or no
    finite residual at X0."""
    obs = np.ascontiguousarray(obs, dtype=np.float64)
    X0 = np.ascontiguousarray(X0, dtype=np.float64).reshape(-1)
    if obs.ndim != 2 or obs.shape[1] != 22 or obs.shape[0] < 2 or X0.shape[0] != 3:
        raise ValueError("refine_point takes [n >= 2, 22] rows (x, y, cam, pose) and a point [3]")
    X, cost = np.zeros(3, dtype=np.float64), np.zeros(1, dtype=np.float64)
    r = lib().posfeat_refine_point(ctypes.c_void_p(obs.ctypes.data), obs.shape[0],
                                   ctypes.c_void_p(X0.ctypes.data), int(steps),
                                   ctypes.c_void_p(X.ctypes.data), ctypes.c_void_p(cost.ctypes.data))
    if r < 0:
        raise ValueError("posfeat_refine_point failed (%d): steps outside 1..32?" % r)
    return X, float(cost[0]), int(r)


def track_edges(batch, inlier):
    """The match graph of a PairBatch: row moff[p] + i of the result holds the
    global pool rows (set_off[s1] + a, set_off[s2] + b) of match i of pair p
    where i < counts[p] and ``inlier`` (the RANSAC mask, [sum n1] uint8 or
    bool) is set, else (-1, -1), which posfeat_triangulate ignores.  Torch ops
    on the device only; the per-row pair tables come from the host tables."""
    set_off = np.asarray(batch.set_off, dtype=np.int64)
    pairs = np.asarray(batch.pairs, dtype=np.int64).reshape(-1, 2)
    moff = np.asarray(batch.moff, dtype=np.int64)
    dev = batch.matches.device
    n1 = np.diff(moff)
    pair_of = np.repeat(np.arange(pairs.shape[0]), n1)
    local = np.arange(int(moff[-1])) - moff[:-1][pair_of]
    tab = np.stack([pair_of, local, set_off[pairs[pair_of, 0]], set_off[pairs[pair_of, 1]],
                    set_off[pairs[pair_of, 1] + 1] - set_off[pairs[pair_of, 1]], n1[pair_of]], 1)
    tab = torch.from_numpy(np.ascontiguousarray(tab)).to(dev)
    if tab.shape[0] == 0:
        return torch.empty(0, 2, dtype=torch.int32, device=dev)
    m = batch.matches.to(torch.int64)
    a, b = m[:, 0], m[:, 1]
    ok = ((tab[:, 1] < batch.counts.to(torch.int64)[tab[:, 0]]) & (inlier.reshape(-1) != 0) &
          (a >= 0) & (a < tab[:, 5]) & (b >= 0) & (b < tab[:, 4]))
    e = torch.stack([tab[:, 2] + a, tab[:, 3] + b], 1)
    return torch.where(ok[:, None], e, torch.full_like(e, -1)).to(torch.int32)


def solve_p3p(m):
    """posfeat_pose_solve3: m [3, 5] rows (xu, yu, X, Y, Z), the undistorted
    normalised image point and the world point -> the candidate poses [c, 3, 4]
    ([R | t], world to camera) in ascending root order; c = 0 for a rejected
    sample."""
    m = np.ascontiguousarray(m, dtype=np.float64)
    if m.shape != (3, 5):
        raise ValueError("solve_p3p takes three (xu, yu, X, Y, Z) rows")
    out = np.zeros((4, 3, 4), dtype=np.float64)
    c = lib().posfeat_pose_solve3(ctypes.c_void_p(m.ctypes.data), ctypes.c_void_p(out.ctypes.data))
    if c < 0:
        raise ValueError("posfeat_pose_solve3 failed (%d)" % c)
    return out[:c]


def ransac_pose_queries(kp_pool, cams, points, corr, q_off, iters=1024, thr=12.0, seed=0):
    """posfeat_ransac_pose: kp_pool [nkp, 2] fp32 (the queries' keypoints), cams
    [nq, 8] fp64, points [npoints, 3] fp64 (posfeat_triangulate's, as left on
    the device), corr [C, 2] int32 = (pool row, point index) device tensors;
    q_off [nq + 1] a host int32 table, query q owning corr[q_off[q]:q_off[q +
    1]].  thr = 12 px is meant as COLMAP's abs_pose_max_error default (written
    from memory, not checked against its sources).  info[q] = (status,
    n_inliers, best_iter, refit_kept | root << 8)."""
    _lib.require_device(kp_pool)
    dev = kp_pool.device
    q_off = np.ascontiguousarray(q_off, dtype=np.int32)
    nq = q_off.shape[0] - 1
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    if nq < 0:
        raise ValueError("q_off needs at least one entry")
    C = int(q_off[-1])
    for name, t, shape, dt in (("cams", cams, (nq, 8), torch.float64),
                               ("points", points, (points.shape[0], 3), torch.float64),
                               ("corr", corr, (C, 2), torch.int32)):
        if t.device != dev or t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError("%s must be a %s %s tensor on the keypoints' device" % (name, shape, dt))
    qo = ctypes.c_void_p(q_off.ctypes.data)
    need = lib().posfeat_ransac_pose_workspace(qo, nq, int(iters))
    if need == 0:
        raise ValueError("invalid query table, or iters outside 1..65536")
    nkp, npoints = int(kp_pool.shape[0]), int(points.shape[0])

    def some(t, *shape):  # the call takes no null pointer, even for an input without elements
        return t.contiguous() if t.numel() else torch.zeros(*shape, dtype=t.dtype, device=dev)
    kp_pool, cams, points, corr = (some(kp_pool, 1, 2), some(cams, 1, 8), some(points, 1, 3),
                                   some(corr, 1, 2))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    poses = torch.empty(max(nq, 1), 12, dtype=torch.float64, device=dev)
    info = torch.empty(max(nq, 1), 4, dtype=torch.int32, device=dev)
    inlier = torch.empty(max(C, 1), dtype=torch.uint8, device=dev)
    check(lib().posfeat_ransac_pose(
        ptr(kp_pool), nkp, ptr(cams), ptr(points), npoints, ptr(corr), qo, nq, int(iters),
        float(thr), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(poses), ptr(info), ptr(inlier), ptr(ws),
        need, stream_ptr(dev)))
    return poses[:nq], info[:nq], inlier[:C]


def pose_correspondences(q_rows, db_rows, point_of_row, tinfo, q_set_off):
    """The 2D-3D correspondences of the queries: match i pairs row q_rows[i] of
    the query keypoint pool with row db_rows[i] of the database pool
    posfeat_triangulate ran on ([M] integer device tensors; rows outside their
    pool are ignored).  A match counts where its database row carries a point
    (point_of_row >= 0) of status 0 with at least two inlier observations
    (tinfo).  Returns (corr [C, 2] int32 on the device: the unique (query row,
    point) rows in ascending order, so grouped by query; q_off [nq + 1] int32 on
    the host for the queries' table q_set_off).  Torch ops on the device only;
    q_off is the one read-back."""
    dev = point_of_row.device
    q_set_off = np.ascontiguousarray(q_set_off, dtype=np.int64)
    nq = q_set_off.shape[0] - 1
    N, T = int(point_of_row.shape[0]), int(tinfo.shape[0])
    q = q_rows.to(device=dev, dtype=torch.int64).reshape(-1)
    d = db_rows.to(device=dev, dtype=torch.int64).reshape(-1)
    if q.numel() == 0 or N == 0 or T == 0 or nq <= 0:
        return (torch.empty(0, 2, dtype=torch.int32, device=dev),
                np.zeros(max(nq, 0) + 1, dtype=np.int32))
    ok = (q >= int(q_set_off[0])) & (q < int(q_set_off[-1])) & (d >= 0) & (d < N)
    pt = point_of_row.to(torch.int64)[d.clamp(0, N - 1)]
    ok &= (pt >= 0) & (pt < T)
    ti = tinfo.to(torch.int64)[pt.clamp(0, T - 1)]
    ok &= (ti[:, 0] == 0) & (ti[:, 1] >= 2)
    key = torch.unique(q[ok] * T + pt[ok])           # sorted
    rows = torch.div(key, T, rounding_mode="floor")
    corr = torch.stack([rows, key - rows * T], 1).to(torch.int32)
    q_off = torch.searchsorted(rows, torch.from_numpy(q_set_off).to(dev))
    return corr, q_off.cpu().numpy().astype(np.int32)
