"""Robust two-view model fitting on the GPU (ransac.hip, fundamental.hip): RANSAC
homographies or fundamental matrices for every pair of a pair list in three
launches, on the matches matchers.match_pairs_device left on the device.  The
definitions (sampler, degeneracy test, minimal solve, score, selection, refit)
are in include/posfeat_hip.h; no CPU path.

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
  sample_indices(seed, pair, it, n, k=4)
        the first k match indices (4 for a homography, 7 for a fundamental
        matrix) iteration ``it`` of pair ``pair`` draws from ``n`` matches (host
        only, needs no device).
  solve7(m)
        the 7-point candidates [c, 3, 3] (c = 0..3) of seven matches m [7, 4] in
        normalised coordinates (host only, needs no device).
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
