"""Robust two-view model fitting on the GPU (ransac.hip): RANSAC homographies
for every pair of a pair list in three launches, on the matches
matchers.match_pairs_device left on the device.  The definitions (sampler,
degeneracy test, minimal solve, score, selection, refit) are in
include/posfeat_hip.h; no CPU path.

  ransac_homography_pairs(kp_pool, batch, iters=1024, thr=3.0, seed=0)
        -> (H [npairs, 3, 3] fp64, info [npairs, 4] int32, inlier [sum n1] uint8)
        device tensors, stream-ordered, nothing read back.  info[p] =
        (status, n_inliers, best_iter, refit_kept); pair p's rows of ``inlier``
        start at ``batch.moff[p]``.
  find_homography(kp1, kp2, matches, iters=1024, thr=3.0, seed=0)
        one pair, numpy in and out: (H [3, 3], mask [m] bool, info [4]).
  sample_indices(seed, pair, it, n)
        the four match indices iteration ``it`` of pair ``pair`` draws from
        ``n`` matches (host only, needs no device).
"""
import ctypes

import numpy as np
import torch

from . import _lib, matchers
from ._lib import check, lib, ptr, stream_ptr


def sample_indices(seed, pair, it, n):
    out = np.zeros(4, dtype=np.int32)
    r = lib().posfeat_ransac_sample(int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair), int(it), int(n),
                                    ctypes.c_void_p(out.ctypes.data))
    if r != 0:
        raise ValueError("sample_indices needs n >= 4 and non-negative pair and iteration "
                         "(got n = %d, pair = %d, it = %d)" % (n, pair, it))
    return out


def ransac_homography_pairs(kp_pool, batch, iters=1024, thr=3.0, seed=0):
    """posfeat_ransac_homography on what ``batch`` (matchers.PairBatch) holds;
    kp_pool: [N, 2] fp32 device tensor with the row numbering of the descriptor
    pool the batch was matched from."""
    _lib.require_device(kp_pool)
    if kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or kp_pool.shape[1] != 2:
        raise ValueError("kp_pool must be a [N, 2] float32 tensor")
    kp_pool = kp_pool.contiguous()
    set_off, pairs = batch.set_off, batch.pairs
    npairs, nsets = pairs.shape[0], set_off.shape[0] - 1
    if kp_pool.shape[0] < int(set_off[-1]):
        raise ValueError("kp_pool has fewer rows than the sets of the batch")
    so, pp = ctypes.c_void_p(set_off.ctypes.data), ctypes.c_void_p(pairs.ctypes.data)
    need = lib().posfeat_ransac_homography_workspace(so, nsets, pp, npairs, int(iters))
    if need == 0:
        raise ValueError("invalid pair tables, or iters outside 1..65536")
    dev = kp_pool.device
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    H = torch.empty(npairs, 3, 3, dtype=torch.float64, device=dev)
    info = torch.empty(npairs, 4, dtype=torch.int32, device=dev)
    inlier = torch.empty(int(batch.moff[-1]), dtype=torch.uint8, device=dev)
    check(lib().posfeat_ransac_homography(
        ptr(kp_pool), so, nsets, pp, npairs, ptr(batch.matches), ptr(batch.counts), int(iters),
        float(thr), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(H), ptr(info), ptr(inlier), ptr(ws), need,
        stream_ptr(dev)))
    return H, info, inlier


def find_homography(kp1, kp2, matches, iters=1024, thr=3.0, seed=0):
    """One pair through the same call: kp1 [n1, >=2], kp2 [n2, >=2] keypoints
    (x, y), matches [m, 2] (index in 1, index in 2), m <= n1.  Returns (H [3, 3]
    fp64 with Frobenius norm 1, mask [m] bool, info [4] int32); H is all zeros
    and info[0] = 1 when no model was found."""
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
    H, info, inlier = ransac_homography_pairs(kp_pool, batch, iters, thr, seed)
    return H[0].cpu().numpy(), inlier[:m].cpu().numpy().astype(bool), info[0].cpu().numpy()
