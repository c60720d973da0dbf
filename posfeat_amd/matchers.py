"""Evaluation matchers on the GPU -- drop-ins with the
reference's names, arguments and return values:

  mnn_matcher(descriptors_a, descriptors_b)        losses/preprocess_utils.py:795-803,
                                                   evaluations/hpatches/evaluation.py:28-38
  mutual_nn_matcher(descriptors1, descriptors2)    evaluations/aachen/matchers.py:5-14,
                                                   ETH_local_feature/custom_matcher.py:5-14
  ratio_matcher(descriptors1, descriptors2, ratio=0.95)            aachen/matchers.py:17-44
  mutual_nn_ratio_matcher(descriptors1, descriptors2, ratio=0.95)  aachen/matchers.py:47-75

Each returns the int64 numpy array [n_matches, 2] of (index in 1, index in 2),
ascending in the first index.  One call = two launches of the fused
MFMA-similarity + top-2 kernel (match.hip; the n1 x n2 similarity matrix is
never written) and one selection kernel; the host reads the match count once
(the reference's ``.cpu().numpy()`` synchronises there too).  Tie rule: the
first (lowest) index wins an arg-max tie.  Descriptors must be L2-normalised
128-d float32 (what Extractor.save_desc writes); numpy inputs are uploaded to
the current device.  No CPU path.

  match_pairs(descs, pairs, matcher="mnn", ratio=0.95)   the same matchers over a
        pair list (matchpairs.hip): four launches and one host read for the
        whole list, results bit-identical to the per-pair functions
  match_pairs_guided_device(pool, kp_pool, set_off, pairs, model, M, thr,
                            matcher="mnn", ratio=0.95)
        the pair-list matchers with the candidates of each pair restricted to
        those its verified homography or fundamental matrix admits within thr
        pixels (posfeat_match_pairs_guided); device tensors in, a PairBatch out
"""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr

_MODES = {"mnn": 0, "ratio": 1, "mnn_ratio": 2}


def _dev(x):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.device.type != "cuda":
        _lib.require_device()
        x = x.to(torch.device("cuda", torch.cuda.current_device()))
    return x.float().contiguous()


def _match(d1, d2, mode, ratio=0.95):
    d1, d2 = _dev(d1), _dev(d2)
    _lib.require_device(d1)
    if d1.dim() != 2 or d2.dim() != 2 or d1.shape[1] != d2.shape[1]:
        raise ValueError("descriptors must be [n1, d] and [n2, d]")
    n1, dim = d1.shape
    n2 = d2.shape[0]
    if mode != "mnn" and min(n1, n2) < 2:
        # the reference's torch.topk(sim, 2, dim=1) / topk(sim.t(), 2, dim=1)
        # (aachen/matchers.py:21, 29, 51, 59) raise here; a second-best
        # similarity of -inf would instead pass every row through the ratio test
        raise RuntimeError("ratio matchers need at least 2 descriptors on each side "
                           "(got %d and %d): selected index k out of range" % (n1, n2))
    if n1 == 0 or n2 == 0:
        return np.zeros((0, 2), dtype=np.int64)
    if dim != 128:
        raise NotImplementedError("the matcher kernel is built for 128-d descriptors")
    need = lib().posfeat_match_workspace(n1, n2)
    ws = torch.empty(need, dtype=torch.uint8, device=d1.device)
    out = torch.empty(n1, 2, dtype=torch.int32, device=d1.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=d1.device)
    check(lib().posfeat_match(ptr(d1), n1, ptr(d2), n2, dim, _MODES[mode], float(ratio),
                              ptr(out), ptr(cnt), ptr(ws), need, stream_ptr()))
    n = int(cnt.item())
    return out[:n].cpu().numpy().astype(np.int64)


def mnn_matcher(descriptors_a, descriptors_b):
    return _match(descriptors_a, descriptors_b, "mnn")


def mutual_nn_matcher(descriptors1, descriptors2, **args):
    return _match(descriptors1, descriptors2, "mnn")


def ratio_matcher(descriptors1, descriptors2, ratio=0.95):
    return _match(descriptors1, descriptors2, "ratio", ratio)


def mutual_nn_ratio_matcher(descriptors1, descriptors2, ratio=0.95):
    return _match(descriptors1, descriptors2, "mnn_ratio", ratio)


# ---- a whole pair list per call (matchpairs.hip) ---------------------------

class PairBatch:
    """What one posfeat_match_pairs call left on the device: ``matches`` int32
    [sum n1, 2] (pair p's rows start at ``moff[p]``), ``counts`` int32 [npairs],
    plus the host tables (``set_off`` [nsets + 1], ``pairs`` [npairs, 2], int32)
    the call was planned from.  ``buf`` is the one tensor holding counts then
    matches, so a single copy brings both to the host."""

    def __init__(self, pool, set_off, pairs, moff, buf):
        self.pool, self.set_off, self.pairs, self.moff, self.buf = pool, set_off, pairs, moff, buf
        n = pairs.shape[0]
        self.counts, self.matches = buf[:n], buf[n:].view(-1, 2)

    def read(self):
        """(counts, matches) on the host: one D2H copy, one synchronisation."""
        host = torch.empty(self.buf.shape, dtype=torch.int32, pin_memory=True)
        host.copy_(self.buf, non_blocking=True)
        torch.cuda.current_stream(self.buf.device).synchronize()
        h = host.numpy()
        n = self.pairs.shape[0]
        return h[:n], h[n:].reshape(-1, 2)


def _host_ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _pool(descs):
    """the sets stacked into one device tensor [N, d] and their row offsets"""
    sizes = []
    for d in descs:
        if d.ndim != 2 or d.shape[1] != descs[0].shape[1]:
            raise ValueError("descriptors must all be [n_i, d] with one d")
        sizes.append(int(d.shape[0]))
    set_off = np.zeros(len(descs) + 1, dtype=np.int64)
    np.cumsum(sizes, out=set_off[1:])
    if set_off[-1] > np.iinfo(np.int32).max:
        raise ValueError("the descriptor pool has more than 2^31 - 1 rows")
    if all(isinstance(d, np.ndarray) for d in descs):   # one upload
        pool = _dev(np.concatenate([np.asarray(d, dtype=np.float32) for d in descs], 0))
    else:
        pool = torch.cat([_dev(d) for d in descs], 0)
    return pool, set_off.astype(np.int32)


def match_pairs_device(pool, set_off, pairs, matcher="mnn", ratio=0.95):
    """posfeat_match_pairs on a pool already on the device; returns a PairBatch
    without reading anything back (stream-ordered)."""
    _lib.require_device(pool)
    set_off = np.ascontiguousarray(set_off, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs, nsets = pairs.shape[0], set_off.shape[0] - 1
    if pairs.size and (pairs.min() < 0 or pairs.max() >= nsets):
        raise IndexError("pair index out of range for %d descriptor sets" % nsets)
    n1 = (set_off[1:] - set_off[:-1])[pairs[:, 0]].astype(np.int64)
    moff = np.concatenate([[0], np.cumsum(n1)])
    need = lib().posfeat_match_pairs_workspace(_host_ptr(set_off), nsets, _host_ptr(pairs), npairs)
    if need == 0:
        raise ValueError("invalid set offsets, or more than 2^31 - 1 match rows in one call")
    ws = torch.empty(need, dtype=torch.uint8, device=pool.device)
    buf = torch.empty(npairs + 2 * int(moff[-1]), dtype=torch.int32, device=pool.device)
    batch = PairBatch(pool, set_off, pairs, moff, buf)
    check(lib().posfeat_match_pairs(ptr(pool), _host_ptr(set_off), nsets, _host_ptr(pairs), npairs,
                                    int(pool.shape[1]), _MODES[matcher], float(ratio),
                                    ptr(batch.matches), ptr(batch.counts), ptr(ws), need,
                                    stream_ptr(pool.device)))
    return batch


_MODELS = {"homography": 0, "fundamental": 1, 0: 0, 1: 1}


def match_pairs_guided_device(pool, kp_pool, set_off, pairs, model, M, thr, matcher="mnn",
                              ratio=0.95):
    """posfeat_match_pairs_guided: match_pairs_device with the candidates of pair
    p restricted to those its model M[p] admits within ``thr`` pixels.  kp_pool:
    [N, 2] fp32 device tensor numbered as ``pool``; model: "homography" / 0 or
    "fundamental" / 1; M: [npairs, 3, 3] fp64 device tensor, what
    geometry.ransac_homography_pairs / ransac_fundamental_pairs return (a zero
    model admits nothing).  Returns a PairBatch laid out as match_pairs_device's,
    nothing read back (stream-ordered)."""
    _lib.require_device(pool)
    if matcher not in _MODES:
        raise ValueError("matcher must be one of %s" % sorted(_MODES))
    if model not in _MODELS:
        raise ValueError("model must be 'homography' (0) or 'fundamental' (1)")
    set_off = np.ascontiguousarray(set_off, dtype=np.int32)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    npairs, nsets = pairs.shape[0], set_off.shape[0] - 1
    if pairs.size and (pairs.min() < 0 or pairs.max() >= nsets):
        raise IndexError("pair index out of range for %d descriptor sets" % nsets)
    if (not torch.is_tensor(kp_pool) or kp_pool.dtype != torch.float32 or kp_pool.dim() != 2 or
            kp_pool.shape[1] != 2 or kp_pool.device != pool.device):
        raise ValueError("kp_pool must be a [N, 2] float32 tensor on the pool's device")
    if kp_pool.shape[0] < int(set_off[-1]) or pool.shape[0] < int(set_off[-1]):
        raise ValueError("the pools have fewer rows than the sets")
    if (not torch.is_tensor(M) or M.dtype != torch.float64 or M.numel() != 9 * npairs or
            M.device != pool.device):
        raise ValueError("M must be a [npairs, 3, 3] float64 tensor on the pool's device")
    if not (np.isfinite(thr) and thr > 0):
        raise ValueError("thr must be a positive number of pixels")
    kp_pool, M = kp_pool.contiguous(), M.contiguous()
    n1 = (set_off[1:] - set_off[:-1])[pairs[:, 0]].astype(np.int64)
    moff = np.concatenate([[0], np.cumsum(n1)])
    need = lib().posfeat_match_pairs_guided_workspace(_host_ptr(set_off), nsets, _host_ptr(pairs),
                                                      npairs)
    if need == 0:
        raise ValueError("invalid set offsets, or more than 2^31 - 1 match rows in one call")
    ws = torch.empty(need, dtype=torch.uint8, device=pool.device)
    buf = torch.empty(npairs + 2 * int(moff[-1]), dtype=torch.int32, device=pool.device)
    batch = PairBatch(pool, set_off, pairs, moff, buf)
    check(lib().posfeat_match_pairs_guided(
        ptr(pool), ptr(kp_pool), _host_ptr(set_off), nsets, _host_ptr(pairs), npairs,
        int(pool.shape[1]), _MODES[matcher], float(ratio), _MODELS[model], ptr(M), float(thr),
        ptr(batch.matches), ptr(batch.counts), ptr(ws), need, stream_ptr(pool.device)))
    return batch


def match_pairs(descs, pairs, matcher="mnn", ratio=0.95):
    """The per-pair matchers over a pair list: ``descs`` is a list of [n_i, 128]
    arrays / tensors, ``pairs`` a list of (i, j) indices into it (sets may be
    shared, on either side); ``matcher`` is "mnn", "ratio" or "mnn_ratio".
    Returns the list of int64 [m, 2] arrays that mnn_matcher / ratio_matcher /
    mutual_nn_ratio_matcher return for (descs[i], descs[j]) -- bit-identical,
    the similarity bits do not depend on the batching -- from four launches, one
    workspace, one device-to-host copy and one synchronisation for the whole
    list (reconstruct_pipeline.py match_features and hpatches/evaluation.py
    call the matcher once per pair)."""
    if matcher not in _MODES:
        raise ValueError("matcher must be one of %s" % sorted(_MODES))
    pairs = [(int(i), int(j)) for i, j in pairs]
    if not pairs:
        return []
    descs = list(descs)
    for i, j in pairs:
        if not (0 <= i < len(descs) and 0 <= j < len(descs)):
            raise IndexError("pair (%d, %d) out of range for %d descriptor sets"
                             % (i, j, len(descs)))
    live = False
    for i, j in pairs:
        n1, n2 = int(descs[i].shape[0]), int(descs[j].shape[0])
        if matcher != "mnn" and min(n1, n2) < 2:   # as _match: the reference's topk(2) raises
            raise RuntimeError("ratio matchers need at least 2 descriptors on each side "
                               "(got %d and %d): selected index k out of range" % (n1, n2))
        live = live or (n1 > 0 and n2 > 0)
    if not live:
        return [np.zeros((0, 2), dtype=np.int64) for _ in pairs]
    pool, set_off = _pool(descs)
    if pool.shape[1] != 128:
        raise NotImplementedError("the matcher kernel is built for 128-d descriptors")
    batch = match_pairs_device(pool, set_off, np.asarray(pairs, dtype=np.int32), matcher, ratio)
    counts, matches = batch.read()
    return [matches[batch.moff[p]:batch.moff[p] + counts[p]].astype(np.int64)
            for p in range(len(pairs))]
