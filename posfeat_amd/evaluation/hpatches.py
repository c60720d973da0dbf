"""HPatches mean matching accuracy (MMA) of a directory written by extract.py
-- evaluations/hpatches/evaluation.py of the reference without its CUDA torch,
scipy, matplotlib, hard-coded paths and run-on-import:

  benchmark_features(features_path, dataset_path, postfix, ...)
        evaluation.py:40-96 with the read function of lines 106-115: returns
        (i_err, v_err, [seq_type, n_feats, n_matches]) with the reference's
        types (dicts keyed by the thresholds 1..15 summing the per-pair
        ``mean(dist <= thr)``; numpy arrays).
  mma_score(i_err, v_err, n_i, n_v)      evaluation.py:160-179
  summary_lines(stats)                   evaluation.py:98-105
  format_row(name, stats, score)         evaluation.py:245-257 (one line)

The sequences are processed in chunks sized by a descriptor-pool byte budget;
each chunk is ONE posfeat_match_pairs call (mutual nearest neighbours of image
1 against images 2..6 of every sequence in the chunk: matchers.match_pairs_device)
and ONE posfeat_reproj_hist call (the homography check of lines 69-90, fp64 on
the device), and the host reads the counts and the integer histograms once per
chunk.  n_i / n_v are counted from the sequences present (52 / 56 on the full
dataset, the reference's constants).

  benchmark_homography(features_path, dataset_path, postfix, ...)
        the homography estimation accuracy reported beside MMA: per chunk one
        more call, geometry.ransac_homography_pairs (ransac.hip), on the same
        matches; the corner error against H_1_k on the host.
  homography_lines(acc)                  its printed rows

Out of scope: the plots (evaluation.py:181-243) and the readers of the other
methods' ``.mat`` / hesaff files (lines 117-129, 143-147).
"""
import ctypes
import os

import numpy as np
import torch

from .. import _lib, matchers
from .._lib import check, lib, ptr, stream_ptr
from ..datasets import _ppm_header

LIM = (1, 15)                               # evaluation.py:24-25
RNG = np.arange(LIM[0], LIM[1] + 1)
MAX_KP = 60000                              # evaluation.py:52-54, 59-61
POOL_BYTES = 512 << 20                      # descriptor pool of one chunk


def _read_feats(features_path, seq, idx, extension, postfix, top_k, max_kp):
    """evaluation.py:106-115 then the row cut of lines 52-54"""
    aux = np.load(os.path.join(features_path, seq, "%d.%s.%s" % (idx, extension, postfix)))
    kp, desc = aux["keypoints"], aux["descriptors"]
    if top_k is not None:
        assert "scores" in aux
        ids = np.argsort(aux["scores"])[-top_k:]
        kp, desc = kp[ids, :], desc[ids, :]
    if kp.shape[0] > max_kp:
        kp, desc = kp[:max_kp, :], desc[:max_kp, :]
    return (np.ascontiguousarray(kp[:, :2], dtype=np.float32),
            np.ascontiguousarray(desc, dtype=np.float32))


def reproj_hist(kp_pool, batch, H, nthr=LIM[1]):
    """posfeat_reproj_hist on what ``batch`` (matchers.PairBatch) holds: kp_pool
    [N, 2] fp32 and H [npairs, 9] fp64 device tensors -> int32 [npairs, nthr]
    device tensor, stream-ordered."""
    npairs = batch.pairs.shape[0]
    need = lib().posfeat_reproj_hist_workspace(npairs)
    ws = torch.empty(need, dtype=torch.uint8, device=kp_pool.device)
    hist = torch.empty(npairs, nthr, dtype=torch.int32, device=kp_pool.device)
    check(lib().posfeat_reproj_hist(
        ptr(kp_pool), ctypes.c_void_p(batch.set_off.ctypes.data), batch.set_off.shape[0] - 1,
        ctypes.c_void_p(batch.pairs.ctypes.data), npairs, ptr(batch.matches), ptr(batch.counts),
        ptr(H), nthr, ptr(hist), ptr(ws), need, stream_ptr(kp_pool.device)))
    return hist


def _run_chunk(chunk, device):
    """chunk: [(kps[6], descs[6], Hs[5])] -> (counts [5 n], hist [5 n, 15]) on the host"""
    descs = [d for _, ds, _ in chunk for d in ds]
    kps = [k for ks, _, _ in chunk for k in ks]
    pairs = np.asarray([(6 * s, 6 * s + k) for s in range(len(chunk)) for k in range(1, 6)],
                       dtype=np.int32)
    H = np.stack([h.reshape(9) for _, _, hs in chunk for h in hs]).astype(np.float64)
    npairs = pairs.shape[0]
    sizes = np.asarray([d.shape[0] for d in descs])
    alive = (sizes[pairs[:, 0]] > 0) & (sizes[pairs[:, 1]] > 0)
    if not alive.any():
        return np.zeros(npairs, np.int32), np.zeros((npairs, LIM[1]), np.int32)
    pool, set_off = matchers._pool(descs)
    if pool.shape[1] != 128:
        raise NotImplementedError("the matcher kernel is built for 128-d descriptors")
    kp_pool = torch.from_numpy(np.concatenate(kps, 0)).to(device)
    batch = matchers.match_pairs_device(pool, set_off, pairs, "mnn")
    hist = reproj_hist(kp_pool, batch, torch.from_numpy(H).to(device))
    # one synchronisation: counts and histograms into one pinned buffer
    host = torch.empty(npairs * (1 + LIM[1]), dtype=torch.int32, pin_memory=True)
    host[:npairs].copy_(batch.counts, non_blocking=True)
    host[npairs:].copy_(hist.view(-1), non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    h = host.numpy()
    return h[:npairs].copy(), h[npairs:].reshape(npairs, LIM[1]).copy()


def _iter_chunks(features_path, dataset_path, postfix, extension, top_k, max_kp, pool_bytes):
    """the sequences in name order, grouped into chunks of at most pool_bytes of
    descriptors: yields ([(kps[6], descs[6], Hs[5])], [sequence name])"""
    seq_names = sorted(n for n in os.listdir(dataset_path)
                       if os.path.isdir(os.path.join(dataset_path, n)))
    chunk, names, held = [], [], 0
    for seq in seq_names:
        kps, descs = [], []
        for idx in range(1, 7):
            kp, desc = _read_feats(features_path, seq, idx, extension, postfix, top_k, max_kp)
            kps.append(kp)
            descs.append(desc)
        Hs = [np.loadtxt(os.path.join(dataset_path, seq, "H_1_%d" % idx)) for idx in range(2, 7)]
        size = sum(d.nbytes for d in descs)
        if chunk and held + size > pool_bytes:
            yield chunk, names
            chunk, names, held = [], [], 0
        chunk.append((kps, descs, Hs))
        names.append(seq)
        held += size
    if chunk:
        yield chunk, names


def benchmark_features(features_path, dataset_path, postfix, extension="ppm", top_k=None,
                       max_kp=MAX_KP, pool_bytes=POOL_BYTES):
    _lib.require_device()
    device = torch.device("cuda", torch.cuda.current_device())
    n_feats, n_matches, seq_type = [], [], []
    i_err = {thr: 0 for thr in RNG}
    v_err = {thr: 0 for thr in RNG}
    for chunk, names in _iter_chunks(features_path, dataset_path, postfix, extension, top_k,
                                     max_kp, pool_bytes):
        n_feats += [kp.shape[0] for kps, _, _ in chunk for kp in kps]
        counts, hist = _run_chunk(chunk, device)
        for p in range(counts.shape[0]):
            name = names[p // 5]
            n_matches.append(int(counts[p]))
            seq_type.append(name[0])
            err = i_err if name[0] == "i" else v_err
            for thr in RNG:
                # mean(dist <= thr); a pair without matches is the reference's [inf]: 0
                err[thr] += (hist[p, thr - 1] / np.float64(counts[p])) if counts[p] else 0.0
    return i_err, v_err, [np.array(seq_type), np.array(n_feats), np.array(n_matches)]


# ---- homography estimation accuracy (ransac.hip) -----------------------------

HA_EPS = (1, 3, 5)


def _image_size(dataset_path, seq, extension):
    """(w, h) of <seq>/1.<extension> from its header"""
    path = os.path.join(dataset_path, seq, "1." + extension)
    with open(path, "rb") as f:
        hdr = _ppm_header(f)
    if hdr is not None:
        return hdr[0], hdr[1]
    from PIL import Image
    with Image.open(path) as im:
        return im.size


def corner_error(H_est, H_gt, w, h):
    """mean distance, over the corners (0,0), (w-1,0), (w-1,h-1), (0,h-1) of
    image 1, between their warps by the two homographies (fp64, host)"""
    c = np.array([[0, 0, 1], [w - 1, 0, 1], [w - 1, h - 1, 1], [0, h - 1, 1]], np.float64)
    with np.errstate(all="ignore"):
        a = c @ np.asarray(H_est, np.float64).reshape(3, 3).T
        b = c @ np.asarray(H_gt, np.float64).reshape(3, 3).T
        d = a[:, :2] / a[:, 2:] - b[:, :2] / b[:, 2:]
        return float(np.mean(np.sqrt(np.sum(d ** 2, axis=1))))


def _run_chunk_homography(chunk, device, iters, thr, seed):
    """chunk -> (H [5 n, 3, 3] fp64, info [5 n, 4] int32) on the host: one
    match_pairs_device call, one ransac_homography_pairs call, one transfer"""
    from .. import geometry
    descs = [d for _, ds, _ in chunk for d in ds]
    kps = [k for ks, _, _ in chunk for k in ks]
    pairs = np.asarray([(6 * s, 6 * s + k) for s in range(len(chunk)) for k in range(1, 6)],
                       dtype=np.int32)
    npairs = pairs.shape[0]
    sizes = np.asarray([d.shape[0] for d in descs])
    failed = np.tile(np.asarray([1, 0, -1, 0], np.int32), (npairs, 1))
    if not ((sizes[pairs[:, 0]] > 0) & (sizes[pairs[:, 1]] > 0)).any():
        return np.zeros((npairs, 3, 3)), failed
    pool, set_off = matchers._pool(descs)
    if pool.shape[1] != 128:
        raise NotImplementedError("the matcher kernel is built for 128-d descriptors")
    kp_pool = torch.from_numpy(np.concatenate(kps, 0)).to(device)
    batch = matchers.match_pairs_device(pool, set_off, pairs, "mnn")
    H, info, _ = geometry.ransac_homography_pairs(kp_pool, batch, iters, thr, seed)
    both = torch.cat([H.view(-1).view(torch.uint8), info.view(-1).view(torch.uint8)])
    host = torch.empty(both.shape, dtype=torch.uint8, pin_memory=True)
    host.copy_(both, non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    h = host.numpy()
    return (h[:npairs * 72].view(np.float64).reshape(npairs, 3, 3).copy(),
            h[npairs * 72:].view(np.int32).reshape(npairs, 4).copy())


def benchmark_homography(features_path, dataset_path, postfix, extension="ppm", top_k=None,
                         iters=1024, thr=3.0, seed=0, eps=HA_EPS, max_kp=MAX_KP,
                         pool_bytes=POOL_BYTES):
    """HPatches homography estimation accuracy: per pair (image 1 against images
    2..6) a RANSAC homography on the mutual-nearest-neighbour matches, scored by
    the mean distance between the four corners of image 1 warped by the
    estimate and by H_1_k; a pair is correct at eps iff that is <= eps, a pair
    without a model (status 1) is wrong at every eps.  The same chunks as
    benchmark_features; pair p of a chunk samples as pair p (so the estimates
    depend on pool_bytes through the chunking, not on anything else).  Returns
    (corner_err [npairs] fp64, inf where no model was found;
     {"all" | "i" | "v": {eps: accuracy}}, nan for an absent class;
     seq_type [npairs])."""
    _lib.require_device()
    device = torch.device("cuda", torch.cuda.current_device())
    errs, seq_type = [], []
    for chunk, names in _iter_chunks(features_path, dataset_path, postfix, extension, top_k,
                                     max_kp, pool_bytes):
        H, info = _run_chunk_homography(chunk, device, iters, thr, seed)
        for p in range(H.shape[0]):
            name = names[p // 5]
            w, h = _image_size(dataset_path, name, extension)
            seq_type.append(name[0])
            errs.append(corner_error(H[p], chunk[p // 5][2][p % 5], w, h)
                        if info[p, 0] == 0 else float("inf"))
    errs, seq_type = np.asarray(errs, np.float64), np.asarray(seq_type)
    acc = {}
    for key, sel in (("all", np.ones(errs.shape[0], bool)), ("i", seq_type == "i"),
                     ("v", seq_type == "v")):
        acc[key] = {e: float(np.mean(errs[sel] <= e)) if sel.any() else float("nan")
                    for e in eps}
    return errs, acc, seq_type


def homography_lines(acc):
    """one line per eps: the accuracy overall and for the i / v sequences"""
    return ["# Homography accuracy @{:g}px: Overall {:.3f}, Illumination {:.3f}, Viewpoint {:.3f}"
            .format(e, acc["all"][e], acc["i"][e], acc["v"][e]) for e in sorted(acc["all"])]


def seq_counts(stats):
    """(n_i, n_v): illumination / viewpoint sequences present (5 pairs each)"""
    seq_type = np.asarray(stats[0])
    return int(np.sum(seq_type == "i")) // 5, int(np.sum(seq_type == "v")) // 5


def summary_lines(stats):
    seq_type, n_feats, n_matches = stats
    n_i, n_v = seq_counts(stats)
    per = lambda s, n: s / (n * 5) if n else float("nan")
    return ["# Features: {:f} - [{:d}, {:d}]".format(np.mean(n_feats), np.min(n_feats),
                                                     np.max(n_feats)),
            "# Matches: Overall {:f}, Illumination {:f}, Viewpoint {:f}".format(
                per(np.sum(n_matches), n_i + n_v), per(np.sum(n_matches[seq_type == "i"]), n_i),
                per(np.sum(n_matches[seq_type == "v"]), n_v))]


def mma_score(i_err, v_err, n_i, n_v):
    """(overall, illumination, viewpoint): the MMA over thresholds 1..10 weighted
    by 2 - thr / 10 and normalised by the weights' sum; nan for an absent class"""
    cur_a = cur_i = cur_v = upper_bound = 0
    for idx, thr in enumerate(range(1, 11)):
        w = 2 - (idx + 1) / 10.
        cur_a += w * ((i_err[thr] + v_err[thr]) / ((n_i + n_v) * 5)) if n_i + n_v else float("nan")
        cur_i += w * (i_err[thr] / (n_i * 5)) if n_i else float("nan")
        cur_v += w * (v_err[thr] / (n_v * 5)) if n_v else float("nan")
        upper_bound += w * 1
    return cur_a / upper_bound, cur_i / upper_bound, cur_v / upper_bound


def format_row(name, stats, score):
    """the reference's hseq*.txt line: name & #features & #matches & MMA scores"""
    seq_type, n_feats, n_matches = stats
    n_i, n_v = seq_counts(stats)
    num_match = np.sum(n_matches) / ((n_i + n_v) * 5) if n_i + n_v else float("nan")
    return "{} & {:.1f} & {:.1f} & {:.3f} & {:.3f} & {:.3f}\n".format(
        name.ljust(25, " "), np.mean(n_feats), num_match, score[0], score[1], score[2])
