"""Geometrically verified matches for a pair list, on the GPU: what the
reference's Aachen / ETH pipelines do with ``match_features`` followed by
COLMAP's ``matches_importer`` (evaluations/aachen/reconstruct_pipeline.py
match_features and geometric_verification), without the COLMAP database.

  verify_pair_list(feature_dir, pairs_file, postfix, matcher="mnn", ratio=0.95,
                   model="fundamental", chunk=1024, iters=2048, thr=4.0, seed=0,
                   output=None, intrinsics=None, guided=False) -> dict

``pairs_file`` holds one ``name1 name2`` per line (image_pairs_to_match.txt);
the features of image ``name`` are ``feature_dir/name.postfix`` as extract.py
wrote them (np.savez: keypoints, descriptors).  Per chunk of at most ``chunk``
pairs: the images the chunk names are read once and stacked into one pool,
matchers.match_pairs_device matches the chunk's pairs, then
geometry.ransac_fundamental_pairs (``model="homography"``:
ransac_homography_pairs; ``model="essential"``: ransac_essential_pairs with
the camera of every image from ``intrinsics``, a database_intrinsics.txt as
evaluation.reconstruction.read_intrinsics reads it) verifies them on the same
PairBatch; counts, matches,
models, info and masks come back in one copy with one synchronisation.  Pair p
of a chunk samples as pair p, so the result depends on ``chunk`` through the
chunking and on nothing else.

The returned dict, also written to ``output`` (np.savez) when given:
  pairs          [npairs, 2] the image names
  match_offsets  [npairs + 1] int64: pair p's rows of ``matches``
  matches        [sum, 2] int32 the inlier matches (index in 1, index in 2)
  model          [npairs, 3, 3] fp64 F (or H), zeros where none was found
  info           [npairs, 4] int32 as the RANSAC call gives it
  n_matches      [npairs] int32 the raw matches before verification
and for ``model="essential"`` only:
  pose           [npairs, 3, 4] fp64 [R | t], x2 ~ R x1 + t, |t| = 1
  cheir          [npairs, 2] int32 (decomposition index, matches in front)

``guided=True`` (COLMAP's guided matching): after RANSAC the chunk's pairs are
matched again by geometry.guided_pairs under the model just found, with the
same ``thr``, matcher and ratio, every descriptor competing only against the
keypoints the model admits (the essential model guides with F = K2^-T E K1^-1
and needs cameras without distortion, k1 = 0).  ``matches`` / ``match_offsets``
then hold the guided matches, and
  n_verified     [npairs] int32 the RANSAC inlier counts they replace
is added; still one copy and one synchronisation per chunk.  Without the flag
the output is what it always was.
"""
import os

import numpy as np
import torch

from .. import _lib, geometry, matchers
from . import reconstruction

MODELS = {"fundamental": geometry.ransac_fundamental_pairs,
          "homography": geometry.ransac_homography_pairs,
          "essential": geometry.ransac_essential_pairs}


def read_pair_list(pairs_file):
    """[(name1, name2)] of the non-empty lines"""
    pairs = []
    with open(pairs_file) as f:
        for line in f:
            parts = line.split()
            if not parts:
                continue
            if len(parts) != 2:
                raise ValueError("expected 'name1 name2' per line, got %r" % line.rstrip("\n"))
            pairs.append((parts[0], parts[1]))
    return pairs


def _read_feats(feature_dir, name, postfix):
    aux = np.load(os.path.join(feature_dir, "%s.%s" % (name, postfix)))
    return (np.ascontiguousarray(aux["keypoints"][:, :2], dtype=np.float32),
            np.ascontiguousarray(aux["descriptors"], dtype=np.float32))


def _guide_model(model, cams, images, pairs, device):
    """the 3x3 model the guided call takes: F or H as RANSAC left it; for an
    essential matrix F = K2^-T E K1^-1 (torch ops on the device, from the
    inverse calibration matrices built here on the host)"""
    if cams is None:
        return model
    kinv = np.zeros((len(images), 3, 3))
    for i, n in enumerate(images):
        fx, fy, cx, cy, k1 = (float(v) for v in cams[n][:5])
        if k1 != 0.0:
            raise ValueError("guided matching under an essential matrix needs cameras without "
                             "distortion (k1 = %g for %s)" % (k1, n))
        kinv[i] = [[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]]
    kinv = torch.from_numpy(kinv).to(device)
    k1i = kinv[torch.from_numpy(pairs[:, 0].astype(np.int64)).to(device)]
    k2i = kinv[torch.from_numpy(pairs[:, 1].astype(np.int64)).to(device)]
    return torch.matmul(k2i.transpose(1, 2), torch.matmul(model, k1i)).contiguous()


def _run_chunk(feature_dir, postfix, names, device, matcher, ratio, fit, iters, thr, seed,
               cams=None, guided=False):
    """names: [(name1, name2)] -> host (counts, matches [sum n1, 2], moff, model, info, mask),
    and with ``cams`` ({image name: camera row}, the essential model) pose and cheir; with
    ``guided`` the guided call's (counts, matches) come last"""
    images = sorted({n for pair in names for n in pair})
    index = {n: i for i, n in enumerate(images)}
    feats = [_read_feats(feature_dir, n, postfix) for n in images]
    pairs = np.asarray([(index[a], index[b]) for a, b in names], dtype=np.int32)
    npairs = pairs.shape[0]
    pool, set_off = matchers._pool([d for _, d in feats])
    if pool.shape[1] != 128:
        raise NotImplementedError("the matcher kernel is built for 128-d descriptors")
    kp_pool = torch.from_numpy(np.concatenate([k for k, _ in feats], 0)).to(device)
    batch = matchers.match_pairs_device(pool, set_off, pairs, matcher, ratio)
    extra = []
    if cams is None:
        model, info, inlier = fit(kp_pool, batch, iters=iters, thr=thr, seed=seed)
    else:
        rows = torch.from_numpy(np.stack([cams[n] for n in images]).astype(np.float64)).to(device)
        model, pose, info, cheir, inlier = fit(kp_pool, rows, batch, iters=iters, thr=thr, seed=seed)
        extra = [pose.view(torch.uint8).view(-1), cheir.view(torch.uint8).view(-1)]
    if guided:
        gbatch = geometry.guided_pairs(
            kp_pool, batch, "homography" if fit is geometry.ransac_homography_pairs
            else "fundamental", _guide_model(model, cams, images, pairs, device), thr, matcher,
            ratio)
        extra = extra + [gbatch.buf.view(torch.uint8)]
    # one synchronisation: everything into one pinned byte buffer
    parts = [batch.buf.view(torch.uint8), model.view(torch.uint8).view(-1),
             info.view(torch.uint8).view(-1), inlier] + extra
    sizes = [int(p.numel()) for p in parts]
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    at = 0
    for p, s in zip(parts, sizes):
        host[at:at + s].copy_(p, non_blocking=True)
        at += s
    torch.cuda.current_stream(device).synchronize()
    h = host.numpy()
    cuts = np.cumsum([0] + sizes)
    buf = h[cuts[0]:cuts[1]].view(np.int32)
    out = (buf[:npairs].copy(), buf[npairs:].reshape(-1, 2).copy(), batch.moff,
           h[cuts[1]:cuts[2]].view(np.float64).reshape(npairs, 3, 3).copy(),
           h[cuts[2]:cuts[3]].view(np.int32).reshape(npairs, 4).copy(),
           h[cuts[3]:cuts[4]].astype(bool))
    if cams is not None:
        out += (h[cuts[4]:cuts[5]].copy().view(np.float64).reshape(npairs, 3, 4),
                h[cuts[5]:cuts[6]].copy().view(np.int32).reshape(npairs, 2))
    if guided:
        gbuf = h[cuts[-2]:cuts[-1]].copy().view(np.int32)
        out += (gbuf[:npairs], gbuf[npairs:].reshape(-1, 2))
    return out


def verify_pair_list(feature_dir, pairs_file, postfix, matcher="mnn", ratio=0.95,
                     model="fundamental", chunk=1024, iters=None, thr=None, seed=0, output=None,
                     intrinsics=None, guided=False):
    if model not in MODELS:
        raise ValueError("model must be one of %s" % sorted(MODELS))
    if (model == "essential") != (intrinsics is not None):
        raise ValueError("the essential model, and no other, takes an intrinsics file")
    if matcher not in matchers._MODES:
        raise ValueError("matcher must be one of %s" % sorted(matchers._MODES))
    if int(chunk) < 1:
        raise ValueError("chunk must be at least one pair")
    _lib.require_device()
    device = torch.device("cuda", torch.cuda.current_device())
    fit = MODELS[model]
    # the model's own defaults (iters, thr, seed) where none is given
    iters = fit.__defaults__[0] if iters is None else int(iters)
    thr = fit.__defaults__[1] if thr is None else float(thr)
    names = read_pair_list(pairs_file)
    cams = None
    if intrinsics is not None:
        cams = {n: reconstruction.camera_row(v[0], v[3])
                for n, v in reconstruction.read_intrinsics(intrinsics).items()}
        missing = sorted({n for pair in names for n in pair} - set(cams))
        if missing:
            raise ValueError("no intrinsics for %s" % ", ".join(missing[:5]))
    kept, offsets, models, infos, raw, poses, cheirs = [], [0], [], [], [], [], []
    guided = bool(guided)
    for at in range(0, len(names), int(chunk)):
        part = names[at:at + int(chunk)]
        got = _run_chunk(feature_dir, postfix, part, device, matcher, ratio, fit, iters, thr, seed,
                         cams, guided)
        counts, matches, moff, M, info, mask = got[:6]
        if cams is not None:
            poses.append(got[6])
            cheirs.append(got[7])
        for p in range(len(part)):
            if guided:
                gcounts, gmatches = got[-2:]
                kept.append(gmatches[int(moff[p]):int(moff[p]) + int(gcounts[p])])
            else:
                rows = slice(int(moff[p]), int(moff[p]) + int(counts[p]))
                kept.append(matches[rows][mask[rows]])
            offsets.append(offsets[-1] + kept[-1].shape[0])
        models.append(M)
        infos.append(info)
        raw.append(counts)
    n = len(names)
    out = dict(
        pairs=np.asarray(names, dtype=str).reshape(n, 2),
        match_offsets=np.asarray(offsets, dtype=np.int64),
        matches=(np.concatenate(kept, 0) if kept else np.zeros((0, 2))).astype(np.int32),
        model=np.concatenate(models, 0) if models else np.zeros((0, 3, 3)),
        info=np.concatenate(infos, 0) if infos else np.zeros((0, 4), np.int32),
        n_matches=np.concatenate(raw, 0) if raw else np.zeros(0, np.int32))
    if cams is not None:
        out.update(pose=np.concatenate(poses, 0) if poses else np.zeros((0, 3, 4)),
                   cheir=np.concatenate(cheirs, 0) if cheirs else np.zeros((0, 2), np.int32))
    if guided:
        out.update(n_verified=out["info"][:, 1].astype(np.int32))
    if output is not None:
        with open(output, "wb") as f:
            np.savez(f, **out)
    return out
