"""detect.hip and sample.hip on the branches the friendly inputs never enter:
the generic sampler (every CPL instantiation, padded and misaligned storage),
thr_mod="mean" / "max" thresholds, negative scores (the T < ZKEY scan), no
survivors, odd and tiny maps, det_mask_kernel's second loop trip (A/B build),
nms_mask on signed maps with ties, and the sampler's n_valid / zero-norm /
argument-check edges.

References: oracle/detect_ref.py (pinned against torch fp64 at these inputs by
tests/test_oracle_edges.py, whose input builders are used here).  The detector
is compare / integer work: n, counts, idx and score are bit-exact; the
soft-argmax coordinate is fp32 arithmetic, compared at the suite's 1e-5 scaled
by the quotient's condition number where scores are signed.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import detect_ref
from test_oracle_edges import (MEAN_CASES, NMS_SIZES, SAMPLE_CASES, ZERO_ROWS, mean_map,
                               nms_radii, quantised_map, sample_inputs)

pytestmark = pytest.mark.gpu


# ================================================================== detector
def _box3(a):
    h, w = a.shape
    s = np.zeros((h - 2, w - 2), np.float64)
    for dy in range(3):
        for dx in range(3):
            s += a[dy:dy + h - 2, dx:dx + w - 2]
    return s


def _coord_check(km_i, idx, coord, c_ref, signed, what):
    """coord [n,2] of one image against the oracle's.  Positive scores: the
    suite's atol 1e-5.  Signed scores: 1e-5 * sum|v| / |sum v| over the row's
    3x3 window (the same tolerance times the condition number of the
    soft-argmax quotient); rows with sum v == 0 (0/0 or x/0 in the reference
    too) are skipped here only, and must be fewer than 1 % of the rows.
    Returns the largest error as a fraction of its bound."""
    n = idx.shape[0]
    if not signed:
        bound = np.full(n, 1e-5)
        use = np.ones(n, bool)
    else:
        m = km_i.astype(np.float64)
        s, a = _box3(m).reshape(-1)[idx], _box3(np.abs(m)).reshape(-1)[idx]
        use = s != 0
        assert (~use).sum() < 0.01 * n, what
        bound = 1e-5 * a / np.where(use, np.abs(s), 1.0)
    err = np.abs(coord.astype(np.float64) - c_ref.astype(np.float64)).max(1)
    frac = float((err[use] / bound[use]).max()) if use.any() else 0.0
    bad = ~(err[use] <= bound[use])  # (a NaN from the device fails here)
    assert not bad.any(), "%s: coord error %.3g of its bound (%d rows)" % (what, frac, bad.sum())
    return frac


def _detect_and_check(gpu, km, r, num_pts, use_nms=True, thr=False, thr_mod="mean", signed=False,
                      coords=True):
    """posfeat_detect on the batch against the oracle on the batch, and
    posfeat_detect_each against the oracle on every image alone: n, counts,
    idx, score bit for bit, coord within its bound (``coords=False``: a map of
    a few signed levels, whose 3x3 sums are zero in many windows).  Returns (n
    of the batch call, counts, idx of the batch call, worst coord error /
    bound)."""
    from posfeat_amd import ops
    b = km.shape[0]
    what = "%dx%d r%d n%s nms%d thr%s/%s" % (km.shape[2], km.shape[3], r, num_pts, use_nms, thr,
                                             thr_mod)
    t = torch.from_numpy(km).to(gpu)
    cnt_ref = detect_ref.detector_count(km, r, use_nms, thr, thr_mod)
    frac = 0.0
    # --- one n for the batch
    c_ref, s_ref, i_ref = detect_ref.generate_kpts_single(km, r, num_pts, use_nms=use_nms, thr=thr,
                                                          thr_mod=thr_mod, return_idx=True)
    idx, coord, score, counts, n = ops.detect(t, r, num_pts, use_nms=use_nms, thr=thr,
                                              thr_mod=thr_mod)
    idx_b = idx.cpu().numpy()
    assert n == i_ref.shape[1], what
    np.testing.assert_array_equal(counts.cpu().numpy(), cnt_ref, err_msg=what)
    np.testing.assert_array_equal(idx_b, i_ref, err_msg=what)
    np.testing.assert_array_equal(score.cpu().numpy(), s_ref, err_msg=what)
    for i in range(b if coords else 0):
        frac = max(frac, _coord_check(km[i, 0], i_ref[i], coord[i].cpu().numpy(), c_ref[i], signed,
                                      what + " img%d" % i))
    # --- every image as if detected alone
    idx, coord, score, counts, nsel = ops.detect(t, r, num_pts, use_nms=use_nms, thr=thr,
                                                 thr_mod=thr_mod, sync=False, each=True)
    nsel = nsel.cpu().numpy()
    np.testing.assert_array_equal(counts.cpu().numpy(), cnt_ref, err_msg=what + " each")
    for i in range(b):
        c_ref, s_ref, i_ref = detect_ref.generate_kpts_single(
            km[i:i + 1], r, num_pts, use_nms=use_nms, thr=thr, thr_mod=thr_mod, return_idx=True)
        k = int(nsel[i])
        assert k == i_ref.shape[1], what + " each img%d" % i
        np.testing.assert_array_equal(idx[i, :k].cpu().numpy(), i_ref[0], err_msg=what)
        np.testing.assert_array_equal(score[i, :k].cpu().numpy(), s_ref[0], err_msg=what)
        if coords:
            frac = max(frac, _coord_check(km[i, 0], i_ref[0], coord[i, :k].cpu().numpy(), c_ref[0],
                                          signed, what + " each img%d" % i))
    print("%s: n %d counts %s coord err %.3f of bound" % (what, n, cnt_ref.tolist(), frac))
    return n, cnt_ref, idx_b, frac


ODD_SIZES = [(37, 53), (33, 131), (13, 15), (10, 18), (5, 67), (67, 5)]


@pytest.mark.parametrize("h,w", ODD_SIZES)
def test_detector_odd_and_tiny_sizes(gpu, h, w):
    """lin_m11 at odd n, reflect padding up to r = Hi - 1 (r = 2 on the 3-wide
    maps), P = 128 exactly (10x18), just above (13x15: 143), below one
    1024-pixel block; n raised to 128 and clamped to P."""
    km = np.random.RandomState(h * 1000 + w).rand(2, 1, h, w).astype(np.float32)
    P = (h - 2) * (w - 2)
    ns = set()
    for r in (1, 2, 3):
        if r >= min(h - 2, w - 2):
            continue
        for num_pts in (300, False):
            n, counts, _, _ = _detect_and_check(gpu, km, r, num_pts)
            ns.add(n)
            assert n == min(max(min(num_pts or P, counts.min()), 128), P)
    if (h, w) == (37, 53):
        assert 128 in ns and max(ns) > 128    # the raise to 128 and a real count
    if (h, w) == (10, 18):
        assert ns == {128} and P == 128       # n = P: every inner cell selected
    if min(h, w) == 5:
        assert min(h - 2, w - 2) == 3          # r = 2 ran: the reflect limit


def test_detector_rejects_what_reflect_cannot_pad(gpu):
    from posfeat_amd import ops
    km = torch.rand(1, 1, 5, 67, device=gpu)
    for r in (3, 4):                           # r >= Hi = 3 with NMS on
        with pytest.raises(RuntimeError):
            ops.detect(km, r, 300)
    with pytest.raises(RuntimeError):          # Wi = 3
        ops.detect(torch.rand(1, 1, 67, 5, device=gpu), 3, 300)
    with pytest.raises(RuntimeError):          # no inner cell at all
        ops.detect(torch.rand(1, 1, 2, 200, device=gpu), 1, 300)


@pytest.mark.parametrize("h,w,thr", MEAN_CASES)
def test_detector_mean_and_max_threshold(gpu, h, w, thr):
    """det_thr_kernel: mode 3 (fp64 sum / P * thr, the reference's default
    thr_mod) and mode 2, one threshold per image.  The inputs keep every score
    more than 32 ulp from the threshold (test_oracle_edges), so the mask is
    bit-exact whichever way the mean is rounded."""
    km = mean_map(h, w)
    for mod, t in (("mean", thr), ("max", 0.5)):
        for num_pts in (300, False):
            _, counts, _, _ = _detect_and_check(gpu, km, 1, num_pts, thr=t, thr_mod=mod)
            assert len(set(counts.tolist())) > 1, (mod, counts)


def _negative_map():
    km = (np.random.RandomState(3).rand(2, 1, 37, 53) - 0.4).astype(np.float32)
    km[0, 0, 5, 5:9] = -0.0
    km[1, 0, 7, 7] = 0.0
    return km


def test_detector_negative_scores_no_nms(gpu):
    """Every cell kept, n beyond the non-negative cells: the cut is a negative
    key (det_select_kernel's T < ZKEY scan), pf_fkey orders negative values,
    and -0.0 == +0.0: the planted zeros rank by index, after every positive
    score and before every negative one."""
    km = _negative_map()
    inner = km[:, 0, 1:-1, 1:-1].reshape(2, -1)
    P = inner.shape[1]
    nonneg = (inner >= 0).sum(1)
    assert P == 1785 and nonneg.tolist() == [1087, 1055]
    zeros = [np.flatnonzero(inner[i] == 0) for i in range(2)]
    assert [z.tolist() for z in zeros] == [[4 * 51 + 4 + k for k in range(4)], [6 * 51 + 6]]
    assert np.signbit(inner[0, zeros[0]]).all() and not np.signbit(inner[1, zeros[1]]).any()
    worst = 0.0
    for num_pts in (False, 1500, 1700):
        n, counts, idx, frac = _detect_and_check(gpu, km, 1, num_pts, use_nms=False, signed=True)
        worst = max(worst, frac)
        assert counts.tolist() == [P, P] and n == (num_pts or P) and n > nonneg.max()
        for i in range(2):
            v = inner[i][idx[i]]
            npos = int((inner[i] > 0).sum())
            assert (v[:npos] > 0).all() and (v[npos + len(zeros[i]):] < 0).all()
            assert (np.diff(v[npos + len(zeros[i]):]) <= 0).all()   # negatives descending
            np.testing.assert_array_equal(idx[i, npos:npos + len(zeros[i])], zeros[i])
    print("negative scores, no nms: worst coord error %.3f of its bound" % worst)


def test_detector_negative_ties_at_cut(gpu):
    """Five signed levels, every cell kept: the cut falls inside the -1/3 level
    (n = 1300), inside the -2/3 level (1500) and five cells short of all
    (P - 5).  In the T < ZKEY scan the keys equal to T are more than are
    taken: the lowest indices win, the rest of the level stays out."""
    km = np.stack([quantised_map(37, 53), quantised_map(37, 53, seed=1)])[:, None]
    inner = km[:, 0, 1:-1, 1:-1].reshape(2, -1)
    P = inner.shape[1]
    for num_pts in (1300, 1500, P - 5):
        n, counts, idx, _ = _detect_and_check(gpu, km, 1, num_pts, use_nms=False, coords=False)
        assert n == num_pts and counts.tolist() == [P, P]
        for i in range(2):
            v = inner[i][idx[i]]
            cut = v[-1]
            level = np.flatnonzero(inner[i] == cut)
            taken = idx[i][v == cut]
            assert cut < 0 and 0 < len(taken) < len(level)      # the level is split
            np.testing.assert_array_equal(taken, level[:len(taken)])


def test_detector_negative_survivors_rank_after_zero_fill(gpu):
    """NMS on signed scores: local maxima below zero survive and are counted
    (they sit in the candidate list and in the radix histogram), but the
    masked-out cells' zeros rank ahead of them: with n = min count the fill is
    zeros by ascending index (the T == ZKEY branch), never a negative key."""
    km = _negative_map()
    # rand - 0.4 alone: a 3x3 maximum is hardly ever below zero (0.4^9), so
    # every survivor is positive and n = min count takes survivors only
    n, counts, idx, frac = _detect_and_check(gpu, km, 1, False, use_nms=True, signed=True)
    assert n == counts.min()
    # rows 19.. all negative: their local maxima survive with negative keys
    km[:, :, 19:] -= np.float32(0.7)
    assert km[:, :, 19:].max() < 0
    inner = km[:, 0, 1:-1, 1:-1].reshape(2, -1)
    n, counts, idx, frac2 = _detect_and_check(gpu, km, 1, False, use_nms=True, signed=True)
    print("negative scores, nms: coord error %.3f of its bound" % max(frac, frac2))
    for i in range(2):
        mask = detect_ref.nms(km[i, 0, 1:-1, 1:-1], 1).reshape(-1)
        masked = np.where(mask, inner[i], np.float32(0))
        npos, nneg = int((masked > 0).sum()), int((masked < 0).sum())
        assert nneg > 50 and counts[i] >= npos + nneg    # negative survivors are counted
        assert npos < n                                 # so the zero fill is entered
        v = masked[idx[i]]
        assert (v[:npos] > 0).all() and (v[npos:] == 0).all()
        fill = idx[i, npos:]
        np.testing.assert_array_equal(fill, np.flatnonzero(masked == 0)[:n - npos])


def test_detector_no_survivors(gpu):
    """count == 0: every selected row comes from the zero fill, in index order."""
    km = np.random.RandomState(9).rand(2, 1, 37, 53).astype(np.float32)
    for use_nms in (True, False):
        n, counts, idx, _ = _detect_and_check(gpu, km, 1, 300, use_nms=use_nms, thr=2.0,
                                              thr_mod="abs")
        assert n == 128 and counts.tolist() == [0, 0]
        np.testing.assert_array_equal(idx, np.tile(np.arange(128), (2, 1)))


@pytest.mark.parametrize("h,w", [(20, 30), (37, 53)])
def test_detector_constant_map(gpu, h, w):
    """All scores 0.5.  NMS keeps nothing (every window's first maximum is an
    earlier cell, or the reflected copy of one).  Without NMS every cell ties
    at the cut: 504 equal keys at 20x30 (ranked by index in LDS), 1785 at
    37x53 (more than the 1024 the LDS list holds: the ordered-scan fallback)."""
    km = np.full((2, 1, h, w), 0.5, np.float32)
    P = (h - 2) * (w - 2)
    n, counts, idx, _ = _detect_and_check(gpu, km, 1, 300, use_nms=True)
    assert n == 128 and counts.tolist() == [0, 0]
    for num_pts in (300, False):
        n, counts, idx, _ = _detect_and_check(gpu, km, 1, num_pts, use_nms=False)
        assert counts.tolist() == [P, P] and n == (num_pts or P)
        np.testing.assert_array_equal(idx, np.tile(np.arange(n), (2, 1)))


@pytest.mark.parametrize("h,w", NMS_SIZES)
def test_nms_mask_signed_ties(gpu, h, w):
    from posfeat_amd import ops
    score = np.stack([quantised_map(h, w), quantised_map(h, w, seed=1)])[:, None]
    t = torch.from_numpy(score).to(gpu)
    for r in nms_radii(h, w):
        got = ops.nms_mask(t, r).cpu().numpy()
        for i in range(2):
            np.testing.assert_array_equal(got[i, 0], detect_ref.nms(score[i, 0], r),
                                          err_msg="r=%d img%d" % (r, i))
    with pytest.raises(RuntimeError):
        ops.nms_mask(t, min(h, w))


# ------------------------------------------------------------------ A/B: POSFEAT_DET_PX
def _px_small_cases():
    return [("m37", mean_map(37, 53), dict(nms_radius=1, num_pts=300, thr=1.2, thr_mod="mean")),
            ("m120", mean_map(120, 160), dict(nms_radius=1, num_pts=False, thr=1.0,
                                              thr_mod="mean"))]


BIG = dict(nms_radius=1, num_pts=4096, thr=0.9, thr_mod="abs")


def _big_map():
    """P = 1027^2 = 1 054 729 > 1024 * 1024: with one pixel per thread the
    1024 blocks of det_mask_kernel<1> cover 1 048 576 cells per trip, and
    blocks 0-6 take a second one."""
    return np.random.RandomState(1029).rand(1, 1, 1029, 1029).astype(np.float32)


def _px_run(cases):
    from posfeat_amd import ops
    out = {}
    for name, km, kw in cases:
        idx, coord, score, counts, n = ops.detect(torch.from_numpy(km).cuda(), **kw)
        for k, v in (("idx", idx), ("coord", coord), ("score", score), ("counts", counts)):
            out["%s_%s" % (name, k)] = v.cpu().numpy()
    return out


AB_PX = r"""
import os
os.environ["POSFEAT_DET_PX"] = %(px)r
import numpy as np
from posfeat_amd import _lib
assert _lib.lib().posfeat_ab_build() == 1
import test_gpu_detect_sample_edges as T
cases = T._px_small_cases()
if %(px)r == "1":
    cases.append(("big", T._big_map(), T.BIG))
np.savez(%(out)r, **T._px_run(cases))
"""


@pytest.mark.parametrize("px", ["1", "8"])
def test_det_mask_pixels_per_thread_ab(gpu, px, tmp_path):
    """det_mask_kernel<1> and <8> (A/B build, POSFEAT_DET_PX) give what the
    default <4> gives, bit for bit; and <1> on a map of more than 1024 * 1024
    inner cells, where blocks run the loop a second time (s_cnt re-zeroed,
    s_base reused), is bit-exact against the oracle."""
    from conftest import run_ab_child
    out = str(tmp_path / "det_px.npz")
    ab = run_ab_child(AB_PX % dict(px=px, out=out), out)
    ref = _px_run(_px_small_cases())
    assert len(set(ref["m37_counts"].tolist())) > 1
    for k in ref:
        np.testing.assert_array_equal(ab[k], ref[k], err_msg=k)
    if px == "1":
        km = _big_map()
        assert (km.shape[2] - 2) * (km.shape[3] - 2) > 1024 * 1024
        c_ref, s_ref, i_ref = detect_ref.generate_kpts_single(
            km, BIG["nms_radius"], BIG["num_pts"], thr=BIG["thr"], thr_mod=BIG["thr_mod"],
            return_idx=True)
        cnt = detect_ref.detector_count(km, 1, True, BIG["thr"], BIG["thr_mod"])
        assert cnt[0] > 4096 and i_ref.max() >= 1024 * 1024  # second-trip cells are selected
        np.testing.assert_array_equal(ab["big_counts"], cnt)
        np.testing.assert_array_equal(ab["big_idx"], i_ref)
        np.testing.assert_array_equal(ab["big_score"], s_ref)
        np.testing.assert_allclose(ab["big_coord"], c_ref, atol=1e-5, rtol=0)


# ================================================================== sampler
PAD = np.float32(1e30)


def _nhwc(x, cs):
    """x [b,c,h,w] -> NHWC [b,h,w,cs], the pad lanes filled with 1e30 (a read
    past channel C shows in the output)."""
    b, c, h, w = x.shape
    m = np.full((b, h, w, cs), PAD, np.float32)
    m[..., :c] = x.transpose(0, 2, 3, 1)
    return m


def _sample(gpu, x, coord, cs, normalize, **kw):
    from posfeat_amd import ops
    fmap = torch.from_numpy(_nhwc(x, cs)).to(gpu)
    assert fmap.data_ptr() % 16 == 0
    return ops.sample_desc_nhwc(fmap, torch.from_numpy(coord).to(gpu), c=x.shape[1],
                                normalize=normalize, **kw).cpu().numpy()


# every generic instantiation (CPL 1, 2, 4, 16), and C = 128 on aligned
# storage: the half-wave kernel, under the same bounds
RAW_CASES = SAMPLE_CASES + [(128, 6, 7)]


def _raw_errors(gpu, c, h, w):
    """(|got - ref|, worst over cstride = C and C + 3, and the bound
    1e-6 * sum_taps |w v|) per output, fp64.  The oracle applied to |x| is
    that sum: the same taps, and the weights are non-negative."""
    x, coord = sample_inputs(c, h, w)
    ref = detect_ref.sample_feat_by_coord(x, coord, norm=False).astype(np.float64)
    s = detect_ref.sample_feat_by_coord(np.abs(x), coord, norm=False).astype(np.float64)
    err = np.zeros_like(ref)
    for cs in ((c, c + 3) if c != 128 else (128, 132)):
        got = _sample(gpu, x, coord, cs, False)
        assert np.isfinite(got).all() and np.abs(got).max() < 1e3, "pad lane read (cs=%d)" % cs
        err = np.maximum(err, np.abs(got - ref))
    return err, 1e-6 * s


def _worst(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(frac.max()), float((frac > 1).mean())


def test_sampler_raw_within_product_and_sum_rounding(gpu):
    """Raw output: |got - ref| <= 1e-6 * sum_taps |w v| (16 ulp of the
    four-term sum; four products and three adds can lose 8).

    The kernels take the source index ((gx + 1) * w - 1) / 2 in fp64, so the
    only float32 roundings are those of the two weights per axis, the four
    products and the sum: at most 4 ulp of the bound's 16.  (With the index
    in float32, ATen's form, its rounding of up to 3.2 w 2^-24 px alone moved
    the output by 2 to 50 times this bound at these sizes.)"""
    bad = []
    for c, h, w in RAW_CASES:
        err, bound = _raw_errors(gpu, c, h, w)
        worst, over = _worst(err, bound)
        print("C=%d %dx%d raw: max err %.3e, %.3g of 1e-6 sum|w v| (%.2f %% of outputs above)"
              % (c, h, w, err.max(), worst, 100 * over))
        if worst > 1:
            bad.append((c, worst))
    assert not bad, bad


@pytest.mark.parametrize("c,h,w", SAMPLE_CASES)
def test_generic_sampler_normalised(gpu, c, h, w):
    """sample_desc_kernel<1, 2, 4, 16> + L2 norm at atol 1e-5 (values in
    [-1, 1]; the norm's reduction at C = 1024 loses about 22 ulp, 1.3e-6
    relative), packed and padded storage, and through the drop-in
    sample_feat_by_coord.  Zero-norm rows are exact zeros: no 0 * 1e12."""
    from posfeat_amd.losses import preprocess_utils
    x, coord = sample_inputs(c, h, w)
    ref = detect_ref.sample_feat_by_coord(x, coord, norm=True)
    got = {cs: _sample(gpu, x, coord, cs, True) for cs in (c, c + 3)}
    got["drop-in"] = preprocess_utils.sample_feat_by_coord(
        torch.from_numpy(x).to(gpu), torch.from_numpy(coord).to(gpu), norm=True).cpu().numpy()
    for k, g in got.items():
        assert np.isfinite(g).all(), k
        err = np.abs(g - ref).max()
        print("C=%d %s normalised: max err %.3e (%.3f of 1e-5)" % (c, k, err, err / 1e-5))
        assert err <= 1e-5, k
        for row in ZERO_ROWS:
            assert not g[:, row].any(), (k, row)
    np.testing.assert_array_equal(got[c], got[c + 3])
    np.testing.assert_array_equal(got[c], got["drop-in"])
    raw = _sample(gpu, x, coord, c + 3, False)
    for row in ZERO_ROWS:
        assert not raw[:, row].any(), row


def test_c128_generic_kernel_equals_half_wave_kernel(gpu):
    """C = 128 through sample_desc_kernel<2>, forced by cstride % 4 != 0, by a
    map pointer off 16 B and by an out pointer off 16 B.  Unnormalised, all
    three equal sample_desc128_kernel's output bit for bit (sample.hip: each
    channel's bilinear sum runs in the same order in both kernels);
    normalised, the sums of squares are grouped differently and both stay
    within 1e-5 of the oracle."""
    from posfeat_amd import ops
    from posfeat_amd._lib import lib, ptr, stream_ptr, check
    b, c, h, w = 2, 128, 6, 7
    x, coord = sample_inputs(c, h, w)
    npts = coord.shape[1]
    cd = torch.from_numpy(coord).to(gpu)
    for normalize in (False, True):
        base = _sample(gpu, x, coord, 128, normalize)            # the half-wave kernel
        got = {"cstride130": _sample(gpu, x, coord, 130, normalize)}
        store = torch.full((1 + b * h * w * 132,), float(PAD), device=gpu)
        store[1:].view(b, h, w, 132)[..., :c] = torch.from_numpy(x).to(gpu).permute(0, 2, 3, 1)
        assert store.data_ptr() % 16 == 0
        got["map+4B"] = ops.sample_desc_strided(store.data_ptr() + 4, b, c, h, w, 132, cd,
                                                normalize=normalize).cpu().numpy()
        fmap = torch.from_numpy(_nhwc(x, 128)).to(gpu)
        obuf = torch.full((1 + b * npts * c,), float("nan"), device=gpu)
        assert fmap.data_ptr() % 16 == 0 and obuf.data_ptr() % 16 == 0
        check(lib().posfeat_sample_desc(ptr(fmap), b, c, h, w, 128, ptr(cd), npts, None,
                                        1 if normalize else 0,
                                        ctypes.c_void_p(obuf.data_ptr() + 4), stream_ptr()))
        got["out+4B"] = obuf[1:].view(b, npts, c).cpu().numpy()
        assert np.isnan(obuf[0].item())
        ref = detect_ref.sample_feat_by_coord(x, coord, norm=normalize)
        for k, g in got.items():
            assert np.isfinite(g).all(), k
            if normalize:
                assert np.abs(g - ref).max() <= 1e-5 and np.abs(base - ref).max() <= 1e-5, k
            else:
                np.testing.assert_array_equal(g, base, err_msg=k)


def _edge_coords(c, h, w, b, npts):
    _, coord = sample_inputs(c, h, w, b)
    # npts = 1: an ordinary point; otherwise the border points lead
    return np.ascontiguousarray(coord[:, 6:7] if npts == 1 else coord[:, :npts])


@pytest.mark.parametrize("b,npts", [(1, 33), (3, 5), (2, 1), (1, 1)])
def test_sampler128_odd_row_counts(gpu, b, npts):
    """b * npts odd: the last wave of sample_desc128_kernel has a dead half
    (its 32 lanes return before the shuffles)."""
    c, h, w = 128, 5, 8
    x = np.random.RandomState(b * 100 + npts).randn(b, c, h, w).astype(np.float32)
    coord = _edge_coords(c, h, w, b, npts)
    for normalize in (True, False):
        got = _sample(gpu, x, coord, 128, normalize)
        assert got.shape == (b, npts, c) and np.isfinite(got).all()
        if normalize:
            ref = detect_ref.sample_feat_by_coord(x, coord, norm=True)
            assert np.abs(got - ref).max() <= 1e-5
        else:  # w = 8: the border points' indices are exact; the general raw bounds are above
            np.testing.assert_array_equal(got, _sample(gpu, x, coord, 130, False))
        if npts >= 5:
            for row in ZERO_ROWS[:npts - 2]:  # one pitch outside, far outside: exact zeros
                assert not got[:, row].any(), row


@pytest.mark.parametrize("c,cs", [(128, 128), (128, 130), (100, 100)])
def test_sampler_n_valid(gpu, c, cs):
    """Rows past n_valid are exact zeros, rows before it are what the call
    without n_valid gives: one count for the batch, and one per image."""
    b, h, w, npts = 3, 5, 8, 7
    x = np.random.RandomState(c + cs).randn(b, c, h, w).astype(np.float32)
    coord = _edge_coords(c, h, w, b, npts)
    for normalize in (True, False):
        full = _sample(gpu, x, coord, cs, normalize)
        for k in (0, 1, npts - 1, npts):
            nv = torch.tensor([k], dtype=torch.int32, device=gpu)
            got = _sample(gpu, x, coord, cs, normalize, n_valid=nv)
            np.testing.assert_array_equal(got[:, :k], full[:, :k])
            assert not got[:, k:].any() and np.isfinite(got).all()
        for per in ([0, npts, 2], [npts - 1, 1, 0]):
            nv = torch.tensor(per, dtype=torch.int32, device=gpu)
            got = _sample(gpu, x, coord, cs, normalize, n_valid=nv, each=True)
            for i, k in enumerate(per):
                np.testing.assert_array_equal(got[i, :k], full[i, :k])
                assert not got[i, k:].any()


def test_sampler_argument_checks(gpu):
    from posfeat_amd import ops
    coord = torch.zeros(1, 4, 2, device=gpu)
    with pytest.raises(RuntimeError):          # no instantiation above 64 * 16 channels
        ops.sample_desc_nhwc(torch.zeros(1, 2, 2, 1025, device=gpu), coord)
    with pytest.raises(RuntimeError):          # cstride < C
        ops.sample_desc_nhwc(torch.zeros(1, 2, 2, 64, device=gpu), coord, c=100)
    for c in (128, 100):                       # no rows: nothing launched, an empty result
        out = ops.sample_desc_nhwc(torch.zeros(2, 3, 4, c, device=gpu),
                                   torch.zeros(2, 0, 2, device=gpu))
        assert out.shape == (2, 0, c)
        out = ops.sample_desc_nhwc(torch.zeros(2, 3, 4, c, device=gpu),
                                   torch.zeros(2, 0, 2, device=gpu),
                                   n_valid=torch.zeros(2, dtype=torch.int32, device=gpu), each=True)
        assert out.shape == (2, 0, c)
    torch.cuda.synchronize()
