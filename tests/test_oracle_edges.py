"""The numpy oracle (oracle/detect_ref.py) against torch on the CPU in fp64, at
the inputs of tests/test_gpu_detect_sample_edges.py: signed maps with many
ties, odd and tiny sizes, every channel count the generic sampler serves,
points on and beyond the border.  The GPU tests rely on the oracle there, so it
is pinned here first.  The input builders at the top are shared with the GPU
file (one definition of every map and coordinate set).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import detect_ref

# ------------------------------------------------------------------ shared inputs
NMS_SIZES = [(35, 51), (8, 16), (3, 65), (1, 9), (9, 1)]
SAMPLE_CASES = [(3, 7, 9), (64, 5, 6), (100, 9, 11), (130, 6, 7), (256, 4, 5), (1024, 3, 4)]
SAMPLE_NPTS = 33
# (h, w, thr) of the thr_mod="mean" detector cases; the map's seed is 77 + h
MEAN_CASES = [(37, 53, 1.2), (64, 96, 1.5), (120, 160, 1.0)]
MEAN_MARGIN_ULP = 32


def nms_radii(h, w):
    """0, 1, 2, 3 and the reflect limit min(h, w) - 1, where r < h and r < w."""
    return sorted(r for r in {0, 1, 2, 3, min(h, w) - 1} if r < h and r < w)


def quantised_map(h, w, seed=0):
    """Five levels in {-2/3 .. 2/3}: negatives and ties in every window."""
    rs = np.random.RandomState(1000 * h + w + seed)
    return ((rs.randint(0, 5, (h, w)) - 2) / 3.0).astype(np.float32)


def sample_inputs(c, h, w, b=2):
    """(x [b,c,h,w] randn, coord [b,33,2]) -- uniform(-1.2, 1.2) points, the
    first six of every image on the border cases: the two corner pixels' outer
    corners, one pixel pitch outside left and right (ix = -1 and ix = w: no
    tap inside), far outside, and one pitch below the map.  1 + 1/w is
    rounded away from the map where float32 cannot hold it (the nearest
    float32 may lie a hair inside the pitch, where one tap still has a weight
    of 1e-7).  Rows ZERO_ROWS have no tap inside: exact zeros."""
    rs = np.random.RandomState(100 * c + 10 * h + w)
    x = rs.randn(b, c, h, w).astype(np.float32)
    coord = rs.uniform(-1.2, 1.2, (b, SAMPLE_NPTS, 2)).astype(np.float32)

    def pitch_outside(n):
        v = np.float32(1 + 1.0 / n)
        return v if float(v) >= 1 + 1.0 / n else np.nextafter(v, np.float32(2))
    ox, oy = pitch_outside(w), pitch_outside(h)
    coord[:, :6] = np.array([(-1, -1), (1, 1), (-ox, 0), (ox, 0), (-3, -3), (0, oy)], np.float32)
    return x, coord


ZERO_ROWS = (2, 3, 4, 5)


def mean_map(h, w):
    km = np.random.RandomState(77 + h).rand(3, 1, h, w).astype(np.float32)
    km[1] *= np.float32(0.37)  # a second threshold: the per-image mean must be per image
    return km


def ulp_distance(a, b):
    """Number of float32 values between a and b (elementwise, +0 == -0)."""
    return np.abs(detect_ref._float_key(np.asarray(a, np.float32)).astype(np.int64) -
                  detect_ref._float_key(np.asarray(b, np.float32)).astype(np.int64))


# ------------------------------------------------------------------ nms
def _aten_nms(score, r):
    """preprocess_utils.nms of the reference: reflect pad, max_pool2d with
    indices (ATen keeps the first maximum of a window), idx == own position."""
    h, w = score.shape
    s = torch.from_numpy(score)[None, None]
    p = F.pad(s, [r, r, r, r], mode="reflect") if r else s
    _, idx = F.max_pool2d(p, kernel_size=2 * r + 1, stride=1, return_indices=True)
    ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    own = (ii + r) * (w + 2 * r) + (jj + r)
    return (idx[0, 0] == own).numpy()


@pytest.mark.parametrize("h,w", NMS_SIZES)
def test_nms_is_aten_first_occurrence(h, w):
    score = quantised_map(h, w)
    assert (score < 0).any() and len(np.unique(score)) <= 5
    for r in nms_radii(h, w):
        got = detect_ref.nms(score, r)
        np.testing.assert_array_equal(got, _aten_nms(score, r), err_msg="r=%d" % r)
        if r == 0:
            assert got.all()


# ------------------------------------------------------------------ sampler
@pytest.mark.parametrize("c,h,w", SAMPLE_CASES)
def test_sample_feat_by_coord_is_grid_sample_fp64(c, h, w):
    x, coord = sample_inputs(c, h, w)
    ref = F.grid_sample(torch.from_numpy(x).double(), torch.from_numpy(coord).double()[:, :, None],
                        mode="bilinear", padding_mode="zeros", align_corners=False)
    ref = ref[..., 0].permute(0, 2, 1).numpy()  # [b, n, c]
    got = detect_ref.sample_feat_by_coord(x, coord, norm=False)
    assert got.dtype == np.float32
    # the oracle returns float32: half an ulp below 4 is 1.2e-7
    assert np.abs(ref).max() < 4.0
    err = np.abs(got.astype(np.float64) - ref).max()
    print("C=%d raw err %.3e" % (c, err))
    assert err <= 2e-7
    refn = F.normalize(torch.from_numpy(ref), p=2, dim=2, eps=1e-12).numpy()
    gotn = detect_ref.sample_feat_by_coord(x, coord, norm=True)
    assert np.abs(gotn.astype(np.float64) - refn).max() <= 2e-7
    # one pitch outside and far outside: no tap inside the map, exact zero
    # rows either way (norm 0, the 1e-12 clamp)
    for k in ZERO_ROWS:
        assert not got[:, k].any() and not gotn[:, k].any(), k


# ------------------------------------------------------------------ refine
@pytest.mark.parametrize("h,w", [(37, 53), (10, 18)])
def test_refine_maps_is_avgpool_quotient_fp64(h, w):
    km = np.random.RandomState(h).rand(h, w).astype(np.float32)
    kp = torch.from_numpy(km).double()[None, None]
    grid = torch.from_numpy(detect_ref.gen_grid(-1, 1, -1, 1, h, w)).double()
    grid = grid.reshape(1, h, w, 2).permute(0, 3, 1, 2)
    ref = F.avg_pool2d(kp * grid, 3, stride=1) / F.avg_pool2d(kp, 3, stride=1)
    rx, ry = detect_ref.refine_maps(km)
    assert rx.shape == (h - 2, w - 2)
    assert np.abs(rx - ref[0, 0].numpy()).max() <= 1e-6
    assert np.abs(ry - ref[0, 1].numpy()).max() <= 1e-6


# ------------------------------------------------------------------ 'mean' inputs
@pytest.mark.parametrize("h,w,thr", MEAN_CASES)
def test_mean_threshold_inputs_clear_the_margin(h, w, thr):
    """A condition on the inputs of the GPU 'mean' tests, not a tolerance: the
    float32 threshold t = thr * mean depends on how the mean is summed (the
    oracle: numpy's float32 pairwise mean; the device: an fp64 sum), so a
    bit-exact mask needs every inner score well clear of t.  A seed that
    fails this is replaced, the margin stays."""
    km = mean_map(h, w)
    inner = km[:, 0, 1:-1, 1:-1].reshape(3, -1)
    t32 = (np.float32(thr) * inner.mean(1, dtype=np.float32)).astype(np.float32)
    t64 = (np.float32(thr) * (inner.astype(np.float64).sum(1) / inner.shape[1])
           .astype(np.float32)).astype(np.float32)
    gap = ulp_distance(inner, t32[:, None]).min(1)
    print("%dx%d thr %.1f: t32 - t64 %s ulp, nearest score %s ulp"
          % (h, w, thr, ulp_distance(t32, t64).tolist(), gap.tolist()))
    assert (gap > MEAN_MARGIN_ULP).all()
    # the two ways of taking the mean stay inside that margin
    assert (ulp_distance(t32, t64) < MEAN_MARGIN_ULP).all()
    # the threshold bites (it removes NMS survivors), and differently per image
    counts = detect_ref.detector_count(km, 1, True, thr, "mean")
    assert len(set(counts.tolist())) > 1 and (counts > 0).all()
    assert (counts < detect_ref.detector_count(km, 1, True)).all()
