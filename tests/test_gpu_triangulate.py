"""posfeat_triangulate on the GPU against the numpy restatement of its
definitions (tests/triangulate_ref.py): one planted scene
(tests/triangulate_fixture.py), one call, shuffled edges.  Ten sets: nine
cameras 0.45 apart on a line (K = 500 / 320 / 240, every second one
SIMPLE_RADIAL with k1 = -0.06) and a tenth 0.002 from the first; one set has
2049 rows, so N crosses the scan's block boundary.  iters = 64, thr = 4,
min_angle = 1.5, max_track = 64.  The preconditions -- no reprojection error of
a scored hypothesis or refit within 1e-6 px of thr, no depth within 1e-9 of 0,
no tested cosine within 1e-9 of cos(min_angle), the refit matrix's second
smallest / largest eigenvalue >= 1e-4 on every kept track -- are asserted on
the restatement before the device result is looked at, so the integer outputs
are compared exactly and the points to 1e-9: fp64 eps over the 1e-4 gap is
about 2e-12, which leaves three orders of margin for the order of the Jacobi
rotations' arithmetic.  ``err`` is held to 1e-9 relative where it is at least
0.1 px (the tracks with real noise) and to 1e-9 px absolutely below that: the
reprojection error of an exact track is the fp32 rounding of its keypoints,
about 1e-5 px, a difference of pixel coordinates of size 300, so a relative
change of 1e-13 in the point is already 1e-8 of that error.  Measured on an
MI355X: points 2.5e-14 relative, err 6.4e-14 px absolute (1.35e-8 of itself on
an exact track).

max_track = 64 keeps no track longer than a wave's 64 lanes, so two more calls
on the same scene cover what the first cannot: one with max_track = 160 on the
edges of a 140-row component (several passes of every lane-strided loop of the
wave kernel), one with iters = 8 (the sampler path of the lane kernel, at 5 and
6 members).  Both are compared with the restatement under the same
preconditions."""
import numpy as np
import pytest
import torch

import triangulate_fixture as fx
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

EXACT = ("counts", "track_off", "track_rows", "obs_inlier", "tinfo", "point_of_row")


def _run(f, edges, **kw):
    from posfeat_amd import geometry
    dev = torch.device("cuda:0")
    args = dict(iters=fx.ITERS, thr=fx.THR, min_angle=fx.MIN_ANGLE, max_track=fx.MAX_TRACK,
                seed=fx.SEED)
    args.update(kw)
    res = geometry.triangulate_tracks(
        torch.from_numpy(f["kp"]).to(dev), f["set_off"], torch.from_numpy(f["cams"]).to(dev),
        torch.from_numpy(f["poses"]).to(dev),
        torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)).to(dev), **args)
    return res.host()


@pytest.fixture(scope="module")
def scene():
    f = fx.build(fx.FIXTURE_SEED)
    ref = tr.triangulate(f["kp"], f["set_off"], f["cams"], f["poses"], f["edges"], fx.ITERS, fx.THR,
                         fx.MIN_ANGLE, fx.MAX_TRACK, fx.SEED)
    got = _run(f, f["edges"])
    return f, ref, got


def _track_of(res, rows):
    root = {int(res["track_rows"][res["track_off"][t]]): t for t in range(int(res["counts"][0]))}
    return root.get(min(rows))


def test_fixture_preconditions(scene):
    f, ref, _ = scene
    mg = ref["margins"]
    print("margins", mg, "eig ratio min", np.nanmin(ref["eig_ratio"]))
    assert mg["err"] > 1e-6 and mg["depth"] > 1e-9 and mg["cos"] > 1e-9
    kept = ref["tinfo"][:, 3] == 1
    assert kept.sum() >= 30 and np.all(ref["eig_ratio"][kept] >= 1e-4)
    # the cases are what they are meant to be
    c = f["cases"]
    for case in c["two_view"] + c["chain8"] + c["noisy"]:
        t = _track_of(ref, case["rows"])
        assert ref["tinfo"][t, 0] == 0 and ref["tinfo"][t, 1] == len(case["rows"])
    t = _track_of(ref, c["outlier"][0]["rows"])
    flags = ref["obs_inlier"][ref["track_off"][t]:ref["track_off"][t + 1]]
    rows = ref["track_rows"][ref["track_off"][t]:ref["track_off"][t + 1]]
    assert flags.sum() == 4 and rows[flags == 0][0] == c["outlier"][0]["rows"][2]
    t = _track_of(ref, c["merge5"][0]["rows"] + c["merge3"][0]["rows"])
    rows = ref["track_rows"][ref["track_off"][t]:ref["track_off"][t + 1]]
    flags = ref["obs_inlier"][ref["track_off"][t]:ref["track_off"][t + 1]]
    assert len(rows) == 8 and set(rows[flags == 1]) == set(c["merge5"][0]["rows"])
    for name in ("low_parallax", "behind"):
        t = _track_of(ref, c[name][0]["rows"])
        assert tuple(ref["tinfo"][t]) == (1, 0, -1, 0)
    full = c["full"][0]
    t = _track_of(ref, full["comp"])
    assert ref["track_off"][t + 1] - ref["track_off"][t] == fx.MAX_TRACK   # one wave's lanes exactly
    assert ref["tinfo"][t, 1] == 8 and fx.MAX_TRACK * (fx.MAX_TRACK - 1) // 2 > fx.ITERS
    assert _track_of(ref, c["oversized"][0]["comp"]) is None and ref["counts"][4] == 1
    assert ref["counts"][5] == f["n_invalid"]
    assert (ref["point_of_row"] < 0).sum() > 2049            # isolated rows


def test_integer_outputs_exact(scene):
    _, ref, got = scene
    for k in EXACT:
        assert np.array_equal(got[k], ref[k]), k


def _check_preconditions(ref):
    mg = ref["margins"]
    print("margins", mg, "eig ratio min", np.nanmin(ref["eig_ratio"]))
    assert mg["err"] > 1e-6 and mg["depth"] > 1e-9 and mg["cos"] > 1e-9
    kept = ref["tinfo"][:, 3] == 1
    assert np.all(ref["eig_ratio"][kept] >= 1e-4)


def _compare(ref, got):
    for k in EXACT:
        assert np.array_equal(got[k], ref[k]), k
    _compare_points(ref, got)


def test_track_longer_than_a_wave(scene):
    """a kept component of 140 rows: sampler path, 64 hypotheses, and three
    passes of the wave kernel's lane-strided loops over the members"""
    f, _, _ = scene
    ref = tr.triangulate(f["kp"], f["set_off"], f["cams"], f["poses"], f["long_edges"], fx.ITERS,
                         fx.THR, fx.MIN_ANGLE, fx.LONG_MAX_TRACK, fx.LONG_SEED)
    _check_preconditions(ref)
    case = f["cases"]["long"][0]
    t = _track_of(ref, case["comp"])
    sl = slice(int(ref["track_off"][t]), int(ref["track_off"][t + 1]))
    assert sl.stop - sl.start == fx.LONG_ROWS > 2 * 64
    assert tuple(ref["tinfo"][t, [0, 1, 3]]) == (0, 9, 1)      # the real 9-view track is found
    assert set(ref["track_rows"][sl][ref["obs_inlier"][sl] == 1]) == set(case["rows"])
    assert np.abs(ref["points"][t] - case["X"]).max() <= 2.2e-6 * np.abs(case["X"]).max()
    assert ref["counts"][0] == 16 and ref["counts"][4] == 0    # and the 15 noisy tracks
    got = _run(f, f["long_edges"], max_track=fx.LONG_MAX_TRACK, seed=fx.LONG_SEED)
    _compare(ref, got)


def test_lane_kernel_sampler_path(scene):
    """iters = 8: tracks of 5 and 6 members (10 and 15 pairs) draw their pairs
    from the sampler inside the lane kernel"""
    f, _, _ = scene
    ref = tr.triangulate(f["kp"], f["set_off"], f["cams"], f["poses"], f["edges"], 8, fx.THR,
                         fx.MIN_ANGLE, fx.MAX_TRACK, fx.SEED)
    _check_preconditions(ref)
    sizes = np.diff(ref["track_off"])
    assert ((sizes == 5) | (sizes == 6)).sum() >= 4
    got = _run(f, f["edges"], iters=8)
    _compare(ref, got)


def test_points_and_errors(scene):
    _, ref, got = scene
    _compare_points(ref, got)


def _compare_points(ref, got):
    scale = np.abs(ref["points"]).max(1)
    ok = ref["tinfo"][:, 0] == 0
    dp = np.abs(got["points"] - ref["points"]).max(1)
    de = np.abs(got["err"] - ref["err"])
    print("max relative point difference %.3g, max err difference %.3g px (rel %.3g)"
          % ((dp[ok] / scale[ok]).max(), de.max(),
             (de[ok] / np.maximum(ref["err"][ok], 1e-300)).max()))
    assert np.all(dp[ok] <= 1e-9 * scale[ok])
    assert np.all(got["points"][~ok] == 0.0) and np.all(got["err"][~ok] == 0.0)
    # relative where the error is real noise; the error of an exact track is
    # the fp32 rounding of its pixels (~1e-5 px), a difference of nearly equal
    # numbers: absolute there
    noisy = ok & (ref["err"] >= 0.1)
    assert np.all(de[noisy] <= 1e-9 * ref["err"][noisy])
    assert np.all(de[ok & ~noisy] <= 1e-9)


def test_planted_points_recovered(scene):
    f, ref, got = scene
    worst_ref, worst_got = 0.0, 0.0
    for name in ("two_view", "chain8", "outlier", "merge5", "full"):
        for case in f["cases"][name]:
            t = _track_of(ref, case.get("comp", case["rows"]))
            s = np.abs(case["X"]).max()
            worst_ref = max(worst_ref, np.abs(ref["points"][t] - case["X"]).max() / s)
            worst_got = max(worst_got, np.abs(got["points"][t] - case["X"]).max() / s)
    print("relative error against ground truth: restatement %.3g, device %.3g"
          % (worst_ref, worst_got))
    assert worst_ref < 1e-5                                   # fp32 pixels, depths 3..9
    assert worst_got <= 2.0 * worst_ref


def test_edge_order_does_not_matter(scene):
    f, _, got = scene
    perm = np.random.RandomState(5).permutation(len(f["edges"]))
    again = _run(f, f["edges"][perm][:, ::-1])
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
        assert got[k].tobytes() == again[k].tobytes(), k


def test_other_components_do_not_matter(scene):
    f, _, got = scene
    free = np.flatnonzero(got["point_of_row"] < 0)
    used = set(got["track_rows"].tolist())
    free = np.array([r for r in free if r not in used])
    sid = tr.set_of_rows(f["set_off"])
    rs = np.random.RandomState(9)
    extra = []
    for _ in range(40):
        a, b = rs.choice(free, 2, replace=False)
        if sid[a] != sid[b]:
            extra.append((a, b))
    more = _run(f, np.concatenate([f["edges"], np.asarray(extra, np.int32)]))
    assert more["counts"][0] > got["counts"][0]
    for t in range(int(got["counts"][0])):
        rows = got["track_rows"][got["track_off"][t]:got["track_off"][t + 1]]
        u = _track_of(more, rows)
        mrows = more["track_rows"][more["track_off"][u]:more["track_off"][u + 1]]
        assert np.array_equal(rows, mrows)
        assert got["points"][t].tobytes() == more["points"][u].tobytes()
        assert got["err"][t].tobytes() == more["err"][u].tobytes()
        assert np.array_equal(got["tinfo"][t], more["tinfo"][u])
        assert np.array_equal(got["obs_inlier"][got["track_off"][t]:got["track_off"][t + 1]],
                              more["obs_inlier"][more["track_off"][u]:more["track_off"][u + 1]])


def test_no_edges(scene):
    f, _, _ = scene
    got = _run(f, np.zeros((0, 2), np.int32))
    assert np.all(got["counts"] == 0) and got["points"].shape == (0, 3)
    assert np.array_equal(got["track_off"], [0]) and np.all(got["point_of_row"] == -1)


def test_track_edges_matches_host_construction():
    from posfeat_amd import geometry, matchers
    dev = torch.device("cuda:0")
    set_off = np.asarray([0, 5, 9, 12], np.int32)
    pairs = np.asarray([[0, 1], [2, 0], [1, 2]], np.int32)
    n1 = [5, 3, 4]
    moff = np.concatenate([[0], np.cumsum(n1)])
    counts = np.asarray([3, 0, 4], np.int32)
    matches = np.full((12, 2), -1, np.int32)
    matches[0:3] = [[0, 1], [2, 3], [4, 0]]
    matches[8:12] = [[0, 2], [1, 1], [2, 0], [3, 2]]
    matches[4] = [1, 1]                                      # past counts[0]: not a match
    inlier = np.zeros(12, np.uint8)
    inlier[[0, 2, 4, 8, 9, 11]] = 1
    buf = torch.from_numpy(np.concatenate([counts, matches.reshape(-1)])).to(dev)
    batch = matchers.PairBatch(None, set_off, pairs, moff, buf)
    got = geometry.track_edges(batch, torch.from_numpy(inlier).to(dev)).cpu().numpy()
    want = np.full((12, 2), -1, np.int32)
    for p, (s1, s2) in enumerate(pairs):
        for i in range(counts[p]):
            r = moff[p] + i
            if inlier[r]:
                want[r] = (set_off[s1] + matches[r, 0], set_off[s2] + matches[r, 1])
    assert got.dtype == np.int32 and np.array_equal(got, want)
    assert (want >= 0).all(1).sum() == 5
