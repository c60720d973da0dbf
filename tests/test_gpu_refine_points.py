"""posfeat_refine_points on the GPU against the numpy restatement of its
definitions (tests/refine_ref.py), on two sources of input.

1. The planted scene of the triangulation tests (tests/triangulate_fixture.py)
   through geometry.triangulate_tracks and then geometry.refine_tracks: the
   first call (max_track = 64, with the component of exactly 64 rows) and the
   LONG_MAX_TRACK call (a 140-row component: three passes of the wave kernel's
   lane-strided loops).  The restatement runs on what the triangulate call left
   (read back), so only the refinement is compared.
2. A track table written by hand (tests/refine_fixture.py) over 33 cameras at
   distances 2..40 with focal lengths 400..1600: the cases no triangulate call
   produces, and tracks of 2, 16, 17, 64, 65 and 130 members; also with rounds =
   1 and with steps = 1.

The margins are asserted on the restatement first: no squared error of a test
within 1e-6 thr^2 of thr^2, no tested cosine within 1e-9 of cos(min_angle).
Statuses, flags, inlier counts, rounds used, point_of_row and counts are then
compared exactly, the points to 1e-9 of their largest coordinate (fp64 eps times
the condition number of the normal matrix, as for posfeat_refine_point), err by
the rule of the triangulate test (1e-9 relative from 0.1 px, 1e-9 px below).
The number of taken steps is not compared exactly: close to convergence
"strictly lower" is decided by rounding.  Measured on an MI355X: points
identical to the restatement on every call, err within 4.4e-14 px, and the
taken-step counts equal as well."""
import numpy as np
import pytest
import torch

import refine_fixture as rf
import refine_ref as rr
import triangulate_fixture as fx

pytestmark = pytest.mark.gpu

EXACT = ("counts", "track_off", "track_rows", "obs_inlier", "tinfo", "point_of_row")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _refine(f, tracks, **kw):
    from posfeat_amd import geometry
    args = dict(thr=rf.THR, min_angle=rf.MIN_ANGLE, rounds=rf.ROUNDS, steps=rf.STEPS)
    args.update(kw)
    got = geometry.refine_tracks(_dev(f["kp"]), f["set_off"], _dev(f["cams"]), _dev(f["poses"]),
                                 tracks, **args).host()
    un = got.pop("unrefined")                                  # the input's err, tinfo, counts
    assert np.array_equal(un["counts"], tracks.counts.cpu().numpy())
    return got


def _table_tracks(f):
    """the hand-built table as the TrackResult a triangulate call would leave"""
    from posfeat_amd import geometry
    t = f["tracks"]
    N = int(f["set_off"][-1])
    return geometry.TrackResult(
        points=_dev(t["points"]), err=torch.zeros(len(t["points"]), dtype=torch.float64,
                                                  device="cuda:0"),
        tinfo=_dev(t["tinfo"]), track_off=_dev(t["track_off"]), track_rows=_dev(t["track_rows"]),
        obs_inlier=_dev(t["obs_inlier"]), counts=_dev(t["counts"]),
        point_of_row=torch.full((N,), -1, dtype=torch.int32, device="cuda:0"))


def _compare(ref, got, steps, rounds):
    mg = ref["margins"]
    print("margins", mg)
    assert mg["err2"] > 1e-6 and mg["cos"] > 1e-9
    for k in EXACT:
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["rinfo"][:, [0, 2, 3]], ref["rinfo"][:, [0, 2, 3]])
    assert np.all(got["rinfo"][:, 1] >= 0) and np.all(got["rinfo"][:, 1] <= steps * got["rinfo"][:, 0])
    assert np.all(got["rinfo"][:, 0] <= rounds)
    ok = ref["tinfo"][:, 0] == 0
    scale = np.abs(ref["points"]).max(1)
    dp = np.abs(got["points"] - ref["points"]).max(1)
    de = np.abs(got["err"] - ref["err"])
    print("max relative point difference %.3g, max err difference %.3g px, steps differ on %d tracks"
          % ((dp[ok] / scale[ok]).max(), de.max(), (got["rinfo"][:, 1] != ref["rinfo"][:, 1]).sum()))
    assert np.all(dp[ok] <= 1e-9 * scale[ok])
    assert np.all(got["points"][~ok] == 0.0) and np.all(got["err"][~ok] == 0.0)
    noisy = ok & (ref["err"] >= 0.1)
    assert np.all(de[noisy] <= 1e-9 * ref["err"][noisy])
    assert np.all(de[ok & ~noisy] <= 1e-9)


def _cost(sc, rows, X):
    return float(sum(sc.reproj2(r, X)[0] for r in rows))


def _cost_does_not_rise(f, tracks, got):
    """the cost over the final set at the output point against the input point.
    Both are evaluated here, not where the steps were accepted: a residual is a
    difference of pixel coordinates of size up to 2000 that two evaluations
    give to about 1e-12 px, so a cost c over n rows is known to 2 sqrt(2 n c)
    1e-12, which is the slack"""
    import triangulate_ref as tr
    sc = tr.Scene(f["kp"], f["set_off"], f["cams"], f["poses"])
    for t in np.flatnonzero(got["tinfo"][:, 0] == 0):
        sl = slice(int(got["track_off"][t]), int(got["track_off"][t + 1]))
        rows = got["track_rows"][sl][got["obs_inlier"][sl] != 0]
        c0, c1 = _cost(sc, rows, tracks["points"][t]), _cost(sc, rows, got["points"][t])
        assert c1 <= c0 + 2.0 * np.sqrt(2.0 * len(rows) * c0) * 1e-12, (t, c0, c1)


@pytest.fixture(scope="module")
def table():
    f = rf.build_table()
    ref = rr.refine(f["kp"], f["set_off"], f["cams"], f["poses"], f["tracks"], rf.THR, rf.MIN_ANGLE,
                    rf.ROUNDS, rf.STEPS)
    got = _refine(f, _table_tracks(f))
    return f, ref, got


def test_hand_built_table(table):
    f, ref, got = table
    _compare(ref, got, rf.STEPS, rf.ROUNDS)
    _cost_does_not_rise(f, f["tracks"], got)
    c = {k: v[0]["t"] for k, v in f["cases"].items()}
    assert tuple(ref["rinfo"][c["outlier"], [0, 3]]) == (2, 1) and ref["tinfo"][c["outlier"], 1] == 13
    assert tuple(ref["tinfo"][[c["one_inlier"], c["low_parallax"], c["status1"], c["nan_point"]], 0]) \
        == (2, 3, 1, 2)
    sizes = np.diff(ref["track_off"])
    assert {2, rf.LANE_TRACK, rf.LANE_TRACK + 1, 64, 65, 130} <= set(sizes.tolist())
    assert ref["counts"][3] >= 3 and ref["counts"][4] >= 2 and ref["counts"][5] == 1


@pytest.mark.parametrize("rounds,steps", [(1, rf.STEPS), (rf.ROUNDS, 1)])
def test_extremes_on_the_table(table, rounds, steps):
    f, _, _ = table
    ref = rr.refine(f["kp"], f["set_off"], f["cams"], f["poses"], f["tracks"], rf.THR, rf.MIN_ANGLE,
                    rounds, steps)
    got = _refine(f, _table_tracks(f), rounds=rounds, steps=steps)
    _compare(ref, got, steps, rounds)


def test_twice_and_with_unrelated_tracks(table):
    f, _, got = table
    again = _refine(f, _table_tracks(f))
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    g = rf.build_table(extra_tracks=25)
    T, M = int(got["counts"][0]), len(got["track_rows"])
    assert np.array_equal(g["tracks"]["track_rows"][:M], f["tracks"]["track_rows"])
    more = _refine(g, _table_tracks(g))
    assert more["counts"][0] == T + 25
    for k in ("points", "err", "tinfo", "rinfo"):
        assert more[k][:T].tobytes() == got[k].tobytes(), k
    assert more["obs_inlier"][:M].tobytes() == got["obs_inlier"].tobytes()
    rows = got["track_rows"][got["track_rows"] < len(got["point_of_row"])]
    assert np.array_equal(more["point_of_row"][rows], got["point_of_row"][rows])


@pytest.mark.parametrize("which", ["main", "long"])
def test_existing_scene(which):
    from posfeat_amd import geometry
    f = fx.build(fx.FIXTURE_SEED)
    edges, mt, seed = ((f["edges"], fx.MAX_TRACK, fx.SEED) if which == "main" else
                       (f["long_edges"], fx.LONG_MAX_TRACK, fx.LONG_SEED))
    tri = geometry.triangulate_tracks(_dev(f["kp"]), f["set_off"], _dev(f["cams"]), _dev(f["poses"]),
                                      _dev(edges.astype(np.int32).reshape(-1, 2)), iters=fx.ITERS,
                                      thr=fx.THR, min_angle=fx.MIN_ANGLE, max_track=mt, seed=seed)
    before = tri.host()
    res = geometry.refine_tracks(_dev(f["kp"]), f["set_off"], _dev(f["cams"]), _dev(f["poses"]), tri,
                                 thr=fx.THR, min_angle=fx.MIN_ANGLE, rounds=rf.ROUNDS,
                                 steps=rf.STEPS)
    assert res.track_off is tri.track_off and res.track_rows is tri.track_rows
    got = res.host()
    un = got.pop("unrefined")
    assert np.array_equal(un["tinfo"], before["tinfo"]) and np.array_equal(un["err"], before["err"])
    after = tri.host()
    for k in before:                                           # the inputs are not written
        assert before[k].tobytes() == after[k].tobytes(), k
    ref = rr.refine(f["kp"], f["set_off"], f["cams"], f["poses"], before, fx.THR, fx.MIN_ANGLE,
                    rf.ROUNDS, rf.STEPS)
    _compare(ref, got, rf.STEPS, rf.ROUNDS)
    _cost_does_not_rise(f, before, got)
    sizes = np.diff(got["track_off"])
    assert (fx.MAX_TRACK if which == "main" else fx.LONG_ROWS) in sizes
    assert np.array_equal(got["tinfo"][:, 2:], before["tinfo"][:, 2:])
    carried = before["tinfo"][:, 0] != 0
    assert np.all(got["tinfo"][carried, 0] == 1) and got["counts"][5] == carried.sum()
