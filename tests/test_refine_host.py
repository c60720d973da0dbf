"""CPU checks of the point-refinement stage (refine.hip / refine_solve.h):
posfeat_refine_point against the numpy restatement (tests/refine_ref.py) and
against properties that do not involve the restatement, the restatement itself
on the hand-built track table (tests/refine_fixture.py), the ABI's argument
validation (no device work) and the pure header under the host sanitizers.

The planted systems are those of the experiment that motivated the stage: 2..8
views at distances 2..40 (log-uniform) with focal lengths 400..1600, every
second camera SIMPLE_RADIAL with k1 = -0.05, every second system with 1 px
noise; the starting point is the DLT point."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import refine_fixture as rf
import refine_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def systems():
    return rf.systems()


def test_fixture_is_well_conditioned(systems):
    assert len(systems) == 200
    assert {len(s["obs"]) for s in systems} == set(range(2, 9))
    for s in systems:
        assert rf.normal_condition(s["obs"], s["X"]) <= rf.COND_MAX
    d = [np.linalg.norm(-o[10:22].reshape(3, 4)[:, :3].T @ o[10:22].reshape(3, 4)[:, 3] - s["X"])
         for s in systems for o in s["obs"]]
    f = [o[2] for s in systems for o in s["obs"]]
    assert min(d) < 3.0 and max(d) > 30.0 and min(f) < 450.0 and max(f) > 1400.0


def test_refine_point_equals_restatement(systems):
    """to 1e-9 max |X|, the bound of the triangulate test: fp64 eps times the
    condition number of the normal matrix, which the fixture holds <= 1e6.
    Measured: identical bits on all 200 systems (the host compiles without
    contraction, numpy does not contract either)."""
    from posfeat_amd import geometry
    worst = 0.0
    for s in systems:
        X, cost, taken = geometry.refine_point(s["obs"], s["X0"], rf.STEPS)
        Xr, cr, tr_ = rr.refine_point(s["obs"], s["X0"], rf.STEPS)
        worst = max(worst, np.abs(X - Xr).max() / np.abs(Xr).max())
        assert np.abs(X - Xr).max() <= 1e-9 * np.abs(Xr).max()
        assert abs(cost - cr) <= 1e-9 * cr + 1e-12 and 0 <= taken <= rf.STEPS
    print("largest relative difference to the restatement %.3g" % worst)


def test_refine_point_properties(systems):
    """independent of the restatement's round: exact observations recover the
    planted point, the cost does not rise, the gradient vanishes, the noisy
    systems gain what the numpy experiment gained.
    First-order optimality: |g|_inf against sum |J| |r| over the rows.  The
    restatement reaches 2.7e-8 at the most on the noisy systems in 10 steps;
    the bound is 1e-6, a margin of 40."""
    from posfeat_amd import geometry
    ratios, worst_g = [], 0.0
    for s in systems:
        X, cost, _ = geometry.refine_point(s["obs"], s["X0"], rf.STEPS)
        c0, c1 = rr.cost_of(s["obs"], s["X0"]), rr.cost_of(s["obs"], X)
        assert cost <= c0 and abs(c1 - cost) <= 1e-9 * c1 + 1e-12
        if not s["noisy"]:
            assert np.abs(X - s["X"]).max() <= 1e-9 * max(1.0, np.abs(s["X"]).max())
            continue
        g, scale = rr.gradient_of(s["obs"], X)
        worst_g = max(worst_g, np.abs(g).max() / scale)
        assert np.abs(g).max() <= 1e-6 * scale
        ratios.append(cost / c0)
    print("median cost ratio to the DLT point %.3f, largest |g| / sum |J||r| %.3g"
          % (np.median(ratios), worst_g))
    assert len(ratios) == 100 and np.median(ratios) < 0.6


def test_refine_point_edges():
    from posfeat_amd import geometry
    s = rf.systems(count=4)[3]
    X, cost, taken = geometry.refine_point(s["obs"], [np.nan, 0.0, 0.0], 10)
    assert taken == 0 and np.isnan(cost) and np.isnan(X[0]) and X[1] == 0.0
    X1, c1, t1 = geometry.refine_point(s["obs"], s["X0"], 1)
    assert t1 <= 1 and c1 <= rr.cost_of(s["obs"], s["X0"])
    for bad in (0, 33, -1):
        with pytest.raises(ValueError):
            geometry.refine_point(s["obs"], s["X0"], bad)
    with pytest.raises(ValueError):
        geometry.refine_point(s["obs"][:1], s["X0"], 10)
    with pytest.raises(ValueError):
        geometry.refine_point(s["obs"][:, :21], s["X0"], 10)


def test_long_track_order_on_the_host():
    """more than LANE_TRACK rows: the 64 partial sums and the butterfly, the
    same in the library and in the restatement"""
    from posfeat_amd import geometry
    rng = np.random.RandomState(2)
    import triangulate_ref as tr
    for n in (17, 64, 65, 130):
        X = rng.uniform(-0.3, 0.3, 3)
        obs = []
        for v in range(n):
            cam, pose = rf.spread_camera(rng, v, np.zeros(3))
            px, py, _ = tr.project(cam, pose, X)
            obs.append(np.concatenate([[px, py] + rng.normal(0, 1.0, 2), cam, pose]))
        obs = np.asarray(obs)
        X0 = X + 0.02
        got, cost, taken = geometry.refine_point(obs, X0, 10)
        want, cr, tr_ = rr.refine_point(obs, X0, 10)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max() and taken >= 1
        assert cost <= rr.cost_of(obs, X0) and np.abs(got - X).max() < 0.05


def test_restatement_on_the_hand_built_table():
    """the restatement itself (no device): the cases are what they are meant to
    be, and the margins the device comparison needs hold"""
    f = rf.build_table()
    ref = rr.refine(f["kp"], f["set_off"], f["cams"], f["poses"], f["tracks"], rf.THR, rf.MIN_ANGLE,
                    rf.ROUNDS, rf.STEPS)
    assert ref["margins"]["err2"] > 1e-6 and ref["margins"]["cos"] > 1e-9
    c = {k: v[0] for k, v in f["cases"].items()}
    tin, rin = ref["tinfo"], ref["rinfo"]

    def flags(case):
        t = case["t"]
        return ref["obs_inlier"][f["tracks"]["track_off"][t]:f["tracks"]["track_off"][t + 1]]

    t = c["outlier"]["t"]
    assert tuple(tin[t, :2]) == (0, 13) and tuple(rin[t, [0, 2, 3]]) == (2, 1, 1)
    assert flags(c["outlier"])[c["outlier"]["rows"].index(c["outlier"]["outlier"])] == 0
    t = c["readmit"]["t"]
    assert tuple(tin[t, :2]) == (0, 5) and tuple(rin[t, [0, 2, 3]]) == (2, 1, 1)
    assert flags(c["readmit"])[c["readmit"]["rows"].index(c["readmit"]["readmitted"])] == 1
    for name in ("one_inlier", "no_inlier", "nan_point"):
        t = c[name]["t"]
        assert tuple(tin[t, :2]) == (2, 0) and not flags(c[name]).any()
        assert np.all(ref["points"][t] == 0) and ref["err"][t] == 0
    assert tuple(rin[c["nan_point"]["t"]]) == (1, 0, 0, 1)
    for name in ("low_parallax", "same_image_only"):
        t = c[name]["t"]
        assert tuple(tin[t, :2]) == (3, 0) and not flags(c[name]).any() and rin[t, 2] == 1
    t = c["same_image_plus_one"]["t"]
    assert tuple(tin[t, :2]) == (0, 3)
    t = c["status1"]["t"]
    assert tuple(tin[t]) == (1, 0, -1, 0) and tuple(rin[t]) == (0, 0, 0, 0)
    t = c["bad_row"]["t"]
    assert tuple(tin[t, :2]) == (0, 4) and flags(c["bad_row"])[-1] == 0 and rin[t, 3] == 1
    for m in (2, rf.LANE_TRACK, rf.LANE_TRACK + 1, 64, 65, 130):
        t = c["size%d" % m]["t"]
        assert len(c["size%d" % m]["rows"]) == m and tin[t, 0] == 0 and rin[t, 1] >= 1
    ok = tin[:, 0] == 0
    assert np.all(ref["cost_out"][ok] <= ref["cost_in"][ok])
    assert np.all(rin[:, 1] <= rf.STEPS * rin[:, 0])
    assert np.array_equal(tin[:, 2:], f["tracks"]["tinfo"][:, 2:])
    assert ref["counts"].tolist() == [len(tin), int(ok.sum()), int(tin[ok, 1].sum()),
                                      int((tin[:, 0] == 2).sum()), int((tin[:, 0] == 3).sum()), 1,
                                      int(rin[:, 3].sum()), 0]
    # the extremes on the same table
    for rounds, steps in ((1, rf.STEPS), (rf.ROUNDS, 1)):
        r = rr.refine(f["kp"], f["set_off"], f["cams"], f["poses"], f["tracks"], rf.THR,
                      rf.MIN_ANGLE, rounds, steps)
        assert r["margins"]["err2"] > 1e-6 and r["margins"]["cos"] > 1e-9
        assert np.all(r["rinfo"][:, 0] <= rounds) and np.all(r["rinfo"][:, 1] <= steps * rounds)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_argument_validation_without_a_device():
    from posfeat_amd import _lib
    L = _lib.lib()
    set_off, so = _i32([0, 300, 300, 2349, 2400])              # set 1 is empty
    need = L.posfeat_refine_points_workspace(so, 4, 1000, 2000)
    assert need >= 2400 * 4 + 5 * 4
    p = ctypes.c_void_p(4096)                                  # dummy, non-null, 256-B aligned
    names = ("kp", "so", "cams", "poses", "points_in", "tinfo_in", "track_off", "track_rows",
             "inlier_in", "counts_in", "points", "err", "tinfo", "obs_inlier", "point_of_row",
             "rinfo", "counts", "ws")

    def call(nsets=4, tmax=1000, mmax=2000, thr=4.0, min_angle=1.5, rounds=3, steps=10,
             ws_bytes=need, **kw):
        a = {k: p for k in names}
        a["so"] = so
        a.update(kw)
        return L.posfeat_refine_points(
            a["kp"], a["so"], nsets, a["cams"], a["poses"], a["points_in"], a["tinfo_in"],
            a["track_off"], a["track_rows"], a["inlier_in"], a["counts_in"], tmax, mmax, thr,
            min_angle, rounds, steps, a["points"], a["err"], a["tinfo"], a["obs_inlier"],
            a["point_of_row"], a["rinfo"], a["counts"], a["ws"], ws_bytes, None)

    for name in names:
        assert call(**{name: None}) == -1, name                # a null pointer
    _, dec = _i32([0, 300, 299, 2349, 2400])
    _, neg = _i32([-1, 300, 300, 2349, 2400])
    _, off = _i32([1, 300, 300, 2349, 2400])
    for bad in (dec, neg, off):
        assert call(so=bad) == -1
        assert L.posfeat_refine_points_workspace(bad, 4, 1000, 2000) == 0
    assert call(nsets=-1) == -1 and L.posfeat_refine_points_workspace(None, 4, 1000, 2000) == 0
    for tmax, mmax in ((-1, 2000), (1000, -1), (2 ** 31 - 1, 2000), (1000, 2 ** 31)):
        assert call(tmax=tmax, mmax=mmax) == -1
        assert L.posfeat_refine_points_workspace(so, 4, tmax, mmax) == 0
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    for ang in (-0.1, 90.0, 180.0, float("nan"), float("inf")):
        assert call(min_angle=ang) == -1
    for rounds in (0, -1, 9):
        assert call(rounds=rounds) == -1
    for steps in (0, -1, 33):
        assert call(steps=steps) == -1
    assert call(ws=ctypes.c_void_p(4096 + 64)) == -1           # ws not 256-B aligned
    for name in ("points_in", "points", "err", "cams", "poses"):
        assert call(**{name: ctypes.c_void_p(4100)}) == -1, name   # not 8-B aligned
    for name in ("kp", "tinfo_in", "track_off", "track_rows", "counts_in", "tinfo", "point_of_row",
                 "rinfo", "counts"):
        assert call(**{name: ctypes.c_void_p(4098)}) == -1, name   # not 4-B aligned
    assert call(inlier_in=ctypes.c_void_p(4097), obs_inlier=ctypes.c_void_p(4099), ws_bytes=0) == -3
    # legal extremes: only the workspace is short
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert call(rounds=1, steps=1, min_angle=0.0, ws_bytes=0) == -3
    assert call(rounds=8, steps=32, min_angle=89.9, tmax=0, mmax=0, ws_bytes=0) == -3
    x = np.zeros(3)
    px = ctypes.c_void_p(x.ctypes.data)
    for args in ((None, 2, px, 10, px, px), (px, 2, None, 10, px, px), (px, 2, px, 10, None, px),
                 (px, 2, px, 10, px, None), (px, 1, px, 10, px, px), (px, 2, px, 0, px, px),
                 (px, 2, px, 33, px, px)):
        assert L.posfeat_refine_point(*args) == -1


def test_refine_solve_under_host_sanitizers(tmp_path):
    """tests/host/refine_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "refine_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "refine_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "refine_solve ok" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]
