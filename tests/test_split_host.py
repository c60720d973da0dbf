"""CPU checks of the split-track stage (posfeat_split_tracks in triangulate.hip,
split_plan.h): the ABI's argument validation (no device work), the numpy
restatement (tests/split_ref.py) on planted components -- triangulated by the
restatement of posfeat_triangulate first, so the input is what that call
leaves -- and on the hand-built table of tests/split_fixture.py, and the pure
header under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import split_fixture as sf
import split_ref as sr
import triangulate_fixture as fx
import triangulate_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


IN_NAMES = ("kp", "so", "cams", "poses", "points_in", "err_in", "tinfo_in", "track_off_in",
            "track_rows_in", "inlier_in", "counts_in")
OUT_NAMES = ("points", "err", "tinfo", "track_off", "track_rows", "obs_inlier", "point_of_row",
             "parent_of", "generation", "counts", "ws")


def test_argument_validation_without_a_device():
    from posfeat_amd import _lib
    L = _lib.lib()
    set_off, so = _i32([0, 300, 300, 2349, 2400])              # set 1 is empty
    need = L.posfeat_split_tracks_workspace(so, 4, 1000, 2000, 1000)
    assert need >= 2400 * 20 + 2000 * 5 + 1000 * (16 + 96 + 32 + 64)
    names = IN_NAMES + OUT_NAMES
    # dummies: non-null, 256-B aligned, all different (an output is no input)
    base = {k: ctypes.c_void_p(4096 * (i + 1)) for i, k in enumerate(names)}

    def call(nsets=4, tmax=1000, mmax=2000, iters=64, thr=4.0, min_angle=1.5, seed=0, rounds=2,
             tmax_out=1000, ws_bytes=need, **kw):
        a = dict(base)
        a["so"] = so
        a.update(kw)
        return L.posfeat_split_tracks(
            a["kp"], a["so"], nsets, a["cams"], a["poses"], a["points_in"], a["err_in"],
            a["tinfo_in"], a["track_off_in"], a["track_rows_in"], a["inlier_in"], a["counts_in"],
            tmax, mmax, iters, thr, min_angle, seed, rounds, tmax_out, a["points"], a["err"],
            a["tinfo"], a["track_off"], a["track_rows"], a["obs_inlier"], a["point_of_row"],
            a["parent_of"], a["generation"], a["counts"], a["ws"], ws_bytes, None)

    for name in names:
        assert call(**{name: None}) == -1, name                # a null pointer
    _, dec = _i32([0, 300, 299, 2349, 2400])
    _, neg = _i32([-1, 300, 300, 2349, 2400])
    _, off = _i32([1, 300, 300, 2349, 2400])
    for bad in (dec, neg, off):
        assert call(so=bad) == -1
        assert L.posfeat_split_tracks_workspace(bad, 4, 1000, 2000, 1000) == 0
    assert call(nsets=-1) == -1
    assert L.posfeat_split_tracks_workspace(None, 4, 1000, 2000, 1000) == 0
    for tmax, mmax, tout in ((-1, 2000, 1000), (1000, -1, 1000), (2 ** 31 - 1, 2000, 2 ** 31 - 1),
                             (1000, 2 ** 31, 1000), (1000, 2000, 999), (1000, 2000, 2 ** 31 - 1)):
        assert call(tmax=tmax, mmax=mmax, tmax_out=tout) == -1
        assert L.posfeat_split_tracks_workspace(so, 4, tmax, mmax, tout) == 0
    for iters in (7, 0, -1, 1025):
        assert call(iters=iters) == -1
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    for ang in (-0.1, 90.0, 180.0, float("nan"), float("inf")):
        assert call(min_angle=ang) == -1
    for rounds in (0, -1, 5):
        assert call(rounds=rounds) == -1
    # an output that is an input
    for o, i in (("points", "points_in"), ("err", "err_in"), ("tinfo", "tinfo_in"),
                 ("track_off", "track_off_in"), ("track_rows", "track_rows_in"),
                 ("obs_inlier", "inlier_in"), ("counts", "counts_in")):
        assert call(**{o: base[i]}) == -1, o
    assert call(ws=ctypes.c_void_p(4096 + 64)) == -1           # ws not 256-B aligned
    for name in ("points_in", "err_in", "points", "err", "cams", "poses"):
        assert call(**{name: ctypes.c_void_p(4100)}) == -1, name   # not 8-B aligned
    for name in ("kp", "tinfo_in", "track_off_in", "track_rows_in", "counts_in", "tinfo",
                 "track_off", "track_rows", "point_of_row", "parent_of", "generation", "counts"):
        assert call(**{name: ctypes.c_void_p(4098)}) == -1, name   # not 4-B aligned
    assert call(inlier_in=ctypes.c_void_p(4097), obs_inlier=ctypes.c_void_p(4099), ws_bytes=0) == -3
    # legal extremes: only the workspace is short
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=0) == -3
    assert call(iters=8, rounds=1, min_angle=0.0, ws_bytes=0) == -3
    assert call(iters=1024, rounds=4, min_angle=89.9, tmax=0, mmax=0, tmax_out=0, ws_bytes=0) == -3
    assert call(tmax_out=5000, seed=2 ** 64 - 1, ws_bytes=0) == -3


def _members(res, t):
    sl = slice(int(res["track_off"][t]), int(res["track_off"][t + 1]))
    return res["track_rows"][sl], res["obs_inlier"][sl]


def _is_partition(inp, res):
    """every parent's range is dealt out to it and its children, ascending in each"""
    Tp = int(res["counts"][0])
    assert res["track_off"][0] == inp["track_off"][0] and res["track_off"][Tp] == inp["track_off"][-1]
    assert np.all(np.diff(res["track_off"]) >= 0)
    for t in range(len(inp["track_off"]) - 1):
        mine = np.flatnonzero(res["parent_of"] == t)
        assert list(res["generation"][mine]) == list(range(len(mine)))
        sl = slice(int(res["track_off"][mine[0]]), int(res["track_off"][mine[-1] + 1]))
        want = inp["track_rows"][inp["track_off"][t]:inp["track_off"][t + 1]]
        assert sl.start == inp["track_off"][t] and sl.stop == inp["track_off"][t + 1]
        assert sorted(res["track_rows"][sl].tolist()) == sorted(want.tolist())
        for u in mine:
            rows, _ = _members(res, u)
            assert np.all(np.diff(rows.astype(np.int64)) > 0)
    return True


def test_restatement_splits_the_joined_component():
    """the 5 + 3 component of the triangulation fixture, joined by one wrong
    edge: posfeat_triangulate keeps the five and drops the three; the split
    gives one child with exactly the three planted rows"""
    f = fx.build(fx.FIXTURE_SEED)
    tri = tr.triangulate(f["kp"], f["set_off"], f["cams"], f["poses"], f["edges"], fx.ITERS, fx.THR,
                         fx.MIN_ANGLE, fx.MAX_TRACK, fx.SEED)
    T, M = int(tri["counts"][0]), int(tri["counts"][1])
    res = sr.split(f["kp"], f["set_off"], f["cams"], f["poses"], tri, T, M, fx.ITERS, fx.THR,
                   fx.MIN_ANGLE, fx.SEED, 2, M // 2)
    assert _is_partition(tri, res)
    five, three = f["cases"]["merge5"][0], f["cases"]["merge3"][0]
    t = [t for t in range(T) if min(five["rows"] + three["rows"]) == tri["track_rows"][tri["track_off"][t]]][0]
    mine = np.flatnonzero(res["parent_of"] == t)
    assert len(mine) == 2
    rows, flags = _members(res, mine[1])
    assert sorted(rows.tolist()) == sorted(three["rows"]) and np.all(flags == 1)
    assert np.abs(res["points"][mine[1]] - three["X"]).max() <= 1e-6 * np.abs(three["X"]).max()
    assert tuple(res["tinfo"][mine[1]][:2]) == (0, 3)
    rows, flags = _members(res, mine[0])
    assert sorted(rows.tolist()) == sorted(five["rows"]) and np.all(flags == 1)
    for r in three["rows"]:
        assert tri["point_of_row"][r] == -1 and res["point_of_row"][r] == mine[1]
    # the parents are the input, bit for bit
    par = res["generation"] == 0
    assert res["points"][par].tobytes() == tri["points"].tobytes()
    assert res["err"][par].tobytes() == tri["err"].tobytes()
    assert np.array_equal(res["tinfo"][par], tri["tinfo"])
    assert res["counts"][6] == (~par).sum() >= 1 and res["counts"][2] == tri["counts"][2] + res["counts"][6]
    assert res["counts"][3] > tri["counts"][3]


@pytest.fixture(scope="module")
def planted():
    b = sf.build(cheap=False)
    tab = sf.table(b)
    T, M = len(b.parents), len(tab["track_rows"])
    res = sr.split(b.kp, b.set_off, b.cams, b.poses, tab, T, M, sf.ITERS, sf.THR, sf.MIN_ANGLE,
                   sf.SEED, sf.ROUNDS, T + M // 2)
    return b, tab, res


def test_restatement_on_the_planted_table(planted):
    b, tab, res = planted
    assert _is_partition(tab, res)
    sf.check_cases(b, tab, res)


def test_restatement_capacity_rule(planted):
    """tmax_out one short: the last child in output order is not created, its
    rows stay with the parent unflagged, every later parent moves up by one"""
    b, tab, res = planted
    T, M = len(b.parents), len(tab["track_rows"])
    Tp = int(res["counts"][0])
    short = sr.split(b.kp, b.set_off, b.cams, b.poses, tab, T, M, sf.ITERS, sf.THR, sf.MIN_ANGLE,
                     sf.SEED, sf.ROUNDS, Tp - 1)
    assert _is_partition(tab, short)
    assert short["counts"][0] == Tp - 1 and short["counts"][4] == 1 and res["counts"][4] == 0
    assert short["counts"][6] == res["counts"][6] - 1
    last = int(np.flatnonzero(res["generation"] > 0)[-1])
    keep = np.ones(Tp, bool)
    keep[last] = False
    assert np.array_equal(short["parent_of"], res["parent_of"][keep])
    assert short["points"].tobytes() == res["points"][keep].tobytes()
    lost, _ = _members(res, last)
    assert np.all(short["point_of_row"][lost] == -1)
    p = int(np.flatnonzero((short["parent_of"] == res["parent_of"][last]) & (short["generation"] == 0))[0])
    rows, flags = _members(short, p)
    assert set(lost.tolist()) <= set(rows.tolist())
    assert np.all(flags[np.isin(rows, lost)] == 0)


def test_split_plan_under_host_sanitizers(tmp_path):
    """tests/host/split_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "split_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "split_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "split_plan ok" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]
