"""posfeat_split_tracks on the GPU against the numpy restatement of its
definitions (tests/split_ref.py) on the hand-built table of
tests/split_fixture.py: parents whose left-over lists have 0, 1, 2 (accepted;
rejected behind the cameras; rejected at a 0.002 baseline), 5, 6, 7, 64 and 65
rows, a 5 + 3 + 3 component, a refit that is not kept, a status-1 parent, rows
outside the pool, and 2100 two-view parents around them so the id scan crosses
a block.  iters = 64, thr = 4, min_angle = 1.5, rounds = 2.

The preconditions -- no reprojection error of a scored hypothesis or refit
within 1e-6 px of thr, no depth within 1e-9 of 0, no tested cosine within 1e-9
of cos(min_angle), the refit matrix's second smallest / largest eigenvalue >=
1e-4 on every kept child -- are asserted on the restatement before the device
result is looked at, so the integer outputs are compared exactly and the points
to 1e-9, ``err`` to 1e-9 relative where it is at least 0.1 px and to 1e-9 px
below that: the bounds of tests/test_gpu_triangulate.py, for its reasons (the
generations run that call's arithmetic)."""
import numpy as np
import pytest
import torch

import split_fixture as sf
import split_ref as sr
import triangulate_ref as tr

pytestmark = pytest.mark.gpu

EXACT = ("counts", "track_off", "track_rows", "obs_inlier", "tinfo", "point_of_row", "parent_of",
         "generation")


def _sub_table(tab, idx):
    """the table of the parents ``idx`` alone, in that order"""
    off = tab["track_off"]
    sl = [np.arange(off[t], off[t + 1]) for t in idx]
    cat = np.concatenate(sl) if sl else np.zeros(0, np.int64)
    tinfo = tab["tinfo"][idx]
    ok = tinfo[:, 0] == 0
    new_off = np.concatenate([[0], np.cumsum([len(s) for s in sl])]).astype(np.int32)
    return dict(points=tab["points"][idx], err=tab["err"][idx], tinfo=tinfo, track_off=new_off,
                track_rows=tab["track_rows"][cat], obs_inlier=tab["obs_inlier"][cat],
                counts=np.array([len(idx), len(cat), ok.sum(), tinfo[ok, 1].sum(), 0, 0, 0, 0],
                                np.int32))


def _device_tracks(b, tab):
    from posfeat_amd import geometry
    dev = torch.device("cuda:0")
    por = np.full(b.N, -1, np.int32)
    for t in range(len(tab["tinfo"])):
        if tab["tinfo"][t, 0] == 0:
            sl = slice(int(tab["track_off"][t]), int(tab["track_off"][t + 1]))
            rows = tab["track_rows"][sl][tab["obs_inlier"][sl] == 1]
            por[rows[(rows >= 0) & (rows < b.N)]] = t
    parts = dict(tab, point_of_row=por)
    return geometry.TrackResult(**{k: torch.from_numpy(np.ascontiguousarray(parts[k])).to(dev)
                                   for k in geometry.TrackResult.FIELDS})


def _scene_tensors(b):
    dev = torch.device("cuda:0")
    return (torch.from_numpy(b.kp).to(dev), b.set_off, torch.from_numpy(b.cams).to(dev),
            torch.from_numpy(b.poses).to(dev))


def _run(b, tab, host=True, **kw):
    from posfeat_amd import geometry
    args = dict(iters=sf.ITERS, thr=sf.THR, min_angle=sf.MIN_ANGLE, rounds=sf.ROUNDS, seed=sf.SEED)
    args.update(kw)
    res = geometry.split_tracks(*_scene_tensors(b), _device_tracks(b, tab), **args)
    return res.host() if host else res


def _ref(b, tab, tmax_out=None, **kw):
    T, M = len(tab["tinfo"]), len(tab["track_rows"])
    args = dict(iters=sf.ITERS, thr=sf.THR, min_angle_deg=sf.MIN_ANGLE, seed=sf.SEED,
                rounds=sf.ROUNDS)
    args.update(kw)
    return sr.split(b.kp, b.set_off, b.cams, b.poses, tab, T, M, tmax_out=max(T, M // 2)
                    if tmax_out is None else tmax_out, **args)


@pytest.fixture(scope="module")
def scene():
    b = sf.build()
    tab = sf.table(b)
    ref = _ref(b, tab)
    got = _run(b, tab)
    cases = [i for i, p in enumerate(b.parents) if p["name"] != "cheap"]
    return b, tab, ref, got, cases


def _compare(ref, got):
    for k in EXACT:
        assert np.array_equal(got[k], ref[k]), k
    scale = np.abs(ref["points"]).max(1)
    ok = ref["tinfo"][:, 0] == 0
    dp = np.abs(got["points"] - ref["points"]).max(1)
    de = np.abs(got["err"] - ref["err"])
    print("max relative point difference %.3g, max err difference %.3g px (rel %.3g)"
          % ((dp[ok] / scale[ok]).max(), de.max(),
             (de[ok] / np.maximum(ref["err"][ok], 1e-300)).max()))
    assert np.all(dp[ok] <= 1e-9 * scale[ok])
    assert np.all(got["points"][~ok] == 0.0) and np.all(got["err"][~ok] == 0.0)
    noisy = ok & (ref["err"] >= 0.1)
    assert np.all(de[noisy] <= 1e-9 * ref["err"][noisy])
    assert np.all(de[ok & ~noisy] <= 1e-9)


def test_fixture_preconditions(scene):
    b, tab, ref, _, cases = scene
    assert sf.check_cases(b, tab, ref)
    assert len(b.parents) > 2048 + len(cases) and min(cases) > 2048    # the scan crosses a block
    kid = np.flatnonzero(ref["generation"] > 0)
    assert ref["counts"][0] == len(b.parents) + len(kid) and ref["counts"][4] == 0
    assert ref["counts"][6] == len(kid) >= 16 and ref["counts"][7] == len(set(ref["parent_of"][kid]))
    assert (ref["generation"] == 2).sum() >= 2                # second generations, lane and wave kind
    g2 = {b.parents[p]["name"] for p in ref["parent_of"][ref["generation"] == 2]}
    assert "533" in g2 and g2 & {"L64", "L65"}


def test_equals_restatement(scene):
    _, _, ref, got, _ = scene
    _compare(ref, got)


def test_partition_and_parents_bit_identical(scene):
    b, tab, _, got, _ = scene
    Tp, T = int(got["counts"][0]), len(b.parents)
    # every row is a member of exactly one output track, and of the parent's range
    assert got["track_off"][0] == 0 and got["track_off"][Tp] == len(tab["track_rows"])
    assert np.all(np.diff(got["track_off"]) >= 2)
    assert np.array_equal(np.sort(got["track_rows"]), np.sort(tab["track_rows"]))
    assert len(np.unique(got["track_rows"])) == len(got["track_rows"])
    par = np.flatnonzero(got["generation"] == 0)
    assert np.array_equal(got["parent_of"][par], np.arange(T))
    assert np.all(np.diff(got["parent_of"]) >= 0)
    for t in range(T):
        lo, hi = int(tab["track_off"][t]), int(tab["track_off"][t + 1])
        mine = np.flatnonzero(got["parent_of"] == t)
        assert got["track_off"][mine[0]] == lo and got["track_off"][mine[-1] + 1] == hi
        assert np.array_equal(got["generation"][mine], np.arange(len(mine)))
    # the parents: point, err, tinfo bit for bit; the flags of the members they keep
    assert got["points"][par].tobytes() == tab["points"].tobytes()
    assert got["err"][par].tobytes() == tab["err"].tobytes()
    assert np.array_equal(got["tinfo"][par], tab["tinfo"])
    flag_in = dict(zip(tab["track_rows"].tolist(), tab["obs_inlier"].tolist()))
    for u in range(Tp):
        sl = slice(int(got["track_off"][u]), int(got["track_off"][u + 1]))
        rows, flags = got["track_rows"][sl], got["obs_inlier"][sl]
        assert np.all(np.diff(rows.astype(np.int64)) > 0)
        if got["generation"][u] == 0:
            assert [flag_in[r] for r in rows.tolist()] == flags.tolist()
        else:
            assert np.all(flags == 1) and got["tinfo"][u, 1] == len(rows)
            assert np.all(got["point_of_row"][rows] == u)


def test_repeat_is_bit_identical(scene):
    b, tab, _, got, _ = scene
    again = _run(b, tab)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_other_parents_do_not_matter(scene):
    b, tab, _, got, cases = scene
    small = _run(b, _sub_table(tab, cases))
    assert small["counts"][0] == got["counts"][0] - (len(b.parents) - len(cases))
    for i, t in enumerate(cases):
        a, c = np.flatnonzero(small["parent_of"] == i), np.flatnonzero(got["parent_of"] == t)
        assert len(a) == len(c)
        for u, v in zip(a, c):
            ru = small["track_rows"][small["track_off"][u]:small["track_off"][u + 1]]
            rv = got["track_rows"][got["track_off"][v]:got["track_off"][v + 1]]
            assert np.array_equal(ru, rv)
            assert small["points"][u].tobytes() == got["points"][v].tobytes()
            assert small["err"][u].tobytes() == got["err"][v].tobytes()
            assert np.array_equal(small["tinfo"][u], got["tinfo"][v])
            assert np.array_equal(
                small["obs_inlier"][small["track_off"][u]:small["track_off"][u + 1]],
                got["obs_inlier"][got["track_off"][v]:got["track_off"][v + 1]])


def test_one_round(scene):
    """rounds = 1: the 5 + 3 + 3 component gives one child; the other group
    stays with the parent as unflagged members"""
    b, tab, _, _, cases = scene
    sub = _sub_table(tab, cases)
    names = [b.parents[t]["name"] for t in cases]
    ref = _ref(b, sub, rounds=1)
    p = names.index("533")
    assert ((ref["parent_of"] == p) & (ref["generation"] > 0)).sum() == 1
    assert ref["generation"].max() == 1
    q = int(np.flatnonzero((ref["parent_of"] == p) & (ref["generation"] == 0))[0])
    sl = slice(int(ref["track_off"][q]), int(ref["track_off"][q + 1]))
    assert sl.stop - sl.start == 8 and ref["obs_inlier"][sl].sum() == 5
    _compare(ref, _run(b, sub, rounds=1))


def test_lane_kernel_sampler_path(scene):
    """iters = 8: the lists of 5 and 6 rows (10 and 15 pairs) draw their pairs
    from the sampler inside the lane kernel"""
    b, tab, _, _, cases = scene
    sub = _sub_table(tab, cases)
    ref = _ref(b, sub, iters=8)
    mg = ref["margins"]
    print("margins", mg)
    assert mg["err"] > 1e-6 and mg["depth"] > 1e-9 and mg["cos"] > 1e-9
    kept = (ref["generation"] > 0) & (ref["tinfo"][:, 3] == 1)
    assert kept.sum() >= 4 and np.all(ref["eig_ratio"][kept] >= 1e-4)
    _compare(ref, _run(b, sub, iters=8))


def test_capacity_one_short(scene):
    """tmax_out = T' - 1: the last child is not created, its rows stay with the
    parent, the parents after it move up by one"""
    b, tab, ref, got, _ = scene
    Tp = int(ref["counts"][0])
    short_ref = _ref(b, tab, tmax_out=Tp - 1)
    assert short_ref["counts"][0] == Tp - 1 and short_ref["counts"][4] == 1
    last = int(np.flatnonzero(ref["generation"] > 0)[-1])
    assert last < Tp - 1                                       # parents follow the refused child
    short = _run(b, tab, tmax_out=Tp - 1)
    _compare(short_ref, short)
    lost = got["track_rows"][got["track_off"][last]:got["track_off"][last + 1]]
    assert np.all(short["point_of_row"][lost] == -1) and short["counts"][4] == 1


def test_result_feeds_refine_and_reprojects(scene):
    """the result goes through refine_tracks as it is; every status-0 point, of
    the split result and of the refined one, reprojects within thr into every
    flagged member"""
    from posfeat_amd import geometry
    b, tab, _, got, _ = scene
    res = _run(b, tab, host=False)
    refined = geometry.refine_tracks(*_scene_tensors(b), res, thr=sf.THR, min_angle=sf.MIN_ANGLE).host()
    assert refined["counts"][0] == got["counts"][0]
    # the exact two-view parents (angles of 4 degrees and more) cannot be lost
    assert refined["counts"][1] >= sf.CHEAP_BEFORE + sf.CHEAP_AFTER
    sc = tr.Scene(b.kp, b.set_off, b.cams, b.poses)
    for name, r in (("split", got), ("refined", refined)):
        worst = 0.0
        for u in np.flatnonzero(r["tinfo"][:, 0] == 0):
            sl = slice(int(r["track_off"][u]), int(r["track_off"][u + 1]))
            rows = r["track_rows"][sl][r["obs_inlier"][sl] != 0].astype(np.int64)
            assert len(rows) == r["tinfo"][u, 1] >= 2 and rows.max() < b.N
            e2, z = sc.reproj2_rows(rows, r["points"][u])
            assert np.all(z > 0) and np.all(e2 <= sf.THR ** 2), (name, u)
            worst = max(worst, float(np.sqrt(e2.max())))
        print("%s: largest reprojection error of a flagged member %.3g px" % (name, worst))
