"""Host-side checks of the five-point RANSAC essential-matrix definitions: the
sampler at k = 5, posfeat_essential_solve5 against an independent method and the
numpy restatement (tests/essential_ref.py), posfeat_essential_decompose on
planted poses, ABI validation with dummy pointers, the solver under the host
sanitizers, the restatement on a planted scene, and the relative-pose metrics.
No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import essential_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 0x123456789ABCDEF0, (1 << 64) - 1)          # those of test_ransac_host.py
KINDS = ("general", "forward", "sideways", "planar")


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("n", [5, 6, 64, 65, 8192])
def test_sampler5_equals_restatement(n):
    from posfeat_amd import geometry
    for seed in SEEDS:
        for pair in (0, 99):
            for it in range(256):
                got = geometry.sample_indices(seed, pair, it, n, k=5)
                assert got.dtype == np.int32 and got.tolist() == ER.sample(seed, pair, it, n, 5)
                assert got[:4].tolist() == geometry.sample_indices(seed, pair, it, n).tolist()
                assert len(set(got.tolist())) == 5 and got.min() >= 0 and got.max() < n


def _rot(ax):
    th = np.linalg.norm(ax)
    k = ax / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def _scene(rs, kind, n=5):
    """n matches (x, y, u, v) in normalised camera coordinates of random 3-D
    points in front of two cameras, with the planted (R, t): general motion,
    pure forward or sideways translation, or a tilted plane under general
    motion"""
    X = np.stack([rs.uniform(-2, 2, n), rs.uniform(-1.5, 1.5, n), rs.uniform(3, 9, n)], 1)
    if kind == "planar":
        X[:, 2] = 6.0 + 0.5 * X[:, 0] - 0.3 * X[:, 1]
    if kind in ("general", "planar"):
        R = _rot(rs.uniform(-0.08, 0.08, 3))
        t = np.array([rs.uniform(0.3, 0.8), rs.uniform(-0.2, 0.2), rs.uniform(0.2, 0.6)])
    elif kind == "forward":
        R, t = np.eye(3), np.array([0.0, 0.0, rs.uniform(0.4, 1.0)])
    else:
        R, t = np.eye(3), np.array([rs.uniform(0.4, 1.0), rs.uniform(-0.3, 0.3), 0.0])
    Y = X @ R.T + t
    return np.concatenate([X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]], 1), R, t


def _cons(E):
    """the ten cubic constraints at a numeric E"""
    EEt = E @ E.T
    return np.concatenate([[np.linalg.det(E)], (2 * EEt @ E - np.trace(EEt) * E).reshape(-1)])


DEG3 = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1),
        (0, 1, 2), (0, 0, 3)]
LOW = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0),
       (0, 0, 1), (0, 0, 0)]


def _independent(m, rs):
    """the candidates by a computation that shares none of the defined steps:
    SVD null space, the 10x20 coefficient matrix fitted to the constraints'
    values at random points, the 10x10 multiplication-by-x action matrix on the
    monomials of degree <= 2, np.linalg.eig.  Returns (unit-norm sign-fixed
    candidates [c, 9], relative separation of the eigenvalues)."""
    _, _, vt = np.linalg.svd(ER.system(m))
    Eb = vt[5:9].reshape(4, 3, 3)
    mons = DEG3 + LOW
    pts = rs.uniform(-1, 1, (60, 3))
    Vm = np.array([[p[0] ** a * p[1] ** b * p[2] ** c for a, b, c in mons] for p in pts])
    vals = np.array([_cons(p[0] * Eb[0] + p[1] * Eb[1] + p[2] * Eb[2] + Eb[3]) for p in pts])
    C = np.linalg.lstsq(Vm, vals, rcond=None)[0].T         # [10, 20]
    Rm = -np.linalg.solve(C[:, :10], C[:, 10:])            # each cubic monomial over LOW
    Ax = np.zeros((10, 10))
    for i, mon in enumerate(LOW):
        t = (mon[0] + 1, mon[1], mon[2])
        if t in LOW:
            Ax[i, LOW.index(t)] = 1.0
        else:
            Ax[i] = Rm[DEG3.index(t)]
    w, V = np.linalg.eig(Ax)
    sep = min(abs(w[i] - w[j]) for i in range(10) for j in range(i)) / max(1.0, np.abs(w).max())
    out = []
    for k in range(10):
        if abs(w[k].imag) <= 1e-9 * max(1.0, abs(w[k])):
            v = (V[:, k] / V[9, k]).real
            out.append(ER.unit(v[6] * Eb[0] + v[7] * Eb[1] + v[8] * Eb[2] + Eb[3]).reshape(-1))
    return np.array(out).reshape(-1, 9), float(sep)


def _set_distance(a, b):
    """largest distance from a member of one set to the nearest of the other,
    members compared up to sign (test_fundamental_host._set_distance)"""
    d = np.minimum(np.abs(a[:, None, :] - b[None, :, :]).max(2),
                   np.abs(a[:, None, :] + b[None, :, :]).max(2))
    return float(max(d.min(1).max(), d.min(0).max()))


def test_solve5_against_an_independent_method():
    """Measured (RandomState(2024), 110 of 120 scenes compared): library and
    restatement each 6.1e-9 from the independent method at worst; cubic
    constraints 4.4e-16 at worst, at most 0.1 of what the independent method
    leaves on the same scene."""
    from posfeat_amd import geometry
    rs = np.random.RandomState(2024)
    worst_lib, worst_ref, used = 0.0, 0.0, 0
    res = dict(epi_lib=0.0, epi_ind=0.0, con_lib=0.0, con_ind=0.0)
    over = []
    for trial in range(120):
        kind = KINDS[trial % 4]
        m, _, _ = _scene(rs, kind)
        ind, sep = _independent(m, rs)
        if sep < 1e-3:                                     # the sets are compared only when the
            continue                                       # solutions are well apart
        used += 1
        got = geometry.solve5(m).reshape(-1, 9)
        ref = np.array(ER.solve5(m)).reshape(-1, 9)
        assert len(got) == len(ind) == len(ref) and len(got) > 0, (trial, kind)
        worst_ref = max(worst_ref, _set_distance(ref, ind))
        worst_lib = max(worst_lib, _set_distance(got, ind))
        A = ER.system(m)
        e_ind = max(np.abs(A @ E).max() for E in ind)
        c_ind = max(np.abs(_cons(E.reshape(3, 3))).max() for E in ind)
        for E in got:
            assert abs(np.sqrt((E ** 2).sum()) - 1.0) <= 1e-14
            assert E.max() >= np.abs(E).max() * (1 - 4e-16)    # a pure translation has two
            e, cc = np.abs(A @ E).max(), np.abs(_cons(E.reshape(3, 3))).max()
            res.update(epi_lib=max(res["epi_lib"], e), epi_ind=max(res["epi_ind"], e_ind),
                       con_lib=max(res["con_lib"], cc), con_ind=max(res["con_ind"], c_ind))
            # against what the independent method's own candidates leave on this scene
            if not (e <= 100 * e_ind and cc <= 100 * c_ind):
                over.append((trial, kind, e / e_ind, cc / c_ind))
    print("solve5 vs SVD + action matrix: library %.3g, restatement %.3g over %d scenes; worst "
          "residuals: epipolar %.3g (independent %.3g), cubic constraints %.3g (independent %.3g)"
          % (worst_lib, worst_ref, used, res["epi_lib"], res["epi_ind"], res["con_lib"],
             res["con_ind"]))
    assert used >= 90
    # the bound: what the two CPU methods disagree by between themselves, times 100
    assert worst_lib <= 100 * worst_ref, (worst_lib, worst_ref)
    m, _, _ = _scene(rs, "general")                        # a repeated match: rejected
    m[4] = m[1]
    assert geometry.solve5(m).shape == (0, 3, 3) and ER.solve5(m) == []
    with pytest.raises(ValueError):
        geometry.solve5(np.zeros((4, 4)))
    # last, so that everything above is checked first
    print("scenes whose residuals exceed 100 x the independent method's: %d of %d, worst ratios "
          "epipolar %.3g, cubic %.3g" % (len(set(o[0] for o in over)), used,
                                         max([o[2] for o in over] + [0]),
                                         max([o[3] for o in over] + [0])))
    assert not over, over[:5]


def test_decompose_essential_recovers_planted_poses():
    from posfeat_amd import geometry
    rs = np.random.RandomState(7)
    reached = set()
    for trial in range(40):
        m, R, t = _scene(rs, KINDS[trial % 4], 20)
        if trial % 2:                                      # the views swapped: the inverse motion
            m, R, t = m[:, [2, 3, 0, 1]], R.T, -R.T @ t
        tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
        E = (tx @ R) * rs.choice([-1.0, 1.0]) * rs.uniform(0.5, 2.0)
        pose, k, nf = geometry.decompose_essential(E, m)
        rpose, rk, rnf = ER.decompose(E, m)
        assert (k, nf) == (rk, rnf) and np.abs(pose - rpose).max() <= 1e-12
        reached.add(k)
        Re, te = pose[:, :3], pose[:, 3]
        assert nf == 20
        assert np.abs(Re @ Re.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(Re) - 1) <= 1e-14
        ang = np.arccos(np.clip((np.trace(Re.T @ R) - 1) / 2, -1, 1))
        # arccos near 1 loses half the digits: the angle from the skew part instead
        S = Re.T @ R
        ang = min(ang, np.linalg.norm([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]]) / 2)
        tang = np.linalg.norm(np.cross(te, t / np.linalg.norm(t)))
        assert ang <= 1e-9 and tang <= 1e-9 and te @ t > 0, (trial, ang, tang)
    print("decompositions reached:", sorted(reached))
    assert reached == {0, 1, 2, 3}
    with pytest.raises(ValueError):
        geometry.decompose_essential(np.zeros((3, 3)), np.zeros((2, 4)))
    with pytest.raises(ValueError):
        geometry.decompose_essential(np.eye(3), np.zeros((2, 3)))


def test_essential_abi_host_only_calls():
    from posfeat_amd import _lib
    L = _lib.lib()
    out, op = _i32([0] * 8)
    assert L.posfeat_essential_solve5(None, op) == -1
    assert L.posfeat_essential_decompose(None, op, 0, op, op) == -1
    assert L.posfeat_essential_decompose(op, None, 1, op, op) == -1
    assert L.posfeat_essential_decompose(op, op, -1, op, op) == -1
    set_off, so = _i32([0, 300, 300, 1300, 3349])          # set 1 is empty
    pairs, pp = _i32([[0, 2], [2, 3], [1, 0], [3, 3]])
    need = L.posfeat_ransac_essential_workspace(so, 4, pp, 4, 256)
    assert need >= 32 * (300 + 1000 + 0 + 2049) + 80 * 2560 * 4
    assert L.posfeat_ransac_essential_workspace(so, 4, pp, 4, 65536) > need
    p = ctypes.c_void_p(4096)                              # dummy, non-null, 256-B aligned

    def call(kp=p, cams=p, so=so, nsets=4, pp=pp, npairs=4, matches=p, counts=p, iters=256,
             thr=3.0, E=p, pose=p, info=p, cheir=p, inlier=p, ws=p, ws_bytes=need):
        return L.posfeat_ransac_essential(kp, cams, so, nsets, pp, npairs, matches, counts, iters,
                                          thr, 0, E, pose, info, cheir, inlier, ws, ws_bytes, None)

    for name in ("kp", "cams", "so", "pp", "matches", "counts", "E", "pose", "info", "cheir",
                 "inlier", "ws"):
        assert call(**{name: None}) == -1, name            # a null pointer
    _, bad_hi = _i32([[0, 2], [2, 4]])
    _, bad_lo = _i32([[0, 2], [-1, 3]])
    _, dec = _i32([0, 300, 299, 1300, 3349])
    _, neg = _i32([-1, 300, 300, 1300, 3349])
    assert call(pp=bad_hi, npairs=2) == -1                 # set index out of range
    assert call(pp=bad_lo, npairs=2) == -1
    assert call(so=dec) == -1                              # decreasing set_off
    assert call(so=neg) == -1                              # negative set_off
    for iters in (0, -1, 65537):
        assert call(iters=iters) == -1
        assert L.posfeat_ransac_essential_workspace(so, 4, pp, 4, iters) == 0
    assert call(iters=65536) == -3                         # a legal count: only the workspace is short
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    # sum n1 = 3 x 2^30 does not fit the int32 match offsets
    _, big = _i32([0, 1 << 30])
    _, bigp = _i32([[0, 0]] * 3)
    assert call(so=big, nsets=1, pp=bigp, npairs=3, ws_bytes=1 << 62) == -1
    assert L.posfeat_ransac_essential_workspace(big, 1, bigp, 3, 256) == 0
    assert call(ws_bytes=need - 1) == -3                   # short workspace
    assert call(ws_bytes=0) == -3
    assert L.posfeat_ransac_essential_workspace(dec, 4, pp, 4, 256) == 0
    assert L.posfeat_ransac_essential_workspace(so, 4, bad_hi, 2, 256) == 0
    assert L.posfeat_ransac_essential_workspace(None, 4, pp, 4, 256) == 0


def test_essential_solve_under_host_sanitizers(tmp_path):
    """tests/host/essential_solve_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "essential_solve_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "essential_solve_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "essential_solve ok" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]


def test_restatement_recovers_a_planted_pose():
    """the restatement itself on a 60-match scene (no device).  Pose bound: the
    40 planted matches are exact up to the fp32 rounding of the pixels (2^-24 *
    640 px = 8e-8 normalised); the refit over them amplifies that by the
    inverse of baseline / depth = 0.1 and the conditioning of the 9x9 fit, a few
    hundred in all: 1e-3 degrees."""
    from posfeat_amd.evaluation.relative_pose import relative_pose_errors
    cam = np.array([500.0, 500.0, 320.0, 240.0, 0, 0, 0, 0])
    rs = np.random.RandomState(5)
    m, R, t = _scene(rs, "general", 60)
    px = np.concatenate([m[:, :2] * 500 + [320, 240], m[:, 2:] * 500 + [320, 240]], 1)
    px[40:, 2:] += rs.uniform(30, 200, (20, 2)) * rs.choice([-1, 1], (20, 2))
    px = px.astype(np.float32)
    out = ER.ransac(px[:, :2], px[:, 2:], cam, cam, 0, 128, 3.0, 5)
    assert out["status"] == 0 and out["mask"][:40].all() and 40 <= out["n_inliers"] <= 43
    E = out["E"]
    assert abs(np.sqrt((E ** 2).sum()) - 1) < 1e-15 and E.reshape(-1)[np.argmax(np.abs(E))] > 0
    s = np.linalg.svd(E, compute_uv=False)
    assert abs(s[0] - s[1]) <= 1e-12 and s[2] <= 1e-12
    gt = np.concatenate([R, (t / np.linalg.norm(t))[:, None]], 1)
    er, et = relative_pose_errors(out["pose"], gt)
    print("restatement pose error: rotation %.3g deg, translation %.3g deg" % (er, et))
    assert er <= 1e-3 and et <= 1e-3 and out["cheir"][1] >= 40
    assert ER.ransac(px[:4, :2], px[:4, 2:], cam, cam, 0, 64, 3.0, 5)["status"] == 1


def test_relative_pose_errors_and_auc():
    from posfeat_amd.evaluation.relative_pose import pose_auc, relative_pose_errors, relative_poses
    I = np.concatenate([np.eye(3), [[1.0], [0.0], [0.0]]], 1)
    assert relative_pose_errors(I, I) == (0.0, 0.0)
    Rz = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])    # 90 degrees about z
    P = np.concatenate([Rz, [[-1.0], [0.0], [0.0]]], 1)    # and t -> -t
    r, t = relative_pose_errors(P, I)
    assert abs(r - 90.0) <= 1e-12 and t == 0.0
    P2 = np.concatenate([np.eye(3), [[0.0], [2.0], [0.0]]], 1)
    r, t = relative_pose_errors(np.stack([I, P2]), np.stack([I, I]))
    assert r.tolist() == [0.0, 0.0] and abs(t[1] - 90.0) <= 1e-12 and t[0] == 0.0
    assert relative_pose_errors(np.zeros((3, 4)), I) == (180.0, 90.0)   # no model
    # errors (1, 6, 30): the recall curve runs (0, 0), (1, 1/3), (6, 2/3), (30, 1).
    #   AUC@5:  0.5 * 1 * 1/3 + (5 - 1) * 1/3 = 3/2; / 5 = 0.3
    #   AUC@10: 1/6 + (6 - 1) * (1/3 + 2/3) / 2 + (10 - 6) * 2/3 = 16/3; / 10 = 8/15
    #   AUC@20: 1/6 + 5/2 + (20 - 6) * 2/3 = 12; / 20 = 0.6
    auc = pose_auc([30.0, 1.0, 6.0])
    assert np.abs(auc - [0.3, 8.0 / 15.0, 0.6]).max() <= 1e-15
    assert pose_auc([]).tolist() == [0.0, 0.0, 0.0]
    assert np.abs(pose_auc([0.0, 0.0]) - 1.0).max() <= 1e-15
    # world-to-camera poses -> relative: camera 2 is camera 1 moved by (R, t)
    P1 = np.concatenate([Rz, [[0.5], [1.0], [2.0]]], 1)
    Rrel, trel = _rot(np.array([0.1, -0.2, 0.05])), np.array([0.3, 0.1, -0.2])
    P2w = np.concatenate([Rrel @ P1[:, :3], (Rrel @ P1[:, 3] + trel)[:, None]], 1)
    rel = relative_poses(np.stack([P1, P2w]), [(0, 1)])[0]
    assert np.abs(rel[:, :3] - Rrel).max() <= 1e-15
    assert np.abs(rel[:, 3] - trel / np.linalg.norm(trel)).max() <= 1e-15
