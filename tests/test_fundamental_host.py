"""CPU checks of the batched fundamental-matrix stage (fundamental.hip /
fundamental_solve.h / ransac_plan.h): the seven-draw sampler against the numpy
restatement (tests/fundamental_ref.py), the 7-point solver against an
independent computation (SVD null space, np.roots), the ABI's argument
validation (no device work), the pure headers under the host sanitizers, and
the restatement itself on a planted scene."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import fundamental_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 0x123456789ABCDEF0, (1 << 64) - 1)          # those of test_ransac_host.py
K_CAM = np.array([[500.0, 0, 320], [0, 500, 240], [0, 0, 1]])


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("n", [7, 8, 63, 64, 65, 8192])
def test_sampler7_equals_restatement(n):
    from posfeat_amd import geometry
    for seed in SEEDS:
        for pair in (0, 99):
            for it in range(256):
                got = geometry.sample_indices(seed, pair, it, n, k=7)
                assert got.dtype == np.int32 and got.tolist() == FR.sample(seed, pair, it, n, 7), \
                    (seed, pair, it, n)
                assert got[:4].tolist() == geometry.sample_indices(seed, pair, it, n).tolist()
                assert len(set(got.tolist())) == 7 and got.min() >= 0 and got.max() < n
                if n == 7:
                    assert sorted(got.tolist()) == list(range(7))


def test_sampler_k_range_and_errors():
    from posfeat_amd import geometry
    for k in (4, 5, 6, 7, 8):
        got = geometry.sample_indices(12345, 99, 7, 65, k=k)
        assert got.shape == (k,) and got.tolist() == FR.sample(12345, 99, 7, 65, k)
    assert geometry.sample_indices(12345, 99, 7, 65).tolist() == [29, 63, 13, 50]   # k = 4 as before
    for n, k in ((6, 7), (3, 4), (7, 8), (0, 7), (-1, 7), (100, 3), (100, 9)):
        with pytest.raises(ValueError):
            geometry.sample_indices(0, 0, 0, n, k=k)


def _scene(rs, kind, n=7):
    """n matches (x, y, u, v) in pixels of random 3-D points in front of two
    cameras: general motion, pure forward translation or pure sideways
    translation"""
    X = np.stack([rs.uniform(-2, 2, n), rs.uniform(-1.5, 1.5, n), rs.uniform(3, 9, n)], 1)
    if kind == "general":
        ax = rs.uniform(-0.08, 0.08, 3)
        th = np.linalg.norm(ax)
        k = ax / th
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
        t = np.array([rs.uniform(0.3, 0.8), rs.uniform(-0.2, 0.2), rs.uniform(0.2, 0.6)])
    elif kind == "forward":
        R, t = np.eye(3), np.array([0.0, 0.0, rs.uniform(0.4, 1.0)])
    else:
        R, t = np.eye(3), np.array([rs.uniform(0.4, 1.0), rs.uniform(-0.3, 0.3), 0.0])
    p1 = X @ K_CAM.T
    p2 = (X @ R.T + t) @ K_CAM.T
    return np.concatenate([p1[:, :2] / p1[:, 2:], p2[:, :2] / p2[:, 2:]], 1)


def _normalised(m):
    nm = (FR.normalisation(m[:, :2]), FR.normalisation(m[:, 2:4]))
    return FR.normalise(m, nm)


def _independent(mn):
    """the candidates by a computation that shares none of the defined steps:
    SVD null space, the cubic interpolated from four determinants, np.roots.
    Returns (unit-norm sign-fixed candidates [c, 9], relative root separation)."""
    A = FR.system(mn)
    _, _, vt = np.linalg.svd(A)
    g1, g2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
    xs = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(x * g1 + (1 - x) * g2) for x in xs])
    co = np.linalg.solve(np.vander(xs, 4), dets)             # highest power first
    r = np.roots(co)
    sep = min(abs(r[i] - r[j]) for i in range(3) for j in range(i)) / max(1.0, np.abs(r).max())
    real = np.sort(r[np.abs(r.imag) <= 1e-9 * np.maximum(1.0, np.abs(r))].real)
    return np.array([FR.unit(l * g1 + (1 - l) * g2).reshape(-1) for l in real]), float(sep)


def _set_distance(a, b):
    """largest distance from a member of one set to the nearest of the other.
    Members are compared up to sign: a pure translation gives F12 = -F21 as the
    two largest entries, so which of them the sign rule makes positive is decided
    by the last bit (the rule itself is asserted on every candidate)."""
    d = np.minimum(np.abs(a[:, None, :] - b[None, :, :]).max(2),
                   np.abs(a[:, None, :] + b[None, :, :]).max(2))
    return float(max(d.min(1).max(), d.min(0).max()))


def test_solve7_against_an_independent_method():
    from posfeat_amd import geometry
    rs = np.random.RandomState(2024)
    worst_lib, worst_ref, used = 0.0, 0.0, 0
    for trial in range(90):
        kind = ("general", "forward", "sideways")[trial % 3]
        mn = _normalised(_scene(rs, kind))
        ind, sep = _independent(mn)
        if sep < 1e-3:                                     # the sets are compared only when the
            continue                                       # roots are well apart
        used += 1
        got = geometry.solve7(mn).reshape(-1, 9)
        ref = np.array([FR.unit(F).reshape(-1) for F in FR.solve7(mn)[0]])
        assert len(got) == len(ind) == len(ref) and len(got) in (1, 3), (trial, kind)
        # the disagreement of the two CPU methods between themselves sets the bound
        d_ref = _set_distance(ref, ind)
        d_lib = _set_distance(got, ind)
        worst_ref, worst_lib = max(worst_ref, d_ref), max(worst_lib, d_lib)
        for F in got:
            assert abs(np.sqrt((F ** 2).sum()) - 1.0) <= 1e-14
            assert F[int(np.argmax(np.abs(F)))] > 0
            assert abs(np.linalg.det(F.reshape(3, 3))) <= 1e-12
            assert np.abs(FR.system(mn) @ F).max() <= 1e-10
    print("solve7 vs SVD + np.roots: library %.3g, restatement %.3g over %d samples"
          % (worst_lib, worst_ref, used))
    assert used >= 60
    # the bound: what the two CPU methods disagree by between themselves, times 100
    assert worst_lib <= 100 * worst_ref, (worst_lib, worst_ref)
    # a repeated point: the null space has three dimensions, the sample is rejected
    mn = _normalised(_scene(rs, "general"))
    mn[5] = mn[2]
    assert geometry.solve7(mn).shape == (0, 3, 3) and FR.solve7(mn)[0] == []
    with pytest.raises(ValueError):
        geometry.solve7(np.zeros((6, 4)))


def test_fundamental_abi_host_only_calls():
    from posfeat_amd import _lib
    L = _lib.lib()
    assert L.posfeat_abi_version() == 1
    out, op = _i32([0] * 8)
    assert L.posfeat_ransac_sample_k(0, 0, 0, 6, 7, op) == -1
    assert L.posfeat_ransac_sample_k(0, 0, 0, 7, 7, None) == -1
    assert L.posfeat_ransac_sample_k(0, 0, 0, 100, 3, op) == -1
    assert L.posfeat_ransac_sample_k(0, 0, 0, 100, 9, op) == -1
    assert L.posfeat_ransac_sample_k(0, 0, 0, 7, 7, op) == 0
    assert sorted(out[:7].tolist()) == list(range(7)) and out[7] == 0
    assert L.posfeat_fundamental_solve7(None, op) == -1
    set_off, so = _i32([0, 300, 300, 1300, 3349])          # set 1 is empty
    pairs, pp = _i32([[0, 2], [2, 3], [1, 0], [3, 3]])
    need = L.posfeat_ransac_fundamental_workspace(so, 4, pp, 4, 256)
    assert need >= 16 * (300 + 1000 + 0 + 2049) + 8 * 4
    assert L.posfeat_ransac_fundamental_workspace(so, 4, pp, 4, 65536) > need
    p = ctypes.c_void_p(4096)                              # dummy, non-null, 256-B aligned

    def call(kp=p, so=so, nsets=4, pp=pp, npairs=4, matches=p, counts=p, iters=256, thr=3.0,
             F=p, info=p, inlier=p, ws=p, ws_bytes=need):
        return L.posfeat_ransac_fundamental(kp, so, nsets, pp, npairs, matches, counts, iters, thr,
                                            0, F, info, inlier, ws, ws_bytes, None)

    for name in ("kp", "so", "pp", "matches", "counts", "F", "info", "inlier", "ws"):
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
        assert L.posfeat_ransac_fundamental_workspace(so, 4, pp, 4, iters) == 0
    assert call(iters=65536) == -3                         # a legal count: only the workspace is short
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    # sum n1 = 3 x 2^30 does not fit the int32 match offsets
    _, big = _i32([0, 1 << 30])
    _, bigp = _i32([[0, 0]] * 3)
    assert call(so=big, nsets=1, pp=bigp, npairs=3, ws_bytes=1 << 62) == -1
    assert L.posfeat_ransac_fundamental_workspace(big, 1, bigp, 3, 256) == 0
    assert call(ws_bytes=need - 1) == -3                   # short workspace
    assert call(ws_bytes=0) == -3
    assert L.posfeat_ransac_fundamental_workspace(dec, 4, pp, 4, 256) == 0
    assert L.posfeat_ransac_fundamental_workspace(so, 4, bad_hi, 2, 256) == 0
    assert L.posfeat_ransac_fundamental_workspace(None, 4, pp, 4, 256) == 0


def test_fundamental_solve_under_host_sanitizers(tmp_path):
    """tests/host/fundamental_solve_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "fundamental_solve_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "fundamental_solve_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "fundamental_solve ok" in r.stdout, \
        r.stdout[-2000:] + r.stderr[-4000:]


def test_restatement_recovers_a_planted_fundamental_matrix():
    """the restatement itself on a 60-match scene (no device)"""
    rs = np.random.RandomState(5)
    m = _scene(rs, "general", 60)
    m[40:, 2:] += rs.uniform(30, 200, (20, 2)) * rs.choice([-1, 1], (20, 2))
    m = m.astype(np.float32)
    out = FR.ransac(m, 0, 128, 3.0, 5)
    assert out["status"] == 0 and out["mask"][:40].all() and 40 <= out["n_inliers"] <= 43
    F = out["F"]
    assert abs(np.sqrt((F ** 2).sum()) - 1) < 1e-15 and F.reshape(-1)[np.argmax(np.abs(F))] > 0
    assert abs(np.linalg.det(F)) <= 1e-12
    exact = _scene(np.random.RandomState(5), "general", 60)[:40]
    assert FR.sampson(F, exact).max() <= 1e-3               # fp32 keypoint rounding
    assert FR.ransac(m[:6], 0, 64, 3.0, 5)["status"] == 1
