"""CPU checks of the batched RANSAC stage (ransac.hip / ransac_plan.h): the
sampler against the numpy restatement (tests/ransac_ref.py), the ABI's
argument validation (no device work) and the pure header under the host
sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import ransac_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 1, 0x123456789ABCDEF0, (1 << 64) - 1)


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 8192, 60000])
def test_sampler_equals_restatement(n):
    from posfeat_amd import geometry
    for seed in SEEDS:
        for pair in (0, 99):
            for it in range(256):
                got = geometry.sample_indices(seed, pair, it, n)
                assert got.dtype == np.int32 and got.tolist() == R.sample(seed, pair, it, n), \
                    (seed, pair, it, n)
                assert len(set(got.tolist())) == 4 and got.min() >= 0 and got.max() < n
                if n == 4:
                    assert sorted(got.tolist()) == [0, 1, 2, 3]


def test_sampler_coverage_and_pinned_values():
    from posfeat_amd import geometry
    hit = np.zeros(64, int)
    for it in range(4096):
        hit[geometry.sample_indices(7, 3, it, 64)] += 1
    assert hit.min() > 0 and hit.sum() == 4 * 4096
    # each position is close to uniform: 256 expected per index and position
    assert hit.max() < 2 * hit.min()
    assert R.mix(0) == 0xE220A8397B1DCDAF                  # splitmix64, first output of seed 0
    assert geometry.sample_indices(0, 0, 0, 4).tolist() == [0, 1, 2, 3]
    assert geometry.sample_indices(0, 0, 1, 5).tolist() == [4, 0, 1, 3]
    assert geometry.sample_indices(0, 0, 0, 8192).tolist() == [1062, 1354, 2545, 3379]
    assert geometry.sample_indices(12345, 99, 7, 65).tolist() == [29, 63, 13, 50]
    assert geometry.sample_indices((1 << 64) - 1, 99, 255, 60000).tolist() == \
        [9431, 11640, 2747, 31281]
    for n in (3, 0, -1):
        with pytest.raises(ValueError):
            geometry.sample_indices(0, 0, 0, n)


def test_ransac_abi_host_only_calls():
    from posfeat_amd import _lib
    L = _lib.lib()
    assert L.posfeat_abi_version() == 1
    out, op = _i32([0, 0, 0, 0])
    assert L.posfeat_ransac_sample(0, 0, 0, 3, op) == -1
    assert L.posfeat_ransac_sample(0, 0, 0, 4, None) == -1
    assert L.posfeat_ransac_sample(0, 0, 0, 4, op) == 0 and sorted(out.tolist()) == [0, 1, 2, 3]
    set_off, so = _i32([0, 300, 300, 1300, 3349])          # set 1 is empty
    pairs, pp = _i32([[0, 2], [2, 3], [1, 0], [3, 3]])
    need = L.posfeat_ransac_homography_workspace(so, 4, pp, 4, 256)
    # at least the gathered rows (16 B per match row) and the block slots
    assert need >= 16 * (300 + 1000 + 0 + 2049) + 8 * 4
    assert L.posfeat_ransac_homography_workspace(so, 4, pp, 4, 65536) > need
    p = ctypes.c_void_p(4096)                              # dummy, non-null, 256-B aligned

    def call(kp=p, so=so, nsets=4, pp=pp, npairs=4, matches=p, counts=p, iters=256, thr=3.0,
             H=p, info=p, inlier=p, ws=p, ws_bytes=need):
        return L.posfeat_ransac_homography(kp, so, nsets, pp, npairs, matches, counts, iters, thr,
                                           0, H, info, inlier, ws, ws_bytes, None)

    for name in ("kp", "so", "pp", "matches", "counts", "H", "info", "inlier", "ws"):
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
        assert L.posfeat_ransac_homography_workspace(so, 4, pp, 4, iters) == 0
    assert call(iters=65536) == -3                         # a legal count: only the workspace is short
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    # sum n1 = 3 x 2^30 does not fit the int32 match offsets
    _, big = _i32([0, 1 << 30])
    _, bigp = _i32([[0, 0]] * 3)
    assert call(so=big, nsets=1, pp=bigp, npairs=3, ws_bytes=1 << 62) == -1
    assert L.posfeat_ransac_homography_workspace(big, 1, bigp, 3, 256) == 0
    assert call(ws_bytes=need - 1) == -3                   # short workspace
    assert call(ws_bytes=0) == -3
    assert L.posfeat_ransac_homography_workspace(dec, 4, pp, 4, 256) == 0
    assert L.posfeat_ransac_homography_workspace(so, 4, bad_hi, 2, 256) == 0
    assert L.posfeat_ransac_homography_workspace(None, 4, pp, 4, 256) == 0


def test_ransac_plan_under_host_sanitizers(tmp_path):
    """tests/host/ransac_plan_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "ransac_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "host", "ransac_plan_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "ransac_plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_restatement_recovers_a_planted_homography():
    """the restatement itself on a small planted case (no device)"""
    rs = np.random.RandomState(3)
    H = np.array([[1.02, 0.03, 5.0], [-0.02, 0.98, -3.0], [2e-5, -1e-5, 1.0]])
    a = (rs.uniform(0, 1, (60, 2)) * [640, 480]).astype(np.float32)
    b = R.warp(H, a.astype(np.float64))
    b[40:] += rs.uniform(30, 300, (20, 2))
    m = np.concatenate([a, b.astype(np.float32)], 1)
    out = R.ransac(m, 0, 64, 3.0, 5)
    assert out["status"] == 0 and out["n_inliers"] == 40 and out["mask"][:40].all()
    assert not out["mask"][40:].any()
    assert R.corner_error(out["H"], H, 640, 480) <= 1e-3
    assert abs(np.sqrt((out["H"] ** 2).sum()) - 1) < 1e-15 and out["H"][2, 2] >= 0
    assert R.ransac(m[:3], 0, 64, 3.0, 5)["status"] == 1
