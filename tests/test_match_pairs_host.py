"""CPU checks of the batched matcher and the HPatches evaluation: the ABI's
argument validation (no device work), the plan header under the host
sanitizers, and mma_score / format_row against a numpy restatement of
evaluations/hpatches/evaluation.py:160-179 and 245-257."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_match_pairs_abi_host_only_calls():
    from posfeat_amd import _lib
    L = _lib.lib()
    assert L.posfeat_abi_version() == 1
    set_off, so = _i32([0, 300, 300, 1300, 3349])          # set 1 is empty
    pairs, pp = _i32([[0, 2], [2, 3], [1, 0], [3, 3]])
    need = L.posfeat_match_pairs_workspace(so, 4, pp, 4)
    assert need > 0
    p = ctypes.c_void_p(4096)                              # dummy, non-null, 256-B aligned

    def call(so=so, nsets=4, pp=pp, npairs=4, dim=128, mode=0, ws_bytes=need):
        return L.posfeat_match_pairs(p, so, nsets, pp, npairs, dim, mode, 0.95, p, p, p, ws_bytes,
                                     None)

    _, bad_hi = _i32([[0, 2], [2, 4]])
    _, bad_lo = _i32([[0, 2], [-1, 3]])
    _, dec = _i32([0, 300, 299, 1300, 3349])
    assert call(pp=bad_hi, npairs=2) == -1                 # set index out of range
    assert call(pp=bad_lo, npairs=2) == -1
    assert call(so=dec) == -1                              # decreasing set_off
    assert L.posfeat_match_pairs_workspace(dec, 4, pp, 4) == 0
    assert L.posfeat_match_pairs_workspace(so, 4, bad_hi, 2) == 0
    # sum n1 = 3 x 2^30 does not fit the int32 match offsets
    _, big = _i32([0, 1 << 30])
    _, bigp = _i32([[0, 0]] * 3)
    assert call(so=big, nsets=1, pp=bigp, npairs=3, ws_bytes=1 << 62) == -1
    assert call(dim=64) == -4
    assert call(mode=3) == -4
    assert call(ws_bytes=need - 1) == -3                   # short workspace
    assert call(ws_bytes=0) == -3
    # the plan report: empty-side pair -> 0 ranges; the others at least one
    ns = np.full(8, -1, np.int32)
    assert L.posfeat_match_pairs_splits(so, 4, pp, 4, ctypes.c_void_p(ns.ctypes.data)) == 0
    assert ns[4] == 0 and ns[5] == 0 and all(ns[[0, 1, 2, 3, 6, 7]] >= 1)
    assert L.posfeat_match_pairs_splits(dec, 4, pp, 4, ctypes.c_void_p(ns.ctypes.data)) == -1
    # posfeat_reproj_hist: the same table checks, nthr in 1..32, workspace
    rneed = L.posfeat_reproj_hist_workspace(4)
    assert rneed >= 4 * 32 and L.posfeat_reproj_hist_workspace(0) == 0

    def rcall(so=so, pp=pp, npairs=4, nthr=15, ws_bytes=rneed):
        return L.posfeat_reproj_hist(p, so, 4, pp, npairs, p, p, p, nthr, p, p, ws_bytes, None)

    assert rcall(pp=bad_hi, npairs=2) == -1
    assert rcall(so=dec) == -1
    assert rcall(nthr=0) == -1 and rcall(nthr=33) == -1
    assert rcall(ws_bytes=rneed - 1) == -3


def test_match_plan_under_host_sanitizers(tmp_path):
    """tests/host/match_plan_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "match_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "host", "match_plan_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "match_plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _ref_mma(i_err, v_err, n_i, n_v):
    """evaluation.py:160-179, restated"""
    tmp_a, tmp_i, tmp_v = [], [], []
    for thr in range(1, 11):
        tmp_a.append((i_err[thr] + v_err[thr]) / ((n_i + n_v) * 5))
        tmp_i.append(i_err[thr] / (n_i * 5))
        tmp_v.append(v_err[thr] / (n_v * 5))
    cur_a = cur_i = cur_v = upper_bound = 0
    for idx, (mma_a, mma_i, mma_v) in enumerate(zip(tmp_a, tmp_i, tmp_v)):
        cur_a += (2 - (idx + 1) / 10.) * mma_a
        cur_i += (2 - (idx + 1) / 10.) * mma_i
        cur_v += (2 - (idx + 1) / 10.) * mma_v
        upper_bound += (2 - (idx + 1) / 10.) * 1
    return cur_a / upper_bound, cur_i / upper_bound, cur_v / upper_bound


def test_mma_score_and_format_row():
    from posfeat_amd.evaluation import hpatches as hp
    rs = np.random.RandomState(7)
    n_i, n_v = 3, 4
    rng = np.arange(1, 16)
    # sums of 5 n per-pair fractions, non-decreasing in the threshold
    i_err = dict(zip(rng, np.sort(rs.uniform(0, n_i * 5, 15))))
    v_err = dict(zip(rng, np.sort(rs.uniform(0, n_v * 5, 15))))
    got = hp.mma_score(i_err, v_err, n_i, n_v)
    ref = _ref_mma(i_err, v_err, n_i, n_v)
    assert got == ref                                      # the same fp64 operations
    assert all(0.0 <= g <= 1.0 for g in got)
    ones = {t: float(n_i * 5) for t in rng}, {t: float(n_v * 5) for t in rng}
    np.testing.assert_allclose(hp.mma_score(ones[0], ones[1], n_i, n_v), (1, 1, 1), rtol=1e-15)
    seq_type = np.array(["i"] * (n_i * 5) + ["v"] * (n_v * 5))
    n_feats = rs.randint(200, 9000, size=(n_i + n_v) * 6)
    n_matches = rs.randint(0, 4000, size=(n_i + n_v) * 5)
    stats = [seq_type, n_feats, n_matches]
    assert hp.seq_counts(stats) == (n_i, n_v)
    # evaluation.py:245-257 for one method
    name = "PoSFeat".ljust(25, " ")
    line = "{} & {:.1f} & {:.1f} & {:.3f} & {:.3f} & {:.3f}\n".format(
        name, np.mean(n_feats), np.sum(n_matches) / ((n_i + n_v) * 5), ref[0], ref[1], ref[2])
    assert hp.format_row("PoSFeat", stats, got) == line
    # evaluation.py:98-105
    lines = hp.summary_lines(stats)
    assert lines[0] == "# Features: {:f} - [{:d}, {:d}]".format(np.mean(n_feats), np.min(n_feats),
                                                                np.max(n_feats))
    assert lines[1] == "# Matches: Overall {:f}, Illumination {:f}, Viewpoint {:f}".format(
        np.sum(n_matches) / ((n_i + n_v) * 5), np.sum(n_matches[seq_type == "i"]) / (n_i * 5),
        np.sum(n_matches[seq_type == "v"]) / (n_v * 5))
