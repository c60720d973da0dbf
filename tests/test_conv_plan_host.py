"""CPU checks of the conv planner (posfeat_amd/csrc/conv_plan.h): the plan
header under the host sanitizers against the plans recorded before it became a
table (tests/golden/conv_plans.txt), and the plan query of the library, which
needs no device."""
import ctypes
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv_plan_under_host_sanitizers(tmp_path):
    """tests/host/conv_plan_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    exe = str(tmp_path / "conv_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "host", "conv_plan_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "conv_plans.txt")],
                       capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "conv_plan ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_conv_plan_query_host_only():
    """posfeat_conv_plan_query plans without a device; a descriptor whose
    n * oh * ow passes INT_MAX is rejected, not wrapped."""
    from posfeat_amd import _lib
    L = _lib.lib()
    assert L.posfeat_abi_version() == 1
    info = _lib.conv_plan_query(2, 16, 24, 256, 64, 1, 1, 0, wplanes=True)
    assert info["tile"] == 30 and info["kernel"] == "(conv_bf6x_kernel<64>)"
    assert info["bm"] == 128 and info["bn"] == 64 and info["block"] == 256
    assert info["grid"] == (2 * 16 * 24 + 127) // 128 and info["ksplit"] == 1 and info["arith"] == 1
    # a forced illegal tile is ignored, a legal one taken
    assert _lib.conv_plan_query(2, 16, 24, 256, 64, 1, 1, 0, wplanes=True, tile=10)["tile"] == 30
    assert _lib.conv_plan_query(2, 16, 24, 256, 64, 1, 1, 0, wplanes=True, tile=35)["tile"] == 35
    # 65536 x 256 x 128 output pixels = 2^31
    assert _lib.conv_plan_query(65536, 256, 128, 64, 64, 1, 1, 0) is None
    assert _lib.conv_plan_query(65535, 256, 128, 64, 64, 1, 1, 0) is not None
    d = _lib.ConvDesc(n=65536, h=256, w=128, cin=64, x_cstride=64, cout=64, kh=1, kw=1, stride=1,
                      pad=0, y_cstride=64, res_cstride=0, act=0)
    assert L.posfeat_conv2d_workspace(ctypes.byref(d)) == 0
