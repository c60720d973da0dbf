"""Every legal conv tile (POSFEAT_CONV_TILE, one child process each) on the
stem, 1x1, strided 1x1, 3x3 s1 / s2 and a B=32 layer1-scale 1x1: three
repeated launches must be BIT-equal and within 1e-5 of Sum|x||w| of the fp64
conv (tools/tile_sweep.py).  This is the regression test of the stale-operand
race of round 2 (an inline-asm v_cvt_pk_bf16_f32 whose VGPR write the
compiler's hazard recognizer could not see, so MFMAs read the register's old
value when scheduled right behind it: conv_glds_kernel<128,64,..,BF6> and the
bf16x6 stem variant); tools/isa_check.py checks the ISA for
the hazard itself."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_every_tile_repeatable_and_accurate():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tile_sweep.py")],
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]


def _fixture_tile(shape, precision):
    """The tile tests/golden/conv_plans.txt records for a conv shape (with
    weight planes, no forced tile, no split) at the default mode."""
    want_s = " ".join(str(v) for v in shape)
    default = [str(precision)] + "0 0 0 1 2 1 1 4 2 -1 0 0 0 0 0 0 3".split()
    sid = mid = None
    star, named, inblock = None, None, False
    tiles = {}
    for ln in open(os.path.join(ROOT, "tests", "golden", "conv_plans.txt")):
        f = ln.split("#")[0].split()
        if not f:
            continue
        if f[0] == "S" and " ".join(f[2:]) == want_s:
            sid = f[1]
        elif f[0] == "M" and f[2:] == default:
            mid = f[1]
        elif f[0] == "R":
            tiles[f[1]] = int(f[3])
        elif f[0] == "B":
            inblock = sid in f[1].split(",")
        elif f[0] == "C" and inblock:
            if f[1] == "*":
                star = f[2]
            elif mid in f[1].split(",") or mid + ".0" in f[1].split(","):
                named = f[2]
    assert sid is not None and mid is not None and star is not None
    return tiles[named if named is not None else star]


@pytest.mark.parametrize("n,h,w,cin,cout,k,stride", [(2, 16, 24, 256, 64, 1, 1),
                                                     (2, 16, 32, 128, 128, 3, 1),
                                                     (2, 32, 48, 4, 64, 7, 2)])
def test_queried_plan_is_the_launched_one(n, h, w, cin, cout, k, stride):
    """posfeat_conv_plan_query names the tile the fixture recorded for the
    shape, and the conv run three times (and once with that tile forced) is
    bit-equal."""
    import torch
    from posfeat_amd import _lib, ops
    pad = k // 2
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    kpad = ops.packed_k(cin, k, k)
    precision = _lib.lib().posfeat_set_conv_precision(-1)
    info = _lib.conv_plan_query(n, h, w, cin, cout, k, stride, pad, wplanes=True)
    shape = (n * oh * ow, oh * ow, oh, ow, cin, cin, cout, k, k, stride, pad, kpad, 1, 0, 0, 0)
    assert info["tile"] == _fixture_tile(shape, precision)
    g = torch.Generator(device="cuda").manual_seed(k)
    x = torch.randn(n, h, w, cin, device="cuda", generator=g)
    wt = torch.randn(cout, cin if cin % 32 == 0 else 3, k, k, device="cuda", generator=g) * 0.05
    wp, bias = ops.pack_conv_weight(wt)
    planes = ops.split_weight_planes(wp)
    ys = [ops.conv2d_nhwc_planes(x, wp, planes, bias, cout, k, k, stride=stride, pad=pad)
          for _ in range(3)]
    ys.append(ops.conv2d_nhwc_planes(x, wp, planes, bias, cout, k, k, stride=stride, pad=pad,
                                     tile=info["tile"]))
    assert bool(torch.isfinite(ys[0]).all()) and float(ys[0].abs().max()) > 0
    for y in ys[1:]:
        assert torch.equal(ys[0], y)
