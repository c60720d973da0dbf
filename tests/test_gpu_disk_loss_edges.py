"""DiskLoss kernels (posfeat_amd/csrc/disk.hip) against a float64 reference at
the tile, split and acceptance edges, through the C ABI.

Every branch of the two flash kernels (disk_flash_kernel: fp32 MFMA, 64-row
steps; disk_flash6_kernel: bf16x6, a ring of 32-row stages), of the stable
compaction, the gather of accepted points, the split merges, the per-cell
point kernel and the gradient kernel depends on how the cell count n, the
per-image accepted counts and the row split fall against FCOLS = 128,
FSTEP = 64 and F6STEP = 32.  tests/disk_fixture.py holds the shape table (n
from 4 to 320, each row named for the edge it reaches and the split plan it
must take), the acceptance patterns (half, all, none, exact counts 31 .. 129
around the stage / step / column-block sizes, a batch whose images differ),
peaky descriptors, extreme score maps, NaN-padded channel strides and
non-default scalars, each with its reference from the torch oracle in
float64.  Every case runs at conv precision 0 (fp32 MFMA) and 1 (bf16x6).

Tolerances, measured on an MI355X as the largest ratio over all cases against
the float64 reference (printed by each test; C_LOSS / C_GRAD are 4x the
maximum over both precisions, to cover seed-to-seed variation, and stay below
the 2e-4 / 1e-4 this loss is held to elsewhere):

  |loss terms - ref| / bound      precision 0: 2.10e-6   precision 1: 1.88e-6
  max|dkp - ref| / max|ref|       precision 0: 3.19e-6   precision 1: 8.45e-6

(the float32 torch oracle itself: 5.7e-7 and 6.9e-6, test_oracle_disk_dtype.py)

posfeat_disk_flash_lse is compared with torch.logsumexp in float64 for n from
1 to 333 within T 128 2^-24 + 1e-5 (4.6e-4 at T = 60): the worst-case fp32
dot-product error of unit vectors (128 terms, unit roundoff 2^-24) times T,
plus exp / log rounding.  Measured maxima: 3.5e-5 at T = 60, 1.2e-4 at
T = 200 (precision 0, peaky; precision 1 is slightly below).  The in-kernel sampler is
compared exactly: the kernel in sampled mode against itself replaying the
float64 Gumbel-max / Bernoulli draws made from the same uniforms."""
import numpy as np
import pytest
import torch

import disk_fixture as DF

pytestmark = pytest.mark.gpu

C_LOSS = 4 * 2.099e-6   # 8.4e-6 (cap: 2e-4, test_disk_loss_vs_reference)
C_GRAD = 4 * 8.453e-6   # 3.4e-5 (cap: 1e-4)
assert C_LOSS <= 2e-4 and C_GRAD <= 1e-4
SENTINEL = -777.25

OK, E_INVALID, E_WORKSPACE, E_UNSUPPORTED = 0, -1, -3, -4


@pytest.fixture
def precision():
    from posfeat_amd._lib import lib
    prev = lib().posfeat_set_conv_precision(1)
    yield lambda m: lib().posfeat_set_conv_precision(m)
    lib().posfeat_set_conv_precision(prev)


def _device_inputs(c, dev):
    b, n = c["b"], c["n"]
    return dict(
        kp1=c["kp1"][:, 0].contiguous().to(dev), kp2=c["kp2"][:, 0].contiguous().to(dev),
        xf1=DF.nhwc_padded(c["xf1"], c["cs"][0]).to(dev),
        xf2=DF.nhwc_padded(c["xf2"], c["cs"][1]).to(dev),
        F1=c["F1"].contiguous().to(dev), F2=c["F2"].contiguous().to(dev),
        prop1=c["prop1"].reshape(b, n).int().contiguous().to(dev),
        prop2=c["prop2"].reshape(b, n).int().contiguous().to(dev),
        acc1=c["acc1"].reshape(b, n).to(torch.uint8).contiguous().to(dev),
        acc2=c["acc2"].reshape(b, n).to(torch.uint8).contiguous().to(dev),
        uni1=c["uni1"].contiguous().to(dev) if "uni1" in c else None,
        uni2=c["uni2"].contiguous().to(dev) if "uni2" in c else None)


def _call(c, d, dev, grad=True, draws="replay", ws_short=0, cs=None, hw=None):
    """One call of posfeat_disk_loss[_grad] with sentinel-filled outputs:
    (status, out[4], dkp1, dkp2) on the host."""
    from posfeat_amd._lib import lib, ptr, stream_ptr
    L = lib()
    b = c["b"]
    H, W = hw or (c["H"], c["W"])
    s = c["scalars"]
    cs1, cs2 = cs or c["cs"]
    out = torch.full((4,), SENTINEL, device=dev)
    d1 = torch.full_like(d["kp1"], SENTINEL)
    d2 = torch.full_like(d["kp2"], SENTINEL)
    need = (L.posfeat_disk_loss_grad_workspace if grad else L.posfeat_disk_loss_workspace)(b, H, W)
    ws = torch.empty(max(need, 1024), dtype=torch.uint8, device=dev)
    pr = [d["prop1"], d["prop2"], d["acc1"], d["acc2"]] if draws == "replay" else [None] * 4
    un = [d["uni1"], d["uni2"]] if draws == "sampled" else [None, None]
    head = [ptr(d["kp1"]), ptr(d["kp2"]), ptr(d["xf1"]), cs1, ptr(d["xf2"]), cs2, b, H, W,
            ptr(d["F1"]), ptr(d["F2"])] + [ptr(t) for t in pr + un] + \
        [s["T"], s["reward_thr"], s["good"], s["bad"], s["kp_penalty"], ptr(out)]
    tail = [ptr(ws), need - ws_short if ws_short else max(need, 1024), stream_ptr()]
    if grad:
        st = L.posfeat_disk_loss_grad(*(head + [ptr(d1), ptr(d2)] + tail))
    else:
        st = L.posfeat_disk_loss(*(head + tail))
    torch.cuda.synchronize()
    return st, out.cpu(), d1.cpu(), d2.cpu()


def _pixel_mask(acc, H, W):
    """[b,1,H/8,W/8] cell flags -> [b,H,W] pixel flags."""
    return acc[:, 0].repeat_interleave(8, 1).repeat_interleave(8, 2)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("name", list(DF.CASES))
def test_disk_loss_vs_fp64(gpu, precision, name, prec):
    c = DF.case(name)
    ref = c["ref"]
    b, n, H, W = c["b"], c["n"], c["H"], c["W"]
    if name in DF.PLANS:
        from posfeat_amd import _lib
        assert _lib.disk_flash_plan(b, n) == DF.PLANS[name]
    a1n = c["acc1"].reshape(b, n).sum(1)
    a2n = c["acc2"].reshape(b, n).sum(1)
    if name == "n320":  # the second split: empty in the SUM passes, live in the LSE passes
        assert int(a1n.max()) < 192 and int(a2n.max()) < 192
    if name == "b3n72":
        assert a1n.tolist()[0] == n and a1n.tolist()[1:] == [0, 1]
        assert a2n.tolist()[0] == n and 0 < a2n.tolist()[1] < n and a2n.tolist()[2] == 1
    precision(prec)
    d = _device_inputs(c, gpu)
    st, out, d1, d2 = _call(c, d, gpu)
    assert st == OK
    assert torch.isfinite(out).all() and torch.isfinite(d1).all() and torch.isfinite(d2).all()
    # n_kps exact; loss terms within C_LOSS of the summed magnitude
    assert out[3].item() == np.float32(ref["n_kps"])
    want = (ref["loss"], ref["reinforce"], ref["penalty"])
    errs = [abs(out[i].item() - want[i]) for i in range(3)]
    print("disk-edges %s prec %d loss-ratio %.3e" % (name, prec,
                                                    max(errs) / max(ref["bound"], 1e-30)))
    if c["acc1"].sum() == 0 and c["acc2"].sum() == 0:
        assert ref["loss"] == 0 and out[:3].tolist() == [0.0, 0.0, 0.0]
    # gradients per side and image
    gratio = 0.0
    gerr = []
    for got, rf, acc in ((d1, ref["dkp1"], c["acc1"]), (d2, ref["dkp2"], c["acc2"])):
        rej = ~_pixel_mask(acc, H, W)
        assert (rf[rej] == 0).all()       # the reference first
        assert (got[rej] == 0).all(), "gradient on a rejected cell"
        for i in range(b):
            scale = float(rf[i].abs().max())
            if scale == 0:
                assert (got[i] == 0).all()
                continue
            err = float((got[i].double() - rf[i]).abs().max())
            gratio = max(gratio, err / scale)
            gerr.append((err, scale))
    print("disk-edges %s prec %d grad-ratio %.3e" % (name, prec, gratio))
    for i in range(3):
        assert errs[i] <= C_LOSS * ref["bound"] + 1e-6, (i, errs[i], ref["bound"])
    for err, scale in gerr:
        assert err <= C_GRAD * scale, (err, scale)
    # the forward-only entry: the same four numbers bit for bit
    stf, outf, s1, s2 = _call(c, d, gpu, grad=False)
    assert stf == OK and torch.equal(outf, out)
    assert (s1 == SENTINEL).all() and (s2 == SENTINEL).all()
    # determinism
    st2, out2, e1, e2 = _call(c, d, gpu)
    assert st2 == OK and torch.equal(out2, out) and torch.equal(e1, d1) and torch.equal(e2, d2)


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("shape", list(DF.SAMPLER_SEEDS))
def test_disk_sampler_matches_fp64_draws(gpu, precision, shape, prec):
    """Sampled mode (Gumbel-max + Bernoulli from uniforms in disk_point_kernel)
    against replay mode with the float64 draws from the same uniforms: after
    disk_point_kernel the two runs are the same code, so every output is
    bit-identical iff the kernel drew what the reference drew.  One crafted
    cell has constant logits and constant uniforms: all keys tie and the
    proposal must be pixel 0."""
    c = DF.sampler_case(shape)
    b, n = c["b"], c["n"]
    assert int(c["prop1"].reshape(b, n)[c["crafted"]]) == 0
    precision(prec)
    d = _device_inputs(c, gpu)
    st_s, out_s, s1, s2 = _call(c, d, gpu, draws="sampled")
    st_r, out_r, r1, r2 = _call(c, d, gpu, draws="replay")
    assert st_s == OK and st_r == OK
    assert torch.isfinite(out_s).all() and torch.isfinite(s1).all() and torch.isfinite(s2).all()
    assert out_r[3].item() == np.float32((int(c["acc1"].sum()) + int(c["acc2"].sum())) / b)
    assert torch.equal(out_s, out_r)
    assert torch.equal(s1, r1) and torch.equal(s2, r2)


LSE_NS = (1, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 320, 333)


def _lse_inputs(n, b, mode, seed):
    g = torch.Generator().manual_seed(seed)
    fa = torch.nn.functional.normalize(torch.randn(b, n, 128, generator=g), dim=-1)
    if mode == "peaky":  # row i of fb next to row i of fa: each column's lse is one sharp term
        fb = fa + 0.02 * torch.randn(b, n, 128, generator=g)
    else:
        fb = torch.randn(b, n, 128, generator=g)
    return fa.contiguous(), torch.nn.functional.normalize(fb, dim=-1).contiguous()


@pytest.mark.parametrize("prec", [0, 1])
@pytest.mark.parametrize("T", [60.0, 200.0])
@pytest.mark.parametrize("mode", ["random", "peaky"])
def test_disk_flash_lse_vs_fp64(gpu, precision, mode, T, prec):
    """lse[b][j] = logsumexp_i(T <fa_i, fb_j> - T) for every n around the stage,
    step, column-block and split sizes.  A dropped or doubled row moves a
    peaky column's lse by up to log 2, far outside the bound."""
    from posfeat_amd import _lib
    from posfeat_amd._lib import lib, ptr, stream_ptr
    L = lib()
    assert _lib.disk_flash_plan(1, 256) == (2, 128) and _lib.disk_flash_plan(1, 320) == (2, 192)
    precision(prec)
    bound = T * 128 * 2.0 ** -24 + 1e-5
    worst = 0.0
    for n in LSE_NS:
        for b in (1, 2):
            fa, fb = _lse_inputs(n, b, mode, 100 * n + b)
            ref = torch.logsumexp(T * (fa.double() @ fb.double().transpose(1, 2) - 1), dim=1)
            need = L.posfeat_disk_flash_lse_workspace(b, n)
            ws = torch.empty(need, dtype=torch.uint8, device=gpu)
            lse = torch.full((b, n), SENTINEL, device=gpu)
            fag, fbg = fa.to(gpu), fb.to(gpu)
            st = L.posfeat_disk_flash_lse(ptr(fag), ptr(fbg), b, n, T, ptr(lse), ptr(ws), need,
                                          stream_ptr())
            torch.cuda.synchronize()
            assert st == OK
            got = lse.cpu()
            assert torch.isfinite(got).all(), (n, b)
            err = float((got.double() - ref).abs().max())
            worst = max(worst, err)
            assert err <= bound, (n, b, err, bound)
    print("disk-edges lse %s T %g prec %d max|dlse| %.3e (bound %.3e)" % (mode, T, prec, worst,
                                                                        bound))


@pytest.mark.parametrize("grad", [True, False])
def test_disk_loss_rejections(gpu, grad):
    """Arguments the entry points refuse: the status, and nothing written."""
    def untouched(r):
        st, out, d1, d2 = r
        assert (out == SENTINEL).all() and (d1 == SENTINEL).all() and (d2 == SENTINEL).all()
        return st

    c = DF.case("n36")
    d = _device_inputs(c, gpu)
    assert untouched(_call(c, d, gpu, grad=grad, cs=(64, 128))) == E_INVALID
    assert untouched(_call(c, d, gpu, grad=grad, ws_short=1)) == E_WORKSPACE
    assert untouched(_call(c, d, gpu, grad=grad, draws="none")) == E_INVALID
    # H % 8 != 0 (buffers of the 48 x 48 case: nothing is read before the refusal)
    assert untouched(_call(c, d, gpu, grad=grad, hw=(20, 16))) == E_INVALID
    # n = 3: not a multiple of 4
    assert untouched(_call(c, d, gpu, grad=grad, hw=(24, 8))) == E_UNSUPPORTED
