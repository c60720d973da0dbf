"""The DiskLoss oracle follows the dtype of its maps (CPU only).

oracle.correlation_ref.disk_loss and oracle.train_ref.disk_loss_autograd run
in float32 (as the reference does; pinned bit-for-bit by the golden tests) and
in float64 (the reference the HIP kernels are compared with in
test_gpu_disk_loss_edges.py).  Here the two runs are compared on the shape
table of tests/disk_fixture.py, and the float64 run against the reference's own
golden loss.

Bounds: the float32 run is held to the tolerances the project uses for this
loss on the GPU -- 2e-4 of ``bound`` (sum |reward p (logp terms)| + |penalty|,
the magnitude the loss is summed from) for the loss terms, 1e-4 of max|grad|
for the score-map gradients.  A float32 evaluation of this loss carries a few
1e-5 (T = 60 times the 128-term cosine rounding, through exp), so both have an
order of magnitude of room; every case keeps its accepted pairs >= 1e-3 px
from the reward step, so no reward differs between the two runs."""
import os

import numpy as np
import pytest
import torch

import disk_fixture as DF
from conftest import GOLDEN

TABLE_CASES = [name for name, _, _, _ in DF.TABLE]


@pytest.mark.parametrize("name", TABLE_CASES)
def test_oracle_fp32_matches_fp64(name):
    c = DF.case(name)
    ref = c["ref"]
    loss, d1, d2, comp = DF.oracle_run(c, torch.float32)
    assert loss.dtype == torch.float32 and d1.dtype == torch.float32
    tol = 2e-4 * ref["bound"] + 1e-6
    errs = {"loss": abs(float(loss) - ref["loss"]),
            "reinforce": abs(float(comp["reinforce"]) - ref["reinforce"]),
            "penalty": abs(float(comp["kp_penalty"]) - ref["penalty"])}
    print(name, {k: "%.3g" % (v / max(ref["bound"], 1e-30)) for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= tol, (k, v, tol)
    assert float(comp["n_kps"]) == ref["n_kps"]
    for got, want in ((d1[:, 0], ref["dkp1"]), (d2[:, 0], ref["dkp2"])):
        scale = float(want.abs().max())
        err = float((got.double() - want).abs().max())
        print(name, "grad err / max|grad| %.3g" % (err / max(scale, 1e-30)))
        assert err <= 1e-4 * scale


def test_oracle_fp64_matches_golden_loss():
    from test_oracle_correlation import _inputs
    d = np.load(os.path.join(GOLDEN, "correlation.npz"))
    b, H, W, xf1, xf2, kp1, kp2, F1, F2 = _inputs("s")
    g = lambda k: torch.from_numpy(d["s_" + k])  # noqa: E731
    from oracle import correlation_ref as cr
    loss, comp = cr.disk_loss(kp1.double(), kp2.double(), xf1.double(), xf2.double(), F1.double(),
                              F2.double(), g("prop1").long(), g("prop2").long(), g("acc1"),
                              g("acc2"))
    assert loss.dtype == torch.float64
    np.testing.assert_allclose(loss.numpy(), d["s_disk_loss"], rtol=2e-4)


def test_disk_flash_plan_query_host_only():
    """posfeat_disk_flash_plan plans without a device.  Each shape row of the
    table is there for the split it takes: if the heuristic is retuned, this
    says the edge is no longer covered."""
    from posfeat_amd import _lib
    assert set(DF.PLANS) == set(TABLE_CASES)
    for name, (b, H, W) in DF.SHAPES.items():
        assert _lib.disk_flash_plan(b, (H // 8) * (W // 8)) == DF.PLANS[name], name
    for b in (1, 2):  # the stand-alone LSE pass's split sizes
        assert _lib.disk_flash_plan(b, 256) == (2, 128)
        assert _lib.disk_flash_plan(b, 320) == (2, 192)
        assert _lib.disk_flash_plan(b, 333) == (2, 192)
    assert _lib.disk_flash_plan(0, 64) is None and _lib.disk_flash_plan(1, 0) is None
