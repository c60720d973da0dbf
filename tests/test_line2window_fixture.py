"""CPU checks behind tests/test_gpu_line2window_edges.py.

* The torch oracle (oracle/correlation_ref.py, oracle/desc_train_ref.py) in
  float32 against the reference's own modules at unequal image sizes and at
  grid 8 (tests/golden/desc_grad_edges.npz, draws replayed): the oracle was
  pinned at equal sizes and grid 16 only.
* The self-checks of tests/line2window_fixture.py: every case's float64
  reference is finite, the float32 and the float64 oracle pick the same line
  centres on >= 0.999 of the points, the window shapes are the ones each case
  is named for, and the zeroed pixels of ``zeropix`` lie inside windows that
  carry loss weight (all asserted in ``line2window_fixture.build``).
* The float32 oracle's own gradient error against the float64 oracle, the
  yardstick for the GPU figures: at most 1.10e-4 of the map's largest gradient
  over all cases (win1x3; the others 1.2e-5 .. 6.7e-5), printed per case.
"""
import os

import numpy as np
import pytest
import torch

import line2window_fixture as LF
from conftest import GOLDEN
from oracle import correlation_ref as cr
from oracle.desc_train_ref import desc_loss_grad


def _close(got, ref, rel, what=""):
    scale = max(float(np.abs(ref).max()), 1e-12)
    err = float(np.abs(got - ref).max())
    assert err <= rel * scale, "%s: max err %.3e vs scale %.3e" % (what, err, scale)


@pytest.mark.parametrize("tag", ["uneq", "g8"])
def test_oracle_desc_grad_edges_vs_reference(tag):
    """Same tolerances as test_oracle_desc_grad_vs_reference (loss rtol 1e-5,
    gradients 1e-5 of the map's scale) and as
    test_line2window_and_epipolar_loss_oracle (components rtol 1e-4, centres
    and window expectations 1e-4)."""
    d = np.load(os.path.join(GOLDEN, "desc_grad_edges.npz"))
    spec = LF.CASES[tag]
    inp = LF.raw_inputs(spec)
    g = lambda k: torch.from_numpy(d["%s_%s" % (tag, k)])  # noqa: E731
    draws = (g("sel1").long(), g("sel2").long(), g("rand1"), g("rand2"))
    assert draws[0].shape == inp["sel1"].shape and draws[1].shape == inp["sel2"].shape
    kw = dict(grid_size=spec["grid"], window_size=spec["window"], line_step=spec["line_step"])
    xf1, xf2, F1, F2 = inp["xf1"], inp["xf2"], inp["F1"], inp["F2"]
    loss, g1, g2, _ = desc_loss_grad(xf1, xf2, F1, F2, spec["hw1"], spec["hw2"], *draws, **kw)
    np.testing.assert_allclose(float(loss), float(d[tag + "_loss"]), rtol=1e-5)
    _close(g1.numpy()[:, ::2, ::2, ::2], d[tag + "_dxf1_sub"], 1e-5, "dxf1")
    _close(g2.numpy()[:, ::2, ::2, ::2], d[tag + "_dxf2_sub"], 1e-5, "dxf2")
    sums = d[tag + "_dxf_sums"]
    np.testing.assert_allclose(float(g1.abs().sum()), sums[1], rtol=1e-4)
    np.testing.assert_allclose(float(g2.abs().sum()), sums[3], rtol=1e-4)
    proc = cr.line2window(xf1, xf2, F1, F2, spec["hw1"], spec["hw2"], *draws, **kw)
    for k, name in (("l1_org", "feat1c_corloc_org"), ("l2_org", "feat2c_corloc_org"),
                    ("w1", "feat1w_corloc"), ("w2", "feat2w_corloc")):
        np.testing.assert_allclose(proc[name].numpy(), d["%s_%s" % (tag, k)], atol=1e-4, rtol=1e-4,
                                   err_msg=k)
    lval, comp = cr.epipolar_loss(proc, F1, F2, spec["hw1"])
    np.testing.assert_allclose(float(lval), float(d[tag + "_loss"]), rtol=1e-4)
    # loss_g* (weight_grid 0 keeps them out of the loss) weigh by 1 / std of a
    # peaked softmax over ~100 grid points, where float32 E[c^2] - E[c]^2
    # cancels: on ``uneq`` the reference's own loss_g1 (27.9789) and this
    # oracle's (27.9640) sit 6.8e-4 and 1.2e-3 from the float64 value (27.9979)
    # and differ by summation order only; every other component is bit-equal.
    for k, v in comp.items():
        np.testing.assert_allclose(float(v), float(d["%s_%s" % (tag, k)]),
                                   rtol=2e-3 if k.startswith("loss_g") else 1e-4, err_msg=k)


@pytest.mark.parametrize("name", list(LF.CASES))
def test_fixture_case_self_checks(name):
    c = LF.case(name)     # build() asserts the conditions listed in the module docstring
    r = c["ref"]
    print("l2w-fixture %s n1 %d n2 %d oracle-agreement %.4f %.4f valid %.3f %.3f loss %.6f"
          % (name, c["n1"], c["n2"], r["oracle_agree"][0], r["oracle_agree"][1], r["valid"][0],
             r["valid"][1], float(r["loss"])))
    assert min(r["oracle_agree"]) >= LF.ORACLE_FLOOR
    if name == "g4mix":   # about half of direction 1's lines miss the smaller image 2
        assert 0.3 < r["valid"][0] < 0.6
        assert c["n1"] == 4352 and c["n2"] == 1280
    if name == "uneq":
        assert (c["n1"], c["n2"]) == (140, 96)
    if name == "zeropix":
        assert len(c["zero1"]) == LF.N_ZERO and len(c["zero2"]) == LF.N_ZERO


@pytest.mark.parametrize("name", list(LF.CASES))
def test_fp32_oracle_gradient_error_vs_fp64(name):
    """The float32 oracle stays inside the project's gradient bound (1e-3 of
    the map's largest gradient) with the float64 oracle's centres and weights."""
    e1, e2 = LF.oracle_fp32_error(name)
    print("l2w-fixture %s fp32-oracle grad-ratio %.3e %.3e" % (name, e1, e2))
    assert max(e1, e2) <= 1e-3


def test_oracle_default_dtype_is_float32():
    """float32 in, float32 out (the golden pins rely on it); float64 in, float64 out."""
    sel = torch.zeros(1, 2, 3, dtype=torch.long)
    assert cr.grid_points(sel, 32, 48, 16).dtype == torch.float32
    assert cr.grid_points(sel, 32, 48, 16, torch.float64).dtype == torch.float64
    c = torch.zeros(1, 4, 2)
    assert cr.denormalize_coords(c, 32, 48).dtype == torch.float32
    assert cr.denormalize_coords(c.double(), 32, 48).dtype == torch.float64
    assert cr.gen_grid(-1, 1, -1, 1, 3, 4).dtype == torch.float32
