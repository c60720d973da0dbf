"""Seeded Line2Window / EpipolarLoss inputs with their float64 reference (test
helper for tests/test_gpu_line2window_edges.py and the CPU self-checks in
tests/test_line2window_fixture.py).

``CASES`` names one input per branch of posfeat_amd/csrc/corr.hip that the
equal-size, grid-16, window-0.1, line_step-100 tests never enter (the table
below says which).  ``make_inputs`` builds the fp32 inputs as
tests/test_desc_grad.py::_case does (3x3 average-pooled Gaussian maps,
``synthetic_fundamental`` unless the case names another F, draws from one
``RandomState``); ``reference(name)`` runs the torch oracle
(oracle/correlation_ref.py, oracle/desc_train_ref.py) on those values cast up
to float64, end to end: grid stage, line search, window stage, loss and the
two map gradients.

The line search ends in a discrete arg-max that may flip on a near tie, which
moves a whole window.  So the line stage is compared on its own (centres
agree on >= ``LINE_FLOOR`` of the points), and everything after it is
computed from the centres it is given: ``window_stage`` and ``grad_reference``
take the GPU's ``l*_exp_n`` (and, for the gradient, the GPU's detached loss
weights), as tests/test_desc_grad.py does.  ``reference`` asserts that the
float32 oracle's own centres agree with the float64 ones on >=
``ORACLE_FLOOR`` of the points: each case's seed was chosen so that this holds.

case      b  image 1 / image 2     grid window step  reaches
uneq      2  160x224 / 128x192     16   0.1    100   n1 = 140 != n2 = 96: rectangular S, the column
                                                     kernel with n2 % 64 != 0 and n1 % COL_CH != 0,
                                                     4x5 and 3x4 windows, the two-count loss
rem8      3  168x232 both          16   0.1    100   H, W = 8 mod 16 (map pixels past the last cell);
                                                     b = 3: pf_xcd_block with a grid % 8 != 0
g8        1  128x160 both          8    0.1    100   3x4 windows; l2norm_bwd's cell search at its
                                                     widest unrolled range (always 3 cells at grid 8)
g4mix     1  256x272 / 128x160     4    0.1    100   n1 = 4352 > WG_MAXN >= n2 = 1280: direction 1 on
                                                     the per-tap fixed-point scatter, direction 2 on
                                                     patch + gather, the mixed memset; 5x5 cell ranges:
                                                     l2norm_bwd's generic cell loop; one map pixel per
                                                     cell; about half of the lines miss the image
win1x3    1  48x128 both           16   0.1    100   win_h = 1 (linspace with n = 1); n = 24
taps484   1  352x352 both          16   0.25   64    22x22 = 484 taps: all 8 logit slots per lane, a
                                                     26x26 forward patch; the backward patch exceeds
                                                     the record stride: per-tap path both ways
ls128     1  160x224 both          16   0.125  128   MAX_LINE; the largest window the record stride
                                                     is sized for (patch == stride)
ls2       1  160x224 both          16   0.1    2     two line samples, lanes 2..63 hold -inf
horiz     1  160x224 both          16   0.1    100   F = [t]x, t = (1,0,0): la == 0 exactly, two of
vert      1  160x224 both          16   0.1    100   the four candidate endpoints +-inf / NaN (t =
                                                     (0,1,0): lb == 0); every line stays valid
stride    1  as uneq               16   0.1    100   channel strides 192 / 256, extra channels NaN
zeropix   1  as g8                 8    0.1    100   six all-zero map pixels per image inside valid
                                                     windows: the |x| <= 1e-12 branch of l2norm_scale
                                                     and l2norm_bwd (query_bwd's needs a zero *sample*
                                                     on a point that still carries gradient, which a
                                                     zero descriptor's all-tie line search rules out)
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import correlation_ref as cr
from oracle.desc_train_ref import desc_loss_grad, loss_weights

T = 60.0
WIN_COST_THR = 0.1
LINE_FLOOR = 0.995     # GPU centres vs the float64 oracle (tests/test_gpu_correlation.py)
ORACLE_FLOOR = 0.999   # float32 oracle vs float64 oracle, per case and direction
LINE_ATOL = 1e-4       # "same centre", normalised units
N_ZERO = 6


def _spec(b, hw1, hw2=None, grid=16, window=0.1, line_step=100, seed=11, fund="synthetic",
          cs=(128, 128), zero=False):
    return dict(b=b, hw1=hw1, hw2=hw2 or hw1, grid=grid, window=window, line_step=line_step,
                seed=seed, fund=fund, cs=cs, zero=zero)


CASES = {
    "uneq": _spec(2, (160, 224), (128, 192)),
    "rem8": _spec(3, (168, 232)),
    "g8": _spec(1, (128, 160), grid=8),
    "g4mix": _spec(1, (256, 272), (128, 160), grid=4),
    "win1x3": _spec(1, (48, 128)),
    "taps484": _spec(1, (352, 352), window=0.25, line_step=64),
    "ls128": _spec(1, (160, 224), window=0.125, line_step=128),
    "ls2": _spec(1, (160, 224), line_step=2),
    "horiz": _spec(1, (160, 224), fund="horiz"),
    "vert": _spec(1, (160, 224), fund="vert"),
    "stride": _spec(1, (160, 224), (128, 192), cs=(192, 256)),
    "zeropix": _spec(1, (128, 160), grid=8, zero=True),
}
# (win_h, win_w) of the window in image 2 (direction 1) and in image 1 (direction 2)
WINDOWS = {"uneq": ((3, 4), (4, 5)), "rem8": ((4, 5), (4, 5)), "g8": ((3, 4), (3, 4)),
           "g4mix": ((3, 4), (6, 6)), "win1x3": ((1, 3), (1, 3)), "taps484": ((22, 22), (22, 22)),
           "ls128": ((5, 7), (5, 7)), "ls2": ((4, 5), (4, 5)), "horiz": ((4, 5), (4, 5)),
           "vert": ((4, 5), (4, 5)), "stride": ((3, 4), (4, 5)), "zeropix": ((3, 4), (3, 4))}

_TX = {"horiz": (1.0, 0.0, 0.0), "vert": (0.0, 1.0, 0.0)}


def window_shape(window, hw):
    """(win_h, win_w) on the H/4 x W/4 map, as the kernels and the oracle size it."""
    w32 = np.float32(window)
    return int(w32 * np.float32(hw[0] // 4)), int(w32 * np.float32(hw[1] // 4))


def _fundamentals(spec):
    from posfeat_amd.correlation import synthetic_fundamental
    b = spec["b"]
    if spec["fund"] == "synthetic":
        F1, F2 = synthetic_fundamental(b, spec["hw1"][0], spec["hw1"][1], spec["seed"])
        return torch.from_numpy(F1), torch.from_numpy(F2)
    tx, ty, tz = _TX[spec["fund"]]
    skew = torch.tensor([[0.0, -tz, ty], [tz, 0.0, -tx], [-ty, tx, 0.0]])
    F1 = skew[None].repeat(b, 1, 1).contiguous()
    return F1, (-F1.transpose(1, 2)).contiguous()


def raw_inputs(spec):
    """The fp32 inputs of a spec before any pixel is zeroed: NCHW maps,
    F1 / F2 [b,3,3], sel [b, H/g, W/g] (long), rand [b, n, 2]."""
    b, g = spec["b"], spec["grid"]
    (H1, W1), (H2, W2) = spec["hw1"], spec["hw2"]
    rs = np.random.RandomState(spec["seed"])
    xf1 = torch.from_numpy(rs.randn(b, 128, H1 // 4, W1 // 4).astype(np.float32))
    xf2 = torch.from_numpy(rs.randn(b, 128, H2 // 4, W2 // 4).astype(np.float32))
    xf1 = F.avg_pool2d(xf1, 3, 1, 1)
    xf2 = F.avg_pool2d(xf2, 3, 1, 1)
    F1, F2 = _fundamentals(spec)
    n1, n2 = (H1 // g) * (W1 // g), (H2 // g) * (W2 // g)
    sel1 = torch.from_numpy(rs.randint(0, g * g, (b, H1 // g, W1 // g))).long()
    sel2 = torch.from_numpy(rs.randint(0, g * g, (b, H2 // g, W2 // g))).long()
    rand1 = torch.from_numpy(rs.rand(b, n1, 2).astype(np.float32))
    rand2 = torch.from_numpy(rs.rand(b, n2, 2).astype(np.float32))
    return dict(b=b, hw1=(H1, W1), hw2=(H2, W2), n1=n1, n2=n2, grid=g, window=spec["window"],
                line_step=spec["line_step"], cs=spec["cs"], xf1=xf1, xf2=xf2, F1=F1, F2=F2,
                sel1=sel1, sel2=sel2, rand1=rand1, rand2=rand2, zero1=None, zero2=None)


def _dbl(inp):
    return [inp[k].double() for k in ("xf1", "xf2", "F1", "F2")]


def _kw(inp):
    return dict(temperature=T, grid_size=inp["grid"], window_size=inp["window"],
                line_step=inp["line_step"], win_cost_thr=WIN_COST_THR)


def _draws(inp):
    return inp["sel1"], inp["sel2"], inp["rand1"], inp["rand2"]


def tap_pixels(center, window, hw):
    """float64: for centres [n,2] (normalised) the map-pixel positions of the
    window taps, (fx [n, win_w], fy [n, win_h])."""
    h, w = hw[0] // 4, hw[1] // 4
    wh, ww = window_shape(window, hw)
    lx = torch.linspace(-window, window, ww, dtype=torch.float64)
    ly = torch.linspace(-window, window, wh, dtype=torch.float64)
    fx = ((center[:, 0:1] + lx[None] + 1) * w - 1) / 2
    fy = ((center[:, 1:2] + ly[None] + 1) * h - 1) / 2
    return fx, fy


def covered(pix, center, live, window, hw):
    """True when map pixel (py, px) is a bilinear corner, with non-zero weight,
    of some tap of a window in ``center[live]``."""
    py, px = pix
    fx, fy = tap_pixels(center[live].double(), window, hw)
    hx = ((fx - px).abs() < 1).any(1)
    hy = ((fy - py).abs() < 1).any(1)
    return bool((hx & hy).any())


def _live(coord, wn, std, valid, Fm, hw_target, short):
    """The points whose window carries loss weight: valid and under the cost threshold."""
    wpx = cr.denormalize_coords(wn, *hw_target)
    return loss_weights(coord, wpx, std, valid, Fm, short, WIN_COST_THR) > 0


def _stages(inp, dtype):
    """Grid stage, line search and window stage of the oracle in ``dtype`` (own centres)."""
    xf1, xf2, F1, F2 = [inp[k].to(dtype) for k in ("xf1", "xf2", "F1", "F2")]
    g = grid_stage(xf1, xf2, inp["hw1"], inp["hw2"], inp["sel1"], inp["sel2"], inp["grid"])
    (H1, W1), (H2, W2) = inp["hw1"], inp["hw2"]
    l1, o1, v1, _ = cr.epipolar_line_search(g["coord1"], F1, g["f1"], g["fm2"], H2, W2, inp["rand1"],
                                            inp["line_step"], inp["window"])
    l2, o2, v2, _ = cr.epipolar_line_search(g["coord2"], F2, g["f2"], g["fm1"], H1, W1, inp["rand2"],
                                            inp["line_step"], inp["window"])
    g.update(l1=l1, l2=l2, l1_org=o1, l2_org=o2, v1=v1, v2=v2,
             e1=cr.get_endpoints(g["coord1"], F1, H2, W2)[2],
             e2=cr.get_endpoints(g["coord2"], F2, H1, W1)[2])
    return g


def _pick_zero_pixels(inp):
    """Six pixels per map, each two map pixels right of the centre of a window
    that carries loss weight (so inside its footprint, off its line sample),
    evenly spread over those windows.  ``reference`` re-checks them on the
    zeroed maps."""
    xf1, xf2, F1, F2 = _dbl(inp)
    s = _stages(inp, torch.float64)
    short = min(inp["hw1"])
    out = []
    for c, l, f, fm, v, Fm, hw in ((s["coord1"], s["l1"], s["f1"], s["fm2"], s["v1"], F1, inp["hw2"]),
                                   (s["coord2"], s["l2"], s["f2"], s["fm1"], s["v2"], F2, inp["hw1"])):
        wn, _, ws = cr.window_expectation(f, fm, l, inp["window"])
        live = _live(c, wn, ws, v, Fm, hw, short)[0]
        h, w = hw[0] // 4, hw[1] // 4
        px = torch.floor(((l[0, :, 0] + 1) * w - 1) / 2).long() + 2
        py = torch.floor(((l[0, :, 1] + 1) * h - 1) / 2).long()
        ok = live & (px >= 0) & (px < w) & (py >= 0) & (py < h)
        idx = torch.nonzero(ok).flatten()
        pix = []
        for i in idx[torch.linspace(0, len(idx) - 1, 3 * N_ZERO).long()].tolist():
            p = (int(py[i]), int(px[i]))
            if p not in pix:
                pix.append(p)
        assert len(pix) >= N_ZERO
        out.append(pix[:N_ZERO])
    return out[1], out[0]   # pixels of image 1 (direction 2's windows), of image 2


def make_inputs(spec):
    inp = raw_inputs(spec)
    if spec["zero"]:
        z1, z2 = _pick_zero_pixels(inp)
        inp["xf1"], inp["xf2"] = inp["xf1"].clone(), inp["xf2"].clone()
        for py, px in z1:
            inp["xf1"][0, :, py, px] = 0
        for py, px in z2:
            inp["xf2"][0, :, py, px] = 0
        inp["zero1"], inp["zero2"] = z1, z2
    return inp


# ------------------------------------------------------------------ reference
def grid_stage(xf1, xf2, hw1, hw2, sel1, sel2, grid, temperature=T):
    """Grid points, their descriptors, the row / column softmax expectations
    and stds (Preprocess_Line2Window's grid branch, oracle.correlation_ref.
    line2window) in the dtype of the maps, for any two image sizes."""
    (H1, W1), (H2, W2) = hw1, hw2
    b = xf1.shape[0]
    c1n = cr.grid_points(sel1.reshape(b, H1 // grid, W1 // grid), H1, W1, grid, xf1.dtype)
    c2n = cr.grid_points(sel2.reshape(b, H2 // grid, W2 // grid), H2, W2, grid, xf2.dtype)
    coord1 = cr.denormalize_coords(c1n, H1, W1)
    coord2 = cr.denormalize_coords(c2n, H2, W2)
    f1 = cr.sample_feat(xf1, c1n, True)
    f2 = cr.sample_feat(xf2, c2n, True)
    cos = f1 @ f2.transpose(1, 2)
    p_row = torch.softmax(temperature * cos, dim=2)                    # [b, n1, n2]
    p_colT = torch.softmax(temperature * cos, dim=1).transpose(1, 2)   # [b, n2, n1]
    g1, g2 = p_row @ coord2, p_colT @ coord1
    s1 = p_row @ c2n ** 2 - cr.normalize_coords(g1, H2, W2) ** 2
    s2 = p_colT @ c1n ** 2 - cr.normalize_coords(g2, H1, W1) ** 2
    return dict(c1n=c1n, c2n=c2n, coord1=coord1, coord2=coord2, f1=f1, f2=f2, g1=g1, g2=g2,
                g1_std=s1.clamp(min=1e-6).sqrt().sum(-1), g2_std=s2.clamp(min=1e-6).sqrt().sum(-1),
                fm1=temperature * F.normalize(xf1, p=2.0, dim=1),
                fm2=temperature * F.normalize(xf2, p=2.0, dim=1))


def fp64_stage(xf1, xf2, F1, F2, hw1, hw2, sel1, sel2, raw, grid=16, window=0.1):
    """The reference's formulas in float64 on fp32 inputs cast up, with the
    window stage centred on the GPU's own jittered line expectations
    ``raw['l*_exp_n']`` and the GPU's validity flags: the processed dict of
    Preprocess_Line2Window (without the line-search entries)."""
    xf1, xf2 = xf1.double(), xf2.double()
    g = grid_stage(xf1, xf2, hw1, hw2, sel1, sel2, grid)
    l1 = raw["l1_exp_n"].cpu().double()
    l2 = raw["l2_exp_n"].cpu().double()
    w1n, _, w1s = cr.window_expectation(g["f1"], g["fm2"], l1, window)
    w2n, _, w2s = cr.window_expectation(g["f2"], g["fm1"], l2, window)
    return {"coord1": g["coord1"], "coord2": g["coord2"], "feat1g_corloc": g["g1"],
            "feat2g_corloc": g["g2"], "feat1w_corloc": cr.denormalize_coords(w1n, *hw2),
            "feat2w_corloc": cr.denormalize_coords(w2n, *hw1), "feat1g_std": g["g1_std"],
            "feat2g_std": g["g2_std"], "feat1w_std": w1s, "feat2w_std": w2s,
            "valid_epi1": raw["valid1"].cpu().bool(), "valid_epi2": raw["valid2"].cpu().bool()}


def _fp64_reference_stage(tag, d, raw):
    """``fp64_stage`` on the inputs and draws of tests/golden/correlation.npz
    (equal sizes, grid 16, window 0.1): (processed, F1, F2, (H, W), half)."""
    from test_oracle_correlation import _inputs
    b, H, W, xf1, xf2, kp1, kp2, F1, F2 = _inputs(tag)
    sel1 = torch.from_numpy(d[tag + "_sel1"]).long()
    sel2 = torch.from_numpy(d[tag + "_sel2"]).long()
    proc = fp64_stage(xf1, xf2, F1, F2, (H, W), (H, W), sel1, sel2, raw)
    return proc, F1.double(), F2.double(), (H, W), np.array([(W - 1) / 2.0, (H - 1) / 2.0])


def window_stage(name, raw):
    """Processed dict in float64 for case ``name`` around the centres in ``raw``."""
    inp = case(name)
    return fp64_stage(inp["xf1"], inp["xf2"], inp["F1"], inp["F2"], inp["hw1"], inp["hw2"],
                      inp["sel1"], inp["sel2"], raw, inp["grid"], inp["window"])


def grad_reference(name, raw):
    """(loss, dxf1, dxf2) of the float64 oracle with the centres and the
    detached loss weights of ``raw`` (a forward's outputs: coord*, w*, w*_std,
    valid*, l*_exp_n), as test_gpu_desc_grad_vs_oracle_same_centres shares them."""
    inp = case(name)
    xf1, xf2, F1, F2 = _dbl(inp)
    short = min(inp["hw1"])
    r = {k: v.cpu() for k, v in raw.items()}
    wts = [loss_weights(r["coord%d" % i].double(), r["w%d" % i].double(), r["w%d_std" % i].double(),
                        r["valid%d" % i].bool(), Fm, short, WIN_COST_THR)
           for i, Fm in ((1, F1), (2, F2))]
    loss, g1, g2, _ = desc_loss_grad(xf1, xf2, F1, F2, inp["hw1"], inp["hw2"], *_draws(inp),
                                     centers=(r["l1_exp_n"].double(), r["l2_exp_n"].double()),
                                     weights=wts, **_kw(inp))
    return loss, g1, g2


def agreement(la, lb):
    """Per-point flag: two sets of centres [b,n,2] are the same window."""
    return ((la.double() - lb.double()).abs() < LINE_ATOL).all(-1)


def build(name):
    spec = CASES[name]
    inp = make_inputs(spec)
    assert (window_shape(inp["window"], inp["hw2"]),
            window_shape(inp["window"], inp["hw1"])) == WINDOWS[name]
    xf1, xf2, F1, F2 = _dbl(inp)
    s64 = _stages(inp, torch.float64)
    s32 = _stages(inp, torch.float32)
    loss, g1, g2, (l1, l2) = desc_loss_grad(xf1, xf2, F1, F2, inp["hw1"], inp["hw2"], *_draws(inp),
                                            **_kw(inp))
    assert torch.equal(l1, s64["l1"]) and torch.equal(l2, s64["l2"])
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(g1).all()) and \
        bool(torch.isfinite(g2).all()), "%s: the float64 reference is not finite" % name
    for k in ("g1", "g2", "g1_std", "g2_std"):
        assert bool(torch.isfinite(s64[k]).all()), (name, k)
    for hw in (inp["hw1"], inp["hw2"]):   # the oracle (double) and the kernels (float) size alike
        assert window_shape(inp["window"], hw) == (int(inp["window"] * (hw[0] // 4)),
                                                   int(inp["window"] * (hw[1] // 4)))
    agree = (float(agreement(s32["l1"], s64["l1"]).double().mean()),
             float(agreement(s32["l2"], s64["l2"]).double().mean()))
    assert min(agree) >= ORACLE_FLOOR, \
        "%s seed %d: float32 and float64 oracle centres agree on %.4f / %.4f" % (
            name, spec["seed"], agree[0], agree[1])
    if spec["fund"] != "synthetic":   # axis-aligned lines: every endpoint pair is in the image
        assert bool(s64["e1"].all()) and bool(s64["e2"].all())
    if spec["zero"]:
        short = min(inp["hw1"])
        for pix, xf, c, l, f, fm, v, Fm, hw in (
                (inp["zero2"], inp["xf2"], s64["coord1"], s64["l1"], s64["f1"], s64["fm2"],
                 s64["v1"], F1, inp["hw2"]),
                (inp["zero1"], inp["xf1"], s64["coord2"], s64["l2"], s64["f2"], s64["fm1"],
                 s64["v2"], F2, inp["hw1"])):
            wn, _, ws = cr.window_expectation(f, fm, l, inp["window"])
            live = _live(c, wn, ws, v, Fm, hw, short)[0]
            for p in pix:
                assert float(xf[0, :, p[0], p[1]].abs().max()) == 0
                assert covered(p, l[0], live, inp["window"], hw), \
                    "%s: zero pixel %s is in no valid window" % (name, p)
    inp["ref"] = dict(stages=s64, loss=loss, dxf1=g1, dxf2=g2, oracle_agree=agree,
                      valid=(float(s64["v1"].double().mean()), float(s64["v2"].double().mean())))
    return inp


@functools.lru_cache(maxsize=None)
def case(name):
    """The built case ``name`` (inputs + float64 reference), computed once per
    session and shared; callers must not modify it."""
    return build(name)


def oracle_fp32_error(name):
    """max|g32 - g64| / max|g64| per map: the float32 oracle against the
    float64 one on the same centres and loss weights (those of the float64 run)."""
    inp = case(name)
    s = inp["ref"]["stages"]
    xf1, xf2, F1, F2 = _dbl(inp)
    short = min(inp["hw1"])
    w1n, _, w1s = cr.window_expectation(s["f1"], s["fm2"], s["l1"], inp["window"])
    w2n, _, w2s = cr.window_expectation(s["f2"], s["fm1"], s["l2"], inp["window"])
    wts = [loss_weights(s["coord1"], cr.denormalize_coords(w1n, *inp["hw2"]), w1s, s["v1"], F1, short),
           loss_weights(s["coord2"], cr.denormalize_coords(w2n, *inp["hw1"]), w2s, s["v2"], F2, short)]
    ref = desc_loss_grad(xf1, xf2, F1, F2, inp["hw1"], inp["hw2"], *_draws(inp),
                         centers=(s["l1"], s["l2"]), weights=wts, **_kw(inp))
    got = desc_loss_grad(inp["xf1"], inp["xf2"], inp["F1"], inp["F2"], inp["hw1"], inp["hw2"],
                         *_draws(inp), centers=(s["l1"].float(), s["l2"].float()),
                         weights=[w.float() for w in wts], **_kw(inp))
    out = []
    for i, zero in ((1, inp["zero1"]), (2, inp["zero2"])):
        keep = nonzero_mask(ref[i], zero)
        scale = float((ref[i].abs() * keep).max())
        out.append(float(((got[i].double() - ref[i]).abs() * keep).max()) / scale)
    return tuple(out)


def nonzero_mask(g, zero):
    """[b,1,h,w] float mask, 0 at the all-zero input pixels ``zero`` of image 0."""
    keep = torch.ones(g.shape[0], 1, g.shape[2], g.shape[3], dtype=g.dtype)
    for py, px in zero or ():
        keep[0, 0, py, px] = 0
    return keep


def find_seed(name, start=0, tries=200):
    """The first seed >= start at which ``name`` meets the oracle-agreement
    condition (CPU only; how a seed other than 11 would be picked)."""
    for seed in range(start, start + tries):
        CASES[name] = dict(CASES[name], seed=seed)
        try:
            build(name)
            return seed
        except AssertionError:
            continue
    raise RuntimeError("no seed for %s" % name)
