"""Seeded DiskLoss inputs with their float64 reference (test helper).

``case(name)`` builds one entry of ``CASES``: fp32 score maps, descriptor maps,
fundamental matrices and explicit Categorical / Bernoulli draws, plus the
reference computed by ``oracle.train_ref.disk_loss_autograd`` and
``oracle.correlation_ref.disk_loss`` in float64 on those same fp32 values cast
up (loss, reinforce, penalty, n_kps and the score-map gradients from
``torch.autograd.grad``).  ``bound`` = sum over accepted pairs of
|reward p (logp_dense + logp1 + logp2)| + |penalty| is the magnitude the loss
terms' error is measured against.

The reward is a step at ``reward_thr``: a pair whose epipolar distance sits on
the threshold may legitimately flip in fp32.  Every case therefore asserts, on
the float64 reference alone, that no accepted pair has either line distance
within ``THR_MARGIN`` px of the threshold; the seeds in ``CASES`` were chosen
(``find_seed``) so that this holds -- no pair is ever masked out.

``sampler_case`` does the same for the in-kernel sampler: uniforms, the
float64 Gumbel-max / Bernoulli draws made from them, and seeds for which no
cell's decision is within rounding of flipping.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import correlation_ref as cr
from oracle.train_ref import disk_loss_autograd

THR_MARGIN = 1e-3    # px: no accepted pair's line distance this close to reward_thr
KEY_GAP = 1e-4       # sampler: top-2 Gumbel key gap of every cell
ACC_GAP = 1e-5       # sampler: |u - sigmoid(logit)| of every cell

DEFAULT_SCALARS = dict(T=60.0, reward_thr=2.0, good=1.0, bad=-0.25, kp_penalty=-0.001)

# name -> spec.  accept: "half" (rate 0.5) | "all" | "none" | ("counts", k1, k2)
# (exactly k1 / k2 accepted on side 1 / 2 of every image) | "b3mix" (image 0
# all, image 1 none on side 1 and half on side 2, image 2 exactly one per side)
TABLE = [  # the shape table: (name, b, H, W), n = (H / 8)(W / 8)
    ("n4", 1, 16, 16), ("n20", 2, 32, 40), ("n32", 1, 32, 64), ("n36", 1, 48, 48),
    ("n64", 1, 64, 64), ("n128", 1, 64, 128), ("n132", 1, 88, 96), ("n256", 1, 128, 128),
    ("n320", 1, 128, 160), ("b3n72", 3, 64, 72),
]
# the flash passes' plan each row must take (posfeat_disk_flash_plan):
# name -> (nsplit, rows_per_split)
PLANS = {"n4": (1, 64), "n20": (1, 64), "n32": (1, 64), "n36": (1, 64), "n64": (1, 64),
         "n128": (1, 128), "n132": (1, 192), "n256": (2, 128), "n320": (2, 192),
         "b3n72": (1, 128)}
SHAPES = {name: (b, H, W) for name, b, H, W in TABLE}


def _spec(shape, seed, accept="half", desc="random", score="rand3", cs=(128, 128), **scalars):
    b, H, W = SHAPES[shape]
    return dict(b=b, H=H, W=W, seed=seed, accept=accept, desc=desc, score=score, cs=cs,
                scalars=dict(DEFAULT_SCALARS, **scalars))


CASES = {
    # the shape table at rate 0.5 (b3n72: the mixed per-image pattern)
    "n4": _spec("n4", 1),
    "n20": _spec("n20", 1),
    "n32": _spec("n32", 1),
    "n36": _spec("n36", 1),
    "n64": _spec("n64", 1),
    "n128": _spec("n128", 1),
    "n132": _spec("n132", 1),
    "n256": _spec("n256", 4),
    "n320": _spec("n320", 2),
    "b3n72": _spec("b3n72", 3, accept="b3mix"),
    # acceptance patterns
    "n320_all": _spec("n320", 21, accept="all"),
    "n36_none": _spec("n36", 1, accept="none"),
    "n132_c31_32": _spec("n132", 1, accept=("counts", 31, 32)),
    "n132_c32_33": _spec("n132", 1, accept=("counts", 32, 33)),
    "n132_c33_64": _spec("n132", 1, accept=("counts", 33, 64)),
    "n132_c64_65": _spec("n132", 1, accept=("counts", 64, 65)),
    "n132_c65_128": _spec("n132", 2, accept=("counts", 65, 128)),
    "n132_c128_129": _spec("n132", 2, accept=("counts", 128, 129)),
    "n132_c129_31": _spec("n132", 1, accept=("counts", 129, 31)),
    # input modes
    "n132_peaky": _spec("n132", 1, desc="peaky"),
    "n132_extreme": _spec("n132", 5, score="extreme"),
    "n36_cs": _spec("n36", 1, cs=(192, 160)),
    "n132_scalars": _spec("n132", 1, T=20.0, reward_thr=1.0, good=2.0, bad=-1.0,
                          kp_penalty=-0.01),
}


def _masks(spec, rs):
    b, n = spec["b"], (spec["H"] // 8) * (spec["W"] // 8)
    acc = spec["accept"]

    def exact(k):
        m = np.zeros(n, bool)
        m[rs.permutation(n)[:k]] = True
        return m

    if isinstance(acc, float):
        return rs.rand(b, n) < acc, rs.rand(b, n) < acc
    if acc == "half":
        return rs.rand(b, n) < 0.5, rs.rand(b, n) < 0.5
    if acc == "all":
        return np.ones((b, n), bool), np.ones((b, n), bool)
    if acc == "none":
        return np.zeros((b, n), bool), np.zeros((b, n), bool)
    if acc == "b3mix":
        assert b == 3
        m1 = np.stack([np.ones(n, bool), np.zeros(n, bool), exact(1)])
        m2 = np.stack([np.ones(n, bool), rs.rand(n) < 0.5, exact(1)])
        return m1, m2
    if isinstance(acc, tuple) and acc[0] == "counts":
        return (np.stack([exact(acc[1]) for _ in range(b)]),
                np.stack([exact(acc[2]) for _ in range(b)]))
    m1, m2 = acc  # explicit per-image masks [b][n]
    return np.asarray(m1, bool).reshape(b, n), np.asarray(m2, bool).reshape(b, n)


def make_inputs(spec):
    """The fp32 inputs of a spec (NCHW maps, draws shaped [b,1,H/8,W/8])."""
    from posfeat_amd.correlation import synthetic_fundamental
    b, H, W, seed = spec["b"], spec["H"], spec["W"], spec["seed"]
    hc, wc = H // 8, W // 8
    rs = np.random.RandomState(seed)
    xf1 = F.avg_pool2d(torch.from_numpy(rs.randn(b, 128, H // 4, W // 4).astype(np.float32)),
                       3, 1, 1)
    if spec["desc"] == "peaky":  # sharp softmax rows: every row matters
        xf2 = xf1 + 0.05 * torch.from_numpy(rs.randn(*xf1.shape).astype(np.float32))
    else:
        xf2 = F.avg_pool2d(torch.from_numpy(rs.randn(b, 128, H // 4, W // 4).astype(np.float32)),
                           3, 1, 1)
    kps = []
    for _ in range(2):
        kp = rs.rand(b, 1, H, W).astype(np.float32) * 3
        if spec["score"] == "extreme":  # a quarter of the cells: logits spread over +-80
            wild = np.repeat(np.repeat(rs.rand(b, 1, hc, wc) < 0.25, 8, 2), 8, 3)
            kp = np.where(wild, (rs.rand(b, 1, H, W) * 160 - 80).astype(np.float32), kp)
        kps.append(torch.from_numpy(kp.astype(np.float32)))
    F1, F2 = synthetic_fundamental(b, H, W, seed)
    prop1 = torch.from_numpy(rs.randint(0, 64, (b, 1, hc, wc)))
    prop2 = torch.from_numpy(rs.randint(0, 64, (b, 1, hc, wc)))
    m1, m2 = _masks(spec, rs)
    return dict(b=b, H=H, W=W, n=hc * wc, kp1=kps[0], kp2=kps[1], xf1=xf1, xf2=xf2,
                F1=torch.from_numpy(F1), F2=torch.from_numpy(F2), prop1=prop1, prop2=prop2,
                acc1=torch.from_numpy(m1.reshape(b, 1, hc, wc)),
                acc2=torch.from_numpy(m2.reshape(b, 1, hc, wc)),
                cs=spec["cs"], scalars=dict(spec["scalars"]))


def oracle_args(inp, dtype):
    """Positional + keyword arguments of the oracle's DiskLoss in ``dtype``."""
    s = inp["scalars"]
    c = lambda k: inp[k].to(dtype)  # noqa: E731
    args = (c("kp1"), c("kp2"), c("xf1"), c("xf2"), c("F1"), c("F2"), inp["prop1"], inp["prop2"],
            inp["acc1"], inp["acc2"])
    kw = dict(temperature=s["T"], g=8, reward_thr=s["reward_thr"], good=s["good"], bad=s["bad"],
              kp_penalty=s["kp_penalty"])
    return args, kw


def oracle_run(inp, dtype):
    """(loss, dkp1, dkp2, components) of the oracle in ``dtype``."""
    args, kw = oracle_args(inp, dtype)
    kp1 = args[0].clone().requires_grad_(True)
    kp2 = args[1].clone().requires_grad_(True)
    loss = disk_loss_autograd(kp1, kp2, *args[2:], **kw)
    d1, d2 = torch.autograd.grad(loss, [kp1, kp2])
    _, comp = cr.disk_loss(*args, **kw)
    return loss.detach(), d1, d2, comp


def pair_terms(inp):
    """float64, over the accepted pairs only: the reinforce terms
    reward p (logp_dense + logp1 + logp2), the two line distances, and
    (logp1, logp2) of all points -- an independent restatement of the oracle's
    pair arithmetic for ``bound`` and the threshold condition."""
    (kp1, kp2, xf1, xf2, F1, F2, prop1, prop2, acc1, acc2), kw = oracle_args(inp, torch.float64)
    b, _, h, w = kp1.shape
    c1, logp1 = cr.disk_point_logp(kp1, 8, prop1, acc1)
    c2, logp2 = cr.disk_point_logp(kp2, 8, prop2, acc2)
    f1 = cr.sample_feat(xf1, cr.normalize_coords(c1, h, w), True)
    f2 = cr.sample_feat(xf2, cr.normalize_coords(c2, h, w), True)
    aff = -kw["temperature"] * (1 - f1 @ f2.transpose(1, 2))
    lrow, lcol = torch.log_softmax(aff, 2), torch.log_softmax(aff, 1)

    def dist(Fm, ca, cb):  # [b][na][nb]: distance of point b to the line of point a
        ln = Fm.bmm(cr.homogenize(ca).transpose(1, 2))
        ln = ln / torch.clamp(torch.norm(ln[:, :2, :], dim=1, keepdim=True), min=1e-8)
        return torch.abs(ln.transpose(1, 2) @ cr.homogenize(cb).transpose(1, 2))

    d1, d2 = dist(F1, c1, c2), dist(F2, c2, c1).transpose(1, 2)
    good = (d1 < kw["reward_thr"]) & (d2 < kw["reward_thr"])
    reward = torch.where(good, torch.tensor(kw["good"], dtype=torch.float64),
                         torch.tensor(kw["bad"], dtype=torch.float64))
    lp = logp1.reshape(b, -1, 1) + logp2.reshape(b, 1, -1)
    terms = reward * (lrow + lcol).exp() * (lrow + lcol + lp)
    am = acc1.reshape(b, -1, 1) & acc2.reshape(b, 1, -1)
    return terms[am], d1[am], d2[am], logp1.reshape(b, -1), logp2.reshape(b, -1)


def threshold_margin(inp):
    """Smallest | |d| - reward_thr | over both line distances of all accepted
    pairs (inf when no pair is accepted)."""
    _, d1, d2, _, _ = pair_terms(inp)
    if d1.numel() == 0:
        return float("inf")
    thr = inp["scalars"]["reward_thr"]
    return float(torch.minimum((d1 - thr).abs(), (d2 - thr).abs()).min())


def build(spec):
    inp = make_inputs(spec)
    margin = threshold_margin(inp)
    assert margin >= THR_MARGIN, \
        "seed %d: an accepted pair lies %.3g px from the reward threshold" % (spec["seed"], margin)
    loss, d1, d2, comp = oracle_run(inp, torch.float64)
    terms, _, _, logp1, logp2 = pair_terms(inp)
    kpp = inp["scalars"]["kp_penalty"]
    a1, a2 = inp["acc1"].reshape(inp["b"], -1), inp["acc2"].reshape(inp["b"], -1)
    penalty = kpp * (logp1[a1].sum() + logp2[a2].sum())
    # the restatement and the oracle agree (both float64)
    assert abs(float(terms.sum()) - float(comp["reinforce"])) <= 1e-9 * (1 + float(terms.abs().sum()))
    assert abs(float(penalty) - float(comp["kp_penalty"])) <= 1e-9 * (1 + abs(float(penalty)))
    inp["ref"] = dict(loss=float(loss), reinforce=float(comp["reinforce"]),
                      penalty=float(comp["kp_penalty"]),
                      n_kps=(int(a1.sum()) + int(a2.sum())) / inp["b"],
                      dkp1=d1[:, 0], dkp2=d2[:, 0],
                      bound=float(terms.abs().sum()) + abs(float(penalty)), margin=margin)
    return inp


@functools.lru_cache(maxsize=None)
def case(name):
    """The built case ``name`` (inputs + float64 reference), computed once per
    session and shared; callers must not modify it."""
    return build(CASES[name])


def find_seed(name, start=0, tries=2000):
    """The first seed >= start at which ``name`` meets the threshold condition
    (CPU only; how the seeds in CASES were picked)."""
    for seed in range(start, start + tries):
        if threshold_margin(make_inputs(dict(CASES[name], seed=seed))) >= THR_MARGIN:
            return seed
    raise RuntimeError("no seed for %s" % name)


def nhwc_padded(xf, cs):
    """NCHW [b,128,h,w] -> NHWC [b,h,w,cs], channels past 128 NaN (never read)."""
    b, c, h, w = xf.shape
    out = torch.full((b, h, w, cs), float("nan"), dtype=xf.dtype)
    out[..., :c] = xf.permute(0, 2, 3, 1)
    return out.contiguous()


# ---------------------------------------------------------------- sampler
U_LO = float(np.float32(1e-20))
U_HI = float(np.float32(1.0) - np.float32(1e-7))  # the clamp in fp32, as uniforms are fp32

SAMPLER_SEEDS = {"n20": 1, "n132": 8}


def sampler_draws(kp, uni, crafted=()):
    """float64 draws from fp32 score map kp [b,1,H,W] and uniforms [b][n][65]:
    proposal = argmax_j (v_j - log(-log u_j)) (lowest index on a tie), accept =
    u[64] < sigmoid(v[proposal]).  Returns (prop [b][n] long, acc [b][n] bool,
    smallest top-2 key gap, smallest |u - sigmoid|), the gaps over the cells
    not listed in ``crafted`` (flat cell ids whose ties are intended)."""
    b, _, H, W = kp.shape
    v = kp.double().unfold(2, 8, 8).unfold(3, 8, 8).reshape(b, -1, 64)
    u = uni.double()
    key = v - torch.log(-torch.log(u[..., :64].clamp(U_LO, U_HI)))
    top = key.max(-1, keepdim=True)[0]
    lanes = torch.arange(64).expand_as(key)
    prop = torch.where(key == top, lanes, torch.full_like(lanes, 64)).min(-1)[0]  # lowest index
    s2 = torch.sort(key, -1, descending=True)[0]
    sg = torch.sigmoid(torch.gather(v, -1, prop[..., None]).squeeze(-1))
    acc = u[..., 64] < sg
    keep = torch.ones(b * v.shape[1], dtype=torch.bool)
    for c in crafted:
        keep[c] = False
    kgap = (s2[..., 0] - s2[..., 1]).reshape(-1)[keep].min()
    agap = (u[..., 64] - sg).abs().reshape(-1)[keep].min()
    return prop, acc, float(kgap), float(agap)


def build_sampler(shape, seed):
    spec = dict(CASES[shape], seed=CASES[shape]["seed"])
    inp = make_inputs(spec)
    b, n, H, W = inp["b"], inp["n"], inp["H"], inp["W"]
    rs = np.random.RandomState(1000 + seed)
    unis = [torch.from_numpy(rs.rand(b, n, 65).astype(np.float32)) for _ in range(2)]
    # crafted cell (image 0, last cell, side 1): constant logits and constant
    # uniforms -- all 64 keys tie, the proposal is pixel 0
    cell = n - 1
    cy, cx = cell // (W // 8), cell % (W // 8)
    inp["kp1"] = inp["kp1"].clone()
    inp["kp1"][0, 0, cy * 8:cy * 8 + 8, cx * 8:cx * 8 + 8] = 0.75
    unis[0][0, cell, :64] = 0.5
    unis[0][0, cell, 64] = 0.25
    p1, a1, kg1, ag1 = sampler_draws(inp["kp1"], unis[0], crafted=(cell,))
    p2, a2, kg2, ag2 = sampler_draws(inp["kp2"], unis[1])
    assert int(p1[0, cell]) == 0 and bool(a1[0, cell])
    hc, wc = H // 8, W // 8
    inp.update(uni1=unis[0], uni2=unis[1], prop1=p1.reshape(b, 1, hc, wc),
               prop2=p2.reshape(b, 1, hc, wc), acc1=a1.reshape(b, 1, hc, wc),
               acc2=a2.reshape(b, 1, hc, wc), key_gap=min(kg1, kg2), acc_gap=min(ag1, ag2),
               crafted=(0, cell))
    return inp


@functools.lru_cache(maxsize=None)
def sampler_case(shape):
    inp = build_sampler(shape, SAMPLER_SEEDS[shape])
    assert inp["key_gap"] >= KEY_GAP, "top-2 key gap %.3g" % inp["key_gap"]
    assert inp["acc_gap"] >= ACC_GAP, "|u - sigmoid| %.3g" % inp["acc_gap"]
    assert threshold_margin(inp) >= THR_MARGIN
    return inp


def find_sampler_seed(shape, start=0, tries=2000):
    for seed in range(start, start + tries):
        inp = build_sampler(shape, seed)
        if (inp["key_gap"] >= KEY_GAP and inp["acc_gap"] >= ACC_GAP
                and threshold_margin(inp) >= THR_MARGIN):
            return seed
    raise RuntimeError("no sampler seed for %s" % shape)
