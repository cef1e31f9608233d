"""Float64 restatement of the distillation point loss (the contract of spfsplatv2_amd.loss.regr3d_loss), the seeded
inputs its tests use, and the knife-edge report that says whether an input's masks are decided beyond float32 rounding.
Written from the contract, not from the reference's code:

    dis_v = |gt_v|; n = H W points per row (view v, batch item b);
    quantile mode: rank r = float32(q) * float32(n - 1) in float32 for q = 0.002, 0.998 (torch.quantile's arithmetic);
        with s the row's sorted norms, q = s[floor r] + (r - floor r) (s[ceil r] - s[floor r]);
        valid = (dis >= q_lo) & (dis <= q_hi) & (conf >= 3) -- which, BY RANK, keeps exactly the values from
        s[ceil r_lo] (s[floor r_lo] when r_lo is an integer) to s[floor r_hi], ties included;
    clip mode: valid = dis <= dist_clip;
    nf[b] = max(sum over both views' valid points of |p| / (n1[b] + n2[b]), 1e-8) (1e-8 when the count is 0: float32's
        n + 1e-8 is n), for the predictions and for the ground truth; 1 without normalisation / with gt_scale;
    loss_v = sum_valid |pr / nf_pr[b] - gt / nf_gt[b]| / N_v over the whole batch, NaN when N_v = 0;
    loss = loss_1 + loss_2, or loss_2 with disable_view1.

The masks are taken by rank on the float64 norms of the float32 inputs.  A float32 evaluation (the product, the
reference) decides the same masks whenever the order statistics either side of each selected rank are further apart
than float32 rounding moves them: rank_gaps() reports those gaps, clip_gap() the distance of the nearest norm to
dist_clip, and the exact gates of the tests (n_valid, zero gradients at invalid points) use only inputs where they are
>= 1e-5 relative.  Gradients come from autograd in float64, which follows torch's rules by construction: zero at
|x| = 0 (vector_norm), nothing for invalid points, and both the direct term and the path through nf_pr."""
from __future__ import annotations

import math

import numpy as np
import torch

Q_LO, Q_HI = 0.002, 0.998
CONF_MIN = 3.0
NF_MIN = float(np.float32(1e-8))


def selected_ranks(n: int):
    """((floor, ceil, weight) for q_lo, the same for q_hi), the weight r - floor r in float32 as torch forms it."""
    out = []
    for q in (Q_LO, Q_HI):
        r = np.float32(q) * np.float32(n - 1)
        lo = np.floor(r)
        out.append((int(lo), int(np.ceil(r)), float(np.float32(r - lo))))
    return tuple(out)


def _norms(p: torch.Tensor) -> torch.Tensor:
    return torch.linalg.vector_norm(p.double(), dim=-1)


def thresholds(dis: torch.Tensor) -> torch.Tensor:
    """q [B,2] (q_lo, q_hi) of dis [B,H,W] (float64), lerp in float64 with torch's float32 weights."""
    flat = dis.flatten(1)
    s = flat.sort(dim=1).values
    cols = []
    for lo, hi, w in selected_ranks(flat.shape[1]):
        cols.append(s[:, lo] + w * (s[:, hi] - s[:, lo]))
    return torch.stack(cols, 1)


def rank_mask(dis: torch.Tensor) -> torch.Tensor:
    """The quantile part of the mask BY RANK: values from s[ceil r_lo] (s[floor r_lo] when the weight is 0) up to
    s[floor r_hi], ties included."""
    flat = dis.flatten(1)
    s = flat.sort(dim=1).values
    (l0, l1, lw), (h0, _h1, _hw) = selected_ranks(flat.shape[1])
    low = s[:, l1 if lw > 0 else l0]
    high = s[:, h0]
    return (dis >= low.view(-1, 1, 1)) & (dis <= high.view(-1, 1, 1))


def rank_gaps(gt: torch.Tensor) -> torch.Tensor:
    """[B, 4, 2]: for each of the four selected ranks k (floor / ceil of r_lo, floor / ceil of r_hi) of every row of
    gt [B,H,W,3], the relative gaps (s[k] - s[k-1]) / s[k] and (s[k+1] - s[k]) / s[k+1] to the order statistics
    either side (inf where there is none).  The mask boundaries lie between such neighbours."""
    s = _norms(gt).flatten(1).sort(dim=1).values
    n = s.shape[1]
    (l0, l1, _), (h0, h1, _) = selected_ranks(n)
    out = torch.full((s.shape[0], 4, 2), math.inf, dtype=torch.float64)
    for j, k in enumerate((l0, l1, h0, h1)):
        if k > 0:
            out[:, j, 0] = (s[:, k] - s[:, k - 1]) / s[:, k].clamp_min(1e-300)
        if k + 1 < n:
            out[:, j, 1] = (s[:, k + 1] - s[:, k]) / s[:, k + 1].clamp_min(1e-300)
    return out


def clip_gap(gt: torch.Tensor, dist_clip: float) -> float:
    """Smallest relative distance of a norm of gt to dist_clip."""
    return float(((_norms(gt) - dist_clip).abs() / dist_clip).min())


def decided(case: dict, tol: float = 1e-5) -> bool:
    """True when float32 rounding cannot move a point of `case` across a mask boundary (see the module docstring)."""
    if case.get("dist_clip") is not None:
        return min(clip_gap(case["gt_pts1"], case["dist_clip"]), clip_gap(case["gt_pts2"], case["dist_clip"])) >= tol
    return min(float(rank_gaps(case["gt_pts1"]).min()), float(rank_gaps(case["gt_pts2"]).min())) >= tol


def regr3d_ref(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1=None, conf2=None, *, dist_clip=None, disable_view1=False,
               norm_mode="avg_dis", gt_scale=False) -> dict:
    """Everything the tests compare, in float64: loss, grad (pr1, pr2), valid [2,B,H,W], n_valid [2,B], q [2,B,2],
    nf_pr [B], nf_gt [B], and the normalised prediction / target a, b ([2,B,H,W,3]) for the gradient tolerance."""
    if norm_mode and norm_mode != "avg_dis":
        raise NotImplementedError(norm_mode)
    gts = [gt_pts1.detach().double(), gt_pts2.detach().double()]
    prs = [pr_pts1.detach().double().clone().requires_grad_(True), pr_pts2.detach().double().clone().requires_grad_(True)]
    B = gts[0].shape[0]
    valid, qs = [], []
    for v, (g, c) in enumerate(zip(gts, (conf1, conf2))):
        dis = _norms(g)
        if dist_clip is not None:
            valid.append(dis <= dist_clip)
            qs.append(torch.tensor([0.0, float(dist_clip)], dtype=torch.float64).expand(B, 2))
        else:
            valid.append(rank_mask(dis) & (c.double() >= CONF_MIN))
            qs.append(thresholds(dis))
    n_valid = torch.stack([m.flatten(1).sum(1) for m in valid])                      # [2,B]
    cnt = n_valid.sum(0).double()
    den = torch.where(cnt > 0, cnt, torch.full_like(cnt, NF_MIN))

    def norm_factor(pts):
        tot = sum((torch.linalg.vector_norm(p, dim=-1) * m).flatten(1).sum(1) for p, m in zip(pts, valid))
        return (tot / den).clamp(min=NF_MIN)
    one = torch.ones(B, dtype=torch.float64)
    nf_pr = norm_factor(prs) if norm_mode else one
    nf_gt = norm_factor(gts) if (norm_mode and not gt_scale) else one
    a = [p / nf_pr.view(-1, 1, 1, 1) for p in prs]
    b = [g / nf_gt.view(-1, 1, 1, 1) for g in gts]
    losses = []
    for v in range(2):
        tot = (torch.linalg.vector_norm(a[v] - b[v], dim=-1) * valid[v]).sum()
        N = int(n_valid[v].sum())
        losses.append(tot / N if N > 0 else tot * 0.0 + math.nan)                   # the mean of nothing
    loss = losses[1] if disable_view1 else losses[0] + losses[1]
    g1, g2 = torch.autograd.grad(loss, prs, allow_unused=True)
    z = lambda g, p: torch.zeros_like(p) if g is None else g                         # noqa: E731
    return {"loss": loss.detach(), "grad": (z(g1, prs[0]), z(g2, prs[1])), "valid": torch.stack(valid),
            "n_valid": n_valid, "q": torch.stack(qs), "nf_pr": nf_pr.detach(), "nf_gt": nf_gt.detach(),
            "a": torch.stack([t.detach() for t in a]), "b": torch.stack(b)}


# ---- inputs --------------------------------------------------------------------------------------------------------

def make_case(seed: int, B: int, H: int, W: int, **opts) -> dict:
    """The seeded recipe: ground-truth points along random forward directions at log-uniform depths in [1, 20], with 1 %
    of the points nearer (down to 0.2) and 1 % farther (up to 200) -- the outliers the quantile mask is there for;
    predictions = ground truth * a per-item scale in [0.5, 2] + noise of ~5 % of the depth; confidences in [1, 9)
    (about a quarter below 3).  Float32, contiguous.  `opts` (dist_clip, disable_view1, norm_mode, gt_scale) ride along."""
    gen = torch.Generator().manual_seed(seed)

    def rand(*shape):
        return torch.rand(*shape, generator=gen, dtype=torch.float64)
    case = {}
    for v in (1, 2):
        xy = (rand(B, H, W, 2) - 0.5) * 1.2
        d = torch.cat([xy, torch.ones(B, H, W, 1, dtype=torch.float64)], -1)
        depth = torch.exp(rand(B, H, W) * math.log(20.0))
        u = rand(B, H, W)
        near = torch.exp(math.log(0.2) + rand(B, H, W) * (0.0 - math.log(0.2)))
        far = torch.exp(math.log(20.0) + rand(B, H, W) * (math.log(200.0) - math.log(20.0)))
        depth = torch.where(u < 0.01, near, torch.where(u > 0.99, far, depth))
        gt = d * depth[..., None]
        scale = 0.5 + 1.5 * rand(B, 1, 1, 1)
        pr = gt * scale + 0.05 * depth[..., None] * torch.randn(B, H, W, 3, generator=gen, dtype=torch.float64)
        case[f"gt_pts{v}"] = gt.float()
        case[f"pr_pts{v}"] = pr.float()
        case[f"conf{v}"] = (1.0 + 8.0 * rand(B, H, W)).float()
    case.update(seed=seed, dist_clip=None, disable_view1=False, norm_mode="avg_dis", gt_scale=False)
    case.update(opts)
    return case


def first_decided_case(B: int, H: int, W: int, start: int = 0, tries: int = 64, **opts) -> dict:
    """The first seed from `start` on whose masks are decided (decided()); the tests assert that it is."""
    for seed in range(start, start + tries):
        case = make_case(seed, B, H, W, **opts)
        if decided(case):
            return case
    raise AssertionError(f"no decided input among seeds {start} .. {start + tries - 1} at {(B, H, W)}")


def run_ref(case: dict) -> dict:
    return regr3d_ref(case["gt_pts1"], case["gt_pts2"], case["pr_pts1"], case["pr_pts2"], case["conf1"], case["conf2"],
                      dist_clip=case["dist_clip"], disable_view1=case["disable_view1"], norm_mode=case["norm_mode"],
                      gt_scale=case["gt_scale"])


def grad_tolerance(ref: dict, c: float) -> torch.Tensor:
    """[2,B,H,W,3]: (1e-4 + c 2^-24 (|a| + |b|) / |d|) m_i + 1e-6 M_b per component -- m_i the point's own largest
    gradient component, M_b the largest entry of its batch item and view, d = a - b (float32 carries the direction
    d / |d| only to eps (|a| + |b|) / |d|)."""
    a, b = ref["a"], ref["b"]
    want = torch.stack(ref["grad"])
    d = torch.linalg.vector_norm(a - b, dim=-1).clamp_min(1e-300)
    cancel = c * 2.0 ** -24 * (torch.linalg.vector_norm(a, dim=-1) + torch.linalg.vector_norm(b, dim=-1)) / d
    m = want.abs().amax(-1, keepdim=True)
    big = want.abs().flatten(2).amax(2).view(2, -1, 1, 1, 1)
    return ((1e-4 + cancel[..., None]) * m + 1e-6 * big).expand_as(want)
