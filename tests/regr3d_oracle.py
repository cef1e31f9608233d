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
|x| = 0 (vector_norm), nothing for invalid points, and both the direct term and the path through nf_pr.

The EXACT SIDE at the end of the file needs no such margin: for ground truth on the coordinate axes float64 and float32
form the same norms, and thresholds, masks and counts are restated in float32, bit for bit (see there)."""
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
               norm_mode="avg_dis", gt_scale=False, valid_override=None) -> dict:
    """Everything the tests compare, in float64: loss, grad (pr1, pr2), valid [2,B,H,W], n_valid [2,B], q [2,B,2],
    nf_pr [B], nf_gt [B], and the normalised prediction / target a, b ([2,B,H,W,3]) for the gradient tolerance.

    `valid_override` (two bool [B,H,W], the float32-exact masks of exact_truth()) replaces the masks by rank: the loss
    and the gradients are then taken over it.  Under it a ground-truth point outside the mask is read as (0, 0, 0): an
    invalid point contributes nothing, and 0 * inf or 0 * NaN must not say otherwise (nan_point, inf_point)."""
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
    if valid_override is not None:
        valid = [torch.as_tensor(m, dtype=torch.bool) for m in valid_override]
        assert all(m.shape == g.shape[:3] for m, g in zip(valid, gts))
        gts = [torch.where(m[..., None], g, torch.zeros_like(g)) for m, g in zip(valid, gts)]
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


def run_ref(case: dict, valid_override=None) -> dict:
    return regr3d_ref(case["gt_pts1"], case["gt_pts2"], case["pr_pts1"], case["pr_pts2"], case["conf1"], case["conf2"],
                      dist_clip=case["dist_clip"], disable_view1=case["disable_view1"], norm_mode=case["norm_mode"],
                      gt_scale=case["gt_scale"], valid_override=valid_override)


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


# ---- the exact side ------------------------------------------------------------------------------------------------
# For a ground-truth point on a coordinate axis the kernel's norm chain sqrtf(fmaf(z, z, fmaf(y, y, x * x))) is |c| bit
# for bit, c the one non-zero coordinate: x * x or the fmaf that meets c forms fl32(c^2), every other step adds an exact
# 0, and a correctly rounded square root takes fl(c^2) back to |c| away from overflow and underflow (build.py passes no
# fast-math flag).  The float64 norm of such a point is |c| as well, so on an input that passes is_exact() the oracle and
# the product see THE SAME norms: ties, thresholds and masks have one truth, in float32, and decided() is not needed.
# That truth is restated here on the host, in numpy float32, from the contract:
#     keys: the norms' bit patterns without the sign; NaN orders above +inf (the product's documented deviation from
#         torch.quantile, which returns NaN for a row that holds one);
#     rank r = float32(q) * float32(n - 1), weight w = r - floor r, q = aten's lerp of s[floor r], s[ceil r]:
#         w < 0.5 ? lo + w (hi - lo) : hi - (hi - lo) (1 - w), each multiply-add fused as torch's kernels fuse it;
#     valid = (dis >= q_lo) & (dis <= q_hi) & (conf >= 3), or dis <= dist_clip.
# Where the float32 lerp rounds q_lo onto s[floor r_lo] (neighbouring patterns), the floor statistic is valid although
# rank_mask() drops it: the float32 thresholds are the contract, not the ranks.
#
# MUTANTS restate one line each the wrong way; tests/test_regr3d_exact.py asserts that every one of them moves n_valid
# or the bits of q on a named case of tests/regr3d_cases.py (nf_per_view: the norm factors), except alias_last, which
# must move nothing.
MUTANTS = ("lo_strict", "hi_strict", "conf_strict", "clip_strict", "rank_n", "ceil_is_floor", "weight_zero",
           "lerp_one_sided", "alias_last", "alias_none_low", "nan_low", "nan_poisons", "nf_per_view")
RADIX_MUTANTS = ("alias_last", "alias_none_low")        # these live in the radix restatement of the select
RADIX_PASSES = ((31, 20, 2048), (20, 9, 2048), (9, 0, 512))   # (shift of the prefix, shift of the digit, bins)
_F4, _F8 = np.float32, np.float64


def norm32(gt: torch.Tensor) -> np.ndarray:
    """The kernel's norm chain on the host, float32 [...] of gt [...,3] (float32).  fmaf is formed in float64 -- the
    product of two float32 is exact there -- and rounded to float32: one rounding wherever the float64 sum is exact,
    which it is when the addend is 0 (every point on an axis)."""
    p = gt.detach().cpu().numpy()
    assert p.dtype == _F4 and p.shape[-1] == 3
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    with np.errstate(all="ignore"):
        t = x * x
        t = (y.astype(_F8) * y.astype(_F8) + t.astype(_F8)).astype(_F4)
        t = (z.astype(_F8) * z.astype(_F8) + t.astype(_F8)).astype(_F4)
        return np.sqrt(t)


def is_exact(gt: torch.Tensor) -> bool:
    """True when the float64 norm of every point of gt, rounded to float32, is norm32's (NaN equal to NaN): float64
    and float32 then order, tie and threshold the row alike."""
    return bool(np.array_equal(_norms(gt).float().numpy(), norm32(gt), equal_nan=True))


def keys32(dis32: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(dis32, dtype=_F4).view(np.uint32) & np.uint32(0x7FFFFFFF)


def ranks32(n: int, mut: str | None = None):
    """((floor, ceil, weight) of r_lo, the same of r_hi) with the weight as a float32."""
    m = _F4(n if mut == "rank_n" else n - 1)
    out = []
    for q in (Q_LO, Q_HI):
        r = _F4(q) * m
        lo = np.floor(r)
        hi = lo if mut == "ceil_is_floor" else np.ceil(r)
        out.append((min(int(lo), n - 1), min(int(hi), n - 1), _F4(r - lo)))
    return tuple(out)


def fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) on float32 arrays, exactly: a b is exact in float64, the float64 sum rounds once more than a fused
    operation does, and that shows only where the sum lands on the midpoint of two float32 -- there the part the float64
    sum lost (TwoSum) says which way the one true rounding goes."""
    a, b, c = (np.asarray(t, dtype=_F4).astype(_F8) for t in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        t = p + c
        bb = t - p
        e = (p - (t - bb)) + (c - bb)
        r = t.astype(_F4)
        away = np.nextafter(r, np.where(t > r.astype(_F8), _F4(np.inf), _F4(-np.inf)).astype(_F4))
        tie = np.isfinite(t) & np.isfinite(away) & (r.astype(_F8) != t) & ((r.astype(_F8) + away.astype(_F8)) / 2 == t) & (e != 0)
        up = np.maximum(r, away)
        return np.where(tie, np.where(e > 0, up, np.minimum(r, away)), r).astype(_F4)


def lerp32(lo: np.ndarray, hi: np.ndarray, w, mut: str | None = None) -> np.ndarray:
    """aten's lerp (Lerp.h) in float32: w < 0.5 ? lo + w (hi - lo) : hi - (hi - lo) (1 - w), the difference and 1 - w
    rounded, the multiply-add FUSED -- torch's kernels form it as one fmadd (the vectorised CPU path spells it out;
    the scalar and device paths get it from the compilers' default contraction)."""
    lo, hi, w = lo.astype(_F4), hi.astype(_F4), _F4(w)
    if mut == "weight_zero":
        return lo
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        out = fma32(w, d, lo) if (w < _F4(0.5) or mut == "lerp_one_sided") else fma32(-d, _F4(1.0) - w, hi)
    assert out.dtype == _F4
    return out


def radix_select32(keys: np.ndarray, wants, mut: str | None = None) -> list:
    """The product's select on one row of keys, restated: three passes over digits of 11, 11 and 9 bits; in each pass a
    rank whose prefix an EARLIER rank has reads that rank's counts (`alias`), and only the first rank of a prefix owns a
    histogram.  Returns the keys at the four wanted ranks.

    alias_last: a rank names the nearest earlier rank with its prefix, not the first, and takes what that one reads.
        Equal prefixes are transitive, so the chain ends at the first: a no-op (in the kernel a rank that does not own
        its prefix has an empty histogram, so the pick has to name the first directly; it does).
    alias_none_low: the ceiling of r_lo, where it shares the floor's prefix, carries on with the floor's rank inside it."""
    keys = keys.astype(np.int64)
    prefix, want = [0, 0, 0, 0], [int(w) for w in wants]
    for p, (pshift, dshift, bins) in enumerate(RADIX_PASSES):
        alias = []
        for t in range(4):
            same = [s for s in range(t) if prefix[s] == prefix[t]]
            alias.append(t if not same else (same[-1] if mut == "alias_last" else same[0]))
        hist = {}
        for t in range(4):
            if alias[t] == t:
                sel = keys if p == 0 else keys[(keys >> pshift) == prefix[t]]
                hist[t] = np.bincount((sel >> dshift) & (bins - 1), minlength=bins)
        if mut == "alias_none_low" and p > 0 and alias[1] == 0:
            want[1] = want[0]
        new_prefix, new_want = [], []
        for t in range(4):
            s = t
            while alias[s] != s:
                s = alias[s]
            cum = np.cumsum(hist[s])
            digit = int(np.searchsorted(cum, want[t], side="right"))
            assert digit < bins, "the row's counts add up to more than the rank"
            new_want.append(want[t] - (int(cum[digit - 1]) if digit else 0))
            new_prefix.append((prefix[t] << (pshift - dshift)) | digit)
        prefix, want = new_prefix, new_want
    assert want == [0, 0, 0, 0] or len(set(keys.tolist())) < len(keys)     # what is left is a rank inside a tie
    return prefix


def order_stats32(dis32: np.ndarray, mut: str | None = None, radix: bool = False):
    """(lo, hi, w) for q_lo and for q_hi of the rows dis32 [R, n]: the float32 order statistics at floor / ceil of the
    two ranks.  By a sort of the keys, or row by row through radix_select32."""
    R, n = dis32.shape
    k = keys32(dis32).astype(np.int64)
    nan = k > 0x7F800000
    (l0, l1, lw), (h0, h1, hw) = ranks32(n, mut)
    if radix:
        assert mut != "nan_low"
        picks = np.array([radix_select32(row, (l0, l1, h0, h1), mut) for row in k], dtype=np.int64).reshape(R, 4)
    else:
        s = np.sort(np.where(nan, -1, k) if mut == "nan_low" else k, axis=1)
        picks = s[:, [l0, l1, h0, h1]]
        picks = np.where(picks < 0, 0x7FC00000, picks)
    val = picks.astype(np.uint32).view(_F4)
    return (val[:, 0], val[:, 1], lw), (val[:, 2], val[:, 3], hw), nan.any(axis=1)


def thresholds32(dis32: np.ndarray, mut: str | None = None, radix: bool = False) -> np.ndarray:
    """[R, 2] float32: (q_lo, q_hi) of every row of dis32 [R, n], NaN keys ordered last."""
    lo, hi, has_nan = order_stats32(np.asarray(dis32), mut, radix)
    q = np.stack([lerp32(*lo, mut), lerp32(*hi, mut)], axis=1)
    if mut == "nan_poisons":
        q[has_nan] = np.nan
    return q


def valid32(dis32: np.ndarray, conf32, q32: np.ndarray, mut: str | None = None) -> np.ndarray:
    """(dis >= q_lo) & (dis <= q_hi) & (conf >= 3) in float32 for rows dis32 [R, n], q32 [R, 2]; conf32 None: the
    thresholds are (0, dist_clip) and only dis <= dist_clip is asked."""
    dis32, q32 = np.asarray(dis32, dtype=_F4), np.asarray(q32, dtype=_F4)
    with np.errstate(invalid="ignore"):
        hi = dis32 < q32[:, 1:2] if mut in ("hi_strict", "clip_strict") else dis32 <= q32[:, 1:2]
        if conf32 is None:
            return hi
        lo = dis32 > q32[:, 0:1] if mut == "lo_strict" else dis32 >= q32[:, 0:1]
        conf32 = np.asarray(conf32, dtype=_F4)
        return lo & hi & (conf32 > _F4(CONF_MIN) if mut == "conf_strict" else conf32 >= _F4(CONF_MIN))


def exact_truth(case: dict, mut: str | None = None, radix: bool = False) -> dict:
    """The float32-exact q [2,B,2] (numpy float32), valid [2,B,H,W] (torch bool) and n_valid [2,B] (torch int64) of a
    case whose ground truth passes is_exact()."""
    qs, valid = [], []
    for v in (1, 2):
        gt = case[f"gt_pts{v}"]
        B, H, W, _ = gt.shape
        dis = norm32(gt).reshape(B, H * W)
        if case["dist_clip"] is not None:
            q = np.tile(np.array([0.0, case["dist_clip"]], dtype=_F4), (B, 1))
            m = valid32(dis, None, q, mut)
        else:
            q = thresholds32(dis, mut, radix)
            m = valid32(dis, case[f"conf{v}"].numpy().reshape(B, H * W), q, mut)
        qs.append(q)
        valid.append(torch.from_numpy(m.reshape(B, H, W)))
    valid = torch.stack(valid)
    return {"q": np.stack(qs), "valid": valid, "n_valid": valid.flatten(2).sum(2)}


def select_patterns(keys: np.ndarray, n: int):
    """For one row's keys: which of the four selected ranks (floor, ceil of r_lo; floor, ceil of r_hi) share a prefix
    after pass 0 (key >> 20), after pass 1 (key >> 9) and at the end (the whole key), each as the kernel's alias
    pattern -- entry t is the first rank s <= t with an equal prefix.  The last digit separates what pass 1 left
    together where the third pattern differs from the second."""
    assert keys.shape == (n,)
    s = np.sort(keys.astype(np.int64))
    (l0, l1, _), (h0, h1, _) = ranks32(n)
    k = s[[l0, l1, h0, h1]]
    return tuple(tuple(next(a for a in range(t + 1) if k[a] >> sh == k[t] >> sh) for t in range(4)) for sh in (20, 9, 0))


def norm_factors64(pts, valid, per_view: bool = False) -> torch.Tensor:
    """nf of the contract in float64 for two point maps [B,H,W,3] under two masks [B,H,W]: [B] jointly over the views;
    per_view (the mutant nf_per_view): [2,B], each view over its own valid points."""
    tot = torch.stack([torch.where(m, torch.linalg.vector_norm(p.double(), dim=-1), torch.zeros(())).flatten(1).sum(1)
                       for p, m in zip(pts, valid)])
    cnt = torch.stack([m.flatten(1).sum(1) for m in valid]).double()
    if not per_view:
        tot, cnt = tot.sum(0), cnt.sum(0)
    return (tot / torch.where(cnt > 0, cnt, torch.full_like(cnt, NF_MIN))).clamp(min=NF_MIN)
