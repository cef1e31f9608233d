"""Oracle of the encoder tail (TEST INFRASTRUCTURE ONLY): this project's own restatement, in plain torch, of the lines of
the reference's encoder between its heads and its decoder (encoder_spfsplatv2.py:218-224, 240, 248-268, 296-321 with
map_pdf_to_opacity, :146-159, and UnifiedGaussianAdapter.forward, gaussian_adapter.py:122-150) -- the per-view
rearrange "b d h w -> b (h w) d", the stack over the views, sigmoid, the opacity map, the adapter and the rearranges to
[b, (v h w), ...] -- dtype- and device-generic: the tests run it in float64 on the CPU and in float32 as the eager
stand-in.  Gradients come from autograd.

The opacity map is written in the STABLE form, (1 - p)^e = exp(e logsigmoid(-x)) and p^(1/e) = exp(logsigmoid(x) / e):
finite, with finite gradients, for every finite logit.  ``opacity_naive`` is the reference's expression on
p = sigmoid(x); tests/test_tail.py pins the two to each other in float64 on [-12, 12].

``mut``: a set of names that turn the oracle into a WRONG one, for the power condition of the gates --
``inv_exponent`` (e and 1/e exchanged), ``no_half`` (the map without its factor 0.5), ``no_sigmoid`` (the logit, clipped
to [0, 1], taken for the probability), ``view_major`` (the Gaussians ordered pixel-then-view), ``channel_off_by_one``
(the adapter reads from channel 0, not 1), ``sh_transposed`` (the harmonics' channels read as [K, 3]), ``no_mask`` (the
harmonics unscaled), ``clamp_min`` (in place of clamp_max on the scales), ``eps_inside_sqrt`` (q / sqrt(|q|^2 + eps)).

Pinned by tests/test_tail.py against tests/golden/tail_goldens.pt (outputs of the reference's own adapter class and of
the body of its map_pdf_to_opacity).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

MUTANTS = ("inv_exponent", "no_half", "no_sigmoid", "view_major", "channel_off_by_one", "sh_transposed", "no_mask",
           "clamp_min", "eps_inside_sqrt")
NONE = frozenset()
OUTPUTS = ("means", "opacities", "scales", "rotations", "harmonics")


def sh_mask(sh_degree: int, dtype=torch.float32, device="cpu"):
    """gaussian_adapter.py:41-48, built in float32 like the reference's buffer, then cast."""
    mask = torch.ones(((sh_degree + 1) ** 2,), dtype=torch.float32)
    for degree in range(1, sh_degree + 1):
        mask[degree ** 2:(degree + 1) ** 2] = 0.1 * 0.25 ** degree
    return mask.to(device=device, dtype=dtype)


def opacity_stable(x, exponent: float, mut=NONE):
    e = 1.0 / exponent if "inv_exponent" in mut else exponent
    half = 1.0 if "no_half" in mut else 0.5
    if "no_sigmoid" in mut:
        p = x.clamp(0, 1)
        return half * (1 - (1 - p) ** e + p ** (1 / e))
    return half * (1 - torch.exp(e * F.logsigmoid(-x)) + torch.exp(F.logsigmoid(x) / e))


def opacity_naive(x, exponent: float):
    """encoder_spfsplatv2.py:159 on pdf = sigmoid(x) (:257), as written there."""
    pdf = x.sigmoid()
    return 0.5 * (1 - (1 - pdf) ** exponent + pdf ** (1 / exponent))


def tail(pts, raw, exponent: float, sh_degree: int, eps: float = 1e-8, mut=NONE, opacity=opacity_stable) -> dict:
    """pts: v tensors [b, h, w, 3]; raw: v tensors [b, 1 + 7 + 3K, h, w] -> {means [b, G, 3], opacities [b, G],
    scales [b, G, 3], rotations [b, G, 4], harmonics [b, G, 3, K]}, G = v h w."""
    K = (sh_degree + 1) ** 2
    b = raw[0].shape[0]
    rows = [r.flatten(2).transpose(1, 2) for r in raw]                 # "b d h w -> b (h w) d"
    g = torch.stack(rows, dim=1)                                       # [b, v, hw, C]
    pts_all = torch.stack(list(pts), dim=1).flatten(2, 3)              # [b, v, hw, 3]
    if "view_major" in mut:
        g, pts_all = g.transpose(1, 2), pts_all.transpose(1, 2)
    opacities = opacity(g[..., 0], exponent, mut) if opacity is opacity_stable else opacity(g[..., 0], exponent)
    params = g[..., 0:-1] if "channel_off_by_one" in mut else g[..., 1:]
    s = 0.001 * F.softplus(params[..., :3])
    scales = s.clamp_min(0.3) if "clamp_min" in mut else s.clamp_max(0.3)
    q = params[..., 3:7]
    if "eps_inside_sqrt" in mut:
        rotations = q / (q.square().sum(-1, keepdim=True) + eps).sqrt()
    else:
        rotations = q / (q.norm(dim=-1, keepdim=True) + eps)
    sh = params[..., 7:]
    if "sh_transposed" in mut:
        sh = sh.reshape(*sh.shape[:-1], K, 3).transpose(-1, -2)
    else:
        sh = sh.reshape(*sh.shape[:-1], 3, K)
    if "no_mask" not in mut:
        sh = sh * sh_mask(sh_degree, sh.dtype, sh.device)
    flat = lambda t: t.reshape(b, -1, *t.shape[3:])                    # "b v r ... -> b (v r) ..."
    return {"means": flat(pts_all), "opacities": flat(opacities), "scales": flat(scales), "rotations": flat(rotations),
            "harmonics": flat(sh)}


def tail_with_grads(pts, raw, ups: dict, exponent: float, sh_degree: int, eps: float = 1e-8, dtype=torch.float64,
                    device="cpu", mut=NONE, opacity=opacity_stable) -> dict:
    """The outputs and, for the upstream gradients ``ups`` ({output name: tensor}; an absent one is zero), the gradients
    ``d_raw`` [v, b, C, h, w] and ``d_pts`` [v, b, h, w, 3], detached, in ``dtype`` on ``device``."""
    pts = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in pts]
    raw = [t.detach().to(device=device, dtype=dtype).requires_grad_(True) for t in raw]
    out = tail(pts, raw, exponent, sh_degree, eps, mut, opacity)
    res = {k: v.detach() for k, v in out.items()}
    names = [k for k in OUTPUTS if ups.get(k) is not None]
    if names:
        grads = torch.autograd.grad([out[k] for k in names], pts + raw,
                                    [ups[k].to(device=device, dtype=dtype) for k in names], allow_unused=True)
        zero = lambda g, t: torch.zeros_like(t) if g is None else g
        v = len(pts)
        res["d_pts"] = torch.stack([zero(g, t) for g, t in zip(grads[:v], pts)])
        res["d_raw"] = torch.stack([zero(g, t) for g, t in zip(grads[v:], raw)])
    return res


def rel_err(got, want) -> float:
    """max|x - x64| / max|x64|; 0 where both are zero throughout, inf where only the oracle is."""
    if want.numel() == 0:
        return 0.0
    diff = float((got.detach().double().cpu() - want.double().cpu()).abs().max())
    scale = float(want.abs().max())
    if scale == 0.0:
        return 0.0 if diff == 0.0 else float("inf")
    return diff / scale
