"""Oracle of the VGGT attention (TEST INFRASTRUCTURE ONLY): a restatement of the reference's
``vggt/layers/attention.py:Attention.forward`` (lines 50-84) -- ``F.layer_norm`` of q and k (qk_norm), the 2-D rotation
(tests/attention_oracle.py:rope2d: VGGT's RotaryPositionEmbedding2D is the same formula as CroCo's fallback), ``scale * q k^T +
mask``, softmax, ``@ v`` -- dtype- and device-generic; the tests run it in float64 on the CPU and in float32 on the
device.  One definition the reference leaves to SDPA: a query row whose keys are ALL excluded (-inf) is zeros, and
autograd then gives it zero gradients.  Gradients come from autograd.

Pinned by tests/test_vggt_attention.py against tests/golden/vggt_attention_goldens.pt (outputs of the reference's own
class).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from tests.attention_oracle import rope2d


def view_positions(B: int, S: int, hh: int, ww: int, special: int) -> torch.Tensor:
    """Positions of S views of `special` + hh * ww tokens each, as aggregator.py:324-333 builds them: the patch grid's
    (y, x) plus one, the special tokens in front of it at (0, 0).  [B, S * P, 2] int64."""
    y, x = torch.meshgrid(torch.arange(hh), torch.arange(ww), indexing="ij")
    grid = torch.stack([y.reshape(-1), x.reshape(-1)], dim=-1) + 1
    view = torch.cat([torch.zeros(special, 2, dtype=grid.dtype), grid])
    return view.repeat(S, 1)[None].expand(B, -1, -1).clone().long()


def view_mask(S: int, P: int, num_target: int) -> torch.Tensor:
    """The global blocks' mask (aggregator.py:291-303 expanded as in 342-346): [1, 1, S*P, S*P] float32, -inf where the
    query's view is a context view (one of the first S - num_target) and the key's view is a target view, else 0."""
    view = torch.arange(S * P) // P
    ctx = S - num_target
    blocked = (view[:, None] < ctx) & (view[None, :] >= ctx)
    return torch.where(blocked, float("-inf"), 0.0).to(torch.float32)[None, None]


def _additive(mask, dtype):
    if mask is None:
        return None
    if mask.dtype == torch.bool:
        return torch.where(mask, 0.0, float("-inf")).to(dtype)
    return mask.to(dtype)


def attention_core(q, k, v, qpos=None, kpos=None, mask=None, q_norm=None, k_norm=None, base: float = 100.0,
                   scale: float | None = None, probe: dict | None = None, F0: float = 1.0):
    """q [B,H,Nq,D], k, v [B,H,Nk,D] -> [B,Nq,H*D].  q_norm / k_norm: (weight, bias, eps) or None; mask: additive or
    bool, broadcast to [B,H,Nq,Nk].  probe: a dict that receives the normalised k (``k_hat``, gradient retained) for
    ``k_bias_cancel_scale``."""
    B, H, Nq, D = q.shape
    if scale is None:
        scale = D ** -0.5
    if q_norm is not None:
        q = F.layer_norm(q, (D,), q_norm[0], q_norm[1], q_norm[2])
        k = F.layer_norm(k, (D,), k_norm[0], k_norm[1], k_norm[2])
        if probe is not None:
            k.retain_grad()
            probe["k_hat"] = k
    if qpos is not None:
        q = rope2d(q, qpos, base, F0)
        k = rope2d(k, kpos, base, F0)
    attn = (q @ k.transpose(-2, -1)) * scale
    m = _additive(mask, attn.dtype)
    if m is not None:
        attn = attn + m
        dead = (attn == float("-inf")).all(dim=-1, keepdim=True)           # every key excluded: the row is zeros
        attn = torch.where(dead, torch.zeros_like(attn), attn).softmax(dim=-1)
        attn = torch.where(dead, torch.zeros_like(attn), attn)
    else:
        attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, Nq, H * D)


def k_bias_cancel_scale(probe: dict) -> float:
    """Without a rotation the k bias adds the same q . beta to every key of a row, which the softmax cancels: its
    gradient sum_rows g[row, d] (g = the gradient with respect to the normalised k) is identically zero in exact
    arithmetic, and a float32 result is the rounding of that cancellation.  The scale "one ulp" then refers to is that
    of the terms that cancel, max_d sum_rows |g[row, d]| -- the analogue of test_gpu_attention.py:cancel_scales.  Call
    after the backward of a run that was given ``probe``."""
    return float(probe["k_hat"].grad.abs().sum(dim=(0, 1, 2)).max())


def core_with_grads(q, k, v, qpos, kpos, dout, mask=None, q_norm=None, k_norm=None, base: float = 100.0,
                    scale: float | None = None, dtype=torch.float64, probe: dict | None = None, F0: float = 1.0):
    """(out, dq, dk, dv, dq_weight, dq_bias, dk_weight, dk_bias) of attention_core evaluated in ``dtype`` on the inputs'
    device; the four parameter gradients are None without the norms."""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    leaves, norms = [q, k, v], (None, None)
    if q_norm is not None:
        params = [t.detach().to(dtype).requires_grad_(True) for t in (*q_norm[:2], *k_norm[:2])]
        norms = ((params[0], params[1], q_norm[2]), (params[2], params[3], k_norm[2]))
        leaves += params
    if mask is not None and mask.dtype != torch.bool:
        mask = mask.to(dtype)
    out = attention_core(q, k, v, qpos, kpos, mask, norms[0], norms[1], base, scale, probe, F0)
    out.backward(dout.to(dtype))
    grads = [t.grad for t in leaves]
    return (out.detach(),) + tuple(grads) + (None,) * (7 - len(grads))


def module_forward(x, pos, mask, w: dict, num_heads: int, base: float | None = 100.0, eps: float = 1e-5,
                   probe: dict | None = None):
    """``Attention.forward`` with the state dict ``w`` (keys qkv.*, q_norm.*, k_norm.*, proj.*; no q_norm.*: qk_norm
    off); base None: rope=None."""
    B, N, C = x.shape
    D = C // num_heads
    qkv = F.linear(x, w["qkv.weight"], w.get("qkv.bias")).reshape(B, N, 3, num_heads, D).permute(2, 0, 3, 1, 4)
    q, k, v = qkv.unbind(0)
    q_norm = k_norm = None
    if "q_norm.weight" in w:
        q_norm = (w["q_norm.weight"], w["q_norm.bias"], eps)
        k_norm = (w["k_norm.weight"], w["k_norm.bias"], eps)
    p = pos if base is not None else None
    y = attention_core(q, k, v, p, p, mask, q_norm, k_norm, base if base is not None else 100.0, D ** -0.5, probe)
    return F.linear(y, w["proj.weight"], w.get("proj.bias"))


def golden_case(gold: dict, name: str, dtype=torch.float64, probe: dict | None = None):
    """Evaluate one case of vggt_attention_goldens.pt with the oracle: (out, dx, {parameter name: gradient}).  The loss
    of the goldens is 0.5 * sum(out^2), i.e. the upstream gradient is the output itself."""
    case = gold["cases"][name]
    w = {k: v.to(dtype).requires_grad_(True) for k, v in gold["weights"].items()}
    x = gold["x"].to(dtype).requires_grad_(True)
    mask = gold["mask"].to(dtype) if case["mask"] else None
    out = module_forward(x, gold["pos"], mask, w, gold["num_heads"], gold["base"] if case["rope"] else None, gold["eps"],
                         probe)
    (0.5 * (out * out).sum()).backward()
    return out.detach(), x.grad, {k: v.grad for k, v in w.items()}
