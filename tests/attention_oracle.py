"""Oracle of the fused attention (TEST INFRASTRUCTURE ONLY): a restatement of the reference's
``Attention.forward`` (src/model/encoder/backbone/croco/blocks.py:94-113) and ``CrossAttention.forward``
(blocks.py:150-179, without a mask), dtype- and device-generic; the tests run it in float64 on the CPU.  The rotation
is oracle/rope_torch_ref.py's (the reference's RoPE2D fallback) restated with the compiled path's ``F0`` (``rope2d``);
gradients come from autograd.

Pinned by tests/test_attention.py against tests/golden/attention_goldens*.pt (outputs of the reference's own classes).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F


def rope2d(tokens_bhnd: torch.Tensor, positions: torch.Tensor, base: float = 100.0, F0: float = 1.0) -> torch.Tensor:
    """oracle/rope_torch_ref.py:rope2d_fallback with the frequency scale of the reference's compiled rotation: the angle
    of feature pair q of Q = D / 4 in each half is  pos * F0 / base^(q / Q)  (curope's ``fwd / powf(base, q / float(Q))``,
    kernels.cu:45, curope.cpp:35).  tokens [B,H,N,D], positions [B,N,2] int64 (y, x) -> new tensor [B,H,N,D].  As in the
    fallback's tables the angle is formed in float32 and only then cast to the tokens' dtype, so at F0 = 1 this is the
    fallback to the last bit (tests/test_attention_params.py); no table, so positions need no common maximum."""
    assert tokens_bhnd.shape[-1] % 4 == 0 and positions.dim() == 3 and positions.shape[-1] == 2
    half = tokens_bhnd.shape[-1] // 2
    exponent = torch.arange(0, half, 2, device=tokens_bhnd.device).float() / half
    inv_freq = float(F0) / (base ** exponent)                             # [half / 2] float32
    angle = (positions.to(inv_freq.dtype)[..., None] * inv_freq).to(tokens_bhnd.dtype)     # [B,N,2,half / 2]
    angle = torch.cat((angle, angle), dim=-1)[:, None]                    # [B,1,N,2,half]
    cos, sin = angle.cos(), angle.sin()

    def rot(t, c, s):
        t1, t2 = t[..., : half // 2], t[..., half // 2:]
        return t * c + torch.cat((-t2, t1), dim=-1) * s

    ty, tx = tokens_bhnd.chunk(2, dim=-1)
    return torch.cat((rot(ty, cos[..., 0, :], sin[..., 0, :]), rot(tx, cos[..., 1, :], sin[..., 1, :])), dim=-1)


def attention_core(q, k, v, qpos=None, kpos=None, base: float = 100.0, scale: float | None = None, F0: float = 1.0):
    """q [B,H,Nq,D], k, v [B,H,Nk,D] -> [B,Nq,H*D]: blocks.py:102-110 / 161-176."""
    B, H, Nq, D = q.shape
    if scale is None:
        scale = D ** -0.5
    if qpos is not None:
        q = rope2d(q, qpos, base, F0)
        k = rope2d(k, kpos, base, F0)
    attn = (q @ k.transpose(-2, -1)) * scale
    attn = attn.softmax(dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B, Nq, H * D)


def core_with_grads(q, k, v, qpos, kpos, dout, base: float = 100.0, scale: float | None = None, dtype=torch.float64,
                    F0: float = 1.0):
    """(out, dq, dk, dv) of attention_core evaluated in ``dtype`` on the inputs' device."""
    q, k, v = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v))
    out = attention_core(q, k, v, qpos, kpos, base, scale, F0)
    dq, dk, dv = torch.autograd.grad(out, (q, k, v), dout.to(dtype))
    return out.detach(), dq, dk, dv


def _lin(x, w, prefix):
    return F.linear(x, w[prefix + ".weight"], w.get(prefix + ".bias"))


def self_attention(x, xpos, w: dict, num_heads: int, base: float | None = 100.0, F0: float = 1.0):
    """``Attention.forward`` with the state dict ``w`` (keys qkv.*, proj.*); base None: rope=None."""
    B, N, C = x.shape
    qkv = _lin(x, w, "qkv").reshape(B, N, 3, num_heads, C // num_heads).transpose(1, 3)
    q, k, v = [qkv[:, :, i] for i in range(3)]
    pos = xpos if base is not None else None
    y = attention_core(q, k, v, pos, pos, base if base is not None else 100.0, (C // num_heads) ** -0.5, F0)
    return _lin(y, w, "proj")


def cross_attention(query, key, value, qpos, kpos, w: dict, num_heads: int, base: float | None = 100.0,
                    F0: float = 1.0):
    """``CrossAttention.forward`` (mask=None) with the state dict ``w`` (keys projq.*, projk.*, projv.*, proj.*)."""
    B, Nq, C = query.shape
    D = C // num_heads
    q = _lin(query, w, "projq").reshape(B, Nq, num_heads, D).permute(0, 2, 1, 3)
    k = _lin(key, w, "projk").reshape(B, key.shape[1], num_heads, D).permute(0, 2, 1, 3)
    v = _lin(value, w, "projv").reshape(B, value.shape[1], num_heads, D).permute(0, 2, 1, 3)
    if base is None:
        qpos = kpos = None
    y = attention_core(q, k, v, qpos, kpos, base if base is not None else 100.0, D ** -0.5, F0)
    return _lin(y, w, "proj")


def golden_case(case: dict, dtype=torch.float64):
    """Evaluate one case of attention_goldens*.pt with the oracle: (out, {input name: gradient}).  The loss of the
    goldens is 0.5 * sum(out^2), i.e. the upstream gradient is the output itself."""
    w = {k: v.to(dtype) for k, v in case["weights"].items()}
    base = case["base"]
    ins = {k: case[k].to(dtype).requires_grad_(True) for k in case["inputs"]}
    if case["kind"] == "self":
        out = self_attention(ins["x"], case["xpos"], w, case["num_heads"], base)
    else:
        out = cross_attention(ins["query"], ins["memory"], ins["memory"], case["qpos"], case["kpos"], w,
                              case["num_heads"], base)
    grads = torch.autograd.grad(0.5 * (out * out).sum(), list(ins.values()))
    return out.detach(), dict(zip(ins, grads))
