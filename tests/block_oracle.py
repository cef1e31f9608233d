"""Oracle of the transformer block (TEST INFRASTRUCTURE ONLY): this project's own restatement of the three kernels of
csrc/block.hip -- add + LayerNorm, bias + GELU -- and of the three module forwards (``Block`` and ``DecoderBlock`` of
croco/blocks.py:115-131 / 181-203, ``Block`` of vggt/layers/block.py:81-107), dtype- and device-generic; the tests run it
in float64 on the CPU and in float32 as the eager stand-in.  Attention comes from tests/attention_oracle.py and
tests/vggt_attention_oracle.py; gradients from autograd.

``mut``: a set of names that turn the oracle into a WRONG one, for the power condition of the gates -- ``eps`` (1e-5 in
place of the module's 1e-6), ``unbiased`` (variance over C - 1), ``tanh`` (the tanh GELU), ``no_residual`` (r left out of
the add), ``no_gamma`` (gamma left out), ``no_bias`` (the bias left out of the GELU argument).

Pinned by tests/test_block.py against tests/golden/block_goldens_*.pt (outputs of the reference's own classes).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import attention_oracle, vggt_attention_oracle

MUTANTS = ("eps", "unbiased", "tanh", "no_residual", "no_gamma", "no_bias")
NONE = frozenset()
OTHER_EPS = 1e-5


def layer_norm(s, weight, bias, eps, mut=NONE):
    if "eps" in mut:
        eps = OTHER_EPS
    mean = s.mean(dim=-1, keepdim=True)
    d = s - mean
    n = s.shape[-1] - (1 if "unbiased" in mut else 0)
    var = (d * d).sum(dim=-1, keepdim=True) / n
    return d / torch.sqrt(var + eps) * weight + bias


def add_layer_norm(x, r, weight, bias, eps, gamma=None, mut=NONE):
    """(s, y): s = x + gamma * r, y = LayerNorm(s); r None: s is x."""
    s = x
    if r is not None and "no_residual" not in mut:
        s = x + (r * gamma if gamma is not None and "no_gamma" not in mut else r)
    return s, layer_norm(s, weight, bias, eps, mut)


def gelu(z, mut=NONE):
    if "tanh" in mut:
        return 0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z * z * z)))
    return 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))


def bias_gelu(u, bias, mut=NONE):
    return gelu(u if bias is None or "no_bias" in mut else u + bias, mut)


def _lin(x, w, prefix, bias=True):
    return F.linear(x, w[prefix + ".weight"], w.get(prefix + ".bias") if bias else None)


def _sub(w, prefix):
    return {k[len(prefix) + 1:]: v for k, v in w.items() if k.startswith(prefix + ".")}


def _ln(w, name):
    return w[name + ".weight"], w[name + ".bias"]


def mlp(x, w, mut=NONE):
    """``Mlp.forward`` with the state dict ``w`` (fc1.*, fc2.*)."""
    return _lin(bias_gelu(_lin(x, w, "fc1", bias=False), w.get("fc1.bias"), mut), w, "fc2")


def block(x, xpos, w, num_heads, eps, base=100.0, mut=NONE):
    a = attention_oracle.self_attention(layer_norm(x, *_ln(w, "norm1"), eps, mut), xpos, _sub(w, "attn"), num_heads, base)
    x, t = add_layer_norm(x, a, *_ln(w, "norm2"), eps, None, mut)
    return x + mlp(t, _sub(w, "mlp"), mut)


def decoder_block(x, y, xpos, ypos, w, num_heads, eps, base=100.0, mut=NONE):
    a = attention_oracle.self_attention(layer_norm(x, *_ln(w, "norm1"), eps, mut), xpos, _sub(w, "attn"), num_heads, base)
    y_ = layer_norm(y, *_ln(w, "norm_y"), eps, mut) if "norm_y.weight" in w else y
    x, t = add_layer_norm(x, a, *_ln(w, "norm2"), eps, None, mut)
    c = attention_oracle.cross_attention(t, y_, y_, xpos, ypos, _sub(w, "cross_attn"), num_heads, base)
    x, t = add_layer_norm(x, c, *_ln(w, "norm3"), eps, None, mut)
    return x + mlp(t, _sub(w, "mlp"), mut)


def vggt_block(x, pos, w, num_heads, eps, base=100.0, qk_eps=1e-5, mask=None, mut=NONE):
    a = vggt_attention_oracle.module_forward(layer_norm(x, *_ln(w, "norm1"), eps, mut), pos, mask, _sub(w, "attn"),
                                             num_heads, base, qk_eps)
    x, t = add_layer_norm(x, a, *_ln(w, "norm2"), eps, w.get("ls1.gamma"), mut)
    m = mlp(t, _sub(w, "mlp"), mut)
    return x + (m * w["ls2.gamma"] if "ls2.gamma" in w and "no_gamma" not in mut else m)


def module_case(gold: dict, dtype=torch.float64, device="cpu", mut=NONE, weights=None):
    """One golden evaluated with the oracle in ``dtype`` on ``device``: (out, {input: gradient}, {parameter: gradient});
    the loss is the goldens' 0.5 * sum(out^2).  ``weights``: the state dict where the golden's file does not hold it."""
    w = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in (weights or gold["weights"]).items()}
    ins = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in gold["inputs"].items()}
    pos = {k: v.to(device) for k, v in gold["pos"].items()}
    H, eps, base = gold["num_heads"], gold["eps"], gold["base"]
    if gold["kind"] == "block":
        out = block(ins["x"], pos["xpos"], w, H, eps, base, mut)
    elif gold["kind"] == "decoder":
        out = decoder_block(ins["x"], ins["y"], pos["xpos"], pos["ypos"], w, H, eps, base, mut)
    else:
        out = vggt_block(ins["x"], pos["pos"], w, H, eps, base, gold["qk_eps"], None, mut)
    leaves = {**ins, **w}
    grads = torch.autograd.grad(0.5 * (out * out).sum(), list(leaves.values()), allow_unused=bool(mut))
    grads = {k: (torch.zeros_like(leaves[k]) if t is None else t) for k, t in zip(leaves, grads)}
    return out.detach(), {k: grads[k] for k in ins}, {k: grads[k] for k in w}


# ---- the kernels with their gradients --------------------------------------------------------------------------------
NORM_NAMES = ("s", "y", "dx", "dr", "dweight", "dbias", "dgamma")
GELU_NAMES = ("h", "du", "db")


def norm_with_grads(x, r, weight, bias, eps, gamma, dy, ds, dtype=torch.float64, device="cpu", mut=NONE):
    """{name: tensor} over NORM_NAMES of add_layer_norm with upstream gradients dy (of y) and ds (of s, or None); the
    entries of absent operands (s, dr without r; dgamma without gamma) are left out."""
    cast = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)
    x, r, weight, bias, gamma = (None if t is None else cast(t).requires_grad_(True) for t in (x, r, weight, bias, gamma))
    s, y = add_layer_norm(x, r, weight, bias, eps, gamma, mut)
    loss = (y * cast(dy)).sum() + ((s * cast(ds)).sum() if ds is not None else 0.0)
    leaves = {"dx": x, "dr": r, "dweight": weight, "dbias": bias, "dgamma": gamma}
    leaves = {k: v for k, v in leaves.items() if v is not None}
    g = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    res = {"y": y.detach(), **{k: (torch.zeros_like(leaves[k]) if t is None else t) for k, t in zip(leaves, g)}}
    if r is not None:
        res["s"] = s.detach()
    return res


def gelu_with_grads(u, bias, dh, dtype=torch.float64, device="cpu", mut=NONE):
    """{h, du[, db]} of bias_gelu with upstream gradient dh."""
    cast = lambda t: t.detach().to(device=device, dtype=dtype)
    u = cast(u).requires_grad_(True)
    b = cast(bias).requires_grad_(True) if bias is not None else None
    h = bias_gelu(u, b, mut)
    g = torch.autograd.grad(h, [u] + ([b] if b is not None else []), cast(dh), allow_unused=True)
    res = {"h": h.detach(), "du": g[0]}
    if b is not None:
        res["db"] = torch.zeros_like(b) if g[1] is None else g[1]
    return res


def rel_err(got, want) -> float:
    """max|x - x64| / max|x64|"""
    return float((got.detach().double().cpu() - want.double().cpu()).abs().max()) / float(want.abs().max())
