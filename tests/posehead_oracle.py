"""Oracle of the pose heads (TEST INFRASTRUCTURE ONLY): this project's own restatement of the six kernels of
csrc/posehead.hip -- token pool, the head's tail, embed + SiLU, the adaptive LayerNorm, attention over the views,
accumulate + activate -- and of the two modules built on them (``PoseHead`` of heads/pose_head.py, ``CameraHead`` of
vggt/heads/camera_head.py), dtype- and device-generic; the tests run it in float64 on the CPU and in float32 as the eager
stand-in.  Gradients come from autograd.

``mut``: a set of names that turn the oracle into a WRONG one, for the power condition of the gates:
  pool      ``sum_not_mean`` (the tokens summed, not averaged), ``dec_first`` (decoder channels in front)
  encode    ``beta_one`` (softplus with beta 1), ``no_clamp`` (h not clamped), ``clamp_min_scale`` (h clamped at
            min_scale = 0.01 in place of 1 / min_scale)
  embed     ``sigmoid_only`` (sigmoid(z) in place of z sigmoid(z)), ``no_bias``
  modulate  ``eps`` (1e-5 in place of 1e-6), ``unbiased`` (variance over C - 1), ``scale_without_one`` (n * scale),
            ``no_gate``, ``no_residual``
  attention ``scale`` (1 / D in place of D^-1/2), ``softmax_over_queries``
  activate  ``relu_everywhere`` (every slice through relu), ``no_accumulate`` (the previous encoding left out)

Pinned by tests/test_posehead.py against tests/golden/posehead_goldens_*.pt (outputs of the reference's own classes).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from tests import block_oracle as bo

MUTANTS = ("sum_not_mean", "dec_first", "beta_one", "no_clamp", "clamp_min_scale", "sigmoid_only", "no_bias", "eps",
           "unbiased", "scale_without_one", "no_gate", "no_residual", "scale", "softmax_over_queries", "relu_everywhere",
           "no_accumulate")
NONE = frozenset()
ADALN_EPS = 1e-6
OTHER_EPS = 1e-5
MAX_SCALE, MIN_SCALE = 4.0, 0.01
HOMOG = (math.log(2) / (1.0 - 1.0 / MAX_SCALE), 1.0 / MAX_SCALE, 1.0 / MIN_SCALE)      # beta, max_inv_scale, min_inv_scale
rel_err = bo.rel_err


# ---- the kernels -----------------------------------------------------------------------------------------------------
def pool(dec, enc=None, mut=NONE):
    """dec [.., L, C] (enc [.., L, C'] or None) -> [.., C' + C]"""
    x = dec if enc is None else torch.cat([dec, enc] if "dec_first" in mut else [enc, dec], dim=-1)
    if x.shape[-2] == 1:
        return x[..., 0, :]
    return x.sum(dim=-2) if "sum_not_mean" in mut else x.mean(dim=-2)


def softplus(x, beta):
    """torch's form: linear where beta x > 20"""
    z = x * beta
    return torch.where(z > 20.0, x, torch.log1p(torch.exp(torch.clamp(z, max=20.0))) / beta)


def encode(rot, t, homog=None, mut=NONE):
    """rot [.., 6], t [.., 3 or 4] -> [.., 9]; homog: (beta, max_inv_scale, min_inv_scale) or None"""
    if homog is not None:
        beta, max_inv, min_inv = homog
        h = softplus(t[..., 3:4], 1.0 if "beta_one" in mut else beta) + max_inv
        if "no_clamp" not in mut:
            h = torch.clamp(h, max=MIN_SCALE if "clamp_min_scale" in mut else min_inv)
        t = t[..., :3] / h
    return torch.cat([rot, t], dim=-1)


def embed_silu(p, weight, bias, mut=NONE):
    z = p @ weight.transpose(0, 1)
    if "no_bias" not in mut:
        z = z + bias
    s = torch.sigmoid(z)
    return s if "sigmoid_only" in mut else z * s


def modulate(x, mod, eps=ADALN_EPS, mut=NONE):
    c = x.shape[-1]
    shift, scale, gate = mod[..., :c], mod[..., c:2 * c], mod[..., 2 * c:]
    if "eps" in mut:
        eps = OTHER_EPS
    d = x - x.mean(dim=-1, keepdim=True)
    var = (d * d).sum(dim=-1, keepdim=True) / (c - (1 if "unbiased" in mut else 0))
    n = d / torch.sqrt(var + eps)
    m = n * (scale if "scale_without_one" in mut else 1.0 + scale) + shift
    if "no_gate" not in mut:
        m = gate * m
    return m if "no_residual" in mut else m + x


def attention(qkv, num_heads: int, mut=NONE):
    """packed qkv [B, S, 3 H D] -> [B, S, H D]"""
    B, S, _ = qkv.shape
    d = qkv.shape[-1] // (3 * num_heads)
    q, k, v = qkv.reshape(B, S, 3, num_heads, d).permute(2, 0, 3, 1, 4)
    a = (q @ k.transpose(-2, -1)) * (1.0 / d if "scale" in mut else d ** -0.5)
    a = torch.softmax(a, dim=-2 if "softmax_over_queries" in mut else -1)
    return (a @ v).transpose(1, 2).reshape(B, S, num_heads * d)


def _act(y, name):
    if name == "linear":
        return y
    if name == "inv_log":
        return torch.sign(y) * torch.expm1(torch.abs(y))
    if name == "exp":
        return torch.exp(y)
    if name == "relu":
        return torch.relu(y)
    raise ValueError(name)


def activate(prev, delta, acts=("linear", "linear", "linear"), mut=NONE):
    """(pred, out)"""
    pred = delta if prev is None or "no_accumulate" in mut else prev.detach() + delta
    if "relu_everywhere" in mut:
        acts = ("relu",) * 3
    out = torch.cat([_act(pred[..., :3], acts[0]), _act(pred[..., 3:7], acts[1]), _act(pred[..., 7:], acts[2])], dim=-1)
    return pred, out


# ---- the kernels with their gradients --------------------------------------------------------------------------------
def with_grads(fn, leaves: dict, consts: dict, ups, dtype=torch.float64, device="cpu"):
    """``fn(**tensors)`` -> a tensor or a tuple of tensors named ``out0, out1, ..`` (one: ``out``); upstream gradients
    ``ups`` (one per output, None: that output gets none); returns {out.., d_<leaf>..}."""
    cast = lambda t: None if t is None else t.detach().to(device=device, dtype=dtype)
    lv = {k: cast(v).requires_grad_(True) for k, v in leaves.items() if v is not None}
    outs = fn(**lv, **{k: (cast(v) if isinstance(v, torch.Tensor) else v) for k, v in consts.items()})
    single = isinstance(outs, torch.Tensor)
    outs = (outs,) if single else tuple(outs)
    loss = sum((o * cast(u)).sum() for o, u in zip(outs, ups) if u is not None)
    g = torch.autograd.grad(loss, list(lv.values()), allow_unused=True)
    res = {("out" if single else f"out{i}"): o.detach() for i, o in enumerate(outs)}
    res.update({"d_" + k: (torch.zeros_like(lv[k]) if t is None else t) for k, t in zip(lv, g)})
    return res


# ---- the modules -----------------------------------------------------------------------------------------------------
def _lin(x, w, prefix):
    return F.linear(x, w[prefix + ".weight"], w.get(prefix + ".bias"))


def pose_head(tokens, w, cfg: dict, mut=NONE):
    """``PoseHead.forward`` with the state dict ``w``: tokens = [enc, .., dec], each [.., L, C] -> [.., 9]"""
    feat = pool(tokens[-1], tokens[0] if cfg["concat_enc"] else None, mut)
    feat = torch.relu(_lin(torch.relu(_lin(feat, w, "more_mlps.0")), w, "more_mlps.2"))
    return encode(_lin(feat, w, "fc_rot"), _lin(feat, w, "fc_t"), HOMOG if cfg["use_homogeneous"] else None, mut)


def trunk_block(x, w, num_heads, eps, mut=NONE):
    """``Block`` of vggt/layers/block.py with plain attention (no rope, no q / k norm, no mask)"""
    a = _lin(attention(_lin(bo.layer_norm(x, w["norm1.weight"], w["norm1.bias"], eps), w, "attn.qkv"), num_heads, mut),
             w, "attn.proj")
    x = x + a * w["ls1.gamma"]
    m = bo.mlp(bo.layer_norm(x, w["norm2.weight"], w["norm2.bias"], eps), bo._sub(w, "mlp"))
    return x + m * w["ls2.gamma"]


def camera_head(tokens, w, cfg: dict, num_iterations: int, mut=NONE):
    """``CameraHead.forward`` with the state dict ``w``: tokens [B, S, N, C] -> a list of [B, S, 9]"""
    eps, H, depth = 1e-5, cfg["num_heads"], cfg["trunk_depth"]
    acts = (cfg["trans_act"], cfg["quat_act"], cfg["fl_act"])
    pose_tokens = bo.layer_norm(tokens[:, :, 0], w["token_norm.weight"], w["token_norm.bias"], eps)
    B, S, _ = pose_tokens.shape
    pred, outs = None, []
    for _ in range(num_iterations):
        p = w["empty_pose_tokens"].expand(B, S, -1) if pred is None else pred.detach()
        mod = _lin(embed_silu(p, w["embed_pose.weight"], w["embed_pose.bias"], mut), w, "poseLN_modulation.1")
        x = modulate(pose_tokens, mod, ADALN_EPS, mut)
        for i in range(depth):
            x = trunk_block(x, bo._sub(w, f"trunk.{i}"), H, eps, mut)
        delta = bo.mlp(bo.layer_norm(x, w["trunk_norm.weight"], w["trunk_norm.bias"], eps), bo._sub(w, "pose_branch"))
        pred, out = activate(pred, delta, acts, mut)
        outs.append(out)
    return outs


def module_case(gold: dict, dtype=torch.float64, device="cpu", mut=NONE):
    """One golden evaluated with the oracle: (outputs as a list, {input: gradient}, {parameter: gradient}); the loss is
    the goldens' 0.5 * sum(out^2) over every output."""
    w = {k: v.to(device=device, dtype=dtype) for k, v in gold["weights"].items()}
    params = [k for k in w if k in gold["param_names"]]
    for k in params:
        w[k].requires_grad_(True)
    ins = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in gold["inputs"].items()}
    if gold["kind"] == "camera":
        outs = camera_head(ins["tokens"], w, gold["cfg"], gold["num_iterations"], mut)
    else:
        outs = [pose_head([ins[k] for k in gold["token_order"]], w, gold["cfg"], mut)]
    leaves = {**ins, **{k: w[k] for k in params}}
    grads = torch.autograd.grad(sum(0.5 * (o * o).sum() for o in outs), list(leaves.values()), allow_unused=True)
    grads = {k: (torch.zeros_like(leaves[k]) if t is None else t) for k, t in zip(leaves, grads)}
    return [o.detach() for o in outs], {k: grads[k] for k in ins}, {k: grads[k] for k in params}
