"""The transformer block on the HIP library: the row work between the GEMMs, and the block modules on top of it.

=====================  =================================================================================
here                   reference
=====================  =================================================================================
``layer_norm``         ``nn.LayerNorm`` (``norm1``, ``norm_y``)
``add_layer_norm``     a residual add and the norm that follows it: ``x = x + r; norm2(x)`` -- with ``gamma`` VGGT's
                       ``x = x + ls1(r)``
``bias_gelu``          ``fc1``'s bias add and ``nn.GELU()`` of ``Mlp``
``Mlp``                croco/blocks.py:58-79 (and vggt/layers/mlp.py: same parameters)
``Block``              croco/blocks.py:115-131
``DecoderBlock``       croco/blocks.py:181-203
``LayerScale``         vggt/layers/layer_scale.py
``VGGTBlock``          ``Block`` of vggt/layers/block.py:27-107 (``forward``; not ``forward_nested``)
=====================  =================================================================================

Kernels: csrc/block.hip.  float32 only (the reference runs these layers in float32); C a multiple of 4 in 4 .. 4096; no
CPU path; no dropout and no stochastic depth in training mode -- each of these raises before anything is launched.  The
GEMMs stay ``nn.Linear``.  The gradients of the norm weights, norm biases, ``gamma`` and the MLP bias come out of the same
pass that produces the gradient of the tokens, summed without atomics: two runs agree bitwise.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._checks import check_device as _check_device, check_float32 as _check_float32
from .attention import Attention, CrossAttention
from .vggt_attention import VGGTAttention

MAX_C = _lib.BLOCK_MAX_C


# ---- checks --------------------------------------------------------------------------------------------------------
def _check_width(what: str, c: int) -> None:
    if c % 4 != 0 or not 4 <= c <= MAX_C:
        raise ValueError(f"{what}: the row width must be a multiple of 4 in 4 .. {MAX_C}, got {c}")


def _check_vector(what: str, name: str, v, c: int) -> None:
    if tuple(v.shape) != (c,):
        raise RuntimeError(f"{what}: {name} must have shape [{c}], got {list(v.shape)}")


def _check_norm_call(what, x, r, weight, bias, gamma) -> None:
    _check_float32(what, x, r, weight, bias, gamma)
    if x.dim() < 1 or x.numel() == 0:
        raise RuntimeError(f"{what}: x must have at least one row, got shape {list(x.shape)}")
    c = x.shape[-1]
    _check_width(what, c)
    if gamma is not None and r is None:
        raise ValueError(f"{what}: gamma is given without r")
    if r is not None and r.shape != x.shape:
        raise RuntimeError(f"{what}: x {list(x.shape)} and r {list(r.shape)} differ in shape")
    for name, v in (("weight", weight), ("bias", bias), ("gamma", gamma)):
        if v is not None:
            _check_vector(what, name, v, c)
    _check_device(what, x, r, weight, bias, gamma)


# ---- rows read in place ----------------------------------------------------------------------------------------------
def _groups(t: torch.Tensor):
    """The leading dimensions of ``t`` [.., C] as (size, stride) groups: neighbours that one stride walks are merged."""
    out = []
    for n, s in zip(t.shape[:-1], t.stride()[:-1]):
        if n == 1:
            continue
        if out and out[-1][1] == n * s:
            out[-1] = (out[-1][0] * n, s)
        else:
            out.append((n, s))
    return out


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` itself when the kernels can read its rows in place -- unit stride along C, a 16-byte aligned base, the rows
    addressed by at most two strides that are multiples of 4 floats (a [B, N, C] slice of a [B, V, N, C] tensor) --, else
    a contiguous copy."""
    if (t.stride(-1) == 1 or t.shape[-1] == 1) and t.data_ptr() % 16 == 0:
        g = _groups(t)
        if len(g) <= 2 and all(s >= 0 and s % 4 == 0 for _, s in g):
            return t
    return t.contiguous()


def _row_map(t: torch.Tensor):
    """(inner, stride, outer_stride) of a tensor ``_rows`` returned."""
    g = _groups(t)
    if not g:
        return 1, 0, 0
    if len(g) == 1:
        return g[0][0], g[0][1], 0
    return g[1][0], g[1][1], g[0][1]


def _norm_args(x, r, gamma, weight, bias, eps) -> _lib.SpfBlockNorm:
    a = _lib.SpfBlockNorm()
    a.x = x.data_ptr()
    a.x_inner, a.x_stride, a.x_outer_stride = _row_map(x)
    if r is not None:
        a.r = r.data_ptr()
        a.r_inner, a.r_stride, a.r_outer_stride = _row_map(r)
    else:
        a.r_inner = 1
    a.gamma, a.weight, a.bias = _lib.ptr(gamma), weight.data_ptr(), _lib.ptr(bias)
    a.rows, a.C, a.eps = x.numel() // x.shape[-1], x.shape[-1], float(eps)
    return a


def partial_blocks(rows: int, c: int, gelu: bool = False) -> int:
    """Rows of the partial workspace of the norm backward (or the GELU backward): the library's grid arithmetic.  Host
    only."""
    n = _lib.load().spf_block_partial_blocks(int(rows), int(c), int(bool(gelu)))
    if n < 0:
        raise _lib.SpfError("spf_block_partial_blocks rejected the sizes: " + _lib.load().spf_last_error().decode())
    return int(n)


# ---- launches --------------------------------------------------------------------------------------------------------
def add_norm_forward(x, r, weight, bias, eps, gamma=None):
    """The forward launch: (s or None, y, stats [rows, 4] = the two parts of the mean, 1 / std and a pad per row).  x and
    r are read in place where ``_rows`` allows."""
    _check_norm_call("add_layer_norm", x, r, weight, bias, gamma)
    if bias is None or weight is None:
        raise RuntimeError("add_layer_norm: weight and bias are required")
    x, r = _rows(x), (_rows(r) if r is not None else None)
    weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
    gamma = gamma.detach().contiguous() if gamma is not None else None
    rows = x.numel() // x.shape[-1]
    s = torch.empty(x.shape, dtype=x.dtype, device=x.device) if r is not None else None
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    stats = torch.empty(rows, 4, dtype=torch.float32, device=x.device)
    _lib.launch("spf_block_add_norm_forward", x.device, _norm_args(x, r, gamma, weight, bias, eps), s, y, stats)
    return s, y, stats


def add_norm_backward(sx, r, weight, gamma, stats, dy, ds, eps):
    """The backward launches on what the forward saved (sx: its s, or its x where it had no r; r only with gamma):
    (dx, dr or None, dparams [K, C] = dweight, dbias[, dgamma])."""
    _check_norm_call("add_layer_norm", sx, r if gamma is not None else None, weight, None, gamma)
    _check_float32("add_layer_norm", dy, ds)
    if dy.shape != sx.shape or (ds is not None and ds.shape != sx.shape):
        raise RuntimeError("add_layer_norm: the gradients must have the shape of the tokens")
    sx, dy = _rows(sx), dy.contiguous()
    ds = ds.contiguous() if ds is not None else None
    r = _rows(r) if gamma is not None else None
    weight = weight.detach().contiguous()
    gamma = gamma.detach().contiguous() if gamma is not None else None
    c = sx.shape[-1]
    rows = sx.numel() // c
    kinds = 3 if gamma is not None else 2
    dx = torch.empty(sx.shape, dtype=sx.dtype, device=sx.device)
    dr = torch.empty(sx.shape, dtype=sx.dtype, device=sx.device) if gamma is not None else None
    partials = torch.empty(kinds * partial_blocks(rows, c) * c, dtype=torch.float32, device=sx.device)
    dparams = torch.empty(kinds, c, dtype=torch.float32, device=sx.device)
    _lib.launch("spf_block_add_norm_backward", sx.device, _norm_args(sx, r, gamma, weight, None, eps), dy, ds, stats,
                dx, dr, partials, dparams)
    return dx, dr, dparams


def _check_gelu_call(u, bias) -> None:
    what = "bias_gelu"
    _check_float32(what, u, bias)
    if u.dim() < 1 or u.numel() == 0:
        raise RuntimeError(f"{what}: u must have at least one row, got shape {list(u.shape)}")
    _check_width(what, u.shape[-1])
    if bias is not None:
        _check_vector(what, "bias", bias, u.shape[-1])
    _check_device(what, u, bias)


def gelu_forward(u, bias):
    _check_gelu_call(u, bias)
    u = u.contiguous()
    bias = bias.detach().contiguous() if bias is not None else None
    h = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    _lib.launch("spf_block_bias_gelu_forward", u.device, u, bias, u.numel() // u.shape[-1], u.shape[-1], h)
    return h


def gelu_backward(u, bias, dh):
    """(du, dbias or None)"""
    _check_gelu_call(u, bias)
    _check_float32("bias_gelu", dh)
    if dh.shape != u.shape:
        raise RuntimeError("bias_gelu: the gradient must have the shape of u")
    u, dh = u.contiguous(), dh.contiguous()
    c = u.shape[-1]
    rows = u.numel() // c
    du = torch.empty(u.shape, dtype=u.dtype, device=u.device)
    partials = dbias = None
    if bias is not None:
        bias = bias.detach().contiguous()
        partials = torch.empty(partial_blocks(rows, c, True) * c, dtype=torch.float32, device=u.device)
        dbias = torch.empty(c, dtype=torch.float32, device=u.device)
    _lib.launch("spf_block_bias_gelu_backward", u.device, u, bias, dh, rows, c, du, partials, dbias)
    return du, dbias


# ---- autograd --------------------------------------------------------------------------------------------------------
class _AddLayerNorm(torch.autograd.Function):
    """r, gamma: None where absent.  Returns y without r, (s, y) with."""

    @staticmethod
    def forward(ctx, x, r, weight, bias, gamma, eps):
        s, y, stats = add_norm_forward(x, r, weight, bias, eps, gamma)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x if r is None else s, r if gamma is not None else None, weight, gamma, stats)
        ctx.has_r = r is not None
        ctx.eps = eps
        return y if r is None else (s, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        sx, r, weight, gamma, stats = ctx.saved_tensors
        ds, dy = grads if ctx.has_r else (None, grads[0])
        if dy is None and ds is None:
            return (None,) * 6
        if dy is None:
            dy = torch.zeros_like(sx)
        dx, dr, dparams = add_norm_backward(sx, r, weight, gamma, stats, dy, ds, ctx.eps)
        need = ctx.needs_input_grad
        return (dx if need[0] else None, (dr if gamma is not None else dx) if ctx.has_r and need[1] else None,
                dparams[0] if need[2] else None, dparams[1] if need[3] else None,
                dparams[2] if gamma is not None and need[4] else None, None)


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, bias):
        h = gelu_forward(u, bias)
        ctx.save_for_backward(u, bias)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        u, bias = ctx.saved_tensors
        du, dbias = gelu_backward(u, bias, dh)
        return du if ctx.needs_input_grad[0] else None, dbias if bias is not None and ctx.needs_input_grad[1] else None


def layer_norm(x, weight, bias, eps: float = 1e-5):
    """``F.layer_norm(x, (C,), weight, bias, eps)`` over the last dimension of ``x`` [.., C], float32.  A view whose rows
    two strides address (``tok[:, i]`` of a [B, V, N, C] tensor) is read in place."""
    _check_norm_call("layer_norm", x, None, weight, bias, None)
    return _AddLayerNorm.apply(x, None, weight, bias, None, float(eps))


def add_layer_norm(x, r, weight, bias, eps: float = 1e-5, gamma=None):
    """``s = x + r`` (``x + gamma * r`` with ``gamma`` [C], VGGT's LayerScale) and ``y = F.layer_norm(s, ..)`` in one pass:
    returns ``(s, y)``.  The backward produces the gradient of the residual stream once -- it is the gradient of x and,
    without gamma, of r: one tensor, no copy -- and the gradients of weight, bias and gamma in the same pass."""
    if r is None:
        raise ValueError("add_layer_norm: r is required (layer_norm is the call without it)")
    _check_norm_call("add_layer_norm", x, r, weight, bias, gamma)
    return _AddLayerNorm.apply(x, r, weight, bias, gamma, float(eps))


def bias_gelu(u, bias=None):
    """``GELU(u + bias)``, the exact (erf) form of ``nn.GELU()``; bias [C] or None.  Only u is saved for the backward,
    which also produces the bias gradient."""
    _check_gelu_call(u, bias)
    return _BiasGelu.apply(u, bias)


# ---- modules ---------------------------------------------------------------------------------------------------------
class DropPath(nn.Module):
    """Stochastic depth, kept for the modules' attributes: the identity in eval mode and at rate 0; the blocks refuse a
    positive rate in training mode."""

    def __init__(self, drop_prob: float = 0., scale_by_keep: bool = True):
        super().__init__()
        self.drop_prob = drop_prob
        self.scale_by_keep = scale_by_keep

    def forward(self, x):
        if self.training and self.drop_prob > 0.:
            raise NotImplementedError("drop_path > 0 in training mode is not supported by the fused block")
        return x

    def extra_repr(self):
        return f"drop_prob={round(self.drop_prob, 3):0.3f}"


class LayerScale(nn.Module):
    """vggt/layers/layer_scale.py: ``x * gamma``.  Inside ``VGGTBlock`` the multiplication rides in the fused add."""

    def __init__(self, dim: int, init_values=1e-5, inplace: bool = False) -> None:
        super().__init__()
        self.inplace = inplace
        self.gamma = nn.Parameter(init_values * torch.ones(dim))

    def forward(self, x):
        return x.mul_(self.gamma) if self.inplace else x * self.gamma


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _layer_norm_of(layer, dim: int, owner: str):
    """The module's norm, checked: an ``nn.LayerNorm`` over the ``dim`` elements of a row with weight and bias."""
    if not (type(layer) is nn.LayerNorm and tuple(layer.normalized_shape) == (dim,) and layer.weight is not None
            and layer.bias is not None):
        raise TypeError(f"{owner}: norm_layer must build an nn.LayerNorm over the {dim} elements of a row with weight and "
                        f"bias, got {layer!r}")
    return layer


def _norm(layer):
    return layer.weight, layer.bias, layer.eps


def _check_rates(mod, drop_path_rate: float, *dropouts) -> None:
    if mod.training and drop_path_rate > 0:
        raise NotImplementedError("drop_path > 0 in training mode is not supported by the fused block")
    if mod.training and any(d.p > 0 for d in dropouts):
        raise NotImplementedError("drop > 0 in training mode is not supported by the fused block")


class Mlp(nn.Module):
    """blocks.py:58-79 with ``fc1``'s bias and the GELU in one kernel; same parameters, same state dict."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, bias=True, drop=0.):
        super().__init__()
        out_features = out_features or in_features
        hidden_features = hidden_features or in_features
        bias, drop_probs = _pair(bias), _pair(drop)
        act = act_layer() if callable(act_layer) else act_layer
        if type(act) is not nn.GELU or act.approximate != "none":
            raise TypeError(f"Mlp: act_layer must be nn.GELU (the exact erf form), got {act!r}")
        self.fc1 = nn.Linear(in_features, hidden_features, bias=bias[0])
        self.act = act
        self.drop1 = nn.Dropout(drop_probs[0])
        self.fc2 = nn.Linear(hidden_features, out_features, bias=bias[1])
        self.drop2 = nn.Dropout(drop_probs[1])

    def forward(self, x):
        _check_rates(self, 0., self.drop1, self.drop2)
        _check_float32("Mlp", x)
        if not x.is_cuda:
            raise RuntimeError("Mlp: x is on the CPU; this build only runs on a HIP device (no CPU fallback)")
        return self.fc2(bias_gelu(F.linear(x, self.fc1.weight), self.fc1.bias))


class Block(nn.Module):
    """blocks.py:115-131 on ``Attention``, ``Mlp`` and the fused add + norm; same parameters, same state dict."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, rope=None):
        super().__init__()
        self.norm1 = _layer_norm_of(norm_layer(dim), dim, "Block")
        self.attn = Attention(dim, rope=rope, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = _layer_norm_of(norm_layer(dim), dim, "Block")
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)

    def forward(self, x, xpos):
        _check_rates(self, getattr(self.drop_path, "drop_prob", 0.), self.attn.proj_drop, self.mlp.drop1, self.mlp.drop2)
        a = self.attn(layer_norm(x, *_norm(self.norm1)), xpos)
        x, t = add_layer_norm(x, a, *_norm(self.norm2))
        return x + self.mlp(t)


class DecoderBlock(nn.Module):
    """blocks.py:181-203 on ``Attention``, ``CrossAttention``, ``Mlp`` and the fused add + norm; same parameters, same
    state dict.  ``mask`` goes to ``CrossAttention``, which refuses one."""

    def __init__(self, dim, num_heads, mlp_ratio=4., qkv_bias=False, drop=0., attn_drop=0., drop_path=0.,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, norm_mem=True, rope=None):
        super().__init__()
        self.norm1 = _layer_norm_of(norm_layer(dim), dim, "DecoderBlock")
        self.attn = Attention(dim, rope=rope, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop, proj_drop=drop)
        self.cross_attn = CrossAttention(dim, rope=rope, num_heads=num_heads, qkv_bias=qkv_bias, attn_drop=attn_drop,
                                         proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = _layer_norm_of(norm_layer(dim), dim, "DecoderBlock")
        self.norm3 = _layer_norm_of(norm_layer(dim), dim, "DecoderBlock")
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.norm_y = _layer_norm_of(norm_layer(dim), dim, "DecoderBlock") if norm_mem else nn.Identity()

    def forward(self, x, y, xpos, ypos, mask=None):
        _check_rates(self, getattr(self.drop_path, "drop_prob", 0.), self.attn.proj_drop, self.cross_attn.proj_drop,
                     self.mlp.drop1, self.mlp.drop2)
        a = self.attn(layer_norm(x, *_norm(self.norm1)), xpos)
        y_ = y if isinstance(self.norm_y, nn.Identity) else layer_norm(y, *_norm(self.norm_y))
        x, t = add_layer_norm(x, a, *_norm(self.norm2))
        x, t = add_layer_norm(x, self.cross_attn(t, y_, y_, xpos, ypos, mask), *_norm(self.norm3))
        return x + self.mlp(t), y


class VGGTBlock(nn.Module):
    """``Block`` of vggt/layers/block.py:27-107 on ``VGGTAttention``, ``Mlp`` and the fused add + norm; same constructor
    arguments, same state dict (``norm1.*``, ``attn.*``, ``ls1.gamma``, ``norm2.*``, ``mlp.*``, ``ls2.gamma``).  ``ls1``
    rides in the add + ``norm2`` call; ``ls2`` is applied at the last add, a tensor operation.  ``forward_nested`` and
    the list form are not served."""

    def __init__(self, dim: int, num_heads: int, mlp_ratio=4.0, qkv_bias: bool = True, proj_bias: bool = True,
                 ffn_bias: bool = True, drop: float = 0.0, attn_drop: float = 0.0, init_values=None, drop_path: float = 0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm, attn_class=VGGTAttention, ffn_layer=Mlp, qk_norm: bool = False,
                 fused_attn: bool = True, rope=None) -> None:
        super().__init__()
        if attn_class is not VGGTAttention or ffn_layer is not Mlp:
            raise TypeError("VGGTBlock: attn_class must be this package's VGGTAttention and ffn_layer its Mlp")
        self.norm1 = _layer_norm_of(norm_layer(dim), dim, "VGGTBlock")
        self.attn = attn_class(dim, num_heads=num_heads, qkv_bias=qkv_bias, proj_bias=proj_bias, attn_drop=attn_drop,
                               proj_drop=drop, qk_norm=qk_norm, fused_attn=fused_attn, rope=rope)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = _layer_norm_of(norm_layer(dim), dim, "VGGTBlock")
        self.mlp = ffn_layer(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop,
                             bias=ffn_bias)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.sample_drop_ratio = drop_path

    def forward(self, x, pos=None, mask=None):
        _check_rates(self, self.sample_drop_ratio, self.attn.proj_drop, self.mlp.drop1, self.mlp.drop2)
        a = self.attn(layer_norm(x, *_norm(self.norm1)), pos=pos, mask=mask)
        gamma = None if isinstance(self.ls1, nn.Identity) else self.ls1.gamma
        x, t = add_layer_norm(x, a, *_norm(self.norm2), gamma=gamma)
        m = self.mlp(t)
        return x + m if isinstance(self.ls2, nn.Identity) else torch.addcmul(x, m, self.ls2.gamma)
