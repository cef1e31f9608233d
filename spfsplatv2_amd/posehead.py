"""The pose heads on the HIP library: from the backbone's tokens to the pose encoding that ``process_pose`` takes.

============================  ==========================================================================================
here                          reference
============================  ==========================================================================================
``PoseHeadCfg``, ``PoseHead`` model/encoder/heads/pose_head.py (``create_pose_head`` likewise)
``camera_head_factory``       model/encoder/heads/__init__.py:27-31
``predict_poses``             the pose loop of encoder_spfsplatv2.py:228-245: ``pose_head`` on view 0, ``pose_head2`` on
                              every other view, ``torch.stack``, ``process_pose``
``pool_tokens``               ``torch.cat([enc, dec], -1)``, ``rearrange``, ``AdaptiveAvgPool2d((1, 1))``, ``view``
``encode_poses``              softplus / clamp / divide of the homogeneous translation and ``torch.cat([out_r, out_t])``
``embed_silu``                ``embed_pose`` and the ``nn.SiLU`` in front of ``poseLN_modulation``'s Linear
``modulate``                  ``gate * modulate(adaln_norm(x), shift, scale) + x`` of vggt/heads/camera_head.py:143-147,
                              the three ``chunk`` thirds read in place
``CameraTrunkAttention``      ``Attention`` of vggt/layers/attention.py as the camera trunk builds it: no rope, no mask,
                              no q / k norm; head dim 64 or 128, at most 32 tokens (the views)
``CameraTrunkBlock``          ``Block`` of vggt/layers/block.py:27-107 on ``CameraTrunkAttention``
``activate_pose``             vggt/heads/head_act.py:12-58
``CameraHead``                vggt/heads/camera_head.py (``forward``, ``trunk_fn``)
============================  ==========================================================================================

Kernels: csrc/posehead.hip.  float32 only; no CPU path; no dropout and no stochastic depth in training mode -- each of
these raises before anything is launched.  The GEMMs stay ``nn.Linear``; the ReLUs between ``PoseHead``'s Linears are
``add_relu``.  Nothing here synchronises the host, reads a value back or loops over the views; no atomics, so two runs
agree bitwise.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._checks import check_device as _check_device, check_float32 as _check_float32
from .block import (MAX_C, DropPath, LayerScale, Mlp, _check_rates, _layer_norm_of, _norm, _check_width, add_layer_norm,
                    bias_gelu, layer_norm)
from .heads import add_relu
from .pose import process_pose

MAX_VIEWS = _lib.POSEHEAD_MAX_S
MAX_ROWS = _lib.POSEHEAD_MAX_ROWS
ACTS = tuple(_lib.POSE_ACTS)
MAX_ENCODE_ROWS = 1 << 24              # spf_posehead_encode_*'s limit (the header's)


# ---- rows read in place ----------------------------------------------------------------------------------------------
def _lead_map(t: torch.Tensor, lead: int, unit: int):
    """(inner, stride, outer_stride) of the rows that the first ``lead`` dimensions of ``t`` count, or None where two
    strides that are multiples of ``unit`` floats do not address them."""
    g = []
    for n, s in zip(t.shape[:lead], t.stride()[:lead]):
        if n == 1:
            continue
        if g and g[-1][1] == n * s:
            g[-1] = (g[-1][0] * n, s)
        else:
            g.append((n, s))
    if len(g) > 2 or any(s < 0 or s % unit for _, s in g):
        return None
    if not g:
        return 1, 0, 0
    if len(g) == 1:
        return g[0][0], g[0][1], 0
    return g[1][0], g[1][1], g[0][1]


def _pool_source(t: torch.Tensor) -> torch.Tensor:
    """``t`` [.., L, C] itself where the pool kernel can read it in place (unit channel stride, 16-byte aligned, the rows
    addressed by at most two strides, everything a multiple of 4 floats), else a contiguous copy."""
    ok = (t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and (t.shape[-2] == 1 or (t.stride(-2) >= 0 and t.stride(-2) % 4 == 0))
          and _lead_map(t, t.dim() - 2, 4) is not None)
    return t if ok else t.contiguous()


# ---- a. pool ---------------------------------------------------------------------------------------------------------
def _check_pool(enc, dec) -> None:
    what = "pool_tokens"
    _check_float32(what, dec, enc)
    for t in (dec, enc):
        if t is None:
            continue
        if t.dim() < 3 or t.numel() == 0:
            raise RuntimeError(f"{what}: tokens must be [.., L, C] with at least one row, got shape {list(t.shape)}")
        if t.shape[-1] % 4 != 0:
            raise ValueError(f"{what}: the channel count must be a multiple of 4, got {t.shape[-1]}")
    if enc is not None and enc.shape[:-1] != dec.shape[:-1]:
        raise RuntimeError(f"{what}: the two sources differ in rows or tokens: {list(enc.shape)} and {list(dec.shape)}")
    rows = dec.numel() // (dec.shape[-1] * dec.shape[-2])
    if rows > MAX_ROWS:
        raise RuntimeError(f"{what}: at most {MAX_ROWS} rows, got {rows}")
    _check_device(what, dec, enc)


def _pool_args(srcs, rows: int, L: int) -> _lib.SpfPosePool:
    a = _lib.SpfPosePool()
    for i, t in enumerate(srcs):
        a.src[i] = t.data_ptr()
        a.inner[i], a.stride[i], a.outer_stride[i] = _lead_map(t, t.dim() - 2, 4)
        a.tok_stride[i] = t.stride(-2) if L > 1 else t.shape[-1]
        a.C[i] = t.shape[-1]
    a.rows, a.L = rows, L
    return a


class _PoolTokens(torch.autograd.Function):
    """first [.., L, C0] (and second [.., L, C1] or None) -> [.., C0 + C1]"""

    @staticmethod
    def forward(ctx, first, second):
        srcs = [_pool_source(t) for t in (first, second) if t is not None]
        lead, L = first.shape[:-2], first.shape[-2]
        rows = first.numel() // (L * first.shape[-1])
        feat = torch.empty(*lead, sum(t.shape[-1] for t in srcs), dtype=torch.float32, device=first.device)
        _lib.launch("spf_posehead_pool_forward", first.device, _pool_args(srcs, rows, L), feat)
        ctx.shapes = [t.shape for t in srcs]
        return feat

    @staticmethod
    @once_differentiable
    def backward(ctx, d_feat):
        d_feat = d_feat.contiguous()
        grads = [torch.empty(s, dtype=torch.float32, device=d_feat.device) for s in ctx.shapes]
        a = _lib.SpfPosePool()
        L = ctx.shapes[0][-2]
        a.rows, a.L = d_feat.numel() // d_feat.shape[-1], L
        for i, s in enumerate(ctx.shapes):
            a.C[i] = s[-1]
        _lib.launch("spf_posehead_pool_backward", d_feat.device, a, d_feat, grads[0], grads[1] if len(grads) > 1 else None)
        return grads[0], grads[1] if len(grads) > 1 else None


def pool_tokens(dec, enc=None):
    """The mean over the L tokens of ``dec`` [.., L, C] -- with ``enc`` [.., L, C'] of ``torch.cat([enc, dec], -1)``:
    [.., C' + C], the encoder's channels first.  ``L = 1`` copies.  A ``tok[:, i]`` view of a [b, v, L, C] tensor and a
    ``tok[:, 1:]`` block of views are read in place."""
    _check_pool(enc, dec)
    return _PoolTokens.apply(dec, None) if enc is None else _PoolTokens.apply(enc, dec)


# ---- b. the head's tail ----------------------------------------------------------------------------------------------
def _encode_args(rows: int, n: int, v: int, homog) -> _lib.SpfPoseEncode:
    a = _lib.SpfPoseEncode()
    a.rows, a.out_inner, a.out_stride, a.out_outer_stride = rows, n, 9, 9 * v
    a.homogeneous = int(homog is not None)
    if homog is not None:
        a.beta, a.max_inv_scale, a.min_inv_scale = homog
    return a


def _check_encode(rot, t, homog, b: int, n: int) -> None:
    what = "encode_poses"
    _check_float32(what, rot, t)
    width = 4 if homog is not None else 3
    if tuple(rot.shape) != (b, n, 6) or tuple(t.shape) != (b, n, width):
        raise RuntimeError(f"{what}: rot must be [{b}, {n}, 6] and t [{b}, {n}, {width}], got {list(rot.shape)} and "
                           f"{list(t.shape)}")
    if b * n > MAX_ENCODE_ROWS:
        raise RuntimeError(f"{what}: at most {MAX_ENCODE_ROWS} pose rows per call, got {b * n}")
    _check_device(what, rot, t)


def encode_into(out, start: int, rot, t, homog) -> None:
    """The forward launch: the pose rows of ``rot`` [b, n, 6] and ``t`` [b, n, 3 or 4] into ``out[:, start:start + n]``
    of the [b, v, 9] tensor ``out``; its other rows are left alone.  No autograd."""
    b, v, _ = out.shape
    n = rot.shape[1]
    _check_encode(rot, t, homog, b, n)
    if not (out.is_contiguous() and out.dtype == torch.float32 and out.shape[-1] == 9 and 0 <= start and start + n <= v):
        raise RuntimeError(f"encode_poses: views {start}..{start + n} do not fit a contiguous float32 [b, v, 9] tensor "
                           f"of shape {list(out.shape)}")
    _check_device("encode_poses", out, rot, t)
    _lib.launch("spf_posehead_encode_forward", out.device, _encode_args(b * n, n, v, homog), rot.contiguous(),
                t.contiguous(), out[:, start:])


class _EncodePoses(torch.autograd.Function):
    """parts: ((first view, homog or None), ..); tensors: rot, t of each part.  -> [b, v, 9]"""

    @staticmethod
    def forward(ctx, parts, v, *tensors):
        b = tensors[0].shape[0]
        out = torch.empty(b, v, 9, dtype=torch.float32, device=tensors[0].device)
        saved = []
        for i, (start, homog) in enumerate(parts):
            rot, t = tensors[2 * i], tensors[2 * i + 1].contiguous()
            encode_into(out, start, rot, t, homog)
            saved.append(t if homog is not None else None)
        ctx.save_for_backward(*saved)
        ctx.parts, ctx.v = parts, v
        ctx.counts = [tensors[2 * i].shape[1] for i in range(len(parts))]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        d_out = d_out.contiguous()
        b, grads = d_out.shape[0], []
        for (start, homog), n, t in zip(ctx.parts, ctx.counts, ctx.saved_tensors):
            d_rot = torch.empty(b, n, 6, dtype=torch.float32, device=d_out.device)
            d_t = torch.empty(b, n, 4 if homog is not None else 3, dtype=torch.float32, device=d_out.device)
            _lib.launch("spf_posehead_encode_backward", d_out.device, _encode_args(b * n, n, ctx.v, homog), t,
                        d_out[:, start:], d_rot, d_t)
            grads += [d_rot, d_t]
        return (None, None, *grads)


def encode_poses(parts, v: int):
    """``parts``: ``(first view, rot [b, n, 6], t [b, n, 3 or 4], homog)`` per head, ``homog`` None or the floats
    ``(beta, max_inv_scale, min_inv_scale)``; together the parts cover the views ``0..v`` once.  Returns the pose
    encoding [b, v, 9], every part written where it belongs: no ``cat``, no ``stack``."""
    cover = sorted((start, start + rot.shape[1]) for start, rot, _, _ in parts)
    if not cover or cover[0][0] != 0 or cover[-1][1] != v or any(a[1] != b[0] for a, b in zip(cover, cover[1:])):
        raise ValueError(f"encode_poses: the parts cover the views {cover}, not 0..{v} once")
    b = parts[0][1].shape[0]
    for _, rot, t, homog in parts:
        _check_encode(rot, t, homog, b, rot.shape[1])
    meta = tuple((start, homog) for start, _, _, homog in parts)
    return _EncodePoses.apply(meta, v, *[x for _, rot, t, _ in parts for x in (rot, t)])


# ---- c. embed + SiLU -------------------------------------------------------------------------------------------------
def _check_embed(p, weight, bias, rows) -> int:
    what = "embed_silu"
    _check_float32(what, p, weight, bias)
    if weight.dim() != 2 or weight.shape[1] != 9 or tuple(bias.shape) != (weight.shape[0],):
        raise RuntimeError(f"{what}: weight must be [C, 9] and bias [C], got {list(weight.shape)} and {list(bias.shape)}")
    if p.dim() < 1 or p.shape[-1] != 9 or p.numel() == 0:
        raise RuntimeError(f"{what}: p must be [.., 9], got shape {list(p.shape)}")
    if rows is None:
        rows = p.numel() // 9
    elif p.numel() != 9:
        raise RuntimeError(f"{what}: with rows given p is the ONE broadcast row, got shape {list(p.shape)}")
    if not 1 <= rows <= MAX_ROWS:
        raise RuntimeError(f"{what}: rows must be 1 .. {MAX_ROWS}, got {rows}")
    _check_device(what, p, weight, bias)
    return rows


class _EmbedSilu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p, weight, bias, rows, bcast):
        p_, w_, b_ = p.contiguous(), weight.contiguous(), bias.contiguous()
        c = w_.shape[0]
        out = torch.empty(rows, c, dtype=torch.float32, device=p.device)
        _lib.launch("spf_posehead_embed_silu_forward", p.device, p_, int(bcast), w_, b_, rows, c, out)
        ctx.save_for_backward(p_, w_, b_)
        ctx.rows, ctx.bcast, ctx.p_shape = rows, bcast, p.shape
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        p, w, b = ctx.saved_tensors
        dout = dout.contiguous()
        dw, db = torch.empty_like(w), torch.empty_like(b)
        dp = torch.empty(ctx.p_shape, dtype=torch.float32, device=p.device) if ctx.needs_input_grad[0] else None
        _lib.launch("spf_posehead_embed_silu_backward", p.device, p, int(ctx.bcast), w, b, dout, ctx.rows, w.shape[0], dw,
                    db, dp)
        return dp, dw, db, None, None


def embed_silu(p, weight, bias, rows=None):
    """``F.silu(F.linear(p, weight, bias))`` for ``p`` [.., 9] and ``weight`` [C, 9]: [.., C].  With ``rows`` given, ``p``
    holds ONE row of nine floats (``empty_pose_tokens``) that stands for ``rows`` equal rows: [rows, C], and the gradient
    of ``p`` is summed over them."""
    n = _check_embed(p, weight, bias, rows)
    out = _EmbedSilu.apply(p, weight, bias, n, rows is not None)
    return out if rows is not None else out.view(*p.shape[:-1], weight.shape[0])


# ---- d. adaptive LayerNorm -------------------------------------------------------------------------------------------
def _check_modulate(x, mod) -> None:
    what = "modulate"
    _check_float32(what, x, mod)
    if x.dim() < 1 or x.numel() == 0:
        raise RuntimeError(f"{what}: x must have at least one row, got shape {list(x.shape)}")
    c = x.shape[-1]
    _check_width(what, c)
    if tuple(mod.shape) != (*x.shape[:-1], 3 * c):
        raise RuntimeError(f"{what}: mod must be {[*x.shape[:-1], 3 * c]} (shift | scale | gate), got {list(mod.shape)}")
    _check_device(what, x, mod)


class _Modulate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod, eps):
        x, mod = x.contiguous(), mod.contiguous()
        c = x.shape[-1]
        out = torch.empty_like(x)
        _lib.launch("spf_posehead_modulate_forward", x.device, x, mod, x.numel() // c, c, eps, out)
        ctx.save_for_backward(x, mod)
        ctx.eps = eps
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, mod = ctx.saved_tensors
        c = x.shape[-1]
        dx, dmod = torch.empty_like(x), torch.empty_like(mod)
        _lib.launch("spf_posehead_modulate_backward", x.device, x, mod, dout.contiguous(), x.numel() // c, c, ctx.eps, dx,
                    dmod)
        return dx, dmod, None


def modulate(x, mod, eps: float = 1e-6):
    """``gate * (LN(x) * (1 + scale) + shift) + x`` with ``shift, scale, gate = mod.chunk(3, -1)`` and ``LN`` a LayerNorm
    without parameters: ``x`` [.., C], ``mod`` [.., 3 C] -- the Linear's output as it is, no chunk copies; the backward
    hands the Linear ONE [.., 3 C] gradient in the same layout."""
    _check_modulate(x, mod)
    return _Modulate.apply(x, mod, float(eps))


# ---- e. attention over the views -------------------------------------------------------------------------------------
def _check_trunk_attention(qkv, num_heads: int) -> int:
    what = "trunk_attention"
    _check_float32(what, qkv)
    if qkv.dim() != 3 or qkv.numel() == 0 or num_heads < 1 or qkv.shape[-1] % (3 * num_heads) != 0:
        raise RuntimeError(f"{what}: qkv must be [B, S, 3 * {num_heads} * D], got shape {list(qkv.shape)}")
    d = qkv.shape[-1] // (3 * num_heads)
    if d not in (64, 128):
        raise ValueError(f"{what}: head dim must be 64 or 128, got {d}")
    if not 1 <= qkv.shape[1] <= MAX_VIEWS:
        raise ValueError(f"{what}: the sequence (the views) must hold 1 .. {MAX_VIEWS} tokens, got {qkv.shape[1]}")
    _check_device(what, qkv)
    return d


class _TrunkAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, num_heads, d):
        qkv = qkv.contiguous()
        B, S, _ = qkv.shape
        out = torch.empty(B, S, num_heads * d, dtype=torch.float32, device=qkv.device)
        _lib.launch("spf_posehead_attn_forward", qkv.device, qkv, B, S, num_heads, d, out)
        ctx.save_for_backward(qkv)
        ctx.dims = (B, S, num_heads, d)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        (qkv,) = ctx.saved_tensors
        dqkv = torch.empty_like(qkv)
        _lib.launch("spf_posehead_attn_backward", qkv.device, qkv, dout.contiguous(), *ctx.dims, dqkv)
        return dqkv, None, None


def trunk_attention(qkv, num_heads: int):
    """``softmax(q k^T / sqrt(D)) v`` of the packed ``qkv`` [B, S, 3 * H * D] (the qkv Linear's output: q, k, v, each
    head-major): [B, S, H * D].  D is 64 or 128, S at most 32."""
    d = _check_trunk_attention(qkv, num_heads)
    return _TrunkAttention.apply(qkv, int(num_heads), d)


# ---- f. accumulate + activate ----------------------------------------------------------------------------------------
def _acts(trans_act, quat_act, fl_act):
    for a in (trans_act, quat_act, fl_act):
        if a not in _lib.POSE_ACTS:
            raise ValueError(f"Unknown act_type: {a} (one of {list(ACTS)})")
    return _lib.POSE_ACTS[trans_act], _lib.POSE_ACTS[quat_act], _lib.POSE_ACTS[fl_act]


def _check_activate(prev, delta) -> None:
    what = "activate_pose"
    _check_float32(what, delta, prev)
    if delta.dim() < 1 or delta.shape[-1] != 9 or delta.numel() == 0:
        raise RuntimeError(f"{what}: the pose encoding must be [.., 9], got shape {list(delta.shape)}")
    if prev is not None and prev.shape != delta.shape:
        raise RuntimeError(f"{what}: prev {list(prev.shape)} and delta {list(delta.shape)} differ in shape")
    _check_device(what, delta, prev)


class _Activate(torch.autograd.Function):
    """(prev or None, delta) -> (pred = prev + delta, out = activate_pose(pred)); prev is a constant."""

    @staticmethod
    def forward(ctx, prev, delta, acts):
        delta = delta.contiguous()
        prev = prev.contiguous() if prev is not None else None
        pred, out = torch.empty_like(delta), torch.empty_like(delta)
        _lib.launch("spf_posehead_activate_forward", delta.device, prev, delta, delta.numel() // 9, *acts, pred, out)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(pred)
        ctx.acts = acts
        return pred, out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_pred, d_out):
        if d_pred is None and d_out is None:
            return None, None, None
        (pred,) = ctx.saved_tensors
        d_delta = torch.empty_like(pred)
        _lib.launch("spf_posehead_activate_backward", pred.device, pred, d_pred.contiguous() if d_pred is not None else None,
                    d_out.contiguous() if d_out is not None else None, pred.numel() // 9, *ctx.acts, d_delta)
        return None, d_delta, None


def accumulate_activate(prev, delta, trans_act="linear", quat_act="linear", fl_act="linear"):
    """``pred = prev.detach() + delta`` (``prev`` None: ``delta``) and ``activate_pose(pred)``, both returned; the gradient
    goes to ``delta`` only, as the reference's ``pred_pose_enc.detach()`` has it."""
    acts = _acts(trans_act, quat_act, fl_act)
    _check_activate(prev, delta)
    return _Activate.apply(prev.detach() if prev is not None else None, delta, acts)


def activate_pose(pred_pose_enc, trans_act="linear", quat_act="linear", fl_act="linear"):
    """head_act.py:12-35: columns 0:3, 3:7 and 7:9 of ``pred_pose_enc`` [.., 9] through ``linear``, ``inv_log``
    (``sign(y) * expm1(|y|)``), ``exp`` or ``relu``."""
    return accumulate_activate(None, pred_pose_enc, trans_act, quat_act, fl_act)[1]


# ---- the MLP pose head -----------------------------------------------------------------------------------------------
@dataclass
class PoseHeadCfg:
    pose_init_t: bool
    use_homogeneous: bool
    concat_enc: bool


class PoseHead(nn.Module):
    """pose_head.py:22-110: same constructor, same parameters and buffers, same state dict, same ``init_pose``.
    ``forward`` also takes tokens of several views at once, [b, n, L, C], and returns [b, n, 9]."""
    cfg: PoseHeadCfg

    def __init__(self, net, cfg: PoseHeadCfg):
        super().__init__()
        self.cfg = cfg
        self.d_model = net.enc_embed_dim + net.dec_embed_dim if cfg.concat_enc else net.dec_embed_dim
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))             # (kept for the attribute; pool_tokens does its work)
        self.more_mlps = nn.Sequential(nn.Linear(self.d_model, self.d_model // 2), nn.ReLU(),
                                       nn.Linear(self.d_model // 2, self.d_model // 4), nn.ReLU())
        self.use_homogeneous = cfg.use_homogeneous
        self.concat_enc = cfg.concat_enc
        self._homog = None
        if cfg.use_homogeneous:
            self.fc_t = nn.Linear(self.d_model // 4, 4)
            self.register_buffer("max_scale", torch.tensor([4.0]))
            self.register_buffer("min_scale", torch.tensor([0.01]))
            self.register_buffer("max_inv_scale", 1. / self.max_scale)
            self.register_buffer("h_beta", math.log(2) / (1. - self.max_inv_scale))
            self.register_buffer("min_inv_scale", 1. / self.min_scale)
            # read once, here: a call never reads a buffer back
            self._homog = (float(self.h_beta), float(self.max_inv_scale), float(self.min_inv_scale))
        else:
            self.fc_t = nn.Linear(self.d_model // 4, 3)
        self.fc_rot = nn.Linear(self.d_model // 4, 6)
        self.init_pose()

    def init_pose(self):
        """Zero rotation weights with the identity's two rows as the bias; with ``pose_init_t`` a zero translation."""
        nn.init.constant_(self.fc_rot.weight, 0.0)
        nn.init.constant_(self.fc_rot.bias, 0.0)
        self.fc_rot.bias.data[:6] = torch.tensor([1, 0, 0, 0, 1, 0], dtype=torch.float32)
        if self.cfg.pose_init_t:
            nn.init.constant_(self.fc_t.weight, 0.0)
            nn.init.constant_(self.fc_t.bias, 0.0)

    def regress(self, encoder_tokens):
        """(rot [b, n, 6], t [b, n, 3 or 4]) of tokens [b, n, L, C]: the pool and the four GEMMs."""
        dec = encoder_tokens[-1]
        enc = encoder_tokens[0] if self.cfg.concat_enc else None
        _check_float32("PoseHead", dec, enc)
        if dec.dim() != 4:
            raise RuntimeError(f"PoseHead: tokens must be [b, L, C] or [b, n, L, C], got shape {list(dec.shape)}")
        L = dec.shape[-2]
        if math.isqrt(L) ** 2 != L:
            raise ValueError(f"PoseHead: the token count must be a perfect square (a p x p grid), got {L}")
        feat = pool_tokens(dec, enc)
        if feat.shape[-1] != self.d_model:
            raise RuntimeError(f"PoseHead: the tokens have {feat.shape[-1]} channels, the head was built for {self.d_model}")
        feat = add_relu(self.more_mlps[0](feat))[1]
        feat = add_relu(self.more_mlps[2](feat))[1]
        return self.fc_rot(feat), self.fc_t(feat)

    def forward(self, encoder_tokens, image_size=None, conf=None):
        single = encoder_tokens[-1].dim() == 3
        if single:
            encoder_tokens = [t.unsqueeze(1) for t in encoder_tokens]
        rot, t = self.regress(encoder_tokens)
        out = encode_poses([(0, rot, t, self._homog)], rot.shape[1])
        return out[:, 0] if single else out


def create_pose_head(net, cfg):
    return PoseHead(net, cfg)


def camera_head_factory(head_type, output_mode, net, cfg):
    if head_type == 'mlp' and output_mode == 'pose':
        return create_pose_head(net, cfg)
    raise NotImplementedError(f"unexpected {head_type=} and {output_mode=}")


def predict_poses(head1: PoseHead, head2: PoseHead, pose_feat, context_views: int, *, pose_make_baseline_1: bool,
                  pose_make_relative: bool):
    """encoder_spfsplatv2.py:228-245: ``pose_feat`` is the list of token tensors [b, v, L, C]; view 0 goes through
    ``head1``, the views 1.. through ``head2`` in ONE call, both write their rows of one [b, v, 9] tensor, and
    ``process_pose`` turns it into the [b, v, 4, 4] extrinsics."""
    v = pose_feat[-1].shape[1]
    rot, t = head1.regress([tok[:, :1] for tok in pose_feat])
    parts = [(0, rot, t, head1._homog)]
    if v > 1:
        rot, t = head2.regress([tok[:, 1:] for tok in pose_feat])
        parts.append((1, rot, t, head2._homog))
    return process_pose(encode_poses(parts, v), context_views, encoding="rot6d", pose_make_baseline_1=pose_make_baseline_1,
                        pose_make_relative=pose_make_relative)


# ---- the camera trunk ------------------------------------------------------------------------------------------------
class CameraTrunkAttention(nn.Module):
    """vggt/layers/attention.py:21-84 as the camera trunk uses it: ``qkv``, attention over the views, ``proj``.  Head dim
    64 or 128, at most 32 tokens; no rope, no mask, no q / k norm.  Same parameters (``qkv.*``, ``proj.*``)."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = True, proj_bias: bool = True, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, qk_norm: bool = False, fused_attn: bool = True, rope=None) -> None:
        super().__init__()
        if dim % num_heads != 0:
            raise ValueError("dim should be divisible by num_heads")
        if qk_norm or rope is not None:
            raise NotImplementedError("CameraTrunkAttention: qk_norm and rope are VGGTAttention's")
        if dim // num_heads not in (64, 128):
            raise ValueError(f"CameraTrunkAttention: head dim must be 64 or 128, got {dim // num_heads}")
        if attn_drop > 0.0:
            raise NotImplementedError("CameraTrunkAttention: attn_drop > 0 is not supported")
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.fused_attn = fused_attn
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = nn.Identity()
        self.k_norm = nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)
        self.proj_drop = nn.Dropout(proj_drop)
        self.rope = None

    def forward(self, x, pos=None, mask=None):
        if pos is not None or mask is not None:
            raise NotImplementedError("CameraTrunkAttention: pos and mask are not served")
        _check_rates(self, 0., self.proj_drop)
        _check_float32("CameraTrunkAttention", x)
        if x.dim() != 3:
            raise RuntimeError(f"CameraTrunkAttention: x must be [B, S, C], got shape {list(x.shape)}")
        if not 1 <= x.shape[1] <= MAX_VIEWS:
            raise ValueError(f"CameraTrunkAttention: the sequence (the views) must hold 1 .. {MAX_VIEWS} tokens, got "
                             f"{x.shape[1]}")
        _check_device("CameraTrunkAttention", x)
        return self.proj(trunk_attention(self.qkv(x), self.num_heads))


def _mlp(mlp: Mlp, x):
    """``mlp(x)``.  A hidden width beyond the bias + GELU kernel's row limit (the production trunk: 4 x 2048) keeps
    ``fc1``'s bias in its GEMM and runs the GELU, which is elementwise, on the same memory seen as rows of a width the
    kernel takes: the widest multiple of 4 within the limit that divides the hidden width.  No copy, same parameters."""
    hidden = mlp.fc1.out_features
    if hidden <= MAX_C:
        return mlp(x)
    _check_rates(mlp, 0., mlp.drop1, mlp.drop2)
    if hidden % 4 != 0:
        raise ValueError(f"Mlp: the hidden width must be a multiple of 4, got {hidden}")
    width = next(w for w in range(MAX_C, 0, -4) if hidden % w == 0)
    u = mlp.fc1(x)
    return mlp.fc2(bias_gelu(u.view(-1, width), None).view(u.shape))


class CameraTrunkBlock(nn.Module):
    """``Block`` of vggt/layers/block.py:27-107 on ``CameraTrunkAttention``, ``Mlp`` and the fused add + norm: same state
    dict (``norm1.*``, ``attn.qkv.*``, ``attn.proj.*``, ``ls1.gamma``, ``norm2.*``, ``mlp.fc1.*``, ``mlp.fc2.*``,
    ``ls2.gamma``)."""

    def __init__(self, dim: int, num_heads: int, mlp_ratio=4.0, qkv_bias: bool = True, proj_bias: bool = True,
                 ffn_bias: bool = True, drop: float = 0.0, attn_drop: float = 0.0, init_values=None, drop_path: float = 0.0,
                 act_layer=nn.GELU, norm_layer=nn.LayerNorm) -> None:
        super().__init__()
        self.norm1 = _layer_norm_of(norm_layer(dim), dim, "CameraTrunkBlock")
        self.attn = CameraTrunkAttention(dim, num_heads=num_heads, qkv_bias=qkv_bias, proj_bias=proj_bias,
                                         attn_drop=attn_drop, proj_drop=drop)
        self.ls1 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path1 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.norm2 = _layer_norm_of(norm_layer(dim), dim, "CameraTrunkBlock")
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop, bias=ffn_bias)
        self.ls2 = LayerScale(dim, init_values=init_values) if init_values else nn.Identity()
        self.drop_path2 = DropPath(drop_path) if drop_path > 0.0 else nn.Identity()
        self.sample_drop_ratio = drop_path

    def forward(self, x, pos=None, mask=None):
        _check_rates(self, self.sample_drop_ratio, self.attn.proj_drop, self.mlp.drop1, self.mlp.drop2)
        a = self.attn(layer_norm(x, *_norm(self.norm1)), pos=pos, mask=mask)
        gamma = None if isinstance(self.ls1, nn.Identity) else self.ls1.gamma
        x, t = add_layer_norm(x, a, *_norm(self.norm2), gamma=gamma)
        m = _mlp(self.mlp, t)
        return x + m if isinstance(self.ls2, nn.Identity) else torch.addcmul(x, m, self.ls2.gamma)


class CameraHead(nn.Module):
    """vggt/heads/camera_head.py:20-170: same constructor, same parameters, same state dict.  The camera token
    ``tokens[:, :, 0]`` is normalised where it lies; every iteration is embed + SiLU, the modulation Linear, ``modulate``,
    the trunk, ``trunk_norm``, ``pose_branch`` and one accumulate + activate launch."""

    def __init__(self, dim_in: int = 2048, trunk_depth: int = 4, pose_encoding_type: str = "absT_quaR_FoV",
                 num_heads: int = 16, mlp_ratio: int = 4, init_values: float = 0.01, trans_act: str = "linear",
                 quat_act: str = "linear", fl_act: str = "relu"):
        super().__init__()
        if pose_encoding_type == "absT_quaR_FoV":
            self.target_dim = 9
        else:
            raise ValueError(f"Unsupported camera encoding type: {pose_encoding_type}")
        _acts(trans_act, quat_act, fl_act)
        self.trans_act, self.quat_act, self.fl_act = trans_act, quat_act, fl_act
        self.trunk_depth = trunk_depth
        self.trunk = nn.Sequential(*[CameraTrunkBlock(dim=dim_in, num_heads=num_heads, mlp_ratio=mlp_ratio,
                                                      init_values=init_values) for _ in range(trunk_depth)])
        self.token_norm = nn.LayerNorm(dim_in)
        self.trunk_norm = nn.LayerNorm(dim_in)
        self.empty_pose_tokens = nn.Parameter(torch.zeros(1, 1, self.target_dim))
        self.embed_pose = nn.Linear(self.target_dim, dim_in)
        self.poseLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim_in, 3 * dim_in, bias=True))
        self.adaln_norm = nn.LayerNorm(dim_in, elementwise_affine=False, eps=1e-6)
        self.pose_branch = Mlp(in_features=dim_in, hidden_features=dim_in // 2, out_features=self.target_dim, drop=0)

    def forward(self, aggregated_tokens_list: list, num_iterations: int = 4) -> list:
        tokens = aggregated_tokens_list[-1]
        _check_float32("CameraHead", tokens)
        if tokens.dim() != 4:
            raise RuntimeError(f"CameraHead: tokens must be [B, S, N, C], got shape {list(tokens.shape)}")
        pose_tokens = layer_norm(tokens[:, :, 0], *_norm(self.token_norm))
        return self.trunk_fn(pose_tokens, num_iterations)

    def trunk_fn(self, pose_tokens, num_iterations: int) -> list:
        B, S, C = pose_tokens.shape
        pred, outs = None, []
        for _ in range(num_iterations):
            if pred is None:
                emb = embed_silu(self.empty_pose_tokens, self.embed_pose.weight, self.embed_pose.bias, rows=B * S)
            else:
                emb = embed_silu(pred.detach(), self.embed_pose.weight, self.embed_pose.bias)
            mod = self.poseLN_modulation[1](emb.view(B, S, C))
            x = self.trunk(modulate(pose_tokens, mod, self.adaln_norm.eps))
            delta = _mlp(self.pose_branch, layer_norm(x, *_norm(self.trunk_norm)))
            pred, out = accumulate_activate(pred, delta, self.trans_act, self.quat_act, self.fl_act)
            outs.append(out)
        return outs
