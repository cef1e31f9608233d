"""Fused RoPE attention on the HIP library: the core of the reference's ``Attention`` and ``CrossAttention``.

=========================  ============================================================================
here                       reference (src/model/encoder/backbone/croco/blocks.py)
=========================  ============================================================================
``rope_attention``         lines 102-110 / 161-176: rope(q), rope(k), q @ k^T * scale, softmax, @ v,
                           ``.transpose(1, 2).reshape(B, N, C)``
``rope_attention_packed``  the same on the three views of one ``[B,N,3,H,D]`` projection (lines 97-98)
``Attention``              ``Attention`` (81-113)
``CrossAttention``         ``CrossAttention`` (133-179)
=========================  ============================================================================

Multi-view decoders (backbone_croco_multiview.py:178-200, backbone_masked_croco.py:216-302) hand ``CrossAttention`` keys
gathered per query view: every view's tokens copied into the key set of every other view.  ``rope_attention_views`` and
``CrossAttention.forward_views`` compute the same result from ONE key set per scene, read in place, with a host-known
table ``allow[query view][key view]``; ``decoder_view_sets`` builds the tables the two backbones' decoder blocks use.

One kernel per direction of the data flow (csrc/attention.hip): the score matrix never exists in memory, q and k are
rotated while they are staged, strided views are read in place.  Head dim 64 only; no dropout on the probabilities, no
CPU path -- each of these raises before anything is launched.

``rope_attention`` and ``rope_attention_packed`` take two keyword-only extras, which the VGGT backbone needs
(vggt_attention.py) and CroCo's two classes here do not use: ``mask`` (additive float32 or bool, broadcast to
[B,H,Nq,Nk], read in place) and ``q_norm`` / ``k_norm`` (``(weight, bias, eps)`` of a LayerNorm over the 64 elements of
every q / k row, applied before the rotation).  With all three None the launch is the one it always was.

``matrix16=True`` (keyword-only, on the two functions and on the two modules) moves a float16 / bfloat16 call to the
16-bit matrix units (csrc/attention16.hip): q and k are rotated in float32 and rounded once, the probabilities are
rounded once as operands, everything else stays float32.  It is opt-in: an unflagged 16-bit call runs the float32
compute path as before.  Plain calls only -- with ``mask``, ``q_norm`` or ``k_norm`` it raises NotImplementedError, with
float32 tokens ValueError; ``rope_attention_views`` does not take it.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from .rope import _DTYPES

HEAD_DIM = 64


def _check_tokens(q, k, v, rank: int, rank_error: str) -> None:
    """What [B,H,N,D] and [b,V,H,N,D] calls ask of q, k and v alike: each one's rank, head dim and dtype, then one dtype
    and one device."""
    for t in (q, k, v):
        if t.dim() != rank:
            raise RuntimeError(rank_error)
        if t.shape[-1] != HEAD_DIM:
            raise ValueError(f"rope_attention: head dim must be {HEAD_DIM}, got {t.shape[-1]}")
        if t.dtype not in _DTYPES:
            raise RuntimeError(f"rope_attention: unsupported dtype {t.dtype}")
    if not (q.dtype == k.dtype == v.dtype):
        raise RuntimeError(f"rope_attention: q, k and v differ in dtype ({q.dtype}, {k.dtype}, {v.dtype})")
    if not (q.device == k.device == v.device):
        raise RuntimeError("rope_attention: q, k and v are not on the same device")


def _have_positions(qpos, kpos) -> bool:
    if (qpos is None) != (kpos is None):
        raise RuntimeError("rope_attention: qpos and kpos must both be given or both be None")
    return qpos is not None


def _check_on_device(q) -> None:
    """The last check of every call."""
    if not q.is_cuda:
        raise RuntimeError("rope_attention: q, k and v are on the CPU; this build only runs on a HIP device "
                           "(no CPU fallback)")


def _check_positions(tokens: torch.Tensor, positions: torch.Tensor) -> None:
    """rope._check's position checks, same messages (tokens here are [B,H,N,D])."""
    if positions.dim() != 3:
        raise RuntimeError("positions must have 3 dimensions")
    if tokens.size(0) != positions.size(0):
        raise RuntimeError("batch size differs between tokens & positions")
    if tokens.size(2) != positions.size(1):
        raise RuntimeError("seq_length differs between tokens & positions")
    if positions.size(2) != 2:
        raise RuntimeError("positions.shape[2] must be equal to 2")
    if tokens.is_cuda != positions.is_cuda or (positions.is_cuda and positions.device != tokens.device):
        raise RuntimeError("tokens and positions are not on the same device")
    if not positions.is_contiguous():
        raise RuntimeError("positions are not contiguous")
    if positions.dtype != torch.int64:
        raise RuntimeError("positions must be int64")


def _check_mask(mask, shape) -> None:
    """What can be said about a mask without touching it; ``shape`` = (B, H, Nq, Nk)."""
    if not isinstance(mask, torch.Tensor):
        raise TypeError(f"rope_attention: mask must be a tensor or None, got {type(mask).__name__}")
    if mask.dtype not in (torch.float32, torch.bool):
        raise RuntimeError(f"rope_attention: mask must be float32 (additive) or bool, got {mask.dtype}")
    if mask.requires_grad:
        raise RuntimeError("rope_attention: the mask is not differentiable (it requires grad)")
    if not 2 <= mask.dim() <= 4:
        raise RuntimeError(f"rope_attention: mask must have 2 to 4 dimensions, got {mask.dim()}")
    full = (1,) * (4 - mask.dim()) + tuple(mask.shape)
    if any(m != 1 and m != n for m, n in zip(full, shape)):
        raise RuntimeError(f"rope_attention: mask of shape {tuple(mask.shape)} does not broadcast to [B,H,Nq,Nk] = "
                           f"{list(shape)}")


def _check_norms(q_norm, k_norm) -> None:
    if (q_norm is None) != (k_norm is None):
        raise RuntimeError("rope_attention: q_norm and k_norm must both be given or both be None")
    if q_norm is None:
        return
    for name, n in (("q_norm", q_norm), ("k_norm", k_norm)):
        if not (isinstance(n, (tuple, list)) and len(n) == 3):
            raise TypeError(f"rope_attention: {name} must be (weight, bias, eps)")
        for t in n[:2]:
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (HEAD_DIM,) or t.dtype != torch.float32:
                raise RuntimeError(f"rope_attention: {name}'s weight and bias must be float32 tensors of shape "
                                   f"[{HEAD_DIM}]")
    if float(q_norm[2]) != float(k_norm[2]):
        raise ValueError("rope_attention: q_norm and k_norm must share one eps")


def _check(q, k, v, qpos, kpos, mask=None, q_norm=None, k_norm=None) -> None:
    _check_tokens(q, k, v, 4, "tokens must have 4 dimensions")
    if k.shape != v.shape or q.shape[:2] != k.shape[:2]:
        raise RuntimeError(f"rope_attention: shapes differ: q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)}")
    if _have_positions(qpos, kpos):
        _check_positions(q, qpos)
        _check_positions(k, kpos)
    if mask is not None:
        _check_mask(mask, (q.shape[0], q.shape[1], q.shape[2], k.shape[2]))
    _check_norms(q_norm, k_norm)
    _check_on_device(q)
    extras = ([mask] if mask is not None else []) + (list(q_norm[:2]) + list(k_norm[:2]) if q_norm is not None else [])
    if any(t.device != q.device for t in extras):
        raise RuntimeError("rope_attention: the mask and the norm parameters must be on the tokens' device")


def _check_matrix16(dtype, mask=None, q_norm=None, k_norm=None) -> None:
    """What ``matrix16=True`` refuses, before anything else is looked at."""
    if mask is not None or q_norm is not None or k_norm is not None:
        raise NotImplementedError("rope_attention: matrix16=True is the plain call only; mask, q_norm and k_norm are not "
                                  "supported on the 16-bit matrix path yet")
    if dtype not in (torch.float16, torch.bfloat16):
        raise ValueError(f"rope_attention: matrix16=True needs float16 or bfloat16 tokens, got {dtype}")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """``t`` ([.., H, N, D], any rank) itself when the kernels can read it in place (unit stride along D, every other
    stride and the base 16-byte aligned), else a copy."""
    es = t.element_size()
    if t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all((s * es) % 16 == 0 for s in t.stride()[:-1]):
        return t
    return t.contiguous()


_rows5 = _rows          # the name the views tests know it by


def _strides(t: torch.Tensor):
    """(batch or scene, token, head) element strides of a [B,H,N,D] or [b,V,H,N,D] tensor."""
    return (C.c_int64 * 3)(t.stride(0), t.stride(-2), t.stride(-3))


def _args(q, k, v, qpos, kpos, base, F0, scale) -> _lib.SpfAttn:
    """SpfAttn of a call on [B,H,N,D] or [b,V,H,N,D] tokens (B: the scenes then; the views travel in SpfAttnViews)."""
    a = _lib.SpfAttn()
    a.q, a.k, a.v = q.data_ptr(), k.data_ptr(), v.data_ptr()
    a.qpos, a.kpos = _lib.ptr(qpos), _lib.ptr(kpos)
    a.q_stride, a.k_stride, a.v_stride = _strides(q), _strides(k), _strides(v)
    a.B, a.H, a.Nq, a.Nk, a.D = q.shape[0], q.shape[-3], q.shape[-2], k.shape[-2], q.shape[-1]
    a.dtype = _DTYPES[q.dtype]
    a.base, a.F0, a.scale = float(base), float(F0), float(scale)
    return a


def _grads(dq, dk, dv, delta) -> _lib.SpfAttnGrads:
    g = _lib.SpfAttnGrads()
    g.dq, g.dk, g.dv, g.delta = dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), delta.data_ptr()
    g.dq_stride, g.dk_stride, g.dv_stride = _strides(dq), _strides(dk), _strides(dv)
    return g


def _saved(out, dout, dtype):
    """What the forward saved and the incoming gradient, contiguous, for a backward launch."""
    out, dout = out.contiguous(), dout.contiguous()
    if dout.dtype != dtype or out.dtype != dtype:
        raise RuntimeError(f"rope_attention: gradient dtype {dout.dtype} differs from the inputs' {dtype}")
    return out, dout


def _mask_view(mask, shape):
    """The mask as a [B,H,Nq,Nk] view the kernels read in place: broadcast axes get stride 0; the key axis must have
    stride 1, so a mask that is strided or broadcast along it is copied once (as ``_rows`` does for tokens)."""
    if mask is None:
        return None
    m = mask.reshape((1,) * (4 - mask.dim()) + tuple(mask.shape))
    if shape[3] > 1 and (m.shape[3] == 1 or m.stride(3) != 1):
        m = m.expand(*m.shape[:3], shape[3]).contiguous()
    return m.expand(shape)


def _ext(mask, q_norm, k_norm, dnorm=None, partials=None) -> _lib.SpfAttnExt:
    """SpfAttnExt of a call; ``mask``: what ``_mask_view`` returned; ``dnorm`` [4,64] float32 and ``partials``: the
    backward's outputs and scratch."""
    e = _lib.SpfAttnExt()
    if mask is not None:
        e.mask, e.mask_dtype = mask.data_ptr(), int(mask.dtype == torch.bool)
        e.mask_stride = (C.c_int64 * 4)(mask.stride(0), mask.stride(1), mask.stride(2), 1)
    if q_norm is not None:
        e.q_weight, e.q_bias, e.k_weight, e.k_bias = (t.data_ptr() for t in (*q_norm[:2], *k_norm[:2]))
        e.eps = float(q_norm[2])
    if dnorm is not None:
        e.dq_weight, e.dq_bias, e.dk_weight, e.dk_bias = (dnorm[i].data_ptr() for i in range(4))
        e.partials = partials.data_ptr()
    return e


def _norm_tensors(n):
    return None if n is None else (n[0].detach().contiguous(), n[1].detach().contiguous(), float(n[2]))


def attention_forward(q, k, v, qpos, kpos, base, F0, scale, *, mask=None, q_norm=None, k_norm=None, matrix16=False):
    """The forward launch: (out [B,Nq,H*D], lse [B,H,Nq] float32).  q, k, v: [B,H,N,64] views, read in place.
    matrix16: the 16-bit matrix path (float16 / bfloat16, plain calls only)."""
    if matrix16:
        _check_matrix16(q.dtype, mask, q_norm, k_norm)
    _check(q, k, v, qpos, kpos, mask, q_norm, k_norm)
    q, k, v = _rows(q), _rows(k), _rows(v)
    B, H, Nq, D = q.shape
    out = torch.empty(B, Nq, H * D, dtype=q.dtype, device=q.device)
    lse = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
    mask = _mask_view(mask, (B, H, Nq, k.shape[2]))
    q_norm, k_norm = _norm_tensors(q_norm), _norm_tensors(k_norm)
    a = _args(q, k, v, qpos, kpos, base, F0, scale)
    if matrix16:
        _lib.launch("spf_attn16_forward", q.device, a, out, lse)
    else:                                               # (an empty SpfAttnExt: the library runs the plain kernels)
        _lib.launch("spf_attn_forward_ext", q.device, a, _ext(mask, q_norm, k_norm), out, lse)
    return out, lse


def attention_backward(q, k, v, qpos, kpos, base, F0, scale, out, lse, dout, dq, dk, dv, *, mask=None, q_norm=None,
                       k_norm=None, matrix16=False):
    """The backward launches: writes dq [B,H,Nq,64], dk, dv [B,H,Nk,64] (any views with 16-byte aligned rows, e.g. the
    three slices of one packed gradient) from what the forward saved.  With q_norm / k_norm it returns the gradients of
    the four norm parameters as one [4,64] float32 tensor (q weight, q bias, k weight, k bias), else None.
    matrix16: the 16-bit matrix path, on what a ``matrix16`` forward saved."""
    if matrix16:
        _check_matrix16(q.dtype, mask, q_norm, k_norm)
    _check(q, k, v, qpos, kpos, mask, q_norm, k_norm)
    q, k, v = _rows(q), _rows(k), _rows(v)
    out, dout = _saved(out, dout, q.dtype)
    B, H, Nq, D = q.shape
    delta = torch.empty(B, H, Nq, dtype=torch.float32, device=q.device)
    mask = _mask_view(mask, (B, H, Nq, k.shape[2]))
    dnorm = partials = None
    if q_norm is not None:
        q_norm, k_norm = _norm_tensors(q_norm), _norm_tensors(k_norm)
        n = _lib.load().spf_attn_ext_scratch_floats(B, H, Nq, k.shape[2])   # (the library's grid arithmetic, not ours)
        if n < 0:
            raise _lib.SpfError("spf_attn_ext_scratch_floats rejected the sizes")
        dnorm = torch.empty(4, HEAD_DIM, dtype=torch.float32, device=q.device)
        partials = torch.empty(n, dtype=torch.float32, device=q.device)
    a, g = _args(q, k, v, qpos, kpos, base, F0, scale), _grads(dq, dk, dv, delta)
    if matrix16:
        _lib.launch("spf_attn16_backward", q.device, a, g, out, lse, dout)
    else:
        _lib.launch("spf_attn_backward_ext", q.device, a, g, _ext(mask, q_norm, k_norm, dnorm, partials), out, lse,
                    dout)
    return dnorm


def _norm_args(q_norm, k_norm):
    """The autograd functions' flat arguments of the two norms: (q weight, q bias, k weight, k bias, eps)."""
    if q_norm is None:
        return None, None, None, None, 0.0
    return q_norm[0], q_norm[1], k_norm[0], k_norm[1], float(q_norm[2])


def _norm_pair(qw, qb, kw, kb, eps):
    """(q_norm, k_norm) back from the flat arguments."""
    return ((qw, qb, eps), (kw, kb, eps)) if qw is not None else (None, None)


def _norm_grads(ctx, first, dnorm):
    """Gradients of the four norm parameters at needs_input_grad[first:first + 4]."""
    if dnorm is None:
        return (None,) * 4
    return tuple(dnorm[i] if ctx.needs_input_grad[first + i] else None for i in range(4))


def _token_major(t):
    """An empty gradient for ``t`` [.., H, N, D] on a token-major buffer [.., N, H, D]: such a view is what a following
    reshape(.., N, C) wants."""
    *lead, H, N, D = t.shape
    return torch.empty(*lead, N, H, D, dtype=t.dtype, device=t.device).transpose(-3, -2)


class _RopeAttention(torch.autograd.Function):
    """mask, qw .. kb: None on a plain call."""

    @staticmethod
    def forward(ctx, q, k, v, qpos, kpos, mask, qw, qb, kw, kb, eps, base, F0, scale, matrix16=False):
        q_norm, k_norm = _norm_pair(qw, qb, kw, kb, eps)
        out, lse = attention_forward(q, k, v, qpos, kpos, base, F0, scale, mask=mask, q_norm=q_norm, k_norm=k_norm,
                                     matrix16=matrix16)
        ctx.save_for_backward(q, k, v, qpos, kpos, mask, qw, qb, kw, kb, out, lse)
        ctx.cfg = (base, F0, scale)
        ctx.eps = eps
        ctx.matrix16 = matrix16
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, qpos, kpos, mask, qw, qb, kw, kb, out, lse = ctx.saved_tensors
        q_norm, k_norm = _norm_pair(qw, qb, kw, kb, ctx.eps)
        dq, dk, dv = _token_major(q), _token_major(k), _token_major(v)
        dnorm = attention_backward(q, k, v, qpos, kpos, *ctx.cfg, out, lse, dout, dq, dk, dv, mask=mask, q_norm=q_norm,
                                   k_norm=k_norm, matrix16=ctx.matrix16)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None,
                *_norm_grads(ctx, 6, dnorm), None, None, None, None, None)


class _RopeAttentionPacked(torch.autograd.Function):
    """mask, qw .. kb: None on a plain call."""

    @staticmethod
    def forward(ctx, qkv, pos, mask, qw, qb, kw, kb, eps, base, F0, scale, matrix16=False):
        q_norm, k_norm = _norm_pair(qw, qb, kw, kb, eps)
        out, lse = attention_forward(*_views(qkv), pos, pos, base, F0, scale, mask=mask, q_norm=q_norm, k_norm=k_norm,
                                     matrix16=matrix16)
        ctx.save_for_backward(qkv, pos, mask, qw, qb, kw, kb, out, lse)
        ctx.cfg = (base, F0, scale)
        ctx.eps = eps
        ctx.matrix16 = matrix16
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        qkv, pos, mask, qw, qb, kw, kb, out, lse = ctx.saved_tensors
        q_norm, k_norm = _norm_pair(qw, qb, kw, kb, ctx.eps)
        dqkv = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        dnorm = attention_backward(*_views(qkv), pos, pos, *ctx.cfg, out, lse, dout, *_views(dqkv), mask=mask,
                                   q_norm=q_norm, k_norm=k_norm, matrix16=ctx.matrix16)
        return (dqkv, None, None, *_norm_grads(ctx, 3, dnorm), None, None, None, None, None)


def _views(qkv: torch.Tensor):
    """q, k, v [B,H,N,D] of a packed [B,N,3,H,D] buffer (blocks.py:97-98)."""
    t = qkv.transpose(1, 3)
    return t[:, :, 0], t[:, :, 1], t[:, :, 2]


def rope_attention(q, k, v, qpos=None, kpos=None, *, base: float = 100.0, F0: float = 1.0, scale=None, mask=None,
                   q_norm=None, k_norm=None, matrix16: bool = False):
    """softmax(scale * rope(norm(q), qpos) @ rope(norm(k), kpos)^T + mask) @ v, returned as [B,Nq,H*D].

    q [B,H,Nq,64], k and v [B,H,Nk,64]: any views with unit stride along D and 16-byte aligned rows are read in place
    (anything else is copied first).  qpos [B,Nq,2], kpos [B,Nk,2]: int64 (y, x), contiguous; both None: no rotation.
    mask: float32 (added to the scaled score; -inf excludes a key) or bool (True: the key takes part), 2 to 4
    dimensions broadcast to [B,H,Nq,Nk] and read in place (broadcast axes cost nothing); no gradient.  A row with
    every key excluded returns zeros and has zero gradients.  q_norm, k_norm: ``(weight, bias, eps)`` of a LayerNorm
    over the 64 elements of every row, float32 [64] each, both or neither; their gradients come out of the backward.
    matrix16: run a float16 / bfloat16 call on the 16-bit matrix units (q, k and the probabilities rounded once to the
    dtype as operands, float32 accumulation and softmax); refuses float32 tokens (ValueError) and mask / q_norm / k_norm
    (NotImplementedError).  Off: 16-bit tokens run the float32 compute path.
    """
    if matrix16:
        _check_matrix16(q.dtype if isinstance(q, torch.Tensor) else None, mask, q_norm, k_norm)
    _check(q, k, v, qpos, kpos, mask, q_norm, k_norm)
    if scale is None:
        scale = q.shape[3] ** -0.5
    return _RopeAttention.apply(q, k, v, qpos, kpos, mask, *_norm_args(q_norm, k_norm), float(base), float(F0),
                                float(scale), bool(matrix16))


def rope_attention_packed(qkv, pos=None, *, base: float = 100.0, F0: float = 1.0, scale=None, mask=None, q_norm=None,
                          k_norm=None, matrix16: bool = False):
    """Self-attention on a packed projection qkv [B,N,3,H,64] (what ``self.qkv(x).reshape(B, N, 3, H, D)`` yields):
    the same result as ``rope_attention`` on its three views, and ONE gradient of the packed shape out of the backward
    instead of three that autograd would have to add up.  mask, q_norm, k_norm, matrix16: as in ``rope_attention``."""
    if matrix16:
        _check_matrix16(qkv.dtype if isinstance(qkv, torch.Tensor) else None, mask, q_norm, k_norm)
    if qkv.dim() != 5 or qkv.shape[2] != 3:
        raise RuntimeError(f"rope_attention_packed: qkv must be [B,N,3,H,D], got {tuple(qkv.shape)}")
    _check(*_views(qkv), pos, pos, mask, q_norm, k_norm)
    if not qkv.is_contiguous():
        qkv = qkv.contiguous()
    if scale is None:
        scale = qkv.shape[4] ** -0.5
    return _RopeAttentionPacked.apply(qkv, pos, mask, *_norm_args(q_norm, k_norm), float(base), float(F0), float(scale),
                                      bool(matrix16))


# ---- multi-view: one key set per scene, whole views left out per query view ------------------------------------------
MAX_VIEWS = 32


def allow_words(allow):
    """``allow`` ([Vq, Vk] bool CPU tensor or nested sequence: query view i may read key view s) as
    ``(words, Vq, Vk)``: one 32-bit word per query view, bit s of word i set iff ``allow[i][s]``.  Host only."""
    if isinstance(allow, torch.Tensor):
        if allow.is_cuda:
            raise RuntimeError("rope_attention_views: allow must be a CPU tensor (it is packed on the host and never "
                               "touches the device)")
        if allow.dtype != torch.bool:
            raise RuntimeError(f"rope_attention_views: allow must be bool, got {allow.dtype}")
        if allow.dim() != 2:
            raise RuntimeError(f"rope_attention_views: allow must be [Vq, Vk], got {tuple(allow.shape)}")
        rows = allow.tolist()
    else:
        try:
            rows = [list(r) for r in allow]
        except TypeError as e:
            raise TypeError("rope_attention_views: allow must be a [Vq, Vk] bool tensor or a nested sequence") from e
    Vq = len(rows)
    Vk = len(rows[0]) if rows else 0
    if any(len(r) != Vk for r in rows):
        raise RuntimeError("rope_attention_views: the rows of allow differ in length")
    if not (1 <= Vq <= MAX_VIEWS and 1 <= Vk <= MAX_VIEWS):
        raise ValueError(f"rope_attention_views: Vq and Vk must be 1 .. {MAX_VIEWS}, got {Vq} and {Vk}")
    words = [sum(1 << s for s, on in enumerate(r) if on) for r in rows]
    for i, w in enumerate(words):
        if w == 0:
            raise ValueError(f"rope_attention_views: query view {i} is allowed no key view")
    return words, Vq, Vk


def _check_view_positions(name, tokens, positions) -> None:
    if positions.dim() != 4 or tuple(positions.shape) != (tokens.shape[0], tokens.shape[1], tokens.shape[3], 2):
        raise RuntimeError(f"rope_attention_views: {name} must be [b, V, N, 2] = "
                           f"{[tokens.shape[0], tokens.shape[1], tokens.shape[3], 2]}, got {list(positions.shape)}")
    if positions.dtype != torch.int64:
        raise RuntimeError("positions must be int64")
    if positions.device != tokens.device:
        raise RuntimeError("tokens and positions are not on the same device")


def _check_views(q, k, v, qpos, kpos, words, Vq, Vk) -> None:
    _check_tokens(q, k, v, 5, "rope_attention_views: q, k and v must have 5 dimensions [b, V, H, N, 64]")
    if k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise RuntimeError(f"rope_attention_views: shapes differ: q {tuple(q.shape)}, k {tuple(k.shape)}, "
                           f"v {tuple(v.shape)}")
    if (q.shape[1], k.shape[1]) != (Vq, Vk):
        raise RuntimeError(f"rope_attention_views: allow is [{Vq}, {Vk}] but q has {q.shape[1]} views and k has "
                           f"{k.shape[1]}")
    if _have_positions(qpos, kpos):
        _check_view_positions("qpos", q, qpos)
        _check_view_positions("kpos", k, kpos)
    _check_on_device(q)


def _pos_rows(p):
    """Positions [b, V, N, 2] whose (token, 2) rows are contiguous: read in place through (scene, view) strides."""
    if p is None or (p.stride(3) == 1 and p.stride(2) == 2) or p.shape[2] == 1 and p.stride(3) == 1:
        return p
    return p.contiguous()


def _view_ext(q, k, v, qpos, kpos, words) -> _lib.SpfAttnViews:
    """What a [b,V,H,N,D] call hands the library next to ``_args``: the view counts, words and strides."""
    w = _lib.SpfAttnViews()
    w.Vq, w.Vk = q.shape[1], k.shape[1]
    w.allow = (C.c_uint32 * 32)(*words)
    w.q_view_stride, w.k_view_stride, w.v_view_stride = q.stride(1), k.stride(1), v.stride(1)
    if qpos is not None:
        w.qpos_stride = (C.c_int64 * 2)(qpos.stride(0), qpos.stride(1))
        w.kpos_stride = (C.c_int64 * 2)(kpos.stride(0), kpos.stride(1))
    return w


def attention_views_forward(q, k, v, qpos, kpos, words, base, F0, scale):
    """The forward launch: (out [b,Vq,Nq,H*D], lse [b,Vq,H,Nq] float32).  q [b,Vq,H,Nq,64], k and v [b,Vk,H,Nk,64]: views,
    read in place; ``words``: what ``allow_words`` returned."""
    _check_views(q, k, v, qpos, kpos, words, len(words), k.shape[1] if k.dim() == 5 else 0)
    q, k, v, qpos, kpos = _rows(q), _rows(k), _rows(v), _pos_rows(qpos), _pos_rows(kpos)
    b, Vq, H, Nq, D = q.shape
    out = torch.empty(b, Vq, Nq, H * D, dtype=q.dtype, device=q.device)
    lse = torch.empty(b, Vq, H, Nq, dtype=torch.float32, device=q.device)
    _lib.launch("spf_attn_views_forward", q.device, _args(q, k, v, qpos, kpos, base, F0, scale),
                _view_ext(q, k, v, qpos, kpos, words), out, lse)
    return out, lse


def attention_views_backward(q, k, v, qpos, kpos, words, base, F0, scale, out, lse, dout, dq, dk, dv):
    """The backward launches: writes dq [b,Vq,H,Nq,64], dk, dv [b,Vk,H,Nk,64] (any views with 16-byte aligned rows, e.g.
    slices of larger tensors), every row once; a key view nobody reads gets zeros."""
    _check_views(q, k, v, qpos, kpos, words, len(words), k.shape[1] if k.dim() == 5 else 0)
    if dq.shape != q.shape or dk.shape != k.shape or dv.shape != v.shape:
        raise RuntimeError("rope_attention_views: dq, dk and dv must have the shapes of q, k and v")
    if any(t.stride(4) != 1 or t.dtype != q.dtype for t in (dq, dk, dv)):
        raise RuntimeError("rope_attention_views: dq, dk and dv must have unit stride along D and the inputs' dtype")
    q, k, v, qpos, kpos = _rows(q), _rows(k), _rows(v), _pos_rows(qpos), _pos_rows(kpos)
    out, dout = _saved(out, dout, q.dtype)
    b, Vq, H, Nq, D = q.shape
    delta = torch.empty(b, Vq, H, Nq, dtype=torch.float32, device=q.device)
    w = _view_ext(q, k, v, qpos, kpos, words)
    w.dq_view_stride, w.dk_view_stride, w.dv_view_stride = dq.stride(1), dk.stride(1), dv.stride(1)
    _lib.launch("spf_attn_views_backward", q.device, _args(q, k, v, qpos, kpos, base, F0, scale), w,
                _grads(dq, dk, dv, delta), out, lse, dout)


class _RopeAttentionViews(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, qpos, kpos, words, base, F0, scale):
        out, lse = attention_views_forward(q, k, v, qpos, kpos, words, base, F0, scale)
        ctx.save_for_backward(q, k, v, qpos, kpos, out, lse)
        ctx.cfg = (words, base, F0, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        q, k, v, qpos, kpos, out, lse = ctx.saved_tensors
        dq, dk, dv = _token_major(q), _token_major(k), _token_major(v)
        attention_views_backward(q, k, v, qpos, kpos, *ctx.cfg, out, lse, dout, dq, dk, dv)
        need = ctx.needs_input_grad
        return (dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None,
                None)


def rope_attention_views(q, k, v, qpos=None, kpos=None, *, allow, base: float = 100.0, F0: float = 1.0, scale=None):
    """Cross-attention of a scene's query views over ONE shared set of key views, whole views left out per query view:

        out[b,i] = softmax_j(scale * rope(q[b,i], qpos[b,i]) @ rope(k[b,s,j], kpos[b,s])^T) @ v[b,s,j],
                   j over all tokens of all key views s with allow[i][s], views ascending

    -- what ``rope_attention`` returns for query batch item (b, i) on the keys of the allowed views gathered in
    ascending order, without the gather.  q [b,Vq,H,Nq,64], k and v [b,Vk,H,Nk,64]: views with unit stride along D and
    16-byte aligned rows are read in place (``x[:, 1:]`` of a projection included).  qpos [b,Vq,Nq,2], kpos [b,Vk,Nk,2]:
    int64 (y, x); both None: no rotation.  allow: [Vq, Vk] bool CPU tensor or nested sequence, Vq, Vk <= 32, at least one
    key view per query view; it is packed into one word per query view on the host and never touches the device.
    Returns [b,Vq,Nq,H*64].  The gradient of a key view is written once (no atomics, bitwise reproducible) and is exact
    zeros for a key view nobody reads."""
    words, Vq, Vk = allow_words(allow)
    _check_views(q, k, v, qpos, kpos, words, Vq, Vk)
    if scale is None:
        scale = q.shape[4] ** -0.5
    return _RopeAttentionViews.apply(q, k, v, qpos, kpos, tuple(words), float(base), float(F0), float(scale))


class ViewSet(tuple):
    """(query view slice, key view slice, allow [Vq, Vk] bool CPU tensor) of one decoder block."""
    __slots__ = ()

    def __new__(cls, query, key, allow):
        return super().__new__(cls, (query, key, allow))

    query = property(lambda self: self[0])
    key = property(lambda self: self[1])
    allow = property(lambda self: self[2])


def decoder_view_sets(v: int, num_target: int = 0):
    """The view sets of the two decoder blocks of the multi-view backbones, as ``(blk1, blk2)`` of
    ``ViewSet(query view slice, key view slice, allow)``; ``v`` views of which the last ``num_target`` are targets,
    ``vc = v - num_target`` context views.

    blk1 (backbone_croco_multiview.py:191, backbone_masked_croco.py's first branch): query view 0 over key views
    1 .. vc-1, all allowed.  blk2: query views 1 .. v-1 over key views 0 .. v-1 with ``allow[i][s]`` iff ``s != i`` and
    (``i >= vc`` or ``s < vc``): a context view sees the other context views, a target view sees every other view --
    ONE call where the masked backbone makes one for the context and one for the target queries.  Host code only."""
    v, num_target = int(v), int(num_target)
    vc = v - num_target
    if num_target < 0 or vc < 2:
        raise ValueError(f"decoder_view_sets: {v} views with {num_target} targets leave {vc} context views; blk1 needs "
                         "at least 2 (view 0 would have no keys)")
    if v > MAX_VIEWS:
        raise ValueError(f"decoder_view_sets: at most {MAX_VIEWS} views, got {v}")
    allow1 = torch.ones(1, vc - 1, dtype=torch.bool)
    allow2 = torch.tensor([[s != i and (i >= vc or s < vc) for s in range(v)] for i in range(1, v)], dtype=torch.bool)
    return ViewSet(slice(0, 1), slice(1, vc), allow1), ViewSet(slice(1, v), slice(0, v), allow2)


def _rope_cfg(rope) -> dict:
    """The rotation's keyword arguments of a rope_attention call; empty (false) without a rope."""
    if rope is None:
        return {}
    if not (hasattr(rope, "base") and hasattr(rope, "F0")):
        raise TypeError(f"rope must be a cuRoPE2D (base, F0) or None, got {type(rope).__name__}")
    return {"base": float(rope.base), "F0": float(rope.F0)}


def _check_module(mod, mask=None) -> None:
    if mask is not None:
        raise NotImplementedError("attention masks are not supported by the fused kernel (the reference's live path, "
                                  "'mask v2', passes none)")
    if mod.training and mod.attn_drop.p > 0:
        raise NotImplementedError("attn_drop > 0 in training mode is not supported by the fused kernel")


def _module_rope(mod, x, what: str, head_dim: int, *pos, then=None):
    """What the three module forwards settle before they project: the head dim, the rope configuration and that ``x``
    (named ``what`` in the message) is on a device -- with ``then()``, forward_views' own checks, at the place between
    them where they have always fired.  Returns (rope keyword arguments, positions); no rope: positions of None."""
    if head_dim != HEAD_DIM:
        raise ValueError(f"rope_attention: head dim must be {HEAD_DIM}, got {head_dim}")
    if then is not None:
        then()
    cfg = _rope_cfg(mod.rope)
    if not x.is_cuda:
        raise RuntimeError(f"{what} is on the CPU; this build only runs on a HIP device (no CPU fallback)")
    return cfg, pos if cfg else (None,) * len(pos)


def _use_matrix16(mod, t: torch.Tensor) -> bool:
    """A flagged module takes the 16-bit matrix path for 16-bit projections and the float32 path, bit for bit, for
    float32 ones: one flag serves a model inside and outside autocast."""
    return bool(getattr(mod, "matrix16", False)) and t.dtype in (torch.float16, torch.bfloat16)


class Attention(nn.Module):
    """blocks.py:81-113 with the fused core; same parameters, same state dict.  matrix16 (keyword-only, also an
    attribute): 16-bit projections (autocast, a half model) run on the 16-bit matrix units; float32 ones are unaffected."""

    def __init__(self, dim, rope=None, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., *, matrix16=False):
        super().__init__()
        self.matrix16 = bool(matrix16)
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.rope = rope

    def forward(self, x, xpos):
        B, N, C = x.shape
        _check_module(self)
        cfg, (xpos,) = _module_rope(self, x, "Attention: x", C // self.num_heads, xpos)
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads)
        x = rope_attention_packed(qkv, xpos, scale=self.scale, matrix16=_use_matrix16(self, qkv), **cfg)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x


class CrossAttention(nn.Module):
    """blocks.py:133-179 with the fused core; same parameters, same state dict.  matrix16 (keyword-only, also an
    attribute): as in ``Attention``; ``forward_views`` ignores it (the multi-view kernels have no 16-bit matrix form yet)."""

    def __init__(self, dim, rope=None, num_heads=8, qkv_bias=False, attn_drop=0., proj_drop=0., *, matrix16=False):
        super().__init__()
        self.matrix16 = bool(matrix16)
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = head_dim ** -0.5
        self.projq = nn.Linear(dim, dim, bias=qkv_bias)
        self.projk = nn.Linear(dim, dim, bias=qkv_bias)
        self.projv = nn.Linear(dim, dim, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.rope = rope

    def forward(self, query, key, value, qpos, kpos, mask=None):
        B, Nq, C = query.shape
        Nk = key.shape[1]
        Nv = value.shape[1]
        _check_module(self, mask)
        H, D = self.num_heads, C // self.num_heads
        cfg, (qpos, kpos) = _module_rope(self, query, "CrossAttention: query", D, qpos, kpos)
        q = self.projq(query).reshape(B, Nq, H, D).permute(0, 2, 1, 3)
        k = self.projk(key).reshape(B, Nk, H, D).permute(0, 2, 1, 3)
        v = self.projv(value).reshape(B, Nv, H, D).permute(0, 2, 1, 3)
        x = rope_attention(q, k, v, qpos, kpos, scale=self.scale, matrix16=_use_matrix16(self, q), **cfg)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x

    def forward_views(self, query, key, qpos, kpos, allow):
        """The layer on a scene's views without gathered keys: query [b,Vq,Nq,C], key [b,Vk,Nk,C] (key and value, as at
        every call site of the reference), qpos [b,Vq,Nq,2], kpos [b,Vk,Nk,2], allow [Vq,Vk] (``rope_attention_views``).
        ``projk`` and ``projv`` run ONCE over the b*Vk*Nk key tokens; returns [b,Vq,Nq,C].  Same parameters as
        ``forward``.  The module's ``matrix16`` flag is ignored here: this call always runs the float32 compute path."""
        _check_module(self)
        if query.dim() != 4 or key.dim() != 4:
            raise RuntimeError("CrossAttention.forward_views: query and key must be [b, V, N, C]")
        b, Vq, Nq, C_ = query.shape
        _, Vk, Nk, _ = key.shape
        H, D = self.num_heads, C_ // self.num_heads

        def allow_fits():
            _, aq, ak = allow_words(allow)
            if (aq, ak) != (Vq, Vk) or key.shape[0] != b:
                raise RuntimeError(f"CrossAttention.forward_views: allow is [{aq}, {ak}], query {tuple(query.shape)}, "
                                   f"key {tuple(key.shape)}")

        cfg, (qpos, kpos) = _module_rope(self, query, "CrossAttention: query", D, qpos, kpos, then=allow_fits)
        q = self.projq(query).reshape(b, Vq, Nq, H, D).transpose(2, 3)
        k = self.projk(key).reshape(b, Vk, Nk, H, D).transpose(2, 3)
        v = self.projv(key).reshape(b, Vk, Nk, H, D).transpose(2, 3)
        x = rope_attention_views(q, k, v, qpos, kpos, allow=allow, scale=self.scale, **cfg)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x
