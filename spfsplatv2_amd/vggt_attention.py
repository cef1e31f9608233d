"""VGGT's attention layer on the fused kernels: ``vggt/layers/attention.py:Attention`` of the reference's
``masked_vggt`` backbone (24 frame and 24 global blocks of ``vggt/models/aggregator.py``).

What it adds to CroCo's layer (attention.py): a ``LayerNorm(64)`` of every q and every k row before the rotation
(``qk_norm=True``, aggregator.py:68) and the additive mask of the global blocks (a dense ``[1,1,S*P,S*P]`` float32
tensor of 0 / -inf, aggregator.py:342-356).  Both run inside the one packed call of ``rope_attention_packed``: no
LayerNorm launch, no rotation launch, no score tensor, and the mask is read in place.

A query row whose keys are all excluded returns zeros and has zero gradients (what ``F.scaled_dot_product_attention``
returns today); see INTEGRATION.md section 3b.
"""
from __future__ import annotations

import torch
from torch import nn

from .attention import HEAD_DIM, _check_mask, rope_attention_packed


class VGGTAttention(nn.Module):
    """attention.py:21-84 of the reference with the fused core: same constructor arguments, same state dict (``qkv.*``,
    ``q_norm.*``, ``k_norm.*``, ``proj.*``), ``forward(x, pos=None, mask=None)``.  ``rope``: this package's
    ``RotaryPositionEmbedding2D`` (its ``base_frequency`` is read) or None.  ``fused_attn`` is kept for the signature:
    the reference's two branches are one formula."""

    def __init__(self, dim: int, num_heads: int = 8, qkv_bias: bool = True, proj_bias: bool = True, attn_drop: float = 0.0,
                 proj_drop: float = 0.0, norm_layer=nn.LayerNorm, qk_norm: bool = False, fused_attn: bool = True,
                 rope=None) -> None:
        super().__init__()
        assert dim % num_heads == 0, "dim should be divisible by num_heads"
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.scale = self.head_dim ** -0.5
        self.fused_attn = fused_attn
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.q_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.k_norm = norm_layer(self.head_dim) if qk_norm else nn.Identity()
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim, bias=proj_bias)
        self.proj_drop = nn.Dropout(proj_drop)
        self.rope = rope

    def _norm(self, layer):
        """(weight, bias, eps) of q_norm / k_norm, or None for the Identity of qk_norm=False."""
        if isinstance(layer, nn.Identity):
            return None
        if not (type(layer) is nn.LayerNorm and tuple(layer.normalized_shape) == (HEAD_DIM,)
                and layer.weight is not None and layer.bias is not None):
            raise TypeError("VGGTAttention: qk_norm needs norm_layer = nn.LayerNorm over the 64 elements of a head with "
                            f"affine parameters, got {layer!r}")
        return layer.weight, layer.bias, layer.eps

    def forward(self, x: torch.Tensor, pos=None, mask=None) -> torch.Tensor:
        B, N, C = x.shape
        if self.head_dim != HEAD_DIM:
            raise ValueError(f"rope_attention: head dim must be {HEAD_DIM}, got {self.head_dim}")
        q_norm, k_norm = self._norm(self.q_norm), self._norm(self.k_norm)
        if self.rope is not None and not hasattr(self.rope, "base_frequency"):
            raise TypeError("rope must be a RotaryPositionEmbedding2D (base_frequency) or None, got "
                            f"{type(self.rope).__name__}")
        if self.rope is not None and pos is None:
            raise RuntimeError("VGGTAttention: the layer has a rope, so pos must be given")
        if mask is not None:
            _check_mask(mask, (B, self.num_heads, N, N))
        if self.training and self.attn_drop.p > 0:
            raise NotImplementedError("attn_drop > 0 in training mode is not supported by the fused kernel")
        if not x.is_cuda:
            raise RuntimeError("VGGTAttention: x is on the CPU; this build only runs on a HIP device (no CPU fallback)")
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, self.head_dim)
        cfg = {"base": float(self.rope.base_frequency)} if self.rope is not None else {}
        x = rope_attention_packed(qkv, pos if cfg else None, scale=self.scale, mask=mask, q_norm=q_norm, k_norm=k_norm,
                                  **cfg)
        x = self.proj(x)
        x = self.proj_drop(x)
        return x
