"""The encoder tail on the HIP library (csrc/tail.hip): the heads' outputs, where they lie, -> the decoder's ``Gaussians``.

Host mirror of the lines of the reference's encoders between its heads and its decoder
(src/model/encoder/encoder_spfsplatv2.py:218-224, 240, 248-268, 296-321, the same lines of
encoder_spfsplat.py, and encoder_spfsplatv2l.py:173-186): ``rearrange(GS_res, "b d h w -> b (h w) d")`` per view,
``torch.stack`` over the views, ``gaussians[..., 0].sigmoid()``, ``map_pdf_to_opacity``, ``UnifiedGaussianAdapter.forward``
and the rearranges to ``[b, (v h w), ...]``.  ``gaussians_from_heads`` is one launch per direction: it reads every view's
channel-major ``[b, 1 + 7 + 3 d_sh, h, w]`` head output and ``[b, h, w, 3]`` point map in place and writes the stacked
tensors the decoder reads; its backward writes each view's gradient in that view's own layout, every byte once.
``density_to_opacity`` is the fused sigmoid + opacity map alone, for a head output that is already in rows.

The density channel is mapped in logarithms (log p = logsigmoid(x), log(1 - p) = logsigmoid(-x)), so outputs and
gradients are finite for every finite logit; float32 autograd of the reference's expression returns NaN gradients for
saturated logits (x >= 17 with an exponent below 1, x <= -104 with one above).

Not served: ``num_surfaces != 1``, 16-bit tensors, CPU tensors, ``sh_degree > 4``.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from .adapter import GaussianAdapterCfg, Gaussians
from ._checks import check_device as _check_device, check_float32 as _check_float32

MAX_VIEWS = _lib.TAIL_MAX_VIEWS
MAX_ELEMENTS = 2 ** 31 - 1

# every copy ``_dense`` makes (as heads.dense_copies): head outputs that are dense and 16-byte aligned -- a convolution's
# output, or a slice of a larger allocation at an aligned offset -- are read in place and this stays at 0
dense_copies = {"calls": 0, "bytes": 0}


def max_grid() -> int:
    """The most blocks a launch of csrc/tail.hip uses (a block takes 64-pixel tiles, grid-stride).  Host only."""
    return int(_lib.load().spf_tail_max_grid())


def _dense(t):
    if t is None:
        return None
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    dense_copies["calls"] += 1
    dense_copies["bytes"] += t.numel() * t.element_size()
    return t.contiguous() if not t.is_contiguous() else t.clone()


def _grad(g):
    """An upstream gradient as the kernels read it (not counted: ``dense_copies`` is about the head outputs)."""
    if g is None:
        return None
    g = g.float().contiguous()
    return g if g.data_ptr() % 16 == 0 else g.clone()


def sh_mask(sh_degree: int) -> Tensor:
    """gaussian_adapter.py:41-48: band l >= 1 is scaled by 0.1 * 0.25 ** l."""
    mask = torch.ones(((sh_degree + 1) ** 2,), dtype=torch.float32)
    for degree in range(1, sh_degree + 1):
        mask[degree ** 2:(degree + 1) ** 2] = 0.1 * 0.25 ** degree
    return mask


# the mask on the device, made once per (sh_degree, device): a call uploads nothing and never waits for the stream
_DEVICE_MASKS = {}


def _device_mask(sh_degree: int, device) -> Tensor:
    key = (int(sh_degree), torch.device(device))
    mask = _DEVICE_MASKS.get(key)
    if mask is None:
        mask = _DEVICE_MASKS[key] = sh_mask(sh_degree).to(device)
    return mask


def _tail_args(raw, pts, mask, exponent, eps) -> _lib.SpfTail:
    b, c, h, w = raw[0].shape
    a = _lib.SpfTail()
    for i, t in enumerate(raw):
        a.raw[i] = t.data_ptr()
    for i, t in enumerate(pts or ()):
        a.pts[i] = t.data_ptr()
    a.sh_mask, a.hw, a.b, a.v, a.K = mask.data_ptr(), h * w, b, len(raw), (c - 8) // 3
    a.exponent, a.eps = float(exponent), float(eps)
    return a


class _TailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, exponent, eps, mask, split, *tensors):
        ctx.set_materialize_grads(False)
        pts = [_dense(t.detach()) for t in tensors[:v]]
        raw = [_dense(t.detach()) for t in tensors[v:]]
        b, c, h, w = raw[0].shape
        K, G = (c - 8) // 3, v * h * w
        f32 = dict(dtype=torch.float32, device=raw[0].device)
        means, opac = torch.empty((b, G, 3), **f32), torch.empty((b, G), **f32)
        scales, rot = torch.empty((b, G, 3), **f32), torch.empty((b, G, 4), **f32)
        sh = torch.empty((b, G, 3, 16 if split else K), **f32)
        sh_hi = torch.empty((b, G, 3, 9), **f32) if split else None
        _lib.launch("spf_tail_forward", raw[0].device, _tail_args(raw, pts, mask, exponent, eps), means, opac, scales, rot,
                    sh, sh_hi)
        ctx.save_for_backward(mask, *raw)
        ctx.v, ctx.exponent, ctx.eps, ctx.split = v, float(exponent), float(eps), bool(split)
        return (means, opac, scales, rot, sh, sh_hi) if split else (means, opac, scales, rot, sh)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_means, g_opac, g_scales, g_rot, g_sh, g_sh_hi=None):
        mask, *raw = ctx.saved_tensors
        b, c, h, w = raw[0].shape
        # (a decoder that evaluates to degree 3 hands back NO gradient for the band-4 plane -- None here -- and the kernel
        #  then writes zeros for those channels without reading anything; likewise for every other absent gradient)
        ups = [_grad(g) for g in (g_means, g_opac, g_scales, g_rot, g_sh, g_sh_hi)]
        out = _lib.SpfTailGrads()
        d_raw = [torch.empty_like(t) for t in raw]
        d_pts = [torch.empty((b, h, w, 3), dtype=torch.float32, device=t.device) for t in raw]
        for i in range(ctx.v):
            out.d_raw[i], out.d_pts[i] = d_raw[i].data_ptr(), d_pts[i].data_ptr()
        _lib.launch("spf_tail_backward", raw[0].device, _tail_args(raw, None, mask, ctx.exponent, ctx.eps), *ups,
                    1 if ctx.split else 0, out)
        return (None, None, None, None, None, *d_pts, *d_raw)


def _check_heads(what: str, pts3d, raw, sh_degree: int):
    pts3d, raw = list(pts3d), list(raw)
    if len(pts3d) != len(raw):
        raise ValueError(f"{what}: {len(pts3d)} point maps for {len(raw)} head outputs")
    if not 1 <= len(raw) <= MAX_VIEWS:
        raise ValueError(f"{what}: the number of views must be 1 .. {MAX_VIEWS}, got {len(raw)}")
    if not 0 <= sh_degree <= 4:
        raise NotImplementedError(f"{what}: sh_degree {sh_degree} is not served (0 .. 4: d_sh = 1, 4, 9, 16, 25)")
    _check_float32(what, *pts3d, *raw)
    d_sh = (sh_degree + 1) ** 2
    if raw[0].dim() != 4:
        raise RuntimeError(f"{what}: a head output must be [b, 1 + 7 + 3 d_sh, h, w], got shape {list(raw[0].shape)}")
    b, c, h, w = raw[0].shape
    if c != 1 + 7 + 3 * d_sh:
        raise RuntimeError(f"{what}: a head output has {c} channels, expected {1 + 7 + 3 * d_sh} (1 + 7 + 3 d_sh)")
    for i, (p, r) in enumerate(zip(pts3d, raw)):
        if tuple(r.shape) != (b, c, h, w):
            raise ValueError(f"{what}: views of unequal shape: raw[{i}] is {list(r.shape)}, raw[0] {[b, c, h, w]}")
        if tuple(p.shape) != (b, h, w, 3):
            raise ValueError(f"{what}: pts3d[{i}] must be {[b, h, w, 3]}, got {list(p.shape)}")
    if b * c * h * w == 0 or b * c * h * w > MAX_ELEMENTS or b * len(raw) * h * w * 3 * d_sh > MAX_ELEMENTS:
        raise RuntimeError(f"{what}: a tensor must hold 1 .. 2^31 - 1 elements, got head outputs of shape {[b, c, h, w]}")
    return pts3d, raw


def gaussians_from_heads(pts3d: Sequence[Tensor], raw: Sequence[Tensor], exponent: float = 1.0, *, sh_degree: int,
                         eps: float = 1e-8, split_harmonics: bool = False, with_covariances: bool = False) -> Gaussians:
    """``pts3d``: per context view the point head's ``[b, h, w, 3]``; ``raw``: per view the gs_params head's
    ``[b, 1 + 7 + 3 d_sh, h, w]``; ``exponent``: the opacity map's (``GaussianTail`` computes it from the step).  Returns
    the ``Gaussians`` of encoder_spfsplatv2.py:296-321 -- every field ``[b, v h w, ...]``, contiguous, Gaussian
    ``vi h w + y w + x`` is pixel (y, x) of view vi -- differentiable in all 2 v tensors.  ``means.view(b, v, h, w, 3)``
    is the stacked point map ``process_depth`` and ``estimate_intrinsics`` take.  ``split_harmonics`` (d_sh = 25):
    ``harmonics`` [.., 3, 16] + ``harmonics_band4`` [.., 3, 9].  ``with_covariances``: built by
    ``adapter_cov.build_covariance``; otherwise the field is a zero-stride NaN tensor, as in ``UnifiedGaussianAdapter``."""
    what = "gaussians_from_heads"
    pts3d, raw = _check_heads(what, pts3d, raw, sh_degree)
    if split_harmonics and sh_degree != 4:
        raise ValueError("split_harmonics is the 16 + 9 split of sh_degree 4 (d_sh = 25)")
    exponent = float(exponent)
    if not 0.0 < exponent < float("inf"):
        raise ValueError(f"{what}: the exponent must be positive and finite, got {exponent}")
    _check_device(what, raw[0], *raw[1:], *pts3d)
    mask = _device_mask(sh_degree, raw[0].device)
    res = _TailFn.apply(len(raw), exponent, float(eps), mask, bool(split_harmonics), *pts3d, *raw)
    means, opac, scales, rot, sh = res[:5]
    if with_covariances:
        from .adapter_cov import build_covariance
        cov = build_covariance(scales, rot)
    else:
        cov = torch.full((), float("nan"), dtype=torch.float32, device=means.device).expand(*scales.shape[:-1], 3, 3)
    return Gaussians(means=means, covariances=cov, scales=scales, rotations=rot, harmonics=sh, opacities=opac,
                     harmonics_band4=res[5] if split_harmonics else None)


def _attr(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def opacity_exponent(global_step: int, opacity_mapping) -> float:
    """encoder_spfsplatv2.py:154-156, on the host: ``opacity_mapping`` has ``initial``, ``final`` and ``warm_up``."""
    initial, final, warm_up = (float(_attr(opacity_mapping, n)) for n in ("initial", "final", "warm_up"))
    return 2.0 ** (initial + min(global_step / warm_up, 1) * (final - initial))


def map_pdf_to_opacity(pdf: Tensor, global_step: int, opacity_mapping) -> Tensor:
    """The reference's method on a probability tensor (encoder_spfsplatv2.py:146-159), in plain torch operations, for
    drop-in callers.  ``density_to_opacity`` is the fused form on the logits."""
    exponent = opacity_exponent(global_step, opacity_mapping)
    return 0.5 * (1 - (1 - pdf) ** exponent + pdf ** (1 / exponent))


class _OpacityFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, exponent):
        x = logits.detach()
        # one element stride over the whole view (channel 0 of a dense channels-last tensor): read in place
        stride = _uniform_stride(x)
        if stride is None:
            dense_copies["calls"] += 1
            dense_copies["bytes"] += x.numel() * x.element_size()
            x, stride = x.contiguous(), 1
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _lib.launch("spf_opacity_forward", x.device, x, stride, x.numel(), exponent, out)
        ctx.save_for_backward(x)
        ctx.stride, ctx.exponent = stride, exponent
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = g.contiguous().float()
        dx = torch.empty(x.shape, dtype=torch.float32, device=x.device)
        _lib.launch("spf_opacity_backward", x.device, x, ctx.stride, x.numel(), ctx.exponent, g, dx)
        return dx, None


def _uniform_stride(x: Tensor) -> Optional[int]:
    """s such that element i of ``x`` (row-major order) lies i * s elements from the first, or None."""
    s = None
    want = 1
    for size, stride in zip(reversed(x.shape), reversed(x.stride())):
        if size == 1:
            continue
        if s is None:
            s = stride
            if s < 1:
                return None
        elif stride != s * want:
            return None
        want *= size
    return 1 if s is None else s


def density_to_opacity(logits: Tensor, exponent: float = 1.0) -> Tensor:
    """``map(sigmoid(logits))`` of encoder_spfsplatv2l.py:176,184 in one launch each way; ``logits`` may be a strided view
    such as ``gaussians[..., 0]`` of a ``[.., 83]`` tensor, which is read in place.  Same shape out, contiguous."""
    what = "density_to_opacity"
    _check_float32(what, logits)
    exponent = float(exponent)
    if not 0.0 < exponent < float("inf"):
        raise ValueError(f"{what}: the exponent must be positive and finite, got {exponent}")
    _check_device(what, logits)
    if logits.numel() == 0:
        return torch.empty(logits.shape, dtype=torch.float32, device=logits.device)
    return _OpacityFn.apply(logits, exponent)


class GaussianTail(nn.Module):
    """The encoder's tail as a module without parameters: ``forward(pts3d, raw, global_step)`` computes the opacity map's
    exponent on the host (``global_step`` is a Python int: no sync) and calls ``gaussians_from_heads``."""

    def __init__(self, adapter_cfg: GaussianAdapterCfg, opacity_mapping, split_harmonics: bool = False,
                 num_surfaces: int = 1):
        super().__init__()
        if num_surfaces != 1:
            raise NotImplementedError(f"GaussianTail: num_surfaces = {num_surfaces} is not served (only 1)")
        if split_harmonics and adapter_cfg.sh_degree != 4:
            raise ValueError("split_harmonics is the 16 + 9 split of sh_degree 4 (d_sh = 25)")
        for n in ("initial", "final", "warm_up"):
            float(_attr(opacity_mapping, n))
        self.cfg, self.opacity_mapping, self.split_harmonics = adapter_cfg, opacity_mapping, bool(split_harmonics)

    @property
    def d_sh(self) -> int:
        return (self.cfg.sh_degree + 1) ** 2

    @property
    def d_in(self) -> int:
        return 7 + 3 * self.d_sh

    def forward(self, pts3d: Sequence[Tensor], raw: Sequence[Tensor], global_step: int = 0, eps: float = 1e-8,
                with_covariances: bool = False) -> Gaussians:
        return gaussians_from_heads(pts3d, raw, opacity_exponent(global_step, self.opacity_mapping),
                                    sh_degree=self.cfg.sh_degree, eps=eps, split_harmonics=self.split_harmonics,
                                    with_covariances=with_covariances)
