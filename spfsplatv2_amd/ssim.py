"""SSIM on the HIP library: host mirror of the reference's differentiable ``ssim`` / ``SSIM``.

==========  =============================================================================================
here        reference (/root/reference/src/loss/loss_ssim.py)
==========  =============================================================================================
``ssim``    loss_ssim.py:129-189 (with ``_ssim``, 58-126, and ``_fspecial_gauss_1d``, 12-26): same argument names
            (``retrun_seprate`` is the reference's spelling), same 4-tuple; differentiable in ``X`` and ``Y``
``SSIM``    loss_ssim.py:274-314: the module; ``forward(X, Y)`` returns what ``ssim`` returns
==========  =============================================================================================

The reference filters the five moment maps with ten grouped convolutions and combines them with ~twenty elementwise
kernels, and autograd runs as many again backward.  Here the forward is one fused pass (tile + halo in LDS, both filter
passes out of LDS) and two small fixed-order reductions, and the backward one pass that recomputes the moments from
``X, Y``; sums are taken in a fixed order (bit-reproducible), the upstream gradient is read on the device (no sync).

Deliberate differences (each a clear error): CPU tensors (no CPU fallback); 5-D inputs (the reference switches to a 3-D
window); an image side shorter than the window (the reference warns and skips that axis); a ``win`` whose rows differ;
windows longer than 33; ``retrun_seprate=True``.  ``ms_ssim`` / ``MS_SSIM`` are not provided.
"""
from __future__ import annotations

import ctypes as C
from functools import lru_cache
from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from . import _lib


@lru_cache(maxsize=32)
def gauss_window(size: int, sigma: float) -> Tensor:
    """The 1-D Gaussian window [size], built in float32 step by step as the reference's ``_fspecial_gauss_1d`` builds it
    (integer offsets from the centre, exp, division by the float32 sum), so that the weights are the same bits."""
    offs = torch.arange(size, dtype=torch.float32) - (size // 2)
    g = torch.exp(-(offs ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _window_weights(win: Optional[Tensor], win_size: int, win_sigma: float) -> tuple:
    """The window as a tuple of Python floats (float32 values).  `win` given: its last dimension is the window, every
    row (the reference repeats one row per channel) must be the same."""
    if win is None:
        if win_size % 2 != 1:
            raise ValueError("Window size should be odd.")
        if win_size > _lib.SSIM_MAX_WIN or win_size < 3:
            raise ValueError(f"ssim: window size {win_size} outside 3..{_lib.SSIM_MAX_WIN}")
        return tuple(gauss_window(int(win_size), float(win_sigma)).tolist())
    if win.shape[-1] % 2 != 1:
        raise ValueError("Window size should be odd.")
    if win.shape[-1] > _lib.SSIM_MAX_WIN or win.shape[-1] < 3:
        raise ValueError(f"ssim: window size {win.shape[-1]} outside 3..{_lib.SSIM_MAX_WIN}")
    rows = win.detach().to("cpu", torch.float32).reshape(-1, win.shape[-1])
    if not bool((rows == rows[:1]).all()):
        raise ValueError("ssim: `win` has different rows per channel; this build filters every channel with one window")
    return tuple(rows[0].tolist())


def _check_images(name: str, X: Tensor, Y: Tensor, ws: int) -> None:
    """What both `ssim` and the metrics ask of two [N,C,H,W] images; raised before anything touches a device."""
    if min(X.shape[-2:]) < ws:
        raise ValueError(f"{name}: image side {min(X.shape[-2:])} is shorter than the window ({ws}); the reference "
                         "skips the filter along that axis, this build does not")
    for what, t in (("X", X), ("Y", Y)):
        if not t.is_floating_point():
            raise RuntimeError(f"{name}: {what} must be a floating-point tensor, got {t.dtype}")
    if X.numel() == 0:
        raise RuntimeError(f"{name}: empty input")
    for what, t in (("X", X), ("Y", Y)):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {what} is on {t.device}; this build only runs on a HIP device (no CPU "
                               "fallback)")


def _args(X: Tensor, Y: Tensor, win: Sequence[float], C1: float, C2: float, cov_norm: float, size_average: bool,
          nonnegative: bool) -> _lib.SpfSsim:
    n, c, h, w = X.shape
    arr = (C.c_float * _lib.SSIM_MAX_WIN)(*win)
    return _lib.SpfSsim(_lib.ptr(X), _lib.ptr(Y), n, c, h, w, len(win), C1, C2, cov_norm,
                        int(bool(size_average)), int(bool(nonnegative)), arr)


def ssim_forward(X: Tensor, Y: Tensor, win: Sequence[float], C1: float, C2: float, cov_norm: float,
                 size_average: bool, nonnegative: bool):
    """The three forward launches on float32 contiguous [N,C,H,W] device tensors -> (out, plane_mean [N,C])."""
    lib = _lib.load()
    dev = X.device
    n, c, h, w = X.shape
    nslots = lib.spf_ssim_partial_blocks(n, c, h, w, len(win))
    if nslots < 0:
        raise RuntimeError(f"ssim: unsupported sizes {tuple(X.shape)} with a window of {len(win)}")
    partial = torch.empty(nslots, dtype=torch.float32, device=dev)
    plane_mean = torch.empty((n, c), dtype=torch.float32, device=dev)
    out = torch.empty(() if size_average else (n,), dtype=torch.float32, device=dev)
    args = _args(X, Y, win, C1, C2, cov_norm, size_average, nonnegative)
    _lib.launch("spf_ssim_forward", dev, args, partial, plane_mean, out)
    return out, plane_mean


class _Ssim(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X: Tensor, Y: Tensor, win: tuple, C1: float, C2: float, cov_norm: float, size_average: bool,
                nonnegative: bool):
        x, y = X.contiguous(), Y.contiguous()
        out, plane_mean = ssim_forward(x, y, win, C1, C2, cov_norm, size_average, nonnegative)
        ctx.save_for_backward(x, y, plane_mean)
        ctx.params = (win, C1, C2, cov_norm, size_average, nonnegative)
        return out

    @staticmethod
    def backward(ctx, grad):
        x, y, plane_mean = ctx.saved_tensors
        win, C1, C2, cov_norm, size_average, nonnegative = ctx.params
        need_x, need_y = ctx.needs_input_grad[:2]
        g = grad.to(torch.float32).contiguous()
        dx = torch.empty_like(x) if need_x else None
        dy = torch.empty_like(y) if need_y else None
        _lib.launch("spf_ssim_backward", x.device, _args(x, y, win, C1, C2, cov_norm, size_average, nonnegative),
                    plane_mean, g, dx, dy)
        return dx, dy, None, None, None, None, None, None


def ssim(X: Tensor, Y: Tensor, data_range: float = 255, size_average: bool = True, win_size: int = 11,
         win_sigma: float = 1.5, win: Optional[Tensor] = None, K: Sequence[float] = (0.01, 0.03),
         nonnegative_ssim: bool = False, retrun_seprate: bool = False):
    """``ssim`` of the reference (loss_ssim.py:129-189) for [N,C,H,W] images on a HIP device: the mean SSIM (0-dim with
    ``size_average``, else one value per image) and three zeros of the same shape (the reference's brightness, contrast
    and structure entries without ``retrun_seprate``).  Any floating dtype and any strides; computed in float32, float32
    results, gradients cast back by autograd."""
    if not X.shape == Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {X.shape} and {Y.shape}.")
    for d in range(X.dim() - 1, 1, -1):                      # trailing singleton dimensions go
        X, Y = X.squeeze(dim=d), Y.squeeze(dim=d)
    if X.dim() == 5:
        raise NotImplementedError("ssim: 5-d inputs (a 3-d window in the reference) are not supported by this build")
    if X.dim() != 4:
        raise ValueError(f"Input images should be 4-d or 5-d tensors, but got {X.shape}")
    weights = _window_weights(win, win_size, win_sigma)
    if retrun_seprate:
        raise NotImplementedError("ssim: retrun_seprate=True (brightness / contrast / structure) is not supported by "
                                  "this build")
    _check_images("ssim", X, Y, len(weights))
    K1, K2 = K
    C1, C2 = float((K1 * data_range) ** 2), float((K2 * data_range) ** 2)
    if X.dtype != torch.float32:
        X = X.float()
    if Y.dtype != torch.float32:
        Y = Y.float()
    value = _Ssim.apply(X, Y, weights, C1, C2, 1.0, bool(size_average), bool(nonnegative_ssim))
    zeros = torch.zeros_like(value)
    return value, zeros, zeros, zeros


class SSIM(nn.Module):
    """The reference's module (loss_ssim.py:274-314): the window is built once, ``forward`` calls ``ssim`` with it."""

    def __init__(self, data_range: float = 255, size_average: bool = True, win_size: int = 11, win_sigma: float = 1.5,
                 channel: int = 3, spatial_dims: int = 2, K: Sequence[float] = (0.01, 0.03),
                 nonnegative_ssim: bool = False) -> None:
        super().__init__()
        if spatial_dims != 2:
            raise NotImplementedError("SSIM: only spatial_dims=2 is supported by this build")
        if win_size % 2 != 1:
            raise ValueError("Window size should be odd.")
        self.win_size = win_size
        self.win = gauss_window(int(win_size), float(win_sigma)).reshape(1, 1, 1, -1).repeat(channel, 1, 1, 1)
        self.size_average = size_average
        self.data_range = data_range
        self.K = K
        self.nonnegative_ssim = nonnegative_ssim

    def forward(self, X: Tensor, Y: Tensor):
        return ssim(X, Y, data_range=self.data_range, size_average=self.size_average, win=self.win, K=self.K,
                    nonnegative_ssim=self.nonnegative_ssim)
