"""Evaluation metrics on the HIP library: host mirror of the reference's ``compute_psnr``, ``compute_ssim`` and
``compute_lpips``.

================  ========================================================================================
here              reference (/root/reference/src/evaluation/metrics.py)
================  ========================================================================================
``compute_psnr``  metrics.py:11-19: ``-10 log10(mean((clip(gt) - clip(pred))^2))`` per image
``compute_ssim``  metrics.py:36-52: scikit-image's ``structural_similarity(win_size=11, gaussian_weights=True,
                  channel_axis=0, data_range=1.0)`` per image, mean over the channels
``compute_lpips`` metrics.py:22-33: ``LPIPS(net="vgg").forward(ground_truth, predicted, normalize=True)[:, 0, 0, 0]``
================  ========================================================================================

The reference copies every image to the host and filters it with scikit-image on one CPU core.  Here both metrics stay on
the device: no host copy, no synchronisation, results in ``predicted.dtype`` on ``predicted.device``.  skimage's
Gaussian-weighted SSIM crops 5 pixels from every border after a reflect-padded filter of radius 5, so what it averages
is the valid convolution of the SSIM kernels (spfsplatv2_amd/csrc/ssim.hip) with a window of 11, sigma 1.5, and its
sample covariance is the factor cov_norm = 121/120.  ``compute_lpips`` runs spfsplatv2_amd/lpips.py (pinned to a
restatement of the published method, tests/lpips_oracle.py, not to the ``lpips`` package itself); its VGG weights come from
the caller: ``weights=`` or ``$SPF_LPIPS_WEIGHTS`` (lpips.py says how to make the file).  Nothing is ever downloaded.
"""
from __future__ import annotations

import torch
from torch import Tensor

from . import _lib
from .ssim import _check_images, _window_weights, ssim_forward

_SSIM_WIN, _SSIM_SIGMA, _SSIM_K1, _SSIM_K2 = 11, 1.5, 0.01, 0.03
_SSIM_COV_NORM = 121.0 / 120.0       # skimage: use_sample_covariance=True, NP = win_size ** 2


def _check_pair(name: str, ground_truth: Tensor, predicted: Tensor) -> None:
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"{name}: ground_truth {tuple(ground_truth.shape)} and predicted {tuple(predicted.shape)} "
                         "differ in shape")
    if predicted.dim() != 4:
        raise ValueError(f"{name}: images must be [batch, channel, height, width], got {tuple(predicted.shape)}")


def _operand(t: Tensor) -> Tensor:
    return t.detach().to(torch.float32).contiguous()


@torch.no_grad()
def compute_ssim(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """[batch, channel, height, width] x 2 -> [batch]: the image's mean SSIM over its channels (data range 1)."""
    _check_pair("compute_ssim", ground_truth, predicted)
    _check_images("compute_ssim", ground_truth, predicted, _SSIM_WIN)
    win = _window_weights(None, _SSIM_WIN, _SSIM_SIGMA)
    out, _ = ssim_forward(_operand(ground_truth), _operand(predicted), win, _SSIM_K1 ** 2, _SSIM_K2 ** 2,
                          _SSIM_COV_NORM, False, False)
    return out.to(predicted.dtype)


@torch.no_grad()
def compute_psnr(ground_truth: Tensor, predicted: Tensor) -> Tensor:
    """[batch, channel, height, width] x 2 -> [batch]: PSNR in dB of the images clipped to [0, 1]; +inf when equal."""
    _check_pair("compute_psnr", ground_truth, predicted)
    _check_images("compute_psnr", ground_truth, predicted, 1)
    gt, pred = _operand(ground_truth), _operand(predicted)
    out = torch.empty(pred.shape[0], dtype=torch.float32, device=pred.device)
    _lib.launch("spf_psnr_forward", pred.device, gt, pred, pred.shape[0], pred[0].numel(), out)
    return out.to(predicted.dtype)


@torch.no_grad()
def compute_lpips(ground_truth: Tensor, predicted: Tensor, weights=None) -> Tensor:
    """[batch, 3, height, width] x 2 in [0, 1] -> [batch]: LPIPS(net="vgg") of every pair, ground truth first."""
    from .lpips import _check_pair as check_lpips_pair, lpips
    _check_pair("compute_lpips", ground_truth, predicted)
    check_lpips_pair("compute_lpips", ground_truth, predicted)
    value = lpips(ground_truth.detach(), predicted.detach(), weights, normalize=True)
    return value[:, 0, 0, 0].to(predicted.dtype)
