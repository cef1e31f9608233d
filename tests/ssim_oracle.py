"""Oracles for SSIM and PSNR (tests/test_ssim.py, tests/test_gpu_ssim.py, tools/ssim_time.py).

* ``ssim_oracle``: a torch restatement of the reference's ``ssim`` + ``_ssim`` (src/loss/loss_ssim.py:58-189) with a
  ``cov_norm`` argument, in the dtype the caller asks for: float64 is the truth, float32 is the yardstick (what the
  reference's own eager expression loses in float32).  The window is built in float32 and then cast, as the reference
  builds it (``window_dtype=torch.float64`` builds it in float64 instead, for the comparison with scipy).
* ``skimage_ssim``: a second, independent restatement of what ``compute_ssim`` calls, scikit-image's Gaussian-weighted
  ``structural_similarity``: scipy's reflect-padded Gaussian filter (sigma 1.5, truncate 3.5), sample covariance
  (121/120), 5 pixels cropped from every border, mean per channel, then over the channels.
* ``psnr_oracle``: ``compute_psnr`` (src/evaluation/metrics.py:11-19).
* the three seeded input kinds of the GPU tests (``noise``, ``smooth``, ``piecewise``) and the error measures.
"""
import torch
import torch.nn.functional as F

SKIMAGE_COV_NORM = 121.0 / 120.0


def gauss_window(size, sigma, dtype=torch.float32):
    offs = torch.arange(size, dtype=dtype) - (size // 2)
    g = torch.exp(-(offs ** 2) / (2 * sigma ** 2))
    return g / g.sum()


def _filter(t, win):
    """Valid separable filter of [N,C,H,W] with the 1-D window `win`, along H and then along W."""
    c = t.shape[1]
    k = win.reshape(1, 1, -1).repeat(c, 1, 1)
    t = F.conv2d(t, k.unsqueeze(-1), groups=c)
    return F.conv2d(t, k.unsqueeze(-2), groups=c)


def ssim_planes(X, Y, win, C1, C2, cov_norm=1.0):
    """[N,C]: every plane's mean SSIM over the valid region."""
    mx, my = _filter(X, win), _filter(Y, win)
    mxx, myy, mxy = mx * mx, my * my, mx * my
    sx = cov_norm * (_filter(X * X, win) - mxx)
    sy = cov_norm * (_filter(Y * Y, win) - myy)
    sxy = cov_norm * (_filter(X * Y, win) - mxy)
    cs = (2 * sxy + C2) / (sx + sy + C2)
    s = ((2 * mxy + C1) / (mxx + myy + C1)) * cs
    return s.flatten(2).mean(-1)


def ssim_oracle(X, Y, data_range=255, size_average=True, win_size=11, win_sigma=1.5, win=None, K=(0.01, 0.03),
                nonnegative_ssim=False, cov_norm=1.0, dtype=torch.float64, window_dtype=torch.float32):
    """The first entry of the reference's ``ssim`` tuple, evaluated in `dtype` on X's device; differentiable in X, Y
    (pass tensors of `dtype` that require grad, or anything else for the value alone)."""
    X, Y = X.to(dtype), Y.to(dtype)
    w = gauss_window(win_size, win_sigma, window_dtype) if win is None else win.reshape(-1, win.shape[-1])[0]
    w = w.to(device=X.device, dtype=dtype)
    C1, C2 = (K[0] * data_range) ** 2, (K[1] * data_range) ** 2
    p = ssim_planes(X, Y, w, C1, C2, cov_norm)
    if nonnegative_ssim:
        p = torch.relu(p)
    return p.mean() if size_average else p.mean(1)


def compute_ssim_oracle(ground_truth, predicted, dtype=torch.float64, window_dtype=torch.float32):
    """``compute_ssim`` as the valid convolution with skimage's sample-covariance factor -> [batch]."""
    return ssim_oracle(ground_truth, predicted, data_range=1.0, size_average=False, cov_norm=SKIMAGE_COV_NORM,
                       dtype=dtype, window_dtype=window_dtype)


def skimage_ssim(ground_truth, predicted):
    """scikit-image's definition with scipy's filter, float64 -> [batch] (CPU tensors)."""
    import numpy as np
    from scipy.ndimage import gaussian_filter
    C1, C2, pad = 0.01 ** 2, 0.03 ** 2, 5

    def filt(a):
        return gaussian_filter(a, sigma=1.5, truncate=3.5, mode="reflect")
    out = []
    for gt, hat in zip(ground_truth.double().numpy(), predicted.double().numpy()):
        per_channel = []
        for x, y in zip(gt, hat):
            ux, uy = filt(x), filt(y)
            vx = SKIMAGE_COV_NORM * (filt(x * x) - ux * ux)
            vy = SKIMAGE_COV_NORM * (filt(y * y) - uy * uy)
            vxy = SKIMAGE_COV_NORM * (filt(x * y) - ux * uy)
            s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
            per_channel.append(s[pad:-pad, pad:-pad].mean(dtype=np.float64))
        out.append(float(np.mean(per_channel)))
    return torch.tensor(out, dtype=torch.float64)


def psnr_oracle(ground_truth, predicted, dtype=torch.float64):
    gt, hat = ground_truth.to(dtype).clip(0, 1), predicted.to(dtype).clip(0, 1)
    return -10 * ((gt - hat) ** 2).flatten(1).mean(1).log10()


# ---- inputs (float32 values, seeded) ---------------------------------------------------------------------------------
def noise(seed, shape):
    """X, Y ~ U(0, 1), independent: SSIM ~ 0.005."""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(shape, generator=g), torch.rand(shape, generator=g)


def smooth(seed, shape):
    """Y: a U(0, 1) grid of (H/8 + 2) x (W/8 + 2) upsampled bicubically and clamped; X = clamp(Y + 0.05 N(0, 1)):
    SSIM ~ 0.86, what a decent render scores."""
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    grid = torch.rand((n, c, h // 8 + 2, w // 8 + 2), generator=g)
    Y = F.interpolate(grid, size=(h, w), mode="bicubic", align_corners=False).clamp(0, 1)
    X = (Y + 0.05 * torch.randn(shape, generator=g)).clamp(0, 1)
    return X.contiguous(), Y.contiguous()


def piecewise(seed, shape):
    """Y: 0 in the top half, 0.7 in the bottom half; X = Y with 0.01 added in the right half: SSIM ~ 0.88, and
    E[x^2] - mu^2 cancels to rounding almost everywhere.  (Nothing random: `seed` is ignored.)"""
    n, c, h, w = shape
    Y = torch.zeros(shape)
    Y[:, :, h // 2:, :] = 0.7
    X = Y.clone()
    X[:, :, :, w // 2:] += 0.01
    return X, Y


KINDS = {"noise": noise, "smooth": smooth, "piecewise": piecewise}


# ---- error measures --------------------------------------------------------------------------------------------------
def grad_errors(got, want):
    """(per plane, per element) for gradients [N,C,H,W] against the truth `want`:
    per plane: the worst max|g - w| / max|w| over the planes; per element: the worst |g - w| / |w| over the entries
    within two orders of their plane's largest.  A plane whose truth is all zero (behind a relu) must be all zero:
    0 if it is, inf otherwise."""
    g, w = got.detach().double().cpu().flatten(2), want.detach().double().cpu().flatten(2)
    big = w.abs().amax(-1, keepdim=True)
    diff = (g - w).abs()
    dead = big == 0
    plane = torch.where(dead, torch.where(diff.amax(-1, keepdim=True) == 0, 0.0, float("inf")),
                        diff.amax(-1, keepdim=True) / big.clamp_min(1e-300))
    keep = (w.abs() >= 1e-2 * big) & ~dead
    ratio = torch.where(keep, diff / w.abs().clamp_min(1e-300), 0.0)
    return float(plane.max()), float(ratio.max())


def value_error(got, want):
    return float((got.detach().double().cpu() - want.detach().double().cpu()).abs().max())
