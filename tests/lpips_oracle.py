"""LPIPS (lpips 0.1, net="vgg", lpips=True, spatial=False, evaluation mode) restated in plain torch ops: the oracle of
tests/test_lpips.py and tests/test_gpu_lpips.py (not collected itself).  Written from the published method, NOT checked
against the ``lpips`` package (it is not installed where this was written).

For in0, in1 [N,3,H,W]: ``x <- 2x - 1`` with normalize; ``x <- (x - shift) / scale``; VGG16 features (zero padding 1 AFTER
the scaling step, bias, ReLU, 2x2 max pools in front of blocks 2..5); taps relu1_2 .. relu5_3; per tap and pixel
``u = a / (||a|| + 1e-10)``, ``v`` alike, ``d = sum_c lin_c (u_c - v_c)^2``; the result is the sum over the taps of the mean
of d, ``[N,1,1,1]``.  Zero-norm rule: where a feature vector is all zero its norm is taken as the CONSTANT 0, so the
``1 / ||a||`` term of the gradient is 0 there (the package's autograd gives NaN: ``0 * inf`` through the square root).
"""
import math

import torch
import torch.nn.functional as F

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
SLICE = (1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5)
CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
TAPS = (1, 3, 6, 9, 12)            # layers (0-based) whose ReLU output is compared
TAP_C = (64, 128, 256, 512, 512)
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)


def make_weights(seed: int, scaling: bool = True) -> dict:
    """Seeded weights as a state dict under the lpips package's key names: He-normal convolutions
    (std = sqrt(2 / (9 C_in))), biases 0.05 x normal, lin uniform in [0, 2 / C)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, s, ci, co in zip(CONV_INDEX, SLICE, CIN, COUT):
        sd[f"net.slice{s}.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * math.sqrt(2.0 / (9 * ci))
        sd[f"net.slice{s}.{i}.bias"] = 0.05 * torch.randn(co, generator=g)
    for k, c in enumerate(TAP_C):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) * (2.0 / c)
    if scaling:
        sd["scaling_layer.shift"] = torch.tensor(SHIFT).reshape(1, 3, 1, 1)
        sd["scaling_layer.scale"] = torch.tensor(SCALE).reshape(1, 3, 1, 1)
    return sd


def params(sd: dict, dtype):
    """(convolutions [(w, b)], lin vectors [1,C,1,1], shift, scale) of a make_weights() dict in `dtype`."""
    convs = [(sd[f"net.slice{s}.{i}.weight"].to(dtype), sd[f"net.slice{s}.{i}.bias"].to(dtype))
             for i, s in zip(CONV_INDEX, SLICE)]
    lins = [sd[f"lin{k}.model.1.weight"].to(dtype) for k in range(5)]
    shift = sd.get("scaling_layer.shift", torch.tensor(SHIFT).reshape(1, 3, 1, 1)).to(dtype)
    scale = sd.get("scaling_layer.scale", torch.tensor(SCALE).reshape(1, 3, 1, 1)).to(dtype)
    return convs, lins, shift, scale


def scaled(x, shift, scale, normalize: bool):
    if normalize:
        x = 2 * x - 1
    return (x - shift) / scale


def conv(x, w, b=None, relu: bool = True):
    y = F.conv2d(x, w, b, padding=1)
    return F.relu(y) if relu else y


def pool(x):
    """2x2 stride-2 max pool, floor mode, the FIRST maximum of a window in row-major order taking the gradient (what
    F.max_pool2d does on exact ties).  In float64 entries within 1e-12 of the window's maximum count as tied: a constant
    image makes every window of its interior an exact tie, and a host float64 convolution whose blocking depends on the
    pixel's position returns those equal sums one ulp apart, which would leave the choice (and with it 10 % of the
    gradient, seen on one host) to rounding noise.  float32: exact comparison."""
    h, w = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * h, :2 * w]
    c = [x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]]
    with torch.no_grad():
        m = torch.maximum(torch.maximum(c[0], c[1]), torch.maximum(c[2], c[3]))
        floor = m - (1e-12 if x.dtype == torch.float64 else 0.0) * m.abs()
    out = c[3]
    for j in (2, 1, 0):
        out = torch.where(c[j] >= floor, c[j], out)
    return out


def features(x, convs, shift, scale, normalize: bool) -> list:
    """The five taps of the (already float-typed) image batch x."""
    h = scaled(x, shift, scale, normalize)
    taps = []
    for l, (w, b) in enumerate(convs):
        if l in (2, 4, 7, 10):
            h = pool(h)
        h = conv(h, w, b)
        if l in TAPS:
            taps.append(h)
    return taps


def unit(a):
    """a / (||a|| + 1e-10) over the channels, with the zero-norm rule."""
    sq = (a * a).sum(1, keepdim=True)
    zero = sq == 0
    n = torch.where(zero, torch.zeros_like(sq), torch.sqrt(torch.where(zero, torch.ones_like(sq), sq)))
    return a / (n + 1e-10)


def head_term(a, b, lin):
    """One tap's term [N]: the mean over the pixels of sum_c lin_c (u_c - v_c)^2."""
    d = (lin * (unit(a) - unit(b)) ** 2).sum(1)
    return d.mean((1, 2))


def lpips(in0, in1, sd: dict, normalize: bool = False, dtype=torch.float64):
    """[N,1,1,1] in `dtype`; differentiable in in0 and in1."""
    convs, lins, shift, scale = params(sd, dtype)
    f0 = features(in0.to(dtype), convs, shift, scale, normalize)
    f1 = features(in1.to(dtype), convs, shift, scale, normalize)
    total = sum(head_term(a, b, lin) for a, b, lin in zip(f0, f1, lins))
    return total.reshape(-1, 1, 1, 1)


def lpips_with_grads(in0, in1, sd, normalize, dtype, upstream=None):
    """(value [N], dL/din0, dL/din1) for L = sum_n upstream[n] * value[n] (upstream None: ones)."""
    a = in0.detach().clone().to(dtype).requires_grad_(True)
    b = in1.detach().clone().to(dtype).requires_grad_(True)
    v = lpips(a, b, sd, normalize, dtype).reshape(-1)
    up = torch.ones_like(v) if upstream is None else upstream.to(dtype)
    ga, gb = torch.autograd.grad(v, [a, b], up)
    return v.detach(), ga, gb


def image_pair(seed: int, shape, noise: float = 0.1):
    """(prediction, target) in [0, 1], float32: prediction = target + noise, clamped."""
    g = torch.Generator().manual_seed(seed)
    target = torch.rand(shape, generator=g)
    pred = (target + noise * torch.randn(shape, generator=g)).clamp(0, 1)
    return pred, target
