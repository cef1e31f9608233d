"""LPIPS (VGG16) on the HIP library: host mirror of what the reference calls from the ``lpips`` package.

==================  ===================================================================================
here                reference
==================  ===================================================================================
``LPIPS``           ``lpips.LPIPS(net="vgg")`` as src/loss/loss_lpips.py:63 and src/evaluation/metrics.py:22-33 build it;
                    ``forward(in0, in1, retPerLayer=False, normalize=False)`` -> ``[N,1,1,1]``
``lpips``           the same as a function
``LpipsWeights``    the frozen VGG16 convolutions, the five 1x1 ``lin`` layers and the scaling layer, packed once
==================  ===================================================================================

Pinned to a RESTATEMENT of the published method (lpips 0.1, ``net="vgg"``, ``lpips=True``, ``spatial=False``, evaluation
mode), tests/lpips_oracle.py: neither ``lpips`` nor ``torchvision`` is imported here, and nothing is ever fetched.  The
weights come from the caller: ``weights=`` (an ``LpipsWeights``, a state dict, a pair of state dicts, or a path that
``torch.load`` reads) or the environment variable ``SPF_LPIPS_WEIGHTS`` (a path); ``LpipsWeights.from_module(m)`` reads
``m.state_dict()`` of an ``lpips.LPIPS`` the caller already holds.

The reference runs thirteen vendor convolutions per image and ~forty elementwise kernels for the head, and autograd as
many again.  Here the trunk is this library's implicit-GEMM convolution on the float32 matrix instructions
(spfsplatv2_amd/csrc/lpips.hip), in0 and in1 as one batch; only images that need a gradient run the backward trunk; sums
are taken in a fixed order (bit-reproducible, an image's value does not depend on its batch); nothing synchronises.

Deliberate differences: where a feature vector is all zero the reference's autograd gives NaN (``0 * inf`` through the
square root), here the ``1 / ||a||`` term of the gradient is 0; CPU tensors, ``net`` other than ``"vgg"``,
``retPerLayer=True``, ``spatial=True`` and images with a side shorter than 16 are errors.

The building blocks of the chain (``conv3x3_forward``, ``conv3x3_backward_data``, ``maxpool_forward``,
``maxpool_backward``, ``head_forward``, ``head_backward``) are callable on plain ``[N,C,H,W]`` float32 tensors; they are
the very kernels the whole-chain calls launch (the layout copy around them is test-path plumbing).
"""
from __future__ import annotations

import os
import re
from pathlib import Path
from typing import Optional, Sequence

import torch
from torch import Tensor, nn

from . import _lib

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)       # positions in torchvision's vgg16().features
CONV_CIN = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512)
CONV_COUT = (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512)
CONV_LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)                 # pools in front of the layer
TAP_LAYER = (1, 3, 6, 9, 12)                                         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
TAP_C = (64, 128, 256, 512, 512)
DEFAULT_SHIFT = (-.030, -.088, -.188)
DEFAULT_SCALE = (.458, .448, .450)
MIN_SIDE = 16
ONE_LINER = 'torch.save(lpips.LPIPS(net="vgg").state_dict(), "lpips_vgg.pt")'

_CONV_KEY = re.compile(r"(?:^|\.)(\d+)\.(weight|bias)$")
_LIN_KEY = re.compile(r"(?:^|\.)lin(?:s\.)?(\d)\.model\.1\.weight$")
_SCALING_KEY = re.compile(r"(?:^|\.)scaling_layer\.(shift|scale)$")


def _pack_offsets() -> tuple:
    off, o = [], 0
    for ci, co in zip(CONV_CIN, CONV_COUT):
        off.append(o)
        o += 9 * ci * co
    return tuple(off), o


PACK_OFFSET, PACK_SIZE = _pack_offsets()


def _wanted_keys() -> list:
    return ([f"<prefix>.{i}.weight [{co},{ci},3,3]" for i, ci, co in zip(CONV_INDEX, CONV_CIN, CONV_COUT)]
            + [f"<prefix>.{i}.bias [{co}]" for i, co in zip(CONV_INDEX, CONV_COUT)]
            + [f"lin{k}.model.1.weight or lins.{k}.model.1.weight [1,{c},1,1]" for k, c in enumerate(TAP_C)]
            + ["scaling_layer.shift, scaling_layer.scale [1,3,1,1] (optional)"])


class LpipsWeights:
    """The frozen weights of LPIPS(net="vgg"), checked and packed once; device copies are cached per device.

    ``conv_w[l]`` [C_out,C_in,3,3], ``conv_b[l]`` [C_out], ``lin[k]`` [C_k], ``shift``, ``scale`` [3]: float32 on the
    host.  ``forward_pack`` / ``backward_pack`` are what the kernels read (include/spfsplat_hip.h, SpfLpips)."""

    def __init__(self, conv_w: Sequence[Tensor], conv_b: Sequence[Tensor], lin: Sequence[Tensor],
                 shift: Optional[Tensor] = None, scale: Optional[Tensor] = None) -> None:
        def host(t):
            return t.detach().to("cpu", torch.float32).contiguous()
        self.conv_w = [host(t) for t in conv_w]
        self.conv_b = [host(t) for t in conv_b]
        self.lin = [host(t).reshape(-1) for t in lin]
        self.shift = host(torch.tensor(DEFAULT_SHIFT) if shift is None else shift).reshape(-1)
        self.scale = host(torch.tensor(DEFAULT_SCALE) if scale is None else scale).reshape(-1)
        if len(self.conv_w) != 13 or len(self.conv_b) != 13 or len(self.lin) != 5:
            raise ValueError("LpipsWeights: 13 convolutions, 13 biases and 5 lin vectors are needed")
        for l, (w, b) in enumerate(zip(self.conv_w, self.conv_b)):
            if tuple(w.shape) != (CONV_COUT[l], CONV_CIN[l], 3, 3) or tuple(b.shape) != (CONV_COUT[l],):
                raise ValueError(f"LpipsWeights: convolution {l} has shapes {tuple(w.shape)}, {tuple(b.shape)}")
        for k, v in enumerate(self.lin):
            if v.numel() != TAP_C[k]:
                raise ValueError(f"LpipsWeights: lin{k} has {v.numel()} entries, {TAP_C[k]} wanted")
        if self.shift.numel() != 3 or self.scale.numel() != 3:
            raise ValueError("LpipsWeights: shift and scale have three entries")
        self._device: dict = {}

    # ---- sources ---------------------------------------------------------------------------------------------------
    @classmethod
    def from_state_dict(cls, state: dict, lin: Optional[dict] = None) -> "LpipsWeights":
        """From an ``lpips.LPIPS(net="vgg")`` state dict, or a torchvision ``vgg16`` (or ``vgg16().features``) state dict
        plus the dict of the ``lin`` layers.  Convolutions are matched by their trailing index under any prefix."""
        items = dict(state)
        if lin is not None:
            items.update({f"__lin__.{k}": v for k, v in lin.items()})
        found: dict = {}

        def put(slot, key, t):
            if slot in found and not (found[slot][1].shape == t.shape and torch.equal(found[slot][1].cpu(), t.cpu())):
                raise cls._key_error(items, f"{found[slot][0]!r} and {key!r} both name {slot} and differ")
            found.setdefault(slot, (key, t))
        for key, t in items.items():
            if not isinstance(t, Tensor):
                continue
            m = _LIN_KEY.search(key)
            if m and int(m.group(1)) < 5:
                put(("lin", int(m.group(1))), key, t)
                continue
            m = _SCALING_KEY.search(key)
            if m:
                put((m.group(1),), key, t)
                continue
            m = _CONV_KEY.search(key)
            if m and int(m.group(1)) in CONV_INDEX and "classifier" not in key:
                if (m.group(2) == "weight") == (t.dim() == 4):
                    put((m.group(2), CONV_INDEX.index(int(m.group(1)))), key, t)
        problems = []
        for l in range(13):
            for what, shape in (("weight", (CONV_COUT[l], CONV_CIN[l], 3, 3)), ("bias", (CONV_COUT[l],))):
                got = found.get((what, l))
                if got is None:
                    problems.append(f"missing <prefix>.{CONV_INDEX[l]}.{what}")
                elif tuple(got[1].shape) != shape:
                    problems.append(f"{got[0]} has shape {tuple(got[1].shape)}, wanted {shape}")
        for k in range(5):
            got = found.get(("lin", k))
            if got is None:
                problems.append(f"missing lin{k}.model.1.weight")
            elif tuple(got[1].shape) != (1, TAP_C[k], 1, 1):
                problems.append(f"{got[0]} has shape {tuple(got[1].shape)}, wanted {(1, TAP_C[k], 1, 1)}")
        for what in ("shift", "scale"):
            got = found.get((what,))
            if got is not None and got[1].numel() != 3:
                problems.append(f"{got[0]} has shape {tuple(got[1].shape)}, wanted (1, 3, 1, 1)")
        if problems:
            raise cls._key_error(items, "; ".join(problems))
        shift, scale = found.get(("shift",)), found.get(("scale",))
        return cls([found[("weight", l)][1] for l in range(13)], [found[("bias", l)][1] for l in range(13)],
                   [found[("lin", k)][1] for k in range(5)], None if shift is None else shift[1],
                   None if scale is None else scale[1])

    @staticmethod
    def _key_error(items: dict, what: str) -> KeyError:
        return KeyError(f"LPIPS weights: {what}.\nkeys found: {sorted(str(k).replace('__lin__.', '') for k in items)}\n"
                        f"keys wanted: {_wanted_keys()}")

    @classmethod
    def from_module(cls, module: nn.Module) -> "LpipsWeights":
        """From an ``lpips.LPIPS(net="vgg")`` instance the caller holds: reads ``module.state_dict()``, nothing else."""
        return cls.from_state_dict(module.state_dict())

    @classmethod
    def from_file(cls, path) -> "LpipsWeights":
        state = torch.load(str(path), map_location="cpu", weights_only=True)
        if isinstance(state, (tuple, list)):
            return cls.from_state_dict(*state)
        return cls.from_state_dict(state)

    # ---- packs -----------------------------------------------------------------------------------------------------
    def forward_pack(self) -> Tensor:
        """Per layer ``[tap = 3 dy + dx][C_in][C_out]``, layers concatenated."""
        return torch.cat([w.permute(2, 3, 1, 0).reshape(-1) for w in self.conv_w])

    def backward_pack(self) -> Tensor:
        """Per layer ``[tap][C_out][C_in]`` with the taps rotated by 180 degrees: the weights of the convolution that maps
        the gradient of the layer's output to the gradient of its input."""
        return torch.cat([w.flip(2, 3).permute(2, 3, 0, 1).reshape(-1) for w in self.conv_w])

    @staticmethod
    def unpack_forward(pack: Tensor) -> list:
        """The convolution weights ``[C_out,C_in,3,3]`` back from a forward pack."""
        return [pack[o:o + 9 * ci * co].reshape(3, 3, ci, co).permute(3, 2, 0, 1).contiguous()
                for o, ci, co in zip(PACK_OFFSET, CONV_CIN, CONV_COUT)]

    @staticmethod
    def unpack_backward(pack: Tensor) -> list:
        """A backward pack as ordinary convolution weights ``[C_in,C_out,3,3]``: ``conv2d(g, w, padding=1)`` with them is
        the layer's backward-data pass."""
        return [pack[o:o + 9 * ci * co].reshape(3, 3, co, ci).permute(3, 2, 0, 1).contiguous()
                for o, ci, co in zip(PACK_OFFSET, CONV_CIN, CONV_COUT)]

    def on(self, device) -> dict:
        """The packed tensors on `device` (copied once)."""
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"lpips: weights asked for on {dev}; this build only runs on a HIP device (no CPU fallback)")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        d = self._device.get(dev)
        if d is None:
            d = self._device[dev] = {
                "wfwd": self.forward_pack().to(dev), "wbwd": self.backward_pack().to(dev),
                "bias": torch.cat(self.conv_b).to(dev), "lin": torch.cat(self.lin).to(dev),
                "shift_scale": torch.cat([self.shift, self.scale]).to(dev)}
        return d


_BY_PATH: dict = {}


def resolve_weights(weights=None) -> LpipsWeights:
    """`weights` (LpipsWeights, state dict, (vgg state dict, lin dict), path), else $SPF_LPIPS_WEIGHTS; never random."""
    if isinstance(weights, LpipsWeights):
        return weights
    if isinstance(weights, dict):
        return LpipsWeights.from_state_dict(weights)
    if isinstance(weights, (tuple, list)):
        return LpipsWeights.from_state_dict(*weights)
    if weights is None:
        weights = os.environ.get("SPF_LPIPS_WEIGHTS") or None
        if weights is None:
            raise RuntimeError(
                "lpips: no weights.  Pass weights= (an LpipsWeights, a state dict or a path) or set SPF_LPIPS_WEIGHTS to "
                "a file; this library never downloads anything.  On any machine that has the lpips package, this one "
                f"line makes the file: {ONE_LINER}")
    if isinstance(weights, (str, Path)):
        key = str(Path(weights).resolve())
        if key not in _BY_PATH:
            _BY_PATH[key] = LpipsWeights.from_file(weights)
        return _BY_PATH[key]
    raise TypeError(f"lpips: weights of type {type(weights).__name__} are not understood")


# ---- plumbing --------------------------------------------------------------------------------------------------------
def _need_device(name: str, **tensors: Tensor) -> None:
    for what, t in tensors.items():
        if not t.is_floating_point():
            raise RuntimeError(f"{name}: {what} must be a floating-point tensor, got {t.dtype}")
    for what, t in tensors.items():
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {what} is on {t.device}; this build only runs on a HIP device (no CPU "
                               "fallback)")


def _check_pair(name: str, in0: Tensor, in1: Tensor) -> None:
    """What every LPIPS call asks of its two image batches; raised before anything touches a device."""
    if in0.dim() != 4 or in1.dim() != 4:
        raise ValueError(f"{name}: images must be [N,3,H,W], got {tuple(in0.shape)} and {tuple(in1.shape)}")
    if in0.shape != in1.shape:
        raise ValueError(f"{name}: the two inputs differ in shape: {tuple(in0.shape)} and {tuple(in1.shape)}")
    if in0.shape[1] != 3:
        raise ValueError(f"{name}: images must have 3 channels, got {in0.shape[1]}")
    if min(in0.shape[-2:]) < MIN_SIDE:
        raise ValueError(f"{name}: image side {min(in0.shape[-2:])} is shorter than {MIN_SIDE}: the fifth tap would be "
                         "empty")
    if in0.shape[0] == 0:
        raise RuntimeError(f"{name}: empty input")
    _need_device(name, in0=in0, in1=in1)


def _args(x0: Tensor, x1: Optional[Tensor], dw: dict, normalize: bool, weight: float = 1.0) -> _lib.SpfLpips:
    n, _, h, w = x0.shape
    ptr = _lib.ptr
    return _lib.SpfLpips(ptr(x0), ptr(x1), x0.stride(0), x1.stride(0) if x1 is not None else 0, n, h, w,
                         int(bool(normalize)), float(weight), 0, ptr(dw["wfwd"]), ptr(dw["wbwd"]), ptr(dw["bias"]),
                         ptr(dw["lin"]), ptr(dw["shift_scale"]))


def _nhwc(t: Tensor) -> Tensor:
    return t.to(torch.float32).permute(0, 2, 3, 1).contiguous()


def _nchw(t: Tensor) -> Tensor:
    return t.permute(0, 3, 1, 2).contiguous()


def _layer(layer: int) -> int:
    if not 1 <= int(layer) <= 13:
        raise ValueError(f"lpips: layer {layer} outside 1..13")
    return int(layer) - 1


# ---- the whole chain -------------------------------------------------------------------------------------------------
class _Lpips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, in0: Tensor, in1: Tensor, W: LpipsWeights, normalize: bool, mean_weight: Optional[float],
                grad_mode: bool):
        x0, x1 = in0.contiguous(), in1.contiguous()
        dev = x0.device
        n, _, h, w = x0.shape
        need = [bool(grad_mode and ctx.needs_input_grad[i]) for i in (0, 1)]
        nbytes = _lib.load().spf_lpips_workspace_bytes(n * sum(need), 2 * n, h, w)
        if nbytes < 0:
            raise RuntimeError(f"lpips: unsupported sizes {tuple(x0.shape)}")
        dw = W.on(dev)
        ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        mean = torch.empty((), dtype=torch.float32, device=dev) if mean_weight is not None else None
        args = _args(x0, x1, dw, normalize, 1.0 if mean_weight is None else mean_weight)
        _lib.launch("spf_lpips_forward", dev, args, ws, out, mean)
        if any(need):
            ctx.save_for_backward(x0, x1)
            ctx.ws, ctx.dw, ctx.params = ws, dw, (normalize, mean_weight)
        return out.view(n, 1, 1, 1) if mean is None else mean

    @staticmethod
    def backward(ctx, grad):
        x0, x1 = ctx.saved_tensors
        normalize, mean_weight = ctx.params
        dev = x0.device
        g = grad.to(torch.float32).contiguous()
        need0, need1 = ctx.needs_input_grad[:2]
        d0 = torch.empty_like(x0, memory_format=torch.contiguous_format) if need0 else None
        d1 = torch.empty_like(x1, memory_format=torch.contiguous_format) if need1 else None
        args = _args(x0, x1, ctx.dw, normalize, 1.0 if mean_weight is None else mean_weight)
        _lib.launch("spf_lpips_backward", dev, args, ctx.ws, g, int(mean_weight is not None), d0, d1)
        return d0, d1, None, None, None, None


def _run(name: str, in0: Tensor, in1: Tensor, weights, normalize: bool, mean_weight: Optional[float]) -> Tensor:
    _check_pair(name, in0, in1)
    W = resolve_weights(weights)
    if in0.dtype != torch.float32:
        in0 = in0.float()
    if in1.dtype != torch.float32:
        in1 = in1.float()
    return _Lpips.apply(in0, in1, W, bool(normalize), mean_weight, torch.is_grad_enabled())


def lpips(in0: Tensor, in1: Tensor, weights=None, normalize: bool = False) -> Tensor:
    """``LPIPS(net="vgg")(in0, in1, normalize=normalize)`` for [N,3,H,W] images on a HIP device -> [N,1,1,1] float32,
    differentiable in both.  ``normalize=True`` for images in [0, 1].  Any floating dtype and any strides; computed in
    float32, gradients cast back by autograd."""
    return _run("lpips", in0, in1, weights, normalize, None)


def lpips_mean(in0: Tensor, in1: Tensor, weights=None, normalize: bool = False, weight: float = 1.0) -> Tensor:
    """``weight * lpips(in0, in1).mean()`` with the mean (and its backward) taken inside the library: 0-dim float32."""
    return _run("lpips", in0, in1, weights, normalize, float(weight))


class LPIPS(nn.Module):
    """The package's module for ``net="vgg"``.  The weights resolve on the first call (see ``resolve_weights``)."""

    def __init__(self, net: str = "vgg", weights=None, spatial: bool = False) -> None:
        super().__init__()
        if net != "vgg":
            raise NotImplementedError(f'LPIPS: net="{net}" is not supported by this build (only "vgg")')
        if spatial:
            raise NotImplementedError("LPIPS: spatial=True is not supported by this build")
        self.weights = weights

    def forward(self, in0: Tensor, in1: Tensor, retPerLayer: bool = False, normalize: bool = False) -> Tensor:
        if retPerLayer:
            raise NotImplementedError("LPIPS: retPerLayer=True is not supported by this build")
        _check_pair("LPIPS", in0, in1)
        if not isinstance(self.weights, LpipsWeights):
            self.weights = resolve_weights(self.weights)
        return lpips(in0, in1, self.weights, normalize)


# ---- the building blocks, one kernel each, on [N,C,H,W] float32 device tensors ---------------------------------------
def conv3x3_forward(x: Tensor, layer: int, weights: LpipsWeights, relu: bool = True, normalize: bool = False) -> Tensor:
    """Convolution `layer` (1..13) with its bias (and ReLU).  Layer 1 takes the image and applies ``2x - 1`` (with
    `normalize`) and the scaling layer at the load, zero padding after it."""
    l = _layer(layer)
    _need_device("conv3x3_forward", x=x)
    if x.dim() != 4 or x.shape[1] != CONV_CIN[l]:
        raise ValueError(f"conv3x3_forward: layer {layer} takes [N,{CONV_CIN[l]},H,W], got {tuple(x.shape)}")
    dev = x.device
    n, _, h, w = x.shape
    dw = weights.on(dev)
    out = torch.empty((n, h, w, CONV_COUT[l]), dtype=torch.float32, device=dev)
    if l == 0:
        if not relu:
            raise NotImplementedError("conv3x3_forward: the first layer's kernel always applies its ReLU")
        xi = x.to(torch.float32).contiguous()
        _lib.launch("spf_lpips_conv1_forward", dev, _args(xi, None, dw, normalize), out)
    else:
        xi = _nhwc(x)
        wp = dw["wfwd"][PACK_OFFSET[l]:]
        bias = dw["bias"][sum(CONV_COUT[:l]):]
        _lib.launch("spf_lpips_conv3x3", dev, xi, None, wp, bias, out, n, h, w, CONV_CIN[l], CONV_COUT[l], int(bool(relu)))
    return _nchw(out)


def conv3x3_backward_data(g: Tensor, layer: int, weights: LpipsWeights, act: Optional[Tensor] = None,
                          normalize: bool = False) -> Tensor:
    """Gradient of layer `layer`'s input from the gradient `g` of its (post-ReLU) output.  `act`, the layer's output, is
    the mask source: `g` counts where ``act > 0`` (None: everywhere).  For layer 1 the result is the gradient of the
    image, the scaling layer (and ``2x - 1`` with `normalize`) included."""
    l = _layer(layer)
    _need_device("conv3x3_backward_data", g=g, **({} if act is None else {"act": act}))
    if g.dim() != 4 or g.shape[1] != CONV_COUT[l] or (act is not None and act.shape != g.shape):
        raise ValueError(f"conv3x3_backward_data: layer {layer} takes [N,{CONV_COUT[l]},H,W] (and `act` alike)")
    dev = g.device
    n, _, h, w = g.shape
    dw = weights.on(dev)
    gi = _nhwc(g)
    ai = _nhwc(act) if act is not None else None
    if l == 0:
        if ai is None:
            ai = torch.ones_like(gi)
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=dev)
        _lib.launch("spf_lpips_conv1_backward", dev, _args(out, None, dw, normalize), gi, ai, out)
        return out
    out = torch.empty((n, h, w, CONV_CIN[l]), dtype=torch.float32, device=dev)
    wp = dw["wbwd"][PACK_OFFSET[l]:]
    _lib.launch("spf_lpips_conv3x3", dev, gi, ai, wp, None, out, n, h, w, CONV_COUT[l], CONV_CIN[l], 0)
    return _nchw(out)


def maxpool_forward(x: Tensor) -> Tensor:
    """2x2 stride-2 max pool, floor mode."""
    _need_device("maxpool_forward", x=x)
    n, c, h, w = x.shape
    if c % 4 or h < 2 or w < 2:
        raise ValueError(f"maxpool_forward: needs C % 4 == 0 and sides >= 2, got {tuple(x.shape)}")
    xi = _nhwc(x)
    out = torch.empty((n, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    _lib.launch("spf_lpips_pool_forward", x.device, xi, out, n, h, w, c)
    return _nchw(out)


def maxpool_backward(g: Tensor, x: Tensor) -> Tensor:
    """The pooled gradient `g` routed to the first maximum (row-major) of every window of `x`."""
    _need_device("maxpool_backward", g=g, x=x)
    n, c, h, w = x.shape
    if c % 4 or h < 2 or w < 2 or tuple(g.shape) != (n, c, h // 2, w // 2):
        raise ValueError(f"maxpool_backward: shapes {tuple(g.shape)} and {tuple(x.shape)} do not belong together")
    gi, xi = _nhwc(g), _nhwc(x)
    out = torch.zeros((n, h, w, c), dtype=torch.float32, device=x.device)
    _lib.launch("spf_lpips_pool_backward", x.device, gi, xi, out, n, h, w, c)
    return _nchw(out)


def _head_operands(name: str, a: Tensor, b: Tensor, lin: Tensor):
    _need_device(name, a=a, b=b, lin=lin)
    if a.dim() != 4 or a.shape != b.shape or a.shape[1] not in (64, 128, 256, 512) or lin.numel() != a.shape[1]:
        raise ValueError(f"{name}: features [N,C,H,W] with C in 64, 128, 256, 512 and C lin entries are needed")
    return _nhwc(a), _nhwc(b), lin.to(torch.float32).reshape(-1).contiguous()


def head_forward(a: Tensor, b: Tensor, lin: Tensor) -> Tensor:
    """One tap's term: the mean over the pixels of ``sum_c lin_c (a_c / (||a|| + 1e-10) - b_c / (||b|| + 1e-10))^2`` -> [N]."""
    ai, bi, li = _head_operands("head_forward", a, b, lin)
    n, c, h, w = a.shape
    partial = torch.empty(n * ((h * w + 63) // 64), dtype=torch.float32, device=a.device)
    out = torch.empty(n, dtype=torch.float32, device=a.device)
    _lib.launch("spf_lpips_head_forward", a.device, ai, bi, li, n, h * w, c, partial, out)
    return out


def head_backward(a: Tensor, b: Tensor, lin: Tensor, upstream: Tensor, need_a: bool = True, need_b: bool = True):
    """(dL/da, dL/db) of one tap's term from ``upstream`` [N]; an entry is None when not asked for."""
    ai, bi, li = _head_operands("head_backward", a, b, lin)
    _need_device("head_backward", upstream=upstream)
    n, c, h, w = a.shape
    if upstream.numel() != n or not (need_a or need_b):
        raise ValueError("head_backward: upstream must have N entries, and one gradient must be asked for")
    up = upstream.to(torch.float32).reshape(-1).contiguous()
    da = torch.empty_like(ai) if need_a else None
    db = torch.empty_like(bi) if need_b else None
    _lib.launch("spf_lpips_head_backward", a.device, ai, bi, li, n, h * w, c, up, da, db)
    return (_nchw(da) if need_a else None), (_nchw(db) if need_b else None)
