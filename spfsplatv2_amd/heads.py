"""The DPT prediction heads on the HIP library: the memory-bound work between the convolutions, and the head modules on
top of it.

=============================  ==========================================================================================
here                           reference (src/model/encoder/heads/)
=============================  ==========================================================================================
``upsample2x``                 ``F.interpolate(scale_factor=2, mode="bilinear", align_corners=True)`` and the add that
                               follows it (``path_1 + direct_img_feat``, dpt_gs_head.py:71-73, with ``input_merger``'s ReLU)
``add_relu``                   the residual adds of a fusion block and the out-of-place ``nn.ReLU`` that follows them
                               (dpt_block.py:129, :142, :201)
``postprocess``                postprocess.py:11-78 for ``depth_mode=('exp', ..)`` and ``conf_mode`` None or ``('exp', ..)``
``ResidualConvUnit_custom``    dpt_block.py:79-142
``FeatureFusionBlock_custom``  dpt_block.py:144-218
``Interpolate``                dpt_block.py:231-262
``DPTOutputAdapter``           dpt_block.py:264-459 with the ``DPTOutputAdapter_fix`` of dpt_head.py:21-68 (no duplicated
                               ``act_N_postprocess``) and, after ``add_image_branch()``, of dpt_gs_head.py:20-78
``PixelwiseTaskWithDPT``       dpt_head.py:71-96
``PixelwiseTaskWithGSDPT``     dpt_gs_head.py:81-109 -- the reference gives this wrapper the SAME class name
                               ``PixelwiseTaskWithDPT`` in another file; one package cannot hold both under one name
``create_dpt_head``            dpt_head.py:99-117
``create_gs_dpt_head``         dpt_gs_head.py:112-130
``head_factory``               heads/__init__.py:13-25, the ``'dpt'`` and ``'dpt_gs'`` rows
=============================  ==========================================================================================

Kernels: csrc/dpt.hip.  float32 only (the encoders call the heads in float32 with autocast off), NCHW, no CPU path; a
non-contiguous or misaligned input (the cropped ``path_4[:, :, :h, :w]`` of dpt_head.py:59) is copied.  The convolutions
stay ``nn.Conv2d`` / ``nn.ConvTranspose2d``; ``nn.ReLU(True)`` on a fresh convolution output and the ``nn.Dropout`` of the
``gs_params`` head stay torch's.  Constructor parameters, attribute names and state-dict keys are the reference's (the
duplicated ``scratch.layerN_rn`` / ``scratch.layer_rn.N`` entries included).  ``input_merger``'s convolution has
``feature_dim`` output channels where the reference writes 256: the same wherever the reference's forward runs at all,
since it adds that tensor to one of ``feature_dim`` channels.  Not served: batch norm, ``output_width_ratio != 1``, any
``Interpolate`` other than (2, bilinear, align_corners=True), ``head_type='semseg'``, ``transpose_to_landscape``, the
linear and pose heads.
"""
from __future__ import annotations

import math
from typing import Iterable, List, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._checks import check_device as _check_device, check_float32 as _check_float32

MAX_SIDE = _lib.DPT_MAX_SIDE
MAX_ELEMENTS = 2 ** 31 - 1


def max_grid() -> int:
    """The most blocks a launch of csrc/dpt.hip uses (the upsample kernels: 4,096-item chunks of a plane per round).  Host only."""
    return int(_lib.load().spf_dpt_max_grid())


# ---- checks --------------------------------------------------------------------------------------------------------
# every copy ``_dense`` makes, for tools/dpt_time.py and the tests: a head step on dense NCHW tensors makes none but the
# crop of path_4, and a copy of a full-size activation is a pass the byte model does not count
dense_copies = {"calls": 0, "bytes": 0}


def _dense(t):
    """``t`` contiguous at a 16-byte aligned address: itself where it is, else a copy (counted in ``dense_copies``)."""
    if t is None:
        return None
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    dense_copies["calls"] += 1
    dense_copies["bytes"] += t.numel() * t.element_size()
    return t.contiguous() if not t.is_contiguous() else t.clone()


def _check_size(what: str, t) -> None:
    if t.numel() == 0 or t.numel() > MAX_ELEMENTS:
        raise RuntimeError(f"{what}: a tensor must hold 1 .. 2^31 - 1 elements, got shape {list(t.shape)}")


def _check_upsample(x, skip, relu_skip) -> None:
    what = "upsample2x"
    _check_float32(what, x, skip)
    if x.dim() != 4:
        raise RuntimeError(f"{what}: x must be [B, C, h, w], got shape {list(x.shape)}")
    if relu_skip and skip is None:
        raise ValueError(f"{what}: relu_skip is set without skip")
    B, C, h, w = x.shape
    if max(h, w) > MAX_SIDE:
        raise RuntimeError(f"{what}: h and w must not exceed {MAX_SIDE}, got {h} x {w}")
    if skip is not None and tuple(skip.shape) != (B, C, 2 * h, 2 * w):
        raise RuntimeError(f"{what}: skip must have shape {[B, C, 2 * h, 2 * w]}, got {list(skip.shape)}")
    _check_size(what, x)
    if 4 * x.numel() > MAX_ELEMENTS:
        raise RuntimeError(f"{what}: the output must hold fewer than 2^31 elements, got x of shape {list(x.shape)}")
    _check_device(what, x, skip)


def _check_add_relu(a, b, c) -> None:
    what = "add_relu"
    _check_float32(what, a, b, c)
    if c is not None and b is None:
        raise ValueError(f"{what}: c is given without b")
    for name, t in (("b", b), ("c", c)):
        if t is not None and t.shape != a.shape:
            raise RuntimeError(f"{what}: a {list(a.shape)} and {name} {list(t.shape)} differ in shape")
    _check_size(what, a)
    _check_device(what, a, b, c)


def _exp_mode(what: str, mode):
    """('exp', vmin, vmax) -> (vmin, vmax) as floats; anything else is not served."""
    if not (isinstance(mode, (tuple, list)) and len(mode) == 3 and mode[0] == "exp"):
        raise NotImplementedError(f"{what} {mode!r} is not served: only ('exp', vmin, vmax)")
    vmin, vmax = float(mode[1]), float(mode[2])
    if math.isnan(vmin) or math.isnan(vmax) or vmin > vmax:
        raise ValueError(f"{what} {mode!r}: the bounds must be ordered")
    return vmin, vmax


def _check_modes(depth_mode, conf_mode):
    return _exp_mode("depth_mode", depth_mode), (None if conf_mode is None else _exp_mode("conf_mode", conf_mode))


def _check_postprocess(out, conf) -> None:
    what = "postprocess"
    _check_float32(what, out)
    need = 4 if conf is not None else 3
    if out.dim() != 4 or out.shape[1] < need:
        raise RuntimeError(f"{what}: out must be [B, C >= {need}, H, W], got shape {list(out.shape)}")
    _check_size(what, out)
    _check_device(what, out)


# ---- autograd --------------------------------------------------------------------------------------------------------
class _Upsample2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip, relu_skip):
        x, skip = _dense(x), _dense(skip)
        B, C, h, w = x.shape
        out = torch.empty(B, C, 2 * h, 2 * w, dtype=x.dtype, device=x.device)
        _lib.launch("spf_dpt_upsample2x_forward", x.device, x, skip, int(relu_skip), B * C, h, w, out)
        ctx.save_for_backward(skip if relu_skip else None)       # the convolution output, never relu(skip)
        ctx.shape, ctx.has_skip, ctx.relu = x.shape, skip is not None, bool(relu_skip)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (skip,) = ctx.saved_tensors
        need_x, need_skip = ctx.needs_input_grad[0], ctx.has_skip and ctx.needs_input_grad[1]
        dy = _dense(dy)
        B, C, h, w = ctx.shape
        dx = dskip = None
        if need_x or (need_skip and ctx.relu):
            dx = torch.empty(ctx.shape, dtype=dy.dtype, device=dy.device) if need_x else None
            dskip = torch.empty_like(dy) if ctx.relu else None
            _lib.launch("spf_dpt_upsample2x_backward", dy.device, dy, skip, B * C, h, w, dx, dskip)
        if not ctx.relu:
            dskip = dy                                           # the same tensor, no copy
        return dx if need_x else None, dskip if need_skip else None, None


def _add_relu_backward(y, dy, ds):
    dy, ds = _dense(dy), _dense(ds)
    g = torch.empty_like(y)
    _lib.launch("spf_dpt_add_relu_backward", y.device, y, dy, ds, y.numel(), g)
    return g


class _Relu(torch.autograd.Function):
    """add_relu with one addend: the out-of-place ReLU."""

    @staticmethod
    def forward(ctx, a):
        a = _dense(a)
        y = torch.empty_like(a)
        _lib.launch("spf_dpt_add_relu_forward", a.device, a, None, None, a.numel(), None, y)
        ctx.save_for_backward(y)                                 # (the convolution that reads y keeps it anyway)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return _add_relu_backward(y, dy, None)


class _AddRelu(torch.autograd.Function):
    """Two or three addends -> (s, y)."""

    @staticmethod
    def forward(ctx, a, b, c):
        a, b, c = _dense(a), _dense(b), _dense(c)
        s, y = torch.empty_like(a), torch.empty_like(a)
        _lib.launch("spf_dpt_add_relu_forward", a.device, a, b, c, a.numel(), s, y)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(y)
        ctx.three = c is not None
        return s, y

    @staticmethod
    @once_differentiable
    def backward(ctx, ds, dy):
        g = ds if dy is None else _add_relu_backward(ctx.saved_tensors[0], dy, ds)
        return g, g, g if ctx.three else None


class _Points(torch.autograd.Function):
    @staticmethod
    def _args(out, depth, conf):
        a = _lib.SpfDptPoints()
        a.in_ = out.data_ptr()
        a.B, a.C, a.HW = out.shape[0], out.shape[1], out.shape[2] * out.shape[3]
        a.has_conf = int(conf is not None)
        a.depth_min, a.depth_max = depth
        a.conf_min, a.conf_max = conf if conf is not None else (0.0, 0.0)
        return a

    @staticmethod
    def forward(ctx, out, depth, conf):
        out = _dense(out)
        B, _, H, W = out.shape
        pts = torch.empty(B, H, W, 3, dtype=out.dtype, device=out.device)
        cf = torch.empty(B, H, W, dtype=out.dtype, device=out.device) if conf is not None else None
        _lib.launch("spf_dpt_points_forward", out.device, _Points._args(out, depth, conf), pts, cf)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out)
        ctx.depth, ctx.conf = depth, conf
        return pts if conf is None else (pts, cf)

    @staticmethod
    @once_differentiable
    def backward(ctx, dpts, dconf=None):
        (out,) = ctx.saved_tensors
        if dpts is None and dconf is None:
            return None, None, None
        B, C, H, W = out.shape
        dpts = _dense(dpts) if dpts is not None else torch.zeros(B, H, W, 3, dtype=out.dtype, device=out.device)
        if ctx.conf is not None:
            dconf = _dense(dconf) if dconf is not None else torch.zeros(B, H, W, dtype=out.dtype, device=out.device)
        used = 4 if ctx.conf is not None else 3
        din = torch.empty_like(out) if C == used else torch.zeros_like(out)
        _lib.launch("spf_dpt_points_backward", out.device, _Points._args(out, ctx.depth, ctx.conf), dpts, dconf, din)
        return din, None, None


def upsample2x(x, skip=None, relu_skip: bool = False):
    """``F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)`` of x [B, C, h, w], plus ``skip``
    [B, C, 2h, 2w], or plus ``relu(skip)`` with ``relu_skip``, in one pass.  The backward gathers the gradient of x per
    input pixel in a fixed order (no atomics); the gradient of skip IS the upstream gradient -- one tensor, no copy --
    or, with ``relu_skip``, that gradient masked by ``skip > 0``: the saved tensor is skip itself."""
    _check_upsample(x, skip, relu_skip)
    return _Upsample2x.apply(x, skip, bool(relu_skip))


def add_relu(a, b=None, c=None):
    """``s = a + b (+ c)`` and ``y = relu(s)`` in one pass: returns ``(s, y)``.  With ``a`` alone it is the out-of-place
    ReLU and ``s`` is ``a``.  The backward writes ``ds + dy * (s > 0)`` once: it is the gradient of every addend."""
    _check_add_relu(a, b, c)
    if b is None:
        return a, _Relu.apply(a)
    return _AddRelu.apply(a, b, c)


def postprocess(out, depth_mode, conf_mode):
    """postprocess.py:11-78 of a head output [B, 3 (+ 1), H, W]: ``{"pts3d": [B, H, W, 3]}`` and, with a ``conf_mode``,
    ``"conf": [B, H, W]``, in one pass each way.  ``depth_mode`` must be ``('exp', vmin, vmax)`` and ``conf_mode`` None or
    ``('exp', vmin, vmax)``: every other mode raises ``NotImplementedError`` before anything is launched."""
    depth, conf = _check_modes(depth_mode, conf_mode)
    _check_postprocess(out, conf)
    res = _Points.apply(out, depth, conf)
    return dict(pts3d=res) if conf is None else dict(pts3d=res[0], conf=res[1])


# ---- modules ---------------------------------------------------------------------------------------------------------
def pair(t):
    return t if isinstance(t, tuple) else (t, t)


def make_scratch(in_shape, out_shape, groups=1, expand=False):
    scratch = nn.Module()
    outs = [out_shape * (2 ** i if expand else 1) for i in range(4)]
    scratch.layer1_rn = nn.Conv2d(in_shape[0], outs[0], kernel_size=3, stride=1, padding=1, bias=False, groups=groups)
    scratch.layer2_rn = nn.Conv2d(in_shape[1], outs[1], kernel_size=3, stride=1, padding=1, bias=False, groups=groups)
    scratch.layer3_rn = nn.Conv2d(in_shape[2], outs[2], kernel_size=3, stride=1, padding=1, bias=False, groups=groups)
    scratch.layer4_rn = nn.Conv2d(in_shape[3], outs[3], kernel_size=3, stride=1, padding=1, bias=False, groups=groups)
    scratch.layer_rn = nn.ModuleList([scratch.layer1_rn, scratch.layer2_rn, scratch.layer3_rn, scratch.layer4_rn])
    return scratch


def _check_relu(owner: str, activation) -> None:
    if not isinstance(activation, nn.ReLU):
        raise TypeError(f"{owner}: activation must be an nn.ReLU, got {activation!r}")


class ResidualConvUnit_custom(nn.Module):
    """dpt_block.py:79-142 without batch norm.  ``branch`` is the unit without its skip add, which a fusion block moves
    into its next fused call."""

    def __init__(self, features, activation, bn):
        super().__init__()
        if bn:
            raise NotImplementedError("ResidualConvUnit_custom: batch norm (bn=True) is not served")
        _check_relu("ResidualConvUnit_custom", activation)
        self.bn = bn
        self.groups = 1
        self.conv1 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=not self.bn, groups=self.groups)
        self.conv2 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=not self.bn, groups=self.groups)
        self.activation = activation
        self.skip_add = torch.ao.nn.quantized.FloatFunctional()

    def branch(self, y):
        """``conv2(relu(conv1(y)))`` of ``y = relu(x)``: the ReLU between the convolutions runs in place on the fresh
        convolution output."""
        return self.conv2(F.relu(self.conv1(y), inplace=True))

    def forward(self, x):
        return self.branch(add_relu(x)[1]) + x


class FeatureFusionBlock_custom(nn.Module):
    """dpt_block.py:144-218 at ``width_ratio == 1``.  With two inputs ``xs[0] + resConfUnit1(xs[1])`` -- itself
    ``conv2(..) + xs[1]`` -- and the ReLU that opens ``resConfUnit2`` are one ``add_relu`` of three addends;
    ``resConfUnit2``'s own skip add stays a tensor add; the upsample is ``upsample2x``."""

    def __init__(self, features, activation, deconv=False, bn=False, expand=False, align_corners=True, width_ratio=1):
        super().__init__()
        if width_ratio != 1:
            raise NotImplementedError("FeatureFusionBlock_custom: width_ratio != 1 (output_width_ratio) is not served")
        if not align_corners:
            raise NotImplementedError("FeatureFusionBlock_custom: only align_corners=True is served")
        self.width_ratio = width_ratio
        self.deconv = deconv
        self.align_corners = align_corners
        self.groups = 1
        self.expand = expand
        out_features = features // 2 if self.expand else features
        self.out_conv = nn.Conv2d(features, out_features, kernel_size=1, stride=1, padding=0, bias=True, groups=1)
        self.resConfUnit1 = ResidualConvUnit_custom(features, activation, bn)
        self.resConfUnit2 = ResidualConvUnit_custom(features, activation, bn)
        self.skip_add = torch.ao.nn.quantized.FloatFunctional()

    def forward(self, *xs):
        if len(xs) == 2:
            r = self.resConfUnit1.branch(add_relu(xs[1])[1])
            s, y = add_relu(r, xs[1], xs[0])
        else:
            s, y = add_relu(xs[0])
        return self.out_conv(upsample2x(self.resConfUnit2.branch(y) + s))


def make_fusion_block(features, use_bn, width_ratio=1, expand=False):
    return FeatureFusionBlock_custom(features, nn.ReLU(False), deconv=False, bn=use_bn, expand=expand, align_corners=True,
                                     width_ratio=width_ratio)


class Interpolate(nn.Module):
    """dpt_block.py:231-262 for the one configuration the heads use: (2, "bilinear", align_corners=True)."""

    def __init__(self, scale_factor, mode, align_corners=False):
        super().__init__()
        if scale_factor != 2 or mode != "bilinear" or align_corners is not True:
            raise NotImplementedError(f"Interpolate: only scale_factor=2, mode='bilinear', align_corners=True is served, "
                                      f"got ({scale_factor!r}, {mode!r}, {align_corners!r})")
        self.interp = upsample2x
        self.scale_factor = scale_factor
        self.mode = mode
        self.align_corners = align_corners

    def forward(self, x):
        return upsample2x(x)


class DPTOutputAdapter(nn.Module):
    """dpt_block.py:264-459 as the heads use it: ``init`` drops the duplicated ``act_N_postprocess`` attributes
    (``DPTOutputAdapter_fix``), and ``add_image_branch`` adds dpt_gs_head.py's ``feat_up`` and ``input_merger``.
    ``forward`` is dpt_head.py's ``forward(tokens, image_size, ray_embedding=None)`` without that branch and
    dpt_gs_head.py's ``forward(tokens, imgs, image_size, conf=None)`` with it."""

    def __init__(self, num_channels: int = 1, stride_level: int = 1, patch_size: Union[int, Tuple[int, int]] = 16,
                 main_tasks: Iterable[str] = ('rgb',), hooks: List[int] = [2, 5, 8, 11],
                 layer_dims: List[int] = [96, 192, 384, 768], feature_dim: int = 256, last_dim: int = 32,
                 use_bn: bool = False, dim_tokens_enc: Optional[int] = None, head_type: str = 'regression',
                 output_width_ratio=1, **kwargs):
        super().__init__()
        if use_bn:
            raise NotImplementedError("DPTOutputAdapter: batch norm (use_bn=True) is not served")
        if output_width_ratio != 1:
            raise NotImplementedError("DPTOutputAdapter: output_width_ratio != 1 is not served")
        if head_type == 'semseg':
            raise NotImplementedError("DPTOutputAdapter: head_type='semseg' is not served")
        if head_type not in ('regression', 'gs_params'):
            raise ValueError('DPT head_type must be "regression" or "gs_params".')
        # the attribute names are the reference's: callers and checkpoints read them
        self.num_channels, self.stride_level, self.patch_size = num_channels, stride_level, pair(patch_size)
        self.main_tasks, self.hooks, self.layer_dims, self.feature_dim = main_tasks, hooks, layer_dims, feature_dim
        self.head_type = head_type
        self.dim_tokens_enc = None if dim_tokens_enc is None else dim_tokens_enc * len(main_tasks)
        # a token covers patch_size / stride_level pixels of the image this head is told about, at least one
        self.P_H, self.P_W = (max(1, side // stride_level) for side in self.patch_size)
        self.scratch = make_scratch(layer_dims, feature_dim, groups=1, expand=False)
        for n in (1, 2, 3, 4):                               # registered in this order: the state dict's
            setattr(self.scratch, f"refinenet{n}", make_fusion_block(feature_dim, use_bn, output_width_ratio))
        if self.head_type == 'regression':
            self.head = nn.Sequential(
                nn.Conv2d(feature_dim, feature_dim // 2, kernel_size=3, stride=1, padding=1),
                Interpolate(scale_factor=2, mode="bilinear", align_corners=True),
                nn.Conv2d(feature_dim // 2, last_dim, kernel_size=3, stride=1, padding=1),
                nn.ReLU(True),
                nn.Conv2d(last_dim, self.num_channels, kernel_size=1, stride=1, padding=0))
        else:
            self.head = nn.Sequential(
                nn.Conv2d(feature_dim, feature_dim, kernel_size=3, padding=1, bias=False),
                nn.Identity(),
                nn.ReLU(True),
                nn.Dropout(0.1, False),
                nn.Conv2d(feature_dim, self.num_channels, kernel_size=1))
        if self.dim_tokens_enc is not None:
            self.init(dim_tokens_enc=dim_tokens_enc)

    def init(self, dim_tokens_enc=768):
        """The parts that depend on the width of the encoder tokens: ``act_postprocess``."""
        if isinstance(dim_tokens_enc, int):
            dim_tokens_enc = 4 * [dim_tokens_enc]
        self.dim_tokens_enc = [dt * len(self.main_tasks) for dt in dim_tokens_enc]
        d, ld = self.dim_tokens_enc, self.layer_dims
        self.act_postprocess = nn.ModuleList([
            nn.Sequential(nn.Conv2d(d[0], ld[0], kernel_size=1, stride=1, padding=0),
                          nn.ConvTranspose2d(ld[0], ld[0], kernel_size=4, stride=4, padding=0, bias=True, dilation=1, groups=1)),
            nn.Sequential(nn.Conv2d(d[1], ld[1], kernel_size=1, stride=1, padding=0),
                          nn.ConvTranspose2d(ld[1], ld[1], kernel_size=2, stride=2, padding=0, bias=True, dilation=1, groups=1)),
            nn.Sequential(nn.Conv2d(d[2], ld[2], kernel_size=1, stride=1, padding=0)),
            nn.Sequential(nn.Conv2d(d[3], ld[3], kernel_size=1, stride=1, padding=0),
                          nn.Conv2d(ld[3], ld[3], kernel_size=3, stride=2, padding=1))])

    def add_image_branch(self):
        """dpt_gs_head.py:35-39: the upsample of ``path_1`` and the 7 x 7 convolution of the image that is added to it."""
        self.feat_up = Interpolate(scale_factor=2, mode="bilinear", align_corners=True)
        self.input_merger = nn.Sequential(nn.Conv2d(3, self.feature_dim, 7, 1, 3), nn.ReLU())

    def adapt_tokens(self, encoder_tokens):
        return encoder_tokens[:, :]

    def _path_1(self, encoder_tokens, image_size):
        if self.dim_tokens_enc is None:
            raise RuntimeError("DPTOutputAdapter: init(dim_tokens_enc) has not been called")
        if image_size is None:
            raise ValueError("DPTOutputAdapter: image_size is required")
        grid = (image_size[0] // (self.stride_level * self.P_H), image_size[1] // (self.stride_level * self.P_W))
        tokens = [self.adapt_tokens(encoder_tokens[hook]) for hook in self.hooks]
        _check_float32("DPTOutputAdapter", *tokens)
        feats = []
        for t, act, project in zip(tokens, self.act_postprocess, self.scratch.layer_rn):
            # [B, nh nw, C] -> a dense [B, C, nh, nw] COPY of the (small) tokens (reshape alone would return a view with
            # channels-last strides): such a view would make the first convolution, and every convolution after it,
            # answer in channels-last, and every fused call would then copy its (large) operands back
            feats.append(project(act(t.transpose(1, 2).contiguous().view(t.shape[0], t.shape[2], *grid))))
        # coarse to fine; refinenet4's x2 output is cropped to the next level's grid (an odd grid halves rounding up)
        path = self.scratch.refinenet4(feats[3])[:, :, :feats[2].shape[2], :feats[2].shape[3]]
        for n in (3, 2, 1):
            path = getattr(self.scratch, f"refinenet{n}")(path, feats[n - 1])
        return path

    def forward_pts(self, encoder_tokens: List[torch.Tensor], image_size=None, ray_embedding=None):
        return self.head(self._path_1(encoder_tokens, image_size))

    def forward_gs(self, encoder_tokens: List[torch.Tensor], imgs, image_size=None, conf=None):
        path_1 = self._path_1(encoder_tokens, image_size)
        # feat_up, input_merger's ReLU and the add in one pass; the convolution output is what the backward keeps
        path_1 = upsample2x(path_1, skip=self.input_merger[0](imgs), relu_skip=True)
        return self.head(path_1)

    def forward(self, encoder_tokens, *args, **kwargs):
        if hasattr(self, "input_merger"):
            return self.forward_gs(encoder_tokens, *args, **kwargs)
        return self.forward_pts(encoder_tokens, *args, **kwargs)


class PixelwiseTaskWithDPT(nn.Module):
    """dpt_head.py:71-96: the DPT head of the point maps; can return 3D points + confidence for all pixels."""

    def __init__(self, *, n_cls_token=0, hooks_idx=None, dim_tokens=None, output_width_ratio=1, num_channels=1,
                 postprocess=None, depth_mode=None, conf_mode=None, **kwargs):
        super().__init__()
        self.return_all_layers = True  # backbone needs to return all layers
        self.postprocess = postprocess
        self.depth_mode = depth_mode
        self.conf_mode = conf_mode
        assert n_cls_token == 0, "Not implemented"
        if postprocess is globals()["postprocess"]:
            _check_modes(depth_mode, conf_mode)
        dpt_args = dict(output_width_ratio=output_width_ratio, num_channels=num_channels, **kwargs)
        if hooks_idx is not None:
            dpt_args.update(hooks=hooks_idx)
        self.dpt = DPTOutputAdapter(**dpt_args)
        dpt_init_args = {} if dim_tokens is None else {'dim_tokens_enc': dim_tokens}
        self.dpt.init(**dpt_init_args)

    def forward(self, x, img_info, ray_embedding=None):
        out = self.dpt(x, image_size=(img_info[0], img_info[1]), ray_embedding=ray_embedding)
        if self.postprocess:
            out = self.postprocess(out, self.depth_mode, self.conf_mode)
        return out


class PixelwiseTaskWithGSDPT(PixelwiseTaskWithDPT):
    """dpt_gs_head.py:81-109, which the reference also names ``PixelwiseTaskWithDPT``: the DPT head of the Gaussian
    parameters, with the image branch; ``forward(x, imgs, img_info, conf=None)``."""

    def __init__(self, *, n_cls_token=0, hooks_idx=None, dim_tokens=None, output_width_ratio=1, num_channels=1,
                 postprocess=None, depth_mode=None, conf_mode=None, **kwargs):
        super().__init__(n_cls_token=n_cls_token, hooks_idx=hooks_idx, dim_tokens=dim_tokens,
                         output_width_ratio=output_width_ratio, num_channels=num_channels, postprocess=postprocess,
                         depth_mode=depth_mode, conf_mode=conf_mode, **kwargs)
        self.dpt.add_image_branch()

    def forward(self, x, imgs, img_info, conf=None):
        out = self.dpt(x, imgs, image_size=(img_info[0], img_info[1]), conf=conf)
        if self.postprocess:
            out = self.postprocess(out, self.depth_mode, self.conf_mode)
        return out


def _head_args(net, has_conf, out_nchan, postprocess_func, head_type):
    assert net.dec_depth > 9
    l2 = net.dec_depth
    feature_dim = 256
    ed, dd = net.enc_embed_dim, net.dec_embed_dim
    return dict(num_channels=out_nchan + has_conf, feature_dim=feature_dim, last_dim=feature_dim // 2,
                hooks_idx=[0, l2 * 2 // 4, l2 * 3 // 4, l2], dim_tokens=[ed, dd, dd, dd], postprocess=postprocess_func,
                depth_mode=net.depth_mode, conf_mode=net.conf_mode, head_type=head_type)


def create_dpt_head(net, has_conf=False, out_nchan=3, postprocess_func=postprocess):
    """dpt_head.py:99-117: the ``PixelwiseTaskWithDPT`` for the given net parameters."""
    return PixelwiseTaskWithDPT(**_head_args(net, has_conf, out_nchan, postprocess_func, 'regression'))


def create_gs_dpt_head(net, has_conf=False, out_nchan=3, postprocess_func=postprocess):
    """dpt_gs_head.py:112-130: the ``PixelwiseTaskWithGSDPT`` for the given net parameters."""
    return PixelwiseTaskWithGSDPT(**_head_args(net, has_conf, out_nchan, postprocess_func, 'gs_params'))


def head_factory(head_type, output_mode, net, has_conf=False, out_nchan=3, pose_init_t=False, use_homogeneous=True,
                 concat_enc=True):
    """heads/__init__.py:13-25 for the DPT rows; the linear head stays the caller's."""
    if head_type == 'dpt' and output_mode == 'pts3d':
        return create_dpt_head(net, has_conf=has_conf)
    if head_type == 'dpt' and output_mode == 'gs_params':
        return create_dpt_head(net, has_conf=False, out_nchan=out_nchan, postprocess_func=None)
    if head_type == 'dpt_gs' and output_mode == 'gs_params':
        return create_gs_dpt_head(net, has_conf=False, out_nchan=out_nchan, postprocess_func=None)
    raise NotImplementedError(f"unexpected {head_type=} and {output_mode=}")
