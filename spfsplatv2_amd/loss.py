"""Photometric MSE loss on the HIP library: host mirror of the reference's ``LossMse``.

=====================  =========================================================================
here                   reference (/root/reference/src/loss/)
=====================  =========================================================================
``LossMseCfg``         loss_mse.py:13-16
``LossMseCfgWrapper``  loss_mse.py:18-20
``Loss``               loss.py:17-40 (the config wrapper convention: one dataclass field = the loss's name)
``LossMse``            loss_mse.py:36-51: ``weight * ((prediction - image) ** 2).mean()``, 0 before ``apply_after_step``
``mse_loss``           the same expression as a function (what ``bench.py`` and the tests call)
``LossReprojCfg``      loss_reproj.py:13-18
``LossReprojCfgWrapper`` loss_reproj.py:21-23
``LossReproj``         loss_reproj.py:29-101 (+ project_to_cam, misc/cam_utils.py:289-307): the reprojection loss
``reproj_loss``        the same as a function; also takes ``[b,v,h,w,3]`` and returns one loss per view in one call
``LossLpipsCfg``       loss_lpips.py:16-19
``LossLpipsCfgWrapper`` loss_lpips.py:22-24
``LossLpips``          loss_lpips.py:57-85: ``weight * LPIPS(net="vgg")(prediction, image, normalize=True).mean()`` over
                       the ``b v`` images, 0 before ``apply_after_step``; the network is spfsplatv2_amd/lpips.py
``Regr3D``             loss_point.py:188-254 (+ normalize_pointcloud, geometry/ptc_geometry.py:270-328): the distillation
                       point loss, as model_wrapper.py:171 builds it and :323-331 calls it
``regr3d_loss``        the same as a function; ``return_stats=True`` also returns the counts, thresholds and norms
=====================  =========================================================================

The reference evaluates the expression with eager PyTorch (four kernels forward, four backward over the rendered
batch); here it is one pass forward and one backward, and the sum is taken in a fixed order (bit-reproducible).
No CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

import math
from abc import ABC, abstractmethod
from dataclasses import dataclass, fields
from typing import Generic, TypeVar

import torch
from torch import Tensor, nn

from . import _lib

T_cfg = TypeVar("T_cfg")
T_wrapper = TypeVar("T_wrapper")


def _check(prediction: Tensor, image: Tensor) -> None:
    for name, t in (("prediction", prediction), ("image", image)):
        if not t.is_cuda:
            raise RuntimeError(f"mse_loss: {name} is on {t.device}; this build only runs on a HIP device (no CPU "
                               "fallback)")
        if not t.is_floating_point():
            raise RuntimeError(f"mse_loss: {name} must be a floating-point tensor, got {t.dtype}")
    if prediction.numel() == 0 or image.numel() == 0:
        raise RuntimeError("mse_loss: empty input")


def _kernel_operand(t: Tensor) -> Tensor:
    """What the kernel reads: float32, contiguous, 16-byte aligned (a slice of an odd-sized image is contiguous but
    may start anywhere: copied once rather than refused)."""
    t = t.to(torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.contiguous_format)


_ONES: dict = {}


def unit_grad(device) -> Tensor:
    """THE dL/dloss = 1 of this process on `device`: a cached 0-dim float32 one.  `loss.backward(gradient=unit_grad(dev))`
    saves autograd's fill kernel, and the loss's backward recognises this very tensor (by its storage) and hands the
    forward's unit gradient on without even the one-scalar look of `spf_mse_scale_grad`: no launch at all.  Never write
    to it."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    t = _ONES.get(dev)
    if t is None:
        t = _ONES[dev] = torch.ones((), dtype=torch.float32, device=dev)
    return t


class _Mse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prediction: Tensor, image: Tensor, weight: float, grad_mode: bool = True):
        p, t = _kernel_operand(prediction), _kernel_operand(image)
        dev = p.device
        # per-call scratch for the block partials (a few KB from the caching allocator): two streams computing
        # losses at the same time never share it
        partial = torch.empty(_lib.load().spf_mse_partial_blocks(), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        # when a backward will come, the forward pass also writes the gradient for dL/dloss = 1 (what
        # `loss.backward()` passes): the backward is then one scalar look at the upstream gradient
        # (`grad_mode` = torch.is_grad_enabled() at the CALL SITE: needs_input_grad stays True under no_grad, and an
        #  evaluation loss on a tensor that requires grad must not pay a batch-sized allocation and write)
        unit = torch.empty_like(p) if (grad_mode and ctx.needs_input_grad[0]) else None
        if unit is not None:
            _lib.launch("spf_mse_forward_grad", dev, p, t, p.numel(), float(weight), partial, loss, unit)
        else:
            _lib.launch("spf_mse_forward", dev, p, t, p.numel(), float(weight), partial, loss)
        ctx.save_for_backward(p, t)
        ctx.unit = unit
        ctx.weight = float(weight)
        ctx.shape = prediction.shape
        return loss

    @staticmethod
    def backward(ctx, g):
        p, t = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        unit, ctx.unit = ctx.unit, None
        if unit is not None:
            # first backward through this node: the forward's unit gradient, scaled in place by dL/dloss (a no-op
            # launch when that is 1).  The buffer is handed to autograd; a second backward (retain_graph) recomputes.
            gp = unit
            one = _ONES.get(g.device)
            if not (one is not None and g.data_ptr() == one.data_ptr()):     # (unit_grad(): exactly 1, nothing to do)
                _lib.launch("spf_mse_scale_grad", p.device, gp, gp.numel(), g)
        else:
            gp = torch.empty_like(p)
            _lib.launch("spf_mse_backward", p.device, p, t, p.numel(), ctx.weight, g, gp)
        gp = gp.view(ctx.shape)
        gi = -gp if ctx.needs_input_grad[1] else None
        return gp, gi, None, None


def mse_loss(prediction: Tensor, image: Tensor, weight: float = 1.0) -> Tensor:
    """``weight * ((prediction - image) ** 2).mean()`` (loss_mse.py:48-51) as one fused pass; 0-dim float32 result.
    Like the reference's expression it accepts broadcastable shapes and any floating dtype (bf16 under autocast):
    operands are expanded / cast to float32 on the host side of the kernel and the gradients are cast / reduced back
    by autograd."""
    _check(prediction, image)
    if prediction.shape != image.shape:
        prediction, image = torch.broadcast_tensors(prediction, image)
    if prediction.dtype != torch.float32:
        prediction = prediction.float()
    if image.dtype != torch.float32:
        image = image.float()
    return _Mse.apply(prediction, image, weight, torch.is_grad_enabled())


class Loss(nn.Module, ABC, Generic[T_cfg, T_wrapper]):
    cfg: T_cfg
    name: str

    def __init__(self, cfg: T_wrapper) -> None:
        super().__init__()
        (field,) = fields(type(cfg))            # the wrapper's single field names the loss (loss.py:24-31)
        self.cfg = getattr(cfg, field.name)
        self.name = field.name

    @abstractmethod
    def forward(self, prediction, batch, gaussians, global_step: int) -> Tensor:
        ...


@dataclass
class LossMseCfg:
    weight: float
    apply_after_step: int


@dataclass
class LossMseCfgWrapper:
    mse: LossMseCfg


class LossMse(Loss[LossMseCfg, LossMseCfgWrapper]):
    def forward(self, prediction: Tensor, image: Tensor, gaussians, global_step: int) -> Tensor:
        if global_step < self.cfg.apply_after_step:           # not applied yet (loss_mse.py:44-46)
            return torch.tensor(0, dtype=torch.float32, device=image.device)
        return mse_loss(prediction, image, self.cfg.weight)


# ---- reprojection loss -------------------------------------------------------------------------------------------
# mode string -> kernel term (include/spfsplat_hip.h SPF_REPROJ_*): "tanh" and "dyntanh" differ only in lw; every
# string the reference does not name takes its `else` branch, the l1 + log term (loss_reproj.py:150-155)
_REPROJ_MODES = {"tanh": 0, "dyntanh": 0, "l1": 1, "l1+sqrt": 2}
_REPROJ_LOG = 3


def reproj_lw(mode: str, global_step, total_iterations, circle_schedule: bool, soft_clamp: float = 50.0,
              soft_clamp_min: float = 1.0) -> float:
    """The tanh scale lw of `mode` (loss_reproj.py:117-133), in float64 on the host as the reference computes it:
    "tanh": soft_clamp; "dyntanh": (1 - s) soft_clamp + soft_clamp_min with s = global_step / total_iterations, or
    1 - sqrt(1 - s^2) with the circle schedule (NaN past total_iterations, as np.sqrt gives there).  Other modes: 1."""
    if mode == "tanh":
        return float(soft_clamp)
    if mode != "dyntanh":
        return 1.0
    s = global_step / total_iterations
    if circle_schedule:
        r = 1 - s ** 2
        s = 1 - math.sqrt(r) if r >= 0 else math.nan
    return (1 - s) * soft_clamp + soft_clamp_min


def _reproj_args(p5: Tensor, poses: Tensor, intr: Tensor, code: int, weight: float, lw: float, hard: float,
                 soft: float):
    b, v, h, w, _ = p5.shape
    return _lib.SpfReproj(_lib.ptr(p5), p5.stride(0), p5.stride(1), _lib.ptr(poses), _lib.ptr(intr), b, v, h, w, code,
                          weight, lw, hard, soft)


class _Reproj(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts3d: Tensor, poses: Tensor, intrinsics: Tensor, code: int, weight: float, lw: float,
                hard: float, soft: float):
        batched = pts3d.dim() == 5
        p5 = pts3d if batched else pts3d.unsqueeze(1)
        if not p5[0, 0].is_contiguous():        # the kernels stride over [b, v] only; each image is read contiguous
            p5 = p5.contiguous()
        b, v, h, w, _ = p5.shape
        po = poses.reshape(b, v, 4, 4).contiguous()
        ki = intrinsics.reshape(b, v, 3, 3).contiguous()
        dev = p5.device
        args = _reproj_args(p5, po, ki, code, weight, lw, hard, soft)
        nslots = _lib.load().spf_reproj_partial_blocks(b, v, h, w)
        partial = torch.empty(2 * nslots, dtype=torch.float32, device=dev)
        loss = torch.empty((v,) if batched else (), dtype=torch.float32, device=dev)
        scale = torch.empty(v, dtype=torch.float32, device=dev)
        _lib.launch("spf_reproj_forward", dev, args, partial, loss, scale)
        ctx.save_for_backward(p5, po, ki, scale)
        ctx.params = (code, weight, lw, hard, soft, nslots)
        ctx.shapes = (pts3d.shape, poses.shape, intrinsics.shape)
        return loss

    @staticmethod
    def backward(ctx, grad):
        p5, po, ki, scale = ctx.saved_tensors
        code, weight, lw, hard, soft, nslots = ctx.params
        need_p, need_pose, need_k = ctx.needs_input_grad[:3]
        b, v = p5.shape[:2]
        dev = p5.device
        g = grad.to(torch.float32).reshape(v).contiguous()
        dp = torch.empty(p5.shape, dtype=torch.float32, device=dev) if need_p else None
        dpose = torch.empty(b, v, 4, 4, dtype=torch.float32, device=dev) if need_pose else None
        dk = torch.empty(b, v, 3, 3, dtype=torch.float32, device=dev) if need_k else None
        gpartial = (torch.empty(24 * nslots, dtype=torch.float32, device=dev) if (need_pose or need_k) else None)
        _lib.launch("spf_reproj_backward", dev, _reproj_args(p5, po, ki, code, weight, lw, hard, soft), scale, g, dp,
                    gpartial, dpose, dk)
        sp, spose, sk = ctx.shapes
        return (dp.view(sp) if dp is not None else None, dpose.view(spose) if dpose is not None else None,
                dk.view(sk) if dk is not None else None, None, None, None, None, None)


def reproj_loss(pts3d: Tensor, im_poses: Tensor, intrinsics: Tensor, *, weight: float, mode: str, global_step,
                total_iterations, circle_schedule: bool, detach_pts3d: bool = False, hard_clamp: float = 1000.0,
                soft_clamp: float = 50.0, soft_clamp_min: float = 1.0) -> Tensor:
    """``LossReproj.forward`` (loss_reproj.py:53-101) on the HIP library: pts3d [b,h,w,3] (world points, one per pixel),
    im_poses [b,4,4] (camera -> world), intrinsics [b,3,3] (normalised) -> a 0-dim float32 loss.  With pts3d
    [b,v,h,w,3], im_poses [b,v,4,4] and intrinsics [b,v,3,3] it returns loss[v], view i normalised by its own valid
    count: what v calls with ``pts3d[:, i]`` return, bitwise, in four launches whatever v is.

    Differences from the reference, all deliberate: when no point is valid the loss is a 0-dim device zero with zero
    gradients (the reference returns the Python int 0); bf16 / f16 / f64 inputs are computed in float32 (the reference
    would compute float64 in float64) and their gradients are cast back by autograd; nothing synchronises the host (no
    pixel grid upload, no torch.inverse singularity check: a singular pose gives non-finite values, not an error)."""
    if pts3d.dim() not in (4, 5) or pts3d.shape[-1] != 3:
        raise RuntimeError(f"reproj_loss: pts3d must be [b,h,w,3] or [b,v,h,w,3], got {tuple(pts3d.shape)}")
    lead = pts3d.shape[:pts3d.dim() - 3]
    if tuple(im_poses.shape) != (*lead, 4, 4) or tuple(intrinsics.shape) != (*lead, 3, 3):
        raise RuntimeError(f"reproj_loss: im_poses {tuple(im_poses.shape)} / intrinsics {tuple(intrinsics.shape)} do not "
                           f"match pts3d {tuple(pts3d.shape)} (want {(*lead, 4, 4)} / {(*lead, 3, 3)})")
    for name, t in (("pts3d", pts3d), ("im_poses", im_poses), ("intrinsics", intrinsics)):
        if not t.is_cuda:
            raise RuntimeError(f"reproj_loss: {name} is on {t.device}; this build only runs on a HIP device (no CPU "
                               "fallback)")
        if not t.is_floating_point():
            raise RuntimeError(f"reproj_loss: {name} must be a floating-point tensor, got {t.dtype}")
    if pts3d.numel() == 0:
        raise RuntimeError("reproj_loss: empty input")
    if detach_pts3d:
        pts3d = pts3d.detach()
    code = _REPROJ_MODES.get(mode, _REPROJ_LOG)
    lw = reproj_lw(mode, global_step, total_iterations, circle_schedule, soft_clamp, soft_clamp_min)
    pts3d, im_poses, intrinsics = (t if t.dtype == torch.float32 else t.float() for t in (pts3d, im_poses, intrinsics))
    return _Reproj.apply(pts3d, im_poses, intrinsics, code, float(weight), float(lw), float(hard_clamp),
                         float(soft_clamp))


@dataclass
class LossReprojCfg:
    weight: float
    mode: str
    circle_schedule: bool
    total_iterations: int


@dataclass
class LossReprojCfgWrapper:
    reproj: LossReprojCfg


class LossReproj(Loss[LossReprojCfg, LossReprojCfgWrapper]):
    """The clamps are instance attributes read at every call, as in the reference (loss_reproj.py:48-50)."""

    def __init__(self, cfg: LossReprojCfgWrapper) -> None:
        super().__init__(cfg)
        self.repro_loss_hard_clamp = 1000
        self.soft_clamp = 50
        self.soft_clamp_min = 1

    def forward(self, pts3d: Tensor, im_poses: Tensor, intrinsics: Tensor, global_step: int,
                detach_pts3d: bool = False) -> Tensor:
        """[b,h,w,3] -> 0-dim loss (the reference's call); [b,v,h,w,3] -> loss[v], one per view (see reproj_loss)."""
        return reproj_loss(pts3d, im_poses, intrinsics, weight=self.cfg.weight, mode=self.cfg.mode,
                           global_step=global_step, total_iterations=self.cfg.total_iterations,
                           circle_schedule=self.cfg.circle_schedule, detach_pts3d=detach_pts3d,
                           hard_clamp=self.repro_loss_hard_clamp, soft_clamp=self.soft_clamp,
                           soft_clamp_min=self.soft_clamp_min)


# ---- LPIPS loss --------------------------------------------------------------------------------------------------
@dataclass
class LossLpipsCfg:
    weight: float
    apply_after_step: int


@dataclass
class LossLpipsCfgWrapper:
    lpips: LossLpipsCfg


class LossLpips(Loss[LossLpipsCfg, LossLpipsCfgWrapper]):
    """The reference builds ``LPIPS(net="vgg")`` (which may download weights) in its constructor; here the weights come
    from `weights` or ``$SPF_LPIPS_WEIGHTS`` (spfsplatv2_amd.lpips.resolve_weights) and resolve on the first step that
    applies the loss, so constructing it needs no file.  The mean over the images and its backward are taken inside the
    library."""

    def __init__(self, cfg: LossLpipsCfgWrapper, weights=None) -> None:
        super().__init__(cfg)
        self.weights = weights

    def forward(self, prediction: Tensor, image: Tensor, gaussians, global_step: int) -> Tensor:
        if global_step < self.cfg.apply_after_step:           # not applied yet (loss_lpips.py:74-76)
            return torch.tensor(0, dtype=torch.float32, device=image.device)
        from .lpips import LpipsWeights, _check_pair, lpips_mean, resolve_weights
        if prediction.dim() != 5 or image.dim() != 5:
            raise ValueError(f"LossLpips: prediction and image must be [b,v,3,h,w], got {tuple(prediction.shape)} and "
                             f"{tuple(image.shape)}")
        pred, img = prediction.flatten(0, 1), image.flatten(0, 1)
        _check_pair("LossLpips", pred, img)
        if not isinstance(self.weights, LpipsWeights):
            self.weights = resolve_weights(self.weights)
        return lpips_mean(pred, img, self.weights, normalize=True, weight=self.cfg.weight)


# ---- distillation point loss ---------------------------------------------------------------------------------------
def _regr3d_rows(t: Tensor) -> Tensor:
    """A [B,H,W,3] operand the kernels can read in place: float32, every batch item's H*W*3 floats contiguous, a
    non-negative batch stride, 4-byte aligned.  The caller's ``means[:, i].squeeze(-2)`` views pass as they are."""
    if t.dtype != torch.float32:
        t = t.float()
    b, h, w, _ = t.shape
    ok = t.stride(3) == 1 and (w == 1 or t.stride(2) == 3) and (h == 1 or t.stride(1) == 3 * w) and \
        (b == 1 or t.stride(0) >= 0)
    return t if ok else t.contiguous()


def _regr3d_args(gt1, gt2, pr1, pr2, c1, c2, dist_clip, disable_view1, normalize, gt_scale):
    b, h, w, _ = gt1.shape
    ptr = _lib.ptr
    return _lib.SpfRegr3d(ptr(gt1), ptr(gt2), ptr(pr1), ptr(pr2), ptr(c1), ptr(c2), gt1.stride(0), gt2.stride(0),
                          pr1.stride(0), pr2.stride(0), b, h, w, int(dist_clip is not None),
                          float(dist_clip) if dist_clip is not None else 0.0, int(bool(disable_view1)),
                          int(bool(normalize)), int(bool(gt_scale)))


class _Regr3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt1: Tensor, gt2: Tensor, pr1: Tensor, pr2: Tensor, conf1, conf2, dist_clip, disable_view1: bool,
                normalize: bool, gt_scale: bool):
        gt1, gt2, pr1, pr2 = (_regr3d_rows(t) for t in (gt1, gt2, pr1, pr2))
        c1, c2 = ((None, None) if dist_clip is not None else
                  tuple(c.to(torch.float32).contiguous() for c in (conf1, conf2)))
        b, h, w, _ = gt1.shape
        dev = gt1.device
        args = _regr3d_args(gt1, gt2, pr1, pr2, c1, c2, dist_clip, disable_view1, normalize, gt_scale)
        nbytes = _lib.load().spf_regr3d_scratch_bytes(b, h, w)
        if nbytes < 0:
            raise RuntimeError(f"regr3d_loss: {b} x {h} x {w} points is not a supported size")
        scratch = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        stats = torch.empty(8 * b, dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.launch("spf_regr3d_forward", dev, args, scratch, stats, loss)
        ctx.save_for_backward(gt1, gt2, pr1, pr2, c1, c2, scratch, stats)
        ctx.params = (dist_clip, disable_view1, normalize, gt_scale)
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, grad, _grad_stats):
        gt1, gt2, pr1, pr2, c1, c2, scratch, stats = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        dev = gt1.device
        g = grad.to(torch.float32).reshape(1).contiguous()
        d1 = torch.empty(pr1.shape, dtype=torch.float32, device=dev) if need1 else None
        d2 = torch.empty(pr2.shape, dtype=torch.float32, device=dev) if need2 else None
        _lib.launch("spf_regr3d_backward", dev, _regr3d_args(gt1, gt2, pr1, pr2, c1, c2, *ctx.params), scratch, stats, g,
                    d1, d2)
        return None, None, d1, d2, None, None, None, None, None, None


def regr3d_loss(gt_pts1: Tensor, gt_pts2: Tensor, pr_pts1: Tensor, pr_pts2: Tensor, conf1: Tensor | None = None,
                conf2: Tensor | None = None, *, dist_clip: float | None = None, disable_view1: bool = False,
                norm_mode="avg_dis", gt_scale: bool = False, return_stats: bool = False):
    """``Regr3D(norm_mode, gt_scale=gt_scale)(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1, conf2, dist_clip,
    disable_view1)`` (loss_point.py:208-254) on the HIP library: point maps [B,H,W,3], confidences [B,H,W] -> a 0-dim
    float32 loss.  ``dist_clip is None``: a point is valid when its ground-truth norm lies within the row's 0.2 % and
    99.8 % quantiles (torch.quantile's definition, found by an exact radix select) and its confidence is >= 3;
    otherwise when the norm is <= dist_clip (the confidences are not read).  Predictions and ground truth are divided by
    their mean valid norm, jointly over the two views and per batch item (``norm_mode='avg_dis'``; falsy: not at all;
    ``gt_scale``: predictions only); the loss is the mean distance over all valid points of view 1 plus that of view 2
    (view 2 alone with ``disable_view1``).  A view without a valid point gives NaN, as the mean of nothing does in the
    reference, with finite gradients.

    Gradients flow to pr_pts1 and pr_pts2 only -- directly and through their normalisation factor -- and invalid points
    get exactly 0.  bf16 / f16 / f64 inputs are computed in float32 and their gradients cast back by autograd.  The
    predictions may be strided views of ``[b,v,h,w,1,3]`` (``means[:, i].squeeze(-2)``): they are read in place.
    Nothing synchronises the host.

    ``return_stats=True``: also a dict of device tensors -- ``n_valid`` [2,B] int32, ``q`` [2,B,2] (q_lo, q_hi; with
    dist_clip: 0, dist_clip), ``nf_pr`` [B], ``nf_gt`` [B]."""
    if norm_mode and norm_mode != "avg_dis":
        raise NotImplementedError(f"regr3d_loss: norm_mode {norm_mode!r} is not implemented (only 'avg_dis' or none)")
    pts = (("gt_pts1", gt_pts1), ("gt_pts2", gt_pts2), ("pr_pts1", pr_pts1), ("pr_pts2", pr_pts2))
    confs = (("conf1", conf1), ("conf2", conf2))
    if dist_clip is None and (conf1 is None or conf2 is None):
        raise ValueError("regr3d_loss: conf1 and conf2 are needed unless dist_clip is given")
    given = pts + tuple((n, c) for n, c in confs if c is not None)
    for name, t in given:
        if not isinstance(t, Tensor):
            raise TypeError(f"regr3d_loss: {name} must be a tensor")
    for name, t in given:
        if t.requires_grad and not name.startswith("pr_"):
            raise ValueError(f"regr3d_loss: {name} requires grad, but gradients flow to pr_pts1 and pr_pts2 only; "
                             "detach it")
    for name, t in given:
        if not t.is_cuda:
            raise RuntimeError(f"regr3d_loss: {name} is on {t.device}; this build only runs on a HIP device (no CPU "
                               "fallback)")
        if not t.is_floating_point():
            raise RuntimeError(f"regr3d_loss: {name} must be a floating-point tensor, got {t.dtype}")
    shape = tuple(gt_pts1.shape)
    if len(shape) != 4 or shape[-1] != 3 or gt_pts1.numel() == 0:
        raise RuntimeError(f"regr3d_loss: gt_pts1 must be a non-empty [B,H,W,3], got {shape}")
    for name, t in pts[1:]:
        if tuple(t.shape) != shape:
            raise RuntimeError(f"regr3d_loss: {name} {tuple(t.shape)} does not match gt_pts1 {shape}")
    for name, c in confs:
        if c is not None and dist_clip is None and tuple(c.shape) != shape[:3]:
            raise RuntimeError(f"regr3d_loss: {name} {tuple(c.shape)} does not match the point maps {shape[:3]}")
    if dist_clip is not None:
        dist_clip = float(dist_clip)
    # (cast here, not inside the function: autograd then casts the gradients back to the inputs' type)
    pr_pts1, pr_pts2 = (t if t.dtype == torch.float32 else t.float() for t in (pr_pts1, pr_pts2))
    loss, stats = _Regr3D.apply(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1, conf2, dist_clip, bool(disable_view1),
                                bool(norm_mode), bool(gt_scale))
    if not return_stats:
        return loss
    b = shape[0]
    return loss, {"n_valid": stats[:2 * b].view(torch.int32).view(2, b), "q": stats[2 * b:6 * b].view(2, b, 2),
                  "nf_pr": stats[6 * b:7 * b], "nf_gt": stats[7 * b:8 * b]}


class Regr3D(nn.Module):
    """The reference's ``Regr3D`` (loss_point.py:188-254), constructor and call signature: drops into
    model_wrapper.py:171 and :326.  ``alpha`` is kept as an attribute, as there; nothing reads it."""

    def __init__(self, norm_mode="avg_dis", alpha=0.2, gt_scale=False):
        super().__init__()
        if norm_mode and norm_mode != "avg_dis":
            raise NotImplementedError(f"Regr3D: norm_mode {norm_mode!r} is not implemented (only 'avg_dis' or none)")
        self.norm_mode = norm_mode
        self.alpha = alpha
        self.gt_scale = gt_scale

    def forward(self, gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1=None, conf2=None, dist_clip=None, disable_view1=False):
        return regr3d_loss(gt_pts1, gt_pts2, pr_pts1, pr_pts2, conf1, conf2, dist_clip=dist_clip,
                           disable_view1=disable_view1, norm_mode=self.norm_mode, gt_scale=self.gt_scale)
