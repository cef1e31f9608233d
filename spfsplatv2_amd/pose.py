"""The pose path on the HIP library: everything between the pose head's raw output and the decoder's ``extrinsics``, and the
pose numbers logged beside the loss (spfsplatv2_amd/csrc/pose.hip).  Nothing here synchronises the host.

=================================  ====================================================================================
here                               reference (/root/reference/src/)
=================================  ====================================================================================
``convert_pose_to_4x4``            misc/cam_utils.py:275-286 (pytorch3d's ``rotation_6d_to_matrix``)
``process_pose``                   model/encoder/encoder_spfsplatv2.py:340-359, encoder_spfsplat.py:342-361
                                   (``encoding="rot6d"``); encoder_spfsplatv2l.py:154,248-269 with
                                   ``pose_encoding_to_extri_intri`` (``encoding="absT_quaR_FoV"``)
``depth_projector``                misc/cam_utils.py:310-318
``process_depth``                  encoder_spfsplatv2.py:361-369
``compute_pose_error``             evaluation/metrics.py:87-99 -- the reference returns CPU tensors, these stay on the
                                   inputs' device
``compute_pose_error_for_batch``   evaluation/metrics.py:102-129 -- likewise (the reference: 2 b v ``.cpu()`` copies)
``pose_errors``                    ours: all three errors of every pose, [N, 3] (``test_step`` takes their ``torch.max``)
``pose_auc``                       misc/cam_utils.py:257-271 (host numpy, with or without ``numpy.trapz``)
``estimate_focal_knowing_depth``   misc/intrinsics_utils.py:33-108, ``focal_mode="weiszfeld"``
``estimate_intrinsics``            misc/intrinsics_utils.py:162-174
=================================  ====================================================================================

``process_pose``, ``convert_pose_to_4x4`` and ``depth_projector`` are autograd functions, differentiable in every tensor
argument; any floating dtype and any strides are accepted, the arithmetic is float32 in and out (float64 inside for the
inverses) and pose outputs are float32, as the reference's ``torch.zeros`` makes them.  The error and focal functions run
under ``no_grad`` and return float32 tensors on the input's device.  CPU tensors raise: there is no CPU fallback.

What the reference really does, mirrored here:

* ``estimate_intrinsics`` uses view 0 of each scene only.
* It calls ``normalize_intrinsics(K, height, width)`` against a signature of ``(K, width, height)``: row 0 is divided by
  ``height`` and row 1 by ``width``.  On 24 x 32: ``fx = f/24, cx = 16/24, fy = f/32, cy = 12/32``.
* ``estimate_focal_knowing_depth`` with ``B > 1`` returns ONE FOCAL PER SCENE here -- what ``estimate_intrinsics``' loop
  over scenes yields.  The reference's boolean-mask compaction pools the points of all scenes into a single focal in
  that case; nothing in the reference calls it so.
* pose errors are evaluated in float64 and rounded at the store; the reference's float32 ``acos`` loses up to 0.03
  degrees near 0 and 180.

``get_pnp_pose`` and ``get_pnp_pose_batch`` (misc/cam_utils.py:162-253, cv2 RANSAC in the reference) are served by
``pnp.py``: P3P RANSAC and refinement on the device.

Out of scope: ``update_pose`` / ``SE3_exp``, ``camera_normalization``, and the trivial
``convert_focal_to_intrinsics`` / ``normalize_intrinsics`` helpers; ``focal_mode="median"`` raises.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import Tensor

from . import _lib

ENCODINGS = {"rot6d": 0, "absT_quaR_FoV": 1}


def _check(name: str, what: str, t) -> None:
    if not isinstance(t, Tensor):
        raise TypeError(f"{name}: {what} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: {what} is on {t.device}; this build only runs on a HIP device (no CPU fallback)")
    if not t.is_floating_point():
        raise RuntimeError(f"{name}: {what} must be a floating-point tensor, got {t.dtype}")
    if t.numel() == 0:
        raise RuntimeError(f"{name}: {what} is empty ({tuple(t.shape)})")


def _f32(t: Tensor) -> Tensor:
    # (cast outside the autograd functions: autograd then casts the gradients back to the inputs' type)
    return t if t.dtype == torch.float32 else t.float()


# ---- composition -----------------------------------------------------------------------------------------------------
class _ComposePose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, enc: Tensor, context_views: int, encoding: int, baseline: bool, relative: bool):
        b, v, _ = enc.shape
        if enc.stride(2) != 1:                       # a view's nine floats must be contiguous; b and v strides are free
            enc = enc.contiguous()
        dev = enc.device
        poses = torch.empty(b, v, 4, 4, dtype=torch.float32, device=dev)
        _lib.launch("spf_pose_compose_forward", dev, enc, enc.stride(0), enc.stride(1), b, v, context_views, encoding,
                    int(baseline), int(relative), poses)
        ctx.save_for_backward(enc)
        ctx.params = (context_views, encoding, baseline, relative)
        return poses

    @staticmethod
    def backward(ctx, grad: Tensor):
        (enc,) = ctx.saved_tensors
        b, v, _ = enc.shape
        dev = enc.device
        g = grad.to(torch.float32).contiguous()
        denc = torch.empty(b, v, 9, dtype=torch.float32, device=dev)
        context_views, encoding, baseline, relative = ctx.params
        _lib.launch("spf_pose_compose_backward", dev, enc, enc.stride(0), enc.stride(1), b, v, context_views, encoding,
                    int(baseline), int(relative), g, denc)
        return denc, None, None, None, None


def process_pose(pose_enc: Tensor, context_views: int, *, encoding: str = "rot6d", pose_make_baseline_1: bool,
                 pose_make_relative: bool) -> Tensor:
    """``pose_enc`` [b, v, 9] -> camera -> world poses [b, v, 4, 4] (float32, bottom rows exactly 0 0 0 1).

    ``encoding="rot6d"``: columns 0:6 are two 3-vectors, orthonormalised into the ROWS of R, columns 6:9 the translation.
    ``encoding="absT_quaR_FoV"``: columns 0:3 the world -> camera translation, 3:7 a scalar-last quaternion that need not
    be normalised, 7:9 ignored (zero gradient); the pose is the closed-form inverse.  ``pose_make_baseline_1`` divides all
    of a scene's translations by ``|t_0 - t_{context_views-1}|`` (``context_views=1`` divides by zero, as in the
    reference); ``pose_make_relative`` left-multiplies every view by the general inverse of view 0.  A ``[..., :9]`` slice
    of a wider head output is read in place."""
    if not isinstance(pose_enc, Tensor) or pose_enc.dim() != 3 or pose_enc.shape[-1] != 9:
        raise RuntimeError(f"process_pose: pose_enc must be a [b, v, 9] tensor, got "
                           f"{tuple(pose_enc.shape) if isinstance(pose_enc, Tensor) else type(pose_enc)}")
    if encoding not in ENCODINGS:
        raise ValueError(f"process_pose: unknown encoding {encoding!r} (one of {sorted(ENCODINGS)})")
    context_views = int(context_views)
    if not 1 <= context_views <= pose_enc.shape[1]:
        raise ValueError(f"process_pose: context_views {context_views} is outside 1..{pose_enc.shape[1]}")
    _check("process_pose", "pose_enc", pose_enc)
    return _ComposePose.apply(_f32(pose_enc), context_views, ENCODINGS[encoding], bool(pose_make_baseline_1),
                              bool(pose_make_relative))


def convert_pose_to_4x4(out: Tensor) -> Tensor:
    """``out`` [B, 9] (6-D rotation, translation) -> camera -> world poses [B, 4, 4] (float32)."""
    _check("convert_pose_to_4x4", "out", out)
    if out.dim() != 2 or out.shape[-1] != 9:
        raise RuntimeError(f"convert_pose_to_4x4: out must be [B, 9], got {tuple(out.shape)}")
    return _ComposePose.apply(_f32(out).unsqueeze(1), 1, ENCODINGS["rot6d"], False, False)[:, 0]


# ---- depth -----------------------------------------------------------------------------------------------------------
class _DepthProject(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pts: Tensor, poses: Tensor):
        N, n, _ = pts.shape
        if pts.stride(2) != 1 or (n > 1 and pts.stride(1) != 3):       # an image's 3 n floats must be contiguous
            pts = pts.contiguous()
        poses = poses.contiguous()
        dev = pts.device
        depth = torch.empty(N, n, 1, dtype=torch.float32, device=dev)
        _lib.launch("spf_depth_project_forward", dev, pts, pts.stride(0), poses, N, n, depth)
        ctx.save_for_backward(pts, poses)
        return depth

    @staticmethod
    def backward(ctx, grad: Tensor):
        pts, poses = ctx.saved_tensors
        N, n, _ = pts.shape
        dev = pts.device
        g = grad.to(torch.float32).contiguous()
        need_pts, need_poses = ctx.needs_input_grad
        dpts = torch.empty(N, n, 3, dtype=torch.float32, device=dev) if need_pts else None
        dposes = gpartial = None
        if need_poses:
            dposes = torch.empty(N, 4, 4, dtype=torch.float32, device=dev)
            gpartial = torch.empty(_lib.load().spf_depth_project_partial_blocks(N, n), 4, dtype=torch.float32, device=dev)
        _lib.launch("spf_depth_project_backward", dev, pts, pts.stride(0), poses, N, n, g, dpts, gpartial, dposes)
        return dpts, dposes


def depth_projector(pts3d: Tensor, im_poses: Tensor) -> Tensor:
    """``pts3d`` [N, n, 3], camera -> world ``im_poses`` [N, 4, 4] -> the points' depth in each camera, [N, n, 1]
    (float32): ``(inverse(pose) [p, 1])_z`` with a general float64 inverse.  ``pts3d`` may be a strided view whose images
    are contiguous (any image stride, any 4-byte alignment): it is read in place."""
    _check("depth_projector", "pts3d", pts3d)
    _check("depth_projector", "im_poses", im_poses)
    if pts3d.dim() != 3 or pts3d.shape[-1] != 3:
        raise RuntimeError(f"depth_projector: pts3d must be [N, n, 3], got {tuple(pts3d.shape)}")
    if tuple(im_poses.shape) != (pts3d.shape[0], 4, 4):
        raise RuntimeError(f"depth_projector: im_poses must be [{pts3d.shape[0]}, 4, 4], got {tuple(im_poses.shape)}")
    if im_poses.device != pts3d.device:
        raise RuntimeError("depth_projector: pts3d and im_poses are on different devices")
    return _DepthProject.apply(_f32(pts3d), _f32(im_poses))


def process_depth(pose: Tensor, pts3d: Tensor) -> Tensor:
    """``pose`` [b, v, 4, 4], ``pts3d`` [b, v, h, w, 3] -> depth of every point in its own camera, [b, v, h, w]."""
    if not isinstance(pts3d, Tensor) or pts3d.dim() != 5 or pts3d.shape[-1] != 3:
        raise RuntimeError("process_depth: pts3d must be [b, v, h, w, 3]")
    b, v, h, w, _ = pts3d.shape
    if not isinstance(pose, Tensor) or tuple(pose.shape) != (b, v, 4, 4):
        raise RuntimeError(f"process_depth: pose must be [{b}, {v}, 4, 4]")
    return depth_projector(pts3d.reshape(b * v, h * w, 3), pose.reshape(b * v, 4, 4)).reshape(b, v, h, w)


# ---- errors ----------------------------------------------------------------------------------------------------------
def _pose_error_launch(name: str, pred: Tensor, tgt: Tensor):
    _check(name, "the predicted pose", pred)
    _check(name, "the target pose", tgt)
    if pred.shape != tgt.shape or pred.dim() < 2 or tuple(pred.shape[-2:]) != (4, 4):
        raise RuntimeError(f"{name}: poses must be two [..., 4, 4] tensors of one shape, got {tuple(pred.shape)} and "
                           f"{tuple(tgt.shape)}")
    if pred.device != tgt.device:
        raise RuntimeError(f"{name}: the poses are on different devices")
    p = pred.detach().to(torch.float32).reshape(-1, 4, 4).contiguous()
    t = tgt.detach().to(torch.float32).reshape(-1, 4, 4).contiguous()
    N = p.shape[0]
    dev = p.device
    errors = torch.empty(N, 3, dtype=torch.float32, device=dev)
    means = torch.empty(3, dtype=torch.float32, device=dev)
    _lib.launch("spf_pose_error", dev, p, t, N, errors, means)
    return errors, means


@torch.no_grad()
def pose_errors(pred: Tensor, tgt: Tensor) -> Tensor:
    """[..., 4, 4] x 2 -> [N, 3]: ``(error_t, error_t_scale, error_R)`` of every pose, in degrees / scene units."""
    return _pose_error_launch("pose_errors", pred, tgt)[0]


@torch.no_grad()
def compute_pose_error(pose_gt: Tensor, pose_pred: Tensor):
    """Two [4, 4] poses -> ``(error_t, error_t_scale, error_R)`` as 0-dim device tensors."""
    if not isinstance(pose_gt, Tensor) or pose_gt.dim() != 2:
        raise RuntimeError("compute_pose_error: poses must be [4, 4]")
    e = _pose_error_launch("compute_pose_error", pose_pred, pose_gt)[0][0]
    return e[0], e[1], e[2]


@torch.no_grad()
def compute_pose_error_for_batch(pred_pose: Tensor, tgt_pose: Tensor):
    """[b, v, 4, 4], [b, 4, 4] or [4, 4] x 2 -> ``(mean error_R, mean error_t)`` as 0-dim device tensors, one launch."""
    means = _pose_error_launch("compute_pose_error_for_batch", pred_pose, tgt_pose)[1]
    return means[2], means[0]


def pose_auc(errors, thresholds):
    """Area under the recall-over-error curve up to each threshold, divided by it (host numpy)."""
    if isinstance(errors, Tensor):
        errors = errors.detach().cpu().numpy()
    errors = np.sort(np.asarray(errors, dtype=np.float64).ravel())
    recall = (np.arange(len(errors)) + 1) / len(errors)
    errors = np.r_[0.0, errors]
    recall = np.r_[0.0, recall]
    aucs = []
    for t in thresholds:
        last = np.searchsorted(errors, t)
        r = np.r_[recall[:last], recall[last - 1]]
        e = np.r_[errors[:last], t]
        aucs.append(float(np.sum(np.diff(e) * (r[1:] + r[:-1]) / 2.0) / t))      # the trapezoid rule, written out
    return aucs


# ---- focal -----------------------------------------------------------------------------------------------------------
def _focal_launch(name: str, pts: Tensor, pp, min_focal: float, max_focal: float, intr):
    """pts [B, H, W, 3] (rows contiguous, read in place) -> focal [B] and, with intr = (height, width), the [B, 3, 3]."""
    _check(name, "pts3d", pts)
    pts = pts.detach()
    if pts.dtype != torch.float32:
        pts = pts.float()
    B, H, W, _ = pts.shape
    if pts.stride(3) != 1 or (W > 1 and pts.stride(2) != 3):         # a row's 3 W floats must be contiguous
        pts = pts.contiguous()
    dev = pts.device
    pp_stride = 0
    if pp is not None:
        _check(name, "pp", pp)
        if pp.device != dev or pp.numel() not in (2, 2 * B) or pp.shape[-1] != 2:
            raise RuntimeError(f"{name}: pp must hold one (x, y) pair, or one per scene, on {dev}; got "
                               f"{tuple(pp.shape)} on {pp.device}")
        pp = pp.detach().to(torch.float32).reshape(-1, 2).contiguous()
        pp_stride = 2 if pp.shape[0] == B and B > 1 else 0
    if _lib.load().spf_focal_scratch_bytes(B, H, W) < 0:
        raise RuntimeError(f"{name}: {B} x {H} x {W} points is not a supported size")
    focal = torch.empty(B, dtype=torch.float32, device=dev)
    K = torch.empty(B, 3, 3, dtype=torch.float32, device=dev) if intr is not None else None
    height, width = intr if intr is not None else (1, 1)
    _lib.launch("spf_focal_estimate", dev, pts, pts.stride(0), pts.stride(1), B, H, W, pp, pp_stride, float(min_focal),
                float(max_focal), width / 2.0, height / 2.0, float(height), float(width), None, focal, K)
    return focal, K


@torch.no_grad()
def estimate_focal_knowing_depth(pts3d: Tensor, pp: Tensor | None = None, focal_mode: str = "weiszfeld",
                                 min_focal: float = 0.0, max_focal: float = math.inf) -> Tensor:
    """``pts3d`` [B, H, W, 3] -> [B] focal lengths in pixels, ONE PER SCENE (see the module's notes), by the Weiszfeld
    iteration over the points with ``z > 0``; ``pp`` (a device tensor, [2] or [B, 2]) defaults to ``(W/2, H/2)``.  A scene
    without a valid point gives NaN."""
    if focal_mode != "weiszfeld":
        if focal_mode == "median":
            raise NotImplementedError("estimate_focal_knowing_depth: focal_mode='median' is not implemented")
        raise ValueError(f"bad focal_mode={focal_mode!r}")
    if not isinstance(pts3d, Tensor) or pts3d.dim() != 4 or pts3d.shape[-1] != 3:
        raise RuntimeError("estimate_focal_knowing_depth: pts3d must be [B, H, W, 3]")
    return _focal_launch("estimate_focal_knowing_depth", pts3d, pp, min_focal, max_focal, None)[0]


@torch.no_grad()
def estimate_intrinsics(pts3d: Tensor, height: int, width: int) -> Tensor:
    """``pts3d`` [b, v, h, w, 3] -> normalised intrinsics [b, 3, 3] from the focal of VIEW 0 of each scene (read in place),
    with the reference's row divisors: row 0 by ``height``, row 1 by ``width``."""
    if not isinstance(pts3d, Tensor) or pts3d.dim() != 5 or pts3d.shape[-1] != 3:
        raise RuntimeError("estimate_intrinsics: pts3d must be [b, v, h, w, 3]")
    return _focal_launch("estimate_intrinsics", pts3d[:, 0], None, 0.0, math.inf, (height, width))[1]
