"""PnP pose from point maps on the HIP library: P3P RANSAC and Gauss-Newton refinement (spfsplatv2_amd/csrc/pnp.hip).

=======================  ==============================================================================================
here                     reference (src/)
=======================  ==============================================================================================
``get_pnp_pose``         misc/cam_utils.py:162-215 -- the reference returns a CPU tensor, this stays on the inputs' device
``get_pnp_pose_batch``   misc/cam_utils.py:218-253 -- likewise (the reference: a Python double loop over ``b`` and ``v``)
``pnp_poses``            ours: the poses with their inlier counts, candidate counts, winning hypotheses and success flags
=======================  ==============================================================================================

All views of a call go through four launches; nothing here synchronises the host, and reading a result is the caller's
synchronisation.  The functions run under ``no_grad``, accept any floating dtype (cast to float32 once) and any strides
whose last dimension of ``pts3d`` is contiguous (a ``[b, v, h, w, 1, 3]`` dump squeezed or a ``[:, -1]`` slice is read in
place), and raise on CPU tensors: there is no CPU fallback.  The workspace comes from the caching allocator per call.

What is mirrored from the reference: pixel ``(row i, column j)`` is the image point ``(x, y) = (j, i)`` without a
half-pixel offset; ``K`` is normalised (row 0 times ``W``, row 1 times ``H``); the candidates are the pixels with
``opacity > opacity_threshold``; the result is the camera -> world pose in float32, ``eye(4)`` on failure.
``initial_pose`` raises ``NotImplementedError``: nothing in the reference passes it.

What is NOT claimed is equality with OpenCV's numbers: the definition is DESIGN.md 7s, restated in ``tests/pnp_oracle.py``
(128 hypotheses from a counter-based hash, Grunert's P3P, inlier counts at 5 px, ten Gauss-Newton steps on the inliers of
the current pose).  A result is bitwise reproducible and a view's pose does not depend on what else is in the call.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import Tensor

from . import _lib


class PnPResult(NamedTuple):
    poses: Tensor         # [b, v, 4, 4] float32, camera -> world; eye(4) where the view failed
    inliers: Tensor       # [b, v] int32: inliers of the final pose (0 on failure)
    candidates: Tensor    # [b, v] int32: pixels with opacity > threshold and finite coordinates
    hypothesis: Tensor    # [b, v] int32: the winning hypothesis (-1 on failure)
    success: Tensor       # [b, v] int32: 1 or 0


def _solve(name: str, pts3d, opacity, K, H, W, opacity_threshold, iterations, reprojection_error, refine_steps, seed,
           with_ranks: bool = False):
    for what, t in (("pts3d", pts3d), ("opacity", opacity), ("K", K)):
        if not isinstance(t, Tensor):
            raise TypeError(f"{name}: {what} must be a tensor")
        if not t.is_floating_point():
            raise RuntimeError(f"{name}: {what} must be a floating-point tensor, got {t.dtype}")
    if pts3d.dim() != 5 or pts3d.shape[-1] != 3 or 0 in pts3d.shape:
        raise RuntimeError(f"{name}: pts3d must be a non-empty [b, v, h, w, 3] tensor, got {tuple(pts3d.shape)}")
    b, v, h, w, _ = pts3d.shape
    if tuple(opacity.shape) != (b, v, h, w):
        raise RuntimeError(f"{name}: opacity must be [{b}, {v}, {h}, {w}], got {tuple(opacity.shape)}")
    if tuple(K.shape) != (b, v, 3, 3):
        raise RuntimeError(f"{name}: K must be [{b}, {v}, 3, 3], got {tuple(K.shape)}")
    if (int(H), int(W)) != (h, w):
        raise RuntimeError(f"{name}: H, W = {H}, {W} differ from the point map's {h} x {w}")
    iterations, refine_steps, seed = int(iterations), int(refine_steps), int(seed)
    if iterations % 64 != 0 or not 64 <= iterations <= 1024:
        raise ValueError(f"{name}: iterations must be a multiple of 64 in 64..1024, got {iterations}")
    if not 0 <= refine_steps <= 64:
        raise ValueError(f"{name}: refine_steps must be in 0..64, got {refine_steps}")
    if not float(reprojection_error) > 0.0:
        raise ValueError(f"{name}: reprojection_error must be positive, got {reprojection_error}")
    if not 0 <= seed < 2 ** 32:
        raise ValueError(f"{name}: seed must fit 32 bits, got {seed}")
    for what, t in (("pts3d", pts3d), ("opacity", opacity), ("K", K)):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: {what} is on {t.device}; this build only runs on a HIP device (no CPU fallback)")
    dev = pts3d.device
    if opacity.device != dev or K.device != dev:
        raise RuntimeError(f"{name}: pts3d, opacity and K are on different devices")
    nbytes = _lib.load().spf_pnp_workspace_bytes(b * v, h, w, iterations)
    if nbytes < 0:
        raise RuntimeError(f"{name}: {b} x {v} views of {h} x {w} pixels is not a supported size")
    pts = pts3d.detach()
    pts = pts if pts.dtype == torch.float32 else pts.float()
    if pts.stride(4) != 1 or min(pts.stride()) < 0:             # only a pixel's three floats must be contiguous
        pts = pts.contiguous()
    opa = opacity.detach()
    opa = opa if opa.dtype == torch.float32 else opa.float()
    Kc = K.detach().to(torch.float32).contiguous()
    args = _lib.SpfPnp(_lib.ptr(pts), _lib.ptr(opa), _lib.ptr(Kc), (_lib.C.c_int64 * 4)(*pts.stride()[:4]),
                       (_lib.C.c_int64 * 4)(*opa.stride()), b, v, h, w, iterations, refine_steps, seed,
                       float(opacity_threshold), float(reprojection_error), 0)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    poses = torch.empty(b, v, 4, 4, dtype=torch.float32, device=dev)
    info = torch.empty(4, b, v, dtype=torch.int32, device=dev)
    ranks = torch.empty(b, v, iterations, 4, dtype=torch.int32, device=dev) if with_ranks else None
    _lib.launch("spf_pnp_solve", dev, args, workspace, poses, info, ranks)
    return PnPResult(poses, info[0], info[1], info[2], info[3]), ranks


@torch.no_grad()
def pnp_poses(pts3d: Tensor, opacity: Tensor, K: Tensor, H: int, W: int, *, opacity_threshold: float = 0.3,
              iterations: int = 128, reprojection_error: float = 5.0, refine_steps: int = 10, seed: int = 0) -> PnPResult:
    """``pts3d`` [b, v, h, w, 3], ``opacity`` [b, v, h, w], normalised ``K`` [b, v, 3, 3] -> ``PnPResult`` of device
    tensors ([b, v, 4, 4] and four [b, v] int32).  ``H, W`` must be the map's ``h, w``; ``iterations`` a multiple of 64
    in 64..1024.  A view with fewer than 4 candidates or 4 inliers fails: ``eye(4)``, ``success = 0``, ``inliers = 0``.
    No host synchronisation: reading a field is the caller's."""
    return _solve("pnp_poses", pts3d, opacity, K, H, W, opacity_threshold, iterations, reprojection_error, refine_steps,
                  seed)[0]


@torch.no_grad()
def get_pnp_pose_batch(pts3d: Tensor, opacity: Tensor, K: Tensor, H: int, W: int, opacity_threshold: float = 0.3) -> Tensor:
    """[b, v, h, w, 3], [b, v, h, w], [b, v, 3, 3] -> camera -> world poses [b, v, 4, 4], float32, ON THE INPUTS' DEVICE
    (the reference returns a CPU tensor); ``eye(4)`` for a view that fails.  One call, four launches, no host sync."""
    return _solve("get_pnp_pose_batch", pts3d, opacity, K, H, W, opacity_threshold, 128, 5.0, 10, 0)[0].poses


@torch.no_grad()
def get_pnp_pose(pts3d: Tensor, opacity: Tensor, K: Tensor, H: int, W: int, opacity_threshold: float = 0.3,
                 initial_pose=None) -> Tensor:
    """[h, w, 3], [h, w], [3, 3] -> the camera -> world pose [4, 4], float32, ON THE INPUTS' DEVICE (the reference
    returns a CPU tensor); ``eye(4)`` on failure.  ``initial_pose`` is not supported."""
    if initial_pose is not None:
        raise NotImplementedError("get_pnp_pose: initial_pose is not supported (nothing in the reference passes it)")
    for what, t, d in (("pts3d", pts3d, 3), ("opacity", opacity, 2), ("K", K, 2)):
        if not isinstance(t, Tensor) or t.dim() != d:
            raise RuntimeError(f"get_pnp_pose: {what} must be a {d}-dimensional tensor")
    return _solve("get_pnp_pose", pts3d[None, None], opacity[None, None], K[None, None], H, W, opacity_threshold, 128,
                  5.0, 10, 0)[0].poses[0, 0]
