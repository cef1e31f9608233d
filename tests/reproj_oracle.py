"""Float64 restatement of the reprojection loss (the contract of spfsplatv2_amd.loss.reproj_loss), and the synthetic
inputs its tests use.  Written from the contract, not from the reference's code:

    W = inverse(pose) (general 4x4); cam = W[:3,:3] p + W[:3,3]; K' = K with row 0 * w and row 1 * h;
    q = K' cam; px = q.xy / max(q.z, 1e-6); e = |px - (j, i)| for point n = i w + j;
    valid = !(e > hard_clamp); loss = weight * sum_valid term(e) / n_valid (0 when none).

Gradients come from autograd in float64, which follows torch's rules by construction: zero at e = 0 (vector_norm),
none through z where q.z < 1e-6 with the gradient passing at equality (clamp), none for invalid points (where).
The clamp threshold is 1e-6 ROUNDED TO FLOAT32: the product clamps float32 tensors, where torch casts the scalar to
the tensor's type, and a point built at exactly that depth must fall on the same side here."""
from __future__ import annotations

import math

import torch

Z_MIN = float(torch.tensor(1e-6, dtype=torch.float32))


def term(e: torch.Tensor, mode: str, lw: float, soft: float) -> torch.Tensor:
    """term(e) of each mode; for e > soft in the l1 family the branch value is evaluated at a safe argument so that
    the unselected side of `where` never produces a NaN gradient."""
    if mode in ("tanh", "dyntanh"):
        return lw * torch.tanh(e / lw)
    small = ~(e > soft)
    l1 = torch.where(small, e, torch.zeros_like(e))
    if mode == "l1":
        return l1
    big_e = torch.where(small, torch.full_like(e, soft + 1.0), e)
    extra = torch.sqrt(soft * big_e) if mode == "l1+sqrt" else torch.log(1 + soft * big_e)
    return l1 + torch.where(small, torch.zeros_like(e), extra)


def lw_of(mode: str, step, total, circle: bool, soft: float, soft_min: float) -> float:
    if mode == "tanh":
        return soft
    if mode != "dyntanh":
        return 1.0
    s = step / total
    if circle:
        r = 1 - s * s
        s = 1 - math.sqrt(r) if r >= 0 else math.nan
    return (1 - s) * soft + soft_min


def errors(pts3d: torch.Tensor, poses: torch.Tensor, intrinsics: torch.Tensor) -> torch.Tensor:
    """e [b,h,w] for pts3d [b,h,w,3], poses [b,4,4], intrinsics [b,3,3] (any float dtype; autograd-able)."""
    b, h, w, _ = pts3d.shape
    W = torch.linalg.inv(poses)
    cam = torch.einsum("bij,bhwj->bhwi", W[:, :3, :3], pts3d) + W[:, None, None, :3, 3]
    scale = torch.tensor([w, h, 1.0], dtype=pts3d.dtype)[:, None]
    q = torch.einsum("bij,bhwj->bhwi", intrinsics * scale, cam)
    z = torch.clamp(q[..., 2:], min=Z_MIN)
    px = q[..., :2] / z
    ii, jj = torch.meshgrid(torch.arange(h, dtype=pts3d.dtype), torch.arange(w, dtype=pts3d.dtype), indexing="ij")
    target = torch.stack([jj, ii], dim=-1)
    return torch.linalg.vector_norm(px - target, dim=-1)


def reproj_ref(pts3d, poses, intrinsics, *, weight, mode, global_step, total_iterations, circle_schedule,
               detach_pts3d=False, hard_clamp=1000.0, soft_clamp=50.0, soft_clamp_min=1.0):
    """(loss, dL/dpts3d, dL/dposes, dL/dintrinsics, e) in float64 for one [b,h,w,3] call (dL/dpts3d is zero with
    detach_pts3d)."""
    p = pts3d.detach().double().requires_grad_(not detach_pts3d)
    po = poses.detach().double().requires_grad_(True)
    k = intrinsics.detach().double().requires_grad_(True)
    e = errors(p, po, k)
    valid = ~(e > hard_clamp)
    lw = lw_of(mode, global_step, total_iterations, circle_schedule, soft_clamp, soft_clamp_min)
    safe = torch.where(valid, e, torch.zeros_like(e))
    s = torch.where(valid, term(safe, mode, lw, soft_clamp), torch.zeros_like(e)).sum()
    n = int(valid.sum())
    loss = weight * s / n if n > 0 else s * 0.0
    leaves = [po, k] if detach_pts3d else [p, po, k]
    grads = torch.autograd.grad(loss, leaves, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, leaves)]
    if detach_pts3d:
        grads = [torch.zeros_like(p)] + grads
    return loss.detach(), grads[0], grads[1], grads[2], e.detach()


def knife_edge(e: torch.Tensor, soft_clamp: float = 50.0, hard_clamp: float = 1000.0) -> torch.Tensor:
    """Points whose float64 error sits where float32 rounding can flip a branch: within 1e-3 px of 0 (the norm's
    direction), or within 1e-5 relative of soft_clamp or hard_clamp."""
    return (e.abs() < 1e-3) | ((e - soft_clamp).abs() < 1e-5 * soft_clamp) | ((e - hard_clamp).abs() < 1e-5 * hard_clamp)


# ---- synthetic inputs ------------------------------------------------------------------------------------------

def general_pose(gen: torch.Generator, baseline: float = 1.0, shear: float = 0.05) -> torch.Tensor:
    """Camera -> world: a small rotation times (I + shear * noise) -- deliberately not rigid -- and a translation."""
    a = torch.randn(3, generator=gen) * 0.1
    kx = torch.tensor([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]], dtype=torch.float64)
    r = torch.linalg.matrix_exp(kx) @ (torch.eye(3, dtype=torch.float64)
                                       + shear * torch.randn(3, 3, generator=gen, dtype=torch.float64))
    p = torch.eye(4, dtype=torch.float64)
    p[:3, :3] = r
    p[:3, 3] = torch.randn(3, generator=gen, dtype=torch.float64) * baseline
    return p


def skewed_intrinsics(gen: torch.Generator) -> torch.Tensor:
    k = torch.eye(3, dtype=torch.float64)
    k[0, 0] = 0.8 + 0.2 * float(torch.rand(1, generator=gen))
    k[1, 1] = 0.9 + 0.2 * float(torch.rand(1, generator=gen))
    k[0, 1] = 0.03
    k[0, 2] = 0.5 + 0.02 * float(torch.randn(1, generator=gen))
    k[1, 2] = 0.5 + 0.02 * float(torch.randn(1, generator=gen))
    return k


def unproject(pose: torch.Tensor, k: torch.Tensor, h: int, w: int, offset: torch.Tensor, depth: torch.Tensor):
    """World points [h,w,3] (float64) that project to pixel (j, i) + offset[h,w,2] at camera-space q.z = depth[h,w]
    through `pose` and normalised `k`."""
    ii, jj = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    kp = k * torch.tensor([w, h, 1.0], dtype=torch.float64)[:, None]
    uv1 = torch.stack([jj + offset[..., 0], ii + offset[..., 1], torch.ones_like(ii)], dim=-1)
    cam = depth[..., None] * (uv1 @ torch.linalg.inv(kp).T)
    return cam @ pose[:3, :3].T + pose[:3, 3]


def pixel_aligned(gen: torch.Generator, b: int, h: int, w: int, noise_px: float = 3.0):
    """What an encoder's pts3d looks like against its own cameras: each pixel centre unprojected at a random depth
    (1 .. 20) through a random small pose and skewed intrinsics, plus pixel noise.  float32 [b,h,w,3], [b,4,4],
    [b,3,3]."""
    pts, poses, ks = [], [], []
    for _ in range(b):
        pose, k = general_pose(gen, 0.5, 0.02), skewed_intrinsics(gen)
        off = 0.5 + noise_px * torch.randn(h, w, 2, generator=gen, dtype=torch.float64)
        depth = torch.exp(torch.rand(h, w, generator=gen, dtype=torch.float64) * math.log(20.0))
        pts.append(unproject(pose, k, h, w, off, depth))
        poses.append(pose)
        ks.append(k)
    return torch.stack(pts).float(), torch.stack(poses).float(), torch.stack(ks).float()


def controlled_points(gen: torch.Generator, b: int, h: int, w: int, kind: str):
    """pts3d [b,h,w,3], poses [b,4,4] (general), intrinsics [b,3,3] (skewed), float32, whose errors are set by
    construction: each pixel (j, i) is unprojected at a random depth (0.5 .. 10.5) from (j, i) + an offset of a chosen
    length in a random direction.
      "mixed"        lengths from four bands: 0 - 8 px, 35 - 65 px (around soft_clamp), 900 - 1100 px (around
                     hard_clamp) and 3000 - 5000 px (invalid)
      "small"        0 - 4 px
      "none_valid"   1500 - 2000 px: no valid point
      "depth_edges"  "mixed", but in image 0 (identity pose: W is exact, so camera depths survive the round trip)
                     row 0 lies behind the camera (clamped, far off: invalid), row 1 at camera depth float32(1e-6)
                     exactly (the clamp's gradient passes at equality) and row 2 at half of it (clamped: no gradient
                     through z).  Their gradients are ~1e6 those of the other points, so they get cases of their own."""
    pts, poses, ks = [], [], []
    for bi in range(b):
        pose, k = general_pose(gen, 1.0, 0.05), skewed_intrinsics(gen)
        depth = 0.5 + 10.0 * torch.rand(h, w, generator=gen, dtype=torch.float64)
        ang = 2 * math.pi * torch.rand(h, w, generator=gen, dtype=torch.float64)
        if kind in ("mixed", "depth_edges"):
            band = torch.randint(0, 4, (h, w), generator=gen)
            lo = torch.tensor([0.0, 35.0, 900.0, 3000.0], dtype=torch.float64)[band]
            hi = torch.tensor([8.0, 65.0, 1100.0, 5000.0], dtype=torch.float64)[band]
            mag = lo + (hi - lo) * torch.rand(h, w, generator=gen, dtype=torch.float64)
        elif kind == "small":
            mag = 4.0 * torch.rand(h, w, generator=gen, dtype=torch.float64)
        elif kind == "none_valid":
            mag = 1500.0 + 500.0 * torch.rand(h, w, generator=gen, dtype=torch.float64)
        else:
            raise ValueError(kind)
        off = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], dim=-1)
        edges = kind == "depth_edges" and bi == 0
        if edges:
            depth[0, :] = -1.0 - depth[0, :]
            pose = torch.eye(4, dtype=torch.float64)
            depth[1, :] = Z_MIN
            depth[2, :] = 0.5 * Z_MIN
            off[1:3] = 0.25 * off[1:3].clamp(-8.0, 8.0)
        p = unproject(pose, k, h, w, off, depth)
        if edges:
            # the depth rows by hand so that float32 keeps q.z exactly (K' row 2 is [0, 0, 1], W = I)
            p[1:3, :, 2] = depth[1:3].float().double()
        pts.append(p)
        poses.append(pose)
        ks.append(k)
    return torch.stack(pts).float(), torch.stack(poses).float(), torch.stack(ks).float()
