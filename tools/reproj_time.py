"""Time the reprojection loss, forward + backward, on one GPU, and count its host syncs.

    python tools/reproj_time.py [--shapes re10k,re10k_10view] [--warmup 20] [--iters 100] [--variants a,b,c]
    python tools/reproj_time.py --stats KERNEL_STATS_CSV --shapes re10k     (bytes over kernel time, no GPU needed)

Variants, per training step (one loss per context view, every input requiring grad, `sum` of the losses backward):
  a  eager: the reference's expression restated here in eager PyTorch (pixel grid built on the host and uploaded,
     torch.inverse, boolean mask, `valid.sum() > 0` on the host), once per view
  b  the HIP loss (spfsplatv2_amd.reproj_loss), once per view on pts3d[:, i]
  c  the HIP loss, all views in one call
Times are device events around each step (median over --iters after --warmup), syncs the warnings of
torch's sync debug mode during one step.  Prints one JSON line.

--stats reads a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a run of ONE shape (e.g. `--variants c
--shapes re10k`) and prints the HIP kernels' bytes over their mean time: 12 B per point forward (pts3d read), 24 B per
point backward (pts3d read, dL/dpts3d written); the per-slot partials are < 0.1 % of that.
"""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

SHAPES = {"re10k": (16, 2, 256, 256), "re10k_10view": (3, 10, 256, 256)}
WEIGHT, STEP, TOTAL = 0.001, 30_000, 200_001
HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12          # B/s: MI355X spec and measured float4-copy rate


def make_inputs(b, v, h, w, seed=0):
    """pts3d [b,v,h,w,3] that reproject to within a few px of their pixel: each pixel corner unprojected at a random
    depth through its view's camera (small random pose, normalised intrinsics), plus noise."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = "cuda"
    n = b * v
    ang = 0.05 * torch.randn(n, 3, generator=g, device=dev)
    zero = torch.zeros(n, device=dev)
    kx = torch.stack([zero, -ang[:, 2], ang[:, 1], ang[:, 2], zero, -ang[:, 0], -ang[:, 1], ang[:, 0], zero], 1)
    pose = torch.eye(4, device=dev).repeat(n, 1, 1)
    pose[:, :3, :3] = torch.linalg.matrix_exp(kx.view(n, 3, 3))
    pose[:, :3, 3] = 0.5 * torch.randn(n, 3, generator=g, device=dev)
    k = torch.tensor([[0.9, 0.0, 0.5], [0.0, 0.9, 0.5], [0.0, 0.0, 1.0]], device=dev).repeat(n, 1, 1)
    ii, jj = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32),
                            torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    uv = torch.stack([jj, ii], -1)[None] + 3.0 * torch.randn(n, h, w, 2, generator=g, device=dev)
    uv1 = torch.cat([uv, torch.ones_like(uv[..., :1])], -1)
    kp = k * torch.tensor([w, h, 1.0], device=dev)[:, None]
    depth = torch.exp(torch.rand(n, h, w, 1, generator=g, device=dev) * math.log(20.0))
    cam = depth * torch.einsum("nij,nhwj->nhwi", torch.linalg.inv(kp), uv1)
    pts = torch.einsum("nij,nhwj->nhwi", pose[:, :3, :3], cam) + pose[:, None, None, :3, 3]
    return pts.view(b, v, h, w, 3), pose.view(b, v, 4, 4), k.view(b, v, 3, 3)


def eager_loss(pts3d, poses, intrinsics, lw):
    """The reference's per-view expression in eager PyTorch, with its host work kept: [b,h,w,3] -> 0-dim (or 0)."""
    import torch
    b, h, w, _ = pts3d.shape
    kp = intrinsics.clone()
    kp[..., 0, :] = intrinsics[..., 0, :] * w
    kp[..., 1, :] = intrinsics[..., 1, :] * h
    world_to_cam = torch.inverse(poses)
    cam = torch.einsum("bij,bnj->bni", world_to_cam[:, :3, :3], pts3d.reshape(b, h * w, 3)) + world_to_cam[:, None, :3, 3]
    q = torch.einsum("bij,bnj->bni", kp, cam)
    q[..., 2].clamp_(min=1e-6)
    px = (q[..., :2] / q[..., 2, None]).reshape(b, h, w, 2)
    xs, ys = torch.meshgrid(torch.arange(w), torch.arange(h), indexing="xy")      # host grid, uploaded every call
    target = torch.stack([xs, ys])[None].repeat(b, 1, 1, 1).permute(0, 2, 3, 1).to(pts3d.device)
    err = torch.norm(px - target, dim=-1, keepdim=True, p=2)
    valid = ~(err > 1000)
    if valid.sum() > 0:
        ve = err[valid]
        return WEIGHT * (lw * torch.tanh(ve / lw).sum()) / ve.shape[0]
    return 0


def run(shape, variants, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    from spfsplatv2_amd.loss import reproj_lw
    b, v, h, w = SHAPES[shape]
    pts, poses, ks = make_inputs(b, v, h, w)
    lw = reproj_lw("dyntanh", STEP, TOTAL, True)
    leaves = [t.clone().requires_grad_(True) for t in (pts, poses, ks)]

    def hip(p, po, k):
        return spf.reproj_loss(p, po, k, weight=WEIGHT, mode="dyntanh", global_step=STEP, total_iterations=TOTAL,
                               circle_schedule=True)

    def step(var):
        for t in leaves:
            t.grad = None
        p, po, k = leaves
        if var == "a":
            loss = sum(eager_loss(p[:, i], po[:, i], k[:, i], lw) for i in range(v))
        elif var == "b":
            loss = sum(hip(p[:, i], po[:, i], k[:, i]) for i in range(v))
        else:
            loss = hip(p, po, k).sum()
        loss.backward()
        return loss

    out = {"shape": shape, "b": b, "v": v, "h": h, "w": w, "points": b * v * h * w, "variants": {}}
    losses = {}
    for var in variants:
        ms = steptime.median_ms(lambda: step(var), warmup, iters)
        syncs, loss = steptime.syncs_and_result(lambda: step(var))
        losses[var] = float(loss)
        out["variants"][var] = {**ms, "syncs_per_step": syncs, "iters": iters, "warmup": warmup}
    out["loss_per_variant"] = losses
    t = {k: r["ms_median"] for k, r in out["variants"].items()}
    if "a" in t and "c" in t:
        out["speedup_c_over_a"] = t["a"] / t["c"]
    if "b" in t and "c" in t:
        out["speedup_c_over_b"] = t["b"] / t["c"]
    return out


def kernel_stats(path, shape):
    """Bytes over mean kernel time of the HIP kernels in a rocprofv3 kernel_stats.csv (one shape per run)."""
    b, v, h, w = SHAPES[shape]
    pts = b * v * h * w
    need = {"spf_reproj_fwd_kernel": 12 * pts, "spf_reproj_bwd_kernel": 24 * pts}
    rates = {"share_of_peak": HBM_PEAK, "share_of_achievable": HBM_ACHIEVABLE}
    return {"shape": shape, "points": pts,
            "kernels": steptime.kernel_stats(path, ("spf_reproj",), need, rates, width=120, named=True)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="re10k,re10k_10view")
    ap.add_argument("--variants", default="a,b,c")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv to turn into bytes over time")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    if args.stats:
        assert len(shapes) == 1, "--stats reads the profile of one shape"
        steptime.emit(kernel_stats(args.stats, shapes[0]), None)
        return
    steptime.require_counts("reproj_time", args, 2, 0)
    res = steptime.require_gpu("reproj_time")
    res["results"] = [run(s, args.variants.split(","), args.warmup, args.iters) for s in shapes]
    steptime.emit(res, None)


if __name__ == "__main__":
    main()
