"""Time the distillation point loss (Regr3D), forward + backward, on one GPU, and count its host syncs.

    python tools/regr3d_time.py [--shapes 16x256x256,3x256x256] [--warmup 20] [--iters 100] [--variants a,b] [--out FILE]

Variants, per training step (the call of model_wrapper.py:326-329: both predictions requiring grad, strided views of a
[b,v,h,w,1,3] tensor, the loss times 0.1 backward):
  a  eager: the reference's expression restated here in eager PyTorch on the device -- torch.quantile per view, the
     boolean index-puts of invalid_to_zeros, the boolean gathers of the loss
  b  the HIP loss (spfsplatv2_amd.Regr3D)
Times are device events around each step (median over --iters >= 100 after --warmup), syncs the warnings of
torch's sync debug mode during one step.  Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

DEFAULT_SHAPES = "16x256x256,3x256x256"


def make_inputs(b, h, w, seed=0):
    """Teacher points at log-uniform depths with 1 % outliers either side, predictions = a rescaled noisy copy held as
    [b,2,h,w,1,3] (the encoder's `means`), confidences in [1, 9)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = "cuda"

    def rand(*s):
        return torch.rand(*s, generator=g, device=dev)
    xy = (rand(b, 2, h, w, 2) - 0.5) * 1.2
    d = torch.cat([xy, torch.ones(b, 2, h, w, 1, device=dev)], -1)
    depth = torch.exp(rand(b, 2, h, w) * math.log(20.0))
    u = rand(b, 2, h, w)
    near = torch.exp(math.log(0.2) - rand(b, 2, h, w) * math.log(0.2))
    far = torch.exp(math.log(20.0) + rand(b, 2, h, w) * math.log(10.0))
    depth = torch.where(u < 0.01, near, torch.where(u > 0.99, far, depth))
    gt = d * depth[..., None]
    means = (gt * (0.5 + 1.5 * rand(b, 1, 1, 1, 1)) +
             0.05 * depth[..., None] * torch.randn(b, 2, h, w, 3, generator=g, device=dev))[:, :, :, :, None, :]
    conf = 1.0 + 8.0 * rand(b, 2, h, w)
    return gt[:, 0].contiguous(), gt[:, 1].contiguous(), means.contiguous(), conf[:, 0].contiguous(), conf[:, 1].contiguous()


def eager_loss(gt1, gt2, pr1, pr2, conf1, conf2):
    """Regr3D.forward with norm_mode 'avg_dis', dist_clip None, in eager PyTorch with the reference's own operations."""
    import torch

    def valid_of(gt, conf):
        dis = gt.norm(dim=-1)
        q = torch.quantile(dis.view(dis.shape[0], -1), torch.tensor([0.002, 0.998]).to(dis.device), dim=1)
        return (dis >= q[0].view(-1, 1, 1)) & (dis <= q[1].view(-1, 1, 1)) & (conf >= 3)

    def normalize(p1, p2, v1, v2):
        z1, z2 = p1.clone(), p2.clone()
        z1[~v1] = 0
        z2[~v2] = 0
        nnz = v1.view(len(v1), -1).sum(1) + v2.view(len(v2), -1).sum(1)
        dis = torch.cat((z1.flatten(1, 2), z2.flatten(1, 2)), dim=1).norm(dim=-1)
        nf = (dis.sum(dim=1) / (nnz + 1e-8)).clip(min=1e-8)[:, None, None, None]
        return p1 / nf, p2 / nf
    v1, v2 = valid_of(gt1, conf1), valid_of(gt2, conf2)
    pr1, pr2 = normalize(pr1, pr2, v1, v2)
    gt1, gt2 = normalize(gt1, gt2, v1, v2)
    l1 = torch.norm(pr1 - gt1, dim=-1)[v1]
    l2 = torch.norm(pr2 - gt2, dim=-1)[v2]
    return l1.mean() + l2.mean()


def run(shape, variants, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    b, h, w = shape
    gt1, gt2, means, conf1, conf2 = make_inputs(b, h, w)
    leaf = means.clone().requires_grad_(True)
    hip = spf.Regr3D()

    def step(var):
        leaf.grad = None
        p1, p2 = leaf[:, 0].squeeze(-2), leaf[:, 1].squeeze(-2)
        loss = (eager_loss if var == "a" else hip)(gt1, gt2, p1, p2, conf1, conf2) * 0.1
        loss.backward()
        return loss

    out = {"shape": list(shape), "points": 2 * b * h * w, "variants": {}}
    losses = {}
    for var in variants:
        ms = steptime.median_ms(lambda: step(var), warmup, iters)
        syncs, loss = steptime.syncs_and_result(lambda: step(var))
        losses[var] = float(loss.detach())
        out["variants"][var] = {**ms, "syncs_per_step": syncs, "iters": iters, "warmup": warmup}
    out["loss_per_variant"] = losses
    t = {k: r["ms_median"] for k, r in out["variants"].items()}
    if "a" in t and "b" in t:
        out["speedup_b_over_a"] = t["a"] / t["b"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=DEFAULT_SHAPES, help="comma-separated BxHxW")
    ap.add_argument("--variants", default="a,b")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    steptime.require_counts("regr3d_time", args, 100, 0)
    res = steptime.require_gpu("regr3d_time")
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",") if s]
    res["results"] = [run(s, args.variants.split(","), args.warmup, args.iters) for s in shapes]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
