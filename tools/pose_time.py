"""Time one "pose step" on one GPU and count its host syncs.

    python tools/pose_time.py [--shape 16x3x256x256] [--context-views 2] [--warmup 20] [--iters 100] [--variants a,b] [--out FILE]

The step, at b scenes of (context + target) views of h x w points: process_pose forward and backward (6-D encoding,
pose_make_baseline_1 and pose_make_relative), process_depth, two compute_pose_error_for_batch calls (as the training step
makes, model_wrapper.py:337-345) and estimate_intrinsics.  Variants:
  a  eager: the oracle's expressions (tests/pose_oracle.py) on the same device, with the reference's control flow -- the
     per-pose .cpu() loop of compute_pose_error_for_batch and the per-scene focal loop with its mask compaction and its
     two `if focal <= 0`
  b  the HIP pose path (spfsplatv2_amd.pose)
Times are device events around each step (median over --iters >= 100 after --warmup >= 20), syncs the warnings of
torch's sync debug mode during one step.  Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402


def make_inputs(b, v, h, w, cv, seed=0):
    import torch

    from tests import pose_oracle as O
    gen = torch.Generator().manual_seed(seed)
    enc = O.make_enc(gen, b, v, cv, "rot6d")
    upstream = torch.randn(b, v, 4, 4, generator=gen)
    gt = O.process_pose(O.make_enc(gen, b, v, cv, "rot6d"), cv, pose_make_baseline_1=True, pose_make_relative=True)
    pts = torch.stack([torch.stack([O.focal_scene(gen, h, w, 0.9 * max(h, w)) for _ in range(v)]) for _ in range(b)])
    return tuple(t.cuda() for t in (enc, upstream, gt, pts))


def run(shape, cv, variants, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    from tests import pose_oracle as O
    b, v, h, w = shape
    enc, upstream, gt, pts = make_inputs(b, v, h, w, cv)
    leaf = enc.clone().requires_grad_(True)

    def step(var):
        leaf.grad = None
        if var == "a":
            poses = O.process_pose(leaf, cv, pose_make_baseline_1=True, pose_make_relative=True)
            poses.backward(upstream)
            depth = O.process_depth(poses.detach(), pts)
            errs = [O.reference_style_pose_error_for_batch(poses.detach()[:, :n], gt[:, :n]) for n in (cv, v)]
            K = O.reference_style_estimate_intrinsics(pts, h, w)
        else:
            poses = spf.process_pose(leaf, cv, pose_make_baseline_1=True, pose_make_relative=True)
            poses.backward(upstream)
            depth = spf.process_depth(poses.detach(), pts)
            errs = [spf.compute_pose_error_for_batch(poses.detach()[:, :n], gt[:, :n]) for n in (cv, v)]
            K = spf.estimate_intrinsics(pts, h, w)
        return poses, depth, errs, K

    out = {"shape": list(shape), "context_views": cv, "variants": {}}
    seen = {}
    for var in variants:
        ms = steptime.median_ms(lambda: step(var), warmup, iters)
        syncs, (poses, depth, errs, K) = steptime.syncs_and_result(lambda: step(var))
        seen[var] = {"focal_scene0": float(K[0, 0, 0]) * h, "error_R_deg": float(errs[1][0]), "error_t_deg": float(errs[1][1]),
                     "depth_mean": float(depth.mean()), "d_enc_abs_max": float(leaf.grad.abs().max())}
        out["variants"][var] = {**ms, "syncs_per_step": syncs, "iters": iters, "warmup": warmup}
    out["values_per_variant"] = seen
    t = {k: r["ms_median"] for k, r in out["variants"].items()}
    if "a" in t and "b" in t:
        out["speedup_b_over_a"] = t["a"] / t["b"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="16x3x256x256", help="BxVxHxW (V = context + target views)")
    ap.add_argument("--context-views", type=int, default=2)
    ap.add_argument("--variants", default="a,b")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    steptime.require_counts("pose_time", args, 100, 20)
    res = steptime.require_gpu("pose_time")
    shape = tuple(int(x) for x in args.shape.split("x"))
    res["results"] = [run(shape, args.context_views, args.variants.split(","), args.warmup, args.iters)]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
