"""Time one optimizer step of the reference's parameter set on one GPU and count its host syncs.

    python tools/optim_time.py [--encoder-blocks 24] [--decoder-blocks 12] [--warmup 20] [--iters 100] [--out FILE]

The parameter set is built analytically from the reference's architecture (no checkpoint is read): a ViT-L encoder (24
blocks at C = 1024: norms, qkv, proj, a 4x MLP, all with biases; patch embedding and final norm), two decoders of 12
blocks at C = 768 with self- and cross-attention (three norms, qkv, proj, projq / projk / projv, proj, a 4x MLP; the
1024 -> 768 embedding and final norm), and a head's worth of small tensors.  The heads form the first parameter group, the
rest the second, with the reference's two learning rates.  Gradients are seeded: N(0, 1e-4^2), so that the total norm is
above 0.5 (the clip is active) and no element is near the guard's threshold (no step is skipped).  Variants:
  a  eager: the lines of the reference's ``optimizer_step`` hook restated -- per parameter ``isnan(grad).any()``,
     ``grad.abs().max().item()`` and ``grad.abs().max() > 5`` -- then ``clip_grad_norm_(parameters, 0.5)``,
     ``torch.optim.AdamW(..., weight_decay=0.05, betas=(0.9, 0.95)).step()`` with torch's defaults and ``zero_grad()``
  b  ``spfsplatv2_amd.GuardedAdamW``: ``step()``, ``zero_grad()``
Variant a runs twice, before and after b (a, b, a), each on its own copy of the parameters.  Before every step, outside
the timed span, every parameter gets a fresh clone of its seeded gradient (``zero_grad`` dropped the last one, and the
eager clip scales gradients in place).  Times are device events around each step (median over --iters >= 100 after
--warmup >= 20), syncs the warnings of torch's sync debug mode during one step, bytes the peak of
allocated device memory during one step above what was allocated before it.  Prints one JSON line (and writes it to
--out, default profiles/optim_time.json).
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

GRAD_SIGMA = 1e-4
LR, BACKBONE_LR_MULTIPLIER = 2e-4, 0.1


def parameter_shapes(encoder_blocks: int = 24, decoder_blocks: int = 12):
    """[(name, shape)] in module order."""
    def linear(prefix, out_f, in_f):
        return [(prefix + ".weight", (out_f, in_f)), (prefix + ".bias", (out_f,))]

    def norm(prefix, c):
        return [(prefix + ".weight", (c,)), (prefix + ".bias", (c,))]

    C, D = 1024, 768
    shapes = [("encoder.backbone.patch_embed.proj.weight", (C, 3, 16, 16)), ("encoder.backbone.patch_embed.proj.bias", (C,))]
    for i in range(encoder_blocks):
        b = f"encoder.backbone.enc_blocks.{i}"
        shapes += norm(b + ".norm1", C) + linear(b + ".attn.qkv", 3 * C, C) + linear(b + ".attn.proj", C, C)
        shapes += norm(b + ".norm2", C) + linear(b + ".mlp.fc1", 4 * C, C) + linear(b + ".mlp.fc2", C, 4 * C)
    shapes += norm("encoder.backbone.enc_norm", C)
    shapes += linear("encoder.backbone.decoder_embed", D, C)
    for dec in ("dec_blocks", "dec_blocks2"):
        for i in range(decoder_blocks):
            b = f"encoder.backbone.{dec}.{i}"
            shapes += norm(b + ".norm1", D) + linear(b + ".attn.qkv", 3 * D, D) + linear(b + ".attn.proj", D, D)
            shapes += norm(b + ".norm_y", D) + norm(b + ".norm2", D)
            shapes += linear(b + ".cross_attn.projq", D, D) + linear(b + ".cross_attn.projk", D, D)
            shapes += linear(b + ".cross_attn.projv", D, D) + linear(b + ".cross_attn.proj", D, D)
            shapes += norm(b + ".norm3", D) + linear(b + ".mlp.fc1", 4 * D, D) + linear(b + ".mlp.fc2", D, 4 * D)
    shapes += norm("encoder.backbone.dec_norm", D)
    head = "encoder.gaussian_param_head"
    shapes += linear(head + ".proj", 256, D) + [(head + ".conv1.weight", (128, 256, 3, 3)), (head + ".conv1.bias", (128,)),
                                                (head + ".conv2.weight", (84, 128, 1, 1)), (head + ".conv2.bias", (84,))]
    shapes += linear("encoder.pose_head.fc1", 512, D) + linear("encoder.pose_head.fc2", 9, 512)
    return shapes


def is_new(name: str) -> bool:
    return any(k in name for k in ("gaussian_param_head", "intrinsic_encoder", "pose_head", "camera_head"))


def eager_step(named, params, optimizer, threshold=5.0):
    """The reference's hook, restated; returns max_gradient (a host float, as the hook logs it)."""
    import torch
    nan_detected = large_detected = False
    max_gradient = 0.0
    for _, p in named:
        if p.grad is None:
            continue
        if torch.isnan(p.grad).any():
            nan_detected = True
            break
        max_gradient = max(max_gradient, p.grad.abs().max().item())
        if p.grad.abs().max() > threshold:
            large_detected = True
            break
    if not (nan_detected or large_detected):
        torch.nn.utils.clip_grad_norm_(params, 0.5)
        optimizer.step()
    optimizer.zero_grad()
    return max_gradient


def run(encoder_blocks, decoder_blocks, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    dev = "cuda"
    shapes = parameter_shapes(encoder_blocks, decoder_blocks)
    gen = torch.Generator(device=dev).manual_seed(0)
    init = [torch.randn(s, generator=gen, device=dev) * 0.02 for _, s in shapes]
    seeded = [torch.randn(s, generator=gen, device=dev) * GRAD_SIGMA for _, s in shapes]
    numel = sum(t.numel() for t in init)

    def make(kind):
        params = [torch.nn.Parameter(t.clone()) for t in init]
        named = [(n, p) for (n, _), p in zip(shapes, params)]
        groups = [{"params": [p for n, p in named if is_new(n)], "lr": LR},
                  {"params": [p for n, p in named if not is_new(n)], "lr": LR * BACKBONE_LR_MULTIPLIER}]
        if kind == "a":
            opt = torch.optim.AdamW(groups, lr=LR, weight_decay=0.05, betas=(0.9, 0.95))
            return params, lambda: eager_step(named, params, opt)
        opt = spf.GuardedAdamW(groups, lr=LR, weight_decay=0.05, betas=(0.9, 0.95), max_grad_value=5.0, max_norm=0.5,
                               named_parameters=named)

        def step():
            opt.step()
            opt.zero_grad()
            return opt.last_step.max_gradient
        return params, step

    def measure(params, step):
        def fresh():
            for p, g in zip(params, seeded):
                p.grad = g.clone()

        res = steptime.median_ms(step, warmup, iters, before=fresh)
        fresh()
        (syncs, max_gradient), peak, _ = steptime.peak_step(lambda: steptime.syncs_and_result(step))
        return {**res, "syncs_per_step": syncs, "peak_extra_bytes_allocated": int(peak),
                "tb_per_s_if_32_bytes_per_parameter": 32.0 * numel / res["ms_median"] * 1e-9,
                "max_gradient": float(max_gradient), "iters": iters, "warmup": warmup}

    pa, sa = make("a")
    pb, sb = make("b")
    out = {"tensors": len(shapes), "parameters": numel, "grad_sigma": GRAD_SIGMA, "variants": {}}
    out["variants"]["a_first"] = measure(pa, sa)
    out["variants"]["b"] = measure(pb, sb)
    out["variants"]["a_second"] = measure(pa, sa)
    a = 0.5 * (out["variants"]["a_first"]["ms_median"] + out["variants"]["a_second"]["ms_median"])
    out["speedup_b_over_a"] = a / out["variants"]["b"]["ms_median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--encoder-blocks", type=int, default=24)
    ap.add_argument("--decoder-blocks", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "optim_time.json"), help="also write the JSON line to this file")
    args = ap.parse_args()
    steptime.require_counts("optim_time", args, 100, 20)
    res = steptime.require_gpu("optim_time")
    res["results"] = [run(args.encoder_blocks, args.decoder_blocks, args.warmup, args.iters)]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
