"""Time forward + backward of the fused RoPE attention core against the eager expression, on one GPU.

    python tools/attention_time.py [--warmup 20] [--iters 100] [--shapes all|name,name] [--out profiles/attention_time.json]
    python tools/attention_time.py --matrix16 [--shapes ...]      (16-bit shapes, writes profiles/attention16_time.json)

Variants, alternated shape by shape in one run:
  eager  the reference's lines (croco/blocks.py:97-110 / 155-176) with the rotation done by this library's own
         rope_2d_pair / cuRoPE2D -- the fastest unfused path a user has today: rope, q @ k^T * scale, softmax, @ v,
         .transpose(1, 2).reshape(B, N, C), and autograd's backward of it
  fused  rope_attention_packed (self) / rope_attention (cross), and their backward
  matrix16      (--matrix16 only) the same calls with matrix16=True: the 16-bit matrix path
  fused_repeat  (--matrix16 only) `fused` a second time in the same rotation: the spread of two runs of one variant, which
                a difference between `fused` and `matrix16` has to exceed to mean anything
All start from the projection's output (a packed [B,N,3,H,D] buffer, or three [B,N,H*D] buffers: non-leaf tensors made
outside the timed region, so the eager path rotates q and k in place with no copy, as the reference does) and a given
upstream gradient, and end with the gradient of those buffers.

Times: device events around each step, median over --iters (>= 100) after --warmup (>= 20); the inputs rotate over
enough buffer sets to exceed the 256 MB last-level cache, so every step reads cold lines.  Bytes: the peak of
torch's allocator during one step above what was allocated before it.  Errors: per tensor max|x - x64| / max|x64|
against the float64 oracle (tests/attention_oracle.py, on the CPU) on a slice of the batch, for both variants -- the
two figures the float32 gate of tests/test_gpu_attention.py compares.
Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

# name: (kind, B, H, Nq, Nk, dtype)
SHAPES = {
    "self_48x16x256_f32": ("self", 48, 16, 256, 256, "float32"),
    "self_32x12x258_f32": ("self", 32, 12, 258, 258, "float32"),
    "self_32x12x258_f16": ("self", 32, 12, 258, 258, "float16"),
    "cross_32x12x258_258_f32": ("cross", 32, 12, 258, 258, "float32"),
    "cross_32x12x258_2322_f32": ("cross", 32, 12, 258, 2322, "float32"),       # the 10-view shape
}
# --matrix16: eager in the 16-bit type, the float32 compute path on the same operands (twice) and the 16-bit matrix path
SHAPES16 = {
    "self_32x12x258_f16": ("self", 32, 12, 258, 258, "float16"),
    "self_32x12x258_bf16": ("self", 32, 12, 258, 258, "bfloat16"),
    "self_48x16x256_bf16": ("self", 48, 16, 256, 256, "bfloat16"),
    "cross_32x12x258_258_bf16": ("cross", 32, 12, 258, 258, "bfloat16"),
    "cross_32x12x258_2322_bf16": ("cross", 32, 12, 258, 2322, "bfloat16"),
}
VARIANTS = ("eager", "fused")
VARIANTS16 = ("eager", "fused", "matrix16", "fused_repeat")


def positions(B, N, gen):
    import torch
    return torch.stack((torch.randint(0, 18, (B, N), generator=gen), torch.randint(0, 18, (B, N), generator=gen)), -1)


def make_set(kind, B, H, Nq, Nk, dtype, gen, dev):
    import torch
    s = {"qpos": positions(B, Nq, gen).to(dev)}
    if kind == "self":
        s["qkv"] = torch.randn(B, Nq, 3, H, 64, generator=gen).to(dtype).to(dev)
        s["kpos"] = s["qpos"]
    else:
        s["kpos"] = positions(B, Nk, gen).to(dev)
        s["xq"] = torch.randn(B, Nq, H * 64, generator=gen).to(dtype).to(dev)
        s["xk"] = torch.randn(B, Nk, H * 64, generator=gen).to(dtype).to(dev)
        s["xv"] = torch.randn(B, Nk, H * 64, generator=gen).to(dtype).to(dev)
    s["dout"] = torch.randn(B, Nq, H * 64, generator=gen).to(dtype).to(dev)
    return s


def prepare(kind, s):
    """OUTSIDE the timed region: the projection buffers as non-leaf tensors (leaf * 1), as a linear layer's output is
    -- the eager path then rotates them in place, as the reference does, with no copy of its own.  Both variants start
    from these and return the gradient of the leaves, so both carry the same one elementwise kernel per buffer in
    their backward."""
    names = ("qkv",) if kind == "self" else ("xq", "xk", "xv")
    leaves = tuple(s[n].detach().requires_grad_(True) for n in names)
    return leaves, tuple(x * 1 for x in leaves)


def step(variant, kind, H, s, leaves, bufs):
    """forward + backward from the projection buffers; returns (out, gradients of the buffers)"""
    import torch

    import spfsplatv2_amd as spf
    if kind == "self":
        (qkv,) = bufs
        if variant != "eager":
            out = spf.rope_attention_packed(qkv, s["qpos"], matrix16=variant == "matrix16")
        else:
            B, N = qkv.shape[:2]
            t = _rope_packed_(qkv, s["qpos"]).transpose(1, 3)
            q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
            attn = ((q @ k.transpose(-2, -1)) * 0.125).softmax(dim=-1)
            out = (attn @ v).transpose(1, 2).reshape(B, N, H * 64)
    else:
        B, Nq = bufs[0].shape[:2]
        q, k, v = (x.reshape(B, x.shape[1], H, 64).permute(0, 2, 1, 3) for x in bufs)
        if variant != "eager":
            out = spf.rope_attention(q, k, v, s["qpos"], s["kpos"], matrix16=variant == "matrix16")
        else:
            rope = spf.cuRoPE2D(100.0, 1.0)                      # in place on the non-leaf views, as blocks.py:161-163
            q, k = rope(q, s["qpos"]), rope(k, s["kpos"])
            attn = ((q @ k.transpose(-2, -1)) * 0.125).softmax(dim=-1)
            out = (attn @ v).transpose(1, 2).reshape(B, Nq, H * 64)
    grads = torch.autograd.grad(out, leaves, s["dout"])
    return out, grads


def _rope_packed_(qkv, pos):
    """q and k of a packed non-leaf [B,N,3,H,D] buffer rotated IN PLACE by ONE rope_2d_pair launch (the fastest unfused
    rotation this library offers), with the matching in-place backward on the gradient; v is not touched."""
    import torch

    import spfsplatv2_amd as spf

    class F(torch.autograd.Function):
        @staticmethod
        def forward(ctx, qkv, pos):
            spf.rope_2d_pair(qkv[:, :, 0], qkv[:, :, 1], pos, 100.0, 1.0)
            ctx.save_for_backward(pos)
            ctx.mark_dirty(qkv)
            return qkv

        @staticmethod
        def backward(ctx, g):
            if not g.is_contiguous():
                g = g.contiguous()
            spf.rope_2d_pair(g[:, :, 0], g[:, :, 1], ctx.saved_tensors[0], 100.0, -1.0)
            return g, None
    return F.apply(qkv, pos)


def errors(kind, H, s, results, rows=2):
    """err of each variant's (out, gradients) against the float64 oracle, on the first `rows` batch items"""
    import torch

    from tests import attention_oracle as O
    sl = {k: v[:rows].cpu() for k, v in s.items()}
    if kind == "self":
        leaves = [sl["qkv"].double().requires_grad_(True)]
        t = leaves[0].transpose(1, 3)
        q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    else:
        leaves = [sl[n].double().requires_grad_(True) for n in ("xq", "xk", "xv")]
        q, k, v = (x.reshape(rows, x.shape[1], H, 64).permute(0, 2, 1, 3) for x in leaves)
    out = O.attention_core(q, k, v, sl["qpos"], sl["kpos"])
    grads = torch.autograd.grad(out, leaves, sl["dout"].double())
    want = [out.detach(), *grads]
    names = ["out", "dq", "dk", "dv"]
    if kind == "self":                                  # the packed gradient's three views, as the gate compares them
        want = [want[0]] + [want[1][:, :, i] for i in range(3)]
    res = {}
    for var, (o, g) in results.items():
        got = [o] + ([g[0][:, :, i] for i in range(3)] if kind == "self" else list(g))
        res[var] = {n: float((a[:rows].double().cpu() - w).abs().max() / w.abs().max()) for n, a, w in zip(names, got, want)}
    return res


def run(name, warmup, iters, shapes=SHAPES, variants=VARIANTS):
    import torch
    kind, B, H, Nq, Nk, dt = shapes[name]
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    sets, set_bytes = steptime.input_sets(lambda: make_set(kind, B, H, Nq, Nk, getattr(torch, dt), gen, dev))
    res = {"shape": name, "kind": kind, "B": B, "H": H, "Nq": Nq, "Nk": Nk, "dtype": dt, "input_sets": len(sets),
           "input_set_bytes": set_bytes}
    steps = {var: (lambda s, leaves, bufs, var=var: step(var, kind, H, s, leaves, bufs)) for var in variants}
    res["variants"], results = steptime.alternate(variants, steps, sets, warmup, iters, prepare=lambda s: prepare(kind, s))
    res["err_vs_float64"] = errors(kind, H, sets[0], results)
    ms = {var: res["variants"][var]["ms_median"] for var in variants}
    res["speedup_fused_over_eager"] = ms["eager"] / ms["fused"]
    if "matrix16" in ms:
        spread = steptime.spread_summary(ms["fused"], ms["matrix16"], ms["fused_repeat"])
        res["fused_spread_ms"] = spread["spread_ms"]
        res["matrix16_gain_over_fused_ms"] = spread["gain_ms"]
        res["speedup_matrix16_over_fused"] = spread["speedup"]
        res["speedup_matrix16_over_eager"] = ms["eager"] / ms["matrix16"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--matrix16", action="store_true", help="the 16-bit shapes with the matrix16 variant")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    shapes, variants = (SHAPES16, VARIANTS16) if args.matrix16 else (SHAPES, VARIANTS)
    if args.out is None:
        args.out = str(ROOT / "profiles" / ("attention16_time.json" if args.matrix16 else "attention_time.json"))
    steptime.require_counts("attention_time", args, 100, 20)
    res = steptime.require_gpu("attention_time")
    names = list(shapes) if args.shapes == "all" else args.shapes.split(",")
    res["results"] = [steptime.note(run(n, args.warmup, args.iters, shapes, variants)) for n in names]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
