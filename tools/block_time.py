"""Time forward + backward of one transformer block: this package's fused block against the same block assembled from
eager row operations, on one GPU.

    python tools/block_time.py [--warmup 20] [--iters 100] [--shapes all|name,name] [--out profiles/block_time.json]

Variants, alternated step by step in one run on one device:
  baseline         the path available without csrc/block.hip: the reference's block (croco/blocks.py:115-131 / 181-203,
                   vggt/layers/block.py:81-107) on this package's Attention / CrossAttention / VGGTAttention with eager
                   nn.LayerNorm, nn.GELU, LayerScale and tensor adds
  fused            spfsplatv2_amd.Block / DecoderBlock / VGGTBlock, the same weights
  baseline_repeat  `baseline` a second time in the same rotation: the spread of two runs of one variant, which a difference
                   between `baseline` and `fused` has to exceed to mean anything
A step is the module's forward and the backward of a given upstream gradient to the tokens and to every parameter.

Times: device events around each step, median over --iters (>= 100) after --warmup (>= 20); the tokens rotate over enough
buffer sets to exceed the 256 MB last-level cache twice, so every step reads cold tokens.  Bytes: the peak of torch's
allocator during one step above what was allocated before it.  Host syncs: the synchronising calls torch reports during
one step (steptime.count_syncs).  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from functools import partial
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

# name: (kind, dim, heads, batch, tokens, memory tokens)
SHAPES = {
    "block_1024x16_48x256": ("block", 1024, 16, 48, 256, 0),
    "decoder_768x12_32x258_258": ("decoder", 768, 12, 32, 258, 258),
    "vggt_1024x16_4x786": ("vggt", 1024, 16, 4, 786, 0),
}
VARIANTS = ("baseline", "fused", "baseline_repeat")
EPS = 1e-6


def build(kind, dim, heads, fused):
    """The fused module, or the eager assembly with the same submodule names (so one state dict serves both)."""
    import torch
    from torch import nn

    import spfsplatv2_amd as spf
    norm = partial(nn.LayerNorm, eps=EPS)
    if fused:
        if kind == "block":
            return spf.Block(dim, heads, qkv_bias=True, norm_layer=norm, rope=spf.cuRoPE2D(100.0))
        if kind == "decoder":
            return spf.DecoderBlock(dim, heads, qkv_bias=True, norm_layer=norm, rope=spf.cuRoPE2D(100.0))
        return spf.VGGTBlock(dim, heads, init_values=0.01, qk_norm=True, norm_layer=norm,
                             rope=spf.RotaryPositionEmbedding2D(frequency=100.0))

    class EagerMlp(nn.Module):
        def __init__(self):
            super().__init__()
            self.fc1, self.act, self.fc2 = nn.Linear(dim, 4 * dim), nn.GELU(), nn.Linear(4 * dim, dim)

        def forward(self, x):
            return self.fc2(self.act(self.fc1(x)))

    class Eager(nn.Module):
        def __init__(self):
            super().__init__()
            self.norm1 = norm(dim)
            if kind == "vggt":
                self.attn = spf.VGGTAttention(dim, num_heads=heads, qk_norm=True,
                                              rope=spf.RotaryPositionEmbedding2D(frequency=100.0))
                self.ls1 = spf.LayerScale(dim, init_values=0.01)
            else:
                self.attn = spf.Attention(dim, rope=spf.cuRoPE2D(100.0), num_heads=heads, qkv_bias=True)
            if kind == "decoder":
                self.cross_attn = spf.CrossAttention(dim, rope=spf.cuRoPE2D(100.0), num_heads=heads, qkv_bias=True)
            self.norm2 = norm(dim)
            if kind == "decoder":
                self.norm3 = norm(dim)
            self.mlp = EagerMlp()
            if kind == "decoder":
                self.norm_y = norm(dim)
            if kind == "vggt":
                self.ls2 = spf.LayerScale(dim, init_values=0.01)

        def forward(self, x, y, xpos, ypos):
            if kind == "vggt":
                x = x + self.ls1(self.attn(self.norm1(x), pos=xpos))
                return x + self.ls2(self.mlp(self.norm2(x)))
            x = x + self.attn(self.norm1(x), xpos)
            if kind == "decoder":
                y_ = self.norm_y(y)
                x = x + self.cross_attn(self.norm2(x), y_, y_, xpos, ypos)
                return x + self.mlp(self.norm3(x))
            return x + self.mlp(self.norm2(x))
    return Eager()


def call(kind, fused, mod, s):
    if not fused:
        return mod(s["x"], s.get("y"), s["xpos"], s.get("ypos"))
    if kind == "block":
        return mod(s["x"], s["xpos"])
    if kind == "decoder":
        return mod(s["x"], s["y"], s["xpos"], s["ypos"])[0]
    return mod(s["x"], pos=s["xpos"])


def make_set(kind, dim, B, N, M, gen, dev):
    import torch

    def positions(n):
        return torch.stack((torch.randint(0, 18, (B, n), generator=gen), torch.randint(0, 18, (B, n), generator=gen)), -1)
    s = {"x": torch.randn(B, N, dim, generator=gen).to(dev).requires_grad_(True), "xpos": positions(N).to(dev),
         "dout": torch.randn(B, N, dim, generator=gen).to(dev)}
    if kind == "decoder":
        s["y"] = torch.randn(B, M, dim, generator=gen).to(dev).requires_grad_(True)
        s["ypos"] = positions(M).to(dev)
    return s


def step(kind, fused, mod, s):
    """forward + backward to the tokens and every parameter"""
    import torch
    out = call(kind, fused, mod, s)
    wrt = [s["x"]] + ([s["y"]] if kind == "decoder" else []) + list(mod.parameters())
    return out, torch.autograd.grad(out, wrt, s["dout"])


def run(name, warmup, iters):
    import torch
    kind, dim, heads, B, N, M = SHAPES[name]
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    mods = {True: build(kind, dim, heads, True).to(dev)}
    mods[False] = build(kind, dim, heads, False).to(dev)
    mods[False].load_state_dict(mods[True].state_dict())                # same names, same weights
    sets, set_bytes = steptime.input_sets(lambda: make_set(kind, dim, B, N, M, gen, dev))
    res = {"shape": name, "kind": kind, "dim": dim, "heads": heads, "B": B, "N": N, "M": M, "input_sets": len(sets),
           "input_set_bytes": set_bytes, "parameters": sum(p.numel() for p in mods[True].parameters())}
    steps = {var: (lambda s, fused=var == "fused": step(kind, fused, mods[fused], s)) for var in VARIANTS}
    res["variants"], results = steptime.alternate(VARIANTS, steps, sets, warmup, iters, warm=VARIANTS[:2], syncs=True)
    # the two paths compute one function: the largest relative difference over the output and every gradient
    (o0, g0), (o1, g1) = results["baseline"], results["fused"]
    res["max_rel_diff_fused_vs_baseline"] = steptime.max_rel_diff((o1, *g1), (o0, *g0))
    ms = {var: res["variants"][var]["ms_median"] for var in VARIANTS}
    spread = steptime.spread_summary(ms["baseline"], ms["fused"], ms["baseline_repeat"])
    res.update(baseline_spread_ms=spread["spread_ms"], gain_ms=spread["gain_ms"], speedup_fused_over_baseline=spread["speedup"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "block_time.json"))
    args = ap.parse_args()
    steptime.require_counts("block_time", args, 100, 20)
    res = steptime.require_gpu("block_time")
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    res["results"] = [steptime.note(run(n, args.warmup, args.iters)) for n in names]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
