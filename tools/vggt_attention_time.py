"""Time forward + backward of the VGGT attention core (q / k LayerNorm, rotation, additive mask) against the
reference's eager lines, on one GPU.  The method is tools/attention_time.py's.

    python tools/vggt_attention_time.py [--warmup 20] [--iters 100] [--shapes all|name,name] [--out profiles/vggt_attention_time.json]

Variants, alternated shape by shape in one run:
  eager  vggt/layers/attention.py:55-71 on the same device: q, k, v unbound from the packed projection, F.layer_norm of
         q and k, this library's RotaryPositionEmbedding2D (one kernel per tensor), F.scaled_dot_product_attention
         with attn_mask, .transpose(1, 2).reshape(B, N, C), and autograd's backward of it
  fused  rope_attention_packed(qkv, pos, mask=, q_norm=, k_norm=) and its backward
Both start from the projection's output (a packed [B,N,3,H,D] non-leaf buffer made outside the timed region) and the
four norm parameters, and end with the gradients of the buffer and of the parameters.

Times: device events around each step, median over --iters (>= 100) after --warmup (>= 20), the inputs rotating over
buffer sets that exceed the last-level cache (cold lines).  Bytes: the peak of torch's allocator during one step above
what was allocated before it.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402
from attention_time import positions  # noqa: E402

# name: (B, H, views S, tokens per view P, mask)
SHAPES = {
    "global_4x16x786": (4, 16, 3, 262, True),          # the reference's global block: 3 views of 262 tokens
    "global_4x16x987": (4, 16, 3, 329, True),
    "frame_12x16x262": (12, 16, 1, 262, False),        # a frame block: no mask
}
EPS = 1e-5


def make_set(B, H, N, gen, dev):
    import torch
    return {"qkv": torch.randn(B, N, 3, H, 64, generator=gen).to(dev), "pos": positions(B, N, gen).to(dev),
            "dout": torch.randn(B, N, H * 64, generator=gen).to(dev)}


def step(variant, H, s, mask, params, leaf, qkv):
    import torch
    import torch.nn.functional as F

    import spfsplatv2_amd as spf
    qw, qb, kw, kb = params
    if variant == "fused":
        out = spf.rope_attention_packed(qkv, s["pos"], mask=mask, q_norm=(qw, qb, EPS), k_norm=(kw, kb, EPS))
    else:
        B, N = qkv.shape[:2]
        q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
        q, k = F.layer_norm(q, (64,), qw, qb, EPS), F.layer_norm(k, (64,), kw, kb, EPS)
        rope = spf.RotaryPositionEmbedding2D(100.0)
        q, k = rope(q, s["pos"]), rope(k, s["pos"])
        out = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2).reshape(B, N, H * 64)
    return out, torch.autograd.grad(out, (leaf, *params), s["dout"])


def run(name, warmup, iters):
    import torch

    from tests.vggt_attention_oracle import view_mask
    B, H, S, P, masked = SHAPES[name]
    N = S * P
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    sets, set_bytes = steptime.input_sets(lambda: make_set(B, H, N, gen, dev))
    mask = view_mask(S, P, 1).to(dev) if masked else None
    params = [(1.0 + 0.3 * torch.randn(64, generator=gen)).to(dev).requires_grad_(True),
              (0.1 * torch.randn(64, generator=gen)).to(dev).requires_grad_(True),
              (1.0 + 0.3 * torch.randn(64, generator=gen)).to(dev).requires_grad_(True),
              (0.1 * torch.randn(64, generator=gen)).to(dev).requires_grad_(True)]

    def prepare(s):                                     # outside the timed region: the projection output as a non-leaf
        leaf = s["qkv"].detach().requires_grad_(True)
        return leaf, leaf * 1

    res = {"shape": name, "B": B, "H": H, "N": N, "mask": masked, "norm": True, "dtype": "float32", "input_sets": len(sets),
           "input_set_bytes": set_bytes}
    variants = ("eager", "fused")
    steps = {var: (lambda s, leaf, qkv, var=var: step(var, H, s, mask, params, leaf, qkv)) for var in variants}
    res["variants"], results = steptime.alternate(variants, steps, sets, warmup, iters, prepare=prepare)
    # the two variants against each other (not an accuracy figure: the gate's figures are the tests')
    (o_e, g_e), (o_f, g_f) = results["eager"], results["fused"]
    res["fused_vs_eager_max_rel"] = {"out": steptime.rel_diff(o_f, o_e), "dqkv": steptime.rel_diff(g_f[0], g_e[0]),
                                     "dparams": steptime.max_rel_diff(g_f[1:], g_e[1:])}
    res["speedup_fused_over_eager"] = res["variants"]["eager"]["ms_median"] / res["variants"]["fused"]["ms_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "vggt_attention_time.json"))
    args = ap.parse_args()
    steptime.require_counts("vggt_attention_time", args, 100, 20)
    res = steptime.require_gpu("vggt_attention_time")
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    res["results"] = [steptime.note(run(n, args.warmup, args.iters)) for n in names]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
