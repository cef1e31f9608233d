"""Golden vectors of multi-view cross-attention from the REFERENCE's own classes (build container only):
``CrossAttention`` of croco/blocks.py with the reference's pure-PyTorch ``RoPE2D`` fallback, loaded by file path as
make_attention_goldens.py does, on the CPU in float32.

The case is the second decoder block of a multi-view backbone on v = 4 views of which the last is a target
(b = 2, l = 37 tokens per view, C = 128, 2 heads): query views 1 .. 3 over the OTHER views' tokens, a context view
over the other context views and the target view over every other view.  This file gathers those key sets itself
(index_select, allowed views ascending) and, as the masked backbone does, calls the layer twice with the same weights
-- once for the two context query views (keys of 2 views each), once for the target query view (keys of 3 views).
Recorded: the tokens ``x`` [b,v,l,C] and their positions, the weights, the output [b,3,l,C] (context views, then the
target view) and the gradients of the loss 0.5 * sum(out^2) with respect to ``x`` and to every weight.

Writes tests/golden/attention_views_goldens.pt:
    python tests/golden/make_attention_views_goldens.py
"""
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from make_attention_goldens import REF, load, positions  # noqa: E402


def main():
    blocks = load("ref_croco_blocks", REF / "blocks.py")
    RoPE2D = load("ref_pos_embed", REF / "pos_embed.py").RoPE2D
    gen = torch.Generator().manual_seed(23)
    b, v, num_target, H = 2, 4, 1, 2
    vc, dim = v - num_target, 64 * H
    mod = blocks.CrossAttention(dim, rope=RoPE2D(freq=100.0, F0=1.0), num_heads=H, qkv_bias=True)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
    pos = positions(b, 5, 7, 2)[:, None].expand(b, v, -1, -1).clone()           # [b,v,37,2], the same grid in every view
    l = pos.shape[2]
    x = torch.randn(b, v, l, dim, generator=gen).requires_grad_(True)
    allow = torch.tensor([[s != i and (i >= vc or s < vc) for s in range(v)] for i in range(1, v)])

    def gathered(t, i):
        idx = torch.tensor([s for s in range(v) if allow[i - 1, s]])
        return t.index_select(1, idx).flatten(1, 2)                              # [b, n*l, ...]

    def call(views):
        """One call of the layer for query views of equal key count: [b*len(views), ...] batches."""
        query = torch.cat([x[:, i] for i in views])
        memory = torch.cat([gathered(x, i) for i in views])
        qpos = torch.cat([pos[:, i] for i in views])
        kpos = torch.cat([gathered(pos, i) for i in views])
        out = mod(query, memory, memory, qpos, kpos)
        return out.reshape(len(views), b, l, dim).transpose(0, 1)                # [b, len(views), l, C]

    out = torch.cat([call(list(range(1, vc))), call(list(range(vc, v)))], dim=1)        # the reference's two calls
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad(0.5 * (out * out).sum(), [x] + list(params.values()))
    case = {"kind": "views", "num_heads": H, "base": 100.0, "v": v, "num_target": num_target,
            "query_views": (1, v), "key_views": (0, v), "allow": allow, "x": x.detach(), "pos": pos,
            "weights": {k: t.detach().clone() for k, t in mod.state_dict().items()}, "out": out.detach(),
            "grads": dict(zip(["x"] + list(params), grads))}
    path = HERE / "attention_views_goldens.pt"
    torch.save({"blk2_2x4x37_t1": case}, path)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
