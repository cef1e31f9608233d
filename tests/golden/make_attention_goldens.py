"""Golden vectors of the attention modules from the REFERENCE's own classes (build container only): ``Attention`` and
``CrossAttention`` of croco/blocks.py, loaded by file path, with the reference's pure-PyTorch ``RoPE2D`` fallback
(croco/pos_embed.py:112-159; its ``from .curope import cuRoPE2D`` fails here, so the reference selects it itself), on
the CPU in float32.  Seeded inputs, the modules' weights, outputs and input gradients of the loss 0.5 * sum(out^2)
(so the upstream gradient is the output and needs no tensor of its own).  The cross case feeds one memory tensor as
key and value, as the decoder blocks do (blocks.py DecoderBlock.forward).

Writes tests/golden/attention_goldens.pt (self-attention) and attention_goldens_cross.pt (cross-attention and the
rope=None case): the weights of a 192- and a 128-wide layer do not fit one file of the size the repository allows.
    python tests/golden/make_attention_goldens.py
"""
import importlib.util
import sys
import types
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/src/model/encoder/backbone/croco")


def load(name, path):
    for m in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(m, types.ModuleType(m))
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def positions(B, hh, ww, extra):
    """(y, x) grid positions as PositionGetter produces them plus `extra` tokens below the grid (intrinsics / pose)."""
    y, x = torch.meshgrid(torch.arange(hh), torch.arange(ww), indexing="ij")
    pos = torch.stack([y.reshape(-1), x.reshape(-1)], dim=-1)
    for i in range(extra):
        pos = torch.cat([pos, torch.tensor([[hh + i, 0]])])
    return pos[None].expand(B, -1, -1).clone().long()


def main():
    blocks = load("ref_croco_blocks", REF / "blocks.py")
    RoPE2D = load("ref_pos_embed", REF / "pos_embed.py").RoPE2D
    gen = torch.Generator().manual_seed(11)

    def init(mod):
        with torch.no_grad():
            for p in mod.parameters():
                p.copy_(torch.randn(p.shape, generator=gen) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
        return mod

    def run_self(B, H, hh, ww, extra, rope):
        dim = 64 * H
        mod = init(blocks.Attention(dim, rope=RoPE2D(freq=100.0, F0=1.0) if rope else None, num_heads=H, qkv_bias=True))
        xpos = positions(B, hh, ww, extra)
        x = torch.randn(B, xpos.shape[1], dim, generator=gen).requires_grad_(True)
        out = mod(x, xpos)
        (dx,) = torch.autograd.grad(0.5 * (out * out).sum(), (x,))
        return {"kind": "self", "num_heads": H, "base": 100.0 if rope else None, "inputs": ["x"], "x": x.detach(),
                "xpos": xpos, "weights": {k: v.detach().clone() for k, v in mod.state_dict().items()},
                "out": out.detach(), "grads": {"x": dx}}

    def run_cross(B, H, q_grid, k_grid):
        dim = 64 * H
        mod = init(blocks.CrossAttention(dim, rope=RoPE2D(freq=100.0, F0=1.0), num_heads=H, qkv_bias=True))
        qpos, kpos = positions(B, *q_grid), positions(B, *k_grid)
        query = torch.randn(B, qpos.shape[1], dim, generator=gen).requires_grad_(True)
        memory = torch.randn(B, kpos.shape[1], dim, generator=gen).requires_grad_(True)
        out = mod(query, memory, memory, qpos, kpos)
        dq, dm = torch.autograd.grad(0.5 * (out * out).sum(), (query, memory))
        return {"kind": "cross", "num_heads": H, "base": 100.0, "inputs": ["query", "memory"], "query": query.detach(),
                "memory": memory.detach(), "qpos": qpos, "kpos": kpos,
                "weights": {k: v.detach().clone() for k, v in mod.state_dict().items()}, "out": out.detach(),
                "grads": {"query": dq, "memory": dm}}

    self_cases = {"self_2x3x70": run_self(2, 3, 17, 4, 2, True)}
    cross_cases = {"cross_2x2x66_131": run_cross(2, 2, (8, 8, 2), (13, 10, 1)),
                   "self_norope_1x1x5": run_self(1, 1, 1, 5, 0, False)}
    torch.save(self_cases, HERE / "attention_goldens.pt")
    torch.save(cross_cases, HERE / "attention_goldens_cross.pt")
    for f in ("attention_goldens.pt", "attention_goldens_cross.pt"):
        print("wrote", HERE / f, (HERE / f).stat().st_size, "bytes")


if __name__ == "__main__":
    main()
