"""Golden vectors of the transformer blocks from the REFERENCE's own classes (build container only): ``Block`` and
``DecoderBlock`` of croco/blocks.py, loaded by file path with the reference's pure-PyTorch ``RoPE2D`` fallback (as
make_attention_goldens.py does), and VGGT's ``Block`` of vggt/layers/block.py with the ``Attention``, ``LayerScale``,
``Mlp`` and ``RotaryPositionEmbedding2D`` the reference vendors next to it (the layers directory is mounted as a package
without running its ``__init__``), on the CPU in float32.

dim = 128, 2 heads of 64, mlp_ratio = 2, LayerNorm eps = 1e-6, qkv_bias; 37 tokens for the self-attention blocks (a 5 x 7
grid + 2), 37 -> 70 (17 x 4 + 2) for the decoder block; ``init_values = 0.1`` and ``qk_norm`` for the VGGT block.  The
tokens have a standard deviation of 0.05, so that the norms' eps = 1e-6 is told from 1e-5 in the output.  Seeded
inputs, the module's weights, the output and the gradients of 0.5 * sum(out^2) with respect to the inputs (so the
upstream gradient is the output and needs no tensor of its own).

Writes tests/golden/block_goldens_{block,decoder,vggt}.pt (data only), one file per module kind, and the decoder block's
weights as block_goldens_decoder_weights.pt: with them its file would exceed the size the repository allows.
    python tests/golden/make_block_goldens.py <reference checkout>
"""
import importlib
import importlib.util
import sys
import types
from functools import partial
from pathlib import Path

import torch
from torch import nn

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
from tests.golden.make_attention_goldens import positions  # noqa: E402
from tests.vggt_attention_oracle import view_positions  # noqa: E402

DIM, HEADS, RATIO, EPS, B = 128, 2, 2.0, 1e-6, 2


def load(name, path):
    for m in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(m, types.ModuleType(m))
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def mount(name, directory):
    """``directory`` as package ``name`` without its __init__ (which would import the whole backbone)."""
    pkg = types.ModuleType(name)
    pkg.__path__ = [str(directory)]
    sys.modules[name] = pkg
    return pkg


def main(ref_root):
    backbone = Path(ref_root) / "src/model/encoder/backbone"
    blocks = load("ref_croco_blocks", backbone / "croco/blocks.py")
    RoPE2D = load("ref_pos_embed", backbone / "croco/pos_embed.py").RoPE2D
    mount("ref_vggt_layers", backbone / "vggt/layers")
    VBlock = importlib.import_module("ref_vggt_layers.block").Block
    VRope = importlib.import_module("ref_vggt_layers.rope").RotaryPositionEmbedding2D
    gen = torch.Generator().manual_seed(29)
    norm = partial(nn.LayerNorm, eps=EPS)

    def init(mod):
        with torch.no_grad():
            for n, p in mod.named_parameters():
                if "norm" in n and n.endswith("weight"):
                    p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=gen))
                elif n.endswith("gamma"):
                    p.copy_(0.1 + 0.03 * torch.randn(p.shape, generator=gen))
                else:
                    p.copy_(torch.randn(p.shape, generator=gen) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
        return mod

    def record(kind, mod, ins, pos, run):
        leaves = {k: v.clone().requires_grad_(True) for k, v in ins.items()}
        out = run(mod, leaves)
        grads = torch.autograd.grad(0.5 * (out * out).sum(), list(leaves.values()))
        return {"kind": kind, "dim": DIM, "num_heads": HEADS, "mlp_ratio": RATIO, "eps": EPS, "base": 100.0,
                "inputs": ins, "pos": pos, "weights": {k: v.detach().clone() for k, v in mod.state_dict().items()},
                "out": out.detach(), "grads": dict(zip(leaves, grads))}

    def tokens(n):
        return 0.05 * torch.randn(B, n, DIM, generator=gen)

    xpos, ypos = positions(B, 5, 7, 2), positions(B, 17, 4, 2)
    block = init(blocks.Block(DIM, HEADS, mlp_ratio=RATIO, qkv_bias=True, norm_layer=norm, rope=RoPE2D(freq=100.0, F0=1.0)))
    gold = record("block", block, {"x": tokens(37)}, {"xpos": xpos}, lambda m, t: m(t["x"], xpos))
    torch.save(gold, HERE / "block_goldens_block.pt")

    dec = init(blocks.DecoderBlock(DIM, HEADS, mlp_ratio=RATIO, qkv_bias=True, norm_layer=norm, norm_mem=True,
                                   rope=RoPE2D(freq=100.0, F0=1.0)))
    gold = record("decoder", dec, {"x": tokens(37), "y": tokens(70)}, {"xpos": xpos, "ypos": ypos},
                  lambda m, t: m(t["x"], t["y"], xpos, ypos)[0])
    # (the decoder block's weights alone come close to the size the repository allows for one file)
    torch.save({"weights": gold.pop("weights")}, HERE / "block_goldens_decoder_weights.pt")
    torch.save(gold, HERE / "block_goldens_decoder.pt")

    vpos = view_positions(B, 1, 5, 7, 2)
    vggt = init(VBlock(DIM, HEADS, mlp_ratio=RATIO, init_values=0.1, norm_layer=norm, qk_norm=True,
                       rope=VRope(frequency=100.0)))
    gold = record("vggt", vggt, {"x": tokens(37)}, {"pos": vpos}, lambda m, t: m(t["x"], pos=vpos))
    gold["init_values"] = 0.1
    gold["qk_eps"] = float(vggt.attn.q_norm.eps)
    torch.save(gold, HERE / "block_goldens_vggt.pt")
    for f in ("block", "decoder", "decoder_weights", "vggt"):
        p = HERE / f"block_goldens_{f}.pt"
        print("wrote", p, p.stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
