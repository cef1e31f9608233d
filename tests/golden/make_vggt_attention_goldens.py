"""Golden vectors of the VGGT attention layer from the REFERENCE's own classes (build container only): ``Attention`` of
vggt/layers/attention.py and ``RotaryPositionEmbedding2D`` of vggt/layers/rope.py, loaded by file path (both need only
torch), on the CPU in float32, with ``qk_norm=True``.  One set of seeded inputs, weights, positions and mask; per case
(mask and rope, rope only, mask only) the output and the gradients of the loss 0.5 * sum(out^2) with respect to the
input, the four norm parameters and the two biases (so the upstream gradient is the output and needs no tensor of its
own; the gradients of the two weight matrices would take the file over the size the repository allows).

Shape: B = 2, H = 2, S = 3 views of P = 23 tokens (3 special + a 4 x 5 patch grid), one target view.  Positions follow
aggregator.py:324-333 (patch grid + 1, special tokens at (0, 0)); the mask is the one aggregator.py:342-346 builds
(tests/vggt_attention_oracle.py:view_mask restates it, and this script checks the restatement on the way).

Writes tests/golden/vggt_attention_goldens.pt (data only).
    python tests/golden/make_vggt_attention_goldens.py <reference checkout>
"""
import importlib.util
import sys
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))
from tests.vggt_attention_oracle import view_mask, view_positions  # noqa: E402


def load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def main(ref_root):
    layers = Path(ref_root) / "src/model/encoder/backbone/vggt/layers"
    Attention = load("ref_vggt_attention", layers / "attention.py").Attention
    Rope = load("ref_vggt_rope", layers / "rope.py").RotaryPositionEmbedding2D
    B, H, S, special, hh, ww = 2, 2, 3, 3, 4, 5
    P, dim = special + hh * ww, 64 * H
    gen = torch.Generator().manual_seed(23)
    mod = Attention(dim, num_heads=H, qkv_bias=True, proj_bias=True, qk_norm=True, rope=Rope(frequency=100.0))
    with torch.no_grad():
        for n, p in mod.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=gen))
            else:
                p.copy_(torch.randn(p.shape, generator=gen) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
    pos = view_positions(B, S, hh, ww, special)
    mask = view_mask(S, P, 1)
    x = torch.randn(B, S * P, dim, generator=gen)
    cases = {}
    for name, use_mask, use_rope in (("mask_rope", True, True), ("rope", False, True), ("mask", True, False)):
        mod.rope = Rope(frequency=100.0) if use_rope else None
        xi = x.clone().requires_grad_(True)
        out = mod(xi, pos=pos if use_rope else None, mask=mask if use_mask else None)
        params = dict(mod.named_parameters())
        grads = torch.autograd.grad(0.5 * (out * out).sum(), [xi] + list(params.values()))
        cases[name] = {"mask": use_mask, "rope": use_rope, "out": out.detach(), "dx": grads[0],
                       "dparams": {k: g for k, g in zip(params, grads[1:]) if g.dim() == 1}}
    gold = {"num_heads": H, "base": 100.0, "eps": float(mod.q_norm.eps), "S": S, "P": P, "x": x, "pos": pos, "mask": mask,
            "weights": {k: v.detach().clone() for k, v in mod.state_dict().items()}, "cases": cases}
    torch.save(gold, HERE / "vggt_attention_goldens.pt")
    print("wrote", HERE / "vggt_attention_goldens.pt", (HERE / "vggt_attention_goldens.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
