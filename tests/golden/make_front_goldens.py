"""Golden vectors of the encoder front from the REFERENCE's own classes (build container only): ``PatchEmbedDust3R`` of
croco/patch_embed.py, VGGT's ``PatchEmbed`` of vggt/layers/patch_embed.py and ``prepare_tokens_with_masks`` of a
``DinoVisionTransformer`` small enough to commit (vggt/layers/vision_transformer.py; the directories are mounted as
packages without their __init__, as make_block_goldens.py does), plus the token / position appends of
``_encode_image`` and ``_decoder`` (backbone_masked_croco.py:161-172, 186-201) and ``normalize_image``
(dataset/shims/normalize_shim.py:15-18), re-run here through the same tensor statements on the reference's outputs.
Writes tests/golden/front_goldens.pt.   python tests/golden/make_front_goldens.py [reference root]
"""
import importlib
import sys
import types
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def mount(name, directory):
    for m in ("timm", "timm.models", "timm.models.layers"):
        sys.modules.setdefault(m, types.ModuleType(m))
    pkg = types.ModuleType(name)
    pkg.__path__ = [str(directory)]
    sys.modules[name] = pkg
    return pkg


def normalize_image(tensor, mean, std):
    mean = torch.as_tensor(mean, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
    std = torch.as_tensor(std, dtype=tensor.dtype, device=tensor.device).view(-1, 1, 1)
    return (tensor - mean) / std


def main(ref_root):
    backbone = Path(ref_root) / "src/model/encoder/backbone"
    mount("ref_croco", backbone / "croco")
    mount("ref_vggt_layers", backbone / "vggt/layers")
    Dust3R = importlib.import_module("ref_croco.patch_embed").PatchEmbedDust3R
    VPatch = importlib.import_module("ref_vggt_layers.patch_embed").PatchEmbed
    Dino = importlib.import_module("ref_vggt_layers.vision_transformer").DinoVisionTransformer
    gen = torch.Generator().manual_seed(61)
    rand = lambda *s: torch.rand(*s, generator=gen)        # noqa: E731
    randn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731

    def init(params):
        with torch.no_grad():
            for p in params:
                p.copy_(randn(*p.shape) * (p[0].numel() ** -0.5 if p.dim() == 4 else 1.0))

    def grads(out, up, leaves):
        got = torch.autograd.grad((out * up).sum(), list(leaves.values()))
        return {k: g.detach() for k, g in zip(leaves, got)}

    out = {"mean": MEAN, "std": STD}

    # --- PatchEmbedDust3R((32, 48), 16, 3, 64) and the encoder's appends behind it
    mod = Dust3R((32, 48), 16, 3, 64)
    init(mod.parameters())
    image = rand(2, 3, 32, 48)
    tokens, pos = mod(normalize_image(image, MEAN, STD), true_shape=None)
    up = randn(*tokens.shape)
    out["dust3r"] = {"args": ((32, 48), 16, 3, 64), "state": {k: v.detach().clone() for k, v in mod.state_dict().items()},
                     "image": image, "tokens": tokens.detach(), "pos": pos, "up": up,
                     "grads": grads(tokens, up, dict(mod.named_parameters()))}
    intr = randn(2, 1, 64).requires_grad_(True)            # per image (intrinsic_encoder's output)
    pose = randn(1, 1, 64).requires_grad_(True)            # a parameter broadcast over the images
    x, p = mod(normalize_image(image, MEAN, STD), true_shape=None)
    x = torch.cat((x, intr), dim=1)
    add_pos = p[:, 0:1, :].clone()
    add_pos[:, :, 0] += (p[:, -1, 0].unsqueeze(-1) + 1)
    p = torch.cat((p, add_pos), dim=1)
    x = torch.cat((x, pose.expand(2, -1, -1)), dim=1)
    add_pos = p[:, 0:1, :].clone()
    add_pos[:, :, 0] += (p[:, -1, 0].unsqueeze(-1) + 1)
    p = torch.cat((p, add_pos), dim=1)
    up = randn(*x.shape)
    out["encode_image"] = {"intrinsics_embed": intr.detach(), "pose_embedding": pose.detach(), "tokens": x.detach(), "pos": p,
                           "up": up, "grads": grads(x, up, {"proj.bias": mod.proj.bias, "intrinsics_embed": intr,
                                                            "pose_embedding": pose})}
    # --- _decoder: feat [b, v, l, c], the tokens appended along dim 2
    feat = randn(2, 3, 6, 64).requires_grad_(True)
    fpos = torch.stack([torch.stack((torch.arange(6) // 3, torch.arange(6) % 3), dim=-1)] * 3)[None].repeat(2, 1, 1, 1)
    intr = randn(2, 3, 1, 64).requires_grad_(True)
    pose = randn(1, 1, 1, 64).requires_grad_(True)
    f = torch.cat((feat, intr), dim=2)
    add_pos = fpos[:, :, 0:1, :].clone()
    add_pos[:, :, :, 0] += (fpos[:, :, -1, 0].unsqueeze(-1) + 1)
    p = torch.cat((fpos, add_pos), dim=2)
    f = torch.cat((f, pose.expand(2, 3, -1, -1)), dim=2)
    add_pos = p[:, :, 0:1, :].clone()
    add_pos[:, :, :, 0] += (p[:, :, -1, 0].unsqueeze(-1) + 1)
    p = torch.cat((p, add_pos), dim=2)
    up = randn(*f.shape)
    out["decoder"] = {"feat": feat.detach(), "pos_in": fpos, "intrinsics_embed": intr.detach(), "pose_embedding": pose.detach(),
                      "tokens": f.detach(), "pos": p, "up": up,
                      "grads": grads(f, up, {"feat": feat, "intrinsics_embed": intr, "pose_embedding": pose})}

    # --- VGGT's PatchEmbed, patch 14 on 28 x 42
    mod = VPatch((28, 42), 14, 3, 64)
    init(mod.parameters())
    image = rand(2, 3, 28, 42)
    tokens = mod(normalize_image(image, MEAN, STD))
    up = randn(*tokens.shape)
    out["vggt_patch"] = {"args": ((28, 42), 14, 3, 64), "state": {k: v.detach().clone() for k, v in mod.state_dict().items()},
                         "image": image, "tokens": tokens.detach(), "up": up,
                         "grads": grads(tokens, up, dict(mod.named_parameters()))}

    # --- prepare_tokens_with_masks of a small DinoVisionTransformer: a 5 x 5 pos_embed table, 4 registers
    cfg = dict(img_size=70, patch_size=14, in_chans=3, embed_dim=64, depth=1, num_heads=2, num_register_tokens=4,
               interpolate_antialias=True, interpolate_offset=0.0)
    vit = Dino(**cfg)
    keep = {"cls_token": vit.cls_token, "pos_embed": vit.pos_embed, "register_tokens": vit.register_tokens,
            "patch_embed.proj.weight": vit.patch_embed.proj.weight, "patch_embed.proj.bias": vit.patch_embed.proj.bias}
    init(keep.values())
    vit.patch_embed.load_state_dict(mod.state_dict())      # the patch weights are vggt_patch's: stored once
    assert tuple(vit.pos_embed.shape) == (1, 26, 64)
    out["dino"] = {"cfg": cfg, "state": {k: v.detach().clone() for k, v in keep.items() if "proj" not in k}, "image": image}
    for name, with_intr in (("plain", False), ("intrinsics", True)):
        intr = randn(2, 1, 64).requires_grad_(True) if with_intr else None
        x = vit.prepare_tokens_with_masks(normalize_image(image, MEAN, STD), None, intr)
        up = randn(*x.shape)
        # (no weight gradient here, the one large tensor: vggt_patch has it for these weights, and the file stays under 1 MB)
        leaves = {k: v for k, v in keep.items() if "weight" not in k}
        if with_intr:
            leaves["intrinsic_embedding"] = intr
        out["dino"][name] = {"intrinsic_embedding": intr.detach() if with_intr else None, "tokens": x.detach(), "up": up,
                             "grads": grads(x, up, leaves)}
    torch.save(out, HERE / "front_goldens.pt")
    print("wrote", HERE / "front_goldens.pt", (HERE / "front_goldens.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "/root/reference")
