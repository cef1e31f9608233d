"""Golden vectors of the pose heads from the REFERENCE's own classes (build container only): ``PoseHead`` of
model/encoder/heads/pose_head.py, loaded by file path, and VGGT's ``CameraHead`` of vggt/heads/camera_head.py with the
``Block``, ``Attention``, ``LayerScale``, ``Mlp`` and ``activate_pose`` the reference vendors next to it (the vggt
directory and its ``heads`` and ``layers`` are mounted as packages without running their ``__init__``), on the CPU in
float32.

``PoseHead`` (concat_enc, use_homogeneous, pose_init_t) = (True, True, False) with 24 encoder and 16 decoder channels, 4
tokens, 3 scenes; and (False, False, True) with 16 decoder channels and one token -- its zero ``fc_rot`` weights give the
rows 1 0 0 0 1 0.  ``CameraHead(dim_in=128, num_heads=1, trunk_depth=2, mlp_ratio=2)`` on a list of two [2, 3, 5, 128]
token tensors, four iterations, all four outputs.  Seeded inputs, the module's state dict, the outputs and the gradients
of 0.5 * sum(out^2) (over all outputs) with respect to the inputs.

Writes tests/golden/posehead_goldens_{mlp,camera}.pt (data only) and the camera head's state dict as
posehead_goldens_camera_weights_{0,1}.pt (``trunk.0.*`` and the rest): in one file it would exceed the size the
repository allows.
    python tests/golden/make_posehead_goldens.py <reference checkout>
"""
import importlib
import importlib.util
import sys
import types
from pathlib import Path
from types import SimpleNamespace

import torch

HERE = Path(__file__).resolve().parent


def load(name, path):
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


def record(kind, mod, ins, run, **extra):
    leaves = {k: v.clone().requires_grad_(True) for k, v in ins.items()}
    outs = run(mod, leaves)
    grads = torch.autograd.grad(sum(0.5 * (o * o).sum() for o in outs), list(leaves.values()), allow_unused=True)
    grads = [torch.zeros_like(v) if g is None else g for g, v in zip(grads, leaves.values())]
    return {"kind": kind, "inputs": ins, "weights": {k: v.detach().clone() for k, v in mod.state_dict().items()},
            "keys": list(mod.state_dict()), "param_names": [k for k, _ in mod.named_parameters()],
            "outs": [o.detach() for o in outs], "grads": dict(zip(leaves, grads)), **extra}


def main(ref_root):
    enc_dir = Path(ref_root) / "src/model/encoder"
    ref = load("ref_pose_head", enc_dir / "heads/pose_head.py")
    vggt = enc_dir / "backbone/vggt"
    mount("ref_vggt", vggt)
    mount("ref_vggt.heads", vggt / "heads")
    mount("ref_vggt.layers", vggt / "layers")
    RefCameraHead = importlib.import_module("ref_vggt.heads.camera_head").CameraHead
    gen = torch.Generator().manual_seed(31)

    def tokens(*shape):
        """std 0.05 about a per-row mean near 0.3, as the norm rows of the kernel cases"""
        return 0.3 + 0.1 * torch.randn(*shape[:-1], 1, generator=gen) + 0.05 * torch.randn(*shape, generator=gen)

    def init(mod, skip=()):
        with torch.no_grad():
            for n, p in mod.named_parameters():
                if n.startswith(skip):
                    continue
                if "norm" in n and n.endswith("weight"):
                    p.copy_(1.0 + 0.3 * torch.randn(p.shape, generator=gen))
                elif n.endswith("gamma"):
                    p.copy_(0.1 + 0.03 * torch.randn(p.shape, generator=gen))
                else:
                    p.copy_(torch.randn(p.shape, generator=gen) * (p.shape[-1] ** -0.5 if p.dim() == 2 else 0.1))
        return mod

    cases = []
    for (concat_enc, homog, init_t), enc_c, dec_c, L in (((True, True, False), 24, 16, 4), ((False, False, True), 0, 16, 1)):
        cfg = ref.PoseHeadCfg(pose_init_t=init_t, use_homogeneous=homog, concat_enc=concat_enc)
        head = ref.PoseHead(SimpleNamespace(enc_embed_dim=enc_c, dec_embed_dim=dec_c), cfg)
        # ``init_pose`` stands: zero fc_rot weights, and a zero fc_t with pose_init_t
        init(head, skip=("fc_rot",) + (("fc_t",) if init_t else ()))
        ins = {"dec": tokens(3, L, dec_c)}
        order = ["dec"]
        if concat_enc:
            ins, order = {"enc": tokens(3, L, enc_c), **ins}, ["enc", "dec"]
        cases.append(record("mlp", head, ins, lambda m, t, order=order: [m([t[k] for k in order])], token_order=order,
                            cfg=dict(pose_init_t=init_t, use_homogeneous=homog, concat_enc=concat_enc),
                            enc_embed_dim=enc_c, dec_embed_dim=dec_c))
    assert torch.equal(cases[1]["outs"][0][:, :6], torch.tensor([1., 0, 0, 0, 1, 0]).expand(3, 6))
    torch.save({"cases": cases}, HERE / "posehead_goldens_mlp.pt")

    cfg = dict(dim_in=128, num_heads=1, trunk_depth=2, mlp_ratio=2, init_values=0.01, trans_act="linear", quat_act="linear",
               fl_act="relu")
    cam = init(RefCameraHead(**cfg))
    other, last = tokens(2, 3, 5, 128), tokens(2, 3, 5, 128)
    gold = record("camera", cam, {"tokens": last}, lambda m, t: m([other, t["tokens"]], num_iterations=4), cfg=cfg,
                  num_iterations=4, other_tokens=other)
    weights = gold.pop("weights")
    torch.save({"weights": {k: v for k, v in weights.items() if k.startswith("trunk.0.")}},
               HERE / "posehead_goldens_camera_weights_0.pt")
    torch.save({"weights": {k: v for k, v in weights.items() if not k.startswith("trunk.0.")}},
               HERE / "posehead_goldens_camera_weights_1.pt")
    torch.save(gold, HERE / "posehead_goldens_camera.pt")
    for f in ("mlp", "camera", "camera_weights_0", "camera_weights_1"):
        p = HERE / f"posehead_goldens_{f}.pt"
        print("wrote", p, p.stat().st_size, "bytes")
        assert p.stat().st_size < 1 << 20, p


if __name__ == "__main__":
    main(sys.argv[1])
