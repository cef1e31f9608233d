"""Golden vectors of the DPT heads from the REFERENCE's own classes (build container only): ``PixelwiseTaskWithDPT`` of
heads/dpt_head.py and of heads/dpt_gs_head.py with heads/dpt_block.py and heads/postprocess.py, loaded by file path (the
heads directory is mounted as a package without running its ``__init__``; ``head_modules``, whose ``UnetExtractor``
dpt_gs_head.py imports and never uses, is a stub), on the CPU in float32.

feature_dim = 16, layer_dims = [8, 8, 16, 16], last_dim = 8, dim_tokens = [32, 24, 24, 24], hooks_idx = [0, 1, 2, 3],
B = 2, image 32 x 48: a patch grid of 2 x 3, so layer 4 is 1 x 2, ``refinenet4`` gives 2 x 4 and the crop to 2 x 3 runs.
  pts   num_channels = 4, head_type='regression', depth_mode=('exp', -inf, inf), conf_mode=('exp', 1, inf)
  gs    num_channels = 11, head_type='gs_params', no postprocess, a [2, 3, 32, 48] image; evaluation mode, because this
        head holds an ``nn.Dropout(0.1)``.  The reference builds ``input_merger`` with 256 output channels whatever
        ``feature_dim`` is, so its forward only runs at feature_dim = 256, whose weights would take 38 MB; here that one
        convolution is replaced by ``nn.Conv2d(3, 16, 7, 1, 3)`` before the weights are drawn.  The forward is the
        reference's.
Seeded inputs, the module's state dict, the outputs and the gradients of 0.5 * sum(out^2) over every output with respect
to every token tensor, the image and every parameter.

``post`` (in the pts file): the reference's ``postprocess`` on the pts head's raw output with three pixels per batch
item forced to d = 0, d = 1e-9 and d = 60, the outputs and the gradient with respect to that input.  The upstream
gradients are drawn and stored instead of being the outputs: at d = 60 the gradient of 0.5 * sum(out^2) is of the order
1e52 and overflows float32 in the reference itself.

Writes tests/golden/dpt_goldens_{pts,gs}.pt (data only).
    python tests/golden/make_dpt_goldens.py <reference checkout>
"""
import importlib
import sys
import types
from pathlib import Path

import torch
from torch import nn

HERE = Path(__file__).resolve().parent
INF = float("inf")
B, H, W, PATCH = 2, 32, 48, 16
ARGS = dict(feature_dim=16, layer_dims=[8, 8, 16, 16], last_dim=8, dim_tokens=[32, 24, 24, 24], hooks_idx=[0, 1, 2, 3])
DEPTH_MODE, CONF_MODE = ("exp", -INF, INF), ("exp", 1.0, INF)
# (batch item, row, column) -> xyz of the forced pixels: d = 0, 1e-9, 60
FORCED = {(0, 0, 0): (0.0, 0.0, 0.0), (0, 5, 7): (6e-10, -8e-10, 0.0), (0, 31, 47): (36.0, -48.0, 0.0),
          (1, 16, 1): (0.0, 0.0, 0.0), (1, 3, 40): (0.0, 6e-10, 8e-10), (1, 20, 20): (-48.0, 0.0, 36.0)}


def mount(name, directory):
    """``directory`` as package ``name`` without its __init__ (which would import every head)."""
    pkg = types.ModuleType(name)
    pkg.__path__ = [str(directory)]
    sys.modules[name] = pkg
    return pkg


def main(ref_root):
    mount("ref_heads", Path(ref_root) / "src/model/encoder/heads")
    stub = types.ModuleType("ref_heads.head_modules")
    stub.UnetExtractor = None
    sys.modules["ref_heads.head_modules"] = stub
    pts_mod = importlib.import_module("ref_heads.dpt_head")
    gs_mod = importlib.import_module("ref_heads.dpt_gs_head")
    postprocess = importlib.import_module("ref_heads.postprocess").postprocess
    gen = torch.Generator().manual_seed(31)

    def init(mod):
        with torch.no_grad():
            for p in mod.parameters():
                if p.dim() > 1:
                    p.copy_(torch.randn(p.shape, generator=gen) * (p[0].numel() ** -0.5))
                else:
                    p.copy_(0.1 * torch.randn(p.shape, generator=gen))
        return mod

    def record(kind, mod, ins, run):
        leaves = {k: v.clone().requires_grad_(True) for k, v in ins.items()}
        params = dict(mod.dpt.named_parameters())
        outs = run(mod, leaves)
        loss = sum(0.5 * (o * o).sum() for o in outs.values())
        wrt = list(leaves.values()) + list(params.values())
        # (refinenet4 has one input: its resConfUnit1 takes no part and gets a zero gradient)
        grads = [torch.zeros_like(t) if g is None else g for t, g in zip(wrt, torch.autograd.grad(loss, wrt, allow_unused=True))]
        return {"kind": kind, "image_size": (H, W), "patch": PATCH, "args": dict(ARGS), "inputs": ins,
                "weights": {k: v.detach().clone() for k, v in mod.state_dict().items()},
                "out": {k: v.detach() for k, v in outs.items()}, "grads": dict(zip(leaves, grads[:len(leaves)])),
                "pgrads": dict(zip(params, grads[len(leaves):]))}

    def tokens():
        n = (H // PATCH) * (W // PATCH)
        return {f"tok{i}": torch.randn(B, n, c, generator=gen) for i, c in enumerate(ARGS["dim_tokens"])}

    def toks(t):
        return [t[f"tok{i}"] for i in range(4)]

    pts = init(pts_mod.PixelwiseTaskWithDPT(num_channels=4, postprocess=postprocess, depth_mode=DEPTH_MODE,
                                            conf_mode=CONF_MODE, head_type="regression", **ARGS))
    gold = record("pts", pts, tokens(), lambda m, t: m(toks(t), (H, W)))
    gold["num_channels"], gold["depth_mode"], gold["conf_mode"] = 4, DEPTH_MODE, CONF_MODE
    with torch.no_grad():
        raw = pts.dpt(toks(gold["inputs"]), image_size=(H, W)).clone()
    for (b, y, x), xyz in FORCED.items():
        raw[b, :3, y, x] = torch.tensor(xyz)
    raw.requires_grad_(True)
    res = postprocess(raw, DEPTH_MODE, CONF_MODE)
    ups = {"pts3d": torch.randn(res["pts3d"].shape, generator=gen), "conf": torch.randn(res["conf"].shape, generator=gen)}
    (din,) = torch.autograd.grad([res["pts3d"], res["conf"]], [raw], [ups["pts3d"], ups["conf"]])
    gold["post"] = {"in": raw.detach(), "forced": sorted(FORCED), "ups": ups,
                    "out": {k: v.detach() for k, v in res.items()}, "din": din}
    torch.save(gold, HERE / "dpt_goldens_pts.pt")

    gs = gs_mod.PixelwiseTaskWithDPT(num_channels=11, postprocess=None, head_type="gs_params", **ARGS)
    gs.dpt.input_merger = nn.Sequential(nn.Conv2d(3, ARGS["feature_dim"], 7, 1, 3), nn.ReLU())
    init(gs).eval()
    ins = tokens()
    ins["img"] = torch.rand(B, 3, H, W, generator=gen)
    gold = record("gs", gs, ins, lambda m, t: {"out": m(toks(t), t["img"], (H, W))})
    gold["num_channels"] = 11
    torch.save(gold, HERE / "dpt_goldens_gs.pt")
    for f in ("pts", "gs"):
        p = HERE / f"dpt_goldens_{f}.pt"
        print("wrote", p, p.stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
