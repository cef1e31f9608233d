"""Time forward + backward of the DPT heads: this package's heads against the same heads assembled from eager
operations, on one GPU.

    python tools/dpt_time.py [--warmup 5] [--iters 20] [--shapes all|name,name] [--batch 16] [--out profiles/dpt_time.json]

Variants, alternated step by step in one run on one device:
  baseline         the path available without csrc/dpt.hip: the same modules and weights with the reference's forwards
                   (dpt_block.py:121-142 / 189-218 / 247-262, dpt_gs_head.py:71-73) on eager nn.ReLU, F.interpolate and
                   tensor adds, and the reference's postprocess expression (postprocess.py:11-78) in eager torch
  fused            spfsplatv2_amd.PixelwiseTaskWithDPT / PixelwiseTaskWithGSDPT
  baseline_repeat  `baseline` a second time in the same rotation: the spread of two runs of one variant, which a difference
                   between `baseline` and `fused` has to exceed to mean anything
A step is the head's forward and the backward of a given upstream gradient to the four token tensors, the image and
every parameter.  The heads are those ``head_factory`` builds for the reference's encoder: feature_dim = 256,
dim_tokens = [1024, 768, 768, 768], a 256 x 256 image (a 16 x 16 patch grid), 3 point channels with
depth_mode=('exp', -inf, inf) and no confidence, 83 raw Gaussian channels.

Times: device events around each step, median over --iters after --warmup (a step is hundreds of milliseconds, so the
defaults are lower than the block tool's); every activation of a step is far larger than the 256 MB last-level cache,
and the tokens and the image rotate over two sets.  Bytes: the peak of torch's allocator during one step above what was
allocated before it, and what is still allocated between the forward and the backward (the saved activations); the
operands and upstream gradients the fused calls had to copy because they did not arrive dense (heads.dense_copies).  Prints
one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import copy
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

SHAPES = {"pts_256_256x256": "pts", "gs_256_256x256": "gs"}
VARIANTS = ("baseline", "fused", "baseline_repeat")
IMAGE = 256
INF = float("inf")


class Net:
    dec_depth, enc_embed_dim, dec_embed_dim = 12, 1024, 768
    depth_mode, conf_mode = ("exp", -INF, INF), None


def eager_twin(mod):
    """A copy of ``mod`` whose submodules run the reference's forwards on eager torch operations."""
    import torch.nn.functional as F

    from spfsplatv2_amd import heads

    def eager_postprocess(out, depth_mode, conf_mode):
        """postprocess.py:11-78 for the 'exp' modes, one eager kernel per piece"""
        fmap = out.permute(0, 2, 3, 1)
        xyz = fmap[..., 0:3]
        d = xyz.norm(dim=-1, keepdim=True)
        e = d.expm1()
        if (depth_mode[1], depth_mode[2]) != (-INF, INF):
            e = e.clip(min=depth_mode[1], max=depth_mode[2])
        res = dict(pts3d=xyz / d.clip(min=1e-8) * e)
        if conf_mode is not None:
            res["conf"] = conf_mode[1] + fmap[..., 3].exp().clip(max=conf_mode[2] - conf_mode[1])
        return res

    class Unit(heads.ResidualConvUnit_custom):
        def forward(self, x):
            out = self.conv1(self.activation(x))
            return self.conv2(self.activation(out)) + x

    class Fusion(heads.FeatureFusionBlock_custom):
        def forward(self, *xs):
            output = xs[0]
            if len(xs) == 2:
                output = output + self.resConfUnit1(xs[1])
            output = self.resConfUnit2(output)
            output = F.interpolate(output, scale_factor=2, mode="bilinear", align_corners=self.align_corners)
            return self.out_conv(output)

    class Interp(heads.Interpolate):
        def forward(self, x):
            return F.interpolate(x, scale_factor=self.scale_factor, mode=self.mode, align_corners=self.align_corners)

    class Adapter(heads.DPTOutputAdapter):
        def forward_gs(self, encoder_tokens, imgs, image_size=None, conf=None):
            path_1 = self._path_1(encoder_tokens, image_size)
            direct_img_feat = self.input_merger(imgs)
            path_1 = self.feat_up(path_1)
            return self.head(path_1 + direct_img_feat)

    swap = {heads.ResidualConvUnit_custom: Unit, heads.FeatureFusionBlock_custom: Fusion, heads.Interpolate: Interp,
            heads.DPTOutputAdapter: Adapter}
    twin = copy.deepcopy(mod)
    for m in twin.modules():
        if type(m) in swap:
            m.__class__ = swap[type(m)]
    if twin.postprocess is not None:
        twin.postprocess = eager_postprocess
    return twin


def make_set(kind, B, gen, dev):
    import torch
    n = (IMAGE // 16) ** 2
    s = {"tokens": [None] * (Net.dec_depth + 1)}
    for hook, c in zip((0, 6, 9, 12), (1024, 768, 768, 768)):
        s["tokens"][hook] = torch.randn(B, n, c, generator=gen).to(dev).requires_grad_(True)
    if kind == "gs":
        s["img"] = torch.rand(B, 3, IMAGE, IMAGE, generator=gen).to(dev).requires_grad_(True)
    return s


def forward(kind, mod, s):
    if kind == "pts":
        return mod(s["tokens"], (IMAGE, IMAGE))["pts3d"]
    return mod(s["tokens"], s["img"], (IMAGE, IMAGE))


def step(kind, mod, s, dout, between=None):
    """forward + backward to the tokens, the image and every parameter that takes part"""
    import torch
    out = forward(kind, mod, s)
    if between is not None:
        between()
    wrt = [t for t in s["tokens"] if t is not None] + ([s["img"]] if kind == "gs" else [])
    wrt += [p for n, p in mod.named_parameters() if "refinenet4.resConfUnit1" not in n]
    return out, torch.autograd.grad(out, wrt, dout)


def run(name, B, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    from spfsplatv2_amd import heads
    kind = SHAPES[name]
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    fused = spf.head_factory("dpt" if kind == "pts" else "dpt_gs", "pts3d" if kind == "pts" else "gs_params", Net(),
                             has_conf=False, out_nchan=83).to(dev).eval()
    with torch.no_grad():                                               # outputs of order one: expm1 stays in range
        for p in fused.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=gen).to(dev) * (p[0].numel() ** -0.5))
    mods = {"fused": fused, "baseline": eager_twin(fused)}
    mods["baseline_repeat"] = mods["baseline"]
    sets = [make_set(kind, B, gen, dev) for _ in range(2)]
    with torch.no_grad():
        shape = forward(kind, fused, sets[0]).shape
    dout = torch.randn(shape, generator=gen).to(dev)
    res = {"shape": name, "kind": kind, "B": B, "image": IMAGE, "feature_dim": 256, "output": list(shape),
           "parameters": sum(p.numel() for p in fused.parameters())}
    copied = {}                                     # per variant, the operands its latest step had to copy

    def counted(var):
        def run_step(s, between=None):
            before = dict(heads.dense_copies)
            out, grads = step(kind, mods[var], s, dout, between)
            copied[var] = {k: heads.dense_copies[k] - v for k, v in before.items()}
            return [out.detach(), *grads]
        return run_step
    res["variants"], results = steptime.alternate(VARIANTS, {var: counted(var) for var in VARIANTS}, sets, warmup, iters,
                                                  warm=VARIANTS[:2], held=True, label=name)
    for var, rec in res["variants"].items():        # (the bytes step is a variant's last)
        rec.update(dense_copies=copied[var]["calls"], dense_copy_bytes=copied[var]["bytes"])
    # the two paths compute one function: the largest relative difference over the output and every gradient, next to
    # the same figure between the two runs of the eager path (what the convolutions' own backward leaves undetermined)
    names = ["out"] + [f"d_tokens[{h}]" for h in (0, 6, 9, 12)] + (["d_img"] if kind == "gs" else [])
    names += ["d_" + n for n, _ in fused.named_parameters() if "refinenet4.resConfUnit1" not in n]

    def diffs(a, b):
        return {n: steptime.rel_diff(x, y) for n, x, y in zip(names, results[a], results[b])}
    for key, d in (("fused_vs_baseline", diffs("fused", "baseline")), ("baseline_repeat_vs_baseline", diffs("baseline_repeat", "baseline"))):
        res["max_rel_diff_" + key] = max(d.values())
        res["rel_diff_out_" + key] = d["out"]
        res["largest_rel_diffs_" + key] = dict(sorted(d.items(), key=lambda kv: -kv[1])[:4])
    ms = {var: res["variants"][var]["ms_median"] for var in VARIANTS}
    spread = steptime.spread_summary(ms["baseline"], ms["fused"], ms["baseline_repeat"])
    res.update(baseline_spread_ms=spread["spread_ms"], gain_ms=spread["gain_ms"], speedup_fused_over_baseline=spread["speedup"])
    res["bytes_held_saved"] = res["variants"]["baseline"]["bytes_held_after_forward"] - res["variants"]["fused"]["bytes_held_after_forward"]
    res["bytes_peak_saved"] = res["variants"]["baseline"]["bytes_allocated_peak"] - res["variants"]["fused"]["bytes_allocated_peak"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dpt_time.json"))
    args = ap.parse_args()
    steptime.require_counts("dpt_time", args, 10, 3)
    res = steptime.require_gpu("dpt_time")
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    res["results"] = [steptime.note(run(n, args.batch, args.warmup, args.iters)) for n in names]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
