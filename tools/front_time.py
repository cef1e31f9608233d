"""Time the step "images -> tokens, forward + backward to every parameter": the encoder front of csrc/front.hip against
the reference's own eager lines, on one GPU.

    python tools/front_time.py [--warmup 5] [--iters 20] [--shapes all|name,name] [--out profiles/front_time.json]

Shapes:
  croco_256    48 images 3 x 256 x 256, P = 16, C = 1024, ImageNet mean / std, no extra rows
  assemble     ``assemble_tokens`` on a [16, 3, 256, 1024] body with two ``after`` tokens (one per sequence, one broadcast)
  vggt_224     48 images 3 x 224 x 224, P = 14, C = 1024, pos table, cls + per-image intrinsics + 4 registers in front
Variants, alternated step by step in one run on one device:
  eager         the reference's lines: ``(x - mean) / std``, ``nn.Conv2d``, ``flatten(2).transpose(1, 2)``, the additions
                and the ``cat``s (never the code under test)
  front         ``spfsplatv2_amd.embed_patches`` / ``assemble_tokens``
  eager_repeat  `eager` a second time in the same rotation: the spread of two runs of one variant, which a difference
                between `eager` and `front` has to exceed to mean anything
A step is the forward and the backward of a given upstream gradient to every parameter (and the body, for `assemble`).

Times: device events around each step, median over --iters after --warmup; the inputs and upstream gradients rotate over
enough sets to exceed twice the 256 MB last-level cache (cold buffers).  Bytes: the peak of torch's allocator during one
step above what was allocated before it, and what is still allocated between the forward and the backward.  Host syncs:
the synchronising calls torch reports during one step (steptime.count_syncs).  Prints one JSON line
and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# name: (kind, images or (b, v), H = W or N, patch, C)
SHAPES = {"croco_256": ("croco", 48, 256, 16, 1024), "assemble": ("assemble", (16, 3), 256, 0, 1024),
          "vggt_224": ("vggt", 48, 224, 14, 1024)}
VARIANTS = ("eager", "front", "eager_repeat")


def make(name, dev, gen):
    """(parameters {name: leaf}, input sets, eager step, front step); a step returns (out, gradients)."""
    import torch
    from torch import nn

    import spfsplatv2_amd as spf
    kind, b, size, p, c = SHAPES[name]
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)               # noqa: E731
    leaf = lambda t: t.requires_grad_(True)                                  # noqa: E731
    if kind == "assemble":
        bb, v = b
        params = {"pose": leaf(rn(1, 1, c))}

        def one_set():
            return {"x": leaf(rn(bb, v, size, c)), "intr": leaf(rn(bb, v, 1, c)), "up": rn(bb, v, size + 2, c)}

        def eager(s):
            out = torch.cat((s["x"], s["intr"], params["pose"].expand(bb, v, -1, -1)), dim=2)
            return out, (s["x"], s["intr"], params["pose"])

        def front(s):
            return spf.assemble_tokens(s["x"], after=[s["intr"], params["pose"]]), (s["x"], s["intr"], params["pose"])
        return params, one_set, eager, front
    conv = nn.Conv2d(3, c, p, p).to(dev)
    n = (size // p) ** 2
    params = {"weight": conv.weight, "bias": conv.bias}
    mean = torch.tensor(MEAN, device=dev).view(-1, 1, 1)
    std = torch.tensor(STD, device=dev).view(-1, 1, 1)
    if kind == "vggt":
        params.update(cls=leaf(rn(1, 1, c)), registers=leaf(rn(1, 4, c)), pos_table=leaf(rn(n, c)), pos_first=leaf(rn(c)))
    extra = 6 if kind == "vggt" else 0

    def one_set():
        s = {"image": torch.rand(b, 3, size, size, device=dev, generator=gen), "up": rn(b, extra + n, c)}
        if kind == "vggt":
            s["intr"] = leaf(rn(b, 1, c))
        return s

    def leaves(s):
        return tuple(params.values()) + ((s["intr"],) if kind == "vggt" else ())

    def eager(s):
        x = conv((s["image"] - mean) / std).flatten(2).transpose(1, 2)
        if kind == "vggt":                                                   # prepare_tokens_with_masks, masks=None
            x = torch.cat((params["cls"].expand(b, -1, -1), x), dim=1)
            x = x + torch.cat((params["pos_first"].view(1, 1, c), params["pos_table"].unsqueeze(0)), dim=1)
            x = torch.cat((x[:, :1], params["registers"].expand(b, -1, -1), x[:, 1:]), dim=1)
            x = torch.cat((x[:, :1], s["intr"], x[:, 1:]), dim=1)
        return x, leaves(s)

    def front(s):
        if kind == "vggt":
            out = spf.embed_patches(s["image"], conv.weight, conv.bias, patch=p, mean=MEAN, std=STD, pos_table=params["pos_table"],
                                    pos_first=params["pos_first"], before=[params["cls"], s["intr"], params["registers"]])
        else:
            out = spf.embed_patches(s["image"], conv.weight, conv.bias, patch=p, mean=MEAN, std=STD)
        return out, leaves(s)
    return params, one_set, eager, front


def run(name, warmup, iters):
    import torch
    dev = torch.device("cuda")
    gen = torch.Generator(dev).manual_seed(0)
    params, one_set, eager, front = make(name, dev, gen)
    sets, set_bytes = steptime.input_sets(one_set)
    fns = {"eager": eager, "front": front, "eager_repeat": eager}

    def step(var):
        def run_step(s, between=None):
            out, lv = fns[var](s)
            if between is not None:
                between()
            return [out.detach(), *torch.autograd.grad(out, lv, s["up"])]
        return run_step

    res = {"shape": name, "spec": SHAPES[name], "input_sets": len(sets), "input_set_bytes": set_bytes,
           "parameters": sum(p.numel() for p in params.values())}
    res["variants"], results = steptime.alternate(VARIANTS, {var: step(var) for var in VARIANTS}, sets, warmup, iters,
                                                  warm=VARIANTS[:2], held=True, syncs=True, ms_max=True)
    res["max_rel_diff_front_vs_eager"] = steptime.max_rel_diff(results["front"], results["eager"])
    ms = {var: res["variants"][var]["ms_median"] for var in VARIANTS}
    spread = steptime.spread_summary(ms["eager"], ms["front"], ms["eager_repeat"])
    res.update(eager_spread_ms=spread["spread_ms"], gain_ms=spread["gain_ms"], speedup_front_over_eager=spread["speedup"],
               faster_beyond_spread=spread["faster_beyond_spread"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "front_time.json"))
    args = ap.parse_args()
    steptime.require_counts("front_time", args, 10, 3)
    res = steptime.require_gpu("front_time")
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    res["results"] = [steptime.note(run(n, args.warmup, args.iters)) for n in names]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
