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
the synchronising calls torch reports during one step (torch.cuda.set_sync_debug_mode("warn")).  Prints one JSON line
and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import warnings
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

CACHE_BYTES = 256 << 20
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
    first = one_set()
    set_bytes = sum(t.numel() * t.element_size() for t in first.values())
    nsets = max(2, -(-2 * CACHE_BYTES // set_bytes))
    sets = [first] + [one_set() for _ in range(nsets - 1)]
    fns = {"eager": eager, "front": front, "eager_repeat": eager}

    def step(var, s, between=None):
        out, lv = fns[var](s)
        if between is not None:
            between()
        return out, torch.autograd.grad(out, lv, s["up"])

    for var in VARIANTS[:2]:
        for i in range(warmup):
            step(var, sets[i % nsets])
    torch.cuda.synchronize()
    times = {var: [] for var in VARIANTS}
    for i in range(iters):                                                   # the variants alternate, on rotating buffers
        for vi, var in enumerate(VARIANTS):
            s = sets[(len(VARIANTS) * i + vi) % nsets]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(var, s)
            e1.record()
            e1.synchronize()
            times[var].append(e0.elapsed_time(e1))
    res = {"shape": name, "spec": SHAPES[name], "input_sets": nsets, "input_set_bytes": set_bytes,
           "parameters": sum(p.numel() for p in params.values()), "variants": {}}
    results = {}
    for var in VARIANTS:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        held = []
        out, grads = step(var, sets[0], lambda: held.append(torch.cuda.memory_allocated() - before))
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        results[var] = [out.detach().clone()] + [g.clone() for g in grads]
        del out, grads
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                step(var, sets[0])
            finally:
                torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        res["variants"][var] = {"ms_median": statistics.median(times[var]), "ms_min": min(times[var]), "ms_max": max(times[var]),
                                "bytes_allocated_peak": peak, "bytes_held_after_forward": held[0],
                                "host_syncs": sum("synchroniz" in str(w.message).lower() for w in caught),
                                "iters": iters, "warmup": warmup}
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))      # noqa: E731
    res["max_rel_diff_front_vs_eager"] = max(rel(x, y) for x, y in zip(results["front"], results["eager"]))
    ms = {var: res["variants"][var]["ms_median"] for var in VARIANTS}
    res["eager_spread_ms"] = abs(ms["eager"] - ms["eager_repeat"])
    res["gain_ms"] = min(ms["eager"], ms["eager_repeat"]) - ms["front"]
    res["speedup_front_over_eager"] = min(ms["eager"], ms["eager_repeat"]) / ms["front"]
    res["faster_beyond_spread"] = bool(res["gain_ms"] > res["eager_spread_ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "front_time.json"))
    args = ap.parse_args()
    if args.iters < 10 or args.warmup < 3:
        raise SystemExit("front_time.py: the median is taken over at least 10 steps after at least 3 warm-ups")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("front_time.py needs a GPU")
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    res = {"tool": "front_time", "device": torch.cuda.get_device_name(0), "results": []}
    for n in names:
        res["results"].append(run(n, args.warmup, args.iters))
        print(json.dumps(res["results"][-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
