"""Time the step "head outputs -> Gaussians, forward + backward": the encoder tail of csrc/tail.hip against the path
available without it, on one GPU.

    python tools/tail_time.py [--warmup 5] [--iters 20] [--shapes all|name,name] [--decoder-batch N] [--out profiles/tail_time.json]

Variants, alternated step by step in one run on one device:
  baseline         what a caller runs without the tail: per view rearrange "b d h w -> b (h w) d", torch.stack over the
                   views, sigmoid and the opacity map in eager torch, then ``UnifiedGaussianAdapter`` (the row kernels)
  tail             ``spfsplatv2_amd.gaussians_from_heads``
  baseline_repeat  `baseline` a second time in the same rotation: the spread of two runs of one variant, which a difference
                   between `baseline` and `tail` has to exceed to mean anything
A step is the forward and the backward of given upstream gradients (means, opacities, scales, rotations, harmonics; under
the band split none for band 4, as a decoder that evaluates to degree 3 returns none) to the 2 v head tensors.  Each shape
is timed with dense and with band-split harmonics.

With --decoder-batch N > 0 a second group is timed on a renderable scene of N batch items (the head outputs are the ones
the adapter maps back onto ``synthetic.make_batch``'s Gaussians): one ``DecoderSplattingCUDA`` step, forward + backward of
a weighted image sum to the head outputs, behind
  fused_decoder         the eager rearrange / stack / sigmoid / map + ``UnifiedGaussianAdapter(fuse_into_decoder=True)``:
                        the decoder reads the stacked raw rows, so the transposing copy is what this mode costs its caller
  tail_decoder          ``gaussians_from_heads`` (band-split) + the decoder
  fused_decoder_repeat  the spread of `fused_decoder`.

Times: device events around each step, median over --iters after --warmup; the head outputs of a step are far larger
than the 256 MB last-level cache and rotate over two sets (cold buffers).  Bytes: the peak of torch's allocator during
one step above what was allocated before it, and what is still allocated between the forward and the backward.  Prints
one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

# name: (b, v, h, w, synthetic config of the decoder group)
SHAPES = {"b16_v2_256x256": (16, 2, 256, 256, "REF2V"), "b4_v10_256x256": (4, 10, 256, 256, "REF10V")}
VARIANTS = ("baseline", "tail", "baseline_repeat")
DEC_VARIANTS = ("fused_decoder", "tail_decoder", "fused_decoder_repeat")
SH_DEGREE, K, C = 4, 25, 83
EXPONENT = 2.0 ** 0.5
FIELDS = ("means", "opacities", "scales", "rotations", "harmonics")


def eager_rows(pts, raw, exponent):
    """encoder_spfsplatv2.py:218-224, 240, 248-250, 257 and map_pdf_to_opacity in eager torch: the stacked rows
    [b, v, hw, C], the stacked points [b, v, hw, 3] and the opacities [b, v, hw]"""
    import torch
    g = torch.stack([r.flatten(2).transpose(1, 2) for r in raw], dim=1)
    pts_all = torch.stack(list(pts), dim=1).flatten(2, 3)
    pdf = g[..., 0].sigmoid()
    return g, pts_all, 0.5 * (1 - (1 - pdf) ** exponent + pdf ** (1 / exponent))


def baseline_gaussians(adapter_mod, pts, raw, exponent):
    g, pts_all, opac = eager_rows(pts, raw, exponent)
    a = adapter_mod(pts_all, opac, g[..., 1:], with_covariances=False)
    b = pts_all.shape[0]
    flat = lambda t: None if t is None else t.reshape(b, -1, *t.shape[3:])
    return {"means": flat(a.means), "opacities": flat(a.opacities), "scales": flat(a.scales), "rotations": flat(a.rotations),
            "harmonics": flat(a.harmonics), "harmonics_band4": flat(a.harmonics_band4), "raw": a.raw}


def tail_gaussians(pts, raw, exponent, split):
    import spfsplatv2_amd as spf
    g = spf.gaussians_from_heads(pts, raw, exponent, sh_degree=SH_DEGREE, split_harmonics=split)
    return {k: getattr(g, k) for k in FIELDS + ("harmonics_band4",)}


def measure(variants, steps, sets, warmup, iters, label):
    """``steps[var](set, between=None) -> tensors``; alternates the variants on rotating input sets."""
    out, results = steptime.alternate(variants, steps, sets, warmup, iters, warm=variants[:2], held=True, ms_max=True,
                                      label=label)
    base, new, repeat = variants
    spread = steptime.spread_summary(out[base]["ms_median"], out[new]["ms_median"], out[repeat]["ms_median"])
    return {"variants": out, "baseline_spread_ms": spread["spread_ms"], "gain_ms": spread["gain_ms"],
            "speedup_over_baseline": spread["speedup"], "faster_beyond_spread": spread["faster_beyond_spread"],
            "bytes_peak_saved": out[base]["bytes_allocated_peak"] - out[new]["bytes_allocated_peak"],
            "max_rel_diff_new_vs_baseline": steptime.max_rel_diff(results[new], results[base]),
            "max_rel_diff_repeat_vs_baseline": steptime.max_rel_diff(results[repeat], results[base])}


def run_tail(name, split, warmup, iters):
    import torch

    from spfsplatv2_amd import adapter, tail
    b, v, h, w, _ = SHAPES[name]
    dev = torch.device("cuda")
    gen = torch.Generator(dev).manual_seed(0)
    rn = lambda *s: torch.randn(*s, device=dev, generator=gen)
    sets = []
    for _ in range(2):
        raw = [rn(b, C, h, w).requires_grad_(True) for _ in range(v)]
        pts = [rn(b, h, w, 3).requires_grad_(True) for _ in range(v)]
        sets.append((pts, raw))
    G = v * h * w
    ups = {"means": rn(b, G, 3), "opacities": rn(b, G), "scales": rn(b, G, 3), "rotations": rn(b, G, 4),
           "harmonics": rn(b, G, 3, 16 if split else K)}
    ad = adapter.UnifiedGaussianAdapter(adapter.GaussianAdapterCfg(0.5, 15.0, SH_DEGREE), split_harmonics=split).to(dev)

    def step(make):
        def run(s, between=None):
            pts, raw = s
            g = make(pts, raw)
            if between is not None:
                between()
            grads = torch.autograd.grad([g[k] for k in FIELDS], pts + raw, [ups[k] for k in FIELDS])
            hi = [g["harmonics_band4"]] if split else []
            return [g[k] for k in FIELDS] + hi + list(grads)
        return run
    base = step(lambda pts, raw: baseline_gaussians(ad, pts, raw, EXPONENT))
    steps = {"baseline": base, "baseline_repeat": base, "tail": step(lambda pts, raw: tail_gaussians(pts, raw, EXPONENT, split))}
    copies = dict(tail.dense_copies)
    res = measure(VARIANTS, steps, sets, warmup, iters, f"{name} {'split' if split else 'dense'}")
    res.update({"shape": name, "b": b, "v": v, "hw": [h, w], "K": K, "harmonics": "split" if split else "dense",
                "gaussians": b * G, "dense_copies": tail.dense_copies["calls"] - copies["calls"],
                "floor_bytes_per_direction": b * G * 2 * 4 * (C + 3)})           # 344 B in + 344 B out per Gaussian
    return res


def run_decoder(name, nb, warmup, iters):
    """The decoder group on ``nb`` batch items of the shape's synthetic scene."""
    import torch

    import spfsplatv2_amd as spf
    from spfsplatv2_amd import adapter, synthetic as syn, tail
    _, v, h, w, config = SHAPES[name]
    dev = torch.device("cuda")
    G = v * h * w
    mask = tail.sh_mask(SH_DEGREE).to(dev)
    sets = []
    cams = []
    for seed in (11, 12):
        bt = syn.make_batch(config, nb, 2, seed=seed).to(dev)
        assert tuple(bt.harmonics.shape) == (nb, G, 3, K), tuple(bt.harmonics.shape)
        y = (bt.scales.double() / 0.001).clamp_min(1e-12)
        raw_scales = torch.where(y > 20.0, y, torch.log(torch.expm1(y.clamp_max(20.0)))).float()
        o = bt.opacities.double().clamp(1e-4, 1 - 1e-4)
        rows = torch.cat((torch.log(o / (1 - o)).float()[..., None], raw_scales, bt.rotations,
                          (bt.harmonics / mask).reshape(nb, G, 3 * K)), dim=-1)
        raw = [rows[:, i * h * w:(i + 1) * h * w].transpose(1, 2).reshape(nb, C, h, w).contiguous().requires_grad_(True)
               for i in range(v)]
        pts = [bt.means[:, i * h * w:(i + 1) * h * w].reshape(nb, h, w, 3).contiguous().requires_grad_(True) for i in range(v)]
        sets.append((pts, raw, len(cams)))
        cams.append(bt)
    H, W = cams[0].image_shape
    wgt = torch.rand(nb, 2, 3, H, W, device=dev, generator=torch.Generator(dev).manual_seed(3))
    cfg = adapter.GaussianAdapterCfg(0.5, 15.0, SH_DEGREE)
    fused = adapter.UnifiedGaussianAdapter(cfg, fuse_into_decoder=True).to(dev)
    decs = {n: spf.get_decoder(spf.DecoderSplattingCUDACfg("splatting_cuda", [0.1, 0.2, 0.3], True, True, True)).to(dev)
            for n in ("fused", "tail")}

    def step(which):
        def run(s, between=None):
            pts, raw, ci = s
            bt = cams[ci]
            if which == "fused":
                g = baseline_gaussians(fused, pts, raw, EXPONENT)
                gs = spf.Gaussians(g["means"], None, None, None, None, g["opacities"],
                                   raw=adapter.RawGaussians(g["raw"].raw.reshape(nb, G, C - 1), g["raw"].sh_mask, g["raw"].eps))
            else:
                g = tail_gaussians(pts, raw, EXPONENT, True)
                gs = spf.Gaussians(g["means"], None, g["rotations"], g["scales"], g["harmonics"], g["opacities"],
                                   harmonics_band4=g["harmonics_band4"])
            out = decs[which](gs, bt.extrinsics, bt.intrinsics, bt.near, bt.far, bt.image_shape)
            if between is not None:
                between()
            grads = torch.autograd.grad((out.color * wgt).sum(), pts + raw)
            return [out.color] + list(grads)
        return run
    f = step("fused")
    steps = {"fused_decoder": f, "fused_decoder_repeat": f, "tail_decoder": step("tail")}
    res = measure(DEC_VARIANTS, steps, sets, warmup, iters, f"{name} decoder")
    res.update({"shape": name, "b": nb, "v": v, "hw": [h, w], "K": K, "image": [H, W], "gaussians": nb * G})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--decoder-batch", type=int, default=0, help="batch items of the decoder group (0: not run)")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "tail_time.json"))
    args = ap.parse_args()
    steptime.require_counts("tail_time", args, 10, 3)
    res = {**steptime.require_gpu("tail_time"), "exponent": EXPONENT, "results": [], "decoder": []}
    for n in SHAPES if args.shapes == "all" else args.shapes.split(","):
        for split in (True, False):
            res["results"].append(steptime.note(run_tail(n, split, args.warmup, args.iters)))
        if args.decoder_batch > 0:
            nb = min(args.decoder_batch, SHAPES[n][0])
            res["decoder"].append(steptime.note(run_decoder(n, nb, args.warmup, args.iters)))
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
