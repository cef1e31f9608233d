"""Time multi-view cross-attention, forward + backward, against the path a caller had before it, on one GPU.

    python tools/attention_views_time.py [--warmup 20] [--iters 100] [--shapes all|name,name] [--out profiles/attention_views_time.json]

The call is the second decoder block's of a multi-view backbone (``decoder_view_sets(v, num_target)[1]``): query views
1 .. v-1 over the other views' tokens, float32, C = 768, 12 heads, l = 258 tokens per view.  Two levels, each with its
variants alternating step by step in one run:

  module  ``views``   CrossAttention.forward_views on the tokens x [b,v,l,C]: projk / projv once per key token, the views
                      kernels, proj -- and its backward to x and to every parameter
          ``gather``  what a caller could do before: gather the other views' tokens per query view (one advanced-index
                      copy, as the backbones' generate_ctx_views; its backward is an accumulating index_put), then
                      CrossAttention.forward on [b*Vq, n*l, C] -- one call per group of query views with the same number
                      of allowed views (the masked backbone's two calls when there are targets)
          ``gather2`` the same path a second time: |gather - gather2| is the spread between two runs of one path in
                      this session, which a difference between the variants has to exceed to mean anything
  core    ``views``   rope_attention_views on the projections q [b,Vq,H,l,64], k, v [b,Vk,H,l,64]
          ``gather``  rope_attention on keys and values gathered OUTSIDE the timed region (the kernels' own cost: the
                      per-view tiling pays up to one partly empty tile per view where the gathered keys pay one in all)

Protocol of tools/attention_time.py: device events around each step, median over --iters (>= 100) after --warmup
(>= 20), inputs rotating over sets that exceed 512 MB together (cold lines), the peak of torch's allocator during one
step above what was allocated before it.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

# name: (b, v, num_target)
SHAPES = {
    "blk2_b16_v3_t1": (16, 3, 1),
    "blk2_b4_v10_t0": (4, 10, 0),          # 36 query batches of 258 -> 2322
}
C_, H, L = 768, 12, 258
ROTATE_BYTES = 512 << 20


def groups_of(allow):
    """Query views grouped by their number of allowed key views: [(query view indices, [their allowed indices])]."""
    by = {}
    for i, row in enumerate(allow.tolist()):
        idx = [s for s, on in enumerate(row) if on]
        by.setdefault(len(idx), ([], []))
        by[len(idx)][0].append(i)
        by[len(idx)][1].append(idx)
    return [by[n] for n in sorted(by)]


def positions(b, v, gen):
    import torch
    return torch.stack((torch.randint(0, 18, (b, v, L), generator=gen), torch.randint(0, 18, (b, v, L), generator=gen)), -1)


def make_set(level, b, v, vs, gen, dev):
    """One input set.  module: tokens x and positions.  core: the projections, and for the gather variant the keys,
    values and positions gathered per group (made here, outside every timed region)."""
    import torch
    qs, ks = vs.query, vs.key
    Vq, Vk = qs.stop - qs.start, ks.stop - ks.start
    pos = positions(b, v, gen).to(dev)
    s = {"pos": pos, "dout": torch.randn(b, Vq, L, C_, generator=gen).to(dev)}
    if level == "module":
        s["x"] = torch.randn(b, v, L, C_, generator=gen).to(dev)
        s["kpos_g"] = [pos[:, ks][:, torch.tensor(idx, device=dev)].reshape(b * len(qv), -1, 2).contiguous()
                       for qv, idx in groups_of(vs.allow)]
    else:
        s["q"] = torch.randn(b, Vq, L, H, 64, generator=gen).to(dev)
        s["k"] = torch.randn(b, Vk, L, H, 64, generator=gen).to(dev)
        s["v"] = torch.randn(b, Vk, L, H, 64, generator=gen).to(dev)
        s["gathered"] = []
        for qv, idx in groups_of(vs.allow):
            it = torch.tensor(idx, device=dev)
            g = len(qv)
            s["gathered"].append({
                "q": s["q"][:, torch.tensor(qv, device=dev)].reshape(b * g, L, H, 64).contiguous(),
                "k": s["k"][:, it].reshape(b * g, -1, H, 64).contiguous(),
                "v": s["v"][:, it].reshape(b * g, -1, H, 64).contiguous(),
                "qpos": pos[:, qs][:, torch.tensor(qv, device=dev)].reshape(b * g, L, 2).contiguous(),
                "kpos": pos[:, ks][:, it].reshape(b * g, -1, 2).contiguous(),
                "dout": s["dout"][:, torch.tensor(qv, device=dev)].reshape(b * g, L, C_).contiguous()})
    return s


def make_plan(vs, dev):
    """The gather path's index tensors, on the device (made once, outside every timed region)."""
    import torch
    return [(torch.tensor(qv, device=dev), torch.tensor(idx, device=dev), len(qv)) for qv, idx in groups_of(vs.allow)]


def step(level, variant, mod, vs, s, plan):
    """forward + backward; returns nothing (the gradients are formed and dropped)"""
    import torch

    import spfsplatv2_amd as spf
    qs, ks = vs.query, vs.key
    if level == "module":
        x = s["x"].detach().requires_grad_(True)
        params = list(mod.parameters())
        if variant == "views":
            out = mod.forward_views(x[:, qs], x[:, ks], s["pos"][:, qs], s["pos"][:, ks], vs.allow)
            torch.autograd.grad(out, [x] + params, s["dout"])
            return
        b = x.shape[0]
        outs, douts = [], []
        for (qi, ki, g), kpos in zip(plan, s["kpos_g"]):
            query = x[:, qs][:, qi].reshape(b * g, L, C_)
            memory = x[:, ks][:, ki].reshape(b * g, -1, C_)                     # the gather: a copy
            qpos = s["pos"][:, qs][:, qi].reshape(b * g, L, 2)
            outs.append(mod(query, memory, memory, qpos, kpos))
            douts.append(s["dout"][:, qi].reshape(b * g, L, C_))
        torch.autograd.grad(outs, [x] + params, douts)
        return
    if variant == "views":
        q, k, v = (s[n].detach().requires_grad_(True) for n in "qkv")
        out = spf.rope_attention_views(q.transpose(2, 3), k.transpose(2, 3), v.transpose(2, 3), s["pos"][:, qs],
                                       s["pos"][:, ks], allow=vs.allow)
        torch.autograd.grad(out, (q, k, v), s["dout"])
        return
    for g in s["gathered"]:
        q, k, v = (g[n].detach().requires_grad_(True) for n in "qkv")
        out = spf.rope_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), g["qpos"], g["kpos"])
        torch.autograd.grad(out, (q, k, v), g["dout"])


def run(name, level, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    b, v, nt = SHAPES[name]
    vs = spf.decoder_view_sets(v, nt)[1]
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(0)
    mod = spf.CrossAttention(C_, rope=spf.cuRoPE2D(100.0, 1.0), num_heads=H, qkv_bias=True).to(dev)
    plan = make_plan(vs, dev)
    # (one set more than the shared rule asks: the recorded input_sets of this tool count it)
    sets, nbytes = steptime.input_sets(lambda: make_set(level, b, v, vs, gen, dev), cache_bytes=ROTATE_BYTES // 2, extra=1)
    variants = ("gather", "views", "gather2")
    res = {"shape": name, "level": level, "b": b, "v": v, "num_target": nt, "Vq": v - 1, "Vk": v, "l": L, "C": C_,
           "heads": H, "dtype": "float32", "calls_of_the_gather_path": len(groups_of(vs.allow)), "input_sets": len(sets),
           "input_set_bytes": nbytes}
    steps = {var: (lambda s, var=var: step(level, var.rstrip("2"), mod, vs, s, plan)) for var in variants}
    res["variants"], _ = steptime.alternate(variants, steps, sets, warmup, iters, warm=variants[:2])
    ms = {var: res["variants"][var]["ms_median"] for var in variants}
    spread = steptime.spread_summary(ms["gather"], ms["views"], ms["gather2"])
    res.update(spread_of_the_gather_path_ms=spread["spread_ms"], gain_ms=spread["gain_ms"],
               speedup_views_over_gather=spread["speedup"], faster_by_more_than_the_spread=spread["faster_beyond_spread"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--levels", default="module,core")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "attention_views_time.json"))
    args = ap.parse_args()
    steptime.require_counts("attention_views_time", args, 100, 20)
    res = steptime.require_gpu("attention_views_time")
    names = list(SHAPES) if args.shapes == "all" else args.shapes.split(",")
    res["results"] = [steptime.note(run(n, level, args.warmup, args.iters)) for n in names for level in args.levels.split(",")]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()

