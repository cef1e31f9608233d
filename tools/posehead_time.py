"""Time the step "backbone tokens -> pose encodings / extrinsics, forward + backward": the pose heads of csrc/posehead.hip
against the same modules assembled from eager torch operations, on one GPU.

    python tools/posehead_time.py [--warmup 5] [--iters 20] [--shapes all|name,name] [--out profiles/posehead_time.json]

Variants, alternated step by step in one run on one device, all three on the SAME parameters:
  baseline         the module in eager torch: ``F.layer_norm``, ``F.silu``, ``F.gelu``, ``F.scaled_dot_product_attention``,
                   ``chunk``, ``F.softplus`` / ``clamp`` / ``cat``, ``mean`` over the tokens, and for ``predict_poses`` the
                   per-view loop with ``torch.stack`` (``process_pose`` is this package's in both: it was served before)
  product          ``spfsplatv2_amd.CameraHead`` / ``spfsplatv2_amd.predict_poses``
  baseline_repeat  `baseline` a second time in the same rotation: the spread of two runs of one variant, which a difference
                   between `baseline` and `product` has to exceed to mean anything
A step is the forward and the backward of a fixed random weighting of the outputs to the tokens and every parameter.
The GEMMs are the same library calls in both variants; what differs is everything between them.

Times: device events around each step, median over --iters after --warmup; the tokens rotate over two sets.  The camera
head's weights (865 MB) exceed the 256 MB last-level cache; the pose heads' tokens and weights do not, so the
``poses_*`` shapes are WARM timings, for every variant alike.  Per
variant also the host synchronisations of one step (torch's sync debug mode, counted as warnings), the peak of torch's
allocator during one step above what was allocated before it, and the launches are NOT counted: no kernel trace or
counter pass is taken here.  Prints one JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path
from types import SimpleNamespace

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

# name: (kind, sizes)
SHAPES = {"camera_B16_S3": ("camera", dict(B=16, S=3, N=8, dim=2048, heads=16, depth=4, iterations=4)),
          "camera_B4_S10": ("camera", dict(B=4, S=10, N=8, dim=2048, heads=16, depth=4, iterations=4)),
          "poses_v2_b16_v3_L1_C768": ("poses", dict(b=16, v=3, L=1, enc=0, dec=768, concat_enc=False, homog=False)),
          "poses_v1_b16_v2_L256_C1792": ("poses", dict(b=16, v=2, L=256, enc=1024, dec=768, concat_enc=True, homog=True))}
VARIANTS = ("baseline", "product", "baseline_repeat")


# ---- the eager modules (our own text, on the product modules' parameters) ---------------------------------------------
def eager_pose_head(head, tokens):
    import torch
    import torch.nn.functional as F
    dec = tokens[-1]
    x = torch.cat([tokens[0], dec], dim=-1) if head.concat_enc else dec
    feat = x.mean(dim=1) if x.shape[1] > 1 else x[:, 0]
    feat = F.relu(head.more_mlps[2](F.relu(head.more_mlps[0](feat))))
    t = head.fc_t(feat)
    if head.use_homogeneous:
        beta, max_inv, min_inv = head._homog
        t = t[:, :3] / (F.softplus(t[:, 3:4], beta=beta) + max_inv).clamp(max=min_inv)
    return torch.cat([head.fc_rot(feat), t], dim=-1)


def eager_predict_poses(h1, h2, feat, context_views, **kw):
    import torch

    import spfsplatv2_amd as spf
    rows = [eager_pose_head(h1, [tok[:, 0] for tok in feat])]
    rows += [eager_pose_head(h2, [tok[:, i] for tok in feat]) for i in range(1, feat[-1].shape[1])]
    return spf.process_pose(torch.stack(rows, dim=1), context_views, **kw)


def eager_camera_head(head, tokens, iterations):
    import torch
    import torch.nn.functional as F
    ln = lambda x, m: F.layer_norm(x, (x.shape[-1],), m.weight, m.bias, m.eps)
    act = {"linear": lambda y: y, "relu": F.relu, "exp": torch.exp, "inv_log": lambda y: torch.sign(y) * torch.expm1(y.abs())}
    pose_tokens = ln(tokens[:, :, 0], head.token_norm)
    B, S, C = pose_tokens.shape
    pred, outs = None, []
    for _ in range(iterations):
        p = head.empty_pose_tokens.expand(B, S, -1) if pred is None else pred.detach()
        shift, scale, gate = head.poseLN_modulation[1](F.silu(head.embed_pose(p))).chunk(3, dim=-1)
        x = gate * (F.layer_norm(pose_tokens, (C,), eps=head.adaln_norm.eps) * (1 + scale) + shift) + pose_tokens
        for blk in head.trunk:
            H = blk.attn.num_heads
            q, k, v = blk.attn.qkv(ln(x, blk.norm1)).reshape(B, S, 3, H, C // H).permute(2, 0, 3, 1, 4)
            a = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, S, C)
            x = x + blk.ls1.gamma * blk.attn.proj(a)
            x = x + blk.ls2.gamma * blk.mlp.fc2(F.gelu(blk.mlp.fc1(ln(x, blk.norm2))))
        delta = head.pose_branch.fc2(F.gelu(head.pose_branch.fc1(ln(x, head.trunk_norm))))
        pred = delta if pred is None else pred.detach() + delta
        outs.append(torch.cat([act[head.trans_act](pred[..., :3]), act[head.quat_act](pred[..., 3:7]),
                               act[head.fl_act](pred[..., 7:])], dim=-1))
    return outs


# ---- measurement -----------------------------------------------------------------------------------------------------
def measure(steps, sets, warmup, iters, label):
    out, results = steptime.alternate(VARIANTS, steps, sets, warmup, iters, warm=VARIANTS[:2], syncs=True, ms_max=True,
                                      label=label)
    for rec in out.values():
        rec["host_syncs_per_step"] = rec.pop("host_syncs")
    spread = steptime.spread_summary(*(out[v]["ms_median"] for v in ("baseline", "product", "baseline_repeat")))
    return {"variants": out, "baseline_spread_ms": spread["spread_ms"], "gain_ms": spread["gain_ms"],
            "speedup_over_baseline": spread["speedup"], "faster_beyond_spread": spread["faster_beyond_spread"],
            "slower_beyond_spread": spread["slower_beyond_spread"],
            "bytes_peak_saved": out["baseline"]["bytes_allocated_peak"] - out["product"]["bytes_allocated_peak"],
            "max_rel_diff_product_vs_baseline": steptime.max_rel_diff(results["product"], results["baseline"]),
            "max_rel_diff_repeat_vs_baseline": steptime.max_rel_diff(results["baseline_repeat"], results["baseline"])}


def _grads(outs, wrt):
    """The loss is a fixed random weighting of every output: 0.5 * sum(out^2) of a pose matrix is all but constant (its
    rotation is orthonormal), and its gradients would be rounding noise."""
    import torch
    gen = torch.Generator(outs[0].device).manual_seed(2)
    ws = [torch.randn(o.shape, device=o.device, generator=gen) for o in outs]
    g = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, ws)), wrt, allow_unused=True)
    return list(outs) + [torch.zeros_like(w) if t is None else t for t, w in zip(g, wrt)]


def run_camera(name, s, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    dev = torch.device("cuda")
    torch.manual_seed(0)
    head = spf.CameraHead(s["dim"], trunk_depth=s["depth"], num_heads=s["heads"]).to(dev)
    gen = torch.Generator(dev).manual_seed(1)
    sets = [(0.3 + 0.05 * torch.randn(s["B"], s["S"], s["N"], s["dim"], device=dev, generator=gen)).requires_grad_(True)
            for _ in range(2)]
    params = list(head.parameters())
    steps = {"product": lambda tok: _grads(head([tok], num_iterations=s["iterations"]), [tok] + params)}
    steps["baseline"] = steps["baseline_repeat"] = lambda tok: _grads(eager_camera_head(head, tok, s["iterations"]),
                                                                      [tok] + params)
    res = measure(steps, sets, warmup, iters, name)
    res.update({"shape": name, **s, "parameters": sum(p.numel() for p in params)})
    return res


def run_poses(name, s, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = SimpleNamespace(enc_embed_dim=s["enc"], dec_embed_dim=s["dec"])
    cfg = spf.PoseHeadCfg(pose_init_t=False, use_homogeneous=s["homog"], concat_enc=s["concat_enc"])
    h1, h2 = spf.PoseHead(net, cfg).to(dev), spf.PoseHead(net, cfg).to(dev)
    for h in (h1, h2):
        torch.nn.init.normal_(h.fc_rot.weight, std=0.02)          # (zero weights would hide the rotation's gradient)
    gen = torch.Generator(dev).manual_seed(1)
    widths = ([s["enc"]] if s["concat_enc"] else []) + [s["dec"]]
    sets = [[torch.randn(s["b"], s["v"], s["L"], c, device=dev, generator=gen).requires_grad_(True) for c in widths]
            for _ in range(2)]
    params = list(h1.parameters()) + list(h2.parameters())
    kw = dict(pose_make_baseline_1=True, pose_make_relative=True)
    steps = {"product": lambda feat: _grads([spf.predict_poses(h1, h2, feat, s["v"], **kw)], list(feat) + params)}
    steps["baseline"] = steps["baseline_repeat"] = lambda feat: _grads([eager_predict_poses(h1, h2, feat, s["v"], **kw)],
                                                                       list(feat) + params)
    res = measure(steps, sets, warmup, iters, name)
    res.update({"shape": name, **s})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="all")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "posehead_time.json"))
    args = ap.parse_args()
    steptime.require_counts("posehead_time", args, 10, 3)
    res = {**steptime.require_gpu("posehead_time"), "kernel_trace": "not taken", "counters": "not taken", "results": []}
    for n in SHAPES if args.shapes == "all" else args.shapes.split(","):
        kind, s = SHAPES[n]
        res["results"].append(steptime.note((run_camera if kind == "camera" else run_poses)(n, s, args.warmup, args.iters)))
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
