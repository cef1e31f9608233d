"""Time SSIM on one GPU: the HIP kernels against the reference's eager expression.

    python tools/ssim_time.py [--shapes headline,re10k_10view,test_step] [--warmup 20] [--iters 100] [--out FILE]
    python tools/ssim_time.py --variants product --shapes headline --iters 20     (the run to put under rocprofv3)
    python tools/ssim_time.py --stats KERNEL_STATS_CSV --shapes headline          (bytes over kernel time, no GPU needed)

Per shape [N,3,256,256] (smooth inputs, tests/ssim_oracle.py), median of --iters after --warmup, device events:
  eager    the reference's expression (tests/ssim_oracle.py in float32 on the device: ten grouped convolutions and ~twenty
           elementwise kernels forward, autograd backward) -- the baseline: there is no earlier implementation
  product  spfsplatv2_amd.ssim / compute_ssim
each for the forward alone (no grad), forward + backward (both inputs requiring grad, scalar loss), and compute_ssim.
  host     compute_ssim by the reference's route restated: per image a device -> host copy and scipy's filter; once, for
           the record; left out when scipy is missing.
Prints one JSON line (and writes it to --out).

--stats reads a `rocprofv3 --kernel-trace --stats` kernel_stats.csv of a product run of ONE shape and sets the kernels'
mean times against the byte model: the forward reads X and Y (8 B per element), the backward reads them and writes two
gradients (16 B per element).
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

SHAPES = {"headline": (32, 3, 256, 256), "re10k_10view": (30, 3, 256, 256), "test_step": (3, 3, 256, 256)}
HBM_PEAK = 8.0e12          # B/s, MI355X


def run(shape, variants, warmup, iters):
    import torch

    import spfsplatv2_amd as spf
    from tests import ssim_oracle as so
    X, Y = (t.cuda() for t in so.smooth(0, SHAPES[shape]))
    x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)

    def eager(a, b):
        return so.ssim_oracle(a, b, data_range=1.0, dtype=torch.float32)

    def product(a, b):
        return spf.ssim(a, b, data_range=1.0)[0]

    def fwd(f):
        with torch.no_grad():
            return f(X, Y)

    def fwd_bwd(f):
        x.grad = y.grad = None
        f(x, y).backward()

    fns = {"eager": (eager, lambda: so.compute_ssim_oracle(X, Y, dtype=torch.float32)),
           "product": (product, lambda: spf.compute_ssim(X, Y))}
    out = {"shape": shape, "nchw": list(SHAPES[shape]), "variants": {}}
    for var in variants:
        f, metric = fns[var]
        out["variants"][var] = {"forward": steptime.median_ms(lambda: fwd(f), warmup, iters),
                                "forward_backward": steptime.median_ms(lambda: fwd_bwd(f), warmup, iters),
                                "compute_ssim": steptime.median_ms(lambda: fwd(lambda a, b: metric()), warmup, iters)}
    v = out["variants"]
    if "eager" in v and "product" in v:
        out["speedup"] = {k: v["eager"][k]["ms_median"] / v["product"][k]["ms_median"] for k in v["eager"]}
    try:
        import scipy  # noqa: F401
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = so.skimage_ssim(X.cpu(), Y.cpu())
        out["host_route_compute_ssim_ms"] = (time.perf_counter() - t0) * 1e3
        out["host_route_max_diff"] = float((spf.compute_ssim(X, Y).double().cpu() - host).abs().max())
    except ImportError:
        out["host_route_compute_ssim_ms"] = None          # no scipy on this machine
    return out


def kernel_stats(path, shape):
    n, c, h, w = SHAPES[shape]
    elems = n * c * h * w
    need = {"spf_ssim_fwd_kernel": 8 * elems, "spf_ssim_bwd_kernel": 16 * elems}
    return {"shape": shape, "elements": elems,
            "kernels": steptime.kernel_stats(path, ("spf_ssim", "spf_psnr"), need, {"share_of_peak": HBM_PEAK}, width=100)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,re10k_10view,test_step")
    ap.add_argument("--variants", default="eager,product")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--out", default=None)
    ap.add_argument("--stats", default=None, help="rocprofv3 kernel_stats.csv to turn into bytes over time")
    args = ap.parse_args()
    shapes = [s for s in args.shapes.split(",") if s]
    if args.stats:
        assert len(shapes) == 1, "--stats reads the profile of one shape"
        steptime.emit(kernel_stats(args.stats, shapes[0]), None)
        return
    steptime.require_counts("ssim_time", args, 2, 0)
    res = {**steptime.require_gpu("ssim_time"), "warmup": args.warmup, "iters": args.iters}
    res["results"] = [run(s, args.variants.split(","), args.warmup, args.iters) for s in shapes]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
