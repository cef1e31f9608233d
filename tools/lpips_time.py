"""Time LPIPS on one GPU: the HIP kernels against the restatement in eager float32 torch ops.

    python tools/lpips_time.py [--workloads train,train_10view,test_step] [--warmup 20] [--iters 100] [--out FILE]
    python tools/lpips_time.py --variants product --workloads train --iters 20 --no-layers   (the run for rocprofv3)

Workloads (256 x 256 images in [0, 1], seeded weights of tests/lpips_oracle.py, median of --iters after --warmup, device
events):
  train         RE10K: batch 16, one target view: 16 rendered + 16 ground-truth images, gradient to the rendered ones,
                forward + backward through LossLpips
  train_10view  re10k_10view: batch 3, one target view: 3 + 3 images, forward + backward
  test_step     3 + 3 images, forward only (compute_lpips)
Variants, on the same device in the same run:
  product  spfsplatv2_amd.LossLpips / compute_lpips
  eager    tests/lpips_oracle.py in float32 on the device (F.conv2d, F.max_pool2d, autograd): what the reference's
           package runs
Per convolution layer (the `train` batch of 32 images, forward): the kernel's time and its TFLOP/s against the float32
matrix peak.  Prints one JSON line (and writes it to --out).
"""
from __future__ import annotations

import argparse
import ctypes as C
import importlib
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

WORKLOADS = {"train": (16, True), "train_10view": (3, True), "test_step": (3, False)}      # pairs, backward
SIDE = 256
F32_MATRIX_PEAK = 157.3e12      # FLOP/s, MI355X


def run(workload, variants, warmup, iters, sd, W):
    import torch

    import spfsplatv2_amd as spf
    from tests import lpips_oracle as lo
    n, backward = WORKLOADS[workload]
    pred, target = (t.cuda() for t in lo.image_pair(0, (n, 3, SIDE, SIDE)))
    x = pred.clone().requires_grad_(True)
    loss = spf.LossLpips(spf.LossLpipsCfgWrapper(spf.LossLpipsCfg(0.05, 0)), weights=W)
    dsd = {k: v.cuda() for k, v in sd.items()}

    def product():
        if backward:
            x.grad = None
            loss(x[None], target[None], None, 0).backward()
        else:
            spf.compute_lpips(target, pred, weights=W)

    def eager():
        if backward:
            x.grad = None
            (0.05 * lo.lpips(x, target, dsd, True, torch.float32).mean()).backward()
        else:
            with torch.no_grad():
                lo.lpips(target, pred, dsd, True, torch.float32)[:, 0, 0, 0]

    fns = {"product": product, "eager": eager}
    out = {"workload": workload, "pairs": n, "backward": backward, "variants": {}}
    for var in variants:
        out["variants"][var] = steptime.median_ms(fns[var], warmup, iters)
    v = out["variants"]
    if "eager" in v and "product" in v:
        out["eager_over_product"] = v["eager"]["ms_median"] / v["product"]["ms_median"]
    return out


def layers(n_img, warmup, iters, W):
    """Every MFMA convolution layer forward on n_img images of its RE10K size, straight through the C entry point on
    channels-last tensors (no layout copies inside the timed region)."""
    import torch

    from spfsplatv2_amd import _lib
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    lib = _lib.load()
    dw = W.on("cuda")
    res = []
    for l in range(1, 13):
        side = SIDE >> lp.CONV_LEVEL[l]
        ci, co = lp.CONV_CIN[l], lp.CONV_COUT[l]
        xin = torch.relu(torch.randn(n_img, side, side, ci, device="cuda"))
        out = torch.empty(n_img, side, side, co, device="cuda")
        wp, bias = dw["wfwd"][lp.PACK_OFFSET[l]:], dw["bias"][sum(lp.CONV_COUT[:l]):]
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            _lib.check(lib.spf_lpips_conv3x3(C.c_void_p(xin.data_ptr()), None, C.c_void_p(wp.data_ptr()),
                                             C.c_void_p(bias.data_ptr()), C.c_void_p(out.data_ptr()), n_img, side, side,
                                             ci, co, 1, stream), "spf_lpips_conv3x3")
        t = steptime.median_ms(call, warmup, iters)
        flop = 2.0 * n_img * side * side * 9 * ci * co
        tf = flop / (t["ms_median"] * 1e-3) / 1e12
        res.append({"layer": l + 1, "side": side, "cin": ci, "cout": co, "images": n_img, "ms_median": t["ms_median"],
                    "tflops": tf, "share_of_f32_matrix_peak": tf * 1e12 / F32_MATRIX_PEAK})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="train,train_10view,test_step")
    ap.add_argument("--variants", default="product,eager")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    steptime.require_counts("lpips_time", args, 2, 0)
    res = {**steptime.require_gpu("lpips_time"), "warmup": args.warmup, "iters": args.iters}
    from tests import lpips_oracle as lo
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    sd = lo.make_weights(1)
    W = lp.LpipsWeights.from_state_dict(sd)
    res["results"] = [run(w, args.variants.split(","), args.warmup, args.iters, sd, W) for w in args.workloads.split(",") if w]
    if not args.no_layers:
        res["conv_layers_forward"] = layers(32, args.warmup, args.iters, W)
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
