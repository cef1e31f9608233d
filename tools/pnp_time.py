"""Time ``pnp_poses`` (csrc/pnp.hip: four launches for all views of a call) on planted scenes, on one GPU.

    python tools/pnp_time.py [--warmup 5] [--iters 20] [--out profiles/pnp_time.json]

Shapes (b, v, h, w): (1, 1, 256, 256), (1, 3, 256, 256), (16, 3, 256, 256); every view is a planted scene of
tests/pnp_cases.py with 30 % gross outliers and 0.5 px noise, each with its own pose.

Times: device events around each call, median over --iters after --warmup; the inputs rotate over enough sets to exceed
twice the 256 MB last-level cache (cold buffers).  Host syncs: the synchronising calls torch reports during one call
(steptime.count_syncs).  If ``cv2`` can be imported where this runs, the reference's expression is timed
on the same inputs as well -- the copy to the host, ``cv2.solvePnPRansac`` with the reference's flags (100 iterations,
5 px, SOLVEPNP_SQPNP) per view in a Python loop, and the copy back --, wall clock; otherwise the file says that no
comparison was possible.  There is no speed gate: no baseline exists on this library to regress against.  Prints one
JSON line and writes it to --out.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import steptime  # noqa: E402

SHAPES = ((1, 1, 256, 256), (1, 3, 256, 256), (16, 3, 256, 256))
DISTINCT_VIEWS = 6                      # planted scenes are built on the host; a set cycles through this many


def make_sets(shape, dev):
    import numpy as np
    import torch

    from tests import pnp_cases as Cs
    b, v, h, w = shape
    views = [Cs.planted_view(h, w, seed=500 + i, outliers=0.3, noise=0.5) for i in range(min(DISTINCT_VIEWS, b * v))]
    pick = [views[i % len(views)] for i in range(b * v)]
    one = {k: torch.from_numpy(np.stack([x[k] for x in pick])).reshape(b, v, *pick[0][k].shape).to(dev)
           for k in ("pts", "opacity", "K")}
    planted = torch.from_numpy(np.stack([x["pose"] for x in pick])).reshape(b, v, 4, 4)
    sets, set_bytes = steptime.input_sets(lambda: {k: t.clone() for k, t in one.items()})
    return sets, set_bytes, planted


def reference_cv2(cv2, s, h, w):
    """The reference's get_pnp_pose_batch, as misc/cam_utils.py words it (host numpy + OpenCV), on device inputs."""
    import numpy as np
    import torch
    b, v = s["pts"].shape[:2]
    out = torch.zeros(b, v, 4, 4)
    pixels = np.mgrid[:w, :h].T.astype(np.float32)
    for i in range(b):
        for j in range(v):
            pts = s["pts"][i, j].cpu().numpy()
            mask = s["opacity"][i, j].cpu().numpy() > 0.3
            K = s["K"][i, j].cpu().numpy().copy()
            K[0] *= w
            K[1] *= h
            ok, R, T, _ = cv2.solvePnPRansac(pts[mask], pixels[mask], K, None, iterationsCount=100, reprojectionError=5,
                                             flags=cv2.SOLVEPNP_SQPNP)
            pose = np.eye(4, dtype=np.float32)
            if ok:
                pose[:3, :3], pose[:3, 3] = cv2.Rodrigues(R)[0], T[:, 0]
                pose = np.linalg.inv(pose)
            out[i, j] = torch.from_numpy(pose)
    return out.to(s["pts"].device)


def run(shape, warmup, iters, cv2):
    import torch

    import spfsplatv2_amd as spf
    dev = torch.device("cuda")
    b, v, h, w = shape
    sets, set_bytes, planted = make_sets(shape, dev)
    call = lambda s: spf.pnp_poses(s["pts"], s["opacity"], s["K"], h, w)       # noqa: E731
    ms = steptime.median_ms(call, warmup, iters, sets=sets, ms_max=True)
    syncs, res = steptime.syncs_and_result(lambda: call(sets[0]))          # (every set is a copy of the first)
    poses = res.poses.cpu().double()
    out = {"shape": list(shape), "input_sets": len(sets), "input_set_bytes": set_bytes,
           "workspace_bytes": int(spf._lib.load().spf_pnp_workspace_bytes(b * v, h, w, 128)),
           **ms, "iters": iters, "warmup": warmup, "host_syncs": syncs,
           "views_succeeded": int(res.success.sum()), "views": b * v,
           "inliers_min_max": [int(res.inliers.min()), int(res.inliers.max())], "candidates": h * w,
           "max_abs_pose_diff_from_planted": float((poses - planted).abs().max())}
    if cv2 is not None:
        wall = []
        for i in range(max(3, iters // 4)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = reference_cv2(cv2, sets[i % len(sets)], h, w)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
        out["cv2_ms_median"] = statistics.median(wall)
        out["cv2_max_abs_pose_diff_from_planted"] = float((ref.cpu().double() - planted).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pnp_time.json"))
    args = ap.parse_args()
    steptime.require_counts("pnp_time", args, 10, 3)
    res = steptime.require_gpu("pnp_time")
    try:
        import cv2
    except ImportError:
        cv2 = None
    res.update(comparison="cv2.solvePnPRansac timed on the same inputs" if cv2 is not None else
               "none: cv2 cannot be imported here, so the reference's expression was not timed",
               kernel_trace="none taken: the times are whole calls between device events")
    res["results"] = [steptime.note(run(shape, args.warmup, args.iters, cv2)) for shape in SHAPES]
    steptime.emit(res, args.out)


if __name__ == "__main__":
    main()
