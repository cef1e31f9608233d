"""The multi-rank PRODUCT path, executed: two processes (one per rank, `gloo`, both on cuda:0 -- the GPU box has one
device) run decoder forward + fused MSE + backward through the HIP library on their shard.

* scene-first sharding (shard.scene_shard; the reference's one-process-per-GPU DDP, src/main.py:141-145, over the
  flat (b v) list of decoder_splatting_cuda.py:53-64): the gathered images equal the single-process batch bit for
  bit and every per-Gaussian gradient matches -- no data-path collective was needed;
* one scene's views split across ranks (BASELINE config 5): after `allreduce_gaussian_grads` every rank holds the
  single-process gradient (1e-5);
* `python bench.py --gpus 2` with no launcher starts two ranks itself and reports `n_gpus: 2`.
"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GNAMES = ("means", "scales", "rotations", "opacities", "harmonics")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _step(spf, b, scenes, views, weight, dev, bucketed=False):
    """decoder forward + LossMse + backward for the given scenes / views of batch b; everything through the product.
    `bucketed`: the backward writes the Gaussian gradients into a shard.GradBucket (returned as the sixth item)."""
    sel = lambda t: t[scenes].to(dev)
    selv = lambda t: t[scenes][:, views].to(dev)
    leaves = {n: sel(getattr(b, n)).clone().requires_grad_(True) for n in GNAMES}
    ext = selv(b.extrinsics).clone().requires_grad_(True)
    color, depth, alpha = spf.render_views(ext, selv(b.intrinsics), selv(b.near), selv(b.far), b.image_shape,
                                           torch.tensor([0.1, 0.2, 0.3], device=dev), leaves["means"],
                                           leaves["harmonics"], leaves["opacities"], leaves["rotations"],
                                           leaves["scales"], scale_invariant=True, enable_cov_grad=True,
                                           enable_sh_grad=True)
    loss = spf.mse_loss(color, selv(b.target), weight)
    if bucketed:
        from spfsplatv2_amd import shard
        bucket = shard.GradBucket(*(leaves[n] for n in GNAMES))
        with bucket:
            loss.backward()
        return color.detach(), depth.detach(), float(loss), {n: leaves[n].grad for n in GNAMES}, ext.grad, bucket
    loss.backward()
    return color.detach(), depth.detach(), float(loss), {n: leaves[n].grad for n in GNAMES}, ext.grad


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist

    import spfsplatv2_amd as spf
    from spfsplatv2_amd import shard, synthetic as syn
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        dev = torch.device("cuda", 0)
        S, V = 5, 4
        b = syn.make_batch("TEST", S, V, seed=77, s_mult=6.0, G=1800, K=4, image_hw=(64, 80))
        everything = list(range(S)), list(range(V))
        # ---- 1) scene-first sharding, no collective on the data path ----
        mine = shard.scene_shard(S, rank, world)
        color, depth, loss, grads, gext = _step(spf, b, mine, everything[1], len(mine) / S, dev)
        full_c = shard.gather_rendered(color.cpu(), S)
        full_d = shard.gather_rendered(depth.cpu(), S)
        full_g = {n: shard.gather_rendered(grads[n].cpu(), S) for n in GNAMES}
        full_e = shard.gather_rendered(gext.cpu(), S)
        losses = [None] * world
        dist.all_gather_object(losses, loss)
        if rank == 0:
            c1, d1, l1, g1, e1 = _step(spf, b, *everything, 1.0, dev)
            ok = torch.equal(full_c, c1.cpu()) and torch.equal(full_d, d1.cpu())
            worst = max(float((full_g[n] - g1[n].cpu()).abs().max() / g1[n].abs().max()) for n in GNAMES)
            worst = max(worst, float((full_e - e1.cpu()).abs().max() / e1.abs().max()))
            q.put(("scene_shard", ok, worst, abs(sum(losses) - l1) / l1))
        # ---- 2) one scene's views split across ranks + the gradient all-reduce ----
        scenes = [0, 1]
        myv = shard.view_shard(V, rank, world)
        _, _, _, g2, _ = _step(spf, b, scenes, myv, len(myv) / V, dev)
        shard.allreduce_gaussian_grads([g2[n] for n in GNAMES])
        _, _, _, gref, _ = _step(spf, b, scenes, everything[1], 1.0, dev)
        worst = max(float((g2[n] - gref[n]).abs().max() / gref[n].abs().max()) for n in GNAMES)
        q.put(("allreduce", rank, worst))
        # ---- 3) the same exchange through a GradBucket: written in place by the backward kernels, ONE collective ----
        _, _, _, g3, _, bucket = _step(spf, b, scenes, myv, len(myv) / V, dev, bucketed=True)
        lo, hi = bucket.flat.data_ptr(), bucket.flat.data_ptr() + 4 * bucket.flat.numel()
        aliased = all(lo <= g3[n].data_ptr() < hi for n in GNAMES)
        work = bucket.all_reduce(async_op=True)
        if work is not None:
            work.wait()
        torch.cuda.synchronize()
        # (two runs of the same step: bit-equal where no dense tile's LDS float atomics are involved, 1e-6 of scale here)
        same = all(float((g3[n] - g2[n]).abs().max() / g2[n].abs().max()) < 1e-6 for n in GNAMES)
        q.put(("bucket", rank, aliased, same))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_world2_product_path_scene_shard_and_allreduce(hip_lib):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
        assert p.exitcode == 0, p.exitcode
    got = [q.get(timeout=10) for _ in range(5)]
    sc = [g for g in got if g[0] == "scene_shard"][0]
    assert sc[1], "scene-sharded images differ from the single-process batch"
    assert sc[2] < 1e-5 and sc[3] < 1e-6, sc          # gradients (dense tiles use LDS float atomics), summed loss
    ar = sorted(g for g in got if g[0] == "allreduce")
    assert [g[1] for g in ar] == [0, 1] and all(g[2] < 1e-5 for g in ar), ar
    # GradBucket: the leaves' gradients live INSIDE the flat buffer (no cat, no copy back) and its one all-reduce gives
    # what the list form gave
    bk = sorted(g for g in got if g[0] == "bucket")
    assert [g[1:] for g in bk] == [(0, True, True), (1, True, True)], bk


def test_bench_gpus2_starts_two_ranks_itself(hip_lib):
    """`python bench.py --gpus 2` with WORLD_SIZE unset (it silently ran one rank)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--gpus", "2", "--one-device", "--backend",
                        "gloo", "--steps", "3", "--warmup", "1", "--min-trials", "3", "--min-seconds", "0", "--scenes", "2",
                        "--views", "2", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, env=env,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["renders_per_step"] == 8
    assert out["timing"]["trials"] == 3 and len(out["trials_ms"]) == 3
    # and the view-split + all-reduce variant (BASELINE config 5's exchange step)
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--gpus", "2", "--one-device", "--backend",
                        "gloo", "--steps", "2", "--warmup", "1", "--min-trials", "2", "--min-seconds", "0", "--scenes", "1",
                        "--views", "2", "--no-cpu-baseline", "--allreduce"], capture_output=True, text=True,
                       timeout=900, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 2 and "all-reduce" in out["config"]["sharding"]


def test_bench_streams2_micro_batches(hip_lib):
    """`bench.py --streams 2`: two micro-batches, two HIP graphs, two streams -- same renders per step, one JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--streams", "2", "--steps", "3", "--warmup", "2",
                        "--min-trials", "3", "--min-seconds", "0", "--scenes", "2", "--views", "2", "--no-cpu-baseline"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["n_gpus"] == 1 and out["config"]["renders_per_step"] == 4 and "2 micro-batches" in out["config"]["launch"]
    assert out["value"] > 0 and out["roofline"]["frac"] > 0


def test_rccl_preflight_world_of_one(hip_lib):
    """The first 8-GPU run must not be the first time RCCL executes: under the driver's own launcher form
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 ...`, /root/reference/src/main.py:141-145 is what it
    stands in for) bench.py initialises the `nccl` (= RCCL) process group with `device_id`, synchronises its ranks with
    RCCL barriers, and -- with --allreduce -- sums the Gaussian gradients through the flat bucket ON THE DEVICE (no host
    staging); the line it prints is a normal single-GPU line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
            "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "bench.py"), "--full", "--gpus", "1", "--steps", "3",
            "--warmup", "1", "--min-trials", "2", "--min-seconds", "0", "--scenes", "2", "--views", "2",
            "--no-cpu-baseline"]
    for extra in ([], ["--allreduce"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=900, env=env, cwd=str(ROOT))
        assert r.returncode == 0, r.stderr[-3000:]
        out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
        assert out["n_gpus"] == 1 and out["value"] > 0 and out["config"]["process_group"] == "nccl"
        if extra:
            assert "all-reduce" in out["config"]["sharding"]


def _nccl_worker(port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import torch.distributed as dist
    from spfsplatv2_amd import shard
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        gen = torch.Generator().manual_seed(3)
        grads = [torch.randn(4, 1000, 3, generator=gen).cuda(), None, torch.randn(4, 1000, generator=gen).cuda(),
                 torch.randn(4, 1000, 3, 4, generator=gen).cuda()]
        want = [None if g is None else g.clone() for g in grads]
        shard.allreduce_gaussian_grads(grads, skip_single=False)        # device bucket through RCCL, world of one
        torch.cuda.synchronize()
        q.put(all(w is None or torch.equal(g, w) for g, w in zip(grads, want)))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_allreduce_bucket_on_device_through_rccl(hip_lib):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_nccl_worker, args=(_free_port(), q))
    p.start()
    p.join(300)
    assert p.exitcode == 0, p.exitcode
    assert q.get(timeout=10) is True
