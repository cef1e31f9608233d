"""The tile lists the rasterizer builds, audited as integers (tests/tile_state.py): every forward call below is followed
by a device-to-host copy of its state and an exact check of the tile counts, the lists (element for element against
np.sort of the keys), the scan, the pair numbering and, where the library keeps one, the launch order -- no tolerance,
no mask.

* the boundary scene: list lengths on both sides of every border between two sort kernels (and the chunk borders of the
  chunked sort), five key patterns, two id layouts -- through every sort kernel, exact and planned, packed lists and
  direct bins;
* random scenes (multi-tile rects): every binning and scan path, both host bindings, the covariance entry, the decoder's
  camera path; their rects are also held against the float64 oracle's.
`SPF_TILE_STATE_REPORT=<file>` appends one JSON line per case: the plan's kernels, the list lengths audited, wall time."""
import functools
import json
import os
import time

import numpy as np
import pytest
import torch

from tests import tile_state as ts
from tests.conftest import ROOT
from tests.test_tile_state import DIRECT_BIN_CAPS, check_sort_plan_coverage, random_scene

pytestmark = pytest.mark.gpu

STATE_ENV = ts.SORT_ENV + ("SPF_DIRECT_BINS", "SPF_TILE_ORDER", "SPF_BIN_VIEWS", "SPF_MAX_LDS_TILES", "SPF_CHUNKS",
                           "SPF_XCD_DEAL")


def _report(case, **rep):
    print(json.dumps({"case": case, **rep}))
    out = os.environ.get("SPF_TILE_STATE_REPORT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": case, **rep}) + "\n")


def _set_env(monkeypatch, env, binding=False):
    """The switches of this case and no others; `binding`: the compiled host binding instead of the ctypes path."""
    from spfsplatv2_amd import _lib
    for name in STATE_ENV:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(_lib, "_fast", False)                    # (decided again at the next call)
    if binding:
        monkeypatch.delenv("SPF_NO_FAST", raising=False)
    else:
        monkeypatch.setenv("SPF_NO_FAST", "1")


def _names():
    ids = ts.sort_ids((ROOT / "include" / "spfsplat_hip.h").read_text())
    return {v: k for k, v in ids.items() if k != "MAX_LAUNCHES"}


def _forward(inp, H, W, max_pairs, sh_degree=0, cov3D=None, camera=None, view64=None):
    """One forward call one level below autograd -> (host copies of the eight state tensors, bin_cap, capacity, record)."""
    from spfsplatv2_amd import rasterizer as rz
    rec = rz.CallRecord()
    _, state, (_, bin_cap, capacity) = rz._forward_impl(
        inp["means"], inp.get("scales"), inp.get("rotations"), inp["opacities"], inp.get("shs"), inp.get("colors"),
        inp["viewmatrix"], inp["projmatrix"], inp["tanfov"], inp["bg"], inp.get("view_scale"), H, W, sh_degree, 1.0,
        max_pairs, record=rec, cov3D=cov3D, camera=camera, view64=view64)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in state), int(bin_cap), int(capacity), rec


def _views():
    from spfsplatv2_amd import rasterizer as rz
    return rz._state_views


def _to(inp, dev="cuda"):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}


# ---- the boundary scene ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _boundary(cap, interleaved, hw=None, lengths=None):
    """(scene, expected counts, expected lists) -- shared between the cases, never changed.  The key patterns rotate with
    the id layout, so the two layouts of a cap put different patterns on each length."""
    scene = ts.boundary_scene(cap, interleaved, hw=hw, rotate=3 if interleaved else 0, seed=cap, lengths=lengths)
    count, keys = ts.boundary_expected(scene)
    return scene, count, keys


def _check_boundary(scene, want_count, want_keys, state, bin_cap, capacity, shards=1):
    S, V, G, H, W = 1, 1, scene["G"], scene["H"], scene["W"]
    out = ts.audit(state, S, V, G, H, W, bin_cap, capacity, _views(), shards=shards)
    assert out == [], out
    count, keys = ts.device_lists(state, _views(), S, V, G, H, W, bin_cap)
    assert np.array_equal(count, want_count), (count.tolist(), want_count.tolist())   # the intended lengths, exactly
    assert np.array_equal(keys, want_keys)
    assert 3 <= int(state[1].min()) and int(state[1].max()) <= 7              # (every Gaussian visible, inside its tile)


@pytest.mark.parametrize("case", ts.sort_cases(), ids=ts.case_id)
def test_sort_classes_on_the_boundary_scene(hip_lib, monkeypatch, case):
    """Exact mode and the planned classic chain on the lengths b - 1, b, b + 1 of every sort-class border up to `cap`
    (the top case: two, three and four chunks of the chunked sort, the last holding one entry)."""
    from spfsplatv2_amd import rasterizer as rz
    cap, env, interleaved = case
    _set_env(monkeypatch, env)
    scene, want_count, want_keys = _boundary(cap, interleaved)
    T, names, L = len(scene["lengths"]), _names(), ts.boundary_lengths(cap)
    inp = _to(scene)
    t0 = time.perf_counter()
    state, bin_cap, capacity, rec = _forward(inp, scene["H"], scene["W"], None)
    assert bin_cap == 0 and rec["num_pairs"] == scene["G"] == capacity and rec["max_tile_list"] == max(L)
    _check_boundary(scene, want_count, want_keys, state, 0, capacity)
    exact_plan = ts.sort_plan(hip_lib, rec["max_tile_list"], T)
    # the same scene from a plan, packed lists
    monkeypatch.setenv("SPF_DIRECT_BINS", "0")
    budget = rz.plan_pair_budget(rec, check="deferred")
    assert (budget.max_tile_list >= max(L)) if max(L) * 1.25 < 16384 else (budget.max_tile_list == 0)   # (0: every class)
    assert budget.capacity > scene["G"]
    state, bin_cap, capacity, rec2 = _forward(inp, scene["H"], scene["W"], budget)
    assert bin_cap == 0 and capacity == budget.capacity and rz.plan_flags(rec2) == 0
    _check_boundary(scene, want_count, want_keys, state, 0, capacity)
    planned_plan = ts.sort_plan(hip_lib, budget.max_tile_list, T)
    used = ts.kernels_sorting(exact_plan, L) | ts.kernels_sorting(planned_plan, L)
    _report(ts.case_id(case), exact=[(names[k], lo, hi) for k, lo, hi in exact_plan],
            planned=[(names[k], lo, hi) for k, lo, hi in planned_plan], kernels_with_lists=sorted(names[k] for k in used),
            lengths=L, gaussians=scene["G"], seconds=round(time.perf_counter() - t0, 3))


def test_sort_cases_cover_every_sort_kernel(hip_lib, monkeypatch):
    """The parametrisation above puts at least one list into every sort kernel's class (ORDER_ONLY: see below)."""
    check_sort_plan_coverage(hip_lib, monkeypatch)


@pytest.mark.parametrize("interleaved", [False, True], ids=["contiguous", "interleaved"])
@pytest.mark.parametrize("cap", DIRECT_BIN_CAPS)
def test_direct_bins_on_the_boundary_scene(hip_lib, monkeypatch, cap, interleaved):
    """The same scenes through a plan with direct bins, for every cap whose plan runs with them (up to 8,192:
    tests/test_tile_state.py::test_direct_bins_take_the_caps_up_to_8192)."""
    from spfsplatv2_amd import rasterizer as rz
    _set_env(monkeypatch, {})
    scene, want_count, want_keys = _boundary(cap, interleaved)
    T, L = len(scene["lengths"]), ts.boundary_lengths(cap)
    budget = rz.plan_pair_budget(dict(num_pairs=scene["G"], max_tile_list=max(L)), check="deferred")
    want_bin = rz._direct_bin_cap(budget, T, T)
    assert want_bin == budget.max_tile_list >= max(L) and want_bin in (1024, 2048, 4096, 8192, 16384)
    t0 = time.perf_counter()
    state, bin_cap, capacity, rec = _forward(_to(scene), scene["H"], scene["W"], budget)
    shards = hip_lib.spf_raster_pair_shards(1, scene["G"])
    assert rec["plan"] == (want_bin, capacity, shards) and bin_cap == want_bin and rz.plan_flags(rec) == 0
    _check_boundary(scene, want_count, want_keys, state, bin_cap, capacity, shards)
    names = _names()
    _report(f"direct-cap{cap}-{'interleaved' if interleaved else 'contiguous'}", bin_cap=bin_cap, shards=shards,
            planned=[(names[k], lo, hi) for k, lo, hi in ts.sort_plan(hip_lib, bin_cap, T)], lengths=L,
            seconds=round(time.perf_counter() - t0, 3))


def test_direct_bins_with_a_sharded_pair_numbering(hip_lib, monkeypatch):
    """From 512 blocks of 256 Gaussians on the projection kernel numbers its pairs from eight cursors: 132,390 Gaussians
    (the lengths of the 4,096 case and eighteen lists of 6,000) -- every record range inside the share of its block's
    shard, every cursor the pairs of its blocks."""
    from spfsplatv2_amd import rasterizer as rz
    _set_env(monkeypatch, {})
    scene, want_count, want_keys = _boundary(4096, True, None, tuple(ts.boundary_lengths(4096) + [6000] * 18))
    assert hip_lib.spf_raster_pair_shards(1, scene["G"]) == 8
    budget = rz.plan_pair_budget(dict(num_pairs=scene["G"], max_tile_list=6000), check="deferred")
    t0 = time.perf_counter()
    state, bin_cap, capacity, rec = _forward(_to(scene), scene["H"], scene["W"], budget)
    assert rec["plan"] == (8192, capacity, 8) and bin_cap == 8192 and rz.plan_flags(rec) == 0
    assert capacity == budget.capacity + budget.capacity // 4
    _check_boundary(scene, want_count, want_keys, state, bin_cap, capacity, shards=8)
    _report("direct-sharded", bin_cap=bin_cap, shards=8, gaussians=scene["G"],
            lengths=sorted(set(scene["lengths"].tolist())), seconds=round(time.perf_counter() - t0, 3))


@pytest.mark.parametrize("variant", ["boundary_lengths", "lists_of_one"])
def test_direct_bins_launch_order_on_2048_tiles(hip_lib, monkeypatch, variant):
    """1024 x 512 px = 2,048 tiles: the library keeps the composite kernels' launch order over tile_start | tile_fill -- a
    permutation of the tiles, each with min(count, bin) -- written by the first sort kernel, or, when no list has more
    than one entry (a bin of one), by the ORDER_ONLY launch."""
    from spfsplatv2_amd import rasterizer as rz
    _set_env(monkeypatch, {})
    names = _names()
    if variant == "boundary_lengths":
        scene, want_count, want_keys = _boundary(1024, True, (1024, 512))
        budget = rz.plan_pair_budget(dict(num_pairs=scene["G"], max_tile_list=1025), check="deferred")
    else:
        scene, want_count, want_keys = _boundary(0, False, (1024, 512), (1, 0, 1, 1))
        budget = rz.PairBudget(scene["G"] + 1024, 1, "deferred")
    T = len(scene["lengths"])
    assert T == 2048 and ts.order_expected(T, budget.max_tile_list)
    plan = ts.sort_plan(hip_lib, budget.max_tile_list, T, with_order=True)
    assert (names[plan[0][0]] == "ORDER_ONLY" and len(plan) == 1) == (variant == "lists_of_one")
    t0 = time.perf_counter()
    state, bin_cap, capacity, rec = _forward(_to(scene), scene["H"], scene["W"], budget)
    assert bin_cap == budget.max_tile_list == rec["plan"][0] and rz.plan_flags(rec) == 0
    _check_boundary(scene, want_count, want_keys, state, bin_cap, capacity)       # (audits the launch order, too)
    # the order the library wrote is more than a permutation: the last window of every XCD's range is longest first
    order = state[3].numpy().view(np.uint32)[2 * T:4 * T].reshape(T, 2).astype(np.int64)
    for x in range(8):
        tail = order[(x + 1) * (T // 8) - 256:(x + 1) * (T // 8), 1]
        cls = 63 - np.minimum(63, tail * 64 // (bin_cap + 1))
        assert bool((np.diff(cls) >= 0).all()), (x, tail.tolist())
    # SPF_TILE_ORDER=0: no launch order, the same lists
    monkeypatch.setenv("SPF_TILE_ORDER", "0")
    state0, _, _, rec0 = _forward(_to(scene), scene["H"], scene["W"], budget)
    assert rz.plan_flags(rec0) == 0
    out = ts.audit(state0, 1, 1, scene["G"], scene["H"], scene["W"], bin_cap, capacity, _views(), launch_order=False)
    assert out == [], out
    assert np.array_equal(ts.device_lists(state0, _views(), 1, 1, scene["G"], scene["H"], scene["W"], bin_cap)[1], want_keys)
    _report(f"launch-order-{variant}", bin_cap=bin_cap, planned=[(names[k], lo, hi) for k, lo, hi in plan],
            lengths=sorted(set(scene["lengths"].tolist())), seconds=round(time.perf_counter() - t0, 3))


@pytest.mark.parametrize("mode", ["exact", "direct_bins"])
def test_sorted_state_does_not_depend_on_the_binning_order(hip_lib, monkeypatch, mode):
    """Atomics fill the bins in another order on every run; the sorted lists are the same bits: the top boundary case
    (packed lists, the chunked sort included) and the largest direct-bins case, each run twice."""
    from spfsplatv2_amd import rasterizer as rz
    _set_env(monkeypatch, {})
    cap = ts.TOP_CAP if mode == "exact" else 8192
    scene, want_count, want_keys = _boundary(cap, True)
    budget = None if mode == "exact" else \
        rz.plan_pair_budget(dict(num_pairs=scene["G"], max_tile_list=max(ts.boundary_lengths(cap))), check="deferred")
    inp = _to(scene)
    a, bin_cap, capacity, _ = _forward(inp, scene["H"], scene["W"], budget)
    b, _, _, _ = _forward(inp, scene["H"], scene["W"], budget)
    if bin_cap:               # (slots past a bin's fill are never written: compare the lists)
        ka, kb = (ts.device_lists(s, _views(), 1, 1, scene["G"], scene["H"], scene["W"], bin_cap)[1] for s in (a, b))
        assert np.array_equal(ka, kb) and np.array_equal(ka, want_keys)
    else:
        assert torch.equal(a[4], b[4]) and a[4].numel() == scene["G"]
        assert np.array_equal(a[4].numpy().view(np.uint64), want_keys)          # (tile order = packed order)
        assert torch.equal(a[5], b[5])                                          # (the pair numbering, too)


# ---- random scenes: every binning and scan path ----------------------------------------------------------------------
def _random_inputs(name):
    batch, args, pr64 = random_scene(name)
    S, V = batch.extrinsics.shape[:2]
    inp = dict(means=batch.means, scales=batch.scales, rotations=batch.rotations, opacities=batch.opacities,
               shs=batch.harmonics.permute(0, 1, 3, 2).contiguous(),
               viewmatrix=torch.stack([a["viewmatrix"] for a in args]).reshape(S, V, 4, 4),
               projmatrix=torch.stack([a["projmatrix"] for a in args]).reshape(S, V, 4, 4),
               tanfov=torch.tensor([[a["tanfovx"], a["tanfovy"]] for a in args], dtype=torch.float32).reshape(S, V, 2),
               bg=torch.zeros(S, V, 3))
    return batch, inp, pr64


RANDOM_CASES = {
    # name: (scene, environment, options)
    "s1v3-bin_views1": ("s1v3", {"SPF_BIN_VIEWS": "1"}, {}),
    "s1v3-bin_views2": ("s1v3", {"SPF_BIN_VIEWS": "2"}, {}),                   # odd number of views: the last block holds one
    "s2v2-bin_views1": ("s2v2", {"SPF_BIN_VIEWS": "1"}, {}),
    "s2v2-bin_views2": ("s2v2", {"SPF_BIN_VIEWS": "2"}, {}),
    "s1v5-bin_views1": ("s1v5", {"SPF_BIN_VIEWS": "1"}, {}),
    "s1v5-bin_views2": ("s1v5", {"SPF_BIN_VIEWS": "2"}, {}),
    "s2v2-global_atomics": ("s2v2", {"SPF_MAX_LDS_TILES": "1"}, {}),           # no LDS histograms: one global atomic per pair
    "tiles1056-lds_no_prefetch": ("tiles1056", {}, {}),                        # > 1,024 tiles: tile starts not prefetched
    "s1v1-single_block_scan": ("s1v1", {}, {}),
    "s2v2-per_render_scan": ("s2v2", {}, {"camera": True}),                    # the decoder's prepared path, R = 4
    "s1v320-single_block_scan_again": ("s1v320", {}, {"camera": True}),        # R > 256
    "s1v320-plain": ("s1v320", {}, {}),
    "s2v2-chunks2": ("s2v2", {"SPF_CHUNKS": "2"}, {}),
    "s1v5-chunks3": ("s1v5", {"SPF_CHUNKS": "3"}, {}),                         # one scene: split by views
    "s2v2-cov3d": ("s2v2", {}, {"cov3d": True}),
    "s2v2-binding": ("s2v2", {}, {"binding": True}),
    "s1v3-binding-planned": ("s1v3", {}, {"binding": True, "planned": "classic"}),
    "s2v2-planned-classic": ("s2v2", {"SPF_DIRECT_BINS": "0"}, {"planned": "classic"}),
    "s2v2-direct_bins": ("s2v2", {}, {"planned": "direct"}),                   # multi-tile rects through the projection kernel's bins
    "s1v5-direct_bins-camera": ("s1v5", {}, {"planned": "direct", "camera": True}),
    "tiles1056-direct_bins": ("tiles1056", {}, {"planned": "direct"}),
}


@pytest.mark.parametrize("case", list(RANDOM_CASES))
def test_binning_and_scan_paths_on_random_scenes(hip_lib, monkeypatch, case):
    from spfsplatv2_amd import _lib, rasterizer as rz
    name, env, opt = RANDOM_CASES[case]
    _set_env(monkeypatch, env, binding=opt.get("binding", False))
    batch, inp, pr64 = _random_inputs(name)
    S, V, G = batch.extrinsics.shape[0], batch.extrinsics.shape[1], batch.means.shape[1]
    H, W = batch.image_shape
    dev = _to(inp)
    kw = {}
    if opt.get("cov3d"):
        # (the covariance of the rasterizer's own convention, quaternions used as given: what the oracle renders)
        from oracle import splat_ref
        kw["cov3D"] = rz._cov6(splat_ref.covariance3d(batch.scales, batch.rotations, 1.0).cuda(), S, G)
        dev["scales"] = dev["rotations"] = None
    if opt.get("camera"):
        # the decoder's path: the camera kernel writes the matrices and clears all the tile bookkeeping
        f32 = dict(dtype=torch.float32, device="cuda")
        dev["viewmatrix"], dev["projmatrix"] = torch.empty((S, V, 4, 4), **f32), torch.empty((S, V, 4, 4), **f32)
        dev["tanfov"] = torch.empty((S, V, 2), **f32)
        view64 = torch.empty((S, V, 4, 4), dtype=torch.float64, device="cuda")
        cam_in = [t.cuda().contiguous() for t in (batch.extrinsics, batch.intrinsics, batch.near, batch.far)]
        kw["camera"] = _lib.SpfCamera(*(rz._ptr(t) for t in cam_in), rz._ptr(dev["viewmatrix"]), rz._ptr(dev["projmatrix"]),
                                      rz._ptr(dev["tanfov"]), None, S * V, 0, rz._ptr(view64))
        kw["view64"] = view64
    budget = None
    if opt.get("planned"):
        D = sum(ts.splat_pairs(p) for p in pr64)
        longest = max(int(ts.expected_lists(ts.oracle_rect(p), np.zeros(G, np.uint32), H, W)[0].max()) for p in pr64)
        budget = rz.plan_pair_budget(dict(num_pairs=D, max_tile_list=longest), slack=1.5, check="deferred")
    t0 = time.perf_counter()
    state, bin_cap, capacity, rec = _forward(dev, H, W, budget, sh_degree=1, **kw)
    assert (bin_cap > 0) == (opt.get("planned") == "direct")
    if budget is not None:
        assert rz.plan_flags(rec) == 0
    if opt.get("binding"):
        assert _lib.fast() is not None                         # (the compiled binding really was the path)
    shards = hip_lib.spf_raster_pair_shards(S, G)
    out = ts.audit(state, S, V, G, H, W, bin_cap, capacity, _views(), shards=shards)
    assert out == [], out
    # the rects against the oracle (the camera path: against the oracle on the matrices the camera kernel wrote)
    if opt.get("camera"):
        _, args, _ = random_scene(name)
        v64, proj, tan = kw["view64"].cpu().reshape(-1, 4, 4), dev["projmatrix"].cpu().reshape(-1, 4, 4), dev["tanfov"].cpu().reshape(-1, 2)
        args = [dict(a, viewmatrix=v64[i], projmatrix=proj[i], tanfovx=float(tan[i, 0]), tanfovy=float(tan[i, 1]))
                for i, a in enumerate(args)]
        pr64 = ts.project_renders(args, torch.float64)
    v = _views()(state[2], state[3], state[5], S * V * np.prod(ts.grid(H, W)), S * V * G, S * V * ((G + 255) // 256))
    rect = (v.pair_off.view(-1, 2)[:, 0] if bin_cap else v.rect).numpy().view(np.uint32)
    out, share = ts.rects_against_oracle(pr64, rect, state[1].numpy().astype(np.int64), H, W)
    assert out == [] and share <= ts.FRAGILE_SHARE, (out, share)
    count = v.tile_count.numpy().view(np.uint32)
    _report("random-" + case, renders=S * V, tiles=int(count.size), pairs=int(count.sum()), longest=int(count.max()),
            bin_cap=bin_cap, knife_edge_share=round(share, 6), seconds=round(time.perf_counter() - t0, 3))
