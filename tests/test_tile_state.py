"""The tile-state auditor (tests/tile_state.py) held to account on the CPU: states built from the oracle in the device
layout audit clean, every single mutation is caught at the right tile, the boundary scene is what it claims to be, the
sort-class parametrisation reaches every sort kernel, and the random scenes of the GPU file stay inside the knife-edge
share."""
import functools

import numpy as np
import pytest
import torch

from spfsplatv2_amd import synthetic as syn
from tests import tile_state as ts
from tests.conftest import ROOT


def _views():
    from spfsplatv2_amd import rasterizer
    return rasterizer._state_views


def _clone(state):
    return tuple(t.clone() for t in state)


def _fields(state, S, V, G, H, W):
    """Named views INTO `state` (mutations through them change it)."""
    tiles_x, tiles_y = ts.grid(H, W)
    R = S * V
    return _views()(state[2], state[3], state[5], R * tiles_x * tiles_y, R * G, R * ((G + ts.BLOCK - 1) // ts.BLOCK))


# ---- scenes (built once, never changed) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _boundary(cap=512, interleaved=False, hw=None):
    scene = ts.boundary_scene(cap, interleaved, hw=hw, rotate=1)
    return scene, ts.project_boundary(scene, torch.float64)


@functools.lru_cache(maxsize=None)
def _random():
    batch = syn.make_batch("TEST", 2, 2, seed=31, s_mult=2.0, G=600, K=4, image_hw=(80, 72))
    args = ts.flat_renders(batch)
    return batch, ts.project_renders(args, torch.float64)


def _state(kind, direct, **kw):
    if kind == "boundary":
        scene, pr = _boundary()
        dims = (1, 1, scene["G"], scene["H"], scene["W"])
        projected = [pr]
    elif kind == "boundary_wide":
        scene, pr = _boundary(512, True, (1024, 512))
        dims = (1, 1, scene["G"], scene["H"], scene["W"])
        projected = [pr]
    else:
        batch, projected = _random()
        dims = (2, 2, batch.means.shape[1]) + tuple(batch.image_shape)
    S, V, G, H, W = dims
    bin_cap = 1024 if direct else 0
    state, capacity = ts.state_from_oracle(projected, S, V, H, W, bin_cap=bin_cap, slack=37, **kw)
    return state, dims, bin_cap, capacity


def _audit(state, dims, bin_cap, capacity, **kw):
    return ts.audit(state, *dims, bin_cap, capacity, _views(), **kw)


# ---- the clean states audit clean ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["boundary", "boundary_wide", "random"])
@pytest.mark.parametrize("direct", [False, True], ids=["classic", "direct"])
def test_oracle_state_is_clean(kind, direct):
    state, dims, bin_cap, capacity = _state(kind, direct)
    assert _audit(state, dims, bin_cap, capacity) == []
    if kind == "boundary_wide":
        assert ts.order_expected(dims[3] // 16 * (dims[4] // 16), 1024) and not ts.order_expected(2040, 1024)


def test_sharded_pair_numbering_is_clean_and_checked():
    """Eight shards: every block's records inside its shard's share; a record range that crosses into the next share, or
    sits in another shard's, is a violation."""
    state, dims, bin_cap, _ = _state("random", True)
    S, V, G, H, W = dims
    state, capacity = ts.state_from_oracle(_random()[1], S, V, H, W, bin_cap=bin_cap, shards=8, slack=5)
    assert _audit(state, dims, bin_cap, capacity, shards=8) == []
    assert _audit(state, dims, bin_cap, capacity, shards=1) != []          # (read as one shard: the cursors do not add up)
    bad = _clone(state)
    f = _fields(bad, *dims)
    off = f.pair_off.view(-1, 2)
    g = int(torch.nonzero((off[:, 0] != 0) & (off[:, 1] > 0))[0])          # (a Gaussian that has pairs)
    off[g, 1] += capacity // 8                       # the next shard's share
    out = _audit(bad, dims, bin_cap, capacity, shards=8)
    assert any(v.startswith("pair_shard") and f"gaussian {g % G}:" in v for v in out), out


# ---- one mutation at a time ------------------------------------------------------------------------------------------
def _tile_with(count, lo, pattern=None, rotate=1):
    """A tile with at least `lo` entries (of the boundary scene: one whose key pattern is `pattern`)."""
    for t in range(count.numel()):
        if int(count[t]) >= lo and (pattern is None or ts.KEY_PATTERNS[(t + rotate) % 5] == pattern):
            return t
    raise AssertionError("no such tile")


def _list_base(f, t, bin_cap):
    return t * bin_cap if bin_cap else int(f.tile_start[t])


def _names(violations, check, tile, T):
    tag = f"render {tile // T} tile {tile % T} "
    return any(v.startswith(check + ":") and tag in v for v in violations)


@pytest.mark.parametrize("kind", ["boundary", "random"])
@pytest.mark.parametrize("direct", [False, True], ids=["classic", "direct"])
def test_list_mutations_are_caught_at_their_tile(kind, direct):
    clean, dims, bin_cap, capacity = _state(kind, direct)
    S, V, G, H, W = dims
    T = np.prod(ts.grid(H, W))
    count = _fields(clean, *dims).tile_count

    def mutated(change):
        state = _clone(clean)
        change(state, _fields(state, *dims))
        return _audit(state, dims, bin_cap, capacity)

    t = _tile_with(count, 5)
    n = int(count[t])

    def swap_neighbours(state, f):
        b = _list_base(f, t, bin_cap) + n // 2
        state[4][[b, b + 1]] = state[4][[b + 1, b]]
    out = mutated(swap_neighbours)
    assert _names(out, "list", t, T) and all(_names([v], "list", t, T) for v in out), out
    assert f"pos {n // 2}:" in out[0] and f"pos {n // 2 + 1}:" in out[1]

    def copy_neighbour(state, f):
        b = _list_base(f, t, bin_cap) + 2
        state[4][b] = state[4][b + 1]
    out = mutated(copy_neighbour)
    assert len(out) == 1 and _names(out, "list", t, T) and "pos 2:" in out[0], out

    def drop_last(state, f):
        f.tile_count[t] -= 1
    out = mutated(drop_last)
    assert _names(out, "count", t, T), out
    assert [v for v in out if v.startswith("count")] == [v for v in out if _names([v], "count", t, T)], out
    if not direct:                         # (packed lists: every later tile's start is off by one, too)
        assert _names(out, "scan", t + 1, T) and not _names(out, "scan", t, T), out

    def garbage_last(state, f):
        state[4][_list_base(f, t, bin_cap) + n - 1] = 0x7FFFFFFF00000000
    out = mutated(garbage_last)
    assert len(out) == 1 and _names(out, "list", t, T) and f"pos {n - 1}:" in out[0], out

    if not direct:
        def shift_start(state, f):
            f.tile_start[t] += 1
        out = mutated(shift_start)
        assert _names(out, "scan", t, T) and _names(out, "list", t, T), out
        assert all(_names([v], v.split(":")[0], t, T) for v in out if not v.endswith("and more")), out

        def wrong_total(state, f):
            f.counters[0] += 1
        assert any(v.startswith("scan") for v in mutated(wrong_total))

        def wrong_longest(state, f):
            f.counters[1] -= 1
        assert any(v.startswith("scan") and "longest" in v for v in mutated(wrong_longest))

        def wrong_first_pair(state, f):
            f.pair_off.view(-1, 2)[G // 2:, 1] += 1
        out = mutated(wrong_first_pair)
        assert out and all(v.startswith("pair_off") for v in out) and f"gaussian {G // 2}:" in out[0], out

        def wrong_block(state, f):
            f.blk_base[1] += 1
        out = mutated(wrong_block)
        assert len(out) == 1 and out[0].startswith("blk: render 0 block 1"), out


def test_id_order_error_among_equal_depths_is_caught():
    """Two entries with EQUAL depth bits swapped: an error in the id half of the key only."""
    for direct in (False, True):
        clean, dims, bin_cap, capacity = _state("boundary", direct)
        T = np.prod(ts.grid(dims[3], dims[4]))
        f0 = _fields(clean, *dims)
        t = _tile_with(f0.tile_count, 64, pattern="equal")
        state = _clone(clean)
        b = _list_base(_fields(state, *dims), t, bin_cap)
        a, c = int(state[4][b + 10]), int(state[4][b + 11])
        assert a >> 32 == c >> 32 and a != c
        state[4][[b + 10, b + 11]] = state[4][[b + 11, b + 10]]
        out = _audit(state, dims, bin_cap, capacity)
        assert len(out) == 2 and all(_names([v], "list", t, T) for v in out) and "pos 10:" in out[0], out


def test_pair_range_overlap_and_launch_order_repeat_are_caught():
    clean, dims, bin_cap, capacity = _state("boundary_wide", True)
    S, V, G, H, W = dims
    T = np.prod(ts.grid(H, W))
    assert T >= ts.ORDER_MIN_TILES
    # two pair_off ranges overlap by one
    state = _clone(clean)
    off = _fields(state, *dims).pair_off.view(-1, 2)
    g = G // 3
    assert int(off[g + 1, 1]) == int(off[g, 1]) + 1          # (every rect of this scene is one tile)
    off[g + 1, 1] -= 1
    out = _audit(state, dims, bin_cap, capacity)
    assert any(v.startswith("pair_ranges") and f"gaussian {g} " in v and f"gaussian {g + 1} " in v for v in out), out
    # a tile repeated in the launch order
    state = _clone(clean)
    order = state[3][2 * T:4 * T].view(T, 2)
    order[7] = order[8]
    out = _audit(state, dims, bin_cap, capacity)
    assert _names(out, "order", 7, T) and "0 slots" in [v for v in out if _names([v], "order", 7, T)][0], out
    assert _names(out, "order", 8, T) and "2 slots" in [v for v in out if _names([v], "order", 8, T)][0], out
    # a stale length in the launch order
    state = _clone(clean)
    state[3][2 * T:4 * T].view(T, 2)[5, 1] += 1
    out = _audit(state, dims, bin_cap, capacity)
    assert len(out) == 1 and _names(out, "order", 5, T), out
    # ... and none of it is looked at when the library keeps no order (SPF_TILE_ORDER=0)
    assert _audit(state, dims, bin_cap, capacity, launch_order=False) == []


def test_rect_radii_depth_and_pixel_mutations_are_caught():
    clean, dims, bin_cap, capacity = _state("random", False)
    S, V, G, H, W = dims
    radii = clean[1]
    g = int(torch.nonzero(radii > 0)[3])
    state = _clone(clean)
    state[1][g] = 0
    assert any(v.startswith("radii_rect") and f"gaussian {g % G}:" in v for v in _audit(state, dims, bin_cap, capacity))
    state = _clone(clean)
    _fields(state, *dims).rect[g] = 0                 # (visible, centre on screen, but no tile)
    state[0][g, ts.REC_X], state[0][g, ts.REC_Y] = 5.0, 5.0
    out = _audit(state, dims, bin_cap, capacity)
    assert any(v.startswith("radii_rect") and "empty rect" in v for v in out), out
    state = _clone(clean)
    state[0][g, ts.REC_DEPTH] += 1.0
    out = _audit(state, dims, bin_cap, capacity)
    assert len(out) == 1 and out[0].startswith("depth") and f"gaussian {g % G}:" in out[0], out
    state = _clone(clean)
    state[7][(H // 2) * W + 3] += 1                   # one more contributor than the tile's list has entries
    out = _audit(state, dims, bin_cap, capacity)
    assert len(out) == 1 and out[0].startswith("pixels") and f"pixel (3, {H // 2})" in out[0], out
    state = _clone(clean)
    _fields(state, *dims).rect[g] = int(ts.pack_rect(0, 0, 200, 1))
    out = _audit(state, dims, bin_cap, capacity)
    assert out and out[0].startswith("rect_grid"), out


def test_views_handle_a_tiles_buffer_without_cursor_words():
    """`_state_views` on the two lengths of the tile buffer: with the eight pair cursors, and without them."""
    RT, RG, RB = 6, 10, 2
    rect, pair_idx = torch.arange(2 * RG + 3, dtype=torch.int32), torch.arange(2 * RG + 2 * RB, dtype=torch.int32)
    long, short = torch.arange(4 * RT + 16, dtype=torch.int32), torch.arange(4 * RT + 5, dtype=torch.int32)
    a, b = _views()(rect, long, pair_idx, RT, RG, RB), _views()(rect, short, pair_idx, RT, RG, RB)
    assert b.pair_cursor is None and a.pair_cursor.tolist() == list(range(4 * RT + 5, 4 * RT + 13))
    for v in (a, b):
        assert v.tile_count.tolist() == list(range(RT)) and v.tile_flags.tolist() == list(range(RT, 2 * RT))
        assert v.tile_start.tolist() == list(range(2 * RT, 3 * RT + 1))
        assert v.tile_fill.tolist() == list(range(3 * RT + 1, 4 * RT + 1))
        assert v.counters.tolist() == list(range(4 * RT + 1, 4 * RT + 5))
        assert v.rect.tolist() == list(range(RG)) and v.zkey[:RG].tolist() == list(range(RG, 2 * RG))
        assert v.sh_clamp.tolist() == list(range(2 * RG, 2 * RG + 3))
        assert v.pair_off.tolist() == list(range(2 * RG)) and v.blk_total.tolist() == list(range(2 * RG, 2 * RG + RB))
        assert v.blk_base.tolist() == list(range(2 * RG + RB, 2 * RG + 2 * RB))
    assert _views()(rect[:2 * RG], long, pair_idx, RT, RG, RB).sh_clamp is None


# ---- the boundary scene is what it claims to be ----------------------------------------------------------------------
def test_boundary_scene_construction():
    """20,000 Gaussians at z in [1, 100]: radius 3 for every one, the centre within 1e-5 px of its tile's centre pixel
    (margin to the tile edge: 4.5 px), every one in exactly its tile, and bits(z) the bits of the input z -- in float64
    and in float32."""
    scene = ts.boundary_scene(0, False, lengths=[0, 1, 2, 3, 4999, 5000, 5001, 4994], rotate=0,
                              patterns=("random", "equal", "descending", "ulp_steps"))
    assert scene["G"] == 20000 and float(scene["z"].min()) >= 1.0 and float(scene["z"].max()) <= 100.0
    tiles_x, _ = ts.grid(scene["H"], scene["W"])
    want_xy = np.stack([16 * (scene["tile_of"] % tiles_x) + 7.5, 16 * (scene["tile_of"] // tiles_x) + 7.5], axis=1)
    for dtype in (torch.float64, torch.float32):
        pr = ts.project_boundary(scene, dtype)
        assert bool((pr.radii == 3).all())
        err = float(np.abs(pr.xy.double().numpy() - want_xy).max())
        print(f"boundary scene, {dtype}: max pixel error {err:.3g}")
        assert err <= 1e-5, (dtype, err)
        assert np.array_equal(ts.f32_bits(pr.depth.float().numpy()), ts.f32_bits(scene["z"]))
        lo, hi = pr.rect_min.numpy(), pr.rect_max.numpy()
        assert np.array_equal(lo[:, 1] * tiles_x + lo[:, 0], scene["tile_of"]) and bool((hi == lo + 1).all())


@pytest.mark.parametrize("cap,interleaved,hw", [(512, False, None), (4096, True, None), (ts.TOP_CAP, True, None),
                                                (2048, False, (1024, 512))])
def test_boundary_scene_lists_follow_from_the_inputs(cap, interleaved, hw):
    """Every key pattern included (z from 0.25 to 1e4): the oracle, in float64 and float32, puts every Gaussian in exactly
    its tile, so the tile counts are the intended lengths and the lists are the sorted keys of the inputs."""
    scene = ts.boundary_scene(cap, interleaved, hw=hw, rotate=2)
    L = ts.boundary_lengths(cap)
    assert scene["lengths"][:len(L)].tolist() == L and set(scene["lengths"][len(L):].tolist()) <= {0, 1}
    assert set(ts.BASE_LENGTHS) <= set(L) and all({b - 1, b, b + 1} <= set(L) for b in ts.SORT_BORDERS if b <= cap)
    assert (set(ts.TOP_LENGTHS) <= set(L)) == (cap == ts.TOP_CAP)
    want_count, want_keys = ts.boundary_expected(scene)
    for dtype in (torch.float64, torch.float32):
        pr = ts.project_boundary(scene, dtype)
        # (radius 3 from z = 1 on; at z = 0.25 on a 1,024 px image the perspective term of the footprint brings it to 7:
        #  still 0.5 px inside the tile, 7.5 px from its centre pixel to its edge)
        assert 3 <= int(pr.radii.min()) and int(pr.radii.max()) <= 7
        assert bool((pr.radii[torch.from_numpy(scene["z"] >= 1.0)] == 3).all())
        rect = ts.pack_rect(pr.rect_min[:, 0].numpy(), pr.rect_min[:, 1].numpy(), pr.rect_max[:, 0].numpy(),
                            pr.rect_max[:, 1].numpy())
        count, keys = ts.expected_lists(rect, ts.f32_bits(pr.depth.float().numpy()), scene["H"], scene["W"])
        assert np.array_equal(count, want_count) and np.array_equal(keys, want_keys)
    # ids: contiguous runs per tile, or dealt round the tiles
    t = scene["tile_of"]
    if interleaved:
        assert int((np.diff(t) != 0).sum()) > scene["G"] // 2
    else:
        assert bool((np.diff(t) >= 0).all())


# ---- the parametrisation reaches every sort kernel -------------------------------------------------------------------
def check_sort_plan_coverage(lib, monkeypatch):
    """Union, over the sort-class cases, of the kernels whose size class holds one of the case's list lengths -- exact
    mode (hint: the longest list) and the planned classic chain (hint: the plan's class): every SPF_SORT_* kernel except
    ORDER_ONLY (which the launch-order test covers)."""
    ids = ts.sort_ids((ROOT / "include" / "spfsplat_hip.h").read_text())
    names = {v: k for k, v in ids.items() if k != "MAX_LAUNCHES"}
    seen, per_case = set(), {}
    for case in ts.sort_cases():
        cap, env, interleaved = case
        for name in ts.SORT_ENV:
            monkeypatch.delenv(name, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L = ts.boundary_lengths(cap)
        tiles = len(ts.boundary_scene(cap, interleaved, lengths=[0] * len(L))["lengths"])
        longest = max(L)
        planned = next((c for c in (128, 256, 512, 1024, 2048, 4096, 8192, 16384) if c >= int(longest * 1.25) + 1), 0)
        got = set()
        for hint in (longest, planned):
            plan = ts.sort_plan(lib, hint, tiles)
            reach = 1
            for _, lo, hi in sorted(plan, key=lambda p: p[1]):
                assert lo == reach
                reach = hi
            assert reach >= longest
            got |= ts.kernels_sorting(plan, L)
        per_case[ts.case_id(case)] = sorted(names[k] for k in got)
        seen |= got
    for name in ts.SORT_ENV:
        monkeypatch.delenv(name, raising=False)
    assert {names[k] for k in seen} == set(names.values()) - {"ORDER_ONLY"}, per_case
    return per_case


def test_sort_cases_cover_every_sort_kernel(hip_lib, monkeypatch):
    per_case = check_sort_plan_coverage(hip_lib, monkeypatch)
    assert len(per_case) == len(ts.sort_cases())          # (ids are unique)


DIRECT_BIN_CAPS = tuple(c for c in ts.CAPS if c <= 8192)


def test_direct_bins_take_the_caps_up_to_8192(hip_lib):
    """Which boundary cases a plan runs with direct bins: a plan names a list class of at most 16,384 entries >= 1.25 x
    the longest list, so the cases up to 8,192 (longest list 8,193) get bins; from 16,384 on (longest 16,385) the class
    is unknown and the call takes the classic chain."""
    from spfsplatv2_amd import rasterizer as rz
    for cap in ts.CAPS:
        L = ts.boundary_lengths(cap)
        T = len(ts.boundary_scene(cap, False, lengths=[0] * len(L))["lengths"])
        budget = rz.plan_pair_budget(dict(num_pairs=sum(L), max_tile_list=max(L)), check="deferred")
        assert (rz._direct_bin_cap(budget, T, T) > 0) == (cap in DIRECT_BIN_CAPS), cap


# ---- the random scenes of the GPU file -------------------------------------------------------------------------------
RANDOM_SCENES = {
    # name: (S, V, G, (H, W), seed, s_mult) -- the shapes of test_two_views_per_binning_block_give_the_same_lists, then one
    # render, more than 256 renders of a tiny image, and an image of more than 1,024 tiles
    "s1v3": (1, 3, 3000, (80, 72), 31, 2.0),
    "s2v2": (2, 2, 1500, (80, 72), 31, 2.0),
    "s1v5": (1, 5, 700, (80, 72), 31, 2.0),
    "s1v1": (1, 1, 3000, (80, 72), 32, 2.0),
    "s1v320": (1, 320, 400, (32, 48), 71, 20.0),
    "tiles1056": (1, 1, 2500, (528, 512), 61, 40.0),
}


@functools.lru_cache(maxsize=None)
def random_scene(name):
    """(batch, rasterizer arguments per render, float64 projection per render) -- shared, never changed."""
    S, V, G, hw, seed, s_mult = RANDOM_SCENES[name]
    batch = syn.make_batch("TEST", S, V, seed=seed, s_mult=s_mult, G=G, K=4, image_hw=hw)
    args = ts.flat_renders(batch)
    return batch, args, ts.project_renders(args, torch.float64)


@pytest.mark.parametrize("name", list(RANDOM_SCENES))
def test_random_scenes_stay_inside_the_knife_edge_share(name):
    """The float32 oracle standing in for the device: away from the Gaussians `radii_fragile` flags -- at most 0.5 % of
    them -- its radii and rects are the float64 oracle's, and multi-tile rects are there to be binned."""
    batch, args, pr64 = random_scene(name)
    H, W = batch.image_shape
    pr32 = ts.project_renders(args, torch.float32)
    rect = np.concatenate([ts.pack_rect(p.rect_min[:, 0].numpy(), p.rect_min[:, 1].numpy(), p.rect_max[:, 0].numpy(),
                                        p.rect_max[:, 1].numpy()) for p in pr32])
    radii = np.concatenate([p.radii.numpy().astype(np.int64) for p in pr32])
    out, share = ts.rects_against_oracle(pr64, rect, radii, H, W)
    print(f"{name}: knife-edge share {share:.5f}")
    assert out == [] and share <= ts.FRAGILE_SHARE, (out, share)
    x0, y0, x1, y1, empty = ts.unpack_rect(rect)
    area = np.where(empty, 0, (x1 - x0) * (y1 - y0))
    assert int((area > 1).sum()) > int((area == 1).sum()) // 4 and int(area.sum()) > 1000
    # a rect that drops a contributing tile, or grows past the 3-sigma rect, is caught
    g = int(np.nonzero(area > 1)[0][0])
    grown = rect.copy()
    grown[g] = ts.pack_rect(x0[g], y0[g], x1[g] + 1, y1[g])[()]
    assert any(v.startswith("rect:") for v in ts.rects_against_oracle(pr64, grown, radii, H, W)[0])
