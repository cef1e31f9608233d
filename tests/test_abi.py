"""C-ABI surface: the library loads without a GPU and exports exactly what include/spfsplat_hip.h declares."""
import ctypes as C
import re

from tests.conftest import ROOT


def _declared_symbols():
    text = (ROOT / "include" / "spfsplat_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(spf_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_all_exported(hip_lib):
    from spfsplatv2_amd import _lib
    declared = _declared_symbols()
    assert declared, "no symbols parsed from the header"
    assert sorted(_lib.SYMBOLS) == declared
    for name in declared:
        assert hasattr(hip_lib, name), name
    assert hip_lib.spf_abi_version() == _lib.ABI_VERSION


def test_struct_sizes_match_header():
    from spfsplatv2_amd import _lib
    assert C.sizeof(_lib.SpfDims) == 72          # ten 4-byte fields + bin_cap + the 8-byte aligned pair_capacity (ABI 4) + raw_stride, adapter_eps (ABI 6)
    assert _lib.SpfDims.pair_capacity.offset == 48 and _lib.SpfDims.bin_cap.offset == 40
    assert C.sizeof(_lib.SpfInputs) == 15 * 8          # + shs_high, raw, sh_mask (ABI 6)
    assert C.sizeof(_lib.SpfState) == 18 * 8            # + verdict_host (ABI 6)
    assert C.sizeof(_lib.SpfOutputs) == 3 * 8
    assert C.sizeof(_lib.SpfGrads) == 15 * 8           # + dL_dshs_high, dL_draw (ABI 6)
    assert C.sizeof(_lib.SpfStateLayout) == 12 * 8     # three sizes, nine offsets, int64 each


def test_host_helpers_no_gpu(hip_lib):
    assert hip_lib.spf_raster_num_tiles(256, 256) == 256
    assert hip_lib.spf_raster_num_tiles(100, 33) == 7 * 3
    assert hip_lib.spf_raster_view_partial_blocks(65536) == 256
    assert hip_lib.spf_raster_view_partial_blocks(257) == 2
    assert hip_lib.spf_stage_kernel_name(5) == b"spf_render_bwd_lists_kernel"


def test_state_layout_is_the_headers(hip_lib):
    """spf_raster_state_layout against the three buffers as include/spfsplat_hip.h words them (formulas written out here,
    not taken from product code): rect (RG) | zkey (RG) | sh_clamp (RG bytes, whole words); tile_count (RT) | tile_flags
    (RT) | tile_start (RT + 1) | tile_fill (RT) | counters (4) | pair_cursor (8) | padding to 16 bytes; pair_off (2 RG) |
    blk_total (RB) | blk_base (RB).  (6, 903, 6): one scene, three views of 301 Gaussians at 40 x 24 px -- a partial last
    block, partial edge tiles and RG % 4 == 3, so the clamp bytes round up."""
    from spfsplatv2_amd import _lib
    for RT, RG, RB in ((1, 1, 1), (6, 903, 6), (2048, 524288, 2048)):
        lay = _lib.SpfStateLayout()
        assert hip_lib.spf_raster_state_layout(RT, RG, RB, C.byref(lay)) == 0
        got = {f: getattr(lay, f) for f, _ in _lib.SpfStateLayout._fields_}
        assert got == dict(rect_words=2 * RG + (RG + 3) // 4, tiles_words=4 * RT + 16, pair_idx_words=2 * RG + 2 * RB,
                           zkey=RG, sh_clamp=2 * RG, tile_flags=RT, tile_start=2 * RT, tile_fill=3 * RT + 1,
                           counters=4 * RT + 1, pair_cursor=4 * RT + 5, blk_total=2 * RG, blk_base=2 * RG + RB), (RT, RG, RB)
        # every field's extent (in words) ends at or before the next field of its buffer, and the last inside the buffer
        buffers = ((("rect", 0, RG), ("zkey", lay.zkey, RG), ("sh_clamp", lay.sh_clamp, (RG + 3) // 4), lay.rect_words),
                   (("tile_count", 0, RT), ("tile_flags", lay.tile_flags, RT), ("tile_start", lay.tile_start, RT + 1),
                    ("tile_fill", lay.tile_fill, RT), ("counters", lay.counters, 4), ("pair_cursor", lay.pair_cursor, 8),
                    lay.tiles_words),
                   (("pair_off", 0, 2 * RG), ("blk_total", lay.blk_total, RB), ("blk_base", lay.blk_base, RB),
                    lay.pair_idx_words))
        for *fields, words in buffers:
            starts = [off for _, off, _ in fields] + [words]
            for (name, off, extent), nxt in zip(fields, starts[1:]):
                assert off < nxt and off + extent <= nxt, (RT, RG, RB, name)
        assert (4 * lay.tiles_words) % 16 == 0 and lay.pair_cursor + 8 <= lay.tiles_words
    lay = _lib.SpfStateLayout()
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-6, 903, 6)):
        assert hip_lib.spf_raster_forward_project(None, None, None, None) == -1          # (another error in between)
        assert hip_lib.spf_raster_state_layout(*bad, C.byref(lay)) == -1                 # SPF_E_INVALID
        assert b"state_layout" in hip_lib.spf_last_error() and b"positive" in hip_lib.spf_last_error(), bad
    assert hip_lib.spf_raster_state_layout(1, 1, 1, None) == -1


def test_launch_slots_cover_every_tile_once(hip_lib):
    """The (XCD, slot) -> tile map of the composite lists launches (spf_common.h::xcd_map) is a bijection for every
    shape -- contiguous ranges of renders per XCD, and strips dealt out when the call has exactly eight renders."""
    for R, T in ((32, 256), (16, 256), (8, 256), (8, 1024), (8, 64), (8, 4096), (8, 200), (24, 256), (9, 256), (128, 16)):
        RT = R * T
        if RT % 8:
            assert hip_lib.spf_raster_launch_slot_tile(R, T, 0, 0) == -1
            continue
        per = RT // 8
        seen = set()
        for x in range(8):
            for j in range(per):
                seen.add(hip_lib.spf_raster_launch_slot_tile(R, T, x, j))
        assert seen == set(range(RT)), (R, T)
        dealt = R == 8 and T % 64 == 0 and T > 64                 # (T == 64: one strip per render, the same map)
        contiguous = all(hip_lib.spf_raster_launch_slot_tile(R, T, x, j) == x * per + j
                         for x in range(8) for j in range(0, per, 61))
        assert contiguous != dealt, (R, T, dealt, contiguous)
    assert hip_lib.spf_raster_launch_slot_tile(8, 256, 8, 0) == -1 and hip_lib.spf_raster_launch_slot_tile(8, 256, 0, 256) == -1


_SORT_ENV = ("SPF_SORT_BLOCKS", "SPF_SORT_BIG_MIXED", "SPF_SORT_SEPARATE", "SPF_SORT_LDS_2K", "SPF_SORT_SINGLE")
_SORT_INF = 0xffffffff


def _sort_ids():
    """The SPF_SORT_* kernel ids of the header, by name without the prefix."""
    text = (ROOT / "include" / "spfsplat_hip.h").read_text()
    return {name: int(val) for name, val in re.findall(r"#define SPF_SORT_([A-Z0-9_]+) (\d+)\b", text)}


def _sort_plan_arrays():
    n_max = _sort_ids()["MAX_LAUNCHES"]
    return (C.c_int32 * n_max)(), (C.c_uint32 * n_max)(), (C.c_uint32 * n_max)(), (C.c_int32 * n_max)()


def _sort_plan(hip_lib, hint, tiles, with_order):
    kernel, lo, hi, order = _sort_plan_arrays()
    n = hip_lib.spf_raster_sort_plan(hint, tiles, int(with_order), kernel, lo, hi, order)
    assert 0 <= n <= len(kernel), (hint, tiles, with_order, n)
    return [(kernel[i], lo[i], hi[i], order[i]) for i in range(n)]


def _set_sort_env(monkeypatch, **values):
    for name in _SORT_ENV:
        v = values.get(name[len("SPF_SORT_"):].lower())
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


def test_sort_plan_covers_every_list_length_once(hip_lib, monkeypatch):
    """Every tile sort kernel sorts the lists of its own size class (lo, hi] and skips the rest, so a call is sorted iff
    the classes of its launches (binning.hip::plan_tile_sort, through spf_raster_sort_plan) tile (1, hint] without gap or
    overlap -- for every hint around the class borders, both families by tile count, and every setting of the five
    switches.  The launch order blocks ride on the first launch, and only there."""
    import itertools
    ids = _sort_ids()
    hints = (0, 1, 2, 64, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 131072)
    combos = 0
    for blocks, big_mixed, separate, lds_2k, single in itertools.product(
            (None, "0", "1"), (None, "0", "1"), (None, "1"), (None, "1"), (None, "1")):
        _set_sort_env(monkeypatch, blocks=blocks, big_mixed=big_mixed, separate=separate, lds_2k=lds_2k, single=single)
        combos += 1
        for hint, tiles, with_order in itertools.product(hints, (256, 6143, 6144, 8192), (False, True)):
            plan = _sort_plan(hip_lib, hint, tiles, with_order)
            where = (blocks, big_mixed, separate, lds_2k, single, hint, tiles, with_order, plan)
            assert [o for _, _, _, o in plan] == ([1] + [0] * (len(plan) - 1) if with_order else [0] * len(plan)), where
            sorts = sorted((lo, hi) for k, lo, hi, _ in plan if k != ids["ORDER_ONLY"])
            if hint == 1:
                assert [k for k, _, _, _ in plan] == ([ids["ORDER_ONLY"]] if with_order else []), where
                continue
            assert len(sorts) == len(plan), where
            reach = 1
            for lo, hi in sorts:
                assert lo == reach and hi > lo, where
                reach = hi
            assert reach >= (hint if hint else _SORT_INF), where
    assert combos == 72
    assert hip_lib.spf_raster_sort_plan(64, 0, 0, *_sort_plan_arrays()) == -1                       # nonsense arguments
    assert hip_lib.spf_raster_sort_plan(64, 256, 0, None, None, None, None) == -1


def test_sort_plan_defaults_and_switches_are_pinned(hip_lib, monkeypatch):
    """What a call launches by default, per hint and family, and what each switch changes (the launches of the chain of
    conditions this table replaced, derived from its code)."""
    ids = _sort_ids()
    names = {v: k for k, v in ids.items() if k != "MAX_LAUNCHES"}

    def plan(hint, tiles, with_order=False):
        return [(names[k], lo, hi) for k, lo, hi, _ in _sort_plan(hip_lib, hint, tiles, with_order)]

    _set_sort_env(monkeypatch)
    lds_4k, lds_8k, big = ("LDS", 4096, 8192), ("LDS", 8192, 16384), ("BIG", 16384, _SORT_INF)
    tails = ((4097, 8192, [lds_4k]), (8193, 16384, [lds_4k, lds_8k]), (16385, 131072, [lds_4k, lds_8k, big]),
             (0, 0, [lds_4k, lds_8k, big]))
    few = [(2, 512, [("WAVE8", 1, 512)]), (513, 2048, [("MIXED", 1, 2048)]), (2049, 4096, [("MIXED_BIG", 1, 4096)])]
    few += [(a, b, few[-1][2] + tail) for a, b, tail in tails]
    waves = [("WAVE16", 1, 1024), ("WAVE32", 1024, 2048)]
    many = [(2, 1024, [("PAIR", 1, 1024)]), (1025, 2048, waves), (2049, 4096, waves + [("BLOCK16", 2048, 4096)])]
    many += [(a, b, many[-1][2] + tail) for a, b, tail in tails]
    for tiles_of, table in (((1, 256, 6143), few), ((6144, 8192, 1 << 20), many)):
        for tiles in tiles_of:
            for a, b, want in table:
                for hint in {a, (a + b) // 2, b}:
                    assert plan(hint, tiles) == want, (hint, tiles)
                    assert plan(hint, tiles, True) == want, (hint, tiles)
            assert plan(1, tiles) == [] and plan(1, tiles, True) == [("ORDER_ONLY", 1, 1)]
    # one line per switch
    _set_sort_env(monkeypatch, separate="1")
    assert plan(2048, 256) == [("WAVE8", 1, 512), ("BLOCK4", 512, 1024), ("BLOCK8", 1024, 2048)]
    _set_sort_env(monkeypatch, big_mixed="0")
    assert plan(4096, 256) == [("MIXED", 1, 2048), ("BLOCK16", 2048, 4096)]
    _set_sort_env(monkeypatch, big_mixed="1")
    assert plan(4096, 256) == [("MIXED_BIG", 1, 4096)]
    _set_sort_env(monkeypatch, lds_2k="1")
    assert plan(4096, 256) == [("MIXED", 1, 2048), ("LDS", 2048, 8192)]
    assert plan(8192, 256) == [("MIXED", 1, 2048), ("LDS", 2048, 8192)]
    assert plan(8193, 8192) == waves + [("LDS", 2048, 8192), lds_8k]
    _set_sort_env(monkeypatch, single="1")
    assert plan(1024, 8192) == [("WAVE16", 1, 1024)] and plan(512, 8192) == [("WAVE8", 1, 512)]
    assert plan(1024, 256) == [("MIXED", 1, 2048)]                             # (the switch is the wave family's)
    for tiles in (256, 8192):
        _set_sort_env(monkeypatch, blocks="0")
        assert plan(2048, tiles) == waves and plan(1024, tiles) == [("PAIR", 1, 1024)]
        _set_sort_env(monkeypatch, blocks="1")
        assert plan(2048, tiles) == [("MIXED", 1, 2048)] and plan(512, tiles) == [("WAVE8", 1, 512)]


def test_argument_validation_without_compute(hip_lib):
    """Bad arguments are rejected before anything touches a device."""
    from spfsplatv2_amd import _lib
    d = _lib.SpfDims(1, 1, 0, 1, 0, 64, 64, 1.0, 0, 0)         # G = 0
    rc = hip_lib.spf_raster_forward_project(C.byref(d), C.byref(_lib.SpfInputs()), C.byref(_lib.SpfState()), None)
    assert rc == -1 and b"positive" in hip_lib.spf_last_error()
    d = _lib.SpfDims(1, 1, 8, 1, 0, 64, 64, 1.0, 0, 0)
    rc = hip_lib.spf_raster_forward_project(C.byref(d), C.byref(_lib.SpfInputs()), C.byref(_lib.SpfState()), None)
    assert rc == -1 and b"null" in hip_lib.spf_last_error()
    d = _lib.SpfDims(1, 1, 8, 1, 0, 64, 5000, 1.0, 0, 0)
    rc = hip_lib.spf_raster_forward_project(C.byref(d), C.byref(_lib.SpfInputs()), C.byref(_lib.SpfState()), None)
    assert rc == -1 and b"4080" in hip_lib.spf_last_error()
    # direct bins (ABI 4): the bins of all tiles must stay below 2^31 keys and the pair capacity must be given
    d = _lib.SpfDims(64, 64, 8, 1, 0, 1024, 1024, 1.0, 0, 0, 16384, 1000)
    rc = hip_lib.spf_raster_forward_project(C.byref(d), C.byref(_lib.SpfInputs()), C.byref(_lib.SpfState()), None)
    assert rc == -1 and b"2^31" in hip_lib.spf_last_error()
    d = _lib.SpfDims(1, 1, 8, 1, 0, 64, 64, 1.0, 0, 0, 128, 0)
    rc = hip_lib.spf_raster_forward_project(C.byref(d), C.byref(_lib.SpfInputs()), C.byref(_lib.SpfState()), None)
    assert rc == -1 and b"pair_capacity" in hip_lib.spf_last_error()
    rc = hip_lib.spf_rope2d(None, None, 1, 1, 1, 64, 64, 64, 64, 1, 0, 100.0, 1.0, None)
    assert rc == -1
    rc = hip_lib.spf_rope2d(C.c_void_p(16), C.c_void_p(16), 1, 1, 1, 6, 6, 6, 6, 1, 0, 100.0, 1.0, None)
    assert rc == -1 and b"multiple of 4" in hip_lib.spf_last_error()


def test_product_refuses_cpu_tensors(hip_lib):
    """No silent fallback: CPU tensors raise."""
    import pytest
    import torch

    import spfsplatv2_amd as spf
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_2d(torch.zeros(1, 4, 2, 16), torch.zeros(1, 4, 2, dtype=torch.int64), 100.0, 1.0)
    G = 4
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rasterize_batch(torch.zeros(1, G, 3), torch.ones(1, G, 3), torch.ones(1, G, 4), torch.ones(1, G),
                            torch.zeros(1, G, 1, 3), None, torch.eye(4)[None, None], torch.eye(4)[None, None],
                            torch.ones(1, 1, 2), torch.zeros(3), 16, 16, 0)


def test_chunk_planning_is_off_by_default_and_whole_scenes(hip_lib, monkeypatch):
    """spf_raster_chunks: 1 unless SPF_CHUNKS asks; whole scenes per chunk (the backward needs that), single scenes
    split by views in the forward only, never more chunks than units."""
    monkeypatch.delenv("SPF_CHUNKS", raising=False)
    assert hip_lib.spf_raster_chunks(8, 4, 256, 256, 0) == 1 and hip_lib.spf_raster_chunks(8, 4, 256, 256, 1) == 1
    monkeypatch.setenv("SPF_CHUNKS", "4")
    assert hip_lib.spf_raster_chunks(8, 4, 256, 256, 0) == 4 and hip_lib.spf_raster_chunks(8, 4, 256, 256, 1) == 4
    assert hip_lib.spf_raster_chunks(3, 2, 256, 256, 0) == 3                  # never more chunks than scenes
    assert hip_lib.spf_raster_chunks(1, 8, 512, 512, 0) == 4                  # one scene: by views, forward only
    assert hip_lib.spf_raster_chunks(1, 8, 512, 512, 1) == 1
    monkeypatch.setenv("SPF_CHUNKS", "1")
    assert hip_lib.spf_raster_chunks(8, 4, 256, 256, 0) == 1
    assert hip_lib.spf_raster_chunks(0, 4, 256, 256, 0) == 1                  # nonsense sizes: one chain


def test_compiled_host_binding_loads_and_can_be_switched_off(hip_lib, monkeypatch):
    """csrc/torch_binding.cpp -> _spf_torch.so: the same C ABI driven from C++ (no compute here).  It is optional at
    run time: absent or SPF_NO_FAST=1, rasterizer.py keeps its ctypes path."""
    import pytest

    from spfsplatv2_amd import _lib, build
    try:
        build.build_binding(verbose=False)
    except Exception as e:  # noqa: BLE001  (no g++ / torch headers: nothing to test)
        pytest.skip(f"binding does not build here: {e}")
    monkeypatch.setattr(_lib, "_fast", False)
    monkeypatch.delenv("SPF_NO_FAST", raising=False)
    mod = _lib.fast()
    assert mod is not None and mod.abi_version() == _lib.ABI_VERSION
    assert callable(mod.raster_forward) and callable(mod.raster_backward)
    import torch
    with pytest.raises(Exception):                      # CPU tensors never reach a launch
        mod.raster_forward(torch.zeros(1, 4, 3), torch.ones(1, 4, 3), torch.ones(1, 4, 4), torch.ones(1, 4), None,
                           torch.zeros(1, 4, 3), torch.eye(4)[None, None], torch.eye(4)[None, None],
                           torch.ones(1, 1, 2), torch.zeros(1, 1, 3), None, None, 16, 16, 0, 1.0, 0, False, -1, 0, 0)
    monkeypatch.setattr(_lib, "_fast", False)
    monkeypatch.setenv("SPF_NO_FAST", "1")
    assert _lib.fast() is None
    monkeypatch.setattr(_lib, "_fast", False)


def test_direct_bins_planning_helpers(hip_lib):
    """Host-side planning of a direct-bins call (no GPU): the pair numbering is sharded from 512 blocks on, the host
    then adds a quarter to the gradient-record capacity (each shard owns an eighth: ADVICE r4, r5), and the bins stay in proportion to
    the plan -- BASELINE config 3 (2,048 tiles, lists of ~1,700 -> 4,096-entry bins) keeps them, a 16,384-entry class on
    8,192 tiles (1 GiB of keys) falls back to the classic chain."""
    from spfsplatv2_amd import rasterizer as rz
    assert hip_lib.spf_raster_pair_shards(1, 256 * 511) == 1 and hip_lib.spf_raster_pair_shards(1, 256 * 512) == 8
    assert hip_lib.spf_raster_pair_shards(8, 65536) == 8 and hip_lib.spf_raster_pair_shards(2, 3000) == 1
    assert hip_lib.spf_raster_max_lds_tiles() == 4096
    assert rz._record_capacity(1000, 2, 3000) == 1000 and rz._record_capacity(1000, 8, 65536) == 1250
    c3 = rz.plan_pair_budget(dict(num_pairs=2_170_000, max_tile_list=1700, dense_tiles=0, tiles=2048))
    assert c3.max_tile_list == 4096 and rz._direct_bin_cap(c3, 2048, 256) == 4096
    c2 = rz.plan_pair_budget(dict(num_pairs=2_250_000, max_tile_list=505, dense_tiles=0, tiles=8192))
    assert c2.max_tile_list == 1024 and rz._direct_bin_cap(c2, 8192, 256) == 1024
    coarse = c2._replace(max_tile_list=16384)
    assert rz._direct_bin_cap(coarse, 8192, 256) == 0                      # 134 M keys: the classic chain
    assert rz._direct_bin_cap(c2, 8192, 4097) == 0                         # more tiles per render than the LDS histogram holds
    assert rz._direct_bin_cap(None, 8192, 256) == 0 and rz._direct_bin_cap(12345, 8192, 256) == 0   # exact mode / bare capacity
