"""Audit of the tile lists a forward call of the rasterizer leaves behind (TEST INFRASTRUCTURE ONLY).

Binning, the tile scan and the tile sort are an all-integer contract: given the device's own packed rects and depth keys,
every tile's list, its length, its start and the numbering of the (Gaussian, tile) pairs are determined exactly.
`audit` checks that contract on HOST COPIES of the state tensors (plain numpy; this module does not import the product --
the one thing it needs from it, where each field sits inside the shared buffers, is handed in as `views`:
`spfsplatv2_amd.rasterizer._state_views`, the function the launcher itself slices with).

`boundary_scene` builds the inputs whose tile lists are known from the inputs alone: Gaussian g projects to the centre
pixel of one chosen tile with a 3 px radius, so tile i holds exactly `L[i]` Gaussians, with `L` sitting on both sides of
every border between two sort kernels.  `state_from_oracle` writes the state a correct device would leave for a scene
the CPU oracle projected -- what the auditor's own tests mutate.
"""
from __future__ import annotations

import numpy as np
import torch

TILE = 16
REC = 12            # floats per screen-space record
REC_X, REC_Y, REC_DEPTH, REC_CULL_R2 = 0, 1, 6, 7      # (project.hip: rec0 = px, py, A, B; rec1 = C, opacity, z, cull r^2)
BLOCK = 256         # Gaussians per block of the projection / binning kernels (spf_raster_view_partial_blocks)
ORDER_MIN_TILES = 2048
ORDER_TILE_MASK = 0x3FFFFFFF
SORT_BORDERS = (512, 1024, 2048, 4096, 8192, 16384)
BASE_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257)
TOP_LENGTHS = (32768, 32769, 49153, 65537)
TOP_CAP = 65537
CAPS = SORT_BORDERS + (TOP_CAP,)
KEY_PATTERNS = ("random", "equal", "descending", "ulp_steps", "wide")
MAX_REPORT = 12     # violations spelled out per check (the rest is counted)


def grid(H: int, W: int):
    return (W + TILE - 1) // TILE, (H + TILE - 1) // TILE


def f32_bits(z) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(z, dtype=np.float32)).view(np.uint32)


def make_keys(zbits: np.ndarray, ids: np.ndarray) -> np.ndarray:
    """The sort key of the contract: float32 bits of view-space z << 32 | Gaussian id (within its render)."""
    return (zbits.astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)


def unpack_rect(rect: np.ndarray):
    """xmin | ymin << 8 | xmax << 16 | ymax << 24, max exclusive -> (x0, y0, x1, y1) int64 and the `empty` mask."""
    r = rect.astype(np.int64)
    x0, y0, x1, y1 = r & 0xFF, (r >> 8) & 0xFF, (r >> 16) & 0xFF, (r >> 24) & 0xFF
    return x0, y0, x1, y1, (x1 <= x0) | (y1 <= y0)


def pack_rect(x0, y0, x1, y1) -> np.ndarray:
    return (np.asarray(x0, np.int64) | (np.asarray(y0, np.int64) << 8) | (np.asarray(x1, np.int64) << 16)
            | (np.asarray(y1, np.int64) << 24)).astype(np.uint32)


def expand_pairs(x0, y0, x1, y1, empty, tiles_x: int):
    """Every (Gaussian, tile) pair of one render, Gaussian-major with the tiles of a rect in row-major order (the pair
    numbering): (Gaussian index, tile index) per pair, and the rect areas."""
    w = np.where(empty, 0, x1 - x0)
    area = w * np.where(empty, 0, y1 - y0)
    g = np.repeat(np.arange(area.size, dtype=np.int64), area)
    first = np.cumsum(area) - area
    k = np.arange(g.size, dtype=np.int64) - first[g]
    wg = np.maximum(w[g], 1)
    tile = (y0[g] + k // wg) * tiles_x + x0[g] + k % wg
    return g, tile, area


def expected_lists(rect: np.ndarray, zbits: np.ndarray, H: int, W: int):
    """(counts [T], keys: every tile's list back to back in tile order, each `np.sort`ed) of one render."""
    tiles_x, tiles_y = grid(H, W)
    x0, y0, x1, y1, empty = unpack_rect(rect)
    g, tile, _ = expand_pairs(x0, y0, x1, y1, empty, tiles_x)
    key = make_keys(zbits[g], g)
    order = np.lexsort((key, tile))
    return np.bincount(tile, minlength=tiles_x * tiles_y).astype(np.int64), key[order]


class _Report:
    def __init__(self):
        self.out, self.seen = [], {}

    def add(self, check: str, text: str):
        n = self.seen[check] = self.seen.get(check, 0) + 1
        if n <= MAX_REPORT:
            self.out.append(f"{check}: {text}")
        elif n == MAX_REPORT + 1:
            self.out.append(f"{check}: ... and more")

    def add_each(self, check: str, idx, fmt):
        for i in np.asarray(idx).reshape(-1)[:MAX_REPORT + 1]:
            self.add(check, fmt(int(i)))


def _np(t, dtype=None):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a if dtype is None else a.view(dtype)


def order_expected(RT: int, bin_cap: int) -> bool:
    """Whether a direct-bins call keeps the composite kernels' launch order in tile_start | tile_fill (the library's
    condition, spf_common.h::tile_order_ptr; `SPF_TILE_ORDER=0` switches it off: the caller says so)."""
    return 0 < bin_cap <= 65536 and RT >= ORDER_MIN_TILES and RT % 8 == 0


def audit(state, S: int, V: int, G: int, H: int, W: int, bin_cap: int, capacity: int, views, shards: int = 1,
          launch_order: bool | None = None) -> list:
    """Violations of the tile-list contract in one forward call's state (empty list: clean).

    `state`: host copies of (rec, radii, rect, tiles, pairs, pair_idx, final_T, n_contrib) as `_forward_impl` returns
    them.  `bin_cap` > 0: direct bins (tile t's list at t * bin_cap, rect and depth as the projection kernel parked them:
    pair_off word 0 and the record's depth), else the classic chain (packed lists at tile_start, rect / zkey arrays).
    `capacity`: entries of `pairs` (classic) or gradient records (direct bins).  `views(rect, tiles, pair_idx, RT, RG, RB)`
    names the fields of the shared buffers.  `shards`: spf_raster_pair_shards(S, G).  `launch_order`: audit the launch
    order array (None: whenever the library keeps one, `order_expected`)."""
    rec, radii, rect_t, tiles_t, pairs_t, pair_idx_t, final_T, n_contrib = state
    R = S * V
    tiles_x, tiles_y = grid(H, W)
    T = tiles_x * tiles_y
    RT, RG, nblk = R * T, R * G, (G + BLOCK - 1) // BLOCK
    v = views(rect_t, tiles_t, pair_idx_t, RT, RG, R * nblk)
    rep = _Report()
    direct = bin_cap > 0
    rec = _np(rec).reshape(RG, REC)
    radii = _np(radii).reshape(RG).astype(np.int64)
    pair_off = _np(v.pair_off, np.uint32).reshape(RG, 2)
    rect = pair_off[:, 0] if direct else _np(v.rect, np.uint32)[:RG]
    depth_bits = np.ascontiguousarray(rec[:, REC_DEPTH]).view(np.uint32)
    zbits = depth_bits if direct else _np(v.zkey, np.uint32)[:RG]
    count = _np(v.tile_count, np.uint32)[:RT].astype(np.int64)
    start = _np(v.tile_start, np.uint32)[:RT + 1].astype(np.int64)
    counters = _np(v.counters, np.uint32).astype(np.int64)
    pairs = _np(pairs_t, np.uint64).reshape(-1) if pairs_t is not None else np.zeros(0, np.uint64)
    where_g = lambda i: f"render {i // G} gaussian {i % G}"
    where_t = lambda i: f"render {i // T} tile {i % T} (tx {i % T % tiles_x}, ty {i % T // tiles_x})"

    # ---- rect and radii -------------------------------------------------------------------------------------------
    x0, y0, x1, y1, empty = unpack_rect(rect)
    rep.add_each("rect_grid", np.nonzero(~empty & ((x1 > tiles_x) | (y1 > tiles_y)))[0],
                 lambda i: f"{where_g(i)}: rect ({x0[i]}, {y0[i]}, {x1[i]}, {y1[i]}) leaves the {tiles_x} x {tiles_y} grid")
    rep.add_each("radii_rect", np.nonzero((radii == 0) & ~empty)[0],
                 lambda i: f"{where_g(i)}: radii 0 with rect ({x0[i]}, {y0[i]}, {x1[i]}, {y1[i]})")
    # (radii reports the 3-sigma rect, the packed rect is that rect SHRUNK to the tiles holding a pixel centre inside the
    #  cull disc (project.hip): a visible Gaussian may keep no tile only if its disc can miss every pixel centre -- its
    #  centre outside the image, or cull r^2 < 1/2, the farthest a point is from the pixel lattice)
    cx, cy, cr2 = rec[:, REC_X], rec[:, REC_Y], rec[:, REC_CULL_R2]
    reaches = (cr2 >= 0.5) & (cx >= 0) & (cx <= W - 1) & (cy >= 0) & (cy <= H - 1)
    rep.add_each("radii_rect", np.nonzero((radii > 0) & empty & reaches)[0],
                 lambda i: f"{where_g(i)}: radii {radii[i]} but an empty rect (centre {cx[i]:.2f}, {cy[i]:.2f}, cull r^2 {cr2[i]:.3g})")
    if not direct:
        rep.add_each("depth", np.nonzero((radii > 0) & (zbits != depth_bits))[0],
                     lambda i: f"{where_g(i)}: zkey bits {zbits[i]:#x} != record depth bits {depth_bits[i]:#x}")
        rep.add_each("pair_off_rect", np.nonzero(pair_off[:, 0] != rect)[0],
                     lambda i: f"{where_g(i)}: pair_off word 0 {pair_off[i, 0]:#x} != rect {rect[i]:#x}")
    if rep.seen.get("rect_grid"):
        return rep.out                      # (tile indices below would be out of range)

    # ---- counts and lists, render by render -------------------------------------------------------------------------
    areas = np.zeros(RG, np.int64)
    for r in range(R):
        sl = slice(r * G, (r + 1) * G)
        g_of, t_of, area = expand_pairs(x0[sl], y0[sl], x1[sl], y1[sl], empty[sl], tiles_x)
        areas[sl] = area
        key = make_keys(zbits[sl][g_of], g_of)
        order = np.lexsort((key, t_of))
        want_keys, want_tile = key[order], t_of[order]
        want_count = np.bincount(t_of, minlength=T).astype(np.int64)
        got_count = count[r * T:(r + 1) * T]
        rep.add_each("count", r * T + np.nonzero(got_count != want_count)[0],
                     lambda i: f"{where_t(i)}: tile_count {count[i]} != {want_count[i % T]} Gaussians whose rect covers it")
        base = (np.arange(r * T, (r + 1) * T, dtype=np.int64) * bin_cap) if direct else start[r * T:(r + 1) * T]
        pos = np.arange(want_keys.size, dtype=np.int64) - (np.cumsum(want_count) - want_count)[want_tile]
        idx = base[want_tile] + pos
        # (an entry the device's own count does not cover is missing -- reported once, as the count; out of the buffer:
        #  cannot be read)
        covered = pos < np.minimum(got_count, bin_cap if direct else np.iinfo(np.int64).max)[want_tile]
        inside = (idx >= 0) & (idx < pairs.size)
        rep.add_each("list_bounds", np.nonzero(covered & ~inside)[0],
                     lambda j: f"{where_t(r * T + int(want_tile[j]))} pos {pos[j]}: entry {idx[j]} outside pairs[{pairs.size}]")
        look = covered & inside
        got = np.zeros_like(want_keys)
        got[look] = pairs[idx[look]]
        rep.add_each("list", np.nonzero(look & (got != want_keys))[0],
                     lambda j: f"{where_t(r * T + int(want_tile[j]))} pos {pos[j]}: key {int(got[j]):#018x} != {int(want_keys[j]):#018x}"
                               f" (depth bits, id: {int(got[j]) >> 32:#x}, {int(got[j]) & 0xFFFFFFFF} != "
                               f"{int(want_keys[j]) >> 32:#x}, {int(want_keys[j]) & 0xFFFFFFFF})")

    # ---- scan, pair numbering ---------------------------------------------------------------------------------------
    if not direct:
        scan = np.concatenate([[0], np.cumsum(count)])
        rep.add_each("scan", np.nonzero(start[:RT] != scan[:RT])[0],
                     lambda i: f"{where_t(i)}: tile_start {start[i]} != exclusive scan {scan[i]}")
        D = int(scan[RT])
        if not (start[RT] == D == counters[0]):
            rep.add("scan", f"tile_start[R*T] {start[RT]}, counters[0] {counters[0]}, sum of the counts {D}: not one number")
        if counters[1] != (count.max() if RT else 0):
            rep.add("scan", f"counters[1] {counters[1]} != longest list {count.max()}")
        if D > capacity or D > pairs.size:
            rep.add("scan", f"D {D} exceeds capacity {capacity} / pairs[{pairs.size}]")
        first = np.cumsum(areas) - areas
        rep.add_each("pair_off", np.nonzero(pair_off[:, 1].astype(np.int64) != first)[0],
                     lambda i: f"{where_g(i)}: first pair {pair_off[i, 1]} != exclusive scan of the rect areas {first[i]}")
        blk_total = _np(v.blk_total, np.uint32)[:R * nblk].astype(np.int64)
        blk_base = _np(v.blk_base, np.uint32)[:R * nblk].astype(np.int64)
        pad = np.zeros((R, nblk * BLOCK), np.int64)
        pad[:, :G] = areas.reshape(R, G)
        want_total = pad.reshape(R * nblk, BLOCK).sum(axis=1)
        rep.add_each("blk", np.nonzero(blk_total != want_total)[0],
                     lambda i: f"render {i // nblk} block {i % nblk}: blk_total {blk_total[i]} != {want_total[i]}")
        want_base = np.cumsum(want_total) - want_total
        rep.add_each("blk", np.nonzero(blk_base != want_base)[0],
                     lambda i: f"render {i // nblk} block {i % nblk}: blk_base {blk_base[i]} != {want_base[i]}")
    else:
        off = pair_off[:, 1].astype(np.int64)
        live = np.nonzero(areas > 0)[0]
        share = capacity // shards
        srt = live[np.argsort(off[live], kind="stable")]
        end = off[srt] + areas[srt]
        for j in np.nonzero(end[:-1] > off[srt][1:])[0][:MAX_REPORT + 1]:
            a, b = int(srt[j]), int(srt[j + 1])
            rep.add("pair_ranges", f"{where_g(a)} [{off[a]}, {end[j]}) overlaps {where_g(b)} [{off[b]}, {off[b] + areas[b]})")
        sh_lo, sh_hi = off[live] // max(share, 1), (off[live] + areas[live] - 1) // max(share, 1)
        # block (x = g / 256, y = scene) of the projection kernel numbers its pairs from cursor (x + y * nblk) % shards
        scene = live // G // V
        want_sh = (live % G // BLOCK + scene * nblk) % shards
        bad = (sh_lo != sh_hi) | (sh_hi >= shards) | (sh_lo != want_sh)
        rep.add_each("pair_shard", live[bad],
                     lambda i: f"{where_g(i)}: records [{off[i]}, {off[i] + areas[i]}) are not inside shard "
                               f"{(i % G // BLOCK + i // G // V * nblk) % shards}'s share of {share} ({shards} shard(s) of {capacity})")
        if v.pair_cursor is not None:
            cursor = _np(v.pair_cursor, np.uint32).astype(np.int64)
            used = np.bincount(want_sh, weights=areas[live], minlength=shards).astype(np.int64)
            for s in np.nonzero(cursor[:shards] != used[:shards])[0]:
                rep.add("pair_cursor", f"shard {s}: cursor {cursor[s]} != {used[s]} pairs of its blocks")

    # ---- launch order (direct bins, many tiles) ---------------------------------------------------------------------
    if launch_order is None:
        launch_order = direct and order_expected(RT, bin_cap)
    if launch_order:
        words = _np(tiles_t, np.uint32).reshape(-1)
        order = words[2 * RT:4 * RT].reshape(RT, 2).astype(np.int64)
        ids = order[:, 0] & ORDER_TILE_MASK
        hits = np.bincount(np.minimum(ids, RT), minlength=RT + 1)
        rep.add_each("order", np.nonzero(ids >= RT)[0], lambda j: f"slot {j}: tile id {ids[j]} >= {RT}")
        rep.add_each("order", np.nonzero(hits[:RT] != 1)[0], lambda i: f"{where_t(i)}: {hits[i]} slots of the launch order")
        ok = ids < RT
        want_n = np.minimum(count[np.minimum(ids, RT - 1)], bin_cap)
        rep.add_each("order", np.nonzero(ok & (order[:, 1] != want_n))[0],
                     lambda j: f"slot {j} ({where_t(int(ids[j]))}): length {order[j, 1]} != min(count, bin_cap) {want_n[j]}")

    # ---- pixels -----------------------------------------------------------------------------------------------------
    nc = _np(n_contrib, np.uint32).reshape(R, H, W).astype(np.int64)
    ty, tx = np.arange(H) // TILE, np.arange(W) // TILE
    per_pixel = count.reshape(R, tiles_y, tiles_x)[:, ty][:, :, tx]
    if direct:
        per_pixel = np.minimum(per_pixel, bin_cap)
    for r, y, x in np.argwhere(nc > per_pixel)[:MAX_REPORT + 1]:
        t = int(r) * T + int(y) // TILE * tiles_x + int(x) // TILE
        rep.add("pixels", f"{where_t(t)} pixel ({x}, {y}): n_contrib {nc[r, y, x]} > list length {per_pixel[r, y, x]}")
    return rep.out


# ---------------------------------------------------------------------------------------------------------------------
# The boundary scene
# ---------------------------------------------------------------------------------------------------------------------
def boundary_lengths(cap: int) -> list:
    """List lengths of the case `cap`: the fixed small ones, b - 1, b, b + 1 for every sort-class border b <= cap, and for
    the top case two chunks (the second full / holding one entry), three chunks plus one, and four chunks plus one."""
    L = list(BASE_LENGTHS)
    for b in SORT_BORDERS:
        if b <= cap:
            L += [b - 1, b, b + 1]
    if cap >= TOP_CAP:
        L += list(TOP_LENGTHS)
    return L


def _pattern_z(name: str, n: int, gen: np.random.Generator) -> np.ndarray:
    """float32 depths of one tile's Gaussians in id order."""
    if name == "random":
        return gen.uniform(1.0, 100.0, n).astype(np.float32)
    if name == "equal":
        return np.full(n, 2.5, np.float32)                                 # pure id order
    if name == "descending":
        return np.linspace(100.0, 1.0, n).astype(np.float32)               # reverse-sorted input
    if name == "ulp_steps":
        return (np.float32(1.5).view(np.uint32) + np.arange(n, dtype=np.uint32)).view(np.float32)
    if name == "wide":
        return (0.25 * 4.0e4 ** gen.uniform(0.0, 1.0, n)).astype(np.float32)   # 0.25 .. 1e4
    raise ValueError(name)


def boundary_scene(cap: int, interleaved: bool, hw=None, rotate: int = 0, seed: int = 0, lengths=None,
                   patterns=KEY_PATTERNS) -> dict:
    """One render whose tile i holds exactly L[i] Gaussians (`boundary_lengths(cap)`, or `lengths`), every one projecting
    to the centre pixel (16 tx + 7.5, 16 ty + 7.5) of its tile: identity view matrix, focal length 32 px, scales 1e-3 (a
    3 px radius whatever the depth), colours given.  `hw`: the image (default: the smallest near-square grid that holds
    the lengths); its further tiles alternate between empty and one Gaussian.  Key pattern of tile i:
    patterns[(i + rotate) % len(patterns)].  Ids: contiguous per tile, or `interleaved` round-robin over the tiles.
    Returns the inputs (float32 torch tensors shaped for one scene and one view) and what must come out:
    `lengths` [T], `tile_of` [G], `z` [G]."""
    L = list(boundary_lengths(cap) if lengths is None else lengths)
    if hw is None:
        gx = int(np.ceil(np.sqrt(len(L))))
        gy = (len(L) + gx - 1) // gx
        H, W = TILE * gy, TILE * gx
    else:
        H, W = hw
    tiles_x, tiles_y = grid(H, W)
    T = tiles_x * tiles_y
    assert T >= len(L), (T, len(L))
    L = np.asarray(L + [(i - len(L)) % 2 for i in range(len(L), T)], np.int64)
    gen = np.random.default_rng(seed)
    tile = np.repeat(np.arange(T, dtype=np.int64), L)
    first = np.cumsum(L) - L
    k = np.arange(tile.size, dtype=np.int64) - first[tile]                   # rank of the Gaussian inside its tile, by id
    z = np.concatenate([_pattern_z(patterns[(i + rotate) % len(patterns)], int(n), gen) for i, n in enumerate(L)]
                       + [np.zeros(0, np.float32)])
    if interleaved:
        order = np.lexsort((tile, k))                                        # ids go round the tiles: rank-major
        tile, z = tile[order], z[order]
    G = tile.size
    tanx, tany = W / 64.0, H / 64.0                                          # focal length W / (2 tan) = 32 px
    px, py = TILE * (tile % tiles_x) + 7.5, TILE * (tile // tiles_x) + 7.5
    z64 = z.astype(np.float64)
    means = np.stack([((2 * px + 1) / W - 1) * tanx * z64, ((2 * py + 1) / H - 1) * tany * z64, z64], axis=1)
    near, far = 0.1, 1.0e5
    P = np.zeros((4, 4))
    P[0, 0], P[1, 1], P[3, 2] = 1 / tanx, 1 / tany, 1.0
    P[2, 2], P[2, 3] = far / (far - near), -(far * near) / (far - near)
    f = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    rot = np.zeros((G, 4), np.float32)
    rot[:, 0] = 1.0
    return dict(
        H=H, W=W, G=G, lengths=L, tile_of=tile, z=z,
        means=f(means)[None], scales=torch.full((1, G, 3), 1e-3), rotations=f(rot)[None],
        opacities=torch.full((1, G), 0.5), colors=f(gen.uniform(0.0, 1.0, (G, 3)))[None],
        viewmatrix=torch.eye(4)[None, None].contiguous(), projmatrix=f(P.T)[None, None], tanfov=f([[[tanx, tany]]]),
        bg=torch.zeros(1, 1, 3))


def boundary_expected(scene: dict):
    """(counts [T], every tile's sorted list back to back) of a boundary scene, from its inputs alone."""
    tile, z = scene["tile_of"], scene["z"]
    key = make_keys(f32_bits(z), np.arange(tile.size))
    order = np.lexsort((key, tile))
    return scene["lengths"].copy(), key[order]


def device_lists(state, views, S, V, G, H, W, bin_cap):
    """(counts [R*T], the device's lists back to back in tile order) -- for exact comparison with `boundary_expected`."""
    rec, radii, rect_t, tiles_t, pairs_t, pair_idx_t, _, _ = state
    R, (tiles_x, tiles_y) = S * V, grid(H, W)
    RT = R * tiles_x * tiles_y
    v = views(rect_t, tiles_t, pair_idx_t, RT, R * G, R * ((G + BLOCK - 1) // BLOCK))
    count = _np(v.tile_count, np.uint32)[:RT].astype(np.int64)
    pairs = _np(pairs_t, np.uint64).reshape(-1)
    base = np.arange(RT, dtype=np.int64) * bin_cap if bin_cap else _np(v.tile_start, np.uint32)[:RT].astype(np.int64)
    n = np.minimum(count, bin_cap) if bin_cap else count
    t = np.repeat(np.arange(RT, dtype=np.int64), n)
    idx = base[t] + np.arange(t.size, dtype=np.int64) - (np.cumsum(n) - n)[t]
    return count, pairs[idx]


# ---------------------------------------------------------------------------------------------------------------------
# A state in the device layout from the CPU oracle's projection
# ---------------------------------------------------------------------------------------------------------------------
def state_from_oracle(projected: list, S: int, V: int, H: int, W: int, bin_cap: int = 0, capacity: int | None = None,
                      shards: int = 1, slack: int = 0, seed: int = 0):
    """What a correct forward call leaves for the renders `projected` (oracle.splat_ref.Projected, scene-major): the eight
    state tensors in the device layout of include/spfsplat_hip.h (written here field by field from that description, not
    through the product's slicing), and the capacity they were built for.  What the contract leaves open holds garbage:
    the slots of a bin past its list's end, the pair buffer past D, and (direct bins) the rect / zkey arrays."""
    from oracle import splat_ref
    R, G = S * V, projected[0].radii.numel()
    tiles_x, tiles_y = grid(H, W)
    T = tiles_x * tiles_y
    RT, RG, nblk = R * T, R * G, (G + BLOCK - 1) // BLOCK
    gen = np.random.default_rng(seed)
    rec = np.zeros((RG, REC), np.float32)
    rect = np.zeros(RG, np.uint32)
    radii = np.zeros(RG, np.int32)
    zbits = np.zeros(RG, np.uint32)
    counts, lists, areas = [], [], np.zeros(RG, np.int64)
    for r, pr in enumerate(projected):
        sl = slice(r * G, (r + 1) * G)
        vis = (pr.radii > 0).numpy()
        rmin, rmax = pr.rect_min.numpy(), pr.rect_max.numpy()
        rect[sl] = np.where(vis, pack_rect(rmin[:, 0], rmin[:, 1], rmax[:, 0], rmax[:, 1]), 0)
        radii[sl] = pr.radii.numpy()
        z32 = pr.depth.detach().to(torch.float32).numpy()
        zbits[sl] = np.where(vis, f32_bits(z32), 0)
        rec[sl, REC_X], rec[sl, REC_Y] = pr.xy[:, 0].detach().float().numpy(), pr.xy[:, 1].detach().float().numpy()
        rec[sl, REC_DEPTH] = np.where(vis, z32, 0)
        rec[sl, REC_CULL_R2] = 1.0e4
        c, keys = expected_lists(rect[sl], zbits[sl], H, W)
        # the oracle's own lists (ids in front-to-back order) must be what the keys sort to
        ids = np.concatenate([i.numpy() for _, _, i in splat_ref.tile_lists(pr, H, W)] + [np.zeros(0, np.int64)])
        assert np.array_equal(keys & np.uint64(0xFFFFFFFF), ids.astype(np.uint64)), "oracle tile_lists vs key order"
        counts.append(c)
        lists.append(keys)
        x0, y0, x1, y1, empty = unpack_rect(rect[sl])
        areas[sl] = np.where(empty, 0, (x1 - x0) * (y1 - y0))
    count = np.concatenate(counts)
    D = int(count.sum())
    tiles = np.zeros(4 * RT + 16, np.uint32)
    tiles[:RT] = count
    pair_idx = np.zeros(2 * RG + 2 * R * nblk, np.uint32)
    pair_idx[0:2 * RG:2] = rect
    pad = np.zeros((R, nblk * BLOCK), np.int64)
    pad[:, :G] = areas.reshape(R, G)
    blk_total = pad.reshape(R * nblk, BLOCK).sum(axis=1)
    if bin_cap:
        assert count.max() <= bin_cap
        capacity = (D + slack) * shards if capacity is None else capacity
        share = capacity // shards
        pairs = gen.integers(0, 2 ** 63, RT * bin_cap, dtype=np.int64).view(np.uint64)
        n_before = np.cumsum(count) - count
        t = np.repeat(np.arange(RT, dtype=np.int64), count)
        pairs[t * bin_cap + np.arange(D, dtype=np.int64) - n_before[t]] = np.concatenate(lists)
        # pair numbering: block (x, scene) takes its pairs of every view from cursor (x + scene * nblk) % shards
        cursor = np.zeros(8, np.int64)
        first = np.zeros(RG, np.int64)
        for s in range(S):
            for b in range(nblk):
                sh = (b + s * nblk) % shards
                for vv in range(V):
                    r = s * V + vv
                    sl = slice(r * G + b * BLOCK, r * G + min(G, (b + 1) * BLOCK))
                    a = areas[sl]
                    first[sl] = sh * share + cursor[sh] + np.cumsum(a) - a
                    cursor[sh] += a.sum()
        assert cursor.max() <= share
        pair_idx[1:2 * RG:2] = first
        tiles[4 * RT + 5:4 * RT + 13] = cursor
        if order_expected(RT, bin_cap):
            ids = np.arange(RT, dtype=np.int64)
            tiles[2 * RT:4 * RT] = np.stack([ids, np.minimum(count, bin_cap)], axis=1).reshape(-1)
        rect_buf_rect, rect_buf_z = gen.integers(0, 2 ** 32, RG, dtype=np.uint32), gen.integers(0, 2 ** 32, RG, dtype=np.uint32)
    else:
        capacity = D + slack if capacity is None else capacity
        pairs = gen.integers(0, 2 ** 63, max(capacity, 1), dtype=np.int64).view(np.uint64)
        pairs[:D] = np.concatenate(lists)
        tiles[2 * RT:3 * RT + 1] = np.concatenate([[0], np.cumsum(count)])
        tiles[3 * RT + 1:4 * RT + 1] = count                                  # (the binning cursors ended at the counts)
        tiles[4 * RT + 1:4 * RT + 5] = (D, count.max(), 0, 0)
        pair_idx[1:2 * RG:2] = np.cumsum(areas) - areas
        pair_idx[2 * RG:2 * RG + R * nblk] = blk_total
        pair_idx[2 * RG + R * nblk:] = np.cumsum(blk_total) - blk_total
        rect_buf_rect, rect_buf_z = rect, zbits
    rect_buf = np.concatenate([rect_buf_rect, rect_buf_z, np.zeros((RG + 3) // 4, np.uint32)])
    n_contrib = np.repeat(np.repeat(count.reshape(R, tiles_y, tiles_x), TILE, axis=1), TILE, axis=2)[:, :H, :W]
    if bin_cap:
        n_contrib = np.minimum(n_contrib, bin_cap)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy())
    state = (torch.from_numpy(rec.reshape(-1, REC).copy()), torch.from_numpy(radii.copy()), i32(rect_buf), i32(tiles),
             torch.from_numpy(pairs.view(np.int64).copy()), i32(pair_idx), torch.ones(R * H * W),
             i32(np.ascontiguousarray(n_contrib.reshape(-1).astype(np.uint32))))
    return state, int(capacity)


def project_boundary(scene: dict, dtype):
    """The oracle's projection of a boundary scene."""
    from oracle import splat_ref
    c = lambda t: t.to(dtype)
    return splat_ref.project(c(scene["means"][0]), c(scene["scales"][0]), c(scene["rotations"][0]), c(scene["opacities"][0]),
                             None, c(scene["colors"][0]), c(scene["viewmatrix"][0, 0]), c(scene["projmatrix"][0, 0]),
                             float(scene["tanfov"][0, 0, 0]), float(scene["tanfov"][0, 0, 1]), scene["H"], scene["W"], 0)


# ---------------------------------------------------------------------------------------------------------------------
# Random scenes: what the product is given, what the oracle makes of it
# ---------------------------------------------------------------------------------------------------------------------
FRAGILE_SHARE = 0.005        # Gaussians whose rect a rounding knife-edge decides: the share `compare` allows for pixels


def flat_renders(batch) -> list:
    """The rasterizer arguments of every (scene, view) of a synthetic batch, scene-major, world scale as is."""
    from oracle import glue_ref
    b, v = batch.extrinsics.shape[:2]
    rep = lambda t: t[:, None].expand(b, v, *t.shape[1:]).reshape(b * v, *t.shape[1:])
    return glue_ref.callsite_args(batch.extrinsics.reshape(b * v, 4, 4), batch.intrinsics.reshape(b * v, 3, 3),
                                  batch.near.reshape(-1), batch.far.reshape(-1), batch.image_shape,
                                  torch.zeros(b * v, 3), rep(batch.means), rep(batch.harmonics), rep(batch.opacities),
                                  rep(batch.rotations), rep(batch.scales), scale_invariant=False)


def project_renders(args: list, dtype) -> list:
    from oracle import splat_ref
    c = lambda t: t.to(dtype)
    return [splat_ref.project(c(a["means3D"]), c(a["scales"]), c(a["rotations"]), c(a["opacities"]), c(a["shs"]), None,
                              c(a["viewmatrix"]), c(a["projmatrix"]), a["tanfovx"], a["tanfovy"], a["image_height"],
                              a["image_width"], a["sh_degree"]) for a in args]


def oracle_rect(pr) -> np.ndarray:
    """The oracle's 3-sigma tile rect of every Gaussian of one render, packed like the device's."""
    lo, hi = pr.rect_min.numpy(), pr.rect_max.numpy()
    return pack_rect(lo[:, 0], lo[:, 1], hi[:, 0], hi[:, 1])


def splat_pairs(pr) -> int:
    """(Gaussian, tile) pairs of the oracle's rects of one render: an upper bound of the device's (its rects are shrunk)."""
    a = (pr.rect_max - pr.rect_min).numpy()
    return int((a[:, 0] * a[:, 1]).sum())


def rects_against_oracle(projected64: list, rect: np.ndarray, radii: np.ndarray, H: int, W: int):
    """The device's packed rects and radii of the renders `projected64` (the oracle in float64) -> (violations, share of
    the Gaussians left out because `radii_fragile` flags them).  Everywhere else: the radii are the oracle's; the rect
    lies inside the oracle's 3-sigma rect; and a tile of that rect the device dropped (it keeps only the tiles with a
    pixel centre inside the cull disc, conservatively) holds no pixel the Gaussian contributes to -- none with
    power <= 0 and alpha >= 1/255 in float64 (the device's disc carries 0.1 % slack, four orders above float32 rounding)."""
    from oracle import splat_ref
    rep = _Report()
    tiles_x, _ = grid(H, W)
    G = projected64[0].radii.numel()
    left_out = 0
    for r, pr in enumerate(projected64):
        frag = splat_ref.radii_fragile(pr, H, W).numpy()
        left_out += int(frag.sum())
        sl = slice(r * G, (r + 1) * G)
        x0, y0, x1, y1, empty = unpack_rect(rect[sl])
        want_r = pr.radii.numpy().astype(np.int64)
        rep.add_each("radii", np.nonzero(~frag & (radii[sl] != want_r))[0],
                     lambda i: f"render {r} gaussian {i}: radii {radii[sl][i]} != oracle {want_r[i]}")
        o0, o1 = pr.rect_min.numpy(), pr.rect_max.numpy()
        o_empty = want_r == 0
        outside = ~frag & ~empty & (o_empty | (x0 < o0[:, 0]) | (y0 < o0[:, 1]) | (x1 > o1[:, 0]) | (y1 > o1[:, 1]))
        rep.add_each("rect", np.nonzero(outside)[0],
                     lambda i: f"render {r} gaussian {i}: rect ({x0[i]}, {y0[i]}, {x1[i]}, {y1[i]}) leaves the oracle's "
                               f"({o0[i, 0]}, {o0[i, 1]}, {o1[i, 0]}, {o1[i, 1]})")
        g_of, t_of, _ = expand_pairs(o0[:, 0], o0[:, 1], o1[:, 0], o1[:, 1], o_empty | frag | outside, tiles_x)
        tx, ty = t_of % tiles_x, t_of // tiles_x
        dropped = empty[g_of] | (tx < x0[g_of]) | (tx >= x1[g_of]) | (ty < y0[g_of]) | (ty >= y1[g_of])
        g_of, tx, ty = g_of[dropped], tx[dropped], ty[dropped]
        xy, con, op = pr.xy.detach().numpy(), pr.conic.detach().numpy(), pr.opacity.detach().numpy()
        for c0 in range(0, g_of.size, 1 << 14):
            g, px0, py0 = g_of[c0:c0 + (1 << 14)], tx[c0:c0 + (1 << 14)] * TILE, ty[c0:c0 + (1 << 14)] * TILE
            px = px0[:, None, None] + np.arange(TILE)[None, None, :]
            py = py0[:, None, None] + np.arange(TILE)[None, :, None]
            dx, dy = xy[g, 0][:, None, None] - px, xy[g, 1][:, None, None] - py
            power = -0.5 * (con[g, 0][:, None, None] * dx * dx + con[g, 2][:, None, None] * dy * dy) \
                - con[g, 1][:, None, None] * dx * dy
            alpha = np.minimum(0.99, op[g][:, None, None] * np.exp(np.minimum(power, 0.0)))
            hit = (power <= 0) & (alpha >= 1.0 / 255.0) & (px < W) & (py < H)
            for j in np.nonzero(hit.any(axis=(1, 2)))[0][:MAX_REPORT + 1]:
                rep.add("rect_dropped", f"render {r} gaussian {g[j]}: tile ({tx[c0 + j]}, {ty[c0 + j]}) of its 3-sigma rect is "
                                        f"not in rect ({x0[g[j]]}, {y0[g[j]]}, {x1[g[j]]}, {y1[g[j]]}) but holds a pixel with "
                                        f"alpha {alpha[j][hit[j]].max():.6f}")
    return rep.out, left_out / max(len(projected64) * G, 1)


# ---------------------------------------------------------------------------------------------------------------------
# The parametrisation of the sort-class tests and its plan coverage (shared by the CPU and the GPU file)
# ---------------------------------------------------------------------------------------------------------------------
SORT_ENV = ("SPF_SORT_BLOCKS", "SPF_SORT_BIG_MIXED", "SPF_SORT_SEPARATE", "SPF_SORT_LDS_2K", "SPF_SORT_SINGLE")


def sort_cases():
    """(cap, env, interleaved) of every sort-class case: both families at every cap with both id variants, and each switch
    alone at the caps where it changes the plan (test_abi.py pins which those are)."""
    cases = []
    for cap in CAPS:
        for blocks in ("0", "1"):
            for interleaved in (False, True):
                cases.append((cap, {"SPF_SORT_BLOCKS": blocks}, interleaved))
    for cap in (1024, 2048):        # BLOCK4 / BLOCK8 as launches of their own (few-tiles family)
        cases.append((cap, {"SPF_SORT_SEPARATE": "1"}, cap == 2048))
    for cap in (512, 1024):         # one wave per list instead of a pair (many-tiles family)
        cases.append((cap, {"SPF_SORT_BLOCKS": "0", "SPF_SORT_SINGLE": "1"}, cap == 512))
    for cap in (4096, 8192):        # the LDS network from 2,049 entries on
        cases.append((cap, {"SPF_SORT_LDS_2K": "1"}, cap == 4096))
    for cap in (2048, 4096):        # BLOCK16 as a launch of its own (few-tiles family)
        cases.append((cap, {"SPF_SORT_BIG_MIXED": "0"}, cap == 2048))
    return cases


def case_id(case) -> str:
    cap, env, interleaved = case
    sw = "-".join(f"{k[len('SPF_SORT_'):].lower()}{v}" for k, v in env.items()) or "default"
    return f"cap{cap}-{sw}-{'interleaved' if interleaved else 'contiguous'}"


def sort_ids(header_text: str) -> dict:
    import re
    return {name: int(val) for name, val in re.findall(r"#define SPF_SORT_([A-Z0-9_]+) (\d+)\b", header_text)}


def sort_plan(lib, hint: int, tiles: int, with_order: bool = False) -> list:
    """[(kernel id, lo, hi)] the library launches for a longest-list hint on a call of `tiles` tiles, environment as is."""
    import ctypes as C
    n_max = 8
    kernel, lo, hi, order = (C.c_int32 * n_max)(), (C.c_uint32 * n_max)(), (C.c_uint32 * n_max)(), (C.c_int32 * n_max)()
    n = lib.spf_raster_sort_plan(int(hint), int(tiles), int(with_order), kernel, lo, hi, order)
    assert 0 <= n <= n_max
    return [(kernel[i], lo[i], hi[i]) for i in range(n)]


def kernels_sorting(plan: list, lengths) -> set:
    """Kernel ids of `plan` whose class (lo, hi] holds at least one of the list lengths."""
    L = np.asarray(lengths)
    return {k for k, lo, hi in plan if bool(((L > lo) & (L <= hi)).any())}
