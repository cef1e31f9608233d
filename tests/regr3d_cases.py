"""Named EXACT inputs for the distillation point loss (tests/test_regr3d_exact.py; truth: the exact side of
tests/regr3d_oracle.py).

Every ground-truth point lies on a coordinate axis -- the axis and the sign drawn per point, the other two coordinates
+0.0 or -0.0 -- so the float32 norm the kernels form is the planted value bit for bit (regr3d_oracle.is_exact) and a case
DICTATES the bit pattern ("key") of every norm of a row: ties, neighbouring patterns, a norm exactly on a threshold.
Predictions are the ground truth times a scale in [0.5, 2] per batch item plus noise of 5 % of the depth, confidences are
uniform in [1, 9) with planted values, as in regr3d_oracle.make_case.  Keys stay within [2^-4, 2^8] unless a case says
otherwise.  Seeded by the case's name; float32; small.

    patterns            33 x 47, 24 rows built key by key: for each of the 8 contiguous partitions of the four selected
                        ranks a row with that alias pattern after pass 0 (key >> 20) and a row with it after pass 1
                        (key >> 9) while all four share key >> 20; among them rows whose four ranks differ in the
                        9-bit last digit only; a row whose four keys are equal while the row is not constant; rows whose
                        floor / ceiling statistics are 0x...fffff | 0x...00000 (pass 0) and 0x...1ff | 0x...200
                        (pass 1), one ulp apart; three ordinary rows
    patterns_seg2       96 x 112 (two histogram segments per row): (0,1,1,3) after pass 0 in view 1, after pass 1 in view 2
    ties                rows of six values: each selected rank inside a run of equal norms, floor and ceiling in one run
                        (every point of the run lies exactly on the threshold) or in neighbouring runs
    constant_two_segments, constant_zero_two_segments
                        96 x 112, every norm of view 1 equal (2.5; or all ground truth (0, 0, 0)): 8,192 increments of one
                        block to one histogram bin; view 2 is an ordinary row
    dense_ulps          rows drawn from 512 consecutive float32 patterns; where the statistics at floor and ceiling are
                        neighbouring patterns the float32 lerp puts q_lo ON the floor statistic and q_hi ON the ceiling
                        one (claims: lo_on_floor, hi_on_ceil), which the masks by rank would drop
    conf_edge           confidences of exactly 3, nextafter(3, 0), NaN and +inf on points in the middle of the band
    clip_edge           dist_clip = 8 with norms of exactly 8, nextafter(8, 9) and nextafter(8, 0)
    nan_point           ONE NaN coordinate in one row.  The product's contract: the point is invalid, its
                        norm orders above +inf, so the row's thresholds are those of the NaN sorted last, and no other row
                        is touched.  The reference (torch.quantile) would return NaN thresholds for that row.
    nan_many            five NaN norms in one row (> 0.2 %): the ceiling of r_hi is a NaN, q_hi is NaN, the row has no
                        valid point and every gradient of the row is 0
    inf_point_15        one infinite norm among 15: it is the ceiling of r_hi with a weight >= 0.5, so q_hi = inf - inf =
                        NaN (torch.quantile's answer too) and the row has no valid point
    inf_point_1551      one infinite norm among 1,551, above both ranks: finite thresholds, the point invalid
    small_n_<n>         H W = 1, 2, 3, 1024, 1025, 8192, 8193 with B = 2
    long_grid_rows      B = 1025, H W = 15: 2,050 rows and slots on grids capped at 2,048 -- the histogram, mask, loss and
                        backward kernels each take a second trip of the slot loop, the pick kernels get 2,050 blocks
    long_grid_slots     B = 171, H W = 6,145: 7 slots per row, 2,394 slots; a looping block changes rows"""
from __future__ import annotations

import functools
import zlib

import numpy as np
import torch

from tests import regr3d_oracle as go

LO_KEY, HI_KEY = 0x3D800000, 0x43800000            # 2^-4, 2^8
KEY_1, KEY_20 = 0x3F800000, 0x41A00000
NAN_KEY, INF_KEY = 0x7FC00000, 0x7F800000
PARTITIONS = ((0, 0, 0, 0), (0, 0, 0, 3), (0, 0, 2, 2), (0, 0, 2, 3), (0, 1, 1, 1), (0, 1, 1, 3), (0, 1, 2, 2),
              (0, 1, 2, 3))
SMALL_N = {1: (1, 1), 2: (1, 2), 3: (3, 1), 1024: (32, 32), 1025: (25, 41), 8192: (64, 128), 8193: (3, 2731)}
SLOT_POINTS, MAX_GRID, SEGMENT_SLOTS = 1024, 2048, 8   # point_slots.h, regr3d.hip


def _rng(name: str) -> np.random.Generator:
    return np.random.default_rng(zlib.crc32(name.encode()))


def ordinary_keys(rng, B: int, n: int) -> np.ndarray:
    """[B, n] keys: depths in [1, 20], 1 % nearer (down to 2^-4) and 1 % farther (up to 2^8), uniform in the pattern."""
    k = rng.integers(KEY_1, KEY_20 + 1, (B, n))
    u = rng.random((B, n))
    k = np.where(u < 0.01, rng.integers(LO_KEY, KEY_1, (B, n)), k)
    return np.where(u > 0.99, rng.integers(KEY_20, HI_KEY + 1, (B, n)), k)


def _view(rng, keys: np.ndarray, H: int, W: int, conf_floor: float = 1.0):
    """(gt [B,H,W,3], pr, conf) for the keys [B, n] of one view."""
    B, n = keys.shape
    assert n == H * W
    val = keys.astype(np.uint32).view(np.float32)
    axis = rng.integers(0, 3, (B, n))
    sign = np.where(rng.random((B, n)) < 0.5, np.float32(-1.0), np.float32(1.0))
    gt = np.where(rng.random((B, n, 3)) < 0.5, np.float32(-0.0), np.float32(0.0))
    np.put_along_axis(gt, axis[..., None], (val * sign)[..., None], axis=2)
    depth = np.where(np.isfinite(val), val, np.float32(1.0)).astype(np.float64)    # the prediction stays finite
    dirn = np.zeros((B, n, 3))
    np.put_along_axis(dirn, axis[..., None], sign.astype(np.float64)[..., None], axis=2)
    scale = 0.5 + 1.5 * rng.random((B, 1, 1))
    pr = dirn * depth[..., None] * scale + 0.05 * np.maximum(depth, 2.0 ** -4)[..., None] * rng.standard_normal((B, n, 3))
    conf = conf_floor + (9.0 - conf_floor) * rng.random((B, n))
    t = lambda a, *s: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(B, H, W, *s))   # noqa: E731
    return t(gt, 3), t(pr, 3), t(conf)


def _case(name, rng, keys1, keys2, H, W, claims=None, conf_floor=1.0, **opts) -> dict:
    case = {"name": name, "claims": claims or {}}
    for v, keys in ((1, keys1), (2, keys2)):
        case[f"gt_pts{v}"], case[f"pr_pts{v}"], case[f"conf{v}"] = _view(rng, keys, H, W, conf_floor)
    case.update(dist_clip=None, disable_view1=False, norm_mode="avg_dis", gt_scale=False)
    case.update(opts)
    return case


def _plant(t: torch.Tensor, b: int, i: int, value: float):
    t[b].view(-1)[i] = value


def _index_of_rank(case: dict, v: int, b: int, rank: int) -> int:
    """The flat index of the point of row (v, b) whose norm has `rank` in the row's order (a stable sort)."""
    return int(np.argsort(go.keys32(go.norm32(case[f"gt_pts{v + 1}"][b]).reshape(-1)), kind="stable")[rank])


# ---- rows built key by key -----------------------------------------------------------------------------------------
def four_keys(rng, part, level: int) -> list:
    """K0 <= K1 <= K2 <= K3 whose alias pattern is `part` at `level` (0: key >> 20, and the same at key >> 9; 1:
    key >> 9 while all four share key >> 20).  Ranks of one group differ in the last digit only."""
    group = [sorted(set(part)).index(p) for p in part]
    if level == 0:
        base, step = int(rng.integers(0x3E0, 0x420)) << 20, int(rng.integers(1, 4)) << 20
    else:
        base = (int(rng.integers(0x3E0, 0x430)) << 20) + (int(rng.integers(0, 1024)) << 9)
        step = int(rng.integers(1, 200)) << 9
    low = int(rng.integers(1, 100))
    return [base + group[t] * step + t * low for t in range(4)]


def row_through(rng, n: int, K) -> np.ndarray:
    """A row of n keys, shuffled, whose order statistics at the four selected ranks are K0 .. K3."""
    (l0, l1, _), (h0, h1, _) = go.ranks32(n)
    assert l0 < l1 < h0 < h1 and LO_KEY <= K[0] <= K[1] <= K[2] <= K[3] <= HI_KEY
    s = np.empty(n, dtype=np.int64)
    s[:l0] = rng.integers(LO_KEY, K[0] + 1, l0)
    s[l1 + 1:h0] = rng.integers(K[1], K[2] + 1, h0 - l1 - 1)
    s[h1 + 1:] = rng.integers(K[3], HI_KEY + 1, n - h1 - 1)
    s[[l0, l1, h0, h1]] = K
    return rng.permutation(s)


def _patterns():
    rng, n = _rng("patterns"), 33 * 47
    rows, labels = [], []
    for level in (0, 1):
        for part in PARTITIONS:
            rows.append(row_through(rng, n, four_keys(rng, part, level)))
            labels.append(f"pass{level}:{part}")
    K = int(rng.integers(KEY_1, KEY_20))
    rows.append(row_through(rng, n, [K] * 4))
    labels.append("four_equal")
    for what in ("straddle0_lo", "straddle0_hi", "straddle1_lo", "straddle1_hi"):
        edge = int(rng.integers(0x3F8, 0x410)) << 20
        if what.startswith("straddle1"):
            edge += int(rng.integers(1, 2047)) << 9
        pair, far = [edge - 1, edge], int(rng.integers(2, 9)) << 20
        rows.append(row_through(rng, n, pair + [edge + far, edge + far + 12345] if what.endswith("lo") else
                                [edge - far - 12345, edge - far] + pair))
        labels.append(what)
    rows += list(ordinary_keys(rng, 3, n))
    labels += ["ordinary"] * 3
    B = len(rows) // 2
    keys = np.stack(rows)
    return _case("patterns", rng, keys[:B], keys[B:], 33, 47, {"labels": labels})


def _patterns_seg2():
    rng, n = _rng("patterns_seg2"), 96 * 112
    k1 = row_through(rng, n, four_keys(rng, (0, 1, 1, 3), 0))[None]
    k2 = row_through(rng, n, four_keys(rng, (0, 1, 1, 3), 1))[None]
    return _case("patterns_seg2", rng, k1, k2, 96, 112, {"labels": ["pass0:(0, 1, 1, 3)", "pass1:(0, 1, 1, 3)"]})


# run lengths of the six values at n = 1,551 (ranks 3 | 4 and 1,546 | 1,547), and where floor and ceiling fall
TIE_RUNS = (((10, 500, 500, 500, 31, 10), "same", "same"),
            ((4, 300, 600, 400, 243, 4), "split", "split"),
            ((4, 100, 100, 100, 1000, 247), "split", "same"),
            ((200, 300, 400, 400, 247, 4), "same", "split"),
            ((2, 2, 2, 1541, 2, 2), "split", "split"),
            ((775, 1, 1, 1, 1, 772), "same", "same"))


def _ties():
    rng, n = _rng("ties"), 33 * 47
    rows = []
    for runs, _, _ in TIE_RUNS:
        assert sum(runs) == n
        values = np.sort(rng.choice(np.arange(KEY_1, KEY_20), 6, replace=False))
        rows.append(rng.permutation(np.repeat(values, runs)))
    keys = np.stack(rows)
    return _case("ties", rng, keys[:3], keys[3:], 33, 47, {"runs": TIE_RUNS})


def _constant(name, key):
    rng, n = _rng(name), 96 * 112
    return _case(name, rng, np.full((1, n), key, dtype=np.int64), ordinary_keys(rng, 1, n), 96, 112, {"key": key})


def _dense_ulps():
    rng, n = _rng("dense_ulps"), 33 * 47

    def ends(base, step):
        s = rng.integers(base + 8 * step, base + 512 - 8 * step, n)
        s[:8] = base + step * np.arange(8)
        s[-8:] = base + 511 - step * np.arange(8)
        return rng.permutation(s)
    rows = [ends(0x40490000, 1), ends(KEY_1 - 256, 1),                # the second straddles 1.0: the ulp doubles inside
            rng.integers(0x41200000, 0x41200000 + 512, n), ends(0x40A00000, 8)]
    keys = np.stack(rows)
    # (view, b) of the rows whose statistics at the selected ranks are neighbouring patterns
    return _case("dense_ulps", rng, keys[:2], keys[2:], 33, 47, {"lo_on_floor": [(0, 0), (0, 1)],
                                                                  "hi_on_ceil": [(0, 0), (0, 1)]})


CONF_PLANTS = (3.0, float(np.nextafter(np.float32(3.0), np.float32(0.0))), float("nan"), float("inf"))


def _conf_edge():
    rng, n = _rng("conf_edge"), 33 * 47
    case = _case("conf_edge", rng, ordinary_keys(rng, 2, n), ordinary_keys(rng, 2, n), 33, 47)
    where = []
    for v in (0, 1):
        for b in (0, 1):
            for j, value in enumerate(CONF_PLANTS):
                i = _index_of_rank(case, v, b, 700 + j)
                _plant(case[f"conf{v + 1}"], b, i, value)
                where.append((v, b, i, value))
    case["claims"]["planted"] = where
    return case


CLIP = 8.0
CLIP_PLANTS = (0x41000000, 0x41000001, 0x40FFFFFF)      # 8, nextafter(8, 9), nextafter(8, 0)


def _clip_edge():
    rng, n = _rng("clip_edge"), 33 * 47
    keys = [ordinary_keys(rng, 2, n), ordinary_keys(rng, 2, n)]
    for k in keys:
        k[:, :3] = CLIP_PLANTS
    return _case("clip_edge", rng, keys[0], keys[1], 33, 47, {"planted": [0, 1, 2]}, dist_clip=CLIP)


def _special(name, n_hw, row, count, key, B=2, conf_floor=1.0):
    rng = _rng(name)
    H, W = n_hw
    keys = [ordinary_keys(rng, B, H * W), ordinary_keys(rng, B, H * W)]
    v, b = row
    at = sorted(int(i) for i in rng.choice(H * W, count, replace=False))
    keys[v][b, at] = key
    return _case(name, rng, keys[0], keys[1], H, W, {"row": row, "at": at}, conf_floor)


def _small_n(n):
    name = f"small_n_{n}"
    rng = _rng(name)
    H, W = SMALL_N[n]
    # (a row of one, two or three points: confidences from 3 up, so that the case has valid points at all)
    return _case(name, rng, ordinary_keys(rng, 2, n), ordinary_keys(rng, 2, n), H, W, conf_floor=3.0 if n <= 3 else 1.0)


def _long_grid(name, B, H, W):
    rng = _rng(name)
    return _case(name, rng, ordinary_keys(rng, B, H * W), ordinary_keys(rng, B, H * W), H, W)


BUILDERS = {
    "patterns": _patterns,
    "patterns_seg2": _patterns_seg2,
    "ties": _ties,
    "constant_two_segments": lambda: _constant("constant_two_segments", 0x40200000),
    "constant_zero_two_segments": lambda: _constant("constant_zero_two_segments", 0),
    "dense_ulps": _dense_ulps,
    "conf_edge": _conf_edge,
    "clip_edge": _clip_edge,
    "nan_point": lambda: _special("nan_point", (33, 47), (0, 1), 1, NAN_KEY),
    "nan_many": lambda: _special("nan_many", (33, 47), (1, 0), 5, NAN_KEY),
    "inf_point_15": lambda: _special("inf_point_15", (3, 5), (0, 0), 1, INF_KEY, conf_floor=2.0),
    "inf_point_1551": lambda: _special("inf_point_1551", (33, 47), (1, 1), 1, INF_KEY),
    **{f"small_n_{n}": functools.partial(_small_n, n) for n in SMALL_N},
    "long_grid_rows": lambda: _long_grid("long_grid_rows", 1025, 3, 5),
    "long_grid_slots": lambda: _long_grid("long_grid_slots", 171, 5, 1229),
}
NAMES = tuple(BUILDERS)
LONG = ("long_grid_rows", "long_grid_slots")


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """The named case; shared between tests, never modified."""
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def truth(name: str) -> dict:
    return go.exact_truth(case(name))


def rows(c: dict):
    """(view, b, keys [n], conf [n]) of every row of a case."""
    for v in (0, 1):
        gt = c[f"gt_pts{v + 1}"]
        k = go.keys32(go.norm32(gt).reshape(gt.shape[0], -1))
        for b in range(gt.shape[0]):
            yield v, b, k[b], c[f"conf{v + 1}"][b].reshape(-1).numpy()


def slot_counts(c: dict) -> dict:
    """Slots of the histogram passes, of the mask / loss / two-view backward passes, and rows (blocks of a pick)."""
    B, H, W, _ = c["gt_pts1"].shape
    nchunk = -(-H * W // SLOT_POINTS)
    return {"hist": 2 * B * -(-nchunk // SEGMENT_SLOTS), "point": 2 * B * nchunk, "rows": 2 * B, "nchunk": nchunk}
