"""Regr3D on EXACT inputs (tests/regr3d_cases.py): ground truth on the coordinate axes, so that the float32 norms the
kernels form are the planted bit patterns and ties, neighbouring patterns, points exactly on a threshold, NaN and inf
norms have ONE truth (the exact side of tests/regr3d_oracle.py) instead of being excluded by decided().

CPU: the float32 restatement of the thresholds equals torch.quantile bit for bit on every finite row of the cases; the
radix restatement of the select equals the sort; every case is what it says it is (all 8 alias patterns at both levels,
ties that straddle the ranks, thresholds that round onto a statistic, planted confidences and clip norms, grids past the
cap); every mutant of the restatement is caught by a named case, or shown to change nothing where that is the claim.

GPU, for every case through regr3d_loss(..., return_stats=True): stats["q"] BITWISE (NaN matching NaN), n_valid, exact
zeros at invalid points, a non-zero gradient wherever float64 has one, and loss / nf_pr / nf_gt / gradients against the
float64 oracle under the exact mask with the suite's tolerances (1e-5 relative; grad_tolerance with c = 8)."""
import math

import numpy as np
import pytest
import torch

from tests import regr3d_cases as rc
from tests import regr3d_oracle as go
from tests.test_regr3d_loss import C_PRODUCT, _check_grads, _hip, _rel

POWER = 4.0            # nf_per_view must move a norm factor by at least this many bounds of its gate (1e-5 relative)


def _quantile_rows(names=rc.NAMES):
    for name in names:
        c = rc.case(name)
        if c["dist_clip"] is None:
            yield from ((name, *r) for r in rc.rows(c))


def _same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and
                np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


# ---- CPU ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", rc.NAMES)
def test_every_input_is_exact(name):
    c = rc.case(name)
    for v in (1, 2):
        gt = c[f"gt_pts{v}"]
        assert gt.dtype == torch.float32 and go.is_exact(gt), (name, v)
        assert int((gt != 0).sum(-1).max()) <= 1                                   # on an axis
        assert bool(torch.isfinite(c[f"pr_pts{v}"]).all())
    gts = torch.cat([c["gt_pts1"].flatten(), c["gt_pts2"].flatten()])
    if name in ("patterns", "ties", "long_grid_slots"):
        assert bool((gts < 0).any()) and bool((gts > 0).any())
        assert bool(torch.signbit(gts[gts == 0]).any()) and not bool(torch.signbit(gts[gts == 0]).all())   # -0.0 and +0.0
    if not name.startswith(("nan", "inf", "constant_zero")):
        k = np.concatenate([r[2] for r in rc.rows(c)])
        assert rc.LO_KEY <= int(k.min()) and int(k.max()) <= rc.HI_KEY, name


def test_thresholds32_equal_torch_quantile_bitwise():
    """On every finite row of the cases, and bit for bit.  Rows with a NaN are the documented deviation (torch returns
    NaN there); an infinite norm is finite arithmetic for both."""
    q = torch.tensor([go.Q_LO, go.Q_HI], dtype=torch.float32)
    rows = 0
    for name in rc.NAMES:
        c = rc.case(name)
        for v in (1, 2):
            dis = go.norm32(c[f"gt_pts{v}"]).reshape(c[f"gt_pts{v}"].shape[0], -1)
            keep = ~np.isnan(dis).any(axis=1)
            want = torch.quantile(torch.from_numpy(dis[keep]), q, dim=1).T.numpy()
            assert _same_bits(go.thresholds32(dis[keep]), want), (name, v)
            rows += int(keep.sum())
    assert rows > 2400                            # (2,050 and 342 of them are the long grids')
    inf15 = rc.truth("inf_point_15")["q"][0, 0]
    assert np.isfinite(inf15[0]) and np.isnan(inf15[1])
    assert bool(np.isfinite(rc.truth("inf_point_1551")["q"]).all())


def test_radix_restatement_equals_the_sort():
    """radix_select32 walks the three passes with the kernel's own[] / alias bookkeeping; it must pick what a sort picks,
    on every row, NaN and inf rows included."""
    for name in rc.NAMES:
        c = rc.case(name)
        if c["dist_clip"] is None:
            assert _same_bits(go.exact_truth(c, radix=True)["q"], rc.truth(name)["q"]), name


def test_cases_are_what_they_claim():
    # all 8 patterns after pass 0 and after pass 1; the census of every row of every case
    census = [{}, {}]
    seen = {}
    for name, v, b, keys, _ in _quantile_rows():
        if np.any(keys > rc.INF_KEY):
            continue
        p = go.select_patterns(keys, len(keys))
        seen[(name, v, b)] = p
        if len(keys) >= 1000:                     # (below that the four ranks are not four different points)
            for level in (0, 1):
                census[level][p[level]] = census[level].get(p[level], 0) + 1
    print("pattern census after pass 0:", sorted(census[0].items()))
    print("pattern census after pass 1:", sorted(census[1].items()))
    c = rc.case("patterns")
    B = c["gt_pts1"].shape[0]
    by_label = {}
    for i, label in enumerate(c["claims"]["labels"]):
        by_label.setdefault(label, []).append(seen[("patterns", i // B, i % B)])
    for part in rc.PARTITIONS:
        (p0,), (p1,) = by_label[f"pass0:{part}"], by_label[f"pass1:{part}"]
        assert p0[0] == part and p0[1] == part, (part, p0)
        assert p1[0] == (0, 0, 0, 0) and p1[1] == part, (part, p1)
    assert set(census[0]) == set(rc.PARTITIONS) and set(census[1]) == set(rc.PARTITIONS)
    # four ranks that only the 9-bit last digit separates; four equal keys in a row that is not constant
    for label in ("pass0:(0, 0, 0, 0)", "pass1:(0, 0, 0, 0)"):
        (p,) = by_label[label]
        assert p[1] == (0, 0, 0, 0) and p[2] == (0, 1, 2, 3), (label, p)
    (p,) = by_label["four_equal"]
    assert p == ((0, 0, 0, 0),) * 3
    row = c["claims"]["labels"].index("four_equal")
    assert len(np.unique(next(k for v, b, k, _ in rc.rows(c) if (v, b) == (row // B, row % B)))) >= 3
    # neighbouring statistics one ulp apart across a digit boundary of pass 0 and of pass 1
    (l0, l1, _), (h0, h1, _) = go.ranks32(33 * 47)
    for label, (i, j), low_bits in (("straddle0_lo", (l0, l1), 20), ("straddle0_hi", (h0, h1), 20),
                                    ("straddle1_lo", (l0, l1), 9), ("straddle1_hi", (h0, h1), 9)):
        row = c["claims"]["labels"].index(label)
        s = np.sort(next(k for v, b, k, _ in rc.rows(c) if (v, b) == (row // B, row % B)).astype(np.int64))
        assert s[j] - s[i] == 1 and s[j] & ((1 << low_bits) - 1) == 0, label
        assert (s[i] >> 20 == s[j] >> 20) == (low_bits == 9), label
    # two histogram segments with (0,1,1,3)
    c = rc.case("patterns_seg2")
    assert rc.slot_counts(c)["nchunk"] > rc.SEGMENT_SLOTS
    assert seen[("patterns_seg2", 0, 0)][0] == (0, 1, 1, 3) and seen[("patterns_seg2", 1, 0)][:2] == ((0, 0, 0, 0), (0, 1, 1, 3))

    # ties: every selected rank inside a run of equal norms; floor / ceiling in one run or in two, as the case says;
    # where they share a run every point of it is ON the threshold, and some of those are valid
    c, t = rc.case("ties"), rc.truth("ties")
    for (v, b, keys, conf), (runs, lo_kind, hi_kind) in zip(rc.rows(c), c["claims"]["runs"]):
        s = np.sort(keys)
        assert len(np.unique(s)) == 6
        for k in (l0, l1, h0, h1):
            assert s[k] == s[k - 1] or s[k] == s[k + 1], (v, b, k)
        assert (s[l0] == s[l1]) == (lo_kind == "same") and (s[h0] == s[h1]) == (hi_kind == "same"), (v, b)
        qk = go.keys32(t["q"][v, b])
        for kind, q_key, at in ((lo_kind, qk[0], l0), (hi_kind, qk[1], h0)):
            on = keys == q_key
            if kind == "same":
                assert q_key == s[at] and int(on.sum()) >= 4 and int((on & (conf >= 3)).sum()) >= 2, (v, b, kind)
                assert bool(t["valid"][v, b].reshape(-1)[torch.from_numpy(on & (conf >= 3))].all())
            else:
                assert not on.any(), (v, b)
    assert {r[1] for r in rc.TIE_RUNS} == {"same", "split"} and {r[2] for r in rc.TIE_RUNS} == {"same", "split"}

    # constant rows: two segments, one key; every confident point is valid
    for name in ("constant_two_segments", "constant_zero_two_segments"):
        c, t = rc.case(name), rc.truth(name)
        v, b, keys, conf = next(rc.rows(c))
        assert len(keys) == 96 * 112 > rc.SEGMENT_SLOTS * rc.SLOT_POINTS and bool((keys == c["claims"]["key"]).all())
        assert go.keys32(t["q"][0, 0]).tolist() == [c["claims"]["key"]] * 2
        assert int(t["n_valid"][0, 0]) == int((conf >= 3).sum()) > 5000
    assert not bool(rc.case("constant_zero_two_segments")["gt_pts1"].any())

    # dense_ulps: 512 consecutive patterns; q_lo ON the floor statistic, q_hi ON the ceiling one, where the case says
    c, t = rc.case("dense_ulps"), rc.truth("dense_ulps")
    on_floor, on_ceil = [], []
    for v, b, keys, conf in rc.rows(c):
        s = np.sort(keys.astype(np.int64))
        assert s[-1] - s[0] <= 511
        qk = go.keys32(t["q"][v, b]).astype(np.int64)
        if s[l0] < s[l1] and qk[0] == s[l0]:
            on_floor.append((v, b))
        if s[h0] < s[h1] and qk[1] == s[h1]:
            on_ceil.append((v, b))
    print("dense_ulps: q_lo on the floor statistic in rows", on_floor, "q_hi on the ceiling statistic in rows", on_ceil)
    assert set(c["claims"]["lo_on_floor"]) <= set(on_floor) and set(c["claims"]["hi_on_ceil"]) <= set(on_ceil)
    by_rank = torch.stack([go.rank_mask(go._norms(c[f"gt_pts{v}"])) & (c[f"conf{v}"] >= 3) for v in (1, 2)])
    extra = (t["valid"] & ~by_rank).flatten(2).sum(2)
    assert not bool((by_rank & ~t["valid"]).any())
    for v, b in c["claims"]["lo_on_floor"]:       # the float32 thresholds keep what the ranks drop
        assert int(extra[v, b]) >= 1, (v, b, extra)

    # conf_edge: the planted confidences sit on points inside the band; 3 and +inf are valid, the other two are not
    c, t = rc.case("conf_edge"), rc.truth("conf_edge")
    assert len(c["claims"]["planted"]) == 16
    for v, b, i, value in c["claims"]["planted"]:
        dis, q = float(go.norm32(c[f"gt_pts{v + 1}"][b]).reshape(-1)[i]), t["q"][v, b]
        got = float(c[f"conf{v + 1}"][b].reshape(-1)[i])
        assert q[0] < dis < q[1] and (got == value or (math.isnan(got) and math.isnan(value)))
        assert bool(t["valid"][v, b].reshape(-1)[i]) == (value >= 3.0), (v, b, value)
    assert rc.CONF_PLANTS[0] == 3.0 and 2.9999 < rc.CONF_PLANTS[1] < 3.0

    # clip_edge: 8 and its lower neighbour are valid, its upper neighbour is not
    c, t = rc.case("clip_edge"), rc.truth("clip_edge")
    assert c["dist_clip"] == 8.0
    for v, b, keys, _ in rc.rows(c):
        assert keys[:3].tolist() == list(rc.CLIP_PLANTS)
        assert t["valid"][v, b].reshape(-1)[:3].tolist() == [True, False, True]
        assert 0 < int(t["n_valid"][v, b]) < len(keys)
    assert np.array([8.0], np.float32).view(np.uint32)[0] == rc.CLIP_PLANTS[0]

    # nan_point: finite thresholds, equal to those of the row without the point sorted in (the NaN is last); the point
    # invalid; nan_many: q_hi NaN, no valid point in that row, valid points in every other
    for name, many in (("nan_point", False), ("nan_many", True)):
        c, t = rc.case(name), rc.truth(name)
        (v, b), at = c["claims"]["row"], c["claims"]["at"]
        dis = go.norm32(c[f"gt_pts{v + 1}"][b]).reshape(-1)
        assert np.isnan(dis).nonzero()[0].tolist() == at and len(at) == (5 if many else 1)
        assert not bool(t["valid"][v, b].reshape(-1)[at].any())
        if many:
            assert len(at) > go.Q_LO * len(dis) and np.isfinite(t["q"][v, b, 0]) and np.isnan(t["q"][v, b, 1])
            assert int(t["n_valid"][v, b]) == 0
        else:
            as_max = np.where(np.isnan(dis), np.float32(np.inf), dis)
            assert _same_bits(t["q"][v, b], go.thresholds32(as_max[None])[0]) and bool(np.isfinite(t["q"][v, b]).all())
        others = t["n_valid"].clone()
        others[v, b] = 1
        assert bool((others > 0).all()) and int(np.isnan(t["q"]).sum()) == (1 if many else 0)

    # inf_point: the inf is invalid in both; at n = 15 the row has no valid point
    for name, n_valid_is_zero in (("inf_point_15", True), ("inf_point_1551", False)):
        c, t = rc.case(name), rc.truth(name)
        (v, b), (at,) = c["claims"]["row"], c["claims"]["at"]
        assert np.isinf(go.norm32(c[f"gt_pts{v + 1}"][b]).reshape(-1)[at])
        assert not bool(t["valid"][v, b].reshape(-1)[at]) and (int(t["n_valid"][v, b]) == 0) == n_valid_is_zero

    # small n and the long grids
    assert sorted(rc.SMALL_N) == [1, 2, 3, 1024, 1025, 8192, 8193]
    for n, (H, W) in rc.SMALL_N.items():
        c = rc.case(f"small_n_{n}")
        assert tuple(c["gt_pts1"].shape) == (2, H, W, 3) and H * W == n
        # (two different norms: q_lo lies above the smaller and q_hi below the larger, nothing is valid, the loss is NaN)
        assert (int(rc.truth(f"small_n_{n}")["n_valid"].sum()) > 0) == (n != 2), n
    s = rc.slot_counts(rc.case("long_grid_rows"))
    assert s["hist"] == s["point"] == s["rows"] == 2050 > rc.MAX_GRID and s["point"] // 2 < rc.MAX_GRID
    s = rc.slot_counts(rc.case("long_grid_slots"))
    assert s["nchunk"] == 7 and s["point"] == 2394 > rc.MAX_GRID and rc.MAX_GRID % 7 != 0      # a block changes rows
    for name in rc.LONG:
        assert int((rc.truth(name)["n_valid"] == 0).sum()) == 0 or name == "long_grid_rows"


# which cases a mutant is shown on (any would do; these are the ones built for it)
MUTANT_CASES = {
    "lo_strict": ("ties",), "hi_strict": ("ties",), "conf_strict": ("conf_edge",), "clip_strict": ("clip_edge",),
    "rank_n": ("patterns", "small_n_2"), "ceil_is_floor": ("patterns", "small_n_2"), "weight_zero": ("patterns",),
    "lerp_one_sided": ("ties", "small_n_2", "long_grid_rows"), "alias_none_low": ("patterns", "patterns_seg2"),
    "nan_low": ("nan_point", "nan_many"), "nan_poisons": ("nan_point",),
}


@pytest.mark.parametrize("mutant", go.MUTANTS)
def test_gate_catches_mutants(mutant):
    """Each mutant of the host restatement moves n_valid or the bits of q on a named case -- the gates the GPU tests
    hold the product to -- so a kernel with that mistake cannot pass.  alias_last is the exception BY CLAIM: naming the
    nearest earlier rank of a prefix instead of the first changes nothing (regr3d_oracle.radix_select32), on any case.
    nf_per_view cannot reach n_valid or q at all; it must move a norm factor by POWER bounds of the 1e-5 gate."""
    radix = mutant in go.RADIX_MUTANTS
    if mutant == "alias_last":
        for name in rc.NAMES:
            c = rc.case(name)
            if c["dist_clip"] is None:
                got = go.exact_truth(c, mutant, radix=True)
                assert _same_bits(got["q"], rc.truth(name)["q"]) and torch.equal(got["n_valid"], rc.truth(name)["n_valid"])
        return
    if mutant == "nf_per_view":
        c, t = rc.case("patterns"), rc.truth("patterns")
        for key in ("pr_pts", "gt_pts"):
            pts = [c[f"{key}1"], c[f"{key}2"]]
            joint, each = go.norm_factors64(pts, t["valid"]), go.norm_factors64(pts, t["valid"], per_view=True)
            assert float(((each - joint).abs() / joint).min()) > POWER * 1e-5, key
        return
    caught = []
    for name in MUTANT_CASES[mutant]:
        got, want = go.exact_truth(rc.case(name), mutant, radix=radix), rc.truth(name)
        if not _same_bits(got["q"], want["q"]) or not torch.equal(got["n_valid"], want["n_valid"]):
            caught.append(name)
    print(mutant, "caught on", caught)
    assert caught == list(MUTANT_CASES[mutant]), (mutant, caught)


# ---- GPU ---------------------------------------------------------------------------------------------------------

_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = go.run_ref(rc.case(name), valid_override=tuple(rc.truth(name)["valid"]))
    return _REF[name]


def _same(a, b):
    return all(torch.equal(x, y) or (x.dim() == 0 and math.isnan(float(x)) and math.isnan(float(y)))
               for x, y in ((a[0], b[0]), (a[2][0], b[2][0]), (a[2][1], b[2][1]))) and \
        all(_same_bits(a[1][k].cpu().numpy().view(np.float32), b[1][k].cpu().numpy().view(np.float32)) for k in a[1])


def _check_exact(name, run):
    c, t, ref = rc.case(name), rc.truth(name), _ref(name)
    loss, stats, grads = run
    q = stats["q"].cpu().numpy()
    bits_ok = _same_bits(q, t["q"])
    counts_ok = torch.equal(stats["n_valid"].cpu().long(), t["n_valid"])
    print(f"{name}: q bitwise {'pass' if bits_ok else 'FAIL'}, n_valid {'pass' if counts_ok else 'FAIL'}, "
          f"loss rel err {_rel(loss.cpu(), ref['loss']):.3g}")
    assert bits_ok, (name, "q", np.argwhere(q.view(np.uint32) != t["q"].view(np.uint32))[:8].tolist())
    assert counts_ok, (name, (stats["n_valid"].cpu().long() - t["n_valid"]).nonzero()[:8].tolist())
    _check_grads(grads, ref, C_PRODUCT, name)          # NaN / inf patterns, exact zeros at invalid points, the bound
    got, want = torch.stack([g.cpu() for g in grads]), torch.stack(ref["grad"])
    moved = t["valid"] & (want.abs().amax(-1) > 0)
    assert bool((got.abs().amax(-1) > 0)[moved].all()), (name, "a valid point without a gradient")
    for key in ("nf_pr", "nf_gt"):
        assert bool(((stats[key].cpu().double() - ref[key]).abs() <= 1e-5 * ref[key].abs()).all()), (name, key)
    assert _rel(loss.cpu(), ref["loss"]) < 1e-5, (name, float(loss), float(ref["loss"]))       # NaN matches NaN only


@pytest.mark.gpu
@pytest.mark.parametrize("name", rc.NAMES)
def test_hip_is_exact(hip_lib, name):
    c = rc.case(name)
    assert go.is_exact(c["gt_pts1"]) and go.is_exact(c["gt_pts2"])
    _check_exact(name, _hip(c))


@pytest.mark.gpu
def test_device_sqrt_is_exact_on_a_constant_row(hip_lib):
    """q of a constant row is lerp(x, x) = x: the planted pattern must come back, which it does only if the device's
    norm chain returns |z| for (0, 0, z)."""
    for name in ("constant_two_segments", "constant_zero_two_segments"):
        c = rc.case(name)
        _, stats, _ = _hip(c, grads=(False, False))
        assert go.keys32(stats["q"][0, 0].cpu().numpy()).tolist() == [c["claims"]["key"]] * 2, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("patterns",) + rc.LONG)
def test_one_view_alone_and_a_second_run_are_bitwise_the_same(hip_lib, name):
    c = rc.case(name)
    both = _hip(c)
    assert _same(both, _hip(c)), (name, "two runs differ")
    for grads in ((True, False), (False, True)):
        one = _hip(c, grads=grads)
        for v in (0, 1):
            want = both[2][v] if grads[v] else torch.zeros_like(both[2][v])
            assert torch.equal(one[2][v], want), (name, grads, v)
