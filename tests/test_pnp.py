"""The PnP solver's definition (tests/pnp_oracle.py) against planted truth, and the public surface of
spfsplatv2_amd/pnp.py -- everything that needs no GPU.

Bounds: the noise-free scene built from float64 points is recovered to 1e-9 (the Gauss-Newton fixed point is the planted
pose; float64 leaves ~1e-15).  A noisy scene is held to twice pnp_cases.PLANTED_ERROR, the float64 oracle's own distance
from the planted pose on that fixture: the same estimator on another seed scatters that much."""
import inspect
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import pnp_cases as Cs
from tests import pnp_oracle as O
from tests.conftest import ROOT

GOLD = torch.load(Path(__file__).parent / "golden" / "pnp_goldens.pt", weights_only=True)


# ---- the oracle against the planted truth ------------------------------------------------------------------------------
def test_noise_free_float64_points_recover_the_planted_pose():
    view = Cs.planted_view(24, 32, seed=11, dtype=np.float64)
    r = O.solve_view(view["pts"], view["opacity"], view["K"], 24, 32)
    assert r["success"] == 1 and r["inliers"] == r["candidates"] == 768
    assert np.abs(r["pose"] - view["pose"]).max() <= 1e-9
    assert (r["pose"][3] == [0, 0, 0, 1]).all()


@pytest.mark.parametrize("name", sorted(Cs.SINGLE))
def test_goldens_are_within_twice_the_recorded_distance_from_the_planted_pose(name):
    g = GOLD["single"][name]
    view = dict(pose=g["planted_pose"].numpy())
    ang, dt = Cs.pose_errors(g["f64"]["pose"].numpy(), view)          # the bound is the float64 oracle's
    lim = Cs.PLANTED_ERROR[name]
    assert ang <= 2 * lim[0] and dt <= 2 * lim[1], (name, ang, dt)
    for tag in ("f64", "f32"):
        assert int(g[tag]["success"]) == 1 and int(g[tag]["inliers"]) == int(g["f64"]["inliers"])


def test_the_goldens_are_what_the_oracle_computes_and_the_scene_is_unambiguous():
    h, w, kw, solve = Cs.SINGLE["tail_20x15"]
    view = Cs.planted_view(h, w, **kw)
    g = GOLD["single"]["tail_20x15"]
    assert torch.equal(torch.from_numpy(view["pts"]), g["pts"]) and torch.equal(torch.from_numpy(view["opacity"]), g["opacity"])
    for tag, dtype in (("f64", np.float64), ("f32", np.float32)):
        r = O.solve_view(view["pts"], view["opacity"], view["K"], h, w, dtype=dtype, **solve)
        assert np.abs(r["pose"] - g[tag]["pose"].numpy()).max() <= 1e-12
        assert [r[f] for f in ("inliers", "candidates", "hypothesis", "success")] == \
               [int(g[tag][f]) for f in ("inliers", "candidates", "hypothesis", "success")]
        if dtype is np.float64:
            Cs.check_unambiguous(view, r)
            assert np.array_equal(r["ranks"], g["ranks"].numpy())
            assert r["inliers"] == int(view["planted"].sum()) == 183


def test_failures_give_the_identity():
    views = Cs.batch_views()
    for view, n in ((views[0][1], 3), (views[1][0], 0)):
        r = O.solve_view(view["pts"], view["opacity"], view["K"], 24, 32)
        assert r["success"] == 0 and r["inliers"] == 0 and r["hypothesis"] == -1 and r["candidates"] == n
        assert np.array_equal(r["pose"], np.eye(4))
    b = GOLD["batch"]
    assert b["f64"]["success"].tolist() == [[1, 0, 1], [0, 1, 1]]
    assert b["f64"]["candidates"][0, 2] == 24 * 32 - 16            # the NaN corner is no candidate although its opacity is on
    assert torch.equal(b["f64"]["pose"][0, 1], torch.eye(4, dtype=torch.float64))


# ---- hash and rank map -------------------------------------------------------------------------------------------------
def test_hash_and_rank_map_against_hand_computed_values():
    assert O.mix32(0) == 0 and O.mix32(1) == 0x688990C0
    assert O.mix32(0x9E3779B9) == 0x01FCE552
    assert O.hash3(0, 0, 0) == 0x944FB554 == O.mix32(O.mix32(0x01FCE552))
    assert O.hash3(0, 5, 2) == 0xFBC15F29 and O.hash3(7, 127, 11) == 0xF79C9C0C
    # mulhi32: floor(h n / 2^32) -- 0x944fb554 / 2^32 = 0.57934..., times 768 = 444.9
    assert O.rank_of(0x944FB554, 768) == 444 == math.floor(0x944FB554 / 2 ** 32 * 768)
    assert O.rank_of(0xFFFFFFFF, 300) == 299 and O.rank_of(0, 300) == 0 and O.rank_of(0x80000000, 5) == 2
    ranks, ok = O.sample_ranks(768)
    assert ranks[:3].tolist() == [[444, 536, 761, 92], [595, 419, 116, 732], [443, 63, 471, 361]] and ok.all()
    assert all(len(set(r)) == 4 and 0 <= min(r) and max(r) < 768 for r in ranks.tolist())


def test_redraws_voids_and_independence_of_the_batch():
    ranks, ok = O.sample_ranks(4)                 # four candidates: most samples need redraws, some run out of them
    assert ranks[:4].tolist() == [[2, 3, 0, 1], [3, 2, 0, -1], [2, 0, 1, 3], [0, 1, 2, 3]]
    assert int(ok.sum()) == 118 and not ok[1]
    assert all(sorted(r) == [0, 1, 2, 3] for r, good in zip(ranks.tolist(), ok) if good)
    ranks, ok = O.sample_ranks(3)
    assert (ranks == -1).all() and not ok.any()
    # nothing but (seed, k, draw) and n enters: the ranks have no argument for the view's place in a batch
    assert list(inspect.signature(O.sample_ranks).parameters) == ["n", "iterations", "seed"]
    assert not np.array_equal(O.sample_ranks(768, seed=1)[0], O.sample_ranks(768, seed=0)[0])


# ---- P3P ---------------------------------------------------------------------------------------------------------------
def test_p3p_roots_reproject_their_three_points():
    rng = np.random.default_rng(5)
    cam = (28.4, 0.3, 16.0, 21.3, 12.0)           # with a skew: the full upper-triangular K
    found_truth = total = 0
    for trial in range(200):
        axis = rng.normal(size=3)
        R = O.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0, 0.5))
        t = rng.normal(size=3) * 0.5
        px = np.stack([rng.uniform(0, 32, 4), rng.uniform(0, 24, 4)], 1)
        Y = (px[:, 1] - cam[4]) / cam[3]
        rays = np.stack([(px[:, 0] - cam[2] - cam[1] * Y) / cam[0], Y, np.ones(4)], 1)
        Xc = rays * np.exp(rng.uniform(0, np.log(20.0), 4))[:, None]
        Pw = (Xc - t) @ R
        roots = O.p3p_all(cam, Pw, px)
        assert 1 <= len(roots) <= 4
        for Rr, tr in roots:
            u, v, Xr = O.project(cam, Rr, tr, Pw[:3])
            assert (Xr[:, 2] > 0).all()
            assert np.abs(u - px[:3, 0]).max() <= 1e-9 and np.abs(v - px[:3, 1]).max() <= 1e-9, trial
            assert np.abs(Rr @ Rr.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rr) - 1) <= 1e-12
            total += 1
        pick = O.p3p(cam, Pw, px)
        assert pick is not None
        found_truth += np.abs(pick[0] - R).max() <= 1e-7 and np.abs(pick[1] - t).max() <= 1e-6
    assert found_truth >= 196 and total > 200      # the fourth point picks the planted root; several trials have >1 root


def test_quartic_roots_on_known_polynomials():
    assert np.allclose(sorted(O.quartic_roots(1, -10, 35, -50, 24)), [1, 2, 3, 4], atol=1e-12)
    assert np.allclose(sorted(O.quartic_roots(2, 0, -10, 0, 8)), [-2, -1, 1, 2], atol=1e-12)       # biquadratic: q = 0
    assert O.quartic_roots(1, 0, 2, 0, 5) == [] and O.quartic_roots(0, 1, 1, 1, 1) == []
    assert np.allclose(sorted(O.quartic_roots(1, -1, -7, 1, 6)), [-2, -1, 1, 3], atol=1e-12)


# ---- the public surface ------------------------------------------------------------------------------------------------
def test_names_signatures_and_build_list():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import _lib, build, pnp
    for name in ("get_pnp_pose", "get_pnp_pose_batch", "pnp_poses", "PnPResult"):
        assert name in spf.__all__ and getattr(spf, name) is getattr(pnp, name)
    assert list(inspect.signature(pnp.get_pnp_pose).parameters) == \
        ["pts3d", "opacity", "K", "H", "W", "opacity_threshold", "initial_pose"]
    assert list(inspect.signature(pnp.get_pnp_pose_batch).parameters) == ["pts3d", "opacity", "K", "H", "W", "opacity_threshold"]
    sig = inspect.signature(pnp.pnp_poses)
    assert {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY} == \
        dict(opacity_threshold=0.3, iterations=128, reprojection_error=5.0, refine_steps=10, seed=0)
    assert inspect.signature(pnp.get_pnp_pose).parameters["opacity_threshold"].default == 0.3
    assert pnp.PnPResult._fields == ("poses", "inliers", "candidates", "hypothesis", "success")
    assert "pnp.hip" in build.SOURCES and (ROOT / "spfsplatv2_amd" / "csrc" / "pnp.hip").exists()
    assert {"spf_pnp_workspace_bytes", "spf_pnp_solve"} <= set(_lib.SYMBOLS) and _lib.ABI_VERSION == 7
    header = (ROOT / "include" / "spfsplat_hip.h").read_text()
    assert "spf_pnp_solve(" in header and "spf_pnp_workspace_bytes(" in header
    assert _lib.SYMBOLS["spf_pnp_solve"][1][-1] is _lib.C.c_void_p            # the stream goes last
    assert (O.ITERATIONS, O.REPROJECTION_ERROR, O.REFINE_STEPS, O.SEED) == (128, 5.0, 10, 0)
    import spfsplatv2_amd.pose as pose
    assert "pnp.py" in pose.__doc__


def test_workspace_sizes_and_entry_point_validation(hip_lib):
    from spfsplatv2_amd import _lib
    G = (300 + 63) // 64
    want = 6 * (8 * G + 4 * (G + 1) + 52 * 128)
    assert hip_lib.spf_pnp_workspace_bytes(6, 20, 15, 128) == (want + 15) // 16 * 16
    for bad in ((0, 20, 15, 128), (6, 0, 15, 128), (6, 20, 15, 100), (6, 20, 15, 32), (6, 20, 15, 2048), (6, 4096, 4096, 128),
                (65536, 20, 15, 128)):
        assert hip_lib.spf_pnp_workspace_bytes(*bad) == -1, bad
    assert hip_lib.spf_pnp_solve(None, None, None, None, None, None) != 0
    args = _lib.SpfPnp(None, None, None, (_lib.C.c_int64 * 4)(), (_lib.C.c_int64 * 4)(), 1, 1, 4, 4, 96, 10, 0, 0.3, 5.0, 0)
    assert hip_lib.spf_pnp_solve(args, None, None, None, None, None) != 0
    assert b"multiple of 64" in hip_lib.spf_last_error()
    args.iterations = 128
    assert hip_lib.spf_pnp_solve(args, None, None, None, None, None) != 0
    assert b"null pointer" in hip_lib.spf_last_error()


def test_every_refusal_comes_before_the_missing_device():
    from spfsplatv2_amd import pnp
    b, v, h, w = 2, 3, 8, 12
    pts, opa, K = torch.zeros(b, v, h, w, 3), torch.ones(b, v, h, w), torch.eye(3).expand(b, v, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pnp.pnp_poses(pts, opa, K, h, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pnp.get_pnp_pose_batch(pts, opa, K, h, w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pnp.get_pnp_pose(pts[0, 0], opa[0, 0], K[0, 0], h, w)
    with pytest.raises(RuntimeError, match="opacity must be"):
        pnp.pnp_poses(pts, opa[:, :, :-1], K, h, w)
    with pytest.raises(RuntimeError, match="K must be"):
        pnp.pnp_poses(pts, opa, K[:, :1], h, w)
    with pytest.raises(RuntimeError, match="pts3d must be"):
        pnp.pnp_poses(pts[..., :2], opa, K, h, w)
    with pytest.raises(RuntimeError, match="pts3d must be"):
        pnp.get_pnp_pose_batch(pts[0], opa[0], K[0], h, w)
    with pytest.raises(RuntimeError, match="differ from the point map"):
        pnp.pnp_poses(pts, opa, K, w, h)
    with pytest.raises(RuntimeError, match="differ from the point map"):
        pnp.get_pnp_pose(pts[0, 0], opa[0, 0], K[0, 0], h, w + 1)
    for bad in (100, 32, 0, 1088, 2048):
        with pytest.raises(ValueError, match="multiple of 64"):
            pnp.pnp_poses(pts, opa, K, h, w, iterations=bad)
    with pytest.raises(ValueError, match="refine_steps"):
        pnp.pnp_poses(pts, opa, K, h, w, refine_steps=-1)
    with pytest.raises(ValueError, match="reprojection_error"):
        pnp.pnp_poses(pts, opa, K, h, w, reprojection_error=0.0)
    with pytest.raises(RuntimeError, match="floating-point"):
        pnp.pnp_poses(pts, opa > 0.5, K, h, w)
    with pytest.raises(TypeError):
        pnp.pnp_poses(pts.numpy(), opa, K, h, w)
    with pytest.raises(NotImplementedError, match="initial_pose"):
        pnp.get_pnp_pose(pts[0, 0], opa[0, 0], K[0, 0], h, w, 0.3, torch.eye(4))
    with pytest.raises(NotImplementedError, match="initial_pose"):
        pnp.get_pnp_pose(pts[0, 0], opa[0, 0], K[0, 0], h, w, initial_pose=torch.eye(4))
