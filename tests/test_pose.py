"""The pose path without a device: the float64 oracle (tests/pose_oracle.py) against goldens recorded from the reference's
own code (tests/golden/make_pose_goldens.py), the Python surface, and the C ABI's argument checks.

Bounds.  The reference ran in float32, the oracle here runs in float64 on the same float32 inputs, so a golden differs
from the oracle by the reference's own rounding: measured on fixtures built like these, poses <= 8e-7 and d enc <= 1.6e-6
of the tensor's largest entry, focals <= 1.6e-7 relative.  The caps are about ten times that: 1e-5, 2e-5, 1e-6.  A pose
error at angle a carries the float32 error of its cosine (about 3e-7) times 1/sin a <= 1/sin 2 deg = 29 on the parity
cases, in degrees 57.3 * 29 * 3e-7 = 5e-4: bound 2e-3 degrees."""
import ctypes as C
import math
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import pose_oracle as O

GOLD = torch.load(Path(__file__).parent / "golden" / "pose_goldens.pt", weights_only=True)
POSE_CAP, GRAD_CAP, FOCAL_CAP, ANGLE_CAP = 1e-5, 2e-5, 1e-6, 2e-3
COMPOSE = [k for k in GOLD["compose"] if k != "convert_pose_to_4x4"]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("name", COMPOSE)
def test_oracle_reproduces_compose_goldens(name):
    g = GOLD["compose"][name]
    e = g["enc"].double().requires_grad_(True)
    poses = O.process_pose(e, g["context_views"], encoding=g["encoding"], pose_make_baseline_1=g["baseline"],
                           pose_make_relative=g["relative"])
    (ge,) = torch.autograd.grad((poses * g["upstream"].double()).sum(), e)
    assert rel(g["poses"], poses.detach()) <= POSE_CAP
    assert rel(g["grad_enc"], ge) <= GRAD_CAP
    assert torch.equal(g["poses"][..., 3, :], torch.tensor([0.0, 0.0, 0.0, 1.0]).expand_as(g["poses"][..., 3, :]))
    if g["encoding"] == "absT_quaR_FoV":
        assert torch.equal(ge[..., 7:], torch.zeros_like(ge[..., 7:]))


def test_oracle_reproduces_convert_pose_to_4x4():
    g = GOLD["compose"]["convert_pose_to_4x4"]
    assert rel(g["poses"], O.convert_pose_to_4x4(g["out"].double())) <= POSE_CAP


def test_compose_fixtures_are_well_conditioned_by_construction():
    gen = torch.Generator().manual_seed(3)
    for encoding in O.ENCODINGS:
        enc = O.make_enc(gen, 65, 3, 2, encoding).double()
        t = O.decode(enc, encoding)[..., :3, 3]
        assert float((t[:, 0] - t[:, 1]).norm(dim=-1).min()) >= 0.3 - 1e-6
        if encoding == "rot6d":
            a1, a2 = enc[..., :3], enc[..., 3:6]
            for a in (a1, a2):
                n = a.norm(dim=-1)
                assert float(n.min()) >= 0.3 - 1e-6 and float(n.max()) <= 2 + 1e-6
            ang = torch.rad2deg(torch.acos((a1 * a2).sum(-1) / (a1.norm(dim=-1) * a2.norm(dim=-1))))
            assert float(ang.min()) >= 18 - 1e-3 and float(ang.max()) <= 162 + 1e-3
        else:
            n = enc[..., 3:7].norm(dim=-1)
            assert float(n.min()) >= 0.5 - 1e-6 and float(n.max()) <= 1.5 + 1e-6


@pytest.mark.parametrize("name", list(GOLD["depth"]))
def test_oracle_reproduces_depth_goldens(name):
    g = GOLD["depth"][name]
    p, q = g["pts3d"].double().requires_grad_(True), g["poses"].double().requires_grad_(True)
    depth = O.depth_projector(p, q)
    gp, gq = torch.autograd.grad((depth * g["upstream"].double()).sum(), [p, q])
    assert rel(g["depth"], depth.detach()) <= POSE_CAP
    assert rel(g["grad_pts3d"], gp) <= GRAD_CAP
    assert rel(g["grad_poses"], gq) <= GRAD_CAP


def test_oracle_reproduces_pose_error_goldens():
    g = GOLD["errors"]["parity"]
    e = O.pose_errors(g["pred"].double(), g["tgt"].double())
    assert float(e[:, 0].min()) >= 2 - 1e-3 and float(e[:, 2].min()) >= 2 - 1e-3 and float(e[:, 2].max()) <= 178 + 1e-3
    assert float((e[:, [0, 2]] - g["per_pose"][:, [0, 2]].double()).abs().max()) <= ANGLE_CAP
    assert rel(g["per_pose"][:, 1], e[:, 1]) <= FOCAL_CAP
    ang, trans = O.compute_pose_error_for_batch(g["pred"].double().reshape(8, 5, 4, 4), g["tgt"].double().reshape(8, 5, 4, 4))
    assert abs(float(ang) - float(g["batch_8x5"][0])) <= ANGLE_CAP and abs(float(trans) - float(g["batch_8x5"][1])) <= ANGLE_CAP
    ang, trans = O.compute_pose_error_for_batch(g["pred"][3].double(), g["tgt"][3].double())
    assert abs(float(ang) - float(g["single_3"][0])) <= ANGLE_CAP and abs(float(trans) - float(g["single_3"][1])) <= ANGLE_CAP


def test_pose_error_edge_cases_as_the_reference_gives_them():
    """Identical poses, a 180 degree rotation, zero translation (90 degrees by the 1e-9 term).  Next to 0 and 180 degrees
    the reference's float32 acos is good to 0.03 degrees only, which is the bound here."""
    g = GOLD["errors"]["edges"]
    assert g["per_pose"].tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 180.0], [90.0, pytest.approx(2.2561028), 0.0]]
    e = O.pose_errors(g["pred"].double(), g["tgt"].double())
    assert float((e - g["per_pose"].double()).abs().max()) <= 0.03


@pytest.mark.parametrize("name", [k for k in GOLD["focal"] if "focal" in GOLD["focal"][k]])
def test_oracle_reproduces_focal_goldens(name):
    g = GOLD["focal"][name]
    pp = g["pp"].double() if "pp" in g else None
    # the subnormal z of the exact scene makes x / z overflow to inf (-> 0) in float32 ONLY: in float64 the quotient is a
    # finite 1e41 that swamps the sums.  Per-point arithmetic is float32 by contract, so that case runs the oracle there.
    dt = torch.float32 if name == "edge_exact_odd_points" else torch.float64
    f = O.estimate_focal_knowing_depth(g["pts3d"].to(dt), pp)
    if g.get("expected", 0.0) is None:
        assert bool(torch.isnan(g["focal"]).all()) and bool(torch.isnan(f).all())
        return
    assert rel(g["focal"], f) <= FOCAL_CAP
    if "expected" in g:
        assert float(g["focal"]) == pytest.approx(g["expected"], rel=1e-6)


def test_named_focal_edge_values():
    assert O.focal_base(12, 16) == pytest.approx(13.8564, abs=1e-4)
    pts, want = O.focal_edges()["mirrored"]
    a = pts[0].double().reshape(-1, 3)
    jj, ii = torch.meshgrid(torch.arange(16.0, dtype=torch.float64), torch.arange(12.0, dtype=torch.float64), indexing="xy")
    px = torch.stack([jj - 8, ii - 6], -1).reshape(-1, 2)
    xy = a[:, :2] / a[:, 2:]
    assert float((xy * px).sum() / xy.square().sum()) == pytest.approx(-10.0)
    assert float(O.estimate_focal_scene(pts[0].double())) == pytest.approx(want)


def test_normalize_intrinsics_row_divisors_on_a_non_square_image():
    g = GOLD["focal"]["intrinsics_24x32"]
    K = g["intrinsics"]
    f = GOLD["focal"]["24x32"]["focal"]
    assert K.shape == (2, 3, 3)
    assert torch.allclose(K[:, 0, 0], f / 24, rtol=1e-6) and torch.allclose(K[:, 1, 1], f / 32, rtol=1e-6)
    assert torch.allclose(K[:, 0, 2], torch.tensor(16 / 24)) and torch.allclose(K[:, 1, 2], torch.tensor(12 / 32))
    assert rel(K, O.estimate_intrinsics(g["pts3d"].double(), 24, 32)) <= FOCAL_CAP
    assert torch.equal(O.intrinsics_from_focal(f, 24, 32)[:, 2], torch.tensor([0.0, 0.0, 1.0]).expand(2, 3))


def test_pose_auc_against_the_reference(monkeypatch):
    from spfsplatv2_amd import pose
    g = GOLD["errors"]["auc"]
    for fn in (pose.pose_auc, O.pose_auc):
        assert fn(g["errors"].numpy(), g["thresholds"]) == pytest.approx(g["auc"], rel=1e-12)
    assert pose.pose_auc(g["errors"], g["thresholds"]) == pytest.approx(g["auc"], rel=1e-12)     # a tensor
    # by hand: recall steps to 1/2 at 1 and to 1 at 3 (linear between); area to 2 = 1/4 + 1/2, to 4 = 1/4 + 3/2 + 1
    assert pose.pose_auc([1.0, 3.0], [2.0, 4.0]) == pytest.approx([0.375, 0.6875])
    for name in ("trapz", "trapezoid"):                      # runs on a numpy with or without either
        monkeypatch.delattr(np, name, raising=False)
    assert pose.pose_auc(g["errors"].numpy(), g["thresholds"]) == pytest.approx(g["auc"], rel=1e-12)


def test_module_surface_and_export_names():
    import inspect

    import spfsplatv2_amd as spf
    from spfsplatv2_amd import pose
    names = ["convert_pose_to_4x4", "process_pose", "depth_projector", "process_depth", "compute_pose_error",
             "compute_pose_error_for_batch", "pose_errors", "pose_auc", "estimate_focal_knowing_depth",
             "estimate_intrinsics"]
    for n in names:
        assert getattr(spf, n) is getattr(pose, n) and n in spf.__all__, n
    assert list(inspect.signature(pose.process_pose).parameters) == [
        "pose_enc", "context_views", "encoding", "pose_make_baseline_1", "pose_make_relative"]
    assert list(inspect.signature(pose.estimate_focal_knowing_depth).parameters) == [
        "pts3d", "pp", "focal_mode", "min_focal", "max_focal"]
    assert list(inspect.signature(pose.compute_pose_error).parameters) == ["pose_gt", "pose_pred"]
    assert list(inspect.signature(pose.compute_pose_error_for_batch).parameters) == ["pred_pose", "tgt_pose"]
    for word in ("view 0", "height", "ONE FOCAL PER SCENE", "CPU tensors", "get_pnp_pose", "SE3_exp",
                 "camera_normalization", "median"):
        assert word in pose.__doc__, word


def test_cpu_tensors_median_and_bad_arguments_raise():
    from spfsplatv2_amd import pose
    enc = GOLD["compose"]["rot6d_both"]["enc"]
    d = GOLD["depth"]["two_small"]
    e = GOLD["errors"]["parity"]
    pts = GOLD["focal"]["24x32"]["pts3d"]
    calls = [lambda: pose.process_pose(enc, 2, pose_make_baseline_1=True, pose_make_relative=True),
             lambda: pose.convert_pose_to_4x4(enc[0]),
             lambda: pose.depth_projector(d["pts3d"], d["poses"]),
             lambda: pose.process_depth(d["poses"][None], d["pts3d"].reshape(1, 2, 20, 15, 3)),
             lambda: pose.compute_pose_error(e["tgt"][0], e["pred"][0]),
             lambda: pose.compute_pose_error_for_batch(e["pred"], e["tgt"]),
             lambda: pose.pose_errors(e["pred"], e["tgt"]),
             lambda: pose.estimate_focal_knowing_depth(pts),
             lambda: pose.estimate_intrinsics(pts[:, None], 24, 32)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(NotImplementedError, match="median"):
        pose.estimate_focal_knowing_depth(pts, focal_mode="median")
    with pytest.raises(ValueError, match="bad focal_mode"):
        pose.estimate_focal_knowing_depth(pts, focal_mode="mean")
    with pytest.raises(ValueError, match="unknown encoding"):
        pose.process_pose(enc, 2, encoding="euler", pose_make_baseline_1=False, pose_make_relative=False)
    for cv in (0, 4):
        with pytest.raises(ValueError, match="context_views"):
            pose.process_pose(enc, cv, pose_make_baseline_1=False, pose_make_relative=False)
    with pytest.raises(RuntimeError, match=r"\[b, v, 9\]"):
        pose.process_pose(enc[..., :8], 2, pose_make_baseline_1=False, pose_make_relative=False)


def test_c_abi_rejects_bad_arguments_without_a_device(hip_lib):
    p = C.c_void_p(256)                   # never dereferenced: every rejection happens before a launch
    odd = C.c_void_p(258)
    err = hip_lib.spf_last_error

    def compose(fn, enc=p, sb=18, sv=9, b=2, v=2, cv=2, encoding=0, extra=(p,)):
        return fn(enc, sb, sv, b, v, cv, encoding, 1, 1, *extra, None)
    for fn, extra in ((hip_lib.spf_pose_compose_forward, (p,)), (hip_lib.spf_pose_compose_backward, (p, p))):
        for kw, msg in (({"enc": None}, b"null"), ({"b": 0}, b"positive"), ({"v": -1}, b"positive"),
                        ({"cv": 0}, b"context_views"), ({"cv": 3}, b"context_views"), ({"encoding": 2}, b"encoding"),
                        ({"sb": -18}, b"negative"), ({"enc": odd}, b"aligned"), ({"extra": (None,) * len(extra)}, b"null")):
            assert compose(fn, **{"extra": extra, **kw}) == -1, kw
            assert msg in err(), (kw, err())
    assert hip_lib.spf_depth_project_partial_blocks(2, 768) == 2 and hip_lib.spf_depth_project_partial_blocks(3, 1551) == 6
    assert hip_lib.spf_depth_project_partial_blocks(1, 65536) == 64
    assert hip_lib.spf_depth_project_partial_blocks(0, 5) == -1 and hip_lib.spf_depth_project_partial_blocks(1, 0) == -1
    assert hip_lib.spf_depth_project_partial_blocks(1, 2 ** 30) == -1
    fwd, bwd = hip_lib.spf_depth_project_forward, hip_lib.spf_depth_project_backward
    for args, msg in (((None, 30, p, 1, 10, p), b"null"), ((p, 30, None, 1, 10, p), b"null"), ((p, 30, p, 1, 10, None), b"null"),
                      ((p, 30, p, 0, 10, p), b"positive"), ((p, 30, p, 1, -1, p), b"positive"),
                      ((p, 30, p, 1, 2 ** 30, p), b"too large"), ((p, -30, p, 1, 10, p), b"negative"),
                      ((odd, 30, p, 1, 10, p), b"aligned")):
        assert fwd(*args, None) == -1 and msg in err(), (args, err())
    assert bwd(p, 30, p, 1, 10, None, p, p, p, None) == -1 and b"null" in err()
    assert bwd(p, 30, p, 1, 10, p, None, None, None, None) == -1 and b"no gradient" in err()
    assert bwd(p, 30, p, 1, 10, p, p, None, p, None) == -1 and b"go together" in err()
    assert bwd(p, 30, p, 1, 10, p, p, C.c_void_p(264), p, None) == -1 and b"16-byte" in err()
    assert bwd(p, 30, p, 0, 10, p, p, p, p, None) == -1 and b"positive" in err()
    pe = hip_lib.spf_pose_error
    assert pe(None, p, 1, p, p, None) == -1 and b"null" in err()
    assert pe(p, p, 1, p, None, None) == -1 and b"null" in err()
    assert pe(p, p, 0, p, p, None) == -1 and b"positive" in err()
    assert pe(p, odd, 1, p, p, None) == -1 and b"aligned" in err()
    assert hip_lib.spf_focal_scratch_bytes(16, 256, 256) == 0 and hip_lib.spf_focal_scratch_bytes(0, 4, 4) == -1
    assert hip_lib.spf_focal_scratch_bytes(1, 40000, 40000) == -1

    def focal(pts=p, ss=36, sr=12, B=1, H=3, W=4, pp=None, pps=0, out=p):
        return hip_lib.spf_focal_estimate(pts, ss, sr, B, H, W, pp, pps, 0.0, math.inf, 2.0, 1.5, 3.0, 4.0, None, out, p, None)
    for kw, msg in (({"pts": None}, b"null"), ({"out": None}, b"null"), ({"B": 0}, b"positive"), ({"W": -4}, b"positive"),
                    ({"H": 40000, "W": 40000}, b"too large"), ({"sr": -12}, b"negative"), ({"pps": 1}, b"pp_stride"),
                    ({"pp": odd}, b"aligned")):
        assert focal(**kw) == -1 and msg in err(), (kw, err())
    assert hip_lib.spf_abi_version() == 7
