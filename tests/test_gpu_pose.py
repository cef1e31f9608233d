"""The pose kernels (spfsplatv2_amd/csrc/pose.hip) on the GPU.

Truth is tests/pose_oracle.py in float64 on the host, on the same float32 inputs.  The yardstick for what float32 may lose
is THE SAME ORACLE IN FLOAT32 on the host -- for golden cases the reference's own recorded float32 run -- never the
product.  With err(x) = max |x - truth| / max |truth|:

    err(product) <= min(4 * err(yardstick) + floor, cap)

4 x: the kernels sum the same products in another order (and chain the backward differently), another draw from the same
rounding, not another order of magnitude -- as in test_gpu_ssim.py.  The caps are about ten times what the reference's
float32 run loses on fixtures built like these (poses 8e-7, d enc 1.6e-6, focal 1.6e-7):

    tensor                      floor   cap
    poses                       1e-7    1e-5
    d enc, depth gradients      1e-7    2e-5
    depth                       --      1e-5 of max |z|
    focal                       --      1e-6 relative

Pose errors are float32 roundings of float64 arithmetic on values up to 180: <= 2e-5 degrees absolute for the angles,
<= 1e-6 relative for error_t_scale, against the float64 oracle; no yardstick is needed.  Every (case, product error,
yardstick error) triple is appended to profiles/pose_parity.jsonl (SPF_POSE_PARITY_LOG names another file)."""
import itertools
import json
import math
import os
from pathlib import Path

import pytest
import torch

from tests import pose_oracle as O

pytestmark = pytest.mark.gpu

GOLD = torch.load(Path(__file__).parent / "golden" / "pose_goldens.pt", weights_only=True)
LOG = Path(os.environ.get("SPF_POSE_PARITY_LOG", Path(__file__).resolve().parents[1] / "profiles" / "pose_parity.jsonl"))
F64, F32 = torch.float64, torch.float32
POSE, GRAD = (1e-7, 1e-5), (1e-7, 2e-5)
DEPTH_CAP, FOCAL_CAP, ANGLE_CAP, SCALE_CAP = 1e-5, 1e-6, 2e-5, 1e-6


def spf():
    import spfsplatv2_amd
    return spfsplatv2_amd


def _log(case, product, yardstick):
    print(case, "product", product, "yardstick", yardstick)
    try:
        with open(LOG, "a") as f:
            f.write(json.dumps({"case": case, "product": product, "yardstick": yardstick}) + "\n")
    except OSError:                       # a read-only tree: the assertions below still hold
        pass


def err(x, truth):
    return float((x.detach().cpu().double() - truth.detach().double()).abs().max() / truth.detach().double().abs().max())


def hold(case, product, yardstick, truth, floor_cap):
    floor, cap = floor_cap
    ep, ey = err(product, truth), err(yardstick, truth)
    _log(case, ep, ey)
    assert ep <= min(4 * ey + floor, cap), (case, ep, ey)


def oracle_compose(enc, cv, encoding, bl, rel, G, dtype):
    e = enc.to(dtype).requires_grad_(True)
    poses = O.process_pose(e, cv, encoding=encoding, pose_make_baseline_1=bl, pose_make_relative=rel)
    (g,) = torch.autograd.grad((poses * G.to(dtype)).sum(), e)
    return poses.detach(), g


def product_compose(enc, cv, encoding, bl, rel, G):
    e = enc.cuda().requires_grad_(True)
    poses = spf().process_pose(e, cv, encoding=encoding, pose_make_baseline_1=bl, pose_make_relative=rel)
    (g,) = torch.autograd.grad(poses, e, G.cuda())
    return poses.detach(), g


# ---- 1. composition --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", O.ENCODINGS)
@pytest.mark.parametrize("shape", [(1, 2), (3, 4), (2, 12), (65, 3)])
def test_compose_matches_the_oracle(hip_lib, shape, encoding):
    b, v = shape
    gen = torch.Generator().manual_seed(100 * b + v)
    bottom = torch.tensor([0.0, 0.0, 0.0, 1.0])
    for cv, (bl, rel) in itertools.product(sorted({1, 2, v}), itertools.product((False, True), repeat=2)):
        case = f"compose/{encoding}/{b}x{v}/cv{cv}/baseline{int(bl)}/relative{int(rel)}"
        enc = O.make_enc(gen, b, v, cv, encoding)
        G = torch.randn(b, v, 4, 4, generator=gen)
        poses, g = product_compose(enc, cv, encoding, bl, rel, G)
        assert poses.dtype == F32 and poses.shape == (b, v, 4, 4) and g.shape == (b, v, 9)
        if bl and cv == 1:
            # |t_0 - t_0| = 0: the reference divides by zero, every translation is +-inf or NaN (and with
            # pose_make_relative the inverse of such a matrix is not defined: torch.linalg.inv may refuse it).  No
            # translation may come out finite; the gradient of 0/0 is not compared.
            assert not bool(torch.isfinite(poses[..., :3, 3]).any()), case
            continue
        assert torch.equal(poses[..., 3, :].cpu(), bottom.expand(b, v, 4)), case
        truth_p, truth_g = oracle_compose(enc, cv, encoding, bl, rel, G, F64)
        yard_p, yard_g = oracle_compose(enc, cv, encoding, bl, rel, G, F32)
        hold(case + "/poses", poses, yard_p, truth_p, POSE)
        hold(case + "/d_enc", g, yard_g, truth_g, GRAD)
        if encoding == "absT_quaR_FoV":
            assert not bool(g[..., 7:].any()), case


@pytest.mark.parametrize("name", [k for k in GOLD["compose"] if k != "convert_pose_to_4x4"])
def test_compose_matches_the_reference_goldens(hip_lib, name):
    g = GOLD["compose"][name]
    args = (g["enc"], g["context_views"], g["encoding"], g["baseline"], g["relative"], g["upstream"])
    poses, ge = product_compose(*args)
    truth_p, truth_g = oracle_compose(*args, F64)
    hold(f"compose_golden/{name}/poses", poses, g["poses"], truth_p, POSE)
    hold(f"compose_golden/{name}/d_enc", ge, g["grad_enc"], truth_g, GRAD)


def test_convert_pose_to_4x4_matches_the_reference_golden(hip_lib):
    g = GOLD["compose"]["convert_pose_to_4x4"]
    x = g["out"].cuda().requires_grad_(True)
    poses = spf().convert_pose_to_4x4(x)
    assert poses.shape == (5, 4, 4) and poses.dtype == F32
    hold("convert_pose_to_4x4", poses, g["poses"], O.convert_pose_to_4x4(g["out"].double()), POSE)
    poses.sum().backward()
    assert bool(torch.isfinite(x.grad).all()) and bool(x.grad[:, 6:].eq(1).all())


def test_compose_strided_view_no_grad_and_other_dtypes(hip_lib):
    gen = torch.Generator().manual_seed(9)
    wide = torch.randn(3, 4, 12, generator=gen)
    wide[..., :9] = O.make_enc(gen, 3, 4, 2, "rot6d")
    wide = wide.cuda()
    view = wide[..., :9]
    assert not view.is_contiguous()
    kw = dict(pose_make_baseline_1=True, pose_make_relative=True)
    G = torch.randn(3, 4, 4, 4, generator=gen).cuda()
    a, b = view.clone().requires_grad_(True), wide.clone().requires_grad_(True)
    pa, pb = spf().process_pose(a, 2, **kw), spf().process_pose(b[..., :9], 2, **kw)
    assert torch.equal(pa, pb)
    pa.backward(G)
    pb.backward(G)
    assert torch.equal(a.grad, b.grad[..., :9]) and not bool(b.grad[..., 9:].any())
    with torch.no_grad():
        p = spf().process_pose(view.clone().requires_grad_(True), 2, **kw)
    assert p.grad_fn is None and not p.requires_grad and torch.equal(p, pa)
    # float64 / bfloat16 heads: float32 arithmetic and poses, gradients in the input's type
    for dt in (torch.float64, torch.bfloat16):
        x = view.to(dt).requires_grad_(True)
        p = spf().process_pose(x, 2, **kw)
        assert p.dtype == F32 and torch.equal(p, spf().process_pose(x.detach().float(), 2, **kw))
        p.backward(G)
        assert x.grad.dtype == dt


# ---- 2. depth --------------------------------------------------------------------------------------------------------
def _depth_inputs(gen, N, n):
    poses = O.process_pose(O.make_enc(gen, N, 1, 1, "rot6d").double(), 1, pose_make_baseline_1=False,
                           pose_make_relative=False)[:, 0].float()
    pts = torch.randn(N, n, 3, generator=gen) * 2 + torch.tensor([0.0, 0.0, 6.0])
    return pts, poses, torch.randn(N, n, 1, generator=gen)


def _oracle_depth(pts, poses, G, dtype):
    p, q = pts.to(dtype).requires_grad_(True), poses.to(dtype).requires_grad_(True)
    depth = O.depth_projector(p, q)
    return (depth.detach(), *torch.autograd.grad((depth * G.to(dtype)).sum(), [p, q]))


def _hold_depth(case, got, yard, truth):
    ed = err(got[0], truth[0])
    _log(case + "/depth", ed, err(yard[0], truth[0]))
    assert ed <= DEPTH_CAP, (case, ed)
    hold(case + "/d_pts3d", got[1], yard[1], truth[1], GRAD)
    hold(case + "/d_poses", got[2], yard[2], truth[2], GRAD)


@pytest.mark.parametrize("shape", [(2, 768), (2, 1026), (3, 1551), (1, 65536), (2049, 5)])
def test_depth_matches_the_oracle_and_a_strided_misaligned_view(hip_lib, shape):
    """(2049, 5): one slot per image, 2,049 slots on a grid capped at 2,048 (point_slots.h), so block 0 of the forward
    and of the backward takes a second trip of its slot loop."""
    N, n = shape
    gen = torch.Generator().manual_seed(N * 7 + n)
    pts, poses, G = _depth_inputs(gen, N, n)
    p, q = pts.cuda().requires_grad_(True), poses.cuda().requires_grad_(True)
    depth = spf().depth_projector(p, q)
    assert depth.shape == (N, n, 1) and depth.dtype == F32
    gp, gq = torch.autograd.grad(depth, [p, q], G.cuda())
    _hold_depth(f"depth/{N}x{n}", (depth, gp, gq), _oracle_depth(pts, poses, G, F32), _oracle_depth(pts, poses, G, F64))
    # the same points as a view with an image stride, starting 4 bytes past a 16-byte boundary: the same bits
    stride = 3 * n + 5
    buf = torch.zeros(N * stride + 1, device="cuda")
    view = buf[1:].as_strided((N, n, 3), (stride, 3, 1))
    view.copy_(pts)
    assert view.data_ptr() % 16 == 4 and not view.is_contiguous() or N == 1
    v = view.detach().requires_grad_(True)
    q2 = poses.cuda().requires_grad_(True)
    d2 = spf().depth_projector(v, q2)
    gv, gq2 = torch.autograd.grad(d2, [v, q2], G.cuda())
    assert torch.equal(d2, depth) and torch.equal(gv, gp) and torch.equal(gq2, gq)
    # one gradient at a time
    (only_q,) = torch.autograd.grad(spf().depth_projector(pts.cuda(), q2), [q2], G.cuda())
    (only_p,) = torch.autograd.grad(spf().depth_projector(v, poses.cuda()), [v], G.cuda())
    assert torch.equal(only_q, gq) and torch.equal(only_p, gp)


@pytest.mark.parametrize("name", list(GOLD["depth"]))
def test_depth_matches_the_reference_goldens(hip_lib, name):
    g = GOLD["depth"][name]
    N, n, _ = g["pts3d"].shape
    h = 3 if n % 3 == 0 else 1
    p, q = g["pts3d"].cuda().requires_grad_(True), g["poses"].cuda().requires_grad_(True)
    depth = spf().process_depth(q[None], p.reshape(1, N, h, n // h, 3))          # through process_depth: [b, v, h, w]
    assert depth.shape == (1, N, h, n // h)
    gp, gq = torch.autograd.grad(depth, [p, q], g["upstream"].cuda().reshape(depth.shape))
    _hold_depth(f"depth_golden/{name}", (depth.reshape(N, n, 1), gp, gq), (g["depth"], g["grad_pts3d"], g["grad_poses"]),
                _oracle_depth(g["pts3d"], g["poses"], g["upstream"], F64))


# ---- 3. pose errors --------------------------------------------------------------------------------------------------
def _hold_errors(case, got, truth):
    got = got.cpu().double()
    ea = float((got[..., [0, 2]] - truth[..., [0, 2]]).abs().max())
    es = float(((got[..., 1] - truth[..., 1]).abs() / truth[..., 1].abs().clamp_min(1e-30)).max()) \
        if bool(truth[..., 1].any()) else float(got[..., 1].abs().max())
    _log(case, {"angles_deg": ea, "scale_rel": es}, None)
    assert ea <= ANGLE_CAP and es <= SCALE_CAP, (case, ea, es)


@pytest.mark.parametrize("shape", [(), (7,), (60, 5)])
def test_pose_errors_match_the_float64_oracle(hip_lib, shape):
    N = math.prod(shape)
    gen = torch.Generator().manual_seed(40 + N)
    pred, tgt = (t.reshape(*shape, 4, 4) for t in O.make_pose_pairs(gen, N))
    truth = O.pose_errors(pred.double(), tgt.double())
    e = spf().pose_errors(pred.cuda(), tgt.cuda())
    assert e.shape == (N, 3) and e.dtype == F32 and e.is_cuda
    _hold_errors(f"errors/N{N}/per_pose", e, truth)
    ang, trans = spf().compute_pose_error_for_batch(pred.cuda(), tgt.cuda())
    assert ang.shape == () and ang.is_cuda and ang.dtype == F32
    _hold_errors(f"errors/N{N}/means", torch.stack([trans, trans.new_zeros(()), ang]), torch.stack(
        [truth[:, 0].mean(), truth.new_zeros(()), truth[:, 2].mean()]))
    one = spf().compute_pose_error(tgt.reshape(-1, 4, 4)[0].cuda(), pred.reshape(-1, 4, 4)[0].cuda())
    assert len(one) == 3 and all(x.shape == () and x.is_cuda for x in one)
    _hold_errors(f"errors/N{N}/compute_pose_error", torch.stack(one), truth[0])


def test_pose_error_goldens_and_edge_cases(hip_lib):
    g = GOLD["errors"]["parity"]
    e = spf().pose_errors(g["pred"].cuda(), g["tgt"].cuda())
    _hold_errors("errors_golden/parity", e, O.pose_errors(g["pred"].double(), g["tgt"].double()))
    # the reference's float32 run itself is good to 2e-3 degrees on these angles (tests/test_pose.py)
    assert float((e.cpu()[:, [0, 2]] - g["per_pose"][:, [0, 2]]).abs().max()) <= 2e-3
    g = GOLD["errors"]["edges"]         # identical poses; a 180 degree rotation; zero translation
    e = spf().pose_errors(g["pred"].cuda(), g["tgt"].cuda())
    _hold_errors("errors_golden/edges", e, O.pose_errors(g["pred"].double(), g["tgt"].double()))
    e = e.cpu()
    assert float(e[0].abs().max()) <= 0.03 and abs(float(e[1, 2]) - 180) <= 0.03 and float(e[1, :2].abs().max()) <= 0.03
    assert float(e[2, 0]) == 90.0 and float(e[2, 1]) == pytest.approx(float(g["per_pose"][2, 1]), rel=1e-6)


# ---- 4. focal --------------------------------------------------------------------------------------------------------
def _hold_focal(case, got, yard, truth):
    ep, ey = err(got, truth), err(yard, truth)
    _log(case, ep, ey)
    assert ep <= FOCAL_CAP, (case, ep, ey)


@pytest.mark.parametrize("name", ["24x32", "33x47", "64x64", "24x32_pp"])
def test_focal_matches_the_reference_goldens(hip_lib, name):
    g = GOLD["focal"][name]
    pp = g.get("pp")
    f = spf().estimate_focal_knowing_depth(g["pts3d"].cuda(), pp=None if pp is None else pp.cuda())
    assert f.shape == (2,) and f.dtype == F32 and f.is_cuda
    truth = O.estimate_focal_knowing_depth(g["pts3d"].double(), None if pp is None else pp.double())
    _hold_focal(f"focal_golden/{name}", f, g["focal"], truth)
    if pp is not None:                                       # one pair per scene reads the same
        f2 = spf().estimate_focal_knowing_depth(g["pts3d"].cuda(), pp=pp.cuda().expand(2, 2))
        assert torch.equal(f, f2)


def test_focal_256_view0_in_place_and_the_3x3(hip_lib):
    gen = torch.Generator().manual_seed(77)
    h = w = 256
    scenes = torch.stack([O.focal_scene(gen, h, w, 230.0), O.focal_scene(gen, h, w, 180.0)])
    views = torch.randn(2, 3, h, w, 3, generator=gen)
    views[:, 0] = scenes
    dev = views.cuda()
    f = spf().estimate_focal_knowing_depth(dev[:, 0])                                 # a strided view, read in place
    assert not dev[:, 0].is_contiguous() and torch.equal(f, spf().estimate_focal_knowing_depth(scenes.cuda()))
    _hold_focal("focal/256x256", f, O.estimate_focal_knowing_depth(scenes), O.estimate_focal_knowing_depth(scenes.double()))
    K = spf().estimate_intrinsics(dev, h, w)
    assert K.shape == (2, 3, 3) and K.dtype == F32
    assert torch.equal(K, O.intrinsics_from_focal(f.cpu(), h, w).cuda())
    # a misaligned start and a row stride: the same bits
    buf = torch.zeros(2 * h * (3 * w + 7) + 1, device="cuda")
    view = buf[1:].as_strided((2, h, w, 3), (h * (3 * w + 7), 3 * w + 7, 3, 1))
    view.copy_(scenes)
    assert torch.equal(f, spf().estimate_focal_knowing_depth(view))


def test_intrinsics_golden_uses_view_0_and_the_reference_row_divisors(hip_lib):
    g = GOLD["focal"]["intrinsics_24x32"]
    K = spf().estimate_intrinsics(g["pts3d"].cuda(), 24, 32).cpu()
    truth = O.estimate_intrinsics(g["pts3d"].double(), 24, 32)
    _hold_focal("focal_golden/intrinsics_24x32", K, g["intrinsics"], truth)
    f = spf().estimate_focal_knowing_depth(g["pts3d"][:, 0].cuda()).cpu()
    assert torch.equal(K[:, 0, 0], f / 24) and torch.equal(K[:, 1, 1], f / 32)
    assert torch.equal(K[:, 0, 2], torch.full((2,), 16.0) / 24) and torch.equal(K[:, 1, 2], torch.full((2,), 12.0) / 32)
    assert torch.equal(K[:, 2], torch.tensor([0.0, 0.0, 1.0]).expand(2, 3)) and not bool(K[:, 0, 1].any() or K[:, 1, 0].any())


def test_focal_edge_cases(hip_lib):
    edges = O.focal_edges()
    batch = torch.cat([edges[k][0] for k in ("none_valid", "mirrored", "exact_odd_points")])
    f = spf().estimate_focal_knowing_depth(batch.cuda()).cpu()
    _log("focal/edges", f.tolist(), [GOLD["focal"]["edge_" + k]["focal"].item() for k in
                                      ("none_valid", "mirrored", "exact_odd_points")])
    assert math.isnan(float(f[0]))                                                    # no valid point
    assert float(f[1]) == pytest.approx(O.focal_base(12, 16), rel=1e-6)                # initial focal -10 -> focal_base
    assert float(f[2]) == pytest.approx(10.0, rel=1e-6)              # subnormal z, an all-zero point, NaN z
    for i, k in enumerate(("mirrored", "exact_odd_points")):
        assert float(f[i + 1]) == pytest.approx(float(GOLD["focal"]["edge_" + k]["focal"]), rel=1e-6)
    # clipping: min_focal above the estimate, max_focal below it
    pts = GOLD["focal"]["24x32"]["pts3d"].cuda()
    base = O.focal_base(24, 32)
    lo = spf().estimate_focal_knowing_depth(pts, min_focal=2.0)
    hi = spf().estimate_focal_knowing_depth(pts, max_focal=0.25)
    assert lo.cpu().tolist() == pytest.approx([2 * base] * 2, rel=1e-6) and hi.cpu().tolist() == pytest.approx([base / 4] * 2, rel=1e-6)


# ---- 5. repeatability and no host sync -------------------------------------------------------------------------------
def _whole_step(enc, G, pts, gt):
    s = spf()
    e = enc.clone().requires_grad_(True)
    poses = s.process_pose(e, 2, pose_make_baseline_1=True, pose_make_relative=True)
    poses.backward(G)
    p, q = pts.clone().requires_grad_(True), poses.detach().clone().requires_grad_(True)
    depth = s.process_depth(q, p)
    depth.backward(torch.ones_like(depth))
    ang, trans = s.compute_pose_error_for_batch(poses.detach(), gt)
    K = s.estimate_intrinsics(pts, pts.shape[2], pts.shape[3])
    f = s.estimate_focal_knowing_depth(pts[:, 0])
    return poses.detach(), e.grad, depth.detach(), p.grad, q.grad, ang, trans, s.pose_errors(poses.detach(), gt), K, f


def _step_inputs():
    gen = torch.Generator().manual_seed(12)
    b, v, h, w = 3, 3, 33, 47
    enc = O.make_enc(gen, b, v, 2, "rot6d").cuda()
    G = torch.randn(b, v, 4, 4, generator=gen).cuda()
    pts = torch.stack([torch.stack([O.focal_scene(gen, h, w, 40.0) for _ in range(v)]) for _ in range(b)]).cuda()
    gt = O.process_pose(O.make_enc(gen, b, v, 2, "rot6d"), 2, pose_make_baseline_1=True, pose_make_relative=True).cuda()
    return enc, G, pts, gt


def test_two_runs_are_bitwise_equal(hip_lib):
    args = _step_inputs()
    first, second = _whole_step(*args), _whole_step(*args)
    for a, b in zip(first, second):
        assert torch.equal(a, b) or (bool(torch.isnan(a).any()) and torch.equal(a.isnan(), b.isnan()))
    enc = O.make_enc(torch.Generator().manual_seed(2), 4, 3, 2, "absT_quaR_FoV")
    G = torch.randn(4, 3, 4, 4, generator=torch.Generator().manual_seed(3))
    one, two = (product_compose(enc, 2, "absT_quaR_FoV", True, True, G) for _ in range(2))
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


def test_the_pose_step_never_syncs(hip_lib):
    args = _step_inputs()
    want = _whole_step(*args)                       # also loads the library before the mode is set
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _whole_step(*args)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(a, b) for a, b in zip(want, got))
