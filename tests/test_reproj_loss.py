"""Reprojection loss (LossReproj): the float64 oracle (tests/reproj_oracle.py) pinned by vectors captured from the
reference's own LossReproj (tests/golden/make_reproj_goldens.py), the module surface and argument checks without a GPU,
and the HIP kernels (spfsplatv2_amd/csrc/reproj.hip) against both on the GPU.

Tolerances: loss 1e-5 relative; dL/dpts3d per point, 1e-4 of the point's own gradient (widened for float32 reasons
written at _check_grads and px_allowance); pose and intrinsics gradients 1e-4 relative in Frobenius norm per image.
Gradients are compared outside the knife-edge mask (reproj_oracle.knife_edge: points whose float64 error lies within
1e-3 px of 0 or within 1e-5 relative of a clamp), which must cover < 0.1 % of the points at the larger shapes."""
import ctypes as C
import math
from pathlib import Path

import pytest
import torch

from tests import reproj_oracle as ro

GOLD = torch.load(Path(__file__).parent / "golden" / "reproj_goldens.pt")
# (b33_grid_stride: 33 x 64 = 2,112 slots, more than the 2,048-block grid -- blocks loop over several slots)
SHAPES = {"re10k": (16, 2, 256, 256), "re10k_10view": (3, 10, 256, 256), "b33_grid_stride": (33, 1, 256, 256),
          "slot_plus_2": (2, 2, 27, 38)}     # 1026 points: a full slot, then a slot that holds two points


def _rel(a, b):
    a, b = float(a), float(b)
    if math.isnan(b):
        return 0.0 if math.isnan(a) else math.inf
    return abs(a - b) / max(abs(b), 1e-30)


def px_allowance(e, h, w):
    """Extra relative error allowed on point i's dL/dpts3d: float32 carries the projected pixel coordinate to about
    16 ulp of the image's extent, eps_px = 16 * 2^-24 * (h + w) px (the product and the reference alike), and the
    gradient's direction (px - target) / e then only to eps_px / e -- a 1e-2 px error is good to ~1e-3.  That is the
    float32 reason the 1e-4-of-max bound is widened by max_c |want_ic| * eps_px / e_i on every component c of point i
    (a direction error moves all three components by the point's gradient size, not by each component's own)."""
    return 16 * 2.0 ** -24 * (h + w) / e.clamp_min(1e-30)


def _check_grads(got, want, keep, what, allow=None):
    """got / want: (dL/dpts3d [b,h,w,3], dL/dposes [b,4,4], dL/dintrinsics [b,3,3]); keep [b,h,w] = points outside the
    knife-edge mask; allow [b,h,w]: the float32 direction allowance (px_allowance).

    Every point on its own scale, so that no point's gradient hides behind another's: component c of point i in image b
    must satisfy |got - want| <= (1e-4 + allow_i) m_i + 1e-6 M_b, with m_i = max_c |want_ic| the point's own gradient
    and M_b the largest entry of image b.  (The 1e-6 M_b floor is float32's: 1 - tanh^2 near tanh = 1 cancels to ~1e-7
    absolute in the product and the reference alike; an invalid point's want is 0 and it gets only that floor.)  Pose and
    intrinsics gradients: 1e-4 relative in Frobenius norm per image.  Non-finite entries (NaN loss) must sit at the same
    places; the finite ones are compared as above."""
    gp, gpo, gk = (t.detach().double().cpu() for t in got)
    wp, wpo, wk = (t.detach().double().cpu() for t in want)
    for name, g, w in (("dpts3d", gp, wp), ("dposes", gpo, wpo), ("dintrinsics", gk, wk)):
        assert torch.equal(torch.isnan(g), torch.isnan(w)), (what, name, "NaN pattern")
        assert torch.equal(torch.isinf(g), torch.isinf(w)), (what, name, "inf pattern")
    fin = torch.isfinite(wp)
    gp, wp = torch.where(fin, gp, 0.0), torch.where(fin, wp, 0.0)
    m = wp.abs().amax(-1, keepdim=True)
    big = wp.flatten(1).abs().amax(1).view(-1, *([1] * (wp.dim() - 1)))
    tol = ((1e-4 + (0.0 if allow is None else allow[..., None].double())) * m + 1e-6 * big).expand_as(wp)
    bad = ((gp - wp).abs() > tol) & keep[..., None] & fin
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError((what, "dpts3d", int(bad.sum()), "first at", i, float(gp.flatten()[i]), float(wp.flatten()[i]),
                              float(tol.flatten()[i])))
    for name, g, w in (("dposes", gpo, wpo), ("dintrinsics", gk, wk)):
        ok = torch.isfinite(w).flatten(1).all(1)
        for b in range(w.shape[0]):
            if ok[b]:
                n, d = float(w[b].norm()), float((g[b] - w[b]).norm())
                assert d <= 1e-4 * n, (what, name, "image", b, d, n)


def _oracle(g):
    return ro.reproj_ref(g["pts3d"], g["poses"], g["intrinsics"], weight=g["weight"], mode=g["mode"],
                         global_step=g["global_step"], total_iterations=g["total_iterations"],
                         circle_schedule=g["circle_schedule"], detach_pts3d=g["detach_pts3d"])


# ---- CPU ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GOLD))
def test_oracle_matches_reference_goldens(name):
    g = GOLD[name]
    loss, dp, dpo, dk, e = _oracle(g)
    assert _rel(loss, g["loss"]) < 1e-5, (float(loss), float(g["loss"]))
    keep = ~ro.knife_edge(e)
    assert int((~keep).sum()) <= 2                          # (tiny cases: bounded by count)
    if float(g["loss"]) == 0.0 and g["loss_is_int"]:
        assert float(dp.abs().max()) == 0 and float(dpo.abs().max()) == 0 and float(dk.abs().max()) == 0
    _check_grads((dp, dpo, dk), (g["grad_pts3d"], g["grad_poses"], g["grad_intrinsics"]), keep, name,
                 px_allowance(e, *e.shape[-2:]))


def test_goldens_cover_the_contract():
    modes = {g["mode"] for g in GOLD.values()}
    assert {"tanh", "dyntanh", "l1", "l1+sqrt", "l1+logl1"} <= modes and modes - {"tanh", "dyntanh", "l1", "l1+sqrt",
                                                                                   "l1+logl1"}
    assert any(g["loss_is_int"] for g in GOLD.values())
    assert any(math.isnan(float(g["loss"])) for g in GOLD.values())
    assert any(g["detach_pts3d"] for g in GOLD.values())
    assert any(g["pts3d"].shape[1:3] == (17, 13) for g in GOLD.values())
    e = ro.errors(GOLD["l1_mixed"]["pts3d"].double(), GOLD["l1_mixed"]["poses"].double(),
                  GOLD["l1_mixed"]["intrinsics"].double())
    assert bool(((e > 40) & (e < 50)).any() and ((e > 50) & (e < 60)).any())
    assert bool(((e > 900) & (e < 1000)).any() and ((e > 1000) & (e < 1100)).any())


def test_module_surface_and_name():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import loss as L
    assert spf.LossReproj is L.LossReproj and spf.reproj_loss is L.reproj_loss
    cfg = L.LossReprojCfg(weight=0.001, mode="dyntanh", circle_schedule=True, total_iterations=200_001)
    m = L.LossReproj(L.LossReprojCfgWrapper(reproj=cfg))
    assert m.name == "reproj" and m.cfg is cfg and len(list(m.parameters())) == 0
    assert (m.repro_loss_hard_clamp, m.soft_clamp, m.soft_clamp_min) == (1000, 50, 1)


@pytest.mark.parametrize("mode,step,circle", [("dyntanh", 0, True), ("dyntanh", 100_000, True),
                                              ("dyntanh", 100_000, False), ("dyntanh", 200_001, True),
                                              ("dyntanh", 250_000, True), ("dyntanh", 250_000, False),
                                              ("tanh", 7, True), ("l1", 7, True)])
def test_schedule_weight(mode, step, circle):
    """lw in float64 on the host, as loss_reproj.py:117-133 computes it (np.sqrt of a negative: NaN)."""
    import numpy as np

    from spfsplatv2_amd.loss import reproj_lw
    got = reproj_lw(mode, step, 200_001, circle, 50, 1)
    if mode == "tanh":
        want = 50.0
    elif mode != "dyntanh":
        want = 1.0
    else:
        s = step / 200_001
        if circle:
            with np.errstate(invalid="ignore"):
                s = 1 - np.sqrt(1 - s ** 2)
        want = float((1 - s) * 50 + 1)
    assert (math.isnan(got) and math.isnan(want)) or got == want, (got, want)


def test_cpu_tensors_are_refused():
    from spfsplatv2_amd import loss as L
    g = GOLD["tanh_mixed"]
    m = L.LossReproj(L.LossReprojCfgWrapper(L.LossReprojCfg(1.0, "tanh", True, 10)))
    with pytest.raises(RuntimeError, match="no CPU"):
        m(g["pts3d"], g["poses"], g["intrinsics"], 0)
    with pytest.raises(RuntimeError, match="do not match"):
        L.reproj_loss(g["pts3d"], g["poses"][:1], g["intrinsics"], weight=1.0, mode="tanh", global_step=0,
                      total_iterations=10, circle_schedule=True)


def test_c_abi_rejects_bad_arguments(hip_lib):
    from spfsplatv2_amd import _lib
    assert hip_lib.spf_reproj_partial_blocks(16, 2, 256, 256) == 16 * 2 * 64
    assert hip_lib.spf_reproj_partial_blocks(3, 10, 17, 13) == 30
    assert hip_lib.spf_reproj_partial_blocks(0, 1, 4, 4) == -1
    p = C.c_void_p(256)                   # never dereferenced: every rejection happens before a launch

    def args(**kw):
        a = dict(pts3d=p, stride_b=48, stride_v=48, poses=p, intrinsics=p, B=1, V=1, H=4, W=4, mode=0, weight=1.0,
                 lw=50.0, hard_clamp=1000.0, soft_clamp=50.0)
        a.update(kw)
        return _lib.SpfReproj(**a)

    fwd = hip_lib.spf_reproj_forward
    bwd = hip_lib.spf_reproj_backward
    for kw, msg in (({"pts3d": None}, b"null"), ({"B": 0}, b"positive"), ({"H": -1}, b"positive"),
                    ({"mode": 4}, b"mode"), ({"mode": -1}, b"mode"), ({"stride_v": -48}, b"negative"),
                    ({"H": 40000, "W": 40000}, b"too large"), ({"poses": C.c_void_p(258)}, b"aligned")):
        assert fwd(C.byref(args(**kw)), p, p, p, None) == -1, kw
        assert msg in hip_lib.spf_last_error(), (kw, hip_lib.spf_last_error())
    assert fwd(None, p, p, p, None) == -1 and b"null" in hip_lib.spf_last_error()
    assert fwd(C.byref(args()), None, p, p, None) == -1 and b"null" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, None, None, None, None, None) == -1
    assert b"no gradient" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, p, None, p, None, None) == -1 and b"gpartial" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, p, p, None, None, None) == -1 and b"gpartial" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, None, C.c_void_p(264), p, None, None) == -1
    assert b"16-byte" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), None, p, p, None, None, None, None) == -1 and b"null" in hip_lib.spf_last_error()


# ---- GPU ---------------------------------------------------------------------------------------------------------

def _hip(g, dev="cuda", **over):
    from spfsplatv2_amd import loss as L
    p = g["pts3d"].to(dev).requires_grad_(True)
    po = g["poses"].to(dev).requires_grad_(True)
    k = g["intrinsics"].to(dev).requires_grad_(True)
    m = L.LossReproj(L.LossReprojCfgWrapper(L.LossReprojCfg(g["weight"], g["mode"], g["circle_schedule"],
                                                            g["total_iterations"])))
    loss = m(p, po, k, g["global_step"], detach_pts3d=g["detach_pts3d"])
    return loss, p, po, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GOLD))
def test_hip_matches_reference_goldens(hip_lib, name):
    g = GOLD[name]
    loss, p, po, k = _hip(g)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    assert _rel(loss.detach().cpu(), g["loss"]) < 1e-5, (float(loss), float(g["loss"]))
    (2.0 * loss).backward()                                  # the upstream scalar is read on the device
    if g["detach_pts3d"]:
        assert p.grad is None
    dp = p.grad if p.grad is not None else torch.zeros_like(p)
    got = (dp / 2, po.grad / 2, k.grad / 2)
    if g["loss_is_int"]:                                     # no valid point: 0 and exact zero gradients, not NaN
        assert float(loss) == 0.0
        assert all(float(t.abs().max()) == 0.0 for t in got)
        return
    loss64, dp64, dpo64, dk64, e = _oracle(g)
    keep, allow = ~ro.knife_edge(e), px_allowance(e, *e.shape[-2:])
    # against the float32 reference, and against the float64 oracle on the same inputs
    _check_grads(got, (g["grad_pts3d"], g["grad_poses"], g["grad_intrinsics"]), keep, name, allow)
    _check_grads(got, (dp64, dpo64, dk64), keep, name, allow)
    assert _rel(loss.detach().cpu(), loss64) < 1e-5


def _pixel_aligned_5d(seed, b, v, h, w):
    gen = torch.Generator().manual_seed(seed)
    pts, poses, ks = [], [], []
    for _ in range(v):
        p, po, k = ro.pixel_aligned(gen, b, h, w)
        pts.append(p)
        poses.append(po)
        ks.append(k)
    return torch.stack(pts, 1), torch.stack(poses, 1), torch.stack(ks, 1)


def _batched(pts, poses, ks, mode="dyntanh", step=30_000, **kw):
    from spfsplatv2_amd import loss as L
    return L.reproj_loss(pts, poses, ks, weight=kw.pop("weight", 0.001), mode=mode, global_step=step,
                         total_iterations=200_001, circle_schedule=True, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,mode", [("re10k", "dyntanh"), ("re10k", "l1+sqrt"), ("re10k_10view", "dyntanh"),
                                        ("re10k_10view", "l1+sqrt"), ("b33_grid_stride", "dyntanh"),
                                        ("slot_plus_2", "dyntanh")])
def test_hip_matches_oracle_at_full_shape(hip_lib, shape, mode):
    b, v, h, w = SHAPES[shape]
    pts, poses, ks = _pixel_aligned_5d(5, b, v, h, w)
    p, po, k = (t.cuda().requires_grad_(True) for t in (pts, poses, ks))
    loss = _batched(p, po, k, mode=mode)
    assert loss.shape == (v,)
    up = torch.linspace(0.5, 1.5, v, device="cuda")
    (loss * up).sum().backward()
    mask_share = []
    for i in range(v):
        ref = ro.reproj_ref(pts[:, i], poses[:, i], ks[:, i], weight=0.001, mode=mode, global_step=30_000,
                            total_iterations=200_001, circle_schedule=True)
        assert _rel(loss[i].cpu(), ref[0]) < 1e-5, (i, float(loss[i]), float(ref[0]))
        knife = ro.knife_edge(ref[4])
        mask_share.append(float(knife.double().mean()))
        u = float(up[i])
        _check_grads((p.grad[:, i] / u, po.grad[:, i] / u, k.grad[:, i] / u), ref[1:4], ~knife, (shape, mode, i),
                     px_allowance(ref[4], h, w))
    assert max(mask_share) < 1e-3, mask_share


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tanh", "dyntanh", "l1", "l1+sqrt", "l1+logl1"])
def test_hip_matches_oracle_odd_misaligned_shape_per_point(hip_lib, mode):
    """33 x 47 images (3 H W floats odd: every other image starts unaligned, and 1,551 points leave a tail of 3) with
    errors on both sides of soft_clamp and hard_clamp: the scalar loads and stores, every branch of every term and the
    invalid points, compared point by point against the oracle -- batched, and per view on the strided pts3d[:, 1]."""
    b, v, h, w = 3, 2, 33, 47
    gen = torch.Generator().manual_seed(31)
    views = [ro.controlled_points(gen, b, h, w, "mixed") for _ in range(v)]
    pts, poses, ks = (torch.stack([x[j] for x in views], 1) for j in range(3))
    refs = [ro.reproj_ref(pts[:, i], poses[:, i], ks[:, i], weight=0.5, mode=mode, global_step=30_000,
                          total_iterations=200_001, circle_schedule=True) for i in range(v)]
    for i in range(v):
        e = refs[i][4]
        assert bool(((e > 40) & (e < 50)).any() and ((e > 50) & (e < 60)).any() and (e > 1000).any())
        assert float(ro.knife_edge(e).double().mean()) < 1e-3
    p, po, k = (t.cuda().requires_grad_(True) for t in (pts, poses, ks))
    loss = _batched(p, po, k, mode=mode, weight=0.5)
    loss.sum().backward()
    for i in range(v):
        loss64, dp, dpo, dk, e = refs[i]
        assert _rel(loss[i].detach().cpu(), loss64) < 1e-5, (mode, i, float(loss[i]), float(loss64))
        _check_grads((p.grad[:, i], po.grad[:, i], k.grad[:, i]), (dp, dpo, dk), ~ro.knife_edge(e), (mode, "batched", i),
                     px_allowance(e, h, w))
    # view 1 alone: read through the batch stride, its gradient written as its own [b,h,w,3] (image b at b * 4,653 floats)
    p2, po2, k2 = (t.cuda().requires_grad_(True) for t in (pts, poses, ks))
    one = _batched(p2[:, 1], po2[:, 1], k2[:, 1], mode=mode, weight=0.5)
    one.backward()
    assert torch.equal(one.detach(), loss[1].detach())
    assert torch.equal(p2.grad[:, 1], p.grad[:, 1]) and torch.equal(po2.grad[:, 1], po.grad[:, 1])


@pytest.mark.gpu
def test_batched_equals_per_view_loop_bitwise_and_runs_repeat(hip_lib):
    b, v, h, w = 3, 4, 64, 80
    pts, poses, ks = (t.cuda() for t in _pixel_aligned_5d(7, b, v, h, w))
    up = torch.linspace(0.25, 2.0, v, device="cuda")

    def batched():
        p, po, k = (t.clone().requires_grad_(True) for t in (pts, poses, ks))
        loss = _batched(p, po, k)
        (loss * up).sum().backward()
        return loss.detach(), p.grad, po.grad, k.grad

    def loop():
        p, po, k = (t.clone().requires_grad_(True) for t in (pts, poses, ks))
        ls = [_batched(p[:, i], po[:, i], k[:, i]) for i in range(v)]
        sum(li * up[i] for i, li in enumerate(ls)).backward()
        return torch.stack([li.detach() for li in ls]), p.grad, po.grad, k.grad

    a, a2, c = batched(), batched(), loop()
    for x, y, z in zip(a, a2, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.gpu
def test_strided_view_equals_contiguous_copy(hip_lib):
    """pts3d[:, i] of the encoder's [b,v,h,w,3] is read in place (odd sizes: images start unaligned -> scalar loads)."""
    b, v, h, w = 2, 3, 33, 47
    pts, poses, ks = (t.cuda() for t in _pixel_aligned_5d(9, b, v, h, w))
    for i in range(v):
        p1 = pts.clone().requires_grad_(True)
        assert not p1[:, i].is_contiguous()
        l1 = _batched(p1[:, i], poses[:, i], ks[:, i])
        l1.backward()
        p2 = pts[:, i].contiguous().requires_grad_(True)
        l2 = _batched(p2, poses[:, i], ks[:, i])
        l2.backward()
        assert torch.equal(l1, l2) and torch.equal(p1.grad[:, i], p2.grad), i


@pytest.mark.gpu
def test_no_valid_point_gives_zero_loss_and_zero_gradients(hip_lib):
    g = GOLD["none_valid"]
    pts = g["pts3d"].cuda()[:, None].expand(-1, 2, -1, -1, -1).contiguous().requires_grad_(True)
    poses = g["poses"].cuda()[:, None].expand(-1, 2, -1, -1).contiguous().requires_grad_(True)
    ks = g["intrinsics"].cuda()[:, None].expand(-1, 2, -1, -1).contiguous().requires_grad_(True)
    for mode in ("tanh", "dyntanh", "l1", "l1+sqrt", "l1+logl1"):
        for t in (pts, poses, ks):
            t.grad = None
        loss = _batched(pts, poses, ks, mode=mode)
        loss.sum().backward()
        assert torch.equal(loss, torch.zeros_like(loss)), mode
        for t in (pts.grad, poses.grad, ks.grad):
            assert torch.equal(t, torch.zeros_like(t)), mode


@pytest.mark.gpu
def test_forward_backward_never_syncs(hip_lib):
    b, v, h, w = 2, 3, 64, 64
    pts, poses, ks = (t.cuda() for t in _pixel_aligned_5d(11, b, v, h, w))

    def go():
        p, po, k = (t.clone().requires_grad_(True) for t in (pts, poses, ks))
        loss = _batched(p, po, k)
        (loss[0] + loss[1:].sum() / (v - 1)).backward()
        single = _batched(p[:, 0], po[:, 0], k[:, 0])
        single.backward()
        return loss.detach(), p.grad
    want = go()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = go()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])


@pytest.mark.gpu
def test_low_precision_inputs_are_computed_in_float32(hip_lib):
    b, v, h, w = 2, 2, 16, 24
    pts, poses, ks = (t.cuda() for t in _pixel_aligned_5d(13, b, v, h, w))
    p = pts.double().requires_grad_(True)
    loss = _batched(p, poses.double(), ks.double())
    loss.sum().backward()
    assert loss.dtype == torch.float32 and p.grad.dtype == torch.float64
    want = _batched(pts, poses, ks)
    assert torch.equal(loss.detach(), want)
