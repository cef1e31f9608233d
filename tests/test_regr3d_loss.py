"""Distillation point loss (Regr3D): the float64 oracle (tests/regr3d_oracle.py) pinned by vectors captured from the
reference's own Regr3D (tests/golden/make_regr3d_goldens.py), the module surface and argument checks without a GPU, and
the HIP kernels (spfsplatv2_amd/csrc/regr3d.hip) against both on the GPU.

Gates.  Exact: n_valid equals the oracle's and gradients at invalid points are exactly 0 -- on inputs whose masks are
DECIDED (regr3d_oracle.decided: the order statistics either side of each of the four selected ranks of every row and
view are >= 1e-5 apart, relatively; no norm within 1e-5 of dist_clip), which every test asserts on the oracle before it
looks at the product.  Thresholds q: 1e-6 relative.  Loss: 1e-5 relative to the float64 oracle.  Gradient of every valid
point, per component: (1e-4 + c 2^-24 (|a| + |b|) / |d|) m_i + 1e-6 M_b with c = 8 (regr3d_oracle.grad_tolerance: a, b the
normalised prediction and target, d = a - b, m_i the point's own largest component, M_b the row's largest entry; the
second term is float32's, the direction d / |d| being good to eps (|a| + |b|) / |d| only).  NaN and inf patterns equal
the golden's.

The c the product needs (printed by the tests as `c_needed`), measured on an MI355X: 0 at every oracle shape and golden
-- all errors sit inside the 1e-4 term -- except 0.23 on the golden `pr_scaled_gt` (predictions 1e-4 from their
targets), where the reference's own float32 gradients need 0.23 as well.  Loss: within 3.6e-7 of the oracle."""
import ctypes as C
import functools
import math
from pathlib import Path

import pytest
import torch

from tests import regr3d_oracle as go

GOLD = torch.load(Path(__file__).parent / "golden" / "regr3d_goldens.pt")
INPUTS = ("gt_pts1", "gt_pts2", "pr_pts1", "pr_pts2", "conf1", "conf2")
C_PRODUCT = 8.0        # the gradient bound's float32 cancellation factor for the product
C_REFERENCE = 2.1      # what the reference's own float32 gradients needed against the oracle


def _rel(a, b):
    a, b = float(a), float(b)
    if math.isnan(b):
        return 0.0 if math.isnan(a) else math.inf
    return abs(a - b) / max(abs(b), 1e-30)


@functools.lru_cache(maxsize=None)
def _golden_case(name):
    g = GOLD[name]
    if "gt_pts1" in g:
        case = {k: g[k] for k in INPUTS}
        case.update({k: g[k] for k in ("seed", "dist_clip", "disable_view1", "norm_mode", "gt_scale")})
    else:
        case = go.make_case(g["seed"], *g["shape"], dist_clip=g["dist_clip"], disable_view1=g["disable_view1"],
                            norm_mode=g["norm_mode"], gt_scale=g["gt_scale"])
    return case, go.run_ref(case)


@functools.lru_cache(maxsize=None)
def _decided_case(B, H, W, start=0, opts=()):
    case = go.first_decided_case(B, H, W, start=start, **dict(opts))
    return case, go.run_ref(case)


def _check_grads(got, ref, c, what, scale=1.0):
    """got: (d_pr1, d_pr2); ref: the oracle's record.  Returns the c the gradients would have needed."""
    got = torch.stack([t.detach().double().cpu() for t in got]) / scale
    want = torch.stack(ref["grad"])
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN pattern")
    assert torch.equal(torch.isinf(got), torch.isinf(want)), (what, "inf pattern")
    valid = ref["valid"][..., None].expand_as(want)
    if bool((~valid).any()):
        assert float(got[~valid].abs().max()) == 0.0, (what, "a gradient at an invalid point is not exactly 0")
    err = (got - want).abs()
    tol = go.grad_tolerance(ref, c)
    # the c that would have been enough: err <= (1e-4 + c k) m + floor  ->  c >= ((err - floor) / m - 1e-4) / k
    base = go.grad_tolerance(ref, 0.0)
    per_c = (tol - base) / c
    need = ((err - base) / per_c.clamp_min(1e-300)).clamp_min(0.0)
    c_needed = float(need[valid].max()) if bool(valid.any()) else 0.0
    print(f"{what}: c_needed {c_needed:.3f}")
    bad = (err > tol) & valid
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError((what, int(bad.sum()), "first at", i, float(got.flatten()[i]), float(want.flatten()[i]),
                              float(tol.flatten()[i]), "c_needed", c_needed))
    return c_needed


# ---- CPU ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GOLD))
def test_oracle_matches_reference_goldens(name):
    g = GOLD[name]
    case, ref = _golden_case(name)
    assert _rel(ref["loss"], g["loss"]) < 1e-5, (float(ref["loss"]), float(g["loss"]))
    assert torch.equal(ref["n_valid"].to(torch.int32), g["n_valid"]), (ref["n_valid"], g["n_valid"])
    if "grad_pr1" in g:
        _check_grads((g["grad_pr1"], g["grad_pr2"]), ref, C_PRODUCT, name)


def test_goldens_cover_the_contract():
    shapes = {g["shape"] for g in GOLD.values()}
    assert (2, 17, 13) in shapes and (3, 3, 167) in shapes
    (l0, l1, lw), (h0, h1, hw) = go.selected_ranks(501)
    assert (l0, l1, lw, h0, h1, hw) == (1, 1, 0.0, 499, 499, 0.0)              # both ranks integers at n = 501
    assert any(g["dist_clip"] == 8.0 for g in GOLD.values())
    assert any(g["disable_view1"] for g in GOLD.values()) and any(g["gt_scale"] for g in GOLD.values())
    g = GOLD["conf1_all_low"]
    assert math.isnan(float(g["loss"])) and int(g["n_valid"][0].sum()) == 0 and bool((g["conf1"] < 3).all())
    assert bool(torch.isfinite(g["grad_pr1"]).all() and torch.isfinite(g["grad_pr2"]).all())
    assert float(g["grad_pr2"].abs().max()) > 0
    g = GOLD["row_none_valid"]
    assert g["n_valid"][:, 1].tolist() == [0, 0] and int(g["n_valid"].sum()) > 0
    assert float(g["grad_pr1"][1].abs().max()) == 0 and float(g["grad_pr2"][1].abs().max()) == 0
    g = GOLD["identical_gt_row"]
    assert bool((g["gt_pts1"][0] == g["gt_pts1"][0, 0, 0]).all()) and int(g["n_valid"][0, 0]) == 17 * 13
    _, ref = _golden_case("pr_scaled_gt")
    d = torch.linalg.vector_norm(ref["a"] - ref["b"], dim=-1)
    na = torch.linalg.vector_norm(ref["a"], dim=-1)
    assert int(((d < 2e-4 * na) & ref["valid"]).sum()) >= 4                     # d ~ 0 on a few valid points
    g, (_, ref) = GOLD["pr_equals_gt_no_norm"], _golden_case("pr_equals_gt_no_norm")
    zero = (torch.linalg.vector_norm(ref["a"] - ref["b"], dim=-1) == 0) & ref["valid"]
    assert g["norm_mode"] is None and int(zero.sum()) >= 4                      # d == 0: no gradient there
    assert float(torch.stack([g["grad_pr1"], g["grad_pr2"]])[zero].abs().max()) == 0
    assert sum("gt_pts1" not in g for g in GOLD.values()) >= 2                  # larger cases: seed and scalars only
    for name, g in GOLD.items():
        if "gt_pts1" not in g:
            assert go.decided(_golden_case(name)[0]), name


def test_module_surface_and_export_names():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import loss as L
    assert spf.Regr3D is L.Regr3D and spf.regr3d_loss is L.regr3d_loss
    assert "Regr3D" in spf.__all__ and "regr3d_loss" in spf.__all__
    m = L.Regr3D()
    assert isinstance(m, torch.nn.Module) and len(list(m.parameters())) == 0
    assert (m.norm_mode, m.alpha, m.gt_scale) == ("avg_dis", 0.2, False)
    m = L.Regr3D(norm_mode=None, alpha=1.0, gt_scale=True)
    assert (m.norm_mode, m.alpha, m.gt_scale) == (None, 1.0, True)
    import inspect
    assert list(inspect.signature(L.Regr3D.forward).parameters) == [
        "self", "gt_pts1", "gt_pts2", "pr_pts1", "pr_pts2", "conf1", "conf2", "dist_clip", "disable_view1"]


def test_other_norm_modes_raise():
    from spfsplatv2_amd import loss as L
    with pytest.raises(NotImplementedError, match="median_dis"):
        L.Regr3D(norm_mode="median_dis")
    g = GOLD["default_2x17x13"]
    with pytest.raises(NotImplementedError, match="avg_log1p"):
        L.regr3d_loss(*(g[k] for k in INPUTS), norm_mode="avg_log1p")


def test_cpu_tensors_and_bad_arguments_are_refused():
    from spfsplatv2_amd import loss as L
    g = GOLD["default_2x17x13"]
    t = [g[k] for k in INPUTS]
    with pytest.raises(RuntimeError, match="no CPU"):
        L.Regr3D()(*t)
    with pytest.raises(ValueError, match="requires grad"):
        L.regr3d_loss(t[0].clone().requires_grad_(True), *t[1:])
    with pytest.raises(ValueError, match="requires grad"):
        L.regr3d_loss(*t[:4], t[4].clone().requires_grad_(True), t[5])
    with pytest.raises(ValueError, match="conf1 and conf2"):
        L.regr3d_loss(*t[:4])


def _scratch_bytes(B, H, W):
    rows, nchunk = 2 * B, (H * W + 1023) // 1024
    words = rows * 4 * 2048 + rows * 8 + 5 * rows * nchunk + rows + 2
    return 4 * ((words + 3) // 4 * 4)


def test_c_abi_scratch_size_and_rejections(hip_lib):
    from spfsplatv2_amd import _lib
    for shape in ((2, 17, 13), (16, 256, 256), (3, 256, 256), (2, 96, 112)):
        assert hip_lib.spf_regr3d_scratch_bytes(*shape) == _scratch_bytes(*shape), shape
    assert hip_lib.spf_regr3d_scratch_bytes(0, 4, 4) == -1 and hip_lib.spf_regr3d_scratch_bytes(1, -4, 4) == -1
    assert hip_lib.spf_regr3d_scratch_bytes(1, 40000, 40000) == -1
    p = C.c_void_p(256)                   # never dereferenced: every rejection happens before a launch

    def args(**kw):
        a = dict(gt_pts1=p, gt_pts2=p, pr_pts1=p, pr_pts2=p, conf1=p, conf2=p, stride_gt1=48, stride_gt2=48,
                 stride_pr1=48, stride_pr2=48, B=1, H=4, W=4, has_dist_clip=0, dist_clip=0.0, disable_view1=0,
                 normalize=1, gt_scale=0)
        a.update(kw)
        return _lib.SpfRegr3d(**a)

    fwd, bwd = hip_lib.spf_regr3d_forward, hip_lib.spf_regr3d_backward
    for kw, msg in (({"gt_pts2": None}, b"null"), ({"pr_pts1": None}, b"null"), ({"conf2": None}, b"confidences"),
                    ({"B": 0}, b"positive"), ({"W": -1}, b"positive"), ({"H": 40000, "W": 40000}, b"too large"),
                    ({"stride_pr2": -48}, b"negative"), ({"pr_pts2": C.c_void_p(258)}, b"aligned"),
                    ({"has_dist_clip": 1, "dist_clip": math.nan}, b"NaN")):
        assert fwd(C.byref(args(**kw)), p, p, p, None) == -1, kw
        assert msg in hip_lib.spf_last_error(), (kw, hip_lib.spf_last_error())
        assert bwd(C.byref(args(**kw)), p, p, p, p, p, None) == -1, kw
    assert fwd(None, p, p, p, None) == -1 and b"null" in hip_lib.spf_last_error()
    assert fwd(C.byref(args()), None, p, p, None) == -1 and b"null" in hip_lib.spf_last_error()
    assert fwd(C.byref(args()), C.c_void_p(264), p, p, None) == -1 and b"16-byte" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, p, None, None, None) == -1 and b"no gradient" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, None, p, p, None) == -1 and b"null" in hip_lib.spf_last_error()
    assert C.sizeof(_lib.SpfRegr3d) == 6 * 8 + 4 * 8 + 8 * 4


# ---- GPU ---------------------------------------------------------------------------------------------------------

def _hip(case, dev="cuda", grads=(True, True), upstream=None, **over):
    from spfsplatv2_amd import loss as L
    t = {k: over[k] if k in over else case[k].to(dev) for k in INPUTS}
    for k, need in zip(("pr_pts1", "pr_pts2"), grads):
        t[k] = t[k].detach().requires_grad_(need)
    loss, stats = L.regr3d_loss(*(t[k] for k in INPUTS), dist_clip=case["dist_clip"],
                                disable_view1=case["disable_view1"], norm_mode=case["norm_mode"],
                                gt_scale=case["gt_scale"], return_stats=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
    if any(grads):
        (loss if upstream is None else loss * upstream).backward()
    z = lambda p: p.grad if p.grad is not None else torch.zeros_like(p)          # noqa: E731
    return loss.detach(), stats, (z(t["pr_pts1"]), z(t["pr_pts2"]))


def _check_against_oracle(case, ref, what, scale=1.0, **kw):
    loss, stats, grads = _hip(case, **kw)
    assert torch.equal(stats["n_valid"].cpu().long(), ref["n_valid"]), (what, stats["n_valid"], ref["n_valid"])
    q, q64 = stats["q"].cpu().double(), ref["q"]
    assert bool(((q - q64).abs() <= 1e-6 * q64.abs()).all()), (what, q, q64)
    for key in ("nf_pr", "nf_gt"):
        assert bool(((stats[key].cpu().double() - ref[key]).abs() <= 1e-5 * ref[key].abs()).all()), (what, key)
    print(f"{what}: loss rel err {_rel(loss.cpu(), ref['loss']):.3g}")
    assert _rel(loss.cpu(), ref["loss"]) < 1e-5, (what, float(loss), float(ref["loss"]))
    return loss, grads, _check_grads(grads, ref, C_PRODUCT, what, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(GOLD))
def test_hip_matches_reference_goldens(hip_lib, name):
    g = GOLD[name]
    case, ref = _golden_case(name)
    loss, grads, _ = _check_against_oracle(case, ref, name)
    assert _rel(loss.cpu(), g["loss"]) < 1e-5, (float(loss), float(g["loss"]))       # NaN matches NaN only
    loss2, stats, _ = _hip(case, grads=(False, False))
    assert torch.equal(stats["n_valid"].cpu(), g["n_valid"])
    assert torch.equal(loss2, loss) or (math.isnan(float(loss2)) and math.isnan(float(loss)))
    if "grad_pr1" in g:
        # against the reference's own float32 gradients: both sides carry their float32 direction error, so the bound is
        # the sum of the two (c = 8 for the product, 2.1 for the reference)
        for got, want in zip(grads, (g["grad_pr1"], g["grad_pr2"])):
            assert torch.equal(torch.isnan(got.cpu()), torch.isnan(want)) and \
                torch.equal(torch.isinf(got.cpu()), torch.isinf(want)), name
        tol = go.grad_tolerance(ref, C_PRODUCT) + go.grad_tolerance(ref, C_REFERENCE)
        err = (torch.stack([t.cpu().double() for t in grads]) - torch.stack([g["grad_pr1"], g["grad_pr2"]]).double()).abs()
        assert bool((err <= tol).all()), (name, float((err / tol).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 17, 13), (2, 27, 38), (3, 64, 64), (2, 96, 112), (2, 256, 256)])
def test_hip_matches_oracle(hip_lib, shape):
    """(2,27,38): 1,026 points, a full slot and a second slot that holds two points; (2,96,112): 10,752 points, not a power of two, 11 slots and two histogram segments per row; (2,256,256): 64 slots
    and eight segments per row, thresholds deep inside the float32 pattern (all three digit passes decide)."""
    case, ref = _decided_case(*shape)
    assert go.decided(case)
    _check_against_oracle(case, ref, shape)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [(("dist_clip", 8.0),), (("disable_view1", True),), (("gt_scale", True),),
                                  (("norm_mode", None),), (("dist_clip", 30.0), ("disable_view1", True))])
def test_hip_matches_oracle_options_on_unaligned_rows(hip_lib, opts):
    """33 x 47: a row is 4,653 floats, so every other row starts off 16-byte alignment (scalar loads and stores) and the
    1,551 points leave a tail; each option of the call, and each view's gradient asked for alone."""
    case, ref = _decided_case(3, 33, 47, 400, opts)
    assert go.decided(case)
    _, both, _ = _check_against_oracle(case, ref, opts)
    for grads in ((True, False), (False, True)):
        _, _, one = _hip(case, grads=grads)
        for v in (0, 1):
            want = both[v] if grads[v] else torch.zeros_like(both[v])
            assert torch.equal(one[v], want), (opts, grads, v)


@pytest.mark.gpu
def test_strided_view_equals_contiguous_copy_bitwise(hip_lib):
    """The caller's predictions are means[:, i].squeeze(-2) of [b,v,h,w,1,3]: read in place through the batch stride."""
    case, _ = _decided_case(2, 33, 47, 400)
    means = torch.stack([case["pr_pts1"], case["pr_pts2"]], 1)[:, :, :, :, None, :].cuda()
    gts = torch.stack([case["gt_pts1"], case["gt_pts2"]], 1).cuda()
    v1, v2 = means[:, 0].squeeze(-2), means[:, 1].squeeze(-2)
    assert not v1.is_contiguous() and not v2.is_contiguous()
    a = _hip(case, pr_pts1=v1, pr_pts2=v2, gt_pts1=gts[:, 0], gt_pts2=gts[:, 1])
    b = _hip(case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])
    for key in ("n_valid", "q", "nf_pr", "nf_gt"):
        assert torch.equal(a[1][key], b[1][key]), key
    # through autograd: the gradient lands in the [b,v,h,w,1,3] leaf
    leaf = means.clone().requires_grad_(True)
    from spfsplatv2_amd import loss as L
    L.Regr3D()(gts[:, 0], gts[:, 1], leaf[:, 0].squeeze(-2), leaf[:, 1].squeeze(-2), case["conf1"].cuda(),
               case["conf2"].cuda()).backward()
    assert torch.equal(leaf.grad[:, 0, :, :, 0], b[2][0]) and torch.equal(leaf.grad[:, 1, :, :, 0], b[2][1])


@pytest.mark.gpu
def test_two_runs_are_bitwise_equal(hip_lib):
    case, _ = _decided_case(3, 64, 64)
    a, b = _hip(case), _hip(case)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])
    for key in ("n_valid", "q", "nf_pr", "nf_gt"):
        assert torch.equal(a[1][key], b[1][key]), key


@pytest.mark.gpu
def test_forward_backward_never_sync(hip_lib):
    case, _ = _decided_case(3, 64, 64)
    dev = {k: case[k].cuda() for k in INPUTS}
    clip = dict(case, dist_clip=8.0)
    want = _hip(case, **dev), _hip(clip, **dev)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _hip(case, **dev), _hip(clip, **dev)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for w, g in zip(want, got):
        assert torch.equal(w[0], g[0]) and torch.equal(w[2][0], g[2][0]) and torch.equal(w[2][1], g[2][1])


@pytest.mark.gpu
def test_bf16_inputs_are_computed_in_float32(hip_lib):
    case, _ = _decided_case(2, 17, 13)
    p1, p2 = case["pr_pts1"].cuda().bfloat16(), case["pr_pts2"].cuda().bfloat16()
    low = _hip(case, pr_pts1=p1, pr_pts2=p2, gt_pts1=case["gt_pts1"].cuda().double())
    assert low[2][0].dtype == torch.bfloat16 and low[2][1].dtype == torch.bfloat16
    full = _hip(case, pr_pts1=p1.float(), pr_pts2=p2.float())
    assert torch.equal(low[0], full[0])
    assert torch.equal(low[2][0], full[2][0].bfloat16()) and torch.equal(low[2][1], full[2][1].bfloat16())
    rounded = dict(case, pr_pts1=p1.float().cpu(), pr_pts2=p2.float().cpu())
    assert _rel(low[0].cpu(), go.run_ref(rounded)["loss"]) < 1e-5


@pytest.mark.gpu
def test_upstream_gradient_is_read_on_the_device(hip_lib):
    """model_wrapper.py:329 multiplies the loss by 0.1."""
    case, ref = _decided_case(3, 64, 64)
    _check_against_oracle(case, ref, "upstream 0.1", scale=0.1, upstream=0.1)
    up = torch.tensor(0.1, device="cuda")
    a, b = _hip(case, upstream=up), _hip(case, upstream=0.1)
    assert torch.equal(a[2][0], b[2][0]) and torch.equal(a[2][1], b[2][1])
