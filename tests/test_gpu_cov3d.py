"""Precomputed 3-D covariances (cov3Ds_precomp) on the MI355X, against the float64 oracle.

The oracle reads scales and rotations only through `splat_ref.covariance3d`, so it renders arbitrary covariances when
that function is replaced: here the oracle's "rotations" leaf IS the packed covariance [b,G,6] (float64, differentiable)
and its "scales" leaf a column of ones, which the scale-invariant glue multiplies by k = 1/near -- Sigma * k^2 per render,
exactly what the product applies."""
from math import isqrt

import pytest
import torch

import spfsplatv2_amd as spf
from oracle import splat_ref
from spfsplatv2_amd import synthetic as syn
from tests import util

pytestmark = pytest.mark.gpu

ROW, COL = torch.triu_indices(3, 3)
NAMES = ("means", "opacities", "harmonics", "extrinsics")
FRAGILE_CAP_C2 = 0.002          # (tests/test_gpu_raster.py: the knife-edge budget at BASELINE config 2's full size)
COV3D = splat_ref.covariance3d  # (the oracle's own, kept before any test replaces it)


def sym(c6):
    xx, xy, xz, yy, yz, zz = c6.unbind(-1)
    return torch.stack([xx, xy, xz, xy, yy, yz, xz, yz, zz], dim=-1).reshape(*c6.shape[:-1], 3, 3)


def pack(m):
    return m[..., ROW, COL]


def cov_of_batch(batch, dtype=torch.float64):
    return pack(COV3D(batch.scales.to(dtype), batch.rotations.to(dtype), 1.0))


def clamped_cholesky_cov(c6):
    """L L^T of the factor the kernels use (include/spfsplat_hip.h: non-positive pivots clamped with their column)."""
    a, b, c, d, e, f = c6.double().unbind(-1)
    l00 = a.clamp_min(0).sqrt()
    i0 = torch.where(l00 > 0, 1 / l00.clamp_min(1e-300), torch.zeros_like(l00))
    l10, l20 = b * i0, c * i0
    p1 = d - l10 * l10
    l11 = p1.clamp_min(0).sqrt()
    i1 = torch.where(l11 > 0, 1 / l11.clamp_min(1e-300), torch.zeros_like(l11))
    l21 = (e - l20 * l10) * i1
    l22 = (f - l20 * l20 - l21 * l21).clamp_min(0).sqrt()
    z = torch.zeros_like(a)
    L = torch.stack([l00, z, z, l10, l11, z, l20, l21, l22], dim=-1).reshape(*a.shape, 3, 3)
    return pack(L @ L.transpose(-1, -2))


@pytest.fixture
def cov_oracle(monkeypatch):
    from oracle import glue_ref
    monkeypatch.setattr(splat_ref, "covariance3d", lambda s, q, m: sym(q) * (s[..., 0] ** 2)[:, None, None])

    def run(batch, cov6, scale_invariant=True, mask_fragile=True, with_grads=True):
        dt = torch.float64
        leaves = {n: getattr(batch, n).detach().clone().to(dt).requires_grad_(with_grads) for n in NAMES}
        cov = cov6.detach().clone().to(dt).requires_grad_(with_grads)
        unit = torch.ones(*cov.shape[:2], 1, dtype=dt)
        color, depth, alpha, radii, frag, rfrag = glue_ref.decoder_forward(
            leaves["means"], leaves["harmonics"], leaves["opacities"], cov, unit, leaves["extrinsics"],
            batch.intrinsics.to(dt), batch.near.to(dt), batch.far.to(dt), batch.image_shape, (0.0, 0.0, 0.0),
            make_scale_invariant=scale_invariant, dtype=dt, want_fragile=True, want_radii_fragile=True)
        res = dict(color=color.detach(), depth=depth.detach(), alpha=alpha.detach(), radii=radii, fragile=frag,
                   radii_fragile=rfrag)
        if with_grads:
            wd, wa = util.loss_weights(batch)
            mask = (~frag).to(torch.float32) if mask_fragile else None
            res["pixel_mask"] = mask
            loss = util.scalar_loss(color, depth, alpha, batch.target.to(dt), wd.to(dt), wa.to(dt), mask)
            loss.backward()
            res["grads"] = {n: leaves[n].grad.detach().clone() for n in NAMES}
            res["grads"]["cov"] = cov.grad.detach().clone()
        return res
    return run


def run_cov_product(batch, cov, pixel_mask=None, scale_invariant=True, max_pairs=None, enable_cov_grad=True,
                    device="cuda"):
    """render_batch on precomputed covariances (`cov` [b,G,6] or [b,G,3,3]) with the parity suite's loss."""
    bd = batch.to(device)
    leaves = {n: getattr(bd, n).detach().clone().requires_grad_() for n in NAMES}
    c = cov.detach().clone().to(device).requires_grad_()
    h, w = batch.image_shape
    deg = isqrt(batch.harmonics.shape[-1]) - 1
    color, depth, alpha, radii = spf.render_batch(
        leaves["extrinsics"], bd.intrinsics, bd.near, bd.far, leaves["means"], None, None, leaves["opacities"],
        leaves["harmonics"], None, torch.zeros(3, device=device), h, w, deg, scale_invariant, enable_cov_grad, True,
        max_pairs=max_pairs, sh_layout="g3k", cov3D=c)
    depth = depth[:, :, 0]
    if scale_invariant:
        depth = depth * bd.near[:, :, None, None]
    wd, wa = util.loss_weights(batch)
    loss = util.scalar_loss(color, depth, alpha, bd.target, wd.to(device), wa.to(device),
                            None if pixel_mask is None else pixel_mask.to(device))
    loss.backward()
    grads = {n: leaves[n].grad.detach().cpu() for n in NAMES}
    grads["cov"] = None if c.grad is None else c.grad.detach().cpu()
    return dict(color=color.detach().cpu(), depth=depth.detach().cpu(), alpha=alpha.detach().cpu(),
                radii=radii.cpu(), grads=grads)


def gate(prod, ref, **kw):
    rep = util.compare(prod, ref, **kw)
    if rep["g_cov"] > 1e-3:
        rep["fails"].append("g_cov")
    if rep["gel_cov"] > 1e-2:
        rep["fails"].append("gel_cov")
    return rep


def finite(res):
    ts = [res["color"], res["depth"], res["alpha"]] + [g for g in res["grads"].values() if g is not None]
    return all(bool(torch.isfinite(t).all()) for t in ts)


@pytest.mark.parametrize("K,s_mult", [(1, 1.0), (16, 2.0)], ids=["c2", "c2_sh3"])
def test_cov_parity_at_full_size(hip_lib, cov_oracle, K, s_mult):
    """BASELINE config 2 at full size, the covariance of every Gaussian formed from its scales and quaternion in
    float64: image, depth, alpha, radii and every gradient (means, opacities, SH, covariance, pose) against the oracle."""
    batch = syn.make_batch(config="C2", n_scenes=1, n_views=1, seed=8, K=K, s_mult=s_mult)
    cov6 = cov_of_batch(batch).to(torch.float32)
    ref = cov_oracle(batch, cov6)
    prod = run_cov_product(batch, cov6, pixel_mask=ref["pixel_mask"])
    rep = gate(prod, ref, max_fragile_frac=FRAGILE_CAP_C2)
    assert not rep["fails"], rep
    assert rep["radii_mismatch"] == 0


def _random_covariances(batch, seed):
    """Covariances no scale/quaternion pair of the batch produced: random orientations, eigenvalues spread over up to
    six decades (condition numbers to 1e6), every third Gaussian FLAT (rank 2: one eigenvalue exactly 0)."""
    gen = torch.Generator().manual_seed(seed)
    b, G = batch.scales.shape[:2]
    q = torch.randn(b, G, 4, generator=gen, dtype=torch.float64)
    Q = splat_ref.quat_to_rotmat(q / q.norm(dim=-1, keepdim=True))
    top = batch.scales.double().amax(dim=-1) ** 2 * 2.0
    lam = torch.stack([top, top * 10 ** (-6 * torch.rand(b, G, generator=gen, dtype=torch.float64)),
                       top * 10 ** (-6 * torch.rand(b, G, generator=gen, dtype=torch.float64))], dim=-1)
    lam[:, ::3, 2] = 0.0
    return pack(Q @ torch.diag_embed(lam) @ Q.transpose(-1, -2))


def test_cov_arbitrary_ill_conditioned_and_flat(hip_lib, cov_oracle):
    batch = syn.make_batch(config="TEST", n_scenes=2, n_views=2, seed=21, s_mult=8.0, G=1500, K=4, image_hw=(80, 112))
    cov6 = _random_covariances(batch, 5).to(torch.float32)
    ref = cov_oracle(batch, cov6)
    prod = run_cov_product(batch, cov6, pixel_mask=ref["pixel_mask"])
    assert finite(prod)
    rep = gate(prod, ref)
    assert not rep["fails"], rep


def test_cov_indefinite_renders_its_clamped_factor(hip_lib, cov_oracle):
    """An indefinite Sigma neither faults nor produces NaN: it renders -- and differentiates -- as L L^T of the Cholesky
    factor with non-positive pivots clamped to zero (the documented behaviour)."""
    batch = syn.make_batch(config="TEST", n_scenes=1, n_views=2, seed=22, s_mult=8.0, G=999, K=4, image_hw=(64, 64))
    cov6 = _random_covariances(batch, 6)
    gen = torch.Generator().manual_seed(7)
    q = torch.randn(1, 5, 4, generator=gen, dtype=torch.float64)
    Q = splat_ref.quat_to_rotmat(q / q.norm(dim=-1, keepdim=True))
    top = batch.scales[0, :5].double().amax(dim=-1) ** 2 * 4.0
    lam = torch.stack([top, -0.5 * top, 0.3 * top], dim=-1)[None]
    cov6[:, :5] = pack(Q @ torch.diag_embed(lam) @ Q.transpose(-1, -2))
    cov6 = cov6.to(torch.float32)
    ref = cov_oracle(batch, clamped_cholesky_cov(cov6).to(torch.float32))
    prod = run_cov_product(batch, cov6, pixel_mask=ref["pixel_mask"])
    assert finite(prod)
    rep = gate(prod, ref)
    assert not rep["fails"], rep


def test_cov_chain_rule_against_scale_rotation_path(hip_lib):
    """cov6 = covariance3d(s, q) in float32 through the covariance path: the image of the scale/rotation path (to 1e-4
    off the oracle's knife-edge pixels; the two factors round differently), and dL/dcov6 pushed through autograd of
    covariance3d gives that path's dL/dscales and dL/drotations."""
    batch = syn.make_batch(config="TEST", n_scenes=2, n_views=3, seed=3, s_mult=8.0, G=1500, K=4, image_hw=(80, 112))
    ref = util.run_oracle(batch, torch.float64, mask_fragile=True)
    base = util.run_product(batch, pixel_mask=ref["pixel_mask"])
    s = batch.scales.detach().clone().requires_grad_()
    q = batch.rotations.detach().clone().requires_grad_()
    cov6 = pack(COV3D(s, q, 1.0))
    prod = run_cov_product(batch, cov6, pixel_mask=ref["pixel_mask"])
    ok = ~ref["fragile"]
    assert float(((prod["color"] - base["color"]).abs() * ok[:, :, None]).max()) <= 1e-4
    ds, dq = torch.autograd.grad(cov6, (s, q), prod["grads"]["cov"])
    assert util.rel_linf(ds, base["grads"]["scales"]) <= 1e-3
    assert util.rel_linf(dq, base["grads"]["rotations"]) <= 1e-3
    assert util.rel_elementwise(ds, base["grads"]["scales"]) <= 1e-2
    assert util.rel_elementwise(dq, base["grads"]["rotations"]) <= 1e-2
    for n in NAMES:
        assert util.rel_linf(prod["grads"][n], base["grads"][n]) <= 1e-3, n


def test_cov_planned_direct_bins_equal_exact_mode(hip_lib):
    """The scale-invariant camera path: a planned call (direct bins, no host sync) gives bit-identical outputs and
    gradients to the exact-mode call; a compiled binding is never used for a covariance call, SPF_NO_FAST or not."""
    from spfsplatv2_amd import _lib
    batch = syn.make_batch(config="TEST", n_scenes=2, n_views=2, seed=23, s_mult=8.0, G=1500, K=16, image_hw=(64, 96))
    cov6 = cov_of_batch(batch).to(torch.float32)
    rec = spf.CallRecord()
    bd = batch.to("cuda")
    h, w = batch.image_shape
    spf.render_batch(bd.extrinsics, bd.intrinsics, bd.near, bd.far, bd.means, None, None, bd.opacities, bd.harmonics,
                     None, torch.zeros(3, device="cuda"), h, w, 3, True, sh_layout="g3k", record=rec,
                     cov3D=cov6.cuda())
    plan = spf.plan_pair_budget(rec)
    assert plan.max_tile_list > 0
    exact = run_cov_product(batch, cov6)
    planned = run_cov_product(batch, cov6, max_pairs=plan)
    assert spf.last_plan_flags() == 0
    for k in ("color", "depth", "alpha", "radii"):
        assert torch.equal(exact[k], planned[k]), k
    for n, g in exact["grads"].items():
        assert torch.equal(g, planned["grads"][n]), n
    orig = _lib.fast
    try:
        def refuse():
            raise AssertionError("the compiled binding was consulted for a covariance call")
        _lib.fast = refuse
        for flag in ("0", "1"):
            import os
            old = os.environ.get("SPF_NO_FAST")
            os.environ["SPF_NO_FAST"] = flag
            try:
                again = run_cov_product(batch, cov6)
            finally:
                if old is None:
                    os.environ.pop("SPF_NO_FAST", None)
                else:
                    os.environ["SPF_NO_FAST"] = old
            assert torch.equal(again["color"], exact["color"]) and torch.equal(again["grads"]["cov"], exact["grads"]["cov"])
    finally:
        _lib.fast = orig


def test_cov_gradient_bucket_raises(hip_lib):
    from spfsplatv2_amd import shard
    batch = syn.make_batch(config="C1", n_scenes=1, n_views=1, seed=1, s_mult=30.0)
    bd = batch.to("cuda")
    means = bd.means.clone().requires_grad_()
    cov = cov_of_batch(batch).to(torch.float32).cuda().requires_grad_()
    h, w = batch.image_shape
    color, *_ = spf.render_batch(bd.extrinsics, bd.intrinsics, bd.near, bd.far, means, None, None, bd.opacities,
                                 bd.harmonics, None, torch.zeros(3, device="cuda"), h, w, 0, True, sh_layout="g3k",
                                 cov3D=cov)
    bucket = shard.GradBucket(means, bd.scales, bd.rotations, bd.opacities, bd.harmonics)
    with pytest.raises(RuntimeError, match="GradBucket"):
        with bucket:
            color.sum().backward()


def test_gaussian_rasterizer_cov3ds_precomp(hip_lib, monkeypatch):
    """The drop-in surface: [G,6] and [G,3,3] give identical images, the gradients match the oracle, scale_modifier is
    not applied to a precomputed covariance, and enable_cov_grad=False leaves it without a gradient."""
    from spfsplatv2_amd import decoder as dec
    monkeypatch.setattr(splat_ref, "covariance3d", lambda s, q, m: sym(q))
    batch = syn.make_batch(config="TEST", n_scenes=1, n_views=1, seed=24, s_mult=8.0, G=1500, K=4, image_hw=(64, 80))
    view, proj, tanfov, _ = dec.camera_tensors(batch.extrinsics[:, 0], batch.intrinsics[:, 0], batch.near[:, 0],
                                               batch.far[:, 0], scale_invariant=False)
    h, w = batch.image_shape
    cov6 = cov_of_batch(batch)[0].to(torch.float32)
    shs = batch.harmonics[0].permute(0, 2, 1).contiguous()                 # [G,K,3], as cuda_splatting.py:79
    wimg = torch.rand(3, h, w, generator=torch.Generator().manual_seed(2))
    # oracle (float64)
    lv = dict(means=batch.means[0].double().requires_grad_(), cov=cov6.double().requires_grad_())
    img, dep, alp, rad, frag = splat_ref.rasterize(
        lv["means"], torch.ones(cov6.shape[0], 1, dtype=torch.float64), lv["cov"], batch.opacities[0, :, None].double(),
        shs.double(), None, view[0].double(), proj[0].double(), torch.zeros(3, dtype=torch.float64),
        float(tanfov[0, 0]), float(tanfov[0, 1]), h, w, 1, 2.5, want_fragile=True)
    mask = (~frag).double()
    (img * wimg.double() * mask).sum().backward()

    def product(c, enable_cov_grad=True):
        s = spf.GaussianRasterizationSettings(h, w, float(tanfov[0, 0]), float(tanfov[0, 1]), torch.zeros(3, device="cuda"),
                                              2.5, proj[0].cuda(), 1, enable_cov_grad=enable_cov_grad)
        m = batch.means[0].cuda().requires_grad_()
        c = c.cuda().requires_grad_()
        out = spf.GaussianRasterizer(s)(means3D=m, opacities=batch.opacities[0, :, None].cuda(), shs=shs.cuda(),
                                        cov3Ds_precomp=c, viewmatrix=view[0].cuda())
        (out[0] * wimg.cuda() * mask.float().cuda()).sum().backward()
        return out[0].detach().cpu(), m.grad.cpu(), c.grad
    i6, gm6, gc6 = product(cov6)
    i33, gm33, gc33 = product(sym(cov6))
    assert torch.equal(i6, i33) and torch.equal(gm6, gm33)
    assert torch.equal(gc6.cpu(), pack(gc33).cpu())
    assert float(gc33.cpu().tril(-1).abs().max()) == 0.0          # the lower triangle is never read
    assert float(((i6.double() - img.detach()).abs() * mask).max()) <= 1e-4
    assert util.rel_linf(gm6, lv["means"].grad) <= 1e-3
    assert util.rel_linf(gc6.cpu(), lv["cov"].grad) <= 1e-3
    assert util.rel_elementwise(gc6.cpu(), lv["cov"].grad) <= 1e-2
    _, _, none = product(cov6, enable_cov_grad=False)
    assert none is None


def test_decoder_use_covariances(hip_lib, cov_oracle):
    """DecoderSplattingCUDA with use_covariances: on covariances built in the rasterizer's (r,x,y,z) convention it
    renders what the default decoder renders; three planned training calls of one shape (prepared steps would take over
    on the default path) all return the oracle's covariance gradients; an evaluation call under no_grad works."""
    from spfsplatv2_amd import decoder as dec
    batch = syn.make_batch(config="TEST", n_scenes=2, n_views=2, seed=25, s_mult=8.0, G=1500, K=4, image_hw=(64, 64))
    cov33 = COV3D(batch.scales.double(), batch.rotations.double(), 1.0).to(torch.float32)
    ref = cov_oracle(batch, pack(cov33))
    base = util.run_product(batch, pixel_mask=ref["pixel_mask"], with_grads=False)
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True, True, True,
                                                    use_covariances=True)).to("cuda")
    d.auto_plan = None
    bd = batch.to("cuda")
    wd, wa = util.loss_weights(batch)

    def call(plan):
        d.max_pairs = plan
        leaves = {n: getattr(bd, n).detach().clone().requires_grad_() for n in NAMES}
        c = cov33.cuda().requires_grad_()
        g = dec.Gaussians(leaves["means"], c, None, None, leaves["harmonics"], leaves["opacities"])
        out, alpha, radii = d.render(g, leaves["extrinsics"], bd.intrinsics, bd.near, bd.far, batch.image_shape)
        loss = util.scalar_loss(out.color, out.depth, alpha, bd.target, wd.cuda(), wa.cuda(), ref["pixel_mask"].cuda())
        loss.backward()
        grads = {n: leaves[n].grad.cpu() for n in NAMES}
        assert float(c.grad.cpu().tril(-1).abs().max()) == 0.0
        grads["cov"] = pack(c.grad.cpu())
        return dict(color=out.color.detach().cpu(), depth=out.depth.detach().cpu(), alpha=alpha.detach().cpu(),
                    radii=radii.cpu(), grads=grads)
    first = call(None)
    ok = ~ref["fragile"]
    assert float(((first["color"] - base["color"]).abs() * ok[:, :, None]).max()) <= 1e-4
    plan = spf.plan_pair_budget(d.last_call)
    for _ in range(3):
        res = call(plan)
        rep = gate(res, ref)
        assert not rep["fails"], rep
    assert not d._prepared_steps
    with torch.no_grad():
        g = dec.Gaussians(bd.means, cov33.cuda(), None, None, bd.harmonics, bd.opacities)
        out = d(g, bd.extrinsics, bd.intrinsics, bd.near, bd.far, batch.image_shape)
    assert torch.equal(out.color.cpu(), res["color"])


def test_cov_full_matrix_planned_call_does_not_sync(hip_lib):
    """A planned call (check="deferred") on the [S,G,3,3] form -- what the decoder hands over -- neither synchronises the
    host in its forward nor in its backward (the packing of the upper triangle moves no index tensor to the device),
    gives the exact-mode result bit for bit, and puts no gradient on the lower triangle."""
    batch = syn.make_batch(config="TEST", n_scenes=2, n_views=2, seed=26, s_mult=8.0, G=1500, K=4, image_hw=(64, 96))
    cov33 = COV3D(batch.scales.double(), batch.rotations.double(), 1.0).to(torch.float32)
    rec = spf.CallRecord()
    bd = batch.to("cuda")
    h, w = batch.image_shape
    spf.render_batch(bd.extrinsics, bd.intrinsics, bd.near, bd.far, bd.means, None, None, bd.opacities, bd.harmonics,
                     None, torch.zeros(3, device="cuda"), h, w, 1, True, sh_layout="g3k", record=rec,
                     cov3D=cov33.cuda())
    plan = spf.plan_pair_budget(rec, check="deferred")
    wd, wa = (t.cuda() for t in util.loss_weights(batch))
    c33 = cov33.cuda()

    def go(max_pairs):                  # (every input already on the device: nothing below copies from the host)
        leaves = {n: getattr(bd, n).detach().clone().requires_grad_() for n in NAMES}
        c = c33.clone().requires_grad_()
        color, depth, alpha, _ = spf.render_batch(
            leaves["extrinsics"], bd.intrinsics, bd.near, bd.far, leaves["means"], None, None, leaves["opacities"],
            leaves["harmonics"], None, torch.zeros(3, device="cuda"), h, w, 1, True, max_pairs=max_pairs,
            sh_layout="g3k", cov3D=c)
        util.scalar_loss(color, depth[:, :, 0] * bd.near[:, :, None, None], alpha, bd.target, wd, wa).backward()
        return color.detach(), c.grad
    exact = go(None)
    go(plan)                                                         # warm-up (allocator, caches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        planned = go(plan)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert spf.last_plan_flags() == 0
    assert torch.equal(exact[0], planned[0]) and torch.equal(exact[1], planned[1])
    assert float(planned[1].tril(-1).abs().max()) == 0.0
    assert float(planned[1].abs().max()) > 0.0


def test_cov_rasterize_batch_never_uses_the_compiled_binding(hip_lib, monkeypatch):
    """rasterize_batch (no camera: the path whose forward would consult the compiled binding) with a covariance takes
    the ctypes route in forward and backward, SPF_NO_FAST set or not."""
    from spfsplatv2_amd import _lib
    from spfsplatv2_amd import decoder as dec
    batch = syn.make_batch(config="TEST", n_scenes=1, n_views=2, seed=27, s_mult=8.0, G=999, K=4, image_hw=(64, 64))
    view, proj, tanfov, scale = dec.camera_tensors(batch.extrinsics.flatten(0, 1), batch.intrinsics.flatten(0, 1),
                                                   batch.near.flatten(), batch.far.flatten())
    shs = batch.harmonics.permute(0, 1, 3, 2).contiguous().cuda()
    cov6 = cov_of_batch(batch).to(torch.float32).cuda()

    def run():
        m = batch.means.cuda().requires_grad_()
        c = cov6.clone().requires_grad_()
        img, *_ = spf.rasterize_batch(m, None, None, batch.opacities.cuda(), shs, None, view.view(1, 2, 4, 4).cuda(),
                                      proj.view(1, 2, 4, 4).cuda(), tanfov.view(1, 2, 2).cuda(),
                                      torch.zeros(3, device="cuda"), 64, 64, 1, view_scale=scale.view(1, 2).cuda(),
                                      cov3D=c)
        img.square().sum().backward()
        return img.detach().cpu(), c.grad.cpu()
    want = run()

    def refuse():
        raise AssertionError("the compiled binding was consulted for a covariance call")
    monkeypatch.setattr(_lib, "fast", refuse)
    for flag in ("0", "1"):
        monkeypatch.setenv("SPF_NO_FAST", flag)
        got = run()
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
