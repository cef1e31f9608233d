"""Parity of the HIP rasterizer (through the C ABI) against the CPU oracle on seeded inputs.

Tolerances (BASELINE.json north_star): RGB 1e-4 absolute, gradients 1e-3 relative to the tensor scale.
"""
import json
import os

import pytest
import torch

from spfsplatv2_amd import synthetic as syn
from tests import util

pytestmark = pytest.mark.gpu

CASES = {
    # name: (make_batch kwargs, background, scale_invariant)
    "c1_k1": (dict(config="C1", n_scenes=1, n_views=1, seed=1, s_mult=30.0), (0.0, 0.0, 0.0), True),
    "c1_bg_nosi": (dict(config="C1", n_scenes=2, n_views=2, seed=2, s_mult=60.0), (0.2, 0.5, 0.9), False),
    "k4_multiview": (dict(config="TEST", n_scenes=2, n_views=3, seed=3, s_mult=8.0, G=1500, K=4,
                          image_hw=(80, 112)), (0.1, 0.2, 0.3), True),
    "k9_ragged": (dict(config="TEST", n_scenes=1, n_views=2, seed=4, s_mult=15.0, G=999, K=9,
                       image_hw=(50, 70)), (0.0, 0.0, 0.0), True),
    "k16_dense": (dict(config="TEST", n_scenes=1, n_views=1, seed=5, s_mult=20.0, G=4096, K=16,
                       image_hw=(64, 64)), (1.0, 1.0, 1.0), True),
    "k25_stride": (dict(config="TEST", n_scenes=1, n_views=2, seed=6, s_mult=10.0, G=700, K=25,
                        image_hw=(48, 48)), (0.0, 0.0, 0.0), True),
    "pixel_aligned": (dict(config="TEST", n_scenes=2, n_views=2, seed=7, s_mult=1.0, G=8192,
                           image_hw=(64, 64)), (0.0, 0.0, 0.0), True),
    # BASELINE.json configs[1] at FULL size (the bench workload): 65,536 pixel-aligned Gaussians, 256x256, two views
}


# knife-edge budget at BASELINE config 2's full size: round 3 flagged 0.8 % of the pixels to hide 0.003 %; with round 4's
# windows (oracle/splat_ref.py FRAG_*) the flagged fraction is measured at 0.05 % (K = 1) -- the cap is twice that
FRAGILE_CAP_C2 = 0.002


@pytest.mark.parametrize("K,s_mult", [(1, 1.0), (16, 2.0)], ids=["c2", "c2_sh3_wider"])
def test_parity_vs_oracle_at_full_size(hip_lib, K, s_mult):
    """BASELINE.json configs[1] at FULL size (the bench workload): 65,536 pixel-aligned Gaussians, 256x256 -- and the
    same scene with SH degree 3 and twice the footprint (BASELINE configs[4]'s coefficient count).
    At this size a few hundred of the 65,536 pixels sit on a knife edge of the algorithm (an alpha within 2e-4 of
    1/255, ...), where float32 and float64 may take different branches: a contribution of up to 1/255 appears or
    not, and so does its gradient.  Those pixels (flagged by the float64 oracle, < 2 %) are excluded from the RGB
    gate as everywhere else AND switched off in the loss of both sides, so that the gradient gate (1e-3 of the
    tensor's scale, over every Gaussian) compares like with like.
    SECOND comparison, forced (util.BranchForcing): the flagged pixels are not masked but held against the float64
    oracle on the branch the kernel took there, image and gradients, same gates.  The report line also carries the
    float32 oracle's own unmasked `gall_*` (`oracle_f32_gall_*`) next to the product's: reported, not gated."""
    batch = syn.make_batch(config="C2", n_scenes=1, n_views=1, seed=8, K=K, s_mult=s_mult)
    ref = util.run_oracle(batch, torch.float64, mask_fragile=True, unmasked_too=True, decisions=True)
    forcing = util.BranchForcing(batch, ref)
    prod = util.run_product(batch, pixel_mask=ref["pixel_mask"], unmasked_too=True, after_forward=forcing.mask_for)
    rep = util.compare(prod, ref, max_fragile_frac=FRAGILE_CAP_C2)
    rep["num_pairs"] = prod["stats"].get("num_pairs")
    forced = forcing.compare(prod)
    _report(f"c2_full_size_K{K}", {**rep, **forcing.report_entry(forced), **util.float32_gall(batch, ref)})
    assert not rep["fails"], rep
    assert not forced["fails"], forced
    assert prod["stats"]["num_pairs"] > 60000


def _report(name, rep):
    out = os.environ.get("SPF_PARITY_REPORT")
    if out:
        with open(out, "a") as f:
            f.write(json.dumps({"case": name, **rep}) + "\n")


@pytest.mark.parametrize("name", list(CASES))
def test_parity_vs_oracle(hip_lib, name):
    kw, bg, si = CASES[name]
    batch = syn.make_batch(**kw)
    # knife-edge pixels (flagged by the float64 oracle) are excluded from the RGB gate and switched off in the loss of
    # both sides, so that the gradient gate compares like with like (see test_parity_vs_oracle_at_full_size)
    ref = util.run_oracle(batch, torch.float64, background=bg, scale_invariant=si, mask_fragile=True, unmasked_too=True,
                          decisions=True)
    forcing = util.BranchForcing(batch, ref, background=bg, scale_invariant=si)
    prod = util.run_product(batch, background=bg, scale_invariant=si, pixel_mask=ref["pixel_mask"], unmasked_too=True,
                            after_forward=forcing.mask_for)
    rep = util.compare(prod, ref)
    rep["num_pairs"] = prod["stats"].get("num_pairs")
    forced = forcing.compare(prod)        # the flagged pixels on the branch the kernel took (util.BranchForcing)
    _report(name, {**rep, **forcing.report_entry(forced)})
    assert not rep["fails"], rep
    assert not forced["fails"], forced
    # (util.compare also gates: radii bit-exact off the Gaussian's own rounding knife-edges, and the number of pixels
    # of the UNMASKED image that are off by > 1e-4 is bounded by the number of flagged pixels)
    assert rep["radii_mismatch"] == 0 and rep["bad_frac_all"] <= rep["fragile_frac"]


def test_radii_and_determinism(hip_lib):
    import spfsplatv2_amd as spf
    kw, bg, si = CASES["k4_multiview"]
    batch = syn.make_batch(**kw)
    a = util.run_product(batch, background=bg, scale_invariant=si)
    b = util.run_product(batch, background=bg, scale_invariant=si)
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["depth"], b["depth"])    # forward is bit-stable
    for n in util.GRAD_NAMES:                                                             # float atomics: ~1e-6
        assert util.rel_linf(a["grads"][n], b["grads"][n]) < 1e-4, n


def test_sync_free_capacity_mode_and_overflow(hip_lib):
    kw, bg, si = CASES["k4_multiview"]
    batch = syn.make_batch(**kw)
    exact = util.run_product(batch, background=bg, scale_invariant=si)
    D = exact["stats"]["num_pairs"]
    roomy = util.run_product(batch, background=bg, scale_invariant=si, max_pairs=2 * D + 7)
    assert torch.equal(exact["color"], roomy["color"])
    for n in util.GRAD_NAMES:
        assert util.rel_linf(roomy["grads"][n], exact["grads"][n]) < 1e-4, n
    from spfsplatv2_amd._lib import SpfError
    with pytest.raises(SpfError, match="overflow"):
        util.run_product(batch, background=bg, scale_invariant=si, max_pairs=max(D // 2, 1))


def test_planned_pair_budget_is_verified_on_the_device(hip_lib):
    """PairBudget: a call planned from an earlier one needs no read-back; the device checks the plan (flag bits
    1 = capacity, 2 = longest list) and a failed plan is never silent."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd._lib import SpfError
    kw, bg, si = CASES["k4_multiview"]
    batch = syn.make_batch(**kw)
    exact = util.run_product(batch, background=bg, scale_invariant=si)
    st = exact["stats"]
    plan = spf.plan_pair_budget(st, slack=1.25, check="deferred")
    assert plan.capacity >= st["num_pairs"] and plan.max_tile_list >= st["max_tile_list"]
    planned = util.run_product(batch, background=bg, scale_invariant=si, max_pairs=plan)
    assert spf.last_plan_flags() == 0
    assert torch.equal(exact["color"], planned["color"]) and torch.equal(exact["depth"], planned["depth"])
    for n in util.GRAD_NAMES:
        assert util.rel_linf(planned["grads"][n], exact["grads"][n]) < 1e-5, n     # (LDS float atomics in dense tiles)

    # a list longer than planned: flag 2, reported (deferred) or raised in backward
    short = plan._replace(max_tile_list=max(st["max_tile_list"] // 2, 1))
    util.run_product(batch, background=bg, scale_invariant=si, max_pairs=short)
    assert spf.last_plan_flags() & 2
    with pytest.raises(SpfError, match="did not hold"):
        util.run_product(batch, background=bg, scale_invariant=si, max_pairs=short._replace(check="backward"))

    # too few pairs: flag 1
    util.run_product(batch, background=bg, scale_invariant=si, max_pairs=plan._replace(capacity=st["num_pairs"] // 2))
    assert spf.last_plan_flags() & 1
    # check="early": the forward itself verifies (behind the projection kernel, the rest of the chain already issued) and
    # raises; a plan that holds gives the planned result with nothing left to check
    early = util.run_product(batch, background=bg, scale_invariant=si, max_pairs=plan._replace(check="early"))
    assert torch.equal(early["color"], exact["color"]) and spf.last_plan_flags() == 0
    for bad in (short, plan._replace(capacity=st["num_pairs"] // 2)):
        with pytest.raises(SpfError):
            util.run_product(batch, background=bg, scale_invariant=si, max_pairs=bad._replace(check="early"), with_grads=False)
    # and a good plan afterwards is clean again
    util.run_product(batch, background=bg, scale_invariant=si, max_pairs=plan)
    assert spf.last_plan_flags() == 0


def test_drop_in_rasterizer_surface(hip_lib):
    """GaussianRasterizationSettings / GaussianRasterizer exactly as the reference calls them
    (cuda_splatting.py:105-138) vs the oracle on the same arguments."""
    import spfsplatv2_amd as spf
    from oracle import glue_ref, splat_ref
    batch = syn.make_batch("TEST", 1, 1, seed=9, s_mult=12.0, G=800, K=4, image_hw=(64, 64))
    args = glue_ref.callsite_args(batch.extrinsics[:, 0], batch.intrinsics[:, 0], batch.near[:, 0], batch.far[:, 0],
                                  batch.image_shape, torch.tensor([[0.3, 0.1, 0.2]]), batch.means, batch.harmonics,
                                  batch.opacities, batch.rotations, batch.scales)[0]
    dev = "cuda"
    t = lambda x: x.to(dev)
    leaves = {k: t(args[k]).clone().requires_grad_(True)
              for k in ("means3D", "shs", "opacities", "scales", "rotations", "viewmatrix")}
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    settings = spf.GaussianRasterizationSettings(
        image_height=args["image_height"], image_width=args["image_width"], tanfovx=args["tanfovx"],
        tanfovy=args["tanfovy"], bg=t(args["bg"]), scale_modifier=1.0,
        projmatrix=t(args["projmatrix"].T.contiguous()).T,            # non-contiguous view, as the reference passes
        sh_degree=args["sh_degree"], prefiltered=False, debug=False, enable_cov_grad=True, enable_sh_grad=True)
    image, depth, norm, alpha, radii, extra = spf.GaussianRasterizer(settings)(
        means3D=leaves["means3D"], means2D=means2D, shs=leaves["shs"], colors_precomp=None,
        opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"],
        viewmatrix=leaves["viewmatrix"])
    assert image.shape == (3, 64, 64) and depth.shape == (1, 64, 64) and alpha.shape == (1, 64, 64)
    assert radii.shape == (800,) and radii.dtype == torch.int32 and norm is None and extra is None
    tgt = batch.target[0, 0].to(dev)
    ((image - tgt) ** 2).mean().backward()

    ol = {k: args[k].double().clone().requires_grad_(True) for k in leaves}
    oimg, odep, oalp, orad, frag = splat_ref.rasterize(
        ol["means3D"], ol["scales"], ol["rotations"], ol["opacities"], ol["shs"], None, ol["viewmatrix"],
        args["projmatrix"].double(), args["bg"].double(), args["tanfovx"], args["tanfovy"], 64, 64,
        args["sh_degree"], 1.0, want_fragile=True)
    ((oimg - batch.target[0, 0].double()) ** 2).mean().backward()
    ok = ~frag
    assert float(((image.detach().cpu().double() - oimg).abs() * ok).max()) < 1e-4
    assert float(((depth.detach().cpu().double() - odep).abs() * ok).max()) < 1e-4 * float(odep.max())
    assert (radii.cpu() != orad).float().mean() < 1e-3
    for k in leaves:
        assert util.rel_linf(leaves[k].grad, ol[k].grad) < 1e-3, k
    # screen-space gradient holder: NDC-scaled d loss / d pixel-centre, zero for culled Gaussians
    assert means2D.grad is not None and means2D.grad.shape == (800, 3)
    assert float(means2D.grad[:, 2].abs().max()) == 0.0
    assert float(means2D.grad[(radii == 0)].abs().max()) == 0.0 if bool((radii == 0).any()) else True
    assert float(means2D.grad.abs().max()) > 0.0


@pytest.mark.parametrize("seed", range(12))
def test_rasterizer_api_random_settings(hip_lib, seed):
    """The per-view drop-in surface away from the reference's own call pattern: `scale_modifier` != 1, an active
    `sh_degree` below what the coefficient count allows (3DGS raises it during training), `colors_precomp` instead of
    SH, non-square images, upstream gradients on all three differentiable outputs; vs the oracle on the same arguments
    (knife-edge pixels are switched off in both losses)."""
    import spfsplatv2_amd as spf
    from oracle import glue_ref, splat_ref
    g = torch.Generator().manual_seed(700 + seed)
    ri = lambda lo, hi: int(torch.randint(lo, hi + 1, (1,), generator=g))
    K = [1, 4, 9, 16, 25][ri(0, 4)]
    max_deg = [0, 1, 2, 3, 3][[1, 4, 9, 16, 25].index(K)]
    sh_degree = ri(0, max_deg)
    use_precomp = ri(0, 3) == 0
    smod = [0.5, 1.0, 1.7][ri(0, 2)]
    H, W = ri(9, 80), ri(9, 100)
    G = ri(50, 1500)
    batch = syn.make_batch("TEST", 1, 1, seed=700 + seed, s_mult=[2.0, 10.0, 40.0][ri(0, 2)], G=G, K=K, image_hw=(H, W))
    bg = torch.rand(1, 3, generator=g)
    args = glue_ref.callsite_args(batch.extrinsics[:, 0], batch.intrinsics[:, 0], batch.near[:, 0], batch.far[:, 0],
                                  batch.image_shape, bg, batch.means, batch.harmonics, batch.opacities,
                                  batch.rotations, batch.scales)[0]
    colors = torch.rand(G, 3, generator=g) if use_precomp else None
    names = ["means3D", "opacities", "scales", "rotations", "viewmatrix"] + (["colors"] if use_precomp else ["shs"])
    src = dict(args, colors=colors)
    wd, wa = torch.rand(1, H, W, generator=g), torch.rand(1, H, W, generator=g)
    tgt = batch.target[0, 0]

    def loss_of(img, dep, alp, mask):
        m = mask.to(img.dtype)
        return (((img - tgt.to(img)) ** 2) * m).mean() + 0.01 * (dep * wd.to(dep) * m).mean() + \
            0.1 * (alp * wa.to(alp) * m).mean()

    ol = {k: src[k].double().clone().requires_grad_(True) for k in names}
    oimg, odep, oalp, orad, frag, rfrag = splat_ref.rasterize(
        ol["means3D"], ol["scales"], ol["rotations"], ol["opacities"], ol.get("shs"), ol.get("colors"),
        ol["viewmatrix"], args["projmatrix"].double(), args["bg"].double(), args["tanfovx"], args["tanfovy"], H, W,
        sh_degree, smod, want_fragile=True, want_radii_fragile=True)
    mask = (~frag)[None]
    lo = loss_of(oimg, odep, oalp, mask)
    if lo.requires_grad:
        lo.backward()

    dev = "cuda"
    leaves = {k: src[k].to(dev).clone().requires_grad_(True) for k in names}
    means2D = torch.zeros(G, 3, device=dev, requires_grad=True)
    settings = spf.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=args["tanfovx"], tanfovy=args["tanfovy"], bg=args["bg"].to(dev),
        scale_modifier=smod, projmatrix=args["projmatrix"].to(dev), sh_degree=sh_degree, prefiltered=False,
        debug=False, enable_cov_grad=True, enable_sh_grad=True)
    image, depth, _norm, alpha, radii, _extra = spf.GaussianRasterizer(settings)(
        means3D=leaves["means3D"], means2D=means2D, shs=leaves.get("shs"), colors_precomp=leaves.get("colors"),
        opacities=leaves["opacities"], scales=leaves["scales"], rotations=leaves["rotations"],
        viewmatrix=leaves["viewmatrix"])
    loss_of(image, depth, alpha, mask.to(dev)).backward()

    ok = ~frag
    desc = dict(K=K, sh_degree=sh_degree, precomp=use_precomp, smod=smod, hw=(H, W), G=G)
    assert float(frag.float().mean()) < 0.1, desc
    oimg, odep, oalp = oimg.detach(), odep.detach(), oalp.detach()
    assert float(((image.detach().cpu().double() - oimg).abs() * ok).max()) < 1e-4, desc
    assert float(((alpha.detach().cpu().double() - oalp).abs() * ok).max()) < 1e-4, desc
    assert float(((depth.detach().cpu().double() - odep).abs() * ok).max()) < 1e-4 * max(float(odep.max()), 1e-9), desc
    assert int(((radii.cpu() != orad) & ~rfrag).sum()) == 0, desc
    for k in names:
        ref_g = ol[k].grad if ol[k].grad is not None else torch.zeros_like(ol[k])
        if float(ref_g.abs().max()) == 0.0:
            assert leaves[k].grad is None or float(leaves[k].grad.abs().max()) == 0.0, (k, desc)
        else:
            assert util.rel_linf(leaves[k].grad, ref_g) < 1e-3, (k, desc)


def test_planned_backward_mode_does_not_sync_in_forward(hip_lib):
    """`PairBudget(check="backward")` (the default) promises that the forward waits for nothing: the plan is verified
    when the backward runs.  (torch.is_grad_enabled() is False INSIDE autograd.Function.forward, so the mode must be
    sampled at the call site -- round 2 read it inside and synchronised on every training step.)  Under `no_grad` no
    backward will come and the forward itself verifies the plan: there the sync is the contract."""
    import spfsplatv2_amd as spf
    kw, bg, si = CASES["k4_multiview"]
    batch = syn.make_batch(**kw)
    exact = util.run_product(batch, background=bg, scale_invariant=si)
    plan = spf.plan_pair_budget(exact["stats"], slack=1.25, check="backward")
    bd = batch.to("cuda")
    d = util.product_decoder(bg, si, "cuda", plan, None)
    from spfsplatv2_amd import decoder as dec
    leaves = {n: getattr(bd, n).detach().clone().requires_grad_(True) for n in util.GRAD_NAMES}
    g = dec.Gaussians(leaves["means"], bd.covariances, leaves["rotations"], leaves["scales"], leaves["harmonics"],
                      leaves["opacities"])
    d.forward(g, leaves["extrinsics"], bd.intrinsics, bd.near, bd.far, bd.image_shape)      # warm-up (allocator, caches)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = d.forward(g, leaves["extrinsics"], bd.intrinsics, bd.near, bd.far, bd.image_shape)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    out.color.mean().backward()                              # the plan is verified here
    assert torch.equal(out.color.detach().cpu(), exact["color"])
    with torch.no_grad():
        torch.cuda.set_sync_debug_mode("error")
        try:
            with pytest.raises(RuntimeError):                # the verification read-back is a synchronising call
                d.forward(g, leaves["extrinsics"], bd.intrinsics, bd.near, bd.far, bd.image_shape)
        finally:
            torch.cuda.set_sync_debug_mode("default")
