"""Every BASELINE.json config under `-m gpu` (C3, C4 and C5 had no GPU test).

* oracle parity at FULL size, one (scene, view) each -- C3: 320,000 Gaussians at 256x256 (five context grids: lists of
  ~1,400 entries per tile, the (1024, 2048] register-sort class and the LDS classes), C5: 500,000 Gaussians, 16 SH
  coefficients, 512x512 (1,024 tiles) -- same gates as everywhere (RGB 1e-4, gradients 1e-3, radii bit-exact);
* size-independent properties on the full BATCHES the bench runs: C3 2 scenes x 4 views, C5 1 x 8, and BASELINE
  config 4's per-GPU share (8 scenes x 4 views of C2): bit-stable forward, background linearity, every scene of the
  batch bit-equal to rendering it alone (renders are independent: the multi-GPU sharding argument), a gradient checksum
  over all (Gaussian, tile) pairs, planned mode == exact mode;
* the reference's test-time pose alignment (model_wrapper.py:549-588): Gaussians frozen, ONLY the poses require grad,
  three Adam steps at lr 0.005 on the product and on the oracle;
* d_sh = 25 (the reference's default sh_degree 4): stride-only by default, band 4 evaluated on request;
* a failed plan is loud and deterministic: NaN everywhere, never uninitialised memory.
"""
import pytest
import torch

from spfsplatv2_amd import synthetic as syn
from tests import util

pytestmark = pytest.mark.gpu
SH_C0 = 0.28209479177387814


# ---- oracle parity at full size --------------------------------------------------------------------------------
# knife-edge budget: about twice the measured fraction of flagged pixels (profiles/r04_parity_reports.jsonl: 0.22 % / 0.19 %
# with round 4's windows; round 3 flagged 3.7 % / 2.1 % to hide 0.014 % / 0.008 % of pixels that actually differ)
FRAGILE_CAP = {"C3": 0.005, "C5": 0.004, "REF10V": 0.025}   # (REF10V: 1.1 % flagged by the float64 oracle: lists of thousands per pixel)
# the cases that ALSO get the forced comparison (util.BranchForcing).  REF10V does not: see the test's docstring.
FORCED = ("C3", "C5")
@pytest.mark.parametrize("config,min_pairs,min_list", [("C3", 250000, 1025), ("C5", 400000, 513),
                                                       ("REF10V", 500000, 2049)])
def test_parity_vs_oracle_full_size_c3_c5(hip_lib, config, min_pairs, min_list):
    """BASELINE configs 3 and 5 at FULL size, forward and every gradient, one (scene, view) each: 320,000 Gaussians at
    256x256; 500,000 Gaussians with 16 SH coefficients at 512x512 (1,024 tiles) -- and one scene of the reference's
    10-view training shape (REF10V: 655,360 Gaussians, 25 SH coefficients, one 256x256 target view = 256 tiles with lists
    of thousands of entries; re10k_10view.yaml:36-37,48).  (The float64 oracle needs seconds for these with 16 threads
    -- tests/conftest.py caps them: on a 256-core host the default is 20x slower.)
    C3 and C5 get the SECOND, forced comparison too (util.BranchForcing): flagged pixels held against the float64 oracle on
    the branch the kernel took, same gates, `unexplained == 0`, at most half of the flagged pixels and 0.1 % of the image
    still masked.  REF10V is NOT covered by it and keeps the masked gate alone: with the float32 oracle standing in for
    the product (CPU, seed 5) 580 of its 723 flagged pixels stay masked (80 %, 0.89 % of the image; 469 undecidable --
    lists of thousands of entries leave most threshold entries under a transmittance at which both branches are within
    1e-4 of the image -- and 110 flagged for other reasons); keeping the undecidable pixels whose candidate rows differ
    only in entries of weight alpha * T < 1e-4 unmasked (branch_explain `keep_light`) leaves 152 (21 % of the flagged, but
    0.23 % of the image: above the 0.1 % cap) and moves the stand-in's `gel_extrinsics` from 2.6e-3 to 9.7e-3, next to
    its 1e-2 gate."""
    batch = syn.make_batch(config, 1, 1, seed=5)
    force = config in FORCED
    ref = util.run_oracle(batch, torch.float64, mask_fragile=True, unmasked_too=True, decisions=force)
    forcing = util.BranchForcing(batch, ref) if force else None
    prod = util.run_product(batch, pixel_mask=ref["pixel_mask"], unmasked_too=True,
                            after_forward=forcing.mask_for if force else None)
    # lists of >1000 entries per pixel: proportionally more pixels sit next to an alpha / transmittance threshold
    rep = util.compare(prod, ref, max_fragile_frac=FRAGILE_CAP[config])
    rep.update(num_pairs=prod["stats"]["num_pairs"], max_tile_list=prod["stats"]["max_tile_list"])
    from tests.test_gpu_raster import _report
    forced = forcing.compare(prod) if force else None
    _report(f"{config.lower()}_full_size", {**rep, **(forcing.report_entry(forced) if force else {}),
                                            **(util.float32_gall(batch, ref) if force else {})})
    assert not rep["fails"], rep
    assert forced is None or not forced["fails"], forced
    assert prod["stats"]["num_pairs"] >= min_pairs and prod["stats"]["max_tile_list"] >= min_list, prod["stats"]
    if config == "C5":
        assert float(prod["grads"]["harmonics"][..., 9:].abs().max()) > 0        # degree-3 coefficients take part


def test_parity_vs_oracle_full_size_stress_regime(hip_lib):
    """SURVEY.md 8(d)'s stress regime at full size (the bench's `C2_stress` line): BASELINE config 2 with footprints x 10
    -- most tiles take the dense "rows" form backward and the sparse "lists" form forward (mean cull box between the two
    thresholds), the rest lists both ways: forward and every gradient of one (scene, view) against the float64 oracle."""
    batch = syn.make_batch("C2", 1, 1, seed=5, s_mult=10.0)
    ref = util.run_oracle(batch, torch.float64, mask_fragile=True, unmasked_too=True, decisions=True)
    forcing = util.BranchForcing(batch, ref)
    prod = util.run_product(batch, pixel_mask=ref["pixel_mask"], unmasked_too=True, after_forward=forcing.mask_for)
    rep = util.compare(prod, ref, max_fragile_frac=0.003)       # (measured: 0.15 % of the pixels flagged; 224 of 256 tiles dense)
    st = prod["stats"]
    rep.update(num_pairs=st["num_pairs"], max_tile_list=st["max_tile_list"], dense_tiles=st["dense_tiles"])
    from tests.test_gpu_raster import _report
    # this is the regime in which forward and backward composite a tile by different forms: the flagged pixels, held
    # against the float64 oracle on the branch the FORWARD took, gate the backward's decision about the same entries
    forced = forcing.compare(prod)
    _report("c2_stress_full_size", {**rep, **forcing.report_entry(forced), **util.float32_gall(batch, ref)})
    assert not rep["fails"], rep
    assert not forced["fails"], forced
    assert st["dense_tiles"] > st["tiles"] // 2 and st["num_pairs"] >= 80000, st


# ---- properties on the bench's batches -------------------------------------------------------------------------
def _render(b, harm=None, bg=(0.0, 0.0, 0.0), max_pairs=None, scenes=None, leaves=False):
    import spfsplatv2_amd as spf
    pick = (lambda t: t) if scenes is None else (lambda t: t[scenes])
    harm = b.harmonics if harm is None else harm
    args = [pick(b.extrinsics), pick(b.intrinsics), pick(b.near), pick(b.far), b.image_shape,
            torch.tensor(bg, device="cuda"), pick(b.means), pick(harm), pick(b.opacities), pick(b.rotations),
            pick(b.scales)]
    return spf.render_views(*args, enable_cov_grad=True, enable_sh_grad=True, max_pairs=max_pairs)


@pytest.mark.parametrize("config,S,V,min_pairs_per_render,min_list",
                         [("C2", 8, 4, 60000, 257), ("C3", 2, 4, 200000, 1025), ("C5", 1, 8, 400000, 513),
                          ("REF10V", 3, 1, 500000, 2049)],
                         ids=["C4_share_8x4", "C3_2x4", "C5_1x8", "REF10V_3x1"])
def test_full_batch_properties(hip_lib, config, S, V, min_pairs_per_render, min_list, monkeypatch):
    import spfsplatv2_amd as spf
    b = syn.make_batch(config, S, V, seed=1000).to("cuda")
    K = b.harmonics.shape[-1]
    b.harmonics[..., 0] = b.harmonics[..., 0].abs() + 1.0       # colours stay > 0: no clamp, the image is linear in DC
    img, dep, alp = _render(b)
    st = spf.last_forward_stats()
    assert st["num_pairs"] >= min_pairs_per_render * S * V and st["max_tile_list"] >= min_list, st
    assert bool(torch.isfinite(img).all()) and bool(torch.isfinite(dep).all())
    assert float(alp.min()) >= 0.0 and float(alp.max()) <= 1.0 and float(alp.mean()) > 0.3
    img2, dep2, _ = _render(b)
    assert torch.equal(img, img2) and torch.equal(dep, dep2)                                  # bit-stable forward
    bgc = (0.3, 0.6, 0.9)
    img_bg, _, _ = _render(b, bg=bgc)                                                         # out = C + T_final * bg
    assert float((img_bg - img - (1 - alp) * torch.tensor(bgc, device="cuda")[None, None, :, None, None])
                 .abs().max()) < 2e-6
    # a scene rendered inside the batch == the scene rendered alone: renders are independent, which is the whole
    # multi-GPU story (scene-first sharding needs no data-path collective)
    for s in sorted({0, S - 1}):
        solo, solo_d, _ = _render(b, scenes=[s])
        assert torch.equal(solo[0], img[s]) and torch.equal(solo_d[0], dep[s]), s
    # planned mode (no host read-back) gives the same pixels as exact mode
    # -- a planned call runs with DIRECT BINS (the projection kernel bins: no tile scan, no binning pass); the same plan
    # on the classic chain (SPF_DIRECT_BINS=0: packed lists) must give the same pixels too
    plan = spf.plan_pair_budget(st, check="deferred")
    img_p, dep_p, _ = _render(b, max_pairs=plan)
    assert spf.last_plan_flags() == 0 and torch.equal(img_p, img) and torch.equal(dep_p, dep)
    monkeypatch.setenv("SPF_DIRECT_BINS", "0")
    img_c, dep_c, _ = _render(b, max_pairs=plan)
    monkeypatch.delenv("SPF_DIRECT_BINS")
    assert spf.last_plan_flags() == 0 and torch.equal(img_c, img) and torch.equal(dep_c, dep)
    # gradient checksum: loss = sum(image), bg = 0  =>  d loss / d DC coefficient of (g, c) = SH_C0 * sum_pixels w_g,
    # so sum_g of it / SH_C0 = sum_pixels (1 - T_final) = sum(alpha), per scene and channel -- a checksum over every
    # (Gaussian, tile) pair of binning, sort order, compositing, pair records and the per-Gaussian reduction
    harm = b.harmonics.clone().requires_grad_(True)
    opac_leaf = b.opacities.clone().requires_grad_(True)
    b2 = syn.Batch(**{**b.__dict__, "opacities": opac_leaf})
    i2, _, a2 = _render(b2, harm=harm)
    i2.sum().backward()
    got = harm.grad[..., 0].sum(dim=1) / SH_C0                                                # [S,3]
    want = a2.detach().sum(dim=(1, 2, 3, 4))                                                  # [S]
    assert float(((got - want[:, None]).abs() / want[:, None]).max()) < 2e-4
    if K > 1:
        assert float(harm.grad[..., 1:].abs().max()) > 0
    assert bool(torch.isfinite(opac_leaf.grad).all()) and float(opac_leaf.grad.abs().max()) > 0


def test_back_to_back_steps_are_bit_stable(hip_lib):
    """120 planned-mode steps (decoder forward + backward) queued with no host synchronisation in between: every step
    must reproduce the first one bit for bit.  This is what the bench's timed region does, and what exposed a
    one-in-a-million LDS reuse race in the lists backward (a wave that ran with its own idea of the list's end: a
    barrier mismatch, then a read of `pairs` at index -1) -- four 50-step trials out of five failed with it."""
    import spfsplatv2_amd as spf
    b = syn.make_batch("C2", 8, 4, seed=1000).to("cuda")
    leaves = {n: getattr(b, n).clone().requires_grad_(True) for n in ("means", "harmonics", "opacities", "extrinsics")}

    def step(max_pairs):
        for t in leaves.values():
            t.grad = None
        img, _, _ = spf.render_views(leaves["extrinsics"], b.intrinsics, b.near, b.far, b.image_shape,
                                     torch.zeros(3, device="cuda"), leaves["means"], leaves["harmonics"],
                                     leaves["opacities"], b.rotations, b.scales, enable_cov_grad=True,
                                     enable_sh_grad=True, max_pairs=max_pairs)
        spf.mse_loss(img, b.target).backward()
        return img.detach(), {n: t.grad for n, t in leaves.items()}

    step(None)
    plan = spf.plan_pair_budget(spf.last_forward_stats(), check="deferred")
    img0, g0 = step(plan)
    last = None
    for _ in range(120):
        last = step(plan)
    torch.cuda.synchronize()
    assert spf.last_plan_flags() == 0
    assert torch.equal(last[0], img0)
    for n in g0:
        assert bool(torch.isfinite(last[1][n]).all()) and torch.equal(last[1][n], g0[n]), n


# ---- pose-only backward (test_step_align) ----------------------------------------------------------------------
def test_pose_alignment_only_extrinsics_require_grad(hip_lib):
    """model_wrapper.py:549-588: `extrinsics = nn.Parameter(...)`, Adam(lr = test.opt_lr = 0.005), every step =
    decoder.forward + MSE + backward; the Gaussians are frozen encoder outputs, so gradient flows ONLY into the poses
    (rasterizer.py: want["view"] = "partials", everything else off)."""
    from oracle import glue_ref
    from spfsplatv2_amd import decoder as dec, loss as spf_loss
    batch = syn.make_batch("TEST", 1, 2, seed=41, s_mult=6.0, G=1500, K=4, image_hw=(64, 64))
    steps, lr = 3, 0.005

    def align_oracle():
        ext = torch.nn.Parameter(batch.extrinsics.clone().double())
        opt = torch.optim.Adam([{"params": [ext], "lr": lr}])
        losses, grads = [], []
        d = lambda t: t.double()
        for _ in range(steps):
            opt.zero_grad()
            color = glue_ref.decoder_forward(d(batch.means), d(batch.harmonics), d(batch.opacities),
                                             d(batch.rotations), d(batch.scales), ext, d(batch.intrinsics),
                                             d(batch.near), d(batch.far), batch.image_shape, (0.0, 0.0, 0.0),
                                             dtype=torch.float64)[0]
            loss = ((color - d(batch.target)) ** 2).mean()
            loss.backward()
            losses.append(float(loss.detach()))
            grads.append(ext.grad.clone())
            opt.step()
        return ext.detach(), losses, grads

    def align_product():
        b = batch.to("cuda")
        decoder = util.product_decoder()
        g = dec.Gaussians(b.means, b.covariances, b.rotations, b.scales, b.harmonics, b.opacities)
        assert not any(t.requires_grad for t in (g.means, g.rotations, g.scales, g.harmonics, g.opacities))
        mse = spf_loss.LossMse(spf_loss.LossMseCfgWrapper(spf_loss.LossMseCfg(weight=1.0, apply_after_step=0)))
        ext = torch.nn.Parameter(b.extrinsics.clone())
        opt = torch.optim.Adam([{"params": [ext], "lr": lr}])
        losses, grads = [], []
        for _ in range(steps):
            opt.zero_grad()
            out = decoder.forward(g, ext, b.intrinsics, b.near, b.far, b.image_shape)
            loss = mse.forward(out.color, b.target, g, 0)
            loss.backward()
            losses.append(float(loss.detach()))
            grads.append(ext.grad.clone().cpu())
            opt.step()
        return ext.detach().cpu(), losses, grads

    e_ref, l_ref, g_ref = align_oracle()
    e_got, l_got, g_got = align_product()
    assert util.rel_linf(g_got[0], g_ref[0]) < 1e-3, "first-step pose gradient"
    for a, r in zip(l_got, l_ref):
        assert abs(a - r) / r < 1e-5, (l_got, l_ref)
    assert l_got[-1] < l_got[0]                                         # it actually aligns
    assert float((e_got.double() - e_ref).abs().max()) < 5e-5           # 1 % of one Adam step
    assert float((e_got - batch.extrinsics).abs().max()) > 0.5 * lr * steps


# ---- d_sh = 25 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("band4", [False, True], ids=["k25_stride_only", "k25_deg4"])
def test_parity_k25_with_and_without_band4(hip_lib, band4):
    batch = syn.make_batch("TEST", 2, 2, seed=6, s_mult=10.0, G=1200, K=25, image_hw=(64, 48))
    batch.harmonics[..., 1:] *= 4.0                      # make the view-dependent part (and band 4) clearly visible
    ref = util.run_oracle(batch, torch.float64, background=(0.2, 0.1, 0.3), mask_fragile=True, band4=band4)
    prod = util.run_product(batch, background=(0.2, 0.1, 0.3), pixel_mask=ref["pixel_mask"], band4=band4)
    rep = util.compare(prod, ref)
    assert not rep["fails"], rep
    hg = prod["grads"]["harmonics"]
    assert (float(hg[..., 16:].abs().max()) > 0) == band4           # band-4 coefficients get gradient only on request
    other = util.run_oracle(batch, torch.float64, background=(0.2, 0.1, 0.3), with_grads=False, want_fragile=False,
                            band4=not band4)
    assert float((other["color"] - ref["color"]).abs().max()) > 1e-3   # the two conventions really differ here


@pytest.mark.parametrize("band4", [False, True], ids=["split_deg3", "split_deg4"])
def test_band_split_harmonics_are_the_dense_layout_bit_for_bit(hip_lib, band4):
    """`Gaussians.harmonics_band4` (SpfDims.sh_layout 2: planes [.,3,16] | [.,3,9], what the fused adapter writes with
    split_harmonics=True): the same coefficients in another place -- images and every gradient are BIT-identical to the
    reference layout's [.,3,25], with band 4 evaluated or not, and hold against the oracle like it; a degree-3
    evaluation hands NO gradient to the band-4 plane (not a zero tensor: nothing is written for it)."""
    batch = syn.make_batch("TEST", 2, 2, seed=6, s_mult=10.0, G=1200, K=25, image_hw=(64, 48))
    batch.harmonics[..., 1:] *= 4.0
    ref = util.run_oracle(batch, torch.float64, background=(0.2, 0.1, 0.3), mask_fragile=True, band4=band4)
    dense = util.run_product(batch, background=(0.2, 0.1, 0.3), pixel_mask=ref["pixel_mask"], band4=band4)
    split = util.run_product(batch, background=(0.2, 0.1, 0.3), pixel_mask=ref["pixel_mask"], band4=band4, split=True)
    rep = util.compare(split, ref)
    assert not rep["fails"], rep
    # degree 3: the SAME kernel instantiation reads plane 0 as a K = 16 block -> bit-identical.  Degree 4 runs the split
    # instantiation of the kernels (two base pointers): the same sums in the same order, but the compiler is free to
    # contract a multiply-add differently from one instantiation to the next -> equal to a few ulp
    same = torch.equal if not band4 else (lambda a, b: util.rel_linf(a, b) < 2e-6)
    for k in ("color", "depth", "alpha", "radii"):
        assert same(split[k], dense[k]), (k, util.rel_linf(split[k], dense[k]))
    for n in util.GRAD_NAMES:
        assert same(split["grads"][n], dense["grads"][n]), (n, util.rel_linf(split["grads"][n], dense["grads"][n]))
    assert (float(split["grads"]["harmonics"][..., 16:].abs().max()) > 0) == band4


def test_band_split_degree3_leaves_band4_without_a_gradient(hip_lib):
    import spfsplatv2_amd as spf
    b = syn.make_batch("TEST", 1, 2, seed=8, s_mult=10.0, G=700, K=25, image_hw=(48, 48)).to("cuda")
    low = b.harmonics[..., :16].contiguous().requires_grad_(True)
    high = b.harmonics[..., 16:].contiguous().requires_grad_(True)
    d = util.product_decoder(band4=False)
    out = d(spf.Gaussians(b.means, None, b.rotations, b.scales, low, b.opacities, harmonics_band4=high),
            b.extrinsics, b.intrinsics, b.near, b.far, b.image_shape)
    out.color.square().mean().backward()
    assert high.grad is None and float(low.grad.abs().max()) > 0
    with pytest.raises(RuntimeError, match="3, 16"):             # the planes go together: [.,3,16] with [.,3,9]
        d(spf.Gaussians(b.means, None, b.rotations, b.scales, b.harmonics, b.opacities, harmonics_band4=high),
          b.extrinsics, b.intrinsics, b.near, b.far, b.image_shape)


def test_band4_switches(hip_lib, monkeypatch):
    """Default: SPF_SH_BAND4 unset -> degree 3; the environment variable, the decoder attribute and the settings field
    all turn it on."""
    import spfsplatv2_amd as spf
    b = syn.make_batch("TEST", 1, 1, seed=6, s_mult=10.0, G=600, K=25, image_hw=(48, 48)).to("cuda")
    b.harmonics[..., 1:] *= 4.0
    args = (b.extrinsics, b.intrinsics, b.near, b.far, b.image_shape, torch.zeros(3, device="cuda"), b.means,
            b.harmonics, b.opacities, b.rotations, b.scales)
    monkeypatch.delenv("SPF_SH_BAND4", raising=False)
    base = spf.render_views(*args)[0]
    on = spf.render_views(*args, sh_band4=True)[0]
    assert float((on - base).abs().max()) > 1e-3
    assert torch.equal(spf.render_views(*args, sh_band4=False)[0], base)
    monkeypatch.setenv("SPF_SH_BAND4", "1")
    assert torch.equal(spf.render_views(*args)[0], on)


def test_direct_bins_give_the_gradients_of_the_classic_chain(hip_lib, monkeypatch):
    """Planned calls bin inside the projection kernel (direct bins, SpfDims.bin_cap).  Same lists, same sort, same
    compositing: every output and every gradient must equal the exact-mode call's and the classic planned chain's
    (SPF_DIRECT_BINS=0) -- bit for bit where no dense tile's LDS float atomics are involved (s_mult = 1), to 1e-5 of
    scale otherwise; also with several view groups per block (V = 9 views at 512x512: three groups of three)."""
    import spfsplatv2_amd as spf
    for cfg, S, V, kw, exact_bits in (("C2", 3, 4, {}, True), ("C5", 1, 9, dict(G=60000), False),
                                      ("TEST", 2, 3, dict(s_mult=12.0, G=3000, K=4, image_hw=(96, 80)), False)):
        batch = syn.make_batch(cfg, S, V, seed=77, **kw)
        exact = util.run_product(batch)
        plan = spf.plan_pair_budget(exact["stats"], check="deferred")
        direct = util.run_product(batch, max_pairs=plan)
        assert spf.plan_flags(direct["decoder"].last_call) == 0
        monkeypatch.setenv("SPF_DIRECT_BINS", "0")
        classic = util.run_product(batch, max_pairs=plan)
        monkeypatch.delenv("SPF_DIRECT_BINS")
        assert spf.plan_flags(classic["decoder"].last_call) == 0
        for other in (exact, classic):
            for k in ("color", "depth", "alpha", "radii"):
                assert torch.equal(direct[k], other[k]), (cfg, k)
            for n in util.GRAD_NAMES:
                if exact_bits:
                    assert torch.equal(direct["grads"][n], other["grads"][n]), (cfg, n)
                else:
                    assert util.rel_linf(direct["grads"][n], other["grads"][n]) < 1e-5, (cfg, n)


def test_longest_first_launch_order_changes_nothing(hip_lib, monkeypatch):
    """Planned calls of 2,048 tiles or more hand the composite lists kernels their tiles longest list first
    (spf_common.h::tile_order_ptr; eight blocks in front of the tile sort's first kernel write the order).  Tiles are
    independent: every output and every gradient must be bit-identical with SPF_TILE_ORDER=0 -- through each of the
    sort kernels that can carry the order blocks (pair: many tiles; mixed: few tiles, long lists; wave: pinned by
    SPF_SORT_SINGLE), with dense tiles in the call, and when the call has exactly eight renders, whose tiles are dealt
    out to the XCDs in strips (spf_common.h::xcd_map: the C3 case here, and one 512 x 512 call of eight views)."""
    import spfsplatv2_amd as spf
    cases = (("C2", 8, 4, {}, {}),                                                  # 8,192 tiles: pair kernel
             ("C3", 2, 4, dict(G=120000), {}),                                      # 2,048 tiles, lists > 512: mixed kernel
             ("C2", 3, 4, {}, {"SPF_SORT_SINGLE": "1"}),                            # wave kernels
             ("C2", 2, 4, dict(s_mult=10.0, G=20000), {}),                          # dense tiles among them
             ("C5", 1, 8, dict(G=80000), {}))                                       # 8 renders of 1,024 tiles: strips dealt
    for cfg, S, V, kw, env in cases:
        batch = syn.make_batch(cfg, S, V, seed=91, **kw)
        exact = util.run_product(batch)
        plan = spf.plan_pair_budget(exact["stats"], check="deferred")
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ordered = util.run_product(batch, max_pairs=plan)
        assert spf.plan_flags(ordered["decoder"].last_call) == 0
        monkeypatch.setenv("SPF_TILE_ORDER", "0")
        plain = util.run_product(batch, max_pairs=plan)
        monkeypatch.delenv("SPF_TILE_ORDER")
        for k in env:
            monkeypatch.delenv(k)
        dense = exact["stats"]["dense_tiles"] > 0
        for k in ("color", "depth", "alpha", "radii"):
            assert torch.equal(ordered[k], plain[k]), (cfg, k)
        for n in util.GRAD_NAMES:
            if dense:                                         # (dense tiles: LDS float atomics, run-to-run ~1e-7)
                assert util.rel_linf(ordered["grads"][n], plain["grads"][n]) < 1e-5, (cfg, n)
            else:
                assert torch.equal(ordered["grads"][n], plain["grads"][n]), (cfg, n)


def test_forward_does_not_depend_on_the_form_that_composites_a_tile(hip_lib, monkeypatch):
    """A tile is composited in the "lists" or the "rows" form (render.hip), chosen per direction from its mean footprint
    (SPF_DENSE_AREA_FWD 120 / SPF_DENSE_AREA 26 px): all forms evaluate alpha with ONE expression tree, so the forward's
    images, depth, alpha -- and the per-pixel state the backward replays from -- are bit-identical whichever form ran, and
    the backward takes the forward's hit decisions whichever pair of forms a tile met.  Gradients agree to rounding (the
    two backward forms sum in different orders)."""
    import spfsplatv2_amd as spf
    forms = {"lists/lists": ("1000000000", "1000000000"), "rows/rows": ("1", "1"), "lists/rows": ("1", "1000000000"),
             "default": (None, None)}
    for cfg, S, V, kw in (("C2", 2, 4, dict(s_mult=6.0, G=20000)), ("C3", 1, 2, dict(s_mult=3.0, G=60000)),
                          ("TEST", 2, 2, dict(s_mult=15.0, G=2500, K=4, image_hw=(72, 100)))):
        batch = syn.make_batch(cfg, S, V, seed=93, **kw)
        exact = util.run_product(batch)
        plan = spf.plan_pair_budget(exact["stats"], check="deferred")
        res = {}
        for name, (bwd, fwd) in forms.items():
            for k, v in (("SPF_DENSE_AREA", bwd), ("SPF_DENSE_AREA_FWD", fwd)):
                monkeypatch.setenv(k, v) if v is not None else monkeypatch.delenv(k, raising=False)
            res[name] = util.run_product(batch, max_pairs=plan)
            assert spf.plan_flags(res[name]["decoder"].last_call) == 0
        monkeypatch.delenv("SPF_DENSE_AREA", raising=False)
        monkeypatch.delenv("SPF_DENSE_AREA_FWD", raising=False)
        for name, r in res.items():
            for k in ("color", "depth", "alpha", "radii"):
                assert torch.equal(r[k], res["lists/lists"][k]), (cfg, name, k)
            for n in util.GRAD_NAMES:
                assert util.rel_linf(r["grads"][n], res["lists/lists"]["grads"][n]) < 2e-5, (cfg, name, n)


def test_backward_round_shapes_give_identical_gradients(hip_lib, monkeypatch):
    """The lists backward comes in three round shapes (entries per round / slot pool / blocks per CU: 192 / 1,536 / 5 for
    many tiles, 224 / 1,792 / 4 up to 2,048 tiles, 256 / 2,560 / 3 up to 768: render.hip) picked by the number of tiles of
    the call.  A pixel replays its contributors in list order and an entry sums its slots in pixel order whatever the
    round boundaries are: every gradient must be bit-identical across the three -- on a call of few tiles with lists of
    thousands of entries (the regime the long rounds are for) and on an ordinary one."""
    for cfg, S, V, kw in (("TESTBIG", 1, 2, dict(G=60000, image_hw=(48, 64))), ("C2", 2, 2, {})):
        batch = syn.make_batch(cfg, S, V, seed=123, **kw)
        got = {}
        for shape in ("192", "224", "256"):
            monkeypatch.setenv("SPF_BWD_ROUNDS", shape)
            got[shape] = util.run_product(batch)
        monkeypatch.delenv("SPF_BWD_ROUNDS")
        default = util.run_product(batch)
        assert default["stats"]["dense_tiles"] == 0
        for shape in ("224", "256"):
            for n in util.GRAD_NAMES:
                assert torch.equal(got[shape]["grads"][n], got["192"]["grads"][n]), (cfg, shape, n)
        for n in util.GRAD_NAMES:
            assert torch.equal(default["grads"][n], got["192"]["grads"][n]), (cfg, n)
        # the forward lists kernel stages 256 or 512 entries per round (calls of <= 2,048 tiles: 512): same pixels, same
        # last contributors, hence the same gradients, bit for bit
        for stage in ("256", "512"):
            monkeypatch.setenv("SPF_FWD_STAGE", stage)
            other = util.run_product(batch)
            monkeypatch.delenv("SPF_FWD_STAGE")
            for k in ("color", "depth", "alpha"):
                assert torch.equal(other[k], default[k]), (cfg, stage, k)
            for n in util.GRAD_NAMES:
                assert torch.equal(other["grads"][n], default["grads"][n]), (cfg, stage, n)


def test_ordered_planned_call_against_the_oracle(hip_lib):
    """The path the bench runs -- a planned call on direct bins whose composite kernels take their tiles from the launch
    order -- held against the float64 oracle itself, not only against the exact-mode call: 32 renders of 128 x 128
    (2,048 tiles, the smallest call that gets an order), the ordinary gates."""
    import spfsplatv2_amd as spf
    batch = syn.make_batch("TEST", 4, 8, seed=57, s_mult=4.0, G=2500, K=4, image_hw=(128, 128))
    ref = util.run_oracle(batch, torch.float64, mask_fragile=True)
    exact = util.run_product(batch, pixel_mask=ref["pixel_mask"])
    assert exact["stats"]["tiles"] == 2048
    plan = spf.plan_pair_budget(exact["stats"], check="deferred")
    prod = util.run_product(batch, max_pairs=plan, pixel_mask=ref["pixel_mask"])
    assert spf.plan_flags(prod["decoder"].last_call) == 0
    rep = util.compare(prod, ref, max_fragile_frac=0.01)
    from tests.test_gpu_raster import _report
    _report("ordered_planned_32x128", rep)
    assert not rep["fails"], rep


# ---- failed plans ----------------------------------------------------------------------------------------------
def test_failed_plan_is_nan_everywhere_and_raises_without_backward(hip_lib):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd._lib import SpfError
    batch = syn.make_batch("TEST", 2, 3, seed=3, s_mult=8.0, G=1500, K=4, image_hw=(80, 112))
    exact = util.run_product(batch)
    st = exact["stats"]
    good = spf.plan_pair_budget(st, check="deferred")
    bad_plans = {1: good._replace(capacity=st["num_pairs"] // 2),
                 2: good._replace(max_tile_list=max(st["max_tile_list"] // 2, 1))}
    for bit, plan in bad_plans.items():
        res = util.run_product(batch, max_pairs=plan)
        assert spf.plan_flags(res["decoder"].last_call) & bit
        for k in ("color", "depth", "alpha"):
            assert bool(torch.isnan(res[k]).all()), (bit, k)           # never uninitialised memory
        for n, g in res["grads"].items():
            assert bool(torch.isnan(g).all()), (bit, n)
        # check="backward" with no backward to come (evaluation): the forward itself verifies and raises
        with pytest.raises(SpfError):
            with torch.no_grad():
                util.run_product(batch, max_pairs=plan._replace(check="backward"), with_grads=False)
    ok = util.run_product(batch, max_pairs=good)
    assert spf.plan_flags(ok["decoder"].last_call) == 0 and torch.equal(ok["color"], exact["color"])


@pytest.mark.parametrize("config,S,V,chunks", [("C2", 8, 4, 4), ("C2", 3, 2, 2), ("C5", 1, 4, 2)])
def test_chunked_two_lane_chains_are_bit_identical(hip_lib, config, S, V, chunks, monkeypatch):
    """SPF_CHUNKS=n (spf_raster_chunks; off by default: measured slower) runs a call as n chunks of renders on two
    streams.  Same launchers on offset pointers: images and every gradient equal the single chain bit for bit, with
    whole scenes per chunk (backward chunked too), a scene count that does not divide evenly, and a single scene
    (forward chunked by views, backward as one chain)."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import _lib
    b = syn.make_batch(config, S, V, seed=77).to("cuda")
    names = ("means", "scales", "rotations", "opacities", "harmonics", "extrinsics")

    def run():
        leaves = {n: getattr(b, n).clone().requires_grad_(True) for n in names}
        img, dep, alp = spf.render_views(leaves["extrinsics"], b.intrinsics, b.near, b.far, b.image_shape,
                                         torch.zeros(3, device="cuda"), leaves["means"], leaves["harmonics"],
                                         leaves["opacities"], leaves["rotations"], leaves["scales"],
                                         enable_cov_grad=True, enable_sh_grad=True)
        (spf.mse_loss(img, b.target) + 0.01 * dep.mean() + 0.1 * alp.mean()).backward()
        return img.detach(), dep.detach(), {n: t.grad for n, t in leaves.items()}

    monkeypatch.delenv("SPF_CHUNKS", raising=False)
    h, w = b.image_shape
    assert _lib.load().spf_raster_chunks(S, V, h, w, 0) == 1
    img1, dep1, g1 = run()
    _, _, g1b = run()
    # (dense tiles -- C5 has a few -- sum their partial gradients with LDS float atomics: run-to-run ~1e-7)
    deterministic = all(torch.equal(g1[n], g1b[n]) for n in names)
    monkeypatch.setenv("SPF_CHUNKS", str(chunks))
    assert _lib.load().spf_raster_chunks(S, V, h, w, 0) == chunks
    assert _lib.load().spf_raster_chunks(S, V, h, w, 1) == (chunks if S > 1 else 1)
    img2, dep2, g2 = run()
    torch.cuda.synchronize()
    assert torch.equal(img1, img2) and torch.equal(dep1, dep2)
    for n in names:
        assert torch.equal(g1[n], g2[n]) if deterministic else util.rel_linf(g2[n], g1[n]) < 1e-5, n
