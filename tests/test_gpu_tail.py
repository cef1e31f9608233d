"""The encoder tail on the device (csrc/tail.hip, spfsplatv2_amd/tail.py).

Gate (tests/tail_cases.py, the rule of tests/block_cases.py): per tensor err = max|x - x64| / max|x64| against the float64
oracle must not exceed twice the err of float32 eager torch on the device plus one float32 ulp; before a gate is trusted
the power condition of tests/test_tail.py is asserted again with the device's eager figures.  Every figure is printed.
"""
import pytest
import torch

from tests import tail_cases as cases
from tests import tail_oracle as to

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- the product -----------------------------------------------------------------------------------------------------
def run_product(case, d, split=False, absent=(), pts=None, raw=None):
    """``gaussians_from_heads`` and its backward in the form of ``tail_oracle.tail_with_grads``; the band-split planes
    are joined to [.., 3, 25].  ``absent``: the outputs that get no upstream gradient."""
    import spfsplatv2_amd as spf
    b, v, hw, deg, e = case
    pts = [t.to(DEV).requires_grad_(True) for t in d["pts"]] if pts is None else pts
    raw = [t.to(DEV).requires_grad_(True) for t in d["raw"]] if raw is None else raw
    g = spf.gaussians_from_heads(pts, raw, e, sh_degree=deg, eps=cases.EPS, split_harmonics=split)
    outs = {"means": g.means, "opacities": g.opacities, "scales": g.scales, "rotations": g.rotations, "harmonics": g.harmonics}
    ups = {k: d["ups"][k].to(DEV) for k in to.OUTPUTS}
    if split:
        assert g.harmonics.shape[-1] == 16 and g.harmonics_band4.shape[-1] == 9
        outs["harmonics_band4"] = g.harmonics_band4
        ups["harmonics"], ups["harmonics_band4"] = ups["harmonics"][..., :16].contiguous(), ups["harmonics"][..., 16:].contiguous()
    else:
        assert g.harmonics_band4 is None
    for k, t in outs.items():
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[:2] == (b, v * hw[0] * hw[1]), k
    names = [k for k in outs if k not in absent]
    grads = torch.autograd.grad([outs[k] for k in names], pts + raw, [ups[k] for k in names])
    for gr, t in zip(grads, pts + raw):
        assert gr.shape == t.shape and gr.is_contiguous()
    res = {k: t.detach() for k, t in outs.items()}
    if split:
        res["harmonics"] = torch.cat((res["harmonics"], res.pop("harmonics_band4")), dim=-1)
    res["d_pts"], res["d_raw"] = torch.stack(grads[:v]), torch.stack(grads[v:])
    return res


def check(case, split=False, muts=None):
    d, x64, dists = cases.reference(case, muts)
    got = cases.split(run_product(case, d, split), d["tiny"])
    label = cases.case_id(case) + (" split" if split else "")
    cases.gate(label, got, cases.oracle(case, d, torch.float32, DEV), x64, dists)
    return d, got


# ---- a. the gate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.covering_cases(), ids=cases.case_id)
def test_tail_against_oracle(case):
    """Every (h, w) of tests/tail_cases.py with every K: one pixel, scalar tails, one tile, a tile plus one, a partial
    tile on the vector path, several tiles; b in {1, 2}, v in {1, 2, 3} and the four exponents cycled."""
    check(case)


@pytest.mark.parametrize("case", cases.SPLIT_CASES, ids=cases.case_id)
def test_tail_band_split_against_oracle(case):
    check(case, split=True)


def test_tile_loop_of_a_capped_grid():
    """Three more tiles than the grid has blocks: the first three blocks take a second tile."""
    from spfsplatv2_amd import tail
    case = cases.loop_case(tail.max_grid())
    assert case[2][0] * case[2][1] == (tail.max_grid() + 3) * 64
    check(case, muts=("no_half", "clamp_min", "channel_off_by_one"))


@pytest.mark.parametrize("absent,split", [(k, False) for k in to.OUTPUTS] + [(k, True) for k in to.OUTPUTS + ("harmonics_band4",)],
                         ids=lambda x: x if isinstance(x, str) else ("split" if x else "dense"))
def test_each_upstream_gradient_absent_in_turn(absent, split):
    """The gradients that remain go through the gate against the oracle given the same upstream gradients; what the
    absent one alone feeds is an exact zero (band 4's channels under the split, without its plane's gradient)."""
    case = cases.ABSENT_CASE
    d = cases.inputs(case)
    ups = dict(d["ups"])
    if absent == "harmonics_band4":
        ups["harmonics"] = ups["harmonics"].clone()
        ups["harmonics"][..., 16:] = 0.0
    elif absent == "harmonics" and split:
        ups["harmonics"] = ups["harmonics"].clone()
        ups["harmonics"][..., :16] = 0.0
    else:
        ups[absent] = None
    x64 = cases.oracle(case, d, ups=ups)
    eager = cases.oracle(case, d, torch.float32, DEV, ups=ups)
    got = cases.split(run_product(case, d, split, absent=(absent,)), d["tiny"])
    zero = [k for k, t in x64.items() if not t.any()]
    assert zero == {"means": ["d_pts"], "opacities": ["d_density"], "scales": ["d_scale"], "rotations": ["d_quat", "d_quat_tiny"],
                    "harmonics": [] if split else ["d_sh"], "harmonics_band4": []}[absent]
    for k in zero:
        assert not got[k].any(), k
    if absent == "harmonics_band4":
        assert not got["d_sh"].unflatten(2, (3, 25))[:, :, :, 16:].any() and got["d_sh"].any()
    if absent == "harmonics" and split:
        assert not got["d_sh"].unflatten(2, (3, 25))[:, :, :, :16].any() and got["d_sh"].any()
    keep = lambda r: {k: t for k, t in r.items() if k not in zero}
    cases.gate(f"{cases.case_id(case)} without d_{absent}" + (" split" if split else ""), keep(got), keep(eager), keep(x64), {})


# ---- b. saturated logits ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [0.5, 2.0])
def test_saturated_logits_give_finite_gradients(e):
    """Logits -200, -104, -30, 17, 30, 200 in the density channel: outputs and gradients finite, the density gradient
    within 4 ulp of the largest gradient of the float64 stable oracle; eager float32 on the reference's expression is
    printed next to them (NaN at 17, 30 and 200 for e = 0.5, at -104 and -200 for e = 2)."""
    case = (1, 1, (1, 8), 0, e)
    d = dict(cases.inputs(case))
    sat = torch.tensor([-200.0, -104.0, -30.0, 17.0, 30.0, 200.0])
    d["raw"] = [d["raw"][0].clone()]
    d["raw"][0][0, 0, 0, :6] = sat
    x64 = cases.oracle(case, d)
    got = cases.split(run_product(case, d), d["tiny"])
    naive = cases.oracle(case, d, torch.float32, DEV, opacity=to.opacity_naive)
    for k, t in got.items():
        assert torch.isfinite(t).all(), k
    scale = float(x64["d_density"].abs().max())
    for i, x in enumerate(sat.tolist()):
        gp, g64, gn = float(got["d_density"][0, 0, 0, i]), float(x64["d_density"][0, 0, 0, i]), float(naive["d_density"][0, 0, 0, i])
        print(f"e = {e} logit {x:+.0f}: product {gp:.6e} float64 {g64:.6e} eager float32, reference's expression {gn:.6e}")
    assert float((got["d_density"].double().cpu() - x64["d_density"]).abs().max()) <= 4 * cases.ULP * scale
    assert float((got["opacities"].double().cpu() - x64["opacities"]).abs().max()) <= 4 * cases.ULP
    assert bool(torch.isnan(naive["d_density"]).any())


def test_exponent_one_shortcut_is_the_general_path_to_rounding():
    """e == 1 skips the powers (p, and p (1 - p)); e = 1 + 2^-23, the next float32, takes the general path on the same
    logits.  The map moves by at most |d/de| 2^-23 <= 0.37 x 2^-23 between the two, so what separates them is rounding.
    Bound (derived, not measured): the general path rounds log p and log(1 - p) (half an ulp of their size, carried by
    the exp: at most half an ulp of 1 after the exp, since exp(y) |y| <= 0.37), two exps (2 ulp each in the device's
    libm, of values <= 1), and three additions and the halving (1.5 ulp): under 4 ulp of the tensor's largest entry, for
    the opacities and, with two more products per branch of values <= 1, for the density gradient as well."""
    import numpy as np
    case = (2, 2, (5, 13), 1, 1.0)
    d = cases.inputs(case)
    e_next = float(np.nextafter(np.float32(1.0), np.float32(2.0)))
    assert e_next != 1.0 and float(np.float32(e_next)) == e_next
    one = cases.split(run_product(case, d), d["tiny"])
    gen = cases.split(run_product((2, 2, (5, 13), 1, e_next), d), d["tiny"])
    for k in ("opacities", "d_density"):
        scale = float(one[k].abs().max())
        diff = float((one[k] - gen[k]).abs().max())
        print(f"e = 1 shortcut against e = 1 + 2^-23, {k}: max difference {diff:.3e} = {diff / (cases.ULP * scale):.2f} ulp of {scale:.3e}")
        assert diff <= 4 * cases.ULP * scale, k
    for k in one:
        if k not in ("opacities", "d_density"):
            assert torch.equal(one[k], gen[k]), k


def test_a_call_uploads_nothing_and_never_waits_for_the_stream(monkeypatch):
    """After the first call for an (sh_degree, device) the SH mask lives on the device: a step builds no host mask, copies
    nothing from the host and never synchronises (torch's sync debug mode turns a blocking host-to-device copy, a
    ``.item()`` or a stream wait into an error), in the function form and through ``GaussianTail`` alike."""
    import types

    import spfsplatv2_amd as spf
    from spfsplatv2_amd import adapter, tail
    case = (2, 2, (5, 13), 4, 2.0)
    d = cases.inputs(case)
    pts = [t.to(DEV).requires_grad_(True) for t in d["pts"]]
    raw = [t.to(DEV).requires_grad_(True) for t in d["raw"]]
    ups = [d["ups"][k].to(DEV) for k in ("means", "opacities", "scales", "rotations")] + [d["ups"]["harmonics"][..., :16].to(DEV).contiguous()]
    mod = spf.GaussianTail(adapter.GaussianAdapterCfg(0.5, 15.0, 4), types.SimpleNamespace(initial=0.0, final=2.0, warm_up=10),
                           split_harmonics=True)

    def step(call):
        g = call()
        return torch.autograd.grad([g.means, g.opacities, g.scales, g.rotations, g.harmonics], pts + raw, ups)

    calls = (lambda: mod(pts, raw, global_step=5), lambda: spf.gaussians_from_heads(pts, raw, 2.0, sh_degree=4, split_harmonics=True))
    want = [step(c) for c in calls]                                 # the first calls: the mask is made here
    mask = tail._device_mask(4, raw[0].device)
    assert mask.is_cuda and torch.equal(mask.cpu(), tail.sh_mask(4))
    torch.cuda.synchronize()

    def no_host_mask(*a, **k):
        raise AssertionError("a second call built the SH mask on the host")
    monkeypatch.setattr(tail, "sh_mask", no_host_mask)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [step(c) for c in calls]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tail._device_mask(4, raw[0].device) is mask
    for a, b in zip(want, got):
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---- c. bitwise ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["dense", "split"])
def test_bitwise_repeatable_and_equal_to_the_row_path_where_it_is_one_multiply(split):
    """Two runs are equal in every output and gradient.  ``harmonics`` equals the existing path's (torch.stack + the row
    adapter) bit for bit; scales and rotations are the same expressions, and whether they come out bitwise equal too is
    printed (the gate above is what they are held to)."""
    from spfsplatv2_amd import adapter
    case = (2, 3, (5, 13), 4, 2.0)
    d = cases.inputs(case)
    a, b = run_product(case, d, split), run_product(case, d, split)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    rows = torch.stack([r.to(DEV).flatten(2).transpose(1, 2) for r in d["raw"]], dim=1)           # [b, v, hw, 83]
    ad = adapter.UnifiedGaussianAdapter(adapter.GaussianAdapterCfg(0.5, 15.0, 4), split_harmonics=split).to(DEV)
    g = ad(a["means"].view(2, 3, 65, 3), a["opacities"].view(2, 3, 65), rows[..., 1:], eps=cases.EPS, with_covariances=False)
    sh = torch.cat((g.harmonics, g.harmonics_band4), dim=-1) if split else g.harmonics
    assert torch.equal(a["harmonics"], sh.reshape(2, -1, 3, 25))
    for k, t in (("scales", g.scales), ("rotations", g.rotations)):
        print(f"{k} bitwise equal to the row kernels': {torch.equal(a[k], t.reshape(a[k].shape))}")


# ---- d. in-place reads -----------------------------------------------------------------------------------------------
def test_head_outputs_are_read_in_place_or_copied_and_counted():
    from spfsplatv2_amd import tail
    case = (2, 2, (5, 13), 1, 2.0)
    d, x64, dists = cases.reference(case)
    C, h, w = 20, 5, 13
    # slices of one larger allocation at 16-byte aligned offsets: batch items 1..2 and 4..5 of a [7, C, h, w] tensor
    big = torch.zeros(7, C, h, w, device=DEV)
    assert (C * h * w * 4) % 16 == 0
    big[1:3], big[4:6] = d["raw"][0].to(DEV), d["raw"][1].to(DEV)
    raw = [big[1:3].requires_grad_(True), big[4:6].requires_grad_(True)]
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 0 and t.data_ptr() != big.data_ptr() for t in raw)
    before = dict(tail.dense_copies)
    got = cases.split(run_product(case, d, raw=raw), d["tiny"])
    assert tail.dense_copies == before
    eager = cases.oracle(case, d, torch.float32, DEV)
    cases.gate("slices in place", got, eager, x64, dists)
    # a permuted (channels-last) head output and a point map 4 bytes off: each copied once, and counted
    perm = d["raw"][0].to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    pad = torch.zeros(d["pts"][1].numel() + 1, device=DEV)
    pad[1:] = d["pts"][1].to(DEV).reshape(-1)
    off = pad[1:].view(d["pts"][1].shape).requires_grad_(True)
    assert not perm.is_contiguous() and off.is_contiguous() and off.data_ptr() % 16 != 0
    raw = [perm, d["raw"][1].to(DEV).requires_grad_(True)]
    pts = [d["pts"][0].to(DEV).requires_grad_(True), off]
    got = cases.split(run_product(case, d, pts=pts, raw=raw), d["tiny"])
    assert tail.dense_copies["calls"] - before["calls"] == 2
    assert tail.dense_copies["bytes"] - before["bytes"] == 4 * (perm.numel() + off.numel())
    cases.gate("permuted and misaligned", got, eager, x64, dists)


# ---- e. the opacity map alone ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", cases.EXPONENTS)
def test_density_to_opacity_on_channel_0_of_rows(e):
    """Channel 0 of a [2, 5, 7, 83] tensor, read in place at a stride of 83: the gate, and the gradient lands in channel 0
    alone."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import tail
    gen = torch.Generator().manual_seed(83)
    rows = torch.randn(2, 5, 7, 83, generator=gen)
    rows[..., 0] = (3.0 * rows[..., 0]).clamp(-12.0, 12.0)
    rows[0, 0, :3, 0] = torch.tensor([-12.0, 12.0, 0.0])
    up = torch.randn(2, 5, 7, generator=gen)

    def ref(dtype, device, mut=to.NONE):
        x = rows.to(device=device, dtype=dtype).requires_grad_(True)
        y = to.opacity_stable(x[..., 0], e, mut)
        (gx,) = torch.autograd.grad(y, x, up.to(device=device, dtype=dtype))
        return {"opacities": y.detach(), "d_density": gx[..., 0], "rest": gx[..., 1:]}

    x = rows.to(DEV).requires_grad_(True)
    before = dict(tail.dense_copies)
    y = spf.density_to_opacity(x[..., 0], e)
    assert tail.dense_copies == before and y.shape == (2, 5, 7) and y.is_contiguous()
    (gx,) = torch.autograd.grad(y, x, up.to(DEV))
    assert not gx[..., 1:].any() and gx[..., 0].any()
    x64, eager = ref(torch.float64, "cpu"), ref(torch.float32, DEV)
    pick = lambda r: {k: r[k] for k in ("opacities", "d_density")}
    muts = ("no_half", "no_sigmoid") + (("inv_exponent",) if e != 1.0 else ())
    dists = {m: {k: to.rel_err(v, x64[k]) for k, v in pick(ref(torch.float64, "cpu", frozenset([m]))).items()} for m in muts}
    cases.gate(f"density_to_opacity e = {e:.3g}", {"opacities": y.detach(), "d_density": gx[..., 0]}, pick(eager), pick(x64), dists)
    # any other view: a permuted one has no single stride and is copied, counted
    z = spf.density_to_opacity(x[..., 0].permute(2, 0, 1), e)
    assert tail.dense_copies["calls"] - before["calls"] == 1 and torch.equal(z, y.detach().permute(2, 0, 1))


# ---- f. through the decoder ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True], ids=["dense", "split"])
def test_gaussians_from_heads_render_through_the_decoder(split):
    """b = 1, two 16 x 16 views, K = 25: the ``Gaussians`` of ``gaussians_from_heads`` go straight into
    ``DecoderSplattingCUDA``; image and the gradients at the head outputs agree with the existing path (rearrange, stack,
    sigmoid, map, slice, ``UnifiedGaussianAdapter``, decoder) within the decoder's documented parity: 1e-4 on RGB, 1e-3
    of scale on the gradients."""
    import types

    import spfsplatv2_amd as spf
    from spfsplatv2_amd import adapter, synthetic as syn
    from tests import util
    v, h, w, K = 2, 16, 16, 25
    G = v * h * w
    bt = syn.make_batch("TEST", 1, 2, seed=77, s_mult=8.0, G=G, K=K, image_hw=(48, 48)).to(DEV)
    y = (bt.scales.double() / 0.001).clamp_min(1e-12)
    raw_scales = torch.where(y > 20.0, y, torch.log(torch.expm1(y.clamp_max(20.0)))).float()
    o = bt.opacities.double().clamp(1e-4, 1 - 1e-4)
    rows = torch.cat((torch.log(o / (1 - o)).float()[..., None], raw_scales, bt.rotations,
                      (bt.harmonics / to.sh_mask(4, device=DEV)).reshape(1, G, 3 * K)), dim=-1)        # [1, G, 83]
    heads = [rows[:, i * h * w:(i + 1) * h * w].transpose(1, 2).reshape(1, 83, h, w).contiguous() for i in range(v)]
    points = [bt.means[:, i * h * w:(i + 1) * h * w].reshape(1, h, w, 3).contiguous() for i in range(v)]
    mapping = types.SimpleNamespace(initial=0.0, final=1.0, warm_up=10)
    cfg = adapter.GaussianAdapterCfg(0.5, 15.0, 4)
    step = 5                                                                                            # exponent 2^0.5
    dec = spf.get_decoder(spf.DecoderSplattingCUDACfg("splatting_cuda", [0.1, 0.2, 0.3], True, True, True)).to(DEV)
    dec.auto_plan = None
    wgt = torch.rand(1, 2, 3, 48, 48, device=DEV, generator=torch.Generator(DEV).manual_seed(3))

    def render(make):
        pts = [t.clone().requires_grad_(True) for t in points]
        raw = [t.clone().requires_grad_(True) for t in heads]
        out = dec(make(pts, raw), bt.extrinsics, bt.intrinsics, bt.near, bt.far, bt.image_shape)
        grads = torch.autograd.grad((out.color * wgt).sum(), pts + raw)
        return out.color.detach(), grads

    def new(pts, raw):
        return spf.GaussianTail(cfg, mapping, split_harmonics=split)(pts, raw, global_step=step)

    def old(pts, raw):
        g = torch.stack([r.flatten(2).transpose(1, 2) for r in raw], dim=1)                             # [b, v, hw, 83]
        opac = spf.map_pdf_to_opacity(g[..., 0].sigmoid(), step, mapping)
        ad = adapter.UnifiedGaussianAdapter(cfg, split_harmonics=split).to(DEV)
        a = ad(torch.stack(pts, dim=1).flatten(2, 3), opac, g[..., 1:], with_covariances=False)
        flat = lambda t: None if t is None else t.reshape(1, G, *t.shape[3:])
        return spf.Gaussians(flat(a.means), None, flat(a.rotations), flat(a.scales), flat(a.harmonics), flat(a.opacities),
                             harmonics_band4=flat(a.harmonics_band4))

    (img_new, g_new), (img_old, g_old) = render(new), render(old)
    assert float(img_old.std()) > 0.01
    err = float((img_new - img_old).abs().max())
    print(f"through the decoder ({'split' if split else 'dense'}): RGB max difference {err:.3e}")
    assert err < 1e-4
    for i, (a, b) in enumerate(zip(g_new, g_old)):
        what = f"pts[{i}]" if i < v else f"raw[{i - v}]"
        print(f"  gradient at {what}: {util.rel_linf(a, b):.3e} of scale {float(b.abs().max()):.3e}")
        assert float(b.abs().max()) > 0 and util.rel_linf(a, b) < 1e-3, what
