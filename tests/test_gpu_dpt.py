"""The DPT heads' kernels and modules on the device (csrc/dpt.hip, spfsplatv2_amd/heads.py).

Gate (tests/dpt_cases.py, the rule of tests/block_cases.py): per tensor err = max|x - x64| / max|x64| against the float64
oracle must not exceed twice the err of float32 eager torch on the device plus one float32 ulp; before a gate is trusted
the power condition of tests/test_dpt.py is asserted again with the device's eager figures.  Every figure is printed.
"""
import pytest
import torch

from tests import dpt_cases as cases
from tests import dpt_oracle as do

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _dev(d, requires_grad=()):
    out = {}
    for k, v in d.items():
        out[k] = None if v is None else v.to(DEV)
        if out[k] is not None and k in requires_grad:
            out[k].requires_grad_(True)
    return out


# ---- the product -----------------------------------------------------------------------------------------------------
def run_up(d, variant):
    import spfsplatv2_amd as spf
    t = _dev(d, ("x", "skip"))
    out = spf.upsample2x(t["x"], t["skip"], cases.UP_VARIANTS[variant][1])
    leaves = {"dx": t["x"]} if t["skip"] is None else {"dx": t["x"], "dskip": t["skip"]}
    return {"out": out.detach(), **dict(zip(leaves, torch.autograd.grad(out, list(leaves.values()), t["dy"])))}, t


def run_add(d):
    import spfsplatv2_amd as spf
    t = _dev(d, ("a", "b", "c"))
    s, y = spf.add_relu(t["a"], t["b"], t["c"])
    leaves = {k: v for k, v in (("da", t["a"]), ("db", t["b"]), ("dc", t["c"])) if v is not None}
    if t["b"] is None:
        assert s is t["a"]
        outs, ups = [y], [t["dy"]]
    else:
        outs, ups = ([y, s], [t["dy"], t["ds"]]) if t["ds"] is not None else ([y], [t["dy"]])
    res = {"y": y.detach(), **dict(zip(leaves, torch.autograd.grad(outs, list(leaves.values()), ups)))}
    if t["b"] is not None:
        res["s"] = s.detach()
    return res


def run_points(d, variant):
    import spfsplatv2_amd as spf
    t = _dev(d, ("out",))
    depth, conf = cases.point_modes(variant)
    res = spf.postprocess(t["out"], depth, conf)
    assert sorted(res) == (["conf", "pts3d"] if conf else ["pts3d"])
    outs, ups = [res["pts3d"]], [t["dpts"]]
    if conf:
        outs.append(res["conf"])
        ups.append(t["dconf"])
    (din,) = torch.autograd.grad(outs, [t["out"]], ups)
    return {**{k: v.detach() for k, v in res.items()}, "din": din}


def _shapes_match(got, x64):
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.shape == x64[k].shape and v.is_contiguous(), k


def check_up(shape, variant):
    d, x64, dists = cases.up_reference(shape, variant)
    got, _ = run_up(d, variant)
    _shapes_match(got, x64)
    cases.gate(f"up2 {shape} {variant}", got, cases.up_oracle(d, variant, torch.float32, DEV), x64, dists)


def check_add(n, variant):
    d, x64, dists = cases.add_reference(n, variant)
    got = run_add(d)
    _shapes_match(got, x64)
    cases.gate(f"add_relu n={n} {variant}", got, cases.add_oracle(d, torch.float32, DEV), x64, dists)


# ---- a. upsample2x ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(cases.UP_VARIANTS))
@pytest.mark.parametrize("shape", cases.UP_SHAPES)
def test_upsample_against_oracle(shape, variant):
    """Forward and backward: single pixels and single rows and columns (scale 0 along that axis), odd sizes (the scalar
    path: the output width is no multiple of 4), 16 x 16 (the vector path) and a row longer than a block."""
    check_up(shape, variant)


@pytest.mark.parametrize("variant", list(cases.UP_VARIANTS))
def test_upsample_plane_loop_of_a_capped_grid(variant):
    """Three more planes than the grid has blocks: the first three blocks take a second plane."""
    from spfsplatv2_amd import heads
    shape = cases.loop_shape(heads.max_grid())
    assert shape[0] * shape[1] == heads.max_grid() + 3 and shape[2:] == (2, 2)
    check_up(shape, variant)


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 4, 16, 16), (1, 2, 3, 258), (1, 2, 1, 5), (1, 1, 2, 2)])
def test_upsample_backward_is_the_transpose_of_the_forward(shape):
    """<up2(x), g> == <x, up2^T(g)> to float32 rounding, both sums taken in float64 from the float32 results.  Bound: an
    output carries at most 6 roundings of its four-tap sum, each of the size of up2(|x|); an input gradient at most 18
    (the weights, seven fused steps along a row, seven across rows), each of the size of up2^T(|g|); summed against g
    and x both are multiples of the one number T = <up2(|x|), |g|> = <|x|, up2^T(|g|)>: 24 ulp of T."""
    import spfsplatv2_amd as spf
    d = cases.up_inputs(shape, "plain")
    x, g = d["x"].to(DEV).requires_grad_(True), d["dy"].to(DEV)
    out = spf.upsample2x(x)
    (dx,) = torch.autograd.grad(out, x, g)
    lhs, rhs = (out.detach().double() * g.double()).sum(), (x.detach().double() * dx.double()).sum()
    scale = float((do.up2(d["x"].double().abs()) * d["dy"].double().abs()).sum())
    print(f"transpose {shape}: <up2 x, g> {float(lhs):.9e} <x, up2^T g> {float(rhs):.9e} T {scale:.3e}")
    assert abs(float(lhs - rhs)) <= 24 * cases.ULP * scale


def test_upsample_is_bitwise_reproducible_and_dskip_is_dy():
    import spfsplatv2_amd as spf
    for shape in ((2, 3, 5, 7), (1, 4, 16, 16)):
        for variant in cases.UP_VARIANTS:
            d = cases.up_inputs(shape, variant)
            (a, _), (b, _) = run_up(d, variant), run_up(d, variant)
            for k in a:
                assert torch.equal(a[k], b[k]), (shape, variant, k)
    d = cases.up_inputs((2, 3, 5, 7), "skip")
    got, t = run_up(d, "skip")
    assert got["dskip"].data_ptr() == t["dy"].data_ptr()                # the same tensor, no copy
    got, t = run_up(cases.up_inputs((2, 3, 5, 7), "relu_skip"), "relu_skip")
    assert got["dskip"].data_ptr() != t["dy"].data_ptr()
    assert torch.equal(got["dskip"], t["dy"] * (t["skip"] > 0))
    # only skip wants a gradient and there is no ReLU: nothing is launched, dskip is still dy
    x, skip, dy = t["x"].detach(), t["skip"].detach().requires_grad_(True), t["dy"]
    (ds,) = torch.autograd.grad(spf.upsample2x(x, skip), skip, dy)
    assert ds.data_ptr() == dy.data_ptr()


def test_upsample_copies_a_cropped_view():
    """The cropped ``path_4[:, :, :h, :w]`` of dpt_head.py:59, and a misaligned contiguous view."""
    import spfsplatv2_amd as spf
    d, x64, dists = cases.up_reference((2, 3, 5, 7), "skip")
    big = torch.randn(2, 3, 6, 8)
    big[:, :, :5, :7] = d["x"]
    x = big.to(DEV)[:, :, :5, :7].requires_grad_(True)
    pad = torch.zeros(d["skip"].numel() + 1, device=DEV)
    pad[1:] = d["skip"].to(DEV).reshape(-1)
    skip = pad[1:].view(d["skip"].shape).requires_grad_(True)
    assert not x.is_contiguous() and skip.is_contiguous() and skip.data_ptr() % 16 != 0
    out = spf.upsample2x(x, skip)
    dx, dskip = torch.autograd.grad(out, [x, skip], d["dy"].to(DEV))
    cases.gate("up2 cropped (2, 3, 5, 7) skip", {"out": out.detach(), "dx": dx, "dskip": dskip},
               cases.up_oracle(d, "skip", torch.float32, DEV), x64, dists)


def test_non_finite_values_spread_no_further_than_in_torch():
    """One inf in the upstream gradient reaches at most the four input pixels its output reads, and none that torch's
    scatter backward leaves finite: a window neighbour with weight zero is selected away, not multiplied.  A NaN sum passes its gradient, as
    torch's threshold backward does; with ``relu_skip`` only skip wanting a gradient, the gather is not run at all."""
    import torch.nn.functional as F

    import spfsplatv2_amd as spf
    for shape, at in (((1, 2, 5, 7), (0, 1, 4, 9)), ((1, 1, 16, 16), (0, 0, 31, 0)), ((1, 1, 3, 258), (0, 0, 2, 515))):
        d = cases.up_inputs(shape, "plain")
        dy = d["dy"].clone()
        dy[at] = float("inf")
        x = d["x"].to(DEV).requires_grad_(True)
        (got,) = torch.autograd.grad(spf.upsample2x(x), x, dy.to(DEV))
        (want,) = torch.autograd.grad(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True), x, dy.to(DEV))
        # (torch also turns a tap of weight exactly 0 into NaN, 0 * inf; here such a tap stays finite)
        assert (torch.isfinite(got) | ~torch.isfinite(want)).all() and 1 <= int((~torch.isfinite(got)).sum()) <= 4, shape
        # and the pixels torch leaves finite pass the gate's rule against the float64 oracle
        x64 = do.upsample_with_grads(d["x"], None, False, dy)["dx"]
        ok = (torch.isfinite(want).cpu() & torch.isfinite(x64))
        e_got, e_eager = do.rel_err(got.cpu()[ok], x64[ok]), do.rel_err(want.cpu()[ok], x64[ok])
        print(f"one inf upstream {shape}: product {e_got:.3e} eager {e_eager:.3e}")
        assert e_got <= 2 * e_eager + cases.ULP, shape
    a = torch.tensor([1.0, float("nan"), -1.0, 2.0, float("nan")], device=DEV, requires_grad=True)
    b = torch.tensor([1.0, 1.0, 0.5, float("nan"), 0.0], device=DEV, requires_grad=True)
    g = torch.arange(1.0, 6.0, device=DEV)
    for args in ((a,), (a, b)):
        s, y = spf.add_relu(*args)
        want = torch.relu(sum(args))
        assert torch.equal(torch.isnan(y), torch.isnan(want)) and torch.equal(y.nan_to_num(7.0), want.nan_to_num(7.0))
        got = torch.autograd.grad(y, args, g)
        ref = torch.autograd.grad(want, args, g)
        for u, v in zip(got, ref):
            assert torch.equal(u, v)
    t = _dev(cases.up_inputs((2, 3, 5, 7), "relu_skip"), ("skip",))
    (dskip,) = torch.autograd.grad(spf.upsample2x(t["x"], t["skip"], True), t["skip"], t["dy"])
    assert torch.equal(dskip, t["dy"] * (t["skip"] > 0))


# ---- b. add_relu -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(cases.ADD_VARIANTS))
@pytest.mark.parametrize("n", cases.ADD_SIZES)
def test_add_relu_against_oracle(n, variant):
    """One, two and three addends, ds present and absent, zeros in s; a single float, a tail only, vectors and a tail."""
    check_add(n, variant)


@pytest.mark.parametrize("variant", ["a", "abc_ds"])
def test_add_relu_loop_of_a_capped_grid(variant):
    from spfsplatv2_amd import heads
    check_add(cases.add_loop_size(heads.max_grid()), variant)


def test_add_relu_shapes_views_and_reproducibility():
    import spfsplatv2_amd as spf
    d = cases.add_inputs(4 * 64 * 4 + 3, "abc_ds")
    a, b = run_add(d), run_add(d)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["da"].data_ptr() != 0 and torch.equal(a["da"], a["db"]) and torch.equal(a["da"], a["dc"])
    x = torch.randn(2, 3, 6, 8, device=DEV)
    s, y = spf.add_relu(x[:, :, :5, :7], x[:, :, 1:, 1:])
    assert s.shape == (2, 3, 5, 7) and torch.equal(s, x[:, :, :5, :7] + x[:, :, 1:, 1:]) and torch.equal(y, torch.relu(s))


# ---- c. postprocess --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(cases.POINT_VARIANTS))
@pytest.mark.parametrize("hw", cases.POINT_SIZES)
def test_postprocess_against_oracle(hw, variant):
    """With and without conf and finite bounds; pixels at d = 0, d = 1e-9 and, with bounds, d = 60; 35 pixels take the
    scalar path, 1536 the vector path."""
    d, x64, dists = cases.point_reference(hw, variant)
    got = run_points(d, variant)
    _shapes_match(got, x64)
    cases.gate(f"points {hw} {variant}", got, cases.point_oracle(d, variant, torch.float32, DEV), x64, dists)
    a = run_points(d, variant)
    for k in a:
        assert torch.equal(a[k], got[k]), k


def test_postprocess_on_the_reference_s_forced_pixels(golden_dir):
    """The golden's d = 0, d = 1e-9 and d = 60 pixels: what autograd gave the reference, pixel by pixel."""
    import spfsplatv2_amd as spf
    g = cases.golden("pts", golden_dir)
    post = g["post"]
    raw = post["in"].to(DEV).requires_grad_(True)
    res = spf.postprocess(raw, g["depth_mode"], g["conf_mode"])
    (din,) = torch.autograd.grad([res["pts3d"], res["conf"]], [raw], [post["ups"]["pts3d"].to(DEV), post["ups"]["conf"].to(DEV)])
    x64 = do.points_with_grads(post["in"], g["depth_mode"], g["conf_mode"], post["ups"]["pts3d"], post["ups"]["conf"])
    eager = do.points_with_grads(post["in"], g["depth_mode"], g["conf_mode"], post["ups"]["pts3d"], post["ups"]["conf"],
                                 torch.float32, DEV)
    cases.gate("points forced", {"pts3d": res["pts3d"].detach(), "conf": res["conf"].detach(), "din": din}, eager, x64, {})
    assert torch.isfinite(din).all()
    for b, y, x in post["forced"]:
        got, want, ref = din[b, :3, y, x].double().cpu(), x64["din"][b, :3, y, x], post["din"][b, :3, y, x].double()
        bound = 2 * float((ref - want).abs().max()) + cases.ULP * float(want.abs().max())
        print(f"forced pixel {(b, y, x)}: product {float((got - want).abs().max()):.3e} reference {float((ref - want).abs().max()):.3e}")
        assert float((got - want).abs().max()) <= bound, (b, y, x)
        pts, pw = res["pts3d"][b, y, x].detach().double().cpu(), x64["pts3d"][b, y, x]
        pr = post["out"]["pts3d"][b, y, x].double()
        assert float((pts - pw).abs().max()) <= 2 * float((pr - pw).abs().max()) + cases.ULP * float(pw.abs().max()), (b, y, x)


def test_postprocess_leaves_further_channels_without_gradient():
    import spfsplatv2_amd as spf
    out = torch.randn(2, 6, 5, 7, device=DEV, requires_grad=True)
    res = spf.postprocess(out, ("exp", -cases.INF, cases.INF), None)
    (din,) = torch.autograd.grad(res["pts3d"].sum(), out)
    assert not din[:, 3:].any() and din[:, :3].any()


# ---- d. modules ------------------------------------------------------------------------------------------------------
def _prepare(kind, g):
    mod = cases.build_module(kind, g).to(DEV)
    ins = {k: v.to(DEV).requires_grad_(True) for k, v in g["inputs"].items()}
    return mod, ins


def _step(kind, g, mod, ins):
    """Forward and the backward of 0.5 * sum(out^2) to the inputs and every parameter."""
    outs = cases.run_module(kind, mod, ins, g["image_size"])
    params = dict(mod.dpt.named_parameters())
    wrt = {**ins, **params}
    loss = sum(0.5 * (o * o).sum() for o in outs.values())
    grads = dict(zip(wrt, torch.autograd.grad(loss, list(wrt.values()), allow_unused=True)))
    for k in params:
        assert (grads[k] is None) == k.startswith(cases.IDLE), k
    return ({k: v.detach() for k, v in outs.items()}, {k: grads[k] for k in ins},
            {k: grads[k] for k in params if grads[k] is not None})


@pytest.mark.parametrize("kind", cases.KINDS)
def test_modules_against_golden_and_oracle(kind, golden_dir):
    """Each head with its golden's state dict, float32 throughout: the outputs through the gate, and the outputs, the
    gradient to every token tensor and to the image and every parameter gradient against the reference's own floats."""
    g, x64, dists = cases.module_reference(kind, golden_dir)
    got = cases.flat(_step(kind, g, *_prepare(kind, g)))
    eager = cases.flat(do.module_case(g, torch.float32, DEV))
    assert sorted(k for k in got if k.startswith("dparam_")) == sorted("dparam_" + k for k in g["pgrads"]
                                                                       if not k.startswith(cases.IDLE))
    outs = list(g["out"])
    pick = lambda d: {k: d[k] for k in outs}
    cases.gate(f"module {kind} forward", pick(got), pick(eager), pick(x64),
               {m: {k: v for k, v in d.items() if k in outs} for m, d in dists.items()})
    for k, v in g["out"].items():
        assert do.rel_err(got[k], v.double()) < cases.GOLDEN_OUT_TOL, k
    for k, v in g["grads"].items():
        assert do.rel_err(got["d_" + k], v.double()) < cases.GOLDEN_GRAD_TOL, k
    for k, v in g["pgrads"].items():
        if not k.startswith(cases.IDLE):
            assert do.rel_err(got["dparam_" + k], v.double()) < cases.GOLDEN_GRAD_TOL, k


@pytest.mark.parametrize("kind", cases.KINDS)
def test_modules_backward_through_exact_convolutions(kind, golden_dir):
    """The gate over every output, input gradient and parameter gradient with the convolutions in float64 on both sides
    and the kernels -- on the eager side the torch operations they replace -- in float32 (tests/dpt_cases.py says why)."""
    g, x64, dists = cases.module_reference(kind, golden_dir)
    mod = cases.build_module(kind, g).double().to(DEV)
    ins = {k: v.double().to(DEV).requires_grad_(True) for k, v in g["inputs"].items()}
    with cases.float32_kernel_sites(mod):
        got = cases.flat(_step(kind, g, mod, ins))
    for v in got.values():
        assert v.dtype == torch.float64
    eager = cases.flat(do.module_case(g, torch.float64, DEV, mixed=True))
    cases.gate(f"module {kind} exact convolutions", got, eager, x64, dists)


@pytest.mark.parametrize("kind", cases.KINDS)
def test_a_head_step_copies_nothing_but_the_crop(kind, golden_dir):
    """The convolutions answer in dense NCHW, so the fused calls take their operands and upstream gradients in place: the
    only copy of a step is the cropped ``path_4`` (2 x 16 x 2 x 3 floats) going into refinenet3's add."""
    from spfsplatv2_amd import heads
    g = cases.golden(kind, golden_dir)
    mod, ins = _prepare(kind, g)
    before = dict(heads.dense_copies)
    _step(kind, g, mod, ins)
    assert heads.dense_copies["calls"] - before["calls"] == 1
    assert heads.dense_copies["bytes"] - before["bytes"] == 2 * 16 * 2 * 3 * 4


@pytest.mark.parametrize("kind", cases.KINDS)
def test_forward_backward_never_sync_and_repeat_bitwise(kind, golden_dir):
    g = cases.golden(kind, golden_dir)
    prepared = _prepare(kind, g)
    want = _step(kind, g, *prepared)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _step(kind, g, *prepared)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # the convolutions' own backward may use atomics: only what the kernels of this package produce alone is compared
    for k in want[0]:
        assert torch.equal(want[0][k], got[0][k]), k


# ---- e. the library's argument checks --------------------------------------------------------------------------------
def test_library_argument_checks_launch_nothing(hip_lib):
    """SPF_E_INVALID with a message, on real device buffers that must come back untouched."""
    import ctypes as C
    x = torch.randn(6, 5, 7, device=DEV)
    out = torch.full((6, 10, 14), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    err = hip_lib.spf_last_error
    uf = hip_lib.spf_dpt_upsample2x_forward
    assert uf(p(x), None, 1, 6, 5, 7, p(out), None) == -1 and b"relu_skip is set without skip" in err()
    assert uf(p(x), None, 0, 0, 5, 7, p(out), None) == -1 and b"must be positive" in err()
    assert uf(p(x), None, 0, 6, 5, 7, C.c_void_p(out.data_ptr() + 4), None) == -1 and b"16-byte aligned" in err()
    assert hip_lib.spf_dpt_add_relu_forward(p(x), None, None, 210, p(out), p(out), None) == -1 and b"second addend" in err()
    assert hip_lib.spf_dpt_add_relu_backward(p(x), p(x), None, 0, p(out), None) == -1 and b"n must be" in err()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert uf(p(x), None, 0, 6, 5, 7, p(out), None) == 0                 # and the same call, well formed, does launch
    torch.cuda.synchronize()
    want = torch.nn.functional.interpolate(x[None].double().cpu(), scale_factor=2, mode="bilinear", align_corners=True)[0]
    assert do.rel_err(out, want) < 1e-6
