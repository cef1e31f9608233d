"""The DPT heads without a device: exports, state dicts, constructor signatures, refusals, the library's host-side
argument checks, the oracle against the reference's goldens and against F.interpolate, and the power condition of the
gates with float32 eager on the CPU standing in for the device (tests/dpt_cases.py states the gate;
tests/test_gpu_dpt.py applies it to the kernels)."""
import ctypes as C
import inspect

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests import dpt_cases as cases
from tests import dpt_oracle as do

NAMES = ("upsample2x", "add_relu", "postprocess", "ResidualConvUnit_custom", "FeatureFusionBlock_custom", "Interpolate",
         "DPTOutputAdapter", "PixelwiseTaskWithDPT", "PixelwiseTaskWithGSDPT", "create_dpt_head", "create_gs_dpt_head",
         "head_factory")
SYMBOLS = ("spf_dpt_max_grid", "spf_dpt_upsample2x_forward", "spf_dpt_upsample2x_backward", "spf_dpt_add_relu_forward",
           "spf_dpt_add_relu_backward", "spf_dpt_points_forward", "spf_dpt_points_backward")
INF = float("inf")
# the upsample loop shape of tests/test_gpu_dpt.py at the cap this library reports; asserted below
LOOP_CAP = 2048


def test_exports(hip_lib):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import _lib, build, heads
    for name in NAMES:
        assert name in spf.__all__ and getattr(spf, name) is getattr(heads, name), name
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name), name
    assert "dpt.hip" in build.SOURCES and hip_lib.spf_abi_version() == 7
    assert heads.max_grid() == LOOP_CAP


# ---- state dicts and signatures --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.KINDS)
def test_state_dict_keys_are_the_reference_s(kind, golden_dir):
    g = cases.golden(kind, golden_dir)
    mod = cases.build_module(kind, g)                                   # (load_state_dict is strict)
    sd = mod.state_dict()
    assert list(sd) == list(g["weights"])
    for k, v in g["weights"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k
    for i in range(4):                                                  # the duplicated entries are one tensor
        assert f"dpt.scratch.layer{i + 1}_rn.weight" in sd and f"dpt.scratch.layer_rn.{i}.weight" in sd
        assert mod.dpt.scratch.layer_rn[i] is getattr(mod.dpt.scratch, f"layer{i + 1}_rn")
    assert not any("act_1_postprocess" in k for k in sd)
    assert sorted(dict(mod.dpt.named_parameters())) == sorted(g["pgrads"])
    assert ("dpt.input_merger.0.weight" in sd) == (kind == "gs")


def test_constructor_signatures_are_the_reference_s():
    """Written out from dpt_block.py:82, :147-156, :234, :280-293, dpt_head.py:74-75 / :99, dpt_gs_head.py:84-85 / :112
    and heads/__init__.py:13."""
    import spfsplatv2_amd as spf
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(spf.ResidualConvUnit_custom.__init__)[1:] == ["features", "activation", "bn"]
    assert sig(spf.FeatureFusionBlock_custom.__init__)[1:] == ["features", "activation", "deconv", "bn", "expand",
                                                               "align_corners", "width_ratio"]
    assert sig(spf.Interpolate.__init__)[1:] == ["scale_factor", "mode", "align_corners"]
    assert sig(spf.DPTOutputAdapter.__init__)[1:] == [
        "num_channels", "stride_level", "patch_size", "main_tasks", "hooks", "layer_dims", "feature_dim", "last_dim", "use_bn",
        "dim_tokens_enc", "head_type", "output_width_ratio", "kwargs"]
    defaults = {k: p.default for k, p in inspect.signature(spf.DPTOutputAdapter.__init__).parameters.items()}
    assert (defaults["num_channels"], defaults["patch_size"], defaults["hooks"], defaults["layer_dims"], defaults["feature_dim"],
            defaults["last_dim"], defaults["head_type"]) == (1, 16, [2, 5, 8, 11], [96, 192, 384, 768], 256, 32, "regression")
    wrapper = ["n_cls_token", "hooks_idx", "dim_tokens", "output_width_ratio", "num_channels", "postprocess", "depth_mode",
               "conf_mode", "kwargs"]
    for cls in (spf.PixelwiseTaskWithDPT, spf.PixelwiseTaskWithGSDPT):
        params = inspect.signature(cls.__init__).parameters
        assert list(params)[1:] == wrapper
        assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in wrapper[:-1])
    assert sig(spf.PixelwiseTaskWithDPT.forward)[1:] == ["x", "img_info", "ray_embedding"]
    assert sig(spf.PixelwiseTaskWithGSDPT.forward)[1:] == ["x", "imgs", "img_info", "conf"]
    assert sig(spf.DPTOutputAdapter.forward_pts)[1:] == ["encoder_tokens", "image_size", "ray_embedding"]
    assert sig(spf.DPTOutputAdapter.forward_gs)[1:] == ["encoder_tokens", "imgs", "image_size", "conf"]
    for f in (spf.create_dpt_head, spf.create_gs_dpt_head):
        assert sig(f) == ["net", "has_conf", "out_nchan", "postprocess_func"]
        assert inspect.signature(f).parameters["postprocess_func"].default is spf.postprocess
    assert sig(spf.head_factory) == ["head_type", "output_mode", "net", "has_conf", "out_nchan", "pose_init_t",
                                     "use_homogeneous", "concat_enc"]
    assert sig(spf.postprocess) == ["out", "depth_mode", "conf_mode"]
    assert sig(spf.upsample2x) == ["x", "skip", "relu_skip"] and sig(spf.add_relu) == ["a", "b", "c"]


class _Net:
    dec_depth, enc_embed_dim, dec_embed_dim = 12, 1024, 768
    depth_mode, conf_mode = ("exp", -INF, INF), ("exp", 1, INF)


def test_factories_build_the_reference_s_heads():
    import spfsplatv2_amd as spf
    net = _Net()
    head = spf.head_factory("dpt", "pts3d", net, has_conf=True)
    assert type(head) is spf.PixelwiseTaskWithDPT and head.postprocess is spf.postprocess and head.return_all_layers
    assert head.dpt.hooks == [0, 6, 9, 12] and head.dpt.num_channels == 4 and head.dpt.head_type == "regression"
    assert head.dpt.head[4].weight.shape == (4, 128, 1, 1) and head.dpt.act_postprocess[0][0].weight.shape == (96, 1024, 1, 1)
    assert isinstance(head.dpt.head[1], spf.Interpolate) and not hasattr(head.dpt, "input_merger")
    raw = spf.head_factory("dpt", "gs_params", net, out_nchan=83)
    assert type(raw) is spf.PixelwiseTaskWithDPT and raw.postprocess is None and raw.dpt.num_channels == 83
    gs = spf.head_factory("dpt_gs", "gs_params", net, out_nchan=83)
    assert type(gs) is spf.PixelwiseTaskWithGSDPT and gs.postprocess is None and gs.dpt.head_type == "gs_params"
    assert gs.dpt.input_merger[0].weight.shape == (256, 3, 7, 7) and isinstance(gs.dpt.feat_up, spf.Interpolate)
    assert gs.dpt.head[0].bias is None and gs.dpt.head[4].weight.shape == (83, 256, 1, 1)
    for row in (("linear", "pts3d"), ("mlp", "pose"), ("dpt", "pose"), ("dpt_gs", "pts3d")):
        with pytest.raises(NotImplementedError, match="unexpected"):
            spf.head_factory(*row, net)


# ---- refusals, all before any launch (there is no device here) -------------------------------------------------------
def test_functions_refuse_cpu_tensors_and_sixteen_bit_types():
    import spfsplatv2_amd as spf
    x, s, out = torch.randn(1, 2, 3, 4), torch.randn(1, 2, 6, 8), torch.randn(1, 4, 3, 4)
    mode = ("exp", -INF, INF)
    calls = (lambda t: spf.upsample2x(t(x)), lambda t: spf.upsample2x(x, t(s)), lambda t: spf.upsample2x(x, t(s), True),
             lambda t: spf.add_relu(t(x)), lambda t: spf.add_relu(x, t(x)), lambda t: spf.add_relu(x, x, t(x)),
             lambda t: spf.postprocess(t(out), mode, None), lambda t: spf.postprocess(t(out), mode, ("exp", 1, INF)))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(lambda v: v)
        for dt in (torch.float16, torch.bfloat16):
            with pytest.raises(NotImplementedError, match="float32"):
                call(lambda v: v.to(dt))
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        spf.add_relu(x.double())


def test_functions_refuse_bad_arguments():
    import spfsplatv2_amd as spf
    x, s = torch.randn(1, 2, 3, 4), torch.randn(1, 2, 6, 8)
    with pytest.raises(RuntimeError, match=r"\[B, C, h, w\]"):
        spf.upsample2x(x[0])
    with pytest.raises(RuntimeError, match="skip must have shape"):
        spf.upsample2x(x, s[:, :, :5])
    with pytest.raises(ValueError, match="relu_skip is set without skip"):
        spf.upsample2x(x, None, True)
    with pytest.raises(RuntimeError, match="1 .. 2\\^31 - 1 elements"):
        spf.upsample2x(x[:0])
    with pytest.raises(ValueError, match="c is given without b"):
        spf.add_relu(x, None, x)
    with pytest.raises(RuntimeError, match="differ in shape"):
        spf.add_relu(x, x[:, :1])
    with pytest.raises(RuntimeError, match="C >= 4"):
        spf.postprocess(torch.randn(1, 3, 2, 2), ("exp", -INF, INF), ("exp", 1, INF))
    with pytest.raises(RuntimeError, match="C >= 3"):
        spf.postprocess(torch.randn(1, 2, 2, 2), ("exp", -INF, INF), None)
    with pytest.raises(ValueError, match="ordered"):
        spf.postprocess(torch.randn(1, 3, 2, 2), ("exp", 2.0, 1.0), None)


def test_postprocess_refuses_every_other_mode():
    """... in Python, before the tensor is looked at: on the CPU these raise NotImplementedError, not 'no CPU fallback'."""
    import spfsplatv2_amd as spf
    out = torch.randn(1, 4, 2, 2)
    ok = ("exp", -INF, INF)
    for depth in (("range", 0, 1), ("linear", -INF, INF), ("exp_direct", -INF, INF), ("square", -INF, INF), None, "exp"):
        with pytest.raises(NotImplementedError, match="depth_mode"):
            spf.postprocess(out, depth, None)
    for conf in (("opacity", 0, 1), ("sigmoid", 0, 1), ("exp", 1)):
        with pytest.raises(NotImplementedError, match="conf_mode"):
            spf.postprocess(out, ok, conf)
    with pytest.raises(NotImplementedError, match="depth_mode"):
        spf.PixelwiseTaskWithDPT(postprocess=spf.postprocess, depth_mode=("linear", -INF, INF), conf_mode=None,
                                 feature_dim=8, layer_dims=[4, 4, 4, 4], last_dim=4, dim_tokens=8)


def test_modules_refuse_at_construction():
    import spfsplatv2_amd as spf
    relu = nn.ReLU(False)
    small = dict(feature_dim=8, layer_dims=[4, 4, 4, 4], last_dim=4, dim_tokens_enc=8)
    with pytest.raises(NotImplementedError, match="bn=True"):
        spf.ResidualConvUnit_custom(8, relu, True)
    with pytest.raises(NotImplementedError, match="bn=True"):
        spf.FeatureFusionBlock_custom(8, relu, bn=True)
    with pytest.raises(NotImplementedError, match="use_bn=True"):
        spf.DPTOutputAdapter(use_bn=True, **small)
    with pytest.raises(NotImplementedError, match="width_ratio"):
        spf.FeatureFusionBlock_custom(8, relu, width_ratio=2)
    with pytest.raises(NotImplementedError, match="output_width_ratio"):
        spf.DPTOutputAdapter(output_width_ratio=2, **small)
    with pytest.raises(NotImplementedError, match="output_width_ratio"):
        spf.PixelwiseTaskWithDPT(output_width_ratio=1.5, feature_dim=8, layer_dims=[4, 4, 4, 4], last_dim=4, dim_tokens=8)
    with pytest.raises(NotImplementedError, match="align_corners=True"):
        spf.FeatureFusionBlock_custom(8, relu, align_corners=False)
    for args in ((2, "bilinear"), (2, "bilinear", False), (2, "nearest", True), (4, "bilinear", True), (2, "bicubic", True)):
        with pytest.raises(NotImplementedError, match="Interpolate"):
            spf.Interpolate(*args)
    assert spf.Interpolate(2, "bilinear", align_corners=True).scale_factor == 2
    with pytest.raises(NotImplementedError, match="semseg"):
        spf.DPTOutputAdapter(head_type="semseg", **small)
    with pytest.raises(ValueError, match="head_type"):
        spf.DPTOutputAdapter(head_type="other", **small)
    with pytest.raises(TypeError, match="nn.ReLU"):
        spf.ResidualConvUnit_custom(8, nn.GELU(), False)


def test_modules_have_no_cpu_path(golden_dir):
    for kind in cases.KINDS:
        g = cases.golden(kind, golden_dir)
        mod = cases.build_module(kind, g)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            cases.run_module(kind, mod, g["inputs"], g["image_size"])
        half = {k: v.half() for k, v in g["inputs"].items()}
        with pytest.raises(NotImplementedError, match="float32"):
            cases.run_module(kind, mod, half, g["image_size"])
        with pytest.raises(ValueError, match="image_size is required"):
            mod.dpt([g["inputs"][f"tok{i}"] for i in range(4)], *([g["inputs"]["img"]] if kind == "gs" else []))


# ---- the library's argument checks -----------------------------------------------------------------------------------
def test_library_argument_checks_on_the_host(hip_lib):
    """Rejected with SPF_E_INVALID (-1) and a message before anything touches a device (the pointers are never read)."""
    from spfsplatv2_amd import _lib
    err = hip_lib.spf_last_error
    p = 4096                                                            # a 16-byte aligned non-null address
    uf, ub = hip_lib.spf_dpt_upsample2x_forward, hip_lib.spf_dpt_upsample2x_backward
    assert uf(None, None, 0, 6, 5, 7, p, None) == -1 and b"null pointer" in err()
    assert uf(p, None, 0, 6, 5, 7, None, None) == -1 and b"null pointer" in err()
    assert uf(p, None, 1, 6, 5, 7, p, None) == -1 and b"relu_skip is set without skip" in err()
    for planes, h, w in ((0, 5, 7), (-1, 5, 7), (6, 0, 7), (6, 5, -3)):
        assert uf(p, None, 0, planes, h, w, p, None) == -1 and b"must be positive" in err()
        assert ub(p, None, planes, h, w, p, None, None) == -1 and b"must be positive" in err()
    for planes, h, w in ((1, 16385, 1), (1, 1, 16385), (1 << 31, 1, 1), (1 << 20, 32, 32), (3, 16384, 16384)):
        assert uf(p, None, 0, planes, h, w, p, None) == -1 and b"below 2^31 elements" in err()
    assert uf(p + 4, None, 0, 6, 5, 7, p, None) == -1 and b"16-byte aligned" in err()
    assert uf(p, p + 8, 0, 6, 5, 7, p, None) == -1 and b"16-byte aligned" in err()
    assert ub(None, None, 6, 5, 7, p, None, None) == -1 and b"null pointer" in err()
    assert ub(p, p, 6, 5, 7, p, None, None) == -1 and b"dskip is dy" in err()
    assert ub(p, None, 6, 5, 7, p, p, None) == -1 and b"dskip is dy" in err()
    assert ub(p, None, 6, 5, 7, p + 4, None, None) == -1 and b"16-byte aligned" in err()
    af, ab = hip_lib.spf_dpt_add_relu_forward, hip_lib.spf_dpt_add_relu_backward
    assert af(None, None, None, 5, None, p, None) == -1 and b"null pointer" in err()
    assert af(p, None, p, 5, p, p, None) == -1 and b"c is given without b" in err()
    assert af(p, p, None, 5, None, p, None) == -1 and b"s is written with a second addend" in err()
    assert af(p, None, None, 5, p, p, None) == -1 and b"s is written with a second addend" in err()
    for n in (0, -1, 1 << 31):
        assert af(p, None, None, n, None, p, None) == -1 and b"n must be 1 .. 2^31 - 1" in err()
        assert ab(p, p, None, n, p, None) == -1 and b"n must be 1 .. 2^31 - 1" in err()
    assert af(p, p + 4, None, 5, p, p, None) == -1 and b"16-byte aligned" in err()
    assert ab(p, None, None, 5, p, None) == -1 and b"null pointer" in err()
    assert ab(p, p, p + 12, 5, p, None) == -1 and b"16-byte aligned" in err()

    def pts(**kw):
        a = _lib.SpfDptPoints()
        a.in_, a.B, a.HW, a.C, a.has_conf, a.depth_min, a.depth_max, a.conf_min, a.conf_max = p, 2, 35, 4, 1, -INF, INF, 1.0, INF
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)
    pf, pb = hip_lib.spf_dpt_points_forward, hip_lib.spf_dpt_points_backward
    assert pf(None, p, p, None) == -1 and b"args is null" in err()
    assert pf(pts(in_=None), p, p, None) == -1 and b"null pointer" in err()
    assert pf(pts(), None, p, None) == -1 and b"null output" in err()
    assert pf(pts(), p, None, None) == -1 and b"with has_conf and only then" in err()
    assert pf(pts(has_conf=0), p, p, None) == -1 and b"with has_conf and only then" in err()
    for kw in (dict(B=0), dict(HW=-1), dict(C=3), dict(C=2, has_conf=0)):
        assert pf(pts(**kw), p, p, None) == -1 and b"must be positive" in err()
    assert pf(pts(B=1 << 20, HW=1 << 10), p, p, None) == -1 and b"below 2^31 elements" in err()
    assert pf(pts(depth_min=2.0, depth_max=1.0), p, p, None) == -1 and b"depth bounds" in err()
    assert pf(pts(conf_min=2.0, conf_max=1.0), p, p, None) == -1 and b"conf bounds" in err()
    assert pf(pts(in_=p + 4), p, p, None) == -1 and b"16-byte aligned" in err()
    assert pb(pts(), None, p, p, None) == -1 and b"null pointer" in err()
    assert pb(pts(), p, None, p, None) == -1 and b"with has_conf and only then" in err()
    assert pb(pts(), p, p, p + 8, None) == -1 and b"16-byte aligned" in err()


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", cases.UP_SHAPES + ((1, 1, 2, 2), (1, 1, 3, 2), (1, 1, 64, 33)))
def test_oracle_up2_is_f_interpolate(shape):
    """The written-out index formula is torch's, in float64 -- and its mutant is torch's other rule."""
    x = torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    want = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
    assert (do.up2(x) - want).abs().max() < 1e-14
    other = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    assert (do.up2(x, frozenset(["no_align_corners"])) - other).abs().max() < 1e-14


def test_oracle_postprocess_is_the_reference_s_on_the_forced_pixels(golden_dir):
    """d = 0, d = 1e-9 and d = 60: outputs and the gradient autograd gave the reference's expression."""
    g = cases.golden("pts", golden_dir)
    post = g["post"]
    raw = post["in"]
    d = raw[:, :3].norm(dim=1)
    forced = sorted(float(d[b, y, x]) for b, y, x in post["forced"])
    assert forced[:2] == [0.0, 0.0] and all(abs(v - 1e-9) < 1e-15 for v in forced[2:4]) and forced[4:] == [60.0, 60.0]
    x64 = do.points_with_grads(raw, g["depth_mode"], g["conf_mode"], post["ups"]["pts3d"], post["ups"]["conf"])
    assert torch.isfinite(post["din"]).all()
    assert do.rel_err(post["out"]["pts3d"], x64["pts3d"]) < 1e-6 and do.rel_err(post["out"]["conf"], x64["conf"]) < 1e-6
    assert do.rel_err(post["din"], x64["din"]) < 1e-6
    for b, y, x in post["forced"]:                                      # pixel by pixel: each at its own scale
        got, want = post["din"][b, :3, y, x].double(), x64["din"][b, :3, y, x]
        assert (got - want).abs().max() <= 1e-6 * want.abs().max(), (b, y, x)
        if float(d[b, y, x]) == 0.0:
            assert not got.any() and not post["out"]["pts3d"][b, y, x].any()


@pytest.mark.parametrize("kind", cases.KINDS)
def test_oracle_reproduces_the_reference_goldens(kind, golden_dir):
    """float64 oracle against the float32 outputs of the reference's own classes: within the float32 run's rounding."""
    g, x64, _ = cases.module_reference(kind, golden_dir)
    assert g["args"] == dict(feature_dim=16, layer_dims=[8, 8, 16, 16], last_dim=8, dim_tokens=[32, 24, 24, 24],
                             hooks_idx=[0, 1, 2, 3]) and g["image_size"] == (32, 48) and g["inputs"]["tok0"].shape == (2, 6, 32)
    for k, v in g["out"].items():
        assert do.rel_err(v, x64[k]) < 2e-6, k
    for k, v in g["grads"].items():
        assert do.rel_err(v, x64["d_" + k]) < 5e-6, k
    for k, v in g["pgrads"].items():
        if k.startswith(cases.IDLE):
            assert not v.any(), k
        else:
            assert do.rel_err(v, x64["dparam_" + k]) < 5e-6, k


# ---- the power condition ---------------------------------------------------------------------------------------------
def _power(label, dists, e_eager, want_mutants):
    assert set(dists) == set(want_mutants), label
    bad = cases.power_failures(label, dists, e_eager)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("variant", list(cases.UP_VARIANTS))
@pytest.mark.parametrize("shape", cases.UP_SHAPES + (cases.loop_shape(LOOP_CAP),))
def test_power_condition_of_the_upsample_gate(shape, variant):
    d, x64, dists = cases.up_reference(shape, variant)
    e_eager = cases.errors(cases.up_oracle(d, variant, torch.float32), x64)
    _power(f"up2 {shape} {variant}", dists, e_eager, cases.up_mutants(shape, variant))
    assert set(x64) == ({"out", "dx"} if variant == "plain" else {"out", "dx", "dskip"})
    if variant != "plain":
        assert (d["skip"] == 0).any() and (d["skip"] < 0).any()


@pytest.mark.parametrize("variant", list(cases.ADD_VARIANTS))
@pytest.mark.parametrize("n", cases.ADD_SIZES + (cases.add_loop_size(LOOP_CAP),))
def test_power_condition_of_the_add_relu_gate(n, variant):
    d, x64, dists = cases.add_reference(n, variant)
    e_eager = cases.errors(cases.add_oracle(d, torch.float32), x64)
    _power(f"add_relu n={n} {variant}", dists, e_eager, cases.add_mutants(variant))
    if n > 1:
        s = x64["s"] if "s" in x64 else d["a"]
        assert (s == 0).any()


@pytest.mark.parametrize("variant", list(cases.POINT_VARIANTS))
@pytest.mark.parametrize("hw", cases.POINT_SIZES)
def test_power_condition_of_the_points_gate(hw, variant):
    d, x64, dists = cases.point_reference(hw, variant)
    e_eager = cases.errors(cases.point_oracle(d, variant, torch.float32), x64)
    _power(f"points {hw} {variant}", dists, e_eager, cases.point_mutants(variant))
    norm = d["out"][:, :3].norm(dim=1)
    assert float(norm.min()) == 0.0 and ((norm > 0) & (norm < 1e-8)).any()
    if cases.POINT_VARIANTS[variant][1] and hw != (1, 1):
        assert float(norm.max()) == 60.0


@pytest.mark.parametrize("kind", cases.KINDS)
def test_power_condition_of_the_module_gate(kind, golden_dir):
    g, x64, dists = cases.module_reference(kind, golden_dir)
    e_eager = cases.errors(cases.flat(do.module_case(g, torch.float32)), x64)
    _power(f"module {kind}", dists, e_eager, cases.MODULE_MUTANTS[kind])
    # and with the convolutions exact and float32 only where the product calls its kernels
    e_mixed = cases.errors(cases.flat(do.module_case(g, mixed=True)), x64)
    _power(f"module {kind} exact convolutions", dists, e_mixed, cases.MODULE_MUTANTS[kind])
    assert 0 < max(e_mixed.values()) < 2e-6


def test_the_gate_rejects_a_mutant_and_accepts_the_eager_run():
    d, x64, dists = cases.up_reference((2, 3, 5, 7), "relu_skip")
    eager = cases.up_oracle(d, "relu_skip", torch.float32)
    cases.gate("control", eager, eager, x64, dists)
    for m in cases.up_mutants((2, 3, 5, 7), "relu_skip"):
        with pytest.raises(AssertionError):
            cases.gate("control " + m, cases.up_oracle(d, "relu_skip", torch.float32, mut=frozenset([m])), eager, x64, {})
