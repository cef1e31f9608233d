"""The pose heads without a device: the oracle against the reference's goldens, the power condition of every gate with
CPU float32 figures, the ABI surface, the state-dict keys and the checks that raise before any launch."""
import re
from types import SimpleNamespace

import pytest
import torch

from tests import posehead_cases as cases
from tests import posehead_oracle as po
from tests.conftest import ROOT

SYMBOLS = [f"spf_posehead_{k}_{d}" for k in ("pool", "encode", "embed_silu", "modulate", "attn", "activate")
           for d in ("forward", "backward")]


def _power(label, ref, oracle):
    d, x64, dists = ref
    e_eager = cases.errors(oracle(d, torch.float32), x64)
    bad = cases.power_failures(label, dists, e_eager)
    assert not bad, "\n".join(bad)


# ---- the surface -----------------------------------------------------------------------------------------------------
def test_exports():
    import spfsplatv2_amd as spf
    for name in ("PoseHeadCfg", "PoseHead", "create_pose_head", "camera_head_factory", "predict_poses", "activate_pose",
                 "modulate", "CameraTrunkAttention", "CameraTrunkBlock", "CameraHead"):
        assert name in spf.__all__ and hasattr(spf, name), name


def test_symbols_are_in_the_header_and_the_binding_and_the_abi_stays_7(hip_lib):
    from spfsplatv2_amd import _lib
    header = (ROOT / "include" / "spfsplat_hip.h").read_text()
    for name in SYMBOLS:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.SYMBOLS and _lib.SYMBOLS[name][1][-1] is __import__("ctypes").c_void_p, name
        assert hasattr(hip_lib, name), name
    assert _lib.ABI_VERSION == 7 and hip_lib.spf_abi_version() == 7
    assert re.search(r"#define SPF_ABI_VERSION 7\b", header)


@pytest.mark.parametrize("name", cases.MODULES)
def test_state_dict_keys_are_the_reference_s(name, golden_dir):
    g = cases.golden(name, golden_dir)
    mod = cases.build_module(name, g)
    assert list(mod.state_dict()) == g["keys"]
    assert [k for k, _ in mod.named_parameters()] == g["param_names"]
    for k, v in mod.state_dict().items():
        assert v.shape == g["weights"][k].shape, k


def test_init_pose_and_the_buffers_are_the_reference_s():
    import spfsplatv2_amd as spf
    net = SimpleNamespace(enc_embed_dim=24, dec_embed_dim=16)
    head = spf.create_pose_head(net, spf.PoseHeadCfg(pose_init_t=True, use_homogeneous=True, concat_enc=True))
    assert head.d_model == 40 and head.fc_t.out_features == 4
    assert torch.equal(head.fc_rot.bias, torch.tensor([1., 0, 0, 0, 1, 0])) and not head.fc_rot.weight.any()
    assert not head.fc_t.weight.any() and not head.fc_t.bias.any()
    assert head._homog == pytest.approx(po.HOMOG, rel=1e-6) and all(type(x) is float for x in head._homog)
    assert [k for k, _ in head.named_buffers()] == ["max_scale", "min_scale", "max_inv_scale", "h_beta", "min_inv_scale"]
    head = spf.PoseHead(net, spf.PoseHeadCfg(pose_init_t=False, use_homogeneous=False, concat_enc=False))
    assert head.d_model == 16 and head.fc_t.out_features == 3 and head.fc_t.weight.any() and head._homog is None
    with pytest.raises(NotImplementedError):
        spf.camera_head_factory("dpt", "pose", net, head.cfg)


# ---- the oracle against the reference --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.MODULES)
def test_oracle_reproduces_the_reference_goldens(name, golden_dir):
    """The reference's float32 outputs and input gradients lie within float32 eager spread of the float64 oracle, and the
    float32 oracle within the same spread of the golden."""
    g, x64, _ = cases.module_reference(name, golden_dir)
    f32 = cases.flat(po.module_case(g, torch.float32))
    for i, o in enumerate(g["outs"]):
        assert cases.rel_err(o, x64[f"out{i}"]) < 2e-6, i
        assert cases.rel_err(f32[f"out{i}"], o.double()) < 2e-6, i
    for k, v in g["grads"].items():
        assert cases.rel_err(v, x64["d_" + k]) < 5e-6, k
    if name == "mlp1":
        assert torch.equal(g["outs"][0][:, :6], torch.tensor([1., 0, 0, 0, 1, 0]).expand(3, 6))
        assert torch.equal(x64["out0"][:, :6].float(), g["outs"][0][:, :6])


def test_oracle_kernels_are_torch_s():
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(5, 9, dtype=torch.float64, generator=gen) * 30
    F = torch.nn.functional
    assert torch.allclose(po.softplus(x, po.HOMOG[0]), F.softplus(x, beta=po.HOMOG[0]), rtol=1e-12, atol=0)
    qkv = torch.randn(2, 5, 3 * 2 * 64, dtype=torch.float64, generator=gen)
    q, k, v = qkv.reshape(2, 5, 3, 2, 64).permute(2, 0, 3, 1, 4)
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(2, 5, 128)
    assert torch.allclose(po.attention(qkv, 2), want, rtol=1e-10, atol=1e-12)
    w, b = torch.randn(8, 9, dtype=torch.float64, generator=gen), torch.randn(8, dtype=torch.float64, generator=gen)
    assert torch.allclose(po.embed_silu(x / 30, w, b), F.silu(F.linear(x / 30, w, b)), rtol=1e-12, atol=1e-14)
    xx, mod = torch.randn(5, 8, dtype=torch.float64, generator=gen), torch.randn(5, 24, dtype=torch.float64, generator=gen)
    sh, sc, ga = mod.chunk(3, dim=-1)
    want = ga * (F.layer_norm(xx, (8,), eps=1e-6) * (1 + sc) + sh) + xx
    assert torch.allclose(po.modulate(xx, mod), want, rtol=1e-10, atol=1e-12)


# ---- the power condition, CPU float32 figures ------------------------------------------------------------------------
@pytest.mark.parametrize("widths", cases.POOL_WIDTHS)
def test_power_condition_of_the_pool_gate(widths):
    for rows in cases.POOL_ROWS:
        for L in cases.POOL_L:
            _power(f"pool rows={rows} L={L} {widths}", cases.pool_reference(rows, L, widths), cases.pool_oracle)


def test_power_condition_of_the_encode_gate():
    from functools import partial
    for b in cases.ROWS:
        d = cases.encode_inputs(b, True)
        h = po.softplus(d["t"][:, 1:, 3].double(), po.HOMOG[0]) + po.HOMOG[1]
        # every case holds the floor, the linear branch and the clamp
        assert (h < 0.2500001).any() and (d["t"][:, 1:, 3] * po.HOMOG[0] > 20).any() and (h > po.HOMOG[2]).any()
        for homog in (True, False):
            _power(f"encode b={b} homog={homog}", cases.encode_reference(b, homog), partial(cases.encode_oracle, homog=homog))


@pytest.mark.parametrize("c", cases.EMBED_C)
def test_power_condition_of_the_embed_gate(c):
    for rows in cases.ROWS:
        for bcast in (False, True):
            _power(f"embed C={c} rows={rows} bcast={bcast}", cases.embed_reference(rows, c, bcast), cases.embed_oracle)


@pytest.mark.parametrize("c", cases.MODULATE_C)
def test_power_condition_of_the_modulate_gate(c):
    for rows in cases.ROWS:
        _power(f"modulate C={c} rows={rows}", cases.modulate_reference(rows, c), cases.modulate_oracle)


@pytest.mark.parametrize("d", cases.ATTN_D)
def test_power_condition_of_the_attention_gate(d):
    for B, H in cases.ATTN_BH:
        for S in cases.ATTN_S:
            _power(f"attn B={B} H={H} S={S} D={d}", cases.attention_reference(B, S, H, d), cases.attention_oracle)


def test_power_condition_of_the_activate_gate():
    from functools import partial
    for acts, later in cases.activate_cases():
        _power(f"activate {acts} later={later}", cases.activate_reference(5, acts, later),
               partial(cases.activate_oracle, acts=acts))


@pytest.mark.parametrize("name", cases.MODULES)
def test_power_condition_of_the_module_gate(name, golden_dir):
    g, x64, dists = cases.module_reference(name, golden_dir)
    e_eager = cases.errors(cases.flat(po.module_case(g, torch.float32)), x64)
    bad = cases.power_failures(f"module {name}", dists, e_eager)
    assert not bad, "\n".join(bad)


def test_the_gate_rejects_a_mutant_and_accepts_the_eager_run():
    d, x64, dists = cases.modulate_reference(5, 128)
    eager = cases.modulate_oracle(d, torch.float32)
    cases.gate("control", eager, eager, x64, dists)
    for m in dists:
        with pytest.raises(AssertionError):
            cases.gate("control " + m, cases.modulate_oracle(d, torch.float32, mut=frozenset([m])), eager, x64, dists)


# ---- checks that raise before any launch -----------------------------------------------------------------------------
def test_cpu_tensors_raise():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import posehead as ph
    z = torch.zeros
    calls = (lambda: ph.pool_tokens(z(2, 4, 8)), lambda: ph.encode_poses([(0, z(2, 1, 6), z(2, 1, 3), None)], 1),
             lambda: ph.embed_silu(z(2, 9), z(8, 9), z(8)), lambda: spf.modulate(z(2, 8), z(2, 24)),
             lambda: ph.trunk_attention(z(1, 2, 192), 1), lambda: spf.activate_pose(z(2, 9)),
             lambda: spf.CameraHead(128, 1, num_heads=1)([z(1, 2, 3, 128)]),
             lambda: spf.PoseHead(SimpleNamespace(enc_embed_dim=8, dec_embed_dim=8),
                                  spf.PoseHeadCfg(False, True, True))([z(2, 4, 8), z(2, 4, 8)]))
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(NotImplementedError):
        spf.modulate(z(2, 8, dtype=torch.float16), z(2, 24, dtype=torch.float16))


def test_bad_sizes_raise():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import posehead as ph
    z = torch.zeros
    with pytest.raises(ValueError, match="1 .. 32"):
        ph.trunk_attention(z(1, 33, 192), 1)                                        # S = 33
    with pytest.raises(ValueError, match="64 or 128"):
        ph.trunk_attention(z(1, 2, 96), 1)                                          # D = 32
    with pytest.raises(ValueError, match="64 or 128"):
        spf.CameraTrunkAttention(128, num_heads=4)
    with pytest.raises(ValueError, match="1 .. 32"):
        spf.CameraTrunkAttention(128, num_heads=1)(z(1, 33, 128))
    with pytest.raises(ValueError, match="multiple of 4"):
        spf.modulate(z(2, 6), z(2, 18))                                             # C % 4
    with pytest.raises(ValueError, match="multiple of 4"):
        ph.pool_tokens(z(2, 4, 6))
    with pytest.raises(RuntimeError, match="shift"):
        spf.modulate(z(2, 8), z(2, 16))
    head = spf.PoseHead(SimpleNamespace(enc_embed_dim=8, dec_embed_dim=8), spf.PoseHeadCfg(False, True, False))
    with pytest.raises(ValueError, match="perfect square"):
        head([z(2, 5, 8)])                                                          # non-square L
    with pytest.raises(ValueError, match="act_type"):
        spf.activate_pose(z(2, 9), trans_act="tanh")
    with pytest.raises(ValueError, match="act_type"):
        spf.CameraHead(128, 1, num_heads=1, fl_act="softplus")
    with pytest.raises(ValueError, match="Unsupported camera encoding"):
        spf.CameraHead(128, 1, num_heads=1, pose_encoding_type="rot6d")
    with pytest.raises(ValueError, match="cover"):
        ph.encode_poses([(1, z(2, 1, 6), z(2, 1, 3), None)], 2)
    big = z(1).expand((1 << 24) + 1, 1, 6)                                          # (a view: no memory behind it)
    with pytest.raises(RuntimeError, match="pose rows"):
        ph.encode_poses([(0, big, big[..., :3], None)], 1)
    with pytest.raises(RuntimeError, match="broadcast"):
        ph.embed_silu(z(2, 9), z(8, 9), z(8), rows=4)


def test_training_mode_dropout_raises():
    import spfsplatv2_amd as spf
    blk = spf.CameraTrunkBlock(128, 1, drop=0.1)
    with pytest.raises(NotImplementedError):
        blk.train()(torch.zeros(1, 2, 128))
    with pytest.raises(NotImplementedError):
        spf.CameraTrunkBlock(128, 1, drop_path=0.2).train()(torch.zeros(1, 2, 128))
    with pytest.raises(NotImplementedError):
        spf.CameraTrunkAttention(128, 1, attn_drop=0.1)


def test_vggt_attention_still_refuses_head_dim_128():
    import spfsplatv2_amd as spf
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.VGGTAttention(128, num_heads=4, qk_norm=True)(torch.zeros(1, 4, 128), torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.VGGTAttention(512, num_heads=4)(torch.zeros(1, 4, 512), torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(TypeError):
        spf.VGGTBlock(128, 2, attn_class=spf.CameraTrunkAttention)


def test_library_argument_checks_on_the_host(hip_lib):
    """SPF_E_INVALID with a message and no launch: the pointers are never dereferenced (no device here)."""
    import ctypes as C

    from spfsplatv2_amd import _lib
    p, err = C.c_void_p(4096), hip_lib.spf_last_error
    assert hip_lib.spf_posehead_attn_forward(p, 1, 33, 1, 64, p, None) == -1 and b"1 .. 32" in err()
    assert hip_lib.spf_posehead_attn_backward(p, p, 1, 2, 1, 32, p, None) == -1 and b"64 or 128" in err()
    assert hip_lib.spf_posehead_attn_forward(None, 1, 2, 1, 64, p, None) == -1 and b"null" in err()
    assert hip_lib.spf_posehead_modulate_forward(p, p, 2, 6, 1e-6, p, None) == -1 and b"multiple of 4" in err()
    assert hip_lib.spf_posehead_modulate_backward(p, p, p, 2, 8192, 1e-6, p, p, None) == -1 and b"multiple of 4" in err()
    assert hip_lib.spf_posehead_modulate_forward(C.c_void_p(4100), p, 2, 8, 1e-6, p, None) == -1 and b"aligned" in err()
    a = _lib.SpfPosePool()
    a.src[0], a.inner[0], a.stride[0], a.tok_stride[0], a.C[0], a.rows, a.L = 4096, 1, 8, 8, 6, 2, 1
    assert hip_lib.spf_posehead_pool_forward(C.byref(a), p, None) == -1 and b"multiple of 4" in err()
    a.C[0], a.rows = 8, 70000
    assert hip_lib.spf_posehead_pool_forward(C.byref(a), p, None) == -1 and b"rows" in err()
    a.rows, a.stride[0] = 2, 6
    assert hip_lib.spf_posehead_pool_forward(C.byref(a), p, None) == -1 and b"stride" in err()
    assert hip_lib.spf_posehead_pool_backward(None, p, p, None, None) == -1 and b"null" in err()
    e = _lib.SpfPoseEncode()
    e.rows, e.out_inner, e.out_stride, e.homogeneous = 0, 1, 9, 0
    assert hip_lib.spf_posehead_encode_forward(C.byref(e), p, p, p, None) == -1 and b"rows" in err()
    e.rows = (1 << 24) + 1
    assert hip_lib.spf_posehead_encode_forward(C.byref(e), p, p, p, None) == -1 and b"rows" in err()
    e.rows, e.homogeneous, e.beta = 2, 1, 0.0
    assert hip_lib.spf_posehead_encode_backward(C.byref(e), p, p, p, p, None) == -1 and b"beta" in err()
    assert hip_lib.spf_posehead_embed_silu_forward(p, 0, p, p, 0, 8, p, None) == -1 and b"rows" in err()
    assert hip_lib.spf_posehead_embed_silu_backward(p, 0, p, p, None, 2, 8, p, p, None, None) == -1 and b"null" in err()
    assert hip_lib.spf_posehead_activate_forward(None, p, 2, 0, 4, 0, p, p, None) == -1 and b"activation" in err()
    assert hip_lib.spf_posehead_activate_backward(p, None, None, 2, 0, 0, 0, p, None) == -1 and b"null" in err()
