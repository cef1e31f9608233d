"""VGGT attention without a device: the oracle against the reference's goldens, state-dict compatibility, the argument
errors of the Python surface (each raised before anything is launched) and the C ABI's additions."""
import ctypes as C
import re

import pytest
import torch
from torch import nn

from tests import vggt_attention_oracle as oracle


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "vggt_attention_goldens.pt", weights_only=True)


def _rel(a, b, den=None):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() if den is None else den))


@pytest.mark.parametrize("name", ["mask_rope", "rope", "mask"])
def test_oracle_matches_reference_goldens(gold, name):
    """The float64 oracle against the reference's float32 run.  Bound as in test_attention.py: 64 ulp (7.6e-6) of the
    tensor's scale, an order above what these float32 chains lose and four below a wrong formula.  Without a rotation
    the k bias has no gradient in exact arithmetic (oracle.k_bias_cancel_scale): that one is measured against the
    magnitude of the terms that cancel."""
    case, probe = gold["cases"][name], {}
    out, dx, dparams = oracle.golden_case(gold, name, probe=probe)
    tol = 64 * 2.0 ** -23
    assert _rel(case["out"], out) < tol
    assert _rel(case["dx"], dx) < tol
    assert set(case["dparams"]) == {"qkv.bias", "proj.bias", "q_norm.weight", "q_norm.bias", "k_norm.weight", "k_norm.bias"}
    for k, g in case["dparams"].items():
        den = oracle.k_bias_cancel_scale(probe) if (k == "k_norm.bias" and not case["rope"]) else None
        assert _rel(g, dparams[k], den) < tol, k


def test_goldens_cover_the_cases(gold):
    S, P = gold["S"], gold["P"]
    assert (S, P) == (3, 23) and tuple(gold["x"].shape) == (2, 69, 128) and gold["num_heads"] == 2
    mask, pos = gold["mask"], gold["pos"]
    assert tuple(mask.shape) == (1, 1, 69, 69) and mask.dtype == torch.float32
    # context views (the first two) may not attend to the target view; the target view sees everything
    assert torch.isinf(mask[0, 0, :46, 46:]).all() and (mask[0, 0, :46, :46] == 0).all() and (mask[0, 0, 46:] == 0).all()
    # special tokens at (0, 0), the patch grid shifted by one
    assert pos[0, :3].abs().sum() == 0 and pos[0, 3].tolist() == [1, 1] and pos[0, 22].tolist() == [4, 5]
    assert torch.equal(pos[0, :23], pos[0, 23:46]) and torch.equal(pos[0], pos[1])
    assert [(c["mask"], c["rope"]) for c in gold["cases"].values()] == [(True, True), (False, True), (True, False)]


def test_state_dict_keys_and_loading(gold):
    import spfsplatv2_amd as spf
    assert "VGGTAttention" in spf.__all__ and hasattr(spf, "VGGTAttention")
    m = spf.VGGTAttention(128, num_heads=2, qk_norm=True, rope=spf.RotaryPositionEmbedding2D(100.0))
    assert sorted(m.state_dict()) == sorted(gold["weights"])
    assert sorted(gold["weights"]) == ["k_norm.bias", "k_norm.weight", "proj.bias", "proj.weight", "q_norm.bias",
                                       "q_norm.weight", "qkv.bias", "qkv.weight"]
    m.load_state_dict(gold["weights"], strict=True)
    plain = spf.VGGTAttention(128, num_heads=2, qkv_bias=False, proj_bias=False)
    assert sorted(plain.state_dict()) == ["proj.weight", "qkv.weight"]
    assert isinstance(plain.q_norm, nn.Identity) and isinstance(m.k_norm, nn.LayerNorm)
    assert m.scale == 64 ** -0.5 and m.head_dim == 64 and m.fused_attn is True
    assert spf.VGGTAttention(128, num_heads=2, fused_attn=False).fused_attn is False


def test_module_errors_raise_before_any_launch():
    import spfsplatv2_amd as spf
    x, pos = torch.zeros(1, 4, 128), torch.zeros(1, 4, 2, dtype=torch.int64)
    rope = spf.RotaryPositionEmbedding2D(100.0)
    ok = spf.VGGTAttention(128, num_heads=2, qk_norm=True, rope=rope)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ok(x, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ok(x, pos, mask=torch.zeros(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.VGGTAttention(128, num_heads=2)(x)
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.VGGTAttention(128, num_heads=4, qk_norm=True)(x, pos)
    with pytest.raises(TypeError, match="nn.LayerNorm"):
        spf.VGGTAttention(128, num_heads=2, qk_norm=True, norm_layer=nn.BatchNorm1d)(x, pos)
    with pytest.raises(TypeError, match="nn.LayerNorm"):
        spf.VGGTAttention(128, num_heads=2, qk_norm=True,
                          norm_layer=lambda d: nn.LayerNorm(d, elementwise_affine=False))(x, pos)
    with pytest.raises(TypeError, match="nn.LayerNorm"):
        spf.VGGTAttention(128, num_heads=2, qk_norm=True, norm_layer=lambda d: nn.LayerNorm(d, bias=False))(x, pos)
    with pytest.raises(TypeError, match="nn.LayerNorm"):
        spf.VGGTAttention(128, num_heads=2, qk_norm=True, norm_layer=lambda d: nn.LayerNorm((1, d)))(x, pos)
    with pytest.raises(RuntimeError, match="float32 .* or bool"):
        ok(x, pos, mask=torch.zeros(4, 4, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="float32 .* or bool"):
        ok(x, pos, mask=torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="not differentiable"):
        ok(x, pos, mask=torch.zeros(4, 4, requires_grad=True))
    with pytest.raises(RuntimeError, match="does not broadcast"):
        ok(x, pos, mask=torch.zeros(1, 1, 4, 5))
    with pytest.raises(RuntimeError, match="does not broadcast"):
        ok(x, pos, mask=torch.zeros(3, 1, 4, 4))
    with pytest.raises(RuntimeError, match="2 to 4 dimensions"):
        ok(x, pos, mask=torch.zeros(4))
    with pytest.raises(RuntimeError, match="2 to 4 dimensions"):
        ok(x, pos, mask=torch.zeros(1, 1, 1, 4, 4))
    with pytest.raises(NotImplementedError, match="attn_drop"):
        spf.VGGTAttention(128, num_heads=2, attn_drop=0.1)(x, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # dropout is the identity in eval mode
        spf.VGGTAttention(128, num_heads=2, attn_drop=0.1).eval()(x, pos)
    with pytest.raises(TypeError, match="RotaryPositionEmbedding2D"):
        spf.VGGTAttention(128, num_heads=2, rope=object())(x, pos)
    with pytest.raises(RuntimeError, match="pos must be given"):
        ok(x)


def test_functional_errors_raise_before_any_launch():
    import spfsplatv2_amd as spf
    q, k, v = torch.zeros(1, 2, 4, 64), torch.zeros(1, 2, 6, 64), torch.zeros(1, 2, 6, 64)
    w, b = torch.ones(64), torch.zeros(64)
    norm = (w, b, 1e-5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention(q, k, v, mask=torch.zeros(4, 6), q_norm=norm, k_norm=norm)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention(q, k, v, mask=torch.ones(2, 1, 6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 64), mask=torch.zeros(1, 1, 4, 4), q_norm=norm, k_norm=norm)
    with pytest.raises(RuntimeError, match="float32 .* or bool"):
        spf.rope_attention(q, k, v, mask=torch.zeros(4, 6, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="not differentiable"):
        spf.rope_attention(q, k, v, mask=torch.zeros(4, 6, requires_grad=True))
    with pytest.raises(RuntimeError, match="does not broadcast"):
        spf.rope_attention(q, k, v, mask=torch.zeros(6, 4))
    with pytest.raises(RuntimeError, match="does not broadcast"):
        spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 64), mask=torch.zeros(1, 3, 4, 4))
    with pytest.raises(RuntimeError, match="2 to 4 dimensions"):
        spf.rope_attention(q, k, v, mask=torch.zeros(6))
    with pytest.raises(TypeError, match="tensor or None"):
        spf.rope_attention(q, k, v, mask=[[0.0]])
    with pytest.raises(RuntimeError, match="both be given or both be None"):
        spf.rope_attention(q, k, v, q_norm=norm)
    with pytest.raises(TypeError, match="weight, bias, eps"):
        spf.rope_attention(q, k, v, q_norm=(w, b), k_norm=norm)
    with pytest.raises(RuntimeError, match=r"float32 tensors of shape \[64\]"):
        spf.rope_attention(q, k, v, q_norm=(torch.ones(32), b, 1e-5), k_norm=norm)
    with pytest.raises(RuntimeError, match=r"float32 tensors of shape \[64\]"):
        spf.rope_attention(q, k, v, q_norm=norm, k_norm=(w, b.half(), 1e-5))
    with pytest.raises(ValueError, match="share one eps"):
        spf.rope_attention(q, k, v, q_norm=norm, k_norm=(w, b, 1e-6))
    # CroCo's classes keep refusing a mask
    with pytest.raises(NotImplementedError, match="mask"):
        x, pos = torch.zeros(1, 4, 128), torch.zeros(1, 4, 2, dtype=torch.int64)
        spf.CrossAttention(128, num_heads=2)(x, x, x, pos, pos, mask=torch.zeros(1, 4, 4))


def test_mask_view_strides():
    """What the kernels are handed: broadcast axes get stride 0 and nothing is copied; a mask without unit key stride is
    copied once."""
    from spfsplatv2_amd import attention
    shape = (2, 3, 5, 7)
    m = torch.zeros(1, 1, 5, 7)
    v = attention._mask_view(m, shape)
    assert v.data_ptr() == m.data_ptr() and v.stride() == (0, 0, 7, 1) and tuple(v.shape) == shape
    v = attention._mask_view(torch.zeros(5, 7), shape)
    assert v.stride() == (0, 0, 7, 1)
    v = attention._mask_view(torch.zeros(2, 1, 5, 7), shape)
    assert v.stride() == (35, 0, 7, 1)
    v = attention._mask_view(torch.zeros(3, 1, 7), shape)
    assert v.stride() == (0, 7, 0, 1)
    t = torch.zeros(7, 5).t()                                           # key stride 5: copied
    v = attention._mask_view(t, shape)
    assert v.data_ptr() != t.data_ptr() and v.stride() == (0, 0, 7, 1)
    v = attention._mask_view(torch.zeros(5, 1), shape)                  # broadcast along the keys: copied
    assert v.stride() == (0, 0, 7, 1)
    assert attention._mask_view(None, shape) is None


def test_new_symbols_in_header_and_bindings(hip_lib):
    from pathlib import Path

    from spfsplatv2_amd import _lib
    header = (Path(__file__).resolve().parents[1] / "include" / "spfsplat_hip.h").read_text()
    for name in ("spf_attn_forward_ext", "spf_attn_backward_ext", "spf_attn_ext_scratch_floats"):
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    assert "typedef struct SpfAttnExt" in header and hasattr(_lib, "SpfAttnExt")
    assert hip_lib.spf_abi_version() == 7 == _lib.ABI_VERSION
    assert "#define SPF_ABI_VERSION 7" in header


def _attn(**kw):
    from spfsplatv2_amd import _lib
    a = _lib.SpfAttn()
    a.q = a.k = a.v = 4096
    a.q_stride = a.k_stride = a.v_stride = (C.c_int64 * 3)(64 * 8 * 2, 64 * 2, 64)
    a.B, a.H, a.Nq, a.Nk, a.D, a.dtype = 1, 2, 8, 8, 64, 0
    a.base, a.F0, a.scale = 100.0, 1.0, 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _ext(**kw):
    from spfsplatv2_amd import _lib
    e = _lib.SpfAttnExt()
    e.mask, e.mask_dtype = 4096, 0
    e.mask_stride = (C.c_int64 * 4)(0, 0, 8, 1)
    e.q_weight = e.q_bias = e.k_weight = e.k_bias = 4096
    e.eps = 1e-5
    for k, v in kw.items():
        setattr(e, k, v)
    return e


def test_abi_argument_validation_without_compute(hip_lib):
    """Bad extras are rejected before anything touches a device (there is none here)."""
    from spfsplatv2_amd import _lib
    out, lse = C.c_void_p(4096), C.c_void_p(4096)

    def fwd(a, e):
        rc = hip_lib.spf_attn_forward_ext(C.byref(a), C.byref(e) if e is not None else None, out, lse, None)
        return rc, hip_lib.spf_last_error()

    rc, msg = fwd(_attn(), None)
    assert rc == -1 and b"ext is null" in msg
    rc, msg = fwd(_attn(), _ext(mask_dtype=2))
    assert rc == -1 and b"mask_dtype" in msg
    rc, msg = fwd(_attn(), _ext(mask_stride=(C.c_int64 * 4)(0, 0, 8, 2)))
    assert rc == -1 and b"key stride must be 1" in msg
    rc, msg = fwd(_attn(), _ext(mask_stride=(C.c_int64 * 4)(0, -1, 8, 1)))
    assert rc == -1 and b"negative" in msg
    rc, msg = fwd(_attn(), _ext(mask=4098))
    assert rc == -1 and b"4-byte aligned" in msg
    rc, msg = fwd(_attn(), _ext(k_bias=None))
    assert rc == -1 and b"all be given or all be null" in msg
    rc, msg = fwd(_attn(), _ext(eps=-1.0))
    assert rc == -1 and b"eps" in msg
    rc, msg = fwd(_attn(D=32), _ext())
    assert rc == -1 and b"head dim must be 64" in msg
    rc, msg = fwd(_attn(q=None), _ext(mask=None))
    assert rc == -1 and b"null" in msg
    # without a mask and without parameters it is the plain call, with the plain call's checks
    rc, msg = fwd(_attn(Nk=0), _lib.SpfAttnExt())
    assert rc == -1 and b"positive" in msg

    g = _lib.SpfAttnGrads()
    g.dq = g.dk = g.dv = g.delta = 4096
    g.dq_stride = g.dk_stride = g.dv_stride = (C.c_int64 * 3)(1024, 128, 64)
    rc = hip_lib.spf_attn_backward_ext(C.byref(_attn()), C.byref(g), C.byref(_ext()), out, lse, out, None)
    assert rc == -1 and b"partials is null" in hip_lib.spf_last_error()
    rc = hip_lib.spf_attn_backward_ext(C.byref(_attn()), None, C.byref(_ext()), out, lse, out, None)
    assert rc == -1 and b"grads is null" in hip_lib.spf_last_error()
    rc = hip_lib.spf_attn_backward_ext(C.byref(_attn()), C.byref(g), None, out, lse, out, None)
    assert rc == -1 and b"ext is null" in hip_lib.spf_last_error()
    g.dv_stride = (C.c_int64 * 3)(1024, 129, 64)
    full = _ext(dq_weight=4096, dq_bias=4096, dk_weight=4096, dk_bias=4096, partials=4096)
    rc = hip_lib.spf_attn_backward_ext(C.byref(_attn()), C.byref(g), C.byref(full), out, lse, out, None)
    assert rc == -1 and b"16-byte aligned" in hip_lib.spf_last_error()


def test_scratch_size_comes_from_the_library(hip_lib):
    f = hip_lib.spf_attn_ext_scratch_floats
    # a [2][64] partial per block of 128 owner rows, per (batch, head), for the query and for the key side
    assert f(1, 1, 1, 1) == 2 * 128
    assert f(2, 3, 128, 129) == 2 * 3 * (1 + 2) * 128
    assert f(1, 16, 786, 786) == 16 * 14 * 128
    assert f(0, 1, 1, 1) == -1 and f(1, 1, 0, 1) == -1 and f(1, 70000, 1, 1) == -1


def test_plain_and_empty_ext_calls_reject_alike(hip_lib):
    """One checker behind both entry points: every invalid plain call gets the same code and the same message from
    spf_attn_forward / spf_attn_backward and from the _ext twin with empty extras.  Nothing here reaches a launch."""
    from spfsplatv2_amd import _lib
    ok, off = C.c_void_p(4096), C.c_void_p(4100)
    empty = _lib.SpfAttnExt()
    odd = (C.c_int64 * 3)(1024, 130, 64)

    def same(plain, ext, args, want):
        ref = C.byref(args) if args is not None else None
        rc = plain(ref)
        msg = hip_lib.spf_last_error()
        rc_ext = ext(ref)
        msg_ext = hip_lib.spf_last_error()
        assert rc == rc_ext == -1 and msg == msg_ext and want in msg, (want, rc, rc_ext, msg, msg_ext)

    forward = [  # (args, out, lse, a piece of the message)
        (None, ok, ok, b"args is null"),
        (_attn(q=None), ok, ok, b"q / k / v is null"),
        (_attn(qpos=4096), ok, ok, b"qpos and kpos must both"),
        (_attn(kpos=4096), ok, ok, b"qpos and kpos must both"),
        (_attn(D=32), ok, ok, b"head dim must be 64"),
        (_attn(D=128), ok, ok, b"head dim must be 64"),
        (_attn(B=0), ok, ok, b"must be positive"),
        (_attn(H=65536), ok, ok, b"must not exceed 65535"),
        (_attn(dtype=3), ok, ok, b"dtype must be"),
        (_attn(q=4100), ok, ok, b"rows of q, k and v must be 16-byte aligned"),
        (_attn(k_stride=odd), ok, ok, b"rows of q, k and v must be 16-byte aligned"),
        (_attn(), None, ok, b"out / lse is null"),
        (_attn(), ok, None, b"out / lse is null"),
        (_attn(), off, ok, b"rows of out must be 16-byte aligned"),
    ]
    for args, out, lse, want in forward:
        same(lambda a: hip_lib.spf_attn_forward(a, out, lse, None),
             lambda a: hip_lib.spf_attn_forward_ext(a, C.byref(empty), out, lse, None), args, want)

    def grads(**kw):
        g = _lib.SpfAttnGrads()
        g.dq = g.dk = g.dv = g.delta = 4096
        g.dq_stride = g.dk_stride = g.dv_stride = (C.c_int64 * 3)(1024, 128, 64)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    backward = [  # (grads, dout, a piece of the message)
        (None, ok, b"grads is null"),
        (grads(), None, b"out / lse / dout is null"),
        (grads(delta=None), ok, b"dq / dk / dv / delta is null"),
        (grads(), off, b"rows of out and dout must be 16-byte aligned"),
        (grads(dk_stride=odd), ok, b"rows of dq, dk and dv must be 16-byte aligned"),
    ]
    for g, dout, want in backward:
        gref = C.byref(g) if g is not None else None
        same(lambda a: hip_lib.spf_attn_backward(a, gref, ok, ok, dout, None),
             lambda a: hip_lib.spf_attn_backward_ext(a, gref, C.byref(empty), ok, ok, dout, None), _attn(), want)
