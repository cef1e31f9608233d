"""Fused attention without a device: the oracle against the reference's goldens, the argument errors of the Python
surface (each raised before anything is launched), state-dict compatibility and the C ABI's argument validation."""
import ctypes as C

import pytest
import torch

from tests import attention_oracle as oracle


@pytest.fixture(scope="module")
def goldens(golden_dir):
    cases = dict(torch.load(golden_dir / "attention_goldens.pt", weights_only=True))
    cases.update(torch.load(golden_dir / "attention_goldens_cross.pt", weights_only=True))
    return cases


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("name", ["self_2x3x70", "cross_2x2x66_131", "self_norope_1x1x5"])
def test_oracle_matches_reference_goldens(goldens, name):
    """The float64 oracle against the reference's float32 run.  Bound: the reference's chain is three products of at
    most 192 float32 terms around a softmax; 64 ulp (7.6e-6) of the tensor's scale is an order above what such chains
    lose and four below a wrong formula (a swapped half, a missing scale: O(1))."""
    case = goldens[name]
    out, grads = oracle.golden_case(case)
    tol = 64 * 2.0 ** -23
    assert _rel(case["out"], out) < tol
    for k in case["inputs"]:
        assert _rel(case["grads"][k], grads[k]) < tol, k


def test_goldens_cover_the_cases(goldens):
    assert tuple(goldens["self_2x3x70"]["x"].shape) == (2, 70, 192)
    c = goldens["cross_2x2x66_131"]
    assert tuple(c["query"].shape) == (2, 66, 128) and tuple(c["memory"].shape) == (2, 131, 128)
    assert goldens["self_norope_1x1x5"]["base"] is None
    # the extra tokens' positions lie outside the patch grid (one row below it, column 0)
    pos = goldens["self_2x3x70"]["xpos"]
    assert pos[0, -1].tolist() == [18, 0] and pos[0, -2].tolist() == [17, 0] and pos[0, :68, 0].max() == 16


def test_state_dict_keys_and_loading(goldens):
    import spfsplatv2_amd as spf
    for name in ("Attention", "CrossAttention", "rope_attention", "rope_attention_packed"):
        assert name in spf.__all__ and hasattr(spf, name)
    a = spf.Attention(192, rope=spf.cuRoPE2D(100.0), num_heads=3, qkv_bias=True)
    assert sorted(a.state_dict()) == sorted(goldens["self_2x3x70"]["weights"])
    a.load_state_dict(goldens["self_2x3x70"]["weights"], strict=True)
    c = spf.CrossAttention(128, rope=spf.cuRoPE2D(100.0), num_heads=2, qkv_bias=True)
    assert sorted(c.state_dict()) == sorted(goldens["cross_2x2x66_131"]["weights"])
    c.load_state_dict(goldens["cross_2x2x66_131"]["weights"], strict=True)
    assert sorted(spf.Attention(128, num_heads=2).state_dict()) == ["proj.bias", "proj.weight", "qkv.weight"]
    assert isinstance(a.qkv, torch.nn.Linear) and isinstance(c.projq, torch.nn.Linear)
    assert a.scale == 64 ** -0.5 and c.num_heads == 2


def _qkv(B=1, H=2, Nq=4, Nk=6, D=64, dtype=torch.float32):
    pos = lambda n: torch.zeros(B, n, 2, dtype=torch.int64)
    return (torch.zeros(B, H, Nq, D, dtype=dtype), torch.zeros(B, H, Nk, D, dtype=dtype),
            torch.zeros(B, H, Nk, D, dtype=dtype), pos(Nq), pos(Nk))


def test_functional_errors_raise_before_any_launch():
    import spfsplatv2_amd as spf
    q, k, v, qpos, kpos = _qkv()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention(q, k, v, qpos, kpos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention(q, k, v)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 64), torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.rope_attention(*_qkv(D=32))
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 128))
    with pytest.raises(RuntimeError, match="must be \\[B,N,3,H,D\\]"):
        spf.rope_attention_packed(torch.zeros(1, 4, 2, 2, 64))
    with pytest.raises(RuntimeError, match="differ in dtype"):
        spf.rope_attention(q, k.half(), v, qpos, kpos)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        spf.rope_attention(q.double(), k.double(), v.double(), qpos, kpos)
    with pytest.raises(RuntimeError, match="positions must be int64"):
        spf.rope_attention(q, k, v, qpos.int(), kpos)
    with pytest.raises(RuntimeError, match="positions are not contiguous"):
        spf.rope_attention(q, k, v, torch.zeros(1, 2, 4, dtype=torch.int64).transpose(1, 2), kpos)
    with pytest.raises(RuntimeError, match="seq_length differs between tokens & positions"):
        spf.rope_attention(q, k, v, qpos, qpos)
    with pytest.raises(RuntimeError, match="batch size differs between tokens & positions"):
        spf.rope_attention(q, k, v, qpos.repeat(2, 1, 1), kpos)
    with pytest.raises(RuntimeError, match=r"positions.shape\[2\] must be equal to 2"):
        spf.rope_attention(q, k, v, torch.zeros(1, 4, 3, dtype=torch.int64), kpos)
    with pytest.raises(RuntimeError, match="positions must have 3 dimensions"):
        spf.rope_attention(q, k, v, qpos[0], kpos)
    with pytest.raises(RuntimeError, match="tokens must have 4 dimensions"):
        spf.rope_attention(q[0], k, v, qpos, kpos)
    with pytest.raises(RuntimeError, match="shapes differ"):
        spf.rope_attention(q, k, v[:, :, :5], qpos, kpos)
    with pytest.raises(RuntimeError, match="both be given or both be None"):
        spf.rope_attention(q, k, v, qpos, None)


def test_module_errors_raise_before_any_launch():
    import spfsplatv2_amd as spf
    x, pos = torch.zeros(1, 4, 128), torch.zeros(1, 4, 2, dtype=torch.int64)
    att = spf.Attention(128, rope=spf.cuRoPE2D(100.0), num_heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        att(x, pos)
    cross = spf.CrossAttention(128, rope=None, num_heads=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cross(x, x, x, pos, pos)
    with pytest.raises(NotImplementedError, match="mask"):
        cross(x, x, x, pos, pos, mask=torch.zeros(1, 4, 4))
    drop = spf.Attention(128, num_heads=2, attn_drop=0.1)
    with pytest.raises(NotImplementedError, match="attn_drop"):
        drop(x, pos)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # dropout is the identity in eval mode
        drop.eval()(x, pos)
    dropc = spf.CrossAttention(128, num_heads=2, attn_drop=0.1)
    with pytest.raises(NotImplementedError, match="attn_drop"):
        dropc(x, x, x, pos, pos)
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.Attention(128, num_heads=4)(x, pos)
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.CrossAttention(128, num_heads=1)(x, x, x, pos, pos)
    with pytest.raises(TypeError, match="cuRoPE2D"):
        spf.Attention(128, rope=object(), num_heads=2)(x, pos)
    # the modules' own wording of the CPU refusal, whole
    with pytest.raises(RuntimeError, match=r"^Attention: x is on the CPU; this build only runs on a HIP device "
                                           r"\(no CPU fallback\)$"):
        att(x, pos)
    with pytest.raises(RuntimeError, match=r"^CrossAttention: query is on the CPU; this build only runs on a HIP device "
                                           r"\(no CPU fallback\)$"):
        cross(x, x, x, pos, pos)
    with pytest.raises(RuntimeError, match=r"^CrossAttention: query is on the CPU; this build only runs on a HIP device "
                                           r"\(no CPU fallback\)$"):
        cross.forward_views(x[None], x[None], pos[None], pos[None], [[True]])
    with pytest.raises(TypeError, match="cuRoPE2D"):                  # the rope's refusal comes before the CPU's
        bad = spf.CrossAttention(128, rope=object(), num_heads=2)
        bad.forward_views(x[None], x[None], pos[None], pos[None], [[True]])


def _attn(**kw):
    from spfsplatv2_amd import _lib
    a = _lib.SpfAttn()
    a.q = a.k = a.v = 4096
    a.qpos = a.kpos = 4096
    a.q_stride = a.k_stride = a.v_stride = (C.c_int64 * 3)(64 * 8 * 2, 64 * 2, 64)
    a.B, a.H, a.Nq, a.Nk, a.D, a.dtype = 1, 2, 8, 8, 64, 0
    a.base, a.F0, a.scale = 100.0, 1.0, 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_abi_argument_validation_without_compute(hip_lib):
    """Bad arguments are rejected before anything touches a device (there is none here)."""
    from spfsplatv2_amd import _lib
    assert hip_lib.spf_abi_version() == _lib.ABI_VERSION
    out, lse = C.c_void_p(4096), C.c_void_p(4096)

    def fwd(a, out=out, lse=lse):
        return hip_lib.spf_attn_forward(C.byref(a), out, lse, None), hip_lib.spf_last_error()

    rc, msg = fwd(_attn(q=None))
    assert rc == -1 and b"null" in msg
    rc, msg = fwd(_attn(), out=None)
    assert rc == -1 and b"null" in msg
    rc, msg = fwd(_attn(kpos=None))
    assert rc == -1 and b"both" in msg
    rc, msg = fwd(_attn(D=32))
    assert rc == -1 and b"head dim must be 64" in msg
    for field in ("B", "H", "Nq", "Nk"):
        rc, msg = fwd(_attn(**{field: 0}))
        assert rc == -1 and b"positive" in msg, field
    rc, msg = fwd(_attn(dtype=3))
    assert rc == -1 and b"dtype" in msg
    rc, msg = fwd(_attn(q=4100))
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(k_stride=(C.c_int64 * 3)(1024, 130, 64)))
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(dtype=1, v_stride=(C.c_int64 * 3)(1024, 132, 64)))     # 264 bytes: not a multiple of 16
    assert rc == -1 and b"16-byte aligned" in msg
    assert hip_lib.spf_attn_forward(None, out, lse, None) == -1

    g = _lib.SpfAttnGrads()
    rc = hip_lib.spf_attn_backward(C.byref(_attn()), C.byref(g), out, lse, out, None)
    assert rc == -1 and b"null" in hip_lib.spf_last_error()
    g.dq = g.dk = g.dv = g.delta = 4096
    g.dq_stride = g.dk_stride = (C.c_int64 * 3)(1024, 128, 64)
    g.dv_stride = (C.c_int64 * 3)(1024, 129, 64)
    rc = hip_lib.spf_attn_backward(C.byref(_attn()), C.byref(g), out, lse, out, None)
    assert rc == -1 and b"16-byte aligned" in hip_lib.spf_last_error()
    rc = hip_lib.spf_attn_backward(C.byref(_attn()), C.byref(g), out, None, out, None)
    assert rc == -1 and b"null" in hip_lib.spf_last_error()
    rc = hip_lib.spf_attn_backward(C.byref(_attn(D=128)), C.byref(g), out, lse, out, None)
    assert rc == -1 and b"head dim must be 64" in hip_lib.spf_last_error()
    rc = hip_lib.spf_attn_backward(C.byref(_attn()), None, out, lse, out, None)
    assert rc == -1
