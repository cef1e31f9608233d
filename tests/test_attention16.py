"""The 16-bit matrix path of the fused attention without a device: the two C entry points and their argument
validation, the refusals of ``matrix16=True`` on the Python surface (each raised before anything is launched) and the
modules' flag."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch

HEADER = Path(__file__).resolve().parents[1] / "include" / "spfsplat_hip.h"


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    from spfsplatv2_amd import _lib
    text = HEADER.read_text()
    assert re.search(r"int\s+spf_attn16_forward\s*\(\s*const SpfAttn\*[^;]*void\* out,\s*float\* lse,\s*void\* stream\)\s*;",
                     text)
    assert re.search(r"int\s+spf_attn16_backward\s*\(\s*const SpfAttn\*[^;]*const SpfAttnGrads\*[^;]*const void\* out,"
                     r"\s*const float\* lse,\s*const void\* dout,\s*void\* stream\)\s*;", text)
    for name in ("spf_attn16_forward", "spf_attn16_backward"):
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name)
    assert hip_lib.spf_abi_version() == 7 == _lib.ABI_VERSION
    assert C.sizeof(_lib.SpfAttn) == 5 * 8 + 9 * 8 + 6 * 4 + 3 * 4 + 4       # unchanged (4: tail padding to 8)


def _attn(**kw):
    from spfsplatv2_amd import _lib
    a = _lib.SpfAttn()
    a.q = a.k = a.v = 4096
    a.qpos = a.kpos = 4096
    a.q_stride = a.k_stride = a.v_stride = (C.c_int64 * 3)(64 * 8 * 2, 64 * 2, 64)
    a.B, a.H, a.Nq, a.Nk, a.D, a.dtype = 1, 2, 8, 8, 64, 1
    a.base, a.F0, a.scale = 100.0, 1.0, 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_abi_argument_validation_without_compute(hip_lib):
    """Bad arguments are rejected before anything touches a device (there is none here)."""
    from spfsplatv2_amd import _lib
    out, lse = C.c_void_p(4096), C.c_void_p(4096)

    def fwd(a, out=out, lse=lse):
        return hip_lib.spf_attn16_forward(C.byref(a), out, lse, None), hip_lib.spf_last_error()

    for dtype in (0, 3):
        rc, msg = fwd(_attn(dtype=dtype))
        assert rc == -1 and b"dtype" in msg, dtype
    rc, msg = fwd(_attn(q=None))
    assert rc == -1 and b"null" in msg
    rc, msg = fwd(_attn(), out=None)
    assert rc == -1 and b"null" in msg
    for which in ("qpos", "kpos"):
        rc, msg = fwd(_attn(**{which: None}))
        assert rc == -1 and b"both" in msg, which
    rc, msg = fwd(_attn(D=32))
    assert rc == -1 and b"head dim must be 64" in msg
    for field in ("B", "H", "Nq", "Nk"):
        rc, msg = fwd(_attn(**{field: 0}))
        assert rc == -1 and b"positive" in msg, field
    rc, msg = fwd(_attn(q=4100))
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(dtype=1, v_stride=(C.c_int64 * 3)(1024, 132, 64)))     # 264 bytes: not a multiple of 16
    assert rc == -1 and b"16-byte aligned" in msg
    assert hip_lib.spf_attn16_forward(None, out, lse, None) == -1

    def bwd(a, g, out=out, lse=lse, dout=out):
        gp = C.byref(g) if g is not None else None
        return hip_lib.spf_attn16_backward(C.byref(a), gp, out, lse, dout, None), hip_lib.spf_last_error()

    g = _lib.SpfAttnGrads()
    rc, msg = bwd(_attn(), g)                                                   # dq / dk / dv / delta are null
    assert rc == -1 and b"null" in msg
    g.dq = g.dk = g.dv = g.delta = 4096
    g.dq_stride = g.dk_stride = g.dv_stride = (C.c_int64 * 3)(1024, 128, 64)
    for dtype in (0, 3):
        rc, msg = bwd(_attn(dtype=dtype), g)
        assert rc == -1 and b"dtype" in msg, dtype
    rc, msg = bwd(_attn(q=None), g)
    assert rc == -1 and b"null" in msg
    rc, msg = bwd(_attn(), g, out=None)
    assert rc == -1 and b"null" in msg
    rc, msg = bwd(_attn(), g, lse=None)
    assert rc == -1 and b"null" in msg
    rc, msg = bwd(_attn(qpos=None), g)
    assert rc == -1 and b"both" in msg
    rc, msg = bwd(_attn(D=32), g)
    assert rc == -1 and b"head dim must be 64" in msg
    rc, msg = bwd(_attn(Nk=0), g)
    assert rc == -1 and b"positive" in msg
    rc, msg = bwd(_attn(), g, dout=C.c_void_p(4100))
    assert rc == -1 and b"16-byte aligned" in msg
    g.dv_stride = (C.c_int64 * 3)(1024, 132, 64)
    rc, msg = bwd(_attn(), g)
    assert rc == -1 and b"16-byte aligned" in msg
    rc, _ = bwd(_attn(), None)
    assert rc == -1


def _qkv(dtype, B=1, H=2, Nq=4, Nk=6):
    pos = lambda n: torch.zeros(B, n, 2, dtype=torch.int64)
    return (torch.zeros(B, H, Nq, 64, dtype=dtype), torch.zeros(B, H, Nk, 64, dtype=dtype),
            torch.zeros(B, H, Nk, 64, dtype=dtype), pos(Nq), pos(Nk))


def test_matrix16_refusals_raise_before_any_launch():
    """On CPU tensors: what the flag refuses is reported before the missing device is."""
    import spfsplatv2_amd as spf
    norm = (torch.ones(64), torch.zeros(64), 1e-6)
    with pytest.raises(ValueError, match="matrix16"):
        spf.rope_attention(*_qkv(torch.float32), matrix16=True)
    with pytest.raises(ValueError, match="matrix16"):
        spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 64), matrix16=True)
    for dtype in (torch.float16, torch.bfloat16):
        q, k, v, qpos, kpos = _qkv(dtype)
        with pytest.raises(NotImplementedError, match="matrix16"):
            spf.rope_attention(q, k, v, qpos, kpos, mask=torch.zeros(4, 6), matrix16=True)
        with pytest.raises(NotImplementedError, match="matrix16"):
            spf.rope_attention(q, k, v, qpos, kpos, q_norm=norm, k_norm=norm, matrix16=True)
        with pytest.raises(NotImplementedError, match="matrix16"):
            spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 64, dtype=dtype), mask=torch.zeros(4, 4), matrix16=True)
        with pytest.raises(NotImplementedError, match="matrix16"):
            spf.rope_attention_packed(torch.zeros(1, 4, 3, 2, 64, dtype=dtype), q_norm=norm, k_norm=norm, matrix16=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):             # accepted: only the device is missing
            spf.rope_attention(q, k, v, qpos, kpos, matrix16=True)
    with pytest.raises(TypeError):                                             # keyword-only
        spf.rope_attention(*_qkv(torch.float16), 100.0)
    with pytest.raises(TypeError, match="matrix16"):                           # the multi-view call does not take it
        spf.rope_attention_views(torch.zeros(1, 1, 2, 4, 64), torch.zeros(1, 1, 2, 4, 64), torch.zeros(1, 1, 2, 4, 64),
                                 allow=[[True]], matrix16=True)


def test_modules_take_the_flag_and_keep_their_state_dict():
    import spfsplatv2_amd as spf
    plain = spf.Attention(128, rope=spf.cuRoPE2D(100.0), num_heads=2, qkv_bias=True)
    flagged = spf.Attention(128, rope=spf.cuRoPE2D(100.0), num_heads=2, qkv_bias=True, matrix16=True)
    assert flagged.matrix16 is True and plain.matrix16 is False
    assert sorted(flagged.state_dict()) == sorted(plain.state_dict())
    flagged.load_state_dict(plain.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(flagged.state_dict().values(), plain.state_dict().values()))
    cplain = spf.CrossAttention(128, num_heads=2, qkv_bias=True)
    cflagged = spf.CrossAttention(128, num_heads=2, qkv_bias=True, matrix16=True)
    assert cflagged.matrix16 is True and cplain.matrix16 is False
    assert sorted(cflagged.state_dict()) == sorted(cplain.state_dict())
    cflagged.load_state_dict(cplain.state_dict(), strict=True)
    cplain.matrix16 = True                                                      # settable as an attribute
    assert cplain.matrix16 is True and sorted(cplain.state_dict()) == sorted(cflagged.state_dict())
    with pytest.raises(TypeError):                                              # keyword-only
        spf.Attention(128, None, 2, False, 0., 0., True)
    with pytest.raises(TypeError):
        spf.CrossAttention(128, None, 2, False, 0., 0., True)
