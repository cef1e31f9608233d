"""Multi-view attention without a device: the C ABI's argument validation, the Python surface's argument errors (each
raised before anything is launched), the packing of ``allow``, ``decoder_view_sets`` and the float64 oracle on gathered
keys against the reference's goldens."""
import ctypes as C
from pathlib import Path

import pytest
import torch

from tests import attention_views_oracle as voracle

ROOT = Path(__file__).resolve().parents[1]


# ---- C ABI -----------------------------------------------------------------------------------------------------------
def _attn(**kw):
    from spfsplatv2_amd import _lib
    a = _lib.SpfAttn()
    a.q = a.k = a.v = 4096
    a.qpos = a.kpos = 4096
    a.q_stride = a.k_stride = a.v_stride = (C.c_int64 * 3)(3 * 64 * 8 * 2, 64 * 2, 64)
    a.B, a.H, a.Nq, a.Nk, a.D, a.dtype = 1, 2, 8, 8, 64, 0
    a.base, a.F0, a.scale = 100.0, 1.0, 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _views(words=(0b110, 0b101), Vk=3, **kw):
    from spfsplatv2_amd import _lib
    w = _lib.SpfAttnViews()
    w.Vq, w.Vk = len(words), Vk
    w.allow = (C.c_uint32 * 32)(*words)
    w.q_view_stride = w.k_view_stride = w.v_view_stride = 64 * 8 * 2
    w.dq_view_stride = w.dk_view_stride = w.dv_view_stride = 64 * 8 * 2
    w.qpos_stride = w.kpos_stride = (C.c_int64 * 2)(3 * 16, 16)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def test_symbols_are_declared_in_the_header_and_the_binding(hip_lib):
    from spfsplatv2_amd import _lib
    header = (ROOT / "include" / "spfsplat_hip.h").read_text()
    for name in ("spf_attn_views_forward", "spf_attn_views_backward"):
        assert name in header and name in _lib.SYMBOLS and hasattr(hip_lib, name)
    assert "typedef struct SpfAttnViews" in header and hasattr(_lib, "SpfAttnViews")
    for field, _ in _lib.SpfAttnViews._fields_:
        assert field in header, field
    # the struct as the header lays it out: two int32, 32 words, then ten int64
    assert C.sizeof(_lib.SpfAttnViews) == 8 + 32 * 4 + 10 * 8
    # the earlier family does not move
    assert C.sizeof(_lib.SpfAttn) == 5 * 8 + 9 * 8 + 6 * 4 + 3 * 4 + 4       # (4: tail padding to 8)


def test_abi_argument_validation_without_compute(hip_lib):
    """Bad arguments are rejected before anything touches a device (there is none here)."""
    from spfsplatv2_amd import _lib
    out, lse = C.c_void_p(4096), C.c_void_p(4096)

    def fwd(a, w, out=out, lse=lse):
        rc = hip_lib.spf_attn_views_forward(C.byref(a), C.byref(w) if w is not None else None, out, lse, None)
        return rc, hip_lib.spf_last_error()

    for bad in (dict(Vq=0), dict(Vq=33), dict(Vk=0), dict(Vk=33)):
        rc, msg = fwd(_attn(), _views(**bad))
        assert rc == -1 and b"1 .. 32" in msg, bad
    rc, msg = fwd(_attn(), _views(words=(0b110, 0)))
    assert rc == -1 and b"no key view" in msg
    rc, msg = fwd(_attn(), _views(words=(0b110, 0b1001)))
    assert rc == -1 and b"at or above Vk" in msg
    rc, msg = fwd(_attn(), _views(words=(0x80000001,), Vk=31))
    assert rc == -1 and b"at or above Vk" in msg
    rc, msg = fwd(_attn(D=32), _views())
    assert rc == -1 and b"head dim must be 64" in msg
    rc, msg = fwd(_attn(q=4100), _views())
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(), _views(k_view_stride=1026))
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(dtype=1), _views(q_view_stride=1028))       # 2056 bytes: not a multiple of 16
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(k_stride=(C.c_int64 * 3)(3072, 130, 64)), _views())
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = fwd(_attn(v=None), _views())
    assert rc == -1 and b"null" in msg
    rc, msg = fwd(_attn(), _views(), out=None)
    assert rc == -1 and b"null" in msg
    rc, msg = fwd(_attn(), _views(), lse=None)
    assert rc == -1 and b"null" in msg
    rc, msg = fwd(_attn(), None)
    assert rc == -1 and b"views is null" in msg
    rc, msg = fwd(_attn(kpos=None), _views())
    assert rc == -1 and b"both" in msg
    rc, msg = fwd(_attn(k_stride=(C.c_int64 * 3)(3072, 1 << 29, 64)), _views())     # 8 tokens reach past 2^31 elements
    assert rc == -1 and b"within 2^31 elements" in msg
    rc, msg = fwd(_attn(B=40000), _views())
    assert rc == -1 and b"65535" in msg
    assert hip_lib.spf_attn_views_forward(None, C.byref(_views()), out, lse, None) == -1

    def bwd(a, w, g, out=out, lse=lse, dout=out):
        rc = hip_lib.spf_attn_views_backward(C.byref(a), C.byref(w) if w is not None else None,
                                             C.byref(g) if g is not None else None, out, lse, dout, None)
        return rc, hip_lib.spf_last_error()

    g = _lib.SpfAttnGrads()
    rc, msg = bwd(_attn(), _views(), g)
    assert rc == -1 and b"null" in msg                                  # dq / dk / dv / delta
    g.dq = g.dk = g.dv = g.delta = 4096
    g.dq_stride = g.dk_stride = g.dv_stride = (C.c_int64 * 3)(3072, 128, 64)
    rc, msg = bwd(_attn(), _views(), None)
    assert rc == -1 and b"null" in msg
    rc, msg = bwd(_attn(), None, g)
    assert rc == -1 and b"views is null" in msg
    rc, msg = bwd(_attn(), _views(), g, dout=None)
    assert rc == -1 and b"null" in msg
    rc, msg = bwd(_attn(), _views(dk_view_stride=1026), g)
    assert rc == -1 and b"16-byte aligned" in msg
    rc, msg = bwd(_attn(), _views(words=(0, 1)), g)
    assert rc == -1 and b"no key view" in msg
    rc, msg = bwd(_attn(), _views(Vk=40), g)
    assert rc == -1 and b"1 .. 32" in msg
    rc, msg = bwd(_attn(D=128), _views(), g)
    assert rc == -1 and b"head dim must be 64" in msg
    g.dv_stride = (C.c_int64 * 3)(3072, 129, 64)
    rc, msg = bwd(_attn(), _views(), g)
    assert rc == -1 and b"16-byte aligned" in msg


# ---- Python surface --------------------------------------------------------------------------------------------------
def test_allow_is_packed_into_one_word_per_query_view():
    from spfsplatv2_amd import attention
    assert attention.allow_words([[1, 1]]) == ([0b11], 1, 2)
    assert attention.allow_words([[0, 1, 0], [0, 0, 1]]) == ([0b010, 0b100], 2, 3)
    assert attention.allow_words(torch.tensor([[True, False, True], [False, True, True]])) == ([0b101, 0b110], 2, 3)
    full = torch.ones(32, 32, dtype=torch.bool)
    words, Vq, Vk = attention.allow_words(full)
    assert (Vq, Vk) == (32, 32) and words == [0xffffffff] * 32
    only_last = torch.zeros(1, 32, dtype=torch.bool)
    only_last[0, 31] = True
    assert attention.allow_words(only_last)[0] == [1 << 31]
    gen = torch.Generator().manual_seed(1)
    t = torch.rand(7, 11, generator=gen) < 0.5
    t[:, 0] = True
    words, _, _ = attention.allow_words(t)
    for i in range(7):
        for s in range(11):
            assert bool(words[i] >> s & 1) == bool(t[i, s])
    # the words as the C struct carries them
    w = (C.c_uint32 * 32)(*attention.allow_words(only_last)[0])
    assert w[0] == 0x80000000 and w[1] == 0


def test_decoder_view_sets():
    import spfsplatv2_amd as spf

    def sets(v, nt):
        (q1, k1, a1), (q2, k2, a2) = spf.decoder_view_sets(v, nt)
        for a in (a1, a2):
            assert isinstance(a, torch.Tensor) and a.dtype == torch.bool and not a.is_cuda
        return (q1, k1, a1.int().tolist()), (q2, k2, a2.int().tolist())

    assert sets(2, 0) == ((slice(0, 1), slice(1, 2), [[1]]), (slice(1, 2), slice(0, 2), [[1, 0]]))
    assert sets(3, 0) == ((slice(0, 1), slice(1, 3), [[1, 1]]),
                          (slice(1, 3), slice(0, 3), [[1, 0, 1], [1, 1, 0]]))
    assert sets(3, 1) == ((slice(0, 1), slice(1, 2), [[1]]),
                          (slice(1, 3), slice(0, 3), [[1, 0, 0], [1, 1, 0]]))
    assert sets(4, 2) == ((slice(0, 1), slice(1, 2), [[1]]),
                          (slice(1, 4), slice(0, 4), [[1, 0, 0, 0], [1, 1, 0, 1], [1, 1, 1, 0]]))
    b1, b2 = sets(10, 0)
    assert b1 == (slice(0, 1), slice(1, 10), [[1] * 9])
    assert b2[:2] == (slice(1, 10), slice(0, 10))
    assert b2[2] == [[int(s != i) for s in range(10)] for i in range(1, 10)]
    with pytest.raises(ValueError, match="context views"):
        spf.decoder_view_sets(2, 1)
    with pytest.raises(ValueError, match="context views"):
        spf.decoder_view_sets(1, 0)
    with pytest.raises(ValueError, match="at most 32"):
        spf.decoder_view_sets(33, 0)
    blk1, blk2 = spf.decoder_view_sets(4, 1)
    assert blk2.query == slice(1, 4) and blk2.key == slice(0, 4) and tuple(blk2.allow.shape) == (3, 4)
    assert blk1.query == slice(0, 1) and blk1.key == slice(1, 3)


def _qkv(b=1, Vq=2, Vk=3, H=2, Nq=4, Nk=6, D=64, dtype=torch.float32):
    pos = lambda V, n: torch.zeros(b, V, n, 2, dtype=torch.int64)
    return (torch.zeros(b, Vq, H, Nq, D, dtype=dtype), torch.zeros(b, Vk, H, Nk, D, dtype=dtype),
            torch.zeros(b, Vk, H, Nk, D, dtype=dtype), pos(Vq, Nq), pos(Vk, Nk))


ALLOW = [[0, 1, 1], [1, 0, 1]]


def test_functional_errors_raise_before_any_launch():
    import spfsplatv2_amd as spf
    assert "rope_attention_views" in spf.__all__ and "decoder_view_sets" in spf.__all__
    q, k, v, qpos, kpos = _qkv()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.rope_attention_views(q, k, v, allow=torch.tensor(ALLOW, dtype=torch.bool))
    with pytest.raises(TypeError):
        spf.rope_attention_views(q, k, v, qpos, kpos)                   # allow is required
    with pytest.raises(ValueError, match="allowed no key view"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=[[0, 1, 1], [0, 0, 0]])
    with pytest.raises(ValueError, match="1 .. 32"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=torch.ones(2, 33, dtype=torch.bool))
    with pytest.raises(ValueError, match="1 .. 32"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=[])
    with pytest.raises(RuntimeError, match="must be bool"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=torch.ones(2, 3))
    with pytest.raises(RuntimeError, match=r"must be \[Vq, Vk\]"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=torch.ones(3, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="differ in length"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=[[1, 1, 1], [1, 1]])
    with pytest.raises(TypeError, match="nested sequence"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=3)
    with pytest.raises(RuntimeError, match=r"allow is \[2, 2\]"):
        spf.rope_attention_views(q, k, v, qpos, kpos, allow=[[1, 1], [1, 1]])
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.rope_attention_views(*_qkv(D=32), allow=ALLOW)
    with pytest.raises(RuntimeError, match="5 dimensions"):
        spf.rope_attention_views(q[0], k, v, qpos, kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match="differ in dtype"):
        spf.rope_attention_views(q, k.half(), v, qpos, kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        spf.rope_attention_views(q.double(), k.double(), v.double(), qpos, kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match="shapes differ"):
        spf.rope_attention_views(q, k, v[:, :, :, :5], qpos, kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match="shapes differ"):
        spf.rope_attention_views(q, k[:, :, :1], v[:, :, :1], qpos, kpos, allow=ALLOW)      # heads
    with pytest.raises(RuntimeError, match="both be given or both be None"):
        spf.rope_attention_views(q, k, v, qpos, None, allow=ALLOW)
    with pytest.raises(RuntimeError, match="positions must be int64"):
        spf.rope_attention_views(q, k, v, qpos.int(), kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match=r"qpos must be \[b, V, N, 2\]"):
        spf.rope_attention_views(q, k, v, qpos[:, 0], kpos, allow=ALLOW)
    with pytest.raises(RuntimeError, match=r"kpos must be \[b, V, N, 2\]"):
        spf.rope_attention_views(q, k, v, qpos, qpos, allow=ALLOW)


def test_module_errors_raise_before_any_launch():
    import spfsplatv2_amd as spf
    cross = spf.CrossAttention(128, rope=spf.cuRoPE2D(100.0), num_heads=2)
    query, key = torch.zeros(1, 2, 4, 128), torch.zeros(1, 3, 6, 128)
    qpos, kpos = torch.zeros(1, 2, 4, 2, dtype=torch.int64), torch.zeros(1, 3, 6, 2, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cross.forward_views(query, key, qpos, kpos, ALLOW)
    with pytest.raises(RuntimeError, match=r"allow is \[2, 2\]"):
        cross.forward_views(query, key, qpos, kpos, [[1, 1], [1, 1]])
    with pytest.raises(ValueError, match="allowed no key view"):
        cross.forward_views(query, key, qpos, kpos, [[1, 1, 1], [0, 0, 0]])
    with pytest.raises(RuntimeError, match=r"must be \[b, V, N, C\]"):
        cross.forward_views(query[0], key, qpos, kpos, ALLOW)
    with pytest.raises(ValueError, match="head dim must be 64"):
        spf.CrossAttention(128, num_heads=1).forward_views(query, key, qpos, kpos, ALLOW)
    with pytest.raises(NotImplementedError, match="attn_drop"):
        spf.CrossAttention(128, num_heads=2, attn_drop=0.1).forward_views(query, key, qpos, kpos, ALLOW)
    # the same parameters and state-dict keys as before: forward_views adds none
    assert sorted(cross.state_dict()) == ["proj.bias", "proj.weight", "projk.weight", "projq.weight", "projv.weight"]


# ---- goldens ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens(golden_dir):
    return torch.load(golden_dir / "attention_views_goldens.pt", weights_only=True)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_goldens_cover_the_case(goldens, golden_dir):
    import spfsplatv2_amd as spf
    case = goldens["blk2_2x4x37_t1"]
    assert tuple(case["x"].shape) == (2, 4, 37, 128) and tuple(case["pos"].shape) == (2, 4, 37, 2)
    assert tuple(case["out"].shape) == (2, 3, 37, 128) and case["num_heads"] == 2
    blk2 = spf.decoder_view_sets(case["v"], case["num_target"])[1]
    assert torch.equal(case["allow"], blk2.allow)
    assert (blk2.query, blk2.key) == (slice(*case["query_views"]), slice(*case["key_views"]))
    assert sorted(case["grads"]) == sorted(["x"] + list(case["weights"]))
    assert sorted(spf.CrossAttention(128, num_heads=2, qkv_bias=True).state_dict()) == sorted(case["weights"])
    assert (golden_dir / "attention_views_goldens.pt").stat().st_size < 1 << 20


def test_oracle_on_gathered_keys_matches_reference_goldens(goldens):
    """The float64 oracle on keys gathered by this test's own index_select against the reference's float32 run (two
    calls of its layer).  Bound: tests/test_attention.py's, 64 ulp of the tensor's scale -- the chains here are no
    longer than there (products of at most 128 terms, a softmax over at most 111 keys, weight gradients summed over
    222 tokens): an order above what they lose, four below a wrong gather (a view missing, doubled or out of order: O(1))."""
    case = goldens["blk2_2x4x37_t1"]
    out, grads = voracle.golden_case(case)
    tol = 64 * 2.0 ** -23
    assert _rel(case["out"], out) < tol
    for k in case["grads"]:
        assert _rel(case["grads"][k], grads[k]) < tol, k
    # the gather decides the result: with every other view allowed for the context views too, the output moves by O(1)
    wrong = dict(case, allow=torch.tensor([[s != i for s in range(4)] for i in range(1, 4)]))
    assert _rel(case["out"], voracle.golden_case(wrong)[0]) > 1e-2
