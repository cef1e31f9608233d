"""No GPU needed: (1) the test-only adapter oracle (oracle/adapter_ref.py) evaluated in float32 reproduces the golden
vectors captured from the reference's own UnifiedGaussianAdapter (tests/golden/make_adapter_goldens.py) -- outputs and
the gradient to the raw channels -- so the float64 arbiter of tests/test_gpu_adapter_parity.py is pinned to the reference
and not to the product; (2) the argument contract of spf_adapter_forward / spf_adapter_backward: every rejection comes
before any launch."""
import ctypes as C

import pytest
import torch

from oracle import adapter_ref

ULP = 2.0 ** -23


@pytest.mark.parametrize("deg", [0, 1, 2, 3, 4])
def test_oracle_float32_reproduces_the_reference_goldens(golden_dir, deg):
    """Same float32 operations in the same order as the reference's class, so the expectation is equality; what is
    allowed for is another CPU's vector libm behind softplus (exp, log1p: an ulp each, 2 ulp on the scales and their
    gradient) and another summation order inside the 4-element norm (1 ulp of the row on the rotations, 2 ulp of
    |g| / (|q| + eps) on their gradient).  The harmonics are one multiply: bit-exact everywhere."""
    g = torch.load(golden_dir / "adapter_goldens.pt")[f"deg{deg}"]
    K = (deg + 1) ** 2
    mask = adapter_ref.sh_mask(deg)
    assert torch.equal(mask, g["sh_mask"])
    raw = g["raw"].reshape(-1, 7 + 3 * K)
    w = g["weights"]
    for chunk in (1 << 16, 13):                         # (chunking is invisible)
        o = adapter_ref.adapter_reference(raw, mask, 1e-8, w[0].reshape(-1, 3), w[1].reshape(-1, 4), w[2].reshape(-1, 3, K),
                                          dtype=torch.float32, chunk_rows=chunk)
        assert o["scales"].dtype == torch.float32
        want_s, want_r = g["scales"].reshape(-1, 3), g["rotations"].reshape(-1, 4)
        assert float(((o["scales"] - want_s).abs() / want_s.abs()).max()) <= 2 * ULP
        assert float(((o["rotations"] - want_r).abs().amax(1) / want_r.abs().amax(1)).max()) <= 1 * ULP
        assert torch.equal(o["harmonics"], g["harmonics"].reshape(-1, 3, K))
        gw = g["raw_grad"].reshape(-1, 7 + 3 * K)
        gs, ws = o["raw_grad"][:, :3], gw[:, :3]
        assert torch.equal(gs == 0, ws == 0) and bool((ws == 0).any())      # the clamped channels, and only those
        nz = ws != 0
        assert float(((gs - ws).abs()[nz] / ws.abs()[nz]).max()) <= 2 * ULP
        q_scale = w[1].reshape(-1, 4).abs().amax(1) / (raw[:, 3:7].norm(dim=1) + 1e-8)
        assert float(((o["raw_grad"][:, 3:7] - gw[:, 3:7]).abs().amax(1) / q_scale).max()) <= 2 * ULP
        assert torch.equal(o["raw_grad"][:, 7:], gw[:, 7:])


def test_oracle_float64_and_leading_shapes():
    """The float64 evaluation agrees with the float32 one to float32 rounding, `adapter_forward` keeps any leading
    shape, K = 0 is the geometric channels alone, and no upstream gradient means no raw_grad."""
    gen = torch.Generator().manual_seed(5)
    raw = torch.randn(2, 3, 11, 1, 1, 19, generator=gen)
    mask = adapter_ref.sh_mask(1)
    s, r, h = adapter_ref.adapter_forward(raw.double(), mask.double())
    assert s.shape == (2, 3, 11, 1, 1, 3) and r.shape == (2, 3, 11, 1, 1, 4) and h.shape == (2, 3, 11, 1, 1, 3, 4)
    o32 = adapter_ref.adapter_reference(raw.reshape(-1, 19), mask, dtype=torch.float32)
    assert o32["raw_grad"] is None
    assert float((o32["scales"].double() - s.reshape(-1, 3)).abs().max()) < 1e-9
    assert float((o32["rotations"].double() - r.reshape(-1, 4)).abs().max()) < 1e-6
    geo = adapter_ref.adapter_reference(raw.reshape(-1, 19)[:, :7], mask[:0], g_scales=torch.ones(66, 3))
    assert geo["harmonics"].shape == (66, 3, 0) and geo["raw_grad"].shape == (66, 7)
    assert torch.equal(geo["scales"], s.reshape(-1, 3)) and float(geo["raw_grad"][:, 3:].abs().max()) == 0.0
    with pytest.raises(ValueError):
        adapter_ref.adapter_forward(raw, adapter_ref.sh_mask(2))


def test_c_abi_rejects_bad_arguments(hip_lib):
    """spf_adapter_forward / spf_adapter_backward: SPF_E_INVALID with the reason in spf_last_error() for every argument
    the kernels could not survive; N = 0 is a successful no-op.  The pointers are made-up non-zero addresses: each
    rejection (and the N = 0 return) happens before any launch."""
    p, odd = C.c_void_p(4096), C.c_void_p(4096 + 4)
    fwd, bwd = hip_lib.spf_adapter_forward, hip_lib.spf_adapter_backward

    def f(**kw):
        a = dict(raw=p, raw_stride=82, N=16, K=25, sh_mask=p, eps=1e-8, scales=p, rotations=p, harmonics=p,
                 harmonics_high=None, stream=None)
        a.update(kw)
        return fwd(*a.values())

    def b(**kw):
        a = dict(raw=p, raw_stride=82, N=16, K=25, sh_mask=p, eps=1e-8, dL_dscales=p, dL_drotations=p, dL_dharmonics=p,
                 dL_dharmonics_high=None, split=0, dL_draw=p, stream=None)
        a.update(kw)
        return bwd(*a.values())

    def rejected(rc, msg, what):
        assert rc == -1, (what, rc)                                              # SPF_E_INVALID
        assert msg in hip_lib.spf_last_error(), (what, hip_lib.spf_last_error())

    for name in ("raw", "sh_mask", "scales", "rotations", "harmonics"):
        rejected(f(**{name: None}), b"null", name)
    for name in ("raw", "sh_mask", "dL_draw"):
        rejected(b(**{name: None}), b"null", name)
    for call in (f, b):
        rejected(call(N=-1), b"N must be >= 0", "N")
        rejected(call(K=0, raw_stride=7), b"K in 1..64", "K = 0")
        rejected(call(K=65, raw_stride=7 + 3 * 65), b"K in 1..64", "K = 65")
        rejected(call(raw_stride=81), b"raw_stride 81 is below the 82 channels", "stride")
        rejected(call(K=64, raw_stride=198), b"raw_stride 198 is below the 199 channels", "stride, K = 64")
        rejected(call(raw_stride=-82), b"raw_stride", "negative stride")
        rejected(call(raw_stride=0), b"raw_stride", "zero stride")
    rejected(f(K=16, raw_stride=55, harmonics_high=p), b"band-split", "high plane, K = 16")
    rejected(b(K=16, raw_stride=55, split=1), b"band-split", "split, K = 16")
    rejected(b(K=16, raw_stride=55, split=1, dL_dharmonics_high=p), b"band-split", "split + high, K = 16")
    rejected(b(dL_dharmonics_high=p), b"dL_dharmonics_high without split", "high without split")
    rejected(b(dL_drotations=odd), b"16-byte", "misaligned dL_drotations")
    rejected(b(dL_drotations=odd, split=1, dL_dharmonics_high=p), b"16-byte", "misaligned dL_drotations, split")
    # N = 0: nothing to do, whatever the (valid) layout -- and still after the checks
    assert f(N=0) == 0 and f(N=0, harmonics_high=p) == 0 and f(N=0, K=64, raw_stride=199) == 0
    assert b(N=0) == 0 and b(N=0, split=1, dL_dharmonics_high=p) == 0
    assert b(N=0, dL_dscales=None, dL_drotations=None, dL_dharmonics=None) == 0
    rejected(f(N=0, raw=None), b"null", "N = 0 does not excuse a null pointer")
    rejected(b(N=0, raw_stride=81), b"raw_stride", "N = 0 does not excuse a short stride")
