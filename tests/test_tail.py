"""The encoder tail without a device: exports, refusals, the library's host-side argument checks, the oracle against the
reference's goldens, the stable opacity form against the reference's expression, and the power condition of the gates
with float32 eager on the CPU standing in for the device (tests/tail_cases.py states the gate; tests/test_gpu_tail.py
applies it to the kernels)."""
import ctypes as C
import types

import pytest
import torch

from tests import tail_cases as cases
from tests import tail_oracle as to

NAMES = ("GaussianTail", "gaussians_from_heads", "density_to_opacity", "map_pdf_to_opacity")
SYMBOLS = ("spf_tail_max_grid", "spf_tail_forward", "spf_tail_backward", "spf_opacity_forward", "spf_opacity_backward")
ULP = cases.ULP
# the loop case of tests/test_gpu_tail.py at the cap this library reports; asserted below
LOOP_CAP = 4096


def test_exports(hip_lib):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import _lib, build, tail
    for name in NAMES:
        assert name in spf.__all__ and getattr(spf, name) is getattr(tail, name), name
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(hip_lib, name), name
    assert "tail.hip" in build.SOURCES and hip_lib.spf_abi_version() == 7
    assert tail.max_grid() == LOOP_CAP
    assert C.sizeof(_lib.SpfTail) == 2 * 32 * 8 + 8 + 8 + 6 * 4 and C.sizeof(_lib.SpfTailGrads) == 2 * 32 * 8


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["deg0_e0", "deg0_e1.5", "deg4_e0", "deg4_e1.5"])
def test_float64_oracle_reproduces_the_reference_goldens(golden_dir, key):
    """Adapter tensors: the tolerances of tests/test_adapter_oracle.py (2 ulp on the scales and their gradient, 1 ulp of
    the row on the rotations, 2 ulp of |g| / (|q| + eps) on their gradient, the harmonics and the means bit for bit).
    Density channel (not covered there; derived, not measured): the reference's float32 chain is a sigmoid, a
    subtraction, two pows (2 ulp each in libm), two additions and a product, every term at most 1 -- 4 ulp of 1 on the
    opacities; its backward repeats them with two more products per branch -- 8 ulp of the largest gradient.  (The
    goldens' exponents are >= 1: the rounding of 1 - p then enters damped by (1 - p)^(e - 1) <= 1.)"""
    g = cases.golden(golden_dir)[key]
    K = (g["sh_degree"] + 1) ** 2
    assert torch.equal(to.sh_mask(g["sh_degree"]), g["sh_mask"])
    o = to.tail_with_grads(g["pts"], g["raw"], g["ups"], g["exponent"], g["sh_degree"])
    want = g["out"]
    assert tuple(want["harmonics"].shape) == (2, 2 * 15, 3, K)
    assert torch.equal(o["means"].float(), want["means"]) and torch.equal(o["harmonics"].float(), want["harmonics"])
    assert float(((o["scales"] - want["scales"]).abs() / want["scales"].abs()).max()) <= 2 * ULP
    assert float(((o["rotations"] - want["rotations"]).abs().amax(-1) / want["rotations"].abs().amax(-1)).max()) <= 1 * ULP
    assert float((o["opacities"] - want["opacities"]).abs().max()) <= 4 * ULP
    assert torch.equal(o["d_pts"].float(), g["d_pts"])
    got, ref = o["d_raw"], g["d_raw"]                                   # [v, b, C, h, w]
    assert float((got[:, :, 0] - ref[:, :, 0]).abs().max()) <= 8 * ULP * float(got[:, :, 0].abs().max())
    gs, ws = got[:, :, 1:4], ref[:, :, 1:4]
    assert torch.equal(gs == 0, ws == 0) and bool((ws == 0).any())      # the clamped channels, and only those
    nz = ws != 0
    assert float(((gs - ws).abs()[nz] / ws.abs()[nz]).max()) <= 2 * ULP
    raw = torch.stack(g["raw"]).double()
    ups_rot = g["ups"]["rotations"].reshape(2, 2, 3, 5, 4).permute(1, 0, 4, 2, 3)          # -> [v, b, 4, h, w]
    q_scale = ups_rot.abs().amax(2) / (raw[:, :, 4:8].norm(dim=2) + 1e-8)
    assert float(((got[:, :, 4:8] - ref[:, :, 4:8]).abs().amax(2) / q_scale).max()) <= 2 * ULP
    assert torch.equal(got[:, :, 8:].float(), ref[:, :, 8:])


@pytest.mark.parametrize("e", [2.0 ** -1.5, 0.5, 1.0, 2.0, 2.0 ** 1.5])
def test_stable_opacity_form_is_the_reference_s_expression(e):
    """float64, logits in [-12, 12]: exp(e logsigmoid(-x)) against (1 - sigmoid(x))^e and the like.  Bound: the stable
    form is accurate to a few ulp; the reference's expression rounds p = sigmoid(x) to half an ulp of 1 (1.1e-16) before
    it forms 1 - p >= 6.1e-6, a relative error of at most 1.8e-11 there, which (1 - p)^e carries as e (1 - p)^(e - 1)
    1.1e-16 <= 0.354 (6.1e-6)^-0.646 1.1e-16 = 9.3e-14 at the smallest exponent: 1e-13 of the map's scale, 1."""
    x = torch.linspace(-12.0, 12.0, 48001, dtype=torch.float64)
    diff = float((to.opacity_stable(x, e) - to.opacity_naive(x, e)).abs().max())
    print(f"stable - naive, e = {e:.4g}: {diff:.3e}")
    assert diff <= 1e-13


def test_product_map_pdf_to_opacity_is_the_reference_s(hip_lib):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import tail
    cfg = types.SimpleNamespace(initial=0.0, final=1.5, warm_up=100)
    assert tail.opacity_exponent(0, cfg) == 1.0 and tail.opacity_exponent(50, cfg) == 2.0 ** 0.75
    assert tail.opacity_exponent(100, cfg) == tail.opacity_exponent(10 ** 6, cfg) == 2.0 ** 1.5
    assert tail.opacity_exponent(50, dict(initial=0.0, final=1.5, warm_up=100)) == 2.0 ** 0.75
    x = torch.linspace(-12.0, 12.0, 4801, dtype=torch.float64)
    assert torch.equal(spf.map_pdf_to_opacity(x.sigmoid(), 50, cfg), to.opacity_naive(x, 2.0 ** 0.75))


def test_device_mask_is_made_once_per_degree_and_device(hip_lib):
    """``gaussians_from_heads`` takes its SH mask from a cache keyed by (sh_degree, device), so only the first call for a
    key copies anything from the host (tests/test_gpu_tail.py pins that a later call never waits for the stream)."""
    from spfsplatv2_amd import tail
    for deg in range(5):
        m = tail._device_mask(deg, "cpu")
        assert m is tail._device_mask(deg, torch.device("cpu")) and torch.equal(m, to.sh_mask(deg))
    assert tail._device_mask(1, "cpu") is not tail._device_mask(2, "cpu")


# ---- the power condition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.covering_cases() + list(cases.SPLIT_CASES), ids=cases.case_id)
def test_every_mutant_is_four_bounds_away(case):
    d, x64, dists = cases.reference(case)
    eager = cases.oracle(case, d, torch.float32)
    e_eager = {k: to.rel_err(eager[k], x64[k]) for k in x64}
    for k, v in e_eager.items():
        print(f"{cases.case_id(case)} {k}: eager {v:.3e}")
    bad = cases.power_failures(cases.case_id(case), dists, e_eager)
    assert not bad, "\n".join(bad)
    assert set(dists) == set(cases.mutants(case, bool(d["tiny"].any())))
    for m, dd in dists.items():
        assert dd, m                                                    # every mutant asked of a case reaches something


def test_eager_float32_is_finite_at_the_pinned_logits_and_nan_at_saturated_ones():
    """What the issue says of the reference's expression under float32 autograd, on the CPU: finite at -12, 0 and 12 for
    every exponent of the tests; NaN gradients for x >= 17 with an exponent below 1 and x <= -104 with one above."""
    for e in cases.EXPONENTS:
        x = torch.tensor([-12.0, 0.0, 12.0], requires_grad=True)
        (g,) = torch.autograd.grad(to.opacity_naive(x, e).sum(), x)
        assert torch.isfinite(g).all(), e
    for e, sat in ((0.5, 17.0), (2.0, -104.0)):
        x = torch.tensor([sat], requires_grad=True)
        (g,) = torch.autograd.grad(to.opacity_naive(x, e).sum(), x)
        assert torch.isnan(g).all(), (e, sat)
        x = torch.tensor([sat], requires_grad=True)
        (g,) = torch.autograd.grad(to.opacity_stable(x, e).sum(), x)
        assert torch.isfinite(g).all(), (e, sat)


# ---- refusals --------------------------------------------------------------------------------------------------------
def _heads(v=2, b=2, c=11, h=3, w=5, dtype=torch.float32):
    return [torch.zeros(b, h, w, 3, dtype=dtype) for _ in range(v)], [torch.zeros(b, c, h, w, dtype=dtype) for _ in range(v)]


def test_argument_validation(hip_lib):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import adapter
    pts, raw = _heads()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.gaussians_from_heads(pts, raw, sh_degree=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.density_to_opacity(torch.zeros(4, 83)[:, 0])
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError):
            spf.gaussians_from_heads(*_heads(dtype=dt), sh_degree=0)
        with pytest.raises(NotImplementedError):
            spf.density_to_opacity(torch.zeros(4, dtype=dt))
    with pytest.raises(ValueError, match="point maps"):
        spf.gaussians_from_heads(pts[:1], raw, sh_degree=0)
    with pytest.raises(ValueError, match="number of views"):
        spf.gaussians_from_heads([], [], sh_degree=0)
    with pytest.raises(RuntimeError, match="channels"):
        spf.gaussians_from_heads(pts, raw, sh_degree=1)                   # 11 channels are sh_degree 0
    with pytest.raises(ValueError, match="unequal shape"):
        spf.gaussians_from_heads(pts, [raw[0], torch.zeros(2, 11, 3, 6)], sh_degree=0)
    with pytest.raises(ValueError, match="pts3d"):
        spf.gaussians_from_heads([pts[0], torch.zeros(2, 3, 5, 2)], raw, sh_degree=0)
    with pytest.raises(NotImplementedError, match="sh_degree"):
        spf.gaussians_from_heads(*_heads(c=8 + 3 * 36), sh_degree=5)      # K = 36: no template instance, refused
    with pytest.raises(ValueError, match="split_harmonics"):
        spf.gaussians_from_heads(pts, raw, sh_degree=0, split_harmonics=True)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="exponent"):
            spf.gaussians_from_heads(pts, raw, bad, sh_degree=0)
        with pytest.raises(ValueError, match="exponent"):
            spf.density_to_opacity(torch.zeros(4), bad)
    mapping = types.SimpleNamespace(initial=0.0, final=0.0, warm_up=1)
    cfg = adapter.GaussianAdapterCfg(0.5, 15.0, 4)
    with pytest.raises(NotImplementedError, match="num_surfaces"):
        spf.GaussianTail(cfg, mapping, num_surfaces=2)
    with pytest.raises(ValueError, match="split_harmonics"):
        spf.GaussianTail(adapter.GaussianAdapterCfg(0.5, 15.0, 2), mapping, split_harmonics=True)
    tail = spf.GaussianTail(cfg, mapping, split_harmonics=True)
    assert not list(tail.parameters()) and not list(tail.buffers()) and tail.d_sh == 25 and tail.d_in == 82
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tail(*_heads(c=83), global_step=3)


def test_c_abi_rejects_bad_arguments(hip_lib):
    """SPF_E_INVALID with the reason in spf_last_error() before any launch: the pointers are made-up addresses."""
    from spfsplatv2_amd import _lib
    p, odd = 4096, 4096 + 4
    err = hip_lib.spf_last_error

    def args(**kw):
        a = _lib.SpfTail()
        a.b, a.v, a.hw, a.K, a.exponent, a.eps, a.sh_mask = 2, 2, 15, 25, 1.0, 1e-8, p
        for i in range(2):
            a.raw[i], a.pts[i] = p, p
        for k, val in kw.items():
            if k in ("raw", "pts"):
                getattr(a, k)[1] = val
            else:
                setattr(a, k, val)
        return a

    def fwd(a, high=None):
        return hip_lib.spf_tail_forward(C.byref(a), p, p, p, p, p, high, None)

    def bwd(a, split=0, high=None, rot=p, grads=True, d_raw1=p):
        g = _lib.SpfTailGrads()
        for i in range(2):
            g.d_raw[i], g.d_pts[i] = p, p
        g.d_raw[1] = d_raw1
        return hip_lib.spf_tail_backward(C.byref(a), p, p, p, rot, p, high, split, C.byref(g) if grads else None, None)

    for call in (fwd, bwd):
        for kw, msg in ((dict(b=0), b"positive"), (dict(hw=0), b"positive"), (dict(v=0), b"v in 1..32"), (dict(v=33), b"v in 1..32"),
                        (dict(K=2), b"one of 1, 4, 9, 16, 25"), (dict(K=36), b"one of 1, 4, 9, 16, 25"),
                        (dict(exponent=0.0), b"exponent"), (dict(exponent=float("nan")), b"exponent"),
                        (dict(sh_mask=None), b"null"), (dict(raw=None), b"null"), (dict(raw=odd), b"16-byte"),
                        (dict(hw=2 ** 31 // 83), b"2^31")):
            assert call(args(**kw)) == -1 and msg in err(), (call.__name__, kw, err())
    assert fwd(args(pts=None)) == -1 and b"null" in err()
    assert hip_lib.spf_tail_forward(C.byref(args()), p, None, p, p, p, None, None) == -1 and b"null output" in err()
    assert hip_lib.spf_tail_forward(C.byref(args()), p, p, p, odd, p, None, None) == -1 and b"16-byte" in err()
    assert hip_lib.spf_tail_forward(None, p, p, p, p, p, None, None) == -1 and b"args is null" in err()
    assert fwd(args(K=16), high=p) == -1 and b"band-split" in err()
    assert bwd(args(K=16), split=1) == -1 and b"band-split" in err()
    assert bwd(args(), high=p) == -1 and b"without split" in err()
    assert bwd(args(), rot=odd) == -1 and b"16-byte" in err()
    assert bwd(args(), grads=False) == -1 and b"grads is null" in err()
    assert bwd(args(), d_raw1=None) == -1 and b"null" in err()
    of, ob = hip_lib.spf_opacity_forward, hip_lib.spf_opacity_backward
    assert of(None, 1, 4, 1.0, p, None) == -1 and b"null" in err()
    assert of(p, 0, 4, 1.0, p, None) == -1 and b"stride >= 1" in err()
    assert of(p, 1, -1, 1.0, p, None) == -1 and b"n must be >= 0" in err()
    assert of(p, 1, 4, -2.0, p, None) == -1 and b"exponent" in err()
    assert of(p, 1, 4, 1.0, None, None) == -1 and b"null" in err()
    assert of(p + 2, 1, 4, 1.0, p, None) == -1 and b"4-byte" in err()
    assert ob(p, 83, 4, 1.0, None, p, None) == -1 and b"null" in err()
    assert ob(p, 83, 4, 1.0, p, p + 1, None) == -1 and b"4-byte" in err()
    assert of(p, 83, 0, 1.0, p, None) == 0 and ob(p, 83, 0, 1.0, p, p, None) == 0      # n = 0: nothing to do
