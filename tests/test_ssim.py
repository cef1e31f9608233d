"""SSIM and PSNR without a GPU: the float64 oracle (tests/ssim_oracle.py) pinned by vectors captured from the
reference's own ``ssim`` (tests/golden/make_ssim_goldens.py), the two restatements of ``compute_ssim`` against each
other, and the surface: argument errors before any launch, C-ABI validation, scratch sizing, no CPU fallback.
The kernels themselves are tested on the GPU (tests/test_gpu_ssim.py)."""
import ctypes as C
from pathlib import Path

import pytest
import torch

from tests import ssim_oracle as so

GOLD = torch.load(Path(__file__).parent / "golden" / "ssim_goldens.pt")


@pytest.mark.parametrize("case", sorted(GOLD))
def test_oracle_matches_reference_goldens(case):
    """Same expression, same dtype, only the operation order differs: value to 1e-12, gradients to 1e-10 of the
    plane's largest entry."""
    g = GOLD[case]
    x = g["X"].double().requires_grad_(True)
    y = g["Y"].double().requires_grad_(True)
    value = so.ssim_oracle(x, y, **g["kwargs"])
    assert value.shape == g["value"].shape
    assert so.value_error(value, g["value"]) <= 1e-12
    gx, gy = torch.autograd.grad(value, [x, y], g["upstream"])
    for got, want in ((gx, g["grad_X"]), (gy, g["grad_Y"])):
        plane, _ = so.grad_errors(got, want)
        assert plane <= 1e-10, (case, plane)


def test_goldens_cover_the_cases():
    kw = [g["kwargs"] for g in GOLD.values()]
    assert {g["X"].shape[1] for g in GOLD.values()} == {1, 3, 4}
    assert {k["data_range"] for k in kw} == {1.0, 255}
    assert any(k.get("win_size") == 7 for k in kw) and any("win" in k for k in kw)
    assert any(k.get("nonnegative_ssim") for k in kw)
    assert {k.get("size_average", True) for k in kw} == {True, False}
    assert {tuple(g["X"].shape) for g in GOLD.values()} >= {(2, 3, 37, 53), (1, 3, 11, 11), (1, 3, 11, 300)}
    for g in GOLD.values():
        assert g["X"].dtype == torch.float32 and g["grad_X"].dtype == torch.float64 and not g["X"].requires_grad


def test_compute_ssim_restatements_agree():
    """The valid convolution with cov_norm = 121/120 IS scikit-image's reflect-filter-and-crop definition: 1e-12 with a
    float64 window on both sides, 1e-6 with the reference's float32-built window (the difference is the window's)."""
    pytest.importorskip("scipy")
    for kind in ("noise", "smooth", "piecewise"):
        gt, hat = so.KINDS[kind](5, (2, 3, 64, 80))
        want = so.skimage_ssim(gt, hat)
        got64 = so.compute_ssim_oracle(gt, hat, window_dtype=torch.float64)
        got32 = so.compute_ssim_oracle(gt, hat)
        assert float((got64 - want).abs().max()) <= 1e-12, kind
        assert float((got32 - want).abs().max()) <= 1e-6, kind
        plain = so.ssim_oracle(gt, hat, data_range=1.0, size_average=False)       # cov_norm = 1 is another number
        if kind != "piecewise":
            assert float((plain - want).abs().max()) > 1e-5, kind


def test_psnr_oracle():
    gt = torch.tensor([[[[0.0, 0.5], [1.5, -1.0]]]])
    hat = torch.tensor([[[[0.1, 0.5], [1.0, 0.0]]]])
    assert float(so.psnr_oracle(gt, hat)) == pytest.approx(-10 * torch.log10(torch.tensor(0.01 / 4, dtype=torch.float64)))
    assert float(so.psnr_oracle(gt, gt)) == float("inf")


def test_window_is_the_reference_window():
    from spfsplatv2_amd.ssim import SSIM, gauss_window
    w = gauss_window(11, 1.5)
    assert w.dtype == torch.float32 and torch.equal(w, so.gauss_window(11, 1.5))
    m = SSIM(data_range=1.0, channel=4, win_size=7)
    assert m.win.shape == (4, 1, 1, 7) and torch.equal(m.win[2, 0, 0], so.gauss_window(7, 1.5))
    # the module's window is the one captured with the goldens' float64 values: same weights -> same numbers
    g = GOLD["win7_smooth"]
    v = so.ssim_oracle(g["X"], g["Y"], data_range=1.0, win=m.win)
    assert so.value_error(v, g["value"]) <= 1e-12


def test_argument_errors_before_any_launch():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd.ssim import SSIM, ssim
    assert spf.ssim is ssim and spf.SSIM is SSIM
    x = torch.rand(2, 3, 16, 16)
    with pytest.raises(ValueError, match="same dimensions"):
        ssim(x, torch.rand(2, 3, 16, 17))
    with pytest.raises(ValueError, match="4-d or 5-d"):
        ssim(x[0], x[0])
    with pytest.raises(ValueError, match="4-d or 5-d"):                       # trailing singletons are squeezed first
        ssim(x[0, :, :, :, None], x[0, :, :, :, None])
    with pytest.raises(NotImplementedError, match="5-d"):
        ssim(x[None], x[None])
    with pytest.raises(ValueError, match="Window size should be odd"):
        ssim(x, x, win_size=8)
    with pytest.raises(ValueError, match="Window size should be odd"):        # win given: its length is the size
        ssim(x, x, win_size=11, win=torch.ones(3, 1, 1, 4) / 4)
    with pytest.raises(ValueError, match="different rows"):
        ssim(x, x, win=torch.rand(3, 1, 1, 5))
    with pytest.raises(ValueError, match="outside 3..33"):
        ssim(torch.rand(1, 1, 40, 40), torch.rand(1, 1, 40, 40), win_size=35)
    with pytest.raises(ValueError, match="shorter than the window"):
        ssim(x[:, :, :10], x[:, :, :10])
    with pytest.raises(NotImplementedError, match="retrun_seprate"):
        ssim(x, x, retrun_seprate=True)
    with pytest.raises(RuntimeError, match="floating-point"):
        ssim((x * 255).to(torch.uint8), (x * 255).to(torch.uint8))
    with pytest.raises(NotImplementedError, match="spatial_dims"):
        SSIM(spatial_dims=3)
    with pytest.raises(ValueError, match="differ in shape"):
        spf.compute_ssim(x, x[:1])
    with pytest.raises(ValueError, match="batch, channel, height, width"):
        spf.compute_psnr(x[0], x[0])
    with pytest.raises(ValueError, match="shorter than the window"):
        spf.compute_ssim(x[:, :, :10], x[:, :, :10])


def test_product_refuses_cpu_tensors(hip_lib):
    import spfsplatv2_amd as spf
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.ssim(x, x, data_range=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.SSIM(data_range=1.0)(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.compute_ssim(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.compute_psnr(x, x)


def _args(N=1, Cn=3, H=16, W=16, ws=11, X=16, Y=16):
    from spfsplatv2_amd import _lib
    return _lib.SpfSsim(C.c_void_p(X), C.c_void_p(Y), N, Cn, H, W, ws, 1e-4, 9e-4, 1.0, 1, 0)


def test_c_abi_argument_validation(hip_lib):
    """Rejected with SPF_E_INVALID and a message before anything touches a device (the pointers are never read)."""
    from spfsplatv2_amd import _lib
    assert C.sizeof(_lib.SpfSsim) == 16 + 10 * 4 + 33 * 4 + 4             # two pointers, ten words, the window, padding
    p = C.c_void_p(16)
    fwd, bwd, psnr, err = hip_lib.spf_ssim_forward, hip_lib.spf_ssim_backward, hip_lib.spf_psnr_forward, hip_lib.spf_last_error
    for bad, msg in ((_args(ws=10), b"odd"), (_args(ws=1), b"3..33"), (_args(ws=35, H=64, W=64), b"3..33"),
                     (_args(H=10), b"shorter"), (_args(W=10), b"shorter"), (_args(N=0), b"positive"),
                     (_args(Cn=-1), b"positive"), (_args(X=None), b"null"), (_args(Y=None), b"null"),
                     (_args(X=18), b"aligned")):
        assert fwd(C.byref(bad), p, p, p, None) == -1 and msg in err(), msg
        assert bwd(C.byref(bad), p, p, p, p, None) == -1 and msg in err(), msg
    assert fwd(None, p, p, p, None) == -1 and b"null" in err()
    for hole in range(3):
        ptrs = [p, p, p]
        ptrs[hole] = None
        assert fwd(C.byref(_args()), *ptrs, None) == -1 and b"null" in err()
    assert bwd(C.byref(_args()), None, p, p, p, None) == -1 and b"null" in err()
    assert bwd(C.byref(_args()), p, None, p, p, None) == -1 and b"null" in err()
    assert bwd(C.byref(_args()), p, p, None, None, None) == -1 and b"no gradient" in err()
    assert psnr(None, p, 1, 10, p, None) == -1 and b"null" in err()
    assert psnr(p, p, 1, 10, None, None) == -1 and b"null" in err()
    assert psnr(p, p, 0, 10, p, None) == -1 and b"positive" in err()
    assert psnr(p, p, 1, 0, p, None) == -1 and b"positive" in err()


def test_partial_blocks(hip_lib):
    """One slot per (32 x 32 tile of the valid region, plane); 32 x 16 tiles once the window is so long that a 32 x 32
    tile and its row moments pass 64 KiB of LDS (ws >= 29); -1 for what the forward rejects."""
    n = hip_lib.spf_ssim_partial_blocks
    assert n(32, 3, 256, 256, 11) == 96 * 8 * 8             # 246 x 246 valid
    assert n(1, 1, 11, 11, 11) == 1 and n(1, 3, 11, 300, 11) == 3 * 10
    assert n(2, 3, 37, 53, 11) == 6 * 1 * 2 and n(2, 3, 43, 43, 11) == 6 * 2 * 2
    assert n(1, 1, 4080, 4080, 11) == 128 * 128
    assert n(1, 1, 64, 64, 27) == 2 * 2 and n(1, 1, 64, 64, 29) == 2 * 3 and n(1, 1, 64, 64, 33) == 1 * 2
    for bad in ((0, 3, 16, 16, 11), (1, 3, 16, 16, 10), (1, 3, 10, 16, 11), (1, 3, 16, 10, 11), (1, 3, 64, 64, 35),
                (1, 3, 16, 16, 1)):
        assert n(*bad) == -1, bad
