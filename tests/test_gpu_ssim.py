"""SSIM and PSNR kernels (spfsplatv2_amd/csrc/ssim.hip) on the GPU.

Truth is tests/ssim_oracle.py in float64 on the host.  The yardstick for float32 is THE SAME ORACLE EVALUATED IN FLOAT32
on the host on the same inputs (for the golden cases: the reference's own float32 run, recorded with the goldens) -- what
the reference's eager expression itself loses in float32 -- never the product:

* value:                   |product - f64| <= 4 |oracle_f32 - f64| + 5e-7, never looser than 5e-4
* gradients, per plane:    max|g - w| / max|w| <= 4 (the same for oracle_f32) + 1e-6, never looser than 1e-3
* gradients, per element   (entries within two orders of their plane's largest): |g - w| / |w| <= 4 (oracle_f32's worst
                           such ratio) + 1e-5, never looser than 1e-2

4 x: the product sums the same products in another order (fused multiply-adds, fixed-order block sums), a different
draw from the same cancellation, not another order of magnitude.  Every (case, product error, yardstick error) triple is
appended to profiles/ssim_parity.jsonl (SPF_SSIM_PARITY_LOG names another file)."""
import json
import os
from pathlib import Path

import pytest
import torch

from tests import ssim_oracle as so
from tests import util

pytestmark = pytest.mark.gpu

GOLD = torch.load(Path(__file__).parent / "golden" / "ssim_goldens.pt")
LOG = Path(os.environ.get("SPF_SSIM_PARITY_LOG", Path(__file__).resolve().parents[1] / "profiles" / "ssim_parity.jsonl"))


def _log(case, product, yardstick):
    try:
        with open(LOG, "a") as f:
            f.write(json.dumps({"case": case, "product": product, "yardstick": yardstick}) + "\n")
    except OSError:                       # a read-only tree: the assertions below still hold
        pass


def _upstream(n, size_average):
    return None if size_average else torch.linspace(0.5, 1.5, n, dtype=torch.float64)


def _oracle(X, Y, kwargs, dtype):
    x, y = X.clone().to(dtype).requires_grad_(True), Y.clone().to(dtype).requires_grad_(True)
    v = so.ssim_oracle(x, y, dtype=dtype, **kwargs)
    up = _upstream(X.shape[0], kwargs.get("size_average", True))
    gx, gy = torch.autograd.grad(v, [x, y], None if up is None else up.to(dtype))
    return v.detach(), gx, gy


def _product(X, Y, kwargs, fn=None):
    import spfsplatv2_amd as spf
    x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
    out = (fn or spf.ssim)(x, y, **{k: v for k, v in kwargs.items() if k != "cov_norm"})
    assert len(out) == 4 and all(o.shape == out[0].shape and not bool(o.any()) for o in out[1:])
    v = out[0]
    up = _upstream(X.shape[0], kwargs.get("size_average", True))
    gx, gy = torch.autograd.grad(v, [x, y], None if up is None else up.to(v))
    return v.detach().cpu(), gx.cpu(), gy.cpu()


def _errors(got, truth):
    ex, ey = so.grad_errors(got[1], truth[1]), so.grad_errors(got[2], truth[2])
    return {"value": so.value_error(got[0], truth[0]), "plane": max(ex[0], ey[0]), "element": max(ex[1], ey[1])}


def _assert_rule(case, product, yardstick):
    print(case, "product", product, "yardstick", yardstick)
    _log(case, product, yardstick)
    assert product["value"] <= min(4 * yardstick["value"] + 5e-7, 5e-4), (case, "value", product, yardstick)
    if "plane" in product:
        assert product["plane"] <= min(4 * yardstick["plane"] + 1e-6, 1e-3), (case, "plane", product, yardstick)
        assert product["element"] <= min(4 * yardstick["element"] + 1e-5, 1e-2), (case, "element", product, yardstick)


def _against_oracle(case, X, Y, kwargs, product=None):
    """X, Y: float32 host tensors.  The product on the device against the float64 oracle, yardstick: the float32 one."""
    truth = _oracle(X, Y, kwargs, torch.float64)
    yard = _errors(_oracle(X, Y, kwargs, torch.float32), truth)
    got = product or _product(X.cuda(), Y.cuda(), kwargs)
    assert got[0].dtype == torch.float32 and got[0].shape == truth[0].shape
    _assert_rule(case, _errors(got, truth), yard)
    return got


# ---- 1. the reference's own vectors -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(GOLD))
def test_goldens(hip_lib, case):
    g = GOLD[case]
    kw = dict(g["kwargs"])
    if "win" in kw:
        kw["win"] = kw["win"].reshape(1, 1, 1, -1).repeat(g["X"].shape[1], 1, 1, 1)
    got = _product(g["X"].cuda(), g["Y"].cuda(), kw)
    _assert_rule("golden/" + case, _errors(got, (g["value"], g["grad_X"], g["grad_Y"])), g["f32_error"])


def test_module_matches_function(hip_lib):
    import spfsplatv2_amd as spf
    g = GOLD["win7_smooth"]
    m = spf.SSIM(data_range=1.0, win_size=7, channel=3)
    a = _product(g["X"].cuda(), g["Y"].cuda(), {}, fn=lambda x, y: m(x, y))
    b = _product(g["X"].cuda(), g["Y"].cuda(), g["kwargs"])
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ---- 2. production sizes -------------------------------------------------------------------------------------------
SHAPES = {"headline_8x4": (32, 3, 256, 256), "re10k_10view": (30, 3, 256, 256), "test_step": (3, 3, 256, 256),
          "512": (16, 3, 512, 512)}


@pytest.mark.parametrize("kind", sorted(so.KINDS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_production_sizes(hip_lib, shape, kind):
    X, Y = so.KINDS[kind](11, SHAPES[shape])
    for size_average in (True, False):
        _against_oracle(f"{shape}/{kind}/size_average={size_average}", X, Y,
                        dict(data_range=1.0, size_average=size_average))


# ---- 3. edges ------------------------------------------------------------------------------------------------------
def test_one_output_and_one_row(hip_lib):
    for shape in ((1, 1, 11, 11), (1, 3, 11, 300), (1, 3, 300, 11)):
        for kind in ("noise", "smooth"):
            X, Y = so.KINDS[kind](3, shape)
            _against_oracle(f"edge/{shape}/{kind}", X, Y, dict(data_range=1.0, size_average=False))


def test_slice_of_a_larger_tensor(hip_lib):
    """(2,3,37,53) cut out of (2,3,40,57) from element (1, 3) on: not contiguous, rows not 16-byte aligned."""
    bx, by = so.smooth(4, (2, 3, 40, 57))
    X, Y = bx[:, :, 1:38, 3:56], by[:, :, 1:38, 3:56]
    dx, dy = bx.cuda()[:, :, 1:38, 3:56], by.cuda()[:, :, 1:38, 3:56]
    assert not dx.is_contiguous()
    kw = dict(data_range=1.0, size_average=False)
    got = _against_oracle("edge/slice_37x53", X.contiguous(), Y.contiguous(), kw, product=_product(dx, dy, kw))
    # an odd plane size: every second plane starts off a 16-byte boundary
    same = _product(X.contiguous().cuda(), Y.contiguous().cuda(), kw)
    assert all(torch.equal(p, q) for p, q in zip(got, same))


def test_bf16_inputs(hip_lib):
    """bf16 -> float32 is exact: the value obeys the rule on the upcast inputs, float32 result; the gradients are the
    float32-input gradients (which obey the rule) rounded to bf16 by autograd."""
    import spfsplatv2_amd as spf
    X, Y = (t.bfloat16() for t in so.smooth(6, (2, 3, 37, 53)))
    kw = dict(data_range=1.0, size_average=False)
    f32 = _against_oracle("edge/bf16_upcast", X.float(), Y.float(), kw)
    x, y = X.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
    v = spf.ssim(x, y, **kw)[0]
    v.backward(_upstream(2, False).to(v))
    assert v.dtype == torch.float32 and torch.equal(v.detach().cpu(), f32[0])
    assert x.grad.dtype == torch.bfloat16 and torch.equal(x.grad.cpu(), f32[1].bfloat16())
    assert torch.equal(y.grad.cpu(), f32[2].bfloat16())


def test_four_channels_and_more_planes_than_blocks(hip_lib):
    X, Y = so.smooth(7, (2, 4, 37, 53))
    _against_oracle("edge/c4", X, Y, dict(data_range=1.0))
    # 2,100 one-tile planes on a grid of at most 2,048 blocks: blocks loop over several slots
    X, Y = so.noise(8, (700, 3, 13, 14))
    _against_oracle("edge/2100_planes", X, Y, dict(data_range=1.0, size_average=False))
    # several tiles per plane and more slots than blocks, forward and backward
    X, Y = so.smooth(9, (40, 3, 96, 96))
    _against_oracle("edge/40x3x96x96", X, Y, dict(data_range=1.0, nonnegative_ssim=True))


def test_long_windows(hip_lib):
    """ws = 19: the generic kernels on smaller backward tiles; ws = 33: the longest window, 32 x 16 forward tiles and a
    backward tile that needs more than the default 64 KiB of LDS."""
    X, Y = so.smooth(10, (1, 2, 70, 90))
    for ws in (5, 19, 33):
        _against_oracle(f"edge/win{ws}", X, Y, dict(data_range=1.0, win_size=ws, win_sigma=ws / 7.0))


def test_only_one_side_needs_a_gradient(hip_lib):
    """dL/dX alone and dL/dY alone come from kernels of their own (three derivative maps instead of four): the same
    rule (the compiler contracts their expressions differently, so they need not equal the two-sided call bitwise)."""
    import spfsplatv2_amd as spf
    hx, hy = so.smooth(12, (2, 3, 37, 53))
    X, Y = hx.cuda(), hy.cuda()
    x = X.clone().requires_grad_(True)
    vx = spf.ssim(x, Y, data_range=1.0)[0]
    vx.backward()
    y = Y.clone().requires_grad_(True)
    vy = spf.ssim(X, y, data_range=1.0)[0]
    vy.backward()
    assert torch.equal(vx, vy)
    _against_oracle("edge/one_sided", hx, hy, dict(data_range=1.0), product=(vx.detach().cpu(), x.grad.cpu(), y.grad.cpu()))


# ---- 4. the metrics --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 256, 256), (2, 3, 37, 53)], ids=str)
def test_compute_ssim_and_psnr(hip_lib, shape):
    import spfsplatv2_amd as spf
    for kind in sorted(so.KINDS):
        gt, hat = so.KINDS[kind](13, shape)
        hat = hat * 1.2 - 0.1                                            # some values outside [0, 1]: PSNR clips them
        truth = so.compute_ssim_oracle(gt, hat)
        yard = so.value_error(so.compute_ssim_oracle(gt, hat, dtype=torch.float32), truth)
        got = spf.compute_ssim(gt.cuda(), hat.cuda())
        assert got.shape == (shape[0],) and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
        _assert_rule(f"compute_ssim/{shape}/{kind}", {"value": so.value_error(got, truth)}, {"value": yard})
        try:
            sk = so.skimage_ssim(gt, hat)
        except ImportError:                                              # no scipy on this machine
            sk = None
        if sk is not None:                    # the independent restatement: 1e-6 from the oracle (the window's dtype)
            assert float((got.double().cpu() - sk).abs().max()) <= 1e-6 + min(4 * yard + 5e-7, 5e-4)
        psnr = spf.compute_psnr(gt.cuda(), hat.cuda())
        want = so.psnr_oracle(gt, hat)
        assert psnr.shape == (shape[0],) and psnr.dtype == torch.float32
        print("psnr", shape, kind, float((psnr.double().cpu() - want).abs().max()))
        assert float((psnr.double().cpu() - want).abs().max()) <= 5e-5
    gt = so.noise(14, shape)[0].cuda()
    assert bool(torch.isinf(spf.compute_psnr(gt, gt)).all()) and bool((spf.compute_psnr(gt, gt) > 0).all())
    assert bool(torch.isinf(spf.compute_psnr(gt + 2, gt + 3)).all())    # both clip to 1
    half = spf.compute_ssim(gt.half(), gt.half())
    assert half.dtype == torch.float16 and bool((half == 1).all())
    assert spf.compute_psnr(gt.bfloat16(), gt.bfloat16() * 0.5).dtype == torch.bfloat16


# ---- 5. bit-reproducible, and a plane's sums do not depend on its neighbours ---------------------------------------
def test_bitwise_reproducible_and_batch_independent(hip_lib):
    import spfsplatv2_amd as spf
    X, Y = (t.cuda() for t in so.smooth(15, (5, 3, 70, 83)))
    kw = dict(data_range=1.0, size_average=False)
    a, b = _product(X, Y, kw), _product(X, Y, kw)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    s1, s2 = _product(X, Y, dict(data_range=1.0)), _product(X, Y, dict(data_range=1.0))
    assert all(torch.equal(p, q) for p, q in zip(s1, s2))
    up = _upstream(5, False)
    for i in range(5):
        x, y = X[i:i + 1].clone().requires_grad_(True), Y[i:i + 1].clone().requires_grad_(True)
        v = spf.ssim(x, y, **kw)[0]
        v.backward(up[i:i + 1].to(v))
        assert torch.equal(v.detach().cpu(), a[0][i:i + 1]), i
        assert torch.equal(x.grad.cpu(), a[1][i:i + 1]) and torch.equal(y.grad.cpu(), a[2][i:i + 1]), i


# ---- 6. no host synchronisation ------------------------------------------------------------------------------------
def test_forward_backward_and_metrics_never_sync(hip_lib):
    import spfsplatv2_amd as spf
    X, Y = (t.cuda() for t in so.smooth(16, (4, 3, 64, 64)))
    up = torch.linspace(0.5, 1.5, 4, device="cuda")
    module = spf.SSIM(data_range=1.0, size_average=False)

    def go():
        x, y = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        v = spf.ssim(x, y, data_range=1.0, nonnegative_ssim=True)[0]
        (1 - v).backward()
        w = module(x, y)[0]
        w.backward(up)
        return v.detach(), w.detach(), x.grad, y.grad, spf.compute_ssim(X, Y), spf.compute_psnr(X, Y)
    want = go()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = go()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(torch.equal(p, q) for p, q in zip(want, got))


# ---- 7. through the decoder ------------------------------------------------------------------------------------------
def test_ssim_term_through_the_decoder(hip_lib):
    """loss = 0.8 mse + 0.2 (1 - ssim) on the decoder's colour: the gradient arriving at out.color obeys the rule against
    the oracle's, and the Gaussians' gradients are finite and not those of the MSE term alone."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import decoder as dec
    from spfsplatv2_amd import synthetic as syn
    b = syn.make_batch("TEST", 1, 2, seed=17, s_mult=12.0, G=800, K=4, image_hw=(64, 64)).to("cuda")
    decoder = util.product_decoder()

    def step(with_ssim):
        leaves = [t.clone().requires_grad_(True) for t in (b.means, b.harmonics, b.opacities)]
        g = dec.Gaussians(leaves[0], b.covariances, b.rotations, b.scales, leaves[1], leaves[2])
        out = decoder.forward(g, b.extrinsics, b.intrinsics, b.near, b.far, b.image_shape)
        seen = {}
        out.color.register_hook(lambda gr: seen.setdefault("g", gr.detach().clone()))
        color, target = out.color.flatten(0, 1), b.target.flatten(0, 1)
        loss = 0.8 * spf.mse_loss(out.color, b.target)
        if with_ssim:
            loss = loss + 0.2 * (1 - spf.ssim(color, target, data_range=1.0)[0])
        loss.backward()
        return out.color.detach().flatten(0, 1).cpu(), seen["g"].flatten(0, 1).cpu(), [t.grad.cpu() for t in leaves]

    color, got, grads = step(True)
    _, _, grads_mse = step(False)
    target = b.target.flatten(0, 1).cpu()

    def oracle(dtype):
        c = color.to(dtype).requires_grad_(True)
        t = target.to(dtype)
        loss = 0.8 * ((c - t) ** 2).mean() + 0.2 * (1 - so.ssim_oracle(c, t, data_range=1.0, dtype=dtype))
        return torch.autograd.grad(loss, c)[0]
    truth = oracle(torch.float64)
    yp, ye = so.grad_errors(oracle(torch.float32), truth)
    pp, pe = so.grad_errors(got, truth)
    print("decoder", {"plane": pp, "element": pe}, {"plane": yp, "element": ye})
    _log("decoder/0.8mse+0.2(1-ssim)", {"plane": pp, "element": pe}, {"plane": yp, "element": ye})
    assert pp <= min(4 * yp + 1e-6, 1e-3) and pe <= min(4 * ye + 1e-5, 1e-2)
    for g_all, g_mse in zip(grads, grads_mse):
        assert bool(torch.isfinite(g_all).all()) and not torch.equal(g_all, g_mse)
        assert float((g_all - g_mse).abs().max()) > 1e-3 * float(g_mse.abs().max())
