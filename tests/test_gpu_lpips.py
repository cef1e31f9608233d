"""LPIPS kernels (spfsplatv2_amd/csrc/lpips.hip) on the GPU.

Truth is tests/lpips_oracle.py in float64 on the host.  The yardstick is THE SAME ORACLE IN FLOAT32 on the host on the
same inputs (what an eager float32 run loses), never the product.  Every (case, product, yardstick) triple is appended
to profiles/lpips_parity.jsonl (SPF_LPIPS_PARITY_LOG names another file).

The value is continuous in the inputs, the gradient is not: a ReLU whose input is within float32 rounding of zero, or a
pool window whose two largest entries are that close, decides differently in float32 and in float64, and the product
flips OTHER units than the float32 oracle does.  Hence three layers:

(a) every operation on GIVEN inputs (the ReLU mask and the pool's choice come from the very float32 tensor the test
    passes to both sides, so no flip is possible): per output tensor
      max|got - f64| / max|f64| <= 8 x yardstick + 2.4e-7, never looser than 1e-5, and per element, for entries within
      two orders of the tensor's largest, |got - f64| / |f64| <= 8 x the yardstick's worst such ratio + 1e-5, never
      looser than 1e-2.
    8: every product output is ONE serial fmaf chain of up to 4,608 products where the host sums in blocks (a factor
    of about two over a different summation order alone); 2.4e-7 is two float32 roundings of a returned number.
(b) end to end, value, per image: |product - f64| / |f64| <= 8 x yardstick + 2.4e-7, never looser than 1e-5.
(c) end to end, gradient, per image: relative L2 error <= 1e-2 and max|g - w| / max|w| <= 1e-1 -- caps, 7 x and 9 x the
    worst the float32 oracle itself showed (flipped units), where a wiring error gives errors of order 1 -- and, in
    every case of four or more images, the product's MEDIAN per-image max-norm error <= 8 x the yardstick's median
    + 2.4e-7 (flips move the worst image, not the median).
(d) properties: identical inputs, a dead tap, bitwise repeatability and batch independence, no host synchronisation.

Record of the first MI355X run (52 of 56 passed; DESIGN.md section 7e has the whole account).  With ONE fmaf chain over
K = 4,608, `a/conv8/re10k_32/backward_data` missed rule (a) with a max-norm error of 2.40e-6 against 8 x 2.47e-7 + 2.4e-7
= 2.22e-6, and `a/conv11/re10k_16/forward` with 2.10e-6 against 1.95e-6; the rule stayed and the kernel now sums one
chain per tap.  `e2e/constant_0.0` and `e2e/constant_1.0` missed the caps of (c) on the gradient to the constant image with
a relative L2 error of 0.1006 / 0.1139 -- and so did the float32 oracle, with the same six digits: every interior pool
window of a constant image is an exact tie, which that host's float64 convolution broke by rounding noise; the oracle's
pool now takes the first entry within 1e-12 of the maximum in float64.  Neither change has been re-run on a GPU yet.
"""
import importlib
import json
import os
from functools import lru_cache
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_oracle as lo

pytestmark = pytest.mark.gpu

LOG = Path(os.environ.get("SPF_LPIPS_PARITY_LOG",
                          Path(__file__).resolve().parents[1] / "profiles" / "lpips_parity.jsonl"))
LEVEL = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
F64, F32 = torch.float64, torch.float32


def lp():
    return importlib.import_module("spfsplatv2_amd.lpips")


@lru_cache(maxsize=4)
def weights(seed=1, dead_tap=False):
    sd = lo.make_weights(seed)
    if dead_tap:                                       # conv5_3 = 0 with a negative bias: relu5_3 is 0 everywhere
        sd["net.slice5.28.weight"] = torch.zeros_like(sd["net.slice5.28.weight"])
        sd["net.slice5.28.bias"] = -0.1 - sd["net.slice5.28.bias"].abs()
    return sd, lp().LpipsWeights.from_state_dict(sd)   # (through the real loader)


def _log(case, product, yardstick):
    print(case, "product", product, "yardstick", yardstick)
    try:
        with open(LOG, "a") as f:
            f.write(json.dumps({"case": case, "product": product, "yardstick": yardstick}) + "\n")
    except OSError:                                    # a read-only tree: the assertions still hold
        pass


def _tensor_errors(t, f64):
    t = t.detach().to("cpu", F64)
    scale = float(f64.abs().max())
    err = (t - f64).abs()
    big = f64.abs() >= scale / 100
    return {"norm": float(err.max()) / scale, "element": float((err[big] / f64.abs()[big]).max())}


def _tight(case, got, f64, f32):
    """Rule (a) for one output tensor."""
    assert got.shape == f64.shape and got.dtype == F32, (case, got.shape, f64.shape, got.dtype)
    assert bool(torch.isfinite(got).all()), case
    if float(f64.abs().max()) == 0.0:
        assert not bool(got.any()), case
        return
    prod, yard = _tensor_errors(got, f64), _tensor_errors(f32, f64)
    _log(case, prod, yard)
    assert prod["norm"] <= min(8 * yard["norm"] + 2.4e-7, 1e-5), (case, "norm", prod, yard)
    assert prod["element"] <= min(8 * yard["element"] + 1e-5, 1e-2), (case, "element", prod, yard)


def _half_zero(shape, gen):
    """Post-ReLU random values: half the entries exactly 0."""
    return torch.relu(torch.randn(shape, generator=gen))


# ---- (a) every operation on given inputs -------------------------------------------------------------------------------
def _conv_oracle(x, layer, sd, dtype, normalize):
    convs, _, shift, scale = lo.params(sd, dtype)
    w, b = convs[layer - 1]
    x = x.to(dtype)
    return lo.conv(lo.scaled(x, shift, scale, normalize) if layer == 1 else x, w, b)


def _conv_bwd_oracle(g, act, layer, sd, dtype, normalize, hw):
    """Input gradient of layer `layer` for the upstream g counted where act > 0 (the mask from the SAME float32 act)."""
    convs, _, shift, scale = lo.params(sd, dtype)
    w, _ = convs[layer - 1]
    x = torch.zeros((g.shape[0], w.shape[1]) + hw, dtype=dtype, requires_grad=True)
    y = F.conv2d(lo.scaled(x, shift, scale, normalize) if layer == 1 else x, w, padding=1)
    return torch.autograd.grad(y, x, (g * (act > 0)).to(dtype))[0]


def _conv_case(name, layer, n, h, w, hip_lib, normalize=False):
    sd, W = weights()
    gen = torch.Generator().manual_seed(100 * layer + h)
    cin, cout = lo.CIN[layer - 1], lo.COUT[layer - 1]
    x = torch.rand((n, 3, h, w), generator=gen) if layer == 1 else _half_zero((n, cin, h, w), gen)
    got = lp().conv3x3_forward(x.cuda(), layer, W, normalize=normalize)
    _tight(f"{name}/forward", got.cpu(), _conv_oracle(x, layer, sd, F64, normalize),
           _conv_oracle(x, layer, sd, F32, normalize))
    g = torch.randn((n, cout, h, w), generator=gen)
    act = _half_zero((n, cout, h, w), gen)
    got = lp().conv3x3_backward_data(g.cuda(), layer, W, act=act.cuda(), normalize=normalize)
    _tight(f"{name}/backward_data", got.cpu(), _conv_bwd_oracle(g, act, layer, sd, F64, normalize, (h, w)),
           _conv_bwd_oracle(g, act, layer, sd, F32, normalize, (h, w)))


@pytest.mark.parametrize("layer", range(1, 14))
def test_conv_layer_at_re10k_size(hip_lib, layer):
    side = 256 >> LEVEL[layer - 1]
    _conv_case(f"a/conv{layer}/re10k_{side}", layer, 2, side, side, hip_lib, normalize=True)


@pytest.mark.parametrize("layer", range(1, 14))
def test_conv_layer_at_33x47_sizes(hip_lib, layer):
    """Rows and tiles that do not divide: the sizes a 33 x 47 image gives (33x47, 16x23, 8x11, 4x5, 2x2)."""
    k = LEVEL[layer - 1]
    _conv_case(f"a/conv{layer}/odd_{33 >> k}x{47 >> k}", layer, 3, 33 >> k, 47 >> k, hip_lib, normalize=True)


@pytest.mark.parametrize("normalize", [True, False])
def test_first_layer_pads_after_scaling(hip_lib, normalize):
    """Against an oracle that pads AFTER the scaling step; an all-zero image shows the difference at the border."""
    _conv_case(f"a/conv1/normalize={normalize}", 1, 2, 40, 56, hip_lib, normalize=normalize)
    sd, W = weights()
    z = torch.zeros(1, 3, 16, 16)
    got = lp().conv3x3_forward(z.cuda(), 1, W, normalize=normalize).cpu()
    _tight(f"a/conv1/zeros/normalize={normalize}", got, _conv_oracle(z, 1, sd, F64, normalize),
           _conv_oracle(z, 1, sd, F32, normalize))
    assert not torch.equal(got[:, :, 0, 0], got[:, :, 8, 8])


@pytest.mark.parametrize("shape", [(2, 64, 32, 32), (2, 128, 33, 47), (3, 64, 7, 5), (1, 512, 2, 2), (2, 256, 16, 23)])
def test_pool_both_ways(hip_lib, shape):
    gen = torch.Generator().manual_seed(shape[2])
    x = _half_zero(shape, gen)
    x[0, :, 0:2, 0:2] = 0.75                           # four equal non-zero entries: the first (row-major) takes it
    x[-1, :, 0:2, 2:4] = 0.0                           # four zeros
    got = lp().maxpool_forward(x.cuda()).cpu()
    assert torch.equal(got, lo.pool(x))
    g = torch.randn(got.shape, generator=gen)
    xr = x.clone().requires_grad_(True)
    want = torch.autograd.grad(lo.pool(xr), xr, g)[0]
    back = lp().maxpool_backward(g.cuda(), x.cuda()).cpu()
    assert torch.equal(back, want)
    assert torch.equal(back[0, :, 0, 0], g[0, :, 0, 0]) and not bool(back[0, :, 0:2, 0:2].flatten(1)[:, 1:].any())


def _head_oracle(a, b, lin, up, dtype):
    x, y = a.to(dtype).requires_grad_(True), b.to(dtype).requires_grad_(True)
    v = lo.head_term(x, y, lin.to(dtype).reshape(1, -1, 1, 1))
    ga, gb = torch.autograd.grad(v, [x, y], up.to(dtype))
    return v.detach(), ga, gb


@pytest.mark.parametrize("c,h,w", [(64, 33, 47), (128, 16, 23), (256, 8, 11), (512, 4, 5), (512, 2, 2), (64, 64, 64)])
def test_head_both_ways(hip_lib, c, h, w):
    n = 3
    gen = torch.Generator().manual_seed(c + h)
    a, b = _half_zero((n, c, h, w), gen), _half_zero((n, c, h, w), gen)
    a[0, :, 0, 1] = 0                                  # an all-zero vector in one image ...
    a[1, :, 1, 0] = 0                                  # ... and in both
    b[1, :, 1, 0] = 0
    lin = torch.rand(c, generator=gen) * (2.0 / c)
    up = torch.linspace(0.5, 1.5, n)
    truth, yard = _head_oracle(a, b, lin, up, F64), _head_oracle(a, b, lin, up, F32)
    name = f"a/head/{c}x{h}x{w}"
    _tight(f"{name}/value", lp().head_forward(a.cuda(), b.cuda(), lin.cuda()).cpu(), truth[0], yard[0])
    ga, gb = lp().head_backward(a.cuda(), b.cuda(), lin.cuda(), up.cuda())
    _tight(f"{name}/grad_a", ga.cpu(), truth[1], yard[1])
    _tight(f"{name}/grad_b", gb.cpu(), truth[2], yard[2])
    only_b = lp().head_backward(a.cuda(), b.cuda(), lin.cuda(), up.cuda(), need_a=False)
    assert only_b[0] is None and torch.equal(only_b[1], gb)
    # identical inputs: exactly 0 out, exactly 0 gradients
    assert not bool(lp().head_forward(a.cuda(), a.cuda(), lin.cuda()).any())
    za, zb = lp().head_backward(a.cuda(), a.cuda(), lin.cuda(), up.cuda())
    assert not bool(za.any()) and not bool(zb.any())


# ---- (b), (c) end to end ---------------------------------------------------------------------------------------------
def _upstream(n):
    return torch.linspace(0.5, 1.5, n)


def _grad_errors(g, truth):
    """Per image: (relative L2 error, max-norm error) of g [N,3,H,W] against truth (float64)."""
    d = (g.detach().to("cpu", F64) - truth).flatten(1)
    t = truth.flatten(1)
    return ((d.norm(dim=1) / t.norm(dim=1)).tolist(), (d.abs().amax(1) / t.abs().amax(1)).tolist())


def _check_value(case, got, truth, yard32):
    got = got.detach().to("cpu", F64).reshape(-1)
    prod = ((got - truth).abs() / truth.abs()).tolist()
    yard = ((yard32.to(F64) - truth).abs() / truth.abs()).tolist()
    _log(case + "/value", prod, yard)
    for p, y in zip(prod, yard):
        assert p <= min(8 * y + 2.4e-7, 1e-5), (case, "value", prod, yard)


def _check_grad(case, g, truth, yard32):
    assert g.shape == truth.shape and bool(torch.isfinite(g).all()), case
    (pl2, pmx), (yl2, ymx) = _grad_errors(g, truth), _grad_errors(yard32, truth)
    _log(case + "/grad", {"l2": pl2, "max": pmx}, {"l2": yl2, "max": ymx})
    assert max(pl2) <= 1e-2 and max(pmx) <= 1e-1, (case, "caps", pl2, pmx)
    if len(pmx) >= 4:
        med = lambda v: float(torch.tensor(v, dtype=F64).median())  # noqa: E731
        assert med(pmx) <= 8 * med(ymx) + 2.4e-7, (case, "median", med(pmx), med(ymx))


def _end_to_end(case, pred, target, normalize, W_seed=1, dead_tap=False):
    import spfsplatv2_amd as spf
    sd, W = weights(W_seed, dead_tap)
    n = pred.shape[0]
    up = _upstream(n)
    t_v, t_g0, t_g1 = lo.lpips_with_grads(pred, target, sd, normalize, F64, up)
    y_v, y_g0, y_g1 = lo.lpips_with_grads(pred, target, sd, normalize, F32, up)
    P, T = pred.cuda(), target.cuda()
    module = spf.LPIPS(net="vgg", weights=W)
    for api, fn in (("lpips", lambda a, b: spf.lpips(a, b, W, normalize=normalize)),
                    ("LPIPS", lambda a, b: module(a, b, normalize=normalize))):
        for need in ((True, False), (False, True), (True, True)):
            a, b = P.clone().requires_grad_(need[0]), T.clone().requires_grad_(need[1])
            v = fn(a, b)
            assert v.shape == (n, 1, 1, 1) and v.dtype == F32
            _check_value(f"{case}/{api}/need={need}", v, t_v, y_v)
            wanted = [(t, tg, yg, which) for t, tg, yg, which, k in ((a, t_g0, y_g0, "in0", need[0]),
                                                                      (b, t_g1, y_g1, "in1", need[1])) if k]
            grads = torch.autograd.grad(v.reshape(-1), [t for t, _, _, _ in wanted], up.cuda())
            for g, (_, tg, yg, which) in zip(grads, wanted):
                _check_grad(f"{case}/{api}/need={need}/{which}", g, tg, yg)
    if normalize:
        # compute_lpips: ground truth first, [batch] in predicted.dtype, no gradient state
        m = spf.compute_lpips(P.clone().requires_grad_(True), T, weights=W)
        assert m.shape == (n,) and m.dtype == P.dtype and not m.requires_grad
        _check_value(f"{case}/compute_lpips", m, t_v, y_v)
        # LossLpips on [b,v,3,h,w]: weight x the mean of the per-image values, and its 0-dim backward
        loss = spf.LossLpips(spf.LossLpipsCfgWrapper(spf.LossLpipsCfg(0.25, 10)), weights=W)
        a = P.clone().requires_grad_(True)
        out = loss(a[None], T[None], None, 10)
        assert out.shape == () and out.dtype == F32
        ones = torch.ones(n)
        m_v, m_g0, _ = lo.lpips_with_grads(pred, target, sd, True, F64, ones * 0.25 / n)
        k_v, k_g0, _ = lo.lpips_with_grads(pred, target, sd, True, F32, ones * 0.25 / n)
        _check_value(f"{case}/LossLpips", out, 0.25 * m_v.mean().reshape(1), 0.25 * k_v.mean().reshape(1))
        out.backward()
        _check_grad(f"{case}/LossLpips/in0", a.grad, m_g0, k_g0)


CASES = {
    "64": ((2, 3, 64, 64), 0.1, True), "40x56": ((2, 3, 40, 56), 0.1, True), "33x47": ((3, 3, 33, 47), 0.1, True),
    "16_minimum": ((1, 3, 16, 16), 0.1, True), "224_vggt": ((2, 3, 224, 224), 0.1, True),
    "256_re10k_step": ((16, 3, 256, 256), 0.1, True), "33x47_noise0.02": ((3, 3, 33, 47), 0.02, True),
    "64_raw": ((2, 3, 64, 64), 0.1, False), "33x47_raw": ((3, 3, 33, 47), 0.1, False),
    "5x48_median": ((5, 3, 48, 48), 0.1, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_end_to_end_value_and_gradients(hip_lib, case):
    shape, noise, normalize = CASES[case]
    pred, target = lo.image_pair(7, shape, noise)
    _end_to_end(f"e2e/{case}", pred, target, normalize)


@pytest.mark.parametrize("level", [0.0, 1.0])
def test_constant_image_against_noisy(hip_lib, level):
    _, noisy = lo.image_pair(9, (2, 3, 40, 56))
    _end_to_end(f"e2e/constant_{level}", torch.full_like(noisy, level), noisy, True)


def test_dtypes_and_strides_are_the_float32_contiguous_result_bitwise(hip_lib):
    import spfsplatv2_amd as spf
    _, W = weights()
    gen = torch.Generator().manual_seed(3)
    big = torch.rand((3, 5, 40, 70), generator=gen).cuda()
    a, b = big[:, 1:4, :, 3:59], big[:, 2:5, :, 10:66]            # channel-sliced, strided views
    assert not a.is_contiguous()
    want = spf.lpips(a.contiguous(), b.contiguous(), W, normalize=True)
    assert torch.equal(spf.lpips(a, b, W, normalize=True), want)
    a16, b16 = a.bfloat16(), b.bfloat16()
    want16 = spf.lpips(a16.float().contiguous(), b16.float().contiguous(), W, normalize=True)
    assert torch.equal(spf.lpips(a16, b16, W, normalize=True), want16)
    x = a16.clone().requires_grad_(True)
    spf.lpips(x, b16, W, normalize=True).sum().backward()
    assert x.grad.dtype == torch.bfloat16 and bool(torch.isfinite(x.grad).all()) and bool(x.grad.any())
    m = spf.compute_lpips(b16, a16, weights=W)
    assert m.dtype == torch.bfloat16 and m.shape == (3,)


# ---- (d) properties -----------------------------------------------------------------------------------------------------
def test_identical_inputs_give_exact_zeros(hip_lib):
    import spfsplatv2_amd as spf
    _, W = weights()
    pred, _ = lo.image_pair(2, (2, 3, 33, 47))
    x = pred.cuda().requires_grad_(True)
    v = spf.lpips(x, x, W, normalize=True)
    assert not bool(v.any())
    v.sum().backward()
    assert not bool(x.grad.any())
    a, b = pred.cuda().requires_grad_(True), pred.clone().cuda().requires_grad_(True)      # a bitwise copy
    v = spf.lpips(a, b, W, normalize=True)
    v.backward(torch.linspace(0.5, 1.5, 2).reshape(2, 1, 1, 1).cuda())
    assert not bool(v.any()) and not bool(a.grad.any()) and not bool(b.grad.any())


def test_dead_tap(hip_lib):
    """relu5_3 is 0 at every pixel (both norms 0 there) while taps 1 to 4 stay alive: the value by rule (b), the gradients
    finite and within (c)."""
    sd, _ = weights(1, True)
    pred, target = lo.image_pair(4, (2, 3, 40, 56))
    convs, _, shift, scale = lo.params(sd, F64)
    taps = lo.features(pred.double(), convs, shift, scale, True)
    assert not bool(taps[4].any()) and all(bool((t > 0).double().mean() > 0.2) for t in taps[:4])
    _end_to_end("d/dead_tap", pred, target, True, dead_tap=True)


def test_bitwise_repeatable_and_independent_of_the_batch(hip_lib):
    import spfsplatv2_amd as spf
    _, W = weights()
    pred, target = lo.image_pair(6, (5, 3, 40, 56))
    up = torch.linspace(0.5, 1.5, 5).cuda()

    def run(p, t, u):
        a, b = p.cuda().requires_grad_(True), t.cuda().requires_grad_(True)
        v = spf.lpips(a, b, W, normalize=True)
        ga, gb = torch.autograd.grad(v.reshape(-1), [a, b], u)
        return v.detach(), ga, gb
    first, second = run(pred, target, up), run(pred, target, up)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    for i in (0, 3):
        alone = run(pred[i:i + 1], target[i:i + 1], up[i:i + 1])
        assert all(torch.equal(x[i:i + 1], y) for x, y in zip(first, alone)), i


def test_forward_backward_loss_and_metric_never_sync(hip_lib):
    import spfsplatv2_amd as spf
    _, W = weights()
    pred, target = lo.image_pair(8, (2, 3, 32, 48))
    P, T = pred.cuda(), target.cuda()
    loss = spf.LossLpips(spf.LossLpipsCfgWrapper(spf.LossLpipsCfg(0.05, 0)), weights=W)
    up = torch.ones(2, 1, 1, 1, device="cuda")
    one = torch.ones((), device="cuda")
    spf.lpips(P, T, W, normalize=True)                 # the weights reach the device once, before the mode is set
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a, b = P.clone().requires_grad_(True), T.clone().requires_grad_(True)
        spf.lpips(a, b, W, normalize=True).backward(up)
        x = P.clone().requires_grad_(True)
        loss(x[None], T[None], None, 1).backward(one)
        m = spf.compute_lpips(T, P, weights=W)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(b.grad).all()) and bool(x.grad.any())
    assert m.shape == (2,) and bool((m > 0).all())
