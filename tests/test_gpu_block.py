"""The transformer block's kernels and modules on the device (csrc/block.hip, spfsplatv2_amd/block.py).

Gate (tests/block_cases.py, the rule of tests/test_gpu_attention_params.py): per tensor err = max|x - x64| / max|x64|
against the float64 oracle must not exceed twice the err of the same oracle run eagerly in float32 on the device plus
one float32 ulp; before a gate is trusted the power condition of tests/test_block.py is asserted again with the device's
eager figures.  Every figure is printed (profiles/block_gate_figures.txt holds one run's).
"""
import ctypes as C

import pytest
import torch

from tests import block_cases as cases
from tests import block_oracle as bo

pytestmark = pytest.mark.gpu

DEV = "cuda"


# ---- the product -----------------------------------------------------------------------------------------------------
def _dev(d, requires_grad=()):
    out = {}
    for k, v in d.items():
        out[k] = None if v is None else v.to(DEV)
        if out[k] is not None and k in requires_grad:
            out[k].requires_grad_(True)
    return out


def run_norm(d, dev=None):
    """{name: tensor} over block_oracle.NORM_NAMES of layer_norm / add_layer_norm on the device."""
    import spfsplatv2_amd as spf
    t = dev or _dev(d, ("x", "r", "weight", "bias", "gamma"))
    if t["r"] is None:
        y = spf.layer_norm(t["x"], t["weight"], t["bias"], cases.EPS)
        outs, ups = [y], [t["dy"]]
    else:
        s, y = spf.add_layer_norm(t["x"], t["r"], t["weight"], t["bias"], cases.EPS, gamma=t["gamma"])
        outs, ups = ([s, y], [t["ds"], t["dy"]]) if t["ds"] is not None else ([y], [t["dy"]])
    leaves = {"dx": t["x"], "dr": t["r"], "dweight": t["weight"], "dbias": t["bias"], "dgamma": t["gamma"]}
    leaves = {k: v for k, v in leaves.items() if v is not None}
    grads = torch.autograd.grad(outs, list(leaves.values()), ups)
    res = {"y": y.detach(), **dict(zip(leaves, grads))}
    if t["r"] is not None:
        res["s"] = s.detach()
    return res


def run_gelu(d):
    import spfsplatv2_amd as spf
    t = _dev(d, ("u", "bias"))
    h = spf.bias_gelu(t["u"], t["bias"])
    g = torch.autograd.grad(h, [t["u"]] + ([t["bias"]] if t["bias"] is not None else []), t["dh"])
    res = {"h": h.detach(), "du": g[0]}
    if t["bias"] is not None:
        res["db"] = g[1]
    return res


def check_norm(rows, c, variant):
    d, x64, dists = cases.norm_reference(rows, c, variant)
    got = run_norm(d)
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.shape == x64[k].shape, k
    cases.gate(f"norm C={c} rows={rows} {variant}", got, cases.norm_oracle(d, torch.float32, DEV), x64, dists)


def check_gelu(rows, c, with_bias):
    d, x64, dists = cases.gelu_reference(rows, c, with_bias)
    got = run_gelu(d)
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.shape == x64[k].shape, k
    cases.gate(f"gelu C={c} rows={rows} bias={with_bias}", got, cases.gelu_oracle(d, torch.float32, DEV), x64, dists)


# ---- a. kernel parity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", cases.ROWS)
@pytest.mark.parametrize("c", cases.WIDTHS)
def test_norm_kernels_against_oracle(c, rows):
    """Forward and every gradient (dx, dr, dweight, dbias, dgamma) with and without r, ds and gamma: the degenerate width
    4, part of a wave idle (128, 192), one vector past a full wave round (260), the real widths and the upper edge."""
    for variant in cases.NORM_VARIANTS:
        check_norm(rows, c, variant)


@pytest.mark.parametrize("rows", cases.ROWS)
@pytest.mark.parametrize("c", cases.WIDTHS)
def test_gelu_kernels_against_oracle(c, rows):
    for with_bias in (True, False):
        check_gelu(rows, c, with_bias)


@pytest.mark.parametrize("variant", ["plain", "r_gamma_ds"])
def test_norm_row_loop_and_partials_of_a_capped_grid(variant):
    """More rows than one pass of the capped grid covers: every block loops over rows and the reducer sums the partials
    of all 1024 blocks."""
    from spfsplatv2_amd import block
    rows = cases.NORM_LOOP_ROWS
    assert block.partial_blocks(rows, 128) * 16 < rows
    check_norm(rows, 128, variant)


def test_gelu_row_loop_and_partials_of_a_capped_grid():
    from spfsplatv2_amd import block
    rows = cases.GELU_LOOP_ROWS
    assert block.partial_blocks(rows, 128, True) * 16 < rows
    check_gelu(rows, 128, True)


def test_the_gate_rejects_the_product_run_at_the_other_eps():
    """The control of the gate on the device: the PRODUCT at eps = 1e-5 leaves the bound in y and dx."""
    import spfsplatv2_amd as spf
    d, x64, _ = cases.norm_reference(37, 768, "plain")
    t = _dev(d, ("x",))
    y = spf.layer_norm(t["x"], t["weight"], t["bias"], bo.OTHER_EPS)
    (dx,) = torch.autograd.grad(y, t["x"], t["dy"])
    e_eager = cases.errors(cases.norm_oracle(d, torch.float32, DEV), x64)
    for k, v in (("y", y), ("dx", dx)):
        a = bo.rel_err(v, x64[k])
        print(f"wrong_eps {k}: product at the other eps {a:.3e} bound {2 * e_eager[k] + cases.ULP:.3e}")
        assert a > 2 * e_eager[k] + cases.ULP, k


# ---- b. strided input ------------------------------------------------------------------------------------------------
def test_a_view_of_a_larger_tensor_is_read_in_place():
    """x = tok[:, 1] of a [B, V, N, C] tensor and r = res[:, 0] of one with another V: two strides address the rows, no
    copy is made, and every result is that of the contiguous copies, bit for bit -- and right."""
    from spfsplatv2_amd import block
    B, N, c = 2, 37, 128
    d, x64, dists = cases.norm_reference(B * N, c, "r_gamma_ds")
    gen = torch.Generator().manual_seed(5)
    tok, res = torch.randn(B, 3, N, c, generator=gen), torch.randn(B, 2, N, c, generator=gen)
    tok[:, 1], res[:, 0] = d["x"].reshape(B, N, c), d["r"].reshape(B, N, c)
    tok, res = tok.to(DEV), res.to(DEV)
    x, r = tok[:, 1], res[:, 0]
    for v in (x, r):
        assert not v.is_contiguous() and block._rows(v) is v            # read in place: no copy
    assert block._row_map(x) == (N, c, 3 * N * c) and block._row_map(r) == (N, c, 2 * N * c)
    shaped = {k: (v.reshape(B, N, c) if v is not None and v.dim() == 2 else v) for k, v in d.items()}
    base = _dev(shaped, ("weight", "bias", "gamma"))

    def run(x, r):
        t = dict(base, x=x.detach().requires_grad_(True), r=r.detach().requires_grad_(True))
        return run_norm(None, t)
    strided, dense = run(x, r), run(x.contiguous(), r.contiguous())
    for k in dense:
        assert torch.equal(strided[k], dense[k]), k
    flat = {k: (v.reshape(B * N, c) if v.dim() == 3 else v) for k, v in strided.items()}
    cases.gate("strided C=128 rows=74 r_gamma_ds", flat, cases.norm_oracle(d, torch.float32, DEV), x64, dists)
    # the plain norm through the same view
    t = dict(base, x=x.detach().requires_grad_(True), r=None, gamma=None, ds=None)
    u = dict(t, x=x.contiguous().requires_grad_(True))
    a, b = run_norm(None, t), run_norm(None, u)
    for k in b:
        assert torch.equal(a[k], b[k]), k


# ---- c. reproducibility ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,c", [(37, 768), (cases.NORM_LOOP_ROWS, 128), (1000, 4096)])
def test_backwards_are_bitwise_reproducible(rows, c):
    """No float atomics: two runs of every backward agree bit for bit (several blocks' partials at each of these sizes)."""
    for variant in cases.NORM_VARIANTS:
        d = cases.norm_inputs(rows, c, variant)
        a, b = run_norm(d), run_norm(d)
        for k in a:
            assert torch.equal(a[k], b[k]), (variant, k)
    for with_bias in (True, False):
        d = cases.gelu_inputs(rows, c, with_bias)
        a, b = run_gelu(d), run_gelu(d)
        for k in a:
            assert torch.equal(a[k], b[k]), (with_bias, k)


# ---- d. modules ------------------------------------------------------------------------------------------------------
def _prepare(kind, g):
    """The module with the golden's weights and its inputs, on the device."""
    mod = cases.build_module(kind, g).to(DEV)
    ins = {k: v.to(DEV).requires_grad_(True) for k, v in g["inputs"].items()}
    pos = {k: v.to(DEV) for k, v in g["pos"].items()}
    return mod, ins, pos


def _step(kind, mod, ins, pos):
    """Forward and the backward of 0.5 * sum(out^2) to the inputs and every parameter."""
    out = cases.run_module(kind, mod, ins, pos)
    wrt = {**ins, **dict(mod.named_parameters())}
    grads = dict(zip(wrt, torch.autograd.grad(0.5 * (out * out).sum(), list(wrt.values()))))
    return out.detach(), {k: grads[k] for k in ins}, {k: grads[k] for k in wrt if k not in ins}


def _run_module(kind, g):
    return _step(kind, *_prepare(kind, g))


@pytest.mark.parametrize("kind", cases.KINDS)
def test_modules_against_golden_and_oracle(kind, golden_dir):
    """Each module with its golden's state dict: the output and the input gradients against the reference's golden
    through the float64 oracle (which test_block.py pins to the golden), the parameter gradients against the oracle."""
    g, x64, dists = cases.module_reference(kind, golden_dir)
    got = cases.flat(_run_module(kind, g))
    eager = cases.flat(bo.module_case(g, torch.float32, DEV))
    assert sorted(k for k in got if k.startswith("dparam_")) == sorted("dparam_" + k for k in g["weights"])
    cases.gate(f"module {kind}", got, eager, x64, dists)
    assert bo.rel_err(got["out"], g["out"].double()) < 2e-6
    for k, v in g["grads"].items():
        assert bo.rel_err(got["d_" + k], v.double()) < 5e-6, k


def test_eval_mode_and_zero_rates_are_identities(golden_dir):
    """drop and drop_path in eval mode change nothing: the same bits as the module built without them."""
    import spfsplatv2_amd as spf
    g = cases.golden("block", golden_dir)
    ref = cases.build_module("block", g).to(DEV).eval()
    mod = spf.Block(g["dim"], g["num_heads"], mlp_ratio=g["mlp_ratio"], qkv_bias=True, drop=0.2, drop_path=0.3,
                    norm_layer=lambda dim: torch.nn.LayerNorm(dim, eps=g["eps"]), rope=spf.cuRoPE2D(freq=g["base"]))
    mod.load_state_dict(g["weights"])
    mod = mod.to(DEV).eval()
    x, pos = g["inputs"]["x"].to(DEV), g["pos"]["xpos"].to(DEV)
    with torch.no_grad():
        assert torch.equal(mod(x, pos), ref(x, pos))
    with pytest.raises(NotImplementedError):
        mod.train()(x, pos)


# ---- e. no host synchronisation --------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.KINDS)
def test_forward_backward_never_sync(kind, golden_dir):
    prepared = _prepare(kind, cases.golden(kind, golden_dir))
    want = _step(kind, *prepared)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = _step(kind, *prepared)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(want[0], got[0])
    for a, b in ((want[1], got[1]), (want[2], got[2])):
        for k in a:
            assert torch.equal(a[k], b[k]), k


# ---- f. the library's argument checks --------------------------------------------------------------------------------
def test_library_argument_checks_launch_nothing(hip_lib):
    """SPF_E_INVALID with a message, on real device buffers that must come back untouched."""
    from spfsplatv2_amd import _lib
    rows, c = 5, 128
    x = torch.randn(rows, c, device=DEV)
    w, b = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    y = torch.full((rows, c), 7.0, device=DEV)
    stats = torch.full((rows, 4), 7.0, device=DEV)

    def norm(**kw):
        a = _lib.SpfBlockNorm()
        a.x, a.weight, a.bias = x.data_ptr(), w.data_ptr(), b.data_ptr()
        a.x_inner, a.x_stride, a.r_inner, a.rows, a.C, a.eps = rows, c, 1, rows, c, 1e-6
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)
    p = lambda t: C.c_void_p(t.data_ptr())
    fwd, bwd, err = hip_lib.spf_block_add_norm_forward, hip_lib.spf_block_add_norm_backward, hip_lib.spf_last_error
    assert fwd(norm(x=None), None, p(y), p(stats), None) == -1 and b"null pointer" in err()
    assert fwd(norm(), None, None, p(stats), None) == -1 and b"null output" in err()
    assert fwd(norm(C=130), None, p(y), p(stats), None) == -1 and b"multiple of 4" in err()
    assert fwd(norm(C=8192), None, p(y), p(stats), None) == -1 and b"multiple of 4" in err()
    assert fwd(norm(gamma=w.data_ptr()), None, p(y), p(stats), None) == -1 and b"gamma is given without r" in err()
    assert bwd(norm(gamma=w.data_ptr()), p(x), None, p(stats), p(y), p(y), p(y), p(y), None) == -1
    assert b"gamma is given without r" in err()
    assert hip_lib.spf_block_bias_gelu_forward(p(x), p(b), rows, 130, p(y), None) == -1 and b"multiple of 4" in err()
    assert hip_lib.spf_block_bias_gelu_forward(None, p(b), rows, c, p(y), None) == -1 and b"null pointer" in err()
    assert hip_lib.spf_block_bias_gelu_backward(p(x), p(b), p(x), rows, c, p(y), None, None, None) == -1
    assert b"with a bias and only then" in err()
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((stats == 7.0).all())
    # and the same calls, well formed, do launch
    assert fwd(norm(), None, p(y), p(stats), None) == 0
    torch.cuda.synchronize()
    assert bo.rel_err(y, torch.nn.functional.layer_norm(x.double().cpu(), (c,), eps=1e-6)) < 1e-6
