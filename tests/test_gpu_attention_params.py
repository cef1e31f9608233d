"""The fused attention on the device with what the other attention tests hold constant set free: positions drawn per
batch item, scene, view and token (query and key tables independent, y and x independent), and ``scale`` / ``base`` /
``F0`` away from 0.125 / 100 / 1 -- every variant: float32 plain, mask / norms, views, the 16-bit matrix path, modules.

Gate (the siblings' rule, per tensor out, dq, dk, dv and the norm or module parameter gradients): err = max|x - x64| /
max|x64| against the float64 oracle must not exceed twice the err of the same oracle evaluated eagerly on the device in
the call's dtype (float32; the 16-bit type for ``matrix16``) plus one ulp of that dtype.  Before a gate is trusted the
POWER CONDITION of tests/test_attention_params.py is asserted again with the device's eager figures: the float64 oracle
on the wrong positions (another item's, scene's or view's table, y and x swapped, one key's position) or with a default
in place of a parameter is at least 4 bounds away in every gated tensor, so a kernel that read them would fail.
Shapes, inputs and mutants: tests/attention_params_cases.py.  Every figure is printed
(profiles/attention_params_gate_figures.txt holds one run's).
"""
import pytest
import torch

from tests import attention_params_cases as cases
from tests.attention_params_cases import BF16, CROSS, DEFAULT, F16, F32, RAGGED, dtype_id
from tests.test_gpu_attention import _ulps, cancel_scales, errs

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = cases.NAMES


# ---- the product -----------------------------------------------------------------------------------------------------
def run_flat(inp, packed, variant="plain", cfg=DEFAULT, rope=True, matrix16=False):
    """(out, dq, dk, dv[, the four norm gradients]) of rope_attention / rope_attention_packed on the device."""
    import spfsplatv2_amd as spf
    scale, base, F0 = cfg
    kw = {"scale": scale, "base": base, "F0": F0}
    if matrix16:
        kw["matrix16"] = True
    params = []
    if "mask" in variant:
        kw["mask"] = inp["mask"].to(DEV)
    if "norm" in variant:
        params = [p.to(DEV).requires_grad_(True) for p in inp["params"]]
        kw.update(q_norm=(params[0], params[1], cases.NORM_EPS), k_norm=(params[2], params[3], cases.NORM_EPS))
    qpos = inp["qpos"].to(DEV) if rope else None
    kpos = inp["kpos"].to(DEV) if rope else None
    dout = inp["dout"].to(DEV)
    if packed:
        qkv = inp["qkv"].to(DEV).requires_grad_(True)
        out = spf.rope_attention_packed(qkv, qpos, **kw)
        g = torch.autograd.grad(out, [qkv] + params, dout)
        assert g[0].shape == qkv.shape and g[0].dtype == qkv.dtype
        gt = g[0].transpose(1, 3)
        return (out.detach(), gt[:, :, 0], gt[:, :, 1], gt[:, :, 2]) + tuple(g[1:])
    q, k, v = (inp[n].to(DEV).requires_grad_(True) for n in "qkv")
    out = spf.rope_attention(q, k, v, qpos, kpos, **kw)
    return (out.detach(),) + tuple(torch.autograd.grad(out, [q, k, v] + params, dout))


def views_on_device(inp):
    d = {n: (t.to(DEV) if isinstance(t, torch.Tensor) else t) for n, t in inp.items()}
    d["q"] = d["q_all"][:, 1:].transpose(2, 3)                          # the slice of the DEVICE buffer
    return d


def run_views(inp, cfg=DEFAULT, qpos=None, kpos=None):
    """(out, dq, dk, dv) of rope_attention_views on the device; qpos / kpos: device tensors to pass instead."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import attention
    d = views_on_device(inp)
    for t in (d["q"], d["k"], d["v"]):
        assert attention._rows5(t) is t                                 # read in place: no copy
    q, k, v = (d[n].requires_grad_(True) for n in "qkv")
    scale, base, F0 = cfg
    out = spf.rope_attention_views(q, k, v, d["qpos"] if qpos is None else qpos, d["kpos"] if kpos is None else kpos,
                                   allow=inp["allow"], scale=scale, base=base, F0=F0)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (q, k, v), d["dout"]))


# ---- the gate --------------------------------------------------------------------------------------------------------
def gate(label, got, eager, x64, dtype, dists, names=NAMES, zero_scales=None):
    """Prints every figure, asserts the power condition on the device's eager figures, then the gate."""
    eps = cases.eps_of(dtype)
    assert len(got) == len(eager) == len(x64) <= len(names)
    zs = None if zero_scales is None else list(zero_scales) + [None] * (len(x64) - len(zero_scales))
    e_got, e_eager = errs(got, x64, zs), errs(eager, x64, zs)
    for n, a, b in zip(names, e_got, e_eager):
        print(f"{label} {n}: product {a:.3e} eager {b:.3e} bound {2 * b + eps:.3e}")
    bad = cases.power_failures(label, dists, e_eager, eps, names)
    assert not bad, "\n".join(bad)
    for g in got:
        assert torch.isfinite(g).all()
    for n, a, b in zip(names, e_got, e_eager):
        assert a <= 2 * b + eps, (label, n, a, b)


def check_run(run, cfg=DEFAULT, rope=True, label=None):
    """One run of cases.POSITION_RUNS / PARAMETER_RUNS: product against oracle, through the gate."""
    layout, name, variant, dtype = run
    inp, fn, x64, dists = cases.reference(layout, name, variant, dtype, cfg, rope)
    eager = fn(dtype=dtype, device=DEV)
    label = label or cases.run_id(run if cfg == DEFAULT else run + (cfg,))
    if layout == "views":
        got = run_views(inp, cfg)
        b, H, Vq, Vk, Nq, Nk = cases.VIEWS[name]
        assert tuple(got[0].shape) == (b, Vq, Nq, H * 64) and got[2].shape == inp["k"].shape
        gate(label, got, eager, x64, dtype, dists)
        return
    got = run_flat(inp, cases.FLAT[name][3] is None, variant, cfg, rope, matrix16=dtype != F32)
    assert all(g.dtype == (dtype if i < 4 else F32) for i, g in enumerate(got))
    gate(label, got, eager, x64, dtype, dists, zero_scales=cancel_scales(inp, cfg[0]))


# ---- a. distinct positions, every variant ----------------------------------------------------------------------------
@pytest.mark.parametrize("run", cases.POSITION_RUNS, ids=cases.run_id)
def test_distinct_positions_against_oracle(run):
    """float32 plain (rope_attention and rope_attention_packed), mask, norms, mask + norms, views, and ``matrix16`` in
    float16 and bfloat16: forward and every gradient with a position table of its own per batch item, scene and view."""
    check_run(run)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=dtype_id)
def test_unflagged_sixteen_bit_types_follow_the_float32_path(dtype):
    """tests/test_gpu_attention.py::test_sixteen_bit_types_follow_the_float32_path with distinct positions: the unflagged
    16-bit kernels' results are the float32 kernels' (gated above) on the upcast operands, rounded."""
    from spfsplatv2_amd import attention
    inp = cases.flat_inputs(CROSS, dtype)
    q, k, v, dout = (inp[n].to(DEV) for n in ("q", "k", "v", "dout"))
    qpos, kpos = inp["qpos"].to(DEV), inp["kpos"].to(DEV)
    cfg = (100.0, 1.0, 0.125)
    out16, lse16 = attention.attention_forward(q, k, v, qpos, kpos, *cfg)
    out32, lse32 = attention.attention_forward(q.float(), k.float(), v.float(), qpos, kpos, *cfg)
    assert out16.dtype == dtype and torch.equal(lse16, lse32)
    assert _ulps(out16, out32.to(dtype)) <= 1

    def backward(q, k, v, out, dout):
        g = [torch.empty(t.shape, dtype=t.dtype, device=DEV) for t in (q, k, v)]
        attention.attention_backward(q, k, v, qpos, kpos, *cfg, out, lse16, dout, *g)
        return g
    g16 = backward(q, k, v, out16, dout)
    g32 = backward(q.float(), k.float(), v.float(), out16.float(), dout.float())
    for n, a, b in zip(NAMES[1:], g16, g32):
        assert a.dtype == dtype and torch.isfinite(a).all()
        assert _ulps(a, b.to(dtype)) <= 1, n
    # and the comparator is right on THESE positions: the float32 call on the upcast operands through the float32 gate
    f32 = {**inp, **{n: inp[n].float() for n in ("q", "k", "v", "dout")}}
    x64 = cases.flat_oracle(f32)
    dists = cases.mutant_distances(x64, lambda **kw: cases.flat_oracle(f32, **kw), cases.position_mutants(f32), True)
    got32 = run_flat(f32, packed=False)
    assert torch.equal(got32[0], out32)
    gate(f"upcast-{CROSS}-{dtype_id(dtype)}", got32, cases.flat_oracle(f32, dtype=F32, device=DEV), x64, F32, dists)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=dtype_id)
def test_the_gate_rejects_the_product_run_on_one_wrong_key_position(dtype):
    """The control of the gate on the device: the PRODUCT given the tightest mutant's tables (one key of 131 at another
    item's position) leaves the bound in every tensor, at float32 and at the widest gate, bfloat16 ``matrix16``."""
    inp, fn, x64, _ = cases.reference("flat", CROSS, "plain", dtype)
    qpos, kpos = cases.position_mutants(inp)["one key's position"]
    assert int((kpos != inp["kpos"]).any(-1).sum()) == 1
    got = run_flat({**inp, "qpos": qpos, "kpos": kpos}, packed=False, matrix16=dtype != F32)
    e_got, e_eager = errs(got, x64), errs(fn(dtype=dtype, device=DEV), x64)
    for n, a, b in zip(NAMES, e_got, e_eager):
        print(f"wrong_key_position-{dtype_id(dtype)} {n}: product on the mutant {a:.3e} bound {2 * b + cases.eps_of(dtype):.3e}")
        assert a > 2 * b + cases.eps_of(dtype), n


# ---- b. views positions read in place --------------------------------------------------------------------------------
def _same(a, b):
    for n, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), n


def test_views_positions_are_read_in_place_through_their_strides():
    """qpos the [:, 1:] slice and kpos the [:, :Vk] slice of buffers with one view more (other numbers in the extra view):
    neither the scene nor the view stride is the dense one, no copy is made, and the results are those of the contiguous
    copies, bit for bit -- and right."""
    from spfsplatv2_amd import attention
    run = ("views", RAGGED, "plain", F32)
    inp, fn, x64, dists = cases.reference(*run)
    b, H, Vq, Vk, Nq, Nk = cases.VIEWS[RAGGED]
    gen = torch.Generator().manual_seed(66)
    q_buf = torch.randint(0, 40, (b, Vq + 1, Nq, 2), generator=gen)
    k_buf = torch.randint(0, 40, (b, Vk + 1, Nk, 2), generator=gen)
    q_buf[:, 1:], k_buf[:, :Vk] = inp["qpos"], inp["kpos"]
    assert not torch.equal(q_buf[:, 0], q_buf[:, 1]) and not torch.equal(k_buf[:, Vk], k_buf[:, 0])
    qpos, kpos = q_buf.to(DEV)[:, 1:], k_buf.to(DEV)[:, :Vk]
    for p, dense in ((qpos, Vq * Nq * 2), (kpos, Vk * Nk * 2)):
        assert not p.is_contiguous() and p.stride(0) != dense
        assert attention._pos_rows(p) is p                              # no copy
    strided = run_views(inp, qpos=qpos, kpos=kpos)
    dense = run_views(inp, qpos=qpos.contiguous(), kpos=kpos.contiguous())
    _same(strided, dense)
    # and with padded token tables, so that the VIEW strides are not the dense ones either
    q_pad = torch.randint(0, 40, (b, Vq + 1, Nq + 3, 2), generator=gen)
    k_pad = torch.randint(0, 40, (b, Vk + 1, Nk + 5, 2), generator=gen)
    q_pad[:, 1:, :Nq], k_pad[:, :Vk, :Nk] = inp["qpos"], inp["kpos"]
    qpos, kpos = q_pad.to(DEV)[:, 1:, :Nq], k_pad.to(DEV)[:, :Vk, :Nk]
    for p, n in ((qpos, Nq), (kpos, Nk)):
        assert p.stride(1) != n * 2 and attention._pos_rows(p) is p
    _same(run_views(inp, qpos=qpos, kpos=kpos), dense)
    gate("strided_positions " + RAGGED, strided, fn(dtype=F32, device=DEV), x64, F32, dists)


def test_views_positions_with_strided_token_rows_take_the_copy_path():
    """Every other token row of a buffer twice as long: not readable in place, so ``_pos_rows`` copies, and the answer is
    that of the contiguous twin."""
    from spfsplatv2_amd import attention
    inp = cases.views_inputs(RAGGED)
    b, H, Vq, Vk, Nq, Nk = cases.VIEWS[RAGGED]
    gen = torch.Generator().manual_seed(67)
    q_buf = torch.randint(0, 40, (b, Vq, 2 * Nq, 2), generator=gen)
    k_buf = torch.randint(0, 40, (b, Vk, 2 * Nk, 2), generator=gen)
    q_buf[:, :, ::2], k_buf[:, :, ::2] = inp["qpos"], inp["kpos"]
    qpos, kpos = q_buf.to(DEV)[:, :, ::2], k_buf.to(DEV)[:, :, ::2]
    for p in (qpos, kpos):
        c = attention._pos_rows(p)
        assert c is not p and c.is_contiguous() and torch.equal(c, p)
    _same(run_views(inp, qpos=qpos, kpos=kpos), run_views(inp))


# ---- c. free scale, base, F0 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", cases.SETTINGS, ids=lambda c: "s%g_b%g_f%g" % c)
@pytest.mark.parametrize("run", cases.PARAMETER_RUNS, ids=cases.run_id)
def test_free_scale_base_and_F0_against_oracle(run, cfg):
    """Plain float32, mask + norms, views and ``matrix16`` at parameters no other test passes; the mutants here: the oracle
    with one changed parameter back at its default (a kernel that hard-codes it, in the forward or in either backward)."""
    check_run(run, cfg)


@pytest.mark.parametrize("dtype", [F32, F16, BF16], ids=dtype_id)
def test_free_scale_without_rope_against_oracle(dtype):
    check_run(("flat", CROSS, "plain", dtype), cases.NOROPE_SCALE, rope=False, label=f"norope-s0.2-{CROSS}-{dtype_id(dtype)}")


# ---- d. modules with a non-default rope ------------------------------------------------------------------------------
def _run_module(case, dtype, matrix16):
    import spfsplatv2_amd as spf
    kind = case["kind"]
    cls = spf.Attention if kind == "self" else spf.CrossAttention
    mod = cls(cases.MODULE_DIM, rope=spf.cuRoPE2D(freq=cases.MODULE_ROPE[0], F0=cases.MODULE_ROPE[1]),
              num_heads=cases.MODULE_HEADS, qkv_bias=True, matrix16=matrix16)
    mod.load_state_dict(case["weights"])
    mod = mod.to(device=DEV, dtype=dtype)
    ins = {k: t.to(device=DEV, dtype=dtype).requires_grad_(True) for k, t in case["inputs"].items()}
    pos = {k: t.to(DEV) for k, t in case["pos"].items()}
    if kind == "self":
        out = mod(ins["x"], pos["xpos"])
    elif kind == "cross":
        out = mod(ins["query"], ins["memory"], ins["memory"], pos["qpos"], pos["kpos"])
    else:
        out = mod.forward_views(ins["query"], ins["key"], pos["qpos"], pos["kpos"], case["allow"])
    wrt = {**ins, **dict(mod.named_parameters())}
    grads = torch.autograd.grad(out, list(wrt.values()), out.detach())
    return out.detach(), dict(zip(wrt, grads))


MODULE_RUNS = [(k, F32) for k in ("self", "cross", "views")] + [(k, d) for k in ("self", "cross") for d in (F16, BF16)]


@pytest.mark.parametrize("kind,dtype", MODULE_RUNS, ids=lambda x: x if isinstance(x, str) else dtype_id(x))
def test_modules_with_a_non_default_rope_against_oracle(kind, dtype):
    """``Attention``, ``CrossAttention`` and ``CrossAttention.forward_views`` (ragged views) with cuRoPE2D(10, 0.5), random
    weights, C = 128, H = 2 and positions per batch item, and the ``matrix16`` modules in both 16-bit types: the gate of
    tests/test_gpu_attention16.py::test_flagged_modules_against_oracle over the output and the gradients of the inputs
    and of every parameter.  Power (the oracle at base 100, at F0 1) is asked of the per-token tensors, as on the CPU."""
    case, names, x64, dists = cases.module_reference(kind, dtype)
    eager = cases.module_tensors(cases.module_oracle(case, dtype, DEV), names)
    result = _run_module(case, dtype, matrix16=dtype != F32)
    assert sorted(result[1]) == sorted(names[1:])
    got = cases.module_tensors(result, names)
    assert all(g.dtype == dtype for g in got)
    label = f"module_{kind}_rope10_F0.5 {dtype_id(dtype)}"
    n = 1 + len(case["inputs"])
    e_eager = cases.errs(eager[:n], x64[:n])
    bad = cases.power_failures(label, dists, e_eager, cases.eps_of(dtype), names[:n])
    assert not bad, "\n".join(bad)
    gate(label, got, eager, x64, dtype, {}, names)
