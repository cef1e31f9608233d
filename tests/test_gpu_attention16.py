"""The 16-bit matrix path of the fused attention (``matrix16=True``) on the device.

Gate (per tensor out, dq, dk, dv, and per parameter gradient of the modules): err = max|x - x64| / max|x64| must not
exceed twice the err of the reference's own expression evaluated eagerly IN THE 16-BIT TYPE on the same device and
inputs, plus one ulp of that type (torch.finfo(dtype).eps).  The inputs are drawn in the 16-bit type, so the float64
oracle sees exactly the operands; the factor 2 covers a different summation order, and the fused path rounds in fewer
places than eager (q, k once after the rotation, P and dS once, the results once), so it is expected below eager.

The statistical gate is about 2e-2 wide at bfloat16 and cannot see one misplaced key among 131: the addressing and the
padding tests use data on which every operand and every product is exact in float16, bfloat16 and float32 accumulation
and pin positions and counts to 1e-6.
"""
import math

import pytest
import torch

from tests import attention_oracle as oracle
from tests.test_gpu_attention import CASES, NAMES, cancel_scales, errs, make_inputs

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = [torch.float16, torch.bfloat16]
CFG = (100.0, 1.0, 0.125)                   # base, F0, scale


def _id(dtype):
    return str(dtype).replace("torch.", "")


def run16(inp, packed, rope=True, scale=None, matrix16=True):
    """(out, dq, dk, dv) of the product with ``matrix16`` on the device."""
    import spfsplatv2_amd as spf
    qpos = inp["qpos"].to(DEV) if rope else None
    kpos = inp["kpos"].to(DEV) if rope else None
    dout = inp["dout"].to(DEV)
    if packed:
        qkv = inp["qkv"].to(DEV).requires_grad_(True)
        out = spf.rope_attention_packed(qkv, qpos, scale=scale, matrix16=matrix16)
        (g,) = torch.autograd.grad(out, (qkv,), dout)
        assert g.shape == qkv.shape and g.dtype == qkv.dtype           # ONE packed gradient of the dtype
        gt = g.transpose(1, 3)
        return out.detach(), gt[:, :, 0], gt[:, :, 1], gt[:, :, 2]
    q, k, v = (inp[n].to(DEV).requires_grad_(True) for n in "qkv")
    out = spf.rope_attention(q, k, v, qpos, kpos, scale=scale, matrix16=matrix16)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (q, k, v), dout))


def gate(label, got, eager, x64, dtype, zero_scales=None):
    eps = torch.finfo(dtype).eps
    e_got, e_eager = errs(got, x64, zero_scales), errs(eager, x64, zero_scales)
    for n, a, b in zip(NAMES, e_got, e_eager):
        print(f"{label} {_id(dtype)} {n}: product {a:.3e} eager {b:.3e} bound {2 * b + eps:.3e}")
    for g in got:
        assert g.dtype == dtype and torch.isfinite(g).all()
    for n, a, b in zip(NAMES, e_got, e_eager):
        assert a <= 2 * b + eps, (label, n, a, b)


_REF = {}


def reference(name, dtype, rope=True):
    """Inputs drawn in ``dtype``, the float64 oracle on exactly those and the eager evaluation in ``dtype`` on the device:
    computed once per case, never modified."""
    key = (name, dtype, rope)
    if key not in _REF:
        inp = make_inputs(name, dtype)
        qpos, kpos = (inp["qpos"], inp["kpos"]) if rope else (None, None)
        x64 = oracle.core_with_grads(inp["q"], inp["k"], inp["v"], qpos, kpos, inp["dout"])
        dpos = (qpos.to(DEV), kpos.to(DEV)) if rope else (None, None)
        eager = oracle.core_with_grads(inp["q"].to(DEV), inp["k"].to(DEV), inp["v"].to(DEV), *dpos, inp["dout"].to(DEV),
                                       dtype=dtype)
        _REF[key] = (inp, x64, eager)
    return _REF[key]


# ---- 1. the gate ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_against_oracle(name, dtype):
    inp, x64, eager = reference(name, dtype)
    got = run16(inp, packed=CASES[name][3] is None)
    gate(name, got, eager, x64, dtype, cancel_scales(inp))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_without_rope_against_oracle(dtype):
    inp, x64, eager = reference("cross_2x2x66_131", dtype, rope=False)
    got = run16(inp, packed=False, rope=False)
    gate("norope_cross_2x2x66_131", got, eager, x64, dtype, cancel_scales(inp))


# ---- 2. extreme logits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("where", ["first_tile", "last_tile"])
def test_extreme_logits(where, dtype):
    """Logits spread over [-80, 80]; the row maximum sits in the first or in the last (partly padded) key tile."""
    B, H, Nq, Nk = 1, 2, 40, 70
    gen = torch.Generator().manual_seed(5)
    u = torch.randn(64, generator=gen)
    u /= u.norm()
    beta = torch.linspace(-80, 78, Nk)[torch.randperm(Nk, generator=gen)]
    peak = 3 if where == "first_tile" else Nk - 2
    beta[peak] = 80.0
    q = (8.0 * u + 0.05 * torch.randn(B, H, Nq, 64, generator=gen)).to(dtype)
    k = (beta[None, None, :, None] * u + 0.05 * torch.randn(B, H, Nk, 64, generator=gen)).to(dtype)
    v = torch.randn(B, H, Nk, 64, generator=gen).to(dtype)
    inp = {"q": q, "k": k, "v": v, "qpos": None, "kpos": None, "dout": torch.randn(B, Nq, H * 64, generator=gen).to(dtype)}
    x64 = oracle.core_with_grads(q, k, v, None, None, inp["dout"])
    s = (q.double() @ k.double().transpose(-2, -1)) * 0.125
    assert s.max() > 79 and s.min() < -79 and (s.argmax(-1) == peak).all()
    eager = oracle.core_with_grads(q.to(DEV), k.to(DEV), v.to(DEV), None, None, inp["dout"].to(DEV), dtype=dtype)
    got = run16(inp, packed=False, rope=False)
    gate("extreme_" + where, got, eager, x64, dtype, cancel_scales(inp))


# ---- 3. addressing on near-exact data -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("seed", [16, 17, 18])
def test_every_query_finds_its_key(seed, dtype):
    """Cross-attention without RoPE, Nq = 70 over Nk = 131: key j is 8 u[j] with u[j] a random sign vector, query i is
    u[pi(i)], scale 1/8: the score of query i is 64 at key pi(i) and at most 64 - gap elsewhere.  With gap >= 24 the mass
    off the peak is below 131 e^-24 ~ 5e-9, under half a float32 ulp of 1: the softmax is 1 at pi(i), and since v and
    dout are small integers every operand and product is exact in both 16-bit types.  Then out[i] = v[pi(i)],
    dv[pi(i)] = dout[i], dv = 0 at keys nobody selects, and dq = dk = 0 (dS vanishes: dP = delta, exact integers)."""
    B, H, Nq, Nk = 1, 2, 70, 131
    gen = torch.Generator().manual_seed(seed)
    u = (torch.randint(0, 2, (B, H, Nk, 64), generator=gen) * 2 - 1).float()
    pi = torch.randperm(Nk, generator=gen)[:Nq]
    gram = u @ u.transpose(-2, -1)
    gram -= 64 * torch.eye(Nk)
    assert 64 - gram.max() >= 24                                        # the condition the test rests on
    k = (8 * u).to(dtype)
    q = u[:, :, pi].to(dtype)
    v = torch.randint(-4, 5, (B, H, Nk, 64), generator=gen).to(dtype)
    dout = torch.randint(-4, 5, (B, Nq, H * 64), generator=gen).to(dtype)
    inp = {"q": q, "k": k, "v": v, "qpos": None, "kpos": None, "dout": dout}
    out, dq, dk, dv = (t.float().cpu() for t in run16(inp, packed=False, rope=False, scale=0.125))
    want = v[:, :, pi].float().transpose(1, 2).reshape(B, Nq, H * 64)
    tol = 1e-6
    assert (out - want).abs().max() <= tol
    g = dout.float().reshape(B, Nq, H, 64).transpose(1, 2)              # [B,H,Nq,64]
    assert (dv[:, :, pi] - g).abs().max() <= tol
    rest = torch.ones(Nk, dtype=torch.bool)
    rest[pi] = False
    assert dv[:, :, rest].abs().max() <= tol
    assert dq.abs().max() <= tol and dk.abs().max() <= tol


# ---- 4. padding and counting on near-exact data ---------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("Nq", [33, 129])
@pytest.mark.parametrize("Nk", [64, 128, 70, 131])
def test_equal_scores_count_every_key_once(Nk, Nq, dtype):
    """All keys equal (k = -8 u, q = u): every score is -64, P = 1 / Nk, out = the mean of v and lse = -64 + ln Nk.  A padded
    key let in with score 0 would take all the mass; a key counted twice or dropped moves the mean and the log-sum-exp."""
    from spfsplatv2_amd import attention
    B, H = 1, 2
    gen = torch.Generator().manual_seed(40 + Nk + Nq)
    u = (torch.randint(0, 2, (B, H, 1, 64), generator=gen) * 2 - 1).float()
    q = u.expand(B, H, Nq, 64).contiguous().to(dtype).to(DEV)
    k = (-8 * u).expand(B, H, Nk, 64).contiguous().to(dtype).to(DEV)
    v = torch.randint(-4, 5, (B, H, Nk, 64), generator=gen).to(dtype)
    out, lse = attention.attention_forward(q, k, v.to(DEV), None, None, *CFG, matrix16=True)
    mean = v.double().mean(dim=2, keepdim=True).expand(B, H, Nq, 64).transpose(1, 2).reshape(B, Nq, H * 64)
    assert out.dtype == dtype and lse.dtype == torch.float32
    if Nk in (64, 128):                                                 # 1 / Nk is exact: bit for bit
        assert torch.equal(out.cpu(), mean.to(dtype))
    else:
        assert (out.double().cpu() - mean).abs().max() <= 2 * torch.finfo(dtype).eps * mean.abs().max()
    assert (lse.double().cpu() - (-64 + math.log(Nk))).abs().max() <= 1e-5


# ---- 5. layouts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("name", ["packed_2x3x70", "packed_1x2x64"])
def test_packed_equals_three_views_bitwise(name, dtype):
    import spfsplatv2_amd as spf
    inp, _, _ = reference(name, dtype)
    out_p, dq_p, dk_p, dv_p = run16(inp, packed=True)
    qkv = inp["qkv"].to(DEV).requires_grad_(True)
    t = qkv.transpose(1, 3)
    pos = inp["qpos"].to(DEV)
    out = spf.rope_attention(t[:, :, 0], t[:, :, 1], t[:, :, 2], pos, pos, matrix16=True)
    (g,) = torch.autograd.grad(out, (qkv,), inp["dout"].to(DEV))
    assert g.shape == qkv.shape and g.dtype == dtype
    assert torch.equal(out, out_p)
    gt = g.transpose(1, 3)
    assert torch.equal(gt[:, :, 0], dq_p) and torch.equal(gt[:, :, 1], dk_p) and torch.equal(gt[:, :, 2], dv_p)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("name", ["packed_2x3x70", "cross_2x2x66_131"])
def test_strided_inputs_are_read_in_place(name, dtype):
    from spfsplatv2_amd import attention
    inp, _, _ = reference(name, dtype)
    base = inp["qkv"].to(DEV) if inp["qkv"] is not None else None
    if base is not None:
        t = base.transpose(1, 3)
        q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    else:
        q, k, v = (inp[n].permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3) for n in "qkv")
    for t in (q, k, v):
        assert not t.is_contiguous()
        assert attention._rows(t) is t and attention._rows(t).data_ptr() == t.data_ptr()      # no copy
    strided = run16({**inp, "q": q, "k": k, "v": v}, packed=False)
    dense = run16({**inp, "q": q.contiguous(), "k": k.contiguous(), "v": v.contiguous()}, packed=False)
    for n, a, b in zip(NAMES, strided, dense):
        assert torch.equal(a, b), n


# ---- 6. reproducibility ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_back_to_back_calls_are_bit_identical(dtype):
    inp, _, _ = reference("cross_2x2x66_131", dtype)
    runs = [run16(inp, packed=False) for _ in range(10)]               # nothing synchronises in between
    for r in runs[1:]:
        for n, a, b in zip(NAMES, runs[0], r):
            assert torch.equal(a, b), n


# ---- 7. modules -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def goldens(golden_dir):
    cases = dict(torch.load(golden_dir / "attention_goldens.pt", weights_only=True))
    cases.update(torch.load(golden_dir / "attention_goldens_cross.pt", weights_only=True))
    return cases


def _rounded(case, dtype):
    """The golden case with its weights and inputs rounded to ``dtype`` (kept as float32 values): what the 16-bit module
    and the float64 oracle both start from."""
    c = dict(case)
    c["weights"] = {k: v.to(dtype).float() for k, v in case["weights"].items()}
    for k in case["inputs"]:
        c[k] = case[k].to(dtype).float()
    return c


def _oracle_module(case, dtype, device):
    """(out, {name: gradient}) of the oracle's self_attention / cross_attention in ``dtype`` on ``device``, for the inputs
    AND the parameters; the upstream gradient is the output itself (the goldens' loss 0.5 * sum(out^2)).  For the inputs in
    float64 on the CPU this is oracle.golden_case."""
    w = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in case["weights"].items()}
    ins = {k: case[k].to(device=device, dtype=dtype).requires_grad_(True) for k in case["inputs"]}
    pos = {k: case[k].to(device) for k in ("xpos", "qpos", "kpos") if k in case}
    if case["kind"] == "self":
        out = oracle.self_attention(ins["x"], pos["xpos"], w, case["num_heads"], case["base"])
    else:
        out = oracle.cross_attention(ins["query"], ins["memory"], ins["memory"], pos["qpos"], pos["kpos"], w,
                                     case["num_heads"], case["base"])
    wrt = {**ins, **w}
    grads = torch.autograd.grad(out, list(wrt.values()), out.detach())
    return out.detach(), dict(zip(wrt, grads))


def _build(case, dtype, matrix16):
    import spfsplatv2_amd as spf
    rope = spf.cuRoPE2D(case["base"], 1.0) if case["base"] is not None else None
    dim = next(iter(case["weights"].values())).shape[-1]
    cls = spf.Attention if case["kind"] == "self" else spf.CrossAttention
    mod = cls(dim, rope=rope, num_heads=case["num_heads"], qkv_bias=True, matrix16=matrix16)
    mod.load_state_dict(case["weights"])
    return mod.to(device=DEV, dtype=dtype)


def _run_module(mod, case, dtype):
    ins = {k: case[k].to(device=DEV, dtype=dtype).requires_grad_(True) for k in case["inputs"]}
    if case["kind"] == "self":
        out = mod(ins["x"], case["xpos"].to(DEV))
    else:
        out = mod(ins["query"], ins["memory"], ins["memory"], case["qpos"].to(DEV), case["kpos"].to(DEV))
    wrt = {**ins, **dict(mod.named_parameters())}
    grads = torch.autograd.grad(out, list(wrt.values()), out.detach())
    return out.detach(), dict(zip(wrt, grads))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("name", ["self_2x3x70", "cross_2x2x66_131"])
def test_flagged_modules_against_oracle(goldens, name, dtype):
    case = _rounded(goldens[name], dtype)
    x64_out, x64_grads = _oracle_module(case, torch.float64, "cpu")
    g64_out, g64_grads = oracle.golden_case(case)                      # the same oracle through its own entry point
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=0.0)
    assert close(g64_out, x64_out) and all(close(g64_grads[k], x64_grads[k]) for k in g64_grads)
    eager_out, eager_grads = _oracle_module(case, dtype, DEV)
    out, grads = _run_module(_build(case, dtype, True), case, dtype)
    assert sorted(grads) == sorted(x64_grads)
    eps = torch.finfo(dtype).eps
    figures = []
    for n, got, eag, x64 in [("out", out, eager_out, x64_out)] + [(k, grads[k], eager_grads[k], x64_grads[k]) for k in grads]:
        assert got.dtype == dtype and torch.isfinite(got).all(), n
        e_got, e_eager = errs([got], [x64])[0], errs([eag], [x64])[0]
        print(f"{name} {_id(dtype)} {n}: product {e_got:.3e} eager {e_eager:.3e} bound {2 * e_eager + eps:.3e}")
        figures.append((n, e_got, e_eager))
    for n, e_got, e_eager in figures:
        assert e_got <= 2 * e_eager + eps, (name, n, e_got, e_eager)


@pytest.mark.parametrize("name", ["self_2x3x70", "cross_2x2x66_131"])
def test_flagged_modules_fed_float32_equal_unflagged_bitwise(goldens, name):
    case = goldens[name]
    out_f, grads_f = _run_module(_build(case, torch.float32, True), case, torch.float32)
    out_u, grads_u = _run_module(_build(case, torch.float32, False), case, torch.float32)
    assert torch.equal(out_f, out_u)
    for k in grads_u:
        assert torch.equal(grads_f[k], grads_u[k]), k
