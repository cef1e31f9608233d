"""Fused RoPE attention on the device: forward and the three gradients against the float64 oracle and the reference's
goldens, layouts, extreme logits, reproducibility and the 16-bit types.

Gate for float32 (per tensor out, dq, dk, dv): err = max|x - x64| / max|x64| must not exceed twice the err of the
reference's own expression evaluated eagerly in float32 on the same device and inputs (tests/attention_oracle.py's
formula, rotation included) plus one float32 ulp: the factor 2 covers a different summation order of an equally long
float32 chain; a layout or tile-edge defect shows orders of magnitude above it.
"""
import pytest
import torch

from tests import attention_oracle as oracle

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
DEV = "cuda"
NAMES = ("out", "dq", "dk", "dv")


def grid_positions(B, hh, ww, extra):
    """PositionGetter's (y, x) grid plus `extra` tokens one row below the grid each (append_token_position)."""
    y, x = torch.meshgrid(torch.arange(hh), torch.arange(ww), indexing="ij")
    pos = torch.stack([y.reshape(-1), x.reshape(-1)], dim=-1)
    for i in range(extra):
        pos = torch.cat([pos, torch.tensor([[hh + i, 0]])])
    return pos[None].expand(B, -1, -1).clone().long()


# name: (B, H, Nq grid, Nk grid or None for packed self-attention)
CASES = {
    "packed_2x3x70": (2, 3, (17, 4, 2), None),
    "cross_2x2x66_131": (2, 2, (8, 8, 2), (13, 10, 1)),
    "one_1x1x1_1": (1, 1, (1, 1, 0), (1, 1, 0)),
    "packed_1x2x64": (1, 2, (8, 8, 0), None),
    "cross_1x1x129_1": (1, 1, (8, 16, 1), (1, 1, 0)),
    "packed_3x12x258": (3, 12, (16, 16, 2), None),      # the decoder's layout: patches + intrinsics + pose token
}


def make_inputs(name, dtype=torch.float32):
    B, H, qg, kg = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    qpos = grid_positions(B, *qg)
    Nq = qpos.shape[1]
    if kg is None:
        qkv = torch.randn(B, Nq, 3, H, 64, generator=gen).to(dtype)
        t = qkv.transpose(1, 3)
        q, k, v, kpos = t[:, :, 0], t[:, :, 1], t[:, :, 2], qpos
    else:
        kpos = grid_positions(B, *kg)
        Nk = kpos.shape[1]
        q = torch.randn(B, Nq, H, 64, generator=gen).to(dtype).permute(0, 2, 1, 3)
        k = torch.randn(B, Nk, H, 64, generator=gen).to(dtype).permute(0, 2, 1, 3)
        v = torch.randn(B, Nk, H, 64, generator=gen).to(dtype).permute(0, 2, 1, 3)
        qkv = None
    dout = torch.randn(B, Nq, H * 64, generator=gen).to(dtype)
    return {"qkv": qkv, "q": q, "k": k, "v": v, "qpos": qpos, "kpos": kpos, "dout": dout}


def run_product(inp, packed, rope=True, scale=None):
    """(out, dq, dk, dv) of the product on the device; packed: through rope_attention_packed and its one gradient."""
    import spfsplatv2_amd as spf
    qpos = inp["qpos"].to(DEV) if rope else None
    kpos = inp["kpos"].to(DEV) if rope else None
    dout = inp["dout"].to(DEV)
    if packed:
        qkv = inp["qkv"].to(DEV).requires_grad_(True)
        out = spf.rope_attention_packed(qkv, qpos, scale=scale)
        (g,) = torch.autograd.grad(out, (qkv,), dout)
        assert g.shape == qkv.shape
        gt = g.transpose(1, 3)
        return out.detach(), gt[:, :, 0], gt[:, :, 1], gt[:, :, 2]
    q, k, v = (inp[n].to(DEV).requires_grad_(True) for n in "qkv")
    out = spf.rope_attention(q, k, v, qpos, kpos, scale=scale)
    return (out.detach(),) + tuple(torch.autograd.grad(out, (q, k, v), dout))


def errs(got, want, zero_scales=None):
    """max|x - x64| / max|x64| per tensor; a tensor whose float64 value is identically zero is measured against its
    entry of `zero_scales` instead (see cancel_scales)."""
    res = []
    for i, (g, w) in enumerate(zip(got, want)):
        den = float(w.abs().max())
        if den == 0.0 and zero_scales is not None:
            den = zero_scales[i]
        res.append(float((g.detach().double().cpu() - w).abs().max()) / den)
    return res


def cancel_scales(inp, scale=0.125):
    """With a single key the probabilities are 1 and dq, dk are exactly zero in float64:
    dq[q] = scale * sum_j P (dP - delta) k[j] and dk[j] = scale * sum_q P (dP - delta) q[q], with
    dP = delta = sum_d dout * v.  A float32 result is the rounding of those differences, so the scale the gate's "one
    ulp" refers to is that of the terms that cancel, T[q,j] = sum_d |dout[q,d]| |v[j,d]|:
    dq: scale * max_q sum_j T max|k|,  dk: scale * max_j sum_q T max|q|.  (out and dv are never identically zero.)"""
    B, H, Nq, D = inp["q"].shape
    g = inp["dout"].double().reshape(B, Nq, H, D).transpose(1, 2).abs()
    T = g @ inp["v"].double().abs().transpose(-2, -1)                    # [B,H,Nq,Nk]
    return [None, float(scale * T.sum(-1).max() * inp["k"].abs().max()),
            float(scale * T.sum(-2).max() * inp["q"].abs().max()), None]


def gate(label, got, eager, x64, inp):
    zs = cancel_scales(inp)
    e_got, e_eager = errs(got, x64, zs), errs(eager, x64, zs)
    for n, a, b in zip(NAMES, e_got, e_eager):
        print(f"{label} {n}: product {a:.3e} eager {b:.3e} bound {2 * b + EPS:.3e}")
    for g in got:
        assert torch.isfinite(g).all()
    for n, a, b in zip(NAMES, e_got, e_eager):
        assert a <= 2 * b + EPS, (label, n, a, b)


_REF = {}


def reference(name):
    """The float64 oracle and the eager float32 evaluation on the device of one case: computed once, never modified."""
    if name not in _REF:
        inp = make_inputs(name)
        x64 = oracle.core_with_grads(inp["q"], inp["k"], inp["v"], inp["qpos"], inp["kpos"], inp["dout"])
        eager = oracle.core_with_grads(inp["q"].to(DEV), inp["k"].to(DEV), inp["v"].to(DEV), inp["qpos"].to(DEV),
                                       inp["kpos"].to(DEV), inp["dout"].to(DEV), dtype=torch.float32)
        _REF[name] = (inp, x64, eager)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_against_oracle(name):
    inp, x64, eager = reference(name)
    got = run_product(inp, packed=CASES[name][3] is None)
    gate(name, got, eager, x64, inp)


@pytest.mark.parametrize("name", ["packed_2x3x70", "packed_1x2x64"])
def test_packed_equals_three_views_bitwise(name):
    import spfsplatv2_amd as spf
    inp, _, _ = reference(name)
    out_p, dq_p, dk_p, dv_p = run_product(inp, packed=True)
    qkv = inp["qkv"].to(DEV).requires_grad_(True)
    t = qkv.transpose(1, 3)
    pos = inp["qpos"].to(DEV)
    out = spf.rope_attention(t[:, :, 0], t[:, :, 1], t[:, :, 2], pos, pos)
    (g,) = torch.autograd.grad(out, (qkv,), inp["dout"].to(DEV))
    assert torch.equal(out, out_p)
    gt = g.transpose(1, 3)
    assert torch.equal(gt[:, :, 0], dq_p) and torch.equal(gt[:, :, 1], dk_p) and torch.equal(gt[:, :, 2], dv_p)


@pytest.mark.parametrize("name", ["packed_2x3x70", "cross_2x2x66_131"])
def test_strided_inputs_are_read_in_place(name):
    from spfsplatv2_amd import attention
    inp, _, _ = reference(name)
    base = inp["qkv"].to(DEV) if inp["qkv"] is not None else None
    if base is not None:
        t = base.transpose(1, 3)
        q, k, v = t[:, :, 0], t[:, :, 1], t[:, :, 2]
    else:
        q, k, v = (inp[n].permute(0, 2, 1, 3).contiguous().to(DEV).permute(0, 2, 1, 3) for n in "qkv")
    for t in (q, k, v):
        assert not t.is_contiguous()
        assert attention._rows(t) is t and attention._rows(t).data_ptr() == t.data_ptr()      # no copy
    strided = run_product({**inp, "q": q, "k": k, "v": v}, packed=False)
    dense = run_product({**inp, "q": q.contiguous(), "k": k.contiguous(), "v": v.contiguous()}, packed=False)
    for n, a, b in zip(NAMES, strided, dense):
        assert torch.equal(a, b), n


@pytest.mark.parametrize("where", ["first_tile", "last_tile"])
def test_extreme_logits(where):
    """Logits spread over [-80, 80]; the row maximum sits in the first or in the last (partly padded) key tile."""
    B, H, Nq, Nk = 1, 2, 40, 70
    gen = torch.Generator().manual_seed(5)
    u = torch.randn(64, generator=gen)
    u /= u.norm()
    beta = torch.linspace(-80, 78, Nk)[torch.randperm(Nk, generator=gen)]
    peak = 3 if where == "first_tile" else Nk - 2
    beta[peak] = 80.0
    q = (8.0 * u + 0.05 * torch.randn(B, H, Nq, 64, generator=gen))
    k = beta[None, None, :, None] * u + 0.05 * torch.randn(B, H, Nk, 64, generator=gen)
    v = torch.randn(B, H, Nk, 64, generator=gen)
    inp = {"q": q, "k": k, "v": v, "qpos": None, "kpos": None, "dout": torch.randn(B, Nq, H * 64, generator=gen)}
    x64 = oracle.core_with_grads(q, k, v, None, None, inp["dout"])
    s = (q.double() @ k.double().transpose(-2, -1)) * 0.125
    assert s.max() > 79 and s.min() < -79 and (s.argmax(-1) == peak).all()
    eager = oracle.core_with_grads(q.to(DEV), k.to(DEV), v.to(DEV), None, None, inp["dout"].to(DEV), dtype=torch.float32)
    got = run_product(inp, packed=False, rope=False)
    gate("extreme_" + where, got, eager, x64, inp)


def test_back_to_back_calls_are_bit_identical():
    inp, _, _ = reference("cross_2x2x66_131")
    runs = [run_product(inp, packed=False) for _ in range(10)]       # nothing synchronises in between
    for r in runs[1:]:
        for n, a, b in zip(NAMES, runs[0], r):
            assert torch.equal(a, b), n


def _ulps(a, b):
    """distance in units of the last place between two tensors of one 16-bit float type"""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs().max().item()


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", ["packed_2x3x70", "cross_2x2x66_131"])
def test_sixteen_bit_types_follow_the_float32_path(name, dtype):
    """One compute path: the 16-bit kernels' results are the float32 kernels' results on the upcast operands, rounded.
    (The backward is given the same saved output and log-sum-exp in both runs: they are its operands too.)"""
    from spfsplatv2_amd import attention
    inp = make_inputs(name, dtype)
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


@pytest.fixture(scope="module")
def goldens(golden_dir):
    cases = dict(torch.load(golden_dir / "attention_goldens.pt", weights_only=True))
    cases.update(torch.load(golden_dir / "attention_goldens_cross.pt", weights_only=True))
    return cases


@pytest.mark.parametrize("name", ["self_2x3x70", "cross_2x2x66_131", "self_norope_1x1x5"])
def test_modules_against_the_reference_goldens(goldens, name):
    """Our modules with the reference's weights against the reference's float32 outputs and input gradients: our
    distance to the float64 oracle may be twice the golden's own (the reference's float32 run) plus one ulp."""
    import spfsplatv2_amd as spf
    case = goldens[name]
    x64_out, x64_grads = oracle.golden_case(case)
    rope = spf.cuRoPE2D(case["base"], 1.0) if case["base"] is not None else None
    dim = next(iter(case["weights"].values())).shape[-1]
    ins = {k: case[k].to(DEV).requires_grad_(True) for k in case["inputs"]}
    if case["kind"] == "self":
        mod = spf.Attention(dim, rope=rope, num_heads=case["num_heads"], qkv_bias=True).to(DEV)
        mod.load_state_dict(case["weights"])
        out = mod(ins["x"], case["xpos"].to(DEV))
    else:
        mod = spf.CrossAttention(dim, rope=rope, num_heads=case["num_heads"], qkv_bias=True).to(DEV)
        mod.load_state_dict(case["weights"])
        out = mod(ins["query"], ins["memory"], ins["memory"], case["qpos"].to(DEV), case["kpos"].to(DEV))
    grads = torch.autograd.grad(0.5 * (out * out).sum(), list(ins.values()))
    pairs = [("out", out, case["out"], x64_out)] + [(k, g, case["grads"][k], x64_grads[k]) for k, g in zip(ins, grads)]
    figures = []
    for n, got, gold, x64 in pairs:
        e_got, e_gold = errs([got], [x64])[0], errs([gold], [x64])[0]
        print(f"{name} {n}: product {e_got:.3e} golden {e_gold:.3e} bound {2 * e_gold + EPS:.3e}")
        figures.append((n, e_got, e_gold))
    for n, e_got, e_gold in figures:
        assert e_got <= 2 * e_gold + EPS, (name, n, e_got, e_gold)
