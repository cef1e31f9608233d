"""VGGT attention on the device: the fused kernels with an additive mask and the q / k LayerNorm against the float64
oracle (tests/vggt_attention_oracle.py) and the reference's goldens; -inf handling, mask layouts, LayerNorm edges,
bitwise properties and the 16-bit types.

The gate is test_gpu_attention.py's (imported): per tensor err = max|x - x64| / max|x64| must not exceed twice the err
of the reference's expression evaluated eagerly in float32 on the same device and inputs plus one float32 ulp.  It
covers out, dq, dk, dv and the gradients of the four norm parameters.  Two tensors are identically zero in exact
arithmetic in some cases and are then measured against the magnitude of the terms that cancel: dq / dk with a single
key (cancel_scales, as before) and the k bias' gradient without a rotation (oracle.k_bias_cancel_scale).
"""
import pytest
import torch

from tests import vggt_attention_oracle as oracle
from tests.test_gpu_attention import DEV, EPS, _ulps, cancel_scales, errs, grid_positions

pytestmark = pytest.mark.gpu

NAMES = ("out", "dq", "dk", "dv", "dq_weight", "dq_bias", "dk_weight", "dk_bias")
NORM_EPS = 1e-5
NEG = float("-inf")


def _self_case(B, H, S, hh, ww, special):
    return {"B": B, "H": H, "qpos": oracle.view_positions(B, S, hh, ww, special), "kpos": None, "S": S}


# name -> layout; packed self-attention unless kpos is given
CASES = {
    "views_3x23": _self_case(2, 2, 3, 4, 5, 3),              # view boundaries 23, 46 inside key tiles, last tile partial
    "first_tiles_masked": _self_case(2, 2, 3, 6, 6, 4),      # P = 40: the last view's rows do not see keys 0 .. 39
    "global_3x262": _self_case(1, 2, 3, 16, 16, 6),          # N = 786: 7 owner blocks, 25 key tiles, rows of 3,144 bytes
    "frame_3x12x258": {"B": 3, "H": 12, "qpos": grid_positions(3, 16, 16, 2), "kpos": None, "S": 1},
    "cross_66_131": {"B": 2, "H": 2, "qpos": grid_positions(2, 8, 8, 2), "kpos": grid_positions(2, 13, 10, 1), "S": 1},
}


def make_inputs(name, dtype=torch.float32):
    c = CASES[name]
    B, H, qpos = c["B"], c["H"], c["qpos"]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    Nq = qpos.shape[1]
    if c["kpos"] is None:
        qkv = torch.randn(B, Nq, 3, H, 64, generator=gen).to(dtype)
        t = qkv.transpose(1, 3)
        q, k, v, kpos = t[:, :, 0], t[:, :, 1], t[:, :, 2], qpos
    else:
        kpos, qkv = c["kpos"], None
        q, k, v = (torch.randn(B, n, H, 64, generator=gen).to(dtype).permute(0, 2, 1, 3)
                   for n in (Nq, kpos.shape[1], kpos.shape[1]))
    dout = torch.randn(B, Nq, H * 64, generator=gen).to(dtype)
    params = [1.0 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen),
              1.0 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen)]
    return {"qkv": qkv, "q": q, "k": k, "v": v, "qpos": qpos, "kpos": kpos, "dout": dout, "params": params,
            "gen": gen}


def case_mask(name):
    """The mask of a case (None: the case has none)."""
    c = CASES[name]
    N = c["qpos"].shape[1]
    if name in ("views_3x23", "global_3x262"):
        return oracle.view_mask(3, N // 3, 1)
    if name == "first_tiles_masked":
        m = torch.zeros(1, 1, N, N)
        m[..., 2 * (N // 3):, :N // 3] = NEG
        return m
    return None


def norms_of(inp):
    p = inp["params"]
    return (p[0], p[1], NORM_EPS), (p[2], p[3], NORM_EPS)


def every_row_has_a_key(mask, shape, but=()):
    """CPU check on the inputs: every query row keeps at least one key, except the rows listed in `but`."""
    alive = (mask.expand(shape) > NEG if mask.dtype != torch.bool else mask.expand(shape)).any(-1)
    want = torch.ones_like(alive)
    for row in but:
        want[..., row] = False
    return bool((alive == want).all())


def run_product(inp, packed, rope=True, mask=None, norm=True):
    """(out, dq, dk, dv, dq_weight, dq_bias, dk_weight, dk_bias) of the product on the device (the last four None
    without the norms); packed: through rope_attention_packed and its one gradient."""
    import spfsplatv2_amd as spf
    qpos = inp["qpos"].to(DEV) if rope else None
    kpos = inp["kpos"].to(DEV) if rope else None
    dout = inp["dout"].to(DEV)
    params = [p.to(DEV).requires_grad_(True) for p in inp["params"]] if norm else []
    kw = {"mask": mask.to(DEV) if mask is not None else None}
    if norm:
        kw.update(q_norm=(params[0], params[1], NORM_EPS), k_norm=(params[2], params[3], NORM_EPS))
    if packed:
        qkv = inp["qkv"].to(DEV).requires_grad_(True)
        out = spf.rope_attention_packed(qkv, qpos, **kw)
        g = torch.autograd.grad(out, [qkv] + params, dout)
        assert g[0].shape == qkv.shape
        gt = g[0].transpose(1, 3)
        grads = (gt[:, :, 0], gt[:, :, 1], gt[:, :, 2]) + tuple(g[1:])
    else:
        q, k, v = (inp[n].to(DEV).requires_grad_(True) for n in "qkv")
        out = spf.rope_attention(q, k, v, qpos, kpos, **kw)
        grads = tuple(torch.autograd.grad(out, [q, k, v] + params, dout))
    return (out.detach(),) + grads + (None,) * (7 - len(grads))


def references(inp, rope=True, mask=None, norm=True):
    """(float64 oracle on the CPU, the same expression eagerly in float32 on the device, zero scales)."""
    qn, kn = norms_of(inp) if norm else (None, None)
    qpos, kpos = (inp["qpos"], inp["kpos"]) if rope else (None, None)
    probe = {}
    x64 = oracle.core_with_grads(inp["q"], inp["k"], inp["v"], qpos, kpos, inp["dout"], mask, qn, kn, probe=probe)
    dev = lambda t: None if t is None else t.to(DEV)
    dn = lambda n: None if n is None else (n[0].to(DEV), n[1].to(DEV), n[2])
    eager = oracle.core_with_grads(dev(inp["q"]), dev(inp["k"]), dev(inp["v"]), dev(qpos), dev(kpos), dev(inp["dout"]),
                                   dev(mask), dn(qn), dn(kn), dtype=torch.float32)
    zs = cancel_scales(inp) + [None] * 4
    kb = oracle.k_bias_cancel_scale(probe) if (norm and not rope) else None
    return x64, eager, zs, kb


def gate(label, got, eager, x64, zs, kb=None):
    """test_gpu_attention.gate for the eight tensors (those a case does not have are None on all three sides); kb: the
    scale the k bias' gradient is measured against where it is identically zero (no rotation)."""
    idx = [i for i, w in enumerate(x64) if w is not None]
    assert all((got[i] is None) == (x64[i] is None) for i in range(8))
    pick = lambda t: [t[i] for i in idx]
    if kb is not None:                                  # measured against kb: err = max|x - x64| / kb
        x64 = list(x64)
        zs = list(zs)
        zs[7] = kb
        shift = x64[7]
        got, eager = list(got), list(eager)
        got[7], eager[7], x64[7] = got[7].double().cpu() - shift, eager[7].double().cpu() - shift, torch.zeros_like(shift)
    e_got, e_eager = errs(pick(got), pick(x64), pick(zs)), errs(pick(eager), pick(x64), pick(zs))
    for i, a, b in zip(idx, e_got, e_eager):
        print(f"{label} {NAMES[i]}: product {a:.3e} eager {b:.3e} bound {2 * b + EPS:.3e}")
    for g in pick(got):
        assert torch.isfinite(g).all()
    for i, a, b in zip(idx, e_got, e_eager):
        assert a <= 2 * b + EPS, (label, NAMES[i], a, b)


_REF = {}


def reference(name):
    """Inputs, mask and references of a named case with everything on: computed once, never modified."""
    if name not in _REF:
        inp, mask = make_inputs(name), case_mask(name)
        _REF[name] = (inp, mask) + references(inp, True, mask, True)
    return _REF[name]


@pytest.mark.parametrize("name", ["views_3x23", "first_tiles_masked", "global_3x262", "frame_3x12x258"])
def test_forward_and_gradients_against_oracle(name):
    inp, mask, x64, eager, zs, kb = reference(name)
    if mask is not None:
        assert every_row_has_a_key(mask, (1, 1) + tuple(mask.shape[-2:]))
    if name == "first_tiles_masked":                    # the first whole key tile is -inf for the last view's rows
        assert (mask[0, 0, 80:, :32] == NEG).all() and (mask[0, 0, 80:, 40:] == 0).all()
    gate(name, run_product(inp, packed=True, mask=mask), eager, x64, zs, kb)


def test_row_fully_masked():
    """One row without any key: out and dq of that row are exactly 0, everything is finite, and everything meets the
    gate against the oracle's definition (that row is zeros)."""
    inp, mask, _, _, _, _ = reference("views_3x23")
    row = 50
    mask = mask.clone()
    mask[..., row, :] = NEG
    assert every_row_has_a_key(mask, (1, 1, 69, 69), but=(row,))
    x64, eager, zs, kb = references(inp, True, mask, True)
    got = run_product(inp, packed=True, mask=mask)
    B, H = inp["q"].shape[:2]
    assert (got[0].reshape(B, 69, H, 64)[:, row] == 0).all() and (got[1][:, :, row] == 0).all()
    assert (x64[0].reshape(B, 69, H, 64)[:, row] == 0).all() and (x64[1][:, :, row] == 0).all()
    gate("row_fully_masked", got, eager, x64, zs, kb)


@pytest.mark.parametrize("shape", ["B1QK", "1HQK", "QK"])
def test_finite_bias(shape):
    """Random finite additive masks through every stride pattern (0 included), Nq != Nk."""
    inp = make_inputs("cross_66_131")
    B, H, Nq, Nk = 2, 2, 66, 131
    dims = {"B1QK": (B, 1, Nq, Nk), "1HQK": (1, H, Nq, Nk), "QK": (Nq, Nk)}[shape]
    mask = 2.0 * torch.randn(dims, generator=torch.Generator().manual_seed(len(shape)))
    x64, eager, zs, kb = references(inp, True, mask, True)
    gate("finite_bias_" + shape, run_product(inp, packed=False, mask=mask), eager, x64, zs, kb)


@pytest.mark.parametrize("rope", [True, False])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("masked", [True, False])
def test_flag_cross(masked, norm, rope):
    inp, mask, _, _, _, _ = reference("views_3x23")
    mask = mask if masked else None
    x64, eager, zs, kb = references(inp, rope, mask, norm)
    got = run_product(inp, packed=True, rope=rope, mask=mask, norm=norm)
    gate(f"flags mask={masked} norm={norm} rope={rope}", got, eager, x64, zs, kb)


@pytest.mark.parametrize("edge", ["constant_row", "offset_rows"])
def test_layernorm_edges(edge):
    """A constant row (variance 0, rstd = eps^-1/2) and rows with mean 1e3 and unit spread (E[x^2] - mean^2 would lose
    every digit of the variance there)."""
    inp, mask, _, _, _, _ = reference("views_3x23")
    inp = dict(inp)
    qkv = inp["qkv"].clone()
    if edge == "constant_row":
        qkv[0, 5, 0, 1] = 0.75                          # one q row and one k row
        qkv[1, 40, 1, 0] = -2.0
    else:
        qkv[:, :, :2] += 1e3
    t = qkv.transpose(1, 3)
    inp.update(qkv=qkv, q=t[:, :, 0], k=t[:, :, 1], v=t[:, :, 2])
    x64, eager, zs, kb = references(inp, True, mask, True)
    gate(edge, run_product(inp, packed=True, mask=mask), eager, x64, zs, kb)


def _same(a, b):
    for n, x, y in zip(NAMES, a, b):
        assert torch.equal(x, y), n


def test_bool_mask_equals_its_float_twin_bitwise():
    inp, mask, _, _, _, _ = reference("views_3x23")
    mask = mask.clone()
    mask[..., 50, :] = NEG                              # (with an empty row too)
    _same(run_product(inp, packed=True, mask=mask), run_product(inp, packed=True, mask=mask == 0))
    inp = make_inputs("cross_66_131")
    keep = torch.rand(2, 1, 66, 131, generator=torch.Generator().manual_seed(1)) < 0.7
    assert every_row_has_a_key(keep, (2, 1, 66, 131))
    _same(run_product(inp, packed=False, mask=torch.where(keep, 0.0, NEG)), run_product(inp, packed=False, mask=keep))


@pytest.mark.parametrize("norm", [True, False])
def test_zero_mask_equals_no_mask_bitwise(norm):
    inp, _, _, _, _, _ = reference("views_3x23")
    a = run_product(inp, packed=True, mask=torch.zeros(1, 1, 69, 69), norm=norm)
    b = run_product(inp, packed=True, mask=None, norm=norm)
    for n, x, y in zip(NAMES, a, b):
        assert (x is None and y is None) or torch.equal(x, y), n


def test_packed_equals_three_views_bitwise():
    inp, mask, _, _, _, _ = reference("views_3x23")
    _same(run_product(inp, packed=True, mask=mask), run_product(inp, packed=False, mask=mask))


def test_back_to_back_calls_are_bit_identical():
    inp, mask, _, _, _, _ = reference("global_3x262")
    runs = [run_product(inp, packed=True, mask=mask) for _ in range(10)]       # nothing synchronises in between
    for r in runs[1:]:
        _same(runs[0], r)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", ["views_3x23", "cross_66_131"])
def test_sixteen_bit_types_follow_the_float32_path(name, dtype):
    """One compute path: the 16-bit kernels' results are the float32 kernels' results on the upcast operands, rounded;
    the mask and the parameters are float32 in both runs."""
    from spfsplatv2_amd import attention
    inp = make_inputs(name, dtype)
    q, k, v, dout = (inp[n].to(DEV) for n in ("q", "k", "v", "dout"))
    qpos, kpos = inp["qpos"].to(DEV), inp["kpos"].to(DEV)
    mask = case_mask(name)
    if mask is None:
        mask = 2.0 * torch.randn(2, 1, 66, 131, generator=inp["gen"])
    p = [t.to(DEV) for t in inp["params"]]
    kw = {"mask": mask.to(DEV), "q_norm": (p[0], p[1], NORM_EPS), "k_norm": (p[2], p[3], NORM_EPS)}
    cfg = (100.0, 1.0, 0.125)
    out16, lse16 = attention.attention_forward(q, k, v, qpos, kpos, *cfg, **kw)
    out32, lse32 = attention.attention_forward(q.float(), k.float(), v.float(), qpos, kpos, *cfg, **kw)
    assert out16.dtype == dtype and torch.equal(lse16, lse32)
    assert _ulps(out16, out32.to(dtype)) <= 1

    def backward(q, k, v, out, dout):
        g = [torch.empty(t.shape, dtype=t.dtype, device=DEV) for t in (q, k, v)]
        return g, attention.attention_backward(q, k, v, qpos, kpos, *cfg, out, lse16, dout, *g, **kw)
    g16, n16 = backward(q, k, v, out16, dout)
    g32, n32 = backward(q.float(), k.float(), v.float(), out16.float(), dout.float())
    for n, a, b in zip(NAMES[1:], g16, g32):
        assert a.dtype == dtype and torch.isfinite(a).all()
        assert _ulps(a, b.to(dtype)) <= 1, n
    # both float32, the same terms in the same order; the compiler may fuse a multiply-add in one instantiation and not
    # in the other, which moves a term by an ulp: 16 ulp of each gradient's scale
    assert n16.dtype == torch.float32 and n16.shape == (4, 64)
    for i in range(4):
        assert float((n16[i] - n32[i]).abs().max()) <= 16 * EPS * float(n32[i].abs().max()), NAMES[4 + i]


@pytest.fixture(scope="module")
def gold(golden_dir):
    return torch.load(golden_dir / "vggt_attention_goldens.pt", weights_only=True)


@pytest.mark.parametrize("name", ["mask_rope", "rope", "mask"])
def test_module_against_the_reference_goldens(gold, name):
    """VGGTAttention with the reference's weights against the reference's float32 outputs and gradients: our distance
    to the float64 oracle may be twice the golden's own plus one ulp (test_modules_against_the_reference_goldens'
    rule), for the output, the input gradient and the gradients of the norm parameters and the biases."""
    import spfsplatv2_amd as spf
    case, probe = gold["cases"][name], {}
    x64_out, x64_dx, x64_dp = oracle.golden_case(gold, name, probe=probe)
    rope = spf.RotaryPositionEmbedding2D(gold["base"]) if case["rope"] else None
    mod = spf.VGGTAttention(128, num_heads=gold["num_heads"], qk_norm=True, rope=rope).to(DEV)
    mod.load_state_dict(gold["weights"])
    x = gold["x"].to(DEV).requires_grad_(True)
    out = mod(x, gold["pos"].to(DEV) if case["rope"] else None, gold["mask"].to(DEV) if case["mask"] else None)
    (0.5 * (out * out).sum()).backward()
    params = dict(mod.named_parameters())
    pairs = [("out", out, case["out"], x64_out, None), ("dx", x.grad, case["dx"], x64_dx, None)]
    for k, g in case["dparams"].items():
        den = oracle.k_bias_cancel_scale(probe) if (k == "k_norm.bias" and not case["rope"]) else None
        pairs.append((k, params[k].grad, g, x64_dp[k], den))
    figures = []
    for n, got, golden, x64, den in pairs:
        den = float(x64.abs().max()) if den is None else den
        e_got = float((got.detach().double().cpu() - x64).abs().max()) / den
        e_gold = float((golden.double() - x64).abs().max()) / den
        print(f"{name} {n}: product {e_got:.3e} golden {e_gold:.3e} bound {2 * e_gold + EPS:.3e}")
        figures.append((n, e_got, e_gold))
    for n, e_got, e_gold in figures:
        assert e_got <= 2 * e_gold + EPS, (name, n, e_got, e_gold)


def test_selective_gradients_are_the_all_grad_run_bitwise():
    """Only some inputs require grad: each gradient that is asked for is bitwise what the run with everything requiring
    grad returns, in its own slot, and nothing else gets one.  N = 33: one owner block, partly empty, and two key tiles,
    the second with one key; unpacked 33 queries on 40 keys."""
    import spfsplatv2_amd as spf
    B, H, N, Nk = 1, 2, 33, 40
    gen = torch.Generator().manual_seed(3340)
    qkv0 = torch.randn(B, N, 3, H, 64, generator=gen)
    q0, k0, v0 = (torch.randn(B, n, H, 64, generator=gen).permute(0, 2, 1, 3) for n in (N, Nk, Nk))
    qpos, kpos = (torch.randint(0, 8, (B, n, 2), generator=gen).to(DEV) for n in (N, Nk))
    dout = torch.randn(B, N, H * 64, generator=gen).to(DEV)
    params0 = [1.0 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen),
               1.0 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen)]

    def band(nk):                                       # keys 3 .. 8 past the row's own index are excluded
        d = torch.arange(nk)[None, :] - torch.arange(N)[:, None]
        m = torch.where((d >= 3) & (d < 9), NEG, 0.0)
        assert every_row_has_a_key(m, (N, nk)) and int((m == NEG).sum()) >= 4 * N
        return m.to(DEV)

    def leaves(tensors, need):
        return [t.to(DEV).requires_grad_(r) for t, r in zip(tensors, need)]

    def norms(p):
        return {"q_norm": (p[0], p[1], NORM_EPS), "k_norm": (p[2], p[3], NORM_EPS)}

    def packed(need_params):
        (qkv,), p = leaves([qkv0], [True]), leaves(params0, need_params)
        spf.rope_attention_packed(qkv, qpos, mask=band(N), **norms(p)).backward(dout)
        return qkv.grad, [t.grad for t in p]

    base, base_p = packed([True] * 4)
    assert all(g is not None for g in base_p)
    some, some_p = packed([False, False, False, True])
    assert torch.equal(some, base) and torch.equal(some_p[3], base_p[3])
    assert some_p[0] is None and some_p[1] is None and some_p[2] is None

    def unpacked(need, need_params):
        t, p = leaves([q0, k0, v0], need), leaves(params0, need_params)
        spf.rope_attention(*t, qpos, kpos, mask=band(Nk), **norms(p)).backward(dout)
        return [x.grad for x in t]

    base = unpacked([True] * 3, [True] * 4)
    some = unpacked([False, True, False], [False] * 4)
    assert torch.equal(some[1], base[1]) and some[0] is None and some[2] is None

    def plain(need):
        t = leaves([q0, k0, v0], need)
        spf.rope_attention(*t, qpos, kpos).backward(dout)
        return [x.grad for x in t]

    base = plain([True] * 3)
    some = plain([False, False, True])
    assert torch.equal(some[2], base[2]) and some[0] is None and some[1] is None
