"""Multi-view attention on the device: one key set per scene read in place, whole views left out per query view.

Gate (tests/test_gpu_attention.py's rule): per tensor out, dq, dk, dv, err = max|x - x64| / max|x64| against the float64
oracle ON GATHERED KEYS (tests/attention_views_oracle.py: the reference's expression per query view on the allowed
views' tokens side by side; the gradient of a key view is the sum of its gathered copies' gradients) must not exceed
twice the err of the same oracle evaluated in float32 on the device, plus 2^-23.  Every figure is printed
(profiles/attention_views_gate_figures.txt holds one run's).
"""
import pytest
import torch

from tests import attention_views_oracle as voracle
from tests.test_gpu_attention import DEV, EPS, _ulps, errs, grid_positions

pytestmark = pytest.mark.gpu

NAMES = ("out", "dq", "dk", "dv")


def _blk2(v, nt):
    import spfsplatv2_amd as spf
    return spf.decoder_view_sets(v, nt)[1].allow.tolist()


# name: (b, H, Vq, Vk, Nq grid, Nk grid, allow); grids as grid_positions takes them (rows, columns, extra tokens)
CASES = {
    "smallest_1x1_1v2_1_1": (1, 1, 1, 2, (1, 1, 0), (1, 1, 0), lambda: [[1, 1]]),
    "ragged_2x2_2v3_66_70": (2, 2, 2, 3, (8, 8, 2), (17, 4, 2), lambda: [[s != i + 1 for s in range(3)] for i in range(2)]),
    "blk2_1x2_3v4_33_33": (1, 2, 3, 4, (4, 8, 1), (4, 8, 1), lambda: _blk2(4, 1)),
    "short_views_1x1_2v3_129_5": (1, 1, 2, 3, (8, 16, 1), (1, 5, 0), lambda: [[0, 1, 1], [1, 1, 1]]),
    "whole_tiles_1x1_2v3_8_64": (1, 1, 2, 3, (2, 4, 0), (8, 8, 0), lambda: [[0, 1, 0], [0, 0, 1]]),
    "decoder_1x12_2v3_258_258": (1, 12, 2, 3, (16, 16, 2), (16, 16, 2), lambda: _blk2(3, 1)),
}
RAGGED, WHOLE = "ragged_2x2_2v3_66_70", "whole_tiles_1x1_2v3_8_64"


def make_inputs(name, dtype=torch.float32):
    """q is the [:, 1:] slice of a token-major buffer with one view more (what a projection of all views gives the
    second decoder block), k and v token-major buffers: all three are strided views the kernels read in place."""
    b, H, Vq, Vk, qg, kg, allow = CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    qpos = grid_positions(b * Vq, *qg).reshape(b, Vq, -1, 2)
    kpos = grid_positions(b * Vk, *kg).reshape(b, Vk, -1, 2)
    Nq, Nk = qpos.shape[2], kpos.shape[2]
    q_all = torch.randn(b, Vq + 1, Nq, H, 64, generator=gen).to(dtype)
    k = torch.randn(b, Vk, Nk, H, 64, generator=gen).to(dtype).transpose(2, 3)
    v = torch.randn(b, Vk, Nk, H, 64, generator=gen).to(dtype).transpose(2, 3)
    dout = torch.randn(b, Vq, Nq, H * 64, generator=gen).to(dtype)
    return {"q_all": q_all, "q": q_all[:, 1:].transpose(2, 3), "k": k, "v": v, "qpos": qpos, "kpos": kpos, "dout": dout,
            "allow": [[bool(x) for x in row] for row in allow()]}


def to_device(inp):
    d = {n: (t.to(DEV) if isinstance(t, torch.Tensor) else t) for n, t in inp.items()}
    d["q"] = d["q_all"][:, 1:].transpose(2, 3)                      # the slice of the DEVICE buffer, not a copy of the view
    return d


def run_product(inp, rope=True):
    """(out, dq, dk, dv) of rope_attention_views on the device."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import attention
    d = to_device(inp)
    for t in (d["q"], d["k"], d["v"]):
        assert attention._rows5(t) is t                             # read in place: no copy
    q, k, v = (d[n].requires_grad_(True) for n in "qkv")
    out = spf.rope_attention_views(q, k, v, d["qpos"] if rope else None, d["kpos"] if rope else None, allow=inp["allow"])
    return (out.detach(),) + tuple(torch.autograd.grad(out, (q, k, v), d["dout"]))


def oracle_pair(inp, rope=True):
    """(float64 on the CPU, float32 on the device) of the oracle on gathered keys."""
    qpos, kpos = (inp["qpos"], inp["kpos"]) if rope else (None, None)
    x64 = voracle.core_views_with_grads(inp["q"], inp["k"], inp["v"], qpos, kpos, inp["allow"], inp["dout"])
    d = to_device(inp)
    eager = voracle.core_views_with_grads(d["q"], d["k"], d["v"], d["qpos"] if rope else None, d["kpos"] if rope else None,
                                          inp["allow"], d["dout"], dtype=torch.float32)
    return x64, eager


def gate(label, got, eager, x64, names=NAMES):
    e_got, e_eager = errs(got, x64), errs(eager, x64)
    for n, a, b in zip(names, e_got, e_eager):
        print(f"{label} {n}: product {a:.3e} eager {b:.3e} bound {2 * b + EPS:.3e}")
    for g in got:
        assert torch.isfinite(g).all()
    for n, a, b in zip(names, e_got, e_eager):
        assert a <= 2 * b + EPS, (label, n, a, b)


_REF = {}


def reference(name):
    """Inputs, float64 oracle and eager float32 evaluation of one case: computed once, never modified."""
    if name not in _REF:
        inp = make_inputs(name)
        _REF[name] = (inp,) + oracle_pair(inp)
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_against_oracle_on_gathered_keys(name):
    inp, x64, eager = reference(name)
    b, H, Vq, Vk, _, _, _ = CASES[name]
    got = run_product(inp)
    assert tuple(got[0].shape) == (b, Vq, inp["q"].shape[3], H * 64)
    assert got[2].shape == inp["k"].shape and got[3].shape == inp["v"].shape
    gate(name, got, eager, x64)


def test_a_key_view_nobody_reads_gets_exact_zeros():
    """Key view 0 of the whole-tiles case is read by no query view: its dk and dv rows are WRITTEN, as zeros."""
    from spfsplatv2_amd import attention
    inp, x64, _ = reference(WHOLE)
    assert not any(row[0] for row in inp["allow"]) and float(x64[2][:, 0].abs().max()) == 0.0
    d = to_device(inp)
    words, _, _ = attention.allow_words(inp["allow"])
    cfg = (words, 100.0, 1.0, 0.125)
    out, lse = attention.attention_views_forward(d["q"], d["k"], d["v"], d["qpos"], d["kpos"], *cfg)
    g = [torch.full(t.shape, float("nan"), device=DEV) for t in (d["q"], d["k"], d["v"])]
    attention.attention_views_backward(d["q"], d["k"], d["v"], d["qpos"], d["kpos"], *cfg, out, lse, d["dout"], *g)
    for n, t in zip(NAMES[1:], g):
        assert torch.isfinite(t).all(), n
    assert (g[1][:, 0] == 0).all() and (g[2][:, 0] == 0).all()
    assert float(g[1][:, 1].abs().max()) > 0 and float(g[2][:, 2].abs().max()) > 0
    _, dq, dk, dv = run_product(inp)
    assert (dk[:, 0] == 0).all() and (dv[:, 0] == 0).all()
    assert torch.equal(dk, g[1]) and torch.equal(dv, g[2]) and torch.equal(dq, g[0])


@pytest.mark.parametrize("where", ["first_tile_after_a_skipped_view", "last_padded_tile_of_the_last_view"])
def test_extreme_logits(where):
    """Logits spread over [-80, 80] (tests/test_gpu_attention.py::test_extreme_logits) over the keys of three views of 70
    tokens; query view 0 skips key view 1, query view 1 skips key view 0.  The row maximum sits in key view 2: in its
    first tile, which for query view 0 is the tile the prefetch reaches by hopping over view 1, or in its last tile,
    which is padded (keys 64 .. 69 of 70) and ends the walk of both query views."""
    b, H, Vq, Vk, Nq, Nk = 1, 2, 2, 3, 40, 70
    allow = [[True, False, True], [False, True, True]]
    gen = torch.Generator().manual_seed(5)
    u = torch.randn(64, generator=gen)
    u /= u.norm()
    beta = torch.linspace(-80, 78, Vk * Nk)[torch.randperm(Vk * Nk, generator=gen)].reshape(Vk, Nk)
    peak = 3 if where.startswith("first") else Nk - 2
    beta[2, peak] = 80.0
    beta[2, 40] = -80.0                                             # (both ends of the range in a view both query views read)
    q_all = 8.0 * u + 0.05 * torch.randn(b, Vq + 1, Nq, H, 64, generator=gen)
    k = (beta[None, :, :, None, None] * u + 0.05 * torch.randn(b, Vk, Nk, H, 64, generator=gen)).transpose(2, 3)
    v = torch.randn(b, Vk, Nk, H, 64, generator=gen).transpose(2, 3)
    inp = {"q_all": q_all, "q": q_all[:, 1:].transpose(2, 3), "k": k, "v": v, "qpos": None, "kpos": None,
           "dout": torch.randn(b, Vq, Nq, H * 64, generator=gen), "allow": allow}
    for i in range(Vq):
        idx = voracle.allowed(allow, i)
        kg = k.index_select(1, idx).transpose(1, 2).flatten(2, 3).double()
        s = (inp["q"][:, i].double() @ kg.transpose(-2, -1)) * 0.125
        assert s.max() > 79 and s.min() < -79 and (s.argmax(-1) == (len(idx) - 1) * Nk + peak).all()
    inp["qpos"] = inp["kpos"] = torch.zeros(0)                      # (to_device moves tensors; unused without rope)
    x64, eager = oracle_pair(inp, rope=False)
    got = run_product(inp, rope=False)
    gate("extreme_" + where, got, eager, x64)


def test_back_to_back_calls_are_bit_identical():
    inp, _, _ = reference(RAGGED)
    runs = [run_product(inp) for _ in range(10)]                    # nothing synchronises in between
    for r in runs[1:]:
        for n, a, b in zip(NAMES, runs[0], r):
            assert torch.equal(a, b), n


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("name", [RAGGED, WHOLE])
def test_sixteen_bit_types_follow_the_float32_path(name, dtype):
    """One compute path: the 16-bit kernels' results are the float32 kernels' results on the upcast operands, rounded
    (1 ulp), the log-sum-exp exactly.  (The backward is given the same saved output and log-sum-exp in both runs.)"""
    from spfsplatv2_amd import attention
    d = to_device(make_inputs(name, dtype))
    q, k, v, dout, qpos, kpos = (d[n] for n in ("q", "k", "v", "dout", "qpos", "kpos"))
    cfg = (attention.allow_words(d["allow"])[0], 100.0, 1.0, 0.125)
    out16, lse16 = attention.attention_views_forward(q, k, v, qpos, kpos, *cfg)
    out32, lse32 = attention.attention_views_forward(q.float(), k.float(), v.float(), qpos, kpos, *cfg)
    assert out16.dtype == dtype and torch.equal(lse16, lse32)
    assert _ulps(out16, out32.to(dtype)) <= 1

    def backward(q, k, v, out, dout):
        g = [torch.empty(t.shape, dtype=t.dtype, device=DEV) for t in (q, k, v)]
        attention.attention_views_backward(q, k, v, qpos, kpos, *cfg, out, lse16, dout, *g)
        return g
    g16 = backward(q, k, v, out16, dout)
    g32 = backward(q.float(), k.float(), v.float(), out16.float(), dout.float())
    for n, a, b in zip(NAMES[1:], g16, g32):
        assert a.dtype == dtype and torch.isfinite(a).all()
        assert _ulps(a, b.to(dtype)) <= 1, n


def test_gradients_written_into_slices_leave_the_rest_untouched():
    """dq into views 1.. of a buffer with one view more; dk and dv into slots 0 and 2 of a [b, Vk + 1, Nk, 3, H, 64]
    buffer: both batch levels and the token and head strides are the caller's, and nothing else is written."""
    from spfsplatv2_amd import attention
    inp, _, _ = reference(RAGGED)
    b, H, Vq, Vk = CASES[RAGGED][:4]
    d = to_device(inp)
    q, k, v, qpos, kpos, dout = (d[n] for n in ("q", "k", "v", "qpos", "kpos", "dout"))
    Nq, Nk = q.shape[3], k.shape[3]
    cfg = (attention.allow_words(inp["allow"])[0], 100.0, 1.0, 0.125)
    out, lse = attention.attention_views_forward(q, k, v, qpos, kpos, *cfg)
    dense = [torch.empty(t.shape, device=DEV) for t in (q, k, v)]
    attention.attention_views_backward(q, k, v, qpos, kpos, *cfg, out, lse, dout, *dense)
    SENT = 7.0
    dq_buf = torch.full((b, Vq + 1, Nq, H, 64), SENT, device=DEV)
    kv_buf = torch.full((b, Vk + 1, Nk, 3, H, 64), SENT, device=DEV)
    dq = dq_buf[:, 1:].transpose(2, 3)
    dk, dv = kv_buf[:, :Vk, :, 0].transpose(2, 3), kv_buf[:, :Vk, :, 2].transpose(2, 3)
    attention.attention_views_backward(q, k, v, qpos, kpos, *cfg, out, lse, dout, dq, dk, dv)
    for n, a, want in zip(NAMES[1:], (dq, dk, dv), dense):
        assert torch.equal(a, want), n
    assert (dq_buf[:, 0] == SENT).all()
    assert (kv_buf[:, Vk] == SENT).all() and (kv_buf[:, :, :, 1] == SENT).all()
    assert not (dq_buf[:, 1:] == SENT).any() and not (kv_buf[:, :Vk, :, 0] == SENT).any()
    # the autograd function hands out the same bits
    for n, a, want in zip(NAMES[1:], run_product(inp)[1:], dense):
        assert torch.equal(a, want), n


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return torch.load(golden_dir / "attention_views_goldens.pt", weights_only=True)


def test_forward_views_against_the_reference_goldens(goldens):
    """``CrossAttention.forward_views`` with the reference's weights on the second decoder block's view sets -- ONE call
    where the reference's layer was called twice on gathered keys -- against the reference's float32 output and its
    gradients of the tokens and of every parameter: our distance to the float64 oracle may be twice the golden's own
    plus one ulp (the bound of tests/test_gpu_attention.py::test_modules_against_the_reference_goldens)."""
    import spfsplatv2_amd as spf
    name = "blk2_2x4x37_t1"
    case = goldens[name]
    x64_out, x64_grads = voracle.golden_case(case)
    blk2 = spf.decoder_view_sets(case["v"], case["num_target"])[1]
    mod = spf.CrossAttention(128, rope=spf.cuRoPE2D(case["base"], 1.0), num_heads=case["num_heads"], qkv_bias=True).to(DEV)
    mod.load_state_dict(case["weights"])
    x = case["x"].to(DEV).requires_grad_(True)
    pos = case["pos"].to(DEV)
    out = mod.forward_views(x[:, blk2.query], x[:, blk2.key], pos[:, blk2.query], pos[:, blk2.key], blk2.allow)
    params = dict(mod.named_parameters())
    grads = torch.autograd.grad(0.5 * (out * out).sum(), [x] + list(params.values()))
    pairs = [("out", out, case["out"], x64_out)]
    pairs += [(k, g, case["grads"][k], x64_grads[k]) for k, g in zip(["x"] + list(params), grads)]
    assert len(pairs) == 2 + len(case["weights"])
    figures = []
    for n, got, gold, x64 in pairs:
        e_got, e_gold = errs([got], [x64])[0], errs([gold], [x64])[0]
        print(f"{name} {n}: product {e_got:.3e} golden {e_gold:.3e} bound {2 * e_gold + EPS:.3e}")
        figures.append((n, e_got, e_gold))
    for n, e_got, e_gold in figures:
        assert e_got <= 2 * e_gold + EPS, (name, n, e_got, e_gold)


def test_forward_views_on_the_first_decoder_block(goldens):
    """View 0 over the other context views (blk1 of decoder_view_sets(4, 1)) with the goldens' weights: the module
    against the float64 oracle on gathered keys, gated by the same oracle in float32 on the device."""
    import spfsplatv2_amd as spf
    case = goldens["blk2_2x4x37_t1"]
    blk1 = spf.decoder_view_sets(case["v"], case["num_target"])[0]
    allow = blk1.allow.tolist()

    def oracle_run(dtype, dev):
        w = {k: t.to(dev, dtype) for k, t in case["weights"].items()}
        x = case["x"].to(dev, dtype).requires_grad_(True)
        pos = case["pos"].to(dev)
        out = voracle.module_views(x[:, blk1.query], x[:, blk1.key], pos[:, blk1.query], pos[:, blk1.key], allow, w,
                                   case["num_heads"], case["base"])
        (dx,) = torch.autograd.grad(0.5 * (out * out).sum(), (x,))
        return out.detach(), dx

    x64, eager = oracle_run(torch.float64, "cpu"), oracle_run(torch.float32, DEV)
    mod = spf.CrossAttention(128, rope=spf.cuRoPE2D(case["base"], 1.0), num_heads=case["num_heads"], qkv_bias=True).to(DEV)
    mod.load_state_dict(case["weights"])
    x = case["x"].to(DEV).requires_grad_(True)
    pos = case["pos"].to(DEV)
    out = mod.forward_views(x[:, blk1.query], x[:, blk1.key], pos[:, blk1.query], pos[:, blk1.key], blk1.allow)
    assert tuple(out.shape) == (2, 1, 37, 128)
    (dx,) = torch.autograd.grad(0.5 * (out * out).sum(), (x,))
    assert (dx[:, 3] == 0).all()                                    # the target view is neither query nor key here
    gate("blk1_2x4x37_t1", (out.detach(), dx), eager, x64, names=("out", "dx"))
