"""The pose heads' kernels and modules on the device (csrc/posehead.hip, spfsplatv2_amd/posehead.py).

Gate (tests/posehead_cases.py, the rule of tests/block_cases.py): per tensor err = max|x - x64| / max|x64| against the
float64 oracle must not exceed twice the err of the same oracle run eagerly in float32 on the device plus one float32
ulp; before a gate is trusted the power condition of tests/test_posehead.py is asserted again with the device's eager
figures.  Every figure is printed.
"""
from functools import partial

import pytest
import torch

from tests import posehead_cases as cases
from tests import posehead_oracle as po

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _leaf(t):
    return None if t is None else t.to(DEV).requires_grad_(True)


def _same_shapes(got, x64):
    for k, v in got.items():
        assert v.dtype == torch.float32 and v.shape == x64[k].shape, (k, v.shape, x64[k].shape)


# ---- a. pool ---------------------------------------------------------------------------------------------------------
def run_pool(d, mode="view"):
    """The sources where they lie: ``view`` -- dec = tok[:, 1] and enc = tok[:, 2] of two [rows, 3, L, C] tensors;
    ``block`` -- both are the ``tok[:, 1:]`` blocks of [rows / 2, 3, L, C] tensors, [rows / 2, 2, L, C]; ``dense`` -- the
    contiguous tensors."""
    from spfsplatv2_amd import posehead as ph
    rows, L, _ = d["dec"].shape

    def source(t, view):
        if mode == "dense":
            leaf = _leaf(t)
            return leaf, leaf, (lambda g: g)
        if mode == "view":
            big = torch.randn(rows, 3, L, t.shape[-1])
            big[:, view] = t
            leaf = _leaf(big)
            return leaf, leaf[:, view], (lambda g: g[:, view])
        big = torch.randn(rows // 2, 3, L, t.shape[-1])
        big[:, 1:] = t.reshape(rows // 2, 2, L, t.shape[-1])
        leaf = _leaf(big)
        return leaf, leaf[:, 1:], (lambda g: g[:, 1:].reshape(rows, L, t.shape[-1]))
    dec_leaf, dec, dec_back = source(d["dec"], 1)
    enc_leaf = enc = None
    if d["enc"] is not None:
        enc_leaf, enc, enc_back = source(d["enc"], 2)
    for v in (dec, enc):
        assert v is None or ph._pool_source(v) is v                     # read in place: no copy
    if mode == "block":
        assert not dec.is_contiguous() and ph._lead_map(dec, 2, 4) == (2, L * dec.shape[-1], 3 * L * dec.shape[-1])
    feat = ph.pool_tokens(dec, enc)
    g = torch.autograd.grad(feat, [dec_leaf] + ([enc_leaf] if enc_leaf is not None else []),
                            d["dy"].to(DEV).reshape(feat.shape))
    res = {"out": feat.detach().reshape(rows, -1), "d_dec": dec_back(g[0])}
    if enc_leaf is not None:
        res["d_enc"] = enc_back(g[1])
    return res


@pytest.mark.parametrize("widths", cases.POOL_WIDTHS)
@pytest.mark.parametrize("L", cases.POOL_L)
def test_pool_against_oracle(L, widths):
    for rows in cases.POOL_ROWS:
        d, x64, dists = cases.pool_reference(rows, L, widths)
        got = run_pool(d)
        _same_shapes(got, x64)
        cases.gate(f"pool rows={rows} L={L} {widths}", got, cases.pool_oracle(d, torch.float32, DEV), x64, dists)
        dense = run_pool(d, "dense")
        for k in got:
            assert torch.equal(got[k], dense[k]), k
        if L == 1:                                       # a copy, bit for bit
            want = d["dec"][:, 0] if d["enc"] is None else torch.cat([d["enc"][:, 0], d["dec"][:, 0]], -1)
            assert torch.equal(got["out"].cpu(), want)


@pytest.mark.parametrize("L", [1, 49])
def test_pool_reads_a_block_of_views_in_place(L):
    """``tok[:, 1:]`` of a [b, 3, L, C] tensor, a [b, 2, L, C] block: rows addressed by two strides, [b, 2, C' + C] out."""
    d, x64, dists = cases.pool_reference(6, L, (8, 4))
    got = run_pool(d, "block")
    _same_shapes(got, x64)
    cases.gate(f"pool block L={L}", got, cases.pool_oracle(d, torch.float32, DEV), x64, dists)


# ---- b. encode -------------------------------------------------------------------------------------------------------
def run_encode(d, homog):
    from spfsplatv2_amd import posehead as ph
    rot, t = _leaf(d["rot"]), _leaf(d["t"])
    h = po.HOMOG if homog else None
    out = ph.encode_poses([(0, rot[:, :1], t[:, :1], h), (1, rot[:, 1:], t[:, 1:], h)], cases.ENCODE_VIEWS)
    g = torch.autograd.grad(out, [rot, t], d["dy"].to(DEV))
    return {"out": out.detach(), "d_rot": g[0], "d_t": g[1]}


@pytest.mark.parametrize("homog", [True, False])
@pytest.mark.parametrize("b", cases.ROWS)
def test_encode_against_oracle(b, homog):
    d, x64, dists = cases.encode_reference(b, homog)
    got = run_encode(d, homog)
    _same_shapes(got, x64)
    cases.gate(f"encode b={b} homog={homog}", got, cases.encode_oracle(d, torch.float32, DEV, homog=homog), x64, dists)
    if homog:                                            # nothing flows through a clamped h
        clamped = d["t"][..., 3] > 120
        assert clamped.any() and not got["d_t"][..., 3].cpu()[clamped].any()


@pytest.mark.parametrize("homog", [True, False])
def test_encode_takes_more_rows_than_one_pass_of_the_capped_grid(homog):
    """The encode launches are capped at 2048 blocks of 256 rows; a part of 2048 * 256 + 37 rows makes every thread
    loop, forward and backward, and every row of the output and of both gradients is written and right."""
    from spfsplatv2_amd import posehead as ph
    b = 2048 * 256 + 37
    gen = torch.Generator().manual_seed(41)
    t = torch.randn(b, 2, 4 if homog else 3, generator=gen)
    if homog:
        t[..., 3] = torch.tensor(cases.T3_VALUES)[torch.randint(0, 6, (b, 2), generator=gen)] + 0.1 * t[..., 3]
    d = {"rot": torch.randn(b, 2, 6, generator=gen), "t": t, "dy": torch.randn(b, 2, 9, generator=gen)}
    rot, tt = _leaf(d["rot"]), _leaf(d["t"])
    h = po.HOMOG if homog else None
    out = ph.encode_poses([(0, rot[:, :1], tt[:, :1], h), (1, rot[:, 1:], tt[:, 1:], h)], 2)
    g = torch.autograd.grad(out, [rot, tt], d["dy"].to(DEV))
    got = {"out": out.detach(), "d_rot": g[0], "d_t": g[1]}
    x64 = cases.encode_oracle(d, homog=homog)
    _same_shapes(got, x64)
    cases.gate(f"encode rows={b} homog={homog}", got, cases.encode_oracle(d, torch.float32, DEV, homog=homog), x64, {})
    # the last rows, which only the second pass of the loop reaches, on their own
    for k in got:
        assert cases.rel_err(got[k][-37:], x64[k][-37:]) < 1e-6, k


def test_encode_leaves_the_other_views_untouched():
    from spfsplatv2_amd import posehead as ph
    d = cases.encode_inputs(5, True)
    out = torch.full((5, cases.ENCODE_VIEWS, 9), 7.0, device=DEV)
    ph.encode_into(out, 1, d["rot"][:, 1:].to(DEV), d["t"][:, 1:].to(DEV), po.HOMOG)
    assert bool((out[:, 0] == 7.0).all()) and not bool((out[:, 1:] == 7.0).any())
    first = out.clone()
    ph.encode_into(out, 0, d["rot"][:, :1].to(DEV), d["t"][:, :1].to(DEV), po.HOMOG)
    assert torch.equal(out[:, 1:], first[:, 1:]) and not bool((out == 7.0).any())
    assert torch.equal(out, run_encode(d, True)["out"])


# ---- c. embed + SiLU -------------------------------------------------------------------------------------------------
def run_embed(d, bcast):
    from spfsplatv2_amd import posehead as ph
    p, w, b = _leaf(d["p"]), _leaf(d["weight"]), _leaf(d["bias"])
    out = ph.embed_silu(p, w, b, rows=d["dy"].shape[0] if bcast else None)
    g = torch.autograd.grad(out, [p, w, b], d["dy"].to(DEV))
    return {"out": out.detach(), "d_p": g[0], "d_weight": g[1], "d_bias": g[2]}


@pytest.mark.parametrize("c", cases.EMBED_C)
@pytest.mark.parametrize("rows", cases.ROWS)
def test_embed_silu_against_oracle(rows, c):
    for bcast in (False, True):
        d, x64, dists = cases.embed_reference(rows, c, bcast)
        got = run_embed(d, bcast)
        _same_shapes(got, x64)
        cases.gate(f"embed C={c} rows={rows} bcast={bcast}", got, cases.embed_oracle(d, torch.float32, DEV), x64, dists)


# ---- d. modulate -----------------------------------------------------------------------------------------------------
def run_modulate(d):
    import spfsplatv2_amd as spf
    x, mod = _leaf(d["x"]), _leaf(d["mod"])
    out = spf.modulate(x, mod)
    g = torch.autograd.grad(out, [x, mod], d["dy"].to(DEV))
    return {"out": out.detach(), "d_x": g[0], "d_mod": g[1]}


@pytest.mark.parametrize("c", cases.MODULATE_C)
@pytest.mark.parametrize("rows", cases.ROWS)
def test_modulate_against_oracle(rows, c):
    """The thirds are read from the one [rows, 3 C] tensor and the backward answers in the same layout."""
    d, x64, dists = cases.modulate_reference(rows, c)
    got = run_modulate(d)
    _same_shapes(got, x64)
    assert got["d_mod"].shape == (rows, 3 * c) and got["d_mod"].is_contiguous()
    cases.gate(f"modulate C={c} rows={rows}", got, cases.modulate_oracle(d, torch.float32, DEV), x64, dists)
    # the layout, third by third: dshift = dout gate, dgate = dout (LN(x) (1 + scale) + shift)
    dy, mod, x = d["dy"].double(), d["mod"].double(), d["x"].double()
    n = torch.nn.functional.layer_norm(x, (c,), eps=po.ADALN_EPS)
    assert cases.rel_err(got["d_mod"][:, :c], dy * mod[:, 2 * c:]) < 1e-6
    assert cases.rel_err(got["d_mod"][:, 2 * c:], dy * (n * (1 + mod[:, c:2 * c]) + mod[:, :c])) < 1e-5


def test_the_gate_rejects_the_product_run_at_the_other_eps():
    import spfsplatv2_amd as spf
    d, x64, _ = cases.modulate_reference(37, 2048)
    x, mod = _leaf(d["x"]), _leaf(d["mod"])
    out = spf.modulate(x, mod, po.OTHER_EPS)
    (dx,) = torch.autograd.grad(out, x, d["dy"].to(DEV))
    e_eager = cases.errors(cases.modulate_oracle(d, torch.float32, DEV), x64)
    for k, v in (("out", out), ("d_x", dx)):
        a = cases.rel_err(v, x64[k])
        print(f"wrong_eps {k}: product at the other eps {a:.3e} bound {2 * e_eager[k] + cases.ULP:.3e}")
        assert a > 2 * e_eager[k] + cases.ULP, k


# ---- e. attention ----------------------------------------------------------------------------------------------------
def run_attention(d):
    from spfsplatv2_amd import posehead as ph
    qkv = _leaf(d["qkv"])
    out = ph.trunk_attention(qkv, d["H"])
    (g,) = torch.autograd.grad(out, qkv, d["dy"].to(DEV))
    return {"out": out.detach(), "d_qkv": g}


@pytest.mark.parametrize("D", cases.ATTN_D)
@pytest.mark.parametrize("S", cases.ATTN_S)
def test_attention_against_oracle(S, D):
    for B, H in cases.ATTN_BH:
        d, x64, dists = cases.attention_reference(B, S, H, D)
        got = run_attention(d)
        _same_shapes(got, x64)
        cases.gate(f"attn B={B} H={H} S={S} D={D}", got, cases.attention_oracle(d, torch.float32, DEV), x64, dists)


# ---- f. activate -----------------------------------------------------------------------------------------------------
def run_activate(d, acts):
    from spfsplatv2_amd import posehead as ph
    delta = _leaf(d["delta"])
    prev = None if d["prev"] is None else d["prev"].to(DEV)
    pred, out = ph.accumulate_activate(prev, delta, *acts)
    (g,) = torch.autograd.grad(out, delta, d["dy"].to(DEV))
    return {"out0": pred.detach(), "out1": out.detach(), "d_delta": g}


def test_activate_against_oracle():
    import spfsplatv2_amd as spf
    for acts, later in cases.activate_cases():
        d, x64, dists = cases.activate_reference(5, acts, later)
        got = run_activate(d, acts)
        _same_shapes(got, x64)
        cases.gate(f"activate {acts} later={later}", got, cases.activate_oracle(d, torch.float32, DEV, acts=acts), x64, dists)
        if not later:
            assert torch.equal(spf.activate_pose(d["delta"].to(DEV), *acts), got["out1"])


# ---- g. modules ------------------------------------------------------------------------------------------------------
def _prepare(name, g):
    mod = cases.build_module(name, g).to(DEV)
    ins = {k: v.to(DEV).requires_grad_(True) for k, v in g["inputs"].items()}
    return mod, ins


def _step(name, mod, ins, g):
    """Forward and the backward of 0.5 * sum(out^2) over every output to the inputs and every parameter."""
    outs = cases.run_module(name, mod, ins, g)
    wrt = {**ins, **dict(mod.named_parameters())}
    grads = torch.autograd.grad(sum(0.5 * (o * o).sum() for o in outs), list(wrt.values()), allow_unused=True)
    grads = {k: (torch.zeros_like(wrt[k]) if t is None else t) for k, t in zip(wrt, grads)}
    return [o.detach() for o in outs], {k: grads[k] for k in ins}, {k: grads[k] for k in wrt if k not in ins}


@pytest.mark.parametrize("name", cases.MODULES)
def test_modules_against_golden_and_oracle(name, golden_dir):
    """Each module with its golden's state dict: outputs and every gradient, parameters included, through the gate; the
    outputs and input gradients also against the reference's golden itself."""
    g, x64, dists = cases.module_reference(name, golden_dir)
    mod, ins = _prepare(name, g)
    got = cases.flat(_step(name, mod, ins, g))
    eager = cases.flat(po.module_case(g, torch.float32, DEV))
    assert sorted(k for k in got if k.startswith("dparam_")) == sorted("dparam_" + k for k in g["param_names"])
    cases.gate(f"module {name}", got, eager, x64, dists)
    for i, o in enumerate(g["outs"]):
        assert cases.rel_err(got[f"out{i}"], o.double()) < 2e-6, i
    for k, v in g["grads"].items():
        assert cases.rel_err(got["d_" + k], v.double()) < 5e-6, k
    if name == "mlp1":
        assert torch.equal(got["out0"][:, :6].cpu(), torch.tensor([1., 0, 0, 0, 1, 0]).expand(3, 6))


def _pose_setup(b=3, v=3, L=4, enc_c=24, dec_c=16):
    from types import SimpleNamespace

    import spfsplatv2_amd as spf
    torch.manual_seed(5)
    net = SimpleNamespace(enc_embed_dim=enc_c, dec_embed_dim=dec_c)
    cfg = spf.PoseHeadCfg(pose_init_t=False, use_homogeneous=True, concat_enc=True)
    heads = [spf.PoseHead(net, cfg).to(DEV) for _ in range(2)]
    for h in heads:
        torch.nn.init.normal_(h.fc_rot.weight, std=0.3)
    feat = [torch.randn(b, v, L, enc_c, device=DEV, requires_grad=True), torch.randn(b, v, L, 8, device=DEV),
            torch.randn(b, v, L, dec_c, device=DEV, requires_grad=True)]
    return heads, feat


def test_predict_poses_is_the_per_view_loop():
    """``predict_poses`` against ``PoseHead.forward`` per view + ``stack`` + ``process_pose``: bitwise in the forward."""
    import spfsplatv2_amd as spf
    (h1, h2), feat = _pose_setup()
    kw = dict(pose_make_baseline_1=True, pose_make_relative=True)
    got = spf.predict_poses(h1, h2, feat, 2, **kw)
    rows = [h1([tok[:, 0] for tok in feat])] + [h2([tok[:, i] for tok in feat]) for i in range(1, feat[0].shape[1])]
    want = spf.process_pose(torch.stack(rows, dim=1), 2, **kw)
    assert got.shape == (3, 3, 4, 4) and torch.equal(got, want)
    ga = torch.autograd.grad((got * got).sum(), [feat[0], feat[2]] + list(h2.parameters()))
    gb = torch.autograd.grad((want * want).sum(), [feat[0], feat[2]] + list(h2.parameters()))
    for a, b in zip(ga, gb):
        assert cases.rel_err(a, b.double().cpu()) < 1e-5


def test_camera_head_at_the_production_width():
    import spfsplatv2_amd as spf
    torch.manual_seed(7)
    head = spf.CameraHead(2048, trunk_depth=1).to(DEV)
    tokens = (0.3 + 0.05 * torch.randn(1, 2, 3, 2048, device=DEV)).requires_grad_(True)
    outs = head([tokens])
    assert len(outs) == 4 and all(o.shape == (1, 2, 9) and torch.isfinite(o).all() for o in outs)
    wrt = [tokens] + list(head.parameters())
    for g in torch.autograd.grad(sum((o * o).sum() for o in outs), wrt):
        assert torch.isfinite(g).all()


@pytest.mark.parametrize("hidden", [8192, 8200])
def test_a_hidden_width_beyond_the_gelu_row_limit(hidden):
    """The production trunk's MLP is 2048 -> 8192 -> 2048, twice the bias + GELU kernel's row limit: the GELU then runs on
    rows of 4096 (8192) or 1640 (8200 = 5 x 1640) floats of the same memory; against the float64 formula, gradients to
    the input and every parameter."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import posehead as ph
    torch.manual_seed(11)
    mlp = spf.Mlp(32, hidden, 16).to(DEV)
    x = torch.randn(2, 3, 32, device=DEV, requires_grad=True)
    wrt = [x] + list(mlp.parameters())
    out = ph._mlp(mlp, x)
    got = [out] + list(torch.autograd.grad(0.5 * (out * out).sum(), wrt))
    x64 = [t.detach().double().cpu().requires_grad_(True) for t in wrt]
    h = torch.nn.functional.gelu(torch.nn.functional.linear(x64[0], x64[1], x64[2]))
    ref = torch.nn.functional.linear(h, x64[3], x64[4])
    want = [ref] + list(torch.autograd.grad(0.5 * (ref * ref).sum(), x64))
    assert out.shape == (2, 3, 16)
    for a, b in zip(got, want):
        assert cases.rel_err(a, b.detach()) < 5e-6


# ---- h. reproducibility ----------------------------------------------------------------------------------------------
def test_backwards_are_bitwise_reproducible(golden_dir):
    runs = [(run_pool, cases.pool_inputs(3, 256, (1024, 768))), (partial(run_encode, homog=True), cases.encode_inputs(37, True)),
            (partial(run_embed, bcast=False), cases.embed_inputs(37, 2048, False)),
            (partial(run_embed, bcast=True), cases.embed_inputs(37, 2048, True)), (run_modulate, cases.modulate_inputs(37, 4096)),
            (run_attention, cases.attention_inputs(3, 32, 16, 128)),
            (partial(run_activate, acts=("inv_log", "exp", "relu")), cases.activate_inputs(5, True))]
    for run, d in runs:
        a, b = run(d), run(d)
        for k in a:
            assert torch.equal(a[k], b[k]), (run, k)
    g = cases.golden("camera", golden_dir)
    prepared = _prepare("camera", g)
    a, b = _step("camera", *prepared, g), _step("camera", *prepared, g)
    for x, y in zip(a, b):
        for k in (x if isinstance(x, dict) else range(len(x))):
            assert torch.equal(x[k], y[k]), k


# ---- i. no host synchronisation --------------------------------------------------------------------------------------
def _no_sync(step):
    want = step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return want, got


def test_camera_head_step_never_syncs(golden_dir):
    g = cases.golden("camera", golden_dir)
    mod, ins = _prepare("camera", g)
    other = g["other_tokens"].to(DEV)

    def step():
        outs = mod([other, ins["tokens"]], num_iterations=4)
        wrt = [ins["tokens"]] + list(mod.parameters())
        return outs, torch.autograd.grad(sum(0.5 * (o * o).sum() for o in outs), wrt)
    want, got = _no_sync(step)
    for a, b in zip(want[0] + list(want[1]), got[0] + list(got[1])):
        assert torch.equal(a, b)


def test_predict_poses_step_never_syncs():
    import spfsplatv2_amd as spf
    (h1, h2), feat = _pose_setup()

    def step():
        poses = spf.predict_poses(h1, h2, feat, 2, pose_make_baseline_1=True, pose_make_relative=True)
        return poses, torch.autograd.grad((poses * poses).sum(), [feat[0], feat[2]] + list(h1.parameters()))
    want, got = _no_sync(step)
    assert torch.equal(want[0], got[0])
    for a, b in zip(want[1], got[1]):
        assert torch.equal(a, b)


# ---- j. the library's argument checks --------------------------------------------------------------------------------
def test_library_argument_checks_launch_nothing(hip_lib):
    import ctypes as C
    qkv = torch.randn(1, 2, 192, device=DEV)
    out = torch.full((1, 2, 64), 7.0, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert hip_lib.spf_posehead_attn_forward(p(qkv), 1, 33, 1, 64, p(out), None) == -1
    assert hip_lib.spf_posehead_attn_forward(p(qkv), 1, 2, 1, 32, p(out), None) == -1
    assert hip_lib.spf_posehead_modulate_forward(p(qkv), p(qkv), 2, 6, 1e-6, p(out), None) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert hip_lib.spf_posehead_attn_forward(p(qkv), 1, 2, 1, 64, p(out), None) == 0
    torch.cuda.synchronize()
    assert cases.rel_err(out, po.attention(qkv.double().cpu(), 1)) < 1e-6
