"""The transformer block without a device: exports, state dicts, refusals, the partial-workspace arithmetic, the oracle
against the reference's goldens, and the power condition of the gates with float32 eager on the CPU standing in for the
device (tests/block_cases.py states the gate; tests/test_gpu_block.py applies it to the kernels)."""
import ctypes as C
from functools import partial

import pytest
import torch
from torch import nn

from tests import block_cases as cases
from tests import block_oracle as bo

NAMES = ("Block", "DecoderBlock", "VGGTBlock", "Mlp", "LayerScale", "layer_norm", "add_layer_norm", "bias_gelu")


def test_exports():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import block
    for name in NAMES:
        assert name in spf.__all__ and getattr(spf, name) is getattr(block, name), name


# ---- state dicts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", cases.KINDS)
def test_state_dict_keys_are_the_reference_s(kind, golden_dir):
    g = cases.golden(kind, golden_dir)
    mod = cases.build_module(kind, g)                                   # (load_state_dict is strict)
    sd = mod.state_dict()
    assert list(sd) == list(g["weights"])
    for k, v in g["weights"].items():
        assert sd[k].shape == v.shape and torch.equal(sd[k], v), k


def test_constructor_signatures_are_the_reference_s():
    import inspect

    import spfsplatv2_amd as spf
    assert list(inspect.signature(spf.Block.__init__).parameters)[1:] == [
        "dim", "num_heads", "mlp_ratio", "qkv_bias", "drop", "attn_drop", "drop_path", "act_layer", "norm_layer", "rope"]
    assert list(inspect.signature(spf.DecoderBlock.__init__).parameters)[1:] == [
        "dim", "num_heads", "mlp_ratio", "qkv_bias", "drop", "attn_drop", "drop_path", "act_layer", "norm_layer", "norm_mem",
        "rope"]
    assert list(inspect.signature(spf.VGGTBlock.__init__).parameters)[1:] == [
        "dim", "num_heads", "mlp_ratio", "qkv_bias", "proj_bias", "ffn_bias", "drop", "attn_drop", "init_values", "drop_path",
        "act_layer", "norm_layer", "attn_class", "ffn_layer", "qk_norm", "fused_attn", "rope"]
    assert list(inspect.signature(spf.Mlp.__init__).parameters)[1:] == [
        "in_features", "hidden_features", "out_features", "act_layer", "bias", "drop"]
    dec = spf.DecoderBlock(128, 2, norm_mem=False)
    assert isinstance(dec.norm_y, nn.Identity) and not any(k.startswith("norm_y") for k in dec.state_dict())
    plain = spf.VGGTBlock(128, 2)
    assert isinstance(plain.ls1, nn.Identity) and isinstance(plain.ls2, nn.Identity)
    assert "fc1.bias" not in spf.VGGTBlock(128, 2, ffn_bias=False).mlp.state_dict()


# ---- refusals, all before any launch (there is no device here) -------------------------------------------------------
def test_functions_refuse_cpu_tensors_and_sixteen_bit_types():
    import spfsplatv2_amd as spf
    x, w, b = torch.randn(5, 128), torch.ones(128), torch.zeros(128)
    for call in (lambda: spf.layer_norm(x, w, b, 1e-6), lambda: spf.add_layer_norm(x, x, w, b, 1e-6),
                 lambda: spf.add_layer_norm(x, x, w, b, 1e-6, gamma=w), lambda: spf.bias_gelu(x, b),
                 lambda: spf.bias_gelu(x, None)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for dt in (torch.float16, torch.bfloat16):
        h = x.to(dt)
        for call in (lambda: spf.layer_norm(h, w, b, 1e-6), lambda: spf.add_layer_norm(x, h, w, b, 1e-6),
                     lambda: spf.add_layer_norm(x, x, w.to(dt), b, 1e-6), lambda: spf.bias_gelu(h, b),
                     lambda: spf.bias_gelu(x, b.to(dt))):
            with pytest.raises(NotImplementedError, match="float32"):
                call()
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        spf.layer_norm(x.double(), w, b, 1e-6)


def test_functions_refuse_bad_arguments():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import block
    for c in (2, 6, 130, 4100, 8192):
        x = torch.randn(3, c)
        with pytest.raises(ValueError, match="multiple of 4"):
            spf.layer_norm(x, torch.ones(c), torch.zeros(c), 1e-6)
        with pytest.raises(ValueError, match="multiple of 4"):
            spf.bias_gelu(x, None)
    x, w, b = torch.randn(5, 128), torch.ones(128), torch.zeros(128)
    with pytest.raises(ValueError, match="gamma is given without r"):
        block._check_norm_call("add_layer_norm", x, None, w, b, w)
    with pytest.raises(ValueError, match="r is required"):
        spf.add_layer_norm(x, None, w, b, 1e-6, gamma=w)
    with pytest.raises(RuntimeError, match="differ in shape"):
        spf.add_layer_norm(x, x[:4], w, b, 1e-6)
    with pytest.raises(RuntimeError, match="weight must have shape"):
        spf.layer_norm(x, torch.ones(64), b, 1e-6)
    with pytest.raises(RuntimeError, match="bias must have shape"):
        spf.bias_gelu(x, torch.ones(64))
    with pytest.raises(RuntimeError, match="at least one row"):
        spf.layer_norm(x[:0], w, b, 1e-6)


def test_modules_refuse_at_construction():
    import spfsplatv2_amd as spf
    for act in (nn.ReLU, nn.SiLU, partial(nn.GELU, approximate="tanh")):
        with pytest.raises(TypeError, match="nn.GELU"):
            spf.Mlp(128, 256, act_layer=act)
        for cls in (spf.Block, spf.DecoderBlock, spf.VGGTBlock):
            with pytest.raises(TypeError, match="nn.GELU"):
                cls(128, 2, act_layer=act)
    for norm in (nn.Identity, nn.BatchNorm1d, partial(nn.LayerNorm, elementwise_affine=False),
                 partial(nn.LayerNorm, bias=False), lambda dim: nn.LayerNorm(2 * dim)):
        for cls in (spf.Block, spf.DecoderBlock, spf.VGGTBlock):
            with pytest.raises(TypeError, match="nn.LayerNorm"):
                cls(128, 2, norm_layer=norm)
    with pytest.raises(TypeError, match="VGGTAttention"):
        spf.VGGTBlock(128, 2, attn_class=spf.Attention)
    with pytest.raises(TypeError, match="Mlp"):
        spf.VGGTBlock(128, 2, ffn_layer=nn.Linear)


def _forwards():
    import spfsplatv2_amd as spf
    x, y = torch.randn(1, 5, 128), torch.randn(1, 7, 128)
    pos = torch.zeros(1, 5, 2, dtype=torch.long)
    ypos = torch.zeros(1, 7, 2, dtype=torch.long)
    return {spf.Block: lambda m: m(x, pos), spf.DecoderBlock: lambda m: m(x, y, pos, ypos),
            spf.VGGTBlock: lambda m: m(x, pos=None)}


def test_modules_refuse_dropout_and_drop_path_in_training_mode():
    """... and in eval mode, or with zero rates, get as far as the device check: both are identities there."""
    import spfsplatv2_amd as spf
    for cls, run in _forwards().items():
        for kw, what in (({"drop_path": 0.1}, "drop_path"), ({"drop": 0.1}, "drop > 0")):
            mod = cls(128, 2, **kw)
            with pytest.raises(NotImplementedError, match=what):
                run(mod)
            mod.eval()
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                run(mod)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            run(cls(128, 2))
    mlp = spf.Mlp(128, 256, drop=0.2)
    with pytest.raises(NotImplementedError, match="drop > 0"):
        mlp(torch.randn(3, 128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp.eval()(torch.randn(3, 128))
    with pytest.raises(NotImplementedError, match="float32"):
        spf.Mlp(128, 256)(torch.randn(3, 128).half())
    drop = spf.block.DropPath(0.3)
    t = torch.randn(4)
    assert drop.eval()(t) is t
    with pytest.raises(NotImplementedError):
        drop.train()(t)
    assert torch.equal(spf.LayerScale(4, init_values=0.5)(torch.ones(2, 4)), torch.full((2, 4), 0.5))


def test_decoder_block_hands_the_mask_to_cross_attention(monkeypatch):
    """... which refuses it, as it does on its own: the refusal is CrossAttention's, reached through the block."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import block
    seen = {}
    ident = lambda x, *a, **k: x
    monkeypatch.setattr(block, "layer_norm", ident)
    monkeypatch.setattr(block, "add_layer_norm", lambda x, r, *a, **k: (x + r, x + r))
    dec = spf.DecoderBlock(128, 2)
    monkeypatch.setattr(dec.attn, "forward", lambda x, xpos: x)
    real = dec.cross_attn.forward

    def spy(q, k, v, qpos, kpos, mask=None):
        seen["mask"] = mask
        return real(q, k, v, qpos, kpos, mask)
    monkeypatch.setattr(dec.cross_attn, "forward", spy)
    mask = torch.zeros(1, 5, 7)
    with pytest.raises(NotImplementedError, match="masks are not supported"):
        dec(torch.randn(1, 5, 128), torch.randn(1, 7, 128), None, None, mask)
    assert seen["mask"] is mask


# ---- the workspace helper --------------------------------------------------------------------------------------------
def test_partial_blocks_formulas(hip_lib):
    """norm backward: one block per 16 rows, at most 1024.  GELU backward: the same, at most 2048 // (column tiles of 256)."""
    from spfsplatv2_amd import block
    for rows in (1, 5, 16, 17, 37, 12288, 16384, 16385, cases.NORM_LOOP_ROWS, cases.GELU_LOOP_ROWS, 1 << 30):
        for c in cases.WIDTHS:
            want = min((rows + 15) // 16, 1024)
            assert hip_lib.spf_block_partial_blocks(rows, c, 0) == want == block.partial_blocks(rows, c)
            tiles = (c + 255) // 256
            want = min((rows + 15) // 16, max(2048 // tiles, 1))
            assert hip_lib.spf_block_partial_blocks(rows, c, 1) == want == block.partial_blocks(rows, c, True)
    assert block.partial_blocks(cases.NORM_LOOP_ROWS, 128) == 1024 < (cases.NORM_LOOP_ROWS + 15) // 16
    assert block.partial_blocks(cases.GELU_LOOP_ROWS, 128, True) == 2048 < (cases.GELU_LOOP_ROWS + 15) // 16
    for rows, c in ((0, 128), (-1, 128), ((1 << 30) + 1, 128), (5, 0), (5, 6), (5, 4100)):
        assert hip_lib.spf_block_partial_blocks(rows, c, 0) == -1 and b"multiple of 4" in hip_lib.spf_last_error()
        with pytest.raises(RuntimeError, match="rejected"):
            block.partial_blocks(rows, c)


def test_library_argument_checks_on_the_host(hip_lib):
    """Rejected with SPF_E_INVALID and a message before anything touches a device (the pointers are never read)."""
    from spfsplatv2_amd import _lib
    err = hip_lib.spf_last_error
    p = 4096                                                            # a 16-byte aligned non-null address

    def norm(**kw):
        a = _lib.SpfBlockNorm()
        a.x, a.weight, a.bias, a.x_inner, a.x_stride, a.r_inner, a.rows, a.C, a.eps = p, p, p, 5, 128, 1, 5, 128, 1e-6
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)
    fwd, bwd = hip_lib.spf_block_add_norm_forward, hip_lib.spf_block_add_norm_backward
    assert fwd(None, p, p, p, None) == -1 and b"args is null" in err()
    assert fwd(norm(x=None), None, p, p, None) == -1 and b"null pointer" in err()
    assert fwd(norm(bias=None), None, p, p, None) == -1 and b"null pointer" in err()
    assert fwd(norm(), None, None, p, None) == -1 and b"null output" in err()
    assert fwd(norm(r=p, r_stride=128), None, p, p, None) == -1 and b"null output" in err()
    assert fwd(norm(gamma=p), None, p, p, None) == -1 and b"gamma is given without r" in err()
    for c in (0, 2, 6, 4100):
        assert fwd(norm(C=c), None, p, p, None) == -1 and b"multiple of 4" in err()
    assert fwd(norm(rows=0), None, p, p, None) == -1 and b"rows must be" in err()
    assert fwd(norm(x=p + 4), None, p, p, None) == -1 and b"16-byte aligned" in err()
    assert fwd(norm(x_stride=130), None, p, p, None) == -1 and b"multiples of 4" in err()
    assert fwd(norm(x_inner=0), None, p, p, None) == -1 and b"group sizes" in err()
    assert bwd(norm(bias=None), None, None, p, p, None, p, p, None) == -1 and b"null pointer" in err()
    assert bwd(norm(gamma=p), p, None, p, p, p, p, p, None) == -1 and b"gamma is given without r" in err()
    assert bwd(norm(r=p), p, None, p, p, None, p, p, None) == -1 and b"only with gamma" in err()
    assert bwd(norm(), p, None, p, p, p, p, p, None) == -1 and b"dr is written with gamma only" in err()
    assert bwd(norm(r=p, gamma=p), p, None, p, p, None, p, p, None) == -1 and b"dr is written with gamma only" in err()
    assert bwd(norm(), p, p + 8, p, p, None, p, p, None) == -1 and b"16-byte aligned" in err()
    gf, gb = hip_lib.spf_block_bias_gelu_forward, hip_lib.spf_block_bias_gelu_backward
    assert gf(None, p, 5, 128, p, None) == -1 and b"null pointer" in err()
    assert gf(p, None, 5, 130, p, None) == -1 and b"multiple of 4" in err()
    assert gf(p, p + 4, 5, 128, p, None) == -1 and b"16-byte aligned" in err()
    assert gb(p, p, None, 5, 128, p, p, p, None) == -1 and b"null pointer" in err()
    assert gb(p, p, p, 5, 128, p, None, p, None) == -1 and b"with a bias and only then" in err()
    assert gb(p, None, p, 5, 128, p, p, None, None) == -1 and b"with a bias and only then" in err()
    assert gb(p, None, p, 5, 8192, p, None, None, None) == -1 and b"multiple of 4" in err()


def test_rows_read_in_place_arithmetic():
    """Which views ``_rows`` passes through and how it addresses them; no device needed."""
    from spfsplatv2_amd import block
    tok = torch.randn(2, 3, 37, 128)
    for view, want in ((tok, (222, 128, 0)), (tok[:, 1], (37, 128, 3 * 37 * 128)), (tok[1], (111, 128, 0)),
                       (tok[:, :, 5], (6, 37 * 128, 0)), (tok[0, 0, 0], (1, 0, 0)), (tok[:, :, :, :64], (222, 128, 0)),
                       (tok[:, 1:, ::2], None), (tok.transpose(-1, -2), None), (tok[..., 1:5], None)):
        got = block._rows(view)
        if want is None:
            assert got is not view and got.is_contiguous() and torch.equal(got, view)
        else:
            assert got is view and block._row_map(view) == want
            inner, stride, outer = want
            flat = view.reshape(-1, view.shape[-1])
            for i in (0, flat.shape[0] // 2, flat.shape[0] - 1):
                off = (i // inner) * outer + (i % inner) * stride
                assert torch.equal(tok.reshape(-1)[view.storage_offset() + off:][:view.shape[-1]], flat[i])


# ---- the oracle ------------------------------------------------------------------------------------------------------
def test_oracle_kernels_are_torch_s():
    """The restated formulas are F.layer_norm and F.gelu, and their mutants are not."""
    import torch.nn.functional as F
    d = cases.norm_inputs(37, 260, "r_gamma_ds")
    x, r, w, b, g = (d[k].double() for k in ("x", "r", "weight", "bias", "gamma"))
    s, y = bo.add_layer_norm(x, r, w, b, cases.EPS, g)
    assert torch.equal(s, x + r * g)
    assert (y - F.layer_norm(x + r * g, (260,), w, b, cases.EPS)).abs().max() < 1e-13
    u = cases.gelu_inputs(37, 260, True)
    assert (bo.bias_gelu(u["u"].double(), u["bias"].double()) - F.gelu(u["u"].double() + u["bias"].double())).abs().max() < 1e-14
    assert (bo.bias_gelu(u["u"].double(), u["bias"].double(), frozenset(["tanh"]))
            - F.gelu(u["u"].double() + u["bias"].double(), approximate="tanh")).abs().max() < 1e-14


@pytest.mark.parametrize("kind", cases.KINDS)
def test_oracle_reproduces_the_reference_goldens(kind, golden_dir):
    """float64 oracle against the float32 outputs of the reference's own classes: within the float32 run's rounding."""
    g, x64, _ = cases.module_reference(kind, golden_dir)
    assert g["dim"] == 128 and g["num_heads"] == 2 and g["mlp_ratio"] == 2 and g["eps"] == 1e-6
    assert g["inputs"]["x"].shape[1] == 37 and (kind != "decoder" or g["inputs"]["y"].shape[1] == 70)
    assert bo.rel_err(g["out"], x64["out"]) < 2e-6
    for k, v in g["grads"].items():
        assert bo.rel_err(v, x64["d_" + k]) < 5e-6, k
    # and in float32 the oracle IS the reference up to the order of its sums
    f32 = cases.flat(bo.module_case(g, torch.float32))
    assert bo.rel_err(f32["out"], g["out"].double()) < 2e-6


# ---- the power condition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(cases.NORM_VARIANTS))
@pytest.mark.parametrize("c", cases.WIDTHS)
def test_power_condition_of_the_norm_gate(c, variant):
    """float32 eager on the CPU stands in for the device: every mutant at least 4 bounds away, at the smallest row count
    with more than one row and at the largest."""
    for rows in (5, 37):
        d, x64, dists = cases.norm_reference(rows, c, variant)
        e_eager = cases.errors(cases.norm_oracle(d, torch.float32), x64)
        bad = cases.power_failures(f"norm C={c} rows={rows} {variant}", dists, e_eager)
        assert not bad, "\n".join(bad)
        assert set(dists) == set(cases.NORM_MUTANTS[variant])
        for m, dist in dists.items():
            assert set(dist) == set(x64) - set(cases.UNREACHED[m])


@pytest.mark.parametrize("c", cases.WIDTHS)
def test_power_condition_of_the_gelu_gate(c):
    for rows in (5, 37):
        for with_bias in (True, False):
            d, x64, dists = cases.gelu_reference(rows, c, with_bias)
            e_eager = cases.errors(cases.gelu_oracle(d, torch.float32), x64)
            bad = cases.power_failures(f"gelu C={c} rows={rows} bias={with_bias}", dists, e_eager)
            assert not bad, "\n".join(bad)
            assert set(x64) == ({"h", "du", "db"} if with_bias else {"h", "du"})


@pytest.mark.parametrize("kind", cases.KINDS)
def test_power_condition_of_the_module_gate(kind, golden_dir):
    g, x64, dists = cases.module_reference(kind, golden_dir)
    e_eager = cases.errors(cases.flat(bo.module_case(g, torch.float32)), x64)
    assert set(dists) == set(cases.MODULE_MUTANTS[kind])
    bad = cases.power_failures(f"module {kind}", dists, e_eager)
    assert not bad, "\n".join(bad)


def test_the_gate_rejects_a_mutant_and_accepts_the_eager_run():
    d, x64, dists = cases.norm_reference(37, 768, "r_gamma_ds")
    eager = cases.norm_oracle(d, torch.float32)
    cases.gate("control", eager, eager, x64, dists)
    for m in cases.NORM_MUTANTS["r_gamma_ds"]:
        with pytest.raises(AssertionError):
            cases.gate("control " + m, cases.norm_oracle(d, torch.float32, mut=frozenset([m])), eager, x64, {})
