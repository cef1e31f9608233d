"""Shapes, inputs, float64 references and the gate of the transformer-block tests (tests/test_block.py on the CPU,
tests/test_gpu_block.py on the device).  TEST INFRASTRUCTURE ONLY.  Every reference is computed once and never modified.

Inputs.  Norm rows are drawn with a standard deviation of 0.05 about a per-row mean near 0.3: the variance is then
2.5e-3, so eps = 1e-6 against 1e-5 moves 1 / std by 1.8e-3 (the eps mutant is visible), and the mean is six deviations
away, so a variance formed as E[x^2] - E[x]^2 in float32 would lose two digits.  ``r`` is drawn at the same scale and
gamma around 0.1 (VGGT's ``init_values``).  GELU arguments are standard normal with a bias of scale 0.5.

Gate (the rule of tests/test_gpu_attention_params.py): per tensor err = max|x - x64| / max|x64| against the float64 oracle
must not exceed twice the err of the float32 eager oracle plus one float32 ulp.  POWER CONDITION: every mutant of
tests/block_oracle.py is at least 4 such bounds away in every gated tensor its mutated quantity enters.  It does not enter
-- so nothing is asked of -- ``s`` under the eps and variance mutants (s = x + gamma r has no norm in it) and ``dbias``
under every norm mutant (dbias = sum over the rows of dy, whatever the norm computes).
"""
from __future__ import annotations

import torch

from tests import block_oracle as bo

EPS = 1e-6                     # the modules' LayerNorm eps (the reference's partial(nn.LayerNorm, eps=1e-6))
ULP = 2.0 ** -23
POWER = 4.0
WIDTHS = (4, 128, 192, 260, 768, 1024, 4096)
ROWS = (1, 5, 37)
# more rows than one pass of the capped grids covers: the norm backward caps at 1024 blocks of 16 rows, the GELU kernels
# at 2048 blocks (C = 128: one column tile) of 16 rows
NORM_LOOP_ROWS = 16 * 1024 + 37
GELU_LOOP_ROWS = 16 * 2048 + 37
# (r given, gamma given, ds given)
NORM_VARIANTS = {"plain": (False, False, False), "r": (True, False, False), "r_ds": (True, False, True),
                 "r_gamma": (True, True, False), "r_gamma_ds": (True, True, True)}
NORM_MUTANTS = {"plain": ("eps", "unbiased"), "r": ("eps", "unbiased", "no_residual"),
                "r_ds": ("eps", "unbiased", "no_residual"), "r_gamma": ("eps", "unbiased", "no_residual", "no_gamma"),
                "r_gamma_ds": ("eps", "unbiased", "no_residual", "no_gamma")}
UNREACHED = {"eps": ("s", "dbias"), "unbiased": ("s", "dbias"), "no_residual": ("dbias",), "no_gamma": ("dbias",),
             "tanh": (), "no_bias": ()}

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def norm_inputs(rows: int, c: int, variant: str) -> dict:
    has_r, has_g, has_ds = NORM_VARIANTS[variant]

    def make():
        gen = torch.Generator().manual_seed(1000 * c + rows)
        rn = lambda *s: torch.randn(*s, generator=gen)
        d = {"x": 0.3 + 0.1 * rn(rows, 1) + 0.05 * rn(rows, c), "weight": 1.0 + 0.3 * rn(c), "bias": 0.1 * rn(c),
             "dy": rn(rows, c), "r": None, "gamma": None, "ds": None}
        if has_r:
            d["r"] = (0.05 * rn(rows, c)) / (0.1 if has_g else 1.0)      # gamma * r at the scale of x's deviations
        if has_g:
            d["gamma"] = 0.1 + 0.03 * rn(c)
        if has_ds:
            d["ds"] = rn(rows, c)
        return d
    return _once(("norm_in", rows, c, variant), make)


def norm_oracle(d: dict, dtype=torch.float64, device="cpu", mut=bo.NONE) -> dict:
    return bo.norm_with_grads(d["x"], d["r"], d["weight"], d["bias"], EPS, d["gamma"], d["dy"], d["ds"], dtype, device, mut)


def norm_reference(rows: int, c: int, variant: str):
    """(inputs, float64 oracle, {mutant: {tensor: distance}})"""
    def make():
        d = norm_inputs(rows, c, variant)
        x64 = norm_oracle(d)
        dists = {m: distances(norm_oracle(d, mut=frozenset([m])), x64, m) for m in NORM_MUTANTS[variant]}
        return d, x64, dists
    return _once(("norm_ref", rows, c, variant), make)


def gelu_inputs(rows: int, c: int, with_bias: bool) -> dict:
    def make():
        gen = torch.Generator().manual_seed(77 * c + rows)
        return {"u": torch.randn(rows, c, generator=gen), "bias": 0.5 * torch.randn(c, generator=gen) if with_bias else None,
                "dh": torch.randn(rows, c, generator=gen)}
    return _once(("gelu_in", rows, c, with_bias), make)


def gelu_oracle(d: dict, dtype=torch.float64, device="cpu", mut=bo.NONE) -> dict:
    return bo.gelu_with_grads(d["u"], d["bias"], d["dh"], dtype, device, mut)


def gelu_reference(rows: int, c: int, with_bias: bool):
    def make():
        d = gelu_inputs(rows, c, with_bias)
        x64 = gelu_oracle(d)
        muts = ("tanh", "no_bias") if with_bias else ("tanh",)
        return d, x64, {m: distances(gelu_oracle(d, mut=frozenset([m])), x64, m) for m in muts}
    return _once(("gelu_ref", rows, c, with_bias), make)


def distances(mutant: dict, x64: dict, name: str) -> dict:
    """Per gated tensor the mutant's distance from the true float64 oracle, without the tensors it cannot reach."""
    return {k: bo.rel_err(mutant[k], x64[k]) for k in x64 if k not in UNREACHED[name]}


def errors(got: dict, x64: dict) -> dict:
    assert sorted(got) == sorted(x64), (sorted(got), sorted(x64))
    return {k: bo.rel_err(got[k], x64[k]) for k in x64}


def power_failures(label: str, dists: dict, e_eager: dict) -> list:
    """The offenders of the power condition as text (empty: the gate can be trusted); prints the tightest ratio."""
    bad, tight = [], (float("inf"), "")
    for name, d in dists.items():
        for k, x in d.items():
            bound = 2 * e_eager[k] + ULP
            tight = min(tight, (x / bound, f"{name}, {k}"))
            if x < POWER * bound:
                bad.append(f"{label}: mutant '{name}' moves {k} by {x:.3e} < {POWER:g} x bound {bound:.3e}")
    if dists:
        print(f"{label} power: tightest mutant / bound = {tight[0]:.1f} ({tight[1]})")
    return bad


def gate(label: str, got: dict, eager: dict, x64: dict, dists: dict) -> None:
    """Prints every figure, asserts the power condition on the eager figures, then the gate."""
    e_got, e_eager = errors(got, x64), errors(eager, x64)
    for k in x64:
        print(f"{label} {k}: product {e_got[k]:.3e} eager {e_eager[k]:.3e} bound {2 * e_eager[k] + ULP:.3e}")
    bad = power_failures(label, dists, e_eager)
    assert not bad, "\n".join(bad)
    for k, t in got.items():
        assert torch.isfinite(t).all(), (label, k)
    for k in x64:
        assert e_got[k] <= 2 * e_eager[k] + ULP, (label, k, e_got[k], e_eager[k])


# ---- modules ---------------------------------------------------------------------------------------------------------
KINDS = ("block", "decoder", "vggt")
MODULE_MUTANTS = {"block": ("eps", "unbiased", "tanh", "no_residual", "no_bias"),
                  "decoder": ("eps", "unbiased", "tanh", "no_residual", "no_bias"),
                  "vggt": ("eps", "unbiased", "tanh", "no_residual", "no_gamma", "no_bias")}


def golden(kind: str, golden_dir) -> dict:
    def make():
        g = torch.load(golden_dir / f"block_goldens_{kind}.pt")
        if kind == "decoder":
            g["weights"] = torch.load(golden_dir / "block_goldens_decoder_weights.pt")["weights"]
        return g
    return _once(("golden", kind), make)


def flat(result) -> dict:
    """(out, input gradients, parameter gradients) -> one {name: tensor}"""
    out, gi, gp = result
    return {"out": out, **{"d_" + k: v for k, v in gi.items()}, **{"dparam_" + k: v for k, v in gp.items()}}


def module_reference(kind: str, golden_dir):
    """(golden, float64 oracle as a flat dict, mutant distances over the output and the input gradients)"""
    def make():
        g = golden(kind, golden_dir)
        x64 = flat(bo.module_case(g))
        per_token = [k for k in x64 if not k.startswith("dparam_")]
        dists = {}
        for m in MODULE_MUTANTS[kind]:
            mu = flat(bo.module_case(g, mut=frozenset([m])))
            dists[m] = {k: bo.rel_err(mu[k], x64[k]) for k in per_token}
        return g, x64, dists
    return _once(("module_ref", kind), make)


def build_module(kind: str, g: dict):
    """This package's module of a golden, with the golden's state dict loaded."""
    from functools import partial

    from torch import nn

    import spfsplatv2_amd as spf
    norm = partial(nn.LayerNorm, eps=g["eps"])
    kw = dict(mlp_ratio=g["mlp_ratio"], norm_layer=norm)
    if kind == "block":
        mod = spf.Block(g["dim"], g["num_heads"], qkv_bias=True, rope=spf.cuRoPE2D(freq=g["base"], F0=1.0), **kw)
    elif kind == "decoder":
        mod = spf.DecoderBlock(g["dim"], g["num_heads"], qkv_bias=True, norm_mem=True,
                               rope=spf.cuRoPE2D(freq=g["base"], F0=1.0), **kw)
    else:
        mod = spf.VGGTBlock(g["dim"], g["num_heads"], init_values=g["init_values"], qk_norm=True,
                            rope=spf.RotaryPositionEmbedding2D(frequency=g["base"]), **kw)
    mod.load_state_dict(g["weights"])
    return mod


def run_module(kind: str, mod, ins: dict, pos: dict):
    if kind == "block":
        return mod(ins["x"], pos["xpos"])
    if kind == "decoder":
        return mod(ins["x"], ins["y"], pos["xpos"], pos["ypos"])[0]
    return mod(ins["x"], pos=pos["pos"])
