"""Shapes, inputs, float64 references and the gate of the pose-head tests (tests/test_posehead.py on the CPU,
tests/test_gpu_posehead.py on the device).  TEST INFRASTRUCTURE ONLY.  Every reference is computed once and never modified.

Inputs.  Norm rows (modulate's x, the goldens' tokens) are drawn as in tests/block_cases.py: a standard deviation of 0.05
about a per-row mean near 0.3, so eps = 1e-6 against 1e-5 moves 1 / std by 1.8e-3 and a one-pass variance would lose two
digits.  The homogeneous logits t3 of the encode cases are drawn from {-60, -3, 0, 3, 25, 150} plus noise of 0.1: every
case is a [b, 7, 9] encoding whose views 1..6 hold all six values in every scene, so the softplus linear branch
(beta x > 20: 25 and 150), the floor h = 0.25 (-60) and the clamp h = 100 (150) occur in every case.

Gate: the rule of tests/block_cases.py, not a new number.  Per tensor err = max|x - x64| / max|x64| against the float64
oracle must not exceed twice the err of the float32 eager oracle plus one float32 ulp (a tensor whose float64 reference
is all zero must be all zero).  POWER CONDITION: every mutant of tests/posehead_oracle.py listed for a case is at least 4
such bounds away in every gated tensor it can reach.  What a mutant cannot reach, by name (UNREACHED):
  no_residual        ``d_mod``: the residual enters neither shift, scale nor gate
  relu_everywhere    ``out0`` (the accumulated encoding, before any activation)
  beta_one, no_clamp, clamp_min_scale   ``d_rot``: the rotation's six floats pass through untouched
  no_accumulate (camera golden)   ``out0``, the first iteration's output: there is nothing to accumulate yet
A mutant is not listed for a case where it changes nothing at all: sum_not_mean at L = 1, dec_first with one source, the
attention mutants at S = 1 (one key: the softmax is 1 whatever the scores), no_accumulate on a first iteration, the
encode mutants without the homogeneous coordinate.  The first PoseHead golden lists no ``no_clamp``: its logits t3 come
out of a freshly initialised ``fc_t`` and stay far below the 108 at which h reaches 100, so the clamp never acts there
(the encode cases reach it in every scene).  The camera golden lists no ``eps``: adaLN there sees LayerNorm
output, whose unit variance hides 1e-5 against 1e-6 (the kernel cases show it).
"""
from __future__ import annotations

import torch

from tests import posehead_oracle as po
from tests.block_cases import POWER, ULP, power_failures  # noqa: F401  (the rule and its two numbers)

ROWS = (1, 5, 37)
POOL_L = (1, 4, 49, 256)
POOL_WIDTHS = ((4,), (8, 4), (1024, 768))
POOL_ROWS = (1, 3)
EMBED_C = (4, 260, 2048)
MODULATE_C = (4, 128, 260, 2048, 4096)
ATTN_S = (1, 2, 3, 10, 32)
ATTN_BH = ((1, 1), (3, 16))
ATTN_D = (64, 128)
ACTS = ("linear", "inv_log", "exp", "relu")
T3_VALUES = (-60.0, -3.0, 0.0, 3.0, 25.0, 150.0)
ENCODE_VIEWS = 7
UNREACHED = {"no_residual": ("d_mod",), "relu_everywhere": ("out0",), "beta_one": ("d_rot",), "no_clamp": ("d_rot",),
             "clamp_min_scale": ("d_rot",)}

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rel_err(got, want) -> float:
    """max|x - x64| / max|x64|; where the reference is all zero: 0 for an all-zero tensor, else inf"""
    ref = float(want.abs().max())
    diff = float((got.detach().double().cpu() - want.double().cpu()).abs().max())
    return diff / ref if ref > 0 else (0.0 if diff == 0 else float("inf"))


def errors(got: dict, x64: dict) -> dict:
    assert sorted(got) == sorted(x64), (sorted(got), sorted(x64))
    return {k: rel_err(got[k], x64[k]) for k in x64}


def distances(mutant: dict, x64: dict, name: str, unreached=UNREACHED) -> dict:
    return {k: rel_err(mutant[k], x64[k]) for k in x64 if k not in unreached.get(name, ())}


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


def _reference(key, inputs, oracle, mutants):
    """(inputs, float64 oracle, {mutant: {tensor: distance}})"""
    def make():
        d = inputs()
        x64 = oracle(d)
        return d, x64, {m: distances(oracle(d, mut=frozenset([m])), x64, m) for m in mutants}
    return _once(key, make)


# ---- a. pool ---------------------------------------------------------------------------------------------------------
def pool_inputs(rows: int, L: int, widths: tuple) -> dict:
    def make():
        gen = torch.Generator().manual_seed(7 * L + 1000 * rows + widths[0])
        rn = lambda *s: torch.randn(*s, generator=gen)
        d = {"dec": 0.3 + 0.5 * rn(rows, L, widths[-1]), "enc": None, "dy": rn(rows, sum(widths))}
        if len(widths) == 2:
            d["enc"] = 0.3 + 0.5 * rn(rows, L, widths[0])
        return d
    return _once(("pool_in", rows, L, widths), make)


def pool_oracle(d, dtype=torch.float64, device="cpu", mut=po.NONE):
    return po.with_grads(lambda dec, enc=None: po.pool(dec, enc, mut), {"dec": d["dec"], "enc": d["enc"]}, {}, [d["dy"]],
                         dtype, device)


def pool_mutants(L: int, widths: tuple) -> tuple:
    return (("sum_not_mean",) if L > 1 else ()) + (("dec_first",) if len(widths) == 2 else ())


def pool_reference(rows, L, widths):
    return _reference(("pool", rows, L, widths), lambda: pool_inputs(rows, L, widths), pool_oracle, pool_mutants(L, widths))


# ---- b. encode -------------------------------------------------------------------------------------------------------
def encode_inputs(b: int, homog: bool) -> dict:
    def make():
        gen = torch.Generator().manual_seed(11 * b + int(homog))
        rn = lambda *s: torch.randn(*s, generator=gen)
        v = ENCODE_VIEWS
        t = rn(b, v, 4 if homog else 3)
        if homog:
            idx = (torch.arange(v)[None, :] + torch.arange(b)[:, None]) % len(T3_VALUES)
            idx[:, 0] = torch.arange(b) % len(T3_VALUES)
            t[..., 3] = torch.tensor(T3_VALUES)[idx] + 0.1 * rn(b, v)
        return {"rot": rn(b, v, 6), "t": t, "dy": rn(b, v, 9)}
    return _once(("encode_in", b, homog), make)


def encode_oracle(d, dtype=torch.float64, device="cpu", mut=po.NONE, homog=True):
    return po.with_grads(lambda rot, t: po.encode(rot, t, po.HOMOG if homog else None, mut), {"rot": d["rot"], "t": d["t"]},
                         {}, [d["dy"]], dtype, device)


def encode_reference(b, homog):
    from functools import partial
    muts = ("beta_one", "no_clamp", "clamp_min_scale") if homog else ()
    return _reference(("encode", b, homog), lambda: encode_inputs(b, homog), partial(encode_oracle, homog=homog), muts)


# ---- c. embed + SiLU -------------------------------------------------------------------------------------------------
def embed_inputs(rows: int, c: int, bcast: bool) -> dict:
    def make():
        gen = torch.Generator().manual_seed(13 * c + rows + 500 * int(bcast))
        rn = lambda *s: torch.randn(*s, generator=gen)
        return {"p": rn(1 if bcast else rows, 9), "weight": rn(c, 9) / 3.0, "bias": 0.5 * rn(c), "dy": rn(rows, c)}
    return _once(("embed_in", rows, c, bcast), make)


def embed_oracle(d, dtype=torch.float64, device="cpu", mut=po.NONE):
    rows = d["dy"].shape[0]
    return po.with_grads(lambda p, weight, bias: po.embed_silu(p.expand(rows, 9), weight, bias, mut),
                         {"p": d["p"], "weight": d["weight"], "bias": d["bias"]}, {}, [d["dy"]], dtype, device)


def embed_reference(rows, c, bcast):
    return _reference(("embed", rows, c, bcast), lambda: embed_inputs(rows, c, bcast), embed_oracle,
                      ("sigmoid_only", "no_bias"))


# ---- d. modulate -----------------------------------------------------------------------------------------------------
def modulate_inputs(rows: int, c: int) -> dict:
    def make():
        gen = torch.Generator().manual_seed(17 * c + rows)
        rn = lambda *s: torch.randn(*s, generator=gen)
        mod = torch.cat([0.3 * rn(rows, c), 0.3 * rn(rows, c), 0.5 + 0.3 * rn(rows, c)], dim=-1)
        return {"x": 0.3 + 0.1 * rn(rows, 1) + 0.05 * rn(rows, c), "mod": mod, "dy": rn(rows, c)}
    return _once(("modulate_in", rows, c), make)


def modulate_oracle(d, dtype=torch.float64, device="cpu", mut=po.NONE):
    return po.with_grads(lambda x, mod: po.modulate(x, mod, po.ADALN_EPS, mut), {"x": d["x"], "mod": d["mod"]}, {},
                         [d["dy"]], dtype, device)


def modulate_reference(rows, c):
    return _reference(("modulate", rows, c), lambda: modulate_inputs(rows, c), modulate_oracle,
                      ("eps", "unbiased", "scale_without_one", "no_gate", "no_residual"))


# ---- e. attention ----------------------------------------------------------------------------------------------------
def attention_inputs(B: int, S: int, H: int, D: int) -> dict:
    def make():
        gen = torch.Generator().manual_seed(19 * S + 100 * B + D)
        return {"qkv": torch.randn(B, S, 3 * H * D, generator=gen), "dy": torch.randn(B, S, H * D, generator=gen), "H": H}
    return _once(("attn_in", B, S, H, D), make)


def attention_oracle(d, dtype=torch.float64, device="cpu", mut=po.NONE):
    return po.with_grads(lambda qkv: po.attention(qkv, d["H"], mut), {"qkv": d["qkv"]}, {}, [d["dy"]], dtype, device)


def attention_reference(B, S, H, D):
    return _reference(("attn", B, S, H, D), lambda: attention_inputs(B, S, H, D), attention_oracle,
                      ("scale", "softmax_over_queries") if S > 1 else ())


# ---- f. activate -----------------------------------------------------------------------------------------------------
def activate_cases():
    """(acts, later): every act name on each slice, the other two slices inv_log (so that every gradient depends on the
    accumulated encoding); first iteration and later iteration."""
    out = []
    for s in range(3):
        for a in ACTS:
            acts = tuple(a if i == s else "inv_log" for i in range(3))
            out += [(acts, False), (acts, True)]
    return out


def activate_inputs(rows: int, later: bool) -> dict:
    def make():
        gen = torch.Generator().manual_seed(23 * rows + int(later))
        rn = lambda *s: torch.randn(*s, generator=gen)
        return {"prev": rn(rows, 9) if later else None, "delta": rn(rows, 9), "dy": rn(rows, 9)}
    return _once(("act_in", rows, later), make)


def activate_oracle(d, dtype=torch.float64, device="cpu", mut=po.NONE, acts=("linear",) * 3):
    return po.with_grads(lambda delta, prev=None: po.activate(prev, delta, acts, mut), {"delta": d["delta"]},
                         {"prev": d["prev"]}, [None, d["dy"]], dtype, device)


def activate_reference(rows, acts, later):
    from functools import partial
    muts = ("relu_everywhere",) + (("no_accumulate",) if later else ())
    return _reference(("act", rows, acts, later), lambda: activate_inputs(rows, later), partial(activate_oracle, acts=acts),
                      muts)


# ---- modules ---------------------------------------------------------------------------------------------------------
MODULES = ("mlp0", "mlp1", "camera")
MODULE_MUTANTS = {"mlp0": ("sum_not_mean", "dec_first", "beta_one", "clamp_min_scale"), "mlp1": (),
                  "camera": ("sigmoid_only", "no_bias", "unbiased", "scale_without_one", "no_gate", "no_residual", "scale",
                             "softmax_over_queries", "relu_everywhere", "no_accumulate")}
MODULE_UNREACHED = {"no_accumulate": ("out0",)}


def golden(name: str, golden_dir) -> dict:
    def make():
        if name == "camera":
            g = torch.load(golden_dir / "posehead_goldens_camera.pt")
            g["weights"] = {**torch.load(golden_dir / "posehead_goldens_camera_weights_0.pt")["weights"],
                            **torch.load(golden_dir / "posehead_goldens_camera_weights_1.pt")["weights"]}
            g["weights"] = {k: g["weights"][k] for k in g["keys"]}
            return g
        return torch.load(golden_dir / "posehead_goldens_mlp.pt")["cases"][int(name[-1])]
    return _once(("golden", name), make)


def flat(result) -> dict:
    """(outputs, input gradients, parameter gradients) -> one {name: tensor}"""
    outs, gi, gp = result
    return {**{f"out{i}": o for i, o in enumerate(outs)}, **{"d_" + k: v for k, v in gi.items()},
            **{"dparam_" + k: v for k, v in gp.items()}}


def module_reference(name: str, golden_dir):
    """(golden, float64 oracle as a flat dict, mutant distances over the outputs and the input gradients)"""
    def make():
        g = golden(name, golden_dir)
        x64 = flat(po.module_case(g))
        per_token = {k: v for k, v in x64.items() if not k.startswith("dparam_")}
        dists = {}
        for m in MODULE_MUTANTS[name]:
            mu = flat(po.module_case(g, mut=frozenset([m])))
            dists[m] = distances({k: mu[k] for k in per_token}, per_token, m, MODULE_UNREACHED)
        return g, x64, dists
    return _once(("module_ref", name), make)


def build_module(name: str, g: dict):
    """This package's module of a golden, with the golden's state dict loaded."""
    from types import SimpleNamespace

    import spfsplatv2_amd as spf
    if name == "camera":
        mod = spf.CameraHead(**g["cfg"])
    else:
        mod = spf.camera_head_factory("mlp", "pose", SimpleNamespace(enc_embed_dim=g["enc_embed_dim"],
                                                                     dec_embed_dim=g["dec_embed_dim"]),
                                      spf.PoseHeadCfg(**g["cfg"]))
    mod.load_state_dict(g["weights"])
    return mod


def run_module(name: str, mod, ins: dict, g: dict) -> list:
    if name == "camera":
        return mod([g["other_tokens"].to(ins["tokens"].device), ins["tokens"]], num_iterations=g["num_iterations"])
    return [mod([ins[k] for k in g["token_order"]])]
