"""Cases of the attention tests that vary what the other attention tests hold constant (TEST INFRASTRUCTURE ONLY):
positions drawn per batch item, scene, view and token, and free ``scale`` / ``base`` / ``F0``.

Shared by tests/test_gpu_attention_params.py (the product on the device) and tests/test_attention_params.py (the power
condition, on the CPU): inputs from seeds, the three oracles behind one call per layout, and the MUTANTS -- the float64
oracle on the positions or the parameter a wrong kernel would read (another item's table, y and x swapped, one key's
position, the default instead of the argument).  A gate is only trusted where every mutant is at least ``POWER`` times
the gate's bound away from the true oracle, in the gate's own norm.
"""
from __future__ import annotations

import torch

from tests import attention_oracle as oracle
from tests import attention_views_oracle as voracle
from tests import vggt_attention_oracle as vggt

NAMES = ("out", "dq", "dk", "dv", "dq_weight", "dq_bias", "dk_weight", "dk_bias")
DEFAULT = (0.125, 100.0, 1.0)                                          # scale, base, F0: what every other test runs
SETTINGS = [(0.2, 100.0, 1.0), (0.125, 10.0, 1.0), (0.125, 100.0, 0.5), (0.07, 1000.0, 2.0)]
POWER = 4.0
NORM_EPS = 1e-5
NEG = float("-inf")
# positions are drawn from [0, POS_RANGE): at bfloat16 eager's own error grows with the angle and the one-key mutant of
# the cross shape is only 2 x the bound on [0, 40), so bfloat16 gets the reference's 18 x 18 patch grid's range
POS_RANGE = {torch.float32: 40, torch.float16: 40, torch.bfloat16: 18}

# name: (B, H, Nq, Nk or None for packed self-attention).  The smallest shapes with a partial last tile, more than one
# owner block and two batch items; 129 x 70: two dq owner blocks with dq, dk != 0
FLAT = {
    "cross_2x2x70_131": (2, 2, 70, 131),
    "packed_2x3x70": (2, 3, 70, None),
    "cross_2x1x129_70": (2, 1, 129, 70),
}
CROSS, PACKED, CROSS129 = FLAT
# name: (b, H, Vq, Vk, Nq, Nk)
VIEWS = {
    "ragged_2x2_2v3_66_70": (2, 2, 2, 3, 66, 70),
    "blk2_2x1_3v4_33_33": (2, 1, 3, 4, 33, 33),
}
RAGGED, BLK2 = VIEWS


def dtype_id(dtype):
    return str(dtype).replace("torch.", "")


def eps_of(dtype):
    """The gate's additive term: one ulp of the type the call computes in."""
    return 2.0 ** -23 if dtype == torch.float32 else torch.finfo(dtype).eps


def views_allow(name):
    if name == RAGGED:                                                  # each query view skips one key view
        return [[s != i + 1 for s in range(3)] for i in range(2)]
    import spfsplatv2_amd as spf
    return [[bool(x) for x in row] for row in spf.decoder_view_sets(4, 1)[1].allow.tolist()]


def _positions(gen, dtype, *shape):
    return torch.randint(0, POS_RANGE[dtype], (*shape, 2), generator=gen)


_INPUTS = {}


def flat_inputs(name, dtype=torch.float32):
    """tests/test_gpu_attention.py:make_inputs' recipe in ``dtype`` with positions drawn per batch item and token (query
    and key tables independent), plus the norm parameters of tests/test_gpu_vggt_attention.py and a [B,1,Nq,Nk] additive
    mask: a random finite bias with a fifth of the keys excluded.  Computed once, never modified."""
    if (name, dtype) in _INPUTS:
        return _INPUTS[name, dtype]
    B, H, Nq, Nk = FLAT[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * POS_RANGE[dtype])
    qpos = _positions(gen, dtype, B, Nq)
    if Nk is None:
        Nk = Nq
        qkv = torch.randn(B, Nq, 3, H, 64, generator=gen).to(dtype)
        t = qkv.transpose(1, 3)
        q, k, v, kpos = t[:, :, 0], t[:, :, 1], t[:, :, 2], qpos
    else:
        kpos, qkv = _positions(gen, dtype, B, Nk), None
        q, k, v = (torch.randn(B, n, H, 64, generator=gen).to(dtype).permute(0, 2, 1, 3) for n in (Nq, Nk, Nk))
    dout = torch.randn(B, Nq, H * 64, generator=gen).to(dtype)
    params = [1.0 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen),
              1.0 + 0.3 * torch.randn(64, generator=gen), 0.1 * torch.randn(64, generator=gen)]
    mask = 2.0 * torch.randn(B, 1, Nq, Nk, generator=gen)
    mask[torch.rand(B, 1, Nq, Nk, generator=gen) < 0.2] = NEG
    assert bool((mask > NEG).any(-1).all())                             # every row keeps a key
    assert not torch.equal(qpos[0], qpos[1]) and not torch.equal(kpos[0], kpos[1])
    inp = {"qkv": qkv, "q": q, "k": k, "v": v, "qpos": qpos, "kpos": kpos, "dout": dout, "params": params, "mask": mask}
    _INPUTS[name, dtype] = inp
    return inp


def views_inputs(name, dtype=torch.float32):
    """tests/test_gpu_attention_views.py:make_inputs' recipe (q the [:, 1:] slice of a buffer with one view more, all
    three token-major) with positions drawn per scene, view and token.  Computed once, never modified."""
    if (name, dtype) in _INPUTS:
        return _INPUTS[name, dtype]
    b, H, Vq, Vk, Nq, Nk = VIEWS[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)) + 1000 * POS_RANGE[dtype])
    qpos, kpos = _positions(gen, dtype, b, Vq, Nq), _positions(gen, dtype, b, Vk, Nk)
    q_all = torch.randn(b, Vq + 1, Nq, H, 64, generator=gen).to(dtype)
    k = torch.randn(b, Vk, Nk, H, 64, generator=gen).to(dtype).transpose(2, 3)
    v = torch.randn(b, Vk, Nk, H, 64, generator=gen).to(dtype).transpose(2, 3)
    dout = torch.randn(b, Vq, Nq, H * 64, generator=gen).to(dtype)
    inp = {"q_all": q_all, "q": q_all[:, 1:].transpose(2, 3), "k": k, "v": v, "qpos": qpos, "kpos": kpos, "dout": dout,
           "allow": views_allow(name)}
    _INPUTS[name, dtype] = inp
    return inp


def _to(t, device):
    return None if t is None else t.to(device)


def flat_oracle(inp, variant="plain", *, cfg=DEFAULT, dtype=torch.float64, device="cpu", qpos=None, kpos=None,
                rope=True):
    """(out, dq, dk, dv[, dq_weight, dq_bias, dk_weight, dk_bias]) of the reference's expression in ``dtype`` on
    ``device``.  variant: plain (tests/attention_oracle.py), mask, norm, mask_norm (tests/vggt_attention_oracle.py);
    qpos / kpos: the tables to use instead of the inputs' (the mutants)."""
    scale, base, F0 = cfg
    qpos = _to(inp["qpos"] if qpos is None else qpos, device) if rope else None
    kpos = _to(inp["kpos"] if kpos is None else kpos, device) if rope else None
    q, k, v, dout = (inp[n].to(device) for n in ("q", "k", "v", "dout"))
    if variant == "plain":
        return oracle.core_with_grads(q, k, v, qpos, kpos, dout, base, scale, dtype, F0)
    mask = inp["mask"].to(device) if "mask" in variant else None
    qn = kn = None
    if "norm" in variant:
        p = [t.to(device) for t in inp["params"]]
        qn, kn = (p[0], p[1], NORM_EPS), (p[2], p[3], NORM_EPS)
    res = vggt.core_with_grads(q, k, v, qpos, kpos, dout, mask, qn, kn, base, scale, dtype, None, F0)
    return tuple(t for t in res if t is not None)


def views_oracle(inp, *, cfg=DEFAULT, dtype=torch.float64, device="cpu", qpos=None, kpos=None):
    """(out, dq, dk, dv) of the oracle on gathered keys (tests/attention_views_oracle.py)."""
    scale, base, F0 = cfg
    qpos = _to(inp["qpos"] if qpos is None else qpos, device)
    kpos = _to(inp["kpos"] if kpos is None else kpos, device)
    q, k, v, dout = (inp[n].to(device) for n in ("q", "k", "v", "dout"))
    return voracle.core_views_with_grads(q, k, v, qpos, kpos, inp["allow"], dout, base, scale, dtype, F0)


# ---- mutants ---------------------------------------------------------------------------------------------------------
def position_mutants(inp):
    """name -> (qpos, kpos) as a kernel with one wrong position offset would read them."""
    qpos, kpos = inp["qpos"], inp["kpos"]
    one = kpos.clone()
    m = {"qpos of the other item": (qpos.roll(1, 0), kpos),
         "kpos of the other item": (qpos, kpos.roll(1, 0)),
         "kpos y and x swapped": (qpos, kpos.flip(-1))}
    if kpos.dim() == 4:
        m["qpos of another view"] = (qpos.roll(1, 1), kpos)
        m["kpos of another view"] = (qpos, kpos.roll(1, 1))
        # the last key anybody reads: the last token of the last key view some query view is allowed, last scene
        view = max(s for row in inp["allow"] for s, on in enumerate(row) if on)
        assert not torch.equal(one[-1, view, -1], one[0, view, -1])
        one[-1, view, -1] = one[0, view, -1]
    else:
        assert not torch.equal(one[-1, -1], one[0, -1])
        one[-1, -1] = one[0, -1]
    m["one key's position"] = (qpos, one)
    return m


def parameter_mutants(cfg, rope=True):
    """name -> (scale, base, F0) with ONE parameter that differs from the default put back to its default: what a kernel
    that hard-codes it computes."""
    m = {}
    for i, n in enumerate(("scale", "base", "F0")):
        if cfg[i] != DEFAULT[i] and (rope or i == 0):
            m[f"{n} {DEFAULT[i]:g} for {cfg[i]:g}"] = cfg[:i] + (DEFAULT[i],) + cfg[i + 1:]
    return m


def errs(got, want):
    """The gates' norm: max|x - x64| / max|x64| per tensor (no tensor of these cases is identically zero)."""
    res = []
    for g, w in zip(got, want):
        den = float(w.abs().max())
        assert den > 0.0
        res.append(float((g.detach().double().cpu() - w).abs().max()) / den)
    return res


def mutant_distances(x64, run, mutants, positions):
    """name -> per-tensor distance of each mutant's float64 oracle from the true one; run(**kw) evaluates the oracle."""
    out = {}
    for name, m in mutants.items():
        kw = {"qpos": m[0], "kpos": m[1]} if positions else {"cfg": m}
        out[name] = errs(run(**kw), x64)
    return out


def power_failures(label, dists, e_eager, eps, names=NAMES):
    """The power condition: every mutant, in every tensor, at least POWER x the gate's bound 2 * eager + eps away.
    Returns the offenders as text (empty: the gate can be trusted) and prints the tightest ratio."""
    bad, tight = [], (float("inf"), "")
    for name, d in dists.items():
        for n, x, e in zip(names, d, e_eager):
            bound = 2 * e + eps
            tight = min(tight, (x / bound, f"{name}, {n}"))
            if x < POWER * bound:
                bad.append(f"{label}: mutant '{name}' moves {n} by {x:.3e} < {POWER:g} x bound {bound:.3e}")
    if dists:
        print(f"{label} power: tightest mutant / bound = {tight[0]:.1f} ({tight[1]})")
    return bad


_REF = {}


def reference(layout, name, variant, dtype, cfg=DEFAULT, rope=True):
    """(inputs drawn in ``dtype``, run, float64 oracle on exactly those, mutant distances) of one run of the tests;
    run(**kw) evaluates the oracle of that run (dtype, device, qpos, kpos, cfg).  At the default parameters the mutants
    are the position mutants, elsewhere the parameter mutants.  Computed once, never modified."""
    key = (layout, name, variant, dtype, cfg, rope)
    if key not in _REF:
        if layout == "views":
            inp = views_inputs(name, dtype)
            run = lambda **kw: views_oracle(inp, **{"cfg": cfg, **kw})
        else:
            inp = flat_inputs(name, dtype)
            run = lambda **kw: flat_oracle(inp, variant, **{"cfg": cfg, "rope": rope, **kw})
        x64 = run()
        if cfg == DEFAULT:
            dists = mutant_distances(x64, run, position_mutants(inp), True)
        else:
            dists = mutant_distances(x64, run, parameter_mutants(cfg, rope), False)
        _REF[key] = (inp, run, x64, dists)
    return _REF[key]


F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (layout, case, variant, dtype) of the distinct-position runs; a 16-bit dtype: the ``matrix16`` call
POSITION_RUNS = [("flat", n, "plain", F32) for n in FLAT]
POSITION_RUNS += [("flat", n, v, F32) for n in (CROSS, PACKED) for v in ("mask", "norm", "mask_norm")]
POSITION_RUNS += [("views", n, "plain", F32) for n in VIEWS]
POSITION_RUNS += [("flat", n, "plain", d) for n in FLAT for d in (F16, BF16)]
# the same at each of SETTINGS
PARAMETER_RUNS = [("flat", n, v, F32) for v in ("plain", "mask_norm") for n in (CROSS, PACKED)]
PARAMETER_RUNS += [("views", RAGGED, "plain", F32)]
PARAMETER_RUNS += [("flat", n, "plain", d) for n in (CROSS, PACKED) for d in (F16, BF16)]
NOROPE_SCALE = (0.2, 100.0, 1.0)


def run_id(r):
    return "-".join(x if isinstance(x, str) else dtype_id(x) if isinstance(x, torch.dtype) else
                    "s%g_b%g_f%g" % x for x in r if x != "flat")


# ---- modules ---------------------------------------------------------------------------------------------------------
MODULE_ROPE = (10.0, 0.5)                                               # cuRoPE2D(freq, F0) of the module tests
MODULE_DIM, MODULE_HEADS = 128, 2


def module_case(kind, dtype=torch.float32):
    """Random weights (C = 128, H = 2, biases on) and inputs of ``Attention`` (self), ``CrossAttention`` (cross) or
    ``CrossAttention.forward_views`` (views), drawn in float32 and rounded to ``dtype`` (kept as float32 values): what the
    module and the float64 oracle both start from.  Positions per batch item / scene / view.  Computed once."""
    if ("module", kind, dtype) in _INPUTS:
        return _INPUTS["module", kind, dtype]
    C = MODULE_DIM
    gen = torch.Generator().manual_seed(sum(map(ord, kind)) + 1000 * POS_RANGE[dtype])
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dtype).float()
    lin = lambda o: (rnd(o, C) / C ** 0.5, 0.1 * rnd(o))
    w = {}
    for p, o in ([("qkv", 3 * C)] if kind == "self" else [("projq", C), ("projk", C), ("projv", C)]) + [("proj", C)]:
        w[p + ".weight"], w[p + ".bias"] = lin(o)
    w = {k: t.to(dtype).float() for k, t in w.items()}
    if kind == "self":
        B, _, N, _ = FLAT[PACKED]
        ins, pos = {"x": rnd(B, N, C)}, {"xpos": _positions(gen, dtype, B, N)}
    elif kind == "cross":
        B, _, Nq, Nk = FLAT[CROSS]
        ins = {"query": rnd(B, Nq, C), "memory": rnd(B, Nk, C)}
        pos = {"qpos": _positions(gen, dtype, B, Nq), "kpos": _positions(gen, dtype, B, Nk)}
    else:
        b, _, Vq, Vk, Nq, Nk = VIEWS[RAGGED]
        ins = {"query": rnd(b, Vq, Nq, C), "key": rnd(b, Vk, Nk, C)}
        pos = {"qpos": _positions(gen, dtype, b, Vq, Nq), "kpos": _positions(gen, dtype, b, Vk, Nk)}
    case = {"kind": kind, "weights": w, "inputs": ins, "pos": pos, "allow": views_allow(RAGGED)}
    _INPUTS["module", kind, dtype] = case
    return case


def module_oracle(case, dtype=torch.float64, device="cpu", rope=MODULE_ROPE):
    """(out, {name: gradient}) of oracle.self_attention / cross_attention / module_views in ``dtype`` on ``device`` for
    the inputs AND the parameters; the upstream gradient is the output itself (tests/test_gpu_attention16.py)."""
    base, F0 = rope
    w = {k: t.to(device=device, dtype=dtype).requires_grad_(True) for k, t in case["weights"].items()}
    ins = {k: t.to(device=device, dtype=dtype).requires_grad_(True) for k, t in case["inputs"].items()}
    pos = {k: t.to(device) for k, t in case["pos"].items()}
    if case["kind"] == "self":
        out = oracle.self_attention(ins["x"], pos["xpos"], w, MODULE_HEADS, base, F0)
    elif case["kind"] == "cross":
        out = oracle.cross_attention(ins["query"], ins["memory"], ins["memory"], pos["qpos"], pos["kpos"], w, MODULE_HEADS,
                                     base, F0)
    else:
        out = voracle.module_views(ins["query"], ins["key"], pos["qpos"], pos["kpos"], case["allow"], w, MODULE_HEADS, base,
                                   F0)
    wrt = {**ins, **w}
    grads = torch.autograd.grad(out, list(wrt.values()), out.detach())
    return out.detach(), dict(zip(wrt, grads))


def module_tensors(result, names):
    """(out, {name: gradient}) as the tuple of tensors in the order of ``names``."""
    out, grads = result
    return tuple(out if n == "out" else grads[n] for n in names)


def module_reference(kind, dtype):
    """(case, tensor names, float64 oracle, mutant distances) of a module run; the mutants: the oracle at the default base
    and at the default F0.  Computed once, never modified."""
    key = ("module", kind, dtype)
    if key not in _REF:
        case = module_case(kind, dtype)
        names = ("out",) + tuple(case["inputs"]) + tuple(case["weights"])
        x64 = module_tensors(module_oracle(case), names)
        mutants = {"base 100 for 10": (DEFAULT[1], MODULE_ROPE[1]), "F0 1 for 0.5": (MODULE_ROPE[0], DEFAULT[2])}
        dists = {m: errs(module_tensors(module_oracle(case, rope=r), names), x64) for m, r in mutants.items()}
        _REF[key] = (case, names, x64, dists)
    return _REF[key]
