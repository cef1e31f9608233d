"""Shapes, inputs, float64 references and the gate of the encoder-tail tests (tests/test_tail.py on the CPU,
tests/test_gpu_tail.py on the device).  TEST INFRASTRUCTURE ONLY.  Every reference is computed once and never modified.

Gate and power condition: those of tests/block_cases.py, taken from there as they stand -- per tensor
err = max|x - x64| / max|x64| against the float64 oracle must not exceed twice the err of float32 eager torch plus one
float32 ulp, and every mutant of tests/tail_oracle.py is at least 4 such bounds away in every gated tensor its mutated
quantity enters (UNREACHED lists, per mutant, the tensors it does not enter).

Gated tensors.  The five outputs as they are.  The gradient to the head outputs is gated per channel group, because the
groups differ in scale by orders of magnitude: ``d_density`` (channel 0), ``d_scale`` (1:4), ``d_quat`` (4:8), ``d_sh``
(8:) -- and ``d_quat_tiny``, the quaternion channels of the pinned near-zero quaternions alone, whose gradient g / eps is
1e8 times everyone else's (they are zeroed in ``d_quat``).  ``d_pts`` is the gradient to the point maps.

Inputs.  Logits 3 randn clamped to [-12, 12]; scale channels 4 randn; quaternions and harmonics standard normal; points
and upstream gradients standard normal.  Pinned, on the first Gaussians of view 0 (as many as the case has): logit -12
with scale channels 25 (softplus's linear branch) and 400 (the 0.3 clamp), logit 12, logit 0, a quaternion of norm 1e-9
and an exact zero quaternion.

Mutants that a case cannot see are not asked of it: ``inv_exponent`` at e = 1, ``view_major`` at v = 1 or hw = 1,
``sh_transposed`` and ``no_mask`` at K = 1 (the mask is [1]), ``eps_inside_sqrt`` without the pinned quaternions (with
|q| of order 1 it moves a rotation by 1e-8).

Tiles.  The kernels take 64 pixels per block and use 16-byte accesses where hw % 4 == 0.  (h, w): (1, 1) one pixel;
(1, 5) and (3, 7) scalar tails; (8, 8) exactly one tile, vector path; (5, 13) a tile plus one, scalar; (4, 17) a tile
plus four, vector path with a partial tile; (16, 20) five tiles.
"""
from __future__ import annotations

import torch

from tests import block_cases
from tests import tail_oracle as to

ULP, POWER = block_cases.ULP, block_cases.POWER
gate, power_failures = block_cases.gate, block_cases.power_failures

EPS = 1e-8
HW = ((1, 1), (1, 5), (3, 7), (8, 8), (5, 13), (4, 17), (16, 20))
DEGREES = (0, 1, 2, 3, 4)
EXPONENTS = (1.0, 0.5, 2.0, 2.0 ** 1.5)
GRADS = ("d_pts", "d_density", "d_scale", "d_quat", "d_quat_tiny", "d_sh")
ALL = to.OUTPUTS + GRADS
_OPACITY = ("opacities", "d_density")
_SH = ("harmonics", "d_sh")
REACHED = {"inv_exponent": _OPACITY, "no_half": _OPACITY, "no_sigmoid": _OPACITY, "view_major": ALL,
           "channel_off_by_one": ("scales", "rotations", "harmonics", "d_density", "d_scale", "d_quat", "d_quat_tiny", "d_sh"),
           "sh_transposed": _SH, "no_mask": _SH, "clamp_min": ("scales", "d_scale"),
           "eps_inside_sqrt": ("rotations", "d_quat_tiny")}
UNREACHED = {m: tuple(k for k in ALL if k not in r) for m, r in REACHED.items()}


def covering_cases():
    """Every (h, w) with every K once, b, v and the exponent cycled; (b, v, (h, w), sh_degree, exponent)."""
    out = []
    for i, hw in enumerate(HW):
        for j, deg in enumerate(DEGREES):
            n = i * len(DEGREES) + j
            out.append((1 + n % 2, 1 + (n + i) % 3, hw, deg, EXPONENTS[(n + j) % 4]))
    return out


SPLIT_CASES = ((2, 2, (1, 1), 4, 0.5), (1, 3, (3, 7), 4, 2.0), (2, 1, (8, 8), 4, 1.0), (1, 2, (5, 13), 4, 2.0 ** 1.5),
               (1, 2, (4, 17), 4, 0.5), (2, 3, (16, 20), 4, 2.0))
ABSENT_CASE = (2, 2, (5, 13), 4, 2.0)
GOLDEN_CASE_SHAPE = (2, 2, (3, 5))

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_id(case) -> str:
    b, v, (h, w), deg, e = case
    return f"b{b}v{v}_{h}x{w}_deg{deg}_e{e:.3g}"


def loop_case(cap: int):
    """Three more 64-pixel tiles than the grid holds blocks, K = 1 (11 channels: 12 MB at a cap of 4,096)."""
    return (1, 1, (cap + 3, 64), 0, 2.0)


def mutants(case, pinned_quats: bool):
    b, v, (h, w), deg, e = case
    m = ["no_half", "no_sigmoid", "channel_off_by_one", "clamp_min"]
    if e != 1.0:
        m.append("inv_exponent")
    if v > 1 and h * w > 1:
        m.append("view_major")
    if deg > 0:
        m += ["sh_transposed", "no_mask"]
    if pinned_quats:
        m.append("eps_inside_sqrt")
    return tuple(m)


def inputs(case) -> dict:
    """{"pts": v x [b, h, w, 3], "raw": v x [b, C, h, w], "ups": {output: tensor}, "tiny": bool [v, b, h, w]}"""
    def make():
        b, v, (h, w), deg, e = case
        K = (deg + 1) ** 2
        C = 8 + 3 * K
        gen = torch.Generator().manual_seed(1000 * h + 10 * w + 100 * deg + v + 7 * b)
        rn = lambda *s: torch.randn(*s, generator=gen)
        raw = rn(v, b, C, h * w)
        raw[:, :, 0] = (3.0 * raw[:, :, 0]).clamp(-12.0, 12.0)
        raw[:, :, 1:4] *= 4.0
        tiny = torch.zeros(v, b, h * w, dtype=torch.bool)
        slots = [(bi, p) for bi in range(b) for p in range(h * w)]          # of view 0
        pins = [{0: -12.0, 1: 25.0, 2: 400.0}, {0: 12.0}, {0: 0.0}]
        for (bi, p), pin in zip(slots, pins):
            for c, val in pin.items():
                raw[0, bi, c, p] = val
        if len(slots) >= 5:
            (b3, p3), (b4, p4) = slots[3], slots[4]
            raw[0, b3, 4:8, p3] = torch.tensor([6e-10, -8e-10, 0.0, 0.0])
            raw[0, b4, 4:8, p4] = 0.0
            tiny[0, b3, p3] = tiny[0, b4, p4] = True
        G = v * h * w
        ups = {"means": rn(b, G, 3), "opacities": rn(b, G), "scales": rn(b, G, 3), "rotations": rn(b, G, 4),
               "harmonics": rn(b, G, 3, K)}
        return {"pts": [rn(b, h, w, 3) for _ in range(v)], "raw": [raw[i].reshape(b, C, h, w).clone() for i in range(v)],
                "ups": ups, "tiny": tiny.reshape(v, b, h, w)}
    return _once(("in", case), make)


def split(res: dict, tiny) -> dict:
    """The result of ``tail_oracle.tail_with_grads`` (or the product's, in the same form) as the gated tensors."""
    out = {k: res[k] for k in to.OUTPUTS}
    if "d_raw" in res:
        d = res["d_raw"]
        t = tiny.to(d.device)[:, :, None]
        out.update({"d_pts": res["d_pts"], "d_density": d[:, :, 0], "d_scale": d[:, :, 1:4],
                    "d_quat": d[:, :, 4:8].masked_fill(t, 0.0), "d_sh": d[:, :, 8:]})
        if bool(tiny.any()):
            out["d_quat_tiny"] = d[:, :, 4:8].movedim(2, -1)[tiny.to(d.device)]
    return out


def oracle(case, d: dict, dtype=torch.float64, device="cpu", mut=to.NONE, ups=None, opacity=to.opacity_stable) -> dict:
    b, v, hw, deg, e = case
    res = to.tail_with_grads(d["pts"], d["raw"], d["ups"] if ups is None else ups, e, deg, EPS, dtype, device, mut, opacity)
    return split(res, d["tiny"])


def distances(mutant: dict, x64: dict, name: str) -> dict:
    return {k: to.rel_err(mutant[k], x64[k]) for k in x64 if k not in UNREACHED[name]}


def reference(case, muts=None):
    """(inputs, float64 oracle, {mutant: {tensor: distance}})"""
    def make():
        d = inputs(case)
        x64 = oracle(case, d)
        names = mutants(case, bool(d["tiny"].any())) if muts is None else muts
        return d, x64, {m: distances(oracle(case, d, mut=frozenset([m])), x64, m) for m in names}
    return _once(("ref", case, muts), make)


def golden(golden_dir) -> dict:
    return _once("golden", lambda: torch.load(golden_dir / "tail_goldens.pt"))
