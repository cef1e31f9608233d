"""Shapes, inputs, float64 references and the gate of the DPT-head tests (tests/test_dpt.py on the CPU,
tests/test_gpu_dpt.py on the device).  TEST INFRASTRUCTURE ONLY.  Every reference is computed once and never modified.

Gate and power condition: those of tests/block_cases.py, taken from there as they stand -- per tensor
err = max|x - x64| / max|x64| against the float64 oracle must not exceed twice the err of float32 eager torch plus one
float32 ulp, and every mutant of tests/dpt_oracle.py is at least 4 such bounds away in every gated tensor its mutated
quantity enters.  It does not enter -- so nothing is asked of -- the tensors of UNREACHED, and:
  * ``no_align_corners`` on a 1 x 1 plane (either rule gives the constant plane),
  * ``clip6`` without a pixel of d < 1e-6 (the module goldens have none), and in the points themselves, which are of the
    order d there and vanish against the other pixels,
  * ``exp`` and ``no_conf_offset`` in each other's output,
  * ``relu_wrong`` in ``db`` and ``dc`` of add_relu at n = 1: the single sum must be positive for y to have a scale at
    all, and then the gradient of an addend the mutant leaves outside its ReLU is the upstream gradient either way.

Modules.  The forward of a head goes through the gate as it runs, in float32 throughout.  Its backward does not: the
gradients come out of torch's float32 convolution backward, which on the device does not return the same floats from
run to run for either side (two runs of one eager head differ by 1e-2 of a parameter gradient's largest entry at the
reference's shape), and a bound of twice one draw of that noise is not a test.  The backward is gated with the
convolutions made exact instead (``float32_kernel_sites`` and ``dpt_oracle.module_case(.., mixed=True)``): the head in
float64, the kernels of csrc/dpt.hip -- and, on the eager side, the torch operations they replace -- in float32 at the
places where the product calls them.  Every output, input gradient and parameter gradient is gated, by the same rule,
and what the gate then measures is the kernels' float32 error alone.  IN ADDITION to the gate, not in its place, the
all-float32 outputs and gradients are held against the reference's own floats in the goldens at GOLDEN_OUT_TOL = 2e-6
and GOLDEN_GRAD_TOL = 5e-6, the tolerances tests/test_dpt.py holds the float64 oracle to (the float32 rounding of the
reference's own run).  These two are not the acceptance rule and are not to be widened to make a failure go away: a
gradient the kernels get wrong fails the gate of the exact-convolution test first.

Inputs.  Upsample: standard normal x and upstream gradient; skip standard normal with exact zeros and negatives.
add_relu: standard normal addends; element 0 is (-0.7, 1.2) or (-0.7, 0.5, 0.9): a sum above zero on a first addend --
and on a sum of two -- below it, which tells the ReLU of the sum from the ReLU of an addend and the sum of three from
the sum of two even at n = 1; element 1 sums to an exact zero.  Points: xyz
standard normal (d around 1.7), pixel 0 of batch item 0 at d = 0, pixel 0 of item 1 at d = 1e-9 and, with finite bounds
(0.5, 100) and more than one pixel, pixel 1 of item 0 at d = 60: below, inside and above the bounds; the confidence
logit standard normal against a span of 2 with finite bounds, so the clip is active on about a quarter of the pixels.
"""
from __future__ import annotations

import contextlib

import torch

from tests import block_cases
from tests import dpt_oracle as do

ULP, POWER = block_cases.ULP, block_cases.POWER
gate, power_failures = block_cases.gate, block_cases.power_failures
INF = float("inf")

GOLDEN_OUT_TOL, GOLDEN_GRAD_TOL = 2e-6, 5e-6
UP_SHAPES = ((1, 1, 1, 1), (2, 3, 1, 5), (1, 2, 5, 1), (2, 3, 5, 7), (1, 4, 16, 16), (1, 2, 3, 258))
# (skip given, relu_skip)
UP_VARIANTS = {"plain": (False, False), "skip": (True, False), "relu_skip": (True, True)}
ADD_SIZES = (1, 5, 4 * 64 * 4 + 3)
# (addends, ds given)
ADD_VARIANTS = {"a": (1, False), "ab": (2, False), "ab_ds": (2, True), "abc": (3, False), "abc_ds": (3, True)}
POINT_SIZES = ((1, 1), (5, 7), (32, 48))
POINT_B = 2
# (conf, finite bounds)
POINT_VARIANTS = {"plain": (False, False), "conf": (True, False), "bounds": (False, True), "conf_bounds": (True, True)}
DEPTH_BOUNDS, CONF_BOUNDS = (0.5, 100.0), (1.0, 3.0)
UNREACHED = {"no_align_corners": ("dskip",), "relu_wrong": ("s",), "no_third": (), "exp": ("conf",),
             "clip6": ("pts3d", "conf"), "no_conf_offset": ("pts3d", "din")}

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def loop_shape(cap: int):
    """Three more 2 x 2 planes than the upsample kernels' grid holds blocks: the plane loop takes a second round."""
    return (1, cap + 3, 2, 2)


def add_loop_size(cap: int) -> int:
    """More floats than one pass of the capped add_relu grid covers (256 lanes of 4 floats per block), and a tail."""
    return cap * 256 * 4 + 5


def errors(got: dict, x64: dict) -> dict:
    assert sorted(got) == sorted(x64), (sorted(got), sorted(x64))
    return {k: do.rel_err(got[k], x64[k]) for k in x64}


def distances(mutant: dict, x64: dict, name: str) -> dict:
    return {k: do.rel_err(mutant[k], x64[k]) for k in x64 if k not in UNREACHED[name]}


# ---- upsample --------------------------------------------------------------------------------------------------------
def up_mutants(shape, variant: str):
    muts = [] if shape[2] == shape[3] == 1 else ["no_align_corners"]
    return tuple(muts + (["relu_wrong"] if variant == "relu_skip" else []))


def up_inputs(shape, variant: str) -> dict:
    has_skip, _ = UP_VARIANTS[variant]

    def make():
        B, C, h, w = shape
        gen = torch.Generator().manual_seed(7 * h + 131 * w + C)
        d = {"x": torch.randn(B, C, h, w, generator=gen), "dy": torch.randn(B, C, 2 * h, 2 * w, generator=gen), "skip": None}
        if has_skip:
            skip = torch.randn(B, C, 2 * h, 2 * w, generator=gen)
            skip.view(-1)[::3] = 0.0                     # exact zeros; the rest has both signs
            skip.view(-1)[1] = -0.75
            d["skip"] = skip
        return d
    return _once(("up_in", shape, variant), make)


def up_oracle(d: dict, variant: str, dtype=torch.float64, device="cpu", mut=do.NONE) -> dict:
    return do.upsample_with_grads(d["x"], d["skip"], UP_VARIANTS[variant][1], d["dy"], dtype, device, mut)


def up_reference(shape, variant: str):
    """(inputs, float64 oracle, {mutant: {tensor: distance}})"""
    def make():
        d = up_inputs(shape, variant)
        x64 = up_oracle(d, variant)
        return d, x64, {m: distances(up_oracle(d, variant, mut=frozenset([m])), x64, m) for m in up_mutants(shape, variant)}
    return _once(("up_ref", shape, variant), make)


# ---- add_relu --------------------------------------------------------------------------------------------------------
def add_mutants(variant: str):
    return {1: (), 2: ("relu_wrong",), 3: ("relu_wrong", "no_third")}[ADD_VARIANTS[variant][0]]


def add_inputs(n: int, variant: str) -> dict:
    addends, has_ds = ADD_VARIANTS[variant]

    def make():
        gen = torch.Generator().manual_seed(3 * n + addends)
        t = [torch.randn(n, generator=gen) for _ in range(3)]
        for v, first in zip(t, (-0.7, 1.2, 0.0) if addends == 2 else (-0.7, 0.5, 0.9)):
            v[0] = first
        if addends == 1:
            t[0][0] = 0.6
        if n > 1:
            t[0][1], t[1][1], t[2][1] = (0.0, 0.0, 0.0) if addends == 1 else (0.5, -0.5, 0.0)
        d = {"a": t[0], "b": t[1] if addends > 1 else None, "c": t[2] if addends > 2 else None,
             "dy": torch.randn(n, generator=gen), "ds": torch.randn(n, generator=gen) if has_ds else None}
        return d
    return _once(("add_in", n, variant), make)


def add_oracle(d: dict, dtype=torch.float64, device="cpu", mut=do.NONE) -> dict:
    return do.add_relu_with_grads(d["a"], d["b"], d["c"], d["dy"], d["ds"], dtype, device, mut)


def add_reference(n: int, variant: str):
    def make():
        d = add_inputs(n, variant)
        x64 = add_oracle(d)
        dists = {m: distances(add_oracle(d, mut=frozenset([m])), x64, m) for m in add_mutants(variant)}
        if n == 1 and "relu_wrong" in dists:
            dists["relu_wrong"] = {k: v for k, v in dists["relu_wrong"].items() if k not in ("db", "dc")}
        return d, x64, dists
    return _once(("add_ref", n, variant), make)


# ---- points ----------------------------------------------------------------------------------------------------------
def point_modes(variant: str):
    conf, bounds = POINT_VARIANTS[variant]
    depth = ("exp",) + (DEPTH_BOUNDS if bounds else (-INF, INF))
    return depth, ((("exp",) + (CONF_BOUNDS if bounds else (1.0, INF))) if conf else None)


def point_mutants(variant: str):
    return ("exp", "clip6") + (("no_conf_offset",) if POINT_VARIANTS[variant][0] else ())


def point_inputs(hw, variant: str) -> dict:
    conf, bounds = POINT_VARIANTS[variant]

    def make():
        H, W = hw
        gen = torch.Generator().manual_seed(17 * H + W)
        out = torch.randn(POINT_B, 4 if conf else 3, H, W, generator=gen)
        flat = out.view(POINT_B, out.shape[1], H * W)
        flat[0, :3, 0] = 0.0
        flat[1, :3, 0] = torch.tensor([6e-10, -8e-10, 0.0])
        if bounds and H * W > 1:
            flat[0, :3, 1] = torch.tensor([36.0, -48.0, 0.0])
        return {"out": out, "dpts": torch.randn(POINT_B, H, W, 3, generator=gen),
                "dconf": torch.randn(POINT_B, H, W, generator=gen) if conf else None}
    return _once(("pt_in", hw, variant), make)


def point_oracle(d: dict, variant: str, dtype=torch.float64, device="cpu", mut=do.NONE) -> dict:
    depth, conf = point_modes(variant)
    return do.points_with_grads(d["out"], depth, conf, d["dpts"], d["dconf"], dtype, device, mut)


def point_reference(hw, variant: str):
    def make():
        d = point_inputs(hw, variant)
        x64 = point_oracle(d, variant)
        return d, x64, {m: distances(point_oracle(d, variant, mut=frozenset([m])), x64, m) for m in point_mutants(variant)}
    return _once(("pt_ref", hw, variant), make)


# ---- modules ---------------------------------------------------------------------------------------------------------
KINDS = ("pts", "gs")
MODULE_MUTANTS = {"pts": ("no_align_corners", "relu_wrong", "no_third", "exp", "no_conf_offset"),
                  "gs": ("no_align_corners", "relu_wrong", "no_third")}
MODULE_UNREACHED = {"exp": ("conf",), "no_conf_offset": ("pts3d",)}
# refinenet4 has one input, so its resConfUnit1 takes no part in a forward: no gradient, nothing to gate
IDLE = "scratch.refinenet4.resConfUnit1."


def golden(kind: str, golden_dir) -> dict:
    return _once(("golden", kind), lambda: torch.load(golden_dir / f"dpt_goldens_{kind}.pt"))


def flat(result) -> dict:
    """({output}, input gradients, parameter gradients) -> one {name: tensor}, without the idle parameters"""
    outs, gi, gp = result
    return {**outs, **{"d_" + k: v for k, v in gi.items()},
            **{"dparam_" + k: v for k, v in gp.items() if not k.startswith(IDLE)}}


def module_reference(kind: str, golden_dir):
    """(golden, float64 oracle as a flat dict, mutant distances over the outputs and the input gradients)"""
    def make():
        g = golden(kind, golden_dir)
        x64 = flat(do.module_case(g))
        per_pixel = [k for k in x64 if not k.startswith("dparam_")]
        dists = {}
        for m in MODULE_MUTANTS[kind]:
            mu = flat(do.module_case(g, mut=frozenset([m])))
            dists[m] = {k: do.rel_err(mu[k], x64[k]) for k in per_pixel if k not in MODULE_UNREACHED.get(m, ())}
        return g, x64, dists
    return _once(("module_ref", kind), make)


def build_module(kind: str, g: dict):
    """This package's head of a golden, with the golden's state dict loaded (strict)."""
    import spfsplatv2_amd as spf
    if kind == "pts":
        mod = spf.PixelwiseTaskWithDPT(num_channels=g["num_channels"], postprocess=spf.postprocess,
                                       depth_mode=g["depth_mode"], conf_mode=g["conf_mode"], head_type="regression", **g["args"])
    else:
        mod = spf.PixelwiseTaskWithGSDPT(num_channels=g["num_channels"], postprocess=None, head_type="gs_params", **g["args"])
    mod.load_state_dict(g["weights"])
    return mod.eval()


@contextlib.contextmanager
def float32_kernel_sites(mod):
    """Inside: ``mod`` (a float64 copy of a head) calls the kernels of csrc/dpt.hip in float32 -- a cast down before
    upsample2x, add_relu and postprocess and a cast up after -- and everything else, the convolutions first of all, runs in
    float64: the product's side of ``dpt_oracle.module_case(.., mixed=True)``."""
    from spfsplatv2_amd import heads
    real = {n: getattr(heads, n) for n in ("add_relu", "upsample2x", "_check_float32")}
    down = lambda t: t.float() if isinstance(t, torch.Tensor) else t

    def add_relu(a, b=None, c=None):
        s, y = real["add_relu"](down(a), down(b), down(c))
        return (a if b is None else s.double()), y.double()

    def upsample2x(x, skip=None, relu_skip=False):
        return real["upsample2x"](down(x), down(skip), relu_skip).double()

    def postprocess(out, depth_mode, conf_mode):
        return {k: v.double() for k, v in post(out.float(), depth_mode, conf_mode).items()}
    post = mod.postprocess
    heads.add_relu, heads.upsample2x, heads._check_float32 = add_relu, upsample2x, lambda *a: None
    if post is not None:
        mod.postprocess = postprocess
    try:
        yield mod
    finally:
        heads.add_relu, heads.upsample2x, heads._check_float32 = real["add_relu"], real["upsample2x"], real["_check_float32"]
        mod.postprocess = post


def run_module(kind: str, mod, ins: dict, image_size) -> dict:
    tokens = [ins[f"tok{i}"] for i in range(4)]
    if kind == "pts":
        return mod(tokens, image_size)
    return {"out": mod(tokens, ins["img"], image_size)}
