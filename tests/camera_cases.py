"""Cameras, sizes, float64 references and the gate of the camera tests (tests/test_camera.py on the CPU,
tests/test_gpu_camera.py on the device).  TEST INFRASTRUCTURE ONLY.  Every reference is computed once and never modified.

Cameras.  Three seeded families of 300 renders; a case of R renders takes a family's first R.
  general    rotations from random unit quaternions, with the identity, a turn of pi - 1e-3 and a turn of pi among the
             first three; translation length log-uniform in [0.01, 5]; near log-uniform in [0.05, 0.5] (even renders) and
             [2, 10] (odd renders) -- never near 1, so that a missed 1/near shows on every render; far / near log-uniform
             in [1.01, 1e4]; fx, fy independent, log-uniform in [0.25, 200] (about 127 degrees down to 0.3 degrees);
             cx, cy in 0.5 +- 0.15; skew 0.02 fx N(0, 1).
  centred    the same poses and depths under the synthetic camera: cx = cy = 0.5, no skew (fx, fy over the whole range).
  offcentre  the same, the lens restricted to where ``fov_from_focal`` can be told from the truth in float32: fx, fy
             log-uniform in [0.25, 4], |cx - 0.5| and |cy - 0.5| in [0.05, 0.15], skew as in general.

Gate.  Per output and render, c_needed = max over the elements of |got - x64| / bound with the bounds of
tests/camera_oracle.py (derived from rounding; a bound of 0 means bitwise) must not exceed 1.  POWER CONDITION: for every
mutant of the oracle and every output it reaches, on EVERY render of the families it reaches, the mutant is at least 4
bounds away from the oracle in at least one element.  UNREACHED lists what a mutant cannot move, FAMILY_UNREACHED where
a mutant that can move an output does not do so by 4 float32 bounds on every render:
  * the four mutants about 1/near change nothing when scale_invariant is off (the scale is 1);
  * fov_from_focal is exact under ``centred``, and under ``general`` it is off by about (cx - 0.5)^2 / fx^2 relative
    (expand atan(a) + atan(b), a + b = 1 / fx): below 4 u wherever fx > |cx - 0.5| / (2 sqrt(u)) -- fx > 100 at an
    offset of 0.05, every fx as the principal point nears the centre -- so it is asked for on ``offcentre`` only,
    where that figure is at least 0.05^2 / 4^2 = 1.6e-4.
"""
from __future__ import annotations

import math

import torch

from tests import camera_oracle as co

POWER = 4.0
FAMILIES = ("general", "centred", "offcentre")
FAMILY_SIZE = 300
SIZES = (1, 63, 64, 65, 300)              # one lane per render in blocks of 64: a lane, a block less one, a block, one more
NBLK = (1, 3, 63, 64, 65, 255, 256, 257, 1954)      # a lane, a wave, a block, one past each; 500,000 Gaussians
PARTIAL_R = (1, 5, 65)
GRAD_OUT = "dL_dextrinsics"

# outputs a mutant cannot move at all
UNREACHED = {
    "no_translation_rescale": ("projmatrix", "tanfov", "view_scale"),
    "far_not_rescaled": ("viewmatrix", "tanfov", "view_scale", "viewmatrix64"),
    "view_not_transposed": ("projmatrix", "tanfov", "view_scale"),
    "view64_without_scale": ("viewmatrix", "projmatrix", "tanfov", "view_scale"),
    "fov_from_focal": ("viewmatrix", "view_scale", "viewmatrix64"),
    "grad_not_transposed": (), "grad_no_rescale": (), "grad_sign": (), "partials_last_column": (),
}
NEEDS_SCALE = ("no_translation_rescale", "far_not_rescaled", "view64_without_scale", "grad_no_rescale")
FAMILY_UNREACHED = {"fov_from_focal": ("centred", "general")}


def reached(mutant: str, family: str, scale_invariant: bool) -> bool:
    return not ((mutant in NEEDS_SCALE and not scale_invariant) or family in FAMILY_UNREACHED.get(mutant, ()))


_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _log_uniform(gen, n, lo, hi):
    return torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _rotations(gen, n, family_index):
    q = torch.randn(n, 4, generator=gen, dtype=torch.float64)
    axis = torch.randn(2, 3, generator=gen, dtype=torch.float64)
    axis = axis / axis.norm(dim=-1, keepdim=True)
    special = [torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64)]
    for a, angle in zip(axis, (math.pi - 1e-3, math.pi)):
        special.append(torch.cat((torch.tensor([math.cos(angle / 2)], dtype=torch.float64), math.sin(angle / 2) * a)))
    for k, s in enumerate(special):
        q[(k + family_index) % 3] = s
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = q.unbind(-1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)), dim=-1).reshape(n, 3, 3)


def family(name: str) -> dict:
    """{extrinsics [300,4,4], intrinsics [300,3,3], near [300], far [300]}, float32, on the CPU."""
    def make():
        n, idx = FAMILY_SIZE, FAMILIES.index(name)
        gen = torch.Generator().manual_seed(20240 + idx)
        ext = torch.zeros(n, 4, 4, dtype=torch.float64)
        ext[:, :3, :3] = _rotations(gen, n, idx)
        t = torch.randn(n, 3, generator=gen, dtype=torch.float64)
        ext[:, :3, 3] = t / t.norm(dim=-1, keepdim=True) * _log_uniform(gen, n, 0.01, 5.0)[:, None]
        ext[:, 3, 3] = 1
        low, high = _log_uniform(gen, n, 0.05, 0.5), _log_uniform(gen, n, 2.0, 10.0)
        near = torch.where(torch.arange(n) % 2 == 0, low, high).float()
        far = (near.double() * _log_uniform(gen, n, 1.01, 1e4)).float()
        f_hi = 4.0 if name == "offcentre" else 200.0
        fx, fy = _log_uniform(gen, n, 0.25, f_hi), _log_uniform(gen, n, 0.25, f_hi)
        off = (torch.rand(n, 2, generator=gen, dtype=torch.float64) * 2 - 1) * 0.15
        if name == "offcentre":
            sign = torch.where(off < 0, -1.0, 1.0)
            off = sign * (0.05 + 0.1 * torch.rand(n, 2, generator=gen, dtype=torch.float64))
        skew = 0.02 * fx * torch.randn(n, generator=gen, dtype=torch.float64)
        if name == "centred":
            off, skew = torch.zeros_like(off), torch.zeros_like(skew)
        K = torch.zeros(n, 3, 3, dtype=torch.float64)
        K[:, 0, 0], K[:, 1, 1], K[:, 0, 1], K[:, 2, 2] = fx, fy, skew, 1
        K[:, 0, 2], K[:, 1, 2] = 0.5 + off[:, 0], 0.5 + off[:, 1]
        return {"extrinsics": ext.float(), "intrinsics": K.float(), "near": near, "far": far}
    return _once(("family", name), make)


def cameras(name: str, R: int) -> dict:
    """The first R renders of a family; R above 300 repeats the family (render r is camera r % 300)."""
    fam = family(name)
    if R <= FAMILY_SIZE:
        return {k: v[:R] for k, v in fam.items()}
    reps = (R + FAMILY_SIZE - 1) // FAMILY_SIZE
    return {k: v.repeat(reps, *([1] * (v.dim() - 1)))[:R] for k, v in fam.items()}


def forward_oracle(cams: dict, scale_invariant: bool, mut=co.NONE) -> dict:
    return co.forward(cams["extrinsics"], cams["intrinsics"], cams["near"], cams["far"], scale_invariant, mut)


def forward_reference(name: str, scale_invariant: bool):
    """(cameras, float64 oracle, bounds, {mutant: {output: per-render distance in bounds}}) of a whole family."""
    def make():
        cams = family(name)
        x64 = forward_oracle(cams, scale_invariant)
        bounds = co.forward_bounds(x64, cams["near"], cams["far"])
        dists = {}
        for m in co.FORWARD_MUTANTS:
            if reached(m, name, scale_invariant):
                mu = forward_oracle(cams, scale_invariant, frozenset([m]))
                dists[m] = {k: co.needed(mu[k], x64[k], bounds[k]) for k in co.FORWARD_NAMES if k not in UNREACHED[m]}
        return cams, x64, bounds, dists
    return _once(("forward_ref", name, scale_invariant), make)


def head(t: dict, R: int) -> dict:
    return {k: v[:R] for k, v in t.items()}


def upstream(name: str) -> torch.Tensor:
    """A random dL/dviewmatrix [300,4,4], float32, per family."""
    def make():
        gen = torch.Generator().manual_seed(777 + FAMILIES.index(name))
        return torch.randn(FAMILY_SIZE, 4, 4, generator=gen)
    return _once(("upstream", name), make)


def grad_reference(name: str, scale_invariant: bool):
    """(cameras, G, float64 gradient, bound, {mutant: per-render distance in bounds}) of a whole family with upstream()."""
    def make():
        cams, x64, _, _ = forward_reference(name, scale_invariant)
        G = upstream(name)
        want, bound = grad_case(cams, x64["viewmatrix"], scale_invariant, G)
        dists = {}
        for m in co.GRAD_MUTANTS:
            if reached(m, name, scale_invariant):
                mu = co.pose_grad(cams["extrinsics"], cams["near"], scale_invariant, G, frozenset([m]))
                dists[m] = {GRAD_OUT: co.needed(mu, want, bound)}
        return cams, G, want, bound, dists
    return _once(("grad_ref", name, scale_invariant), make)


def grad_case(cams: dict, view64, scale_invariant: bool, G):
    """(float64 gradient, bound) for an upstream gradient G [R,4,4]."""
    want = co.pose_grad(cams["extrinsics"], cams["near"], scale_invariant, G)
    return want, co.grad_bound(view64, co.f64(cams["near"]), scale_invariant, G)


def one_hot_sweep(name: str, renders=(0, 1, 2)):
    """(cameras [16 * len(renders)], G): each of a few renders sixteen times, G one-hot at entry k of the 4x4."""
    fam = family(name)
    idx = torch.tensor([r for r in renders for _ in range(16)])
    G = torch.eye(16).reshape(16, 4, 4).repeat(len(renders), 1, 1)
    return {k: v[idx] for k, v in fam.items()}, G


def exact_partials(R: int, nblk: int, pad: int = 0) -> torch.Tensor:
    """[R * nblk * 12 + pad] float32: integer multiples of 2^-8 in [-4, 4] -- every sum of up to 4096 of them is exact in
    float32 in any order (|sum| <= 2^14 = 2^22 units of 2^-8) -- followed by ``pad`` NaNs."""
    assert nblk <= 4096
    gen = torch.Generator().manual_seed(31 * nblk + R)
    p = torch.randint(-1024, 1025, (R * nblk * 12,), generator=gen).float() / 256.0
    return torch.cat((p, torch.full((pad,), float("nan"))))


def random_partials(R: int, nblk: int) -> torch.Tensor:
    gen = torch.Generator().manual_seed(57 * nblk + R)
    return torch.randn(R * nblk * 12, generator=gen)


def one_hot_partials(R: int, nblk: int) -> torch.Tensor:
    """[12 * R, nblk, 12]: copy s of render r (row 12 r + s) holds a single 1, in slot s of block (5 s + r) % nblk."""
    p = torch.zeros(12 * R, nblk, 12)
    for r in range(R):
        for s in range(12):
            p[12 * r + s, (5 * s + r) % nblk, s] = 1.0
    return p


def partial_mutant_distance(cams, view64, scale_invariant, sums, want, bound):
    mu = co.pose_grad(cams["extrinsics"], cams["near"], scale_invariant,
                      co.map_partials(sums, frozenset(["partials_last_column"])))
    return {"partials_last_column": {GRAD_OUT: co.needed(mu, want, bound)}}


# ---- the gate --------------------------------------------------------------------------------------------------------
def power_failures(label: str, dists: dict, R: int = FAMILY_SIZE) -> list:
    """The offenders of the power condition over the first R renders as text (empty: the gate can be trusted)."""
    bad, tight = [], (float("inf"), "")
    for m, per_out in dists.items():
        for k, d in per_out.items():
            d = d[:R]
            r = int(d.argmin())
            tight = min(tight, (float(d[r]), f"{m}, {k}, render {r}"))
            if float(d[r]) < POWER:
                bad.append(f"{label}: mutant '{m}' moves {k} of render {r} by {float(d[r]):.3g} bounds < {POWER:g}")
    if dists:
        print(f"{label} power: tightest mutant distance = {tight[0]:.3g} bounds ({tight[1]})")
    return bad


def gate(label: str, got: dict, x64: dict, bounds: dict, dists: dict, eager: dict | None = None) -> dict:
    """Prints c_needed of every output (and eager float32's, for information), asserts the power condition, then that
    every output is finite and within its bound on every render.  Returns {output: c_needed}."""
    assert sorted(got) == sorted(x64), (sorted(got), sorted(x64))
    R = next(iter(x64.values())).shape[0]
    need = {k: co.needed(got[k], x64[k], bounds[k]) for k in x64}
    for k in x64:
        info = f" eager float32 {float(co.needed(eager[k], x64[k], bounds[k]).max()):.3g}" if eager and k in eager else ""
        print(f"{label} {k}: c_needed {float(need[k].max()):.3f}{info}")
    bad = power_failures(label, dists, R)
    assert not bad, "\n".join(bad)
    for k, t in got.items():
        assert tuple(t.shape) == tuple(x64[k].shape), (label, k, tuple(t.shape))
        assert bool(torch.isfinite(t).all()), (label, k)
        c = float(need[k].max())
        assert c <= 1.0, (label, k, "render", int(need[k].argmax()), "c_needed", c)
    return {k: float(v.max()) for k, v in need.items()}
