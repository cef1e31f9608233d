"""Cases, operands and the gate of the encoder front's tests (tests/test_front.py on the host, tests/test_gpu_front.py on
the device).

A case is (gh, gw, B, P, C_in, C, form): a gh x gw patch grid, B images, patch size P, C_in input channels of which the
first three are normalised with the ImageNet mean / std, embedding width C, and the extra rows:
  "none"   no extra rows
  "croco"  after = a per-image token + a broadcast token (the CroCo encoder: intrinsics and pose token)
  "dino"   before = cls (broadcast) + a per-image intrinsics token + 4 registers (broadcast), pos_table, pos_first

Gate (rule (a) of tests/test_gpu_lpips.py: K-long sums in another order than eager's): per gated tensor
err = max|x - x64| / max|x64| <= min(8 x yardstick + 2.4e-7, 1e-5), the yardstick being float32 eager torch (the
reference's own lines, tests/front_oracle.py::eager_embed) on the same operands.  Power condition: every mutant moves
every tensor it reaches by at least 4 bounds.
"""
import torch

from tests import front_oracle as fo

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
POWER = 4.0
CAP = 1e-5
FORMS = ("none", "croco", "dino")

# grids x images of the issue: one row, a partial row tile, tiles that straddle two images, whole tiles, H != W; widths
# 64 / 192 / 320 / 1024 and the three forms cycled over them
COVER = (
    (1, 1, 1, 16, 3, 64, "none"), (3, 5, 1, 16, 3, 192, "croco"), (6, 11, 3, 16, 3, 320, "dino"),
    (16, 16, 2, 16, 3, 64, "croco"), (9, 15, 3, 16, 3, 192, "none"), (16, 16, 2, 16, 3, 320, "dino"),
    (1, 1, 1, 14, 5, 192, "dino"), (3, 5, 1, 14, 5, 320, "none"), (6, 11, 3, 14, 5, 64, "croco"),
    (6, 11, 3, 14, 5, 320, "dino"), (3, 5, 1, 16, 3, 1024, "dino"), (1, 1, 1, 16, 3, 64, "croco"),
)

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def case_id(case) -> str:
    gh, gw, b, p, c_in, c, form = case
    return f"{gh}x{gw}x{b}-P{p}-in{c_in}-C{c}-{form}"


def bound(yardstick: float) -> float:
    return min(8.0 * yardstick + 2.4e-7, CAP)


def operands(case) -> dict:
    """float32 host tensors of a case, made once."""
    def make():
        gh, gw, b, p, c_in, c, form = case
        gen = torch.Generator().manual_seed(sum(map(ord, case_id(case))))
        n, k = gh * gw, c_in * p * p
        d = {"image": torch.rand(b, c_in, gh * p, gw * p, generator=gen),
             "weight": torch.randn(c, c_in, p, p, generator=gen) * k ** -0.5, "bias": torch.randn(c, generator=gen),
             "before": [], "after": [], "pos_table": None, "pos_first": None}
        if form == "croco":
            d["after"] = [torch.randn(b, 1, c, generator=gen), torch.randn(1, 1, c, generator=gen)]
        if form == "dino":
            d["before"] = [torch.randn(1, 1, c, generator=gen), torch.randn(b, 1, c, generator=gen),
                           torch.randn(1, 4, c, generator=gen)]
            d["pos_table"], d["pos_first"] = torch.randn(n, c, generator=gen), torch.randn(c, generator=gen)
        rows = sum(t.shape[1] for t in d["before"] + d["after"]) + n
        d["up"] = torch.randn(b, rows, c, generator=gen)
        return d
    return _once(("ops", case), make)


def leaves_of(d, dtype, device) -> dict:
    """The differentiable operands as leaves: {name: tensor}."""
    to = lambda t: t.to(device=device, dtype=dtype).requires_grad_(True)       # noqa: E731
    out = {"weight": to(d["weight"]), "bias": to(d["bias"])}
    if d["pos_table"] is not None:
        out["pos_table"], out["pos_first"] = to(d["pos_table"]), to(d["pos_first"])
    for name in ("before", "after"):
        for i, t in enumerate(d[name]):
            out[f"{name}{i}"] = to(t)
    return out


def call(fn, case, d, leaves, image, **kw):
    """``fn`` (fo.embed, fo.eager_embed or the product in the same signature) on a case's operands."""
    before = [leaves[f"before{i}"] for i in range(len(d["before"]))]
    after = [leaves[f"after{i}"] for i in range(len(d["after"]))]
    return fn(image, leaves["weight"], leaves["bias"], case[3], mean=MEAN, std=STD, pos_table=leaves.get("pos_table"),
              pos_first=leaves.get("pos_first"), before=before, after=after, **kw)


def with_grads(out, up, leaves) -> dict:
    grads = torch.autograd.grad((out * up).sum(), list(leaves.values()), allow_unused=True)
    res = {"out": out.detach()}
    for (k, t), g in zip(leaves.items(), grads):
        res["d_" + k] = torch.zeros_like(t) if g is None else g.detach()
    return res


def run(fn, case, d, dtype=torch.float64, device="cpu", **kw) -> dict:
    leaves = leaves_of(d, dtype, device)
    out = call(fn, case, d, leaves, d["image"].to(device=device, dtype=dtype), **kw)
    return with_grads(out, d["up"].to(device=device, dtype=dtype), leaves)


def oracle(case, d, dtype=torch.float64, device="cpu", mut=fo.NONE) -> dict:
    return run(fo.embed, case, d, dtype, device, mut=mut)


def eager(case, d, device="cpu") -> dict:
    return run(fo.eager_embed, case, d, torch.float32, device)


def mutants_of(case) -> dict:
    """{mutant: the tensors it reaches} for a case."""
    gh, gw, b, p, c_in, c, form = case
    reach = {"swap_patch": ("out", "d_weight"), "pixel_major": ("out", "d_weight"), "no_norm": ("out", "d_weight"),
             "times_std": ("out", "d_weight"), "no_bias": ("out",)}
    if form == "dino":
        if gh * gw > 1:
            reach["pos_shift"] = ("out", "d_pos_table")
        reach["pos_all"] = ("out", "d_pos_table")
        if b > 1:
            reach["mean_grad"] = ("d_before0", "d_before2")
    if form == "croco":
        reach["after_front"] = ("out", "d_weight", "d_bias")
        if b > 1:
            reach["mean_grad"] = ("d_after1",)
    return reach


def reference(case, muts=None):
    """(operands, the float64 oracle's results, {mutant: {tensor: distance from them}}), made once per case."""
    def make():
        d = operands(case)
        x64 = oracle(case, d)
        dists = {}
        for name, reach in mutants_of(case).items():
            if muts is not None and name not in muts:
                continue
            m = oracle(case, d, mut=frozenset([name]))
            dists[name] = {k: fo.rel_err(m[k], x64[k]) for k in reach}
        return d, x64, dists
    return _once(("ref", case, muts), make)


def errors(res: dict, x64: dict) -> dict:
    return {k: fo.rel_err(res[k], x64[k]) for k in x64}


def power_failures(label: str, dists: dict, e_eager: dict) -> list:
    """The offenders of the power condition as text (empty: the gate can be trusted); prints the tightest ratio."""
    bad, tight = [], (float("inf"), "")
    for name, d in dists.items():
        for k, x in d.items():
            b = bound(e_eager[k])
            tight = min(tight, (x / b, f"{name}, {k}"))
            if x < POWER * b:
                bad.append(f"{label}: mutant '{name}' moves {k} by {x:.3e} < {POWER:g} x bound {b:.3e}")
    if dists:
        print(f"{label} power: tightest mutant / bound = {tight[0]:.1f} ({tight[1]})")
    return bad


def gate(label: str, got: dict, eager_res: dict, x64: dict, dists: dict) -> None:
    """Prints every figure, asserts the power condition on the eager figures, then the gate."""
    e_got, e_eager = errors(got, x64), errors(eager_res, x64)
    for k in x64:
        print(f"{label} {k}: product {e_got[k]:.3e} eager {e_eager[k]:.3e} bound {bound(e_eager[k]):.3e}")
    bad = power_failures(label, dists, e_eager)
    assert not bad, "\n".join(bad)
    for k, t in got.items():
        assert t.shape == x64[k].shape and torch.isfinite(t).all(), (label, k)
    for k in x64:
        assert e_got[k] <= bound(e_eager[k]), (label, k, e_got[k], e_eager[k])


# ---- assemble_tokens -------------------------------------------------------------------------------------------------
def assemble_operands(b=2, v=3, n=7, c=64) -> dict:
    def make():
        gen = torch.Generator().manual_seed(186)
        return {"x": torch.randn(b, v, n, c, generator=gen), "intr": torch.randn(b, v, 1, c, generator=gen),
                "pose": torch.randn(1, 1, c, generator=gen), "up": torch.randn(b, v, n + 2, c, generator=gen)}
    return _once(("assemble", b, v, n, c), make)


# ---- the goldens -----------------------------------------------------------------------------------------------------
def goldens(golden_dir) -> dict:
    return _once("goldens", lambda: torch.load(golden_dir / "front_goldens.pt"))
