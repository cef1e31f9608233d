"""Float64 oracle of the guarded AdamW step, in this project's own words: the walk of the reference's ``optimizer_step``
hook over the gradients, ``clip_grad_norm_`` and the AdamW update with a step count per parameter -- plus the parameter
set, the scenarios and the gate arithmetic that tests/test_optim.py, tests/test_gpu_optim.py and
tests/golden/make_optim_goldens.py share.

The walk: tensors in guard order; no gradient -> passed over; a NaN ends the walk (before that tensor's maximum is looked
at); otherwise the running maximum takes the tensor's max |g| and a max |g| STRICTLY above the threshold ends the walk.
A walk that ended skips the step.  Otherwise every gradient is scaled by min(1, max_norm / (total_norm + 1e-6)) and every
parameter that has a gradient takes one AdamW step with its own step count:

    p *= 1 - lr wd;  m += (1 - b1)(g - m);  v = b2 v + (1 - b2) g^2
    p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
"""
from __future__ import annotations

import math

import torch

# ---- the parameter set of the goldens ----------------------------------------------------------------------------------
SHAPES = ((1,), (3,), (5, 7), (1023,), (1024,), (1025,), (4097,), (64, 33))
NAMES = ("encoder.backbone.cls_token", "encoder.backbone.norm.bias", "encoder.gaussian_param_head.proj.weight",
         "encoder.backbone.blocks.0.bias", "encoder.pose_head.fc.bias", "encoder.backbone.blocks.1.bias",
         "encoder.backbone.pos_embed", "encoder.gaussian_param_head.out.weight")
NEW_KEYS = ("gaussian_param_head", "intrinsic_encoder", "pose_head", "camera_head")     # the reference's "new" group
LR, BACKBONE_LR_MULTIPLIER = 2e-3, 0.1
LR_FACTORS = (1.0, 0.7, 0.4)                # what a scheduler does to both groups' lr over the three steps
STEPS = 3
BETAS, EPS, WEIGHT_DECAY, MAX_NORM = (0.9, 0.95), 1e-8, 0.05, 0.5
ADAM = dict(lr=5e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)                    # test_step_align's torch.optim.Adam

F32 = torch.float32
NEXT_ABOVE_5 = float(torch.nextafter(torch.tensor(5.0, dtype=F32), torch.tensor(math.inf, dtype=F32)))
NAN, INF = math.nan, math.inf

# name: gradient scale, threshold, edits (step, tensor, flat index, value) applied to the scaled base gradients, and the
# (step, tensor) pairs without gradient.  Tensors are numbered in guard order = NAMES order.
SCENARIOS = {
    "clean_small_norm": dict(scale=0.002, threshold=5, edits=(), absent=()),
    "clean_clipped": dict(scale=0.05, threshold=5, edits=(), absent=()),
    "at_threshold": dict(scale=0.002, threshold=5, edits=((1, 5, 1024, -5.0),), absent=()),
    "above_threshold": dict(scale=0.002, threshold=5, edits=((1, 5, 1024, NEXT_ABOVE_5),), absent=()),
    "nan_fifth": dict(scale=0.002, threshold=5, edits=((1, 4, 1023, NAN),), absent=()),
    "large_second_nan_sixth": dict(scale=0.002, threshold=5, edits=((1, 1, 2, 7.5), (1, 5, 0, NAN)), absent=()),
    "nan_and_large_same": dict(scale=0.002, threshold=5, edits=((1, 6, 4096, NAN), (1, 6, 17, 100.0)), absent=()),
    "infinities": dict(scale=0.002, threshold=5, edits=((0, 3, 5, INF), (2, 7, 2111, -INF)), absent=()),
    "absent_at_step_2": dict(scale=0.05, threshold=5, edits=(), absent=((1, 3), (1, 7))),
    "threshold_20": dict(scale=0.002, threshold=20, edits=((1, 2, 34, 10.0), (2, 6, 4000, -20.5)), absent=()),
    "adam_step_align": dict(scale=0.05, threshold=None, edits=(), absent=(), adam=True),
}


def groups_of_names(names=NAMES):
    """(new, pretrained): tensor numbers per group, as configure_optimizers sorts them."""
    new = [i for i, n in enumerate(names) if any(k in n for k in NEW_KEYS)]
    return new, [i for i in range(len(names)) if i not in new]


def base_inputs(seed: int = 20):
    """Seeded float32 parameters and three steps of unit-variance base gradients (stored in the goldens)."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=gen, dtype=F32) * 0.3 for s in SHAPES]
    grads = [[torch.randn(s, generator=gen, dtype=F32) for s in SHAPES] for _ in range(STEPS)]
    return {"params": params, "grads": grads}


def scenario_grads(base, name: str):
    """Per step the list of float32 gradients (None = absent) of a scenario."""
    sc = SCENARIOS[name]
    out = []
    for s in range(STEPS):
        gs = [(g * sc["scale"]).to(F32) for g in base["grads"][s]]
        for (es, t, i, val) in sc["edits"]:
            if es == s:
                gs[t].view(-1)[i] = val
        for (es, t) in sc["absent"]:
            if es == s:
                gs[t] = None
        out.append(gs)
    return out


def scenario_groups(name: str):
    """[{lr, betas, eps, weight_decay, tensors}] in the optimizer's group order, and (threshold, max_norm)."""
    sc = SCENARIOS[name]
    if sc.get("adam"):
        return [dict(ADAM, tensors=list(range(len(SHAPES))))], None, None
    new, pre = groups_of_names()
    common = dict(betas=BETAS, eps=EPS, weight_decay=WEIGHT_DECAY)
    return ([dict(common, lr=LR, tensors=new), dict(common, lr=LR * BACKBONE_LR_MULTIPLIER, tensors=pre)],
            sc["threshold"], MAX_NORM)


def sample_index(numel: int, limit: int = 128) -> torch.Tensor:
    """The elements of a tensor the goldens keep: all of a small one, `limit` evenly spaced ones (first and last
    included) otherwise -- a committed file stays small, and every element follows the same formula."""
    if numel <= limit:
        return torch.arange(numel)
    return torch.unique(torch.linspace(0, numel - 1, limit).round().long())


# ---- the oracle ------------------------------------------------------------------------------------------------------
def guard_walk(grads, order, threshold):
    """The hook's loop.  grads: per tensor a tensor or None; order: tensor numbers in walk order."""
    rep = dict(skipped=False, nan_detected=False, large_detected=False, offender=-1, max_gradient=0.0)
    if threshold is None:
        return rep
    for pos, t in enumerate(order):
        g = grads[t]
        if g is None:
            continue
        if bool(torch.isnan(g).any()):
            rep.update(skipped=True, nan_detected=True, offender=pos)
            break
        mx = float(g.abs().max())
        rep["max_gradient"] = max(rep["max_gradient"], mx)
        if mx > threshold:
            rep.update(skipped=True, large_detected=True, offender=pos)
            break
    return rep


def total_norm(grads) -> float:
    return float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads if g is not None)))


def clip_coefficient(norm: float, max_norm) -> float:
    if max_norm is None:
        return 1.0
    coef = max_norm / (norm + 1e-6)
    return 1.0 if coef > 1.0 else coef


class Oracle:
    """The guarded step in float64.  ``mutant``: None, or one deliberate mistake -- "beta2" (0.999 for the configured
    value), "noclip" (the clip left out), "coupled" (weight decay added to the gradient as Adam's L2 term) -- that a gate
    worth trusting must catch."""

    def __init__(self, params, groups, order=None, threshold=5, max_norm=0.5, mutant=None, dtype=torch.float64):
        self.p = [p.detach().to(dtype).clone() for p in params]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.step_count = [0] * len(self.p)
        self.groups = [dict(g) for g in groups]
        self.group_of = {t: gi for gi, g in enumerate(groups) for t in g["tensors"]}
        self.order = list(range(len(self.p))) if order is None else list(order)
        self.threshold, self.max_norm, self.mutant, self.dtype = threshold, max_norm, mutant, dtype

    def step(self, grads, lrs=None):
        """grads: per tensor a tensor or None.  lrs: this step's lr per group (default: the groups' own)."""
        rep = guard_walk(grads, self.order, self.threshold)
        rep["total_norm"] = total_norm(grads)
        rep["clip_coef"] = clip_coefficient(rep["total_norm"], self.max_norm)
        if rep["skipped"]:
            return rep
        coef = 1.0 if self.mutant == "noclip" else rep["clip_coef"]
        for t, g in enumerate(grads):
            if g is None:
                continue
            grp = self.groups[self.group_of[t]]
            lr = grp["lr"] if lrs is None else lrs[self.group_of[t]]
            b1, b2 = grp["betas"]
            if self.mutant == "beta2":
                b2 = 0.999 if b2 != 0.999 else 0.95
            wd, eps = grp["weight_decay"], grp["eps"]
            g = g.to(self.dtype) * coef
            self.step_count[t] += 1
            n = self.step_count[t]
            if self.mutant == "coupled":
                g = g + wd * self.p[t]
            else:
                self.p[t] = self.p[t] * (1.0 - lr * wd)
            self.m[t] = self.m[t] + (1.0 - b1) * (g - self.m[t])
            self.v[t] = b2 * self.v[t] + (1.0 - b2) * g * g
            step_size = lr / (1.0 - b1 ** n)
            denom = self.v[t].sqrt() / math.sqrt(1.0 - b2 ** n) + eps
            self.p[t] = self.p[t] - step_size * self.m[t] / denom
        return rep


def scenario_lrs(name: str):
    """Per step the lr of every group."""
    groups = scenario_groups(name)[0]
    return [[g["lr"] * f for g in groups] for f in LR_FACTORS]


def oracle_run(params, groups, grads_per_step, lrs_per_step, threshold, max_norm, mutant=None, dtype=torch.float64):
    """The oracle over consecutive steps: (oracle, [report per step])."""
    o = Oracle(params, groups, threshold=threshold, max_norm=max_norm, mutant=mutant, dtype=dtype)
    return o, [o.step(gs, lrs) for gs, lrs in zip(grads_per_step, lrs_per_step)]


def run_scenario(name: str, base, mutant=None, dtype=torch.float64):
    groups, threshold, max_norm = scenario_groups(name)
    return oracle_run(base["params"], groups, scenario_grads(base, name), scenario_lrs(name), threshold, max_norm,
                      mutant, dtype)


def torch_run(params, groups, grads_per_step, lrs_per_step, threshold, max_norm, adam=False, dtype=F32):
    """Live ``torch.optim.AdamW`` (``adam``: ``torch.optim.Adam``) + ``clip_grad_norm_`` on the CPU over consecutive
    steps, skipping where the walk says so: ([p], [m], [v], [step]) per tensor number."""
    live = [torch.nn.Parameter(p.detach().to(dtype).clone()) for p in params]
    dicts = [dict(params=[live[t] for t in g["tensors"]], lr=g["lr"], betas=g["betas"], eps=g["eps"],
                  weight_decay=g["weight_decay"]) for g in groups]
    opt = (torch.optim.Adam if adam else torch.optim.AdamW)(dicts)
    for gs, lrs in zip(grads_per_step, lrs_per_step):
        for gi, lr in enumerate(lrs):
            opt.param_groups[gi]["lr"] = lr
        for p, g in zip(live, gs):
            p.grad = None if g is None else g.to(dtype).clone()
        if not guard_walk(gs, range(len(live)), threshold)["skipped"]:
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_(live, max_norm)
            opt.step()
    state = [opt.state.get(p, {}) for p in live]
    zeros = [torch.zeros_like(p) for p in live]
    return ([p.detach() for p in live], [s.get("exp_avg", z) for s, z in zip(state, zeros)],
            [s.get("exp_avg_sq", z) for s, z in zip(state, zeros)], [int(s.get("step", 0)) for s in state])


def run_torch(name: str, base, dtype=F32):
    groups, threshold, max_norm = scenario_groups(name)
    return torch_run(base["params"], groups, scenario_grads(base, name), scenario_lrs(name), threshold, max_norm,
                     adam=bool(SCENARIOS[name].get("adam")), dtype=dtype)


# ---- the gate ----------------------------------------------------------------------------------------------------------
def ulp32(x: float) -> float:
    """One unit in the last place of float32 at magnitude x."""
    x = abs(float(x))
    if x == 0.0 or not math.isfinite(x):
        return 2.0 ** -149
    return max(2.0 ** (math.floor(math.log2(x)) - 23), 2.0 ** -149)


def tensor_error(got: torch.Tensor, want64: torch.Tensor) -> float:
    """max |got - want| over a tensor; inf where one is non-finite and the other differs."""
    got, want64 = got.double().cpu(), want64.double().cpu()
    same = (got == want64) | (torch.isnan(got) & torch.isnan(want64))
    diff = torch.where(same, torch.zeros_like(want64), (got - want64).abs())
    diff = torch.where(torch.isnan(diff), torch.full_like(diff, math.inf), diff)
    return float(diff.max())


def gate(torch_error: float, want64: torch.Tensor) -> float:
    """max(2 x the error of float32 torch on the same inputs, 1 ulp of float32 at the tensor's largest magnitude)."""
    finite = want64[torch.isfinite(want64)]
    top = float(finite.abs().max()) if finite.numel() else 0.0
    return max(2.0 * torch_error, ulp32(top))
