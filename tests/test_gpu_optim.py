"""The guarded AdamW step on the device against the float64 oracle (tests/optim_oracle.py) and the reference's goldens.

Verdict fields, the offender and max_gradient are compared bitwise; total_norm and clip_coef within 2e-6 relative (a
4096-wide float32 tree and a float64 tail: (log2 4096 + 2) 2^-24 ~ 8e-7); parameters and both moments per tensor within
max(2 x the error of float32 torch.optim.AdamW on the same inputs against the same oracle, 1 ulp of float32 at the
tensor's largest magnitude) -- the factor 2 is for a different but equally valid order of float32 operations.  Run with
-s for the figures (profiles/optim_gate_figures.txt holds one run's)."""
import math

import pytest
import torch

from tests import optim_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
REPORT_FIELDS = ("skipped", "nan_detected", "large_detected", "offender", "max_gradient", "total_norm", "clip_coef")


def _read(report):
    return {f: getattr(report, f).item() for f in REPORT_FIELDS}


def _bits(x: float) -> bytes:
    return torch.tensor(x, dtype=torch.float32).numpy().tobytes()


def device_run(params, groups, grads_per_step, lrs_per_step, threshold, max_norm, names=None, offset=0):
    """The product over consecutive steps.  ``offset`` > 0: every parameter and gradient is ``buffer[offset:]`` -- 4-byte
    but not 16-byte aligned.  Gradients are new tensors at every step.  Returns per tensor number p, m, v, step counts,
    and the report of every step."""
    import spfsplatv2_amd as spf

    def place(t):
        if not offset:
            return t.to(DEV)
        buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
        buf[offset:].copy_(t.reshape(-1))
        out = buf[offset:].view(t.shape)
        assert out.data_ptr() % 16 == 4 * offset % 16
        return out

    live = [torch.nn.Parameter(place(p.detach().to(torch.float32))) for p in params]
    dicts = [dict(params=[live[t] for t in g["tensors"]], lr=g["lr"], betas=g["betas"], eps=g["eps"],
                  weight_decay=g["weight_decay"]) for g in groups]
    named = None if names is None else list(zip(names, live))
    opt = spf.GuardedAdamW(dicts, max_grad_value=threshold, max_norm=max_norm, named_parameters=named)
    reports, keep = [], []
    for gs, lrs in zip(grads_per_step, lrs_per_step):
        for gi, lr in enumerate(lrs):
            opt.param_groups[gi]["lr"] = lr
        for p, g in zip(live, gs):
            p.grad = None if g is None else place(g)
        keep.append([p.grad for p in live])                      # (kept alive: the next step's land elsewhere)
        opt.step()
        reports.append(_read(opt.last_step))
        opt.zero_grad()
    flat = [t for g in groups for t in g["tensors"]]
    state = opt.state_dict()["state"]
    m, v, steps = [None] * len(live), [None] * len(live), [0] * len(live)
    for i, t in enumerate(flat):
        st = state.get(i)
        m[t] = st["exp_avg"].cpu() if st else torch.zeros(params[t].shape)
        v[t] = st["exp_avg_sq"].cpu() if st else torch.zeros(params[t].shape)
        steps[t] = int(st["step"]) if st else 0
    return [p.detach().cpu() for p in live], m, v, steps, reports, opt


def _scenario_device(name, base, offset=0):
    groups, threshold, max_norm = O.scenario_groups(name)
    return device_run(base["params"], groups, O.scenario_grads(base, name), O.scenario_lrs(name), threshold, max_norm,
                      names=O.NAMES, offset=offset)


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return torch.load(golden_dir / "optim_goldens.pt", weights_only=False)


@pytest.fixture(scope="module")
def runs(goldens, hip_lib):
    """Every scenario once: the product on the device, the float64 oracle and float32 torch on the CPU."""
    base = goldens["base"]
    out = {}
    for name in O.SCENARIOS:
        oracle, oracle_reports = O.run_scenario(name, base)
        out[name] = dict(device=_scenario_device(name, base)[:5], oracle=oracle, oracle_reports=oracle_reports,
                         torch32=O.run_torch(name, base))
    return out


def _close(got: float, want: float, rel: float) -> bool:
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return abs(got - want) <= rel * abs(want)


@pytest.mark.parametrize("name", list(O.SCENARIOS))
def test_verdicts(runs, goldens, name):
    """Per step: the verdict fields, the offender and max_gradient bitwise (against the oracle's walk AND what the
    reference logged in float32), total_norm and clip_coef within 2e-6 of the float64 oracle."""
    reports = runs[name]["device"][4]
    logs = goldens["scenarios"][name]["float32"]["logs"]
    for s, (got, want, log) in enumerate(zip(reports, runs[name]["oracle_reports"], logs)):
        print(f"{name} step {s}: {got}")
        for f in ("skipped", "nan_detected", "large_detected"):
            assert got[f] == int(want[f]) == int(log[f]), (name, s, f)
        assert got["offender"] == want["offender"], (name, s)
        if log["offender"]:
            assert O.NAMES[got["offender"]] == log["offender"]
        assert _bits(got["max_gradient"]) == _bits(want["max_gradient"]) == _bits(log["max_gradient"]), (name, s)
        if O.SCENARIOS[name].get("adam"):                        # no guard, no clip: pass A is not run
            assert got["total_norm"] == 0.0 and got["clip_coef"] == 1.0
            continue
        assert _close(got["total_norm"], want["total_norm"], 2e-6), (name, s, got["total_norm"], want["total_norm"])
        assert _close(got["clip_coef"], want["clip_coef"], 2e-6), (name, s, got["clip_coef"], want["clip_coef"])
        if not math.isnan(want["clip_coef"]):
            assert got["clip_coef"] <= 1.0 and (got["clip_coef"] == 1.0) == (want["clip_coef"] == 1.0)


def _gate_figures(label, device, oracle, torch32):
    """[(what, tensor, product error, torch float32 error, bound)] for p, m, v of every tensor."""
    rows = []
    for what, got, want, ref in (("p", device[0], oracle.p, torch32[0]), ("m", device[1], oracle.m, torch32[1]),
                                 ("v", device[2], oracle.v, torch32[2])):
        for t in range(len(want)):
            e_got, e_ref = O.tensor_error(got[t], want[t]), O.tensor_error(ref[t], want[t])
            rows.append((what, t, e_got, e_ref, O.gate(e_ref, want[t])))
            print(f"{label} {what}[{t}] n={want[t].numel()}: product {e_got:.3e} torch32 {e_ref:.3e} bound {rows[-1][4]:.3e}")
    return rows


@pytest.mark.parametrize("name", list(O.SCENARIOS))
def test_parity_after_three_steps(runs, name):
    r = runs[name]
    assert r["device"][3] == r["oracle"].step_count == r["torch32"][3]
    for what, t, e_got, e_ref, bound in _gate_figures(name, r["device"], r["oracle"], r["torch32"]):
        assert e_got <= bound, (name, what, t, e_got, e_ref, bound)


@pytest.mark.parametrize("mutant", ["beta2", "noclip", "coupled"])
def test_gate_catches_mutants(runs, goldens, mutant):
    """The gate is worth something: with the bounds it has for the true oracle, an oracle with one deliberate mistake
    (standing for a kernel that makes it) fails against the same device results."""
    name = "clean_clipped"
    r = runs[name]
    wrong, _ = O.run_scenario(name, goldens["base"], mutant=mutant)
    failures = 0
    for what, got, want, bad, ref in (("p", r["device"][0], r["oracle"].p, wrong.p, r["torch32"][0]),
                                      ("m", r["device"][1], r["oracle"].m, wrong.m, r["torch32"][1]),
                                      ("v", r["device"][2], r["oracle"].v, wrong.v, r["torch32"][2])):
        for t in range(len(want)):
            bound = O.gate(O.tensor_error(ref[t], want[t]), want[t])
            failures += O.tensor_error(got[t], bad[t]) > bound
    print(f"mutant {mutant}: {failures} of {3 * len(O.SHAPES)} tensor gates fail")
    assert failures >= len(O.SHAPES), (mutant, failures)


def test_skipped_step_leaves_everything_bitwise(goldens):
    """Parameters, both moments and all step counters after a skipped step are those before it -- for a NaN and for a
    large gradient, with moments that are not zero."""
    import spfsplatv2_amd as spf
    base = goldens["base"]
    live = [torch.nn.Parameter(p.to(DEV)) for p in base["params"]]
    opt = spf.GuardedAdamW(live, lr=1e-3, betas=(0.9, 0.95), weight_decay=0.05)
    for p, g in zip(live, base["grads"][0]):
        p.grad = (g * 0.01).to(DEV)
    opt.step()
    assert not opt.last_step.skipped.item()

    def snapshot():
        sd = opt.state_dict()["state"]
        return ([p.detach().clone() for p in live], [sd[i]["exp_avg"].clone() for i in range(len(live))],
                [sd[i]["exp_avg_sq"].clone() for i in range(len(live))], [float(sd[i]["step"]) for i in range(len(live))])

    before = snapshot()
    assert before[3] == [1.0] * len(live) and float(before[1][6].abs().max()) > 0
    for value, field in ((math.nan, "nan_detected"), (1e3, "large_detected")):
        for p, g in zip(live, base["grads"][1]):
            p.grad = (g * 0.01).to(DEV)
        live[6].grad[4096] = value
        opt.step()
        rep = _read(opt.last_step)
        assert rep["skipped"] == 1 and rep[field] == 1 and rep["offender"] == 6 and opt.last_step.offender_name() == "group0.param6"
        after = snapshot()
        for a, b in zip(before[:3], after[:3]):
            for x, y in zip(a, b):
                assert torch.equal(x, y)
        assert after[3] == before[3]


SHAPES_NUMEL = (1, 3, 4095, 4096, 4097)


def _shapes_case(seed=7):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=gen) * 0.3 for n in SHAPES_NUMEL]
    groups = [dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, tensors=[0, 2, 4]),
              dict(lr=3e-4, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, tensors=[1, 3])]
    grads = [[torch.randn(n, generator=gen) * 0.02 for n in SHAPES_NUMEL] for _ in range(3)]
    grads[1][3] = None                                           # a gradient missing in between
    lrs = [[g["lr"] * f for g in groups] for f in (1.0, 0.5, 0.25)]
    return params, groups, grads, lrs


@pytest.mark.parametrize("offset", [0, 1, 3])
def test_shapes_and_addresses(offset):
    """numel 1, 3, 4095, 4096, 4097; parameters and gradients that are ``buffer[offset:]`` (4-byte but not 16-byte
    aligned: the scalar path); gradients at new addresses on every step; one gradient None at the middle step."""
    params, groups, grads, lrs = _shapes_case()
    device = device_run(params, groups, grads, lrs, 5.0, 0.5, offset=offset)
    oracle, oracle_reports = O.oracle_run(params, groups, grads, lrs, 5.0, 0.5)
    torch32 = O.torch_run(params, groups, grads, lrs, 5.0, 0.5)
    assert device[3] == oracle.step_count == [3, 3, 3, 2, 3]
    for got, want in zip(device[4], oracle_reports):
        assert got["skipped"] == 0 and got["offender"] == -1
        assert _bits(got["max_gradient"]) == _bits(want["max_gradient"])
        assert _close(got["total_norm"], want["total_norm"], 2e-6) and _close(got["clip_coef"], want["clip_coef"], 2e-6)
    for what, t, e_got, e_ref, bound in _gate_figures(f"shapes+{offset}", device, oracle, torch32):
        assert e_got <= bound, (offset, what, t, e_got, e_ref, bound)


def test_large_tensor_wraps_the_grid():
    """One tensor of 2 * 2^20 * 4 + 5 floats next to a small one: 2049 chunks on at most 2048 blocks, so the grid-stride
    loop wraps, and the last chunk holds 5 floats."""
    n = 2 * 2 ** 20 * 4 + 5
    gen = torch.Generator().manual_seed(11)
    params = [torch.randn(n, generator=gen) * 0.3, torch.randn(7, generator=gen)]
    groups = [dict(lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, tensors=[0, 1])]
    grads = [[torch.randn(n, generator=gen) * 1e-3, torch.randn(7, generator=gen) * 1e-3] for _ in range(2)]
    grads[1][0][n - 1] = 4.5                                     # the maximum sits in the partial last chunk
    lrs = [[1e-3], [5e-4]]
    device = device_run(params, groups, grads, lrs, 5.0, 0.5)
    oracle, oracle_reports = O.oracle_run(params, groups, grads, lrs, 5.0, 0.5)
    torch32 = O.torch_run(params, groups, grads, lrs, 5.0, 0.5)
    for got, want in zip(device[4], oracle_reports):
        assert got["skipped"] == 0 and _bits(got["max_gradient"]) == _bits(want["max_gradient"])
        assert _close(got["total_norm"], want["total_norm"], 2e-6) and _close(got["clip_coef"], want["clip_coef"], 2e-6)
    assert device[4][1]["max_gradient"] == 4.5
    for what, t, e_got, e_ref, bound in _gate_figures("large", device, oracle, torch32):
        assert e_got <= bound, (what, t, e_got, e_ref, bound)


def test_three_steps_without_a_host_sync(goldens):
    """After the first step (which builds the table) three steps, their gradient uploads and ``zero_grad`` included, raise
    nothing under ``set_sync_debug_mode("error")``; reading a value of the report then does."""
    import spfsplatv2_amd as spf
    base = goldens["base"]
    live = [torch.nn.Parameter(p.to(DEV)) for p in base["params"]]
    opt = spf.GuardedAdamW([dict(params=live[:3], lr=1e-3), dict(params=live[3:], lr=1e-4)], betas=(0.9, 0.95),
                           weight_decay=0.05, named_parameters=zip(O.NAMES, live))
    sched = torch.optim.lr_scheduler.LinearLR(opt, 0.25, 1.0, total_iters=4)
    grads = [[(g * 0.01).to(DEV) for g in base["grads"][s % 3]] for s in range(4)]
    for p, g in zip(live, grads[3]):
        p.grad = g
    opt.step()                                                   # warm-up: table, scratch, pinned buffers
    opt.zero_grad()
    sched.step()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for s in range(3):
            for p, g in zip(live, grads[s]):
                p.grad = g
            if s == 1:
                live[2].grad = None
            opt.step()
            opt.zero_grad()
            sched.step()
        report = opt.last_step
        with pytest.raises(RuntimeError):                        # the caller's own sync, and only then
            report.max_gradient.item()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-3) and float(report.max_gradient) > 0
    steps = [int(st["step"]) for st in opt.state_dict()["state"].values()]
    assert steps == [4, 4, 3, 4, 4, 4, 4, 4]


def test_two_runs_agree_bitwise(runs, goldens):
    """The same inputs twice: every output -- parameters, moments, step counts, every field of every report -- agrees
    bit for bit (and on another allocation, with misaligned bases, the sums keep their order too)."""
    for name in ("clean_clipped", "absent_at_step_2", "large_second_nan_sixth"):
        first, second = runs[name]["device"], _scenario_device(name, goldens["base"])
        third = _scenario_device(name, goldens["base"], offset=1)
        for other in (second, third):
            for a, b in zip(first[:3], other[:3]):
                for x, y in zip(a, b):
                    assert torch.equal(x, y), name
            assert first[3] == other[3]
            for ra, rb in zip(first[4], other[4]):
                assert {f: _bits(float(ra[f])) for f in REPORT_FIELDS} == {f: _bits(float(rb[f])) for f in REPORT_FIELDS}
