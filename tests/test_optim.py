"""The guarded AdamW step without a GPU: the float64 oracle against the reference's goldens and against live torch, the
spf_optim_* argument checks and chunk arithmetic, every Python refusal, and the state dict round trip."""
import ctypes as C
import math

import pytest
import torch

from tests import optim_oracle as O


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return torch.load(golden_dir / "optim_goldens.pt", weights_only=False)


def _rel(got, want):
    """max |got - want| relative to the tensor's largest magnitude.  (Not element by element: an element of a moment that
    is the small remainder of a cancellation, m + 0.1 (g - m) with m ~ g, carries the float64 rounding of its operands,
    not of itself -- the reference's own result is no better known than that.)"""
    want = want.double()
    return float((got.double() - want).abs().max() / want.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("name", list(O.SCENARIOS))
def test_oracle_reproduces_the_reference_float64(goldens, name):
    """The oracle over the three steps of every scenario: parameters and moments within 1e-12 relative of what the
    reference's hook left (float64 run), step counts, verdicts and the logged max_gradient exactly."""
    base, gold = goldens["base"], goldens["scenarios"][name]["float64"]
    oracle, reports = O.run_scenario(name, base)
    assert oracle.step_count == gold["step"]
    for rep, log in zip(reports, gold["logs"]):
        assert (rep["skipped"], rep["nan_detected"], rep["large_detected"]) == \
               (log["skipped"], log["nan_detected"], log["large_detected"])
        assert rep["max_gradient"] == log["max_gradient"]
        want = O.NAMES.index(log["offender"]) if log["offender"] else None
        if log["large_detected"]:
            assert rep["offender"] == want
        assert (rep["offender"] >= 0) == log["skipped"]
    for t in range(len(O.SHAPES)):
        pick = O.sample_index(oracle.p[t].numel())
        for got, want in ((oracle.p[t], gold["p"][t]), (oracle.m[t], gold["m"][t]), (oracle.v[t], gold["v"][t])):
            assert want.dtype == torch.float64
            assert _rel(got.view(-1)[pick], want) <= 1e-12, (name, t)


def test_golden_scenarios_are_what_the_issue_lists(goldens):
    """The recorded runs show each scenario's point: which steps were skipped, by what, and whose step count lags."""
    logs = {n: [(lg["skipped"], lg["nan_detected"], lg["large_detected"]) for lg in s["float32"]["logs"]]
            for n, s in goldens["scenarios"].items()}
    step, skip_nan, skip_large = (False, False, False), (True, True, False), (True, False, True)
    assert logs["clean_small_norm"] == [step] * 3 and logs["clean_clipped"] == [step] * 3
    assert logs["at_threshold"] == [step] * 3 and logs["above_threshold"] == [step, skip_large, step]
    assert goldens["scenarios"]["at_threshold"]["float32"]["logs"][1]["max_gradient"] == 5.0
    assert goldens["scenarios"]["above_threshold"]["float32"]["logs"][1]["max_gradient"] == O.NEXT_ABOVE_5 > 5.0
    assert logs["nan_fifth"] == [step, skip_nan, step]
    assert logs["large_second_nan_sixth"] == [step, skip_large, step]
    assert goldens["scenarios"]["large_second_nan_sixth"]["float32"]["logs"][1]["max_gradient"] == 7.5
    assert logs["nan_and_large_same"] == [step, skip_nan, step]
    assert goldens["scenarios"]["nan_and_large_same"]["float32"]["logs"][1]["max_gradient"] < 1.0
    assert logs["infinities"] == [skip_large, step, skip_large]
    assert goldens["scenarios"]["infinities"]["float32"]["logs"][0]["max_gradient"] == math.inf
    assert goldens["scenarios"]["absent_at_step_2"]["float32"]["step"] == [3, 3, 3, 2, 3, 3, 3, 2]
    assert logs["threshold_20"] == [step, step, skip_large]
    assert goldens["scenarios"]["threshold_20"]["float32"]["logs"][1]["max_gradient"] == 10.0
    assert set(goldens["scenarios"]) == set(O.SCENARIOS)


@pytest.mark.parametrize("name", ["clean_clipped", "absent_at_step_2", "adam_step_align"])
def test_live_torch_float32_is_the_references_float32(goldens, name):
    """``optim_oracle.run_torch`` -- the float32 yardstick of the GPU gate -- gives bit for bit what the reference's hook
    gave in float32."""
    gold = goldens["scenarios"][name]["float32"]
    p, m, v, steps = O.run_torch(name, goldens["base"])
    assert steps == gold["step"]
    for t in range(len(O.SHAPES)):
        pick = O.sample_index(p[t].numel())
        for got, want in ((p[t], gold["p"][t]), (m[t], gold["m"][t]), (v[t], gold["v"][t])):
            assert torch.equal(got.view(-1)[pick], want), (name, t)


@pytest.mark.parametrize("seed", [1, 2])
def test_oracle_equals_live_torch_float64(seed):
    """Fresh seeds, float64: the oracle against ``torch.optim.AdamW`` + ``clip_grad_norm_`` run live, five steps, one
    tensor without gradient at one step, both sides of the clip."""
    gen = torch.Generator().manual_seed(seed)
    shapes = ((7,), (3, 5), (129,), (2, 3, 4))
    params = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    groups = [dict(lr=3e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.05, tensors=[1, 3]),
              dict(lr=4e-4, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0, tensors=[0, 2])]
    oracle = O.Oracle(params, groups, threshold=None, max_norm=0.5)
    live = [torch.nn.Parameter(p.clone()) for p in params]
    opt = torch.optim.AdamW([dict(params=[live[t] for t in g["tensors"]], lr=g["lr"], betas=g["betas"], eps=g["eps"],
                                  weight_decay=g["weight_decay"]) for g in groups])
    for s in range(5):
        scale = 0.01 if s % 2 else 1.0
        grads = [torch.randn(sh, generator=gen, dtype=torch.float64) * scale for sh in shapes]
        if s == 2:
            grads[2] = None
        lrs = [g["lr"] * (1.0 - 0.1 * s) for g in groups]
        for gi, lr in enumerate(lrs):
            opt.param_groups[gi]["lr"] = lr
        for p, g in zip(live, grads):
            p.grad = None if g is None else g.clone()
        want_norm = torch.nn.utils.clip_grad_norm_(live, 0.5)
        opt.step()
        rep = oracle.step(grads, lrs)
        assert abs(rep["total_norm"] - float(want_norm)) <= 1e-14 * float(want_norm)
        assert (rep["clip_coef"] == 1.0) == (float(want_norm) + 1e-6 < 0.5)
    assert oracle.step_count == [5, 5, 4, 5]
    for t, p in enumerate(live):
        assert _rel(oracle.p[t], p.detach()) <= 1e-12
        assert _rel(oracle.m[t], opt.state[p]["exp_avg"]) <= 1e-12
        assert _rel(oracle.v[t], opt.state[p]["exp_avg_sq"]) <= 1e-12


def test_mutants_differ_from_the_oracle(goldens):
    """The three deliberate mistakes move the float64 result by far more than float32 rounding -- so a float32 gate can
    tell them apart (tests/test_gpu_optim.py checks that its gate does)."""
    good, _ = O.run_scenario("clean_clipped", goldens["base"])
    for mutant in ("beta2", "noclip", "coupled"):
        bad, _ = O.run_scenario("clean_clipped", goldens["base"], mutant=mutant)
        worst = max(float((bad.p[t] - good.p[t]).abs().max()) for t in range(len(O.SHAPES)))
        assert worst > 1e-5, (mutant, worst)


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def _table(entries):
    from spfsplatv2_amd import _lib
    table = (_lib.SpfOptimTensor * len(entries))()
    for i, (numel, group) in enumerate(entries):
        table[i] = _lib.SpfOptimTensor(64, 128, 192, numel, group, 0)
    return table


def test_optim_chunks_and_plan(hip_lib):
    from spfsplatv2_amd import _lib
    assert _lib.OPTIM_CHUNK == 4096 and _lib.OPTIM_MAX_GROUPS == 8
    numel = [1, 3, 4095, 4096, 4097, 2 * 2 ** 20 * 4 + 5]
    want = [1, 1, 1, 1, 2, 2049]
    arr = (C.c_int64 * len(numel))(*numel)
    assert hip_lib.spf_optim_chunks(arr, len(numel)) == sum(want)
    for n, w in zip(numel, want):
        assert hip_lib.spf_optim_chunks((C.c_int64 * 1)(n), 1) == w
    starts = (C.c_int64 * (len(numel) + 1))()
    assert hip_lib.spf_optim_plan(_table([(n, i % 2) for i, n in enumerate(numel)]), len(numel), 2, starts) == sum(want)
    assert list(starts) == [0, 1, 2, 3, 4, 6, 2055]
    assert hip_lib.spf_optim_scratch_bytes(6, 2055) == 16 * 2055 + 24 * 6
    assert C.sizeof(_lib.SpfOptimTensor) == 40 and C.sizeof(_lib.SpfOptimGroup) == 40
    assert C.sizeof(_lib.SpfOptimHyper) == 32 + 8 * 40 and C.sizeof(_lib.SpfOptim) == 72


def test_optim_argument_refusals(hip_lib):
    """Bad arguments return -1 with a message, before anything touches a device."""
    from spfsplatv2_amd import _lib

    def err():
        return hip_lib.spf_last_error()

    assert hip_lib.spf_optim_chunks(None, 3) == -1 and b"null" in err()
    assert hip_lib.spf_optim_chunks((C.c_int64 * 1)(5), 0) == -1 and b"T must be positive" in err()
    assert hip_lib.spf_optim_chunks((C.c_int64 * 2)(5, 0), 2) == -1 and b"numel" in err()
    assert hip_lib.spf_optim_plan(None, 1, 1, None) == -1 and b"table is null" in err()
    assert hip_lib.spf_optim_plan(_table([(5, 0)]), 0, 1, None) == -1 and b"T must be positive" in err()
    assert hip_lib.spf_optim_plan(_table([(5, 0), (-1, 0)]), 2, 1, None) == -1 and b"numel" in err()
    assert hip_lib.spf_optim_plan(_table([(5, 0)]), 1, 9, None) == -1 and b"groups" in err()
    assert hip_lib.spf_optim_plan(_table([(5, 0)]), 1, 0, None) == -1 and b"groups" in err()
    assert hip_lib.spf_optim_plan(_table([(5, 0), (5, 2)]), 2, 2, None) == -1 and b"out of range" in err()
    assert hip_lib.spf_optim_plan(_table([(5, -1)]), 1, 2, None) == -1 and b"out of range" in err()
    assert hip_lib.spf_optim_scratch_bytes(0, 5) == -1 and hip_lib.spf_optim_scratch_bytes(4, 3) == -1

    hp = _lib.SpfOptimHyper(num_groups=1, guard=1, clip=1, max_grad_value=5.0, max_norm=0.5)
    hp.group[0] = _lib.SpfOptimGroup(1e-3, 0.9, 0.95, 1e-8, 0.05)
    ok = dict(table=256, chunk_start=256, grads=256, guard_order=256, step=256, scratch=256, report=256, T=2, chunks=2)

    def step(hyper=hp, **change):
        return hip_lib.spf_optim_step(C.byref(_lib.SpfOptim(**{**ok, **change})), C.byref(hyper), None)

    assert hip_lib.spf_optim_step(None, C.byref(hp), None) == -1 and b"null" in err()
    assert step(table=None) == -1 and b"table is null" in err()
    assert step(T=0) == -1 and b"T must be positive" in err()
    assert step(T=-3) == -1 and b"T must be positive" in err()
    assert step(chunks=1) == -1 and b"chunks" in err()
    for field in ("chunk_start", "grads", "guard_order", "step", "scratch", "report"):
        assert step(**{field: None}) == -1 and b"null pointer" in err(), field
    assert step(scratch=260) == -1 and b"16-byte" in err()
    many = _lib.SpfOptimHyper(num_groups=9, guard=1, clip=1, max_grad_value=5.0, max_norm=0.5)
    assert step(hyper=many) == -1 and b"groups" in err()
    bad = _lib.SpfOptimHyper(num_groups=1, guard=1, clip=1, max_grad_value=5.0, max_norm=0.5)
    bad.group[0] = _lib.SpfOptimGroup(1e-3, 1.0, 0.95, 1e-8, 0.05)
    assert step(hyper=bad) == -1 and b"betas" in err()


# ---- Python --------------------------------------------------------------------------------------------------------------
def test_exported():
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import optim
    for name in ("GuardedAdamW", "StepReport"):
        assert name in spf.__all__ and getattr(spf, name) is getattr(optim, name)
    assert issubclass(spf.GuardedAdamW, torch.optim.Optimizer)


def _params(*shapes, **kwargs):
    return [torch.nn.Parameter(torch.zeros(s, **kwargs)) for s in shapes]


def test_python_refusals_before_any_launch(hip_lib, monkeypatch):
    """Every refusal is raised on the host: the library's step entry point is never reached."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import _lib

    def no_launch(*args):
        raise AssertionError("spf_optim_step was reached")

    monkeypatch.setattr(_lib.load(), "spf_optim_step", no_launch)
    opt = spf.GuardedAdamW(_params((4,), (2, 3)), lr=1e-3)
    for p in opt.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(RuntimeError, match="no step has been taken"):
        opt.last_step
    with pytest.raises(RuntimeError, match="must be float32"):
        spf.GuardedAdamW(_params((4,), dtype=torch.float64))
    with pytest.raises(RuntimeError, match="must be float32"):
        spf.GuardedAdamW(_params((4,), dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="sparse"):
        spf.GuardedAdamW([torch.zeros(4, 4).to_sparse().requires_grad_(True)])
    with pytest.raises(RuntimeError, match="at most 8"):
        spf.GuardedAdamW([dict(params=_params((2,))) for _ in range(9)])
    spf.GuardedAdamW([dict(params=_params((2,))) for _ in range(8)])
    with pytest.raises(RuntimeError, match="amsgrad"):
        spf.GuardedAdamW(_params((4,)), amsgrad=True)
    with pytest.raises(RuntimeError, match="maximize"):
        spf.GuardedAdamW(_params((4,)), maximize=True)
    with pytest.raises(RuntimeError, match="maximize"):
        spf.GuardedAdamW([dict(params=_params((4,)), maximize=True)])
    with pytest.raises(RuntimeError, match="fused"):
        spf.GuardedAdamW(_params((4,)), fused=True)
    with pytest.raises(RuntimeError, match="foreach"):
        spf.GuardedAdamW(_params((4,)), foreach=True)
    with pytest.raises(ValueError, match="learning rate"):
        spf.GuardedAdamW(_params((4,)), lr=-1.0)
    with pytest.raises(ValueError, match="beta"):
        spf.GuardedAdamW(_params((4,)), betas=(0.9, 1.0))
    late = spf.GuardedAdamW(_params((4,)))
    with pytest.raises(RuntimeError, match="at most 8"):
        for _ in range(8):
            late.add_param_group(dict(params=_params((2,))))
    # the checks a tensor meets at the step, on the host function itself (a CPU tensor stops the step earlier)
    check = spf.GuardedAdamW._check_tensor
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        check("x", torch.zeros(3), None)


def test_tensor_checks_of_the_step():
    """``_check_tensor`` on stand-ins that claim to be device tensors: dtype, layout, contiguity, device."""
    import spfsplatv2_amd as spf

    class Fake:
        is_cuda, is_sparse, dtype, device, shape = True, False, torch.float32, "cuda:0", (4, 4)

        def __init__(self, **kw):
            self.__dict__.update(kw)
            self._contiguous = kw.get("contiguous", True)

        def is_contiguous(self):
            return self._contiguous

        def stride(self):
            return (1, 4)

    check = spf.GuardedAdamW._check_tensor
    check("x", Fake(), "cuda:0")
    with pytest.raises(RuntimeError, match="must be float32"):
        check("x", Fake(dtype=torch.float16), None)
    with pytest.raises(RuntimeError, match="sparse"):
        check("x", Fake(is_sparse=True), None)
    with pytest.raises(RuntimeError, match="not contiguous"):
        check("x", Fake(contiguous=False), None)
    with pytest.raises(RuntimeError, match="one device per optimizer"):
        check("x", Fake(device="cuda:1"), "cuda:0")


def test_state_dict_round_trip_with_torch_adamw():
    """``torch.optim.AdamW``'s state dict loads here and ours loads there, entries only for parameters that stepped --
    on CPU tensors, so nothing is launched."""
    import spfsplatv2_amd as spf
    gen = torch.Generator().manual_seed(5)
    shapes = ((4,), (2, 3), (5,))
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    groups = lambda: [dict(params=ps[:2], lr=1e-3), dict(params=ps[2:], lr=1e-4)]      # noqa: E731
    ref = torch.optim.AdamW(groups(), betas=(0.9, 0.95), weight_decay=0.05)
    for n in range(3):
        for i, p in enumerate(ps):
            p.grad = None if (i == 1 and n < 2) or i == 2 else torch.randn(p.shape, generator=gen)
        ref.step()                                     # steps: 3, 1, none
    import copy
    sd = copy.deepcopy(ref.state_dict())               # (a state dict holds the optimizer's live tensors)
    assert sorted(sd["state"]) == [0, 1]

    ours = spf.GuardedAdamW(groups(), betas=(0.5, 0.5), weight_decay=0.0)
    assert ours.state_dict()["state"] == {}
    ours.load_state_dict(sd)
    back = ours.state_dict()
    assert sorted(back["state"]) == [0, 1]
    for i in (0, 1):
        assert float(back["state"][i]["step"]) == float(sd["state"][i]["step"]) == (3.0, 1.0)[i]
        assert back["state"][i]["step"].dtype == torch.float32 and back["state"][i]["step"].device.type == "cpu"
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(back["state"][i][key], sd["state"][i][key])
    for got, want in zip(back["param_groups"], sd["param_groups"]):
        for key in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "params"):
            assert got[key] == want[key], key
    assert ours.param_groups[0]["betas"] == (0.9, 0.95) and ours.param_groups[1]["lr"] == 1e-4

    fresh = torch.optim.AdamW(groups())
    fresh.load_state_dict(back)
    again = fresh.state_dict()
    assert sorted(again["state"]) == [0, 1]
    for i in (0, 1):
        assert float(again["state"][i]["step"]) == float(sd["state"][i]["step"])
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(again["state"][i][key], sd["state"][i][key])
    for p in ps:                                       # and torch steps on from it exactly as from its own
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    fresh.step()
    after_ours = [p.detach().clone() for p in ps]
    with torch.no_grad():
        for p, b in zip(ps, before):
            p.copy_(b)
    ref.step()
    for a, p in zip(after_ours, ps):
        assert torch.equal(a, p.detach())

    bad = {"state": {0: {"step": torch.tensor(1.0)}}, "param_groups": sd["param_groups"]}
    with pytest.raises(RuntimeError, match="not an AdamW state"):
        ours.load_state_dict(bad)
