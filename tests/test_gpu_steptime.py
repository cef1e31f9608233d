"""tools/steptime.py on a device: the harness itself, on two trivial steps (it tests no speed).  The tests run in the
file's order: the first one holds the process's first counted call, the one torch's prototype notice rides on."""
import math
import sys
from pathlib import Path

import pytest
import torch

TOOLS_DIR = Path(__file__).resolve().parents[1] / "tools"
if str(TOOLS_DIR) not in sys.path:
    sys.path.insert(0, str(TOOLS_DIR))

import steptime  # noqa: E402

pytestmark = pytest.mark.gpu
WARMUP, ITERS = 3, 5


def make_x(gen):
    return torch.randn(64, 64, generator=gen).cuda()


def test_count_syncs_from_the_first_counted_call_on():
    x = make_x(torch.Generator().manual_seed(0))
    x @ x                                                                 # (the BLAS handle's set-up is not the step's)
    assert steptime.count_syncs(lambda: x @ x) == 0                       # the notice comes with this call, and is no sync
    assert steptime.count_syncs(lambda: (x @ x).sum().item()) == 1
    assert steptime.count_syncs(lambda: x @ x) == 0
    syncs, res = steptime.syncs_and_result(lambda: float((x @ x).relu().sum()))
    assert syncs == 1 and math.isfinite(res)


def test_timed_and_median_ms():
    x = make_x(torch.Generator().manual_seed(0))
    ms = steptime.timed(lambda: x @ x)
    assert math.isfinite(ms) and ms > 0
    calls = []
    sets = [make_x(torch.Generator().manual_seed(i)) for i in range(2)]
    res = steptime.median_ms(lambda s: calls.append(s) or s @ s, WARMUP, ITERS, sets=sets, before=lambda: calls.append("b"),
                             ms_max=True)
    assert set(res) == {"ms_median", "ms_min", "ms_max"} and 0 < res["ms_min"] <= res["ms_median"] <= res["ms_max"]
    assert calls[0::2] == ["b"] * (WARMUP + ITERS)
    assert all(c is sets[i % 2] for i, c in zip([*range(WARMUP), *range(ITERS)], calls[1::2]))
    assert set(steptime.median_ms(lambda: x @ x, WARMUP, ITERS)) == {"ms_median", "ms_min"}


def test_alternate_three_variants():
    gen = torch.Generator().manual_seed(0)
    sets, set_bytes = steptime.input_sets(lambda: {"x": make_x(gen)}, cache_bytes=64 * 64 * 4)
    assert set_bytes == 64 * 64 * 4 and len(sets) == 2
    seen = {"base": [], "new": [], "repeat": []}

    def step(var, fn):
        def run(s, between=None):
            seen[var].append((next(i for i, t in enumerate(sets) if t is s), between is not None))
            out = fn(s["x"])
            if between is not None:
                between()
            return [out, out.sum()]
        return run
    base = lambda x: x @ x                                                # noqa: E731
    steps = {"base": step("base", base), "new": step("new", lambda x: (x @ x).relu()), "repeat": step("repeat", base)}
    variants = ("base", "new", "repeat")
    records, outputs = steptime.alternate(variants, steps, sets, WARMUP, ITERS, warm=variants[:2], held=True, syncs=True,
                                          ms_max=True)
    assert list(records) == list(variants) == list(outputs)
    for var in variants:
        r = records[var]
        assert set(r) == {"ms_median", "ms_min", "ms_max", "bytes_allocated_peak", "bytes_held_after_forward", "host_syncs",
                          "iters", "warmup"}
        assert (r["iters"], r["warmup"], r["host_syncs"]) == (ITERS, WARMUP, 0)
        assert 0 < r["ms_min"] <= r["ms_median"] <= r["ms_max"]
        assert r["bytes_allocated_peak"] >= r["bytes_held_after_forward"] >= 64 * 64 * 4          # the output is held
        # warm-ups (not for the repeat), the schedule's steps, the bytes step with its hook, the counted step
        warm = [(i % 2, False) for i in range(WARMUP)] if var != "repeat" else []
        timed = [(si, False) for _, v, si in steptime.schedule(variants, ITERS, 2) if v == var]
        assert seen[var] == warm + timed + [(0, True), (0, False)] and len(timed) == ITERS
    assert steptime.max_rel_diff(outputs["repeat"], outputs["base"]) == 0.0
    assert steptime.max_rel_diff(outputs["new"], outputs["base"]) > 0.0
    plain, _ = steptime.alternate(variants[:2], {v: (lambda s, v=v: steps[v](s)) for v in variants[:2]}, sets, WARMUP, ITERS)
    assert all(set(r) == {"ms_median", "ms_min", "bytes_allocated_peak", "iters", "warmup"} for r in plain.values())


def test_alternate_prepares_outside_the_step():
    sets = [{"x": make_x(torch.Generator().manual_seed(i))} for i in range(3)]
    order = []

    def prepare(s):
        order.append("p")
        return (s["x"] * 1,)

    def step(s, copy):
        order.append("s")
        return copy @ s["x"]
    records, outputs = steptime.alternate(("a", "b"), {"a": step, "b": step}, sets, WARMUP, ITERS, prepare=prepare)
    assert order == ["p", "s"] * (2 * (WARMUP + ITERS + 1))
    assert torch.equal(outputs["a"], outputs["b"]) and torch.equal(outputs["a"], sets[0]["x"] @ sets[0]["x"])


def test_peak_step():
    x = make_x(torch.Generator().manual_seed(0))
    res, peak, held = steptime.peak_step(lambda: x @ x)
    assert held is None and peak >= res.numel() * 4
