"""CPU side of the attention tests with free positions and parameters (tests/test_gpu_attention_params.py):

1. the oracle's rotation with ``F0`` (tests/attention_oracle.py:rope2d) is the reference's: at F0 = 1 it is
   oracle/rope_torch_ref.py's fallback, and it reproduces tests/golden/rope_goldens.pt at the goldens' base and F0;
2. THE POWER CONDITION of the device tests, from the oracle alone: at the shapes, dtypes and position ranges those tests
   use, reading the wrong positions (another batch item's, scene's or view's table, y and x swapped, ONE key's position)
   or a default in place of ``scale`` / ``base`` / ``F0`` moves every gated tensor by at least 4 x the bound the gate
   allows it (2 x eager + eps, eager being the oracle in the call's dtype, here on the CPU).  A condition on the tests,
   not a measurement: where a range misses it, the range is narrowed (tests/attention_params_cases.py:POS_RANGE).
"""
import pytest
import torch

from oracle.rope_torch_ref import rope2d_fallback
from tests import attention_oracle as oracle
from tests import attention_params_cases as cases
from tests import util


# ---- 1. the rotation -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [100.0, 10.0])
def test_rope2d_at_unit_F0_is_the_fallback(base):
    gen = torch.Generator().manual_seed(7)
    tok = torch.randn(3, 2, 37, 64, generator=gen, dtype=torch.float64)
    pos = torch.randint(0, 40, (3, 37, 2), generator=gen)
    got, want = oracle.rope2d(tok, pos, base, 1.0), rope2d_fallback(tok, pos, base)
    assert got.dtype == torch.float64
    assert float((got - want).abs().max()) <= 1e-14 * float(want.abs().max())
    for dtype in (torch.float32, torch.float16, torch.bfloat16):       # dtype-generic, and the fallback there too
        assert torch.equal(oracle.rope2d(tok.to(dtype), pos, base), rope2d_fallback(tok.to(dtype), pos, base))


@pytest.fixture(scope="module")
def goldens(golden_dir):
    return torch.load(golden_dir / "rope_goldens.pt")


def test_rope2d_reproduces_the_reference_goldens(goldens):
    """Both of the reference's paths, within tests/test_rope_oracle.py's tolerances: its PyTorch fallback (1e-6, that
    test's bound for a restatement in the same torch ops) and its compiled C++ loop, the one that takes F0 (1e-5, that
    test's bound between a torch evaluation and the C++ loop: the two reference paths themselves differ by 4e-6)."""
    assert len(goldens["cases"]) >= 5
    for name, c in goldens["cases"].items():
        got = oracle.rope2d(c["tokens_BHND"], c["positions"], c["base"], c["F0"])
        assert float((got.transpose(1, 2) - c["out_cpp_BNHD"]).abs().max()) <= 1e-5, name
        if c["F0"] == 1.0:                           # (the fallback module ignores F0 in its tables)
            assert float((got - c["out_fallback_BHND"]).abs().max()) <= 1e-6, name


@pytest.mark.parametrize("base,F0", [(100.0, 0.5), (10.0, 0.5), (1000.0, 2.0), (100.0, -1.0)])
def test_rope2d_with_F0_is_the_compiled_loop(base, F0):
    """The goldens hold F0 = 1 only; the C restatement of curope.cpp's loop (oracle/rope_ref.c, pinned to the goldens by
    tests/test_rope_oracle.py) takes F0: float32 against float32, angles up to 2 * 39."""
    gen = torch.Generator().manual_seed(11)
    tok = torch.randn(2, 3, 29, 64, generator=gen)
    pos = torch.randint(0, 40, (2, 29, 2), generator=gen)
    want = util.rope_oracle(tok.transpose(1, 2), pos, base, F0).transpose(1, 2)
    assert float((oracle.rope2d(tok, pos, base, F0) - want).abs().max()) <= 1e-5
    assert float((oracle.rope2d(tok, pos, base, 1.0) - want).abs().max()) > 0.1      # and F0 is not ignored


# ---- 2. the power condition ------------------------------------------------------------------------------------------
def _assert_power(label, run, x64, dists, dtype, names=cases.NAMES):
    assert dists, label
    e_eager = cases.errs(run(dtype=dtype), x64)
    for n, e in zip(names, e_eager):
        print(f"{label} {n}: eager {e:.3e} bound {2 * e + cases.eps_of(dtype):.3e}")
    bad = cases.power_failures(label, dists, e_eager, cases.eps_of(dtype), names)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("run", cases.POSITION_RUNS, ids=cases.run_id)
def test_wrong_positions_are_four_bounds_away(run):
    layout, name, variant, dtype = run
    inp, fn, x64, dists = cases.reference(*run)
    assert len(dists) == (6 if layout == "views" else 4)
    _assert_power(cases.run_id(run), fn, x64, dists, dtype)


@pytest.mark.parametrize("cfg", cases.SETTINGS, ids=lambda c: "s%g_b%g_f%g" % c)
@pytest.mark.parametrize("run", cases.PARAMETER_RUNS, ids=cases.run_id)
def test_default_parameters_are_four_bounds_away(run, cfg):
    inp, fn, x64, dists = cases.reference(*run, cfg)
    assert len(dists) == sum(a != b for a, b in zip(cfg, cases.DEFAULT))
    _assert_power(cases.run_id(run + (cfg,)), fn, x64, dists, run[3])


@pytest.mark.parametrize("dtype", [cases.F32, cases.F16, cases.BF16], ids=cases.dtype_id)
def test_default_scale_without_rope_is_four_bounds_away(dtype):
    inp, fn, x64, dists = cases.reference("flat", cases.CROSS, "plain", dtype, cases.NOROPE_SCALE, False)
    assert list(dists) == ["scale 0.125 for 0.2"]
    _assert_power("norope-" + cases.dtype_id(dtype), fn, x64, dists, dtype)


MODULE_RUNS = [(k, cases.F32) for k in ("self", "cross", "views")] + [(k, d) for k in ("self", "cross")
                                                                      for d in (cases.F16, cases.BF16)]


@pytest.mark.parametrize("kind,dtype", MODULE_RUNS, ids=lambda x: x if isinstance(x, str) else cases.dtype_id(x))
def test_modules_default_rope_is_four_bounds_away(kind, dtype):
    """The modules at cuRoPE2D(10, 0.5): the oracle at base 100 or at F0 1 instead.  Asked of the per-token tensors, the
    output and the gradients of the inputs: a parameter's gradient is a sum over every token, a bias' over nothing else,
    and the device test gates those too but does not rest on them (at bfloat16 the wrong base moves two bias gradients of
    the cross module by 3.8 bounds only)."""
    case, names, x64, dists = cases.module_reference(kind, dtype)
    eager = cases.module_tensors(cases.module_oracle(case, dtype), names)
    n = 1 + len(case["inputs"])
    e_eager = cases.errs(eager[:n], x64[:n])
    bad = cases.power_failures(f"module-{kind}-{cases.dtype_id(dtype)}", dists, e_eager, cases.eps_of(dtype), names[:n])
    assert not bad, "\n".join(bad)
