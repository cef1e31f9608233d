"""tools/steptime.py, the measurement module every tools/<component>_time.py stands on, and the tools' command lines --
everything of them that needs no GPU."""
import argparse
import importlib
import json
import subprocess
import sys
from pathlib import Path

import pytest

TOOLS_DIR = Path(__file__).resolve().parents[1] / "tools"
if str(TOOLS_DIR) not in sys.path:                    # as `python tools/x.py` has it
    sys.path.insert(0, str(TOOLS_DIR))

import steptime  # noqa: E402

# tool: (its least --iters, its least --warmup)
TOOLS = {"attention_time": (100, 20), "attention_views_time": (100, 20), "vggt_attention_time": (100, 20),
         "block_time": (100, 20), "dpt_time": (10, 3), "front_time": (10, 3), "tail_time": (10, 3), "posehead_time": (10, 3),
         "pnp_time": (10, 3), "pose_time": (100, 20), "regr3d_time": (100, 0), "reproj_time": (2, 0), "ssim_time": (2, 0),
         "lpips_time": (2, 0), "optim_time": (100, 20)}


def test_every_time_tool_is_listed():
    assert sorted(p.stem for p in TOOLS_DIR.glob("*_time.py")) == sorted(TOOLS)


# ---- schedule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvar,nsets", [(2, 2), (3, 2), (4, 2), (2, 3), (3, 4), (4, 5), (3, 7)])
def test_schedule_is_the_alternating_loop(nvar, nsets):
    variants = tuple(f"v{k}" for k in range(nvar))
    iters = nsets + 2
    want = [(i, var, (len(variants) * i + vi) % nsets) for i in range(iters) for vi, var in enumerate(variants)]
    assert list(steptime.schedule(variants, iters, nsets)) == want


@pytest.mark.parametrize("nvar,nsets", [(2, 3), (3, 2), (3, 4), (4, 5), (3, 7), (2, 5)])
def test_schedule_shows_every_set_to_every_variant(nvar, nsets):
    """nsets coprime to the variant count, iters >= nsets"""
    variants = tuple(range(nvar))
    met = {var: set() for var in variants}
    for _, var, si in steptime.schedule(variants, nsets, nsets):
        met[var].add(si)
    assert all(m == set(range(nsets)) for m in met.values())


# ---- input sets --------------------------------------------------------------------------------------------------------
class Buf:
    """what tensor_bytes asks of a tensor"""
    def __init__(self, n, size=4):
        self.n, self.size = n, size

    def numel(self):
        return self.n

    def element_size(self):
        return self.size


def test_tensor_bytes_walks_nests():
    assert steptime.tensor_bytes({"a": Buf(10), "b": [Buf(3, 2), (Buf(1), "text")], "c": 5}) == 40 + 6 + 4


@pytest.mark.parametrize("set_bytes,min_sets,want", [(4096, 2, 2), (512, 2, 16), (8196, 2, 2), (8196, 3, 3), (4100, 2, 2),
                                                     (4092, 2, 3), (3000, 2, 3)])
def test_input_sets_exceed_twice_the_cache(set_bytes, min_sets, want):
    made = []

    def make_one():
        made.append({"x": Buf(set_bytes // 4), "y": [Buf(set_bytes % 4, 1)]})
        return made[-1]
    sets, nbytes = steptime.input_sets(make_one, min_sets=min_sets, cache_bytes=4096)
    assert nbytes == set_bytes and len(sets) == want and sets == made
    if want > min_sets:                                   # the rule, and no set more than it asks
        assert want * set_bytes >= 2 * 4096 > (want - 1) * set_bytes


def test_input_sets_extra_and_default_cache():
    assert len(steptime.input_sets(lambda: Buf(128), cache_bytes=4096, extra=1)[0]) == 17
    assert steptime.CACHE_BYTES == 256 << 20
    assert len(steptime.input_sets(lambda: Buf(32 << 20, 1))[0]) == 16


# ---- the sync warnings -------------------------------------------------------------------------------------------------
# c10's texts (c10/cuda/CUDAFunctions.cpp, CUDAMiscFunctions / hipified alike): warn_or_error_on_sync and the notice
# torch.cuda.set_sync_debug_mode raises once per process
SYNC_TEXTS = ["called a synchronizing CUDA operation", "called a synchronizing HIP operation"]
NOTICE = "Synchronization debug mode is a prototype feature and does not yet detect all synchronizing operations"


def test_sync_warning_classifier():
    assert all(steptime.is_sync_warning(t) for t in SYNC_TEXTS)
    assert steptime.is_sync_warning(SYNC_TEXTS[1] + " (Triggered internally at /x/y.cpp:12.)")
    assert not steptime.is_sync_warning(NOTICE)
    assert not steptime.is_sync_warning(NOTICE + " (Triggered internally at /x/y.cpp:12.)")
    assert not steptime.is_sync_warning("an output with one or more elements was resized")


def test_sync_texts_are_the_installed_torch_s():
    import torch
    lib = Path(torch.__file__).parent / "lib"
    c10 = [p.read_bytes() for name in ("libc10_hip.so", "libc10_cuda.so") for p in [lib / name] if p.exists()]
    if c10:                                               # (a torch laid out otherwise: the texts above are the tools' own)
        assert any(t.encode() in b for t in SYNC_TEXTS for b in c10)
    if (lib / "libtorch_python.so").exists():
        assert NOTICE.encode() in (lib / "libtorch_python.so").read_bytes()


# ---- spread ------------------------------------------------------------------------------------------------------------
def test_spread_summary_faster():
    s = steptime.spread_summary(10.0, 6.0, 11.0)
    assert s == {"spread_ms": 1.0, "gain_ms": 4.0, "speedup": 10.0 / 6.0, "faster_beyond_spread": True,
                 "slower_beyond_spread": False}


def test_spread_summary_repeat_below_base():
    s = steptime.spread_summary(10.0, 8.5, 9.0)            # the gain counts from the faster of the two runs
    assert (s["spread_ms"], s["gain_ms"], s["speedup"]) == (1.0, 0.5, 9.0 / 8.5)
    assert s["faster_beyond_spread"] is False and s["slower_beyond_spread"] is False


def test_spread_summary_gain_equal_to_the_spread_is_not_beyond():
    s = steptime.spread_summary(8.0, 6.0, 10.0)
    assert s["gain_ms"] == s["spread_ms"] == 2.0 and s["faster_beyond_spread"] is False
    s = steptime.spread_summary(8.0, 12.0, 10.0)           # slower by exactly the spread: not beyond either
    assert s["slower_beyond_spread"] is False and s["faster_beyond_spread"] is False


def test_spread_summary_slower():
    s = steptime.spread_summary(10.0, 14.0, 11.0)
    assert s["gain_ms"] == -4.0 and s["speedup"] == 10.0 / 14.0
    assert s["faster_beyond_spread"] is False and s["slower_beyond_spread"] is True
    assert all(type(s[k]) is bool for k in ("faster_beyond_spread", "slower_beyond_spread"))


def test_max_rel_diff():
    import torch
    a, b = torch.tensor([1.0, -4.0]), torch.tensor([1.5, -4.0]).requires_grad_(True)
    assert steptime.rel_diff(a, b) == 0.125 and steptime.max_rel_diff([a, b], [b, b]) == 0.125
    assert steptime.max_rel_diff([a, torch.zeros(2)], [a, torch.zeros(2)]) == 0.0


# ---- the command line's common end -------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters,warmup", [(9, 3), (10, 2)])
def test_require_counts_names_the_tool_and_both_minima(iters, warmup):
    with pytest.raises(SystemExit) as e:
        steptime.require_counts("some_time", argparse.Namespace(iters=iters, warmup=warmup), 10, 3)
    assert str(e.value) == "some_time.py: the median is taken over at least 10 steps after at least 3 warm-ups"
    steptime.require_counts("some_time", argparse.Namespace(iters=10, warmup=3), 10, 3)


def test_emit_writes_one_line_into_a_new_directory(tmp_path, capsys):
    out = tmp_path / "not" / "there" / "x.json"
    steptime.emit({"tool": "x", "results": [1, 2]}, str(out))
    assert out.read_text() == '{"tool": "x", "results": [1, 2]}\n'
    assert capsys.readouterr().out == out.read_text()
    steptime.emit({"a": 1}, None)
    assert capsys.readouterr().out == '{"a": 1}\n'


# ---- the tools ---------------------------------------------------------------------------------------------------------
def test_importing_the_tools_imports_no_torch():
    code = ("import sys, importlib\n"
            f"for name in {sorted(TOOLS) + ['steptime']!r}:\n"
            "    importlib.import_module(name)\n"
            "assert 'torch' not in sys.modules, 'a tool imported torch at import time'\n")
    subprocess.run([sys.executable, "-c", code], cwd=TOOLS_DIR, check=True, timeout=120)


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_guards_its_own_minima(tool, monkeypatch):
    min_iters, min_warmup = TOOLS[tool]
    mod = importlib.import_module(tool)
    monkeypatch.setattr(sys, "argv", [tool + ".py", "--iters", "1"])
    with pytest.raises(SystemExit) as e:
        mod.main()
    assert str(e.value) == (f"{tool}.py: the median is taken over at least {min_iters} steps after at least "
                            f"{min_warmup} warm-ups")


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_tool_needs_a_gpu(tool, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(sys, "argv", [tool + ".py"])
    with pytest.raises(SystemExit) as e:
        importlib.import_module(tool).main()
    assert str(e.value) == f"{tool}.py needs a GPU"


STATS_CSV = '''"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"
"void spf_ssim_fwd_kernel<4>(float const*, float const*, float*, int)",20,2000000,100000.0,40.0,90000,110000,5000.0
"spf_reproj_bwd_kernel(float const*, float*, int)",40,8000000,200000.0,50.0,190000,210000,4000.0
"at::native::vectorized_elementwise_kernel<4, at::native::FillFunctor<float>>",7,70000,10000.0,10.0,9000,11000,100.0
"spf_ssim_bwd_kernel(float const*, float const*, float const*, float*, float*, int)",20,6000000,300000.0,0.0,1,2,0.0
"spf_reproj_fwd_kernel(float const*, float*, int)",40,4000000,100000.0,0.0,1,2,0.0
'''
# what the tools printed for that file before they shared kernel_stats (the templated name has no byte model: its
# short name keeps the "void ")
STATS_WANT = {
    "ssim_time": ("test_step", {"shape": "test_step", "elements": 589824, "kernels": {
        "void spf_ssim_fwd_kernel<4>(float const*, float const*, float*, int)": {"calls": 20, "avg_us": 100.0},
        "spf_ssim_bwd_kernel(float const*, float const*, float const*, float*, float*, int)": {
            "calls": 20, "avg_us": 300.0, "bytes": 9437184, "GBps": 31.457279999999997, "share_of_peak": 0.00393216}}}),
    "reproj_time": ("re10k_10view", {"shape": "re10k_10view", "points": 1966080, "kernels": {
        "spf_reproj_bwd_kernel(float const*, float*, int)": {
            "calls": 40, "avg_us": 200.0, "name": "spf_reproj_bwd_kernel(float const*, float*, int)", "bytes": 47185920,
            "GBps": 235.9296, "share_of_peak": 0.0294912, "share_of_achievable": 0.037449142857142854},
        "spf_reproj_fwd_kernel(float const*, float*, int)": {
            "calls": 40, "avg_us": 100.0, "name": "spf_reproj_fwd_kernel(float const*, float*, int)", "bytes": 23592960,
            "GBps": 235.9296, "share_of_peak": 0.0294912, "share_of_achievable": 0.037449142857142854}}}),
}


@pytest.mark.parametrize("tool", sorted(STATS_WANT))
def test_stats_mode_needs_no_gpu_and_prints_what_it_did(tool, tmp_path, monkeypatch, capsys):
    shape, want = STATS_WANT[tool]
    (tmp_path / "kernel_stats.csv").write_text(STATS_CSV)
    monkeypatch.setattr(sys, "argv", [tool + ".py", "--stats", str(tmp_path / "kernel_stats.csv"), "--shapes", shape])
    importlib.import_module(tool).main()
    out = capsys.readouterr().out
    assert out.endswith("\n") and out.count("\n") == 1
    assert json.loads(out) == want
    assert list(json.loads(out)["kernels"]) == list(want["kernels"])         # in the file's order
