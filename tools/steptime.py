"""What every tools/<component>_time.py has in common: how a step is timed, how inputs are kept cold, how host syncs and
bytes are counted, how two variants are told apart from the spread of one, and how a result line is written.

A tool runs as ``python tools/x.py``, so ``tools/`` is ``sys.path[0]`` and ``import steptime`` finds this file.  Nothing
here knows a component, and importing it imports no torch: every function that needs a device imports torch itself.

Two protocols, never mixed within one figure:
  sequential   ``median_ms``: warm one variant up, time it --iters times, go on to the next variant
  alternating  ``alternate``: warm the variants up, then time them in turn step by step (``schedule``) on rotating input
               sets, then run one more step per variant for bytes, syncs and the outputs
"""
from __future__ import annotations

import csv
import json
import statistics
import sys
import warnings
from pathlib import Path

CACHE_BYTES = 256 << 20          # the last-level cache of one MI355X


# ---- one step ----------------------------------------------------------------------------------------------------------
def timed(fn) -> float:
    """Milliseconds between two device events around ``fn()``."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _stats(times, ms_max=False):
    res = {"ms_median": statistics.median(times), "ms_min": min(times)}
    if ms_max:
        res["ms_max"] = max(times)
    return res


def median_ms(fn, warmup, iters, sets=None, before=None, ms_max=False):
    """The sequential protocol: ``warmup`` calls, a device sync, ``iters`` timed calls.  With ``sets`` call i is
    ``fn(sets[i % len(sets)])``, in the warm-up and in the timed loop alike; ``before()`` runs ahead of every call,
    outside the timed window."""
    import torch

    def call(i):
        return (lambda: fn(sets[i % len(sets)])) if sets is not None else fn
    for i in range(warmup):
        if before is not None:
            before()
        call(i)()
    torch.cuda.synchronize()
    times = []
    for i in range(iters):
        if before is not None:
            before()
        times.append(timed(call(i)))
    return _stats(times, ms_max)


def is_sync_warning(message: str) -> bool:
    """Whether a warning raised under torch's sync debug mode reports a synchronising call.  The mode's own
    once-per-process notice ("Synchronization debug mode is a prototype feature ...") names the word too and is no sync."""
    return "synchroniz" in message.lower() and "prototype" not in message


def syncs_and_result(fn):
    """(the synchronising calls torch reports during ``fn()`` (torch.cuda.set_sync_debug_mode("warn")), what it returned)"""
    import torch
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            res = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum(is_sync_warning(str(w.message)) for w in seen), res


def count_syncs(fn) -> int:
    return syncs_and_result(fn)[0]


def peak_step(fn, held=False):
    """One run of ``fn`` for bytes: (what it returned, the peak of torch's allocator during it above what was allocated
    before it, held bytes).  With ``held`` the call is ``fn(between)``, and ``between()``, which ``fn`` calls after its
    forward, notes what is allocated there above the same base; without it held bytes are None."""
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    noted = []
    res = fn(lambda: noted.append(torch.cuda.memory_allocated() - base)) if held else fn()
    torch.cuda.synchronize()
    return res, torch.cuda.max_memory_allocated() - base, noted[0] if held else None


# ---- cold inputs -------------------------------------------------------------------------------------------------------
def tensor_bytes(o) -> int:
    """Bytes of every tensor in a nest of dicts, lists and tuples (a tensor met twice counts twice)."""
    if hasattr(o, "element_size"):
        return o.numel() * o.element_size()
    if isinstance(o, dict):
        return sum(tensor_bytes(x) for x in o.values())
    if isinstance(o, (list, tuple)):
        return sum(tensor_bytes(x) for x in o)
    return 0


def input_sets(make_one, min_sets=2, cache_bytes=CACHE_BYTES, extra=0):
    """(sets, bytes of one set): enough sets from ``make_one()`` that a rotation over them exceeds twice the last-level
    cache, so that every step reads cold lines; at least ``min_sets``, and ``extra`` more than the rule asks."""
    one = make_one()
    set_bytes = tensor_bytes(one)
    nsets = max(min_sets, -(-2 * cache_bytes // set_bytes) + extra)
    return [one] + [make_one() for _ in range(nsets - 1)], set_bytes


# ---- the alternating protocol ------------------------------------------------------------------------------------------
def schedule(variants, iters, nsets):
    """(i, variant, set index) of every timed step, in the order they run: the variants take turns within round i, and
    the set index moves on with every step, so each variant meets every set."""
    for i in range(iters):
        for vi, var in enumerate(variants):
            yield i, var, (len(variants) * i + vi) % nsets


def alternate(variants, steps, sets, warmup, iters, *, warm=None, prepare=None, held=False, syncs=False, ms_max=False,
              label=None):
    """The alternating protocol over ``steps[variant](set, *prepared)``.

    Warm-up: every variant of ``warm`` (default: all) runs ``warmup`` times, on set i % len(sets).  Timing: ``schedule``,
    one event pair per step.  Then per variant one more step on set 0 for the peak bytes -- with ``held`` it is called
    with ``between=`` a hook the step calls after its forward, for the bytes held there -- and, with ``syncs``, another
    one under ``count_syncs``.  ``prepare(set)`` runs before every step, outside the timed window and before the bytes'
    base is read.  ``label`` prints progress lines to stderr.

    Returns ({variant: record}, {variant: what the bytes step returned}); a record holds ms_median, ms_min[, ms_max],
    bytes_allocated_peak[, bytes_held_after_forward][, host_syncs], iters, warmup.
    """
    import torch
    prepare = prepare or (lambda s: ())
    say = (lambda text: print(f"{label}: {text}", file=sys.stderr, flush=True)) if label else (lambda text: None)
    for var in variants if warm is None else warm:
        for i in range(warmup):
            steps[var](sets[i % len(sets)], *prepare(sets[i % len(sets)]))
        torch.cuda.synchronize()
        say(f"{var} warm")
    times = {var: [] for var in variants}
    for i, var, si in schedule(variants, iters, len(sets)):
        prepared = prepare(sets[si])
        times[var].append(timed(lambda: steps[var](sets[si], *prepared)))
        del prepared
        if var == variants[-1] and i % 5 == 4:
            say(f"{i + 1} rounds")
    records, outputs = {}, {}
    for var in variants:
        prepared = prepare(sets[0])
        if held:
            outputs[var], peak, kept = peak_step(lambda between: steps[var](sets[0], *prepared, between=between), True)
        else:
            outputs[var], peak, kept = peak_step(lambda: steps[var](sets[0], *prepared))
        records[var] = {**_stats(times[var], ms_max), "bytes_allocated_peak": peak}
        if held:
            records[var]["bytes_held_after_forward"] = kept
        if syncs:
            records[var]["host_syncs"] = count_syncs(lambda: steps[var](sets[0], *prepared))
        del prepared
        records[var].update(iters=iters, warmup=warmup)
    return records, outputs


def spread_summary(ms_base, ms_new, ms_repeat):
    """``ms_base`` and ``ms_repeat`` are two runs of one variant in the same rotation: their distance is the spread a
    difference to ``ms_new`` has to exceed to mean anything.  The gain is taken from the faster of the two."""
    spread, lo, hi = abs(ms_base - ms_repeat), min(ms_base, ms_repeat), max(ms_base, ms_repeat)
    return {"spread_ms": spread, "gain_ms": lo - ms_new, "speedup": lo / ms_new,
            "faster_beyond_spread": bool(lo - ms_new > spread), "slower_beyond_spread": bool(ms_new - hi > spread)}


def rel_diff(x, y) -> float:
    x, y = x.detach(), y.detach()
    return float((x - y).abs().max() / y.abs().max().clamp_min(1e-30))


def max_rel_diff(xs, ys) -> float:
    """The largest max|x - y| / max|y| over two lists of tensors."""
    return max(rel_diff(x, y) for x, y in zip(xs, ys))


# ---- rocprofv3 kernel statistics (no GPU needed) -----------------------------------------------------------------------
def kernel_stats(path, prefixes, need, rates, width, named=False):
    """{kernel name: calls, mean time, and for the kernels of ``need`` {short name: bytes} the bytes over the mean time as
    a share of every rate of ``rates`` {key: B/s}} of the kernels of a ``rocprofv3 --kernel-trace --stats``
    kernel_stats.csv whose name holds one of ``prefixes``."""
    kernels = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            if not any(p in name for p in prefixes):
                continue
            avg = float(row.get("AverageNs") or row.get("AverageNs ") or 0)
            short = name.split("(")[0].split("<")[0].split("::")[-1].strip()
            ent = {"calls": int(float(row.get("Calls") or 0)), "avg_us": avg / 1e3}
            if named:
                ent["name"] = name[:width]
            if short in need and avg > 0:
                bps = need[short] / (avg * 1e-9)
                ent.update(bytes=need[short], GBps=bps / 1e9, **{key: bps / rate for key, rate in rates.items()})
            kernels[name[:width]] = ent
    return kernels


# ---- the command line's common end -------------------------------------------------------------------------------------
def require_counts(tool, args, min_iters, min_warmup):
    if args.iters < min_iters or args.warmup < min_warmup:
        raise SystemExit(f"{tool}.py: the median is taken over at least {min_iters} steps after at least {min_warmup} "
                         f"warm-ups")


def require_gpu(tool):
    """The result's header; without a GPU the tool ends here (nothing is ever timed on the CPU)."""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}.py needs a GPU")
    return {"tool": tool, "device": torch.cuda.get_device_name(0)}


def note(result):
    """One finished result: its JSON line to stderr, and the allocator's cache handed back before the next one."""
    import torch
    print(json.dumps(result), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    return result


def emit(res, out):
    """The whole result as one JSON line: written to ``out`` (if given; its directory is made) and printed."""
    line = json.dumps(res)
    if out:
        Path(out).parent.mkdir(parents=True, exist_ok=True)
        Path(out).write_text(line + "\n")
    print(line)
