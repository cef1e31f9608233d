"""Argument checks shared by the modules that call the HIP library (block.py, heads.py, tail.py)."""
from __future__ import annotations

import torch


def check_float32(what: str, *tensors) -> None:
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
        if t.dtype in (torch.float16, torch.bfloat16):
            raise NotImplementedError(f"{what}: {t.dtype} is not supported; these layers run in float32")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{what}: unsupported dtype {t.dtype}")


def check_device(what: str, first, *others) -> None:
    """The last check of every call."""
    if not first.is_cuda:
        raise RuntimeError(f"{what}: the tensors are on the CPU; this build only runs on a HIP device (no CPU fallback)")
    if any(t is not None and t.device != first.device for t in others):
        raise RuntimeError(f"{what}: the tensors are not on one device")

