"""The guarded AdamW step on the HIP library (spfsplatv2_amd/csrc/optim.hip): the reference's ``optimizer_step`` hook --
NaN / large-gradient guard, ``clip_grad_norm_`` and ``torch.optim.AdamW.step()`` -- as three launches over the whole
parameter set and no host synchronisation.

=================================  ====================================================================================
here                               reference (/root/reference/src/)
=================================  ====================================================================================
``GuardedAdamW``                   model/model_wrapper.py:1067-1111 (``configure_optimizers``: ``torch.optim.AdamW`` with
                                   two groups, ``betas=(0.9, 0.95)``, ``weight_decay=0.05``) and :1113-1151
                                   (``optimizer_step``: the per-parameter guard loop, ``clip_grad_norm_(.., 0.5)``, the step)
``StepReport``                     what that hook logs and prints: ``max_gradient``, the NaN / large verdict, the offender
=================================  ====================================================================================

What the hook does, mirrored here: tensors are walked in ``named_parameters`` order; a tensor without gradient is passed
over; NaN is tested before the maximum of the same tensor and ends the walk; a maximum STRICTLY above the threshold ends it
too; ``max_gradient`` covers the tensors up to and including a large offender and up to but excluding a NaN one; an
offender skips the step.  Otherwise the gradients are scaled by ``min(1, max_norm / (total_norm + 1e-6))`` and AdamW steps
every parameter that has a gradient, each with its own step count.  The clipped gradient is not written back: the
reference drops it in ``zero_grad()`` right after.

With ``max_grad_value=None`` and ``max_norm=None`` this is ``torch.optim.AdamW``; with ``weight_decay=0`` on top,
``torch.optim.Adam``.  With the guard off, non-finite gradients flow through as in torch.

Out of scope: graph capture of the step, the compiled host binding, 16-bit parameters, ``amsgrad``, ``maximize`` and the
``foreach`` / ``fused`` / ``capturable`` / ``differentiable`` switches.  CPU tensors raise: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch
from torch import Tensor

from . import _lib

_NAME = "GuardedAdamW"


class StepReport:
    """The report block of the last step, as 0-dim views of device memory: nothing here synchronises until a value is
    read (``float(report.max_gradient)``, ``bool(report.skipped)``, printing).  Every step overwrites the block, so the
    views always show the most recent step."""

    def __init__(self, block: Tensor, names: list[str]):
        floats = block.view(torch.float32)
        self.skipped, self.nan_detected, self.large_detected, self.offender = block[0], block[1], block[2], block[3]
        self.max_gradient, self.total_norm, self.clip_coef = floats[4], floats[5], floats[6]
        self.names = names

    def offender_name(self):
        """The name of the tensor that made the step skip, or None.  Synchronises."""
        i = int(self.offender)
        return None if i < 0 else self.names[i]


class _Slot:
    """One pinned buffer of gradient addresses and the event that says its copy is done."""

    def __init__(self, n: int):
        self.pinned = torch.empty(n, dtype=torch.int64).pin_memory()
        self.array = self.pinned.numpy()
        self.event = torch.cuda.Event()
        self.pending = False


class _Plan:
    pass


class GuardedAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` with the reference's guard and clip in front, stepped by HIP kernels.

    ``max_grad_value``: the guard's threshold (the reference: 5, or 20 with a VGGT backbone); ``None`` = no guard.
    ``max_norm``: the clip's norm; ``None`` = no clip.  ``named_parameters``: an iterable of ``(name, parameter)`` that
    fixes the order of the guard's walk and the names of the report (default: the groups in order).
    ``param_groups[i]["lr"]`` is read on the host at every step, so the schedulers drive it unchanged."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *,
                 maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                 max_grad_value=5.0, max_norm=0.5, named_parameters=None):
        if isinstance(lr, Tensor):
            raise RuntimeError(f"{_NAME}: lr must be a number (it is read on the host every step), not a tensor")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_value is not None and not max_grad_value >= 0:
            raise ValueError(f"Invalid max_grad_value: {max_grad_value}")
        if max_norm is not None and not max_norm >= 0:
            raise ValueError(f"Invalid max_norm: {max_norm}")
        self.max_grad_value = max_grad_value
        self.max_norm = max_norm
        self._names_by_id = None if named_parameters is None else [(str(n), p) for n, p in named_parameters]
        self._plan = None
        self._moments: dict[Tensor, tuple[Tensor, Tensor]] = {}
        self._host_steps: dict[Tensor, int] = {}
        self._steps_dev = None
        self._steps_params: list[Tensor] = []
        self._ring: list[_Slot] = []
        self._report = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)
        self._check_groups()

    # ---- refusals (all before any launch) ----------------------------------------------------------------------------
    def _check_groups(self, params: bool = True) -> None:
        """The group switches, and (``params``) every parameter's layout and type."""
        if len(self.param_groups) > _lib.OPTIM_MAX_GROUPS:
            raise RuntimeError(f"{_NAME}: {len(self.param_groups)} parameter groups; at most {_lib.OPTIM_MAX_GROUPS} are "
                               "supported")
        for gi, group in enumerate(self.param_groups):
            for key in ("amsgrad", "maximize", "foreach", "capturable", "differentiable", "fused"):
                if group.get(key):
                    raise RuntimeError(f"{_NAME}: {key}={group[key]!r} (group {gi}) is not supported")
            if isinstance(group["lr"], Tensor):
                raise RuntimeError(f"{_NAME}: lr of group {gi} must be a number, not a tensor")
            if not params:
                continue
            for j, p in enumerate(group["params"]):
                if p.is_sparse:
                    raise RuntimeError(f"{_NAME}: parameter {j} of group {gi} is sparse; only dense tensors are supported")
                if p.dtype != torch.float32:
                    raise RuntimeError(f"{_NAME}: parameter {j} of group {gi} must be float32, got {p.dtype}")
                if p.numel() == 0:
                    raise RuntimeError(f"{_NAME}: parameter {j} of group {gi} is empty ({tuple(p.shape)})")

    @staticmethod
    def _check_tensor(what: str, t: Tensor, dev) -> None:
        if not t.is_cuda:
            raise RuntimeError(f"{_NAME}: {what} is on {t.device}; this build only runs on a HIP device (no CPU fallback)")
        if t.is_sparse:
            raise RuntimeError(f"{_NAME}: {what} is sparse; only dense tensors are supported")
        if t.dtype != torch.float32:
            raise RuntimeError(f"{_NAME}: {what} must be float32, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{_NAME}: {what} is not contiguous (shape {tuple(t.shape)}, strides {t.stride()})")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"{_NAME}: {what} is on {t.device}, the first parameter on {dev}; one device per optimizer")

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if getattr(self, "_ring", None) is not None:        # (the base constructor comes through here before ours is done)
            self._check_groups()
            self._plan = None

    # ---- state ---------------------------------------------------------------------------------------------------------
    def _flat(self):
        return [(p, gi) for gi, g in enumerate(self.param_groups) for p in g["params"]]

    def _moments_of(self, p: Tensor):
        mv = self._moments.get(p)
        if mv is None:
            mv = self._moments[p] = (torch.zeros_like(p, memory_format=torch.contiguous_format),
                                     torch.zeros_like(p, memory_format=torch.contiguous_format))
        return mv

    def _steps_now(self) -> dict:
        """{parameter: steps taken}.  Synchronises when steps live on the device."""
        steps = dict(self._host_steps)
        if self._steps_dev is not None:
            for p, n in zip(self._steps_params, self._steps_dev.cpu().tolist()):
                steps[p] = n
        return steps

    def state_dict(self):
        """``torch.optim.AdamW``'s format: ``step`` (a float32 scalar on the CPU), ``exp_avg``, ``exp_avg_sq`` for every
        parameter that has stepped.  May synchronise."""
        steps = self._steps_now()
        self.state.clear()
        try:
            for p, _ in self._flat():
                n = steps.get(p, 0)
                if n > 0:
                    m, v = self._moments_of(p)
                    self.state[p] = {"step": torch.tensor(float(n), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
            return super().state_dict()
        finally:
            self.state.clear()

    def load_state_dict(self, state_dict) -> None:
        """Takes a state dict of this class or of ``torch.optim.AdamW`` (a checkpoint of the reference).  Parameters
        without an entry start afresh, as in torch."""
        self.state.clear()
        super().load_state_dict(state_dict)
        try:
            self._check_groups()
            moments, steps = {}, {}
            for p, st in self.state.items():
                if "exp_avg" not in st or "exp_avg_sq" not in st or "step" not in st:
                    raise RuntimeError(f"{_NAME}: a state entry lacks step / exp_avg / exp_avg_sq (not an AdamW state)")
                # (copies: torch hands over the state dict's own tensors, which may be another optimizer's live state)
                m = st["exp_avg"].to(device=p.device, dtype=torch.float32, copy=True).contiguous()
                v = st["exp_avg_sq"].to(device=p.device, dtype=torch.float32, copy=True).contiguous()
                if m.shape != p.shape or v.shape != p.shape:
                    raise RuntimeError(f"{_NAME}: a loaded moment has shape {tuple(m.shape)}, its parameter {tuple(p.shape)}")
                moments[p] = (m, v)
                steps[p] = int(round(float(st["step"])))
        finally:
            self.state.clear()
        self._moments, self._host_steps = moments, steps
        self._steps_dev, self._steps_params, self._plan = None, [], None

    # ---- the device plan: table, chunk starts, guard order, scratch --------------------------------------------------
    def _upload(self, plan, array: np.ndarray, dev) -> Tensor:
        """Host array -> device through a pinned buffer that the plan keeps alive: no blocking copy."""
        host = torch.from_numpy(np.ascontiguousarray(array)).pin_memory()
        plan.keep.append(host)
        return host.to(dev, non_blocking=True)

    def _make_plan(self):
        self._check_groups()
        flat = self._flat()
        if not flat:
            raise RuntimeError(f"{_NAME}: no parameters")
        dev = None
        for i, (p, gi) in enumerate(flat):
            self._check_tensor(f"parameter {i} (group {gi})", p, dev)
            dev = p.device
        lib = _lib.load()
        T = len(flat)
        plan = _Plan()
        plan.keep = []
        plan.params = [p for p, _ in flat]
        plan.device = dev
        table = (_lib.SpfOptimTensor * T)()
        with torch.cuda.device(dev):
            for i, (p, gi) in enumerate(flat):
                m, v = self._moments_of(p)
                self._check_tensor(f"a moment of parameter {i}", m, dev)
                self._check_tensor(f"a moment of parameter {i}", v, dev)
                table[i] = _lib.SpfOptimTensor(p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), gi, 0)
            starts = (C.c_int64 * (T + 1))()
            chunks = lib.spf_optim_plan(table, T, len(self.param_groups), starts)
            if chunks < 0:
                _lib.check(int(chunks), "spf_optim_plan")
            plan.param_ptrs = [p.data_ptr() for p in plan.params]
            plan.moments = [self._moments[p] for p in plan.params]
            # guard order: named_parameters' order where given, then whatever it does not name, in group order
            index = {p: i for i, p in enumerate(plan.params)}
            order, names, seen = [], [], set()
            for name, p in self._names_by_id or ():
                i = index.get(p)
                if i is not None and i not in seen:
                    seen.add(i)
                    order.append(i)
                    names.append(name)
            counters = [0] * len(self.param_groups)
            for i, (p, gi) in enumerate(flat):
                if i not in seen:
                    order.append(i)
                    names.append(f"group{gi}.param{counters[gi]}")
                counters[gi] += 1
            plan.names = names
            plan.table = self._upload(plan, np.frombuffer(table, dtype=np.uint8), dev)
            plan.chunk_start = self._upload(plan, np.frombuffer(starts, dtype=np.int64), dev)
            plan.guard_order = self._upload(plan, np.asarray(order, dtype=np.int32), dev)
            plan.grads = torch.zeros(T, dtype=torch.int64, device=dev)
            plan.scratch = torch.empty(int(lib.spf_optim_scratch_bytes(T, chunks)), dtype=torch.uint8, device=dev)
            if self._report is None or self._report.device != dev:
                self._report = torch.zeros(8, dtype=torch.int32, device=dev)
                self._report[3] = -1
            # step counters: carried over while the parameter list only grows; otherwise from the host's copy
            if self._steps_dev is not None and self._steps_dev.device == dev and \
                    [id(p) for p in self._steps_params] == [id(p) for p in plan.params[:len(self._steps_params)]]:
                extra = T - len(self._steps_params)
                if extra:
                    self._steps_dev = torch.cat([self._steps_dev, torch.zeros(extra, dtype=torch.int32, device=dev)])
            else:
                steps = self._steps_now()
                self._steps_dev = self._upload(plan, np.asarray([steps.get(p, 0) for p in plan.params], np.int32), dev)
            self._steps_params = list(plan.params)
            self._host_steps = {}
        plan.args = _lib.SpfOptim(plan.table.data_ptr(), plan.chunk_start.data_ptr(), plan.grads.data_ptr(),
                                  plan.guard_order.data_ptr(), self._steps_dev.data_ptr(), plan.scratch.data_ptr(),
                                  self._report.data_ptr(), T, 0, int(chunks))
        plan.ptrs = [0] * T
        plan.report = StepReport(self._report, names)
        self._ring = []
        self._plan = plan
        return plan

    def _slot(self, n: int) -> _Slot:
        """A pinned buffer whose last copy is done -- never one that may still be read; the ring grows instead of waiting."""
        for s in self._ring:
            if not s.pending or s.event.query():
                s.pending = False
                return s
        s = _Slot(n)
        self._ring.append(s)
        return s

    def _hyper(self) -> _lib.SpfOptimHyper:
        hp = _lib.SpfOptimHyper()
        hp.num_groups = len(self.param_groups)
        hp.guard = int(self.max_grad_value is not None)
        hp.clip = int(self.max_norm is not None)
        hp.max_grad_value = float(self.max_grad_value) if hp.guard else 0.0
        hp.max_norm = float(self.max_norm) if hp.clip else 0.0
        for gi, g in enumerate(self.param_groups):
            b1, b2 = g["betas"]
            hp.group[gi] = _lib.SpfOptimGroup(float(g["lr"]), float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]))
        return hp

    @property
    def last_step(self) -> StepReport:
        """The report of the most recent step (device tensors; reading a value is the caller's synchronisation)."""
        if self._plan is None:
            raise RuntimeError(f"{_NAME}: no step has been taken yet")
        return self._plan.report

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._plan
        if plan is not None:                                   # a parameter or a moment that moved: plan again
            for p, (m, v), ptr in zip(plan.params, plan.moments, plan.param_ptrs):
                if p.data_ptr() != ptr or self._moments.get(p, (None, None))[0] is not m:
                    plan = None
                    break
        if plan is None:
            plan = self._make_plan()
        else:
            self._check_groups(params=False)               # (a scheduler or a loaded checkpoint may have touched the groups)
        dev = plan.device
        ptrs = plan.ptrs
        for i, p in enumerate(plan.params):
            g = p.grad
            if g is None:
                ptrs[i] = 0
                continue
            if not (g.is_cuda and g.dtype == torch.float32 and not g.is_sparse and g.is_contiguous() and g.device == dev):
                self._check_tensor(f"the gradient of parameter {i}", g, dev)
            if g.shape != p.shape:
                raise RuntimeError(f"{_NAME}: the gradient of parameter {i} has shape {tuple(g.shape)}, not {tuple(p.shape)}")
            ptrs[i] = g.data_ptr()
        hp = self._hyper()
        with torch.cuda.device(dev):
            slot = self._slot(len(ptrs))
            slot.array[:] = ptrs
            plan.grads.copy_(slot.pinned, non_blocking=True)
            slot.event.record(torch.cuda.current_stream(dev))
            slot.pending = True
        _lib.launch("spf_optim_step", dev, plan.args, hp)
        return loss
