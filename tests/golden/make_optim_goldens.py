"""Golden vectors for the guarded AdamW step from the REFERENCE's own code (build container only).

``ModelWrapper.optimizer_step`` (/root/reference/src/model/model_wrapper.py:1113-1151) is cut out of the reference's file
with ``ast`` at run time and executed, unmodified, against a stand-in ``self`` that has ``named_parameters``,
``parameters``, ``log`` and ``encoder.backbone.cfg.name``; the optimizer it steps is built by evaluating
``configure_optimizers``' own ``torch.optim.AdamW(...)`` call (:1091) on parameter groups sorted as that method sorts
them, and for the Adam scenario ``test_step_align``'s ``torch.optim.Adam(opt_params)`` call (:561).  Everything runs on
the CPU, once in float64 and once in float32, over the three steps of every scenario of tests/optim_oracle.py with the
learning rates changing from step to step.  None of the reference's text is written anywhere.

Recorded: the shared seeded inputs (parameters, three steps of base gradients) in full; per scenario and dtype the
parameters and both moments after the third step at the elements ``optim_oracle.sample_index`` keeps, every tensor's
step count, and per step what the hook logged (``max_gradient``, the NaN / large flags and the offender's name).
Writes tests/golden/optim_goldens.pt.
    python tests/golden/make_optim_goldens.py
"""
import ast
import contextlib
import io
import sys
import types
from pathlib import Path

import torch

REF = Path("/root/reference/src/model/model_wrapper.py")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from tests import optim_oracle as O  # noqa: E402


def _function(tree, name):
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            return node
    raise KeyError(name)


def _method(tree, name, namespace):
    """The function `name` cut out of the reference's class, compiled against `namespace`."""
    exec(compile(ast.Module(body=[_function(tree, name)], type_ignores=[]), str(REF), "exec"), namespace)
    return namespace[name]


def _constructor_call(tree, function, attr):
    """The ``torch.optim.<attr>(...)`` call inside `function`, as a compiled expression."""
    for node in ast.walk(_function(tree, function)):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == attr:
            return compile(ast.fix_missing_locations(ast.Expression(body=node)), str(REF), "eval")
    raise KeyError((function, attr))


class StandIn:
    def __init__(self, params, backbone_name):
        self._named = list(zip(O.NAMES, params))
        self.encoder = types.SimpleNamespace(backbone=types.SimpleNamespace(cfg=types.SimpleNamespace(name=backbone_name)))
        self.optimizer_cfg = types.SimpleNamespace(lr=O.LR, backbone_lr_multiplier=O.BACKBONE_LR_MULTIPLIER)
        self.logged = {}

    def named_parameters(self):
        return iter(self._named)

    def parameters(self):
        return (p for _, p in self._named)

    def log(self, key, value, **kwargs):
        self.logged[key] = value


def run_reference(tree, hook, name, base, dtype):
    sc = O.SCENARIOS[name]
    params = [torch.nn.Parameter(p.to(dtype).clone()) for p in base["params"]]
    stand_in = StandIn(params, "vggt_large" if sc["threshold"] == 20 else "croco")
    if sc.get("adam"):
        opt_params = [{"params": params, "lr": O.ADAM["lr"]}]
        optimizer = eval(_constructor_call(tree, "test_step_align", "Adam"), {"torch": torch, "opt_params": opt_params})
    else:
        new, pre = O.groups_of_names()                                  # configure_optimizers' sorting, :1070-1090
        param_dicts = [{"params": [params[t] for t in new], "lr": stand_in.optimizer_cfg.lr},
                       {"params": [params[t] for t in pre],
                        "lr": stand_in.optimizer_cfg.lr * stand_in.optimizer_cfg.backbone_lr_multiplier}]
        optimizer = eval(_constructor_call(tree, "configure_optimizers", "AdamW"),
                         {"torch": torch, "param_dicts": param_dicts, "self": stand_in})
    base_lrs = [g["lr"] for g in optimizer.param_groups]
    logs = []
    for s, gs in enumerate(O.scenario_grads(base, name)):
        for g, lr in zip(optimizer.param_groups, base_lrs):
            g["lr"] = lr * O.LR_FACTORS[s]

        def closure():
            for p, g in zip(params, gs):
                p.grad = None if g is None else g.to(dtype).clone()

        stand_in.logged = {}
        if sc.get("adam"):                                              # test_step_align: backward, then step (:565-588)
            optimizer.zero_grad()
            closure()
            optimizer.step()
            logs.append(dict(skipped=False, nan_detected=False, large_detected=False, offender=None, max_gradient=0.0))
            continue
        with contextlib.redirect_stdout(io.StringIO()):
            hook(stand_in, 0, s, optimizer, closure)
        large = [k for k in stand_in.logged if k.startswith("large_gradient_detected in ")]
        nan = "nan_gradient_detected" in stand_in.logged
        logs.append(dict(skipped=bool(nan or large), nan_detected=nan, large_detected=bool(large),
                         offender=large[0][len("large_gradient_detected in "):] if large else None,
                         max_gradient=float(stand_in.logged["max_gradient"])))
        assert all(p.grad is None for p in params), "the hook leaves no gradient behind"
    pick = [O.sample_index(p.numel()) for p in params]
    zero = [torch.zeros_like(p) for p in params]
    state = [optimizer.state.get(p, {}) for p in params]
    return {"p": [p.detach().view(-1)[i].clone() for p, i in zip(params, pick)],
            "m": [st.get("exp_avg", z).view(-1)[i].clone() for st, z, i in zip(state, zero, pick)],
            "v": [st.get("exp_avg_sq", z).view(-1)[i].clone() for st, z, i in zip(state, zero, pick)],
            "step": [int(st.get("step", 0)) for st in state], "logs": logs}


def main():
    tree = ast.parse(REF.read_text())
    hook = _method(tree, "optimizer_step", {"torch": torch})
    base = O.base_inputs()
    out = {"base": base, "scenarios": {}}
    for name in O.SCENARIOS:
        out["scenarios"][name] = {"float64": run_reference(tree, hook, name, base, torch.float64),
                                  "float32": run_reference(tree, hook, name, base, torch.float32)}
        r = out["scenarios"][name]["float32"]
        print(f"{name:24s} steps {r['step']} " + " | ".join(
            f"{'skip' if lg['skipped'] else 'step'} max {lg['max_gradient']:.6g} {lg['offender'] or ''}" for lg in r["logs"]))
    path = HERE / "optim_goldens.pt"
    torch.save(out, path)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
