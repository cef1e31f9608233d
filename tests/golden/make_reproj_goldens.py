"""Golden vectors for the reprojection loss from the REFERENCE's own ``LossReproj`` (build container only).

/root/reference/src/loss/{loss,loss_reproj}.py and src/misc/cam_utils.py are imported under a synthetic ``src.*``
package tree; their import-only dependencies (jaxtyping annotations, cv2, pytorch3d.transforms, dataset / decoder /
Gaussians types) get empty stand-in modules -- ``LossReproj.forward`` and ``project_to_cam`` run unmodified, on the CPU
in float32.  Records loss and all three gradients per case.  Writes tests/golden/reproj_goldens.pt.
    python tests/golden/make_reproj_goldens.py
"""
import importlib.util
import sys
import types
import warnings
from pathlib import Path

import torch

REF = Path("/root/reference/src")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from tests.reproj_oracle import controlled_points  # noqa: E402


class _Ann:
    def __class_getitem__(cls, item):
        return cls


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference_reproj():
    _module("jaxtyping", Float=type("Float", (_Ann,), {}))
    _module("cv2")
    _module("pytorch3d")
    sys.modules["pytorch3d"].transforms = _module("pytorch3d.transforms")
    for p in ("src", "src.loss", "src.misc", "src.dataset", "src.model", "src.model.decoder"):
        _module(p)
    _module("src.dataset.types", BatchedExample=dict)
    _module("src.model.decoder.decoder", DecoderOutput=object)
    _module("src.model.types", Gaussians=object)
    for pkg, name in (("misc", "cam_utils"), ("loss", "loss"), ("loss", "loss_reproj")):
        spec = importlib.util.spec_from_file_location(f"src.{pkg}.{name}", REF / pkg / f"{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"src.{pkg}.{name}"] = m
        spec.loader.exec_module(m)
    return sys.modules["src.loss.loss_reproj"]


TOTAL = 200_001
CASES = {
    # name: (b, h, w, kind, mode, weight, step, circle, detach)
    "tanh_mixed": (2, 17, 13, "mixed", "tanh", 1.0, 0, True, False),
    # points behind the camera and at the depth clamp, in image 0 only (their gradients are ~1e6 the others')
    "dyntanh_depth_edges": (2, 17, 13, "depth_edges", "dyntanh", 0.001, 100_000, True, False),
    "l1sqrt_depth_edges": (2, 17, 13, "depth_edges", "l1+sqrt", 0.5, 0, True, False),
    "dyntanh_step0_circle": (2, 17, 13, "mixed", "dyntanh", 0.001, 0, True, False),
    "dyntanh_mid_circle": (2, 17, 13, "mixed", "dyntanh", 0.001, 100_000, True, False),
    "dyntanh_mid_linear": (2, 17, 13, "mixed", "dyntanh", 0.001, 100_000, False, False),
    "dyntanh_total_circle": (2, 17, 13, "mixed", "dyntanh", 0.001, TOTAL, True, False),
    "dyntanh_past_circle": (1, 8, 12, "mixed", "dyntanh", 0.001, 250_000, True, False),    # lw = NaN -> NaN
    "dyntanh_past_linear": (1, 8, 12, "mixed", "dyntanh", 0.001, 250_000, False, False),   # lw < 0, finite
    "l1_mixed": (2, 17, 13, "mixed", "l1", 0.5, 0, True, False),
    "l1sqrt_mixed": (2, 17, 13, "mixed", "l1+sqrt", 0.5, 0, True, False),
    "l1logl1_mixed": (2, 17, 13, "mixed", "l1+logl1", 0.5, 0, True, False),
    "other_string_mixed": (1, 12, 9, "mixed", "huber", 0.5, 0, True, False),              # the reference's `else`
    "dyntanh_detach": (2, 17, 13, "mixed", "dyntanh", 0.001, 50_000, True, True),
    "dyntanh_small_24x32": (2, 24, 32, "small", "dyntanh", 1.0, 20_000, True, False),
    "none_valid": (2, 9, 7, "none_valid", "dyntanh", 0.001, 10, True, False),
    "weight0": (1, 17, 13, "mixed", "dyntanh", 0.0, 10, True, False),
}


def main():
    ref = load_reference_reproj()
    gen = torch.Generator().manual_seed(23)
    out = {}
    for name, (b, h, w, kind, mode, weight, step, circle, detach) in CASES.items():
        pts, poses, ks = controlled_points(gen, b, h, w, kind)
        cfg = ref.LossReprojCfg(weight=weight, mode=mode, circle_schedule=circle, total_iterations=TOTAL)
        m = ref.LossReproj(ref.LossReprojCfgWrapper(reproj=cfg))
        assert m.name == "reproj"
        p = pts.clone().requires_grad_(True)
        po = poses.clone().requires_grad_(True)
        k = ks.clone().requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)       # np.sqrt of a negative past total_iterations
            loss = m(p, po, k, step, detach_pts3d=detach)
        if isinstance(loss, torch.Tensor):
            gp, gpo, gk = torch.autograd.grad(loss, [p, po, k], allow_unused=True)
            loss_t = loss.detach()
        else:                                                     # no valid point: the reference returns the int 0
            assert loss == 0
            gp = gpo = gk = None
            loss_t = torch.tensor(0.0)
        z = lambda g, x: torch.zeros_like(x) if g is None else g  # noqa: E731
        out[name] = {"pts3d": pts, "poses": poses, "intrinsics": ks, "mode": mode, "weight": weight,
                     "global_step": step, "total_iterations": TOTAL, "circle_schedule": circle, "detach_pts3d": detach,
                     "loss": loss_t, "loss_is_int": not isinstance(loss, torch.Tensor),
                     "grad_pts3d": z(gp, pts), "grad_poses": z(gpo, poses), "grad_intrinsics": z(gk, ks)}
        print(f"{name:24s} loss {float(loss_t):.8g}")
    torch.save(out, HERE / "reproj_goldens.pt")
    print("wrote", HERE / "reproj_goldens.pt", (HERE / "reproj_goldens.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
