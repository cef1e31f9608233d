"""Golden vectors for SSIM from the REFERENCE's own ``ssim`` (build container only).

/root/reference/src/loss/loss_ssim.py is imported by path (it needs torch alone) and ``ssim`` runs unmodified on the CPU,
once in float64 and once in float32, on small seeded cases.  Per case the file holds the inputs (float32: exact in both
runs), the settings, the float64 value and gradients, and the float32 run's own error against the float64 run (value,
per plane, per element: tests/ssim_oracle.py::grad_errors) -- the yardstick of the GPU tests.  With
``size_average=False`` the upstream gradient is linspace(0.5, 1.5, N).  Writes tests/golden/ssim_goldens.pt.
    python tests/golden/make_ssim_goldens.py
"""
import importlib.util
import sys
from pathlib import Path

import torch

REF = Path("/root/reference/src/loss/loss_ssim.py")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from tests import ssim_oracle as so  # noqa: E402


def load_reference_ssim():
    spec = importlib.util.spec_from_file_location("ref_loss_ssim", REF)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _negative_plane(seed, shape):
    """smooth inputs whose plane [0, 0] is anticorrelated (Y = 1 - X there): that plane's SSIM is far below 0."""
    X, Y = so.smooth(seed, shape)
    Y[0, 0] = 1 - X[0, 0]
    return X, Y


def _scaled(kind, scale):
    return lambda seed, shape: tuple(t * scale for t in so.KINDS[kind](seed, shape))


CUSTOM_WIN = torch.tensor([0.05, 0.15, 0.4, 0.25, 0.15])       # not symmetric: the filter's direction shows
CASES = {
    # name: (shape, inputs, kwargs)
    "noise_dr1": ((2, 3, 19, 23), so.noise, dict(data_range=1.0)),
    "smooth_dr255_per_image": ((2, 3, 19, 23), _scaled("smooth", 255.0), dict(data_range=255, size_average=False)),
    "piecewise_c4_per_image": ((2, 4, 19, 23), so.piecewise, dict(data_range=1.0, size_average=False)),
    "nonnegative_c1": ((2, 1, 19, 23), _negative_plane, dict(data_range=1.0, nonnegative_ssim=True)),
    "nonnegative_per_image": ((2, 3, 19, 23), _negative_plane,
                              dict(data_range=1.0, nonnegative_ssim=True, size_average=False)),
    "win7_smooth": ((2, 3, 19, 23), so.smooth, dict(data_range=1.0, win_size=7)),
    "custom_win_c1": ((2, 1, 19, 23), so.noise, dict(data_range=1.0, win=CUSTOM_WIN, size_average=False)),
    "smooth_37x53_per_image": ((2, 3, 37, 53), so.smooth, dict(data_range=1.0, size_average=False)),
    "noise_11x11": ((1, 3, 11, 11), so.noise, dict(data_range=1.0)),
    "piecewise_11x300": ((1, 3, 11, 300), so.piecewise, dict(data_range=1.0)),
}


def run(ref, X, Y, kwargs, dtype, upstream):
    x = X.clone().to(dtype).requires_grad_(True)
    y = Y.clone().to(dtype).requires_grad_(True)
    kw = dict(kwargs)
    if "win" in kw:                                           # the reference's layout: one row per channel
        kw["win"] = kw["win"].reshape(1, 1, 1, -1).repeat(X.shape[1], 1, 1, 1)
    value = ref.ssim(x, y, **kw)[0]
    gx, gy = torch.autograd.grad(value, [x, y], None if upstream is None else upstream.to(dtype))
    return value.detach(), gx, gy


def main():
    ref = load_reference_ssim()
    out = {}
    for i, (name, (shape, make, kwargs)) in enumerate(CASES.items()):
        X, Y = (t.float().contiguous() for t in make(100 + i, shape))
        upstream = None if kwargs.get("size_average", True) else torch.linspace(0.5, 1.5, shape[0], dtype=torch.float64)
        v64, gx64, gy64 = run(ref, X, Y, kwargs, torch.float64, upstream)
        v32, gx32, gy32 = run(ref, X, Y, kwargs, torch.float32, upstream)
        if kwargs.get("nonnegative_ssim"):
            w = kwargs.get("win")
            planes = so.ssim_planes(X.double(), Y.double(),
                                    (so.gauss_window(kwargs.get("win_size", 11), 1.5) if w is None else w).double(),
                                    (0.01 * kwargs["data_range"]) ** 2, (0.03 * kwargs["data_range"]) ** 2)
            assert float(planes.abs().min()) > 1e-3, (name, planes)        # the relu's kink decides nothing
            assert bool((planes < 0).any()) and bool((planes > 0).any()), (name, planes)
        ex, ey = so.grad_errors(gx32, gx64), so.grad_errors(gy32, gy64)
        err = {"value": so.value_error(v32, v64), "plane": max(ex[0], ey[0]), "element": max(ex[1], ey[1])}
        out[name] = {"X": X, "Y": Y, "kwargs": kwargs, "upstream": upstream, "value": v64, "grad_X": gx64,
                     "grad_Y": gy64, "f32_error": err}
        print(f"{name:26s} value {v64.flatten().tolist()}  f32 error: value {err['value']:.3g} plane {err['plane']:.3g} "
              f"element {err['element']:.3g}")
    path = HERE / "ssim_goldens.pt"
    torch.save(out, path)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
