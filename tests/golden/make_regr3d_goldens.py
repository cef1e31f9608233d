"""Golden vectors for the distillation point loss from the REFERENCE's own ``Regr3D`` (build container only).

/root/reference/src/loss/loss_point.py, src/geometry/ptc_geometry.py and src/model/encoder/backbone/croco/misc.py are
imported under a synthetic ``src.*`` package tree (scipy's cKDTree, an import-only dependency, gets a stand-in when
scipy is missing) -- ``Regr3D.forward`` and ``normalize_pointcloud`` run unmodified, on the CPU in float32.  Records the
loss, both gradients and the valid counts (the masks the reference hands to normalize_pointcloud).  Tiny cases keep
their inputs; the larger ones only their seed (tests/regr3d_oracle.make_case rebuilds them) and scalars.
Writes tests/golden/regr3d_goldens.pt.
    python tests/golden/make_regr3d_goldens.py
"""
import importlib.util
import sys
import types
from pathlib import Path

import torch

REF = Path("/root/reference/src")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from tests import regr3d_oracle as go  # noqa: E402


def _module(name, **attrs):
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference_regr3d():
    try:
        import scipy.spatial  # noqa: F401
    except ImportError:
        _module("scipy")
        sys.modules["scipy"].spatial = _module("scipy.spatial", cKDTree=object)
    for p in ("src", "src.loss", "src.geometry", "src.model", "src.model.encoder", "src.model.encoder.backbone",
              "src.model.encoder.backbone.croco"):
        _module(p)
    for name, rel in (("src.model.encoder.backbone.croco.misc", "model/encoder/backbone/croco/misc.py"),
                      ("src.geometry.ptc_geometry", "geometry/ptc_geometry.py"),
                      ("src.loss.loss_point", "loss/loss_point.py")):
        spec = importlib.util.spec_from_file_location(name, REF / rel)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
    return sys.modules["src.loss.loss_point"]


def _tiny(seed, B, H, W, **opts):
    return go.make_case(seed, B, H, W, **opts)


def _conf1_all_low():
    c = _tiny(106, 2, 17, 13)
    c["conf1"] = c["conf1"].clamp(max=2.5)
    return c


def _row_none_valid():
    c = _tiny(107, 3, 17, 13)
    c["conf1"][1] = 1.0
    c["conf2"][1] = 2.0
    return c


def _identical_gt_row():
    c = _tiny(108, 2, 17, 13)
    c["gt_pts1"][0] = torch.tensor([0.25, -0.5, 3.0])
    c["conf1"][0] = 5.0
    return c


PICK = [(0, 2, 3), (0, 9, 11), (1, 16, 0), (1, 5, 5)]


def _pr_scaled_gt():
    """pr == gt * s (1 + 1e-4) on a few points, s the ratio of the two norm factors (a fixed point, iterated in float64):
    the normalised prediction misses its target by 1e-4 of its length there, so d ~ 0 and float32 carries its direction
    to ~1e-3 only -- but it HAS a direction.  (With d at rounding level, |d| ~ 1e-7 |a|, the direction is noise in any
    precision, and through nf_pr that noise moves every gradient of the row by k / n_valid for k such points: nothing a
    test could hold anybody to.  d == 0 exactly is the next case.)"""
    c = _tiny(109, 2, 17, 13)
    for key in ("conf1", "conf2"):
        for b, i, j in PICK:
            c[key][b, i, j] = 6.0
    for _ in range(6):
        ref = go.run_ref(c)
        s = (ref["nf_pr"] / ref["nf_gt"]).float()
        for v in (1, 2):
            for b, i, j in PICK:
                c[f"pr_pts{v}"][b, i, j] = c[f"gt_pts{v}"][b, i, j] * (s[b] * (1 + 1e-4))
    return c


def _pr_equals_gt():
    """No normalisation (norm_mode None, which the constructor takes) and pr == gt on a few valid points: d == 0 exactly,
    where |x| passes no gradient."""
    c = _tiny(110, 2, 17, 13, norm_mode=None)
    for key in ("conf1", "conf2"):
        for b, i, j in PICK:
            c[key][b, i, j] = 6.0
    for v in (1, 2):
        for b, i, j in PICK:
            c[f"pr_pts{v}"][b, i, j] = c[f"gt_pts{v}"][b, i, j]
    return c


CASES = {
    # name: (builder, keep the inputs)
    "default_2x17x13": (lambda: _tiny(101, 2, 17, 13), True),
    "integer_ranks_3x3x167": (lambda: _tiny(102, 3, 3, 167), True),            # n = 501: both ranks are integers
    "dist_clip_8": (lambda: _tiny(103, 2, 17, 13, dist_clip=8.0), True),
    "disable_view1": (lambda: _tiny(104, 2, 17, 13, disable_view1=True), True),
    "gt_scale": (lambda: _tiny(105, 2, 17, 13, gt_scale=True), True),
    "conf1_all_low": (_conf1_all_low, True),                                    # NaN loss, finite gradients
    "row_none_valid": (_row_none_valid, True),
    "identical_gt_row": (_identical_gt_row, True),                              # ties keep every point of the row
    "pr_scaled_gt": (_pr_scaled_gt, True),                                      # d ~ 0 on a few points
    "pr_equals_gt_no_norm": (_pr_equals_gt, True),                              # d == 0 on a few points
    "seeded_2x64x64": (lambda: go.first_decided_case(2, 64, 64, start=200), False),
    "seeded_2x96x112": (lambda: go.first_decided_case(2, 96, 112, start=300), False),
}
OPTS = ("seed", "dist_clip", "disable_view1", "norm_mode", "gt_scale")
INPUTS = ("gt_pts1", "gt_pts2", "pr_pts1", "pr_pts2", "conf1", "conf2")


def main():
    ref = load_reference_regr3d()
    seen = {}
    inner = ref.normalize_pointcloud

    def spy(pts1, pts2, norm_mode="avg_dis", valid1=None, valid2=None):
        seen.setdefault("valid", (valid1.clone(), valid2.clone()))
        return inner(pts1, pts2, norm_mode, valid1, valid2)
    ref.normalize_pointcloud = spy
    out = {}
    for name, (build, keep) in CASES.items():
        c = build()
        m = ref.Regr3D(norm_mode=c["norm_mode"], gt_scale=c["gt_scale"])
        p1 = c["pr_pts1"].clone().requires_grad_(True)
        p2 = c["pr_pts2"].clone().requires_grad_(True)
        seen.clear()
        loss = m(c["gt_pts1"], c["gt_pts2"], p1, p2, c["conf1"], c["conf2"], dist_clip=c["dist_clip"],
                 disable_view1=c["disable_view1"])
        g1, g2 = torch.autograd.grad(loss, [p1, p2], allow_unused=True)
        z = lambda g, x: torch.zeros_like(x) if g is None else g  # noqa: E731
        if not c["norm_mode"]:          # the masks do not depend on the normalisation: a second call shows them
            with torch.no_grad():
                ref.Regr3D(gt_scale=c["gt_scale"])(c["gt_pts1"], c["gt_pts2"], p1, p2, c["conf1"], c["conf2"],
                                                   dist_clip=c["dist_clip"], disable_view1=c["disable_view1"])
        v1, v2 = seen["valid"]
        rec = {k: c[k] for k in OPTS}
        rec.update(shape=tuple(c["gt_pts1"].shape[:3]), loss=loss.detach(),
                   n_valid=torch.stack([v1.flatten(1).sum(1), v2.flatten(1).sum(1)]).to(torch.int32))
        if keep:
            rec.update({k: c[k] for k in INPUTS})
            rec.update(grad_pr1=z(g1, p1), grad_pr2=z(g2, p2))
        out[name] = rec
        print(f"{name:24s} loss {float(loss.detach()):.8g}  n_valid {rec['n_valid'].tolist()}")
    torch.save(out, HERE / "regr3d_goldens.pt")
    print("wrote", HERE / "regr3d_goldens.pt", (HERE / "regr3d_goldens.pt").stat().st_size, "bytes")


if __name__ == "__main__":
    main()
