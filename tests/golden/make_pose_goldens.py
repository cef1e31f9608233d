"""Golden vectors for the pose path from the REFERENCE's own code (build container only).

/root/reference/src/misc/{cam_utils,intrinsics_utils}.py, src/evaluation/metrics.py and
src/model/encoder/backbone/vggt/utils/{rotation,geometry}.py are loaded by path under stand-in modules (jaxtyping, cv2,
lpips, skimage get empty ones), and run unmodified on the CPU in float32.  ``pytorch3d`` is not installed here: its
``rotation_6d_to_matrix`` is tests/pose_oracle.py's restatement of the published 6-D map, injected as
``pytorch3d.transforms`` -- so for that one function the goldens pin the oracle to itself, and everything around it to the
reference.  ``process_pose`` is a method of the encoder classes, which cannot be imported without the whole model: its
source is cut out of encoder_spfsplatv2.py / encoder_spfsplatv2l.py and executed against a stand-in ``self.cfg``.  For
the VGGT variant the extrinsics ``[R(q) | T]`` are assembled as ``pose_encoding_to_extri_intri`` does, from the
reference's ``quat_to_mat``.

Every case records its inputs, the reference's float32 outputs and its autograd gradients for a seeded upstream.
Writes tests/golden/pose_goldens.pt.
    python tests/golden/make_pose_goldens.py
"""
import ast
import contextlib
import importlib.util
import io
import sys
import types
from pathlib import Path

import torch

REF = Path("/root/reference/src")
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parents[1]))

from tests import pose_oracle as O  # noqa: E402


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


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def _method(path: Path, name: str, namespace: dict):
    """The function `name` cut out of the class in `path`, compiled against `namespace`."""
    src = path.read_text()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.FunctionDef) and node.name == name:
            mod = ast.Module(body=[node], type_ignores=[])
            exec(compile(mod, str(path), "exec"), namespace)
            return namespace[name]
    raise KeyError(name)


def load_reference():
    _module("jaxtyping", Float=type("Float", (_Ann,), {}))
    _module("cv2")
    _module("lpips", LPIPS=object)
    _module("skimage")
    _module("skimage.metrics", structural_similarity=None)
    _module("pytorch3d")
    sys.modules["pytorch3d"].transforms = _module("pytorch3d.transforms", rotation_6d_to_matrix=O.rotation_6d_to_matrix)
    cam = _load("ref_cam_utils", REF / "misc" / "cam_utils.py")
    intr = _load("ref_intrinsics_utils", REF / "misc" / "intrinsics_utils.py")
    met = _load("ref_metrics", REF / "evaluation" / "metrics.py")
    vggt = REF / "model" / "encoder" / "backbone" / "vggt" / "utils"
    rot = _load("ref_rotation", vggt / "rotation.py")
    geo = _load("ref_geometry", vggt / "geometry.py")
    from einops import rearrange
    enc = REF / "model" / "encoder"
    pp6 = _method(enc / "encoder_spfsplatv2.py", "process_pose",
                  {"torch": torch, "rearrange": rearrange, "convert_pose_to_4x4": cam.convert_pose_to_4x4})
    ppq = _method(enc / "encoder_spfsplatv2l.py", "process_pose",
                  {"torch": torch, "rearrange": rearrange, "closed_form_inverse_se3": geo.closed_form_inverse_se3})
    return cam, intr, met, rot, pp6, ppq


COMPOSE = {   # name: (encoding, b, v, context_views, baseline, relative)
    "rot6d_both": ("rot6d", 2, 3, 2, True, True),
    "rot6d_baseline_last": ("rot6d", 3, 4, 4, True, False),
    "rot6d_relative_cv1": ("rot6d", 2, 2, 1, False, True),
    "rot6d_plain": ("rot6d", 1, 2, 2, False, False),
    "rot6d_12_views": ("rot6d", 2, 12, 2, True, True),
    "quat_both": ("absT_quaR_FoV", 2, 3, 2, True, True),
    "quat_baseline_last": ("absT_quaR_FoV", 3, 4, 4, True, False),
    "quat_relative_cv1": ("absT_quaR_FoV", 2, 2, 1, False, True),
    "quat_plain": ("absT_quaR_FoV", 1, 2, 2, False, False),
}
DEPTH = {"two_small": (2, 300), "three_odd": (3, 1551)}
FOCAL = {"24x32": (24, 32, 21.0), "33x47": (33, 47, 40.0), "64x64": (64, 64, 55.0)}


def main():
    cam, intr, met, rot, pp6, ppq = load_reference()
    gen = torch.Generator().manual_seed(31)
    out = {"compose": {}, "depth": {}, "errors": {}, "focal": {}}

    for name, (encoding, b, v, cv, bl, rel) in COMPOSE.items():
        enc = O.make_enc(gen, b, v, cv, encoding)
        e = enc.clone().requires_grad_(True)
        stand_in = types.SimpleNamespace(cfg=types.SimpleNamespace(pose_make_baseline_1=bl, pose_make_relative=rel))
        if encoding == "rot6d":
            poses = pp6(stand_in, e, cv)
        else:
            extri = torch.cat([rot.quat_to_mat(e[..., 3:7]), e[..., :3, None]], dim=-1)
            poses = ppq(stand_in, extri, cv)
        G = torch.randn(b, v, 4, 4, generator=gen)
        (ge,) = torch.autograd.grad((poses * G).sum(), e)
        assert poses.dtype == torch.float32
        out["compose"][name] = {"enc": enc, "encoding": encoding, "context_views": cv, "baseline": bl, "relative": rel,
                                "poses": poses.detach(), "upstream": G, "grad_enc": ge}
        print(f"compose {name:22s} |poses| {float(poses.abs().max()):.4g} |grad| {float(ge.abs().max()):.4g}")

    conv_in = O.make_enc(gen, 5, 1, 1, "rot6d")[:, 0]
    out["compose"]["convert_pose_to_4x4"] = {"out": conv_in, "poses": cam.convert_pose_to_4x4(conv_in)}

    for name, (N, n) in DEPTH.items():
        poses = O.process_pose(O.make_enc(gen, N, 1, 1, "rot6d").double(), 1, pose_make_baseline_1=False,
                               pose_make_relative=False)[:, 0].float()
        pts = (torch.randn(N, n, 3, generator=gen) * 2 + torch.tensor([0.0, 0.0, 6.0]))
        p, q = pts.clone().requires_grad_(True), poses.clone().requires_grad_(True)
        depth = cam.depth_projector(p, q)
        G = torch.randn(N, n, 1, generator=gen)
        gp, gq = torch.autograd.grad((depth * G).sum(), [p, q])
        out["depth"][name] = {"pts3d": pts, "poses": poses, "depth": depth.detach(), "upstream": G, "grad_pts3d": gp,
                              "grad_poses": gq}
        print(f"depth {name:12s} |z| {float(depth.abs().max()):.4g}")

    pred, tgt = O.make_pose_pairs(gen, 40)
    per_pose = torch.stack([torch.stack(met.compute_pose_error(tgt[i], pred[i])) for i in range(40)])
    ang, trans = met.compute_pose_error_for_batch(pred.reshape(8, 5, 4, 4), tgt.reshape(8, 5, 4, 4))
    ang1, trans1 = met.compute_pose_error_for_batch(pred[3], tgt[3])
    out["errors"]["parity"] = {"pred": pred, "tgt": tgt, "per_pose": per_pose, "batch_8x5": torch.stack([ang, trans]),
                               "single_3": torch.stack([ang1, trans1])}
    ep, et = O.pose_error_edges()
    out["errors"]["edges"] = {"pred": ep, "tgt": et,
                              "per_pose": torch.stack([torch.stack(met.compute_pose_error(et[i], ep[i]))
                                                       for i in range(3)])}
    print("errors edges (reference, float32):", out["errors"]["edges"]["per_pose"].tolist())
    errs = per_pose[:, 2].numpy()
    thresholds = [5, 10, 20, 90]
    out["errors"]["auc"] = {"errors": torch.from_numpy(errs.copy()), "thresholds": thresholds,
                            "auc": cam.pose_auc(errs, thresholds)}

    with contextlib.redirect_stdout(io.StringIO()):          # the reference prints when it falls back to focal_base
        for name, (h, w, f) in FOCAL.items():
            pts = torch.stack([O.focal_scene(gen, h, w, f), O.focal_scene(gen, h, w, 0.7 * f)])
            focal = torch.cat([intr.estimate_focal_knowing_depth(pts[i][None]) for i in range(2)])
            out["focal"][name] = {"pts3d": pts, "focal": focal}
        pts = out["focal"]["24x32"]["pts3d"]
        pp = torch.tensor([14.5, 13.0])
        out["focal"]["24x32_pp"] = {"pts3d": pts, "pp": pp,
                                    "focal": torch.cat([intr.estimate_focal_knowing_depth(pts[i][None], pp=pp)
                                                        for i in range(2)])}
        views = torch.stack([pts, torch.randn(2, 24, 32, 3, generator=gen)], dim=1)       # view 1 must not matter
        out["focal"]["intrinsics_24x32"] = {"pts3d": views, "height": 24, "width": 32,
                                            "intrinsics": intr.estimate_intrinsics(views, 24, 32)}
        for name, (pts, want) in O.focal_edges().items():
            out["focal"]["edge_" + name] = {"pts3d": pts, "focal": intr.estimate_focal_knowing_depth(pts),
                                            "expected": want}
    for name, c in out["focal"].items():
        print(f"focal {name:24s}", (c["focal"] if "focal" in c else c["intrinsics"][:, 0]).flatten().tolist())

    path = HERE / "pose_goldens.pt"
    torch.save(out, path)
    print("wrote", path, path.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
