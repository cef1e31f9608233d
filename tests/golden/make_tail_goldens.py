"""Golden vectors of the reference encoder's tail (build container only): its own UnifiedGaussianAdapter.forward and the
body of its map_pdf_to_opacity (encoder_spfsplatv2.py:146-159), run in float32 on the CPU on the tensors its forward
hands them (:218-224, 240, 248-268; the rearranges and the stack are written here with torch's own operations) and taken
to the shape of :296-321.  The adapter's module is loaded as tests/golden/make_adapter_goldens.py loads it, with the same
stubs; the encoder's module imports the whole model, so map_pdf_to_opacity alone is compiled from its source, read at
run time.         python tests/golden/make_tail_goldens.py"""
import ast
import importlib.util
import sys
import types
from pathlib import Path

import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/src")
jt = types.ModuleType("jaxtyping")
class _Ann:
    def __class_getitem__(cls, item): return cls
for n in ("Float", "Int64", "Bool", "Shaped", "Int"): setattr(jt, n, type(n, (_Ann,), {}))
sys.modules["jaxtyping"] = jt
def pkg(name):
    m = types.ModuleType(name); m.__path__ = []; sys.modules[name] = m; return m
for p in ("src", "src.geometry", "src.misc", "src.model", "src.model.encoder", "src.model.encoder.common"): pkg(p)
sh = types.ModuleType("src.misc.sh_rotation"); sh.rotate_sh = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("unused"))
sys.modules["src.misc.sh_rotation"] = sh
def load(name, rel):
    spec = importlib.util.spec_from_file_location(name, REF / rel); m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m; spec.loader.exec_module(m); return m
load("src.geometry.projection", "geometry/projection.py")
load("src.model.encoder.common.gaussians", "model/encoder/common/gaussians.py")
ga = load("src.model.encoder.common.gaussian_adapter", "model/encoder/common/gaussian_adapter.py")


def reference_method(rel: str, name: str):
    """The function ``name`` of the reference file ``rel``, compiled on its own without its annotations."""
    tree = ast.parse((REF / rel).read_text())
    fn = next(n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name)
    fn.returns = None
    for a in fn.args.args:
        a.annotation = None
    mod = ast.fix_missing_locations(ast.Module(body=[fn], type_ignores=[]))
    scope = {}
    exec(compile(mod, str(REF / rel), "exec"), scope)
    return scope[name]


map_pdf_to_opacity = reference_method("model/encoder/encoder_spfsplatv2.py", "map_pdf_to_opacity")

gen = torch.Generator().manual_seed(21)
b, v, h, w = 2, 2, 3, 5
out = {}
for deg in (0, 4):
    for log2_e in (0.0, 1.5):
        ad = ga.UnifiedGaussianAdapter(ga.GaussianAdapterCfg(gaussian_scale_min=0.5, gaussian_scale_max=15.0, sh_degree=deg))
        C = 1 + ad.d_in
        raw = [(torch.randn(b, C, h, w, generator=gen) * 3.0).requires_grad_(True) for _ in range(v)]
        raw[0].data[0, 1:4, 0, 0] = torch.tensor([25.0, -30.0, 6.0])       # softplus linear branch / tiny / ordinary
        raw[0].data[0, 1:4, 0, 1] = 400.0                                    # the clamp at 0.3
        pts = [torch.randn(b, h, w, 3, generator=gen).requires_grad_(True) for _ in range(v)]
        enc = types.SimpleNamespace(cfg=types.SimpleNamespace(
            opacity_mapping=types.SimpleNamespace(initial=log2_e, final=log2_e, warm_up=1), num_surfaces=1))
        # the tensors encoder_spfsplatv2.py:218-224, 240, 248-250, 255-259 hand to the two functions: per view the head
        # output as rows, the views stacked, one surface; probabilities from channel 0, the adapter's channels after it
        rows = torch.stack([r.flatten(2).transpose(1, 2) for r in raw], dim=1).unflatten(-1, (enc.cfg.num_surfaces, C))
        points = torch.stack(pts, dim=1).flatten(2, 3)[..., None, None, :]                     # [b, v, hw, srf, spp, 3]
        pdf = torch.sigmoid(rows[..., :1])                                                     # [b, v, hw, srf, 1]
        g = ad.forward(points, map_pdf_to_opacity(enc, pdf, 0), rows[..., None, 1:])           # (:264-268)
        # :296-321
        res = {"means": g.means.reshape(b, -1, 3), "covariances": g.covariances.reshape(b, -1, 3, 3),
               "rotations": g.rotations.reshape(b, -1, 4), "scales": g.scales.reshape(b, -1, 3),
               "harmonics": g.harmonics.reshape(b, -1, 3, ad.d_sh), "opacities": g.opacities.reshape(b, -1)}
        names = ("means", "opacities", "scales", "rotations", "harmonics")
        ups = {k: torch.randn(res[k].shape, generator=gen) for k in names}
        sum((res[k] * ups[k]).sum() for k in names).backward()
        out[f"deg{deg}_e{log2_e:g}"] = {
            "sh_degree": deg, "exponent": 2.0 ** log2_e, "raw": [r.detach().clone() for r in raw],
            "pts": [p.detach().clone() for p in pts], "out": {k: t.detach().clone() for k, t in res.items()}, "ups": ups,
            "d_raw": torch.stack([r.grad for r in raw]), "d_pts": torch.stack([p.grad for p in pts]),
            "sh_mask": ad.sh_mask.clone()}
torch.save(out, HERE / "tail_goldens.pt")
print("wrote tail_goldens.pt", {k: tuple(x["raw"][0].shape) for k, x in out.items()})
