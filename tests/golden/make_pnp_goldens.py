"""Writes tests/golden/pnp_goldens.pt: the planted PnP scenes of tests/pnp_cases.py with the float64 and float32 results of
tests/pnp_oracle.py (pose, inliers, candidates, hypothesis, success) and the sample ranks.  Reference-free.

    python tests/golden/make_pnp_goldens.py

Fails if the oracle alone does not meet what the tests rely on: every scene is unambiguous (pnp_cases.check_unambiguous:
nothing between 4 and 6 px, the inliers are the planted ones), the noise-free scene with float64 points is recovered to
1e-9, and the noisy ones within twice pnp_cases.PLANTED_ERROR."""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
from tests import pnp_cases as Cs  # noqa: E402
from tests import pnp_oracle as O  # noqa: E402

FIELDS = ("inliers", "candidates", "hypothesis", "success")


def results(views, **solve):
    """Stacked oracle results of a list of views for both precisions, and the float64 run's full dictionaries."""
    out, full = {}, []
    for tag, dtype in (("f64", np.float64), ("f32", np.float32)):
        rs = [O.solve_view(v["pts"], v["opacity"], v["K"], *v["pts"].shape[:2], dtype=dtype, **solve) for v in views]
        out[tag] = {"pose": torch.from_numpy(np.stack([r["pose"] for r in rs]))}
        for f in FIELDS:
            out[tag][f] = torch.tensor([r[f] for r in rs], dtype=torch.int32)
        if dtype is np.float64:
            full = rs
            out["ranks"] = torch.from_numpy(np.stack([r["ranks"] for r in rs]).astype(np.int32))
    return out, full


def pack(views):
    return {"pts": torch.from_numpy(np.stack([v["pts"] for v in views])),
            "opacity": torch.from_numpy(np.stack([v["opacity"] for v in views])),
            "K": torch.from_numpy(np.stack([v["K"] for v in views])),
            "planted_pose": torch.from_numpy(np.stack([v["pose"] for v in views]))}


def main():
    gold = {"single": {}}
    for name, (h, w, kw, solve) in Cs.SINGLE.items():
        view = Cs.planted_view(h, w, **kw)
        res, full = results([view], **solve)
        Cs.check_unambiguous(view, full[0])
        assert res["f32"]["inliers"].equal(res["f64"]["inliers"]) and int(res["f32"]["success"][0]) == 1, name
        ang, dt = Cs.pose_errors(full[0]["pose"], view)
        lim = Cs.PLANTED_ERROR[name]
        assert ang <= 2 * lim[0] and dt <= 2 * lim[1], (name, ang, dt)
        e32 = float(np.abs(res["f32"]["pose"].numpy() - full[0]["pose"]).max() / np.abs(full[0]["pose"]).max())
        print(f"{name}: inliers {full[0]['inliers']} of {full[0]['candidates']}, hypothesis {full[0]['hypothesis']}, "
              f"planted error {ang:.3e} rad {dt:.3e}, float32 oracle err {e32:.2e}")
        entry = pack([view])
        entry.update(res)
        entry["solve"] = dict(solve)
        gold["single"][name] = {k: (v[0] if isinstance(v, torch.Tensor) else v) for k, v in entry.items() if k not in ("f64", "f32")}
        for tag in ("f64", "f32"):
            gold["single"][name][tag] = {k: v[0] for k, v in res[tag].items()}
    exact = Cs.planted_view(24, 32, **{**Cs.SINGLE["clean_24x32"][2], "dtype": np.float64})
    r = O.solve_view(exact["pts"], exact["opacity"], exact["K"], 24, 32)
    assert np.abs(r["pose"] - exact["pose"]).max() <= 1e-9, "the noise-free scene is not recovered to 1e-9"
    b, v, h, w = Cs.BATCH_SHAPE
    views = [x for row in Cs.batch_views() for x in row]
    res, full = results(views)
    for view, rr in zip(views, full):
        if rr["success"]:
            Cs.check_unambiguous(view, rr)
    assert res["f64"]["success"].tolist() == [1, 0, 1, 0, 1, 1] and res["f64"]["candidates"][1] == 3
    assert res["f32"]["inliers"].equal(res["f64"]["inliers"])
    entry = pack(views)
    entry.update({k: val for k, val in res.items() if k == "ranks"})
    gold["batch"] = {k: val.reshape(b, v, *val.shape[1:]) for k, val in entry.items()}
    for tag in ("f64", "f32"):
        gold["batch"][tag] = {k: val.reshape(b, v, *val.shape[1:]) for k, val in res[tag].items()}
    out = Path(__file__).parent / "pnp_goldens.pt"
    torch.save(gold, out)
    print("wrote", out, out.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
