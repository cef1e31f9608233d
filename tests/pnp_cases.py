"""Planted scenes for the PnP solver: a known camera, a point map that projects onto its own pixel grid, pixel noise and
GROSS outliers built in the image, so that the inlier set is unambiguous.

* camera: normalised ``fx = fy = 0.889``, principal point at the centre (synthetic.py's);
* pose (world -> camera): a random rotation of <= 0.3 rad and a translation of N(0, 0.5);
* depths: log-uniform in [1, 20], or a tilted plane;
* pixel noise: N(0, ``noise``) per axis, clipped at 2 px -- the point lies on the ray of the displaced pixel;
* outliers: the point lies on the ray of ANOTHER image position 20..60 px away, at a random depth, so under the true
  pose its reprojection error is >= 20 px and it cannot land inside the 5 px band.

``check_unambiguous`` is what the golden generator asserts for every case: under the float64 oracle's final pose no
candidate lies between 4 and 6 px, and the oracle's inliers are exactly the planted ones.
"""
from __future__ import annotations

import numpy as np

from tests import pnp_oracle as O

FOCAL = 0.889


def intrinsics():
    return np.array([[FOCAL, 0, 0.5], [0, FOCAL, 0.5], [0, 0, 1]], dtype=np.float32)


def planted_view(h, w, seed, outliers=0.0, noise=0.0, planar=False, opacity="all", dtype=np.float32):
    """dict(pts [h, w, 3], opacity [h, w], K [3, 3] normalised, R, t (world -> camera, float64), pose (camera -> world
    [4, 4] float64), planted [h w] bool: candidate and no outlier)."""
    rng = np.random.default_rng(seed)
    K = intrinsics()
    fx, sk, cx, fy, cy = O.camera_px(K, h, w)
    axis = rng.normal(size=3)
    R = O.rodrigues(axis / np.linalg.norm(axis) * rng.uniform(0.05, 0.3))
    t = rng.normal(size=3) * 0.5
    ys, xs = np.mgrid[:h, :w]
    xy = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    n = h * w
    nz = np.clip(rng.normal(size=(n, 2)) * noise, -2.0, 2.0)
    is_out = rng.random(n) < outliers
    ang, far = rng.uniform(0, 2 * np.pi, n), rng.uniform(20.0, 60.0, n)
    shift = np.where(is_out[:, None], np.stack([np.cos(ang), np.sin(ang)], 1) * far[:, None], nz)
    seen = xy + shift
    rays = np.stack([(seen[:, 0] - cx) / fx, (seen[:, 1] - cy) / fy, np.ones(n)], 1)
    if planar:
        z = 4.0 / (rays @ np.array([0.2, -0.1, 1.0]))
        z = np.where(is_out, np.exp(rng.uniform(0, np.log(20.0), n)), z)
    else:
        z = np.exp(rng.uniform(0, np.log(20.0), n))
    Xc = rays * z[:, None]
    P = (Xc - t) @ R                                   # X = R P + t  <=>  P = R^T (X - t)
    if opacity == "all":
        on = np.ones(n, dtype=bool)
    elif opacity == "pattern":                         # rows of 64: full words, checkers and empty words
        on = np.where(ys % 4 == 0, True, np.where(ys % 4 == 3, False, (xs + ys) % 2 == 0)).ravel()
    else:
        raise ValueError(opacity)
    opa = np.where(on, rng.uniform(0.5, 1.0, n), rng.uniform(0.0, 0.25, n))
    pose = np.eye(4)
    pose[:3, :3], pose[:3, 3] = R.T, -R.T @ t
    return dict(pts=P.reshape(h, w, 3).astype(dtype), opacity=opa.reshape(h, w).astype(np.float32), K=K, R=R, t=t,
                pose=pose, planted=on & ~is_out)


def check_unambiguous(view, result):
    """The generator's conditions on a float64 oracle result of a planted view."""
    assert result["success"] == 1, "the oracle failed on a planted scene"
    e = result["errors"]
    assert not ((e > 4.0) & (e < 6.0)).any(), f"a candidate lies {e[(e > 4.0) & (e < 6.0)]} px from its pixel"
    got = np.zeros(view["planted"].shape, dtype=bool)
    got[result["pixels"][result["inlier_mask"]]] = True
    assert (got == view["planted"]).all(), "the oracle's inliers are not the planted ones"


def pose_errors(pose, view):
    """(rotation angle in rad, |translation difference|) of a camera -> world pose against the planted one."""
    dR = pose[:3, :3].T @ view["pose"][:3, :3]
    skew = 0.5 * np.array([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    ang = float(np.arcsin(min(np.linalg.norm(skew), 1.0)))          # small angles: exact where arccos(trace) is not
    return ang, float(np.linalg.norm(pose[:3, 3] - view["pose"][:3, 3]))


# name -> (h, w, keyword arguments of planted_view, keyword arguments of the solve)
SINGLE = {
    "clean_24x32": (24, 32, dict(seed=11), {}),
    "tail_20x15": (20, 15, dict(seed=12, outliers=0.4, noise=0.5), {}),
    "pattern_64x64": (64, 64, dict(seed=13, outliers=0.3, noise=0.5, opacity="pattern"), {}),
    "planar_48x64": (48, 64, dict(seed=14, outliers=0.3, noise=0.5, planar=True), {}),
    "groups_72x72_it64": (72, 72, dict(seed=15, outliers=0.3, noise=0.5), dict(iterations=64)),
    "groups_72x72_it1024": (72, 72, dict(seed=15, outliers=0.3, noise=0.5), dict(iterations=1024)),
}
BATCH_SHAPE = (2, 3, 24, 32)


def batch_views():
    """Six views with different poses; (0, 1) keeps 3 candidates, (1, 0) none, (0, 2) has NaN points in a corner whose
    opacity is on."""
    b, v, h, w = BATCH_SHAPE
    views = [[planted_view(h, w, seed=100 + 3 * i + j, outliers=0.3, noise=0.5) for j in range(v)] for i in range(b)]
    few = views[0][1]
    keep = np.zeros(h * w, dtype=bool)
    keep[[5, 300, 700]] = True
    few["opacity"] = np.where(keep.reshape(h, w), few["opacity"], 0.1).astype(np.float32)
    few["planted"] &= keep
    views[1][0]["opacity"] = np.full((h, w), 0.2, dtype=np.float32)
    views[1][0]["planted"][:] = False
    nan = views[0][2]
    nan["pts"][:4, :4] = np.nan
    nan["opacity"][:4, :4] = 0.9
    corner = np.zeros((h, w), dtype=bool)
    corner[:4, :4] = True
    nan["planted"] &= ~corner.ravel()
    return views


# What the float64 oracle's final pose is from the planted one on the fixtures above, (rotation in rad, translation):
# the estimator's own scatter under 0.5 px noise.  The tests allow twice this -- the same estimator on another seed
# scatters that much -- and 1e-9 for the noise-free scene built from float64 points.
PLANTED_ERROR = {
    "clean_24x32": (4.9e-10, 3.7e-9),        # no noise: what rounding the points to float32 costs
    "tail_20x15": (6.2e-3, 3.1e-2),
    "pattern_64x64": (9.3e-4, 2.2e-3),
    "planar_48x64": (3.3e-3, 1.7e-2),
    "groups_72x72_it64": (2.4e-4, 7.4e-4),
    "groups_72x72_it1024": (2.4e-4, 7.4e-4),
}
