"""The definition of the PnP solver in numpy: what csrc/pnp.hip computes, stage by stage.

``dtype`` is the precision of the bulk arithmetic -- the pixel-space camera, the scores and the per-point residuals,
Jacobians and their sums: ``numpy.float64`` is the truth the tests measure against, ``numpy.float32`` the yardstick that
shows what single precision loses.  The stages the definition places in float64 (the P3P, the 6 x 6 solve, the pose
update, the closed-form inverse) are float64 for both.  Integer stages (hash, ranks, counts) are exact.
"""
from __future__ import annotations

import math

import numpy as np

ITERATIONS, REPROJECTION_ERROR, REFINE_STEPS, SEED, REDRAWS = 128, 5.0, 10, 0, 8
M32 = 0xFFFFFFFF


def mix32(x: int) -> int:
    """lowbias32 (Chris Wellons, hash-prospector)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def hash3(seed: int, k: int, draw: int) -> int:
    return mix32(mix32(mix32((seed + 0x9E3779B9) & M32) ^ k) ^ draw)


def rank_of(h: int, n: int) -> int:
    return (h * n) >> 32                      # mulhi32


def sample_ranks(n: int, iterations: int = ITERATIONS, seed: int = SEED):
    """[iterations, 4] ranks (-1: not drawn) and [iterations] 'the sample is complete'."""
    ranks = -np.ones((iterations, 4), dtype=np.int64)
    ok = np.zeros(iterations, dtype=bool)
    if n < 4:
        return ranks, ok
    for k in range(iterations):
        draw = redraws = 0
        good = True
        for j in range(4):
            while True:
                r = rank_of(hash3(seed, k, draw), n)
                draw += 1
                if r not in ranks[k, :j]:
                    ranks[k, j] = r
                    break
                redraws += 1
                if redraws > REDRAWS:
                    good = False
                    break
            if not good:
                break
        ok[k] = good
    return ranks, ok


def candidate_mask(pts, opacity, threshold):
    """Row-major flat mask: opacity > threshold (in float32, as the kernels compare) and finite coordinates."""
    p = np.asarray(pts, dtype=np.float32).reshape(-1, 3)
    o = np.asarray(opacity, dtype=np.float32).reshape(-1)
    with np.errstate(invalid="ignore"):
        return (o > np.float32(threshold)) & np.isfinite(p).all(axis=1)


def quartic_roots(A4, A3, A2, A1, A0):
    """Real roots by Ferrari's resolvent cubic, two Newton steps each (the order is part of the definition)."""
    if not abs(A4) > 1e-14 * (abs(A3) + abs(A2) + abs(A1) + abs(A0)):
        return []
    a, b, c, d = A3 / A4, A2 / A4, A1 / A4, A0 / A4
    a2 = a * a
    p = b - 0.375 * a2
    q = c - 0.5 * a * b + 0.125 * a2 * a
    r = d - 0.25 * a * c + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2
    c2, c1, c0 = p, 0.25 * p * p - r, -0.125 * q * q
    P = c1 - c2 * c2 / 3.0
    Q = 2.0 * c2 * c2 * c2 / 27.0 - c2 * c1 / 3.0 + c0
    disc = 0.25 * Q * Q + P * P * P / 27.0
    if disc > 0.0:
        sd = math.sqrt(disc)
        t = float(np.cbrt(-0.5 * Q + sd) + np.cbrt(-0.5 * Q - sd))
    else:
        rho = math.sqrt(max(-P / 3.0, 0.0))
        den = rho * rho * rho
        arg = min(max(-0.5 * Q / den, -1.0), 1.0) if den > 0.0 else 1.0
        t = 2.0 * rho * math.cos(math.acos(arg) / 3.0)
    m = t - c2 / 3.0
    for _ in range(2):
        f = ((m + c2) * m + c1) * m + c0
        fp = (3.0 * m + 2.0 * c2) * m + c1
        if fp != 0.0:
            m -= f / fp
    y = []
    if not m > 1e-14 * (abs(p) + abs(r) + 1.0):
        D = p * p - 4.0 * r
        if D >= 0.0:
            sD = math.sqrt(D)
            for z in (0.5 * (-p + sD), 0.5 * (-p - sD)):
                if z >= 0.0:
                    y += [math.sqrt(z), -math.sqrt(z)]
    else:
        s = math.sqrt(2.0 * m)
        h, e = 0.5 * p + m, q / (2.0 * s)
        D1, D2 = s * s - 4.0 * (h + e), s * s - 4.0 * (h - e)
        if D1 >= 0.0:
            y += [0.5 * (s + math.sqrt(D1)), 0.5 * (s - math.sqrt(D1))]
        if D2 >= 0.0:
            y += [0.5 * (-s + math.sqrt(D2)), 0.5 * (-s - math.sqrt(D2))]
    out = []
    for v in y:
        v -= 0.25 * a
        for _ in range(2):
            f = (((v + a) * v + b) * v + c) * v + d
            fp = ((4.0 * v + 3.0 * a) * v + 2.0 * b) * v + c
            if fp != 0.0:
                v -= f / fp
        out.append(v)
    return out


def camera_px(K, H, W, dtype=np.float64):
    """(fx, sk, cx, fy, cy) in pixels from the normalised float32 K: row 0 times W, row 1 times H."""
    K = np.asarray(K, dtype=np.float32).astype(dtype)
    return (K[0, 0] * dtype(W), K[0, 1] * dtype(W), K[0, 2] * dtype(W), K[1, 1] * dtype(H), K[1, 2] * dtype(H))


def _frame(A, B, C):
    e1 = (B - A) / np.linalg.norm(B - A)
    e3 = np.cross(e1, C - A)
    e3 = e3 / np.linalg.norm(e3)
    return np.stack([e1, np.cross(e3, e1), e3])


def polish_depths(s1, s2, s3, cosines, sides2, steps=2):
    """Newton steps on the three distance equations |s_i f_i - s_j f_j|^2 = d_ij^2 (Cramer's rule): u comes out of a
    division that loses digits where its denominator is small, the depths are then consistent to ~1e-8 only."""
    ca, cb, cg = cosines
    a2, b2, c2 = sides2
    for _ in range(steps):
        F0 = s1 * s1 + s2 * s2 - 2 * s1 * s2 * cg - c2
        F1 = s1 * s1 + s3 * s3 - 2 * s1 * s3 * cb - b2
        F2 = s2 * s2 + s3 * s3 - 2 * s2 * s3 * ca - a2
        j00, j01 = 2 * (s1 - s2 * cg), 2 * (s2 - s1 * cg)
        j10, j12 = 2 * (s1 - s3 * cb), 2 * (s3 - s1 * cb)
        j21, j22 = 2 * (s2 - s3 * ca), 2 * (s3 - s2 * ca)
        det = -j00 * j12 * j21 - j01 * j10 * j22
        if not abs(det) > 0:
            break
        d1 = (F0 * j12 * j21 + j01 * (F1 * j22 - j12 * F2)) / det
        d2 = (-j00 * (j22 * F1 - j12 * F2) + F0 * j10 * j22) / det
        d3 = (j00 * j21 * F1 + j01 * j10 * F2 - F0 * j10 * j21) / det
        s1, s2, s3 = s1 + d1, s2 + d2, s3 + d3
    return s1, s2, s3


def p3p_all(cam, Pw, px):
    """Every admissible root of Grunert's quartic for three points as (R, t), world -> camera, float64."""
    fx, sk, cx, fy, cy = (float(c) for c in cam)
    Pw, px = np.asarray(Pw, dtype=np.float64), np.asarray(px, dtype=np.float64)
    Y = (px[:3, 1] - cy) / fy
    X = (px[:3, 0] - cx - sk * Y) / fx
    f = np.stack([X, Y, np.ones(3)], 1)
    f /= np.linalg.norm(f, axis=1, keepdims=True)
    a2 = float(np.sum((Pw[1] - Pw[2]) ** 2))
    b2 = float(np.sum((Pw[0] - Pw[2]) ** 2))
    c2 = float(np.sum((Pw[0] - Pw[1]) ** 2))
    if not (a2 > 0 and b2 > 0 and c2 > 0):
        return []
    ca, cb, cg = float(f[1] @ f[2]), float(f[0] @ f[2]), float(f[0] @ f[1])
    q, p, cr, ar = (a2 - c2) / b2, (a2 + c2) / b2, c2 / b2, a2 / b2
    A4 = (q - 1) ** 2 - 4 * cr * ca * ca
    A3 = 4 * (q * (1 - q) * cb - (1 - p) * ca * cg + 2 * cr * ca * ca * cb)
    A2 = 2 * (q * q - 1 + 2 * q * q * cb * cb + 2 * (1 - cr) * ca * ca - 4 * p * ca * cb * cg + 2 * (1 - ar) * cg * cg)
    A1 = 4 * (-q * (1 + q) * cb + 2 * ar * cg * cg * cb - (1 - p) * ca * cg)
    A0 = (1 + q) ** 2 - 4 * ar * cg * cg
    with np.errstate(all="ignore"):
        fw = _frame(Pw[0], Pw[1], Pw[2])
        out = []
        for v in quartic_roots(A4, A3, A2, A1, A0):
            if not v > 0:
                continue
            den = 2 * (cg - v * ca)
            if not abs(den) > 1e-12:
                continue
            u = ((q - 1) * v * v - 2 * q * cb * v + 1 + q) / den
            if not u > 0:
                continue
            dd = 1 + u * u - 2 * u * cg
            if not dd > 0:
                continue
            s1 = math.sqrt(c2 / dd)
            s1, s2, s3 = polish_depths(s1, u * s1, v * s1, (ca, cb, cg), (a2, b2, c2))
            if not (s1 > 0 and s2 > 0 and s3 > 0):
                continue
            Xc = np.stack([s1 * f[0], s2 * f[1], s3 * f[2]])
            fc = _frame(Xc[0], Xc[1], Xc[2])
            R = fc.T @ fw
            out.append((R, Xc[0] - R @ Pw[0]))
    return out


def project(cam, R, t, P):
    """(u, v, z) of world points under the world -> camera pose, in the dtype of the arguments."""
    fx, sk, cx, fy, cy = cam
    Xc = P @ R.T + t
    with np.errstate(all="ignore"):
        iz = 1 / Xc[:, 2]
        return (fx * Xc[:, 0] + sk * Xc[:, 1]) * iz + cx, fy * Xc[:, 1] * iz + cy, Xc


def p3p(cam, Pw, px):
    """The root whose reprojection of the fourth point is nearest and in front of the camera, or None."""
    best, pick = math.inf, None
    Pw, px = np.asarray(Pw, dtype=np.float64), np.asarray(px, dtype=np.float64)
    cam = tuple(float(c) for c in cam)
    for R, t in p3p_all(cam, Pw, px):
        u, v, Xc = project(cam, R, t, Pw[3:4])
        if not Xc[0, 2] > 0:
            continue
        e2 = float((u[0] - px[3, 0]) ** 2 + (v[0] - px[3, 1]) ** 2)
        if e2 < best:
            best, pick = e2, (R, t)
    return pick


def rodrigues(w):
    th2 = float(w @ w)
    th = math.sqrt(th2)
    Kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.float64)
    A, B = (math.sin(th) / th, (1 - math.cos(th)) / th2) if th >= 1e-12 else (1.0, 0.0)
    return np.eye(3) + A * Kx + B * (Kx @ Kx)


def orthonormal_rows(R):
    """Gram-Schmidt on the rows (float64): the stored float32 hypothesis is a rotation only to 6e-8."""
    r0 = R[0] / np.linalg.norm(R[0])
    r1 = R[1] - (R[1] @ r0) * r0
    r1 = r1 / np.linalg.norm(r1)
    return np.stack([r0, r1, np.cross(r0, r1)])


def inliers_of(cam, R, t, P, xy, thr2, dtype):
    u, v, Xc = project(cam, R.astype(dtype), t.astype(dtype), P)
    ru, rv = u - xy[:, 0], v - xy[:, 1]
    with np.errstate(invalid="ignore"):
        return (Xc[:, 2] > 0) & (ru * ru + rv * rv < thr2), ru, rv, Xc


def solve_view(pts, opacity, K, H, W, opacity_threshold=0.3, iterations=ITERATIONS,
               reprojection_error=REPROJECTION_ERROR, refine_steps=REFINE_STEPS, seed=SEED, dtype=np.float64):
    """One view.  Returns dict(pose [4, 4] float64 before the float32 store, inliers, candidates, hypothesis, success,
    ranks [iterations, 4], inlier_mask over the candidates, pixels of the candidates)."""
    pts = np.asarray(pts)                              # float64 points are taken as they are (the planted-truth tests)
    pts = pts if pts.dtype == np.float64 else pts.astype(np.float32)
    h, w = pts.shape[:2]
    assert (h, w) == (H, W)
    mask = candidate_mask(pts, opacity, opacity_threshold)
    idx = np.flatnonzero(mask)
    n = len(idx)
    fail = dict(pose=np.eye(4), inliers=0, candidates=n, hypothesis=-1, success=0)
    ranks, drawn = sample_ranks(n, iterations, seed)
    fail["ranks"] = ranks
    if n < 4:
        return fail
    P32 = pts.reshape(-1, 3)[idx]
    xy64 = np.stack([idx % w, idx // w], 1).astype(np.float64)
    P, xy = P32.astype(dtype), xy64.astype(dtype)
    cam64, cam = camera_px(K, H, W, np.float64), camera_px(K, H, W, dtype)
    thr2 = dtype(reprojection_error) * dtype(reprojection_error)
    best, kbest, pose = 0, -1, None
    for k in range(iterations):
        if not drawn[k]:
            continue
        hyp = p3p(cam64, P32[ranks[k]].astype(np.float64), xy64[ranks[k]])
        if hyp is None:
            continue
        R, t = (x.astype(np.float32).astype(np.float64) for x in hyp)      # hypotheses are stored as float32
        if not np.isfinite(R).all() or not np.isfinite(t).all():
            continue
        cnt = int(inliers_of(cam, R, t, P, xy, thr2, dtype)[0].sum())
        if cnt > best:
            best, kbest, pose = cnt, k, (R, t)
    if best < 4:
        return fail
    R, t = orthonormal_rows(pose[0]), pose[1]
    fx, sk, cx, fy, cy = cam
    for step in range(refine_steps + 1):
        m, ru, rv, Xc = inliers_of(cam, R, t, P, xy, thr2, dtype)
        cnt = int(m.sum())
        if cnt < 4:
            return fail
        if step == refine_steps:
            break
        X, Y, Z, ru, rv = Xc[m, 0], Xc[m, 1], Xc[m, 2], ru[m], rv[m]
        iz = 1 / Z
        du = np.stack([fx * iz, sk * iz, -(fx * X + sk * Y) * iz * iz], 1)
        dv = np.stack([0 * iz, fy * iz, -fy * Y * iz * iz], 1)
        Xm = np.stack([X, Y, Z], 1)
        ju = np.concatenate([np.cross(Xm, du), du], 1)
        jv = np.concatenate([np.cross(Xm, dv), dv], 1)
        JJ = (ju.T @ ju + jv.T @ jv).astype(np.float64)
        Jr = (ju.T @ ru + jv.T @ rv).astype(np.float64)
        try:
            d = np.linalg.solve(JJ + 1e-9 * np.trace(JJ) * np.eye(6), -Jr)
        except np.linalg.LinAlgError:
            return fail
        if not np.isfinite(d).all():
            return fail
        E = rodrigues(d[:3])
        R, t = E @ R, E @ t + d[3:]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -R.T @ t
    return dict(pose=out, inliers=cnt, candidates=n, hypothesis=kbest, success=1, ranks=ranks, inlier_mask=m, pixels=idx,
                errors=np.sqrt((ru * ru + rv * rv).astype(np.float64)))
