"""The footprint scatter of the lists kernels (csrc/render.hip, `scatter_box`): the straight-line body for boxes of at
most 4 x 4 against the loops, on rounds that are full, one entry short, and a few entries into the next one.

Every case is one hand-built scene: 300 - 700 rotated Gaussians (axes 1 : 0.8 : 0.6) in front of an identity camera
(plus a second, shifted view), each placed by its pixel centre and the radius of its cull disc, so that tile (0, 0) of
the first view holds

  * a 1 x 1 box, a box of exactly 4 x 4, a 5 x 4 and a 4 x 5 one (one lane over the limit sends its wave to the loops),
    one that fills the tile, and four whose centre lies outside the tile and whose box is clipped at the tile's left,
    right, top and bottom edge;
  * a list of a chosen length: 255 / 256 / 257 and 256 + 63 / + 64 / + 65 (the forward's remainder round ends inside
    its first wave, on its edge, in the second wave), and 400 (the backward, at most 192 entries a round, runs three).

`_tile_model` restates what decides a tile list and a box (3-sigma rect, cull-disc box: csrc/project.hip, spf_common.h)
on the float64 oracle's projection; the test asserts the boxes and the length on it, and the model itself against the
pair count and the longest list the product reports.  Then, per case: colour, depth, alpha and every gradient are
bit-identical between SPF_SCATTER_STRAIGHT unset and =0 (the lists form has no float atomics), for the instantiations
the headline step runs (256 entries a forward round, 192 a backward one) and for the ones a call of few tiles gets;
and the product passes the suite's ordinary gates against the float64 oracle (seeds: the oracle flags no more than
`max_fragile_frac` of the pixels, checked without a GPU)."""
import math

import pytest
import torch

from spfsplatv2_amd import synthetic as syn
from tests import util

pytestmark = pytest.mark.gpu

TILE = 16
FAR_AWAY = 1000000000          # SPF_DENSE_AREA: no tile takes the rows form
Z0, DZ = 2.0, 0.004            # depths: distinct in float32, list order is not index order

# (image (h, w), Gaussians, entries in tile (0, 0) of view 0, seed)
CASES = [((16, 16), 300, 255, 11), ((16, 16), 300, 256, 12), ((16, 16), 300, 257, 13),
         ((24, 40), 500, 256 + 63, 14), ((17, 33), 450, 256 + 64, 15), ((48, 48), 700, 256 + 65, 16),
         ((48, 48), 700, 400, 17)]

# the placed footprints: (pixel centre x, y, cull-disc radius in pixels or None = as small as the low-pass allows, opacity)
SPECIALS = {
    "1x1": (5.0, 5.0, None, 0.0095),
    "4x4": (9.5, 4.5, 1.8, 0.6),
    "5x4": (4.0, 10.5, 2.2, 0.6),
    "4x5": (11.5, 11.0, 2.2, 0.6),
    "16x16": (7.5, 7.5, 13.0, 0.3),
    "left": (-1.6, 7.5, 1.9, 0.6),
    "right": (16.6, 7.5, 1.9, 0.6),
    "top": (7.5, -1.6, 1.9, 0.6),
    "bottom": (7.5, 16.6, 1.9, 0.6),
}
BIG = ("5x4", "4x5", "16x16")  # these go to the back of the list, next to each other


AXES = torch.tensor([1.0, 0.8, 0.6], dtype=torch.float64)      # axis ratios: a rotation changes the picture


def _gaussian(u, v, z, rb, opac, quat, hw):
    """Mean and scales s * AXES of a Gaussian of rotation `quat` that the identity camera sees at pixel (u, v), depth z,
    with a cull disc of radius rb: lambda_max(cov2D) = s^2 lambda_max(J R AXES^2 R^T J^T) + 0.3 and
    rb^2 = 2 ln(255 opacity) lambda_max."""
    from oracle import splat_ref
    h, w = hw
    fx, fy = syn.FX * w, syn.FX * h
    x, y = (u - 0.5 * w + 0.5) * z / fx, (v - 0.5 * h + 0.5) * z / fy
    if rb is None:
        return (x, y, z), (1e-6 * z * AXES).tolist()
    J = torch.tensor([[fx / z, 0.0, -fx * x / (z * z)], [0.0, fy / z, -fy * y / (z * z)]], dtype=torch.float64)
    M = J @ splat_ref.quat_to_rotmat(quat.to(torch.float64)) * AXES
    lam = float(torch.linalg.eigvalsh(M @ M.T)[-1])
    need = rb * rb / (2.0 * math.log(255.0 * opac)) - 0.3
    assert need > 0, (rb, opac)
    return (x, y, z), (math.sqrt(need / lam) * AXES).tolist()


def _build(hw, G, length, seed):
    h, w = hw
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda n=1: torch.rand(n, generator=gen).tolist()
    n_in = length - len(SPECIALS)                        # fillers strictly inside tile (0, 0)
    spots = []                                           # (u, v, rb, opacity)
    for _ in range(n_in):
        a, b, c, d = rnd(4)
        opac = 0.05 + 0.85 * d
        lo = 1.03 * math.sqrt(0.3 * 2.0 * math.log(255.0 * opac))
        spots.append((2.0 + 11.0 * a, 2.0 + 11.0 * b, lo + (1.9 - lo) * c, opac))
    while len(spots) < G - len(SPECIALS):                # the rest: other tiles, or off the image where there are none
        a, b, c, d = rnd(4)
        opac = 0.05 + 0.85 * d
        lo = 1.03 * math.sqrt(0.3 * 2.0 * math.log(255.0 * opac))
        u, v = a * (w - 1), b * (h - 1)
        if w == TILE and h == TILE:
            u, v = -300.0 - 20.0 * a, -300.0 - 20.0 * b
        elif u < 19.0 and v < 19.0:
            continue
        spots.append((u, v, lo + (1.9 - lo) * c, opac))
    order = torch.randperm(len(spots) + len(SPECIALS) - len(BIG), generator=gen).tolist()
    names = [None] * len(spots) + [n for n in SPECIALS if n not in BIG]
    spots += [SPECIALS[n] for n in SPECIALS if n not in BIG]
    depth = [Z0 + DZ * r for r in order]
    for i, n in enumerate(BIG):                          # behind everything else, adjacent in every list
        names.append(n)
        spots.append(SPECIALS[n])
        depth.append(Z0 + DZ * (len(order) + 10 + i))
    n = len(spots)
    assert n == G
    rot = torch.randn(n, 4, generator=gen)
    rot = (rot / rot.norm(dim=-1, keepdim=True))[None]
    means, scales = [], []
    for (u, v, rb, opac), z, q in zip(spots, depth, rot[0]):
        m, s = _gaussian(u, v, z, rb, opac, q, hw)
        means.append(m)
        scales.append(s)
    ext = torch.eye(4).repeat(1, 2, 1, 1)
    ext[0, 1, :3, 3] = torch.tensor([0.05, -0.03, 0.0])  # view 1: the same scene a fraction of a pixel to the side
    batch = syn.Batch(means=torch.tensor(means, dtype=torch.float32)[None], scales=torch.tensor(scales, dtype=torch.float32)[None],
                      rotations=rot, opacities=torch.tensor([s[3] for s in spots], dtype=torch.float32)[None],
                      harmonics=torch.randn(1, n, 3, 1, generator=gen), covariances=torch.zeros(1, n, 3, 3), extrinsics=ext,
                      intrinsics=syn.intrinsics(2).reshape(1, 2, 3, 3), near=torch.full((1, 2), 0.1),
                      far=torch.full((1, 2), 100.0), image_shape=hw, target=torch.rand(1, 2, 3, h, w, generator=gen))
    return batch, names


def _tile_model(batch):
    """Per view: {(tx, ty): [(Gaussian, gx, gy, xl, yl, bw, bh), ...]}: the tile lists (3-sigma rect shrunk to the tiles
    that hold a pixel of the cull disc's box) and each entry's box clipped to its tile, from the float64 projection."""
    from oracle import glue_ref, splat_ref
    h, w = batch.image_shape
    b, v = batch.extrinsics.shape[:2]
    rep = lambda t: t[:, None].expand(b, v, *t.shape[1:]).reshape(b * v, *t.shape[1:])
    args = glue_ref.callsite_args(batch.extrinsics.reshape(b * v, 4, 4), batch.intrinsics.reshape(b * v, 3, 3),
                                  batch.near.reshape(-1), batch.far.reshape(-1), batch.image_shape,
                                  torch.zeros(b * v, 3), rep(batch.means), rep(batch.harmonics), rep(batch.opacities),
                                  rep(batch.rotations), rep(batch.scales))
    tiles_x, tiles_y = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    views = []
    for a in args:
        c = lambda t: None if t is None else t.to(torch.float64)
        pr = splat_ref.project(c(a["means3D"]), c(a["scales"]), c(a["rotations"]), c(a["opacities"]), c(a["shs"]), None,
                               c(a["viewmatrix"]), c(a["projmatrix"]), a["tanfovx"], a["tanfovy"], h, w, a["sh_degree"])
        A, B, C = pr.conic.unbind(-1)
        mu = 0.5 * (A + C) - torch.sqrt(0.25 * (A - C) ** 2 + B * B)
        thr = 2.0 * torch.log(255.0 * pr.opacity)
        r2 = torch.where(255.0 * pr.opacity > 1.0, (thr * 1.001 + 1e-3) / mu * 1.001, torch.full_like(mu, -1.0))
        rb = torch.sqrt(r2.clamp(min=0.0)) * 1.0001 + 1e-3
        gx, gy = pr.xy.unbind(-1)
        xlo, xhi, ylo, yhi = torch.ceil(gx - rb), torch.floor(gx + rb), torch.ceil(gy - rb), torch.floor(gy + rb)
        lists = {}
        for g in torch.nonzero((pr.radii > 0) & (r2 >= 0)).flatten().tolist():
            x0 = max(int(pr.rect_min[g, 0]), min(tiles_x, max(0, math.floor(float(xlo[g]) / TILE))))
            y0 = max(int(pr.rect_min[g, 1]), min(tiles_y, max(0, math.floor(float(ylo[g]) / TILE))))
            x1 = min(int(pr.rect_max[g, 0]), min(tiles_x, max(0, math.floor(float(xhi[g]) / TILE) + 1)))
            y1 = min(int(pr.rect_max[g, 1]), min(tiles_y, max(0, math.floor(float(yhi[g]) / TILE) + 1)))
            for ty in range(y0, y1):
                for tx in range(x0, x1):
                    X0, Y0 = tx * TILE, ty * TILE
                    xl, yl = int(max(float(xlo[g]) - X0, 0.0)), int(max(float(ylo[g]) - Y0, 0.0))
                    bw = max(0, int(min(float(xhi[g]) - X0, TILE - 1.0)) - xl + 1)
                    bh = max(0, int(min(float(yhi[g]) - Y0, TILE - 1.0)) - yl + 1)
                    lists.setdefault((tx, ty), []).append((g, float(gx[g]), float(gy[g]), xl, yl, bw, bh))
        views.append(lists)
    return views


def _check_scene(batch, names, length):
    """The scene holds what the case is about (no GPU needed)."""
    views = _tile_model(batch)
    tile = views[0][(0, 0)]
    assert len(tile) == length, (len(tile), length)
    box = {names[g]: (gx, gy, xl, yl, bw, bh) for g, gx, gy, xl, yl, bw, bh in tile if names[g]}
    assert set(box) == set(SPECIALS), sorted(box)
    for n, want in (("1x1", (1, 1)), ("4x4", (4, 4)), ("5x4", (5, 4)), ("4x5", (4, 5)), ("16x16", (16, 16))):
        assert box[n][4:] == want, (n, box[n])
    gx, gy, xl, yl, bw, bh = box["left"]
    assert gx < -0.5 and xl == 0 and 1 <= bw <= 4 and 1 <= bh <= 4, box["left"]
    gx, gy, xl, yl, bw, bh = box["right"]
    assert gx > TILE - 0.5 and xl + bw == TILE and 1 <= bw <= 4 and 1 <= bh <= 4, box["right"]
    gx, gy, xl, yl, bw, bh = box["top"]
    assert gy < -0.5 and yl == 0 and 1 <= bh <= 4 and 1 <= bw <= 4, box["top"]
    gx, gy, xl, yl, bw, bh = box["bottom"]
    assert gy > TILE - 0.5 and yl + bh == TILE and 1 <= bh <= 4 and 1 <= bw <= 4, box["bottom"]
    small = sum(1 for e in tile if e[5] <= 4 and e[6] <= 4)
    assert small >= length - len(BIG) - 1, (small, length)           # the straight body is what most waves take
    counts = [len(l) for v in views for l in v.values()]
    return sum(counts), max(counts)


@pytest.mark.parametrize("hw,G,length,seed", CASES, ids=[f"{h}x{w}-{n}" for (h, w), _, n, _ in CASES])
def test_straight_scatter_equals_the_loops_and_the_oracle(hip_lib, monkeypatch, hw, G, length, seed):
    batch, names = _build(hw, G, length, seed)
    pairs, longest = _check_scene(batch, names, length)
    assert longest == length
    ref = util.run_oracle(batch, torch.float64, mask_fragile=True)
    monkeypatch.setenv("SPF_DENSE_AREA", str(FAR_AWAY))
    monkeypatch.setenv("SPF_DENSE_AREA_FWD", str(FAR_AWAY))
    runs = {}
    for shapes in ("headline", "few-tiles"):
        if shapes == "headline":                         # 256 entries a forward round, 192 a backward round
            monkeypatch.setenv("SPF_FWD_STAGE", "256")
            monkeypatch.setenv("SPF_BWD_ROUNDS", "192")
        else:                                            # what a call of this few tiles gets: 512 and 256
            monkeypatch.delenv("SPF_FWD_STAGE")
            monkeypatch.delenv("SPF_BWD_ROUNDS")
        for straight in ("unset", "0"):
            if straight == "0":
                monkeypatch.setenv("SPF_SCATTER_STRAIGHT", "0")
            else:
                monkeypatch.delenv("SPF_SCATTER_STRAIGHT", raising=False)
            runs[shapes, straight] = util.run_product(batch, pixel_mask=ref["pixel_mask"])
        monkeypatch.delenv("SPF_SCATTER_STRAIGHT", raising=False)
    first = runs["headline", "unset"]
    assert first["stats"]["dense_tiles"] == 0
    assert (first["stats"]["num_pairs"], first["stats"]["max_tile_list"]) == (pairs, longest), first["stats"]
    for key, r in runs.items():
        for k in ("color", "depth", "alpha"):
            assert torch.equal(r[k], first[k]), (key, k)
        for n in util.GRAD_NAMES:
            assert torch.equal(r["grads"][n], first["grads"][n]), (key, n)
    rep = util.compare(first, ref)
    print("lists scatter", hw, length, {k: v for k, v in rep.items() if k != "fails"})
    assert not rep["fails"], rep
