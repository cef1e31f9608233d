"""Oracle of the camera set-up (TEST INFRASTRUCTURE ONLY): this project's own float64 restatement of what csrc/camera.hip
computes -- the camera preamble of the reference's render_cuda (cuda_splatting.py:66-74, 84-91: the scale-invariant
rescale, ``get_fov`` of projection.py:269-283, ``get_projection_matrix`` of cuda_splatting.py:15-42, the inverse and the
two transposes) and the chain of dL/dviewmatrix back to the poses.  It follows the REFERENCE's chain (``linalg.inv``,
unit rays, ``acos``, ``tan``), not the kernel's algebra (cofactors, tan(theta/2) from |a||b| -+ a.b), on float32 inputs
promoted exactly; the two ill-conditioned parts have a second float64 form each (``tan_half_fov(..., form="atan2")``,
``view_closed_form``) which tests/test_camera.py holds against the first on every test camera.

``mut``: a set of names that turn the oracle into a WRONG one, for the power condition of the gates:
  no_translation_rescale  forward: the translation is not multiplied by 1/near
  far_not_rescaled        forward: far stays as given while near becomes 1
  view_not_transposed     forward: viewmatrix = inverse(extrinsics'), not its transpose
  view64_without_scale    forward: viewmatrix64 = viewmatrix, the world scale not folded in
  fov_from_focal          forward: tan(fov/2) = 0.5/fx, 0.5/fy (right only for a centred principal point and no skew)
  grad_not_transposed     backward: dL/dviewmatrix used untransposed
  grad_no_rescale         backward: the translation column of the result not multiplied by 1/near
  grad_sign               backward: the sign
  partials_last_column    partials: the 12 slots read four per row (three full rows of the 4x4, the last COLUMN filled
                          and the last row empty) where the kernel reads three per row (four rows, the last column
                          empty: slot 3i+j -> [i][j], i < 4, j < 3 -- camera.hip's ``i < 3 ? 3*i+j : 9+j``)

The bounds of the gate (``forward_bounds``, ``grad_bound``) are derived from float32 / float64 rounding -- see each -- and
not from what the product gives.
"""
from __future__ import annotations

import torch

FORWARD_MUTANTS = ("no_translation_rescale", "far_not_rescaled", "view_not_transposed", "view64_without_scale",
                   "fov_from_focal")
GRAD_MUTANTS = ("grad_not_transposed", "grad_no_rescale", "grad_sign")
PARTIAL_MUTANTS = ("partials_last_column",)
MUTANTS = FORWARD_MUTANTS + GRAD_MUTANTS + PARTIAL_MUTANTS
NONE = frozenset()
FORWARD_NAMES = ("viewmatrix", "projmatrix", "tanfov", "view_scale", "viewmatrix64")

U = 2.0 ** -24                   # float32 unit roundoff
TINY = 2.0 ** -36                # what float64 work may cost, relative to a render's largest entry: 16 x TWO_FORMS_INV
TWO_FORMS_INV = 2.0 ** -40       # linalg.inv against [M^-1, -M^-1 t], relative to a render's largest entry
TWO_FORMS_TAN = 1e-9             # tan(acos(.)/2) against tan(atan2(.)/2), relative
GRAD_C = 16.0                    # the gradient bound's factor of u (12 counted roundings and a third on top)


def f64(t: torch.Tensor) -> torch.Tensor:
    """A float32 input promoted exactly."""
    assert t.dtype == torch.float32, t.dtype
    return t.detach().double().cpu()


# ---- forward ---------------------------------------------------------------------------------------------------------
def rescale(ext, near, far, scale_invariant: bool, mut=NONE):
    """cuda_splatting.py:66-74 -> (extrinsics', near', far', scale), float64."""
    scale = 1.0 / near if scale_invariant else torch.ones_like(near)
    ext = ext.clone()
    if "no_translation_rescale" not in mut:
        ext[:, :3, 3] = ext[:, :3, 3] * scale[:, None]
    return ext, near * scale, (far if "far_not_rescaled" in mut else far * scale), scale


def edge_rays(K):
    """The four rays of get_fov, un-normalised: through (0,.5,1) (1,.5,1) (.5,0,1) (.5,1,1) with K^-1."""
    inv = torch.linalg.inv(K)
    pts = torch.tensor([[0.0, 0.5, 1.0], [1.0, 0.5, 1.0], [0.5, 0.0, 1.0], [0.5, 1.0, 1.0]], dtype=K.dtype)
    return torch.einsum("bij,pj->pbi", inv, pts)


def tan_half_fov(K, form: str = "acos", mut=NONE):
    """[R,2] tan(fov_x / 2), tan(fov_y / 2).  ``acos``: the reference's chain (unit rays, acos of their dot product, tan
    of half of it).  ``atan2``: fov = atan2(|a x b|, a.b) of the un-normalised rays, well conditioned at every angle."""
    if "fov_from_focal" in mut:
        return torch.stack((0.5 / K[:, 0, 0], 0.5 / K[:, 1, 1]), dim=-1)
    left, right, top, bottom = edge_rays(K)

    def fov(a, b):
        if form == "acos":
            a, b = a / a.norm(dim=-1, keepdim=True), b / b.norm(dim=-1, keepdim=True)
            return (a * b).sum(dim=-1).acos()
        assert form == "atan2", form
        return torch.atan2(torch.linalg.cross(a, b).norm(dim=-1), (a * b).sum(dim=-1))
    return torch.stack(((0.5 * fov(left, right)).tan(), (0.5 * fov(top, bottom)).tan()), dim=-1)


def projection(near, far, tan):
    """get_projection_matrix (cuda_splatting.py:15-42) with tan = tan(fov / 2) [R,2]; column-vector form, NOT transposed."""
    top, right = tan[:, 1] * near, tan[:, 0] * near
    bottom, left = -top, -right
    out = torch.zeros((near.shape[0], 4, 4), dtype=near.dtype)
    out[:, 0, 0] = 2 * near / (right - left)
    out[:, 1, 1] = 2 * near / (top - bottom)
    out[:, 0, 2] = (right + left) / (right - left)
    out[:, 1, 2] = (top + bottom) / (top - bottom)
    out[:, 3, 2] = 1
    out[:, 2, 2] = far / (far - near)
    out[:, 2, 3] = -(far * near) / (far - near)
    return out


class _Inverse(torch.autograd.Function):
    """torch.linalg.inv with its derivative dA = -B^T dB B^T, and one thing known exactly put in by hand: the inverse of
    a pose (last row 0 0 0 1) has the last row 0 0 0 1.  linalg.inv leaves ~1e-17 there on some matrices, which no
    tolerance relative to the element itself -- the gradient bound is one, and holds exact zeros bitwise -- can absorb."""

    @staticmethod
    def forward(ctx, a):
        b = torch.linalg.inv(a)
        last = torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=a.dtype)
        pose = (a[:, 3] == last).all(dim=-1)
        b[pose, 3] = last
        ctx.save_for_backward(b)
        return b

    @staticmethod
    def backward(ctx, g):
        bt = ctx.saved_tensors[0].transpose(-1, -2)
        return -bt @ g @ bt


def view_of(ext_rescaled, mut=NONE):
    inv = _Inverse.apply(ext_rescaled)
    return inv if "view_not_transposed" in mut else inv.transpose(-1, -2)


def view_closed_form(ext_rescaled):
    """The second form of the inverse: [M t; 0 1]^-1 = [M^-1, -M^-1 t; 0 1], transposed.  (Poses only: last row 0 0 0 1.)"""
    assert bool((ext_rescaled[:, 3] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=ext_rescaled.dtype)).all())
    mi = torch.linalg.inv(ext_rescaled[:, :3, :3])
    inv = torch.zeros_like(ext_rescaled)
    inv[:, :3, :3] = mi
    inv[:, :3, 3] = -(mi @ ext_rescaled[:, :3, 3:])[..., 0]
    inv[:, 3, 3] = 1
    return inv.transpose(-1, -2)


def fold_scale(view, scale, mut=NONE):
    """SpfInputs.viewmatrix64: the view matrix with its first three rows times the world scale."""
    if "view64_without_scale" in mut:
        return view.clone()
    rows = torch.cat((scale[:, None].expand(-1, 3), torch.ones_like(scale)[:, None]), dim=1)
    return view * rows[:, :, None]


def forward(extrinsics, intrinsics, near, far, scale_invariant: bool, mut=NONE) -> dict:
    """{name: float64 tensor} over FORWARD_NAMES for float32 inputs [R,4,4], [R,3,3], [R], [R]."""
    ext, K, near, far = f64(extrinsics), f64(intrinsics), f64(near), f64(far)
    ext, nr, fr, scale = rescale(ext, near, far, bool(scale_invariant), mut)
    view = view_of(ext, mut)
    tan = tan_half_fov(K, "acos", mut)
    return {"viewmatrix": view, "projmatrix": projection(nr, fr, tan).transpose(-1, -2), "tanfov": tan,
            "view_scale": scale, "viewmatrix64": fold_scale(view, scale, mut)}


# ---- pose gradient ---------------------------------------------------------------------------------------------------
def pose_grad(extrinsics, near, scale_invariant: bool, dL_dview, mut=NONE):
    """dL/dextrinsics [R,4,4], float64 autograd through the chain above for the ``viewmatrix`` output only (the contract
    of spf_camera_backward).  ``dL_dview`` float32 or float64."""
    ext = f64(extrinsics).requires_grad_(True)
    nr = f64(near)
    g = dL_dview.detach().double().cpu()
    if "grad_not_transposed" in mut:
        g = g.transpose(-1, -2)
    e2, _, _, scale = rescale(ext, nr, nr, bool(scale_invariant))
    (d,) = torch.autograd.grad((view_of(e2) * g).sum(), ext)
    if "grad_no_rescale" in mut:
        d = d.clone()
        d[:, :3, 3] = d[:, :3, 3] / scale[:, None]
    return -d if "grad_sign" in mut else d


def _column_scale(scale):
    """[R,4,4] of ones with ``scale`` on the translation column (rows 0-2 of column 3)."""
    s = torch.ones((scale.shape[0], 4, 4), dtype=scale.dtype)
    s[:, :3, 3] = scale[:, None]
    return s


def pose_grad_closed(view, near, scale_invariant: bool, dL_dview):
    """The same gradient in closed form: D = -V G^T V, D[:3,3] times 1/near."""
    scale = 1.0 / near if scale_invariant else torch.ones_like(near)
    g = dL_dview.detach().double().cpu()
    return -(view @ g.transpose(-1, -2) @ view) * _column_scale(scale)


def grad_weight(view, near, scale_invariant: bool, g_abs):
    """|V| |G|^T |V| with the column scaling: what a rounding of relative size 1 in G, or in one factor, can move."""
    scale = 1.0 / near if scale_invariant else torch.ones_like(near)
    v = view.abs()
    return (v @ g_abs.transpose(-1, -2) @ v) * _column_scale(scale)


def grad_bound(view, near, scale_invariant: bool, dL_dview):
    """Per element |got - D| <= 16 u (|V| |G|^T |V|), column scaled.  The kernel reads the float32 V twice (2 u), forms two
    length-4 float32 inner products (4 u each), rounds 1/near and multiplies by it (2 u): 12 u, and a third on top for
    contraction and ordering."""
    return GRAD_C * U * grad_weight(view, near, scale_invariant, dL_dview.detach().double().cpu().abs())


def map_partials(sums, mut=NONE):
    """[R,12] summed partials -> dL/dviewmatrix [R,4,4]: slot 3i+j -> [i][j] for i < 3, 9+j -> [3][j], j < 3; the last
    column gets none (the view matrix's last column is constant)."""
    g = torch.zeros((sums.shape[0], 4, 4), dtype=sums.dtype)
    if "partials_last_column" in mut:
        g[:, :3, :] = sums.reshape(-1, 3, 4)
    else:
        g[:, :, :3] = sums.reshape(-1, 4, 3)
    return g


# ---- bounds ----------------------------------------------------------------------------------------------------------
def forward_bounds(x64: dict, near, far) -> dict:
    """Per element bound of |got - x64| for every forward output; ``near``, ``far`` float32 as given to the kernel.

    viewmatrix, tanfov, projmatrix[0][0] and [1][1] are formed in float64 and rounded once: u |x| + 2^-36 M, M the
    render's largest entry (the value itself for tanfov and the two projection entries).  viewmatrix64 is a float64
    output: 2^-36 M.  view_scale is one float32 division: 2 u |x|.  The z entries of the projection -- [2][2] and [2][3]
    of the untransposed matrix -- are float32 from fr = far * scale, nr = near * scale, each carrying at most two
    roundings which the subtraction fr - nr amplifies by (far + near) / (far - near): twice that worst case,
    2 u (2 + 2 (far + near) / (far - near)) |x|.  Every other projection entry is exact: bound 0."""
    n, f = f64(near), f64(far)
    v, v64, t, p = x64["viewmatrix"], x64["viewmatrix64"], x64["tanfov"], x64["projmatrix"]
    big = lambda m: m.abs().amax(dim=(-1, -2), keepdim=True)
    pb = torch.zeros_like(p)
    pb[:, 0, 0] = (U + TINY) * p[:, 0, 0].abs()
    pb[:, 1, 1] = (U + TINY) * p[:, 1, 1].abs()
    z = 2 * U * (2 + 2 * (f + n) / (f - n))
    pb[:, 2, 2] = z * p[:, 2, 2].abs()                   # stored transposed: [2][2] and [3][2]
    pb[:, 3, 2] = z * p[:, 3, 2].abs()
    return {"viewmatrix": U * v.abs() + TINY * big(v), "viewmatrix64": TINY * big(v64).expand_as(v64),
            "tanfov": (U + TINY) * t.abs(), "view_scale": 2 * U * x64["view_scale"].abs(), "projmatrix": pb}


def needed(got, want, bound) -> torch.Tensor:
    """Per render the factor of ``bound`` that ``got`` needs: max over the render's elements of |got - want| / bound
    (0 where both are 0, inf where the bound is 0 and the element is off)."""
    err = (got.detach().double().cpu() - want).abs().reshape(want.shape[0], -1)
    b = bound.reshape(want.shape[0], -1)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)          # x / 0 = inf, 0 / 0 handled
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return ratio.amax(dim=1)
