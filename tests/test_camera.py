"""The camera oracle, its cases and its gate, on the CPU (no GPU): tests/camera_oracle.py against the reference's recorded
call sites and against ``spfsplatv2_amd.decoder.camera_tensors`` in float64, the two float64 forms of its
ill-conditioned parts against each other, the pose gradient against central differences and the closed form, the
partial-slot mapping, the bounds against float32 restatements of the kernel's arithmetic, the power condition of the gate
for every mutant, and the library's argument checks that need no device."""
import ctypes as C

import pytest
import torch

from tests import camera_cases as cases
from tests import camera_oracle as co

CALLSITES = ("decoder_k4_si", "decoder_k25_nosi")
ALL = [(f, si) for f in cases.FAMILIES for si in (True, False)]


def _close(a, b, tol):
    """The closeness of tests/test_glue_goldens.py."""
    assert a.shape == b.shape, (a.shape, b.shape)
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CALLSITES)
def test_oracle_reproduces_the_recorded_call_sites(golden_dir, tag):
    g = torch.load(golden_dir / f"callsite_{tag}.pt")
    i = g["inputs"]
    n = i["near"].numel()
    x = co.forward(i["extrinsics"].reshape(n, 4, 4), i["intrinsics"].reshape(n, 3, 3), i["near"].reshape(n),
                   i["far"].reshape(n), i["make_scale_invariant"])
    view = torch.stack([c["kwargs"]["viewmatrix"] for c in g["calls"]]).double()
    proj = torch.stack([c["settings"]["projmatrix"] for c in g["calls"]]).double()
    tanfov = torch.tensor([[c["settings"]["tanfovx"], c["settings"]["tanfovy"]] for c in g["calls"]], dtype=torch.float64)
    scale = (1 / i["near"].double()).reshape(-1) if i["make_scale_invariant"] else torch.ones(n, dtype=torch.float64)
    _close(x["viewmatrix"], view, 2e-6); _close(x["projmatrix"], proj, 2e-6)
    _close(x["tanfov"], tanfov, 2e-6); _close(x["view_scale"], scale, 2e-6)


@pytest.mark.parametrize("family,si", ALL)
def test_oracle_agrees_with_camera_tensors_in_float64(family, si):
    """The package's own torch preamble run in float64: the same chain, so the same numbers to float64 rounding -- except
    its projection, which it stores in float32 whatever the input (one rounding of each entry)."""
    from spfsplatv2_amd import decoder as dec
    cams, x64, _, _ = cases.forward_reference(family, si)
    view, proj, tanfov, scale = dec.camera_tensors(*(co.f64(cams[k]) for k in ("extrinsics", "intrinsics", "near", "far")),
                                                   si)
    big = x64["viewmatrix"].abs().amax(dim=(-1, -2), keepdim=True)
    assert bool(((view - x64["viewmatrix"]).abs() <= co.TWO_FORMS_INV * big).all())
    assert bool(((tanfov - x64["tanfov"]).abs() <= co.TWO_FORMS_TAN * x64["tanfov"].abs()).all())
    assert torch.equal(scale, x64["view_scale"])
    assert proj.dtype == torch.float32
    p = x64["projmatrix"]
    assert bool(((proj.double() - p).abs() <= (co.U + co.TWO_FORMS_TAN) * p.abs()).all())


@pytest.mark.parametrize("family,si", ALL)
def test_the_two_float64_forms_agree_on_every_camera(family, si):
    """tan(fov/2) through atan2(|a x b|, a.b) against the acos form to 1e-9 relative; the inverse as [M^-1, -M^-1 t]
    against linalg.inv to 2^-40 of the render's largest entry."""
    cams, x64, _, _ = cases.forward_reference(family, si)
    K = co.f64(cams["intrinsics"])
    a, b = co.tan_half_fov(K, "acos"), co.tan_half_fov(K, "atan2")
    assert torch.equal(a, x64["tanfov"])
    rel = ((a - b).abs() / b.abs()).max()
    ext, _, _, _ = co.rescale(co.f64(cams["extrinsics"]), co.f64(cams["near"]), co.f64(cams["far"]), si)
    v = co.view_closed_form(ext)
    big = v.abs().amax(dim=(-1, -2), keepdim=True)
    inv = ((v - x64["viewmatrix"]).abs() / big).max()
    print(f"{family} si={si}: two forms differ by tan {float(rel):.2e} inverse {float(inv):.2e}")
    assert float(rel) <= co.TWO_FORMS_TAN and float(inv) <= co.TWO_FORMS_INV


def test_viewmatrix64_is_the_view_matrix_with_scaled_rows():
    """SpfInputs.viewmatrix64: [p, 1] @ M64 is the rescaled view-space position of the UNscaled mean p."""
    cams, x64, _, _ = cases.forward_reference("general", True)
    p = torch.randn(cases.FAMILY_SIZE, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    one = torch.ones(cases.FAMILY_SIZE, 1, dtype=torch.float64)
    s = x64["view_scale"][:, None]
    a = torch.einsum("ri,rij->rj", torch.cat((p * s, one), dim=1), x64["viewmatrix"])
    b = torch.einsum("ri,rij->rj", torch.cat((p, one), dim=1), x64["viewmatrix64"])
    assert float((a - b).abs().max()) <= 1e-12 * float(a.abs().max())
    off = cases.forward_reference("general", False)[1]
    assert torch.equal(off["viewmatrix64"], off["viewmatrix"]) and bool((off["view_scale"] == 1).all())


# ---- the pose gradient -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,si", ALL)
def test_pose_grad_against_central_differences_and_the_closed_form(family, si):
    """d sum(G * viewmatrix) / d extrinsics, all 16 entries of 24 renders: float64 central differences with h = 1e-6
    (truncation ~ h^2 |V|^2 relative, rounding ~ 1e-16 / h: both below 1e-7 for |V| <= 100) to 1e-6 of the render's
    largest entry; the closed form -V G^T V with its translation column times 1/near to 1e-12."""
    n = 24
    cams, G, want, _, _ = cases.grad_reference(family, si)
    cams, G, want = cases.head(cams, n), G[:n].double(), want[:n]
    ext, near = co.f64(cams["extrinsics"]), co.f64(cams["near"])

    def loss(e):
        e2, _, _, _ = co.rescale(e, near, near, si)
        return (co.view_of(e2) * G).sum(dim=(-1, -2))
    h = 1e-6
    fd = torch.zeros_like(want)
    for i in range(4):
        for j in range(4):
            d = torch.zeros(4, 4, dtype=torch.float64)
            d[i, j] = h
            fd[:, i, j] = (loss(ext + d) - loss(ext - d)) / (2 * h)
    big = want.abs().amax(dim=(-1, -2), keepdim=True)
    assert float(((fd - want).abs() / big).max()) <= 1e-6
    view = cases.forward_reference(family, si)[1]["viewmatrix"][:n]
    closed = co.pose_grad_closed(view, near, si, G)
    assert float(((closed - want).abs() / big).max()) <= 1e-12


@pytest.mark.parametrize("family,si", ALL)
def test_one_hot_gradients_have_exact_zeros(family, si):
    """dL/dviewmatrix one-hot: every element of the result is a single product, so the bound is 0 -- bitwise -- wherever
    the view matrix has a zero.  The oracle must then hold an exact 0 there (the last column of a pose's view matrix is
    0 0 0 1 exactly, whatever linalg.inv leaves in it), and a float32 restatement of the kernel passes."""
    cams, G = cases.one_hot_sweep(family)
    x64 = cases.forward_oracle(cams, si)
    assert bool((x64["viewmatrix"][:, :, 3] == torch.tensor([0.0, 0.0, 0.0, 1.0], dtype=torch.float64)).all())
    want, bound = cases.grad_case(cams, x64["viewmatrix"], si, G)
    assert int((bound == 0).sum()) > 0 and bool((want[bound == 0] == 0).all())
    v = x64["viewmatrix"].float()
    d = -(v @ G.transpose(-1, -2) @ v)
    if si:
        d[:, :3, 3] = d[:, :3, 3] * (1.0 / cams["near"])[:, None]
    assert float(co.needed(d, want, bound).max()) <= 1.0


def test_partial_slot_mapping_element_by_element():
    """Slot 3i+j -> [i][j] (i, j < 3), 9+j -> [3][j], nothing to the last column; the mutant reads four per row."""
    s = torch.arange(1.0, 25.0, dtype=torch.float64).reshape(2, 12)
    g, m = co.map_partials(s), co.map_partials(s, frozenset(["partials_last_column"]))
    for r in range(2):
        for i in range(4):
            for j in range(4):
                want = 0.0 if j == 3 else float(s[r, 3 * i + j if i < 3 else 9 + j])
                assert float(g[r, i, j]) == want
                assert float(m[r, i, j]) == (0.0 if i == 3 else float(s[r, 4 * i + j]))
    p = cases.exact_partials(5, 1954, pad=7)
    assert bool(torch.isnan(p[-7:]).all()) and p.numel() == 5 * 1954 * 12 + 7
    q = p[:-7].reshape(5, 1954, 12)
    assert bool((q * 256 == (q * 256).round()).all()) and float(q.abs().max()) <= 4.0
    assert torch.equal(q.sum(dim=1), q.flip(1).sum(dim=1)) and torch.equal(q.sum(dim=1).double(), q.double().sum(dim=1))


# ---- the bounds ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,si", ALL)
def test_float32_restatements_of_the_kernel_pass_the_gate(family, si):
    """The bounds are not impossible: the oracle rounded once to float32, and the projection's z entries formed in
    float32 the way the kernel forms them (scale = 1/near, nr = near * scale, fr = far * scale, fr / (fr - nr),
    -(fr * nr) / (fr - nr)), pass -- and a float32 gradient formed like the kernel's passes the gradient bound."""
    cams, x64, bounds, dists = cases.forward_reference(family, si)
    got = {k: v.float() for k, v in x64.items()}
    got["viewmatrix64"] = x64["viewmatrix64"].clone()
    near, far = cams["near"], cams["far"]
    scale = (1.0 / near) if si else torch.ones_like(near)
    nr, fr = near * scale, far * scale
    got["projmatrix"][:, 2, 2] = fr / (fr - nr)
    got["projmatrix"][:, 3, 2] = -(fr * nr) / (fr - nr)
    need = cases.gate(f"float32 restatement {family} si={si}", got, x64, bounds, dists)
    assert need["viewmatrix64"] == 0.0
    _, G, want, bound, _ = cases.grad_reference(family, si)
    v = got["viewmatrix"]
    d = -(v @ G.transpose(-1, -2) @ v)
    d[:, :3, 3] = d[:, :3, 3] * scale[:, None]
    c = float(co.needed(d, want, bound).max())
    print(f"float32 restatement {family} si={si} {cases.GRAD_OUT}: c_needed {c:.3f}")
    assert c <= 1.0


def test_the_gate_fails_what_is_one_float32_rounding_too_many():
    """A float32 intermediate cannot hide: the inverse taken in float32 leaves the viewmatrix bound on most renders."""
    cams, x64, bounds, _ = cases.forward_reference("general", True)
    ext, _, _, _ = co.rescale(co.f64(cams["extrinsics"]), co.f64(cams["near"]), co.f64(cams["far"]), True)
    v32 = torch.linalg.inv(ext.float()).transpose(-1, -2)
    need = co.needed(v32, x64["viewmatrix"], bounds["viewmatrix"])
    assert int((need > 1).sum()) > cases.FAMILY_SIZE // 2


# ---- the power condition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,si", ALL)
def test_power_condition_of_every_mutant(family, si):
    """Every mutant, in every output it reaches, on every render of the families it reaches, at every size."""
    _, _, _, fdists = cases.forward_reference(family, si)
    cams, _, want, bound, gdists = cases.grad_reference(family, si)
    for m in co.FORWARD_MUTANTS + co.GRAD_MUTANTS:
        assert (m in fdists or m in gdists) == cases.reached(m, family, si), m
    for m, d in fdists.items():
        assert sorted(d) == sorted(k for k in co.FORWARD_NAMES if k not in cases.UNREACHED[m]), m
    bad = []
    for R in cases.SIZES:
        bad += cases.power_failures(f"{family} si={si} R={R}", {**fdists, **gdists}, R)
    assert not bad, "\n".join(bad)


def test_unreached_pairs_are_unreached():
    """What the lists say a mutant cannot move, it does not move at all: bitwise the oracle."""
    for family, si in ALL:
        cams, x64, _, _ = cases.forward_reference(family, si)
        _, G, want, _, _ = cases.grad_reference(family, si)
        for m in co.FORWARD_MUTANTS:
            mu = cases.forward_oracle(cams, si, frozenset([m]))
            names = co.FORWARD_NAMES if (m in cases.NEEDS_SCALE and not si) else cases.UNREACHED[m]
            for k in names:
                assert torch.equal(mu[k], x64[k]), (m, family, si, k)
        if not si:
            assert torch.equal(co.pose_grad(cams["extrinsics"], cams["near"], si, G, frozenset(["grad_no_rescale"])), want)
    # fov_from_focal under the centred family: the truth to float64 rounding
    cams, x64, _, _ = cases.forward_reference("centred", True)
    mu = cases.forward_oracle(cams, True, frozenset(["fov_from_focal"]))
    assert float(((mu["tanfov"] - x64["tanfov"]).abs() / x64["tanfov"]).max()) <= co.TWO_FORMS_TAN


@pytest.mark.parametrize("si", [True, False])
def test_power_condition_of_the_partials_mutant(si):
    for R in cases.PARTIAL_R:
        cams = cases.cameras("general", R)
        view = cases.forward_reference("general", si)[1]["viewmatrix"][:R]
        for nblk in cases.NBLK:
            sums = cases.exact_partials(R, nblk).reshape(R, nblk, 12).double().sum(dim=1)
            want, bound = cases.grad_case(cams, view, si, co.map_partials(sums))
            d = cases.partial_mutant_distance(cams, view, si, sums, want, bound)
            bad = cases.power_failures(f"partials R={R} nblk={nblk} si={si}", d, R)
            assert not bad, "\n".join(bad)


def test_cameras_cover_the_ranges():
    for name in cases.FAMILIES:
        c = cases.family(name)
        assert all(v.dtype == torch.float32 and v.shape[0] == cases.FAMILY_SIZE for v in c.values())
        near, far, K = c["near"].double(), c["far"].double(), c["intrinsics"].double()
        assert bool((((near >= 0.049) & (near <= 0.501)) | ((near >= 1.99) & (near <= 10.01))).all())
        assert float((far / near).min()) >= 1.0099 and float((far / near).max()) <= 1.0001e4
        t = c["extrinsics"][:, :3, 3].double().norm(dim=-1)
        assert 0.0099 <= float(t.min()) and float(t.max()) <= 5.001
        hi = 4.0 if name == "offcentre" else 200.0
        for f in (K[:, 0, 0], K[:, 1, 1]):
            assert 0.2499 <= float(f.min()) and float(f.max()) <= hi * 1.0001
        assert float((K[:, :2, 2] - 0.5).abs().max()) <= 0.1501
        R3 = c["extrinsics"][:, :3, :3].double()
        assert float((R3 @ R3.transpose(-1, -2) - torch.eye(3, dtype=torch.float64)).abs().max()) < 1e-6
        angle = torch.acos(((R3.diagonal(dim1=-1, dim2=-2).sum(-1) - 1) / 2).clamp(-1, 1))
        first = angle[:3].sort().values                                  # the identity, pi - 1e-3 and pi
        assert float(first[0]) < 1e-3 and 3.14 < float(first[1]) < 3.1412 and float(first[2]) > 3.1414
    g = cases.family("general")["intrinsics"]
    assert float(g[:, 0, 0].max()) > 100 and float(g[:, 0, 0].min()) < 0.5       # narrow and wide lenses are drawn
    assert bool((cases.family("centred")["intrinsics"][:, :2, 2] == 0.5).all())
    assert float((cases.family("offcentre")["intrinsics"][:, :2, 2] - 0.5).abs().min()) >= 0.0499
    big = cases.cameras("general", 700)
    assert big["near"].shape == (700,)
    assert torch.equal(big["extrinsics"][650], cases.family("general")["extrinsics"][50])


# ---- the library's argument checks, host side ------------------------------------------------------------------------
def test_library_argument_checks_on_the_host(hip_lib):
    """Rejected with -1 and a message before anything touches a device (the pointers are never read)."""
    from spfsplatv2_amd import _lib
    err = hip_lib.spf_last_error
    p = 4096                                                            # a 16-byte aligned non-null address

    def cam(**kw):
        c = _lib.SpfCamera(p, p, p, p, p, p, p, p, 5, 1, p)
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)
    fwd, prep = hip_lib.spf_camera_forward, hip_lib.spf_decoder_prepare
    bwd, part = hip_lib.spf_camera_backward, hip_lib.spf_camera_backward_partials
    assert fwd(None, None) == -1 and b"camera is null" in err()
    assert prep(None, p, 16, None) == -1 and b"camera is null" in err()
    assert bwd(None, p, p, None) == -1 and b"camera is null" in err()
    assert part(None, p, 1, p, None) == -1 and b"camera is null" in err()
    for R in (0, -3):
        assert fwd(cam(R=R), None) == -1 and b"R must be positive" in err()
        assert prep(cam(R=R), p, 16, None) == -1 and b"R must be positive" in err()
        assert bwd(cam(R=R), p, p, None) == -1 and b"R must be positive" in err()
        assert part(cam(R=R), p, 1, p, None) == -1 and b"R must be positive" in err()
    for name in ("extrinsics", "intrinsics", "near", "far", "viewmatrix", "projmatrix", "tanfov"):
        assert fwd(cam(**{name: None}), None) == -1 and b"a camera pointer is null" in err(), name
        assert prep(cam(**{name: None}), p, 16, None) == -1 and b"a camera pointer is null" in err(), name
    for name in ("near", "viewmatrix"):                                  # all the backward reads
        assert bwd(cam(**{name: None}), p, p, None) == -1 and b"a camera pointer is null" in err(), name
        assert part(cam(**{name: None}), p, 1, p, None) == -1 and b"a camera pointer is null" in err(), name
    for zero, nbytes in ((None, 16), (p + 4, 16), (p + 8, 32), (p, 8), (p, 24)):
        assert prep(cam(), zero, nbytes, None) == -1 and b"16-byte aligned and sized" in err(), (zero, nbytes)
    assert bwd(cam(), None, p, None) == -1 and b"gradient pointer is null" in err()
    assert bwd(cam(), p, None, None) == -1 and b"gradient pointer is null" in err()
    for args in ((None, 1, p), (p, 1, None), (p, 0, p), (p, -1, p)):
        assert part(cam(), *args, None) == -1 and b"camera_backward_partials: bad argument" in err(), args
    for off in (4, 8, 12):
        assert part(cam(), p + off, 1, p, None) == -1 and b"vpartial must be 16-byte aligned" in err(), off
