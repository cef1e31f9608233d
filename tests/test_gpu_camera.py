"""The camera kernels on the device (csrc/camera.hip: spf_camera_fwd_kernel, spf_camera_fwd_zero_kernel,
spf_camera_bwd_kernel, spf_camera_bwd_reduce_kernel), driven through the C ABI -- spf_camera_forward, spf_decoder_prepare,
spf_camera_backward, spf_camera_backward_partials -- and through ``spf.camera_forward``.

Gate (tests/camera_cases.py): per output and render c_needed = max |got - x64| / bound against the float64 oracle of
tests/camera_oracle.py, with bounds derived from float32 / float64 rounding, must not exceed 1; before a gate is trusted
the power condition of tests/test_camera.py is asserted again.  Every figure is printed, with the figures of the float32
eager ``decoder.camera_tensors`` on the device beside them for information (profiles/camera_gate_figures.txt holds one
run's).
"""
import ctypes as C

import pytest
import torch

from tests import camera_cases as cases
from tests import camera_oracle as co

pytestmark = pytest.mark.gpu

DEV = "cuda"
FILL = 7.0                                 # what the output buffers hold before a call
FWD = ("viewmatrix", "projmatrix", "tanfov", "view_scale", "viewmatrix64")


# ---- the product -----------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(d):
    return {k: v.to(DEV).contiguous() for k, v in d.items()}


def _outputs(R):
    f = lambda *s, dt=torch.float32: torch.full(s, FILL, dtype=dt, device=DEV)
    return {"viewmatrix": f(R, 4, 4), "projmatrix": f(R, 4, 4), "tanfov": f(R, 2), "view_scale": f(R),
            "viewmatrix64": f(R, 4, 4, dt=torch.float64)}


def _camera(d, out, si, without=()):
    from spfsplatv2_amd import _lib
    o = {k: (None if k in without else v) for k, v in out.items()}
    R = d["near"].shape[0]
    return _lib.SpfCamera(_p(d["extrinsics"]), _p(d["intrinsics"]), _p(d["near"]), _p(d["far"]), _p(o["viewmatrix"]),
                          _p(o["projmatrix"]), _p(o["tanfov"]), _p(o["view_scale"]), R, 1 if si else 0,
                          _p(o["viewmatrix64"]))


def run_forward(lib, d, si, without=(), out=None):
    """spf_camera_forward on device inputs ``d`` -> {output: device tensor} (the outputs in ``without`` passed as NULL)."""
    out = out or _outputs(d["near"].shape[0])
    cam = _camera(d, out, si, without)
    assert lib.spf_camera_forward(C.byref(cam), _stream()) == 0, lib.spf_last_error()
    return out


def run_prepare(lib, d, si, zero, zero_bytes, out=None):
    out = out or _outputs(d["near"].shape[0])
    cam = _camera(d, out, si)
    assert lib.spf_decoder_prepare(C.byref(cam), zero, zero_bytes, _stream()) == 0, lib.spf_last_error()
    return out


def run_backward(lib, d, out, si, G, dext=None):
    """spf_camera_backward with cam->viewmatrix of a forward -> dL/dextrinsics [R,4,4]."""
    dext = torch.full_like(out["viewmatrix"], FILL) if dext is None else dext
    cam = _camera(d, out, si)
    assert lib.spf_camera_backward(C.byref(cam), _p(G), _p(dext), _stream()) == 0, lib.spf_last_error()
    return dext


def run_partials(lib, d, out, si, vpartial, nblk, dext=None):
    dext = torch.full_like(out["viewmatrix"], FILL) if dext is None else dext
    cam = _camera(d, out, si)
    assert lib.spf_camera_backward_partials(C.byref(cam), _p(vpartial), nblk, _p(dext), _stream()) == 0, \
        lib.spf_last_error()
    return dext


def eager_forward(d, si):
    """decoder.camera_tensors in float32 on the device (information only)."""
    from spfsplatv2_amd import decoder as dec
    view, proj, tanfov, scale = dec.camera_tensors(d["extrinsics"], d["intrinsics"], d["near"], d["far"], si)
    return {"viewmatrix": view, "projmatrix": proj, "tanfov": tanfov, "view_scale": scale}


def eager_grad(d, si, G):
    from spfsplatv2_amd import decoder as dec
    ext = d["extrinsics"].clone().requires_grad_(True)
    view = dec.camera_tensors(ext, d["intrinsics"], d["near"], d["far"], si)[0]
    return torch.autograd.grad(view, ext, G)[0]


def _same(a: dict, b: dict, names=None):
    for k in names or a:
        assert torch.equal(a[k], b[k]), k


# ---- a. spf_camera_forward -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [True, False])
@pytest.mark.parametrize("R", cases.SIZES)
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_forward_against_oracle(hip_lib, family, R, si):
    """All five outputs of every camera family at every R, both ways of scale_invariant."""
    cams, x64, bounds, dists = cases.forward_reference(family, si)
    cams, x64, bounds = cases.head(cams, R), cases.head(x64, R), cases.head(bounds, R)
    d = _dev(cams)
    got = run_forward(hip_lib, d, si)
    eager = eager_forward(d, si) if R == cases.FAMILY_SIZE else None
    assert got["viewmatrix64"].dtype == torch.float64
    cases.gate(f"forward {family} R={R} si={si}", got, x64, bounds, dists, eager)
    # what the bounds call exact, bit for bit: +0 off the five entries, 1 at the w entry (stored transposed: [2][3])
    bits = got["projmatrix"].view(torch.int32).cpu()
    zero = torch.ones(4, 4, dtype=torch.bool)
    for i, j in ((0, 0), (1, 1), (2, 2), (3, 2), (2, 3)):
        zero[i, j] = False
    assert bool((bits[:, zero] == 0).all())
    assert bool((got["projmatrix"][:, 2, 3] == 1.0).all())
    if not si:
        assert bool((got["view_scale"] == 1.0).all())


@pytest.mark.parametrize("si", [True, False])
def test_optional_outputs_may_be_null(hip_lib, si):
    """view_scale = NULL and viewmatrix64 = NULL leave the other outputs bitwise unchanged (and their buffers alone)."""
    d = _dev(cases.cameras("general", 65))
    full = run_forward(hip_lib, d, si)
    for without in (("view_scale",), ("viewmatrix64",), ("view_scale", "viewmatrix64")):
        got = run_forward(hip_lib, d, si, without)
        _same(got, full, [k for k in FWD if k not in without])
        for k in without:
            assert bool((got[k] == FILL).all()), k


def test_the_gate_rejects_the_product_run_with_a_neighbours_near(hip_lib):
    """The control of the gate on the device: the PRODUCT fed near of the next render (the families alternate between
    near < 0.5 and near > 2) leaves the bound on every render in everything 1/near enters."""
    cams, x64, bounds, _ = cases.forward_reference("general", True)
    wrong = dict(cams, near=cams["near"].roll(-1))
    got = run_forward(hip_lib, _dev(wrong), True)
    for k in ("viewmatrix", "viewmatrix64", "view_scale", "projmatrix"):
        need = co.needed(got[k], x64[k], bounds[k])
        print(f"neighbour's near {k}: least c_needed over the renders {float(need.min()):.3g}")
        assert float(need.min()) > 1.0, k
    assert float(co.needed(got["tanfov"], x64["tanfov"], bounds["tanfov"]).max()) <= 1.0


@pytest.mark.parametrize("mutant", co.MUTANTS)
def test_gate_catches_mutants(hip_lib, mutant):
    """The gate is worth something: with the bounds it has for the true oracle, an oracle with one deliberate mistake
    (standing for a kernel that makes it) fails against the product's real output -- on every render, in every output the
    mutant reaches."""
    mut = frozenset([mutant])
    family = "offcentre" if mutant == "fov_from_focal" else "general"
    cams, x64, bounds, _ = cases.forward_reference(family, True)
    d = _dev(cams)
    out = run_forward(hip_lib, d, True)
    if mutant in co.FORWARD_MUTANTS:
        wrong = cases.forward_oracle(cams, True, mut)
        for k in FWD:
            need = co.needed(out[k], wrong[k], bounds[k])
            print(f"mutant {mutant} {k}: c_needed {float(need.min()):.3g} .. {float(need.max()):.3g}")
            if k in cases.UNREACHED[mutant]:
                assert float(need.max()) <= 1.0, k
            else:
                assert float(need.min()) > 1.0, k
        return
    if mutant in co.GRAD_MUTANTS:
        _, G, _, bound, _ = cases.grad_reference(family, True)
        got = run_backward(hip_lib, d, out, True, G.to(DEV))
    else:
        nblk = 65
        p = cases.exact_partials(cases.FAMILY_SIZE, nblk)
        G = co.map_partials(p.reshape(-1, nblk, 12).double().sum(dim=1), mut)
        bound = cases.grad_case(cams, x64["viewmatrix"], True, co.map_partials(p.reshape(-1, nblk, 12).double().sum(dim=1)))[1]
        got = run_partials(hip_lib, d, out, True, p.to(DEV), nblk)
        mut = co.NONE
    wrong = co.pose_grad(cams["extrinsics"], cams["near"], True, G, mut)
    need = co.needed(got, wrong, bound)
    print(f"mutant {mutant} {cases.GRAD_OUT}: c_needed {float(need.min()):.3g} .. {float(need.max()):.3g}")
    assert float(need.min()) > 1.0


# ---- b. spf.camera_forward -------------------------------------------------------------------------------------------
def _sv(d, S, V):
    return {k: v.reshape(S, V, *v.shape[1:]) for k, v in d.items()}


def test_python_entry_point_is_the_flat_call(hip_lib):
    """[S,V] = [3,5] inputs give the R = 15 result, bit for bit."""
    import spfsplatv2_amd as spf
    d = _dev(cases.cameras("general", 15))
    for si in (True, False):
        flat = run_forward(hip_lib, d, si)
        s = _sv(d, 3, 5)
        got = spf.camera_forward(s["extrinsics"], s["intrinsics"], s["near"], s["far"], si)
        for k, t in zip(FWD, got):
            assert torch.equal(t.reshape(flat[k].shape), flat[k]), k


def test_python_entry_point_copies_views_and_refuses_float64(hip_lib):
    """rasterizer._check_camera: a dense float32 tensor goes through as it is, a non-contiguous view ([:, ::2]) is COPIED
    to a dense one -- the result is that of the contiguous copy, bit for bit -- and float64 is REFUSED, not cast."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import rasterizer
    S, V = 3, 5
    wide = _sv(_dev(cases.cameras("general", S * 2 * V)), S, 2 * V)
    view = {k: v[:, ::2] for k, v in wide.items()}
    dense = {k: v.contiguous() for k, v in view.items()}
    order = ("extrinsics", "intrinsics", "near", "far")
    assert not any(view[k].is_contiguous() for k in order)
    for a, b, c in zip(rasterizer._check_camera(*(view[k] for k in order), S, V), (view[k] for k in order),
                       (dense[k] for k in order)):
        assert a.is_contiguous() and a.data_ptr() != b.data_ptr() and torch.equal(a, c)
    for a, c in zip(rasterizer._check_camera(*(dense[k] for k in order), S, V), (dense[k] for k in order)):
        assert a is c
    got = spf.camera_forward(*(view[k] for k in order), True)
    want = spf.camera_forward(*(dense[k] for k in order), True)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    flat = {k: dense[k].reshape(S * V, *dense[k].shape[2:]).cpu() for k in order}
    x64 = cases.forward_oracle(flat, True)
    bounds = co.forward_bounds(x64, flat["near"], flat["far"])
    for k, t in zip(FWD, got):
        assert float(co.needed(t.reshape(x64[k].shape), x64[k], bounds[k]).max()) <= 1.0, k
    for k in order:
        args = [dense[n].double() if n == k else dense[n] for n in order]
        with pytest.raises(RuntimeError, match=f"{k} must be float32"):
            spf.camera_forward(*args, True)
        with pytest.raises(RuntimeError, match=f"{k} must be float32"):
            rasterizer._check_camera(*args, S, V)


# ---- c. spf_decoder_prepare ------------------------------------------------------------------------------------------
GUARD = 16
STRIDED_RENDERS = 1024 * 256 + 5


@pytest.mark.parametrize("R,zero_bytes", [(1, 0), (300, 16), (5, 48), (65, 16 * 1000), (5, 4 * 1024 * 1024 + 592),
                                          (STRIDED_RENDERS, 16)])
def test_decoder_prepare_clears_its_bytes_and_sets_the_cameras_up(hip_lib, R, zero_bytes):
    """The cameras of spf_camera_forward bit for bit, and exactly ``zero_bytes`` bytes cleared: more renders than vectors,
    more vectors than renders, more vectors than one pass of the 1024 x 256 lanes covers (the clearing loop strides),
    more renders than that (the camera loop strides); 16 guard bytes on either side keep their pattern."""
    si = True
    cams = cases.cameras("general", R)
    d = _dev(cams)
    want = run_forward(hip_lib, d, si)
    buf = torch.full((GUARD + zero_bytes + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    got = run_prepare(hip_lib, d, si, C.c_void_p(buf.data_ptr() + GUARD), zero_bytes)
    _same(got, want)
    assert bool((buf[:GUARD] == 0xFF).all()) and bool((buf[GUARD + zero_bytes:] == 0xFF).all())
    assert bool((buf[GUARD:GUARD + zero_bytes] == 0).all())
    assert buf.numel() == 2 * GUARD + zero_bytes
    # against the oracle: every render, or a strided sample of 300 of them (render r is camera r % 300)
    idx = torch.arange(min(R, cases.FAMILY_SIZE)) * (871 if R > cases.FAMILY_SIZE else 1) + (7 if R > cases.FAMILY_SIZE else 0)
    assert int(idx.max()) < R
    fam = idx % cases.FAMILY_SIZE
    _, x64, bounds, dists = cases.forward_reference("general", si)
    pick = lambda t: {k: v[fam] for k, v in t.items()}
    cases.gate(f"prepare R={R} zero_bytes={zero_bytes}", {k: v[idx.to(DEV)] for k, v in got.items()}, pick(x64),
               pick(bounds), {m: pick(v) for m, v in dists.items()})


# ---- d. spf_camera_backward ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [True, False])
@pytest.mark.parametrize("R", cases.SIZES)
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_backward_against_oracle(hip_lib, family, R, si):
    """cam->viewmatrix from the forward, a random dL/dviewmatrix."""
    cams, G, want, bound, dists = cases.grad_reference(family, si)
    cams, G, want, bound = cases.head(cams, R), G[:R], want[:R], bound[:R]
    d, Gd = _dev(cams), G.to(DEV)
    out = run_forward(hip_lib, d, si)
    got = run_backward(hip_lib, d, out, si, Gd)
    eager = {cases.GRAD_OUT: eager_grad(d, si, Gd)} if R == cases.FAMILY_SIZE else None
    cases.gate(f"backward {family} R={R} si={si}", {cases.GRAD_OUT: got}, {cases.GRAD_OUT: want}, {cases.GRAD_OUT: bound},
               dists, eager)


@pytest.mark.parametrize("si", [True, False])
@pytest.mark.parametrize("family", cases.FAMILIES)
def test_backward_one_hot_sweep(hip_lib, family, si):
    """dL/dviewmatrix one-hot at each of its 16 entries, on the first three renders of the family (the identity and the
    two half turns among them): which entry goes where, element by element, under the same bound."""
    cams, G = cases.one_hot_sweep(family)
    d = _dev(cams)
    out = run_forward(hip_lib, d, si)
    got = run_backward(hip_lib, d, out, si, G.to(DEV))
    x64 = cases.forward_oracle(cams, si)
    want, bound = cases.grad_case(cams, x64["viewmatrix"], si, G)
    assert int((bound == 0).sum()) > 0                  # a one-hot leaves exact zeros: those are held bitwise
    cases.gate(f"backward one-hot {family} si={si}", {cases.GRAD_OUT: got}, {cases.GRAD_OUT: want},
               {cases.GRAD_OUT: bound}, {})


# ---- e. spf_camera_backward_partials ---------------------------------------------------------------------------------
POISON = 12 * 64


def _partial_setup(hip_lib, R, si):
    cams = cases.cameras("general", R)
    d = _dev(cams)
    out = run_forward(hip_lib, d, si)
    view = cases.forward_reference("general", si)[1]["viewmatrix"][:R]
    return cams, d, out, view


@pytest.mark.parametrize("nblk", cases.NBLK)
@pytest.mark.parametrize("R", cases.PARTIAL_R)
def test_partials_with_exact_sums(hip_lib, R, nblk):
    """Partials that are integer multiples of 2^-8: the summed dL/dviewmatrix is exact in float32 in any order, so the
    result obeys the plain gradient bound against the oracle fed the mapped 4x4.  The floats past R * nblk * 12 are NaN
    and are not read."""
    for si in (True, False):
        cams, d, out, view = _partial_setup(hip_lib, R, si)
        p = cases.exact_partials(R, nblk, pad=POISON)
        sums = p[:R * nblk * 12].reshape(R, nblk, 12).double().sum(dim=1)
        want, bound = cases.grad_case(cams, view, si, co.map_partials(sums))
        dists = cases.partial_mutant_distance(cams, view, si, sums, want, bound)
        pd = p.to(DEV)
        assert pd.data_ptr() % 16 == 0
        got = run_partials(hip_lib, d, out, si, pd, nblk)
        cases.gate(f"partials exact R={R} nblk={nblk} si={si}", {cases.GRAD_OUT: got}, {cases.GRAD_OUT: want},
                   {cases.GRAD_OUT: bound}, dists)
        clean = run_partials(hip_lib, d, out, si, p[:R * nblk * 12].to(DEV), nblk)
        assert torch.equal(got, clean)


@pytest.mark.parametrize("nblk", cases.NBLK)
@pytest.mark.parametrize("R", cases.PARTIAL_R)
def test_partials_with_random_floats(hip_lib, R, nblk):
    """General float partials: two runs agree bit for bit, and the result is within the gradient bound plus the
    order-free summation bound (nblk - 1) u sum|p| carried through |V| . |V| -- loose, as any bound that knows nothing
    of the order is."""
    for si in (True, False):
        cams, d, out, view = _partial_setup(hip_lib, R, si)
        p = cases.random_partials(R, nblk)
        p3 = p.reshape(R, nblk, 12).double()
        want, bound = cases.grad_case(cams, view, si, co.map_partials(p3.sum(dim=1)))
        slack = co.grad_weight(view, co.f64(cams["near"]), si, co.map_partials((nblk - 1) * co.U * p3.abs().sum(dim=1)))
        pd = p.to(DEV)
        got, again = run_partials(hip_lib, d, out, si, pd, nblk), run_partials(hip_lib, d, out, si, pd, nblk)
        assert torch.equal(got, again)
        cases.gate(f"partials random R={R} nblk={nblk} si={si}", {cases.GRAD_OUT: got}, {cases.GRAD_OUT: want},
                   {cases.GRAD_OUT: bound + slack}, {})


@pytest.mark.parametrize("nblk", [1, 65, 257])
def test_partials_one_hot_sweep(hip_lib, nblk):
    """A single 1 in each of the 12 slots in turn (in some block of the record): the mapping, element by element."""
    R = 5
    for si in (True, False):
        p = cases.one_hot_partials(R, nblk)
        idx = torch.arange(R).repeat_interleave(12)
        cams = {k: v[idx] for k, v in cases.cameras("general", R).items()}
        d = _dev(cams)
        out = run_forward(hip_lib, d, si)
        G = co.map_partials(p.double().sum(dim=1))
        for r in range(R):
            for s in range(12):
                assert float(G[12 * r + s, s // 3, s % 3]) == 1.0 and float(G[12 * r + s].sum()) == 1.0
        x64 = cases.forward_oracle(cams, si)
        want, bound = cases.grad_case(cams, x64["viewmatrix"], si, G)
        got = run_partials(hip_lib, d, out, si, p.to(DEV), nblk)
        cases.gate(f"partials one-hot nblk={nblk} si={si}", {cases.GRAD_OUT: got}, {cases.GRAD_OUT: want},
                   {cases.GRAD_OUT: bound}, {})


# ---- f. repeatability, g. no host synchronisation --------------------------------------------------------------------
def _all_entry_points(lib, d, G, p, nblk, buf):
    """Every entry point once -> the tensors they wrote."""
    import spfsplatv2_amd as spf
    a = run_forward(lib, d, True)
    b = run_prepare(lib, d, True, C.c_void_p(buf.data_ptr()), buf.numel())
    c = run_backward(lib, d, a, True, G)
    e = run_partials(lib, d, a, True, p, nblk)
    R = d["near"].shape[0]
    f = spf.camera_forward(*(d[k].reshape(1, R, *d[k].shape[1:]) for k in ("extrinsics", "intrinsics", "near", "far")))
    return [*a.values(), *b.values(), c, e, *f]


def test_every_entry_point_is_bitwise_repeatable_and_never_syncs(hip_lib):
    R, nblk = 300, 257
    d = _dev(cases.cameras("general", R))
    G, p = cases.upstream("general").to(DEV), cases.random_partials(R, nblk).to(DEV)
    buf = torch.full((16 * 1000,), 0xFF, dtype=torch.uint8, device=DEV)
    first = _all_entry_points(hip_lib, d, G, p, nblk, buf)
    assert bool((buf == 0).all())
    second = _all_entry_points(hip_lib, d, G, p, nblk, buf)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        third = _all_entry_points(hip_lib, d, G, p, nblk, buf)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(first) == len(second) == len(third) == 16
    for a, b, c in zip(first, second, third):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---- h. the library's argument checks --------------------------------------------------------------------------------
def test_library_argument_checks_launch_nothing(hip_lib):
    """-1 with a message in spf_last_error(), on real device buffers that must come back untouched."""
    R, nblk = 5, 3
    d = _dev(cases.cameras("general", R))
    out = _outputs(R)
    dext = torch.full((R, 4, 4), FILL, device=DEV)
    G = torch.ones(R, 4, 4, device=DEV)
    vp = torch.ones(R * nblk * 12 + 4, device=DEV)
    buf = torch.full((64,), 0xFF, dtype=torch.uint8, device=DEV)
    err, s = hip_lib.spf_last_error, _stream()
    fwd, prep = hip_lib.spf_camera_forward, hip_lib.spf_decoder_prepare
    bwd, part = hip_lib.spf_camera_backward, hip_lib.spf_camera_backward_partials

    def cam(**kw):
        c = _camera(d, out, True)
        for k, v in kw.items():
            setattr(c, k, v)
        return C.byref(c)
    zero = C.c_void_p(buf.data_ptr() + 16)
    assert fwd(None, s) == -1 and b"camera is null" in err()
    assert prep(None, zero, 16, s) == -1 and b"camera is null" in err()
    assert bwd(None, _p(G), _p(dext), s) == -1 and b"camera is null" in err()
    assert part(None, _p(vp), nblk, _p(dext), s) == -1 and b"camera is null" in err()
    assert fwd(cam(R=0), s) == -1 and b"R must be positive" in err()
    assert prep(cam(R=0), zero, 16, s) == -1 and b"R must be positive" in err()
    assert bwd(cam(R=0), _p(G), _p(dext), s) == -1 and b"R must be positive" in err()
    assert part(cam(R=0), _p(vp), nblk, _p(dext), s) == -1 and b"R must be positive" in err()
    for name in ("extrinsics", "intrinsics", "near", "far", "viewmatrix", "projmatrix", "tanfov"):
        assert fwd(cam(**{name: None}), s) == -1 and b"a camera pointer is null" in err(), name
        assert prep(cam(**{name: None}), zero, 16, s) == -1 and b"a camera pointer is null" in err(), name
    for name in ("near", "viewmatrix"):
        assert bwd(cam(**{name: None}), _p(G), _p(dext), s) == -1 and b"a camera pointer is null" in err(), name
        assert part(cam(**{name: None}), _p(vp), nblk, _p(dext), s) == -1 and b"a camera pointer is null" in err(), name
    for z, n in ((None, 16), (C.c_void_p(buf.data_ptr() + 20), 16), (zero, 24), (zero, 8)):
        assert prep(cam(), z, n, s) == -1 and b"16-byte aligned and sized" in err(), n
    assert bwd(cam(), None, _p(dext), s) == -1 and b"gradient pointer is null" in err()
    assert bwd(cam(), _p(G), None, s) == -1 and b"gradient pointer is null" in err()
    assert part(cam(), _p(vp), 0, _p(dext), s) == -1 and b"camera_backward_partials: bad argument" in err()
    assert part(cam(), None, nblk, _p(dext), s) == -1 and b"camera_backward_partials: bad argument" in err()
    assert part(cam(), _p(vp), nblk, None, s) == -1 and b"camera_backward_partials: bad argument" in err()
    assert vp.data_ptr() % 16 == 0                     # one float on: off the 16-byte boundary, rejected on the host
    assert part(cam(), C.c_void_p(vp.data_ptr() + 4), nblk, _p(dext), s) == -1 and b"must be 16-byte aligned" in err()
    torch.cuda.synchronize()
    for k, t in out.items():
        assert bool((t == FILL).all()), k
    assert bool((dext == FILL).all()) and bool((buf == 0xFF).all())
    # and the same calls, well formed, do launch
    assert fwd(cam(), s) == 0 and prep(cam(), zero, 32, s) == 0
    assert bwd(cam(), _p(G), _p(dext), s) == 0 and part(cam(), _p(vp), nblk, _p(dext), s) == 0
    torch.cuda.synchronize()
    assert bool((out["viewmatrix"] != FILL).any()) and bool((dext != FILL).any())
    assert bool((buf[:16] == 0xFF).all()) and bool((buf[16:48] == 0).all()) and bool((buf[48:] == 0xFF).all())
