"""Precomputed 3-D covariances (cov3Ds_precomp) on the host side: the ABI 7 entry points, their argument validation
before any launch, and the Python surfaces' exclusivity rules.  No GPU needed."""
import ctypes as C

import pytest
import torch

from tests.test_abi import _declared_symbols

EXCLUSIVE = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"
NEW = ("spf_raster_forward_project_cov3d", "spf_raster_backward_cov3d")


def test_abi_7_declares_and_exports_the_cov3d_entry_points(hip_lib):
    from spfsplatv2_amd import _lib
    assert hip_lib.spf_abi_version() == 7 == _lib.ABI_VERSION
    declared = _declared_symbols()
    for name in NEW:
        assert name in declared and name in _lib.SYMBOLS and hasattr(hip_lib, name), name
    assert len(_lib.SYMBOLS["spf_raster_forward_project_cov3d"][1]) == 6
    assert len(_lib.SYMBOLS["spf_raster_backward_cov3d"][1]) == 9


def _dims(layout=0):
    from spfsplatv2_amd import _lib
    return _lib.SpfDims(1, 1, 8, 1, 0, 64, 64, 1.0, layout, 0)


def _inputs(scales=None, rotations=None):
    from spfsplatv2_amd import _lib
    p = C.c_void_p(16)                       # never dereferenced: every rejection happens before a launch
    return _lib.SpfInputs(p, scales, rotations, p, p, None, p, p, p, p)


def test_cov3d_forward_rejections_before_any_launch(hip_lib):
    from spfsplatv2_amd import _lib
    cov, st = C.c_void_p(16), _lib.SpfState()
    fwd = hip_lib.spf_raster_forward_project_cov3d
    rc = fwd(C.byref(_dims()), C.byref(_inputs(scales=C.c_void_p(16))), cov, C.byref(st), 0, None)
    assert rc == -1 and b"scales and rotations must be null" in hip_lib.spf_last_error()
    rc = fwd(C.byref(_dims()), C.byref(_inputs(rotations=C.c_void_p(16))), cov, C.byref(st), 0, None)
    assert rc == -1 and b"scales and rotations must be null" in hip_lib.spf_last_error()
    for layout in (2, 3):
        rc = fwd(C.byref(_dims(layout)), C.byref(_inputs()), cov, C.byref(st), 0, None)
        assert rc == -1 and f"sh_layout {layout} is not supported".encode() in hip_lib.spf_last_error()
    rc = fwd(C.byref(_dims()), C.byref(_inputs()), None, C.byref(st), 0, None)
    assert rc == -1 and b"cov3D is null" in hip_lib.spf_last_error()
    # past the covariance checks the usual ones apply (here: the state is empty)
    rc = fwd(C.byref(_dims()), C.byref(_inputs()), cov, C.byref(st), 0, None)
    assert rc == -1 and b"state pointer" in hip_lib.spf_last_error()


def test_cov3d_backward_rejections_before_any_launch(hip_lib):
    from spfsplatv2_amd import _lib
    cov, st = C.c_void_p(16), _lib.SpfState()
    bwd = hip_lib.spf_raster_backward_cov3d
    rc = bwd(C.byref(_dims()), C.byref(_inputs(scales=C.c_void_p(16))), cov, C.byref(st), C.byref(_lib.SpfGrads()),
             None, 1, 0, None)
    assert rc == -1 and b"scales and rotations must be null" in hip_lib.spf_last_error()
    for field in ("dL_dscales", "dL_drotations"):
        g = _lib.SpfGrads()
        setattr(g, field, C.c_void_p(16))
        rc = bwd(C.byref(_dims()), C.byref(_inputs()), cov, C.byref(st), C.byref(g), None, 1, 0, None)
        assert rc == -1 and b"dL_dscales and dL_drotations must be null" in hip_lib.spf_last_error(), field
    for layout in (2, 3):
        rc = bwd(C.byref(_dims(layout)), C.byref(_inputs()), cov, C.byref(st), C.byref(_lib.SpfGrads()), None, 1, 0,
                 None)
        assert rc == -1 and f"sh_layout {layout} is not supported".encode() in hip_lib.spf_last_error()
    rc = bwd(C.byref(_dims()), C.byref(_inputs()), None, C.byref(st), C.byref(_lib.SpfGrads()), None, 1, 0, None)
    assert rc == -1 and b"cov3D is null" in hip_lib.spf_last_error()


def _settings(**kw):
    import spfsplatv2_amd as spf
    return spf.GaussianRasterizationSettings(16, 16, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), 0, **kw)


def _call(G=4, **kw):
    base = dict(means3D=torch.zeros(G, 3), opacities=torch.ones(G, 1), shs=torch.zeros(G, 1, 3),
                viewmatrix=torch.eye(4))
    base.update(kw)
    return base


def test_gaussian_rasterizer_cov3ds_precomp_on_cpu_has_no_fallback(hip_lib):
    import spfsplatv2_amd as spf
    G = 4
    for cov in (torch.ones(G, 6), torch.eye(3).expand(G, 3, 3)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            spf.GaussianRasterizer(_settings())(**_call(G, cov3Ds_precomp=cov, scales=None, rotations=None))


def test_exactly_one_of_scale_rotation_pair_or_covariance(hip_lib):
    import spfsplatv2_amd as spf
    G = 4
    r = spf.GaussianRasterizer(_settings())
    with pytest.raises(Exception, match=EXCLUSIVE.replace("!", "")):        # both
        r(**_call(G, scales=torch.ones(G, 3), rotations=torch.ones(G, 4), cov3Ds_precomp=torch.ones(G, 6)))
    with pytest.raises(Exception, match=EXCLUSIVE.replace("!", "")):        # half a pair and a covariance
        r(**_call(G, scales=torch.ones(G, 3), cov3Ds_precomp=torch.ones(G, 6)))
    with pytest.raises(Exception, match=EXCLUSIVE.replace("!", "")):        # neither
        r(**_call(G))
    with pytest.raises(Exception, match="Please provide scales and rotations"):   # (the existing message: half a pair)
        r(**_call(G, scales=torch.ones(G, 3)))
    with pytest.raises(RuntimeError, match=EXCLUSIVE.replace("!", "")):
        spf.rasterize_batch(torch.zeros(1, G, 3), torch.ones(1, G, 3), None, torch.ones(1, G), torch.zeros(1, G, 1, 3),
                            None, torch.eye(4)[None, None], torch.eye(4)[None, None], torch.ones(1, 1, 2),
                            torch.zeros(3), 16, 16, 0, cov3D=torch.ones(1, G, 6))
    with pytest.raises(RuntimeError, match=EXCLUSIVE.replace("!", "")):
        spf.render_batch(torch.eye(4)[None, None], torch.eye(3)[None, None], torch.ones(1, 1), torch.ones(1, 1),
                         torch.zeros(1, G, 3), None, torch.ones(1, G, 4), torch.ones(1, G), torch.zeros(1, G, 3, 1),
                         None, torch.zeros(3), 16, 16, 0, cov3D=torch.ones(1, G, 6))


def test_render_norm_is_refused_with_covariances(hip_lib):
    import spfsplatv2_amd as spf
    G = 4
    with pytest.raises(Exception, match="render_norm"):
        spf.GaussianRasterizer(_settings(render_norm=True))(**_call(G, cov3Ds_precomp=torch.ones(G, 6)))


def test_raw_rows_and_band_split_are_refused_with_covariances(hip_lib):
    import spfsplatv2_amd as spf
    G = 4
    args = (torch.eye(4)[None, None], torch.eye(3)[None, None], torch.ones(1, 1), torch.ones(1, 1), torch.zeros(1, G, 3),
            None, None, torch.ones(1, G))
    with pytest.raises(RuntimeError, match="not supported with raw rows or band-split"):
        spf.render_batch(*args, None, None, torch.zeros(3), 16, 16, 0, raw=torch.zeros(1, G, 10),
                         sh_mask=torch.ones(1), cov3D=torch.ones(1, G, 6))
    with pytest.raises(RuntimeError, match="not supported with raw rows or band-split"):
        spf.render_batch(*args, torch.zeros(1, G, 3, 16), None, torch.zeros(3), 16, 16, 3, sh_layout="g3k",
                         shs_high=torch.zeros(1, G, 3, 9), cov3D=torch.ones(1, G, 6))


def test_fused_adapter_with_a_covariance_decoder_is_refused(hip_lib):
    from spfsplatv2_amd import adapter
    from spfsplatv2_amd import decoder as dec
    b, G = 1, 8
    d = dec.get_decoder(dec.DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True, True, True,
                                                    use_covariances=True))
    assert d.use_covariances
    # (what UnifiedGaussianAdapter(..., fuse_into_decoder=True) hands over: raw rows, no scales / rotations / harmonics)
    raw = adapter.RawGaussians(torch.zeros(b, G, 7 + 3 * 4), torch.ones(4), 1e-8)
    gs = dec.Gaussians(torch.zeros(b, G, 3), None, None, None, None, torch.ones(b, G), raw=raw)
    with pytest.raises(RuntimeError, match="fuse_into_decoder=False"):
        d(gs, torch.eye(4)[None, None], torch.eye(3)[None, None], torch.ones(1, 1), torch.ones(1, 1), (16, 16))


def test_decoder_config_default_keeps_the_scale_rotation_path():
    from spfsplatv2_amd import decoder as dec
    cfg = dec.DecoderSplattingCUDACfg("splatting_cuda", [0.0, 0.0, 0.0], True, True, True)
    assert cfg.use_covariances is False


def test_cov3d_entry_points_reject_a_null_state(hip_lib):
    from spfsplatv2_amd import _lib
    cov = C.c_void_p(16)
    rc = hip_lib.spf_raster_forward_project_cov3d(C.byref(_dims()), C.byref(_inputs()), cov, None, 0, None)
    assert rc == -1 and b"null" in hip_lib.spf_last_error()
    rc = hip_lib.spf_raster_backward_cov3d(C.byref(_dims()), C.byref(_inputs()), cov, None, C.byref(_lib.SpfGrads()),
                                           None, 1, 0, None)
    assert rc == -1 and b"null" in hip_lib.spf_last_error()


class _Stop(Exception):
    pass


def _recorder(calls):
    def fake(*a, **kw):
        calls.append((a, kw))
        raise _Stop
    return fake


def test_render_cuda_and_orthographic_pass_the_covariances_on(monkeypatch):
    """use_covariances=True hands the covariances to the rasterizer (the scale/rotation pair is dropped); without it
    they stay dead, and asking for it without covariances raises instead of falling back to the pair."""
    from spfsplatv2_amd import decoder as dec
    B, G = 2, 5
    ext, intr = torch.eye(4).expand(B, 4, 4), torch.eye(3).expand(B, 3, 3)
    near, far = torch.full((B,), 0.5), torch.full((B,), 50.0)
    means, cov = torch.zeros(B, G, 3), torch.eye(3).expand(B, G, 3, 3)
    harm, opac, rot, scl = torch.zeros(B, G, 3, 1), torch.ones(B, G), torch.ones(B, G, 4), torch.ones(B, G, 3)
    bg = torch.zeros(B, 3)
    for flag in (False, True):
        calls = []
        monkeypatch.setattr(dec, "render_batch", _recorder(calls))
        with pytest.raises(_Stop):
            dec.render_cuda(ext, intr, near, far, (8, 8), bg, means, cov, harm, opac, rot, scl, use_covariances=flag)
        a, kw = calls[0]
        assert (kw.get("cov3D") is cov) == flag and (a[5] is None) == flag and (a[6] is None) == flag
        calls = []
        monkeypatch.setattr(dec, "rasterize_batch", _recorder(calls))
        with pytest.raises(_Stop):
            dec.render_cuda_orthographic(ext, torch.ones(B), torch.ones(B), near, far, (8, 8), bg, means, cov, harm,
                                         opac, rot, scl, use_covariances=flag)
        a, kw = calls[0]
        assert (kw.get("cov3D") is cov) == flag and (a[1] is None) == flag and (a[2] is None) == flag
    with pytest.raises(RuntimeError, match="use_covariances needs gaussian_covariances"):
        dec.render_cuda_orthographic(ext, torch.ones(B), torch.ones(B), near, far, (8, 8), bg, means, None, harm, opac,
                                     rot, scl, use_covariances=True)
    with pytest.raises(RuntimeError, match="use_covariances needs gaussian_covariances"):
        dec.render_cuda(ext, intr, near, far, (8, 8), bg, means, None, harm, opac, rot, scl, use_covariances=True)
