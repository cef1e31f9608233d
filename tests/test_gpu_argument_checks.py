"""The argument checks every entry point of the rasterizer shares (rasterizer._check_camera / _check_gaussians /
_check_sh): one wording whichever way a call comes in, and the coefficient count of raw rows held against the degree that
will really be evaluated."""
import pytest
import torch

from tests import util

pytestmark = pytest.mark.gpu


def _scene(S, V, G, K, seed=5):
    """Cameras at the origin looking down +z, G Gaussians two to three units in front of them; raw rows [S,G,7+3K]."""
    gen = torch.Generator().manual_seed(seed)
    means = torch.cat([torch.rand(S, G, 2, generator=gen) - 0.5, 2.0 + torch.rand(S, G, 1, generator=gen)], dim=-1)
    intr = torch.tensor([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, 1.0]])
    raw = torch.randn(S, G, 7 + 3 * K, generator=gen)
    raw[..., :3] += 8.0                                           # (softplus -> scales near the adapter's 0.3 clamp)
    cam = dict(extrinsics=torch.eye(4).expand(S, V, 4, 4).contiguous(), intrinsics=intr.expand(S, V, 3, 3).contiguous(),
               near=torch.full((S, V), 0.1), far=torch.full((S, V), 100.0))
    rest = dict(means=means, opacities=torch.full((S, G), 0.8), raw=raw, sh_mask=torch.ones(K), bg=torch.zeros(3))
    return {k: v.cuda() for k, v in {**cam, **rest}.items()}


def _render_raw(sc, sh_degree, **kw):
    import spfsplatv2_amd as spf
    return spf.render_batch(sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"], sc["means"], None, None,
                            sc["opacities"], None, None, sc["bg"], 16, 16, sh_degree, raw=sc["raw"], sh_mask=sc["sh_mask"],
                            **kw)


def test_raw_rows_too_short_for_band4_are_refused_before_any_launch(hip_lib, monkeypatch):
    """SPF_SH_BAND4=1, sh_degree 4, sh_band4 left to the default: the default is resolved BEFORE the coefficient count is
    checked, so 16-coefficient raw rows are refused by the Python check (not by the C API, after the camera kernel), and
    25-coefficient rows render."""
    from spfsplatv2_amd import _lib
    from spfsplatv2_amd import rasterizer as rz
    monkeypatch.setenv("SPF_SH_BAND4", "1")
    launches = []
    launcher = rz._forward_impl
    monkeypatch.setattr(rz, "_forward_impl", lambda *a, **kw: launches.append(1) or launcher(*a, **kw))
    _lib.stage_timing_enable(True)
    try:
        with pytest.raises(RuntimeError, match="too few for sh_degree") as err:
            _render_raw(_scene(1, 1, 4, 16), 4, sh_band4=None)
        assert not isinstance(err.value, _lib.SpfError), err.value
        torch.cuda.synchronize()
        assert launches == [] and all(n == 0 for _, n in _lib.stage_times().values()), _lib.stage_times()
        image, depth, alpha, radii = _render_raw(_scene(1, 1, 4, 25), 4, sh_band4=None)
        torch.cuda.synchronize()
        assert launches == [1] and _lib.stage_times()["project_fwd"][1] == 1
    finally:
        _lib.stage_timing_enable(False)
    assert image.shape == (1, 1, 3, 16, 16) and bool(torch.isfinite(image).all()) and float(alpha.max()) > 0.0
    assert int((radii > 0).sum()) > 0


@pytest.mark.parametrize("name,bad,message", [
    ("intrinsics", torch.zeros(1, 2, 4, 4), "intrinsics has shape (1, 2, 4, 4), expected (1, 2, 3, 3)"),
    ("near", torch.full((2,), 0.1), "near has shape (2,), expected (1, 2)")])
def test_every_entry_point_words_a_bad_camera_block_alike(hip_lib, name, bad, message):
    """A wrong-shaped `intrinsics` / `near` through render_batch, render_batch on raw rows, camera_forward and the decoder
    module's prepared-step path (the second call of a shape under a plan with a list-length class): the same sentence."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import decoder as dec
    sc = _scene(1, 2, 8, 4)
    sc[name] = bad.cuda()
    cam = (sc["extrinsics"], sc["intrinsics"], sc["near"], sc["far"])
    scales, rotations = torch.full((1, 8, 3), 0.05).cuda(), torch.tensor([1.0, 0.0, 0.0, 0.0]).expand(1, 8, 4).contiguous().cuda()
    harmonics = torch.zeros(1, 8, 3, 4).cuda()
    said = {}

    def hear(path, call):
        with pytest.raises(RuntimeError) as err:
            call()
        said[path] = str(err.value)

    hear("render_batch", lambda: spf.render_batch(*cam, sc["means"], scales, rotations, sc["opacities"], harmonics, None,
                                                  sc["bg"], 16, 16, 1, sh_layout="g3k"))
    hear("render_batch(raw)", lambda: _render_raw(sc, 1))
    hear("camera_forward", lambda: spf.camera_forward(*cam))
    d = util.product_decoder(max_pairs=spf.PairBudget(4096, 128, "deferred"))
    prepared = []
    prepare = d._prepare_step
    d._prepare_step = lambda *a, **kw: prepared.append(1) or prepare(*a, **kw)
    g = dec.Gaussians(sc["means"], None, rotations, scales, harmonics, sc["opacities"])
    with torch.no_grad():
        hear("decoder, first call", lambda: d(g, *cam, (16, 16)))
        assert prepared == []
        hear("decoder, prepared step", lambda: d(g, *cam, (16, 16)))
    assert prepared == [1]
    assert said == dict.fromkeys(said, message) and len(said) == 5, said
