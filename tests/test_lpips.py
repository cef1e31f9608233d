"""LPIPS without a GPU: the oracle against a second restatement that shares no code with it, the weight loader and its
errors, the two weight packs, the surface (argument errors before any device is touched), the C ABI, and the compiled
convolution kernel's resource report."""
import ctypes as C
import importlib
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_oracle as lo


# ---- 1. the oracle against a second restatement --------------------------------------------------------------------
def _conv_unfold(x, w, b):
    """3x3 convolution as explicit zero padding + unfold + matmul, ReLU."""
    n, c, h, wd = x.shape
    xp = torch.zeros(n, c, h + 2, wd + 2, dtype=x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    cols = xp.unfold(2, 3, 1).unfold(3, 3, 1)                       # [n, c, h, w, 3, 3]
    cols = cols.permute(0, 2, 3, 1, 4, 5).reshape(n, h, wd, c * 9)
    y = cols @ w.reshape(w.shape[0], -1).t() + b
    return y.clamp_min(0).permute(0, 3, 1, 2)


def _pool_loops(x):
    h, w = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * h, :2 * w]
    return torch.maximum(torch.maximum(x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2]),
                         torch.maximum(x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]))


def _second_lpips(in0, in1, sd, normalize):
    dt = torch.float64
    total = 0
    feats = []
    for x in (in0.to(dt), in1.to(dt)):
        if normalize:
            x = x * 2 - 1
        shift, scale = sd["scaling_layer.shift"].reshape(3).tolist(), sd["scaling_layer.scale"].reshape(3).tolist()
        h = torch.stack([(x[:, c] - shift[c]) / scale[c] for c in range(3)], 1)
        taps = []
        for l, (i, s) in enumerate(zip(lo.CONV_INDEX, lo.SLICE)):
            if l in (2, 4, 7, 10):
                h = _pool_loops(h)
            h = _conv_unfold(h, sd[f"net.slice{s}.{i}.weight"].to(dt), sd[f"net.slice{s}.{i}.bias"].to(dt))
            if l in lo.TAPS:
                taps.append(h)
        feats.append(taps)
    for k, (a, b) in enumerate(zip(*feats)):
        na = a.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
        nb = b.pow(2).sum(1, keepdim=True).sqrt() + 1e-10
        lin = sd[f"lin{k}.model.1.weight"].to(dt)
        total = total + (lin * (a / na - b / nb).pow(2)).sum(1).flatten(1).mean(1)
    return total


@pytest.mark.parametrize("normalize", [True, False])
def test_oracle_against_second_restatement(normalize):
    sd = lo.make_weights(3)
    pred, target = lo.image_pair(5, (2, 3, 19, 35))
    a = lo.lpips(pred, target, sd, normalize, torch.float64).reshape(-1)
    b = _second_lpips(pred, target, sd, normalize)
    assert a.shape == (2,) and bool((a > 1e-4).all())
    assert float(((a - b).abs() / b.abs()).max()) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_oracle_pool_is_max_pool2d_first_maximum(dtype):
    g = torch.Generator().manual_seed(1)
    x = torch.relu(torch.randn(2, 8, 7, 9, generator=g, dtype=dtype))       # windows of four zeros among them
    x[0, :, 0:2, 0:2] = 0.75
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    up = torch.randn(2, 8, 3, 4, generator=g, dtype=dtype)
    assert torch.equal(lo.pool(a), F.max_pool2d(b, 2, 2))
    assert torch.equal(torch.autograd.grad(lo.pool(a), a, up)[0], torch.autograd.grad(F.max_pool2d(b, 2, 2), b, up)[0])


def _head_backward_by_hand(a, b, lin, up):
    """dL/da, dL/db of sum_n up[n] head_term(a, b, lin)[n], written out; the 1 / ||a|| term is 0 where ||a|| = 0."""
    hw = a.shape[2] * a.shape[3]
    na, nb = a.pow(2).sum(1, keepdim=True).sqrt(), b.pow(2).sum(1, keepdim=True).sqrt()
    da, db = na + 1e-10, nb + 1e-10
    g = 2 * lin * (a / da - b / db) * (up.reshape(-1, 1, 1, 1) / hw)
    ka = torch.where(na > 0, (g * a).sum(1, keepdim=True) / (da * da * torch.where(na > 0, na, torch.ones_like(na))),
                     torch.zeros_like(na))
    kb = torch.where(nb > 0, (g * b).sum(1, keepdim=True) / (db * db * torch.where(nb > 0, nb, torch.ones_like(nb))),
                     torch.zeros_like(nb))
    return g / da - ka * a, kb * b - g / db


def test_oracle_head_backward_against_hand_written():
    g = torch.Generator().manual_seed(0)
    a = torch.relu(torch.randn(3, 64, 5, 7, generator=g, dtype=torch.float64))
    b = torch.relu(torch.randn(3, 64, 5, 7, generator=g, dtype=torch.float64))
    a[0, :, 1, 2] = 0                                   # all-zero vectors: in one image, and in both
    a[1, :, 3, 3] = 0
    b[1, :, 3, 3] = 0
    lin = torch.rand(1, 64, 1, 1, generator=g, dtype=torch.float64) / 32
    up = torch.linspace(0.5, 1.5, 3, dtype=torch.float64)
    x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ga, gb = torch.autograd.grad(lo.head_term(x, y, lin), [x, y], up)
    ha, hb = _head_backward_by_hand(a, b, lin, up)
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all())
    for got, want in ((ga, ha), (gb, hb)):
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-12


# ---- 2. the loader -----------------------------------------------------------------------------------------------------
def _same(w, sd):
    convs, lins, shift, scale = lo.params(sd, torch.float32)
    return (all(torch.equal(a, b[0]) and torch.equal(c, b[1]) for a, c, b in zip(w.conv_w, w.conv_b, convs))
            and all(torch.equal(a, b.reshape(-1)) for a, b in zip(w.lin, lins))
            and torch.equal(w.shift, shift.reshape(-1)) and torch.equal(w.scale, scale.reshape(-1)))


def test_loader_lpips_keys_and_both_lin_spellings(tmp_path, monkeypatch):
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    sd = lo.make_weights(1)
    assert _same(lp.LpipsWeights.from_state_dict(sd), sd)
    both = dict(sd)
    for k in range(5):                                  # the package's state dict names every lin layer twice
        both[f"lins.{k}.model.1.weight"] = sd[f"lin{k}.model.1.weight"].clone()
    assert _same(lp.resolve_weights(both), sd)
    only_lins = {k.replace("lin", "lins.", 1) if k.startswith("lin") else k: v for k, v in sd.items()}
    assert "lins.3.model.1.weight" in only_lins and _same(lp.LpipsWeights.from_state_dict(only_lins), sd)
    path = tmp_path / "w.pt"
    torch.save(sd, path)
    assert _same(lp.resolve_weights(str(path)), sd)
    monkeypatch.setenv("SPF_LPIPS_WEIGHTS", str(path))
    assert _same(lp.resolve_weights(None), sd)
    w = lp.LpipsWeights.from_state_dict(sd)
    assert lp.resolve_weights(w) is w

    class Holder(torch.nn.Module):
        def state_dict(self, *a, **k):
            return sd
    assert _same(lp.LpipsWeights.from_module(Holder()), sd)


def test_loader_torchvision_keys_with_separate_lin_dict_and_default_scaling():
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    sd = lo.make_weights(2, scaling=False)
    for prefix in ("features.", ""):
        vgg = {f"{prefix}{i}.{what}": sd[f"net.slice{s}.{i}.{what}"] for i, s in zip(lo.CONV_INDEX, lo.SLICE)
               for what in ("weight", "bias")}
        vgg["classifier.0.weight"] = torch.zeros(8, 8)             # a whole vgg16 state dict: ignored
        vgg["classifier.0.bias"] = torch.zeros(8)
        lin = {k: v for k, v in sd.items() if k.startswith("lin")}
        w = lp.resolve_weights((vgg, lin))
        assert _same(w, sd)
        assert w.shift.tolist() == pytest.approx(list(lo.SHIFT)) and w.scale.tolist() == pytest.approx(list(lo.SCALE))


def test_loader_errors(monkeypatch):
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    sd = lo.make_weights(1)
    missing = {k: v for k, v in sd.items() if k != "net.slice3.12.bias"}
    with pytest.raises(KeyError) as e:
        lp.LpipsWeights.from_state_dict(missing)
    assert "missing <prefix>.12.bias" in str(e.value) and "keys found" in str(e.value) and "keys wanted" in str(e.value)
    wrong = dict(sd)
    wrong["net.slice2.7.weight"] = torch.zeros(128, 64, 3, 3)
    with pytest.raises(KeyError, match=r"net\.slice2\.7\.weight has shape \(128, 64, 3, 3\)"):
        lp.LpipsWeights.from_state_dict(wrong)
    nolin = {k: v for k, v in sd.items() if k != "lin4.model.1.weight"}
    with pytest.raises(KeyError, match="missing lin4"):
        lp.LpipsWeights.from_state_dict(nolin)
    twice = dict(sd)
    twice["other.0.weight"] = sd["net.slice1.0.weight"] + 1
    with pytest.raises(KeyError, match="differ"):
        lp.LpipsWeights.from_state_dict(twice)
    monkeypatch.delenv("SPF_LPIPS_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError) as e:
        lp.resolve_weights(None)
    assert 'torch.save(lpips.LPIPS(net="vgg").state_dict(), "lpips_vgg.pt")' in str(e.value)


def test_library_imports_neither_lpips_nor_torchvision():
    import sys

    import spfsplatv2_amd  # noqa: F401
    src = "".join(p.read_text() for p in (__import__("tests.conftest").conftest.ROOT / "spfsplatv2_amd").glob("*.py"))
    assert not re.search(r"^\s*(import|from)\s+(lpips|torchvision)\b", src, re.M)
    assert "lpips" not in sys.modules or sys.modules["lpips"].__name__.startswith("spfsplatv2_amd")


# ---- 3. the two packs ------------------------------------------------------------------------------------------------
def test_forward_pack_unpacks_to_the_weights():
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    sd = lo.make_weights(4)
    w = lp.LpipsWeights.from_state_dict(sd)
    pack = w.forward_pack()
    assert pack.numel() == lp.PACK_SIZE == sum(9 * a * b for a, b in zip(lo.CIN, lo.COUT))
    for got, want in zip(lp.LpipsWeights.unpack_forward(pack), w.conv_w):
        assert torch.equal(got, want)
    # the layout the kernels index: [tap = 3 dy + dx][c_in][c_out]
    l, o = 2, lp.PACK_OFFSET[2]
    assert float(pack[o + ((3 * 2 + 1) * 64 + 5) * 128 + 7]) == float(w.conv_w[l][7, 5, 2, 1])


@pytest.mark.parametrize("layer", [0, 1, 2, 7])
def test_backward_pack_is_the_input_gradient_of_conv2d(layer):
    """The backward pack, unpacked and run through the oracle's convolution, equals autograd's input gradient of
    F.conv2d in float64: pins the 180-degree rotation and the channel swap."""
    lp = importlib.import_module("spfsplatv2_amd.lpips")
    w = lp.LpipsWeights.from_state_dict(lo.make_weights(6))
    wb = lp.LpipsWeights.unpack_backward(w.backward_pack())[layer].double()
    assert wb.shape == (lo.CIN[layer], lo.COUT[layer], 3, 3)
    g = torch.Generator().manual_seed(layer)
    x = torch.randn(1, lo.CIN[layer], 6, 9, generator=g, dtype=torch.float64, requires_grad=True)
    up = torch.randn(1, lo.COUT[layer], 6, 9, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad(F.conv2d(x, w.conv_w[layer].double(), padding=1), x, up)
    got = lo.conv(up, wb, None, relu=False)
    assert float((got - want).abs().max() / want.abs().max()) <= 1e-12
    pack = w.backward_pack()                                     # [tap][c_out][c_in], taps rotated
    o = lp.PACK_OFFSET[layer]
    ci, co = lo.CIN[layer], lo.COUT[layer]
    assert float(pack[o + ((3 * 0 + 1) * co + 3) * ci + 2]) == float(w.conv_w[layer][3, 2, 2, 1])


# ---- 4. the surface --------------------------------------------------------------------------------------------------
def test_api_errors_before_any_device(monkeypatch):
    import spfsplatv2_amd as spf
    monkeypatch.delenv("SPF_LPIPS_WEIGHTS", raising=False)
    x = torch.rand(2, 3, 32, 32)
    for call in (lambda: spf.lpips(x, x), lambda: spf.LPIPS()(x, x), lambda: spf.compute_lpips(x, x),
                 lambda: spf.LossLpips(spf.LossLpipsCfgWrapper(spf.LossLpipsCfg(1.0, 0)))(x[None], x[None], None, 0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="3 channels"):
        spf.lpips(torch.rand(2, 4, 32, 32), torch.rand(2, 4, 32, 32))
    with pytest.raises(ValueError, match="shorter than 16"):
        spf.lpips(torch.rand(2, 3, 15, 32), torch.rand(2, 3, 15, 32))
    with pytest.raises(ValueError, match="differ in shape"):
        spf.lpips(x, torch.rand(2, 3, 32, 33))
    with pytest.raises(ValueError, match="differ in shape"):
        spf.compute_lpips(x, torch.rand(1, 3, 32, 32))
    with pytest.raises(NotImplementedError, match="alex"):
        spf.LPIPS(net="alex")
    with pytest.raises(NotImplementedError, match="spatial"):
        spf.LPIPS(spatial=True)
    with pytest.raises(NotImplementedError, match="retPerLayer"):
        spf.LPIPS()(x, x, retPerLayer=True)


def test_loss_lpips_surface(monkeypatch):
    import dataclasses

    import spfsplatv2_amd as spf
    monkeypatch.delenv("SPF_LPIPS_WEIGHTS", raising=False)
    assert [f.name for f in dataclasses.fields(spf.LossLpipsCfgWrapper)] == ["lpips"]
    assert [f.name for f in dataclasses.fields(spf.LossLpipsCfg)] == ["weight", "apply_after_step"]
    loss = spf.LossLpips(spf.LossLpipsCfgWrapper(spf.LossLpipsCfg(0.05, 100)))       # needs no weights
    assert loss.name == "lpips"
    x = torch.rand(1, 2, 3, 32, 32)
    out = loss(x, x, None, 99)                          # before apply_after_step: 0, no weights, no device
    assert out.shape == () and out.dtype == torch.float32 and float(out) == 0.0
    for name in ("LossLpips", "LossLpipsCfg", "LossLpipsCfgWrapper", "lpips", "LPIPS", "LpipsWeights", "compute_lpips"):
        assert name in spf.__all__ and hasattr(spf, name)


# ---- 5. the C ABI ----------------------------------------------------------------------------------------------------
def test_abi_struct_and_workspace(hip_lib):
    from spfsplatv2_amd import _lib
    assert C.sizeof(_lib.SpfLpips) == 96 and _lib.SpfLpips.wfwd.offset == 56 and _lib.SpfLpips.N.offset == 32
    wb = hip_lib.spf_lpips_workspace_bytes

    def floats(n_grad, n_total, h, w):
        """The layout of csrc/lpips.hip restated: 13 activations, one pooled map, head partials, tap gradients and two
        gradient buffers, each rounded up to 64 floats."""
        def up(v):
            return (v + 63) // 64 * 64
        hs, ws = [h >> k for k in range(5)], [w >> k for k in range(5)]
        lev = (0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4)
        o = sum(up(n_total * hs[k] * ws[k] * c) for k, c in zip(lev, lo.COUT))
        o += up(n_total * hs[1] * ws[1] * 64)
        o += sum(up(n_total // 2 * ((hs[k] * ws[k] + 63) // 64)) for k in range(5))
        o += sum(up(n_grad * hs[k] * ws[k] * c) for k, c in enumerate(lo.TAP_C))
        return o + 2 * up(n_grad * h * w * 64)
    for args in ((0, 2, 16, 16), (1, 2, 16, 16), (16, 32, 256, 256), (0, 6, 33, 47), (6, 6, 33, 47), (2, 4, 224, 224)):
        assert wb(*args) == 4 * floats(*args), args
    assert wb(16, 32, 256, 256) > wb(0, 32, 256, 256)
    for bad in ((0, 2, 15, 16), (0, 2, 16, 8), (0, 3, 32, 32), (0, 0, 32, 32), (1, 4, 32, 32), (-1, 2, 32, 32)):
        assert wb(*bad) == -1, bad


def test_abi_rejects_invalid_arguments_before_any_launch(hip_lib):
    from spfsplatv2_amd import _lib
    p = C.c_void_p(64)

    def args(**kw):
        base = dict(in0=p, in1=p, stride0=3 * 32 * 32, stride1=3 * 32 * 32, N=1, H=32, W=32, normalize=1, weight=1.0,
                    reserved=0, wfwd=p, wbwd=p, bias=p, lin=p, shift_scale=p)
        base.update(kw)
        return _lib.SpfLpips(*[base[f[0]] for f in _lib.SpfLpips._fields_])
    fwd, bwd = hip_lib.spf_lpips_forward, hip_lib.spf_lpips_backward
    assert fwd(None, p, p, None, None) == -1 and b"null" in hip_lib.spf_last_error()
    assert fwd(C.byref(args(H=15)), p, p, None, None) == -1 and b"shorter than 16" in hip_lib.spf_last_error()
    assert fwd(C.byref(args(N=0)), p, p, None, None) == -1
    assert fwd(C.byref(args(in1=None)), p, p, None, None) == -1 and b"null image" in hip_lib.spf_last_error()
    assert fwd(C.byref(args(stride0=100)), p, p, None, None) == -1 and b"stride" in hip_lib.spf_last_error()
    assert fwd(C.byref(args(lin=None)), p, p, None, None) == -1 and b"weight pointer" in hip_lib.spf_last_error()
    assert fwd(C.byref(args(wfwd=C.c_void_p(68))), p, p, None, None) == -1 and b"aligned" in hip_lib.spf_last_error()
    assert fwd(C.byref(args()), None, p, None, None) == -1
    assert fwd(C.byref(args()), C.c_void_p(68), p, None, None) == -1 and b"aligned" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, p, 0, None, None, None) == -1 and b"no gradient" in hip_lib.spf_last_error()
    assert bwd(C.byref(args()), p, None, 0, p, None, None) == -1
    assert hip_lib.spf_lpips_conv3x3(p, None, p, None, p, 1, 8, 8, 24, 64, 1, None) == -1
    assert b"multiple of 16" in hip_lib.spf_last_error()
    assert hip_lib.spf_lpips_conv3x3(p, None, p, None, p, 1, 8, 8, 64, 96, 1, None) == -1
    assert hip_lib.spf_lpips_conv3x3(p, None, None, None, p, 1, 8, 8, 64, 64, 1, None) == -1
    assert hip_lib.spf_lpips_pool_forward(p, p, 1, 8, 8, 6, None) == -1
    assert hip_lib.spf_lpips_pool_backward(p, None, p, 1, 8, 8, 64, None) == -1
    assert hip_lib.spf_lpips_head_forward(p, p, p, 1, 16, 100, p, p, None) == -1 and b"64, 128" in hip_lib.spf_last_error()
    assert hip_lib.spf_lpips_head_backward(p, p, p, 1, 16, 64, p, None, None, None) == -1
    assert hip_lib.spf_lpips_conv1_forward(C.byref(args()), None, None) == -1
    assert hip_lib.spf_lpips_conv1_backward(C.byref(args()), p, p, None, None) == -1


# ---- 6. the compiled convolution kernel ---------------------------------------------------------------------------------
def test_conv_kernel_issues_f32_mfma_and_no_kernel_uses_scratch(tmp_path):
    """Cross-compile csrc/lpips.hip to assembly with the build's flags: the convolution kernel issues
    v_mfma_f32_32x32x2_f32, and the resource report shows no scratch for any kernel of the file."""
    from spfsplatv2_amd import build
    asm = tmp_path / "lpips.s"
    r = subprocess.run([build._hipcc(), *build.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                        str(build.CSRC / "lpips.hip"), "-o", str(asm)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(names) == len(scratch) >= 10 and any("spf_lpips_conv_kernel" in n for n in names)
    assert all(v == 0 for v in scratch), dict(zip(names, scratch))
    text = asm.read_text()
    bodies = re.findall(r"^(_ZN3spf21spf_lpips_conv_kernel\w+):[^\n]*\n(.*?)\n\s*s_endpgm", text, re.S | re.M)
    assert len(bodies) == 2, [b[0] for b in bodies]
    for name, body in bodies:
        assert body.count("v_mfma_f32_32x32x2_f32") >= 16, name
        assert "scratch_" not in body, name
