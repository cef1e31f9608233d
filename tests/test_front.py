"""The encoder front without a device (spfsplatv2_amd/front.py, csrc/front.hip): exports, refusals, the oracle against the
reference's goldens, the power condition of the gate on every case, the chunk helper's arithmetic.

Gate and power condition: tests/front_cases.py.  Here the yardstick is float32 eager torch on the CPU.
"""
import re

import pytest
import torch

from tests import front_cases as cases
from tests import front_oracle as fo

SYMBOLS = ("spf_front_geometry", "spf_front_workspace_floats", "spf_front_embed_forward", "spf_front_assemble",
           "spf_front_tokens_backward", "spf_front_embed_backward")


# ---- exports ---------------------------------------------------------------------------------------------------------
def test_exports_and_header_symbols(hip_lib):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import _lib, build
    for name in ("embed_patches", "assemble_tokens", "PatchEmbedDust3R", "VGGTPatchEmbed", "prepare_tokens"):
        assert name in spf.__all__ and callable(getattr(spf, name)), name
    header = build.HEADERS[1].read_text()
    for name in SYMBOLS:
        assert name in _lib.SYMBOLS and re.search(rf"\b{name}\(", header) and hasattr(hip_lib, name), name
    assert "front.hip" in build.SOURCES
    assert int(re.search(r"#define SPF_FRONT_MAX_TOKENS (\d+)", header).group(1)) == _lib.FRONT_MAX_TOKENS


def test_chunk_helper_arithmetic(hip_lib):
    """The chunk height is a multiple of the reduction step that never changes below ``chunks x height`` rows, the chunks
    cover M exactly once, and their number is bounded (the workspace is chunks x C x K floats)."""
    from spfsplatv2_amd import front
    assert front.tile_rows() > 0 and front.tile_cols() > 0 and front.tile_cols() % 32 == 0
    h0 = front.chunk_rows(1)
    most = max(front.chunks(m) for m in (1, h0, 10 ** 4, 10 ** 6, 2 ** 31 - 1))
    for m in (1, 2, h0 - 1, h0, h0 + 1, 3 * h0, 3 * h0 + 1, most * h0, most * h0 + 1, 12288, 10 ** 6 + 7, 2 ** 31 - 1):
        h, n = front.chunk_rows(m), front.chunks(m)
        assert h >= h0 and h % 16 == 0 and 1 <= n <= most
        assert (n - 1) * h < m <= n * h, (m, h, n)
        if m <= most * h0:
            assert h == h0
    assert front.chunks(h0 + 1) == 2 and front.chunks(3 * h0 + 1) == 4
    assert hip_lib.spf_front_geometry(99, 5) == -1


# ---- refusals --------------------------------------------------------------------------------------------------------
def _ops(p=16, c_in=3, c=64, b=2, gh=2, gw=3):
    return torch.rand(b, c_in, gh * p, gw * p), torch.randn(c, c_in, p, p), torch.randn(c)


def test_refusals_without_a_device():
    import spfsplatv2_amd as spf
    image, weight, bias = _ops()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.embed_patches(image, weight, bias, patch=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.assemble_tokens(torch.randn(2, 5, 64), after=[torch.randn(1, 1, 64)])
    with pytest.raises(NotImplementedError, match="gradient to the image"):
        spf.embed_patches(image.clone().requires_grad_(True), weight, bias, patch=16)
    for p in (8, 32, (16, 14)):
        with pytest.raises(NotImplementedError, match="patch"):
            spf.embed_patches(image, weight, bias, patch=p)
    for dt in (torch.float16, torch.bfloat16):
        with pytest.raises(NotImplementedError, match="float32"):
            spf.embed_patches(image.to(dt), weight.to(dt), bias.to(dt), patch=16)
    with pytest.raises(RuntimeError, match="dtype"):
        spf.embed_patches(image.double(), weight.double(), bias.double(), patch=16)
    # a misaligned image: one float off a 16-byte boundary, and a row stride that is no multiple of 4 floats
    buf = torch.rand(image.numel() + 1)
    with pytest.raises(RuntimeError, match="read in place"):
        spf.embed_patches(buf[1:].view(image.shape), weight, bias, patch=16)
    wide = torch.rand(2, 3, 32, 50)
    with pytest.raises(RuntimeError, match="read in place"):
        spf.embed_patches(wide[..., :48], weight, bias, patch=16)
    with pytest.raises(RuntimeError, match="read in place"):
        spf.embed_patches(image.transpose(2, 3).contiguous().transpose(2, 3)[:, :, :32, :32], weight, bias, patch=16)
    with pytest.raises(ValueError, match="multiple of 4"):
        spf.embed_patches(image, torch.randn(66, 3, 16, 16), torch.randn(66), patch=16)
    with pytest.raises(ValueError, match="C_in"):
        spf.embed_patches(torch.rand(1, 33, 16, 16), torch.randn(64, 33, 16, 16), None, patch=16)
    with pytest.raises(RuntimeError, match="multiples of the patch size"):
        spf.embed_patches(torch.rand(2, 3, 32, 40), weight, bias, patch=16)
    with pytest.raises(RuntimeError, match="must be \\[1, k, 64\\]"):
        spf.embed_patches(image, weight, bias, patch=16, after=[torch.randn(3, 1, 64)])
    with pytest.raises(ValueError, match="pos_first"):
        spf.embed_patches(image, weight, bias, patch=16, pos_first=torch.randn(64))
    with pytest.raises(ValueError, match="mean and std"):
        spf.embed_patches(image, weight, bias, patch=16, mean=(0.5,) * 3)
    with pytest.raises(ValueError, match="non-zero"):
        spf.embed_patches(image, weight, bias, patch=16, mean=(0.5,) * 3, std=(0.5, 0.0, 0.5))


def test_module_refusals_without_a_device():
    import spfsplatv2_amd as spf
    from torch import nn
    for cls in (spf.PatchEmbedDust3R, spf.VGGTPatchEmbed):
        with pytest.raises(NotImplementedError, match="norm_layer"):
            cls(32, 16, 3, 64, norm_layer=nn.LayerNorm)
        with pytest.raises(NotImplementedError, match="patch"):
            cls(32, 8, 3, 64)
    mod = spf.PatchEmbedDust3R((32, 48), 16, 3, 64)
    image = torch.rand(2, 3, 32, 48)
    with pytest.raises(NotImplementedError, match="portrait"):
        mod(image, true_shape=torch.tensor([[32, 48], [48, 32]]))
    with pytest.raises(NotImplementedError, match="portrait"):
        mod(image, true_shape=[(32, 48), (48, 32)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mod(image, true_shape=[(32, 48), (32, 48)])
    vp = spf.VGGTPatchEmbed((28, 42), 14, 3, 64)
    cls_token, pos_embed = torch.randn(1, 1, 64), torch.randn(1, 26, 64)
    with pytest.raises(NotImplementedError, match="masks"):
        spf.prepare_tokens(torch.rand(2, 3, 28, 42), vp, cls_token, pos_embed, masks=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spf.prepare_tokens(torch.rand(2, 3, 28, 42), vp, cls_token, pos_embed, torch.randn(1, 4, 64))


# ---- the oracle against the reference --------------------------------------------------------------------------------
def _close(label, x, ref, tol=1e-5):
    e = fo.rel_err(x, ref)
    print(f"{label}: {e:.3e}")
    assert x.shape == ref.shape and e <= tol, (label, e)


def test_oracle_against_the_reference_goldens(golden_dir):
    """The float64 oracle on the goldens' operands against the reference's own float32 outputs and gradients (1e-5: the
    gate's cap, five times what eager float32 loses on these sums)."""
    import spfsplatv2_amd as spf
    g = cases.goldens(golden_dir)
    mean, std = g["mean"], g["std"]
    f64 = lambda t: t.double().requires_grad_(True)       # noqa: E731

    for key, patch in (("dust3r", 16), ("vggt_patch", 14)):
        r = g[key]
        mod = (spf.PatchEmbedDust3R if key == "dust3r" else spf.VGGTPatchEmbed)(*r["args"])
        mod.load_state_dict(r["state"], strict=True)        # the reference's keys load unchanged
        w, b = f64(mod.proj.weight.detach()), f64(mod.proj.bias.detach())
        out = fo.embed(r["image"].double(), w, b, patch, mean, std)
        _close(f"{key} tokens", out, r["tokens"])
        gw, gb = torch.autograd.grad((out * r["up"].double()).sum(), (w, b))
        _close(f"{key} d proj.weight", gw, r["grads"]["proj.weight"])
        _close(f"{key} d proj.bias", gb, r["grads"]["proj.bias"])
    # the encoder's appends
    r, e = g["dust3r"], g["encode_image"]
    w, b = r["state"]["proj.weight"].double(), f64(r["state"]["proj.bias"])
    intr, pose = f64(e["intrinsics_embed"]), f64(e["pose_embedding"])
    out = fo.embed(r["image"].double(), w, b, 16, mean, std, after=[intr, pose])
    _close("encode_image tokens", out, e["tokens"])
    for t, k in zip(torch.autograd.grad((out * e["up"].double()).sum(), (b, intr, pose)),
                    ("proj.bias", "intrinsics_embed", "pose_embedding")):
        _close(f"encode_image d {k}", t, e["grads"][k])
    # the decoder's appends
    d = g["decoder"]
    feat, intr, pose = f64(d["feat"]), f64(d["intrinsics_embed"]), f64(d["pose_embedding"])
    out = fo.assemble(feat, after=[intr, pose.reshape(1, 1, -1)])
    _close("decoder tokens", out, d["tokens"], 0.0)
    for t, k in zip(torch.autograd.grad((out * d["up"].double()).sum(), (feat, intr, pose)),
                    ("feat", "intrinsics_embed", "pose_embedding")):
        _close(f"decoder d {k}", t, d["grads"][k])
    # prepare_tokens_with_masks
    from spfsplatv2_amd import front
    v, dn = g["vggt_patch"], g["dino"]
    for name in ("plain", "intrinsics"):
        r = dn[name]
        leaves = {k: f64(t) for k, t in dn["state"].items()}
        leaves["patch_embed.proj.bias"] = f64(v["state"]["proj.bias"])
        if r["intrinsic_embedding"] is not None:
            leaves["intrinsic_embedding"] = f64(r["intrinsic_embedding"])
        first, rows = front.interpolate_pos_embed(leaves["pos_embed"], 28, 42, 14, dn["cfg"]["interpolate_antialias"],
                                                  dn["cfg"]["interpolate_offset"])
        before = [leaves["cls_token"]] + ([leaves["intrinsic_embedding"]] if "intrinsic_embedding" in leaves else [])
        out = fo.embed(dn["image"].double(), v["state"]["proj.weight"].double(), leaves["patch_embed.proj.bias"], 14, mean,
                       std, pos_table=rows, pos_first=first, before=before + [leaves["register_tokens"]])
        _close(f"dino {name} tokens", out, r["tokens"])
        assert set(r["grads"]) == set(leaves)
        for t, k in zip(torch.autograd.grad((out * r["up"].double()).sum(), list(leaves.values())), leaves):
            _close(f"dino {name} d {k}", t, r["grads"][k])


def test_positions_bit_exact(golden_dir):
    from spfsplatv2_amd import PositionGetter, append_token_position
    g = cases.goldens(golden_dir)
    pos = PositionGetter()(2, 2, 3, "cpu")
    assert torch.equal(pos, g["dust3r"]["pos"]) and pos.dtype == torch.int64
    assert torch.equal(append_token_position(append_token_position(pos)), g["encode_image"]["pos"])
    d = g["decoder"]
    assert torch.equal(append_token_position(append_token_position(d["pos_in"])), d["pos"])


def test_oracle_is_the_convolution():
    """The explicit patch matrix of the oracle against ``conv2d`` in float64, both patch sizes."""
    for case in (cases.COVER[2], cases.COVER[9]):
        d = cases.operands(case)
        a, b = cases.oracle(case, d), cases.run(fo.eager_embed, case, d, torch.float64)
        for k in a:
            assert fo.rel_err(a[k], b[k]) < 1e-13, (case, k)


# ---- the power condition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.COVER, ids=cases.case_id)
def test_power_condition(case):
    """Every mutant of the case moves every tensor it reaches by at least 4 bounds, with eager float32 on the CPU as the
    yardstick -- and eager itself passes the gate."""
    d, x64, dists = cases.reference(case)
    assert set(dists) == set(cases.mutants_of(case)) and len(dists) >= 5
    e = cases.eager(case, d)
    cases.gate(cases.case_id(case) + " (eager on the CPU as the product)", e, e, x64, dists)


def test_every_mutant_is_exercised():
    seen = set()
    for case in cases.COVER:
        seen |= set(cases.mutants_of(case))
    assert seen == set(fo.MUTANTS)


def test_power_condition_of_assemble_tokens():
    d = cases.assemble_operands()

    def run(dtype, mut=fo.NONE):
        leaves = {k: d[k].to(dtype).requires_grad_(True) for k in ("x", "intr", "pose")}
        out = fo.assemble(leaves["x"], after=[leaves["intr"], leaves["pose"]], mut=mut)
        return cases.with_grads(out, d["up"].to(dtype), leaves)
    x64, e = run(torch.float64), run(torch.float32)
    dists = {"after_front": {k: fo.rel_err(run(torch.float64, frozenset(["after_front"]))[k], x64[k]) for k in ("out", "d_x")},
             "mean_grad": {"d_pose": fo.rel_err(run(torch.float64, frozenset(["mean_grad"]))["d_pose"], x64["d_pose"])}}
    cases.gate("assemble_tokens (eager on the CPU as the product)", e, e, x64, dists)
