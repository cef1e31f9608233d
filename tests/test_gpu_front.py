"""The encoder front on the device (csrc/front.hip, spfsplatv2_amd/front.py).

Gate (tests/front_cases.py, rule (a) of tests/test_gpu_lpips.py): per tensor err = max|x - x64| / max|x64| against the
float64 oracle must not exceed min(8 x the err of float32 eager torch on the device + 2.4e-7, 1e-5); before a gate is
trusted the power condition of tests/test_front.py is asserted again with the device's eager figures.  Every figure is
printed.  Tile and chunk sizes come from the library's helpers.
"""
import pytest
import torch

from tests import front_cases as cases
from tests import front_oracle as fo

pytestmark = pytest.mark.gpu

DEV = "cuda"


def product(image, weight, bias, patch, mean=None, std=None, pos_table=None, pos_first=None, before=(), after=()):
    import spfsplatv2_amd as spf
    return spf.embed_patches(image, weight, bias, patch=patch, mean=mean, std=std, pos_table=pos_table, pos_first=pos_first,
                             before=before, after=after)


def run_product(case, d):
    res = cases.run(product, case, d, torch.float32, DEV)
    for k, t in res.items():
        assert t.dtype == torch.float32 and t.is_cuda, k
    assert res["out"].is_contiguous()
    return res


def check(case, muts=None):
    d, x64, dists = cases.reference(case, muts)
    got = run_product(case, d)
    cases.gate(cases.case_id(case), got, cases.eager(case, d, DEV), x64, dists)
    return d, got


# ---- a. the gate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.COVER, ids=cases.case_id)
def test_embed_against_oracle(case):
    """Grids x images: one row, a partial row tile, tiles that straddle images, whole tiles, H != W, both patch sizes;
    C = 64 (less than a column tile), 192, 320 (whole tiles and a partial one), 1024; the three forms of extra rows."""
    check(case)


def test_exact_tiles_and_one_row_more():
    """C = one column tile exactly; M = one row tile exactly, and one row more (three images of 43 patches)."""
    from spfsplatv2_amd import front
    rows, cols = front.tile_rows(), front.tile_cols()
    check((1, rows, 1, 16, 3, cols, "croco"), muts=("swap_patch", "after_front"))
    assert (rows + 1) % 3 == 0
    check((1, (rows + 1) // 3, 3, 14, 5, 2 * cols, "dino"), muts=("pixel_major", "pos_shift", "mean_grad"))


# ---- b. the weight gradient ------------------------------------------------------------------------------------------
def _wgrad_case(images, form="none"):
    return (1, 1, images, 16, 3, 64, form)


@pytest.mark.parametrize("k", [1, 3])
def test_weight_gradient_one_row_above_k_chunks(k):
    """1 x 1 patches per image, C = 64, M = k chunk heights + 1: the last chunk holds one row."""
    from spfsplatv2_amd import front
    h = front.chunk_rows(1)
    m = k * h + 1
    assert front.chunk_rows(m) == h and front.chunks(m) == k + 1
    check(_wgrad_case(m, "croco"), muts=("swap_patch", "no_norm", "after_front", "mean_grad"))


@pytest.mark.parametrize("m", [1, 3])
def test_weight_gradient_of_fewer_rows_than_a_chunk(m):
    """The library never makes more chunks than rows (chunks = ceil(M / height)); the smallest M: one chunk of m rows,
    fewer than one reduction step."""
    from spfsplatv2_amd import front
    assert front.chunks(m) == 1 and m < front.chunk_rows(m)
    check(_wgrad_case(m), muts=("swap_patch", "times_std"))


def _grads(case, d, up, requires=None):
    leaves = cases.leaves_of(d, torch.float32, DEV)
    if requires is not None:
        for k, t in leaves.items():
            t.requires_grad_(k in requires)
    out = cases.call(product, case, d, leaves, d["image"].to(DEV))
    live = {k: t for k, t in leaves.items() if t.requires_grad}
    return out.detach(), dict(zip(live, torch.autograd.grad(out, list(live.values()), up)))


def test_upstream_gradient_read_in_place_or_copied_and_counted():
    """A strided upstream gradient with unit stride along C (a slice of wider rows) is read in place, bitwise equal to the
    dense one's results; one with another stride along C is copied once, and counted."""
    from spfsplatv2_amd import front
    case = (6, 11, 3, 16, 3, 192, "dino")
    d = cases.operands(case)
    up = d["up"].to(DEV)
    _, want = _grads(case, d, up)
    wide = torch.zeros(up.shape[0], up.shape[1] + 3, up.shape[2] + 8, device=DEV)
    wide[:, 2:-1, 4:-4] = up
    view = wide[:, 2:-1, 4:-4]
    assert not view.is_contiguous() and view.stride(2) == 1 and view.data_ptr() % 16 == 0
    before = dict(front.copies)
    _, got = _grads(case, d, view)
    assert front.copies == before
    for k in want:
        assert torch.equal(got[k], want[k]), k
    odd = torch.zeros(*up.shape[:2], 2 * up.shape[2], device=DEV)
    odd[..., ::2] = up
    _, got = _grads(case, d, odd[..., ::2])
    assert front.copies["calls"] - before["calls"] == 1 and front.copies["bytes"] - before["bytes"] == 4 * up.numel()
    for k in want:
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("requires", [("weight",), ("bias", "pos_table"), ("before0", "before1"), ("weight", "pos_first", "before2")],
                         ids="+".join)
def test_gradients_absent_for_some_inputs(requires):
    """``needs_input_grad`` false for the others: what remains is bitwise what the full backward returns."""
    case = (3, 5, 2, 14, 5, 64, "dino")
    d = cases.operands(case)
    up = d["up"].to(DEV)
    _, want = _grads(case, d, up)
    _, got = _grads(case, d, up, requires)
    assert set(got) == set(requires)
    for k in got:
        assert torch.equal(got[k], want[k]), k


# ---- c. images given as views ----------------------------------------------------------------------------------------
def test_image_views_are_read_in_place(monkeypatch):
    """View 1 of a [b, v, C_in, H, W] tensor (a free batch stride), views 1.. of one scene flattened (a view), and a
    channel slice of a 5-channel tensor: the kernel gets the view's own pointer and strides -- nothing is copied."""
    from spfsplatv2_amd import _lib, front
    case = (3, 5, 2, 16, 3, 192, "croco")
    d, x64, dists = cases.reference(case, ("swap_patch", "no_norm"))
    want = run_product(case, d)
    image = d["image"].to(DEV)
    seen = []
    launch = _lib.launch

    def spy(name, device, *args):
        if name == "spf_front_embed_forward":
            seen.append((args[0].image, args[0].stride_b, args[0].stride_c))
        return launch(name, device, *args)
    monkeypatch.setattr(_lib, "launch", spy)

    scenes = torch.rand(2, 3, 3, *image.shape[2:], device=DEV)
    scenes[:, 1] = image
    flat = torch.rand(1, 3, 3, *image.shape[2:], device=DEV)
    flat[0, 1:] = image
    five = torch.rand(2, 5, *image.shape[2:], device=DEV)
    five[:, 1:4] = image
    views = {"view 1 of every scene": scenes[:, 1], "views 1.. of one scene": flat[:, 1:].flatten(0, 1), "channels 1:4 of 5": five[:, 1:4]}
    before = dict(front.copies)
    for label, v in views.items():
        assert v.data_ptr() not in (scenes.data_ptr(), flat.data_ptr(), five.data_ptr()) and v.shape == image.shape
        got = run_product(case, dict(d, image=v))
        assert seen[-1] == (v.data_ptr(), v.stride(0), v.stride(1)), label
        for k in want:
            assert torch.equal(got[k], want[k]), (label, k)
    assert front.copies == before and not scenes[:, 1].is_contiguous() and not five[:, 1:4].is_contiguous()
    cases.gate("views", got, cases.eager(case, d, DEV), x64, dists)


# ---- d. assemble_tokens ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("view", [False, True], ids=["body", "view"])
def test_assemble_tokens(view):
    """A [2, 3, N, C] body, and the view ``tok[:, 1:]`` of a [2, 4, N, C] tensor read in place, with a per-sequence token and
    a broadcast one behind (the decoder's form): the rows are exact copies, the gradients pass the gate."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import block
    d = cases.assemble_operands()

    def run(fn, dtype, device, mut=None):
        leaves = {k: d[k].to(device=device, dtype=dtype).requires_grad_(True) for k in ("x", "intr", "pose")}
        x = leaves["x"]
        if view and device == DEV and mut is None and fn is spf.assemble_tokens:
            big = torch.zeros(2, 4, *x.shape[2:], device=DEV)
            big[:, 1:] = x.detach()
            leaves["x"] = big.requires_grad_(True)
            x = leaves["x"][:, 1:]
            assert block._rows(x) is x and not x.is_contiguous()
        kw = {} if mut is None else {"mut": mut}
        out = fn(x, after=[leaves["intr"], leaves["pose"]], **kw)
        res = cases.with_grads(out, d["up"].to(device=device, dtype=dtype), leaves)
        if res["d_x"].shape[1] == 4:
            assert not res["d_x"][:, 0].any()
            res["d_x"] = res["d_x"][:, 1:]
        return res
    x64 = run(fo.assemble, torch.float64, "cpu", fo.NONE)
    eager = run(fo.assemble, torch.float32, DEV, fo.NONE)
    got = run(spf.assemble_tokens, torch.float32, DEV)
    dists = {m: {k: fo.rel_err(run(fo.assemble, torch.float64, "cpu", frozenset([m]))[k], x64[k]) for k in keys}
             for m, keys in (("after_front", ("out", "d_x")), ("mean_grad", ("d_pose",)))}
    cases.gate("assemble_tokens" + (" view" if view else ""), got, eager, x64, dists)
    for k in ("out", "d_x", "d_intr"):
        assert torch.equal(got[k], eager[k]), k
    again = run(spf.assemble_tokens, torch.float32, DEV)
    for k in got:
        assert torch.equal(got[k], again[k]), k
    # tokens in front as well, and a per-sequence token given as [S, k, C]
    x = d["x"].to(DEV)
    tok, every = torch.randn(1, 2, 64, device=DEV), torch.randn(6, 1, 64, device=DEV)
    out = spf.assemble_tokens(x, before=[tok, every], after=[every])
    want = torch.cat((tok.expand(6, -1, -1), every, x.flatten(0, 1), every), dim=1).view(2, 3, -1, 64)
    assert torch.equal(out, want)


# ---- e. modules against the reference's goldens ----------------------------------------------------------------------
def _golden_gate(label, got: dict, ref32: dict, x64: dict):
    """The gate with the REFERENCE's float32 outputs and gradients as the yardstick."""
    cases.gate(label, got, ref32, x64, {})


def _dust3r(spf, r):
    mod = spf.PatchEmbedDust3R(*r["args"])
    mod.load_state_dict(r["state"], strict=True)
    return mod.to(DEV)


def test_patch_embed_modules_against_the_goldens(golden_dir):
    import spfsplatv2_amd as spf
    g = cases.goldens(golden_dir)
    mean, std = g["mean"], g["std"]
    for key, patch in (("dust3r", 16), ("vggt_patch", 14)):
        r = g[key]
        mod = (spf.PatchEmbedDust3R if key == "dust3r" else spf.VGGTPatchEmbed)(*r["args"])
        mod.load_state_dict(r["state"], strict=True)
        mod = mod.to(DEV)
        image = r["image"].to(DEV)
        if key == "dust3r":
            tokens, pos = mod(image, true_shape=None, mean=mean, std=std)
            assert torch.equal(pos.cpu(), r["pos"])
        else:
            tokens = mod(image, mean=mean, std=std)
        gw, gb = torch.autograd.grad(tokens, (mod.proj.weight, mod.proj.bias), r["up"].to(DEV))
        w, b = r["state"]["proj.weight"].double().requires_grad_(True), r["state"]["proj.bias"].double().requires_grad_(True)
        o64 = fo.embed(r["image"].double(), w, b, patch, mean, std)
        gw64, gb64 = torch.autograd.grad((o64 * r["up"].double()).sum(), (w, b))
        _golden_gate(key, {"out": tokens.detach(), "d_weight": gw, "d_bias": gb},
                     {"out": r["tokens"], "d_weight": r["grads"]["proj.weight"], "d_bias": r["grads"]["proj.bias"]},
                     {"out": o64.detach(), "d_weight": gw64, "d_bias": gb64})
    # the encoder's appends through the module
    r, e = g["dust3r"], g["encode_image"]
    intr, pose = e["intrinsics_embed"].to(DEV).requires_grad_(True), e["pose_embedding"].to(DEV).requires_grad_(True)
    tokens, pos = _dust3r(spf, r)(r["image"].to(DEV), mean=mean, std=std, after=[intr, pose])
    assert torch.equal(pos.cpu(), e["pos"])
    gi, gp = torch.autograd.grad(tokens, (intr, pose), e["up"].to(DEV))
    i64, p64 = e["intrinsics_embed"].double().requires_grad_(True), e["pose_embedding"].double().requires_grad_(True)
    o64 = fo.embed(r["image"].double(), r["state"]["proj.weight"].double(), r["state"]["proj.bias"].double(), 16, mean, std,
                   after=[i64, p64])
    gi64, gp64 = torch.autograd.grad((o64 * e["up"].double()).sum(), (i64, p64))
    _golden_gate("encode_image", {"out": tokens.detach(), "d_intr": gi, "d_pose": gp},
                 {"out": e["tokens"], "d_intr": e["grads"]["intrinsics_embed"], "d_pose": e["grads"]["pose_embedding"]},
                 {"out": o64.detach(), "d_intr": gi64, "d_pose": gp64})
    # the decoder's appends
    dd = g["decoder"]
    leaves = {k: dd[k].to(DEV).requires_grad_(True) for k in ("feat", "intrinsics_embed", "pose_embedding")}
    out = spf.assemble_tokens(leaves["feat"], after=[leaves["intrinsics_embed"], leaves["pose_embedding"].reshape(1, 1, -1)])
    assert torch.equal(out.cpu(), dd["tokens"])
    grads = torch.autograd.grad(out, list(leaves.values()), dd["up"].to(DEV))
    l64 = {k: dd[k].double().requires_grad_(True) for k in leaves}
    o64 = fo.assemble(l64["feat"], after=[l64["intrinsics_embed"], l64["pose_embedding"].reshape(1, 1, -1)])
    g64 = torch.autograd.grad((o64 * dd["up"].double()).sum(), list(l64.values()))
    _golden_gate("decoder", dict(zip(leaves, grads)), dd["grads"], dict(zip(leaves, g64)))


@pytest.mark.parametrize("name", ["plain", "intrinsics"])
def test_prepare_tokens_against_the_goldens(golden_dir, name):
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import front
    g = cases.goldens(golden_dir)
    mean, std, v, dn = g["mean"], g["std"], g["vggt_patch"], g["dino"]
    r, cfg = dn[name], dn["cfg"]
    pe = spf.VGGTPatchEmbed(cfg["img_size"], cfg["patch_size"], cfg["in_chans"], cfg["embed_dim"])
    pe.load_state_dict(v["state"], strict=True)
    pe = pe.to(DEV)
    leaves = {k: t.to(DEV).requires_grad_(True) for k, t in dn["state"].items()}
    leaves["patch_embed.proj.bias"] = pe.proj.bias
    if r["intrinsic_embedding"] is not None:
        leaves["intrinsic_embedding"] = r["intrinsic_embedding"].to(DEV).requires_grad_(True)
    out = spf.prepare_tokens(dn["image"].to(DEV), pe, leaves["cls_token"], leaves["pos_embed"], leaves["register_tokens"],
                             leaves.get("intrinsic_embedding"), mean=mean, std=std,
                             interpolate_antialias=cfg["interpolate_antialias"], interpolate_offset=cfg["interpolate_offset"])
    assert out.shape == r["tokens"].shape
    grads = torch.autograd.grad(out, list(leaves.values()), r["up"].to(DEV))
    l64 = {k: t.double().requires_grad_(True) for k, t in dn["state"].items()}
    l64["patch_embed.proj.bias"] = v["state"]["proj.bias"].double().requires_grad_(True)
    if r["intrinsic_embedding"] is not None:
        l64["intrinsic_embedding"] = r["intrinsic_embedding"].double().requires_grad_(True)
    first, rows = front.interpolate_pos_embed(l64["pos_embed"], 28, 42, 14, cfg["interpolate_antialias"], cfg["interpolate_offset"])
    before = [l64["cls_token"]] + ([l64["intrinsic_embedding"]] if "intrinsic_embedding" in l64 else []) + [l64["register_tokens"]]
    o64 = fo.embed(dn["image"].double(), v["state"]["proj.weight"].double(), l64["patch_embed.proj.bias"], 14, mean, std,
                   pos_table=rows, pos_first=first, before=before)
    g64 = torch.autograd.grad((o64 * r["up"].double()).sum(), list(l64.values()))
    assert list(l64) == list(leaves) and set(leaves) == set(r["grads"])
    _golden_gate(f"prepare_tokens {name}", {"out": out.detach(), **{"d_" + k: t for k, t in zip(leaves, grads)}},
                 {"out": r["tokens"], **{"d_" + k: r["grads"][k] for k in leaves}},
                 {"out": o64.detach(), **{"d_" + k: t for k, t in zip(l64, g64)}})


# ---- f. contracts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [cases.COVER[2], cases.COVER[8]], ids=cases.case_id)
def test_bitwise_repeatable_and_independent_of_the_batch(case):
    """Two runs agree in the output and every gradient; an image's rows are the same bits alone and in the batch; the
    rows the patch kernel does not own are exactly the extra tokens."""
    d = cases.operands(case)
    a, b = run_product(case, d), run_product(case, d)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    gh, gw, nb, p, c_in, c, form = case
    for i in range(nb):
        one = dict(d, image=d["image"][i:i + 1], up=d["up"][i:i + 1],
                   before=[t if t.shape[0] == 1 else t[i:i + 1] for t in d["before"]],
                   after=[t if t.shape[0] == 1 else t[i:i + 1] for t in d["after"]])
        alone = run_product((gh, gw, 1, p, c_in, c, form), one)
        assert torch.equal(alone["out"][0], a["out"][i]), i
    n_before = sum(t.shape[1] for t in d["before"])
    front = [t.to(DEV).expand(nb, -1, -1) for t in d["before"]]
    if front:
        want = torch.cat(front, dim=1).clone()
        want[:, 0] += d["pos_first"].to(DEV)
        assert torch.equal(a["out"][:, :n_before], want)
    if d["after"]:
        want = torch.cat([t.to(DEV).expand(nb, -1, -1) for t in d["after"]], dim=1)
        assert torch.equal(a["out"][:, n_before + gh * gw:], want)
    assert a["out"].shape[1] == n_before + gh * gw + sum(t.shape[1] for t in d["after"])


def test_a_call_uploads_nothing_and_never_waits_for_the_stream(monkeypatch):
    """After the first call for a (mean, std, device) the scale / shift table lives on the device: a step makes no host
    tensor, copies nothing from the host and never synchronises (torch's sync debug mode turns a blocking copy, an
    ``.item()`` or a stream wait into an error) -- ``embed_patches``, ``prepare_tokens``'s form and ``assemble_tokens``."""
    import spfsplatv2_amd as spf
    from spfsplatv2_amd import front
    case = (6, 11, 3, 14, 5, 320, "dino")
    d = cases.operands(case)
    leaves = cases.leaves_of(d, torch.float32, DEV)
    image, up = d["image"].to(DEV), d["up"].to(DEV)
    body = torch.randn(2, 3, 7, 64, device=DEV, requires_grad=True)
    tok = torch.randn(1, 1, 64, device=DEV, requires_grad=True)
    up2 = torch.randn(2, 3, 8, 64, device=DEV)

    def step():
        out = cases.call(product, case, d, leaves, image)
        res = list(torch.autograd.grad(out, list(leaves.values()), up))
        out2 = spf.assemble_tokens(body, after=[tok])
        return [out.detach(), out2.detach()] + res + list(torch.autograd.grad(out2, (body, tok), up2))

    want = step()
    torch.cuda.synchronize()
    tables = dict(front._AFFINES)
    assert tables and all(t.is_cuda for t in tables.values())

    def no_upload(*a, **k):
        raise AssertionError("a second call built a host tensor (the scale / shift table is made once)")
    monkeypatch.setattr(torch, "tensor", no_upload)
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.undo()
    assert set(front._AFFINES) == set(tables) and all(front._AFFINES[k] is t for k, t in tables.items())
    for x, y in zip(want, got):
        assert torch.equal(x, y)

