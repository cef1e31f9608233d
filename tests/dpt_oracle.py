"""Oracle of the DPT heads (TEST INFRASTRUCTURE ONLY): this project's own restatement, in plain torch, of the three
functions of csrc/dpt.hip -- x2 bilinear upsample (+ skip), add + ReLU, the point-map postprocess -- and of both head
forwards (dpt_block.py:121-142 / 189-218 / 428-459, dpt_head.py:35-68, dpt_gs_head.py:41-78, postprocess.py:11-78),
dtype- and device-generic; the tests run it in float64 on the CPU and in float32 as the eager stand-in.  Gradients come
from autograd.

``up2`` is the index formula written out (scale = (in - 1) / (out - 1), src = scale * dst, i0 = floor(src),
i1 = i0 + (i0 < in - 1), lambda1 = src - i0); ``impl="torch"`` takes ``F.interpolate`` in its place: that is what the
float32 eager runs use, and tests/test_dpt.py pins the two to each other in float64.

``mut``: a set of names that turn the oracle into a WRONG one, for the power condition of the gates --
``no_align_corners`` (the align_corners=False rule), ``relu_wrong`` (the ReLU on the wrong addend: on the upsampled
tensor in place of skip; on the first addend in place of the sum), ``no_third`` (the third addend left out), ``exp`` (exp
in place of expm1), ``clip6`` (the norm clipped at 1e-6 in place of 1e-8), ``no_conf_offset`` (conf without its vmin).

Pinned by tests/test_dpt.py against tests/golden/dpt_goldens_{pts,gs}.pt (outputs of the reference's own classes).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

MUTANTS = ("no_align_corners", "relu_wrong", "no_third", "exp", "clip6", "no_conf_offset")
NONE = frozenset()


# ---- the three functions ---------------------------------------------------------------------------------------------
def taps(n_in: int, dtype, device, mut=NONE):
    """(i0, i1, lambda0, lambda1) of the 2 n_in outputs along one axis."""
    n_out = 2 * n_in
    o = torch.arange(n_out, dtype=dtype, device=device)
    if "no_align_corners" in mut:
        src = ((o + 0.5) * 0.5 - 0.5).clamp(min=0)
    else:
        src = o * (torch.tensor(n_in - 1, dtype=dtype, device=device) / (n_out - 1))
    i0 = src.floor().long().clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).long()
    l1 = src - i0.to(dtype)
    return i0, i1, 1 - l1, l1


def up2(x, mut=NONE, impl="formula"):
    """x [B, C, h, w] -> [B, C, 2h, 2w], bilinear, align_corners=True."""
    if impl == "torch":
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners="no_align_corners" not in mut)
    y0, y1, ly0, ly1 = taps(x.shape[2], x.dtype, x.device, mut)
    x0, x1, lx0, lx1 = taps(x.shape[3], x.dtype, x.device, mut)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = lx0 * r0[..., x0] + lx1 * r0[..., x1]
    bot = lx0 * r1[..., x0] + lx1 * r1[..., x1]
    return ly0[:, None] * top + ly1[:, None] * bot


def upsample2x(x, skip=None, relu_skip=False, mut=NONE, impl="formula"):
    u = up2(x, mut, impl)
    if skip is None:
        return u
    if relu_skip:
        return torch.relu(u) + skip if "relu_wrong" in mut else u + torch.relu(skip)
    return u + skip


def add_relu(a, b=None, c=None, mut=NONE):
    """(s, y)"""
    s = a
    if b is not None:
        s = s + b
    if c is not None and "no_third" not in mut:
        s = s + c
    y = torch.relu(s)
    if "relu_wrong" in mut and b is not None:
        y = torch.relu(a) + (s - a)
    return s, y


def postprocess(out, depth_mode, conf_mode, mut=NONE):
    """postprocess.py:11-78 for the 'exp' modes: {"pts3d": [B, H, W, 3][, "conf": [B, H, W]]}"""
    fmap = out.permute(0, 2, 3, 1)
    xyz = fmap[..., 0:3]
    _, vmin, vmax = depth_mode
    no_bounds = vmin == -float("inf") and vmax == float("inf")
    d = xyz.norm(dim=-1, keepdim=True)
    xyz = xyz / d.clip(min=1e-6 if "clip6" in mut else 1e-8)
    e = d.exp() if "exp" in mut else d.expm1()
    if not no_bounds:
        e = e.clip(min=vmin, max=vmax)
    res = dict(pts3d=xyz * e)
    if conf_mode is not None:
        _, cmin, cmax = conf_mode
        conf = fmap[..., 3].exp().clip(max=cmax - cmin)
        res["conf"] = conf if "no_conf_offset" in mut else cmin + conf
    return res


# ---- the functions with their gradients ------------------------------------------------------------------------------
def _cast(t, dtype, device, grad=False):
    if t is None:
        return None
    t = t.detach().to(device=device, dtype=dtype)
    return t.requires_grad_(True) if grad else t


def _impl(dtype):
    """float32 runs are eager torch: F.interpolate itself; float64 runs are the restated formula."""
    return "torch" if dtype == torch.float32 else "formula"


def _grads(outs, ups, leaves):
    pairs = [(o, u) for o, u in zip(outs, ups) if u is not None]
    g = torch.autograd.grad([o for o, _ in pairs], list(leaves.values()), [u for _, u in pairs], allow_unused=True)
    return {k: (torch.zeros_like(leaves[k]) if t is None else t) for k, t in zip(leaves, g)}


def upsample_with_grads(x, skip, relu_skip, dy, dtype=torch.float64, device="cpu", mut=NONE):
    """{out, dx[, dskip]}"""
    x, skip = _cast(x, dtype, device, True), _cast(skip, dtype, device, True)
    out = upsample2x(x, skip, relu_skip, mut, _impl(dtype))
    leaves = {"dx": x} if skip is None else {"dx": x, "dskip": skip}
    return {"out": out.detach(), **_grads([out], [_cast(dy, dtype, device)], leaves)}


def add_relu_with_grads(a, b, c, dy, ds, dtype=torch.float64, device="cpu", mut=NONE):
    """{y, da[, s, db[, dc]]}: ds None where s has no other consumer"""
    a, b, c = (_cast(t, dtype, device, True) for t in (a, b, c))
    s, y = add_relu(a, b, c, mut)
    leaves = {k: v for k, v in (("da", a), ("db", b), ("dc", c)) if v is not None}
    res = {"y": y.detach(), **_grads([y, s], [_cast(dy, dtype, device), _cast(ds, dtype, device)], leaves)}
    if b is not None:
        res["s"] = s.detach()
    return res


def points_with_grads(out, depth_mode, conf_mode, dpts, dconf, dtype=torch.float64, device="cpu", mut=NONE):
    """{pts3d[, conf], din}"""
    out = _cast(out, dtype, device, True)
    res = postprocess(out, depth_mode, conf_mode, mut)
    outs, ups = [res["pts3d"]], [_cast(dpts, dtype, device)]
    if conf_mode is not None:
        outs.append(res["conf"])
        ups.append(_cast(dconf, dtype, device))
    return {**{k: v.detach() for k, v in res.items()}, **_grads(outs, ups, {"din": out})}


# ---- the heads -------------------------------------------------------------------------------------------------------
# ``impl="mixed"`` (with float64 tensors): every place where the product calls a kernel of csrc/dpt.hip -- the ReLU that
# opens a residual unit, the add of three with its ReLU, the upsamples, the Gaussian head's tail, postprocess -- runs in
# float32 eager torch between a cast down and a cast up, and everything else (the convolutions, the ReLU between a unit's
# convolutions, the tensor add) in float64.  What such a run differs by from the float64 oracle is the float32 error of
# those places alone, carried through exact convolutions: the convolutions' own float32 backward, which does not return
# the same floats from run to run on the device, takes no part.
def _site(fn, impl, *tensors):
    """fn(*tensors, impl) -> a tuple of tensors, in float32 eager torch under ``mixed``."""
    if impl != "mixed":
        return fn(*tensors, impl)
    outs = fn(*(None if t is None else t.float() for t in tensors), "torch")
    return tuple(o.double() for o in outs)


def _conv(x, w, name, **kw):
    return F.conv2d(x, w[name + ".weight"], w.get(name + ".bias"), **kw)


def _rcu_branch(y, w, p):
    return _conv(torch.relu(_conv(y, w, p + ".conv1", padding=1)), w, p + ".conv2", padding=1)


def _relu_site(x, impl):
    return _site(lambda t, _: (torch.relu(t),), impl, x)[0]


def _up_site(x, mut, impl):
    return _site(lambda t, i: (up2(t, mut, i),), impl, x)[0]


def _fusion(xs, w, p, mut, impl):
    if len(xs) == 2:
        res = _rcu_branch(_relu_site(xs[1], impl), w, p + ".resConfUnit1")
        s, y = _site(lambda a, b, c, _: add_relu(a, b, c, mut), impl, res, xs[1], xs[0])
    else:
        s, y = xs[0], _relu_site(xs[0], impl)
    out = _rcu_branch(y, w, p + ".resConfUnit2") + s
    return _conv(_up_site(out, mut, impl), w, p + ".out_conv")


def _path_1(tokens, image_size, w, patch, mut, impl):
    n_h, n_w = image_size[0] // patch, image_size[1] // patch
    layers = [t.transpose(1, 2).reshape(t.shape[0], t.shape[2], n_h, n_w) for t in tokens]
    a = "act_postprocess."
    layers[0] = F.conv_transpose2d(_conv(layers[0], w, a + "0.0"), w[a + "0.1.weight"], w[a + "0.1.bias"], stride=4)
    layers[1] = F.conv_transpose2d(_conv(layers[1], w, a + "1.0"), w[a + "1.1.weight"], w[a + "1.1.bias"], stride=2)
    layers[2] = _conv(layers[2], w, a + "2.0")
    layers[3] = _conv(_conv(layers[3], w, a + "3.0"), w, a + "3.1", stride=2, padding=1)
    layers = [_conv(l, w, f"scratch.layer_rn.{i}", padding=1) for i, l in enumerate(layers)]
    path_4 = _fusion([layers[3]], w, "scratch.refinenet4", mut, impl)[:, :, :layers[2].shape[2], :layers[2].shape[3]]
    path_3 = _fusion([path_4, layers[2]], w, "scratch.refinenet3", mut, impl)
    path_2 = _fusion([path_3, layers[1]], w, "scratch.refinenet2", mut, impl)
    return _fusion([path_2, layers[0]], w, "scratch.refinenet1", mut, impl)


def pts_head(tokens, image_size, w, patch, depth_mode, conf_mode, mut=NONE, impl="formula"):
    """``PixelwiseTaskWithDPT.forward`` of dpt_head.py with the state dict ``w`` of its ``dpt`` (keys without the
    ``dpt.`` prefix) and head_type='regression'."""
    x = _conv(_path_1(tokens, image_size, w, patch, mut, impl), w, "head.0", padding=1)
    x = torch.relu(_conv(_up_site(x, mut, impl), w, "head.2", padding=1))
    names = ("pts3d",) if conf_mode is None else ("pts3d", "conf")
    res = _site(lambda t, _: tuple(postprocess(t, depth_mode, conf_mode, mut)[k] for k in names), impl, _conv(x, w, "head.4"))
    return dict(zip(names, res))


def gs_head(tokens, imgs, image_size, w, patch, mut=NONE, impl="formula"):
    """``PixelwiseTaskWithDPT.forward`` of dpt_gs_head.py (head_type='gs_params', evaluation mode, no postprocess)."""
    path_1 = _path_1(tokens, image_size, w, patch, mut, impl)
    path_1 = _site(lambda x, skip, i: (upsample2x(x, skip, True, mut, i),), impl, path_1,
                   _conv(imgs, w, "input_merger.0", padding=3))[0]
    return _conv(torch.relu(_conv(path_1, w, "head.0", padding=1)), w, "head.4")


def module_case(gold: dict, dtype=torch.float64, device="cpu", mut=NONE, mixed=False):
    """One golden evaluated with the oracle in ``dtype`` on ``device``: ({output}, {input: gradient}, {parameter:
    gradient}); the loss is the goldens' 0.5 * sum(out^2) over every output.  ``mixed`` (float64 only): see above."""
    names = sorted(gold["pgrads"])                       # one entry per parameter: the duplicated keys share it
    params = {k: gold["weights"]["dpt." + k].to(device=device, dtype=dtype).requires_grad_(True) for k in names}
    w = dict(params)
    for i in range(4):                                   # (scratch.layerN_rn is scratch.layer_rn.N-1)
        w[f"scratch.layer_rn.{i}.weight"] = params[f"scratch.layer{i + 1}_rn.weight"]
    ins = {k: v.to(device=device, dtype=dtype).requires_grad_(True) for k, v in gold["inputs"].items()}
    tokens = [ins[f"tok{i}"] for i in range(4)]
    impl = "mixed" if mixed else _impl(dtype)
    assert not mixed or dtype == torch.float64
    if gold["kind"] == "pts":
        outs = pts_head(tokens, gold["image_size"], w, gold["patch"], gold["depth_mode"], gold["conf_mode"], mut, impl)
    else:
        outs = {"out": gs_head(tokens, ins["img"], gold["image_size"], w, gold["patch"], mut, impl)}
    leaves = {**ins, **params}
    loss = sum(0.5 * (o * o).sum() for o in outs.values())
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    grads = {k: (torch.zeros_like(leaves[k]) if t is None else t) for k, t in zip(leaves, grads)}
    return {k: v.detach() for k, v in outs.items()}, {k: grads[k] for k in ins}, {k: grads[k] for k in params}


def rel_err(got, want) -> float:
    """max|x - x64| / max|x64|"""
    return float((got.detach().double().cpu() - want.double().cpu()).abs().max()) / float(want.abs().max())
