"""The encoder front on the HIP library (csrc/front.hip): image -> tokens.

Host mirror of the first link of the reference's training step:

* CroCo backbones: ``normalize_image`` (dataset/shims/normalize_shim.py:15), ``PatchEmbedDust3R.forward``
  (croco/patch_embed.py:19-29: ``nn.Conv2d(3, 1024, 16, 16)``, ``flatten(2).transpose(1, 2)``) and the ``torch.cat`` of the
  intrinsics and pose tokens behind the patch rows (backbone_masked_croco.py:161-172 in the encoder, :186-201 in the
  decoder);
* VGGT: the ``_resnet_mean`` / ``_resnet_std`` affine (aggregator.py:206), the 14 x 14 ``PatchEmbed``
  (vggt/layers/patch_embed.py:68-81), ``prepare_tokens_with_masks`` (vision_transformer.py:223-267) and the aggregator's
  ``cat([camera_token, register_token, patch_tokens])`` (aggregator.py:237-244).

``embed_patches`` is one launch for the patch rows (an implicit GEMM on the float32 matrix instruction that reads the
image and ``proj.weight`` where they lie, the normalisation applied as one fma at staging, bias and ``pos_embed`` rows in
the epilogue, every row written at its place among the extra tokens) and one small launch for the extra rows.  Its
backward reads the upstream gradient at its placed rows.  ``assemble_tokens`` is the case where the extra tokens arrive
after the encoder blocks.

Not served (refused with an error): a gradient to the image, ``ManyAR_PatchEmbed``'s portrait branch, ``masks`` /
``mask_token``, a ``norm_layer``, any dtype but float32, patch sizes other than 14 and 16, CPU tensors.  The pixelwise
intrinsic embedding (``get_intrinsic_embedding``) stays the caller's: its channels are input channels 3.. here.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch
from torch import Tensor, nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._checks import check_device as _check_device, check_float32 as _check_float32
from .block import _row_map, _rows
from .rope import PositionGetter, append_token_position

PATCH_SIZES = (14, 16)
MAX_IN_CHANS = 32
MAX_TOKENS = _lib.FRONT_MAX_TOKENS

# every copy made of an operand that could not be read in place (as tail.dense_copies): an image is never copied -- a
# layout the kernels cannot read is refused --, so this counts upstream gradients and token tensors only
copies = {"calls": 0, "bytes": 0}


def _geometry(what: int, m: int = 0) -> int:
    return int(_lib.load().spf_front_geometry(what, int(m)))


def tile_rows() -> int:
    """Patch rows of one block's tile of the forward kernel.  Host only."""
    return _geometry(_lib.FRONT_TILE_ROWS)


def tile_cols() -> int:
    """Embedding channels of one block's tile.  Host only."""
    return _geometry(_lib.FRONT_TILE_COLS)


def chunk_rows(m: int) -> int:
    """The height of a chunk of the weight gradient for ``m`` patch rows (all images): the library's arithmetic."""
    return _geometry(_lib.FRONT_CHUNK_ROWS, m)


def chunks(m: int) -> int:
    """The number of chunks the weight gradient of ``m`` patch rows is summed in: ceil(m / chunk_rows(m))."""
    return _geometry(_lib.FRONT_CHUNKS, m)


# ---- checks ----------------------------------------------------------------------------------------------------------
def _check_patch(what: str, patch) -> int:
    if isinstance(patch, (tuple, list)):
        if len(patch) != 2 or patch[0] != patch[1]:
            raise NotImplementedError(f"{what}: only square patches are served, got {tuple(patch)}")
        patch = patch[0]
    if patch not in PATCH_SIZES:
        raise NotImplementedError(f"{what}: patch size {patch} is not served (14 or 16)")
    return int(patch)


def _check_image(what: str, image: Tensor, p: int, c_in: int) -> None:
    if image.dim() != 4:
        raise RuntimeError(f"{what}: the image must be [B, C_in, H, W], got shape {list(image.shape)}")
    b, c, h, w = image.shape
    if c != c_in:
        raise RuntimeError(f"{what}: the image has {c} channels, the weight {c_in}")
    if not 1 <= c_in <= MAX_IN_CHANS:
        raise ValueError(f"{what}: C_in must be 1 .. {MAX_IN_CHANS}, got {c_in}")
    if b < 1 or h < p or w < p or h % p or w % p:
        raise RuntimeError(f"{what}: image height ({h}) and width ({w}) must be positive multiples of the patch size ({p})")
    if b * (h // p) * (w // p) > 2 ** 31 - 1:
        raise RuntimeError(f"{what}: more than 2^31 - 1 patches")
    if image.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{what}: a gradient to the image is not served (requires_grad is set on it)")
    v = 4 if p == 16 else 2
    strides = [s for n, s in zip(image.shape[:3], image.stride()[:3]) if n > 1]
    if image.stride(3) != 1 or any(s % v or s < 0 for s in strides) or image.stride(2) < w or image.data_ptr() % (4 * v):
        raise RuntimeError(f"{what}: the image is read in place and must have unit stride along a row, a {4 * v}-byte aligned "
                           f"base and batch / channel / row strides that are multiples of {v} floats for patch size {p} "
                           f"(got strides {list(image.stride())}, base % {4 * v} = {image.data_ptr() % (4 * v)}); it is "
                           "not copied")


def _check_tokens(what: str, name: str, tokens, s: int, c: int) -> list:
    tokens = list(tokens)
    for i, t in enumerate(tokens):
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: {name}[{i}] must be a tensor, got {type(t).__name__}")
        if t.dim() != 3 or t.shape[0] not in (1, s) or t.shape[1] < 1 or t.shape[2] != c:
            raise RuntimeError(f"{what}: {name}[{i}] must be [1, k, {c}] or [{s}, k, {c}] with k >= 1, got {list(t.shape)}")
    return tokens


def _affine_values(what: str, mean, std, c_in: int):
    """(scale, shift) per input channel as Python floats: x * scale + shift = (x - mean) / std; channels beyond
    len(mean) pass through.  None without a normalisation."""
    if mean is None and std is None:
        return None
    if mean is None or std is None:
        raise ValueError(f"{what}: mean and std come together")
    vals = []
    for name, v in (("mean", mean), ("std", std)):
        if isinstance(v, Tensor):
            if v.is_cuda:
                raise TypeError(f"{what}: {name} must be host numbers (a sequence of floats or a CPU tensor): a device "
                                "tensor would have to be read back")
            v = v.reshape(-1).tolist()
        vals.append(tuple(float(x) for x in v))
    mean, std = vals
    if len(mean) != len(std) or not 1 <= len(mean) <= c_in:
        raise ValueError(f"{what}: mean and std must have the same length in 1 .. C_in = {c_in}, got {len(mean)} and {len(std)}")
    if any(s == 0.0 or not math.isfinite(s) for s in std) or not all(math.isfinite(m) for m in mean):
        raise ValueError(f"{what}: mean must be finite and std finite and non-zero")
    pad = c_in - len(mean)
    return tuple(1.0 / s for s in std) + (1.0,) * pad, tuple(-m / s for m, s in zip(mean, std)) + (0.0,) * pad


# the [2, C_in] scale / shift table on the device, made once per (values, device): a call uploads nothing
_AFFINES = {}


def _device_affine(values, device) -> Optional[Tensor]:
    if values is None:
        return None
    key = (values, torch.device(device))
    t = _AFFINES.get(key)
    if t is None:
        t = _AFFINES[key] = torch.tensor(values, dtype=torch.float64).to(torch.float32).to(device)
    return t


# ---- operands --------------------------------------------------------------------------------------------------------
def _dense(t: Optional[Tensor]) -> Optional[Tensor]:
    """A parameter-sized operand as the kernels read it: dense and 16-byte aligned."""
    if t is None:
        return None
    t = t.detach()
    if t.is_contiguous() and t.data_ptr() % 16 == 0:
        return t
    copies["calls"] += 1
    copies["bytes"] += t.numel() * t.element_size()
    return t.contiguous() if not t.is_contiguous() else t.clone()


def _grad_rows(g: Tensor) -> Tensor:
    """The upstream gradient [S, T, C] read where it lies when its rows allow it (unit stride along C, sequence and row
    strides that are multiples of 4 floats, rows apart, a 16-byte aligned base), else one dense copy, counted."""
    s, t, c = g.shape
    ok = g.dtype == torch.float32 and g.data_ptr() % 16 == 0 and g.stride(2) == 1
    ok = ok and (t == 1 or (g.stride(1) % 4 == 0 and g.stride(1) >= c)) and (s == 1 or (g.stride(0) % 4 == 0 and g.stride(0) >= 0))
    if ok:
        return g
    copies["calls"] += 1
    copies["bytes"] += g.numel() * 4
    return g.float().contiguous() if not (g.is_contiguous() and g.dtype == torch.float32) else g.clone()


def _grad_strides(g: Tensor):
    s, t, c = g.shape
    return (g.stride(0) if s > 1 else 0), (g.stride(1) if t > 1 else c)


def _token_args(tensors) -> _lib.SpfFrontTokens:
    """The pointers of the token tensors (or of their gradients' destinations; None: none)."""
    a = _lib.SpfFrontTokens()
    for i, t in enumerate(tensors):
        if t is not None:
            a.tok[i] = t.data_ptr()
    return a


def _describe(a: _lib.SpfFrontTokens, shapes, n_before: int, s: int) -> None:
    """rows / per_image / counts of ``a`` from the token tensors' shapes."""
    for i, (rows, per_image) in enumerate(shapes):
        a.rows[i], a.per_image[i] = rows, per_image
    a.n_before, a.n_after = n_before, len(shapes) - n_before
    a.before = sum(r for r, _ in shapes[:n_before])
    a.after = sum(r for r, _ in shapes[n_before:])


def _token_shapes(tokens, s: int):
    # [1, k, C] with one sequence is a per-image tensor and a broadcast one alike; it is treated as broadcast
    return [(int(t.shape[1]), int(t.shape[0] != 1)) for t in tokens]


def _token_grads(ctx_shapes, n_before, needs, g, n_body, s, c, d_pos_first):
    """The gradients of the extra tokens from the upstream gradient ``g`` [S, T, C]: per-image tensors as views of ``g``,
    broadcast ones summed over the sequences in one launch (which also serves ``d_pos_first``)."""
    grads, dst, r = [], [], 0
    for i, ((rows, per_image), need) in enumerate(zip(ctx_shapes, needs)):
        if i == n_before:
            r += n_body
        if not need:
            grads.append(None)
            dst.append(None)
        elif per_image:
            grads.append(g[:, r:r + rows])
            dst.append(None)
        else:
            t = torch.empty((1, rows, c), dtype=torch.float32, device=g.device)
            grads.append(t)
            dst.append(t)
        r += rows
    if any(t is not None for t in dst) or d_pos_first is not None:
        a = _token_args(dst)
        _describe(a, ctx_shapes, n_before, s)
        ss, sr = _grad_strides(g)
        _lib.launch("spf_front_tokens_backward", g.device, a, g, ss, sr, s, n_body, c, d_pos_first)
    return grads


class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, weight, bias, pos_table, pos_first, patch, affine, n_before, *tokens):
        ctx.set_materialize_grads(False)
        image = image.detach()
        b, c_in, h, w = image.shape
        c, gh, gw = weight.shape[0], h // patch, w // patch
        toks = [_dense(t) for t in tokens]
        shapes = _token_shapes(toks, b)
        a = _lib.SpfFront()
        a.image, a.affine = image.data_ptr(), (affine.data_ptr() if affine is not None else None)
        a.stride_b = image.stride(0) if b > 1 else 0
        a.stride_c = image.stride(1) if c_in > 1 else 0
        a.stride_y = image.stride(2)
        a.B, a.C_in, a.gh, a.gw, a.P, a.C = b, c_in, gh, gw, patch, c
        ta = _token_args(toks)
        _describe(ta, shapes, n_before, b)
        a.before, a.after = ta.before, ta.after
        out = torch.empty((b, a.before + gh * gw + a.after, c), dtype=torch.float32, device=image.device)
        _lib.launch("spf_front_embed_forward", image.device, a, _dense(weight), _dense(bias), _dense(pos_table), out)
        if toks:
            first = _dense(pos_first)
            ta.pos_first = first.data_ptr() if first is not None else None
            _lib.launch("spf_front_assemble", image.device, ta, None, 1, 0, 0, b, gh * gw, c, out)
        ctx.save_for_backward(image, affine)
        ctx.args, ctx.shapes, ctx.n_before = a, shapes, n_before
        ctx.has = (bias is not None, pos_table is not None, pos_first is not None)
        ctx.weight_shape = tuple(weight.shape)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        n_in = 8 + len(ctx.shapes)
        if g is None:
            return (None,) * n_in
        image, affine = ctx.saved_tensors
        a = ctx.args                                   # (its pointers are those of the saved tensors, alive in ctx)
        g = _grad_rows(g)
        c, np_ = a.C, a.gh * a.gw
        need = ctx.needs_input_grad
        f32 = dict(dtype=torch.float32, device=g.device)
        dw = torch.empty(ctx.weight_shape, **f32) if need[1] else None
        db = torch.empty((c,), **f32) if ctx.has[0] and need[2] else None
        dpos = torch.empty((np_, c), **f32) if ctx.has[1] and need[3] else None
        if dw is not None or db is not None or dpos is not None:
            floats = int(_lib.load().spf_front_workspace_floats(a, int(dw is not None)))
            if floats < 0:
                raise _lib.SpfError("spf_front_workspace_floats: " + _lib.load().spf_last_error().decode())
            ws = torch.empty((floats,), **f32)
            ss, sr = _grad_strides(g)
            _lib.launch("spf_front_embed_backward", g.device, a, g, ss, sr, ws, dw, db, dpos)
        dfirst = torch.empty((c,), **f32) if ctx.has[2] and need[4] else None
        dtok = _token_grads(ctx.shapes, ctx.n_before, need[8:], g, np_, a.B, c, dfirst)
        return (None, dw, db, dpos, dfirst, None, None, None, *dtok)


def embed_patches(image: Tensor, weight: Tensor, bias: Optional[Tensor] = None, *, patch, mean=None, std=None,
                  pos_table: Optional[Tensor] = None, pos_first: Optional[Tensor] = None, before: Sequence[Tensor] = (),
                  after: Sequence[Tensor] = ()) -> Tensor:
    """``image`` [B, C_in, H, W] -> tokens [B, before + (H / patch)(W / patch) + after, C]: the patch rows are
    ``conv2d((image - mean) / std, weight, bias, stride=patch).flatten(2).transpose(1, 2)`` (``+ pos_table`` [N, C]),
    ``before`` / ``after`` are token tensors [1, k, C] (broadcast over the images) or [B, k, C] written around them and
    ``pos_first`` [C] is added to the first row of ``before``.  ``mean`` / ``std``: host numbers, one per leading input
    channel; the other channels pass through.  Differentiable in everything but the image, which is read in place."""
    what = "embed_patches"
    p = _check_patch(what, patch)
    for t in (image, weight):
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}: expected a tensor, got {type(t).__name__}")
    _check_float32(what, image, weight, bias, pos_table, pos_first, *before, *after)
    if weight.dim() != 4 or weight.shape[2] != p or weight.shape[3] != p:
        raise RuntimeError(f"{what}: the weight must be [C, C_in, {p}, {p}], got {list(weight.shape)}")
    c, c_in = int(weight.shape[0]), int(weight.shape[1])
    if c < 4 or c % 4:
        raise ValueError(f"{what}: the embedding width must be a positive multiple of 4, got {c}")
    _check_image(what, image, p, c_in)
    b, n = image.shape[0], (image.shape[2] // p) * (image.shape[3] // p)
    if bias is not None and tuple(bias.shape) != (c,):
        raise RuntimeError(f"{what}: bias must have shape [{c}], got {list(bias.shape)}")
    if pos_table is not None:
        if pos_table.dim() == 3 and pos_table.shape[0] == 1:
            pos_table = pos_table[0]
        if tuple(pos_table.shape) != (n, c):
            raise RuntimeError(f"{what}: pos_table must be [{n}, {c}] (one row per patch), got {list(pos_table.shape)}")
    before, after = _check_tokens(what, "before", before, b, c), _check_tokens(what, "after", after, b, c)
    if len(before) + len(after) > MAX_TOKENS:
        raise ValueError(f"{what}: at most {MAX_TOKENS} token tensors, got {len(before) + len(after)}")
    if pos_first is not None:
        if pos_first.numel() != c:
            raise RuntimeError(f"{what}: pos_first must hold {c} values, got shape {list(pos_first.shape)}")
        if not before:
            raise ValueError(f"{what}: pos_first is added to the first row of `before`, which is empty")
        pos_first = pos_first.reshape(c)
    values = _affine_values(what, mean, std, c_in)
    _check_device(what, image, weight, bias, pos_table, pos_first, *before, *after)
    affine = _device_affine(values, image.device)
    return _EmbedFn.apply(image, weight, bias, pos_table, pos_first, p, affine, len(before), *before, *after)


# ---- tokens that arrive after the encoder blocks -----------------------------------------------------------------------
class _AssembleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_before, *tokens):
        ctx.set_materialize_grads(False)
        lead, n, c = x.shape[:-2], x.shape[-2], x.shape[-1]
        s = math.prod(lead)
        xr = _rows(x.detach())
        toks = [_dense(t.reshape(-1, t.shape[-2], c) if t.dim() != 3 else t) for t in tokens]
        shapes = _token_shapes(toks, s)
        ta = _token_args(toks)
        _describe(ta, shapes, n_before, s)
        out = torch.empty((*lead, ta.before + n + ta.after, c), dtype=torch.float32, device=x.device)
        inner, stride, outer = _row_map(xr)
        _lib.launch("spf_front_assemble", x.device, ta, xr if n else None, inner, stride, outer, s, n, c, out)
        ctx.shapes, ctx.n_before, ctx.x_shape, ctx.tok_shapes = shapes, n_before, tuple(x.shape), [tuple(t.shape) for t in tokens]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if g is None:
            return (None,) * (2 + len(ctx.shapes))
        n, c = ctx.x_shape[-2:]
        s = math.prod(ctx.x_shape[:-2])
        g = _grad_rows(g.reshape(s, -1, c))
        need = ctx.needs_input_grad
        dx = None
        if need[0]:
            dx = torch.empty(ctx.x_shape, dtype=torch.float32, device=g.device)
            if dx.numel():
                before = sum(r for r, _ in ctx.shapes[:ctx.n_before])
                ss, sr = _grad_strides(g)
                _lib.launch("spf_front_assemble", g.device, _lib.SpfFrontTokens(), g[:, before:before + n], n, sr, ss, s, n, c,
                            dx)
        dtok = _token_grads(ctx.shapes, ctx.n_before, need[2:], g, n, s, c, None)
        dtok = [t if t is None else t.reshape(shape) for t, shape in zip(dtok, ctx.tok_shapes)]
        return (dx, None, *dtok)


def assemble_tokens(x: Tensor, before: Sequence[Tensor] = (), after: Sequence[Tensor] = ()) -> Tensor:
    """``torch.cat((*before, x, *after), dim=-2)`` for a body ``x`` [.., N, C] and token tensors [1, k, C] (broadcast over
    the sequences) or [.., k, C] (one per sequence), in one launch each way (backbone_masked_croco.py:186-201).  The body
    is read in place under the row rules of ``block._rows``."""
    what = "assemble_tokens"
    if not isinstance(x, Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(x).__name__}")
    _check_float32(what, x, *before, *after)
    if x.dim() < 2:
        raise RuntimeError(f"{what}: the body must be [.., N, C], got shape {list(x.shape)}")
    c, lead = int(x.shape[-1]), tuple(x.shape[:-2])
    s = math.prod(lead)
    if c < 4 or c % 4 or s < 1:
        raise ValueError(f"{what}: the row width must be a positive multiple of 4 and there must be a sequence, got "
                         f"shape {list(x.shape)}")
    before, after = list(before), list(after)
    if len(before) + len(after) > MAX_TOKENS:
        raise ValueError(f"{what}: at most {MAX_TOKENS} token tensors, got {len(before) + len(after)}")
    for name, toks in (("before", before), ("after", after)):
        for i, t in enumerate(toks):
            if not isinstance(t, Tensor):
                raise TypeError(f"{what}: {name}[{i}] must be a tensor, got {type(t).__name__}")
            ok = t.dim() >= 3 and t.shape[-1] == c and t.shape[-2] >= 1 and (tuple(t.shape[:-2]) == lead or
                                                                             (t.dim() == 3 and t.shape[0] in (1, s)))
            if not ok:
                raise RuntimeError(f"{what}: {name}[{i}] must be [1, k, {c}] or [{', '.join(map(str, lead))}, k, {c}], "
                                   f"got {list(t.shape)}")
    if s * (x.shape[-2] + sum(t.shape[-2] for t in before + after)) > 2 ** 31 - 1:
        raise RuntimeError(f"{what}: more than 2^31 - 1 rows")
    _check_device(what, x, *before, *after)
    return _AssembleFn.apply(x, len(before), *before, *after)


# ---- modules ---------------------------------------------------------------------------------------------------------
class PatchEmbedDust3R(nn.Module):
    """croco/patch_embed.py's ``PatchEmbedDust3R`` (over croco/blocks.py's ``PatchEmbed``): the same constructor, the
    same parameters (``proj.weight``, ``proj.bias`` of an ``nn.Conv2d`` that is never run) and ``position_getter``.
    ``forward(x, true_shape=None, mean=None, std=None, after=())`` returns ``(tokens, pos)``; ``mean`` / ``std`` fold
    ``normalize_image`` in, ``after`` the intrinsics / pose tokens, whose positions ``append_token_position`` adds."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten=True):
        super().__init__()
        if norm_layer is not None:
            raise NotImplementedError("PatchEmbedDust3R: a norm_layer is not served (only None)")
        if not flatten:
            raise NotImplementedError("PatchEmbedDust3R: flatten=False is not served")
        p = _check_patch("PatchEmbedDust3R", patch_size)
        img_size = tuple(img_size) if isinstance(img_size, (tuple, list)) else (img_size, img_size)
        self.img_size, self.patch_size = img_size, (p, p)
        self.grid_size = (img_size[0] // p, img_size[1] // p)
        self.num_patches = self.grid_size[0] * self.grid_size[1]
        self.flatten = flatten
        self.embed_dim = embed_dim
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=p, stride=p)
        self.norm = nn.Identity()
        self.position_getter = PositionGetter()

    def forward(self, x: Tensor, true_shape=None, mean=None, std=None, after: Sequence[Tensor] = ()):
        p = self.patch_size[0]
        if true_shape is not None and x.dim() == 4:
            # ManyAR_PatchEmbed's portrait branch transposes images whose true height exceeds their width
            if isinstance(true_shape, Tensor):
                raise NotImplementedError("PatchEmbedDust3R: a true_shape tensor (ManyAR_PatchEmbed's portrait branch) is "
                                          "not served; pass None, or host (height, width) pairs of landscape images")
            if any(int(hh) > int(ww) for hh, ww in true_shape):
                raise NotImplementedError("PatchEmbedDust3R: ManyAR_PatchEmbed's portrait branch is not served")
        tokens = embed_patches(x, self.proj.weight, self.proj.bias, patch=p, mean=mean, std=std, after=after)
        pos = self.position_getter(x.shape[0], x.shape[2] // p, x.shape[3] // p, x.device)
        for t in after:
            for _ in range(t.shape[1]):
                pos = append_token_position(pos)
        return tokens, pos


class VGGTPatchEmbed(nn.Module):
    """vggt/layers/patch_embed.py's ``PatchEmbed``: the same constructor and keys.  ``forward(x, **kw)`` passes ``mean``,
    ``std``, ``pos_table``, ``pos_first``, ``before`` and ``after`` on to ``embed_patches``."""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768, norm_layer=None, flatten_embedding=True):
        super().__init__()
        if norm_layer is not None:
            raise NotImplementedError("VGGTPatchEmbed: a norm_layer is not served (only None)")
        if not flatten_embedding:
            raise NotImplementedError("VGGTPatchEmbed: flatten_embedding=False is not served")
        p = _check_patch("VGGTPatchEmbed", patch_size)
        img_size = tuple(img_size) if isinstance(img_size, (tuple, list)) else (img_size, img_size)
        self.img_size, self.patch_size = img_size, (p, p)
        self.patches_resolution = (img_size[0] // p, img_size[1] // p)
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim, self.flatten_embedding = in_chans, embed_dim, flatten_embedding
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=p, stride=p)
        self.norm = nn.Identity()

    def forward(self, x: Tensor, **kw) -> Tensor:
        return embed_patches(x, self.proj.weight, self.proj.bias, patch=self.patch_size[0], **kw)


def interpolate_pos_embed(pos_embed: Tensor, h: int, w: int, patch: int, interpolate_antialias: bool = False,
                          interpolate_offset: float = 0.1):
    """``DinoVisionTransformer.interpolate_pos_encoding`` (vision_transformer.py:190-221) as (the cls row [C], the patch
    rows [h0 w0, C]) for an ``h`` x ``w`` image: plain torch on a parameter-sized tensor, nothing cached -- autograd
    carries the table's gradient through the interpolation."""
    n = pos_embed.shape[1] - 1
    h0, w0 = h // patch, w // patch
    table = pos_embed.float()
    first, rows = table[0, 0], table[0, 1:]
    if h0 * w0 == n and w == h:
        return first, rows
    m = int(math.sqrt(n))
    if m * m != n:
        raise RuntimeError(f"interpolate_pos_embed: pos_embed holds {n} patch rows, not a square number")
    dim = table.shape[-1]
    if interpolate_offset:
        kwargs = dict(scale_factor=(float(h0 + interpolate_offset) / m, float(w0 + interpolate_offset) / m))
    else:
        kwargs = dict(size=(h0, w0))
    grid = nn.functional.interpolate(rows.reshape(1, m, m, dim).permute(0, 3, 1, 2), mode="bicubic",
                                     antialias=interpolate_antialias, **kwargs)
    if tuple(grid.shape[-2:]) != (h0, w0):
        raise RuntimeError(f"interpolate_pos_embed: the interpolation gave {list(grid.shape[-2:])}, expected {[h0, w0]}")
    return first, grid.permute(0, 2, 3, 1).reshape(h0 * w0, dim)


def prepare_tokens(image: Tensor, patch_embed, cls_token: Tensor, pos_embed: Tensor, register_tokens: Optional[Tensor] = None,
                   intrinsic_embedding: Optional[Tensor] = None, mean=None, std=None, masks=None,
                   interpolate_antialias: bool = False, interpolate_offset: float = 0.1) -> Tensor:
    """What ``DinoVisionTransformer.prepare_tokens_with_masks`` returns for ``masks=None``
    (vision_transformer.py:223-267): rows cls, [intrinsics], registers, patches; ``pos_embed`` (interpolated to the
    image's grid) is added to the cls row and the patch rows.  ``patch_embed``: a ``VGGTPatchEmbed`` (or anything with
    ``proj`` and ``patch_size``)."""
    what = "prepare_tokens"
    if masks is not None:
        raise NotImplementedError(f"{what}: masks / mask_token are not served")
    if not isinstance(image, Tensor) or image.dim() != 4:
        raise RuntimeError(f"{what}: the image must be a [B, C_in, H, W] tensor")
    p = _check_patch(what, patch_embed.patch_size)
    if not isinstance(getattr(patch_embed, "norm", None), (nn.Identity, type(None))):
        raise NotImplementedError(f"{what}: a norm_layer is not served (only None)")
    _check_float32(what, image, cls_token, pos_embed, register_tokens, intrinsic_embedding)
    if pos_embed.dim() != 3 or pos_embed.shape[0] != 1:
        raise RuntimeError(f"{what}: pos_embed must be [1, 1 + N, C], got {list(pos_embed.shape)}")
    first, rows = interpolate_pos_embed(pos_embed, image.shape[2], image.shape[3], p, interpolate_antialias,
                                        interpolate_offset)
    before = [cls_token.reshape(1, 1, -1)]
    if intrinsic_embedding is not None:
        before.append(intrinsic_embedding)
    if register_tokens is not None:
        before.append(register_tokens)
    return embed_patches(image, patch_embed.proj.weight, patch_embed.proj.bias, patch=p, mean=mean, std=std, pos_table=rows,
                         pos_first=first, before=before)
