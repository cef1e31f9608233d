"""The encoder front restated in plain torch (any dtype, any device): patch embedding as an explicit patch matrix times
``proj.weight`` viewed as [C, C_in P P], the normalisation, the ``pos_embed`` rows and the token rows around the patches.
``mut``: a frozenset of mutant names -- wrong programs a gate must tell from the right one (tests/front_cases.py)."""
import torch

NONE = frozenset()
MUTANTS = ("swap_patch", "pixel_major", "no_norm", "times_std", "no_bias", "pos_shift", "pos_all", "after_front",
           "mean_grad")


def rel_err(x, ref) -> float:
    """max|x - ref| / max|ref| (0 / 0 = 0)."""
    ref = ref.detach().double().cpu()
    scale = float(ref.abs().max()) if ref.numel() else 0.0
    diff = float((x.detach().double().cpu() - ref).abs().max()) if ref.numel() else 0.0
    return diff / scale if scale > 0 else diff


def normalize(image, mean, std, mut=NONE):
    """``normalize_image`` on the leading len(mean) channels; the others pass through."""
    if mean is None or "no_norm" in mut:
        return image
    k = len(mean)
    m = torch.as_tensor(mean, dtype=image.dtype, device=image.device).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=image.dtype, device=image.device).view(-1, 1, 1)
    head = (image[:, :k] - m) * s if "times_std" in mut else (image[:, :k] - m) / s
    return torch.cat((head, image[:, k:]), dim=1)


def patch_rows(image, weight, bias, patch, mut=NONE):
    """[B, C_in, H, W] -> [B, N, C]: ``conv2d(stride = kernel = patch).flatten(2).transpose(1, 2)``."""
    b, c_in, h, w = image.shape
    gh, gw, p = h // patch, w // patch, patch
    x = image.reshape(b, c_in, gh, p, gw, p)
    if "swap_patch" in mut:
        x = x.permute(0, 2, 4, 1, 5, 3)                     # the patch transposed
    elif "pixel_major" in mut:
        x = x.permute(0, 2, 4, 3, 5, 1)                     # K as (py, px, c)
    else:
        x = x.permute(0, 2, 4, 1, 3, 5)                     # K as (c, py, px): proj.weight's order
    out = x.reshape(b, gh * gw, c_in * p * p) @ weight.reshape(weight.shape[0], -1).t()
    if bias is not None and "no_bias" not in mut:
        out = out + bias
    return out


def _expand(t, s, mut):
    if t.shape[0] != 1 or s == 1:
        return t if t.shape[0] == s else t.expand(s, -1, -1)
    e = t.expand(s, -1, -1)
    if "mean_grad" in mut:                                  # same values, the gradient divided by the sequences
        e = e / s + (e - e / s).detach()
    return e


def place(body, before, after, mut=NONE):
    """``cat((*before, body, *after), dim=1)`` for body [S, N, C] and tokens [1 or S, k, C]."""
    s = body.shape[0]
    front, back = [_expand(t, s, mut) for t in before], [_expand(t, s, mut) for t in after]
    if "after_front" in mut:
        front, back = back + front, []
    return torch.cat((*front, body, *back), dim=1)


def embed(image, weight, bias, patch, mean=None, std=None, pos_table=None, pos_first=None, before=(), after=(), mut=NONE):
    """What ``spfsplatv2_amd.embed_patches`` returns."""
    rows = patch_rows(normalize(image, mean, std, mut), weight, bias, patch, mut)
    before = list(before)
    if pos_table is not None:
        table = torch.roll(pos_table, 1, dims=0) if "pos_shift" in mut else pos_table
        rows = rows + table
    if pos_first is not None:
        before[0] = torch.cat((before[0][:, :1] + pos_first, before[0][:, 1:]), dim=1)
    out = place(rows, before, after, mut)
    if pos_table is not None and "pos_all" in mut:
        n_before = sum(t.shape[1] for t in before)
        extra = torch.ones(out.shape[1], dtype=torch.bool, device=out.device)
        extra[n_before:n_before + rows.shape[1]] = False
        out = out + extra[None, :, None].to(out.dtype) * pos_table[0]
    return out


def assemble(x, before=(), after=(), mut=NONE):
    """What ``spfsplatv2_amd.assemble_tokens`` returns: x [.., N, C]."""
    lead, c = x.shape[:-2], x.shape[-1]
    flat = lambda t: t.reshape(-1, t.shape[-2], c)          # noqa: E731
    out = place(flat(x), [flat(t) for t in before], [flat(t) for t in after], mut)
    return out.reshape(*lead, out.shape[-2], c)


def eager_embed(image, weight, bias, patch, mean=None, std=None, pos_table=None, pos_first=None, before=(), after=()):
    """The reference's own lines, the yardstick's path: ``(x - mean) / std``, ``conv2d``, ``flatten(2).transpose(1, 2)``,
    the additions and the ``cat``s."""
    x = normalize(image, mean, std)
    rows = torch.nn.functional.conv2d(x, weight, bias, stride=patch).flatten(2).transpose(1, 2)
    if pos_table is not None:
        rows = rows + pos_table
    before = list(before)
    if pos_first is not None:
        before[0] = torch.cat((before[0][:, :1] + pos_first, before[0][:, 1:]), dim=1)
    s = rows.shape[0]
    return torch.cat((*[t.expand(s, -1, -1) for t in before], rows, *[t.expand(s, -1, -1) for t in after]), dim=1)
