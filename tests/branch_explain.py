"""Which branch did the kernel take?  (helper of the parity tests; not collected)

Next to a threshold of the compositing rule -- an alpha at 1/255, an exponent at 0, a transmittance at the 1e-4 stop
-- a float32 evaluation may legitimately decide differently from the float64 oracle.  The parity tests mask those
pixels (oracle/splat_ref.py FRAG_*).  `explain` removes most of that mask again: for every pixel inside one of the
three windows it enumerates the ADMISSIBLE settings of the ambiguous decisions, composites each in float64 from what
the oracle recorded (`decisions`, splat_ref.composite), and asks which of them the observed pixel is.

* exactly one setting within `rgb_tol` of the observed colour and alpha: EXPLAINED.  The oracle is then run again with
  that pixel's keep row forced (`force_keep`): image and gradients of the float64 function on the observed branch.
* two different settings within `rgb_tol`: UNDECIDABLE, the image cannot tell them apart.  The pixel stays masked.
* none: UNEXPLAINED.  The pixel is neither branch of the algorithm -- a defect, never a mask.

Pixels flagged for another reason (depth-order tie, tile membership, SH clamp, the smooth exponent-rounding limit), or
with more than MAX_AMBIGUOUS ambiguous entries, stay masked too.  Everything that stays masked is the RESIDUAL.
"""
from __future__ import annotations

import itertools

import torch

from oracle import splat_ref

MAX_AMBIGUOUS = 4


def _keep_row(alpha, valid, shift):
    """The oracle's keep rule (splat_ref.composite) on one pixel's list for a given validity setting; `shift` moves the
    1e-4 stop by one entry (-1: the last kept entry is refused too, +1: the first refused entry is kept) and returns
    None where that shift is not admissible: the transmittance that decides it is outside the near_T window."""
    a = torch.where(valid, alpha, torch.zeros_like(alpha))
    incl = torch.cumprod(1.0 - a, dim=0)
    keep = valid & (incl >= splat_ref.T_MIN)
    refused = valid & ~keep
    stopped = torch.cumsum(refused.to(torch.int32), dim=0) > 0
    keep = keep & ~stopped
    if shift == 0:
        return keep
    near = (incl - splat_ref.T_MIN).abs() < splat_ref.FRAG_T_REL * splat_ref.T_MIN
    if shift > 0:
        idx = torch.nonzero(refused).flatten()
    else:
        idx = torch.nonzero(keep).flatten().flip(0)
    if idx.numel() == 0 or not bool(near[idx[0]]):
        return None
    keep = keep.clone()
    keep[idx[0]] = shift > 0
    return keep


def composite_row(alpha, keep, rgb, background, scale=None):
    """Colour [3] and alpha of one pixel from its list, float64.  `scale` [L] multiplies the entries' alphas (tests)."""
    a = torch.where(keep, alpha, torch.zeros_like(alpha))
    if scale is not None:
        a = a * scale
    incl = torch.cumprod(1.0 - a, dim=0)
    t_excl = torch.cat([torch.ones_like(incl[:1]), incl[:-1]])
    w = a * t_excl
    return w @ rgb + incl[-1] * background, 1.0 - incl[-1], w


def _settings(alpha, valid0, amb, near_t):
    """Every keep row of the settings of the ambiguous entries `amb`, and the furthest entry any of them can reach (one
    past its stop: the stop itself may shift by one)."""
    rows, seen, reach = [], set(), 0
    for flips in itertools.product((False, True), repeat=len(amb)):
        valid = valid0.clone()
        for i, f in zip(amb, flips):
            if f:
                valid[i] = ~valid[i]
        refused = torch.nonzero(valid & ~_keep_row(alpha, valid, 0)).flatten()
        reach = max(reach, int(refused[0]) + 1 if refused.numel() else alpha.numel())
        for shift in ((0, -1, 1) if bool(near_t.any()) else (0,)):
            keep = _keep_row(alpha, valid, shift)
            if keep is None:
                continue
            key = keep.numpy().tobytes()
            if key not in seen:
                seen.add(key)
                rows.append(keep)
    return rows, reach


def alternatives(alpha, pow_ok, near_alpha, near_pow, near_t):
    """The distinct admissible keep rows of one pixel (the oracle's own first), or None if it has too many ambiguous
    entries.  Only ambiguous entries that some setting can REACH count: an entry beyond the stop (and the one after it)
    changes nothing.  Toggling an entry out moves the stop later, so the reach is taken over all settings and the
    enumeration repeated until it no longer grows."""
    valid0 = pow_ok & (alpha >= splat_ref.ALPHA_MIN)
    all_amb = [int(i) for i in torch.nonzero(near_alpha | near_pow).flatten()]
    _, reach = _settings(alpha, valid0, [], near_t)
    while True:
        amb = [i for i in all_amb if i <= reach]
        if len(amb) > MAX_AMBIGUOUS:
            return None
        rows, new_reach = _settings(alpha, valid0, amb, near_t)
        if len([i for i in all_amb if i <= new_reach]) == len(amb):
            return rows
        reach = new_reach


LIGHT_WEIGHT = 1e-4


def _only_light_entries_differ(alpha, rows, fits):
    """True if the oracle's own row (rows[0]) fits and every other fitting row differs from it only in entries whose
    compositing weight alpha * T is below LIGHT_WEIGHT (T along the oracle's own row)."""
    if fits[0] != 0:
        return False
    own = rows[0]
    a = torch.where(own, alpha, torch.zeros_like(alpha))
    incl = torch.cumprod(1.0 - a, dim=0)
    weight = alpha * torch.cat([torch.ones_like(incl[:1]), incl[:-1]])
    return all(bool((weight[rows[i] ^ own] < LIGHT_WEIGHT).all()) for i in fits[1:])


def explain(decisions, observed_color, observed_alpha, background, H, W, rgb_tol=1e-4, keep_light=False):
    """One (scene, view).  `decisions`: what splat_ref.rasterize(..., decisions={}) recorded; `observed_color` [3,H,W],
    `observed_alpha` [1,H,W]: the implementation under test; `background` [3].

    Returns (force_keep, residual, counters, unexplained):
      force_keep  {(tx, ty): bool [256, L]} for the tiles with an explained pixel on another branch than the oracle's;
      residual    [H,W] bool, the pixels that stay masked;
      counters    flagged (by a window), explained, took_other_branch, undecidable, undecidable_light, too_many, also_other (inside a window AND flagged
                  for another reason), other (all pixels flagged for another reason), residual, unexplained;
      unexplained [(x, y, best distance, oracle's own distance)].
    `keep_light`: an undecidable pixel whose candidate rows differ from the oracle's own only in entries of weight
    alpha * T < 1e-4 is NOT masked; it is compared on the oracle's own branch (counted `undecidable_light`).
    """
    T = splat_ref.TILE
    obs_c = observed_color.detach().double().cpu()
    obs_a = observed_alpha.detach().double().cpu().reshape(H, W)
    bg = torch.as_tensor(background, dtype=torch.float64)
    other = decisions.get("other")
    residual = torch.zeros(H, W, dtype=torch.bool) if other is None else other.clone()
    cnt = dict(flagged=0, explained=0, took_other_branch=0, undecidable=0, undecidable_light=0, too_many=0, also_other=0,
               other=0, unexplained=0)
    force, unexplained = {}, []
    for (tx, ty), rec in decisions.get("tiles", {}).items():
        rgb = rec["rgb"].double()
        forced = None
        for r, row in enumerate(rec["rows"].tolist()):
            x, y = tx * T + row % T, ty * T + row // T
            if x >= W or y >= H:
                continue
            cnt["flagged"] += 1
            if bool(residual[y, x]):            # also flagged for a reason that is no keep decision
                cnt["also_other"] += 1
                continue
            alpha = rec["alpha"][r].double()
            rows = alternatives(alpha, rec["pow_ok"][r], rec["near_alpha"][r], rec["near_pow"][r], rec["near_T"][r])
            if rows is None:
                cnt["too_many"] += 1
                residual[y, x] = True
                continue
            dist = []
            for keep in rows:
                c, a, _ = composite_row(alpha, keep, rgb, bg)
                dist.append(max(float((c - obs_c[:, y, x]).abs().max()), abs(float(a) - float(obs_a[y, x]))))
            fits = [i for i, d in enumerate(dist) if d <= rgb_tol]
            if len(fits) == 1:
                cnt["explained"] += 1
                if not torch.equal(rows[fits[0]], rec["keep"][row]):
                    cnt["took_other_branch"] += 1
                    if forced is None:
                        forced = rec["keep"].clone()
                    forced[row] = rows[fits[0]]
            elif len(fits) > 1:
                cnt["undecidable"] += 1
                if keep_light and _only_light_entries_differ(alpha, rows, fits):
                    cnt["undecidable_light"] += 1
                else:
                    residual[y, x] = True
            else:
                cnt["unexplained"] += 1
                unexplained.append((x, y, min(dist), dist[0]))
                residual[y, x] = True           # (masked so that the other gates still speak; the count is the failure)
        if forced is not None:
            force[(tx, ty)] = forced
    cnt["other"] = 0 if other is None else int(other.sum())
    cnt["residual"] = int(residual.sum())
    return force, residual, cnt, unexplained
