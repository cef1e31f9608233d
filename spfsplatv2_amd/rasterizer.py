"""Host side of the MI355X Gaussian-splat rasterizer.

Two surfaces over the same HIP library (C ABI in include/spfsplat_hip.h):

* ``GaussianRasterizationSettings`` / ``GaussianRasterizer`` -- the exact call surface the reference
  uses (/root/reference/src/model/decoder/cuda_splatting.py:105-138): one (scene, view) per call,
  keyword arguments, 6-tuple result ``(image, depth, norm, alpha, radii, extra)``.
* ``rasterize_batch`` -- S scenes x V views in ONE launch chain sharing each scene's Gaussian
  buffers (what the Python loop at cuda_splatting.py:96-143 plus the ``repeat`` copies at
  decoder_splatting_cuda.py:59-64 amount to).  This is what fills 256 CUs at 256x256.

PyTorch is plumbing here (device memory, current stream, autograd bookkeeping); all arithmetic is
in the HIP kernels.  There is no CPU path: tensors must live on a HIP device.
"""
from __future__ import annotations

import ctypes as C
import inspect
import os
from collections import namedtuple
from typing import NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib

__all__ = ["GaussianRasterizationSettings", "GaussianRasterizer", "rasterize_batch", "render_batch", "camera_forward", "StaticStep",
           "last_forward_stats", "PairBudget", "plan_pair_budget", "last_plan_flags", "plan_flags", "CallRecord",
           "sh_band4_default", "gaussian_normals"]

_REC = 12


class CallRecord(dict):
    """What one forward call left behind: ``num_pairs / max_tile_list / dense_tiles / tiles`` (exact mode) and, for a
    planned call, ``counters`` -- the device tensor whose element 2 is the plan verdict.  Pass your own instance as
    ``record=`` to keep the calls of several decoders / threads apart; without one the process-wide ``_last`` is used
    (what ``last_forward_stats`` / ``last_plan_flags`` read)."""


_last = CallRecord()


_warned_band4 = False


def _note_band4_not_evaluated(sh_degree: int, sh_band4: bool) -> None:
    """One warning per process when a d_sh = 25 model (sh_degree 4: the reference's shipped configuration,
    config/model/encoder/spfsplatv2.yaml:20) is rendered WITHOUT band 4 because nobody chose: whether the `pose` fork
    evaluates band 4 cannot be checked offline (oracle/PINNING.md row 9b) -- an open parity risk, not a settled
    default; `SPF_SH_BAND4=1` / `decoder.sh_band4 = True` / `settings.sh_band4` evaluate it."""
    global _warned_band4
    if sh_degree == 4 and not sh_band4 and not _warned_band4 and "SPF_SH_BAND4" not in os.environ:
        _warned_band4 = True
        import warnings
        warnings.warn("spfsplatv2_amd: sh_degree 4 (25 SH coefficients) is evaluated to degree 3 like the published 3DGS "
                      "kernels; whether the reference's rasterizer fork evaluates band 4 is unknown (oracle/PINNING.md). "
                      "Set SPF_SH_BAND4=1 (or sh_band4=True) to evaluate it, SPF_SH_BAND4=0 to silence this note.",
                      stacklevel=4)


def sh_band4_default() -> bool:
    """Whether SH band 4 of a d_sh = 25 model is evaluated when the caller does not say: the ``SPF_SH_BAND4``
    environment variable ("1" = yes).  Default off: the published 3DGS kernels stop at degree 3 and only carry the
    25-coefficient stride; the `pose` fork's behaviour cannot be checked offline."""
    return os.environ.get("SPF_SH_BAND4", "0") == "1"


class PairBudget(NamedTuple):
    """A PLAN for the (Gaussian, tile) pair buffer, taken from an earlier call on similar inputs, so that a call
    needs no device->host read-back (and can be captured in a HIP graph).  The plan is verified on the device:
    see ``last_plan_flags``.

    capacity       pair-buffer entries to allocate
    max_tile_list  assumed upper bound of the longest tile list (0 = unknown: all sort size classes are launched)
    check          "backward": the backward pass reads the flag (one host sync) and raises if the plan failed (a call
                   that will have no backward verifies at once; ``DecoderSplattingCUDA``'s replayed evaluation graphs
                   re-run such a call in exact mode instead of raising);
                   "deferred": the library never reads it -- call ``last_plan_flags()`` when convenient;
                   "early": the FORWARD verifies and raises, at the cost of one short wait -- with direct bins the verdict
                   is final when the projection kernel has run, so it is copied to pinned memory right behind that kernel,
                   the rest of the chain (sort, compositing) is issued, and only then does the host wait for the copy:
                   the GPU keeps working through the wait (exact mode's read-back sits at the same point of the chain but
                   with nothing issued behind it).  What ``DecoderSplattingCUDA`` uses for its own planning.  (Calls that
                   cannot run with direct bins, and calls through the compiled per-view binding, verify when the whole
                   forward has been issued; under stream capture nothing is read: the flag stays for the caller.)
    """
    capacity: int
    max_tile_list: int = 0
    check: str = "backward"


_SORT_CLASSES = (128, 256, 512, 1024, 2048, 4096, 8192, 16384)


def plan_pair_budget(stats: Optional[dict] = None, slack: float = 1.25, check: str = "backward") -> PairBudget:
    """Budget for the next calls from the statistics of an exact-mode call (default: the most recent one, see
    ``last_forward_stats``): ``slack`` x the pairs it produced and the list-length class its longest list (x slack) falls
    in.  (Rounds 2 - 4 also planned which of two compositing kernels to launch from the call's dense-tile census; one
    kernel composites every tile now, so there is nothing left to assume -- ``dense_tiles`` stays a statistic.)"""
    st = dict(_last if stats is None else stats)
    if "num_pairs" not in st:
        raise RuntimeError("plan_pair_budget needs the statistics of an exact-mode forward call (max_pairs=None)")
    want = int(st["max_tile_list"] * slack) + 1
    max_tile = next((c for c in _SORT_CLASSES if c >= want), 0)
    return PairBudget(int(st["num_pairs"] * slack) + 1024, max_tile, check)


def plan_flags(record: Optional[CallRecord] = None) -> int:
    """Device-side verdict on the plan of a planned forward call (synchronises with the device): 0 = the plan held;
    bit 1 = pair buffer too small, bit 2 = a tile list longer than planned.
    Non-zero: that call's outputs and its backward's gradients are all NaN (never garbage) -- re-run it in exact mode
    or with a larger budget.  `record`: the CallRecord the call was given (default: the process-wide last call)."""
    c = (_last if record is None else record).get("counters")
    return 0 if c is None else int(c[2])


def last_plan_flags() -> int:
    """``plan_flags()`` of the most recent planned forward call in this process."""
    return plan_flags(None)


def last_forward_stats() -> dict:
    """{'num_pairs': D, 'max_tile_list': n, ...} of the most recent exact-mode forward call in this process."""
    return {k: v for k, v in _last.items() if k != "counters"}


_ptr = _lib.ptr


def _f32c(t: Tensor, name: str, shape: tuple) -> Tensor:
    if not isinstance(t, Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} is on {t.device}: the rasterizer only runs on a HIP device "
                           "(there is no CPU fallback)")
    if tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    return t.contiguous()


_bg_cache: dict = {}     # id(source) -> (weakref to the source, its version, S, V, expanded copy)


def _background(bg: Tensor, S: int, V: int) -> Tensor:
    """Background colours as a contiguous [S,V,3] tensor.  A single colour [3] is broadcast once and the copy is
    reused for as long as the caller passes the same, unmodified tensor (a decoder's `background_color` buffer):
    no per-call expand kernel."""
    if bg.dim() != 1:
        return _f32c(bg, "bg", (S, V, 3))
    import weakref
    hit = _bg_cache.get(id(bg))
    if hit is not None and hit[0]() is bg and hit[1:4] == (bg._version, S, V):
        return hit[4]
    out = _f32c(bg.expand(S, V, 3), "bg", (S, V, 3))
    if len(_bg_cache) >= 16:
        _bg_cache.clear()
    _bg_cache[id(bg)] = (weakref.ref(bg), bg._version, S, V, out)
    return out


_tanfov_cache: dict = {}


def _tanfov_tensor(tx: float, ty: float, device) -> Tensor:
    """[1,1,2] device tensor of a settings object's two Python floats.  The reference builds its settings from
    `.item()` values once per view (cuda_splatting.py:108-109) and a training run sees the same few cameras' values
    again and again: the host->device copy is paid once per value pair.  A cached tensor is shared by every later call
    on ANY stream, so (a) a miss waits for its copy (one stream synchronisation per new value pair -- the reference's
    glue has just synchronised twice for the `.item()`s that produced the pair) and (b) cached tensors are never
    released: the caching allocator cannot hand their memory to someone else while a side stream still reads it.  Beyond
    4096 pairs new values are simply not cached."""
    key = (tx, ty, device)
    t = _tanfov_cache.get(key)
    if t is None:
        src = torch.tensor([[[tx, ty]]], dtype=torch.float32)
        if torch.cuda.is_current_stream_capturing():
            # (a miss inside a HIP-graph capture: a pageable copy is illegal there; stage through pinned memory, uncached)
            return src.pin_memory().to(device, non_blocking=True)
        t = src.to(device)
        if len(_tanfov_cache) < 4096:
            torch.cuda.current_stream(t.device).synchronize()
            _tanfov_cache[key] = t
    return t


def raw_rows(raw: Tensor, d_in: int) -> Tensor:
    """`raw` as [N, d_in] rows a kernel can read IN PLACE: unit stride along the channels, ONE row stride over all the
    leading dimensions.  The encoder hands over `gaussians[..., 1:]`, a view into its 83-channel head output
    (encoder_spfsplatv2.py:261-268): that qualifies -- no contiguous copy, 328 bytes per Gaussian read and written less.
    Anything else (a permuted tensor, another dtype) is copied once."""
    if raw.dtype == torch.float32 and raw.stride(-1) == 1:
        rs, span, ok = None, None, True
        for size, stride in zip(reversed(raw.shape[:-1]), reversed(raw.stride()[:-1])):
            if size == 1:
                continue                       # (unit dimensions -- "b v r srf () c" -- carry no stride of their own)
            if rs is None:
                rs = span = stride
                ok = rs >= d_in
            elif stride != span:
                ok = False
            if not ok:
                break
            span *= size
        if ok:
            n = raw.numel() // d_in
            return raw.as_strided((n, d_in), (d_in if rs is None else rs, 1), raw.storage_offset())
    return raw.reshape(-1, d_in).contiguous().float()


COV_EXCLUSIVE = "Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!"


def _cov6(cov3D: Tensor, S: int, G: int) -> Tensor:
    """Precomputed covariances as the [S,G,6] packed upper triangle (xx, xy, xz, yy, yz, zz) the kernels read.  A full
    [S,G,3,3] matrix is packed as cov[..., row, col] with (row, col) = triu_indices(3, 3): the lower triangle is never
    read, and autograd puts each off-diagonal gradient on the upper entry.  (Six basic-index slices, not an index
    tensor: a host index tensor is copied to the device -- a synchronising copy, forward and backward -- which a planned
    call must not make and a graph capture does not allow.)"""
    if not isinstance(cov3D, Tensor):
        raise TypeError("cov3D must be a torch.Tensor")
    if tuple(cov3D.shape) == (S, G, 3, 3):
        cov3D = torch.stack([cov3D[..., 0, 0], cov3D[..., 0, 1], cov3D[..., 0, 2], cov3D[..., 1, 1], cov3D[..., 1, 2],
                             cov3D[..., 2, 2]], dim=-1)
    return _f32c(cov3D, "cov3D", (S, G, 6))


def _check_camera(extrinsics, intrinsics, near, far, S: int, V: int):
    """The camera block of a call, [S,V,4,4] / [S,V,3,3] / [S,V] / [S,V], as dense float32 device tensors."""
    return (_f32c(extrinsics, "extrinsics", (S, V, 4, 4)), _f32c(intrinsics, "intrinsics", (S, V, 3, 3)),
            _f32c(near, "near", (S, V)), _f32c(far, "far", (S, V)))


def _check_gaussians(means3D, scales, rotations, opacities, cov3D, S: int, G: int, pair: bool = True):
    """The Gaussian block: means [S,G,3], then the scale/rotation pair or `cov3D` (neither with `pair` False: raw rows
    carry them), then the opacities as [S,G] -> (means3D, scales, rotations, opacities, cov3D [S,G,6])."""
    means3D = _f32c(means3D, "means3D", (S, G, 3))
    if cov3D is not None:
        cov3D = _cov6(cov3D, S, G)
    elif pair:
        scales, rotations = _f32c(scales, "scales", (S, G, 3)), _f32c(rotations, "rotations", (S, G, 4))
    return means3D, scales, rotations, _f32c(opacities.reshape(S, G), "opacities", (S, G)), cov3D


def _check_sh(S, G, sh_degree, sh_band4, shs=None, sh_layout="gk3", shs_high=None, raw=None, sh_mask=None):
    """The harmonics, however they come -- `shs` [S,G,K,3] ("gk3") or [S,G,3,K] ("g3k"), band-split with `shs_high`
    [S,G,3,9], raw rows [.., 7+3K] with their `sh_mask` [K], or none (colours) -> (shs, shs_high, sh_mask, K,
    SpfDims.sh_layout, sh_band4).  `sh_band4` None is resolved FIRST: the count is held against the degree evaluated."""
    if sh_layout not in ("gk3", "g3k"):
        raise RuntimeError(f"sh_layout must be 'gk3' or 'g3k', got {sh_layout!r}")
    layout = 1 if sh_layout == "g3k" else 0
    if sh_band4 is None:
        sh_band4 = sh_band4_default()
        _note_band4_not_evaluated(sh_degree, sh_band4)
    fewest = (min(sh_degree, 4 if sh_band4 else 3) + 1) ** 2
    if raw is not None and (not isinstance(raw, Tensor) or not raw.is_cuda or raw.dtype != torch.float32):
        raise RuntimeError("raw must be a float32 tensor on a HIP device (there is no CPU fallback)")
    K = _sh_coefficients(shs, 2 if shs_high is not None else layout, raw)
    if raw is not None:
        if raw.shape[-1] != 7 + 3 * K or K < 1 or raw.numel() != S * G * raw.shape[-1]:
            raise RuntimeError(f"raw must hold S*G = {S * G} rows of 7 + 3*d_sh channels, got {tuple(raw.shape)}")
        if not (0 <= sh_degree <= 4) or K < fewest:
            raise RuntimeError(f"raw holds {K} coefficients per channel, too few for sh_degree {sh_degree}")
        if sh_mask is None:
            raise RuntimeError("raw rows need the adapter's sh_mask")
        sh_mask, layout = _f32c(sh_mask, "sh_mask", (K,)), 3
    elif shs_high is not None:
        if shs is None or not layout:
            raise RuntimeError("shs_high (band 4 of the band-split layout) goes with shs [S,G,3,16] and sh_layout='g3k'")
        shs, shs_high, layout = _f32c(shs, "shs", (S, G, 3, 16)), _f32c(shs_high, "shs_high", (S, G, 3, 9)), 2
    elif shs is not None:
        if K < fewest:
            raise RuntimeError(f"shs holds {K} coefficients, too few for sh_degree {sh_degree}")
        shs = _f32c(shs, "shs", (S, G, 3, K) if layout else (S, G, K, 3))
    if not (0 <= sh_degree <= 4):
        raise RuntimeError(f"sh_degree {sh_degree} outside 0..4")
    return shs, shs_high, sh_mask, K, layout, bool(sh_band4)


_stream_ptr = _lib.stream_ptr


def _on_device_of_first_arg(fn):
    """HIP launches go to the CURRENT device: make the tensors' device current for the duration of the call."""
    import functools

    @functools.wraps(fn)
    def wrapped(first, *a, **kw):
        t = first[0] if isinstance(first, (tuple, list)) else first
        with torch.cuda.device(t.device):
            return fn(first, *a, **kw)
    return wrapped


_early_cache: dict = {}


def _early_verdict(dev: torch.device):
    """(pinned int32[1], event) of a device, for check="early" plans: one pair per device and host thread is enough --
    a forward call has read its verdict before it returns."""
    import threading
    key = (dev.index, threading.get_ident())
    got = _early_cache.get(key)
    if got is None:
        got = _early_cache[key] = (torch.empty(1, dtype=torch.int32, pin_memory=True), torch.cuda.Event())
    return got


_Inputs = namedtuple("_Inputs", [f for f, _ in _lib.SpfInputs._fields_], defaults=(None,) * 5)   # SpfInputs, field for field
_State = namedtuple("_State", "rec radii rect tiles pairs pair_idx final_T n_contrib")            # what a forward leaves behind
_Geometry = namedtuple("_Geometry", "S V G K sh_degree H W scale_modifier sh_layout sh_band4 plan_mode")   # (_plan_mode)
_Plan = namedtuple("_Plan", "dense bin_cap capacity")   # dense-tile hint, bin size (0: packed lists), pair = record capacity
_Forward = namedtuple("_Forward", "outs state plan")      # _forward_impl's; outs: (image, depth, alpha, radii [S,V,G])
# every gradient under its input's name, None where absent (`view`: dL/dviewmatrix, or its per-block partial sums)
_Grads = namedtuple("_Grads", "means3D scales rotations opacities shs colors view means2D shs_high raw cov3D",
                    defaults=(None,) * 3)
_SAVED = _Inputs._fields + _State._fields + ("cov3D", "near")    # save_for_backward's order, both autograd functions


def _saved(ctx):
    """ctx.saved_tensors by name: (dict, _Inputs, _State)."""
    t = dict(zip(_SAVED, ctx.saved_tensors))
    return t, _Inputs(*map(t.get, _Inputs._fields)), _State(*map(t.get, _State._fields))


def _input_grads(args: tuple, g: _Grads, **other) -> tuple:
    """backward's result, one slot per name in `args` (forward's inputs): `other`'s gradient, else `g`'s, else None."""
    named = {**g._asdict(), **other}
    return tuple(named.get(a) for a in args)


def _sh_coefficients(shs, sh_layout: int, raw=None) -> int:
    """SpfDims.K from the tensors of a call (raw rows: 7 + 3K channels; band split: 16 + 9 = 25; colours: 0)."""
    if raw is not None:
        return (raw.shape[-1] - 7) // 3
    if shs is None:
        return 0
    return 25 if sh_layout == 2 else shs.shape[3 if sh_layout else 2]


def _geometry(i: _Inputs, sh_degree, H, W, scale_modifier, sh_layout, sh_band4, max_pairs) -> _Geometry:
    (S, G, _), V = i.means3D.shape, i.viewmatrix.shape[1]
    return _Geometry(S, V, G, _sh_coefficients(i.shs, sh_layout, i.raw), sh_degree, H, W, float(scale_modifier),
                     int(sh_layout), bool(sh_band4), _plan_mode(max_pairs))


def _dims(g: _Geometry, bin_cap: int, rec_cap: int, raw=None, adapter_eps: float = 0.0):
    return _lib.SpfDims(g.S, g.V, g.G, g.K, g.sh_degree, g.H, g.W, g.scale_modifier, g.sh_layout, int(g.sh_band4),
                        int(bin_cap), int(rec_cap) if bin_cap else 0, 0 if raw is None else raw.stride(0), float(adapter_eps))


def _inputs_struct(inputs: _Inputs):
    return _lib.SpfInputs(*map(_ptr, inputs))


@_on_device_of_first_arg
def _forward_impl(means3D, scales, rotations, opacities, shs, colors, viewmatrix, projmatrix, tanfov, bg,
                  view_scale, H, W, sh_degree, scale_modifier, max_pairs, sh_layout=0, camera=None, sh_band4=False,
                  record=None, nothing_needs_grad=False, view64=None, shs_high=None, raw=None, sh_mask=None,
                  adapter_eps=0.0, cov3D=None) -> _Forward:
    """Launch the forward chain.  `camera` (an SpfCamera whose outputs are viewmatrix / projmatrix / tanfov / view_scale):
    the decoder fast path -- camera set-up and the clearing of the tile counters are one kernel.  `cov3D` [S,G,6] (scales /
    rotations None): precomputed covariances, through the ctypes path always (the compiled binding does not take them)."""
    lib = _lib.load()
    inputs = _Inputs(means3D, scales, rotations, opacities, shs, colors, viewmatrix, projmatrix, tanfov, bg, view_scale,
                     view64, shs_high, raw, sh_mask)
    geom = _geometry(inputs, sh_degree, H, W, scale_modifier, sh_layout, sh_band4, max_pairs)
    S, V, G, R, dev = geom.S, geom.V, geom.G, geom.S * geom.V, means3D.device
    rec_out = _last if record is None else record
    T, nblk = lib.spf_raster_num_tiles(H, W), lib.spf_raster_view_partial_blocks(G)
    fast = _lib.fast() if (camera is None and cov3D is None) else None
    if fast is not None:
        # the same chain through the compiled binding (csrc/torch_binding.cpp): allocation, structs, launches and the
        # exact-mode read-back in C++ -- what a per-view caller of the drop-in surface pays b*v times per step
        capacity, max_tile, dense = (-1, 0, 0) if max_pairs is None else _plan_numbers(max_pairs, R * T)
        with _spf_errors():
            ts, (D, max_tile, dense, RT) = fast.raster_forward(
                means3D, scales, rotations, opacities, shs, colors, viewmatrix, projmatrix, tanfov, bg, view_scale,
                view64, H, W, sh_degree, float(scale_modifier), int(sh_layout), bool(sh_band4), capacity, max_tile, dense)
        image, depth, alpha, radii_v, rec, rect, tiles, pairs, pair_idx, final_T, n_contrib = ts
        lay = _layout(RT, R * G, R * nblk)
        counters = tiles[lay.counters:lay.pair_cursor]
        if max_pairs is None:
            rec_out.update(num_pairs=D, max_tile_list=max_tile, dense_tiles=dense, tiles=RT, counters=None)
            if rec_out is not _last:
                _last.update(rec_out)
        else:
            rec_out["counters"] = counters
            _last["counters"] = counters
            early = isinstance(max_pairs, PairBudget) and max_pairs.check == "early"
            if ((geom.plan_mode == 1 and nothing_needs_grad) or early) and not torch.cuda.is_current_stream_capturing():
                _raise_if_plan_failed(counters, pairs.numel())
        return _Forward((image, depth, alpha, radii_v),
                        _State(rec, radii_v.view(-1), rect, tiles, pairs, pair_idx, final_T, n_contrib),
                        _Plan(dense, 0, pairs.numel()))
    # DIRECT BINS (planned calls): every tile owns a fixed bin of `bin_cap` keys that the projection kernel fills itself
    # -- no tile scan, no binning pass (SpfDims.bin_cap).  The bin size is the plan's list-length class.
    bin_cap = _direct_bin_cap(max_pairs, R * T, T)
    # gradient records the backward will allocate: the plan's capacity -- with headroom when the pair numbering is
    # sharded (each of 8 shards owns an eighth: see _record_capacity)
    rec_cap = _record_capacity(_plan_numbers(max_pairs, R * T)[0], S, G) if bin_cap else 0
    dims = _dims(geom, bin_cap, rec_cap, raw, adapter_eps)
    state, lay = _alloc_state(dev, R, G, T, nblk, H * W)
    image, depth, alpha = _alloc_outputs(dev, S, V, H, W)
    views = _slice_state(lay, state.rect, state.tiles, state.pair_idx)
    tiles, counters = state.tiles, views.counters
    inp = _inputs_struct(inputs)
    if bin_cap:
        state = state._replace(pairs=torch.empty((R * T * bin_cap,), dtype=torch.int64, device=dev))
    # check="early" with direct bins: the projection kernel mirrors a raised plan flag into a pinned word the host reads
    # behind an event -- no device->host copy on the stream (SpfState.verdict_host)
    early = None
    if isinstance(max_pairs, PairBudget) and max_pairs.check == "early" and not torch.cuda.is_current_stream_capturing():
        early = _early_verdict(dev)
        early[0].zero_()
    # (a caller that captures the call in a graph hands its own pinned word over in the call record: the decoder's
    #  evaluation graphs read it behind a stream synchronisation instead of copying counters[2] back)
    vh = early[0] if early is not None else rec_out.get("verdict_host")
    st = _state_struct(state, views, verdict_host=vh if bin_cap else None)
    rec_out["verdict_mirrored"] = bool(bin_cap and vh is not None)
    stream = _stream_ptr(dev)
    # camera set-up, with the clearing of ALL the tile bookkeeping in the same kernel where the buffer's alignment allows
    # it (the scan then needs no single-block pass: see spf_tile_scan_render_kernel); then the projection
    cleared = 0
    if camera is not None and tiles.data_ptr() % 16 == 0:
        cleared = 4 * tiles.numel()
        _lib.check(lib.spf_decoder_prepare(C.byref(camera), _ptr(tiles), cleared, stream), "spf_decoder_prepare")
    elif camera is not None:
        _lib.check(lib.spf_camera_forward(C.byref(camera), stream), "spf_camera_forward")
    if cov3D is not None:
        _lib.check(lib.spf_raster_forward_project_cov3d(C.byref(dims), C.byref(inp), _ptr(cov3D), C.byref(st), cleared,
                                                        stream), "spf_raster_forward_project_cov3d")
    elif cleared:
        _lib.check(lib.spf_raster_forward_project_prepared(C.byref(dims), C.byref(inp), C.byref(st), cleared, stream),
                   "spf_raster_forward_project_prepared")
    else:
        _lib.check(lib.spf_raster_forward_project(C.byref(dims), C.byref(inp), C.byref(st), stream),
                   "spf_raster_forward_project")
    if max_pairs is None:
        # exact mode: one 16-byte read-back per BATCH (the reference syncs twice per view,
        # cuda_splatting.py:108-109, plus once inside its rasterizer)
        host = counters.cpu()
        D, max_tile, dense = int(host[0]), int(host[1]), int(host[3])
        capacity = D
        rec_out.update(num_pairs=D, max_tile_list=max_tile, dense_tiles=dense, tiles=R * T, counters=None)
        if rec_out is not _last:
            _last.update(rec_out)
    else:
        capacity, max_tile, dense = _plan_numbers(max_pairs, R * T)
        if bin_cap:
            capacity = rec_cap
        rec_out["counters"] = counters
        _last["counters"] = counters
        rec_out["plan"] = _last["plan"] = (int(bin_cap), int(capacity), lib.spf_raster_pair_shards(S, G) if bin_cap else 1)
    if early is not None and bin_cap:      # direct bins: the projection kernel has binned -- the verdict is final behind it
        early[1].record()
    if not bin_cap:
        state = state._replace(pairs=torch.empty((max(capacity, 1),), dtype=torch.int64, device=dev))
        st.pairs = _ptr(state.pairs)
    out = _lib.SpfOutputs(_ptr(image), _ptr(depth), _ptr(alpha))
    _lib.check(lib.spf_raster_forward_render(C.byref(dims), C.byref(inp), C.byref(st), C.byref(out),
                                             capacity, max_tile, dense, stream),
               "spf_raster_forward_render")
    if early is not None:
        if bin_cap:
            early[1].synchronize()                   # (waits for the projection kernel and 4 bytes, not for the chain)
            failed = early[0].item() != 0
        else:
            failed = True                            # classic chain: the binning kernel decides -- read it the slow way
        if failed:
            _raise_if_plan_failed(tiles[lay.counters:], capacity, rec_out.get("plan"))
    if geom.plan_mode == 1 and nothing_needs_grad and not torch.cuda.is_current_stream_capturing():
        # check="backward" promises that a failed plan raises -- but no backward will come (evaluation under
        # no_grad, or nothing requires grad): verify now (one host sync; eval loops should use exact mode anyway)
        _raise_if_plan_failed(tiles[lay.counters:], capacity, rec_out.get("plan"))
    return _Forward((image, depth, alpha, state.radii.view(S, V, G)), state, _Plan(dense, bin_cap, max(int(capacity), 1)))


def _alloc_state(dev, R: int, G: int, T: int, nblk: int, P: int):
    """What a forward keeps for its backward, sized by the library: (_State with `pairs` None, its SpfStateLayout)."""
    lay = _layout(R * T, R * G, R * nblk)
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    rec, radii = torch.empty((R * G, _REC), **f32), torch.empty((R * G,), **i32)
    rect, pair_idx = torch.empty((lay.rect_words,), **i32), torch.empty((lay.pair_idx_words,), **i32)
    tiles = torch.empty((lay.tiles_words,), **i32)
    return _State(rec, radii, rect, tiles, None, pair_idx, torch.empty((R * P,), **f32), torch.empty((R * P,), **i32)), lay


def _alloc_camera(dev, S: int, V: int, scale_invariant: bool = True):
    """What the camera kernel writes: (viewmatrix, projmatrix [S,V,4,4], tanfov [S,V,2], view_scale [S,V] or None, the pose
    once more in float64 with the world scale folded in -- SpfInputs.viewmatrix64: the view-space position comes from it)."""
    f32 = dict(dtype=torch.float32, device=dev)
    return (torch.empty((S, V, 4, 4), **f32), torch.empty((S, V, 4, 4), **f32), torch.empty((S, V, 2), **f32),
            torch.empty((S, V), **f32) if scale_invariant else None, torch.empty((S, V, 4, 4), dtype=torch.float64, device=dev))


def _alloc_outputs(dev, S: int, V: int, H: int, W: int):
    """(image [S,V,3,H,W], depth [S,V,1,H,W], alpha [S,V,1,H,W]); colour and depth are two views of ONE allocation,
    colour first (the decoder module's captured evaluation graphs copy both out with a single clone)."""
    n, f32 = S * V * H * W, dict(dtype=torch.float32, device=dev)
    img_dep = torch.empty((4 * n,), **f32)
    return img_dep[:3 * n].view(S, V, 3, H, W), img_dep[3 * n:].view(S, V, 1, H, W), torch.empty((S, V, 1, H, W), **f32)


def _direct_bin_cap(max_pairs, RT: int, T: int) -> int:
    """Bin size of a planned call that runs with DIRECT BINS (0: packed lists, the classic chain).  Needs a plan with a
    list-length class (PairBudget.max_tile_list), the per-render tile histogram in LDS (the library's limit,
    spf_raster_max_lds_tiles) and bins that stay in proportion to the plan: R*T*cap keys <= 8 x the planned pairs (a
    coarse list class on a many-tile call would otherwise hold far more than the classic chain's memory until the
    backward; calls may use up to 2^24 keys = 128 MiB regardless: BASELINE config 3's eight renders of ~1,700-entry lists
    sit in 4,096-entry bins, 6 x their pairs) and <= 2^27 in any case; `SPF_DIRECT_BINS=0` pins the classic chain (A/B
    runs)."""
    if max_pairs is None or os.environ.get("SPF_DIRECT_BINS", "1") == "0":
        return 0
    cap = max_pairs.max_tile_list if isinstance(max_pairs, PairBudget) else 0
    if cap <= 0 or T > _lib.load().spf_raster_max_lds_tiles():
        return 0
    keys = RT * cap
    if keys > (1 << 27) or keys > max(8 * int(max_pairs.capacity), 1 << 24):
        return 0
    return int(cap)


def _record_capacity(capacity: int, S: int, G: int) -> int:
    """Gradient records (`gpair`) of a direct-bins call.  The projection kernel numbers the (Gaussian, tile) pairs from
    up to eight sharded cursors (block b -> shard b % 8; one cursor would be a hot word), each shard owning an eighth of
    the records, and raises plan flag 1 when ONE shard outgrows its share -- so with the plan's bare capacity a call
    whose pairs fit in total could fail on the imbalance of the deal.  Shard b % 8 takes every eighth block of
    256 consecutive Gaussians of EVERY scene, i.e. eight interleaved samples of the same scenes: their pair counts differ
    by a few per cent, not by factors, so each shard gets a quarter more than its fair share on top of the plan's own slack
    (round 5 gave 2x: with the module's default slack of 1.5 that was 3x exact mode's records, 40 bytes each, committed
    by the allocator in every backward -- ADVICE r5).  A deal that is more lopsided raises flag 1 like any plan that does
    not hold: exact re-run and a new plan (module), or the caller's larger capacity."""
    shards = _lib.load().spf_raster_pair_shards(S, G)
    return int(capacity) + (int(capacity) // 4 if shards > 1 else 0)


def _plan_numbers(max_pairs, RT: int):
    """(capacity, longest-list hint, dense-tile hint) of a planned call as spf_raster_forward_render takes them (the
    last is ignored by the library since one kernel composites every tile: always SPF_UNKNOWN)."""
    plan = max_pairs if isinstance(max_pairs, PairBudget) else PairBudget(int(max_pairs))
    return int(plan.capacity), int(plan.max_tile_list), 0xFFFFFFFF


class _spf_errors:
    """Library failures raised inside the compiled binding arrive as RuntimeError("SPF: ..."): re-raise them as the
    SpfError the ctypes path raises (everything else -- out of memory, a bad tensor -- passes through unchanged)."""

    def __enter__(self):
        return self

    def __exit__(self, et, ev, tb):
        if et is RuntimeError and str(ev).startswith("SPF: "):
            raise _lib.SpfError(str(ev)[5:]) from None
        return False


class StateViews(NamedTuple):
    """The fields of SpfState that share a buffer, as named views of the three tensors a forward call returns them in
    (`rect`, `tiles`, `pair_idx`).  Where each field starts is the library's word (spf_raster_state_layout)."""
    rect: Tensor                    # [RG]      packed tile rect
    zkey: Tensor                    # [RG...]   depth key (float bits), then the SH clamp bytes
    sh_clamp: Optional[Tensor]      # [..]      SH clamp masks (None: the buffer holds none)
    tile_count: Tensor              # [RT]
    tile_flags: Tensor              # [RT]
    tile_start: Tensor              # [RT + 1]  (direct bins, >= 2,048 tiles: the launch order [RT][2] starts here)
    tile_fill: Tensor               # [RT]
    counters: Tensor                # [4]
    pair_cursor: Optional[Tensor]   # [8]       (None: the buffer is too short to hold them)
    pair_off: Tensor                # [2 RG]    (rect, first pair) per (render, Gaussian)
    blk_total: Tensor               # [RB]
    blk_base: Tensor                # [RB...]


def _layout(RT: int, RG: int, RB: int):
    lay = _lib.SpfStateLayout()
    _lib.check(_lib.load().spf_raster_state_layout(RT, RG, RB, C.byref(lay)), "spf_raster_state_layout")
    return lay


def _slice_state(lay, rect, tiles, pair_idx) -> StateViews:
    return StateViews(
        rect=rect[:lay.zkey], zkey=rect[lay.zkey:], sh_clamp=rect[lay.sh_clamp:] if rect.numel() > lay.sh_clamp else None,
        tile_count=tiles[:lay.tile_flags], tile_flags=tiles[lay.tile_flags:lay.tile_start],
        tile_start=tiles[lay.tile_start:lay.tile_fill], tile_fill=tiles[lay.tile_fill:lay.counters],
        counters=tiles[lay.counters:lay.pair_cursor],
        pair_cursor=tiles[lay.pair_cursor:lay.pair_cursor + 8] if tiles.numel() >= lay.pair_cursor + 8 else None,
        pair_off=pair_idx[:lay.blk_total], blk_total=pair_idx[lay.blk_total:lay.blk_base], blk_base=pair_idx[lay.blk_base:])


def _state_views(rect, tiles, pair_idx, RT: int, RG: int, RB: int) -> StateViews:
    """Slice the three shared state buffers into their fields, at the library's offsets (SpfStateLayout).  Pure indexing:
    works on device tensors and on host copies alike (the tests audit host copies with it)."""
    return _slice_state(_layout(RT, RG, RB), rect, tiles, pair_idx)


def _state_struct(state: _State, v: StateViews, verdict_host=None):
    named = {**state._asdict(), **v._asdict(), "verdict_host": verdict_host}     # (SpfState.rect: the view, not the buffer)
    return _lib.SpfState(*(_ptr(named[f]) for f, _ in _lib.SpfState._fields_))


def _raise_if_plan_failed(counters: Tensor, capacity: int, plan=None) -> None:
    """`counters`: the tiles buffer from its counters on (the pair cursors too, where it holds them).  `plan` = (bin_cap, record capacity, shards) of a direct-bins call (its counters[0] / [1] are not maintained: the
    message then names what the device actually checked), None for the classic chain."""
    host = counters.cpu()
    flag = int(host[2])
    direct = plan is not None and plan[0] > 0
    if flag & 1:
        if direct:
            cursors = host[4:12] if host.numel() >= 12 else None
            used = "" if cursors is None else f"; pairs numbered per shard: {[int(c) for c in cursors[:plan[2]]]}"
            raise _lib.SpfError("pair budget overflow in the forward pass: a shard of the (Gaussian, tile) pair numbering "
                                f"outgrew its {plan[1] // plan[2]} of {plan[1]} gradient records ({plan[2]} shard(s))"
                                f"{used}; the outputs are NaN -- plan with a larger capacity")
        raise _lib.SpfError("pair buffer overflow in the forward pass: max_pairs was too small "
                            f"({capacity} < {int(host[0])}); the outputs are NaN")
    if flag:
        longer = f"a tile needs more than its bin of {plan[0]} entries" if direct else \
            f"a tile list longer than planned ({int(host[1])})"
        raise _lib.SpfError(f"the PairBudget of the forward pass did not hold (flags {flag}: 2 = {longer}); "
                            "the outputs are NaN")


def _plan_mode(max_pairs) -> int:
    """0 = exact mode, 1 = planned and verified in backward, 2 = planned, verification left to the caller."""
    if max_pairs is None:
        return 0
    return 2 if isinstance(max_pairs, PairBudget) and max_pairs.check in ("deferred", "early") else 1


@_on_device_of_first_arg
def _backward_impl(i: _Inputs, state: _State, geom: _Geometry, plan: _Plan, grads_out, want, adapter_eps=0.0,
                   cov3D=None) -> _Grads:
    """Launch the backward chain.  `want`: dict of booleans (scales_rot, shs, colors, view, means2D[, cov]).  Band-split
    harmonics (i.shs_high): the band-4 plane's gradient is None unless band 4 was evaluated (a degree-3 evaluation
    neither reads the plane nor writes its gradient); raw rows (i.raw [S*G, 7+3K]; scales / rotations / shs None):
    dL/draw [S*G, 7+3K]; `cov3D` [S,G,6] (scales / rotations None): dL/dcov3D [S,G,6] when want["cov"]."""
    lib = _lib.load()
    means3D, scales, rotations, opacities, shs, colors = i.means3D, i.scales, i.rotations, i.opacities, i.shs, i.colors
    shs_high, raw = i.shs_high, i.raw
    S, V, G, H, W = geom.S, geom.V, geom.G, geom.H, geom.W
    dense, bin_cap, capacity = plan
    R, dev = S * V, means3D.device
    nblk = lib.spf_raster_view_partial_blocks(G)
    lay = _layout(R * lib.spf_raster_num_tiles(H, W), R * G, R * nblk)
    # (a device->host read is illegal while a HIP graph is being captured: graph users check the flag themselves
    # with `pair_buffer_overflowed` after a replay)
    if geom.plan_mode == 1 and not torch.cuda.is_current_stream_capturing():
        _raise_if_plan_failed(state.tiles[lay.counters:], capacity,
                              (bin_cap, capacity, lib.spf_raster_pair_shards(S, G)) if bin_cap else None)
    from .shard import active_bucket
    bucket = active_bucket()
    if cov3D is not None and bucket is not None:
        # (GradBucket.NAMES has no slot for a covariance: its gradient must not land in another tensor's place)
        raise RuntimeError("a shard.GradBucket is active, but this backward renders precomputed covariances: gradient "
                           "buckets hold no covariance gradient -- run covariance calls outside the bucket")
    fast = _lib.fast() if (bucket is None and shs_high is None and raw is None and cov3D is None) else None   # (a gradient bucket supplies the output buffers, the split layout a second plane, raw rows another input: ctypes path)
    if fast is not None:
        wv = want["view"]
        with _spf_errors():
            return _Grads(*fast.raster_backward(
                means3D, scales, rotations, opacities, shs, colors, i.viewmatrix, i.projmatrix, i.tanfov, i.bg, i.view_scale,
                i.viewmatrix64, *state, H, W, geom.sh_degree, geom.scale_modifier, geom.sh_layout, geom.sh_band4,
                int(dense), int(bin_cap), int(capacity), grads_out[0], grads_out[1], grads_out[2],
                bool(want["scales_rot"]), bool(want["shs"]), bool(want["colors"]),
                2 if wv == "partials" else (1 if wv else 0), bool(want["means2D"])))
    dims = _dims(geom, bin_cap, capacity, raw, adapter_eps)
    f32 = dict(dtype=torch.float32, device=dev)
    g_image, g_depth, g_alpha = (None if g is None else g.contiguous().float() for g in grads_out)
    gpair = torch.empty((capacity, 10), **f32)     # packed gradient records: 9 (+1 with a depth gradient) floats
    def out(name, like):          # a view of the caller's flat gradient bucket (shard.GradBucket) or a fresh buffer
        v = bucket.take(name, like) if bucket is not None else None
        return torch.empty_like(like) if v is None else v
    d_means = out("means", means3D)
    d_opac = out("opacities", opacities)
    d_scales = out("scales", scales) if (want["scales_rot"] and raw is None) else None
    d_rot = out("rotations", rotations) if (want["scales_rot"] and raw is None) else None
    d_raw = torch.empty((raw.shape[0], raw.shape[1]), **f32) if raw is not None else None
    d_cov = torch.empty_like(cov3D) if (cov3D is not None and want.get("cov")) else None
    d_shs = out("harmonics", shs) if (shs is not None and want["shs"]) else None
    d_shs_high = None
    if d_shs is not None and geom.sh_layout == 2 and geom.sh_band4 and geom.sh_degree == 4:
        d_shs_high = out("harmonics_band4", shs_high)
    d_col = torch.empty_like(colors) if (colors is not None and want["colors"]) else None
    # want["view"] == "partials": leave the viewmatrix gradient as per-block partial sums (the decoder chains them to
    # the poses in one kernel, spf_camera_backward_partials); returned in place of d_view
    d_view = torch.empty_like(i.viewmatrix) if want["view"] is True else None
    vpartial = torch.empty((R, nblk, 12), **f32) if want["view"] else None
    d_m2d = torch.zeros((R, G, 3), **f32) if want["means2D"] else None
    inp = _inputs_struct(i)
    st = _state_struct(state, _slice_state(lay, state.rect, state.tiles, state.pair_idx))
    gr = _lib.SpfGrads(_ptr(g_image), _ptr(g_depth), _ptr(g_alpha), _ptr(gpair), _ptr(vpartial),
                       _ptr(d_means), _ptr(d_scales), _ptr(d_rot), _ptr(d_opac), _ptr(d_shs), _ptr(d_col),
                       _ptr(d_view), _ptr(d_m2d), _ptr(d_shs_high), _ptr(d_raw))
    if cov3D is not None:
        _lib.check(lib.spf_raster_backward_cov3d(C.byref(dims), C.byref(inp), _ptr(cov3D), C.byref(st), C.byref(gr),
                                                 _ptr(d_cov), capacity, dense, _stream_ptr(dev)),
                   "spf_raster_backward_cov3d")
    else:
        _lib.check(lib.spf_raster_backward(C.byref(dims), C.byref(inp), C.byref(st), C.byref(gr), capacity, dense,
                                           _stream_ptr(dev)), "spf_raster_backward")
    return _Grads(d_means, d_scales, d_rot, d_opac, d_shs, d_col, vpartial if want["view"] == "partials" else d_view, d_m2d,
                  d_shs_high, d_raw, d_cov)


class _RasterizeBatch(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, opacities, shs, colors, viewmatrix, projmatrix, tanfov, bg,
                view_scale, H, W, sh_degree, scale_modifier, enable_cov_grad, enable_sh_grad, means2D, max_pairs,
                sh_band4, record, grad_mode, cov3D=None):
        # `grad_mode`: torch.is_grad_enabled() AT THE CALL SITE (inside Function.forward it is always False, and
        # ctx.needs_input_grad stays True under no_grad): a backward will come only if both say so
        ctx.set_materialize_grads(False)
        fw = _forward_impl(means3D, scales, rotations, opacities, shs, colors, viewmatrix, projmatrix, tanfov, bg,
                           view_scale, H, W, sh_degree, scale_modifier, max_pairs, sh_band4=sh_band4, record=record,
                           nothing_needs_grad=not (grad_mode and any(ctx.needs_input_grad)), cov3D=cov3D)
        inputs = _Inputs(means3D, scales, rotations, opacities, shs, colors, viewmatrix, projmatrix, tanfov, bg, view_scale)
        ctx.geom, ctx.plan = _geometry(inputs, sh_degree, H, W, scale_modifier, 0, sh_band4, max_pairs), fw.plan
        ctx.flags = (bool(enable_cov_grad), bool(enable_sh_grad))
        ctx.means2D_shape = None if means2D is None else tuple(means2D.shape)
        ctx.save_for_backward(*inputs, *fw.state, cov3D)
        ctx.mark_non_differentiable(fw.outs[3])
        return fw.outs

    ARGS = tuple(inspect.signature(forward.__func__).parameters)[1:]       # forward's inputs, in order

    @staticmethod
    def backward(ctx, g_image, g_depth, g_alpha, _g_radii):
        t, inputs, state = _saved(ctx)
        need = dict(zip(_RasterizeBatch.ARGS, ctx.needs_input_grad))
        enable_cov_grad, enable_sh_grad = ctx.flags
        want = dict(scales_rot=enable_cov_grad and (need["scales"] or need["rotations"]),
                    shs=enable_sh_grad and need["shs"], colors=need["colors"], view=need["viewmatrix"],
                    means2D=ctx.means2D_shape is not None and need["means2D"],
                    cov=enable_cov_grad and need.get("cov3D", False))
        g = _backward_impl(inputs, state, ctx.geom, ctx.plan, (g_image, g_depth, g_alpha), want, cov3D=t["cov3D"])
        return _input_grads(_RasterizeBatch.ARGS, g, viewmatrix=g.view,
                            means2D=None if g.means2D is None else g.means2D.view(ctx.means2D_shape))


class _DecoderRender(torch.autograd.Function):
    """Camera set-up + rasterizer as ONE autograd node (poses in, images out): the whole of
    render_cuda (cuda_splatting.py:45-144) for b scenes x v views without any intermediate torch op."""

    @staticmethod
    def forward(ctx, extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs, colors, bg,
                H, W, sh_degree, scale_invariant, enable_cov_grad, enable_sh_grad, max_pairs, sh_layout, sh_band4,
                record, grad_mode, shs_high=None, raw=None, sh_mask=None, adapter_eps=0.0, cov3D=None):
        ctx.set_materialize_grads(False)
        S, V = extrinsics.shape[:2]
        view, proj, tanfov, vscale, view64 = _alloc_camera(means3D.device, S, V, scale_invariant)
        # raw rows (sh_layout 3): the caller's tensor, whatever its shape; its [S*G, 7+3K] rows are taken HERE, outside
        # autograd's view (an as_strided under autograd costs a zero fill and a scatter of the whole tensor in backward)
        rows = None
        if raw is not None:
            rows = raw_rows(raw.detach(), raw.shape[-1])
            ctx.raw_shape = tuple(raw.shape)
        cam = _lib.SpfCamera(_ptr(extrinsics), _ptr(intrinsics), _ptr(near), _ptr(far), _ptr(view), _ptr(proj),
                             _ptr(tanfov), _ptr(vscale), S * V, 1 if scale_invariant else 0, _ptr(view64))
        fw = _forward_impl(means3D, scales, rotations, opacities, shs, colors, view, proj, tanfov, bg, vscale, H, W,
                           sh_degree, 1.0, max_pairs, sh_layout, camera=cam, sh_band4=sh_band4, record=record,
                           nothing_needs_grad=not (grad_mode and any(ctx.needs_input_grad)), view64=view64,
                           shs_high=shs_high, raw=rows, sh_mask=sh_mask, adapter_eps=adapter_eps, cov3D=cov3D)
        ctx.adapter_eps = float(adapter_eps)
        inputs = _Inputs(means3D, scales, rotations, opacities, shs, colors, view, proj, tanfov, bg, vscale, view64,
                         shs_high, rows, sh_mask)
        ctx.geom, ctx.plan = _geometry(inputs, sh_degree, H, W, 1.0, sh_layout, sh_band4, max_pairs), fw.plan
        ctx.flags = (bool(enable_cov_grad), bool(enable_sh_grad), bool(scale_invariant))
        ctx.save_for_backward(*inputs, *fw.state, cov3D, near)
        ctx.mark_non_differentiable(fw.outs[3])
        return fw.outs

    ARGS = tuple(inspect.signature(forward.__func__).parameters)[1:]

    @staticmethod
    def backward(ctx, g_image, g_depth, g_alpha, _g_radii):
        t, inputs, state = _saved(ctx)
        need = dict(zip(_DecoderRender.ARGS, ctx.needs_input_grad))
        enable_cov_grad, enable_sh_grad, scale_invariant = ctx.flags
        fused = inputs.raw is not None                     # (raw rows: the pair and the harmonics are inside dL/draw)
        want = dict(scales_rot=fused or (enable_cov_grad and (need["scales"] or need["rotations"])),
                    shs=fused or (enable_sh_grad and need["shs"]), colors=need["colors"],
                    view="partials" if need["extrinsics"] else False, means2D=False,
                    cov=enable_cov_grad and need.get("cov3D", False))
        g = _backward_impl(inputs, state, ctx.geom, ctx.plan, (g_image, g_depth, g_alpha), want,
                           adapter_eps=ctx.adapter_eps, cov3D=t["cov3D"])
        d_ext = None
        if need["extrinsics"]:
            view = inputs.viewmatrix
            d_ext = torch.empty_like(view)
            cam = _lib.SpfCamera(None, None, _ptr(t["near"]), None, _ptr(view), None, None, None,
                                 view.shape[0] * view.shape[1], 1 if scale_invariant else 0)
            with torch.cuda.device(view.device):
                _lib.check(_lib.load().spf_camera_backward_partials(C.byref(cam), _ptr(g.view), g.view.shape[1],
                                                                    _ptr(d_ext), _stream_ptr(view.device)),
                           "spf_camera_backward_partials")
        return _input_grads(_DecoderRender.ARGS, g, extrinsics=d_ext, raw=None if g.raw is None else g.raw.view(ctx.raw_shape))


class StaticStep:
    """One planned decoder step (camera -> projection + bins -> sort -> composite; composite backward -> projection
    backward -> pose chain) PREPARED once: the state the chain keeps between its kernels (records, bins, tile bookkeeping,
    per-pixel state, gradient records, pose partials) lives at fixed addresses, the argument structs are built once, and
    what a call costs the host is a handful of C-ABI calls -- no allocation besides its OUTPUTS, no validation, no struct
    marshalling.  Outputs (image | depth, alpha; every gradient) are fresh tensors per call -- gradients a gradient bucket
    holds go into its views --: nothing a caller holds is ever rewritten.  `DecoderSplattingCUDA` uses it for training
    calls whose SHAPES repeat (decoder.py): the inputs are bound per call (`bind`: a dozen pointer fields; the step holds
    the tensors until the next `bind`, so they outlive the backward) -- an encoder that hands over fresh tensors every
    step runs on the same prepared state as a loop over static leaves.  Direct bins only.

    `launch_project()` touches state only; `render()` and `backward()` write fresh outputs.  Between a
    `launch_project()` and the `backward()` that belongs to it the state must stay as it is: one step at a time.
    (Round 6 measured the same chain replayed from three HIP graphs with copies in and out -- no faster on the host, the
    copies cost the GPU 8 - 290 us per step -- and its state-only part from one small graph: a two-kernel hipGraphLaunch
    costs MORE host time than the two launches.  The step's host cost is allocation, validation and marshalling; that is
    what is prepared here.)"""

    def __init__(self, extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs, shs_high, bg,
                 H, W, sh_degree, scale_invariant, plan: PairBudget, sh_band4, want: dict, forward_only: bool = False):
        lib = _lib.load()
        self.lib = lib
        S, G, _ = means3D.shape
        V = extrinsics.shape[1]
        R, dev = S * V, means3D.device
        self.dev = dev
        T = lib.spf_raster_num_tiles(H, W)
        bin_cap = _direct_bin_cap(plan, R * T, T)
        if not bin_cap:
            raise RuntimeError("StaticStep needs a plan that runs with direct bins")
        layout = 2 if shs_high is not None else 1
        rec_cap = _record_capacity(int(plan.capacity), S, G)
        geom = _Geometry(S, V, G, _sh_coefficients(shs, layout), sh_degree, H, W, 1.0, layout, bool(sh_band4), _plan_mode(plan))
        self.dims = _dims(geom, bin_cap, rec_cap)
        self.shape = (S, V, G, H, W)
        f32 = dict(dtype=torch.float32, device=dev)
        self.f32 = f32
        self.view, self.proj, self.tanfov, self.vscale, self.view64 = _alloc_camera(dev, S, V, scale_invariant)
        nblk = lib.spf_raster_view_partial_blocks(G)
        state, lay = _alloc_state(dev, R, G, T, nblk, H * W)     # (state only: the outputs are the calls' own)
        if state.tiles.data_ptr() % 16:
            raise RuntimeError("StaticStep: the tile bookkeeping buffer is not 16-byte aligned")
        self.state = state = state._replace(pairs=torch.empty((R * T * bin_cap,), dtype=torch.int64, device=dev))
        self.tiles, self.radii = state.tiles, state.radii
        views = _slice_state(lay, state.rect, state.tiles, state.pair_idx)
        self.counters, self.plan_words = views.counters, state.tiles[lay.counters:]
        self.capacity, self.bin_cap = rec_cap, bin_cap
        self.plan_info = (int(bin_cap), int(rec_cap), lib.spf_raster_pair_shards(S, G))
        self.bgx = _background(bg, S, V)
        self.scale_invariant = bool(scale_invariant)
        self.cam = _lib.SpfCamera(None, None, None, None, _ptr(self.view), _ptr(self.proj), _ptr(self.tanfov),
                                  _ptr(self.vscale), R, 1 if scale_invariant else 0, _ptr(self.view64))
        self.inp = _inputs_struct(_Inputs(None, None, None, None, None, None, self.view, self.proj, self.tanfov, self.bgx,
                                          self.vscale, self.view64))
        self.cam_b = _lib.SpfCamera(None, None, None, None, _ptr(self.view), None, None, None, R,
                                    1 if scale_invariant else 0)
        self.verdict = torch.zeros(1, dtype=torch.int32, pin_memory=True)      # SpfState.verdict_host
        self.verdict_event = torch.cuda.Event()
        self.st = _state_struct(state, views, verdict_host=self.verdict)
        self.out = _lib.SpfOutputs(None, None, None)
        self.max_tile = int(plan.max_tile_list)
        # ---- backward ----
        self.gpair = None if forward_only else torch.empty((rec_cap, 10), **f32)     # (evaluation calls' steps: no backward)
        like = {"means": means3D, "opacities": opacities}
        if want["scales_rot"]:
            like["scales"], like["rotations"] = scales, rotations
        if want["shs"]:
            like["harmonics"] = shs
            if layout == 2 and sh_band4 and sh_degree == 4:
                like["harmonics_band4"] = shs_high
        if want["view"]:
            like["extrinsics"] = self.view
        one = torch.empty((1,), **f32)   # each gradient's shape, dtype and device for GradBucket.take: one float expanded
        self.grad_like = {name: one.expand(t.shape) for name, t in like.items()}
        self.vpartial = torch.empty((R, nblk, 12), **f32) if want["view"] else None
        self.gr = _lib.SpfGrads(None, None, None, _ptr(self.gpair), _ptr(self.vpartial))
        self.nblk = nblk
        self.nbytes = sum(t.numel() * t.element_size() for t in state + (self.gpair,) if t is not None)
        # the same step driven from the compiled binding when it has been built (csrc/torch_binding.cpp::PreparedStep takes
        # the structs over by value): bind / forward / backward are then one C++ call each
        mod = _lib.fast()
        self.fast = None
        if mod is not None and hasattr(mod, "PreparedStep"):
            with _spf_errors():
                self.fast = mod.PreparedStep(
                    C.addressof(self.dims), C.addressof(self.inp), C.addressof(self.st), C.addressof(self.cam),
                    C.addressof(self.cam_b), C.addressof(self.gr), self.tiles, self.capacity, self.max_tile, nblk,
                    self.verdict, self.view, self.vpartial, bool(want["scales_rot"]), bool(want["shs"]),
                    "harmonics_band4" in self.grad_like, bool(want["view"]))
        self.bind(extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs, shs_high)

    def bind(self, extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs, shs_high) -> None:
        """This call's inputs (dense float32 device tensors of the shapes the step was prepared for -- the caller's
        key guarantees that): a dozen pointer fields.  The step holds their STORAGE until the next `bind` (detached
        aliases: an encoder's autograd graph is not kept alive through them)."""
        if self.fast is not None:
            self.fast.bind(extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs, shs_high)
            return
        (extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs) = (
            t if t.grad_fn is None else t.detach()
            for t in (extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs))
        if shs_high is not None and shs_high.grad_fn is not None:
            shs_high = shs_high.detach()
        cam, inp = self.cam, self.inp
        cam.extrinsics, cam.intrinsics, cam.near, cam.far = (extrinsics.data_ptr(), intrinsics.data_ptr(), near.data_ptr(),
                                                             far.data_ptr())
        inp.means3D, inp.scales, inp.rotations, inp.opacities = (means3D.data_ptr(), scales.data_ptr(),
                                                                 rotations.data_ptr(), opacities.data_ptr())
        inp.shs, inp.shs_high = shs.data_ptr(), _ptr(shs_high)
        self.cam_b.near = cam.near
        self.near_b = near[:, :, None, None] if self.scale_invariant else None   # depth x near (decoder_splatting_cuda.py:72-76)
        self._held = (extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs, shs_high)

    def forward(self, early: bool):
        """The forward chain on the current binding: (colour, depth, alpha, failed).  `early`: wait for the projection
        kernel's verdict (an event behind it, waited for once sort and compositing have been queued -- the GPU works
        through the wait, nothing is copied on the stream); `failed` then says that the plan did not hold (outputs NaN)."""
        if self.fast is not None:
            with _spf_errors():
                return self.fast.forward(bool(early))
        with torch.cuda.device(self.dev):
            if early:
                self.verdict.zero_()                 # (host memory: the projection kernel stores here if it raises a flag)
            self.launch_project()
            if early:
                self.verdict_event.record()
            color, depth, alpha = self.render()
            failed = False
            if early:
                self.verdict_event.synchronize()
                failed = self.verdict.item() != 0
        return color, depth, alpha, failed

    def launch_project(self) -> None:
        """Camera set-up + clearing of the tile bookkeeping, projection + binning (state only: capturable)."""
        lib, stream = self.lib, _stream_ptr(self.dev)
        _lib.check(lib.spf_decoder_prepare(C.byref(self.cam), _ptr(self.tiles), 4 * self.tiles.numel(), stream),
                   "spf_decoder_prepare")
        _lib.check(lib.spf_raster_forward_project_prepared(C.byref(self.dims), C.byref(self.inp), C.byref(self.st),
                                                           4 * self.tiles.numel(), stream),
                   "spf_raster_forward_project_prepared")

    def render(self):
        """Sort + compositing into FRESH outputs: (colour [S,V,3,H,W], depth [S,V,H,W] -- x near when scale-invariant --,
        alpha [S,V,1,H,W])."""
        S, V, G, H, W = self.shape
        color = torch.empty((S, V, 3, H, W), **self.f32)
        depth = torch.empty((S, V, H, W), **self.f32)
        alpha = torch.empty((S, V, 1, H, W), **self.f32)
        self.out.image, self.out.depth, self.out.alpha = color.data_ptr(), depth.data_ptr(), alpha.data_ptr()
        _lib.check(self.lib.spf_raster_forward_render(C.byref(self.dims), C.byref(self.inp), C.byref(self.st),
                                                      C.byref(self.out), self.capacity, self.max_tile, 0xFFFFFFFF,
                                                      _stream_ptr(self.dev)), "spf_raster_forward_render")
        if self.scale_invariant:
            depth.mul_(self.near_b)
        return color, depth, alpha

    GRADS = ("means", "opacities", "scales", "rotations", "harmonics", "harmonics_band4", "extrinsics")

    def backward(self, g_image, g_depth, g_alpha, bucket=None) -> list:
        """The whole backward chain on the current binding: the gradients of `GRADS` (`extrinsics`: the poses'), None
        where none was asked for.  `g_depth` is the gradient of the [S,V,H,W] depth output (x near is undone here).
        Gradients are fresh tensors; with a gradient bucket (shard.GradBucket) those it holds are written into its views."""
        taken = {} if bucket is None else {name: bucket.take(name, like) for name, like in self.grad_like.items()}
        if self.fast is not None:
            with _spf_errors():
                return self.fast.backward(g_image, g_depth, g_alpha, [taken.get(n) for n in self.GRADS] if taken else None)
        c = lambda g: None if g is None else g.contiguous().float()
        g_image, g_alpha = c(g_image), c(g_alpha)
        if g_depth is not None:                          # (the node's depth output is [S,V,H,W], already x near)
            g_depth = c(g_depth * self.near_b if self.scale_invariant else g_depth)
        g = {name: torch.empty(like.shape, **self.f32) if taken.get(name) is None else taken[name]
             for name, like in self.grad_like.items()}
        gr = self.gr
        gr.dL_dimage, gr.dL_ddepth, gr.dL_dalpha = _ptr(g_image), _ptr(g_depth), _ptr(g_alpha)
        gr.dL_dmeans3D, gr.dL_dopacities = g["means"].data_ptr(), g["opacities"].data_ptr()
        gr.dL_dscales, gr.dL_drotations = _ptr(g.get("scales")), _ptr(g.get("rotations"))
        gr.dL_dshs, gr.dL_dshs_high = _ptr(g.get("harmonics")), _ptr(g.get("harmonics_band4"))
        lib, stream = self.lib, _stream_ptr(self.dev)
        with torch.cuda.device(self.dev):
            _lib.check(lib.spf_raster_backward(C.byref(self.dims), C.byref(self.inp), C.byref(self.st), C.byref(gr),
                                               self.capacity, 0xFFFFFFFF, stream), "spf_raster_backward")
            if "extrinsics" in g:
                _lib.check(lib.spf_camera_backward_partials(C.byref(self.cam_b), _ptr(self.vpartial), self.nblk,
                                                            _ptr(g["extrinsics"]), stream), "spf_camera_backward_partials")
        return [g.get(name) for name in self.GRADS]

    def raise_if_failed(self) -> None:
        _raise_if_plan_failed(self.plan_words, self.capacity, self.plan_info)


def camera_forward(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor, scale_invariant: bool = True):
    """HIP camera set-up kernel on its own (no autograd): [S,V,...] poses -> (viewmatrix [S,V,4,4],
    projmatrix [S,V,4,4], tanfov [S,V,2], view_scale [S,V]) exactly as ``render_batch`` feeds the rasterizer."""
    lib = _lib.load()
    S, V = extrinsics.shape[:2]
    extrinsics, intrinsics, near, far = _check_camera(extrinsics.detach(), intrinsics, near, far, S, V)
    view, proj, tanfov, vscale, view64 = _alloc_camera(extrinsics.device, S, V)
    cam = _lib.SpfCamera(_ptr(extrinsics), _ptr(intrinsics), _ptr(near), _ptr(far), _ptr(view), _ptr(proj),
                         _ptr(tanfov), _ptr(vscale), S * V, 1 if scale_invariant else 0, _ptr(view64))
    with torch.cuda.device(extrinsics.device):
        _lib.check(lib.spf_camera_forward(C.byref(cam), _stream_ptr(extrinsics.device)), "spf_camera_forward")
    return view, proj, tanfov, vscale


def render_batch(extrinsics: Tensor, intrinsics: Tensor, near: Tensor, far: Tensor,
                 means3D: Tensor, scales: Tensor, rotations: Tensor, opacities: Tensor,
                 shs: Optional[Tensor], colors_precomp: Optional[Tensor], bg: Tensor,
                 image_height: int, image_width: int, sh_degree: int, scale_invariant: bool = True,
                 enable_cov_grad: bool = True, enable_sh_grad: bool = True, max_pairs=None,
                 sh_layout: str = "gk3", sh_band4: Optional[bool] = None, record: Optional[CallRecord] = None,
                 shs_high: Optional[Tensor] = None, raw: Optional[Tensor] = None, sh_mask: Optional[Tensor] = None,
                 adapter_eps: float = 1e-8, cov3D: Optional[Tensor] = None):
    """Poses in, images out: camera set-up (render_cuda's preamble) and rasterization in one autograd node.

    extrinsics [S,V,4,4] camera-to-world, intrinsics [S,V,3,3] normalised, near/far [S,V]; Gaussians as in
    ``rasterize_batch``; ``sh_layout="g3k"`` takes ``shs`` as [S,G,3,K] -- the encoder's native layout
    (``Gaussians.harmonics``), so the transposed copy at cuda_splatting.py:79 never happens; with ``shs_high`` [S,G,3,9]
    (band 4) ``shs`` is [S,G,3,16] (bands 0 - 3): the BAND-SPLIT layout of d_sh = 25 the fused adapter writes
    (``UnifiedGaussianAdapter(..., split_harmonics=True)``) -- a degree-3 evaluation then never touches band 4's bytes,
    forward or backward.  ``sh_band4``: evaluate
    band 4 when ``sh_degree`` is 4 (None = ``sh_band4_default()``).  ``record``: a ``CallRecord`` that receives this
    call's statistics / plan counters.  ``cov3D`` ([S,G,6] or [S,G,3,3], with ``scales`` and ``rotations`` None):
    precomputed covariances, as in ``rasterize_batch`` (with ``scale_invariant`` render (s,v) sees ``Sigma * k^2``).
    ``raw`` (RAW ROWS, SpfDims.sh_layout 3: [S,G,7+3K] -- any leading shape with S*G rows and unit stride along the channels,
    e.g. a view of the encoder's 83-channel head output) is what UnifiedGaussianAdapter.forward takes (gaussian_adapter.py:
    122-150), ``sh_mask`` [K] and ``adapter_eps`` the adapter's: the projection kernels apply its activations as they read a
    row and chain the backward into dL/draw -- adapter -> decoder to float32 rounding, without the adapter's two passes.
    Returns image [S,V,3,H,W], depth [S,V,1,H,W] (rasterizer units), alpha [S,V,1,H,W], radii [S,V,G]."""
    if cov3D is not None:
        if scales is not None or rotations is not None:
            raise RuntimeError(COV_EXCLUSIVE)
        if raw is not None or shs_high is not None:
            raise RuntimeError("precomputed covariances (cov3D) are not supported with raw rows or band-split harmonics "
                               "(shs_high)")
    fused = raw is not None
    if not fused and (shs is None) == (colors_precomp is None):
        raise RuntimeError("provide exactly one of shs / colors_precomp")
    S, G, _ = means3D.shape
    V = extrinsics.shape[1]
    extrinsics, intrinsics, near, far = _check_camera(extrinsics, intrinsics, near, far, S, V)
    if fused:          # (the rows carry the pair and the harmonics: whatever else was passed for them is not looked at)
        scales = rotations = shs = colors_precomp = shs_high = None
        sh_layout, enable_cov_grad, enable_sh_grad = "g3k", True, True
    means3D, scales, rotations, opacities, cov3D = _check_gaussians(means3D, scales, rotations, opacities, cov3D, S, G,
                                                                    pair=not fused)
    shs, shs_high, sh_mask, _, layout, sh_band4 = _check_sh(S, G, sh_degree, sh_band4, shs, sh_layout, shs_high, raw, sh_mask)
    if colors_precomp is not None:
        colors_precomp = _f32c(colors_precomp, "colors_precomp", (S, G, 3))
    bg = _background(bg, S, V)
    return _DecoderRender.apply(extrinsics, intrinsics, near, far, means3D, scales, rotations, opacities, shs,
                                colors_precomp, bg, int(image_height), int(image_width), int(sh_degree),
                                bool(scale_invariant), enable_cov_grad, enable_sh_grad, max_pairs, layout, sh_band4, record,
                                torch.is_grad_enabled(), shs_high, raw, sh_mask if fused else None,
                                float(adapter_eps) if fused else 0.0, cov3D)


def rasterize_batch(means3D: Tensor, scales: Tensor, rotations: Tensor, opacities: Tensor,
                    shs: Optional[Tensor], colors_precomp: Optional[Tensor],
                    viewmatrix: Tensor, projmatrix: Tensor, tanfov: Tensor, bg: Tensor,
                    image_height: int, image_width: int, sh_degree: int, scale_modifier: float = 1.0,
                    enable_cov_grad: bool = True, enable_sh_grad: bool = True,
                    means2D: Optional[Tensor] = None, max_pairs=None,
                    view_scale: Optional[Tensor] = None, sh_band4: Optional[bool] = None,
                    record: Optional[CallRecord] = None, cov3D: Optional[Tensor] = None):
    """Render S scenes x V views.

    means3D [S,G,3], scales [S,G,3], rotations [S,G,4] (r,x,y,z; used as given), opacities [S,G] or
    [S,G,1], shs [S,G,K,3] XOR colors_precomp [S,G,3], viewmatrix / projmatrix [S,V,4,4] (row-vector
    convention, i.e. the transposes the reference builds at cuda_splatting.py:89-90), tanfov [S,V,2],
    bg [S,V,3] or [3].  Returns image [S,V,3,H,W], depth [S,V,1,H,W], alpha [S,V,1,H,W],
    radii [S,V,G] int32.

    ``view_scale`` ([S,V], optional): per-render world scale; render (s,v) sees ``means3D[s] * k`` and
    ``scales[s] * k`` with ``k = view_scale[s,v]`` (the reference's scale-invariant normalisation,
    cuda_splatting.py:66-74, fused into the projection kernel instead of materialised per view).

    ``means2D`` ([S,V,G,3], optional) is only a gradient holder: if it requires grad it receives the
    NDC-scaled screen-space gradient of every Gaussian centre (cuda_splatting.py:98-102,130).

    ``max_pairs``: None = exact mode (one tiny device->host read per call to size the pair buffer);
    an integer or a ``PairBudget`` (see ``plan_pair_budget``) = planned mode, no read-back in the forward pass: the
    plan is verified on the device and a failed plan raises in backward (``check="backward"``) or is reported by
    ``last_plan_flags()`` (``check="deferred"``, fully sync-free and graph-capturable).

    ``cov3D`` ([S,G,6] packed (xx, xy, xz, yy, yz, zz), or [S,G,3,3] of which the upper triangle is read; ``scales``
    and ``rotations`` None): precomputed 3-D covariances instead of the scale/rotation pair (the public rasterizer's
    ``cov3D_precomp``).  Used as given -- ``scale_modifier`` does not apply -- and scaled to ``Sigma * k^2`` by
    ``view_scale``.  Its gradient has the packed input's shape (an off-diagonal entry receives G_ij + G_ji); none with
    ``enable_cov_grad=False``.  Positive semidefinite input is the contract (rank-deficient is fine); an indefinite
    matrix renders as L L^T of its Cholesky factor with non-positive pivots clamped to zero (include/spfsplat_hip.h).
    """
    if (shs is None) == (colors_precomp is None):
        raise RuntimeError("provide exactly one of shs / colors_precomp")
    if cov3D is not None and (scales is not None or rotations is not None):
        raise RuntimeError(COV_EXCLUSIVE)
    if means3D.dim() != 3 or means3D.shape[-1] != 3:
        raise RuntimeError(f"means3D must be [S,G,3], got {tuple(means3D.shape)}")
    S, G, _ = means3D.shape
    if viewmatrix.dim() != 4:
        raise RuntimeError(f"viewmatrix must be [S,V,4,4], got {tuple(viewmatrix.shape)}")
    V = viewmatrix.shape[1]
    means3D, scales, rotations, opacities, cov3D = _check_gaussians(means3D, scales, rotations, opacities, cov3D, S, G)
    if shs is not None and (shs.dim() != 4 or shs.shape[-1] != 3):
        raise RuntimeError(f"shs must be [S,G,K,3], got {tuple(shs.shape)}")
    shs, _, _, _, _, sh_band4 = _check_sh(S, G, sh_degree, sh_band4, shs)
    if shs is None:
        colors_precomp = _f32c(colors_precomp, "colors_precomp", (S, G, 3))
    viewmatrix, projmatrix = _f32c(viewmatrix, "viewmatrix", (S, V, 4, 4)), _f32c(projmatrix, "projmatrix", (S, V, 4, 4))
    tanfov = _f32c(tanfov, "tanfov", (S, V, 2))
    bg = _background(bg, S, V)
    if view_scale is not None:
        view_scale = _f32c(view_scale.detach(), "view_scale", (S, V))
    if means2D is not None and means2D.numel() != S * V * G * 3:
        raise RuntimeError(f"means2D must hold S*V*G*3 elements, got {tuple(means2D.shape)}")
    return _RasterizeBatch.apply(means3D, scales, rotations, opacities, shs, colors_precomp, viewmatrix,
                                 projmatrix, tanfov, bg, view_scale, int(image_height), int(image_width),
                                 int(sh_degree), float(scale_modifier), enable_cov_grad, enable_sh_grad, means2D,
                                 max_pairs, bool(sh_band4), record, torch.is_grad_enabled(), cov3D)


# ---------------------------------------------------------------------------------------------
# Drop-in surface of the reference's rasterizer package (diff_gauss_pose)
# ---------------------------------------------------------------------------------------------
class GaussianRasterizationSettings(NamedTuple):
    """Field-for-field the settings tuple built at cuda_splatting.py:105-120."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: Tensor
    scale_modifier: float
    projmatrix: Tensor
    sh_degree: int
    prefiltered: bool = False
    debug: bool = False
    enable_cov_grad: bool = True
    enable_sh_grad: bool = True
    sh_band4: Optional[bool] = None    # (not a field of the reference's tuple) None = sh_band4_default()
    render_norm: bool = False          # (not a field of the reference's tuple) also produce `rendered_norm`


def gaussian_normals(means3D: Tensor, scales: Tensor, rotations: Tensor, viewmatrix: Tensor) -> Tensor:
    """View-space unit normal of every Gaussian [G,3]: its axis of least extent (the column of R(q) that belongs to the
    smallest scale; q read as (r,x,y,z) like the rasterizer does), taken to view space with the
    row-vector `viewmatrix` and turned to face the camera.  ASSUMED definition of the fork's `rendered_norm` (its source
    is not available offline -- oracle/PINNING.md, last row); the reference never reads that output."""
    r, x, y, z = rotations.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=-1).reshape(-1, 3, 3)
    axis = scales.argmin(dim=-1)
    n_world = R[torch.arange(R.shape[0], device=R.device), :, axis]
    n_view = n_world @ viewmatrix[:3, :3]
    t_view = means3D @ viewmatrix[:3, :3] + viewmatrix[3, :3]
    n_view = n_view / n_view.norm(dim=-1, keepdim=True).clamp_min(1e-20)
    away = (n_view * t_view).sum(dim=-1, keepdim=True) > 0
    return torch.where(away, -n_view, n_view)


class GaussianRasterizer(torch.nn.Module):
    """``GaussianRasterizer(settings)(means3D=..., means2D=..., shs=..., colors_precomp=..., opacities=...,
    scales=..., rotations=..., viewmatrix=...) -> (image[3,H,W], depth[1,H,W], norm, alpha[1,H,W], radii[G], extra)``
    (call site: cuda_splatting.py:124-138).  The reference never reads ``norm`` and ``extra``
    (cuda_splatting.py:141-144), so they cost nothing unless asked for: ``norm`` is None unless
    ``settings.render_norm`` (or ``SPF_RENDER_NORM=1``), ``extra`` is None unless ``extra_attrs`` [G,C] is passed.  Both are
    alpha-blended per-Gaussian attributes, ``sum_i a_i alpha_i T_i`` -- rendered by further passes of the same
    rasterizer, three channels at a time, through its ``colors_precomp`` input (differentiable like any colour)."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D=None, opacities=None, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3Ds_precomp=None, viewmatrix=None, extra_attrs=None):
        s = self.raster_settings
        if (shs is None) == (colors_precomp is None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if cov3Ds_precomp is not None:
            # precomputed covariances [G,6] or [G,3,3] (the reference's call is commented out, cuda_splatting.py:136)
            if scales is not None or rotations is not None:
                raise Exception(COV_EXCLUSIVE)
            if s.render_norm or os.environ.get("SPF_RENDER_NORM", "0") == "1":
                raise Exception("render_norm is defined from scales and rotations: it is not available with "
                                "cov3Ds_precomp")
        elif scales is None and rotations is None:
            raise Exception(COV_EXCLUSIVE)
        elif scales is None or rotations is None:
            raise Exception("Please provide scales and rotations")
        if viewmatrix is None:
            raise Exception("viewmatrix is a forward argument of this rasterizer (cuda_splatting.py:137)")
        dev = means3D.device
        if not means3D.is_cuda:            # (before the settings' tan fov is staged on the tensors' device)
            raise RuntimeError(f"means3D is on {dev}: the rasterizer only runs on a HIP device (there is no CPU fallback)")
        tanfov = _tanfov_tensor(float(s.tanfovx), float(s.tanfovy), dev)

        def render(shs_, colors_, bg, m2d=None):
            return rasterize_batch(
                means3D[None], None if scales is None else scales[None], None if rotations is None else rotations[None],
                opacities.reshape(1, -1),
                None if shs_ is None else shs_[None], None if colors_ is None else colors_[None],
                viewmatrix[None, None], s.projmatrix[None, None], tanfov, bg.reshape(1, 1, 3),
                s.image_height, s.image_width, s.sh_degree, s.scale_modifier,
                s.enable_cov_grad, s.enable_sh_grad, means2D=m2d, sh_band4=s.sh_band4,
                cov3D=None if cov3Ds_precomp is None else cov3Ds_precomp[None])

        def blend(attrs: Tensor) -> Tensor:            # [G,C] -> [C,H,W], three channels per pass, no background
            out = []
            for c0 in range(0, attrs.shape[1], 3):
                chunk = attrs[:, c0:c0 + 3]
                pad = 3 - chunk.shape[1]
                if pad:
                    chunk = torch.cat([chunk, chunk.new_zeros(chunk.shape[0], pad)], dim=1)
                out.append(render(None, chunk.contiguous(), torch.zeros(3, device=dev))[0][0, 0][:3 - pad])
            return torch.cat(out, dim=0)

        image, depth, alpha, radii = render(shs, colors_precomp, s.bg, means2D)
        norm = extra = None
        if s.render_norm or os.environ.get("SPF_RENDER_NORM", "0") == "1":
            norm = blend(gaussian_normals(means3D, scales * s.scale_modifier, rotations, viewmatrix))
        if extra_attrs is not None:
            extra = blend(extra_attrs.to(torch.float32))
        return image[0, 0], depth[0, 0], norm, alpha[0, 0], radii[0, 0], extra
