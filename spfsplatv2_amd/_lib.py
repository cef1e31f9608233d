"""ctypes binding of libspfsplat_hip.so (C ABI: include/spfsplat_hip.h).

The HIP library is the only compute path of this package: if it is missing or does not export the
ABI declared in the header, importing/using the package fails loudly -- there is no CPU or
PyTorch fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import torch

# SPF_LIB_DIR: development only -- a profiling/experimental build kept next to the regular one (see build.py)
LIB_PATH = Path(__file__).resolve().parent / os.environ.get("SPF_LIB_DIR", "_C") / "libspfsplat_hip.so"
ABI_VERSION = 7

STAGE_NAMES = ("project_fwd", "tile_scan", "bin_pairs", "tile_sort", "render_fwd", "render_bwd",
               "project_bwd", "rope2d")
STAGE_COUNT = len(STAGE_NAMES)


class SpfDims(C.Structure):
    _fields_ = [("S", C.c_int32), ("V", C.c_int32), ("G", C.c_int32), ("K", C.c_int32),
                ("sh_degree", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("scale_modifier", C.c_float), ("sh_layout", C.c_int32), ("sh_band4", C.c_int32),
                ("bin_cap", C.c_int32), ("pair_capacity", C.c_int64), ("raw_stride", C.c_int64), ("adapter_eps", C.c_float)]


def _struct_of(name, fields, ctype=C.c_void_p):
    return type(name, (C.Structure,), {"_fields_": [(f, ctype) for f in fields]})


SpfInputs = _struct_of("SpfInputs", ["means3D", "scales", "rotations", "opacities", "shs", "colors",
                                      "viewmatrix", "projmatrix", "tanfov", "bg", "view_scale", "viewmatrix64",
                                      "shs_high", "raw", "sh_mask"])
SpfState = _struct_of("SpfState", ["rec", "radii", "rect", "zkey", "tile_count", "tile_start", "tile_fill",
                                    "tile_flags", "counters", "pairs", "pair_off", "blk_total", "blk_base", "final_T",
                                    "n_contrib", "pair_cursor", "sh_clamp", "verdict_host"])
SpfOutputs = _struct_of("SpfOutputs", ["image", "depth", "alpha"])
SpfGrads = _struct_of("SpfGrads", ["dL_dimage", "dL_ddepth", "dL_dalpha", "gpair", "vpartial",
                                    "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dopacities",
                                    "dL_dshs", "dL_dcolors", "dL_dviewmatrix", "dL_dmeans2D", "dL_dshs_high",
                                    "dL_draw"])
SpfStateLayout = _struct_of("SpfStateLayout", ["rect_words", "tiles_words", "pair_idx_words", "zkey", "sh_clamp", "tile_flags",
                                             "tile_start", "tile_fill", "counters", "pair_cursor", "blk_total", "blk_base"], C.c_int64)


class SpfCamera(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("extrinsics", "intrinsics", "near", "far", "viewmatrix", "projmatrix",
                                          "tanfov", "view_scale")] + [("R", C.c_int32), ("scale_invariant", C.c_int32),
                                                                    ("viewmatrix64", C.c_void_p)]


class SpfReproj(C.Structure):
    _fields_ = [("pts3d", C.c_void_p), ("stride_b", C.c_int64), ("stride_v", C.c_int64), ("poses", C.c_void_p),
                ("intrinsics", C.c_void_p), ("B", C.c_int32), ("V", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("mode", C.c_int32), ("weight", C.c_float), ("lw", C.c_float), ("hard_clamp", C.c_float),
                ("soft_clamp", C.c_float)]


class SpfRegr3d(C.Structure):
    _fields_ = [("gt_pts1", C.c_void_p), ("gt_pts2", C.c_void_p), ("pr_pts1", C.c_void_p), ("pr_pts2", C.c_void_p),
                ("conf1", C.c_void_p), ("conf2", C.c_void_p), ("stride_gt1", C.c_int64), ("stride_gt2", C.c_int64),
                ("stride_pr1", C.c_int64), ("stride_pr2", C.c_int64), ("B", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("has_dist_clip", C.c_int32), ("dist_clip", C.c_float), ("disable_view1", C.c_int32),
                ("normalize", C.c_int32), ("gt_scale", C.c_int32)]


SSIM_MAX_WIN = 33


class SpfSsim(C.Structure):
    _fields_ = [("X", C.c_void_p), ("Y", C.c_void_p), ("N", C.c_int32), ("C", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("ws", C.c_int32), ("C1", C.c_float), ("C2", C.c_float), ("cov_norm", C.c_float),
                ("size_average", C.c_int32), ("nonnegative", C.c_int32), ("win", C.c_float * SSIM_MAX_WIN)]


class SpfLpips(C.Structure):
    _fields_ = [("in0", C.c_void_p), ("in1", C.c_void_p), ("stride0", C.c_int64), ("stride1", C.c_int64),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("normalize", C.c_int32), ("weight", C.c_float),
                ("reserved", C.c_int32), ("wfwd", C.c_void_p), ("wbwd", C.c_void_p), ("bias", C.c_void_p),
                ("lin", C.c_void_p), ("shift_scale", C.c_void_p)]


class SpfAttn(C.Structure):
    _fields_ = [("q", C.c_void_p), ("k", C.c_void_p), ("v", C.c_void_p), ("qpos", C.c_void_p), ("kpos", C.c_void_p),
                ("q_stride", C.c_int64 * 3), ("k_stride", C.c_int64 * 3), ("v_stride", C.c_int64 * 3),
                ("B", C.c_int32), ("H", C.c_int32), ("Nq", C.c_int32), ("Nk", C.c_int32), ("D", C.c_int32),
                ("dtype", C.c_int32), ("base", C.c_float), ("F0", C.c_float), ("scale", C.c_float)]


class SpfAttnGrads(C.Structure):
    _fields_ = [("dq", C.c_void_p), ("dk", C.c_void_p), ("dv", C.c_void_p), ("dq_stride", C.c_int64 * 3),
                ("dk_stride", C.c_int64 * 3), ("dv_stride", C.c_int64 * 3), ("delta", C.c_void_p)]


class SpfAttnExt(C.Structure):
    _fields_ = [("mask", C.c_void_p), ("mask_dtype", C.c_int32), ("mask_stride", C.c_int64 * 4),
                ("q_weight", C.c_void_p), ("q_bias", C.c_void_p), ("k_weight", C.c_void_p), ("k_bias", C.c_void_p),
                ("eps", C.c_float), ("dq_weight", C.c_void_p), ("dq_bias", C.c_void_p), ("dk_weight", C.c_void_p),
                ("dk_bias", C.c_void_p), ("partials", C.c_void_p)]


class SpfAttnViews(C.Structure):
    _fields_ = [("Vq", C.c_int32), ("Vk", C.c_int32), ("allow", C.c_uint32 * 32), ("q_view_stride", C.c_int64),
                ("k_view_stride", C.c_int64), ("v_view_stride", C.c_int64), ("qpos_stride", C.c_int64 * 2),
                ("kpos_stride", C.c_int64 * 2), ("dq_view_stride", C.c_int64), ("dk_view_stride", C.c_int64),
                ("dv_view_stride", C.c_int64)]


OPTIM_CHUNK = 4096
OPTIM_MAX_GROUPS = 8


class SpfOptimTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("numel", C.c_int64),
                ("group", C.c_int32), ("reserved", C.c_int32)]


class SpfOptimGroup(C.Structure):
    _fields_ = [(f, C.c_double) for f in ("lr", "beta1", "beta2", "eps", "weight_decay")]


class SpfOptimHyper(C.Structure):
    _fields_ = [("num_groups", C.c_int32), ("guard", C.c_int32), ("clip", C.c_int32), ("reserved", C.c_int32),
                ("max_grad_value", C.c_double), ("max_norm", C.c_double), ("group", SpfOptimGroup * OPTIM_MAX_GROUPS)]


class SpfOptim(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("table", "chunk_start", "grads", "guard_order", "step", "scratch",
                                          "report")] + [("T", C.c_int32), ("reserved", C.c_int32), ("chunks", C.c_int64)]


BLOCK_MAX_C = 4096


class SpfBlockNorm(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in ("x", "r", "gamma", "weight", "bias")] + \
               [(f, C.c_int64) for f in ("x_inner", "x_stride", "x_outer_stride", "r_inner", "r_stride", "r_outer_stride",
                                         "rows")] + [("C", C.c_int32), ("eps", C.c_float)]


DPT_MAX_SIDE = 16384


class SpfDptPoints(C.Structure):
    _fields_ = [("in_", C.c_void_p), ("B", C.c_int64), ("HW", C.c_int64), ("C", C.c_int32), ("has_conf", C.c_int32),
                ("depth_min", C.c_float), ("depth_max", C.c_float), ("conf_min", C.c_float), ("conf_max", C.c_float)]


TAIL_MAX_VIEWS = 32


class SpfTail(C.Structure):
    _fields_ = [("raw", C.c_void_p * TAIL_MAX_VIEWS), ("pts", C.c_void_p * TAIL_MAX_VIEWS), ("sh_mask", C.c_void_p),
                ("hw", C.c_int64), ("b", C.c_int32), ("v", C.c_int32), ("K", C.c_int32), ("exponent", C.c_float),
                ("eps", C.c_float), ("reserved", C.c_int32)]


class SpfTailGrads(C.Structure):
    _fields_ = [("d_raw", C.c_void_p * TAIL_MAX_VIEWS), ("d_pts", C.c_void_p * TAIL_MAX_VIEWS)]


POSEHEAD_MAX_S = 32
POSEHEAD_MAX_ROWS = 65535
POSE_ACTS = {"linear": 0, "inv_log": 1, "exp": 2, "relu": 3}


class SpfPosePool(C.Structure):
    _fields_ = [("src", C.c_void_p * 2), ("inner", C.c_int64 * 2), ("stride", C.c_int64 * 2),
                ("outer_stride", C.c_int64 * 2), ("tok_stride", C.c_int64 * 2), ("C", C.c_int32 * 2), ("rows", C.c_int64),
                ("L", C.c_int32), ("reserved", C.c_int32)]


class SpfPoseEncode(C.Structure):
    _fields_ = [("rows", C.c_int64), ("out_inner", C.c_int64), ("out_stride", C.c_int64), ("out_outer_stride", C.c_int64),
                ("homogeneous", C.c_int32), ("beta", C.c_float), ("max_inv_scale", C.c_float), ("min_inv_scale", C.c_float)]


FRONT_MAX_TOKENS = 16
FRONT_TILE_ROWS, FRONT_TILE_COLS, FRONT_CHUNK_ROWS, FRONT_CHUNKS = range(4)


class SpfFront(C.Structure):
    _fields_ = [("image", C.c_void_p), ("affine", C.c_void_p), ("stride_b", C.c_int64), ("stride_c", C.c_int64),
                ("stride_y", C.c_int64), ("B", C.c_int32), ("C_in", C.c_int32), ("gh", C.c_int32), ("gw", C.c_int32),
                ("P", C.c_int32), ("C", C.c_int32), ("before", C.c_int32), ("after", C.c_int32)]


class SpfFrontTokens(C.Structure):
    _fields_ = [("tok", C.c_void_p * FRONT_MAX_TOKENS), ("rows", C.c_int32 * FRONT_MAX_TOKENS),
                ("per_image", C.c_int32 * FRONT_MAX_TOKENS), ("n_before", C.c_int32), ("n_after", C.c_int32),
                ("before", C.c_int32), ("after", C.c_int32), ("pos_first", C.c_void_p)]


class SpfPnp(C.Structure):
    _fields_ = [("pts3d", C.c_void_p), ("opacity", C.c_void_p), ("K", C.c_void_p), ("pts_stride", C.c_int64 * 4),
                ("opa_stride", C.c_int64 * 4), ("b", C.c_int32), ("v", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("iterations", C.c_int32), ("refine_steps", C.c_int32), ("seed", C.c_uint32),
                ("opacity_threshold", C.c_float), ("reprojection_error", C.c_float), ("reserved", C.c_int32)]


# Every symbol include/spfsplat_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "spf_abi_version": (C.c_int, []),
    "spf_last_error": (C.c_char_p, []),
    "spf_raster_num_tiles": (C.c_int, [C.c_int32, C.c_int32]),
    "spf_raster_view_partial_blocks": (C.c_int, [C.c_int32]),
    "spf_raster_state_layout": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, C.POINTER(SpfStateLayout)]),
    "spf_raster_launch_slot_tile": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_raster_chunks": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_raster_sort_plan": (C.c_int, [C.c_uint32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "spf_raster_pair_shards": (C.c_int, [C.c_int32, C.c_int32]),
    "spf_raster_max_lds_tiles": (C.c_int, []),
    "spf_camera_forward": (C.c_int, [C.POINTER(SpfCamera), C.c_void_p]),
    "spf_camera_backward": (C.c_int, [C.POINTER(SpfCamera), C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_raster_forward_project": (C.c_int, [C.POINTER(SpfDims), C.POINTER(SpfInputs), C.POINTER(SpfState),
                                             C.c_void_p]),
    "spf_raster_forward_render": (C.c_int, [C.POINTER(SpfDims), C.POINTER(SpfInputs), C.POINTER(SpfState),
                                            C.POINTER(SpfOutputs), C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]),
    "spf_raster_backward": (C.c_int, [C.POINTER(SpfDims), C.POINTER(SpfInputs), C.POINTER(SpfState),
                                      C.POINTER(SpfGrads), C.c_uint64, C.c_uint32, C.c_void_p]),
    "spf_decoder_prepare": (C.c_int, [C.POINTER(SpfCamera), C.c_void_p, C.c_uint64, C.c_void_p]),
    "spf_raster_forward_project_prepared": (C.c_int, [C.POINTER(SpfDims), C.POINTER(SpfInputs), C.POINTER(SpfState),
                                                      C.c_uint64, C.c_void_p]),
    "spf_raster_forward_project_cov3d": (C.c_int, [C.POINTER(SpfDims), C.POINTER(SpfInputs), C.c_void_p,
                                                   C.POINTER(SpfState), C.c_uint64, C.c_void_p]),
    "spf_raster_backward_cov3d": (C.c_int, [C.POINTER(SpfDims), C.POINTER(SpfInputs), C.c_void_p, C.POINTER(SpfState),
                                            C.POINTER(SpfGrads), C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "spf_camera_backward_partials": (C.c_int, [C.POINTER(SpfCamera), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_mse_partial_blocks": (C.c_int, []),
    "spf_mse_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_mse_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_mse_forward_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "spf_mse_scale_grad": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "spf_reproj_partial_blocks": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_reproj_forward": (C.c_int, [C.POINTER(SpfReproj), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_reproj_backward": (C.c_int, [C.POINTER(SpfReproj), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "spf_regr3d_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "spf_regr3d_forward": (C.c_int, [C.POINTER(SpfRegr3d), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_regr3d_backward": (C.c_int, [C.POINTER(SpfRegr3d), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "spf_pose_compose_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_pose_compose_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_depth_project_partial_blocks": (C.c_int64, [C.c_int32, C.c_int32]),
    "spf_depth_project_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p]),
    "spf_depth_project_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_pose_error": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_focal_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "spf_focal_estimate": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                     C.c_int64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_ssim_partial_blocks": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_ssim_forward": (C.c_int, [C.POINTER(SpfSsim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_ssim_backward": (C.c_int, [C.POINTER(SpfSsim), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_psnr_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "spf_lpips_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_lpips_forward": (C.c_int, [C.POINTER(SpfLpips), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_lpips_backward": (C.c_int, [C.POINTER(SpfLpips), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "spf_lpips_conv3x3": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "spf_lpips_conv1_forward": (C.c_int, [C.POINTER(SpfLpips), C.c_void_p, C.c_void_p]),
    "spf_lpips_conv1_backward": (C.c_int, [C.POINTER(SpfLpips), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_lpips_pool_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p]),
    "spf_lpips_pool_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_void_p]),
    "spf_lpips_head_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_lpips_head_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_adapter_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_adapter_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_rope2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                             C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float,
                             C.c_void_p]),
    "spf_rope2d_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                  C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float,
                                  C.c_void_p]),
    "spf_attn_forward": (C.c_int, [C.POINTER(SpfAttn), C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn_backward": (C.c_int, [C.POINTER(SpfAttn), C.POINTER(SpfAttnGrads),
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn16_forward": (C.c_int, [C.POINTER(SpfAttn), C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn16_backward": (C.c_int, [C.POINTER(SpfAttn), C.POINTER(SpfAttnGrads),
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn_ext_scratch_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_attn_forward_ext": (C.c_int, [C.POINTER(SpfAttn), C.POINTER(SpfAttnExt), C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn_backward_ext": (C.c_int, [C.POINTER(SpfAttn), C.POINTER(SpfAttnGrads), C.POINTER(SpfAttnExt),
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn_views_forward": (C.c_int, [C.POINTER(SpfAttn), C.POINTER(SpfAttnViews), C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_attn_views_backward": (C.c_int, [C.POINTER(SpfAttn), C.POINTER(SpfAttnViews), C.POINTER(SpfAttnGrads),
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_optim_chunks": (C.c_int64, [C.POINTER(C.c_int64), C.c_int32]),
    "spf_optim_plan": (C.c_int64, [C.POINTER(SpfOptimTensor), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "spf_optim_scratch_bytes": (C.c_int64, [C.c_int32, C.c_int64]),
    "spf_optim_step": (C.c_int, [C.POINTER(SpfOptim), C.POINTER(SpfOptimHyper), C.c_void_p]),
    "spf_block_partial_blocks": (C.c_int64, [C.c_int64, C.c_int32, C.c_int32]),
    "spf_block_add_norm_forward": (C.c_int, [C.POINTER(SpfBlockNorm), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_block_add_norm_backward": (C.c_int, [C.POINTER(SpfBlockNorm), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_block_bias_gelu_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_block_bias_gelu_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_dpt_max_grid": (C.c_int32, []),
    "spf_dpt_upsample2x_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p]),
    "spf_dpt_upsample2x_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "spf_dpt_add_relu_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "spf_dpt_add_relu_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "spf_dpt_points_forward": (C.c_int, [C.POINTER(SpfDptPoints), C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_dpt_points_backward": (C.c_int, [C.POINTER(SpfDptPoints), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_tail_max_grid": (C.c_int32, []),
    "spf_tail_forward": (C.c_int, [C.POINTER(SpfTail), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "spf_tail_backward": (C.c_int, [C.POINTER(SpfTail), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_int32, C.POINTER(SpfTailGrads), C.c_void_p]),
    "spf_opacity_forward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "spf_opacity_backward": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_posehead_pool_forward": (C.c_int, [C.POINTER(SpfPosePool), C.c_void_p, C.c_void_p]),
    "spf_posehead_pool_backward": (C.c_int, [C.POINTER(SpfPosePool), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_posehead_encode_forward": (C.c_int, [C.POINTER(SpfPoseEncode), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_posehead_encode_backward": (C.c_int, [C.POINTER(SpfPoseEncode), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p]),
    "spf_posehead_embed_silu_forward": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                                  C.c_void_p, C.c_void_p]),
    "spf_posehead_embed_silu_backward": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_posehead_modulate_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_void_p,
                                                C.c_void_p]),
    "spf_posehead_modulate_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_float,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_posehead_attn_forward": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p]),
    "spf_posehead_attn_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p]),
    "spf_posehead_activate_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_posehead_activate_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_front_geometry": (C.c_int64, [C.c_int32, C.c_int64]),
    "spf_front_workspace_floats": (C.c_int64, [C.POINTER(SpfFront), C.c_int32]),
    "spf_front_embed_forward": (C.c_int, [C.POINTER(SpfFront), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_front_assemble": (C.c_int, [C.POINTER(SpfFrontTokens), C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                     C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_front_tokens_backward": (C.c_int, [C.POINTER(SpfFrontTokens), C.c_void_p, C.c_int64, C.c_int64, C.c_int64,
                                            C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "spf_front_embed_backward": (C.c_int, [C.POINTER(SpfFront), C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_pnp_workspace_bytes": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "spf_pnp_solve": (C.c_int, [C.POINTER(SpfPnp), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spf_stage_timing_enable": (C.c_int, [C.c_int32]),
    "spf_stage_timing_sample_every": (C.c_int, [C.c_int32]),
    "spf_stage_times_ms": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "spf_stage_kernel_name": (C.c_char_p, [C.c_int32]),
}

_lib = None


class SpfError(RuntimeError):
    pass


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises ImportError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m spfsplatv2_amd.build` "
            "(hipcc, gfx950).  spfsplatv2_amd has no fallback path.")
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ImportError(f"{LIB_PATH} does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    got = lib.spf_abi_version()
    if got != ABI_VERSION:
        raise ImportError(f"{LIB_PATH} has ABI version {got}, expected {ABI_VERSION}; rebuild it")
    _lib = lib
    return lib


_fast = False          # False: not tried yet; None: not available


def fast():
    """The compiled host binding (csrc/torch_binding.cpp -> _spf_torch.so next to the HIP library), or None when it has
    not been built or SPF_NO_FAST=1.  It drives the same C ABI of the same library -- only the interpreter time of a
    call differs (rasterizer.py keeps the ctypes path for that case)."""
    global _fast
    if _fast is False:
        _fast = None
        path = LIB_PATH.parent / "_spf_torch.so"
        if os.environ.get("SPF_NO_FAST", "0") != "1" and path.exists():
            load()                                   # the HIP library first (and its ABI check)
            import importlib.util
            try:
                spec = importlib.util.spec_from_file_location("_spf_torch", str(path))
                mod = importlib.util.module_from_spec(spec)
                spec.loader.exec_module(mod)
                if mod.abi_version() == ABI_VERSION:
                    _fast = mod
                else:                                # a stale build left next to a newer library: say so, once
                    import warnings
                    warnings.warn(f"spfsplatv2_amd: {path} was built for ABI {mod.abi_version()}, the library is ABI "
                                  f"{ABI_VERSION}; using the (slower) ctypes binding -- rebuild with "
                                  "`python -m spfsplatv2_amd.build`")
            except (ImportError, OSError) as e:      # e.g. built against another torch: fall back, but say so once
                import warnings
                warnings.warn(f"spfsplatv2_amd: {path} could not be loaded ({e}); using the ctypes binding")
    return _fast


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().spf_last_error().decode(errors="replace")
        raise SpfError(f"{what} failed (code {rc}): {msg}")


def ptr(t):
    """The data pointer of a tensor as a c_void_p; None (the null pointer) for None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr(device):
    """The current stream of `device` as a c_void_p."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


_AS_IS = frozenset((int, float, bool, type(None)))      # tested first: half of a small kernel's arguments are sizes


def cargs(args) -> list:
    """Python arguments as ctypes ones: a tensor as its pointer, None as the null pointer, a structure by reference;
    ints, bools, floats and ctypes scalars and arrays pass through for `argtypes` to convert.  Needs no GPU."""
    return [a if a.__class__ in _AS_IS else C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor)
            else C.byref(a) if isinstance(a, C.Structure) else a for a in args]


def launch(name: str, device, *args) -> None:
    """The one way Python starts a kernel: inside `device`, call the entry point `name` with `cargs(args)` and the
    current stream of `device` LAST, and raise SpfError unless it returns 0.  Every launching entry point in SYMBOLS
    takes its stream as its last argument -- keep that true.  Entry points that launch nothing (*_partial_blocks,
    *_scratch_bytes, spf_optim_plan, ..) are plain calls on `load()`.  No sync, no allocation, no host read."""
    fn = getattr(load(), name)
    with torch.cuda.device(device):
        check(fn(*cargs(args), stream_ptr(device)), name)


def stage_timing_enable(stages=True) -> None:
    """True = all stages, False = off, or an iterable of stage names (see STAGE_NAMES)."""
    if stages is True:
        mask = -1
    elif not stages:
        mask = 0
    else:
        mask = 0
        for s in stages:
            mask |= 1 << STAGE_NAMES.index(s)
    check(load().spf_stage_timing_enable(mask), "spf_stage_timing_enable")


def stage_timing_sample_every(n: int) -> None:
    """Record only every n-th launch of an enabled stage (an event pair costs ~11 us of idle GPU per launch)."""
    check(load().spf_stage_timing_sample_every(int(n)), "spf_stage_timing_sample_every")


def stage_times() -> dict[str, tuple[float, int]]:
    """{stage: (total device ms, launches)} since the last stage_timing_enable(True)."""
    ms = (C.c_float * STAGE_COUNT)()
    cnt = (C.c_int32 * STAGE_COUNT)()
    check(load().spf_stage_times_ms(ms, cnt), "spf_stage_times_ms")
    return {STAGE_NAMES[i]: (float(ms[i]), int(cnt[i])) for i in range(STAGE_COUNT)}


def stage_kernel_name(stage: str) -> str:
    return load().spf_stage_kernel_name(STAGE_NAMES.index(stage)).decode()
