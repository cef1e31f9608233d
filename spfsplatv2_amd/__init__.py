"""spfsplatv2_amd -- MI355X (gfx950) native Gaussian-splat rasterizer + RoPE-2D behind SPFSplatV2's
decoder / curope call surfaces.  All compute lives in libspfsplat_hip.so (C ABI: include/spfsplat_hip.h).
"""
from . import _lib, hostbind
from .decoder import (DECODERS, camera_tensors, Decoder, DecoderOutput, DecoderSplattingCUDA, DecoderSplattingCUDACfg,
                      DecoderSplattingHIP, Gaussians, get_decoder, get_fov, get_projection_matrix, render_cuda,
                      orthographic_camera, render_cuda_orthographic, render_views)
from .rasterizer import (CallRecord, GaussianRasterizationSettings, GaussianRasterizer, PairBudget, camera_forward,
                         last_forward_stats, last_plan_flags, plan_flags, plan_pair_budget, rasterize_batch,
                         render_batch, sh_band4_default)
from .loss import (Loss, LossLpips, LossLpipsCfg, LossLpipsCfgWrapper, LossMse, LossMseCfg, LossMseCfgWrapper, LossReproj,
                   LossReprojCfg, LossReprojCfgWrapper, Regr3D, mse_loss, regr3d_loss, reproj_loss, unit_grad)
from .lpips import LPIPS, LpipsWeights, lpips
from .metrics import compute_lpips, compute_psnr, compute_ssim
from .pose import (compute_pose_error, compute_pose_error_for_batch, convert_pose_to_4x4, depth_projector,
                   estimate_focal_knowing_depth, estimate_intrinsics, pose_auc, pose_errors, process_depth, process_pose)
from .ssim import SSIM, ssim
from .attention import (Attention, CrossAttention, decoder_view_sets, rope_attention, rope_attention_packed,
                        rope_attention_views)
from .vggt_attention import VGGTAttention
from .block import Block, DecoderBlock, LayerScale, Mlp, VGGTBlock, add_layer_norm, bias_gelu, layer_norm
from .heads import (DPTOutputAdapter, FeatureFusionBlock_custom, Interpolate, PixelwiseTaskWithDPT, PixelwiseTaskWithGSDPT,
                    ResidualConvUnit_custom, add_relu, create_dpt_head, create_gs_dpt_head, head_factory, postprocess,
                    upsample2x)
from .optim import GuardedAdamW, StepReport
from .tail import GaussianTail, density_to_opacity, gaussians_from_heads, map_pdf_to_opacity
from .pnp import PnPResult, get_pnp_pose, get_pnp_pose_batch, pnp_poses
from .posehead import (CameraHead, CameraTrunkAttention, CameraTrunkBlock, PoseHead, PoseHeadCfg, activate_pose,
                       camera_head_factory, create_pose_head, modulate, predict_poses)
from .front import PatchEmbedDust3R, VGGTPatchEmbed, assemble_tokens, embed_patches, prepare_tokens
from .rope import (PositionGetter, RoPE2D, RotaryPositionEmbedding2D, append_token_position, cuRoPE2D, cuRoPE2D_func,
                   rope_2d, rope_2d_head_major, rope_2d_pair)

__all__ = [
    "DECODERS", "Decoder", "DecoderOutput", "DecoderSplattingCUDA", "DecoderSplattingCUDACfg",
    "DecoderSplattingHIP", "Gaussians", "get_decoder", "get_fov", "get_projection_matrix", "render_cuda",
    "render_cuda_orthographic", "render_views", "GaussianRasterizationSettings", "GaussianRasterizer",
    "last_forward_stats", "PairBudget", "plan_pair_budget", "last_plan_flags", "plan_flags", "CallRecord", "sh_band4_default", "orthographic_camera", "rasterize_batch", "render_batch", "camera_forward", "camera_tensors", "Loss", "LossMse", "LossMseCfg", "LossMseCfgWrapper", "mse_loss", "unit_grad", "LossReproj", "LossReprojCfg", "LossReprojCfgWrapper", "reproj_loss", "Regr3D", "regr3d_loss", "ssim", "SSIM", "compute_ssim", "compute_psnr", "LossLpips", "LossLpipsCfg", "LossLpipsCfgWrapper", "lpips", "LPIPS", "LpipsWeights", "compute_lpips", "convert_pose_to_4x4", "process_pose", "depth_projector", "process_depth", "compute_pose_error", "compute_pose_error_for_batch", "pose_errors", "pose_auc", "estimate_focal_knowing_depth", "estimate_intrinsics", "PositionGetter", "append_token_position", "RoPE2D", "RotaryPositionEmbedding2D", "cuRoPE2D", "cuRoPE2D_func", "rope_2d", "rope_2d_head_major", "rope_2d_pair", "Attention", "CrossAttention", "rope_attention", "rope_attention_packed", "rope_attention_views", "decoder_view_sets", "VGGTAttention", "Block", "DecoderBlock", "VGGTBlock", "Mlp", "LayerScale", "layer_norm", "add_layer_norm", "bias_gelu", "upsample2x", "add_relu", "postprocess", "ResidualConvUnit_custom", "FeatureFusionBlock_custom", "Interpolate", "DPTOutputAdapter", "PixelwiseTaskWithDPT", "PixelwiseTaskWithGSDPT", "create_dpt_head", "create_gs_dpt_head", "head_factory", "GuardedAdamW", "StepReport", "hostbind", "GaussianTail", "gaussians_from_heads", "density_to_opacity", "map_pdf_to_opacity",
    "get_pnp_pose", "get_pnp_pose_batch", "pnp_poses", "PnPResult",
    "PoseHeadCfg", "PoseHead", "create_pose_head", "camera_head_factory", "predict_poses", "activate_pose", "modulate",
    "CameraTrunkAttention", "CameraTrunkBlock", "CameraHead",
    "embed_patches", "assemble_tokens", "PatchEmbedDust3R", "VGGTPatchEmbed", "prepare_tokens",
]
