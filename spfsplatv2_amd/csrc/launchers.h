// Every host function that a kernel file defines and api.hip calls, declared ONCE, in the order of build.py's SOURCES.
// api.hip and each defining .hip include this: a drifted signature or a second default argument fails to compile, not
// to load.  Defaults live here only.  Declarations only: no device code changes (profiles/launchers_header_isa.txt).
#pragma once
#include "spf_common.h"
namespace spf {
hipError_t launch_project_fwd(const SpfDims& d_in, const SpfInputs& in_, const SpfState& st, int tiles_x, int tiles_y,
                              hipStream_t stream, const float* cov3D = nullptr);
hipError_t launch_project_bwd(const SpfDims& d_in, const SpfInputs& in_, const SpfState& st, const SpfGrads& g_, int nblk,
                              uint64_t capacity, hipStream_t stream, const float* cov3D = nullptr,
                              float* dL_dcov3D = nullptr);
hipError_t launch_tile_scan(const SpfState& st, int R, int T, int nblk, uint32_t dense_thr, bool zeroed, hipStream_t stream);
hipError_t launch_bin_pairs(const SpfDims& d, const SpfState& st, uint64_t capacity, int T, int tiles_x,
                            uint32_t max_tile_hint, hipStream_t stream);
SortSwitches read_sort_switches();
int plan_tile_sort(uint32_t max_tile_hint, int tiles_call, bool with_order, const SortSwitches& sw, SortLaunch* out);
hipError_t launch_tile_sort(const SpfState& st, const TileLists& tl, int RT, int RT_call, uint64_t capacity,
                            uint32_t max_tile_hint, const uint2* order_c, int T, hipStream_t stream);
uint32_t dense_threshold();
hipError_t launch_render_fwd(const SpfDims& d, const SpfInputs& in, const SpfState& st, const SpfOutputs& out,
                             uint64_t capacity, int T, int tiles_x, bool ordered, hipStream_t stream);
hipError_t launch_render_bwd(const SpfDims& d, const SpfInputs& in, const SpfState& st, const SpfGrads& g, int T,
                             int tiles_x, uint64_t capacity, bool ordered, hipStream_t stream);
hipError_t launch_adapter_fwd(const float* raw, int64_t stride, int64_t N, int K, const float* mask, float eps,
                              float* scales, float* rot, float* sh, float* sh_hi, hipStream_t stream);
hipError_t launch_adapter_bwd(const float* raw, int64_t stride, int64_t N, int K, const float* mask, float eps,
                              const float* g_scales, const float* g_rot, const float* g_sh, const float* g_sh_hi, int split,
                              float* g_raw, hipStream_t stream);
int mse_partial_blocks();
hipError_t launch_mse_fwd(const float* pred, const float* target, int64_t n, float scale, float* partial, float* loss,
                          float scale2, float* unit_grad, hipStream_t stream);
hipError_t launch_mse_scale(float* grad, int64_t n, const float* grad_loss, hipStream_t stream);
hipError_t launch_mse_bwd(const float* pred, const float* target, int64_t n, float scale2, const float* grad_loss,
                          float* grad_pred, hipStream_t stream);
int64_t reproj_slots(int B, int V, int H, int W, int* nchunk);
hipError_t launch_reproj_fwd(const SpfReproj& a, void* partial, float* loss, float* scale, hipStream_t stream);
hipError_t launch_reproj_bwd(const SpfReproj& a, const float* scale, const float* dL_dloss, float* dpts, float* gpartial,
                             float* dposes, float* dintr, hipStream_t stream);
int64_t regr3d_scratch_words(int B, int H, int W);
hipError_t launch_regr3d_fwd(const SpfRegr3d& a, void* scratch, float* stats, float* loss, hipStream_t stream);
hipError_t launch_regr3d_bwd(const SpfRegr3d& a, const void* scratch, const float* stats, const float* dL_dloss,
                             float* d_pr1, float* d_pr2, hipStream_t stream);
hipError_t launch_pose_compose_fwd(const float* enc, int64_t stride_b, int64_t stride_v, int b, int v, int cv, int encoding,
                                   int baseline, int relative, float* poses, hipStream_t stream);
hipError_t launch_pose_compose_bwd(const float* enc, int64_t stride_b, int64_t stride_v, int b, int v, int cv, int encoding,
                                   int baseline, int relative, const float* dposes, float* denc, hipStream_t stream);
int64_t depth_slots(int N, int n, int* nchunk);
hipError_t launch_depth_fwd(const float* pts, int64_t stride_img, const float* poses, int N, int n, float* depth,
                            hipStream_t stream);
hipError_t launch_depth_bwd(const float* pts, int64_t stride_img, const float* poses, int N, int n, const float* gdepth,
                            float* dpts, float* gpartial, float* dposes, hipStream_t stream);
hipError_t launch_pose_error(const float* pred, const float* gt, int N, float* errors, float* means, hipStream_t stream);
hipError_t launch_focal(const float* pts, int64_t stride_scene, int64_t stride_row, int B, int H, int W, const float* pp,
                        int64_t pp_stride, float focal_base, float lo, float hi, float cx, float cy, float div0, float div1,
                        float* focal, float* intrinsics, hipStream_t stream);
int64_t ssim_slots(int N, int C, int H, int W, int ws);
hipError_t launch_ssim_fwd(const SpfSsim& a, float* partial, float* plane_mean, float* out, hipStream_t stream);
hipError_t launch_ssim_bwd(const SpfSsim& a, const float* plane_mean, const float* dL_dout, float* dX, float* dY,
                           hipStream_t stream);
hipError_t launch_psnr(const float* gt, const float* pred, int N, int64_t n, float* psnr, hipStream_t stream);
int64_t lpips_workspace_bytes(int n_grad, int n_total, int H, int W);
hipError_t launch_lpips_fwd(const SpfLpips& a, float* ws, float* out, float* mean, hipStream_t stream);
hipError_t launch_lpips_bwd(const SpfLpips& a, float* ws, const float* up, int is_mean, float* d0, float* d1,
                            hipStream_t stream);
hipError_t launch_lpips_conv(const float* in, const float* mask, const float* wpack, const float* bias, float* out,
                             int n_img, int H, int W, int Cin, int Cout, int relu, hipStream_t stream);
hipError_t launch_lpips_conv1(const SpfLpips& a, int n_img, float* out, hipStream_t stream);
hipError_t launch_lpips_conv1_bwd(const SpfLpips& a, const float* g, const float* act, int n_img, float* d0, int n0,
                                  float* d1, hipStream_t stream);
hipError_t launch_lpips_pool(const float* in, float* out, int n_img, int H, int W, int C, hipStream_t stream);
hipError_t launch_lpips_pool_bwd(const float* gp, const float* act, float* inout, int n_img, int H, int W, int C,
                                 hipStream_t stream);
hipError_t launch_lpips_head_single(const float* fa, const float* fb, const float* lin, int N, int HW, int C, float* partial,
                                    float* out, hipStream_t stream);
hipError_t launch_lpips_head_bwd(const float* fa, const float* fb, const float* lin, int N, int HW, int C, const float* up,
                                 int is_mean, float mean_scale, float* dA, float* dB, hipStream_t stream);
hipError_t launch_camera_fwd(const SpfCamera& c, hipStream_t stream);
hipError_t launch_camera_bwd(const SpfCamera& c, const float* dL_dview, float* dL_dext, hipStream_t stream);
hipError_t launch_camera_fwd_zero(const SpfCamera& c, void* zero, uint64_t nbytes, hipStream_t stream);
hipError_t launch_camera_bwd_reduce(const SpfCamera& c, const float* vpartial, int nblk, float* dL_dext, hipStream_t stream);
hipError_t launch_attn_forward(const SpfAttn& p, const SpfAttnExt* e, void* out, float* lse, hipStream_t stream);
hipError_t launch_attn_backward(const SpfAttn& p, const SpfAttnGrads& g, const SpfAttnExt* e, const void* out,
                                const float* lse, const void* dout, hipStream_t stream);
int64_t attn_ext_scratch_floats(int B, int H, int Nq, int Nk);
hipError_t launch_attn_views_forward(const SpfAttn& p, const SpfAttnViews& w, void* out, float* lse, hipStream_t stream);
hipError_t launch_attn_views_backward(const SpfAttn& p, const SpfAttnViews& w, const SpfAttnGrads& g, const void* out,
                                      const float* lse, const void* dout, hipStream_t stream);
hipError_t launch_attn16_forward(const SpfAttn& p, void* out, float* lse, hipStream_t stream);
hipError_t launch_attn16_backward(const SpfAttn& p, const SpfAttnGrads& g, const void* out, const float* lse,
                                  const void* dout, hipStream_t stream);
hipError_t launch_rope2d(void* tokens, void* tokens2, const int64_t* pos, int B, int N, int H, int D, int64_t sb, int64_t sn,
                         int64_t sh, int pos_div, int dtype, float base, float fwd, hipStream_t stream);
int64_t optim_chunks_of(int64_t numel);
int64_t optim_scratch_bytes(int T, int64_t chunks);
hipError_t launch_optim_step(const SpfOptim& o, const SpfOptimHyper& hp, hipStream_t stream);
int64_t block_partial_blocks(int64_t rows, int C, int gelu);
hipError_t launch_block_norm_fwd(const SpfBlockNorm& a, float* s, float* y, float* stats, hipStream_t st);
hipError_t launch_block_norm_bwd(const SpfBlockNorm& a, const float* dy, const float* ds, const float* stats, float* dx,
                                 float* dr, float* partial, float* dparams, hipStream_t st);
hipError_t launch_block_gelu_fwd(const float* u, const float* bias, int64_t rows, int C, float* h, hipStream_t st);
hipError_t launch_block_gelu_bwd(const float* u, const float* bias, const float* dh, int64_t rows, int C, float* du,
                                 float* partial, float* dbias, hipStream_t st);
int dpt_max_grid();
hipError_t launch_dpt_up2_fwd(const float* x, const float* skip, int relu_skip, int64_t planes, int h, int w, float* out,
                              hipStream_t st);
hipError_t launch_dpt_up2_bwd(const float* dy, const float* skip, int64_t planes, int h, int w, float* dx, float* dskip,
                              hipStream_t st);
hipError_t launch_dpt_add_relu_fwd(const float* a, const float* b, const float* c, int64_t n, float* s, float* y,
                                   hipStream_t st);
hipError_t launch_dpt_add_relu_bwd(const float* mask, const float* dy, const float* ds, int64_t n, float* g, hipStream_t st);
hipError_t launch_dpt_points(int fwd, const float* in, const float* dpts, const float* dconf, int64_t B, int64_t HW, int C,
                             int has_conf, float dmin, float dmax, float cmin, float cmax, float* pts, float* conf,
                             float* din, hipStream_t st);
int tail_max_grid();
hipError_t launch_tail_fwd(const SpfTail& a, float* means, float* opac, float* scales, float* rot, float* sh, float* sh_hi,
                           hipStream_t stream);
hipError_t launch_tail_bwd(const SpfTail& a, const SpfTailGrads& out, const float* g_means, const float* g_opac,
                           const float* g_scales, const float* g_rot, const float* g_sh, const float* g_sh_hi, int split,
                           hipStream_t stream);
hipError_t launch_opacity_fwd(const float* x, int64_t stride, int64_t n, float e, float* y, hipStream_t stream);
hipError_t launch_opacity_bwd(const float* x, int64_t stride, int64_t n, float e, const float* dy, float* dx,
                              hipStream_t stream);
hipError_t launch_posehead_pool_fwd(const SpfPosePool& a, float* feat, hipStream_t st);
hipError_t launch_posehead_pool_bwd(const SpfPosePool& a, const float* d_feat, float* d0, float* d1, hipStream_t st);
hipError_t launch_posehead_encode_fwd(const SpfPoseEncode& a, const float* rot, const float* t, float* out, hipStream_t st);
hipError_t launch_posehead_encode_bwd(const SpfPoseEncode& a, const float* t, const float* d_out, float* d_rot, float* d_t,
                                      hipStream_t st);
hipError_t launch_posehead_embed_fwd(const float* p, int bcast, const float* W, const float* b, int64_t rows, int C,
                                     float* out, hipStream_t st);
hipError_t launch_posehead_embed_bwd(const float* p, int bcast, const float* W, const float* b, const float* dout,
                                     int64_t rows, int C, float* dW, float* db, float* dp, hipStream_t st);
hipError_t launch_posehead_modulate_fwd(const float* x, const float* mod, int64_t rows, int C, float eps, float* out,
                                        hipStream_t st);
hipError_t launch_posehead_modulate_bwd(const float* x, const float* mod, const float* dout, int64_t rows, int C, float eps,
                                        float* dx, float* dmod, hipStream_t st);
hipError_t launch_posehead_attn_fwd(const float* qkv, int B, int S, int H, int D, float* out, hipStream_t st);
hipError_t launch_posehead_attn_bwd(const float* qkv, const float* dout, int B, int S, int H, int D, float* dqkv,
                                    hipStream_t st);
hipError_t launch_posehead_activate_fwd(const float* prev, const float* delta, int64_t rows, int trans_act, int quat_act,
                                        int fl_act, float* pred, float* out, hipStream_t st);
hipError_t launch_posehead_activate_bwd(const float* pred, const float* d_pred, const float* d_out, int64_t rows,
                                        int trans_act, int quat_act, int fl_act, float* d_delta, hipStream_t st);
int64_t front_geometry(int what, int64_t M);
int64_t front_workspace_floats(const SpfFront& a, bool with_dweight);
hipError_t launch_front_embed_fwd(const SpfFront& a, const float* weight, const float* bias, const float* pos, float* out,
                                  hipStream_t st);
hipError_t launch_front_assemble(const SpfFrontTokens& t, const float* body, int64_t inner, int64_t stride,
                                 int64_t outer_stride, int64_t S, int N, int C, float* out, hipStream_t st);
hipError_t launch_front_tokens_bwd(const SpfFrontTokens& t, const float* dy, int64_t dy_ss, int64_t dy_sr, int64_t S, int N,
                                   int C, float* d_pos_first, hipStream_t st);
hipError_t launch_front_embed_bwd(const SpfFront& a, const float* dy, int64_t dy_sb, int64_t dy_sr, float* ws, float* dweight,
                                  float* dbias, float* dpos, hipStream_t st);
int64_t pnp_workspace_bytes(int views, int h, int w, int iters);
hipError_t launch_pnp_solve(const SpfPnp& a, void* workspace, float* poses, int32_t* info, int32_t* ranks, hipStream_t stream);
}  // namespace spf
