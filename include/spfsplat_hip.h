/*
 * spfsplat_hip.h -- C ABI of the MI355X (gfx950) Gaussian-splat rasterizer + RoPE-2D library
 * (libspfsplat_hip.so).
 *
 * Plain pointers and sizes only: no torch / pybind types.  Every pointer is a DEVICE pointer
 * unless its comment says "host".  The library never allocates device memory, never
 * synchronises the device (except spf_stage_times_ms, which the caller asks for) and launches
 * everything on the stream it is given, so it can be driven from any host language.
 *
 * What each entry point replaces in the reference (ranrhuang/SPFSplatV2):
 *
 *   spf_raster_*            the external rasterizer behind
 *                           `GaussianRasterizer(settings)(means3D=..., viewmatrix=...)`
 *                           src/model/decoder/cuda_splatting.py:105-138 (forward) and its autograd
 *                           backward; package diff_gauss_pose, requirements.txt:88.  One call here
 *                           covers a whole batch of (scene, view) renders, i.e. the Python loop at
 *                           cuda_splatting.py:96-143 and the per-view `repeat` copies at
 *                           src/model/decoder/decoder_splatting_cuda.py:59-64.
 *   spf_camera_*            the camera preparation inside render_cuda: scale-invariant rescale
 *                           (cuda_splatting.py:66-74), get_fov (src/geometry/projection.py:269-283),
 *                           get_projection_matrix (cuda_splatting.py:15-42), extrinsics.inverse() and the
 *                           transposes (cuda_splatting.py:84-91), and its autograd backward to the poses.
 *   spf_adapter_*           UnifiedGaussianAdapter.forward (src/model/encoder/common/gaussian_adapter.py:122-150)
 *   spf_rope2d              `rope_2d(tokens, positions, base, fwd)` (and VGGT's RotaryPositionEmbedding2D,
 *                           src/model/encoder/backbone/vggt/layers/rope.py:62-188, same rotation out of place)
 *                           src/model/encoder/backbone/croco/curope/curope.cpp:49-65 and
 *                           curope/kernels.cu:84-108 (in place, forward and backward).
 *   spf_reproj_*            LossReproj.forward (src/loss/loss_reproj.py:53-101, project_to_cam in
 *                           src/misc/cam_utils.py:289-307) and its autograd backward, for all context views at once.
 *   spf_ssim_*, spf_psnr_*  ssim / SSIM (src/loss/loss_ssim.py:58-189) with its autograd backward, and compute_ssim /
 *                           compute_psnr (src/evaluation/metrics.py:11-52), for a whole batch of images on the device.
 *   spf_lpips_*             LPIPS(net="vgg") as LossLpips (src/loss/loss_lpips.py:57-85) and compute_lpips
 *                           (src/evaluation/metrics.py:22-33) call it, with its backward; weights come from the caller.
 *   spf_regr3d_*            Regr3D.forward, the distillation point loss (src/loss/loss_point.py:188-254, with
 *                           normalize_pointcloud 'avg_dis', src/geometry/ptc_geometry.py:270-328, and invalid_to_zeros,
 *                           src/model/encoder/backbone/croco/misc.py:129-138) as src/model/model_wrapper.py:171,323-331
 *                           builds and calls it, with its autograd backward to the two predicted point maps.
 *   spf_pose_compose_*      process_pose (src/model/encoder/encoder_spfsplatv2.py:340-359 with convert_pose_to_4x4,
 *                           src/misc/cam_utils.py:275-286; the VGGT variant encoder_spfsplatv2l.py:248-269) and its backward.
 *   spf_depth_project_*     depth_projector / process_depth (src/misc/cam_utils.py:310-318) and its backward.
 *   spf_pose_error          compute_pose_error (src/evaluation/metrics.py:70-99) for N pairs, with the three means.
 *   spf_focal_*             estimate_focal_knowing_depth 'weiszfeld' and estimate_intrinsics
 *                           (src/misc/intrinsics_utils.py:33-108,162-174), one focal per scene.
 *   spf_optim_*             ModelWrapper.optimizer_step (src/model/model_wrapper.py:1113-1151): the NaN / large-gradient
 *                           guard, clip_grad_norm_(parameters, 0.5) and the torch.optim.AdamW step that
 *                           configure_optimizers (:1067-1111) sets up, for the whole parameter set at once.
 *
 * Return value of every int function: 0 = success, otherwise a negative SPF_E_* code;
 * spf_last_error() returns a host string describing the most recent failure on this thread.
 */
#ifndef SPFSPLAT_HIP_H
#define SPFSPLAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPF_ABI_VERSION 7   /* unchanged by the spf_regr3d_* family: it only ADDS a struct and three entry points; no
                              existing struct, signature or meaning moved, so a caller built against 7 still fits.
                              The same holds for the pose path (spf_pose_compose_*, spf_depth_project_*, spf_pose_error,
                              spf_focal_*): eight entry points added, nothing moved; spf_raster_state_layout likewise; and for the
                              fused attention (SpfAttn, SpfAttnGrads, spf_attn_forward, spf_attn_backward) and its
                              mask / q-k-LayerNorm extras (SpfAttnExt, spf_attn_forward_ext, spf_attn_backward_ext,
                              spf_attn_ext_scratch_floats) and its multi-view family (SpfAttnViews,
                              spf_attn_views_forward, spf_attn_views_backward) and the opt-in 16-bit matrix path of
                              the plain call (spf_attn16_forward, spf_attn16_backward) and the guarded AdamW step
                              (SpfOptimTensor, SpfOptimGroup, SpfOptimHyper, SpfOptimReport, SpfOptim, spf_optim_chunks,
                              spf_optim_plan, spf_optim_scratch_bytes, spf_optim_step): four entry points added */

#define SPF_OK 0
#define SPF_E_INVALID (-1)   /* bad argument (null pointer, size, unsupported degree ...) */
#define SPF_E_LAUNCH (-2)    /* a HIP call failed; see spf_last_error() */
#define SPF_E_CAPACITY (-3)  /* pair buffer smaller than the number of (Gaussian, tile) pairs */

#define SPF_UNKNOWN 0xffffffffu
#define SPF_TILE 16          /* square tile edge in pixels (four waves per tile); spf_raster_num_tiles() counts them */
#define SPF_DENSE_AREA 26    /* mean cull-box area (px) above which a tile's BACKWARD takes the dense "rows" form inside the
                                compositing kernel (and what the dense-tile census, counters[3], counts) */
#define SPF_DENSE_AREA_FWD 120 /* the same for the FORWARD: the sparse "lists" form stays ahead of the rows form up to much
                                denser tiles than in the backward (round 5 sweep), so a tile may composite forward through
                                lists and backward through rows -- both write / read the same per-pixel state */

/* Geometry of one batched call: S scenes, V views each => R = S*V renders of H x W pixels.
 * All scenes hold G Gaussians with K SH coefficients per colour channel (stride); the SH basis is
 * evaluated up to min(sh_degree, 3), or min(sh_degree, 4) when sh_band4 is set.  K == 0 means colours are given
 * directly (colors_precomp). */
typedef struct SpfDims {
    int32_t S, V, G, K, sh_degree, H, W;
    float scale_modifier;
    int32_t sh_layout;   /* 0: shs / dL_dshs are [S,G,K,3] (what the reference hands its rasterizer,
                            cuda_splatting.py:79); 1: [S,G,3,K] (the encoder's native layout: no transposed copy);
                            2 ("band split", K = 25 only): TWO planes, shs / dL_dshs = [S,G,3,16] (bands 0 - 3) and
                            shs_high / dL_dshs_high = [S,G,3,9] (band 4) -- what spf_adapter_forward writes when it is given
                            a second plane.  The reference ships d_sh = 25 (config/model/encoder/spfsplatv2.yaml:20) and
                            a degree-3 evaluation (sh_band4 = 0) then touches plane 0 only: the band-4 third of every
                            coefficient block neither crosses HBM in the forward nor is zero-written in the backward
                            (in one [3,25] block it shares cache lines with the bands that are read);
                            3 ("raw rows"): the ADAPTER IS FUSED INTO THE PROJECTION KERNELS -- scales, rotations and shs are
                            NULL and every Gaussian is one row of SpfInputs.raw, the network's 7 + 3K raw channels
                            (UnifiedGaussianAdapter.forward, gaussian_adapter.py:122-150): the kernels form
                            scales = min(0.001 softplus(raw[0:3]), 0.3), rotations = raw[3:7] / (|.| + adapter_eps) and
                            sh[c][k] = raw[7 + c K + k] * sh_mask[k] as they read the row, and the backward chains through
                            them into dL_draw -- the adapter's own pass over 656 + 576 bytes per Gaussian and step (more
                            than the decoder's) never happens.  The same expressions in the same order as
                            spf_adapter_forward -> sh_layout 1: results agree to float32 rounding */
    int32_t sh_band4;    /* 0 (default): the reference's d_sh = 25 / sh_degree 4 (config/model/encoder/spfsplatv2.yaml:20,
                            cuda_splatting.py:77-78,114) is accepted as a stride and evaluated to degree 3 like the
                            published 3DGS kernels; 1: band 4 (coefficients 16..24) is evaluated too, forward and
                            backward (the `pose` fork's behaviour is not knowable offline: SURVEY.md 0.6) */
    int32_t bin_cap;     /* 0: tile lists are packed (tile_start = exclusive scan of the tile counts; the classic chain
                            project -> scan -> bin -> sort).  > 0 ("direct bins", planned calls only): every tile owns a
                            fixed bin of bin_cap entries at pairs[tile * bin_cap ..] and the PROJECTION kernel itself
                            writes the keys there -- no scan, no binning pass, two launches and one pass over the
                            (Gaussian, view) pairs fewer.  The caller sizes st->pairs for S*V*tiles*bin_cap entries
                            (<= 2^31) and passes the same value to every call of the forward/backward pair; a tile that
                            needs more than bin_cap entries raises plan flag 2 (see spf_raster_forward_render). */
    int64_t pair_capacity; /* direct bins only: number of gradient records g->gpair will hold (the `capacity` the
                            backward is given); the projection kernel numbers the (Gaussian, tile) pairs and raises plan
                            flag 1 if they do not fit -- per SHARD of the numbering when it is sharded: each of the
                            spf_raster_pair_shards(S, G) shards owns pair_capacity / shards records (see there) */
    int64_t raw_stride;  /* sh_layout 3 only: floats between two Gaussians' rows of SpfInputs.raw (>= 7 + 3K) */
    float adapter_eps;   /* sh_layout 3 only: the eps of rotations = q / (|q| + eps) (gaussian_adapter.py:136) */
} SpfDims;

/* Inputs (all float32, contiguous, row-major). */
typedef struct SpfInputs {
    const float* means3D;    /* [S,G,3] */
    const float* scales;     /* [S,G,3] */
    const float* rotations;  /* [S,G,4] quaternion (r,x,y,z), used as given (not normalised) */
    const float* opacities;  /* [S,G]   */
    const float* shs;        /* [S,G,K,3] ([S,G,3,K] with sh_layout 1; [S,G,3,16] with sh_layout 2) or NULL when colors is set */
    const float* colors;     /* [S,G,3]  or NULL when shs is set (colors_precomp) */
    const float* viewmatrix; /* [S,V,4,4] world->view, row-vector convention (p_view = [p,1] @ M) */
    const float* projmatrix; /* [S,V,4,4] perspective only, row-vector convention */
    const float* tanfov;     /* [S,V,2] (tanfovx, tanfovy) */
    const float* bg;         /* [S,V,3] background colour */
    const float* view_scale; /* [S,V] or NULL (= 1): per-render world scale applied to means3D and scales
                                inside the projection kernel -- the reference's scale-invariant
                                normalisation (cuda_splatting.py:66-74) without per-view copies */
    const double* viewmatrix64; /* [S,V,4,4] or NULL: the same world->view matrix in float64 with view_scale already
                                folded into its first three rows, so that [p,1] @ M64 is the (rescaled) view-space
                                position of the UNscaled mean p.  Written by spf_camera_forward / spf_decoder_prepare.
                                The view-space position p R + t is a difference of terms ~|t| for Gaussians near the
                                camera (after the 1/near rescale |t| is tens of units while z may be 0.2): the
                                projection kernels form it in float64 -- from this matrix when given, else from the
                                float32 one promoted -- and round once.  Everything else stays float32. */
    const float* shs_high;   /* sh_layout 2 only: [S,G,3,9], band 4; read only when sh_band4 is set (may be NULL otherwise) */
    const float* raw;        /* sh_layout 3 only: [S*G rows of 7+3K floats at SpfDims.raw_stride]: the adapter's input, read in
                                place (the encoder hands over gaussians[..., 1:], a view of its 83-channel head output) */
    const float* sh_mask;    /* sh_layout 3 only: [K] per-coefficient scale of the harmonics (gaussian_adapter.py:47-48) */
} SpfInputs;

/* State written by the forward pass and read by the backward pass (owned by the caller, e.g. the
 * autograd context).  T = ceil(W/16)*ceil(H/16) tiles per render, P = H*W pixels per render. */
typedef struct SpfState {
    float* rec;            /* [R*G,12]  screen-space record: xy, conic(3), opacity, rgb, depth, cull r^2, flags */
    int32_t* radii;        /* [R*G]     pixel radius, 0 = culled (also an output) */
    uint32_t* rect;        /* [R*G]     packed tile rect: xmin | ymin<<8 | xmax<<16 | ymax<<24 */
    float* zkey;           /* [R*G]     view-space depth again, compact (the binning pass reads 8 B per Gaussian
                                        instead of pulling the 48-byte record through the cache) */
    uint32_t* tile_count;  /* [R*T]     Gaussians per tile */
    uint32_t* tile_start;  /* [R*T+1]   exclusive scan of tile_count; last = D.  Direct bins: scratch -- when tile_start |
                            *            tile_fill are ONE 8-byte aligned piece (tile_fill == tile_start + R*T + 1, as in the
                            *            one-buffer layout below) and the call has >= 2,048 tiles, the library keeps the
                            *            composite kernels' launch order there: [R*T][2] = (tile | dense-backward << 31 | dense-forward << 30, list length),
                            *            longest lists first, written by spf_raster_forward_render and read again by
                            *            spf_raster_backward -- leave it alone between the two */
    uint32_t* tile_fill;   /* [R*T]     scratch cursor for the binning pass (direct bins: see tile_start) */
    uint32_t* tile_flags;  /* [R*T]     footprint load of the tile: sum over its list of min(cull-disc bounding-box
                                        area in pixels, 256); tiles whose mean exceeds SPF_DENSE_AREA(_FWD) take the dense
                                        "rows" form of the compositing kernels, the others the sparse "lists" form */
    uint32_t* counters;    /* [4]       0: D (total pairs) 1: max tile_count 2: plan verdict (0 = held) 3: number of dense tiles
                                        (direct bins: 0 and 3 are not maintained) */
    uint64_t* pairs;       /* [capacity] per-tile lists, each sorted by (depth bits << 32 | Gaussian id)
                                        (direct bins: [R*T*bin_cap], tile t's list at t * bin_cap) */
    uint32_t* pair_off;    /* [R*G,2]   (packed tile rect as in `rect`, index of the Gaussian's first (Gaussian, tile) pair):
                                        its pair with the k-th tile of its rect (row-major) has index pair_off + k.  One
                                        8-byte record so that the composite backward finds a list entry's gradient slot
                                        with ONE gather (round 3: rect and pair_off were two arrays, two gathers) */
    uint32_t* blk_total;   /* [R*nblk]  pairs per block of 256 Gaussians, nblk = spf_raster_view_partial_blocks(G) */
    uint32_t* blk_base;    /* [R*nblk]  exclusive scan of blk_total */
    float* final_T;        /* [R*P]     transmittance left after the last contributor */
    uint32_t* n_contrib;   /* [R*P]     per pixel: 1 + list position of the last contributor (0 = none) */
    uint32_t* pair_cursor; /* [8]       direct bins only (may be NULL otherwise): cursors of the pair numbering, ZERO on
                                        entry of spf_raster_forward_project* (spf_decoder_prepare clears them when they
                                        lie inside the buffer it is given) */
    uint8_t* sh_clamp;     /* [R*G]     SH colours only (may be NULL with colors_precomp): bit c = colour channel c of this
                                        (render, Gaussian) was clamped at 0 by the forward (such a
                                        channel passes no gradient).  Written by spf_raster_forward_project*, read by
                                        spf_raster_backward for sh_degree >= 1 -- the backward contracts dL/dcolour with the
                                        coefficients BEFORE the basis derivatives (three accumulators instead of twelve: the
                                        degree-4 kernel fits two waves per SIMD) and so needs the clamp decision up front
                                        instead of re-evaluating the colour */
    uint32_t* verdict_host; /* [1]      may be NULL.  A HOST-MAPPED word (hipHostMalloc / pinned memory, device-accessible) that
                                        the projection kernel of a direct-bins call stores a non-zero value to when it raises
                                        a plan flag (counters[2]); the caller zeroes it before the call.  A host that wants the
                                        verdict EARLY then needs no device->host copy on the stream (a 4-byte copy is a trip
                                        through the copy engine that the next kernel of the stream waits for): it records
                                        an event behind spf_raster_forward_project*, queues the rest of the chain, waits for the
                                        event and reads the word */
} SpfState;

typedef struct SpfOutputs {
    float* image;  /* [R,3,H,W] */
    float* depth;  /* [R,1,H,W]  sum_i z_i alpha_i T_i */
    float* alpha;  /* [R,1,H,W]  1 - final_T */
} SpfOutputs;

/* Upstream gradients (any may be NULL = zero) and the gradients to produce (any may be NULL = skip). */
typedef struct SpfGrads {
    const float* dL_dimage;   /* [R,3,H,W] */
    const float* dL_ddepth;   /* [R,1,H,W] */
    const float* dL_dalpha;   /* [R,1,H,W] */
    float* gpair;             /* [capacity,10] scratch: screen-space gradient of every (Gaussian, tile) pair, written
                                 once per pair by its tile (no global atomics, no memset), indexed by pair_off + k;
                                 records are packed: 9 floats each, 10 when dL_ddepth != NULL
                                 (dL/d pixel centre xy, dL/d 2-D covariance (a, b, c), dL/d opacity, dL/d rgb[, dL/d depth]) */
    float* vpartial;          /* [R, nblk, 12] (16-byte aligned) scratch for the deterministic viewmatrix reduction,
                                 nblk = spf_raster_view_partial_blocks(G) */
    float* dL_dmeans3D;       /* [S,G,3] */
    float* dL_dscales;        /* [S,G,3]   (NULL when enable_cov_grad is false) */
    float* dL_drotations;     /* [S,G,4]   (NULL when enable_cov_grad is false) */
    float* dL_dopacities;     /* [S,G]   */
    float* dL_dshs;           /* same layout as shs (NULL when enable_sh_grad is false) */
    float* dL_dcolors;        /* [S,G,3]   */
    float* dL_dviewmatrix;    /* [S,V,4,4] */
    float* dL_dmeans2D;       /* [R,G,3]   NDC-scaled screen-space gradient (xy, 0) */
    float* dL_dshs_high;      /* sh_layout 2 with sh_band4 only: [S,G,3,9] (otherwise never touched, may be NULL: the
                                 gradient of band 4 is zero and its consumer, spf_adapter_backward, takes NULL for that) */
    float* dL_draw;           /* sh_layout 3 only: [S*G, 7+3K] contiguous -- what spf_adapter_backward would have written;
                                 dL_dscales / dL_drotations / dL_dshs are not used then */
} SpfGrads;

/* Camera set-up for R = S*V renders (all float32, contiguous). */
typedef struct SpfCamera {
    const float* extrinsics;  /* [R,4,4] camera-to-world (OpenCV), as the decoder receives it */
    const float* intrinsics;  /* [R,3,3] normalised */
    const float* near;        /* [R] */
    const float* far;         /* [R] */
    float* viewmatrix;        /* [R,4,4] out: inverse(extrinsics')^T (row-vector convention) */
    float* projmatrix;        /* [R,4,4] out: perspective^T */
    float* tanfov;            /* [R,2]   out */
    float* view_scale;        /* [R]     out (may be NULL): 1/near when scale_invariant else 1 */
    int32_t R;
    int32_t scale_invariant;  /* cuda_splatting.py:66-74: translation, means, scales x 1/near; near -> 1 */
    double* viewmatrix64;     /* [R,4,4] out (may be NULL): see SpfInputs.viewmatrix64 */
} SpfCamera;

int spf_abi_version(void);
const char* spf_last_error(void);

/* Number of tiles per render and size of the vpartial scratch. */
int spf_raster_num_tiles(int32_t H, int32_t W);
int spf_raster_view_partial_blocks(int32_t G);
/* Where the 13 fields of SpfState that the host bindings keep in THREE buffers start, in 4-byte words:
 *   rect      rect (RG) | zkey (RG) | sh_clamp (RG bytes, rounded up to whole words)
 *   tiles     tile_count (RT) | tile_flags (RT) | tile_start (RT + 1) | tile_fill (RT) | counters (4) | pair_cursor (8) |
 *             padding to a multiple of 16 bytes
 *   pair_idx  pair_off (2 RG) | blk_total (RB) | blk_base (RB)
 * for RT = R*T tiles, RG = R*G (render, Gaussian) pairs and RB = R * spf_raster_view_partial_blocks(G) blocks; rect,
 * tile_count and pair_off sit at offset 0.  The one definition: every binding allocates and slices by it.  Host
 * arithmetic only (no launch, no device, no environment); SPF_E_INVALID unless RT, RG and RB are positive. */
typedef struct SpfStateLayout {
    int64_t rect_words, tiles_words, pair_idx_words;                     /* what to allocate */
    int64_t zkey, sh_clamp;                                              /* offsets into the rect buffer */
    int64_t tile_flags, tile_start, tile_fill, counters, pair_cursor;    /* offsets into the tiles buffer */
    int64_t blk_total, blk_base;                                         /* offsets into the pair_idx buffer */
} SpfStateLayout;
int spf_raster_state_layout(int64_t RT, int64_t RG, int64_t RB, SpfStateLayout* out);
/* Which tile (render * T + tile) block slot `slot` (< R*T / 8) of XCD `xcd` (0..7) of a composite lists launch stands for
 * before the end of every XCD's range is sorted longest list first (planned calls on direct bins of >= 2,048 tiles, R*T
 * a multiple of 8): a contiguous range of renders per XCD -- or, for calls of exactly eight renders, strips of 64 tiles
 * dealt out so that no XCD is left with ONE render (strip q of render r -> XCD (r + q) % 8).  A bijection; host-side
 * arithmetic only (documentation and tests).  -1 for arguments out of range. */
int spf_raster_launch_slot_tile(int32_t R, int32_t T, int32_t xcd, int32_t slot);
/* Direct bins: how the (Gaussian, tile) pair numbering of a call of S scenes x G Gaussians is sharded, and the largest
 * number of tiles per render whose histogram the projection kernel keeps in LDS (direct bins need it).
 * spf_raster_pair_shards: 1 or 8.  With 8 shards the blocks of the projection kernel number their pairs from eight
 * cursors (block b -> shard b % 8; one cursor would be a hot word) and shard i owns the gradient records
 * [i * pair_capacity / 8, (i + 1) * pair_capacity / 8): plan flag 1 is raised when ONE shard outgrows its eighth, so a
 * caller that wants "D <= capacity never fails" sizes pair_capacity (and g->gpair) with headroom for the imbalance of a
 * round-robin deal of blocks -- the Python host passes 1.25 x the planned capacity (the shards are interleaved samples of
 * the same scenes: they differ by per cents). */
int spf_raster_pair_shards(int32_t S, int32_t G);
int spf_raster_max_lds_tiles(void);
/* Into how many chunks of renders spf_raster_forward_render (backward = 0) / spf_raster_backward (backward = 1) split a
 * call of S scenes x V views.  1 unless the environment says SPF_CHUNKS=n: then, after the joint tile scan, the chunks
 * (whole scenes each) run as independent launch chains alternating between the caller's stream and one auxiliary stream
 * of the library (fork / join by events; capturable in a HIP graph); results are bit-identical to the single chain and
 * the stage timing below counts one launch per chunk.  Measured slower than the single chain on MI355X (see api.hip),
 * hence off by default. */
int spf_raster_chunks(int32_t S, int32_t V, int32_t H, int32_t W, int32_t backward);
/* Which tile sort kernels a call launches, in launch order, for a longest-list hint (0 = unknown), `tiles_call` tiles in
 * the whole call and the environment as it is now (SPF_SORT_BLOCKS / _SEPARATE / _BIG_MIXED / _LDS_2K / _SINGLE): launch
 * i runs kernel[i] (SPF_SORT_*), which sorts the lists with lo[i] < entries <= hi[i] and returns at once on every other
 * tile, so the intervals must tile (1, hint] without gap or overlap; order[i] is 1 on the launch that also writes the
 * composite kernels' launch order (with_order != 0: the first launch, which is SPF_SORT_ORDER_ONLY when there is
 * nothing to sort).  Arrays of SPF_SORT_MAX_LAUNCHES entries.  The plan the library itself launches from; host-side
 * arithmetic only.  Returns the number of launches, -1 for tiles_call < 1 or a null array. */
#define SPF_SORT_ORDER_ONLY 0   /* spf_tile_order_kernel */
#define SPF_SORT_MIXED 1        /* spf_sort_tiles_mixed_kernel<false>: (1, 2048] */
#define SPF_SORT_MIXED_BIG 2    /* spf_sort_tiles_mixed_kernel<true>: (1, 4096] */
#define SPF_SORT_PAIR 3         /* spf_sort_tiles_pair_kernel: (1, 1024] */
#define SPF_SORT_WAVE8 4        /* spf_sort_tiles_wave_kernel<8, true>: (1, 512] */
#define SPF_SORT_WAVE16 5       /* spf_sort_tiles_wave_kernel<16, true>: (1, 1024] */
#define SPF_SORT_WAVE32 6       /* spf_sort_tiles_wave_kernel<32, false>: (1024, 2048] */
#define SPF_SORT_BLOCK4 7       /* spf_sort_tiles_block_kernel<4>: (512, 1024] */
#define SPF_SORT_BLOCK8 8       /* spf_sort_tiles_block_kernel<8>: (1024, 2048] */
#define SPF_SORT_BLOCK16 9      /* spf_sort_tiles_block_kernel<16>: (2048, 4096] */
#define SPF_SORT_LDS 10         /* spf_sort_tiles_lds_kernel<1024>: (4096, 8192], (2048, 8192] or (8192, 16384] */
#define SPF_SORT_BIG 11         /* spf_sort_tiles_big_kernel: (16384, 0xffffffff] */
#define SPF_SORT_MAX_LAUNCHES 8
int spf_raster_sort_plan(uint32_t max_tile_hint, int32_t tiles_call, int32_t with_order, int32_t* kernel, uint32_t* lo,
                         uint32_t* hi, int32_t* order);

/* Camera tensors from poses / intrinsics, and the gradient of the poses from dL/dviewmatrix
 * (dL_dviewmatrix [R,4,4] in, dL_dextrinsics [R,4,4] out; cam->viewmatrix must hold the forward result). */
int spf_camera_forward(const SpfCamera* cam, void* stream);
int spf_camera_backward(const SpfCamera* cam, const float* dL_dviewmatrix, float* dL_dextrinsics, void* stream);

/* Forward, stage 1: per-Gaussian projection / 2-D covariance / colour, per-tile counts and their
 * scan.  On return (stream order) st->counters[0] = D and st->counters[1] = longest tile list. */
int spf_raster_forward_project(const SpfDims* d, const SpfInputs* in, SpfState* st, void* stream);

/* Decoder fast path (the batched DecoderSplattingCUDA.forward, decoder_splatting_cuda.py:41-78): two launches fewer
 * per step than the calls above.
 *   spf_decoder_prepare           = spf_camera_forward AND the clearing of `zero_bytes` bytes at `zero` in ONE kernel.
 *                                   Pass the tiles buffer of SpfStateLayout and clear all of it (4 * tiles_words bytes;
 *                                   16-byte aligned; without the cursors and the padding: 16*R*T + 20 bytes, rounded up);
 *   spf_raster_forward_project_prepared = spf_raster_forward_project without its own clearing.  `cleared_bytes` says how
 *                                   much of that buffer (from tile_count on) the caller cleared: all of it -> the tile scan
 *                                   runs with one block per render instead of a single block; only the first 8*R*T bytes
 *                                   (the two count arrays) or a buffer laid out differently -> the self-initialising
 *                                   single-block scan; less -> the call clears the counts itself.  Nothing is assumed;
 *   spf_camera_backward_partials  = the deterministic sum of g->vpartial [R,nblk,12] (as written by spf_raster_backward
 *                                   when g->vpartial != NULL; pass g->dL_dviewmatrix = NULL to skip its own reduction)
 *                                   AND spf_camera_backward, in ONE kernel. */
int spf_decoder_prepare(const SpfCamera* cam, void* zero, uint64_t zero_bytes, void* stream);
int spf_raster_forward_project_prepared(const SpfDims* d, const SpfInputs* in, SpfState* st, uint64_t cleared_bytes,
                                        void* stream);
int spf_camera_backward_partials(const SpfCamera* cam, const float* vpartial, int32_t nblk, float* dL_dextrinsics,
                                 void* stream);

/* Forward, stage 2: bin (Gaussian, tile) pairs into per-tile lists, depth-sort every list and
 * composite.  `capacity` = number of uint64 entries st->pairs can hold.  `max_tile_hint` = upper bound of the
 * longest tile list the caller assumes (exact mode: host copy of counters[1]; 0 = unknown: every sort size class
 * is launched).  `dense_tiles_hint` is IGNORED (pass SPF_UNKNOWN): up to round 4 sparse and dense tiles had a kernel
 * each and the hint let the host skip one; since round 5 one kernel composites every tile in the form that suits it.
 * A caller that PLANS the call from an earlier one instead of reading the counters back (no device->host
 * synchronisation; capturable in a HIP graph) passes its assumptions here and they are checked on the device:
 * counters[2] = 0 if the plan held, else a bit mask: 1 = D > capacity, 2 = a tile list longer than max_tile_hint
 * (it could not be sorted); bit 4 (a wrong dense_tiles_hint, rounds 2 - 4) is never set.  A failed plan is
 * never silent and never undefined: with a non-zero flag EVERY output of this call (image, depth, alpha) and every
 * gradient of the matching backward is filled with NaN -- deterministic, and caught by the reference's own
 * NaN-gradient guard (src/model/model_wrapper.py:1117-1151) even if the caller never reads the flag. */
int spf_raster_forward_render(const SpfDims* d, const SpfInputs* in, SpfState* st, SpfOutputs* out,
                              uint64_t capacity, uint32_t max_tile_hint, uint32_t dense_tiles_hint, void* stream);

/* Backward of both stages.  `capacity` = number of 10-float records g->gpair can hold (>= D); `dense_tiles_hint`: ignored,
 * as in spf_raster_forward_render. */
int spf_raster_backward(const SpfDims* d, const SpfInputs* in, const SpfState* st,
                        const SpfGrads* g, uint64_t capacity, uint32_t dense_tiles_hint, void* stream);

/* Precomputed 3-D covariances (the public rasterizer's cov3Ds_precomp) in place of the scale/rotation pair, forward
 * and backward.  Everything else -- dims, inputs, state, outputs, upstream gradients, spf_raster_forward_render between
 * the two -- is what the calls above take.
 *   cov3D [S,G,6]       the upper triangle of each Gaussian's Sigma in 3DGS order (xx, xy, xz, yy, yz, zz); the lower
 *                       triangle is implied by symmetry.  Used as given: SpfDims.scale_modifier does NOT apply (as in the
 *                       public 3DGS rasterizer); SpfInputs.view_scale does, render (s, v) sees Sigma * k^2 with
 *                       k = view_scale[s, v] (the reference's scale-invariant rescale, cuda_splatting.py:70).
 *   dL_dcov3D [S,G,6]   or NULL (enable_cov_grad off: no covariance gradient is produced).  Diagonal entry i receives
 *                       G_ii, off-diagonal entry (i, j) G_ij + G_ji -- G the gradient w.r.t. the full 3x3 matrix, since
 *                       the stored value fills both symmetric slots (autograd through Sigma = sym(cov6); 3DGS's
 *                       computeCov2DCUDA backward).
 *   Input domain        covariances are positive semidefinite.  The projection kernels factor Sigma = L L^T once per
 *                       Gaussian (Cholesky in float64, rounded to float32) and use L where the scale/rotation path uses
 *                       R diag(s): a rank-deficient Sigma (a flat splat, one zero eigenvalue) renders exactly.  A
 *                       non-positive pivot is taken as zero together with the rest of its column, so an INDEFINITE Sigma
 *                       neither faults nor produces NaN: it renders as L L^T of that clamped factor, and dL_dcov3D is the
 *                       gradient at that matrix.
 *   Rejected (SPF_E_INVALID, before any launch): in->scales or in->rotations non-NULL, g->dL_dscales or
 *                       g->dL_drotations non-NULL, sh_layout 2 (band split) or 3 (raw rows), cov3D NULL.
 *   spf_raster_forward_project_cov3d: `cleared_bytes` as in spf_raster_forward_project_prepared; 0 = the call clears
 *                       for itself, like spf_raster_forward_project.
 *   spf_raster_backward_cov3d: spf_raster_backward with the covariance gradient; the call always runs as one launch
 *                       chain (SPF_CHUNKS does not split it). */
int spf_raster_forward_project_cov3d(const SpfDims* d, const SpfInputs* in, const float* cov3D /* [S,G,6] */,
                                     SpfState* st, uint64_t cleared_bytes, void* stream);
int spf_raster_backward_cov3d(const SpfDims* d, const SpfInputs* in, const float* cov3D, const SpfState* st,
                              const SpfGrads* g, float* dL_dcov3D /* [S,G,6] or NULL */, uint64_t capacity,
                              uint32_t dense_tiles_hint, void* stream);

/* Fused Gaussian adapter (UnifiedGaussianAdapter.forward, src/model/encoder/common/gaussian_adapter.py:122-150):
 * raw[N, 7+3K] network channels (row stride `raw_stride` floats >= 7+3K: the encoder hands over `gaussians[..., 1:]`, a view
 * of its 83-channel head output, encoder_spfsplatv2.py:261-268 -- read in place, no contiguous copy) ->
 * scales[N,3] = min(0.001*softplus, 0.3), rotations[N,4] = q/(|q|+eps), harmonics[N,3,K] = raw[7:] * sh_mask[K];
 * with harmonics_high != NULL (K = 25): the band-split layout, harmonics = [N,3,16] and harmonics_high = [N,3,9]
 * (SpfDims.sh_layout 2).  One pass: every raw row is read once, through LDS, and every output is written coalesced.
 * Backward: dL_draw[N, 7+3K] (contiguous); any upstream gradient may be NULL = zero; `split` says dL_dharmonics is
 * [N,3,16] with band 4's gradient in dL_dharmonics_high [N,3,9] -- or NULL, which is never read and costs nothing. */
int spf_adapter_forward(const float* raw, int64_t raw_stride, int64_t N, int32_t K, const float* sh_mask, float eps,
                        float* scales, float* rotations, float* harmonics, float* harmonics_high, void* stream);
int spf_adapter_backward(const float* raw, int64_t raw_stride, int64_t N, int32_t K, const float* sh_mask, float eps,
                         const float* dL_dscales, const float* dL_drotations, const float* dL_dharmonics,
                         const float* dL_dharmonics_high, int32_t split, float* dL_draw, void* stream);

/* Photometric MSE on the decoder output (LossMse.forward, src/loss/loss_mse.py:36-51):
 * loss[0] = weight * mean((prediction - image)^2) over n floats, and its backward
 * dL_dprediction = (2 * weight / n) * dL_dloss[0] * (prediction - image) (dL_dloss is read on the device).
 * partial: scratch of spf_mse_partial_blocks() floats.  The sum is taken in a fixed order: results are run-to-run
 * identical.  Tensors 16-byte aligned. */
int spf_mse_partial_blocks(void);
int spf_mse_forward(const float* prediction, const float* image, int64_t n, float weight, float* partial,
                    float* loss, void* stream);
int spf_mse_backward(const float* prediction, const float* image, int64_t n, float weight, const float* dL_dloss,
                     float* dL_dprediction, void* stream);
/* The same forward that ALSO writes dL_dprediction_unit[i] = (2 * weight / n) * (prediction[i] - image[i]) -- the gradient
 * for dL_dloss = 1 -- so that the backward is spf_mse_scale_grad: dL_dprediction[i] *= dL_dloss[0] in place, which returns
 * after one scalar read when dL_dloss[0] is exactly 1 (what `loss.backward()` passes): the backward of the loss costs a
 * launch instead of a pass over prediction, image and gradient. */
int spf_mse_forward_grad(const float* prediction, const float* image, int64_t n, float weight, float* partial,
                         float* loss, float* dL_dprediction_unit, void* stream);
int spf_mse_scale_grad(float* dL_dprediction, int64_t n, const float* dL_dloss, void* stream);

/* Reprojection loss (LossReproj.forward, src/loss/loss_reproj.py:53-101, with project_to_cam,
 * src/misc/cam_utils.py:289-307) for B x V images at once; view v is normalised by its own valid count over the B images,
 * which is what V separate calls of the reference return.  Per point n = i W + j of image (b, v):
 *   cam = W[:3,:3] p + W[:3,3] with W = inverse(pose) (a general 4x4 inverse, float64, rounded to float32);
 *   q = K' cam with K' = K, row 0 scaled by W and row 1 by H; px = q.xy / max(q.z, 1e-6);
 *   e = |px - (j, i)|; valid iff !(e > hard_clamp) (NaN is valid and propagates);
 *   loss[v] = weight * sum_valid term(e) / n_valid, 0 (and zero gradients) when no point is valid.
 * term: SPF_REPROJ_TANH lw tanh(e / lw) ("tanh": lw = soft_clamp; "dyntanh": lw from the schedule, on the host);
 *       SPF_REPROJ_L1 e where !(e > soft_clamp); SPF_REPROJ_L1_SQRT that + sqrt(soft_clamp e) where e > soft_clamp;
 *       SPF_REPROJ_L1_LOG that + log(1 + soft_clamp e) where e > soft_clamp (the reference's `else`: any other mode).
 * pts3d is read in place: element strides stride_b, stride_v (>= 0) for its first two dimensions; each image's H*W*3
 * floats are contiguous (16-byte aligned images are read with 16-byte loads).  poses [B,V,4,4] (camera -> world) and
 * intrinsics [B,V,3,3] (normalised) are contiguous.  A singular pose gives non-finite results (torch.inverse raises).
 * No atomics, no allocation, no synchronisation; results are run-to-run identical, and view v's results do not depend on
 * V (the batched call equals the per-view calls bitwise). */
#define SPF_REPROJ_TANH 0
#define SPF_REPROJ_L1 1
#define SPF_REPROJ_L1_SQRT 2
#define SPF_REPROJ_L1_LOG 3
typedef struct SpfReproj {
    const float* pts3d;
    int64_t stride_b, stride_v;
    const float* poses;
    const float* intrinsics;
    int32_t B, V, H, W;
    int32_t mode;                 /* SPF_REPROJ_* */
    float weight, lw, hard_clamp, soft_clamp;
} SpfReproj;
/* Scratch sizing: the number of (1024-point chunk, image) slots, B * V * ceil(H W / 1024), or -1 for bad sizes.  The
 * forward needs 2 * slots 32-bit words of `partial`, the backward 24 * slots floats of `gpartial` (16-byte aligned). */
int64_t spf_reproj_partial_blocks(int32_t B, int32_t V, int32_t H, int32_t W);
/* Forward (two launches): loss[V], and scale[V] = weight / n_valid (0 when none) for the backward. */
int spf_reproj_forward(const SpfReproj* args, void* partial, float* loss, float* scale, void* stream);
/* Backward (one or two launches): dL_dloss[V] and scale[V] are read on the device.  dL_dpts3d [B,V,H,W,3] contiguous, or
 * NULL when pts3d needs no gradient; dL_dposes [B,V,4,4] and dL_dintrinsics [B,V,3,3] contiguous, either may be NULL;
 * gpartial is needed (and only then) when one of them is given. */
int spf_reproj_backward(const SpfReproj* args, const float* scale, const float* dL_dloss, float* dL_dpts3d,
                        float* gpartial, float* dL_dposes, float* dL_dintrinsics, void* stream);

/* Distillation point loss (Regr3D.forward, src/loss/loss_point.py:188-254, norm_mode 'avg_dis' or none) of two views of
 * B point maps of n = H W points.  With dis = |gt| in float32, per view v and batch item b:
 *   quantile mode (has_dist_clip = 0): q_lo, q_hi = torch.quantile(dis[b], [0.002, 0.998]) by torch's definition -- rank
 *     r = float32(q) * (n - 1) in float32, lerp(sorted[floor r], sorted[ceil r], r - floor r) -- the four order statistics
 *     found EXACTLY by a radix select over the bit patterns (histogram passes, no sort);
 *     valid = q_lo <= dis <= q_hi and conf >= 3;
 *   clip mode (has_dist_clip = 1): valid = dis <= dist_clip; conf1 / conf2 are not read (may be NULL);
 *   nf_pr[b] = max((sum_valid1 |pr1| + sum_valid2 |pr2|) / (n1[b] + n2[b] + 1e-8), 1e-8), nf_gt[b] likewise from gt
 *     (normalize = 0: both are 1; gt_scale = 1: nf_gt is 1);
 *   loss_v = mean over ALL valid points of view v of |pr / nf_pr[b] - gt / nf_gt[b]| (NaN for a view without one: the mean
 *     of nothing); loss = loss_1 + loss_2, or loss_2 with disable_view1.
 * A NaN norm compares false, so such a point is invalid; it orders above +inf in the select (torch.quantile would
 * return NaN for that row).
 * gt_pts*, pr_pts* are read in place: batch item b of a tensor starts b * stride floats from its pointer (stride >= 0),
 * its H*W*3 floats are contiguous, and a 16-byte aligned row is read with 16-byte loads.  conf1, conf2 [B,H,W] are
 * contiguous.  No float atomics, no allocation, no synchronisation: every float sum is formed from per-slot partials in a
 * fixed order, so results are run-to-run identical and do not depend on the strides. */
typedef struct SpfRegr3d {
    const float* gt_pts1;
    const float* gt_pts2;
    const float* pr_pts1;
    const float* pr_pts2;
    const float* conf1;
    const float* conf2;
    int64_t stride_gt1, stride_gt2, stride_pr1, stride_pr2;
    int32_t B, H, W;
    int32_t has_dist_clip;        /* 0: quantile mask (dist_clip is None in the reference); 1: dis <= dist_clip */
    float dist_clip;
    int32_t disable_view1;
    int32_t normalize;            /* norm_mode 'avg_dis' (1) or falsy (0) */
    int32_t gt_scale;             /* 1: the ground truth is not normalised */
} SpfRegr3d;
/* Bytes of the caller's scratch (16-byte aligned; it carries the per-slot partials and the per-row scalars from the forward
 * to the backward -- nothing per point), or -1 for sizes the forward would reject.  Host only. */
int64_t spf_regr3d_scratch_bytes(int32_t B, int32_t H, int32_t W);
/* Forward: loss[1], and the stats block of 8 B 32-bit words that the backward reads and a caller may log:
 *   n_valid[2][B] (int32) | q[2][B][2] (q_lo, q_hi; clip mode: 0, dist_clip) | nf_pr[B] | nf_gt[B]. */
int spf_regr3d_forward(const SpfRegr3d* args, void* scratch, float* stats, float* loss, void* stream);
/* Backward (one launch) after the forward on the same args, scratch and stats: d_pr1, d_pr2 [B,H,W,3] contiguous, either may
 * be NULL (not wanted; at least one is).  dL_dloss[1] is read on the device.  Both the direct term and the path through
 * nf_pr count (with disable_view1, pr_pts1 still receives the latter); |x| has gradient 0 at 0; invalid points get
 * exactly 0. */
int spf_regr3d_backward(const SpfRegr3d* args, const void* scratch, const float* stats, const float* dL_dloss,
                        float* d_pr1, float* d_pr2, void* stream);

/* The pose path.  Every function: float32 in and out, no allocation, no synchronisation, no atomics; every float sum has
 * one order, so a run repeats bitwise and a strided view gives the bits of its contiguous copy.
 *
 * Pose composition (process_pose).  enc[b, v, 9]: view (s, i) starts at enc + s * stride_b + i * stride_v floats, its nine
 * floats are contiguous.  Encodings:
 *   SPF_POSE_ROT6D  columns 0:3 = a1, 3:6 = a2: b1 = a1 / max(|a1|, 1e-12), b2 = normalise(a2 - (b1 . a2) b1) likewise,
 *                   b3 = b1 x b2 are the ROWS of R; columns 6:9 = t; (R, t) is camera -> world.
 *   SPF_POSE_QUAT   ("absT_quaR_FoV") columns 0:3 = T, 3:7 = a scalar-LAST quaternion that is NOT normalised
 *                   (two_s = 2 / sum q^2), 7:9 ignored (zero gradient); (R, T) is world -> camera and the pose is its
 *                   closed-form inverse [R^T | -R^T T].
 * make_baseline_1: all translations of a scene are divided by |t_0 - t_{context_views - 1}|.  make_relative: every view is
 * left-multiplied by the GENERAL inverse (float64) of view 0.  poses[b, v, 4, 4] contiguous, bottom rows exactly 0 0 0 1.
 * The backward recomputes everything from enc: dL_dposes[b, v, 4, 4] -> dL_denc[b, v, 9], both contiguous. */
#define SPF_POSE_ROT6D 0
#define SPF_POSE_QUAT 1
int spf_pose_compose_forward(const float* enc, int64_t stride_b, int64_t stride_v, int32_t b, int32_t v,
                             int32_t context_views, int32_t encoding, int32_t make_baseline_1, int32_t make_relative,
                             float* poses, void* stream);
int spf_pose_compose_backward(const float* enc, int64_t stride_b, int64_t stride_v, int32_t b, int32_t v,
                              int32_t context_views, int32_t encoding, int32_t make_baseline_1, int32_t make_relative,
                              const float* dL_dposes, float* dL_denc, void* stream);

/* Depth projection (depth_projector): depth[i, p] = (inverse(poses[i]) [pts[i, p], 1])_z for pts[N, n, 3] (image i starts
 * i * stride_img floats from pts, its 3 n floats are contiguous; a 16-byte aligned image is read with 16-byte loads) and
 * poses[N, 4, 4] contiguous; the inverse is a general float64 inverse, once per image.  depth[N, n] contiguous.
 * Backward: dL_dpts[N, n, 3] contiguous (may be NULL) = g W[2, :3]; dL_dposes[N, 4, 4] (may be NULL, then gpartial too) =
 * -W^T dW W^T with dW[2, :] = sum_p g [p, 1], summed over gpartial: 4 floats per slot, 16-byte aligned,
 * spf_depth_project_partial_blocks(N, n) slots (-1 for sizes the calls would reject). */
int64_t spf_depth_project_partial_blocks(int32_t N, int32_t n);
int spf_depth_project_forward(const float* pts, int64_t stride_img, const float* poses, int32_t N, int32_t n, float* depth,
                              void* stream);
int spf_depth_project_backward(const float* pts, int64_t stride_img, const float* poses, int32_t N, int32_t n,
                               const float* dL_ddepth, float* dL_dpts, float* gpartial, float* dL_dposes, void* stream);

/* Pose errors of N pairs of 4x4 poses (contiguous), one launch: errors[N, 3] = (error_t, error_t_scale, error_R) per pair
 * and means[3].  error_R = deg |acos(clamp((tr(R_pred^T R_gt) - 1) / 2, -1, 1))|; error_t = deg acos(clamp(t . t_gt /
 * (|t| |t_gt| + 1e-9), -1, 1)), then min(e, 180 - e); error_t_scale = |t - t_gt|.  Evaluated in float64 and rounded at the
 * store (the reference's float32 acos loses up to 0.03 degrees near 0 and 180). */
int spf_pose_error(const float* pred, const float* gt, int32_t N, float* errors, float* means, void* stream);

/* Focal estimate (estimate_focal_knowing_depth, 'weiszfeld'), one focal per scene over the H W points of ONE image: scene s
 * starts s * stride_scene floats from pts, its row i another i * stride_row, a row's 3 W floats are contiguous.  Valid:
 * z > 0 (NaN is not).  a = (x / z, y / z) with +-inf and NaN replaced by 0; pixel (j - pp_x, i - pp_y), pp a device pointer
 * to one pair (pp_stride 0) or one per scene (pp_stride 2), NULL: (W / 2, H / 2).  f0 = sum a . px / sum a . a, focal_base =
 * max(H, W) / (2 tan 30 deg) if f0 <= 0; ten rounds f = sum w (a . px) / sum w (a . a), w = 1 / max(|px - f a|, 1e-8); clip to
 * [min_focal, max_focal] focal_base; focal_base if the result is <= 0.  No valid point gives NaN (NaN takes no <= 0
 * branch).  Per-point float32, the running sums float64.  focal[B]; intrinsics[B, 3, 3] (may be NULL) = rows (f, 0, cx) /
 * div0, (0, f, cy) / div1, (0, 0, 1) in float32.  spf_focal_scratch_bytes: bytes of scratch the call needs (16-byte
 * aligned; 0 today -- a scene is one block's work -- and then scratch may be NULL), -1 for sizes it would reject. */
int64_t spf_focal_scratch_bytes(int32_t B, int32_t H, int32_t W);
int spf_focal_estimate(const float* pts, int64_t stride_scene, int64_t stride_row, int32_t B, int32_t H, int32_t W,
                       const float* pp, int64_t pp_stride, float min_focal, float max_focal, float cx, float cy, float div0,
                       float div1, void* scratch, float* focal, float* intrinsics, void* stream);

/* SSIM (ssim / SSIM, src/loss/loss_ssim.py:58-189, and compute_ssim, src/evaluation/metrics.py:36-52) of X, Y [N,C,H,W]
 * contiguous float32, every H x W plane on its own.  With the 1-D window win[0 .. ws) (ws odd, 3 .. 33) applied along
 * both axes over the VALID region, n_valid = (H - ws + 1)(W - ws + 1) positions, and E[.] the filtered moments:
 *   mu_x = E[x], mu_y = E[y], s_x = cov_norm (E[xx] - mu_x^2), s_y likewise, s_xy = cov_norm (E[xy] - mu_x mu_y)
 *   S = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1) * (2 s_xy + C2) / (s_x + s_y + C2)
 *   plane_mean[n,c] = sum S / n_valid
 *   out: size_average ? mean over all planes (1 float) : mean over the channels (N floats); with `nonnegative` each
 *   plane's mean goes through relu first.
 * cov_norm = 1 is the reference's `_ssim`; cov_norm = 121/120 with ws = 11 is scikit-image's Gaussian-weighted
 * structural_similarity (sample covariance), which compute_ssim calls.  The moment maps and the S map stay in LDS and
 * registers.  No atomics, no allocation, no synchronisation; results are run-to-run identical and a plane's numbers do
 * not depend on the other planes of the call.  Planes may start at any 4-byte aligned address. */
#define SPF_SSIM_MAX_WIN 33
typedef struct SpfSsim {
    const float* X;
    const float* Y;
    int32_t N, C, H, W;
    int32_t ws;                   /* window length: odd, 3 .. SPF_SSIM_MAX_WIN, <= H and <= W */
    float C1, C2, cov_norm;
    int32_t size_average;         /* 0: out[N]; otherwise out[1] */
    int32_t nonnegative;          /* relu on every plane's mean */
    float win[SPF_SSIM_MAX_WIN];  /* the window's weights, by value; entries from ws on are ignored */
} SpfSsim;
/* Scratch sizing (host only, no GPU): the number of (tile, plane) slots of the forward = floats of `partial`, or -1 for
 * sizes that the forward would reject. */
int64_t spf_ssim_partial_blocks(int32_t N, int32_t C, int32_t H, int32_t W, int32_t ws);
/* Forward (three launches): plane_mean [N,C] (before the relu; the backward reads it) and out. */
int spf_ssim_forward(const SpfSsim* args, float* partial, float* plane_mean, float* out, void* stream);
/* Backward (one launch): dL_dX and / or dL_dY [N,C,H,W] contiguous (NULL: not wanted; at least one is).  dL_dout (1 or N
 * floats, as `out`) and plane_mean are read on the device.  The moments are recomputed from X and Y: nothing but
 * plane_mean is kept between the passes. */
int spf_ssim_backward(const SpfSsim* args, const float* plane_mean, const float* dL_dout, float* dL_dX, float* dL_dY,
                      void* stream);
/* PSNR (compute_psnr, src/evaluation/metrics.py:11-19) of N images of n floats each, contiguous:
 * psnr[i] = -10 log10(mean((clip(gt, 0, 1) - clip(pred, 0, 1))^2)), +inf for identical images.  One launch, fixed order. */
int spf_psnr_forward(const float* ground_truth, const float* predicted, int32_t N, int64_t n, float* psnr, void* stream);

/* LPIPS (lpips 0.1, net="vgg", lpips=True, spatial=False, evaluation mode; LossLpips, src/loss/loss_lpips.py:57-85, and
 * compute_lpips, src/evaluation/metrics.py:22-33) of N image pairs in0[n], in1[n], each [3,H,W] float32 with contiguous
 * planes, H, W >= 16:
 *   x <- 2x - 1 (normalize), x <- (x - shift_c) / scale_c; VGG16 features (zero padding 1 applied AFTER that step, bias,
 *   ReLU, 2x2 max pool in front of blocks 2..5); taps relu1_2, relu2_2, relu3_3, relu4_3, relu5_3;
 *   per tap and pixel u = a / (||a|| + 1e-10), v likewise, d = sum_c lin[c] (u_c - v_c)^2; out[n] = sum over the taps
 *   of the mean of d over the tap's pixels.
 * Weights, packed once by the caller (all float32, 16-byte aligned):
 *   wfwd   per layer l = 0..12 in order [tap = 3 dy + dx][C_in][C_out] = W_l[c_out][c_in][dy][dx]
 *   wbwd   per layer [tap][C_out][C_in] = W_l[c_out][c_in][2 - dy][2 - dx] (the backward-data convolution)
 *   bias   the 13 bias vectors in order; lin: the five 1x1 vectors (64, 128, 256, 512, 512) in order
 *   shift_scale  shift[3] then scale[3]
 * The convolutions run on the float32 matrix instructions (every output the sum of nine k-ordered fmaf chains, one per
 * tap); activations are
 * channels-last inside the workspace.  No atomics, no allocation, no synchronisation: results are run-to-run identical
 * and a pair's numbers do not depend on the other pairs of the call.  Where a feature vector is all zero the 1 / ||a||
 * term of the gradient is taken as 0. */
typedef struct SpfLpips {
    const float* in0;
    const float* in1;
    int64_t stride0, stride1;     /* floats from one image to the next (>= 3 H W) */
    int32_t N, H, W;
    int32_t normalize;            /* 1: inputs are in [0, 1] */
    float weight;                 /* of the mean (spf_lpips_forward's `mean`, and the backward from it) */
    int32_t reserved;
    const float* wfwd;
    const float* wbwd;
    const float* bias;
    const float* lin;
    const float* shift_scale;
} SpfLpips;
/* Bytes of the caller-allocated workspace for n_total = 2 N images of which n_with_grad (0, N or 2 N) will go through
 * the backward trunk; negative for unsupported sizes.  Host only. */
int64_t spf_lpips_workspace_bytes(int32_t n_with_grad, int32_t n_total, int32_t h, int32_t w);
/* Forward (the whole launch chain): out[N], and when `mean` is given mean[0] = weight * mean_n out[n].  The workspace
 * keeps every activation for the backward. */
int spf_lpips_forward(const SpfLpips* args, void* workspace, float* out, float* mean, void* stream);
/* Backward after spf_lpips_forward on the same workspace: d_in0 and / or d_in1 [N,3,H,W] contiguous (NULL: not wanted; at
 * least one is; only the wanted images run the backward trunk).  dL_dout: N floats, or with upstream_is_mean one float,
 * the gradient of `mean`; read on the device. */
int spf_lpips_backward(const SpfLpips* args, void* workspace, const float* dL_dout, int32_t upstream_is_mean,
                       float* d_in0, float* d_in1, void* stream);
/* The kernels of the chain one at a time, on channels-last [n,h,w,c] float32 tensors (the tests drive these).
 * conv3x3: out[n,h,w,cout] = (relu)(conv(in where mask > 0, wpack) + bias); wpack [9][cin][cout] (a layer's slice of wfwd,
 * or of wbwd with cin and cout swapped); mask (same shape as in) and bias may be NULL; cin % 16 == 0, cout % 64 == 0. */
int spf_lpips_conv3x3(const float* in, const float* mask, const float* wpack, const float* bias, float* out, int32_t n,
                      int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t relu, void* stream);
/* First layer on args->in0 (N images, [3,H,W] planes) -> out [N,H,W,64]; and its backward-data: g, act [N,H,W,64] ->
 * d_in0 [N,3,H,W], g counted where act > 0. */
int spf_lpips_conv1_forward(const SpfLpips* args, float* out, void* stream);
int spf_lpips_conv1_backward(const SpfLpips* args, const float* g, const float* act, float* d_in0, void* stream);
/* 2x2 max pool (floor mode) [n,h,w,c] -> [n,h/2,w/2,c], c % 4 == 0; backward: inout [n,h,w,c] += gp routed to the first
 * maximum (row-major) of each window of act. */
int spf_lpips_pool_forward(const float* in, float* out, int32_t n, int32_t h, int32_t w, int32_t c, void* stream);
int spf_lpips_pool_backward(const float* gp, const float* act, float* inout, int32_t n, int32_t h, int32_t w, int32_t c,
                            void* stream);
/* One tap of the head on fa, fb [n,hw,c] (c = 64, 128, 256 or 512): out[n] = mean over the pixels of d; partial:
 * n * ceil(hw / 64) floats of scratch.  Backward: d_a and / or d_b [n,hw,c] from the upstream gradient up[n]. */
int spf_lpips_head_forward(const float* fa, const float* fb, const float* lin, int32_t n, int32_t hw, int32_t c,
                           float* partial, float* out, void* stream);
int spf_lpips_head_backward(const float* fa, const float* fb, const float* lin, int32_t n, int32_t hw, int32_t c,
                            const float* up, float* d_a, float* d_b, void* stream);

/* In-place 2-D rotary embedding.  tokens[B,N,H,D] with element strides (stride_b, stride_n, stride_h) and
 * stride(D) == 1; dtype: 0 = float32, 1 = float16, 2 = bfloat16.  positions[B / pos_div, N, 2] int64 contiguous
 * (y, x): batch item b uses positions[b / pos_div] (pos_div = 1 for the CroCo layout; a head-major [B,H,N,D] tensor
 * is passed as B*H batches of one head with pos_div = H).  fwd = +F0 for forward, -F0 for backward. */
int spf_rope2d(void* tokens, const int64_t* positions, int32_t B, int32_t N, int32_t H, int32_t D,
               int64_t stride_b, int64_t stride_n, int64_t stride_h, int32_t pos_div, int32_t dtype, float base,
               float fwd, void* stream);
/* The same rotation applied to TWO tensors of identical shape, strides, dtype and positions in one launch (the angles
 * are evaluated once): q and k of an attention layer, which the reference rotates with two calls
 * (src/model/encoder/backbone/croco/blocks.py:102-104). */
int spf_rope2d_pair(void* tokens, void* tokens2, const int64_t* positions, int32_t B, int32_t N, int32_t H, int32_t D,
                    int64_t stride_b, int64_t stride_n, int64_t stride_h, int32_t pos_div, int32_t dtype, float base,
                    float fwd, void* stream);

/* Fused RoPE attention, head dim 64 (croco/blocks.py Attention.forward:94-113 and CrossAttention.forward:150-179
 * without mask and dropout):  out = softmax(scale * R(qpos) q * (R(kpos) k)^T) * v.
 * q [B,H,Nq,64] and k, v [B,H,Nk,64] are read through element strides (batch, token, head; stride(D) == 1), so the
 * views of a packed [B,N,3,H,D] projection are read in place.  Every row must be 16-byte aligned (pointers and
 * strides * element size).  dtype: 0 = float32, 1 = float16, 2 = bfloat16 (one float32 compute path).  qpos [B,Nq,2],
 * kpos [B,Nk,2]: int64 contiguous (y, x), rotation of spf_rope2d with (base, F0); both null: no rotation. */
typedef struct SpfAttn {
    const void* q;
    const void* k;
    const void* v;
    const int64_t* qpos;
    const int64_t* kpos;
    int64_t q_stride[3], k_stride[3], v_stride[3];
    int32_t B, H, Nq, Nk, D, dtype;
    float base, F0, scale;
} SpfAttn;
/* Where the backward writes: dq [B,H,Nq,64], dk, dv [B,H,Nk,64] through strides of their own (the three may be views of
 * one packed gradient), same dtype as the inputs; delta: B*H*Nq floats of scratch. */
typedef struct SpfAttnGrads {
    void* dq;
    void* dk;
    void* dv;
    int64_t dq_stride[3], dk_stride[3], dv_stride[3];
    float* delta;
} SpfAttnGrads;
/* out [B,Nq,H*64] contiguous (dtype), lse [B,H,Nq] float32 (log-sum-exp of the scaled scores, for the backward).
 * Nothing is allocated or synchronised. */
int spf_attn_forward(const SpfAttn* args, void* out, float* lse, void* stream);
/* out, lse: what the forward wrote; dout [B,Nq,H*64] contiguous.  No atomics: bitwise reproducible. */
int spf_attn_backward(const SpfAttn* args, const SpfAttnGrads* grads, const void* out, const float* lse,
                      const void* dout, void* stream);

/* The same two calls on the 16-bit matrix units (an additive, opt-in family: nothing above moves): dtype must be 1
 * (float16) or 2 (bfloat16); every product runs on the 32x32x16 f16 / bf16 matrix instructions with float32 accumulators.
 * q and k are rotated in float32 and rounded once to the element type; the score, the softmax statistics, lse, delta, the
 * scale factor and the gradients' rotate-back stay float32; the probabilities (and dS in the backward) are rounded once
 * to the element type as operands; out, dq, dk and dv are rounded at the store.  Same arguments, same checks and messages
 * as spf_attn_forward / spf_attn_backward; nothing is allocated or synchronised; no atomics: bitwise reproducible. */
int spf_attn16_forward(const SpfAttn* args, void* out, float* lse, void* stream);
int spf_attn16_backward(const SpfAttn* args, const SpfAttnGrads* grads, const void* out, const float* lse,
                        const void* dout, void* stream);

/* The same attention with the two things vggt/layers/attention.py adds (an additive family: SpfAttn, SpfAttnGrads and
 * the two entry points above do not move):
 *   score = scale * R(qpos) LN_q(q) * (R(kpos) LN_k(k))^T + mask[b,h,q,k]
 * mask (null: none): read in place through four element strides (batch, head, query, key); a stride of 0 broadcasts
 * that axis, the key stride must be 1, nothing else about its alignment is assumed.  mask_dtype 0: float32, added to
 * the score (-inf excludes a key); 1: bool / uint8, nonzero = the key takes part, zero = -inf.  A row whose keys are
 * all excluded gives out = 0 and lse = -inf and contributes exactly zero to every gradient.  The mask has no gradient.
 * q_weight, q_bias, k_weight, k_bias (all four or none): float32[64] each, LayerNorm over the 64 elements of every q
 * and every k row with `eps` (biased variance, float32, two passes), applied while the row is staged, before the
 * rotation; q and k are never written back normalised.
 * Backward only: dq_weight, dq_bias, dk_weight, dk_bias float32[64] each (written, not accumulated) and `partials`,
 * spf_attn_ext_scratch_floats(B, H, Nq, Nk) floats of scratch: every block writes its rows' sums there and one small
 * kernel adds them in block order in double -- no atomics, bitwise reproducible.  dq and dk are the gradients of the
 * rows BEFORE the normalisation. */
typedef struct SpfAttnExt {
    const void* mask;
    int32_t mask_dtype;
    int64_t mask_stride[4];
    const float* q_weight;
    const float* q_bias;
    const float* k_weight;
    const float* k_bias;
    float eps;
    float* dq_weight;
    float* dq_bias;
    float* dk_weight;
    float* dk_bias;
    float* partials;
} SpfAttnExt;
/* Floats of SpfAttnExt.partials for a backward call of these sizes (-1: invalid sizes). */
int64_t spf_attn_ext_scratch_floats(int32_t B, int32_t H, int32_t Nq, int32_t Nk);
/* spf_attn_forward / spf_attn_backward with the extras; ext without a mask and without norm parameters is the plain
 * call.  Argument errors return SPF_E_INVALID before anything is launched. */
int spf_attn_forward_ext(const SpfAttn* args, const SpfAttnExt* ext, void* out, float* lse, void* stream);
int spf_attn_backward_ext(const SpfAttn* args, const SpfAttnGrads* grads, const SpfAttnExt* ext, const void* out,
                          const float* lse, const void* dout, void* stream);

/* The same attention for a multi-view decoder's cross-attention (an additive family: nothing above moves; plain only,
 * no mask and no q/k norm).  A scene has Vq query views and ONE set of Vk key views that all its query views share:
 *   out[b,i] = softmax_j(scale * R(qpos[b,i]) q[b,i] * (R(kpos[b,s]) k[b,s,j])^T) v[b,s,j],
 *   j over all tokens of all key views s with bit s of allow[i] set, views ascending
 * -- the reference's expression on keys gathered per query view (backbone_croco_multiview.py generate_ctx_views), without
 * the gather.  SpfAttn describes one (scene, view): B = scenes, q [B,Vq,H,Nq,64], k and v [B,Vk,H,Nk,64] with
 * q_stride[0] / k_stride[0] / v_stride[0] the element stride between SCENES and the strides below between VIEWS, so a
 * slice x[:, 1:] of a [b, v, l, c] projection is read in place.  qpos [B,Vq,Nq,2], kpos [B,Vk,Nk,2] int64 with contiguous
 * (token, 2) rows, read through (scene, view) strides in int64 elements; both null: no rotation.  allow: a host-known
 * table, the same for every scene, passed by value (Vq, Vk <= 32); every query view must read at least one key view.
 * The gradients' scene strides are SpfAttnGrads' batch strides, their view strides are below; a key view that no query
 * view reads gets zeros.  All view strides must keep rows 16-byte aligned, and the rows of one view must lie within
 * 2^31 elements of its first (N * token stride; scenes and views are reached through 64-bit strides). */
typedef struct SpfAttnViews {
    int32_t Vq, Vk;
    uint32_t allow[32];
    int64_t q_view_stride, k_view_stride, v_view_stride;
    int64_t qpos_stride[2], kpos_stride[2];
    int64_t dq_view_stride, dk_view_stride, dv_view_stride;     /* backward only */
} SpfAttnViews;
/* out [B,Vq,Nq,H*64] contiguous (dtype), lse [B,Vq,H,Nq] float32.  Argument errors return SPF_E_INVALID before anything
 * is launched; nothing is allocated or synchronised. */
int spf_attn_views_forward(const SpfAttn* args, const SpfAttnViews* views, void* out, float* lse, void* stream);
/* out, lse: what the forward wrote; dout [B,Vq,Nq,H*64] contiguous; grads->delta: B*Vq*H*Nq floats of scratch.  No
 * atomics: every dq, dk, dv row is written once, in a fixed order of sums -- bitwise reproducible. */
int spf_attn_views_backward(const SpfAttn* args, const SpfAttnViews* views, const SpfAttnGrads* grads, const void* out,
                            const float* lse, const void* dout, void* stream);

/* ---- the guarded AdamW step (spfsplatv2_amd/csrc/optim.hip) --------------------------------------------------------
 * One call steps a whole parameter set: T float32 tensors of any sizes.  Three launches on the given stream and no
 * host synchronisation: (A) per-chunk gradient statistics, (B) the verdict -- the reference's walk over the tensors
 * (NaN before maximum, a maximum strictly above the threshold is "large", the first offender ends the walk), the total
 * norm and the clip coefficient of clip_grad_norm_, and every present tensor's step counter and bias corrections --,
 * (C) the AdamW update, which every block leaves after one read when the verdict is "skipped". */
#define SPF_OPTIM_CHUNK 4096      /* floats per chunk: every tensor is cut into chunks of this size, the last one partial */
#define SPF_OPTIM_MAX_GROUPS 8
typedef struct SpfOptimTensor {   /* one entry of the static table */
    float* param;
    float* exp_avg;
    float* exp_avg_sq;            /* numel floats each, 4-byte aligned (16-byte aligned bases take the vector path) */
    int64_t numel;
    int32_t group;                /* index into SpfOptimHyper.group */
    int32_t reserved;
} SpfOptimTensor;
typedef struct SpfOptimGroup {
    double lr, beta1, beta2, eps, weight_decay;
} SpfOptimGroup;
typedef struct SpfOptimHyper {    /* by value, every step: a scheduler changes lr without any copy */
    int32_t num_groups;           /* 1 .. SPF_OPTIM_MAX_GROUPS */
    int32_t guard;                /* 0: no NaN / large-gradient guard (non-finite gradients flow through, as in torch) */
    int32_t clip;                 /* 0: no clip (clip_coef = 1) */
    int32_t reserved;
    double max_grad_value;        /* guard threshold, compared as float32: max |g| > threshold is large */
    double max_norm;              /* clip_coef = min(1, max_norm / (total_norm + 1e-6)) */
    SpfOptimGroup group[SPF_OPTIM_MAX_GROUPS];
} SpfOptimHyper;
typedef struct SpfOptimReport {   /* 32 bytes on the device, written by every step */
    int32_t skipped, nan_detected, large_detected;
    int32_t offender;             /* position in the guard order, -1 if none */
    float max_gradient;           /* over the positions up to and including a large offender, excluding a NaN one */
    float total_norm;             /* sqrt of the sum of squares of all present gradients */
    float clip_coef;
    float clip_coef_lo;           /* the coefficient minus its float32 value: pass C multiplies by both parts */
} SpfOptimReport;
typedef struct SpfOptim {
    const SpfOptimTensor* table;  /* T entries */
    const int64_t* chunk_start;   /* T + 1: first chunk of every tensor, and the total (spf_optim_plan fills a host copy) */
    const uint64_t* grads;        /* T gradient addresses of this step, 0 = the tensor has no gradient */
    const int32_t* guard_order;   /* T: the tensor at every position of the guard's walk (a permutation of 0 .. T-1) */
    int32_t* step;                /* T step counters, the caller's persistent state; incremented for present tensors */
    void* scratch;                /* spf_optim_scratch_bytes(T, chunks) bytes, 16-byte aligned */
    void* report;                 /* one SpfOptimReport, 16-byte aligned */
    int32_t T, reserved;
    int64_t chunks;               /* chunk_start[T] */
} SpfOptim;
/* host only: chunks of one set, sum of ceil(numel[t] / SPF_OPTIM_CHUNK); -1 (SPF_E_INVALID) on a null array, T <= 0 or a
 * numel <= 0 */
int64_t spf_optim_chunks(const int64_t* numel /* host */, int32_t T);
/* host only: checks a HOST copy of the table (null table or pointer, T <= 0, numel <= 0, num_groups outside
 * 1 .. SPF_OPTIM_MAX_GROUPS, a group index out of range) and fills chunk_start[0 .. T] (host, may be null); returns the
 * number of chunks or SPF_E_INVALID */
int64_t spf_optim_plan(const SpfOptimTensor* table /* host */, int32_t T, int32_t num_groups,
                       int64_t* chunk_start /* host, T + 1 */);
int64_t spf_optim_scratch_bytes(int32_t T, int64_t chunks);
/* the three launches (pass A is left out when neither guard nor clip is set).  Argument errors return SPF_E_INVALID
 * before anything is launched; nothing is allocated or synchronised; no float atomics: bitwise repeatable. */
int spf_optim_step(const SpfOptim* args, const SpfOptimHyper* hyper, void* stream);

/* ---- the transformer block's row work (spfsplatv2_amd/csrc/block.hip) ------------------------------------------------
 * Residual add + LayerNorm and bias + exact GELU, forward and backward, float32 only, for rows of C floats with
 * C % 4 == 0 and 4 <= C <= 4096 (SPF_BLOCK_MAX_C).  Every pointer is 16-byte aligned and every stride a multiple of 4
 * floats (all accesses are 16-byte vectors).  Nothing is allocated or synchronised; no float atomics: the parameter
 * gradients are summed per block into `partials` and then by a reducer in a fixed order, bitwise reproducible.
 * Argument errors return SPF_E_INVALID (spf_last_error) before anything is launched. */
#define SPF_BLOCK_MAX_C 4096
typedef struct SpfBlockNorm {
    const float* x;               /* rows of C floats; row i starts at (i / x_inner) * x_outer_stride + (i % x_inner) * x_stride */
    const float* r;               /* optional second addend, addressed the same way through its own three numbers */
    const float* gamma;           /* optional [C], legal only with r: s = x + gamma * r (without it s = x + r) */
    const float* weight;          /* [C] */
    const float* bias;            /* [C]; not read by the backward */
    int64_t x_inner, x_stride, x_outer_stride;   /* x_inner >= 1 rows per outer group; a dense [rows, C]: rows, C, 0 */
    int64_t r_inner, r_stride, r_outer_stride;
    int64_t rows;                 /* 1 .. 2^30 */
    int32_t C;
    float eps;
} SpfBlockNorm;
/* host only: the number of blocks that write one row of partial column sums each, of the norm backward (gelu = 0) or
 * of the GELU backward (gelu = 1) on `rows` rows of C floats; SPF_E_INVALID on sizes out of range */
int64_t spf_block_partial_blocks(int64_t rows, int32_t C, int32_t gelu);
/* s [rows, C] (written only with r; may be null without), y [rows, C], stats [rows, 4]: per row of s the mean as two
 * floats (a float32 mean and the mean of the deviations about it, i.e. what float32 dropped), 1 / sqrt(var + eps) and a
 * pad; the biased variance is taken from the deviations about that two-part mean, its sum in float64 */
int spf_block_add_norm_forward(const SpfBlockNorm* args, float* s, float* y, float* stats, void* stream);
/* args->x: the saved s (the forward's x where it had no r); args->r and gamma: given only where the forward had a
 * gamma.  dy [rows, C]; ds [rows, C] or null; dx [rows, C] = ds + LN'(dy); dr [rows, C] = gamma * dx (only with gamma:
 * without it dr IS dx and the pointer must be null).  partials: K * spf_block_partial_blocks(rows, C, 0) * C floats,
 * dparams: [K, C] = dweight, dbias[, dgamma], K = 2 without gamma, 3 with. */
int spf_block_add_norm_backward(const SpfBlockNorm* args, const float* dy, const float* ds, const float* stats, float* dx,
                                float* dr, float* partials, float* dparams, void* stream);
/* h = GELU(u + bias), erf form; u, h [rows, C] dense, bias [C] or null */
int spf_block_bias_gelu_forward(const float* u, const float* bias, int64_t rows, int32_t C, float* h, void* stream);
/* du = dh * GELU'(u + bias); with a bias, dbias [C] = the column sums of du through partials
 * (spf_block_partial_blocks(rows, C, 1) * C floats); without, both must be null */
int spf_block_bias_gelu_backward(const float* u, const float* bias, const float* dh, int64_t rows, int32_t C, float* du,
                                 float* partials, float* dbias, void* stream);

/* ---- the DPT heads' work between their convolutions (spfsplatv2_amd/csrc/dpt.hip) -------------------------------------
 * x2 bilinear upsample (+ skip), add + ReLU and the point-map postprocess, forward and backward, float32 only, NCHW
 * contiguous.  Every pointer is 16-byte aligned; every tensor of a call holds fewer than 2^31 elements.  Nothing is
 * allocated or synchronised; no float atomics: bitwise reproducible.  Argument errors return SPF_E_INVALID
 * (spf_last_error) before anything is launched. */
#define SPF_DPT_MAX_SIDE 16384
/* host only: the most blocks any of these launches uses; the rest of the work is taken grid-stride (an upsample block
 * takes 4,096 items of one plane per round, so a plane of up to 4,096 input pixels is one unit) */
int32_t spf_dpt_max_grid(void);
/* out [planes, 2h, 2w] = up2(x [planes, h, w]) + (skip | relu(skip) with relu_skip) [planes, 2h, 2w] (skip may be null).
 * up2 is torch's bilinear rule with align_corners=True: scale = (in - 1) / (2 in - 1) in float32 (0 for in = 1),
 * src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), lambda1 = src - i0. */
int spf_dpt_upsample2x_forward(const float* x, const float* skip, int32_t relu_skip, int64_t planes, int32_t h, int32_t w,
                               float* out, void* stream);
/* dx [planes, h, w] = up2^T(dy), gathered per input pixel in a fixed order.  With the forward's ReLU flag: skip (the
 * forward's) and dskip = dy * (skip > 0); without it both are null, because dskip IS dy.  dx may be null where dskip is
 * written: the gather is then not run. */
int spf_dpt_upsample2x_backward(const float* dy, const float* skip, int64_t planes, int32_t h, int32_t w, float* dx,
                                float* dskip, void* stream);
/* s = a + b (+ c), y = relu(s), n floats each; b, c optional (c only with b).  With a alone s must be null (s is a). */
int spf_dpt_add_relu_forward(const float* a, const float* b, const float* c, int64_t n, float* s, float* y, void* stream);
/* g = ds + dy * (mask > 0): the gradient of every addend; mask: the forward's s or y (the same sign), ds optional */
int spf_dpt_add_relu_backward(const float* mask, const float* dy, const float* ds, int64_t n, float* g, void* stream);
typedef struct SpfDptPoints {
    const float* in;              /* [B, C, HW]: channels 0..2 xyz, channel 3 the confidence logit (has_conf) */
    int64_t B, HW;
    int32_t C, has_conf;
    float depth_min, depth_max;   /* bounds of expm1(d); -inf, +inf: none */
    float conf_min, conf_max;     /* conf = conf_min + min(exp(x), conf_max - conf_min) */
} SpfDptPoints;
/* pts3d [B, HW, 3] = xyz / max(d, 1e-8) * clip(expm1(d), depth_min, depth_max), d = |xyz|; conf [B, HW] (with has_conf
 * and only then) */
int spf_dpt_points_forward(const SpfDptPoints* args, float* pts3d, float* conf, void* stream);
/* din [B, C, HW]: channels 0..2 (and 3 with has_conf) are written, what autograd gives for the expression above (d = 0:
 * zero through the norm; d < 1e-8: nothing through the clip); further channels are left to the caller */
int spf_dpt_points_backward(const SpfDptPoints* args, const float* dpts3d, const float* dconf, float* din, void* stream);

/* ---- the encoder tail (spfsplatv2_amd/csrc/tail.hip) ------------------------------------------------------------------
 * The heads' outputs, where they lie, -> the decoder's Gaussians (encoder_spfsplatv2.py:218-224, 240, 248-268, 296-321):
 * per view vi the gs_params head's raw[vi] [b, C = 1 + 7 + 3K, hw] (channel-major, dense) and the point head's pts[vi]
 * [b, hw, 3]; Gaussian n = vi hw + p of batch item bi is pixel p of view vi.  Per Gaussian, x = raw channels of a pixel:
 *   means = pts;  opacities = 0.5 (1 - (1 - p)^e + p^(1/e)), p = sigmoid(x[0]), e = exponent (map_pdf_to_opacity);
 *   scales = min(0.001 softplus(x[1:4]), 0.3);  rotations = x[4:8] / (|x[4:8]| + eps);
 *   harmonics[c][k] = x[8 + c K + k] sh_mask[k].
 * K is one of 1, 4, 9, 16, 25 (sh_degree 0..4); any other K is SPF_E_INVALID.  float32 only; every pointer is 16-byte
 * aligned; b hw C and b v hw 3 K stay below 2^31.  One launch per direction; nothing is allocated or synchronised; no
 * atomics: bitwise reproducible.  Argument errors return SPF_E_INVALID (spf_last_error) before anything is launched. */
#define SPF_TAIL_MAX_VIEWS 32
typedef struct SpfTail {
    const float* raw[SPF_TAIL_MAX_VIEWS];   /* the first v entries: [b, 8 + 3K, hw] each */
    const float* pts[SPF_TAIL_MAX_VIEWS];   /* the first v entries: [b, hw, 3] each (backward: not read, may be NULL) */
    const float* sh_mask;                   /* [K] */
    int64_t hw;
    int32_t b, v, K;
    float exponent, eps;
    int32_t reserved;
} SpfTail;
typedef struct SpfTailGrads {
    float* d_raw[SPF_TAIL_MAX_VIEWS];       /* the first v entries: [b, 8 + 3K, hw] each, EVERY element is written */
    float* d_pts[SPF_TAIL_MAX_VIEWS];       /* the first v entries: [b, hw, 3] each, every element is written */
} SpfTailGrads;
/* host only: the most blocks a launch of tail.hip uses; a block takes 64-pixel tiles of one (batch item, view),
 * further tiles grid-stride */
int32_t spf_tail_max_grid(void);
/* means [b, v hw, 3], opacities [b, v hw], scales [b, v hw, 3], rotations [b, v hw, 4], harmonics [b, v hw, 3, K]; with
 * harmonics_high != NULL (K = 25 only) the band split: harmonics [.., 3, 16] and harmonics_high [.., 3, 9]
 * (SpfDims.sh_layout 2) */
int spf_tail_forward(const SpfTail* args, float* means, float* opacities, float* scales, float* rotations,
                     float* harmonics, float* harmonics_high, void* stream);
/* Any upstream gradient may be NULL = zero (never read).  `split`: dL_dharmonics is [.., 3, 16] and band 4's gradient
 * is dL_dharmonics_high [.., 3, 9], or NULL: those channels of d_raw are written as zeros.  The density channel's
 * derivative is taken in logit form, 0.5 (e (1 - p)^e p + (1/e) p^(1/e) (1 - p)) with 1 - p = sigmoid(-x): finite for
 * every finite logit. */
int spf_tail_backward(const SpfTail* args, const float* dL_dmeans, const float* dL_dopacities, const float* dL_dscales,
                      const float* dL_drotations, const float* dL_dharmonics, const float* dL_dharmonics_high,
                      int32_t split, const SpfTailGrads* grads, void* stream);
/* The opacity map alone, for a head output that is already in rows (encoder_spfsplatv2l.py:176,184):
 * opacities[i] = map(logits[i * stride]), i < n (stride >= 1 in floats: channel 0 of a [.., 83] tensor read in place),
 * and dL_dlogits[i] = dL_dopacities[i] * map'(logits[i * stride]) (both contiguous).  4-byte alignment suffices. */
int spf_opacity_forward(const float* logits, int64_t stride, int64_t n, float exponent, float* opacities, void* stream);
int spf_opacity_backward(const float* logits, int64_t stride, int64_t n, float exponent, const float* dL_dopacities,
                         float* dL_dlogits, void* stream);

/* ---- the pose heads between their GEMMs (spfsplatv2_amd/csrc/posehead.hip) ---------------------------------------------
 * The MLP PoseHead (heads/pose_head.py) and VGGT's CameraHead (vggt/heads/camera_head.py): token pooling, the head's
 * tail, embed + SiLU, the adaptive LayerNorm, attention over the views and activate_pose, forward and backward.  float32
 * only; every pointer of the pool, modulate and attention calls is 16-byte aligned, the others 4-byte.  Nothing is
 * allocated or synchronised; no atomics: every sum has one order, two runs agree bitwise.  Argument errors return
 * SPF_E_INVALID (spf_last_error) before anything is launched. */
#define SPF_POSEHEAD_MAX_S 32
#define SPF_POSEHEAD_MAX_ROWS 65535
enum { SPF_POSE_ACT_LINEAR = 0, SPF_POSE_ACT_INV_LOG = 1, SPF_POSE_ACT_EXP = 2, SPF_POSE_ACT_RELU = 3 };
typedef struct SpfPosePool {
    const float* src[2];          /* source s: [rows, L, C[s]] with unit channel stride; src[1] NULL: one source.  The
                                   * backward reads no source: both may be NULL there */
    int64_t inner[2], stride[2], outer_stride[2];   /* row i of source s starts at (i / inner) * outer_stride +
                                                     * (i % inner) * stride (floats, multiples of 4; inner >= 1) */
    int64_t tok_stride[2];        /* floats between two tokens of a row, a multiple of 4 */
    int32_t C[2];                 /* multiples of 4, 4 .. 2^20; C[1] is ignored without a second source */
    int64_t rows;                 /* 1 .. SPF_POSEHEAD_MAX_ROWS */
    int32_t L;                    /* tokens per row, 1 .. 2^20; L = 1 copies */
    int32_t reserved;
} SpfPosePool;
/* feat [rows, C[0] + C[1]] dense: the mean over the L tokens, source 0's channels first */
int spf_posehead_pool_forward(const SpfPosePool* args, float* feat, void* stream);
/* d_src0 [rows, L, C[0]], d_src1 [rows, L, C[1]] dense (d_src1 with a second source and only then; whether there is one
 * is read from d_src1 here): d_feat / L at every token */
int spf_posehead_pool_backward(const SpfPosePool* args, const float* d_feat, float* d_src0, float* d_src1, void* stream);
typedef struct SpfPoseEncode {
    int64_t rows;                 /* 1 .. 2^24 */
    int64_t out_inner, out_stride, out_outer_stride;   /* pose row i starts at (i / out_inner) * out_outer_stride +
                                                        * (i % out_inner) * out_stride: views 1.. of a [b, v, 9] tensor */
    int32_t homogeneous;          /* t is [rows, 4] and out[6:9] = t[:3] / h, h = min(softplus(t[3], beta) +
                                   * max_inv_scale, min_inv_scale); else t is [rows, 3], copied */
    float beta, max_inv_scale, min_inv_scale;
} SpfPoseEncode;
/* rot [rows, 6] and t dense; out: the 9-float pose rows (rot, then the translation), addressed as above.  softplus is
 * torch's: x where beta x > 20. */
int spf_posehead_encode_forward(const SpfPoseEncode* args, const float* rot, const float* t, float* out, void* stream);
/* d_out addressed as out was; d_rot [rows, 6], d_t [rows, 3 or 4] dense.  Nothing flows through a clamped h. */
int spf_posehead_encode_backward(const SpfPoseEncode* args, const float* t, const float* d_out, float* d_rot, float* d_t,
                                 void* stream);
/* out [rows, C] = SiLU(p W^T + b): p [rows, 9] dense, or with `broadcast` ONE row of 9 floats used for every row;
 * W [C, 9], b [C]; rows 1 .. SPF_POSEHEAD_MAX_ROWS, C 1 .. 2^20 */
int spf_posehead_embed_silu_forward(const float* p, int32_t broadcast, const float* W, const float* b, int64_t rows,
                                    int32_t C, float* out, void* stream);
/* The pre-activation is recomputed.  dW [C, 9], db [C] (both always written: a thread per column sums down the rows);
 * dp: NULL, or [rows, 9] -- with `broadcast` [9], summed over the rows too. */
int spf_posehead_embed_silu_backward(const float* p, int32_t broadcast, const float* W, const float* b, const float* dout,
                                     int64_t rows, int32_t C, float* dW, float* db, float* dp, void* stream);
/* out [rows, C] = gate * (LN(x) * (1 + scale) + shift) + x with mod [rows, 3 C] = shift | scale | gate (the column
 * thirds), LN without parameters, the biased variance from the centred values; C as SpfBlockNorm's, rows 1 .. 2^30 */
int spf_posehead_modulate_forward(const float* x, const float* mod, int64_t rows, int32_t C, float eps, float* out,
                                  void* stream);
/* dx [rows, C] and dmod [rows, 3 C] in mod's layout (every element written); the row statistics are recomputed */
int spf_posehead_modulate_backward(const float* x, const float* mod, const float* dout, int64_t rows, int32_t C, float eps,
                                   float* dx, float* dmod, void* stream);
/* out [B, S, H D] = softmax(q k^T / sqrt(D)) v per (batch item, head) of the packed qkv [B, S, 3, H, D]; D is 64 or 128,
 * 1 <= S <= SPF_POSEHEAD_MAX_S, B H < 2^31 / 3.  No rotation, no mask, no q / k norm. */
int spf_posehead_attn_forward(const float* qkv, int32_t B, int32_t S, int32_t H, int32_t D, float* out, void* stream);
/* dqkv [B, S, 3, H, D], every element written; the probabilities are recomputed */
int spf_posehead_attn_backward(const float* qkv, const float* dout, int32_t B, int32_t S, int32_t H, int32_t D,
                               float* dqkv, void* stream);
/* pred [rows, 9] = prev + delta (prev NULL: delta), out [rows, 9] = the SPF_POSE_ACT_* of columns 0:3 (trans_act),
 * 3:7 (quat_act), 7:9 (fl_act) of pred; rows 1 .. 2^24 */
int spf_posehead_activate_forward(const float* prev, const float* delta, int64_t rows, int32_t trans_act, int32_t quat_act,
                                  int32_t fl_act, float* pred, float* out, void* stream);
/* d_delta = d_pred + d_out * act'(pred); d_pred or d_out may be NULL (zero), not both */
int spf_posehead_activate_backward(const float* pred, const float* d_pred, const float* d_out, int64_t rows,
                                   int32_t trans_act, int32_t quat_act, int32_t fl_act, float* d_delta, void* stream);

/* ---- the encoder front (spfsplatv2_amd/csrc/front.hip) ------------------------------------------------------------------
 * Image -> tokens: the patch embedding (`nn.Conv2d(C_in, C, P, P)`, `flatten(2).transpose(1, 2)`) as an implicit GEMM on
 * the float32 matrix instruction, the token rows around the patch rows, and the gradients to every parameter.  float32
 * only; nothing is allocated or synchronised; no atomics: every sum has one order, two runs agree bitwise.  Argument
 * errors return SPF_E_INVALID (spf_last_error) before anything is launched. */
#define SPF_FRONT_MAX_TOKENS 16
typedef struct SpfFront {
    const float* image;           /* [B, C_in, gh P, gw P]: unit stride along a row; the base 16-byte aligned for P = 16,
                                   * 8-byte aligned for P = 14 */
    const float* affine;          /* NULL, or [2, C_in]: channel c is read as image * affine[c] + affine[C_in + c] */
    int64_t stride_b, stride_c, stride_y;   /* floats between images, channels and rows: multiples of 4 (P = 16) or 2 */
    int32_t B, C_in;              /* B gh gw < 2^31; 1 <= C_in <= 32 */
    int32_t gh, gw;               /* the patch grid */
    int32_t P;                    /* 14 or 16 */
    int32_t C;                    /* embed_dim, a multiple of 4 */
    int32_t before, after;        /* token rows in front of / behind the patch rows of an image of `out` / `dY` */
} SpfFront;
typedef struct SpfFrontTokens {
    const float* tok[SPF_FRONT_MAX_TOKENS];     /* the tensors in front (n_before of them), then those behind: [1, rows, C]
                                                 * or [S, rows, C], dense, 16-byte aligned.  In the backward call: the
                                                 * DESTINATION of a broadcast tensor's gradient, NULL where none is wanted */
    int32_t rows[SPF_FRONT_MAX_TOKENS];         /* >= 1 */
    int32_t per_image[SPF_FRONT_MAX_TOKENS];    /* 1: [S, rows, C]; 0: broadcast over the sequences */
    int32_t n_before, n_after;                  /* tensors */
    int32_t before, after;                      /* rows: the sums of `rows` */
    const float* pos_first;                     /* NULL, or [C]: added to row 0 (which must be an extra row) */
} SpfFrontTokens;
enum { SPF_FRONT_TILE_ROWS = 0, SPF_FRONT_TILE_COLS = 1, SPF_FRONT_CHUNK_ROWS = 2, SPF_FRONT_CHUNKS = 3 };
/* host only: the rows (patches) and columns (channels) of a block's tile, and for M patch rows the height of a chunk of
 * the weight gradient and the number of chunks; -1 for another `what` */
int64_t spf_front_geometry(int32_t what, int64_t M);
/* host only: floats of the backward's workspace (with_dweight: the chunks' partials of dW; then one [gh gw, C] sum), or
 * -1 */
int64_t spf_front_workspace_floats(const SpfFront* args, int32_t with_dweight);
/* out [B, before + gh gw + after, C] dense: row before + n of image b = bias + weight . patch n (+ pos_table[n]).
 * weight [C, C_in P P] dense (`proj.weight` in place); bias [C] or NULL; pos_table [gh gw, C] or NULL.  Only the patch
 * rows are written. */
int spf_front_embed_forward(const SpfFront* args, const float* weight, const float* bias, const float* pos_table, float* out,
                            void* stream);
/* out [S, before + N + after, C] dense.  The extra rows from `tokens`; with `body` (N rows per sequence, row i of all S N
 * at (i / inner) * outer_stride + (i % inner) * stride floats, multiples of 4) the body's rows too, else they are left
 * alone.  N >= 0, C a multiple of 4. */
int spf_front_assemble(const SpfFrontTokens* tokens, const float* body, int64_t inner, int64_t stride, int64_t outer_stride,
                       int64_t S, int32_t N, int32_t C, float* out, void* stream);
/* dY: sequence s, row r at s * dy_stride_s + r * dy_stride_r (multiples of 4), unit stride along C.  Writes, for every
 * broadcast tensor with a destination, the sum over s (ascending) of its rows; d_pos_first [C] (or NULL) likewise from
 * row 0. */
int spf_front_tokens_backward(const SpfFrontTokens* tokens, const float* dY, int64_t dy_stride_s, int64_t dy_stride_r,
                              int64_t S, int32_t N, int32_t C, float* d_pos_first, void* stream);
/* dweight [C, C_in P P], dbias [C], dpos_table [gh gw, C]: each NULL or written whole.  dY is read at its placed rows
 * (image b, row before + n).  workspace: spf_front_workspace_floats(args, dweight != NULL) floats, 16-byte aligned. */
int spf_front_embed_backward(const SpfFront* args, const float* dY, int64_t dy_stride_b, int64_t dy_stride_r,
                             float* workspace, float* dweight, float* dbias, float* dpos_table, void* stream);

/* ---- PnP pose from point maps (csrc/pnp.hip): P3P RANSAC and Gauss-Newton refinement, all b v views of a
 * call in four launches.  Pixel (row i, column j) of view (bi, vi) is the image point (x, y) = (j, i); its three
 * contiguous floats are at pts3d + bi pts_stride[0] + vi pts_stride[1] + i pts_stride[2] + j pts_stride[3] (floats), its
 * opacity likewise through opa_stride.  K: [b v, 3, 3] dense, normalised (row 0 is multiplied by w, row 1 by h). */
typedef struct SpfPnp {
    const float* pts3d;
    const float* opacity;
    const float* K;
    int64_t pts_stride[4];
    int64_t opa_stride[4];
    int32_t b, v, h, w;
    int32_t iterations;          /* a multiple of 64 in 64..1024 */
    int32_t refine_steps;        /* 0..64 */
    uint32_t seed;
    float opacity_threshold;     /* candidates: opacity > threshold, finite coordinates */
    float reprojection_error;    /* pixels */
    int32_t reserved;
} SpfPnp;
/* host only: bytes of the workspace for `views` views of h x w pixels, or -1 for sizes spf_pnp_solve refuses */
int64_t spf_pnp_workspace_bytes(int32_t views, int32_t h, int32_t w, int32_t iterations);
/* poses [b v, 4, 4]: camera -> world, or the identity for a view that fails.  info [4, b v] int32: final inliers,
 * candidates n, winning hypothesis (-1 on failure), success.  ranks: NULL, or [b v, iterations, 4] int32, the sample
 * ranks of every hypothesis (-1: not drawn).  workspace: 16-byte aligned, needs no clearing. */
int spf_pnp_solve(const SpfPnp* args, void* workspace, float* poses, int32_t* info, int32_t* ranks, void* stream);

/* Per-stage device timing with HIP events recorded on the launch stream around every kernel
 * stage.  spf_stage_timing_enable(mask) clears the log and starts recording the stages whose bit
 * (1 << SPF_STAGE_x) is set in `mask` (0 = off, -1 = all) (up to
 * SPF_STAGE_LOG launches per stage are kept); spf_stage_times_ms synchronises on the recorded
 * events and returns, per stage, the summed device time and the number of launches logged since
 * enable -- average launch duration = total_ms[i] / count[i]. */
enum {
    SPF_STAGE_PROJECT = 0,   /* forward per-Gaussian kernel */
    SPF_STAGE_SCAN = 1,
    SPF_STAGE_BIN = 2,
    SPF_STAGE_SORT = 3,
    SPF_STAGE_RENDER_FWD = 4,
    SPF_STAGE_RENDER_BWD = 5,
    SPF_STAGE_PROJECT_BWD = 6,
    SPF_STAGE_ROPE = 7,
    SPF_STAGE_COUNT = 8
};
#define SPF_STAGE_LOG 1024
int spf_stage_timing_enable(int32_t mask);
/* Record only every n-th launch of an enabled stage (default 1): an event pair leaves the GPU idle for ~11 us. */
int spf_stage_timing_sample_every(int32_t n);
int spf_stage_times_ms(float* total_ms /* host, [SPF_STAGE_COUNT] */,
                       int32_t* count /* host, [SPF_STAGE_COUNT] */);
const char* spf_stage_kernel_name(int32_t stage);

#ifdef __cplusplus
}
#endif
#endif /* SPFSPLAT_HIP_H */
