// The encoder tail for gfx950: the DPT heads' outputs, where they lie, -> the decoder's Gaussians, forward and backward
// (encoder_spfsplatv2.py:218-224, 240, 248-268, 296-321 of the reference: rearrange "b d h w -> b (h w) d", torch.stack
// over the views, sigmoid, map_pdf_to_opacity, UnifiedGaussianAdapter.forward and the final rearranges).
//   raw  : per view [b, C = 1 + 7 + 3K, hw]   channel-major, as the gs_params head writes it
//   pts  : per view [b, hw, 3]                as the point head's postprocess writes it
//   out  : means [b, v hw, 3], opacities [b, v hw], scales [b, v hw, 3], rotations [b, v hw, 4],
//          harmonics [b, v hw, 3, K] (or band-split [.., 3, 16] + [.., 3, 9], K = 25)
// ONE pass per direction.  A block takes a tile of kTailPix = 64 pixels of one (batch item, view).  Lanes run along the
// pixels: every plane read (forward) or plane write (backward) is a full coalesced line, 16 bytes per lane where
// hw % 4 == 0 (a tile then starts 16-byte aligned), one float per lane otherwise.  The tile is transposed through LDS
// as rows [pixel][channel] with an odd row stride, so the outputs whose unit stride is the channel (harmonics, scales,
// rotations; in backward their gradients) leave or arrive as flat coalesced accesses too.  64 x 83 floats = 21 KB per
// block (K = 25): seven blocks per CU.  No atomics, nothing allocated, no host sync; every output byte is written once.
#include "adapter_math.h"
#include "launchers.h"

namespace spf {

constexpr int kTailPix = 64;            // pixels per tile
constexpr int kTailMaxGrid = 4096;      // blocks of a launch; further tiles are taken grid-stride
constexpr int kTailLow = 16, kTailHigh = 9;
// The harmonics loops (19 trips of 256 floats at K = 25) are unrolled by two.  Unrolled in full the compiler keeps every
// trip's address and value live: 166 VGPRs, three blocks per CU, and the step "forward + backward" at b = 16, v = 2,
// 256 x 256 took 1.31 ms (band-split) / 1.46 ms (dense); by 8: 95 VGPRs, 0.95 / 0.99 ms; by 2: 66 VGPRs, the seven
// blocks per CU the LDS allows, 0.83 / 0.85 ms (variant builds, same device, two passes each).

int tail_max_grid() { return kTailMaxGrid; }

struct TailTile {
    int64_t bi, n0;          // batch item; first Gaussian of the tile in the stacked outputs: (bi v + vi) hw + p0
    int64_t p0;              // first pixel
    int vi, npix;
};
__device__ __forceinline__ TailTile tail_tile(int64_t t, int64_t tiles_per, int v, int64_t hw) {
    TailTile o;
    const int64_t bv = t / tiles_per;
    o.p0 = (t - bv * tiles_per) * kTailPix;
    o.bi = bv / v;
    o.vi = (int)(bv - o.bi * v);
    o.n0 = bv * hw + o.p0;
    o.npix = (int)min((int64_t)kTailPix, hw - o.p0);
    return o;
}

// ---- forward ------------------------------------------------------------------------------------------------------
template <int K, bool VEC>
__global__ __launch_bounds__(kBlock) void spf_tail_fwd_kernel(SpfTail a, int64_t tiles_per, int64_t ntiles, float inv_e,
                                                             float* __restrict__ means, float* __restrict__ opac,
                                                             float* __restrict__ scales, float* __restrict__ rot,
                                                             float* __restrict__ sh, float* __restrict__ sh_hi) {
    constexpr int C = 8 + 3 * K, CS = C | 1;
    __shared__ float s[kTailPix * CS];
    __shared__ float s_mask[K];
    const int tid = threadIdx.x;
    const int64_t hw = a.hw;
    if (tid < K) s_mask[tid] = a.sh_mask[tid];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TailTile tl = tail_tile(t, tiles_per, a.v, hw);
        const int npix = tl.npix;
        const float* __restrict__ raw = a.raw[tl.vi] + (tl.bi * C) * hw + tl.p0;
        float m = 0.f;
        if (tid < npix * 3) m = a.pts[tl.vi][(tl.bi * hw + tl.p0) * 3 + tid];
        __syncthreads();                                                // (the previous tile's rows have been read)
        if (VEC) {
            const int q = tid & 15;
            if (4 * q < npix) {
#pragma unroll
                for (int i = 0; i < (C + 15) / 16; ++i) {
                    const int c = (tid >> 4) + 16 * i;
                    if (c >= C) break;
                    const float4 x = *reinterpret_cast<const float4*>(raw + c * hw + 4 * q);
                    s[(4 * q + 0) * CS + c] = x.x;
                    s[(4 * q + 1) * CS + c] = x.y;
                    s[(4 * q + 2) * CS + c] = x.z;
                    s[(4 * q + 3) * CS + c] = x.w;
                }
            }
        } else {
            const int p = tid & 63;
            if (p < npix) {
#pragma unroll
                for (int i = 0; i < (C + 3) / 4; ++i) {
                    const int c = (tid >> 6) + 4 * i;
                    if (c < C) s[p * CS + c] = raw[c * hw + p];
                }
            }
        }
        __syncthreads();
        // ---- geometry: one output float per lane ----
        if (tid < npix * 3) {
            const int r = tid / 3, k = tid - 3 * r;
            means[tl.n0 * 3 + tid] = m;
            scales[tl.n0 * 3 + tid] = adapter_scale(s[r * CS + 1 + k]);
        }
        if (tid < npix * 4) {
            const float* __restrict__ q = s + (tid >> 2) * CS + 4;
            rot[tl.n0 * 4 + tid] = q[tid & 3] * quat_inv_norm(q[0], q[1], q[2], q[3], a.eps);
        }
        if (tid < npix) opac[tl.n0 + tid] = opacity_map(s[tid * CS], a.exponent, inv_e);
        // ---- harmonics: flat planes ----
        if (K == 25 && sh_hi) {
            float* __restrict__ lo = sh + tl.n0 * 3 * kTailLow;
#pragma unroll 2
            for (int i = 0; i < kTailPix * 3 * kTailLow / kBlock; ++i) {
                const int e = tid + kBlock * i;
                const int p = e / (3 * kTailLow), rem = e - p * 3 * kTailLow, c = rem / kTailLow, k = rem - c * kTailLow;
                if (p < npix) lo[e] = s[p * CS + 8 + c * K + k] * s_mask[k];
            }
            float* __restrict__ hi = sh_hi + tl.n0 * 3 * kTailHigh;
#pragma unroll 2
            for (int i = 0; i < (kTailPix * 3 * kTailHigh + kBlock - 1) / kBlock; ++i) {
                const int e = tid + kBlock * i;
                const int p = e / (3 * kTailHigh), rem = e - p * 3 * kTailHigh, c = rem / kTailHigh;
                const int k = kTailLow + rem - c * kTailHigh;
                if (p < npix) hi[e] = s[p * CS + 8 + c * K + k] * s_mask[k];
            }
        } else {
            float* __restrict__ o = sh + tl.n0 * 3 * K;
#pragma unroll 2
            for (int i = 0; i < (kTailPix * 3 * K + kBlock - 1) / kBlock; ++i) {
                const int e = tid + kBlock * i;
                const int p = e / (3 * K), rem = e - p * 3 * K;
                if (p < npix) o[e] = s[p * CS + 8 + rem] * s_mask[rem % K];
            }
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// dL/draw of every view in that view's own [b, C, hw] layout, all C channels, and dL/dpts per view [b, hw, 3].  The
// harmonics' gradients arrive flat and are scaled into the tile's rows; lanes 0..63 chain the density and the scales of
// one pixel each, lanes 64..127 the quaternion; then the rows leave as planes.  A NULL upstream gradient is zero and is
// never read (`split` with g_sh_hi NULL: band 4's channels are written as zeros).
template <int K, bool VEC>
__global__ __launch_bounds__(kBlock) void spf_tail_bwd_kernel(SpfTail a, SpfTailGrads out, int64_t tiles_per,
                                                             int64_t ntiles, float inv_e,
                                                             const float* __restrict__ g_means,
                                                             const float* __restrict__ g_opac,
                                                             const float* __restrict__ g_scales,
                                                             const float* __restrict__ g_rot,
                                                             const float* __restrict__ g_sh,
                                                             const float* __restrict__ g_sh_hi, int split) {
    constexpr int C = 8 + 3 * K, CS = C | 1;
    __shared__ float s[kTailPix * CS];
    __shared__ float s_mask[K];
    const int tid = threadIdx.x;
    const int64_t hw = a.hw;
    if (tid < K) s_mask[tid] = a.sh_mask[tid];
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const TailTile tl = tail_tile(t, tiles_per, a.v, hw);
        const int npix = tl.npix;
        const float* __restrict__ raw = a.raw[tl.vi] + (tl.bi * C) * hw + tl.p0;
        if (tid < npix * 3) out.d_pts[tl.vi][(tl.bi * hw + tl.p0) * 3 + tid] = g_means ? g_means[tl.n0 * 3 + tid] : 0.f;
        __syncthreads();                                                // (the previous tile's rows have left; the mask)
        // ---- harmonics into the rows ----
        if (K == 25 && split) {
#pragma unroll 2
            for (int i = 0; i < kTailPix * 3 * kTailLow / kBlock; ++i) {
                const int e = tid + kBlock * i;
                const int p = e / (3 * kTailLow), rem = e - p * 3 * kTailLow, c = rem / kTailLow, k = rem - c * kTailLow;
                if (p < npix) s[p * CS + 8 + c * K + k] = g_sh ? g_sh[tl.n0 * 3 * kTailLow + e] * s_mask[k] : 0.f;
            }
#pragma unroll 2
            for (int i = 0; i < (kTailPix * 3 * kTailHigh + kBlock - 1) / kBlock; ++i) {
                const int e = tid + kBlock * i;
                const int p = e / (3 * kTailHigh), rem = e - p * 3 * kTailHigh, c = rem / kTailHigh;
                const int k = kTailLow + rem - c * kTailHigh;
                if (p < npix) s[p * CS + 8 + c * K + k] = g_sh_hi ? g_sh_hi[tl.n0 * 3 * kTailHigh + e] * s_mask[k] : 0.f;
            }
        } else {
#pragma unroll 2
            for (int i = 0; i < (kTailPix * 3 * K + kBlock - 1) / kBlock; ++i) {
                const int e = tid + kBlock * i;
                const int p = e / (3 * K), rem = e - p * 3 * K;
                if (p < npix) s[p * CS + 8 + rem] = g_sh ? g_sh[tl.n0 * 3 * K + e] * s_mask[rem % K] : 0.f;
            }
        }
        // ---- geometry: one pixel per lane, the raw channels read along the pixels ----
        if (tid < kTailPix) {
            if (tid < npix) {
                float* __restrict__ o = s + tid * CS;
                const int64_t n = tl.n0 + tid;
                o[0] = g_opac ? g_opac[n] * opacity_map_grad(raw[tid], a.exponent, inv_e) : 0.f;
#pragma unroll
                for (int i = 0; i < 3; ++i) o[1 + i] = g_scales ? adapter_scale_grad(raw[(1 + i) * hw + tid], g_scales[n * 3 + i]) : 0.f;
            }
        } else if (tid < 2 * kTailPix) {
            const int p = tid - kTailPix;
            if (p < npix) {
                float* __restrict__ o = s + p * CS + 4;
                if (g_rot) {
                    const float4 gv = *reinterpret_cast<const float4*>(g_rot + (tl.n0 + p) * 4);
                    const float q[4] = {raw[4 * hw + p], raw[5 * hw + p], raw[6 * hw + p], raw[7 * hw + p]};
                    const float g[4] = {gv.x, gv.y, gv.z, gv.w};
                    float d[4];
                    quat_normalise_grad(q, g, a.eps, d);
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = d[i];
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) o[i] = 0.f;
                }
            }
        }
        __syncthreads();
        // ---- the rows leave as planes ----
        float* __restrict__ dst = out.d_raw[tl.vi] + (tl.bi * C) * hw + tl.p0;
        if (VEC) {
            const int q = tid & 15;
            if (4 * q < npix) {
#pragma unroll
                for (int i = 0; i < (C + 15) / 16; ++i) {
                    const int c = (tid >> 4) + 16 * i;
                    if (c >= C) break;
                    float4 x;
                    x.x = s[(4 * q + 0) * CS + c];
                    x.y = s[(4 * q + 1) * CS + c];
                    x.z = s[(4 * q + 2) * CS + c];
                    x.w = s[(4 * q + 3) * CS + c];
                    *reinterpret_cast<float4*>(dst + c * hw + 4 * q) = x;
                }
            }
        } else {
            const int p = tid & 63;
            if (p < npix) {
#pragma unroll
                for (int i = 0; i < (C + 3) / 4; ++i) {
                    const int c = (tid >> 6) + 4 * i;
                    if (c < C) dst[c * hw + p] = s[p * CS + c];
                }
            }
        }
    }
}

static unsigned tail_grid(int64_t ntiles) { return (unsigned)(ntiles < kTailMaxGrid ? (ntiles < 1 ? 1 : ntiles) : kTailMaxGrid); }

#define SPF_TAIL_K(FN, ...)                                              \
    switch (a.K) {                                                       \
        case 25: if (vec) FN<25, true> __VA_ARGS__; else FN<25, false> __VA_ARGS__; break; \
        case 16: if (vec) FN<16, true> __VA_ARGS__; else FN<16, false> __VA_ARGS__; break; \
        case 9: if (vec) FN<9, true> __VA_ARGS__; else FN<9, false> __VA_ARGS__; break;    \
        case 4: if (vec) FN<4, true> __VA_ARGS__; else FN<4, false> __VA_ARGS__; break;    \
        case 1: if (vec) FN<1, true> __VA_ARGS__; else FN<1, false> __VA_ARGS__; break;    \
        default: return hipErrorInvalidValue;                            \
    }

hipError_t launch_tail_fwd(const SpfTail& a, float* means, float* opac, float* scales, float* rot, float* sh, float* sh_hi,
                           hipStream_t stream) {
    const int64_t tiles_per = (a.hw + kTailPix - 1) / kTailPix, ntiles = tiles_per * a.b * a.v;
    const bool vec = a.hw % 4 == 0;
    const float inv_e = 1.0f / a.exponent;
    SPF_TAIL_K(spf_tail_fwd_kernel, <<<tail_grid(ntiles), kBlock, 0, stream>>>(a, tiles_per, ntiles, inv_e, means, opac, scales,
                                                                              rot, sh, sh_hi))
    return hipGetLastError();
}

hipError_t launch_tail_bwd(const SpfTail& a, const SpfTailGrads& out, const float* g_means, const float* g_opac,
                           const float* g_scales, const float* g_rot, const float* g_sh, const float* g_sh_hi, int split,
                           hipStream_t stream) {
    const int64_t tiles_per = (a.hw + kTailPix - 1) / kTailPix, ntiles = tiles_per * a.b * a.v;
    const bool vec = a.hw % 4 == 0;
    const float inv_e = 1.0f / a.exponent;
    SPF_TAIL_K(spf_tail_bwd_kernel, <<<tail_grid(ntiles), kBlock, 0, stream>>>(a, out, tiles_per, ntiles, inv_e, g_means, g_opac,
                                                                              g_scales, g_rot, g_sh, g_sh_hi, split))
    return hipGetLastError();
}
#undef SPF_TAIL_K

// ---- the opacity map alone: n logits at an element stride (channel 0 of a channels-last tensor read in place) ---------
__global__ __launch_bounds__(kBlock) void spf_opacity_fwd_kernel(const float* __restrict__ x, int64_t stride, int64_t n,
                                                                float e, float inv_e, float* __restrict__ y) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        y[i] = opacity_map(x[i * stride], e, inv_e);
}
__global__ __launch_bounds__(kBlock) void spf_opacity_bwd_kernel(const float* __restrict__ x, int64_t stride, int64_t n,
                                                                float e, float inv_e, const float* __restrict__ dy,
                                                                float* __restrict__ dx) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        dx[i] = dy[i] * opacity_map_grad(x[i * stride], e, inv_e);
}

hipError_t launch_opacity_fwd(const float* x, int64_t stride, int64_t n, float e, float* y, hipStream_t stream) {
    spf_opacity_fwd_kernel<<<tail_grid((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(x, stride, n, e, 1.0f / e, y);
    return hipGetLastError();
}
hipError_t launch_opacity_bwd(const float* x, int64_t stride, int64_t n, float e, const float* dy, float* dx,
                              hipStream_t stream) {
    spf_opacity_bwd_kernel<<<tail_grid((n + kBlock - 1) / kBlock), kBlock, 0, stream>>>(x, stride, n, e, 1.0f / e, dy, dx);
    return hipGetLastError();
}

}  // namespace spf
