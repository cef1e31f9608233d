// The row work of a transformer block between its GEMMs, for gfx950, float32: residual add + LayerNorm (forward and
// backward, with VGGT's LayerScale vector riding in the add) and bias + exact GELU (forward and backward).
//
// Replaces, around the nn.Linear calls of croco/blocks.py:115-131 / 181-203 and vggt/layers/block.py:27-107, the eager
// nn.LayerNorm, nn.GELU, LayerScale and residual-add kernels and the separate passes that sum their parameter gradients.
//
//   spf_block_norm_fwd_kernel   s = x + gamma * r (r, gamma optional), y = LayerNorm(s), per-row mean (two floats) and 1 / std
//   spf_block_norm_bwd_kernel   dx = ds + LN'(dy), dr = gamma * dx, and per block the column sums of dy * xhat, dy and
//                               dx * r (dweight, dbias, dgamma)
//   spf_block_gelu_fwd_kernel   h = GELU(u + b), erf form
//   spf_block_gelu_bwd_kernel   du = dh * GELU'(u + b), and per block the column sums of du (db)
//   spf_block_reduce_kernel     the blocks' partial column sums -> the parameter gradients
//
// Norm kernels: one wave per row, the row in registers as NV 16-byte vectors per lane (vector k of lane l holds columns
// 4 (64 k + l) .. + 3), NV = 1, 2, 4, 8, 16 for C <= 256 .. 4096.  The mean is taken twice -- a float32 mean, then the
// mean of the deviations about it -- and the sums behind the variance and behind the two row means of the backward are
// float64: with 1 / std = 20 a float32 mean alone costs 4e-7 of xhat, more than everything else in the norm together.  A block's four waves take rows grid-stride.  The backward keeps the column
// sums of its rows in registers and the four waves combine them through LDS once, (w0 + w1) + (w2 + w3).
// GELU kernels: no row statistic, so a lane owns four columns and walks down the rows; blockIdx.x picks 256 columns,
// blockIdx.y the rows.  Same combine.
// No float atomic anywhere: every sum has a fixed order (lane -> wave -> block -> the reducer's slices), so two runs
// agree bitwise.  Rows are addressed as (row / inner) * outer_stride + (row % inner) * stride, so that a [B, N, C] slice
// of a [B, V, N, C] tensor is read in place.
#include <math.h>

#include <type_traits>

#include "spf_common.h"
#include "launchers.h"

namespace spf {

constexpr int kBlockWaves = kBlock / kWave;      // rows a block has in flight
constexpr int kNormRowsPerBlock = 16;            // a backward block takes at least this many rows: its partial rows
                                                 // (2 or 3 x C floats) cost as much as 2 or 3 rows of traffic
constexpr int kNormMaxPartialBlocks = 1024;
constexpr int kNormFwdMaxGrid = 2048;
constexpr int kGeluMaxGrid = 2048;               // column tiles x row blocks
constexpr int kGeluTile = 4 * kWave;             // columns of one column tile
constexpr int kReduceSlices = 16;                // the reducer cuts the partial blocks into this many interleaved slices
constexpr int kReduceCols = 4 * (kBlock / kReduceSlices);

struct RowMap {
    int inner;
    int64_t stride, outer_stride;
};
__device__ __forceinline__ int64_t row_offset(const RowMap& m, int row) {
    const int o = row / m.inner;
    return o * m.outer_stride + (row - o * m.inner) * m.stride;
}

// A parameter vector is re-read for every row (from L1 / L2) where a whole row of it would not fit in registers next to
// the row itself: the pointer is made opaque so that the loads are not hoisted out of the row loop and spilled.
template <bool OPAQUE>
__device__ __forceinline__ const float* per_row(const float* p) {
    if constexpr (OPAQUE) asm volatile("" : "+s"(p));
    return p;
}
__device__ __forceinline__ float4 ld4(const float* __restrict__ p, int col, bool on) {
    return on ? *reinterpret_cast<const float4*>(p + col) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void st4(float* __restrict__ p, int col, bool on, float4 v) {
    if (on) *reinterpret_cast<float4*>(p + col) = v;
}
// a row sum in float64, the same in every lane (a butterfly: one order, whatever the grid)
__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// ---- add + LayerNorm, forward ----------------------------------------------------------------------------------------
// MODE 0: y = LN(x); 1: s = x + r; 2: s = x + gamma * r
template <int NV, int MODE>
__global__ __launch_bounds__(kBlock) void spf_block_norm_fwd_kernel(const float* __restrict__ x, RowMap xm,
                                                                    const float* __restrict__ r, RowMap rm,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ weight,
                                                                    const float* __restrict__ bias, int rows, int C,
                                                                    float eps, float* __restrict__ s_out,
                                                                    float* __restrict__ y, float* __restrict__ stats) {
    constexpr bool kReload = NV > 4;
    const int lane = threadIdx.x & (kWave - 1), wave = wave_id();
    const float inv_c = 1.f / (float)C;
    for (int row = blockIdx.x * kBlockWaves + wave; row < rows; row += gridDim.x * kBlockWaves) {
        const float* __restrict__ xr = x + row_offset(xm, row);
        float4 v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = ld4(xr, 4 * (k * kWave + lane), 4 * (k * kWave + lane) < C);
        if constexpr (MODE != 0) {
            const float* __restrict__ rr = r + row_offset(rm, row);
            const float* gp = MODE == 2 ? per_row<kReload>(gamma) : nullptr;
            float* __restrict__ so = s_out + (int64_t)row * C;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int col = 4 * (k * kWave + lane);
                const bool on = col < C;
                const float4 t = ld4(rr, col, on);
                if constexpr (MODE == 2) {
                    const float4 g = ld4(gp, col, on);
                    v[k].x = fmaf(g.x, t.x, v[k].x); v[k].y = fmaf(g.y, t.y, v[k].y);
                    v[k].z = fmaf(g.z, t.z, v[k].z); v[k].w = fmaf(g.w, t.w, v[k].w);
                } else {
                    v[k].x += t.x; v[k].y += t.y; v[k].z += t.z; v[k].w += t.w;
                }
                st4(so, col, on, v[k]);
            }
        }
        // The mean in two steps: mean0, then the mean of the deviations about it, which is what float32 dropped of the
        // row's mean.  With 1 / std large the rounding of a single float32 mean is the largest error of the whole norm.
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) sum += (v[k].x + v[k].y) + (v[k].z + v[k].w);
        const float mean0 = wave_sum(sum) * inv_c;
        float rest = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const bool on = 4 * (k * kWave + lane) < C;
            v[k].x -= mean0; v[k].y -= mean0; v[k].z -= mean0; v[k].w -= mean0;
            rest += on ? (v[k].x + v[k].y) + (v[k].z + v[k].w) : 0.f;
        }
        const float corr = wave_sum(rest) * inv_c;
        double sq = 0.0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const bool on = 4 * (k * kWave + lane) < C;
            v[k].x -= corr; v[k].y -= corr; v[k].z -= corr; v[k].w -= corr;
            const double q = ((double)v[k].x * v[k].x + (double)v[k].y * v[k].y) + ((double)v[k].z * v[k].z + (double)v[k].w * v[k].w);
            sq += on ? q : 0.0;
        }
        const float rstd = (float)(1.0 / sqrt(wave_sum_f64(sq) / (double)C + (double)eps));
        const float* wp = per_row<kReload>(weight);
        const float* bp = per_row<kReload>(bias);
        float* __restrict__ yo = y + (int64_t)row * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const bool on = col < C;
            const float4 w = ld4(wp, col, on), b = ld4(bp, col, on);
            float4 o;
            o.x = fmaf(v[k].x * rstd, w.x, b.x); o.y = fmaf(v[k].y * rstd, w.y, b.y);
            o.z = fmaf(v[k].z * rstd, w.z, b.z); o.w = fmaf(v[k].w * rstd, w.w, b.w);
            st4(yo, col, on, o);
        }
        if (lane == 0) *reinterpret_cast<float4*>(stats + 4 * (int64_t)row) = make_float4(mean0, corr, rstd, 0.f);
    }
}

// The four waves' column sums acc[NV] -> one row of the block's partials, (w0 + w1) + (w2 + w3).  s: [3][NV * 256]
// floats; all threads call it, outside divergent control flow.
template <int NV>
__device__ __forceinline__ void combine_columns(float4 (&acc)[NV], float* __restrict__ s, int lane, int wave, int C,
                                                float* __restrict__ out) {
    constexpr int kRow = NV * 4 * kWave;
    __syncthreads();                                   // the previous call's readers are done
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            *reinterpret_cast<float4*>(s + (wave - 1) * kRow + 4 * (k * kWave + lane)) = acc[k];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const float4 a = *reinterpret_cast<const float4*>(s + col);
            const float4 b = *reinterpret_cast<const float4*>(s + kRow + col);
            const float4 c = *reinterpret_cast<const float4*>(s + 2 * kRow + col);
            float4 o;
            o.x = (acc[k].x + a.x) + (b.x + c.x); o.y = (acc[k].y + a.y) + (b.y + c.y);
            o.z = (acc[k].z + a.z) + (b.z + c.z); o.w = (acc[k].w + a.w) + (b.w + c.w);
            st4(out, col, col < C, o);
        }
    }
}

// ---- add + LayerNorm, backward ---------------------------------------------------------------------------------------
// sx: the saved s (or x where the forward had no r); r, gamma: only with HAS_G.  partial: [2 or 3][gridDim.x][C].
template <int NV, bool HAS_DS, bool HAS_G>
__global__ __launch_bounds__(kBlock) void spf_block_norm_bwd_kernel(const float* __restrict__ sx, RowMap sm,
                                                                    const float* __restrict__ r, RowMap rm,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ weight,
                                                                    const float* __restrict__ dy,
                                                                    const float* __restrict__ ds,
                                                                    const float* __restrict__ stats, int rows, int C,
                                                                    float* __restrict__ dx, float* __restrict__ dr,
                                                                    float* __restrict__ partial) {
    constexpr bool kReload = NV > 4;
    __shared__ float s_acc[3 * NV * 4 * kWave];
    const int lane = threadIdx.x & (kWave - 1), wave = wave_id();
    // the lane's part of the two row sums: float64 (at C = 4 it is the whole sum), float32 where 64 elements per lane
    // leave no register for it (NV = 16, with the wave's sum)
    using LaneSum = typename std::conditional<(NV > 8), float, double>::type;
    float4 acc_w[NV], acc_b[NV], acc_g[HAS_G ? NV : 1];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        acc_w[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        acc_b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (HAS_G) acc_g[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int row = blockIdx.x * kBlockWaves + wave; row < rows; row += gridDim.x * kBlockWaves) {
        const float* __restrict__ xr = sx + row_offset(sm, row);
        const float* __restrict__ gr = dy + (int64_t)row * C;
        const float4 st = *reinterpret_cast<const float4*>(stats + 4 * (int64_t)row);
        // (NV = 16 has no register left for the second part of the mean: there it is folded into one float)
        const float mean0 = NV > 8 ? st.x + st.y : st.x, corr = NV > 8 ? 0.f : st.y, rstd = st.z;
        float4 xh[NV], g[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            xh[k] = ld4(xr, col, col < C);
            g[k] = ld4(gr, col, col < C);
        }
        const float* wp = per_row<kReload>(weight);
        LaneSum s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const bool on = col < C;
            const float4 w = ld4(wp, col, on);
            // (a vector past the row's end holds dy = 0, so its xhat = -mean * rstd reaches no sum)
            xh[k].x = ((xh[k].x - mean0) - corr) * rstd; xh[k].y = ((xh[k].y - mean0) - corr) * rstd;
            xh[k].z = ((xh[k].z - mean0) - corr) * rstd; xh[k].w = ((xh[k].w - mean0) - corr) * rstd;
            acc_b[k].x += g[k].x; acc_b[k].y += g[k].y; acc_b[k].z += g[k].z; acc_b[k].w += g[k].w;
            acc_w[k].x = fmaf(g[k].x, xh[k].x, acc_w[k].x); acc_w[k].y = fmaf(g[k].y, xh[k].y, acc_w[k].y);
            acc_w[k].z = fmaf(g[k].z, xh[k].z, acc_w[k].z); acc_w[k].w = fmaf(g[k].w, xh[k].w, acc_w[k].w);
            g[k].x *= w.x; g[k].y *= w.y; g[k].z *= w.z; g[k].w *= w.w;
            s1 += ((LaneSum)g[k].x + g[k].y) + ((LaneSum)g[k].z + g[k].w);
            s2 += ((LaneSum)g[k].x * xh[k].x + (LaneSum)g[k].y * xh[k].y) + ((LaneSum)g[k].z * xh[k].z + (LaneSum)g[k].w * xh[k].w);
        }
        float c1, c2;
        if constexpr (NV > 8) {
            c1 = wave_sum(s1) / (float)C;
            c2 = wave_sum(s2) / (float)C;
        } else {
            c1 = (float)(wave_sum_f64(s1) / (double)C);
            c2 = (float)(wave_sum_f64(s2) / (double)C);
        }
        float* __restrict__ dxo = dx + (int64_t)row * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const bool on = col < C;
            float4 d;
            d.x = (g[k].x - c1 - xh[k].x * c2) * rstd; d.y = (g[k].y - c1 - xh[k].y * c2) * rstd;
            d.z = (g[k].z - c1 - xh[k].z * c2) * rstd; d.w = (g[k].w - c1 - xh[k].w * c2) * rstd;
            if constexpr (HAS_DS) {
                const float4 u = ld4(ds + (int64_t)row * C, col, on);
                d.x += u.x; d.y += u.y; d.z += u.z; d.w += u.w;
            }
            st4(dxo, col, on, d);
            if constexpr (HAS_G) {
                const float4 t = ld4(r + row_offset(rm, row), col, on);
                const float4 gm = ld4(per_row<kReload>(gamma), col, on);
                acc_g[k].x = fmaf(d.x, t.x, acc_g[k].x); acc_g[k].y = fmaf(d.y, t.y, acc_g[k].y);
                acc_g[k].z = fmaf(d.z, t.z, acc_g[k].z); acc_g[k].w = fmaf(d.w, t.w, acc_g[k].w);
                st4(dr + (int64_t)row * C, col, on, make_float4(gm.x * d.x, gm.y * d.y, gm.z * d.z, gm.w * d.w));
            }
        }
    }
    const int64_t kind = (int64_t)gridDim.x * C;
    float* __restrict__ mine = partial + (int64_t)blockIdx.x * C;
    combine_columns<NV>(acc_w, s_acc, lane, wave, C, mine);
    combine_columns<NV>(acc_b, s_acc, lane, wave, C, mine + kind);
    if constexpr (HAS_G) combine_columns<NV>(acc_g, s_acc, lane, wave, C, mine + 2 * kind);
}

// ---- bias + GELU -----------------------------------------------------------------------------------------------------
// torch's formulas (aten/src/ATen/native/cuda/ActivationGeluKernel.cu, 'none'): 0.5 z (1 + erf(z / sqrt 2)) and
// dh (cdf + z pdf), cdf = 0.5 (1 + erf(z / sqrt 2)), pdf = exp(-z^2 / 2) / sqrt(2 pi)
__device__ __forceinline__ float gelu_f(float z) { return 0.5f * z * (1.f + erff(z * 0.70710678118654752440f)); }
__device__ __forceinline__ float gelu_grad_f(float z) {
    const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752440f));
    const float pdf = expf(-0.5f * z * z) * 0.39894228040143267794f;
    return fmaf(z, pdf, cdf);
}

template <bool HAS_B>
__global__ __launch_bounds__(kBlock) void spf_block_gelu_fwd_kernel(const float* __restrict__ u,
                                                                    const float* __restrict__ bias, int rows, int C,
                                                                    float* __restrict__ h) {
    const int lane = threadIdx.x & (kWave - 1), wave = wave_id();
    const int col = blockIdx.x * kGeluTile + 4 * lane;
    if (col >= C) return;                                // (no barrier below)
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (HAS_B) b = *reinterpret_cast<const float4*>(bias + col);
#pragma unroll 4
    for (int row = blockIdx.y * kBlockWaves + wave; row < rows; row += gridDim.y * kBlockWaves) {
        const float4 z = *reinterpret_cast<const float4*>(u + (int64_t)row * C + col);
        *reinterpret_cast<float4*>(h + (int64_t)row * C + col) =
            make_float4(gelu_f(z.x + b.x), gelu_f(z.y + b.y), gelu_f(z.z + b.z), gelu_f(z.w + b.w));
    }
}

// partial: [gridDim.y][C] (only with HAS_B)
template <bool HAS_B>
__global__ __launch_bounds__(kBlock) void spf_block_gelu_bwd_kernel(const float* __restrict__ u,
                                                                    const float* __restrict__ bias,
                                                                    const float* __restrict__ dh, int rows, int C,
                                                                    float* __restrict__ du, float* __restrict__ partial) {
    __shared__ float s_acc[3 * kGeluTile];
    const int lane = threadIdx.x & (kWave - 1), wave = wave_id();
    const int col = blockIdx.x * kGeluTile + 4 * lane;
    const bool on = col < C;
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (HAS_B) b = ld4(bias, col, on);
    float4 acc[1] = {make_float4(0.f, 0.f, 0.f, 0.f)};
    if (on) {
#pragma unroll 4
        for (int row = blockIdx.y * kBlockWaves + wave; row < rows; row += gridDim.y * kBlockWaves) {
            const float4 z = *reinterpret_cast<const float4*>(u + (int64_t)row * C + col);
            const float4 g = *reinterpret_cast<const float4*>(dh + (int64_t)row * C + col);
            float4 d;
            d.x = g.x * gelu_grad_f(z.x + b.x); d.y = g.y * gelu_grad_f(z.y + b.y);
            d.z = g.z * gelu_grad_f(z.z + b.z); d.w = g.w * gelu_grad_f(z.w + b.w);
            *reinterpret_cast<float4*>(du + (int64_t)row * C + col) = d;
            acc[0].x += d.x; acc[0].y += d.y; acc[0].z += d.z; acc[0].w += d.w;
        }
    }
    if constexpr (HAS_B) {
        // combine_columns with the tile's 256 columns: its column index is the tile's, so hand it the tile's origin
        const int base = blockIdx.x * kGeluTile;
        combine_columns<1>(acc, s_acc, lane, wave, C - base, partial + (int64_t)blockIdx.y * C + base);
    }
}

// ---- the reducer -----------------------------------------------------------------------------------------------------
// partial [K][nb][C] -> out [K][C]; blockIdx.x: 64 columns, blockIdx.y: k.  Slice j of 16 sums blocks j, j + 16, .. in
// that order, then the slices as a tree that halves from 8 down.
__global__ __launch_bounds__(kBlock) void spf_block_reduce_kernel(const float* __restrict__ partial, int nb, int C,
                                                                  float* __restrict__ out) {
    __shared__ float4 s_tree[kReduceSlices][kBlock / kReduceSlices];
    const int cv = threadIdx.x & (kBlock / kReduceSlices - 1), slice = threadIdx.x / (kBlock / kReduceSlices);
    const int col = blockIdx.x * kReduceCols + 4 * cv;
    const bool on = col < C;
    const float* __restrict__ p = partial + (int64_t)blockIdx.y * nb * C;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (on) {
#pragma unroll 4
        for (int b = slice; b < nb; b += kReduceSlices) {
            const float4 t = *reinterpret_cast<const float4*>(p + (int64_t)b * C + col);
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
        }
    }
    s_tree[slice][cv] = a;
    __syncthreads();
    for (int half = kReduceSlices / 2; half > 0; half >>= 1) {
        if (slice < half) {
            const float4 t = s_tree[slice + half][cv];
            a.x += t.x; a.y += t.y; a.z += t.z; a.w += t.w;
            s_tree[slice][cv] = a;
        }
        __syncthreads();
    }
    if (slice == 0 && on) *reinterpret_cast<float4*>(out + (int64_t)blockIdx.y * C + col) = a;
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int ceil_div64(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// blocks that write one row of partial column sums each: the norm backward (gelu = 0) or the GELU backward (gelu = 1)
int64_t block_partial_blocks(int64_t rows, int C, int gelu) {
    const int64_t want = (rows + kNormRowsPerBlock - 1) / kNormRowsPerBlock;
    int64_t cap = kNormMaxPartialBlocks;
    if (gelu) {
        const int tiles = (C + kGeluTile - 1) / kGeluTile;
        cap = kGeluMaxGrid / tiles > 0 ? kGeluMaxGrid / tiles : 1;
    }
    return want < cap ? want : cap;
}

static RowMap row_map(int64_t inner, int64_t stride, int64_t outer_stride) {
    return RowMap{(int)(inner > 0 ? inner : 1), stride, outer_stride};
}
static int vectors_per_lane(int C) {
    int nv = 1;
    while (nv * 4 * kWave < C) nv *= 2;
    return nv;
}

template <int NV>
static void norm_fwd_nv(const SpfBlockNorm& a, int grid, float* s, float* y, float* stats, hipStream_t st) {
    const RowMap xm = row_map(a.x_inner, a.x_stride, a.x_outer_stride), rm = row_map(a.r_inner, a.r_stride, a.r_outer_stride);
    const int rows = (int)a.rows;
    if (!a.r)
        spf_block_norm_fwd_kernel<NV, 0><<<grid, kBlock, 0, st>>>(a.x, xm, nullptr, rm, nullptr, a.weight, a.bias, rows, a.C, a.eps, s, y, stats);
    else if (!a.gamma)
        spf_block_norm_fwd_kernel<NV, 1><<<grid, kBlock, 0, st>>>(a.x, xm, a.r, rm, nullptr, a.weight, a.bias, rows, a.C, a.eps, s, y, stats);
    else
        spf_block_norm_fwd_kernel<NV, 2><<<grid, kBlock, 0, st>>>(a.x, xm, a.r, rm, a.gamma, a.weight, a.bias, rows, a.C, a.eps, s, y, stats);
}

hipError_t launch_block_norm_fwd(const SpfBlockNorm& a, float* s, float* y, float* stats, hipStream_t st) {
    const int need = ceil_div64(a.rows, kBlockWaves);
    const int grid = need < kNormFwdMaxGrid ? need : kNormFwdMaxGrid;
    switch (vectors_per_lane(a.C)) {
        case 1: norm_fwd_nv<1>(a, grid, s, y, stats, st); break;
        case 2: norm_fwd_nv<2>(a, grid, s, y, stats, st); break;
        case 4: norm_fwd_nv<4>(a, grid, s, y, stats, st); break;
        case 8: norm_fwd_nv<8>(a, grid, s, y, stats, st); break;
        default: norm_fwd_nv<16>(a, grid, s, y, stats, st); break;
    }
    return hipGetLastError();
}

template <int NV, bool HAS_DS>
static void norm_bwd_nv(const SpfBlockNorm& a, int grid, const float* dy, const float* ds, const float* stats, float* dx,
                        float* dr, float* partial, hipStream_t st) {
    const RowMap xm = row_map(a.x_inner, a.x_stride, a.x_outer_stride), rm = row_map(a.r_inner, a.r_stride, a.r_outer_stride);
    const int rows = (int)a.rows;
    if (a.gamma)
        spf_block_norm_bwd_kernel<NV, HAS_DS, true><<<grid, kBlock, 0, st>>>(a.x, xm, a.r, rm, a.gamma, a.weight, dy, ds, stats, rows, a.C, dx, dr, partial);
    else
        spf_block_norm_bwd_kernel<NV, HAS_DS, false><<<grid, kBlock, 0, st>>>(a.x, xm, nullptr, rm, nullptr, a.weight, dy, ds, stats, rows, a.C, dx, nullptr, partial);
}
template <int NV>
static void norm_bwd_ds(const SpfBlockNorm& a, int grid, const float* dy, const float* ds, const float* stats, float* dx,
                        float* dr, float* partial, hipStream_t st) {
    if (ds) norm_bwd_nv<NV, true>(a, grid, dy, ds, stats, dx, dr, partial, st);
    else norm_bwd_nv<NV, false>(a, grid, dy, nullptr, stats, dx, dr, partial, st);
}

static void launch_reduce(const float* partial, int kinds, int nb, int C, float* out, hipStream_t st) {
    const dim3 grid((C + kReduceCols - 1) / kReduceCols, kinds);
    spf_block_reduce_kernel<<<grid, kBlock, 0, st>>>(partial, nb, C, out);
}

hipError_t launch_block_norm_bwd(const SpfBlockNorm& a, const float* dy, const float* ds, const float* stats, float* dx,
                                 float* dr, float* partial, float* dparams, hipStream_t st) {
    const int grid = (int)block_partial_blocks(a.rows, a.C, 0);
    switch (vectors_per_lane(a.C)) {
        case 1: norm_bwd_ds<1>(a, grid, dy, ds, stats, dx, dr, partial, st); break;
        case 2: norm_bwd_ds<2>(a, grid, dy, ds, stats, dx, dr, partial, st); break;
        case 4: norm_bwd_ds<4>(a, grid, dy, ds, stats, dx, dr, partial, st); break;
        case 8: norm_bwd_ds<8>(a, grid, dy, ds, stats, dx, dr, partial, st); break;
        default: norm_bwd_ds<16>(a, grid, dy, ds, stats, dx, dr, partial, st); break;
    }
    launch_reduce(partial, a.gamma ? 3 : 2, grid, a.C, dparams, st);
    return hipGetLastError();
}

hipError_t launch_block_gelu_fwd(const float* u, const float* bias, int64_t rows, int C, float* h, hipStream_t st) {
    const dim3 grid((C + kGeluTile - 1) / kGeluTile, (unsigned)block_partial_blocks(rows, C, 1));
    if (bias) spf_block_gelu_fwd_kernel<true><<<grid, kBlock, 0, st>>>(u, bias, (int)rows, C, h);
    else spf_block_gelu_fwd_kernel<false><<<grid, kBlock, 0, st>>>(u, nullptr, (int)rows, C, h);
    return hipGetLastError();
}

hipError_t launch_block_gelu_bwd(const float* u, const float* bias, const float* dh, int64_t rows, int C, float* du,
                                 float* partial, float* dbias, hipStream_t st) {
    const int nb = (int)block_partial_blocks(rows, C, 1);
    const dim3 grid((C + kGeluTile - 1) / kGeluTile, nb);
    if (bias) {
        spf_block_gelu_bwd_kernel<true><<<grid, kBlock, 0, st>>>(u, bias, dh, (int)rows, C, du, partial);
        launch_reduce(partial, 1, nb, C, dbias, st);
    } else {
        spf_block_gelu_bwd_kernel<false><<<grid, kBlock, 0, st>>>(u, nullptr, dh, (int)rows, C, du, nullptr);
    }
    return hipGetLastError();
}

}  // namespace spf
