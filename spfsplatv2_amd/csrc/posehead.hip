// The pose heads between their GEMMs, for gfx950, float32: the MLP PoseHead of heads/pose_head.py and VGGT's CameraHead
// (vggt/heads/camera_head.py) with its adaptive-LayerNorm trunk.  The nn.Linear calls stay GEMMs; everything between
// them is here, forward and backward:
//
//   spf_posehead_pool_*        token mean of up to two sources, concatenated on the channel axis (cat + rearrange +
//                              AdaptiveAvgPool2d + view); L = 1 is a copy
//   spf_posehead_encode_*      fc_rot's six floats and fc_t's three (or four: t / h, h = min(softplus(t3) + 1 / max_scale,
//                              1 / min_scale)) -> the 9-float pose row, written where the caller's [b, v, 9] tensor has it
//   spf_posehead_embed_silu_*  SiLU(p W^T + b), p [rows, 9] or one broadcast row: embed_pose and the SiLU of
//                              poseLN_modulation
//   spf_posehead_modulate_*    gate * (LN(x) * (1 + scale) + shift) + x, LN without parameters; shift, scale, gate are the
//                              three column thirds of the Linear's [rows, 3 C] output, read (and their gradient written)
//                              in place
//   spf_posehead_attn_*        softmax(q k^T D^-1/2) v over S <= 32 views, D = 64 or 128, packed qkv in, packed dqkv out
//   spf_posehead_activate_*    pred = prev + delta, out = activate_pose(pred)
//
// Row kernels (modulate) have the shape of block.hip's norm: one wave per row, the row in registers as NV 16-byte vectors
// per lane, the mean in two steps and the variance from the centred values with a float64 sum.  Attention: one block per
// (batch item, head), K and V of the head in LDS (rows padded by four floats), q and dout read from global memory -- a
// row of them is read by all lanes that share a query.  The scores of a head (at most 32 x 32) live in LDS.
// No atomics anywhere: every sum has one order (lane -> wave -> block, or a loop over the rows), two runs agree bitwise.
#include <math.h>

#include <type_traits>

#include "spf_common.h"
#include "launchers.h"

namespace spf {

constexpr int kPhWaves = kBlock / kWave;
constexpr int kPhMaxGrid = 2048;
constexpr int kPhTile = 4 * kWave;                 // columns of one column tile: a 16-byte vector per lane
constexpr int kPhMaxS = SPF_POSEHEAD_MAX_S;
constexpr int kPhPad = 4;                          // floats added to a K / V row in LDS: 16-byte reads stay aligned

struct PhRowMap {
    int inner;
    int64_t stride, outer_stride;
};
__device__ __forceinline__ int64_t ph_row_offset(const PhRowMap& m, int row) {
    const int o = row / m.inner;
    return o * m.outer_stride + (row - o * m.inner) * m.stride;
}
static PhRowMap ph_row_map(int64_t inner, int64_t stride, int64_t outer_stride) {
    return PhRowMap{(int)(inner > 0 ? inner : 1), stride, outer_stride};
}
__device__ __forceinline__ float4 ph_ld4(const float* __restrict__ p, int col, bool on) {
    return on ? *reinterpret_cast<const float4*>(p + col) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ void ph_st4(float* __restrict__ p, int col, bool on, float4 v) {
    if (on) *reinterpret_cast<float4*>(p + col) = v;
}
__device__ __forceinline__ double ph_wave_sum_f64(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}
__device__ __forceinline__ int ph_wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
static int ph_grid(int64_t items) {
    const int64_t need = (items + kBlock - 1) / kBlock;
    return (int)(need < 1 ? 1 : need < kPhMaxGrid ? need : kPhMaxGrid);
}

// ---- a. token mean, two sources ----------------------------------------------------------------------------------------
struct PhPoolSrc {
    const float* p;
    PhRowMap m;
    int64_t tok;
    int C;
};

// grid (column tiles of C0 + C1, rows).  The block's four waves take the tokens l = wave, wave + 4, ..; their sums are
// float64 (the kernel waits for memory, and a float32 sum of 64 tokens would be the largest error of the head) and meet
// in LDS as (w0 + w1) + (w2 + w3).
__global__ __launch_bounds__(kBlock) void spf_posehead_pool_fwd_kernel(PhPoolSrc s0, PhPoolSrc s1, int L, int Ct,
                                                                       float* __restrict__ out) {
    __shared__ double s_acc[3][kPhTile];
    const int lane = threadIdx.x & (kWave - 1), wave = ph_wave_id();
    const int row = blockIdx.y, col = blockIdx.x * kPhTile + 4 * lane;
    const bool on = col < Ct, first = col < s0.C;
    const PhPoolSrc& s = first ? s0 : s1;
    const int c = first ? col : col - s0.C;
    const float* __restrict__ base = on ? s.p + ph_row_offset(s.m, row) + c : nullptr;
    float* __restrict__ o = out + (int64_t)row * Ct;
    if (L == 1) {                                          // the mean of one value is that value, bit for bit
        if (wave == 0 && on) *reinterpret_cast<float4*>(o + col) = *reinterpret_cast<const float4*>(base);
        return;
    }
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (on) {
#pragma unroll 4
        for (int l = wave; l < L; l += kPhWaves) {
            const float4 t = *reinterpret_cast<const float4*>(base + (int64_t)l * s.tok);
            a[0] += t.x; a[1] += t.y; a[2] += t.z; a[3] += t.w;
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_acc[wave - 1][4 * lane + k] = a[k];
    }
    __syncthreads();
    if (wave == 0 && on) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            r[k] = (float)(((a[k] + s_acc[0][4 * lane + k]) + (s_acc[1][4 * lane + k] + s_acc[2][4 * lane + k])) / (double)L);
        *reinterpret_cast<float4*>(o + col) = make_float4(r[0], r[1], r[2], r[3]);
    }
}

// d_src s [rows, L, C_s] dense = d_feat[row, off_s + c] / L: flat over the 16-byte vectors of both gradients
__global__ __launch_bounds__(kBlock) void spf_posehead_pool_bwd_kernel(const float* __restrict__ d_feat, int L, int C0,
                                                                       int C1, int64_t n0, int64_t n1,
                                                                       float* __restrict__ d0, float* __restrict__ d1) {
    const int Ct = C0 + C1;
    const float n = (float)L;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n0 + n1; i += (int64_t)gridDim.x * kBlock) {
        const bool first = i < n0;
        const int64_t j = first ? i : i - n0;
        const int cv = (first ? C0 : C1) / 4;
        const int64_t row = j / ((int64_t)L * cv);
        const int c = 4 * (int)(j % cv);
        const float4 g = *reinterpret_cast<const float4*>(d_feat + row * Ct + (first ? 0 : C0) + c);
        reinterpret_cast<float4*>(first ? d0 : d1)[j] = make_float4(g.x / n, g.y / n, g.z / n, g.w / n);
    }
}

hipError_t launch_posehead_pool_fwd(const SpfPosePool& a, float* feat, hipStream_t st) {
    const PhPoolSrc s0{a.src[0], ph_row_map(a.inner[0], a.stride[0], a.outer_stride[0]), a.tok_stride[0], a.C[0]};
    const PhPoolSrc s1{a.src[1], ph_row_map(a.inner[1], a.stride[1], a.outer_stride[1]), a.tok_stride[1],
                       a.src[1] ? a.C[1] : 0};
    const int Ct = s0.C + s1.C;
    const dim3 grid((Ct + kPhTile - 1) / kPhTile, (unsigned)a.rows);
    spf_posehead_pool_fwd_kernel<<<grid, kBlock, 0, st>>>(s0, s1, a.L, Ct, feat);
    return hipGetLastError();
}

hipError_t launch_posehead_pool_bwd(const SpfPosePool& a, const float* d_feat, float* d0, float* d1, hipStream_t st) {
    const int C1 = d1 ? a.C[1] : 0;
    const int64_t n0 = a.rows * a.L * (a.C[0] / 4), n1 = a.rows * a.L * (C1 / 4);
    spf_posehead_pool_bwd_kernel<<<ph_grid(n0 + n1), kBlock, 0, st>>>(d_feat, a.L, a.C[0], C1, n0, n1, d0, d1);
    return hipGetLastError();
}

// ---- b. the head's tail ------------------------------------------------------------------------------------------------
// torch's softplus: linear where beta x > 20
__device__ __forceinline__ float ph_softplus(float x, float beta) {
    const float z = x * beta;
    return z > 20.f ? x : log1pf(expf(z)) / beta;
}
__device__ __forceinline__ float ph_softplus_grad(float x, float beta) {
    const float z = x * beta;
    if (z > 20.f) return 1.f;
    const float e = expf(z);
    return e / (e + 1.f);
}

__global__ __launch_bounds__(kBlock) void spf_posehead_encode_fwd_kernel(const float* __restrict__ rot,
                                                                         const float* __restrict__ t, int rows, int homog,
                                                                         float beta, float max_inv, float min_inv,
                                                                         PhRowMap om, float* __restrict__ out) {
    // (the grid is capped: a thread takes rows grid-stride)
    for (int row = blockIdx.x * kBlock + threadIdx.x; row < rows; row += gridDim.x * kBlock) {
        float* __restrict__ o = out + ph_row_offset(om, row);
#pragma unroll
        for (int k = 0; k < 6; ++k) o[k] = rot[6 * (int64_t)row + k];
        const float* __restrict__ tr = t + (homog ? 4 : 3) * (int64_t)row;
        float h = 1.f;
        if (homog) h = fminf(ph_softplus(tr[3], beta) + max_inv, min_inv);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[6 + k] = homog ? tr[k] / h : tr[k];
    }
}

__global__ __launch_bounds__(kBlock) void spf_posehead_encode_bwd_kernel(const float* __restrict__ t,
                                                                         const float* __restrict__ d_out, int rows,
                                                                         int homog, float beta, float max_inv,
                                                                         float min_inv, PhRowMap om,
                                                                         float* __restrict__ d_rot, float* __restrict__ d_t) {
    for (int row = blockIdx.x * kBlock + threadIdx.x; row < rows; row += gridDim.x * kBlock) {
        const float* __restrict__ g = d_out + ph_row_offset(om, row);
#pragma unroll
        for (int k = 0; k < 6; ++k) d_rot[6 * (int64_t)row + k] = g[k];
        if (!homog) {
#pragma unroll
            for (int k = 0; k < 3; ++k) d_t[3 * (int64_t)row + k] = g[6 + k];
            continue;
        }
        const float* __restrict__ tr = t + 4 * (int64_t)row;
        const float raw = ph_softplus(tr[3], beta) + max_inv;
        const float h = fminf(raw, min_inv);
        float dh = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            d_t[4 * (int64_t)row + k] = g[6 + k] / h;
            dh -= g[6 + k] * tr[k] / (h * h);
        }
        d_t[4 * (int64_t)row + 3] = raw <= min_inv ? dh * ph_softplus_grad(tr[3], beta) : 0.f;   // nothing through the clamp
    }
}

hipError_t launch_posehead_encode_fwd(const SpfPoseEncode& a, const float* rot, const float* t, float* out, hipStream_t st) {
    spf_posehead_encode_fwd_kernel<<<ph_grid(a.rows), kBlock, 0, st>>>(
        rot, t, (int)a.rows, a.homogeneous, a.beta, a.max_inv_scale, a.min_inv_scale,
        ph_row_map(a.out_inner, a.out_stride, a.out_outer_stride), out);
    return hipGetLastError();
}

hipError_t launch_posehead_encode_bwd(const SpfPoseEncode& a, const float* t, const float* d_out, float* d_rot, float* d_t,
                                      hipStream_t st) {
    spf_posehead_encode_bwd_kernel<<<ph_grid(a.rows), kBlock, 0, st>>>(
        t, d_out, (int)a.rows, a.homogeneous, a.beta, a.max_inv_scale, a.min_inv_scale,
        ph_row_map(a.out_inner, a.out_stride, a.out_outer_stride), d_rot, d_t);
    return hipGetLastError();
}

// ---- c. SiLU(p W^T + b) ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ph_sigmoid(float z) { return 1.f / (1.f + expf(-z)); }
__device__ __forceinline__ float ph_embed_z(const float* __restrict__ p, const float* __restrict__ w, float b) {
    float z = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) z = fmaf(p[k], w[k], z);
    return z + b;
}
// dSiLU / dz = sigma (1 + z (1 - sigma))
__device__ __forceinline__ float ph_silu_grad(float z) {
    const float sg = ph_sigmoid(z);
    return sg * fmaf(z, 1.f - sg, 1.f);
}

__global__ __launch_bounds__(kBlock) void spf_posehead_embed_fwd_kernel(const float* __restrict__ p, int bcast,
                                                                        const float* __restrict__ W,
                                                                        const float* __restrict__ b, int64_t n, int C,
                                                                        float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int64_t r = i / C;
        const int c = (int)(i - r * C);
        const float z = ph_embed_z(bcast ? p : p + 9 * r, W + 9 * c, b[c]);
        out[i] = z * ph_sigmoid(z);
    }
}

// a thread owns a column and walks down the rows: dW[c, :] and db[c], one order
__global__ __launch_bounds__(kBlock) void spf_posehead_embed_bwd_params_kernel(const float* __restrict__ p, int bcast,
                                                                               const float* __restrict__ W,
                                                                               const float* __restrict__ b,
                                                                               const float* __restrict__ dout, int rows,
                                                                               int C, float* __restrict__ dW,
                                                                               float* __restrict__ db) {
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    float w[9];
    double acc[9], accb = 0.0;                             // float64 down the rows: a handful of adds per launch
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = W[9 * c + k], acc[k] = 0.0;
    const float bc = b[c];
    for (int r = 0; r < rows; ++r) {
        const float* __restrict__ pr = bcast ? p : p + 9 * (int64_t)r;
        const float dz = dout[(int64_t)r * C + c] * ph_silu_grad(ph_embed_z(pr, w, bc));
        accb += dz;
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] += (double)dz * pr[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) dW[9 * c + k] = (float)acc[k];
    db[c] = (float)accb;
}

// dp[r, :] = sum over c of dz[r, c] W[c, :], one block per row; with the broadcast row the sum over the rows too, which
// is sum over c of db[c] W[c, :]: one block reads db
template <bool BCAST>
__global__ __launch_bounds__(kBlock) void spf_posehead_embed_bwd_p_kernel(const float* __restrict__ p,
                                                                          const float* __restrict__ W,
                                                                          const float* __restrict__ b,
                                                                          const float* __restrict__ dout,
                                                                          const float* __restrict__ db, int C,
                                                                          float* __restrict__ dp) {
    __shared__ double s_part[kPhWaves][9];
    const int lane = threadIdx.x & (kWave - 1), wave = ph_wave_id();
    const int r = blockIdx.x;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = 0.0;
    for (int c = threadIdx.x; c < C; c += kBlock) {
        const float* __restrict__ w = W + 9 * c;
        float dz;
        if constexpr (BCAST) dz = db[c];
        else dz = dout[(int64_t)r * C + c] * ph_silu_grad(ph_embed_z(p + 9 * (int64_t)r, w, b[c]));
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[k] += (double)dz * w[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const double t = ph_wave_sum_f64(acc[k]);
        if (lane == 0) s_part[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const int k = threadIdx.x;
        dp[9 * (int64_t)r + k] = (float)((s_part[0][k] + s_part[1][k]) + (s_part[2][k] + s_part[3][k]));
    }
}

hipError_t launch_posehead_embed_fwd(const float* p, int bcast, const float* W, const float* b, int64_t rows, int C,
                                     float* out, hipStream_t st) {
    spf_posehead_embed_fwd_kernel<<<ph_grid(rows * C), kBlock, 0, st>>>(p, bcast, W, b, rows * C, C, out);
    return hipGetLastError();
}

hipError_t launch_posehead_embed_bwd(const float* p, int bcast, const float* W, const float* b, const float* dout,
                                     int64_t rows, int C, float* dW, float* db, float* dp, hipStream_t st) {
    spf_posehead_embed_bwd_params_kernel<<<(C + kBlock - 1) / kBlock, kBlock, 0, st>>>(p, bcast, W, b, dout, (int)rows, C,
                                                                                     dW, db);
    if (dp) {
        if (bcast) spf_posehead_embed_bwd_p_kernel<true><<<1, kBlock, 0, st>>>(p, W, b, dout, db, C, dp);
        else spf_posehead_embed_bwd_p_kernel<false><<<(unsigned)rows, kBlock, 0, st>>>(p, W, b, dout, db, C, dp);
    }
    return hipGetLastError();
}

// ---- d. adaptive LayerNorm ---------------------------------------------------------------------------------------------
// Centres the row held in v (the mean in two steps, as block.hip takes it) and returns 1 / sqrt(var + eps), the variance
// from the centred values with a float64 sum.  Vectors past the row's end hold rubbish afterwards: mask what reads them.
template <int NV>
__device__ __forceinline__ float ph_centre_row(float4 (&v)[NV], int C, float eps, int lane) {
    const float inv_c = 1.f / (float)C;
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
    return (float)(1.0 / sqrt(ph_wave_sum_f64(sq) / (double)C + (double)eps));
}

template <int NV>
__global__ __launch_bounds__(kBlock) void spf_posehead_modulate_fwd_kernel(const float* __restrict__ x,
                                                                           const float* __restrict__ mod, int rows, int C,
                                                                           float eps, float* __restrict__ out) {
    const int lane = threadIdx.x & (kWave - 1), wave = ph_wave_id();
    for (int row = blockIdx.x * kPhWaves + wave; row < rows; row += gridDim.x * kPhWaves) {
        const float* __restrict__ xr = x + (int64_t)row * C;
        const float* __restrict__ mr = mod + (int64_t)row * 3 * C;
        float* __restrict__ o = out + (int64_t)row * C;
        float4 v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = ph_ld4(xr, 4 * (k * kWave + lane), 4 * (k * kWave + lane) < C);
        const float rstd = ph_centre_row<NV>(v, C, eps, lane);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const bool on = col < C;
            const float4 sh = ph_ld4(mr, col, on), sc = ph_ld4(mr + C, col, on), g = ph_ld4(mr + 2 * C, col, on);
            const float4 x0 = ph_ld4(xr, col, on);
            float4 r;
            r.x = fmaf(g.x, fmaf(v[k].x * rstd, 1.f + sc.x, sh.x), x0.x);
            r.y = fmaf(g.y, fmaf(v[k].y * rstd, 1.f + sc.y, sh.y), x0.y);
            r.z = fmaf(g.z, fmaf(v[k].z * rstd, 1.f + sc.z, sh.z), x0.z);
            r.w = fmaf(g.w, fmaf(v[k].w * rstd, 1.f + sc.w, sh.w), x0.w);
            ph_st4(o, col, on, r);
        }
    }
}

// n = LN(x), m = n (1 + scale) + shift, out = gate m + x:
//   dgate = dout m, dshift = dm = dout gate, dscale = dm n, dn = dm (1 + scale), dx = dout + LN'(dn)
template <int NV>
__global__ __launch_bounds__(kBlock) void spf_posehead_modulate_bwd_kernel(const float* __restrict__ x,
                                                                           const float* __restrict__ mod,
                                                                           const float* __restrict__ dout, int rows, int C,
                                                                           float eps, float* __restrict__ dx,
                                                                           float* __restrict__ dmod) {
    using LaneSum = typename std::conditional<(NV > 8), float, double>::type;
    const int lane = threadIdx.x & (kWave - 1), wave = ph_wave_id();
    for (int row = blockIdx.x * kPhWaves + wave; row < rows; row += gridDim.x * kPhWaves) {
        const float* __restrict__ xr = x + (int64_t)row * C;
        const float* __restrict__ mr = mod + (int64_t)row * 3 * C;
        const float* __restrict__ gr = dout + (int64_t)row * C;
        float* __restrict__ dm = dmod + (int64_t)row * 3 * C;
        float4 n[NV], dn[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) n[k] = ph_ld4(xr, 4 * (k * kWave + lane), 4 * (k * kWave + lane) < C);
        const float rstd = ph_centre_row<NV>(n, C, eps, lane);
        LaneSum s1 = 0, s2 = 0;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const bool on = col < C;
            const float4 sh = ph_ld4(mr, col, on), sc = ph_ld4(mr + C, col, on), gt = ph_ld4(mr + 2 * C, col, on);
            const float4 g = ph_ld4(gr, col, on);                 // (zero past the row's end, and so is everything below)
            n[k].x *= rstd; n[k].y *= rstd; n[k].z *= rstd; n[k].w *= rstd;
            const float4 d = make_float4(g.x * gt.x, g.y * gt.y, g.z * gt.z, g.w * gt.w);
            ph_st4(dm, col, on, d);
            ph_st4(dm + C, col, on, make_float4(d.x * n[k].x, d.y * n[k].y, d.z * n[k].z, d.w * n[k].w));
            ph_st4(dm + 2 * C, col, on, make_float4(g.x * fmaf(n[k].x, 1.f + sc.x, sh.x), g.y * fmaf(n[k].y, 1.f + sc.y, sh.y),
                                                   g.z * fmaf(n[k].z, 1.f + sc.z, sh.z), g.w * fmaf(n[k].w, 1.f + sc.w, sh.w)));
            dn[k] = make_float4(d.x * (1.f + sc.x), d.y * (1.f + sc.y), d.z * (1.f + sc.z), d.w * (1.f + sc.w));
            s1 += ((LaneSum)dn[k].x + dn[k].y) + ((LaneSum)dn[k].z + dn[k].w);
            s2 += ((LaneSum)dn[k].x * n[k].x + (LaneSum)dn[k].y * n[k].y) + ((LaneSum)dn[k].z * n[k].z + (LaneSum)dn[k].w * n[k].w);
        }
        float c1, c2;
        if constexpr (NV > 8) {
            c1 = wave_sum(s1) / (float)C;
            c2 = wave_sum(s2) / (float)C;
        } else {
            c1 = (float)(ph_wave_sum_f64(s1) / (double)C);
            c2 = (float)(ph_wave_sum_f64(s2) / (double)C);
        }
        float* __restrict__ o = dx + (int64_t)row * C;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int col = 4 * (k * kWave + lane);
            const bool on = col < C;
            const float4 g = ph_ld4(gr, col, on);
            ph_st4(o, col, on, make_float4(fmaf(dn[k].x - c1 - n[k].x * c2, rstd, g.x), fmaf(dn[k].y - c1 - n[k].y * c2, rstd, g.y),
                                           fmaf(dn[k].z - c1 - n[k].z * c2, rstd, g.z), fmaf(dn[k].w - c1 - n[k].w * c2, rstd, g.w)));
        }
    }
}

static int ph_vectors_per_lane(int C) {
    int nv = 1;
    while (nv * 4 * kWave < C) nv *= 2;
    return nv;
}
static int ph_row_grid(int64_t rows) {
    const int64_t need = (rows + kPhWaves - 1) / kPhWaves;
    return (int)(need < kPhMaxGrid ? need : kPhMaxGrid);
}

hipError_t launch_posehead_modulate_fwd(const float* x, const float* mod, int64_t rows, int C, float eps, float* out,
                                        hipStream_t st) {
    const int grid = ph_row_grid(rows), r = (int)rows;
    switch (ph_vectors_per_lane(C)) {
        case 1: spf_posehead_modulate_fwd_kernel<1><<<grid, kBlock, 0, st>>>(x, mod, r, C, eps, out); break;
        case 2: spf_posehead_modulate_fwd_kernel<2><<<grid, kBlock, 0, st>>>(x, mod, r, C, eps, out); break;
        case 4: spf_posehead_modulate_fwd_kernel<4><<<grid, kBlock, 0, st>>>(x, mod, r, C, eps, out); break;
        case 8: spf_posehead_modulate_fwd_kernel<8><<<grid, kBlock, 0, st>>>(x, mod, r, C, eps, out); break;
        default: spf_posehead_modulate_fwd_kernel<16><<<grid, kBlock, 0, st>>>(x, mod, r, C, eps, out); break;
    }
    return hipGetLastError();
}

hipError_t launch_posehead_modulate_bwd(const float* x, const float* mod, const float* dout, int64_t rows, int C, float eps,
                                        float* dx, float* dmod, hipStream_t st) {
    const int grid = ph_row_grid(rows), r = (int)rows;
    switch (ph_vectors_per_lane(C)) {
        case 1: spf_posehead_modulate_bwd_kernel<1><<<grid, kBlock, 0, st>>>(x, mod, dout, r, C, eps, dx, dmod); break;
        case 2: spf_posehead_modulate_bwd_kernel<2><<<grid, kBlock, 0, st>>>(x, mod, dout, r, C, eps, dx, dmod); break;
        case 4: spf_posehead_modulate_bwd_kernel<4><<<grid, kBlock, 0, st>>>(x, mod, dout, r, C, eps, dx, dmod); break;
        case 8: spf_posehead_modulate_bwd_kernel<8><<<grid, kBlock, 0, st>>>(x, mod, dout, r, C, eps, dx, dmod); break;
        default: spf_posehead_modulate_bwd_kernel<16><<<grid, kBlock, 0, st>>>(x, mod, dout, r, C, eps, dx, dmod); break;
    }
    return hipGetLastError();
}

// ---- e. attention over the views ---------------------------------------------------------------------------------------
// qkv [B, S, 3, H, D]: row i of q / k / v of head h of batch item b starts at ((b S + i) 3 + which) H D + h D.
template <int D>
struct alignas(16) PhAttnLds {                       // read and written as 16-byte vectors
    float k[kPhMaxS][D + kPhPad];
    float v[kPhMaxS][D + kPhPad];
    float p[kPhMaxS][kPhMaxS + 1];
    float ds[kPhMaxS][kPhMaxS + 1];
};

__device__ __forceinline__ float ph_dot4(float4 a, float4 b, float acc) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// K and V of the head -> LDS; p = softmax(q k^T scale) (rows sum to 1).  All threads call it.
template <int D>
__device__ __forceinline__ void ph_attn_scores(PhAttnLds<D>& s, const float* __restrict__ base, int S, int64_t tok,
                                               int64_t hd, float scale) {
    constexpr int DV = D / 4;
    for (int i = threadIdx.x; i < S * DV; i += kBlock) {
        const int j = i / DV, d = 4 * (i - j * DV);
        *reinterpret_cast<float4*>(&s.k[j][d]) = *reinterpret_cast<const float4*>(base + j * tok + hd + d);
        *reinterpret_cast<float4*>(&s.v[j][d]) = *reinterpret_cast<const float4*>(base + j * tok + 2 * hd + d);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < S * S; e += kBlock) {
        const int i = e / S, j = e - i * S;
        const float* __restrict__ q = base + i * tok;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
        for (int d = 0; d < D; d += 8) {
            a0 = ph_dot4(*reinterpret_cast<const float4*>(q + d), *reinterpret_cast<const float4*>(&s.k[j][d]), a0);
            a1 = ph_dot4(*reinterpret_cast<const float4*>(q + d + 4), *reinterpret_cast<const float4*>(&s.k[j][d + 4]), a1);
        }
        s.p[i][j] = (a0 + a1) * scale;
    }
    __syncthreads();
    if (threadIdx.x < S) {                                  // a thread per query: at most 32 keys
        const int i = threadIdx.x;
        float m = s.p[i][0];
        for (int j = 1; j < S; ++j) m = fmaxf(m, s.p[i][j]);
        float sum = 0.f;
        for (int j = 0; j < S; ++j) {
            const float e = expf(s.p[i][j] - m);
            s.p[i][j] = e;
            sum += e;
        }
        const float inv = 1.f / sum;
        for (int j = 0; j < S; ++j) s.p[i][j] *= inv;
    }
    __syncthreads();
}

template <int D>
__global__ __launch_bounds__(kBlock) void spf_posehead_attn_fwd_kernel(const float* __restrict__ qkv, int S, int H,
                                                                       float scale, float* __restrict__ out) {
    __shared__ PhAttnLds<D> s;
    constexpr int DV = D / 4;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int64_t hd = (int64_t)H * D, tok = 3 * hd;
    const float* __restrict__ base = qkv + (int64_t)b * S * tok + (int64_t)h * D;
    ph_attn_scores<D>(s, base, S, tok, hd, scale);
    for (int e = threadIdx.x; e < S * DV; e += kBlock) {
        const int i = e / DV, d = 4 * (e - i * DV);
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int j = 0; j < S; ++j) {
            const float w = s.p[i][j];
            const float4 v = *reinterpret_cast<const float4*>(&s.v[j][d]);
            a.x = fmaf(w, v.x, a.x); a.y = fmaf(w, v.y, a.y); a.z = fmaf(w, v.z, a.z); a.w = fmaf(w, v.w, a.w);
        }
        *reinterpret_cast<float4*>(out + ((int64_t)b * S + i) * hd + (int64_t)h * D + d) = a;
    }
}

// dV = P^T dO, dP = dO V^T, dS = P (dP - rowsum(P dP)), dQ = scale dS K, dK = scale dS^T Q
template <int D>
__global__ __launch_bounds__(kBlock) void spf_posehead_attn_bwd_kernel(const float* __restrict__ qkv,
                                                                       const float* __restrict__ dout, int S, int H,
                                                                       float scale, float* __restrict__ dqkv) {
    __shared__ PhAttnLds<D> s;
    constexpr int DV = D / 4;
    const int b = blockIdx.x / H, h = blockIdx.x - b * H;
    const int64_t hd = (int64_t)H * D, tok = 3 * hd;
    const float* __restrict__ base = qkv + (int64_t)b * S * tok + (int64_t)h * D;
    const float* __restrict__ go = dout + (int64_t)b * S * hd + (int64_t)h * D;
    float* __restrict__ gbase = dqkv + (int64_t)b * S * tok + (int64_t)h * D;
    ph_attn_scores<D>(s, base, S, tok, hd, scale);
    for (int e = threadIdx.x; e < S * S; e += kBlock) {           // dP
        const int i = e / S, j = e - i * S;
        const float* __restrict__ g = go + i * hd;
        float a0 = 0.f, a1 = 0.f;
#pragma unroll 4
        for (int d = 0; d < D; d += 8) {
            a0 = ph_dot4(*reinterpret_cast<const float4*>(g + d), *reinterpret_cast<const float4*>(&s.v[j][d]), a0);
            a1 = ph_dot4(*reinterpret_cast<const float4*>(g + d + 4), *reinterpret_cast<const float4*>(&s.v[j][d + 4]), a1);
        }
        s.ds[i][j] = a0 + a1;
    }
    __syncthreads();
    if (threadIdx.x < S) {
        const int i = threadIdx.x;
        float dot = 0.f;
        for (int j = 0; j < S; ++j) dot = fmaf(s.p[i][j], s.ds[i][j], dot);
        for (int j = 0; j < S; ++j) s.ds[i][j] = s.p[i][j] * (s.ds[i][j] - dot) * scale;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < S * DV; e += kBlock) {
        const int i = e / DV, d = 4 * (e - i * DV);               // i: the query of dq, the key of dk and dv
        float4 dq = make_float4(0.f, 0.f, 0.f, 0.f), dk = dq, dv = dq;
        for (int j = 0; j < S; ++j) {
            const float a = s.ds[i][j], c = s.ds[j][i], w = s.p[j][i];
            const float4 kj = *reinterpret_cast<const float4*>(&s.k[j][d]);
            const float4 qj = *reinterpret_cast<const float4*>(base + j * tok + d);
            const float4 gj = *reinterpret_cast<const float4*>(go + j * hd + d);
            dq.x = fmaf(a, kj.x, dq.x); dq.y = fmaf(a, kj.y, dq.y); dq.z = fmaf(a, kj.z, dq.z); dq.w = fmaf(a, kj.w, dq.w);
            dk.x = fmaf(c, qj.x, dk.x); dk.y = fmaf(c, qj.y, dk.y); dk.z = fmaf(c, qj.z, dk.z); dk.w = fmaf(c, qj.w, dk.w);
            dv.x = fmaf(w, gj.x, dv.x); dv.y = fmaf(w, gj.y, dv.y); dv.z = fmaf(w, gj.z, dv.z); dv.w = fmaf(w, gj.w, dv.w);
        }
        float* __restrict__ o = gbase + i * tok + d;
        *reinterpret_cast<float4*>(o) = dq;
        *reinterpret_cast<float4*>(o + hd) = dk;
        *reinterpret_cast<float4*>(o + 2 * hd) = dv;
    }
}

hipError_t launch_posehead_attn_fwd(const float* qkv, int B, int S, int H, int D, float* out, hipStream_t st) {
    const float scale = 1.f / sqrtf((float)D);
    if (D == 64) spf_posehead_attn_fwd_kernel<64><<<B * H, kBlock, 0, st>>>(qkv, S, H, scale, out);
    else spf_posehead_attn_fwd_kernel<128><<<B * H, kBlock, 0, st>>>(qkv, S, H, scale, out);
    return hipGetLastError();
}

hipError_t launch_posehead_attn_bwd(const float* qkv, const float* dout, int B, int S, int H, int D, float* dqkv,
                                    hipStream_t st) {
    const float scale = 1.f / sqrtf((float)D);
    if (D == 64) spf_posehead_attn_bwd_kernel<64><<<B * H, kBlock, 0, st>>>(qkv, dout, S, H, scale, dqkv);
    else spf_posehead_attn_bwd_kernel<128><<<B * H, kBlock, 0, st>>>(qkv, dout, S, H, scale, dqkv);
    return hipGetLastError();
}

// ---- f. accumulate + activate_pose -------------------------------------------------------------------------------------
// act: SPF_POSE_ACT_LINEAR, _INV_LOG (sign(y) expm1(|y|)), _EXP, _RELU
__device__ __forceinline__ float ph_act(float y, int act) {
    switch (act) {
        case SPF_POSE_ACT_INV_LOG: return y == 0.f ? 0.f : copysignf(expm1f(fabsf(y)), y);
        case SPF_POSE_ACT_EXP: return expf(y);
        case SPF_POSE_ACT_RELU: return y > 0.f ? y : 0.f;
        default: return y;
    }
}
__device__ __forceinline__ float ph_act_grad(float y, int act) {
    switch (act) {
        case SPF_POSE_ACT_INV_LOG: return y == 0.f ? 0.f : expf(fabsf(y));      // (sign(0) = 0 takes the gradient with it)
        case SPF_POSE_ACT_EXP: return expf(y);
        case SPF_POSE_ACT_RELU: return y > 0.f ? 1.f : 0.f;
        default: return 1.f;
    }
}
__device__ __forceinline__ int ph_act_of(int k, int trans_act, int quat_act, int fl_act) {
    return k < 3 ? trans_act : k < 7 ? quat_act : fl_act;
}

__global__ __launch_bounds__(kBlock) void spf_posehead_activate_fwd_kernel(const float* __restrict__ prev,
                                                                           const float* __restrict__ delta, int64_t n,
                                                                           int trans_act, int quat_act, int fl_act,
                                                                           float* __restrict__ pred, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const float y = prev ? prev[i] + delta[i] : delta[i];
        pred[i] = y;
        out[i] = ph_act(y, ph_act_of((int)(i % 9), trans_act, quat_act, fl_act));
    }
}

__global__ __launch_bounds__(kBlock) void spf_posehead_activate_bwd_kernel(const float* __restrict__ pred,
                                                                           const float* __restrict__ d_pred,
                                                                           const float* __restrict__ d_out, int64_t n,
                                                                           int trans_act, int quat_act, int fl_act,
                                                                           float* __restrict__ d_delta) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        float g = d_pred ? d_pred[i] : 0.f;
        if (d_out) g = fmaf(d_out[i], ph_act_grad(pred[i], ph_act_of((int)(i % 9), trans_act, quat_act, fl_act)), g);
        d_delta[i] = g;
    }
}

hipError_t launch_posehead_activate_fwd(const float* prev, const float* delta, int64_t rows, int trans_act, int quat_act,
                                        int fl_act, float* pred, float* out, hipStream_t st) {
    spf_posehead_activate_fwd_kernel<<<ph_grid(9 * rows), kBlock, 0, st>>>(prev, delta, 9 * rows, trans_act, quat_act, fl_act,
                                                                          pred, out);
    return hipGetLastError();
}

hipError_t launch_posehead_activate_bwd(const float* pred, const float* d_pred, const float* d_out, int64_t rows,
                                        int trans_act, int quat_act, int fl_act, float* d_delta, hipStream_t st) {
    spf_posehead_activate_bwd_kernel<<<ph_grid(9 * rows), kBlock, 0, st>>>(pred, d_pred, d_out, 9 * rows, trans_act, quat_act,
                                                                          fl_act, d_delta);
    return hipGetLastError();
}

}  // namespace spf
