// The memory-bound work of the DPT heads between their convolutions, for gfx950, float32, NCHW contiguous:
//
//   spf_dpt_up2_fwd_kernel      out[P, 2h, 2w] = up2(x[P, h, w]) (+ skip | + relu(skip)), up2 = torch's bilinear x2 rule
//                               with align_corners=True
//   spf_dpt_up2_bwd_kernel      dx = up2^T(dy) in gather form, and with the ReLU flag dskip = dy * (skip > 0)
//   spf_dpt_add_relu_fwd_kernel s = a + b (+ c), y = relu(s), both written (a alone: y = relu(a), s is a)
//   spf_dpt_add_relu_bwd_kernel g = ds + dy * (mask > 0), the gradient of every addend
//   spf_dpt_points_fwd_kernel   postprocess: [B, C, H, W] -> pts3d [B, H, W, 3] = xyz / max(d, 1e-8) * clip(expm1(d)),
//                               d = |xyz|, and conf [B, H, W] = vmin + min(exp(x), vmax - vmin)
//   spf_dpt_points_bwd_kernel   its backward, recomputed from the saved head output
//
// Replaces, around the nn.Conv2d calls of heads/dpt_block.py:121-142 / 189-218, dpt_gs_head.py:71-73 and
// postprocess.py:11-78, the eager ReLU, add, F.interpolate and permute / norm / clip / div / expm1 / mul kernels.
//
// up2: a block takes chunks of 4,096 items of a plane grid-stride and its threads the items, four output columns per
// lane as one 16-byte store where the output width is a multiple of 4 (w even), one per lane where it is not.  The taps are the
// forward's index formula (tap_of) in both directions: the backward gives every INPUT pixel the window of seven output
// rows and columns 2 i - 3 .. 2 i + 3, a superset of the outputs that read it for every h (src = scale * o with
// scale = (h - 1) / (2 h - 1) in [0, 1/2): an output outside the window is at least 0.2 away in src from reading i),
// and weighs each member of the window by tap_of itself -- l0 where its i0 is i plus l1 where its i1 is i, zero for
// both where it reads neither.  One fixed order of summation, no float atomic: two runs agree bitwise.
// add_relu, points: flat, 16-byte vectors with a scalar tail (add_relu) or a scalar path (points with H W % 4 != 0).
#include <math.h>

#include "spf_common.h"
#include "launchers.h"

namespace spf {

constexpr int kDptMaxGrid = 2048;       // blocks of any launch here; the rest of the work is taken grid-stride

int dpt_max_grid() { return kDptMaxGrid; }

struct Tap {
    int i0, i1;
    float l0, l1;
};
// aten/src/ATen/native/cuda/UpSampleBilinear2d.cu with align_corners: src = scale * dst, i0 = (int)src,
// i1 = i0 + (i0 < in - 1), lambda1 = src - i0, lambda0 = 1 - lambda1
__device__ __forceinline__ Tap tap_of(int o, float scale, int in) {
    const float src = scale * (float)o;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.f - t.l1;
    return t;
}
// the weight with which output o reads input i (0 where it does not)
__device__ __forceinline__ float tap_weight(int o, int i, float scale, int in) {
    const Tap t = tap_of(o, scale, in);
    return (t.i0 == i ? t.l0 : 0.f) + (t.i1 == i ? t.l1 : 0.f);
}
// torch's relu and threshold_backward: a NaN passes through both (NaN <= 0 is false)
__device__ __forceinline__ float relu_f(float v) { return v <= 0.f ? 0.f : v; }
__device__ __forceinline__ float pass_f(float m, float g) { return m <= 0.f ? 0.f : g; }

// A block's unit of work: kUpChunk consecutive items (output vectors or pixels forward, input pixels backward) of one
// plane, so that a few large planes fill the machine as well as many small ones; units are taken grid-stride.
constexpr int kUpChunk = 16 * kBlock;
// ---- x2 upsample (+ skip), forward -----------------------------------------------------------------------------------
// SKIP 0: none; 1: + skip; 2: + relu(skip)
template <int SKIP, bool VEC>
__global__ __launch_bounds__(kBlock) void spf_dpt_up2_fwd_kernel(const float* __restrict__ x,
                                                                 const float* __restrict__ skip, int planes, int h, int w,
                                                                 int chunks, float sy, float sx, float* __restrict__ out) {
    const int H = 2 * h, W = 2 * w;
    const int per_row = VEC ? W / 4 : W;
    const int items = H * per_row;
    const int64_t units = (int64_t)planes * chunks;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int p = (int)(u / chunks), first = (int)(u - (int64_t)p * chunks) * kUpChunk;
        const int last = items - first > kUpChunk ? first + kUpChunk : items;
        const float* __restrict__ xp = x + (int64_t)p * h * w;
        const int64_t ob = (int64_t)p * H * W;
        for (int it = first + threadIdx.x; it < last; it += kBlock) {
            const int oy = it / per_row, v = it - oy * per_row;
            const Tap ty = tap_of(oy, sy, h);
            const float* __restrict__ r0 = xp + ty.i0 * w;
            const float* __restrict__ r1 = xp + ty.i1 * w;
            constexpr int kN = VEC ? 4 : 1;
            const int ox = kN * v;
            float o[kN];
#pragma unroll
            for (int j = 0; j < kN; ++j) {
                const Tap tx = tap_of(ox + j, sx, w);
                o[j] = ty.l0 * (tx.l0 * r0[tx.i0] + tx.l1 * r0[tx.i1]) + ty.l1 * (tx.l0 * r1[tx.i0] + tx.l1 * r1[tx.i1]);
            }
            const int64_t at = ob + (int64_t)oy * W + ox;
            if constexpr (VEC) {
                if constexpr (SKIP != 0) {
                    const float4 s = *reinterpret_cast<const float4*>(skip + at);
                    o[0] += SKIP == 2 ? relu_f(s.x) : s.x; o[1] += SKIP == 2 ? relu_f(s.y) : s.y;
                    o[2] += SKIP == 2 ? relu_f(s.z) : s.z; o[3] += SKIP == 2 ? relu_f(s.w) : s.w;
                }
                *reinterpret_cast<float4*>(out + at) = make_float4(o[0], o[1], o[2], o[3]);
            } else {
                if constexpr (SKIP != 0) o[0] += SKIP == 2 ? relu_f(skip[at]) : skip[at];
                out[at] = o[0];
            }
        }
    }
}

// ---- x2 upsample, backward -------------------------------------------------------------------------------------------
constexpr int kUpWindow = 7;            // outputs 2 i - 3 .. 2 i + 3 per axis
template <bool RELU>
__global__ __launch_bounds__(kBlock) void spf_dpt_up2_bwd_kernel(const float* __restrict__ dy,
                                                                 const float* __restrict__ skip, int planes, int h, int w,
                                                                 int chunks, float sy, float sx, float* __restrict__ dx,
                                                                 float* __restrict__ dskip) {
    const int H = 2 * h, W = 2 * w;
    const int pixels = h * w;
    const int64_t units = (int64_t)planes * chunks;
    for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {
        const int p = (int)(u / chunks), first = (int)(u - (int64_t)p * chunks) * kUpChunk;
        const int last = pixels - first > kUpChunk ? first + kUpChunk : pixels;
        const int64_t ob = (int64_t)p * H * W;
        const float* __restrict__ gp = dy + ob;
        // (dx is null where only skip wants its gradient: no gather then)
        float* __restrict__ dxp = dx ? dx + (int64_t)p * pixels : nullptr;
        for (int it = first + threadIdx.x; dxp != nullptr && it < last; it += kBlock) {
            const int iy = it / w, ix = it - iy * w;
            const int x0 = 2 * ix - 3 > 0 ? 2 * ix - 3 : 0, y0 = 2 * iy - 3 > 0 ? 2 * iy - 3 : 0;
            float wx[kUpWindow];
            int cx[kUpWindow];
#pragma unroll
            for (int k = 0; k < kUpWindow; ++k) {
                const int ox = x0 + k;
                wx[k] = ox < W ? tap_weight(ox, ix, sx, w) : 0.f;
                cx[k] = ox < W ? ox : W - 1;
            }
            float acc = 0.f;
            for (int k = 0; k < kUpWindow; ++k) {
                const int oy = y0 + k;
                if (oy >= H) break;
                const float wy = tap_weight(oy, iy, sy, h);
                if (wy == 0.f) continue;
                const float* __restrict__ row = gp + oy * W;
                float r = 0.f;
#pragma unroll
                for (int j = 0; j < kUpWindow; ++j) r = wx[j] != 0.f ? fmaf(wx[j], row[cx[j]], r) : r;   // (a select: an
                                                                        // output that does not read this pixel may be inf)
                acc = fmaf(wy, r, acc);
            }
            dxp[it] = acc;
        }
        if constexpr (RELU) {
            const float* __restrict__ sp = skip + ob;
            float* __restrict__ dp = dskip + ob;
            for (int it = first + threadIdx.x; it < last; it += kBlock) {    // a plane of 4 h w outputs is h w vectors
                const float4 s = *reinterpret_cast<const float4*>(sp + 4 * it);
                const float4 g = *reinterpret_cast<const float4*>(gp + 4 * it);
                *reinterpret_cast<float4*>(dp + 4 * it) =
                    make_float4(pass_f(s.x, g.x), pass_f(s.y, g.y), pass_f(s.z, g.z), pass_f(s.w, g.w));
            }
        }
    }
}

// ---- add + ReLU ------------------------------------------------------------------------------------------------------
// N addends; s is written for N > 1
template <int N>
__global__ __launch_bounds__(kBlock) void spf_dpt_add_relu_fwd_kernel(const float* __restrict__ a,
                                                                      const float* __restrict__ b,
                                                                      const float* __restrict__ c, int64_t n,
                                                                      float* __restrict__ s, float* __restrict__ y) {
    const int64_t nv = n / 4, tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = tid; i < nv; i += (int64_t)gridDim.x * kBlock) {
        float4 v = reinterpret_cast<const float4*>(a)[i];
        if constexpr (N > 1) {
            const float4 t = reinterpret_cast<const float4*>(b)[i];
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if constexpr (N > 2) {
            const float4 t = reinterpret_cast<const float4*>(c)[i];
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        if constexpr (N > 1) reinterpret_cast<float4*>(s)[i] = v;
        reinterpret_cast<float4*>(y)[i] = make_float4(relu_f(v.x), relu_f(v.y), relu_f(v.z), relu_f(v.w));
    }
    const int64_t t = 4 * nv + tid;                      // the scalar tail: n % 4 elements
    if (t < n) {
        float v = a[t];
        if constexpr (N > 1) v += b[t];
        if constexpr (N > 2) v += c[t];
        if constexpr (N > 1) s[t] = v;
        y[t] = relu_f(v);
    }
}

template <bool HAS_DS>
__global__ __launch_bounds__(kBlock) void spf_dpt_add_relu_bwd_kernel(const float* __restrict__ mask,
                                                                      const float* __restrict__ dy,
                                                                      const float* __restrict__ ds, int64_t n,
                                                                      float* __restrict__ g) {
    const int64_t nv = n / 4, tid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    for (int64_t i = tid; i < nv; i += (int64_t)gridDim.x * kBlock) {
        const float4 m = reinterpret_cast<const float4*>(mask)[i];
        const float4 u = reinterpret_cast<const float4*>(dy)[i];
        float4 o = make_float4(pass_f(m.x, u.x), pass_f(m.y, u.y), pass_f(m.z, u.z), pass_f(m.w, u.w));
        if constexpr (HAS_DS) {
            const float4 t = reinterpret_cast<const float4*>(ds)[i];
            o.x += t.x; o.y += t.y; o.z += t.z; o.w += t.w;
        }
        reinterpret_cast<float4*>(g)[i] = o;
    }
    const int64_t t = 4 * nv + tid;
    if (t < n) {
        float o = pass_f(mask[t], dy[t]);
        if constexpr (HAS_DS) o += ds[t];
        g[t] = o;
    }
}

// ---- points ----------------------------------------------------------------------------------------------------------
struct PointsMode {
    float dmin, dmax;       // bounds of expm1(d) (only with BOUNDS)
    float cmin, cspan;      // conf = cmin + min(exp(x), cspan), cspan = vmax - vmin
};
constexpr float kMinNorm = 1e-8f;   // postprocess.py:48

template <bool BOUNDS>
__device__ __forceinline__ void points_px(float x, float y, float z, const PointsMode& m, float (&o)[3]) {
    const float d = sqrtf(x * x + y * y + z * z);
    const float dc = fmaxf(d, kMinNorm);
    float e = expm1f(d);
    if constexpr (BOUNDS) e = fminf(fmaxf(e, m.dmin), m.dmax);
    o[0] = x / dc * e; o[1] = y / dc * e; o[2] = z / dc * e;
}
// autograd of that expression: out = n e, n = xyz / dc, dc = clip(d, min=1e-8) (passes the gradient where d >= 1e-8),
// e = clip(expm1(d)) (passes it inside the bounds, expm1' = expm1 + 1), d = |xyz| (gradient xyz / d, 0 at d = 0)
template <bool BOUNDS>
__device__ __forceinline__ void points_px_bwd(float x, float y, float z, float gx, float gy, float gz,
                                              const PointsMode& m, float (&o)[3]) {
    const float d = sqrtf(x * x + y * y + z * z);
    const float dc = fmaxf(d, kMinNorm);
    const float eu = expm1f(d);
    float e = eu;
    bool inside = true;
    if constexpr (BOUNDS) {
        e = fminf(fmaxf(eu, m.dmin), m.dmax);
        inside = eu >= m.dmin && eu <= m.dmax;
    }
    const float G = gx * x + gy * y + gz * z;
    const float de = inside ? (G / dc) * (eu + 1.f) : 0.f;          // through e
    const float dd = d >= kMinNorm ? de - (e * G) / (dc * dc) : de; // and through dc
    const float coef = d > 0.f ? dd / d : 0.f;
    const float q = e / dc;
    o[0] = fmaf(coef, x, gx * q); o[1] = fmaf(coef, y, gy * q); o[2] = fmaf(coef, z, gz * q);
}

// in [B, C, HW]: channels 0..2 xyz, 3 the confidence logit (CONF); pts [B, HW, 3], conf [B, HW]
template <bool CONF, bool BOUNDS, bool VEC>
__global__ __launch_bounds__(kBlock) void spf_dpt_points_fwd_kernel(const float* __restrict__ in, int64_t B, int64_t HW,
                                                                    int C, PointsMode m, float* __restrict__ pts,
                                                                    float* __restrict__ conf) {
    constexpr int kN = VEC ? 4 : 1;
    const int64_t per = HW / kN, total = B * per;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = i / per, px = kN * (i - b * per);
        const float* __restrict__ base = in + (b * C) * HW + px;
        float v[4][kN];
#pragma unroll
        for (int ch = 0; ch < (CONF ? 4 : 3); ++ch) {
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(base + ch * HW);
                v[ch][0] = t.x; v[ch][1] = t.y; v[ch][2] = t.z; v[ch][3] = t.w;
            } else {
                v[ch][0] = base[ch * HW];
            }
        }
        float o[3 * kN], cf[kN];
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            float r[3];
            points_px<BOUNDS>(v[0][j], v[1][j], v[2][j], m, r);
            o[3 * j] = r[0]; o[3 * j + 1] = r[1]; o[3 * j + 2] = r[2];
            if constexpr (CONF) cf[j] = m.cmin + fminf(expf(v[3][j]), m.cspan);
        }
        float* __restrict__ po = pts + 3 * (b * HW + px);
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                reinterpret_cast<float4*>(po)[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
            if constexpr (CONF) *reinterpret_cast<float4*>(conf + b * HW + px) = make_float4(cf[0], cf[1], cf[2], cf[3]);
        } else {
            po[0] = o[0]; po[1] = o[1]; po[2] = o[2];
            if constexpr (CONF) conf[b * HW + px] = cf[0];
        }
    }
}

// din [B, C, HW]: channels 0..2 (and 3 with CONF) are written; the caller zeroes any further channel
template <bool CONF, bool BOUNDS, bool VEC>
__global__ __launch_bounds__(kBlock) void spf_dpt_points_bwd_kernel(const float* __restrict__ in,
                                                                    const float* __restrict__ dpts,
                                                                    const float* __restrict__ dconf, int64_t B, int64_t HW,
                                                                    int C, PointsMode m, float* __restrict__ din) {
    constexpr int kN = VEC ? 4 : 1;
    const int64_t per = HW / kN, total = B * per;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        const int64_t b = i / per, px = kN * (i - b * per);
        const float* __restrict__ base = in + (b * C) * HW + px;
        float* __restrict__ dbase = din + (b * C) * HW + px;
        float v[4][kN], g[3 * kN], gc[kN];
#pragma unroll
        for (int ch = 0; ch < (CONF ? 4 : 3); ++ch) {
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(base + ch * HW);
                v[ch][0] = t.x; v[ch][1] = t.y; v[ch][2] = t.z; v[ch][3] = t.w;
            } else {
                v[ch][0] = base[ch * HW];
            }
        }
        const float* __restrict__ gp = dpts + 3 * (b * HW + px);
        if constexpr (VEC) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 t = reinterpret_cast<const float4*>(gp)[k];
                g[4 * k] = t.x; g[4 * k + 1] = t.y; g[4 * k + 2] = t.z; g[4 * k + 3] = t.w;
            }
            if constexpr (CONF) {
                const float4 t = *reinterpret_cast<const float4*>(dconf + b * HW + px);
                gc[0] = t.x; gc[1] = t.y; gc[2] = t.z; gc[3] = t.w;
            }
        } else {
            g[0] = gp[0]; g[1] = gp[1]; g[2] = gp[2];
            if constexpr (CONF) gc[0] = dconf[b * HW + px];
        }
        float d[4][kN];
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            float r[3];
            points_px_bwd<BOUNDS>(v[0][j], v[1][j], v[2][j], g[3 * j], g[3 * j + 1], g[3 * j + 2], m, r);
            d[0][j] = r[0]; d[1][j] = r[1]; d[2][j] = r[2];
            if constexpr (CONF) {
                const float ex = expf(v[3][j]);
                d[3][j] = ex <= m.cspan ? gc[j] * ex : 0.f;
            }
        }
#pragma unroll
        for (int ch = 0; ch < (CONF ? 4 : 3); ++ch) {
            if constexpr (VEC) *reinterpret_cast<float4*>(dbase + ch * HW) = make_float4(d[ch][0], d[ch][1], d[ch][2], d[ch][3]);
            else dbase[ch * HW] = d[ch][0];
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------
static int capped(int64_t want) { return (int)(want < 1 ? 1 : (want < kDptMaxGrid ? want : kDptMaxGrid)); }
static float up_scale(int in) { return in > 1 ? (float)(in - 1) / (float)(2 * in - 1) : 0.f; }
static int up_chunks(int64_t items) { return (int)((items + kUpChunk - 1) / kUpChunk); }

template <int SKIP>
static void up2_fwd_vec(const float* x, const float* skip, int planes, int h, int w, float* out, hipStream_t st) {
    const int chunks = up_chunks(w % 2 == 0 ? (int64_t)2 * h * (w / 2) : (int64_t)4 * h * w);
    const int grid = capped((int64_t)planes * chunks);
    if (w % 2 == 0) spf_dpt_up2_fwd_kernel<SKIP, true><<<grid, kBlock, 0, st>>>(x, skip, planes, h, w, chunks, up_scale(h), up_scale(w), out);
    else spf_dpt_up2_fwd_kernel<SKIP, false><<<grid, kBlock, 0, st>>>(x, skip, planes, h, w, chunks, up_scale(h), up_scale(w), out);
}
hipError_t launch_dpt_up2_fwd(const float* x, const float* skip, int relu_skip, int64_t planes, int h, int w, float* out,
                              hipStream_t st) {
    if (!skip) up2_fwd_vec<0>(x, nullptr, (int)planes, h, w, out, st);
    else if (!relu_skip) up2_fwd_vec<1>(x, skip, (int)planes, h, w, out, st);
    else up2_fwd_vec<2>(x, skip, (int)planes, h, w, out, st);
    return hipGetLastError();
}

hipError_t launch_dpt_up2_bwd(const float* dy, const float* skip, int64_t planes, int h, int w, float* dx, float* dskip,
                              hipStream_t st) {
    const int P = (int)planes, chunks = up_chunks((int64_t)h * w);
    const int grid = capped(planes * chunks);
    const float sy = up_scale(h), sx = up_scale(w);
    if (!skip) spf_dpt_up2_bwd_kernel<false><<<grid, kBlock, 0, st>>>(dy, nullptr, P, h, w, chunks, sy, sx, dx, nullptr);
    else spf_dpt_up2_bwd_kernel<true><<<grid, kBlock, 0, st>>>(dy, skip, P, h, w, chunks, sy, sx, dx, dskip);
    return hipGetLastError();
}

hipError_t launch_dpt_add_relu_fwd(const float* a, const float* b, const float* c, int64_t n, float* s, float* y,
                                   hipStream_t st) {
    const int grid = capped((n / 4 + kBlock - 1) / kBlock);
    if (!b) spf_dpt_add_relu_fwd_kernel<1><<<grid, kBlock, 0, st>>>(a, nullptr, nullptr, n, nullptr, y);
    else if (!c) spf_dpt_add_relu_fwd_kernel<2><<<grid, kBlock, 0, st>>>(a, b, nullptr, n, s, y);
    else spf_dpt_add_relu_fwd_kernel<3><<<grid, kBlock, 0, st>>>(a, b, c, n, s, y);
    return hipGetLastError();
}

hipError_t launch_dpt_add_relu_bwd(const float* mask, const float* dy, const float* ds, int64_t n, float* g,
                                   hipStream_t st) {
    const int grid = capped((n / 4 + kBlock - 1) / kBlock);
    if (ds) spf_dpt_add_relu_bwd_kernel<true><<<grid, kBlock, 0, st>>>(mask, dy, ds, n, g);
    else spf_dpt_add_relu_bwd_kernel<false><<<grid, kBlock, 0, st>>>(mask, dy, nullptr, n, g);
    return hipGetLastError();
}

static bool bounded(float lo, float hi) { return !(lo == -INFINITY && hi == INFINITY); }

template <bool CONF, bool BOUNDS>
static void points_vec(bool fwd, const float* in, const float* dpts, const float* dconf, int64_t B, int64_t HW, int C,
                       const PointsMode& m, float* pts, float* conf, float* din, hipStream_t st) {
    const bool vec = HW % 4 == 0;
    const int grid = capped((B * (vec ? HW / 4 : HW) + kBlock - 1) / kBlock);
    if (fwd) {
        if (vec) spf_dpt_points_fwd_kernel<CONF, BOUNDS, true><<<grid, kBlock, 0, st>>>(in, B, HW, C, m, pts, conf);
        else spf_dpt_points_fwd_kernel<CONF, BOUNDS, false><<<grid, kBlock, 0, st>>>(in, B, HW, C, m, pts, conf);
    } else {
        if (vec) spf_dpt_points_bwd_kernel<CONF, BOUNDS, true><<<grid, kBlock, 0, st>>>(in, dpts, dconf, B, HW, C, m, din);
        else spf_dpt_points_bwd_kernel<CONF, BOUNDS, false><<<grid, kBlock, 0, st>>>(in, dpts, dconf, B, HW, C, m, din);
    }
}

// one dispatch for both directions: fwd writes pts (and conf), the backward din
hipError_t launch_dpt_points(int fwd, const float* in, const float* dpts, const float* dconf, int64_t B, int64_t HW,
                             int C, int has_conf, float dmin, float dmax, float cmin, float cmax, float* pts, float* conf,
                             float* din, hipStream_t st) {
    const PointsMode m{dmin, dmax, cmin, cmax - cmin};
    const bool bounds = bounded(dmin, dmax);
    if (has_conf) {
        if (bounds) points_vec<true, true>(fwd != 0, in, dpts, dconf, B, HW, C, m, pts, conf, din, st);
        else points_vec<true, false>(fwd != 0, in, dpts, dconf, B, HW, C, m, pts, conf, din, st);
    } else {
        if (bounds) points_vec<false, true>(fwd != 0, in, dpts, dconf, B, HW, C, m, pts, conf, din, st);
        else points_vec<false, false>(fwd != 0, in, dpts, dconf, B, HW, C, m, pts, conf, din, st);
    }
    return hipGetLastError();
}

}  // namespace spf
