// LPIPS (VGG16, lpips 0.1 `net="vgg"`, evaluation mode) for batches of image pairs on gfx950: value and gradients.
//
// For in0, in1 [N,3,H,W] the 2N images run the VGG16 trunk up to relu5_3 as ONE batch (in0's images first), the head
// compares the five taps of image n with those of image N + n.  Activations are channels-last ([image, y, x, channel]
// float32), so that the K index of the implicit GEMM (9 taps x C_in) is contiguous per tap and a pixel's feature vector
// is one contiguous run for the head.
//
//   spf_lpips_conv1_kernel      first layer (3 -> 64, K = 27) on the vector ALU: reads the caller's [N,3,H,W] image,
//                               applies `2x - 1` and the scaling layer at the load; outside the image the tile is 0 (the
//                               zero padding comes AFTER the scaling step), bias + ReLU, channels-last out
//   spf_lpips_conv_kernel<BN>   3x3 convolution as an implicit GEMM on v_mfma_f32_32x32x2_f32: M = pixels of the whole
//                               batch (128 per block), N = output channels (BN = 64 or 128 per block), K = 9 x C_in in
//                               steps of 16 channels of one tap.  Four waves as 2 (M) x 2 (N), 2 x BN/64 accumulator
//                               tiles of 32 x 32 each.  The next K step's global loads are in flight while the MFMAs of
//                               the current one run out of LDS.  Epilogue: bias, ReLU.  float32 in, float32 accumulate:
//                               every output is the sum of nine k-ordered fmaf chains, one per tap (C_in products each).
//                               The same kernel is the backward-data pass:
//                               second weight pack (taps rotated by 180 degrees, channels swapped), no bias, no ReLU,
//                               and the incoming gradient is masked AT THE LOAD by the saved activation of the layer it
//                               leaves (`mask` > 0).
//   spf_lpips_conv1_bwd_kernel  backward-data of the first layer into the caller's [N,3,H,W] gradient, with d(scaling)/dx
//   spf_lpips_pool_kernel       2x2 stride-2 max pool (floor mode)
//   spf_lpips_pool_bwd_kernel   routes a pooled gradient to the first maximum (row-major) of its window, recomputed from
//                               the saved activation, and ADDS it to the head's gradient already in the buffer
//   spf_lpips_head_kernel       one wave per pixel: both norms, d_k, block partials (one float per 64 pixels)
//   spf_lpips_head_sum_kernel   one block per image: the partials of every tap in a fixed order (float64) -> out[n]
//   spf_lpips_mean_kernel       weight * mean_n out[n], fixed order
//   spf_lpips_head_bwd_kernel   dL/da and / or dL/db of one tap; the upstream gradient is read on the device.  Where a
//                               feature vector is all zero the 1 / ||a|| term is taken as 0 (autograd gives NaN there).
// No atomics anywhere: results are run-to-run identical and an image's numbers do not depend on its batch.
#include "point_slots.h"
#include "launchers.h"

namespace spf {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kLpLayers = 13, kLpTaps = 5;
static const int kLpCin[kLpLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
static const int kLpCout[kLpLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
static const int kLpLevel[kLpLayers] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
static const int kLpTapLayer[kLpTaps] = {1, 3, 6, 9, 12};
static const int kLpTapC[kLpTaps] = {64, 128, 256, 512, 512};
constexpr int kHeadPix = 64;               // pixels per block of the head kernels (16 per wave)

// floats before layer l in a weight pack (both packs: 9 x C_in x C_out per layer) and in the bias vector
size_t lpips_pack_offset(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += (size_t)9 * kLpCin[i] * kLpCout[i];
    return o;
}
static size_t lpips_bias_offset(int l) {
    size_t o = 0;
    for (int i = 0; i < l; ++i) o += kLpCout[i];
    return o;
}
static size_t lpips_lin_offset(int k) {
    size_t o = 0;
    for (int i = 0; i < k; ++i) o += kLpTapC[i];
    return o;
}

// Workspace layout, in floats.  The forward's part comes first and does not depend on n_grad.
struct LpipsLayout {
    int h[kLpTaps], w[kLpTaps];
    size_t act[kLpLayers];        // activation of layer l, all n_total images
    size_t pool;                  // the pooled input of the current block (scratch)
    size_t partial[kLpTaps];      // head partials of tap k: [N][nblk[k]]
    int nblk[kLpTaps];
    size_t gtap[kLpTaps];         // gradient at tap k (n_grad images): the head's, then plus the routed pool gradient
    size_t gbuf[2];               // ping-pong for the backward-data outputs
    size_t total;
};
static size_t align64(size_t v) { return (v + 63) & ~(size_t)63; }
LpipsLayout lpips_layout(int n_grad, int n_total, int H, int W) {
    LpipsLayout L;
    for (int k = 0; k < kLpTaps; ++k) {
        L.h[k] = H >> k;
        L.w[k] = W >> k;
    }
    size_t o = 0;
    for (int l = 0; l < kLpLayers; ++l) {
        const int k = kLpLevel[l];
        L.act[l] = o;
        o = align64(o + (size_t)n_total * L.h[k] * L.w[k] * kLpCout[l]);
    }
    L.pool = o;
    o = align64(o + (size_t)n_total * L.h[1] * L.w[1] * 64);      // the largest pooled map
    for (int k = 0; k < kLpTaps; ++k) {
        L.nblk[k] = (L.h[k] * L.w[k] + kHeadPix - 1) / kHeadPix;
        L.partial[k] = o;
        o = align64(o + (size_t)(n_total / 2) * L.nblk[k]);
    }
    for (int k = 0; k < kLpTaps; ++k) {
        L.gtap[k] = o;
        o = align64(o + (size_t)n_grad * L.h[k] * L.w[k] * kLpTapC[k]);
    }
    for (int i = 0; i < 2; ++i) {
        L.gbuf[i] = o;
        o = align64(o + (size_t)n_grad * H * W * 64);
    }
    L.total = o;
    return L;
}
int64_t lpips_workspace_bytes(int n_grad, int n_total, int H, int W) {
    return (int64_t)(lpips_layout(n_grad, n_total, H, W).total * sizeof(float));
}

// ---- first layer ---------------------------------------------------------------------------------------------------
// Four lanes per pixel, sixteen output channels each.  wf: [27][64] (k = tap * 3 + channel), sc: shift[3], scale[3].
__global__ __launch_bounds__(kBlock) void spf_lpips_conv1_kernel(const float* __restrict__ in0, int64_t stride0,
                                                                 const float* __restrict__ in1, int64_t stride1, int n0,
                                                                 int n_img, int H, int W, int normalize,
                                                                 const float* __restrict__ wf,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ sc, float* __restrict__ out) {
    __shared__ float s_w[27 * 64];
    for (int i = threadIdx.x; i < 27 * 64; i += kBlock) s_w[i] = wf[i];
    __syncthreads();
    const int64_t HW = (int64_t)H * W, idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t p = idx >> 2;
    const int g = (int)(idx & 3);
    if (p >= n_img * HW) return;
    const int img = (int)(p / HW);
    const int r = (int)(p - img * HW), y = r / W, x = r - y * W;
    const float* __restrict__ src = img < n0 ? in0 + img * stride0 : in1 + (img - n0) * stride1;
    float v[27];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int sy = y + dy - 1, sx = x + dx - 1;
            const bool in = sy >= 0 && sy < H && sx >= 0 && sx < W;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float t = 0.f;
                if (in) {
                    t = src[c * HW + (int64_t)sy * W + sx];
                    if (normalize) t = 2.f * t - 1.f;
                    t = (t - sc[c]) / sc[3 + c];
                }
                v[(dy * 3 + dx) * 3 + c] = t;
            }
        }
    float acc[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const float* __restrict__ w = s_w + k * 64 + g * 16;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = fmaf(v[k], w[j], acc[j]);
    }
    float* __restrict__ o = out + p * 64 + g * 16;
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
        f4a q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q[e] = fmaxf(acc[j + e] + bias[g * 16 + j + e], 0.f);
        *reinterpret_cast<f4a*>(o + j) = q;
    }
}

// One lane per pixel.  g, act: [n_img,H,W,64]; wb: [9][64][3] (the backward pack of layer 0); the gradient of local
// image j goes to d0 + j * 3HW for j < n0, else to d1 + (j - n0) * 3HW.
__global__ __launch_bounds__(kBlock) void spf_lpips_conv1_bwd_kernel(const float* __restrict__ g,
                                                                     const float* __restrict__ act, int n_img, int H,
                                                                     int W, int normalize, const float* __restrict__ wb,
                                                                     const float* __restrict__ sc, float* __restrict__ d0,
                                                                     int n0, float* __restrict__ d1) {
    __shared__ float s_w[9 * 64 * 3];
    for (int i = threadIdx.x; i < 9 * 64 * 3; i += kBlock) s_w[i] = wb[i];
    __syncthreads();
    const int64_t HW = (int64_t)H * W, p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_img * HW) return;
    const int img = (int)(p / HW);
    const int r = (int)(p - img * HW), y = r / W, x = r - y * W;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int dy = 0; dy < 3; ++dy)
        for (int dx = 0; dx < 3; ++dx) {
            const int sy = y + dy - 1, sx = x + dx - 1;
            if (sy < 0 || sy >= H || sx < 0 || sx >= W) continue;
            const int64_t o = (img * HW + (int64_t)sy * W + sx) * 64;
            const float* __restrict__ w = s_w + (dy * 3 + dx) * 64 * 3;
#pragma unroll 4
            for (int c4 = 0; c4 < 16; ++c4) {
                const f4a gv = *reinterpret_cast<const f4a*>(g + o + 4 * c4);
                const f4a av = *reinterpret_cast<const f4a*>(act + o + 4 * c4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float gm = av[e] > 0.f ? gv[e] : 0.f;
                    const float* __restrict__ wk = w + (4 * c4 + e) * 3;
                    acc[0] = fmaf(gm, wk[0], acc[0]);
                    acc[1] = fmaf(gm, wk[1], acc[1]);
                    acc[2] = fmaf(gm, wk[2], acc[2]);
                }
            }
        }
    float* __restrict__ d = img < n0 ? d0 + (int64_t)img * 3 * HW : d1 + (int64_t)(img - n0) * 3 * HW;
    const float f = normalize ? 2.f : 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c * HW + r] = f * (acc[c] / sc[3 + c]);
}

// ---- 3x3 convolution as an implicit GEMM on the float32 matrix instruction ----------------------------------------
constexpr int kConvBM = 128, kConvBK = 16;
constexpr int kConvLdA = kConvBM + 4;      // k-major A image: a lane's four k rows land 16 banks apart, 16 pixels wide

template <int BN>
__global__ __launch_bounds__(kBlock) void spf_lpips_conv_kernel(const float* __restrict__ in,
                                                                const float* __restrict__ mask,
                                                                const float* __restrict__ wpack,
                                                                const float* __restrict__ bias, float* __restrict__ out,
                                                                int n_img, int H, int W, int Cin, int Cout, int relu) {
    constexpr int NT = BN / 64;            // accumulator tiles per wave along N
    constexpr int BV = BN / 64;            // float4 of the B tile per lane (16 x BN floats over 256 lanes)
    __shared__ float s_a[kConvBK * kConvLdA];
    __shared__ float s_b[kConvBK * BN];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int64_t HW = (int64_t)H * W, M = n_img * HW, m0 = (int64_t)blockIdx.x * kConvBM;
    const int n0 = blockIdx.y * BN;

    // the two (pixel, four-channel group) pieces of the A tile this lane stages in every step
    int py[2], px[2];
    int64_t pbase[2];
    bool pok[2];
    const int q = tid & 3;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int64_t p = m0 + (tid >> 2) + 64 * r;
        pok[r] = p < M;
        const int64_t pc = pok[r] ? p : 0;
        const int img = (int)(pc / HW);
        const int rem = (int)(pc - img * HW);
        py[r] = rem / W;
        px[r] = rem - py[r] * W;
        pbase[r] = pc;
    }
    const int nci = Cin / kConvBK, niter = 9 * nci;
    f4a ra[2], rb[BV];
    auto load = [&](int it) {
        const int tap = it / nci, c0 = (it - tap * nci) * kConvBK;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int sy = py[r] + dy, sx = px[r] + dx;
            const bool ok = pok[r] && sy >= 0 && sy < H && sx >= 0 && sx < W;
            f4a v = {0.f, 0.f, 0.f, 0.f};
            if (ok) {
                const int64_t o = (pbase[r] + (int64_t)dy * W + dx) * Cin + c0 + 4 * q;
                v = *reinterpret_cast<const f4a*>(in + o);
                if (mask) {
                    const f4a mv = *reinterpret_cast<const f4a*>(mask + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = mv[e] > 0.f ? v[e] : 0.f;
                }
            }
            ra[r] = v;
        }
#pragma unroll
        for (int r = 0; r < BV; ++r) {
            const int i = tid + kBlock * r, k = i / (BN / 4), c4 = i - k * (BN / 4);
            rb[r] = *reinterpret_cast<const f4a*>(wpack + ((int64_t)tap * Cin + c0 + k) * Cout + n0 + 4 * c4);
        }
    };
    // acc: the fmaf chain of the current tap (C_in products); tot: the sum of the finished taps.  One chain over all of
    // K = 9 x C_in (4,608 products in blocks 4 and 5) measured 9.7 x the error of the host's blocked float32 sum at the
    // production sizes; nine chains of C_in and their sum stay inside twice that.
    f16v acc[2][NT], tot[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = tot[i][j][e] = 0.f;

    load(0);
    const int kl = lane >> 5, il = lane & 31;
    for (int it = 0; it < niter; ++it) {
        __syncthreads();                                   // the previous step's readers are done
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int e = 0; e < 4; ++e) s_a[(4 * q + e) * kConvLdA + (tid >> 2) + 64 * r] = ra[r][e];
#pragma unroll
        for (int r = 0; r < BV; ++r) *reinterpret_cast<f4a*>(s_b + 4 * (tid + kBlock * r)) = rb[r];
        __syncthreads();
        if (it + 1 < niter) load(it + 1);                  // in flight under the MFMAs below
#pragma unroll
        for (int kk = 0; kk < kConvBK; kk += 2) {
            float a[2], b[NT];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = s_a[(kk + kl) * kConvLdA + wm * 64 + i * 32 + il];
#pragma unroll
            for (int j = 0; j < NT; ++j) b[j] = s_b[(kk + kl) * BN + wn * (BN / 2) + j * 32 + il];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if ((it + 1) % nci == 0) {                         // the tap is complete
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        tot[i][j][e] += acc[i][j][e];
                        acc[i][j][e] = 0.f;
                    }
        }
    }
    // C/D map of the 32 x 32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int co = n0 + wn * (BN / 2) + j * 32 + il;
        const float bv = bias ? bias[co] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int64_t p = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kl;
                if (p < M) {
                    float v = tot[i][j][e] + bv;
                    if (relu) v = fmaxf(v, 0.f);
                    out[p * Cout + co] = v;
                }
            }
    }
}

// ---- pool ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void spf_lpips_pool_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                int n_img, int H, int W, int C) {
    const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
    const int64_t total = (int64_t)n_img * Ho * Wo * C4, i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const int64_t po = i / C4;
    const int xo = (int)(po % Wo);
    const int64_t t = po / Wo;
    const int yo = (int)(t % Ho), img = (int)(t / Ho);
    const float* __restrict__ s = in + (((int64_t)img * H + 2 * yo) * W + 2 * xo) * C + 4 * c4;
    const f4a a = *reinterpret_cast<const f4a*>(s), b = *reinterpret_cast<const f4a*>(s + C);
    const f4a c = *reinterpret_cast<const f4a*>(s + (int64_t)W * C), d = *reinterpret_cast<const f4a*>(s + (int64_t)W * C + C);
    f4a m;
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = fmaxf(fmaxf(a[e], b[e]), fmaxf(c[e], d[e]));
    *reinterpret_cast<f4a*>(out + po * C + 4 * c4) = m;
}

// inout[img,y,x,c] += gp[img,y/2,x/2,c] where (y, x) is the first maximum (row-major) of its window of `act`
__global__ __launch_bounds__(kBlock) void spf_lpips_pool_bwd_kernel(const float* __restrict__ gp,
                                                                    const float* __restrict__ act,
                                                                    float* __restrict__ inout, int n_img, int H, int W,
                                                                    int C) {
    const int Ho = H >> 1, Wo = W >> 1, C4 = C >> 2;
    const int64_t total = (int64_t)n_img * Ho * Wo * C4, i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total) return;
    const int c4 = (int)(i % C4);
    const int64_t po = i / C4;
    const int xo = (int)(po % Wo);
    const int64_t t = po / Wo;
    const int yo = (int)(t % Ho), img = (int)(t / Ho);
    const int64_t o00 = (((int64_t)img * H + 2 * yo) * W + 2 * xo) * C + 4 * c4;
    const int64_t off[4] = {o00, o00 + C, o00 + (int64_t)W * C, o00 + (int64_t)W * C + C};
    f4a v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const f4a*>(act + off[j]);
    const f4a gv = *reinterpret_cast<const f4a*>(gp + po * C + 4 * c4);
    int arg[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        int a = 0;
        float m = v[0][e];
#pragma unroll
        for (int j = 1; j < 4; ++j)
            if (v[j][e] > m) {
                m = v[j][e];
                a = j;
            }
        arg[e] = a;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f4a o = *reinterpret_cast<const f4a*>(inout + off[j]);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += arg[e] == j ? gv[e] : 0.f;
        *reinterpret_cast<f4a*>(inout + off[j]) = o;
    }
}

// ---- head ----------------------------------------------------------------------------------------------------------
// fa, fb: [N,HW,C] channels-last features of the two images of every pair.  grid (nblk, N).
template <int CPL>
__global__ __launch_bounds__(kBlock) void spf_lpips_head_kernel(const float* __restrict__ fa, const float* __restrict__ fb,
                                                                const float* __restrict__ lin, int HW, int nblk,
                                                                float* __restrict__ partial) {
    constexpr int C = CPL * 64;
    __shared__ SumRow<1> s_sum;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y;
    float l[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) l[j] = lin[lane + 64 * j];
    float accw = 0.f;
    for (int i = 0; i < kHeadPix / 4; ++i) {
        const int pix = blockIdx.x * kHeadPix + wave * (kHeadPix / 4) + i;
        if (pix >= HW) break;                              // (the same for the whole wave)
        const int64_t o = ((int64_t)n * HW + pix) * C + lane;
        float a[CPL], b[CPL], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            a[j] = fa[o + 64 * j];
            b[j] = fb[o + 64 * j];
            sa = fmaf(a[j], a[j], sa);
            sb = fmaf(b[j], b[j], sb);
        }
        const float da = sqrtf(wave_sum(sa)) + 1e-10f, db = sqrtf(wave_sum(sb)) + 1e-10f;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            const float t = a[j] / da - b[j] / db;
            d = fmaf(l[j] * t, t, d);
        }
        accw += wave_sum(d);
    }
    // accw is a wave total already (the same in every lane), so the row is filled here and not by block_sum; it is
    // written once per block: nobody reads it before this write
    if (lane == 0) s_sum.w[wave][0] = __float_as_uint(accw);
    __syncthreads();
    if (threadIdx.x == 0) partial[(int64_t)n * nblk + blockIdx.x] = sum_row_f32(s_sum, 0);
}

struct LpipsHeadTaps {
    int ntap;
    int nblk[kLpTaps];
    int64_t off[kLpTaps];          // floats from `partial` to tap k's [N][nblk]
    double inv_hw[kLpTaps];
};

__global__ __launch_bounds__(kBlock) void spf_lpips_head_sum_kernel(const float* __restrict__ partial, LpipsHeadTaps t,
                                                                    float* __restrict__ out) {
    __shared__ double s_d[kBlock];
    const int n = blockIdx.x;
    double tot = 0.0;
    for (int k = 0; k < t.ntap; ++k) {
        const float* __restrict__ p = partial + t.off[k] + (int64_t)n * t.nblk[k];
        double acc = 0.0;
        for (int i = threadIdx.x; i < t.nblk[k]; i += kBlock) acc += (double)p[i];
        tot += block_tree_sum<kBlock>(acc, s_d) * t.inv_hw[k];
    }
    if (threadIdx.x == 0) out[n] = (float)tot;
}

__global__ __launch_bounds__(kBlock) void spf_lpips_mean_kernel(const float* __restrict__ out, int N, float weight,
                                                                float* __restrict__ mean) {
    __shared__ double s_d[kBlock];
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += kBlock) acc += (double)out[i];
    const double tot = block_tree_sum<kBlock>(acc, s_d);
    if (threadIdx.x == 0) mean[0] = (float)((double)weight * (tot / (double)N));
}

// dA, dB: [N,HW,C] or null.  Upstream of pair n: up[n], or with `is_mean` up[0] * mean_scale (= weight / N).
template <int CPL>
__global__ __launch_bounds__(kBlock) void spf_lpips_head_bwd_kernel(const float* __restrict__ fa,
                                                                    const float* __restrict__ fb,
                                                                    const float* __restrict__ lin, int HW,
                                                                    const float* __restrict__ up, int is_mean,
                                                                    float mean_scale, float* __restrict__ dA,
                                                                    float* __restrict__ dB) {
    constexpr int C = CPL * 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = blockIdx.y;
    const float s = (is_mean ? up[0] * mean_scale : up[n]) / (float)HW;
    float l[CPL];
#pragma unroll
    for (int j = 0; j < CPL; ++j) l[j] = lin[lane + 64 * j];
    for (int i = 0; i < kHeadPix / 4; ++i) {
        const int pix = blockIdx.x * kHeadPix + wave * (kHeadPix / 4) + i;
        if (pix >= HW) break;
        const int64_t o = ((int64_t)n * HW + pix) * C + lane;
        float a[CPL], b[CPL], sa = 0.f, sb = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            a[j] = fa[o + 64 * j];
            b[j] = fb[o + 64 * j];
            sa = fmaf(a[j], a[j], sa);
            sb = fmaf(b[j], b[j], sb);
        }
        const float na = sqrtf(wave_sum(sa)), nb = sqrtf(wave_sum(sb));
        const float da = na + 1e-10f, db = nb + 1e-10f;
        float g[CPL], ga = 0.f, gb = 0.f;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
            g[j] = 2.f * l[j] * (a[j] / da - b[j] / db) * s;
            ga = fmaf(g[j], a[j], ga);
            gb = fmaf(g[j], b[j], gb);
        }
        if (dA) {
            const float t = wave_sum(ga);
            const float ka = na > 0.f ? t / (da * da * na) : 0.f;
#pragma unroll
            for (int j = 0; j < CPL; ++j) dA[o + 64 * j] = g[j] / da - ka * a[j];
        }
        if (dB) {
            const float t = wave_sum(gb);
            const float kb = nb > 0.f ? t / (db * db * nb) : 0.f;
#pragma unroll
            for (int j = 0; j < CPL; ++j) dB[o + 64 * j] = kb * b[j] - g[j] / db;
        }
    }
}

// ---- launches ------------------------------------------------------------------------------------------------------
static int blocks_for(int64_t items) { return (int)((items + kBlock - 1) / kBlock); }

hipError_t launch_lpips_conv(const float* in, const float* mask, const float* wpack, const float* bias, float* out,
                             int n_img, int H, int W, int Cin, int Cout, int relu, hipStream_t stream) {
    const int64_t M = (int64_t)n_img * H * W;
    const int mb = (int)((M + kConvBM - 1) / kConvBM);
    if (Cout % 128 == 0)
        spf_lpips_conv_kernel<128><<<dim3(mb, Cout / 128), kBlock, 0, stream>>>(in, mask, wpack, bias, out, n_img, H, W,
                                                                                Cin, Cout, relu);
    else
        spf_lpips_conv_kernel<64><<<dim3(mb, Cout / 64), kBlock, 0, stream>>>(in, mask, wpack, bias, out, n_img, H, W,
                                                                              Cin, Cout, relu);
    return hipGetLastError();
}

hipError_t launch_lpips_conv1(const SpfLpips& a, int n_img, float* out, hipStream_t stream) {
    const int64_t items = (int64_t)n_img * a.H * a.W * 4;
    spf_lpips_conv1_kernel<<<blocks_for(items), kBlock, 0, stream>>>(a.in0, a.stride0, a.in1, a.stride1, a.N, n_img, a.H,
                                                                     a.W, a.normalize, a.wfwd, a.bias, a.shift_scale, out);
    return hipGetLastError();
}

hipError_t launch_lpips_conv1_bwd(const SpfLpips& a, const float* g, const float* act, int n_img, float* d0, int n0,
                                  float* d1, hipStream_t stream) {
    spf_lpips_conv1_bwd_kernel<<<blocks_for((int64_t)n_img * a.H * a.W), kBlock, 0, stream>>>(
        g, act, n_img, a.H, a.W, a.normalize, a.wbwd, a.shift_scale, d0, n0, d1);
    return hipGetLastError();
}

hipError_t launch_lpips_pool(const float* in, float* out, int n_img, int H, int W, int C, hipStream_t stream) {
    const int64_t items = (int64_t)n_img * (H / 2) * (W / 2) * (C / 4);
    if (items > 0) spf_lpips_pool_kernel<<<blocks_for(items), kBlock, 0, stream>>>(in, out, n_img, H, W, C);
    return hipGetLastError();
}

hipError_t launch_lpips_pool_bwd(const float* gp, const float* act, float* inout, int n_img, int H, int W, int C,
                                 hipStream_t stream) {
    const int64_t items = (int64_t)n_img * (H / 2) * (W / 2) * (C / 4);
    if (items > 0) spf_lpips_pool_bwd_kernel<<<blocks_for(items), kBlock, 0, stream>>>(gp, act, inout, n_img, H, W, C);
    return hipGetLastError();
}

hipError_t launch_lpips_head(const float* fa, const float* fb, const float* lin, int N, int HW, int C, float* partial,
                             hipStream_t stream) {
    const int nblk = (HW + kHeadPix - 1) / kHeadPix;
    const dim3 grid(nblk, N);
    switch (C) {
        case 64: spf_lpips_head_kernel<1><<<grid, kBlock, 0, stream>>>(fa, fb, lin, HW, nblk, partial); break;
        case 128: spf_lpips_head_kernel<2><<<grid, kBlock, 0, stream>>>(fa, fb, lin, HW, nblk, partial); break;
        case 256: spf_lpips_head_kernel<4><<<grid, kBlock, 0, stream>>>(fa, fb, lin, HW, nblk, partial); break;
        case 512: spf_lpips_head_kernel<8><<<grid, kBlock, 0, stream>>>(fa, fb, lin, HW, nblk, partial); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_lpips_head_bwd(const float* fa, const float* fb, const float* lin, int N, int HW, int C,
                                 const float* up, int is_mean, float mean_scale, float* dA, float* dB,
                                 hipStream_t stream) {
    const dim3 grid((HW + kHeadPix - 1) / kHeadPix, N);
#define SPF_LP_HB(CPL) \
    spf_lpips_head_bwd_kernel<CPL><<<grid, kBlock, 0, stream>>>(fa, fb, lin, HW, up, is_mean, mean_scale, dA, dB)
    switch (C) {
        case 64: SPF_LP_HB(1); break;
        case 128: SPF_LP_HB(2); break;
        case 256: SPF_LP_HB(4); break;
        case 512: SPF_LP_HB(8); break;
        default: return hipErrorInvalidValue;
    }
#undef SPF_LP_HB
    return hipGetLastError();
}

// One tap's term per pair: the head kernel and the fixed-order sum (the building block the tests drive).
hipError_t launch_lpips_head_single(const float* fa, const float* fb, const float* lin, int N, int HW, int C,
                                    float* partial, float* out, hipStream_t stream) {
    if (hipError_t e = launch_lpips_head(fa, fb, lin, N, HW, C, partial, stream)) return e;
    LpipsHeadTaps t = {};
    t.ntap = 1;
    t.nblk[0] = (HW + kHeadPix - 1) / kHeadPix;
    t.off[0] = 0;
    t.inv_hw[0] = 1.0 / (double)HW;
    spf_lpips_head_sum_kernel<<<N, kBlock, 0, stream>>>(partial, t, out);
    return hipGetLastError();
}

#define SPF_LP_TRY(expr)                       \
    do {                                       \
        if (hipError_t e_ = (expr)) return e_; \
    } while (0)

hipError_t launch_lpips_fwd(const SpfLpips& a, float* ws, float* out, float* mean, hipStream_t stream) {
    const int nt = 2 * a.N;
    const LpipsLayout L = lpips_layout(0, nt, a.H, a.W);
    SPF_LP_TRY(launch_lpips_conv1(a, nt, ws + L.act[0], stream));
    for (int l = 1; l < kLpLayers; ++l) {
        const int k = kLpLevel[l];
        const float* src = ws + L.act[l - 1];
        if (kLpLevel[l - 1] != k) {
            SPF_LP_TRY(launch_lpips_pool(src, ws + L.pool, nt, L.h[k - 1], L.w[k - 1], kLpCin[l], stream));
            src = ws + L.pool;
        }
        SPF_LP_TRY(launch_lpips_conv(src, nullptr, a.wfwd + lpips_pack_offset(l), a.bias + lpips_bias_offset(l),
                                     ws + L.act[l], nt, L.h[k], L.w[k], kLpCin[l], kLpCout[l], 1, stream));
    }
    LpipsHeadTaps t = {};
    t.ntap = kLpTaps;
    for (int k = 0; k < kLpTaps; ++k) {
        const int hw = L.h[k] * L.w[k], C = kLpTapC[k];
        const float* f = ws + L.act[kLpTapLayer[k]];
        SPF_LP_TRY(launch_lpips_head(f, f + (size_t)a.N * hw * C, a.lin + lpips_lin_offset(k), a.N, hw, C,
                                     ws + L.partial[k], stream));
        t.nblk[k] = L.nblk[k];
        t.off[k] = (int64_t)(L.partial[k] - L.partial[0]);
        t.inv_hw[k] = 1.0 / (double)hw;
    }
    spf_lpips_head_sum_kernel<<<a.N, kBlock, 0, stream>>>(ws + L.partial[0], t, out);
    if (mean) spf_lpips_mean_kernel<<<1, kBlock, 0, stream>>>(out, a.N, a.weight, mean);
    return hipGetLastError();
}

hipError_t launch_lpips_bwd(const SpfLpips& a, float* ws, const float* up, int is_mean, float* d0, float* d1,
                            hipStream_t stream) {
    const int nt = 2 * a.N;
    const int gs = d0 ? 0 : a.N, ng = (d0 && d1) ? nt : a.N;       // the images that go through the backward trunk
    const LpipsLayout L = lpips_layout(ng, nt, a.H, a.W);
    for (int k = 0; k < kLpTaps; ++k) {
        const int hw = L.h[k] * L.w[k], C = kLpTapC[k];
        const float* f = ws + L.act[kLpTapLayer[k]];
        float* g = ws + L.gtap[k];
        SPF_LP_TRY(launch_lpips_head_bwd(f, f + (size_t)a.N * hw * C, a.lin + lpips_lin_offset(k), a.N, hw, C, up,
                                         is_mean, a.weight / (float)a.N, d0 ? g : nullptr,
                                         d1 ? g + (size_t)(a.N - gs) * hw * C : nullptr, stream));
    }
    const float* g = ws + L.gtap[kLpTaps - 1];
    int tap = kLpTaps - 1;
    for (int l = kLpLayers - 1; l >= 1; --l) {
        const int k = kLpLevel[l];
        const size_t hw = (size_t)L.h[k] * L.w[k];
        float* o = ws + L.gbuf[g == ws + L.gbuf[0] ? 1 : 0];
        SPF_LP_TRY(launch_lpips_conv(g, ws + L.act[l] + (size_t)gs * hw * kLpCout[l], a.wbwd + lpips_pack_offset(l),
                                     nullptr, o, ng, L.h[k], L.w[k], kLpCout[l], kLpCin[l], 0, stream));
        g = o;
        if (kLpLevel[l - 1] != k) {                        // o is the gradient of the pooled map: route it to tap k - 1
            --tap;
            const size_t hwp = (size_t)L.h[k - 1] * L.w[k - 1];
            SPF_LP_TRY(launch_lpips_pool_bwd(o, ws + L.act[l - 1] + (size_t)gs * hwp * kLpCin[l], ws + L.gtap[tap], ng,
                                             L.h[k - 1], L.w[k - 1], kLpCin[l], stream));
            g = ws + L.gtap[tap];
        }
    }
    float* first = d0 ? d0 : d1;
    return launch_lpips_conv1_bwd(a, g, ws + L.act[0] + (size_t)gs * a.H * a.W * 64, ng, first, a.N, d0 ? d1 : nullptr,
                                  stream);
}

}  // namespace spf
