// Reprojection loss (LossReproj.forward, src/loss/loss_reproj.py:53-101 with project_to_cam, src/misc/cam_utils.py:289-307)
// for a batch of views in four launches, none of which synchronises the host.
//
// The reference, once per context view: a pixel grid built on the host and uploaded, torch.inverse of the poses (a host
// sync for its singularity check), ~25 eager kernels, `valid_mask.sum() > 0` and boolean indexing (two more syncs) and a
// division by a host integer.  Here, for pts3d[B,V,H,W,3] (each view normalised by its own valid count over the batch):
//   spf_reproj_fwd_kernel     one block per (chunk of 1024 points, image) slot, grid-stride: the block derives its camera
//                             (float64 4x4 inverse, rounded to float32), then per point the error, the valid flag and
//                             the term; a (float sum, integer count) partial per slot
//   spf_reproj_reduce_kernel  one block per view, fixed order: loss[v], and scale[v] = weight / n_valid for the backward
//   spf_reproj_bwd_kernel     the same slots, every point recomputed from pts3d (saving per-point state would cost the
//                             same bytes): dL/dpts3d, and 21-float partials of dL/dW[3x4] and dL/dK'[3x3] per slot
//   spf_reproj_cam_kernel     one block per image, fixed order: the partials chained through the inverse (float64) to
//                             dL/dposes and scaled back to dL/dintrinsics
// No atomics; a slot's content depends on the image and the chunk only, so a view's sums are formed in the same order
// whether it comes alone or in a batch: the batched call equals the per-view loop bitwise.
#include "point_slots.h"
#include "launchers.h"

namespace spf {

constexpr int kReprojCam = 21;             // W rows 0-2 (3x4, world -> camera) then K' (3x3, pixel units)
constexpr int kReprojGrad = 24;            // floats per backward partial: dW[12], dK'[9], padding

// The camera of image `img` (= b * V + v) into LDS: W = inverse(pose) in float64 (a GENERAL inverse, as torch.inverse),
// rounded to float32, and K' = K with row 0 scaled by W and row 1 by H in float32 (loss_reproj.py:72-74).
__device__ __forceinline__ void reproj_camera(const SpfReproj& a, int img, float* __restrict__ s_cam) {
    double P[16], Wd[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = (double)a.poses[16 * (int64_t)img + i];
    inv4<double>(P, Wd);
#pragma unroll
    for (int i = 0; i < 12; ++i) s_cam[i] = (float)Wd[i];
    const float* K = a.intrinsics + 9 * (int64_t)img;
    const float fw = (float)a.W, fh = (float)a.H;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        s_cam[12 + j] = K[j] * fw;
        s_cam[15 + j] = K[3 + j] * fh;
        s_cam[18 + j] = K[6 + j];
    }
}

// One point through project_to_cam and the error against its pixel corner (x = j, y = i).
struct ReprojPt {
    float cx, cy, cz;   // camera coordinates
    float qx, qy, qz;   // K' cam
    float z;            // max(qz, 1e-6) (NaN stays NaN, as clamp_)
    float dx, dy, e;    // px - target and its norm
};
__device__ __forceinline__ ReprojPt reproj_point(const float (&c)[kReprojCam], float x, float y, float zz, float tx,
                                                 float ty) {
    ReprojPt r;
    r.cx = c[0] * x + c[1] * y + c[2] * zz + c[3];
    r.cy = c[4] * x + c[5] * y + c[6] * zz + c[7];
    r.cz = c[8] * x + c[9] * y + c[10] * zz + c[11];
    r.qx = c[12] * r.cx + c[13] * r.cy + c[14] * r.cz;
    r.qy = c[15] * r.cx + c[16] * r.cy + c[17] * r.cz;
    r.qz = c[18] * r.cx + c[19] * r.cy + c[20] * r.cz;
    r.z = r.qz < 1e-6f ? 1e-6f : r.qz;
    r.dx = r.qx / r.z - tx;
    r.dy = r.qy / r.z - ty;
    r.e = sqrtf(r.dx * r.dx + r.dy * r.dy);
    return r;
}

// term(e) as summed (tanh modes: tanh(e / lw); the reduce multiplies by lw, as weighted_tanh does) and dterm/de of the
// loss's own term (tanh modes: d[lw tanh(e / lw)]/de = 1 - tanh^2).  The l1 family follows the reference's code: l1 keeps
// e where !(e > soft_clamp); l1+sqrt adds sqrt(soft_clamp e) above it; every other mode string adds log(1 + soft_clamp e).
template <int MODE>
__device__ __forceinline__ float reproj_term(float e, float lw, float soft) {
    if (MODE == SPF_REPROJ_TANH) return tanhf(e / lw);
    if (MODE == SPF_REPROJ_L1) return e > soft ? 0.f : e;
    if (MODE == SPF_REPROJ_L1_SQRT) return e > soft ? sqrtf(soft * e) : e;
    return e > soft ? logf(1.f + soft * e) : e;
}
template <int MODE>
__device__ __forceinline__ float reproj_dterm(float e, float lw, float soft) {
    if (MODE == SPF_REPROJ_TANH) {
        const float t = tanhf(e / lw);
        return 1.f - t * t;
    }
    if (MODE == SPF_REPROJ_L1) return e > soft ? 0.f : 1.f;
    if (MODE == SPF_REPROJ_L1_SQRT) return e > soft ? soft / (2.f * sqrtf(soft * e)) : 1.f;
    return e > soft ? soft / (1.f + soft * e) : 1.f;
}

__device__ __forceinline__ const float* reproj_image(const SpfReproj& a, int img) {
    const int b = img / a.V, v = img - b * a.V;
    return a.pts3d + (int64_t)b * a.stride_b + (int64_t)v * a.stride_v;
}

template <int MODE>
__global__ __launch_bounds__(kBlock) void spf_reproj_fwd_kernel(SpfReproj a, int nchunk, int64_t nslots,
                                                                float* __restrict__ psum, uint32_t* __restrict__ pcnt) {
    __shared__ float s_cam[kReprojCam];
    __shared__ SumRow<2> s_sum;
    const int n = a.H * a.W;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int img = (int)(slot / nchunk), chunk = (int)(slot - (int64_t)img * nchunk);
        __syncthreads();                                  // the previous slot's readers of s_cam are done
        if (threadIdx.x == 0) reproj_camera(a, img, s_cam);
        __syncthreads();
        float cam[kReprojCam];
#pragma unroll
        for (int i = 0; i < kReprojCam; ++i) cam[i] = s_cam[i];
        const float* base = reproj_image(a, img);
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float v[12];
        load4_xyz(base, aligned16(base), p0, n, v);
        float acc[1] = {0.f};
        uint32_t cnt[1] = {0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + k;
            if (p < n) {
                const int i = p / a.W, j = p - i * a.W;
                const ReprojPt r = reproj_point(cam, v[3 * k], v[3 * k + 1], v[3 * k + 2], (float)j, (float)i);
                const bool valid = !(r.e > a.hard_clamp);         // NaN counts as valid (and propagates)
                acc[0] += valid ? reproj_term<MODE>(r.e, a.lw, a.soft_clamp) : 0.f;
                cnt[0] += valid ? 1u : 0u;
            }
        }
        block_sum(acc, cnt, s_sum);
        if (threadIdx.x == 0) {
            psum[slot] = acc[0];
            pcnt[slot] = cnt[0];
        }
    }
}

// One block per view: its B * nchunk slots in a fixed order (slot k = b * nchunk + c of the view, whatever V is).
// loss[v] = weight * (lw * sum) / n_valid (lw = 1 outside the tanh modes), 0 when no point is valid; scale[v] =
// weight / n_valid, or 0: the backward then writes exact zeros.
__global__ __launch_bounds__(kBlock) void spf_reproj_reduce_kernel(const float* __restrict__ psum,
                                                                   const uint32_t* __restrict__ pcnt, int B, int V,
                                                                   int nchunk, float weight, float lw_mul,
                                                                   float* __restrict__ loss, float* __restrict__ scale) {
    __shared__ SumRow<2> s_sum;
    const int v = blockIdx.x;
    const int64_t m = (int64_t)B * nchunk;
    float acc[1] = {0.f};
    uint32_t cnt[1] = {0u};
    for (int64_t k = threadIdx.x; k < m; k += kBlock) {
        const int64_t b = k / nchunk, c = k - b * nchunk;
        const int64_t slot = (b * V + v) * nchunk + c;
        acc[0] += psum[slot];
        cnt[0] += pcnt[slot];
    }
    block_sum(acc, cnt, s_sum);
    if (threadIdx.x == 0) {
        const float tot = acc[0];
        const uint32_t nv = cnt[0];
        loss[v] = nv ? (weight * (lw_mul * tot)) / (float)nv : 0.f;
        scale[v] = nv ? weight / (float)nv : 0.f;
    }
}

// GPTS: write dL/dpts3d [B,V,H,W,3] (contiguous).  GCAM: write the slot's 24-float partial of dL/dW (12) and dL/dK' (9).
template <int MODE, bool GPTS, bool GCAM>
__global__ __launch_bounds__(kBlock) void spf_reproj_bwd_kernel(SpfReproj a, int nchunk, int64_t nslots,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ dL_dloss,
                                                                float* __restrict__ dpts, float* __restrict__ gpartial) {
    __shared__ float s_cam[kReprojCam];
    __shared__ SumRow<kReprojGrad> s_g;
    const int n = a.H * a.W;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int img = (int)(slot / nchunk), chunk = (int)(slot - (int64_t)img * nchunk);
        __syncthreads();                                  // the previous slot's readers of s_cam are done
        if (threadIdx.x == 0) reproj_camera(a, img, s_cam);
        __syncthreads();
        float cam[kReprojCam];
#pragma unroll
        for (int i = 0; i < kReprojCam; ++i) cam[i] = s_cam[i];
        const int view = img % a.V;
        const float gs = dL_dloss[view] * scale[view];           // upstream gradient read on the device: no sync
        const float* base = reproj_image(a, img);
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float v[12], o[12];
        load4_xyz(base, aligned16(base), p0, n, v);
        float g[kReprojGrad];
#pragma unroll
        for (int k = 0; k < kReprojGrad; ++k) g[k] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + k < n ? p0 + k : n - 1;            // (a point past the end contributes nothing)
            const int i = p / a.W, j = p - i * a.W;
            const ReprojPt r = reproj_point(cam, v[3 * k], v[3 * k + 1], v[3 * k + 2], (float)j, (float)i);
            const bool valid = p0 + k < n && !(r.e > a.hard_clamp);
            // norm backward (zero at e = 0), then invalid points get nothing
            const float ge = gs * reproj_dterm<MODE>(r.e, a.lw, a.soft_clamp);
            const float ke = (valid && r.e != 0.f) ? ge / r.e : 0.f;
            const float gx = valid ? r.dx * ke : 0.f, gy = valid ? r.dy * ke : 0.f;
            // px = q.xy / z: dq.xy = g / z, dz = -sum g q / z^2, through the clamp only where qz >= 1e-6
            const float z2 = r.z * r.z;
            const float dqx = gx / r.z, dqy = gy / r.z;
            const float dz = -gx * r.qx / z2 + -gy * r.qy / z2;
            const float dqz = r.qz >= 1e-6f ? dz : 0.f;
            // q = K' cam
            const float dcx = cam[12] * dqx + cam[15] * dqy + cam[18] * dqz;
            const float dcy = cam[13] * dqx + cam[16] * dqy + cam[19] * dqz;
            const float dcz = cam[14] * dqx + cam[17] * dqy + cam[20] * dqz;
            if (GPTS) {                                           // cam = W[:3,:3] p + W[:3,3]
                o[3 * k] = cam[0] * dcx + cam[4] * dcy + cam[8] * dcz;
                o[3 * k + 1] = cam[1] * dcx + cam[5] * dcy + cam[9] * dcz;
                o[3 * k + 2] = cam[2] * dcx + cam[6] * dcy + cam[10] * dcz;
            }
            if (GCAM) {
                const float dc[3] = {dcx, dcy, dcz}, dq[3] = {dqx, dqy, dqz}, cc[3] = {r.cx, r.cy, r.cz};
#pragma unroll
                for (int rr = 0; rr < 3; ++rr) {
                    g[4 * rr] += dc[rr] * v[3 * k];
                    g[4 * rr + 1] += dc[rr] * v[3 * k + 1];
                    g[4 * rr + 2] += dc[rr] * v[3 * k + 2];
                    g[4 * rr + 3] += dc[rr];
#pragma unroll
                    for (int c = 0; c < 3; ++c) g[12 + 3 * rr + c] += dq[rr] * cc[c];
                }
            }
        }
        if (GPTS) {
            float* out = dpts + (int64_t)img * n * 3;
            store4_xyz(out, aligned16(out), p0, n, o);
        }
        if (GCAM) {
            float lo[12], hi[12], slo[3], shi[3];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                lo[k] = g[k];
                hi[k] = g[12 + k];
            }
            wave_sum12(lo, slo);
            wave_sum12(hi, shi);
            // the row filled from wave_sum12's lane layout, with block_sum's two barriers (point_slots.h)
            const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
            __syncthreads();                              // the previous slot's readers of s_g are done
            if (lane < 4) {
#pragma unroll
                for (int jj = 0; jj < 3; ++jj) {
                    s_g.w[wave][4 * jj + lane] = __float_as_uint(slo[jj]);
                    s_g.w[wave][12 + 4 * jj + lane] = __float_as_uint(shi[jj]);
                }
            }
            __syncthreads();
            if (threadIdx.x < kReprojGrad) gpartial[slot * kReprojGrad + threadIdx.x] = sum_row_f32(s_g, threadIdx.x);
        }
    }
}

// One block per image: its nchunk partials in a fixed order, then dL/dpose = -W^T dW W^T (float64, W recomputed as the
// forward did; dW's last row is zero) and dL/dK = dL/dK' with row 0 scaled by W and row 1 by H.
__global__ __launch_bounds__(kBlock) void spf_reproj_cam_kernel(SpfReproj a, int nchunk,
                                                                const float* __restrict__ gpartial,
                                                                float* __restrict__ dposes, float* __restrict__ dintr) {
    __shared__ SumRow<kReprojGrad> s_sum;
    const int img = blockIdx.x;
    float acc[kReprojGrad];
#pragma unroll
    for (int k = 0; k < kReprojGrad; ++k) acc[k] = 0.f;
    for (int c = threadIdx.x; c < nchunk; c += kBlock) {
        const float4* pp = reinterpret_cast<const float4*>(gpartial + ((int64_t)img * nchunk + c) * kReprojGrad);
#pragma unroll
        for (int q = 0; q < kReprojGrad / 4; ++q) {
            const float4 x = pp[q];
            acc[4 * q] += x.x; acc[4 * q + 1] += x.y; acc[4 * q + 2] += x.z; acc[4 * q + 3] += x.w;
        }
    }
    block_sum(acc, s_sum);
    if (threadIdx.x != 0) return;
    double tot[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) tot[k] = (double)acc[k];
    if (dposes) {
        double P[16], Wd[16], T1[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) P[i] = (double)a.poses[16 * (int64_t)img + i];
        inv4<double>(P, Wd);
        // T1 = W^T dW  (dW rows 0-2 = tot[0..11], row 3 = 0)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) s += Wd[4 * k + i] * tot[4 * k + j];
                T1[4 * i + j] = s;
            }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += T1[4 * i + k] * Wd[4 * j + k];
                dposes[16 * (int64_t)img + 4 * i + j] = (float)-s;
            }
    }
    if (dintr) {
        const double fw = (double)a.W, fh = (double)a.H;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            dintr[9 * (int64_t)img + c] = (float)(tot[12 + c] * fw);
            dintr[9 * (int64_t)img + 3 + c] = (float)(tot[15 + c] * fh);
            dintr[9 * (int64_t)img + 6 + c] = (float)tot[18 + c];
        }
    }
}

int64_t reproj_slots(int B, int V, int H, int W, int* nchunk) {
    const int64_t n = (int64_t)H * W;
    const int64_t nc = slot_chunks(n);
    if (nchunk) *nchunk = (int)nc;
    return (int64_t)B * V * nc;
}

template <int MODE>
static void reproj_fwd_launch(const SpfReproj& a, int nchunk, int64_t nslots, float* psum, uint32_t* pcnt,
                              hipStream_t stream) {
    spf_reproj_fwd_kernel<MODE><<<slot_grid(nslots), kBlock, 0, stream>>>(a, nchunk, nslots, psum, pcnt);
}

hipError_t launch_reproj_fwd(const SpfReproj& a, void* partial, float* loss, float* scale, hipStream_t stream) {
    int nchunk = 0;
    const int64_t nslots = reproj_slots(a.B, a.V, a.H, a.W, &nchunk);
    float* psum = static_cast<float*>(partial);
    uint32_t* pcnt = reinterpret_cast<uint32_t*>(psum + nslots);
    switch (a.mode) {
        case SPF_REPROJ_TANH: reproj_fwd_launch<SPF_REPROJ_TANH>(a, nchunk, nslots, psum, pcnt, stream); break;
        case SPF_REPROJ_L1: reproj_fwd_launch<SPF_REPROJ_L1>(a, nchunk, nslots, psum, pcnt, stream); break;
        case SPF_REPROJ_L1_SQRT: reproj_fwd_launch<SPF_REPROJ_L1_SQRT>(a, nchunk, nslots, psum, pcnt, stream); break;
        default: reproj_fwd_launch<SPF_REPROJ_L1_LOG>(a, nchunk, nslots, psum, pcnt, stream); break;
    }
    const float lw_mul = a.mode == SPF_REPROJ_TANH ? a.lw : 1.f;
    spf_reproj_reduce_kernel<<<a.V, kBlock, 0, stream>>>(psum, pcnt, a.B, a.V, nchunk, a.weight, lw_mul, loss, scale);
    return hipGetLastError();
}

template <int MODE>
static void reproj_bwd_launch(const SpfReproj& a, int nchunk, int64_t nslots, const float* scale, const float* dL_dloss,
                              float* dpts, float* gpartial, hipStream_t stream) {
    const int grid = slot_grid(nslots);
    if (dpts && gpartial)
        spf_reproj_bwd_kernel<MODE, true, true><<<grid, kBlock, 0, stream>>>(a, nchunk, nslots, scale, dL_dloss, dpts,
                                                                              gpartial);
    else if (dpts)
        spf_reproj_bwd_kernel<MODE, true, false><<<grid, kBlock, 0, stream>>>(a, nchunk, nslots, scale, dL_dloss, dpts,
                                                                               nullptr);
    else
        spf_reproj_bwd_kernel<MODE, false, true><<<grid, kBlock, 0, stream>>>(a, nchunk, nslots, scale, dL_dloss,
                                                                               nullptr, gpartial);
}

hipError_t launch_reproj_bwd(const SpfReproj& a, const float* scale, const float* dL_dloss, float* dpts, float* gpartial,
                             float* dposes, float* dintr, hipStream_t stream) {
    int nchunk = 0;
    const int64_t nslots = reproj_slots(a.B, a.V, a.H, a.W, &nchunk);
    switch (a.mode) {
        case SPF_REPROJ_TANH:
            reproj_bwd_launch<SPF_REPROJ_TANH>(a, nchunk, nslots, scale, dL_dloss, dpts, gpartial, stream); break;
        case SPF_REPROJ_L1:
            reproj_bwd_launch<SPF_REPROJ_L1>(a, nchunk, nslots, scale, dL_dloss, dpts, gpartial, stream); break;
        case SPF_REPROJ_L1_SQRT:
            reproj_bwd_launch<SPF_REPROJ_L1_SQRT>(a, nchunk, nslots, scale, dL_dloss, dpts, gpartial, stream); break;
        default:
            reproj_bwd_launch<SPF_REPROJ_L1_LOG>(a, nchunk, nslots, scale, dL_dloss, dpts, gpartial, stream); break;
    }
    if (gpartial) spf_reproj_cam_kernel<<<a.B * a.V, kBlock, 0, stream>>>(a, nchunk, gpartial, dposes, dintr);
    return hipGetLastError();
}

}  // namespace spf
