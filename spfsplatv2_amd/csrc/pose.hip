// The pose path of SPFSplatV2's pose-free step, between the pose head's raw output and the decoder's extrinsics, and the
// pose numbers logged beside the loss -- none of it synchronises the host, none of it uses an atomic, and no block
// waits for another.
//
//   spf_pose_compose_{fwd,bwd}_kernel   process_pose (encoder_spfsplatv2.py:340-359, encoder_spfsplatv2l.py:248-269):
//                             one LANE per scene walks its views in float64 (pose_math.h): the views of a scene are
//                             coupled through the baseline and the base pose, scenes are not
//   spf_depth_{fwd,bwd,cam}_kernel      depth_projector (cam_utils.py:310-318): slots of 1024 points as in reproj.hip,
//                             row 2 of the float64 inverse once per block; the backward writes dL/dpts and a 4-float
//                             partial per slot, one block per image sums them in order and chains them through the
//                             inverse
//   spf_pose_error_kernel     compute_pose_error (evaluation/metrics.py:70-99) for N pairs and the three means, one
//                             block, float64 inside
//   spf_focal_kernel          estimate_focal_knowing_depth (misc/intrinsics_utils.py:33-108, 'weiszfeld'), one block of
//                             1024 lanes per scene: the closed-form start and ten reweighting rounds over the same
//                             H W points, re-read from L2 each round (a scene is 768 KB at 256 x 256; keeping x/z, y/z
//                             of 64 points per lane would take 128 VGPRs at four waves per SIMD, and LDS holds a third
//                             of them); per-point float32, the two running sums float64 in a fixed order
#include "point_slots.h"
#include "pose_math.h"
#include "launchers.h"

namespace spf {

constexpr int kPoseBlock = 64;
constexpr int kFocalBlock = 1024;

__device__ __forceinline__ PoseScene pose_scene(const float* enc, int64_t stride_b, int64_t stride_v, int scene, int v,
                                                int cv, int encoding, int baseline, int relative) {
    return PoseScene{enc + scene * stride_b, stride_v, v, cv, encoding, baseline, relative};
}

__global__ __launch_bounds__(kPoseBlock) void spf_pose_compose_fwd_kernel(const float* __restrict__ enc, int64_t stride_b,
                                                                          int64_t stride_v, int b, int v, int cv,
                                                                          int encoding, int baseline, int relative,
                                                                          float* __restrict__ poses) {
    const int scene = blockIdx.x * kPoseBlock + threadIdx.x;
    if (scene >= b) return;
    pose_scene_forward(pose_scene(enc, stride_b, stride_v, scene, v, cv, encoding, baseline, relative),
                       poses + 16 * (int64_t)scene * v);
}

__global__ __launch_bounds__(kPoseBlock) void spf_pose_compose_bwd_kernel(const float* __restrict__ enc, int64_t stride_b,
                                                                          int64_t stride_v, int b, int v, int cv,
                                                                          int encoding, int baseline, int relative,
                                                                          const float* __restrict__ dposes,
                                                                          float* __restrict__ denc) {
    const int scene = blockIdx.x * kPoseBlock + threadIdx.x;
    if (scene >= b) return;
    pose_scene_backward(pose_scene(enc, stride_b, stride_v, scene, v, cv, encoding, baseline, relative),
                        dposes + 16 * (int64_t)scene * v, denc + 9 * (int64_t)scene * v);
}

hipError_t launch_pose_compose_fwd(const float* enc, int64_t stride_b, int64_t stride_v, int b, int v, int cv,
                                   int encoding, int baseline, int relative, float* poses, hipStream_t stream) {
    spf_pose_compose_fwd_kernel<<<(b + kPoseBlock - 1) / kPoseBlock, kPoseBlock, 0, stream>>>(
        enc, stride_b, stride_v, b, v, cv, encoding, baseline, relative, poses);
    return hipGetLastError();
}

hipError_t launch_pose_compose_bwd(const float* enc, int64_t stride_b, int64_t stride_v, int b, int v, int cv,
                                   int encoding, int baseline, int relative, const float* dposes, float* denc,
                                   hipStream_t stream) {
    spf_pose_compose_bwd_kernel<<<(b + kPoseBlock - 1) / kPoseBlock, kPoseBlock, 0, stream>>>(
        enc, stride_b, stride_v, b, v, cv, encoding, baseline, relative, dposes, denc);
    return hipGetLastError();
}

// ---- depth projection --------------------------------------------------------------------------------------------
// Row 2 of W = inverse(pose) (float64, general), rounded to float32.
__device__ __forceinline__ void depth_row(const float* __restrict__ poses, int img, float* __restrict__ s_row) {
    double P[16], Wd[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = (double)poses[16 * (int64_t)img + i];
    inv4<double>(P, Wd);
#pragma unroll
    for (int i = 0; i < 4; ++i) s_row[i] = (float)Wd[8 + i];
}

__global__ __launch_bounds__(kBlock) void spf_depth_fwd_kernel(const float* __restrict__ pts, int64_t stride_img,
                                                               const float* __restrict__ poses, int n, int nchunk,
                                                               int64_t nslots, float* __restrict__ depth) {
    __shared__ float s_row[4];
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int img = (int)(slot / nchunk), chunk = (int)(slot - (int64_t)img * nchunk);
        __syncthreads();
        if (threadIdx.x == 0) depth_row(poses, img, s_row);
        __syncthreads();
        const float w0 = s_row[0], w1 = s_row[1], w2 = s_row[2], w3 = s_row[3];
        const float* base = pts + (int64_t)img * stride_img;
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float v[12], o[4];
        load4_xyz(base, aligned16(base), p0, n, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = w0 * v[3 * k] + w1 * v[3 * k + 1] + w2 * v[3 * k + 2] + w3;
        float* out = depth + (int64_t)img * n;
        store4(out, aligned16(out), p0, n, o);
    }
}

// dL/dpts = g W[2,:3] (dpts may be null), and the slot's partial sum of g [p, 1] (gpartial may be null).
__global__ __launch_bounds__(kBlock) void spf_depth_bwd_kernel(const float* __restrict__ pts, int64_t stride_img,
                                                               const float* __restrict__ poses, int n, int nchunk,
                                                               int64_t nslots, const float* __restrict__ gdepth,
                                                               float* __restrict__ dpts, float* __restrict__ gpartial) {
    __shared__ float s_row[4];
    __shared__ SumRow<4> s_sum;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int img = (int)(slot / nchunk), chunk = (int)(slot - (int64_t)img * nchunk);
        __syncthreads();                                  // the previous slot's readers of s_row are done
        if (threadIdx.x == 0) depth_row(poses, img, s_row);
        __syncthreads();
        const float w0 = s_row[0], w1 = s_row[1], w2 = s_row[2];
        const float* base = pts + (int64_t)img * stride_img;
        const float* gin = gdepth + (int64_t)img * n;
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = p0 + k < n ? gin[p0 + k] : 0.f;
        if (dpts) {
            float* out = dpts + (int64_t)img * n * 3;
            float o[12];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                o[3 * k] = g[k] * w0;
                o[3 * k + 1] = g[k] * w1;
                o[3 * k + 2] = g[k] * w2;
            }
            store4_xyz(out, aligned16(out), p0, n, o);
        }
        if (gpartial) {                             // (the same for the whole block: block_sum's barriers are uniform)
            float v[12];
            load4_xyz(base, aligned16(base), p0, n, v);
            float a[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < 4; ++k) {           // (g is 0 past the end, and so are the points loaded there)
                a[0] += g[k] * v[3 * k];
                a[1] += g[k] * v[3 * k + 1];
                a[2] += g[k] * v[3 * k + 2];
                a[3] += g[k];
            }
            block_sum(a, s_sum);
            if (threadIdx.x == 0) {
#pragma unroll
                for (int c = 0; c < 4; ++c) gpartial[4 * slot + c] = a[c];
            }
        }
    }
}

// One block per image: its nchunk partials in a fixed order = dL/dW[2, :]; dL/dpose = -W^T dW W^T in float64.
__global__ __launch_bounds__(kBlock) void spf_depth_cam_kernel(const float* __restrict__ poses, int nchunk,
                                                               const float* __restrict__ gpartial,
                                                               float* __restrict__ dposes) {
    __shared__ SumRow<4> s_sum;
    const int img = blockIdx.x;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = threadIdx.x; c < nchunk; c += kBlock) {
        const float4 x = *reinterpret_cast<const float4*>(gpartial + 4 * ((int64_t)img * nchunk + c));
        acc[0] += x.x; acc[1] += x.y; acc[2] += x.z; acc[3] += x.w;
    }
    block_sum(acc, s_sum);
    if (threadIdx.x != 0) return;
    double tot[4], P[16], Wd[16];
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] = (double)acc[k];
#pragma unroll
    for (int i = 0; i < 16; ++i) P[i] = (double)poses[16 * (int64_t)img + i];
    inv4<double>(P, Wd);
    // (W^T dW)[i][j] = W[2][i] tot[j]; times W^T: sum_k tot[k] W[j][k]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double r = tot[0] * Wd[4 * j] + tot[1] * Wd[4 * j + 1] + tot[2] * Wd[4 * j + 2] + tot[3] * Wd[4 * j + 3];
#pragma unroll
        for (int i = 0; i < 4; ++i) dposes[16 * (int64_t)img + 4 * i + j] = (float)-(Wd[8 + i] * r);
    }
}

int64_t depth_slots(int N, int n, int* nchunk) {
    const int nc = (int)slot_chunks(n);
    if (nchunk) *nchunk = nc;
    return (int64_t)N * nc;
}

hipError_t launch_depth_fwd(const float* pts, int64_t stride_img, const float* poses, int N, int n, float* depth,
                            hipStream_t stream) {
    int nchunk = 0;
    const int64_t nslots = depth_slots(N, n, &nchunk);
    spf_depth_fwd_kernel<<<slot_grid(nslots), kBlock, 0, stream>>>(pts, stride_img, poses, n, nchunk, nslots, depth);
    return hipGetLastError();
}

hipError_t launch_depth_bwd(const float* pts, int64_t stride_img, const float* poses, int N, int n, const float* gdepth,
                            float* dpts, float* gpartial, float* dposes, hipStream_t stream) {
    int nchunk = 0;
    const int64_t nslots = depth_slots(N, n, &nchunk);
    spf_depth_bwd_kernel<<<slot_grid(nslots), kBlock, 0, stream>>>(pts, stride_img, poses, n, nchunk, nslots, gdepth,
                                                                    dpts, gpartial);
    if (gpartial) spf_depth_cam_kernel<<<N, kBlock, 0, stream>>>(poses, nchunk, gpartial, dposes);
    return hipGetLastError();
}

// ---- pose errors -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void spf_pose_error_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ gt, int N,
                                                                float* __restrict__ errors, float* __restrict__ means) {
    __shared__ double s[kBlock][3];
    double acc[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < N; i += kBlock) {
        double e[3];
        pose_error_one(pred + 16 * (int64_t)i, gt + 16 * (int64_t)i, e);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            errors[3 * (int64_t)i + k] = (float)e[k];
            acc[k] += e[k];
        }
    }
    block_tree_sum<kBlock>(acc, s);
    if (threadIdx.x < 3) {                               // one float64 division per lane, not three in a row
        const double tot = threadIdx.x == 0 ? acc[0] : (threadIdx.x == 1 ? acc[1] : acc[2]);
        means[threadIdx.x] = (float)(tot / (double)N);
    }
}

hipError_t launch_pose_error(const float* pred, const float* gt, int N, float* errors, float* means,
                             hipStream_t stream) {
    spf_pose_error_kernel<<<1, kBlock, 0, stream>>>(pred, gt, N, errors, means);
    return hipGetLastError();
}

// ---- focal estimate ----------------------------------------------------------------------------------------------
struct FocalArgs {
    const float* pts;
    int64_t stride_scene, stride_row;      // floats; a row's W points are contiguous
    const float* pp;                       // [2] or one pair per scene (pp_stride 2), or null: (W/2, H/2)
    int64_t pp_stride;
    int H, W;
    float focal_base, lo, hi;              // the clip bounds min_focal * base, max_focal * base
    float cx, cy, div0, div1;              // the 3x3: rows (f, 0, cx) / div0, (0, f, cy) / div1, (0, 0, 1)
};

// One round over the scene's points: sums of w (a . px) and w (a . a) with w = 1 (FIRST) or 1 / max(|px - f a|, 1e-8).
// Lane t takes points 4 (k 1024 + t) .. + 3 of trip k whatever the strides are, so the order of every sum is fixed.
template <bool FIRST>
__device__ __forceinline__ void focal_round(const FocalArgs& a, const float* __restrict__ base, bool wide, float ppx,
                                            float ppy, float f, double (*s)[3], double& s1, double& s2) {
    const int n = a.H * a.W;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int p0 = 4 * threadIdx.x; p0 < n; p0 += 4 * kFocalBlock) {
        float v[12];
        if (wide && p0 + 3 < n) {
            load12(base + 3 * (int64_t)p0, v);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int p = p0 + k < n ? p0 + k : n - 1;
                const int i = p / a.W, j = p - i * a.W;
                const float* q = base + i * a.stride_row + 3 * j;
                v[3 * k] = q[0]; v[3 * k + 1] = q[1]; v[3 * k + 2] = q[2];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int p = p0 + k;
            const float z = v[3 * k + 2];
            if (p < n && z > 0.f) {                              // (NaN z is invalid)
                const int i = p / a.W, j = p - i * a.W;
                float ax = v[3 * k] / z, ay = v[3 * k + 1] / z;
                ax = (ax != ax || fabsf(ax) == INFINITY) ? 0.f : ax;      // nan_to_num(posinf=0, neginf=0)
                ay = (ay != ay || fabsf(ay) == INFINITY) ? 0.f : ay;
                const float px = (float)j - ppx, py = (float)i - ppy;
                const float dpx = ax * px + ay * py, daa = ax * ax + ay * ay;
                if (FIRST) {
                    acc[0] += (double)dpx;
                    acc[1] += (double)daa;
                } else {
                    const float dx = px - f * ax, dy = py - f * ay;
                    const float dis = sqrtf(dx * dx + dy * dy);
                    const float w = 1.f / (dis < 1e-8f ? 1e-8f : dis);   // (NaN stays NaN, as clip)
                    acc[0] += (double)(w * dpx);
                    acc[1] += (double)(w * daa);
                }
            }
        }
    }
    block_tree_sum<kFocalBlock>(acc, s);
    s1 = acc[0];
    s2 = acc[1];
}

__global__ __launch_bounds__(kFocalBlock) void spf_focal_kernel(FocalArgs a, float* __restrict__ focal,
                                                                float* __restrict__ intrinsics) {
    __shared__ double s[kFocalBlock][3];
    const int scene = blockIdx.x;
    const float* base = a.pts + scene * a.stride_scene;
    const bool wide = a.stride_row == 3 * (int64_t)a.W && aligned16(base);
    const float ppx = a.pp ? a.pp[scene * a.pp_stride] : (float)a.W / 2.f;
    const float ppy = a.pp ? a.pp[scene * a.pp_stride + 1] : (float)a.H / 2.f;
    double s1, s2;
    focal_round<true>(a, base, wide, ppx, ppy, 0.f, s, s1, s2);
    float f = (float)(s1 / s2);
    if (f <= 0.f) f = a.focal_base;                              // (NaN does not take the branch)
    for (int it = 0; it < 10; ++it) {
        focal_round<false>(a, base, wide, ppx, ppy, f, s, s1, s2);
        f = (float)(s1 / s2);
    }
    f = f < a.lo ? a.lo : f;                                     // clip(min, max): NaN stays NaN
    f = f > a.hi ? a.hi : f;
    if (f <= 0.f) f = a.focal_base;
    if (threadIdx.x == 0) {
        focal[scene] = f;
        if (intrinsics) {
            float* K = intrinsics + 9 * (int64_t)scene;
            K[0] = f / a.div0; K[1] = 0.f; K[2] = a.cx / a.div0;
            K[3] = 0.f; K[4] = f / a.div1; K[5] = a.cy / a.div1;
            K[6] = 0.f; K[7] = 0.f; K[8] = 1.f;
        }
    }
}

hipError_t launch_focal(const float* pts, int64_t stride_scene, int64_t stride_row, int B, int H, int W, const float* pp,
                        int64_t pp_stride, float focal_base, float lo, float hi, float cx, float cy, float div0,
                        float div1, float* focal, float* intrinsics, hipStream_t stream) {
    const FocalArgs a{pts, stride_scene, stride_row, pp, pp_stride, H, W, focal_base, lo, hi, cx, cy, div0, div1};
    spf_focal_kernel<<<B, kFocalBlock, 0, stream>>>(a, focal, intrinsics);
    return hipGetLastError();
}

}  // namespace spf
