// Block- and slot-level helpers of the loss, pose and metric kernels (reproj, regr3d, pose, loss, ssim, lpips, and the
// camera backward reduce): the one copy of the "slot" pattern that gives these operators their guarantees -- sums that
// are bitwise repeatable, do not depend on the batch and do not depend on the strides, without a float atomic.
//
// A slot is kSlotPoints = 1024 points of one row (an image, a point map), four consecutive points per lane of a
// 256-thread block: where the row's base is 16-byte aligned the four xyz points are three 16-byte loads.  A block takes
// slots grid-stride; what it writes for a slot depends on (row, chunk) only.  Every sum goes lane -> wave (the DPP
// ladder of spf_common.h) -> block, the four waves as (w0 + w1) + (w2 + w3) -> slot -> row, each level in a fixed order.
//
// Barrier contract of the block reductions (block_sum, block_tree_sum): the CONSERVATIVE form.  Each starts with a
// barrier before it writes its LDS row and has one after, so
//   on entry   nothing is asked of the row: whoever still reads it -- the previous call on the same row, the previous
//              slot of a grid-stride loop -- is past that read when the first write lands;
//   on return  every thread holds the totals in registers, and the row may still be being read by other threads: only
//              another call of these helpers may write it without a barrier of the caller's own.
// They must be called by all threads of the block, outside divergent control flow.  A kernel that fills a SumRow itself
// shows its barriers at the call site: the reprojection backward (from wave_sum12's lane layout, once per slot: both
// barriers) and the LPIPS head (per-wave totals, once per block: nobody reads the row before, so only the one after).
#pragma once

#include "spf_common.h"

namespace spf {

// ---- slot geometry --------------------------------------------------------------------------------------------------
constexpr int kSlotPoints = 4 * kBlock;   // points per slot: four per lane (three 16-byte loads of xyz)
constexpr int kSlotMaxGrid = 2048;        // memory-bound kernels: a few blocks per CU, grid-stride over the slots
constexpr int kWaves = kBlock / kWave;

inline int64_t slot_chunks(int64_t n) { return (n + kSlotPoints - 1) / kSlotPoints; }
inline int slot_grid(int64_t nslots) { return (int)(nslots < kSlotMaxGrid ? nslots : kSlotMaxGrid); }

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- loads and stores of a lane's four points ----------------------------------------------------------------------
// (p0 = first of the lane's four points, n = points in the row.  The vector path is taken only when the row's base is
//  16-byte aligned -- `aligned`, the caller's aligned16(row) -- and all four points exist; a point past the end reads as
//  0 and is not stored.)
__device__ __forceinline__ void load12(const float* __restrict__ p, float (&v)[12]) {   // p 16-byte aligned
    const float4* p4 = reinterpret_cast<const float4*>(p);
    const float4 a = p4[0], b = p4[1], c = p4[2];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = c.x; v[9] = c.y; v[10] = c.z; v[11] = c.w;
}
__device__ __forceinline__ void load4_xyz(const float* __restrict__ row, bool aligned, int p0, int n, float (&v)[12]) {
    if (aligned && p0 + 3 < n) {
        load12(row + 3 * (int64_t)p0, v);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = p0 + k < n;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * k + c] = in ? row[3 * (int64_t)(p0 + k) + c] : 0.f;
        }
    }
}
__device__ __forceinline__ void store4_xyz(float* __restrict__ row, bool aligned, int p0, int n, const float (&v)[12]) {
    if (aligned && p0 + 3 < n) {
        float4* o4 = reinterpret_cast<float4*>(row + 3 * (int64_t)p0);
        o4[0] = make_float4(v[0], v[1], v[2], v[3]);
        o4[1] = make_float4(v[4], v[5], v[6], v[7]);
        o4[2] = make_float4(v[8], v[9], v[10], v[11]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < n) {
#pragma unroll
                for (int c = 0; c < 3; ++c) row[3 * (int64_t)(p0 + k) + c] = v[3 * k + c];
            }
    }
}
// one float per point: a 16-byte access
__device__ __forceinline__ void load4(const float* __restrict__ row, bool aligned, int p0, int n, float (&v)[4]) {
    if (aligned && p0 + 3 < n) {
        const float4 x = *reinterpret_cast<const float4*>(row + p0);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = p0 + k < n ? row[p0 + k] : 0.f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ row, bool aligned, int p0, int n, const float (&v)[4]) {
    if (aligned && p0 + 3 < n) {
        *reinterpret_cast<float4*>(row + p0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (p0 + k < n) row[p0 + k] = v[k];
    }
}

// ---- block sums, float32 and uint32 ---------------------------------------------------------------------------------
// The LDS row of a block sum of N values per lane: one 32-bit word per (wave, value) -- floats by their bit pattern, so
// that sums and counts formed back to back share a row and its two barriers.
template <int N>
struct SumRow {
    uint32_t w[kWaves][N];
};
// The four waves' entries of value k in the fixed order (w0 + w1) + (w2 + w3).  No barrier: the caller has one between
// the writes of the row and this read.
template <int N>
__device__ __forceinline__ float sum_row_f32(const SumRow<N>& s, int k) {
    return (__uint_as_float(s.w[0][k]) + __uint_as_float(s.w[1][k])) +
           (__uint_as_float(s.w[2][k]) + __uint_as_float(s.w[3][k]));
}
template <int N>
__device__ __forceinline__ uint32_t sum_row_u32(const SumRow<N>& s, int k) {
    return (s.w[0][k] + s.w[1][k]) + (s.w[2][k] + s.w[3][k]);
}

// Sums over the kBlock threads of NF floats and NU counts per lane, in place: on return f[] and u[] hold the block's
// totals in EVERY thread.  Per value wave_sum / wave_sum_u32, lane 0 of each wave to the row, then the fixed wave order.
// Barrier contract: conservative (see the head of this file) -- safe anywhere all threads reach it.
template <int NF, int NU>
__device__ __forceinline__ void block_sum_words(float* __restrict__ f, uint32_t* __restrict__ u, SumRow<NF + NU>& s) {
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = wave_sum(f[k]);
#pragma unroll
    for (int k = 0; k < NU; ++k) u[k] = wave_sum_u32(u[k]);
    __syncthreads();                                   // every earlier reader of the row is done
    if ((threadIdx.x & (kWave - 1)) == 0) {
        const int wave = threadIdx.x >> 6;
#pragma unroll
        for (int k = 0; k < NF; ++k) s.w[wave][k] = __float_as_uint(f[k]);
#pragma unroll
        for (int k = 0; k < NU; ++k) s.w[wave][NF + k] = u[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NF; ++k) f[k] = sum_row_f32(s, k);
#pragma unroll
    for (int k = 0; k < NU; ++k) u[k] = sum_row_u32(s, NF + k);
}
template <int NF, int NU>
__device__ __forceinline__ void block_sum(float (&f)[NF], uint32_t (&u)[NU], SumRow<NF + NU>& s) {
    block_sum_words<NF, NU>(f, u, s);
}
template <int NF>
__device__ __forceinline__ void block_sum(float (&f)[NF], SumRow<NF>& s) {
    block_sum_words<NF, 0>(f, nullptr, s);
}
__device__ __forceinline__ float block_sum(float x, SumRow<1>& s) {
    block_sum_words<1, 0>(&x, nullptr, s);
    return x;
}

// ---- block sum, float64 ----------------------------------------------------------------------------------------------
// Sums over the NT threads of the block of N doubles per lane, in place (totals in every thread on return), through the
// LDS tree s[NT][N] that halves from NT / 2 down: entry t takes entry t + half.
// Barrier contract: conservative, as block_sum.
template <int NT, int N>
__device__ __forceinline__ void block_tree_sum(double (&x)[N], double (*__restrict__ s)[N]) {
    __syncthreads();                                   // every earlier reader of s[0] is done
#pragma unroll
    for (int k = 0; k < N; ++k) s[threadIdx.x][k] = x[k];
    __syncthreads();
    for (int half = NT / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
#pragma unroll
            for (int k = 0; k < N; ++k) s[threadIdx.x][k] += s[threadIdx.x + half][k];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = s[0][k];
}
template <int NT>
__device__ __forceinline__ double block_tree_sum(double x, double* __restrict__ s) {   // s[NT]
    double v[1] = {x};
    block_tree_sum<NT, 1>(v, reinterpret_cast<double (*)[1]>(s));
    return v[0];
}

}  // namespace spf
