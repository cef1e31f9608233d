// What the two fused-attention translation units share (attention.hip: float32 matrix path with MASK / NORM / VIEWS;
// attention16.hip: 16-bit matrix path): the tile sizes, the kernels' plain argument blocks and how the host fills them,
// the convert-at-load / convert-at-store of four elements, a lane's share of a staged tile as it comes from memory, and
// the store of an accumulator row.  Everything here has a caller in each file.  What a file does with a staged tile
// (stage_commit, own_rows, the LDS images) is its own and stays there.
#pragma once

#include "rope_math.h"

namespace spf {

typedef float f16v __attribute__((ext_vector_type(16)));

constexpr int kAttnD = 64;          // head dim (the only one)
constexpr int kAttnT = 32;          // rows of a staged tile = rows a wave owns
constexpr int kAttnOwn = 128;       // rows a block owns

inline int attn_blocks(int n) { return (n + kAttnOwn - 1) / kAttnOwn; }

struct AttnArgs {
    const void *q, *k, *v;
    const int64_t *qpos, *kpos;
    int64_t qs[3], ks[3], vs[3];    // element strides: batch, token, head
    int B, H, Nq, Nk;
    float scale;
    RopeFreq f;                     // +F0 / base^(q/16)
};
struct AttnGradArgs {
    void *dq, *dk, *dv;
    int64_t dqs[3], dks[3], dvs[3];
};

inline AttnArgs make_attn_args(const SpfAttn& p) {
    AttnArgs a;
    a.q = p.q; a.k = p.k; a.v = p.v;
    a.qpos = p.qpos; a.kpos = p.kpos;
    for (int i = 0; i < 3; ++i) { a.qs[i] = p.q_stride[i]; a.ks[i] = p.k_stride[i]; a.vs[i] = p.v_stride[i]; }
    a.B = p.B; a.H = p.H; a.Nq = p.Nq; a.Nk = p.Nk;
    a.scale = p.scale;
    a.f = rope_freq(kAttnD, p.base, p.F0);
    return a;
}
inline AttnGradArgs make_attn_grad_args(const SpfAttnGrads& gr) {
    AttnGradArgs g;
    g.dq = gr.dq; g.dk = gr.dk; g.dv = gr.dv;
    for (int i = 0; i < 3; ++i) { g.dqs[i] = gr.dq_stride[i]; g.dks[i] = gr.dk_stride[i]; g.dvs[i] = gr.dv_stride[i]; }
    return g;
}

// delta[b,h,q] = sum_d dout[b,q,h,d] * out[b,q,h,d]: the row-dot pre-pass of every backward (spf_attn_delta_kernel,
// defined in attention.hip).  dtype: 0 = float32, 1 = float16, 2 = bfloat16.
hipError_t launch_attn_delta(int dtype, const void* out, const void* dout, float* delta, int B, int H, int Nq,
                             hipStream_t stream);

template <typename T> __device__ __forceinline__ void load4(const T* p, float* f);
template <> __device__ __forceinline__ void load4<float>(const float* p, float* f) {
    const f4a v = *reinterpret_cast<const f4a*>(p);
    f[0] = v[0]; f[1] = v[1]; f[2] = v[2]; f[3] = v[3];
}
template <typename H> struct __attribute__((aligned(8))) Half4 { H h[4]; };
template <typename H> __device__ __forceinline__ void load4h(const H* p, float* f) {
    const Half4<H> v = *reinterpret_cast<const Half4<H>*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = to_f<H>(v.h[i]);
}
template <> __device__ __forceinline__ void load4<__half>(const __half* p, float* f) { load4h(p, f); }
template <> __device__ __forceinline__ void load4<__hip_bfloat16>(const __hip_bfloat16* p, float* f) { load4h(p, f); }

template <typename T> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<f4a*>(p) = f4a{a, b, c, d};
}
template <typename H> __device__ __forceinline__ void store4h(H* p, float a, float b, float c, float d) {
    Half4<H> v;
    v.h[0] = from_f<H>(a); v.h[1] = from_f<H>(b); v.h[2] = from_f<H>(c); v.h[3] = from_f<H>(d);
    *reinterpret_cast<Half4<H>*>(p) = v;
}
template <> __device__ __forceinline__ void store4<__half>(__half* p, float a, float b, float c, float d) { store4h(p, a, b, c, d); }
template <> __device__ __forceinline__ void store4<__hip_bfloat16>(__hip_bfloat16* p, float a, float b, float c, float d) { store4h(p, a, b, c, d); }

// One lane's share of a staged tile of 32 rows x 64: row tid >> 3, and of that row the four (u, v) pairs with
// frequencies q0 .. q0 + 3 of half x (y positions rotate d < 32, x positions d >= 32; u at 32 x + q, v at 32 x + 16 + q).
struct Stage {
    float u[4], v[4], p;
};
// NARROW (the VIEWS kernels, whose `base` moves from view to view): the lane's offset into the view is formed in 32
// bits -- a uniform base plus a 32-bit lane offset is one address register per lane instead of two, which is what keeps
// the VIEWS dk/dv pass inside its plain sibling's registers; the host refuses a view whose rows reach past 2^31 elements.
template <typename T, bool NARROW = false>
__device__ __forceinline__ void stage_load(Stage& r, const T* __restrict__ base, int64_t stride_n,
                                           const int64_t* __restrict__ pos, int row0, int N, int tid) {
    const int row = row0 + (tid >> 3), part = tid & 7, x = part >> 2, q0 = (part & 3) * 4;
    r.p = 0.f;
    if (row < N) {
        const T* __restrict__ s;
        if constexpr (NARROW) s = base + (uint32_t)(row * (int)stride_n + 32 * x + q0);
        else s = base + (int64_t)row * stride_n + 32 * x + q0;
        load4<T>(s, r.u);
        load4<T>(s + 16, r.v);
        if (pos) r.p = NARROW ? (float)pos[(uint32_t)(row * 2 + x)] : (float)pos[(int64_t)row * 2 + x];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.u[k] = r.v[k] = 0.f;
    }
}

// C/D map of the 32 x 32 accumulator: the row of register r on lane half kl (the column is lane & 31)
__device__ __forceinline__ int acc_row(int r, int kl) { return (r & 3) + 8 * (r >> 2) + 4 * kl; }

// one half (y or x) of a row's gradient rotated by -angle; p = the row's position along that axis
__device__ __forceinline__ void unrotate_half(f16v& a, float p, const RopeFreq& f, int kl) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {               // u: registers 0..7 (d < 16 of the half), v: registers 8..15 (d + 16)
        float sn, cs;
        rope_sincos(p * f.inv[(r & 3) + 8 * (r >> 2) + 4 * kl], sn, cs);
        const float u = a[r], v = a[r + 8];
        a[r] = fmaf(u, cs, v * sn);
        a[r + 8] = fmaf(v, cs, -(u * sn));
    }
}

// A row of a transposed result on this lane (rows of the accumulator = d, acc0: d < 32, acc1: d >= 32) times mult,
// rotated back by -angle when pos (the row's (y, x)) is given, converted and stored at g.
template <typename T>
__device__ __forceinline__ void store_row(T* __restrict__ g, f16v acc0, f16v acc1, float mult, const int64_t* __restrict__ pos,
                                          const RopeFreq& f, int kl) {
#pragma unroll
    for (int x = 0; x < 2; ++x) {
        f16v a = x ? acc1 : acc0;
        if (pos) unrotate_half(a, (float)pos[x], f, kl);
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
            store4<T>(g + 32 * x + 8 * gq + 4 * kl, a[4 * gq] * mult, a[4 * gq + 1] * mult, a[4 * gq + 2] * mult,
                      a[4 * gq + 3] * mult);
    }
}

}  // namespace spf
