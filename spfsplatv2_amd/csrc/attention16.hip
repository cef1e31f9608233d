// Fused RoPE attention on the 16-bit matrix units of gfx950, head dim 64: the opt-in sibling of attention.hip for
// float16 / bfloat16 operands (plain calls only: no mask, no q/k norm, no views).  Forward and backward of
//   out = softmax(scale * R(qpos) q * (R(kpos) k)^T) * v
// with every product on v_mfma_f32_32x32x16_f16 / _bf16 (float32 accumulators) and the softmax in float32.
//
// Rounding points (the contract): q and k are rotated in float32 while they are staged and rounded ONCE to
// T; the score, the running maximum and sum, lse, delta, the scale factor and the rotate-back of the gradients stay
// float32 (scale multiplies the float32 score, never q); P (forward) and P, dS (backward) are rounded once to T as
// operands of the second products; the row sum is taken from the float32 P; out, dq, dk, dv are rounded at the store.
//
// Tiles: attention.hip's.  A block is 4 waves, a wave owns 32 rows of the block's 128 and keeps them as the B operand
// of the first product (lane l: row l & 31, k-step s: elements d = 16 s + 8 (l >> 5) + j, j < 8); the other side is
// walked in tiles of 32 rows staged in LDS, the next tile's global loads in flight under the matrix instructions.  The
// score tile is computed TRANSPOSED with respect to the owner (X = staged * owner^T), so the owner's row is the
// accumulator's column and lives on one lane and its partner l ^ 32: row statistics are per lane with one exchange, and
// the second product (Y^T = staged^T * X) sums over X's ROW index, so X's registers, converted, are its B operand as
// they are: registers 8 s .. 8 s + 7 are k-step s, element j of lane half h being row 16 s + 8 (j >> 2) + 4 h + (j & 3).
// The A operand of that product must present the SAME k order: it is read from a transposed LDS image [d][staged row]
// as two 8-byte runs (rows 16 s + 4 h .. + 3 and 16 s + 8 + 4 h .. + 3).
//
// LDS images of a staged tile, 16-bit elements: the ROW image [32][72] (144-byte pitch: the 16-byte operand reads of 16
// lanes fall on 16 disjoint groups of 4 banks) feeds the first product; the TRANSPOSED image [64][36] (72-byte pitch: the
// 8-byte reads of a lane half fall on 32 disjoint bank pairs) feeds the second.  A kernel writes only the images it reads.
//
// Backward: no atomics, two passes as in attention.hip (dq owns queries, dk/dv owns keys), both recompute P from the
// saved log-sum-exp; delta = sum_d dout * out is a small pre-pass.  The float32 path's refined row term (delta~ + c) is
// not carried: the gate against eager 16-bit is met without it and it costs 10 % of the step (DESIGN.md 7k has the
// figures of both forms: it lowers dq's error about 3 x where the logits reach +-80 and nowhere else), so the two passes
// are independent of each other.  Every sum has a fixed order: bitwise reproducible.
#include "rope_math.h"

namespace spf {

namespace {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef short s8v __attribute__((ext_vector_type(8)));          // a matrix operand: 8 x 16 bits
typedef short s4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef __bf16 b8v __attribute__((ext_vector_type(8)));
typedef unsigned short bits16;

constexpr int kD = 64;              // head dim (the only one)
constexpr int kT = 32;              // rows of a staged tile = rows a wave owns
constexpr int kOwn = 128;           // rows a block owns
constexpr int kRowLd = 72;          // pitch of the row image, elements
constexpr int kTrLd = 36;           // pitch of the transposed image, elements

struct Args16 {
    const void *q, *k, *v;
    const int64_t *qpos, *kpos;
    int64_t qs[3], ks[3], vs[3];    // element strides: batch, token, head
    int B, H, Nq, Nk;
    float scale;
    RopeFreq f;
};
struct GradArgs16 {
    void *dq, *dk, *dv;
    int64_t dqs[3], dks[3], dvs[3];
};

template <typename T> __device__ __forceinline__ float bits_to_f(bits16 b);
template <> __device__ __forceinline__ float bits_to_f<__half>(bits16 b) { return __half2float(__ushort_as_half(b)); }
template <> __device__ __forceinline__ float bits_to_f<__hip_bfloat16>(bits16 b) { return __uint_as_float((uint32_t)b << 16); }
template <typename T> __device__ __forceinline__ bits16 f_to_bits(float v);
template <> __device__ __forceinline__ bits16 f_to_bits<__half>(float v) { return __half_as_ushort(__float2half(v)); }
template <> __device__ __forceinline__ bits16 f_to_bits<__hip_bfloat16>(float v) {
    return __bfloat16_as_ushort(__float2bfloat16(v));
}

template <typename T> __device__ __forceinline__ f16v mfma16(s8v a, s8v b, f16v c);
template <> __device__ __forceinline__ f16v mfma16<__half>(s8v a, s8v b, f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8v, a), __builtin_bit_cast(h8v, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ f16v mfma16<__hip_bfloat16>(s8v a, s8v b, f16v c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b8v, a), __builtin_bit_cast(b8v, b), c, 0, 0, 0);
}

struct __attribute__((aligned(8))) Bits4 { bits16 h[4]; };
template <typename T> __device__ __forceinline__ void load4(const T* p, float* f) {
    const Bits4 v = *reinterpret_cast<const Bits4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) f[i] = bits_to_f<T>(v.h[i]);
}
template <typename T> __device__ __forceinline__ void store4(T* p, float a, float b, float c, float d) {
    Bits4 v;
    v.h[0] = f_to_bits<T>(a); v.h[1] = f_to_bits<T>(b); v.h[2] = f_to_bits<T>(c); v.h[3] = f_to_bits<T>(d);
    *reinterpret_cast<Bits4*>(p) = v;
}

// One lane's share of a staged tile of 32 rows x 64 (attention.hip's split): row tid >> 3, and of that row the four
// (u, v) pairs with frequencies q0 .. q0 + 3 of half x (u at 32 x + q, v at 32 x + 16 + q).
struct Stage {
    float u[4], v[4], p;
};
template <typename T>
__device__ __forceinline__ void stage_load(Stage& r, const T* __restrict__ base, int64_t stride_n,
                                           const int64_t* __restrict__ pos, int row0, int N, int tid) {
    const int row = row0 + (tid >> 3), part = tid & 7, x = part >> 2, q0 = (part & 3) * 4;
    r.p = 0.f;
    if (row < N) {
        const T* __restrict__ s = base + (int64_t)row * stride_n + 32 * x + q0;
        load4<T>(s, r.u);
        load4<T>(s + 16, r.v);
        if (pos) r.p = (float)pos[(int64_t)row * 2 + x];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.u[k] = r.v[k] = 0.f;
    }
}
// rotate (rot) by +angle in float32, round once to T, write the images the kernel reads (ROW: s_row, TR: s_tr)
template <typename T, bool ROW, bool TR>
__device__ __forceinline__ void stage_commit(const Stage& r, bits16* __restrict__ s_row, bits16* __restrict__ s_tr, bool rot,
                                             const RopeFreq& f, int tid) {
    const int row = tid >> 3, part = tid & 7, x = part >> 2, q0 = (part & 3) * 4;
    Bits4 bu, bv;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float u = r.u[k], v = r.v[k];
        if (rot) {
            float sn, cs;
            rope_sincos(r.p * f.inv[q0 + k], sn, cs);
            const float uo = fmaf(u, cs, -(v * sn)), vo = fmaf(v, cs, u * sn);
            u = uo; v = vo;
        }
        bu.h[k] = f_to_bits<T>(u);
        bv.h[k] = f_to_bits<T>(v);
    }
    const int d = 32 * x + q0;
    if constexpr (ROW) {
        *reinterpret_cast<Bits4*>(s_row + row * kRowLd + d) = bu;
        *reinterpret_cast<Bits4*>(s_row + row * kRowLd + d + 16) = bv;
    }
    if constexpr (TR) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            s_tr[(d + k) * kTrLd + row] = bu.h[k];
            s_tr[(d + 16 + k) * kTrLd + row] = bv.h[k];
        }
    }
}

// Operand of the first product (A: the staged row, B: the owner's row) from a row image: row il, elements
// d = 16 s + 8 kl + j.
__device__ __forceinline__ s8v row_frag(const bits16* __restrict__ s_row, int il, int kl, int s) {
    return *reinterpret_cast<const s8v*>(s_row + il * kRowLd + 16 * s + 8 * kl);
}
// A operand of the second product from a transposed image: row d of the result, k-step s, in the k order of a converted
// accumulator: element j = staged row 16 s + 8 (j >> 2) + 4 kl + (j & 3).
__device__ __forceinline__ s8v tr_frag(const bits16* __restrict__ s_tr, int d, int kl, int s) {
    const s4v lo = *reinterpret_cast<const s4v*>(s_tr + d * kTrLd + 16 * s + 4 * kl);
    const s4v hi = *reinterpret_cast<const s4v*>(s_tr + d * kTrLd + 16 * s + 8 + 4 * kl);
    return s8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// B operand of the second product: registers 8 s .. 8 s + 7 of an accumulator, rounded once to T.
template <typename T> __device__ __forceinline__ s8v acc_frag(const f16v& x, int s) {
    s8v r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (short)f_to_bits<T>(x[8 * s + j]);
    return r;
}

__device__ __forceinline__ int acc_row(int r, int kl) { return (r & 3) + 8 * (r >> 2) + 4 * kl; }

// The rows a wave owns, as B operands: stage the block's 128 rows 32 at a time through the row images s_a (and s_b for a
// second operand with the same rows, never rotated); each wave keeps its own chunk.
template <typename T>
__device__ __forceinline__ void own_rows(s8v (&ra)[4], const T* __restrict__ a, int64_t a_sn, const int64_t* __restrict__ pos,
                                         s8v (&rb)[4], const T* __restrict__ b, int64_t b_sn, int row0, int N,
                                         bits16* __restrict__ s_a, bits16* __restrict__ s_b, const RopeFreq& f, int tid) {
    const int lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        Stage sa, sb;
        stage_load<T>(sa, a, a_sn, pos, row0 + kT * w, N, tid);
        if (b) stage_load<T>(sb, b, b_sn, nullptr, row0 + kT * w, N, tid);
        __syncthreads();
        stage_commit<T, true, false>(sa, s_a, nullptr, pos != nullptr, f, tid);
        if (b) stage_commit<T, true, false>(sb, s_b, nullptr, false, f, tid);
        __syncthreads();
        if (w == wave) {
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                ra[s] = row_frag(s_a, il, kl, s);
                if (b) rb[s] = row_frag(s_b, il, kl, s);
            }
        }
    }
}

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

// A row of a transposed result (rows of the accumulator = d, acc0: d < 32, acc1: d >= 32) times mult, rotated back when
// pos is given, rounded once and stored at g.
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

// ---- forward -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void spf_attn16_fwd_kernel(Args16 a, T* __restrict__ out, float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) bits16 s_k[kT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_vt[kD * kTrLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kOwn;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + b * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + b * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + b * a.vs[0] + h * a.vs[2];
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;

    s8v qf[4], unused[4];
    own_rows<T>(qf, qb, a.qs[1], qp, unused, nullptr, 0, q0, a.Nq, s_k, nullptr, a.f, tid);
    const bool active = q0 + kT * wave < a.Nq;          // wave-uniform: a wave without queries only helps staging
    const int qi = q0 + kT * wave + il;

    f16v o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) o0[e] = o1[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    Stage sk, sv;
    stage_load<T>(sk, kb, a.ks[1], kp, 0, a.Nk, tid);
    stage_load<T>(sv, vb, a.vs[1], nullptr, 0, a.Nk, tid);
#pragma unroll 1
    for (int k0 = 0; k0 < a.Nk; k0 += kT) {
        __syncthreads();                                // the previous tile's readers are done
        stage_commit<T, true, false>(sk, s_k, nullptr, kp != nullptr, a.f, tid);
        stage_commit<T, false, true>(sv, nullptr, s_vt, false, a.f, tid);
        __syncthreads();
        if (k0 + kT < a.Nk) {                           // in flight under the matrix instructions below
            stage_load<T>(sk, kb, a.ks[1], kp, k0 + kT, a.Nk, tid);
            stage_load<T>(sv, vb, a.vs[1], nullptr, k0 + kT, a.Nk, tid);
        }
        if (!active) continue;
        f16v s;                                         // S^T: rows = keys, column = this lane's query
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) s = mfma16<T>(row_frag(s_k, il, kl, st), qf[st], s);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= a.scale;
        if (k0 + kT > a.Nk) {                           // padded keys: probability 0
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (k0 + acc_row(r, kl) >= a.Nk) s[r] = -INFINITY;
        }
        float tmax = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
        const float mn = fmaxf(m, tmax);                // finite: every tile holds at least one key
        const float alpha = expf(m - mn);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = expf(s[r] - mn);
            ps += s[r];                                 // the row sum: from the float32 P
        }
        l = l * alpha + ps;
#pragma unroll
        for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
#pragma unroll
        for (int st = 0; st < 2; ++st) {                // O^T += V^T P^T
            const s8v pf = acc_frag<T>(s, st);
            o0 = mfma16<T>(tr_frag(s_vt, il, kl, st), pf, o0);
            o1 = mfma16<T>(tr_frag(s_vt, il + 32, kl, st), pf, o1);
        }
    }
    if (!active) return;
    const float lt = l + __shfl_xor(l, 32, kWave);
    if (qi >= a.Nq) return;
    if (kl == 0) lse[((int64_t)b * a.H + h) * a.Nq + qi] = m + logf(lt);
    store_row<T>(out + (((int64_t)b * a.Nq + qi) * a.H + h) * kD, o0, o1, 1.f / lt, nullptr, a.f, kl);
}

// ---- backward ------------------------------------------------------------------------------------------------------
// delta[b,h,q] = sum_d dout[b,q,h,d] * out[b,q,h,d], one lane per row, one float32 fma chain over d in ascending order
// (attention.hip's row-dot kernel for the two element types of this file).
template <typename T>
__global__ __launch_bounds__(kBlock) void spf_attn16_delta_kernel(const T* __restrict__ out, const T* __restrict__ dout,
                                                                  float* __restrict__ delta, int B, int H, int Nq) {
    const int64_t rows = (int64_t)B * Nq * H, row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    float acc = 0.f;
#pragma unroll
    for (int part = 0; part < 16; ++part) {
        float o[4], g[4];
        load4<T>(out + row * kD + 4 * part, o);
        load4<T>(dout + row * kD + 4 * part, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(g[e], o[e], acc);
    }
    const int64_t bq = row / H;
    const int h = (int)(row - bq * H);
    const int64_t b = bq / Nq;
    delta[(b * H + h) * Nq + (bq - b * Nq)] = acc;
}

// dq: the block owns 128 queries, walks the keys.
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void spf_attn16_dq_kernel(Args16 a, GradArgs16 g, const T* __restrict__ dout,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ delta) {
    __shared__ __attribute__((aligned(16))) bits16 s_k[kT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_v[kT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_kt[kD * kTrLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kOwn;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + b * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + b * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + b * a.vs[0] + h * a.vs[2];
    const T* __restrict__ gb = dout + ((int64_t)b * a.Nq * a.H + h) * kD;
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;

    s8v qf[4], gf[4];
    own_rows<T>(qf, qb, a.qs[1], qp, gf, gb, (int64_t)a.H * kD, q0, a.Nq, s_k, s_v, a.f, tid);
    const bool active = q0 + kT * wave < a.Nq;
    const int qi = q0 + kT * wave + il;
    float my_lse = INFINITY, my_dl = 0.f;               // a padded query: probability 0
    if (qi < a.Nq) {
        my_lse = lse[((int64_t)b * a.H + h) * a.Nq + qi];
        my_dl = delta[((int64_t)b * a.H + h) * a.Nq + qi];
    }

    f16v dq0, dq1;
#pragma unroll
    for (int e = 0; e < 16; ++e) dq0[e] = dq1[e] = 0.f;
    Stage sk, sv;
    stage_load<T>(sk, kb, a.ks[1], kp, 0, a.Nk, tid);
    stage_load<T>(sv, vb, a.vs[1], nullptr, 0, a.Nk, tid);
#pragma unroll 1
    for (int k0 = 0; k0 < a.Nk; k0 += kT) {
        __syncthreads();
        stage_commit<T, true, true>(sk, s_k, s_kt, kp != nullptr, a.f, tid);
        stage_commit<T, true, false>(sv, s_v, nullptr, false, a.f, tid);
        __syncthreads();
        if (k0 + kT < a.Nk) {
            stage_load<T>(sk, kb, a.ks[1], kp, k0 + kT, a.Nk, tid);
            stage_load<T>(sv, vb, a.vs[1], nullptr, k0 + kT, a.Nk, tid);
        }
        if (!active) continue;
        f16v s, dp;                                     // S^T, dP^T: rows = keys, column = this lane's query
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            s = mfma16<T>(row_frag(s_k, il, kl, st), qf[st], s);
            dp = mfma16<T>(row_frag(s_v, il, kl, st), gf[st], dp);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float p = expf(fmaf(s[r], a.scale, -my_lse));
            if (k0 + acc_row(r, kl) >= a.Nk) p = 0.f;   // padded keys
            dp[r] = p * (dp[r] - my_dl);
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {                // dQ^T += Kr^T dS^T
            const s8v df = acc_frag<T>(dp, st);
            dq0 = mfma16<T>(tr_frag(s_kt, il, kl, st), df, dq0);
            dq1 = mfma16<T>(tr_frag(s_kt, il + 32, kl, st), df, dq1);
        }
    }
    if (!active || qi >= a.Nq) return;
    store_row<T>(static_cast<T*>(g.dq) + b * g.dqs[0] + (int64_t)qi * g.dqs[1] + h * g.dqs[2], dq0, dq1, a.scale,
                 qp ? qp + (int64_t)qi * 2 : nullptr, a.f, kl);
}

// dk, dv: the block owns 128 keys, walks the queries.
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void spf_attn16_dkdv_kernel(Args16 a, GradArgs16 g, const T* __restrict__ dout,
                                                                    const float* __restrict__ lse,
                                                                    const float* __restrict__ delta) {
    __shared__ __attribute__((aligned(16))) bits16 s_q[kT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_do[kT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_qt[kD * kTrLd];
    __shared__ __attribute__((aligned(16))) bits16 s_dot[kD * kTrLd];
    __shared__ float s_lse[kT], s_dl[kT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * kOwn;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + b * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + b * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + b * a.vs[0] + h * a.vs[2];
    const T* __restrict__ gb = dout + ((int64_t)b * a.Nq * a.H + h) * kD;
    const int64_t g_sn = (int64_t)a.H * kD;
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;
    const float* __restrict__ lse_r = lse + ((int64_t)b * a.H + h) * a.Nq;
    const float* __restrict__ dl_r = delta + ((int64_t)b * a.H + h) * a.Nq;

    s8v kf[4], vf[4];
    own_rows<T>(kf, kb, a.ks[1], kp, vf, vb, a.vs[1], k0, a.Nk, s_q, s_do, a.f, tid);
    const bool active = k0 + kT * wave < a.Nk;

    f16v dk0, dk1, dv0, dv1;
#pragma unroll
    for (int e = 0; e < 16; ++e) dk0[e] = dk1[e] = dv0[e] = dv1[e] = 0.f;
    Stage sq, sd;
    float rl = INFINITY, rd = 0.f;                      // a padded query: probability 0
    stage_load<T>(sq, qb, a.qs[1], qp, 0, a.Nq, tid);
    stage_load<T>(sd, gb, g_sn, nullptr, 0, a.Nq, tid);
    if (tid < kT && tid < a.Nq) { rl = lse_r[tid]; rd = dl_r[tid]; }
#pragma unroll 1
    for (int q0 = 0; q0 < a.Nq; q0 += kT) {
        __syncthreads();
        stage_commit<T, true, true>(sq, s_q, s_qt, qp != nullptr, a.f, tid);
        stage_commit<T, true, true>(sd, s_do, s_dot, false, a.f, tid);
        if (tid < kT) { s_lse[tid] = rl; s_dl[tid] = rd; }
        __syncthreads();
        if (q0 + kT < a.Nq) {
            stage_load<T>(sq, qb, a.qs[1], qp, q0 + kT, a.Nq, tid);
            stage_load<T>(sd, gb, g_sn, nullptr, q0 + kT, a.Nq, tid);
            rl = INFINITY; rd = 0.f;
            if (tid < kT && q0 + kT + tid < a.Nq) { rl = lse_r[q0 + kT + tid]; rd = dl_r[q0 + kT + tid]; }
        }
        if (!active) continue;
        f16v s, dp;                                     // S, dP: rows = queries, column = this lane's key
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            s = mfma16<T>(row_frag(s_q, il, kl, st), kf[st], s);
            dp = mfma16<T>(row_frag(s_do, il, kl, st), vf[st], dp);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, kl);
            const float p = expf(fmaf(s[r], a.scale, -s_lse[row]));
            s[r] = p;
            dp[r] = p * (dp[r] - s_dl[row]);
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {                // dV^T += dO^T P, dK^T += Qr^T dS
            const s8v pf = acc_frag<T>(s, st), df = acc_frag<T>(dp, st);
            dv0 = mfma16<T>(tr_frag(s_dot, il, kl, st), pf, dv0);
            dv1 = mfma16<T>(tr_frag(s_dot, il + 32, kl, st), pf, dv1);
            dk0 = mfma16<T>(tr_frag(s_qt, il, kl, st), df, dk0);
            dk1 = mfma16<T>(tr_frag(s_qt, il + 32, kl, st), df, dk1);
        }
    }
    if (!active) return;
    const int key = k0 + kT * wave + il;
    if (key >= a.Nk) return;
    store_row<T>(static_cast<T*>(g.dv) + b * g.dvs[0] + (int64_t)key * g.dvs[1] + h * g.dvs[2], dv0, dv1, 1.f, nullptr, a.f,
                 kl);
    store_row<T>(static_cast<T*>(g.dk) + b * g.dks[0] + (int64_t)key * g.dks[1] + h * g.dks[2], dk0, dk1, a.scale,
                 kp ? kp + (int64_t)key * 2 : nullptr, a.f, kl);
}

Args16 make_args(const SpfAttn& p) {
    Args16 a;
    a.q = p.q; a.k = p.k; a.v = p.v;
    a.qpos = p.qpos; a.kpos = p.kpos;
    for (int i = 0; i < 3; ++i) { a.qs[i] = p.q_stride[i]; a.ks[i] = p.k_stride[i]; a.vs[i] = p.v_stride[i]; }
    a.B = p.B; a.H = p.H; a.Nq = p.Nq; a.Nk = p.Nk;
    a.scale = p.scale;
    a.f = rope_freq(kD, p.base, p.F0);
    return a;
}

inline int blocks_of(int n) { return (n + kOwn - 1) / kOwn; }

template <typename T>
hipError_t forward16(const SpfAttn& p, void* out, float* lse, hipStream_t stream) {
    spf_attn16_fwd_kernel<T><<<dim3(blocks_of(p.Nq), p.H, p.B), kBlock, 0, stream>>>(make_args(p), static_cast<T*>(out), lse);
    return hipGetLastError();
}

template <typename T>
hipError_t backward16(const SpfAttn& p, const SpfAttnGrads& gr, const void* out, const float* lse, const void* dout,
                      hipStream_t stream) {
    const Args16 a = make_args(p);
    GradArgs16 g;
    g.dq = gr.dq; g.dk = gr.dk; g.dv = gr.dv;
    for (int i = 0; i < 3; ++i) { g.dqs[i] = gr.dq_stride[i]; g.dks[i] = gr.dk_stride[i]; g.dvs[i] = gr.dv_stride[i]; }
    const T* go = static_cast<const T*>(dout);
    const int64_t rows = (int64_t)p.B * p.Nq * p.H;
    spf_attn16_delta_kernel<T><<<(unsigned)((rows + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
        static_cast<const T*>(out), go, gr.delta, p.B, p.H, p.Nq);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    spf_attn16_dq_kernel<T><<<dim3(blocks_of(p.Nq), p.H, p.B), kBlock, 0, stream>>>(a, g, go, lse, gr.delta);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    spf_attn16_dkdv_kernel<T><<<dim3(blocks_of(p.Nk), p.H, p.B), kBlock, 0, stream>>>(a, g, go, lse, gr.delta);
    return hipGetLastError();
}

}  // namespace

// dtype: 1 = float16, 2 = bfloat16 (the caller has checked it)
hipError_t launch_attn16_forward(const SpfAttn& p, void* out, float* lse, hipStream_t stream) {
    return p.dtype == 1 ? forward16<__half>(p, out, lse, stream) : forward16<__hip_bfloat16>(p, out, lse, stream);
}

hipError_t launch_attn16_backward(const SpfAttn& p, const SpfAttnGrads& g, const void* out, const float* lse, const void* dout,
                                  hipStream_t stream) {
    return p.dtype == 1 ? backward16<__half>(p, g, out, lse, dout, stream)
                        : backward16<__hip_bfloat16>(p, g, out, lse, dout, stream);
}

}  // namespace spf
