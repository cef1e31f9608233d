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
//
// attention_tiles.h holds what this file shares with attention.hip: the tile sizes, AttnArgs / AttnGradArgs and their
// fill, load4 / store4, Stage and stage_load, acc_row, unrotate_half and store_row; the row-dot pre-pass is
// attention.hip's kernel behind launch_attn_delta.  This file owns the 16-bit LDS images (stage_commit, own_rows), the
// operand fragments and the three matrix kernels.
#include "attention_tiles.h"
#include "launchers.h"

namespace spf {

namespace {

typedef short s8v __attribute__((ext_vector_type(8)));          // a matrix operand: 8 x 16 bits
typedef short s4v __attribute__((ext_vector_type(4)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef __bf16 b8v __attribute__((ext_vector_type(8)));
typedef unsigned short bits16;

constexpr int kRowLd = 72;          // pitch of the row image, elements
constexpr int kTrLd = 36;           // pitch of the transposed image, elements

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

struct __attribute__((aligned(8))) Bits4 { bits16 h[4]; };    // four elements of an LDS image

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
        stage_load<T>(sa, a, a_sn, pos, row0 + kAttnT * w, N, tid);
        if (b) stage_load<T>(sb, b, b_sn, nullptr, row0 + kAttnT * w, N, tid);
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

// ---- forward -------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void spf_attn16_fwd_kernel(AttnArgs a, T* __restrict__ out, float* __restrict__ lse) {
    __shared__ __attribute__((aligned(16))) bits16 s_k[kAttnT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_vt[kAttnD * kTrLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kAttnOwn;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + b * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + b * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + b * a.vs[0] + h * a.vs[2];
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;

    s8v qf[4], unused[4];
    own_rows<T>(qf, qb, a.qs[1], qp, unused, nullptr, 0, q0, a.Nq, s_k, nullptr, a.f, tid);
    const bool active = q0 + kAttnT * wave < a.Nq;          // wave-uniform: a wave without queries only helps staging
    const int qi = q0 + kAttnT * wave + il;

    f16v o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) o0[e] = o1[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    Stage sk, sv;
    stage_load<T>(sk, kb, a.ks[1], kp, 0, a.Nk, tid);
    stage_load<T>(sv, vb, a.vs[1], nullptr, 0, a.Nk, tid);
#pragma unroll 1
    for (int k0 = 0; k0 < a.Nk; k0 += kAttnT) {
        __syncthreads();                                // the previous tile's readers are done
        stage_commit<T, true, false>(sk, s_k, nullptr, kp != nullptr, a.f, tid);
        stage_commit<T, false, true>(sv, nullptr, s_vt, false, a.f, tid);
        __syncthreads();
        if (k0 + kAttnT < a.Nk) {                           // in flight under the matrix instructions below
            stage_load<T>(sk, kb, a.ks[1], kp, k0 + kAttnT, a.Nk, tid);
            stage_load<T>(sv, vb, a.vs[1], nullptr, k0 + kAttnT, a.Nk, tid);
        }
        if (!active) continue;
        f16v s;                                         // S^T: rows = keys, column = this lane's query
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 4; ++st) s = mfma16<T>(row_frag(s_k, il, kl, st), qf[st], s);
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] *= a.scale;
        if (k0 + kAttnT > a.Nk) {                           // padded keys: probability 0
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
    store_row<T>(out + (((int64_t)b * a.Nq + qi) * a.H + h) * kAttnD, o0, o1, 1.f / lt, nullptr, a.f, kl);
}

// ---- backward ------------------------------------------------------------------------------------------------------
// dq: the block owns 128 queries, walks the keys.
template <typename T>
__global__ __launch_bounds__(kBlock, 2) void spf_attn16_dq_kernel(AttnArgs a, AttnGradArgs g, const T* __restrict__ dout,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ delta) {
    __shared__ __attribute__((aligned(16))) bits16 s_k[kAttnT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_v[kAttnT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_kt[kAttnD * kTrLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kAttnOwn;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + b * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + b * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + b * a.vs[0] + h * a.vs[2];
    const T* __restrict__ gb = dout + ((int64_t)b * a.Nq * a.H + h) * kAttnD;
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;

    s8v qf[4], gf[4];
    own_rows<T>(qf, qb, a.qs[1], qp, gf, gb, (int64_t)a.H * kAttnD, q0, a.Nq, s_k, s_v, a.f, tid);
    const bool active = q0 + kAttnT * wave < a.Nq;
    const int qi = q0 + kAttnT * wave + il;
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
    for (int k0 = 0; k0 < a.Nk; k0 += kAttnT) {
        __syncthreads();
        stage_commit<T, true, true>(sk, s_k, s_kt, kp != nullptr, a.f, tid);
        stage_commit<T, true, false>(sv, s_v, nullptr, false, a.f, tid);
        __syncthreads();
        if (k0 + kAttnT < a.Nk) {
            stage_load<T>(sk, kb, a.ks[1], kp, k0 + kAttnT, a.Nk, tid);
            stage_load<T>(sv, vb, a.vs[1], nullptr, k0 + kAttnT, a.Nk, tid);
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
__global__ __launch_bounds__(kBlock, 2) void spf_attn16_dkdv_kernel(AttnArgs a, AttnGradArgs g, const T* __restrict__ dout,
                                                                    const float* __restrict__ lse,
                                                                    const float* __restrict__ delta) {
    __shared__ __attribute__((aligned(16))) bits16 s_q[kAttnT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_do[kAttnT * kRowLd];
    __shared__ __attribute__((aligned(16))) bits16 s_qt[kAttnD * kTrLd];
    __shared__ __attribute__((aligned(16))) bits16 s_dot[kAttnD * kTrLd];
    __shared__ float s_lse[kAttnT], s_dl[kAttnT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * kAttnOwn;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + b * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + b * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + b * a.vs[0] + h * a.vs[2];
    const T* __restrict__ gb = dout + ((int64_t)b * a.Nq * a.H + h) * kAttnD;
    const int64_t g_sn = (int64_t)a.H * kAttnD;
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;
    const float* __restrict__ lse_r = lse + ((int64_t)b * a.H + h) * a.Nq;
    const float* __restrict__ dl_r = delta + ((int64_t)b * a.H + h) * a.Nq;

    s8v kf[4], vf[4];
    own_rows<T>(kf, kb, a.ks[1], kp, vf, vb, a.vs[1], k0, a.Nk, s_q, s_do, a.f, tid);
    const bool active = k0 + kAttnT * wave < a.Nk;

    f16v dk0, dk1, dv0, dv1;
#pragma unroll
    for (int e = 0; e < 16; ++e) dk0[e] = dk1[e] = dv0[e] = dv1[e] = 0.f;
    Stage sq, sd;
    float rl = INFINITY, rd = 0.f;                      // a padded query: probability 0
    stage_load<T>(sq, qb, a.qs[1], qp, 0, a.Nq, tid);
    stage_load<T>(sd, gb, g_sn, nullptr, 0, a.Nq, tid);
    if (tid < kAttnT && tid < a.Nq) { rl = lse_r[tid]; rd = dl_r[tid]; }
#pragma unroll 1
    for (int q0 = 0; q0 < a.Nq; q0 += kAttnT) {
        __syncthreads();
        stage_commit<T, true, true>(sq, s_q, s_qt, qp != nullptr, a.f, tid);
        stage_commit<T, true, true>(sd, s_do, s_dot, false, a.f, tid);
        if (tid < kAttnT) { s_lse[tid] = rl; s_dl[tid] = rd; }
        __syncthreads();
        if (q0 + kAttnT < a.Nq) {
            stage_load<T>(sq, qb, a.qs[1], qp, q0 + kAttnT, a.Nq, tid);
            stage_load<T>(sd, gb, g_sn, nullptr, q0 + kAttnT, a.Nq, tid);
            rl = INFINITY; rd = 0.f;
            if (tid < kAttnT && q0 + kAttnT + tid < a.Nq) { rl = lse_r[q0 + kAttnT + tid]; rd = dl_r[q0 + kAttnT + tid]; }
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
    const int key = k0 + kAttnT * wave + il;
    if (key >= a.Nk) return;
    store_row<T>(static_cast<T*>(g.dv) + b * g.dvs[0] + (int64_t)key * g.dvs[1] + h * g.dvs[2], dv0, dv1, 1.f, nullptr, a.f,
                 kl);
    store_row<T>(static_cast<T*>(g.dk) + b * g.dks[0] + (int64_t)key * g.dks[1] + h * g.dks[2], dk0, dk1, a.scale,
                 kp ? kp + (int64_t)key * 2 : nullptr, a.f, kl);
}

template <typename T>
hipError_t forward16(const SpfAttn& p, void* out, float* lse, hipStream_t stream) {
    spf_attn16_fwd_kernel<T><<<dim3(attn_blocks(p.Nq), p.H, p.B), kBlock, 0, stream>>>(make_attn_args(p),
                                                                                       static_cast<T*>(out), lse);
    return hipGetLastError();
}

template <typename T>
hipError_t backward16(const SpfAttn& p, const SpfAttnGrads& gr, const void* out, const float* lse, const void* dout,
                      hipStream_t stream) {
    const AttnArgs a = make_attn_args(p);
    const AttnGradArgs g = make_attn_grad_args(gr);
    const T* go = static_cast<const T*>(dout);
    hipError_t err = launch_attn_delta(p.dtype, out, dout, gr.delta, p.B, p.H, p.Nq, stream);
    if (err != hipSuccess) return err;
    spf_attn16_dq_kernel<T><<<dim3(attn_blocks(p.Nq), p.H, p.B), kBlock, 0, stream>>>(a, g, go, lse, gr.delta);
    err = hipGetLastError();
    if (err != hipSuccess) return err;
    spf_attn16_dkdv_kernel<T><<<dim3(attn_blocks(p.Nk), p.H, p.B), kBlock, 0, stream>>>(a, g, go, lse, gr.delta);
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
