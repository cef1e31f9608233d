// Fused RoPE attention for gfx950, head dim 64: forward and backward of
//   out = softmax(scale * R(qpos) q * (R(kpos) k)^T) * v
// (croco/blocks.py Attention.forward / CrossAttention.forward without mask and dropout).  The score matrix never
// exists in memory and the rotation costs no pass of its own: q and k are rotated while they are staged.
//
// Arithmetic: every product runs on v_mfma_f32_32x32x2_f32 (exact float32 fma chains), the softmax in float32;
// float16 / bfloat16 operands are converted when they are loaded and stored -- one compute path.
//
// Tiles.  A block is 4 waves; a wave owns 32 rows of the block's 128 ("owner" rows: queries in the forward and in
// the dq pass, keys in the dk/dv pass) and keeps them, rotated, in 32 registers per operand as the B operand of the
// matrix instruction (lane l: row l & 31, elements d = 2 s + (l >> 5), s < 32).  The other side is walked in tiles of
// 32 rows staged in LDS (pitch 65 floats: a column read by 32 lanes and a row read by 32 lanes are both free of bank
// conflicts); the next tile's global loads are in flight under the current tile's matrix instructions.
//
// The score tile is computed TRANSPOSED with respect to the owner: X = staged * owner^T, so the owner's row is the
// accumulator's column, which lives on ONE lane (and its partner l ^ 32): C/D map of the 32 x 32 tile: column =
// lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  Row-wise softmax statistics are then per lane (one exchange
// with lane ^ 32), and the second product Y = staged^T * X sums over X's ROW index, so X's registers are its B operand
// as they are: register r of lane half h is row rowbase(r) + 4 h, i.e. k-step r pairs rows (i, i + 4).  No LDS round
// trip for the probabilities.
//
// Backward: no atomics.  spf_attn_dkdv_kernel owns key rows and loops over query tiles; spf_attn_dq_kernel owns query
// rows and loops over key tiles; both recompute the probabilities from the saved log-sum-exp.  The row term
// delta = sum_d dout * out is a small pre-pass, which the dq pass (run first) refines to sum_j p dP for the dk/dv pass.
// Every sum has a fixed order: results are bitwise reproducible.
//
// Two compile-time features serve vggt/layers/attention.py (template flags: without them the kernels are the code above):
// MASK adds mask[b,h,q,k] (float32, or bool as 0 / -inf; read in place through strides) to the score, with -inf safe in
// the online softmax and in both recomputations -- a row without any key gives out = 0, lse = -inf and zero gradients;
// NORM applies LayerNorm(64) with weight and bias to every q and k row while it is staged, before the rotation, and its
// backward in the epilogues of the two backward passes, with the parameter gradients summed from per-block partials.
// The host part at the end is one path for every call: the extras are a nullable SpfAttnExt, and one dispatch picks the
// instantiation from (element type, mask present, norm present) for both directions.
//
// A third feature, VIEWS (plain only: neither MASK nor NORM), serves the multi-view decoder's cross-attention: a batch
// item of the owner side is a (scene, view) pair, the keys of a scene are ONE [Vk] set of views shared by all of that
// scene's query views, and query view i reads key view s iff bit s of a host-known word allow[i] is set.  The walk over
// the other side becomes a walk over the allowed views in ascending order and, inside, over each view's tiles; an
// excluded view is never loaded.  Everything about views is a function of blockIdx and kernel arguments: scalar registers.
//
// attention_tiles.h holds what this file shares with attention16.hip: the tile sizes, AttnArgs / AttnGradArgs and their
// fill, load4 / store4, Stage and stage_load, acc_row, unrotate_half and store_row.  This file owns the float32 LDS image
// (stage_commit, own_rows), everything of MASK, NORM and VIEWS, and the row-dot kernel, which attention16.hip launches
// through launch_attn_delta.
#include "attention_tiles.h"
#include "launchers.h"

namespace spf {

namespace {

constexpr int kAttnLd = 65;         // LDS pitch of a staged row, floats

// What the flagged instantiations read on top of AttnArgs.  MASK: score += mask[b,h,q,k], read in place through element
// strides (0: broadcast; the key stride is 1), float32 additive or uint8 (nonzero: the key takes part, zero: -inf).
// NORM: LayerNorm(64) with weight and bias of every q and every k row while it is staged, before the rotation.
// The unflagged instantiations keep AttnArgs as their argument: they are the code they were.
struct AttnExt {
    const void* mask;
    int64_t ms[3];                  // batch, head, query
    int mask_bool;
    const float *qw, *qb, *kw, *kb; // float[64] each
    float eps;
    float* part;                    // backward: this pass's [blocks][2][64] partial sums of (dweight, dbias)
};
struct AttnArgsX : AttnArgs {
    AttnExt x;
};
// What the VIEWS instantiations read on top of AttnArgs (B = scenes; qs[0] / ks[0] / vs[0] = the stride between scenes).
// words: forward and dq pass, [query view] = the key views it reads; dk/dv pass, [key view] = the query views that read it
// (the transpose, formed on the host).  Strides in elements; positions [scene][view][token][2] through two strides.
struct AttnViews {
    int Vq, Vk;
    uint32_t words[32];
    int64_t qv, kv, vv;             // between views
    int64_t qpb, qpv, kpb, kpv;     // positions: between scenes, between views
    int64_t dqv, dkv, dvv;          // gradients: between views (between scenes: AttnGradArgs' batch stride)
};
struct AttnArgsV : AttnArgs {
    AttnViews w;
};
template <bool X, bool V = false> struct ArgsOf { typedef AttnArgs type; };
template <> struct ArgsOf<true, false> { typedef AttnArgsX type; };
template <> struct ArgsOf<false, true> { typedef AttnArgsV type; };
// A word of views is walked by DISTANCE, so that a kernel keeps the pointers of the view it is loading and nothing else:
// `rest` holds the views above the current one, bit 0 = the next; this returns how many views ahead the next set one is
// (>= 1) and shifts it out.  Before the first view `rest` is the whole word, and the result minus 1 is that view.
__device__ __forceinline__ int view_step(uint32_t& rest) {
    const int d = __builtin_ctz(rest);
    rest = rest >> d >> 1;                              // (two shifts: d + 1 may be 32)
    return d + 1;
}

// rotate (rot) by +angle, scale by mult, write into the LDS image
__device__ __forceinline__ void stage_commit(const Stage& r, float* __restrict__ s_t, bool rot, const RopeFreq& f,
                                             float mult, int tid) {
    const int part = tid & 7, x = part >> 2, q0 = (part & 3) * 4;
    float* __restrict__ d = s_t + (tid >> 3) * kAttnLd + 32 * x + q0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float u = r.u[k], v = r.v[k];
        if (rot) {
            float sn, cs;
            rope_sincos(r.p * f.inv[q0 + k], sn, cs);
            // (explicit fused steps: every element type must round the rotation the same way)
            const float uo = fmaf(u, cs, -(v * sn)), vo = fmaf(v, cs, u * sn);
            u = uo; v = vo;
        }
        d[k] = u * mult;
        d[16 + k] = v * mult;
    }
}

// ---- NORM ----------------------------------------------------------------------------------------------------------
// The four parameter vectors in LDS: [0] q weight, [1] q bias, [2] k weight, [3] k bias (only kernels that call this
// carry the 1 KB).
__device__ __forceinline__ float* norm_lds() {
    __shared__ __attribute__((aligned(16))) float s_n[4 * kAttnD];
    return s_n;
}
__device__ __forceinline__ void norm_lds_fill(const AttnExt& x, int tid) {
    const float* __restrict__ src = tid < 64 ? x.qw : tid < 128 ? x.qb : tid < 192 ? x.kw : x.kb;
    norm_lds()[tid] = src[tid & 63];                    // (visible after the first barrier of own_rows)
}
// LayerNorm of the staged row in place: the 8 lanes that hold a row (tid & 7) exchange their sums; two passes (mean,
// then the squared distances to it), float32.  A row past the end becomes zeros, as it is without the norm.
__device__ __forceinline__ void stage_norm(Stage& r, const float* __restrict__ w, const float* __restrict__ b, float eps,
                                           bool valid, int tid) {
    const int part = tid & 7, x = part >> 2, q0 = (part & 3) * 4;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) sum += r.u[k] + r.v[k];
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) sum += __shfl_xor(sum, o, kWave);
    const float mean = sum * (1.f / kAttnD);
    float d2 = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float du = r.u[k] - mean, dv = r.v[k] - mean;
        d2 = fmaf(du, du, d2);
        d2 = fmaf(dv, dv, d2);
    }
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) d2 += __shfl_xor(d2, o, kWave);
    const float rstd = 1.f / sqrtf(d2 * (1.f / kAttnD) + eps);
    const int d = 32 * x + q0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.u[k] = valid ? fmaf((r.u[k] - mean) * rstd, w[d + k], b[d + k]) : 0.f;
        r.v[k] = valid ? fmaf((r.v[k] - mean) * rstd, w[d + 16 + k], b[d + 16 + k]) : 0.f;
    }
}

// ---- MASK ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mask_value(float m) { return m; }
__device__ __forceinline__ float mask_value(uint8_t m) { return m ? 0.f : -INFINITY; }

// A lane's 16 mask entries of a tile are loaded before the tile is committed to LDS (in flight under that work), parked
// in LDS (mask_park: every lane has 16 words of its own, [r][tid], free of bank conflicts) and added to the finished score
// (mask_add): the matrix instructions in between run without 16 more live registers, and the score is
// round(scale q . k) + mask as the reference forms it -- a zero mask leaves the bits of the unmasked product.
__device__ __forceinline__ float* mask_lds() {
    __shared__ float s_m[16 * kBlock];
    return s_m;
}
__device__ __forceinline__ void mask_park(const f16v& mv, int tid) {
#pragma unroll
    for (int r = 0; r < 16; ++r) mask_lds()[r * kBlock + tid] = mv[r];
}
__device__ __forceinline__ void mask_add(f16v& s, int tid) {
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] += mask_lds()[r * kBlock + tid];
}
// Forward and dq pass: register r is key i0 + acc_row(r, kl) of the lane's mask row `row` (runs of 4 consecutive keys).
// Dwords (or bytes): no alignment is assumed.  FULL: the tile lies inside the matrix and the loads are unconditional; else entries past the end are 0 (the
// padding rules of the passes deal with those).  A lane without a row of its own is handed an existing one: what it
// computes is never stored.
template <typename M, bool FULL>
__device__ __forceinline__ void mask_tile_t(f16v& mv, const M* __restrict__ row, int i0, int n, int kl) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = i0 + acc_row(r, kl);
        mv[r] = (FULL || i < n) ? mask_value(row[i]) : 0.f;
    }
}
__device__ __forceinline__ void mask_tile(f16v& mv, const AttnExt& x, int64_t off, int i0, int n, int kl) {
    const bool full = i0 + kAttnT <= n;                 // (both conditions are wave-uniform)
    if (x.mask_bool) {
        const uint8_t* __restrict__ row = static_cast<const uint8_t*>(x.mask) + off;
        if (full) mask_tile_t<uint8_t, true>(mv, row, i0, n, kl);
        else mask_tile_t<uint8_t, false>(mv, row, i0, n, kl);
    } else {
        const float* __restrict__ row = static_cast<const float*>(x.mask) + off;
        if (full) mask_tile_t<float, true>(mv, row, i0, n, kl);
        else mask_tile_t<float, false>(mv, row, i0, n, kl);
    }
}
// The same for a lane that owns a key and walks queries (dk/dv pass): register r is query i0 + acc_row(r, kl) at the
// lane's key.  A mask row starts at a wave-uniform address; a lane picks the row of its half (kl) and adds its key, so
// lanes consecutive in k coalesce.  No branch per load: a query past the end reads the last row instead (its
// probability is 0 through its log-sum-exp of +inf, whatever the mask says), a lane past the last key the last key
// (what it computes is never stored).
template <typename M>
__device__ __forceinline__ void mask_tile_cols_t(f16v& mv, const M* __restrict__ base, int64_t step, int key, int i0, int n,
                                                 int kl) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int rr = i0 + (r & 3) + 8 * (r >> 2);
        const M* __restrict__ r0 = base + min(rr, n - 1) * step;
        const M* __restrict__ r1 = base + min(rr + 4, n - 1) * step;
        mv[r] = mask_value((kl ? r1 : r0)[key]);
    }
}
__device__ __forceinline__ void mask_tile_cols(f16v& mv, const AttnExt& x, int64_t off, int key, int i0, int n, int kl) {
    if (x.mask_bool) mask_tile_cols_t(mv, static_cast<const uint8_t*>(x.mask) + off, x.ms[2], key, i0, n, kl);
    else mask_tile_cols_t(mv, static_cast<const float*>(x.mask) + off, x.ms[2], key, i0, n, kl);
}

// The rows a wave owns, as B operands: stage the block's 128 rows 32 at a time through s_a (and s_b for a second
// operand with the same rows), each wave keeps its own chunk.
template <typename T, bool NORM = false>
__device__ __forceinline__ void own_rows(float (&ra)[32], const T* __restrict__ a, int64_t a_sn, const int64_t* __restrict__ pos,
                                         float mult, float (&rb)[32], const T* __restrict__ b, int64_t b_sn, int row0, int N,
                                         float* __restrict__ s_a, float* __restrict__ s_b, const RopeFreq& f, int tid,
                                         const float* __restrict__ nw = nullptr, float eps = 0.f) {
    const int lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        Stage sa, sb;
        stage_load<T>(sa, a, a_sn, pos, row0 + kAttnT * w, N, tid);
        if (b) stage_load<T>(sb, b, b_sn, nullptr, row0 + kAttnT * w, N, tid);
        __syncthreads();
        if constexpr (NORM) stage_norm(sa, nw, nw + kAttnD, eps, row0 + kAttnT * w + (tid >> 3) < N, tid);
        stage_commit(sa, s_a, pos != nullptr, f, mult, tid);
        if (b) stage_commit(sb, s_b, false, f, 1.f, tid);
        __syncthreads();
        if (w == wave) {
#pragma unroll
            for (int s = 0; s < 32; ++s) {
                ra[s] = s_a[il * kAttnLd + 2 * s + kl];
                if (b) rb[s] = s_b[il * kAttnLd + 2 * s + kl];
            }
        }
    }
}

// ---- forward -------------------------------------------------------------------------------------------------------
// VIEWS: b = (scene, query view) is the batch item of out and lse; the keys walked are the views of word a.w.words[view]
// of the scene, in ascending order.  kb, vb, kp then point at the view being LOADED (the prefetch runs one tile ahead and
// hops to the next allowed view when the current one is used up), which nothing after a tile's commit depends on.
template <typename T, bool MASK = false, bool NORM = false, bool VIEWS = false>
__global__ __launch_bounds__(kBlock) void spf_attn_fwd_kernel(typename ArgsOf<MASK || NORM, VIEWS>::type a, T* __restrict__ out,
                                                              float* __restrict__ lse) {
    static_assert(!(VIEWS && (MASK || NORM)), "VIEWS is plain only");
    __shared__ float s_k[kAttnT * kAttnLd];
    __shared__ float s_v[kAttnT * kAttnLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kAttnOwn;
    int sb = b;                                         // the batch item of q, k, v: the scene when VIEWS
    if constexpr (VIEWS) sb = b / a.w.Vq;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + sb * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + sb * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + sb * a.vs[0] + h * a.vs[2];
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;
    [[maybe_unused]] uint32_t rest = 0;                 // VIEWS: the allowed views not yet loaded
    [[maybe_unused]] bool more = false;                 // VIEWS: a next view's first tile is in flight
    if constexpr (VIEWS) {
        const int vi = b - sb * a.w.Vq;
        qb += vi * a.w.qv;
        qp = a.qpos ? a.qpos + sb * a.w.qpb + vi * a.w.qpv : nullptr;
        rest = a.w.words[vi];                           // (never 0: the host refuses a query view without keys)
        const int s = view_step(rest) - 1;
        kb += s * a.w.kv;
        vb += s * a.w.vv;
        kp = a.kpos ? a.kpos + sb * a.w.kpb + s * a.w.kpv : nullptr;
    }

    float qr[32], unused[32];
    if constexpr (NORM) {
        norm_lds_fill(a.x, tid);
        own_rows<T, true>(qr, qb, a.qs[1], qp, a.scale, unused, nullptr, 0, q0, a.Nq, s_k, s_v, a.f, tid, norm_lds(), a.x.eps);
    } else {
        own_rows<T>(qr, qb, a.qs[1], qp, a.scale, unused, nullptr, 0, q0, a.Nq, s_k, s_v, a.f, tid);
    }
    const bool active = q0 + kAttnT * wave < a.Nq;      // wave-uniform: a wave without queries only helps staging
    const int qi = q0 + kAttnT * wave + il;
    int64_t moff = 0;                                   // MASK: this lane's row of the mask
    if constexpr (MASK) moff = b * a.x.ms[0] + h * a.x.ms[1] + min(qi, a.Nq - 1) * a.x.ms[2];

    f16v o0, o1;
#pragma unroll
    for (int e = 0; e < 16; ++e) o0[e] = o1[e] = 0.f;
    float m = -INFINITY, l = 0.f;
    Stage sk, sv;
    stage_load<T>(sk, kb, a.ks[1], kp, 0, a.Nk, tid);
    stage_load<T>(sv, vb, a.vs[1], nullptr, 0, a.Nk, tid);
#pragma unroll 1
    do {                                                // VIEWS: one round per allowed view; else one round
#pragma unroll 1
    for (int k0 = 0; k0 < a.Nk; k0 += kAttnT) {
        f16v s;                                         // S^T: rows = keys, column = this lane's query
        if constexpr (MASK) {
            if (active) mask_tile(s, a.x, moff, k0, a.Nk, kl);
        }
        __syncthreads();                                // the previous tile's readers are done
        if constexpr (MASK) {
            if (active) mask_park(s, tid);
        }
        if constexpr (NORM) stage_norm(sk, norm_lds() + 2 * kAttnD, norm_lds() + 3 * kAttnD, a.x.eps, k0 + (tid >> 3) < a.Nk, tid);
        stage_commit(sk, s_k, kp != nullptr, a.f, 1.f, tid);
        stage_commit(sv, s_v, false, a.f, 1.f, tid);
        __syncthreads();
        if constexpr (VIEWS) {                          // the next tile: of this view, or the first of the next allowed one
            int n0 = k0 + kAttnT;
            if (n0 >= a.Nk) {                           // the view is used up: hop (scalar work only)
                more = rest != 0;
                if (more) {
                    const int d = view_step(rest);
                    kb += d * a.w.kv;
                    vb += d * a.w.vv;
                    if (kp) kp += d * a.w.kpv;
                    n0 = 0;
                }
            }
            if (n0 < a.Nk) {                            // ONE load site: in flight under the matrix instructions below
                stage_load<T, true>(sk, kb, a.ks[1], kp, n0, a.Nk, tid);
                stage_load<T, true>(sv, vb, a.vs[1], nullptr, n0, a.Nk, tid);
            }
        } else if (k0 + kAttnT < a.Nk) {                // in flight under the matrix instructions below
            stage_load<T>(sk, kb, a.ks[1], kp, k0 + kAttnT, a.Nk, tid);
            stage_load<T>(sv, vb, a.vs[1], nullptr, k0 + kAttnT, a.Nk, tid);
        }
        if (!active) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 32; ++st)
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(s_k[il * kAttnLd + 2 * st + kl], qr[st], s, 0, 0, 0);
        if constexpr (MASK) mask_add(s, tid);
        if (k0 + kAttnT > a.Nk) {                       // padded keys: probability 0
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (k0 + acc_row(r, kl) >= a.Nk) s[r] = -INFINITY;
        }
        float tmax = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, kWave));
        const float mn = fmaxf(m, tmax);                // finite: every tile holds at least one key -- unless MASK:
        float mref = mn;                                // while every key so far is masked the maximum is still -inf;
        if constexpr (MASK) mref = mn == -INFINITY ? 0.f : mn;      // exp(-inf - 0) = 0 then, where -inf - -inf is NaN
        const float alpha = expf(m - mref);
        m = mn;
        float ps = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            s[r] = expf(s[r] - mref);
            ps += s[r];
        }
        l = l * alpha + ps;
#pragma unroll
        for (int e = 0; e < 16; ++e) { o0[e] *= alpha; o1[e] *= alpha; }
#pragma unroll
        for (int r = 0; r < 16; ++r) {                  // O^T += V^T P^T: k-step r pairs keys (i, i + 4)
            const float* __restrict__ vrow = s_v + acc_row(r, kl) * kAttnLd + il;
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[0], s[r], o0, 0, 0, 0);
            o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32], s[r], o1, 0, 0, 0);
        }
    }
    } while (VIEWS && more);
    if (!active) return;
    const float lt = l + __shfl_xor(l, 32, kWave);
    if (qi >= a.Nq) return;
    float row_lse = m + logf(lt), inv = 1.f / lt;
    if constexpr (MASK) {
        if (!(lt > 0.f)) { row_lse = -INFINITY; inv = 0.f; }       // every key masked: out = 0, lse = -inf
    }
    if (kl == 0) lse[((int64_t)b * a.H + h) * a.Nq + qi] = row_lse;
    store_row<T>(out + (((int64_t)b * a.Nq + qi) * a.H + h) * kAttnD, o0, o1, inv, nullptr, a.f, kl);
}

// ---- backward ------------------------------------------------------------------------------------------------------
// NORM epilogue of an owner row.  a0 / a1: the gradient with respect to the normalised row y = x^ gamma + beta, un-rotated
// (this lane: elements d = 32 x + acc_row(r, kl) of row il; its partner lane ^ 32 holds the rest).  The row's mean and
// rstd are recomputed from the input row `xrow` (two passes), then
//   dx = rstd (g^ - mean(g^) - x^ mean(g^ x^)),  g^ = g gamma
// is stored at `dst`, and the block's 128 rows of (g x^, g) are added per column in a fixed order -- wave by wave
// through the tile buffers, rows ascending, in double -- into part[2][64] (float32: one rounding per block).  EVERY thread of the block calls this (barriers); a row
// that does not exist has valid = false and adds zeros.
template <typename T>
__device__ __forceinline__ void norm_backward_row(T* __restrict__ dst, const T* __restrict__ xrow, f16v a0, f16v a1,
                                                  const float* __restrict__ gamma, float eps, bool valid,
                                                  float* __restrict__ s_a, float* __restrict__ s_b,
                                                  float* __restrict__ part, int tid) {
    const int lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    float xh[32], g[32];
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        g[i] = valid ? (i < 16 ? a0[i & 15] : a1[i & 15]) : 0.f;
        xh[i] = 0.f;
    }
    if (valid) {
#pragma unroll
        for (int gq = 0; gq < 8; ++gq) load4<T>(xrow + 32 * (gq >> 2) + 8 * (gq & 3) + 4 * kl, xh + 4 * gq);
    }
    // The row statistics and the three-term difference below in double (64 elements per row, once per row: the cost is
    // nothing): each stored element then carries one rounding of its own instead of the roundings of two float32 means.
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) sum += (double)xh[i];
    sum += __shfl_xor(sum, 32, kWave);
    const double mean = sum * (1.0 / kAttnD);
    double d2 = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const double d = (double)xh[i] - mean;
        d2 = fma(d, d, d2);
    }
    d2 += __shfl_xor(d2, 32, kWave);
    const double rstd = 1.0 / sqrt(d2 * (1.0 / kAttnD) + (double)eps);
    double m1 = 0.0, m2 = 0.0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        xh[i] = (float)(((double)xh[i] - mean) * rstd);
        const double gh = (double)g[i] * (double)gamma[32 * (i >> 4) + acc_row(i & 15, kl)];
        m1 += gh;
        m2 = fma(gh, (double)xh[i], m2);
    }
    m1 += __shfl_xor(m1, 32, kWave);
    m2 += __shfl_xor(m2, 32, kWave);
    m1 *= 1.0 / kAttnD;
    m2 *= 1.0 / kAttnD;
    if (valid) {
#pragma unroll
        for (int gq = 0; gq < 8; ++gq) {
            float dx[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int i = 4 * gq + e;
                const double gh = (double)g[i] * (double)gamma[32 * (i >> 4) + acc_row(i & 15, kl)];
                dx[e] = (float)(rstd * (gh - m1 - (double)xh[i] * m2));
            }
            store4<T>(dst + 32 * (gq >> 2) + 8 * (gq & 3) + 4 * kl, dx[0], dx[1], dx[2], dx[3]);
        }
    }
    double acc = 0.0;                                   // (128 terms a column: double costs nothing and rounds once)
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        __syncthreads();                                // the tile loop's (or the previous wave's) readers are done
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int d = 32 * (i >> 4) + acc_row(i & 15, kl);
                s_a[il * kAttnLd + d] = xh[i];
                s_b[il * kAttnLd + d] = g[i];
            }
        }
        __syncthreads();
        if (tid < 2 * kAttnD) {
            const int col = tid & 63;
#pragma unroll 8
            for (int row = 0; row < kAttnT; ++row) {
                const double gv = (double)s_b[row * kAttnLd + col];
                acc = tid < kAttnD ? fma(gv, (double)s_a[row * kAttnLd + col], acc) : acc + gv;
            }
        }
    }
    if (tid < 2 * kAttnD) part[tid] = (float)acc;
}

// dweight, dbias [64] = the partials of all blocks added in block order, in double: one block of 256 lanes, lane =
// (half of the blocks, which of the two, column); the two halves meet in LDS.  Fixed order: reproducible.
__global__ __launch_bounds__(kBlock) void spf_attn_norm_reduce_kernel(const float* __restrict__ part, int nblk,
                                                                      float* __restrict__ dw, float* __restrict__ db) {
    __shared__ double s_sum[kBlock];
    const int tid = threadIdx.x, seg = tid >> 7, per = (nblk + 1) / 2;
    const int end = min(nblk, (seg + 1) * per);
    double sum = 0.0;
    for (int i = seg * per; i < end; ++i) sum += (double)part[(int64_t)i * 2 * kAttnD + (tid & 127)];
    s_sum[tid] = sum;
    __syncthreads();
    if (tid < 2 * kAttnD) (tid >> 6 ? db : dw)[tid & 63] = (float)(s_sum[tid] + s_sum[tid + 128]);
}

// delta[b,h,q] = sum_d dout[b,q,h,d] * out[b,q,h,d], one lane per row: ONE fma chain over d in ascending order, which
// is bit for bit how the matrix instruction accumulates dP = dout . v in the two passes below -- where a row attends
// to a single key (out = v exactly) dP - delta is then exactly zero, as it is in exact arithmetic.
template <typename T>
__global__ __launch_bounds__(kBlock) void spf_attn_delta_kernel(const T* __restrict__ out, const T* __restrict__ dout,
                                                                float* __restrict__ delta, int B, int H, int Nq) {
    const int64_t rows = (int64_t)B * Nq * H, row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= rows) return;
    float acc = 0.f;
#pragma unroll
    for (int part = 0; part < 16; ++part) {
        float o[4], g[4];
        load4<T>(out + row * kAttnD + 4 * part, o);
        load4<T>(dout + row * kAttnD + 4 * part, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = fmaf(g[e], o[e], acc);
    }
    const int64_t bq = row / H;
    const int h = (int)(row - bq * H);
    const int64_t b = bq / Nq;
    delta[(b * H + h) * Nq + (bq - b * Nq)] = acc;
}

// dk, dv: the block owns 128 keys, walks the queries.
// VIEWS: b = (scene, key view); the queries walked are those of the views in a.w.words[key view], ascending, then each
// view's tiles ascending -- one fixed order, each dk / dv row written once.  A key view nobody reads walks nothing and
// stores the zeros the accumulators start from.
template <typename T, bool MASK = false, bool NORM = false, bool VIEWS = false>
__global__ __launch_bounds__(kBlock, 2) void spf_attn_dkdv_kernel(typename ArgsOf<MASK || NORM, VIEWS>::type a, AttnGradArgs g,
                                                               const T* __restrict__ dout,
                                                               const float* __restrict__ lse,
                                                               const float* __restrict__ delta) {
    __shared__ float s_q[kAttnT * kAttnLd];
    __shared__ float s_do[kAttnT * kAttnLd];
    __shared__ float s_lse[kAttnT], s_dl[kAttnT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    static_assert(!(VIEWS && (MASK || NORM)), "VIEWS is plain only");
    const int b = blockIdx.z, h = blockIdx.y, k0 = blockIdx.x * kAttnOwn;
    int sb = b;                                         // the batch item of q, k, v: the scene when VIEWS
    if constexpr (VIEWS) sb = b / a.w.Vk;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + sb * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + sb * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + sb * a.vs[0] + h * a.vs[2];
    const T* __restrict__ gb = dout + ((int64_t)b * a.Nq * a.H + h) * kAttnD;
    const int64_t g_sn = (int64_t)a.H * kAttnD;
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;
    const float* __restrict__ lse_r = lse + ((int64_t)b * a.H + h) * a.Nq;
    const float* __restrict__ dl_r = delta + ((int64_t)b * a.H + h) * a.Nq;
    [[maybe_unused]] uint32_t rest = 0;                 // VIEWS: the reading query views not yet loaded
    [[maybe_unused]] bool more = false;                 // VIEWS: a next view's first tile is in flight
    // VIEWS: move the query side (q, its positions, dout, lse, delta) d query views ahead
    [[maybe_unused]] auto hop = [&](int d) {
        if constexpr (VIEWS) {
            const int64_t rows = (int64_t)d * a.H * a.Nq;       // (dout, lse and delta are contiguous)
            qb += d * a.w.qv;
            if (qp) qp += d * a.w.qpv;
            gb += rows * kAttnD;
            lse_r += rows;
            dl_r += rows;
        }
    };
    if constexpr (VIEWS) {
        const int kview = b - sb * a.w.Vk;
        const int64_t bq = (int64_t)sb * a.w.Vq;        // query view 0 of the scene
        kb += kview * a.w.kv;
        vb += kview * a.w.vv;
        kp = a.kpos ? a.kpos + sb * a.w.kpb + kview * a.w.kpv : nullptr;
        qp = a.qpos ? a.qpos + sb * a.w.qpb : nullptr;
        gb = dout + (bq * a.Nq * a.H + h) * kAttnD;
        lse_r = lse + (bq * a.H + h) * a.Nq;
        dl_r = delta + (bq * a.H + h) * a.Nq;
        rest = a.w.words[kview];
        more = rest != 0;                               // (0: nobody reads this view)
        if (more) hop(view_step(rest) - 1);
    }

    float kr[32], vr[32];
    if constexpr (NORM) {
        norm_lds_fill(a.x, tid);
        own_rows<T, true>(kr, kb, a.ks[1], kp, 1.f, vr, vb, a.vs[1], k0, a.Nk, s_q, s_do, a.f, tid, norm_lds() + 2 * kAttnD,
                          a.x.eps);
    } else {
        own_rows<T>(kr, kb, a.ks[1], kp, 1.f, vr, vb, a.vs[1], k0, a.Nk, s_q, s_do, a.f, tid);
    }
    const bool active = k0 + kAttnT * wave < a.Nk;
    [[maybe_unused]] int okey = 0;                      // (flagged only: the unflagged pass forms its key at the end)
    if constexpr (MASK || NORM) okey = k0 + kAttnT * wave + il;

    f16v dk0, dk1, dv0, dv1;
#pragma unroll
    for (int e = 0; e < 16; ++e) dk0[e] = dk1[e] = dv0[e] = dv1[e] = 0.f;
    Stage sq, sd;
    float rl = INFINITY, rd = 0.f;                      // a padded query: probability 0
    if (!VIEWS || more) {
    stage_load<T>(sq, qb, a.qs[1], qp, 0, a.Nq, tid);
    stage_load<T>(sd, gb, g_sn, nullptr, 0, a.Nq, tid);
    if (tid < kAttnT && tid < a.Nq) { rl = lse_r[tid]; rd = dl_r[tid]; }
#pragma unroll 1
    do {                                                // VIEWS: one round per reading query view; else one round
#pragma unroll 1
    for (int q0 = 0; q0 < a.Nq; q0 += kAttnT) {
        f16v s, dp;                                     // S, dP: rows = queries, column = this lane's key
        if constexpr (MASK) {
            if (active)
                mask_tile_cols(s, a.x, b * a.x.ms[0] + h * a.x.ms[1], min(okey, a.Nk - 1), q0, a.Nq, kl);
        }
        __syncthreads();
        if constexpr (MASK) {
            if (active) mask_park(s, tid);
        }
        if constexpr (NORM) stage_norm(sq, norm_lds(), norm_lds() + kAttnD, a.x.eps, q0 + (tid >> 3) < a.Nq, tid);
        stage_commit(sq, s_q, qp != nullptr, a.f, a.scale, tid);
        stage_commit(sd, s_do, false, a.f, 1.f, tid);
        if (tid < kAttnT) { s_lse[tid] = rl; s_dl[tid] = rd; }
        __syncthreads();
        if constexpr (VIEWS) {                          // the next tile: of this view, or the first of the next reading one
            int n0 = q0 + kAttnT;
            if (n0 >= a.Nq) {                           // the view is used up: hop (scalar work only)
                more = rest != 0;
                if (more) {
                    hop(view_step(rest));
                    n0 = 0;
                }
            }
            if (n0 < a.Nq) {                            // ONE load site
                stage_load<T, true>(sq, qb, a.qs[1], qp, n0, a.Nq, tid);
                stage_load<T, true>(sd, gb, g_sn, nullptr, n0, a.Nq, tid);
                rl = INFINITY; rd = 0.f;
                if (tid < kAttnT && n0 + tid < a.Nq) { rl = lse_r[n0 + tid]; rd = dl_r[n0 + tid]; }
            }
        } else if (q0 + kAttnT < a.Nq) {
            stage_load<T>(sq, qb, a.qs[1], qp, q0 + kAttnT, a.Nq, tid);
            stage_load<T>(sd, gb, g_sn, nullptr, q0 + kAttnT, a.Nq, tid);
            rl = INFINITY; rd = 0.f;
            if (tid < kAttnT && q0 + kAttnT + tid < a.Nq) { rl = lse_r[q0 + kAttnT + tid]; rd = dl_r[q0 + kAttnT + tid]; }
        }
        if (!active) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 32; ++st) {
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(s_q[il * kAttnLd + 2 * st + kl], kr[st], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(s_do[il * kAttnLd + 2 * st + kl], vr[st], dp, 0, 0, 0);
        }
        if constexpr (MASK) mask_add(s, tid);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = acc_row(r, kl);
            float p = expf(s[r] - s_lse[row]);
            if constexpr (MASK) p = s[r] == -INFINITY ? 0.f : p;    // (a fully masked row has lse = -inf: -inf - -inf)
            s[r] = p;
            dp[r] = p * (dp[r] - s_dl[row]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {                  // dV^T += dO^T P, dK^T += Qs^T dS
            const int row = acc_row(r, kl);
            const float* __restrict__ grow = s_do + row * kAttnLd + il;
            const float* __restrict__ qrow = s_q + row * kAttnLd + il;
            dv0 = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[0], s[r], dv0, 0, 0, 0);
            dv1 = __builtin_amdgcn_mfma_f32_32x32x2f32(grow[32], s[r], dv1, 0, 0, 0);
            dk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[0], dp[r], dk0, 0, 0, 0);
            dk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(qrow[32], dp[r], dk1, 0, 0, 0);
        }
    }
    } while (VIEWS && more);
    }
    if constexpr (NORM) {
        const int key = okey;
        const bool valid = active && key < a.Nk;
        T* __restrict__ dv_row = static_cast<T*>(g.dv) + b * g.dvs[0] + (int64_t)key * g.dvs[1] + h * g.dvs[2];
        T* __restrict__ dk_row = static_cast<T*>(g.dk) + b * g.dks[0] + (int64_t)key * g.dks[1] + h * g.dks[2];
        if (valid) store_row<T>(dv_row, dv0, dv1, 1.f, nullptr, a.f, kl);
        if (valid && kp) {
            unrotate_half(dk0, (float)kp[(int64_t)key * 2], a.f, kl);
            unrotate_half(dk1, (float)kp[(int64_t)key * 2 + 1], a.f, kl);
        }
        norm_backward_row<T>(dk_row, kb + (int64_t)key * a.ks[1], dk0, dk1, norm_lds() + 2 * kAttnD, a.x.eps, valid, s_q, s_do,
                             a.x.part + (((int64_t)b * a.H + h) * gridDim.x + blockIdx.x) * 2 * kAttnD, tid);
    } else {
        if (!active) return;
        const int key = k0 + kAttnT * wave + il;
        if (key >= a.Nk) return;
        int64_t dv_view = 0, dk_view = 0;
        if constexpr (VIEWS) { dv_view = (b - sb * a.w.Vk) * a.w.dvv; dk_view = (b - sb * a.w.Vk) * a.w.dkv; }
        store_row<T>(static_cast<T*>(g.dv) + sb * g.dvs[0] + dv_view + (int64_t)key * g.dvs[1] + h * g.dvs[2], dv0, dv1, 1.f, nullptr, a.f, kl);
        store_row<T>(static_cast<T*>(g.dk) + sb * g.dks[0] + dk_view + (int64_t)key * g.dks[1] + h * g.dks[2], dk0, dk1, 1.f,
                     kp ? kp + (int64_t)key * 2 : nullptr, a.f, kl);
    }
}

// dq: the block owns 128 queries, walks the keys.  It also settles the row term.  `delta` comes in as sum_d dout * out
// (delta~), whose rounding is independent of the roundings of the recomputed dP[j]; where a row's probability sits on few
// keys with large |k|, p (dP - delta~) then keeps an error that sum_j p[j] (dP[j] - delta) k[j] would cancel.  So the pass
// accumulates c = sum_j p[j] (dP[j] - delta~) (tiny: the residual of delta~) and B = sum_j p[j] k[j] next to
// A = sum_j p[j] (dP[j] - delta~) k[j], returns dq = scale (A - c B) -- the gradient with delta = sum_j p[j] dP[j], the
// softmax backward's own row sum -- and writes delta~ + c back for the dk/dv pass, which recomputes the same dP bits.
// VIEWS: as in the forward -- b = (scene, query view), the keys are the allowed views' in ascending order.
template <typename T, bool MASK = false, bool NORM = false, bool VIEWS = false>
__global__ __launch_bounds__(kBlock, 2) void spf_attn_dq_kernel(typename ArgsOf<MASK || NORM, VIEWS>::type a, AttnGradArgs g,
                                                             const T* __restrict__ dout,
                                                             const float* __restrict__ lse,
                                                             float* __restrict__ delta) {
    __shared__ float s_k[kAttnT * kAttnLd];
    __shared__ float s_v[kAttnT * kAttnLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, il = lane & 31, kl = lane >> 5;
    static_assert(!(VIEWS && (MASK || NORM)), "VIEWS is plain only");
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * kAttnOwn;
    int sb = b;                                         // the batch item of q, k, v: the scene when VIEWS
    if constexpr (VIEWS) sb = b / a.w.Vq;
    const T* __restrict__ qb = static_cast<const T*>(a.q) + sb * a.qs[0] + h * a.qs[2];
    const T* __restrict__ kb = static_cast<const T*>(a.k) + sb * a.ks[0] + h * a.ks[2];
    const T* __restrict__ vb = static_cast<const T*>(a.v) + sb * a.vs[0] + h * a.vs[2];
    const T* __restrict__ gb = dout + ((int64_t)b * a.Nq * a.H + h) * kAttnD;
    const int64_t* __restrict__ qp = a.qpos ? a.qpos + (int64_t)b * a.Nq * 2 : nullptr;
    const int64_t* __restrict__ kp = a.kpos ? a.kpos + (int64_t)b * a.Nk * 2 : nullptr;
    [[maybe_unused]] uint32_t rest = 0;                 // VIEWS: the allowed views not yet loaded
    [[maybe_unused]] bool more = false;                 // VIEWS: a next view's first tile is in flight
    if constexpr (VIEWS) {
        const int vi = b - sb * a.w.Vq;
        qb += vi * a.w.qv;
        qp = a.qpos ? a.qpos + sb * a.w.qpb + vi * a.w.qpv : nullptr;
        rest = a.w.words[vi];                           // (never 0: the host refuses a query view without keys)
        const int s = view_step(rest) - 1;
        kb += s * a.w.kv;
        vb += s * a.w.vv;
        kp = a.kpos ? a.kpos + sb * a.w.kpb + s * a.w.kpv : nullptr;
    }

    float qr[32], gr[32];
    if constexpr (NORM) {
        norm_lds_fill(a.x, tid);
        own_rows<T, true>(qr, qb, a.qs[1], qp, a.scale, gr, gb, (int64_t)a.H * kAttnD, q0, a.Nq, s_k, s_v, a.f, tid, norm_lds(),
                          a.x.eps);
    } else {
        own_rows<T>(qr, qb, a.qs[1], qp, a.scale, gr, gb, (int64_t)a.H * kAttnD, q0, a.Nq, s_k, s_v, a.f, tid);
    }
    const bool active = q0 + kAttnT * wave < a.Nq;
    const int qi = q0 + kAttnT * wave + il;
    int64_t moff = 0;                                   // MASK: this lane's row of the mask
    if constexpr (MASK) moff = b * a.x.ms[0] + h * a.x.ms[1] + min(qi, a.Nq - 1) * a.x.ms[2];
    float my_lse = INFINITY, my_dl = 0.f;
    if (qi < a.Nq) {
        my_lse = lse[((int64_t)b * a.H + h) * a.Nq + qi];
        my_dl = delta[((int64_t)b * a.H + h) * a.Nq + qi];
    }

    f16v dq0, dq1, pk0, pk1;
#pragma unroll
    for (int e = 0; e < 16; ++e) dq0[e] = dq1[e] = pk0[e] = pk1[e] = 0.f;
    float cres = 0.f;
    Stage sk, sv;
    stage_load<T>(sk, kb, a.ks[1], kp, 0, a.Nk, tid);
    stage_load<T>(sv, vb, a.vs[1], nullptr, 0, a.Nk, tid);
#pragma unroll 1
    do {                                                // VIEWS: one round per allowed view; else one round
#pragma unroll 1
    for (int k0 = 0; k0 < a.Nk; k0 += kAttnT) {
        f16v s, dp;                                     // S^T, dP^T: rows = keys, column = this lane's query
        if constexpr (MASK) {
            if (active) mask_tile(s, a.x, moff, k0, a.Nk, kl);
        }
        __syncthreads();
        if constexpr (MASK) {
            if (active) mask_park(s, tid);
        }
        if constexpr (NORM) stage_norm(sk, norm_lds() + 2 * kAttnD, norm_lds() + 3 * kAttnD, a.x.eps, k0 + (tid >> 3) < a.Nk, tid);
        stage_commit(sk, s_k, kp != nullptr, a.f, 1.f, tid);
        stage_commit(sv, s_v, false, a.f, 1.f, tid);
        __syncthreads();
        if constexpr (VIEWS) {                          // the next tile, as in the forward
            int n0 = k0 + kAttnT;
            if (n0 >= a.Nk) {
                more = rest != 0;
                if (more) {
                    const int d = view_step(rest);
                    kb += d * a.w.kv;
                    vb += d * a.w.vv;
                    if (kp) kp += d * a.w.kpv;
                    n0 = 0;
                }
            }
            if (n0 < a.Nk) {
                stage_load<T, true>(sk, kb, a.ks[1], kp, n0, a.Nk, tid);
                stage_load<T, true>(sv, vb, a.vs[1], nullptr, n0, a.Nk, tid);
            }
        } else if (k0 + kAttnT < a.Nk) {
            stage_load<T>(sk, kb, a.ks[1], kp, k0 + kAttnT, a.Nk, tid);
            stage_load<T>(sv, vb, a.vs[1], nullptr, k0 + kAttnT, a.Nk, tid);
        }
        if (!active) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
        for (int st = 0; st < 32; ++st) {
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(s_k[il * kAttnLd + 2 * st + kl], qr[st], s, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x2f32(s_v[il * kAttnLd + 2 * st + kl], gr[st], dp, 0, 0, 0);
        }
        if constexpr (MASK) mask_add(s, tid);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float p = expf(s[r] - my_lse);
            if (k0 + acc_row(r, kl) >= a.Nk) p = 0.f;   // padded keys
            if constexpr (MASK) p = s[r] == -INFINITY ? 0.f : p;    // (a fully masked row has lse = -inf: -inf - -inf)
            s[r] = p;
            dp[r] = p * (dp[r] - my_dl);
            cres += dp[r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {                  // A^T += Kr^T dS^T, B^T += Kr^T P^T
            const float* __restrict__ krow = s_k + acc_row(r, kl) * kAttnLd + il;
            const float k0v = krow[0], k1v = krow[32];
            dq0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0v, dp[r], dq0, 0, 0, 0);
            dq1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1v, dp[r], dq1, 0, 0, 0);
            pk0 = __builtin_amdgcn_mfma_f32_32x32x2f32(k0v, s[r], pk0, 0, 0, 0);
            pk1 = __builtin_amdgcn_mfma_f32_32x32x2f32(k1v, s[r], pk1, 0, 0, 0);
        }
    }
    } while (VIEWS && more);
    T* __restrict__ dq_row = static_cast<T*>(g.dq) + sb * g.dqs[0] + (int64_t)qi * g.dqs[1] + h * g.dqs[2];
    if constexpr (VIEWS) dq_row += (b - sb * a.w.Vq) * a.w.dqv;
    if constexpr (NORM) {
        const bool valid = active && qi < a.Nq;
        const float c = cres + __shfl_xor(cres, 32, kWave);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            dq0[e] = fmaf(-c, pk0[e], dq0[e]);
            dq1[e] = fmaf(-c, pk1[e], dq1[e]);
        }
        if (valid && kl == 0) delta[((int64_t)b * a.H + h) * a.Nq + qi] = my_dl + c;
        if (valid && qp) {
            unrotate_half(dq0, (float)qp[(int64_t)qi * 2], a.f, kl);
            unrotate_half(dq1, (float)qp[(int64_t)qi * 2 + 1], a.f, kl);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) { dq0[e] *= a.scale; dq1[e] *= a.scale; }
        norm_backward_row<T>(dq_row, qb + (int64_t)qi * a.qs[1], dq0, dq1, norm_lds(), a.x.eps, valid, s_k, s_v,
                             a.x.part + (((int64_t)b * a.H + h) * gridDim.x + blockIdx.x) * 2 * kAttnD, tid);
    } else {
        if (!active) return;
        const float c = cres + __shfl_xor(cres, 32, kWave);
        if (qi >= a.Nq) return;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            dq0[e] = fmaf(-c, pk0[e], dq0[e]);
            dq1[e] = fmaf(-c, pk1[e], dq1[e]);
        }
        if (kl == 0) delta[((int64_t)b * a.H + h) * a.Nq + qi] = my_dl + c;
        store_row<T>(dq_row, dq0, dq1, a.scale, qp ? qp + (int64_t)qi * 2 : nullptr, a.f, kl);
    }
}

// The kernels' argument of a call: AttnArgs, and for a flagged instantiation (X) the extras behind it.
template <bool X>
typename ArgsOf<X>::type make_args(const SpfAttn& p, [[maybe_unused]] const SpfAttnExt* e) {
    typename ArgsOf<X>::type a;
    static_cast<AttnArgs&>(a) = make_attn_args(p);
    if constexpr (X) {
        a.x.mask = e->mask;
        for (int i = 0; i < 3; ++i) a.x.ms[i] = e->mask_stride[i];
        a.x.mask_bool = e->mask_dtype != 0;
        a.x.qw = e->q_weight; a.x.qb = e->q_bias; a.x.kw = e->k_weight; a.x.kb = e->k_bias;
        a.x.eps = e->eps;
        a.x.part = nullptr;
    }
    return a;
}

template <typename T, bool MASK, bool NORM>
hipError_t attn_forward(const SpfAttn& p, const SpfAttnExt* e, void* out, float* lse, hipStream_t stream) {
    spf_attn_fwd_kernel<T, MASK, NORM><<<dim3(attn_blocks(p.Nq), p.H, p.B), kBlock, 0, stream>>>(
        make_args<MASK || NORM>(p, e), static_cast<T*>(out), lse);
    return hipGetLastError();
}

template <typename T, bool MASK, bool NORM>
hipError_t attn_backward(const SpfAttn& p, const SpfAttnGrads& gr, const SpfAttnExt* e, const void* out, const float* lse,
                         const void* dout, hipStream_t stream) {
    auto a = make_args<MASK || NORM>(p, e);
    const AttnGradArgs g = make_attn_grad_args(gr);
    const T* go = static_cast<const T*>(dout);
    const int qblk = attn_blocks(p.Nq), kblk = attn_blocks(p.Nk);
    [[maybe_unused]] float *part_q = nullptr, *part_k = nullptr;    // NORM: the two passes' partials, q blocks first
    if constexpr (NORM) {
        part_q = e->partials;
        part_k = e->partials + (int64_t)p.B * p.H * qblk * 2 * kAttnD;
    }
    hipError_t err = launch_attn_delta(p.dtype, out, dout, gr.delta, p.B, p.H, p.Nq, stream);
    if (err != hipSuccess) return err;
    if constexpr (NORM) a.x.part = part_q;
    spf_attn_dq_kernel<T, MASK, NORM><<<dim3(qblk, p.H, p.B), kBlock, 0, stream>>>(a, g, go, lse, gr.delta);
    err = hipGetLastError();                                        // (dq settles delta: before the dk/dv pass)
    if (err != hipSuccess) return err;
    if constexpr (NORM) a.x.part = part_k;
    spf_attn_dkdv_kernel<T, MASK, NORM><<<dim3(kblk, p.H, p.B), kBlock, 0, stream>>>(a, g, go, lse, gr.delta);
    err = hipGetLastError();
    if constexpr (NORM) {
        if (err != hipSuccess) return err;
        spf_attn_norm_reduce_kernel<<<1, kBlock, 0, stream>>>(part_q, p.B * p.H * qblk, e->dq_weight, e->dq_bias);
        spf_attn_norm_reduce_kernel<<<1, kBlock, 0, stream>>>(part_k, p.B * p.H * kblk, e->dk_weight, e->dk_bias);
        err = hipGetLastError();
    }
    return err;
}

// The instantiation of a call: f(AttnKind<element type, mask present, norm present>()); e null: a plain call.
template <typename T, bool MASK, bool NORM> struct AttnKind {
    typedef T type;
    static constexpr bool mask = MASK, norm = NORM;
};
template <typename F>
hipError_t attn_dispatch(int dtype, const SpfAttnExt* e, F f) {
    const bool mask = e && e->mask, norm = e && e->q_weight;
    auto flags = [&](auto t) {
        typedef decltype(t) T;
        if (mask) return norm ? f(AttnKind<T, true, true>()) : f(AttnKind<T, true, false>());
        return norm ? f(AttnKind<T, false, true>()) : f(AttnKind<T, false, false>());
    };
    switch (dtype) {
        case 0: return flags(float());
        case 1: return flags(__half());
        default: return flags(__hip_bfloat16());
    }
}

// ---- VIEWS: the host part ---------------------------------------------------------------------------------------------
// words: SpfAttnViews.allow itself (forward, dq pass) or its transpose (dk/dv pass)
AttnArgsV make_view_args(const SpfAttn& p, const SpfAttnViews& w, bool transpose) {
    AttnArgsV a;
    static_cast<AttnArgs&>(a) = make_attn_args(p);
    a.w.Vq = w.Vq; a.w.Vk = w.Vk;
    for (int i = 0; i < 32; ++i) a.w.words[i] = 0;
    for (int i = 0; i < w.Vq; ++i)
        for (int s = 0; s < w.Vk; ++s)
            if (w.allow[i] >> s & 1u) {
                if (transpose) a.w.words[s] |= 1u << i;
                else a.w.words[i] |= 1u << s;
            }
    a.w.qv = w.q_view_stride; a.w.kv = w.k_view_stride; a.w.vv = w.v_view_stride;
    a.w.qpb = w.qpos_stride[0]; a.w.qpv = w.qpos_stride[1];
    a.w.kpb = w.kpos_stride[0]; a.w.kpv = w.kpos_stride[1];
    a.w.dqv = w.dq_view_stride; a.w.dkv = w.dk_view_stride; a.w.dvv = w.dv_view_stride;
    return a;
}

template <typename T>
hipError_t attn_views_forward(const SpfAttn& p, const SpfAttnViews& w, void* out, float* lse, hipStream_t stream) {
    spf_attn_fwd_kernel<T, false, false, true><<<dim3(attn_blocks(p.Nq), p.H, p.B * w.Vq), kBlock, 0, stream>>>(
        make_view_args(p, w, false), static_cast<T*>(out), lse);
    return hipGetLastError();
}

template <typename T>
hipError_t attn_views_backward(const SpfAttn& p, const SpfAttnViews& w, const SpfAttnGrads& gr, const void* out,
                               const float* lse, const void* dout, hipStream_t stream) {
    const AttnGradArgs g = make_attn_grad_args(gr);
    const T* go = static_cast<const T*>(dout);
    hipError_t err = launch_attn_delta(p.dtype, out, dout, gr.delta, p.B * w.Vq, p.H, p.Nq, stream);
    if (err != hipSuccess) return err;
    spf_attn_dq_kernel<T, false, false, true><<<dim3(attn_blocks(p.Nq), p.H, p.B * w.Vq), kBlock, 0, stream>>>(
        make_view_args(p, w, false), g, go, lse, gr.delta);
    err = hipGetLastError();                                        // (dq settles delta: before the dk/dv pass)
    if (err != hipSuccess) return err;
    spf_attn_dkdv_kernel<T, false, false, true><<<dim3(attn_blocks(p.Nk), p.H, p.B * w.Vk), kBlock, 0, stream>>>(
        make_view_args(p, w, true), g, go, lse, gr.delta);
    return hipGetLastError();
}

template <typename T>
hipError_t attn_delta(const void* out, const void* dout, float* delta, int B, int H, int Nq, hipStream_t stream) {
    const int64_t rows = (int64_t)B * Nq * H;
    spf_attn_delta_kernel<T><<<(unsigned)((rows + kBlock - 1) / kBlock), kBlock, 0, stream>>>(
        static_cast<const T*>(out), static_cast<const T*>(dout), delta, B, H, Nq);
    return hipGetLastError();
}

}  // namespace

// The row-dot pre-pass of every backward: this file's three and attention16.hip's.
hipError_t launch_attn_delta(int dtype, const void* out, const void* dout, float* delta, int B, int H, int Nq,
                             hipStream_t stream) {
    switch (dtype) {
        case 0: return attn_delta<float>(out, dout, delta, B, H, Nq, stream);
        case 1: return attn_delta<__half>(out, dout, delta, B, H, Nq, stream);
        default: return attn_delta<__hip_bfloat16>(out, dout, delta, B, H, Nq, stream);
    }
}

hipError_t launch_attn_views_forward(const SpfAttn& p, const SpfAttnViews& w, void* out, float* lse, hipStream_t stream) {
    switch (p.dtype) {
        case 0: return attn_views_forward<float>(p, w, out, lse, stream);
        case 1: return attn_views_forward<__half>(p, w, out, lse, stream);
        default: return attn_views_forward<__hip_bfloat16>(p, w, out, lse, stream);
    }
}

hipError_t launch_attn_views_backward(const SpfAttn& p, const SpfAttnViews& w, const SpfAttnGrads& g, const void* out,
                                      const float* lse, const void* dout, hipStream_t stream) {
    switch (p.dtype) {
        case 0: return attn_views_backward<float>(p, w, g, out, lse, dout, stream);
        case 1: return attn_views_backward<__half>(p, w, g, out, lse, dout, stream);
        default: return attn_views_backward<__hip_bfloat16>(p, w, g, out, lse, dout, stream);
    }
}

// e: the extras of the call, or null for a plain one (the caller has checked both).
hipError_t launch_attn_forward(const SpfAttn& p, const SpfAttnExt* e, void* out, float* lse, hipStream_t stream) {
    return attn_dispatch(p.dtype, e, [&](auto k) {
        typedef decltype(k) K;
        return attn_forward<typename K::type, K::mask, K::norm>(p, e, out, lse, stream);
    });
}

hipError_t launch_attn_backward(const SpfAttn& p, const SpfAttnGrads& g, const SpfAttnExt* e, const void* out,
                                const float* lse, const void* dout, hipStream_t stream) {
    return attn_dispatch(p.dtype, e, [&](auto k) {
        typedef decltype(k) K;
        return attn_backward<typename K::type, K::mask, K::norm>(p, g, e, out, lse, dout, stream);
    });
}

int64_t attn_ext_scratch_floats(int B, int H, int Nq, int Nk) {
    return (int64_t)B * H * (attn_blocks(Nq) + attn_blocks(Nk)) * 2 * kAttnD;
}

}  // namespace spf
