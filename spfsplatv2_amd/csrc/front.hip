// The encoder front on gfx950: image -> tokens.  Patch embedding (a stride = kernel convolution) as an implicit GEMM on
// v_mfma_f32_32x32x2_f32 that reads the caller's image and `proj.weight` where they lie, the tokens around the patch rows,
// and the gradients to every parameter.  float32 only.
//
//   spf_front_embed_kernel<P>   out[b, before + n, :] = bias + W . patch(b, n) [+ pos_table[n]]: M = all patches of all
//                               images (128 per block), N = embed channels (128 per block), K = C_in P P in the order of
//                               `proj.weight` [C, C_in, P, P], which is the B operand as [N, K], no packed copy.  A K step
//                               is ONE row of a patch of one channel (P floats, contiguous in the image and in the weight).
//                               The per-channel affine (x - mean) / std is one fma at staging.  Four waves as 2 x 2, four
//                               32 x 32 accumulator tiles each; the next step's loads are in flight under the MFMAs.
//                               One K-long chain per output: an image's rows do not depend on its batch.
//   spf_front_assemble_kernel   the rows of `out` the patch kernel does not own: token tensors [1, k, C] (broadcast over
//                               the images) or [B, k, C] in front of and behind the patch rows, `pos_first` added to row 0;
//                               with a body (assemble_tokens) it copies the body's rows as well: one launch.
//   spf_front_wgrad_kernel<P>   dW[n, k] = sum_m dY[m, n] A[m, k]: A re-read from the image with the same staging, dY read
//                               at its placed rows.  M is cut into chunks (front_chunk_rows); a block owns a 128 x 128 tile
//                               of one chunk and writes it to the workspace.
//   spf_front_reduce_kernel     the chunks' partials summed in chunk order
//   spf_front_rowsum_kernel     out[j, :] = sum_i src[off + j sj + i si, :] in the order of i: d pos_table (over the
//                               images), dbias (over the rows of that)
//   spf_front_tokens_bwd_kernel a broadcast token's gradient: the sum over the images of its rows of dY, in a fixed order
//                               (blocks of 16 images, front_blocked_sum)
// No atomics: two runs agree bitwise.  Every index is bounded by the sizes api.hip has checked.
#include "launchers.h"

namespace spf {

typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f2a __attribute__((ext_vector_type(2)));

constexpr int kFrontTile = 128;            // rows and columns of a block's output tile (both matrix kernels)
constexpr int kFrontLd = kFrontTile + 4;   // LDS row pitch in floats: a multiple of 4, rows 16 bytes aligned
constexpr int kFrontRed = 16;              // reduction step of the weight gradient (rows of M per LDS tile)
constexpr int kFrontChunkRows = 256;       // least chunk height of the weight gradient
constexpr int kFrontMaxChunks = 16;        // 1,024 x 768 floats per chunk at the flagship size: 48 MB of partials at most

int64_t front_chunk_rows(int64_t M) {
    if (M <= (int64_t)kFrontChunkRows * kFrontMaxChunks) return kFrontChunkRows;
    const int64_t h = (M + kFrontMaxChunks - 1) / kFrontMaxChunks;
    return (h + kFrontRed - 1) / kFrontRed * kFrontRed;
}
int64_t front_chunks(int64_t M) {
    const int64_t h = front_chunk_rows(M);
    return M < 1 ? 1 : (M + h - 1) / h;
}
int64_t front_geometry(int what, int64_t M) {
    switch (what) {
        case SPF_FRONT_TILE_ROWS: return kFrontTile;
        case SPF_FRONT_TILE_COLS: return kFrontTile;
        case SPF_FRONT_CHUNK_ROWS: return front_chunk_rows(M);
        case SPF_FRONT_CHUNKS: return front_chunks(M);
    }
    return -1;
}
int64_t front_workspace_floats(const SpfFront& a, bool with_dweight) {
    const int64_t Np = (int64_t)a.gh * a.gw, M = Np * a.B, K = (int64_t)a.C_in * a.P * a.P;
    return (with_dweight ? front_chunks(M) * a.C * K : 0) + Np * a.C;
}

template <int VW> struct FrontVec;
template <> struct FrontVec<4> { typedef f4a type; };
template <> struct FrontVec<2> { typedef f2a type; };

// ---- forward -------------------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kBlock) void spf_front_embed_kernel(SpfFront a, const float* __restrict__ weight,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ pos, float* __restrict__ out) {
    constexpr int VW = P == 16 ? 4 : 2, PR = P / VW;              // floats per load, loads per patch row
    constexpr int NP = (kFrontTile * PR + kBlock - 1) / kBlock;   // loads per lane and operand in a step: 2 (P 16), 4 (P 14)
    typedef typename FrontVec<VW>::type vec;
    __shared__ float s_a[P * kFrontLd];
    __shared__ float s_b[P * kFrontLd];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int Np = a.gh * a.gw;
    const int64_t M = (int64_t)a.B * Np, m0 = (int64_t)blockIdx.x * kFrontTile;
    const int n0 = blockIdx.y * kFrontTile;
    const int64_t K = (int64_t)a.C_in * P * P;
    const float* __restrict__ image = a.image;
    const float* __restrict__ affine = a.affine;

    int row[NP], q[NP];
    int64_t abase[NP], bbase[NP];
    bool aok[NP], bok[NP];
#pragma unroll
    for (int r = 0; r < NP; ++r) {
        const int idx = tid + kBlock * r;
        row[r] = idx / PR;
        q[r] = idx - row[r] * PR;
        const bool valid = idx < kFrontTile * PR;
        const int64_t p = m0 + row[r];
        aok[r] = valid && p < M;
        const int64_t pc = aok[r] ? p : 0;
        const int b = (int)(pc / Np), n = (int)(pc - (int64_t)b * Np);
        const int y0 = n / a.gw, x0 = n - y0 * a.gw;
        abase[r] = (int64_t)b * a.stride_b + (int64_t)y0 * P * a.stride_y + x0 * P + q[r] * VW;
        const int co = n0 + row[r];
        bok[r] = valid && co < a.C;
        bbase[r] = (bok[r] ? (int64_t)co : 0) * K + q[r] * VW;
    }
    const int niter = a.C_in * P;
    vec ra[NP], rb[NP];
    auto load = [&](int it) {
        const int c = it / P, py = it - c * P;
        const float sc = affine ? affine[c] : 1.f, sh = affine ? affine[a.C_in + c] : 0.f;
        const int64_t ao = (int64_t)c * a.stride_c + (int64_t)py * a.stride_y, bo = (int64_t)it * P;
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            vec va = {}, vb = {};
            if (aok[r]) {
                va = *reinterpret_cast<const vec*>(image + abase[r] + ao);
#pragma unroll
                for (int e = 0; e < VW; ++e) va[e] = fmaf(va[e], sc, sh);
            }
            if (bok[r]) vb = *reinterpret_cast<const vec*>(weight + bbase[r] + bo);
            ra[r] = va;
            rb[r] = vb;
        }
    };
    f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    load(0);
    const int kl = lane >> 5, il = lane & 31;
    for (int it = 0; it < niter; ++it) {
        __syncthreads();                                   // the previous step's readers are done
#pragma unroll
        for (int r = 0; r < NP; ++r)
            if (tid + kBlock * r < kFrontTile * PR) {
#pragma unroll
                for (int e = 0; e < VW; ++e) {
                    s_a[(q[r] * VW + e) * kFrontLd + row[r]] = ra[r][e];
                    s_b[(q[r] * VW + e) * kFrontLd + row[r]] = rb[r][e];
                }
            }
        __syncthreads();
        if (it + 1 < niter) load(it + 1);                  // in flight under the MFMAs below
#pragma unroll
        for (int kk = 0; kk < P; kk += 2) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = s_a[(kk + kl) * kFrontLd + wm * 64 + i * 32 + il];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = s_b[(kk + kl) * kFrontLd + wn * 64 + j * 32 + il];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    // C/D map of the 32 x 32 tile: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int T = a.before + Np + a.after;
    float bcol[2];
    int co[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        co[j] = n0 + wn * 64 + j * 32 + il;
        bcol[j] = bias && co[j] < a.C ? bias[co[j]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t p = m0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kl;
            if (p >= M) continue;
            const int b = (int)(p / Np), n = (int)(p - (int64_t)b * Np);
            float* __restrict__ o = out + ((int64_t)b * T + a.before + n) * a.C;
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (co[j] < a.C) {
                    float v = acc[i][j][e] + bcol[j];
                    if (pos) v += pos[(int64_t)n * a.C + co[j]];
                    o[co[j]] = v;
                }
        }
}

// sum_{i < cnt} f(i) in a fixed order: blocks of 16 consecutive terms, the block sums added in order.  The rounding error
// of a sum over a thousand images grows with the square root of the number of blocks, not of the terms.
template <typename F>
__device__ __forceinline__ f4a front_blocked_sum(int cnt, F&& f) {
    f4a tot = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = 0; i0 < cnt; i0 += 16) {
        const int end = i0 + 16 < cnt ? i0 + 16 : cnt;
        f4a s = f(i0);
        for (int i = i0 + 1; i < end; ++i) s += f(i);
        tot += s;
    }
    return tot;
}

// ---- the rows around the patches -----------------------------------------------------------------------------------
// A block takes kFrontRowsPerBlock consecutive (sequence, row) pairs -- with a body every row of out[s], without one only
// the extra rows -- and has all of their loads in flight before the first store; the addresses are block-uniform.
constexpr int kFrontRowsPerBlock = 8;
__global__ __launch_bounds__(kBlock) void spf_front_assemble_kernel(SpfFrontTokens t, const float* __restrict__ body,
                                                                    int64_t inner, int64_t stride, int64_t outer_stride,
                                                                    int64_t total, int N, int C, float* __restrict__ out) {
    const int extra = t.before + t.after, per = body ? extra + N : extra;
    const int T = extra + N, C4 = C >> 2;
    const f4a* src[kFrontRowsPerBlock];
    const f4a* add[kFrontRowsPerBlock];
    f4a* dst[kFrontRowsPerBlock];
#pragma unroll
    for (int j = 0; j < kFrontRowsPerBlock; ++j) {
        const int64_t item = (int64_t)blockIdx.x * kFrontRowsPerBlock + j;
        src[j] = nullptr;
        add[j] = nullptr;
        dst[j] = nullptr;
        if (item >= total) continue;
        const int64_t s = item / per;
        int r = (int)(item - s * per);                          // row of out[s] ...
        if (!body && r >= t.before) r += N;                     // ... skipping the patch rows, which have their owner
        dst[j] = reinterpret_cast<f4a*>(out + (s * T + r) * C);
        if (r >= t.before && r < t.before + N) {
            const int64_t i = s * N + (r - t.before);
            src[j] = reinterpret_cast<const f4a*>(body + (i / inner) * outer_stride + (i % inner) * stride);
        } else {
            int e = r < t.before ? r : r - N, g = 0;            // index among the extra rows -> its tensor
            while (g < t.n_before + t.n_after - 1 && e >= t.rows[g]) e -= t.rows[g++];
            src[j] = reinterpret_cast<const f4a*>(t.tok[g] + ((t.per_image[g] ? s : 0) * t.rows[g] + e) * C);
            if (r == 0) add[j] = reinterpret_cast<const f4a*>(t.pos_first);
        }
    }
    for (int c = threadIdx.x; c < C4; c += kBlock) {
        f4a v[kFrontRowsPerBlock];
#pragma unroll
        for (int j = 0; j < kFrontRowsPerBlock; ++j)
            if (src[j]) {
                v[j] = src[j][c];
                if (add[j]) v[j] += add[j][c];
            }
#pragma unroll
        for (int j = 0; j < kFrontRowsPerBlock; ++j)
            if (dst[j]) dst[j][c] = v[j];
    }
}

// d tok[g][j, :] = sum over the sequences of dY[s, row, :], for the broadcast tensors with a destination; row 0 also
// feeds d pos_first.  One block per extra row.
__global__ __launch_bounds__(kBlock) void spf_front_tokens_bwd_kernel(SpfFrontTokens t, const float* __restrict__ dy,
                                                                      int64_t dy_ss, int64_t dy_sr, int S, int N, int C,
                                                                      float* __restrict__ d_pos_first) {
    int e = blockIdx.x, g = 0;
    const int r = e < t.before ? e : e + N;
    while (g < t.n_before + t.n_after - 1 && e >= t.rows[g]) e -= t.rows[g++];
    float* dst = t.n_before + t.n_after > 0 && !t.per_image[g] && t.tok[g] ? const_cast<float*>(t.tok[g]) + (int64_t)e * C
                                                                          : nullptr;
    float* dst2 = r == 0 ? d_pos_first : nullptr;
    if (!dst && !dst2) return;
    const float* __restrict__ p = dy + (int64_t)r * dy_sr;
    for (int c = threadIdx.x; c < (C >> 2); c += kBlock) {
        const f4a sum = front_blocked_sum(S, [&](int s) { return reinterpret_cast<const f4a*>(p + (int64_t)s * dy_ss)[c]; });
        if (dst) reinterpret_cast<f4a*>(dst)[c] = sum;
        if (dst2) reinterpret_cast<f4a*>(dst2)[c] = sum;
    }
}

// ---- weight gradient -----------------------------------------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(kBlock) void spf_front_wgrad_kernel(SpfFront a, const float* __restrict__ dy, int64_t dy_sb,
                                                                 int64_t dy_sr, int64_t chunk_rows,
                                                                 float* __restrict__ partial) {
    constexpr int VW = P == 16 ? 4 : 2, PCS = kFrontTile / VW;    // floats per load of A, loads per row of the K tile
    constexpr int NB = kFrontRed * PCS / kBlock;                  // loads of A per lane in a step: 2 (P 16), 4 (P 14)
    constexpr int NA = kFrontRed * (kFrontTile / 4) / kBlock;     // float4 loads of dY per lane in a step: 2
    constexpr int MB = kBlock / PCS;                              // rows of M between two loads of a lane
    typedef typename FrontVec<VW>::type vec;
    __shared__ float s_a[kFrontRed * kFrontLd];                   // dY^T: [m][n]
    __shared__ float s_b[kFrontRed * kFrontLd];                   // A:    [m][k]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave & 1, wn = wave >> 1;
    const int Np = a.gh * a.gw;
    const int64_t M = (int64_t)a.B * Np, K = (int64_t)a.C_in * P * P;
    const int64_t k0 = (int64_t)blockIdx.x * kFrontTile;
    const int n0 = blockIdx.y * kFrontTile;
    const int64_t mbeg = (int64_t)blockIdx.z * chunk_rows, mend = mbeg + chunk_rows < M ? mbeg + chunk_rows : M;
    const float* __restrict__ image = a.image;

    // this lane's column of dY and its piece of a patch row: fixed over the steps
    const int n4 = tid & 31, ma = tid >> 5;
    const bool nok = n0 + 4 * n4 < a.C;
    const int kp = tid % PCS, mb = tid / PCS;
    const int64_t k = k0 + kp * VW;
    const bool kok = k < K;
    int64_t koff = 0;
    float sc = 1.f, sh = 0.f;
    if (kok) {
        const int c = (int)(k / (P * P)), rem = (int)(k - (int64_t)c * (P * P)), py = rem / P, px = rem - py * P;
        koff = (int64_t)c * a.stride_c + (int64_t)py * a.stride_y + px;
        if (a.affine) {
            sc = a.affine[c];
            sh = a.affine[a.C_in + c];
        }
    }
    f4a ra[NA];
    vec rb[NB];
    auto load = [&](int64_t ms) {
#pragma unroll
        for (int r = 0; r < NA; ++r) {
            const int64_t m = ms + ma + 8 * r;
            f4a v = {0.f, 0.f, 0.f, 0.f};
            if (nok && m < mend) {
                const int b = (int)(m / Np), n = (int)(m - (int64_t)b * Np);
                v = *reinterpret_cast<const f4a*>(dy + (int64_t)b * dy_sb + (int64_t)(a.before + n) * dy_sr + n0 + 4 * n4);
            }
            ra[r] = v;
        }
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const int64_t m = ms + mb + MB * r;
            vec v = {};
            if (kok && m < mend) {
                const int b = (int)(m / Np), n = (int)(m - (int64_t)b * Np);
                const int y0 = n / a.gw, x0 = n - y0 * a.gw;
                v = *reinterpret_cast<const vec*>(image + (int64_t)b * a.stride_b + (int64_t)y0 * P * a.stride_y + x0 * P + koff);
#pragma unroll
                for (int e = 0; e < VW; ++e) v[e] = fmaf(v[e], sc, sh);
            }
            rb[r] = v;
        }
    };
    f16v acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int kl = lane >> 5, il = lane & 31;
    if (mbeg < mend) load(mbeg);
    for (int64_t ms = mbeg; ms < mend; ms += kFrontRed) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NA; ++r) *reinterpret_cast<f4a*>(s_a + (ma + 8 * r) * kFrontLd + 4 * n4) = ra[r];
#pragma unroll
        for (int r = 0; r < NB; ++r) *reinterpret_cast<vec*>(s_b + (mb + MB * r) * kFrontLd + kp * VW) = rb[r];
        __syncthreads();
        if (ms + kFrontRed < mend) load(ms + kFrontRed);
#pragma unroll
        for (int kk = 0; kk < kFrontRed; kk += 2) {
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = s_a[(kk + kl) * kFrontLd + wm * 64 + i * 32 + il];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = s_b[(kk + kl) * kFrontLd + wn * 64 + j * 32 + il];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }
    float* __restrict__ o = partial + (int64_t)blockIdx.z * a.C * K;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int n = n0 + wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * kl;
            if (n >= a.C) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t kc = k0 + wn * 64 + j * 32 + il;
                if (kc < K) o[(int64_t)n * K + kc] = acc[i][j][e];
            }
        }
}

// out[i] = sum_c partial[c n + i], c ascending; n a multiple of 4
__global__ __launch_bounds__(kBlock) void spf_front_reduce_kernel(const float* __restrict__ partial, int nchunk, int64_t n4,
                                                                  float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) {
        f4a s = reinterpret_cast<const f4a*>(partial)[i];
        for (int c = 1; c < nchunk; ++c) s += reinterpret_cast<const f4a*>(partial)[(int64_t)c * n4 + i];
        reinterpret_cast<f4a*>(out)[i] = s;
    }
}

// out[j, :] = sum_{i < cnt} src[off + j sj + i si + :], in the order of front_blocked_sum
__global__ __launch_bounds__(kBlock) void spf_front_rowsum_kernel(const float* __restrict__ src, int64_t off, int64_t sj,
                                                                  int64_t si, int cnt, int64_t J, int C,
                                                                  float* __restrict__ out) {
    const int C4 = C >> 2;
    const int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (idx >= J * C4) return;
    const int64_t j = idx / C4;
    const int c4 = (int)(idx - j * C4);
    const float* __restrict__ p = src + off + j * sj + 4 * c4;
    *reinterpret_cast<f4a*>(out + j * C + 4 * c4) =
        front_blocked_sum(cnt, [&](int i) { return *reinterpret_cast<const f4a*>(p + (int64_t)i * si); });
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_front_embed_fwd(const SpfFront& a, const float* weight, const float* bias, const float* pos, float* out,
                                  hipStream_t st) {
    const int64_t M = (int64_t)a.B * a.gh * a.gw;
    const dim3 grid((unsigned)((M + kFrontTile - 1) / kFrontTile), (unsigned)((a.C + kFrontTile - 1) / kFrontTile));
    if (a.P == 16)
        spf_front_embed_kernel<16><<<grid, kBlock, 0, st>>>(a, weight, bias, pos, out);
    else
        spf_front_embed_kernel<14><<<grid, kBlock, 0, st>>>(a, weight, bias, pos, out);
    return hipGetLastError();
}

hipError_t launch_front_assemble(const SpfFrontTokens& t, const float* body, int64_t inner, int64_t stride,
                                 int64_t outer_stride, int64_t S, int N, int C, float* out, hipStream_t st) {
    const int64_t total = S * (t.before + t.after + (body ? N : 0));
    if (total == 0) return hipSuccess;
    spf_front_assemble_kernel<<<(unsigned)((total + kFrontRowsPerBlock - 1) / kFrontRowsPerBlock), kBlock, 0, st>>>(
        t, body, inner, stride, outer_stride, total, N, C, out);
    return hipGetLastError();
}

hipError_t launch_front_tokens_bwd(const SpfFrontTokens& t, const float* dy, int64_t dy_ss, int64_t dy_sr, int64_t S, int N,
                                   int C, float* d_pos_first, hipStream_t st) {
    if (t.before + t.after == 0) return hipSuccess;
    spf_front_tokens_bwd_kernel<<<(unsigned)(t.before + t.after), kBlock, 0, st>>>(t, dy, dy_ss, dy_sr, (int)S, N, C,
                                                                                  d_pos_first);
    return hipGetLastError();
}

hipError_t launch_front_embed_bwd(const SpfFront& a, const float* dy, int64_t dy_sb, int64_t dy_sr, float* ws, float* dweight,
                                  float* dbias, float* dpos, hipStream_t st) {
    const int64_t Np = (int64_t)a.gh * a.gw, M = Np * a.B, K = (int64_t)a.C_in * a.P * a.P;
    if (dweight) {
        const int64_t rows = front_chunk_rows(M), chunks = front_chunks(M);
        const dim3 grid((unsigned)((K + kFrontTile - 1) / kFrontTile), (unsigned)((a.C + kFrontTile - 1) / kFrontTile),
                        (unsigned)chunks);
        if (a.P == 16)
            spf_front_wgrad_kernel<16><<<grid, kBlock, 0, st>>>(a, dy, dy_sb, dy_sr, rows, ws);
        else
            spf_front_wgrad_kernel<14><<<grid, kBlock, 0, st>>>(a, dy, dy_sb, dy_sr, rows, ws);
        if (const hipError_t e = hipGetLastError()) return e;
        const int64_t n4 = a.C * K / 4;
        const int64_t nb = (n4 + kBlock - 1) / kBlock;
        spf_front_reduce_kernel<<<(unsigned)(nb < 4096 ? nb : 4096), kBlock, 0, st>>>(ws, (int)chunks, n4, dweight);
        if (const hipError_t e = hipGetLastError()) return e;
    }
    if (dpos || dbias) {
        // the sum over the images per patch row (d pos_table itself, or the workspace's tail), then dbias over its rows
        float* per_row = dpos ? dpos : ws + front_workspace_floats(a, dweight != nullptr) - Np * a.C;
        const int64_t n = Np * (a.C / 4);
        spf_front_rowsum_kernel<<<(unsigned)((n + kBlock - 1) / kBlock), kBlock, 0, st>>>(
            dy, (int64_t)a.before * dy_sr, dy_sr, dy_sb, a.B, Np, a.C, per_row);
        if (const hipError_t e = hipGetLastError()) return e;
        if (dbias) {
            spf_front_rowsum_kernel<<<(unsigned)((a.C / 4 + kBlock - 1) / kBlock), kBlock, 0, st>>>(per_row, 0, 0, a.C,
                                                                                                    (int)Np, 1, a.C, dbias);
            if (const hipError_t e = hipGetLastError()) return e;
        }
    }
    return hipSuccess;
}

}  // namespace spf
