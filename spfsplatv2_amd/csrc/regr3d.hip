// Distillation point loss (Regr3D.forward, src/loss/loss_point.py:188-254, with normalize_pointcloud 'avg_dis',
// src/geometry/ptc_geometry.py:270-328) for two views of B point maps, forward and backward, without a host sync.
//
// The reference, per call: torch.quantile twice (a full sort of every row of H W norms), four boolean index-puts and two
// boolean gathers (a host sync each) and ~40 eager kernels.  Here, with row (v, b) = view v of batch item b, n = H W
// points per row and slots of 1024 points (four per lane, three 16-byte loads per tensor):
//   spf_regr3d_zero_kernel    clears the select histograms (quantile mode only, as the next six launches)
//   spf_regr3d_hist_kernel    x3: radix select over the float32 bit patterns of dis = |gt| (non-negative, so the pattern
//                             orders like the value): digits of 11, 11 and 9 bits from the top.  A block counts a segment
//                             of up to 8 slots of one row in LDS -- one histogram per DISTINCT prefix of the four wanted
//                             ranks -- and adds its non-empty bins to the row's global histogram (integer atomics)
//   spf_regr3d_pick_kernel    x3: one block per row, one wave per rank: scan the bins, fix the digit, keep the rank
//                             inside it, clear the histogram for the next pass; the last one writes q_lo, q_hi (torch's
//                             lerp of the two order statistics either side of float32(q) * (n - 1))
//   spf_regr3d_mask_kernel    per slot: the valid count and the sums of |pr| and |gt| over the valid points
//   spf_regr3d_norm_kernel    one block per b, fixed order: n_valid[2][b], nf_pr[b], nf_gt[b]
//   spf_regr3d_loss_kernel    per slot: sum of |pr / nf_pr - gt / nf_gt| and of u . pr (u its direction) over the valid
//                             points -- the second is what the gradient through nf_pr needs
//   spf_regr3d_final_kernel   blocks 0 .. B-1: T[v][b] = the row's sum of u . pr; block B: the loss, and scale[v] =
//                             w_v / N_v (0 for a view without a valid point or switched off) for the backward
//   spf_regr3d_bwd_kernel     one launch, every point recomputed from the inputs:
//                             dL/dpr_i = g (scale_v u_i / nf - S_b / (nf^2 n_b) pr_i / |pr_i|), S_b = sum_v scale_v T[v][b]
// dis is recomputed from gt in every pass by the same inlined expression (explicit fmaf chain: the same bits each time),
// so nothing per point is kept anywhere.  No float atomics; every float sum is lane -> wave -> block -> slot -> row in a
// fixed order, and a slot's content depends on (row, chunk) only: results are run-to-run identical and do not depend
// on the batch strides.
#include "point_slots.h"
#include "launchers.h"

namespace spf {

constexpr int kRegrSeg = 8;               // slots per block of a histogram pass (8,192 points share one LDS flush)
constexpr int kRegrBins = 2048;           // bins of the widest digit (11 bits)
constexpr int kRegrRanks = 4;             // floor / ceil of the two quantile ranks
constexpr int kRegrSel = 2 * kRegrRanks;  // select state per row: prefix[4], rank inside the prefix[4]
constexpr float kRegrQLo = 0.002f, kRegrQHi = 0.998f;   // loss_point.py:228-229
constexpr float kRegrConfMin = 3.f;                     // loss_point.py:236-237
constexpr float kRegrNfMin = 1e-8f;                     // ptc_geometry.py:302,321

// Layout of the caller's scratch, in 32-bit words, for R = 2 B rows of nchunk slots each
struct RegrScratch {
    int64_t hist, sel, pcnt, ppr, pgt, ploss, pdot, T, scale, words;
};
__host__ __device__ inline RegrScratch regr_scratch(int B, int nchunk) {
    const int64_t R = 2 * (int64_t)B, S = R * nchunk;
    RegrScratch s;
    s.hist = 0;
    s.sel = s.hist + R * kRegrRanks * kRegrBins;
    s.pcnt = s.sel + R * kRegrSel;
    s.ppr = s.pcnt + S;
    s.pgt = s.ppr + S;
    s.ploss = s.pgt + S;
    s.pdot = s.ploss + S;
    s.T = s.pdot + S;
    s.scale = s.T + R;
    s.words = (s.scale + 2 + 3) & ~(int64_t)3;
    return s;
}

int regr3d_chunks(int H, int W) { return (int)slot_chunks((int64_t)H * W); }
int64_t regr3d_scratch_words(int B, int H, int W) { return regr_scratch(B, regr3d_chunks(H, W)).words; }

// |p| by one explicit chain, so that every pass forms the same bits
__device__ __forceinline__ float regr_norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }

__device__ __forceinline__ const float* regr_gt(const SpfRegr3d& a, int v, int b) {
    return v == 0 ? a.gt_pts1 + (int64_t)b * a.stride_gt1 : a.gt_pts2 + (int64_t)b * a.stride_gt2;
}
__device__ __forceinline__ const float* regr_pr(const SpfRegr3d& a, int v, int b) {
    return v == 0 ? a.pr_pts1 + (int64_t)b * a.stride_pr1 : a.pr_pts2 + (int64_t)b * a.stride_pr2;
}

// The four confidences of a lane's points (one 16-byte load), or +inf when the mask does not read them (dist_clip)
__device__ __forceinline__ void regr_conf4(const SpfRegr3d& a, int v, int b, int p0, int n, float (&c)[4]) {
    if (a.has_dist_clip) {
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = __builtin_inff();
        return;
    }
    const float* row = (v == 0 ? a.conf1 : a.conf2) + (int64_t)b * n;
    load4(row, aligned16(row), p0, n, c);
}
// valid (loss_point.py:214-215, 232-237): NaN compares false everywhere, as in torch
__device__ __forceinline__ bool regr_valid(float dis, float conf, float qlo, float qhi) {
    return dis >= qlo && dis <= qhi && conf >= kRegrConfMin;
}

// ---- selection -----------------------------------------------------------------------------------------------------
// Pass p looks at the digit below a prefix of PrefixBits(p) bits: (shift of the prefix, shift of the digit, bins)
template <int PASS> struct RegrDigit;
template <> struct RegrDigit<0> { static constexpr int pshift = 31, dshift = 20, bins = 2048; };
template <> struct RegrDigit<1> { static constexpr int pshift = 20, dshift = 9, bins = 2048; };
template <> struct RegrDigit<2> { static constexpr int pshift = 9, dshift = 0, bins = 512; };

__global__ __launch_bounds__(kBlock) void spf_regr3d_zero_kernel(uint32_t* __restrict__ p, int64_t words) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < words; i += (int64_t)gridDim.x * kBlock) p[i] = 0u;
}

template <int PASS>
__global__ __launch_bounds__(kBlock) void spf_regr3d_hist_kernel(SpfRegr3d a, int nchunk, int nseg, int64_t nslots,
                                                                 const uint32_t* __restrict__ sel,
                                                                 uint32_t* __restrict__ ghist) {
    using D = RegrDigit<PASS>;
    __shared__ uint32_t s_hist[kRegrRanks * kRegrBins];
    const int n = a.H * a.W;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int row = (int)(slot / nseg), seg = (int)(slot - (int64_t)row * nseg);
        const int v = row / a.B, b = row - v * a.B;
        // the prefixes of the four ranks; a rank whose prefix an earlier rank has counts nothing (the pick reads the
        // earlier rank's histogram)
        uint32_t prefix[kRegrRanks];
        bool own[kRegrRanks];
#pragma unroll
        for (int t = 0; t < kRegrRanks; ++t) {
            prefix[t] = PASS == 0 ? 0u : sel[(int64_t)row * kRegrSel + t];
            own[t] = true;
#pragma unroll
            for (int s = 0; s < t; ++s) own[t] = own[t] && prefix[s] != prefix[t];
        }
        __syncthreads();                                  // the previous slot's flush has read s_hist
        for (int i = threadIdx.x; i < kRegrRanks * kRegrBins; i += kBlock) s_hist[i] = 0u;
        __syncthreads();
        const float* base = regr_gt(a, v, b);
        const bool al = aligned16(base);
        const int c_end = min(nchunk, (seg + 1) * kRegrSeg);
        for (int chunk = seg * kRegrSeg; chunk < c_end; ++chunk) {
            const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
            float x[12];
            load4_xyz(base, al, p0, n, x);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (p0 + k >= n) continue;
                // (sign bit dropped: a NaN norm orders above +inf whatever its sign; digits stay inside the bins)
                const uint32_t key = __float_as_uint(regr_norm3(x[3 * k], x[3 * k + 1], x[3 * k + 2])) & 0x7fffffffu;
                const uint32_t digit = (key >> D::dshift) & (uint32_t)(D::bins - 1);
                const uint32_t pre = PASS == 0 ? 0u : key >> D::pshift;
#pragma unroll
                for (int t = 0; t < kRegrRanks; ++t)
                    if (own[t] && pre == prefix[t]) atomicAdd(&s_hist[t * kRegrBins + digit], 1u);
            }
        }
        __syncthreads();
        uint32_t* g = ghist + (int64_t)row * kRegrRanks * kRegrBins;
        for (int i = threadIdx.x; i < kRegrRanks * kRegrBins; i += kBlock) {
            const uint32_t c = s_hist[i];
            if (c) atomicAdd(&g[i], c);
        }
    }
}

// torch's lerp (aten/src/ATen/native/Lerp.h) in float32: the difference and 1 - w are rounded, the multiply-add is ONE
// fused operation, as torch's kernels form it (torch.quantile on the CPU gives these bits; tests/test_regr3d_exact.py)
__device__ __forceinline__ float regr_lerp(float lo, float hi, float w) {
    const float d = __fsub_rn(hi, lo);
    return w < 0.5f ? __fmaf_rn(w, d, lo) : __fmaf_rn(-d, __fsub_rn(1.f, w), hi);
}

// One block per row, wave t = rank t.
template <int PASS>
__global__ __launch_bounds__(kBlock) void spf_regr3d_pick_kernel(int n, uint32_t* __restrict__ sel,
                                                                 uint32_t* __restrict__ ghist, float* __restrict__ q) {
    using D = RegrDigit<PASS>;
    __shared__ uint32_t s_digit[kRegrRanks], s_rank[kRegrRanks];
    const int row = blockIdx.x, lane = threadIdx.x & (kWave - 1), t = threadIdx.x >> 6;
    // torch.quantile: rank = float32(q) * (n - 1) in float32; the order statistics at its floor and its ceiling
    const float r_lo = __fmul_rn(kRegrQLo, (float)(n - 1)), r_hi = __fmul_rn(kRegrQHi, (float)(n - 1));
    // this wave's rank and prefix, and the first rank with the same prefix: it holds the counts
    uint32_t my_prefix = 0u, want;
    int alias = t;
    if (PASS == 0) {
        const float r = t < 2 ? r_lo : r_hi;
        want = (uint32_t)((t & 1) ? ceilf(r) : floorf(r));
        alias = 0;
    } else {
        my_prefix = sel[(int64_t)row * kRegrSel + t];
        want = sel[(int64_t)row * kRegrSel + kRegrRanks + t];
#pragma unroll
        for (int s = kRegrRanks - 2; s >= 0; --s)
            if (s < t && sel[(int64_t)row * kRegrSel + s] == my_prefix) alias = s;
    }
    if (threadIdx.x < kRegrRanks) {
        s_digit[threadIdx.x] = (uint32_t)(D::bins - 1);   // (never kept: the row's counts add up to more than the rank)
        s_rank[threadIdx.x] = 0u;
    }
    __syncthreads();
    uint32_t* g = ghist + (int64_t)row * kRegrRanks * kRegrBins;
    constexpr int kPer = D::bins / kWave;                // consecutive bins per lane
    uint32_t c[kPer], sum = 0u;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        c[j] = g[alias * kRegrBins + lane * kPer + j];
        sum += c[j];
    }
    const uint32_t incl = wave_iscan_u32(sum);
    uint32_t cum = incl - sum;
    if (want >= cum && want < incl) {
        int digit = lane * kPer;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (want >= cum + c[j]) {
                cum += c[j];
                digit = lane * kPer + j + 1;
            } else {
                break;
            }
        }
        s_digit[t] = (uint32_t)digit;
        s_rank[t] = want - cum;
    }
    __syncthreads();                                     // every wave has read the histograms
    for (int i = threadIdx.x; i < kRegrRanks * kRegrBins; i += kBlock) g[i] = 0u;
    if (PASS < 2) {
        if (lane == 0) {                                 // (this wave's own two words: nobody else reads them any more)
            sel[(int64_t)row * kRegrSel + t] = (my_prefix << (D::pshift - D::dshift)) | s_digit[t];
            sel[(int64_t)row * kRegrSel + kRegrRanks + t] = s_rank[t];
        }
    } else if (threadIdx.x == 0) {
        float val[kRegrRanks];
#pragma unroll
        for (int s = 0; s < kRegrRanks; ++s)
            val[s] = __uint_as_float((sel[(int64_t)row * kRegrSel + s] << 9) | s_digit[s]);
        q[2 * (int64_t)row] = regr_lerp(val[0], val[1], __fsub_rn(r_lo, floorf(r_lo)));
        q[2 * (int64_t)row + 1] = regr_lerp(val[2], val[3], __fsub_rn(r_hi, floorf(r_hi)));
    }
}

// dist_clip: the thresholds are (0, dist_clip) for every row
__global__ __launch_bounds__(kBlock) void spf_regr3d_clip_kernel(int rows, float clip, float* __restrict__ q) {
    const int row = blockIdx.x * kBlock + threadIdx.x;
    if (row < rows) {
        q[2 * row] = 0.f;
        q[2 * row + 1] = clip;
    }
}

// ---- mask, counts, norm sums ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void spf_regr3d_mask_kernel(SpfRegr3d a, int nchunk, int64_t nslots,
                                                                 const float* __restrict__ q, uint32_t* __restrict__ pcnt,
                                                                 float* __restrict__ ppr, float* __restrict__ pgt) {
    __shared__ SumRow<3> s_sum;
    const int n = a.H * a.W;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int row = (int)(slot / nchunk), chunk = (int)(slot - (int64_t)row * nchunk);
        const int v = row / a.B, b = row - v * a.B;
        const float qlo = q[2 * row], qhi = q[2 * row + 1];
        const float* gt = regr_gt(a, v, b);
        const float* pr = regr_pr(a, v, b);
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float x[12], y[12], cf[4];
        load4_xyz(gt, aligned16(gt), p0, n, x);
        load4_xyz(pr, aligned16(pr), p0, n, y);
        regr_conf4(a, v, b, p0, n, cf);
        uint32_t cnt[1] = {0u};
        float s[2] = {0.f, 0.f};                          // sums of |pr| and of |gt|
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dis = regr_norm3(x[3 * k], x[3 * k + 1], x[3 * k + 2]);
            const bool valid = p0 + k < n && regr_valid(dis, cf[k], qlo, qhi);
            cnt[0] += valid ? 1u : 0u;
            s[1] += valid ? dis : 0.f;
            s[0] += valid ? regr_norm3(y[3 * k], y[3 * k + 1], y[3 * k + 2]) : 0.f;
        }
        block_sum(s, cnt, s_sum);
        if (threadIdx.x == 0) {
            pcnt[slot] = cnt[0];
            ppr[slot] = s[0];
            pgt[slot] = s[1];
        }
    }
}

// One block per batch item b: its two rows' slots in a fixed order (view 0's chunks, then view 1's).
// stats: n_valid[2][B] (int32), q[2][B][2], nf_pr[B], nf_gt[B]
__global__ __launch_bounds__(kBlock) void spf_regr3d_norm_kernel(int B, int nchunk, int normalize, int gt_scale,
                                                                 const uint32_t* __restrict__ pcnt,
                                                                 const float* __restrict__ ppr,
                                                                 const float* __restrict__ pgt, float* __restrict__ stats) {
    __shared__ SumRow<4> s_sum;
    const int b = blockIdx.x;
    uint32_t cnt[2] = {0u, 0u};                           // valid points of view 0, of view 1
    float s[2] = {0.f, 0.f};                              // sums of |pr| and of |gt|
    for (int k = threadIdx.x; k < 2 * nchunk; k += kBlock) {
        const int v = k / nchunk, c = k - v * nchunk;
        const int64_t slot = ((int64_t)v * B + b) * nchunk + c;
        const uint32_t cc = pcnt[slot];
        cnt[0] += v == 0 ? cc : 0u;
        cnt[1] += v == 0 ? 0u : cc;
        s[0] += ppr[slot];
        s[1] += pgt[slot];
    }
    block_sum(s, cnt, s_sum);
    const uint32_t n0 = cnt[0], n1 = cnt[1];
    const float tpr = s[0], tgt = s[1];
    if (threadIdx.x == 0) {
        int32_t* nv = reinterpret_cast<int32_t*>(stats);
        nv[b] = (int32_t)n0;
        nv[B + b] = (int32_t)n1;
        // norm_factor = sum / (nnz1 + nnz2 + 1e-8), clipped from below (float32: the 1e-8 only shows when the count is 0)
        const float den = (float)(n0 + n1) + kRegrNfMin;
        stats[6 * (int64_t)B + b] = normalize ? fmaxf(tpr / den, kRegrNfMin) : 1.f;
        stats[7 * (int64_t)B + b] = (normalize && !gt_scale) ? fmaxf(tgt / den, kRegrNfMin) : 1.f;
    }
}

// ---- loss ----------------------------------------------------------------------------------------------------------
// One valid point: d = pr / nf_pr - gt / nf_gt, e = |d|, u = d / e (0 where e = 0, as torch.norm's backward)
struct RegrPt {
    float ux, uy, uz, e;
};
__device__ __forceinline__ RegrPt regr_point(const float* __restrict__ pr, const float* __restrict__ gt, float nf_pr,
                                             float nf_gt) {
    const float dx = pr[0] / nf_pr - gt[0] / nf_gt, dy = pr[1] / nf_pr - gt[1] / nf_gt, dz = pr[2] / nf_pr - gt[2] / nf_gt;
    RegrPt r;
    r.e = regr_norm3(dx, dy, dz);
    const bool nz = r.e != 0.f;
    r.ux = nz ? dx / r.e : 0.f;
    r.uy = nz ? dy / r.e : 0.f;
    r.uz = nz ? dz / r.e : 0.f;
    return r;
}

__global__ __launch_bounds__(kBlock) void spf_regr3d_loss_kernel(SpfRegr3d a, int nchunk, int64_t nslots,
                                                                 const float* __restrict__ stats,
                                                                 float* __restrict__ ploss, float* __restrict__ pdot) {
    __shared__ SumRow<2> s_sum;
    const int n = a.H * a.W;
    const float* q = stats + 2 * (int64_t)a.B;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int row = (int)(slot / nchunk), chunk = (int)(slot - (int64_t)row * nchunk);
        const int v = row / a.B, b = row - v * a.B;
        const float qlo = q[2 * row], qhi = q[2 * row + 1];
        const float nf_pr = stats[6 * (int64_t)a.B + b], nf_gt = stats[7 * (int64_t)a.B + b];
        const float* gt = regr_gt(a, v, b);
        const float* pr = regr_pr(a, v, b);
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float x[12], y[12], cf[4];
        load4_xyz(gt, aligned16(gt), p0, n, x);
        load4_xyz(pr, aligned16(pr), p0, n, y);
        regr_conf4(a, v, b, p0, n, cf);
        float s[2] = {0.f, 0.f};                          // sums of e and of u . pr
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dis = regr_norm3(x[3 * k], x[3 * k + 1], x[3 * k + 2]);
            const bool valid = p0 + k < n && regr_valid(dis, cf[k], qlo, qhi);
            const RegrPt r = regr_point(y + 3 * k, x + 3 * k, nf_pr, nf_gt);
            s[0] += valid ? r.e : 0.f;
            s[1] += valid ? fmaf(r.uz, y[3 * k + 2], fmaf(r.uy, y[3 * k + 1], r.ux * y[3 * k])) : 0.f;
        }
        block_sum(s, s_sum);
        if (threadIdx.x == 0) {
            ploss[slot] = s[0];
            pdot[slot] = s[1];
        }
    }
}

// Blocks 0 .. B-1: T[v][b], the row sums of u . pr.  Block B: N_v = sum_b n_valid[v][b], loss_v = sum / N_v (NaN for a
// view without a valid point: the mean of nothing), loss = loss_1 + loss_2 or loss_2, and scale[v] = w_v / N_v or 0.
__global__ __launch_bounds__(kBlock) void spf_regr3d_final_kernel(int B, int nchunk, int disable_view1,
                                                                  const float* __restrict__ stats,
                                                                  const float* __restrict__ ploss,
                                                                  const float* __restrict__ pdot, float* __restrict__ T,
                                                                  float* __restrict__ scale, float* __restrict__ loss) {
    __shared__ SumRow<2> s_t;
    __shared__ SumRow<4> s_sum;
    if ((int)blockIdx.x < B) {
        const int b = blockIdx.x;
        float acc[2] = {0.f, 0.f};
#pragma unroll
        for (int v = 0; v < 2; ++v)
            for (int c = threadIdx.x; c < nchunk; c += kBlock) acc[v] += pdot[((int64_t)v * B + b) * nchunk + c];
        block_sum(acc, s_t);
        if (threadIdx.x == 0) {
            T[b] = acc[0];
            T[(int64_t)B + b] = acc[1];
        }
        return;
    }
    const int32_t* nv = reinterpret_cast<const int32_t*>(stats);
    float lv[2] = {0.f, 0.f};
    uint32_t Nv[2] = {0u, 0u};
    const int64_t m = (int64_t)B * nchunk;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        for (int b = threadIdx.x; b < B; b += kBlock) Nv[v] += (uint32_t)nv[(int64_t)v * B + b];
        for (int64_t k = threadIdx.x; k < m; k += kBlock) lv[v] += ploss[(int64_t)v * m + k];
    }
    block_sum(lv, Nv, s_sum);
#pragma unroll
    for (int v = 0; v < 2; ++v) lv[v] = lv[v] / (float)Nv[v];
    if (threadIdx.x == 0) {
        loss[0] = disable_view1 ? lv[1] : lv[0] + lv[1];
        scale[0] = (Nv[0] && !disable_view1) ? 1.f / (float)Nv[0] : 0.f;
        scale[1] = Nv[1] ? 1.f / (float)Nv[1] : 0.f;
    }
}

// ---- backward ------------------------------------------------------------------------------------------------------
// Rows v_first .. v_first + n_views - 1 (the views whose gradient is wanted); d_pr1 / d_pr2 [B,H,W,3] contiguous.
__global__ __launch_bounds__(kBlock) void spf_regr3d_bwd_kernel(SpfRegr3d a, int nchunk, int64_t nslots, int v_first,
                                                                const float* __restrict__ stats,
                                                                const float* __restrict__ T,
                                                                const float* __restrict__ scale,
                                                                const float* __restrict__ dL_dloss,
                                                                float* __restrict__ d_pr1, float* __restrict__ d_pr2) {
    const int n = a.H * a.W;
    const int32_t* nv = reinterpret_cast<const int32_t*>(stats);
    const float* q = stats + 2 * (int64_t)a.B;
    const float g = dL_dloss[0];                          // upstream gradient read on the device: no sync
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int row = (int)(slot / nchunk) + v_first * a.B, chunk = (int)(slot % nchunk);
        const int v = row / a.B, b = row - v * a.B;
        const float qlo = q[2 * row], qhi = q[2 * row + 1];
        const float nf_pr = stats[6 * (int64_t)a.B + b], nf_gt = stats[7 * (int64_t)a.B + b];
        const float direct = g * scale[v] / nf_pr;
        // through nf_pr = sum_valid |pr| / n_b (both views' valid points, whichever view the loss counts); nothing
        // where the clip at 1e-8 holds it or there is no normalisation
        const uint32_t nb = (uint32_t)nv[b] + (uint32_t)nv[a.B + b];
        const float S = scale[0] * T[b] + scale[1] * T[a.B + b];
        const float through = (a.normalize && nb && nf_pr > kRegrNfMin) ? g * S / (nf_pr * nf_pr * (float)nb) : 0.f;
        const float* gt = regr_gt(a, v, b);
        const float* pr = regr_pr(a, v, b);
        const int p0 = chunk * kSlotPoints + 4 * threadIdx.x;
        float x[12], y[12], cf[4], o[12];
        load4_xyz(gt, aligned16(gt), p0, n, x);
        load4_xyz(pr, aligned16(pr), p0, n, y);
        regr_conf4(a, v, b, p0, n, cf);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dis = regr_norm3(x[3 * k], x[3 * k + 1], x[3 * k + 2]);
            const bool valid = p0 + k < n && regr_valid(dis, cf[k], qlo, qhi);
            const RegrPt r = regr_point(y + 3 * k, x + 3 * k, nf_pr, nf_gt);
            const float np = regr_norm3(y[3 * k], y[3 * k + 1], y[3 * k + 2]);
            const float w = np != 0.f ? through / np : 0.f;
            o[3 * k] = valid ? direct * r.ux - w * y[3 * k] : 0.f;
            o[3 * k + 1] = valid ? direct * r.uy - w * y[3 * k + 1] : 0.f;
            o[3 * k + 2] = valid ? direct * r.uz - w * y[3 * k + 2] : 0.f;
        }
        float* out = (v == 0 ? d_pr1 : d_pr2) + (int64_t)b * n * 3;
        store4_xyz(out, aligned16(out), p0, n, o);
    }
}

template <int PASS>
static void regr_select_pass(const SpfRegr3d& a, int nchunk, uint32_t* hist, uint32_t* sel, float* q,
                             hipStream_t stream) {
    const int nseg = (nchunk + kRegrSeg - 1) / kRegrSeg;
    const int64_t nslots = 2 * (int64_t)a.B * nseg;
    spf_regr3d_hist_kernel<PASS><<<slot_grid(nslots), kBlock, 0, stream>>>(a, nchunk, nseg, nslots, sel, hist);
    spf_regr3d_pick_kernel<PASS><<<2 * a.B, kBlock, 0, stream>>>(a.H * a.W, sel, hist, q);
}

hipError_t launch_regr3d_fwd(const SpfRegr3d& a, void* scratch, float* stats, float* loss, hipStream_t stream) {
    const int nchunk = regr3d_chunks(a.H, a.W);
    const RegrScratch s = regr_scratch(a.B, nchunk);
    uint32_t* w = static_cast<uint32_t*>(scratch);
    float* f = static_cast<float*>(scratch);
    float* q = stats + 2 * (int64_t)a.B;
    const int rows = 2 * a.B;
    if (a.has_dist_clip) {
        spf_regr3d_clip_kernel<<<(rows + kBlock - 1) / kBlock, kBlock, 0, stream>>>(rows, a.dist_clip, q);
    } else {
        const int64_t hw = s.sel - s.hist;
        spf_regr3d_zero_kernel<<<slot_grid((hw + kBlock - 1) / kBlock), kBlock, 0, stream>>>(w + s.hist, hw);
        regr_select_pass<0>(a, nchunk, w + s.hist, w + s.sel, q, stream);
        regr_select_pass<1>(a, nchunk, w + s.hist, w + s.sel, q, stream);
        regr_select_pass<2>(a, nchunk, w + s.hist, w + s.sel, q, stream);
    }
    const int64_t nslots = (int64_t)rows * nchunk;
    spf_regr3d_mask_kernel<<<slot_grid(nslots), kBlock, 0, stream>>>(a, nchunk, nslots, q, w + s.pcnt, f + s.ppr,
                                                                     f + s.pgt);
    spf_regr3d_norm_kernel<<<a.B, kBlock, 0, stream>>>(a.B, nchunk, a.normalize, a.gt_scale, w + s.pcnt, f + s.ppr,
                                                       f + s.pgt, stats);
    spf_regr3d_loss_kernel<<<slot_grid(nslots), kBlock, 0, stream>>>(a, nchunk, nslots, stats, f + s.ploss, f + s.pdot);
    spf_regr3d_final_kernel<<<a.B + 1, kBlock, 0, stream>>>(a.B, nchunk, a.disable_view1, stats, f + s.ploss, f + s.pdot,
                                                            f + s.T, f + s.scale, loss);
    return hipGetLastError();
}

hipError_t launch_regr3d_bwd(const SpfRegr3d& a, const void* scratch, const float* stats, const float* dL_dloss,
                             float* d_pr1, float* d_pr2, hipStream_t stream) {
    const int nchunk = regr3d_chunks(a.H, a.W);
    const RegrScratch s = regr_scratch(a.B, nchunk);
    const float* f = static_cast<const float*>(scratch);
    const int v_first = d_pr1 ? 0 : 1, n_views = (d_pr1 ? 1 : 0) + (d_pr2 ? 1 : 0);
    const int64_t nslots = (int64_t)n_views * a.B * nchunk;
    spf_regr3d_bwd_kernel<<<slot_grid(nslots), kBlock, 0, stream>>>(a, nchunk, nslots, v_first, stats, f + s.T,
                                                                    f + s.scale, dL_dloss, d_pr1, d_pr2);
    return hipGetLastError();
}

}  // namespace spf
