// The guarded AdamW step over a whole parameter set, for gfx950: NaN / large-gradient guard, global-norm clip and the
// AdamW update in three launches, none of which the host waits for.
//
// Replaces ModelWrapper.optimizer_step (/root/reference/src/model/model_wrapper.py:1113-1151): per parameter tensor
// `isnan(grad).any()`, `grad.abs().max().item()` and `grad.abs().max() > max_grad_norm` (three host syncs each), then
// `clip_grad_norm_(parameters, 0.5)` and `torch.optim.AdamW.step()` (configure_optimizers, :1067-1111).
//
// The set is T float32 tensors of any sizes, described by a static device table (SpfOptimTensor) and an array of T
// gradient addresses that the caller refreshes every step (0 = no gradient).  Every tensor is cut into chunks of
// kOptimChunk = 4 slots of point_slots.h; chunk c of the set belongs to the tensor t with
// chunk_start[t] <= c < chunk_start[t + 1], found by a wave-uniform binary search (scalar loads).  Blocks take chunks
// grid-stride.
//
//   A  spf_optim_stats_kernel    reads every present gradient once; per chunk {max |g| without NaN, sum g^2, NaN count}
//   B  spf_optim_verdict_kernel  one block: chunk records -> tensor records (sum g^2 in float64, chunk order), the
//                                reference's walk in guard order, the report, and per tensor the step counter and the
//                                two bias-correction factors (float64)
//   C  spf_optim_apply_kernel    reads the report; skipped: every block leaves after that read.  Otherwise clip, decay,
//                                moments, update, in float32; the gradient is not written back
//
// No float atomic anywhere: every sum has a fixed order (lane -> wave -> block -> chunk -> tensor -> set), so two runs
// from the same inputs agree bitwise and nothing depends on the grid.
#include <math.h>

#include "point_slots.h"
#include "launchers.h"

namespace spf {

constexpr int kOptimSlots = 4;                            // slots per chunk: four 16-byte loads per lane and array
constexpr int kOptimChunk = kOptimSlots * kSlotPoints;    // 4096 floats
constexpr int kVerdictThreads = 1024;
static_assert(kOptimChunk == SPF_OPTIM_CHUNK, "the header's chunk size is the kernels'");
static_assert(kOptimChunk % kSlotPoints == 0, "a chunk is whole slots");

struct ChunkRecord {      // 16 bytes, written by pass A for every chunk of a tensor with a gradient
    float max_abs;        // over the chunk's elements that are not NaN (+-inf counts)
    float sum_sq;
    uint32_t nan_count;
    uint32_t pad;
};
struct TensorRecord {     // 16 bytes, written by pass B
    double sum_sq;
    float max_abs;
    uint32_t has_nan;
};
struct StepState {        // 8 bytes per tensor, written by pass B for pass C
    float step_size;      // lr / (1 - beta1^step)
    float bc2_sqrt;       // sqrt(1 - beta2^step)
};

// the tensor that owns chunk c (uniform over the block: scalar loads)
__device__ __forceinline__ int chunk_tensor(const int64_t* __restrict__ chunk_start, int T, int64_t c) {
    int lo = 0, hi = T;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (chunk_start[mid] <= c) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- pass A ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void spf_optim_stats_kernel(const SpfOptimTensor* __restrict__ table,
                                                                 const int64_t* __restrict__ chunk_start,
                                                                 const uint64_t* __restrict__ grads, int T,
                                                                 int64_t chunks, ChunkRecord* __restrict__ rec) {
    __shared__ SumRow<3> s_row;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int t = chunk_tensor(chunk_start, T, c);
        const float* __restrict__ g = reinterpret_cast<const float*>(grads[t]);
        if (!g) continue;                                            // (uniform: the whole block passes over it)
        const int64_t off = (c - chunk_start[t]) * kOptimChunk;
        const int64_t left = table[t].numel - off;
        const int n = (int)(left < kOptimChunk ? left : kOptimChunk);
        const bool al = aligned16(g);
        g += off;
        float v[kOptimSlots][4];
#pragma unroll
        for (int k = 0; k < kOptimSlots; ++k) load4(g, al, k * kSlotPoints + 4 * (int)threadIdx.x, n, v[k]);
        float ss = 0.f;
        uint32_t mx = 0, nn = 0;
#pragma unroll
        for (int k = 0; k < kOptimSlots; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = v[k][j];
                const bool isnan_ = x != x;
                const uint32_t a = __float_as_uint(x) & 0x7fffffffu;     // |x|: non-negative floats order as integers
                nn += isnan_ ? 1u : 0u;
                mx = isnan_ ? mx : (a > mx ? a : mx);
                ss += x * x;
            }
        }
        ss = wave_sum(ss);
        nn = wave_sum_u32(nn);
        mx = wave_max_u32(mx);
        __syncthreads();                                             // the previous chunk's readers of the row are done
        if (lane == 0) {
            s_row.w[wave][0] = __float_as_uint(ss);
            s_row.w[wave][1] = nn;
            s_row.w[wave][2] = mx;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t m01 = s_row.w[0][2] > s_row.w[1][2] ? s_row.w[0][2] : s_row.w[1][2];
            const uint32_t m23 = s_row.w[2][2] > s_row.w[3][2] ? s_row.w[2][2] : s_row.w[3][2];
            ChunkRecord r;
            r.max_abs = __uint_as_float(m01 > m23 ? m01 : m23);
            r.sum_sq = sum_row_f32(s_row, 0);
            r.nan_count = sum_row_u32(s_row, 1);
            r.pad = 0;
            rec[c] = r;
        }
    }
}

// ---- pass B ------------------------------------------------------------------------------------------------------------
// One block.  (1) a thread per tensor folds the tensor's chunk records in chunk order; (2) the walk: the offender is the
// first position of the guard order whose tensor has a NaN or a maximum above the threshold -- a minimum over positions
// --, max_gradient the maximum over the positions before it, and over the offender itself when it is a large one;
// (3) the total norm, a float64 tree over the tensors; (4) the report and every present tensor's step state.
__global__ __launch_bounds__(kVerdictThreads) void spf_optim_verdict_kernel(
    const SpfOptimTensor* __restrict__ table, const int64_t* __restrict__ chunk_start,
    const uint64_t* __restrict__ grads, const int32_t* __restrict__ guard_order, int T, const ChunkRecord* __restrict__ rec,
    TensorRecord* __restrict__ trec, StepState* __restrict__ sstate, int32_t* __restrict__ step, SpfOptimHyper hp,
    int have_stats, SpfOptimReport* __restrict__ report) {
    __shared__ double s_tree[kVerdictThreads];
    __shared__ int s_offender;
    __shared__ uint32_t s_max;
    const int tid = threadIdx.x;
    if (tid == 0) {
        s_offender = T;
        s_max = 0;
    }
    double norm_sq = 0.0;
    if (have_stats) {
        for (int t = tid; t < T; t += kVerdictThreads) {
            TensorRecord r;
            r.sum_sq = 0.0;
            r.max_abs = 0.f;
            r.has_nan = 0;
            if (grads[t]) {
                for (int64_t c = chunk_start[t]; c < chunk_start[t + 1]; ++c) {
                    const ChunkRecord k = rec[c];
                    r.sum_sq += (double)k.sum_sq;
                    r.max_abs = k.max_abs > r.max_abs ? k.max_abs : r.max_abs;
                    r.has_nan |= k.nan_count != 0;
                }
            }
            trec[t] = r;
            norm_sq += r.sum_sq;                                     // (this thread's tensors in index order)
        }
    }
    __threadfence_block();
    __syncthreads();
    const float threshold = (float)hp.max_grad_value;
    if (have_stats && hp.guard) {
        int first = T;
        for (int i = tid; i < T; i += kVerdictThreads) {
            const int t = guard_order[i];
            if (!grads[t]) continue;
            const TensorRecord r = trec[t];
            if ((r.has_nan || r.max_abs > threshold) && i < first) first = i;
        }
        if (first < T) atomicMin(&s_offender, first);
    }
    __syncthreads();
    const int offender = s_offender;
    int off_nan = 0;
    if (have_stats) {
        if (offender < T) off_nan = (int)trec[guard_order[offender]].has_nan;
        uint32_t mx = 0;
        const int end = offender < T ? offender + (off_nan ? 0 : 1) : T;     // NaN is tested before the maximum
        for (int i = tid; i < end; i += kVerdictThreads) {
            const int t = guard_order[i];
            if (!grads[t]) continue;
            const uint32_t a = __float_as_uint(trec[t].max_abs);
            mx = a > mx ? a : mx;
        }
        if (mx) atomicMax(&s_max, mx);
    }
    s_tree[tid] = norm_sq;
    __syncthreads();
    for (int half = kVerdictThreads / 2; half > 0; half >>= 1) {
        if (tid < half) s_tree[tid] += s_tree[tid + half];
        __syncthreads();
    }
    const double total_norm = sqrt(s_tree[0]);
    const bool skipped = offender < T;
    if (tid == 0) {
        SpfOptimReport r;
        r.skipped = skipped;
        r.nan_detected = skipped && off_nan;
        r.large_detected = skipped && !off_nan;
        r.offender = skipped ? offender : -1;
        r.max_gradient = __uint_as_float(s_max);
        r.total_norm = (float)total_norm;
        double coef = 1.0;
        if (hp.clip) {
            coef = hp.max_norm / (total_norm + 1e-6);
            coef = coef > 1.0 ? 1.0 : coef;                          // (NaN stays NaN, as torch.clamp leaves it)
        }
        r.clip_coef = (float)coef;
        r.clip_coef_lo = (float)(coef - (double)r.clip_coef);        // (NaN or 0 where the coefficient is not finite or exact)
        *report = r;
    }
    if (skipped) return;
    for (int t = tid; t < T; t += kVerdictThreads) {
        if (!grads[t]) continue;
        const int32_t n = step[t] + 1;
        step[t] = n;
        const SpfOptimGroup g = hp.group[table[t].group];
        StepState s;
        s.step_size = (float)(g.lr / (1.0 - pow(g.beta1, (double)n)));
        s.bc2_sqrt = (float)sqrt(1.0 - pow(g.beta2, (double)n));
        sstate[t] = s;
    }
}

// ---- pass C ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void spf_optim_apply_kernel(const SpfOptimTensor* __restrict__ table,
                                                                 const int64_t* __restrict__ chunk_start,
                                                                 const uint64_t* __restrict__ grads, int T,
                                                                 int64_t chunks, const StepState* __restrict__ sstate,
                                                                 SpfOptimHyper hp,
                                                                 const SpfOptimReport* __restrict__ report) {
    // The operations of torch's single-tensor AdamW in its order (mul_, lerp_, mul_ + addcmul_, sqrt / div / add_,
    // addcdiv_), each rounded where torch rounds it: no contraction into fused multiply-adds beyond the two written out
    // below, so that the result differs from torch's by as little as the formula allows.  The pass is bound by memory,
    // not by these few instructions.
#pragma clang fp contract(off)
    if (report->skipped) return;
    // the coefficient as float32 + what float32 dropped of it: g' = g coef is then rounded once, not twice
    const float coef = report->clip_coef, coef_lo = report->clip_coef_lo;
    const bool two_part = coef_lo != 0.f && coef_lo == coef_lo;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int t = chunk_tensor(chunk_start, T, c);
        const float* __restrict__ g = reinterpret_cast<const float*>(grads[t]);
        if (!g) continue;
        const SpfOptimTensor e = table[t];
        const int64_t off = (c - chunk_start[t]) * kOptimChunk;
        const int64_t left = e.numel - off;
        const int n = (int)(left < kOptimChunk ? left : kOptimChunk);
        const SpfOptimGroup grp = hp.group[e.group];
        const float decay = (float)(1.0 - grp.lr * grp.weight_decay);
        const float w1 = (float)(1.0 - grp.beta1), b2 = (float)grp.beta2, w2 = (float)(1.0 - grp.beta2);
        const float eps = (float)grp.eps;
        const StepState s = sstate[t];
        const bool ag = aligned16(g), ap = aligned16(e.param), am = aligned16(e.exp_avg), av = aligned16(e.exp_avg_sq);
        g += off;
        float* __restrict__ p = e.param + off;
        float* __restrict__ m = e.exp_avg + off;
        float* __restrict__ v = e.exp_avg_sq + off;
        float gv[kOptimSlots][4], pv[kOptimSlots][4], mv[kOptimSlots][4], vv[kOptimSlots][4];
#pragma unroll
        for (int k = 0; k < kOptimSlots; ++k) {
            const int p0 = k * kSlotPoints + 4 * (int)threadIdx.x;
            load4(g, ag, p0, n, gv[k]);
            load4(p, ap, p0, n, pv[k]);
            load4(m, am, p0, n, mv[k]);
            load4(v, av, p0, n, vv[k]);
        }
#pragma unroll
        for (int k = 0; k < kOptimSlots; ++k) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float gc = two_part ? fmaf(gv[k][j], coef, gv[k][j] * coef_lo) : gv[k][j] * coef;
                const float pd = pv[k][j] * decay;
                const float mn = fmaf(w1, gc - mv[k][j], mv[k][j]);          // lerp_, fused as torch's kernels have it
                const float vn = vv[k][j] * b2 + (w2 * gc) * gc;
                const float denom = sqrtf(vn) / s.bc2_sqrt + eps;
                pv[k][j] = pd + (-s.step_size * mn) / denom;
                mv[k][j] = mn;
                vv[k][j] = vn;
            }
            const int p0 = k * kSlotPoints + 4 * (int)threadIdx.x;
            store4(p, ap, p0, n, pv[k]);
            store4(m, am, p0, n, mv[k]);
            store4(v, av, p0, n, vv[k]);
        }
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------
int64_t optim_chunks_of(int64_t numel) { return (numel + kOptimChunk - 1) / kOptimChunk; }

// scratch: chunk records | tensor records | step states (each 16-byte aligned: 16 c, 16 T, 8 T bytes)
int64_t optim_scratch_bytes(int T, int64_t chunks) { return 16 * chunks + 16 * (int64_t)T + 8 * (int64_t)T; }

hipError_t launch_optim_step(const SpfOptim& o, const SpfOptimHyper& hp, hipStream_t stream) {
    ChunkRecord* rec = static_cast<ChunkRecord*>(o.scratch);
    TensorRecord* trec = reinterpret_cast<TensorRecord*>(rec + o.chunks);
    StepState* sstate = reinterpret_cast<StepState*>(trec + o.T);
    const int grid = slot_grid(o.chunks);
    const int have_stats = hp.guard || hp.clip;      // neither: pass A is not needed, the report says "not skipped"
    if (have_stats)
        spf_optim_stats_kernel<<<grid, kBlock, 0, stream>>>(o.table, o.chunk_start, o.grads, o.T, o.chunks, rec);
    spf_optim_verdict_kernel<<<1, kVerdictThreads, 0, stream>>>(o.table, o.chunk_start, o.grads, o.guard_order, o.T, rec,
                                                                trec, sstate, o.step, hp, have_stats,
                                                                static_cast<SpfOptimReport*>(o.report));
    spf_optim_apply_kernel<<<grid, kBlock, 0, stream>>>(o.table, o.chunk_start, o.grads, o.T, o.chunks, sstate, hp,
                                                        static_cast<const SpfOptimReport*>(o.report));
    return hipGetLastError();
}

}  // namespace spf
