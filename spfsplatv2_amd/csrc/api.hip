// extern "C" entry points of libspfsplat_hip.so (see include/spfsplat_hip.h).
// Validation + launch sequencing only; no device allocation, no device synchronisation.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "launchers.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// every pointer is a multiple of N bytes; a null pointer passes (whether it may be null is the caller's own check)
template <unsigned N> bool aligned(std::initializer_list<const void*> ps) {
    uintptr_t x = 0;
    for (const void* p : ps) x |= reinterpret_cast<uintptr_t>(p);
    return (x & (N - 1)) == 0;
}

#define SPF_HIP(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(SPF_E_LAUNCH, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// ---- stage timing --------------------------------------------------------------------------
struct StageLog {
    hipEvent_t ev[SPF_STAGE_LOG][2];
    int created = 0;
    int used = 0;
};
StageLog g_log[SPF_STAGE_COUNT];
uint32_t g_timing = 0;   // bit i: record stage i
int g_sample_every = 1;  // record every n-th launch of an enabled stage (an event pair costs ~11 us of idle GPU)
int g_calls[SPF_STAGE_COUNT] = {};

struct StageScope {
    int stage;
    hipStream_t stream;
    int slot = -1;
    StageScope(int st, hipStream_t s) : stage(st), stream(s) {
        if (!((g_timing >> stage) & 1u)) return;
        // (a stream that is being captured launches nothing now: an event recorded here would become a graph node and
        //  could never be timed -- a caller that captures while stage timing is on simply gets no sample)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone) return;
        if (g_calls[stage]++ % g_sample_every != 0) return;
        StageLog& L = g_log[stage];
        if (L.used >= SPF_STAGE_LOG) return;
        if (L.used >= L.created) {
            if (hipEventCreate(&L.ev[L.created][0]) != hipSuccess) return;
            if (hipEventCreate(&L.ev[L.created][1]) != hipSuccess) return;
            L.created++;
        }
        slot = L.used;
        (void)hipEventRecord(L.ev[slot][0], stream);
    }
    ~StageScope() {
        if (slot < 0) return;
        (void)hipEventRecord(g_log[stage].ev[slot][1], stream);
        g_log[stage].used = slot + 1;
    }
};


// ---- two lanes: one batched call as several chunks of renders on two streams (OFF by default) -----------------
// Renders are independent, so after the joint tile scan the rest of the forward (bin -> sort -> composite) and the whole
// backward (composite backward -> projection backward) can run as C chunks of whole scenes alternating between the
// caller's stream and one auxiliary stream, the second lane one kernel behind the first (fork / join by events,
// capturable in a HIP graph; every buffer is render-major, so a chunk is the same launcher on offset pointers and the
// results are bit-identical to the single chain: tests/test_gpu_configs.py).  The idea: a latency-bound kernel of one
// chunk fills the launch gaps and tails of the other chunk's compositing kernel, as two whole-step micro-batches on two
// streams do (bench.py --streams 2: +13 %).  MEASURED (C2, 8 x 4 renders, HIP-graph replay, same box, ms per step):
// 1 chain 0.442 / 0.443, 2 chunks 0.472 / 0.464, 4 chunks 0.514 / 0.508, 8 chunks 0.578 / 0.568 -- it LOSES.  A call must
// hand complete outputs to the caller's stream, so every forward and every backward ends in a join at which both lanes
// drain, half-size launches have twice the tail, and the cross-queue event edges cost as much as the dependent
// launches they were meant to hide; free-running micro-batches never join.  SPF_CHUNKS=n (n > 1) enables it for
// experiments; the default is the single chain, whose per-kernel timings are exclusive.
constexpr int kMaxChunks = 8;
struct LaneSet {
    hipStream_t s = nullptr;
    hipEvent_t stagger = nullptr, join = nullptr;
};
LaneSet* lane_set() {
    // per (device, calling thread): see render.hip::aux_stream.  One stream and two events per pair, created on first
    // use and kept for the life of the process (SPF_CHUNKS experiments only; nothing is created by default)
    static thread_local LaneSet lanes[32];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return nullptr;
    LaneSet& a = lanes[dev];
    if (!a.s) {
        if (hipStreamCreateWithFlags(&a.s, hipStreamNonBlocking) != hipSuccess) { a.s = nullptr; return nullptr; }
        if (hipEventCreateWithFlags(&a.stagger, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&a.join, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(a.s);
            a.s = nullptr;
            return nullptr;
        }
    }
    return &a;
}
// Chunk boundaries in RENDERS: bounds[0..C].  Whole scenes per chunk when there are several scenes (`by_scene`),
// else groups of views of the one scene.  One chunk unless SPF_CHUNKS asks for more (experiments only: no lower bound
// on a chunk's size is applied -- small chunks are what the bit-identity tests run).
int plan_chunks(int S, int V, int T, int* bounds, bool* by_scene) {
    const char* e = getenv("SPF_CHUNKS");
    int want = e ? atoi(e) : 1;
    if (want > kMaxChunks) want = kMaxChunks;
    const int units = S > 1 ? S : V, per_unit = S > 1 ? V : 1;
    *by_scene = S > 1;
    int C = want < 1 ? 1 : want;
    (void)T;
    if (C > units) C = units;
    for (int c = 0; c <= C; ++c) bounds[c] = (int)(((long)units * c) / C) * per_unit;
    return C;
}
struct Chunk {
    SpfDims d;
    SpfInputs in;
    SpfState st;
    SpfOutputs out;
    SpfGrads g;
};
template <typename P>
P* off(P* p, size_t n) { return p ? p + n : p; }
// renders [r0, r1) of the batch as a call of its own.  `scene0` >= 0: the chunk is scenes [scene0, scene0 + nscene)
// (per-scene inputs and gradients are offset too: the projection backward); < 0: tile-stage kernels only.
Chunk make_chunk(const SpfDims& d, const SpfInputs& in, const SpfState& st, const SpfOutputs* out, const SpfGrads* g,
                 int r0, int r1, int scene0, int nscene) {
    Chunk c;
    const size_t G = (size_t)d.G, P = (size_t)d.H * d.W;
    const size_t T = (size_t)spf_raster_num_tiles(d.H, d.W), nblk = (size_t)spf_raster_view_partial_blocks(d.G);
    const size_t r = (size_t)r0;
    c.d = d;
    if (scene0 >= 0) { c.d.S = nscene; } else { c.d.S = 1; c.d.V = r1 - r0; }
    c.in = in;
    c.in.viewmatrix = off(in.viewmatrix, 16 * r); c.in.projmatrix = off(in.projmatrix, 16 * r);
    c.in.tanfov = off(in.tanfov, 2 * r); c.in.bg = off(in.bg, 3 * r); c.in.view_scale = off(in.view_scale, r);
    c.in.viewmatrix64 = off(in.viewmatrix64, 16 * r);
    if (scene0 >= 0) {
        const size_t sg = (size_t)scene0 * G;
        c.in.means3D = off(in.means3D, 3 * sg); c.in.scales = off(in.scales, 3 * sg);
        c.in.rotations = off(in.rotations, 4 * sg); c.in.opacities = off(in.opacities, sg);
        c.in.shs = off(in.shs, 3 * sg * (size_t)(d.sh_layout == 2 ? 16 : d.K)); c.in.colors = off(in.colors, 3 * sg);
        c.in.shs_high = off(in.shs_high, 3 * sg * 9);
        c.in.raw = off(in.raw, sg * (size_t)d.raw_stride);
    }
    c.st = st;
    c.st.rec = off(st.rec, r * G * spf::kRec); c.st.radii = off(st.radii, r * G); c.st.rect = off(st.rect, r * G);
    c.st.zkey = off(st.zkey, r * G); c.st.tile_count = off(st.tile_count, r * T);
    c.st.tile_start = off(st.tile_start, r * T); c.st.tile_fill = off(st.tile_fill, r * T);
    c.st.tile_flags = off(st.tile_flags, r * T); c.st.pair_off = off(st.pair_off, 2 * r * G);
    c.st.blk_total = off(st.blk_total, r * nblk); c.st.blk_base = off(st.blk_base, r * nblk);
    c.st.final_T = off(st.final_T, r * P); c.st.n_contrib = off(st.n_contrib, r * P);
    c.st.sh_clamp = off(st.sh_clamp, r * G);
    if (out) {
        c.out.image = off(out->image, 3 * r * P); c.out.depth = off(out->depth, r * P);
        c.out.alpha = off(out->alpha, r * P);
    } else {
        c.out = SpfOutputs{nullptr, nullptr, nullptr};
    }
    if (g) {
        c.g = *g;
        c.g.dL_dimage = off(g->dL_dimage, 3 * r * P); c.g.dL_ddepth = off(g->dL_ddepth, r * P);
        c.g.dL_dalpha = off(g->dL_dalpha, r * P);
        c.g.vpartial = off(g->vpartial, r * nblk * 12); c.g.dL_dviewmatrix = off(g->dL_dviewmatrix, 16 * r);
        c.g.dL_dmeans2D = off(g->dL_dmeans2D, 3 * r * G);
        if (scene0 >= 0) {
            const size_t sg = (size_t)scene0 * G;
            c.g.dL_dmeans3D = off(g->dL_dmeans3D, 3 * sg); c.g.dL_dscales = off(g->dL_dscales, 3 * sg);
            c.g.dL_drotations = off(g->dL_drotations, 4 * sg); c.g.dL_dopacities = off(g->dL_dopacities, sg);
            c.g.dL_dshs = off(g->dL_dshs, 3 * sg * (size_t)(d.sh_layout == 2 ? 16 : d.K)); c.g.dL_dcolors = off(g->dL_dcolors, 3 * sg);
            c.g.dL_dshs_high = off(g->dL_dshs_high, 3 * sg * 9);
            c.g.dL_draw = off(g->dL_draw, sg * (size_t)(7 + 3 * d.K));
        }
    } else {
        memset(&c.g, 0, sizeof c.g);
    }
    return c;
}
const char* kStageKernel[SPF_STAGE_COUNT] = {
    "spf_project_fwd_kernel", "spf_tile_scan_kernel",  "spf_bin_pairs_kernel",   "spf_sort_tiles_wave_kernel",
    "spf_render_fwd_lists_kernel", "spf_render_bwd_lists_kernel", "spf_project_bwd_kernel", "spf_rope2d_vec_kernel"};

int check_dims(const SpfDims* d) {
    if (!d) return fail(SPF_E_INVALID, "dims is null");
    if (d->S <= 0 || d->V <= 0 || d->G <= 0 || d->H <= 0 || d->W <= 0)
        return fail(SPF_E_INVALID, "S, V, G, H, W must be positive (got %d %d %d %d %d)", d->S, d->V, d->G, d->H, d->W);
    if ((d->W + SPF_TILE - 1) / SPF_TILE > 255 || (d->H + SPF_TILE - 1) / SPF_TILE > 255)
        return fail(SPF_E_INVALID, "image larger than 4080 px per side is not supported");
    if (d->sh_degree < 0 || d->sh_degree > 4) return fail(SPF_E_INVALID, "sh_degree %d outside 0..4", d->sh_degree);
    if (d->K < 0) return fail(SPF_E_INVALID, "K must be >= 0");
    if (d->sh_band4 != 0 && d->sh_band4 != 1) return fail(SPF_E_INVALID, "sh_band4 must be 0 or 1");
    if (d->sh_layout < 0 || d->sh_layout > 3) return fail(SPF_E_INVALID, "sh_layout must be 0 .. 3");
    if (d->sh_layout == 3 && (d->K < 1 || d->raw_stride < 7 + 3 * (int64_t)d->K))
        return fail(SPF_E_INVALID, "sh_layout 3 (raw rows): K >= 1 and raw_stride >= 7 + 3 K (got K = %d, raw_stride = %lld)", d->K, (long long)d->raw_stride);
    if (d->sh_layout == 2 && d->K != 25 && d->K != 0)
        return fail(SPF_E_INVALID, "sh_layout 2 (band split) is the 16 + 9 split of K = 25 coefficients (got K = %d)", d->K);
    if (d->bin_cap < 0) return fail(SPF_E_INVALID, "bin_cap must be >= 0");
    if (d->bin_cap > 0) {
        const int64_t rt = (int64_t)d->S * d->V * spf_raster_num_tiles(d->H, d->W);
        if (rt * d->bin_cap > ((int64_t)1 << 31))
            return fail(SPF_E_INVALID, "direct bins: S*V*tiles*bin_cap = %lld exceeds 2^31", (long long)(rt * d->bin_cap));
        if (spf_raster_num_tiles(d->H, d->W) > spf::max_lds_tiles())
            return fail(SPF_E_INVALID, "direct bins need the per-render tile histogram in LDS (<= %d tiles)", spf::max_lds_tiles());
        if (d->pair_capacity <= 0) return fail(SPF_E_INVALID, "direct bins: pair_capacity must be positive");
    }
    return SPF_OK;
}

// `no_pair`: the scale/rotation pair is not needed -- replaced by precomputed covariances (checked by the *_cov3d entry
// points), or not read at all (spf_raster_forward_render)
int check_inputs(const SpfDims* d, const SpfInputs* in, bool no_pair = false) {
    if (!in) return fail(SPF_E_INVALID, "inputs is null");
    const bool raw = d->sh_layout == 3;
    if (!in->means3D || !in->opacities || !in->viewmatrix || !in->projmatrix || !in->tanfov || !in->bg)
        return fail(SPF_E_INVALID, "a required input pointer is null");
    if (raw) {
        if (!in->raw || !in->sh_mask) return fail(SPF_E_INVALID, "sh_layout 3: raw and sh_mask are required");
        if (in->shs || in->colors) return fail(SPF_E_INVALID, "sh_layout 3: shs / colors must be null (the harmonics are in the raw rows)");
    } else {
        if (!no_pair && (!in->scales || !in->rotations)) return fail(SPF_E_INVALID, "a required input pointer is null");
        if ((in->shs == nullptr) == (in->colors == nullptr))
            return fail(SPF_E_INVALID, "exactly one of shs / colors must be given");
    }
    if (in->shs || raw) {
        const int cap = d->sh_band4 ? 4 : 3;
        const int deg = d->sh_degree > cap ? cap : d->sh_degree;
        if (d->K < (deg + 1) * (deg + 1))
            return fail(SPF_E_INVALID, "K = %d is too small for sh_degree %d", d->K, d->sh_degree);
        if (d->sh_layout == 2 && deg == 4 && !in->shs_high)
            return fail(SPF_E_INVALID, "sh_layout 2 with sh_band4: shs_high (band 4) is null");
    }
    return SPF_OK;
}

}  // namespace

extern "C" {

int spf_abi_version(void) { return SPF_ABI_VERSION; }
const char* spf_last_error(void) { return g_err; }

int spf_raster_num_tiles(int32_t H, int32_t W) {
    return ((W + SPF_TILE - 1) / SPF_TILE) * ((H + SPF_TILE - 1) / SPF_TILE);
}
int spf_raster_view_partial_blocks(int32_t G) { return (G + spf::kBlock - 1) / spf::kBlock; }
// the ONE place that knows where the fields of the three shared state buffers start (header: SpfStateLayout)
static SpfStateLayout state_layout(int64_t RT, int64_t RG, int64_t RB) {
    SpfStateLayout l;
    l.rect_words = 2 * RG + (RG + 3) / 4, l.zkey = RG, l.sh_clamp = 2 * RG;
    l.tiles_words = 4 * RT + 16, l.tile_flags = RT, l.tile_start = 2 * RT, l.tile_fill = 3 * RT + 1, l.counters = 4 * RT + 1, l.pair_cursor = 4 * RT + 5;
    l.pair_idx_words = 2 * RG + 2 * RB, l.blk_total = 2 * RG, l.blk_base = 2 * RG + RB;
    return l;
}
int spf_raster_state_layout(int64_t RT, int64_t RG, int64_t RB, SpfStateLayout* out) {
    if (!out || RT <= 0 || RG <= 0 || RB <= 0) return fail(SPF_E_INVALID, "state_layout: out is null, or RT, RG, RB not all positive (got %lld %lld %lld)", (long long)RT, (long long)RG, (long long)RB);
    *out = state_layout(RT, RG, RB);
    return SPF_OK;
}
int spf_raster_launch_slot_tile(int32_t R, int32_t T, int32_t xcd, int32_t slot) {
    if (R < 1 || T < 1 || (int64_t)R * T > (int64_t)1 << 30 || (((int64_t)R * T) & 7) != 0) return -1;
    const int RT = R * T;
    if (xcd < 0 || xcd > 7 || slot < 0 || slot >= (RT >> 3)) return -1;
    return spf::xcd_tile(spf::xcd_map(RT, T), T, xcd, slot);
}
int spf_raster_pair_shards(int32_t S, int32_t G) {
    if (S < 1 || G < 1) return 1;
    const int64_t nblocks = (int64_t)S * ((G + spf::kBlock - 1) / spf::kBlock);
    return spf::pair_shards(nblocks > 0x7fffffff ? 0x7fffffff : (int)nblocks);
}
int spf_raster_max_lds_tiles(void) { return spf::max_lds_tiles(); }
int spf_raster_chunks(int32_t S, int32_t V, int32_t H, int32_t W, int32_t backward) {
    if (S < 1 || V < 1 || H < 1 || W < 1) return 1;
    int bounds[kMaxChunks + 1];
    bool by_scene = false;
    const int C = plan_chunks(S, V, spf_raster_num_tiles(H, W), bounds, &by_scene);
    return (backward && !by_scene) ? 1 : C;
}
int spf_raster_sort_plan(uint32_t max_tile_hint, int32_t tiles_call, int32_t with_order, int32_t* kernel, uint32_t* lo,
                         uint32_t* hi, int32_t* order) {
    if (tiles_call < 1 || !kernel || !lo || !hi || !order) return -1;
    spf::SortLaunch plan[SPF_SORT_MAX_LAUNCHES];
    const int n = spf::plan_tile_sort(max_tile_hint, tiles_call, with_order != 0, spf::read_sort_switches(), plan);
    for (int i = 0; i < n; ++i) kernel[i] = plan[i].kernel, lo[i] = plan[i].lo, hi[i] = plan[i].hi, order[i] = plan[i].order;
    return n;
}

static int check_camera(const SpfCamera* c, bool fwd) {
    if (!c) return fail(SPF_E_INVALID, "camera is null");
    if (c->R <= 0) return fail(SPF_E_INVALID, "camera R must be positive");
    if (!c->near || !c->viewmatrix) return fail(SPF_E_INVALID, "a camera pointer is null");
    if (fwd && (!c->extrinsics || !c->intrinsics || !c->far || !c->projmatrix || !c->tanfov))
        return fail(SPF_E_INVALID, "a camera pointer is null");
    return SPF_OK;
}

int spf_camera_forward(const SpfCamera* cam, void* stream_) {
    int rc = check_camera(cam, true);
    if (rc) return rc;
    SPF_HIP(spf::launch_camera_fwd(*cam, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_camera_backward(const SpfCamera* cam, const float* dL_dviewmatrix, float* dL_dextrinsics, void* stream_) {
    int rc = check_camera(cam, false);
    if (rc) return rc;
    if (!dL_dviewmatrix || !dL_dextrinsics) return fail(SPF_E_INVALID, "gradient pointer is null");
    SPF_HIP(spf::launch_camera_bwd(*cam, dL_dviewmatrix, dL_dextrinsics, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// tiles_cleared: 0 = nothing (this call clears the counts), 1 = tile_count | tile_flags, 2 = all the tile bookkeeping
static int forward_project(const SpfDims* d, const SpfInputs* in, SpfState* st, int tiles_cleared, void* stream_,
                           uint64_t cleared_words = 0, const float* cov3D = nullptr) {
    int rc = check_dims(d);
    if (rc) return rc;
    rc = check_inputs(d, in, cov3D != nullptr);
    if (rc) return rc;
    if (!st || !st->rec || !st->radii || !st->rect || !st->zkey || !st->tile_count || !st->tile_start ||
        !st->tile_fill || !st->tile_flags || !st->counters || !st->blk_total || !st->blk_base)
        return fail(SPF_E_INVALID, "a state pointer needed by forward_project is null");
    if ((in->shs || in->raw) && !st->sh_clamp) return fail(SPF_E_INVALID, "sh_clamp is needed by forward_project when shs are given");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tiles_x = (d->W + SPF_TILE - 1) / SPF_TILE, tiles_y = (d->H + SPF_TILE - 1) / SPF_TILE;
    const int RT = d->S * d->V * tiles_x * tiles_y;
    const bool direct = d->bin_cap > 0;
    if (direct) {
        if (!st->pairs || !st->pair_cursor || !st->pair_off)
            return fail(SPF_E_INVALID, "direct bins: pairs, pair_cursor and pair_off are needed by forward_project");
        // counters[0..3] and the cursors start at zero: inside what spf_decoder_prepare cleared, or cleared here
        const uint32_t* const end = st->tile_count + cleared_words;
        if (!(tiles_cleared == 2 && st->counters >= st->tile_count && st->counters + 4 <= end))
            SPF_HIP(hipMemsetAsync(st->counters, 0, 4 * sizeof(uint32_t), stream));
        if (!(tiles_cleared == 2 && st->pair_cursor >= st->tile_count && st->pair_cursor + 8 <= end))
            SPF_HIP(hipMemsetAsync(st->pair_cursor, 0, 8 * sizeof(uint32_t), stream));
    }
    if (tiles_cleared) {
        // spf_decoder_prepare cleared tile_count | tile_flags | tile_start | tile_fill | counters with the camera set-up
    } else if (st->tile_flags == st->tile_count + RT) {   // adjacent (the Python binding lays them out so): one fill
        SPF_HIP(hipMemsetAsync(st->tile_count, 0, sizeof(uint32_t) * 2 * (size_t)RT, stream));
    } else {
        SPF_HIP(hipMemsetAsync(st->tile_count, 0, sizeof(uint32_t) * (size_t)RT, stream));
        SPF_HIP(hipMemsetAsync(st->tile_flags, 0, sizeof(uint32_t) * (size_t)RT, stream));
    }
    {
        StageScope t(SPF_STAGE_PROJECT, stream);
        SPF_HIP(spf::launch_project_fwd(*d, *in, *st, tiles_x, tiles_y, stream, cov3D));
    }
    if (direct) return SPF_OK;              // the projection kernel binned; tile_count is the bins' fill: no scan
    {
        StageScope t(SPF_STAGE_SCAN, stream);
        SPF_HIP(spf::launch_tile_scan(*st, d->S * d->V, tiles_x * tiles_y, spf_raster_view_partial_blocks(d->G),
                                      spf::dense_threshold(), tiles_cleared == 2, stream));
    }
    return SPF_OK;
}

int spf_raster_forward_project(const SpfDims* d, const SpfInputs* in, SpfState* st, void* stream_) {
    return forward_project(d, in, st, 0, stream_);
}

static int forward_project_cleared(const SpfDims* d, const SpfInputs* in, SpfState* st, uint64_t cleared_bytes,
                                   void* stream_, const float* cov3D) {
    // `cleared_bytes`: how much of tile_count | tile_flags | tile_start | tile_fill | counters (one buffer, in this order)
    // the caller cleared.  All of it: one-block-per-render scan.  Only the two count arrays (the older contract): the
    // self-initialising single-block scan.  Less than that: this call clears the counts itself.
    if (!d || !st) return fail(SPF_E_INVALID, "dims / state is null");
    const SpfStateLayout l = state_layout((int64_t)d->S * d->V * spf_raster_num_tiles(d->H, d->W), 1, 1);
    const bool laid_out = st->tile_count && st->tile_flags == st->tile_count + l.tile_flags && st->tile_start == st->tile_count + l.tile_start &&
                          st->tile_fill == st->tile_count + l.tile_fill && st->counters == st->tile_count + l.counters;
    if (laid_out && cleared_bytes >= 4 * (uint64_t)(l.counters + 4)) return forward_project(d, in, st, 2, stream_, cleared_bytes / 4, cov3D);
    if (laid_out && cleared_bytes >= 4 * (uint64_t)l.tile_start) return forward_project(d, in, st, 1, stream_, cleared_bytes / 4, cov3D);
    return forward_project(d, in, st, 0, stream_, 0, cov3D);
}

int spf_raster_forward_project_prepared(const SpfDims* d, const SpfInputs* in, SpfState* st, uint64_t cleared_bytes,
                                        void* stream_) {
    return forward_project_cleared(d, in, st, cleared_bytes, stream_, nullptr);
}

// what the covariance entry points reject before anything is launched (the scale/rotation pair, the band-split and
// raw-row layouts, a missing covariance)
static int check_cov3d(const SpfDims* d, const SpfInputs* in, const float* cov3D, const SpfState* st) {
    if (!d || !in || !st) return fail(SPF_E_INVALID, "dims / inputs / state is null");
    if (in->scales || in->rotations)
        return fail(SPF_E_INVALID, "cov3d: scales and rotations must be null (exactly one of a scale/rotation pair or a "
                                   "precomputed 3D covariance)");
    if (d->sh_layout == 2 || d->sh_layout == 3)
        return fail(SPF_E_INVALID, "cov3d: sh_layout %d is not supported with precomputed covariances (0 or 1 only)",
                    d->sh_layout);
    if (!cov3D) return fail(SPF_E_INVALID, "cov3d: cov3D is null");
    return SPF_OK;
}

int spf_raster_forward_project_cov3d(const SpfDims* d, const SpfInputs* in, const float* cov3D, SpfState* st,
                                     uint64_t cleared_bytes, void* stream_) {
    const int rc = check_cov3d(d, in, cov3D, st);
    if (rc) return rc;
    return forward_project_cleared(d, in, st, cleared_bytes, stream_, cov3D);
}

int spf_decoder_prepare(const SpfCamera* cam, void* zero, uint64_t zero_bytes, void* stream_) {
    int rc = check_camera(cam, true);
    if (rc) return rc;
    if (!zero || !aligned<16>({zero}) || (zero_bytes & 15))
        return fail(SPF_E_INVALID, "decoder_prepare: the buffer to clear must be 16-byte aligned and sized");
    SPF_HIP(spf::launch_camera_fwd_zero(*cam, zero, zero_bytes, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_camera_backward_partials(const SpfCamera* cam, const float* vpartial, int32_t nblk, float* dL_dextrinsics,
                                 void* stream_) {
    int rc = check_camera(cam, false);
    if (rc) return rc;
    if (!vpartial || !dL_dextrinsics || nblk < 1) return fail(SPF_E_INVALID, "camera_backward_partials: bad argument");
    if (!aligned<16>({vpartial})) return fail(SPF_E_INVALID, "camera_backward_partials: vpartial must be 16-byte aligned");
    SPF_HIP(spf::launch_camera_bwd_reduce(*cam, vpartial, nblk, dL_dextrinsics, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// SPF_TILE_ORDER=0: the composite lists kernels take their tiles in image order also with direct bins (experiments)
static bool tile_order_enabled() {
    const char* e = getenv("SPF_TILE_ORDER");       // (read per call: the tests flip it; a backward follows its forward's)
    return !(e && e[0] == '0');
}

// SPF_XCD_DEAL=0: every XCD keeps a contiguous range of renders whatever their number (experiments, tests; see
// spf_common.h::xcd_map)
static bool xcd_deal_enabled() {
    const char* e = getenv("SPF_XCD_DEAL");
    return !(e && e[0] == '0');
}

int spf_raster_forward_render(const SpfDims* d, const SpfInputs* in, SpfState* st, SpfOutputs* out, uint64_t capacity,
                              uint32_t max_tile_hint, uint32_t dense_tiles_hint, void* stream_) {
    (void)dense_tiles_hint;       // (ignored: one kernel composites sparse and dense tiles -- see the header)
    int rc = check_dims(d);
    if (rc) return rc;
    rc = check_inputs(d, in, true);          // (the compositing stage never reads the scale/rotation pair)
    if (rc) return rc;
    if (!st || !st->rec || !st->rect || !st->zkey || !st->tile_start || !st->tile_fill || !st->tile_flags ||
        !st->counters || !st->tile_count ||
        !st->final_T || !st->n_contrib || !st->pair_off || !st->blk_base)
        return fail(SPF_E_INVALID, "a state pointer needed by forward_render is null");
    if (capacity > 0 && !st->pairs) return fail(SPF_E_INVALID, "pairs is null but capacity > 0");
    if (!out || !out->image || !out->depth || !out->alpha) return fail(SPF_E_INVALID, "an output pointer is null");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tiles_x = (d->W + SPF_TILE - 1) / SPF_TILE, tiles_y = (d->H + SPF_TILE - 1) / SPF_TILE;
    const int T = tiles_x * tiles_y, RT = d->S * d->V * T;
    if (d->bin_cap > 0) {
        // direct bins: the lists are already in their bins (spf_raster_forward_project*): sort and composite.  `capacity`
        // is the number of gradient records here; the bins are memory-safe by construction.
        if (max_tile_hint != 0u && (uint32_t)d->bin_cap > max_tile_hint) max_tile_hint = (uint32_t)d->bin_cap;
        const spf::TileLists tl = spf::tile_lists(*st, *d);
        const bool ordered = tile_order_enabled();
        {
            StageScope t(SPF_STAGE_SORT, stream);
            // (with `ordered`, eight blocks of the sort's first kernel also write the composite lists kernels' launch order:
            //  long lists first, see tile_order_ptr)
            SPF_HIP(spf::launch_tile_sort(*st, tl, RT, RT, ~0ull, max_tile_hint ? max_tile_hint : (uint32_t)d->bin_cap,
                                          ordered ? spf::tile_order_ptr(*st, *d, RT) : nullptr,
                                          xcd_deal_enabled() ? T : 0, stream));
        }
        {
            StageScope t(SPF_STAGE_RENDER_FWD, stream);
            SPF_HIP(spf::launch_render_fwd(*d, *in, *st, *out, ~0ull, T, tiles_x, ordered, stream));
        }
        return SPF_OK;
    }
    int bounds[kMaxChunks + 1];
    bool by_scene = false;
    int C = plan_chunks(d->S, d->V, T, bounds, &by_scene);
    LaneSet* lanes = C > 1 ? lane_set() : nullptr;
    if (!lanes) { C = 1; bounds[0] = 0; bounds[1] = d->S * d->V; }
    // (a failure inside the loop must not leave the auxiliary lane forked: an un-joined stream invalidates an ongoing
    //  HIP-graph capture -- the chunk body reports, the join below runs either way)
    auto chunk = [&](int c) -> int {
        const hipStream_t cs = (c & 1) ? lanes->s : stream;
        const Chunk ch = make_chunk(*d, *in, *st, out, nullptr, bounds[c], bounds[c + 1], -1, 0);
        const int rt = (bounds[c + 1] - bounds[c]) * T;
        if (c == 1) SPF_HIP(hipStreamWaitEvent(cs, lanes->stagger, 0));     // second lane: one kernel behind the first
        {
            StageScope t(SPF_STAGE_BIN, cs);
            SPF_HIP(spf::launch_bin_pairs(ch.d, ch.st, capacity, T, tiles_x, max_tile_hint, cs));
        }
        if (c == 0 && C > 1) SPF_HIP(hipEventRecord(lanes->stagger, cs));
        {
            StageScope t(SPF_STAGE_SORT, cs);
            SPF_HIP(spf::launch_tile_sort(ch.st, spf::tile_lists(ch.st, ch.d), rt, RT, capacity, max_tile_hint,
                                          /*order*/ nullptr, 0, cs));
        }
        {
            StageScope t(SPF_STAGE_RENDER_FWD, cs);
            SPF_HIP(spf::launch_render_fwd(ch.d, ch.in, ch.st, ch.out, capacity, T, tiles_x, false, cs));
        }
        return SPF_OK;
    };
    for (int c = 0; c < C && rc == SPF_OK; ++c) rc = chunk(c);
    if (C > 1) {
        const hipError_t e1 = hipEventRecord(lanes->join, lanes->s), e2 = hipStreamWaitEvent(stream, lanes->join, 0);
        if (rc == SPF_OK && (e1 != hipSuccess || e2 != hipSuccess))
            return fail(SPF_E_LAUNCH, "joining the auxiliary lane: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    }
    return rc;
}

static int raster_backward(const SpfDims* d, const SpfInputs* in, const SpfState* st, const SpfGrads* g,
                           uint64_t capacity, void* stream_, const float* cov3D, float* dL_dcov3D) {
    int rc = check_dims(d);
    if (rc) return rc;
    rc = check_inputs(d, in, cov3D != nullptr);
    if (rc) return rc;
    if (!st || !st->rec || !st->radii || !st->rect || !st->tile_start || !st->tile_flags || !st->pairs ||
        !st->final_T || !st->n_contrib || !st->pair_off || !st->tile_count)
        return fail(SPF_E_INVALID, "a state pointer needed by backward is null");
    if (!g || !g->gpair || !g->dL_dmeans3D || !g->dL_dopacities)
        return fail(SPF_E_INVALID, "gpair, dL_dmeans3D and dL_dopacities are required");
    if (d->sh_layout == 3 && !g->dL_draw) return fail(SPF_E_INVALID, "sh_layout 3: dL_draw is required");
    if ((in->shs || in->raw) && !st->sh_clamp) return fail(SPF_E_INVALID, "sh_clamp (written by the forward) is needed by backward when shs are given");
    if (g->dL_dviewmatrix && !g->vpartial) return fail(SPF_E_INVALID, "vpartial is required with dL_dviewmatrix");
    if ((g->dL_dscales == nullptr) != (g->dL_drotations == nullptr))
        return fail(SPF_E_INVALID, "dL_dscales and dL_drotations must be given together");
    if (in->shs && d->sh_layout == 2 && d->sh_band4 && d->sh_degree == 4 && g->dL_dshs && !g->dL_dshs_high)
        return fail(SPF_E_INVALID, "sh_layout 2 with sh_band4: dL_dshs_high is needed next to dL_dshs");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int tiles_x = (d->W + SPF_TILE - 1) / SPF_TILE, tiles_y = (d->H + SPF_TILE - 1) / SPF_TILE;
    const int T = tiles_x * tiles_y;
    // (every pair record is written exactly once by its tile: no memset of gpair)
    int bounds[kMaxChunks + 1];
    bool by_scene = false;
    // (covariance calls run as one chain: make_chunk offsets the scale/rotation pair, not a [S,G,6] covariance)
    int C = (d->bin_cap > 0 || cov3D) ? 1 : plan_chunks(d->S, d->V, T, bounds, &by_scene);
    LaneSet* lanes = (C > 1 && by_scene) ? lane_set() : nullptr;     // the projection backward owns whole scenes
    if (!lanes) { C = 1; bounds[0] = 0; bounds[1] = d->S * d->V; }
    auto chunk = [&](int c) -> int {                                        // (see spf_raster_forward_render)
        const hipStream_t cs = (c & 1) ? lanes->s : stream;
        const int s0 = bounds[c] / d->V, ns = (bounds[c + 1] - bounds[c]) / d->V;
        const Chunk ch = C > 1 ? make_chunk(*d, *in, *st, nullptr, g, bounds[c], bounds[c + 1], s0, ns)
                               : Chunk{*d, *in, *st, SpfOutputs{nullptr, nullptr, nullptr}, *g};
        if (c == 1) SPF_HIP(hipStreamWaitEvent(cs, lanes->stagger, 0));     // second lane: one kernel behind the first
        {
            StageScope t(SPF_STAGE_RENDER_BWD, cs);
            SPF_HIP(spf::launch_render_bwd(ch.d, ch.in, ch.st, ch.g, T, tiles_x, capacity,
                                           d->bin_cap > 0 && C == 1 && tile_order_enabled(), cs));
        }
        if (c == 0 && C > 1) SPF_HIP(hipEventRecord(lanes->stagger, cs));
        {
            StageScope t(SPF_STAGE_PROJECT_BWD, cs);
            SPF_HIP(spf::launch_project_bwd(ch.d, ch.in, ch.st, ch.g, spf_raster_view_partial_blocks(d->G), capacity,
                                            cs, cov3D, dL_dcov3D));
        }
        return SPF_OK;
    };
    for (int c = 0; c < C && rc == SPF_OK; ++c) rc = chunk(c);
    if (C > 1) {
        const hipError_t e1 = hipEventRecord(lanes->join, lanes->s), e2 = hipStreamWaitEvent(stream, lanes->join, 0);
        if (rc == SPF_OK && (e1 != hipSuccess || e2 != hipSuccess))
            return fail(SPF_E_LAUNCH, "joining the auxiliary lane: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
    }
    return rc;
}

int spf_raster_backward(const SpfDims* d, const SpfInputs* in, const SpfState* st, const SpfGrads* g,
                        uint64_t capacity, uint32_t dense_tiles_hint, void* stream_) {
    (void)dense_tiles_hint;
    return raster_backward(d, in, st, g, capacity, stream_, nullptr, nullptr);
}

int spf_raster_backward_cov3d(const SpfDims* d, const SpfInputs* in, const float* cov3D, const SpfState* st,
                              const SpfGrads* g, float* dL_dcov3D, uint64_t capacity, uint32_t dense_tiles_hint,
                              void* stream_) {
    (void)dense_tiles_hint;
    int rc = check_cov3d(d, in, cov3D, st);
    if (rc) return rc;
    if (g && (g->dL_dscales || g->dL_drotations))
        return fail(SPF_E_INVALID, "cov3d: dL_dscales and dL_drotations must be null (the covariance gradient goes to "
                                   "dL_dcov3D)");
    return raster_backward(d, in, st, g, capacity, stream_, cov3D, dL_dcov3D);
}

int spf_adapter_forward(const float* raw, int64_t raw_stride, int64_t N, int32_t K, const float* sh_mask, float eps,
                        float* scales, float* rotations, float* harmonics, float* harmonics_high, void* stream_) {
    if (!raw || !sh_mask || !scales || !rotations || !harmonics) return fail(SPF_E_INVALID, "adapter: null pointer");
    if (N < 0 || K < 1 || K > 64) return fail(SPF_E_INVALID, "adapter: N must be >= 0 and K in 1..64");
    if (raw_stride < 7 + 3 * (int64_t)K) return fail(SPF_E_INVALID, "adapter: raw_stride %lld is below the %d channels of a row", (long long)raw_stride, 7 + 3 * K);
    if (harmonics_high && K != 25) return fail(SPF_E_INVALID, "adapter: the band-split layout is the 16 + 9 split of K = 25 (got K = %d)", K);
    if (N == 0) return SPF_OK;
    SPF_HIP(spf::launch_adapter_fwd(raw, raw_stride, N, K, sh_mask, eps, scales, rotations, harmonics, harmonics_high,
                                    static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_adapter_backward(const float* raw, int64_t raw_stride, int64_t N, int32_t K, const float* sh_mask, float eps,
                         const float* dL_dscales, const float* dL_drotations, const float* dL_dharmonics,
                         const float* dL_dharmonics_high, int32_t split, float* dL_draw, void* stream_) {
    if (!raw || !sh_mask || !dL_draw) return fail(SPF_E_INVALID, "adapter: null pointer");
    if (N < 0 || K < 1 || K > 64) return fail(SPF_E_INVALID, "adapter: N must be >= 0 and K in 1..64");
    if (raw_stride < 7 + 3 * (int64_t)K) return fail(SPF_E_INVALID, "adapter: raw_stride %lld is below the %d channels of a row", (long long)raw_stride, 7 + 3 * K);
    if (split && K != 25) return fail(SPF_E_INVALID, "adapter: the band-split layout is the 16 + 9 split of K = 25 (got K = %d)", K);
    if (!split && dL_dharmonics_high) return fail(SPF_E_INVALID, "adapter: dL_dharmonics_high without split");
    if (!aligned<16>({dL_drotations})) return fail(SPF_E_INVALID, "adapter: dL_drotations must be 16-byte aligned");
    if (N == 0) return SPF_OK;
    SPF_HIP(spf::launch_adapter_bwd(raw, raw_stride, N, K, sh_mask, eps, dL_dscales, dL_drotations, dL_dharmonics,
                                    dL_dharmonics_high, split ? 1 : 0, dL_draw, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_mse_partial_blocks(void) { return spf::mse_partial_blocks(); }

int spf_mse_forward(const float* prediction, const float* image, int64_t n, float weight, float* partial,
                    float* loss, void* stream_) {
    if (!prediction || !image || !partial || !loss) return fail(SPF_E_INVALID, "mse: null pointer");
    if (n <= 0) return fail(SPF_E_INVALID, "mse: n must be positive (got %lld)", (long long)n);
    if (!aligned<16>({prediction, image})) return fail(SPF_E_INVALID, "mse: prediction / image must be 16-byte aligned");
    SPF_HIP(spf::launch_mse_fwd(prediction, image, n, weight / (float)n, partial, loss, 0.f, nullptr,
                                static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_mse_forward_grad(const float* prediction, const float* image, int64_t n, float weight, float* partial,
                         float* loss, float* dL_dprediction_unit, void* stream_) {
    if (!prediction || !image || !partial || !loss || !dL_dprediction_unit) return fail(SPF_E_INVALID, "mse: null pointer");
    if (n <= 0) return fail(SPF_E_INVALID, "mse: n must be positive (got %lld)", (long long)n);
    if (!aligned<16>({prediction, image, dL_dprediction_unit})) return fail(SPF_E_INVALID, "mse: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_mse_fwd(prediction, image, n, weight / (float)n, partial, loss, 2.0f * weight / (float)n,
                                dL_dprediction_unit, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_mse_scale_grad(float* dL_dprediction, int64_t n, const float* dL_dloss, void* stream_) {
    if (!dL_dprediction || !dL_dloss) return fail(SPF_E_INVALID, "mse: null pointer");
    if (n <= 0) return fail(SPF_E_INVALID, "mse: n must be positive (got %lld)", (long long)n);
    if (!aligned<16>({dL_dprediction})) return fail(SPF_E_INVALID, "mse: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_mse_scale(dL_dprediction, n, dL_dloss, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_mse_backward(const float* prediction, const float* image, int64_t n, float weight, const float* dL_dloss,
                     float* dL_dprediction, void* stream_) {
    if (!prediction || !image || !dL_dloss || !dL_dprediction) return fail(SPF_E_INVALID, "mse: null pointer");
    if (n <= 0) return fail(SPF_E_INVALID, "mse: n must be positive (got %lld)", (long long)n);
    if (!aligned<16>({prediction, image, dL_dprediction})) return fail(SPF_E_INVALID, "mse: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_mse_bwd(prediction, image, n, 2.0f * weight / (float)n, dL_dloss, dL_dprediction,
                                static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static bool regr3d_sizes_ok(int32_t B, int32_t H, int32_t W) {
    if (B < 1 || H < 1 || W < 1) return false;
    // (a row's 3 H W floats are indexed with 32-bit point numbers; per-view counts and slot numbers are 32-bit)
    if ((int64_t)H * W * 3 >= ((int64_t)1 << 31) || (int64_t)B * H * W >= ((int64_t)1 << 30)) return false;
    return B < (1 << 18);
}

int64_t spf_regr3d_scratch_bytes(int32_t B, int32_t H, int32_t W) {
    if (!regr3d_sizes_ok(B, H, W)) return -1;
    return 4 * spf::regr3d_scratch_words(B, H, W);
}

static int check_regr3d(const SpfRegr3d* a) {
    if (!a) return fail(SPF_E_INVALID, "regr3d: args is null");
    if (!a->gt_pts1 || !a->gt_pts2 || !a->pr_pts1 || !a->pr_pts2) return fail(SPF_E_INVALID, "regr3d: null pointer");
    if (!a->has_dist_clip && (!a->conf1 || !a->conf2))
        return fail(SPF_E_INVALID, "regr3d: null confidences (they are needed unless dist_clip is given)");
    if (a->B < 1 || a->H < 1 || a->W < 1)
        return fail(SPF_E_INVALID, "regr3d: B, H, W must be positive (got %d %d %d)", a->B, a->H, a->W);
    if (!regr3d_sizes_ok(a->B, a->H, a->W))
        return fail(SPF_E_INVALID, "regr3d: %d x %d x %d points is too large", a->B, a->H, a->W);
    if (a->stride_gt1 < 0 || a->stride_gt2 < 0 || a->stride_pr1 < 0 || a->stride_pr2 < 0)
        return fail(SPF_E_INVALID, "regr3d: negative batch strides are not supported");
    if (a->has_dist_clip && a->dist_clip != a->dist_clip) return fail(SPF_E_INVALID, "regr3d: dist_clip is NaN");
    if (!aligned<4>({a->gt_pts1, a->gt_pts2, a->pr_pts1, a->pr_pts2, a->conf1, a->conf2}))
        return fail(SPF_E_INVALID, "regr3d: tensors must be 4-byte aligned");
    return SPF_OK;
}

int spf_regr3d_forward(const SpfRegr3d* args, void* scratch, float* stats, float* loss, void* stream_) {
    if (int rc = check_regr3d(args)) return rc;
    if (!scratch || !stats || !loss) return fail(SPF_E_INVALID, "regr3d: null pointer");
    if (!aligned<16>({scratch})) return fail(SPF_E_INVALID, "regr3d: scratch must be 16-byte aligned");
    if (!aligned<4>({stats, loss})) return fail(SPF_E_INVALID, "regr3d: stats and loss must be 4-byte aligned");
    SPF_HIP(spf::launch_regr3d_fwd(*args, scratch, stats, loss, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_regr3d_backward(const SpfRegr3d* args, const void* scratch, const float* stats, const float* dL_dloss,
                        float* d_pr1, float* d_pr2, void* stream_) {
    if (int rc = check_regr3d(args)) return rc;
    if (!scratch || !stats || !dL_dloss) return fail(SPF_E_INVALID, "regr3d: null pointer");
    if (!d_pr1 && !d_pr2) return fail(SPF_E_INVALID, "regr3d: no gradient requested");
    if (!aligned<16>({scratch})) return fail(SPF_E_INVALID, "regr3d: scratch must be 16-byte aligned");
    if (!aligned<4>({d_pr1, d_pr2, stats, dL_dloss}))
        return fail(SPF_E_INVALID, "regr3d: gradients, stats and dL_dloss must be 4-byte aligned");
    SPF_HIP(spf::launch_regr3d_bwd(*args, scratch, stats, dL_dloss, d_pr1, d_pr2, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int check_pose_compose(const float* enc, int64_t stride_b, int64_t stride_v, int32_t b, int32_t v, int32_t cv,
                              int32_t encoding) {
    if (!enc) return fail(SPF_E_INVALID, "pose_compose: enc is null");
    if (b < 1 || v < 1) return fail(SPF_E_INVALID, "pose_compose: b and v must be positive (got %d %d)", b, v);
    if ((int64_t)b * v >= ((int64_t)1 << 26)) return fail(SPF_E_INVALID, "pose_compose: %d x %d poses is too large", b, v);
    if (cv < 1 || cv > v) return fail(SPF_E_INVALID, "pose_compose: context_views %d is outside 1..%d", cv, v);
    if (encoding != SPF_POSE_ROT6D && encoding != SPF_POSE_QUAT)
        return fail(SPF_E_INVALID, "pose_compose: unknown encoding %d", encoding);
    if (stride_b < 0 || stride_v < 0) return fail(SPF_E_INVALID, "pose_compose: negative strides are not supported");
    return SPF_OK;
}

int spf_pose_compose_forward(const float* enc, int64_t stride_b, int64_t stride_v, int32_t b, int32_t v, int32_t cv,
                             int32_t encoding, int32_t make_baseline_1, int32_t make_relative, float* poses,
                             void* stream_) {
    if (int rc = check_pose_compose(enc, stride_b, stride_v, b, v, cv, encoding)) return rc;
    if (!poses) return fail(SPF_E_INVALID, "pose_compose: poses is null");
    if (!aligned<4>({enc, poses})) return fail(SPF_E_INVALID, "pose_compose: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_pose_compose_fwd(enc, stride_b, stride_v, b, v, cv, encoding, make_baseline_1 != 0,
                                         make_relative != 0, poses, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_pose_compose_backward(const float* enc, int64_t stride_b, int64_t stride_v, int32_t b, int32_t v, int32_t cv,
                              int32_t encoding, int32_t make_baseline_1, int32_t make_relative, const float* dL_dposes,
                              float* dL_denc, void* stream_) {
    if (int rc = check_pose_compose(enc, stride_b, stride_v, b, v, cv, encoding)) return rc;
    if (!dL_dposes || !dL_denc) return fail(SPF_E_INVALID, "pose_compose: null gradient pointer");
    if (!aligned<4>({enc, dL_dposes, dL_denc})) return fail(SPF_E_INVALID, "pose_compose: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_pose_compose_bwd(enc, stride_b, stride_v, b, v, cv, encoding, make_baseline_1 != 0,
                                         make_relative != 0, dL_dposes, dL_denc, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static bool depth_sizes_ok(int32_t N, int32_t n) {
    // (a point number times 3 is a 32-bit index inside an image; slots are 64-bit)
    return N >= 1 && n >= 1 && (int64_t)n * 3 < ((int64_t)1 << 31) && N < (1 << 24);
}

int64_t spf_depth_project_partial_blocks(int32_t N, int32_t n) {
    if (!depth_sizes_ok(N, n)) return -1;
    return spf::depth_slots(N, n, nullptr);
}

static int check_depth(const float* pts, int64_t stride_img, const float* poses, int32_t N, int32_t n) {
    if (!pts || !poses) return fail(SPF_E_INVALID, "depth_project: null pointer");
    if (N < 1 || n < 1) return fail(SPF_E_INVALID, "depth_project: N and n must be positive (got %d %d)", N, n);
    if (!depth_sizes_ok(N, n)) return fail(SPF_E_INVALID, "depth_project: %d x %d points is too large", N, n);
    if (stride_img < 0) return fail(SPF_E_INVALID, "depth_project: a negative image stride is not supported");
    return SPF_OK;
}

int spf_depth_project_forward(const float* pts, int64_t stride_img, const float* poses, int32_t N, int32_t n,
                              float* depth, void* stream_) {
    if (int rc = check_depth(pts, stride_img, poses, N, n)) return rc;
    if (!depth) return fail(SPF_E_INVALID, "depth_project: depth is null");
    if (!aligned<4>({pts, poses, depth})) return fail(SPF_E_INVALID, "depth_project: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_depth_fwd(pts, stride_img, poses, N, n, depth, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_depth_project_backward(const float* pts, int64_t stride_img, const float* poses, int32_t N, int32_t n,
                               const float* dL_ddepth, float* dL_dpts, float* gpartial, float* dL_dposes,
                               void* stream_) {
    if (int rc = check_depth(pts, stride_img, poses, N, n)) return rc;
    if (!dL_ddepth) return fail(SPF_E_INVALID, "depth_project: dL_ddepth is null");
    if (!dL_dpts && !dL_dposes) return fail(SPF_E_INVALID, "depth_project: no gradient requested");
    if ((dL_dposes != nullptr) != (gpartial != nullptr))
        return fail(SPF_E_INVALID, "depth_project: dL_dposes and gpartial go together");
    if (!aligned<4>({pts, poses, dL_ddepth, dL_dpts, dL_dposes}))
        return fail(SPF_E_INVALID, "depth_project: tensors must be 4-byte aligned");
    if (!aligned<16>({gpartial})) return fail(SPF_E_INVALID, "depth_project: gpartial must be 16-byte aligned");
    SPF_HIP(spf::launch_depth_bwd(pts, stride_img, poses, N, n, dL_ddepth, dL_dpts, gpartial, dL_dposes,
                                  static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_pose_error(const float* pred, const float* gt, int32_t N, float* errors, float* means, void* stream_) {
    if (!pred || !gt || !errors || !means) return fail(SPF_E_INVALID, "pose_error: null pointer");
    if (N < 1) return fail(SPF_E_INVALID, "pose_error: N must be positive (got %d)", N);
    if (!aligned<4>({pred, gt, errors, means})) return fail(SPF_E_INVALID, "pose_error: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_pose_error(pred, gt, N, errors, means, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static bool focal_sizes_ok(int32_t B, int32_t H, int32_t W) {
    return B >= 1 && H >= 1 && W >= 1 && (int64_t)H * W * 3 < ((int64_t)1 << 31) && B < (1 << 24);
}

int64_t spf_focal_scratch_bytes(int32_t B, int32_t H, int32_t W) { return focal_sizes_ok(B, H, W) ? 0 : -1; }

int spf_focal_estimate(const float* pts, int64_t stride_scene, int64_t stride_row, int32_t B, int32_t H, int32_t W,
                       const float* pp, int64_t pp_stride, float min_focal, float max_focal, float cx, float cy,
                       float div0, float div1, void* scratch, float* focal, float* intrinsics, void* stream_) {
    (void)scratch;
    if (!pts || !focal) return fail(SPF_E_INVALID, "focal_estimate: null pointer");
    if (B < 1 || H < 1 || W < 1)
        return fail(SPF_E_INVALID, "focal_estimate: B, H, W must be positive (got %d %d %d)", B, H, W);
    if (!focal_sizes_ok(B, H, W)) return fail(SPF_E_INVALID, "focal_estimate: %d x %d x %d points is too large", B, H, W);
    if (stride_scene < 0 || stride_row < 0) return fail(SPF_E_INVALID, "focal_estimate: negative strides are not supported");
    if (pp_stride != 0 && pp_stride != 2) return fail(SPF_E_INVALID, "focal_estimate: pp_stride must be 0 or 2");
    if (!aligned<4>({pts, pp, focal, intrinsics})) return fail(SPF_E_INVALID, "focal_estimate: tensors must be 4-byte aligned");
    // focal_base as the reference forms it (a Python float), the clip bounds as torch.clip receives them
    const double base = (double)(H > W ? H : W) / (2.0 * tan(30.0 * 3.14159265358979323846 / 180.0));
    SPF_HIP(spf::launch_focal(pts, stride_scene, stride_row, B, H, W, pp, pp_stride, (float)base,
                              (float)((double)min_focal * base), (float)((double)max_focal * base), cx, cy, div0, div1,
                              focal, intrinsics, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int64_t spf_reproj_partial_blocks(int32_t B, int32_t V, int32_t H, int32_t W) {
    if (B < 1 || V < 1 || H < 1 || W < 1) return -1;
    return spf::reproj_slots(B, V, H, W, nullptr);
}

static int check_reproj(const SpfReproj* a) {
    if (!a) return fail(SPF_E_INVALID, "reproj: args is null");
    if (!a->pts3d || !a->poses || !a->intrinsics) return fail(SPF_E_INVALID, "reproj: null pointer");
    if (a->B < 1 || a->V < 1 || a->H < 1 || a->W < 1)
        return fail(SPF_E_INVALID, "reproj: B, V, H, W must be positive (got %d %d %d %d)", a->B, a->V, a->H, a->W);
    // (one image's 3 H W floats are indexed with 32-bit point numbers; per-view counts are 32-bit)
    if ((int64_t)a->H * a->W * 3 >= ((int64_t)1 << 31) || (int64_t)a->B * a->H * a->W >= ((int64_t)1 << 31))
        return fail(SPF_E_INVALID, "reproj: %d x %d x %d points is too large", a->B, a->H, a->W);
    if ((int64_t)a->B * a->V >= ((int64_t)1 << 31) / 1024) return fail(SPF_E_INVALID, "reproj: B * V is too large");
    if (a->mode < SPF_REPROJ_TANH || a->mode > SPF_REPROJ_L1_LOG)
        return fail(SPF_E_INVALID, "reproj: mode %d outside 0..3", a->mode);
    if (a->stride_b < 0 || a->stride_v < 0)
        return fail(SPF_E_INVALID, "reproj: negative pts3d strides (%lld, %lld) are not supported",
                    (long long)a->stride_b, (long long)a->stride_v);
    if (!aligned<4>({a->pts3d, a->poses, a->intrinsics})) return fail(SPF_E_INVALID, "reproj: tensors must be 4-byte aligned");
    return SPF_OK;
}

int spf_reproj_forward(const SpfReproj* args, void* partial, float* loss, float* scale, void* stream_) {
    if (int rc = check_reproj(args)) return rc;
    if (!partial || !loss || !scale) return fail(SPF_E_INVALID, "reproj: null pointer");
    if (!aligned<4>({partial})) return fail(SPF_E_INVALID, "reproj: partial must be 4-byte aligned");
    SPF_HIP(spf::launch_reproj_fwd(*args, partial, loss, scale, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_reproj_backward(const SpfReproj* args, const float* scale, const float* dL_dloss, float* dL_dpts3d,
                        float* gpartial, float* dL_dposes, float* dL_dintrinsics, void* stream_) {
    if (int rc = check_reproj(args)) return rc;
    if (!scale || !dL_dloss) return fail(SPF_E_INVALID, "reproj: null pointer");
    const bool cam = dL_dposes || dL_dintrinsics;
    if (!dL_dpts3d && !cam) return fail(SPF_E_INVALID, "reproj: no gradient requested");
    if (cam != (gpartial != nullptr))
        return fail(SPF_E_INVALID, "reproj: gpartial is needed exactly when dL_dposes or dL_dintrinsics is given");
    if (!aligned<16>({gpartial})) return fail(SPF_E_INVALID, "reproj: gpartial must be 16-byte aligned");
    if (!aligned<4>({dL_dpts3d})) return fail(SPF_E_INVALID, "reproj: dL_dpts3d must be 4-byte aligned");
    SPF_HIP(spf::launch_reproj_bwd(*args, scale, dL_dloss, dL_dpts3d, gpartial, dL_dposes, dL_dintrinsics,
                                   static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// sizes of an SSIM call: 0, or the message of the first one that is wrong
static const char* ssim_size_error(int N, int C, int H, int W, int ws) {
    if (N < 1 || C < 1 || H < 1 || W < 1) return "ssim: N, C, H, W must be positive";
    if (ws < 3 || ws > SPF_SSIM_MAX_WIN) return "ssim: window size outside 3..33";
    if (!(ws & 1)) return "ssim: window size must be odd";
    if (H < ws || W < ws) return "ssim: image side shorter than the window";
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return "ssim: H x W is too large";
    if ((int64_t)N * C >= ((int64_t)1 << 31)) return "ssim: N x C is too large";
    return nullptr;
}

int64_t spf_ssim_partial_blocks(int32_t N, int32_t C, int32_t H, int32_t W, int32_t ws) {
    if (ssim_size_error(N, C, H, W, ws)) return -1;
    return spf::ssim_slots(N, C, H, W, ws);
}

static int check_ssim(const SpfSsim* a) {
    if (!a) return fail(SPF_E_INVALID, "ssim: args is null");
    if (const char* e = ssim_size_error(a->N, a->C, a->H, a->W, a->ws))
        return fail(SPF_E_INVALID, "%s (got N %d C %d H %d W %d ws %d)", e, a->N, a->C, a->H, a->W, a->ws);
    if (!a->X || !a->Y) return fail(SPF_E_INVALID, "ssim: null pointer");
    if (!aligned<4>({a->X, a->Y})) return fail(SPF_E_INVALID, "ssim: tensors must be 4-byte aligned");
    return SPF_OK;
}

int spf_ssim_forward(const SpfSsim* args, float* partial, float* plane_mean, float* out, void* stream_) {
    if (int rc = check_ssim(args)) return rc;
    if (!partial || !plane_mean || !out) return fail(SPF_E_INVALID, "ssim: null pointer");
    SPF_HIP(spf::launch_ssim_fwd(*args, partial, plane_mean, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_ssim_backward(const SpfSsim* args, const float* plane_mean, const float* dL_dout, float* dL_dX, float* dL_dY,
                      void* stream_) {
    if (int rc = check_ssim(args)) return rc;
    if (!plane_mean || !dL_dout) return fail(SPF_E_INVALID, "ssim: null pointer");
    if (!dL_dX && !dL_dY) return fail(SPF_E_INVALID, "ssim: no gradient requested");
    if (!aligned<4>({dL_dX, dL_dY})) return fail(SPF_E_INVALID, "ssim: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_ssim_bwd(*args, plane_mean, dL_dout, dL_dX, dL_dY, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_psnr_forward(const float* ground_truth, const float* predicted, int32_t N, int64_t n, float* psnr,
                     void* stream_) {
    if (!ground_truth || !predicted || !psnr) return fail(SPF_E_INVALID, "psnr: null pointer");
    if (N < 1 || n < 1) return fail(SPF_E_INVALID, "psnr: N and n must be positive (got %d, %lld)", N, (long long)n);
    SPF_HIP(spf::launch_psnr(ground_truth, predicted, N, n, psnr, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int rope2d_impl(void* tokens, void* tokens2, const int64_t* positions, int32_t B, int32_t N, int32_t H, int32_t D,
                       int64_t stride_b, int64_t stride_n, int64_t stride_h, int32_t pos_div, int32_t dtype, float base,
                       float fwd, void* stream_) {
    if (!tokens || !positions) return fail(SPF_E_INVALID, "tokens / positions is null");
    if (B < 0 || N < 0 || H < 0 || D <= 0) return fail(SPF_E_INVALID, "negative size");
    if (D % 4 != 0) return fail(SPF_E_INVALID, "token dim must be multiple of 4");
    if (D > 256) return fail(SPF_E_INVALID, "token dim > 256 is not supported");
    if (dtype < 0 || dtype > 2) return fail(SPF_E_INVALID, "dtype must be 0 (f32), 1 (f16) or 2 (bf16)");
    if (pos_div < 1) return fail(SPF_E_INVALID, "pos_div must be >= 1");
    if ((size_t)B * N * H == 0) return SPF_OK;
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    StageScope t(SPF_STAGE_ROPE, stream);
    SPF_HIP(spf::launch_rope2d(tokens, tokens2, positions, B, N, H, D, stride_b, stride_n, stride_h, pos_div, dtype, base,
                               fwd, stream));
    return SPF_OK;
}

int spf_rope2d(void* tokens, const int64_t* positions, int32_t B, int32_t N, int32_t H, int32_t D, int64_t stride_b,
               int64_t stride_n, int64_t stride_h, int32_t pos_div, int32_t dtype, float base, float fwd,
               void* stream_) {
    return rope2d_impl(tokens, nullptr, positions, B, N, H, D, stride_b, stride_n, stride_h, pos_div, dtype, base, fwd,
                       stream_);
}

int spf_rope2d_pair(void* tokens, void* tokens2, const int64_t* positions, int32_t B, int32_t N, int32_t H, int32_t D,
                    int64_t stride_b, int64_t stride_n, int64_t stride_h, int32_t pos_div, int32_t dtype, float base,
                    float fwd, void* stream_) {
    if (!tokens2) return fail(SPF_E_INVALID, "tokens2 is null");
    return rope2d_impl(tokens, tokens2, positions, B, N, H, D, stride_b, stride_n, stride_h, pos_div, dtype, base, fwd,
                       stream_);
}

// arguments of an attention call: 0, or the message of the first one that is wrong
static bool attn_rows_aligned(const void* p, const int64_t* stride, int esize) {
    if (!aligned<16>({p})) return false;
    for (int i = 0; i < 3; ++i)
        if ((stride[i] * esize) % 16 != 0) return false;
    return true;
}
static const char* attn_args_error(const SpfAttn* a) {
    if (!a) return "attention: args is null";
    if (!a->q || !a->k || !a->v) return "attention: q / k / v is null";
    if ((a->qpos == nullptr) != (a->kpos == nullptr)) return "attention: qpos and kpos must both be given or both be null";
    if (a->D != 64) return "attention: head dim must be 64";
    if (a->B < 1 || a->H < 1 || a->Nq < 1 || a->Nk < 1) return "attention: B, H, Nq and Nk must be positive";
    if (a->B > 65535 || a->H > 65535) return "attention: B and H must not exceed 65535";
    if (a->dtype < 0 || a->dtype > 2) return "attention: dtype must be 0 (f32), 1 (f16) or 2 (bf16)";
    const int es = a->dtype == 0 ? 4 : 2;
    if (!attn_rows_aligned(a->q, a->q_stride, es) || !attn_rows_aligned(a->k, a->k_stride, es) ||
        !attn_rows_aligned(a->v, a->v_stride, es))
        return "attention: rows of q, k and v must be 16-byte aligned";
    return nullptr;
}

// a forward call: args, out, lse and alignment
static const char* attn_forward_error(const SpfAttn* a, const void* out, const float* lse) {
    if (const char* e = attn_args_error(a)) return e;
    if (!out || !lse) return "attention: out / lse is null";
    if (!aligned<16>({out})) return "attention: rows of out must be 16-byte aligned";
    return nullptr;
}
// a backward call; ext: the extras with a mask or norm parameters, or null (its outputs are checked in their place)
static const char* attn_backward_error(const SpfAttn* a, const SpfAttnGrads* g, const SpfAttnExt* ext, const void* out,
                                       const float* lse, const void* dout) {
    if (const char* e = attn_args_error(a)) return e;
    if (!g) return "attention: grads is null";
    if (!out || !lse || !dout) return "attention: out / lse / dout is null";
    if (!g->dq || !g->dk || !g->dv || !g->delta) return "attention: dq / dk / dv / delta is null";
    if (ext && ext->q_weight && (!ext->dq_weight || !ext->dq_bias || !ext->dk_weight || !ext->dk_bias || !ext->partials))
        return "attention: dq_weight / dq_bias / dk_weight / dk_bias / partials is null";
    const int es = a->dtype == 0 ? 4 : 2;
    if (!aligned<16>({out, dout})) return "attention: rows of out and dout must be 16-byte aligned";
    if (!attn_rows_aligned(g->dq, g->dq_stride, es) || !attn_rows_aligned(g->dk, g->dk_stride, es) ||
        !attn_rows_aligned(g->dv, g->dv_stride, es))
        return "attention: rows of dq, dk and dv must be 16-byte aligned";
    return nullptr;
}

// the extras of an attention call: 0, or the message of the first one that is wrong
static const char* attn_ext_error(const SpfAttnExt* e) {
    if (!e) return "attention: ext is null";
    if (e->mask) {
        if (e->mask_dtype != 0 && e->mask_dtype != 1) return "attention: mask_dtype must be 0 (float32) or 1 (bool / uint8)";
        if (e->mask_stride[3] != 1) return "attention: the mask's key stride must be 1";
        for (int i = 0; i < 3; ++i)
            if (e->mask_stride[i] < 0) return "attention: mask strides must not be negative";
        if (e->mask_dtype == 0 && !aligned<4>({e->mask})) return "attention: a float32 mask must be 4-byte aligned";
    }
    const int given = (e->q_weight != nullptr) + (e->q_bias != nullptr) + (e->k_weight != nullptr) + (e->k_bias != nullptr);
    if (given != 0 && given != 4) return "attention: q_weight, q_bias, k_weight and k_bias must all be given or all be null";
    if (given == 4 && !(e->eps >= 0.f)) return "attention: eps must not be negative";
    return nullptr;
}
// what the launch takes: null when the extras hold neither a mask nor norm parameters (the unflagged kernels)
static const SpfAttnExt* attn_ext_or_null(const SpfAttnExt* e) { return e->mask || e->q_weight ? e : nullptr; }

int spf_attn_forward(const SpfAttn* args, void* out, float* lse, void* stream_) {
    if (const char* e = attn_forward_error(args, out, lse)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn_forward(*args, nullptr, out, lse, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_attn_backward(const SpfAttn* args, const SpfAttnGrads* g, const void* out, const float* lse, const void* dout,
                      void* stream_) {
    if (const char* e = attn_backward_error(args, g, nullptr, out, lse, dout)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn_backward(*args, *g, nullptr, out, lse, dout, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// the 16-bit matrix path (attention16.hip): the checks of the plain call, and the element type must be a 16-bit one
static const char* attn16_dtype_error(const SpfAttn* a) {
    return a->dtype == 1 || a->dtype == 2 ? nullptr : "attention16: dtype must be 1 (f16) or 2 (bf16)";
}

int spf_attn16_forward(const SpfAttn* args, void* out, float* lse, void* stream_) {
    if (const char* e = attn_forward_error(args, out, lse)) return fail(SPF_E_INVALID, "%s", e);
    if (const char* e = attn16_dtype_error(args)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn16_forward(*args, out, lse, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_attn16_backward(const SpfAttn* args, const SpfAttnGrads* g, const void* out, const float* lse, const void* dout,
                        void* stream_) {
    if (const char* e = attn_backward_error(args, g, nullptr, out, lse, dout)) return fail(SPF_E_INVALID, "%s", e);
    if (const char* e = attn16_dtype_error(args)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn16_backward(*args, *g, out, lse, dout, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int64_t spf_attn_ext_scratch_floats(int32_t B, int32_t H, int32_t Nq, int32_t Nk) {
    if (B < 1 || H < 1 || Nq < 1 || Nk < 1 || B > 65535 || H > 65535) return -1;
    return spf::attn_ext_scratch_floats(B, H, Nq, Nk);
}

int spf_attn_forward_ext(const SpfAttn* args, const SpfAttnExt* ext, void* out, float* lse, void* stream_) {
    if (const char* e = attn_ext_error(ext)) return fail(SPF_E_INVALID, "%s", e);
    if (const char* e = attn_forward_error(args, out, lse)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn_forward(*args, attn_ext_or_null(ext), out, lse, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_attn_backward_ext(const SpfAttn* args, const SpfAttnGrads* g, const SpfAttnExt* ext, const void* out, const float* lse,
                          const void* dout, void* stream_) {
    if (const char* e = attn_ext_error(ext)) return fail(SPF_E_INVALID, "%s", e);
    if (const char* e = attn_backward_error(args, g, ext, out, lse, dout)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn_backward(*args, *g, attn_ext_or_null(ext), out, lse, dout, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// the views of a multi-view attention call (args has passed attn_args_error): 0, or the message of the first thing wrong
static const char* attn_views_error(const SpfAttn* a, const SpfAttnViews* w) {
    if (!w) return "attention: views is null";
    if (w->Vq < 1 || w->Vq > 32 || w->Vk < 1 || w->Vk > 32) return "attention: Vq and Vk must be 1 .. 32";
    const uint32_t known = w->Vk == 32 ? 0xffffffffu : (1u << w->Vk) - 1u;
    for (int i = 0; i < w->Vq; ++i) {
        if (w->allow[i] == 0) return "attention: a query view is allowed no key view";
        if (w->allow[i] & ~known) return "attention: allow names a key view at or above Vk";
    }
    if ((int64_t)a->B * w->Vq > 65535 || (int64_t)a->B * w->Vk > 65535) return "attention: B * Vq and B * Vk must not exceed 65535";
    const int es = a->dtype == 0 ? 4 : 2;
    if ((w->q_view_stride * es) % 16 != 0 || (w->k_view_stride * es) % 16 != 0 || (w->v_view_stride * es) % 16 != 0)
        return "attention: rows of q, k and v must be 16-byte aligned";
    // the kernels form a lane's offset INTO a view in 32 bits (the views themselves are reached through 64-bit strides)
    const int64_t lim = (int64_t)1 << 31;
    if (a->q_stride[1] < 0 || a->k_stride[1] < 0 || a->v_stride[1] < 0 || (int64_t)a->Nq * a->q_stride[1] + 64 >= lim ||
        (int64_t)a->Nk * a->k_stride[1] + 64 >= lim || (int64_t)a->Nk * a->v_stride[1] + 64 >= lim ||
        (int64_t)a->Nq * a->H * 64 >= lim)
        return "attention: the rows of one view must lie within 2^31 elements";
    return nullptr;
}

int spf_attn_views_forward(const SpfAttn* args, const SpfAttnViews* views, void* out, float* lse, void* stream_) {
    if (const char* e = attn_forward_error(args, out, lse)) return fail(SPF_E_INVALID, "%s", e);
    if (const char* e = attn_views_error(args, views)) return fail(SPF_E_INVALID, "%s", e);
    SPF_HIP(spf::launch_attn_views_forward(*args, *views, out, lse, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_attn_views_backward(const SpfAttn* args, const SpfAttnViews* views, const SpfAttnGrads* g, const void* out,
                            const float* lse, const void* dout, void* stream_) {
    if (const char* e = attn_backward_error(args, g, nullptr, out, lse, dout)) return fail(SPF_E_INVALID, "%s", e);
    if (const char* e = attn_views_error(args, views)) return fail(SPF_E_INVALID, "%s", e);
    const int es = args->dtype == 0 ? 4 : 2;
    if ((views->dq_view_stride * es) % 16 != 0 || (views->dk_view_stride * es) % 16 != 0 || (views->dv_view_stride * es) % 16 != 0)
        return fail(SPF_E_INVALID, "attention: rows of dq, dk and dv must be 16-byte aligned");
    SPF_HIP(spf::launch_attn_views_backward(*args, *views, *g, out, lse, dout, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// sizes of an LPIPS call: 0, or the message of the first one that is wrong
static const char* lpips_size_error(int N, int H, int W) {
    if (N < 1 || N > 65535) return "lpips: N must be 1 .. 65535";
    if (H < 16 || W < 16) return "lpips: image side shorter than 16 (the fifth tap would be empty)";
    if ((int64_t)2 * N * H * W * 64 >= ((int64_t)1 << 40)) return "lpips: N x H x W is too large";
    if ((int64_t)2 * N * H * W >= ((int64_t)1 << 31) - 256) return "lpips: N x H x W is too large";
    return nullptr;
}

int64_t spf_lpips_workspace_bytes(int32_t n_with_grad, int32_t n_total, int32_t h, int32_t w) {
    if (n_total < 2 || (n_total & 1) || lpips_size_error(n_total / 2, h, w)) return -1;
    if (n_with_grad != 0 && n_with_grad != n_total / 2 && n_with_grad != n_total) return -1;
    return spf::lpips_workspace_bytes(n_with_grad, n_total, h, w);
}

static int check_lpips(const SpfLpips* a, bool first_only) {
    if (!a) return fail(SPF_E_INVALID, "lpips: args is null");
    if (const char* e = lpips_size_error(a->N, a->H, a->W))
        return fail(SPF_E_INVALID, "%s (got N %d H %d W %d)", e, a->N, a->H, a->W);
    if (!a->in0 || (!first_only && !a->in1)) return fail(SPF_E_INVALID, "lpips: null image pointer");
    const int64_t img = (int64_t)3 * a->H * a->W;
    if (a->stride0 < img || (!first_only && a->stride1 < img))
        return fail(SPF_E_INVALID, "lpips: image stride shorter than 3 H W");
    if (!aligned<4>({a->in0, a->in1})) return fail(SPF_E_INVALID, "lpips: images must be 4-byte aligned");
    if (!a->wfwd || !a->wbwd || !a->bias || !a->shift_scale || (!first_only && !a->lin))
        return fail(SPF_E_INVALID, "lpips: null weight pointer");
    if (!aligned<16>({a->wfwd, a->wbwd})) return fail(SPF_E_INVALID, "lpips: weight packs must be 16-byte aligned");
    return SPF_OK;
}

int spf_lpips_forward(const SpfLpips* args, void* workspace, float* out, float* mean, void* stream_) {
    if (int rc = check_lpips(args, false)) return rc;
    if (!workspace || !out) return fail(SPF_E_INVALID, "lpips: null pointer");
    if (!aligned<16>({workspace})) return fail(SPF_E_INVALID, "lpips: workspace must be 16-byte aligned");
    SPF_HIP(spf::launch_lpips_fwd(*args, static_cast<float*>(workspace), out, mean, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_lpips_backward(const SpfLpips* args, void* workspace, const float* dL_dout, int32_t upstream_is_mean,
                       float* d_in0, float* d_in1, void* stream_) {
    if (int rc = check_lpips(args, false)) return rc;
    if (!workspace || !dL_dout) return fail(SPF_E_INVALID, "lpips: null pointer");
    if (!aligned<16>({workspace})) return fail(SPF_E_INVALID, "lpips: workspace must be 16-byte aligned");
    if (!d_in0 && !d_in1) return fail(SPF_E_INVALID, "lpips: no gradient requested");
    SPF_HIP(spf::launch_lpips_bwd(*args, static_cast<float*>(workspace), dL_dout, upstream_is_mean ? 1 : 0, d_in0, d_in1,
                                  static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int check_lpips_map(const char* what, int32_t n, int32_t h, int32_t w, int32_t c, int32_t cmul) {
    if (n < 1 || h < 1 || w < 1 || c < 1) return fail(SPF_E_INVALID, "%s: n, h, w, c must be positive", what);
    if (c % cmul) return fail(SPF_E_INVALID, "%s: channel count %d is not a multiple of %d", what, c, cmul);
    if ((int64_t)n * h * w >= ((int64_t)1 << 31) - 256) return fail(SPF_E_INVALID, "%s: n x h x w is too large", what);
    return SPF_OK;
}

int spf_lpips_conv3x3(const float* in, const float* mask, const float* wpack, const float* bias, float* out, int32_t n,
                      int32_t h, int32_t w, int32_t cin, int32_t cout, int32_t relu, void* stream_) {
    if (int rc = check_lpips_map("lpips conv3x3", n, h, w, cin, 16)) return rc;
    if (cout < 64 || cout % 64) return fail(SPF_E_INVALID, "lpips conv3x3: cout %d is not a multiple of 64", cout);
    if (!in || !wpack || !out) return fail(SPF_E_INVALID, "lpips conv3x3: null pointer");
    if (!aligned<16>({in, mask, wpack, out})) return fail(SPF_E_INVALID, "lpips conv3x3: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_lpips_conv(in, mask, wpack, bias, out, n, h, w, cin, cout, relu ? 1 : 0,
                                   static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_lpips_conv1_forward(const SpfLpips* args, float* out, void* stream_) {
    if (int rc = check_lpips(args, true)) return rc;
    if (!out || !aligned<16>({out})) return fail(SPF_E_INVALID, "lpips conv1: out is null or not 16-byte aligned");
    SPF_HIP(spf::launch_lpips_conv1(*args, args->N, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_lpips_conv1_backward(const SpfLpips* args, const float* g, const float* act, float* d_in0, void* stream_) {
    if (int rc = check_lpips(args, true)) return rc;
    if (!g || !act || !d_in0) return fail(SPF_E_INVALID, "lpips conv1 backward: null pointer");
    if (!aligned<16>({g, act})) return fail(SPF_E_INVALID, "lpips conv1 backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_lpips_conv1_bwd(*args, g, act, args->N, d_in0, args->N, nullptr, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_lpips_pool_forward(const float* in, float* out, int32_t n, int32_t h, int32_t w, int32_t c, void* stream_) {
    if (int rc = check_lpips_map("lpips pool", n, h, w, c, 4)) return rc;
    if (!in || !out || !aligned<16>({in, out}))
        return fail(SPF_E_INVALID, "lpips pool: null or not 16-byte aligned pointer");
    SPF_HIP(spf::launch_lpips_pool(in, out, n, h, w, c, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_lpips_pool_backward(const float* gp, const float* act, float* inout, int32_t n, int32_t h, int32_t w, int32_t c,
                            void* stream_) {
    if (int rc = check_lpips_map("lpips pool backward", n, h, w, c, 4)) return rc;
    if (!gp || !act || !inout || !aligned<16>({gp, act, inout}))
        return fail(SPF_E_INVALID, "lpips pool backward: null or not 16-byte aligned pointer");
    SPF_HIP(spf::launch_lpips_pool_bwd(gp, act, inout, n, h, w, c, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int check_lpips_head(int32_t n, int32_t hw, int32_t c) {
    if (n < 1 || hw < 1) return fail(SPF_E_INVALID, "lpips head: n and hw must be positive");
    if (c != 64 && c != 128 && c != 256 && c != 512) return fail(SPF_E_INVALID, "lpips head: c must be 64, 128, 256 or 512 (got %d)", c);
    if ((int64_t)n * hw >= ((int64_t)1 << 31) - 256) return fail(SPF_E_INVALID, "lpips head: n x hw is too large");
    if (n > 65535) return fail(SPF_E_INVALID, "lpips head: more than 65535 pairs");
    return SPF_OK;
}

int spf_lpips_head_forward(const float* fa, const float* fb, const float* lin, int32_t n, int32_t hw, int32_t c,
                           float* partial, float* out, void* stream_) {
    if (int rc = check_lpips_head(n, hw, c)) return rc;
    if (!fa || !fb || !lin || !partial || !out) return fail(SPF_E_INVALID, "lpips head: null pointer");
    SPF_HIP(spf::launch_lpips_head_single(fa, fb, lin, n, hw, c, partial, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_lpips_head_backward(const float* fa, const float* fb, const float* lin, int32_t n, int32_t hw, int32_t c,
                            const float* up, float* d_a, float* d_b, void* stream_) {
    if (int rc = check_lpips_head(n, hw, c)) return rc;
    if (!fa || !fb || !lin || !up) return fail(SPF_E_INVALID, "lpips head: null pointer");
    if (!d_a && !d_b) return fail(SPF_E_INVALID, "lpips head: no gradient requested");
    SPF_HIP(spf::launch_lpips_head_bwd(fa, fb, lin, n, hw, c, up, 0, 0.f, d_a, d_b, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int64_t spf_optim_chunks(const int64_t* numel, int32_t T) {
    if (!numel) return fail(SPF_E_INVALID, "optim: numel is null");
    if (T <= 0) return fail(SPF_E_INVALID, "optim: T must be positive (got %d)", T);
    int64_t chunks = 0;
    for (int32_t t = 0; t < T; ++t) {
        if (numel[t] <= 0) return fail(SPF_E_INVALID, "optim: tensor %d has numel %lld; it must be positive", t, (long long)numel[t]);
        chunks += spf::optim_chunks_of(numel[t]);
    }
    return chunks;
}

int64_t spf_optim_plan(const SpfOptimTensor* table, int32_t T, int32_t num_groups, int64_t* chunk_start) {
    if (!table) return fail(SPF_E_INVALID, "optim: table is null");
    if (T <= 0) return fail(SPF_E_INVALID, "optim: T must be positive (got %d)", T);
    if (num_groups < 1 || num_groups > SPF_OPTIM_MAX_GROUPS)
        return fail(SPF_E_INVALID, "optim: %d parameter groups; 1 .. %d are supported", num_groups, SPF_OPTIM_MAX_GROUPS);
    int64_t chunks = 0;
    for (int32_t t = 0; t < T; ++t) {
        const SpfOptimTensor& e = table[t];
        if (!e.param || !e.exp_avg || !e.exp_avg_sq) return fail(SPF_E_INVALID, "optim: tensor %d has a null pointer", t);
        if (!aligned<4>({e.param, e.exp_avg, e.exp_avg_sq}))
            return fail(SPF_E_INVALID, "optim: tensor %d is not 4-byte aligned", t);
        if (e.numel <= 0) return fail(SPF_E_INVALID, "optim: tensor %d has numel %lld; it must be positive", t, (long long)e.numel);
        if (e.group < 0 || e.group >= num_groups)
            return fail(SPF_E_INVALID, "optim: tensor %d names group %d, out of range 0 .. %d", t, e.group, num_groups - 1);
        if (chunk_start) chunk_start[t] = chunks;
        chunks += spf::optim_chunks_of(e.numel);
    }
    if (chunk_start) chunk_start[T] = chunks;
    return chunks;
}

int64_t spf_optim_scratch_bytes(int32_t T, int64_t chunks) {
    if (T <= 0 || chunks < T) return fail(SPF_E_INVALID, "optim: T must be positive and chunks >= T (got %d, %lld)", T, (long long)chunks);
    return spf::optim_scratch_bytes(T, chunks);
}

int spf_optim_step(const SpfOptim* o, const SpfOptimHyper* hp, void* stream_) {
    if (!o || !hp) return fail(SPF_E_INVALID, "optim: args / hyper is null");
    if (!o->table) return fail(SPF_E_INVALID, "optim: table is null");
    if (o->T <= 0) return fail(SPF_E_INVALID, "optim: T must be positive (got %d)", o->T);
    if (o->chunks < o->T) return fail(SPF_E_INVALID, "optim: chunks = %lld is below T = %d", (long long)o->chunks, o->T);
    if (!o->chunk_start || !o->grads || !o->guard_order || !o->step || !o->scratch || !o->report)
        return fail(SPF_E_INVALID, "optim: null pointer");
    if (!aligned<16>({o->scratch, o->report}))
        return fail(SPF_E_INVALID, "optim: scratch and report must be 16-byte aligned");
    if (hp->num_groups < 1 || hp->num_groups > SPF_OPTIM_MAX_GROUPS)
        return fail(SPF_E_INVALID, "optim: %d parameter groups; 1 .. %d are supported", hp->num_groups, SPF_OPTIM_MAX_GROUPS);
    if (hp->guard && !(hp->max_grad_value >= 0.0)) return fail(SPF_E_INVALID, "optim: max_grad_value must be >= 0");
    if (hp->clip && !(hp->max_norm >= 0.0)) return fail(SPF_E_INVALID, "optim: max_norm must be >= 0");
    for (int32_t i = 0; i < hp->num_groups; ++i) {
        const SpfOptimGroup& g = hp->group[i];
        if (!(g.lr >= 0.0) || !(g.eps >= 0.0) || !(g.weight_decay >= 0.0) || !(g.beta1 >= 0.0 && g.beta1 < 1.0) ||
            !(g.beta2 >= 0.0 && g.beta2 < 1.0))
            return fail(SPF_E_INVALID, "optim: group %d: lr, eps, weight_decay must be >= 0 and the betas in [0, 1)", i);
    }
    SPF_HIP(spf::launch_optim_step(*o, *hp, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// ---- the transformer block's row work ----------------------------------------------------------------------------------
static bool block_sizes_ok(int64_t rows, int32_t C) {
    return rows >= 1 && rows <= ((int64_t)1 << 30) && C >= 4 && C <= SPF_BLOCK_MAX_C && C % 4 == 0;
}
static int block_sizes_fail(const char* what, int64_t rows, int32_t C) {
    return fail(SPF_E_INVALID, "%s: rows must be 1 .. 2^30 and C a multiple of 4 in 4 .. %d (got rows = %lld, C = %d)", what,
                SPF_BLOCK_MAX_C, (long long)rows, C);
}
// one addressed operand of SpfBlockNorm: the group size and the two strides
static bool block_rows_ok(int64_t inner, int64_t stride, int64_t outer_stride) {
    return inner >= 1 && inner <= ((int64_t)1 << 30) && stride >= 0 && outer_stride >= 0 && stride % 4 == 0 &&
           outer_stride % 4 == 0;
}
static int block_norm_check(const char* what, const SpfBlockNorm* a, bool backward) {
    if (!a) return fail(SPF_E_INVALID, "%s: args is null", what);
    if (!block_sizes_ok(a->rows, a->C)) return block_sizes_fail(what, a->rows, a->C);
    if (!a->x || !a->weight || (!backward && !a->bias)) return fail(SPF_E_INVALID, "%s: null pointer (x, weight or bias)", what);
    if (a->gamma && !a->r) return fail(SPF_E_INVALID, "%s: gamma is given without r", what);
    if (backward && a->r && !a->gamma) return fail(SPF_E_INVALID, "%s: the backward reads r only with gamma; pass r = null", what);
    if (!(a->eps >= 0.f)) return fail(SPF_E_INVALID, "%s: eps must be >= 0", what);
    if (!block_rows_ok(a->x_inner, a->x_stride, a->x_outer_stride) || (a->r && !block_rows_ok(a->r_inner, a->r_stride, a->r_outer_stride)))
        return fail(SPF_E_INVALID, "%s: group sizes must be >= 1 and strides non-negative multiples of 4 floats", what);
    if (!aligned<16>({a->x, a->r, a->gamma, a->weight, a->bias}))
        return fail(SPF_E_INVALID, "%s: tensors must be 16-byte aligned", what);
    return SPF_OK;
}

int64_t spf_block_partial_blocks(int64_t rows, int32_t C, int32_t gelu) {
    if (!block_sizes_ok(rows, C)) return block_sizes_fail("block_partial_blocks", rows, C);
    return spf::block_partial_blocks(rows, C, gelu != 0);
}

int spf_block_add_norm_forward(const SpfBlockNorm* a, float* s, float* y, float* stats, void* stream_) {
    if (const int rc = block_norm_check("block_add_norm_forward", a, false)) return rc;
    if (!y || !stats || (a->r && !s)) return fail(SPF_E_INVALID, "block_add_norm_forward: null output pointer");
    if (!aligned<16>({s, y, stats})) return fail(SPF_E_INVALID, "block_add_norm_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_block_norm_fwd(*a, s, y, stats, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_block_add_norm_backward(const SpfBlockNorm* a, const float* dy, const float* ds, const float* stats, float* dx,
                                float* dr, float* partials, float* dparams, void* stream_) {
    if (const int rc = block_norm_check("block_add_norm_backward", a, true)) return rc;
    if (!dy || !stats || !dx || !partials || !dparams) return fail(SPF_E_INVALID, "block_add_norm_backward: null pointer");
    if ((a->gamma != nullptr) != (dr != nullptr))
        return fail(SPF_E_INVALID, "block_add_norm_backward: dr is written with gamma only (without it dr is dx)");
    if (!aligned<16>({dy, ds, stats, dx, dr, partials, dparams}))
        return fail(SPF_E_INVALID, "block_add_norm_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_block_norm_bwd(*a, dy, ds, stats, dx, dr, partials, dparams, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_block_bias_gelu_forward(const float* u, const float* bias, int64_t rows, int32_t C, float* h, void* stream_) {
    if (!block_sizes_ok(rows, C)) return block_sizes_fail("block_bias_gelu_forward", rows, C);
    if (!u || !h) return fail(SPF_E_INVALID, "block_bias_gelu_forward: null pointer");
    if (!aligned<16>({u, bias, h})) return fail(SPF_E_INVALID, "block_bias_gelu_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_block_gelu_fwd(u, bias, rows, C, h, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_block_bias_gelu_backward(const float* u, const float* bias, const float* dh, int64_t rows, int32_t C, float* du,
                                 float* partials, float* dbias, void* stream_) {
    if (!block_sizes_ok(rows, C)) return block_sizes_fail("block_bias_gelu_backward", rows, C);
    if (!u || !dh || !du) return fail(SPF_E_INVALID, "block_bias_gelu_backward: null pointer");
    if (bias ? (!partials || !dbias) : (partials || dbias))
        return fail(SPF_E_INVALID, "block_bias_gelu_backward: partials and dbias are given with a bias and only then");
    if (!aligned<16>({u, bias, dh, du, partials, dbias}))
        return fail(SPF_E_INVALID, "block_bias_gelu_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_block_gelu_bwd(u, bias, dh, rows, C, du, partials, dbias, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// ---- the DPT heads' work between the convolutions ------------------------------------------------------------------------
// every tensor of a call stays below 2^31 elements, so no index product can overflow
static const int64_t kDptMaxElements = ((int64_t)1 << 31) - 1;

int32_t spf_dpt_max_grid(void) { return spf::dpt_max_grid(); }

static int dpt_up2_check(const char* what, int64_t planes, int32_t h, int32_t w) {
    if (planes < 1 || h < 1 || w < 1)
        return fail(SPF_E_INVALID, "%s: planes, h and w must be positive (got %lld, %d, %d)", what, (long long)planes, h, w);
    if (h > SPF_DPT_MAX_SIDE || w > SPF_DPT_MAX_SIDE || planes > kDptMaxElements || planes * 4 * h * w > kDptMaxElements)
        return fail(SPF_E_INVALID, "%s: h and w must not exceed %d and the output must stay below 2^31 elements (got "
                    "planes = %lld, h = %d, w = %d)", what, SPF_DPT_MAX_SIDE, (long long)planes, h, w);
    return SPF_OK;
}

int spf_dpt_upsample2x_forward(const float* x, const float* skip, int32_t relu_skip, int64_t planes, int32_t h, int32_t w,
                               float* out, void* stream_) {
    if (const int rc = dpt_up2_check("dpt_upsample2x_forward", planes, h, w)) return rc;
    if (!x || !out) return fail(SPF_E_INVALID, "dpt_upsample2x_forward: null pointer (x or out)");
    if (relu_skip && !skip) return fail(SPF_E_INVALID, "dpt_upsample2x_forward: relu_skip is set without skip");
    if (!aligned<16>({x, skip, out})) return fail(SPF_E_INVALID, "dpt_upsample2x_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_dpt_up2_fwd(x, skip, relu_skip != 0, planes, h, w, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_dpt_upsample2x_backward(const float* dy, const float* skip, int64_t planes, int32_t h, int32_t w, float* dx,
                                float* dskip, void* stream_) {
    if (const int rc = dpt_up2_check("dpt_upsample2x_backward", planes, h, w)) return rc;
    if (!dy || (!dx && !dskip))
        return fail(SPF_E_INVALID, "dpt_upsample2x_backward: null pointer (dy; dx may be null only where dskip is written)");
    if ((skip != nullptr) != (dskip != nullptr))
        return fail(SPF_E_INVALID, "dpt_upsample2x_backward: skip and dskip are given with the ReLU flag and only then "
                    "(without it dskip is dy)");
    if (!aligned<16>({dy, skip, dx, dskip})) return fail(SPF_E_INVALID, "dpt_upsample2x_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_dpt_up2_bwd(dy, skip, planes, h, w, dx, dskip, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int dpt_count_check(const char* what, int64_t n) {
    if (n < 1 || n > kDptMaxElements)
        return fail(SPF_E_INVALID, "%s: n must be 1 .. 2^31 - 1 (got %lld)", what, (long long)n);
    return SPF_OK;
}

int spf_dpt_add_relu_forward(const float* a, const float* b, const float* c, int64_t n, float* s, float* y, void* stream_) {
    if (const int rc = dpt_count_check("dpt_add_relu_forward", n)) return rc;
    if (!a || !y) return fail(SPF_E_INVALID, "dpt_add_relu_forward: null pointer (a or y)");
    if (c && !b) return fail(SPF_E_INVALID, "dpt_add_relu_forward: c is given without b");
    if ((b != nullptr) != (s != nullptr))
        return fail(SPF_E_INVALID, "dpt_add_relu_forward: s is written with a second addend and only then (without one s is a)");
    if (!aligned<16>({a, b, c, s, y})) return fail(SPF_E_INVALID, "dpt_add_relu_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_dpt_add_relu_fwd(a, b, c, n, s, y, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_dpt_add_relu_backward(const float* mask, const float* dy, const float* ds, int64_t n, float* g, void* stream_) {
    if (const int rc = dpt_count_check("dpt_add_relu_backward", n)) return rc;
    if (!mask || !dy || !g) return fail(SPF_E_INVALID, "dpt_add_relu_backward: null pointer (mask, dy or g)");
    if (!aligned<16>({mask, dy, ds, g})) return fail(SPF_E_INVALID, "dpt_add_relu_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_dpt_add_relu_bwd(mask, dy, ds, n, g, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int dpt_points_check(const char* what, const SpfDptPoints* a) {
    if (!a) return fail(SPF_E_INVALID, "%s: args is null", what);
    if (a->B < 1 || a->HW < 1 || a->C < 3 + (a->has_conf ? 1 : 0) || a->C > 4096)
        return fail(SPF_E_INVALID, "%s: B and HW must be positive and C at least 3 (4 with conf) (got %lld, %lld, %d)", what,
                    (long long)a->B, (long long)a->HW, a->C);
    if (a->B > kDptMaxElements || a->HW > kDptMaxElements || a->B * a->HW > kDptMaxElements / a->C)
        return fail(SPF_E_INVALID, "%s: the head output must stay below 2^31 elements (got B = %lld, C = %d, HW = %lld)", what,
                    (long long)a->B, a->C, (long long)a->HW);
    if (!a->in) return fail(SPF_E_INVALID, "%s: null pointer (in)", what);
    if (!(a->depth_min <= a->depth_max)) return fail(SPF_E_INVALID, "%s: depth bounds must be ordered", what);
    if (a->has_conf && !(a->conf_max - a->conf_min >= 0.f)) return fail(SPF_E_INVALID, "%s: conf bounds must be ordered", what);
    return SPF_OK;
}

int spf_dpt_points_forward(const SpfDptPoints* a, float* pts3d, float* conf, void* stream_) {
    if (const int rc = dpt_points_check("dpt_points_forward", a)) return rc;
    if (!pts3d || (a->has_conf != 0) != (conf != nullptr))
        return fail(SPF_E_INVALID, "dpt_points_forward: null output pointer (pts3d; conf is given with has_conf and only then)");
    if (!aligned<16>({a->in, pts3d, conf})) return fail(SPF_E_INVALID, "dpt_points_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_dpt_points(1, a->in, nullptr, nullptr, a->B, a->HW, a->C, a->has_conf, a->depth_min, a->depth_max,
                                   a->conf_min, a->conf_max, pts3d, conf, nullptr, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_dpt_points_backward(const SpfDptPoints* a, const float* dpts3d, const float* dconf, float* din, void* stream_) {
    if (const int rc = dpt_points_check("dpt_points_backward", a)) return rc;
    if (!dpts3d || !din || (a->has_conf != 0) != (dconf != nullptr))
        return fail(SPF_E_INVALID, "dpt_points_backward: null pointer (dpts3d, din; dconf is given with has_conf and only then)");
    if (!aligned<16>({a->in, dpts3d, dconf, din})) return fail(SPF_E_INVALID, "dpt_points_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_dpt_points(0, a->in, dpts3d, dconf, a->B, a->HW, a->C, a->has_conf, a->depth_min, a->depth_max,
                                   a->conf_min, a->conf_max, nullptr, nullptr, din, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// ---- the encoder front (front.hip) -------------------------------------------------------------------------------------
int64_t spf_front_geometry(int32_t what, int64_t M) { return spf::front_geometry(what, M < 0 ? 0 : M); }

static int front_check(const char* what, const SpfFront* a) {
    if (!a) return fail(SPF_E_INVALID, "%s: args is null", what);
    if (a->P != 14 && a->P != 16) return fail(SPF_E_INVALID, "%s: the patch size must be 14 or 16 (got %d)", what, a->P);
    if (a->B < 1 || a->gh < 1 || a->gw < 1 || (int64_t)a->B * a->gh * a->gw > 0x7fffffffLL || (int64_t)a->gw * a->P > 0x7fffffffLL ||
        (int64_t)a->gh * a->gw > 0x7fffffffLL)
        return fail(SPF_E_INVALID, "%s: B, gh, gw must be positive and B gh gw < 2^31 (got %d, %d, %d)", what, a->B, a->gh, a->gw);
    if (a->C_in < 1 || a->C_in > 32) return fail(SPF_E_INVALID, "%s: C_in must be 1 .. 32 (got %d)", what, a->C_in);
    if (a->C < 4 || a->C % 4 != 0) return fail(SPF_E_INVALID, "%s: C must be a positive multiple of 4 (got %d)", what, a->C);
    if (a->before < 0 || a->after < 0 || (int64_t)a->before + a->after + (int64_t)a->gh * a->gw > 0x7fffffffLL)
        return fail(SPF_E_INVALID, "%s: before and after must be >= 0 and the rows of an image < 2^31", what);
    if (!a->image) return fail(SPF_E_INVALID, "%s: null pointer (image)", what);
    const int v = a->P == 16 ? 4 : 2;
    if ((reinterpret_cast<uintptr_t>(a->image) & (4 * v - 1)) != 0 || a->stride_b % v || a->stride_c % v || a->stride_y % v ||
        a->stride_b < 0 || a->stride_c < 0 || a->stride_y < (int64_t)a->gw * a->P)
        return fail(SPF_E_INVALID, "%s: the image must be %d-byte aligned with strides that are multiples of %d floats and rows "
                    "that do not overlap", what, 4 * v, v);
    if (!aligned<16>({a->affine})) return fail(SPF_E_INVALID, "%s: affine must be 16-byte aligned", what);
    return SPF_OK;
}

int64_t spf_front_workspace_floats(const SpfFront* a, int32_t with_dweight) {
    if (front_check("front_workspace_floats", a)) return -1;
    return spf::front_workspace_floats(*a, with_dweight != 0);
}

int spf_front_embed_forward(const SpfFront* a, const float* weight, const float* bias, const float* pos_table, float* out,
                            void* stream_) {
    if (const int rc = front_check("front_embed_forward", a)) return rc;
    if (!weight || !out) return fail(SPF_E_INVALID, "front_embed_forward: null pointer (weight or out)");
    if (!aligned<16>({weight, bias, pos_table, out})) return fail(SPF_E_INVALID, "front_embed_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_front_embed_fwd(*a, weight, bias, pos_table, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int front_tokens_check(const char* what, const SpfFrontTokens* t, int64_t S, int32_t N, int32_t C, bool sources) {
    if (!t) return fail(SPF_E_INVALID, "%s: tokens is null", what);
    if (S < 1 || N < 0 || C < 4 || C % 4 != 0 || S > 0x7fffffffLL)
        return fail(SPF_E_INVALID, "%s: S must be 1 .. 2^31 - 1, N >= 0, C a positive multiple of 4 (got %lld, %d, %d)", what, (long long)S, N, C);
    if (t->n_before < 0 || t->n_after < 0 || t->n_before + t->n_after > SPF_FRONT_MAX_TOKENS)
        return fail(SPF_E_INVALID, "%s: at most %d token tensors (got %d + %d)", what, SPF_FRONT_MAX_TOKENS, t->n_before, t->n_after);
    int64_t before = 0, after = 0;
    for (int g = 0; g < t->n_before + t->n_after; ++g) {
        if (t->rows[g] < 1) return fail(SPF_E_INVALID, "%s: token tensor %d has %d rows", what, g, t->rows[g]);
        if (sources && !t->tok[g]) return fail(SPF_E_INVALID, "%s: null pointer (token tensor %d)", what, g);
        if (!aligned<16>({t->tok[g]})) return fail(SPF_E_INVALID, "%s: token tensor %d must be 16-byte aligned", what, g);
        (g < t->n_before ? before : after) += t->rows[g];
    }
    if (before != t->before || after != t->after)
        return fail(SPF_E_INVALID, "%s: before / after (%d / %d) are not the sums of the tensors' rows (%lld / %lld)", what,
                    t->before, t->after, (long long)before, (long long)after);
    if (before + after + N > 0x7fffffffLL || S * (before + after + N) > 0x7fffffffLL)
        return fail(SPF_E_INVALID, "%s: S (before + N + after) must stay below 2^31", what);
    if (t->pos_first && t->before < 1) return fail(SPF_E_INVALID, "%s: pos_first without a row in front", what);
    if (!aligned<16>({t->pos_first})) return fail(SPF_E_INVALID, "%s: pos_first must be 16-byte aligned", what);
    return SPF_OK;
}

int spf_front_assemble(const SpfFrontTokens* t, const float* body, int64_t inner, int64_t stride, int64_t outer_stride,
                       int64_t S, int32_t N, int32_t C, float* out, void* stream_) {
    if (const int rc = front_tokens_check("front_assemble", t, S, N, C, true)) return rc;
    if (!out) return fail(SPF_E_INVALID, "front_assemble: null pointer (out)");
    if (body && (inner < 1 || stride < 0 || outer_stride < 0 || stride % 4 || outer_stride % 4))
        return fail(SPF_E_INVALID, "front_assemble: the body's rows need inner >= 1 and strides that are multiples of 4 floats");
    if (!aligned<16>({body, out})) return fail(SPF_E_INVALID, "front_assemble: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_front_assemble(*t, body, inner, stride, outer_stride, S, N, C, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int front_dy_check(const char* what, const float* dY, int64_t ss, int64_t sr, int32_t C) {
    if (!dY) return fail(SPF_E_INVALID, "%s: null pointer (dY)", what);
    if (!aligned<16>({dY}) || ss < 0 || sr < C || ss % 4 || sr % 4)
        return fail(SPF_E_INVALID, "%s: dY must be 16-byte aligned with strides that are multiples of 4 floats, rows apart", what);
    return SPF_OK;
}

int spf_front_tokens_backward(const SpfFrontTokens* t, const float* dY, int64_t dy_stride_s, int64_t dy_stride_r, int64_t S,
                              int32_t N, int32_t C, float* d_pos_first, void* stream_) {
    if (const int rc = front_tokens_check("front_tokens_backward", t, S, N, C, false)) return rc;
    if (const int rc = front_dy_check("front_tokens_backward", dY, dy_stride_s, dy_stride_r, C)) return rc;
    if (d_pos_first && t->before < 1) return fail(SPF_E_INVALID, "front_tokens_backward: d_pos_first without a row in front");
    if (!aligned<16>({d_pos_first})) return fail(SPF_E_INVALID, "front_tokens_backward: d_pos_first must be 16-byte aligned");
    SPF_HIP(spf::launch_front_tokens_bwd(*t, dY, dy_stride_s, dy_stride_r, S, N, C, d_pos_first, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_front_embed_backward(const SpfFront* a, const float* dY, int64_t dy_stride_b, int64_t dy_stride_r, float* workspace,
                             float* dweight, float* dbias, float* dpos_table, void* stream_) {
    if (const int rc = front_check("front_embed_backward", a)) return rc;
    if (const int rc = front_dy_check("front_embed_backward", dY, dy_stride_b, dy_stride_r, a->C)) return rc;
    if (!workspace) return fail(SPF_E_INVALID, "front_embed_backward: null pointer (workspace)");
    if (!aligned<16>({workspace, dweight, dbias, dpos_table})) return fail(SPF_E_INVALID, "front_embed_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_front_embed_bwd(*a, dY, dy_stride_b, dy_stride_r, workspace, dweight, dbias, dpos_table, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// ---- PnP pose from point maps (pnp.hip) --------------------------------------------------------------------------------
// h w < 2^24 keeps every pixel index and count in 32 bits with room to spare; b v is the y extent of the score grid
static bool pnp_sizes_ok(int64_t views, int32_t h, int32_t w, int32_t iterations) {
    return views >= 1 && views <= 65535 && h >= 1 && w >= 1 && (int64_t)h * w < ((int64_t)1 << 24) && iterations >= 64 &&
           iterations <= 1024 && iterations % 64 == 0;
}

int64_t spf_pnp_workspace_bytes(int32_t views, int32_t h, int32_t w, int32_t iterations) {
    return pnp_sizes_ok(views, h, w, iterations) ? spf::pnp_workspace_bytes(views, h, w, iterations) : -1;
}

int spf_pnp_solve(const SpfPnp* a, void* workspace, float* poses, int32_t* info, int32_t* ranks, void* stream_) {
    if (!a) return fail(SPF_E_INVALID, "pnp_solve: args is null");
    if (a->b < 1 || a->v < 1) return fail(SPF_E_INVALID, "pnp_solve: b and v must be positive (got %d %d)", a->b, a->v);
    if (a->iterations < 64 || a->iterations > 1024 || a->iterations % 64 != 0)
        return fail(SPF_E_INVALID, "pnp_solve: iterations must be a multiple of 64 in 64..1024 (got %d)", a->iterations);
    if (!pnp_sizes_ok((int64_t)a->b * a->v, a->h, a->w, a->iterations))
        return fail(SPF_E_INVALID, "pnp_solve: %d x %d views of %d x %d pixels is not a supported size", a->b, a->v, a->h, a->w);
    if (a->refine_steps < 0 || a->refine_steps > 64)
        return fail(SPF_E_INVALID, "pnp_solve: refine_steps must be in 0..64 (got %d)", a->refine_steps);
    if (!(a->reprojection_error > 0.f) || !isfinite(a->reprojection_error) || isnan(a->opacity_threshold))
        return fail(SPF_E_INVALID, "pnp_solve: reprojection_error must be positive and finite, opacity_threshold a number");
    if (!a->pts3d || !a->opacity || !a->K || !workspace || !poses || !info) return fail(SPF_E_INVALID, "pnp_solve: null pointer");
    for (int i = 0; i < 4; ++i)
        if (a->pts_stride[i] < 0 || a->opa_stride[i] < 0) return fail(SPF_E_INVALID, "pnp_solve: negative strides are not supported");
    if (!aligned<4>({a->pts3d, a->opacity, a->K, poses, info, ranks})) return fail(SPF_E_INVALID, "pnp_solve: tensors must be 4-byte aligned");
    if (!aligned<16>({workspace})) return fail(SPF_E_INVALID, "pnp_solve: workspace must be 16-byte aligned");
    SPF_HIP(spf::launch_pnp_solve(*a, workspace, poses, info, ranks, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// ---- the encoder tail (tail.hip) ---------------------------------------------------------------------------------------
int32_t spf_tail_max_grid(void) { return spf::tail_max_grid(); }

static int tail_check(const char* what, const SpfTail* a, bool need_pts) {
    if (!a) return fail(SPF_E_INVALID, "%s: args is null", what);
    if (a->b < 1 || a->hw < 1 || a->v < 1 || a->v > SPF_TAIL_MAX_VIEWS)
        return fail(SPF_E_INVALID, "%s: b and hw must be positive and v in 1..%d (got b = %d, v = %d, hw = %lld)", what,
                    SPF_TAIL_MAX_VIEWS, a->b, a->v, (long long)a->hw);
    if (a->K != 1 && a->K != 4 && a->K != 9 && a->K != 16 && a->K != 25)
        return fail(SPF_E_INVALID, "%s: K must be one of 1, 4, 9, 16, 25 (got %d)", what, a->K);
    const int64_t lim = ((int64_t)1 << 31) - 1;
    if (a->hw > lim / ((int64_t)a->b * (8 + 3 * a->K)) || a->hw > lim / ((int64_t)a->b * a->v * 3 * a->K))
        return fail(SPF_E_INVALID, "%s: b hw (8 + 3K) and b v hw 3K must stay below 2^31 (got b = %d, v = %d, hw = %lld, K = %d)",
                    what, a->b, a->v, (long long)a->hw, a->K);
    if (!(a->exponent > 0.f) || !(a->exponent < 3.0e38f)) return fail(SPF_E_INVALID, "%s: exponent must be positive and finite", what);
    if (!a->sh_mask) return fail(SPF_E_INVALID, "%s: null pointer (sh_mask)", what);
    for (int i = 0; i < a->v; ++i) {
        if (!a->raw[i] || (need_pts && !a->pts[i])) return fail(SPF_E_INVALID, "%s: null pointer (raw or pts of view %d)", what, i);
        if (!aligned<16>({a->raw[i], a->pts[i]})) return fail(SPF_E_INVALID, "%s: tensors must be 16-byte aligned (view %d)", what, i);
    }
    return SPF_OK;
}

int spf_tail_forward(const SpfTail* a, float* means, float* opacities, float* scales, float* rotations, float* harmonics,
                     float* harmonics_high, void* stream_) {
    if (const int rc = tail_check("tail_forward", a, true)) return rc;
    if (!means || !opacities || !scales || !rotations || !harmonics) return fail(SPF_E_INVALID, "tail_forward: null output pointer");
    if (harmonics_high && a->K != 25) return fail(SPF_E_INVALID, "tail_forward: the band-split layout is the 16 + 9 split of K = 25 (got K = %d)", a->K);
    if (!aligned<16>({means, opacities, scales, rotations, harmonics, harmonics_high, a->sh_mask}))
        return fail(SPF_E_INVALID, "tail_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_tail_fwd(*a, means, opacities, scales, rotations, harmonics, harmonics_high, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_tail_backward(const SpfTail* a, const float* dL_dmeans, const float* dL_dopacities, const float* dL_dscales,
                      const float* dL_drotations, const float* dL_dharmonics, const float* dL_dharmonics_high, int32_t split,
                      const SpfTailGrads* g, void* stream_) {
    if (const int rc = tail_check("tail_backward", a, false)) return rc;
    if (!g) return fail(SPF_E_INVALID, "tail_backward: grads is null");
    if (split && a->K != 25) return fail(SPF_E_INVALID, "tail_backward: the band-split layout is the 16 + 9 split of K = 25 (got K = %d)", a->K);
    if (!split && dL_dharmonics_high) return fail(SPF_E_INVALID, "tail_backward: dL_dharmonics_high without split");
    for (int i = 0; i < a->v; ++i) {
        if (!g->d_raw[i] || !g->d_pts[i]) return fail(SPF_E_INVALID, "tail_backward: null pointer (d_raw or d_pts of view %d)", i);
        if (!aligned<16>({g->d_raw[i], g->d_pts[i]})) return fail(SPF_E_INVALID, "tail_backward: tensors must be 16-byte aligned (view %d)", i);
    }
    if (!aligned<16>({dL_dmeans, dL_dopacities, dL_dscales, dL_drotations, dL_dharmonics, dL_dharmonics_high, a->sh_mask}))
        return fail(SPF_E_INVALID, "tail_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_tail_bwd(*a, *g, dL_dmeans, dL_dopacities, dL_dscales, dL_drotations, dL_dharmonics, dL_dharmonics_high,
                                 split ? 1 : 0, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int opacity_check(const char* what, const float* logits, int64_t stride, int64_t n, float exponent) {
    if (!logits) return fail(SPF_E_INVALID, "%s: null pointer (logits)", what);
    if (n < 0 || stride < 1 || (n > 0 && stride > (((int64_t)1 << 62) / n)))
        return fail(SPF_E_INVALID, "%s: n must be >= 0 and stride >= 1 (got n = %lld, stride = %lld)", what, (long long)n, (long long)stride);
    if (!(exponent > 0.f) || !(exponent < 3.0e38f)) return fail(SPF_E_INVALID, "%s: exponent must be positive and finite", what);
    return SPF_OK;
}

int spf_opacity_forward(const float* logits, int64_t stride, int64_t n, float exponent, float* opacities, void* stream_) {
    if (const int rc = opacity_check("opacity_forward", logits, stride, n, exponent)) return rc;
    if (!opacities) return fail(SPF_E_INVALID, "opacity_forward: null pointer (opacities)");
    if (!aligned<4>({logits, opacities})) return fail(SPF_E_INVALID, "opacity_forward: tensors must be 4-byte aligned");
    if (n == 0) return SPF_OK;
    SPF_HIP(spf::launch_opacity_fwd(logits, stride, n, exponent, opacities, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_opacity_backward(const float* logits, int64_t stride, int64_t n, float exponent, const float* dL_dopacities,
                         float* dL_dlogits, void* stream_) {
    if (const int rc = opacity_check("opacity_backward", logits, stride, n, exponent)) return rc;
    if (!dL_dopacities || !dL_dlogits) return fail(SPF_E_INVALID, "opacity_backward: null pointer (dL_dopacities or dL_dlogits)");
    if (!aligned<4>({logits, dL_dopacities, dL_dlogits})) return fail(SPF_E_INVALID, "opacity_backward: tensors must be 4-byte aligned");
    if (n == 0) return SPF_OK;
    SPF_HIP(spf::launch_opacity_bwd(logits, stride, n, exponent, dL_dopacities, dL_dlogits, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

// ---- the pose heads (posehead.hip) ---------------------------------------------------------------------------------------
static bool pose_rows_ok(int64_t inner, int64_t stride, int64_t outer_stride, int64_t unit) {
    return inner >= 1 && stride >= 0 && outer_stride >= 0 && stride % unit == 0 && outer_stride % unit == 0;
}

static int pose_pool_check(const char* what, const SpfPosePool* a, int sources) {
    if (!a) return fail(SPF_E_INVALID, "%s: args is null", what);
    if (a->rows < 1 || a->rows > SPF_POSEHEAD_MAX_ROWS || a->L < 1 || a->L > (1 << 20))
        return fail(SPF_E_INVALID, "%s: rows must be 1 .. %d and L 1 .. 2^20 (got %lld, %d)", what, SPF_POSEHEAD_MAX_ROWS,
                    (long long)a->rows, a->L);
    for (int s = 0; s < sources; ++s) {
        if (a->C[s] < 4 || a->C[s] > (1 << 20) || a->C[s] % 4 != 0)
            return fail(SPF_E_INVALID, "%s: the width of source %d must be a multiple of 4 in 4 .. 2^20 (got %d)", what, s, a->C[s]);
    }
    return SPF_OK;
}

int spf_posehead_pool_forward(const SpfPosePool* a, float* feat, void* stream_) {
    const int sources = a && a->src[1] ? 2 : 1;
    if (const int rc = pose_pool_check("posehead_pool_forward", a, sources)) return rc;
    if (!a->src[0] || !feat) return fail(SPF_E_INVALID, "posehead_pool_forward: null pointer (src[0] or feat)");
    for (int s = 0; s < sources; ++s)
        if (!pose_rows_ok(a->inner[s], a->stride[s], a->outer_stride[s], 4) || a->tok_stride[s] < 0 || a->tok_stride[s] % 4 != 0)
            return fail(SPF_E_INVALID, "posehead_pool_forward: inner must be >= 1 and every stride a non-negative multiple of 4 floats (source %d)", s);
    if (!aligned<16>({a->src[0], a->src[1], feat})) return fail(SPF_E_INVALID, "posehead_pool_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_posehead_pool_fwd(*a, feat, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_pool_backward(const SpfPosePool* a, const float* d_feat, float* d_src0, float* d_src1, void* stream_) {
    if (const int rc = pose_pool_check("posehead_pool_backward", a, d_src1 ? 2 : 1)) return rc;
    if (!d_feat || !d_src0) return fail(SPF_E_INVALID, "posehead_pool_backward: null pointer (d_feat or d_src0)");
    if (!aligned<16>({d_feat, d_src0, d_src1})) return fail(SPF_E_INVALID, "posehead_pool_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_posehead_pool_bwd(*a, d_feat, d_src0, d_src1, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int pose_encode_check(const char* what, const SpfPoseEncode* a) {
    if (!a) return fail(SPF_E_INVALID, "%s: args is null", what);
    if (a->rows < 1 || a->rows > (1 << 24)) return fail(SPF_E_INVALID, "%s: rows must be 1 .. 2^24 (got %lld)", what, (long long)a->rows);
    if (!pose_rows_ok(a->out_inner, a->out_stride, a->out_outer_stride, 1))
        return fail(SPF_E_INVALID, "%s: out_inner must be >= 1 and the strides non-negative", what);
    if (a->homogeneous && (!(a->beta > 0.f) || !(a->max_inv_scale > 0.f) || !(a->min_inv_scale >= a->max_inv_scale) || !(a->min_inv_scale < 3.0e38f) || !(a->beta < 3.0e38f)))
        return fail(SPF_E_INVALID, "%s: beta and max_inv_scale must be positive and finite, min_inv_scale finite and not below max_inv_scale", what);
    return SPF_OK;
}

int spf_posehead_encode_forward(const SpfPoseEncode* a, const float* rot, const float* t, float* out, void* stream_) {
    if (const int rc = pose_encode_check("posehead_encode_forward", a)) return rc;
    if (!rot || !t || !out) return fail(SPF_E_INVALID, "posehead_encode_forward: null pointer (rot, t or out)");
    if (!aligned<4>({rot, t, out})) return fail(SPF_E_INVALID, "posehead_encode_forward: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_posehead_encode_fwd(*a, rot, t, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_encode_backward(const SpfPoseEncode* a, const float* t, const float* d_out, float* d_rot, float* d_t,
                                 void* stream_) {
    if (const int rc = pose_encode_check("posehead_encode_backward", a)) return rc;
    if ((a->homogeneous && !t) || !d_out || !d_rot || !d_t) return fail(SPF_E_INVALID, "posehead_encode_backward: null pointer (t, d_out, d_rot or d_t)");
    if (!aligned<4>({t, d_out, d_rot, d_t})) return fail(SPF_E_INVALID, "posehead_encode_backward: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_posehead_encode_bwd(*a, t, d_out, d_rot, d_t, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int pose_embed_check(const char* what, int64_t rows, int32_t C) {
    if (rows < 1 || rows > SPF_POSEHEAD_MAX_ROWS || C < 1 || C > (1 << 20))
        return fail(SPF_E_INVALID, "%s: rows must be 1 .. %d and C 1 .. 2^20 (got %lld, %d)", what, SPF_POSEHEAD_MAX_ROWS, (long long)rows, C);
    return SPF_OK;
}

int spf_posehead_embed_silu_forward(const float* p, int32_t broadcast, const float* W, const float* b, int64_t rows,
                                    int32_t C, float* out, void* stream_) {
    if (const int rc = pose_embed_check("posehead_embed_silu_forward", rows, C)) return rc;
    if (!p || !W || !b || !out) return fail(SPF_E_INVALID, "posehead_embed_silu_forward: null pointer (p, W, b or out)");
    if (!aligned<4>({p, W, b, out})) return fail(SPF_E_INVALID, "posehead_embed_silu_forward: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_posehead_embed_fwd(p, broadcast != 0, W, b, rows, C, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_embed_silu_backward(const float* p, int32_t broadcast, const float* W, const float* b, const float* dout,
                                     int64_t rows, int32_t C, float* dW, float* db, float* dp, void* stream_) {
    if (const int rc = pose_embed_check("posehead_embed_silu_backward", rows, C)) return rc;
    if (!p || !W || !b || !dout || !dW || !db) return fail(SPF_E_INVALID, "posehead_embed_silu_backward: null pointer (p, W, b, dout, dW or db)");
    if (!aligned<4>({p, W, b, dout, dW, db, dp})) return fail(SPF_E_INVALID, "posehead_embed_silu_backward: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_posehead_embed_bwd(p, broadcast != 0, W, b, dout, rows, C, dW, db, dp, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_modulate_forward(const float* x, const float* mod, int64_t rows, int32_t C, float eps, float* out,
                                  void* stream_) {
    if (!block_sizes_ok(rows, C)) return block_sizes_fail("posehead_modulate_forward", rows, C);
    if (!(eps >= 0.f) || !(eps < 3.0e38f)) return fail(SPF_E_INVALID, "posehead_modulate_forward: eps must be finite and not negative");
    if (!x || !mod || !out) return fail(SPF_E_INVALID, "posehead_modulate_forward: null pointer (x, mod or out)");
    if (!aligned<16>({x, mod, out})) return fail(SPF_E_INVALID, "posehead_modulate_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_posehead_modulate_fwd(x, mod, rows, C, eps, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_modulate_backward(const float* x, const float* mod, const float* dout, int64_t rows, int32_t C, float eps,
                                   float* dx, float* dmod, void* stream_) {
    if (!block_sizes_ok(rows, C)) return block_sizes_fail("posehead_modulate_backward", rows, C);
    if (!(eps >= 0.f) || !(eps < 3.0e38f)) return fail(SPF_E_INVALID, "posehead_modulate_backward: eps must be finite and not negative");
    if (!x || !mod || !dout || !dx || !dmod) return fail(SPF_E_INVALID, "posehead_modulate_backward: null pointer");
    if (!aligned<16>({x, mod, dout, dx, dmod})) return fail(SPF_E_INVALID, "posehead_modulate_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_posehead_modulate_bwd(x, mod, dout, rows, C, eps, dx, dmod, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int pose_attn_check(const char* what, int32_t B, int32_t S, int32_t H, int32_t D) {
    if (D != 64 && D != 128) return fail(SPF_E_INVALID, "%s: the head dim must be 64 or 128 (got %d)", what, D);
    if (S < 1 || S > SPF_POSEHEAD_MAX_S) return fail(SPF_E_INVALID, "%s: S must be 1 .. %d (got %d)", what, SPF_POSEHEAD_MAX_S, S);
    if (B < 1 || H < 1 || (int64_t)B * H > ((int64_t)1 << 31) / 3 - 1)
        return fail(SPF_E_INVALID, "%s: B and H must be positive and B H below 2^31 / 3 (got %d, %d)", what, B, H);
    return SPF_OK;
}

int spf_posehead_attn_forward(const float* qkv, int32_t B, int32_t S, int32_t H, int32_t D, float* out, void* stream_) {
    if (const int rc = pose_attn_check("posehead_attn_forward", B, S, H, D)) return rc;
    if (!qkv || !out) return fail(SPF_E_INVALID, "posehead_attn_forward: null pointer (qkv or out)");
    if (!aligned<16>({qkv, out})) return fail(SPF_E_INVALID, "posehead_attn_forward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_posehead_attn_fwd(qkv, B, S, H, D, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_attn_backward(const float* qkv, const float* dout, int32_t B, int32_t S, int32_t H, int32_t D, float* dqkv,
                               void* stream_) {
    if (const int rc = pose_attn_check("posehead_attn_backward", B, S, H, D)) return rc;
    if (!qkv || !dout || !dqkv) return fail(SPF_E_INVALID, "posehead_attn_backward: null pointer (qkv, dout or dqkv)");
    if (!aligned<16>({qkv, dout, dqkv})) return fail(SPF_E_INVALID, "posehead_attn_backward: tensors must be 16-byte aligned");
    SPF_HIP(spf::launch_posehead_attn_bwd(qkv, dout, B, S, H, D, dqkv, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

static int pose_act_check(const char* what, int64_t rows, int32_t trans_act, int32_t quat_act, int32_t fl_act) {
    if (rows < 1 || rows > (1 << 24)) return fail(SPF_E_INVALID, "%s: rows must be 1 .. 2^24 (got %lld)", what, (long long)rows);
    for (const int32_t act : {trans_act, quat_act, fl_act})
        if (act < SPF_POSE_ACT_LINEAR || act > SPF_POSE_ACT_RELU)
            return fail(SPF_E_INVALID, "%s: unknown activation %d (SPF_POSE_ACT_*)", what, act);
    return SPF_OK;
}

int spf_posehead_activate_forward(const float* prev, const float* delta, int64_t rows, int32_t trans_act, int32_t quat_act,
                                  int32_t fl_act, float* pred, float* out, void* stream_) {
    if (const int rc = pose_act_check("posehead_activate_forward", rows, trans_act, quat_act, fl_act)) return rc;
    if (!delta || !pred || !out) return fail(SPF_E_INVALID, "posehead_activate_forward: null pointer (delta, pred or out)");
    if (!aligned<4>({prev, delta, pred, out})) return fail(SPF_E_INVALID, "posehead_activate_forward: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_posehead_activate_fwd(prev, delta, rows, trans_act, quat_act, fl_act, pred, out, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_posehead_activate_backward(const float* pred, const float* d_pred, const float* d_out, int64_t rows,
                                   int32_t trans_act, int32_t quat_act, int32_t fl_act, float* d_delta, void* stream_) {
    if (const int rc = pose_act_check("posehead_activate_backward", rows, trans_act, quat_act, fl_act)) return rc;
    if (!pred || !d_delta || (!d_pred && !d_out)) return fail(SPF_E_INVALID, "posehead_activate_backward: null pointer (pred, d_delta, or both gradients)");
    if (!aligned<4>({pred, d_pred, d_out, d_delta})) return fail(SPF_E_INVALID, "posehead_activate_backward: tensors must be 4-byte aligned");
    SPF_HIP(spf::launch_posehead_activate_bwd(pred, d_pred, d_out, rows, trans_act, quat_act, fl_act, d_delta, static_cast<hipStream_t>(stream_)));
    return SPF_OK;
}

int spf_stage_timing_enable(int32_t mask) {
    g_timing = (uint32_t)mask;
    if (g_timing)
        for (int s = 0; s < SPF_STAGE_COUNT; ++s) g_log[s].used = 0;
    return SPF_OK;
}

int spf_stage_timing_sample_every(int32_t n) {
    if (n < 1) return fail(SPF_E_INVALID, "sample stride must be >= 1 (got %d)", n);
    g_sample_every = n;
    for (int s = 0; s < SPF_STAGE_COUNT; ++s) g_calls[s] = 0;
    return SPF_OK;
}

int spf_stage_times_ms(float* total_ms, int32_t* count) {
    if (!total_ms || !count) return fail(SPF_E_INVALID, "null output");
    for (int s = 0; s < SPF_STAGE_COUNT; ++s) {
        total_ms[s] = 0.f;
        count[s] = g_log[s].used;
        for (int i = 0; i < g_log[s].used; ++i) {
            SPF_HIP(hipEventSynchronize(g_log[s].ev[i][1]));
            float ms = 0.f;
            SPF_HIP(hipEventElapsedTime(&ms, g_log[s].ev[i][0], g_log[s].ev[i][1]));
            total_ms[s] += ms;
        }
    }
    return SPF_OK;
}

const char* spf_stage_kernel_name(int32_t stage) {
    return (stage >= 0 && stage < SPF_STAGE_COUNT) ? kStageKernel[stage] : "";
}

}  // extern "C"
