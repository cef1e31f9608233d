// SSIM (value and gradients) and PSNR for batches of images, fused for gfx950.
//
// The reference has the same arithmetic twice: `ssim` / `SSIM` (src/loss/loss_ssim.py:58-189), ten grouped
// convolutions and ~twenty elementwise kernels forward and as many backward in eager PyTorch, and `compute_ssim`
// (src/evaluation/metrics.py:36-52), a per-image device -> host copy and a scikit-image filter on one CPU core.  skimage's
// Gaussian-weighted SSIM averages exactly the VALID convolution that `_ssim` computes, with the (co)variances scaled by
// cov_norm = 121/120; one set of kernels with a cov_norm argument serves both.
//
// For X, Y [N,C,H,W] (every H x W plane on its own), a 1-D window w of odd length ws and h = ws - 1:
//   spf_ssim_fwd_kernel      one block per (tile of TX x TY outputs, plane) slot, grid-stride.  The (TY+h) x (TX+h) input
//                            tile of X and of Y is staged in LDS once; a horizontal pass leaves the five row moments
//                            (x, y, xx, yy, xy) in LDS, a vertical pass takes them to registers (four rows of a column
//                            per lane when the window length is the compiled-in 11), forms S and sums it.
//                            Neither the moment maps nor the S map ever reach HBM.  One float partial per slot.
//   spf_ssim_plane_kernel    one block per plane: its tiles' partials in a fixed order (float64) -> the plane's mean
//   spf_ssim_finalize_kernel one block: relu per plane, mean over channels -> [N], or over everything -> scalar
//   spf_ssim_bwd_kernel      design "recompute": one block per (tile of TX x TY INPUT pixels, plane).  Inputs with a
//                            2h halo -> row moments -> the derivative maps b = dS/dE[xx] (= dS/dE[yy]), c = dS/dE[xy],
//                            aX = dS/dmu_x, aY = dS/dmu_y (total derivatives, zero outside the valid region) on the tile
//                            plus an h halo -> transposed filter, rows then columns ->
//                            dL/dX = gs (W'aX + 2 X W'b + Y W'c), dL/dY = gs (W'aY + 2 Y W'b + X W'c),
//                            gs = upstream gradient of the plane's mean / n_valid, read on the device.
//                            Reads X, Y, writes the gradients; no state is kept between forward and backward.
//   spf_psnr_kernel          one block per image: mean((clip(gt) - clip(pred))^2) in a fixed order (float64), -10 log10
// No atomics: every result is run-to-run identical, and a plane's numbers do not depend on its neighbours in the batch.
//
// LDS access: in every pass consecutive lanes take consecutive columns of one row (the column index is the fast one),
// so the row pass reads and the column pass reads are both stride-1 across a wave: conflict-free (MI355X: 64 banks of
// 4 bytes, ds_read_b32 serviced in two 32-lane groups).
#include "point_slots.h"
#include "launchers.h"

namespace spf {

constexpr int kSsimHead = 40;              // floats ahead of the tiles in LDS: the window (33) and the four wave sums
constexpr size_t kLdsDefault = 64 * 1024;  // dynamic LDS a kernel gets without asking
constexpr size_t kLdsMax = 152 * 1024;     // what one workgroup may ask for (160 KiB per CU on gfx950)

struct SsimTiling {
    int tx, ty, ntx, nty;
    size_t lds;                            // bytes of dynamic LDS
};

static size_t ssim_fwd_lds(int tx, int ty, int ws) {
    const size_t ri = ty + ws - 1, ci = tx + ws - 1;
    return sizeof(float) * (kSsimHead + 2 * ri * ci + 5 * ri * tx);
}
// region A: the inputs (2 maps, 2h halo), later the derivative maps (2 + GX + GY maps, h halo); region B: the row moments
// (5 maps), later the row-filtered derivative maps
static size_t ssim_bwd_lds(int tx, int ty, int ws, int nmaps) {
    const size_t h = ws - 1, ri = ty + 2 * h, ci = tx + 2 * h, rd = ty + h, cd = tx + h;
    const size_t a = 2 * ri * ci > nmaps * rd * cd ? 2 * ri * ci : nmaps * rd * cd;
    return sizeof(float) * (kSsimHead + a + 5 * ri * cd);
}

// Forward: tiles over the valid region (H - h) x (W - h).  32 x 32 outputs unless the window is so long that the tile
// and its row moments pass 64 KiB; 32 x 16 always fits (ws = 33: 55 KiB).
SsimTiling ssim_fwd_tiling(int H, int W, int ws) {
    SsimTiling t;
    t.tx = 32;
    t.ty = ssim_fwd_lds(32, 32, ws) <= kLdsDefault ? 32 : 16;
    t.lds = ssim_fwd_lds(t.tx, t.ty, ws);
    t.ntx = (W - ws + 1 + t.tx - 1) / t.tx;
    t.nty = (H - ws + 1 + t.ty - 1) / t.ty;
    return t;
}
// Backward: tiles over the H x W input pixels.  The largest tile that fits 64 KiB (32 x 16 up to ws = 15, with four
// maps); longer windows take 16 x 16 or 8 x 8 inside the 160 KiB a workgroup may ask for.
SsimTiling ssim_bwd_tiling(int H, int W, int ws, int nmaps) {
    static const int cand[][2] = {{32, 16}, {16, 16}, {16, 8}, {8, 8}};
    SsimTiling t;
    t.tx = 0;
    for (int pass = 0; pass < 2 && !t.tx; ++pass)
        for (const auto& c : cand)
            if (ssim_bwd_lds(c[0], c[1], ws, nmaps) <= (pass ? kLdsMax : kLdsDefault)) {
                t.tx = c[0];
                t.ty = c[1];
                break;
            }
    t.lds = ssim_bwd_lds(t.tx, t.ty, ws, nmaps);   // (8 x 8 at ws = 33: 97 KiB, so a tile is always found)
    t.ntx = (W + t.tx - 1) / t.tx;
    t.nty = (H + t.ty - 1) / t.ty;
    return t;
}

int64_t ssim_slots(int N, int C, int H, int W, int ws) {
    const SsimTiling t = ssim_fwd_tiling(H, W, ws);
    return (int64_t)N * C * t.ntx * t.nty;
}

// One valid position from its five moments.
struct SsimPt {
    float L, CS, B1, B2;      // luminance and contrast-structure quotients and their denominators
};
__device__ __forceinline__ SsimPt ssim_point(float mx, float my, float exx, float eyy, float exy, float C1, float C2,
                                             float cn) {
    const float sx = cn * (exx - mx * mx), sy = cn * (eyy - my * my), sxy = cn * (exy - mx * my);
    SsimPt p;
    p.B1 = mx * mx + my * my + C1;
    p.B2 = sx + sy + C2;
    p.L = (2.f * mx * my + C1) / p.B1;
    p.CS = (2.f * sxy + C2) / p.B2;
    return p;
}

__device__ __forceinline__ void ssim_load_window(const SpfSsim& a, int ws, float* __restrict__ s_win) {
    if ((int)threadIdx.x < ws) s_win[threadIdx.x] = a.win[threadIdx.x];
}

// A lane's walk over the items of a (rows x cols) map, kBlock items per step, as (row, column): one integer division
// where the walk starts and an add, a compare and a select per step (a division by a run-time `cols` costs ~25
// instructions, as much as the arithmetic of an item).
struct SsimWalk {
    int r, c, dq, dr, cols;
    __device__ __forceinline__ SsimWalk(int cols_) : cols(cols_) {
        r = (int)threadIdx.x / cols;
        c = (int)threadIdx.x - r * cols;
        dq = kBlock / cols;
        dr = kBlock - dq * cols;
    }
    __device__ __forceinline__ void step() {
        r += dq;
        c += dr;
        if (c >= cols) {
            c -= cols;
            ++r;
        }
    }
};

// rows x cols floats of the planes X and Y (H x W) starting at (y0, x0) into LDS; zero outside the plane.  Four
// entries of each plane per lane and trip, all eight loads issued before the first is stored: with three or four
// blocks per CU it is the loads in flight per lane, not the lanes, that hide the memory latency.
__device__ __forceinline__ void ssim_stage(const float* __restrict__ X, const float* __restrict__ Y, int H, int W,
                                           int y0, int x0, int rows, int cols, float* __restrict__ dx,
                                           float* __restrict__ dy) {
    const int n = rows * cols;
    SsimWalk w(cols);
    for (int i0 = threadIdx.x; i0 < n; i0 += 4 * kBlock) {
        float vx[4], vy[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int y = y0 + w.r, x = x0 + w.c;
            const bool in = i0 + u * kBlock < n && y >= 0 && y < H && x >= 0 && x < W;
            const int64_t o = in ? (int64_t)y * W + x : 0;
            vx[u] = in ? X[o] : 0.f;
            vy[u] = in ? Y[o] : 0.f;
            w.step();
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * kBlock;
            if (i < n) {
                dx[i] = vx[u];
                dy[i] = vy[u];
            }
        }
    }
}

// Row pass: the five moments of sx, sy (rows x cin, cin = cout + ws - 1) along x into mom[5][rows x cout].
template <int WS>
__device__ __forceinline__ void ssim_row_moments(const float* __restrict__ sx, const float* __restrict__ sy,
                                                 const float* __restrict__ s_win, int ws, int rows, int cin, int cout,
                                                 float* __restrict__ mom) {
    const int n = rows * cout;
    SsimWalk at(cout);
    for (int i = threadIdx.x; i < n; i += kBlock, at.step()) {
        const float* __restrict__ px = sx + at.r * cin + at.c;
        const float* __restrict__ py = sy + at.r * cin + at.c;
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
#pragma unroll
        for (int k = 0; k < (WS ? WS : ws); ++k) {
            const float w = s_win[k], x = px[k], y = py[k];
            const float wx = w * x, wy = w * y;
            mx += wx;
            my += wy;
            xx = fmaf(wx, x, xx);
            yy = fmaf(wy, y, yy);
            xy = fmaf(wx, y, xy);
        }
        mom[i] = mx;
        mom[n + i] = my;
        mom[2 * n + i] = xx;
        mom[3 * n + i] = yy;
        mom[4 * n + i] = xy;
    }
}

// Column pass at (r, c): the five moments from mom[5][rows x cols] (rows r .. r + ws - 1 of column c).
template <int WS>
__device__ __forceinline__ void ssim_col_moments(const float* __restrict__ mom, const float* __restrict__ s_win, int ws,
                                                 int n, int cols, int r, int c, float (&m)[5]) {
#pragma unroll
    for (int j = 0; j < 5; ++j) m[j] = 0.f;
    const float* __restrict__ p = mom + r * cols + c;
#pragma unroll
    for (int k = 0; k < (WS ? WS : ws); ++k) {
        const float w = s_win[k];
#pragma unroll
        for (int j = 0; j < 5; ++j) m[j] = fmaf(w, p[j * n + k * cols], m[j]);
    }
}

// The same for RB rows r0 .. r0 + RB - 1 of column c at once (window length known at compile time): the rows share
// their reads, WS + RB - 1 per map instead of RB x WS, and every output adds its terms in the order of the single-row
// form: the same bits.  Reads rows up to r0 + RB + WS - 2 of `mom`.
template <int WS, int RB>
__device__ __forceinline__ void ssim_col_moments_rows(const float* __restrict__ mom, const float* __restrict__ s_win,
                                                      int n, int cols, int r0, int c, float (&m)[RB][5]) {
    float w[WS];
#pragma unroll
    for (int k = 0; k < WS; ++k) w[k] = s_win[k];
#pragma unroll
    for (int o = 0; o < RB; ++o)
#pragma unroll
        for (int j = 0; j < 5; ++j) m[o][j] = 0.f;
    const float* __restrict__ p = mom + r0 * cols + c;
#pragma unroll
    for (int k = 0; k < WS + RB - 1; ++k) {
        float v[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) v[j] = p[j * n + k * cols];
#pragma unroll
        for (int o = 0; o < RB; ++o)
            if (k - o >= 0 && k - o < WS) {
#pragma unroll
                for (int j = 0; j < 5; ++j) m[o][j] = fmaf(w[k - o], v[j], m[o][j]);
            }
    }
}

template <int WS>
__global__ __launch_bounds__(kBlock) void spf_ssim_fwd_kernel(SpfSsim a, int TX, int TY, int ntx, int nty,
                                                              int64_t nslots, float* __restrict__ partial) {
    extern __shared__ float s_mem[];
    const int ws = WS ? WS : a.ws, h = ws - 1;
    const int RI = TY + h, CI = TX + h, Hv = a.H - h, Wv = a.W - h;
    float* s_win = s_mem;
    SumRow<1>& s_sum = *reinterpret_cast<SumRow<1>*>(s_mem + 36);
    float* s_x = s_mem + kSsimHead;
    float* s_y = s_x + RI * CI;
    float* s_m = s_y + RI * CI;
    ssim_load_window(a, ws, s_win);
    const int ntiles = ntx * nty, nrow = RI * TX;
    const int64_t plane_elems = (int64_t)a.H * a.W;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int64_t plane = slot / ntiles;
        const int tile = (int)(slot - plane * ntiles);
        const int ty = tile / ntx, tx = tile - ty * ntx;
        const int y0 = ty * TY, x0 = tx * TX;
        __syncthreads();                                   // the previous slot's readers are done (and s_win is written)
        ssim_stage(a.X + plane * plane_elems, a.Y + plane * plane_elems, a.H, a.W, y0, x0, RI, CI, s_x, s_y);
        __syncthreads();
        ssim_row_moments<WS>(s_x, s_y, s_win, ws, RI, CI, TX, s_m);
        __syncthreads();
        float acc = 0.f;
        if constexpr (WS != 0) {                           // four rows of a column per lane (TY is a multiple of four)
            constexpr int RB = 4;
            SsimWalk at(TX);
            for (int i = threadIdx.x; i < (TY / RB) * TX; i += kBlock, at.step()) {
                const int c = at.c, r0 = at.r * RB;
                if (y0 + r0 < Hv && x0 + c < Wv) {
                    float m[RB][5];
                    ssim_col_moments_rows<WS, RB>(s_m, s_win, nrow, TX, r0, c, m);
#pragma unroll
                    for (int o = 0; o < RB; ++o)
                        if (y0 + r0 + o < Hv) {
                            const SsimPt p = ssim_point(m[o][0], m[o][1], m[o][2], m[o][3], m[o][4], a.C1, a.C2,
                                                        a.cov_norm);
                            acc += p.L * p.CS;
                        }
                }
            }
        } else {
            SsimWalk at(TX);
            for (int i = threadIdx.x; i < TY * TX; i += kBlock, at.step()) {
                const int r = at.r, c = at.c;
                if (y0 + r < Hv && x0 + c < Wv) {
                    float m[5];
                    ssim_col_moments<WS>(s_m, s_win, ws, nrow, TX, r, c, m);
                    const SsimPt p = ssim_point(m[0], m[1], m[2], m[3], m[4], a.C1, a.C2, a.cov_norm);
                    acc += p.L * p.CS;
                }
            }
        }
        const float tot = block_sum(acc, s_sum);
        if (threadIdx.x == 0) partial[slot] = tot;
    }
}

__global__ __launch_bounds__(kBlock) void spf_ssim_plane_kernel(const float* __restrict__ partial, int ntiles,
                                                                double inv_valid, float* __restrict__ plane_mean) {
    __shared__ double s_d[kBlock];
    const float* __restrict__ p = partial + (int64_t)blockIdx.x * ntiles;
    double acc = 0.0;
    for (int t = threadIdx.x; t < ntiles; t += kBlock) acc += (double)p[t];
    const double tot = block_tree_sum<kBlock>(acc, s_d);
    if (threadIdx.x == 0) plane_mean[blockIdx.x] = (float)(tot * inv_valid);
}

// relu(NaN) stays NaN, as torch.relu
__device__ __forceinline__ float ssim_relu(float v, int nonneg) { return (nonneg && v < 0.f) ? 0.f : v; }

__global__ __launch_bounds__(kBlock) void spf_ssim_finalize_kernel(const float* __restrict__ plane_mean, int N, int C,
                                                                   int size_average, int nonneg,
                                                                   float* __restrict__ out) {
    __shared__ double s_d[kBlock];
    if (!size_average) {                                   // out[n]: the image's channels in order
        for (int n = threadIdx.x; n < N; n += kBlock) {
            double acc = 0.0;
            for (int c = 0; c < C; ++c) acc += (double)ssim_relu(plane_mean[(int64_t)n * C + c], nonneg);
            out[n] = (float)(acc / (double)C);
        }
        return;
    }
    const int64_t np = (int64_t)N * C;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < np; i += kBlock) acc += (double)ssim_relu(plane_mean[i], nonneg);
    const double tot = block_tree_sum<kBlock>(acc, s_d);
    if (threadIdx.x == 0) out[0] = (float)(tot / (double)np);
}

// Derivative maps in LDS: [b, c, aX (GX), aY (GY)].
template <int WS, bool GX, bool GY>
__global__ __launch_bounds__(kBlock) void spf_ssim_bwd_kernel(SpfSsim a, int TX, int TY, int ntx, int nty,
                                                              int64_t nslots, const float* __restrict__ plane_mean,
                                                              const float* __restrict__ dL_dout,
                                                              float* __restrict__ dX, float* __restrict__ dY) {
    constexpr int NM = 2 + (GX ? 1 : 0) + (GY ? 1 : 0);
    constexpr int MAX = 2, MAY = GX ? 3 : 2;
    extern __shared__ float s_mem[];
    const int ws = WS ? WS : a.ws, h = ws - 1;
    const int RI = TY + 2 * h, CI = TX + 2 * h, RD = TY + h, CD = TX + h, Hv = a.H - h, Wv = a.W - h;
    const int nin = 2 * RI * CI, nder = NM * RD * CD;
    float* s_win = s_mem;
    float* s_a = s_mem + kSsimHead;                        // inputs, then the derivative maps
    float* s_b = s_a + (nin > nder ? nin : nder);          // row moments, then the row-filtered derivative maps
    ssim_load_window(a, ws, s_win);
    const int ntiles = ntx * nty;
    const int64_t plane_elems = (int64_t)a.H * a.W;
    const float inv_valid = 1.f / ((float)Hv * (float)Wv);
    const float inv_count = a.size_average ? 1.f / ((float)a.N * (float)a.C) : 1.f / (float)a.C;
    for (int64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const int64_t plane = slot / ntiles;
        const int tile = (int)(slot - plane * ntiles);
        const int ty = tile / ntx, tx = tile - ty * ntx;
        const int y0 = ty * TY, x0 = tx * TX;
        const float* __restrict__ X = a.X + plane * plane_elems;
        const float* __restrict__ Y = a.Y + plane * plane_elems;
        // upstream gradient reaching this plane's mean: the batch / channel mean and the relu folded in
        const float pm = plane_mean[plane];
        const float up = dL_dout[a.size_average ? 0 : plane / a.C];
        const float gs = (a.nonnegative && !(pm > 0.f)) ? 0.f : up * inv_count * inv_valid;
        __syncthreads();
        ssim_stage(X, Y, a.H, a.W, y0 - h, x0 - h, RI, CI, s_a, s_a + RI * CI);
        __syncthreads();
        ssim_row_moments<WS>(s_a, s_a + RI * CI, s_win, ws, RI, CI, CD, s_b);
        __syncthreads();                                   // (the inputs in s_a are dead from here)
        const int nd = RD * CD;
        // entry i = (r, c) of the derivative maps from its moments; zero outside the valid region
        auto entry = [&](int i, int r, int c, const float (&m)[5]) {
            const int qy = y0 - h + r, qx = x0 - h + c;    // valid-region position of this entry
            float vb = 0.f, vc = 0.f, vax = 0.f, vay = 0.f;
            if (qy >= 0 && qy < Hv && qx >= 0 && qx < Wv) {
                const SsimPt p = ssim_point(m[0], m[1], m[2], m[3], m[4], a.C1, a.C2, a.cov_norm);
                const float S = p.L * p.CS;
                vb = -S * a.cov_norm / p.B2;
                vc = 2.f * a.cov_norm * p.L / p.B2;
                const float k = 2.f * p.CS / p.B1;
                if (GX) vax = k * (m[1] - p.L * m[0]) - 2.f * m[0] * vb - m[1] * vc;
                if (GY) vay = k * (m[0] - p.L * m[1]) - 2.f * m[1] * vb - m[0] * vc;
            }
            s_a[i] = vb;
            s_a[nd + i] = vc;
            if (GX) s_a[MAX * nd + i] = vax;
            if (GY) s_a[MAY * nd + i] = vay;
        };
        if constexpr (WS != 0) {                           // two rows of a column per lane (RD = TY + h is even)
            SsimWalk at(CD);
            for (int i = threadIdx.x; i < (RD / 2) * CD; i += kBlock, at.step()) {
                const int c = at.c, r0 = 2 * at.r;
                float m[2][5];
                ssim_col_moments_rows<WS, 2>(s_b, s_win, RI * CD, CD, r0, c, m);
                entry(r0 * CD + c, r0, c, m[0]);
                entry((r0 + 1) * CD + c, r0 + 1, c, m[1]);
            }
        } else {
            SsimWalk at(CD);
            for (int i = threadIdx.x; i < nd; i += kBlock, at.step()) {
                const int r = at.r, c = at.c;
                float m[5];
                ssim_col_moments<WS>(s_b, s_win, ws, RI * CD, CD, r, c, m);
                entry(i, r, c, m);
            }
        }
        __syncthreads();                                   // (the row moments in s_b are dead from here)
        // transposed filter along x: input column x0 + c collects entry column c + h - k with weight w[k]
        const int nh = RD * TX;
        SsimWalk ah(TX);
        for (int i = threadIdx.x; i < nh; i += kBlock, ah.step()) {
            const float* __restrict__ p = s_a + ah.r * CD + ah.c + h;
            float v[NM];
#pragma unroll
            for (int j = 0; j < NM; ++j) v[j] = 0.f;
#pragma unroll
            for (int k = 0; k < (WS ? WS : ws); ++k) {
                const float w = s_win[k];
#pragma unroll
                for (int j = 0; j < NM; ++j) v[j] = fmaf(w, p[j * nd - k], v[j]);
            }
#pragma unroll
            for (int j = 0; j < NM; ++j) s_b[j * nh + i] = v[j];
        }
        __syncthreads();
        // the same along y, then the gradients of this tile's pixels
        SsimWalk av(TX);
        for (int i = threadIdx.x; i < TY * TX; i += kBlock, av.step()) {
            const int r = av.r, c = av.c;
            const int py = y0 + r, px = x0 + c;
            if (py < a.H && px < a.W) {
                const float* __restrict__ p = s_b + (r + h) * TX + c;
                float v[NM];
#pragma unroll
                for (int j = 0; j < NM; ++j) v[j] = 0.f;
#pragma unroll
                for (int k = 0; k < (WS ? WS : ws); ++k) {
                    const float w = s_win[k];
#pragma unroll
                    for (int j = 0; j < NM; ++j) v[j] = fmaf(w, p[j * nh - k * TX], v[j]);
                }
                const int64_t o = (int64_t)py * a.W + px;
                const float x = X[o], y = Y[o];
                if (GX) dX[plane * plane_elems + o] = gs * (v[MAX] + 2.f * x * v[0] + y * v[1]);
                if (GY) dY[plane * plane_elems + o] = gs * (v[MAY] + 2.f * y * v[0] + x * v[1]);
            }
        }
    }
}

// One block per image: mse = mean((clip(gt, 0, 1) - clip(pred, 0, 1))^2) over n floats, psnr = -10 log10(mse)
// (+inf for identical images).  clip keeps NaN, as torch.clip.
__device__ __forceinline__ float psnr_clip(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
__global__ __launch_bounds__(kBlock) void spf_psnr_kernel(const float* __restrict__ gt, const float* __restrict__ pred,
                                                          int64_t n, float* __restrict__ psnr) {
    __shared__ double s_d[kBlock];
    const float* __restrict__ g = gt + (int64_t)blockIdx.x * n;
    const float* __restrict__ p = pred + (int64_t)blockIdx.x * n;
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kBlock) {
        const float d = psnr_clip(g[i]) - psnr_clip(p[i]);
        acc += (double)(d * d);
    }
    const double tot = block_tree_sum<kBlock>(acc, s_d);
    if (threadIdx.x == 0) psnr[blockIdx.x] = -10.f * log10f((float)(tot / (double)n));
}

template <typename K>
static hipError_t ssim_allow_lds(K kernel, size_t lds) {
    if (lds <= kLdsDefault) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds);
}

hipError_t launch_ssim_fwd(const SpfSsim& a, float* partial, float* plane_mean, float* out, hipStream_t stream) {
    const SsimTiling t = ssim_fwd_tiling(a.H, a.W, a.ws);
    const int ntiles = t.ntx * t.nty;
    const int64_t nslots = (int64_t)a.N * a.C * ntiles;
    if (a.ws == 11)
        spf_ssim_fwd_kernel<11><<<slot_grid(nslots), kBlock, t.lds, stream>>>(a, t.tx, t.ty, t.ntx, t.nty, nslots, partial);
    else
        spf_ssim_fwd_kernel<0><<<slot_grid(nslots), kBlock, t.lds, stream>>>(a, t.tx, t.ty, t.ntx, t.nty, nslots, partial);
    const double inv_valid = 1.0 / ((double)(a.H - a.ws + 1) * (double)(a.W - a.ws + 1));
    spf_ssim_plane_kernel<<<a.N * a.C, kBlock, 0, stream>>>(partial, ntiles, inv_valid, plane_mean);
    spf_ssim_finalize_kernel<<<1, kBlock, 0, stream>>>(plane_mean, a.N, a.C, a.size_average, a.nonnegative, out);
    return hipGetLastError();
}

template <int WS, bool GX, bool GY>
static hipError_t ssim_bwd_launch(const SpfSsim& a, const float* plane_mean, const float* dL_dout, float* dX, float* dY,
                                  hipStream_t stream) {
    const SsimTiling t = ssim_bwd_tiling(a.H, a.W, a.ws, 2 + (GX ? 1 : 0) + (GY ? 1 : 0));
    const int64_t nslots = (int64_t)a.N * a.C * t.ntx * t.nty;
    if (hipError_t e = ssim_allow_lds(spf_ssim_bwd_kernel<WS, GX, GY>, t.lds)) return e;
    spf_ssim_bwd_kernel<WS, GX, GY><<<slot_grid(nslots), kBlock, t.lds, stream>>>(a, t.tx, t.ty, t.ntx, t.nty, nslots,
                                                                                 plane_mean, dL_dout, dX, dY);
    return hipGetLastError();
}

template <int WS>
static hipError_t ssim_bwd_which(const SpfSsim& a, const float* plane_mean, const float* dL_dout, float* dX, float* dY,
                                 hipStream_t stream) {
    if (dX && dY) return ssim_bwd_launch<WS, true, true>(a, plane_mean, dL_dout, dX, dY, stream);
    if (dX) return ssim_bwd_launch<WS, true, false>(a, plane_mean, dL_dout, dX, nullptr, stream);
    return ssim_bwd_launch<WS, false, true>(a, plane_mean, dL_dout, nullptr, dY, stream);
}

hipError_t launch_ssim_bwd(const SpfSsim& a, const float* plane_mean, const float* dL_dout, float* dX, float* dY,
                           hipStream_t stream) {
    return a.ws == 11 ? ssim_bwd_which<11>(a, plane_mean, dL_dout, dX, dY, stream)
                      : ssim_bwd_which<0>(a, plane_mean, dL_dout, dX, dY, stream);
}

hipError_t launch_psnr(const float* gt, const float* pred, int N, int64_t n, float* psnr, hipStream_t stream) {
    spf_psnr_kernel<<<N, kBlock, 0, stream>>>(gt, pred, n, psnr);
    return hipGetLastError();
}

}  // namespace spf
