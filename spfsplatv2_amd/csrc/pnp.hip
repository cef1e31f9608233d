// PnP pose from point maps: P3P RANSAC and Gauss-Newton refinement, four launches for all views of a call
// (DESIGN.md 7s holds the definition; tests/pnp_oracle.py restates it in float64 and float32).
//
//   spf_pnp_mask_kernel        one block per view: a 64-bit candidate word per 64 pixels, the scanned counts, n
//   spf_pnp_hypotheses_kernel  one lane per (view, hypothesis): hash -> four ranks -> pixels -> P3P (float64) -> R | t
//   spf_pnp_score_kernel       (pixel chunk, view): every hypothesis against the lane's points, ballot + popcount
//   spf_pnp_refine_kernel      one block per view: arg-max, Gauss-Newton with re-selected inliers (float64), the pose
//
// Nothing here uses a float atomic, a device-scope fence or a host read: the counts are integer adds (order-free) and
// every float sum has a fixed order, so a call is bitwise reproducible and a view's result does not depend on its
// neighbours in the batch.
#include <math.h>

#include "launchers.h"
#include "spf_common.h"

namespace spf {
namespace {

constexpr int kPnpMaskBlock = 1024;
constexpr int kPnpScoreBlock = 256;
constexpr int kPnpScorePts = 4;          // points a lane keeps in registers
constexpr int kPnpRefineBlock = 1024;
constexpr int kPnpSums = 28;             // 21 (upper triangle of J^T J) + 6 (J^T r) + 1 (inliers)
constexpr int kPnpRedraws = 8;

struct PnpWs {
    uint64_t* words;      // [views][G]        candidate bits of 64 pixels
    uint32_t* prefix;     // [views][G + 1]    exclusive scan of the words' popcounts; [G] = n
    float* hyp;           // [views][iters][12] R (row-major) | t, world -> camera; hyp[0] = NaN marks a void one
    uint32_t* counts;     // [views][iters]
    int G;
};

__host__ __device__ inline int pnp_groups(int hw) { return (hw + 63) >> 6; }

inline PnpWs pnp_workspace(void* base, int views, int hw, int iters) {
    PnpWs ws;
    ws.G = pnp_groups(hw);
    char* p = static_cast<char*>(base);
    ws.words = reinterpret_cast<uint64_t*>(p);
    p += sizeof(uint64_t) * (size_t)views * ws.G;
    ws.prefix = reinterpret_cast<uint32_t*>(p);
    p += sizeof(uint32_t) * (size_t)views * (ws.G + 1);
    ws.hyp = reinterpret_cast<float*>(p);
    p += sizeof(float) * 12 * (size_t)views * iters;
    ws.counts = reinterpret_cast<uint32_t*>(p);
    return ws;
}

// lowbias32 (Chris Wellons, "hash-prospector"): the published two-multiply 32-bit mixer
__device__ __forceinline__ uint32_t pnp_mix(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
__device__ __forceinline__ uint32_t pnp_hash(uint32_t seed, uint32_t k, uint32_t draw) {
    return pnp_mix(pnp_mix(pnp_mix(seed + 0x9e3779b9u) ^ k) ^ draw);
}

// Pixel p of a view: its three floats, and whether it is a candidate (opacity > threshold, finite coordinates).
__device__ __forceinline__ bool pnp_load(const SpfPnp& a, int view, int p, float& x, float& y, float& z) {
    const int bi = view / a.v, vi = view - bi * a.v, i = p / a.w, j = p - i * a.w;
    const float* __restrict__ q = a.pts3d + bi * a.pts_stride[0] + vi * a.pts_stride[1] + i * a.pts_stride[2] + j * a.pts_stride[3];
    const float o = a.opacity[bi * a.opa_stride[0] + vi * a.opa_stride[1] + i * a.opa_stride[2] + j * a.opa_stride[3]];
    x = q[0]; y = q[1]; z = q[2];
    return o > a.opacity_threshold && isfinite(x) && isfinite(y) && isfinite(z);
}

// ---- candidates ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPnpMaskBlock) void spf_pnp_mask_kernel(const SpfPnp a, const PnpWs ws) {
    const int view = blockIdx.x, hw = a.h * a.w, G = ws.G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t* __restrict__ words = ws.words + (size_t)view * G;
    uint32_t* __restrict__ prefix = ws.prefix + (size_t)view * (G + 1);
    for (int g = wave; g < G; g += kPnpMaskBlock / 64) {
        const int p = g * 64 + lane;
        float x, y, z;
        const bool c = p < hw && pnp_load(a, view, p, x, y, z);
        const uint64_t m = lane_ballot(c);
        if (lane == 0) {
            words[g] = m;
            prefix[g] = (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    if (wave == 0) {                      // the scan: 64 groups a round, the carry in a scalar
        uint32_t carry = 0;
        for (int base = 0; base < G; base += 64) {
            const int g = base + lane;
            const uint32_t c = g < G ? prefix[g] : 0u;
            const uint32_t inc = wave_iscan_u32(c);
            if (g < G) prefix[g] = carry + inc - c;
            carry += (uint32_t)__shfl((int)inc, 63, 64);
        }
        if (lane == 0) prefix[G] = carry;
    }
}

// ---- P3P (Grunert's quartic), float64 --------------------------------------------------------------------------------
// Real roots of A4 x^4 + .. + A0 by Ferrari's resolvent cubic, each polished with two Newton steps; at most four.
__device__ int pnp_quartic(double A4, double A3, double A2, double A1, double A0, double* x) {
    if (!(fabs(A4) > 1e-14 * (fabs(A3) + fabs(A2) + fabs(A1) + fabs(A0)))) return 0;
    const double a = A3 / A4, b = A2 / A4, c = A1 / A4, d = A0 / A4;
    const double a2 = a * a;
    const double p = b - 0.375 * a2, q = c - 0.5 * a * b + 0.125 * a2 * a;
    const double r = d - 0.25 * a * c + 0.0625 * a2 * b - (3.0 / 256.0) * a2 * a2;
    // m^3 + p m^2 + (p^2 / 4 - r) m - q^2 / 8 = 0: its largest real root (>= 0)
    const double c2 = p, c1 = 0.25 * p * p - r, c0 = -0.125 * q * q;
    const double P = c1 - c2 * c2 / 3.0, Q = 2.0 * c2 * c2 * c2 / 27.0 - c2 * c1 / 3.0 + c0;
    const double disc = 0.25 * Q * Q + P * P * P / 27.0;
    double t;
    if (disc > 0.0) {
        const double sd = sqrt(disc);
        t = cbrt(-0.5 * Q + sd) + cbrt(-0.5 * Q - sd);
    } else {
        const double rho = sqrt(fmax(-P / 3.0, 0.0));
        const double den = rho * rho * rho;
        const double arg = den > 0.0 ? fmin(fmax(-0.5 * Q / den, -1.0), 1.0) : 1.0;
        t = 2.0 * rho * cos(acos(arg) / 3.0);
    }
    double m = t - c2 / 3.0;
    for (int i = 0; i < 2; ++i) {
        const double f = ((m + c2) * m + c1) * m + c0, fp = (3.0 * m + 2.0 * c2) * m + c1;
        if (fp != 0.0) m -= f / fp;
    }
    double y[4];
    int n = 0;
    if (!(m > 1e-14 * (fabs(p) + fabs(r) + 1.0))) {          // q = 0: a quadratic in y^2
        const double D = p * p - 4.0 * r;
        if (D >= 0.0) {
            const double sD = sqrt(D);
            const double z1 = 0.5 * (-p + sD), z2 = 0.5 * (-p - sD);
            if (z1 >= 0.0) { y[n++] = sqrt(z1); y[n++] = -sqrt(z1); }
            if (z2 >= 0.0) { y[n++] = sqrt(z2); y[n++] = -sqrt(z2); }
        }
    } else {
        const double s = sqrt(2.0 * m), h = 0.5 * p + m, e = q / (2.0 * s);
        const double D1 = s * s - 4.0 * (h + e), D2 = s * s - 4.0 * (h - e);
        if (D1 >= 0.0) { const double sD = sqrt(D1); y[n++] = 0.5 * (s + sD); y[n++] = 0.5 * (s - sD); }
        if (D2 >= 0.0) { const double sD = sqrt(D2); y[n++] = 0.5 * (-s + sD); y[n++] = 0.5 * (-s - sD); }
    }
    for (int i = 0; i < n; ++i) {
        double v = y[i] - 0.25 * a;
        for (int it = 0; it < 2; ++it) {
            const double f = (((v + a) * v + b) * v + c) * v + d, fp = ((4.0 * v + 3.0 * a) * v + 2.0 * b) * v + c;
            if (fp != 0.0) v -= f / fp;
        }
        x[i] = v;
    }
    return n;
}

struct PnpCam { double fx, sk, cx, fy, cy; };
__device__ __forceinline__ PnpCam pnp_camera(const SpfPnp& a, int view) {
    const float* __restrict__ K = a.K + 9 * (size_t)view;
    PnpCam c;
    c.fx = (double)K[0] * a.w; c.sk = (double)K[1] * a.w; c.cx = (double)K[2] * a.w;
    c.fy = (double)K[4] * a.h; c.cy = (double)K[5] * a.h;
    return c;
}

__device__ __forceinline__ void pnp_cross(const double* u, const double* v, double* o) {
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}
// e1 = normalize(B - A), e3 = normalize(e1 x (C - A)), e2 = e3 x e1
__device__ __forceinline__ void pnp_frame(const double* A, const double* B, const double* C, double (*e)[3]) {
    double d1[3], d2[3];
    for (int i = 0; i < 3; ++i) { d1[i] = B[i] - A[i]; d2[i] = C[i] - A[i]; }
    const double n1 = 1.0 / sqrt(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]);
    for (int i = 0; i < 3; ++i) e[0][i] = d1[i] * n1;
    pnp_cross(e[0], d2, e[2]);
    const double n3 = 1.0 / sqrt(e[2][0] * e[2][0] + e[2][1] * e[2][1] + e[2][2] * e[2][2]);
    for (int i = 0; i < 3; ++i) e[2][i] *= n3;
    pnp_cross(e[2], e[0], e[1]);
}

// P3P on points 0..2, the root chosen by point 3.  P [4][3] world points, px [4][2] pixels.  false: void.
__device__ bool pnp_p3p(const PnpCam& cam, const double (*Pw)[3], const double (*px)[2], double* R, double* t) {
    double f[3][3];
    for (int i = 0; i < 3; ++i) {
        const double Y = (px[i][1] - cam.cy) / cam.fy, X = (px[i][0] - cam.cx - cam.sk * Y) / cam.fx;
        const double inv = 1.0 / sqrt(X * X + Y * Y + 1.0);
        f[i][0] = X * inv; f[i][1] = Y * inv; f[i][2] = inv;
    }
    double a2 = 0, b2 = 0, c2 = 0, ca = 0, cb = 0, cg = 0;
    for (int i = 0; i < 3; ++i) {
        a2 += (Pw[1][i] - Pw[2][i]) * (Pw[1][i] - Pw[2][i]);
        b2 += (Pw[0][i] - Pw[2][i]) * (Pw[0][i] - Pw[2][i]);
        c2 += (Pw[0][i] - Pw[1][i]) * (Pw[0][i] - Pw[1][i]);
        ca += f[1][i] * f[2][i];
        cb += f[0][i] * f[2][i];
        cg += f[0][i] * f[1][i];
    }
    if (!(a2 > 0.0 && b2 > 0.0 && c2 > 0.0)) return false;
    const double q = (a2 - c2) / b2, p = (a2 + c2) / b2, cr = c2 / b2, ar = a2 / b2;
    const double A4 = (q - 1.0) * (q - 1.0) - 4.0 * cr * ca * ca;
    const double A3 = 4.0 * (q * (1.0 - q) * cb - (1.0 - p) * ca * cg + 2.0 * cr * ca * ca * cb);
    const double A2 = 2.0 * (q * q - 1.0 + 2.0 * q * q * cb * cb + 2.0 * (1.0 - cr) * ca * ca - 4.0 * p * ca * cb * cg +
                             2.0 * (1.0 - ar) * cg * cg);
    const double A1 = 4.0 * (-q * (1.0 + q) * cb + 2.0 * ar * cg * cg * cb - (1.0 - p) * ca * cg);
    const double A0 = (1.0 + q) * (1.0 + q) - 4.0 * ar * cg * cg;
    double roots[4];
    const int nr = pnp_quartic(A4, A3, A2, A1, A0, roots);
    double fw[3][3];
    pnp_frame(Pw[0], Pw[1], Pw[2], fw);
    double best = INFINITY;
    bool found = false;
    for (int ri = 0; ri < nr; ++ri) {
        const double v = roots[ri];
        if (!(v > 0.0)) continue;
        const double den = 2.0 * (cg - v * ca);
        if (!(fabs(den) > 1e-12)) continue;
        const double u = ((q - 1.0) * v * v - 2.0 * q * cb * v + 1.0 + q) / den;
        if (!(u > 0.0)) continue;
        const double dd = 1.0 + u * u - 2.0 * u * cg;
        if (!(dd > 0.0)) continue;
        double s1 = sqrt(c2 / dd), s2 = u * s1, s3 = v * s1;
        // two Newton steps on |s_i f_i - s_j f_j|^2 = d_ij^2 (Cramer's rule): u comes out of a division that loses digits
        // where `den` is small, and the depths are then consistent to ~1e-8 only
        for (int it = 0; it < 2; ++it) {
            const double F0 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2;
            const double F1 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2;
            const double F2 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2;
            const double j00 = 2.0 * (s1 - s2 * cg), j01 = 2.0 * (s2 - s1 * cg);
            const double j10 = 2.0 * (s1 - s3 * cb), j12 = 2.0 * (s3 - s1 * cb);
            const double j21 = 2.0 * (s2 - s3 * ca), j22 = 2.0 * (s3 - s2 * ca);
            const double det = -j00 * j12 * j21 - j01 * j10 * j22;
            if (!(fabs(det) > 0.0)) break;
            const double d1 = (F0 * j12 * j21 + j01 * (F1 * j22 - j12 * F2)) / det;
            const double d2 = (-j00 * (j22 * F1 - j12 * F2) + F0 * j10 * j22) / det;
            const double d3 = (j00 * j21 * F1 + j01 * j10 * F2 - F0 * j10 * j21) / det;
            s1 += d1; s2 += d2; s3 += d3;
        }
        if (!(s1 > 0.0 && s2 > 0.0 && s3 > 0.0)) continue;
        double X[3][3], fc[3][3];
        for (int i = 0; i < 3; ++i) { X[0][i] = s1 * f[0][i]; X[1][i] = s2 * f[1][i]; X[2][i] = s3 * f[2][i]; }
        pnp_frame(X[0], X[1], X[2], fc);
        double Rc[9], tc[3];                                  // R = sum_e fc[e] fw[e]^T
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) Rc[3 * i + j] = fc[0][i] * fw[0][j] + fc[1][i] * fw[1][j] + fc[2][i] * fw[2][j];
        for (int i = 0; i < 3; ++i)
            tc[i] = X[0][i] - (Rc[3 * i] * Pw[0][0] + Rc[3 * i + 1] * Pw[0][1] + Rc[3 * i + 2] * Pw[0][2]);
        double Y[3];
        for (int i = 0; i < 3; ++i) Y[i] = Rc[3 * i] * Pw[3][0] + Rc[3 * i + 1] * Pw[3][1] + Rc[3 * i + 2] * Pw[3][2] + tc[i];
        if (!(Y[2] > 0.0)) continue;
        const double du = (cam.fx * Y[0] + cam.sk * Y[1]) / Y[2] + cam.cx - px[3][0];
        const double dv = cam.fy * Y[1] / Y[2] + cam.cy - px[3][1];
        const double e2 = du * du + dv * dv;
        if (e2 < best) {
            best = e2;
            found = true;
            for (int i = 0; i < 9; ++i) R[i] = Rc[i];
            for (int i = 0; i < 3; ++i) t[i] = tc[i];
        }
    }
    return found;
}

__global__ __launch_bounds__(64) void spf_pnp_hypotheses_kernel(const SpfPnp a, const PnpWs ws, int32_t* __restrict__ ranks_out) {
    const int idx = blockIdx.x * 64 + threadIdx.x;           // iterations is a multiple of 64: no tail
    const int view = idx / a.iterations, k = idx - view * a.iterations, G = ws.G;
    const uint32_t* __restrict__ prefix = ws.prefix + (size_t)view * (G + 1);
    const uint64_t* __restrict__ words = ws.words + (size_t)view * G;
    ws.counts[idx] = 0u;
    const uint32_t n = prefix[G];
    int ranks[4] = {-1, -1, -1, -1};
    bool ok = n >= 4u;
    if (ok) {
        uint32_t draw = 0;
        int redraws = 0;
        for (int j = 0; j < 4 && ok; ++j) {
            for (;;) {
                const int r = (int)__umulhi(pnp_hash(a.seed, (uint32_t)k, draw++), n);
                bool dup = false;
                for (int e = 0; e < j; ++e) dup = dup || ranks[e] == r;
                if (!dup) { ranks[j] = r; break; }
                if (++redraws > kPnpRedraws) { ok = false; break; }
            }
        }
    }
    if (ranks_out)
        for (int j = 0; j < 4; ++j) ranks_out[4 * (size_t)idx + j] = ranks[j];
    double R[9], t[3];
    if (ok) {
        double Pw[4][3], px[4][2];
        for (int j = 0; j < 4; ++j) {
            const uint32_t r = (uint32_t)ranks[j];
            int lo = 0, hi = G;                               // the last group whose scanned count is <= r
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (prefix[mid] <= r) lo = mid; else hi = mid;
            }
            uint64_t m = words[lo];
            for (uint32_t s = min(r - prefix[lo], 63u); s > 0; --s) m &= m - 1;      // drop the lower set bits
            const int p = lo * 64 + (m ? __builtin_ctzll(m) : 0);
            float x, y, z;
            pnp_load(a, view, p < a.h * a.w ? p : 0, x, y, z);
            Pw[j][0] = x; Pw[j][1] = y; Pw[j][2] = z;
            px[j][0] = (double)(p % a.w); px[j][1] = (double)(p / a.w);
        }
        ok = pnp_p3p(pnp_camera(a, view), Pw, px, R, t);
    }
    float* __restrict__ o = ws.hyp + 12 * (size_t)idx;
    if (ok) {
        bool fin = true;
        for (int i = 0; i < 9; ++i) { o[i] = (float)R[i]; fin = fin && isfinite(o[i]); }
        for (int i = 0; i < 3; ++i) { o[9 + i] = (float)t[i]; fin = fin && isfinite(o[9 + i]); }
        if (!fin) o[0] = NAN;
    } else {
        o[0] = NAN;
        for (int i = 1; i < 12; ++i) o[i] = 0.f;
    }
}

// ---- score -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPnpScoreBlock) void spf_pnp_score_kernel(const SpfPnp a, const PnpWs ws) {
    extern __shared__ float sh[];                             // [iters][12] hypotheses | [iters] counts
    const int view = blockIdx.y, hw = a.h * a.w, iters = a.iterations, tid = threadIdx.x;
    uint32_t* shc = reinterpret_cast<uint32_t*>(sh + 12 * iters);
    const float* __restrict__ hyp = ws.hyp + 12 * (size_t)view * iters;
    for (int i = tid; i < 12 * iters; i += kPnpScoreBlock) sh[i] = hyp[i];
    for (int i = tid; i < iters; i += kPnpScoreBlock) shc[i] = 0u;
    const float* __restrict__ K = a.K + 9 * (size_t)view;
    const float fx = K[0] * a.w, sk = K[1] * a.w, cx = K[2] * a.w, fy = K[4] * a.h, cy = K[5] * a.h;
    const float thr2 = a.reprojection_error * a.reprojection_error;
    float X[kPnpScorePts], Y[kPnpScorePts], Z[kPnpScorePts], U[kPnpScorePts], V[kPnpScorePts];
#pragma unroll
    for (int i = 0; i < kPnpScorePts; ++i) {
        const int p = (blockIdx.x * kPnpScorePts + i) * kPnpScoreBlock + tid;
        const bool c = p < hw && pnp_load(a, view, p, X[i], Y[i], Z[i]);
        if (!c) X[i] = Y[i] = Z[i] = NAN;                      // fails every test below
        U[i] = (float)(p % a.w) - cx;
        V[i] = (float)(p / a.w) - cy;
    }
    __syncthreads();
    const bool first = (tid & 63) == 0;
    for (int k = 0; k < iters; ++k) {
        const float* h = sh + 12 * k;                          // one address for the wave: an LDS broadcast read
        const float r0 = h[0], r1 = h[1], r2 = h[2], r3 = h[3], r4 = h[4], r5 = h[5], r6 = h[6], r7 = h[7], r8 = h[8];
        const float t0 = h[9], t1 = h[10], t2 = h[11];
        uint32_t cnt = 0;
#pragma unroll
        for (int i = 0; i < kPnpScorePts; ++i) {
            const float xc = r0 * X[i] + r1 * Y[i] + r2 * Z[i] + t0;
            const float yc = r3 * X[i] + r4 * Y[i] + r5 * Z[i] + t1;
            const float zc = r6 * X[i] + r7 * Y[i] + r8 * Z[i] + t2;
            const float iz = __builtin_amdgcn_rcpf(zc);
            const float du = (fx * xc + sk * yc) * iz - U[i], dv = fy * yc * iz - V[i];
            cnt += (uint32_t)__popcll(lane_ballot(zc > 0.f && du * du + dv * dv < thr2));
        }
        if (first && cnt) atomicAdd(&shc[k], cnt);
    }
    __syncthreads();
    uint32_t* __restrict__ counts = ws.counts + (size_t)view * iters;
    for (int k = tid; k < iters; k += kPnpScoreBlock)
        if (shc[k]) atomicAdd(&counts[k], shc[k]);
}

// ---- refinement ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double pnp_wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// (A + 1e-9 trace(A) I) d = -g for the symmetric positive definite A given by its upper triangle (row-major, 21
// entries): Cholesky, straight-line.  false if a pivot is not positive or the result is not finite.
__device__ bool pnp_solve6(const double* s, double* d) {
    double A[6][6], L[6][6];
    int e = 0;
    double tr = 0.0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { A[i][j] = A[j][i] = s[e++]; }
    for (int i = 0; i < 6; ++i) tr += A[i][i];
    for (int i = 0; i < 6; ++i) A[i][i] += 1e-9 * tr;
    for (int j = 0; j < 6; ++j) {
        double dg = A[j][j];
        for (int k = 0; k < j; ++k) dg -= L[j][k] * L[j][k];
        if (!(dg > 0.0)) return false;
        L[j][j] = sqrt(dg);
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = -s[21 + i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
    bool fin = true;
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * d[k];
        d[i] = v / L[i][i];
        fin = fin && isfinite(d[i]);
    }
    return fin;
}

// R <- exp(w) R, t <- exp(w) t + dt  (pose = R[9] | t[3])
__device__ void pnp_update(double* pose, const double* d) {
    const double th2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2], th = sqrt(th2);
    double A = 1.0, B = 0.0;
    if (th >= 1e-12) { A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
    const double Kx[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
    double E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double kk = 0.0;
            for (int k = 0; k < 3; ++k) kk += Kx[3 * i + k] * Kx[3 * k + j];
            E[3 * i + j] = (i == j ? 1.0 : 0.0) + A * Kx[3 * i + j] + B * kk;
        }
    double Rn[9], tn[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Rn[3 * i + j] = E[3 * i] * pose[j] + E[3 * i + 1] * pose[3 + j] + E[3 * i + 2] * pose[6 + j];
        tn[i] = E[3 * i] * pose[9] + E[3 * i + 1] * pose[10] + E[3 * i + 2] * pose[11] + d[3 + i];
    }
    for (int i = 0; i < 9; ++i) pose[i] = Rn[i];
    for (int i = 0; i < 3; ++i) pose[9 + i] = tn[i];
}

__global__ __launch_bounds__(kPnpRefineBlock) void spf_pnp_refine_kernel(const SpfPnp a, const PnpWs ws, float* __restrict__ poses,
                                                                      int32_t* __restrict__ info) {
    __shared__ double red[kPnpRefineBlock / 64][kPnpSums];
    __shared__ unsigned long long keys[kPnpRefineBlock / 64];
    __shared__ double pose_sh[12];
    __shared__ int alive_sh;
    const int view = blockIdx.x, views = gridDim.x, hw = a.h * a.w, iters = a.iterations;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t n = ws.prefix[(size_t)view * (ws.G + 1) + ws.G];
    // arg-max of the counts, ties to the lowest k
    const uint32_t* __restrict__ counts = ws.counts + (size_t)view * iters;
    unsigned long long key = 0ull;
    for (int k = tid; k < iters; k += kPnpRefineBlock) {
        const unsigned long long c = ((unsigned long long)counts[k] << 32) | (0xffffffffu - (uint32_t)k);
        key = c > key ? c : key;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64);
        key = other > key ? other : key;
    }
    if (lane == 0) keys[wave] = key;
    __syncthreads();
    key = 0ull;
    for (int i = 0; i < kPnpRefineBlock / 64; ++i) key = keys[i] > key ? keys[i] : key;
    const uint32_t best = (uint32_t)(key >> 32);
    const int kbest = (int)(0xffffffffu - (uint32_t)key);
    bool alive = n >= 4u && best >= 4u;
    double pose[12];
    for (int i = 0; i < 12; ++i) pose[i] = alive ? (double)ws.hyp[12 * ((size_t)view * iters + kbest) + i] : 0.0;
    if (alive) {                                              // Gram-Schmidt on the rows: the float32 store left a rotation to 6e-8 only
        const double n0 = 1.0 / sqrt(pose[0] * pose[0] + pose[1] * pose[1] + pose[2] * pose[2]);
        for (int i = 0; i < 3; ++i) pose[i] *= n0;
        const double dt = pose[3] * pose[0] + pose[4] * pose[1] + pose[5] * pose[2];
        for (int i = 0; i < 3; ++i) pose[3 + i] -= dt * pose[i];
        const double n1 = 1.0 / sqrt(pose[3] * pose[3] + pose[4] * pose[4] + pose[5] * pose[5]);
        for (int i = 0; i < 3; ++i) pose[3 + i] *= n1;
        pnp_cross(pose, pose + 3, pose + 6);
    }
    const PnpCam cam = pnp_camera(a, view);
    const double thr2 = (double)a.reprojection_error * (double)a.reprojection_error;
    int inliers = 0;
    for (int it = 0; alive && it <= a.refine_steps; ++it) {
        const bool last = it == a.refine_steps;              // the last pass only counts
        double acc[kPnpSums];
#pragma unroll
        for (int i = 0; i < kPnpSums; ++i) acc[i] = 0.0;
        for (int p = tid; p < hw; p += kPnpRefineBlock) {
            float xf, yf, zf;
            if (!pnp_load(a, view, p, xf, yf, zf)) continue;
            const double X = pose[0] * xf + pose[1] * yf + pose[2] * zf + pose[9];
            const double Y = pose[3] * xf + pose[4] * yf + pose[5] * zf + pose[10];
            const double Z = pose[6] * xf + pose[7] * yf + pose[8] * zf + pose[11];
            if (!(Z > 0.0)) continue;
            const double iz = 1.0 / Z;
            const double ru = (cam.fx * X + cam.sk * Y) * iz + cam.cx - (double)(p % a.w);
            const double rv = cam.fy * Y * iz + cam.cy - (double)(p / a.w);
            if (!(ru * ru + rv * rv < thr2)) continue;
            acc[27] += 1.0;
            if (last) continue;
            const double du[3] = {cam.fx * iz, cam.sk * iz, -(cam.fx * X + cam.sk * Y) * iz * iz};
            const double dv[3] = {0.0, cam.fy * iz, -cam.fy * Y * iz * iz};
            const double ju[6] = {Y * du[2] - Z * du[1], Z * du[0] - X * du[2], X * du[1] - Y * du[0], du[0], du[1], du[2]};
            const double jv[6] = {Y * dv[2] - Z * dv[1], Z * dv[0] - X * dv[2], X * dv[1] - Y * dv[0], dv[0], dv[1], dv[2]};
            int e = 0;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) acc[e++] += ju[i] * ju[j] + jv[i] * jv[j];
#pragma unroll
            for (int i = 0; i < 6; ++i) acc[21 + i] += ju[i] * ru + jv[i] * rv;
        }
#pragma unroll
        for (int i = 0; i < kPnpSums; ++i) {
            const double s = pnp_wave_sum(acc[i]);
            if (lane == 0) red[wave][i] = s;
        }
        __syncthreads();
        if (tid == 0) {
            double s[kPnpSums];
            for (int i = 0; i < kPnpSums; ++i) {
                double v = 0.0;
                for (int w = 0; w < kPnpRefineBlock / 64; ++w) v += red[w][i];
                s[i] = v;
            }
            const int cnt = (int)s[27];
            int ok = cnt >= 4;
            if (ok && !last) {
                double d[6], np[12];
                for (int i = 0; i < 12; ++i) np[i] = pose[i];
                ok = pnp_solve6(s, d);
                if (ok) {
                    pnp_update(np, d);
                    for (int i = 0; i < 12; ++i) { pose_sh[i] = np[i]; ok = ok && isfinite(np[i]); }
                }
            }
            alive_sh = ok ? cnt : -1;
        }
        __syncthreads();
        alive = alive_sh >= 0;
        inliers = alive_sh;
        if (alive && !last)
            for (int i = 0; i < 12; ++i) pose[i] = pose_sh[i];
        __syncthreads();                                      // red, pose_sh and alive_sh are rewritten next round
    }
    if (tid == 0) {
        float* __restrict__ o = poses + 16 * (size_t)view;
        if (alive) {                                          // camera -> world: [R^T | -R^T t]
            for (int i = 0; i < 3; ++i) {
                for (int j = 0; j < 3; ++j) o[4 * i + j] = (float)pose[3 * j + i];
                o[4 * i + 3] = (float)-(pose[i] * pose[9] + pose[3 + i] * pose[10] + pose[6 + i] * pose[11]);
            }
        } else {
            for (int i = 0; i < 12; ++i) o[i] = (i % 5 == 0) ? 1.f : 0.f;
        }
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
        info[view] = alive ? inliers : 0;
        info[views + view] = (int32_t)n;
        info[2 * views + view] = alive ? kbest : -1;
        info[3 * views + view] = alive ? 1 : 0;
    }
}

}  // namespace

int64_t pnp_workspace_bytes(int views, int h, int w, int iters) {
    const int64_t G = pnp_groups(h * w);
    const int64_t bytes = (int64_t)views * (8 * G + 4 * (G + 1) + 52 * (int64_t)iters);
    return (bytes + 15) & ~(int64_t)15;
}

hipError_t launch_pnp_solve(const SpfPnp& a, void* workspace, float* poses, int32_t* info, int32_t* ranks, hipStream_t stream) {
    const int views = a.b * a.v, hw = a.h * a.w;
    const PnpWs ws = pnp_workspace(workspace, views, hw, a.iterations);
    spf_pnp_mask_kernel<<<views, kPnpMaskBlock, 0, stream>>>(a, ws);
    spf_pnp_hypotheses_kernel<<<views * (a.iterations / 64), 64, 0, stream>>>(a, ws, ranks);
    const int chunk = kPnpScoreBlock * kPnpScorePts;
    spf_pnp_score_kernel<<<dim3((hw + chunk - 1) / chunk, views), kPnpScoreBlock, (size_t)a.iterations * 52, stream>>>(a, ws);
    spf_pnp_refine_kernel<<<views, kPnpRefineBlock, 0, stream>>>(a, ws, poses, info);
    return hipGetLastError();
}

}  // namespace spf
