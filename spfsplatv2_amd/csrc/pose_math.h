// Per-scene pose arithmetic of pose.hip, in float64: decode of the two pose encodings, the baseline / relative-pose
// coupling of a scene's views and the gradient of all of it, and the pose-error formulas.  A scene is a few hundred
// flops, so one lane walks its views in order: every sum has one order and nothing is shared between lanes.
// Included by pose.hip after spf_common.h (inv4); it includes nothing itself.
#pragma once

namespace spf {

constexpr double kPoseEps = 1e-12;   // torch.nn.functional.normalize's eps, as rotation_6d_to_matrix uses it

__device__ __forceinline__ double pose_dot3(const double* a, const double* b) {
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2];
}
__device__ __forceinline__ void pose_cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// The nine entries of Q in quat_to_mat's R = I + two_s Q for the scalar-LAST quaternion (i, j, k, r).
__device__ __forceinline__ void pose_quat_q(double i, double j, double k, double r, double* Q) {
    Q[0] = -(j * j + k * k); Q[1] = i * j - k * r;    Q[2] = i * k + j * r;
    Q[3] = i * j + k * r;    Q[4] = -(i * i + k * k); Q[5] = j * k - i * r;
    Q[6] = i * k - j * r;    Q[7] = j * k + i * r;    Q[8] = -(i * i + j * j);
}

// One view's camera->world pose P (3x4 row-major: R | t) from its nine floats.
//   SPF_POSE_ROT6D: Gram-Schmidt of columns 0:3, 3:6 into the ROWS of R; t = columns 6:9.
//   SPF_POSE_QUAT:  world->camera (R(q), T) with T = 0:3 and q = 3:7 scalar-last and not normalised; P = [R^T | -R^T T].
__device__ __forceinline__ void pose_decode(const float* __restrict__ e, int encoding, double* __restrict__ P) {
    if (encoding == SPF_POSE_ROT6D) {
        const double a1[3] = {(double)e[0], (double)e[1], (double)e[2]};
        const double a2[3] = {(double)e[3], (double)e[4], (double)e[5]};
        const double n1 = sqrt(pose_dot3(a1, a1)), m1 = n1 > kPoseEps ? n1 : kPoseEps;
        const double b1[3] = {a1[0] / m1, a1[1] / m1, a1[2] / m1};
        const double c = pose_dot3(b1, a2);
        const double u[3] = {a2[0] - c * b1[0], a2[1] - c * b1[1], a2[2] - c * b1[2]};
        const double n2 = sqrt(pose_dot3(u, u)), m2 = n2 > kPoseEps ? n2 : kPoseEps;
        const double b2[3] = {u[0] / m2, u[1] / m2, u[2] / m2};
        double b3[3];
        pose_cross3(b1, b2, b3);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            P[k] = b1[k];
            P[4 + k] = b2[k];
            P[8 + k] = b3[k];
            P[4 * k + 3] = (double)e[6 + k];
        }
    } else {
        const double T[3] = {(double)e[0], (double)e[1], (double)e[2]};
        const double i = e[3], j = e[4], k = e[5], r = e[6];
        const double two_s = 2.0 / (i * i + j * j + k * k + r * r);
        double Q[9];
        pose_quat_q(i, j, k, r, Q);
#pragma unroll
        for (int m = 0; m < 9; ++m) Q[m] = ((m & 3) == 0 ? 1.0 : 0.0) + two_s * Q[m];   // R (world->camera); m = 0, 4, 8: diagonal
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) P[4 * a + b] = Q[3 * b + a];
            P[4 * a + 3] = -(Q[a] * T[0] + Q[3 + a] * T[1] + Q[6 + a] * T[2]);
        }
    }
}

// dL/de[9] from dL/dP[12] of pose_decode (same layout).
__device__ __forceinline__ void pose_decode_bwd(const float* __restrict__ e, int encoding, const double* __restrict__ dP,
                                                double* __restrict__ de) {
    if (encoding == SPF_POSE_ROT6D) {
        const double a1[3] = {(double)e[0], (double)e[1], (double)e[2]};
        const double a2[3] = {(double)e[3], (double)e[4], (double)e[5]};
        const double n1 = sqrt(pose_dot3(a1, a1)), m1 = n1 > kPoseEps ? n1 : kPoseEps;
        const double b1[3] = {a1[0] / m1, a1[1] / m1, a1[2] / m1};
        const double c = pose_dot3(b1, a2);
        const double u[3] = {a2[0] - c * b1[0], a2[1] - c * b1[1], a2[2] - c * b1[2]};
        const double n2 = sqrt(pose_dot3(u, u)), m2 = n2 > kPoseEps ? n2 : kPoseEps;
        const double b2[3] = {u[0] / m2, u[1] / m2, u[2] / m2};
        const double g1[3] = {dP[0], dP[1], dP[2]}, g2[3] = {dP[4], dP[5], dP[6]}, g3[3] = {dP[8], dP[9], dP[10]};
        // b3 = b1 x b2
        double x1[3], x2[3];
        pose_cross3(b2, g3, x1);
        pose_cross3(g3, b1, x2);
        double gb1[3] = {g1[0] + x1[0], g1[1] + x1[1], g1[2] + x1[2]};
        const double gb2[3] = {g2[0] + x2[0], g2[1] + x2[1], g2[2] + x2[2]};
        // b2 = u / max(|u|, eps): the clamp passes no gradient to the norm below eps
        const double p2 = n2 > kPoseEps ? pose_dot3(b2, gb2) : 0.0;
        const double du[3] = {(gb2[0] - b2[0] * p2) / m2, (gb2[1] - b2[1] * p2) / m2, (gb2[2] - b2[2] * p2) / m2};
        // u = a2 - (b1 . a2) b1
        const double q = pose_dot3(b1, du);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            de[3 + k] = du[k] - q * b1[k];
            gb1[k] += -q * a2[k] - c * du[k];
        }
        const double p1 = n1 > kPoseEps ? pose_dot3(b1, gb1) : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            de[k] = (gb1[k] - b1[k] * p1) / m1;
            de[6 + k] = dP[4 * k + 3];
        }
    } else {
        const double T[3] = {(double)e[0], (double)e[1], (double)e[2]};
        const double i = e[3], j = e[4], k = e[5], r = e[6];
        const double n = i * i + j * j + k * k + r * r, two_s = 2.0 / n;
        double Q[9], R[9], dR[9];
        pose_quat_q(i, j, k, r, Q);
#pragma unroll
        for (int m = 0; m < 9; ++m) R[m] = ((m & 3) == 0 ? 1.0 : 0.0) + two_s * Q[m];
        // P[a][b] = R[b][a]; P[a][3] = -sum_m R[m][a] T[m]
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            de[m] = -(R[3 * m] * dP[3] + R[3 * m + 1] * dP[7] + R[3 * m + 2] * dP[11]);
#pragma unroll
            for (int a = 0; a < 3; ++a) dR[3 * m + a] = dP[4 * a + m] - T[m] * dP[4 * a + 3];
        }
        double dts = 0.0;
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            dts += dR[m] * Q[m];
            dR[m] *= two_s;                      // now dL/dQ
        }
        const double dn = -2.0 / (n * n) * dts;
        de[3] = 2.0 * i * dn + j * (dR[1] + dR[3]) + k * (dR[2] + dR[6]) - 2.0 * i * (dR[4] + dR[8]) + r * (dR[7] - dR[5]);
        de[4] = 2.0 * j * dn + i * (dR[1] + dR[3]) + k * (dR[5] + dR[7]) - 2.0 * j * (dR[0] + dR[8]) + r * (dR[2] - dR[6]);
        de[5] = 2.0 * k * dn + i * (dR[2] + dR[6]) + j * (dR[5] + dR[7]) - 2.0 * k * (dR[0] + dR[4]) + r * (dR[3] - dR[1]);
        de[6] = 2.0 * r * dn + k * (dR[3] - dR[1]) + j * (dR[2] - dR[6]) + i * (dR[7] - dR[5]);
        de[7] = 0.0;
        de[8] = 0.0;
    }
}

struct PoseScene {
    const float* enc;          // view i's nine floats start at enc + i * stride_v
    int64_t stride_v;
    int v, cv, encoding, baseline, relative;
};

// The scene's scale s = |t_0 - t_{cv-1}| (1 without make_baseline_1) and its difference vector d.
__device__ __forceinline__ double pose_scene_scale(const PoseScene& sc, double* d) {
    d[0] = d[1] = d[2] = 0.0;
    if (!sc.baseline) return 1.0;
    double P0[12], Pc[12];
    pose_decode(sc.enc, sc.encoding, P0);
    pose_decode(sc.enc + (sc.cv - 1) * sc.stride_v, sc.encoding, Pc);
#pragma unroll
    for (int k = 0; k < 3; ++k) d[k] = P0[4 * k + 3] - Pc[4 * k + 3];
    return sqrt(pose_dot3(d, d));
}

// View i after the baseline division, as a 4x4 (bottom row 0 0 0 1).
__device__ __forceinline__ void pose_scene_view(const PoseScene& sc, int i, double s, double* P4) {
    pose_decode(sc.enc + i * sc.stride_v, sc.encoding, P4);
    if (sc.baseline) {
#pragma unroll
        for (int k = 0; k < 3; ++k) P4[4 * k + 3] /= s;
    }
    P4[12] = P4[13] = P4[14] = 0.0;
    P4[15] = 1.0;
}

// poses[v][16] of one scene.
__device__ __forceinline__ void pose_scene_forward(const PoseScene& sc, float* __restrict__ poses) {
    double d[3], B[16], P[16];
    const double s = pose_scene_scale(sc, d);
    if (sc.relative) {
        pose_scene_view(sc, 0, s, P);
        inv4<double>(P, B);                      // a GENERAL inverse, as torch.inverse
    }
    for (int i = 0; i < sc.v; ++i) {
        pose_scene_view(sc, i, s, P);
        float* o = poses + 16 * (int64_t)i;
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double x = P[4 * r + c];
                if (sc.relative) x = B[4 * r] * P[c] + B[4 * r + 1] * P[4 + c] + B[4 * r + 2] * P[8 + c] + B[4 * r + 3] * P[12 + c];
                o[4 * r + c] = (float)x;
            }
        o[12] = 0.f; o[13] = 0.f; o[14] = 0.f; o[15] = 1.f;
    }
}

// dL/dP_i (3x4, the pose after the baseline division) of view i from the upstream G_i = dL/dposes[i]: B3^T G_i with
// make_relative (plus E = the top rows of -B^T dB B^T for view 0, the base pose), else G_i itself.  The bottom row of
// G_i reaches only the constant bottom rows, so it is not read.
__device__ __forceinline__ void pose_scene_dview(const PoseScene& sc, int i, const float* __restrict__ G,
                                                 const double* B, const double* E, double* dP) {
    const float* g = G + 16 * (int64_t)i;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            double x = (double)g[4 * r + c];
            if (sc.relative) {
                x = B[r] * (double)g[c] + B[4 + r] * (double)g[4 + c] + B[8 + r] * (double)g[8 + c];
                if (i == 0) x += E[4 * r + c];
            }
            dP[4 * r + c] = x;
        }
}

// Through the baseline division (t = t_raw / s; dd = dL/d(t_0 - t_{cv-1}) goes to views 0 and cv-1) and the decode.
__device__ __forceinline__ void pose_scene_finish(const PoseScene& sc, int i, double s, const double* dd, double* dP,
                                                  float* __restrict__ denc) {
    if (sc.baseline) {
        const double sign = (i == 0 ? 1.0 : 0.0) - (i == sc.cv - 1 ? 1.0 : 0.0);
#pragma unroll
        for (int k = 0; k < 3; ++k) dP[4 * k + 3] = dP[4 * k + 3] / s + sign * dd[k];
    }
    double de[9];
    pose_decode_bwd(sc.enc + i * sc.stride_v, sc.encoding, dP, de);
    float* o = denc + 9 * (int64_t)i;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[k] = (float)de[k];
}

// dL/denc[v][9] of one scene from G = dL/dposes[v][16]; everything is recomputed from enc.
__device__ __forceinline__ void pose_scene_backward(const PoseScene& sc, const float* __restrict__ G,
                                                    float* __restrict__ denc) {
    double d[3], B[16], E[12], P[16], dP[12];
    const double s = pose_scene_scale(sc, d);
#pragma unroll
    for (int k = 0; k < 12; ++k) E[k] = 0.0;
    if (sc.relative) {
        pose_scene_view(sc, 0, s, P);
        inv4<double>(P, B);
        // dB[r][c] = sum_i sum_k G_i[r][k] P_i[c][k] (rows 0-2; out_i = B P_i)
        double dB[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) dB[k] = 0.0;
        for (int i = 0; i < sc.v; ++i) {
            pose_scene_view(sc, i, s, P);
            const float* g = G + 16 * (int64_t)i;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    dB[4 * r + c] += (double)g[4 * r] * P[4 * c] + (double)g[4 * r + 1] * P[4 * c + 1] +
                                     (double)g[4 * r + 2] * P[4 * c + 2] + (double)g[4 * r + 3] * P[4 * c + 3];
        }
        // E = rows 0-2 of -B^T dB B^T
        double T1[16];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                T1[4 * r + c] = B[r] * dB[c] + B[4 + r] * dB[4 + c] + B[8 + r] * dB[8 + c];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c)
                E[4 * r + c] = -(T1[4 * r] * B[4 * c] + T1[4 * r + 1] * B[4 * c + 1] + T1[4 * r + 2] * B[4 * c + 2] +
                                 T1[4 * r + 3] * B[4 * c + 3]);
    }
    // every view but 0 and cv-1 finishes at once; those two wait for dL/ds, which sums over all views
    double acc = 0.0;
    const double none[3] = {0.0, 0.0, 0.0};
    for (int i = 0; i < sc.v; ++i) {
        pose_scene_dview(sc, i, G, B, E, dP);
        if (sc.baseline) {
            pose_decode(sc.enc + i * sc.stride_v, sc.encoding, P);
            acc += dP[3] * P[3] + dP[7] * P[7] + dP[11] * P[11];
            if (i == 0 || i == sc.cv - 1) continue;
        }
        pose_scene_finish(sc, i, s, none, dP, denc);
    }
    if (sc.baseline) {
        const double ds = -acc / (s * s);
        const double dd[3] = {ds * d[0] / s, ds * d[1] / s, ds * d[2] / s};
        pose_scene_dview(sc, 0, G, B, E, dP);
        pose_scene_finish(sc, 0, s, dd, dP, denc);
        if (sc.cv != 1) {
            pose_scene_dview(sc, sc.cv - 1, G, B, E, dP);
            pose_scene_finish(sc, sc.cv - 1, s, dd, dP, denc);
        }
    }
}

// (error_t, error_t_scale, error_R) of one predicted / ground-truth pair of 4x4 poses (src/evaluation/metrics.py:70-99).
__device__ __forceinline__ void pose_error_one(const float* __restrict__ p, const float* __restrict__ g, double* out) {
    const double kDeg = 57.29577951308232;
    double tr = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) tr += (double)p[4 * r + c] * (double)g[4 * r + c];
    double cr = (tr - 1.0) / 2.0;
    cr = cr < -1.0 ? -1.0 : (cr > 1.0 ? 1.0 : cr);
    const double t[3] = {(double)p[3], (double)p[7], (double)p[11]}, tg[3] = {(double)g[3], (double)g[7], (double)g[11]};
    const double df[3] = {t[0] - tg[0], t[1] - tg[1], t[2] - tg[2]};
    double ct = pose_dot3(t, tg) / (sqrt(pose_dot3(t, t)) * sqrt(pose_dot3(tg, tg)) + 1e-9);
    ct = ct < -1.0 ? -1.0 : (ct > 1.0 ? 1.0 : ct);
    const double et = acos(ct) * kDeg;
    out[0] = et < 180.0 - et ? et : 180.0 - et;
    out[1] = sqrt(pose_dot3(df, df));
    out[2] = fabs(acos(cr)) * kDeg;
}

}  // namespace spf
