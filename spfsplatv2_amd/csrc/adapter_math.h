// Per-Gaussian math of the Gaussian adapter and of the encoder tail (tail.hip, one channel per plane):
//   scales    = min(0.001 softplus(x), 0.3)                      (gaussian_adapter.py:133)
//   rotations = q / (|q| + eps)                                  (gaussian_adapter.py:136)
//   opacity   = 0.5 (1 - (1 - p)^e + p^(1/e)),  p = sigmoid(x)   (encoder_spfsplatv2.py:146-159, 257)
// and their derivatives.  The expressions of the first two are those of adapter.hip's row kernels, term by term (on the
// device the two files' scales and rotations come out bit for bit equal: tests/test_gpu_tail.py prints it).  adapter.hip
// keeps its own copy: with these functions in its kernels the compiler reports the same VGPR / SGPR / LDS / scratch
// figures (profiles/tail_resources.txt) but schedules the instructions differently, and the row kernels' measured
// times and bits are not this file's to move.
#pragma once
#include "spf_common.h"

namespace spf {

__device__ __forceinline__ float adapter_scale(float x) { return fminf(0.001f * softplus_torch(x), 0.3f); }

// d scale / d x times the upstream gradient g: softplus' = sigmoid; clamp_max passes the gradient up to the bound
__device__ __forceinline__ float adapter_scale_grad(float x, float g) {
    const float sp = softplus_torch(x);
    const float dsp = x > 20.f ? 1.f : 1.f / (1.f + expf(-x));
    const float pass = (0.001f * sp <= 0.3f) ? 1.f : 0.f;
    return g * 0.001f * dsp * pass;
}

// 1 / (|q| + eps)
__device__ __forceinline__ float quat_inv_norm(float q0, float q1, float q2, float q3, float eps) {
    return 1.0f / (sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3) + eps);
}

// r = q / (|q| + eps): dq = g / d - q (q . g) / (|q| d^2), d = |q| + eps; the zero quaternion passes g / eps
__device__ __forceinline__ void quat_normalise_grad(const float (&q)[4], const float (&g)[4], float eps, float (&out)[4]) {
    const float nrm = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float d = nrm + eps, dot = g[0] * q[0] + g[1] * q[1] + g[2] * q[2] + g[3] * q[3];
    const float k = nrm > 0.f ? dot / (nrm * d * d) : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = g[i] / d - q[i] * k;
}

// The opacity map on a density LOGIT x, in logarithms: log p = logsigmoid(x) and log(1 - p) = logsigmoid(-x) share one
// log1p(exp(-|x|)), so (1 - p)^e = exp(e log(1 - p)) and p^(1/e) = exp(log p / e) are finite and accurate in relative
// terms for every finite x -- there is no 1 - p that cancels to 0 and no 0 raised to a negative power.  p and 1 - p
// themselves, the plain factors of the derivative, come from the same exp(-|x|) as quotients (exp(log p) would carry
// the rounding of log p, 4 ulp at |x| = 12).
struct OpacityTerms {
    float lp, lq;            // log p, log(1 - p)
    float p, q;              // p = sigmoid(x), 1 - p = sigmoid(-x)
};
__device__ __forceinline__ OpacityTerms opacity_terms(float x) {
    const float ex = expf(-fabsf(x));
    const float t = log1pf(ex), r = 1.0f / (1.0f + ex);
    const bool neg = x < 0.f;
    return {fminf(x, 0.f) - t, fminf(-x, 0.f) - t, neg ? ex * r : r, neg ? r : ex * r};
}
__device__ __forceinline__ float opacity_map(float x, float e, float inv_e) {
    const OpacityTerms l = opacity_terms(x);
    if (e == 1.0f) return l.p;                                   // 0.5 (1 - (1 - p) + p), without the powers
    return 0.5f * (1.0f - expf(e * l.lq) + expf(l.lp * inv_e));
}
// d opacity / d x = 0.5 (e (1 - p)^e p + (1/e) p^(1/e) (1 - p))
__device__ __forceinline__ float opacity_map_grad(float x, float e, float inv_e) {
    const OpacityTerms l = opacity_terms(x);
    if (e == 1.0f) return l.p * l.q;                             // 0.5 ((1 - p) p + p (1 - p))
    return 0.5f * (e * expf(e * l.lq) * l.p + inv_e * expf(l.lp * inv_e) * l.q);
}

}  // namespace spf
