// The 2-D rotary embedding's arithmetic, shared by the in-place kernels (rope2d.hip) and the fused attention
// kernels (attention.hip): the inverse-frequency table, the element conversions and the angle evaluation.  Both
// rotate with exactly these functions, so a token rotated in place and one rotated while it is staged agree bitwise.
#pragma once

#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#include <math.h>

#include "spf_common.h"

namespace spf {

struct RopeFreq {
    float inv[64];  // fwd / base^(q/Q), q < Q <= 64
};

template <typename T>
__device__ __forceinline__ float to_f(T v);
template <> __device__ __forceinline__ float to_f<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f<__half>(__half v) { return __half2float(v); }
template <> __device__ __forceinline__ float to_f<__hip_bfloat16>(__hip_bfloat16 v) { return __bfloat162float(v); }
template <typename T>
__device__ __forceinline__ T from_f(float v);
template <> __device__ __forceinline__ float from_f<float>(float v) { return v; }
template <> __device__ __forceinline__ __half from_f<__half>(float v) { return __float2half(v); }
template <> __device__ __forceinline__ __hip_bfloat16 from_f<__hip_bfloat16>(float v) { return __float2bfloat16(v); }

// The Q inverse frequencies, computed on the host with libm powf (what the reference's CPU path evaluates,
// curope/curope.cpp:35); they travel in the kernel-argument segment.
inline RopeFreq rope_freq(int D, float base, float fwd) {
    RopeFreq f;
    const int Q = D / 4;
    for (int q = 0; q < 64; ++q) f.inv[q] = q < Q ? fwd / powf(base, q / float(Q)) : 0.f;
    return f;
}

// sin and cos of a rotation angle: Cody-Waite reduction by pi/2 in three fused steps (pi/2 = hi + mid + lo to ~72 bits;
// the fma keeps each partial product exact, so the reduced argument is good to half an ulp for |k| < 2^15) and the
// cephes minimax polynomials on [-pi/4, pi/4]: max abs error 8.9e-8 against float64 over positions 0..30000 x every
// frequency (checked on the CPU with emulated float32 fmas) -- the libm sincosf this replaces is good to 1 ulp too, at
// three times the instructions (its Payne-Hanek path for huge arguments is kept for exactly those).  The angle's
// evaluation was what made the half types compute-bound.
__device__ __forceinline__ void rope_sincos(float x, float& s, float& c) {
    if (!(fabsf(x) < 30000.f)) { sincosf(x, &s, &c); return; }           // (huge positions, inf, nan: libm)
    const float kf = rintf(x * 0.63661977236758134f);
    float r = fmaf(-kf, 1.5707963705062866f, x);
    r = fmaf(-kf, -4.371138828673793e-08f, r);
    r = fmaf(-kf, -1.7763568394002505e-15f, r);
    const float z = r * r;
    const float ps = fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f);
    const float sr = fmaf(ps * z, r, r);
    const float pc = fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f);
    const float cr = fmaf(pc * z, z, fmaf(-0.5f, z, 1.0f));
    const int k = (int)kf;
    const float a = (k & 1) ? cr : sr, b = (k & 1) ? sr : cr;            // quadrant: (s, c) = (sr, cr), (cr, -sr), (-sr, -cr), (-cr, sr)
    s = (k & 2) ? -a : a;
    c = ((k + 1) & 2) ? -b : b;
}

}  // namespace spf
