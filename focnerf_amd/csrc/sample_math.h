// sample_math.h — the per-sample arithmetic that several kernels must evaluate to the same bits, defined once: the SH row, the half
// sigmoid, trunc_exp's backward factor, the background pick. A fused kernel is pinned bit for bit to the chain of plain kernels it
// replaces because both call these functions (the library is compiled with -ffp-contract=off -fno-fast-math: inlining keeps the arithmetic).
#pragma once
#include "common.h"

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// degree-4 real spherical harmonics (focnerf_amd/shencoder.py), same expressions in fp32.
// ffmlp.hip nf_sh16_half evaluates one half of this row chosen at run time and repeats the expressions for that reason.
__device__ __forceinline__ void foc_sh16(float x, float y, float z, float (&o)[16]) {
    const float xy = x * y, xz = x * z, yz = y * z, x2 = x * x, y2 = y * y, z2 = z * z;
    o[0] = 0.28209479177387814f;
    o[1] = -0.48860251190291987f * y;
    o[2] = 0.48860251190291987f * z;
    o[3] = -0.48860251190291987f * x;
    o[4] = 1.0925484305920792f * xy;
    o[5] = -1.0925484305920792f * yz;
    o[6] = 0.94617469575755997f * z2 - 0.31539156525251999f;
    o[7] = -1.0925484305920792f * xz;
    o[8] = 0.54627421529603959f * x2 - 0.54627421529603959f * y2;
    o[9] = 0.59004358992664352f * y * (-3.0f * x2 + y2);
    o[10] = 2.8906114426405538f * xy * z;
    o[11] = 0.45704579946446572f * y * (1.0f - 5.0f * z2);
    o[12] = 0.3731763325901154f * z * (5.0f * z2 - 3.0f);
    o[13] = 0.45704579946446572f * x * (1.0f - 5.0f * z2);
    o[14] = 1.4453057213202769f * z * (x2 - y2);
    o[15] = 0.59004358992664352f * x * (-x2 + 3.0f * y2);
}
// the row as it stands in the colour network's input: each value rounded to fp16 on its own
__device__ __forceinline__ void foc_sh16_h(float x, float y, float z, h8 &lo, h8 &hi) {
    float sh[16];
    foc_sh16(x, y, z, sh);
#pragma unroll
    for (int k = 0; k < 8; k++) { lo[k] = foc_f2h(sh[k]); hi[k] = foc_f2h(sh[8 + k]); }
}

// torch.sigmoid on a HALF tensor (network_ff.py:117): evaluated in fp32, one rounding to fp16
__device__ __forceinline__ float foc_sigmoid_h(float x) { return (float)(_Float16)(1.0f / (1.0f + expf(-x))); }

// trunc_exp's backward factor exp(clamp(x, -15, 15)) (activation.py:15-18); a NaN input stays NaN
__device__ __forceinline__ float foc_clamp15(float x) { return x < -15.0f ? -15.0f : (x > 15.0f ? 15.0f : x); }
__device__ __forceinline__ float foc_trunc_exp_bwd(float x) { return expf(foc_clamp15(x)); }
// the same where e = expf(x) is at hand: a second exp only for the clamped inputs
__device__ __forceinline__ float foc_trunc_exp_bwd(float x, float e) {
    const float xc = foc_clamp15(x);
    return xc != x ? expf(xc) : e;
}
// The factor from sigma = expf(x) alone, for a kernel that does not read x: clamp(sigma, exp(-15), exp(15)) — the same bits, expf being
// monotonic. The bounds must come out of the device's expf like every other exp, so they are taken from values the compiler cannot fold.
struct FocExp15 { float lo, hi; };
__device__ __forceinline__ FocExp15 foc_exp15() {
    float a = -15.0f, b = 15.0f;
    asm volatile("" : "+v"(a));
    asm volatile("" : "+v"(b));
    return FocExp15{expf(a), expf(b)};
}
__device__ __forceinline__ float foc_trunc_exp_bwd_of_sigma(float sigma, const FocExp15 &e) { return fminf(fmaxf(sigma, e.lo), e.hi); }

// a ray's background colour: its row of the per-ray table [N,3], or the scalar three times
struct FocBg { float b0, b1, b2; };
__device__ __forceinline__ FocBg foc_bg(const float *__restrict__ bg_ray, float bg_scalar, uint32_t k) {
    return FocBg{bg_ray ? bg_ray[k * 3] : bg_scalar, bg_ray ? bg_ray[k * 3 + 1] : bg_scalar, bg_ray ? bg_ray[k * 3 + 2] : bg_scalar};
}
