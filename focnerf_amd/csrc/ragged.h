// ragged.h — the composite over ragged sample lists (raymarching.cu:500-693), one wave per ray and 64 samples per step, defined once for
// k_composite_train_fwd / _bwd (raymarching.hip) and the fused tails k_occ_tail_fwd / _bwd (occtrain.hip): the kernels differ in how
// they load a sample and in what they store, so the tails are the bits of the plain chain by construction.
#pragma once
#include "common.h"

// Row n of the `rays` table and whether its samples take part (raymarching.cu:515: empty rays and rays past the list are skipped). The
// sum is taken in 64 bits; a 32-bit sum differs only where offset + count wraps, which no list this library can allocate reaches.
struct OtRay { uint32_t index, offset, count; bool fits; };
__device__ __forceinline__ OtRay ot_ray(const int32_t *__restrict__ rays, uint32_t n, uint32_t M) {
    OtRay r;
    r.index = (uint32_t)rays[n * 3]; r.offset = (uint32_t)rays[n * 3 + 1]; r.count = (uint32_t)rays[n * 3 + 2];
    r.fits = r.count != 0u && (uint64_t)r.offset + r.count <= M;
    return r;
}

// One step of 64 samples, the lane's sample given by (valid, sigma, dt0): transmittance before / after it, `term` = the lanes at which
// the ray drops below T_thresh (non-zero: this is the ray's last step), act = the sample counts (the reference breaks AFTER
// accumulating the sample whose T drops below the threshold), w = its weight (0 where it does not count).
struct OtStep { float T_before, T_after, w; unsigned long long term; bool act; };
__device__ __forceinline__ OtStep ot_step(bool valid, float sigma, float dt0, float T_carry, float T_thresh, uint32_t lane) {
    OtStep st;
    const float alpha = valid ? 1.0f - __expf(-sigma * dt0) : 0.0f;
    const float om = 1.0f - alpha;
    float P;
    const float Pex = wave_prod_scan(om, lane, P);
    st.T_before = T_carry * Pex;
    st.T_after = T_carry * P;
    st.term = __ballot(valid && (st.T_after < T_thresh));
    const int first = st.term ? (int)__ffsll((long long)st.term) - 1 : 64;
    st.act = valid && (int)lane <= first;
    st.w = st.act ? alpha * st.T_before : 0.0f;
    return st;
}

// The backward's view of a ray: the image gradient, the forward's colour, and ws_term = grad_weights_sum (1 - weights_sum).
struct OtRayGrad { float g0, g1, g2, r_final, g_final, b_final, ws_term; };
__device__ __forceinline__ OtRayGrad ot_ray_grad(const float *__restrict__ grad_image, const float *__restrict__ image, const float *__restrict__ weights_sum,
                                                 uint32_t index, float gws) {
    return OtRayGrad{grad_image[index * 3], grad_image[index * 3 + 1], grad_image[index * 3 + 2],
                     image[index * 3],      image[index * 3 + 1],      image[index * 3 + 2],      gws * (1 - weights_sum[index])};
}
// The running colour INCLUDING the lane's sample (:648-650) and, from it, grad_sigma / dt0 of that sample (:664-671).
struct OtColour { float r, g, b; };
__device__ __forceinline__ OtColour ot_running(const OtColour &carry, float w, float c0, float c1, float c2, uint32_t lane) {
    return OtColour{carry.r + wave_incl_sum(w * c0, (int)lane), carry.g + wave_incl_sum(w * c1, (int)lane), carry.b + wave_incl_sum(w * c2, (int)lane)};
}
__device__ __forceinline__ OtColour ot_last(const OtColour &acc) { return OtColour{__shfl(acc.r, 63, 64), __shfl(acc.g, 63, 64), __shfl(acc.b, 63, 64)}; }
__device__ __forceinline__ float ot_grad_acc(const OtRayGrad &q, float T_after, float c0, float c1, float c2, const OtColour &acc) {
    float a = q.g0 * fmaf(T_after, c0, -(q.r_final - acc.r));
    a = fmaf(q.g1, fmaf(T_after, c1, -(q.g_final - acc.g)), a);
    a = fmaf(q.g2, fmaf(T_after, c2, -(q.b_final - acc.b)), a);
    return a + q.ws_term;
}
