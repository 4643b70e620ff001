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

// ---------------------------------------------------------------- ray distortion (include/focnerf.h foc_occ_tail_forward_dist)
// dist = sum_i (1/3) dt0_i w_i^2 + 2 sum_i w_i (m_i W_<i - WM_<i), W_<i = sum_{j<i} w_j, WM_<i = sum_{j<i} w_j m_j, over the samples that count:
// m_i = the running sum of dt1 including sample i (the forward's tsum), the interval dt0_i, w = OtStep::w (0 behind the stop). One step of
// 64 samples: the two running sums by wave scan (W, WM = their values in front of the step, moved behind it). The forward adds the lane's
// own terms to `acc` (summed over the wave by the caller at the end). The backward, which walks from the front too, takes the sums behind
// a sample as total - front - own and returns G_i = d dist / d w_i = (2/3) dt0_i w_i + 2 (m_i (W_<i - W_>i) + (WM_>i - WM_<i)); `acc` is
// then the running sum of G_j w_j in front of the step, and Gw_incl the one including the lane's sample: sum_{j>i} G_j w_j =
// 2 dist - Gw_incl, because sum_j G_j w_j = 2 dist (dist is homogeneous of degree 2 in w) — the forward's output supplies the total.
struct OtDist { float W, WM, acc; };
__device__ __forceinline__ void ot_dist_front(OtDist &d, float w, float wm, uint32_t lane, float &Wb, float &WMb) {
    const float iw = wave_incl_sum(w, (int)lane), iwm = wave_incl_sum(wm, (int)lane);
    float ew = __shfl_up(iw, 1, 64), ewm = __shfl_up(iwm, 1, 64);       // the sums in front of the lane, within the step
    if (lane == 0) { ew = 0.0f; ewm = 0.0f; }
    Wb = d.W + ew; WMb = d.WM + ewm;
    d.W += __shfl(iw, 63, 64); d.WM += __shfl(iwm, 63, 64);
}
__device__ __forceinline__ void ot_dist_fwd_step(OtDist &d, float w, float m, float dt0, uint32_t lane) {
    float Wb, WMb;
    ot_dist_front(d, w, w * m, lane, Wb, WMb);
    d.acc += (1.0f / 3.0f) * dt0 * (w * w) + 2.0f * (w * (m * Wb - WMb));
}
__device__ __forceinline__ float ot_dist_bwd_step(OtDist &d, float w, float m, float dt0, float W_total, float WM_total, uint32_t lane, float &Gw_incl) {
    const float wm = w * m;
    float Wb, WMb;
    ot_dist_front(d, w, wm, lane, Wb, WMb);
    const float Wa = (W_total - Wb) - w, WMa = (WM_total - WMb) - wm;
    const float G = (2.0f / 3.0f) * dt0 * w + 2.0f * (m * (Wb - Wa) + (WMa - WMb));
    Gw_incl = d.acc + wave_incl_sum(G * w, (int)lane);
    d.acc = __shfl(Gw_incl, 63, 64);
    return G;
}

// ---------------------------------------------------------------- depth gradient (include/focnerf.h foc_occ_tail_backward_depth)
// depth = clamp(depth_raw - near, 0) / (far - near), depth_raw = sum_i w_i t_i over the samples that count (t_i = the forward's tsum). Per ray
// s = d loss / d depth_raw: the forward's own clamp branch (the gradient passes at exactly 0, as torch.clamp(min=0) does), 0 on a ray with
// !(far > near). Per sample grad_sigma_i / dt0_i gains s (T_after_i t_i - (depth_raw - D_acc_i)), D_acc_i = sum_{j<=i} w_j t_j: the colour
// term of ot_grad_acc with t in the colour's place, one wave scan and a carry (D_carry: the sum in front of the step, moved behind it).
__device__ __forceinline__ float ot_depth_scale(float depth_raw, float near, float far, float grad_depth) {
    return (depth_raw - near < 0.0f || !(far > near)) ? 0.0f : grad_depth / (far - near);
}
__device__ __forceinline__ float ot_depth_bwd_step(float &D_carry, float s, float w, float t, float T_after, float depth_raw, uint32_t lane) {
    const float D_acc = D_carry + wave_incl_sum(w * t, (int)lane);
    D_carry = __shfl(D_acc, 63, 64);
    return s * fmaf(T_after, t, -(depth_raw - D_acc));
}
