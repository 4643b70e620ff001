// occtrain.hip — the tail of the occupancy-grid TRAINING path (legacy/nerf/renderer.py:256-322) on ragged sample lists.
//
// What the caller's torch glue evaluates between the colour network and the loss, as one kernel per direction, one wave per ray:
//     sigma = density_scale * trunc_exp(h[:, 0])                      (network_ff.py:60, activation.py:8-18; legacy renderer :300)
//     rgb   = sigmoid(c[:, 0:3])                                      (network_ff.py:73, a half tensor: rounded to fp16)
//     weights_sum, depth, image = composite_rays_train(sigma, rgb, deltas, rays, T_thresh)     (raymarching.cu:500-588)
//     image = image + (1 - weights_sum) * bg_color                    (:313)
//     depth = clamp(depth - nears, min=0) / (fars - nears)            (:314, no gradient)
// and their derivatives (raymarching.cu:601-693; trunc_exp's g * exp(clamp(x, -15, 15)); the half sigmoid's g (1 - y) y).
// h [M,16] fp16 is the density network's output, c [M,c_width] fp16 the colour network's (c_width 4: rgb logits + one pad column,
// the form foc_color_head_forward / _backward exchange; 16: the padded FFMLP output). Per sample and lane the arithmetic is the shared
// definitions k_head_fwd / k_rgb_fwd / k_composite_train_fwd are written in (sample_math.h, ragged.h ot_step), so the forward values are the
// bits of the three-kernel chain; sigma [M], rgbs [M,3] and their gradients are never stored (4 x 16 B per sample and direction).
//
// The backward writes EVERY row of grad_c and grad_h0: a ray's wave covers the ray's whole slot range (zeros behind the sample at which
// the ray became opaque, zeros for a ray that did not fit the list), and the rows behind the last ray's range are zeroed by spare
// waves — the colour network's backward reads all M rows, and the caller's zero fill of them was a launch of its own.
//
// Below the kernels: the whole training node as one call each way (foc_occ_train_forward / _backward, their _pad31 and _obj forms, and the
// _tail pair that carries the distortion and depth buffers beside the node). One forward and one backward sequence serve every layout of
// the colour input; the entry points differ in their checks only.
#include "common.h"
#include "sample_math.h"     // foc_sigmoid_h, foc_trunc_exp_bwd, foc_bg, h8
#include "ragged.h"          // ot_ray, ot_step, ot_grad_acc: the composite, shared with k_composite_train_fwd / _bwd
#include "mlp_common.h"      // host: the colour-input layouts' shared bodies (field_forward_train, color_head_forward / _backward), head_layer_pair

#define OT_PAD_BLOCKS 64u

// CRIT (foc_occ_tail_forward_sumsq): also ray_sumsq[ray] = sum of exp(h0)^2 over ALL of the ray's samples, those behind the sample at
// which the composite stopped included (0 for a ray that did not fit): lane l sums samples l, l + 64, ... in order, then one wave_sum.
// DIST (foc_occ_tail_forward_dist): also ray_dist[ray] = the ray's distortion and ray_wm[ray] = sum w m over the samples that count (ragged.h
// ot_dist_fwd_step; both 0 for a ray that did not fit); every other output is the bits of the instantiation without it.
// DEPTH (foc_occ_tail_forward_depth): also depth_raw[ray] = sum w t, the `d` below before `depth` is normalised (0 for a ray that did not fit):
// what the backward's depth term needs beside nears / fars.
template <bool CRIT, bool DIST, bool DEPTH>
__global__ void __launch_bounds__(256) k_occ_tail_fwd(const _Float16 *__restrict__ h, const _Float16 *__restrict__ c, uint32_t c_ld,
                                                      const float *__restrict__ deltas, const int32_t *__restrict__ rays, uint32_t M, uint32_t N,
                                                      float T_thresh, float density_scale, const float *__restrict__ bg_ray, float bg_scalar,
                                                      const float *__restrict__ nears, const float *__restrict__ fars,
                                                      float *__restrict__ weights_sum, float *__restrict__ image_raw, float *__restrict__ image,
                                                      float *__restrict__ depth, float *__restrict__ ray_sumsq, float *__restrict__ ray_dist,
                                                      float *__restrict__ ray_wm, float *__restrict__ depth_raw) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const OtRay ry = ot_ray(rays, n, M);
    float r = 0, g = 0, b = 0, ws = 0, d = 0, sq = 0;
    OtDist dist = {0, 0, 0};
    if (ry.fits) {
        float T_carry = 1.0f, t_carry = 0.0f;
        uint32_t base = 0;
        for (; base < ry.count; base += 64) {
            const uint32_t i = base + lane;
            const bool valid = i < ry.count;
            float sigma = 0, dt0 = 0, dt1 = 0, c0 = 0, c1 = 0, c2 = 0;
            if (valid) {
                const uint64_t s = (uint64_t)ry.offset + i;
                sigma = expf((float)h[s * 16]);                              // k_head_fwd
                if constexpr (CRIT) sq = fmaf(sigma, sigma, sq);
                if (density_scale != 1.0f) sigma = density_scale * sigma;
                const float2 dl = *reinterpret_cast<const float2 *>(deltas + s * 2);
                dt0 = dl.x; dt1 = dl.y;
                const uint2 raw = *reinterpret_cast<const uint2 *>(c + s * c_ld);
                const _Float16 *cc = reinterpret_cast<const _Float16 *>(&raw);
                c0 = foc_sigmoid_h((float)cc[0]); c1 = foc_sigmoid_h((float)cc[1]); c2 = foc_sigmoid_h((float)cc[2]);      // k_rgb_fwd
            }
            const OtStep st = ot_step(valid, sigma, dt0, T_carry, T_thresh, lane);
            const float tsum = t_carry + wave_incl_sum(dt1, (int)lane);
            r = fmaf(st.w, c0, r); g = fmaf(st.w, c1, g); b = fmaf(st.w, c2, b);
            d = fmaf(st.w, tsum, d);
            ws += st.w;
            if constexpr (DIST) ot_dist_fwd_step(dist, st.w, tsum, dt0, lane);
            if (st.term) { base += 64; break; }
            T_carry = __shfl(st.T_after, 63, 64);
            t_carry = __shfl(tsum, 63, 64);
        }
        if constexpr (CRIT) {                                  // the samples behind the stop: the penalty is on the density, not on the composite
            for (; base < ry.count; base += 64) {
                if (base + lane < ry.count) { const float e = expf((float)h[((uint64_t)ry.offset + base + lane) * 16]); sq = fmaf(e, e, sq); }
            }
            sq = wave_sum(sq);
        }
        r = wave_sum(r); g = wave_sum(g); b = wave_sum(b); ws = wave_sum(ws); d = wave_sum(d);
        if constexpr (DIST) dist.acc = wave_sum(dist.acc);
    }
    if (lane == 0) {
        const uint32_t k = ry.index;
        weights_sum[k] = ws;
        image_raw[k * 3] = r; image_raw[k * 3 + 1] = g; image_raw[k * 3 + 2] = b;
        const float rest = 1 - ws;
        // `image + rest` for the default white background ((1 - w) * 1 is (1 - w)), `image + rest * bg` otherwise: the caller's two torch forms
        const FocBg bg = foc_bg(bg_ray, bg_scalar, k);
        image[k * 3] = r + rest * bg.b0; image[k * 3 + 1] = g + rest * bg.b1; image[k * 3 + 2] = b + rest * bg.b2;
        const float nr = nears[k], dd = d - nr;
        depth[k] = (dd < 0.0f ? 0.0f : dd) / (fars[k] - nr);
        if constexpr (CRIT) ray_sumsq[k] = sq;
        if constexpr (DIST) { ray_dist[k] = dist.acc; ray_wm[k] = dist.WM; }
        if constexpr (DEPTH) depth_raw[k] = d;
    }
}

// grad_image [N,3] (of the FINAL image), grad_ws [N] or NULL -> grad_c [M,c_ld] fp16, grad_h0 [M] fp16 (every row written).
// CRIT (foc_occ_tail_backward_sumsq): grad_sumsq [N] is the gradient of the forward's ray_sumsq; 2 exp(h0) grad_sumsq[ray] joins the
// density path before trunc_exp's factor on EVERY row of a ray that fits — the rows behind the stop carry that term alone.
// DIST (foc_occ_tail_backward_dist): grad_dist [N] is the gradient of the forward's ray_dist; with g = grad_dist[ray] and G_i = d dist / d w_i
// (ragged.h ot_dist_bwd_step) grad_sigma_i gains dt0_i (g G_i T_after_i - g sum_{j>i} G_j w_j) on the samples that count. Rows behind a stop
// and rays that did not fit get nothing from it; a ray whose grad_dist is 0 is the plain backward's bits.
// DEPTH (foc_occ_tail_backward_depth): grad_depth [N] is the gradient of the forward's normalised `depth`; with s = its share of depth_raw
// (ragged.h ot_depth_scale: 0 on a clamped ray) grad_sigma_i gains dt0_i s (T_after_i t_i - (depth_raw - D_acc_i)) on the samples that count
// (ot_depth_bwd_step). The dt1 load and the scan of t are DIST's when both are on. Rows behind a stop, rays that did not fit and rays with
// s == 0 get nothing from it: such a ray is the bits of the instantiation without DEPTH.
template <bool CRIT, bool DIST, bool DEPTH>
__global__ void __launch_bounds__(256) k_occ_tail_bwd(const float *__restrict__ grad_image, const float *__restrict__ grad_ws,
                                                      const _Float16 *__restrict__ h, const _Float16 *__restrict__ c, uint32_t c_ld,
                                                      const float *__restrict__ deltas, const int32_t *__restrict__ rays, const int32_t *__restrict__ counter,
                                                      const float *__restrict__ weights_sum, const float *__restrict__ image_raw, uint32_t M, uint32_t N,
                                                      float T_thresh, float density_scale, const float *__restrict__ bg_ray, float bg_scalar,
                                                      _Float16 *__restrict__ grad_c, _Float16 *__restrict__ grad_h0,
                                                      const float *__restrict__ grad_sumsq, const float *__restrict__ ray_wm,
                                                      const float *__restrict__ ray_dist, const float *__restrict__ grad_dist,
                                                      const float *__restrict__ nears, const float *__restrict__ fars,
                                                      const float *__restrict__ depth_raw, const float *__restrict__ grad_depth) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (blockIdx.x >= (N + 3u) / 4u) {
        // spare workgroups: the rows behind the last ray's slot range (the list is padded to a multiple of 128 rows, or sized by mean_count)
        const uint32_t total = (uint32_t)counter[0];
        const uint32_t pb = blockIdx.x - (N + 3u) / 4u;
        for (uint64_t s = (uint64_t)total + pb * 256u + threadIdx.x; s < M; s += (uint64_t)OT_PAD_BLOCKS * 256u) {
            grad_h0[s] = (_Float16)0;
            if (c_ld == 4) *reinterpret_cast<uint2 *>(grad_c + s * 4) = make_uint2(0u, 0u);
            else { *reinterpret_cast<uint4 *>(grad_c + s * 16) = make_uint4(0u, 0u, 0u, 0u); *reinterpret_cast<uint4 *>(grad_c + s * 16 + 8) = make_uint4(0u, 0u, 0u, 0u); }
        }
        return;
    }
    if (n >= N) return;
    const OtRay ry = ot_ray(rays, n, M);
    auto store = [&](uint64_t s, float gs, float q0, float q1, float q2) {
        grad_h0[s] = foc_f2h(gs);
        h8 o = {0, 0, 0, 0, 0, 0, 0, 0};
        o[0] = foc_f2h(q0); o[1] = foc_f2h(q1); o[2] = foc_f2h(q2);
        if (c_ld == 4) *reinterpret_cast<uint2 *>(grad_c + s * 4) = *reinterpret_cast<const uint2 *>(&o);
        else { *reinterpret_cast<h8 *>(grad_c + s * 16) = o; *reinterpret_cast<uint4 *>(grad_c + s * 16 + 8) = make_uint4(0u, 0u, 0u, 0u); }
    };
    if (!ry.fits) {                                            // its slots (the part of them that lies inside the list) carry no gradient
        const uint64_t end = min((uint64_t)ry.offset + ry.count, (uint64_t)M);
        for (uint64_t s = (uint64_t)ry.offset + lane; s < end; s += 64) store(s, 0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const uint32_t index = ry.index;
    // image = raw + (1 - ws) bg: the background term hands -(g . bg) to the opacity's gradient (white: -(g0 + g1 + g2), torch's sum over the channel axis)
    const FocBg bg = foc_bg(bg_ray, bg_scalar, index);
    const float g0 = grad_image[index * 3], g1 = grad_image[index * 3 + 1], g2 = grad_image[index * 3 + 2];
    const float gws = (grad_ws ? grad_ws[index] : 0.0f) - ((g0 * bg.b0 + g1 * bg.b1) + g2 * bg.b2);
    const OtRayGrad q = ot_ray_grad(grad_image, image_raw, weights_sum, index, gws);
    float gsq2 = 0.0f;
    if constexpr (CRIT) gsq2 = 2.0f * grad_sumsq[index];      // d(sum sigma^2) / d sigma = 2 sigma
    // the criterion's share of a row's grad_h0: 2 exp(x) grad_sumsq * exp(clamp(x, -15, 15))
    auto crit_only = [&](uint64_t s) {
        const float x = (float)h[s * 16], e = expf(x);
        return gsq2 * e * foc_trunc_exp_bwd(x, e);
    };
    float gdist = 0.0f, W_total = 0.0f, WM_total = 0.0f, dist2 = 0.0f, t_carry = 0.0f;
    OtDist dist = {0, 0, 0};
    if constexpr (DIST) { gdist = grad_dist[index]; W_total = weights_sum[index]; WM_total = ray_wm[index]; dist2 = 2.0f * ray_dist[index]; }
    float sdep = 0.0f, d_total = 0.0f, D_carry = 0.0f;
    if constexpr (DEPTH) { d_total = depth_raw[index]; sdep = ot_depth_scale(d_total, nears[index], fars[index], grad_depth[index]); }
    float T_carry = 1.0f;
    OtColour carry = {0, 0, 0};
    bool dead = false;                                         // wave-uniform: the ray became opaque in an earlier block of 64
    for (uint32_t base = 0; base < ry.count; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < ry.count;
        const uint64_t s = (uint64_t)ry.offset + (valid ? i : 0);
        if (dead) { if (valid) store(s, CRIT ? crit_only(s) : 0.0f, 0.0f, 0.0f, 0.0f); continue; }
        float sigma = 0, e0 = 0, dt0 = 0, dt1 = 0, c0 = 0, c1 = 0, c2 = 0, e_raw = 0;
        if (valid) {
            const float x = (float)h[s * 16];
            e_raw = expf(x);
            sigma = density_scale != 1.0f ? density_scale * e_raw : e_raw;
            if constexpr (DIST || DEPTH) { const float2 dl = *reinterpret_cast<const float2 *>(deltas + s * 2); dt0 = dl.x; dt1 = dl.y; }
            else dt0 = deltas[s * 2];
            const uint2 raw = *reinterpret_cast<const uint2 *>(c + s * c_ld);
            const _Float16 *cc = reinterpret_cast<const _Float16 *>(&raw);
            c0 = foc_sigmoid_h((float)cc[0]); c1 = foc_sigmoid_h((float)cc[1]); c2 = foc_sigmoid_h((float)cc[2]);
            e0 = foc_trunc_exp_bwd(x, e_raw);
        }
        const OtStep st = ot_step(valid, sigma, dt0, T_carry, T_thresh, lane);
        const OtColour acc = ot_running(carry, st.w, c0, c1, c2, lane);
        float dist_term = 0.0f;                                // g (G_i T_after_i - sum_{j>i} G_j w_j)
        float depth_term = 0.0f;                               // s (T_after_i t_i - sum_{j>i} w_j t_j)
        if constexpr (DIST || DEPTH) {
            if (gdist != 0.0f || sdep != 0.0f) {               // wave-uniform
                const float tsum = t_carry + wave_incl_sum(dt1, (int)lane);        // the forward's running t
                if constexpr (DIST) {
                    if (gdist != 0.0f) {
                        float Gw_incl;
                        const float G = ot_dist_bwd_step(dist, st.w, tsum, dt0, W_total, WM_total, lane, Gw_incl);
                        dist_term = gdist * (G * st.T_after - (dist2 - Gw_incl));
                    }
                }
                if constexpr (DEPTH) {
                    if (sdep != 0.0f) depth_term = ot_depth_bwd_step(D_carry, sdep, st.w, tsum, st.T_after, d_total, lane);
                }
                t_carry = __shfl(tsum, 63, 64);
            }
        }
        if (st.act) {
            // k_composite_train_bwd: grad_rgbs = g w; grad_sigmas = dt0 (...)
            float ga = ot_grad_acc(q, st.T_after, c0, c1, c2, acc);
            if constexpr (DIST) { if (gdist != 0.0f) ga += dist_term; }
            if constexpr (DEPTH) { if (sdep != 0.0f) ga += depth_term; }
            float gs = dt0 * ga;
            if (density_scale != 1.0f) gs = density_scale * gs;       // through `density_scale * sigmas`
            if constexpr (CRIT) gs = fmaf(gsq2, e_raw, gs);
            // k_rgb_bwd: half(g) (1 - y) y;  k_head_bwd: grad_sigma * exp(clamp(h0))
            const float q0 = (float)(_Float16)(g0 * st.w), q1 = (float)(_Float16)(g1 * st.w), q2 = (float)(_Float16)(g2 * st.w);
            store(s, gs * e0, q0 * (1.0f - c0) * c0, q1 * (1.0f - c1) * c1, q2 * (1.0f - c2) * c2);
        } else if (valid) store(s, CRIT ? gsq2 * e_raw * e0 : 0.0f, 0.0f, 0.0f, 0.0f);
        if (st.term) { dead = true; continue; }
        T_carry = __shfl(st.T_after, 63, 64);
        carry = ot_last(acc);
    }
}

extern "C" {

// ray_sumsq / grad_sumsq NULL: the plain kernels (foc_occ_tail_forward / _backward); `who` names the entry point in messages
static int occ_tail_forward(const char *who, const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N,
                            float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, const float *nears, const float *fars,
                            float *weights_sum, float *image_raw, float *image, float *depth, float *ray_sumsq, float *ray_dist, float *ray_wm, float *depth_raw,
                            void *stream) {
    FocDeviceGuard foc_guard_(stream, h);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(c_width == 16 || c_width == 4, FOC_E_INVALID, "%s: c_width must be 16 or 4 (got %u)", who, c_width);
    FOC_REQUIRE(rays && nears && fars && weights_sum && image_raw && image && depth && (M == 0 || (h && c && deltas)), FOC_E_INVALID, "%s: null pointer", who);
    static constexpr decltype(&k_occ_tail_fwd<false, false, false>) kerns[8] = {
                               k_occ_tail_fwd<false, false, false>, k_occ_tail_fwd<true, false, false>, k_occ_tail_fwd<false, true, false>,
                               k_occ_tail_fwd<true, true, false>,   k_occ_tail_fwd<false, false, true>, k_occ_tail_fwd<true, false, true>,
                               k_occ_tail_fwd<false, true, true>,   k_occ_tail_fwd<true, true, true>};
    auto kern = kerns[(ray_sumsq ? 1 : 0) + (ray_dist ? 2 : 0) + (depth_raw ? 4 : 0)];
    hipLaunchKernelGGL(kern, dim3(foc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream, (const _Float16 *)h,
                       (const _Float16 *)c, c_width, deltas, rays, M, N, T_thresh, density_scale, bg_ray, bg_scalar, nears, fars, weights_sum, image_raw, image, depth,
                       ray_sumsq, ray_dist, ray_wm, depth_raw);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

static int occ_tail_backward(const char *who, const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width, const float *deltas,
                             const int32_t *rays, const int32_t *counter, const float *weights_sum, const float *image_raw, uint32_t M, uint32_t N,
                             float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0, const float *grad_sumsq,
                             const float *ray_wm, const float *ray_dist, const float *grad_dist, const float *nears, const float *fars,
                             const float *depth_raw, const float *grad_depth, void *stream) {
    FocDeviceGuard foc_guard_(stream, grad_image);
    if (N == 0 || M == 0) return FOC_OK;
    FOC_REQUIRE(c_width == 16 || c_width == 4, FOC_E_INVALID, "%s: c_width must be 16 or 4 (got %u)", who, c_width);
    FOC_REQUIRE(grad_image && h && c && deltas && rays && counter && weights_sum && image_raw && grad_c && grad_h0, FOC_E_INVALID, "%s: null pointer", who);
    static constexpr decltype(&k_occ_tail_bwd<false, false, false>) kerns[8] = {
                               k_occ_tail_bwd<false, false, false>, k_occ_tail_bwd<true, false, false>, k_occ_tail_bwd<false, true, false>,
                               k_occ_tail_bwd<true, true, false>,   k_occ_tail_bwd<false, false, true>, k_occ_tail_bwd<true, false, true>,
                               k_occ_tail_bwd<false, true, true>,   k_occ_tail_bwd<true, true, true>};
    auto kern = kerns[(grad_sumsq ? 1 : 0) + (grad_dist ? 2 : 0) + (grad_depth ? 4 : 0)];
    hipLaunchKernelGGL(kern, dim3(foc_div_up(N, 4) + OT_PAD_BLOCKS), dim3(256), 0, (hipStream_t)stream, grad_image,
                       grad_ws, (const _Float16 *)h, (const _Float16 *)c, c_width, deltas, rays, counter, weights_sum, image_raw, M, N, T_thresh, density_scale, bg_ray,
                       bg_scalar, (_Float16 *)grad_c, (_Float16 *)grad_h0, grad_sumsq, ray_wm, ray_dist, grad_dist, nears, fars, depth_raw, grad_depth);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

int foc_occ_tail_forward(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N,
                         float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, const float *nears, const float *fars,
                         float *weights_sum, float *image_raw, float *image, float *depth, void *stream) {
    return occ_tail_forward("occ_tail_forward", h, c, c_width, deltas, rays, M, N, T_thresh, density_scale, bg_ray, bg_scalar, nears, fars, weights_sum, image_raw,
                            image, depth, nullptr, nullptr, nullptr, nullptr, stream);
}

int foc_occ_tail_backward(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width, const float *deltas,
                          const int32_t *rays, const int32_t *counter, const float *weights_sum, const float *image_raw, uint32_t M, uint32_t N,
                          float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0, void *stream) {
    return occ_tail_backward("occ_tail_backward", grad_image, grad_ws, h, c, c_width, deltas, rays, counter, weights_sum, image_raw, M, N, T_thresh, density_scale,
                             bg_ray, bg_scalar, grad_c, grad_h0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int foc_occ_tail_forward_sumsq(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N,
                               float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, const float *nears, const float *fars,
                               float *weights_sum, float *image_raw, float *image, float *depth, float *ray_sumsq, void *stream) {
    FOC_REQUIRE(ray_sumsq || N == 0, FOC_E_INVALID, "occ_tail_forward_sumsq: null ray_sumsq");
    return occ_tail_forward("occ_tail_forward_sumsq", h, c, c_width, deltas, rays, M, N, T_thresh, density_scale, bg_ray, bg_scalar, nears, fars, weights_sum,
                            image_raw, image, depth, ray_sumsq, nullptr, nullptr, nullptr, stream);
}

int foc_occ_tail_backward_sumsq(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width, const float *deltas,
                                const int32_t *rays, const int32_t *counter, const float *weights_sum, const float *image_raw, uint32_t M, uint32_t N,
                                float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0,
                                const float *grad_sumsq, void *stream) {
    FOC_REQUIRE(grad_sumsq || N == 0 || M == 0, FOC_E_INVALID, "occ_tail_backward_sumsq: null grad_sumsq");
    return occ_tail_backward("occ_tail_backward_sumsq", grad_image, grad_ws, h, c, c_width, deltas, rays, counter, weights_sum, image_raw, M, N, T_thresh,
                             density_scale, bg_ray, bg_scalar, grad_c, grad_h0, grad_sumsq, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

// the two tails with the ray distortion (include/focnerf.h); ray_sumsq / grad_sumsq may be NULL: with or without the criterion
int foc_occ_tail_forward_dist(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N,
                              float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, const float *nears, const float *fars,
                              float *weights_sum, float *image_raw, float *image, float *depth, float *ray_sumsq, float *ray_dist, float *ray_wm, void *stream) {
    FOC_REQUIRE((ray_dist && ray_wm) || N == 0, FOC_E_INVALID, "occ_tail_forward_dist: null ray_dist / ray_wm");
    return occ_tail_forward("occ_tail_forward_dist", h, c, c_width, deltas, rays, M, N, T_thresh, density_scale, bg_ray, bg_scalar, nears, fars, weights_sum,
                            image_raw, image, depth, ray_sumsq, ray_dist, ray_wm, nullptr, stream);
}

int foc_occ_tail_backward_dist(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width, const float *deltas,
                               const int32_t *rays, const int32_t *counter, const float *weights_sum, const float *image_raw, uint32_t M, uint32_t N,
                               float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0,
                               const float *grad_sumsq, const float *ray_wm, const float *ray_dist, const float *grad_dist, void *stream) {
    FOC_REQUIRE(!grad_dist || (ray_wm && ray_dist) || N == 0 || M == 0, FOC_E_INVALID, "occ_tail_backward_dist: grad_dist needs ray_wm and ray_dist");
    return occ_tail_backward("occ_tail_backward_dist", grad_image, grad_ws, h, c, c_width, deltas, rays, counter, weights_sum, image_raw, M, N, T_thresh,
                             density_scale, bg_ray, bg_scalar, grad_c, grad_h0, grad_sumsq, ray_wm, ray_dist, grad_dist, nullptr, nullptr, nullptr, nullptr, stream);
}

// the supersets of the pairs above (include/focnerf.h): every extra output / incoming gradient optional, the depth's among them
int foc_occ_tail_forward_depth(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays, uint32_t M, uint32_t N,
                               float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, const float *nears, const float *fars,
                               float *weights_sum, float *image_raw, float *image, float *depth, float *ray_sumsq, float *ray_dist, float *ray_wm,
                               float *depth_raw, void *stream) {
    FOC_REQUIRE((ray_dist != nullptr) == (ray_wm != nullptr), FOC_E_INVALID, "occ_tail_forward_depth: ray_dist and ray_wm come together");
    return occ_tail_forward("occ_tail_forward_depth", h, c, c_width, deltas, rays, M, N, T_thresh, density_scale, bg_ray, bg_scalar, nears, fars, weights_sum,
                            image_raw, image, depth, ray_sumsq, ray_dist, ray_wm, depth_raw, stream);
}

int foc_occ_tail_backward_depth(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width, const float *deltas,
                                const int32_t *rays, const int32_t *counter, const float *weights_sum, const float *image_raw, uint32_t M, uint32_t N,
                                float T_thresh, float density_scale, const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0,
                                const float *grad_sumsq, const float *ray_wm, const float *ray_dist, const float *grad_dist, const float *nears,
                                const float *fars, const float *depth_raw, const float *grad_depth, void *stream) {
    FOC_REQUIRE(!grad_dist || (ray_wm && ray_dist) || N == 0 || M == 0, FOC_E_INVALID, "occ_tail_backward_depth: grad_dist needs ray_wm and ray_dist");
    FOC_REQUIRE(!grad_depth || (depth_raw && nears && fars) || N == 0 || M == 0, FOC_E_INVALID,
                "occ_tail_backward_depth: grad_depth needs depth_raw, nears and fars");
    return occ_tail_backward("occ_tail_backward_depth", grad_image, grad_ws, h, c, c_width, deltas, rays, counter, weights_sum, image_raw, M, N, T_thresh,
                             density_scale, bg_ray, bg_scalar, grad_c, grad_h0, grad_sumsq, ray_wm, ray_dist, grad_dist, nears, fars, depth_raw, grad_depth, stream);
}

// ---------------------------------------------------------------- the node as one call each way
// ONE sequence each way for the three layouts of the colour input (mlp_common.h MlpHead): plain (32 wide, last column 0), pad31 (32 wide,
// column 31 = input_pad: network_tcnn_legacy.py) and object-conditioned (48 wide, obj_feat [16], column 47 = input_pad: network_foc.py,
// network_tcnn.py). Sequencing only: each step is the body of the public entry point a caller would have called itself, with its own
// argument checks and device guard. The six exported entry points at the end run their own checks, all before the first launch.
static int ot_check_node(const FocOccTrainNode *n, const char *who) {
    FOC_REQUIRE(n != nullptr, FOC_E_INVALID, "%s: null node", who);
    FOC_REQUIRE(n->struct_bytes == (uint32_t)sizeof(FocOccTrainNode), FOC_E_INVALID, "%s: node of %u bytes, this library's FocOccTrainNode has %zu", who,
                n->struct_bytes, sizeof(FocOccTrainNode));
    FOC_REQUIRE(n->cap > 0 && n->n_rays > 0, FOC_E_INVALID, "%s: empty node (cap %u, rays %u): nothing to sequence, call nothing", who, n->cap, n->n_rays);
    FOC_REQUIRE(n->grid_workspace && n->grid_workspace_bytes && n->offsets_host, FOC_E_INVALID, "%s: the binned encoder backward's workspace is required", who);
    return FOC_OK;
}

static int ot_check_pad31(const FocOccTrainNode *n, float input_pad, const char *who) {
    FOC_REQUIRE(input_pad == 0.0f || head_layer_pair(n->sigma_layers, n->color_layers), FOC_E_INVALID,
                "%s: a pad needs (sigma_layers, color_layers) in (1,2), (1,3), (2,2), (2,3), (3,3) (got %u, %u)", who, n->sigma_layers, n->color_layers);
    return FOC_OK;
}

// the shapes of the kernel that runs both networks (csrc/field_fwd.hip)
static bool ot_whole_field(const FocOccTrainNode *n) {
    return n->sigma_input_dim == 32 && n->sigma_hidden == 64 && n->color_hidden == 64 && head_layer_pair(n->sigma_layers, n->color_layers) &&
           n->sigma_activation == n->color_activation && (n->sigma_activation == 0 || n->sigma_activation == 6) && n->sigma_output_activation == 6;
}

// the companion of an object-conditioned network (FocOccTrainObject beside the node)
static int ot_check_object(const FocOccTrainNode *n, const FocOccTrainObject *ob, const char *who) {
    int rc = ot_check_node(n, who);
    if (rc != FOC_OK) return rc;
    FOC_REQUIRE(ob != nullptr, FOC_E_INVALID, "%s: null object", who);
    FOC_REQUIRE(ob->struct_bytes == (uint32_t)sizeof(FocOccTrainObject), FOC_E_INVALID, "%s: object of %u bytes, this library's FocOccTrainObject has %zu", who,
                ob->struct_bytes, sizeof(FocOccTrainObject));
    FOC_REQUIRE(ob->obj_feat || ob->input_pad == 0.0f, FOC_E_INVALID, "%s: a pad (column 47 = %g) needs an object feature, obj_feat is NULL", who, (double)ob->input_pad);
    FOC_REQUIRE(ob->obj_feat, FOC_E_INVALID, "%s: obj_feat is NULL (a network without an object feature takes foc_occ_train_forward / _backward)", who);
    FOC_REQUIRE(head_layer_pair(n->sigma_layers, n->color_layers), FOC_E_INVALID,
                "%s: (sigma_layers, color_layers) must be in (1,2), (1,3), (2,2), (2,3), (3,3) (got %u, %u)", who, n->sigma_layers, n->color_layers);
    FOC_REQUIRE(ot_whole_field(n), FOC_E_INVALID,
                "%s: the object node serves 32 -> 64 density and 48 -> 64 colour networks with one hidden activation, relu(0) or none(6)", who);
    return FOC_OK;
}

// march -> counted encode -> both networks (one kernel, or sigma MLP + colour head) -> tail. ray_sumsq [n_rays] or NULL: the tail that
// also sums sigma^2 per ray. tail (FocOccTrainTail beside the node) or NULL: the tail that also returns the distortion and / or depth_raw.
static int occ_train_forward(const FocOccTrainNode *n, const void *obj_feat, float input_pad, bool pad31, float *ray_sumsq, const FocOccTrainTail *tail,
                             void *stream) {
    const uint32_t M = n->cap;
    int rc = foc_march_rays_train_field(n->rays_o, n->rays_d, n->bitfield, n->bound, n->dt_gamma, n->max_steps, n->n_rays, n->cascade, n->grid_size, M, n->nears,
                                        n->fars, n->enc_in, n->sh_rows, n->deltas, n->rays, n->counter, n->jitter, n->march_scratch, n->pad_align, n->aabb, n->min_near,
                                        stream);
    if (rc != FOC_OK) return rc;
    rc = foc_grid_encode_forward_counted(n->enc_in, n->embeddings, n->offsets, n->planes, M, 3, 2, n->levels, n->per_level_scale_log2, n->base_resolution, n->gridtype,
                                         n->align_corners, n->interp, n->table_dtype, n->offsets_host, n->grid_workspace, n->grid_workspace_bytes, stream);
    if (rc != FOC_OK) return rc;
    // both networks in one kernel when the shapes are FOC's (csrc/field_fwd.hip: bit for bit the two calls below). The plain layout takes
    // that kernel from two sigma layers on; one sigma hidden layer ((1, 2), (1, 3)) came with the pad31 and object layouts.
    if (ot_whole_field(n) && (n->sigma_layers > 1 || pad31 || obj_feat) && foc_opt(FOC_OPT_FIELD_FWD_FUSED)) {
        rc = field_forward_train(n->planes, n->w_sigma, n->sigma_layers, n->sh_rows, 1, n->w_color, n->color_layers, 64, n->sigma_activation, M, n->h, n->c,
                                 n->c_width, obj_feat, input_pad, pad31, stream);
        if (rc != FOC_OK) return rc;
    } else {
        rc = foc_ffmlp_forward_planar(n->planes, n->w_sigma, M, n->sigma_input_dim, 16, n->sigma_hidden, n->sigma_layers, n->sigma_activation, n->sigma_output_activation,
                                      n->h, stream);
        if (rc != FOC_OK) return rc;
        rc = color_head_forward(n->h, n->sh_rows, 1, n->w_color, M, n->color_hidden, n->color_layers, n->color_activation, n->c, n->c_width, obj_feat, input_pad, pad31,
                                stream);
        if (rc != FOC_OK) return rc;
    }
    return occ_tail_forward(tail ? "occ_tail_forward_depth" : ray_sumsq ? "occ_tail_forward_sumsq" : "occ_tail_forward", n->h, n->c, n->c_width, n->deltas, n->rays,
                            M, n->n_rays, n->T_thresh, n->density_scale, n->bg_ray, n->bg_scalar, n->nears, n->fars, n->weights_sum, n->image_raw, n->image, n->depth,
                            ray_sumsq, tail ? tail->ray_dist : nullptr, tail ? tail->ray_wm : nullptr, tail ? tail->depth_raw : nullptr, stream);
}

// tail -> colour head -> sigma MLP -> binned encoder backward. grad_sumsq [n_rays] or NULL: the gradient of the forward's ray_sumsq;
// grad_obj [16] fp32 or NULL: the object feature's gradient. tail or NULL: the gradients of the distortion and / or the depth.
static int occ_train_backward(const FocOccTrainNode *n, const void *obj_feat, float input_pad, bool pad31, const float *grad_sumsq, float *grad_obj,
                              const FocOccTrainTail *tail, void *stream) {
    const uint32_t M = n->cap;
    const float *grad_dist = tail ? tail->grad_dist : nullptr, *grad_depth = tail ? tail->grad_depth : nullptr;
    int rc = occ_tail_backward(tail ? "occ_tail_backward_depth" : grad_sumsq ? "occ_tail_backward_sumsq" : "occ_tail_backward", n->grad_image, n->grad_ws, n->h, n->c,
                               n->c_width, n->deltas, n->rays, n->counter, n->weights_sum, n->image_raw, M, n->n_rays, n->T_thresh, n->density_scale, n->bg_ray,
                               n->bg_scalar, n->grad_c, n->grad_h0, grad_sumsq, grad_dist ? tail->ray_wm : nullptr, grad_dist ? tail->ray_dist : nullptr, grad_dist,
                               grad_depth ? n->nears : nullptr, grad_depth ? n->fars : nullptr, grad_depth ? tail->depth_raw : nullptr, grad_depth, stream);
    if (rc != FOC_OK) return rc;
    rc = color_head_backward(n->grad_c, n->h, n->sh_rows, 1, n->grad_h0, n->w_color, M, n->color_hidden, n->color_layers, n->color_activation, n->grad_h,
                             n->grad_w_color, n->mlp_workspace, n->mlp_workspace_bytes, n->c_width, obj_feat, grad_obj, input_pad, pad31, stream);
    if (rc != FOC_OK) return rc;
    rc = foc_ffmlp_backward_planar(n->grad_h, n->planes, n->w_sigma, M, n->sigma_input_dim, 16, n->sigma_hidden, n->sigma_layers, n->sigma_activation,
                                   n->sigma_output_activation, 1, n->grad_planes, n->grad_w_sigma, n->mlp_workspace, n->mlp_workspace_bytes, stream);
    if (rc != FOC_OK) return rc;
    return (n->precounted ? foc_grid_encode_backward_binned_counted : foc_grid_encode_backward_binned)(
        n->grad_planes, n->enc_in, n->embeddings, n->offsets, n->grad_embeddings, M, 3, 2, n->levels, n->per_level_scale_log2, n->base_resolution, nullptr, nullptr,
        n->gridtype, n->align_corners, n->interp, n->table_dtype, 0, n->offsets_host, n->grid_workspace, n->grid_workspace_bytes, stream);
}

int foc_occ_train_forward(const FocOccTrainNode *n, void *stream) {
    const int rc = ot_check_node(n, "occ_train_forward");
    return rc != FOC_OK ? rc : occ_train_forward(n, nullptr, 0.0f, false, nullptr, nullptr, stream);
}

int foc_occ_train_backward(const FocOccTrainNode *n, void *stream) {
    const int rc = ot_check_node(n, "occ_train_backward");
    return rc != FOC_OK ? rc : occ_train_backward(n, nullptr, 0.0f, false, nullptr, nullptr, nullptr, stream);
}

// column 31 of the 32-wide colour input holds input_pad (the legacy tinycudann layout)
int foc_occ_train_forward_pad31(const FocOccTrainNode *n, float input_pad, void *stream) {
    int rc = ot_check_node(n, "occ_train_forward_pad31");
    if (rc == FOC_OK) rc = ot_check_pad31(n, input_pad, "occ_train_forward_pad31");
    return rc != FOC_OK ? rc : occ_train_forward(n, nullptr, input_pad, true, nullptr, nullptr, stream);
}

int foc_occ_train_backward_pad31(const FocOccTrainNode *n, float input_pad, void *stream) {
    int rc = ot_check_node(n, "occ_train_backward_pad31");
    if (rc == FOC_OK) rc = ot_check_pad31(n, input_pad, "occ_train_backward_pad31");
    return rc != FOC_OK ? rc : occ_train_backward(n, nullptr, input_pad, true, nullptr, nullptr, nullptr, stream);
}

// the 48-wide colour head of an object-conditioned network: the feature, its pad (column 47) and the sums of sigma^2 travel in `ob`
int foc_occ_train_forward_obj(const FocOccTrainNode *n, const FocOccTrainObject *ob, void *stream) {
    const int rc = ot_check_object(n, ob, "occ_train_forward_obj");
    return rc != FOC_OK ? rc : occ_train_forward(n, ob->obj_feat, ob->input_pad, false, ob->ray_sumsq, nullptr, stream);
}

int foc_occ_train_backward_obj(const FocOccTrainNode *n, const FocOccTrainObject *ob, void *stream) {
    const int rc = ot_check_object(n, ob, "occ_train_backward_obj");
    if (rc != FOC_OK) return rc;
    FOC_REQUIRE(n->mlp_workspace_bytes >= foc_ffmlp_backward_workspace_bytes(48, 64, n->color_layers), FOC_E_INVALID,
                "occ_train_backward_obj: MLP workspace of %llu bytes, the 48-wide colour head asks for foc_ffmlp_backward_workspace_bytes(48, 64, %u) = %llu",
                (unsigned long long)n->mlp_workspace_bytes, n->color_layers, (unsigned long long)foc_ffmlp_backward_workspace_bytes(48, 64, n->color_layers));
    return occ_train_backward(n, ob->obj_feat, ob->input_pad, false, ob->grad_sumsq, ob->grad_obj, nullptr, stream);
}

// The node with the tail's optional per-ray outputs (FocOccTrainTail beside it): one pair for the three layouts. object NULL: the plain
// layout (input_pad 0) or column 31 = input_pad; else the object's own pad, input_pad is not read.
static int ot_check_tail(const FocOccTrainNode *n, const FocOccTrainObject *ob, float input_pad, const FocOccTrainTail *tail, const char *who) {
    int rc = ob ? ot_check_object(n, ob, who) : ot_check_node(n, who);
    if (rc == FOC_OK && !ob) rc = ot_check_pad31(n, input_pad, who);
    if (rc != FOC_OK) return rc;
    FOC_REQUIRE(tail != nullptr, FOC_E_INVALID, "%s: null tail (a node without the tail's extra outputs takes foc_occ_train_forward / _backward and their twins)", who);
    FOC_REQUIRE(tail->struct_bytes == (uint32_t)sizeof(FocOccTrainTail), FOC_E_INVALID, "%s: tail of %u bytes, this library's FocOccTrainTail has %zu", who,
                tail->struct_bytes, sizeof(FocOccTrainTail));
    FOC_REQUIRE((tail->ray_dist != nullptr) == (tail->ray_wm != nullptr), FOC_E_INVALID, "%s: ray_dist and ray_wm come together", who);
    return FOC_OK;
}

int foc_occ_train_forward_tail(const FocOccTrainNode *n, const FocOccTrainObject *ob, float input_pad, const FocOccTrainTail *tail, void *stream) {
    const int rc = ot_check_tail(n, ob, input_pad, tail, "occ_train_forward_tail");
    if (rc != FOC_OK) return rc;
    return ob ? occ_train_forward(n, ob->obj_feat, ob->input_pad, false, ob->ray_sumsq, tail, stream)
              : occ_train_forward(n, nullptr, input_pad, input_pad != 0.0f, nullptr, tail, stream);
}

int foc_occ_train_backward_tail(const FocOccTrainNode *n, const FocOccTrainObject *ob, float input_pad, const FocOccTrainTail *tail, void *stream) {
    const int rc = ot_check_tail(n, ob, input_pad, tail, "occ_train_backward_tail");
    if (rc != FOC_OK) return rc;
    FOC_REQUIRE(!tail->grad_dist || tail->ray_dist, FOC_E_INVALID, "occ_train_backward_tail: grad_dist needs ray_wm and ray_dist");
    FOC_REQUIRE(!tail->grad_depth || (tail->depth_raw && n->nears && n->fars), FOC_E_INVALID, "occ_train_backward_tail: grad_depth needs depth_raw, nears and fars");
    if (!ob) return occ_train_backward(n, nullptr, input_pad, input_pad != 0.0f, nullptr, nullptr, tail, stream);
    FOC_REQUIRE(n->mlp_workspace_bytes >= foc_ffmlp_backward_workspace_bytes(48, 64, n->color_layers), FOC_E_INVALID,
                "occ_train_backward_tail: MLP workspace of %llu bytes, the 48-wide colour head asks for foc_ffmlp_backward_workspace_bytes(48, 64, %u) = %llu",
                (unsigned long long)n->mlp_workspace_bytes, n->color_layers, (unsigned long long)foc_ffmlp_backward_workspace_bytes(48, 64, n->color_layers));
    return occ_train_backward(n, ob->obj_feat, ob->input_pad, false, ob->grad_sumsq, ob->grad_obj, tail, stream);
}

} // extern "C"
