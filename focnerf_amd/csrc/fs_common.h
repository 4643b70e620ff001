// fs_common.h — the fixed-step sample positions and composite steps, shared by fixedstep.hip (sample generation, heads, tails),
// fixedcull.hip (occupancy cull) and combine.hip (the multi-object composite): one definition of a sample's depth, of its clipped position,
// of its row in the block-interleaved order, of the per-sample (z, delta, oz), of the transmittance scan and of the two backward steps, so
// that the files — and a fused tail and the plain kernels it replaces — produce the same bits.
#pragma once
#include "common.h"
#include "sample_math.h"

struct FsGeom { float near, far, span, sample_dist, step; };

// Block-interleaved sample order of the inference path (k_fs_sample): rows of 64 consecutive rays interleaved by depth.
#define FS_RAY_BLOCK 64u
__host__ __device__ __forceinline__ uint64_t fs_block_row(uint32_t n, uint32_t i, uint32_t T) {
    return (uint64_t)(n / FS_RAY_BLOCK) * FS_RAY_BLOCK * T + (uint64_t)i * FS_RAY_BLOCK + n % FS_RAY_BLOCK;
}

__device__ __forceinline__ FsGeom fs_geom(const float *__restrict__ nears, const float *__restrict__ fars, uint32_t n, uint32_t T) {
    FsGeom g;
    g.near = nears[n]; g.far = fars[n];
    g.span = g.far - g.near;
    g.sample_dist = g.span / (float)T;
    g.step = 1.0f / (float)(T - 1);
    return g;
}
// torch.linspace(0, 1, T) as torch's DEVICE kernel fills it: symmetric halves, and the upper half `end - step*k` is one
// fused multiply-add (the device compilers — nvcc for the reference, hipcc for torch-ROCm — contract it; torch's CPU kernel
// and therefore the CPU oracle round twice). Then z = near + span * lin [+ (u - 0.5) * sample_dist], separate torch ops.
__device__ __forceinline__ float fs_z0(const FsGeom &g, uint32_t i, uint32_t T) {
    const float lin = (i < T / 2) ? (g.step * (float)i) : fmaf(-g.step, (float)(T - 1 - i), 1.0f);
    return g.near + g.span * lin;
}
__device__ __forceinline__ float fs_jitter(const FsGeom &g, float z, float u) { return z + (u - 0.5f) * g.sample_dist; }
// with the sample's noise draw loaded here (a null `noise`: none) ...
__device__ __forceinline__ float fs_z(const FsGeom &g, uint32_t i, uint32_t T, const float *__restrict__ noise, uint64_t s) {
    float z = fs_z0(g, i, T);
    if (noise) z = fs_jitter(g, z, noise[s]);
    return z;
}
// ... and with the draw u already in a register (jitter = false: no jitter term at all, u unused)
__device__ __forceinline__ float fs_zu(const FsGeom &g, uint32_t i, uint32_t T, bool jitter, float u) {
    float z = fs_z0(g, i, T);
    if (jitter) z = fs_jitter(g, z, u);
    return z;
}

// Sample i of a ray as the composites see it: depth z, distance to the next sample delta (the last one: sample_dist) and the depth
// output's oz = clamp((z - near) / span, 0, 1), which keeps NaN (0/0 on rays that miss the box) like torch.clamp. ic = i on lanes that
// hold a sample, T - 1 on the others. u0 / u1 are the draws of samples ic and i + 1 AS REGISTER VALUES: the tail kernels load both
// unconditionally up front so that all loads of an iteration are in flight together — behind `if (noise)` / `if (i + 1 < T)` each load
// was its own round trip (s_waitcnt vmcnt(0) after every one of them).
struct FsSample { float z, delta, oz; };
__device__ __forceinline__ FsSample fs_sample(const FsGeom &g, uint32_t i, uint32_t ic, uint32_t T, bool jitter, float u0, float u1) {
    FsSample p;
    p.z = fs_zu(g, ic, T, jitter, u0);
    p.delta = g.sample_dist;
    if (i + 1 < T) p.delta = fs_zu(g, i + 1, T, jitter, u1) - p.z;
    p.oz = (p.z - g.near) / g.span;
    p.oz = p.oz < 0.0f ? 0.0f : (p.oz > 1.0f ? 1.0f : p.oz);
    return p;
}
// for the kernels that take `noise` as a run-time pointer: the draws loaded where they are needed (s = the row of sample ic)
__device__ __forceinline__ FsSample fs_sample_ld(const FsGeom &g, uint32_t i, uint32_t ic, uint32_t T, const float *__restrict__ noise, uint64_t s) {
    const bool jitter = noise != nullptr;
    return fs_sample(g, i, ic, T, jitter, jitter ? noise[s] : 0.0f, jitter && i + 1 < T ? noise[s + 1] : 0.0f);
}

// The transmittance scan of one 64-sample step: om = 1 - alpha + 1e-15 on the lanes that hold a sample, 1 on the others. Returns the
// transmittance BEFORE the lane's sample and moves the carry Tc behind the step.
__device__ __forceinline__ float fs_trans_scan(float om, uint32_t lane, float &Tc) {
    float P;
    const float Tb = Tc * wave_prod_scan(om, lane, P);
    Tc *= __shfl(P, 63, 64);
    return Tb;
}

// reverse (suffix) inclusive sum across the wave
__device__ __forceinline__ float wave_suffix_incl_sum(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_down(v, o, 64);
        if (lane + o < 64) v += u;
    }
    return v;
}
// The density head's backward for one 64-sample step, walked from the ray's end (k_fs_head_bwd, k_fs_tail_bwd): gi = the gradient of the
// lane's weight without the depth's share, gdp = grad_depth of the ray; S_carry = sum of g_j w_j over the samples behind this step, moved
// in front of it here. Returns d/d sigma through weights -> alpha -> sigma.
__device__ __forceinline__ float fs_head_bwd_step(const FsSample &p, bool valid, float sigma, float Tb, float gi, float gdp, float density_scale, uint32_t lane,
                                                  float &S_carry) {
    const float ex = expf((-p.delta * density_scale) * sigma);          // 1 - alpha
    const float alpha = 1 - ex;
    const float om = 1 - alpha + 1e-15f;
    if (gdp != 0.0f) gi += gdp * p.oz;
    const float gw_i = valid ? gi * (alpha * Tb) : 0.0f;                // g_i * w_i
    const float incl = wave_suffix_incl_sum(gw_i, (int)lane);
    const float S_i = S_carry + (incl - gw_i);                          // strictly after i
    const float dalpha = gi * Tb - S_i / om;
    S_carry += __shfl(incl, 0, 64);
    return dalpha * (p.delta * density_scale) * ex;
}

// ---------------------------------------------------------------- ray distortion (include/focnerf.h foc_fixed_tail_forward_dist)
// dist = sum_i (1/3) delta_i w_i^2 + 2 sum_i w_i (m_i W_<i - WM_<i), W_<i = sum_{j<i} w_j, WM_<i = sum_{j<i} w_j m_j: the interval midpoint
// m_i = (z_i - near) + delta_i / 2 and the interval delta_i of the FsSample, the raw weight. One 64-sample step: the two running sums by
// wave scan (W, WM = their values in front of the step, moved behind it), the lane's own terms added to `acc` (summed over the wave by
// the caller at the end). w = 0 on lanes without a sample. The backward walks from the ray's end, so there W / WM are the sums BEHIND the
// step and the sums in front of a sample are total - behind - own; it returns G_i = d dist / d w_i =
// (2/3) delta_i w_i + 2 (m_i (W_<i - W_>i) + (WM_>i - WM_<i)).
struct FsDist { float W, WM, acc; };
__device__ __forceinline__ float fs_dist_m(const FsGeom &g, const FsSample &p) { return (p.z - g.near) + 0.5f * p.delta; }
__device__ __forceinline__ void fs_dist_fwd_step(FsDist &d, float w, float m, float delta, uint32_t lane) {
    const float wm = w * m;
    const float iw = wave_incl_sum(w, (int)lane), iwm = wave_incl_sum(wm, (int)lane);
    float ew = __shfl_up(iw, 1, 64), ewm = __shfl_up(iwm, 1, 64);       // the sums in front of the lane, within the step
    if (lane == 0) { ew = 0.0f; ewm = 0.0f; }
    const float Wb = d.W + ew, WMb = d.WM + ewm;
    d.acc += (1.0f / 3.0f) * delta * (w * w) + 2.0f * (w * (m * Wb - WMb));
    d.W += __shfl(iw, 63, 64); d.WM += __shfl(iwm, 63, 64);
}
__device__ __forceinline__ float fs_dist_bwd_step(FsDist &d, float w, float m, float delta, float W_total, float WM_total, uint32_t lane) {
    const float wm = w * m;
    const float iw = wave_suffix_incl_sum(w, (int)lane), iwm = wave_suffix_incl_sum(wm, (int)lane);
    float ew = __shfl_down(iw, 1, 64), ewm = __shfl_down(iwm, 1, 64);   // the sums behind the lane, within the step
    if (lane == 63) { ew = 0.0f; ewm = 0.0f; }
    const float Wa = d.W + ew, WMa = d.WM + ewm;
    const float Wb = (W_total - Wa) - w, WMb = (WM_total - WMa) - wm;
    d.W += __shfl(iw, 0, 64); d.WM += __shfl(iwm, 0, 64);
    return (2.0f / 3.0f) * delta * w + 2.0f * (m * (Wb - Wa) + (WMa - WMb));
}

// The composite's backward for one sample (k_fs_composite_bwd, k_fs_tail_bwd): returns the gradient of its weight and sets o0 = columns
// 0..7 of its grad_c row (rgb logits in 0..2 where the weight passes the threshold, zeros otherwise). cc -> the sample's rgb logits,
// read above the threshold only.
struct FsRayGrad { float g0, g1, g2; FocBg bg; };
__device__ __forceinline__ FsRayGrad fs_ray_grad(const float *__restrict__ grad_image, const float *__restrict__ bg_ray, float bg_scalar, uint32_t n) {
    return FsRayGrad{grad_image[n * 3], grad_image[n * 3 + 1], grad_image[n * 3 + 2], foc_bg(bg_ray, bg_scalar, n)};
}
__device__ __forceinline__ float fs_composite_bwd_sample(const FsRayGrad &q, float w, float thresh, const _Float16 *cc, h8 &o0) {
    float gw = -(q.g0 * q.bg.b0 + q.g1 * q.bg.b1 + q.g2 * q.bg.b2);
#pragma unroll
    for (int k = 0; k < 8; k++) o0[k] = (_Float16)0;
    if (w > thresh) {
        const uint2 raw = *reinterpret_cast<const uint2 *>(cc);
        const _Float16 *y = reinterpret_cast<const _Float16 *>(&raw);
        const float y0 = foc_sigmoid_h((float)y[0]), y1 = foc_sigmoid_h((float)y[1]), y2 = foc_sigmoid_h((float)y[2]);
        gw += q.g0 * y0 + q.g1 * y1 + q.g2 * y2;
        o0[0] = foc_f2h(q.g0 * w * y0 * (1 - y0)); o0[1] = foc_f2h(q.g1 * w * y1 * (1 - y1)); o0[2] = foc_f2h(q.g2 * w * y2 * (1 - y2));
    }
    return gw;
}

// torch: rays_o + rays_d * z (two kernels, two roundings), then min(max(., aabb_lo), aabb_hi)
struct FsBox { float a0, a1, a2, a3, a4, a5; };
__device__ __forceinline__ FsBox fs_box(const float *__restrict__ aabb) { return FsBox{aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5]}; }
__device__ __forceinline__ void fs_point(float ox, float oy, float oz, float dx, float dy, float dz, float z, const FsBox &b, float &x, float &y, float &w) {
    x = ox + dx * z; y = oy + dy * z; w = oz + dz * z;
    x = fminf(fmaxf(x, b.a0), b.a3); y = fminf(fmaxf(y, b.a1), b.a4); w = fminf(fmaxf(w, b.a2), b.a5);
}
// the GridEncoder's normalised input (grid.py:149): (x + bound) / (2 bound)
__device__ __forceinline__ float fs_norm(float x, float bound, float two_b) { return (x + bound) / two_b; }

// ---------------------------------------------------------------- inference tail, one 64-sample tile of one ray
struct FsRayAcc { float Tc, ws, dp, r, g, b; };

// The inference path's own weight of the lane's sample, w = alpha * transmittance in front of it (the carry Tc moves behind the step):
// what masks an object's rgb in fs_infer_tile and in the combine fed from culled lists (combine.hip k_combine_culled).
__device__ __forceinline__ float fs_infer_weight(float &Tc, const FsSample &p, bool valid, float sigma, float density_scale, uint32_t lane) {
    const float alpha = valid ? 1 - expf((-p.delta * density_scale) * sigma) : 0.0f;
    const float om = valid ? (1 - alpha + 1e-15f) : 1.0f;
    return alpha * fs_trans_scan(om, lane, Tc);
}

// 64 samples of ray n, sample i on the lane (sigma / c0..c2 are that sample's values; unread where i >= T): weights by wave scan, the
// masked sums on the lane, the per-sample outputs written ray-major.
template <bool PACK>
__device__ __forceinline__ void fs_infer_tile(FsRayAcc &a, const FsGeom &g, uint32_t n, uint32_t i, uint32_t lane, uint32_t T, float sigma, float c0, float c1,
                                              float c2, const float *__restrict__ noise, float density_scale, float thresh, float *__restrict__ rgb_masked,
                                              float4 *__restrict__ field4, float *__restrict__ sigma_rm) {
    const bool valid = i < T;
    const uint64_t s = (uint64_t)n * T + (valid ? i : T - 1);
    const FsSample p = fs_sample_ld(g, i, valid ? i : T - 1, T, noise, s);
    const float w = fs_infer_weight(a.Tc, p, valid, sigma, density_scale, lane);
    if (valid) {
        a.ws += w; a.dp += w * p.oz;
        const bool on = w > thresh;
        if (on) { a.r += w * c0; a.g += w * c1; a.b += w * c2; }
        if (rgb_masked) { rgb_masked[s * 3] = on ? c0 : 0.0f; rgb_masked[s * 3 + 1] = on ? c1 : 0.0f; rgb_masked[s * 3 + 2] = on ? c2 : 0.0f; }
        if (PACK) field4[s] = make_float4(sigma, on ? c0 : 0.0f, on ? c1 : 0.0f, on ? c2 : 0.0f);
        if (sigma_rm) sigma_rm[s] = sigma;
    }
}
