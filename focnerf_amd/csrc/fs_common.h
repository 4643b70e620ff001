// fs_common.h — the fixed-step sample positions, shared by fixedstep.hip (sample generation, tails) and fixedcull.hip (occupancy cull):
// one definition of a sample's depth, of its clipped position and of its row in the block-interleaved order, so that the two files
// produce the same bits.
#pragma once
#include "common.h"

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
__device__ __forceinline__ float fs_z(const FsGeom &g, uint32_t i, uint32_t T, const float *__restrict__ noise, uint64_t s) {
    const float lin = (i < T / 2) ? (g.step * (float)i) : fmaf(-g.step, (float)(T - 1 - i), 1.0f);
    float z = g.near + g.span * lin;
    if (noise) z = z + (noise[s] - 0.5f) * g.sample_dist;
    return z;
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

// 64 samples of ray n, sample i on the lane (sigma / c0..c2 are that sample's values; unread where i >= T): weights by wave scan, the
// masked sums on the lane, the per-sample outputs written ray-major.
template <bool PACK>
__device__ __forceinline__ void fs_infer_tile(FsRayAcc &a, const FsGeom &g, uint32_t n, uint32_t i, uint32_t lane, uint32_t T, float sigma, float c0, float c1,
                                              float c2, const float *__restrict__ noise, float density_scale, float thresh, float *__restrict__ rgb_masked,
                                              float4 *__restrict__ field4, float *__restrict__ sigma_rm) {
    const bool valid = i < T;
    const uint64_t s = (uint64_t)n * T + (valid ? i : T - 1);
    const float z = fs_z(g, valid ? i : T - 1, T, noise, s);
    float delta = g.sample_dist;
    if (i + 1 < T) delta = fs_z(g, i + 1, T, noise, s + 1) - z;
    const float alpha = valid ? 1 - expf((-delta * density_scale) * sigma) : 0.0f;
    const float om = valid ? (1 - alpha + 1e-15f) : 1.0f;
    const float P = wave_incl_prod(om, (int)lane);
    float Pex = __shfl_up(P, 1, 64);
    if (lane == 0) Pex = 1.0f;
    const float w = alpha * (a.Tc * Pex);
    if (valid) {
        float oz = (z - g.near) / g.span;
        oz = oz < 0.0f ? 0.0f : (oz > 1.0f ? 1.0f : oz);
        a.ws += w; a.dp += w * oz;
        const bool on = w > thresh;
        if (on) { a.r += w * c0; a.g += w * c1; a.b += w * c2; }
        if (rgb_masked) { rgb_masked[s * 3] = on ? c0 : 0.0f; rgb_masked[s * 3 + 1] = on ? c1 : 0.0f; rgb_masked[s * 3 + 2] = on ? c2 : 0.0f; }
        if (PACK) field4[s] = make_float4(sigma, on ? c0 : 0.0f, on ? c1 : 0.0f, on ? c2 : 0.0f);
        if (sigma_rm) sigma_rm[s] = sigma;
    }
    a.Tc *= __shfl(P, 63, 64);
}
