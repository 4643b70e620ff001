// raymarching.hip — gfx950 kernels behind the _raymarching entry points of include/focnerf.h.
//
// Semantics follow raymarching/src/raymarching.cu of the reference (line cites per kernel);
// the kernels themselves are organised for CDNA4:
//   * marching is split into count -> ordered scan -> write, so slot reservation is a
//     deterministic prefix sum in ray order instead of the reference's atomicAdd race
//     (raymarching.cu:405-406);
//   * train-time compositing runs ONE WAVE PER RAY: 64 consecutive samples are loaded
//     coalesced, transmittance is a wave product-scan (DPP shuffles), early termination
//     is a ballot, the per-ray sums are wave reductions — instead of the reference's one
//     thread walking its own ray segment (uncoalesced, 128 rays per block).
// Every form of the march (one ray per lane, one wave per ray, 16 lanes per ray, two phases, staged in LDS) has to emit the reference's
// samples bit for bit, so what they share is defined once and they are written in terms of it:
//   RmRay / rm_load_ray (o, d, 1 / d); rm_dt, rm_start (the step clamp(t dt_gamma, dt_min, dt_max), the jittered start of a walk); rm_pos,
//   rm_cell, rm_skip_target, rm_skip (clamped position, cell lookup, voxel exit, the walk over an empty cell); rm_train_range (near / far of a
//   training ray, both count kernels); rm_lattice<DPP, COUNT, MED3> (the general step of the t lattice on 64 lanes, k_march_count_wave's slow
//   path, or on 16, rm_row_walk); rm_lane_walk<BAIL, DIRS> (THE serial loop: k_march_rays, k_march_rays_first, k_march_walkers and, into LDS,
//   k_march_rays_staged); RmSlots / rm_put_sample (where a walk's samples go, the record of one); rm_zero_row (k_march_emit); RmAcc,
//   rm_acc_load, rm_composite_sample, rm_composite_finish (k_composite_rays, k_composite_rays_pre); rm_scan_1024 (k_march_scan, k_compact_scan);
//   on the host rm_check_grid, rm_launch_row, rm_launch_lane (the grid refusals and the two launches the R9 entry points share).
// Floating-point policy: compiled with -ffp-contract=off; fused multiply-adds are written
// as explicit fmaf() exactly where oracle/oracle.c has them, so the marching control flow
// (and therefore every sample index and position) is bit-identical to the oracle.
#include "common.h"
#include "occ_cell.h"
#include "sample_math.h"
#include "ragged.h"
#include <float.h>

#define RM_SQRT3 1.7320508075688772f
#define RM_RPI   0.3183098861837907f

__device__ __forceinline__ float rm_sign(float x) { return copysignf(1.0f, x); }

// ---------------------------------------------------------------- R1 (raymarching.cu:92-145)
// slab test of one ray against the box a[0..5]; a miss gives FLT_MAX twice
__device__ __forceinline__ void rm_near_far(float ox, float oy, float oz, float dx, float dy, float dz, float a0, float a1, float a2, float a3, float a4, float a5,
                                            float min_near, float &near_out, float &far_out) {
    const float rdx = 1 / dx, rdy = 1 / dy, rdz = 1 / dz;
    float near = (a0 - ox) * rdx, far = (a3 - ox) * rdx, t;
    if (near > far) { t = near; near = far; far = t; }
    float near_y = (a1 - oy) * rdy, far_y = (a4 - oy) * rdy;
    if (near_y > far_y) { t = near_y; near_y = far_y; far_y = t; }
    bool miss = (near > far_y || near_y > far);
    if (!miss) {
        if (near_y > near) near = near_y;
        if (far_y < far) far = far_y;
        float near_z = (a2 - oz) * rdz, far_z = (a5 - oz) * rdz;
        if (near_z > far_z) { t = near_z; near_z = far_z; far_z = t; }
        miss = (near > far_z || near_z > far);
        if (!miss) {
            if (near_z > near) near = near_z;
            if (far_z < far) far = far_z;
            if (near < min_near) near = min_near;
        }
    }
    near_out = miss ? FLT_MAX : near;
    far_out = miss ? FLT_MAX : far;
}

__global__ void __launch_bounds__(256) k_near_far_from_aabb(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                     const float *__restrict__ aabb, uint32_t N, float min_near,
                                     float *__restrict__ nears, float *__restrict__ fars) {
    const float a0 = aabb[0], a1 = aabb[1], a2 = aabb[2], a3 = aabb[3], a4 = aabb[4], a5 = aabb[5];
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        float near, far;
        rm_near_far(rays_o[n * 3], rays_o[n * 3 + 1], rays_o[n * 3 + 2], rays_d[n * 3], rays_d[n * 3 + 1], rays_d[n * 3 + 2], a0, a1, a2, a3, a4, a5, min_near, near, far);
        nears[n] = near;
        fars[n] = far;
    }
}

// ---------------------------------------------------------------- R2 (raymarching.cu:163-198)
__global__ void __launch_bounds__(256) k_sph_from_ray(const float *__restrict__ rays_o, const float *__restrict__ rays_d, float radius,
                               uint32_t N, float *__restrict__ coords) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const float ox = rays_o[n * 3], oy = rays_o[n * 3 + 1], oz = rays_o[n * 3 + 2];
        const float dx = rays_d[n * 3], dy = rays_d[n * 3 + 1], dz = rays_d[n * 3 + 2];
        const float A = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const float B = fmaf(oz, dz, fmaf(oy, dy, ox * dx));
        const float C = fmaf(-radius, radius, fmaf(oz, oz, fmaf(oy, oy, ox * ox)));
        const float t = (-B + sqrtf(fmaf(B, B, -(A * C)))) / A;
        const float x = fmaf(t, dx, ox), y = fmaf(t, dy, oy), z = fmaf(t, dz, oz);
        const float theta = atan2f(sqrtf(fmaf(z, z, x * x)), y);
        const float phi = atan2f(z, x);
        coords[n * 2] = fmaf(2 * theta, RM_RPI, -1.0f);
        coords[n * 2 + 1] = phi * RM_RPI;
    }
}

// ---------------------------------------------------------------- R3/R4 (raymarching.cu:214-254)
__global__ void __launch_bounds__(256) k_morton3D(const int32_t *__restrict__ coords, uint32_t N, int32_t *__restrict__ indices) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x)
        indices[n] = (int32_t)rm_morton3D((uint32_t)coords[n * 3], (uint32_t)coords[n * 3 + 1], (uint32_t)coords[n * 3 + 2]);
}
__global__ void __launch_bounds__(256) k_morton3D_invert(const int32_t *__restrict__ indices, uint32_t N, int32_t *__restrict__ coords) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        const int32_t ind = indices[n];
        coords[n * 3] = (int32_t)rm_morton3D_invert((uint32_t)(ind >> 0));
        coords[n * 3 + 1] = (int32_t)rm_morton3D_invert((uint32_t)(ind >> 1));
        coords[n * 3 + 2] = (int32_t)rm_morton3D_invert((uint32_t)(ind >> 2));
    }
}

// ---------------------------------------------------------------- R5 (raymarching.cu:267-289)
// One thread packs 32 cells (8 x float4 loads, 128 B contiguous per lane) into one dword, so a
// wave streams 8 KiB per iteration and stores 256 contiguous bytes.
__global__ void __launch_bounds__(256) k_packbits_x4(const float4 *__restrict__ grid4, uint32_t N4, float thresh,
                              uint32_t *__restrict__ bitfield4) {
    for (uint32_t n = blockIdx.x * blockDim.x + threadIdx.x; n < N4; n += gridDim.x * blockDim.x) {
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const float4 v = grid4[(uint64_t)n * 8 + q];
            bits |= (v.x > thresh ? 1u : 0u) << (q * 4 + 0);
            bits |= (v.y > thresh ? 1u : 0u) << (q * 4 + 1);
            bits |= (v.z > thresh ? 1u : 0u) << (q * 4 + 2);
            bits |= (v.w > thresh ? 1u : 0u) << (q * 4 + 3);
        }
        bitfield4[n] = bits;
    }
}
__global__ void __launch_bounds__(256) k_packbits_tail(const float *__restrict__ grid, uint32_t n0, uint32_t N, float thresh,
                                uint8_t *__restrict__ bitfield) {
    for (uint32_t n = n0 + blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
        uint32_t bits = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) bits |= (grid[(uint64_t)n * 8 + i] > thresh ? 1u : 0u) << i;
        bitfield[n] = (uint8_t)bits;
    }
}

// ---------------------------------------------------------------- marching core
// One cell lookup (raymarching.cu:361-379 == :429-448 == :752-770).
struct RmCell { float x, y, z, dt, mip_bound; int nx, ny, nz; };

struct RmParams {
    float bound, dt_gamma, dt_min, dt_max, rH, H3, Hf, Cf, Hm1;
    uint32_t H;
    float norm_inv;                    // 0: sample positions leave as they are; else they leave as (x + bound) * norm_inv, the encoder's [0,1] coordinates
    int rederive;                      // != 0: after every emitted sample t continues from last_t + (t - last_t), the value composite_rays hands to the NEXT call
                                       // (raymarching.cu:871, 899) — a burst of k samples then marches what k calls of one sample would (see foc_march_rays_two_phase)
    int gamma_pow2;                    // dt_gamma is a power of two (1/128, the reference's default for its scenes): t * dt_gamma is exact, so t + t * dt_gamma
                                       // rounds once — it IS fmaf(t, dt_gamma, t)
};
// position of an emitted sample as it is stored (the native render step asks for the normalised form: csrc/occrender.hip)
__device__ __forceinline__ float rm_out(const RmParams &p, float x) { return p.norm_inv != 0.0f ? (x + p.bound) * p.norm_inv : x; }

// One ray as every walk holds it: origin, direction, 1 / direction (the voxel exit needs it; where no walk skips, as in k_march_emit, the compiler drops it).
struct RmRay { float ox, oy, oz, dx, dy, dz, rdx, rdy, rdz; };
template <typename I>                                      // (the row index keeps its caller's type: uint32_t ray number or int list entry)
__device__ __forceinline__ RmRay rm_load_ray(const float *__restrict__ rays_o, const float *__restrict__ rays_d, I i) {
    RmRay r;
    r.ox = rays_o[i * 3]; r.oy = rays_o[i * 3 + 1]; r.oz = rays_o[i * 3 + 2];
    r.dx = rays_d[i * 3]; r.dy = rays_d[i * 3 + 1]; r.dz = rays_d[i * 3 + 2];
    r.rdx = 1 / r.dx; r.rdy = 1 / r.dy; r.rdz = 1 / r.dz;
    return r;
}
// the step at t (raymarching.cu:371 == :385 == :397) and the jittered start of a walk (:357)
__device__ __forceinline__ float rm_dt(const RmParams &p, float t) { return rm_clamp(t * p.dt_gamma, p.dt_min, p.dt_max); }
__device__ __forceinline__ float rm_start(const RmParams &p, float t, float noise) { return fmaf(rm_dt(p, t), noise, t); }
// clamped position of the ray at t
__device__ __forceinline__ void rm_pos(const RmParams &p, const RmRay &r, float t, float &x, float &y, float &z) {
    x = rm_clamp(fmaf(t, r.dx, r.ox), -p.bound, p.bound);
    y = rm_clamp(fmaf(t, r.dy, r.oy), -p.bound, p.bound);
    z = rm_clamp(fmaf(t, r.dz, r.oz), -p.bound, p.bound);
}

__device__ __forceinline__ bool rm_cell(const uint8_t *__restrict__ grid, const RmParams &p, const RmRay &r, float t, RmCell &c) {
    rm_pos(p, r, t, c.x, c.y, c.z);
    c.dt = rm_dt(p, t);
    // mip_from_pos / mip_from_dt (:42-54): float min/max, then truncation
    const int l1 = rm_mip_from_pos(c.x, c.y, c.z, p.Cf);
    const float mdt = (float)((double)(c.dt * p.Hf) * 0.5);
    const int l2 = (int)fminf(p.Cf - 1, fmaxf(0.0f, (float)rm_frexp_exp(mdt)));
    const int level = l1 > l2 ? l1 : l2;
    return rm_cell_bit(grid, rm_cell_index(c.x, c.y, c.z, level, p.bound, p.H, p.Hm1, p.H3, c.mip_bound, c.nx, c.ny, c.nz));
}

// Empty cell: jump to the voxel exit (:389-398).
__device__ __forceinline__ float rm_skip_target(const RmParams &p, const RmCell &c, float t, const RmRay &r) {
    const float tx = fmaf(fmaf(fmaf(0.5f, rm_sign(r.dx), (float)c.nx + 0.5f) * p.rH, 2.0f, -1.0f), c.mip_bound, -c.x) * r.rdx;
    const float ty = fmaf(fmaf(fmaf(0.5f, rm_sign(r.dy), (float)c.ny + 0.5f) * p.rH, 2.0f, -1.0f), c.mip_bound, -c.y) * r.rdy;
    const float tz = fmaf(fmaf(fmaf(0.5f, rm_sign(r.dz), (float)c.nz + 0.5f) * p.rH, 2.0f, -1.0f), c.mip_bound, -c.z) * r.rdz;
    return t + fmaxf(0.0f, fminf(tx, fminf(ty, tz)));
}

__device__ __forceinline__ float rm_skip(const RmParams &p, const RmCell &c, float t, const RmRay &r) {
    const float tt = rm_skip_target(p, c, t, r);
    do { t += rm_dt(p, t); } while (t < tt);
    return t;
}

static RmParams rm_make_params(float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H) {
    RmParams p;
    p.bound = bound; p.dt_gamma = dt_gamma;
    // same float expressions as raymarching.cu:345-346 (IEEE division on host == device)
    p.dt_min = 2 * RM_SQRT3 / (float)max_steps;
    p.dt_max = 2 * RM_SQRT3 * (float)(1 << (C - 1)) / (float)H;
    p.rH = 1 / (float)H;
    p.H3 = (float)(H * H * H);
    p.Hf = (float)H; p.Cf = (float)C; p.Hm1 = (float)(H - 1);
    p.H = H;
    p.norm_inv = 0.0f;
    p.rederive = 0;
    int e = 0;
    p.gamma_pow2 = (dt_gamma > 0.0f && frexpf(dt_gamma, &e) == 0.5f) ? 1 : 0;
    return p;
}

// The range of training ray n (both count kernels). aabb != NULL: nears / fars are OUTPUTS — the ray's slab test (k_near_far_from_aabb's
// expressions) is done here and written by the lanes with `writer` set.
__device__ __forceinline__ void rm_train_range(const RmRay &r, uint32_t n, const float *__restrict__ aabb, float min_near, bool writer,
                                               float *__restrict__ nears, float *__restrict__ fars, float &near, float &far) {
    if (aabb) {
        rm_near_far(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, aabb[0], aabb[1], aabb[2], aabb[3], aabb[4], aabb[5], min_near, near, far);
        if (writer) { nears[n] = near; fars[n] = far; }
    } else { near = nears[n]; far = fars[n]; }
}

// The general step of the lattice t_{j+1} = t_j + clamp(t_j dt_gamma, dt_min, dt_max) on COUNT lanes: every lane runs the recurrence from t_cur,
// each new value enters at the last lane of the wave (DPP 0x130, wave_shl:1) or of the 16-lane row (0x101, row_shl:1) while the earlier ones
// move down one lane, so after COUNT steps lane j holds T = t_j and every lane t_next = t_COUNT. MED3 (dt_min <= dt_max, any real setting):
// the clamp is one v_med3_f32 — for ordered operands the median IS fminf(hi, fmaxf(lo, x)), bit for bit.
template <int DPP, uint32_t COUNT, bool MED3>
__device__ __forceinline__ void rm_lattice(const RmParams &p, float t_cur, float &T, float &t_next) {
    constexpr uint32_t UNROLL = COUNT > 16u ? 8u : COUNT;
    T = t_cur; t_next = t_cur;
#pragma unroll UNROLL
    for (uint32_t j = 0; j < COUNT; j++) {
        T = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, t_next), __builtin_bit_cast(int, T), DPP, 0xf, 0xf, false));
        const float raw = t_next * p.dt_gamma;
        t_next += MED3 ? __builtin_amdgcn_fmed3f(raw, p.dt_min, p.dt_max) : rm_clamp(raw, p.dt_min, p.dt_max);
    }
}

// ---------------------------------------------------------------- R6 pass 1: count (raymarching.cu:348-400)
__global__ void __launch_bounds__(64) k_march_count(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                              const uint8_t *__restrict__ grid, RmParams p, uint32_t max_steps, uint32_t N,
                              float *__restrict__ nears, float *__restrict__ fars,
                              const float *__restrict__ noises, int32_t *__restrict__ counts, float *__restrict__ tstrip,
                              const float *__restrict__ aabb, float min_near) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const RmRay r = rm_load_ray(rays_o, rays_d, n);
    float near_n, far;
    rm_train_range(r, n, aabb, min_near, true, nears, fars, near_n, far);
    float t = rm_start(p, near_n, noises[n]);
    uint32_t num_steps = 0;
    RmCell c;
    // The marching loop is a chain of dependent L2 lookups: running it a second time to write the samples (as the reference does,
    // raymarching.cu:415-479) doubles that latency-bound cost. The `t` of every emitted sample is kept in a per-ray strip instead
    // (max_steps floats per ray), from which k_march_emit rebuilds position, dt and the two deltas with the loop's own expressions.
    float *strip = tstrip + (uint64_t)n * max_steps;
    while (t < far && num_steps < max_steps) {
        if (rm_cell(grid, p, r, t, c)) { strip[num_steps] = t; num_steps++; t += c.dt; }
        else t = rm_skip(p, c, t, r);
    }
    counts[n] = (int32_t)num_steps;
}

// ---------------------------------------------------------------- R6 pass 1, one WAVE per ray
// The loop above is a chain of dependent cell lookups, one ray per lane: with 4096 rays that is 64 waves, each as slow as its longest
// ray (0.135 ms per training batch). But the values `t` can take do not depend on the occupancy grid at all: both branches advance it
// by t += clamp(t * dt_gamma, dt_min, dt_max) (:385 and :397), so every ray walks a fixed lattice t_0, t_1, ... and the grid only
// decides which lattice points are visited and which of those are emitted. Here a wave takes 64 consecutive lattice points of ONE ray
// (lane j = point j, generated with the loop's own expression), looks all 64 cells up at once, and then replays the loop's control
// flow on wave-uniform bit masks: an occupied visited point emits and moves to the next lane, an empty one moves to the first lane
// whose t is not below its voxel exit (carried into the next 64 points when there is none). Same visits, same emitted t, bit for bit.
#define RM_MAX_ROUNDS (1u << 22)                           // x 64 lattice points: far beyond any real ray; makes the loop finite whatever the inputs
template <bool MED3>                                       // dt_min <= dt_max (any real setting): the clamp of the recurrence is one v_med3_f32
__global__ void __launch_bounds__(256) k_march_count_wave(const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                              const uint8_t *__restrict__ grid, RmParams p, uint32_t max_steps, uint32_t N,
                              float *__restrict__ nears, float *__restrict__ fars,
                              const float *__restrict__ noises, int32_t *__restrict__ counts, float *__restrict__ tstrip,
                              const float *__restrict__ aabb, float min_near, const int32_t *__restrict__ counter_in) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (n >= N) return;                                    // whole wave
    // the emit pass does the slot reservation itself (k_march_emit<.., true>): it takes the counter's entry values from a snapshot behind the
    // counts, because its last workgroup overwrites the counter while others may not have started
    if (counter_in && n == 0 && lane == 0) { counts[N] = counter_in[0]; counts[N + 1] = counter_in[1]; }
    const RmRay r = rm_load_ray(rays_o, rays_d, n);
    float near_n, far;
    rm_train_range(r, n, aabb, min_near, lane == 0, nears, fars, near_n, far);        // (wave-uniform but for the writer)
    float t_cur = rm_start(p, near_n, noises[n]);
    float *strip = tstrip + (uint64_t)n * max_steps;
    uint32_t num_steps = 0;
    bool skipping = false;                                 // inside the do-while of an empty cell whose exit `skip_to` lies beyond the last 64 points
    float skip_to = 0.0f;
    for (uint32_t round = 0; round < RM_MAX_ROUNDS; round++) {
        // lane j: t_cur advanced j times. Every lane runs the same recurrence; each new value enters at lane 63 while the earlier
        // ones move down one lane (DPP wave_shl:1), so the 64th insertion leaves value j in lane j and costs one move per step.
        float T = t_cur, t_next = t_cur;
        // The step clamp(t dt_gamma, dt_min, dt_max) has three regimes and t only grows: a ray walks dt_min steps near the camera, then
        // t dt_gamma, then dt_max. A round that lies in ONE regime needs no clamp — its 64 steps are `t += dt_min`, `t += t dt_gamma`
        // (one fma when dt_gamma is a power of two) or `t += dt_max`, the same values bit for bit — which halves the instructions of the
        // recurrence (move + 1 instead of move + mul + med3 + add; the recurrence is half of this kernel's VALU work). The regime is
        // read off the round's first point and confirmed on its last one (lane 63 after the loop); a round that crosses a boundary —
        // at most two per ray — is generated again with the general step.
        bool fast = false;
        if constexpr (MED3) {
            const float raw0 = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t_cur * p.dt_gamma)));
            const int regime = raw0 <= p.dt_min ? 0 : (raw0 >= p.dt_max ? 2 : 1);
            if (regime == 0 || regime == 2) {
                const float step = regime == 0 ? p.dt_min : p.dt_max;
#pragma unroll 8
                for (uint32_t j = 0; j < 64; j++) {
                    T = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, t_next), __builtin_bit_cast(int, T), 0x130, 0xf, 0xf, false));
                    t_next += step;
                }
            } else if (p.gamma_pow2) {
#pragma unroll 8
                for (uint32_t j = 0; j < 64; j++) {
                    T = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, t_next), __builtin_bit_cast(int, T), 0x130, 0xf, 0xf, false));
                    t_next = fmaf(t_next, p.dt_gamma, t_next);
                }
            } else {
#pragma unroll 8
                for (uint32_t j = 0; j < 64; j++) {
                    T = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, t_next), __builtin_bit_cast(int, T), 0x130, 0xf, 0xf, false));
                    t_next += t_next * p.dt_gamma;
                }
            }
            // the last point the general step would have clamped: lattice point 63 (in lane 63 now)
            const float raw63 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, T), 63)) * p.dt_gamma;
            fast = regime == 0 ? raw63 <= p.dt_min : (regime == 2 ? true : raw63 <= p.dt_max);
        }
        if (!fast) rm_lattice<0x130, 64u, MED3>(p, t_cur, T, t_next);
        const uint64_t in_range = __ballot(T < far);
        uint32_t k = 0;                                    // lane of the lattice point the loop is at
        if (skipping) {
            const uint64_t landed = __ballot(!(T < skip_to));
            if (landed == 0ull) {
                if (!((in_range >> 63) & 1ull)) break;     // t only grows: wherever the skip lands, it is beyond `far`
                t_cur = t_next;
                continue;
            }
            k = (uint32_t)__builtin_ctzll(landed);
            skipping = false;
        }
        RmCell c;
        const bool occupied_here = rm_cell(grid, p, r, T, c);
        const float exit_here = rm_skip_target(p, c, T, r);
        const uint64_t emit_ok = __ballot(occupied_here) & in_range;
        uint64_t emitted = 0ull;
        uint32_t room = (uint32_t)__builtin_amdgcn_readfirstlane((int)(max_steps - num_steps));
        // The replay is scalar code — one iteration per visited point, ~50 of them per round in empty space — and the CU has ONE scalar unit
        // for its sixteen waves: the kernel was bound by it (SQ counters: 3970 scalar against 3040 vector instructions per wave, the
        // compiler's lowering of the loop with its `done` / `skipping` flags ran to ~40 scalar instructions per iteration). Hence the
        // spare form: in_range is a PREFIX mask (t only grows), so "the point is out of range" is k >= k_far; one exit code instead of
        // flags; the mask of the lanes above k as one shift; and the walk over empty points as a hand-written block.
        const uint32_t k_far = ~in_range ? (uint32_t)__builtin_ctzll(~in_range) : 64u;       // first lattice point at or beyond `far`
        int state = room == 0u ? 1 : 0;                    // 0: ran off the 64 points; 1: the loop of :359 ended (far / step cap); 2: a skip carries over
        uint32_t ks = (uint32_t)__builtin_amdgcn_readfirstlane((int)k);
        // (wave-uniform by construction; said again so that the block's scalar operands are scalar registers)
        const uint32_t k_far_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)k_far);
        const uint64_t emit_s = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(emit_ok >> 32)) << 32) |
                                (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)emit_ok);
        while (state == 0) {
            // Walk over EMPTY points until an occupied one, the end of the range or a skip that leaves the 64 points. Hand-written: nine
            // instructions per visited point (seven of them scalar) where the compiler's lowering of the same loop took about thirty.
            //   why 0: ks >= k_far      why 1: the point at ks is occupied      why 2: no point of this round lies at or beyond the voxel exit
            uint32_t why, tt_bits;
            uint64_t tmp;
            asm volatile("1:\n\t"
                         "s_cmp_ge_u32 %[k], %[kfar]\n\t"
                         "s_cbranch_scc1 2f\n\t"
                         "s_bitcmp1_b64 %[emit], %[k]\n\t"
                         "s_cbranch_scc1 3f\n\t"
                         "s_nop 3\n\t"                                      // SALU wrote %[k]: four wait states before it selects a lane
                         "v_readlane_b32 %[tt], %[exitv], %[k]\n\t"         // the voxel exit of the point at ks
                         "s_lshl_b64 %[tmp], -2, %[k]\n\t"                  // the lanes above ks: do { advance } while (t < tt) advances at least once
                         "v_cmp_ngt_f32_e32 vcc, %[tt], %[T]\n\t"           // !(tt > T) == !(T < tt)
                         "s_and_b64 %[tmp], vcc, %[tmp]\n\t"
                         "s_cbranch_scc0 4f\n\t"
                         "s_ff1_i32_b64 %[k], %[tmp]\n\t"
                         "s_branch 1b\n\t"
                         "2: s_mov_b32 %[why], 0\n\t"
                         "s_branch 5f\n\t"
                         "3: s_mov_b32 %[why], 1\n\t"
                         "s_branch 5f\n\t"
                         "4: s_mov_b32 %[why], 2\n\t"
                         "5:"
                         : [k] "+s"(ks), [tt] "=&s"(tt_bits), [tmp] "=&s"(tmp), [why] "=&s"(why)
                         : [kfar] "s"(k_far_s), [emit] "s"(emit_s), [exitv] "v"(exit_here), [T] "v"(T)
                         : "vcc", "scc");
            if (why == 0u) { state = ks >= 64u ? 0 : 1; break; }
            if (why == 2u) { state = 2; skip_to = __builtin_bit_cast(float, tt_bits); break; }
            // a run of occupied points: each emits and steps to its successor
            const uint64_t rest = ~(emit_s >> ks);         // bit 0 clear; for ks > 0 the bits shifted in end the run at lane 63
            uint32_t len = rest ? (uint32_t)__builtin_ctzll(rest) : 64u;
            len = (uint32_t)__builtin_amdgcn_readfirstlane((int)(len < room ? len : room));      // (uniform; a scalar register for the block above)
            emitted |= (len >= 64u ? ~0ull : ((1ull << len) - 1ull)) << ks;
            room -= len;
            ks += len;
            if (room == 0u) state = 1;                     // what the loop condition finds at its next test (:359)
        }
        skipping = state == 2;
        const bool done = state == 1;
        if ((emitted >> lane) & 1ull) strip[num_steps + (uint32_t)__builtin_popcountll(emitted & ((1ull << lane) - 1ull))] = T;
        num_steps += (uint32_t)__builtin_popcountll(emitted);
        if (done) break;
        t_cur = t_next;
    }
    if (lane == 0) counts[n] = (int32_t)num_steps;
}

// ---------------------------------------------------------------- R6 pass 2: ordered slot reservation
// One 1024-thread workgroup scans the N counts in ray order (each thread owns a contiguous
// chunk), writes rays[n] = (n, base + exclusive_prefix, count) and bumps the two counters —
// the deterministic stand-in for the atomicAdd pair of raymarching.cu:405-413.
// (the scan itself: rm_scan_1024, shared with the compaction's k_compact_scan)
struct RmScan { uint32_t lo, hi; int base; };              // this thread's chunk [lo, hi) of the values and the sum of all values before it
__device__ __forceinline__ RmScan rm_scan_1024(const int32_t *v, uint32_t n, int *total) {
    __shared__ int s_wave[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t per = (n + 1023) / 1024;
    RmScan sc;
    sc.lo = tid * per; sc.hi = min(n, sc.lo + per);
    int local = 0;
    for (uint32_t i = sc.lo; i < sc.hi; i++) local += v[i];
    const int incl = wave_incl_sum_i(local, (int)lane);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        int w = lane < 16 ? s_wave[lane] : 0;
        const int wi = wave_incl_sum_i(w, (int)lane);
        if (lane < 16) s_wave[lane] = wi - w;   // exclusive base per wave
        if (lane == 15) *total = wi;            // (one thread writes the sum of all values: to LDS or to memory, as the caller needs it)
    }
    __syncthreads();
    sc.base = s_wave[wave] + (incl - local);
    return sc;
}

__global__ void __launch_bounds__(1024) k_march_scan(const int32_t *__restrict__ counts, uint32_t N,
                                                     int32_t *__restrict__ rays, int32_t *__restrict__ counter) {
    __shared__ int s_total;
    const RmScan sc = rm_scan_1024(counts, N, &s_total);
    const int base0 = counter[0];
    const int ray0 = counter[1];
    int run = base0 + sc.base;
    for (uint32_t i = sc.lo; i < sc.hi; i++) {
        const int c = counts[i];
        const uint32_t r = i;   // rows in ray order; a non-zero counter[1] would index past rays[N,3] in the reference
        rays[r * 3] = (int32_t)i; rays[r * 3 + 1] = run; rays[r * 3 + 2] = c;
        run += c;
    }
    __syncthreads();
    if (threadIdx.x == 0) { counter[0] = base0 + s_total; counter[1] = ray0 + (int32_t)N; }
}

// ---------------------------------------------------------------- R6 pass 3: emit (raymarching.cu:415-479)
// One wave per ray, lane k = sample k: t_k from the strip; xyz = clamp(o + t d), dt = clamp(t dt_gamma) exactly as rm_cell forms them;
// deltas = (dt_k, (t_k + dt_k) - last_t) with last_t = t_{k-1} + dt_{k-1} (the start t for k = 0), as the loop accumulates them.
// Stores are contiguous across the wave (768 B of xyz per 64 samples).
// FIELD: the sample list in the layout the fused training path consumes (foc_march_rays_train_field) — `xyzs` receives the encoder's
// [0,1] coordinates (x + bound) * 1 / (2 bound) (rm_out), `dirs` is not written, and `sh` [M,16] fp16 receives each sample's degree-4
// SH row (the first k-chunk of the colour network's input, sample_math.h foc_sh16_h as k_head_fwd stores it): one row per sample of
// a ray, all equal. Every row of both arrays is written — rays that do not fit the list and the rows behind the last ray get zeros
// (spare workgroups; `counter` from k_march_scan) — so the caller needs no zero fill.
#define RM_PAD_BLOCKS 64u
// row s of the FIELD list that holds no sample
__device__ __forceinline__ void rm_zero_row(float *__restrict__ xyzs, float *__restrict__ deltas, _Float16 *__restrict__ sh, uint64_t s) {
    xyzs[s * 3] = 0.0f; xyzs[s * 3 + 1] = 0.0f; xyzs[s * 3 + 2] = 0.0f;
    deltas[s * 2] = 0.0f; deltas[s * 2 + 1] = 0.0f;
    *reinterpret_cast<uint4 *>(sh + s * 16) = make_uint4(0u, 0u, 0u, 0u); *reinterpret_cast<uint4 *>(sh + s * 16 + 8) = make_uint4(0u, 0u, 0u, 0u);
}
// SCAN (round 5): the ordered slot reservation of k_march_scan done HERE, by every workgroup for itself — a workgroup's rays start at the sum
// of the counts of all rays before them, 256 threads add those up (at most 16 384 ints, L2 resident) and the wave of ray n adds the counts of
// the workgroup's earlier rays: the same integers as the one-workgroup scan, with no launch of its own (8.6 us + a launch gap of the configs[2]
// step), no atomics and no ticket. The `rays` table is written here (lane 0 of each ray's wave), the counter by the workgroup of the last ray;
// the entry values of the counter come from the snapshot the count pass left behind the counts (`counts[N], counts[N + 1]`).
template <bool FIELD, bool SCAN>
__global__ void __launch_bounds__(256) k_march_emit(const float *__restrict__ rays_o, const float *__restrict__ rays_d, RmParams p, uint32_t max_steps,
                                                    uint32_t N, uint32_t M, const float *__restrict__ nears, const float *__restrict__ noises,
                                                    int32_t *__restrict__ rays, const float *__restrict__ tstrip,
                                                    float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                                                    _Float16 *__restrict__ sh, int32_t *__restrict__ counter, uint32_t pad_align,
                                                    const int32_t *__restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    uint32_t scan_point = 0, scan_steps = 0, scan_total = 0;
    if constexpr (SCAN) {
        __shared__ int s_part[4];
        const uint32_t first = min(blockIdx.x * 4u, N);            // spare workgroups (FIELD): all N rays lie before them
        int part = 0;
        for (uint32_t i = threadIdx.x; i < first; i += 256u) part += counts[i];
        part = wave_sum_i(part);
        if (lane == 0) s_part[threadIdx.x >> 6] = part;
        __syncthreads();
        const int before = s_part[0] + s_part[1] + s_part[2] + s_part[3];
        const int base0 = counts[N], ray0 = counts[N + 1];
        const uint32_t w = threadIdx.x >> 6;
        int mine = 0, earlier = 0, here = 0;
        for (uint32_t j = 0; j < 4u; j++) {
            const int cj = first + j < N ? counts[first + j] : 0;
            if (j < w) earlier += cj;
            if (j == w) mine = cj;
            here += cj;
        }
        scan_point = (uint32_t)(base0 + before + earlier);
        scan_steps = (uint32_t)mine;
        scan_total = (uint32_t)(base0 + before + (blockIdx.x * 4u < N ? here : 0));
        if (n < N && lane == 0) { rays[n * 3] = (int32_t)n; rays[n * 3 + 1] = (int32_t)scan_point; rays[n * 3 + 2] = mine; }
        if (blockIdx.x == (N + 3u) / 4u - 1u && threadIdx.x == 0) { counter[0] = (int32_t)scan_total; counter[1] = ray0 + (int32_t)N; }
    }
    if constexpr (FIELD) {
        if (blockIdx.x >= (N + 3u) / 4u) {
            // pad_align > 0: the caller cuts the list to the samples marched, rounded up like raymarching.py:226 — nothing behind that is read
            const uint32_t total = SCAN ? scan_total : (uint32_t)counter[0], pb = blockIdx.x - (N + 3u) / 4u;
            const uint64_t end = pad_align ? min((uint64_t)M, (uint64_t)total + (pad_align - total % pad_align)) : (uint64_t)M;
            for (uint64_t s = (uint64_t)total + pb * 256u + threadIdx.x; s < end; s += (uint64_t)RM_PAD_BLOCKS * 256u) rm_zero_row(xyzs, deltas, sh, s);
            return;
        }
    }
    if (n >= N) return;
    const uint32_t point_index = SCAN ? scan_point : (uint32_t)rays[n * 3 + 1];
    const uint32_t num_steps = SCAN ? scan_steps : (uint32_t)rays[n * 3 + 2];
    if (num_steps == 0) return;
    if (point_index + num_steps > M) {                             // raymarching.cu:413
        if constexpr (FIELD) {
            const uint64_t end = min((uint64_t)point_index + num_steps, (uint64_t)M);
            for (uint64_t s = (uint64_t)point_index + lane; s < end; s += 64) rm_zero_row(xyzs, deltas, sh, s);
        }
        return;
    }
    const RmRay r = rm_load_ray(rays_o, rays_d, n);        // (1 / d is not used here and not computed)
    const float t0 = rm_start(p, nears[n], noises[n]);
    const float *strip = tstrip + (uint64_t)n * max_steps;
    h8 sh0, sh1;
    if constexpr (FIELD) foc_sh16_h(r.dx, r.dy, r.dz, sh0, sh1);
    for (uint32_t k = lane; k < num_steps; k += 64) {
        const float t = strip[k];
        const float dt = rm_dt(p, t);
        float last_t = t0;
        if (k > 0) { const float tp = strip[k - 1]; last_t = tp + rm_dt(p, tp); }
        const uint64_t s = (uint64_t)point_index + k;
        float x, y, z;
        rm_pos(p, r, t, x, y, z);
        xyzs[s * 3] = rm_out(p, x); xyzs[s * 3 + 1] = rm_out(p, y); xyzs[s * 3 + 2] = rm_out(p, z);
        if constexpr (FIELD) { *reinterpret_cast<h8 *>(sh + s * 16) = sh0; *reinterpret_cast<h8 *>(sh + s * 16 + 8) = sh1; }
        else { dirs[s * 3] = r.dx; dirs[s * 3 + 1] = r.dy; dirs[s * 3 + 2] = r.dz; }
        deltas[s * 2] = dt;
        deltas[s * 2 + 1] = (t + dt) - last_t;
    }
}

// ---------------------------------------------------------------- R7 (raymarching.cu:500-577), one wave per ray; the step is ragged.h ot_step
__global__ void __launch_bounds__(256) k_composite_train_fwd(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                      const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                      uint32_t M, uint32_t N, float T_thresh,
                                      float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const OtRay ry = ot_ray(rays, n, M);
    const uint32_t index = ry.index;
    if (!ry.fits) {
        if (lane == 0) { weights_sum[index] = 0; depth[index] = 0; image[index * 3] = 0; image[index * 3 + 1] = 0; image[index * 3 + 2] = 0; }
        return;
    }
    float T_carry = 1.0f, t_carry = 0.0f;
    float r = 0, g = 0, b = 0, ws = 0, d = 0;
    for (uint32_t base = 0; base < ry.count; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < ry.count;
        float sigma = 0, dt0 = 0, dt1 = 0, c0 = 0, c1 = 0, c2 = 0;
        if (valid) {
            const uint64_t s = (uint64_t)ry.offset + i;
            sigma = sigmas[s];
            const float2 dl = *reinterpret_cast<const float2 *>(deltas + s * 2);
            dt0 = dl.x; dt1 = dl.y;
            c0 = rgbs[s * 3]; c1 = rgbs[s * 3 + 1]; c2 = rgbs[s * 3 + 2];
        }
        const OtStep st = ot_step(valid, sigma, dt0, T_carry, T_thresh, lane);
        const float tsum = t_carry + wave_incl_sum(dt1, (int)lane);
        r = fmaf(st.w, c0, r); g = fmaf(st.w, c1, g); b = fmaf(st.w, c2, b);
        d = fmaf(st.w, tsum, d);
        ws += st.w;
        if (st.term) break;
        T_carry = __shfl(st.T_after, 63, 64);
        t_carry = __shfl(tsum, 63, 64);
    }
    r = wave_sum(r); g = wave_sum(g); b = wave_sum(b); ws = wave_sum(ws); d = wave_sum(d);
    if (lane == 0) {
        weights_sum[index] = ws; depth[index] = d;
        image[index * 3] = r; image[index * 3 + 1] = g; image[index * 3 + 2] = b;
    }
}

// ---------------------------------------------------------------- R8 (raymarching.cu:601-682), one wave per ray
__global__ void __launch_bounds__(256) k_composite_train_bwd(const float *__restrict__ grad_weights_sum, const float *__restrict__ grad_image,
                                      const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                      const float *__restrict__ deltas, const int32_t *__restrict__ rays,
                                      const float *__restrict__ weights_sum, const float *__restrict__ image,
                                      uint32_t M, uint32_t N, float T_thresh,
                                      float *__restrict__ grad_sigmas, float *__restrict__ grad_rgbs) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (n >= N) return;
    const OtRay ry = ot_ray(rays, n, M);
    if (!ry.fits) return;
    const OtRayGrad q = ot_ray_grad(grad_image, image, weights_sum, ry.index, grad_weights_sum ? grad_weights_sum[ry.index] : 0.0f);
    float T_carry = 1.0f;
    OtColour carry = {0, 0, 0};
    for (uint32_t base = 0; base < ry.count; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < ry.count;
        const uint64_t s = (uint64_t)ry.offset + (valid ? i : 0);
        float sigma = 0, dt0 = 0, c0 = 0, c1 = 0, c2 = 0;
        if (valid) {
            sigma = sigmas[s];
            dt0 = deltas[s * 2];
            c0 = rgbs[s * 3]; c1 = rgbs[s * 3 + 1]; c2 = rgbs[s * 3 + 2];
        }
        const OtStep st = ot_step(valid, sigma, dt0, T_carry, T_thresh, lane);
        const OtColour acc = ot_running(carry, st.w, c0, c1, c2, lane);
        if (st.act) {
            grad_rgbs[s * 3] = q.g0 * st.w; grad_rgbs[s * 3 + 1] = q.g1 * st.w; grad_rgbs[s * 3 + 2] = q.g2 * st.w;
            grad_sigmas[s] = dt0 * ot_grad_acc(q, st.T_after, c0, c1, c2, acc);
        }
        if (st.term) break;
        T_carry = __shfl(st.T_after, 63, 64);
        carry = ot_last(acc);
    }
}

// ---------------------------------------------------------------- R9 (raymarching.cu:700-805)
// Where a walk puts its samples: position [3], direction [3] and (dt, span) [2] per slot. The global arrays carry a direction per sample (DIRS);
// an LDS record does not — the flush adds it.
struct RmSlots { float *px, *pd, *pl; };
__device__ __forceinline__ RmSlots rm_slots_global(float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas, uint32_t n, uint32_t n_step) {
    return RmSlots{xyzs + (uint64_t)n * n_step * 3, dirs + (uint64_t)n * n_step * 3, deltas + (uint64_t)n * n_step * 2};
}
__device__ __forceinline__ RmSlots rm_slots_lds(float *rec, uint32_t n_step) { return RmSlots{rec, nullptr, rec + 3u * n_step}; }
// The record of one emitted sample (raymarching.cu:776-787): the position as it is stored, the direction, dt and the span since the previous sample's end.
template <bool DIRS>
__device__ __forceinline__ void rm_put_sample(const RmSlots &o, uint32_t slot, const RmParams &p, const RmCell &c, const RmRay &r, float span) {
    o.px[slot * 3] = rm_out(p, c.x); o.px[slot * 3 + 1] = rm_out(p, c.y); o.px[slot * 3 + 2] = rm_out(p, c.z);
    if (DIRS) { o.pd[slot * 3] = r.dx; o.pd[slot * 3 + 1] = r.dy; o.pd[slot * 3 + 2] = r.dz; }
    o.pl[slot * 2] = c.dt; o.pl[slot * 2 + 1] = span;
}

// The serial loop of one list entry n (ray `index`), its samples into `o` from slot 0 on. BAIL: stop at the first empty cell and report it (the
// two-phase form below: such a ray is a "walker" and is marched again, from its start, by the walkers' kernel). The number of samples emitted
// and the ray's direction come back for a caller that writes the samples out itself (k_march_rays_staged).
struct RmWalked { uint32_t step; bool bailed; float dx, dy, dz; };
template <bool BAIL, bool DIRS>
__device__ __forceinline__ RmWalked rm_lane_walk(uint32_t n, int index, uint32_t n_step, const float *__restrict__ rays_t, const float *__restrict__ rays_o,
                                                 const float *__restrict__ rays_d, const uint8_t *__restrict__ grid, const RmParams &p, const float *__restrict__ fars,
                                                 const float *__restrict__ noises, RmSlots o) {
    const RmRay r = rm_load_ray(rays_o, rays_d, index);
    float t = rays_t[index];
    const float far = fars[index];
    t = rm_start(p, t, noises[n]);
    float last_t = t;
    RmWalked w = {0u, false, r.dx, r.dy, r.dz};
    RmCell c;
    while (t < far && w.step < n_step) {
        if (rm_cell(grid, p, r, t, c)) {
            t += c.dt;
            const float span = t - last_t;
            rm_put_sample<DIRS>(o, 0u, p, c, r, span);
            if (p.rederive) t = last_t + span;
            last_t = t;
            o.px += 3; o.pl += 2; w.step++;
            if (DIRS) o.pd += 3;
        } else {
            if (BAIL) { w.bailed = true; return w; }
            t = rm_skip(p, c, t, r);
        }
    }
    return w;
}

__global__ void __launch_bounds__(64) k_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                             const float *__restrict__ rays_t, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                             const uint8_t *__restrict__ grid, RmParams p, const float *__restrict__ fars,
                             float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                             const float *__restrict__ noises) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_alive) return;
    const int index = rays_alive[n];
    if (index < 0) return;             // a list entry marked dead (-1, as composite_rays leaves them): its slots stay zero = "terminated"
    (void)rm_lane_walk<false, true>(n, index, n_step, rays_t, rays_o, rays_d, grid, p, fars, noises, rm_slots_global(xyzs, dirs, deltas, n, n_step));
}

// ---------------------------------------------------------------- R9, one ray per lane, the wave's samples staged in LDS
// k_march_rays writes a ray's samples as single dwords at a 32 n_step-byte lane stride (a burst of 8: 64 stores per lane, each touching 64
// cache lines) and relies on the caller for the zeros of the slots a ray does not fill. Here a lane collects its ray's burst in LDS
// ([3 n_step] positions | [2 n_step] deltas | samples filled, direction) and the wave then writes the three arrays of its 64 list entries as
// runs of consecutive floats, zeros included: every slot of every entry is written, whole cache lines at a time. The loop is rm_lane_walk's.
__global__ void __launch_bounds__(64) k_march_rays_staged(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                             const float *__restrict__ rays_t, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                             const uint8_t *__restrict__ grid, RmParams p, const float *__restrict__ fars,
                             float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                             const float *__restrict__ noises, int sample_major) {
    extern __shared__ float rm_stage[];                    // [64][5 n_step + 4]
    const uint32_t lane = threadIdx.x, n0 = blockIdx.x * 64u, n = n0 + lane;
    const uint32_t stride = 5u * n_step + 4u;
    float *mine = rm_stage + lane * stride;
    const int index = n < n_alive ? rays_alive[n] : -1;
    RmWalked w = {0u, false, 0.0f, 0.0f, 0.0f};
    if (index >= 0) w = rm_lane_walk<false, false>(n, index, n_step, rays_t, rays_o, rays_d, grid, p, fars, noises, rm_slots_lds(mine, n_step));
    float *tail = mine + 5u * n_step;
    tail[0] = __builtin_bit_cast(float, w.step); tail[1] = w.dx; tail[2] = w.dy; tail[3] = w.dz;
    __syncthreads();                                       // one wave per workgroup: orders the LDS traffic, costs nothing
    const uint32_t cnt = min(64u, n_alive - n0);           // list entries of this wave (n0 < n_alive by the launch)
    if (sample_major) {
        // [n_step][n_alive] arrays: slot s of the wave's entries is one run of 3 cnt (2 cnt) consecutive floats. The 64 rows of an encoder /
        // network wave are then 64 NEIGHBOURING rays at the same burst slot — closer to each other than 8 consecutive samples of 8 rays
        // (a pixel apart against a step apart) — and the composite kernel's loads are contiguous across lanes.
        for (uint32_t sl = 0; sl < n_step; sl++) {
            float *gx = xyzs + ((uint64_t)sl * n_alive + n0) * 3u, *gd = dirs + ((uint64_t)sl * n_alive + n0) * 3u, *gl = deltas + ((uint64_t)sl * n_alive + n0) * 2u;
            for (uint32_t k = lane; k < cnt * 3u; k += 64u) {
                const uint32_t r = k / 3u, cc = k - r * 3u;
                const float *rec = rm_stage + r * stride;
                const bool on = sl < __builtin_bit_cast(uint32_t, rec[5u * n_step]);
                gx[k] = on ? rec[sl * 3u + cc] : 0.0f;
                gd[k] = on ? rec[5u * n_step + 1u + cc] : 0.0f;
            }
            for (uint32_t k = lane; k < cnt * 2u; k += 64u) {
                const uint32_t r = k >> 1;
                const float *rec = rm_stage + r * stride;
                gl[k] = sl < __builtin_bit_cast(uint32_t, rec[5u * n_step]) ? rec[3u * n_step + sl * 2u + (k & 1u)] : 0.0f;
            }
        }
        return;
    }
    const uint32_t lx = 3u * n_step, ll = 2u * n_step;
    const float inv_lx = 1.0f / (float)lx, inv_ll = 1.0f / (float)ll;
    float *gx = xyzs + (uint64_t)n0 * lx, *gd = dirs + (uint64_t)n0 * lx, *gl = deltas + (uint64_t)n0 * ll;
    for (uint32_t i = lane; i < cnt * lx; i += 64u) {
        const uint32_t r = (uint32_t)(((float)i + 0.5f) * inv_lx), j = i - r * lx, slot = j / 3u, cc = j - slot * 3u;
        const float *rec = rm_stage + r * stride;
        const bool on = slot < __builtin_bit_cast(uint32_t, rec[5u * n_step]);
        gx[i] = on ? rec[j] : 0.0f;
        gd[i] = on ? rec[5u * n_step + 1u + cc] : 0.0f;
    }
    for (uint32_t i = lane; i < cnt * ll; i += 64u) {
        const uint32_t r = (uint32_t)(((float)i + 0.5f) * inv_ll), j = i - r * ll;
        const float *rec = rm_stage + r * stride;
        gl[i] = (j >> 1) < __builtin_bit_cast(uint32_t, rec[5u * n_step]) ? rec[3u * n_step + j] : 0.0f;
    }
}

// ---------------------------------------------------------------- R9, G lanes per ray
// k_march_rays above is a chain of dependent bitfield lookups per ray, and a render iteration has few rays left alive (the host loop keeps
// live x n_step <= N, so most iterations march ~N/8 rays by 8 samples: about one wave per SIMD, nothing to hide a lookup's latency
// behind, and the launch lasts as long as its longest ray — one that leaves the object and walks ~100 cells to the box's far side).
// As in k_march_count_wave the values t can take are a fixed lattice per ray (both branches of the loop advance t by
// clamp(t dt_gamma, dt_min, dt_max), raymarching.cu:758-795), so G consecutive lattice points of a ray are generated on G lanes (the
// recurrence itself, each value entering at the row's last lane through a DPP row_shl:1 move), looked up with ONE round of loads, and the
// loop's control flow is replayed on the G-bit masks of the ray's lane group: an occupied visited point emits (position, direction, dt,
// t_new - last_t) into the ray's next slot and moves on by one lane; an empty one moves to the first lane whose t is not below the voxel
// exit, carried into the next G points when there is none. Same visits, same samples, bit for bit — with chains G times shorter. A full
// wave per ray (G = 64, the training kernel's form) would spend 64 recurrence steps for the 8 samples an iteration asks for; G = 16
// (one DPP row, 4 rays per wave) generates what a burst of 8 typically consumes in one or two rounds.
#define RM_ROW_MAX_ROUNDS (1u << 14)                       // x 16 lattice points: far beyond any real ray; makes the loop finite whatever the inputs
// all 64 lanes of a wave call this together; `have`, `n`, `index` are uniform over each 16-lane group
// The samples go to `o`: the ray's slots of the global arrays (DIRS), or its LDS record (rm_slots_lds: 5 n_step floats per 16-lane group), which
// leaves in rm_row_flush — whole runs of consecutive floats per group, zeros in the slots the ray did not fill — instead of as single dwords at
// a 32 n_step-byte lane stride.
template <bool MED3, bool DIRS>
__device__ __forceinline__ uint32_t rm_row_walk(bool have, uint32_t n, int index, uint32_t n_step, const float *__restrict__ rays_t, const float *__restrict__ rays_o,
                                            const float *__restrict__ rays_d, const uint8_t *__restrict__ grid, const RmParams &p, const float *__restrict__ fars,
                                            const float *__restrict__ noises, const RmSlots o) {
    constexpr uint32_t G = 16u;
    const uint32_t lane = threadIdx.x & 63u, sub = lane & (G - 1u), gbase = lane & ~(G - 1u), gshift = gbase;
    const RmRay r = rm_load_ray(rays_o, rays_d, index);
    const float far = fars[index];
    float t_cur = rm_start(p, rays_t[index], noises[have ? n : 0u]);
    float last_t = t_cur;
    uint32_t step = 0;
    bool skipping = false, live = have;                    // live: this ray's loop has not ended (uniform over the ray's G lanes)
    float skip_to = 0.0f;
    const uint32_t below = (1u << sub) - 1u;
    for (uint32_t round = 0; round < RM_ROW_MAX_ROUNDS && __builtin_amdgcn_ballot_w64(live) != 0ull; round++) {
        float T, t_next;
        rm_lattice<0x101, G, MED3>(p, t_cur, T, t_next);
        // every lane of the wave evaluates its lattice point (rays that have ended idle along: their results are not looked at)
        RmCell c;
        const bool occupied_here = rm_cell(grid, p, r, T, c);
        const float exit_here = rm_skip_target(p, c, T, r);
        const float t_new = T + c.dt;                      // the loop's `t += dt` of an emitting visit (== the next lattice point)
        const uint32_t in_range = (uint32_t)(__ballot(T < far) >> gshift) & 0xFFFFu;
        const uint32_t occ = (uint32_t)(__ballot(occupied_here) >> gshift) & 0xFFFFu;
        uint32_t emitted = 0u;
        if (live) {
            uint32_t k = 0;
            bool go = true;
            if (skipping) {
                const uint32_t landed = (uint32_t)(__ballot(!(T < skip_to)) >> gshift) & 0xFFFFu;
                if (landed == 0u) {
                    if (!((in_range >> (G - 1u)) & 1u)) live = false;      // t only grows: wherever the skip lands, it is beyond `far`
                    go = false;
                } else { k = (uint32_t)__builtin_ctz(landed); skipping = false; }
            }
            const uint32_t emit_ok = occ & in_range;
            uint32_t room = n_step - step;
            while (go && k < G) {
                if (!((in_range >> k) & 1u) || room == 0u) { live = false; break; }        // the loop condition of raymarching.cu:745
                if ((emit_ok >> k) & 1u) {                 // a run of occupied points: each emits and steps to its successor
                    const uint32_t rest = ~(emit_ok >> k) & (0xFFFFu >> k);
                    uint32_t len = rest ? (uint32_t)__builtin_ctz(rest) : G - k;
                    len = len < room ? len : room;
                    emitted |= ((1u << len) - 1u) << k;
                    room -= len;
                    k += len;
                } else {
                    const float tt = __shfl(exit_here, (int)(gbase + k), 64);
                    const uint32_t above = k >= G - 1u ? 0u : ((0xFFFFu << (k + 1u)) & 0xFFFFu);
                    const uint32_t landed = (uint32_t)(__ballot(!(T < tt)) >> gshift) & above;      // do { advance } while (t < tt): at least one advance
                    if (landed == 0u) { skipping = true; skip_to = tt; break; }
                    k = (uint32_t)__builtin_ctz(landed);
                }
            }
        }
        // the emitting lanes write their samples; delta[1] spans from the previous emitted sample's end (or the carried one)
        const uint32_t before = emitted & below;
        const int prev_lane = before ? (int)(gbase + 31u - (uint32_t)__builtin_clz(before)) : (int)lane;
        const float prev_end = __shfl(t_new, prev_lane, 64);
        if ((emitted >> sub) & 1u) rm_put_sample<DIRS>(o, step + (uint32_t)__builtin_popcount(before), p, c, r, t_new - (before ? prev_end : last_t));
        const int top_lane = emitted ? (int)(gbase + 31u - (uint32_t)__builtin_clz(emitted)) : (int)lane;
        const float top_end = __shfl(t_new, top_lane, 64);
        if (emitted) last_t = top_end;
        step += (uint32_t)__builtin_popcount(emitted);
        t_cur = t_next;
    }
    return step;
}

// the staged samples of list entry n (`filled` of its n_step slots) -> memory; every lane of the 16-lane group calls this after the block's barrier
__device__ __forceinline__ void rm_row_flush(uint32_t n, int index, uint32_t n_step, uint32_t filled, const float *__restrict__ rays_d, const float *stage,
                                             float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas) {
    const uint32_t sub = threadIdx.x & 15u;
    const float dx = rays_d[index * 3], dy = rays_d[index * 3 + 1], dz = rays_d[index * 3 + 2];
    float *px = xyzs + (uint64_t)n * n_step * 3, *pd = dirs + (uint64_t)n * n_step * 3, *pl = deltas + (uint64_t)n * n_step * 2;
    for (uint32_t i = sub; i < n_step * 3u; i += 16u) {
        const uint32_t slot = i / 3u, c = i - slot * 3u;
        const bool on = slot < filled;
        px[i] = on ? stage[i] : 0.0f;
        pd[i] = on ? (c == 0u ? dx : c == 1u ? dy : dz) : 0.0f;
    }
    for (uint32_t i = sub; i < n_step * 2u; i += 16u) pl[i] = (i >> 1) < filled ? stage[3 * n_step + i] : 0.0f;
}

template <bool MED3>
__global__ void __launch_bounds__(256) k_march_rays_row(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                             const float *__restrict__ rays_t, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                             const uint8_t *__restrict__ grid, RmParams p, const float *__restrict__ fars,
                             float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                             const float *__restrict__ noises) {
    __shared__ float stage[16][5 * 16];                     // per 16-lane group: positions [n_step, 3] | deltas [n_step, 2], n_step <= 16
    const uint32_t n = (blockIdx.x * 256u + threadIdx.x) / 16u;
    const int listed = n < n_alive ? rays_alive[n] : -1;
    const bool have = listed >= 0;     // beyond the list, or an entry marked dead (-1): nothing to march
    float *mine = stage[threadIdx.x >> 4];
    const uint32_t filled = rm_row_walk<MED3, false>(have, n, have ? listed : 0, n_step, rays_t, rays_o, rays_d, grid, p, fars, noises, rm_slots_lds(mine, n_step));
    __syncthreads();
    // every entry of the list leaves with all of its slots written (a dead one: zeros = "terminated"), so the caller need not have zeroed them
    if (n < n_alive) rm_row_flush(n, have ? listed : 0, n_step, have ? filled : 0u, rays_d, mine, xyzs, dirs, deltas);
}

// ---------------------------------------------------------------- R9 in two phases (the native render step, csrc/occrender.hip)
// A launch with hundreds of thousands of live rays asks each of them for one sample: a ray inside the object evaluates one cell and is
// done, while the few percent that have just left it walk ~100 empty cells to the far side of the box — and every wave runs as long as
// its longest lane (48 us per launch, of which the cell evaluations proper are ~3 us). Phase 1 (k_march_rays_first): the serial loop
// per lane, but a ray that meets an EMPTY cell stops there and puts its list entry on a worklist (one atomic per wave). Phase 2
// (k_march_walkers): the worklist's rays are marched again from their start — densely packed: 16 lanes per ray while there are few of them
// (chains 16 times shorter), one ray per lane when the list is long (the first iteration of a view, where every ray starts in empty
// space). Same samples as the single kernel, bit for bit: a walker's slots are simply written twice with the same values.
__global__ void __launch_bounds__(256) k_march_rays_first(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                             const float *__restrict__ rays_t, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                             const uint8_t *__restrict__ grid, RmParams p, const float *__restrict__ fars,
                             float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                             const float *__restrict__ noises, int32_t *__restrict__ worklist, int32_t *__restrict__ wl_count) {
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    bool walker = false;
    if (n < n_alive) {
        const int index = rays_alive[n];
        if (index >= 0) walker = rm_lane_walk<true, true>(n, index, n_step, rays_t, rays_o, rays_d, grid, p, fars, noises, rm_slots_global(xyzs, dirs, deltas, n, n_step)).bailed;
    }
    const uint64_t mask = __ballot(walker);
    if (mask != 0ull) {
        const uint32_t lane = threadIdx.x & 63u;
        int base = 0;
        if (lane == (uint32_t)__builtin_ctzll(mask)) base = atomicAdd(wl_count, (int)__builtin_popcountll(mask));
        base = __shfl(base, (int)__builtin_ctzll(mask), 64);
        if (walker) worklist[base + (int)__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = (int32_t)n;
    }
}

template <bool MED3>
__global__ void __launch_bounds__(256) k_march_walkers(uint32_t n_alive, uint32_t n_step, const int32_t *__restrict__ rays_alive,
                             const float *__restrict__ rays_t, const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                             const uint8_t *__restrict__ grid, RmParams p, const float *__restrict__ fars,
                             float *__restrict__ xyzs, float *__restrict__ dirs, float *__restrict__ deltas,
                             const float *__restrict__ noises, const int32_t *__restrict__ worklist, const int32_t *__restrict__ wl_count, uint32_t row_max) {
    const uint32_t count = min((uint32_t)max(*wl_count, 0), n_alive);         // grid-uniform
    if (count <= row_max) {
        const uint32_t groups_total = gridDim.x * 16u;                          // 16-lane groups of the grid
        const uint32_t wave_first = (blockIdx.x * 256u + (threadIdx.x & ~63u)) / 16u;
        for (uint32_t base = wave_first; base < count; base += groups_total) {  // wave-uniform trip count: the four groups walk together
            const uint32_t i = base + ((threadIdx.x & 63u) >> 4);
            const bool have = i < count;
            const uint32_t n = have ? (uint32_t)worklist[i] : 0u;
            rm_row_walk<MED3, true>(have, n, have ? rays_alive[n] : 0, n_step, rays_t, rays_o, rays_d, grid, p, fars, noises, rm_slots_global(xyzs, dirs, deltas, n, n_step));
        }
    } else {
        for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < count; i += gridDim.x * 256u) {
            const uint32_t n = (uint32_t)worklist[i];
            (void)rm_lane_walk<false, true>(n, rays_alive[n], n_step, rays_t, rays_o, rays_d, grid, p, fars, noises, rm_slots_global(xyzs, dirs, deltas, n, n_step));
        }
    }
}

// Where rays die, for a caller that deals the samples over iterations differently from the reference and must know what the reference's
// own loop would have done (focnerf_amd/renderer.py): hist[min(base + j, len - 1)][slice] += 1 for a ray that ends at slot j of this call
// (no sample there, or the transmittance test after it). hist == nullptr: nothing recorded. A view's rays die in a few iterations, tens of
// thousands per launch into n_step bins: the wave adds its rays per bin with one atomic, and the bins come in RM_DEATH_SLICES copies
// (slice = wave index mod RM_DEATH_SLICES; the reader sums them) — one add per ray on 8 addresses cost 5 ms per view.
#define RM_DEATH_SLICES 64u
struct RmDeaths { int32_t *hist; uint32_t base, len; int sample_major; };      // (sample_major: the layout of the sample arrays rides along)
__device__ __forceinline__ void rm_record_deaths(const RmDeaths &dh, bool died, uint32_t at, uint32_t n_step, uint32_t n) {
    if (!dh.hist) return;
    if (__ballot(died) == 0ull) return;
    const uint32_t slice = (n >> 6) & (RM_DEATH_SLICES - 1u);
    for (uint32_t j = 0; j < n_step; j++) {
        const uint64_t m = __ballot(died && at == j);
        if (m != 0ull && (threadIdx.x & 63u) == 0u)
            atomicAdd(&dh.hist[(uint64_t)min(dh.base + j, dh.len - 1u) * RM_DEATH_SLICES + slice], (int)__builtin_popcountll(m));
    }
}

// ---------------------------------------------------------------- R10 (raymarching.cu:818-905)
// What a ray accumulates over the calls of a view, and the three pieces both composite kernels are made of.
// AUX (compile time): a SECOND payload of three floats per sample rides along — the encoded normal next to the colour in the native render step
// (foc_occ_render_step_normals, mode AUX) — accumulated with the first payload's weights into a second [N,3] image. One set of weights, one
// stop test, one deaths histogram; AUX = false is the code it was before the flag existed (same members, same kernel arguments).
template <bool AUX> struct RmAcc { float t, weight_sum, d, r, g, b; };
template <> struct RmAcc<true> { float t, weight_sum, d, r, g, b, x, y, z; };
// what the second payload adds to a kernel's arguments: its samples (laid out as rgbs) and its accumulator (laid out as image)
template <bool AUX> struct RmSide : RmDeaths {};
template <> struct RmSide<true> : RmDeaths { const float *aux; float *aux_image; };
template <bool AUX>
__device__ __forceinline__ RmAcc<AUX> rm_acc_load(int index, const float *__restrict__ rays_t, const float *__restrict__ weights_sum, const float *__restrict__ depth,
                                                  const float *__restrict__ image, const RmSide<AUX> &side) {
    if constexpr (AUX)
        return RmAcc<true>{rays_t[index], weights_sum[index], depth[index], image[index * 3], image[index * 3 + 1], image[index * 3 + 2],
                           side.aux_image[index * 3], side.aux_image[index * 3 + 1], side.aux_image[index * 3 + 2]};
    else
        return RmAcc<false>{rays_t[index], weights_sum[index], depth[index], image[index * 3], image[index * 3 + 1], image[index * 3 + 2]};
}
// one sample (:862-896) -> the ray ends here: the slot holds no sample (dt0 == 0), or the transmittance before it was below T_thresh.
// Not free: k_composite_rays compiles to 153 / 218 instructions (COUNT off / on) through this function and rm_composite_finish, to 140 / 203 with
// both spelled out in it (scalar control flow; registers, occupancy and the burst-1 view's time are unchanged): NOTEBOOK "One definition of the
// occupancy march". Compare the counts again when changing either function.
// (p0, p1, p2: the sample's second payload, read with AUX only)
template <bool AUX>
__device__ __forceinline__ bool rm_composite_sample(RmAcc<AUX> &a, float sigma, float dt0, float dt1, float c0, float c1, float c2, float p0, float p1, float p2,
                                                    float T_thresh) {
    if (dt0 == 0) return true;
    const float alpha = 1.0f - __expf(-sigma * dt0);
    const float T = 1 - a.weight_sum;
    const float weight = alpha * T;
    a.weight_sum += weight;
    a.t += dt1;
    a.d = fmaf(weight, a.t, a.d);
    a.r = fmaf(weight, c0, a.r); a.g = fmaf(weight, c1, a.g); a.b = fmaf(weight, c2, a.b);
    if constexpr (AUX) { a.x = fmaf(weight, p0, a.x); a.y = fmaf(weight, p1, a.y); a.z = fmaf(weight, p2, a.z); }
    return T < T_thresh;
}
// List entry n after its burst: ended at slot `ended_at` (marked dead) or still going (its t is kept for the next call); the accumulators go back.
// Every lane of the wave comes here — `index` < 0: beyond the list or already marked dead (stays dead, nothing to accumulate).
// COUNT: the wave also adds its number of surviving entries to block_counts[n / 1024] (zeroed by the caller) — the first pass of the ordered
// compaction that follows in the native render step (k_compact_count otherwise) — and records where its rays died.
template <bool COUNT, bool AUX>
__device__ __forceinline__ void rm_composite_finish(uint32_t n, int index, const RmAcc<AUX> &a, bool ended, uint32_t ended_at, uint32_t n_step,
                                                    int32_t *__restrict__ rays_alive, float *__restrict__ rays_t, float *__restrict__ weights_sum,
                                                    float *__restrict__ depth, float *__restrict__ image, int32_t *__restrict__ block_counts, const RmSide<AUX> &dh) {
    if (index >= 0) {
        if (ended) rays_alive[n] = -1; else rays_t[index] = a.t;
        weights_sum[index] = a.weight_sum; depth[index] = a.d;
        image[index * 3] = a.r; image[index * 3 + 1] = a.g; image[index * 3 + 2] = a.b;
        if constexpr (AUX) { dh.aux_image[index * 3] = a.x; dh.aux_image[index * 3 + 1] = a.y; dh.aux_image[index * 3 + 2] = a.z; }
    }
    if (COUNT) {
        const uint64_t alive = __ballot(index >= 0 && !ended);
        if ((threadIdx.x & 63u) == 0u && alive != 0ull) atomicAdd(&block_counts[n >> 10], (int)__builtin_popcountll(alive));
        rm_record_deaths(dh, index >= 0 && ended, ended_at, n_step, n);
    }
}

template <bool COUNT, bool AUX = false>
__global__ void __launch_bounds__(64) k_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh,
                                 int32_t *__restrict__ rays_alive, float *__restrict__ rays_t,
                                 const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                 float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image, int32_t *__restrict__ block_counts,
                                 RmSide<AUX> dh) {
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    const int index = n < n_alive ? rays_alive[n] : -1;
    RmAcc<AUX> a = {};
    uint32_t step = 0;
    if (index >= 0) {
        // ray-major [n_alive][n_step] (the reference's layout) or sample-major [n_step][n_alive] (dh.sample_major: the native render step)
        const uint64_t first = dh.sample_major ? (uint64_t)n : (uint64_t)n * n_step, hop = dh.sample_major ? (uint64_t)n_alive : 1ull;
        const float *s = sigmas + first, *c = rgbs + first * 3, *dl = deltas + first * 2;
        a = rm_acc_load(index, rays_t, weights_sum, depth, image, dh);
        if constexpr (AUX) {
            const float *p = dh.aux + first * 3;
            while (step < n_step) {
                if (rm_composite_sample(a, s[0], dl[0], dl[1], c[0], c[1], c[2], p[0], p[1], p[2], T_thresh)) break;
                s += hop; c += 3 * hop; p += 3 * hop; dl += 2 * hop; step++;
            }
        } else {
        while (step < n_step) {
            if (rm_composite_sample(a, s[0], dl[0], dl[1], c[0], c[1], c[2], 0.0f, 0.0f, 0.0f, T_thresh)) break;
            s += hop; c += 3 * hop; dl += 2 * hop; step++;
        }
        }
    }
    rm_composite_finish<COUNT>(n, index, a, step < n_step, step, n_step, rays_alive, rays_t, weights_sum, depth, image, block_counts, dh);
}

// The same with a compile-time burst length that is a multiple of 4: the lane first loads ALL of its ray's sigmas / colours / deltas with
// 16-byte loads (NS, 3 NS and 2 NS consecutive floats: whole cache lines per lane, every load in flight at once) and then runs the serial
// accumulation on registers — with the pointer-chasing loop above a burst of 8 is 8 dependent rounds of 4-byte loads at a 32-byte lane stride
// (86 us per 5.1 M samples, 1.4 TB/s). Same operations in the same order: same bits.
// AUX: 3 NS more floats per lane, loaded the same way and kept in registers like the rest, not staged in LDS: the compiler gives the counting
// kernels 64 / 112 / 254 VGPRs at NS 4 / 8 / 16 (72 / 176 at 8 / 16 without the payload), no spills, 8 / 4 / 2 waves per SIMD — every load of a
// lane is in flight before its first use, which is what the kernel lives on, not on waves to switch between.
template <int NS, bool COUNT, bool AUX = false>
__global__ void __launch_bounds__(64) k_composite_rays_pre(uint32_t n_alive, float T_thresh, int32_t *__restrict__ rays_alive, float *__restrict__ rays_t,
                                     const float *__restrict__ sigmas, const float *__restrict__ rgbs, const float *__restrict__ deltas,
                                     float *__restrict__ weights_sum, float *__restrict__ depth, float *__restrict__ image, int32_t *__restrict__ block_counts,
                                     RmSide<AUX> dh) {
    static_assert(NS % 4 == 0, "whole float4 loads");
    const uint32_t n = blockIdx.x * blockDim.x + threadIdx.x;
    const int index = n < n_alive ? rays_alive[n] : -1;
    RmAcc<AUX> a = {};
    bool ended = false;
    uint32_t ended_at = 0;
    if (index >= 0) {
        float sg[NS], cl[3 * NS], dl[2 * NS], px[AUX ? 3 * NS : 1];
        if (dh.sample_major) {             // [NS][n_alive]: consecutive lanes read consecutive rays of one slot
#pragma unroll
            for (int i = 0; i < NS; i++) {
                const uint64_t m = (uint64_t)i * n_alive + n;
                sg[i] = sigmas[m];
                cl[3 * i] = rgbs[m * 3]; cl[3 * i + 1] = rgbs[m * 3 + 1]; cl[3 * i + 2] = rgbs[m * 3 + 2];
                if constexpr (AUX) { px[3 * i] = dh.aux[m * 3]; px[3 * i + 1] = dh.aux[m * 3 + 1]; px[3 * i + 2] = dh.aux[m * 3 + 2]; }
                const float2 v = *reinterpret_cast<const float2 *>(deltas + m * 2);
                dl[2 * i] = v.x; dl[2 * i + 1] = v.y;
            }
        } else {
        const float4 *ps = reinterpret_cast<const float4 *>(sigmas + (uint64_t)n * NS);
        const float4 *pc = reinterpret_cast<const float4 *>(rgbs + (uint64_t)n * NS * 3);
        const float4 *pd = reinterpret_cast<const float4 *>(deltas + (uint64_t)n * NS * 2);
#pragma unroll
        for (int i = 0; i < NS / 4; i++) { const float4 v = ps[i]; sg[4 * i] = v.x; sg[4 * i + 1] = v.y; sg[4 * i + 2] = v.z; sg[4 * i + 3] = v.w; }
#pragma unroll
        for (int i = 0; i < 3 * NS / 4; i++) { const float4 v = pc[i]; cl[4 * i] = v.x; cl[4 * i + 1] = v.y; cl[4 * i + 2] = v.z; cl[4 * i + 3] = v.w; }
#pragma unroll
        for (int i = 0; i < 2 * NS / 4; i++) { const float4 v = pd[i]; dl[4 * i] = v.x; dl[4 * i + 1] = v.y; dl[4 * i + 2] = v.z; dl[4 * i + 3] = v.w; }
        if constexpr (AUX) {
            const float4 *pp = reinterpret_cast<const float4 *>(dh.aux + (uint64_t)n * NS * 3);
#pragma unroll
            for (int i = 0; i < 3 * NS / 4; i++) { const float4 v = pp[i]; px[4 * i] = v.x; px[4 * i + 1] = v.y; px[4 * i + 2] = v.z; px[4 * i + 3] = v.w; }
        }
        }
        a = rm_acc_load(index, rays_t, weights_sum, depth, image, dh);
#pragma unroll
        for (int step = 0; step < NS; step++) {
            if (!ended) {
                ended_at = (uint32_t)step;
                if constexpr (AUX)
                    ended = rm_composite_sample(a, sg[step], dl[2 * step], dl[2 * step + 1], cl[3 * step], cl[3 * step + 1], cl[3 * step + 2], px[3 * step],
                                                px[3 * step + 1], px[3 * step + 2], T_thresh);
                else
                ended = rm_composite_sample(a, sg[step], dl[2 * step], dl[2 * step + 1], cl[3 * step], cl[3 * step + 1], cl[3 * step + 2], 0.0f, 0.0f, 0.0f, T_thresh);
            }
        }
    }
    rm_composite_finish<COUNT>(n, index, a, ended, ended_at, (uint32_t)NS, rays_alive, rays_t, weights_sum, depth, image, block_counts, dh);
}

template <bool COUNT, bool AUX = false>
static void rm_launch_composite(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t, const float *sigmas, const float *rgbs,
                                const float *deltas, float *weights_sum, float *depth, float *image, int32_t *block_counts, hipStream_t st,
                                RmSide<AUX> dh = RmSide<AUX>{RmDeaths{nullptr, 0u, 1u, 0}}) {
    uintptr_t addresses = reinterpret_cast<uintptr_t>(sigmas) | reinterpret_cast<uintptr_t>(rgbs) | reinterpret_cast<uintptr_t>(deltas);
    if constexpr (AUX) addresses |= reinterpret_cast<uintptr_t>(dh.aux);
    const bool aligned = (addresses & 15u) == 0;
    // (`burst`: the run-time n_step argument of the general kernel; the others have it in their name)
    const auto launch = [&](auto kernel, auto... burst) {
        hipLaunchKernelGGL(kernel, dim3(foc_div_up(n_alive, 64)), dim3(64), 0, st, n_alive, burst..., T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth,
                           image, block_counts, dh);
    };
    if (aligned && n_step == 4u) launch(k_composite_rays_pre<4, COUNT, AUX>);
    else if (aligned && n_step == 8u) launch(k_composite_rays_pre<8, COUNT, AUX>);
    else if (aligned && n_step == 16u) launch(k_composite_rays_pre<16, COUNT, AUX>);
    else launch(k_composite_rays<COUNT, AUX>, n_step);
}

// ---------------------------------------------------------------- ordered compaction of rays_alive >= 0
__global__ void __launch_bounds__(1024) k_compact_count(const int32_t *__restrict__ in, uint32_t n, int32_t *__restrict__ block_counts) {
    __shared__ int s_w[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    const int keep = (i < n && in[i] >= 0) ? 1 : 0;
    const int c = wave_sum_i(keep);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { int t = 0; for (int k = 0; k < 16; k++) t += s_w[k]; block_counts[blockIdx.x] = t; }
}
__global__ void __launch_bounds__(1024) k_compact_scan(int32_t *__restrict__ block_counts, uint32_t nb, int32_t *__restrict__ n_out) {
    // single workgroup: exclusive scan of nb block counts in place
    const RmScan sc = rm_scan_1024(block_counts, nb, n_out);
    int run = sc.base;
    for (uint32_t i = sc.lo; i < sc.hi; i++) { const int c = block_counts[i]; block_counts[i] = run; run += c; }
}
__global__ void __launch_bounds__(1024) k_compact_scatter(const int32_t *__restrict__ in, uint32_t n, const int32_t *__restrict__ block_base,
                                                          int32_t *__restrict__ out) {
    __shared__ int s_w[16];
    const uint32_t i = blockIdx.x * 1024 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v = i < n ? in[i] : -1;
    const int keep = v >= 0 ? 1 : 0;
    const int incl = wave_incl_sum_i(keep, (int)lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int wbase = 0;
    for (uint32_t k = 0; k < wave; k++) wbase += s_w[k];
    if (keep) out[block_base[blockIdx.x] + wbase + incl - 1] = v;
}

// ================================================================= host entry points
/* foc_composite_rays + the ordered compaction of the survivors into `out` (count in n_out), the compaction's counting pass done by the
 * composite kernel itself: block_counts = int32[n_alive / 1024 + 2], ZEROED by the caller on this stream. (csrc/occrender.hip) */
template <bool AUX>
static int rm_composite_compact(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t, const float *sigmas, const float *rgbs,
                                const float *deltas, float *weights_sum, float *depth, float *image, int32_t *out, int32_t *n_out, int32_t *block_counts,
                                const RmSide<AUX> &side, hipStream_t st) {
    rm_launch_composite<true, AUX>(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, block_counts, st, side);
    FOC_CHECK_LAUNCH("composite_compact(composite)");
    const uint32_t nb = foc_div_up(n_alive, 1024);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, block_counts, nb, n_out);
    FOC_CHECK_LAUNCH("composite_compact(scan)");
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(1024), 0, st, rays_alive, n_alive, block_counts, out);
    FOC_CHECK_LAUNCH("composite_compact(scatter)");
    return FOC_OK;
}

extern "C" {

int foc_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb, uint32_t N, float min_near,
                           float *nears, float *fars, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(rays_o && rays_d && aabb && nears && fars, FOC_E_INVALID, "near_far_from_aabb: null pointer");
    hipLaunchKernelGGL(k_near_far_from_aabb, dim3(foc_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream,
                       rays_o, rays_d, aabb, N, min_near, nears, fars);
    FOC_CHECK_LAUNCH("near_far_from_aabb");
    return FOC_OK;
}

int foc_sph_from_ray(const float *rays_o, const float *rays_d, float radius, uint32_t N, float *coords, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(rays_o && rays_d && coords, FOC_E_INVALID, "sph_from_ray: null pointer");
    hipLaunchKernelGGL(k_sph_from_ray, dim3(foc_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, radius, N, coords);
    FOC_CHECK_LAUNCH("sph_from_ray");
    return FOC_OK;
}

int foc_morton3D(const int32_t *coords, uint32_t N, int32_t *indices, void *stream) {
    FocDeviceGuard foc_guard_(stream, coords);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(coords && indices, FOC_E_INVALID, "morton3D: null pointer");
    hipLaunchKernelGGL(k_morton3D, dim3(foc_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, coords, N, indices);
    FOC_CHECK_LAUNCH("morton3D");
    return FOC_OK;
}

int foc_morton3D_invert(const int32_t *indices, uint32_t N, int32_t *coords, void *stream) {
    FocDeviceGuard foc_guard_(stream, indices);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(coords && indices, FOC_E_INVALID, "morton3D_invert: null pointer");
    hipLaunchKernelGGL(k_morton3D_invert, dim3(foc_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, indices, N, coords);
    FOC_CHECK_LAUNCH("morton3D_invert");
    return FOC_OK;
}

int foc_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, void *stream) {
    FocDeviceGuard foc_guard_(stream, grid);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(grid && bitfield, FOC_E_INVALID, "packbits: null pointer");
    uint32_t N4 = 0;
    if ((((uintptr_t)grid) & 15u) == 0 && (((uintptr_t)bitfield) & 3u) == 0) N4 = N / 4;
    if (N4) {
        hipLaunchKernelGGL(k_packbits_x4, dim3(foc_grid_1d(N4, 256)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4 *>(grid), N4, density_thresh, reinterpret_cast<uint32_t *>(bitfield));
        FOC_CHECK_LAUNCH("packbits");
    }
    if (N4 * 4 < N) {
        hipLaunchKernelGGL(k_packbits_tail, dim3(foc_grid_1d(N - N4 * 4, 256)), dim3(256), 0, (hipStream_t)stream,
                           grid, N4 * 4, N, density_thresh, bitfield);
        FOC_CHECK_LAUNCH("packbits(tail)");
    }
    return FOC_OK;
}

// what every marching entry point refuses: a grid the kernels are not written for
// (`n_step_max` != 0: the entry point marches bursts of 1 .. n_step_max samples and names n_step in its refusal)
static int rm_check_grid(const char *who, uint32_t C, uint32_t H, uint32_t max_steps, uint32_t n_step_max = 0, uint32_t n_step = 1) {
    const bool ok = C >= 1 && C <= 8 && H >= 2 && H <= 512 && max_steps >= 1;
    if (n_step_max) FOC_REQUIRE(ok && n_step >= 1 && n_step <= n_step_max, FOC_E_INVALID, "%s: unsupported C=%u H=%u max_steps=%u n_step=%u", who, C, H, max_steps, n_step);
    FOC_REQUIRE(ok, FOC_E_INVALID, "%s: unsupported C=%u H=%u max_steps=%u", who, C, H, max_steps);
    // the float index `level*H^3 + morton` of raymarching.cu:378 is exact only below 2^24
    FOC_REQUIRE((uint64_t)C * H * H * H <= (1ull << 24), FOC_E_INVALID, "%s: C*H^3 exceeds 2^24", who);
    return FOC_OK;
}

// counts [N] (+ pad), then the per-ray strips of sample positions [N, max_steps]
static uint64_t rm_strip_offset(uint32_t N) { return (((uint64_t)N + 64) * sizeof(int32_t) + 255) & ~(uint64_t)255; }
uint64_t foc_march_rays_train_scratch_bytes(uint32_t N, uint32_t max_steps) { return rm_strip_offset(N) + (uint64_t)N * max_steps * sizeof(float); }

static int rm_march_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                          uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                          float *nears, float *fars, float *xyzs, float *dirs, float *deltas,
                          int32_t *rays, int32_t *counter, const float *noises, int32_t *scratch, void *sh_rows, bool field, uint32_t pad_align,
                          const float *aabb, float min_near, void *stream) {
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(rays_o && rays_d && grid && nears && fars && rays && counter && noises && scratch, FOC_E_INVALID,
                "march_rays_train: null pointer");
    FOC_REQUIRE(M == 0 || (xyzs && deltas && (field ? sh_rows != nullptr : dirs != nullptr)), FOC_E_INVALID, "march_rays_train: null output with M > 0");
    if (const int bad = rm_check_grid("march_rays_train", C, H, max_steps)) return bad;
    RmParams p = rm_make_params(bound, dt_gamma, max_steps, C, H);
    hipStream_t st = (hipStream_t)stream;
    float *tstrip = reinterpret_cast<float *>(reinterpret_cast<char *>(scratch) + rm_strip_offset(N));
    // A wave per ray repeats the lattice recurrence on 64 lanes: about 4x the instructions of a ray per lane, in exchange for a chain
    // of dependent lookups 64x shorter. That pays while the lane-per-ray kernel is latency-bound. Measured per call (tools/
    // time_march_modes.py, wave / lane): 4096 rays 77 / 138 us, 8192 127 / 178, 16384 221 / 267, 32768 417 / 278, 65536 825 / 460.
    // FOC_MARCH_SERIAL=1 / 0 forces one.
    const int forced = foc_opt(FOC_OPT_MARCH_SERIAL);
    const bool serial = forced >= 0 ? forced != 0 : N > 16384u;
    if (serial)
        hipLaunchKernelGGL(k_march_count, dim3(foc_div_up(N, 64)), dim3(64), 0, st, rays_o, rays_d, grid, p, max_steps, N, nears, fars, noises, scratch, tstrip, aabb, min_near);
    else
        hipLaunchKernelGGL(p.dt_min <= p.dt_max ? k_march_count_wave<true> : k_march_count_wave<false>, dim3(foc_div_up(N, 4)), dim3(256), 0, st, rays_o, rays_d,
                           grid, p, max_steps, N, nears, fars, noises, scratch, tstrip, aabb, min_near, (const int32_t *)counter);
    FOC_CHECK_LAUNCH("march_rays_train(count)");
    // The reference's callers always pass a freshly zeroed counter (legacy/nerf/renderer.py:281-283):
    // rays rows are written at index i (ray order); counter[0] is honoured as the base offset.
    // Batches of the wave form (<= 16 384 rays: every emit workgroup can afford to add up the counts before its rays) reserve their slots in
    // the emit pass; larger ones keep the one-workgroup scan.
    const bool scan_in_emit = !serial && N <= 16384u;     // (FOC_MARCH_SERIAL=0 can force the wave form on larger batches)
    if (!scan_in_emit) {
        hipLaunchKernelGGL(k_march_scan, dim3(1), dim3(1024), 0, st, scratch, N, rays, counter);
        FOC_CHECK_LAUNCH("march_rays_train(scan)");
    }
    if (field) {
        p.norm_inv = 1.0f / (2.0f * bound);                // (x + bound) / (2 bound) as torch evaluates it: times the reciprocal (grid.py:149)
        auto emit = k_march_emit<true, false>;
        if (scan_in_emit) emit = k_march_emit<true, true>;
        hipLaunchKernelGGL(emit, dim3(foc_div_up(N, 4) + RM_PAD_BLOCKS), dim3(256), 0, st, rays_o, rays_d, p, max_steps, N, M, nears, noises, rays, tstrip, xyzs,
                           (float *)nullptr, deltas, (_Float16 *)sh_rows, counter, pad_align, (const int32_t *)scratch);
    } else {
        auto emit = k_march_emit<false, false>;
        if (scan_in_emit) emit = k_march_emit<false, true>;
        hipLaunchKernelGGL(emit, dim3(foc_div_up(N, 4)), dim3(256), 0, st, rays_o, rays_d, p, max_steps, N, M, nears, noises, rays, tstrip, xyzs, dirs, deltas,
                           (_Float16 *)nullptr, counter, 0u, (const int32_t *)scratch);
    }
    FOC_CHECK_LAUNCH("march_rays_train(emit)");
    return FOC_OK;
}

int foc_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                         uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                         const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                         int32_t *rays, int32_t *counter, const float *noises, int32_t *scratch, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    return rm_march_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, const_cast<float *>(nears), const_cast<float *>(fars), xyzs, dirs, deltas, rays,
                          counter, noises, scratch, nullptr, false, 0u, nullptr, 0.0f, stream);
}

int foc_march_rays_train_field(const float *rays_o, const float *rays_d, const uint8_t *grid, float bound, float dt_gamma,
                               uint32_t max_steps, uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                               float *nears, float *fars, float *enc_in, void *sh_rows, float *deltas,
                               int32_t *rays, int32_t *counter, const float *noises, int32_t *scratch, uint32_t pad_align,
                               const float *aabb, float min_near, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    return rm_march_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nears, fars, enc_in, nullptr, deltas, rays, counter, noises, scratch, sh_rows, true,
                          pad_align, aabb, min_near, stream);
}

int foc_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas, const int32_t *rays,
                                     uint32_t M, uint32_t N, float T_thresh, float *weights_sum, float *depth, float *image,
                                     void *stream) {
    FocDeviceGuard foc_guard_(stream, sigmas);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(rays && weights_sum && depth && image, FOC_E_INVALID, "composite_rays_train_forward: null pointer");
    FOC_REQUIRE(M == 0 || (sigmas && rgbs && deltas), FOC_E_INVALID, "composite_rays_train_forward: null input with M > 0");
    hipLaunchKernelGGL(k_composite_train_fwd, dim3(foc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream,
                       sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image);
    FOC_CHECK_LAUNCH("composite_rays_train_forward");
    return FOC_OK;
}

int foc_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image, const float *sigmas,
                                      const float *rgbs, const float *deltas, const int32_t *rays, const float *weights_sum,
                                      const float *image, uint32_t M, uint32_t N, float T_thresh, float *grad_sigmas,
                                      float *grad_rgbs, void *stream) {
    FocDeviceGuard foc_guard_(stream, grad_image);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(grad_image && rays && weights_sum && image, FOC_E_INVALID, "composite_rays_train_backward: null pointer");
    FOC_REQUIRE(M == 0 || (sigmas && rgbs && deltas && grad_sigmas && grad_rgbs), FOC_E_INVALID,
                "composite_rays_train_backward: null buffer with M > 0");
    hipLaunchKernelGGL(k_composite_train_bwd, dim3(foc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream,
                       grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh,
                       grad_sigmas, grad_rgbs);
    FOC_CHECK_LAUNCH("composite_rays_train_backward");
    return FOC_OK;
}

// the 16-lanes-per-ray and the one-ray-per-lane launch of R9 (foc_march_rays and foc_march_rays_two_phase)
static void rm_launch_row(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o, const float *rays_d,
                          const uint8_t *grid, const RmParams &p, const float *fars, float *xyzs, float *dirs, float *deltas, const float *noises, hipStream_t st) {
    hipLaunchKernelGGL(p.dt_min <= p.dt_max ? k_march_rays_row<true> : k_march_rays_row<false>, dim3(foc_div_up((uint64_t)n_alive * 16u, 256)), dim3(256), 0, st,
                       n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises);
}
static void rm_launch_lane(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o, const float *rays_d,
                           const uint8_t *grid, const RmParams &p, const float *fars, float *xyzs, float *dirs, float *deltas, const float *noises, hipStream_t st) {
    hipLaunchKernelGGL(k_march_rays, dim3(foc_div_up(n_alive, 64)), dim3(64), 0, st, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars, xyzs, dirs,
                       deltas, noises);
}

int foc_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                   const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                   const uint8_t *grid, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                   const float *noises, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    (void)nears;
    if (n_alive == 0) return FOC_OK;
    FOC_REQUIRE(rays_alive && rays_t && rays_o && rays_d && grid && fars && xyzs && dirs && deltas && noises, FOC_E_INVALID,
                "march_rays: null pointer");
    if (const int bad = rm_check_grid("march_rays", C, H, max_steps, ~0u, n_step)) return bad;
    const RmParams p = rm_make_params(bound, dt_gamma, max_steps, C, H);
    // 16 lanes per ray (k_march_rays_row) while the launch is latency-bound, one ray per lane beyond (FOC_MARCH_RAYS_ROW_MAX = most rays
    // the row form takes; 0 = never). Measured on the 800 x 800 occupancy render (profiles/, tools/quick_render_stats.sh; 549 launches,
    // most of them with > 262 144 rays alive and one sample per ray): one ray per lane 48.1 us average; the row form for every launch
    // 79.9 us (16x the cell evaluations where a ray needs one); row form up to 65 536 / 131 072 rays: 26-28 us on those launches (120 of
    // 549) against ~40 us. A lane form looking 8 lattice points ahead measured 53.8 us against 48.1 (round 3; removed): with
    // ~10 waves per SIMD the big launches are bound by the divergent walks' instruction count, not by their lookup chains.
    const long row_max = foc_opt(FOC_OPT_MARCH_RAYS_ROW_MAX);
    if ((long)n_alive <= row_max && n_step <= 16u) rm_launch_row(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises, (hipStream_t)stream);
    else rm_launch_lane(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises, (hipStream_t)stream);
    FOC_CHECK_LAUNCH("march_rays");
    return FOC_OK;
}

// which kernels foc_march_rays_two_phase takes for a burst of n_step samples of n_alive rays: 0 = the two phases, 1 = 16 lanes per ray (samples
// staged in LDS), 2 = one ray per lane, 3 = one ray per lane with the wave's samples staged in LDS. Measured on the 800 x 800 occupancy view
// (tools/time_occ_burst.py; 640 000 rays alive for most of it, bursts of 8): form 3 15.8 ms per view, form 1 17.4, form 2 18.2, form 0 18.8
// — with ten waves per SIMD the lanes' lookup chains hide each other and what counts is instructions and how the samples reach memory.
static int rm_burst_form(uint32_t n_step, uint32_t n_alive, bool rederive = false) {
    const int forced = foc_opt(FOC_OPT_OCC_MARCH_FORM);
    // the forms that generate a ray's lattice 16 points ahead (row, the walkers of the two phases) cannot re-derive t sample by sample
    if (rederive && n_step > 1u) return forced == 2 ? 2 : 3;
    if (forced >= 0) return forced;
    (void)n_alive;
    return n_step <= 2u ? 0 : 3;       // (16 lanes per ray for short lists, as foc_march_rays does: 14.7 against 14.0 ms per view — its samples stay ray-major)
}
/* 1 when foc_march_rays_two_phase writes every slot of every list entry for this burst length (the caller need not zero them) */
int foc_march_rays_two_phase_fills(uint32_t n_step, int flags) { const int f = rm_burst_form(n_step, 1u << 30, (flags & 2) != 0); return (f == 1 || f == 3) ? 1 : 0; }
/* 1 when foc_march_rays_two_phase honours flag bit 2 (sample-major output) for this call: the staged one-ray-per-lane kernel does */
int foc_march_rays_two_phase_sample_major(uint32_t n_alive, uint32_t n_step, int flags) { return rm_burst_form(n_step, n_alive, (flags & 2) != 0) == 3 ? 1 : 0; }

/* R9 in two phases (k_march_rays_first + k_march_walkers): `scratch` = int32[n_alive + 4], its first word the worklist length, which the
 * caller has zeroed on this stream. Same arguments and results as foc_march_rays. */
int foc_march_rays_two_phase(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                             const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                             const uint8_t *grid, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                             const float *noises, int32_t *scratch, int normalised, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    (void)nears;
    if (n_alive == 0) return FOC_OK;
    FOC_REQUIRE(rays_alive && rays_t && rays_o && rays_d && grid && fars && xyzs && dirs && deltas && noises && scratch, FOC_E_INVALID,
                "march_rays_two_phase: null pointer");
    if (const int bad = rm_check_grid("march_rays_two_phase", C, H, max_steps, 16u, n_step)) return bad;
    RmParams p = rm_make_params(bound, dt_gamma, max_steps, C, H);
    if (normalised & 1) p.norm_inv = 1.0f / (2.0f * bound);    // `xyzs` receives (x + bound) / (2 bound) as torch evaluates it: times the reciprocal (grid.py:149)
    p.rederive = (normalised & 2) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    // A burst of several samples per ray meets an empty cell on most rays (every one of them would be marched twice): the two phases are
    // for bursts of one or two samples. Longer bursts take one launch — one ray per lane with the wave's samples staged in LDS ("staged"),
    // 16 lanes per ray when few rays are left ("row"); FOC_OCC_MARCH_FORM = two | row | lane | staged overrides the choice (A/B runs, tests).
    const int form = rm_burst_form(n_step, n_alive, p.rederive != 0);
    if (form == 1) {
        rm_launch_row(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises, st);
        FOC_CHECK_LAUNCH("march_rays(row form)");
        return FOC_OK;
    } else if (form == 2) {
        rm_launch_lane(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises, st);
        FOC_CHECK_LAUNCH("march_rays(lane form)");
        return FOC_OK;
    } else if (form == 3) {
        hipLaunchKernelGGL(k_march_rays_staged, dim3(foc_div_up(n_alive, 64)), dim3(64), 64u * (5u * n_step + 4u) * sizeof(float), st, n_alive, n_step, rays_alive, rays_t,
                           rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises, (normalised & 4) ? 1 : 0);
        FOC_CHECK_LAUNCH("march_rays(staged lane form)");
        return FOC_OK;
    }
    int32_t *wl_count = scratch, *worklist = scratch + 4;
    hipLaunchKernelGGL(k_march_rays_first, dim3(foc_div_up(n_alive, 256)), dim3(256), 0, st, n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, grid, p, fars,
                       xyzs, dirs, deltas, noises, worklist, wl_count);
    FOC_CHECK_LAUNCH("march_rays(first visits)");
    const uint32_t row_max = (uint32_t)max(0, foc_opt(FOC_OPT_MARCH_RAYS_ROW_MAX));
    uint32_t blocks = foc_div_up((uint64_t)n_alive * 16u, 256);
    if (blocks > 4096u) blocks = 4096u;                     // 16 workgroups per CU; longer worklists are walked grid-stride
    hipLaunchKernelGGL(p.dt_min <= p.dt_max ? k_march_walkers<true> : k_march_walkers<false>, dim3(blocks), dim3(256), 0, st, n_alive, n_step, rays_alive, rays_t,
                       rays_o, rays_d, grid, p, fars, xyzs, dirs, deltas, noises, worklist, wl_count, row_max);
    FOC_CHECK_LAUNCH("march_rays(walkers)");
    return FOC_OK;
}

int foc_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                       const float *sigmas, const float *rgbs, const float *deltas, float *weights_sum, float *depth,
                       float *image, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    if (n_alive == 0) return FOC_OK;
    FOC_REQUIRE(rays_alive && rays_t && sigmas && rgbs && deltas && weights_sum && depth && image, FOC_E_INVALID,
                "composite_rays: null pointer");
    rm_launch_composite<false>(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, nullptr, (hipStream_t)stream);
    FOC_CHECK_LAUNCH("composite_rays");
    return FOC_OK;
}

int foc_composite_compact(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                          const float *sigmas, const float *rgbs, const float *deltas, float *weights_sum, float *depth,
                          float *image, int32_t *out, int32_t *n_out, int32_t *block_counts, int32_t *deaths, uint32_t deaths_base, uint32_t deaths_len,
                          int sample_major, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    FOC_REQUIRE(n_alive > 0 && rays_alive && rays_t && sigmas && rgbs && deltas && weights_sum && depth && image && out && n_out && block_counts, FOC_E_INVALID,
                "composite_compact: null pointer");
    FOC_REQUIRE(!deaths || deaths_len >= 1, FOC_E_INVALID, "composite_compact: empty death histogram");
    return rm_composite_compact(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, out, n_out, block_counts,
                                RmSide<false>{RmDeaths{deaths, deaths_base, deaths ? deaths_len : 1u, sample_major ? 1 : 0}}, (hipStream_t)stream);
}

int foc_compact_alive(const int32_t *rays_alive, uint32_t n_alive, int32_t *out, int32_t *n_out, int32_t *scratch, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    FOC_REQUIRE(n_out && scratch, FOC_E_INVALID, "compact_alive: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t nb = foc_div_up(n_alive, 1024);
    if (n_alive == 0) { (void)foc_zero_async(n_out, sizeof(int32_t), st); return FOC_OK; }
    FOC_REQUIRE(rays_alive && out, FOC_E_INVALID, "compact_alive: null pointer");
    hipLaunchKernelGGL(k_compact_count, dim3(nb), dim3(1024), 0, st, rays_alive, n_alive, scratch);
    FOC_CHECK_LAUNCH("compact_alive(count)");
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, st, scratch, nb, n_out);
    FOC_CHECK_LAUNCH("compact_alive(scan)");
    hipLaunchKernelGGL(k_compact_scatter, dim3(nb), dim3(1024), 0, st, rays_alive, n_alive, scratch, out);
    FOC_CHECK_LAUNCH("compact_alive(scatter)");
    return FOC_OK;
}

} // extern "C"

// foc_composite_compact with a second payload (common.h): aux [n_alive * n_step, 3] laid out as rgbs, accumulated into aux_image [N,3] with the
// weights of the first. Everything else — what is written, which rays are marked, counted and recorded in `deaths` — is foc_composite_compact's.
int composite_compact_aux(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t, const float *sigmas, const float *rgbs,
                          const float *aux, const float *deltas, float *weights_sum, float *depth, float *image, float *aux_image, int32_t *out, int32_t *n_out,
                          int32_t *block_counts, int32_t *deaths, uint32_t deaths_base, uint32_t deaths_len, int sample_major, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    FOC_REQUIRE(n_alive > 0 && rays_alive && rays_t && sigmas && rgbs && aux && deltas && weights_sum && depth && image && aux_image && out && n_out && block_counts,
                FOC_E_INVALID, "composite_compact_aux: null pointer");
    FOC_REQUIRE(!deaths || deaths_len >= 1, FOC_E_INVALID, "composite_compact_aux: empty death histogram");
    return rm_composite_compact(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image, out, n_out, block_counts,
                                RmSide<true>{RmDeaths{deaths, deaths_base, deaths ? deaths_len : 1u, sample_major ? 1 : 0}, aux, aux_image}, (hipStream_t)stream);
}
