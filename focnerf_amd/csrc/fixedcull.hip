// fixedcull.hip — occupancy-culled fixed-step fields for the multi-object combiner (no reference binding).
//
// The combiner's per-sample max-select (COMBINED.py best_densities_and_colors_v3) needs every object at the SAME T positions of the
// same rays, so an object cannot march its own ragged samples. What it can do is skip the field where its occupancy grid says
// "empty": keep the fixed positions of foc_fixed_sample (64-ray block order), test each against the bitfield, evaluate encoder +
// networks on the occupied ones only, and take sigma = 0 everywhere else — the approximation run_cuda's marching already makes.
//
//   foc_fixed_cull              positions (fs_common.h: the bits of k_fs_sample) -> cell (occ_cell.h: rm_cell's index, level from the
//                               position alone) -> one 64-bit ballot per (ray block, depth) row -> mask [R], offsets [R + 1], count
//   foc_fixed_cull_emit         the occupied samples' normalised positions and directions, compact, in row order
//   foc_fixed_field_pack_culled k_fs_render_infer's pass (fs_infer_tile) fed from the compact sigma / rgb through mask + offsets
//
//   foc_fixed_cull_placed / foc_fixed_cull_emit_placed / foc_fixed_field_pack_culled_gain
//                               the same three for an object PLACED in a scene (rotation, uniform scale, translation): the world sample
//                               is mapped into the object's frame in front of the cell test (FcPlace, 12 coefficients + the object's box in
//                               the kernel argument block: scalar registers, no loads), and the sample's sigma takes the gain 1 / scale
//
// Slots are reserved by prefix sum, never by atomics: the compact list is the same list on every run (as march_rays_train's is).
// Shape: one wave per GROUP of up to 64 consecutive rows of one ray block — the lanes are the block's 64 rays throughout, so a lane
// loads its ray once; lane j keeps the ballot of row j, and a group's 64 mask words / offsets leave as one coalesced store each.
#include <cmath>
#include "common.h"
#include "fs_common.h"
#include "occ_cell.h"
#include "fc_place.h"

#define FC_GROUP 64u                       // rows per wave

struct FcRay { float ox, oy, oz, dx, dy, dz; FsGeom g; };

__device__ __forceinline__ FcRay fc_ray(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ nears,
                                        const float *__restrict__ fars, uint32_t n, uint32_t T) {
    FcRay r;
    r.ox = rays_o[n * 3]; r.oy = rays_o[n * 3 + 1]; r.oz = rays_o[n * 3 + 2];
    r.dx = rays_d[n * 3]; r.dy = rays_d[n * 3 + 1]; r.dz = rays_d[n * 3 + 2];
    r.g = fs_geom(nears, fars, n, T);
    return r;
}

// group -> (ray block, first depth, rows in the group, first row)
struct FcGroup { uint32_t blk, i0, rows; uint64_t row0; };
__device__ __forceinline__ FcGroup fc_group(uint32_t g, uint32_t T) {
    const uint32_t gt = (T + FC_GROUP - 1) / FC_GROUP;
    FcGroup q;
    q.blk = g / gt; q.i0 = (g % gt) * FC_GROUP;
    q.rows = min(FC_GROUP, T - q.i0);
    q.row0 = (uint64_t)q.blk * T + q.i0;
    return q;
}

// ---------------------------------------------------------------- pass 1: ballots, per-group exclusive offsets, group totals
template <bool PLACED>
__global__ void __launch_bounds__(256) k_fc_mask(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ nears,
                                                 const float *__restrict__ fars, const float *__restrict__ aabb, uint32_t N, uint32_t T, FcGrid G,
                                                 FcPlace P, uint32_t n_groups, uint64_t *__restrict__ mask, uint32_t *__restrict__ offsets,
                                                 uint32_t *__restrict__ group_total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_groups) return;
    const FcGroup q = fc_group(g, T);
    const uint32_t n = q.blk * FS_RAY_BLOCK + lane;
    const bool own = n < N;                                    // the padding lanes of the last block never set a bit
    const FcRay r = fc_ray(rays_o, rays_d, nears, fars, own ? n : N - 1, T);
    const FsBox box = fs_box(aabb);
    uint64_t mine = 0;
    // four rows per step: their four bitfield loads are in flight together before the first ballot waits for one
    for (uint32_t j0 = 0; j0 < q.rows; j0 += 4) {
        bool occ[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const float z = fs_z(r.g, min(q.i0 + j0 + u, T - 1), T, nullptr, 0);
            float x, y, w;
            fs_point(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, z, box, x, y, w);
            if (PLACED) {                                      // the bitfield is read for the samples inside the object's box only
                float qx, qy, qz;
                fc_to_object(P, x, y, w, qx, qy, qz);
                occ[u] = own && j0 + u < q.rows && fc_inside(P, qx, qy, qz) && fc_occupied(G, qx, qy, qz);
            } else {
                occ[u] = fc_occupied(G, x, y, w) && own && j0 + u < q.rows;
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < 4; u++) {
            const uint64_t b = __ballot(occ[u]);
            if (lane == j0 + u) mine = b;
        }
    }
    const int cnt = __popcll(mine);
    const int incl = wave_incl_sum_i(cnt, (int)lane);
    if (lane < q.rows) { mask[q.row0 + lane] = mine; offsets[q.row0 + lane] = (uint32_t)(incl - cnt); }
    if (lane == 63) group_total[g] = (uint32_t)incl;
}

// ---------------------------------------------------------------- pass 2: exclusive scan of the group totals (one workgroup), in place
__global__ void __launch_bounds__(1024) k_fc_scan(uint32_t *__restrict__ group_total, uint32_t n_groups, uint32_t *__restrict__ offsets_end,
                                                  uint32_t *__restrict__ count) {
    __shared__ int wave_tot[16];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_groups; base += 1024) {
        const uint32_t k = base + threadIdx.x;
        const int v = k < n_groups ? (int)group_total[k] : 0;
        const int incl = wave_incl_sum_i(v, (int)lane);
        if (lane == 63) wave_tot[wv] = incl;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int u = 0; u < 16; u++) { const int t = wave_tot[u]; all += t; if (u < (int)wv) before += t; }
        if (k < n_groups) group_total[k] = carry + (uint32_t)(before + incl - v);
        carry += (uint32_t)all;
        __syncthreads();
    }
    if (threadIdx.x == 0) { *offsets_end = carry; *count = carry; }
}

// ---------------------------------------------------------------- pass 3: offsets[row] += base of the row's group
__global__ void __launch_bounds__(256) k_fc_finish(const uint32_t *__restrict__ group_base, uint32_t T, uint64_t n_rows, uint32_t *__restrict__ offsets) {
    const uint32_t gt = (T + FC_GROUP - 1) / FC_GROUP;
    for (uint64_t row = (uint64_t)blockIdx.x * 256 + threadIdx.x; row < n_rows; row += (uint64_t)gridDim.x * 256) {
        const uint32_t blk = (uint32_t)(row / T), i = (uint32_t)(row - (uint64_t)blk * T);
        offsets[row] += group_base[blk * gt + i / FC_GROUP];
    }
}

// ---------------------------------------------------------------- emit: compact positions and directions
template <bool PLACED>
__global__ void __launch_bounds__(256) k_fc_emit(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ nears,
                                                 const float *__restrict__ fars, const float *__restrict__ aabb, uint32_t N, uint32_t T, float bound,
                                                 FcPlace P, uint32_t n_groups, const uint64_t *__restrict__ mask, const uint32_t *__restrict__ offsets,
                                                 uint32_t capacity, float *__restrict__ enc_in_c, float *__restrict__ dirs_c) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_groups) return;
    const FcGroup q = fc_group(g, T);
    const uint64_t mine = lane < q.rows ? mask[q.row0 + lane] : 0ull;
    if (__ballot(mine != 0) == 0) return;                      // an empty group (most of a 5 % occupied box)
    const uint32_t my_off = lane < q.rows ? offsets[q.row0 + lane] : 0u;
    const uint32_t n = q.blk * FS_RAY_BLOCK + lane;
    const FcRay r = fc_ray(rays_o, rays_d, nears, fars, n < N ? n : N - 1, T);
    const FsBox box = fs_box(aabb);
    const float two_b = 2 * bound;
    const uint64_t below = (1ull << lane) - 1ull;
    float ex = r.dx, ey = r.dy, ez = r.dz;                     // the emitted direction: the ray's, once per ray; placed: turned and scaled, not renormalised
    if (PLACED) {
        ex = P.dir_scale * ((P.a00 * r.dx + P.a01 * r.dy) + P.a02 * r.dz);
        ey = P.dir_scale * ((P.a10 * r.dx + P.a11 * r.dy) + P.a12 * r.dz);
        ez = P.dir_scale * ((P.a20 * r.dx + P.a21 * r.dy) + P.a22 * r.dz);
    }
    for (uint32_t j = 0; j < q.rows; j++) {
        const uint64_t m = ((uint64_t)(uint32_t)__shfl((int)(mine >> 32), (int)j, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)mine, (int)j, 64);
        if (m == 0) continue;                                  // wave-uniform
        const uint32_t off = (uint32_t)__shfl((int)my_off, (int)j, 64);
        const uint32_t slot = off + (uint32_t)__popcll(m & below);
        if (((m >> lane) & 1ull) && slot < capacity) {
            const float z = fs_z(r.g, q.i0 + j, T, nullptr, 0);
            float x, y, w;
            fs_point(r.ox, r.oy, r.oz, r.dx, r.dy, r.dz, z, box, x, y, w);
            if (PLACED) {
                float qx, qy, qz;
                fc_to_object(P, x, y, w, qx, qy, qz);
                x = qx; y = qy; w = qz;
            }
            float *e = enc_in_c + (uint64_t)slot * 3, *d = dirs_c + (uint64_t)slot * 3;
            e[0] = fs_norm(x, bound, two_b); e[1] = fs_norm(y, bound, two_b); e[2] = fs_norm(w, bound, two_b);
            d[0] = ex; d[1] = ey; d[2] = ez;
        }
    }
}

// ---------------------------------------------------------------- culled pack: k_fs_render_infer<PACK> fed through mask + offsets
// One wave per ray, sample i on the lane: the row's mask word and offset (consecutive rows on consecutive lanes), the ray's bit, its
// slot in the compact arrays; an unoccupied sample enters the pass as sigma = 0, rgb = 0.
template <bool GAIN>
__global__ void __launch_bounds__(256) k_fc_pack(const float *__restrict__ sigma_c, const float *__restrict__ rgb_c, const uint64_t *__restrict__ mask,
                                                 const uint32_t *__restrict__ offsets, uint32_t m_occ, const float *__restrict__ nears,
                                                 const float *__restrict__ fars, uint32_t N, uint32_t T, float density_scale, float thresh,
                                                 float sigma_gain, float4 *__restrict__ field4) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= N) return;
    const FsGeom g = fs_geom(nears, fars, n, T);
    const uint32_t bit = n % FS_RAY_BLOCK;
    const uint64_t below = (1ull << bit) - 1ull;
    const uint64_t row0 = (uint64_t)(n / FS_RAY_BLOCK) * T;
    FsRayAcc a = {1.0f, 0, 0, 0, 0, 0};
    for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t i = base + lane;
        const uint64_t row = row0 + (i < T ? i : T - 1);
        const uint64_t m = mask[row];
        const uint32_t slot = offsets[row] + (uint32_t)__popcll(m & below);
        float sigma = 0, c0 = 0, c1 = 0, c2 = 0;
        if (i < T && ((m >> bit) & 1ull) && slot < m_occ) {
            sigma = sigma_c[slot];
            if (GAIN) sigma *= sigma_gain;                     // a placed object's density in world units: one fp32 multiply, in front of the weights
            c0 = rgb_c[(uint64_t)slot * 3]; c1 = rgb_c[(uint64_t)slot * 3 + 1]; c2 = rgb_c[(uint64_t)slot * 3 + 2];
        }
        fs_infer_tile<true>(a, g, n, i, lane, T, sigma, c0, c1, c2, nullptr, density_scale, thresh, nullptr, field4, nullptr);
    }
}

static inline uint32_t fc_groups(uint32_t N, uint32_t T) { return foc_div_up(N, FS_RAY_BLOCK) * foc_div_up(T, FC_GROUP); }

// foc_fixed_cull and foc_fixed_cull_placed: one set of refusals, one launch sequence (`who` names the entry point in the messages)
template <bool PLACED>
static int fc_cull(const char *who, const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb, uint32_t N,
                   uint32_t T, const FcPlace &P, float bound, const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size, uint64_t *mask,
                   uint32_t *offsets, uint32_t *count, void *scratch, uint64_t scratch_bytes, void *stream) {
    FOC_REQUIRE(offsets && count, FOC_E_INVALID, "%s: null pointer", who);
    hipStream_t st = (hipStream_t)stream;
    if (N == 0) {                                              // no rows: offsets [1] = {0}, count = 0
        if (foc_zero_async(offsets, sizeof(uint32_t), st) != hipSuccess || foc_zero_async(count, sizeof(uint32_t), st) != hipSuccess) {
            foc_set_error("%s: zero fill failed", who);
            return FOC_E_LAUNCH;
        }
        return FOC_OK;
    }
    FOC_REQUIRE(rays_o && rays_d && nears && fars && aabb && bitfield && mask && scratch, FOC_E_INVALID, "%s: null pointer", who);
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "%s: T must be >= 2", who);
    FOC_REQUIRE(cascade >= 1 && cascade <= 16, FOC_E_INVALID, "%s: cascade must be 1..16 (got %u)", who, cascade);
    FOC_REQUIRE(grid_size >= 2 && grid_size <= 1024 && (grid_size & (grid_size - 1)) == 0, FOC_E_INVALID,
                "%s: grid_size must be a power of two in 2..1024 (got %u)", who, grid_size);
    FOC_REQUIRE((uint64_t)cascade * grid_size * grid_size * grid_size < (1ull << 32), FOC_E_INVALID, "%s: cascade * grid_size^3 must fit 32 bits", who);
    const uint64_t n_rows = (uint64_t)foc_div_up(N, FS_RAY_BLOCK) * T;
    FOC_REQUIRE(n_rows * FS_RAY_BLOCK < (1ull << 31), FOC_E_INVALID, "%s: ceil(N/64)*64*T must stay below 2^31 (the offsets are uint32, their scan runs on int lanes)", who);
    FOC_REQUIRE(scratch_bytes >= foc_fixed_cull_scratch_bytes(N, T), FOC_E_INVALID, "%s: scratch of %llu bytes, foc_fixed_cull_scratch_bytes(%u, %u) asks for %llu",
                who, (unsigned long long)scratch_bytes, N, T, (unsigned long long)foc_fixed_cull_scratch_bytes(N, T));
    FOC_REQUIRE((((uintptr_t)mask) & 7) == 0, FOC_E_INVALID, "%s: mask must be 8-byte aligned", who);
    const uint32_t n_groups = fc_groups(N, T);
    const uint64_t cells = (uint64_t)cascade * grid_size * grid_size * grid_size;
    FcGrid G;
    G.bits = bitfield; G.bound = bound; G.Cf = (float)cascade; G.Hm1 = (float)(grid_size - 1);
    G.H3 = (float)((uint64_t)grid_size * grid_size * grid_size); G.H = grid_size; G.n_cells = (uint32_t)cells;
    uint32_t *group_total = reinterpret_cast<uint32_t *>(scratch);
    hipLaunchKernelGGL(k_fc_mask<PLACED>, dim3(foc_div_up(n_groups, 4)), dim3(256), 0, st, rays_o, rays_d, nears, fars, aabb, N, T, G, P, n_groups, mask, offsets,
                       group_total);
    FOC_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_fc_scan, dim3(1), dim3(1024), 0, st, group_total, n_groups, offsets + n_rows, count);
    FOC_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_fc_finish, dim3(foc_grid_1d(n_rows, 256)), dim3(256), 0, st, group_total, T, n_rows, offsets);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

template <bool PLACED>
static int fc_emit(const char *who, const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb, uint32_t N,
                   uint32_t T, const FcPlace &P, float bound, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ, float *enc_in_c, float *dirs_c,
                   void *stream) {
    if (N == 0 || m_occ == 0) return FOC_OK;
    FOC_REQUIRE(rays_o && rays_d && nears && fars && aabb && mask && offsets && enc_in_c && dirs_c, FOC_E_INVALID, "%s: null pointer", who);
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "%s: T must be >= 2", who);
    const uint32_t n_groups = fc_groups(N, T);
    hipLaunchKernelGGL(k_fc_emit<PLACED>, dim3(foc_div_up(n_groups, 4)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, nears, fars, aabb, N, T, bound, P,
                       n_groups, mask, offsets, m_occ, enc_in_c, dirs_c);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

template <bool GAIN>
static int fc_pack(const char *who, const float *sigma_c, const float *rgb_c, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ,
                   const float *nears, const float *fars, uint32_t N, uint32_t T, float density_scale, float thresh, float sigma_gain, float *field4,
                   void *stream) {
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(mask && offsets && nears && fars && field4, FOC_E_INVALID, "%s: null pointer", who);
    FOC_REQUIRE(m_occ == 0 || (sigma_c && rgb_c), FOC_E_INVALID, "%s: null sigma / rgb with %u occupied samples", who, m_occ);
    FOC_REQUIRE(((uintptr_t)field4 & 15) == 0, FOC_E_INVALID, "%s: field4 must be 16-byte aligned", who);
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "%s: T must be >= 2", who);
    hipLaunchKernelGGL(k_fc_pack<GAIN>, dim3(foc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream, sigma_c, rgb_c, mask, offsets, m_occ, nears, fars, N, T,
                       density_scale, thresh, sigma_gain, (float4 *)field4);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

extern "C" {

uint64_t foc_fixed_cull_scratch_bytes(uint32_t N, uint32_t T) {
    return (uint64_t)fc_groups(N, T) * sizeof(uint32_t);
}

int foc_fixed_cull(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb, uint32_t N, uint32_t T,
                   float bound, const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size, uint64_t *mask, uint32_t *offsets, uint32_t *count,
                   void *scratch, uint64_t scratch_bytes, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    return fc_cull<false>("fixed_cull", rays_o, rays_d, nears, fars, aabb, N, T, FcPlace{}, bound, bitfield, cascade, grid_size, mask, offsets, count, scratch,
                          scratch_bytes, stream);
}

int foc_fixed_cull_emit(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb, uint32_t N, uint32_t T,
                        float bound, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ, float *enc_in_c, float *dirs_c, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    return fc_emit<false>("fixed_cull_emit", rays_o, rays_d, nears, fars, aabb, N, T, FcPlace{}, bound, mask, offsets, m_occ, enc_in_c, dirs_c, stream);
}

int foc_fixed_field_pack_culled(const float *sigma_c, const float *rgb_c, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ,
                                const float *nears, const float *fars, uint32_t N, uint32_t T, float density_scale, float thresh, float *field4,
                                void *stream) {
    FocDeviceGuard foc_guard_(stream, mask);
    return fc_pack<false>("fixed_field_pack_culled", sigma_c, rgb_c, mask, offsets, m_occ, nears, fars, N, T, density_scale, thresh, 1.0f, field4, stream);
}

int foc_fixed_cull_placed(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *scene_aabb, uint32_t N, uint32_t T,
                          const float *world_to_object, const float *obj_aabb, float bound, const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size,
                          uint64_t *mask, uint32_t *offsets, uint32_t *count, void *scratch, uint64_t scratch_bytes, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    FOC_REQUIRE(world_to_object && obj_aabb, FOC_E_INVALID, "fixed_cull_placed: null world_to_object / obj_aabb (host arrays of 12 and 6 floats)");
    FOC_REQUIRE(fc_all_finite(world_to_object, 12) && fc_all_finite(obj_aabb, 6), FOC_E_INVALID, "fixed_cull_placed: non-finite world_to_object / obj_aabb");
    return fc_cull<true>("fixed_cull_placed", rays_o, rays_d, nears, fars, scene_aabb, N, T, fc_place(world_to_object, obj_aabb, 1.0f), bound, bitfield, cascade,
                         grid_size, mask, offsets, count, scratch, scratch_bytes, stream);
}

int foc_fixed_cull_emit_placed(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *scene_aabb, uint32_t N,
                               uint32_t T, const float *world_to_object, float dir_scale, float bound, const uint64_t *mask, const uint32_t *offsets,
                               uint32_t m_occ, float *enc_in_c, float *dirs_c, void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_o);
    FOC_REQUIRE(world_to_object, FOC_E_INVALID, "fixed_cull_emit_placed: null world_to_object (a host array of 12 floats)");
    FOC_REQUIRE(fc_all_finite(world_to_object, 12) && std::isfinite(dir_scale), FOC_E_INVALID, "fixed_cull_emit_placed: non-finite world_to_object / dir_scale");
    const float no_box[6] = {0, 0, 0, 0, 0, 0};               // the emit pass reads the mask: the box is not consulted again
    return fc_emit<true>("fixed_cull_emit_placed", rays_o, rays_d, nears, fars, scene_aabb, N, T, fc_place(world_to_object, no_box, dir_scale), bound, mask,
                         offsets, m_occ, enc_in_c, dirs_c, stream);
}

int foc_fixed_field_pack_culled_gain(const float *sigma_c, const float *rgb_c, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ,
                                     const float *nears, const float *fars, uint32_t N, uint32_t T, float density_scale, float thresh, float sigma_gain,
                                     float *field4, void *stream) {
    FocDeviceGuard foc_guard_(stream, mask);
    FOC_REQUIRE(std::isfinite(sigma_gain) && sigma_gain > 0, FOC_E_INVALID, "fixed_field_pack_culled_gain: sigma_gain must be finite and > 0 (got %g)", (double)sigma_gain);
    return fc_pack<true>("fixed_field_pack_culled_gain", sigma_c, rgb_c, mask, offsets, m_occ, nears, fars, N, T, density_scale, thresh, sigma_gain, field4, stream);
}

} // extern "C"
