// mesh.hip — triangle meshes on the device: marching cubes on a float32 volume, and the lattice cull / scatter that fill such a volume from
// per-object networks (no reference binding: the reference samples the lattice in 128^3 pieces through the host and calls PyMCubes).
//
//   foc_mc_count            one pass over the lattice points: the owned crossed edges (0..3) and the triangles of the cube anchored at each
//                           point -> one 64-bit ballot per 64 points and axis, per-chunk exclusive offsets, the three totals
//   foc_mc_emit             vertices (one per crossed lattice edge, shared by the cubes around it by construction), optional normals, and
//                           indexed triangles, each at its offset
//   foc_lattice_cull / _emit  which points of a lattice slab lie in an object's box and in an occupied cell (fc_place.h: the placement and the
//                           cell test of the fixed-step cull), and their compact position list in lattice order
//   foc_volume_scatter_max  volume = max(volume, gain * sigma) at those points
//   foc_points_cull / _emit the same cull for a LIST of points (the mask and emit kernels are templates over where a point comes from), emitting
//                           the object-frame position and / or the encoder's coordinates: the front of the scene point query (query.py)
//   foc_surface_frame       per compacted point the unit normal of the density gradient (unit_normal.h, shared with normals.hip), rotated
//                           into the world, and the direction the colour network is asked about (against the normal, or from an eye point)
//   foc_scene_select        the scatter with a payload: the object with the strictly largest gained sigma keeps index, colour and normal
//
// Slots come from prefix sums, never from atomics: the same mesh on every run, in both deterministic modes. Shape, as fixedcull.hip: a
// CHUNK is 64 consecutive points (one ballot word), one wave owns a GROUP of up to 64 consecutive chunks; lane j keeps what chunk j
// produced, so a group's words and offsets leave as one coalesced store each. One workgroup scans the group totals, a last pass adds
// each group's base. All of it is memory-bound (4 bytes read per point; the emit pass skips chunks without surface from their words).
#include <cmath>
#include "common.h"
#include "occ_cell.h"
#include "fc_place.h"
#include "ms_scan.h"
#include "fs_common.h"
#include "unit_normal.h"
#define MC_TABLE_ATTR __device__
#include "mc_table.h"

#define MC_MAX_POINTS (1ull << 29)

struct McDim { uint32_t nx, ny, nz, sx, n; };          // sx = ny * nz: the stride of x (y: nz, z: 1)

// the cube anchored at lattice point i: its eight corner values (corner c at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1); a corner past the
// lattice repeats the value before it and is never used), the point's coordinates and what exists there
struct McCell { float u[8]; uint32_t x, y, z; bool valid, ex, ey, ez; };

__device__ __forceinline__ McCell mc_cell(const float *__restrict__ vol, const McDim &D, uint32_t i) {
    McCell c;
    c.valid = i < D.n;
    i = min(i, D.n - 1u);
    c.x = i / D.sx;
    const uint32_t r = i - c.x * D.sx;
    c.y = r / D.nz;
    c.z = r - c.y * D.nz;
    c.ex = c.valid && c.x + 1 < D.nx; c.ey = c.valid && c.y + 1 < D.ny; c.ez = c.valid && c.z + 1 < D.nz;
    const uint32_t dx = c.x + 1 < D.nx ? D.sx : 0u, dy = c.y + 1 < D.ny ? D.nz : 0u, dz = c.z + 1 < D.nz ? 1u : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 8; k++) c.u[k] = vol[i + ((k & 1) ? dx : 0u) + ((k & 2) ? dy : 0u) + ((k & 4) ? dz : 0u)];
    return c;
}
// bit c set iff corner c is inside (u >= thr; a NaN is outside); 0 where no cube is anchored
__device__ __forceinline__ uint32_t mc_case(const McCell &c, float thr) {
    uint32_t k = 0;
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) k |= (c.u[q] >= thr ? 1u : 0u) << q;
    return (c.ex && c.ey && c.ez) ? k : 0u;
}
__device__ __forceinline__ bool mc_crossed(float u0, float u1, float thr) { return (u0 >= thr) != (u1 >= thr); }
__device__ __forceinline__ bool mc_finite(float v) { return fabsf(v) <= 3.402823466e38f; }     // false for NaN

// the workspace of foc_mc_count / foc_mc_emit: W chunks, G groups
struct McWs { uint32_t *totals; uint64_t *mx, *my, *mz, *mt; uint32_t *voff, *toff, *gv, *gt, *gb; };

// ---------------------------------------------------------------- marching cubes, pass 1
__global__ void __launch_bounds__(256) k_mc_count(const float *__restrict__ vol, McDim D, float thr, uint32_t W, uint32_t n_groups, McWs ws) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_groups) return;
    const uint32_t c0 = g * MS_GROUP, chunks = min(MS_GROUP, W - c0);
    uint64_t kx = 0, ky = 0, kz = 0, kt = 0;
    int nv = 0, nt = 0;
    bool bad_any = false;
    for (uint32_t j = 0; j < chunks; j++) {
        const McCell c = mc_cell(vol, D, (c0 + j) * 64u + lane);
        const bool cx = c.ex && mc_crossed(c.u[0], c.u[1], thr), cy = c.ey && mc_crossed(c.u[0], c.u[2], thr), cz = c.ez && mc_crossed(c.u[0], c.u[4], thr);
        const bool bad = ((cx || cy || cz) && !mc_finite(c.u[0])) || (cx && !mc_finite(c.u[1])) || (cy && !mc_finite(c.u[2])) || (cz && !mc_finite(c.u[4]));
        const int ntri = (int)MC_NTRI[mc_case(c, thr)];
        const uint64_t bx = __ballot(cx), by = __ballot(cy), bz = __ballot(cz), bt = __ballot(ntri > 0);
        const int tsum = wave_sum_i(ntri);
        bad_any = bad_any || __ballot(bad) != 0;
        if (lane == j) { kx = bx; ky = by; kz = bz; kt = bt; nv = __popcll(bx) + __popcll(by) + __popcll(bz); nt = tsum; }
    }
    const int vi = wave_incl_sum_i(nv, (int)lane), ti = wave_incl_sum_i(nt, (int)lane);
    if (lane < chunks) {
        const uint32_t c = c0 + lane;
        ws.mx[c] = kx; ws.my[c] = ky; ws.mz[c] = kz; ws.mt[c] = kt;
        ws.voff[c] = (uint32_t)(vi - nv); ws.toff[c] = (uint32_t)(ti - nt);
    }
    if (lane == 63) { ws.gv[g] = (uint32_t)vi; ws.gt[g] = (uint32_t)ti; ws.gb[g] = bad_any ? 1u : 0u; }
}

// passes 2 and 3 (k_ms_scan: one workgroup scans the group totals; k_ms_finish: offsets[chunk] += base of the chunk's group): ms_scan.h

// ---------------------------------------------------------------- marching cubes, emit
// number of the vertex on the edge of axis `a` owned by lattice point q: (owner, axis) order inside the owner's chunk, after the chunk's offset
__device__ __forceinline__ uint32_t mc_vid(const McWs &ws, uint32_t q, uint32_t a) {
    const uint32_t c = q >> 6, l = q & 63;
    const uint64_t X = ws.mx[c], Y = ws.my[c], Z = ws.mz[c], below = (1ull << l) - 1ull;
    uint32_t id = ws.voff[c] + (uint32_t)(__popcll(X & below) + __popcll(Y & below) + __popcll(Z & below));
    if (a > 0) id += (uint32_t)((X >> l) & 1ull);
    if (a > 1) id += (uint32_t)((Y >> l) & 1ull);
    return id;
}

// gradient of u at (x, y, z) in lattice units: central differences, one-sided on the border
__device__ __forceinline__ void mc_grad(const float *__restrict__ vol, const McDim &D, uint32_t x, uint32_t y, uint32_t z, float &gx, float &gy, float &gz) {
    const uint32_t i = x * D.sx + y * D.nz + z;
    const uint32_t xh = min(x + 1, D.nx - 1) - x, xl = x - (max(x, 1u) - 1u);
    const uint32_t yh = min(y + 1, D.ny - 1) - y, yl = y - (max(y, 1u) - 1u);
    const uint32_t zh = min(z + 1, D.nz - 1) - z, zl = z - (max(z, 1u) - 1u);
    gx = (vol[i + xh * D.sx] - vol[i - xl * D.sx]) * (xh + xl == 2 ? 0.5f : 1.0f);
    gy = (vol[i + yh * D.nz] - vol[i - yl * D.nz]) * (yh + yl == 2 ? 0.5f : 1.0f);
    gz = (vol[i + zh] - vol[i - zl]) * (zh + zl == 2 ? 0.5f : 1.0f);
}

struct McMap { float ox, oy, oz, sx, sy, sz; };        // world = fmaf(lattice, spacing, origin) per axis

template <bool NORMALS>
__device__ __forceinline__ void mc_vertex(const float *__restrict__ vol, const McDim &D, const McCell &c, uint32_t axis, float u1, float thr, const McMap &M,
                                          uint32_t id, float *__restrict__ vertices, float *__restrict__ normals) {
    const float t = (thr - c.u[0]) / (u1 - c.u[0]);
    float px = (float)c.x, py = (float)c.y, pz = (float)c.z;
    if (axis == 0) px += t;
    if (axis == 1) py += t;
    if (axis == 2) pz += t;
    float *v = vertices + (uint64_t)id * 3;
    v[0] = fmaf(px, M.sx, M.ox); v[1] = fmaf(py, M.sy, M.oy); v[2] = fmaf(pz, M.sz, M.oz);
    if (NORMALS) {
        float ax, ay, az, bx, by, bz;
        mc_grad(vol, D, c.x, c.y, c.z, ax, ay, az);
        mc_grad(vol, D, c.x + (axis == 0), c.y + (axis == 1), c.z + (axis == 2), bx, by, bz);
        const float gx = (ax + t * (bx - ax)) / M.sx, gy = (ay + t * (by - ay)) / M.sy, gz = (az + t * (bz - az)) / M.sz;
        const float len = sqrtf(gx * gx + gy * gy + gz * gz);
        const float inv = len > 0 ? -1.0f / len : 0.0f;
        float *nrm = normals + (uint64_t)id * 3;
        nrm[0] = len > 0 ? gx * inv : 0.0f; nrm[1] = len > 0 ? gy * inv : 0.0f; nrm[2] = len > 0 ? gz * inv : 0.0f;
    }
}

template <bool NORMALS>
__global__ void __launch_bounds__(256) k_mc_emit(const float *__restrict__ vol, McDim D, float thr, uint32_t W, uint32_t n_groups, McWs ws, McMap M,
                                                 float *__restrict__ vertices, float *__restrict__ normals, int32_t *__restrict__ triangles) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_groups) return;
    const uint32_t c0 = g * MS_GROUP, chunks = min(MS_GROUP, W - c0);
    const bool have = lane < chunks;
    const uint64_t kx = have ? ws.mx[c0 + lane] : 0ull, ky = have ? ws.my[c0 + lane] : 0ull, kz = have ? ws.mz[c0 + lane] : 0ull,
                   kt = have ? ws.mt[c0 + lane] : 0ull;
    if (__ballot((kx | ky | kz | kt) != 0) == 0) return;       // a group without surface (most of a volume)
    const uint32_t kv = have ? ws.voff[c0 + lane] : 0u, kf = have ? ws.toff[c0 + lane] : 0u;
    const uint32_t v_total = ws.totals[0], f_total = ws.totals[1];      // what the caller sized the outputs by: nothing is written past them
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t j = 0; j < chunks; j++) {
        const uint64_t bx = ms_shfl64(kx, j), by = ms_shfl64(ky, j), bz = ms_shfl64(kz, j), bt = ms_shfl64(kt, j);
        if ((bx | by | bz | bt) == 0) continue;                // wave-uniform
        const uint32_t voff = (uint32_t)__shfl((int)kv, (int)j, 64), toff = (uint32_t)__shfl((int)kf, (int)j, 64);
        const uint32_t i = (c0 + j) * 64u + lane;
        const McCell c = mc_cell(vol, D, i);
        uint32_t id = voff + (uint32_t)(__popcll(bx & below) + __popcll(by & below) + __popcll(bz & below));
        if ((bx >> lane) & 1ull) { if (id < v_total) mc_vertex<NORMALS>(vol, D, c, 0, c.u[1], thr, M, id, vertices, normals); id++; }
        if ((by >> lane) & 1ull) { if (id < v_total) mc_vertex<NORMALS>(vol, D, c, 1, c.u[2], thr, M, id, vertices, normals); id++; }
        if ((bz >> lane) & 1ull) { if (id < v_total) mc_vertex<NORMALS>(vol, D, c, 2, c.u[4], thr, M, id, vertices, normals); id++; }
        if (bt == 0) continue;
        const uint32_t kase = mc_case(c, thr);
        const int ntri = (int)MC_NTRI[kase];
        const uint32_t slot0 = toff + (uint32_t)(wave_incl_sum_i(ntri, (int)lane) - ntri);
        for (int k = 0; k < ntri; k++) {
            if (slot0 + (uint32_t)k >= f_total) break;
            int32_t *tri = triangles + (uint64_t)(slot0 + (uint32_t)k) * 3;
#pragma unroll
            for (int v = 0; v < 3; v++) {
                const uint32_t e = (uint32_t)MC_TRI[kase][3 * k + v];
                const uint32_t cn = MC_EDGE_CORNER[e];
                const uint32_t q = i + ((cn & 1) ? D.sx : 0u) + ((cn & 2) ? D.nz : 0u) + ((cn & 4) ? 1u : 0u);      // inside the lattice: the cube exists
                tri[v] = (int32_t)mc_vid(ws, q, e >> 2);
            }
        }
    }
}

// ---------------------------------------------------------------- lattice cull, point cull
// Where a point comes from: the slab of a separable lattice (per-axis coordinates) or a list [count,3]. A source is wave-uniform and passed
// by value; `at` clamps past the end (the caller masks such a lane out).
struct LcLattice {
    const float *xs, *ys, *zs;
    uint32_t ry, rz, first, count;
    __device__ __forceinline__ void at(uint32_t local, float &x, float &y, float &z) const {
        const uint32_t i = first + min(local, count - 1u);
        const uint32_t s = ry * rz, ix = i / s, r = i - ix * s, iy = r / rz;
        x = xs[ix]; y = ys[iy]; z = zs[r - iy * rz];
    }
};
struct LcList {
    const float *points;
    uint32_t count;
    __device__ __forceinline__ void at(uint32_t local, float &x, float &y, float &z) const {
        const float *p = points + (uint64_t)min(local, count - 1u) * 3;
        x = p[0]; y = p[1]; z = p[2];
    }
};

template <bool PLACED, bool GRID, class SRC>
__global__ void __launch_bounds__(256) k_lc_mask(SRC S, FcGrid G, FcPlace P, uint32_t W, uint32_t n_groups, uint64_t *__restrict__ mask,
                                                 uint32_t *__restrict__ offsets, uint32_t *__restrict__ group_total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_groups) return;
    const uint32_t c0 = g * MS_GROUP, chunks = min(MS_GROUP, W - c0);
    uint64_t mine = 0;
    for (uint32_t j = 0; j < chunks; j++) {
        const uint32_t local = (c0 + j) * 64u + lane;
        float x, y, z;
        S.at(local, x, y, z);
        bool occ = local < S.count;
        if (PLACED) {
            float qx, qy, qz;
            fc_to_object(P, x, y, z, qx, qy, qz);
            occ = occ && fc_inside(P, qx, qy, qz);
            x = qx; y = qy; z = qz;
        }
        if (GRID) occ = occ && fc_occupied(G, x, y, z);        // the bitfield is read for the points still in question only
        const uint64_t b = __ballot(occ);
        if (lane == j) mine = b;
    }
    const int cnt = __popcll(mine);
    const int incl = wave_incl_sum_i(cnt, (int)lane);
    if (lane < chunks) { mask[c0 + lane] = mine; offsets[c0 + lane] = (uint32_t)(incl - cnt); }
    if (lane == 63) group_total[g] = (uint32_t)incl;
}

// pos_c = the point in the object's frame, xn_c = (pos + bound) / (2 bound) (fs_norm: the emit of the fixed-step cull); either may be null
template <bool PLACED, class SRC>
__global__ void __launch_bounds__(256) k_lc_emit(SRC S, FcPlace P, const uint64_t *__restrict__ mask, const uint32_t *__restrict__ offsets, uint32_t m_occ,
                                                 float bound, float *__restrict__ pos_c, float *__restrict__ xn_c) {
    const float two_b = 2 * bound;
    for (uint32_t local = blockIdx.x * 256 + threadIdx.x; local < S.count; local += gridDim.x * 256) {
        const uint32_t c = local >> 6, l = local & 63;
        const uint64_t m = mask[c];
        if (!((m >> l) & 1ull)) continue;
        const uint32_t slot = offsets[c] + (uint32_t)__popcll(m & ((1ull << l) - 1ull));
        if (slot >= m_occ) continue;
        float x, y, z;
        S.at(local, x, y, z);
        if (PLACED) {
            float qx, qy, qz;
            fc_to_object(P, x, y, z, qx, qy, qz);
            x = qx; y = qy; z = qz;
        }
        if (pos_c) {
            float *p = pos_c + (uint64_t)slot * 3;
            p[0] = x; p[1] = y; p[2] = z;
        }
        if (xn_c) {
            float *e = xn_c + (uint64_t)slot * 3;
            e[0] = fs_norm(x, bound, two_b); e[1] = fs_norm(y, bound, two_b); e[2] = fs_norm(z, bound, two_b);
        }
    }
}

// volume[i] = max(volume[i], gain * sigma_c[slot]) at the set bits; a NaN on either side stays a NaN (as torch.maximum)
__global__ void __launch_bounds__(256) k_volume_scatter_max(const float *__restrict__ sigma_c, const uint64_t *__restrict__ mask, const uint32_t *__restrict__ offsets,
                                                            float gain, float *__restrict__ volume, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t c = i >> 6, l = i & 63;
        const uint64_t m = mask[c];
        if (!((m >> l) & 1ull)) continue;
        const float v = gain * sigma_c[offsets[c] + (uint32_t)__popcll(m & ((1ull << l) - 1ull))];
        const float cur = volume[i];
        volume[i] = (v > cur || v != v) ? v : cur;
    }
}

// the scatter with a payload: at the set bits v = gain * sigma_c[slot]; v > best_sigma[i] (strict: a tie keeps what is there, a NaN v never
// wins) takes the point for `id` with its colour and normal. One thread per point, each point touched once: no atomics.
__global__ void __launch_bounds__(256) k_scene_select(const float *__restrict__ sigma_c, const float *__restrict__ rgb_c, const float *__restrict__ normal_c,
                                                      const uint64_t *__restrict__ mask, const uint32_t *__restrict__ offsets, float gain, int32_t id,
                                                      float *__restrict__ best_sigma, int32_t *__restrict__ best_id, float *__restrict__ best_rgb,
                                                      float *__restrict__ best_normal, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const uint32_t c = i >> 6, l = i & 63;
        const uint64_t m = mask[c];
        if (!((m >> l) & 1ull)) continue;
        const uint32_t slot = offsets[c] + (uint32_t)__popcll(m & ((1ull << l) - 1ull));
        const float v = gain * sigma_c[slot];
        if (!(v > best_sigma[i])) continue;
        best_sigma[i] = v;
        best_id[i] = id;
        if (best_rgb) {
            const float *s = rgb_c + (uint64_t)slot * 3;
            float *d = best_rgb + (uint64_t)i * 3;
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        }
        if (best_normal) {
            const float *s = normal_c + (uint64_t)slot * 3;
            float *d = best_normal + (uint64_t)i * 3;
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        }
    }
}

// per compacted point: the object-frame normal of grad_raw_c (unit_normal.h), its rotation into the world, and the direction the colour
// network is asked about: against the normal, or from the eye to the point; (0, 0, -1) where that direction does not exist
struct SfFrame { float R[9], eye[3]; };
template <bool EYE, bool ROT>
__global__ void __launch_bounds__(256) k_surface_frame(const float *__restrict__ grad_raw_c, const float *__restrict__ pos_c, uint32_t m, SfFrame F,
                                                       float *__restrict__ dirs_c, float *__restrict__ normal_c) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
        float n[3] = {0.0f, 0.0f, 0.0f}, v[3];
        if (grad_raw_c) {
            const float g[3] = {grad_raw_c[(uint64_t)i * 3], grad_raw_c[(uint64_t)i * 3 + 1], grad_raw_c[(uint64_t)i * 3 + 2]};
            un_unit_normal(g, n);
        }
        if (dirs_c) {
            if (EYE) {
                const float d[3] = {pos_c[(uint64_t)i * 3] - F.eye[0], pos_c[(uint64_t)i * 3 + 1] - F.eye[1], pos_c[(uint64_t)i * 3 + 2] - F.eye[2]};
                un_unit_normal(d, v);            // -(d / |d|): negated below
            } else {
                v[0] = n[0]; v[1] = n[1]; v[2] = n[2];
            }
            const bool none = v[0] == 0.0f && v[1] == 0.0f && v[2] == 0.0f;
            float *o = dirs_c + (uint64_t)i * 3;
            o[0] = none ? 0.0f : -v[0]; o[1] = none ? 0.0f : -v[1]; o[2] = none ? -1.0f : -v[2];
        }
        if (normal_c) {
            if (ROT) un_rotate(F.R, n);
            float *o = normal_c + (uint64_t)i * 3;
            o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
        }
    }
}

// ---------------------------------------------------------------- host side
static bool mc_dims_ok(const char *who, uint32_t nx, uint32_t ny, uint32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2) { foc_set_error("%s: every dimension must be >= 2 (got %u x %u x %u)", who, nx, ny, nz); return false; }
    if ((uint64_t)nx * ny > MC_MAX_POINTS || (uint64_t)nx * ny * nz > MC_MAX_POINTS) {
        foc_set_error("%s: nx * ny * nz must not exceed 2^29 points (got %u x %u x %u)", who, nx, ny, nz);
        return false;
    }
    return true;
}
static McWs mc_ws(void *workspace, uint32_t W, uint32_t G) {
    McWs ws;
    uint8_t *p = reinterpret_cast<uint8_t *>(workspace);
    ws.totals = reinterpret_cast<uint32_t *>(p); p += 16;
    ws.mx = reinterpret_cast<uint64_t *>(p); p += (uint64_t)W * 8;
    ws.my = reinterpret_cast<uint64_t *>(p); p += (uint64_t)W * 8;
    ws.mz = reinterpret_cast<uint64_t *>(p); p += (uint64_t)W * 8;
    ws.mt = reinterpret_cast<uint64_t *>(p); p += (uint64_t)W * 8;
    ws.voff = reinterpret_cast<uint32_t *>(p); p += (uint64_t)W * 4;
    ws.toff = reinterpret_cast<uint32_t *>(p); p += (uint64_t)W * 4;
    ws.gv = reinterpret_cast<uint32_t *>(p); p += (uint64_t)G * 4;
    ws.gt = reinterpret_cast<uint32_t *>(p); p += (uint64_t)G * 4;
    ws.gb = reinterpret_cast<uint32_t *>(p);
    return ws;
}
static inline McDim mc_dim(uint32_t nx, uint32_t ny, uint32_t nz) { return McDim{nx, ny, nz, ny * nz, nx * ny * nz}; }

// the refusals of foc_lattice_cull and foc_lattice_cull_emit that concern the lattice and the slab
static bool lc_slab_ok(const char *who, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t first, uint32_t count) {
    if (rx < 1 || ry < 1 || rz < 1 || (uint64_t)rx * ry > MC_MAX_POINTS || (uint64_t)rx * ry * rz > MC_MAX_POINTS) {
        foc_set_error("%s: a lattice of 1 .. 2^29 points expected (got %u x %u x %u)", who, rx, ry, rz);
        return false;
    }
    if ((uint64_t)first + count > (uint64_t)rx * ry * rz) {
        foc_set_error("%s: the slab [%u, %u + %u) leaves the lattice of %llu points", who, first, first, count, (unsigned long long)rx * ry * rz);
        return false;
    }
    return true;
}

// foc_lattice_cull / foc_points_cull behind the refusals that concern where the points come from: the placement, the grid, the scratch, then
// the mask, scan and finish launches
template <class SRC>
static int lc_cull(const char *who, const SRC &S, const float *world_to_object, const float *obj_aabb, float bound, const uint8_t *bitfield, uint32_t cascade,
                   uint32_t grid_size, uint64_t *mask, uint32_t *offsets, uint32_t *count_out, void *scratch, uint64_t scratch_bytes, void *stream) {
    FOC_REQUIRE((world_to_object == nullptr) == (obj_aabb == nullptr), FOC_E_INVALID, "%s: world_to_object and obj_aabb (host arrays of 12 and 6 floats) come together", who);
    FOC_REQUIRE(!world_to_object || (fc_all_finite(world_to_object, 12) && fc_all_finite(obj_aabb, 6)), FOC_E_INVALID, "%s: non-finite world_to_object / obj_aabb", who);
    FcGrid G{};
    if (bitfield) {
        FOC_REQUIRE(cascade >= 1 && cascade <= 16, FOC_E_INVALID, "%s: cascade must be 1..16 (got %u)", who, cascade);
        FOC_REQUIRE(grid_size >= 2 && grid_size <= 1024 && (grid_size & (grid_size - 1)) == 0, FOC_E_INVALID,
                    "%s: grid_size must be a power of two in 2..1024 (got %u)", who, grid_size);
        const uint64_t cells = (uint64_t)cascade * grid_size * grid_size * grid_size;
        FOC_REQUIRE(cells < (1ull << 32), FOC_E_INVALID, "%s: cascade * grid_size^3 must fit 32 bits", who);
        FOC_REQUIRE(std::isfinite(bound) && bound > 0, FOC_E_INVALID, "%s: bound must be finite and > 0", who);
        G.bits = bitfield; G.bound = bound; G.Cf = (float)cascade; G.Hm1 = (float)(grid_size - 1);
        G.H3 = (float)((uint64_t)grid_size * grid_size * grid_size); G.H = grid_size; G.n_cells = (uint32_t)cells;
    }
    const uint32_t count = S.count;
    FOC_REQUIRE(scratch_bytes >= foc_lattice_cull_scratch_bytes(count), FOC_E_INVALID, "%s: scratch of %llu bytes, foc_lattice_cull_scratch_bytes(%u) asks for %llu", who,
                (unsigned long long)scratch_bytes, count, (unsigned long long)foc_lattice_cull_scratch_bytes(count));
    FOC_REQUIRE((((uintptr_t)mask) & 7) == 0, FOC_E_INVALID, "%s: mask must be 8-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    const uint32_t W = ms_chunks(count), NG = ms_groups(W);
    const FcPlace P = world_to_object ? fc_place(world_to_object, obj_aabb, 1.0f) : FcPlace{};
    uint32_t *group_total = reinterpret_cast<uint32_t *>(scratch);
    const dim3 grid(foc_div_up(NG, 4)), block(256);
    if (world_to_object && bitfield) hipLaunchKernelGGL((k_lc_mask<true, true, SRC>), grid, block, 0, st, S, G, P, W, NG, mask, offsets, group_total);
    else if (world_to_object) hipLaunchKernelGGL((k_lc_mask<true, false, SRC>), grid, block, 0, st, S, G, P, W, NG, mask, offsets, group_total);
    else if (bitfield) hipLaunchKernelGGL((k_lc_mask<false, true, SRC>), grid, block, 0, st, S, G, P, W, NG, mask, offsets, group_total);
    else hipLaunchKernelGGL((k_lc_mask<false, false, SRC>), grid, block, 0, st, S, G, P, W, NG, mask, offsets, group_total);
    FOC_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_ms_scan, dim3(1), dim3(1024), 0, st, group_total, (uint32_t *)nullptr, (const uint32_t *)nullptr, NG, offsets + W, count_out, 1u);
    FOC_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(k_ms_finish, dim3(foc_grid_1d(W, 256)), dim3(256), 0, st, group_total, offsets, (const uint32_t *)nullptr, (uint32_t *)nullptr, W);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

template <class SRC>
static int lc_emit(const char *who, const SRC &S, const float *world_to_object, float bound, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ,
                   float *pos_c, float *xn_c, void *stream) {
    FOC_REQUIRE(!world_to_object || fc_all_finite(world_to_object, 12), FOC_E_INVALID, "%s: non-finite world_to_object", who);
    const float no_box[6] = {0, 0, 0, 0, 0, 0};                // the emit pass reads the mask: the box is not consulted again
    const dim3 grid(foc_grid_1d(S.count, 256)), block(256);
    if (world_to_object) hipLaunchKernelGGL((k_lc_emit<true, SRC>), grid, block, 0, (hipStream_t)stream, S, fc_place(world_to_object, no_box, 1.0f), mask, offsets, m_occ, bound, pos_c, xn_c);
    else hipLaunchKernelGGL((k_lc_emit<false, SRC>), grid, block, 0, (hipStream_t)stream, S, FcPlace{}, mask, offsets, m_occ, bound, pos_c, xn_c);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

extern "C" {

uint64_t foc_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz) {
    if (!mc_dims_ok("mc_workspace_bytes", nx, ny, nz)) return 0;
    const uint32_t W = ms_chunks((uint64_t)nx * ny * nz), G = ms_groups(W);
    return 16 + (uint64_t)W * (4 * 8 + 2 * 4) + (uint64_t)G * 3 * 4;
}

int foc_mc_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float thr, void *workspace, uint32_t *counts3, void *stream) {
    FocDeviceGuard foc_guard_(stream, volume);
    FOC_REQUIRE(volume && workspace && counts3, FOC_E_INVALID, "mc_count: null pointer");
    if (!mc_dims_ok("mc_count", nx, ny, nz)) return FOC_E_INVALID;
    FOC_REQUIRE(std::isfinite(thr), FOC_E_INVALID, "mc_count: the threshold must be finite");
    FOC_REQUIRE((((uintptr_t)workspace) & 7) == 0, FOC_E_INVALID, "mc_count: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const McDim D = mc_dim(nx, ny, nz);
    const uint32_t W = ms_chunks(D.n), G = ms_groups(W);
    const McWs ws = mc_ws(workspace, W, G);
    hipLaunchKernelGGL(k_mc_count, dim3(foc_div_up(G, 4)), dim3(256), 0, st, volume, D, thr, W, G, ws);
    FOC_CHECK_LAUNCH("mc_count");
    hipLaunchKernelGGL(k_ms_scan, dim3(1), dim3(1024), 0, st, ws.gv, ws.gt, ws.gb, G, ws.totals, counts3, 3u);
    FOC_CHECK_LAUNCH("mc_count");
    hipLaunchKernelGGL(k_ms_finish, dim3(foc_grid_1d(W, 256)), dim3(256), 0, st, ws.gv, ws.voff, ws.gt, ws.toff, W);
    FOC_CHECK_LAUNCH("mc_count");
    return FOC_OK;
}

int foc_mc_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float thr, const void *workspace, const float *origin3, const float *spacing3,
                float *vertices, float *normals, int32_t *triangles, void *stream) {
    FocDeviceGuard foc_guard_(stream, volume);
    FOC_REQUIRE(volume && workspace && vertices && triangles, FOC_E_INVALID, "mc_emit: null pointer");
    if (!mc_dims_ok("mc_emit", nx, ny, nz)) return FOC_E_INVALID;
    FOC_REQUIRE(std::isfinite(thr), FOC_E_INVALID, "mc_emit: the threshold must be finite");
    FOC_REQUIRE((((uintptr_t)workspace) & 7) == 0, FOC_E_INVALID, "mc_emit: workspace must be 8-byte aligned");
    McMap M{0, 0, 0, 1, 1, 1};
    if (origin3) { FOC_REQUIRE(fc_all_finite(origin3, 3), FOC_E_INVALID, "mc_emit: non-finite origin"); M.ox = origin3[0]; M.oy = origin3[1]; M.oz = origin3[2]; }
    if (spacing3) {
        FOC_REQUIRE(fc_all_finite(spacing3, 3) && spacing3[0] != 0 && spacing3[1] != 0 && spacing3[2] != 0, FOC_E_INVALID, "mc_emit: spacing must be finite and non-zero");
        M.sx = spacing3[0]; M.sy = spacing3[1]; M.sz = spacing3[2];
    }
    const McDim D = mc_dim(nx, ny, nz);
    const uint32_t W = ms_chunks(D.n), G = ms_groups(W);
    const McWs ws = mc_ws(const_cast<void *>(workspace), W, G);
    if (normals) hipLaunchKernelGGL(k_mc_emit<true>, dim3(foc_div_up(G, 4)), dim3(256), 0, (hipStream_t)stream, volume, D, thr, W, G, ws, M, vertices, normals, triangles);
    else hipLaunchKernelGGL(k_mc_emit<false>, dim3(foc_div_up(G, 4)), dim3(256), 0, (hipStream_t)stream, volume, D, thr, W, G, ws, M, vertices, normals, triangles);
    FOC_CHECK_LAUNCH("mc_emit");
    return FOC_OK;
}

uint64_t foc_lattice_cull_scratch_bytes(uint32_t count) {
    return (uint64_t)ms_groups(ms_chunks(count)) * sizeof(uint32_t);
}

int foc_lattice_cull(const float *xs, const float *ys, const float *zs, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t first, uint32_t count,
                     const float *world_to_object, const float *obj_aabb, float bound, const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size,
                     uint64_t *mask, uint32_t *offsets, uint32_t *count_out, void *scratch, uint64_t scratch_bytes, void *stream) {
    FocDeviceGuard foc_guard_(stream, xs);
    FOC_REQUIRE(xs && ys && zs && mask && offsets && count_out && scratch, FOC_E_INVALID, "lattice_cull: null pointer");
    if (!lc_slab_ok("lattice_cull", rx, ry, rz, first, count)) return FOC_E_INVALID;
    FOC_REQUIRE(count >= 1, FOC_E_INVALID, "lattice_cull: an empty slab");
    return lc_cull("lattice_cull", LcLattice{xs, ys, zs, ry, rz, first, count}, world_to_object, obj_aabb, bound, bitfield, cascade, grid_size, mask, offsets,
                   count_out, scratch, scratch_bytes, stream);
}

int foc_lattice_cull_emit(const float *xs, const float *ys, const float *zs, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t first, uint32_t count,
                          const float *world_to_object, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ, float *pos_c, void *stream) {
    FocDeviceGuard foc_guard_(stream, xs);
    if (m_occ == 0) return FOC_OK;
    FOC_REQUIRE(xs && ys && zs && mask && offsets && pos_c, FOC_E_INVALID, "lattice_cull_emit: null pointer");
    if (!lc_slab_ok("lattice_cull_emit", rx, ry, rz, first, count)) return FOC_E_INVALID;
    FOC_REQUIRE(count >= 1, FOC_E_INVALID, "lattice_cull_emit: an empty slab");
    return lc_emit("lattice_cull_emit", LcLattice{xs, ys, zs, ry, rz, first, count}, world_to_object, 1.0f, mask, offsets, m_occ, pos_c, nullptr, stream);
}

int foc_points_cull(const float *points, uint32_t M, const float *world_to_object, const float *obj_aabb, float bound, const uint8_t *bitfield, uint32_t cascade,
                    uint32_t grid_size, uint64_t *mask, uint32_t *offsets, uint32_t *count_out, void *scratch, uint64_t scratch_bytes, void *stream) {
    FocDeviceGuard foc_guard_(stream, points);
    if (M == 0) return FOC_OK;
    FOC_REQUIRE(points && mask && offsets && count_out && scratch, FOC_E_INVALID, "points_cull: null pointer");
    FOC_REQUIRE(M <= MC_MAX_POINTS, FOC_E_INVALID, "points_cull: M must not exceed 2^29 points (got %u)", M);
    return lc_cull("points_cull", LcList{points, M}, world_to_object, obj_aabb, bound, bitfield, cascade, grid_size, mask, offsets, count_out, scratch,
                   scratch_bytes, stream);
}

int foc_points_cull_emit(const float *points, uint32_t M, const float *world_to_object, float bound, const uint64_t *mask, const uint32_t *offsets,
                         uint32_t m_occ, float *pos_c, float *xn_c, void *stream) {
    FocDeviceGuard foc_guard_(stream, points);
    if (M == 0 || m_occ == 0 || !(pos_c || xn_c)) return FOC_OK;
    FOC_REQUIRE(points && mask && offsets, FOC_E_INVALID, "points_cull_emit: null pointer");
    FOC_REQUIRE(M <= MC_MAX_POINTS && m_occ <= M, FOC_E_INVALID, "points_cull_emit: M must not exceed 2^29 points and m_occ not M (got %u, %u)", M, m_occ);
    FOC_REQUIRE(!xn_c || (std::isfinite(bound) && bound > 0), FOC_E_INVALID, "points_cull_emit: bound must be finite and > 0 for xn_c");
    return lc_emit("points_cull_emit", LcList{points, M}, world_to_object, xn_c ? bound : 1.0f, mask, offsets, m_occ, pos_c, xn_c, stream);
}

int foc_surface_frame(const float *grad_raw_c, const float *pos_c, uint32_t m, const float *rot9, int mode, const float *eye_obj, float *dirs_c,
                      float *normal_c, void *stream) {
    FocDeviceGuard foc_guard_(stream, grad_raw_c ? grad_raw_c : pos_c);
    FOC_REQUIRE(mode == 0 || mode == 1, FOC_E_INVALID, "surface_frame: mode must be 0 (normal) or 1 (eye), got %d", mode);
    if (m == 0 || !(dirs_c || normal_c)) return FOC_OK;
    FOC_REQUIRE(m <= MC_MAX_POINTS, FOC_E_INVALID, "surface_frame: m must not exceed 2^29 points (got %u)", m);
    const bool eye = mode == 1 && dirs_c;
    FOC_REQUIRE(grad_raw_c || !(normal_c || (dirs_c && !eye)), FOC_E_INVALID, "surface_frame: null pointer (grad_raw_c: the normal and the mode-0 direction come from it)");
    FOC_REQUIRE(!eye || (pos_c && eye_obj), FOC_E_INVALID, "surface_frame: null pointer (mode 1 takes pos_c and eye_obj, 3 floats in host memory)");
    FOC_REQUIRE(!eye || fc_all_finite(eye_obj, 3), FOC_E_INVALID, "surface_frame: non-finite eye_obj");
    FOC_REQUIRE(!rot9 || fc_all_finite(rot9, 9), FOC_E_INVALID, "surface_frame: non-finite rot9");
    SfFrame F{};
    if (rot9) for (int k = 0; k < 9; k++) F.R[k] = rot9[k];
    if (eye) for (int k = 0; k < 3; k++) F.eye[k] = eye_obj[k];
    const dim3 grid(foc_grid_1d(m, 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const bool rot = rot9 && normal_c;
    if (eye && rot) hipLaunchKernelGGL((k_surface_frame<true, true>), grid, block, 0, st, grad_raw_c, pos_c, m, F, dirs_c, normal_c);
    else if (eye) hipLaunchKernelGGL((k_surface_frame<true, false>), grid, block, 0, st, grad_raw_c, pos_c, m, F, dirs_c, normal_c);
    else if (rot) hipLaunchKernelGGL((k_surface_frame<false, true>), grid, block, 0, st, grad_raw_c, pos_c, m, F, dirs_c, normal_c);
    else hipLaunchKernelGGL((k_surface_frame<false, false>), grid, block, 0, st, grad_raw_c, pos_c, m, F, dirs_c, normal_c);
    FOC_CHECK_LAUNCH("surface_frame");
    return FOC_OK;
}

int foc_scene_select(const float *sigma_c, const float *rgb_c, const float *normal_c, const uint64_t *mask, const uint32_t *offsets, float gain,
                     int32_t object_index, float *best_sigma, int32_t *best_id, float *best_rgb, float *best_normal, uint32_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, best_sigma);
    if (n == 0) return FOC_OK;
    FOC_REQUIRE(sigma_c && mask && offsets && best_sigma && best_id, FOC_E_INVALID, "scene_select: null pointer");
    FOC_REQUIRE((rgb_c == nullptr) == (best_rgb == nullptr) && (normal_c == nullptr) == (best_normal == nullptr), FOC_E_INVALID,
                "scene_select: rgb_c / best_rgb and normal_c / best_normal come in pairs");
    FOC_REQUIRE(n <= MC_MAX_POINTS, FOC_E_INVALID, "scene_select: n must not exceed 2^29 points (got %u)", n);
    FOC_REQUIRE(std::isfinite(gain) && gain > 0, FOC_E_INVALID, "scene_select: gain must be finite and > 0 (got %g)", (double)gain);
    hipLaunchKernelGGL(k_scene_select, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, sigma_c, rgb_c, normal_c, mask, offsets, gain, object_index,
                       best_sigma, best_id, best_rgb, best_normal, n);
    FOC_CHECK_LAUNCH("scene_select");
    return FOC_OK;
}

int foc_volume_scatter_max(const float *sigma_c, const uint64_t *mask, const uint32_t *offsets, float gain, float *volume, uint32_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, volume);
    if (n == 0) return FOC_OK;
    FOC_REQUIRE(sigma_c && mask && offsets && volume, FOC_E_INVALID, "volume_scatter_max: null pointer");
    FOC_REQUIRE(n <= MC_MAX_POINTS, FOC_E_INVALID, "volume_scatter_max: n must not exceed 2^29 points (got %u)", n);
    FOC_REQUIRE(std::isfinite(gain) && gain > 0, FOC_E_INVALID, "volume_scatter_max: gain must be finite and > 0 (got %g)", (double)gain);
    hipLaunchKernelGGL(k_volume_scatter_max, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, sigma_c, mask, offsets, gain, volume, n);
    FOC_CHECK_LAUNCH("volume_scatter_max");
    return FOC_OK;
}

} // extern "C"
