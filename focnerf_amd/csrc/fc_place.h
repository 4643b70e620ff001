// fc_place.h — the occupancy bit of a position and an object's placement, as the cull kernels see them: shared by the fixed-step cull
// (fixedcull.hip) and the lattice cull of the mesh extraction (mesh.hip), so that both test the same cell with the same arithmetic.
#pragma once
#include <cmath>
#include "common.h"
#include "occ_cell.h"

struct FcGrid { const uint8_t *bits; float bound, Cf, Hm1, H3; uint32_t H, n_cells; };

// the occupancy bit of a clipped position: rm_cell without the dt term (a fixed-step sample has no marching step)
__device__ __forceinline__ bool fc_occupied(const FcGrid &G, float x, float y, float z) {
    const int level = rm_mip_from_pos(x, y, z, G.Cf);
    float mip_bound;
    int nx, ny, nz;
    uint32_t index = rm_cell_index(x, y, z, level, G.bound, G.H, G.Hm1, G.H3, mip_bound, nx, ny, nz);
    index = min(index, G.n_cells - 1u);          // the float index is exact for every grid the library builds (C * H^3 <= 2^24); never read past the bitfield
    return rm_cell_bit(G.bits, index);
}

// An object's placement as the kernels see it (include/focnerf.h foc_fixed_cull_placed): world -> object q = A x + b, the object's own box
// and the factor of the emitted direction. Wave-uniform and passed by value: it sits in scalar registers. The unplaced instantiations
// take an all-zero one and never read it.
struct FcPlace { float a00, a01, a02, a10, a11, a12, a20, a21, a22, b0, b1, b2, lo0, lo1, lo2, hi0, hi1, hi2, dir_scale; };
// per axis ((A_k0 x + A_k1 y) + A_k2 z) + b_k, in this order, unfused (-ffp-contract=off); q is not clamped
__device__ __forceinline__ void fc_to_object(const FcPlace &P, float x, float y, float z, float &qx, float &qy, float &qz) {
    qx = ((P.a00 * x + P.a01 * y) + P.a02 * z) + P.b0;
    qy = ((P.a10 * x + P.a11 * y) + P.a12 * z) + P.b1;
    qz = ((P.a20 * x + P.a21 * y) + P.a22 * z) + P.b2;
}
// false for a NaN coordinate: such a sample is never looked up
__device__ __forceinline__ bool fc_inside(const FcPlace &P, float qx, float qy, float qz) {
    return qx >= P.lo0 && qx <= P.hi0 && qy >= P.lo1 && qy <= P.hi1 && qz >= P.lo2 && qz <= P.hi2;
}

// the placement of a *_placed call from its host arrays: world_to_object [12] = A row-major then b, obj_aabb [6] = lo then hi
static inline FcPlace fc_place(const float *w2o, const float *obj_aabb, float dir_scale) {
    return FcPlace{w2o[0], w2o[1], w2o[2], w2o[3], w2o[4], w2o[5], w2o[6], w2o[7], w2o[8], w2o[9], w2o[10], w2o[11],
                   obj_aabb[0], obj_aabb[1], obj_aabb[2], obj_aabb[3], obj_aabb[4], obj_aabb[5], dir_scale};
}
static inline bool fc_all_finite(const float *v, int n) {
    for (int k = 0; k < n; k++) if (!std::isfinite(v[k])) return false;
    return true;
}
