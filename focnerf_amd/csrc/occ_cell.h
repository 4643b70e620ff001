// occ_cell.h — the occupancy-grid cell of a position (raymarching.cu:42-54, :361-379), shared by the marching kernels
// (raymarching.hip rm_cell) and the fixed-step cull (fixedcull.hip): cascade level, cell coordinates, Morton index. The Morton expand / compact pair
// is defined here once (densitygrid.hip enumerates and draws cells with it).
#pragma once
#include "common.h"

__device__ __forceinline__ float rm_clamp(float x, float lo, float hi) { return fminf(hi, fmaxf(lo, x)); }

__device__ __forceinline__ uint32_t rm_expand_bits(uint32_t v) {
    v = (v * 0x00010001u) & 0xFF0000FFu;
    v = (v * 0x00000101u) & 0x0F00F00Fu;
    v = (v * 0x00000011u) & 0xC30C30C3u;
    v = (v * 0x00000005u) & 0x49249249u;
    return v;
}
__device__ __forceinline__ uint32_t rm_morton3D(uint32_t x, uint32_t y, uint32_t z) {
    return rm_expand_bits(x) | (rm_expand_bits(y) << 1) | (rm_expand_bits(z) << 2);
}

__device__ __forceinline__ uint32_t rm_morton3D_invert(uint32_t x) {
    x = x & 0x49249249u;
    x = (x | (x >> 2)) & 0xc30c30c3u;
    x = (x | (x >> 4)) & 0x0f00f00fu;
    x = (x | (x >> 8)) & 0xff0000ffu;
    x = (x | (x >> 16)) & 0x0000ffffu;
    return x;
}

// frexpf exponent of a non-negative finite float without the libcall: for x = 0 frexpf
// returns exponent 0; subnormals never reach a positive exponent, and only max(0, e) is used.
__device__ __forceinline__ int rm_frexp_exp(float x) {
    int e;
    (void)frexpf(x, &e);
    return e;
}

// mip_from_pos (:42-47): float min/max, then truncation. Cf = (float)cascade.
__device__ __forceinline__ int rm_mip_from_pos(float x, float y, float z, float Cf) {
    const float mx = fmaxf(fabsf(x), fmaxf(fabsf(y), fabsf(z)));
    return (int)fminf(Cf - 1, fmaxf(0.0f, (float)rm_frexp_exp(mx)));
}

// Cell of (x, y, z) at cascade `level`: mip_bound = min(2^level, bound); per axis 0.5 * (x * mip_rbound + 1) * H in double, narrowed to
// float by clamp()'s parameter (:374-376); index = level * H3 + morton in float (:339, :378). Hm1 = (float)(H - 1), H3 = (float)H^3.
__device__ __forceinline__ uint32_t rm_cell_index(float x, float y, float z, int level, float bound, uint32_t H, float Hm1, float H3,
                                                  float &mip_bound, int &nx, int &ny, int &nz) {
    mip_bound = fminf(scalbnf(1.0f, level), bound);
    const float mip_rbound = 1 / mip_bound;
    nx = (int)rm_clamp((float)(0.5 * (double)fmaf(x, mip_rbound, 1.0f) * (double)H), 0.0f, Hm1);
    ny = (int)rm_clamp((float)(0.5 * (double)fmaf(y, mip_rbound, 1.0f) * (double)H), 0.0f, Hm1);
    nz = (int)rm_clamp((float)(0.5 * (double)fmaf(z, mip_rbound, 1.0f) * (double)H), 0.0f, Hm1);
    return (uint32_t)fmaf((float)level, H3, (float)rm_morton3D((uint32_t)nx, (uint32_t)ny, (uint32_t)nz));
}
__device__ __forceinline__ bool rm_cell_bit(const uint8_t *__restrict__ grid, uint32_t index) { return (grid[index >> 3] & (1u << (index & 7u))) != 0; }
