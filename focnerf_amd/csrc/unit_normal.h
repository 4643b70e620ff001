// unit_normal.h — the normalise and rotate rules of a surface normal, stated once: the normals kernel (normals.hip, k_field_normals) and the
// point pipeline's frame kernel (mesh.hip, k_surface_frame) both end in them, so a normal has the same bits whichever of the two made it.
#pragma once
#include "common.h"

// n = -g / |g| scaled by the largest component first (no overflow, no underflow): m = max |g_d|; m zero or a component not finite -> n = 0;
// else u = g / m, n = -u / sqrt(u . u), the squares summed by fmaf from u0 u0. All fp32.
__device__ __forceinline__ void un_unit_normal(const float (&g)[3], float (&n)[3]) {
    const float m = fmaxf(fmaxf(fabsf(g[0]), fabsf(g[1])), fabsf(g[2]));
    n[0] = 0.0f; n[1] = 0.0f; n[2] = 0.0f;
    if (m > 0.0f && isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2])) {
        const float u0 = g[0] / m, u1 = g[1] / m, u2 = g[2] / m;
        const float len = sqrtf(fmaf(u2, u2, fmaf(u1, u1, u0 * u0)));
        n[0] = -u0 / len; n[1] = -u1 / len; n[2] = -u2 / len;
    }
}

// n <- R n for a row-major 3 x 3 R: per row fmaf from the product of column 0
__device__ __forceinline__ void un_rotate(const float (&R)[9], float (&n)[3]) {
    const float r0 = fmaf(R[2], n[2], fmaf(R[1], n[1], R[0] * n[0])), r1 = fmaf(R[5], n[2], fmaf(R[4], n[1], R[3] * n[0])),
                r2 = fmaf(R[8], n[2], fmaf(R[7], n[1], R[6] * n[0]));
    n[0] = r0; n[1] = r1; n[2] = r2;
}
