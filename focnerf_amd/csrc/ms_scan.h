// ms_scan.h — the compaction scaffold mesh.hip and simplify.hip share: ballot words, popcounts, one scan, one finish pass.
// A CHUNK is 64 consecutive elements (one ballot word), one wave owns a GROUP of up to MS_GROUP consecutive chunks and leaves per-chunk
// exclusive offsets inside the group plus the group's total; k_ms_scan (one workgroup) turns the group totals into exclusive prefix sums
// and writes the grand totals, k_ms_finish adds each group's base to its chunks' offsets. Kernels are `static`: one copy per translation
// unit, as k_foc_zero.
#pragma once
#include "common.h"

#define MS_GROUP 64u                       // chunks per wave

__device__ __forceinline__ uint64_t ms_shfl64(uint64_t v, uint32_t j) {
    return ((uint64_t)(uint32_t)__shfl((int)(v >> 32), (int)j, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)v, (int)j, 64);
}

// ---------------------------------------------------------------- pass 2: one workgroup scans the group totals
// a and b (b may be null) become exclusive prefix sums in place, c (may be null) is only summed; the first n_out of the three totals go to
// out_a and out_b (either may be null)
__global__ static void __launch_bounds__(1024) k_ms_scan(uint32_t *__restrict__ a, uint32_t *__restrict__ b, const uint32_t *__restrict__ c, uint32_t n_groups,
                                                  uint32_t *__restrict__ out_a, uint32_t *__restrict__ out_b, uint32_t n_out) {
    __shared__ int wave_tot[3][16];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t carry[3] = {0, 0, 0};
    for (uint32_t base = 0; base < n_groups; base += 1024) {
        const uint32_t k = base + threadIdx.x;
        int v[3], incl[3];
        v[0] = k < n_groups ? (int)a[k] : 0;
        v[1] = (b && k < n_groups) ? (int)b[k] : 0;
        v[2] = (c && k < n_groups) ? (int)c[k] : 0;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            incl[q] = wave_incl_sum_i(v[q], (int)lane);
            if (lane == 63) wave_tot[q][wv] = incl[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; q++) {
            int before = 0, all = 0;
#pragma unroll
            for (int u = 0; u < 16; u++) { const int t = wave_tot[q][u]; all += t; if (u < (int)wv) before += t; }
            if (k < n_groups) {
                if (q == 0) a[k] = carry[0] + (uint32_t)(before + incl[0] - v[0]);
                if (q == 1 && b) b[k] = carry[1] + (uint32_t)(before + incl[1] - v[1]);
            }
            carry[q] += (uint32_t)all;
        }
        __syncthreads();
    }
    if (threadIdx.x < n_out) {
        const uint32_t t = threadIdx.x == 0 ? carry[0] : threadIdx.x == 1 ? carry[1] : carry[2];
        if (out_a) out_a[threadIdx.x] = t;
        if (out_b) out_b[threadIdx.x] = t;
    }
}

// ---------------------------------------------------------------- pass 3: offsets[chunk] += base of the chunk's group
__global__ static void __launch_bounds__(256) k_ms_finish(const uint32_t *__restrict__ base_a, uint32_t *__restrict__ off_a, const uint32_t *__restrict__ base_b,
                                                   uint32_t *__restrict__ off_b, uint32_t W) {
    for (uint32_t c = blockIdx.x * 256 + threadIdx.x; c < W; c += gridDim.x * 256) {
        off_a[c] += base_a[c / MS_GROUP];
        if (off_b) off_b[c] += base_b[c / MS_GROUP];
    }
}

static inline uint32_t ms_chunks(uint64_t n) { return foc_div_up(n, 64); }
static inline uint32_t ms_groups(uint32_t W) { return foc_div_up(W, MS_GROUP); }
