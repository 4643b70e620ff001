// background.hip — the background model of torch-ngp's default network as one kernel per direction (legacy/nerf/network.py:145-160,
// called per ray at legacy/nerf/renderer.py:232-234 and 271-274):
//
//     bg = sigmoid(W1 . relu(W0 . [SH16(d) | grid8((sph_from_ray(o, d, R) + 1) / 2)]))
//
// grid8: a 4-level hash grid over D = 2 with C = 2 (encoder_bg: levels 0-2 dense, level 3 hashed); W0 [64,24], W1 [3,64], no biases.
// The op path is a dozen launches each way (sph_from_ray, grid_encode, SH, cat, two GEMMs, ReLU, sigmoid and their backwards); here one
// thread carries one ray through all of it. The arithmetic of every stage is the op path's under fp16 autocast:
//   * the sphere coordinates: k_sph_from_ray (raymarching.hip), then (x + 1) / 2 as GridEncoder.forward takes it;
//   * the grid: gridencoder.hip's D = 2 forward (same index math, corner order and fmaf chain); the fp32 table is rounded to fp16 on
//     load, which gives the values of the op path's `.half()` copy, and each level's pair is rounded to fp16;
//   * SH: sample_math.h foc_sh16 (k_sh_encode's row) in fp32, rounded to fp16 (autocast casts the promoted cat to fp16 for nn.Linear);
//   * the MLP: fp32 sums of fp16 products, rounded to fp16 per layer, ReLU on the rounded value, sigmoid in fp32 rounded to fp16.
// The MLP sums run in another order than the GEMMs of the op path: rgb agrees within a few fp16 ulps (tests/test_gpu_network_linear.py).
//
// Weights: the FFMLP blob of bg_net (ffmlp.PackedMLP): W0 padded to [64,32] (columns 24..31 zero), W1 padded to [16,64] (rows 3..15 zero).
// The MLP runs on the VALU from weights staged in LDS (1728 fp32): 64 x 24 + 3 x 64 products per ray.
//
// Backward (rays carry no gradient, so there is no input gradient): the forward is recomputed per ray, then
//   * the table gradient: per ray 4 levels x 4 corners x 2 channels, w * g added with fp32 atomics into the fp32 gradient — each table
//     row's sum depends on the order in which rays arrive (rows shared by several rays: every row of the dense levels 0-2, hash
//     collisions on level 3); nothing else does. FOC_DETERMINISTIC: the addends go, as 2^-40-scaled 64-bit integers, into a hash table
//     keyed by table row that lives in the workspace (BgDetEntry; integer atomics: which entry a row claims depends on arrival, its
//     sums do not), and k_bg_det_finish adds each row's total to the gradient once;
//   * dW0 (64 x 24 used entries) and dW1 (3 x 64): each workgroup (one wave) stages 64 rays' inputs, activations and output gradients
//     in LDS and sums every weight's products over its rays in ray order, chunk after chunk; k_bg_dw_reduce adds the workgroups'
//     partials in workgroup order. The assignment of rays to workgroups depends only on N: the same bits on every run.
#include "common.h"
#include "sample_math.h"
#include <math.h>

#define BG_LEVELS 4
#define BG_HIDDEN 64
#define BG_IN 24                       // SH 16 + grid 4 x 2
#define BG_OUT 3
#define BG_W0_LD 32                    // blob row width of W0
#define BG_BLOB (BG_HIDDEN * BG_W0_LD + 16 * BG_HIDDEN)
#define BG_DW (BG_HIDDEN * BG_IN + BG_OUT * BG_HIDDEN)     // 1728 used weight entries = 27 per lane of a wave
#define BG_RAYS 64                     // rays per chunk of the backward (one wave, one ray per lane)
#define BG_LDS_LD 66                   // row stride (halfs) of the backward's [feature][ray] arrays: consecutive features in other banks
#define BG_MAX_WG 2048                 // workgroups of the backward (its partials: BG_MAX_WG x 1728 fp32 at most)
#define RM_RPI_BG 0.3183098861837907f  // 1 / pi, as raymarching.hip's RM_RPI

static_assert(BG_RAYS == BG_HIDDEN && BG_DW == BG_RAYS * (BG_IN + BG_OUT), "lane m of the backward owns row m of dW0 and column m of dW1");

struct BgLevels {
    float scale[BG_LEVELS];
    uint32_t resolution[BG_LEVELS];
};

__device__ __forceinline__ float bg_h(float v) { return (float)foc_f2h(v); }

// gridencoder.hip ge_index<2> (gridencoder.cu:50-84) for align_corners = false, gridtype hash
__device__ __forceinline__ uint32_t bg_index(uint32_t hashmap_size, uint32_t resolution, uint32_t px, uint32_t py) {
    uint32_t stride = 1, index = 0;
    if (stride <= hashmap_size) { index += px * stride; stride *= resolution + 1; }
    if (stride <= hashmap_size) { index += py * stride; stride *= resolution + 1; }
    if (stride > hashmap_size) index = px ^ (py * 2654435761u);
    if (index >= hashmap_size) index = ((hashmap_size & (hashmap_size - 1u)) == 0u) ? (index & (hashmap_size - 1u)) : (index % hashmap_size);
    return index;
}

// One ray's MLP input x[24] (fp16 values held in fp32) and, for the backward, its grid corners: rows (absolute table rows) and weights.
// false: the point lies outside [0,1]^2 (the grid part is 0 and takes no gradient, gridencoder.cu:119-135, 276-281).
template <bool CORNERS>
__device__ __forceinline__ bool bg_input(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ coords,
                                         float radius, uint32_t n, const float *__restrict__ emb, const int32_t *__restrict__ offsets,
                                         const BgLevels &lv, float (&x)[BG_IN], uint32_t (&rows)[BG_LEVELS][4], float (&wts)[BG_LEVELS][4]) {
    const float dx = rays_d[(uint64_t)n * 3], dy = rays_d[(uint64_t)n * 3 + 1], dz = rays_d[(uint64_t)n * 3 + 2];
    float sh[16];
    foc_sh16(dx, dy, dz, sh);
#pragma unroll
    for (int j = 0; j < 16; j++) x[j] = bg_h(sh[j]);
    float cx, cy;
    if (coords) {
        cx = coords[(uint64_t)n * 2]; cy = coords[(uint64_t)n * 2 + 1];
    } else {                                                     // k_sph_from_ray
        const float ox = rays_o[(uint64_t)n * 3], oy = rays_o[(uint64_t)n * 3 + 1], oz = rays_o[(uint64_t)n * 3 + 2];
        const float A = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
        const float B = fmaf(oz, dz, fmaf(oy, dy, ox * dx));
        const float C = fmaf(-radius, radius, fmaf(oz, oz, fmaf(oy, oy, ox * ox)));
        const float t = (-B + sqrtf(fmaf(B, B, -(A * C)))) / A;
        const float px = fmaf(t, dx, ox), py = fmaf(t, dy, oy), pz = fmaf(t, dz, oz);
        const float theta = atan2f(sqrtf(fmaf(pz, pz, px * px)), py);
        const float phi = atan2f(pz, px);
        cx = fmaf(2 * theta, RM_RPI_BG, -1.0f);
        cy = phi * RM_RPI_BG;
    }
    const float u = (cx + 1.0f) / 2.0f, v = (cy + 1.0f) / 2.0f;  // GridEncoder._unit_cube(x, bound=1)
    const bool inside = !(u < 0 || u > 1 || v < 0 || v > 1);
#pragma unroll
    for (int l = 0; l < BG_LEVELS; l++) {
        float r0 = 0.0f, r1 = 0.0f;
        if (inside) {
            const uint32_t off0 = (uint32_t)offsets[l], size = (uint32_t)offsets[l + 1] - off0;
            const float pu = fmaf(u, lv.scale[l], 0.5f), pv = fmaf(v, lv.scale[l], 0.5f);
            const uint32_t gu = (uint32_t)floorf(pu), gv = (uint32_t)floorf(pv);
            const float fu = pu - (float)gu, fv = pv - (float)gv;
#pragma unroll
            for (uint32_t idx = 0; idx < 4; idx++) {
                float w = 1;
                w *= (idx & 1u) ? fu : 1 - fu;
                w *= (idx & 2u) ? fv : 1 - fv;
                const uint32_t row = off0 + bg_index(size, lv.resolution[l], gu + (idx & 1u), gv + ((idx >> 1) & 1u));
                const float2 e = *reinterpret_cast<const float2 *>(emb + (uint64_t)row * 2);
                r0 = fmaf(w, bg_h(e.x), r0);
                r1 = fmaf(w, bg_h(e.y), r1);
                if (CORNERS) { rows[l][idx] = row; wts[l][idx] = w; }
            }
        }
        x[16 + 2 * l] = bg_h(r0);
        x[17 + 2 * l] = bg_h(r1);
    }
    return inside;
}

// weights -> LDS as fp32: W0[n][j] at n * 24 + j, W1[k][n] at 1536 + k * 64 + n
__device__ __forceinline__ void bg_stage_weights(const _Float16 *__restrict__ W, float *w) {
    for (uint32_t i = threadIdx.x; i < BG_DW; i += blockDim.x) {
        const uint32_t src = i < BG_HIDDEN * BG_IN ? (i / BG_IN) * BG_W0_LD + i % BG_IN : BG_HIDDEN * BG_W0_LD + (i - BG_HIDDEN * BG_IN);
        w[i] = (float)W[src];
    }
    __syncthreads();
}

// output logits o[3] (fp16 values). Layer 0 runs neuron by neuron and each ReLU'd value goes straight into the output sums (in neuron
// order, as a dense second layer would add them), so no [64] activation vector stays live; `as_col` (or null) receives the activations
// with a stride of BG_LDS_LD (the backward's LDS column of this ray).
__device__ __forceinline__ void bg_mlp(const float *w, const float (&x)[BG_IN], float (&o)[BG_OUT], _Float16 *as_col) {
#pragma unroll
    for (int k = 0; k < BG_OUT; k++) o[k] = 0.0f;
#pragma unroll 2
    for (int m = 0; m < BG_HIDDEN; m++) {
        float z = 0.0f;
#pragma unroll
        for (int j = 0; j < BG_IN; j++) z = fmaf(w[m * BG_IN + j], x[j], z);
        const float hz = bg_h(z);
        const float am = hz > 0.0f ? hz : 0.0f;
        if (as_col) as_col[m * BG_LDS_LD] = (_Float16)am;
#pragma unroll
        for (int k = 0; k < BG_OUT; k++) o[k] = fmaf(w[BG_HIDDEN * BG_IN + k * BG_HIDDEN + m], am, o[k]);
    }
#pragma unroll
    for (int k = 0; k < BG_OUT; k++) o[k] = bg_h(o[k]);
}

// torch.sigmoid on a half tensor: evaluated in fp32, rounded to half — sample_math.h foc_sigmoid_h's expression, rounded through foc_f2h
// (bg_h, like every rounding of this file) where foc_sigmoid_h casts directly. The values are the same; the barrier in foc_f2h makes the
// compiler emit another instruction sequence for k_bg_forward / k_bg_backward, so this form stays here, with the kernels it was measured in.
__device__ __forceinline__ float bg_sigmoid_h(float v) { return bg_h(1.0f / (1.0f + expf(-v))); }

__global__ void __launch_bounds__(256) k_bg_forward(const float *__restrict__ rays_o, const float *__restrict__ rays_d, const float *__restrict__ coords,
                                                    float radius, uint32_t N, const float *__restrict__ emb, const int32_t *__restrict__ offsets,
                                                    BgLevels lv, const _Float16 *__restrict__ W, _Float16 *__restrict__ rgb) {
    __shared__ float w[BG_DW];
    bg_stage_weights(W, w);
    for (uint32_t n = blockIdx.x * 256 + threadIdx.x; n < N; n += gridDim.x * 256) {
        float x[BG_IN], o[BG_OUT];
        uint32_t rows[BG_LEVELS][4];
        float wts[BG_LEVELS][4];
        bg_input<false>(rays_o, rays_d, coords, radius, n, emb, offsets, lv, x, rows, wts);
        bg_mlp(w, x, o, nullptr);
#pragma unroll
        for (int k = 0; k < BG_OUT; k++) rgb[(uint64_t)n * 3 + k] = foc_f2h(bg_sigmoid_h(o[k]));
    }
}

// FOC_DETERMINISTIC: one entry per touched table row, open addressing with linear probing in a zeroed table of 2^k >= 32 N entries (a ray
// touches at most 16 rows: the table is at most half full, a probe always ends). |w g| < 2^16 (g a half, w <= 1), so an addend is below
// 2^56 and is exact from 2^-16 up; smaller ones are rounded to 2^-40. The sums wrap at 2^23, far above what a half gradient can carry.
struct BgDetEntry { uint32_t key, bad; unsigned long long sum[2]; };      // key = row + 1 (0: free); bad bit c: channel c got an inf / NaN addend
static_assert(sizeof(BgDetEntry) == 24, "bg_det_table_bytes");
__device__ __forceinline__ void bg_det_add(BgDetEntry *__restrict__ tab, uint32_t mask, uint32_t row, float v0, float v1) {
    const uint32_t key = row + 1u;
    uint32_t h = (row * 2654435761u) & mask;
    bool mine = false;
    for (uint32_t probe = 0; probe <= mask && !mine; probe++) {
        const uint32_t prev = atomicCAS(&tab[h].key, 0u, key);
        mine = prev == 0u || prev == key;
        if (!mine) h = (h + 1u) & mask;
    }
    if (!mine) return;                                      // cannot happen: the table has more entries than the launch has rows
    const float v[2] = {v0, v1};
#pragma unroll
    for (int c = 0; c < 2; c++) {
        if (v[c] == 0.0f) continue;
        if (!(fabsf(v[c]) < 8388608.0f)) { (void)__hip_atomic_fetch_or(&tab[h].bad, 1u << c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); continue; }
        const long long q = __double2ll_rn((double)v[c] * 1099511627776.0);
        (void)__hip_atomic_fetch_add(&tab[h].sum[c], (unsigned long long)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
__global__ void __launch_bounds__(256) k_bg_det_finish(const BgDetEntry *__restrict__ tab, uint32_t entries, float *__restrict__ grad_emb) {
    for (uint32_t e = blockIdx.x * 256 + threadIdx.x; e < entries; e += gridDim.x * 256) {
        const BgDetEntry t = tab[e];
        if (!t.key) continue;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float a = (t.bad >> c) & 1u ? __builtin_nanf("") : (float)((double)(long long)t.sum[c] * (1.0 / 1099511627776.0));
            if (a != 0.0f) grad_emb[(uint64_t)(t.key - 1u) * 2 + c] += a;        // the one entry of this row: nothing else adds to it
        }
    }
}

// One wave per workgroup; workgroup b takes the 64-ray chunks b, b + G, b + 2G, ... (G = gridDim.x, a function of N only).
__global__ void __launch_bounds__(BG_RAYS) k_bg_backward(const _Float16 *__restrict__ grad_rgb, const float *__restrict__ rays_o,
                                                         const float *__restrict__ rays_d, const float *__restrict__ coords, float radius, uint32_t N,
                                                         const float *__restrict__ emb, const int32_t *__restrict__ offsets, BgLevels lv,
                                                         const _Float16 *__restrict__ W, float *__restrict__ grad_emb, float *__restrict__ partials,
                                                         BgDetEntry *__restrict__ det_tab, uint32_t det_mask) {
    __shared__ float w[BG_DW];
    __shared__ _Float16 xs[BG_IN * BG_LDS_LD], as[BG_HIDDEN * BG_LDS_LD], gzs[BG_HIDDEN * BG_LDS_LD], g2s[BG_OUT * BG_LDS_LD];
    bg_stage_weights(W, w);
    const uint32_t lane = threadIdx.x;
    float acc[BG_IN + BG_OUT];
#pragma unroll
    for (int k = 0; k < BG_IN + BG_OUT; k++) acc[k] = 0.0f;
    const uint32_t chunks = (N + BG_RAYS - 1) / BG_RAYS;
    for (uint32_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint32_t n = ch * BG_RAYS + lane;
        __syncthreads();                                        // the previous chunk's sums are done with the arrays
        if (n < N) {
            float x[BG_IN], o[BG_OUT], g2[BG_OUT], gx[8];
            uint32_t rows[BG_LEVELS][4];
            float wts[BG_LEVELS][4];
            const bool inside = bg_input<true>(rays_o, rays_d, coords, radius, n, emb, offsets, lv, x, rows, wts);
            bg_mlp(w, x, o, as + lane);
#pragma unroll
            for (int j = 0; j < BG_IN; j++) xs[j * BG_LDS_LD + lane] = (_Float16)x[j];
#pragma unroll
            for (int k = 0; k < BG_OUT; k++) {                  // torch's half sigmoid backward: g * (1 - y) * y in fp32, rounded
                const float y = bg_sigmoid_h(o[k]);
                const float g = (float)grad_rgb[(uint64_t)n * 3 + k];
                g2[k] = bg_h(g * (1.0f - y) * y);
                g2s[k * BG_LDS_LD + lane] = (_Float16)g2[k];
            }
#pragma unroll
            for (int i = 0; i < 8; i++) gx[i] = 0.0f;
#pragma unroll 2
            for (int m = 0; m < BG_HIDDEN; m++) {
                // through W1 (rounded as the GEMM's fp16 output), the ReLU gate on the stored activation, then W0's grid columns
                float s = 0.0f;
#pragma unroll
                for (int k = 0; k < BG_OUT; k++) s = fmaf(g2[k], w[BG_HIDDEN * BG_IN + k * BG_HIDDEN + m], s);
                const float gz = (float)as[m * BG_LDS_LD + lane] > 0.0f ? bg_h(s) : 0.0f;
                gzs[m * BG_LDS_LD + lane] = (_Float16)gz;
#pragma unroll
                for (int i = 0; i < 8; i++) gx[i] = fmaf(gz, w[m * BG_IN + 16 + i], gx[i]);
            }
            if (inside && det_tab) {                            // FOC_DETERMINISTIC: the same addends, as integers (bg_det_add)
#pragma unroll
                for (int l = 0; l < BG_LEVELS; l++) {
                    const float g0 = bg_h(gx[2 * l]), g1 = bg_h(gx[2 * l + 1]);
#pragma unroll
                    for (int idx = 0; idx < 4; idx++) {
                        const float v0 = wts[l][idx] * g0, v1 = wts[l][idx] * g1;
                        if (v0 != 0.0f || v1 != 0.0f) bg_det_add(det_tab, det_mask, rows[l][idx], v0, v1);
                    }
                }
            } else if (inside) {                                // the grid columns of the input gradient (fp16, as the GEMM's) -> the table
#pragma unroll
                for (int l = 0; l < BG_LEVELS; l++) {
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        const float g = bg_h(gx[2 * l + c]);
#pragma unroll
                        for (int idx = 0; idx < 4; idx++) {
                            const float v = wts[l][idx] * g;
                            if (v != 0.0f) (void)__hip_atomic_fetch_add(grad_emb + (uint64_t)rows[l][idx] * 2 + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                }
            }
        } else {                                                // past N: zeros in the ray's column
#pragma unroll
            for (int j = 0; j < BG_IN; j++) xs[j * BG_LDS_LD + lane] = (_Float16)0;
#pragma unroll
            for (int m = 0; m < BG_HIDDEN; m++) { as[m * BG_LDS_LD + lane] = (_Float16)0; gzs[m * BG_LDS_LD + lane] = (_Float16)0; }
#pragma unroll
            for (int k = 0; k < BG_OUT; k++) g2s[k * BG_LDS_LD + lane] = (_Float16)0;
        }
        __syncthreads();
        // lane m owns row m of dW0 (24 entries: the sums of gz[m] x[j] over the rays) and column m of dW1 (3 entries: g2[k] a[m]); the
        // rays' x and g2 are broadcast reads
#pragma unroll 2
        for (int r = 0; r < BG_RAYS; r++) {
            const float gz = (float)gzs[lane * BG_LDS_LD + r], am = (float)as[lane * BG_LDS_LD + r];
#pragma unroll
            for (int j = 0; j < BG_IN; j++) acc[j] = fmaf(gz, (float)xs[j * BG_LDS_LD + r], acc[j]);
#pragma unroll
            for (int k = 0; k < BG_OUT; k++) acc[BG_IN + k] = fmaf((float)g2s[k * BG_LDS_LD + r], am, acc[BG_IN + k]);
        }
    }
    float *part = partials + (uint64_t)blockIdx.x * BG_DW;
#pragma unroll
    for (int j = 0; j < BG_IN; j++) part[lane * BG_IN + j] = acc[j];
#pragma unroll
    for (int k = 0; k < BG_OUT; k++) part[BG_HIDDEN * BG_IN + k * BG_HIDDEN + lane] = acc[BG_IN + k];
}

// partials [G, 1728] -> grad_w: the fp32 gradient of the whole blob (3072 entries; the padding entries 0), partials summed in workgroup order
__global__ void __launch_bounds__(256) k_bg_dw_reduce(const float *__restrict__ partials, uint32_t G, float *__restrict__ grad_w) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= BG_BLOB) return;
    int32_t e = -1;
    if (i < BG_HIDDEN * BG_W0_LD) {
        const uint32_t m = i / BG_W0_LD, j = i % BG_W0_LD;
        if (j < BG_IN) e = (int32_t)(m * BG_IN + j);
    } else {
        const uint32_t f = i - BG_HIDDEN * BG_W0_LD, k = f / BG_HIDDEN;
        if (k < BG_OUT) e = (int32_t)(BG_HIDDEN * BG_IN + f);
    }
    float s = 0.0f;
    if (e >= 0)
        for (uint32_t b = 0; b < G; b++) s += partials[(uint64_t)b * BG_DW + e];
    grad_w[i] = s;
}

static void bg_levels(float S, uint32_t H, BgLevels &lv) {
    for (uint32_t l = 0; l < BG_LEVELS; l++) {           // gridencoder.hip ge_make_levels (gridencoder.cu:138-139)
        const float sc = exp2f((float)l * S) * (float)H - 1.0f;
        lv.scale[l] = sc;
        lv.resolution[l] = (uint32_t)ceil((double)sc) + 1;
    }
}

static uint32_t bg_workgroups(uint32_t N) {
    const uint32_t chunks = foc_div_up(N, BG_RAYS);
    return chunks < BG_MAX_WG ? chunks : BG_MAX_WG;
}

static int bg_check(const char *who, const float *rays_o, const float *rays_d, const float *coords, float radius, const float *emb,
                    const int32_t *offsets, const void *weights) {
    FOC_REQUIRE(rays_d && emb && offsets && weights, FOC_E_INVALID, "%s: null pointer", who);
    FOC_REQUIRE(coords || rays_o, FOC_E_INVALID, "%s: null pointer (coords or rays_o)", who);
    FOC_REQUIRE(coords || radius > 0.0f, FOC_E_INVALID, "%s: radius must be > 0 when the coordinates come from the rays", who);
    return FOC_OK;
}

extern "C" {

// FOC_DETERMINISTIC: entries of the row table behind the partials (a power of two, at least twice the 16 N rows a launch can touch)
static uint32_t bg_det_entries(uint32_t N) {
    uint32_t e = 1024u;
    while (e < (1u << 31) && (uint64_t)e < 32ull * N) e <<= 1;
    return e;
}
static uint64_t bg_partials_bytes(uint32_t N) { return ((uint64_t)bg_workgroups(N) * BG_DW * sizeof(float) + 255) & ~(uint64_t)255; }
static uint64_t bg_workspace_bytes(uint32_t N, bool det) {
    if (!det) return (uint64_t)bg_workgroups(N) * BG_DW * sizeof(float);
    return bg_partials_bytes(N) + (uint64_t)bg_det_entries(N) * sizeof(BgDetEntry);
}
uint64_t foc_background_backward_workspace_bytes(uint32_t N) { return bg_workspace_bytes(N, foc_opt(FOC_OPT_DETERMINISTIC) != 0); }

int foc_background_forward(const float *rays_o, const float *rays_d, const float *coords, float radius, uint32_t N, const float *embeddings,
                           const int32_t *offsets, float per_level_scale_log2, uint32_t base_resolution, const void *weights, void *rgb,
                           void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_d);
    if (N == 0) return FOC_OK;
    if (int rc = bg_check("background_forward", rays_o, rays_d, coords, radius, embeddings, offsets, weights)) return rc;
    FOC_REQUIRE(rgb, FOC_E_INVALID, "background_forward: null pointer (rgb)");
    BgLevels lv;
    bg_levels(per_level_scale_log2, base_resolution, lv);
    hipLaunchKernelGGL(k_bg_forward, dim3(foc_grid_1d(N, 256)), dim3(256), 0, (hipStream_t)stream, rays_o, rays_d, coords, radius, N, embeddings,
                       offsets, lv, (const _Float16 *)weights, (_Float16 *)rgb);
    FOC_CHECK_LAUNCH("background_forward");
    return FOC_OK;
}

int foc_background_backward(const void *grad_rgb, const float *rays_o, const float *rays_d, const float *coords, float radius, uint32_t N,
                            const float *embeddings, const int32_t *offsets, float per_level_scale_log2, uint32_t base_resolution,
                            const void *weights, float *grad_embeddings, float *grad_weights, void *workspace, uint64_t workspace_bytes,
                            void *stream) {
    FocDeviceGuard foc_guard_(stream, grad_weights);
    FOC_REQUIRE(grad_weights, FOC_E_INVALID, "background_backward: null pointer (grad_weights)");
    const uint32_t G = N ? bg_workgroups(N) : 0u;
    if (N) {
        if (int rc = bg_check("background_backward", rays_o, rays_d, coords, radius, embeddings, offsets, weights)) return rc;
        FOC_REQUIRE(grad_rgb && grad_embeddings && workspace, FOC_E_INVALID, "background_backward: null pointer");
        const bool det = foc_opt(FOC_OPT_DETERMINISTIC) != 0;      // read once: the size asked for and the launches agree
        const uint64_t need = bg_workspace_bytes(N, det);
        FOC_REQUIRE(workspace_bytes >= need, FOC_E_INVALID, "background_backward: workspace of %llu bytes, %u rays need %llu "
                    "(foc_background_backward_workspace_bytes%s)", (unsigned long long)workspace_bytes, N, (unsigned long long)need,
                    det ? "; FOC_DETERMINISTIC adds the row table" : "");
        FOC_REQUIRE(!det || N <= (1u << 26), FOC_E_INVALID, "background_backward: FOC_DETERMINISTIC serves up to 2^26 rays per call (got %u)", N);
        BgDetEntry *det_tab = det ? reinterpret_cast<BgDetEntry *>(reinterpret_cast<char *>(workspace) + bg_partials_bytes(N)) : nullptr;
        const uint32_t det_entries = det ? bg_det_entries(N) : 0u;
        if (det && foc_zero_async(det_tab, (size_t)det_entries * sizeof(BgDetEntry), (hipStream_t)stream) != hipSuccess) {
            foc_set_error("background_backward: zero fill of the row table failed");
            return FOC_E_LAUNCH;
        }
        BgLevels lv;
        bg_levels(per_level_scale_log2, base_resolution, lv);
        hipLaunchKernelGGL(k_bg_backward, dim3(G), dim3(BG_RAYS), 0, (hipStream_t)stream, (const _Float16 *)grad_rgb, rays_o, rays_d, coords, radius,
                           N, embeddings, offsets, lv, (const _Float16 *)weights, grad_embeddings, (float *)workspace, det_tab, det_entries - 1u);
        FOC_CHECK_LAUNCH("background_backward");
        if (det) {
            hipLaunchKernelGGL(k_bg_det_finish, dim3(foc_grid_1d(det_entries, 256)), dim3(256), 0, (hipStream_t)stream, (const BgDetEntry *)det_tab, det_entries, grad_embeddings);
            FOC_CHECK_LAUNCH("background_backward(deterministic finish)");
        }
    }
    hipLaunchKernelGGL(k_bg_dw_reduce, dim3(foc_div_up(BG_BLOB, 256)), dim3(256), 0, (hipStream_t)stream, (const float *)workspace, G, grad_weights);
    FOC_CHECK_LAUNCH("background_dw_reduce");
    return FOC_OK;
}

}  // extern "C"
