// ge_common.h — the grid encoder's general path, stated once for every input dimension and shared by gridencoder.hip (D = 2 / 3, the
// dimension a compile-time value) and gridencoder_nd.hip (D = 4 / 5, a runtime value): storage-type helpers; the arithmetic of one
// (point, level) — point load, row index, cell, corner loop; the D = 3 forward specialisations; the general kernels (forward with dy_dx,
// atomic backward, grad_inputs, grad_tv) templated on <T, DIM, C>; their launches and the one host dispatch over (dtype, C).
// Semantics: gridencoder/src/gridencoder.cu of the reference (kernel_grid :87-245, kernel_grid_backward :248-340,
// kernel_input_backward :343-369, kernel_grad_tv :506-610). Compiled with -ffp-contract=off; explicit fmaf() mirrors oracle/oracle.c.
#pragma once
#include "common.h"
#include <math.h>
#include <stdlib.h>

#define GE_MAX_LEVELS 32

struct GeLevels {
    float scale[GE_MAX_LEVELS];
    uint32_t resolution[GE_MAX_LEVELS];
    uint32_t merge_max_res;                    // binned backward: levels up to this resolution merge runs of samples in one cell (count + scatter)
};

// Host: the per-level scale and resolution of a call (L <= GE_MAX_LEVELS, else 1), and the merge threshold of the binned backward
static int ge_make_levels(uint32_t L, float S, uint32_t H, GeLevels &lv) {
    if (L > GE_MAX_LEVELS) return 1;
    for (uint32_t l = 0; l < L; l++) {
        // gridencoder.cu:138-139, evaluated with the host libm (identical to oracle/oracle.c)
        const float sc = exp2f((float)l * S) * (float)H - 1.0f;
        lv.scale[l] = sc;
        lv.resolution[l] = (uint32_t)ceil((double)sc) + 1;
    }
    for (uint32_t l = L; l < GE_MAX_LEVELS; l++) { lv.scale[l] = 0; lv.resolution[l] = 1; }
    int merge_res = foc_opt(FOC_OPT_GB_MERGE_MAX_RES);                 // <= 1023: the run key packs 10 bits per axis
    if (merge_res > 1023) merge_res = 1023;
    if (merge_res < 0) merge_res = 0;
    lv.merge_max_res = (uint32_t)merge_res;
    return 0;
}

// ---- storage-type helpers -------------------------------------------------------------
// Keeps an fp32 value materialised in a VGPR. Without it LLVM folds `(half)fma(a,b,c)` into
// v_fma_mixlo_f16, which rounds the exact fma ONCE to fp16; the reference (and the oracle) round to
// fp32 first and then to fp16, and the two differ on fp32 values that sit on an fp16 tie.
__device__ __forceinline__ float ge_opaque(float v) { asm volatile("" : "+v"(v)); return v; }

template <typename T> struct GeT;
template <> struct GeT<float> {
    static __device__ __forceinline__ float ld(const float *p) { return *p; }
    static __device__ __forceinline__ void st(float *p, float v) { *p = v; }
};
template <> struct GeT<__half> {
    static __device__ __forceinline__ float ld(const __half *p) { return __half2float(*p); }
    static __device__ __forceinline__ void st(__half *p, float v) { *p = __float2half_rn(ge_opaque(v)); }
};

template <typename T, uint32_t C> struct GeVec;
// loads C consecutive table entries as floats with the widest aligned access
template <uint32_t C> struct GeVec<float, C> {
    static __device__ __forceinline__ void ld(const float *p, float (&v)[C]) {
        if constexpr (C == 1) v[0] = p[0];
        else if constexpr (C == 2) { const float2 t = *reinterpret_cast<const float2 *>(p); v[0] = t.x; v[1] = t.y; }
        else {
#pragma unroll
            for (uint32_t i = 0; i < C; i += 4) { const float4 t = *reinterpret_cast<const float4 *>(p + i); v[i] = t.x; v[i + 1] = t.y; v[i + 2] = t.z; v[i + 3] = t.w; }
        }
    }
    static __device__ __forceinline__ void st(float *p, const float (&v)[C]) {
        if constexpr (C == 1) p[0] = v[0];
        else if constexpr (C == 2) *reinterpret_cast<float2 *>(p) = make_float2(v[0], v[1]);
        else {
#pragma unroll
            for (uint32_t i = 0; i < C; i += 4) *reinterpret_cast<float4 *>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
        }
    }
};
template <uint32_t C> struct GeVec<__half, C> {
    static __device__ __forceinline__ void ld(const __half *p, float (&v)[C]) {
        if constexpr (C == 1) v[0] = __half2float(p[0]);
        else {
#pragma unroll
            for (uint32_t i = 0; i < C; i += 2) { const float2 t = __half22float2(*reinterpret_cast<const __half2 *>(p + i)); v[i] = t.x; v[i + 1] = t.y; }
        }
    }
    static __device__ __forceinline__ void st(__half *p, const float (&v)[C]) {
        if constexpr (C == 1) p[0] = __float2half_rn(ge_opaque(v[0]));
        else {
#pragma unroll
            for (uint32_t i = 0; i < C; i += 2) *reinterpret_cast<__half2 *>(p + i) = __halves2half2(__float2half_rn(ge_opaque(v[i])), __float2half_rn(ge_opaque(v[i + 1])));
        }
    }
};


// ---- gradient scatter: one packed atomic per pair of channels (fp16) / one per channel (fp32) ----------
template <typename T> struct GeAtomic;
template <> struct GeAtomic<float> {
    template <uint32_t C> static __device__ __forceinline__ void add(float *p, const float (&v)[C]) {
#pragma unroll
        for (uint32_t c = 0; c < C; c++)
            if (v[c] != 0.0f) (void)__hip_atomic_fetch_add(p + c, v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
template <> struct GeAtomic<__half> {
    template <uint32_t C> static __device__ __forceinline__ void add(__half *p, const float (&v)[C]) {
        if constexpr (C == 1) {
            // C == 1 under fp16 is never produced by the reference wrapper (grid.py:43: half only when C % 2 == 0);
            // handled with a CAS loop on the containing dword for completeness.
            const __half hv = __float2half_rn(ge_opaque(v[0]));
            if (__half2float(hv) == 0.0f) return;
            uint32_t *w = reinterpret_cast<uint32_t *>(reinterpret_cast<uintptr_t>(p) & ~(uintptr_t)3);
            const bool hi = (reinterpret_cast<uintptr_t>(p) & 2) != 0;
            uint32_t old = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), assumed;
            do {
                assumed = old;
                const uint16_t cur = hi ? (uint16_t)(assumed >> 16) : (uint16_t)(assumed & 0xFFFFu);
                const __half sum = __float2half_rn(__half2float(__ushort_as_half(cur)) + __half2float(hv));
                const uint32_t nv = hi ? ((assumed & 0x0000FFFFu) | ((uint32_t)__half_as_ushort(sum) << 16))
                                       : ((assumed & 0xFFFF0000u) | (uint32_t)__half_as_ushort(sum));
                old = assumed;
                __hip_atomic_compare_exchange_strong(w, &old, nv, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } while (old != assumed);
        } else {
            typedef _Float16 __attribute__((ext_vector_type(2))) v2h;
#pragma unroll
            for (uint32_t c = 0; c < C; c += 2) {
                // the reference rounds each addend to half before the packed atomic (gridencoder.cu:329)
                v2h hv;
                hv[0] = (_Float16)ge_opaque(v[c]);
                hv[1] = (_Float16)ge_opaque(v[c + 1]);
                if ((float)hv[0] == 0.0f && (float)hv[1] == 0.0f) continue;
                (void)__builtin_amdgcn_global_atomic_fadd_v2f16(
                    (__attribute__((address_space(1))) v2h *)(p + c), hv);
            }
        }
    }
};


// ================================================================= the arithmetic of one (point, level), stated once for every D
// The input dimension is a compile-time value for D = 2, 3 (every loop over axes and corners unrolls; the D = 3 specialisations below
// sit behind `DIM::STATIC == 3`) or a runtime value for D = 4, 5 (gridencoder_nd.hip: 16 / 32 unrolled corners per (D, C, dtype)
// multiplied the build time of the library). MAX sizes the per-axis arrays; STATIC is the dimension where the compiler knows it, else 0.
template <uint32_t N> struct GeDimCT {
    static constexpr uint32_t MAX = N, STATIC = N, UNROLL = 1u << N;
    __host__ __device__ __forceinline__ constexpr GeDimCT(uint32_t = N) {}
    __host__ __device__ __forceinline__ constexpr uint32_t n() const { return N; }
};
struct GeDimRT {
    static constexpr uint32_t MAX = 5, STATIC = 0, UNROLL = 1;
    uint32_t d;
    __host__ __device__ __forceinline__ explicit GeDimRT(uint32_t d_) : d(d_) {}
    __host__ __device__ __forceinline__ uint32_t n() const { return d; }
};
// Loops over the axes and corners carry `#pragma unroll DIM::UNROLL`: every such loop unrolls in full for a compile-time dimension
// (UNROLL = 2^N covers the longest of them) and is left a loop for a runtime one (a plain `#pragma unroll` on a runtime bound cannot
// be honoured and says so under -Wall).

// the point b of `inputs` (fp32 positions; grad_tv passes them in the table dtype) -> x; true when it lies outside [0, 1]^D
template <typename DIM, typename E>
__device__ __forceinline__ bool ge_load_point(DIM dim, const E *__restrict__ inputs, uint32_t b, float (&x)[DIM::MAX]) {
    bool oob = false;
#pragma unroll DIM::UNROLL
    for (uint32_t d = 0; d < dim.n(); d++) { x[d] = GeT<E>::ld(inputs + (uint64_t)b * dim.n() + d); oob |= (x[d] < 0 || x[d] > 1); }
    return oob;
}

// ---- row index (gridencoder.cu:50-84) --------------------------------------------------
template <typename DIM>
__device__ __forceinline__ uint32_t ge_index(DIM dim, uint32_t gridtype, bool align_corners, uint32_t hashmap_size, uint32_t resolution,
                                             const uint32_t (&pos_grid)[DIM::MAX]) {
    constexpr uint32_t primes[7] = {1u, 2654435761u, 805459861u, 3674653429u, 2097192037u, 1434869437u, 2165219737u};
    uint32_t stride = 1, index = 0;
#pragma unroll DIM::UNROLL
    for (uint32_t d = 0; d < dim.n(); d++) {
        if (stride <= hashmap_size) {
            index += pos_grid[d] * stride;
            stride *= align_corners ? resolution : (resolution + 1);
        }
    }
    if (gridtype == 0 && stride > hashmap_size) {
        uint32_t result = 0;
#pragma unroll DIM::UNROLL
        for (uint32_t i = 0; i < dim.n(); i++) { result ^= pos_grid[i] * primes[i]; }
        index = result;
    }
    // `index % hashmap_size` (gridencoder.cu:83) without the integer division in the common cases: dense levels have
    // index < size already, hashed levels have a power-of-two size (2^log2_hashmap_size); the generic path remains for
    // tiled grids / odd sizes. A runtime u32 modulo is ~35 VALU instructions and this runs 2^D times per (point, level).
    if (index >= hashmap_size) index = ((hashmap_size & (hashmap_size - 1u)) == 0u) ? (index & (hashmap_size - 1u)) : (index % hashmap_size);
    return index;                  // row index; caller multiplies by C
}

// ---- cell and in-cell position of one (point, level) (gridencoder.cu:147-159), pos_deriv where the caller writes dy_dx ------------
// `pos -= fl` stands for the reference's `pos -= (float)pos_grid`: fl is a whole number, so for 0 <= fl < 2^32 the conversion to
// uint32 and back returns it and the two forms give the same bits; one conversion less per axis. A point outside [0, 1]^D (fl may be
// negative there) never gets this far with its value used: the forward stores zeros for it before it calls ge_cell, k_grid_bwd and
// k_grad_tv return at the point load, and the binned count / scatter kernels discard the cell of a point that is not `inside`.
// (Two fp32 D = 3 C = 4 forward kernels notice the form. k_grid_fwd_lbc<float, 3, 4> keeps fl live beside the converted cell: 80 -> 84
// VGPRs, 6 -> 5 waves per SIMD, and runs in 0.992 / 0.999 of the parent's time without / with dy_dx. k_grid_fwd_bl<float, 3, 4> with
// dy_dx, 90 -> 88 VGPRs and 5 waves as before, takes 1.024 of it — 0.995 with the conversion form, which would put three conversions per
// level back into the count and scatter kernels of the training step. Pinning pos after ge_cell brings lbc to 76 VGPRs and costs
// both point-major C = 4 forwards 3-4 %. NOTEBOOK.md.)
template <typename DIM>
__device__ __forceinline__ void ge_cell(DIM dim, const float (&x)[DIM::MAX], float scale, bool align_corners, uint32_t interp,
                                        uint32_t (&pos_grid)[DIM::MAX], float (&pos)[DIM::MAX], float *pos_deriv = nullptr) {
#pragma unroll DIM::UNROLL
    for (uint32_t d = 0; d < dim.n(); d++) {
        pos[d] = fmaf(x[d], scale, align_corners ? 0.0f : 0.5f);
        const float fl = floorf(pos[d]);
        pos_grid[d] = (uint32_t)fl;
        pos[d] -= fl;
        if (pos_deriv) pos_deriv[d] = 1.0f;
        if (interp == 1) {                                       // smoothstep
            const float v = pos[d];
            if (pos_deriv) pos_deriv[d] = 6 * v * (1.0f - v);
            pos[d] = v * v * fmaf(-2.0f, v, 3.0f);
        }
    }
}

// ---- corner idx of the cell (gridencoder.cu:167-191): w *= its interpolation weight, pgl = its grid position; bit k of idx set = +1
// along the k-th axis. `skip` (the dy_dx loop, :201-244) leaves one axis out of both: the bits of idx then count the remaining axes.
template <typename DIM>
__device__ __forceinline__ void ge_corner(DIM dim, uint32_t idx, const float (&pos)[DIM::MAX], const uint32_t (&pos_grid)[DIM::MAX], float &w,
                                          uint32_t (&pgl)[DIM::MAX], uint32_t skip = ~0u) {
#pragma unroll DIM::UNROLL
    for (uint32_t d = 0; d < dim.n(); d++) {
        if (d == skip) continue;
        const uint32_t bit = d > skip ? d - 1u : d;
        const bool up = (idx & (1u << bit)) != 0;
        w *= up ? pos[d] : 1 - pos[d];
        pgl[d] = pos_grid[d] + (up ? 1u : 0u);
    }
}

// Decode a linear block id into (level, chunk) so that all blocks of a level share
// blockIdx % 8, i.e. one XCD under the observed round-robin dispatch.
__device__ __forceinline__ bool ge_decode_block(uint32_t id, uint32_t chunks, uint32_t L, uint32_t &level, uint32_t &chunk) {
    const uint32_t xcd = id & 7u, j = id >> 3;
    level = xcd + 8u * (j / chunks);
    chunk = j % chunks;
    return level < L;
}
static inline uint32_t ge_xcd_grid(uint32_t chunks, uint32_t L) { return 8u * chunks * ((L + 7u) / 8u); }

// ================================================================= forward
// The same 8 rows for D = 3 with the per-level decisions (which dimensions enter the dense index, dense or hashed, power-of-two
// size) taken once on wave-uniform values and the per-axis terms shared between the corners: (p+1)*k = p*k + k in uint32, so every
// row is two adds or two xors instead of ge_index's per-corner multiplies and branches. Bit-identical to ge_index per corner (corner idx: bit d set = +1 along axis d).
__device__ __forceinline__ void ge_rows3(const uint32_t (&pos_grid)[3], uint32_t hashmap_size, uint32_t resolution, uint32_t gridtype,
                                              bool align_corners, uint32_t (&rows)[8], bool *is_hashed = nullptr) {
    const uint32_t r1 = align_corners ? resolution : resolution + 1u;
    uint32_t stride = 1u, st[3];
    bool part[3];
#pragma unroll
    for (int d = 0; d < 3; d++) { part[d] = stride <= hashmap_size; st[d] = part[d] ? stride : 0u; if (part[d]) stride *= r1; }
    const bool hashed = gridtype == 0u && stride > hashmap_size;
    if (is_hashed) *is_hashed = hashed;
    uint32_t t[3][2];
    if (hashed) {
        constexpr uint32_t primes[3] = {1u, 2654435761u, 805459861u};
#pragma unroll
        for (int d = 0; d < 3; d++) { t[d][0] = pos_grid[d] * primes[d]; t[d][1] = t[d][0] + primes[d]; }
    } else {
#pragma unroll
        for (int d = 0; d < 3; d++) { t[d][0] = pos_grid[d] * st[d]; t[d][1] = t[d][0] + st[d]; }
    }
    // `index % hashmap_size` (gridencoder.cu:83), decided once per level: a dense level that takes all three axes has index < size
    // already; a power-of-two size (every hashed level: 2^log2_hashmap_size) is a mask; the division is left for tiled grids with odd sizes
    const bool need_mod = hashed || stride > hashmap_size || !part[2];
    const bool pow2 = (hashmap_size & (hashmap_size - 1u)) == 0u;
    if (!need_mod) {
#pragma unroll
        for (uint32_t idx = 0; idx < 8; idx++) rows[idx] = t[0][idx & 1u] + t[1][(idx >> 1) & 1u] + t[2][(idx >> 2) & 1u];
    } else if (pow2) {
        const uint32_t mask = hashmap_size - 1u;
        if (hashed) {
#pragma unroll
            for (uint32_t idx = 0; idx < 8; idx++) rows[idx] = (t[0][idx & 1u] ^ t[1][(idx >> 1) & 1u] ^ t[2][(idx >> 2) & 1u]) & mask;
        } else {
#pragma unroll
            for (uint32_t idx = 0; idx < 8; idx++) rows[idx] = (t[0][idx & 1u] + t[1][(idx >> 1) & 1u] + t[2][(idx >> 2) & 1u]) & mask;
        }
    } else {
#pragma unroll
        for (uint32_t idx = 0; idx < 8; idx++) {
            const uint32_t a = t[0][idx & 1u], b = t[1][(idx >> 1) & 1u], c = t[2][(idx >> 2) & 1u];
            rows[idx] = (hashed ? (a ^ b ^ c) : (a + b + c)) % hashmap_size;
        }
    }
}

// ---- forward: one (point, level) ---------------------------------------------------------
// out points at the C outputs of this (point, level); dy points at its [D,C] block or null.
template <typename T, typename DIM, uint32_t C, bool PAIRS = false>
__device__ __forceinline__ void ge_forward_one(DIM dim, const float (&x)[DIM::MAX], bool oob, const T *__restrict__ table, uint32_t hashmap_size,
                                               float scale, uint32_t resolution, T *__restrict__ out, T *__restrict__ dy,
                                               uint32_t gridtype, bool align_corners, uint32_t interp) {
    float results[C];
#pragma unroll
    for (uint32_t c = 0; c < C; c++) results[c] = 0.0f;
    if (oob) {                                                   // gridencoder.cu:119-135
        GeVec<T, C>::st(out, results);
        if (dy) {
#pragma unroll DIM::UNROLL
            for (uint32_t d = 0; d < dim.n(); d++) {
#pragma unroll
                for (uint32_t c = 0; c < C; c++) GeT<T>::st(dy + d * C + c, 0.0f);
            }
        }
        return;
    }
    float pos[DIM::MAX], pos_deriv[DIM::MAX];
    uint32_t pos_grid[DIM::MAX];
    ge_cell(dim, x, scale, align_corners, interp, pos_grid, pos, pos_deriv);
    uint32_t rows3[8];
    if constexpr (DIM::STATIC == 3) ge_rows3(pos_grid, hashmap_size, resolution, gridtype, align_corners, rows3);
    constexpr bool paired = PAIRS && DIM::STATIC == 3 && C == 2 && sizeof(T) == 2;
    // compile-time D: all 2^D gathers are issued before any is consumed (latency-bound: keep them in flight); runtime D: corner by corner
    constexpr uint32_t NV = DIM::STATIC ? 1u << DIM::STATIC : 1u;
    float vals[NV][C], ws[NV];
    if constexpr (paired) {
        // The two corners along x of a (y, z) pair are ROW NEIGHBOURS whenever row(x+1) == row(x) ^ 1: always on a dense level with an
        // even row, and on a hashed level for every even x (the hash xors x in with prime 1, so x -> x+1 flips bit 0 only). One
        // 8-byte load of the aligned row pair then serves both corners — the gathers are bound by the number of distinct cache-line
        // requests, not by bytes (tools/bench_gather.hip) — and only the other lanes issue the second, 4-byte load.
        const uint32_t *tw = reinterpret_cast<const uint32_t *>(table);
        uint2 wide[4];
        uint32_t nar[4];
#pragma unroll
        for (int j = 0; j < 4; j++) wide[j] = *reinterpret_cast<const uint2 *>(tw + (rows3[2 * j] & ~1u));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            nar[j] = 0u;
            if (rows3[2 * j + 1] != (rows3[2 * j] ^ 1u)) nar[j] = tw[rows3[2 * j + 1]];
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool odd = (rows3[2 * j] & 1u) != 0u, pr = rows3[2 * j + 1] == (rows3[2 * j] ^ 1u);
            const uint32_t v0 = odd ? wide[j].y : wide[j].x;
            const uint32_t v1 = pr ? (odd ? wide[j].x : wide[j].y) : nar[j];
            const __half2 h0 = *reinterpret_cast<const __half2 *>(&v0), h1 = *reinterpret_cast<const __half2 *>(&v1);
            vals[2 * j][0] = __low2float(h0); vals[2 * j][1] = __high2float(h0);
            vals[2 * j + 1][0] = __low2float(h1); vals[2 * j + 1][1] = __high2float(h1);
        }
    }
#pragma unroll DIM::UNROLL
    for (uint32_t idx = 0; idx < (1u << dim.n()); idx++) {       // :167-191
        const uint32_t slot = DIM::STATIC ? idx : 0u;
        float w = 1;
        uint32_t pgl[DIM::MAX];
        ge_corner(dim, idx, pos, pos_grid, w, pgl);
        ws[slot] = w;
        if constexpr (!paired) {
            uint32_t row;
            if constexpr (DIM::STATIC == 3) row = rows3[idx];
            else row = ge_index(dim, gridtype, align_corners, hashmap_size, resolution, pgl);
            GeVec<T, C>::ld(table + (uint64_t)row * C, vals[slot]);
        }
        if constexpr (DIM::STATIC == 0) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) results[c] = fmaf(ws[0], vals[0][c], results[c]);
        }
    }
    if constexpr (DIM::STATIC != 0) {
#pragma unroll
        for (uint32_t idx = 0; idx < NV; idx++) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) results[c] = fmaf(ws[idx], vals[idx][c], results[c]);
        }
    }
    GeVec<T, C>::st(out, results);

    if (!dy) return;
#pragma unroll DIM::UNROLL
    for (uint32_t gd = 0; gd < dim.n(); gd++) {                  // :201-244
        float rg[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) rg[c] = 0.0f;
#pragma unroll DIM::UNROLL
        for (uint32_t idx = 0; idx < (1u << (dim.n() - 1)); idx++) {
            float w = scale;
            uint32_t pgl[DIM::MAX];
            ge_corner(dim, idx, pos, pos_grid, w, pgl, gd);
            pgl[gd] = pos_grid[gd];
            const uint32_t rl = ge_index(dim, gridtype, align_corners, hashmap_size, resolution, pgl);
            pgl[gd] = pos_grid[gd] + 1;
            const uint32_t rr = ge_index(dim, gridtype, align_corners, hashmap_size, resolution, pgl);
            float vl[C], vr[C];
            GeVec<T, C>::ld(table + (uint64_t)rl * C, vl);
            GeVec<T, C>::ld(table + (uint64_t)rr * C, vr);
#pragma unroll
            for (uint32_t c = 0; c < C; c++) rg[c] = fmaf(w * (vr[c] - vl[c]), pos_deriv[gd], rg[c]);
        }
#pragma unroll
        for (uint32_t c = 0; c < C; c++) GeT<T>::st(dy + gd * C + c, rg[c]);
    }
}

// ---- forward, the shape FOC runs: hash gridtype, align_corners off, linear interpolation, fp16 tables with C = 2, D = 3, no dy_dx, row pairs
// 8-byte aligned. ge_forward_one with every per-call decision already taken: what is left at run time is dense-or-hashed (wave-uniform,
// decided by the caller with ge_level_hashed) and, on a hashed level, ONE lane-divergent branch (x odd: the four x+1 corners are no row
// neighbours and take their own 4-byte loads) instead of four. Same arithmetic in the same order: bit-identical results.
__host__ __device__ __forceinline__ bool ge_level_hashed(uint32_t hashmap_size, uint32_t resolution, uint32_t &st1, uint32_t &st2) {
    const uint32_t r1 = resolution + 1u;                 // the reference's uint32 stride walk (gridencoder.cu:70-83), D = 3
    uint32_t stride = 1u;
    st1 = st2 = 0u;
    if (stride <= hashmap_size) stride *= r1;
    if (stride <= hashmap_size) { st1 = stride; stride *= r1; }
    if (stride <= hashmap_size) { st2 = stride; stride *= r1; }
    return stride > hashmap_size;
}

__device__ __forceinline__ void ge_forward_hash3(const float (&x)[3], bool oob, const uint32_t *__restrict__ tw, uint32_t hashmap_size, bool hashed,
                                                 uint32_t st1, uint32_t st2, float scale, __half *__restrict__ out) {
    if (oob) { *reinterpret_cast<uint32_t *>(out) = 0u; return; }
    float pos[3];
    uint32_t pg[3];
#pragma unroll
    for (int d = 0; d < 3; d++) {
        const float p = fmaf(x[d], scale, 0.5f);         // >= 0.5 here (0 <= x <= 1): truncation is the floor, and p - floor(p) is exact —
        pg[d] = (uint32_t)p;                             // v_fract_f32 returns that same value in one instruction
        pos[d] = __builtin_amdgcn_fractf(p);
    }
    // rows as 32-bit BYTE offsets from the level's base: the loads take the base from scalar registers (global_load ... v_off, s[base])
    // instead of a 64-bit address per lane and load (the launch wrapper admits this path for levels below 2^30 rows only)
    const char *tb = reinterpret_cast<const char *>(tw);
    // b0[j]: BYTE offset of the row of corner (x, y_j, z_j), j = y bit | z bit << 1; the row pair it belongs to starts at b0 & ~7.
    uint32_t b0[4];
    uint2 wide[4];
    uint32_t nar[4] = {0u, 0u, 0u, 0u};
    bool pr[4];
    if (hashmap_size <= (1u << 22)) {
        // Tables of at most 2^22 rows (every NeRF grid: log2_hashmap_size 19): the index arithmetic runs on byte offsets below 2^24 with
        // FULL-RATE 24-bit multiplies. Only the low bits of the hash survive the `% hashmap_size` (a power of two here), and they depend on
        // the low bits of the factors alone: (x ^ y P1 ^ z P2) & m, times 4, == ((x << 2) ^ y (4 (P1 & m)) ^ z (4 (P2 & m))) & (m << 2). The
        // generic form below spends two quarter-rate 32-bit multiplies, a shift and a mask per corner; this one a shift for x, two
        // v_mul_u32_u24 and one xor + and per corner (~20 of the ~100 VALU slots per point and level). A dense level likewise: strides
        // below 2^22, rows below the table size.
        const uint32_t x4 = pg[0] << 2;
        uint32_t yz4[4];
        if (hashed) {
            const uint32_t m = hashmap_size - 1u, m4 = m << 2;
            const uint32_t p1 = (2654435761u & m) << 2, p2 = (805459861u & m) << 2;
            const uint32_t t1 = __umul24(pg[1], p1), t2 = __umul24(pg[2], p2);
            yz4[0] = t1 ^ t2; yz4[1] = (t1 + p1) ^ t2; yz4[2] = t1 ^ (t2 + p2); yz4[3] = (t1 + p1) ^ (t2 + p2);
#pragma unroll
            for (int j = 0; j < 4; j++) b0[j] = (x4 ^ yz4[j]) & m4;
#pragma unroll
            for (int j = 0; j < 4; j++) wide[j] = *reinterpret_cast<const uint2 *>(tb + (b0[j] & ~7u));
            const bool even = (x4 & 4u) == 0u;           // x even: x + 1 == x ^ 1, every (x, x+1) corner pair is an aligned row pair
            if (!even) {
#pragma unroll
                for (int j = 0; j < 4; j++) nar[j] = *reinterpret_cast<const uint32_t *>(tb + (((x4 + 4u) ^ yz4[j]) & m4));
            }
#pragma unroll
            for (int j = 0; j < 4; j++) pr[j] = even;
        } else {
            const uint32_t s1 = st1 << 2, s2 = st2 << 2;
            const uint32_t t1 = __umul24(pg[1], s1), t2 = __umul24(pg[2], s2);
            yz4[0] = t1 + t2; yz4[1] = (t1 + s1) + t2; yz4[2] = t1 + (t2 + s2); yz4[3] = (t1 + s1) + (t2 + s2);
#pragma unroll
            for (int j = 0; j < 4; j++) b0[j] = x4 + yz4[j];
#pragma unroll
            for (int j = 0; j < 4; j++) wide[j] = *reinterpret_cast<const uint2 *>(tb + (b0[j] & ~7u));
#pragma unroll
            for (int j = 0; j < 4; j++) {
                pr[j] = (b0[j] & 4u) == 0u;
                if (!pr[j]) nar[j] = *reinterpret_cast<const uint32_t *>(tb + (b0[j] + 4u));
            }
        }
    } else if (hashed) {
        const uint32_t mask = hashmap_size - 1u;
        const uint32_t t1 = pg[1] * 2654435761u, t2 = pg[2] * 805459861u;
        const uint32_t yz[4] = {t1 ^ t2, (t1 + 2654435761u) ^ t2, t1 ^ (t2 + 805459861u), (t1 + 2654435761u) ^ (t2 + 805459861u)};
#pragma unroll
        for (int j = 0; j < 4; j++) b0[j] = ((pg[0] ^ yz[j]) & mask) << 2;
#pragma unroll
        for (int j = 0; j < 4; j++) wide[j] = *reinterpret_cast<const uint2 *>(tb + (b0[j] & ~7u));
        const bool even = (pg[0] & 1u) == 0u;
        if (!even) {
#pragma unroll
            for (int j = 0; j < 4; j++) nar[j] = *reinterpret_cast<const uint32_t *>(tb + ((((pg[0] + 1u) ^ yz[j]) & mask) << 2));
        }
#pragma unroll
        for (int j = 0; j < 4; j++) pr[j] = even;
    } else {
        const uint32_t t1 = pg[1] * st1, t2 = pg[2] * st2;
        const uint32_t yz[4] = {t1 + t2, (t1 + st1) + t2, t1 + (t2 + st2), (t1 + st1) + (t2 + st2)};
#pragma unroll
        for (int j = 0; j < 4; j++) b0[j] = (pg[0] + yz[j]) << 2;
#pragma unroll
        for (int j = 0; j < 4; j++) wide[j] = *reinterpret_cast<const uint2 *>(tb + (b0[j] & ~7u));
#pragma unroll
        for (int j = 0; j < 4; j++) {
            pr[j] = (b0[j] & 4u) == 0u;
            if (!pr[j]) nar[j] = *reinterpret_cast<const uint32_t *>(tb + (b0[j] + 4u));
        }
    }
    const float wx[2] = {1 - pos[0], pos[0]}, wy[2] = {1 - pos[1], pos[1]}, wz[2] = {1 - pos[2], pos[2]};
    float res0 = 0.0f, res1 = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const bool odd = (b0[j] & 4u) != 0u;
        const uint32_t v0 = odd ? wide[j].y : wide[j].x;
        const uint32_t v1 = pr[j] ? (odd ? wide[j].x : wide[j].y) : nar[j];
        const __half2 h0 = *reinterpret_cast<const __half2 *>(&v0), h1 = *reinterpret_cast<const __half2 *>(&v1);
        const float w0 = (wx[0] * wy[j & 1]) * wz[j >> 1], w1 = (wx[1] * wy[j & 1]) * wz[j >> 1];
        res0 = fmaf(w0, __low2float(h0), res0); res1 = fmaf(w0, __high2float(h0), res1);
        res0 = fmaf(w1, __low2float(h1), res0); res1 = fmaf(w1, __high2float(h1), res1);
    }
    *reinterpret_cast<__half2 *>(out) = __halves2half2(__float2half_rn(ge_opaque(res0)), __float2half_rn(ge_opaque(res1)));
}

// One level of the fast shape or of the general one (`fast`: the launch-wide part of the decision, taken on the host).
// ge_forward_hash3 addresses rows by 32-bit BYTE offsets inside the level: levels of up to 2^30 rows of 4 bytes; a hashed level must
// have a power-of-two size (its `% hashmap_size` is a mask there). Within it, levels of at most 2^22 rows take the 24-bit multiplies.
__host__ __device__ __forceinline__ bool ge_hash3_admits(uint32_t hashmap_size, bool hashed) {
    return (!hashed || (hashmap_size & (hashmap_size - 1u)) == 0u) && hashmap_size <= (1u << 30);
}

template <typename T, typename DIM, uint32_t C>
__device__ __forceinline__ void ge_forward_level(DIM dim, const float (&x)[DIM::MAX], bool oob, const T *__restrict__ grid, uint32_t off0, uint32_t hashmap_size,
                                                 float scale, uint32_t resolution, T *__restrict__ out, T *__restrict__ dy, uint32_t gridtype,
                                                 bool align_corners, uint32_t interp, uint32_t pairs) {
    if constexpr (sizeof(T) == 2 && DIM::STATIC == 3 && C == 2) {              // the tables whose rows travel in pairs
        const bool aligned = ((off0 | hashmap_size) & 1u) == 0u;               // row pairs of this level are 8-byte aligned and inside it
        if (pairs == 2u && aligned) {
            uint32_t st1, st2;
            const bool hashed = ge_level_hashed(hashmap_size, resolution, st1, st2);
            if (ge_hash3_admits(hashmap_size, hashed)) {
                ge_forward_hash3(x, oob, reinterpret_cast<const uint32_t *>(grid) + off0, hashmap_size, hashed, st1, st2, scale,
                                 reinterpret_cast<__half *>(out));
                return;
            }
        }
        if (pairs && aligned) {
            ge_forward_one<T, DIM, C, true>(dim, x, oob, grid + (uint64_t)off0 * C, hashmap_size, scale, resolution, out, dy, gridtype, align_corners, interp);
            return;
        }
    }
    ge_forward_one<T, DIM, C, false>(dim, x, oob, grid + (uint64_t)off0 * C, hashmap_size, scale, resolution, out, dy, gridtype, align_corners, interp);
}

// Encoding workgroup f of a plain level walk -> chunk of 256 points and the range of levels it encodes: the `lc` leading levels (the
// small dense tables, 1.4 MiB together for the default grid) are done by ONE workgroup per chunk, which loads its points once; the
// levels from `lc` up follow one at a time. At those small levels a launch moves 12 bytes of position per 4 bytes of result: what
// they cost is reading the positions (0.015 ms per level and 2 M points), not the gathers.
__device__ __forceinline__ void ge_walk(uint32_t f, uint32_t chunks, uint32_t lc, uint32_t &chunk, uint32_t &l0, uint32_t &l1) {
    const uint32_t grp = f / chunks;
    chunk = f - grp * chunks;
    if (lc < 2u) { l0 = grp; l1 = grp + 1u; }
    else if (grp == 0u) { l0 = 0u; l1 = lc; }
    else { l0 = lc + grp - 1u; l1 = l0 + 1u; }
}

// Level-major launch, outputs [L,B,C]: thread = point. `plain`: blocks are numbered level by level, so the whole chip walks ONE
// level at a time and every XCD's 4 MiB L2 holds that level's table (<= 2 MiB at 2^19 x half2); otherwise a level is pinned to one
// XCD (ge_decode_block), which balances badly because the cost of a level grows ~5x from level 0 to 15 (tools/time_levels.py).
template <typename T, typename DIM, uint32_t C>
__global__ void __launch_bounds__(256) k_grid_fwd_lbc(const float *__restrict__ inputs, const T *__restrict__ grid,
                                                      const int32_t *__restrict__ offsets, T *__restrict__ outputs,
                                                      uint32_t B, uint32_t L, GeLevels lv, T *__restrict__ dy_dx,
                                                      uint32_t gridtype, bool align_corners, uint32_t interp, uint32_t chunks, uint32_t plain,
                                                      uint32_t pairs, uint32_t lc) {
    const DIM dim;                                               // a compile-time dimension (GeDimRT has no default): the runtime one launches k_grid_fwd_pl
    uint32_t chunk, l0, l1;
    if (plain) ge_walk(blockIdx.x, chunks, lc, chunk, l0, l1);
    else { if (!ge_decode_block(blockIdx.x, chunks, L, l0, chunk)) return; l1 = l0 + 1u; }
    const uint32_t b = chunk * 256 + threadIdx.x;
    if (b >= B || l0 >= L) return;
    float x[DIM::MAX];
    const bool oob = ge_load_point(dim, inputs, b, x);
    for (uint32_t level = l0; level < l1; level++) {
        const uint32_t off0 = (uint32_t)offsets[level];
        const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
        T *dy = dy_dx ? dy_dx + ((uint64_t)b * L + level) * dim.n() * C : nullptr;
        ge_forward_level<T, DIM, C>(dim, x, oob, grid, off0, hashmap_size, lv.scale[level], lv.resolution[level], outputs + ((uint64_t)level * B + b) * C, dy,
                                    gridtype, align_corners, interp, pairs);
    }
}

// Point-major launch, outputs [B, L*C]: consecutive lanes = consecutive levels of one point, so
// the wave's store is contiguous. Thread id g -> b = g / L, level = g % L.
template <typename T, typename DIM, uint32_t C>
__global__ void __launch_bounds__(256) k_grid_fwd_bl(const float *__restrict__ inputs, const T *__restrict__ grid,
                                                     const int32_t *__restrict__ offsets, T *__restrict__ outputs,
                                                     uint32_t B, uint32_t L, GeLevels lv, T *__restrict__ dy_dx,
                                                     uint32_t gridtype, bool align_corners, uint32_t interp) {
    const DIM dim;                                               // compile-time dimensions only, like k_grid_fwd_lbc
    const uint64_t total = (uint64_t)B * L;
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < total; g += (uint64_t)gridDim.x * 256) {
        const uint32_t b = (uint32_t)(g / L), level = (uint32_t)(g - (uint64_t)b * L);
        const uint32_t off0 = (uint32_t)offsets[level];
        const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
        float x[DIM::MAX];
        const bool oob = ge_load_point(dim, inputs, b, x);
        T *dy = dy_dx ? dy_dx + ((uint64_t)b * L + level) * dim.n() * C : nullptr;
        ge_forward_one<T, DIM, C>(dim, x, oob, grid + (uint64_t)off0 * C, hashmap_size, lv.scale[level], lv.resolution[level],
                                  outputs + g * C, dy, gridtype, align_corners, interp);
    }
}

// Thread = (point, level) with blockIdx.y = level (gridencoder.cu:103), either output layout: the forward launch of the RUNTIME dimension.
// Under the two launches above the same body needs more registers there — the point stays live across the levels of a walk, or the
// grid-stride loop and its 64-bit division stay live across the body: 64-84 VGPRs for C = 4, 8 against 44-60 here, 5-7 waves per SIMD
// against 8 — and no D = 4 / 5 caller has the 2^19-row levels whose L2 placement those launches are about.
template <typename T, uint32_t C>
__global__ void __launch_bounds__(256) k_grid_fwd_pl(const float *__restrict__ inputs, const T *__restrict__ grid, const int32_t *__restrict__ offsets,
                                                     T *__restrict__ outputs, uint32_t B, uint32_t L, GeLevels lv, T *__restrict__ dy_dx,
                                                     uint32_t gridtype, bool align_corners, uint32_t interp, bool out_bl, uint32_t D) {
    const GeDimRT dim(D);
    const uint32_t level = blockIdx.y, b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float x[GeDimRT::MAX];
    const bool oob = ge_load_point(dim, inputs, b, x);
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
    T *out = out_bl ? outputs + ((uint64_t)b * L + level) * C : outputs + ((uint64_t)level * B + b) * C;
    T *dy = dy_dx ? dy_dx + ((uint64_t)b * L + level) * dim.n() * C : nullptr;
    ge_forward_one<T, GeDimRT, C>(dim, x, oob, grid + (uint64_t)off0 * C, hashmap_size, lv.scale[level], lv.resolution[level], out, dy, gridtype, align_corners, interp);
}

// ================================================================= backward with atomics, grad_inputs, grad_tv
// kernel_grid_backward (gridencoder.cu:248-340): w * grad to the 2^D corners with packed fp16 / fp32 atomics.
// grad layout: GRAD_BL ? [B, L*C] : [L, B, C].  Level-major XCD-aware launch, thread = point.
// (With the cell, corner and index loops in helpers of their own the compiler keeps a wave-uniform branch per corner where the loops
// written in place became selects: 17 more instructions of 340-560 for D = 2, 42-54 of 730-1140 for D = 3, 3-5 VGPRs fewer; the time is
// the atomics' — 1.214 ms before and after for D = 2 fp16 at 2^18 points x 16 levels, NOTEBOOK.md.)
template <typename T, typename DIM, uint32_t C, bool GRAD_BL>
__global__ void __launch_bounds__(256) k_grid_bwd(const T *__restrict__ grad, const float *__restrict__ inputs,
                                                  const int32_t *__restrict__ offsets, T *__restrict__ grad_grid,
                                                  uint32_t B, uint32_t L, GeLevels lv, uint32_t gridtype, bool align_corners,
                                                  uint32_t interp, uint32_t chunks, uint32_t D) {
    const DIM dim(D);
    uint32_t level, chunk;
    if (!ge_decode_block(blockIdx.x, chunks, L, level, chunk)) return;
    const uint32_t b = chunk * 256 + threadIdx.x;
    if (b >= B) return;
    float x[DIM::MAX];
    if (ge_load_point(dim, inputs, b, x)) return;                 // :276-281
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
    float g[C];
    const T *gp = GRAD_BL ? grad + ((uint64_t)b * L + level) * C : grad + ((uint64_t)level * B + b) * C;
    GeVec<T, C>::ld(gp, g);
    bool any = false;
#pragma unroll
    for (uint32_t c = 0; c < C; c++) any |= (g[c] != 0.0f);
    if (!any) return;
    T *grad_table = grad_grid + (uint64_t)off0 * C;
    const uint32_t resolution = lv.resolution[level];
    float pos[DIM::MAX];
    uint32_t pos_grid[DIM::MAX];
    ge_cell(dim, x, lv.scale[level], align_corners, interp, pos_grid, pos);
#pragma unroll DIM::UNROLL
    for (uint32_t idx = 0; idx < (1u << dim.n()); idx++) {
        float w = 1;
        uint32_t pgl[DIM::MAX];
        ge_corner(dim, idx, pos, pos_grid, w, pgl);
        const uint32_t row = ge_index(dim, gridtype, align_corners, hashmap_size, resolution, pgl);
        float v[C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) v[c] = w * g[c];
        GeAtomic<T>::template add<C>(grad_table + (uint64_t)row * C, v);
    }
}

// gridencoder.cu:343-369: grad_inputs[b,d] = sum_{l,c} grad[l,b,c] * dy_dx[b,l,d,c]   (fp32 accumulate)
template <typename T, typename DIM, uint32_t C, bool GRAD_BL>
__global__ void __launch_bounds__(256) k_grid_input_bwd(const T *__restrict__ grad, const T *__restrict__ dy_dx, T *__restrict__ grad_inputs,
                                                        uint32_t B, uint32_t L, uint32_t D_) {
    const uint32_t D = DIM(D_).n();
    const uint64_t total = (uint64_t)B * D;
    for (uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (uint64_t)gridDim.x * 256) {
        const uint32_t b = (uint32_t)(t / D), d = (uint32_t)(t - (uint64_t)b * D);
        float r = 0;
        for (uint32_t l = 0; l < L; l++) {
#pragma unroll
            for (uint32_t c = 0; c < C; c++) {
                const float gv = GeT<T>::ld(GRAD_BL ? grad + ((uint64_t)b * L + l) * C + c : grad + ((uint64_t)l * B + b) * C + c);
                r = fmaf(gv, GeT<T>::ld(dy_dx + (((uint64_t)b * L + l) * D + d) * C + c), r);
            }
        }
        GeT<T>::st(grad_inputs + t, r);
    }
}

// gridencoder.cu:506-610 kernel_grad_tv
// (Runtime D: ~210 instructions more than the kernel it replaces, 790-1080 — each of the three inlined ge_index now carries the mask
// shortcut beside the division the old runtime index always took; D = 4 / 5 at 2^18 points: 0.99 / 0.90 of the time before.)
template <typename T, typename DIM, uint32_t C>
__global__ void __launch_bounds__(256) k_grad_tv(const T *__restrict__ inputs, const T *__restrict__ grid, T *__restrict__ grad,
                                                 const int32_t *__restrict__ offsets, float weight, uint32_t B, uint32_t L,
                                                 GeLevels lv, uint32_t gridtype, bool align_corners, uint32_t chunks, uint32_t D) {
    const DIM dim(D);
    uint32_t level, chunk;
    if (!ge_decode_block(blockIdx.x, chunks, L, level, chunk)) return;
    const uint32_t b = chunk * 256 + threadIdx.x;
    if (b >= B) return;
    float x[DIM::MAX];
    if (ge_load_point(dim, inputs, b, x)) return;
    const uint32_t off0 = (uint32_t)offsets[level];
    const uint32_t hashmap_size = (uint32_t)offsets[level + 1] - off0;
    const uint32_t resolution = lv.resolution[level];
    const T *tab = grid + (uint64_t)off0 * C;
    uint32_t pos_grid[DIM::MAX];
    float pos[DIM::MAX];                                          // the in-cell position is not used: the centre of the stencil is the cell itself
    ge_cell(dim, x, lv.scale[level], align_corners, 0u, pos_grid, pos);
    float results[C], idelta[C], center[C];
#pragma unroll
    for (uint32_t c = 0; c < C; c++) { results[c] = 0; idelta[c] = 0; }
    const uint32_t row = ge_index(dim, gridtype, align_corners, hashmap_size, resolution, pos_grid);
    GeVec<T, C>::ld(tab + (uint64_t)row * C, center);
    const float w = weight / (float)(2 * dim.n());
    const auto neighbour = [&]() __attribute__((always_inline)) {
        float o[C];
        GeVec<T, C>::ld(tab + (uint64_t)ge_index(dim, gridtype, align_corners, hashmap_size, resolution, pos_grid) * C, o);
#pragma unroll
        for (uint32_t c = 0; c < C; c++) { const float gv = center[c] - o[c]; results[c] += gv; idelta[c] = fmaf(gv, gv, idelta[c]); }
    };
#pragma unroll DIM::UNROLL
    for (uint32_t d = 0; d < dim.n(); d++) {
        const uint32_t cur = pos_grid[d];
        if (cur < resolution) { pos_grid[d] = cur + 1; neighbour(); }
        if (cur > 0) { pos_grid[d] = cur - 1; neighbour(); }
        pos_grid[d] = cur;
    }
    float v[C];
#pragma unroll
    for (uint32_t c = 0; c < C; c++) v[c] = w * results[c] * (1.0f / sqrtf(idelta[c] + 1e-9f));
    GeAtomic<T>::template add<C>(grad + ((uint64_t)off0 + row) * C, v);
}

// ================================================================= host side: launches and the one dispatch over (dtype, D, C)
enum GeOp { GE_FORWARD, GE_BACKWARD, GE_TV };
struct GeCall {                                // the arguments of one forward / backward / grad_tv call, checked by the entry point
    int dtype;
    uint32_t D, C, B, L;
    GeLevels lv;
    uint32_t gridtype, interp;
    bool ac, bl;                               // align_corners; [B, L*C] outputs (forward) / gradient (backward)
    const void *inputs;                        // fp32 positions; grad_tv: positions in the table dtype
    const void *emb;                           // forward, grad_tv: the table
    const int32_t *offsets;
    void *out;                                 // forward: outputs; backward: grad_embeddings; grad_tv: grad
    const void *grad;                          // backward: the incoming gradient
    void *dy_dx, *grad_inputs;                 // forward writes dy_dx; backward reads it when grad_inputs is asked for
    float weight;                              // grad_tv
    hipStream_t st;
};

// Leading levels encoded by one workgroup per chunk (ge_walk): resolution <= 160 and at most L / 2 of them; fewer than two -> plain
// walk. Measured on FOC's 16-level grid (forward + count, 2 M points): threshold 63 0.358 ms, 120 0.353, 160 0.350 (8 levels),
// 250 without the L / 2 cap 0.353, 600 0.422, every level 0.640. FOC_GRID_FUSE_SMALL=0 switches it off.
static uint32_t ge_small_levels(uint32_t L, const GeLevels &lv) {
    const int on = foc_opt(FOC_OPT_GRID_FUSE_SMALL);
    if (!on) return 0u;
    const uint32_t finest = on > 1 ? (uint32_t)on : 160u;            // a value above 1 is taken as the resolution threshold (A/B runs)
    const uint32_t most = L / 2;                                     // most levels in the shared group (10 / 12 / 14 / 16 of 16 measured: NOTEBOOK.md, rounds 1-4 section 9)
    uint32_t lc = 0;
    while (lc < most && lc < L && lv.resolution[lc] <= finest) lc++;
    return lc >= 2u ? lc : 0u;
}

// FOC_GRID_PAIRS=0: one 4-byte load per corner (A/B runs). 16-byte groups of 4 rows (which would also cover x = 1 mod 4 on a hashed
// level) were measured SLOWER: 0.064 vs 0.052 ms per 2 M random points and level — the 16-byte gather is not free like the 8-byte one.
static bool ge_pairs_enabled() {
    return foc_opt(FOC_OPT_GRID_PAIRS) != 0;
}
// The `pairs` argument of the level-major forward kernels: 0 = one load per corner, 1 = row pairs, 2 = row pairs and the call is of the
// shape ge_forward_hash3 serves (the per-level part of that decision is taken in the kernel). FOC_GRID_FAST=0: never 2 (A/B runs).
static uint32_t ge_pairs_mode(const void *emb, const void *dy_dx, size_t elem, uint32_t D, uint32_t C, uint32_t gridtype, bool ac, uint32_t interp) {
    const int fast = foc_opt(FOC_OPT_GRID_FAST);
    if (!ge_pairs_enabled() || ((uintptr_t)emb & 7u) != 0u || dy_dx) return 0u;
    return (fast && elem == 2 && D == 3 && C == 2 && gridtype == 0u && !ac && interp == 0u) ? 2u : 1u;
}

template <typename T, typename DIM, uint32_t C>
static int ge_forward_launch(const GeCall &a) {
    if constexpr (DIM::STATIC == 0) {
        hipLaunchKernelGGL((k_grid_fwd_pl<T, C>), dim3(foc_div_up(a.B, 256), a.L), dim3(256), 0, a.st, (const float *)a.inputs, (const T *)a.emb, a.offsets, (T *)a.out,
                           a.B, a.L, a.lv, (T *)a.dy_dx, a.gridtype, a.ac, a.interp, a.bl, a.D);
    } else if (a.bl) {
        const uint64_t total = (uint64_t)a.B * a.L;
        const uint32_t grid = (uint32_t)((total + 255) / 256 > 0x7FFFFFFFull ? 0x7FFFFFFFull : (total + 255) / 256);
        hipLaunchKernelGGL((k_grid_fwd_bl<T, DIM, C>), dim3(grid), dim3(256), 0, a.st, (const float *)a.inputs, (const T *)a.emb, a.offsets, (T *)a.out, a.B, a.L, a.lv,
                           (T *)a.dy_dx, a.gridtype, a.ac, a.interp);
    } else {
        const int lm_plain = 1;                  // blocks numbered level by level: the whole chip walks one level at a time (pinning a level to one XCD balanced badly)
        const uint32_t chunks = foc_div_up(a.B, 256);
        const uint32_t lc = lm_plain ? ge_small_levels(a.L, a.lv) : 0u;
        const uint32_t groups = lc >= 2u ? a.L - lc + 1u : a.L;
        // FOC_GRID_FWD_LDS=<bytes>: unused dynamic LDS per workgroup — caps the resident workgroups per CU (occupancy experiments: what the
        // forward's gathers cost with fewer waves in flight, NOTEBOOK.md, rounds 1-4 section 9)
        const int pad_lds = 0;
        hipLaunchKernelGGL((k_grid_fwd_lbc<T, DIM, C>), dim3(lm_plain ? chunks * groups : ge_xcd_grid(chunks, a.L)), dim3(256), (size_t)pad_lds, a.st, (const float *)a.inputs,
                           (const T *)a.emb, a.offsets, (T *)a.out, a.B, a.L, a.lv, (T *)a.dy_dx, a.gridtype, a.ac, a.interp, chunks, (uint32_t)lm_plain,
                           ge_pairs_mode(a.emb, a.dy_dx, sizeof(T), a.D, C, a.gridtype, a.ac, a.interp), lc);
    }
    FOC_CHECK_LAUNCH("grid_encode_forward");
    return FOC_OK;
}

template <typename T, typename DIM, uint32_t C>
static int ge_input_backward_launch(const void *grad, const void *dy_dx, void *grad_inputs, uint32_t B, uint32_t D, uint32_t L, bool bl, hipStream_t st) {
    const uint32_t g = foc_grid_1d((uint64_t)B * D, 256);
    if (bl) hipLaunchKernelGGL((k_grid_input_bwd<T, DIM, C, true>), dim3(g), dim3(256), 0, st, (const T *)grad, (const T *)dy_dx, (T *)grad_inputs, B, L, D);
    else hipLaunchKernelGGL((k_grid_input_bwd<T, DIM, C, false>), dim3(g), dim3(256), 0, st, (const T *)grad, (const T *)dy_dx, (T *)grad_inputs, B, L, D);
    FOC_CHECK_LAUNCH("grid_encode_backward(inputs)");
    return FOC_OK;
}

template <typename T, typename DIM, uint32_t C>
static int ge_backward_launch(const GeCall &a) {
    const uint32_t chunks = foc_div_up(a.B, 256);
    if (a.bl) hipLaunchKernelGGL((k_grid_bwd<T, DIM, C, true>), dim3(ge_xcd_grid(chunks, a.L)), dim3(256), 0, a.st, (const T *)a.grad, (const float *)a.inputs, a.offsets,
                                 (T *)a.out, a.B, a.L, a.lv, a.gridtype, a.ac, a.interp, chunks, a.D);
    else hipLaunchKernelGGL((k_grid_bwd<T, DIM, C, false>), dim3(ge_xcd_grid(chunks, a.L)), dim3(256), 0, a.st, (const T *)a.grad, (const float *)a.inputs, a.offsets,
                            (T *)a.out, a.B, a.L, a.lv, a.gridtype, a.ac, a.interp, chunks, a.D);
    FOC_CHECK_LAUNCH("grid_encode_backward");
    if (a.dy_dx && a.grad_inputs) return ge_input_backward_launch<T, DIM, C>(a.grad, a.dy_dx, a.grad_inputs, a.B, a.D, a.L, a.bl, a.st);
    return FOC_OK;
}

template <typename T, typename DIM, uint32_t C>
static int ge_tv_launch(const GeCall &a) {
    const uint32_t chunks = foc_div_up(a.B, 256);
    hipLaunchKernelGGL((k_grad_tv<T, DIM, C>), dim3(ge_xcd_grid(chunks, a.L)), dim3(256), 0, a.st, (const T *)a.inputs, (const T *)a.emb, (T *)a.out, a.offsets,
                       a.weight, a.B, a.L, a.lv, a.gridtype, a.ac, chunks, a.D);
    FOC_CHECK_LAUNCH("grad_total_variation");
    return FOC_OK;
}

// (dtype, C) of a call -> the launch of `op` for the dimension type DIM. gridencoder.hip calls it for GeDimCT<2> and GeDimCT<3> after it
// has refused a D outside 2..5, gridencoder_nd.hip for GeDimRT (D = 4, 5); C is refused here, before any launch (gridencoder.cu:381).
template <typename T, typename DIM, uint32_t C>
static int ge_launch(GeOp op, const GeCall &a) {
    switch (op) {
        case GE_FORWARD: return ge_forward_launch<T, DIM, C>(a);
        case GE_BACKWARD: return ge_backward_launch<T, DIM, C>(a);
        default: return ge_tv_launch<T, DIM, C>(a);
    }
}
template <typename DIM>
static int ge_dispatch(GeOp op, const GeCall &a) {
    const bool h16 = a.dtype == FOC_F16;
    switch (a.C) {
        case 1: return h16 ? ge_launch<__half, DIM, 1>(op, a) : ge_launch<float, DIM, 1>(op, a);
        case 2: return h16 ? ge_launch<__half, DIM, 2>(op, a) : ge_launch<float, DIM, 2>(op, a);
        case 4: return h16 ? ge_launch<__half, DIM, 4>(op, a) : ge_launch<float, DIM, 4>(op, a);
        case 8: return h16 ? ge_launch<__half, DIM, 8>(op, a) : ge_launch<float, DIM, 8>(op, a);
        default: foc_set_error("GridEncoding: C must be 1, 2, 4, or 8."); return FOC_E_INVALID;
    }
}
int ge_nd_dispatch(GeOp op, const GeCall &a);   // gridencoder_nd.hip: ge_dispatch<GeDimRT>, a translation unit of its own for the build time
