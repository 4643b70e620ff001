// simplify.hip — vertex clustering of an indexed triangle mesh on a cell grid (no reference binding: the reference hands its mesh to
// trimesh, where a user decimates on the host). include/focnerf.h states the definition; tests/simplify_ref.py is its numpy statement and
// the kernels are held to it bit for bit.
//
//   foc_simplify_count   per vertex its cell number; per triangle the range check of its indices and whether it survives (three different
//                        cells), one ballot word per 64 triangles, and the survivors' cells set in a bit array over the grid (64-bit
//                        atomicOr); popcounts of the cell words and of the triangle words, per group of 64 words, then the group totals
//                        of both through ONE scan (ms_scan.h) -> counts4
//   foc_simplify_emit    per vertex the number of its kept cell (chunk offset + popcount below its bit) and int64 atomicAdd of its
//                        fixed-point coordinates and attributes; per kept cell the mean, normal, colour and id; per triangle the
//                        survivors at chunk offset + popcount below, renumbered and rotated
//
// Only integer atomics (or / add / max): sums do not depend on the order of arrival, the same bits on every run and in both deterministic
// modes. Every index is range-checked before anything is read through it; every store is guarded by the totals of the count pass.
#include <cmath>
#include "common.h"
#include "ms_scan.h"

#define SP_MAX_CELLS (1ull << 30)
#define SP_MAX_ELEMS 0x7FFFFFFFull         // V and F: indices are int32
#define SP_FIX 1073741824.0f               // 2^30: r * 2^30 is exact in fp32 for every fp32 r

struct SpGrid { float o[3], inv[3]; double od[3], celld[3]; uint32_t g[3]; };

// rule 1 on one axis: the cell coordinate, and r = the position inside the cell in [0, 1]
__device__ __forceinline__ uint32_t sp_axis(float v, float o, float inv, uint32_t g, float &r) {
    const float t = __fmul_rn(__fsub_rn(v, o), inv);
    const float f = floorf(t);
    uint32_t c = 0;                                          // f <= 0, or a NaN (such a vertex is counted and the mesh refused)
    if (f > 0.0f) c = f >= 2147483648.0f ? g - 1u : min((uint32_t)f, g - 1u);
    r = fminf(fmaxf(__fsub_rn(t, (float)c), 0.0f), 1.0f);
    return c;
}
__device__ __forceinline__ bool sp_finite(float v) { return fabsf(v) <= 3.402823466e38f; }     // false for NaN
__device__ __forceinline__ unsigned long long sp_fixed(float r) { return (unsigned long long)(long long)__fmul_rn(r, SP_FIX); }
// one atomicAdd of the lanes' count where `flag` holds (rare: a refused mesh)
__device__ __forceinline__ void sp_count_flag(bool flag, uint32_t *__restrict__ counter) {
    const uint64_t b = __ballot(flag);
    if (flag && (threadIdx.x & 63) == (uint32_t)(__ffsll((long long)b) - 1)) atomicAdd(counter, (uint32_t)__popcll(b));
}

// the workspace: Wc cell words, Wt triangle words, G = max of their group counts
struct SpWs { uint32_t *totals; uint64_t *bits; uint32_t *gc, *gt; uint64_t *tmask; uint32_t *coff, *toff, *vcell; };

// ---------------------------------------------------------------- count, pass 1: the cell of every vertex
__global__ void __launch_bounds__(256) k_sp_cell(const float *__restrict__ vertices, uint32_t V, SpGrid G, uint32_t *__restrict__ vcell,
                                                 uint32_t *__restrict__ bad_vertices) {
    for (uint32_t v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        const float *p = vertices + (uint64_t)v * 3;
        const float x = p[0], y = p[1], z = p[2];
        float r;
        const uint32_t cx = sp_axis(x, G.o[0], G.inv[0], G.g[0], r), cy = sp_axis(y, G.o[1], G.inv[1], G.g[1], r), cz = sp_axis(z, G.o[2], G.inv[2], G.g[2], r);
        vcell[v] = (cx * G.g[1] + cy) * G.g[2] + cz;          // < gx gy gz <= 2^30 whatever the vertex holds
        sp_count_flag(!(sp_finite(x) && sp_finite(y) && sp_finite(z)), bad_vertices);
    }
}

// set bit k of the grid's bit array; the word is looked at first (bits are only ever set: a set bit that is seen is set)
__device__ __forceinline__ void sp_mark(uint64_t *__restrict__ bits, uint32_t k) {
    const uint64_t bit = 1ull << (k & 63);
    unsigned long long *w = reinterpret_cast<unsigned long long *>(bits + (k >> 6));
    if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, (unsigned long long)bit);
}

// ---------------------------------------------------------------- count, pass 2: the triangles
// one wave per chunk of 64 triangles and pass: the chunk's ballot word leaves as one store (k_sp_words counts it). The loads of a
// triangle depend on each other (indices -> cells -> the grid's word), so the parallelism is across chunks, not inside a wave's loop.
__global__ void __launch_bounds__(256) k_sp_tri(const int32_t *__restrict__ triangles, uint32_t F, uint32_t V, uint32_t W, SpWs ws,
                                                uint32_t *__restrict__ bad_indices) {
    const uint32_t lane = threadIdx.x & 63;
    for (uint32_t ch = blockIdx.x * 4 + (threadIdx.x >> 6); ch < W; ch += gridDim.x * 4) {        // wave-uniform
        const uint32_t f = ch * 64u + lane;
        const bool valid = f < F;
        const int32_t *t = triangles + (uint64_t)min(f, F - 1u) * 3;
        const uint32_t a = (uint32_t)t[0], b = (uint32_t)t[1], c = (uint32_t)t[2];      // a negative index reads as >= 2^31 > V
        const bool inr = valid && a < V && b < V && c < V;
        uint32_t ka = 0, kb = 0, kc = 0;
        if (inr) { ka = ws.vcell[a]; kb = ws.vcell[b]; kc = ws.vcell[c]; }
        const bool sv = inr && ka != kb && kb != kc && ka != kc;
        if (sv) { sp_mark(ws.bits, ka); sp_mark(ws.bits, kb); sp_mark(ws.bits, kc); }
        sp_count_flag(valid && !inr, bad_indices);
        const uint64_t bt = __ballot(sv);
        if (lane == 0) ws.tmask[ch] = bt;
    }
}

// ---------------------------------------------------------------- count, pass 3: popcounts of the cell words or of the triangle words
// one wave per group of MS_GROUP words: per-word exclusive offsets inside the group, and the group's total
__global__ void __launch_bounds__(256) k_sp_words(const uint64_t *__restrict__ words, uint32_t W, uint32_t n_groups, uint32_t *__restrict__ offsets,
                                                  uint32_t *__restrict__ group_total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (g >= n_groups) return;
    const uint32_t c = g * MS_GROUP + lane;
    const int cnt = c < W ? __popcll(words[c]) : 0;
    const int incl = wave_incl_sum_i(cnt, (int)lane);
    if (c < W) offsets[c] = (uint32_t)(incl - cnt);
    if (lane == 63) group_total[g] = (uint32_t)incl;
}

// ---------------------------------------------------------------- emit
// the accumulators of foc_simplify_emit, Vc entries each: int64 sums (coordinates, then normals, then colours), the member count, and
// 0xFFFFFFFF - (smallest member index) so that a zeroed buffer is the empty state of an atomicMax
struct SpAcc { unsigned long long *pos, *nrm, *col; uint32_t *count, *first; };

template <bool NORMALS, bool COLORS>
__global__ void __launch_bounds__(256) k_sp_accum(const float *__restrict__ vertices, const float *__restrict__ normals, const float *__restrict__ colors, uint32_t V,
                                                  SpGrid G, SpWs ws, SpAcc A, uint32_t Vc, int32_t *__restrict__ vertex_map) {
    const uint32_t kept = min(Vc, ws.totals[0]);
    for (uint32_t v = blockIdx.x * 256 + threadIdx.x; v < V; v += gridDim.x * 256) {
        const uint32_t k = ws.vcell[v], l = k & 63;
        const uint64_t w = ws.bits[k >> 6];
        const uint32_t id = ws.coff[k >> 6] + (uint32_t)__popcll(w & ((1ull << l) - 1ull));
        if (!((w >> l) & 1ull) || id >= kept) { vertex_map[v] = -1; continue; }
        vertex_map[v] = (int32_t)id;
        const float *p = vertices + (uint64_t)v * 3;
#pragma unroll
        for (uint32_t a = 0; a < 3; a++) {
            float r;
            sp_axis(p[a], G.o[a], G.inv[a], G.g[a], r);
            atomicAdd(A.pos + (uint64_t)a * Vc + id, sp_fixed(r));
        }
        if (NORMALS) {
            const float *n = normals + (uint64_t)v * 3;
#pragma unroll
            for (uint32_t a = 0; a < 3; a++) {
                const float x = n[a];
                atomicAdd(A.nrm + (uint64_t)a * Vc + id, sp_fixed(sp_finite(x) ? fminf(fmaxf(x, -1.0f), 1.0f) : 0.0f));
            }
        }
        if (COLORS) {
            const float *c = colors + (uint64_t)v * 3;
#pragma unroll
            for (uint32_t a = 0; a < 3; a++) {
                const float x = c[a];
                atomicAdd(A.col + (uint64_t)a * Vc + id, sp_fixed(x != x ? 0.0f : fminf(fmaxf(x, 0.0f), 1.0f)));
            }
        }
        atomicAdd(A.count + id, 1u);
        atomicMax(A.first + id, 0xFFFFFFFFu - v);
    }
}

__device__ __forceinline__ double sp_mean(unsigned long long S, double count) {
    return __ddiv_rn(__ddiv_rn((double)(long long)S, count), 1073741824.0);
}

template <bool NORMALS, bool COLORS>
__global__ void __launch_bounds__(256) k_sp_cells(const int32_t *__restrict__ object_id, uint32_t V, SpGrid G, SpWs ws, SpAcc A, uint32_t Vc,
                                                  float *__restrict__ out_vertices, float *__restrict__ out_normals, float *__restrict__ out_colors,
                                                  int32_t *__restrict__ out_object_id, int32_t *__restrict__ members) {
    const uint32_t kept = min(Vc, ws.totals[0]);
    for (uint32_t j = blockIdx.x * 256 + threadIdx.x; j < kept; j += gridDim.x * 256) {
        const uint32_t cnt = A.count[j], first = 0xFFFFFFFFu - A.first[j];
        const bool some = cnt > 0 && first < V;                // always, for a kept cell: a surviving triangle's corner lies in it
        const uint32_t k = some ? ws.vcell[first] : 0u;
        const uint32_t c[3] = {k / (G.g[1] * G.g[2]), (k / G.g[2]) % G.g[1], k % G.g[2]};
        const double n = (double)cnt;
        members[j] = (int32_t)cnt;
#pragma unroll
        for (uint32_t a = 0; a < 3; a++) {
            const double m = sp_mean(A.pos[(uint64_t)a * Vc + j], n);
            out_vertices[(uint64_t)j * 3 + a] = some ? (float)__dadd_rn(G.od[a], __dmul_rn(__dadd_rn((double)c[a], m), G.celld[a])) : 0.0f;
        }
        if (NORMALS) {
            const double sx = (double)(long long)A.nrm[j], sy = (double)(long long)A.nrm[(uint64_t)Vc + j], sz = (double)(long long)A.nrm[2ull * Vc + j];
            const double len = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(sx, sx), __dmul_rn(sy, sy)), __dmul_rn(sz, sz)));
            float *o = out_normals + (uint64_t)j * 3;
            o[0] = len > 0 ? (float)__ddiv_rn(sx, len) : 0.0f; o[1] = len > 0 ? (float)__ddiv_rn(sy, len) : 0.0f; o[2] = len > 0 ? (float)__ddiv_rn(sz, len) : 0.0f;
        }
        if (COLORS) {
#pragma unroll
            for (uint32_t a = 0; a < 3; a++) out_colors[(uint64_t)j * 3 + a] = some ? (float)sp_mean(A.col[(uint64_t)a * Vc + j], n) : 0.0f;
        }
        if (out_object_id) out_object_id[j] = some ? object_id[first] : -1;
    }
}

__global__ void __launch_bounds__(256) k_sp_triangles(const int32_t *__restrict__ triangles, uint32_t F, uint32_t V, SpWs ws, uint32_t Fc,
                                                      const int32_t *__restrict__ vertex_map, int32_t *__restrict__ out_triangles) {
    const uint32_t total = min(Fc, ws.totals[1]);
    for (uint32_t f = blockIdx.x * 256 + threadIdx.x; f < F; f += gridDim.x * 256) {
        const uint32_t ch = f >> 6, l = f & 63;
        const uint64_t m = ws.tmask[ch];
        if (!((m >> l) & 1ull)) continue;
        const uint32_t slot = ws.toff[ch] + (uint32_t)__popcll(m & ((1ull << l) - 1ull));
        if (slot >= total) continue;
        const int32_t *t = triangles + (uint64_t)f * 3;
        const uint32_t a = (uint32_t)t[0], b = (uint32_t)t[1], c = (uint32_t)t[2];
        if (!(a < V && b < V && c < V)) continue;              // a survivor's indices were checked by the count pass; checked again before the read
        const int32_t na = vertex_map[a], nb = vertex_map[b], nc = vertex_map[c];
        int32_t *o = out_triangles + (uint64_t)slot * 3;
        if (na < nb && na < nc) { o[0] = na; o[1] = nb; o[2] = nc; }
        else if (nb < nc) { o[0] = nb; o[1] = nc; o[2] = na; }
        else { o[0] = nc; o[1] = na; o[2] = nb; }
    }
}

// ---------------------------------------------------------------- host side
struct SpSizes { uint32_t Wc, Wt, Gc, Gt, G; };
static inline SpSizes sp_sizes(uint32_t F, uint64_t cells) {
    SpSizes s;
    s.Wc = ms_chunks(cells); s.Wt = ms_chunks(F);
    s.Gc = ms_groups(s.Wc); s.Gt = ms_groups(s.Wt);
    s.G = s.Gc > s.Gt ? s.Gc : s.Gt;
    return s;
}
// what the count pass zeroes stands first: the totals, the bit array, the two group-total arrays (the shorter one is padded with zeros so
// that ONE scan serves both)
static inline uint64_t sp_zeroed_bytes(const SpSizes &s) { return 16 + (uint64_t)s.Wc * 8 + (uint64_t)s.G * 8; }
static SpWs sp_ws(void *workspace, const SpSizes &s) {
    SpWs ws;
    uint8_t *p = reinterpret_cast<uint8_t *>(workspace);
    ws.totals = reinterpret_cast<uint32_t *>(p); p += 16;
    ws.bits = reinterpret_cast<uint64_t *>(p); p += (uint64_t)s.Wc * 8;
    ws.gc = reinterpret_cast<uint32_t *>(p); p += (uint64_t)s.G * 4;
    ws.gt = reinterpret_cast<uint32_t *>(p); p += (uint64_t)s.G * 4;
    ws.tmask = reinterpret_cast<uint64_t *>(p); p += (uint64_t)s.Wt * 8;
    ws.coff = reinterpret_cast<uint32_t *>(p); p += (uint64_t)s.Wc * 4;
    ws.toff = reinterpret_cast<uint32_t *>(p); p += (uint64_t)s.Wt * 4;
    ws.vcell = reinterpret_cast<uint32_t *>(p);
    return ws;
}
static uint64_t sp_ws_bytes(uint32_t V, const SpSizes &s) {
    return sp_zeroed_bytes(s) + (uint64_t)s.Wt * 12 + (uint64_t)s.Wc * 4 + (uint64_t)V * 4;
}

// the refusals every entry point shares: sizes, the grid; fills G
static bool sp_grid_ok(const char *who, uint32_t V, uint32_t F, const float *origin3, const float *cell3, uint32_t gx, uint32_t gy, uint32_t gz, SpGrid *G) {
    if (V > SP_MAX_ELEMS || F > SP_MAX_ELEMS) { foc_set_error("%s: V and F must not exceed 2^31 - 1 (got %u, %u)", who, V, F); return false; }
    if (gx < 1 || gy < 1 || gz < 1 || (uint64_t)gx * gy > SP_MAX_CELLS || (uint64_t)gx * gy * gz > SP_MAX_CELLS) {
        foc_set_error("%s: dims must be >= 1 each with gx * gy * gz <= 2^30 (got %u x %u x %u)", who, gx, gy, gz);
        return false;
    }
    if (!G) return true;
    if (!origin3 || !cell3) { foc_set_error("%s: null pointer (origin3 / cell3: 3 floats each in host memory)", who); return false; }
    const uint32_t g[3] = {gx, gy, gz};
    for (int a = 0; a < 3; a++) {
        if (!std::isfinite(origin3[a])) { foc_set_error("%s: non-finite origin3", who); return false; }
        if (!(std::isfinite(cell3[a]) && cell3[a] > 0)) { foc_set_error("%s: cell3 must be finite and > 0 (got %g)", who, (double)cell3[a]); return false; }
        const float inv = 1.0f / cell3[a];                    // one fp32 division
        if (!std::isfinite(inv)) { foc_set_error("%s: cell3 is too small: 1 / %g is not finite", who, (double)cell3[a]); return false; }
        G->o[a] = origin3[a]; G->inv[a] = inv; G->od[a] = (double)origin3[a]; G->celld[a] = (double)cell3[a]; G->g[a] = g[a];
    }
    return true;
}

extern "C" {

uint64_t foc_simplify_workspace_bytes(uint32_t V, uint32_t F, uint32_t gx, uint32_t gy, uint32_t gz) {
    if (!sp_grid_ok("simplify_workspace_bytes", V, F, nullptr, nullptr, gx, gy, gz, nullptr)) return 0;
    return sp_ws_bytes(V, sp_sizes(F, (uint64_t)gx * gy * gz));
}

uint64_t foc_simplify_accum_bytes(uint32_t Vc, int normals, int colors) {
    return (uint64_t)Vc * (8 * (3 + (normals ? 3 : 0) + (colors ? 3 : 0)) + 8);
}

int foc_simplify_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t F, const float *origin3, const float *cell3, uint32_t gx,
                       uint32_t gy, uint32_t gz, void *workspace, uint64_t workspace_bytes, uint32_t *counts4, void *stream) {
    FocDeviceGuard foc_guard_(stream, workspace);
    FOC_REQUIRE(workspace && counts4 && (vertices || V == 0) && (triangles || F == 0), FOC_E_INVALID, "simplify_count: null pointer");
    SpGrid G;
    if (!sp_grid_ok("simplify_count", V, F, origin3, cell3, gx, gy, gz, &G)) return FOC_E_INVALID;
    const SpSizes s = sp_sizes(F, (uint64_t)gx * gy * gz);
    FOC_REQUIRE(workspace_bytes >= sp_ws_bytes(V, s), FOC_E_INVALID, "simplify_count: workspace of %llu bytes, foc_simplify_workspace_bytes asks for %llu",
                (unsigned long long)workspace_bytes, (unsigned long long)sp_ws_bytes(V, s));
    FOC_REQUIRE((((uintptr_t)workspace) & 7) == 0 && (((uintptr_t)counts4) & 3) == 0, FOC_E_INVALID, "simplify_count: workspace must be 8-byte aligned, counts4 4-byte");
    hipStream_t st = (hipStream_t)stream;
    const SpWs ws = sp_ws(workspace, s);
    uint32_t *bad = counts4 + 2;                               // {bad vertices, bad indices}: counted in place, behind the scan's two totals
    if (foc_zero_async(workspace, sp_zeroed_bytes(s), st) != hipSuccess || foc_zero_async(counts4, 16, st) != hipSuccess) {
        foc_set_error("simplify_count: launch failed (zero)");
        return FOC_E_LAUNCH;
    }
    if (V) {
        hipLaunchKernelGGL(k_sp_cell, dim3(foc_grid_1d(V, 256)), dim3(256), 0, st, vertices, V, G, ws.vcell, bad);
        FOC_CHECK_LAUNCH("simplify_count");
    }
    if (F) {
        hipLaunchKernelGGL(k_sp_tri, dim3(foc_grid_1d(s.Wt, 4)), dim3(256), 0, st, triangles, F, V, s.Wt, ws, bad + 1);
        FOC_CHECK_LAUNCH("simplify_count");
        hipLaunchKernelGGL(k_sp_words, dim3(foc_div_up(s.Gt, 4)), dim3(256), 0, st, (const uint64_t *)ws.tmask, s.Wt, s.Gt, ws.toff, ws.gt);
        FOC_CHECK_LAUNCH("simplify_count");
    }
    hipLaunchKernelGGL(k_sp_words, dim3(foc_div_up(s.Gc, 4)), dim3(256), 0, st, (const uint64_t *)ws.bits, s.Wc, s.Gc, ws.coff, ws.gc);
    FOC_CHECK_LAUNCH("simplify_count");
    hipLaunchKernelGGL(k_ms_scan, dim3(1), dim3(1024), 0, st, ws.gc, ws.gt, (const uint32_t *)nullptr, s.G, ws.totals, counts4, 2u);
    FOC_CHECK_LAUNCH("simplify_count");
    hipLaunchKernelGGL(k_ms_finish, dim3(foc_grid_1d(s.Wc, 256)), dim3(256), 0, st, ws.gc, ws.coff, (const uint32_t *)nullptr, (uint32_t *)nullptr, s.Wc);
    FOC_CHECK_LAUNCH("simplify_count");
    if (s.Wt) {
        hipLaunchKernelGGL(k_ms_finish, dim3(foc_grid_1d(s.Wt, 256)), dim3(256), 0, st, ws.gt, ws.toff, (const uint32_t *)nullptr, (uint32_t *)nullptr, s.Wt);
        FOC_CHECK_LAUNCH("simplify_count");
    }
    return FOC_OK;
}

int foc_simplify_emit(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t F, const float *normals, const float *colors,
                      const int32_t *object_id, const float *origin3, const float *cell3, uint32_t gx, uint32_t gy, uint32_t gz, const void *workspace,
                      void *accum, uint64_t accum_bytes, uint32_t Vc, uint32_t Fc, float *out_vertices, float *out_normals, float *out_colors,
                      int32_t *out_object_id, int32_t *vertex_map, int32_t *members, int32_t *out_triangles, void *stream) {
    FocDeviceGuard foc_guard_(stream, workspace);
    FOC_REQUIRE(workspace && vertices && triangles && accum && out_vertices && vertex_map && members && out_triangles, FOC_E_INVALID, "simplify_emit: null pointer");
    FOC_REQUIRE((normals == nullptr) == (out_normals == nullptr) && (colors == nullptr) == (out_colors == nullptr) &&
                (object_id == nullptr) == (out_object_id == nullptr), FOC_E_INVALID,
                "simplify_emit: normals / out_normals, colors / out_colors and object_id / out_object_id come in pairs");
    SpGrid G;
    if (!sp_grid_ok("simplify_emit", V, F, origin3, cell3, gx, gy, gz, &G)) return FOC_E_INVALID;
    FOC_REQUIRE(V >= 1 && F >= 1 && Vc >= 1 && Fc >= 1 && Vc <= V && Fc <= F, FOC_E_INVALID,
                "simplify_emit: 1 <= Vc <= V and 1 <= Fc <= F expected (got Vc %u, V %u, Fc %u, F %u); an empty result needs no emit", Vc, V, Fc, F);
    const uint64_t need = foc_simplify_accum_bytes(Vc, normals != nullptr, colors != nullptr);
    FOC_REQUIRE(accum_bytes >= need, FOC_E_INVALID, "simplify_emit: accum of %llu bytes, foc_simplify_accum_bytes asks for %llu", (unsigned long long)accum_bytes,
                (unsigned long long)need);
    FOC_REQUIRE(((((uintptr_t)workspace) | ((uintptr_t)accum)) & 7) == 0, FOC_E_INVALID, "simplify_emit: workspace and accum must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const SpWs ws = sp_ws(const_cast<void *>(workspace), sp_sizes(F, (uint64_t)gx * gy * gz));
    SpAcc A;
    unsigned long long *q = reinterpret_cast<unsigned long long *>(accum);
    A.pos = q; q += 3ull * Vc;
    A.nrm = normals ? q : nullptr; q += normals ? 3ull * Vc : 0;
    A.col = colors ? q : nullptr; q += colors ? 3ull * Vc : 0;
    A.count = reinterpret_cast<uint32_t *>(q); A.first = A.count + Vc;
    if (foc_zero_async(accum, need, st) != hipSuccess) { foc_set_error("simplify_emit: launch failed (zero)"); return FOC_E_LAUNCH; }
    const dim3 gv(foc_grid_1d(V, 256)), gk(foc_grid_1d(Vc, 256)), block(256);
#define SP_LAUNCH(N, C)                                                                                                                                        \
    do {                                                                                                                                                       \
        hipLaunchKernelGGL((k_sp_accum<N, C>), gv, block, 0, st, vertices, normals, colors, V, G, ws, A, Vc, vertex_map);                                       \
        FOC_CHECK_LAUNCH("simplify_emit");                                                                                                                     \
        hipLaunchKernelGGL((k_sp_cells<N, C>), gk, block, 0, st, object_id, V, G, ws, A, Vc, out_vertices, out_normals, out_colors, out_object_id, members);    \
        FOC_CHECK_LAUNCH("simplify_emit");                                                                                                                     \
    } while (0)
    if (normals && colors) SP_LAUNCH(true, true);
    else if (normals) SP_LAUNCH(true, false);
    else if (colors) SP_LAUNCH(false, true);
    else SP_LAUNCH(false, false);
#undef SP_LAUNCH
    hipLaunchKernelGGL(k_sp_triangles, dim3(foc_grid_1d(F, 256)), block, 0, st, triangles, F, V, ws, Fc, vertex_map, out_triangles);
    FOC_CHECK_LAUNCH("simplify_emit");
    return FOC_OK;
}

} // extern "C"
