// combine.hip — multi-object combine (COMBINED.py:247-251, 141-200) and library bookkeeping.
//
// foc_combine_select      : per-sample strict-'>' max-density select (first object wins ties).
// foc_combine_pack_keys / foc_combine_unpack : the same select expressed as an order-preserving
//   64-bit key, so K objects living on K GPUs can be merged with ONE RCCL all-reduce(MAX) of the
//   keys plus one all-reduce(SUM) of rgb masked to the winning rank (exactly one non-zero
//   contributor per sample -> bit-exact).
// foc_composite_fixed_steps : the fixed-step alpha composite the reference writes with
//   torch.cumprod (COMBINED.py:141-200 / nerf/renderer.py:169-221), one wave per ray with a
//   wave product-scan over 64 samples at a time.
// foc_combine_select_composite{,_attr} : select + composite (+ attribution) fused over K objects' dense packed fields;
// foc_combine_select_composite_culled  : the same fed from the objects' compact culled lists (fixedcull.hip), no dense field.
#include "common.h"
#include "fs_common.h"        // fs_geom, fs_sample, fs_trans_scan: the fixed-step sample step of fixedstep.hip
#include <string.h>
#include <cmath>

// ---------------------------------------------------------------- error plumbing
static thread_local char g_err[512] = "";

void foc_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// ---------------------------------------------------------------- kernels
__global__ void __launch_bounds__(256) k_combine_select(const float *__restrict__ dens, const float *__restrict__ rgb,
                                                        float *__restrict__ max_dens, float *__restrict__ best_rgb, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const float d = dens[i], m = max_dens[i];
        if (d > m) { best_rgb[i * 3] = rgb[i * 3]; best_rgb[i * 3 + 1] = rgb[i * 3 + 1]; best_rgb[i * 3 + 2] = rgb[i * 3 + 2]; }
        // torch.maximum propagates NaN
        max_dens[i] = (d != d || m != m) ? __builtin_nanf("") : (d > m ? d : m);
    }
}

__global__ void __launch_bounds__(256) k_combine_pack(const float *__restrict__ dens, uint32_t rank, uint64_t *__restrict__ keys, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        float d = dens[i];
        d = d > 0.0f ? d : 0.0f;                       // sigma >= 0 (trunc_exp): bit pattern is order preserving; -0/NaN -> 0
        keys[i] = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)(0xFFFFFFFFu - rank);
    }
}

__global__ void __launch_bounds__(256) k_combine_unpack(const uint64_t *__restrict__ keys, uint32_t rank, const float *__restrict__ rgb,
                                                        float *__restrict__ max_dens, float *__restrict__ masked_rgb, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const uint64_t k = keys[i];
        const bool mine = (uint32_t)(k & 0xFFFFFFFFu) == 0xFFFFFFFFu - rank;
        max_dens[i] = __uint_as_float((uint32_t)(k >> 32));
        masked_rgb[i * 3] = mine ? rgb[i * 3] : 0.0f;
        masked_rgb[i * 3 + 1] = mine ? rgb[i * 3 + 1] : 0.0f;
        masked_rgb[i * 3 + 2] = mine ? rgb[i * 3 + 2] : 0.0f;
    }
}

// One wave per ray. z_i, deltas = diff(z) with last = (far-near)/T and the depth's oz: fs_common.h fs_sample without noise;
// w_i = alpha_i * prod_{j<i}(1 - alpha_j + 1e-15) (fs_trans_scan). alpha is this file's own rounding: 1 - __expf(-delta * sigma).
__global__ void __launch_bounds__(256) k_composite_fixed(const float *__restrict__ sigmas, const float *__restrict__ rgbs,
                                                         const float *__restrict__ nears, const float *__restrict__ fars,
                                                         uint32_t N, uint32_t T, float bg, float *__restrict__ image4, float *__restrict__ depth) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const FsGeom geo = fs_geom(nears, fars, n, T);
    float Tc = 1.0f, r = 0, g = 0, b = 0, a = 0, d = 0, ws = 0;
    for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < T;
        float alpha = 0, sigma = 0, c0 = 0, c1 = 0, c2 = 0, oz = 0;
        if (valid) {
            const FsSample p = fs_sample(geo, i, i, T, false, 0.0f, 0.0f);
            const uint64_t s = (uint64_t)n * T + i;
            sigma = sigmas[s];
            c0 = rgbs[s * 3]; c1 = rgbs[s * 3 + 1]; c2 = rgbs[s * 3 + 2];
            alpha = 1 - __expf(-p.delta * sigma);
            oz = p.oz;
        }
        const float om = valid ? (1 - alpha + 1e-15f) : 1.0f;
        const float w = alpha * fs_trans_scan(om, lane, Tc);
        r = fmaf(w, c0, r); g = fmaf(w, c1, g); b = fmaf(w, c2, b);
        a = fmaf(w, sigma, a); d = fmaf(w, oz, d); ws += w;
    }
    r = wave_sum(r); g = wave_sum(g); b = wave_sum(b); a = wave_sum(a); d = wave_sum(d); ws = wave_sum(ws);
    if (lane == 0) {
        const float rest = (1 - ws) * bg;
        float o[4] = {r + rest, g + rest, b + rest, a + rest};
#pragma unroll
        for (int k = 0; k < 4; k++) image4[(uint64_t)n * 4 + k] = fminf(1.0f, fmaxf(0.0f, o[k]));
        depth[n] = d;
    }
}

// ---------------------------------------------------------------- fused select + composite over K objects' packed fields
// fields.p[k] -> object k's field4 [N,T] (sigma, r, g, b) on the SAME rays and sample positions, k in checkpoint order. One wave per
// ray, 64 samples at a time: every lane reads its sample of each object with one 16-byte load, keeps the entry with the strictly larger
// density (object 0 first, `d > max` for the others: COMBINED.py:247-251, torch.maximum's NaN propagation included) and the composite of
// image_depth_generation (:141-200) runs on the merged values without the merged field ever being stored: 16 B read per sample and
// object, 20 B written per ray and background. n_bg backgrounds (the reference composites every view twice, white and black,
// compute_metrics_both_backgrounds): image4 [n_bg,N,4]. merged4 (optional) [N,T] receives (max density, best rgb) for callers that
// keep the reference's max_densities / max_rgbs.
struct CombineFields { const float4 *p[FOC_COMBINE_MAX_OBJECTS]; };

// Attribution (foc_combine_select_composite_attr): who supplied the surviving sample. Field k carries a constant object id, or a uint8
// [N,T] plane when it is itself a pre-merge of several objects (k_combine_select4_ids).
struct CombineAttr {
    const uint8_t *plane[FOC_COMBINE_MAX_OBJECTS];     // nullptr: the constant id[k]
    uint32_t id[FOC_COMBINE_MAX_OBJECTS];
    uint32_t n_obj;
    float *obj_weights, *obj_depth;                    // [N, n_obj]
    int32_t *instance;                                 // [N]
    uint8_t *winner;                                   // [N,T] or nullptr
};

// The statements of the fused select + composite, written once for the kernels that read dense packed fields (below) and the one that forms
// its entries from the compact culled lists (k_combine_culled). NOBJ == 0: select + composite, nothing else (every attribution statement
// is compiled out and `at` is never read). NOBJ = 4 / 8 / 16 >= n_obj: the winner id travels with the rgb through the select — replaced by
// the very comparison that replaces the rgb — and each lane keeps NOBJ weight and NOBJ depth accumulators updated with compare-selects; the
// loops over objects are bounded by the template argument, so the accumulators are registers (an array indexed by the winner itself would
// live in scratch memory). The composite's own arithmetic is the same statements in the same order: image4 / depth / merged4 are bit for
// bit those of NOBJ == 0.
template <int NOBJ>
struct CombineAcc {
    float Tc, r, g, b, a, d, ws;
    float aw[NOBJ > 0 ? NOBJ : 1], ad[NOBJ > 0 ? NOBJ : 1];
};
template <int NOBJ>
__device__ __forceinline__ void combine_acc_init(CombineAcc<NOBJ> &A) {
    A.Tc = 1.0f; A.r = A.g = A.b = A.a = A.d = A.ws = 0.0f;
#pragma unroll
    for (int k = 0; k < (NOBJ > 0 ? NOBJ : 1); k++) A.aw[k] = A.ad[k] = 0.0f;
}

// the select: a later object's entry f (its id: idk) against the running best
template <int NOBJ>
__device__ __forceinline__ void combine_select_step(float4 &best, uint32_t &win, const float4 f, uint32_t idk) {
    const float m = best.x;
    if constexpr (NOBJ > 0) {
        if (f.x > m) win = idk;
    }
    if (f.x > m) { best.y = f.y; best.z = f.z; best.w = f.w; }
    best.x = (f.x != f.x || m != m) ? __builtin_nanf("") : (f.x > m ? f.x : m);      // torch.maximum propagates NaN
}

// what a lane's sample gives the composite; a lane past T holds no sample: all zero, no column
struct CombineSample { float alpha, sigma, c0, c1, c2, oz; uint32_t win; };
__device__ __forceinline__ CombineSample combine_no_sample() { return CombineSample{0, 0, 0, 0, 0, 0, 0xFFu}; }

// the per-sample outputs of a lane that holds sample s
template <int NOBJ>
__device__ __forceinline__ void combine_store(const float4 best, uint32_t win, uint64_t s, float4 *__restrict__ merged4, const CombineAttr *at) {
    if (merged4) merged4[s] = best;
    if constexpr (NOBJ > 0) {
        if (at->winner) at->winner[s] = (uint8_t)win;
    }
}
// ... and its merged entry as the composite takes it (p: the sample's FsSample)
__device__ __forceinline__ CombineSample combine_take(const float4 best, uint32_t win, const FsSample &p) {
    CombineSample q;
    q.sigma = best.x; q.c0 = best.y; q.c1 = best.z; q.c2 = best.w;
    q.alpha = 1 - __expf(-p.delta * q.sigma);
    q.oz = p.oz;
    q.win = win;
    return q;
}

// one 64-sample step of the composite on the merged samples
template <int NOBJ>
__device__ __forceinline__ void combine_accumulate(CombineAcc<NOBJ> &A, const CombineSample &q, bool valid, uint32_t lane) {
    const float om = valid ? (1 - q.alpha + 1e-15f) : 1.0f;
    const float w = q.alpha * fs_trans_scan(om, lane, A.Tc);
    A.r = fmaf(w, q.c0, A.r); A.g = fmaf(w, q.c1, A.g); A.b = fmaf(w, q.c2, A.b);
    A.a = fmaf(w, q.sigma, A.a); A.d = fmaf(w, q.oz, A.d); A.ws += w;
    if constexpr (NOBJ > 0) {
#pragma unroll
        for (int k = 0; k < NOBJ; k++) {                                         // the statements of `ws` and `d`, kept by the winner's column only
            const bool mine = q.win == (uint32_t)k;
            A.aw[k] = mine ? A.aw[k] + w : A.aw[k];
            A.ad[k] = mine ? fmaf(w, q.oz, A.ad[k]) : A.ad[k];
        }
    }
}

// the ray's sums, backgrounds and clamp
template <int NOBJ>
__device__ __forceinline__ void combine_finish(CombineAcc<NOBJ> &A, const CombineAttr *at, uint32_t n, uint32_t N, uint32_t lane, float bg0, float bg1,
                                               uint32_t n_bg, float *__restrict__ image4, float *__restrict__ depth) {
    const float r = wave_sum(A.r), g = wave_sum(A.g), b = wave_sum(A.b), a = wave_sum(A.a), d = wave_sum(A.d), ws = wave_sum(A.ws);
    if constexpr (NOBJ > 0) {
        // one fixed tree per used column (no atomics: run-to-run bit-stable); every lane ends up with every sum, lane k stores column k
        const uint32_t n_obj = at->n_obj;
        float my_w = 0.0f, my_d = 0.0f, top = 0.0f;
        int32_t inst = -1;
#pragma unroll
        for (int k = 0; k < NOBJ; k++) {
            if ((uint32_t)k < n_obj) {                                           // wave-uniform
                const float sw = wave_sum(A.aw[k]), sd = wave_sum(A.ad[k]);
                if (lane == (uint32_t)k) { my_w = sw; my_d = sd; }
                if (sw > top) { top = sw; inst = k; }                            // strict: the first of equal columns; NaN and 0 never
            }
        }
        if (lane < n_obj) {
            at->obj_weights[(uint64_t)n * n_obj + lane] = my_w;
            at->obj_depth[(uint64_t)n * n_obj + lane] = my_d;
        }
        if (lane == 0) at->instance[n] = inst;
    }
    if (lane == 0) {
        for (uint32_t q = 0; q < n_bg; q++) {
            const float rest = (1 - ws) * (q == 0 ? bg0 : bg1);
            const float o[4] = {r + rest, g + rest, b + rest, a + rest};
#pragma unroll
            for (int k = 0; k < 4; k++) image4[((uint64_t)q * N + n) * 4 + k] = fminf(1.0f, fmaxf(0.0f, o[k]));
        }
        depth[n] = d;
    }
}

// The body of both dense kernels: every lane reads its sample of each object's field4.
template <int NOBJ>
__device__ __forceinline__ void combine_select_composite_body(const CombineFields &fields, const CombineAttr *at, uint32_t K,
                                                              const float *__restrict__ nears, const float *__restrict__ fars, uint32_t N,
                                                              uint32_t T, float bg0, float bg1, uint32_t n_bg, float *__restrict__ image4,
                                                              float *__restrict__ depth, float4 *__restrict__ merged4) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const FsGeom geo = fs_geom(nears, fars, n, T);
    CombineAcc<NOBJ> A;
    combine_acc_init(A);
    for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < T;
        CombineSample q = combine_no_sample();
        if (valid) {
            const uint64_t s = (uint64_t)n * T + i;
            float4 best = fields.p[0][s];
            uint32_t win = 0xFFu;
            if constexpr (NOBJ > 0) win = at->plane[0] ? (uint32_t)at->plane[0][s] : at->id[0];
            for (uint32_t k = 1; k < K; k++) {
                const float4 f = fields.p[k][s];
                uint32_t idk = 0;
                if constexpr (NOBJ > 0) idk = at->plane[k] ? (uint32_t)at->plane[k][s] : at->id[k];
                combine_select_step<NOBJ>(best, win, f, idk);
            }
            combine_store<NOBJ>(best, win, s, merged4, at);
            q = combine_take(best, win, fs_sample(geo, i, i, T, false, 0.0f, 0.0f));
        }
        combine_accumulate(A, q, valid, lane);
    }
    combine_finish(A, at, n, N, lane, bg0, bg1, n_bg, image4, depth);
}

__global__ void __launch_bounds__(256) k_combine_select_composite(CombineFields fields, uint32_t K, const float *__restrict__ nears,
                                                                  const float *__restrict__ fars, uint32_t N, uint32_t T, float bg0, float bg1,
                                                                  uint32_t n_bg, float *__restrict__ image4, float *__restrict__ depth,
                                                                  float4 *__restrict__ merged4) {
    combine_select_composite_body<0>(fields, nullptr, K, nears, fars, N, T, bg0, bg1, n_bg, image4, depth, merged4);
}

template <int NOBJ>
__global__ void __launch_bounds__(256) k_combine_select_composite_attr(CombineFields fields, CombineAttr at, uint32_t K,
                                                                       const float *__restrict__ nears, const float *__restrict__ fars, uint32_t N,
                                                                       uint32_t T, float bg0, float bg1, uint32_t n_bg, float *__restrict__ image4,
                                                                       float *__restrict__ depth, float4 *__restrict__ merged4) {
    combine_select_composite_body<NOBJ>(fields, &at, K, nears, fars, N, T, bg0, bg1, n_bg, image4, depth, merged4);
}

// ---------------------------------------------------------------- the same select + composite fed from K objects' compact culled lists
// include/focnerf.h foc_combine_select_composite_culled. Object k arrives as foc_fixed_cull{,_placed} and the field kernels left it: the row
// masks, their offsets and the compact sigma / rgb. One wave per ray, sample i on the lane, as k_fc_pack and the body above: the wave forms
// object k's entry with the pack's statements (fs_common.h fs_infer_weight on the object's own transmittance carry Tk[k], the rgb masked
// by w > thresh), feeds it to combine_select_step and composites: no field4 [N,T,4] exists. KMAX >= K bounds the loops over objects, so
// the carries and the lanes' slots are registers. The objects travel by value in the kernel argument block (48 bytes each).
struct CulledObj {
    const uint64_t *mask; const uint32_t *offsets; const float *sigma_c, *rgb_c;
    uint32_t m_occ; float density_scale, thresh, sigma_gain;
};
template <int KMAX> struct CulledObjs { CulledObj o[KMAX]; };

#define CC_NO_BIT 0xFFFFFFFFu
template <int KMAX, int NOBJ>
__global__ void __launch_bounds__(256) k_combine_culled(CulledObjs<KMAX> objs, CombineAttr at, uint32_t K, const float *__restrict__ nears,
                                                        const float *__restrict__ fars, uint32_t N, uint32_t T, float bg0, float bg1, uint32_t n_bg,
                                                        float *__restrict__ image4, float *__restrict__ depth, float4 *__restrict__ merged4) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t n = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (n >= N) return;
    const FsGeom geo = fs_geom(nears, fars, n, T);
    const uint32_t bit = n % FS_RAY_BLOCK;
    const uint64_t below = (1ull << bit) - 1ull;
    const uint64_t row0 = (uint64_t)(n / FS_RAY_BLOCK) * T;
    CombineAcc<NOBJ> A;
    combine_acc_init(A);
    float Tk[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) Tk[k] = 1.0f;
    for (uint32_t base = 0; base < T; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < T;
        const uint32_t ic = valid ? i : T - 1;
        const uint64_t row = row0 + ic, s = (uint64_t)n * T + ic;
        const FsSample p = fs_sample(geo, i, ic, T, false, 0.0f, 0.0f);
        // the lane's bit per object: its rank among the row's bits, or CC_NO_BIT. `plain`: an all-zero entry leaves every carry and every sum
        // of this lane as it is — alpha = 1 - exp(-0) = 0, om = 1.0f, w = 0 — which needs finite exponents' factors and an oz that is not NaN
        // (a ray that misses the box has oz = 0/0, and its depth is NaN by 0 * NaN in the dense composite too)
        uint32_t pre[KMAX];
        bool any = false, plain = fabsf(p.delta) < INFINITY && p.oz == p.oz;
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            pre[k] = CC_NO_BIT;
            if ((uint32_t)k < K) {                                               // wave-uniform
                const uint64_t m = objs.o[k].mask[row];
                if (valid && ((m >> bit) & 1ull)) { pre[k] = (uint32_t)__popcll(m & below); any = true; }
                plain = plain && fabsf(p.delta * objs.o[k].density_scale) < INFINITY;
            }
        }
        if (__ballot(any || !plain) == 0 && fabsf(A.Tc) < INFINITY) {            // no object has a bit for this ray in the tile: nothing changes
            if (valid) {
                uint32_t win = 0xFFu;
                if constexpr (NOBJ > 0) win = at.id[0];
                combine_store<NOBJ>(make_float4(0.0f, 0.0f, 0.0f, 0.0f), win, s, merged4, &at);
            }
            continue;
        }
        float4 best = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint32_t win = 0xFFu;
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            if ((uint32_t)k < K) {
                const CulledObj &o = objs.o[k];
                float sigma = 0, c0 = 0, c1 = 0, c2 = 0;
                if (pre[k] != CC_NO_BIT) {
                    const uint32_t slot = o.offsets[row] + pre[k];
                    if (slot < o.m_occ) {
                        sigma = o.sigma_c[slot];
                        if (o.sigma_gain != 1.0f) sigma *= o.sigma_gain;         // a placed object's density in world units, in front of the weights
                        c0 = o.rgb_c[(uint64_t)slot * 3]; c1 = o.rgb_c[(uint64_t)slot * 3 + 1]; c2 = o.rgb_c[(uint64_t)slot * 3 + 2];
                    }
                }
                const bool on = fs_infer_weight(Tk[k], p, valid, sigma, o.density_scale, lane) > o.thresh;
                const float4 f = make_float4(sigma, on ? c0 : 0.0f, on ? c1 : 0.0f, on ? c2 : 0.0f);
                if (k == 0) {
                    best = f;
                    if constexpr (NOBJ > 0) win = at.id[0];
                } else {
                    combine_select_step<NOBJ>(best, win, f, at.id[k]);
                }
            }
        }
        CombineSample q = combine_no_sample();
        if (valid) {
            combine_store<NOBJ>(best, win, s, merged4, &at);
            q = combine_take(best, win, p);
        }
        combine_accumulate(A, q, valid, lane);
    }
    combine_finish(A, &at, n, N, lane, bg0, bg1, n_bg, image4, depth);
}

struct CulledLaunch {
    const FocCulledField *objs; uint32_t K; CombineAttr at; const float *nears, *fars; uint32_t N, T; float bg0, bg1; uint32_t n_bg;
    float *image4, *depth; float4 *merged4; hipStream_t stream;
};
template <int KMAX, int NOBJ>
static void cc_launch(const CulledLaunch &L) {
    CulledObjs<KMAX> o;
    memset(&o, 0, sizeof(o));
    for (uint32_t k = 0; k < L.K; k++) {
        const FocCulledField &f = L.objs[k];
        o.o[k] = CulledObj{f.mask, f.offsets, f.sigma_c, f.rgb_c, f.m_occ, f.density_scale, f.thresh, f.sigma_gain};
    }
    hipLaunchKernelGGL((k_combine_culled<KMAX, NOBJ>), dim3(foc_div_up(L.N, 4)), dim3(256), 0, L.stream, o, L.at, L.K, L.nears, L.fars, L.N, L.T, L.bg0,
                       L.bg1, L.n_bg, L.image4, L.depth, L.merged4);
}
template <int KMAX>
static void cc_launch_k(const CulledLaunch &L, uint32_t n_obj) {
    if (n_obj == 0) cc_launch<KMAX, 0>(L);
    else if (n_obj <= 4) cc_launch<KMAX, 4>(L);
    else if (n_obj <= 8) cc_launch<KMAX, 8>(L);
    else cc_launch<KMAX, 16>(L);
}

// Pre-merge of the objects that share a rank before the exchange (K objects on fewer GPUs): acc4 <- select(acc4, f4), same rule. The
// select is associative over the object order, so merging a rank's consecutive objects first and the ranks afterwards equals the
// reference's one sequential pass.
__global__ void __launch_bounds__(256) k_combine_select4(const float4 *__restrict__ f4, float4 *__restrict__ acc4, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const float4 f = f4[i];
        float4 best = acc4[i];
        const float m = best.x;
        if (f.x > m) { best.y = f.y; best.z = f.z; best.w = f.w; }
        best.x = (f.x != f.x || m != m) ? __builtin_nanf("") : (f.x > m ? f.x : m);
        acc4[i] = best;
    }
}

// The same pre-merge when the view's attribution is asked for: acc_ids [n] holds, per sample, the id of the object whose rgb acc4 holds (the
// caller fills it with the first object's id); the incoming field is ONE object, and the plane takes its id exactly where the rgb is taken.
__global__ void __launch_bounds__(256) k_combine_select4_ids(const float4 *__restrict__ f4, uint8_t id, float4 *__restrict__ acc4,
                                                             uint8_t *__restrict__ acc_ids, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
        const float4 f = f4[i];
        float4 best = acc4[i];
        const float m = best.x;
        if (f.x > m) { best.y = f.y; best.z = f.z; best.w = f.w; acc_ids[i] = id; }
        best.x = (f.x != f.x || m != m) ? __builtin_nanf("") : (f.x > m ? f.x : m);
        acc4[i] = best;
    }
}

// MONeRFNetwork's running select (nerf/multiobjectnetwork.py:66-82): torch.max over stack([new, best]) and take_along_dim of the rows that
// travel with the density (geo_feat [n,15] or colour [n,3]). torch.max returns the FIRST maximal index and treats NaN as maximal, and the
// new object is stacked first: the new object wins ties (the opposite of COMBINED.py's strict '>') and a NaN density of either side stays.
// One wave per 64 samples: the lanes decide their sample, the ballot is the row mask, and the wave copies the 64 x width elements of the
// taken rows as one contiguous run (rows are 30 or 6 bytes in fp16: no lane-per-row accesses).
template <typename T>
__global__ void __launch_bounds__(256) k_mo_select(const T *__restrict__ sig_new, const T *__restrict__ feat_new, T *__restrict__ sig_best,
                                                   T *__restrict__ feat_best, uint64_t n, uint32_t width) {
    const uint64_t s0 = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;          // wave-uniform
    if (s0 >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    bool take = false;
    if (s0 + lane < n) {
        const T a_raw = sig_new[s0 + lane];
        const float a = (float)a_raw, b = (float)sig_best[s0 + lane];
        take = (a != a) || (b == b && a >= b);
        if (take) sig_best[s0 + lane] = a_raw;
    }
    const uint64_t rows = __ballot(take);
    const uint32_t live = (uint32_t)(n - s0 < 64u ? n - s0 : 64u);
    const uint64_t base = s0 * width;
    for (uint32_t e = lane; e < live * width; e += 64u)
        if ((rows >> (e / width)) & 1ull) feat_best[base + e] = feat_new[base + e];
}

// ---------------------------------------------------------------- options (common.h FocOpt)
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <mutex>
// values are atomics and the table is filled from the environment exactly once (std::call_once): a second thread entering foc_opt() while the
// first one initialises waits for it instead of reading defaults; foc_set_option from one thread is seen by launches issued afterwards
struct FocOptionRow { const char *name; std::atomic<int> value; };
static FocOptionRow foc_option_table[FOC_OPT_COUNT] = {
    {"FOC_MLP_BWD_FUSED", 1}, {"FOC_FIELD_FWD_FUSED", 1}, {"FOC_GB_MERGE_MAX_RES", 480}, {"FOC_GB_FACTORED", 1}, {"FOC_GB_TAIL_SPLIT", 16}, {"FOC_GRID_FUSE_SMALL", 1},
    {"FOC_GRID_PAIRS", 1}, {"FOC_GRID_FAST", 1}, {"FOC_MARCH_SERIAL", -1}, {"FOC_MARCH_RAYS_ROW_MAX", 131072}, {"FOC_OCC_MARCH_FORM", -1},
    {"FOC_OCC_SAMPLE_MAJOR", 1}, {"FOC_OCC_FIELD_PIECE", 1 << 23}, {"FOC_DETERMINISTIC", 0},
};
static int foc_option_parse(int which, const char *text) {
    if (which == FOC_OPT_OCC_MARCH_FORM) {                  // the forms have names: two | row | lane | staged (or 0..3, -1 = by burst length)
        if (text[0] == 't') return 0;
        if (text[0] == 'r') return 1;
        if (text[0] == 'l') return 2;
        if (text[0] == 's') return 3;
    }
    return atoi(text);
}
static void foc_options_init() {
    static std::once_flag once;
    std::call_once(once, [] {
        for (int i = 0; i < FOC_OPT_COUNT; i++) {           // the ONE place the library reads its environment
            const char *e = getenv(foc_option_table[i].name);
            if (e && e[0]) foc_option_table[i].value.store(foc_option_parse(i, e), std::memory_order_relaxed);
        }
    });
}
int foc_opt(FocOpt which) { foc_options_init(); return foc_option_table[which].value.load(std::memory_order_relaxed); }

extern "C" {

int foc_set_option(const char *name, int value) {
    foc_options_init();
    for (int i = 0; i < FOC_OPT_COUNT; i++)
        if (name && strcmp(name, foc_option_table[i].name) == 0) { foc_option_table[i].value.store(value, std::memory_order_relaxed); return FOC_OK; }
    foc_set_error("set_option: unknown option '%s'", name ? name : "(null)");
    return FOC_E_INVALID;
}

int foc_get_option(const char *name, int *value) {
    foc_options_init();
    for (int i = 0; i < FOC_OPT_COUNT; i++)
        if (name && value && strcmp(name, foc_option_table[i].name) == 0) { *value = foc_option_table[i].value.load(std::memory_order_relaxed); return FOC_OK; }
    foc_set_error("get_option: unknown option '%s'", name ? name : "(null)");
    return FOC_E_INVALID;
}

int foc_guard_pick_device(int stream_is_null, int stream_device, int pointer_device, int current_device) {
    return foc_guard_pick(stream_is_null != 0, stream_device, pointer_device, current_device);
}


int foc_combine_select_composite(const float *const *fields4, uint32_t K, const float *nears, const float *fars, uint32_t N, uint32_t T,
                                 const float *bgs, uint32_t n_bg, float *image4, float *depth, float *merged4, void *stream) {
    FocDeviceGuard foc_guard_(stream, nears);
    FOC_REQUIRE(K >= 1 && K <= FOC_COMBINE_MAX_OBJECTS, FOC_E_INVALID, "combine_select_composite: 1 <= K <= %d objects per call (got %u)",
                FOC_COMBINE_MAX_OBJECTS, K);
    FOC_REQUIRE(n_bg >= 1 && n_bg <= 2 && bgs, FOC_E_INVALID, "combine_select_composite: one or two backgrounds");
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "combine_select_composite: T must be >= 2");
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(fields4 && nears && fars && image4 && depth, FOC_E_INVALID, "combine_select_composite: null pointer");
    CombineFields f;
    for (uint32_t k = 0; k < FOC_COMBINE_MAX_OBJECTS; k++) {
        f.p[k] = reinterpret_cast<const float4 *>(k < K ? fields4[k] : fields4[0]);
        FOC_REQUIRE(f.p[k] && ((uintptr_t)f.p[k] & 15) == 0, FOC_E_INVALID, "combine_select_composite: field %u is null or not 16-byte aligned", k);
    }
    FOC_REQUIRE(((uintptr_t)merged4 & 15) == 0, FOC_E_INVALID, "combine_select_composite: merged4 must be 16-byte aligned");
    hipLaunchKernelGGL(k_combine_select_composite, dim3(foc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream, f, K, nears, fars, N, T, bgs[0],
                       n_bg > 1 ? bgs[1] : 0.0f, n_bg, image4, depth, reinterpret_cast<float4 *>(merged4));
    FOC_CHECK_LAUNCH("combine_select_composite");
    return FOC_OK;
}

int foc_combine_select4(const float *field4, float *acc4, uint64_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, field4);
    FOC_REQUIRE(n == 0 || (field4 && acc4), FOC_E_INVALID, "combine_select4: null pointer");
    FOC_REQUIRE((((uintptr_t)field4 | (uintptr_t)acc4) & 15) == 0, FOC_E_INVALID, "combine_select4: fields must be 16-byte aligned");
    if (n == 0) return FOC_OK;
    hipLaunchKernelGGL(k_combine_select4, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(field4),
                       reinterpret_cast<float4 *>(acc4), n);
    FOC_CHECK_LAUNCH("combine_select4");
    return FOC_OK;
}

int foc_combine_select_composite_attr(const float *const *fields4, uint32_t K, const uint8_t *const *id_planes, const uint32_t *ids,
                                      uint32_t n_obj, const float *nears, const float *fars, uint32_t N, uint32_t T, const float *bgs,
                                      uint32_t n_bg, float *image4, float *depth, float *merged4, float *obj_weights, float *obj_depth,
                                      int32_t *instance, uint8_t *winner, void *stream) {
    FocDeviceGuard foc_guard_(stream, nears);
    FOC_REQUIRE(K >= 1 && K <= FOC_COMBINE_MAX_OBJECTS, FOC_E_INVALID, "combine_select_composite_attr: 1 <= K <= %d fields per call (got %u)",
                FOC_COMBINE_MAX_OBJECTS, K);
    FOC_REQUIRE(n_obj >= 1 && n_obj <= FOC_COMBINE_MAX_OBJECTS, FOC_E_INVALID, "combine_select_composite_attr: 1 <= n_obj <= %d objects (got %u)",
                FOC_COMBINE_MAX_OBJECTS, n_obj);
    FOC_REQUIRE(n_bg >= 1 && n_bg <= 2 && bgs, FOC_E_INVALID, "combine_select_composite_attr: one or two backgrounds");
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "combine_select_composite_attr: T must be >= 2");
    FOC_REQUIRE(fields4, FOC_E_INVALID, "combine_select_composite_attr: fields4 is null");
    CombineFields f;
    CombineAttr at;
    for (uint32_t k = 0; k < FOC_COMBINE_MAX_OBJECTS; k++) {
        const uint32_t j = k < K ? k : 0;
        at.plane[k] = id_planes ? id_planes[j] : nullptr;
        FOC_REQUIRE(at.plane[k] || ids, FOC_E_INVALID, "combine_select_composite_attr: field %u has neither an id plane nor a constant id (ids is null)", j);
        at.id[k] = at.plane[k] ? 0u : ids[j];
        FOC_REQUIRE(at.id[k] < n_obj, FOC_E_INVALID, "combine_select_composite_attr: ids[%u] = %u is not below n_obj = %u", j, at.id[k], n_obj);
    }
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(nears && fars && image4 && depth, FOC_E_INVALID, "combine_select_composite_attr: null pointer");
    FOC_REQUIRE(obj_weights && obj_depth && instance, FOC_E_INVALID, "combine_select_composite_attr: obj_weights, obj_depth and instance must not be null");
    for (uint32_t k = 0; k < FOC_COMBINE_MAX_OBJECTS; k++) {
        f.p[k] = reinterpret_cast<const float4 *>(k < K ? fields4[k] : fields4[0]);
        FOC_REQUIRE(f.p[k] && ((uintptr_t)f.p[k] & 15) == 0, FOC_E_INVALID, "combine_select_composite_attr: field %u is null or not 16-byte aligned", k);
    }
    FOC_REQUIRE(((uintptr_t)merged4 & 15) == 0, FOC_E_INVALID, "combine_select_composite_attr: merged4 must be 16-byte aligned");
    FOC_REQUIRE(((uintptr_t)obj_weights & 3) == 0 && ((uintptr_t)obj_depth & 3) == 0 && ((uintptr_t)instance & 3) == 0, FOC_E_INVALID,
                "combine_select_composite_attr: obj_weights, obj_depth and instance must be 4-byte aligned");
    at.n_obj = n_obj;
    at.obj_weights = obj_weights; at.obj_depth = obj_depth; at.instance = instance; at.winner = winner;
    const dim3 grid(foc_div_up(N, 4)), block(256);
    const float bg1 = n_bg > 1 ? bgs[1] : 0.0f;
    float4 *m4 = reinterpret_cast<float4 *>(merged4);
    if (n_obj <= 4)
        hipLaunchKernelGGL(k_combine_select_composite_attr<4>, grid, block, 0, (hipStream_t)stream, f, at, K, nears, fars, N, T, bgs[0], bg1, n_bg, image4, depth, m4);
    else if (n_obj <= 8)
        hipLaunchKernelGGL(k_combine_select_composite_attr<8>, grid, block, 0, (hipStream_t)stream, f, at, K, nears, fars, N, T, bgs[0], bg1, n_bg, image4, depth, m4);
    else
        hipLaunchKernelGGL(k_combine_select_composite_attr<16>, grid, block, 0, (hipStream_t)stream, f, at, K, nears, fars, N, T, bgs[0], bg1, n_bg, image4, depth, m4);
    FOC_CHECK_LAUNCH("combine_select_composite_attr");
    return FOC_OK;
}

int foc_combine_select_composite_culled(const FocCulledField *objs, uint32_t K, uint32_t struct_bytes, const uint32_t *ids, uint32_t n_obj,
                                        const float *nears, const float *fars, uint32_t N, uint32_t T, const float *bgs, uint32_t n_bg, float *image4,
                                        float *depth, float *merged4, float *obj_weights, float *obj_depth, int32_t *instance, uint8_t *winner,
                                        void *stream) {
    const char *who = "combine_select_composite_culled";
    FocDeviceGuard foc_guard_(stream, nears);
    FOC_REQUIRE(K >= 1 && K <= FOC_COMBINE_MAX_OBJECTS, FOC_E_INVALID, "%s: 1 <= K <= %d objects per call (got %u)", who, FOC_COMBINE_MAX_OBJECTS, K);
    FOC_REQUIRE(struct_bytes == sizeof(FocCulledField), FOC_E_INVALID, "%s: FocCulledField of %u bytes, this library's has %u", who, struct_bytes,
                (uint32_t)sizeof(FocCulledField));
    FOC_REQUIRE(objs, FOC_E_INVALID, "%s: objs is null", who);
    FOC_REQUIRE(n_obj <= FOC_COMBINE_MAX_OBJECTS, FOC_E_INVALID, "%s: n_obj <= %d objects (got %u)", who, FOC_COMBINE_MAX_OBJECTS, n_obj);
    FOC_REQUIRE(n_bg >= 1 && n_bg <= 2 && bgs, FOC_E_INVALID, "%s: one or two backgrounds", who);
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "%s: T must be >= 2", who);
    FOC_REQUIRE((uint64_t)foc_div_up(N, FS_RAY_BLOCK) * FS_RAY_BLOCK * T < (1ull << 31), FOC_E_INVALID,
                "%s: ceil(N/64)*64*T must stay below 2^31 (foc_fixed_cull's limit)", who);
    CulledLaunch L;
    memset(&L.at, 0, sizeof(L.at));
    for (uint32_t k = 0; k < K; k++) {
        const FocCulledField &f = objs[k];
        FOC_REQUIRE(std::isfinite(f.sigma_gain) && f.sigma_gain > 0, FOC_E_INVALID, "%s: object %u: sigma_gain must be finite and > 0 (got %g)", who, k,
                    (double)f.sigma_gain);
        L.at.id[k] = ids ? ids[k] : k;
        FOC_REQUIRE(n_obj == 0 || L.at.id[k] < n_obj, FOC_E_INVALID, "%s: ids[%u] = %u is not below n_obj = %u", who, k, L.at.id[k], n_obj);
    }
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(nears && fars && image4 && depth, FOC_E_INVALID, "%s: null pointer", who);
    FOC_REQUIRE(n_obj == 0 || (obj_weights && obj_depth && instance), FOC_E_INVALID, "%s: obj_weights, obj_depth and instance must not be null when n_obj > 0", who);
    for (uint32_t k = 0; k < K; k++) {
        const FocCulledField &f = objs[k];
        FOC_REQUIRE(f.mask && f.offsets, FOC_E_INVALID, "%s: object %u: null pointer (mask / offsets)", who, k);
        FOC_REQUIRE(f.m_occ == 0 || (f.sigma_c && f.rgb_c), FOC_E_INVALID, "%s: object %u: null sigma / rgb with %u occupied samples", who, k, f.m_occ);
        FOC_REQUIRE(((uintptr_t)f.mask & 7) == 0 && ((uintptr_t)f.offsets & 3) == 0 && ((uintptr_t)f.sigma_c & 3) == 0 && ((uintptr_t)f.rgb_c & 3) == 0,
                    FOC_E_INVALID, "%s: object %u: mask must be 8-byte, offsets / sigma_c / rgb_c 4-byte aligned", who, k);
    }
    FOC_REQUIRE(((uintptr_t)merged4 & 15) == 0, FOC_E_INVALID, "%s: merged4 must be 16-byte aligned", who);
    FOC_REQUIRE(((uintptr_t)obj_weights & 3) == 0 && ((uintptr_t)obj_depth & 3) == 0 && ((uintptr_t)instance & 3) == 0, FOC_E_INVALID,
                "%s: obj_weights, obj_depth and instance must be 4-byte aligned", who);
    L.objs = objs; L.K = K; L.nears = nears; L.fars = fars; L.N = N; L.T = T; L.bg0 = bgs[0]; L.bg1 = n_bg > 1 ? bgs[1] : 0.0f; L.n_bg = n_bg;
    L.image4 = image4; L.depth = depth; L.merged4 = reinterpret_cast<float4 *>(merged4); L.stream = (hipStream_t)stream;
    L.at.n_obj = n_obj;
    L.at.obj_weights = obj_weights; L.at.obj_depth = obj_depth; L.at.instance = instance; L.at.winner = n_obj ? winner : nullptr;
    if (K <= 2) cc_launch_k<2>(L, n_obj);
    else if (K <= 4) cc_launch_k<4>(L, n_obj);
    else if (K <= 8) cc_launch_k<8>(L, n_obj);
    else cc_launch_k<16>(L, n_obj);
    FOC_CHECK_LAUNCH(who);
    return FOC_OK;
}

int foc_combine_select4_ids(const float *field4, uint32_t id, float *acc4, uint8_t *acc_ids, uint64_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, field4);
    FOC_REQUIRE(id < FOC_COMBINE_MAX_OBJECTS, FOC_E_INVALID, "combine_select4_ids: id %u is not below %d", id, FOC_COMBINE_MAX_OBJECTS);
    FOC_REQUIRE(n == 0 || (field4 && acc4 && acc_ids), FOC_E_INVALID, "combine_select4_ids: null pointer");
    FOC_REQUIRE((((uintptr_t)field4 | (uintptr_t)acc4) & 15) == 0, FOC_E_INVALID, "combine_select4_ids: fields must be 16-byte aligned");
    if (n == 0) return FOC_OK;
    hipLaunchKernelGGL(k_combine_select4_ids, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(field4),
                       (uint8_t)id, reinterpret_cast<float4 *>(acc4), acc_ids, n);
    FOC_CHECK_LAUNCH("combine_select4_ids");
    return FOC_OK;
}

int foc_mo_select(const void *sigma_new, const void *feat_new, void *sigma_best, void *feat_best, uint64_t n, uint32_t feat_width,
                  uint32_t elem_bytes, void *stream) {
    FocDeviceGuard foc_guard_(stream, sigma_new);
    FOC_REQUIRE(elem_bytes == 2 || elem_bytes == 4, FOC_E_INVALID, "mo_select: elem_bytes must be 2 (half) or 4 (float), got %u", elem_bytes);
    FOC_REQUIRE(feat_width >= 1 && feat_width <= 64, FOC_E_INVALID, "mo_select: feat_width %u outside 1..64", feat_width);
    FOC_REQUIRE(n == 0 || (sigma_new && feat_new && sigma_best && feat_best), FOC_E_INVALID, "mo_select: null pointer");
    FOC_REQUIRE(n < (1ull << 38), FOC_E_INVALID, "mo_select: n too large");
    if (n == 0) return FOC_OK;
    const dim3 grid((uint32_t)((n + 255u) / 256u));
    if (elem_bytes == 2)
        hipLaunchKernelGGL(k_mo_select<__half>, grid, dim3(256), 0, (hipStream_t)stream, (const __half *)sigma_new, (const __half *)feat_new,
                           (__half *)sigma_best, (__half *)feat_best, n, feat_width);
    else
        hipLaunchKernelGGL(k_mo_select<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float *)sigma_new, (const float *)feat_new,
                           (float *)sigma_best, (float *)feat_best, n, feat_width);
    FOC_CHECK_LAUNCH("mo_select");
    return FOC_OK;
}

int foc_abi_version(void) { return FOC_ABI_VERSION; }
const char *foc_last_error(void) { return g_err; }
const char *foc_arch(void) { return "gfx950"; }

int foc_combine_select(const float *dens, const float *rgb, float *max_dens, float *best_rgb, uint64_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, dens);
    FOC_REQUIRE(n == 0 || (dens && rgb && max_dens && best_rgb), FOC_E_INVALID, "combine_select: null pointer");
    if (n == 0) return FOC_OK;
    hipLaunchKernelGGL(k_combine_select, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, dens, rgb, max_dens, best_rgb, n);
    FOC_CHECK_LAUNCH("combine_select");
    return FOC_OK;
}

int foc_combine_pack_keys(const float *dens, uint32_t rank, uint64_t *keys, uint64_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, dens);
    FOC_REQUIRE(n == 0 || (dens && keys), FOC_E_INVALID, "combine_pack_keys: null pointer");
    if (n == 0) return FOC_OK;
    hipLaunchKernelGGL(k_combine_pack, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, dens, rank, keys, n);
    FOC_CHECK_LAUNCH("combine_pack_keys");
    return FOC_OK;
}

int foc_combine_unpack(const uint64_t *keys, uint32_t rank, const float *rgb, float *max_dens, float *masked_rgb, uint64_t n, void *stream) {
    FocDeviceGuard foc_guard_(stream, keys);
    FOC_REQUIRE(n == 0 || (keys && rgb && max_dens && masked_rgb), FOC_E_INVALID, "combine_unpack: null pointer");
    if (n == 0) return FOC_OK;
    hipLaunchKernelGGL(k_combine_unpack, dim3(foc_grid_1d(n, 256)), dim3(256), 0, (hipStream_t)stream, keys, rank, rgb, max_dens, masked_rgb, n);
    FOC_CHECK_LAUNCH("combine_unpack");
    return FOC_OK;
}

int foc_composite_fixed_steps(const float *sigmas, const float *rgbs, const float *nears, const float *fars, uint32_t N, uint32_t T,
                              float bg, float *image4, float *depth, void *stream) {
    FocDeviceGuard foc_guard_(stream, sigmas);
    FOC_REQUIRE(N == 0 || (sigmas && rgbs && nears && fars && image4 && depth), FOC_E_INVALID, "composite_fixed_steps: null pointer");
    FOC_REQUIRE(T >= 2, FOC_E_INVALID, "composite_fixed_steps: T must be >= 2");
    if (N == 0) return FOC_OK;
    hipLaunchKernelGGL(k_composite_fixed, dim3(foc_div_up(N, 4)), dim3(256), 0, (hipStream_t)stream, sigmas, rgbs, nears, fars, N, T, bg, image4, depth);
    FOC_CHECK_LAUNCH("composite_fixed_steps");
    return FOC_OK;
}

} // extern "C"
