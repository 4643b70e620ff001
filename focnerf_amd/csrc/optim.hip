// optim.hip — the trainer's optimizer step as two launches (no reference binding: the reference trainer runs torch.optim.Adam under a
// GradScaler, nerf/utils.py:1225-1235; about twenty launches per step).
//
//   k_opt_check   A: one pass over every grad of the group for a non-finite element (every finder stores the same flag value, so the
//                 result has no order); the LAST workgroup to finish (a ticket counter) takes the decision of the whole step and writes
//                 the step record: skip, 1 / scale, and per tensor lr / (1 - beta1^t) and sqrt(1 - beta2^t) in double from that tensor's
//                 own step counter; it advances the step counters (unless skipped) and applies torch._amp_update_scale_'s rule to the
//                 scale and the growth tracker. Nothing of a step reads the scale or a step counter after this launch has changed them.
//   k_opt_adam    B: a workgroup finds its (tensor, chunk of OPT_CHUNK elements) in the descriptors, reads the record and updates
//                 p, exp_avg, exp_avg_sq in one pass (optionally zeroing the grad); skipped steps leave all three untouched.
//   k_opt_record  the record alone, one workgroup, where somebody else has done the check (torch's GradScaler hands over found_inf and
//                 grad_scale) or there is none (plain Adam): then k_opt_record, k_opt_adam.
//   k_opt_decide  the decision alone, for a step of more than 16 tensors: every group's check launch (no decision), this, then every
//                 group's record and update with the decision's words as their found_inf / grad_scale.
//
// The parameter EMA (torch_ema's rule, include/focnerf.h): s <- s - (s - p) * omd, three fp32 roundings, omd = float(1 - decay_t) with
// decay_t = min(decay, (1 + n) / (10 + n)) in double from a device int64 counter n that the step advances first.
//   k_opt_adam_ema  k_opt_adam's body with the shadow flag: the rule on the p it has just computed, still in registers; the shadow is a
//                   fifth stream under the same access rules (the update's 343 MB become 441 MB). A skipped step reads p and s and
//                   writes s. A tensor without a shadow takes k_opt_adam's path. k_opt_adam itself is the instantiation without the
//                   flag: the same instructions as before the flag existed.
//   omd             one lane, where the record is written (k_opt_check's last workgroup, k_opt_decide, k_opt_record), into record word
//                   OPT_W_EMA_OMD; the counter advances there and nothing reads it after that launch.
//   k_ema_update    parameters no step touches, and a bare update: reads p, reads and writes s. Opening a step (advance), every
//                   workgroup derives omd from the counter itself (one double division on one lane) and the last one to finish — the
//                   check's ticket — stores the advanced counter and the record word; otherwise it reads the record word.
//
// Measured on the headline parameter set (12.2 M floats, MI355X), which is why the shapes are these: B reading a finished record runs
// at 51 us (6.7 TB/s of its 343 MB). A first form of the one-launch route — every workgroup of B computing its corrections (two double
// pow on one lane, a barrier) and taking a ticket behind a fence so that the last one could advance the counters — ran at 160 us; a
// one-workgroup launch in front of B costs a few microseconds. A with one workgroup and one ticket per chunk (3000) ran at 73 us for a
// 49 MB read, with 768 workgroups walking the chunks at 32 us, and without the fence in front of a clean workgroup's ticket at 14 us
// (9 us of it the stream): the fence, not the ticket word, was the cost (~28 ns per workgroup).
//
// Streaming work: 16-byte loads and stores per lane where p, grad, exp_avg and exp_avg_sq of a tensor are all 16-byte aligned (chunks
// start at multiples of OPT_CHUNK elements, so a chunk is aligned when its tensor is), 4-byte accesses otherwise (a view at a storage
// offset of one element) and for the last n % 4 elements. 256 threads x 4 elements x 4 rounds per chunk; the headline parameter set is
// ~3000 chunks. No LDS beyond one broadcast word, no order-dependent sums: FOC_DETERMINISTIC changes nothing.
#include <cmath>
#include "common.h"

#define OPT_MAX_TENSORS FOC_OPTIM_MAX_TENSORS
#define OPT_CHUNK FOC_OPTIM_CHUNK                // elements per workgroup
#define OPT_THREADS 256
#ifndef OPT_CHECK_WGS
#define OPT_CHECK_WGS 768                        // three workgroups per CU walk the check's chunks
#endif

// workspace words (uint32 / float); the caller zeroes them ONCE, every launch leaves flag and tickets at zero again
#define OPT_W_FLAG 0                             // != 0: a non-finite grad was seen in this step
#define OPT_W_TICKET_A 1                         // second-level ticket of the check
#define OPT_W_SKIP 3                             // the record: uint32 skip
#define OPT_W_INV_SCALE 4                        //             float 1 / scale
#define OPT_W_FOUND 5                            // k_opt_decide: float found_inf (0 / 1) and the scale this step's grads carry,
#define OPT_W_SCALE_USED 6                       //               in the form torch's GradScaler hands them to an optimizer
#define OPT_W_EMA_OMD 7                          // the record: float 1 - decay_t of this step's parameter EMA
#define OPT_W_TENSORS 8                          // the record: per tensor float step_size, float sqrt(1 - beta2^t)
#define OPT_SHARDS 8                             // first-level ticket words of the check,
#define OPT_SHARD_STRIDE 32                      // one per 128-byte line
#define OPT_W_TICKET_SHARD 64
#define OPT_W_WORDS (OPT_W_TICKET_SHARD + OPT_SHARDS * OPT_SHARD_STRIDE)
static_assert(OPT_W_TENSORS + 2 * OPT_MAX_TENSORS <= OPT_W_TICKET_SHARD, "the record ends before the ticket lines");

struct OptTensor {
    float *p, *g, *m, *v, *step;
    const float *lr_ptr;                         // 0-dim fp32 on the device, or NULL: `lr`
    uint64_t n;
    double lr, beta1, beta2;
    float b2, om_b1, om_b2, eps, wd;             // beta2, 1 - beta1, 1 - beta2 rounded once from double
    uint32_t chunk0;                             // first workgroup of this tensor
};
struct OptGroup {
    OptTensor t[OPT_MAX_TENSORS];
    uint32_t n_tensors, n_chunks, zero_grads;
};
struct OptScale {
    float *scale;
    int32_t *tracker;
    float growth, backoff;
    int32_t interval;
};
struct OptShadow {
    float *s[OPT_MAX_TENSORS];                   // the EMA shadow of tensor k, or NULL: that tensor has none
};
struct OptEma {
    int64_t *counter;                            // torch_ema's num_updates on the device, or NULL: constant decay
    double decay;
    uint32_t advance;                            // != 0: this launch opens the step's EMA (advances the counter, writes OPT_W_EMA_OMD)
};

// step_size = lr / (1 - beta1^t) and sqrt(1 - beta2^t) for the step that makes the counter t, in double, rounded once each
__device__ __forceinline__ void opt_corrections(const OptTensor &T, float t, float &step_size, float &bc2_sqrt) {
    const double lr = T.lr_ptr ? (double)*T.lr_ptr : T.lr;
    step_size = (float)(lr / (1.0 - pow(T.beta1, (double)t)));
    bc2_sqrt = (float)sqrt(1.0 - pow(T.beta2, (double)t));
}

__device__ __forceinline__ int opt_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }      // inf or nan

// torch._amp_update_scale_ (ATen/native/cuda/AmpKernels.cu amp_update_scale_cuda_kernel), one thread
__device__ __forceinline__ void opt_update_scale(const OptScale &S, bool found) {
    if (found) {
        *S.scale = *S.scale * S.backoff;
        *S.tracker = 0;
    } else {
        const int32_t successful = *S.tracker + 1;
        if (successful == S.interval) {
            const float grown = *S.scale * S.growth;
            if (isfinite(grown)) *S.scale = grown;
            *S.tracker = 0;
        } else {
            *S.tracker = successful;
        }
    }
}

// torch_ema's schedule at the count n that this update makes, in double, rounded once
__device__ __forceinline__ float opt_ema_omd(double decay, int64_t n) {
    const double warm = (1.0 + (double)n) / (10.0 + (double)n);
    return (float)(1.0 - (warm < decay ? warm : decay));
}

// one thread, where the step record is written: advance the counter and leave 1 - decay_t in the record
__device__ __forceinline__ void opt_ema_open(const OptEma &E, uint32_t *ws) {
    if (!E.advance) return;
    float omd = (float)(1.0 - E.decay);
    if (E.counter) {
        const int64_t n = *E.counter + 1;
        *E.counter = n;
        omd = opt_ema_omd(E.decay, n);
    }
    reinterpret_cast<float *>(ws)[OPT_W_EMA_OMD] = omd;
}

// the workgroup's tensor: the last one whose first chunk is not beyond this workgroup (n_tensors <= 16, uniform)
__device__ __forceinline__ uint32_t opt_find_tensor(const OptGroup &G, uint32_t wg) {
    uint32_t ti = 0;
    for (uint32_t k = 1; k < G.n_tensors; k++) ti = G.t[k].chunk0 <= wg ? k : ti;
    return ti;
}

// the record of one group, by the threads of ONE workgroup (all of them call): lane k takes tensor k in a uniform walk over the argument
// block, then up to sixteen lanes compute their corrections side by side; the step counters advance unless the step is skipped
__device__ __forceinline__ void opt_write_record(const OptGroup &G, uint32_t *ws, bool found, float inv_scale) {
    const uint32_t tid = threadIdx.x;
    OptTensor T = G.t[0];
    for (uint32_t k = 1; k < G.n_tensors; k++)
        if (tid == k) T = G.t[k];
    if (tid < G.n_tensors) {
        const float t = *T.step + 1.0f;
        float step_size, bc2_sqrt;
        opt_corrections(T, t, step_size, bc2_sqrt);
        reinterpret_cast<float *>(ws)[OPT_W_TENSORS + 2 * tid] = step_size;
        reinterpret_cast<float *>(ws)[OPT_W_TENSORS + 2 * tid + 1] = bc2_sqrt;
        if (!found) *T.step = t;
    }
    if (tid == 0) {
        ws[OPT_W_SKIP] = found ? 1u : 0u;
        reinterpret_cast<float *>(ws)[OPT_W_INV_SCALE] = inv_scale;
    }
}

// true in every thread of the LAST workgroup of the launch to get here, found in two levels: each takes a ticket of its shard (blockIdx
// mod 8, a cache line each), the last of a shard one of the eight second-level tickets. The shard words are left at zero; the caller
// zeroes OPT_W_TICKET_A.
__device__ __forceinline__ bool opt_last_workgroup(uint32_t *ws) {
    __shared__ uint32_t s_last;
    if (threadIdx.x == 0) {
        const uint32_t shard = blockIdx.x % OPT_SHARDS, shards = gridDim.x < OPT_SHARDS ? gridDim.x : OPT_SHARDS;
        const uint32_t in_shard = (gridDim.x - shard + OPT_SHARDS - 1) / OPT_SHARDS;
        uint32_t last = 0;
        if (atomicAdd(&ws[OPT_W_TICKET_SHARD + OPT_SHARD_STRIDE * shard], 1u) == in_shard - 1) {
            ws[OPT_W_TICKET_SHARD + OPT_SHARD_STRIDE * shard] = 0;         // everybody of this shard has been here
            last = atomicAdd(&ws[OPT_W_TICKET_A], 1u) == shards - 1;
        }
        s_last = last;
    }
    __syncthreads();
    return s_last != 0;
}

// ---------------------------------------------------------------- A: check (+ decide)
// At most OPT_CHECK_WGS workgroups walk the chunks, so the tail below runs 768 times, not once per chunk; a full aligned chunk is four
// independent 16-byte loads per lane.
__global__ void __launch_bounds__(OPT_THREADS) k_opt_check(OptGroup G, OptScale S, OptEma E, uint32_t decide, uint32_t *__restrict__ ws) {
    const uint32_t tid = threadIdx.x;
    int bad = 0;
    for (uint32_t c = blockIdx.x; c < G.n_chunks; c += gridDim.x) {
        const uint32_t ti = opt_find_tensor(G, c);
        const float *g = G.t[ti].g;
        const uint64_t n = G.t[ti].n;
        const uint64_t begin = (uint64_t)(c - G.t[ti].chunk0) * OPT_CHUNK;
        const uint64_t end = begin + OPT_CHUNK < n ? begin + OPT_CHUNK : n;
        if ((((uintptr_t)g) & 15) == 0) {
            if (end - begin == OPT_CHUNK) {
                float4 x[OPT_CHUNK / (4 * OPT_THREADS)];
#pragma unroll
                for (uint32_t k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); k++) x[k] = *reinterpret_cast<const float4 *>(g + begin + (uint64_t)tid * 4 + k * (4 * OPT_THREADS));
#pragma unroll
                for (uint32_t k = 0; k < OPT_CHUNK / (4 * OPT_THREADS); k++) bad |= opt_nonfinite(x[k].x) | opt_nonfinite(x[k].y) | opt_nonfinite(x[k].z) | opt_nonfinite(x[k].w);
                continue;
            }
            const uint64_t end4 = begin + ((end - begin) & ~(uint64_t)3);
            for (uint64_t i = begin + (uint64_t)tid * 4; i < end4; i += OPT_THREADS * 4) {
                const float4 x = *reinterpret_cast<const float4 *>(g + i);
                bad |= opt_nonfinite(x.x) | opt_nonfinite(x.y) | opt_nonfinite(x.z) | opt_nonfinite(x.w);
            }
            for (uint64_t i = end4 + tid; i < end; i += OPT_THREADS) bad |= opt_nonfinite(g[i]);
        } else {
            for (uint64_t i = begin + tid; i < end; i += OPT_THREADS) bad |= opt_nonfinite(g[i]);
        }
    }
    bad = __syncthreads_or(bad);
    if (tid == 0 && bad) {
        atomicOr(&ws[OPT_W_FLAG], 1u);
        __threadfence();                                                  // the flag is set before this workgroup's ticket is taken
    }
    if (!decide) return;

    // The last workgroup to finish, found in two levels: each takes a ticket of its shard (blockIdx mod 8, a cache line each), the last
    // of a shard one of the eight second-level tickets. The flag and the tickets are touched by device-scope atomics only, so a
    // workgroup that found nothing has nothing to publish and takes its ticket without a fence: with a fence in front of every ticket
    // this tail cost ~28 ns per workgroup (22 us at 768 workgroups, measured), one fence per XCD at a time.
    if (!opt_last_workgroup(ws)) return;
    __threadfence();
    const bool found = atomicOr(&ws[OPT_W_FLAG], 0u) != 0;               // every workgroup's flag store is ordered before its ticket
    opt_write_record(G, ws, found, 1.0f / *S.scale);
    if (tid == 0) {
        opt_update_scale(S, found);
        opt_ema_open(E, ws);
        ws[OPT_W_FLAG] = 0;
        ws[OPT_W_TICKET_A] = 0;
    }
}

// the decision of a step that spans several groups: after every group's check launch, before every group's record and update
__global__ void k_opt_decide(OptScale S, OptEma E, uint32_t *__restrict__ ws) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const bool found = atomicOr(&ws[OPT_W_FLAG], 0u) != 0;
    reinterpret_cast<float *>(ws)[OPT_W_FOUND] = found ? 1.0f : 0.0f;
    reinterpret_cast<float *>(ws)[OPT_W_SCALE_USED] = *S.scale;
    opt_update_scale(S, found);
    opt_ema_open(E, ws);
    ws[OPT_W_FLAG] = 0;
}

// the record of a group whose check somebody else has done (torch's GradScaler, the decide launch above) or that has none: one workgroup
__global__ void __launch_bounds__(64) k_opt_record(OptGroup G, OptEma E, const float *__restrict__ grad_scale, const float *__restrict__ found_inf,
                                                   uint32_t *__restrict__ ws) {
    const bool found = found_inf != nullptr && *found_inf != 0.0f;
    opt_write_record(G, ws, found, grad_scale ? 1.0f / *grad_scale : 1.0f);
    if (threadIdx.x == 0) opt_ema_open(E, ws);
}

// ---------------------------------------------------------------- B: update
struct OptCoef { float inv_scale, wd, om_b1, b2, om_b2, step_size, bc2_sqrt, eps; };

// one element; every rounding is one of these operations (the tree builds with -ffp-contract=off, division and sqrt correctly rounded)
__device__ __forceinline__ void opt_adam1(const OptCoef &c, float &p, float grad, float &m, float &v) {
    float g = grad * c.inv_scale;
    if (c.wd != 0.0f) g = fmaf(c.wd, p, g);
    m = fmaf(g - m, c.om_b1, m);
    v = fmaf(c.om_b2, g * g, c.b2 * v);
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p - c.step_size * m / denom;
}

// the parameter EMA on one element: three roundings (fp contraction is off in this tree; the intrinsics say so here too)
__device__ __forceinline__ float opt_ema1(float s, float p, float omd) { return __fsub_rn(s, __fmul_rn(__fsub_rn(s, p), omd)); }

// EMA: the shadow of the workgroup's tensor is a fifth stream, updated from the p just computed (or, in a skipped step, just read).
// EMA = false is the update as it was before the flag existed: `s` is not looked at and every `if (EMA)` folds away.
template <bool EMA>
__device__ __forceinline__ void opt_adam_body(const OptGroup &G, const uint32_t ti, float *s, const uint32_t *__restrict__ ws) {
    const uint32_t tid = threadIdx.x, wg = blockIdx.x;
    const OptTensor &T = G.t[ti];
    float *p = T.p, *g = T.g, *m = T.m, *v = T.v;
    const uint64_t n = T.n;
    const uint64_t begin = (uint64_t)(wg - T.chunk0) * OPT_CHUNK;
    const uint64_t end = begin + OPT_CHUNK < n ? begin + OPT_CHUNK : n;
    const uint64_t end4 = begin + ((end - begin) & ~(uint64_t)3);
    const bool vec = (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (EMA ? (uintptr_t)s : (uintptr_t)0)) & 15) == 0;
    const float omd = EMA ? reinterpret_cast<const float *>(ws)[OPT_W_EMA_OMD] : 0.0f;

    if (ws[OPT_W_SKIP] != 0) {                                            // params, moments and step counters stay as they are;
        if (EMA) {                                                        // the shadow still moves toward the unchanged params
            if (vec) {
                for (uint64_t i = begin + (uint64_t)tid * 4; i < end4; i += OPT_THREADS * 4) {
                    const float4 pp = *reinterpret_cast<const float4 *>(p + i);
                    float4 ss = *reinterpret_cast<const float4 *>(s + i);
                    ss.x = opt_ema1(ss.x, pp.x, omd); ss.y = opt_ema1(ss.y, pp.y, omd); ss.z = opt_ema1(ss.z, pp.z, omd); ss.w = opt_ema1(ss.w, pp.w, omd);
                    *reinterpret_cast<float4 *>(s + i) = ss;
                }
            }
            for (uint64_t i = (vec ? end4 : begin) + tid; i < end; i += OPT_THREADS) s[i] = opt_ema1(s[i], p[i], omd);
        }
        if (G.zero_grads) {                                               // a grad the caller asked to have zeroed is zeroed all the same
            if (vec) {
                for (uint64_t i = begin + (uint64_t)tid * 4; i < end4; i += OPT_THREADS * 4) *reinterpret_cast<float4 *>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
                for (uint64_t i = end4 + tid; i < end; i += OPT_THREADS) g[i] = 0.0f;
            } else {
                for (uint64_t i = begin + tid; i < end; i += OPT_THREADS) g[i] = 0.0f;
            }
        }
        return;
    }

    OptCoef c;
    c.wd = T.wd; c.om_b1 = T.om_b1; c.b2 = T.b2; c.om_b2 = T.om_b2; c.eps = T.eps;
    c.inv_scale = reinterpret_cast<const float *>(ws)[OPT_W_INV_SCALE];
    c.step_size = reinterpret_cast<const float *>(ws)[OPT_W_TENSORS + 2 * ti];
    c.bc2_sqrt = reinterpret_cast<const float *>(ws)[OPT_W_TENSORS + 2 * ti + 1];

    const bool zero = G.zero_grads != 0;
    if (vec) {
        for (uint64_t i = begin + (uint64_t)tid * 4; i < end4; i += OPT_THREADS * 4) {
            float4 pp = *reinterpret_cast<const float4 *>(p + i);
            const float4 gg = *reinterpret_cast<const float4 *>(g + i);
            float4 mm = *reinterpret_cast<const float4 *>(m + i);
            float4 vv = *reinterpret_cast<const float4 *>(v + i);
            float4 ss;
            if (EMA) ss = *reinterpret_cast<const float4 *>(s + i);
            opt_adam1(c, pp.x, gg.x, mm.x, vv.x);
            opt_adam1(c, pp.y, gg.y, mm.y, vv.y);
            opt_adam1(c, pp.z, gg.z, mm.z, vv.z);
            opt_adam1(c, pp.w, gg.w, mm.w, vv.w);
            *reinterpret_cast<float4 *>(p + i) = pp;
            *reinterpret_cast<float4 *>(m + i) = mm;
            *reinterpret_cast<float4 *>(v + i) = vv;
            if (EMA) {
                ss.x = opt_ema1(ss.x, pp.x, omd); ss.y = opt_ema1(ss.y, pp.y, omd); ss.z = opt_ema1(ss.z, pp.z, omd); ss.w = opt_ema1(ss.w, pp.w, omd);
                *reinterpret_cast<float4 *>(s + i) = ss;
            }
            if (zero) *reinterpret_cast<float4 *>(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    for (uint64_t i = (vec ? end4 : begin) + tid; i < end; i += OPT_THREADS) {
        float pp = p[i], mm = m[i], vv = v[i];
        opt_adam1(c, pp, g[i], mm, vv);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (EMA) s[i] = opt_ema1(s[i], pp, omd);
        if (zero) g[i] = 0.0f;
    }
}

__global__ void __launch_bounds__(OPT_THREADS) k_opt_adam(OptGroup G, const uint32_t *__restrict__ ws) {
    opt_adam_body<false>(G, opt_find_tensor(G, blockIdx.x), nullptr, ws);
}

// the update with shadows: a tensor of the group that has none takes k_opt_adam's path
__global__ void __launch_bounds__(OPT_THREADS) k_opt_adam_ema(OptGroup G, OptShadow SH, const uint32_t *__restrict__ ws) {
    const uint32_t ti = opt_find_tensor(G, blockIdx.x);
    float *s = SH.s[0];
    for (uint32_t k = 1; k < G.n_tensors; k++) s = k == ti ? SH.s[k] : s;
    if (s != nullptr) opt_adam_body<true>(G, ti, s, ws);
    else opt_adam_body<false>(G, ti, nullptr, ws);
}

// ---------------------------------------------------------------- the EMA alone
struct EmaTensor {
    const float *p;
    float *s;
    uint64_t n;
    uint32_t chunk0;
};
struct EmaGroup {
    EmaTensor t[OPT_MAX_TENSORS];
    uint32_t n_tensors;
};

// One workgroup per chunk of OPT_CHUNK elements. E.advance with a counter: lane 0 of EVERY workgroup reads the counter and derives omd
// (no workgroup waits for another); each takes its ticket after that read has been used, and the last one stores the advanced counter
// and the record word, so nobody reads the counter after it has changed. E.advance without a counter: omd is `omd_const`. Otherwise
// omd is the record word that the launch which opened this step has left.
__global__ void __launch_bounds__(OPT_THREADS) k_ema_update(EmaGroup G, OptEma E, float omd_const, uint32_t *__restrict__ ws) {
    const uint32_t tid = threadIdx.x, wg = blockIdx.x;
    __shared__ float s_omd;
    int64_t count = 0;
    if (tid == 0) {
        float o = omd_const;
        if (!E.advance) o = reinterpret_cast<const float *>(ws)[OPT_W_EMA_OMD];
        else if (E.counter) {
            count = *E.counter + 1;
            o = opt_ema_omd(E.decay, count);
        }
        s_omd = o;
    }
    __syncthreads();
    const float omd = s_omd;

    uint32_t ti = 0;
    for (uint32_t k = 1; k < G.n_tensors; k++) ti = G.t[k].chunk0 <= wg ? k : ti;
    const EmaTensor &T = G.t[ti];
    const float *p = T.p;
    float *s = T.s;
    const uint64_t begin = (uint64_t)(wg - T.chunk0) * OPT_CHUNK;                    // (a launch for the counter alone: n = 0, nothing below runs)
    const uint64_t end = begin + OPT_CHUNK < T.n ? begin + OPT_CHUNK : (begin < T.n ? T.n : begin);
    const uint64_t end4 = begin + ((end - begin) & ~(uint64_t)3);
    const bool vec = (((uintptr_t)p | (uintptr_t)s) & 15) == 0;
    if (vec) {
        for (uint64_t i = begin + (uint64_t)tid * 4; i < end4; i += OPT_THREADS * 4) {
            const float4 pp = *reinterpret_cast<const float4 *>(p + i);
            float4 ss = *reinterpret_cast<const float4 *>(s + i);
            ss.x = opt_ema1(ss.x, pp.x, omd); ss.y = opt_ema1(ss.y, pp.y, omd); ss.z = opt_ema1(ss.z, pp.z, omd); ss.w = opt_ema1(ss.w, pp.w, omd);
            *reinterpret_cast<float4 *>(s + i) = ss;
        }
    }
    for (uint64_t i = (vec ? end4 : begin) + tid; i < end; i += OPT_THREADS) s[i] = opt_ema1(s[i], p[i], omd);

    if (!E.advance) return;
    if (E.counter == nullptr) {
        if (wg == 0 && tid == 0) reinterpret_cast<float *>(ws)[OPT_W_EMA_OMD] = omd;
        return;
    }
    if (!opt_last_workgroup(ws)) return;
    if (tid == 0) {
        *E.counter = count;
        reinterpret_cast<float *>(ws)[OPT_W_EMA_OMD] = omd;
        ws[OPT_W_TICKET_A] = 0;
    }
}

// ---------------------------------------------------------------- host side
extern "C" {

size_t foc_optim_workspace_bytes(int n_tensors) {
    if (n_tensors < 1 || n_tensors > OPT_MAX_TENSORS) return 0;
    return (size_t)OPT_W_WORDS * sizeof(uint32_t);
}

// foc_optim_step (shadow NULL, E all zero) and foc_optim_step_ema behind its own checks
static int optim_step(const FocOptimStep *s, const uint64_t *shadow, const OptEma &E, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FOC_REQUIRE(s != nullptr, FOC_E_INVALID, "optim_step: null step");
    FOC_REQUIRE(s->struct_bytes == sizeof(FocOptimStep), FOC_E_INVALID, "optim_step: struct of %u bytes, this library's FocOptimStep has %zu", s->struct_bytes,
                sizeof(FocOptimStep));
    FOC_REQUIRE(s->tensor_bytes == sizeof(FocOptimTensor), FOC_E_INVALID, "optim_step: tensor descriptors of %u bytes, this library's FocOptimTensor has %zu",
                s->tensor_bytes, sizeof(FocOptimTensor));
    FOC_REQUIRE(s->phase <= FOC_OPTIM_DECIDE, FOC_E_INVALID, "optim_step: phase must be FOC_OPTIM_STEP, _CHECK or _DECIDE (got %u)", s->phase);
    const bool has_scaler = s->scale != nullptr || s->growth_tracker != nullptr;
    const bool external = s->grad_scale != nullptr || s->found_inf != nullptr;
    FOC_REQUIRE((s->scale != nullptr) == (s->growth_tracker != nullptr), FOC_E_INVALID, "optim_step: null pointer (scale and growth_tracker come together)");
    FOC_REQUIRE(!(has_scaler && external), FOC_E_INVALID, "optim_step: scale / growth_tracker and external grad_scale / found_inf exclude each other");
    FOC_REQUIRE(s->phase == FOC_OPTIM_STEP || has_scaler, FOC_E_INVALID, "optim_step: null pointer (the check and decide phases need scale and growth_tracker)");
    FOC_REQUIRE(s->workspace != nullptr, FOC_E_INVALID, "optim_step: null pointer (workspace)");
    FOC_REQUIRE((((uintptr_t)s->workspace) & 3) == 0, FOC_E_INVALID, "optim_step: workspace must be 4-byte aligned");
    FOC_REQUIRE(s->workspace_bytes >= (uint64_t)OPT_W_WORDS * sizeof(uint32_t), FOC_E_INVALID, "optim_step: workspace of %llu bytes, foc_optim_workspace_bytes asks for %zu",
                (unsigned long long)s->workspace_bytes, (size_t)OPT_W_WORDS * sizeof(uint32_t));
    OptScale S{};
    if (has_scaler) {
        FOC_REQUIRE(std::isfinite(s->growth_factor) && std::isfinite(s->backoff_factor) && s->growth_factor > 0 && s->backoff_factor > 0 && s->growth_interval >= 1,
                    FOC_E_INVALID, "optim_step: growth_factor and backoff_factor must be finite and > 0, growth_interval >= 1");
        S.scale = s->scale; S.tracker = s->growth_tracker; S.growth = s->growth_factor; S.backoff = s->backoff_factor; S.interval = s->growth_interval;
    }
    uint32_t *ws = reinterpret_cast<uint32_t *>(s->workspace);
    if (s->phase == FOC_OPTIM_DECIDE) {
        FocDeviceGuard foc_guard_(stream_, s->workspace);
        hipLaunchKernelGGL(k_opt_decide, dim3(1), dim3(64), 0, stream, S, E, ws);
        FOC_CHECK_LAUNCH("optim_step (decide)");
        return FOC_OK;
    }

    FOC_REQUIRE(s->n_tensors >= 1 && s->n_tensors <= OPT_MAX_TENSORS, FOC_E_INVALID, "optim_step: n_tensors must be 1 .. %d (got %d)", OPT_MAX_TENSORS, s->n_tensors);
    FOC_REQUIRE(s->tensors != nullptr, FOC_E_INVALID, "optim_step: null pointer (tensors)");
    OptGroup G{};
    OptShadow SH{};
    bool any_shadow = false;
    uint64_t chunks = 0;
    for (int k = 0; k < s->n_tensors; k++) {
        const FocOptimTensor &t = s->tensors[k];
        if (shadow != nullptr && shadow[k] != 0) {
            FOC_REQUIRE((shadow[k] & 3) == 0, FOC_E_INVALID, "optim_step_ema: tensor %d: the shadow must be 4-byte aligned", k);
            SH.s[k] = reinterpret_cast<float *>((uintptr_t)shadow[k]);
            any_shadow = true;
        }
        FOC_REQUIRE(t.param && t.grad && t.exp_avg && t.exp_avg_sq && t.step, FOC_E_INVALID, "optim_step: null pointer (tensor %d)", k);
        FOC_REQUIRE(t.n >= 0, FOC_E_INVALID, "optim_step: negative size (tensor %d: %lld)", k, (long long)t.n);
        FOC_REQUIRE(t.beta1 >= 0 && t.beta1 < 1 && t.beta2 >= 0 && t.beta2 < 1, FOC_E_INVALID, "optim_step: betas must lie in [0, 1) (tensor %d: %g, %g)", k, t.beta1,
                    t.beta2);
        FOC_REQUIRE(t.eps >= 0 && t.lr >= 0 && t.weight_decay >= 0, FOC_E_INVALID, "optim_step: eps, lr and weight_decay must not be negative (tensor %d: %g, %g, %g)", k,
                    t.eps, t.lr, t.weight_decay);
        FOC_REQUIRE(((((uintptr_t)t.param) | ((uintptr_t)t.grad) | ((uintptr_t)t.exp_avg) | ((uintptr_t)t.exp_avg_sq) | ((uintptr_t)t.step) | ((uintptr_t)t.lr_tensor)) & 3) == 0,
                    FOC_E_INVALID, "optim_step: tensor %d: pointers must be 4-byte aligned", k);
        OptTensor &o = G.t[k];
        o.p = t.param; o.g = t.grad; o.m = t.exp_avg; o.v = t.exp_avg_sq; o.step = t.step; o.lr_ptr = t.lr_tensor;
        o.n = (uint64_t)t.n;
        o.lr = t.lr; o.beta1 = t.beta1; o.beta2 = t.beta2;
        o.b2 = (float)t.beta2; o.om_b1 = (float)(1.0 - t.beta1); o.om_b2 = (float)(1.0 - t.beta2); o.eps = (float)t.eps; o.wd = (float)t.weight_decay;
        o.chunk0 = (uint32_t)chunks;
        chunks += (o.n + OPT_CHUNK - 1) / OPT_CHUNK;
        FOC_REQUIRE(chunks < (1ull << 31), FOC_E_INVALID, "optim_step: more than 2^31 chunks of %d elements", OPT_CHUNK);
    }
    G.n_tensors = (uint32_t)s->n_tensors;
    G.n_chunks = (uint32_t)chunks;
    G.zero_grads = s->zero_grads ? 1u : 0u;

    FocDeviceGuard foc_guard_(stream_, s->tensors[0].param);
    if (has_scaler) {
        const uint32_t decide = s->phase == FOC_OPTIM_STEP;
        if (chunks > 0 || decide) {                                        // a group of empty tensors still takes its decision
            const uint32_t wgs = chunks == 0 ? 1u : chunks < OPT_CHECK_WGS ? (uint32_t)chunks : (uint32_t)OPT_CHECK_WGS;
            hipLaunchKernelGGL(k_opt_check, dim3(wgs), dim3(OPT_THREADS), 0, stream, G, S, E, decide, ws);
            FOC_CHECK_LAUNCH("optim_step (check)");
        }
        if (!decide) return FOC_OK;
    } else {
        hipLaunchKernelGGL(k_opt_record, dim3(1), dim3(64), 0, stream, G, E, s->grad_scale, s->found_inf, ws);
        FOC_CHECK_LAUNCH("optim_step (record)");
    }
    if (chunks > 0 && any_shadow) {
        hipLaunchKernelGGL(k_opt_adam_ema, dim3((uint32_t)chunks), dim3(OPT_THREADS), 0, stream, G, SH, ws);
        FOC_CHECK_LAUNCH("optim_step_ema (adam)");
    } else if (chunks > 0) {
        hipLaunchKernelGGL(k_opt_adam, dim3((uint32_t)chunks), dim3(OPT_THREADS), 0, stream, G, ws);
        FOC_CHECK_LAUNCH("optim_step (adam)");
    }
    return FOC_OK;
}

int foc_optim_step(const FocOptimStep *s, void *stream) { return optim_step(s, nullptr, OptEma{}, stream); }

int foc_optim_step_ema(const FocOptimStep *s, const uint64_t *shadow, double decay, int64_t *num_updates, uint32_t advance, void *stream) {
    FOC_REQUIRE(s != nullptr, FOC_E_INVALID, "optim_step_ema: null step");
    FOC_REQUIRE(shadow != nullptr || s->phase != FOC_OPTIM_STEP, FOC_E_INVALID, "optim_step_ema: null pointer (shadow)");
    FOC_REQUIRE(std::isfinite(decay) && decay >= 0 && decay <= 1, FOC_E_INVALID, "optim_step_ema: decay must lie in [0, 1] (got %g)", decay);
    FOC_REQUIRE((((uintptr_t)num_updates) & 7) == 0, FOC_E_INVALID, "optim_step_ema: num_updates must be 8-byte aligned");
    FOC_REQUIRE(!(advance && s->phase == FOC_OPTIM_CHECK), FOC_E_INVALID, "optim_step_ema: the check alone writes no record: advance belongs to the decide or step phase");
    return optim_step(s, s->phase == FOC_OPTIM_STEP ? shadow : nullptr, OptEma{num_updates, decay, advance ? 1u : 0u}, stream);
}

int foc_ema_update(const uint64_t *param, const uint64_t *shadow, const int64_t *n, int n_tensors, double decay, int64_t *num_updates, uint32_t advance,
                   void *workspace, uint64_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FOC_REQUIRE(param != nullptr && shadow != nullptr && n != nullptr, FOC_E_INVALID, "ema_update: null pointer (param, shadow and n are arrays of n_tensors entries)");
    FOC_REQUIRE(n_tensors >= 1 && n_tensors <= OPT_MAX_TENSORS, FOC_E_INVALID, "ema_update: n_tensors must be 1 .. %d (got %d)", OPT_MAX_TENSORS, n_tensors);
    FOC_REQUIRE(std::isfinite(decay) && decay >= 0 && decay <= 1, FOC_E_INVALID, "ema_update: decay must lie in [0, 1] (got %g)", decay);
    FOC_REQUIRE((((uintptr_t)num_updates) & 7) == 0, FOC_E_INVALID, "ema_update: num_updates must be 8-byte aligned");
    FOC_REQUIRE(workspace != nullptr, FOC_E_INVALID, "ema_update: null pointer (workspace)");
    FOC_REQUIRE((((uintptr_t)workspace) & 3) == 0, FOC_E_INVALID, "ema_update: workspace must be 4-byte aligned");
    FOC_REQUIRE(workspace_bytes >= (uint64_t)OPT_W_WORDS * sizeof(uint32_t), FOC_E_INVALID, "ema_update: workspace of %llu bytes, foc_optim_workspace_bytes asks for %zu",
                (unsigned long long)workspace_bytes, (size_t)OPT_W_WORDS * sizeof(uint32_t));
    EmaGroup G{};
    uint64_t chunks = 0;
    for (int k = 0; k < n_tensors; k++) {
        FOC_REQUIRE(param[k] != 0 && shadow[k] != 0, FOC_E_INVALID, "ema_update: null pointer (tensor %d)", k);
        FOC_REQUIRE(n[k] >= 0, FOC_E_INVALID, "ema_update: negative size (tensor %d: %lld)", k, (long long)n[k]);
        FOC_REQUIRE(((param[k] | shadow[k]) & 3) == 0, FOC_E_INVALID, "ema_update: tensor %d: pointers must be 4-byte aligned", k);
        EmaTensor &o = G.t[k];
        o.p = reinterpret_cast<const float *>((uintptr_t)param[k]);
        o.s = reinterpret_cast<float *>((uintptr_t)shadow[k]);
        o.n = (uint64_t)n[k];
        o.chunk0 = (uint32_t)chunks;
        chunks += (o.n + OPT_CHUNK - 1) / OPT_CHUNK;
        FOC_REQUIRE(chunks < (1ull << 31), FOC_E_INVALID, "ema_update: more than 2^31 chunks of %d elements", OPT_CHUNK);
    }
    G.n_tensors = (uint32_t)n_tensors;
    if (chunks == 0 && !advance) return FOC_OK;                            // empty tensors and no step to open: nothing to do
    const OptEma E{num_updates, decay, advance ? 1u : 0u};
    FocDeviceGuard foc_guard_(stream_, workspace);
    hipLaunchKernelGGL(k_ema_update, dim3(chunks == 0 ? 1u : (uint32_t)chunks), dim3(OPT_THREADS), 0, stream, G, E, (float)(1.0 - decay),
                       reinterpret_cast<uint32_t *>(workspace));
    FOC_CHECK_LAUNCH("ema_update");
    return FOC_OK;
}

} // extern "C"
