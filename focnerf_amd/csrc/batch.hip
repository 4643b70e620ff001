// batch.hip — the two ends of a training step (no reference binding: the reference trainer builds a batch with about fifteen torch ops,
// nerf/provider.py:398-447 NeRFDataset.collate and nerf/utils.py:57-157 get_rays, and its loss with about ten more and their backward
// nodes, nerf/utils.py:840-899 Trainer.train_step).
//
//   k_batch_sample  one thread per ray: the pixel (a stateless Philox draw, or the jittered cell of the error-map route), the ray of
//                   get_rays (:131-139), the pixel-wise random background (:853), the pixel and its blend (:856). Every value is a pure
//                   function of (seed, step, ray index): the number of workgroups changes nothing. Every workgroup reads `step` first
//                   and takes a ticket when it is done; the LAST one writes step + 1 and `view` and puts the ticket back to zero, so a
//                   replayed graph draws batch t, t + 1, t + 2 with nothing from the host and no memset node. No workgroup waits.
//   k_view_rays     the same ray arithmetic (one device function) for all H * W pixels of a view.
//   k_photo_loss    per ray the criterion (:867), its gradient with the mean's 1 / (3 N) applied, the error map's EMA (:893-894); per
//                   workgroup a fixed tree in double into one slot; the last workgroup (ticket) adds the slots in index order and writes
//                   float(sum / N) (:899). No float atomics, no order that depends on scheduling: the same bits on every run.
//
// Fences (csrc/optim.hip's header: the fence in front of a ticket, not the ticket word, is what costs, ~28 ns per workgroup). The sampler's
// workgroups publish nothing to one another — the last one writes `step + 1` from the value it read itself — so their tickets are taken
// without a fence; the workgroup barrier in front of the ticket is what orders every lane's read of `step` before it. The loss's
// workgroups do publish a slot: an agent-scope store, a fence, the ticket; the last one fences and reads the slots with agent-scope
// loads. At most PL_MAX_WGS (256) workgroups, so the fences cost a few microseconds at the very most and 16 of them at N = 4096.
//
// Every product and sum below is its own fp32 operation (the tree builds with -ffp-contract=off; division and sqrt correctly rounded):
// tests/batch_ref.py states the same operations in numpy, and the GPU tests compare bits.
#include <cmath>
#include "common.h"

#define BT_THREADS 256
#define BT_MAX_WGS 1024
#define PL_MAX_WGS FOC_PHOTO_LOSS_MAX_WGS
#define BT_CELLS 128                             // the error map is 128 x 128 cells per view (nerf/provider.py:320)
#define BT_WS_BYTES 128                          // the sampler's workspace: word 0 is the ticket
#define PL_WS_BYTES (128 + 8 * PL_MAX_WGS)       // the loss's workspace: word 0 the ticket, one slot (double) per workgroup from byte 128

// ---------------------------------------------------------------- Philox4x32-10 (Salmon et al., SC'11), stateless
struct Philox4 { uint32_t w[4]; };

__host__ __device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}
__device__ __forceinline__ float bt_uniform(uint32_t w) { return (float)(w >> 8) * 5.9604644775390625e-08f; }      // (w >> 8) * 2^-24, exact, in [0, 1)

// ---------------------------------------------------------------- the ray of one pixel (nerf/utils.py:131-139)
struct BtCamera { float fx, fy, cx, cy; };
struct BtPose { float r[3][3], t[3]; };

__device__ __forceinline__ BtPose bt_load_pose(const float *__restrict__ p) {                    // [4,4] row-major
    BtPose P;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        P.r[k][0] = p[4 * k]; P.r[k][1] = p[4 * k + 1]; P.r[k][2] = p[4 * k + 2]; P.t[k] = p[4 * k + 3];
    }
    return P;
}
__device__ __forceinline__ void bt_ray(const BtCamera &K, const BtPose &P, uint32_t row, uint32_t col, float *__restrict__ o, float *__restrict__ d) {
    const float x = (((float)col + 0.5f) - K.cx) / K.fx;
    const float y = (((float)row + 0.5f) - K.cy) / K.fy;
    const float n = sqrtf((x * x + y * y) + 1.0f);
    const float dx = x / n, dy = y / n, dz = 1.0f / n;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        d[k] = (P.r[k][0] * dx + P.r[k][1] * dy) + P.r[k][2] * dz;
        o[k] = P.t[k];
    }
}

// srgb_to_linear (nerf/utils.py:52-53) in double, rounded once
__device__ __forceinline__ float bt_srgb_to_linear(float x) {
    const double v = (double)x;
    return (float)(v < 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4));
}

template <int DT> __device__ __forceinline__ float bt_pixel(const void *__restrict__ images, size_t i);
template <> __device__ __forceinline__ float bt_pixel<FOC_F32>(const void *__restrict__ images, size_t i) { return reinterpret_cast<const float *>(images)[i]; }
template <> __device__ __forceinline__ float bt_pixel<FOC_F16>(const void *__restrict__ images, size_t i) { return (float)reinterpret_cast<const _Float16 *>(images)[i]; }
template <> __device__ __forceinline__ float bt_pixel<FOC_U8>(const void *__restrict__ images, size_t i) { return (float)reinterpret_cast<const uint8_t *>(images)[i] / 255.0f; }

struct BtSample {
    const void *images;
    const float *poses;
    const int32_t *order;
    int64_t *step;
    const int64_t *inds_coarse;
    int64_t *inds;
    float *rays_o, *rays_d, *bg_color, *gt_rgb;
    int32_t *view;
    uint32_t *ws;
    uint64_t seed;
    BtCamera K;
    uint32_t V, H, W, C, N, random_bg, linear;
};

template <int DT> __global__ void __launch_bounds__(BT_THREADS) k_batch_sample(BtSample a) {
    const uint64_t step = (uint64_t)*a.step;                                   // before anything else: the last workgroup will change it
    uint32_t v = (uint32_t)a.order[step % a.V];
    v = v < a.V ? v : v % a.V;                                                 // a permutation never gets here; never read outside `images`
    const BtPose P = bt_load_pose(a.poses + (size_t)v * 16);
    const uint32_t HW = a.H * a.W;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32), s0 = (uint32_t)step, s1 = (uint32_t)(step >> 32);
    const bool blend = a.C == 4, rnd = blend && a.random_bg;

    for (uint32_t r = blockIdx.x * BT_THREADS + threadIdx.x; r < a.N; r += gridDim.x * BT_THREADS) {
        const Philox4 q = philox4x32_10(r, s0, s1, 0u, k0, k1);
        uint32_t row, col, pix;
        if (a.inds_coarse) {                                                   // nerf/utils.py:104-110
            const uint32_t c = (uint32_t)a.inds_coarse[r] & (BT_CELLS * BT_CELLS - 1);
            const float sx = (float)a.H / 128.0f, sy = (float)a.W / 128.0f;
            const int ri = (int)((float)(c / BT_CELLS) * sx + bt_uniform(q.w[1]) * sx);
            const int ci = (int)((float)(c % BT_CELLS) * sy + bt_uniform(q.w[2]) * sy);
            row = (uint32_t)(ri < (int)a.H - 1 ? ri : (int)a.H - 1);
            col = (uint32_t)(ci < (int)a.W - 1 ? ci : (int)a.W - 1);
            pix = row * a.W + col;
        } else {
            pix = (uint32_t)(((uint64_t)q.w[0] * HW) >> 32);                   // < H * W
            row = pix / a.W;
            col = pix % a.W;
        }
        a.inds[r] = (int64_t)pix;
        float o[3], d[3];
        bt_ray(a.K, P, row, col, o, d);

        float bg[3] = {1.0f, 1.0f, 1.0f};
        if (rnd) {
            const Philox4 b = philox4x32_10(r, s0, s1, 1u, k0, k1);
            bg[0] = bt_uniform(b.w[0]); bg[1] = bt_uniform(b.w[1]); bg[2] = bt_uniform(b.w[2]);
        }
        const size_t at = ((size_t)v * HW + pix) * a.C;
        float rgb[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            rgb[k] = bt_pixel<DT>(a.images, at + k);
            if (a.linear) rgb[k] = bt_srgb_to_linear(rgb[k]);
        }
        if (blend) {                                                           // nerf/utils.py:856
            const float al = bt_pixel<DT>(a.images, at + 3), om = 1.0f - al;
#pragma unroll
            for (int k = 0; k < 3; k++) rgb[k] = rgb[k] * al + bg[k] * om;
        }
        const size_t r3 = (size_t)r * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            a.rays_o[r3 + k] = o[k];
            a.rays_d[r3 + k] = d[k];
            a.bg_color[r3 + k] = bg[k];
            a.gt_rgb[r3 + k] = rgb[k];
        }
    }

    __syncthreads();                                                           // every lane's read of `step` has landed
    if (threadIdx.x == 0 && atomicAdd(&a.ws[0], 1u) == gridDim.x - 1) {        // everybody has read `step`: nobody reads it after this
        a.ws[0] = 0;
        *a.step = (int64_t)(step + 1);
        a.view[0] = (int32_t)v;
    }
}

__global__ void __launch_bounds__(BT_THREADS) k_view_rays(const float *__restrict__ pose, BtCamera K, uint32_t H, uint32_t W, float *__restrict__ rays_o,
                                                          float *__restrict__ rays_d) {
    const BtPose P = bt_load_pose(pose);
    const uint32_t HW = H * W;
    for (uint32_t p = blockIdx.x * BT_THREADS + threadIdx.x; p < HW; p += gridDim.x * BT_THREADS) {
        float o[3], d[3];
        bt_ray(K, P, p / W, p % W, o, d);
        const size_t p3 = (size_t)p * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            rays_o[p3 + k] = o[k];
            rays_d[p3 + k] = d[k];
        }
    }
}

// ---------------------------------------------------------------- the loss
struct PlArgs {
    const void *pred;
    const float *gt;
    float *error_map;
    const int32_t *view;
    const int64_t *inds_coarse;
    float *ray_loss, *grad, *loss;
    uint32_t *ws;
    uint32_t N, V, huber;
    float delta, n3;                                                           // n3 = float(3 N)
};

template <int DT> __global__ void __launch_bounds__(BT_THREADS) k_photo_loss(PlArgs a) {
    __shared__ double s_sum[BT_THREADS];
    const uint32_t tid = threadIdx.x;
    float *map_row = nullptr;
    if (a.error_map) {
        const uint32_t v = (uint32_t)a.view[0];
        if (v < a.V) map_row = a.error_map + (size_t)v * (BT_CELLS * BT_CELLS);
    }
    const float half_delta = 0.5f * a.delta;
    double acc = 0.0;
    for (uint32_t r = blockIdx.x * BT_THREADS + tid; r < a.N; r += gridDim.x * BT_THREADS) {
        const size_t r3 = (size_t)r * 3;
        float l[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float d = bt_pixel<DT>(a.pred, r3 + k) - a.gt[r3 + k];
            float g;
            if (!a.huber) {
                l[k] = d * d;
                g = 2.0f * d;
            } else if (fabsf(d) <= a.delta) {                                  // torch.nn.HuberLoss
                l[k] = 0.5f * (d * d);
                g = d;
            } else {
                l[k] = a.delta * (fabsf(d) - half_delta);
                g = d < 0.0f ? -a.delta : a.delta;
            }
            a.grad[r3 + k] = g / a.n3;
        }
        const float rl = ((l[0] + l[1]) + l[2]) / 3.0f;
        a.ray_loss[r] = rl;
        if (map_row) {                                                         // distinct cells (a draw without replacement): no atomics
            const uint32_t c = (uint32_t)a.inds_coarse[r] & (BT_CELLS * BT_CELLS - 1);
            map_row[c] = 0.1f * map_row[c] + 0.9f * rl;
        }
        acc += (double)rl;                                                     // this lane's rays in index order
    }
    s_sum[tid] = acc;
    __syncthreads();
#pragma unroll
    for (uint32_t s = BT_THREADS / 2; s > 0; s >>= 1) {                        // a fixed tree
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    unsigned long long *slots = reinterpret_cast<unsigned long long *>(a.ws + 32);
    __hip_atomic_store(&slots[blockIdx.x], (unsigned long long)__double_as_longlong(s_sum[0]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();                                                           // the slot is out before this workgroup's ticket is taken
    if (atomicAdd(&a.ws[0], 1u) != gridDim.x - 1) return;
    __threadfence();
    double total = 0.0;
    for (uint32_t b = 0; b < gridDim.x; b++)
        total += __longlong_as_double((long long)__hip_atomic_load(&slots[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    a.loss[0] = (float)(total / (double)a.N);
    a.ws[0] = 0;
}

// ---------------------------------------------------------------- host side
static_assert(128 % 8 == 0 && PL_WS_BYTES == 128 + 8 * FOC_PHOTO_LOSS_MAX_WGS, "the slots are 8-byte aligned behind the ticket line");

extern "C" {

uint64_t foc_batch_workspace_bytes(void) { return BT_WS_BYTES; }
uint64_t foc_photo_loss_workspace_bytes(void) { return PL_WS_BYTES; }

int foc_philox4x32_10(const uint32_t *ctr, const uint32_t *key, uint32_t *out) {      // the kernels' own function, on the host
    FOC_REQUIRE(ctr && key && out, FOC_E_INVALID, "philox4x32_10: null pointer");
    const Philox4 q = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
    for (int k = 0; k < 4; k++) out[k] = q.w[k];
    return FOC_OK;
}

static int bt_check_camera(const char *who, uint32_t H, uint32_t W, float fx, float fy, float cx, float cy) {
    FOC_REQUIRE(H >= 1 && W >= 1 && (uint64_t)H * W <= (1ull << 30), FOC_E_INVALID, "%s: H * W must be 1 .. 2^30 pixels (got %u x %u)", who, H, W);
    FOC_REQUIRE(std::isfinite(fx) && std::isfinite(fy) && std::isfinite(cx) && std::isfinite(cy) && fx != 0.0f && fy != 0.0f, FOC_E_INVALID,
                "%s: intrinsics must be finite, fx and fy not zero (got %g %g %g %g)", who, fx, fy, cx, cy);
    return FOC_OK;
}

int foc_batch_sample(const void *images, int image_dtype, uint32_t V, uint32_t H, uint32_t W, uint32_t C, const float *poses, float fx, float fy,
                     float cx, float cy, const int32_t *order, int64_t *step, uint64_t seed, uint32_t N, const int64_t *inds_coarse, int random_bg,
                     int linear, int64_t *inds, float *rays_o, float *rays_d, float *bg_color, float *gt_rgb, int32_t *view, void *workspace,
                     uint64_t workspace_bytes, uint32_t workgroups, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FOC_REQUIRE(images && poses && order && step && inds && rays_o && rays_d && bg_color && gt_rgb && view && workspace, FOC_E_INVALID,
                "batch_sample: null pointer");
    FOC_REQUIRE(C == 3 || C == 4, FOC_E_INVALID, "batch_sample: C must be 3 or 4 (got %u)", C);
    FOC_REQUIRE(image_dtype == FOC_F32 || image_dtype == FOC_F16 || image_dtype == FOC_U8, FOC_E_DTYPE,
                "batch_sample: image dtype must be FOC_F32, FOC_F16 or FOC_U8 (got %d)", image_dtype);
    FOC_REQUIRE(N >= 1, FOC_E_INVALID, "batch_sample: N must be >= 1");
    if (int rc = bt_check_camera("batch_sample", H, W, fx, fy, cx, cy)) return rc;
    FOC_REQUIRE(V >= 1, FOC_E_INVALID, "batch_sample: V must be >= 1");
    FOC_REQUIRE((((uintptr_t)workspace) & 3) == 0 && workspace_bytes >= BT_WS_BYTES, FOC_E_INVALID,
                "batch_sample: workspace of %llu bytes, foc_batch_workspace_bytes asks for %d (4-byte aligned)", (unsigned long long)workspace_bytes, BT_WS_BYTES);
    FOC_REQUIRE(workgroups <= BT_MAX_WGS, FOC_E_INVALID, "batch_sample: at most %d workgroups (got %u)", BT_MAX_WGS, workgroups);
    BtSample a{};
    a.images = images; a.poses = poses; a.order = order; a.step = step; a.inds_coarse = inds_coarse; a.inds = inds;
    a.rays_o = rays_o; a.rays_d = rays_d; a.bg_color = bg_color; a.gt_rgb = gt_rgb; a.view = view;
    a.ws = reinterpret_cast<uint32_t *>(workspace);
    a.seed = seed; a.K = BtCamera{fx, fy, cx, cy};
    a.V = V; a.H = H; a.W = W; a.C = C; a.N = N; a.random_bg = random_bg ? 1u : 0u; a.linear = linear ? 1u : 0u;
    const uint32_t wgs = workgroups ? workgroups : foc_grid_1d(N, BT_THREADS, BT_MAX_WGS);
    FocDeviceGuard foc_guard_(stream_, images);
    if (image_dtype == FOC_F32) hipLaunchKernelGGL(k_batch_sample<FOC_F32>, dim3(wgs), dim3(BT_THREADS), 0, stream, a);
    else if (image_dtype == FOC_F16) hipLaunchKernelGGL(k_batch_sample<FOC_F16>, dim3(wgs), dim3(BT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(k_batch_sample<FOC_U8>, dim3(wgs), dim3(BT_THREADS), 0, stream, a);
    FOC_CHECK_LAUNCH("batch_sample");
    return FOC_OK;
}

int foc_view_rays(const float *pose, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, float *rays_o, float *rays_d, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FOC_REQUIRE(pose && rays_o && rays_d, FOC_E_INVALID, "view_rays: null pointer");
    if (int rc = bt_check_camera("view_rays", H, W, fx, fy, cx, cy)) return rc;
    FocDeviceGuard foc_guard_(stream_, pose);
    hipLaunchKernelGGL(k_view_rays, dim3(foc_grid_1d((uint64_t)H * W, BT_THREADS)), dim3(BT_THREADS), 0, stream, pose, BtCamera{fx, fy, cx, cy}, H, W, rays_o,
                       rays_d);
    FOC_CHECK_LAUNCH("view_rays");
    return FOC_OK;
}

int foc_photo_loss(const void *pred, int pred_dtype, const float *gt, uint32_t N, int kind, float delta, float *error_map, uint32_t V, const int32_t *view,
                   const int64_t *inds_coarse, float *ray_loss, float *grad, float *loss, void *workspace, uint64_t workspace_bytes, void *stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    FOC_REQUIRE(pred && gt && ray_loss && grad && loss && workspace, FOC_E_INVALID, "photo_loss: null pointer");
    FOC_REQUIRE(pred_dtype == FOC_F32 || pred_dtype == FOC_F16, FOC_E_DTYPE, "photo_loss: pred dtype must be FOC_F32 or FOC_F16 (got %d)", pred_dtype);
    FOC_REQUIRE(kind == FOC_LOSS_MSE || kind == FOC_LOSS_HUBER, FOC_E_INVALID, "photo_loss: kind must be FOC_LOSS_MSE or FOC_LOSS_HUBER (got %d)", kind);
    FOC_REQUIRE(kind != FOC_LOSS_HUBER || (std::isfinite(delta) && delta > 0.0f), FOC_E_INVALID, "photo_loss: Huber's delta must be finite and > 0 (got %g)", delta);
    FOC_REQUIRE(N >= 1 && N <= (1u << 30), FOC_E_INVALID, "photo_loss: N must be 1 .. 2^30 (got %u)", N);
    if (error_map) {
        FOC_REQUIRE(view && inds_coarse, FOC_E_INVALID, "photo_loss: null pointer (an error map comes with view and inds_coarse)");
        FOC_REQUIRE(V >= 1, FOC_E_INVALID, "photo_loss: V must be >= 1");
    }
    FOC_REQUIRE((((uintptr_t)workspace) & 7) == 0 && workspace_bytes >= PL_WS_BYTES, FOC_E_INVALID,
                "photo_loss: workspace of %llu bytes, foc_photo_loss_workspace_bytes asks for %d (8-byte aligned)", (unsigned long long)workspace_bytes, PL_WS_BYTES);
    PlArgs a{};
    a.pred = pred; a.gt = gt; a.error_map = error_map; a.view = view; a.inds_coarse = inds_coarse;
    a.ray_loss = ray_loss; a.grad = grad; a.loss = loss; a.ws = reinterpret_cast<uint32_t *>(workspace);
    a.N = N; a.V = V; a.huber = kind == FOC_LOSS_HUBER ? 1u : 0u; a.delta = delta; a.n3 = (float)(3.0 * (double)N);
    const uint32_t wgs = foc_grid_1d(N, BT_THREADS, PL_MAX_WGS);
    FocDeviceGuard foc_guard_(stream_, pred);
    if (pred_dtype == FOC_F32) hipLaunchKernelGGL(k_photo_loss<FOC_F32>, dim3(wgs), dim3(BT_THREADS), 0, stream, a);
    else hipLaunchKernelGGL(k_photo_loss<FOC_F16>, dim3(wgs), dim3(BT_THREADS), 0, stream, a);
    FOC_CHECK_LAUNCH("photo_loss");
    return FOC_OK;
}

} // extern "C"
