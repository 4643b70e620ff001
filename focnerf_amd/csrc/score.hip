// score.hip — PSNR and SSIM of a combined view against its ground truth, for every background, on the device (no reference binding:
// COMBINED.py:295-378 copies the float image to the host, quantises it with numpy and runs forty scipy.ndimage.gaussian_filter calls per
// view in float64).
//
//   foc_score_quantize   the alpha threshold, the background fill and the truncating 8-bit quantisation of process_images_with_background
//                        (:353-366), for prediction, ground truth and depth; one thread per (background, pixel), 4-byte stores
//   foc_score_view       per (16 x 16 tile, background) one workgroup: tile plus halo of both byte images in LDS (borders reflected while
//                        loading), per colour channel the horizontal then the vertical pass of the separable Gaussian over the five
//                        moments x, y, x^2, y^2, xy of byte / 255.0, the SSIM expression of ssim_channel (:315-332) per pixel, all in
//                        float64; partial sums of the SSIM maps and of the squared byte differences to the workspace; a second kernel
//                        adds the partials in a fixed order. No atomics: the same bits on every run, in both deterministic modes.
//
// LDS per workgroup at the largest radius (12): 2 x 40 x 40 x 4 B of pixels, 5 x 40 x 16 x 8 B of row-filtered moments, 2 KiB for the
// table of byte / 255.0 (one correctly rounded division per entry instead of one per tap) = 40.2 KiB, four workgroups per CU. Lanes
// walk rows of both buffers, so consecutive lanes read consecutive words; only the table look-up can meet a bank conflict.
#include <cmath>
#include "common.h"

#define SC_TILE 16                               // output pixels per tile side: 256 threads, one pixel each in the vertical pass
#define SC_MAX_RADIUS 12
#define SC_SIDE (SC_TILE + 2 * SC_MAX_RADIUS)    // 40: tile plus halo
#define SC_MAX_BG 8
#define SC_MAX_PIXELS (1ull << 30)

struct ScBgs { float v[SC_MAX_BG]; };
struct ScTaps { double w[SC_MAX_RADIUS + 1]; };  // w[j]: the tap at distance j from the centre (the filter is symmetric)
struct ScPartial { unsigned long long sse; double ssim[3]; };

// ---------------------------------------------------------------- quantise
// uint8(trunc(x * 255.0f)): one float32 multiply, truncation toward zero — numpy's (img * 255).astype(np.uint8) for x in [0, 1]
__device__ __forceinline__ uint32_t sc_byte(float x) { return (uint32_t)(int)(x * 255.0f) & 255u; }
// a pixel below the alpha threshold takes the background; alpha becomes 1
__device__ __forceinline__ uint32_t sc_pixel(float4 p, float bg) {
    const bool masked = p.w < 0.5f;
    const float r = masked ? bg : p.x, g = masked ? bg : p.y, b = masked ? bg : p.z;
    return sc_byte(r) | (sc_byte(g) << 8) | (sc_byte(b) << 16) | (sc_byte(1.0f) << 24);
}

__global__ void __launch_bounds__(256) k_score_quantize(const float4 *__restrict__ image4, const float *__restrict__ depth, const float4 *__restrict__ gt,
                                                        ScBgs bgs, uint32_t N, uint32_t B, uint32_t *__restrict__ pred_u8, uint32_t *__restrict__ gt_u8,
                                                        uint8_t *__restrict__ depth_u8) {
    const uint64_t total = (uint64_t)N * B;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint32_t b = (uint32_t)(i / N), n = (uint32_t)(i - (uint64_t)b * N);
        float bg = bgs.v[0];
#pragma unroll
        for (uint32_t k = 1; k < SC_MAX_BG; k++) bg = b == k ? bgs.v[k] : bg;
        pred_u8[i] = sc_pixel(image4[i], bg);
        gt_u8[i] = sc_pixel(gt[n], bg);
        if (b == 0 && depth_u8) depth_u8[n] = (uint8_t)sc_byte(depth[n]);
    }
}

// ---------------------------------------------------------------- SSIM and SSE of one tile
// scipy's mode='reflect' (d c b a | a b c d), for any offset and any n >= 1
__device__ __forceinline__ uint32_t sc_reflect(int64_t i, int64_t n) {
    int64_t m = i % (2 * n);
    if (m < 0) m += 2 * n;
    return (uint32_t)(m < n ? m : 2 * n - 1 - m);
}

__device__ __forceinline__ double sc_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ unsigned long long sc_wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (unsigned long long)__shfl_xor((long long)v, o, 64);
    return v;
}

__global__ void __launch_bounds__(256) k_score_view(const uint32_t *__restrict__ pred_u8, const uint32_t *__restrict__ gt_u8, uint32_t H, uint32_t W,
                                                    uint32_t tiles_x, uint32_t n_tiles, uint32_t R, ScTaps taps, double C1, double C2,
                                                    ScPartial *__restrict__ partial) {
    __shared__ uint32_t sp[SC_SIDE * SC_SIDE], sg[SC_SIDE * SC_SIDE];
    __shared__ double hb[5][SC_SIDE * SC_TILE];
    __shared__ double lut[256];
    __shared__ double sw[SC_MAX_RADIUS + 1];
    __shared__ double red_d[4][3];
    __shared__ unsigned long long red_u[4];

    const uint32_t tid = threadIdx.x, b = blockIdx.y, tile = blockIdx.x;
    const uint32_t ty0 = (tile / tiles_x) * SC_TILE, tx0 = (tile % tiles_x) * SC_TILE;
    const uint32_t S = SC_TILE + 2 * R;                                     // side of tile plus halo
    const uint64_t image = (uint64_t)b * H * W;

    lut[tid] = (double)tid / 255.0;
    if (tid <= SC_MAX_RADIUS) sw[tid] = tid <= R ? taps.w[tid] : 0.0;
    for (uint32_t i = tid; i < S * S; i += 256) {
        const uint32_t ry = i / S, rx = i - ry * S;
        const uint32_t y = sc_reflect((int64_t)ty0 + ry - R, H), x = sc_reflect((int64_t)tx0 + rx - R, W);
        const uint64_t at = image + (uint64_t)y * W + x;
        sp[i] = pred_u8[at];
        sg[i] = gt_u8[at];
    }
    __syncthreads();

    const uint32_t tx = tid & (SC_TILE - 1), ty = tid / SC_TILE;
    const bool valid = ty0 + ty < H && tx0 + tx < W;
    unsigned long long sse = 0;
    if (valid) {
        const uint32_t p = sp[(ty + R) * S + tx + R], g = sg[(ty + R) * S + tx + R];
#pragma unroll
        for (uint32_t c = 0; c < 4; c++) {
            const int d = (int)((p >> (8 * c)) & 255u) - (int)((g >> (8 * c)) & 255u);
            sse += (unsigned long long)(d * d);
        }
    }

    double ssim[3];
#pragma unroll 1
    for (uint32_t c = 0; c < 3; c++) {
        const uint32_t shift = 8 * c;
        // horizontal pass: the S rows of the region, the tile's 16 columns
        for (uint32_t i = tid; i < S * SC_TILE; i += 256) {
            const uint32_t at = (i / SC_TILE) * S + (i & (SC_TILE - 1)) + R;
            const double x0 = lut[(sp[at] >> shift) & 255u], y0 = lut[(sg[at] >> shift) & 255u];
            const double w0 = sw[0];
            double ax = w0 * x0, ay = w0 * y0, axx = w0 * (x0 * x0), ayy = w0 * (y0 * y0), axy = w0 * (x0 * y0);
            for (uint32_t j = 1; j <= R; j++) {
                const double w = sw[j];
                const double xp = lut[(sp[at + j] >> shift) & 255u], xm = lut[(sp[at - j] >> shift) & 255u];
                const double yp = lut[(sg[at + j] >> shift) & 255u], ym = lut[(sg[at - j] >> shift) & 255u];
                ax = fma(w, xp + xm, ax);
                ay = fma(w, yp + ym, ay);
                axx = fma(w, xp * xp + xm * xm, axx);
                ayy = fma(w, yp * yp + ym * ym, ayy);
                axy = fma(w, xp * yp + xm * ym, axy);
            }
            hb[0][i] = ax; hb[1][i] = ay; hb[2][i] = axx; hb[3][i] = ayy; hb[4][i] = axy;
        }
        __syncthreads();
        // vertical pass and the SSIM expression at this thread's pixel
        double m[5];
        const uint32_t at = (ty + R) * SC_TILE + tx;
#pragma unroll
        for (uint32_t q = 0; q < 5; q++) {
            double a = sw[0] * hb[q][at];
            for (uint32_t j = 1; j <= R; j++) a = fma(sw[j], hb[q][at + j * SC_TILE] + hb[q][at - j * SC_TILE], a);
            m[q] = a;
        }
        const double mu1 = m[0], mu2 = m[1];
        const double s1 = m[2] - mu1 * mu1, s2 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
        const double num = (2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2);
        const double den = (mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2);
        ssim[c] = valid ? num / den : 0.0;
        __syncthreads();                                                     // hb is rewritten by the next channel
    }

    // the workgroup's sums: lanes by butterfly, then the four waves in order
    const uint32_t lane = tid & 63, wv = tid >> 6;
    const unsigned long long wsse = sc_wave_sum_u64(sse);
    const double w0 = sc_wave_sum_d(ssim[0]), w1 = sc_wave_sum_d(ssim[1]), w2 = sc_wave_sum_d(ssim[2]);
    if (lane == 0) { red_u[wv] = wsse; red_d[wv][0] = w0; red_d[wv][1] = w1; red_d[wv][2] = w2; }
    __syncthreads();
    if (tid == 0) {
        ScPartial out;
        out.sse = ((red_u[0] + red_u[1]) + red_u[2]) + red_u[3];
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) out.ssim[c] = ((red_d[0][c] + red_d[1][c]) + red_d[2][c]) + red_d[3][c];
        partial[(uint64_t)b * n_tiles + tile] = out;
    }
}

// one workgroup per background: thread t adds tiles t, t + 256, ... in that order, then the 256 sums meet in a fixed tree
__global__ void __launch_bounds__(256) k_score_finish(const ScPartial *__restrict__ partial, uint32_t n_tiles, double n_pixels, double *__restrict__ out) {
    __shared__ double red_d[4][3];
    __shared__ unsigned long long red_u[4];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    unsigned long long sse = 0;
    double s[3] = {0.0, 0.0, 0.0};
    for (uint32_t t = tid; t < n_tiles; t += 256) {
        const ScPartial p = partial[(uint64_t)b * n_tiles + t];
        sse += p.sse;
        s[0] += p.ssim[0]; s[1] += p.ssim[1]; s[2] += p.ssim[2];
    }
    const uint32_t lane = tid & 63, wv = tid >> 6;
    sse = sc_wave_sum_u64(sse);
    s[0] = sc_wave_sum_d(s[0]); s[1] = sc_wave_sum_d(s[1]); s[2] = sc_wave_sum_d(s[2]);
    if (lane == 0) { red_u[wv] = sse; red_d[wv][0] = s[0]; red_d[wv][1] = s[1]; red_d[wv][2] = s[2]; }
    __syncthreads();
    if (tid == 0) {
        out[b * 4 + 0] = (double)(((red_u[0] + red_u[1]) + red_u[2]) + red_u[3]);
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) out[b * 4 + 1 + c] = (((red_d[0][c] + red_d[1][c]) + red_d[2][c]) + red_d[3][c]) / n_pixels;
    }
}

// ---------------------------------------------------------------- host side
static bool sc_dims_ok(const char *who, uint32_t H, uint32_t W, uint32_t B) {
    if (H < 1 || W < 1 || (uint64_t)H * W > SC_MAX_PIXELS) {
        foc_set_error("%s: H * W must be 1 .. 2^30 pixels (got %u x %u)", who, H, W);
        return false;
    }
    if (B < 1 || B > SC_MAX_BG) {
        foc_set_error("%s: 1 .. %d backgrounds expected (got %u)", who, SC_MAX_BG, B);
        return false;
    }
    return true;
}
static inline uint32_t sc_tiles_x(uint32_t W) { return foc_div_up(W, SC_TILE); }
static inline uint32_t sc_tiles(uint32_t H, uint32_t W) { return foc_div_up(H, SC_TILE) * sc_tiles_x(W); }

extern "C" {

uint64_t foc_score_workspace_bytes(uint32_t H, uint32_t W, uint32_t B) {
    if (!sc_dims_ok("score_workspace_bytes", H, W, B)) return 0;
    return (uint64_t)B * sc_tiles(H, W) * sizeof(ScPartial);
}

int foc_score_quantize(const float *image4, const float *depth, const float *gt, const float *bgs, uint32_t H, uint32_t W, uint32_t B, uint8_t *pred_u8,
                       uint8_t *gt_u8, uint8_t *depth_u8, void *stream) {
    FocDeviceGuard foc_guard_(stream, image4);
    FOC_REQUIRE(image4 && gt && bgs && pred_u8 && gt_u8, FOC_E_INVALID, "score_quantize: null pointer");
    FOC_REQUIRE((depth == nullptr) == (depth_u8 == nullptr), FOC_E_INVALID, "score_quantize: depth and depth_u8 come together");
    if (!sc_dims_ok("score_quantize", H, W, B)) return FOC_E_INVALID;
    FOC_REQUIRE(((((uintptr_t)image4) | ((uintptr_t)gt)) & 15) == 0 && ((((uintptr_t)pred_u8) | ((uintptr_t)gt_u8)) & 3) == 0, FOC_E_INVALID,
                "score_quantize: image4 and gt must be 16-byte aligned, pred_u8 and gt_u8 4-byte aligned");
    ScBgs bg{};
    for (uint32_t k = 0; k < B; k++) {
        FOC_REQUIRE(std::isfinite(bgs[k]), FOC_E_INVALID, "score_quantize: background %u is not finite", k);
        bg.v[k] = bgs[k];
    }
    const uint32_t N = H * W;
    hipLaunchKernelGGL(k_score_quantize, dim3(foc_grid_1d((uint64_t)N * B, 256)), dim3(256), 0, (hipStream_t)stream, reinterpret_cast<const float4 *>(image4), depth,
                       reinterpret_cast<const float4 *>(gt), bg, N, B, reinterpret_cast<uint32_t *>(pred_u8), reinterpret_cast<uint32_t *>(gt_u8), depth_u8);
    FOC_CHECK_LAUNCH("score_quantize");
    return FOC_OK;
}

int foc_score_view(const uint8_t *pred_u8, const uint8_t *gt_u8, uint32_t H, uint32_t W, uint32_t B, const double *taps, uint32_t radius, double C1, double C2,
                   double *out, void *workspace, uint64_t workspace_bytes, void *stream) {
    FocDeviceGuard foc_guard_(stream, pred_u8);
    FOC_REQUIRE(pred_u8 && gt_u8 && taps && out && workspace, FOC_E_INVALID, "score_view: null pointer");
    if (!sc_dims_ok("score_view", H, W, B)) return FOC_E_INVALID;
    FOC_REQUIRE(radius <= SC_MAX_RADIUS, FOC_E_INVALID, "score_view: radius must not exceed %d (got %u)", SC_MAX_RADIUS, radius);
    ScTaps T{};
    for (uint32_t j = 0; j <= radius; j++) {
        FOC_REQUIRE(std::isfinite(taps[radius + j]) && taps[radius + j] == taps[radius - j], FOC_E_INVALID, "score_view: the 2 * radius + 1 taps must be finite and symmetric");
        T.w[j] = taps[radius + j];
    }
    FOC_REQUIRE(std::isfinite(C1) && std::isfinite(C2) && C1 >= 0 && C2 >= 0, FOC_E_INVALID, "score_view: C1 and C2 must be finite and >= 0");
    FOC_REQUIRE(workspace_bytes >= foc_score_workspace_bytes(H, W, B), FOC_E_INVALID, "score_view: workspace of %llu bytes, foc_score_workspace_bytes(%u, %u, %u) asks for %llu",
                (unsigned long long)workspace_bytes, H, W, B, (unsigned long long)foc_score_workspace_bytes(H, W, B));
    FOC_REQUIRE(((((uintptr_t)workspace) | ((uintptr_t)out)) & 7) == 0 && ((((uintptr_t)pred_u8) | ((uintptr_t)gt_u8)) & 3) == 0, FOC_E_INVALID,
                "score_view: workspace and out must be 8-byte aligned, pred_u8 and gt_u8 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_tiles = sc_tiles(H, W);
    ScPartial *partial = reinterpret_cast<ScPartial *>(workspace);
    hipLaunchKernelGGL(k_score_view, dim3(n_tiles, B), dim3(256), 0, st, reinterpret_cast<const uint32_t *>(pred_u8), reinterpret_cast<const uint32_t *>(gt_u8), H, W,
                       sc_tiles_x(W), n_tiles, radius, T, C1, C2, partial);
    FOC_CHECK_LAUNCH("score_view");
    hipLaunchKernelGGL(k_score_finish, dim3(B), dim3(256), 0, st, partial, n_tiles, (double)((uint64_t)H * W), out);
    FOC_CHECK_LAUNCH("score_view");
    return FOC_OK;
}

} // extern "C"
