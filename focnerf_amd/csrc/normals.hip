// normals.hip — surface normals from the density field in one launch: n = -grad(sigma) / |grad(sigma)| per sample, from the hash grid's
// position derivative and the sigma network's input gradient (foc_field_normals, include/focnerf.h). Shape served: fp16 table, D 3, C 2,
// L 16, hash gridtype, align_corners off, linear interpolation; sigma network 32 -> 64 (x 1, 2, 3) -> 16 with ReLU, raw = h[0].
//
// A wave takes tiles of 32 samples. Lane (c, h) — c = lane & 31 the sample, h = lane >> 5 — owns the EIGHT levels 8 kc + 4 h + i
// (kc = 0, 1; i = 0..3) of sample c: exactly the halves its B fragment of the layer-0 MFMA holds (mlp_common.h ld_planar8), so the two
// lane halves share the encoder's work and nothing is exchanged before the MLP.
//   encode    per owned level: ge_cell / ge_rows3 / ge_corner (ge_common.h), eight 4-byte gathers; the 2 features with ge_forward_one's
//             arithmetic, and the 6 derivatives dy_dx[l, d, c] from the SAME eight values (ge_forward_one re-gathers them).
//   forward   the sigma network's MFMA chain in k_nerf_infer's order on the forward image of stage_weights_fwd: sigma = expf(half(h[0])) has
//             the bits of foc_nerf_field_inference on foc_grid_encode_forward's planes. The post-ReLU fragments of every layer stay in registers.
//   backward  gradient of raw = h[0]: delta of the last hidden layer = gate * W_out[0, :] (row 0 of the forward image, exact), then per
//             hidden matrix one 64 x 64 MFMA product on the transposed image of stage_weights_bwd, rounded to half and gated (relu_gate);
//             grad_enc = W0^T delta_0 on a transposed image of W0 whose rows are permuted so that lane (c, h) receives the 16 features of
//             ITS eight levels in accumulator registers 8 kc + 2 i + ch.
//   contract  grad_raw[d] = sum over the lane's 16 (level, channel) of grad_enc * dy_dx, fmaf in (kc, i, ch) order from 0; the two lane halves
//             meet in one addition (half 0 + half 1).
//   normalise m = max |g_d|; zero or not finite -> n = 0; else u = g / m, n = -u / sqrt(u . u); n <- rot9 n (fmaf from the product of column 0);
//             normal_rgb = fmaf(0.5, n, 0.5).
//
// Where the 96 derivatives live between the encode and the contraction: in registers, fp32, 48 per lane (the lane split halves candidate
// (b) of the design notes). No LDS tile, no second gather walk.
//
// ROUNDING POINTS (the reference's bounds, tests/normal_ref.py, are counted from this list)
//   position in cell, corner weights, features : fp32, ge_forward_one's order; each feature rounded to half ONCE (the encoder's output bits)
//   dy_dx                                       : fp32, never rounded to half: per axis 4 terms fmaf(w (vr - vl), 1, acc), w = (scale w_a) w_b in fp32,
//                                                 vr - vl exact (two halves)
//   forward activations                         : fp32 MFMA sums, rounded to half once per layer, then ReLU (k_nerf_infer)
//   deltas                                      : last hidden layer: a half weight, exact; below it fp32 MFMA sums rounded to half once per layer, then gated
//   grad_enc                                    : the fp32 MFMA sum, NOT rounded to half; written as fp32 [M, 32] (feature 2 l + c) when asked for
//   contraction, normalisation, rotation        : fp32
// Out of range (a coordinate outside [0, 1]): features and derivatives are zero, every gate is closed: grad_enc = 0, grad_raw = 0, n = 0,
// normal_rgb = 0.5 (and rot9 n = 0), sigma = exp(0) as the inference kernel gives it.
// No atomics, no host synchronisation, nothing order-dependent: the same bits on every run, whichever outputs are asked for.
#include "mlp_common.h"
#include "ge_common.h"
#include "unit_normal.h"

#define FN_LEVELS 16

struct FnLevelsLds {                 // per-level facts of the launch, staged once per workgroup: a lane reads the eight levels it owns
    float scale[FN_LEVELS];
    uint32_t resolution[FN_LEVELS], off0[FN_LEVELS], size[FN_LEVELS];
};

// Feature (column of W0) that row `r` of the 32-row grad_enc tile stands for: lane half h = (r >> 2) & 1 holds the row in accumulator
// register reg = (r & 3) + 4 (r >> 3) (acc_row's inverse), and wants feature 8 h + reg (levels 4 h .. 4 h + 3) in registers 0..7,
// 16 + 8 h + (reg - 8) (levels 8 + 4 h ..) in registers 8..15.
__device__ __forceinline__ uint32_t fn_row_feature(uint32_t r) {
    const uint32_t h = (r >> 2) & 1u, reg = (r & 3u) + 4u * (r >> 3);
    return reg < 8u ? 8u * h + reg : 16u + 8u * h + (reg - 8u);
}

// grad_enc image: fragment kc, lane (r, h), element j = W0[chain_k(kc, h, j)][fn_row_feature(r)] (k = the hidden neuron, chained order)
__device__ void fn_stage_dx(const _Float16 *__restrict__ W0, _Float16 *lds) {
    for (uint32_t idx = threadIdx.x; idx < 4u * 64u; idx += MLP_BLOCK) {
        const uint32_t kc = idx >> 6, lane = idx & 63u, r = lane & 31u, h = lane >> 5;
        const uint32_t f = fn_row_feature(r);
        h8 v;
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = W0[(size_t)chain_k((int)kc, (int)h, j) * 32 + f];
        *reinterpret_cast<h8 *>(lds + (size_t)kc * 512 + lane * 8) = v;
    }
}

// One owned level of one sample: the two features (fp32, before their rounding) and dy[d][c].
__device__ __forceinline__ void fn_encode_level(const float (&x)[3], const __half *__restrict__ table, uint32_t size, float scale, uint32_t resolution,
                                                float (&feat)[2], float (&dy)[3][2]) {
    const GeDimCT<3> dim;
    float pos[3], pos_deriv[3];
    uint32_t pos_grid[3], rows[8];
    ge_cell(dim, x, scale, false, 0u, pos_grid, pos, pos_deriv);
    ge_rows3(pos_grid, size, resolution, 0u, false, rows);
    float vals[8][2], ws[8];
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) GeVec<__half, 2>::ld(table + (uint64_t)rows[idx] * 2, vals[idx]);
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) {
        float w = 1;
        uint32_t pgl[3];
        ge_corner(dim, idx, pos, pos_grid, w, pgl);
        ws[idx] = w;
    }
    feat[0] = feat[1] = 0.0f;
#pragma unroll
    for (uint32_t idx = 0; idx < 8; idx++) {
#pragma unroll
        for (uint32_t c = 0; c < 2; c++) feat[c] = fmaf(ws[idx], vals[idx][c], feat[c]);
    }
#pragma unroll
    for (uint32_t gd = 0; gd < 3; gd++) {
        float rg[2] = {0.0f, 0.0f};
#pragma unroll
        for (uint32_t idx = 0; idx < 4; idx++) {
            float w = scale;
            uint32_t pgl[3];
            ge_corner(dim, idx, pos, pos_grid, w, pgl, gd);
            const uint32_t lo = (idx & ((1u << gd) - 1u)) | ((idx >> gd) << (gd + 1u)), hi = lo | (1u << gd);   // the corner pair along gd
#pragma unroll
            for (uint32_t c = 0; c < 2; c++) rg[c] = fmaf(w * (vals[hi][c] - vals[lo][c]), pos_deriv[gd], rg[c]);
        }
        dy[gd][0] = rg[0]; dy[gd][1] = rg[1];
    }
}

template <int NLS>
__global__ void __launch_bounds__(MLP_BLOCK, 2) k_field_normals(const float *__restrict__ xn, uint32_t M, const __half *__restrict__ emb,
                                                                const uint32_t *__restrict__ offsets, GeLevels lv, const _Float16 *__restrict__ w_sigma,
                                                                const float *__restrict__ rot9, float *__restrict__ sigma_out, float *__restrict__ grad_raw,
                                                                float *__restrict__ normal_rgb, float *__restrict__ grad_enc) {
    constexpr int HIDDEN = 64, MT = 2, KC = 4, KS0 = 2;
    constexpr uint32_t FS = MT * KS0 + (NLS - 1) * MT * KC + KC;          // forward image: layer 0 | hidden | out
    constexpr uint32_t FB = MT + (NLS - 1) * MT * KC;                     // backward image: out (not read here) | hidden
    extern __shared__ __attribute__((aligned(16))) _Float16 lds[];
    _Float16 *ldsF = lds, *ldsB = lds + (size_t)FS * 512, *ldsX = ldsB + (size_t)FB * 512;
    FnLevelsLds *lvl = reinterpret_cast<FnLevelsLds *>(ldsX + (size_t)KC * 512);
    stage_weights_fwd<HIDDEN>(w_sigma, ldsF, 32, NLS);
    stage_weights_bwd<HIDDEN>(w_sigma, ldsB, 32, NLS, false);
    fn_stage_dx(w_sigma, ldsX);
    if (threadIdx.x < FN_LEVELS) {
        const uint32_t l = threadIdx.x, o0 = offsets[l];
        lvl->scale[l] = lv.scale[l]; lvl->resolution[l] = lv.resolution[l]; lvl->off0[l] = o0; lvl->size[l] = offsets[l + 1] - o0;
    }
    __syncthreads();

    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = lane & 31, h = lane >> 5;
    const uint32_t n_tiles = (M + 31u) / 32u;
    float R[9];
    if (rot9) {
#pragma unroll
        for (int i = 0; i < 9; i++) R[i] = rot9[i];
    }
    for (uint32_t tile = blockIdx.x * MLP_WAVES + wave; tile < n_tiles; tile += gridDim.x * MLP_WAVES) {
        const uint64_t row_raw = (uint64_t)tile * 32 + c;
        const uint32_t row = (uint32_t)min(row_raw, (uint64_t)M - 1);     // ragged last tile: computed on the last row, dropped at the stores
        float x[3];
        const bool oob = ge_load_point(GeDimCT<3>(), xn, row, x);
        // ---- encode: the lane's eight levels
        h8 xb[KS0];
        float dy[KS0][4][3][2];
#pragma unroll
        for (int kc = 0; kc < KS0; kc++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float feat[2] = {0.0f, 0.0f};
#pragma unroll
                for (int d = 0; d < 3; d++) dy[kc][i][d][0] = dy[kc][i][d][1] = 0.0f;
                if (!oob) {
                    const uint32_t l = 8u * kc + 4u * h + i;
                    fn_encode_level(x, emb + (uint64_t)lvl->off0[l] * 2, lvl->size[l], lvl->scale[l], lvl->resolution[l], feat, dy[kc][i]);
                }
                xb[kc][2 * i] = foc_f2h(feat[0]);
                xb[kc][2 * i + 1] = foc_f2h(feat[1]);
            }
        // ---- sigma network forward, k_nerf_infer's order; the post-ReLU fragments of every layer are kept for the gates
        f16v acc[MT], o;
        h8 act[NLS][KC];
#pragma unroll
        for (int mt = 0; mt < MT; mt++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[mt][e] = 0.0f;
#pragma unroll
        for (int kc = 0; kc < KS0; kc++)
#pragma unroll
            for (int mt = 0; mt < MT; mt++) acc[mt] = mfma16(ld_frag(ldsF, mt * KS0 + kc, lane), xb[kc], acc[mt]);
#pragma unroll
        for (int l = 1; l <= NLS; l++) {
#pragma unroll
            for (int kc = 0; kc < KC; kc++) act[l - 1][kc] = acc_to_frag<true>(acc[kc >> 1], kc & 1);
            if (l < NLS) {
                const uint32_t fbase = MT * KS0 + (l - 1) * MT * KC;
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[mt][e] = 0.0f;
#pragma unroll
                for (int kc = 0; kc < KC; kc++)
#pragma unroll
                    for (int mt = 0; mt < MT; mt++) acc[mt] = mfma16(ld_frag(ldsF, fbase + mt * KC + kc, lane), act[l - 1][kc], acc[mt]);
            } else {
#pragma unroll
                for (int e = 0; e < 16; e++) o[e] = 0.0f;
#pragma unroll
                for (int kc = 0; kc < KC; kc++) o = mfma16(ld_frag(ldsF, FS - KC + kc, lane), act[l - 1][kc], o);
            }
        }
        // ---- backward of raw = h[0]: row 0 of the output matrix in chained order is lane 32 h of the forward image's output fragments
        h8 dl[KC];
#pragma unroll
        for (int kc = 0; kc < KC; kc++) dl[kc] = relu_gate(ld_frag(ldsF, FS - KC + kc, 32u * h), act[NLS - 1][kc]);
#pragma unroll
        for (int l = NLS - 2; l >= 0; l--) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++)
#pragma unroll
                for (int e = 0; e < 16; e++) acc[mt][e] = 0.0f;
#pragma unroll
            for (int kc = 0; kc < KC; kc++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++) acc[mt] = mfma16(ld_frag(ldsB, MT + l * MT * KC + mt * KC + kc, lane), dl[kc], acc[mt]);
#pragma unroll
            for (int kc = 0; kc < KC; kc++) dl[kc] = relu_gate(acc_to_frag<false>(acc[kc >> 1], kc & 1), act[l][kc]);
        }
        f16v g;
#pragma unroll
        for (int e = 0; e < 16; e++) g[e] = 0.0f;
#pragma unroll
        for (int kc = 0; kc < KC; kc++) g = mfma16(ld_frag(ldsX, kc, lane), dl[kc], g);
        // ---- contraction with the lane's derivatives; the two lane halves of a sample meet in one addition
        float gr[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kc = 0; kc < KS0; kc++)
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int ch = 0; ch < 2; ch++)
#pragma unroll
                    for (int d = 0; d < 3; d++) gr[d] = fmaf(g[8 * kc + 2 * i + ch], dy[kc][i][d][ch], gr[d]);
#pragma unroll
        for (int d = 0; d < 3; d++) gr[d] = gr[d] + __shfl_xor(gr[d], 32, 64);
        if (row_raw >= M) continue;
        if (grad_enc) {
            typedef float f4 __attribute__((ext_vector_type(4)));
            float *ge = grad_enc + row_raw * 32;
#pragma unroll
            for (int kc = 0; kc < KS0; kc++)
#pragma unroll
                for (int q = 0; q < 2; q++)
                    *reinterpret_cast<f4 *>(ge + 16 * kc + 8 * h + 4 * q) = f4{g[8 * kc + 4 * q], g[8 * kc + 4 * q + 1], g[8 * kc + 4 * q + 2], g[8 * kc + 4 * q + 3]};
        }
        if (h != 0) continue;
        if (sigma_out) sigma_out[row_raw] = expf((float)acc_to_frag<false>(o, 0)[0]);
        if (grad_raw) {
#pragma unroll
            for (int d = 0; d < 3; d++) grad_raw[row_raw * 3 + d] = gr[d];
        }
        if (normal_rgb) {
            float n[3];
            un_unit_normal(gr, n);               // unit_normal.h: the rule the point pipeline's frame kernel shares
            if (rot9) un_rotate(R, n);
#pragma unroll
            for (int d = 0; d < 3; d++) normal_rgb[row_raw * 3 + d] = fmaf(0.5f, n[d], 0.5f);
        }
    }
}

template <int NLS>
static int fn_launch(const float *xn, uint32_t M, const void *emb, const uint32_t *offsets, const GeLevels &lv, const void *w, const float *rot9, float *sigma,
                     float *grad_raw, float *normal_rgb, float *grad_enc, hipStream_t st) {
    auto kern = k_field_normals<NLS>;
    const size_t lds = (size_t)((4 + (NLS - 1) * 8 + 4) + (2 + (NLS - 1) * 8) + 4) * 1024 + sizeof(FnLevelsLds);
    const uint32_t grid = foc_persistent_grid(kern, MLP_BLOCK, lds, foc_div_up(foc_div_up(M, 32), MLP_WAVES));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(MLP_BLOCK), lds, st, xn, M, (const __half *)emb, offsets, lv, (const _Float16 *)w, rot9, sigma, grad_raw, normal_rgb,
                       grad_enc);
    FOC_CHECK_LAUNCH("foc_field_normals");
    return FOC_OK;
}

// A composited normal map out of its accumulators (foc_normal_map_finish): acc = sum_k w_k (0.5 + 0.5 n_k), W = sum_k w_k, so that
// s = 2 acc - W = sum_k w_k n_k (2 acc exact, one rounding); normal = s / |s| by un_unit_normal's rule on -s (a negation is exact); the encoded
// map on a white background is acc + (1 - W), as the renderer finishes a colour image. One pixel per lane, nothing shared.
__global__ void __launch_bounds__(256) k_normal_map_finish(const float *__restrict__ acc, const float *__restrict__ weights_sum, uint32_t N, float *__restrict__ normal,
                                                           float *__restrict__ normal_rgb) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= N) return;
    const float W = weights_sum[i], rest = 1.0f - W;
    float g[3], n[3];
#pragma unroll
    for (int d = 0; d < 3; d++) g[d] = -(2.0f * acc[(uint64_t)i * 3 + d] - W);
    un_unit_normal(g, n);
#pragma unroll
    for (int d = 0; d < 3; d++) {
        normal[(uint64_t)i * 3 + d] = n[d];
        normal_rgb[(uint64_t)i * 3 + d] = acc[(uint64_t)i * 3 + d] + rest;
    }
}

extern "C" {

int foc_normal_map_finish(const float *normal_acc, const float *weights_sum, uint32_t N, float *normal, float *normal_rgb, void *stream) {
    FocDeviceGuard foc_guard_(stream, normal_acc);
    if (N == 0) return FOC_OK;
    FOC_REQUIRE(normal_acc && weights_sum && normal && normal_rgb, FOC_E_INVALID, "foc_normal_map_finish: null pointer (normal_acc, weights_sum, normal, normal_rgb)");
    hipLaunchKernelGGL(k_normal_map_finish, dim3(foc_div_up(N, 256)), dim3(256), 0, (hipStream_t)stream, normal_acc, weights_sum, N, normal, normal_rgb);
    FOC_CHECK_LAUNCH("foc_normal_map_finish");
    return FOC_OK;
}

int foc_field_normals(const float *xn, uint32_t M, const void *embeddings, const uint32_t *offsets, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                      uint32_t gridtype, int align_corners, uint32_t interp, int dtype, const int32_t *offsets_host, const void *sigma_weights,
                      uint32_t sigma_layers, uint32_t hidden_dim, uint32_t activation, const float *rot9, float *sigma, float *grad_raw, float *normal_rgb,
                      void *grad_enc, void *stream) {
    FocDeviceGuard foc_guard_(stream, xn);
    (void)offsets_host;
    FOC_REQUIRE(D == 3, FOC_E_INVALID, "foc_field_normals: D must be 3 (got %u)", D);
    FOC_REQUIRE(C == 2, FOC_E_INVALID, "foc_field_normals: C must be 2 (got %u)", C);
    FOC_REQUIRE(L == FN_LEVELS, FOC_E_INVALID, "foc_field_normals: L must be %d (got %u)", FN_LEVELS, L);
    FOC_REQUIRE(dtype == FOC_F16, FOC_E_DTYPE, "foc_field_normals: dtype must be FOC_F16 (a half table)");
    FOC_REQUIRE(gridtype == 0, FOC_E_INVALID, "foc_field_normals: gridtype must be hash(0) (got %u)", gridtype);
    FOC_REQUIRE(!align_corners, FOC_E_INVALID, "foc_field_normals: align_corners must be off");
    FOC_REQUIRE(interp == 0, FOC_E_INVALID, "foc_field_normals: interp must be linear(0) (got %u)", interp);
    FOC_REQUIRE(H >= 1, FOC_E_INVALID, "foc_field_normals: H must be at least 1");
    FOC_REQUIRE(hidden_dim == 64, FOC_E_INVALID, "foc_field_normals: hidden_dim must be 64 (got %u)", hidden_dim);
    FOC_REQUIRE(activation == FOC_ACT_RELU, FOC_E_INVALID, "foc_field_normals: activation must be relu(0) (got %u)", activation);
    FOC_REQUIRE(sigma_layers >= 1 && sigma_layers <= 3, FOC_E_INVALID, "foc_field_normals: sigma_layers must be 1, 2 or 3 (got %u)", sigma_layers);
    FOC_REQUIRE(xn && embeddings && offsets && sigma_weights, FOC_E_INVALID, "foc_field_normals: null pointer (xn, embeddings, offsets, sigma_weights)");
    FOC_REQUIRE(((uintptr_t)embeddings & 3u) == 0 && ((uintptr_t)sigma_weights & 15u) == 0 && (!grad_enc || ((uintptr_t)grad_enc & 15u) == 0), FOC_E_INVALID,
                "foc_field_normals: embeddings must be 4-byte, sigma_weights and grad_enc 16-byte aligned");
    if (M == 0 || !(sigma || grad_raw || normal_rgb || grad_enc)) return FOC_OK;
    GeLevels lv;
    ge_make_levels(L, S, H, lv);
    hipStream_t st = (hipStream_t)stream;
    switch (sigma_layers) {
        case 1: return fn_launch<1>(xn, M, embeddings, offsets, lv, sigma_weights, rot9, sigma, grad_raw, normal_rgb, (float *)grad_enc, st);
        case 2: return fn_launch<2>(xn, M, embeddings, offsets, lv, sigma_weights, rot9, sigma, grad_raw, normal_rgb, (float *)grad_enc, st);
        default: return fn_launch<3>(xn, M, embeddings, offsets, lv, sigma_weights, rot9, sigma, grad_raw, normal_rgb, (float *)grad_enc, st);
    }
}

} // extern "C"
