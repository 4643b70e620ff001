// occrender.hip — one iteration of the occupancy-grid inference loop as ONE native call.
//
// The caller of the inference ops (legacy/nerf/renderer.py:323-372) runs, per iteration and from Python: march_rays -> the network on the
// new samples -> composite_rays -> compaction of the list of live rays. An 800 x 800 view is ~150 such iterations of ~0.17 ms of kernels
// each, and ~20 Python-level operations per iteration cost more than that to enqueue. foc_occ_render_step enqueues the whole iteration —
// nine launches — from C, on buffers the caller allocated once per view:
//
//   prepare   fill the output list with -1, reset the walkers' worklist and the compaction's block counts; zero the iteration's sample slots
//             (the reference's torch.zeros, raymarching.py:334-336) where the march kernel of this burst length does not write them all itself
//   march     foc_march_rays_two_phase (raymarching.hip). One sample per ray: first visits per lane, then the walkers densely packed. A burst
//             of several samples (focnerf_amd/renderer.py marches 8 per ray and iteration): one ray per lane, the wave's samples staged in
//             LDS and written as whole runs, SAMPLE-MAJOR ([n_step][n_alive]: the 64 rows of an encoder / network wave are 64 neighbouring
//             rays at one burst slot), t re-derived after every sample so that the samples are those of one-sample iterations. The
//             positions leave already normalised, x -> (x + bound) * (1 / (2 bound))  (gridencoder/grid.py:149 as torch evaluates it:
//             division by a scalar = multiplication by its reciprocal) — nobody but the encoder reads them here
//   encode    foc_grid_encode_forward ([L, M, 2] planes)
//   field     nerf_field_inference (the body of foc_nerf_field_inference[_pad | _pad31]: sigma net -> head -> colour net, per-sample directions)
//   composite foc_composite_compact: composite_rays in place (weights_sum, depth, image, rays_t; finished rays marked -1; a burst's samples
//             loaded at once), its waves counting their survivors and recording where rays died, then scan + ordered scatter into the output
//             list, whose tail stays -1 (march / composite skip such entries)
//
// foc_occ_render_step_normals is the same iteration with the surface normal of every sample (normals.hip, foc_field_normals on the march's
// normalised positions) as the composite's payload: instead of the colour (encode and field give way to it: no planes, no colour network), or
// next to it (one composite, two payloads: raymarching.hip, composite_compact_aux). Same prepare, same march, same compaction.
//
// The live count stays on the device (`count`, one int); the caller reads it late (focnerf_amd/renderer.py) and passes an upper bound.
#include "mlp_common.h"     // host: nerf_field_inference, head_layer_pair
#include <cstdlib>

__global__ void __launch_bounds__(256) k_occ_prepare(uint32_t *__restrict__ samples, uint64_t n_sample_words, int32_t *__restrict__ list_out, uint32_t n_list,
                                                     int32_t *__restrict__ wl_count, int32_t *__restrict__ block_counts, uint32_t n_blocks) {
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_sample_words; i += stride) samples[i] = 0u;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_list; i += stride) list_out[i] = -1;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_blocks; i += stride) block_counts[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) *wl_count = 0;
}

extern "C" {


uint64_t foc_occ_render_step_scratch_bytes(uint32_t n_rays) {
    // int32[n + 4] worklist | compaction block counts int32[n / 1024 + 2], both 256-byte aligned
    const uint64_t wl = (((uint64_t)n_rays + 4) * 4 + 255) & ~(uint64_t)255;
    const uint64_t cc = (((uint64_t)n_rays / 1024 + 2) * 4 + 255) & ~(uint64_t)255;
    return wl + cc;
}

// The colour input's layout is (obj_feat, input_pad, pad31), as nerf_field_inference takes it (mlp_common.h). pad31
// (foc_occ_render_step_pad31): input_pad is column 31 of the 32-wide row; else column 47 of the object-conditioned 48-wide row
// (foc_occ_render_step_pad), and with input_pad 0 that is the plain step (foc_occ_render_step), which nothing below can refuse.
// normals_mode (foc_occ_render_step_normals; 0 for the three steps above, which pass no normal_rgb / normal_acc): FOC_OCC_NORMALS_ONLY puts
// foc_field_normals where encode + field stand — its sigma has their bits — and composites the encoded normal as the colour, into normal_acc;
// FOC_OCC_NORMALS_AUX runs it next to them, for the normal alone, and one composite accumulates both payloads (composite_compact_aux).
static int occ_render_step(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                           float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                           uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                           float *samples, void *planes, float *sigma, float *rgb,
                           const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                           const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                           const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags, int32_t *deaths,
                           uint32_t deaths_base, uint32_t deaths_len, float input_pad, bool pad31, uint32_t normals_mode, float *normal_rgb, float *normal_acc,
                           void *stream) {
    FocDeviceGuard foc_guard_(stream, rays_alive);
    FOC_REQUIRE(count, FOC_E_INVALID, "occ_render_step: null pointer");
    // refused before anything is enqueued
    if (pad31) FOC_REQUIRE(!obj_feat, FOC_E_INVALID, "occ_render_step_pad31: input_pad is column 31 of the 32-wide colour input, obj_feat must be NULL");
    else FOC_REQUIRE(obj_feat || input_pad == 0.0f, FOC_E_INVALID, "occ_render_step_pad: input_pad is column 47 of the 48-wide colour input, it needs obj_feat");
    FOC_REQUIRE(input_pad == 0.0f || head_layer_pair(sigma_layers, color_layers), FOC_E_INVALID,
                "occ_render_step_%s: a pad needs (sigma_layers, color_layers) in (1,2), (1,3), (2,2), (2,3), (3,3) (got %u, %u)", pad31 ? "pad31" : "pad", sigma_layers,
                color_layers);
    const bool only = normals_mode == FOC_OCC_NORMALS_ONLY, aux = normals_mode == FOC_OCC_NORMALS_AUX;
    if (normals_mode) FOC_REQUIRE(normal_rgb && normal_acc, FOC_E_INVALID, "occ_render_step_normals: null pointer (normal_rgb, normal_acc)");
    hipStream_t st = (hipStream_t)stream;
    if (n_alive == 0) return foc_zero_async(count, sizeof(int32_t), st) == hipSuccess ? FOC_OK : FOC_E_LAUNCH;
    FOC_REQUIRE(rays_alive && rays_alive_out && rays_t && rays_o && rays_d && grid && fars && noises && samples && sigma && embeddings && offsets && sigma_weights &&
                weights_sum && depth && scratch, FOC_E_INVALID, "occ_render_step: null pointer");
    // what the colour step needs and the normals alone do not: the encoder's planes, the colour network, its output and its image
    FOC_REQUIRE(only || (planes && rgb && color_weights && image), FOC_E_INVALID,
                normals_mode ? "occ_render_step_normals: null pointer (planes, rgb, color_weights, image: FOC_OCC_NORMALS_AUX runs the colour step)"
                             : "occ_render_step: null pointer");
    FOC_REQUIRE(n_step >= 1 && n_step <= 16, FOC_E_INVALID, "occ_render_step: n_step must be in [1, 16] (got %u)", n_step);
    const uint64_t M = (uint64_t)n_alive * n_step;
    FOC_REQUIRE(M < (1ull << 31), FOC_E_INVALID, "occ_render_step: n_alive * n_step must fit 31 bits");
    if (normals_mode) {
        // foc_field_normals' own refusals (normals.hip), asked for an empty list: it launches nothing, and none of them can surface at the first piece
        const int refused = foc_field_normals(samples, 0, embeddings, reinterpret_cast<const uint32_t *>(offsets), 3, 2, L, S, base_res, 0, 0, 0, FOC_F16, offsets_host,
                                              sigma_weights, sigma_layers, 64, activation, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
        if (refused) return refused;
    }
    float *xyzs = samples, *dirs = samples + 3 * M, *deltas = samples + 6 * M;
    int32_t *worklist = reinterpret_cast<int32_t *>(scratch);
    int32_t *compact_scratch = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(scratch) + ((((uint64_t)n_alive + 4) * 4 + 255) & ~(uint64_t)255));
    // the sample slots are zeroed here (the reference's torch.zeros) unless the march kernel of this burst length writes every one of them itself
    int march_flags = 1 | ((flags & 1u) ? 2 : 0);          // normalised positions; flags bit 0: t re-derived after every sample (focnerf.h)
    // sample-major sample arrays ([n_step][n_alive]) where the march kernel of this call can write them (FOC_OCC_SAMPLE_MAJOR=0: ray-major)
    const int sample_major = (n_step > 1 && foc_opt(FOC_OPT_OCC_SAMPLE_MAJOR) != 0 && foc_march_rays_two_phase_sample_major(n_alive, n_step, march_flags)) ? 1 : 0;
    if (sample_major) march_flags |= 4;
    const uint64_t to_zero = foc_march_rays_two_phase_fills(n_step, march_flags) ? 0 : M * 8;
    hipLaunchKernelGGL(k_occ_prepare, dim3(foc_grid_1d((to_zero > n_alive ? to_zero : n_alive) + 1, 256)), dim3(256), 0, st, reinterpret_cast<uint32_t *>(samples), to_zero,
                       rays_alive_out, n_alive, worklist, compact_scratch, n_alive / 1024 + 2);
    FOC_CHECK_LAUNCH("occ_render_step(prepare)");
    int rc = foc_march_rays_two_phase(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, xyzs, dirs, deltas,
                                      noises, worklist, march_flags, stream);
    if (rc) return rc;
    // the field in pieces of at most `piece` samples: the [L, piece, 2] planes between the encoder and the whole-field kernel (64 B per sample)
    // are bounded whatever the burst length (FOC_OCC_FIELD_PIECE, samples; default 2^23. Measured on the 800 x 800 view, 5.1 M samples per iteration:
    // one piece 18.5 ms per view, pieces of 2^21 — planes that fit the 256 MiB Infinity Cache — 19.3, of 2^20 20.0: fewer launches win)
    uint64_t piece = (uint64_t)(uint32_t)foc_opt(FOC_OPT_OCC_FIELD_PIECE);
    if (piece < 1024) piece = 1024;
    piece &= ~(uint64_t)63;
    for (uint64_t m0 = 0; m0 < M; m0 += piece) {
        const uint32_t mc = (uint32_t)(M - m0 < piece ? M - m0 : piece);
        if (!only) {
            rc = foc_grid_encode_forward(xyzs + 3 * m0, embeddings, offsets, planes, mc, 3, 2, L, S, base_res, nullptr, 0, 0, 0, FOC_F16, offsets_host, stream);
            if (rc) return rc;
            rc = nerf_field_inference(planes, 1, dirs + 3 * m0, 1, 0, mc, sigma_weights, sigma_layers, color_weights, color_layers, 64, activation, mc, sigma + m0,
                                      rgb + 3 * m0, obj_feat, input_pad, pad31, stream);
            if (rc) return rc;
        }
        if (normals_mode) {                                 // the normals' own sigma is asked for only where it is the step's sigma
            rc = foc_field_normals(xyzs + 3 * m0, mc, embeddings, reinterpret_cast<const uint32_t *>(offsets), 3, 2, L, S, base_res, 0, 0, 0, FOC_F16, offsets_host,
                                   sigma_weights, sigma_layers, 64, activation, nullptr, only ? sigma + m0 : nullptr, nullptr, normal_rgb + 3 * m0, nullptr, stream);
            if (rc) return rc;
        }
    }
    // composite marks finished rays in the INPUT list; the compaction then writes the survivors to the output list
    if (aux)
        return composite_compact_aux(n_alive, n_step, T_thresh, const_cast<int32_t *>(rays_alive), rays_t, sigma, rgb, normal_rgb, deltas, weights_sum, depth, image,
                                     normal_acc, rays_alive_out, count, compact_scratch, deaths, deaths_base, deaths_len, sample_major, stream);
    return foc_composite_compact(n_alive, n_step, T_thresh, const_cast<int32_t *>(rays_alive), rays_t, sigma, only ? normal_rgb : rgb, deltas, weights_sum, depth,
                                 only ? normal_acc : image, rays_alive_out, count, compact_scratch, deaths, deaths_base, deaths_len, sample_major, stream);
}

int foc_occ_render_step(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                        float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                        uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                        float *samples /* [n_alive*n_step*8]: normalised xyzs | dirs | deltas */,
                        void *planes /* fp16 [L, n_alive*n_step, 2] */, float *sigma, float *rgb,
                        const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                        const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                        const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags, int32_t *deaths, uint32_t deaths_base,
                        uint32_t deaths_len, void *stream) {
    return occ_render_step(n_alive, n_step, rays_alive, rays_alive_out, count, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, noises,
                           samples, planes, sigma, rgb, embeddings, offsets, offsets_host, L, S, base_res, sigma_weights, sigma_layers, color_weights, color_layers,
                           activation, obj_feat, T_thresh, weights_sum, depth, image, scratch, flags, deaths, deaths_base, deaths_len, 0.0f, false, 0u, nullptr, nullptr, stream);
}

int foc_occ_render_step_pad31(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                              float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                              uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                              float *samples, void *planes, float *sigma, float *rgb,
                              const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                              const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                              const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags, int32_t *deaths,
                              uint32_t deaths_base, uint32_t deaths_len, float input_pad, void *stream) {
    return occ_render_step(n_alive, n_step, rays_alive, rays_alive_out, count, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, noises,
                           samples, planes, sigma, rgb, embeddings, offsets, offsets_host, L, S, base_res, sigma_weights, sigma_layers, color_weights, color_layers,
                           activation, obj_feat, T_thresh, weights_sum, depth, image, scratch, flags, deaths, deaths_base, deaths_len, input_pad, true, 0u, nullptr, nullptr, stream);
}

int foc_occ_render_step_pad(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                            float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                            uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                            float *samples, void *planes, float *sigma, float *rgb,
                            const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                            const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                            const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags, int32_t *deaths,
                            uint32_t deaths_base, uint32_t deaths_len, float input_pad, void *stream) {
    return occ_render_step(n_alive, n_step, rays_alive, rays_alive_out, count, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, noises,
                           samples, planes, sigma, rgb, embeddings, offsets, offsets_host, L, S, base_res, sigma_weights, sigma_layers, color_weights, color_layers,
                           activation, obj_feat, T_thresh, weights_sum, depth, image, scratch, flags, deaths, deaths_base, deaths_len, input_pad, false, 0u, nullptr, nullptr, stream);
}

int foc_occ_render_step_normals(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                                float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                                float *samples, void *planes, float *sigma, float *rgb,
                                const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                                const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                                const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags, int32_t *deaths,
                                uint32_t deaths_base, uint32_t deaths_len, float input_pad, uint32_t pad_column, uint32_t mode, float *normal_rgb, float *normal_acc,
                                void *stream) {
    // its own refusals; the pad's (which colour input takes it, which layer pairs) are the twins', inside occ_render_step
    FOC_REQUIRE(mode == FOC_OCC_NORMALS_ONLY || mode == FOC_OCC_NORMALS_AUX, FOC_E_INVALID,
                "occ_render_step_normals: mode must be FOC_OCC_NORMALS_ONLY (1) or FOC_OCC_NORMALS_AUX (2) (got %u)", mode);
    FOC_REQUIRE(pad_column == 0 || pad_column == 31 || pad_column == 47, FOC_E_INVALID, "occ_render_step_normals: pad_column must be 0, 31 or 47 (got %u)", pad_column);
    FOC_REQUIRE(pad_column != 0 || input_pad == 0.0f, FOC_E_INVALID, "occ_render_step_normals: pad_column 0 is the colour input without a pad, input_pad must be 0");
    FOC_REQUIRE(pad_column != 47 || obj_feat, FOC_E_INVALID, "occ_render_step_normals: pad_column 47 is the last column of the 48-wide colour input, it needs obj_feat");
    return occ_render_step(n_alive, n_step, rays_alive, rays_alive_out, count, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, noises,
                           samples, planes, sigma, rgb, embeddings, offsets, offsets_host, L, S, base_res, sigma_weights, sigma_layers, color_weights, color_layers,
                           activation, obj_feat, T_thresh, weights_sum, depth, image, scratch, flags, deaths, deaths_base, deaths_len, input_pad, pad_column == 31, mode,
                           normal_rgb, normal_acc, stream);
}

} // extern "C"
