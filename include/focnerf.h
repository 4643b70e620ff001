/*
 * focnerf.h — C ABI of libfocnerf_hip.so, the MI355X (gfx950) implementation of
 * FOCNeRF's volume-rendering hot path.
 *
 * Every entry point replaces one function of the reference's four pybind11
 * extension modules (_raymarching, _gridencoder, _freqencoder, _ffmlp); the
 * reference declaration each one stands in for is cited as file:line into the
 * reference tree. Argument ORDER and MEANING follow the reference binding; the
 * differences are mechanical:
 *   - at::Tensor  -> raw device pointer (caller owns every buffer, as in the
 *                    reference where the Python wrapper allocates all outputs);
 *   - an explicit dtype code where the reference dispatches on scalar_type();
 *   - a trailing hipStream_t passed as void* (the reference launches on the
 *     legacy default stream; here the caller picks the stream);
 *   - int return: 0 = ok, non-zero = FOC_E_* with foc_last_error() holding a
 *     thread-local message (the reference raises through TORCH_CHECK /
 *     std::runtime_error, or checks nothing at all in _raymarching).
 * No function allocates, frees or synchronises; all are safe to capture into a
 * hipGraph. All pointers are DEVICE pointers unless stated otherwise.
 */
#ifndef FOCNERF_H
#define FOCNERF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FOC_OK            0
#define FOC_E_INVALID     1   /* bad argument (null pointer, unsupported C/D/hidden_dim, ...) */
#define FOC_E_DTYPE       2   /* unsupported dtype code for this entry point */
#define FOC_E_LAUNCH      3   /* hipGetLastError() != hipSuccess after a launch */

#define FOC_F32 0
#define FOC_F16 1

/* ABI version of this header; bump on any change of a signature OR of a buffer contract.
 *   2 (round 5): the workspace of foc_ffmlp_backward / _backward_planar / foc_color_head_backward is
 *     [fp32 image of the weight blob | one slot of partial weight-gradient tiles per workgroup of the launch], written without a zero fill and
 *     tens of MB large — a buffer sized by version 1's blob formula (input_dim, hidden_dim, num_layers -> ~50 KB) is too small: size it with
 *     foc_ffmlp_backward_workspace_bytes(); the three entry points take the buffer's size (`workspace_bytes`) and refuse one that is too small;
 *     FocOccTrainNode carries `mlp_workspace_bytes`; foc_field_forward_train is new; input_dim up to 256 at every hidden width. */
#define FOC_ABI_VERSION 2
int         foc_abi_version(void);
/* Thread-local message of the last non-zero return on this thread ("" if none). */
const char *foc_last_error(void);
/* Tuning / test switches (csrc/common.h FocOpt): ints with a default, initialised once from the environment variable of the same name
 * (FOC_MLP_BWD_FUSED, FOC_FIELD_FWD_FUSED, FOC_GB_MERGE_MAX_RES, FOC_GB_FACTORED, FOC_GB_TAIL_SPLIT, FOC_GRID_FUSE_SMALL, FOC_GRID_PAIRS, FOC_GRID_FAST,
 * FOC_MARCH_SERIAL, FOC_MARCH_RAYS_ROW_MAX, FOC_OCC_MARCH_FORM, FOC_OCC_SAMPLE_MAJOR, FOC_OCC_FIELD_PIECE, FOC_DETERMINISTIC — INTEGRATION.md has
 * the table) and changeable at run time; no entry point reads the environment per call. Unknown name: FOC_E_INVALID. */
int foc_set_option(const char *name, int value);
int foc_get_option(const char *name, int *value);
/* Deterministic mode — the option FOC_DETERMINISTIC (default 0; Python: focnerf_amd.use_deterministic / is_deterministic / deterministic).
 *
 * DEFAULT MODE. Five kinds of sums take their addends in arrival order, so their last bits change from run to run:
 *   (a) foc_grid_encode_backward_binned[_counted], fp16 tables: inside a 32768-record chunk the sum is exact (2^24-scaled 64-bit
 *       integers) and order-free, but the chunks of one (level, 8192-row segment) slot are each rounded to half and meet in
 *       grad_embeddings through half2 atomics; fp32 tables: the in-chunk sum is a double LDS atomic, the chunks meet through fp32 atomics;
 *   (b) foc_background_backward: fp32 atomics into grad_embeddings;
 *   (c) foc_grid_update_apply: a double atomic across workgroups feeds the mean, hence the threshold and the bitfield;
 *   (d) foc_ffmlp_backward[_planar] on its two-kernel path (hidden_dim 128 / 256, the general activations, FOC_MLP_BWD_FUSED=0): the
 *       split-K weight gradient is summed with fp32 atomics;
 *   (e) foc_grid_encode_backward (every shape, D = 4 / 5 included) and foc_grad_total_variation: scattered float atomics.
 * Every other entry point gives the same bits on every run in both modes: the forwards and all inference, the marches and their
 * ray order, the composites and tails, the fused MLP / colour-head backward (per-workgroup slots, summed in workgroup order),
 * the background weight gradient, the occupancy-grid scatter (atomicMax).
 *
 * FOC_DETERMINISTIC != 0. Same GPU model, same build, same inputs and same option values give the same bits. Per entry point:
 *   (a) fp16 tables: DETERMINISTIC FORM. Per table element the result is the exact integer sum S of ALL the slot's 2^24-scaled addends,
 *       converted once: (_Float16)(float)((double)S / 2^24), NaN for a row that received an inf / NaN addend. A slot with one chunk
 *       gives the default mode's bits; a slot with several is rounded once instead of once per chunk and once per add. The chunks
 *       meet through 64-bit integer atomics into a zeroed int64 image in the workspace (1; integer addition is associative) or through
 *       per-chunk planes summed in a second pass (2, kept for measurements) — identical results. The addends depend on the sample
 *       ORDER where runs of equal cells are merged (levels up to FOC_GB_MERGE_MAX_RES), never on timing; with FOC_GB_MERGE_MAX_RES=0
 *       the result is also independent of the order of the samples.
 *       fp32 tables: REFUSED (FOC_E_INVALID).
 *   (b) DETERMINISTIC FORM: the addends are summed as 2^-40-scaled 64-bit integers in a row table in the workspace (exact from 2^-16
 *       up, |sum| < 2^23), each row's total is added to grad_embeddings once; at most 2^26 rays per call.
 *   (c) DETERMINISTIC FORM: per-workgroup partial sums, added in workgroup order.
 *   (d) DETERMINISTIC FORM: at most 32 split-K workgroups per layer, each with its own image of the blob, summed in workgroup order.
 *   (e) REFUSED (FOC_E_INVALID before any launch; the message names the entry point and FOC_DETERMINISTIC).
 * The *_workspace_bytes functions of (a) - (d) return a size that is sufficient under the CURRENT value of the option (larger when it
 * is set); the entry points check `workspace_bytes` against the value they run under and refuse a buffer that is too small. The mode
 * adds no host synchronisation and no memset node: it captures into a HIP graph like the default mode. */
/* Which device an entry point makes current for its call (host-only query of the rule, for tests): a non-null stream's device; for the
 * NULL stream (it exists on every device) the device the first pointer argument lives on; else the current device. -1 = unknown. */
int foc_guard_pick_device(int stream_is_null, int stream_device, int pointer_device, int current_device);
/* Compiled-for architecture string, e.g. "gfx950". */
const char *foc_arch(void);

/* ------------------------------------------------------------------------- *
 * _raymarching  (reference: raymarching/src/raymarching.h:7-18,
 *                           raymarching/src/bindings.cpp:5-19)
 * All floating tensors are fp32 (the reference's wrappers force fp32 with
 * custom_fwd(cast_inputs=torch.float32), raymarching/raymarching.py:21).
 * ------------------------------------------------------------------------- */

/* raymarching.cu:92-156  near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars)
 * rays_o/rays_d [N,3], aabb [6] (device), nears/fars [N]. Miss -> both FLT_MAX. */
int foc_near_far_from_aabb(const float *rays_o, const float *rays_d, const float *aabb,
                           uint32_t N, float min_near, float *nears, float *fars, void *stream);

/* raymarching.cu:163-209  sph_from_ray(rays_o, rays_d, radius, N, coords)   coords [N,2] */
int foc_sph_from_ray(const float *rays_o, const float *rays_d, float radius, uint32_t N,
                     float *coords, void *stream);

/* raymarching.cu:214-232  morton3D(coords int32 [N,3], N, indices int32 [N]) */
int foc_morton3D(const int32_t *coords, uint32_t N, int32_t *indices, void *stream);

/* raymarching.cu:237-260  morton3D_invert(indices int32 [N], N, coords int32 [N,3]) */
int foc_morton3D_invert(const int32_t *indices, uint32_t N, int32_t *coords, void *stream);

/* raymarching.cu:267-300  packbits(grid fp32 [N*8], N, density_thresh, bitfield u8 [N]) */
int foc_packbits(const float *grid, uint32_t N, float density_thresh, uint8_t *bitfield, void *stream);

/* raymarching.cu:311-490  march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps,
 *                                          N, C, H, M, nears, fars, xyzs, dirs, deltas, rays, counter, noises)
 * grid u8 [C*H^3/8]; xyzs/dirs [M,3], deltas [M,2] (caller pre-zeroed, raymarching.py:205-207);
 * rays int32 [N,3] = (ray id, point offset, point count); counter int32[2] is ADDED to
 * (counter[0] += total points, counter[1] += N) exactly like the reference's atomicAdd pair
 * (raymarching.cu:405-406).
 * Order: the reference's slot order depends on atomicAdd arrival; this implementation
 * reserves slots by an exclusive scan in RAY ORDER (one of the reference's legal outcomes),
 * so the result is deterministic: rays[i] = (i, counter0_before + sum_{j<i} n_j, n_i).
 * scratch: caller-owned device bytes (foc_march_rays_train_scratch_bytes): per-ray counts + scan carry, and one
 * strip of max_steps sample positions per ray, so that the occupancy walk runs once (the reference walks every ray
 * twice, raymarching.cu:357-399 and :415-479). */
int foc_march_rays_train(const float *rays_o, const float *rays_d, const uint8_t *grid,
                         float bound, float dt_gamma, uint32_t max_steps,
                         uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                         const float *nears, const float *fars,
                         float *xyzs, float *dirs, float *deltas,
                         int32_t *rays, int32_t *counter, const float *noises,
                         int32_t *scratch, void *stream);
/* Bytes of `scratch` needed by foc_march_rays_train for N rays of at most max_steps samples. */
uint64_t foc_march_rays_train_scratch_bytes(uint32_t N, uint32_t max_steps);

/* Extension (no reference binding): the same march — same rays table, counter and per-ray samples — with the sample list in the
 * layout the fused occupancy-grid training path consumes (focnerf_amd/occtrain.py; the caller-side expressions of
 * legacy/nerf/renderer.py:288-300 and nerf/network_ff.py:51-68 folded into the emit pass):
 *   enc_in [M,3] fp32  = (xyz + bound) * (1 / (2 bound)), the encoder's [0,1] coordinates as torch evaluates (x + bound) / (2 bound);
 *   sh_rows [M,16] fp16 = the degree-4 SH values of each sample's ray direction (k-chunk 0 of the colour network's input);
 *   deltas [M,2] as above. No `dirs`. EVERY row of the three arrays is written (rays that do not fit the list and the rows behind the
 *   last ray receive zeros): the caller does not pre-zero them. pad_align > 0: the rows behind the last ray are zeroed only up to the
 *   next multiple of pad_align above counter[0] (a caller that cuts the list there, raymarching.py:223-229, reads nothing beyond).
 *   aabb != NULL: nears / fars [N] are OUTPUTS — the slab test of foc_near_far_from_aabb(aabb [6], min_near) is done by the count pass
 *   (same expressions, same bits); aabb == NULL: they are inputs as in foc_march_rays_train. */
int foc_march_rays_train_field(const float *rays_o, const float *rays_d, const uint8_t *grid,
                               float bound, float dt_gamma, uint32_t max_steps,
                               uint32_t N, uint32_t C, uint32_t H, uint32_t M,
                               float *nears, float *fars,
                               float *enc_in, void *sh_rows, float *deltas,
                               int32_t *rays, int32_t *counter, const float *noises,
                               int32_t *scratch, uint32_t pad_align, const float *aabb, float min_near, void *stream);

/* raymarching.cu:500-588  composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh,
 *                                                      weights_sum, depth, image) */
int foc_composite_rays_train_forward(const float *sigmas, const float *rgbs, const float *deltas,
                                     const int32_t *rays, uint32_t M, uint32_t N, float T_thresh,
                                     float *weights_sum, float *depth, float *image, void *stream);

/* raymarching.cu:601-693  composite_rays_train_backward(grad_weights_sum, grad_image, sigmas, rgbs,
 *       deltas, rays, weights_sum, image, M, N, T_thresh, grad_sigmas, grad_rgbs)
 * grad_sigmas/grad_rgbs must be pre-zeroed by the caller (raymarching.py:283-284). grad_weights_sum may be NULL (= all zero: the loss
 * does not read weights_sum). */
int foc_composite_rays_train_backward(const float *grad_weights_sum, const float *grad_image,
                                      const float *sigmas, const float *rgbs, const float *deltas,
                                      const int32_t *rays, const float *weights_sum, const float *image,
                                      uint32_t M, uint32_t N, float T_thresh,
                                      float *grad_sigmas, float *grad_rgbs, void *stream);

/* raymarching.cu:700-815  march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound,
 *       dt_gamma, max_steps, C, H, grid, nears, fars, xyzs, dirs, deltas, noises)
 * xyzs/dirs/deltas [n_alive*n_step (+pad), 3|3|2] pre-zeroed (raymarching.py:334-336). */
int foc_march_rays(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t,
                   const float *rays_o, const float *rays_d, float bound, float dt_gamma,
                   uint32_t max_steps, uint32_t C, uint32_t H, const uint8_t *grid,
                   const float *nears, const float *fars,
                   float *xyzs, float *dirs, float *deltas, const float *noises, void *stream);

/* raymarching.cu:818-914  composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs,
 *       deltas, weights_sum, depth, image)   — in place; rays_alive[n] = -1 marks a finished ray. */
int foc_composite_rays(uint32_t n_alive, uint32_t n_step, float T_thresh,
                       int32_t *rays_alive, float *rays_t,
                       const float *sigmas, const float *rgbs, const float *deltas,
                       float *weights_sum, float *depth, float *image, void *stream);

/* Device-side compaction of rays_alive (replaces the reference caller's
 * `rays_alive = rays_alive[rays_alive >= 0]`, legacy/nerf/renderer.py:363, which costs a
 * host sync per marching iteration). Writes the surviving ids, in order, to `out` and
 * their count to n_out[0] (device int32). Extension: no reference binding. */
/* One iteration of the inference loop of legacy/nerf/renderer.py:323-372 as one call (csrc/occrender.hip): zero the iteration's sample
 * slots -> march_rays (two phases: first visits, then the walkers densely packed) -> x to [0,1] -> grid_encode_forward ([L,M,2] planes) ->
 * foc_nerf_field_inference (per-sample directions) -> composite_rays (in place; finished rays marked -1 in rays_alive) -> ordered
 * compaction into rays_alive_out, whose entries behind the count are -1. M = n_alive * n_step.
 * n_alive may be an UPPER BOUND of the live count: entries of rays_alive that are -1 are skipped by every stage, so a caller may read
 * `count` (device int) late. samples: fp32 [M * 8] = positions [M,3] (in the encoder's [0,1] coordinates) | dirs [M,3] | deltas [M,2]; planes fp16
 * [L, min(M, piece), 2]: the field is evaluated in pieces of FOC_OCC_FIELD_PIECE samples (default 2^23), whose planes stay in the Infinity Cache;
 * sigma [M], rgb [M,3] fp32; scratch: foc_occ_render_step_scratch_bytes(n_alive of the FIRST iteration) bytes. Hash grid D = 3, C = 2,
 * fp16 table (embeddings), linear interpolation; networks as foc_nerf_field_inference (hidden 64; obj_feat may be NULL). density_scale 1.
 * flags bit 0: the march re-derives t after every sample (foc_march_rays_two_phase, flag bit 1): a caller that marches n_step samples where
 * the reference's loop would march one per iteration sets it and receives the reference's samples. deaths / deaths_base / deaths_len: as
 * foc_composite_compact. */
/* The two building blocks of the step that have no reference counterpart, usable on their own:
 * foc_march_rays_two_phase — foc_march_rays with the same arguments and results (bit for bit), as two launches: first visits per lane, then
 *   the rays that met an empty cell ("walkers") compacted on a worklist and marched 16 lanes per ray (one ray per lane when the list is
 *   long). scratch: int32[n_alive + 4] whose first word the caller has zeroed on this stream. `normalised` is a flag word. Bit 0: xyzs
 *   receives (x + bound) * (1 / (2 bound)), the encoder's [0,1] coordinates, instead of x. Bit 1 ("re-derive"): after every emitted sample
 *   the march continues from last_t + (t - last_t) instead of t — the value composite_rays reconstructs from deltas[:,1] and stores in
 *   rays_t for the NEXT call (raymarching.cu:871, 899). The two differ by an ulp when t - last_t is not exact in fp32 (a skip over empty
 *   space that more than doubles t), so the reference's samples depend on where its bursts end; with bit 1 a burst of k samples marches
 *   exactly what k consecutive calls with n_step = 1 would, whatever k. Bit 2 ("sample-major"): xyzs / dirs / deltas are written as
 *   [n_step][n_alive] arrays instead of [n_alive][n_step] — honoured by the staged one-ray-per-lane kernel only
 *   (foc_march_rays_two_phase_sample_major(n_alive, n_step, flags) != 0 says whether this call would); foc_composite_compact reads that
 *   layout with sample_major != 0. The 64 rows an encoder / network wave works on are then 64 neighbouring rays at one burst slot. Bursts of more than two samples (most rays meet an
 *   empty cell inside them and would be marched twice) take ONE launch instead — one ray per lane — of a kernel that collects the
 *   samples in LDS and writes ALL n_step slots of every list entry
 *   as runs of consecutive floats (zeros where the ray ended early or the entry is -1): foc_march_rays_two_phase_fills(n_step) != 0 says
 *   so, and the caller may then skip zeroing xyzs / dirs / deltas. FOC_OCC_MARCH_FORM = two | row | lane | staged overrides the choice
 *   (A/B runs, tests; "lane" = foc_march_rays' serial kernel, which needs the zeros).
 * foc_composite_compact — foc_composite_rays followed by the ordered compaction of the surviving list entries into `out` (count in n_out),
 *   the compaction's counting pass done by the composite kernel. block_counts: int32[n_alive / 1024 + 2], zeroed by the caller.
 *   deaths (may be NULL): int32[deaths_len][64] histogram in 64 slices (sum them): deaths[min(deaths_base + j, deaths_len - 1)][slice] += 1
 *   for every ray that ends at slot j of this call (no sample there, or the transmittance test after it). With deaths_base = the samples marched per ray so far, the histogram
 *   over a view tells how many rays were alive after any number of samples — what the reference's burst rule (renderer.py:337) looks at —
 *   to a caller that deals the samples over iterations differently. */
int foc_march_rays_two_phase(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, const float *rays_t, const float *rays_o,
                             const float *rays_d, float bound, float dt_gamma, uint32_t max_steps, uint32_t C, uint32_t H,
                             const uint8_t *grid, const float *nears, const float *fars, float *xyzs, float *dirs, float *deltas,
                             const float *noises, int32_t *scratch, int normalised, void *stream);
int foc_march_rays_two_phase_fills(uint32_t n_step, int flags);
int foc_march_rays_two_phase_sample_major(uint32_t n_alive, uint32_t n_step, int flags);
int foc_composite_compact(uint32_t n_alive, uint32_t n_step, float T_thresh, int32_t *rays_alive, float *rays_t,
                          const float *sigmas, const float *rgbs, const float *deltas, float *weights_sum, float *depth,
                          float *image, int32_t *out, int32_t *n_out, int32_t *block_counts, int32_t *deaths, uint32_t deaths_base,
                          uint32_t deaths_len, int sample_major, void *stream);
uint64_t foc_occ_render_step_scratch_bytes(uint32_t n_rays);
int foc_occ_render_step(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                        float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                        uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                        float *samples, void *planes, float *sigma, float *rgb,
                        const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                        const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                        const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags,
                        int32_t *deaths, uint32_t deaths_base, uint32_t deaths_len, void *stream);
/* foc_occ_render_step with input column 31 of the 32-wide colour row [SH16 | h[1:16] | input_pad] = input_pad: the field through
 * foc_nerf_field_inference_pad31 (the legacy tinycudann layout, focnerf_amd/network_tcnn_legacy.py, pad 1.0). obj_feat must be NULL;
 * input_pad != 0 needs (sigma_layers, color_layers) in (1,2), (1,3), (2,2), (2,3), (3,3); both are refused before anything is enqueued.
 * input_pad = 0: the bits of foc_occ_render_step. */
int foc_occ_render_step_pad31(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                              float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                              uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                              float *samples, void *planes, float *sigma, float *rgb,
                              const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                              const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                              const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags,
                              int32_t *deaths, uint32_t deaths_base, uint32_t deaths_len, float input_pad, void *stream);
/* foc_occ_render_step with input column 47 of the 48-wide object-conditioned colour row [SH16 | h[1:16] | obj_feat | input_pad] = input_pad:
 * the field through foc_nerf_field_inference_pad (the tinycudann layout, focnerf_amd/network_tcnn.py, pad 1.0). input_pad != 0 needs
 * obj_feat and (sigma_layers, color_layers) in (1,2), (1,3), (2,2), (2,3), (3,3); both are refused before anything is enqueued.
 * input_pad = 0: the bits of foc_occ_render_step. */
int foc_occ_render_step_pad(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                            float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                            uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                            float *samples, void *planes, float *sigma, float *rgb,
                            const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                            const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                            const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags,
                            int32_t *deaths, uint32_t deaths_base, uint32_t deaths_len, float input_pad, void *stream);
/* foc_occ_render_step with the surface normal of every sample as a payload of the composite: prepare, march and compaction are that step's,
 * foc_field_normals runs on the march's normalised positions, piece by piece (FOC_OCC_FIELD_PIECE), with rot9 NULL and no grad_raw / grad_enc.
 * Arguments as foc_occ_render_step, then:
 *   input_pad, pad_column  the colour input's constant last column, and which one: 0 (none; input_pad must be 0: foc_occ_render_step), 31
 *                          (foc_occ_render_step_pad31) or 47 (foc_occ_render_step_pad)
 *   mode                   1 = FOC_OCC_NORMALS_ONLY, 2 = FOC_OCC_NORMALS_AUX (the names the sources and this text use for the two values; the
 *                          header defines no macro for them)
 *   normal_rgb             fp32 [n_alive * n_step, 3] scratch: the encoded normal 0.5 + 0.5 n of every sample slot, laid out as rgb
 *   normal_acc             fp32 [N, 3], zeroed by the caller before a view's first call: sum_k w_k (0.5 + 0.5 n_k), accumulated as image is
 *                          (foc_normal_map_finish turns it into a normal map)
 * FOC_OCC_NORMALS_ONLY: march -> foc_field_normals (sigma and normal_rgb) -> foc_composite_compact with rgbs = normal_rgb, image = normal_acc.
 *   No encoder planes, no colour network: planes, rgb, image, color_weights and obj_feat may be NULL and are not touched. weights_sum, depth,
 *   rays_t, the output list, count and deaths are BIT-IDENTICAL to foc_occ_render_step's on the same arguments (foc_field_normals' sigma has
 *   the bits of foc_nerf_field_inference's), and normal_acc to what that step's image would be with normal_rgb for its colours.
 * FOC_OCC_NORMALS_AUX: the colour step as it is (encode, field with the given pad) plus foc_field_normals for normal_rgb alone on the same
 *   pieces, then ONE composite that accumulates both payloads with one set of weights, one stop at T_thresh and one deaths histogram.
 *   weights_sum, depth, image, rays_t, list, count and deaths are bit-identical to the colour step's, normal_acc to FOC_OCC_NORMALS_ONLY's.
 * Refused with FOC_E_INVALID before anything is enqueued, the message names the argument: mode not one of the two; pad_column not 0, 31 or 47;
 *   pad_column 0 with input_pad != 0, 31 with obj_feat, 47 without it; a non-zero pad with (sigma_layers, color_layers) outside (1,2), (1,3),
 *   (2,2), (2,3), (3,3); NULL normal_rgb / normal_acc; with n_alive > 0 a NULL pointer the mode needs (AUX: every one of the colour step's),
 *   and whatever foc_field_normals refuses (L != 16, sigma_layers outside 1..3, activation not ReLU, a misaligned sigma_weights: the level
 *   width 2, the hash gridtype, linear interpolation and hidden 64 are this step's own). */
int foc_occ_render_step_normals(uint32_t n_alive, uint32_t n_step, const int32_t *rays_alive, int32_t *rays_alive_out, int32_t *count,
                                float *rays_t, const float *rays_o, const float *rays_d, float bound, float dt_gamma, uint32_t max_steps,
                                uint32_t C, uint32_t H, const uint8_t *grid, const float *nears, const float *fars, const float *noises,
                                float *samples, void *planes, float *sigma, float *rgb,
                                const void *embeddings, const int32_t *offsets, const int32_t *offsets_host, uint32_t L, float S, uint32_t base_res,
                                const void *sigma_weights, uint32_t sigma_layers, const void *color_weights, uint32_t color_layers, uint32_t activation,
                                const void *obj_feat, float T_thresh, float *weights_sum, float *depth, float *image, void *scratch, uint32_t flags,
                                int32_t *deaths, uint32_t deaths_base, uint32_t deaths_len, float input_pad, uint32_t pad_column, uint32_t mode,
                                float *normal_rgb, float *normal_acc, void *stream);

int foc_compact_alive(const int32_t *rays_alive, uint32_t n_alive, int32_t *out, int32_t *n_out,
                      int32_t *scratch, void *stream);

/* ------------------------------------------------------------------------- *
 * _gridencoder  (reference: gridencoder/src/gridencoder.h:12-15,
 *                           gridencoder/src/bindings.cpp)
 * inputs fp32 [B,D] in [0,1]; embeddings/outputs/dy_dx/grad* share `dtype`
 * (FOC_F32 or FOC_F16 — the reference dispatches on embeddings.scalar_type(),
 * gridencoder.cu:467-470); offsets int32 [L+1] (device). D in {2,3}, C in {1,2,4,8}.
 * S = log2(per_level_scale). Per-level scale = exp2f(l*S)*H-1 is evaluated on the
 * HOST (libm) and handed to the kernel, so the integer index math does not depend on
 * a device transcendental. offsets_host: the same L+1 ints in HOST memory (needed to
 * size launches without a D2H copy); may be NULL, in which case dense-level LDS
 * fast paths are disabled.
 * ------------------------------------------------------------------------- */

/* gridencoder.cu:448-471  grid_encode_forward(inputs, embeddings, offsets, outputs, B, D, C, L, S, H,
 *                                             dy_dx?, gridtype, align_corners, interp)
 * outputs [L,B,C] (level-major, as the reference kernel writes it); dy_dx [B,L,D,C] or NULL. */
int foc_grid_encode_forward(const float *inputs, const void *embeddings, const int32_t *offsets,
                            void *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                            float S, uint32_t H, void *dy_dx, uint32_t gridtype,
                            int align_corners, uint32_t interp, int dtype,
                            const int32_t *offsets_host, void *stream);

/* Same computation, but writes outputs as [B, L*C] (what the reference's Python wrapper
 * produces with a permute+reshape copy, gridencoder/grid.py:57). Extension used by this
 * repo's wrapper to skip that copy; results are element-for-element identical. */
int foc_grid_encode_forward_bl(const float *inputs, const void *embeddings, const int32_t *offsets,
                               void *outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                               float S, uint32_t H, void *dy_dx, uint32_t gridtype,
                               int align_corners, uint32_t interp, int dtype,
                               const int32_t *offsets_host, void *stream);
/* [L,B,C] -> [B,L*C] for C * sizeof(element) = unit_bytes in {4, 8}: the permute + copy of grid.py:57 as one kernel, so that
 * the [B,L*C] result can come from the level-major forward kernel (faster than the point-major one on incoherent points). */
int foc_grid_planes_to_rows(const void *planes, void *rows, uint32_t B, uint32_t L, uint32_t unit_bytes, void *stream);
/* Host-only query (tests): the index arithmetic foc_grid_encode_forward uses for one level of an fp16, D = 3, C = 2 hash grid —
 * 2: 32-bit byte offsets with 24-bit multiplies (levels of at most 2^22 rows: every NeRF grid), 1: 32-bit byte offsets, generic
 * multiplies (up to 2^30 rows; a hashed level must have a power-of-two size), 0: the general 64-bit form (everything else). */
int foc_grid_forward_index_path(uint32_t level_rows, uint32_t resolution, uint32_t level_offset_rows);
/* [B,L*C] -> [L,B,C]: the permute + copy of grid.py:75 (the gradient on its way into the backward kernel) as one kernel. */
int foc_grid_rows_to_planes(const void *rows, void *planes, uint32_t B, uint32_t L, uint32_t unit_bytes, void *stream);

/* gridencoder.cu:473-503  grid_encode_backward(grad, inputs, embeddings, offsets, grad_embeddings,
 *       B, D, C, L, S, H, dy_dx?, grad_inputs?, gridtype, align_corners, interp)
 * grad [L,B,C]; grad_embeddings pre-zeroed (grid.py:77); grad_inputs [B,D] (dtype) or NULL.
 * grad_is_bl != 0: grad is laid out [B, L*C] instead (skips the wrapper's permute copy,
 * gridencoder/grid.py:75). */
int foc_grid_encode_backward(const void *grad, const float *inputs, const void *embeddings,
                             const int32_t *offsets, void *grad_embeddings,
                             uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             const void *dy_dx, void *grad_inputs, uint32_t gridtype,
                             int align_corners, uint32_t interp, int dtype, int grad_is_bl,
                             const int32_t *offsets_host, void *stream);

/* Same result as foc_grid_encode_backward for D = 3, C = 2 tables, computed WITHOUT scattered atomics:
 * the (row, w*grad) contributions are partitioned by 8192-row table segment and summed per segment in
 * LDS, then added to grad_embeddings with contiguous atomics. Scattered memory-side atomics cap
 * the atomic entry point at ~2x10^10 corner updates/s on MI355X; this path streams instead.
 * Order: a segment's records are summed in chunks of 32768. fp16 tables: the sum inside a chunk is exact (2^24-scaled 64-bit integers)
 * and independent of order; the chunks of a segment are rounded to half each and meet in grad_embeddings through half2 atomics in
 * arrival order, so the result repeats only to a few half ulps — unless FOC_DETERMINISTIC is set ("Deterministic mode" above: one
 * exact integer total per element, rounded once; the workspace is then larger). fp32 tables: double LDS atomics inside a chunk, fp32
 * atomics across chunks; order-dependent, and refused under FOC_DETERMINISTIC.
 * workspace: device scratch of foc_grid_encode_backward_workspace_bytes() bytes (0 = shape not
 * supported: call foc_grid_encode_backward). offsets_host (L+1 ints in HOST memory) is required.
 * Extension: no reference binding (the reference has only the atomic kernel, gridencoder.cu:248-340). */
uint64_t foc_grid_encode_backward_workspace_bytes(uint32_t B, uint32_t D, uint32_t C, uint32_t L, int dtype);
int foc_grid_encode_backward_binned(const void *grad, const float *inputs, const void *embeddings,
                                    const int32_t *offsets, void *grad_embeddings,
                                    uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                    const void *dy_dx, void *grad_inputs, uint32_t gridtype,
                                    int align_corners, uint32_t interp, int dtype, int grad_is_bl,
                                    const int32_t *offsets_host, void *workspace, uint64_t workspace_bytes,
                                    void *stream);

/* The binned pass in two halves, so that the gradient-independent one (record counts -> record ranges, which needs the
 * sample positions only) can run ahead of time: foc_grid_encode_backward_count fills the workspace header on its own;
 * foc_grid_encode_forward_counted is foc_grid_encode_forward ([L,B,C] outputs, no dy_dx; D = 3, C = 2) with that pass riding
 * along in the same launch — the forward gathers are bound by cache requests and leave the VALU idle, so the count costs
 * almost nothing there (a training forward). foc_grid_encode_backward_binned_counted then does
 * the scatter + reduce for the SAME inputs / offsets / B / dtype on the SAME workspace (nothing else may have used the
 * workspace in between; the caller orders the two calls, across streams with an event). */
int foc_grid_encode_forward_counted(const float *inputs, const void *embeddings, const int32_t *offsets, void *outputs,
                                    uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                    uint32_t gridtype, int align_corners, uint32_t interp, int dtype,
                                    const int32_t *offsets_host, void *workspace, uint64_t workspace_bytes, void *stream);
int foc_grid_encode_backward_count(const float *inputs, const int32_t *offsets, uint32_t B, uint32_t D, uint32_t C,
                                   uint32_t L, float S, uint32_t H, uint32_t gridtype, int align_corners,
                                   uint32_t interp, int dtype, const int32_t *offsets_host, void *workspace,
                                   uint64_t workspace_bytes, void *stream);
int foc_grid_encode_backward_binned_counted(const void *grad, const float *inputs, const void *embeddings,
                                            const int32_t *offsets, void *grad_embeddings,
                                            uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                            const void *dy_dx, void *grad_inputs, uint32_t gridtype,
                                            int align_corners, uint32_t interp, int dtype, int grad_is_bl,
                                            const int32_t *offsets_host, void *workspace, uint64_t workspace_bytes,
                                            void *stream);

/* gridencoder.cu:639-645  grad_total_variation(inputs, embeddings, grad, offsets, weight,
 *       B, D, C, L, S, H, gridtype, align_corners)   — inputs share `dtype` with embeddings. */
int foc_grad_total_variation(const void *inputs, const void *embeddings, void *grad,
                             const int32_t *offsets, float weight,
                             uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                             uint32_t gridtype, int align_corners, int dtype, void *stream);

/* ------------------------------------------------------------------------- *
 * _freqencoder  (reference: freqencoder/src/freqencoder.h:7,10) — fp32 only.
 * ------------------------------------------------------------------------- */

/* freqencoder.cu:97-110  freq_encode_forward(inputs [B,D], B, D, deg, C, outputs [B,C]) */
int foc_freq_encode_forward(const float *inputs, uint32_t B, uint32_t D, uint32_t deg, uint32_t C,
                            float *outputs, void *stream);
/* freqencoder.cu:113-129 freq_encode_backward(grad [B,C], outputs [B,C], B, D, deg, C, grad_inputs [B,D]) */
int foc_freq_encode_backward(const float *grad, const float *outputs, uint32_t B, uint32_t D,
                             uint32_t deg, uint32_t C, float *grad_inputs, void *stream);

/* ------------------------------------------------------------------------- *
 * _ffmlp  (reference: ffmlp/src/ffmlp.h:8-14) — fp16 storage, fp32 MFMA accumulation.
 * weights: one fp16 blob [hidden*input_dim | (num_layers-1)*hidden*hidden | 16*hidden],
 * each block row-major with the OUTPUT neuron as the row (ffmlp.cu:631-634).
 * inputs [B,input_dim], outputs [B,16] (output_dim is the padded 16), row-major.
 * Any B >= 1 is accepted (the reference kernels need a multiple of 128 and its wrapper pads with a copy,
 * ffmlp/ffmlp.py:157-159; here the ragged last tile is handled in the kernels, so no padded copy is needed);
 * hidden_dim in {16,32,64,128,256}; input_dim % 16 == 0; output_dim <= 16; num_layers (hidden layers) 1..16, at hidden_dim 256
 * 2..16. num_layers 1 is input -> hidden -> output, two matmuls (tcnn's FullyFusedMLP with one hidden layer; the reference's FFMLP
 * module asks for >= 2, ffmlp.py:115). The colour-head and whole-field entry points below keep their own layer counts.
 * activation codes follow ffmlp.py:86-93: 0 relu, 1 exponential, 2 sine, 3 sigmoid, 4 squareplus, 5 softplus, 6 none — the hidden
 * activations of ffmlp/src/utils.h:424-589, evaluated as there (fp32 function of the half-rounded sum; the backward factor from the stored
 * post-activation in half arithmetic; Sine's backward a pass-through, as the reference leaves it). Codes 1..5 take the reference's data
 * flow: foc_ffmlp_backward then needs forward_buffer and backward_buffer (the single-pass kernel and the planar / head / whole-field forms
 * serve relu|none, which is what every FOC network uses). Output activation none (FFMLP can construct no other, ffmlp.py:107-108).
 * ------------------------------------------------------------------------- */

/* ffmlp.cu:635-671  ffmlp_forward(inputs, weights, B, input_dim, output_dim, hidden_dim, num_layers,
 *       activation, output_activation, forward_buffer [num_layers,B,hidden], outputs)
 * forward_buffer may be NULL: no activations are kept (outputs are the same bits); pass NULL
 * to foc_ffmlp_backward as well and it re-evaluates them from `inputs` on chip (hidden_dim <= 64,
 * input_dim <= 64, num_layers 1..4 — the shapes of the fused backward kernel). */
int foc_ffmlp_forward(const void *inputs, const void *weights, uint32_t B, uint32_t input_dim,
                      uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                      uint32_t activation, uint32_t output_activation,
                      void *forward_buffer, void *outputs, void *stream);

/* ffmlp.cu:673-709  ffmlp_inference(..., inference_buffer [B,hidden] (unused here), outputs) */
int foc_ffmlp_inference(const void *inputs, const void *weights, uint32_t B, uint32_t input_dim,
                        uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                        uint32_t activation, uint32_t output_activation,
                        void *inference_buffer, void *outputs, void *stream);

/* ffmlp.cu:749-895  ffmlp_backward(grad [B,16], inputs, weights, forward_buffer, B, input_dim,
 *       output_dim, hidden_dim, num_layers, activation, output_activation, calc_grad_inputs,
 *       backward_buffer [num_layers,B,hidden], grad_inputs [B,input_dim], grad_weights (blob))
 * forward_buffer NULL: see foc_ffmlp_forward. backward_buffer may be NULL for the same shapes (the
 * activation gradients then never leave the chip); other shapes need both (FOC_E_INVALID otherwise).
 * workspace: device memory, foc_ffmlp_backward_workspace_bytes(input_dim, hidden_dim, num_layers) bytes, caller-owned, needs NO zero fill:
 * [fp32 image of the weight blob: the split-K sums of the two-kernel form, the object-conditioned head's finalize] followed, for the shapes
 * the single-pass kernel serves (hidden_dim <= 64, input_dim <= 64, 1..4 layers), by up to 1024 per-workgroup slots of
 * (num_layers + 1) x 4096 fp32 partial weight-gradient tiles that a second kernel sums in a fixed order (33 - 80 MB; the reference's CUTLASS
 * split-K workspace, cutlass_matmul.h:335-363, is a process-global map instead). `workspace_bytes` = the size of the caller's buffer: a
 * buffer smaller than foc_ffmlp_backward_workspace_bytes() is refused (FOC_E_INVALID) instead of being written past its end; for the colour
 * head with an object feature ask for input_dim 48 (the slots start behind a 48-wide blob image). */
int foc_ffmlp_backward(const void *grad, const void *inputs, const void *weights,
                       const void *forward_buffer, uint32_t B, uint32_t input_dim,
                       uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                       uint32_t activation, uint32_t output_activation, int calc_grad_inputs,
                       void *backward_buffer, void *grad_inputs, void *grad_weights,
                       void *workspace, uint64_t workspace_bytes, void *stream);
uint64_t foc_ffmlp_backward_workspace_bytes(uint32_t input_dim, uint32_t hidden_dim, uint32_t num_layers);

/* Planar-input forms for the encoder -> MLP pair. `inputs_planar` is [input_dim/2][B] half2 planes: exactly the
 * [L, B, C=2] tensor foc_grid_encode_forward writes (gridencoder.cu:218), consumed here without the
 * permute + copy to [B, L*C] the reference wrapper makes (grid.py:57); `grad_inputs_planar` has the same layout,
 * i.e. the [L, B, C] gradient foc_grid_encode_backward(_binned) reads (grid.py:75 builds it with another permute).
 * Semantics otherwise as foc_ffmlp_forward / foc_ffmlp_backward with forward_buffer and backward_buffer NULL
 * (same shape limits: hidden_dim <= 64, input_dim <= 64, num_layers 1..4 for the backward). */
int foc_ffmlp_forward_planar(const void *inputs_planar, const void *weights, uint32_t B, uint32_t input_dim,
                             uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                             uint32_t activation, uint32_t output_activation, void *outputs, void *stream);
int foc_ffmlp_backward_planar(const void *grad, const void *inputs_planar, const void *weights, uint32_t B,
                              uint32_t input_dim, uint32_t output_dim, uint32_t hidden_dim, uint32_t num_layers,
                              uint32_t activation, uint32_t output_activation, int calc_grad_inputs,
                              void *grad_inputs_planar, void *grad_weights, void *workspace, uint64_t workspace_bytes, void *stream);

/* Inference of the whole NeRF field per sample in one kernel (nerf/network_ff.py:51-75): sigma network on the hash-grid
 * encoding `enc` ([B,32] fp16 row-major, or the encoder's [16,B,2] planes when enc_planar), trunc_exp, degree-4 SH of the
 * direction, colour network, sigmoid. dirs [B / dir_div, 3] fp32: sample s uses direction s / dir_div (dir_div = 1 for
 * per-sample directions, = samples per ray when they are per ray). sigma [B] fp32 (may be NULL), rgb [B,3] fp32 (values
 * rounded to fp16 like the half sigmoid). Same bits as foc_ffmlp_inference -> foc_sample_head_forward -> foc_ffmlp_inference
 * -> foc_rgb_head_forward; hidden_dim 64, (sigma_layers, color_layers) in {(2,2), (2,3), (3,3)}.
 * dir_block > 0: the rows stand in the block-interleaved sample order of foc_fixed_sample (ray_block = dir_block, dir_div =
 * samples per ray): row r uses direction min((r / (dir_block*dir_div))*dir_block + r % dir_block, n_dirs - 1). dir_block = 0:
 * n_dirs is not read.
 * obj_feat (may be NULL): FOC's object-conditioned colour network, nerf/network_tcnn.py:611-640 — [16] fp16, the ENCODED object
 * feature (yolo_feat_encoder output), one vector for every sample. The colour network's input row is then
 * [SH16 | h[1:16] | obj_feat 16 | 0] (48 wide, W0 rows of 48 in color_weights); its share W0[:,31:47] . obj_feat enters as the
 * initial value of the layer-0 accumulators (fp32), nothing else changes. Needs enc_planar = 1 and ReLU. */
int foc_nerf_field_inference(const void *enc, int enc_planar, const float *dirs, uint32_t dir_div,
                             uint32_t dir_block, uint32_t n_dirs, const void *sigma_weights, uint32_t sigma_layers, const void *color_weights,
                             uint32_t color_layers, uint32_t hidden_dim, uint32_t activation, uint32_t B,
                             float *sigma, float *rgb, const void *obj_feat, void *stream);
/* foc_nerf_field_inference with the value of input column 47 of the 48-wide object-conditioned colour row (replaces
 * foc_nerf_field_inference for the tinycudann parameter layout, focnerf_amd/network_tcnn.py, whose padded input column holds 1.0 and so acts
 * as a bias): W0[:,47] * input_pad joins the per-neuron constant W0[:,31:47] . obj_feat. input_pad = 0 gives the bits of
 * foc_nerf_field_inference; input_pad != 0 needs obj_feat. (sigma_layers, color_layers) here and there: (1,2), (1,3), (2,2), (2,3), (3,3). */
int foc_nerf_field_inference_pad(const void *enc, int enc_planar, const float *dirs, uint32_t dir_div,
                                 uint32_t dir_block, uint32_t n_dirs, const void *sigma_weights, uint32_t sigma_layers, const void *color_weights,
                                 uint32_t color_layers, uint32_t hidden_dim, uint32_t activation, uint32_t B,
                                 float *sigma, float *rgb, const void *obj_feat, float input_pad, void *stream);
/* foc_nerf_field_inference with the value of input column 31 of the 32-wide colour row [SH16 | h[1:16] | input_pad] (replaces
 * foc_nerf_field_inference for the legacy tinycudann layout, focnerf_amd/network_tcnn_legacy.py: tcnn pads the 31-wide input with 1.0, a
 * bias): W0[:,31] * input_pad is the initial value of the colour layer-0 accumulators. 32-wide W0 rows; obj_feat must be NULL (a 48-wide
 * row takes its pad through foc_nerf_field_inference_pad); input_pad != 0 needs enc_planar = 1 and ReLU. input_pad = 0 gives the bits of
 * foc_nerf_field_inference. (sigma_layers, color_layers): (1,2), (1,3), (2,2), (2,3), (3,3). */
int foc_nerf_field_inference_pad31(const void *enc, int enc_planar, const float *dirs, uint32_t dir_div,
                                   uint32_t dir_block, uint32_t n_dirs, const void *sigma_weights, uint32_t sigma_layers, const void *color_weights,
                                   uint32_t color_layers, uint32_t hidden_dim, uint32_t activation, uint32_t B,
                                   float *sigma, float *rgb, const void *obj_feat, float input_pad, void *stream);

/* Surface normals from the density field, one launch: sigma, the gradient of raw = h[0] with respect to the position, and the normal
 * n = -grad / |grad| encoded as a colour, per sample (csrc/normals.hip). Extension: the reference has no such kernel; what it computes is
 * torch.autograd.grad through its encoder (dy_dx) and its MLP.
 *   xn [M,3] fp32, encoder coordinates in [0,1]; embeddings, offsets, D, C, L, S, H, gridtype, align_corners, interp, dtype, offsets_host as
 *   foc_grid_encode_forward takes them (offsets_host is not read); sigma_weights: the sigma network's blob (foc_ffmlp_forward's layout,
 *   input_dim 32, output_dim 16), fp16, 16-byte aligned.
 *   rot9: NULL, or 9 fp32 in DEVICE memory: a row-major 3 x 3 rotation (object -> scene) applied to the normal.
 *   Outputs, each may be NULL (all NULL or M = 0: nothing is launched): sigma [M] fp32; grad_raw [M,3] fp32 = d raw / d xn; normal_rgb [M,3]
 *   fp32 = 0.5 + 0.5 (rot9) n; grad_enc [M,32] fp32 (16-byte aligned; NULL in production): d raw / d encoding, feature 2 l + c, exactly as
 *   the contraction consumed it — it exists so that the stages can be checked one at a time, like forward_buffer / backward_buffer.
 * Shape served — anything else is refused with FOC_E_INVALID (dtype: FOC_E_DTYPE) before any launch, the message names the argument:
 *   D 3, C 2, L 16, dtype FOC_F16, gridtype 0 (hash), align_corners 0, interp 0 (linear); hidden_dim 64, activation 0 (ReLU), sigma_layers 1..3.
 * Per sample:
 *   encode     the 32 features with foc_grid_encode_forward's arithmetic and bits (fp32, each rounded to half once) and the 96 derivatives
 *              dy_dx[l,d,c] = scale_l * sum over the 4 corner pairs along d of (w_a w_b) (v_right - v_left), from the same eight corner
 *              rows; fp32, NOT rounded to half (foc_grid_encode_forward's dy_dx is stored in the table dtype).
 *   forward    the sigma network as foc_nerf_field_inference runs it (fp32 MFMA sums, half once per layer, ReLU): sigma = exp(half(h[0]))
 *              has the SAME BITS as that entry point's sigma on foc_grid_encode_forward's output for the same points.
 *   backward   delta of the last hidden layer = [a > 0] W_out[0,:] (exact); per hidden matrix delta = [a > 0] half(W^T delta) (fp32 MFMA sum,
 *              rounded to half once, gated by the forward's own post-ReLU half a); grad_enc = W0^T delta_0, the fp32 sum, not rounded.
 *   contract   grad_raw[d] = sum_{l,c} grad_enc[l,c] dy_dx[l,d,c]: fp32 fmaf, two partial sums of 8 levels each ({0-3, 8-11} and {4-7, 12-15},
 *              level then channel ascending), added once.
 *   normalise  m = max_d |g_d|; m == 0 or a component not finite: n = 0; else u = g / m, n = -u / sqrt(u.u); n <- rot9 n; normal_rgb =
 *              fma(0.5, n, 0.5). All fp32.
 *   A point with a coordinate outside [0,1] has zero features and derivatives, as in the encoder: grad_enc = grad_raw = 0, n = 0,
 *   normal_rgb = 0.5 exactly, sigma = exp(0).
 * No atomics, no host synchronisation (capturable in a graph), nothing order-dependent: FOC_DETERMINISTIC changes nothing, and every subset
 * of the outputs has the bits of the full call. */
int foc_field_normals(const float *xn, uint32_t M, const void *embeddings, const uint32_t *offsets, uint32_t D, uint32_t C, uint32_t L,
                      float S, uint32_t H, uint32_t gridtype, int align_corners, uint32_t interp, int dtype, const int32_t *offsets_host,
                      const void *sigma_weights, uint32_t sigma_layers, uint32_t hidden_dim, uint32_t activation, const float *rot9,
                      float *sigma, float *grad_raw, float *normal_rgb, void *grad_enc, void *stream);
/* A composited normal map out of its accumulators, one launch over N pixels: normal_acc [N,3] = sum_k w_k (0.5 + 0.5 n_k) (the image a
 * composite makes of foc_field_normals' normal_rgb: foc_occ_render_step_normals) and weights_sum [N] = W. Per pixel, all fp32:
 *   s = 2 acc - W per component (= sum_k w_k n_k; 2 acc is exact, one rounding); m = max_d |s_d|; m == 0 or a component not finite: normal = 0;
 *   else u = s / m, normal = u / sqrt(u.u) (foc_field_normals' rule); normal_rgb = acc + (1 - W): the encoded map on a white background.
 * normal [N,3], normal_rgb [N,3]; neither may alias an input. No atomics, nothing order-dependent: FOC_DETERMINISTIC changes nothing. */
int foc_normal_map_finish(const float *normal_acc, const float *weights_sum, uint32_t N, float *normal, float *normal_rgb, void *stream);

/* The colour network of a ray-ordered sample list without its materialised input (network_ff.py:104-108 builds
 * cin = [SH16(dir) | h[:,1:16] | 0] per sample, 64 B written and read twice): the kernels take the sigma network's output
 * rows h [B,16] fp16 and one SH row per ray, ray_sh [B / samples_per_ray, 16] fp16 (foc_fixed_sample), and place
 * every value at the k position it has in cin — same bits as foc_ffmlp_forward / foc_ffmlp_backward (forward_buffer NULL,
 * input_dim 32, output_dim 16) on that cin. outputs [B,16] fp16.
 * Backward: grad [B,16] fp16 -> grad_weights (blob layout of foc_ffmlp_backward, same workspace) and grad_h [B,16] fp16 =
 * [grad_h0 | grad_cin[:,16:31]] with grad_h0 [B] fp16 (NULL = zeros) the density path's gradient of h[:,0]
 * (foc_fixed_tail_backward) — the row the sigma network's backward consumes, written once. hidden_dim 64, 2 or 3 layers.
 * out_width 16: outputs / grad are [B,16]; 4: only the columns that are ever read exist, outputs / grad are [B,4] (of the 16 padded
 * outputs of a 3-output network columns 0..2 are the rgb logits; the gradient of the others is zero by construction).
 * obj_feat (may be NULL): FOC's object-conditioned colour network (nerf/network_tcnn.py:611-640; see foc_nerf_field_inference) —
 * [16] fp16, cin = [SH16 | h[:,1:16] | obj_feat | 0] (48 wide; weights and grad_weights then have 48-wide W0 rows, the workspace is
 * foc_ffmlp_backward_workspace_bytes(48, ...)). Same values as foc_ffmlp_forward / _backward on that cin up to fp32 summation order
 * (the object columns' products are summed first). Backward: grad_weights[:, 31:47] = (sum_b delta_0[b,:]) (x) obj_feat, and
 * grad_obj [16] fp32 (may be NULL) = W0[:,31:47]^T sum_b delta_0[b,:], the gradient the object-feature encoder consumes. */
int foc_color_head_forward(const void *h, const void *ray_sh, uint32_t samples_per_ray, const void *weights,
                           uint32_t B, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                           void *outputs, uint32_t out_width, const void *obj_feat, void *stream);
int foc_color_head_backward(const void *grad, const void *h, const void *ray_sh, uint32_t samples_per_ray,
                            const void *grad_h0, const void *weights, uint32_t B, uint32_t hidden_dim,
                            uint32_t num_layers, uint32_t activation, void *grad_h, void *grad_weights,
                            void *workspace, uint64_t workspace_bytes, uint32_t out_width, const void *obj_feat, float *grad_obj, void *stream);
/* The two above with the value of input column 47 of the 48-wide row (replace foc_color_head_forward / _backward for the tinycudann
 * layout, as foc_nerf_field_inference_pad): cin = [SH16 | h[:,1:16] | obj_feat | input_pad]. Forward: W0[:,47] * input_pad is added to
 * the per-neuron constant after the object columns' products. Backward: grad_weights[:,47] = (sum_b delta_0[b,:]) * input_pad; grad_h and
 * grad_obj do not change. input_pad = 0 gives the bits of the entry points above; input_pad != 0 needs obj_feat. */
int foc_color_head_forward_pad(const void *h, const void *ray_sh, uint32_t samples_per_ray, const void *weights,
                               uint32_t B, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                               void *outputs, uint32_t out_width, const void *obj_feat, float input_pad, void *stream);
int foc_color_head_backward_pad(const void *grad, const void *h, const void *ray_sh, uint32_t samples_per_ray,
                                const void *grad_h0, const void *weights, uint32_t B, uint32_t hidden_dim,
                                uint32_t num_layers, uint32_t activation, void *grad_h, void *grad_weights,
                                void *workspace, uint64_t workspace_bytes, uint32_t out_width, const void *obj_feat, float *grad_obj,
                                float input_pad, void *stream);
/* foc_color_head_forward / _backward with input column 31 of the 32-wide row = input_pad (replace them for the legacy tinycudann layout,
 * as foc_nerf_field_inference_pad31): cin = [SH16 | h[:,1:16] | input_pad], 32-wide W0 rows; obj_feat must be NULL (grad_obj is not
 * written). Forward: W0[:,31] * input_pad is the initial value of the layer-0 accumulators (the object feature's slot). Backward: column 31
 * of the layer-0 input tile holds input_pad, so grad_weights[:,31] = sum_b delta_0[b,:] * input_pad — the products of the materialised
 * input; grad_h does not change. Same values as foc_ffmlp_forward / _backward on that cin up to fp32 summation order; input_pad = 0
 * gives the bits of the entry points above. num_layers 2 or 3. */
int foc_color_head_forward_pad31(const void *h, const void *ray_sh, uint32_t samples_per_ray, const void *weights,
                                 uint32_t B, uint32_t hidden_dim, uint32_t num_layers, uint32_t activation,
                                 void *outputs, uint32_t out_width, const void *obj_feat, float input_pad, void *stream);
int foc_color_head_backward_pad31(const void *grad, const void *h, const void *ray_sh, uint32_t samples_per_ray,
                                  const void *grad_h0, const void *weights, uint32_t B, uint32_t hidden_dim,
                                  uint32_t num_layers, uint32_t activation, void *grad_h, void *grad_weights,
                                  void *workspace, uint64_t workspace_bytes, uint32_t out_width, const void *obj_feat, float *grad_obj,
                                  float input_pad, void *stream);

/* The TRAINING forward of the whole field in ONE kernel (csrc/field_fwd.hip): foc_ffmlp_forward_planar on the encoder's planes ->
 * h [B,16] fp16 (written: the compositing tail and the backward read it) -> foc_color_head_forward fed from h and ray_sh, back to back in
 * registers — nerf/network_ff.py:51-75 as ffmlp.cu:331-407 evaluates it twice. Results are BIT FOR BIT those of the two separate calls
 * (same operands in the same k positions and order for every MFMA); h is not read back for the colour network (-32 B per sample, one
 * launch). planes [16][B] half2 (input width 32), hidden_dim 64, (sigma_layers, color_layers) in {(1,2), (1,3), (2,2), (2,3), (3,3)}, activation relu(0) /
 * none(6); ray_sh / samples_per_ray / out_width / obj_feat as foc_color_head_forward. The backward stays the two calls
 * foc_color_head_backward -> foc_ffmlp_backward_planar (they re-evaluate the activations from h and the planes). */
int foc_field_forward_train(const void *planes, const void *sigma_weights, uint32_t sigma_layers, const void *ray_sh, uint32_t samples_per_ray,
                            const void *color_weights, uint32_t color_layers, uint32_t hidden_dim, uint32_t activation, uint32_t B,
                            void *h, void *c, uint32_t out_width, const void *obj_feat, void *stream);
/* foc_field_forward_train with input column 47 of the 48-wide colour row = input_pad (replaces foc_field_forward_train for the tinycudann
 * layout; the bits of foc_ffmlp_forward_planar + foc_color_head_forward_pad). input_pad = 0: the bits of foc_field_forward_train. */
int foc_field_forward_train_pad(const void *planes, const void *sigma_weights, uint32_t sigma_layers, const void *ray_sh, uint32_t samples_per_ray,
                                const void *color_weights, uint32_t color_layers, uint32_t hidden_dim, uint32_t activation, uint32_t B,
                                void *h, void *c, uint32_t out_width, const void *obj_feat, float input_pad, void *stream);
/* foc_field_forward_train with input column 31 of the 32-wide colour row = input_pad (replaces it for the legacy tinycudann layout; the
 * bits of foc_ffmlp_forward_planar + foc_color_head_forward_pad31). obj_feat must be NULL. input_pad = 0: the bits of
 * foc_field_forward_train. Layer pairs as there. */
int foc_field_forward_train_pad31(const void *planes, const void *sigma_weights, uint32_t sigma_layers, const void *ray_sh, uint32_t samples_per_ray,
                                  const void *color_weights, uint32_t color_layers, uint32_t hidden_dim, uint32_t activation, uint32_t B,
                                  void *h, void *c, uint32_t out_width, const void *obj_feat, float input_pad, void *stream);

/* ffmlp.cu:721-740  allocate_splitk(size) / free_splitk(): the reference creates side
 * streams for its CUTLASS split-K GEMMs. Weight gradients here are produced inside the
 * backward launch sequence on the caller's stream, so both are no-ops kept for API parity. */
int foc_allocate_splitk(uint64_t size);
int foc_free_splitk(void);

/* ------------------------------------------------------------------------- *
 * Multi-object combine (reference: COMBINED.py:247-251 best_densities_and_colors_v3).
 * Per-sample strict-'>' max-density select; first object wins ties.
 * ------------------------------------------------------------------------- */

/* In place: where dens[i] > max_dens[i]: best_rgb[i,:] = rgb[i,:]; max_dens[i] = max(dens, max_dens).
 * n = number of samples. */
int foc_combine_select(const float *dens, const float *rgb, float *max_dens, float *best_rgb,
                       uint64_t n, void *stream);

/* Pack (sigma, rank) into the order-preserving 64-bit key used for the RCCL MAX
 * all-reduce of the one-object-per-GPU combine: key = (float_bits(max(sigma,0)) << 32) |
 * (0xFFFFFFFF - rank); and the inverse select of the winning rank's rgb. */
int foc_combine_pack_keys(const float *dens, uint32_t rank, uint64_t *keys, uint64_t n, void *stream);
int foc_combine_unpack(const uint64_t *keys, uint32_t rank, const float *rgb,
                       float *max_dens, float *masked_rgb, uint64_t n, void *stream);

/* Fixed-step composite of a merged field (COMBINED.py:141-200 image_depth_generation):
 * sigmas [N,T], rgbs [N,T,3], nears/fars [N]; out image4 [N,4] (rgb + sum w*sigma), depth [N].
 * bg: background value broadcast over the 4 channels; result clamped to [0,1]. */
int foc_composite_fixed_steps(const float *sigmas, const float *rgbs, const float *nears,
                              const float *fars, uint32_t N, uint32_t T, float bg,
                              float *image4, float *depth, void *stream);

#define FOC_COMBINE_MAX_OBJECTS 16 /* fields per fused call (the kernel's argument block), and objects per attributed scene */

/* The same select and composite fused over K objects' PACKED fields, the form the one-object-per-GPU exchange moves
 * (focnerf_amd/combine.py): fields4[k] -> device pointer to object k's [N,T,4] fp32 rows (sigma, r, g, b), k in checkpoint
 * order (host array of K device pointers, K <= 16; more objects: pre-merge with foc_combine_select4, the rule is
 * associative over the order). Replaces the object loop of COMBINED.py:598-618 + image_depth_generation :141-200 for one
 * ray chunk without storing the merged field. bgs: host array of n_bg (1 or 2) background values (the reference composites
 * white and black, compute_metrics_both_backgrounds); image4 [n_bg,N,4], depth [N]; merged4 [N,T,4] or NULL. */
int foc_combine_select_composite(const float *const *fields4, uint32_t K, const float *nears, const float *fars,
                                 uint32_t N, uint32_t T, const float *bgs, uint32_t n_bg, float *image4, float *depth,
                                 float *merged4, void *stream);

/* acc4 <- select(acc4, field4) on n packed samples (same rule; acc4 holds the earlier objects). */
int foc_combine_select4(const float *field4, float *acc4, uint64_t n, void *stream);

/* Attribution of the combined render: foc_combine_select_composite that also says WHICH object each part of the result came
 * from (no reference counterpart: COMBINED.py forgets the select's decision; a caller would have to store merged4 and repeat
 * the select). Inputs as above, plus an identity per field: the constant object id ids[k], or — for a field that is already a
 * pre-merge of several objects (foc_combine_select4_ids) — a uint8 [N,T] plane id_planes[k] with the id per sample.
 * id_planes: host array of K device pointers, an entry or the whole array may be NULL (= use ids[k]); ids: host array of K
 * values, read only for fields without a plane (NULL allowed when every field has one). n_obj = number of objects in the
 * scene, 1 <= n_obj <= FOC_COMBINE_MAX_OBJECTS; every id is < n_obj.
 *
 * Winner of a sample = the id travelling with the rgb the select keeps: field 0's id to begin with; field k's id replaces it
 * exactly when `sigma_k > running max` at k's turn — the comparison that replaces the rgb. So the first object keeps ties and
 * a NaN density never takes the rgb and therefore never the id.
 * Per ray, with w_i = alpha_i * T_i the composite's own weight of sample i and oz_i its clamped normalised depth:
 *   obj_weights [N, n_obj]  sum of w_i over the samples whose winner is that object. Columns of objects that never win are
 *                           exactly 0; a row sums to the ray's weights_sum up to rounding.
 *   obj_depth   [N, n_obj]  sum of w_i * oz_i over the same samples; a row sums to depth[n] up to rounding.
 *   instance    [N] int32   the first index of the row's largest obj_weights entry, or -1 when no entry is > 0 (an empty
 *                           ray; NaN entries are never the largest, a row of NaN gives -1).
 *   winner      [N,T] uint8 (optional, NULL: not written) the winner per sample.
 * image4, depth and merged4 are what foc_combine_select_composite writes, bit for bit. No atomics: a ray's sums are one
 * wave's fixed tree, so every output is run-to-run bit-stable whatever FOC_DETERMINISTIC says.
 * Constant ids are checked here (ids[k] >= n_obj: FOC_E_INVALID). The bytes of an id plane cannot be: a sample whose plane
 * says id >= n_obj is counted in NO column and can never be the instance; it still composites into image4 / depth. */
int foc_combine_select_composite_attr(const float *const *fields4, uint32_t K, const uint8_t *const *id_planes,
                                      const uint32_t *ids, uint32_t n_obj, const float *nears, const float *fars,
                                      uint32_t N, uint32_t T, const float *bgs, uint32_t n_bg, float *image4, float *depth,
                                      float *merged4, float *obj_weights, float *obj_depth, int32_t *instance,
                                      uint8_t *winner, void *stream);

/* The fused select + composite (+ attribution) fed directly from K objects' COMPACT culled lists: what foc_fixed_field_pack_culled{,_gain}
 * per object followed by foc_combine_select_composite{,_attr} computes, bit for bit in every output, without any field4 [N,T,4] being
 * written or read. One FocCulledField per object of the scene, as foc_fixed_cull{,_placed} and the field kernels left it; the array lives
 * in host memory and travels by value in the kernel argument block. */
typedef struct FocCulledField {
    const uint64_t *mask;     /* [R], R = ceil(N/64) * T rows in foc_fixed_cull's layout; 8-byte aligned */
    const uint32_t *offsets;  /* [R + 1] */
    const float *sigma_c;     /* [m_occ]; may be NULL when m_occ == 0 */
    const float *rgb_c;       /* [m_occ,3]; may be NULL when m_occ == 0 */
    uint32_t m_occ;
    float density_scale;      /* the pack's arguments */
    float thresh;
    float sigma_gain;         /* finite and > 0; 1: an unplaced object (foc_fixed_field_pack_culled's bits) */
} FocCulledField;
/* Entry of object k at sample (n, i), the pack's statements: row = (n/64) * T + i; occupied = bit n % 64 of mask[row] is set and
 * slot = offsets[row] + popcount(mask[row] & ((1 << (n % 64)) - 1)) < m_occ. Occupied: sigma = sigma_c[slot], times sigma_gain when that is
 * not 1, rgb = rgb_c[slot*3 ..]; otherwise all zero. Own weight w_k = alpha_k * prod_{j<i}(1 - alpha_j + 1e-15) with
 * alpha_k = 1 - expf((-delta * density_scale_k) * sigma), along object k's OWN transmittance; entry = (sigma, w_k > thresh_k ? rgb : 0).
 * Select, composite and attribution: foc_combine_select_composite_attr's, in its order — object 0 first, strict '>', NaN propagated;
 * ids: host array of K object ids (NULL: object k is k), n_obj = 0: no attribution, then obj_weights / obj_depth / instance / winner are
 * not written and may be NULL; n_obj > 0: as foc_combine_select_composite_attr (winner optional). merged4 [N,T,4] optional.
 * A 64-sample tile of a ray in which no object has a bit is skipped by its wave when skipping changes no bit (finite sample spacing and
 * normalised depth, a finite transmittance carry): every entry is zero there, alpha = 0 and 1 - 0 + 1e-15f == 1.0f, so carries and sums
 * stay as they are; merged4 = (0,0,0,0) and winner = ids[0] are still written for it. A ray that misses the box (near = far = FLT_MAX)
 * is never skipped: its depth is NaN (0 * NaN) as in the dense composite.
 * Refused with FOC_E_INVALID before any launch: K == 0 or K > FOC_COMBINE_MAX_OBJECTS; struct_bytes != sizeof(FocCulledField); n_bg not 1
 * or 2; T < 2; ceil(N/64) * 64 * T >= 2^31; a sigma_gain that is not finite and > 0; ids[k] >= n_obj; n_obj > FOC_COMBINE_MAX_OBJECTS;
 * a null objs; and, for N > 0: null mask / offsets / nears / fars / image4 / depth, m_occ > 0 with a null sigma_c or rgb_c, a misaligned
 * mask or merged4, n_obj > 0 with a null obj_weights / obj_depth / instance. N == 0 returns FOC_OK without a launch. No atomics, no shared
 * memory, no synchronisation. */
int foc_combine_select_composite_culled(const FocCulledField *objs, uint32_t K, uint32_t struct_bytes, const uint32_t *ids,
                                        uint32_t n_obj, const float *nears, const float *fars, uint32_t N, uint32_t T,
                                        const float *bgs, uint32_t n_bg, float *image4, float *depth, float *merged4,
                                        float *obj_weights, float *obj_depth, int32_t *instance, uint8_t *winner, void *stream);

/* foc_combine_select4 that keeps the identity: acc_ids [n] uint8 holds, per sample, the id of the object whose rgb acc4 holds
 * (the caller fills it with the first object's id). field4 is ONE object with the constant id `id` (< FOC_COMBINE_MAX_OBJECTS);
 * acc_ids[i] takes it exactly where acc4 takes field4's rgb. acc4 is updated as by foc_combine_select4, bit for bit. */
int foc_combine_select4_ids(const float *field4, uint32_t id, float *acc4, uint8_t *acc_ids, uint64_t n, void *stream);

/* MONeRFNetwork's running select (reference: nerf/multiobjectnetwork.py:66-82 — torch.max over stack([new, best]) with
 * take_along_dim of the rows that travel with the density: geo_feat [n,15] in density(), colour [n,3] in color()).
 * In place: where the new object takes sample i, sigma_best[i] = sigma_new[i] and feat_best[i,:] = feat_new[i,:].
 * The rule is torch.max's: the first maximal index wins and the new object is stacked first, so the NEW object takes
 * ties (COMBINED.py's select keeps the earlier one); NaN counts as maximal (a NaN of either side stays, the new one's
 * on both). sigma and feat have the same element type: elem_bytes 2 (half, under autocast) or 4 (float);
 * feat_width 1..64 elements per row, rows contiguous. */
int foc_mo_select(const void *sigma_new, const void *feat_new, void *sigma_best, void *feat_best, uint64_t n,
                  uint32_t feat_width, uint32_t elem_bytes, void *stream);

/* ------------------------------------------------------------------------- *
 * Fixed-step render path as fused ops. No reference binding: these replace the torch
 * code of nerf/renderer.py:145-221 (== COMBINED.py:451-534) and the glue of nerf/network_ff.py:51-134
 * between the encoder and the two MLPs. M = N*T samples, ray-major. `noise` ([M] uniform(0,1), the
 * reference's torch.rand for perturb, always ray-major) may be NULL.
 *
 * Sample order of the inference entry points (`ray_block`): 0 = ray-major, sample i of ray n at row n*T + i.
 * 64 = block-interleaved: row (n/64)*64*T + i*64 + n%64, ceil(N/64)*64*T rows, the last block padded with copies
 * of ray N-1 — 64 neighbouring rays at one depth are 64 consecutive rows, which is what makes the level-major
 * encoder forward fast on a rendered view (its wave then finds its corner rows in a few cache lines). What
 * leaves the path for the caller (image, depth, field4, rgb_masked, sigma_raymajor) is ray-major either way.
 * ------------------------------------------------------------------------- */

/* z = near + (far-near)*linspace(0,1,T)[i] (+ (noise-0.5)*(far-near)/T); xyz = clip(o + d z, aabb) -> xyzs [M,3]
 * and/or enc_in [M,3] = (xyz + bound)/(2 bound), the GridEncoder's normalised input (grid.py:149). */
int foc_fixed_sample(const float *rays_o, const float *rays_d, const float *nears, const float *fars,
                     const float *aabb, const float *noise, uint32_t N, uint32_t T, float bound,
                     float *xyzs, float *enc_in, void *ray_sh, uint32_t ray_block, void *stream);
/* ray_sh [N,16] fp16 or NULL: the degree-4 SH values of each ray's direction, rounded to fp16 as they stand in columns 0..15 of
 * the colour-net input (for foc_color_head_forward). */

/* h [M,16] fp16 = sigma-net output. sigma = exp(h[:,0]); weights = alpha * cumprod(1-alpha+1e-15);
 * trans [M] = transmittance before each sample; weights_sum/depth [N]; cin [M,cin_width] fp16 or NULL:
 *   cin_width 32: [SH16(dir) | h[:,1:16] | 0]                 (the colour-net input, network_ff.py:62-68)
 *   cin_width 48: [SH16(dir) | h[:,1:16] | obj_feat[16] | 0]  (FOC network with the encoded YOLO object feature,
 *                 nerf/network_tcnn.py:641-643; obj_feat = 16 fp16 values shared by all samples, NULL = zeros). */
int foc_fixed_head_forward(const void *h, const float *rays_d, const float *nears, const float *fars,
                           const float *noise, uint32_t N, uint32_t T, float density_scale,
                           float *sigma, float *trans, float *weights, float *weights_sum, float *depth,
                           void *cin, const void *obj_feat, uint32_t cin_width, void *stream);
/* grad_w [M], grad_ws [N], grad_depth [N], grad_cin [M,cin_width] fp16 (each may be NULL) -> grad_h [M,16] fp16
 * (the object-feature gradient is the column sum of grad_cin[:,31:47], left to the caller). */
int foc_fixed_head_backward(const void *h, const float *sigma, const float *trans, const float *nears,
                            const float *fars, const float *noise, const float *grad_w, const float *grad_ws,
                            const float *grad_depth, const void *grad_cin, uint32_t N, uint32_t T,
                            float density_scale, void *grad_h, uint32_t cin_width, void *stream);

/* Training tail in one pass per direction (one wave per ray): foc_fixed_head_forward (cin NULL) + foc_fixed_composite_forward,
 * and foc_fixed_composite_backward + column 0 of foc_fixed_head_backward (written as grad_h0 [M] fp16) — the same bits as the pairs; the weights are not
 * re-read, their gradient never leaves the lane, and the backward does not read h (exp(clamp(h0,-15,15)) = clamp(sigma, ...)).
 * c_width 16: c and grad_c are [M,16] rows as above; 4: they are [M,4] (rgb logits + one pad column), the compact form
 * foc_color_head_forward / _backward exchange with out_width 4.
 * ray_sumsq [N] (may be NULL): sum over the ray's samples of sigma^2 — what FOC's outside-mask density criterion
 * ||sigma[rays outside the object mask]||_2 (nerf/renderer.py:163-165) needs from the samples; grad_sumsq [N] (may be NULL) is its
 * gradient, added to the density path as 2 sigma grad_sumsq[ray] before trunc_exp's backward factor. */
int foc_fixed_tail_forward(const void *h, const void *c, const float *nears, const float *fars, const float *noise,
                           const float *bg_ray, float bg_scalar, uint32_t N, uint32_t T, float density_scale, float thresh,
                           float *sigma, float *trans, float *weights, float *weights_sum, float *depth, float *image,
                           uint32_t c_width, float *ray_sumsq, void *stream);
int foc_fixed_tail_backward(const float *grad_image, const float *grad_ws, const float *grad_depth, const void *c,
                            const float *sigma, const float *trans, const float *weights, const float *nears,
                            const float *fars, const float *noise, const float *bg_ray, float bg_scalar, uint32_t N,
                            uint32_t T, float density_scale, float thresh, void *grad_c, void *grad_h0, uint32_t c_width,
                            const float *grad_sumsq, void *stream);

/* Tail of the occupancy-grid TRAINING path on a ragged sample list (csrc/occtrain.hip; legacy/nerf/renderer.py:300-314):
 *   sigma = density_scale * exp(h[:,0]); rgb = sigmoid(c[:,0:3]) (rounded to fp16); composite_rays_train (raymarching.cu:500-588);
 *   image = raw + (1 - weights_sum) * bg (bg_ray [N,3] or NULL -> bg_scalar); depth = clamp(depth - nears, 0) / (fars - nears).
 * h [M,16] fp16 (density network output), c [M,c_width] fp16 (colour network output, c_width 4 or 16), deltas [M,2], rays [N,3].
 * Outputs [N] / [N,3] fp32: weights_sum, image_raw (the composite's own image: the backward needs it), image, depth.
 * Backward: grad_image [N,3] (of `image`), grad_ws [N] or NULL -> grad_c [M,c_width] fp16 and grad_h0 [M] fp16 (the gradient of
 * h[:,0], trunc_exp's factor applied) — what foc_color_head_backward consumes. EVERY row of both is written (zeros where a ray
 * stopped early, did not fit the list, and behind the last ray: `counter` = the march's counter, counter[0] = samples marched). */
int foc_occ_tail_forward(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays,
                         uint32_t M, uint32_t N, float T_thresh, float density_scale, const float *bg_ray, float bg_scalar,
                         const float *nears, const float *fars, float *weights_sum, float *image_raw, float *image,
                         float *depth, void *stream);
int foc_occ_tail_backward(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width,
                          const float *deltas, const int32_t *rays, const int32_t *counter, const float *weights_sum,
                          const float *image_raw, uint32_t M, uint32_t N, float T_thresh, float density_scale,
                          const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0, void *stream);
/* The two above with FOC's outside-mask density criterion (legacy nerf/renderer.py:163-165 on a ragged list), as foc_fixed_tail_forward /
 * _backward carry it: ray_sumsq [N] = sum of exp(h[:,0])^2 (sigma before density_scale) over ALL rays[n].count samples of the ray, those
 * behind the sample at which the composite stopped at T_thresh included; 0 for a ray that did not fit the list. One wave per ray in a fixed
 * order: the same bits on every run. Backward: grad_sumsq [N] is its gradient; 2 sigma grad_sumsq[ray] is added to the density path before
 * trunc_exp's factor on every row of a ray that fits — the rows behind an early stop, zeros above, carry that term alone. Everything
 * else is bit for bit the two entry points above. */
int foc_occ_tail_forward_sumsq(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays,
                               uint32_t M, uint32_t N, float T_thresh, float density_scale, const float *bg_ray, float bg_scalar,
                               const float *nears, const float *fars, float *weights_sum, float *image_raw, float *image,
                               float *depth, float *ray_sumsq, void *stream);
int foc_occ_tail_backward_sumsq(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width,
                                const float *deltas, const int32_t *rays, const int32_t *counter, const float *weights_sum,
                                const float *image_raw, uint32_t M, uint32_t N, float T_thresh, float density_scale,
                                const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0, const float *grad_sumsq, void *stream);

/* The four tails above with the per-ray DISTORTION of mip-NeRF 360 (the reference's loss.py eff_distloss without its division by the ray
 * count), a differentiable output, from the weights the tails already form:
 *   dist = sum_i (1/3) delta_i w_i^2 + 2 sum_i w_i (m_i W_<i - WM_<i),   W_<i = sum_{j<i} w_j,  WM_<i = sum_{j<i} w_j m_j
 * fixed-step: m_i = (z_i - near) + delta_i / 2 and delta_i = the distance to the next sample (the last one: (far - near) / T), world units,
 *   the raw weight (not the `w > thresh` colour mask); a ray with !(far > near) gets dist = 0, ray_wm = 0 and no distortion gradient (its
 *   weights are 0 and its m may be non-finite).
 * ragged: m_i = the running sum of deltas[:,1] including sample i (the depth's t), delta_i = deltas[:,0], w = the composite's weight: 0
 *   behind the sample at which the ray stopped at T_thresh, that sample counts. A ray with count 0 or one that does not fit the list gets
 *   0 and no gradient; rows behind a stop get no distortion gradient.
 * m and delta carry no gradient; the only gradient is through w: G_i = d dist / d w_i = (2/3) delta_i w_i + 2 (m_i (W_<i - W_>i) + (WM_>i - WM_<i)).
 * Forward: ray_dist [N] and ray_wm [N] (= sum_i w_i m_i, which the backward needs beside weights_sum), both required; ray_sumsq [N] may be
 *   NULL (with or without the outside-mask criterion). Every other output is bit for bit the plain entry point's.
 * Backward: grad_dist [N] = the gradient of ray_dist; NULL: the plain backward (ray_wm / ray_dist are then not read). Otherwise ray_wm
 *   [N] and weights_sum [N] of the forward are required; grad_dist[ray] G_i joins the gradient of w_i — fixed-step: before the density
 *   head's backward; ragged: grad_sigma_i gains dt0_i g (G_i T_after_i - sum_{j>i} G_j w_j), with sum_j G_j w_j = 2 dist taken from
 *   ray_dist [N] (required there; the fixed-step backward walks from the ray's end, accepts ray_dist and does not read it). A ray whose
 *   grad_dist is 0 gets the plain backward's bits. grad_sumsq [N] may be NULL. One wave per ray, wave scans only: the same bits on every run. */
int foc_fixed_tail_forward_dist(const void *h, const void *c, const float *nears, const float *fars, const float *noise,
                                const float *bg_ray, float bg_scalar, uint32_t N, uint32_t T, float density_scale, float thresh,
                                float *sigma, float *trans, float *weights, float *weights_sum, float *depth, float *image,
                                uint32_t c_width, float *ray_sumsq, float *ray_dist, float *ray_wm, void *stream);
int foc_fixed_tail_backward_dist(const float *grad_image, const float *grad_ws, const float *grad_depth, const void *c,
                                 const float *sigma, const float *trans, const float *weights, const float *weights_sum, const float *nears,
                                 const float *fars, const float *noise, const float *bg_ray, float bg_scalar, uint32_t N,
                                 uint32_t T, float density_scale, float thresh, void *grad_c, void *grad_h0, uint32_t c_width,
                                 const float *grad_sumsq, const float *ray_wm, const float *ray_dist, const float *grad_dist, void *stream);
int foc_occ_tail_forward_dist(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays,
                              uint32_t M, uint32_t N, float T_thresh, float density_scale, const float *bg_ray, float bg_scalar,
                              const float *nears, const float *fars, float *weights_sum, float *image_raw, float *image,
                              float *depth, float *ray_sumsq, float *ray_dist, float *ray_wm, void *stream);
int foc_occ_tail_backward_dist(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width,
                               const float *deltas, const int32_t *rays, const int32_t *counter, const float *weights_sum,
                               const float *image_raw, uint32_t M, uint32_t N, float T_thresh, float density_scale,
                               const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0, const float *grad_sumsq,
                               const float *ray_wm, const float *ray_dist, const float *grad_dist, void *stream);
/* The ragged tails with a DIFFERENTIABLE depth: supersets of the _dist pair above. The reference's composite ignores grad_depth
 * (raymarching.cu:601-693) and foc_occ_tail_backward keeps doing so; these carry it, as foc_fixed_tail_backward does on the fixed-step path.
 * Forward: depth_raw [N] (may be NULL) = sum_i w_i t_i over the samples that count, t_i = the running sum of deltas[:,1] including sample
 *   i — the composite's own depth before depth = clamp(depth_raw - near, 0) / (far - near); exactly 0 for a ray with count 0 or one that
 *   does not fit the list. ray_sumsq [N] may be NULL; ray_dist and ray_wm [N] may be NULL together (one without the other is refused).
 *   Every other output is bit for bit the plain / _sumsq / _dist entry point's; with all four NULL this is foc_occ_tail_forward.
 * Backward: grad_depth [N] (may be NULL) = the gradient of the NORMALISED depth. Per ray
 *     s = (depth_raw - near < 0 || !(far > near)) ? 0 : grad_depth / (far - near)
 *   — the forward's own clamp branch, which passes the gradient at exactly 0 as torch.clamp(min=0) does — and on the samples that count
 *     grad_sigma_i += dt0_i s (T_after_i t_i - (depth_raw - D_acc_i)),    D_acc_i = sum_{j<=i} w_j t_j.
 *   t carries no gradient (deltas are inputs). Rows behind a stop, rays that do not fit, clamped rays and rays whose grad_depth is 0 get
 *   nothing from it: the plain backward's bits. grad_depth needs depth_raw, nears and fars (refused otherwise; without grad_depth none of
 *   the three is read); grad_dist needs ray_wm and ray_dist as above; grad_sumsq, grad_dist, grad_depth NULL = absent, in any combination.
 *   One wave per ray, wave scans only, no atomics: the same bits on every run. */
int foc_occ_tail_forward_depth(const void *h, const void *c, uint32_t c_width, const float *deltas, const int32_t *rays,
                               uint32_t M, uint32_t N, float T_thresh, float density_scale, const float *bg_ray, float bg_scalar,
                               const float *nears, const float *fars, float *weights_sum, float *image_raw, float *image,
                               float *depth, float *ray_sumsq, float *ray_dist, float *ray_wm, float *depth_raw, void *stream);
int foc_occ_tail_backward_depth(const float *grad_image, const float *grad_ws, const void *h, const void *c, uint32_t c_width,
                                const float *deltas, const int32_t *rays, const int32_t *counter, const float *weights_sum,
                                const float *image_raw, uint32_t M, uint32_t N, float T_thresh, float density_scale,
                                const float *bg_ray, float bg_scalar, void *grad_c, void *grad_h0, const float *grad_sumsq,
                                const float *ray_wm, const float *ray_dist, const float *grad_dist, const float *nears,
                                const float *fars, const float *depth_raw, const float *grad_depth, void *stream);

/* The whole occupancy-grid TRAINING node as ONE call each way (csrc/occtrain.hip): what legacy/nerf/renderer.py:256-322 (`run_cuda`, training
 * branch, a fixed sample budget) + nerf/network_ff.py:51-75 do between the rays and the image, in the order
 *   forward:  foc_march_rays_train_field -> foc_grid_encode_forward_counted -> foc_ffmlp_forward_planar -> foc_color_head_forward -> foc_occ_tail_forward
 *   backward: foc_occ_tail_backward -> foc_color_head_backward -> foc_ffmlp_backward_planar -> foc_grid_encode_backward_binned[_counted]
 * — the SAME entry points with the same arguments, launched from C instead of from the host language: nine library calls per step cost a
 * Python caller ~0.25 ms of the ~0.8 ms a 4096-ray step takes on the GPU, and the step then depends on the host's speed. Every buffer is the
 * caller's (device memory, sizes as the entry points above document them; `cap` = rows of the sample arrays = the sample budget M);
 * the encoder must be one the binned backward serves (D = 3, C = 2, fp16 table: foc_grid_encode_backward_workspace_bytes != 0).
 * `struct_bytes` = sizeof(FocOccTrainNode): a binding built against another layout is refused. Backward: `precounted` != 0 when the
 * workspace header still holds the count pass of THIS node's forward (nothing else used `grid_workspace` in between). */
typedef struct FocOccTrainNode {
    uint32_t struct_bytes;
    /* rays, occupancy grid, march (foc_march_rays_train_field) */
    uint32_t n_rays, max_steps, cascade, grid_size, cap, pad_align;
    float bound, dt_gamma, min_near;
    const float *rays_o, *rays_d, *aabb, *jitter;
    const uint8_t *bitfield;
    float *nears, *fars, *enc_in, *deltas;
    void *sh_rows;
    int32_t *rays, *counter, *march_scratch;
    /* hash-grid encoder, [L,M,2] planes */
    uint32_t levels, base_resolution, gridtype, interp;
    int32_t align_corners, table_dtype;
    float per_level_scale_log2;
    const void *embeddings;
    const int32_t *offsets, *offsets_host;
    void *planes, *grid_workspace;
    uint64_t grid_workspace_bytes;
    /* density network (FFMLP, planar input) and colour head */
    uint32_t sigma_input_dim, sigma_hidden, sigma_layers, sigma_activation, sigma_output_activation;
    uint32_t color_hidden, color_layers, color_activation, c_width;
    const void *w_sigma, *w_color;
    void *h, *c;
    /* tail */
    float T_thresh, density_scale, bg_scalar;
    const float *bg_ray;
    float *weights_sum, *image_raw, *image, *depth;
    /* backward only */
    int32_t precounted;
    const float *grad_image, *grad_ws;
    void *grad_c, *grad_h0, *grad_h, *grad_planes, *grad_w_color, *grad_w_sigma, *grad_embeddings, *mlp_workspace;
    uint64_t mlp_workspace_bytes;       /* size of mlp_workspace: >= foc_ffmlp_backward_workspace_bytes() of both networks */
} FocOccTrainNode;
int foc_occ_train_forward(const FocOccTrainNode *node, void *stream);
int foc_occ_train_backward(const FocOccTrainNode *node, void *stream);
/* The node with input column 31 of the 32-wide colour row = input_pad (the legacy tinycudann layout, focnerf_amd/network_tcnn_legacy.py):
 * the same sequence through foc_field_forward_train_pad31 / foc_color_head_forward_pad31 / foc_color_head_backward_pad31; the one-kernel
 * forward of both networks also serves (sigma_layers, color_layers) = (1,2), (1,3). The node's layout is FocOccTrainNode's; input_pad
 * travels beside it, and the backward must get the forward's value. input_pad != 0 needs (1,2), (1,3), (2,2), (2,3) or (3,3), refused
 * before anything is enqueued. input_pad = 0: the bits of the two entry points above. */
int foc_occ_train_forward_pad31(const FocOccTrainNode *node, float input_pad, void *stream);
int foc_occ_train_backward_pad31(const FocOccTrainNode *node, float input_pad, void *stream);
/* The node of an object-conditioned network (focnerf_amd/network_foc.py, network_tcnn.py: a 48-wide colour input [SH16 | h[1:16] | obj_feat |
 * input_pad]). FocOccTrainNode keeps its layout; what the object adds travels beside it in FocOccTrainObject, as input_pad does for the
 * *_pad31 twins. The same sequence through foc_field_forward_train[_pad] / foc_color_head_forward[_pad] / foc_color_head_backward[_pad] with
 * obj_feat, w_color and grad_w_color with 48-wide W0 rows, mlp_workspace sized for input_dim 48 (foc_ffmlp_backward_workspace_bytes(48, 64,
 * color_layers)). ray_sumsq [n_rays] (may be NULL): the tail is foc_occ_tail_forward_sumsq; grad_sumsq [n_rays] (may be NULL): the backward's
 * tail is foc_occ_tail_backward_sumsq. grad_obj [16] fp32 (may be NULL): the gradient of obj_feat, as foc_color_head_backward writes it.
 * `struct_bytes` = sizeof(FocOccTrainObject). Refused before anything is enqueued: a wrong struct_bytes of either struct, a NULL obj_feat,
 * input_pad != 0 without obj_feat, (sigma_layers, color_layers) outside (1,2), (1,3), (2,2), (2,3), (3,3), sigma_input_dim != 32, sigma_hidden
 * or color_hidden != 64, sigma_activation != color_activation, a hidden activation other than relu (0) or none (6), sigma_output_activation
 * != 6 (the shapes the 48-wide head and foc_field_forward_train are built for), a workspace too small. */
typedef struct FocOccTrainObject {
    uint32_t struct_bytes;
    float input_pad;                    /* column 47 of the colour input: 0 (network_foc.py) or 1.0 (network_tcnn.py) */
    const void *obj_feat;               /* [16] fp16, the ENCODED object feature */
    float *ray_sumsq;
    /* backward only */
    const float *grad_sumsq;
    float *grad_obj;
} FocOccTrainObject;
int foc_occ_train_forward_obj(const FocOccTrainNode *node, const FocOccTrainObject *object, void *stream);
int foc_occ_train_backward_obj(const FocOccTrainNode *node, const FocOccTrainObject *object, void *stream);
/* The node whose tail also returns the per-ray distortion and / or a differentiable depth (foc_occ_tail_forward_depth / _backward_depth in
 * the tail's place). FocOccTrainNode and FocOccTrainObject keep their layouts; the tail's optional buffers travel beside them in
 * FocOccTrainTail, as the object's do. ONE pair serves the three layouts of the colour input: object NULL and input_pad 0 = the sequence of
 * foc_occ_train_forward / _backward; object NULL and input_pad != 0 = the _pad31 pair; an object = the _obj pair (the pad is the object's,
 * `input_pad` is not read) — the same checks, all before the first launch. Forward: ray_dist and ray_wm [n_rays] (NULL together),
 * depth_raw [n_rays] (may be NULL). Backward: grad_dist [n_rays] (may be NULL; needs the forward's ray_dist / ray_wm), grad_depth [n_rays]
 * (may be NULL; needs depth_raw and the node's nears / fars). `struct_bytes` = sizeof(FocOccTrainTail). Refused: a NULL tail, a wrong
 * struct_bytes, ray_dist without ray_wm or the reverse, a gradient without its forward buffers. */
typedef struct FocOccTrainTail {
    uint32_t struct_bytes;
    float *ray_dist, *ray_wm, *depth_raw;
    /* backward only */
    const float *grad_dist, *grad_depth;
} FocOccTrainTail;
int foc_occ_train_forward_tail(const FocOccTrainNode *node, const FocOccTrainObject *object, float input_pad,
                               const FocOccTrainTail *tail, void *stream);
int foc_occ_train_backward_tail(const FocOccTrainNode *node, const FocOccTrainObject *object, float input_pad,
                                const FocOccTrainTail *tail, void *stream);

/* Extension (no reference binding; focnerf_amd/rayorder.py): perm [N] int64 = the order in which a staged render walks a view's rays —
 * tile_h x tile_w pixel tiles when rays_d [N,3] fp32 is a row-major H x W pixel grid (recognised from the directions: W >= 16, H >= 8),
 * else the identity. Found and built on the device, no host round trip. state16: 16 bytes of device scratch. */
int foc_view_tile_order(const float *rays_d, uint32_t N, uint32_t tile_h, uint32_t tile_w, int64_t *perm, void *state16,
                        void *stream);

/* c [M,16] fp16 = colour-net output; rgb = sigmoid(c[:, :3]) (rounded to fp16 like the reference's half
 * sigmoid) where weights > thresh, else 0; image [N,3] = sum w rgb + (1 - sum w) bg. bg_ray [N,3] or NULL
 * (then bg_scalar). */
int foc_fixed_composite_forward(const void *c, const float *weights, const float *bg_ray, float bg_scalar,
                                uint32_t N, uint32_t T, float thresh, float *image, void *stream);
int foc_fixed_composite_backward(const float *grad_image, const void *c, const float *weights,
                                 const float *bg_ray, float bg_scalar, uint32_t N, uint32_t T, float thresh,
                                 void *grad_c, float *grad_w, void *stream);

/* Inference tail of the fixed-step renderer in one pass: sigma [M] fp32, rgb [M,3] fp32 (e.g. from
 * foc_nerf_field_inference) -> weights (alpha * cumprod), image [N,3] = sum w rgb [w > thresh] + (1 - sum w) bg,
 * depth [N], weights_sum [N]; rgb_masked [M,3] (may be NULL) = rgb where w > thresh else 0, the `rgbs` field of
 * nerf/renderer.py:187. ray_block = 64: sigma / rgb stand in the block-interleaved order (16-byte aligned,
 * ceil(N/64)*64*T rows); sigma_raymajor [M] (may be NULL) then receives the densities in ray-major order, the
 * `densities` field. Same bits either way. */
int foc_fixed_render_inference(const float *sigma, const float *rgb, const float *nears, const float *fars,
                               const float *noise, const float *bg_ray, float bg_scalar, uint32_t N, uint32_t T,
                               float density_scale, float thresh, float *image, float *depth, float *weights_sum,
                               float *rgb_masked, uint32_t ray_block, float *sigma_raymajor, void *stream);

/* foc_fixed_render_inference that also (or only: image, depth and weights_sum may then all be NULL) writes the object's
 * per-sample field packed as field4 [N,T,4] fp32 = (sigma, rgb where w > thresh else 0): the (`densities`, `rgbs`) pair
 * of nerf/renderer.py:187 / COMBINED.py:598-600 in the layout foc_combine_select_composite reads. */
int foc_fixed_field_pack(const float *sigma, const float *rgb, const float *nears, const float *fars,
                         const float *noise, const float *bg_ray, float bg_scalar, uint32_t N, uint32_t T,
                         float density_scale, float thresh, float *image, float *depth, float *weights_sum,
                         float *field4, uint32_t ray_block, void *stream);

/* Occupancy-culled fixed-step field of ONE object for the multi-object combiner (csrc/fixedcull.hip; no reference binding). The
 * combiner's per-sample select needs every object at the same T positions of the same rays, so the positions stay those of
 * foc_fixed_sample(noise = NULL, ray_block = 64) — the same bits — and each is tested against the object's occupancy bitfield
 * (uint8 [cascade * grid_size^3 / 8], Morton order, as foc_packbits writes it). The cell is the one foc_march_rays finds for that
 * position, with the cascade level taken from the position alone (no dt term: a fixed-step sample has no marching step):
 *   level = min(cascade - 1, max(0, frexp exponent of max |x|)); mip_bound = min(2^level, bound);
 *   n = (int)clamp(0.5 * (x / mip_bound + 1) * grid_size, 0, grid_size - 1) per axis; index = level * grid_size^3 + morton3D(n);
 *   occupied = bit (index & 7) of byte (index >> 3).
 * Only occupied samples go through the encoder and the networks; every other sample has sigma = 0. That is the approximation the
 * occupancy-grid renderer makes: densities below the grid's threshold are dropped.
 *
 * Rows: R = ceil(N/64) * T, row (n/64) * T + i holds sample i of the 64 rays of block n/64 (the block-interleaved order, one row =
 * 64 consecutive samples of it). The compact list holds the occupied samples in that order:
 *   slot(n, i) = offsets[row] + popcount(mask[row] & ((1 << (n % 64)) - 1)).
 * Slots come from a prefix sum, not from atomics: the same list on every run.
 *
 * foc_fixed_cull       writes mask [R] uint64 (bit n % 64 of a row: sample i of ray n is occupied; bits of the padding lanes n >= N
 *                      are never set), offsets [R + 1] uint32 (exclusive prefix sum of the rows' popcounts, offsets[R] = M_occ) and
 *                      count [1] uint32 = M_occ. scratch: foc_fixed_cull_scratch_bytes(N, T) device bytes, no initialisation needed.
 *                      cascade 1..16, grid_size a power of two <= 1024, cascade * grid_size^3 < 2^32, ceil(N/64) * 64 * T < 2^31,
 *                      T >= 2. N = 0 writes offsets[0] = count = 0.
 * foc_fixed_cull_emit  from that mask / offsets: enc_in_c [m_occ,3] = the occupied samples' normalised positions (foc_fixed_sample's
 *                      enc_in rows) and dirs_c [m_occ,3] = their rays' directions. m_occ = the count the caller read; the arrays hold
 *                      m_occ rows and nothing is written past them.
 * Neither call synchronises; reading count on the host between them is the caller's one synchronisation. */
uint64_t foc_fixed_cull_scratch_bytes(uint32_t N, uint32_t T);
int foc_fixed_cull(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb,
                   uint32_t N, uint32_t T, float bound, const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size,
                   uint64_t *mask, uint32_t *offsets, uint32_t *count, void *scratch, uint64_t scratch_bytes, void *stream);
int foc_fixed_cull_emit(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *aabb,
                        uint32_t N, uint32_t T, float bound, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ,
                        float *enc_in_c, float *dirs_c, void *stream);

/* foc_fixed_field_pack(ray_block = 64, image = depth = weights_sum = NULL) for a culled object: sigma_c [m_occ] and rgb_c [m_occ,3]
 * fp32 are the field on the compact list (foc_nerf_field_inference on enc_in_c / dirs_c with dir_div 1), mask / offsets as
 * foc_fixed_cull wrote them. field4 [N,T,4] fp32, ray-major, 16-byte aligned: (sigma, rgb where the object's own weight
 * alpha * cumprod > thresh else 0) at occupied samples, (0, 0, 0, 0) at every other. Bit for bit what foc_fixed_field_pack gives
 * on dense block-interleaved arrays whose sigma was zeroed at the unoccupied samples; no dense per-sample array is read or
 * written. m_occ = 0: sigma_c / rgb_c may be NULL, field4 is all zeros. */
int foc_fixed_field_pack_culled(const float *sigma_c, const float *rgb_c, const uint64_t *mask, const uint32_t *offsets,
                                uint32_t m_occ, const float *nears, const float *fars, uint32_t N, uint32_t T,
                                float density_scale, float thresh, float *field4, void *stream);

/* The three calls above for an object PLACED in a scene: object -> world is x_world = s R (x_obj - pivot) + pivot + translation with a
 * rotation R and a uniform scale s > 0; the calls take its inverse, world_to_object = 12 floats IN HOST MEMORY: A = R^T / s row-major,
 * then b (q = A x + b). obj_aabb: 6 floats in host memory, the object's own box (lo, then hi). Both travel by value in the kernel
 * argument block. scene_aabb [6] is device memory like foc_fixed_cull's aabb.
 *   World sample.  Exactly the point foc_fixed_sample(noise = NULL, ray_block = 64) produces for (rays_o, rays_d, nears, fars,
 *                  scene_aabb): clamped to scene_aabb, the same bits. nears / fars belong to the view's rays against the scene box and
 *                  are passed in.
 *   Object-frame point.  Per axis k: q_k = ((A_k0 x + A_k1 y) + A_k2 z) + b_k — this operation order, no contraction. q is not clamped.
 *   Inside.        obj_aabb_lo <= q <= obj_aabb_hi on all three axes. occupied = inside && bit(cell(q)), cell = foc_fixed_cull's on q
 *                  with the object's bound / cascade / grid_size.
 *   Emit.          enc_in_c = (q + bound) / (2 bound); dirs_c = dir_scale * ((A_k0 dx + A_k1 dy) + A_k2 dz), computed per ray and not
 *                  renormalised (dir_scale = s gives the turned direction at its original length).
 *   Pack with gain.  The sample's sigma is sigma_c[slot] * sigma_gain, one fp32 multiply (sigma_gain = 1 / s: the object's density per
 *                  unit of WORLD length); that value goes into field4.x and into the own-weight mask. sigma_gain finite and > 0. With
 *                  sigma_gain == 1 the bits are those of foc_fixed_field_pack_culled.
 *   Everything else as foc_fixed_cull: mask / offsets layout, slots by prefix sum, refusals (plus: null or non-finite host arrays),
 *                  N = 0, the 2^31 limit, no synchronisation.
 *   Identity case. With A = I, b = 0, dir_scale = 1 and obj_aabb = scene_aabb, mask, offsets, enc_in_c and dirs_c equal the unplaced
 *                  entry points' bit for bit. */
int foc_fixed_cull_placed(const float *rays_o, const float *rays_d, const float *nears, const float *fars, const float *scene_aabb,
                          uint32_t N, uint32_t T, const float *world_to_object, const float *obj_aabb, float bound,
                          const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size, uint64_t *mask, uint32_t *offsets,
                          uint32_t *count, void *scratch, uint64_t scratch_bytes, void *stream);
int foc_fixed_cull_emit_placed(const float *rays_o, const float *rays_d, const float *nears, const float *fars,
                               const float *scene_aabb, uint32_t N, uint32_t T, const float *world_to_object, float dir_scale,
                               float bound, const uint64_t *mask, const uint32_t *offsets, uint32_t m_occ, float *enc_in_c,
                               float *dirs_c, void *stream);
int foc_fixed_field_pack_culled_gain(const float *sigma_c, const float *rgb_c, const uint64_t *mask, const uint32_t *offsets,
                                     uint32_t m_occ, const float *nears, const float *fars, uint32_t N, uint32_t T,
                                     float density_scale, float thresh, float sigma_gain, float *field4, void *stream);

/* ---------------------------------------------------------------------------
 * Per-sample network glue for callers with arbitrary sample lists (the occupancy-grid paths): the torch
 * expressions of nerf/network_ff.py:51-75 between the sigma network, the SH-encoded direction and the
 * colour network. No reference binding (the reference runs them as ~25 torch kernels per call).
 * ------------------------------------------------------------------------- */

/* h [M,16] fp16 = sigma-net output, dirs [M,3] fp32. sigma [M] fp32 = trunc_exp(h[:,0]) (activation.py:8-13);
 * cin [M,cin_width] fp16 = [SH degree 4 of dir | h[:,1:16] | 0] (cin_width 32, network_ff.py:62-68) or
 * [SH | h[:,1:16] | obj_feat[16] | 0] (cin_width 48, see foc_fixed_head_forward). sigma or cin may be NULL. */
int foc_sample_head_forward(const void *h, const float *dirs, uint64_t M, float *sigma, void *cin,
                            const void *obj_feat, uint32_t cin_width, void *stream);
/* grad_sigma [M] fp32, grad_cin [M,cin_width] fp16 (either may be NULL) -> grad_h [M,16] fp16
 * (column 0: grad_sigma * exp(clamp(h0,-15,15)), activation.py:16-18; columns 1..15: grad_cin[:,16:31]). */
int foc_sample_head_backward(const void *h, const float *grad_sigma, const void *grad_cin, uint64_t M,
                             void *grad_h, uint32_t cin_width, void *stream);
/* Degree-4 real spherical harmonics of dirs [M,3] fp32 -> out [M,16] fp32: the direction encoder the reference imports as
 * encoding.get_encoder('sphere_harmonics') (network_ff.py:43) but does not ship. */
int foc_sh_encode(const float *dirs, uint64_t M, float *out, void *stream);
/* c [M,16] fp16 = colour-net output -> rgb [M,3] fp32 = sigmoid(c[:, :3]) rounded to fp16 (network_ff.py:73). */
int foc_rgb_head_forward(const void *c, uint64_t M, float *rgb, void *stream);
/* grad_rgb [M,3] fp32 -> grad_c [M,16] fp16 (columns 3..15 zero). */
int foc_rgb_head_backward(const void *c, const float *grad_rgb, uint64_t M, void *grad_c, void *stream);

/* ---------------------------------------------------------------------------
 * Occupancy-grid maintenance on the device (csrc/densitygrid.hip). Reference: the torch code of
 * NeRFRenderer.mark_untrained_grid (nerf/renderer.py:356-418) and NeRFRenderer.update_extra_state
 * (nerf/renderer.py:420-508), which the reference runs from Python (no binding). density_grid is
 * [cascade, H^3] fp32 in Morton order, bitfield uint8 [cascade * H^3 / 8]; random numbers come in as
 * arrays so that a call can be replayed by the oracle.
 * ------------------------------------------------------------------------- */

/* poses [B,4,4] fp32 camera-to-world, row-major. count (int32 [cascade,H^3], may be NULL) = cameras that see
 * the cell; density_grid[count == 0] = -1 (renderer.py:416). */
int foc_mark_untrained_grid(const float *poses, uint32_t B, float fx, float fy, float cx, float cy, float bound,
                            uint32_t cascade, uint32_t H, float *density_grid, int32_t *count, void *stream);
/* Query points of the full sweep (the first 16 updates, renderer.py:430-453): xyzs [cascade*H^3,3], cell m of a
 * cascade at row m (Morton order); jitter [cascade*H^3,3] uniform in [0,1) or NULL. */
int foc_grid_cells_xyz(uint32_t cascade, uint32_t H, float bound, const float *jitter, float *xyzs, void *stream);
/* Query points of the steady-state update (renderer.py:476-493): per cascade N uniformly random cells
 * (rand_coords int32 [cascade,N,3] in [0,H)) followed by N cells drawn uniformly from the occupied ones
 * (density_grid > 0; pick k = floor(rand_pick * n_occupied), rand_pick fp32 [cascade,N] in [0,1)).
 * Outputs indices int32 [cascade,2N] (Morton), xyzs [cascade*2N,3] jittered by jitter [cascade*2N,3]. */
uint64_t foc_grid_update_sample_workspace_bytes(uint32_t cascade, uint32_t H);
int foc_grid_update_sample(const float *density_grid, uint32_t cascade, uint32_t H, float bound, uint32_t N,
                           const int32_t *rand_coords, const float *rand_pick, const float *jitter,
                           int32_t *indices, float *xyzs, void *workspace, uint64_t workspace_bytes, void *stream);
/* tmp = -1; tmp[cas, indices] = sigmas * density_scale (largest on duplicates); where density_grid >= 0 and tmp >= 0:
 * density_grid = max(density_grid * decay, tmp); mean_out (device fp32, may be NULL) = mean(clamp(density_grid, 0));
 * bitfield = packbits(density_grid, min(mean, density_thresh))  (renderer.py:428, :493-503). sigmas fp32 [cascade*Mc];
 * indices int32 [cascade*Mc], or NULL when sigmas cover every cell in Morton order (Mc == H^3). No host synchronisation. */
uint64_t foc_grid_update_apply_workspace_bytes(uint32_t cascade, uint32_t H);
int foc_grid_update_apply(float *density_grid, uint32_t cascade, uint32_t H, const float *sigmas, const int32_t *indices,
                          uint32_t Mc, float density_scale, float decay, float density_thresh, uint8_t *bitfield,
                          float *mean_out, void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Background model of torch-ngp's default network (focnerf_amd/network_linear.py, csrc/background.hip): per ray
 *     rgb = sigmoid(W1 . relu(W0 . [SH16(d) | grid8((sph_from_ray(o, d, radius) + 1) / 2)]))
 * replacing the op chain of legacy/nerf/network.py:145-160 (NeRFNetwork.background) with sph_from_ray in front of it
 * (legacy/nerf/renderer.py:232-234, 271-274), fp16 autocast semantics.
 * coords [N,2] fp32 in [-1,1] (the sphere coordinates), or NULL: then they are computed from rays_o [N,3] with `radius` (> 0);
 * rays_d [N,3] fp32. embeddings [rows,2] fp32: a 4-level hash grid over D = 2 (offsets int32 [5] on the device, per-level scale
 * log2 and base resolution as foc_grid_encode_forward takes them; linear interpolation, align_corners off), read as fp16.
 * weights fp16: the FFMLP blob of the 32 -> 64 -> 16 network, W0 [64,32] (columns 24..31 zero) | W1 [16,64] (rows 3..15 zero).
 * rgb [N,3] fp16.
 * ------------------------------------------------------------------------- */
int foc_background_forward(const float *rays_o, const float *rays_d, const float *coords, float radius, uint32_t N, const float *embeddings,
                           const int32_t *offsets, float per_level_scale_log2, uint32_t base_resolution, const void *weights, void *rgb,
                           void *stream);
/* grad_rgb [N,3] fp16 -> grad_embeddings [rows,2] fp32 (ADDED to: the caller zero-fills; fp32 atomics, so a row's sum depends on the
 * order of arrival — FOC_DETERMINISTIC: integer sums in a row table of the (then larger) workspace, one add per row) and grad_weights fp32 [64*32 + 16*64] (written whole; padding entries 0; a fixed-order reduction: the same bits on
 * every run). workspace: foc_background_backward_workspace_bytes(N) bytes, no zero fill; `workspace_bytes` = its size, a smaller
 * buffer is refused. The rays take no gradient. */
uint64_t foc_background_backward_workspace_bytes(uint32_t N);
int foc_background_backward(const void *grad_rgb, const float *rays_o, const float *rays_d, const float *coords, float radius, uint32_t N,
                            const float *embeddings, const int32_t *offsets, float per_level_scale_log2, uint32_t base_resolution,
                            const void *weights, float *grad_embeddings, float *grad_weights, void *workspace, uint64_t workspace_bytes,
                            void *stream);

/* ---------------------------------------------------------------------------
 * Triangle meshes (csrc/mesh.hip; no reference binding: nerf/utils.py:512-541 samples model.density on a lattice in 128^3 pieces
 * through the host and calls PyMCubes). Orientation and ordering are DEFINED here; parity with PyMCubes is not pinned.
 *
 * Marching cubes. volume: fp32 u[nx, ny, nz], C-contiguous with z fastest; every dimension >= 2 and nx * ny * nz <= 2^29 (so that
 * V <= 3 * 2^29 and F <= 5 * 2^29 fit uint32 and the indices int32), larger volumes are refused before any launch. thr finite.
 *   A corner is inside iff u >= thr (a NaN is outside). Corner c of a cube sits at offset (c & 1, (c >> 1) & 1, (c >> 2) & 1) in
 *   (x, y, z). The 12 edges are listed axis-major (x, y, z), within an axis by lower corner number. The 256 cases are those of
 *   csrc/mc_table.h, generated by tools/make_mc_table.py (its docstring states the rule); triangles face the outside (lower values).
 *   A vertex belongs to the lattice edge it lies on, owned by the edge's lower endpoint p: t = (thr - u[p]) / (u[p + e] - u[p]) in
 *   fp32, position = index of p plus t along the axis, then origin + position * spacing per axis with one fmaf. It is computed once
 *   per edge: the cubes around an edge share it. Vertices are numbered by (linear index of the owner, axis), triangles by (linear
 *   index of the cube = of its corner 0, table order). Every slot comes from a prefix sum, never from an atomic: the same mesh on
 *   every run and in both deterministic modes.
 * foc_mc_count  fills workspace (foc_mc_workspace_bytes(nx, ny, nz) device bytes, 8-byte aligned, no initialisation needed; 0 is
 *               returned for dimensions that are refused) and writes counts3 [3] uint32 on the device: V, F, and the number of 4096-point
 *               groups that hold a non-finite value on a crossed edge (the caller refuses the volume when it is not 0).
 * foc_mc_emit   after the caller read counts3 (its one synchronisation), with the SAME volume, dimensions, threshold and workspace:
 *               vertices [V,3] fp32, triangles [F,3] int32, and with normals != NULL normals [V,3] fp32. Nothing is written past V / F
 *               rows. origin3 / spacing3: 3 floats each IN HOST MEMORY (NULL: 0 / 1, the lattice-unit result); spacing non-zero.
 *               Normals: the gradient of u by central differences (one-sided on the border) at the edge's two endpoints, mixed as
 *               g0 + t (g1 - g0), divided per axis by the spacing, negated and normalised; a zero gradient gives (0, 0, 0).
 * --------------------------------------------------------------------------- */
uint64_t foc_mc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int foc_mc_count(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float thr, void *workspace, uint32_t *counts3,
                 void *stream);
int foc_mc_emit(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float thr, const void *workspace,
                const float *origin3, const float *spacing3, float *vertices, float *normals, int32_t *triangles, void *stream);

/* The density volume of an object, or of objects placed in a scene, on a lattice: which points need the network at all.
 * Lattice point i (linear, z fastest, of rx * ry * rz <= 2^29 points) stands at (xs[ix], ys[iy], zs[iz]), per-axis fp32 coordinates on
 * the device. A call treats the SLAB of `count` >= 1 points from `first`; bit i % 64 of mask[i / 64] (i counted from the slab's start)
 * is point i's, R = ceil(count / 64) words.
 *   world_to_object / obj_aabb (12 and 6 floats in host memory, both or neither): the point is mapped by foc_fixed_cull_placed's
 *       q_k = ((A_k0 x + A_k1 y) + A_k2 z) + b_k — the same device function — and is empty outside obj_aabb_lo <= q <= obj_aabb_hi.
 *   bitfield (may be NULL, then cascade / grid_size / bound are not read): the point's cell, foc_fixed_cull's, must be occupied.
 * foc_lattice_cull       mask [R] uint64, offsets [R + 1] uint32 (exclusive prefix sum of the words' popcounts), count [1] uint32;
 *                        scratch: foc_lattice_cull_scratch_bytes(count) device bytes. No synchronisation.
 * foc_lattice_cull_emit  pos_c [m_occ,3] fp32: the set points' positions (q with a placement) in lattice order, as the network's
 *                        density(x) takes them; nothing is written past m_occ rows.
 * foc_volume_scatter_max volume[i] = max(volume[i], gain * sigma_c[slot(i)]) at the set bits of a slab of n points (`volume` points at
 *                        the slab's first value); a NaN stays a NaN. Each point is touched once per call, calls run in stream order:
 *                        no atomics. gain finite and > 0 (a placement's 1 / scale). */
uint64_t foc_lattice_cull_scratch_bytes(uint32_t count);
int foc_lattice_cull(const float *xs, const float *ys, const float *zs, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t first,
                     uint32_t count, const float *world_to_object, const float *obj_aabb, float bound, const uint8_t *bitfield,
                     uint32_t cascade, uint32_t grid_size, uint64_t *mask, uint32_t *offsets, uint32_t *count_out, void *scratch,
                     uint64_t scratch_bytes, void *stream);
int foc_lattice_cull_emit(const float *xs, const float *ys, const float *zs, uint32_t rx, uint32_t ry, uint32_t rz, uint32_t first,
                          uint32_t count, const float *world_to_object, const uint64_t *mask, const uint32_t *offsets,
                          uint32_t m_occ, float *pos_c, void *stream);
int foc_volume_scatter_max(const float *sigma_c, const uint64_t *mask, const uint32_t *offsets, float gain, float *volume,
                           uint32_t n, void *stream);

/* A placed scene at ARBITRARY points (csrc/mesh.hip; focnerf_amd/query.py sequences the calls): the lattice cull for a list, the frame
 * of a surface point, and the select that keeps the winning object's density, index, colour and normal per point.
 *
 * foc_points_cull / foc_points_cull_emit: foc_lattice_cull / foc_lattice_cull_emit for points [M,3] fp32 on the device, in world units,
 *   point i in place of lattice point i. The SAME kernels (templates over where a point comes from), hence the same arithmetic in the same
 *   order: q by foc_fixed_cull_placed's device function, the box test, then the cell test, the bitfield read only for points still in
 *   question; a point with a NaN coordinate is never inside a box (every comparison fails). mask [R] uint64, offsets [R + 1] uint32,
 *   count_out [1] uint32 with R = ceil(M / 64); scratch: foc_lattice_cull_scratch_bytes(M) device bytes. M <= 2^29. world_to_object /
 *   obj_aabb: 12 and 6 floats in host memory, both or neither. Refused (FOC_E_INVALID) before anything is enqueued: a null pointer, M > 2^29,
 *   non-finite host arrays, a bad cascade / grid_size / bound with a bitfield, a scratch smaller than asked for. M = 0 returns FOC_OK and
 *   enqueues nothing (no output is written). No host synchronisation.
 *   The emit writes either or both of (a NULL one is skipped; both NULL or m_occ = 0: nothing is enqueued), m_occ rows each and nothing
 *   past them:
 *     pos_c [m_occ,3] fp32  the point in the object's frame: q with world_to_object, the point itself without
 *     xn_c  [m_occ,3] fp32  (pos + bound) / (2 bound): the encoder's coordinates, with the arithmetic (one addition, one division by the
 *                           fp32 product 2 bound) of foc_fixed_cull_emit_placed's enc_in_c. bound finite and > 0 (not read without xn_c).
 *
 * foc_surface_frame: one thread per compacted point, m <= 2^29 of them. grad_raw_c [m,3] fp32 is foc_field_normals' grad_raw of the points
 *   (object frame), pos_c [m,3] their object-frame positions.
 *     n_obj     foc_field_normals' normalise rule — the same device function (csrc/unit_normal.h): m = max|g_d|; zero or a component not
 *               finite: n = 0; else u = g / m, n = -u / sqrt(u.u).
 *     normal_c  [m,3] = rot9 n_obj with that kernel's rotate order (per row fmaf from the product of column 0); n_obj when rot9 is NULL.
 *               rot9: 9 finite floats IN HOST MEMORY, row-major (object -> world).
 *     dirs_c    [m,3], the view direction the colour network is asked about. mode 0 (NORMAL): -n_obj, or (0, 0, -1) where n_obj = 0.
 *               mode 1 (EYE): pos_c - eye_obj at unit length by the same scale-by-max rule in fp32, or (0, 0, -1) where that difference is
 *               zero or not finite; eye_obj: 3 finite floats in host memory, the eye in the OBJECT's frame (mapped in float64 by the
 *               caller and rounded once).
 *   dirs_c or normal_c may be NULL (both: nothing is enqueued). grad_raw_c may be NULL when neither normal_c nor a mode-0 dirs_c is asked
 *   for; pos_c and eye_obj are read in mode 1 with dirs_c only. Refused: another mode, a null pointer that is needed, non-finite host arrays.
 *
 * foc_scene_select: foc_volume_scatter_max's twin with a payload, for a run of n <= 2^29 points (the best_* pointers stand at the run's
 *   first point, mask / offsets are the run's). At every set bit i: v = gain * sigma_c[slot(i)], one fp32 multiply; if v > best_sigma[i]:
 *   best_sigma[i] = v, best_id[i] = object_index, best_rgb[i] = rgb_c[slot], best_normal[i] = normal_c[slot]. rgb_c / best_rgb and
 *   normal_c / best_normal may be NULL in pairs. The comparison is strict: on a tie the earlier call's object stays (the tie rule of
 *   foc_combine_select). A NaN v never wins — this DIFFERS from foc_volume_scatter_max, which propagates a NaN into the volume. Points
 *   whose bit is clear are not touched. Each point is touched once per call and calls run in stream order: no atomics, nothing depends on
 *   the order of arrival, the same bits on every run. gain finite and > 0. n = 0 returns FOC_OK. */
int foc_points_cull(const float *points, uint32_t M, const float *world_to_object, const float *obj_aabb, float bound,
                    const uint8_t *bitfield, uint32_t cascade, uint32_t grid_size, uint64_t *mask, uint32_t *offsets,
                    uint32_t *count_out, void *scratch, uint64_t scratch_bytes, void *stream);
int foc_points_cull_emit(const float *points, uint32_t M, const float *world_to_object, float bound, const uint64_t *mask,
                         const uint32_t *offsets, uint32_t m_occ, float *pos_c, float *xn_c, void *stream);
int foc_surface_frame(const float *grad_raw_c, const float *pos_c, uint32_t m, const float *rot9, int mode, const float *eye_obj,
                      float *dirs_c, float *normal_c, void *stream);
int foc_scene_select(const float *sigma_c, const float *rgb_c, const float *normal_c, const uint64_t *mask, const uint32_t *offsets,
                     float gain, int32_t object_index, float *best_sigma, int32_t *best_id, float *best_rgb, float *best_normal,
                     uint32_t n, void *stream);

/* ---------------------------------------------------------------------------
 * Connected components of a thresholded volume (csrc/components.hip; no reference binding: the reference hands its mesh to trimesh, where
 * `split()` finds the floaters on the host). volume: fp32 u[nx, ny, nz], z fastest, the dimensions foc_mc_count serves (each >= 2,
 * nx * ny * nz <= 2^29); lattice point i is inside iff u[i] >= thr (a NaN is outside): foc_mc_count's rule. Two inside points are
 * connected when they differ by at most 1 in every coordinate (26-connectivity): the eight corners of a marching cube are mutually
 * adjacent, so all inside corners of one cube lie in one component, and putting a component's points below the threshold removes exactly
 * that component's triangles while every other vertex and triangle keeps its bits. A component's label is the SMALLEST LINEAR INDEX among
 * its points: unique, hence the same bits on every run and in both deterministic modes, whatever order the unions ran in. Integer
 * atomics only (atomicMin on the parent words, one atomicAdd per tile-local component for the sizes): nothing is refused under
 * FOC_DETERMINISTIC. FOC_CC_NONE, the label of an outside point, is 0xFFFFFFFF (all bits set; -1 read as int32).
 * foc_cc_label   labels [n] uint32: the component's smallest linear index, FOC_CC_NONE outside. sizes [n] uint32: the component's point
 *                count at sizes[root], 0 everywhere else. counts4 [4] uint32 on the device: components, inside points, largest size,
 *                error flag. workspace: foc_cc_workspace_bytes(nx, ny, nz) device bytes (0 for refused dimensions), 4-byte aligned, no
 *                initialisation needed. Every find / union loop walks strictly down and is capped at n turns all the same; a loop that
 *                reaches its cap sets the error flag and leaves (the result is then not to be used) — no loop can spin.
 * foc_cc_select  out[i] = (labels[i] != FOC_CC_NONE && !keep[labels[i]]) ? fill : volume[i] for n <= 2^29 points; keep [n] uint8 is
 *                indexed by root. out may be volume.
 * Refused with FOC_E_INVALID before any launch, the message names the argument: a null pointer, dimensions foc_mc_count refuses, a
 * non-finite thr, a workspace smaller than foc_cc_workspace_bytes, a NaN fill. No host synchronisation inside either call.
 * --------------------------------------------------------------------------- */
uint64_t foc_cc_workspace_bytes(uint32_t nx, uint32_t ny, uint32_t nz);
int foc_cc_label(const float *volume, uint32_t nx, uint32_t ny, uint32_t nz, float thr, uint32_t *labels, uint32_t *sizes,
                 void *workspace, uint64_t workspace_bytes, uint32_t *counts4, void *stream);
int foc_cc_select(const float *volume, const uint32_t *labels, const uint8_t *keep, float fill, float *out, uint32_t n,
                  void *stream);

/* ---------------------------------------------------------------------------
 * Mesh simplification by vertex clustering on a cell grid (csrc/simplify.hip; no reference binding: the reference hands its mesh to
 * trimesh, where a user decimates on the host). vertices [V,3] fp32, triangles [F,3] int32, V and F <= 2^31 - 1. The grid: origin3 and
 * cell3, 3 floats each IN HOST MEMORY (cell finite and > 0 with a finite 1 / cell), and gx, gy, gz >= 1 with gx * gy * gz <= 2^30;
 * inv = 1.0f / cell in fp32. The definition, which tests/simplify_ref.py states in numpy and the kernels follow bit for bit:
 *   1. Per axis t = (v - origin) * inv — one fp32 subtraction, one fp32 multiplication, never fused, never a division;
 *      c = clamp(floor(t), 0, g - 1); r = clamp(t - float(c), 0, 1); cell number k = (cx * gy + cy) * gz + cz. A vertex outside the
 *      grid belongs to the border cell and counts as lying on its border.
 *   2. A triangle survives iff its three corners lie in three different cells.
 *   3. A cell is kept iff a surviving triangle has a corner in it; kept cells are numbered 0 .. Vc - 1 in rising k. vertex_map[v] is the
 *      number of v's cell, or -1 when that cell is not kept (a vertex no triangle uses; a cell all of whose triangles collapsed): the
 *      output has no unreferenced vertex.
 *   4. The vertex of a kept cell is the mean of ALL input vertices in it: per axis q = (int64)(r * 2^30) (the product is exact), S = the
 *      int64 sum, m = (double)S / (double)count / 2^30, x = fp32(origin + (c + m) * cell) with every double operation rounded on its
 *      own. members = count.
 *   5. Normal: per component the int64 sum of (int64)(clamp(n, -1, 1) * 2^30), a non-finite component counting 0; s / sqrt(sx sx + sy sy
 *      + sz sz) in double, summed left to right, 0 for length 0. Colour: the mean of clamp(c, 0, 1), a NaN counting 0, through the same
 *      fixed point. Object id: that of the member with the smallest vertex index.
 *   6. Output triangles: the survivors in input order, renumbered through vertex_map and rotated so that the smallest number stands
 *      first (orientation is preserved; a closed input gives a closed output, counted with multiplicity).
 * Integer atomics only (64-bit or / add, 32-bit add / max): nothing depends on the order of arrival, the same bits on every run, and
 * nothing is refused under FOC_DETERMINISTIC.
 * foc_simplify_count  fills workspace (foc_simplify_workspace_bytes(V, F, gx, gy, gz) device bytes, 8-byte aligned, no initialisation
 *                     needed; 0 is returned for sizes that are refused) and writes counts4 [4] uint32 on the device: Vc, Fc, the number
 *                     of vertices with a non-finite coordinate, the number of triangles with an index outside [0, V). The caller refuses
 *                     the mesh when either of the last two is not 0. No index is read through before it is range-checked. V = 0 and
 *                     F = 0 are served (Vc = Fc = 0).
 * foc_simplify_emit   after the caller read counts4 (its one synchronisation) and found Vc >= 1, Fc >= 1 and no flag, with the SAME
 *                     mesh, grid and workspace: out_vertices [Vc,3] fp32, members [Vc] int32, vertex_map [V] int32, out_triangles
 *                     [Fc,3] int32, and for each attribute given (normals / colors [V,3] fp32, object_id [V] int32; NULL in pairs with
 *                     its output) out_normals / out_colors [Vc,3] fp32, out_object_id [Vc] int32. accum: foc_simplify_accum_bytes(Vc,
 *                     normals != NULL, colors != NULL) device bytes, 8-byte aligned, zeroed by the call. Nothing is written past Vc / Fc
 *                     rows (the stores are guarded by the totals kept in the workspace as well).
 * Refused with FOC_E_INVALID before any launch, the message names the argument: a null pointer, V or F beyond 2^31 - 1, dims outside
 * the limit, a non-finite origin3, a cell3 that is not finite, not > 0 or whose reciprocal overflows, a workspace or accum smaller than
 * asked for, attribute pointers not in pairs, and for the emit Vc or Fc of 0 or beyond V / F. No host synchronisation inside.
 * --------------------------------------------------------------------------- */
uint64_t foc_simplify_workspace_bytes(uint32_t V, uint32_t F, uint32_t gx, uint32_t gy, uint32_t gz);
uint64_t foc_simplify_accum_bytes(uint32_t Vc, int normals, int colors);
int foc_simplify_count(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t F, const float *origin3,
                       const float *cell3, uint32_t gx, uint32_t gy, uint32_t gz, void *workspace, uint64_t workspace_bytes,
                       uint32_t *counts4, void *stream);
int foc_simplify_emit(const float *vertices, uint32_t V, const int32_t *triangles, uint32_t F, const float *normals,
                      const float *colors, const int32_t *object_id, const float *origin3, const float *cell3, uint32_t gx,
                      uint32_t gy, uint32_t gz, const void *workspace, void *accum, uint64_t accum_bytes, uint32_t Vc, uint32_t Fc,
                      float *out_vertices, float *out_normals, float *out_colors, int32_t *out_object_id, int32_t *vertex_map,
                      int32_t *members, int32_t *out_triangles, void *stream);

/* ---------------------------------------------------------------------------
 * Scoring a combined view (csrc/score.hip; no reference binding: COMBINED.py:335-378 process_images_with_background copies the float
 * image to the host and quantises it with numpy, :267-291 calculate_psnr, :295-332 ssim_rgba / ssim_channel run
 * scipy.ndimage.gaussian_filter forty times per view in float64). H * W in 1 .. 2^30 pixels, B in 1 .. 8 backgrounds, N = H * W,
 * images row-major; anything else is refused (FOC_E_INVALID) before any launch. No atomics anywhere: the same bits on every run, in
 * both modes of FOC_DETERMINISTIC.
 *
 * foc_score_quantize  (:353-366) image4 [B,N,4] fp32, gt [N,4] fp32 (both 16-byte aligned), depth [N] fp32, bgs: B floats IN HOST
 *     MEMORY -> pred_u8 [B,H,W,4], gt_u8 [B,H,W,4] (4-byte aligned), depth_u8 [H,W]; depth and depth_u8 may both be NULL.
 *     A pixel whose own alpha is < 0.5 in fp32 (exactly 0.5 is kept) becomes (bg_b, bg_b, bg_b); alpha is then always 1; every channel
 *     is uint8(trunc(fp32(x) * 255.0f)) — one fp32 multiply and truncation toward zero, numpy's (img * 255).astype(np.uint8), not
 *     round-to-nearest. The ground truth is masked by ITS alpha, and every background starts from the original ground truth (the
 *     reference edits a shared numpy view in place only when the image tensor already lives on the host; that is not reproduced).
 *     Domain: finite inputs in [0, 1] (the composite's clamp, a loaded RGBA image); outside it numpy's cast is itself undefined and
 *     nothing is promised.
 * foc_score_view      pred_u8, gt_u8 as above; taps: the 2 * radius + 1 weights of the filter as float64 IN HOST MEMORY, symmetric,
 *     radius <= 12; C1, C2 >= 0 -> out [B,4] float64 on the device: the sum over r, g, b, a of the squared byte differences (an
 *     integer, exact below 2^53; it passes 2^32 at 800 x 800), then the mean over the pixels of the SSIM map of r, g and b.
 *     The caller computes the taps as scipy does: radius = int(4.0 * sigma + 0.5), w_k = exp(-0.5 / sigma^2 * k^2) for
 *     k = -radius .. radius, divided by their sum. The reference passes window_size = 11, which nothing there reads: sigma 1.5 means
 *     13 taps. Borders are scipy's mode='reflect', the half-sample symmetric form d c b a | a b c d, for any H, W >= 1 (a dimension
 *     smaller than the radius reflects repeatedly): with m = i mod 2n >= 0 the index is m if m < n, else 2n - 1 - m.
 *     Per channel x = byte / 255.0 in float64; the five moments x, y, x^2, y^2, xy are filtered along the rows, then along the
 *     columns, each as w_0 v_0 + sum_j w_j (v_+j + v_-j) with one fma per j; SSIM = (2 mu1 mu2 + C1)(2 s12 + C2) /
 *     ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) with s = E[.] - mu mu, all in float64 (sigma^2 cancels against C2 = 9e-4).
 *     workspace: foc_score_workspace_bytes(H, W, B) device bytes (0 for refused dimensions), 8-byte aligned, no initialisation;
 *     `workspace_bytes` = its size, a smaller buffer is refused. One workgroup per (16 x 16 tile, background) writes its partial
 *     sums there; a second kernel adds them in a fixed order. No synchronisation.
 * --------------------------------------------------------------------------- */
uint64_t foc_score_workspace_bytes(uint32_t H, uint32_t W, uint32_t B);
int foc_score_quantize(const float *image4, const float *depth, const float *gt, const float *bgs, uint32_t H, uint32_t W, uint32_t B,
                       uint8_t *pred_u8, uint8_t *gt_u8, uint8_t *depth_u8, void *stream);
int foc_score_view(const uint8_t *pred_u8, const uint8_t *gt_u8, uint32_t H, uint32_t W, uint32_t B, const double *taps,
                   uint32_t radius, double C1, double C2, double *out, void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * The optimizer step (csrc/optim.hip; no reference binding: the reference trainer runs torch.optim.Adam(betas=(0.9, 0.99), eps=1e-15)
 * under torch's GradScaler, nerf/utils.py:1225-1235): the overflow check of the scaled grads, the decision to skip, the scale update,
 * the unscale and Adam with L2 weight decay, for up to FOC_OPTIM_MAX_TENSORS fp32 tensors per call. Every tensor: param, grad, exp_avg,
 * exp_avg_sq [n] fp32 contiguous (4-byte aligned; 16-byte accesses where all four are 16-byte aligned), step: its 0-dim fp32 counter
 * on the device, lr_tensor: a 0-dim fp32 learning rate on the device or NULL (then `lr`). The descriptors are read on the host and
 * travel in the kernel arguments: nothing of the struct has to outlive the call.
 *
 * Per element, in fp32, one rounding per operation: g = grad * inv_scale; if weight_decay != 0: g = fma(weight_decay, p, g);
 * m = fma(g - m, 1 - beta1, m); v = fma(1 - beta2, g * g, beta2 * v); p = p - step_size * m / (sqrt(v) / bc2 + eps), with
 * step_size = lr / (1 - beta1^t) and bc2 = sqrt(1 - beta2^t) computed in double from the tensor's own counter (t = step + 1) and
 * rounded once, inv_scale = 1 / scale in fp32.
 *
 * Three forms, chosen by the pointers:
 *   scale and growth_tracker (both device, fp32 and int32)     phase FOC_OPTIM_STEP: two launches. The check reads every grad; its last
 *       workgroup decides: skip when any element is not finite; step counters advance unless skipped; scale and tracker follow
 *       torch._amp_update_scale_ (overflow: scale *= backoff_factor, tracker = 0; else tracker += 1 and, when it reaches
 *       growth_interval, scale *= growth_factor if that is finite, tracker = 0). The update then reads only the decision.
 *       A step of MORE than 16 tensors: FOC_OPTIM_CHECK for every group (the check alone), FOC_OPTIM_DECIDE once (tensors are not
 *       read), then for every group the external form below with found_inf = (float *)workspace + 5 and grad_scale =
 *       (float *)workspace + 6, where the decision has left them — all with the same workspace, on one stream.
 *   grad_scale and / or found_inf (device fp32, either may be NULL), scale NULL      somebody else (torch's GradScaler) has checked:
 *       skipped when *found_inf != 0, inv_scale = 1 / *grad_scale (1 without it). Scale and tracker are not touched.
 *   neither                                                    plain Adam.
 * In the last two forms a one-workgroup launch writes the decision and the corrections and advances the counters, then the update runs
 * as above. A skipped step leaves params, moments and counters bit-for-bit; zero_grads != 0 writes zeros to the grads in the same
 * pass — also in a skipped step (the grads of a skipped step are of no use to anybody; torch would leave them).
 * workspace: foc_optim_workspace_bytes(n_tensors) device bytes (0 for n_tensors outside 1 .. 16), 4-byte aligned, ZEROED ONCE by the
 * caller; every call leaves its flag and ticket words at zero again, so steps and graph replays need no memset. One workspace serves
 * one stream at a time.
 * Refused with FOC_E_INVALID before any launch: a null struct; struct_bytes != sizeof(FocOptimStep) or tensor_bytes !=
 * sizeof(FocOptimTensor); n_tensors outside 1 .. 16; a null pointer (tensors, workspace, a tensor's param / grad / exp_avg /
 * exp_avg_sq / step; scale without growth_tracker or the reverse; CHECK or DECIDE without them); a negative size; a beta outside
 * [0, 1); negative eps, lr or weight_decay; a workspace that is too small; a scaler together with external pointers. `stream` is a
 * hipStream_t. No order-dependent sums: FOC_DETERMINISTIC changes nothing here and refuses nothing.
 * --------------------------------------------------------------------------- */
#define FOC_OPTIM_MAX_TENSORS 16
#define FOC_OPTIM_CHUNK 4096 /* elements per chunk: one workgroup of the update */
#define FOC_OPTIM_STEP 0
#define FOC_OPTIM_CHECK 1
#define FOC_OPTIM_DECIDE 2
typedef struct FocOptimTensor {
    float *param, *grad, *exp_avg, *exp_avg_sq, *step;
    const float *lr_tensor;
    int64_t n;
    double lr, beta1, beta2, eps, weight_decay;
} FocOptimTensor;
typedef struct FocOptimStep {
    uint32_t struct_bytes;
    uint32_t tensor_bytes;
    int32_t n_tensors;
    uint32_t phase, zero_grads;
    int32_t growth_interval;
    float growth_factor, backoff_factor;
    const FocOptimTensor *tensors;
    float *scale;
    int32_t *growth_tracker;
    const float *grad_scale, *found_inf;
    void *workspace;
    uint64_t workspace_bytes;
} FocOptimStep;
size_t foc_optim_workspace_bytes(int n_tensors);
int foc_optim_step(const FocOptimStep *step, void *stream);

/* ---------------------------------------------------------------------------
 * The parameter EMA (csrc/optim.hip; the reference trainer runs torch_ema's ExponentialMovingAverage.update() after every optimizer
 * step, nerf/utils.py:739,1125,1256: three torch ops and one temporary per tensor). For a parameter p and its shadow s, both [n] fp32
 * contiguous:
 *     n_upd  <- n_upd + 1                                  (only with num_updates; it starts at 0)
 *     decay_t = min(decay, (1 + n_upd) / (10 + n_upd))     in double; `decay` itself when num_updates is NULL
 *     omd     = float(1 - decay_t)
 *     s      <- s - (s - p) * omd                          three fp32 roundings, no contraction
 * num_updates: one int64 on the device, 8-byte aligned, or NULL. omd is computed once per step on the device and kept in word 7 of
 * the optimizer workspace (float); nothing reads the counter after the launch that advanced it, so steps capture in a graph.
 * advance != 0: this call OPENS the step's EMA — it advances the counter (if there is one) and writes omd; advance == 0: the call uses
 * the omd a call with advance != 0 has left in the same workspace, on the same stream. One step = exactly one call with advance != 0.
 *
 * foc_optim_step_ema  foc_optim_step with shadows: `shadow` is a HOST array of step->n_tensors device addresses (0: that tensor has no
 *     shadow and is updated exactly as foc_optim_step updates it). The update launch applies the rule to the p it has just computed;
 *     16-byte accesses where param, grad, exp_avg, exp_avg_sq and the shadow are all 16-byte aligned, 4-byte accesses otherwise. A
 *     SKIPPED step (overflow) leaves params, moments and step counters as they are, and the shadow still moves toward the unchanged
 *     param by the rule, the counter still advances (the reference calls ema.update() after a skipped scaler.step too). omd is written
 *     where the step record is: by the check's last workgroup (scale / growth_tracker form), by the one-workgroup record launch (the
 *     other two forms), or in phase FOC_OPTIM_DECIDE (shadow may be NULL there: tensors are not read). The launches are those of
 *     foc_optim_step, one for one. A step of more than 16 tensors: advance != 0 in the DECIDE call (scaler form) or in the first
 *     group's call (other forms), 0 in every other call. FOC_OPTIM_CHECK takes no part in the EMA: advance != 0 there is refused.
 *     Refused with FOC_E_INVALID before any launch: everything foc_optim_step refuses; a null shadow array in phase FOC_OPTIM_STEP;
 *     decay outside [0, 1] or not finite; a shadow that is not 4-byte aligned; num_updates not 8-byte aligned.
 * foc_ema_update  the rule alone, for parameters no optimizer step touches and for a bare update: param, shadow (device addresses)
 *     and n (element counts) are three HOST arrays of n_tensors (1 .. FOC_OPTIM_MAX_TENSORS) entries; one launch of one workgroup per
 *     FOC_OPTIM_CHUNK elements that reads p and reads and writes s (16-byte accesses where both are 16-byte aligned). With advance
 *     != 0 every workgroup derives omd from the counter and the last one to finish stores the advanced counter and omd — no separate
 *     launch, and a call whose tensors are all empty still advances. workspace: the optimizer's (foc_optim_workspace_bytes, zeroed
 *     once, one stream at a time). Refused with FOC_E_INVALID before any launch: a null array; n_tensors outside 1 .. 16; decay
 *     outside [0, 1] or not finite; a null or misaligned pointer (param, shadow: 4 bytes; num_updates: 8; workspace: 4); a negative
 *     size; a workspace that is too small.
 * `stream` is a hipStream_t. No order-dependent sums: FOC_DETERMINISTIC changes nothing here and refuses nothing.
 * --------------------------------------------------------------------------- */
int foc_optim_step_ema(const FocOptimStep *step, const uint64_t *shadow, double decay, int64_t *num_updates, uint32_t advance, void *stream);
int foc_ema_update(const uint64_t *param, const uint64_t *shadow, const int64_t *n, int n_tensors, double decay, int64_t *num_updates,
                   uint32_t advance, void *workspace, uint64_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------
 * Training batches and the photometric loss (csrc/batch.hip; no reference binding: the reference builds a batch with torch ops in
 * nerf/provider.py:398-447 NeRFDataset.collate and nerf/utils.py:57-157 get_rays, and its loss in nerf/utils.py:840-899
 * Trainer.train_step). One launch each, no host synchronisation, no float atomics: the same bits on every run, FOC_DETERMINISTIC
 * changes nothing and refuses nothing.
 *
 * Random numbers: Philox4x32-10, stateless (multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9, 0xBB67AE85). key = (seed low
 * 32, seed high 32), counter = (ray index r, step low 32, step high 32, stream). Stream 0: word 0 the pixel, words 1 and 2 the two
 * jitters of the error-map route; stream 1: words 0..2 the background colour. A uniform float is (w >> 8) * 2^-24, in [0, 1); a pixel is
 * (uint64(w) * (H * W)) >> 32 (bias at most H * W / 2^32). Every value of a batch is a pure function of (seed, step, r); the number of
 * workgroups does not change it. foc_philox4x32_10 is that function on the host (ctr: 4 words, key: 2 words -> out: 4 words).
 *
 * foc_batch_sample  images [V,H,W,C] (FOC_U8, FOC_F16 or FOC_F32; C = 3 or 4), poses [V,4,4] fp32, order [V] int32 (an epoch's
 *     permutation), step: one int64, all on the device; view = order[step mod V] (an entry outside 0 .. V-1 is taken mod V). Outputs:
 *     inds [N] int64, rays_o, rays_d, bg_color, gt_rgb [N,3] fp32, view [1] int32.
 *     The pixel (nerf/utils.py:96): the draw above; with inds_coarse [N] int64 (:101-110, cells of the 128 x 128 error map; NULL
 *     without), in fp32 with no contraction: row = min(int(float(c / 128) * sx + u1 * sx), H - 1) with sx = H / 128.f, the column
 *     likewise from c % 128, sy = W / 128.f and u2. inds = row * W + col.
 *     The ray (:131-139): x = ((col + 0.5f) - cx) / fx, y = ((row + 0.5f) - cy) / fy, n = sqrt((x x + y y) + 1), (x, y, 1) / n, then
 *     rays_d[k] = (R[k][0] dx + R[k][1] dy) + R[k][2] dz with R the pose's 3 x 3; rays_o is the pose's translation, bit for bit.
 *     The pixel's value: a uint8 is float(v) / 255.f, an fp16 is widened exactly. linear != 0 (:844-845, color_space 'linear') applies
 *     srgb_to_linear (:52-53) to r, g, b in double, rounded once: x < 0.04045 ? x / 12.92 : pow((x + 0.055) / 1.055, 2.4).
 *     Background and target (:847-858): with C = 4 and random_bg != 0, bg = the three stream-1 floats and gt = rgb * a + bg * (1 - a),
 *     each product and sum its own fp32 operation; otherwise bg = 1 and gt = rgb (C = 3) or the same blend against 1 (C = 4).
 *     The step counter advances inside the launch: every workgroup reads `step` first and takes a ticket when it is done, the last one
 *     writes step + 1 and view and puts the ticket back to zero. A replayed graph draws batch t, t + 1, t + 2 with nothing from the host.
 *     workspace: foc_batch_workspace_bytes() device bytes, 4-byte aligned, ZEROED ONCE by the caller; one workspace serves one stream
 *     at a time. workgroups: 0 for the library's choice, or 1 .. 1024 (a test's way to show that the launch size changes nothing).
 * foc_view_rays     the same ray arithmetic for all H * W pixels of one view, row-major (:127, the evaluation route): pose [4,4] on
 *     the device -> rays_o, rays_d [H*W,3].
 * foc_photo_loss    pred [N,3] (FOC_F32, or FOC_F16 widened exactly), gt [N,3] fp32; kind FOC_LOSS_MSE, or FOC_LOSS_HUBER with delta in
 *     torch.nn.HuberLoss's definition (the reference's commented alternative, delta 0.1). Per component d = pred - gt;
 *     MSE: l = d * d, g = 2 d; Huber: |d| <= delta: l = 0.5f * (d * d), g = d; else l = delta * (|d| - 0.5f * delta), g = +-delta.
 *     ray_loss [N] = ((l0 + l1) + l2) / 3.f (:867); grad [N,3] = g / float(3 N), which is d(mean loss) / d(pred); loss [1] =
 *     float(sum / N) with the sum in double: a fixed tree per workgroup, one slot per workgroup, the last workgroup (a ticket) adds
 *     the slots in index order (:899). With error_map [V,16384] fp32 (NULL without), view [1] int32 and inds_coarse [N] int64:
 *     error_map[view, c] = 0.1f * old + 0.9f * ray_loss (:893-894); the cells are distinct (a draw without replacement), so no
 *     atomics; a view outside 0 .. V-1 updates nothing.
 *     workspace: foc_photo_loss_workspace_bytes() device bytes, 8-byte aligned, ZEROED ONCE by the caller, one stream at a time.
 * Refused before any launch: a null pointer; C not 3 or 4; an unknown dtype (FOC_E_DTYPE) or kind; N < 1; H * W outside 1 .. 2^30;
 * V < 1; intrinsics that are not finite, fx or fy zero; a delta that is not finite and > 0; a workspace that is too small.
 * The caller clamps N to H * W as the reference does (:73).
 * --------------------------------------------------------------------------- */
#define FOC_U8 2 /* image dtype of foc_batch_sample, beside FOC_F32 and FOC_F16 */
#define FOC_LOSS_MSE 0
#define FOC_LOSS_HUBER 1
#define FOC_PHOTO_LOSS_MAX_WGS 256 /* slots of the loss's workspace */
int foc_philox4x32_10(const uint32_t *ctr, const uint32_t *key, uint32_t *out);
uint64_t foc_batch_workspace_bytes(void);
int foc_batch_sample(const void *images, int image_dtype, uint32_t V, uint32_t H, uint32_t W, uint32_t C, const float *poses, float fx,
                     float fy, float cx, float cy, const int32_t *order, int64_t *step, uint64_t seed, uint32_t N,
                     const int64_t *inds_coarse, int random_bg, int linear, int64_t *inds, float *rays_o, float *rays_d, float *bg_color,
                     float *gt_rgb, int32_t *view, void *workspace, uint64_t workspace_bytes, uint32_t workgroups, void *stream);
int foc_view_rays(const float *pose, float fx, float fy, float cx, float cy, uint32_t H, uint32_t W, float *rays_o, float *rays_d,
                  void *stream);
uint64_t foc_photo_loss_workspace_bytes(void);
int foc_photo_loss(const void *pred, int pred_dtype, const float *gt, uint32_t N, int kind, float delta, float *error_map, uint32_t V,
                   const int32_t *view, const int64_t *inds_coarse, float *ray_loss, float *grad, float *loss, void *workspace,
                   uint64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FOCNERF_H */
