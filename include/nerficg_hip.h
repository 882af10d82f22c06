/*
 * nerficg_hip.h -- C ABI of libnerficg_hip.so, the MI355X (gfx950) replacement for the native ops behind
 * nerficg's src/Methods plugins.  Plain pointers + sizes, no torch types.  All pointers are DEVICE pointers unless a
 * parameter is documented as host.  `stream` is a hipStream_t passed as void* (NULL = the null stream).
 * Every function returns NRC_OK (0) or a negative NRC_ERR_* code; nothing is allocated and nothing synchronises
 * inside the library (workspaces are caller-provided), so every entry point is hipGraph-capturable.
 *
 * Each group cites the reference interface it replaces (paths relative to the nerficg repository root).
 */
#ifndef NERFICG_HIP_H
#define NERFICG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* nrc_stream_t;

enum {
    NRC_OK = 0,
    NRC_ERR_INVALID = -1, /* bad argument (null pointer, negative size, unsupported configuration) */
    NRC_ERR_LAUNCH = -2,  /* hipGetLastError() != hipSuccess after a launch */
    NRC_ERR_UNSUPPORTED = -3
};

/* Version of THIS header's contract (signatures, buffer sizes, meaning of the counters).  Bumped on every incompatible change; a caller
 * compares nrc_abi_version() of the library it loaded with the NRC_ABI_VERSION it was built against and refuses a mismatch (a stale .so under
 * newer bindings -- or the reverse -- would pass a stream where a pointer is expected, or under-allocate a workspace).
 * History: 1 = rounds 1-2; 2 = round 3 (nrc_gs_backward gained grad_records, nrc_ngp_render_count writes 2 * n_tiles ints into tile_rows,
 * counter[1] = total samples, save buffers padded to nrc_nwie_save_rows); 3 = round 4 (see the notes at the changed entry points);
 * 4 = round 4, later: nrc_gs_preprocess and nrc_ngp_render_count gained count_mailbox / mailbox_ticket, nrc_host_mailbox_alloc / _free are new;
 * nrc_ngp_query_samples gained arena_tile_off / arena_rows, nrc_ngp_composite_image arena_rows, nrc_ngp_render_write accepts ts = NULL;
 * nrc_photometric_loss_* are new; 5 = round 5: group 13 (the fused InstantNGP training iteration) is new; nrc_ngp_train_query_forward gained
 * n_samples_dev (NULL = every row, as before); 7 = the band entry points of group 4 (nrc_gs_*_band: one frame rendered and differentiated as bands of tile
 * rows) are new, every earlier signature is unchanged; 8 = nrc_gs_bin_render_aux_band / nrc_gs_backward_aux_band (group 4: differentiable depth and alpha maps
 * beside the colour) are new, float [3].w of a splat record carries the view-space depth, slot [9] of a gradient record dL/dz; every earlier signature is unchanged;
 * 9 = group 15 (nrc_map_losses_*: the depth-smoothness and alpha-entropy losses on the rasterizer's maps) is new, every earlier signature is unchanged;
 * 10 = nrc_ngp_set_encoder_xcd_run (group 6) is new, every earlier signature is unchanged;
 * 11 = nrc_ngp_set_encoder_block_levels / _block_view, nrc_ngp_block_view_bytes, nrc_ngp_build_block_view (group 6: the cell-block view of the dense
 * levels) are new, every earlier signature is unchanged;
 * 12 = nrc_ngp_render_count_rays (group 6: the count pass for a caller's own ray list) is new, every earlier signature is unchanged;
 * 13 = nrc_grid_backward_input / nrc_sh_identity_backward_input (group 3: the encodings' derivatives with respect to their input) are new, every
 * earlier signature is unchanged;
 * 14 = nrc_gs_pose_partials_floats / nrc_gs_backward_pose_band / nrc_gs_camera_block_backward (group 4: gradients to the camera pose) are new, every
 * earlier signature is unchanged;
 * 15 = group 16 (nrc_gs_mcmc_*: the relocation, SGLD noise and regularisers of 3DGS-MCMC) is new, every earlier signature is unchanged;
 * 16 = group 17 (nrc_nerf_*: the vanilla NeRF block's inference forward as one kernel) is new, every earlier signature is unchanged;
 * 17 = group 18 (the vanilla NeRF block's training forward and backward) is new, every earlier signature is unchanged;
 * 18 = group 19 (nrc_nerf_rays_* / nrc_nerf_sample_* / nrc_nerf_integrate_*: NeRF sampling, compositing and resampling) is new, every earlier signature is
 * unchanged;
 * 19 = group 20 (the vanilla NeRF path's gradients to sample positions, viewing directions and rays) is new, every earlier signature is unchanged;
 * 20 = group 21 (nrc_gs_render_features_band / nrc_gs_backward_features_band: N-channel per-Gaussian features blended by the rasterizer's weights) is new,
 * every earlier signature is unchanged;
 * 21 = group 22 (nrc_gs_contributions_band: per-Gaussian contribution statistics of a rendered view) is new, every earlier signature is unchanged;
 * 22 = nrc_ngp_set_encoder_vertex_levels / _vertex_view, nrc_ngp_vertex_view_bytes, nrc_ngp_build_vertex_view (group 6: the vertex view of the leading
 * hashed levels) are new, every earlier signature is unchanged.  Added under 22 without a bump (additive: no earlier signature, record slot or default
 * launch changes): group 23, nrc_gs_backward_absgrad_band -- slots [10], [11] of a gradient record carry sum_pixels |dL_pixel/dmean2D| in that call only;
 * group 24, nrc_adam_step_rows_multi -- the visibility-masked Adam step, a new entry in a translation unit of its own; group 25,
 * nrc_ngp_set_encoder_ypair_levels / _ypair_view, nrc_ngp_ypair_view_bytes, nrc_ngp_build_ypair_view -- the y-pair view of the leading hashed levels, read
 * only by a call that was handed one; group 26, nrc_ngp_set_frame_density_encoder -- the single-pass frame's kernel pair (the workspace of
 * nrc_ngp_render_frame is what it was, the pictures are the same bits); group 27, nrc_gs_preprocess_antialias_band / nrc_gs_backward_antialias_band /
 * nrc_gs_filter3d -- anti-aliased splats and the 3-D smoothing filter: instances and a kernel of their own, no existing launch changes; group 28,
 * nrc_bilagrid_* -- bilateral-grid colour correction (slice, total variation, their gradients), a translation unit of its own; group 29,
 * nrc_ngp_density_frag_image -- the density net's weights as ready-made MFMA fragments, the 6 KB image that nrc_ngp_render_frame now writes into a
 * new trailing part of its workspace (nrc_ngp_render_frame_ws_bytes grows by 6 144 bytes; signatures and pictures are what they were); group 30,
 * nrc_ngp_set_frame_full_encoder / nrc_ngp_colour_frag_image -- the single-pass frame's third form (both nets inside the encoder, 8-byte records, one
 * compositor launch) and the colour net's 14 KB fragment image, which the workspace now holds directly in front of the density image
 * (nrc_ngp_render_frame_ws_bytes grows by 14 336 bytes; signatures and pictures are what they were). */
#define NRC_ABI_VERSION 22
/* library identification; also used by the loader's symbol check */
int nrc_abi_version(void);
const char* nrc_build_info(void);
/* text of the HIP error behind the calling thread's most recent NRC_ERR_LAUNCH */
const char* nrc_last_error(void);

/* =====================================================================================================
 * Group 1 -- VolumeRenderingV2  (replaces the pybind module of
 *            src/Methods/InstantNGP/VolumeRenderingV2/csrc/binding.cpp:234-250)
 * dtypes are fixed like in the reference: f32 data, i64 rays_a / alive_indices / hits_voxel_idx,
 * i32 counter / N_eff_samples / Morton codes, u8 bitfield.  All arrays dense row-major.
 * ===================================================================================================== */

/* binding.cpp:4-16 -> intersection.cu:59-100.  hits_t (n_rays,max_hits,2) and hits_voxel_idx (n_rays,max_hits) are
 * fully written (-1 fill, then hits, then sorted ascending by t1 like the reference's torch::sort). hit_cnt (n_rays). */
int nrc_ray_aabb_intersect(const float* rays_o, const float* rays_d, const float* centers, const float* half_sizes,
                           int64_t n_rays, int64_t n_voxels, int32_t max_hits, int32_t* hit_cnt, float* hits_t,
                           int64_t* hits_voxel_idx, nrc_stream_t stream);
/* binding.cpp:19-31 -> intersection.cu:156-196 */
int nrc_ray_sphere_intersect(const float* rays_o, const float* rays_d, const float* centers, const float* radii,
                             int64_t n_rays, int64_t n_spheres, int32_t max_hits, int32_t* hit_cnt, float* hits_t,
                             int64_t* hits_sphere_idx, nrc_stream_t stream);
/* binding.cpp:46-50 -> raymarching.cu:72-88.  coords (n,3) i32 -> indices (n) i32 */
int nrc_morton3D(const int32_t* coords, int64_t n, int32_t* indices, nrc_stream_t stream);
/* binding.cpp:53-57 -> raymarching.cu:103-119 */
int nrc_morton3D_invert(const int32_t* indices, int64_t n, int32_t* coords, nrc_stream_t stream);
/* binding.cpp:34-43 -> raymarching.cu:143-161.  grid_dtype: 0 = f32, 1 = f16.  n_bytes = len(bitfield); grid has 8*n_bytes cells. */
int nrc_packbits(const void* density_grid, int32_t grid_dtype, int64_t n_bytes, float density_threshold,
                 uint8_t* density_bitfield, nrc_stream_t stream);

/* binding.cpp:60-81 -> raymarching.cu:283-332, split in two calls so that the caller can allocate exactly
 * counter[0] sample rows instead of the reference's n_rays*max_samples zero-filled rows.
 *   _count : marches every ray once, writes rays_a (n_rays,3) = (ray_idx, start_idx, n_samples) in RAY ORDER with
 *            start_idx = exclusive prefix sum (deterministic; the reference's order is atomic-arrival order) and
 *            counter[0] = total samples, counter[1] = n_rays.  workspace: nrc_raymarching_train_ws_bytes(n_rays, max_samples) bytes;
 *            for batches of <= 32768 rays the pass also parks every sample's t there (max_samples f32 per ray).
 *   _write : writes xyzs/dirs (total,3), deltas/ts (total): with the workspace of the count pass it expands the parked positions
 *            (no second march); with workspace == NULL it marches again. */
int64_t nrc_raymarching_train_ws_bytes(int64_t n_rays, int32_t max_samples);
int nrc_raymarching_train_count(const float* rays_o, const float* rays_d, const float* hits_t,
                                const uint8_t* density_bitfield, int32_t cascades, float scale, float exp_step_factor,
                                const float* noise, int32_t grid_size, int32_t max_samples, int64_t n_rays,
                                int64_t* rays_a, int32_t* counter, void* workspace, nrc_stream_t stream);
/* nrc_raymarching_train_count for batches of at most 32 768 rays as TWO launches (wave-per-ray march + one workgroup that scans the counts: no block
 * sums to clear, no separate assignment pass), whose scan also stores (total samples, n_rays, mailbox_ticket) in HOST memory from
 * nrc_host_mailbox_alloc (group 4) -- the caller polls the ticket and sizes xyzs / dirs / deltas / ts without a device-to-host copy or a stream wait
 * (the one host read of the reference's training march, custom_functions.py:112-119).  Same rays_a / counter / parked positions as the plain call. */
int nrc_raymarching_train_count_posted(const float* rays_o, const float* rays_d, const float* hits_t, const uint8_t* density_bitfield, int32_t cascades,
                                       float scale, float exp_step_factor, const float* noise, int32_t grid_size, int32_t max_samples, int64_t n_rays,
                                       int64_t* rays_a, int32_t* counter, void* workspace, int64_t* count_mailbox, int64_t mailbox_ticket,
                                       nrc_stream_t stream);
int nrc_raymarching_train_write(const float* rays_o, const float* rays_d, const float* hits_t,
                                const uint8_t* density_bitfield, int32_t cascades, float scale, float exp_step_factor,
                                const float* noise, int32_t grid_size, int32_t max_samples, int64_t n_rays,
                                const int64_t* rays_a, float* xyzs, float* dirs, float* deltas, float* ts,
                                const void* workspace, nrc_stream_t stream);
/* The ray preparation of InstantNGPRenderer.render_rays (Renderer.py:55-77: origin - centre, ray_aabb_intersect against the scene box,
 * clamp of the interval to [near, far]) as ONE launch: origin_centred (n,3), spans (n,2) = (t_in, t_out), a miss is (near, -1).
 * center3 / half3: HOST float[3].  Same values as nrc_ray_aabb_intersect + the two torch clamps. */
int nrc_ngp_clip_rays(int64_t n_rays, const float* origin, const float* dirs, const float* center3, const float* half3,
                      float near_plane, float far_plane, float* origin_centred, float* spans, nrc_stream_t stream);
/* What render_rays_training does with the composited sums (Renderer.py:80-84), one launch each way: rgb_out = rgb + (1 - opacity) * bg,
 * depth_out = depth / (opacity + 1e-6); bg_dev: DEVICE float[3].  _bw turns the gradients of (rgb_out, opacity as alpha, depth_out) --
 * each may be NULL -- into dL_dopacity / dL_ddepth for nrc_composite_train_bw (dL_drgb is g_rgb itself).  nrc_composite_train_bw accepts
 * NULL for dL_dopacity, dL_ddepth and dL_dws (no gradient reached that output). */
int nrc_ngp_train_pixels_fw(int64_t n_rays, const float* opacity, const float* depth, const float* rgb, const float* bg_dev,
                            float* rgb_out, float* depth_out, nrc_stream_t stream);
int nrc_ngp_train_pixels_bw(int64_t n_rays, const float* g_rgb, const float* g_alpha, const float* g_depth, const float* opacity,
                            const float* depth, const float* bg_dev, float* dL_dopacity, float* dL_ddepth, nrc_stream_t stream);
/* Fixed-capacity variant for graph capture (no host read of counter[0] between _count and _write): call between the two passes with
 * sample buffers of `sample_capacity` rows.  Rays whose segment would cross the capacity keep the samples that fit (n_samples in rays_a is
 * cut, start_idx <= sample_capacity), rows [min(counter[0], capacity), capacity) are filled with inert samples (position = box centre,
 * direction +z, delta = t = 0) that no ray references.  counter[0] keeps the uncut total: counter[0] > sample_capacity <=> samples were
 * dropped.  The reference has no counterpart: it allocates n_rays*max_samples rows and slices by counter[0] on the host
 * (custom_functions.py:112-119). */
int nrc_raymarching_train_cap(int64_t n_rays, int64_t sample_capacity, const int32_t* counter, int64_t* rays_a, float* xyzs,
                              float* dirs, float* deltas, float* ts, nrc_stream_t stream);
/* Same, and *overflow (device int64, may be NULL) = max(counter[0] - sample_capacity, 0): the number of dropped samples without two more
 * element-wise launches in a recorded iteration. */
int nrc_raymarching_train_cap_overflow(int64_t n_rays, int64_t sample_capacity, const int32_t* counter, int64_t* rays_a, float* xyzs,
                                       float* dirs, float* deltas, float* ts, int64_t* overflow, nrc_stream_t stream);
/* count + cap + write for a batch of at most 32 768 rays with a fixed sample capacity, as THREE launches (march with parked positions, one
 * workgroup that scans the per-ray counts and writes the cut rays_a / counter / *overflow, expansion of the parked positions + inert tail):
 * what nrc_raymarching_train_count, _cap_overflow and _write do in seven.  workspace: nrc_raymarching_train_ws_bytes(n_rays, max_samples). */
int nrc_raymarching_train_capped(const float* rays_o, const float* rays_d, const float* hits_t, const uint8_t* density_bitfield, int32_t cascades,
                                 float scale, float exp_step_factor, const float* noise, int32_t grid_size, int32_t max_samples, int64_t n_rays,
                                 int64_t sample_capacity, int64_t* rays_a, int32_t* counter, float* xyzs, float* dirs, float* deltas, float* ts,
                                 int64_t* overflow, void* workspace, nrc_stream_t stream);
/* The batch of a training iteration out of the resident ray pool (RayPoolSampler.get, src/Optim/Samplers/DatasetSamplers.py:53-66:
 * ray_pool[indices], one fancy-index gather per field) as ONE launch: rows ids[i] of up to four pools of the same length -- three of
 * row width 3 (origin, view direction, rgb; any may be NULL) and one of width 1 (alpha; may be NULL) -- into dense outputs.
 * ids: int64, -n_pool <= ids[i] < n_pool; a negative id counts from the end like torch's indexing; an id out of range (torch: device
 * assert) writes a NaN row, so a broken sampler shows up in the loss / the GradScaler's check instead of training on black rays. */
int nrc_gather_ray_batch(const int64_t* ids, int64_t n, int64_t n_pool, const float* pool_a3, const float* pool_b3, const float* pool_c3,
                         const float* pool_d1, float* out_a3, float* out_b3, float* out_c3, float* out_d1, nrc_stream_t stream);
/* The colour term of the InstantNGP loss with the GradScaler's multiplication folded in (Trainer.py:87-89: mse_loss(rgb, target),
 * scaler.scale(loss)): out2[0] = mean((pred - target)^2) over n values, out2[1] = out2[0] * *scale (scale: DEVICE float, NULL = 1).
 * One workgroup, fixed summation order (the result does not depend on the run).  _backward: grad_pred = 2 / n * (pred - target) *
 * (g_loss + g_scaled * scale); g_loss / g_scaled: DEVICE floats, either may be NULL (no gradient reached that output).  Replaces
 * seven element-wise / reduction launches of the op-by-op expression in a recorded iteration.  n <= 2^24. */
int nrc_mse_scaled_forward(int64_t n, const float* pred, const float* target, const float* scale, float* out2, nrc_stream_t stream);
int nrc_mse_scaled_backward(int64_t n, const float* pred, const float* target, const float* scale, const float* g_loss,
                            const float* g_scaled, float* grad_pred, nrc_stream_t stream);
/* binding.cpp:84-106 -> raymarching.cu:407-454.  hits_t (n_total_rays,2) is advanced in place.  Outputs
 * (n_alive,N_samples[,3]) are fully written (zero beyond N_eff_samples), N_eff_samples (n_alive) i32. */
int nrc_raymarching_test(const float* rays_o, const float* rays_d, float* hits_t, const int64_t* alive_indices,
                         int64_t n_alive, const uint8_t* density_bitfield, int32_t cascades, float scale,
                         float exp_step_factor, int32_t grid_size, int32_t max_samples, int32_t N_samples, float* xyzs,
                         float* dirs, float* deltas, float* ts, int32_t* N_eff_samples, nrc_stream_t stream);

/* binding.cpp:109-126 -> volumerendering.cu:48-84.  rays_a (n_rays,3) i64; sample arrays have n_samples rows.
 * Outputs are fully written: total_samples (n_rays) i64, opacity/depth (n_rays), rgb (n_rays,3), ws (n_samples). */
int nrc_composite_train_fw(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                           const int64_t* rays_a, int64_t n_rays, int64_t n_samples, float T_threshold,
                           int64_t* total_samples, float* opacity, float* depth, float* rgb, float* ws,
                           nrc_stream_t stream);
/* binding.cpp:129-163 -> volumerendering.cu:154-202 */
int nrc_composite_train_bw(const float* dL_dopacity, const float* dL_ddepth, const float* dL_drgb, const float* dL_dws,
                           const float* sigmas, const float* rgbs, const float* ws, const float* deltas, const float* ts,
                           const int64_t* rays_a, const float* opacity, const float* depth, const float* rgb,
                           int64_t n_rays, int64_t n_samples, float T_threshold, float* dL_dsigmas, float* dL_drgbs,
                           nrc_stream_t stream);
/* binding.cpp:166-194 -> volumerendering.cu:252-285.  In place on opacity/depth/rgb (n_total_rays[,3]) and on
 * alive_indices (entries of dead rays become -1). */
int nrc_composite_test_fw(const float* sigmas, const float* rgbs, const float* deltas, const float* ts,
                          int64_t* alive_indices, int64_t n_alive, int32_t N_samples, float T_threshold,
                          const int32_t* N_eff_samples, float* opacity, float* depth, float* rgb, nrc_stream_t stream);
/* Backward of raymarching_train w.r.t. the rays (the reference does this in Python with torch_scatter.segment_csr,
 * custom_functions.py:122-137): row n of rays_a = (ray, start, count) gets dL_drays_o[n] = sum dL_dxyzs[start:start+count] and
 * dL_drays_d[n] = sum (ts * dL_dxyzs + dL_ddirs)[start:start+count].  dL_ddirs may be NULL (no gradient reached the directions). */
int nrc_raymarching_train_bw(const float* dL_dxyzs, const float* dL_ddirs, const float* ts, const int64_t* rays_a, int64_t n_rays,
                             int64_t n_samples, float* dL_drays_o, float* dL_drays_d, nrc_stream_t stream);
/* binding.cpp:197-209 -> losses.cu:64-109 */
int nrc_distortion_loss_fw(const float* ws, const float* deltas, const float* ts, const int64_t* rays_a, int64_t n_rays,
                           int64_t n_samples, float* loss, float* ws_inclusive_scan, float* wts_inclusive_scan,
                           nrc_stream_t stream);
/* binding.cpp:212-231 -> losses.cu:145-174 */
int nrc_distortion_loss_bw(const float* dL_dloss, const float* ws_inclusive_scan, const float* wts_inclusive_scan,
                           const float* ws, const float* deltas, const float* ts, const int64_t* rays_a, int64_t n_rays,
                           int64_t n_samples, float* dL_dws, nrc_stream_t stream);

/* =====================================================================================================
 * Group 2 -- MortonEncoding._C  (replaces src/CudaUtils/MortonEncoding/MortonEncoding/morton_encoding.cu:48-79)
 * positions (n,3) f32 -> codes (n) i64.  The bounding cube (reference: host aminmax, :54-57) is reduced on device
 * into `workspace` (nrc_morton_encode_ws_bytes(n) bytes) by the same call.
 * ===================================================================================================== */
int64_t nrc_morton_encode_ws_bytes(int64_t n);
int nrc_morton_encode(const float* positions, int64_t n, int64_t* codes, void* workspace, nrc_stream_t stream);

/* =====================================================================================================
 * Group 3 -- tinycudann subset  (replaces the tiny-cuda-nn modules built at src/Methods/InstantNGP/Model.py:58-114 and
 *            queried at src/Methods/InstantNGP/Renderer.py:48-60; external dependency src/Thirdparty/TinyCudaNN.py:10)
 * Networks: input encoding (32 features) -> 64-wide ReLU MLP (n_hidden 1 or 2, no bias) -> 16 padded outputs.
 *   encoding 0: multiresolution hash grid, fp16 table of nrc_grid_layout()[n_levels] entries x F features; F = (encoding >> 8) & 0xff (0 = 2).
 *               16 levels x 2 features (the shipped yaml) runs on the tuned kernels; any other F in {2, 4} with n_levels * F <= 32 -- what
 *               HASHGRID_N_LEVELS / HASHGRID_N_FEATURES_PER_LEVEL of src/Methods/InstantNGP/Model.py:18-29 can ask for within the 32 first-layer
 *               inputs -- on a general kernel (input k = level * F + c, zero behind n_levels * F; backward: nrc_grid_backward_general)
 *   encoding 1: [SphericalHarmonics degree 4 of input dims 0..2 | Identity of input dims 3..18]
 * weights_f16: [W0 (64,32) | hidden (64,64) x (n_hidden-1) | Wout (16,64)] row-major fp16 (rows >= n_out_rows read as 0).
 * ===================================================================================================== */

/* HOST helper: entry offsets of the levels, offsets_host[n_levels+1] (last = total entries); NULL only validates */
int nrc_grid_layout(int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                    uint32_t* offsets_host);
/* backward of the general grid: d_in (M,32) f32 as nrc_nwie_backward writes it with d_in_pair_major = 0; grad_table (entries, F) f32, ACCUMULATED */
int nrc_grid_backward_general(const float* x01, int64_t M, const float* d_in, int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size,
                              int32_t base_resolution, float per_level_scale, float* grad_table, nrc_stream_t stream);
/* fp32 master parameters -> fp16 compute copy */
int nrc_f32_to_f16(const float* src, void* dst_f16, int64_t n, nrc_stream_t stream);
/* NetworkWithInputEncoding.forward.  input: encoding 0 -> (M,3) f32 in [0,1], input_ld ignored; encoding 1 -> (M,input_ld>=19)
 * fp16 rows [d01(3) | features(16)].  out_act: 0 none, 1 sigmoid.  out (M,out_ld) fp16, columns [0,n_store) written
 * (n_store in {4,8,12,16}).  save_in (R,32) fp16 and save_acts (n_hidden,R,64) fp16, R = nrc_nwie_save_rows(M) (M rounded up to whole
 * 32-sample tiles), receive the encoded inputs and the post-ReLU activations for the backward pass (both NULL for inference) in a
 * layout private to the two calls (MFMA-fragment-major, so that both sides move whole cache lines).  Of a network with two hidden layers only the FIRST layer's
 * activations are written (the buffer keeps its documented size): the backward pass recomputes the second from the first with the forward's own eight matrix
 * instructions per 32 samples -- 128 B per sample less in either direction (round 6). */
int64_t nrc_nwie_save_rows(int64_t M);
/* workspace (optional, grid encoding only): nrc_nwie_forward_ws_bytes(M) bytes -> the encoding runs as its own kernel (faster);
 * NULL -> one kernel gathers and runs the MLP. */
int64_t nrc_nwie_forward_ws_bytes(int64_t M);
int nrc_nwie_forward(int32_t encoding, const void* input, int32_t input_ld, int64_t M, const void* weights_f16,
                     const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution,
                     float per_level_scale, int32_t n_hidden, int32_t out_act, int32_t n_out_rows, void* out_f16,
                     int32_t out_ld, int32_t n_store, void* save_in, void* save_acts, void* workspace, nrc_stream_t stream);
/* NetworkWithInputEncoding.backward through the MLP.  d_out / out: (M,out_ld) fp16 (upstream gradient of, and the forward
 * value of, the stored output columns).  Upstream gradients are multiplied by loss_scale before they are rounded to fp16
 * MFMA operands and every result is divided by it again (tiny-cuda-nn's internal loss scale).  grad_weights: f32, layout
 * of weights_f16, ACCUMULATED atomically (caller zeroes).  d_in f32 = gradient w.r.t. the 32 encoded inputs, laid out (M,32)
 * (d_in_pair_major = 0) or as 16 feature pairs [16][M][2] (d_in_pair_major = 1: the layout nrc_grid_backward reads coalesced). */
int nrc_nwie_backward(int64_t M, const void* weights_f16, int32_t n_hidden, int32_t out_act, int32_t n_out_rows,
                      const void* d_out_f16, const void* out_f16, int32_t out_ld, const void* save_in,
                      const void* save_acts, float loss_scale, float* grad_weights, float* d_in, int32_t d_in_pair_major,
                      nrc_stream_t stream);
/* hash-grid backward: grad_table (entries,2) f32 += trilinear scatter of d_features f32, (M, 2*n_levels) or pair-major
 * [n_levels][M][2] (caller zeroes grad_table).  workspace: optional (NULL allowed), nrc_grid_backward_ws_bytes(...) bytes, 16-byte
 * aligned -- with it (and pair-major gradients, M >= 16384) the hashed levels are split into per-slice record buckets once and
 * accumulated in LDS by one workgroup per slice instead of by atomics */
int64_t nrc_grid_backward_ws_bytes(int64_t M, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution,
                                   float per_level_scale);
int nrc_grid_backward(const float* x01, int64_t M, const float* d_features, int32_t d_features_pair_major, int32_t n_levels,
                      int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, float* grad_table,
                      void* workspace, nrc_stream_t stream);
/* nrc_grid_backward over the rows that hold samples: n_samples_dev (DEVICE i32[1]) <= M, the capacity the launch and the workspace are sized for
 * (the pair-major layout of d_features keeps following M).  NULL = all M rows. */
int nrc_grid_backward_live(const float* x01, int64_t M, const float* d_features, int32_t d_features_pair_major, int32_t n_levels,
                           int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, float* grad_table, void* workspace,
                           const int32_t* n_samples_dev, nrc_stream_t stream);
/* Gradients with respect to the encodings' INPUT (ABI 13): what tiny-cuda-nn's NetworkWithInputEncoding hands back for `x`, behind the d_in of
 * nrc_nwie_backward.  Both validate before any launch (NRC_ERR_INVALID: M < 0, a null pointer with M > 0, n_features outside {2, 4},
 * n_levels * n_features > 32, the pair-major layout with n_features = 4, input_ld < 19, a grid nrc_grid_layout refuses), use no atomics and no
 * workspace, write every row of their output (nothing to zero) and give the same bits on every call.
 *
 * nrc_grid_backward_input: d_x01 (M,3) f32 = sum over levels and features of d_features * d(feature)/d(x01).  d_features is d_in in either layout
 *   nrc_nwie_backward writes -- (M,32) f32 rows with column level * F + c (16-byte aligned), or pair-major [n_levels][M][2] (F = 2 only).  The
 *   derivative is the piecewise one of the cell the forward pass interpolated in (cell and fractions: fmaf(scale, x, 0.5) in f32 and its floor) and
 *   ignores the forward's final fp16 rounding of the feature, as tiny-cuda-nn does.  table_f16: the forward's table, (entries, F) fp16.  A row of
 *   d_features that is all zero reads nothing from the table and yields zeros.
 * nrc_sh_identity_backward_input: input_f16 (M,input_ld >= 19) fp16 rows [d01(3) | features(16)] as nrc_nwie_forward (encoding 1) read them; d_in
 *   (M,32) f32, sample-major; d_input (M,19) f32: columns 0-2 = sum_c d_in[c] dSH_c/dd01 at the fp16 input (d = 2 d01 - 1, the 16 coefficients of
 *   degree 4), columns 3-18 = d_in[16:32]. */
int nrc_grid_backward_input(const float* x01, int64_t M, const float* d_features, int32_t d_features_pair_major, const void* table_f16,
                            int32_t n_levels, int32_t n_features, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                            float* d_x01, nrc_stream_t stream);
int nrc_sh_identity_backward_input(const void* input_f16, int32_t input_ld, int64_t M, const float* d_in, float* d_input, nrc_stream_t stream);
/* query_model (src/Methods/InstantNGP/Renderer.py:48-53) for TRAINING as one forward and one backward call instead of ~55 small
 * launches: world positions xyzs (M,3) / directions dirs (M,3) f32 -> sigmas (M), rgbs (M,3) f32 (what VolumeRenderer consumes), and
 * dL/dsigmas, dL/drgbs -> gradients of both parameter vectors (ACCUMULATED; caller zeroes; layout of the tinycudann modules).
 * Kept between the calls: x01 (M,3) f32, h (M,16) f16, rgb (M,4) f16, save_in_* (R,32) f16, save_acts_d (1,R,64) / save_acts_c (2,R,64) f16,
 * R = nrc_nwie_save_rows(M).
 * forward workspace: nrc_ngp_train_query_ws_bytes(M); backward scratch: nrc_ngp_train_query_scratch_bytes(M). */
int64_t nrc_ngp_train_query_ws_bytes(int64_t M);
int64_t nrc_ngp_train_query_scratch_bytes(int64_t M);
int nrc_ngp_train_query_forward(const float* xyzs, const float* dirs, int64_t M, const float* xyz_min3, const float* xyz_size3,
                                const void* density_weights_f16, const void* color_weights_f16, const void* table_f16,
                                int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                                float* x01, void* h_f16, void* rgb_f16, float* sigmas, float* rgbs, void* save_in_d,
                                void* save_acts_d, void* save_in_c, void* save_acts_c, void* workspace,
                                const int32_t* n_samples_dev, nrc_stream_t stream);
int nrc_ngp_train_query_backward(const float* dL_dsigmas, const float* dL_drgbs, int64_t M, const float* x01,
                                 const void* density_weights_f16, const void* color_weights_f16, int32_t n_levels,
                                 int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, const void* h_f16,
                                 const void* rgb_f16, const void* save_in_d, const void* save_acts_d, const void* save_in_c,
                                 const void* save_acts_c, float loss_scale, float* grad_density_params, float* grad_color_params,
                                 int64_t n_density_mlp_params, void* scratch, nrc_stream_t stream);
/* Same with UNINITIALISED gradient buffers of n_density_params / n_color_params values: the call SETS them (no accumulation).  What it
 * saves: the caller's 49 MB fill of the table gradient, and the read half of the read-modify-write of the hashed levels' slices -- their
 * owners write every entry, only the small levels and the MLP parts are zeroed first (one launch). */
int nrc_ngp_train_query_backward_set(const float* dL_dsigmas, const float* dL_drgbs, int64_t M, const float* x01,
                                     const void* density_weights_f16, const void* color_weights_f16, int32_t n_levels,
                                     int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, const void* h_f16,
                                     const void* rgb_f16, const void* save_in_d, const void* save_acts_d, const void* save_in_c,
                                     const void* save_acts_c, float loss_scale, float* grad_density_params, float* grad_color_params,
                                     int64_t n_density_mlp_params, int64_t n_density_params, int64_t n_color_params, void* scratch,
                                     nrc_stream_t stream);
/* InstantNGPRayRenderingComponent.query_model (Renderer.py:48-53) as an encode + MLP kernel pair over Infinity-Cache sized
 * chunks (workspace: nrc_ngp_query_ws_bytes(M) bytes): xyz01 (M,3) f32 in [0,1], dirs (M,3) f32 unit
 * vectors -> sigmas (M) f32 = exp(fp16 feature 0), rgbs (M,3) f32 = fp16 sigmoid outputs. */
int64_t nrc_ngp_query_ws_bytes(int64_t M);
int nrc_ngp_query_fused(const float* xyz01, const float* dirs, int64_t M, const void* density_weights_f16,
                        const void* color_weights_f16, const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size,
                        int32_t base_resolution, float per_level_scale, float* sigmas, float* rgbs, void* workspace,
                        nrc_stream_t stream);

/* =====================================================================================================
 * Group 4 -- diff_gaussian_rasterization  (replaces the external CUDA rasterizer pinned at
 *            src/Thirdparty/DiffGaussianRasterization.py:9 behind src/Methods/GaussianSplatting/Renderer.py:60-81,94-153,163-183)
 * P Gaussians, SH degree D (0..3), M = SH coefficients per Gaussian in `shs` (P,M,3); exactly one of shs | colors_precomp (P,3)
 * and exactly one of (scales (P,3), rotations (P,4)) | cov3D_precomp (P,6).  viewmatrix / projmatrix (16 floats each, the
 * (4,4) tensors the reference passes: w2c.T and w2c.T @ P.T), campos (3), bg (3) are HOST pointers.  16x16-pixel tiles.
 * Per-Gaussian state (geometry buffer): radii (P) i32, depths (P), points_xy (P,2), conic_opacity (P,4), rgb (P,3),
 * clamped (P) u8 bit mask (bit c = channel c clamped), cov3D (P,6), tiles_touched (P) u32.
 * Model-side parameters (extension beyond the reference's call, for callers that own the Gaussians: src/Methods/GaussianSplatting/Model.py:45-87):
 * shs_rest != NULL: `shs` is the DC part (P,1,3) and shs_rest the (P,M-1,3) remainder as the model stores them -- the (P,M,3) concatenation
 * of get_features is never built; raw_parameters != 0: opacities are logits, scales log-scales, rotations unnormalised, and sigmoid / exp /
 * normalisation run inside preprocess (the backward returns gradients w.r.t. the raw values; dL_dsh_rest receives the remainder's gradient).
 * splat_records (P,16) f32: one 64-byte line per Gaussian with everything the blend kernels read of it (screen position, conic, opacity,
 * colour) and the per-Gaussian part of their block-culling test; written by nrc_gs_preprocess, read by nrc_gs_bin_render / nrc_gs_backward.
 * (tile_fill doubles as `tile_order`: the tiles sorted by list length, longest first = launch order of the blend kernels.  ABI 3: with a binning
 * workspace it is written by nrc_gs_preprocess already -- the last workgroup of the tile scan orders the tiles --, otherwise by nrc_gs_bin_render;
 * either way it is valid after nrc_gs_bin_render and must reach nrc_gs_backward unchanged.)
 * Binning state: tile_counts, tile_fill (n_tiles) u32, ranges (n_tiles,2) u32, keys (num_rendered) u64, point_list
 * (num_rendered) i32.  Image state: n_contrib (H*W) u32, final_T (H*W).
 *   nrc_gs_preprocess : stages 1-2; num_rendered (DEVICE i64[2]): [0] = number of (tile, Gaussian) instances -- the caller reads it
 *                       to size keys / point_list (the reference's rasterizer pays the same device->host read); [1] = number of
 *                       (tile row, Gaussian) span records the binning needed: if it exceeds the span capacity the workspace was
 *                       sized for, [0] is not valid and the call is repeated with a workspace for at least [1] spans.
 *                       instance_capacity > 0 (fixed-capacity mode, for graph capture): point_list has that many entries and nothing
 *                       needs to be read back -- tile ranges are cut at the capacity, the instances that would land behind it are
 *                       dropped (the farthest of the last tiles), and [0] > instance_capacity / [1] > span capacity report it.
 *                       count_mailbox (ABI 4, optional, binning-workspace path only): HOST memory from nrc_host_mailbox_alloc.  The kernel
 *                       that finishes the counts also stores {[0], [1], mailbox_ticket} into mailbox[0..2], the ticket last: a host that wants the
 *                       counts as soon as they exist polls mailbox[2] for the ticket it passed (a value it has not used on this mailbox
 *                       before) instead of placing an event / copy / stream wait behind the call -- which on this runtime costs ~6 us of idle
 *                       GPU between this call's kernels and the next, and arrives ~15 us later.  One frame in flight per mailbox.
 *   camera_dev        : optional DEVICE float[38] = viewmatrix (16), projmatrix (16), campos (3), bg (3).  When given, the kernels read the
 *                       pose from it and the host arrays (viewmatrix, projmatrix, campos, bg) may be NULL: a camera that lives in device
 *                       tensors (GaussianRasterizationSettings) never crosses to the host, and a recorded graph follows its updates.
 *   nrc_gs_bin_render : stages 3-5 -> out_color (3,H,W) = C + T * bg, n_contrib, final_T.
 *   nrc_gs_backward   : dL_dpix (3,H,W) -> every gradient (all fully written; dL_dmean2D (P,3) is the screen-space gradient
 *                       consumed by densification, src/Methods/GaussianSplatting/Model.py:258).  grad_records: WORKSPACE (P,16) f32, 64-byte
 *                       aligned: the blend backward accumulates its nine per-Gaussian sums in one 64-byte record per
 *                       Gaussian (colour 3, opacity 1, mean2D 2, conic 3) so that a tile's flush for a Gaussian is one contiguous group of one
 *                       atomic instruction; dL_dmean2D / dL_dopacity (and dL_dconic (P,4) / dL_dcolor (P,3), which may be NULL) are written
 *                       from the records by the per-Gaussian backward, WHICH LEAVES EVERY RECORD IT READ CLEARED (ABI 3).  records_clear = 0:
 *                       the call clears the workspace first (any contents); records_clear != 0: the caller guarantees that all P x 16 floats
 *                       are zero, or as nrc_gs_backward_features_band (group 21) left them -- e.g. the same buffer after a previous nrc_gs_backward of
 *                       the same P -- and the clearing launch is skipped.
 * ===================================================================================================== */
/* bytes of the binning workspace `bin_hist` (depth pre-sort buffers, row-span records, cursors) for `span_capacity` span records
 * (0 = default 4 P + 65536); returns 0 when the image has more than 256 tile rows or columns: pass NULL, the per-tile key sort is used.
 * The same span_capacity goes to nrc_gs_preprocess and nrc_gs_bin_render. */
int64_t nrc_gs_bin_hist_bytes(int32_t P, int32_t W, int32_t H, int64_t span_capacity);
int nrc_gs_preprocess(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* means3D, const float* shs,
                      const float* shs_rest, int32_t raw_parameters, const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                      const float* campos, const float* camera_dev, float tan_fovx, float tan_fovy, int32_t* radii, float* depths,
                      float* points_xy, float* conic_opacity, float* rgb, uint8_t* clamped, float* cov3D, uint32_t* tiles_touched,
                      uint32_t* tile_counts, uint32_t* ranges, uint32_t* tile_fill, uint32_t* bin_hist, int64_t span_capacity,
                      int64_t instance_capacity, float* splat_records, int64_t* num_rendered, int64_t* count_mailbox, int64_t mailbox_ticket,
                      nrc_stream_t stream);
/* 64 bytes of pinned, device-mapped, coherent host memory (zeroed) that kernels of this library may write and the host may poll: one address on
 * both sides; NRC_ERR_UNSUPPORTED when the runtime maps it elsewhere (use the device counters then).  Free with nrc_host_mailbox_free. */
int nrc_host_mailbox_alloc(int64_t** mailbox);
int nrc_host_mailbox_free(int64_t* mailbox);
/* camera_dev of a frame from a DEVICE pose: c2w_dev = the first 12 floats of a row-major camera-to-world (3,4) / (4,4), proj_t_dev = P^T (16) of
 * Cameras/Perspective.py's projection, bg3_dev (optional): out[0..16) = viewmatrix = w2c^T, [16..32) = viewmatrix @ P^T, [32..35) = camera position,
 * [35..38) = background (GaussianSplatting/Renderer.py:60-74 in one launch; the pose never visits the host). */
int nrc_gs_camera_block(const float* c2w_dev, const float* proj_t_dev, const float* bg3_dev, float* camera_dev_out, nrc_stream_t stream);
int nrc_gs_bin_render(int32_t P, int32_t W, int32_t H, const float* bg, const float* camera_dev, const int32_t* radii,
                      const float* depths, const float* points_xy, const float* conic_opacity, const float* rgb,
                      const uint32_t* ranges, uint32_t* tile_fill, const uint32_t* bin_hist, int64_t span_capacity,
                      int64_t instance_capacity, uint64_t* keys, int32_t* point_list, const float* splat_records, float* out_color,
                      uint32_t* n_contrib, float* final_T, nrc_stream_t stream);
int nrc_gs_backward(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg, const float* means3D, const float* shs,
                    const float* shs_rest, int32_t raw_parameters, const float* opacities, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list,
                    const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib,
                    const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest, float* dL_dscale, float* dL_drot, float* grad_records,
                    int32_t records_clear, nrc_stream_t stream);
/* nrc_gs_backward + the optimizer step of the `rest` SH tensor in one pass (round 6): 45 of a Gaussian's 59 parameters are SH coefficients above the dc term, and
 * their gradient rows sit in LDS at the end of the preprocessing backward -- Adam (apex FusedAdam, src/Methods/GaussianSplatting/Model.py:121-138, group 'f_rest':
 * no weight decay, eps as given) is applied THERE: dL/d shs_rest is never written and read back (180 B per Gaussian each way), the parameters are not read a second time.
 * shs_rest_param: the (P, M-1, 3) tensor the forward read, updated in place; rest_exp_avg / rest_exp_avg_sq its moments; bias corrections as host values.  Device camera
 * block only.  Same per-element arithmetic as nrc_adam_step.  The caller's optimizer must skip that tensor in this step (its .grad stays empty). */
int nrc_gs_backward_rest_step(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg_host, const float* means3D, const float* shs,
                    float* shs_rest_param, int32_t raw_parameters, const float* opacities, const float* scales, float scale_modifier, const float* rotations,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list, const uint32_t* ranges,
                    const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib, const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dopacity, float* dL_dmean3D, float* dL_dcov3D, float* dL_dsh, float* dL_dscale,
                    float* dL_drot, float* grad_records, int32_t records_clear, float* rest_exp_avg, float* rest_exp_avg_sq, float lr, float beta1, float beta2,
                    float eps, float bias_correction1, float bias_correction2, nrc_stream_t stream);
/* Bands (ABI 7): ONE frame rendered and differentiated as contiguous ranges of 16-pixel tile rows, [tile_row_begin, tile_row_begin + n_tile_rows) of the
 * gy = ceil(H / 16) rows -- the unit a single view is sharded by across GPUs (nerficg_amd.parallel.tile_row_band).  The four entry points below are
 * nrc_gs_bin_hist_bytes / nrc_gs_preprocess / nrc_gs_bin_render / nrc_gs_backward with a band; the entry points above are the band (0, gy).  A band is checked
 * before anything else (no HIP call in front of it): tile_row_begin < 0, n_tile_rows < 1 or tile_row_begin + n_tile_rows > gy return NRC_ERR_INVALID.
 *   nrc_gs_preprocess_band : projects ALL P Gaussians -- radii, depths, points_xy, conic_opacity, rgb, clamped, cov3D, tiles_touched and splat_records are those
 *                       of the whole-frame call bit for bit, and so is the depth order.  Binning is CLIPPED: a Gaussian's tile rectangle is intersected with the
 *                       band where the rectangles are made, a Gaussian that misses the band takes part in nothing behind the depth sort, tiles outside the
 *                       band get empty `ranges`, num_rendered[0] / [1] count the band's instances / spans only (point_list and span_capacity may be sized for
 *                       the band; the bytes of the workspace depend on span_capacity alone), instance_capacity and the count mailbox work as on a frame.  The
 *                       list of a band tile equals that tile's list of the whole-frame call.  tile_fill receives the launch order of the BAND's gx *
 *                       n_tile_rows tiles in its first entries.  band_mask (P) u8, optional: 1 where the clipped rectangle is non-empty, i.e. the Gaussians
 *                       that can receive a gradient from this band (written on the binning-workspace path only).
 *   nrc_gs_bin_render_band : blends the band's tiles only (gx * n_tile_rows workgroups).  out_color, n_contrib, final_T stay FULL-FRAME buffers of which only the
 *                       pixel rows [16 begin, min(H, 16 (begin + n))) are written -- bit for bit the whole-frame call's values --, the rest is untouched.
 *   nrc_gs_backward_band : dL_dpix is full-frame, only the band's rows are read; the blend backward runs over the band's tiles, the per-Gaussian backward over
 *                       all P on records that hold the band's contributions.  It is linear in the records: every gradient tensor is this band's SHARE of the
 *                       whole-frame gradient (the shares of a partition sum to it), exactly zero for a Gaussian whose rectangle misses the band.  There is no
 *                       band form of nrc_gs_backward_rest_step: an Adam step inside the backward pass would be taken on a partial gradient.
 * The per-tile key sort fallback (more than 256 tile rows or columns, or bin_hist == NULL) bins whole frames only: with P > 0 a band other than (0, gy)
 * returns NRC_ERR_UNSUPPORTED there. */
int64_t nrc_gs_bin_hist_bytes_band(int32_t P, int32_t W, int32_t H, int64_t span_capacity, int32_t tile_row_begin, int32_t n_tile_rows);
int nrc_gs_preprocess_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* means3D, const float* shs,
                      const float* shs_rest, int32_t raw_parameters, const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                      const float* campos, const float* camera_dev, float tan_fovx, float tan_fovy, int32_t* radii, float* depths,
                      float* points_xy, float* conic_opacity, float* rgb, uint8_t* clamped, float* cov3D, uint32_t* tiles_touched,
                      uint32_t* tile_counts, uint32_t* ranges, uint32_t* tile_fill, uint32_t* bin_hist, int64_t span_capacity,
                      int64_t instance_capacity, float* splat_records, int64_t* num_rendered, int64_t* count_mailbox, int64_t mailbox_ticket,
                      int32_t tile_row_begin, int32_t n_tile_rows, uint8_t* band_mask, nrc_stream_t stream);
int nrc_gs_bin_render_band(int32_t P, int32_t W, int32_t H, const float* bg, const float* camera_dev, const int32_t* radii,
                      const float* depths, const float* points_xy, const float* conic_opacity, const float* rgb,
                      const uint32_t* ranges, uint32_t* tile_fill, const uint32_t* bin_hist, int64_t span_capacity,
                      int64_t instance_capacity, uint64_t* keys, int32_t* point_list, const float* splat_records, float* out_color,
                      uint32_t* n_contrib, float* final_T, int32_t tile_row_begin, int32_t n_tile_rows, nrc_stream_t stream);
int nrc_gs_backward_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg, const float* means3D, const float* shs,
                    const float* shs_rest, int32_t raw_parameters, const float* opacities, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list,
                    const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib,
                    const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest, float* dL_dscale, float* dL_drot, float* grad_records,
                    int32_t records_clear, int32_t tile_row_begin, int32_t n_tile_rows, nrc_stream_t stream);
/* Depth and alpha maps (ABI 8): two further blended channels with background 0, accumulated with the colour's own weights w_i = alpha_i T_i --
 *   depth = sum_i w_i z_i  (z_i = the view-space depth of `depths`, the value the sort orders by; NOT normalised by alpha),   alpha = sum_i w_i = 1 - final_T.
 * Both are differentiable: the alpha channel behaves like a colour that is 1 for every Gaussian, the depth channel like a colour z_i whose own gradient
 * dL/dz_i = sum_pixels w_i g_d (slot [9] of the 64-byte gradient record) reaches dL_dmean3D through the third column of the view matrix.
 *   nrc_gs_bin_render_aux_band : nrc_gs_bin_render_band + out_depth_alpha (2, H, W) f32, FULL-FRAME like out_color: plane 0 = depth, plane 1 = alpha; only the band's
 *                       pixel rows are written.  out_color, n_contrib and final_T are those of nrc_gs_bin_render_band bit for bit.  NULL: the colour-only kernel,
 *                       i.e. nrc_gs_bin_render_band itself.  z travels in float [3].w of the splat record (written by nrc_gs_preprocess since ABI 8).
 *   nrc_gs_backward_aux_band : nrc_gs_backward_band + dL_ddepth_alpha (2, H, W) f32, full-frame, only the band's rows are read: every gradient tensor is the gradient
 *                       (the band's share) of  <dL_dpix, colour> + <dL_ddepth_alpha[0], depth> + <dL_ddepth_alpha[1], alpha>.  NULL: nrc_gs_backward_band itself.
 *                       The records are left cleared as by every backward (records_clear covers slot [9]: whole records are cleared).
 * Whole frames: the band (0, ceil(H / 16)); the per-tile key sort fallback supports both on whole frames.  There is no aux form of nrc_gs_backward_rest_step. */
int nrc_gs_bin_render_aux_band(int32_t P, int32_t W, int32_t H, const float* bg, const float* camera_dev, const int32_t* radii,
                      const float* depths, const float* points_xy, const float* conic_opacity, const float* rgb,
                      const uint32_t* ranges, uint32_t* tile_fill, const uint32_t* bin_hist, int64_t span_capacity,
                      int64_t instance_capacity, uint64_t* keys, int32_t* point_list, const float* splat_records, float* out_color,
                      uint32_t* n_contrib, float* final_T, int32_t tile_row_begin, int32_t n_tile_rows, float* out_depth_alpha, nrc_stream_t stream);
int nrc_gs_backward_aux_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg, const float* means3D, const float* shs,
                    const float* shs_rest, int32_t raw_parameters, const float* opacities, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list,
                    const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib,
                    const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest, float* dL_dscale, float* dL_drot, float* grad_records,
                    int32_t records_clear, int32_t tile_row_begin, int32_t n_tile_rows, const float* dL_ddepth_alpha, nrc_stream_t stream);
/* Gradients to the camera (ABI 14).  dL_dcamera: DEVICE float[35] in the layout of camera_dev without the background -- dL/dviewmatrix (16), dL/dprojmatrix (16),
 * dL/dcampos (3) -- always fully written; viewmatrix[.][3] and projmatrix[.][2] (the column of the clip-space z, which the rasterizer does not use) receive exact
 * zeros.  It is the gradient of the same scalar as the other outputs (the band's share for a band: the shares of a partition sum to the frame's), a reduction over
 * all Gaussians of quantities the per-Gaussian backward forms anyway, computed by two extra launches between the blend backward and the per-Gaussian backward; the
 * other outputs and the cleared records are bit for bit those of nrc_gs_backward_aux_band.  Deterministic: no float atomics, fixed summation order.
 *   nrc_gs_pose_partials_floats : floats of the WORKSPACE pose_partials for P Gaussians (one 32-float slab per workgroup of the reduction; 16-byte aligned).
 *   nrc_gs_backward_pose_band   : nrc_gs_backward_aux_band (dL_ddepth_alpha may be NULL) + pose_partials + dL_dcamera.  dL_dcamera == NULL: nrc_gs_backward_aux_band
 *                       itself.  P == 0: 35 zeros.  The pose may come from the host arrays or from camera_dev.  NRC_ERR_INVALID before any HIP call for a bad band,
 *                       for dL_dcamera without pose_partials and for a misaligned workspace.  There is no camera gradient in nrc_gs_backward_rest_step.
 *   nrc_gs_camera_block_backward : the transpose of nrc_gs_camera_block -- dL_dcamera (35) -> dL_dc2w_out (12 floats = the (3, 4) rows of the pose), with the c2w_dev
 *                       and proj_t_dev the block was made from. */
int64_t nrc_gs_pose_partials_floats(int32_t P);
int nrc_gs_backward_pose_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg, const float* means3D, const float* shs,
                    const float* shs_rest, int32_t raw_parameters, const float* opacities, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list,
                    const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib,
                    const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest, float* dL_dscale, float* dL_drot, float* grad_records,
                    int32_t records_clear, int32_t tile_row_begin, int32_t n_tile_rows, const float* dL_ddepth_alpha, float* pose_partials,
                    float* dL_dcamera, nrc_stream_t stream);
int nrc_gs_camera_block_backward(const float* c2w_dev, const float* proj_t_dev, const float* dL_dcamera, float* dL_dc2w_out, nrc_stream_t stream);

/* =====================================================================================================
 * Group 5 -- ray generation (replaces PerspectiveCamera.compute_local_ray_directions src/Cameras/Perspective.py:64-94
 * + View.get_rays / cam_to_world src/Datasets/utils.py:1033-1074 for undistorted perspective cameras).
 * intrinsics (HOST, 4 doubles): focal_x, focal_y, center_x, center_y.  c2w (HOST, 16 doubles, row-major 4x4).
 * Outputs (H*W,3) f32 each, y-major then x; any output pointer may be NULL.
 * ===================================================================================================== */
int nrc_generate_rays(int32_t width, int32_t height, const double* intrinsics, const double* c2w, float* origin,
                      float* direction, float* view_direction, nrc_stream_t stream);

/* =====================================================================================================
 * Group 6 -- fused InstantNGP image pipeline (MI355X-native restructuring of InstantNGPRenderer.render_image ->
 *            render_rays_inference, src/Methods/InstantNGP/Renderer.py:30-46,86-138,172-180): no ray tensors, no
 *            per-iteration host syncs, 4-byte sample records, 8-byte sample values, TILE-INTERLEAVED sample layout:
 *            a tile = 8x8 pixels (lane = (y&7)*8 + (x&7)); sample k of lane l of local tile T is slot
 *            (tile_off[T] + k) * 64 + l.  A shard is a range of tiles [tile_begin, tile_begin + n_tiles) of the
 *            ceil(W/8) x ceil(H/8) tile grid (row-major); per-ray arrays have n_tiles*64 entries.
 *   1. nrc_ngp_render_count : pixel -> ray (Group 5 semantics) -> centre shift, box slab test, near/far clamp -> DDA sample
 *                             count; writes ray_od (n_tiles,6,64) = per-tile SoA of (o - centre, d), ray_t (n,2), ray_cnt (n), tile_rows (2*n_tiles: rows per tile,
 *                             then samples per tile), tile_off (n_tiles+1), counter = (total rows, total samples).  intr/c2w/center3/half3: HOST pointers.
 *   2. nrc_ngp_render_write : ts (rows*64) f32 (-1 = hole), row_tile (rows) i32.
 *   3. nrc_ngp_query_samples: slots -> packed (h0, r, g, b) fp16 (sigma = exp(h0)); xyz_min3/xyz_size3 HOST pointers;
 *                             n_ray_tiles = tiles in ray_od (their SH coefficients are evaluated once per ray);
 *                             workspace: nrc_ngp_query_samples_ws_bytes(rows, n_ray_tiles) bytes.
 *      ABI 3, fixed row capacity (a frame without the host read of `counter`, e.g. inside a stream capture): the caller sizes ts / row_tile /
 *      packed / workspace for `row_capacity` rows, passes it to nrc_ngp_render_write (rows that would land behind it are not written; 0 = no
 *      bound) and as n_rows to nrc_ngp_query_samples together with n_rows_dev = counter (DEVICE, the count pass's total): the kernels then
 *      process only the rows that exist.  counter[0] > row_capacity afterwards means the frame overflowed and must be rendered again.
 *   4. nrc_ngp_composite_image: serial per-ray compositing + background / clamps (bg3 HOST) into full-image buffers
 *                             rgb (H*W,3), alpha (H*W), depth (H*W) -- only the shard's pixels are written.
 * ===================================================================================================== */
/* pixel footprint of a tile (tile width x height = 64; the tile grid is ceil(W / tw) x ceil(H / th), row-major) */
int nrc_ngp_tile_width(void);
int nrc_ngp_tile_height(void);
int nrc_ngp_render_count(int32_t width, int32_t height, const double* intrinsics, const double* c2w, const float* center3,
                         const float* half3, float near_plane, float far_plane, int64_t tile_begin, int64_t n_tiles,
                         const uint8_t* density_bitfield, int32_t cascades, float scale, float exp_step_factor,
                         int32_t grid_size, int32_t max_samples, float* ray_od, float* ray_t, int32_t* ray_cnt,
                         int32_t* tile_rows, int32_t* tile_off, int32_t* counter, float* ts_provisional, int64_t* count_mailbox,
                         int64_t mailbox_ticket, nrc_stream_t stream);
/* count_mailbox (ABI 4, optional, NULL allowed): HOST memory from nrc_host_mailbox_alloc (group 4).  The scan that closes the count pass stores
 * {counter[0], counter[1], mailbox_ticket} into mailbox[0..2], the ticket last; the host polls mailbox[2] for its ticket instead of copying
 * `counter` back (no device-to-host copy and no stream wait between the count pass and nrc_ngp_render_write: 42 -> ~10 us of idle GPU per frame). */
/* ts_provisional (optional, NULL allowed; nrc_ngp_render_provisional_bytes(n_tiles, max_samples) bytes = max_samples rows of 256 B per
 * tile): the count pass parks every sample's t there and steps 2 copy them into their final rows instead of marching the rays a
 * second time (pass the same buffer to both calls).  HBM is plentiful on this part: 2.6 GB for an 800x800 image. */
int64_t nrc_ngp_render_provisional_bytes(int64_t n_tiles, int32_t max_samples);
/* ABI 12, the count pass for a caller's own rays: nrc_ngp_render_count with the ray of pixel p read from row p of origin / view_direction (DEVICE,
 * (n_rays,3) f32 each) instead of derived from a camera.  The origin is shifted by center3, the direction is used AS GIVEN (not normalised: the reference
 * hands rays.view_direction through untouched, Renderer.py:40), box test / near-far clamp / march and every output are those of nrc_ngp_render_count, so
 * steps 2-4 (and the layer / frame variants) follow unchanged -- they read rays from ray_od only.  A lane whose pixel has no row (p >= n_rays) is an
 * out-of-image pixel: no samples, background.  Refused (NRC_ERR_INVALID): n_rays < 0, n_rays > width * height, a NULL ray array with n_rays > 0, and
 * whatever nrc_ngp_render_count refuses.  Two ways to use it:
 *   a ray list            width = nrc_ngp_tile_width(), height = nrc_ngp_tile_height() * ceil(N / 64): the virtual image is one tile wide, so pixel index
 *                         = ray index and tile T holds rays 64 T .. 64 T + 63; every later stage is called with this width / height and with output
 *                         buffers of 64 * n_tiles entries (the first N are the rays').
 *   a row-major image of  (what View.get_rays() returns) the real width, height and n_rays = width * height: tiles are the 8x8 pixel blocks of the camera
 *   rays                  path, so the encoder sees the same spatial coherence -- any camera model, its ray generator stays the caller's. */
int nrc_ngp_render_count_rays(int32_t width, int32_t height, int64_t n_rays, const float* origin, const float* view_direction, const float* center3,
                              const float* half3, float near_plane, float far_plane, int64_t tile_begin, int64_t n_tiles,
                              const uint8_t* density_bitfield, int32_t cascades, float scale, float exp_step_factor, int32_t grid_size,
                              int32_t max_samples, float* ray_od, float* ray_t, int32_t* ray_cnt, int32_t* tile_rows, int32_t* tile_off,
                              int32_t* counter, float* ts_provisional, int64_t* count_mailbox, int64_t mailbox_ticket, nrc_stream_t stream);
int nrc_ngp_render_write(int64_t n_tiles, const uint8_t* density_bitfield, int32_t cascades, float scale,
                         float exp_step_factor, int32_t grid_size, int32_t max_samples, const float* ray_od,
                         const float* ray_t, const int32_t* ray_cnt, const int32_t* tile_off, float* ts, int32_t* row_tile,
                         const float* ts_provisional, int64_t row_capacity, nrc_stream_t stream);
int64_t nrc_ngp_query_samples_ws_bytes(int64_t n_rows, int64_t n_ray_tiles);
int nrc_ngp_query_samples(const float* ts, int32_t* row_tile, const float* ray_od, int64_t n_rows, int64_t n_ray_tiles,
                          const float* xyz_min3, const float* xyz_size3, const void* density_weights_f16, const void* color_weights_f16,
                          const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution,
                          float per_level_scale, void* packed_f16, void* workspace, const int32_t* n_rows_dev, const int32_t* arena_tile_off,
                          int32_t arena_rows, nrc_stream_t stream);
/* ABI 4, the arena queried in place (the default of the single-pass frame): with ts_provisional the count pass has every sample's t already in
 * 256-byte rows per tile -- sample k of local tile lt in arena row lt * max_samples + k, holes (-1) up to the tile's longest ray included -- and the
 * compact `ts` rows differ from it only by WHERE a row lives.  nrc_ngp_render_write is then not needed at all (the 2 x 320 MB copy of an 800x800
 * frame is skipped: 150 us): nrc_ngp_query_samples takes ts = ts_provisional, arena_tile_off = tile_off, arena_rows = max_samples, FILLS row_tile
 * (n_rows entries, from tile_off, in the launch that evaluates the rays' SH) and reads slot i of row r = i >> 6 at arena row
 * row_tile[r] * arena_rows + (r - tile_off[row_tile[r]]); nrc_ngp_composite_image takes the same pointer and arena_rows (0 = compact rows).
 * (nrc_ngp_render_write(ts = NULL) writes row_tile only, for callers of the single stages.)  `packed` stays indexed by compact rows.  Same values,
 * same pictures. */
/* Layer-major variant of steps 2-4: rows ordered by sample index k first (all tiles' k = 0, then k = 1, ...), so that consecutive
 * chunks of rows are depth slabs of the image; after every slab the finished tiles (all rays saturated below T_threshold or out of
 * samples) write their pixels and their remaining rows are skipped -- the early termination of the reference's alive-ray loop
 * (src/Methods/InstantNGP/Renderer.py:118-132) at slab granularity, without host round trips.  Same image as steps 2-4.
 *   nrc_ngp_render_write_layers: like step 2, plus layer_off (max_samples + 1) i32 and row_of (rows) i32 = the row of (tile, k).
 *   nrc_ngp_render_layers      : steps 3 + 4 interleaved per slab; workspace nrc_ngp_render_layers_ws_bytes(rows, n_tiles);
 *                                skipped_rows (optional, 1 i32): number of rows the early termination saved.
 *   ABI 4: row_tile is READ AND WRITTEN -- when a tile finishes, the slab compositor overwrites the entries of its remaining rows with -1 - tile,
 *   which is where the query kernels of the following slabs look first (no feature is computed, read or written for such a row).
 *   ABI 4, the arena queried in place (as for the single pass): nrc_ngp_render_write_layers(ts = NULL, ..., row_k) copies nothing and also writes
 *   row_k (rows) i32 = which sample of its tile a row is; nrc_ngp_render_layers takes ts = ts_provisional, arena_row_k = row_k, arena_rows =
 *   max_samples and reads slot i of row r at arena row row_tile[r] * arena_rows + row_k[r] (305 -> ~10 us for the write step of an 800x800 frame). */
int nrc_ngp_render_write_layers(int64_t n_tiles, const uint8_t* density_bitfield, int32_t cascades, float scale, float exp_step_factor,
                                int32_t grid_size, int32_t max_samples, const float* ray_od, const float* ray_t, const int32_t* ray_cnt,
                                const int32_t* tile_rows, const int32_t* tile_off, float* ts, int32_t* row_tile, int32_t* layer_off,
                                int32_t* row_of, const float* ts_provisional, int32_t* row_k, nrc_stream_t stream);
int64_t nrc_ngp_render_layers_ws_bytes(int64_t n_rows, int64_t n_ray_tiles);
int nrc_ngp_render_layers(const float* ts, int32_t* row_tile, const float* ray_od, int64_t n_rows, int64_t n_ray_tiles,
                          const float* xyz_min3, const float* xyz_size3, const void* density_weights_f16,
                          const void* color_weights_f16, const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size,
                          int32_t base_resolution, float per_level_scale, const int32_t* ray_cnt, const int32_t* tile_rows,
                          const int32_t* tile_off, const int32_t* row_of, int32_t width, int32_t height, int64_t tile_begin,
                          int32_t cascades, float exp_step_factor, int32_t grid_size, int32_t max_samples, float T_threshold,
                          const float* bg3_host, void* packed_f16, float* rgb, float* alpha, float* depth, int32_t* skipped_rows,
                          void* workspace, const int32_t* arena_row_k, int32_t arena_rows, nrc_stream_t stream);
/* stage 3a on its own (the dominant kernel of the pipeline; used by bench.py's roofline leg -- which sets no block view, see
 * nrc_ngp_set_encoder_block_view below: its figure is the kernel with every level read from the table, ~3 % above the kernel as the frame runs it):
 * hash-grid features of the n_rows (<= 131072) rows
 * first_row .. first_row + n_rows - 1 of the frame -- ts / row_tile are the FRAME's arrays, not offset ones (ABI 4) --, fragment-major: the 16-byte
 * vector [((j>>5)*4 + ((g + (j>>5))&3))*32 + (j&31)] = levels 4g..4g+3 (fp16x2) of slot j of the chunk.  arena_tile_off / arena_rows: as for
 * nrc_ngp_query_samples (NULL / 0: compact rows), so that the kernel is timed in the form the frame runs it */
/* The brick of the tiled layout that ONE WAVE of the encoder gathers for: 2^log2_x x 2^log2_y pixels of a ray tile x 2^(6 - log2_x - log2_y) consecutive
 * steps (default 8 x 2 x 4).  Hash-table entries are contiguous along world x only, so which brick shares the most cache lines depends on how the
 * image axes and the viewing direction lie to that axis: the host may pick a shape per pose (InstantNGPRenderer does, from the camera's axes).
 * Both < 0: back to the default.  A setting of the CALLING HOST THREAD, read when that thread launches the encoder (set it on the thread that
 * enqueues the frame); the features are identical for every shape. */
int nrc_ngp_set_encoder_shape(int32_t log2_x, int32_t log2_y);
/* k_grid_encode deals its workgroups to the 8 XCDs in runs: inside a run of 8 * `workgroups` workgroups every XCD takes `workgroups` consecutive ones, so
 * that the XCDs work inside the same part of the frame at the same time (what is left behind the last whole run is split in eight the same way).
 * 0: the library's default (a compile-time constant, the measured best).  A positive multiple of 4 (blocks of 1024 slots stay whole); anything else is
 * refused.  A setting of the CALLING HOST THREAD like the shape above; the features are identical for every value -- it exists so that tests reach run
 * boundaries with small frames, the renderer does not call it. */
int nrc_ngp_set_encoder_xcd_run(int32_t workgroups);
/* Cell-block view of the table's leading dense levels (at most 5, the levels in front of the first hashed one; 11.29 MB for the shipped grid): for
 * every cell (gx, gy, gz) in [0, res]^3 of such a level one 32-byte record with the fp16 pairs of its eight corners (corner k: x + (k & 1),
 * y + ((k >> 1) & 1), z + (k >> 2)), record gx + (res + 1) * (gy + (res + 1) * gz), the levels one behind the other.  The image encoder
 * (k_grid_encode of the four entry points below) reads a sample's corners at these levels as two 16-byte loads of one address instead of eight
 * gathers; the features are identical with and without the view for every sample inside the model box (normalised position in [0, 1]^3, cell
 * in [0, res]^3).  A position outside it gets meaningless features either way, and not the same ones: the view clamps the cell coordinates to res,
 * the table path wraps and clamps the linear index.
 *   nrc_ngp_block_view_bytes  : size of the view of a grid (0: no level qualifies; < 0: an error code)
 *   nrc_ngp_build_block_view  : fills `view` from table_f16 -- again whenever the table's VALUES change (one pass over the view)
 *   nrc_ngp_set_encoder_block_view : hands the view of the table that the NEXT call of nrc_ngp_render_frame / _render_layers / _query_samples /
 *       _encode_samples on the calling host thread is given.  That call takes it, whichever way it ends: a call without a view set in front of
 *       it (or with NULL) reads the table at every level, and so does a grid whose level 0 is hashed.  The library cannot check whose view it is
 *       given (no size, no identity): it must be the view of THAT call's table_f16, built since the table's values last changed.  A caller whose
 *       entry-point call may not happen after the view was set (an exception in between) sets NULL again itself -- InstantNGPRenderer does, behind
 *       every call -- or the next entry point on the thread, perhaps for another table, would take it.
 *   nrc_ngp_set_encoder_block_levels : how many of the view's levels the encoder reads through it (0 .. 5; the levels a view does not hold are
 *       read from the table whatever is asked for), -1: the library's default, the measured best.  A setting of the CALLING HOST THREAD like the
 *       shape above; it exists for tests and measurements, the renderer does not call it. */
int64_t nrc_ngp_block_view_bytes(int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale);
int nrc_ngp_build_block_view(const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                             void* view, nrc_stream_t stream);
int nrc_ngp_set_encoder_block_view(const void* view);
int nrc_ngp_set_encoder_block_levels(int32_t levels);
/* Vertex view of the hashed levels that follow the block view's levels (at most 4 consecutive hashed levels, as long as the view stays below 128 MB;
 * levels 5-8 of the shipped grid, res 81 112 154 213: 63.2 MB): level by level a dense array of the 4-byte fp16 pairs of its vertices, vertex (x, y, z)
 * in [0, R)^3 at dword x + R * (y + R * z), R = res + 2, holding the table entry the spatial hash names for that vertex.  The image encoder reads a
 * sample's corners at these levels as four 8-byte loads (the two x-neighbours of a (y, z) pair are adjacent) instead of four 16-byte loads, a
 * predicated round of four more and the hash; the features are identical with and without the view for every sample inside the model box.  A
 * position outside it gets meaningless features either way, and not the same ones: the view clamps the cell coordinates to res, the table path
 * hashes whatever cell it is given.  A buffer of its own: the block view, its size and its functions are what they were.
 *   nrc_ngp_vertex_view_bytes  : size of the view of a grid (0: no level qualifies, e.g. the first hashed level alone passes 128 MB; < 0: an error code)
 *   nrc_ngp_build_vertex_view  : fills `view` from table_f16 -- again whenever the table's VALUES change (one gather pass over the view)
 *   nrc_ngp_set_encoder_vertex_view : as nrc_ngp_set_encoder_block_view -- for the NEXT call of the four entry points on the calling host thread, taken
 *       by that call whichever way it ends, never checked, NULL or no call = the table path.
 *   nrc_ngp_set_encoder_vertex_levels : how many of the view's levels the encoder reads through it (0 .. 4), -1: the library's default, the measured
 *       best.  A setting of the CALLING HOST THREAD; it exists for tests and measurements, the renderer does not call it. */
int64_t nrc_ngp_vertex_view_bytes(int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale);
int nrc_ngp_build_vertex_view(const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                              void* view, nrc_stream_t stream);
int nrc_ngp_set_encoder_vertex_view(const void* view);
int nrc_ngp_set_encoder_vertex_levels(int32_t levels);
/* Group 25 -- y-pair view of the hashed levels that follow the block view's levels (at most 6 consecutive hashed levels, as long as the view stays below
 * 1 GiB, and no more than the library reads by default, 5; the shipped grid: level 5 4.6 MB, 6 11.9, 7 30.4, 8 79.5, 9 209.6 = 335.9 MB): level by level a
 * dense array of 8-byte records, record (x, y, z) in [0, R)^3 at index x + R * (y + R * z), R = res + 2, holding the table entries the spatial hash
 * names for vertex (x, y, z) and for vertex (x, y + 1, z); the records of the row y = res + 1 are never read and hold zeros.  One 16-byte load at the
 * record of a sample's cell returns the four corners of a z-plane, so the image encoder reads a level as two loads of one address instead of the vertex
 * view's four or the table's four, a predicated round of four more and the hash.  The features are identical with and without the view for every
 * sample inside the model box; a position outside it gets meaningless features either way, and not the same ones (the view clamps the cell
 * coordinates to res).  A buffer of its own: the block view and the vertex view, their sizes and their functions are what they were.  A level that a
 * call reads through the y-pair view is not read through the vertex view, so a caller whose y-pair view holds the vertex view's levels needs no
 * vertex view.
 *   nrc_ngp_ypair_view_bytes  : size of the view of a grid (0: no level qualifies; < 0: an error code)
 *   nrc_ngp_build_ypair_view  : fills `view` from table_f16 -- again whenever the table's VALUES change (one gather pass over the view)
 *   nrc_ngp_set_encoder_ypair_view : as nrc_ngp_set_encoder_block_view -- for the NEXT call of the four entry points on the calling host thread, taken
 *       by that call whichever way it ends, never checked, NULL or no call = the vertex view or the table.
 *   nrc_ngp_set_encoder_ypair_levels : how many of the view's levels the encoder reads through it (0 .. 6; the levels a view does not hold are read
 *       from the vertex view or the table whatever is asked for), -1: the library's default, the measured best.  A setting of the CALLING HOST
 *       THREAD; it exists for tests and measurements, the renderer does not call it. */
int64_t nrc_ngp_ypair_view_bytes(int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale);
int nrc_ngp_build_ypair_view(const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                             void* view, nrc_stream_t stream);
int nrc_ngp_set_encoder_ypair_view(const void* view);
int nrc_ngp_set_encoder_ypair_levels(int32_t levels);
int nrc_ngp_encode_samples(const float* ts, const int32_t* row_tile, const float* ray_od, int64_t first_row, int64_t n_rows, const float* xyz_min3,
                           const float* xyz_size3, const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size,
                           int32_t base_resolution, float per_level_scale, void* features_f16, const int32_t* arena_tile_off,
                           int32_t arena_rows, nrc_stream_t stream);
/* stage 3b on its own (the MFMA kernel; bench.py's second roofline object): features as written by nrc_ngp_encode_samples for the same
 * n_rows (<= 131072) rows -> packed (h0, r, g, b) fp16 of the FRAME (indexed by the frame's slots); ray_sh_workspace: n_ray_tiles * 2048 bytes,
 * filled by this call with the rays' SH coefficients; n_ray_tiles = 0: it holds them already (they belong to the image, a caller looping over
 * chunks fills it once).  Only the records of SAMPLES are written: the record of a hole (t < 0) and the records of a finished tile's rows
 * (row_tile = -1 - tile) keep what they held, as do the features of such rows in nrc_ngp_encode_samples (a hole's features are all zero) */
int nrc_ngp_mlp_samples(const float* ts, const int32_t* row_tile, const float* ray_od, int64_t first_row, int64_t n_rows, int64_t n_ray_tiles,
                        const void* features_f16, const void* density_weights_f16, const void* color_weights_f16,
                        void* packed_f16, void* ray_sh_workspace, const int32_t* arena_tile_off, int32_t arena_rows, nrc_stream_t stream);
int nrc_ngp_composite_image(const void* packed_f16, const float* ts, const int32_t* ray_cnt, const int32_t* tile_off,
                            int32_t width, int32_t height, int64_t tile_begin, int64_t n_tiles, int32_t cascades,
                            float exp_step_factor, int32_t grid_size, int32_t max_samples, float T_threshold,
                            const float* bg3, float* rgb, float* alpha, float* depth, int64_t row_capacity, int32_t arena_rows,
                            nrc_stream_t stream);
/* Steps 3 + 4 as ONE pass over the arena (the default single-pass frame): the MLP kernel composites the rows it evaluates, so no packed
 * outputs are written or read back.  Takes the count pass's arena in place exactly like nrc_ngp_query_samples(ts = ts_provisional,
 * arena_tile_off = tile_off, arena_rows = max_samples) and FILLS row_tile (n_rows entries) likewise; writes rgb / alpha / depth of the
 * shard's pixels like nrc_ngp_composite_image.  Same pictures as steps 3 + 4, bit for bit (the per-sample step is shared).
 * The frame runs in chunks of WHOLE ray tiles of at most row_budget rows (<= 0: the library default, 2 Mi rows = one chunk for an 800x800
 * frame; otherwise >= 2 * max_samples); inside a chunk the tiles are processed longest first.  workspace:
 * nrc_ngp_render_frame_ws_bytes(n_rows, n_ray_tiles, max_samples, row_budget) bytes.
 * Group 26 -- which kernel pair the frame runs, nrc_ngp_set_frame_density_encoder(mode):
 *   0: the 64-byte pair.  The encoder writes the 64 B of grid features of every slot (the records of nrc_ngp_encode_samples) and the MLP-composite
 *      kernel runs the density net, its head and the colour net on them.
 *   1: the density-encoder pair.  The encoder runs the density net on the samples it has just gathered for and writes the 16 fp16 density features,
 *      32 B per slot: for the 32-sample tile T of a chunk (slots 32 T .. 32 T + 31) a 1 KB record, the 16-byte vector 64 T + 32 hh + r holding
 *      features 8 hh .. 8 hh + 7 of slot 32 T + r; the MLP-composite kernel runs the colour net from there.  The records fill the first half of
 *      the workspace's feature part.  Chunks of more than 2^24 rows run the 64-byte pair whatever is set.
 *  -1: the library's default (a compile-time constant).
 * The pictures are the same bit for bit: the same MFMAs on the same operands, only in another kernel.  A setting of the CALLING HOST THREAD, read by
 * nrc_ngp_render_frame alone: nrc_ngp_render_frame_ws_bytes does not depend on it (64 B per slot), so a workspace serves either pair
 * (InstantNGPRenderer sets the mode from FRAME_DENSITY_ENCODER in front of every frame).  No other entry point reads it: nrc_ngp_encode_samples /
 * nrc_ngp_mlp_samples, the layered and the fixed-capacity frames and all training paths keep the 64-byte features.
 * Group 29 -- the density net's fragment image.  The workspace ends with 6 144 bytes (rounded up to 256) that EVERY call of nrc_ngp_render_frame
 * rewrites from density_weights_f16 (one extra workgroup of its first launch; nothing is cached from call to call, so weights that changed between
 * two frames are followed) and that the density-encoder pair's encoder copies into LDS instead of building the fragments from the row-major weights
 * in each of its workgroups.  Image slot f = 0 .. 5, lane l = 0 .. 63, 16-byte vector f * 64 + l, with W = density_weights_f16 (row-major: 64 x 32
 * first layer, then the 16 x 64 head):
 *   f < 4:   elements e = 0 .. 7 = W[(32 (f >> 1) + (l & 31)) * 32 + 16 (f & 1) + 8 (l >> 5) + e]
 *   f = 4, 5: with m = l & 15, kg = l >> 4, ks = f - 4:  element e = W[2048 + 64 m + 32 ks + (e & 3) + 8 (2 (kg & 1) + (e >> 2)) + 4 (kg >> 1)]
 * -- every one of the 3 072 weights exactly once.  nrc_ngp_density_frag_image runs the same builder on its own: image_out receives the 6 144 bytes.
 * Group 30 -- the full-encoder form, nrc_ngp_set_frame_full_encoder(mode): 1 = on, 0 = off, -1 = the library's default (a compile-time constant, 1).  A
 * setting of the CALLING HOST THREAD, read by nrc_ngp_render_frame alone, and only where the density-encoder pair would run (mode 1 of group 26 and a
 * chunk of at most 2^24 rows): with group 26 at 0 the frame is the 64-byte pair whatever is set here, with group 26 at 1 and this switch at 0 it is the
 * 32-byte pair.  Where it is on and n_rows <= 8 x (rows of the largest chunk) and n_rows < 2^25, the encoder runs the density net AND the colour net on
 * the samples it gathered for and stores the 8-byte record (h0, r, g, b) in fp16 of nrc_ngp_mlp_samples at the slot's ABSOLUTE place, record s of the
 * workspace's feature part = slot s of the frame (a hole's record and the records behind n_rows * 64 are not written); ONE launch of the kernel of
 * nrc_ngp_composite_image (arena_rows = max_samples) then composites every ray tile.  No MLP-composite kernel and no chunk table run in this form; larger
 * frames keep the 32-byte pair.  Same pictures, bit for bit; the workspace size does not depend on the setting.
 * The colour net's fragment image: 14 336 bytes directly in FRONT of the density image, rewritten by every call of nrc_ngp_render_frame (the same extra
 * workgroup) from color_weights_f16 = W (row-major: 64 x 32 first layer, 64 x 64 second layer, 16 x 64 head).  Image slot f = 0 .. 13, lane l:
 *   f < 4 (first layer, m-tile f >> 1, k-step f & 1):  element e = W[(32 (f >> 1) + (l & 31)) * 32 + 16 (f & 1) + 8 (l >> 5) + e]
 *   4 <= f < 12 (second layer, g = f - 4, m-tile g >> 2, k-step g & 3, accumulator order):
 *            element e = W[2048 + (32 (g >> 2) + (l & 31)) * 64 + 16 (g & 3) + 8 (e >> 2) + 4 (l >> 5) + (e & 3)]
 *   f = 12, 13 (head, ks = f - 12, m = l & 15, kg = l >> 4):  element e = W[6144 + 64 m + 32 ks + (e & 3) + 8 (2 (kg & 1) + (e >> 2)) + 4 (kg >> 1)]
 * -- every one of the 7 168 weights exactly once.  nrc_ngp_colour_frag_image runs the same builder on its own: image_out receives the 14 336 bytes. */
int nrc_ngp_set_frame_density_encoder(int32_t mode);
int nrc_ngp_set_frame_full_encoder(int32_t mode);
int nrc_ngp_colour_frag_image(const void* color_weights_f16, void* image_out, nrc_stream_t stream);
int64_t nrc_ngp_render_frame_ws_bytes(int64_t n_rows, int64_t n_ray_tiles, int32_t max_samples, int64_t row_budget);
int nrc_ngp_density_frag_image(const void* density_weights_f16, void* image_out, nrc_stream_t stream);
int nrc_ngp_render_frame(const float* ts_arena, int32_t* row_tile, const float* ray_od, int64_t n_rows, int64_t n_ray_tiles,
                         const float* xyz_min3, const float* xyz_size3, const void* density_weights_f16, const void* color_weights_f16,
                         const void* table_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                         const int32_t* ray_cnt, const int32_t* tile_off, int32_t width, int32_t height, int64_t tile_begin, int32_t cascades,
                         float exp_step_factor, int32_t grid_size, int32_t max_samples, float T_threshold, const float* bg3_host, float* rgb,
                         float* alpha, float* depth, int64_t row_budget, void* workspace, nrc_stream_t stream);

/* =====================================================================================================
 * Group 7 -- SSIM map and its gradient (3DGS loss): replaces fused_ssim as imported at
 *            src/Thirdparty/FusedSSIM.py:15 and called at src/Optim/Losses/DSSIM.py:11-18.  Images are (planes, H, W) f32 with
 *            planes = batch * channels; 11x11 Gaussian window (sigma 1.5), zero "same" padding.  The three derivative maps
 *            (d ssim / d mu1, d sigma1^2, d sigma12) are written when all three pointers are non-null (training).
 * ===================================================================================================== */
int nrc_ssim_forward(const float* img1, const float* img2, int64_t planes, int32_t H, int32_t W, float C1, float C2, float* ssim_map,
                     float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12, nrc_stream_t stream);
int nrc_ssim_backward(const float* img1, const float* img2, int64_t planes, int32_t H, int32_t W, const float* dL_dmap,
                      const float* dm_dmu1, const float* dm_dsigma1_sq, const float* dm_dsigma12, float* dL_dimg1,
                      nrc_stream_t stream);
/* The whole photometric loss of the 3DGS trainer (src/Methods/GaussianSplatting/Loss.py:11-23: lambda_l1 * L1 + lambda_dssim * (1 - SSIM), weights
 * Trainer.py:34-35) in three launches instead of the ~22 that the L1 term, the two means and the weighting take as tensor operations around
 * nrc_ssim_forward / _backward (each of them >= 5 us on a scalar): the SSIM stencil also sums |image - target| and the SSIM values per workgroup,
 * one workgroup adds the partial sums up in a fixed order (double accumulators), and the backward stencil takes dL/dmap = -lambda_dssim * g / n as a
 * constant and adds lambda_l1 * g / n * sign(image - target); g = upstream_dev[0], the gradient of the loss VALUE, read on the device (NULL: 1).
 * loss3 (DEVICE float[3]) = {loss, mean |image - target|, mean SSIM}; workspace: nrc_photometric_loss_ws_floats(planes, H, W) floats; the three
 * derivative maps (planes x H x W each) as for nrc_ssim_forward (all NULL: value only).  planes = B * C, "same" padding. */
int64_t nrc_photometric_loss_ws_floats(int64_t planes, int32_t H, int32_t W);
int nrc_photometric_loss_forward(const float* image, const float* target, int64_t planes, int32_t H, int32_t W, float C1, float C2,
                                 float lambda_l1, float lambda_dssim, float* dm_dmu1, float* dm_dsigma1_sq, float* dm_dsigma12,
                                 float* workspace, float* loss3, nrc_stream_t stream);
int nrc_photometric_loss_backward(const float* image, const float* target, int64_t planes, int32_t H, int32_t W, float lambda_l1,
                                  float lambda_dssim, const float* upstream_dev, const float* dm_dmu1, const float* dm_dsigma1_sq,
                                  const float* dm_dsigma12, float* dL_dimage, nrc_stream_t stream);

/* =====================================================================================================
 * Group 8 -- fused Adam step: replaces apex.optimizers.FusedAdam (src/Thirdparty/Apex.py:17) as constructed at
 *            src/Methods/InstantNGP/Trainer.py:33-38 and src/Methods/GaussianSplatting/Model.py:131-136.  One flat f32 tensor
 *            per call (16-byte aligned pointers take the vector path).  bias_correction_k = 1 - beta_k^step (host).  adam_w_mode = 0: L2
 *            weight decay added to the gradient (apex ADAM_MODE_0), 1: decoupled.  grad_scale / found_inf: optional DEVICE
 *            scalars of torch.amp.GradScaler (gradient divided by *grad_scale; the whole step is skipped when *found_inf != 0).
 *            bias_corrections_dev (optional DEVICE float[2]) overrides the two host values: nrc_adam_prepare writes it once per
 *            group and step as 1 - beta^(host_step - *skipped_steps) and advances *skipped_steps when *found_inf != 0, so the
 *            effective step count stands still on an overflow-skipped step (with apex the scaler does not call step() then)
 *            without a host read of found_inf.  With device_step (optional DEVICE int32, apex's capturable mode) host_step / skipped_steps are
 *            not used: the kernel advances *device_step itself unless *found_inf != 0, so a step recorded in a HIP graph counts on replay.
 *            lr_dev (optional DEVICE float) overrides lr for the same reason.  l2_slice_coeff / l2_slice_count: the gradient of the first
 *            l2_slice_count elements gets + l2_slice_coeff * parameter -- the reference's weight-decay LOSS term on the MLP weights in front of
 *            the hash table (InstantNGP/Model.py:38-44, Loss.py:15: 0.5e-6 * mean w^2 -> coeff 1e-6 / n) applied where the parameters are
 *            read anyway, instead of a dense 12 M-element gradient through autograd; 0 / 0 = off.  param_f16_out (optional): the updated parameters are also written as fp16 --
 *            the compute copy the tinycudann replacement reads (Group 3), which therefore can never go stale after a step.
 * ===================================================================================================== */
/* GradScaler's inf / NaN check of one f32 gradient tensor (torch.amp.GradScaler._check_inf_per_device, used at InstantNGP/Trainer.py:89-93 with an
 * optimizer that applies the scale itself): *found_inf (DEVICE f32, not cleared here) is set to 1 when any of the n values is not finite. */
int nrc_nonfinite_check(const float* grad, int64_t n, float* found_inf, nrc_stream_t stream);
/* The same for up to four tensors in ONE launch (an entry with n = 0 is skipped): the two parameter vectors of the InstantNGP model. */
int nrc_nonfinite_check4(const float* g0, int64_t n0, const float* g1, int64_t n1, const float* g2, int64_t n2, const float* g3, int64_t n3,
                         float* found_inf, nrc_stream_t stream);
int nrc_adam_prepare(int32_t host_step, float beta1, float beta2, const float* found_inf, int32_t* skipped_steps,
                     int32_t* device_step, float* bias_corrections, nrc_stream_t stream);
int nrc_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int32_t adam_w_mode, float bias_correction1,
                  float bias_correction2, const float* bias_corrections_dev, const float* lr_dev, const float* grad_scale,
                  const float* found_inf, void* param_f16_out, float l2_slice_coeff, int64_t l2_slice_count, nrc_stream_t stream);
/* nrc_adam_step on up to 12 tensors in ONE launch, each with its own learning rate and bias corrections (host values: the plain, non-capturable step of
 * apex.optimizers.FusedAdam over several single-tensor groups -- src/Methods/GaussianSplatting/Model.py:121-138 builds six; apex's multi_tensor_apply).
 * params / grads / exp_avg / exp_avg_sq: HOST arrays of n_tensors device pointers; sizes / lrs / bias_correction1 / bias_correction2: HOST arrays.
 * Same arithmetic per element as nrc_adam_step (csrc/adam_math.h). */
int nrc_adam_step_multi(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                        const int64_t* sizes, const float* lrs, const float* bias_correction1, const float* bias_correction2, float beta1, float beta2,
                        float eps, float weight_decay, int32_t adam_w_mode, nrc_stream_t stream);

/* =====================================================================================================
 * Group 9 -- mean squared distance to the 3 nearest neighbours (3DGS scale initialisation): replaces simple_knn._C.distCUDA2
 *            (src/Thirdparty/SimpleKNN.py:17-18, used at src/Optim/knn_utils.py:34-38).  The points must arrive in Morton order
 *            (Group 2 codes + a sort: nerficg_amd/simple_knn does both); out_sorted[i] belongs to sorted point i.  n >= 4.
 *            workspace: nrc_knn3_ws_bytes(n) bytes.  Exact (not approximate) neighbours.
 * ===================================================================================================== */
int64_t nrc_knn3_ws_bytes(int64_t n);
int nrc_knn3_mean_sq_dist(const float* points_morton_sorted, int64_t n, float* out_sorted, void* workspace, nrc_stream_t stream);

/* =====================================================================================================
 * Group 10 -- 3DGS densification bookkeeping on the device: replaces the boolean-mask / torch.cat surgery of
 *            src/Methods/GaussianSplatting/Model.py:157-246 and src/Optim/adam_utils.py:21-98.
 *   nrc_gs_densify_stats : add_densification_stats (Model.py:243-246): where radii > 0, grad_accum += |viewspace_grad[:, :2]|,
 *                          n_observations += 1.  viewspace_grad is (P, ld) f32 (ld = 3 or 4 as the rasterizer hands it out).
 *   nrc_gs_densify_plan  : densify_and_prune (Model.py:226-241) as a row list.  grads = accum / max(n_obs, 1); clone where
 *                          grads >= grad_threshold and max exp(log_scale) <= dense_extent (= percent_dense * cameras_extent), split
 *                          where it is larger; prune where sigmoid(opacity_logit) < min_opacity or (max_scale > 0 and) max scale >
 *                          max_scale, applied to originals, clones and the two /1.6 children like the reference's final prune.
 *                          Row o of the resulting arrays comes from Gaussian src[o]; kind[o] = 0 kept original, 1 clone, 2 split
 *                          child with aux[o] = row of the (2 * counts[4], 3) standard-normal tensor (else -1).  Order as the
 *                          reference leaves it: originals, clones, children copy 0, children copy 1.  src/kind/aux need 2 * P
 *                          entries.  counts[5] = {rows out, kept originals, kept clones, kept children per copy, split selected}.
 *                          grad_accum == n_observations == NULL: prune only.  grad_threshold must be > 0 (a threshold <= 0 would
 *                          also split the fresh clones; NRC_ERR_UNSUPPORTED).  workspace: nrc_gs_densify_plan_ws_bytes(P).
 *   nrc_gs_densify_split_children : positions / log-scales of the kind-2 rows (Model.py:196-202): R(q) (z * exp(log_scale)) + p and
 *                          log(exp(log_scale) / 1.6); z = noise[aux[o]] are the draws of torch.normal(0, std) before scaling.
 *   nrc_gather_rows      : out[t][o, :] = in[t][src[o], :] for up to 24 f32 tensors of row_floats[t] floats per row in one launch
 *                          (prune / extend / sort of src/Optim/adam_utils.py:21-98 for every group and both Adam moments at once);
 *                          tensors with zero_new[t] != 0 get zeros in rows with kind[o] != 0 (the moments of new Gaussians).  in, out,
 *                          row_floats, zero_new are HOST arrays of n_tensors entries; kind may be NULL (pure permutation / prune).
 *   nrc_scatter_rows     : the inverse for a list of distinct rows: out[t][dst[r], :] = in[t][r, :], r < n_in (the reduced union rows of a view-parallel
 *                          step go back into the gradient tensors: nerficg_amd.parallel.UnionRowExchange; no reference counterpart).
 *   nrc_compact_mask     : indices[0..*count) = ascending positions where mask != 0 (u8); workspace nrc_compact_mask_ws_bytes(n).
 * ===================================================================================================== */
int nrc_gs_densify_stats(const float* viewspace_grad, int32_t ld, const int32_t* radii, int64_t P, float* grad_accum,
                         int32_t* n_observations, nrc_stream_t stream);
int64_t nrc_gs_densify_plan_ws_bytes(int64_t P);
int nrc_gs_densify_plan(const float* grad_accum, const int32_t* n_observations, const float* log_scales, const float* opacity_logits,
                        int64_t P, float grad_threshold, float dense_extent, float min_opacity, float max_scale, int32_t* src,
                        int32_t* kind, int32_t* aux, int32_t* counts, void* workspace, nrc_stream_t stream);
int nrc_gs_densify_split_children(const int32_t* src, const int32_t* kind, const int32_t* aux, int64_t n_out, const float* positions,
                                  const float* log_scales, const float* rotations, const float* noise, float* positions_out,
                                  float* log_scales_out, nrc_stream_t stream);
int nrc_gather_rows(const float* const* in, float* const* out, const int32_t* row_floats, const int32_t* zero_new, int32_t n_tensors,
                    const int32_t* src, const int32_t* kind, int64_t n_out, nrc_stream_t stream);
int nrc_scatter_rows(const float* const* in, float* const* out, const int32_t* row_floats, int32_t n_tensors, const int32_t* dst, int64_t n_in,
                     nrc_stream_t stream);
int64_t nrc_compact_mask_ws_bytes(int64_t n);
int nrc_compact_mask(const uint8_t* mask, int64_t n, int32_t* indices, int32_t* count, void* workspace, nrc_stream_t stream);

/* =====================================================================================================
 * Group 11 -- InstantNGP occupancy-grid maintenance in one call: replaces the scratch-grid index_put, the
 *            where/maximum EMA, the masked mean pulled to the host and the packbits call of
 *            src/Methods/InstantNGP/Renderer.py:258-272.  grid (cascades, cells_per_cascade) f32 is updated in place:
 *            cells >= 0 become max(grid * decay, density sampled for the cell this round (0 if none; the maximum if several)), cells < 0
 *            (carved) stay.  threshold_out[0] = min(mean of the cells > 0, density_threshold) (NaN when there is none, like the
 *            reference's empty mean), threshold_out[1] = that mean; bitfield bit = cell > threshold_out[0] (raymarching.cu:138-161).
 *            cell_indices (cascades, samples_per_cascade) i64 Morton indices, densities the same shape, f32 (dtype 0) or f16 (1).
 *            Everything stays on the device (threshold_out is a DEVICE pointer to 2 floats).  cells_per_cascade % 8 == 0; grid and
 *            workspace 16-byte aligned; workspace: nrc_occupancy_update_ws_bytes(cascades * cells_per_cascade).
 * ===================================================================================================== */
int64_t nrc_occupancy_update_ws_bytes(int64_t n_cells_total);
int nrc_occupancy_update(float* grid, const int64_t* cell_indices, const void* densities, int32_t densities_dtype, int32_t cascades,
                         int64_t cells_per_cascade, int64_t samples_per_cascade, float decay, float density_threshold,
                         uint8_t* bitfield, float* threshold_out, void* workspace, nrc_stream_t stream);
/* Which cells are re-queried and where (src/Methods/InstantNGP/Renderer.py:183-206 cell choice, :251-258 positions): mode 0 = every cell
 * of every cascade (warm-up; per cascade grid_size^3 entries in Morton order), mode 1 = per cascade n_per_half cells drawn uniformly from
 * the grid followed by n_per_half cells drawn uniformly from occupied_indices[c * occupied_stride + [0, occupied_counts[c])) (Morton
 * indices of the cells with grid > threshold, e.g. from nrc_compact_mask; a cascade without any gets ignored entries, index -1).
 * cell_indices (cascades, per) i64 Morton indices, points (cascades * per, 3) f32 = box-centred query positions
 * ((coord / (G-1)) * 2 - 1) * (s - s/G) + U(-1,1) * s/G with s = min(2^(c-1), scale).  seed: DEVICE pointer to one i64; the draws are a pure
 * function of it (counter-based generator), so no host synchronisation and no dependence on the launch geometry. */
int nrc_occupancy_draw_cells(int32_t cascades, int32_t grid_size, float scale, int32_t mode, int64_t n_per_half, const int64_t* seed,
                             const int32_t* occupied_indices, const int32_t* occupied_counts, int64_t occupied_stride,
                             int64_t* cell_indices, float* points, nrc_stream_t stream);
/* Frustum / alpha-mask carving (Renderer.py:208-245).  remaining (cascades, G^3) u8, cell (x,y,z) at x + G*(y + G*z), initialised by the
 * caller to `subtractive`; one call per view: remaining = remaining OR seen (AND when subtractive), seen = the cell centre projects inside
 * the image (world -> camera (p - position) @ R, Datasets/utils.py:1027-1031; pinhole Perspective.py:39-52) with near < depth < far and,
 * when alpha_mask (height, width) f32 on the device is given, some pixel of the 3x3 neighbourhood of the hit pixel has alpha > 0.
 * c2w_rotation9 / position3 / center3 are HOST arrays.  nrc_occupancy_carve_finish dilates the survivors by one cell (3x3x3) and
 * writes grid[c][morton(x,y,z)] = 0 for them and -1 (never sampled again) for the rest. */
int nrc_occupancy_carve_view(uint8_t* remaining, int32_t cascades, int32_t grid_size, float scale, const float* center3,
                             const float* c2w_rotation9, const float* position3, float focal_x, float focal_y, float center_x,
                             float center_y, int32_t width, int32_t height, float near_plane, float far_plane,
                             const float* alpha_mask, int32_t subtractive, nrc_stream_t stream);
int nrc_occupancy_carve_finish(const uint8_t* remaining, int32_t cascades, int32_t grid_size, float* grid, nrc_stream_t stream);

/* =====================================================================================================
 * Group 12 -- stage timer (measurement; no reference counterpart).  bench.py's per-kernel roofline entries must be
 * timed with HIP events on the launch stream INSIDE the run that reports them; the kernels of one entry point are
 * launched back to back inside the library, where a caller cannot place events.  While armed, the multi-kernel entry
 * points (nrc_gs_preprocess / nrc_gs_bin_render / nrc_gs_backward, nrc_grid_backward, nrc_ngp_train_query_forward /
 * _backward) record an event behind each of their kernels; nothing is recorded inside a stream capture.
 *   _begin(capacity): clears the list, arms the timer (at most `capacity` marks are kept).
 *   _end: disarms, waits for the last mark, writes up to max_stages (name, milliseconds) pairs in launch order -- names as
 *         32-byte zero-terminated slots -- and the number written to *count (host pointers).
 * One harness, one stream, one call sequence at a time (not thread-safe).
 * ===================================================================================================== */
int nrc_stage_timer_begin(int32_t capacity);
int nrc_stage_timer_end(int32_t max_stages, char* names, float* ms, int32_t* count);

/* =====================================================================================================
 * Group 13 -- the InstantNGP training iteration on device-resident state (round 5).  Replaces, for ONE iteration of
 *            src/Methods/InstantNGP/Trainer.py:79-94: RayPoolSampler.get (Optim/Samplers/DatasetSamplers.py:53-66: ray_pool[ids]), `torch.rand(3)`,
 *            InstantNGPRayRenderingComponent.forward + render_rays_training (Renderer.py:55-84), InstantNGPLoss's colour term (Loss.py:15-22: mean
 *            squared error; the weight-decay term is FusedAdam's L2 slice, group 8), GradScaler.scale / .step / .update (Trainer.py:88-91) and
 *            FusedAdam.step -- as five enqueue-only calls, 13 kernel launches (the recorded iteration of round 4: 33).  Nothing is read back;
 *            every count the host may want (marched samples, dropped samples, loss) stays in device memory for the caller to look at when convenient.
 *
 *   nrc_ngp_train_march : the batch and its samples.  Ray n of the batch is pool row ids[n] (ids != NULL) or order[cursor[0] + n] (the
 *            resident sampling order; the call advances cursor[0] by the number of live rays).  n_rays_dev (DEVICE i32[1], NULL = ray_capacity):
 *            live rays; rows behind them become rays that miss the box (the batch size can change between replays of a recorded iteration).
 *            Outputs: rays_o (box-centred) / rays_d (ray_capacity,3), hits_t (ray_capacity,2) = [t_in, t_out] clipped to [near, far]
 *            (nrc_ngp_clip_rays values), target_rgb (ray_capacity,3) = pool_rgb, or lerp(bg, pool_rgb, pool_alpha).clamp(0,1) when pool_alpha is
 *            given (Datasets/utils.py:185-189), bg (3) = this iteration's random background; then the march of nrc_raymarching_train_capped on
 *            those rays with jitter noise[n]: rays_a, counter (uncut samples, live rays), xyzs / dirs / deltas / ts (sample_capacity rows, the
 *            unused tail inert), *overflow (may be NULL).  Random numbers: Philox4x32-10, key = rng_state[0] (seed), counter = (global ray
 *            index ray_offset + n | iteration rng_state[1]); the call advances rng_state[1].  bg_in (3) / noise_in (ray_capacity), when given,
 *            are used instead of the draws.  center3 / half3: HOST.  workspace: nrc_ngp_train_march_ws_bytes, ZEROED once by the caller
 *            (it starts with arrival counters that every call leaves at zero).  ray_capacity <= 32 768 (one wave per ray).
 *   nrc_ngp_train_query_forward (group 3) on (xyzs, dirs), n_samples_dev = counter: a launch sized for sample_capacity rows works on the rows that
 *            hold samples (min(counter[0], sample_capacity)); the same pointer goes to nrc_ngp_train_query_backward_cleared.
 *   nrc_ngp_train_loss  : compositing, `rgb + (1 - alpha) bg`, mean squared error against target_rgb over the live rays (counter[1]), times
 *            *loss_scale_dev (NULL = 1), and the whole way back: dL_dsigmas (M), dL_drgbs (M,3) of loss2[1] -- every row written.  loss2[0] =
 *            the loss, loss2[1] = scaled; ray_rgb / ray_alpha / ray_depth (optional) = the 'rgb' / 'alpha' / 'depth' of Renderer.py:83.  The same
 *            launch clears zero_a[0, n_zero_a) and zero_b[0, n_zero_b) (f32): what nrc_ngp_train_query_backward_cleared wants cleared.
 *            workspace: nrc_ngp_train_loss_ws_bytes(ray_capacity), zeroed once.
 *   nrc_ngp_train_query_backward_cleared : nrc_ngp_train_query_backward_set without its clearing launch; the caller has cleared
 *            grad_density_params[0, nrc_ngp_train_query_clear_floats(...)) and all of grad_color_params.
 *   nrc_amp_adam_step (group 8 family): GradScaler.step + FusedAdam(capturable).step + GradScaler.update for the (up to two) tensors of one
 *            parameter group in two launches.  Launch 1 checks the gradients for inf / NaN; its last workgroup holds or advances *device_step,
 *            writes bias_corrections (2), state4[1] = found_inf of this step, state4[2] = 1 / scale the gradients carry, and applies torch's
 *            scale update rule (back off on overflow; grow after growth_interval clean steps) to *scale / *growth_tracker (scale NULL: no
 *            scaler).  state4[3] (sticky): set when the Adam launch met an inf / NaN gradient element and left that element alone (round 6).  Launch 2 is the Adam update of nrc_adam_step for both tensors (skipped when found_inf).  state4 (f32[4]) and ticket
 *            (u32[272]: a two-level arrival counter) zeroed once by the caller.  lr_dev (NULL: the host value lr).  skipped_steps (optional, i32[1]): counts
 *            the steps an overflow skipped.
 * ===================================================================================================== */
/* InstantNGPModel.weight_decay_mlp (src/Methods/InstantNGP/Model.py:38-44: mean squared MLP weight over both networks) as one launch each way.
 *   nrc_sum_squares_two: out[0] = (sum a[0,n_a)^2 + sum b[0,n_b)^2) * inv_n, one workgroup, fixed order.
 *   nrc_clear_seed_two : what stands in front of nrc_ngp_train_query_backward_cleared -- grad_a[0,clear_a) / grad_b[0,clear_b) are cleared, and their
 *                        leading seed_a / seed_b elements start at coeff * upstream_dev[0] * w instead of zero: the gradient of the weight-decay term
 *                        (coeff = 2 / n, upstream = dL/d(term), DEVICE scalar) joins the networks' gradients without a dense 12 M-element tensor. */
/* InstantNGPLoss.forward (src/Methods/InstantNGP/Loss.py:18-26) as one launch: out3 = (mse + weight_decay_weight * wd, mse, wd) with
 * mse = mean((pred - target)^2) over n elements and wd = (sum a^2 + sum b^2) * inv_n_weights.  Backward: nrc_mse_scaled_backward for pred, and the
 * weight-decay gradient as seeds of nrc_clear_seed_two. */
int nrc_ngp_loss_forward(int64_t n, const float* pred, const float* target, const float* weights_a, int64_t n_a, const float* weights_b, int64_t n_b,
                         float inv_n_weights, float weight_decay_weight, float* out3, nrc_stream_t stream);
int nrc_sum_squares_two(const float* a, int64_t n_a, const float* b, int64_t n_b, float inv_n, float* out, nrc_stream_t stream);
int nrc_clear_seed_two(float* grad_a, int64_t clear_a, const float* w_a, int64_t seed_a, float* grad_b, int64_t clear_b, const float* w_b, int64_t seed_b,
                       const float* upstream_dev, float coeff, nrc_stream_t stream);
int64_t nrc_ngp_train_march_ws_bytes(int64_t ray_capacity, int32_t max_samples);
int nrc_ngp_train_march(const int64_t* ids, const int64_t* order, int64_t* cursor, const int32_t* n_rays_dev, int64_t ray_capacity, int64_t n_pool,
                        int64_t ray_offset, const float* pool_origin, const float* pool_dir, const float* pool_rgb, const float* pool_alpha,
                        const float* center3, const float* half3, float near_plane, float far_plane, const uint8_t* density_bitfield, int32_t cascades,
                        float scale, float exp_step_factor, int32_t grid_size, int32_t max_samples, uint64_t* rng_state, const float* bg_in,
                        const float* noise_in, int64_t sample_capacity, float* rays_o, float* rays_d, float* hits_t, float* target_rgb, float* bg,
                        int64_t* rays_a, int32_t* counter, float* xyzs, float* dirs, float* deltas, float* ts, int64_t* overflow, void* workspace,
                        nrc_stream_t stream);
int64_t nrc_ngp_train_loss_ws_bytes(int64_t ray_capacity);
int nrc_ngp_train_loss(const float* sigmas, const float* rgbs, const float* deltas, const float* ts, const int64_t* rays_a, const int32_t* counter,
                       int64_t ray_capacity, int64_t sample_capacity, float T_threshold, const float* bg_dev, const float* target_rgb,
                       const float* loss_scale_dev, float* ray_rgb, float* ray_alpha, float* ray_depth, float* loss2, float* dL_dsigmas, float* dL_drgbs,
                       float* zero_a, int64_t n_zero_a, float* zero_b, int64_t n_zero_b, void* workspace, nrc_stream_t stream);
int64_t nrc_ngp_train_query_clear_floats(int64_t M, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale,
                                         int64_t n_density_mlp_params, int64_t n_density_params);
int nrc_ngp_train_query_backward_cleared(const float* dL_dsigmas, const float* dL_drgbs, int64_t M, const float* x01,
                                         const void* density_weights_f16, const void* color_weights_f16, int32_t n_levels,
                                         int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, const void* h_f16,
                                         const void* rgb_f16, const void* save_in_d, const void* save_acts_d, const void* save_in_c,
                                         const void* save_acts_c, float loss_scale, float* grad_density_params, float* grad_color_params,
                                         int64_t n_density_mlp_params, int64_t n_density_params, int64_t n_color_params, void* scratch,
                                         const int32_t* n_samples_dev, nrc_stream_t fork_stream, nrc_stream_t stream);
/* nrc_ngp_train_query_backward_cleared + nrc_amp_adam_step as ONE call WITHOUT the pass over the gradients: found_inf is known before the grid
 * backward starts -- the two network backward launches flag every inf / NaN they hand on (input gradients, weight-gradient sums: state4[0]), and the
 * hash-grid gradient is a finite-weighted sum of those -- so one thread settles step counter / bias corrections / scale (state4 as in
 * nrc_amp_adam_step) behind them, and the 49 MB read of nrc_amp_adam_step's check goes away (7 launches: 2 network backward, 1 settle, 3 grid
 * backward, 1 Adam over both vectors).  fork_stream (optional, also on nrc_ngp_train_query_backward_cleared): a second stream of the caller's on
 * which the dense levels' atomics run next to the hashed levels' split / accumulate; joined before the call returns.  Same arithmetic per parameter
 * as nrc_adam_step (csrc/adam_math.h). */
int nrc_ngp_train_backward_step(const float* dL_dsigmas, const float* dL_drgbs, int64_t M, const float* x01, const void* density_weights_f16,
                                const void* color_weights_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution,
                                float per_level_scale, const void* h_f16, const void* rgb_f16, const void* save_in_d, const void* save_acts_d,
                                const void* save_in_c, const void* save_acts_c, float loss_scale, float* grad_density_params,
                                float* grad_color_params, int64_t n_density_mlp_params, int64_t n_density_params, int64_t n_color_params,
                                void* scratch, const int32_t* n_samples_dev, float* param_d, float* exp_avg_d, float* exp_avg_sq_d,
                                void* param_f16_d, float l2_coeff_d, int64_t l2_count_d, float* param_c, float* exp_avg_c, float* exp_avg_sq_c,
                                void* param_f16_c, float l2_coeff_c, int64_t l2_count_c, float lr, const float* lr_dev, float beta1, float beta2,
                                float eps, float weight_decay, int32_t adam_w_mode, int32_t* device_step, float* bias_corrections, float* scale,
                                int32_t* growth_tracker, float growth_factor, float backoff_factor, int32_t growth_interval, float* state4,
                                nrc_stream_t fork_stream, nrc_stream_t stream);
int nrc_amp_adam_step(float* param_a, const float* grad_a, float* exp_avg_a, float* exp_avg_sq_a, void* param_f16_a, int64_t n_a, float l2_coeff_a,
                      int64_t l2_count_a, float* param_b, const float* grad_b, float* exp_avg_b, float* exp_avg_sq_b, void* param_f16_b, int64_t n_b,
                      float l2_coeff_b, int64_t l2_count_b, float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                      int32_t adam_w_mode, int32_t* device_step, float* bias_corrections, float* scale, int32_t* growth_tracker, float growth_factor,
                      float backoff_factor, int32_t growth_interval, float* state4, void* ticket, int32_t* skipped_steps, nrc_stream_t stream);

/* =====================================================================================================
 * Group 14 -- the training iteration of a DATA-PARALLEL rank, in pieces (round 6).  The reference has no counterpart (its DataParallel wrapper is a
 *            no-op for ray batches, src/Methods/Base/Renderer.py:24-33); SURVEY 8(e) names the shape: reduce-scatter of the gradients, Adam on the
 *            rank's 1/N of the parameters, all-gather of what the kernels read.  The collectives are the host's (torch.distributed over RCCL); these
 *            calls are what stands between them, enqueue-only like group 13:
 *   nrc_ngp_train_networks_backward : the two network launches of nrc_ngp_train_query_backward_cleared (same arguments); *nonfinite_flag (DEVICE f32,
 *            cleared by the caller) is set to 1 when a launch hands on an inf / NaN.  After it the MLP-weight gradients are final -- the caller's small
 *            all-reduce (both MLPs' gradients + the flag) can start while the grid backward runs.
 *   nrc_ngp_train_grid_backward     : the hash-grid backward of the same call (reads the input gradient the first call left in `scratch`).
 *   nrc_amp_settle                  : one thread: found_inf = (*flag_sum != 0) (a sum of the ranks' flags), step counter, bias corrections, scale update
 *            rule, state4[2] = 1 / (scale * grad_divisor) -- grad_divisor = world size when the gradients are a SUM over the ranks.  state4 as in nrc_amp_adam_step.
 *   nrc_wire_pack_f16 / nrc_wire_unpack_f16 : the optional 16-bit wire of the table's reduce-scatter -- f32 -> fp16 round-to-nearest, saturating at +-65504
 *            (*saturated, optional DEVICE u64, counts the clamped values; NaN stays NaN), and the reduced shard back to f32.  Halves the reduce-scatter's
 *            bytes; the sum over the ranks is then formed in fp16 (what tiny-cuda-nn's own fp16 gradient storage does under the same loss scale).  Off by default.
 *   nrc_amp_adam_slices             : the Adam launch of nrc_amp_adam_step on two arbitrary slices (pointers already offset; l2_count relative to the
 *            slice) -- a rank's shard of the table, or the replicated MLP weights.  Skipped when state4[1] says so.  Either slice may be empty.
 * ===================================================================================================== */
int nrc_ngp_train_networks_backward(const float* dL_dsigmas, const float* dL_drgbs, int64_t M, const float* x01, const void* density_weights_f16,
                                    const void* color_weights_f16, int32_t n_levels, int32_t log2_hashmap_size, int32_t base_resolution,
                                    float per_level_scale, const void* h_f16, const void* rgb_f16, const void* save_in_d, const void* save_acts_d,
                                    const void* save_in_c, const void* save_acts_c, float loss_scale, float* grad_density_params,
                                    float* grad_color_params, int64_t n_density_mlp_params, int64_t n_density_params, int64_t n_color_params,
                                    void* scratch, const int32_t* n_samples_dev, float* nonfinite_flag, nrc_stream_t stream);
int nrc_ngp_train_grid_backward(int64_t M, const float* x01, const void* density_weights_f16, const void* color_weights_f16, int32_t n_levels,
                                int32_t log2_hashmap_size, int32_t base_resolution, float per_level_scale, float* grad_density_params,
                                float* grad_color_params, int64_t n_density_mlp_params, int64_t n_density_params, int64_t n_color_params, void* scratch,
                                const int32_t* n_samples_dev, nrc_stream_t fork_stream, nrc_stream_t stream);
int nrc_wire_pack_f16(const float* src, void* dst_f16, int64_t n, uint64_t* saturated, nrc_stream_t stream);
int nrc_wire_unpack_f16(const void* src_f16, float* dst, int64_t n, nrc_stream_t stream);
int nrc_amp_settle(const float* flag_sum, float grad_divisor, float beta1, float beta2, int32_t* device_step, float* bias_corrections, float* scale,
                   int32_t* growth_tracker, float growth_factor, float backoff_factor, int32_t growth_interval, float* state4, int32_t* skipped_steps,
                   nrc_stream_t stream);
int nrc_amp_adam_slices(float* param_a, const float* grad_a, float* exp_avg_a, float* exp_avg_sq_a, void* param_f16_a, int64_t n_a, float l2_coeff_a,
                        int64_t l2_count_a, float* param_b, const float* grad_b, float* exp_avg_b, float* exp_avg_sq_b, void* param_f16_b, int64_t n_b,
                        float l2_coeff_b, int64_t l2_count_b, float lr, const float* lr_dev, float beta1, float beta2, float eps, float weight_decay,
                        int32_t adam_w_mode, const float* bias_corrections, const float* state4, nrc_stream_t stream);

/* =====================================================================================================
 * Group 15 -- the regularisers on the 3DGS depth and alpha maps as three launches: replaces depth_smoothness_loss
 *            (src/Optim/Losses/DepthSmoothness.py:31-43), background_entropy (src/Optim/Losses/BackgroundEntropy.py:6-8) and the
 *            depth / (alpha + 1e-6) normalisation in front of them (InstantNGP/Renderer.py:82), ~30 tensor operations forward and as many backward.
 *            All f32, contiguous: depth (B, H, W) -- the rasterizer's accumulated depth sum w z, or any depth map --, alpha (B, H, W),
 *            image (B, C, H, W), 1 <= C <= 4.
 *              d = normalize ? depth / (alpha + 1e-6f) : depth;   lap_x = d[x-1] + d[x+1] - 2 d[x], x in [1, W-2];   w_x = exp(-mean_c |I_c[x] - I_c[x-1]|);
 *              S_x = mean over B H (W-2) of |lap_x w_x|, S_y the same along y over B (H-2) W;   a = clamp(alpha, 1e-6f, 1 - 1e-6f) (the bounds as f32);
 *              E = mean(-a log a), with symmetrical mean(-a log a - (1-a) log(1-a));   loss = lambda_smooth (S_x + S_y) + lambda_entropy E.
 *   _forward : a stencil launch writes per-workgroup partial sums (no atomics), one workgroup adds them in a fixed order with double accumulators:
 *              loss4 (DEVICE float[4]) = {loss, S_x, S_y, E}, bit-identical from call to call.  workspace: nrc_map_losses_ws_floats(B, H, W) floats,
 *              16-byte aligned.
 *   _backward: one stencil launch, a gather (no atomics).  dL_ddepth (B,H,W), dL_dalpha (B,H,W), dL_dimage (B,C,H,W): each is written when its pointer
 *              is non-null (at least one must be).  dL_dalpha = the normalisation's -g_d depth / (alpha + 1e-6)^2 (with normalize) + the entropy term (zero
 *              outside the clamp, passed at the bounds like torch.clamp); sign(0) = 0 throughout.  upstream_dev: the gradient of the loss VALUE, a DEVICE
 *              scalar (NULL: 1), as for nrc_photometric_loss_backward.
 *   A weight of zero skips that term's work: lambda_smooth == 0 allows depth == image == NULL (and writes neither dL_ddepth nor dL_dimage),
 *   lambda_entropy == 0 skips the entropy.  NRC_ERR_INVALID before any HIP call: a null required pointer, B < 1 (or > 65535), C outside 1..4, H < 3 or
 *   W < 3 (the reference's mean over an empty set is NaN there), both weights zero.
 * ===================================================================================================== */
int64_t nrc_map_losses_ws_floats(int64_t B, int32_t H, int32_t W);
int nrc_map_losses_forward(const float* depth, const float* alpha, const float* image, int64_t B, int32_t C, int32_t H, int32_t W, int32_t normalize,
                           float lambda_smooth, float lambda_entropy, int32_t symmetrical, float* workspace, float* loss4, nrc_stream_t stream);
int nrc_map_losses_backward(const float* depth, const float* alpha, const float* image, int64_t B, int32_t C, int32_t H, int32_t W, int32_t normalize,
                            float lambda_smooth, float lambda_entropy, int32_t symmetrical, const float* upstream_dev, float* dL_ddepth, float* dL_dalpha,
                            float* dL_dimage, nrc_stream_t stream);

/* =====================================================================================================
 * Group 16 -- 3DGS-MCMC (Kheradmand et al., "3D Gaussian Splatting as Markov Chain Monte Carlo", NeurIPS 2024): the steps that replace clone / split /
 *            prune.  The method's source is not part of the reference tree; these comments are the specification.  All on the RAW training parameters,
 *            f32, contiguous: opacity_logits (P) with o = sigmoid(logit), log_scales (P, 3) with s = exp(log_scale), rotations (P, 4) with
 *            q = rotation / max(|rotation|, 1e-12), real part first, R = R(q) (the matrix of nrc_gs_densify_split_children), positions (P, 3).
 *            Every call: NRC_ERR_INVALID before any launch for P < 0 or a null required pointer; P == 0 is a successful no-op.
 *
 *   nrc_gs_mcmc_noise: the SGLD noise on the positions, after the optimizer step of every iteration, in place:
 *              gate = 1 / (1 + exp(-100 ((1 - o) - 0.995)));   v = z * gate * (noise_lr * lr);   x += R diag(s^2) R^T v;   z ~ N(0, I3).
 *            lr_dev (optional DEVICE f32) replaces lr, device_step (optional DEVICE i32) replaces iteration: a capturable optimizer's own scalars, so that
 *            a step recorded in a HIP graph does not replay one draw.  z_in (optional, (P, 3)): the caller's draw.  Without it the kernel draws:
 *            Philox4x32-10, counter = (index lo, index hi, iteration lo, iteration hi), key = (seed lo, seed hi), index = row_offset + local row (the
 *            Gaussian's GLOBAL row: the draw does not depend on the rank or on how P is cut into launches); the four words w0..w3 become
 *              ua = ((w0 >> 8) + 1) 2^-24,  ub = (w1 >> 8) 2^-24,  uc = ((w2 >> 8) + 1) 2^-24,  ud = (w3 >> 8) 2^-24,
 *              z0 = sqrt(-2 ln ua) cos(2 pi ub),  z1 = sqrt(-2 ln ua) sin(2 pi ub),  z2 = sqrt(-2 ln uc) cos(2 pi ud)      (|z| <= 5.77).
 *            z_out (optional, (P, 3)) receives the draw that was used.  One streaming launch: 44 B read and 12 B written per Gaussian.
 *
 *   nrc_gs_mcmc_relocation: one Gaussian that was drawn count times becomes one of N = clamp(count + 1, 1, 50) stacked copies that render like it did;
 *            rows with count <= 0 are not touched.  In place on opacity_logits and log_scales, evaluated in f64 and rounded once:
 *              o_new = 1 - (1 - o)^(1/N);   denom = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k / sqrt(k+1) o_new^(k+1);   s_new = (o / denom) s;
 *              o_new <- clamp(o_new, 0.005, 1 - 2^-24);   logit_new = log(o_new / (1 - o_new));   log_scale_new = log(s_new).
 *            (At the centre the copies composite to 1 - (1 - o_new)^N = o; along any line through the centre the integral of the composited opacity,
 *            sigma_new sqrt(2 pi) denom, equals o sigma sqrt(2 pi).)  moments: HOST array of n_moments <= 12 DEVICE pointers, moment_row_floats: HOST
 *            array of their floats per row (the convention of nrc_gather_rows): rows with count > 0 are cleared in the same launch (both Adam moments
 *            of the six groups).  More than 12: NRC_ERR_INVALID.  opacity_out (P), scales_out (P, 3), both optional: the clamped o_new and s_new as
 *            f32, written for the rows with count > 0 only.
 *
 *   nrc_gs_mcmc_regularise: L_o = opacity_reg mean(o), L_s = scale_reg mean(s); the gradients are ADDED to what the backward pass left:
 *              grad_opacity_logits[i] += opacity_reg / P * o_i (1 - o_i);   grad_log_scales[i][j] += scale_reg / (3 P) * s_ij
 *            (each the f32 rounding of the f64 sum), losses (DEVICE float[2]) = {L_o, L_s}: one slab of plain stores per workgroup, added in f64 in a
 *            fixed order by a finishing launch -- no atomics, bit-identical from call to call.  workspace: nrc_gs_mcmc_regularise_ws_bytes(P) bytes,
 *            8-byte aligned.
 * ===================================================================================================== */
int nrc_gs_mcmc_noise(const float* rotations, const float* log_scales, const float* opacity_logits, float* positions, int64_t P, int64_t row_offset,
                      float noise_lr, float lr, const float* lr_dev, uint64_t seed, uint64_t iteration, const int32_t* device_step, const float* z_in,
                      float* z_out, nrc_stream_t stream);
int nrc_gs_mcmc_relocation(float* opacity_logits, float* log_scales, const int32_t* count, int64_t P, float* const* moments, const int32_t* moment_row_floats,
                           int32_t n_moments, float* opacity_out, float* scales_out, nrc_stream_t stream);
int64_t nrc_gs_mcmc_regularise_ws_bytes(int64_t P);
int nrc_gs_mcmc_regularise(const float* opacity_logits, const float* log_scales, int64_t P, double opacity_reg, double scale_reg, float* grad_opacity_logits,
                           float* grad_log_scales, float* losses, void* workspace, nrc_stream_t stream);

/* =====================================================================================================
 * Group 17 -- the vanilla NeRF block, INFERENCE forward, as one kernel (csrc/nerf_net.hip).  Replaces src/Methods/NeRF/Model.py:59-83
 *            (NeRFBlock.forward) and utils.py:12-36 (FrequencyEncoding.forward) under no_grad: frequency encodings, n_layers x (Linear W + ReLU) with
 *            the encoded position re-entering behind every layer of the skip set, density head (Linear(W, 1) + ReLU), feature layer (Linear(W, W)),
 *            colour head (Linear(W + n_dir, W/2) + ReLU, (n_color_layers - 1) x (Linear(W/2, W/2) + ReLU), Linear(W/2, 3) + Sigmoid).
 *            cfg = (width, n_layers, n_color_layers, n_frequencies_position, n_frequencies_direction, append_input, skip_mask); bit k of skip_mask:
 *            the input of layer k (0-based) is [hidden, encoded position], i.e. k is in the module's input_skips, 1 <= k <= n_layers - 1.
 *            Supported: width 128 or 256, n_layers 1..8, n_color_layers 1..3, n_frequencies_position 0..10 with encoded width 1..64,
 *            n_frequencies_direction 0..4 with encoded width 1..32, any such skip_mask.  Everything else: nrc_nerf_supported = 0, the other calls
 *            NRC_ERR_UNSUPPORTED.  Arithmetic contract (fp16 operands, f32 accumulation from the f32 bias, convert -> ReLU -> saturate at 65504,
 *            sigma / rgb straight from the accumulator, accurate sincosf with |error| <= 2^-22): top of csrc/nerf_net.hip, DESIGN.md.
 *
 *   nrc_nerf_tile_rows: rows per workgroup (the sizes at which a launch gains a workgroup).
 *   nrc_nerf_packed_bytes: size of the packed blob (fp16 weight fragments in the order the forward kernel reads them, then f32 biases).
 *   nrc_nerf_pack_weights: params = HOST array of n_params = 2 x linears DEVICE f32 pointers, (weight, bias) of initial_layers[0..], density_layer,
 *            feature_layer, the colour head's linears in order; copied into the launch's arguments, one kernel, no host sync, capturable.
 *            blob: DEVICE, 16-byte aligned.
 *   nrc_nerf_block_forward: positions (M, 3) f32; directions (ceil(M / dir_group), 3) f32 -- row i reads direction row i / dir_group (1 = per sample,
 *            S = per ray of S consecutive samples); sigma (M) f32, rgb (M, 3) f32.  tap = 0: production.  tap = t > 0 (a separate instantiation):
 *            additionally writes the fp16 operand of stage t of [enc_pos, enc_dir, H_1 .. H_L, F, C_1 .. C_n] (1-based) to tap_out (M, width of the
 *            stage), unpadded, row-major.  M == 0: NRC_OK without a launch.  M < 0, dir_group < 1, a tap out of range, a null pointer: NRC_ERR_INVALID.
 * ===================================================================================================== */
int nrc_nerf_supported(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                       int32_t append_input, int32_t skip_mask);
int nrc_nerf_tile_rows(void);
int64_t nrc_nerf_packed_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                              int32_t append_input, int32_t skip_mask);
int nrc_nerf_pack_weights(const float* const* params, int32_t n_params, int32_t width, int32_t n_layers, int32_t n_color_layers,
                          int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, void* blob,
                          nrc_stream_t stream);
int nrc_nerf_block_forward(const float* positions, const float* directions, int64_t dir_group, int64_t M, const void* blob, int32_t width,
                           int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                           int32_t append_input, int32_t skip_mask, float* sigma, float* rgb, int32_t tap, void* tap_out, nrc_stream_t stream);

/* =====================================================================================================
 * Group 18 -- the vanilla NeRF block, TRAINING: a forward that keeps what the backward needs, and the backward through the whole block
 *            (csrc/nerf_net.hip: k_nerf_forward<W, 2>; csrc/nerf_grad.hip).  Replaces autograd through NeRFBlock.forward (Model.py:59-83) for the block's
 *            PARAMETERS; positions and directions receive theirs from group 20.  cfg as in group 17.  Supported: everything group 17 supports with
 *            n_color_layers = 1 (nrc_nerf_train_supported; a deeper colour head: NRC_ERR_UNSUPPORTED, the caller trains on torch).
 *            Arithmetic contract (fp16 MFMA operands, f32 accumulation, one power-of-two scale, fixed summation order): top of csrc/nerf_grad.hip.
 *
 *   nrc_nerf_train_workspace_bytes: one caller-allocated DEVICE buffer (16-byte aligned) shared by the forward and the backward of ONE batch of M rows;
 *            its layout is private.  With Mp = M rounded up to 128 rows and W = width it holds 256 bytes of header, the saved fp16 operands
 *            (Mp x 2 x (64 + 32 + (n_layers + 1) W + W / 2) bytes), the fp16 pre-activation gradients (Mp x 2 x (32 + (n_layers + 1) W + W / 2) bytes) --
 *            9 984 bytes per row for the 8 x 256 block -- and ceil(Mp / nrc_nerf_wgrad_chunk_rows()) f32 partial sums of about the parameter count
 *            each (2.4 MB per chunk for the 8 x 256 block).
 *   nrc_nerf_wgrad_chunk_rows: rows per partial sum of the weight gradient (the sizes at which the reduction gains a term).
 *   nrc_nerf_grad_params_floats: floats in grad_params = the block's parameter count.
 *   nrc_nerf_packed_transposed_bytes / nrc_nerf_pack_weights_transposed: the fp16 weights in the fragment order of the data gradient (W^T as the A operand),
 *            the SAME fp16 values as nrc_nerf_pack_weights stores (round-to-nearest-even, clamped at +-65504); params as there.  One kernel, no host
 *            sync, capturable.
 *   nrc_nerf_block_forward_train: nrc_nerf_block_forward with tap = 0, plus the workspace: sigma and rgb are bit-identical to that call on the same inputs
 *            and blob, and every saved stage operand (nrc_nerf_saved_stage) is bit-identical to what tap = stage + 1 returns.
 *   nrc_nerf_block_backward: d_sigma (M) f32, d_rgb (M, 3) f32: the upstream gradients; sigma, rgb: what the forward wrote; workspace: as the forward of the
 *            same M rows left it; blob_transposed: nrc_nerf_pack_weights_transposed of the same parameters.  grad_scale: 0 = automatic
 *            (2^(12 - floor(log2 max |head gradient|)), computed on the device), or a positive power of two in [2^-126, 2^126] (anything else:
 *            NRC_ERR_INVALID).  grad_params (nrc_nerf_grad_params_floats f32): per linear in the order of params -- weight (out, in) row-major, then
 *            bias -- UNSCALED gradients; every element is overwritten, nothing needs clearing.  stats (4 int32, DEVICE): [0] the exponent of the scale
 *            used, [1] gradient elements whose magnitude reached the fp16 overflow threshold before the conversion (they were saturated at +-65504),
 *            [2..3] 0.  No host synchronisation; five launches on `stream` in one linear order (capturable); two calls on the same inputs give the same bits.
 *   nrc_nerf_saved_stage / nrc_nerf_grad_stage (tests): one stage of the workspace as (M, width) row-major fp16.  Saved stages: 0 enc_pos, 1 enc_dir,
 *            2 .. n_layers + 1 H_1 .. H_L, n_layers + 2 F, n_layers + 3 C_1.  Gradient stages, in backward order: 0 rgb head (3 wide), 1 C_1 (W / 2),
 *            2 F, 3 sigma head (1 wide), 4 .. n_layers + 3 H_L .. H_1.
 *   M == 0: NRC_OK without a launch (nothing is written).  M < 0, dir_group < 1, a stage out of range, a null or misaligned pointer: NRC_ERR_INVALID.
 * ===================================================================================================== */
int nrc_nerf_train_supported(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                             int32_t append_input, int32_t skip_mask);
int64_t nrc_nerf_train_workspace_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                                       int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, int64_t M);
int nrc_nerf_wgrad_chunk_rows(void);
int64_t nrc_nerf_grad_params_floats(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                                    int32_t append_input, int32_t skip_mask);
int64_t nrc_nerf_packed_transposed_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                                         int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask);
int nrc_nerf_pack_weights_transposed(const float* const* params, int32_t n_params, int32_t width, int32_t n_layers, int32_t n_color_layers,
                                     int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, void* blob,
                                     nrc_stream_t stream);
int nrc_nerf_block_forward_train(const float* positions, const float* directions, int64_t dir_group, int64_t M, const void* blob, int32_t width,
                                 int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                                 int32_t append_input, int32_t skip_mask, float* sigma, float* rgb, void* workspace, nrc_stream_t stream);
int nrc_nerf_block_backward(const float* d_sigma, const float* d_rgb, const float* sigma, const float* rgb, int64_t M, const void* blob_transposed,
                            int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                            int32_t append_input, int32_t skip_mask, void* workspace, float grad_scale, float* grad_params, int32_t* stats,
                            nrc_stream_t stream);
int nrc_nerf_saved_stage(const void* workspace, int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                         int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, int64_t M, int32_t stage, void* out, nrc_stream_t stream);
int nrc_nerf_grad_stage(const void* workspace, int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position,
                        int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, int64_t M, int32_t stage, void* out, nrc_stream_t stream);

/* =====================================================================================================
 * Group 19 -- what surrounds the vanilla NeRF block (csrc/nerf_rays.hip): stratified sampling, compositing with its backward, and the fine pass's
 *            resampling with the sorted union of both depth sets.  Replaces src/Methods/NeRF/utils.py:57-75 (generate_samples), :78-109
 *            (generate_samples_from_pdf), :112-136 (integrate_samples) and, in src/Methods/NeRF/Renderer.py:54, :70 and :75, the position broadcast o + d t and
 *            sort(cat(t_coarse, t_fine)).  Dense: N rays x S samples, S the same for every ray, f32, row-major.  One wave per ray,
 *            nrc_nerf_rays_per_group() rays per workgroup.  One launch per call, no host synchronisation, no atomics, every reduction in a fixed order
 *            (two calls give the same bits; a ray's outputs do not depend on the other rays); capturable.  The arithmetic contract, operation by
 *            operation: top of csrc/nerf_rays.hip; restated in tests/nerf_rays_ref.py.
 *            Every call: NRC_ERR_UNSUPPORTED outside the supported sample counts, then NRC_ERR_INVALID before any launch for N < 0, a null required
 *            pointer or a pointer that is not 4-byte aligned; N == 0: NRC_OK without a launch.
 *
 *   nrc_nerf_rays_supported(S_coarse, S_fine): S_fine == 0 asks for sampling / compositing with S = S_coarse: 1 <= S <= 1024.  S_fine != 0 asks for
 *            resampling: 3 <= S_coarse <= 1024, 1 <= S_fine <= 1024, S_coarse + S_fine <= 2048.
 *   nrc_nerf_sample_coarse: origins, directions (N, 3); t_row (S): the caller's evenly spaced depths; u (N, S) or NULL.  t (N, S): t_row for every ray
 *            without u, otherwise lower + (upper - lower) u with the strata meeting at the mid points of t_row and the outer ones ending at t_row[0] /
 *            t_row[S-1].  positions (N S, 3) = o + d t, one multiplication and one addition per component.
 *   nrc_nerf_integrate_forward: t (N, S), directions (N, 3), sigma (N S), rgb_samples (N S, 3), background (3) or NULL, final_delta.  Segment length =
 *            (t[i+1] - t[i], the last one final_delta) |d|; a = 1 - expf(-sigma len); w = a T; the leftover transmittance goes to the background.
 *            rgb (N, 3), depth (N) = sum w t / alpha where the leftover is < 1, else 0; alpha (N) = 1 - leftover; weights (N, S).  No early-out.
 *   nrc_nerf_integrate_backward: upstream d_rgb (N, 3), d_alpha (N), d_weights (N, S), each may be NULL (= zero); the forward's inputs again.
 *            d_sigma (N S), d_rgb_samples (N S, 3).  The transmittance is recomputed; one reverse scan, no division by 1 - a.  No gradient to t, to the
 *            directions (group 20: nrc_nerf_integrate_backward_dirs) or through depth.
 *   nrc_nerf_sample_fine: t_coarse, weights (N, S_coarse); u with a row stride in ELEMENTS: 0 = one row of S_fine values shared by all rays, >= S_fine =
 *            one row per ray (anything between: NRC_ERR_INVALID); origins, directions (N, 3).  t (N, S_coarse + S_fine): the ascending sort of the multiset
 *            t_coarse u t_fine (FINITE inputs required); positions (N (S_coarse + S_fine), 3).  Optional, for tests (NULL = not written): cdf
 *            (N, S_coarse - 1) and t_fine (N, S_fine), unsorted, in the order of u.
 *   Stage-timer names: k_nerf_sample_coarse, k_nerf_integrate_fw, k_nerf_integrate_bw, k_nerf_sample_fine.
 * ===================================================================================================== */
int nrc_nerf_rays_per_group(void);
int nrc_nerf_rays_supported(int32_t S_coarse, int32_t S_fine);
int nrc_nerf_sample_coarse(const float* origins, const float* directions, const float* t_row, const float* u, int64_t N, int32_t S, float* t,
                           float* positions, nrc_stream_t stream);
int nrc_nerf_integrate_forward(const float* t, const float* directions, const float* sigma, const float* rgb_samples, const float* background,
                               float final_delta, int64_t N, int32_t S, float* rgb, float* depth, float* alpha, float* weights, nrc_stream_t stream);
int nrc_nerf_integrate_backward(const float* d_rgb, const float* d_alpha, const float* d_weights, const float* t, const float* directions, const float* sigma,
                                const float* rgb_samples, const float* background, float final_delta, int64_t N, int32_t S, float* d_sigma,
                                float* d_rgb_samples, nrc_stream_t stream);
int nrc_nerf_sample_fine(const float* t_coarse, const float* weights, const float* u, int64_t u_stride, const float* origins, const float* directions,
                         int64_t N, int32_t S_coarse, int32_t S_fine, float* t, float* positions, float* cdf, float* t_fine, nrc_stream_t stream);

/* =====================================================================================================
 * Group 20 -- the vanilla NeRF path's gradients to its INPUTS: sample positions and viewing directions through the block (csrc/nerf_input_grad.hip),
 *            ray origins and directions through o + d t and through the segment lengths of the compositor (csrc/nerf_rays.hip).  Opt-in
 *            (nerf.fused_apply / sample_coarse / sample_fine / composite / render_rays with input_grad=True); no call of groups 17 - 19 changes.
 *            cfg as in group 17; supported: whatever nrc_nerf_train_supported accepts.  The arithmetic contract (fp16 operands and one f32 accumulator for
 *            the encoded-input gradients, the f32 encoding backward with the forward's own sin / cos, the summation orders): top of
 *            csrc/nerf_input_grad.hip and csrc/nerf_rays.hip; restated in tests/nerf_input_grad_ref.py.
 *
 *   nrc_nerf_packed_input_bytes / nrc_nerf_pack_weights_input: a third weight stream, the SAME fp16 values as the two other blobs (round-to-nearest-even,
 *            clamped at +-65504), transposed with the encoded features as the m-tile rows in natural order: all of W_0, W_k[:, W : W + n_pos] for every
 *            skip bit k (ascending), W_colour[:, W : W + n_dir].  params as nrc_nerf_pack_weights.  One kernel, no host sync, capturable.
 *   nrc_nerf_block_input_grad: to be called after nrc_nerf_block_backward of the same M rows, with the workspace as that call left it, the same positions,
 *            directions and dir_group as the forward and the same grad_scale as the backward (0 = the automatic scale, read from the workspace header on
 *            the device).  d_positions (M, 3) f32, d_directions (ceil(M / dir_group), 3) f32: UNSCALED gradients, every element overwritten.  A group's
 *            d_directions is the sum of its rows' direction gradients in a fixed order (the last group may be partial); with dir_group > 1 the per-row
 *            values pass through the workspace's weight-gradient partial sums, which the backward has consumed (nothing else of the workspace is
 *            written: nrc_nerf_grad_stage / nrc_nerf_saved_stage read the same values afterwards), and a second small launch reduces them.  A row's
 *            d_positions and, with dir_group = 1, its d_directions depend on that row and the weights only; two calls give the same bits; no
 *            floating-point atomics; no host synchronisation; capturable.  Optional, for tests (NULL = not written): d_enc_pos (M, n_pos) and d_enc_dir
 *            (M, n_dir) f32, the gradients with respect to the encoded inputs, still scaled by the gradient scale.
 *            M == 0: NRC_OK without a launch.  M < 0, dir_group < 1, a grad_scale nrc_nerf_block_backward refuses, a null required pointer, a blob or
 *            workspace that is not 16-byte aligned, any other pointer that is not 4-byte aligned: NRC_ERR_INVALID before any launch.
 *   nrc_nerf_positions_backward: the backward of positions = o + d t.  d_positions (N S, 3), t (N, S) -> d_origins (N, 3) = sum_s g_s, d_directions (N, 3) =
 *            sum_s t_s g_s.  One wave per ray, fixed order, no atomics.  Validation as in group 19.
 *   nrc_nerf_integrate_backward_dirs: nrc_nerf_integrate_backward plus d_directions (N, 3), the gradient through the segment lengths (t[i+1] - t[i]) |d|:
 *            (d / |d|) sum_i q_i sigma_i Delta_i with q_i the factor whose product with len_i is d_sigma_i and the last Delta = final_delta; 0 where
 *            |d| = 0; finite for finite inputs with final_delta = 1e10.  d_sigma and d_rgb_samples are bit-identical to nrc_nerf_integrate_backward.  t
 *            receives no gradient and depth stays non-differentiable.  Validation as in group 19; d_directions is required.
 *   Stage-timer names: k_nerf_pack_i, k_nerf_input_grad, k_nerf_dir_reduce, k_nerf_positions_bw, k_nerf_integrate_bw_dirs.
 * ===================================================================================================== */
int64_t nrc_nerf_packed_input_bytes(int32_t width, int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction,
                                    int32_t append_input, int32_t skip_mask);
int nrc_nerf_pack_weights_input(const float* const* params, int32_t n_params, int32_t width, int32_t n_layers, int32_t n_color_layers,
                                int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input, int32_t skip_mask, void* blob,
                                nrc_stream_t stream);
int nrc_nerf_block_input_grad(const float* positions, const float* directions, int64_t dir_group, int64_t M, const void* blob_input, int32_t width,
                              int32_t n_layers, int32_t n_color_layers, int32_t n_frequencies_position, int32_t n_frequencies_direction, int32_t append_input,
                              int32_t skip_mask, void* workspace, float grad_scale, float* d_positions, float* d_directions, float* d_enc_pos, float* d_enc_dir,
                              nrc_stream_t stream);
int nrc_nerf_positions_backward(const float* d_positions, const float* t, int64_t N, int32_t S, float* d_origins, float* d_directions, nrc_stream_t stream);
int nrc_nerf_integrate_backward_dirs(const float* d_rgb, const float* d_alpha, const float* d_weights, const float* t, const float* directions,
                                     const float* sigma, const float* rgb_samples, const float* background, float final_delta, int64_t N, int32_t S,
                                     float* d_sigma, float* d_rgb_samples, float* d_directions, nrc_stream_t stream);

/* =====================================================================================================
 * Group 21 -- N-channel per-Gaussian features blended by the 3DGS rasterizer's own weights, differentiably (csrc/gs_features.hip).  No reference
 *            counterpart: the upstream rasterizer blends three colour channels, and ceil(C / 3) full calls with colors_precomp triples and bg = 0 are the
 *            only way to the same maps there.  Both calls run on the state a colour forward of group 4 left behind (point_list, ranges, splat_records,
 *            tile_order = the tile_fill of nrc_gs_bin_render*, n_contrib, final_T) for the same P, W, H and band: no preprocess, no sort, no binning.
 *
 *   features (P, C) f32, the caller's tensor, 1 <= C <= 256.  For a pixel p the blended set and the weights are the colour pass's own: the entries
 *            k <= n_contrib[p] of the tile's list with !(power > 0) and alpha >= 1/255, alpha = min(0.99, o exp(power)) in k_render's statements,
 *            T <- fmaf(-T, alpha, T), w_i = alpha_i T_i -- bit for bit the weight the colour received.
 *   nrc_gs_render_features_band: out_features (C, H, W), full frame, the band's pixel rows written: feature_map[c, p] = sum_i w_i(p) f[i, c] in list order
 *            as F = fmaf(f, w, F), background 0, NOT normalised by alpha.  P == 0: the band's rows are zero.  One launch, k_render_features.
 *   nrc_gs_backward_features_band: the backward of L = <dL_dfeature_map, feature_map> ((C, H, W), the band's rows read).  dL_dfeatures (P, C), fully written
 *            (rows no pixel blended are zero), may be NULL: dL/df[i, c] = sum_p w_i g_c(p).  The gradient through the weights,
 *            dL/dalpha_i(p) = T_i sum_c (f[i, c] - n_c) g_c with n_c <- alpha f_c + (1 - alpha) n_c walked back to front from final_T (no background term),
 *            is ADDED as six per-Gaussian sums (opacity, mean2D x, y, conic xx, xy, yy) to slots [3..8] of grad_records, the (P, 16) f32, 64-byte aligned
 *            workspace of nrc_gs_backward.  records_clear = 0: the call clears the records first; != 0: the caller guarantees they are zero.  The caller then
 *            MUST run one of nrc_gs_backward / _band / _aux_band / _pose_band with records_clear != 0 on the same frame state and the same band: its blend
 *            backward adds the colour's (and the maps') sums, and its per-Gaussian backward consumes and clears both -- dL_dmean2D, every leaf gradient and
 *            dL_dcamera of that call are then the gradients of colour + maps + features together.  (With a zero dL_dpix that call adds nothing of its
 *            own.)  There is no feature form of nrc_gs_backward_rest_step.  Sums are f32: LDS float atomics across a tile's blocks, one global float atomic
 *            per (tile, Gaussian, value), so two runs agree to rounding, not bitwise.  Launches: up to two clears, k_render_features_bw.
 *   C > 16 runs as ceil(C / 16) chunks in the second grid dimension of the one launch.  Neither call synchronises the host or reads anything back: both work
 *            inside a stream capture.  NRC_ERR_INVALID before any HIP call: a band that nrc_gs_*_band refuses; C < 1 or C > 256; P < 0, W < 1, H < 1; a null
 *            features, point_list or splat_records with P > 0; a null ranges, tile_order, n_contrib, out_features, final_T or dL_dfeature_map; grad_records
 *            null with P > 0 or not 64-byte aligned; splat_records not 16-byte aligned.
 * ===================================================================================================== */
int nrc_gs_render_features_band(int32_t P, int32_t C, int32_t W, int32_t H, const float* features, const int32_t* point_list, const uint32_t* ranges,
                                const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib, int32_t tile_row_begin, int32_t n_tile_rows,
                                float* out_features, nrc_stream_t stream);
int nrc_gs_backward_features_band(int32_t P, int32_t C, int32_t W, int32_t H, const float* features, const int32_t* point_list, const uint32_t* ranges,
                                  const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib, const float* final_T,
                                  const float* dL_dfeature_map, float* dL_dfeatures, float* grad_records, int32_t records_clear, int32_t tile_row_begin,
                                  int32_t n_tile_rows, nrc_stream_t stream);

/* =====================================================================================================
 * Group 22 -- per-Gaussian contribution statistics of a rendered 3DGS view (csrc/gs_contrib.hip).  No reference counterpart: the upstream rasterizer reports
 *            per pixel only.  The call stands in for what the compaction and scoring methods built on 3DGS each patch into their own rasterizer fork: the
 *            maximum blending weight over the training views (RadSplat pruning), hit counts and importance sums (LightGaussian, Mini-Splatting),
 *            error-weighted scores for densification (Taming-3DGS), sensitivity pruning (PUP 3D-GS) and the removal of Gaussians no view sees.  It runs on the
 *            state a colour forward of group 4 left behind (point_list, ranges, splat_records, tile_order = the tile_fill of nrc_gs_bin_render*, n_contrib)
 *            for the same P, W, H and band: no preprocess, no sort, no binning, one launch (k_gs_contributions).  Nothing here is differentiable.
 *
 *   The blended set of a pixel p and the weights are the colour pass's own, as in group 21: the entries k <= n_contrib[p] of the tile's list with
 *            !(power > 0) and alpha >= 1/255, alpha = min(0.99, o exp(power)) in k_render's statements, T <- fmaf(-T, alpha, T), w_i = alpha_i T_i -- bit for
 *            bit the weight the colour received.
 *   pixel_weights (H * W) f32, finite, or NULL (= 1 everywhere): the map m.  A pixel PARTICIPATES iff m(p) != 0.  Only the band's pixel rows are read.
 *   weight_sum (P) f32:  weight_sum[i] += sum over the participating pixels that blended i of m(p) w_i(p), accumulated in f32 (DPP row sums, LDS float atomics
 *            across a tile's blocks, one global float atomic per (tile, Gaussian): two runs agree to rounding, not bitwise).
 *   weight_max (P) f32:  weight_max[i] = max(weight_max[i], largest w_i(p) over the participating pixels that blended i): the colour's w, no rounding added.
 *            Compared as bit patterns: the buffer must hold values >= 0 (zeros, or an earlier call's maxima).
 *   hits (P) int32:      hits[i] += number of participating pixels that blended i, exact.
 *   All three ACCUMULATE into the caller's buffers (one call per view gives multi-view statistics); clear != 0 zeroes the wanted ones first.  Any of the three
 *            may be NULL (not wanted), not all three.  Gaussians outside every list are untouched.  The bands of a partition add up to the frame.
 *   P == 0: NRC_OK, no launch.  The call neither synchronises the host nor reads anything back: it works inside a stream capture.  NRC_ERR_INVALID before any
 *            HIP call: a band that nrc_gs_*_band refuses; P < 0, W < 1, H < 1; a null point_list or splat_records with P > 0; a null ranges, tile_order or
 *            n_contrib; all three outputs null; splat_records not 16-byte aligned; pixel_weights or an output not 4-byte aligned.
 * ===================================================================================================== */
int nrc_gs_contributions_band(int32_t P, int32_t W, int32_t H, const int32_t* point_list, const uint32_t* ranges, const float* splat_records,
                              const uint32_t* tile_order, const uint32_t* n_contrib, const float* pixel_weights, float* weight_sum, float* weight_max,
                              int32_t* hits, int32_t clear, int32_t tile_row_begin, int32_t n_tile_rows, nrc_stream_t stream);

/* =====================================================================================================
 * Group 23 -- absolute screen-space gradients of the 3DGS rasterizer (csrc/gs_raster.hip: k_render_bw<., true>).  The densification statistic of AbsGS, gsplat's
 *            absgrad=True, which Mip-Splatting and GOF rely on: the norm of dL_dmean2D is a SIGNED sum over pixels that cancels where a large Gaussian blurs
 *            fine texture; the sum of the per-pixel magnitudes does not.  It exists only inside the blend backward, before its row reduction.
 *
 *   nrc_gs_backward_absgrad_band : nrc_gs_backward_pose_band (dL_ddepth_alpha, pose_partials and dL_dcamera stay optional as there) + dL_dmean2D_abs (P, 3) f32:
 *            dL_dmean2D_abs[i][0] = sum over the band's tiles and the pixels that blended i of | -w (dx A + dy B) W/2 |
 *            dL_dmean2D_abs[i][1] = sum ...                                                   of | -w (dy C + dx B) H/2 |        dL_dmean2D_abs[i][2] = 0
 *            with w = o G dL/dalpha of the WHOLE call (colour, and with dL_ddepth_alpha the depth and alpha channels): the addends of dL_dmean2D[i][0..1], their
 *            absolute value taken PER PIXEL before any row, block, tile or band sum, in the units of dL_dmean2D (the factors W/2, H/2 included).  Every row is
 *            written: exact zeros for culled Gaussians and for Gaussians no pixel of the band blended.  Bands: the band's share; the shares of a partition sum
 *            to the frame's.  Every other output is the one nrc_gs_backward_pose_band computes from the same per-Gaussian sums (float atomics in another order).
 *   Gradient record (64 bytes, 16 f32 per Gaussian): [0..2] colour, [3] opacity, [4], [5] mean2D x, y, [6..8] conic xx, xy, yy, [9] dL/dz (depth-and-alpha
 *            backward only), [10], [11] sum |dL_pixel/dmean2D| x, y (this call only; never written otherwise), [12..15] free.  The call leaves every record it
 *            read all zero again, slots [10], [11] included.
 *   dL_dmean2D_abs == NULL: nrc_gs_backward_pose_band itself (same kernels, same launches).  P == 0: nothing is written to dL_dmean2D_abs.  The same validation
 *            before any HIP call as nrc_gs_backward_pose_band (bad band, dL_dcamera without or with a misaligned workspace, grad_records not 64-byte aligned).
 *            There is no absgrad form of nrc_gs_backward_rest_step or of nrc_gs_backward_features_band: the feature backward forms its share of dL/dalpha in
 *            another kernel, and |a + b| cannot be assembled from two kernels' sums.
 * ===================================================================================================== */
int nrc_gs_backward_absgrad_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg, const float* means3D, const float* shs,
                    const float* shs_rest, int32_t raw_parameters, const float* opacities, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list,
                    const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib,
                    const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest, float* dL_dscale, float* dL_drot, float* grad_records,
                    int32_t records_clear, int32_t tile_row_begin, int32_t n_tile_rows, const float* dL_ddepth_alpha, float* pose_partials,
                    float* dL_dcamera, float* dL_dmean2D_abs, nrc_stream_t stream);

/* =====================================================================================================
 * Group 24 -- the visibility-masked Adam step (csrc/adam_rows.hip: k_adam_rows).  The sparse step of Taming-3DGS, of 3DGS `--optimizer_type sparse_adam`
 *            (SparseGaussianAdam.step(visibility, N)) and of gsplat's SelectiveAdam: a Gaussian that the frame did not see keeps its parameters and both
 *            moments, every other row gets the ordinary update.  Added under ABI version 22 without a bump (additive, like group 23).
 *
 *   nrc_adam_step_rows_multi : up to 12 tensors in ONE launch, tensor k contiguous f32 of shape (n_rows, row_widths[k]), all sharing the row mask `visible`.
 *            The calling convention of nrc_adam_step_multi (group 8): params / grads / exp_avg / exp_avg_sq are HOST arrays of n_tensors device pointers;
 *            row_widths / lrs / bc1 / bc2 are HOST arrays (bc = the bias corrections 1 - beta^t, or 1).  visible is a DEVICE array of n_rows entries:
 *            visible_kind 0 = uint8 / bool, non-zero = visible; 1 = int32 radii as the rasterizer returns them, > 0 = visible.
 *            Row r visible: every element of row r of every tensor gets nrc_adam_update of csrc/adam_math.h (no L2 slice, inv_scale = 1) -- bit for bit what
 *            nrc_adam_step_multi does to it; weight decay (either mode) therefore acts on visible rows only.
 *            Row r invisible: its parameters, exp_avg and exp_avg_sq keep their bits, whatever its gradient holds (NaN and inf included).
 *            The work item is four consecutive floats; one none of whose elements is visible issues no load and no store of the four streams; inside a
 *            touched one the elements of invisible rows are written back as read.  16-byte accesses where all four pointers of a tensor are 16-byte
 *            aligned, single floats otherwise.  Element indices are 64-bit: n_rows * width may pass 2^31.  Nothing else may write the tensors meanwhile.
 *   NRC_ERR_INVALID before any HIP call: a null array or a null `visible`; n_tensors outside 1..12; a width <= 0; n_rows < 0; a visible_kind other than
 *            0 / 1; a bias correction <= 0; with n_rows > 0 a null tensor pointer.  n_rows == 0: NRC_OK, nothing is launched.
 * ===================================================================================================== */
int nrc_adam_step_rows_multi(int32_t n_tensors, float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                             const int32_t* row_widths, int64_t n_rows, const void* visible, int32_t visible_kind, const float* lrs, const float* bc1,
                             const float* bc2, float beta1, float beta2, float eps, float weight_decay, int32_t adam_w_mode, nrc_stream_t stream);

/* =====================================================================================================
 * Group 27 -- anti-aliased splats and the 3-D smoothing filter of Mip-Splatting (csrc/gs_raster.hip: k_preprocess<., true>, k_preprocess_bw<0 / 1, true>;
 *            csrc/gs_densify.hip: k_filter3d).  Upstream diff_gaussian_rasterization carries the first as the `antialiasing` field of
 *            GaussianRasterizationSettings (gsplat: rasterize_mode="antialiased"): the 0.3-pixel dilation of the projected 2-D covariance adds energy, and
 *            a model trained at one resolution dilates and brightens at another unless that energy is taken back.  Added under ABI version 22 without a bump
 *            (additive, like groups 23-26: no earlier signature, record slot or default launch changes).
 *
 *   With (a0, b, c0) the projected covariance BEFORE the dilation, a = a0 + 0.3, c = c0 + 0.3, det0 = a0 c0 - b^2, det1 = a c - b^2:
 *            comp = sqrt(max(0.000025, det0 / det1))                                                       (upstream's h_convolution_scaling, floor included)
 *   nrc_gs_preprocess_antialias_band : nrc_gs_preprocess_band, except that the opacity in conic_opacity[4 i + 3] and in the splat record is o comp (o after the
 *            sigmoid with raw_parameters).  Radii, tile rectangles, depths, conic, colour, lists and counts are bit for bit those of nrc_gs_preprocess_band, so
 *            every blend pass (colour, depth and alpha, features, contributions, their backwards) takes the compensated opacity without a change.
 *   nrc_gs_backward_antialias_band : nrc_gs_backward_absgrad_band (dL_ddepth_alpha and dL_dmean2D_abs stay optional as there) for a forward made by
 *            nrc_gs_preprocess_antialias_band.  With g = dL/d(o comp) (slot [3] of the gradient record): dL_dopacity = g comp (times o (1 - o) with
 *            raw_parameters), and where det0 / det1 > 0.000025, with k = g o / (2 comp),
 *                dL/da0 += k (c0 det1 - c det0) / det1^2    dL/dc0 += k (a0 det1 - a det0) / det1^2    dL/db += k (-2 b) (det1 - det0) / det1^2
 *            in front of the chain to cov3D, scales, rotations and means; at or below the floor nothing is added.  `opacities` is REQUIRED here also without
 *            raw_parameters (the activated values the forward read).  dL_dmean2D and dL_dmean2D_abs are those of nrc_gs_backward_absgrad_band.
 *            pose_partials / dL_dcamera: the camera backward has no anti-aliased form -- dL_dcamera != NULL returns NRC_ERR_UNSUPPORTED before any HIP call;
 *            there is no anti-aliased form of nrc_gs_backward_rest_step either.
 *   nrc_gs_filter3d : filter_3D (P) f32 from means3D (P, 3) and V views, `views` (V, 20) f32 on the device: the world-to-camera matrix row-major (16; p_cam =
 *            m[:3, :3] p + m[:3, 3]), fx, fy, W, H.  View v sees Gaussian i iff z > 0.2 and the pixel (x / z fx + W / 2, y / z fy + H / 2) lies in
 *            [-0.15 W, 1.15 W] x [-0.15 H, 1.15 H]; filter_3D[i] = sqrt(0.2) min over the seeing views of z / fx (f64 arithmetic on the promoted inputs, rounded
 *            once).  A Gaussian no view sees gets the largest value among the seen ones (0 when none is seen).  Two launches, no float atomics, the same
 *            bits on every call.  workspace: 4 bytes on the device.  NRC_ERR_INVALID before any HIP call: P < 0 or > 2^30, V < 1, a null views / workspace,
 *            with P > 0 a null means3D / filter_3D.  P == 0: NRC_OK, nothing is launched.
 * ===================================================================================================== */
int nrc_gs_preprocess_antialias_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* means3D, const float* shs,
                      const float* shs_rest, int32_t raw_parameters, const float* colors_precomp, const float* opacities, const float* scales, float scale_modifier,
                      const float* rotations, const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix,
                      const float* campos, const float* camera_dev, float tan_fovx, float tan_fovy, int32_t* radii, float* depths,
                      float* points_xy, float* conic_opacity, float* rgb, uint8_t* clamped, float* cov3D, uint32_t* tiles_touched,
                      uint32_t* tile_counts, uint32_t* ranges, uint32_t* tile_fill, uint32_t* bin_hist, int64_t span_capacity,
                      int64_t instance_capacity, float* splat_records, int64_t* num_rendered, int64_t* count_mailbox, int64_t mailbox_ticket,
                      int32_t tile_row_begin, int32_t n_tile_rows, uint8_t* band_mask, nrc_stream_t stream);
int nrc_gs_backward_antialias_band(int32_t P, int32_t D, int32_t M, int32_t W, int32_t H, const float* bg, const float* means3D, const float* shs,
                    const float* shs_rest, int32_t raw_parameters, const float* opacities, const float* colors_precomp, const float* scales, float scale_modifier, const float* rotations,
                    const float* cov3D_precomp, const float* viewmatrix, const float* projmatrix, const float* campos,
                    const float* camera_dev, float tan_fovx, float tan_fovy, const int32_t* radii, const float* points_xy, const float* conic_opacity,
                    const float* rgb, const uint8_t* clamped, const float* cov3D, const int32_t* point_list,
                    const uint32_t* ranges, const float* splat_records, const uint32_t* tile_order, const uint32_t* n_contrib,
                    const float* final_T, const float* dL_dpix,
                    float* dL_dmean2D, float* dL_dconic, float* dL_dopacity, float* dL_dcolor, float* dL_dmean3D,
                    float* dL_dcov3D, float* dL_dsh, float* dL_dsh_rest, float* dL_dscale, float* dL_drot, float* grad_records,
                    int32_t records_clear, int32_t tile_row_begin, int32_t n_tile_rows, const float* dL_ddepth_alpha, float* pose_partials,
                    float* dL_dcamera, float* dL_dmean2D_abs, nrc_stream_t stream);
int nrc_gs_filter3d(const float* means3D, int64_t P, const float* views, int32_t V, float* filter_3D, void* workspace, nrc_stream_t stream);

/* =====================================================================================================
 * Group 28 -- bilateral-grid colour correction (csrc/bilateral_grid.hip): the learned per-image post-process of "Bilateral Guided Radiance Field Processing"
 *            (Wang et al., SIGGRAPH 2024; gsplat: use_bilateral_grid).  Every training image owns a small 3-D grid of 3 x 4 colour transforms, sliced per pixel
 *            by position and luminance and applied to the rendered image before the loss; a total-variation term on the grids is added.  Added under ABI
 *            version 22 without a bump (additive, like groups 23-27).
 *
 *   grids (N, 12, L, Gh, Gw) f32, contiguous; channel c = 4 r + k is entry (r, k) of a 3 x 4 matrix.  The identity has channels 0, 5, 10 one, the rest zero.
 *   For pixel (x, y) of an H x W image with colour p = (p0, p1, p2), sliced with grid n:
 *            u = (x + 0.5) / W        v = (y + 0.5) / H        g = 0.299 p0 + 0.587 p1 + 0.114 p2
 *            along each axis a, with coordinate t in {u, v, g} and extent n_a in {Gw, Gh, L}:
 *                c_a = clamp(t, 0, 1) (n_a - 1);   i_a = min(floor(c_a), n_a - 2);   f_a = c_a - i_a        (n_a = 1: i_a = 0, f_a = 0, one vertex only)
 *            A(r,k) = sum over the <= 8 corners of  w_z w_y w_x G[n, 4r+k, i_z+dz, i_y+dy, i_x+dx],   w = f or 1 - f
 *            out_r  = A(r,0) p0 + A(r,1) p1 + A(r,2) p2 + A(r,3)
 *   Gradients: to G[n]: w_z w_y w_x d_out_r (p_k or 1); every other grid gets exactly zero.  To p, the linear part: sum_r d_out_r A(r,k); through the guidance:
 *            (0.299, 0.587, 0.114) (L - 1) sum_r d_out_r sum_k (dA(r,k)/dc_z) (p_k or 1), zero when g < 0 or g > 1; at g == 1 exactly (a white pixel) it takes the
 *            last cell's slope, at g == 0 the first cell's.  u and v carry no gradient.  On interior inputs this is grid_sample(mode='bilinear',
 *            align_corners=True, padding_mode='border') on the coordinates (2u - 1, 2v - 1, 2g - 1).
 *   Total variation: TV(G) = (1/N) sum_{axis in z,y,x} sum (G[.., i+1, ..] - G[.., i, ..])^2 / count_axis, count_axis = 12 (n_axis - 1) (product of the other two
 *            extents), the number of differences per grid along that axis; an axis of extent 1 contributes zero.
 *
 *   Pixels: element (y, x, channel ch) of rgb, out, d_out and d_rgb lies at (y W + x) pixel_stride + ch channel_stride floats -- (3, H, W) is (1, H W),
 *            (H, W, 3) is (3, 1).  idx: the grid index n as a host integer, or, when idx_dev != NULL, an int32 on the device read by the kernels (a captured
 *            iteration can change it; a device value outside [0, N) is clamped into it).
 *   nrc_bilagrid_ws_floats   : floats of the workspace that nrc_bilagrid_slice_backward (with d_grids) and nrc_bilagrid_tv_forward need for these shapes
 *            (H, W may be 0 for the TV term alone); the workspace is 16-byte aligned.
 *   nrc_bilagrid_slice_forward : out from grids, rgb; affine (H, W, 12) f32, the sliced matrices, is written when non-NULL (16-byte aligned).  One launch.
 *   nrc_bilagrid_slice_backward: d_rgb and / or d_grids (either may be NULL, not both; d_grids needs the workspace) from d_out.  d_grids (N, 12, L, Gh, Gw) is
 *            written whole: slice n holds the gradient, every other slice zeros.  The grid gradient is summed in a fixed order (per wave, per workgroup, then
 *            over the workgroups' partial windows in the workspace; no atomics): the same input gives the same bits on every call.  Two launches.
 *   nrc_bilagrid_tv_forward  : tv[0] = TV(grids); double sums in a fixed order, two launches.
 *   nrc_bilagrid_tv_backward : d_grids = upstream dTV/dG, the stencil (2 / (N count_axis)) (second difference) summed over the axes; upstream_dev: a device
 *            scalar (NULL: 1).  One launch.
 *   Nothing is read back and every size comes from the shapes: every call is capturable.  NRC_ERR_INVALID before any HIP call: a null pointer that is
 *            required, N, L, Gh or Gw < 1 (or an extent above 4096), H or W < 0, idx outside [0, N) when given on the host, a stride < 1.  An empty image
 *            (H == 0 or W == 0): NRC_OK; the forward launches nothing, the backward writes zeros into d_grids.
 * ===================================================================================================== */
int64_t nrc_bilagrid_ws_floats(int64_t N, int32_t L, int32_t Gh, int32_t Gw, int32_t H, int32_t W);
int nrc_bilagrid_slice_forward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, int32_t H, int32_t W, int64_t pixel_stride,
                               int64_t channel_stride, int64_t idx, const int32_t* idx_dev, float* out, float* affine, nrc_stream_t stream);
int nrc_bilagrid_slice_backward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, const float* rgb, const float* d_out, int32_t H, int32_t W,
                                int64_t pixel_stride, int64_t channel_stride, int64_t idx, const int32_t* idx_dev, float* workspace, float* d_rgb,
                                float* d_grids, nrc_stream_t stream);
int nrc_bilagrid_tv_forward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, float* workspace, float* tv, nrc_stream_t stream);
int nrc_bilagrid_tv_backward(const float* grids, int64_t N, int32_t L, int32_t Gh, int32_t Gw, const float* upstream_dev, float* d_grids, nrc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NERFICG_HIP_H */
