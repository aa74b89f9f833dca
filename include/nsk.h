/*
 * nsk.h -- C-ABI of the MI355X-native NICE-SLAM render / map / track hot path ("neural slam kernels").
 *
 * This is the drop-in boundary.  The reference exposes no FFI layer: its boundary is the
 * C++ class surface of include/Renderer.h:11-13, include/Mapper.h:20-25, include/Tracker.h:11-15 and
 * include/models/NICE.h:6-7, all of which hand libtorch tensors to stock libtorch ops.  The entry points below
 * are what thin Renderer / NICE / Mapper / Tracker classes with those exact signatures marshal into
 * (nice-slam-cpp_amd/host/); every entry point cites the reference code it replaces.
 *
 * Conventions
 *   - plain C, no torch types.  `d_` pointers are device (HIP) pointers, `h_` pointers are host pointers.
 *   - the caller owns every buffer it passes; the context owns grids, decoder parameters, their gradients
 *     and the Adam moments.
 *   - every function returns 0 on success, <0 on error; nsk_last_error() gives a thread-local message.
 *     (The reference defines no error behaviour: libtorch c10::Error exceptions propagate out of main.)
 *   - one nsk_ctx = one GPU + one HIP stream.  Calls are asynchronous on that stream unless stated; a context
 *     is not thread-safe, different contexts may be driven from different threads.
 *   - levels / stages / decoders share ids: 0 coarse, 1 middle, 2 fine, 3 color (src/models/NICE.cpp:16-52).
 *   - all arithmetic is fp32 (the reference's dtype); tolerance contract: 1e-4 relative L2 on rendered
 *     depth / colour and on optimised grids / poses.
 */
#ifndef NSK_H
#define NSK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NSK_COARSE 0
#define NSK_MIDDLE 1
#define NSK_FINE 2
#define NSK_COLOR 3

/* nsk_render_backward / nsk_map_step `flags` */
#define NSK_GRAD_GRIDS 1u     /* accumulate d loss / d grid features of the levels the stage reads         */
#define NSK_GRAD_DECODERS 2u  /* accumulate d loss / d decoder parameters of decoders marked trainable     */
#define NSK_GRAD_RAYS 4u      /* write d loss / d rays_o, d loss / d rays_d (Tracker, BA)                  */

/* Adam parameter groups, in the order of torch::optim::Adam's groups at src/Mapper.cpp:330 */
#define NSK_GROUP_DECODERS 0
#define NSK_GROUP_COARSE 1
#define NSK_GROUP_MIDDLE 2
#define NSK_GROUP_FINE 3
#define NSK_GROUP_COLOR 4
#define NSK_GROUP_CAMERA 5
#define NSK_NUM_GROUPS 6
#define NSK_MAX_POSE_FRAMES 32     /* frames of one nsk_pose_step_multi call (a mapping window; color_refine doubles mapping_window_size 5 -> 10) */

typedef struct nsk_ctx nsk_ctx;

const char* nsk_last_error(void);
int nsk_version(void);

/* ---- context ------------------------------------------------------------------------------------------- */
/* Replaces the 33 hard-coded torch::Device(torch::kCUDA,0) sites (e.g. src/Renderer.cpp:31,69,76).
 * hip_stream: a hipStream_t to launch on (NULL = the context creates its own non-blocking stream). */
int nsk_ctx_create(int device, void* hip_stream, nsk_ctx** out);
int nsk_ctx_destroy(nsk_ctx* ctx);
int nsk_sync(nsk_ctx* ctx);                         /* hipStreamSynchronize */
void* nsk_stream(nsk_ctx* ctx);                     /* the hipStream_t in use */

/* How the MLP decoders' FORWARD matrix products are evaluated (results agree within the 1e-4 contract; measured against the fp64
 * oracle all three are equally close, tests/test_gpu_parity.py::test_forward_bf16_split_mode_matches_oracle):
 *   2 = fp32 operands split into two fp16 pieces (x = h + l/2048: 22 significant bits), three v_mfma_f32_16x16x32_f16 per K=32
 *       block, fp32 accumulation (DEFAULT);
 *   1 = three bf16 pieces (24 significant bits, the full fp32 exponent range), six v_mfma_f32_16x16x32_bf16 per block;
 *   0 = v_mfma_f32_16x16x4_f32, plain fp32.
 * The mode governs the stages that run several decoders in one launch (fine, colour) of nsk_render_forward and of the steps.  Launches of
 * one decoder -- nsk_eval_points, nsk_eval_lattice, the coarse and middle stages -- and the coarse decoder everywhere run on the fp32 MFMA
 * in every mode.
 * Operand range, as tested (tests/test_gpu_operand_range.py: hidden values, grid features and weights moved by exact powers of two):
 *   mode 2: the 1e-4 contract holds for activations, grid features and weights with peak magnitudes from 2^-14 up to 2^15 (fp16's largest
 *       number is 65504); below 2^-14 the pieces lose bits gradually (fp16 subnormals are kept, not flushed).  An operand beyond 65504 has
 *       the pieces inf and -inf and its products are NaN: every ray that has such a sample is rendered NON-FINITE (NaN or +-inf in depth,
 *       colour, variance or weights), never as a finite wrong number;
 *   modes 1 and 0: no upper limit short of fp32's own.
 * Non-finite values already in the map (a diverged voxel, a NaN weight) propagate as in the reference: the hidden ReLUs and the
 * compositing's relu(sigma) pass a NaN of either sign on (torch::relu), -inf becomes 0; the outputs that ATen makes non-finite are
 * non-finite here, every other output is untouched, in all three modes.
 * Independent of the mode: the backward chains of the frozen decoders (without ray gradients) and of a trainable middle / colour
 * decoder run on two fp16 pieces of a per-sample power-of-two multiple of the upstream gradient (exact scaling: no range
 * restriction); frozen chains that carry ray gradients, the coarse decoder and a trainable fine decoder on the fp32 MFMA; the
 * weight-gradient panels on two bf16 pieces with fp32 sums.
 * Changing the mode rebuilds the forward images of the loaded decoders and invalidates captured graphs.
 * The library reads no environment variables: this call and nsk_set_render_opts are the only behaviour switches. */
int nsk_set_matmul_mode(nsk_ctx* ctx, int mode);
/* The same choice for the BACKWARD's gradient chains (g_h -> W^T, fc^T products of every decoder of the stage): 2 (default) = two fp16 pieces
 * on a per-sample power-of-two multiple of the upstream gradient; 0 = the fp32 MFMA (full-width operands: what the reference's fp32 autograd
 * multiplies, src/Mapper.cpp:443-444) for the frozen AND the trainable roles -- a measuring stick for the gradient error and the step time of
 * full-width arithmetic (tests/test_gpu_configs.py, bench.py extras), 1.5-2x slower.  The trainable decoder's weight-gradient panels keep two
 * bf16 pieces (16 significant bits, fp32 sums over the samples) in both modes. */
int nsk_set_backward_mode(nsk_ctx* ctx, int mode);

/* Order in which the decoder kernels of a step walk the rays' samples (results differ only by the order of floating-point sums in the
 * gradients): -1 = automatic (DEFAULT: cell-sorted for steps that scatter into the grids without ray gradients and have >= 14336 samples -- about
 * 300 rays x 48, the measured crossover on the reference's grids: below it the two sort launches cost more than the scatter saves -- or at
 * least four samples per cell of the finest level read, where ray order serialises the atomics of the many samples that share a cell),
 * 0 = ray order always, 1 = cell-sorted always.  Cell-sorted: k_sample also bins every sample by the grid cell it falls in and two small
 * launches build the permutation; tiles of 16 samples then share cells and the backward issues one atomic flush per cell run. */
int nsk_set_sort_mode(nsk_ctx* ctx, int mode);
/* Debug and experiment switches (never needed for correct results):
 *   "deterministic" 1: bit-reproducible gradients, to tell a real defect from the order sensitivity of floating-point atomics: ray order
 *                      (no cell sort), one backward launch per decoder in a fixed order, ONE workgroup each whose waves add their tiles'
 *                      contributions strictly one after the other (orders of magnitude slower; the trainable decoder's pose gradients are
 *                      not covered);
 *   "roctx" 1:         roctxRangePush/Pop around every launch group (names as in nsk_profile_end) for rocprofv3 --marker-trace;
 *   "frozen_cost" n:   relative cost of a frozen decoder's tile in the backward's workgroup split (0 = built-in value);
 *                      this and the other cost keys of the splits ("frozen_cost_rays", "fwd_fine_cost", "fwd_occ_cost", "fwd_color_cost")
 *                      take 0 .. 1 000 000, anything else is refused;
 *   "no_fused_median" 1: nsk_track_step computes the Tracker's median threshold in a launch of its own (composite, median, composite)
 *                      even where a fused form applies;
 *   "no_deferred_median" 1: with ray gradients and frozen decoders the threshold is found inside the compositing launch behind a grid
 *                      barrier (round 3's form) instead of by the backward launch's workgroups;
 *   "no_piggyback" 1:  a batch registered with nsk_map_prepare is sampled by launches of its own at the start of its step;
 *   "no_occ_role" 1 | 2: the forward's middle and fine decoders never | always as one workgroup role (default: where the split predicts
 *                      the shorter launch; same results either way);
 *   "no_dead_skip" 1:  the backward's frozen roles run every tile even where an optimiser mask discards all it scatters (see nsk_set_mask);
 *   "dead_tile_pct" p: what a skipped tile counts for in the backward's workgroup split, in percent of a tile that runs (default 12);
 *   "static_deal" 1:   every role of the backward takes its tiles round-robin, as before the queues.  By default, in a mapping launch with a
 *                      trainable decoder, a frozen role that skips dead tiles and whose waves have "deal_min_rounds" rounds of tiles or more
 *                      deals only the first part of its tiles that way and claims the rest, a few consecutive tiles at a time, from a cursor
 *                      in device memory, so that waves whose tiles were mostly dead take more (k_decode_bwd_multi_deal; same gradients up to
 *                      the order of the atomic adds).  The deterministic mode, launches with ray gradients, the launches without a trainable
 *                      decoder (their 16-wave kernel) and the trainable role always deal statically;
 *   "deal_head_pct" p: share of such a role's rounds that stay dealt statically (0 .. 100, default 75);
 *   "deal_chunk" n:    consecutive tiles per claim of the rest (1 .. 16, default 2);
 *   "deal_min_rounds" n: a role with fewer rounds of tiles per wave deals statically (default 24; 0: every skipping role claims: tests). */
int nsk_set_tuning(nsk_ctx* ctx, const char* key, int value);

/* Scene bound [[x0,x1],[y0,y1],[z0,z1]]; the reference hard-codes it in five places
 * (src/main.cpp:33, src/Renderer.cpp:15, src/Mapper.cpp:29, src/Tracker.cpp:23, src/models/MLP.cpp:53-56). */
int nsk_set_bound(nsk_ctx* ctx, const float h_bound[6]);

/* Renderer::Renderer() constants (src/Renderer.cpp:5-15): N_samples 32, N_surface 16, lindisp false, perturb 0,
 * occupancy: 0 = the density branch the reference executes (src/Renderer.cpp:125 passes false, utils.h:155-157),
 * 1 = alpha = sigmoid(10 sigma).  n_samples + n_surface <= 64. */
int nsk_set_render_opts(nsk_ctx* ctx, int n_samples, int n_surface, int lindisp, float perturb, int occupancy,
                        uint64_t seed);

/* ---- hierarchical importance sampling: rendering.N_importance (upstream NICE-SLAM's sample_pdf) ----------
 * n_importance > 0 makes every renderer of the context (nsk_render_forward, nsk_render_backward, nsk_map_step, nsk_track_step,
 * nsk_render_image, nsk_mesh_vertex_colors) run two passes: a first pass over the stratified and surface samples, then n_importance extra
 * depths drawn from the compositing weights of that pass, then a second pass over the merged set, which is what the call returns: its
 * samples per ray are S2 = n_samples (+ n_surface with a depth) + n_importance, d_weights is [N][S2].  Default 0: one pass, as before.
 *
 * The rule (upstream's sample_pdf, fixed operation by operation).  The first pass has S1 = n_samples (+ n_surface with a depth) sorted
 * depths z[0..S1) and compositing weights w[0..S1), the weights nsk_render_forward returns.  With Ni = n_importance > 0, per ray, every
 * operation is an fp32 operation of its own (rounded add, multiply, subtract, divide; no contraction):
 *    1. bins[k] = 0.5 * (z[k+1] + z[k]), k = 0..S1-2 (S1-1 bins).
 *    2. q[k] = w[k+1] + 1e-5f, k = 0..S1-3 (the interior weights w[1..S1-1)).
 *    3. total = the sum of q taken left to right.
 *    4. pdf[k] = q[k] / total.
 *    5. cdf[0] = 0, cdf[k+1] = cdf[k] + pdf[k], left to right (S1-1 entries).
 *    6. u[j], j = 0..Ni-1: with perturb == 0 (deterministic) u[j] is the t of at::linspace(0, 1, Ni) at j, the helper the first-pass
 *       samples use (step = 1 / (Ni-1); j < Ni/2: step * j, else 1 - step * (Ni-1-j); Ni = 1: 0).  Otherwise
 *       u[j] = (hash(seed, ray, 64 + j) >> 8) * 2^-24, the counter hash of the perturbation; the offset 64 keeps the stream apart from
 *       the perturbation's lanes.
 *    7. inds = the number of cdf entries <= u[j] (searchsorted, right = true; a NaN compares false).
 *    8. below = max(inds - 1, 0), above = min(inds, S1 - 2).
 *    9. denom = cdf[above] - cdf[below]; if denom < 1e-5f then denom = 1.
 *   10. t = (u[j] - cdf[below]) / denom.
 *   11. zs[j] = bins[below] + t * (bins[above] - bins[below]).
 *   12. The second pass's depths are the S2 = S1 + Ni values of [z, zs], rank-sorted by the sampling's rule: ascending; ties by position
 *       in the concatenation; a NaN ranks as +inf.  Then come points, decoders and compositing, exactly as for any z.
 * zs is a constant to the backward (upstream detaches it): gradients flow through the second pass only, and the first pass saves nothing
 * for a backward.  A ray whose first-pass weights are not finite gets NaN extra depths and renders non-finite; no other ray sees it.
 *
 * Needs n_samples >= 3 and n_samples + n_surface + n_importance <= 64 (one wave per ray); refused otherwise, and when negative;
 * nsk_set_render_opts makes the same check against the installed value.  Setting another value invalidates captured graphs, as the matmul
 * mode does; a step with n_importance > 0 is captured like any other.  With n_importance > 0 nsk_map_prepare registers nothing and returns
 * success (no launch of the running step can carry a resampling): the batch's own step samples it.  nsk_last_call_stats counts both passes.
 * Not done: gradients through zs, a separate coarse network for the first pass (upstream has none either), more than 64 samples per ray. */
int nsk_set_importance(nsk_ctx* ctx, int n_importance);

/* The installed n_importance (-1: null ctx).  A caller that changes the sample counts and n_importance together reads it to order its two
 * calls so that each check passes: towards a smaller n_importance that one first, towards a larger one nsk_set_render_opts first. */
int nsk_get_importance(nsk_ctx* ctx);

/* Steps 1 - 12 above on their own, beside nsk_raw2outputs: d_z [N][S] sorted depths, d_weights [N][S] -> d_z_out [N][S + n_importance].
 * det != 0: the deterministic u of step 6, else the hash of (seed, ray index, 64 + j).  S >= 3, n_importance >= 1, S + n_importance <= 64. */
int nsk_importance_resample(nsk_ctx* ctx, int N, int S, const float* d_z, const float* d_weights, int n_importance, int det, uint64_t seed,
                            float* d_z_out);

/* ---- feature grids: c10::Dict<string,Tensor> "grid_<level>" [1,C,Z,Y,X] fp32 (src/main.cpp:33-78) ------ */
/* h_czyx is the reference layout [C][Z][Y][X] (C must be 32); the device copy is voxel-major [Z][Y][X][C]
 * so that the 32 channels of a voxel are one 128-byte line (conversion happens here).
 * A dimension of 1 is valid: grid_sample's align_corners scaling multiplies the normalised coordinate by dim - 1 = 0, so every point reads
 * voxel 0 along that axis with weight 1 and the lookup has no spatial gradient there (what ATen does; tests/test_local_parity_cpu.py). */
int nsk_grid_upload(nsk_ctx* ctx, int level, const float* h_czyx, int C, int Z, int Y, int X);
int nsk_grid_download(nsk_ctx* ctx, int level, float* h_czyx);
int nsk_grid_grad_download(nsk_ctx* ctx, int level, float* h_czyx);
/* frustum feature selection (src/Mapper.cpp:254-290,333-350): h_mask_zyx[Z*Y*X] != 0 marks voxels that are
 * optimiser parameters; NULL = all voxels.  Gradients of unmarked voxels are discarded: nsk_grid_grad_download returns zeros for them,
 * nsk_adam_step and nsk_grad_pack never read them, and in the raw slab (nsk_grad_slab) their entries are UNSPECIFIED -- whatever partial
 * sums the scatter left there.  A frozen decoder's backward (no NSK_GRAD_RAYS) does not even run a 16-sample tile none of whose samples
 * touches a marked voxel of its level, so those entries differ from build to build and with nsk_set_tuning("no_dead_skip", 1). */
int nsk_set_mask(nsk_ctx* ctx, int level, const uint8_t* h_mask_zyx);

/* Mapper::get_mask_from_c2w (src/Mapper.cpp:42-130, intended semantics): builds the frustum mask of `level` on the device from
 * a depth image (d_depth [H][W], device) and the current pose h_c2w (16 floats, row-major [4][4]) and installs it like
 * nsk_set_mask; h_mask_out [Z*Y*X] (host, may be NULL) receives a copy.  A voxel is kept if its centre projects inside the image
 * with 0 <= depth_along_-z <= sampled_depth + 0.5 (zero depths count as the maximum sampled depth) or lies within 0.5 m of the
 * camera centre; grid_coarse keeps every voxel.  Unmarked voxels' gradients: as for nsk_set_mask.
 * The maximum sampled depth has the floor 0: it is max(0, max over the voxels of the sampled depth).  A zero depth means "no reading",
 * so an image without a positive sample (all zeros, or all negative) has the maximum 0 and a negative sample never becomes it.  Every
 * call takes the maximum of its own image; nothing is carried from one call to the next (tests/test_gpu_keyframe.py). */
int nsk_frustum_mask(nsk_ctx* ctx, int level, const float* d_depth, int H, int W, float fx, float fy, float cx, float cy,
                     const float h_c2w[16], uint8_t* h_mask_out);

/* Mapper::keyframe_selection_overlap (src/Mapper.cpp:132-196; include/torchlib/utils.h:58-130): the rays of N pixels of the
 * current frame (device arrays, e.g. from nsk_rays_from_pixels) are sampled at n_samples depths in [0.8 depth, depth + 0.5] and
 * projected into each of K keyframes (h_c2w: K row-major 4x4 poses, host); h_percent[k] = fraction of the points inside keyframe
 * k's image (20-pixel edge, in front of the camera).  Ranking and truncation to the window stay with the caller (Mapper). */
int nsk_keyframe_overlap(nsk_ctx* ctx, int N, const float* d_rays_o, const float* d_rays_d, const float* d_gt_depth, int n_samples,
                         int H, int W, float fx, float fy, float cx, float cy, int K, const float* h_c2w, float* h_percent);

/* ---- decoders (src/models/MLP.cpp:3-49,104-138; src/models/GaussianFFT.cpp:3-8) -------------------------- */
/* packed parameter order (row-major [out,in] as torch::nn::Linear):
 *   middle/fine/color: B[3][93], pts_linear[0..4].{weight,bias}, fc[0..4].{weight,bias}, output_linear.{weight,bias}
 *   coarse:            pts_linear[0..4].{weight,bias}, output_linear.{weight,bias}
 * counts: coarse 6337, middle 15800, fine 20920, color 15899. */
size_t nsk_decoder_param_count(int which);
int nsk_decoder_upload(nsk_ctx* ctx, int which, const float* h_packed, size_t n);
int nsk_decoder_download(nsk_ctx* ctx, int which, float* h_packed, size_t n);
int nsk_decoder_grad_download(nsk_ctx* ctx, int which, float* h_packed, size_t n);
/* which decoders receive gradients / Adam updates (src/Mapper.cpp:292-301: fine if !fix_fine, color if !fix_color).  Set it
 * before the forward of the step: the forward of a trainable decoder stores its block outputs for the backward (the entry points
 * that contain both -- nsk_map_step, nsk_track_step, nsk_render_backward -- always do); a backward that finds them stale fails. */
int nsk_decoder_set_trainable(nsk_ctx* ctx, int which, int trainable);

/* ---- rendering ------------------------------------------------------------------------------------------ */
/* Renderer::render_batch_ray (src/Renderer.cpp:44-126) = z sampling + Renderer::eval_points (:19-42) +
 * NICE::forward (src/models/NICE.cpp:16-52) + raw2outputs_nerf_color (include/torchlib/utils.h:148-172).
 *   d_rays_o, d_rays_d [N][3]; d_gt_depth [N] or NULL (then N_surface = 0, :54-57);
 *   gt_depth_max: max over the WHOLE batch of gt_depth (:76,:93).  Pass < 0 to have it computed on the device
 *   from d_gt_depth; multi-GPU callers pass the global maximum so that sharding rays does not change results.
 *   outputs: d_rgb [N][3], d_depth [N], d_var [N], d_weights [N][S] or NULL (S = n_samples (+ n_surface)).
 * At the geometric edges (every entry point that samples rays; pinned per ray and per voxel by tests/test_gpu_edges.py):
 *   - a zero direction component is valid: (bound - o) / 0 = +-inf never wins the minimum over the axes;
 *   - an origin outside the bound is valid: samples outside are looked up at the clamped coordinate, get occupancy 100 (:36), send no
 *     gradient to the grids and none through the clipped coordinate (ATen's border padding); a ray that misses the bound has far < 0,
 *     clamped to 0 with ground truth (:76), a descending z without;
 *   - an origin ON a face with a zero direction component across it (a ray running inside the face) has 0/0 in the box exit.  ATen's max / min
 *     propagate the NaN: the reference renders every such ray non-finite.  Here (and in the CPU oracle) the comparisons `t0 > t1 ? t0 : t1`,
 *     `m < far` drop a NaN, except for the upper x face (o_x = bound x1, d_x = 0), whose NaN is taken as the first axis' value unconditionally:
 *     those rays come out non-finite (outputs and the gradients of the voxels they touch -- all addresses stay inside the grid; a NaN z sorts
 *     behind every number, as in torch.sort); every other in-face ray is rendered with the exit of the remaining axes.  Which in-face rays
 *     render is an accident of the comparison order, recorded here because the tests pin it, NOT a promise: callers drop such rays with
 *     nsk_inside_filter / nsk_set_ray_mask.  A ray the mask drops whose exit is NaN is sampled with far = 0 instead (nsk_map_step,
 *     nsk_track_step, nsk_render_backward): its outputs (d_rgb, d_depth, d_var) are then finite numbers without meaning, its loss and
 *     gradients exactly zero, and it cannot reach the sums of the rays that are kept (0 x NaN in a shared voxel row). */
int nsk_render_forward(nsk_ctx* ctx, int stage, int N, const float* d_rays_o, const float* d_rays_d,
                       const float* d_gt_depth, float gt_depth_max, float* d_rgb, float* d_depth, float* d_var,
                       float* d_weights);

/* Renderer::eval_points (src/Renderer.cpp:19-42): raw [M][4] = (rgb, occupancy) of M points, occupancy = 100
 * outside the bound. */
int nsk_eval_points(nsk_ctx* ctx, int stage, int M, const float* d_points, float* d_raw);

/* raw2outputs_nerf_color (include/torchlib/utils.h:148-172) on its own: d_raw [N][S][4] (rgb, sigma), d_z [N][S] sorted,
 * d_rays_d [N][3]; occupancy 0 = density branch (what src/Renderer.cpp:125 passes). */
int nsk_raw2outputs(nsk_ctx* ctx, int N, int S, const float* d_raw, const float* d_z, const float* d_rays_d, int occupancy,
                    float* d_rgb, float* d_depth, float* d_var, float* d_weights);

/* Backward of render_batch_ray given upstream gradients (what loss.backward() at src/Mapper.cpp:444 /
 * src/Tracker.cpp:84 is meant to do).  The forward is recomputed internally.
 *   d_g_rgb [N][3], d_g_depth [N], d_g_var [N] or NULL (depth_var detached).
 *   Gradients ACCUMULATE into the context-owned gradient slab (grids, trainable decoders) until nsk_adam_step
 *   or nsk_zero_grads; d_g_rays_o / d_g_rays_d [N][3] are overwritten (NSK_GRAD_RAYS). */
int nsk_render_backward(nsk_ctx* ctx, int stage, int N, const float* d_rays_o, const float* d_rays_d,
                        const float* d_gt_depth, float gt_depth_max, const float* d_g_rgb, const float* d_g_depth,
                        const float* d_g_var, unsigned flags, float* d_g_rays_o, float* d_g_rays_d);

/* One mapping iteration without the Adam step: render forward, Mapper loss (src/Mapper.cpp:435-442:
 * sum_{gt>0}|gt_d - d| + use_color * w_color * sum|gt_c - c|) and backward, fused so that the loss gradient
 * never leaves the GPU.  d_loss (device float, may be NULL) receives the loss; outputs d_rgb/d_depth/d_var may
 * be NULL. */
int nsk_map_step(nsk_ctx* ctx, int stage, int N, const float* d_rays_o, const float* d_rays_d,
                 const float* d_gt_depth, const float* d_gt_color, float gt_depth_max, float w_color, int use_color,
                 unsigned flags, float* d_loss, float* d_rgb, float* d_depth, float* d_var, float* d_g_rays_o,
                 float* d_g_rays_d);

/* One tracking iteration without the Adam step (src/Tracker.cpp:41-89): render, dynamic-outlier mask
 * |gt_d - d| < 10 median (:67-71), loss sum_mask |gt_d - d| / sqrt(var + 1e-10) + w_color sum_mask |gt_c - c|
 * (:75-82), backward onto the rays.  detach_var: treat depth_var as a constant.
 * With handle_dynamic and at most 1024 rays the median needs no launch of its own.  With NSK_GRAD_RAYS and no trainable decoder (the
 * Tracker as the reference runs it) the loss launch writes the residuals and every workgroup of the backward launch selects the
 * median and drops the rays that fail it; otherwise (and while the grid is at most one 4-ray workgroup per CU) the
 * median is found inside the loss launch: the residuals meet at a device-wide barrier whose wait is bounded; should it ever time
 * out, that step ran with an infinite threshold and the next nsk_sync returns the error. */
int nsk_track_step(nsk_ctx* ctx, int stage, int N, const float* d_rays_o, const float* d_rays_d,
                   const float* d_gt_depth, const float* d_gt_color, float gt_depth_max, float w_color, int use_color,
                   int handle_dynamic, int detach_var, unsigned flags, float* d_loss, float* d_g_rays_o,
                   float* d_g_rays_d);

/* Stand-alone losses with seed gradients (same formulas as above) for callers that drive
 * nsk_render_forward / nsk_render_backward themselves. */
int nsk_loss_map(nsk_ctx* ctx, int N, const float* d_depth, const float* d_rgb, const float* d_gt_depth,
                 const float* d_gt_color, float w_color, int use_color, float* d_g_depth, float* d_g_rgb,
                 float* d_loss);
int nsk_loss_track(nsk_ctx* ctx, int N, const float* d_depth, const float* d_rgb, const float* d_var,
                   const float* d_gt_depth, const float* d_gt_color, float w_color, int use_color, int handle_dynamic,
                   int detach_var, float* d_g_depth, float* d_g_rgb, float* d_g_var, float* d_loss);

/* ---- rays and pose (include/torchlib/utils.h:13-55,141-146,174-210; src/Mapper.cpp:416-427) ------------- */
/* raySampler's direction/origin part for given pixel indices (the reference draws them with torch::randint,
 * utils.h:32; streams cannot match, so indices are an input).  d_c2w: 12 floats, row-major [3][4].
 * mode bit0: as-written j_t=(i-cy)/fy without sign flip (D11); bit1: truncate intrinsics to int (D10);
 * 0 = intended OpenGL camera dirs=[(i-cx)/fx, -(j-cy)/fy, -1]. */
/* raySampler's pixel draw (utils.h:19-36: n indices, with replacement, uniform over the window [H0,H1) x [W0,W1)) and its
 * gather of the ground truth (utils.h:38-43) on the device.  The draw uses a counter-based hash of (seed, ray index) instead of
 * torch::randint's stream; pix_i = column, pix_j = row.  d_depth [H][W], d_color [H][W][3] (d_color / d_gt_color may be NULL). */
int nsk_sample_pixels(nsk_ctx* ctx, unsigned long long seed, int n, int H0, int H1, int W0, int W1, int32_t* d_pix_i, int32_t* d_pix_j);
int nsk_gather_pixels(nsk_ctx* ctx, int n, const int32_t* d_pix_i, const int32_t* d_pix_j, int H, int W, const float* d_depth,
                      const float* d_color, float* d_gt_depth, float* d_gt_color);
int nsk_rays_from_pixels(nsk_ctx* ctx, int n, const int32_t* d_pix_i, const int32_t* d_pix_j, float fx, float fy,
                         float cx, float cy, const float* d_c2w, int mode, float* d_rays_o, float* d_rays_d);
/* fused forms for a device-resident Tracker iteration (same arithmetic as the calls they replace, fewer launches):
 * nsk_rays_from_camera = nsk_camera_from_tensor + nsk_rays_from_pixels (d_c2w_out: optional 12 floats);
 * nsk_pose_step = nsk_rays_backward + nsk_camera_backward + nsk_adam_vector on the 7-vector (d_g_cam_out: optional 7 floats). */
int nsk_rays_from_camera(nsk_ctx* ctx, int n, const int32_t* d_pix_i, const int32_t* d_pix_j, float fx, float fy, float cx, float cy,
                         const float* d_cam, int mode, float* d_rays_o, float* d_rays_d, float* d_c2w_out);
int nsk_pose_step(nsk_ctx* ctx, int n, const int32_t* d_pix_i, const int32_t* d_pix_j, float fx, float fy, float cx, float cy, int mode,
                  const float* d_g_rays_o, const float* d_g_rays_d, float* d_cam, float* d_m, float* d_v, float lr, float b1, float b2,
                  float eps, int step, float* d_g_cam_out);
/* One launch for the whole ray preparation of an iteration (src/Mapper.cpp:376-427 for a window of frames, src/Tracker.cpp:44-58 for
 * one): for each of `nframes` frames, rays_per_frame times  nsk_sample_pixels (window [H0,H1) x [W0,W1), frame's own seed) ->
 * nsk_gather_pixels (frame's images, [H][W] / [H][W][3]) -> nsk_rays_from_pixels (pose = 12 floats c2w) or nsk_rays_from_camera
 * (pose_is_cam7: 7 floats quaternion + translation) -> nsk_inside_filter, with the arithmetic of those entry points (results are
 * bit-identical; tests/test_gpu_dist.py).  Outputs are [nframes * rays_per_frame] arrays, frame-major; d_keep may be NULL (no
 * filter), d_color / d_gt_color may be NULL.  The frame table is read on the host at call time (at most 64 frames per call).
 * The reference spends 3 kernels and ~15 small tensor ops per frame here; the device-resident Mapper iteration spent 16 launches. */
typedef struct nsk_frame_rays {
    const float* d_depth; const float* d_color;      /* the frame's images on the device */
    const float* d_pose;                             /* device: 12 floats (c2w rows) or 7 floats (pose vector) */
    int pose_is_cam7;
    unsigned long long seed;                         /* pixel-draw seed of this frame in this iteration */
} nsk_frame_rays;
int nsk_prepare_rays(nsk_ctx* ctx, int nframes, const nsk_frame_rays* h_frames, int rays_per_frame, int H0, int H1, int W0, int W1,
                     int H, int W, float fx, float fy, float cx, float cy, int mode, int32_t* d_pix_i, int32_t* d_pix_j,
                     float* d_gt_depth, float* d_gt_color, float* d_rays_o, float* d_rays_d, uint8_t* d_keep);
/* nsk_pose_step for every frame of a mapping window in ONE launch (bundle adjustment, src/Mapper.cpp:305-329,366-368,467-489): frame f owns
 * the rays [h_first[f], h_first[f] + h_count[f]) of the batch's pixel / ray-gradient arrays (a shard of the batch at N > 1: the part of
 * the frame's rays that falls into this rank's range, possibly none) and the pose d_cams[8 f .. 8 f + 6] with moments d_m / d_v in the same
 * layout; h_active[f] = 0 marks a frame whose pose is not optimised (the oldest frame of the window).
 *   step >= 1: gradient + Adam step of every active pose, the arithmetic of nsk_pose_step frame by frame (one GPU);
 *   step == 0: gradients only, d_g_cams[8 f + k] = d loss / d pose (zeros for inactive frames) -- the form for N > 1: register d_g_cams
 *              with nsk_grad_extra so that it is summed over the ranks with the grid gradients, then step all poses at once with
 *              nsk_adam_vector(8 * nframes, d_cams, d_g_cams, ...) (a zero gradient leaves a pose and its moments untouched).
 * d_g_cams may be NULL for step >= 1; when given it has room for 8 * nframes + 8 floats and d_g_cams[8 nframes + 1] receives the number
 * of rays of d_keep[0 .. n_keep) that take part (d_keep NULL: n_keep), the count a sharded step's ranks must add up to the batch's. */
int nsk_pose_step_multi(nsk_ctx* ctx, int nframes, const int* h_first, const int* h_count, const uint8_t* h_active, const int32_t* d_pix_i,
                        const int32_t* d_pix_j, float fx, float fy, float cx, float cy, int mode, const float* d_g_rays_o, const float* d_g_rays_d,
                        float* d_cams, float* d_m, float* d_v, float lr, float beta1, float beta2, float eps, int step, float* d_g_cams,
                        const uint8_t* d_keep, int n_keep);
/* d loss / d c2w (12 floats, overwritten) from per-ray gradients */
int nsk_rays_backward(nsk_ctx* ctx, int n, const int32_t* d_pix_i, const int32_t* d_pix_j, float fx, float fy,
                      float cx, float cy, int mode, const float* d_g_rays_o, const float* d_g_rays_d, float* d_g_c2w);
/* get_camera_from_tensor / quad2rotation (utils.h:174-210): cam = (qw,qx,qy,qz,tx,ty,tz) -> c2w [3][4] */
int nsk_camera_from_tensor(nsk_ctx* ctx, const float* d_cam, float* d_c2w);
int nsk_camera_backward(nsk_ctx* ctx, const float* d_cam, const float* d_g_c2w, float* d_g_cam);
/* inside-bbox pre-filter (src/Mapper.cpp:416-427, src/Tracker.cpp:48-58): d_keep[n] = (t >= gt_depth), t = min over the axes of max over
 * the two sides of (bound - o) / d, every operation a correctly rounded fp32 one.  NaN rule: as torch.max / torch.min hand a NaN on, a NaN
 * in ANY of the six quotients (0/0: an origin on a bound plane with a zero direction component along that axis) drops the ray, whichever
 * plane and axis it is; so does a NaN gt_depth.  Bit for bit the ATen expression on the CPU (tests/test_keyframe_cpu.py,
 * tests/test_gpu_keyframe.py); the filter inside nsk_prepare_rays is the same function.  The box exit of the sampling kernels (the in-face
 * note at nsk_render_forward) is a different text and unchanged: a ray this filter drops never reaches them with a meaning. */
int nsk_inside_filter(nsk_ctx* ctx, int N, const float* d_rays_o, const float* d_rays_d, const float* d_gt_depth,
                      uint8_t* d_keep);
/* Registers the NEXT batch, so that its sampling and cell sort leave the front of its own step: call it BEFORE the nsk_map_step of the current
 * batch, with the arguments the next nsk_map_step will get (same device pointers, same gt_depth_max, same flags, the next batch's ray mask
 * installed while you call it, the same render options and seed).  Nothing is launched by this call.  The nsk_map_step that follows carries
 * the registered batch's sampling in its composite launch, its backward launch carries the offsets of the cell sort and the nsk_adam_step
 * after it the placement; the next nsk_map_step finds its samples ready and starts with the forward.  Whatever has not been carried by then
 * (the call came after the step, another call needed the cell histogram in between, gt_depth_max < 0 with more than 8192 rays, a graph
 * capture) is launched at that point, as for an unprepared batch; a registered batch that is never asked for is dropped.  The rays and
 * the ground truth must stay valid and unchanged until their step has run, and must not depend on the running step's result (bundle
 * adjustment moves poses: do not prepare then).  The same holds for the ray mask: what is remembered is the BUFFER installed with
 * nsk_set_ray_mask at the time of this call, and its contents are read later -- when the batch's sampling runs inside the current step's
 * composite launch, or at the batch's own step -- so the next batch's mask must live in a different buffer from the current step's mask and
 * stay unchanged until the batch's step has run (two mask buffers used alternately, as Mapper::optimize_map does).
 * Results are those of the unprepared step.  Everything runs on the context's stream.
 * With hipGraphs: nsk_graph_begin first runs whatever of a prepared batch's sampling / sort is still pending (a capture never records it),
 * nsk_graph_launch does the same and drops a prepared batch that lives in the buffer set the graph writes (its own step samples it again). */
int nsk_map_prepare(nsk_ctx* ctx, int stage, int N, const float* d_rays_o, const float* d_rays_d, const float* d_gt_depth, float gt_depth_max,
                    unsigned flags);

/* The reference drops the rays that fail the test above before it renders them (boolean-index compaction, src/Mapper.cpp:423-427,
 * src/Tracker.cpp:55-58), which needs their count on the host.  Here they stay in place and are neutralised instead: with a mask
 * installed (d_keep [N] as written by nsk_inside_filter, device memory, must stay valid; NULL = none), nsk_map_step, nsk_track_step and
 * nsk_render_backward leave the rays with d_keep == 0 out of max(gt_depth), the Tracker's median, the loss and every gradient --
 * the same sums the reference forms over the compacted batch, with no device-to-host round trip. */
int nsk_set_ray_mask(nsk_ctx* ctx, const uint8_t* d_keep);
/* A rank that renders a SHARD of a batch (rays shard over the GPUs of a node) still needs the batch-global max(gt_depth)
 * (src/Renderer.cpp:76,93).  Every rank can hold the whole batch's ground-truth depths and keep bytes (they come from the same pixel draw:
 * nsk_prepare_rays of the full window is one small launch), so no collective is needed: with a depth-max batch installed
 * (d_gt_depth[n], d_keep[n] or NULL; n = 0 removes it) every step that is given gt_depth_max < 0 takes the maximum over THAT array
 * instead of over its own rays (inside the sampling launch, every wave for itself, while that batch has at most 8192 rays; one extra
 * single-block launch in front of the sampling beyond that).  nsk_map_prepare remembers the batch installed at registration, like the ray mask. */
int nsk_set_depth_max_batch(nsk_ctx* ctx, const float* d_gt_depth, const uint8_t* d_keep, int n);
/* plain Adam on a caller-owned vector (camera 7-vectors: src/Tracker.cpp:103, src/Mapper.cpp:305-329) */
int nsk_adam_vector(nsk_ctx* ctx, int n, float* d_p, const float* d_g, float* d_m, float* d_v, float lr, float beta1,
                    float beta2, float eps, int step);

/* ---- optimiser (torch::optim::Adam, src/Mapper.cpp:330,360-368,445-446) ---------------------------------- */
/* lr[g] for NSK_GROUP_*; groups whose gradients were produced since the last step are updated (an lr of 0
 * still advances their moments, as torch does); gradients are zeroed afterwards (optimizer.zero_grad(), :446).
 * Only masked voxels move (nsk_set_mask).  nsk_adam_reset drops the moments and step counts (the reference
 * re-creates the optimiser on every optimize_map call, :330). */
int nsk_adam_step(nsk_ctx* ctx, const float lr[NSK_NUM_GROUPS], float beta1, float beta2, float eps);
int nsk_adam_reset(nsk_ctx* ctx);

/* ---- hipGraph capture of a step ------------------------------------------------------------------------------
 * The kernels of the nsk_* calls made between nsk_graph_begin and nsk_graph_end (e.g. nsk_map_step + nsk_adam_step with fixed
 * device buffers, sizes, learning rates and a device-computed or fixed gt_depth_max) are recorded instead of run, and
 * nsk_graph_launch replays them with one launch on the context's stream; Adam's step counts advance per replay (the recorded
 * Adam node is patched with the new bias-correction constants).  Run the step once eagerly first (workspaces are sized then);
 * at most one nsk_adam_step per graph; calls that synchronise (uploads, downloads, nsk_grad_slab) are not capturable.
 * A recorded step holds buffer addresses and the optimiser masks' voxel lists as kernel arguments: after a reallocation (larger
 * batch, new grid shape) or ANY nsk_set_mask / nsk_frustum_mask call (new mask contents included) every graph is stale --
 * nsk_graph_launch then fails with a message instead of replaying; run the step eagerly once and capture again. */
int nsk_graph_begin(nsk_ctx* ctx);
int nsk_graph_end(nsk_ctx* ctx, int* graph_id);
int nsk_graph_launch(nsk_ctx* ctx, int graph_id);
int nsk_graph_destroy(nsk_ctx* ctx, int graph_id);
int nsk_zero_grads(nsk_ctx* ctx);

/* ---- multi-GPU ------------------------------------------------------------------------------------------- */
/* The gradient slab (all grid gradients, all decoder gradients, one loss scalar) is one contiguous device
 * buffer so that a mapping step needs exactly one all-reduce.  The decoder gradients of a step
 * are summed into the slab lazily (inside nsk_adam_step when nobody looks earlier): nsk_grad_slab, nsk_allreduce_grads and
 * nsk_decoder_grad_download complete that sum first, so call nsk_grad_slab after nsk_map_step, every step, before reading
 * or exchanging the slab yourself.  Entries of voxels an optimiser mask leaves unmarked are unspecified (nsk_set_mask). */
int nsk_grad_slab(nsk_ctx* ctx, float** d_ptr, size_t* n_floats);
/* The exchange in compact form.  Every rank holds the same optimiser masks (nsk_set_mask / nsk_frustum_mask), and Adam discards the
 * gradient of an unmarked voxel, so only marked voxels need to travel: nsk_grad_pack gathers, into one contiguous buffer, the marked
 * voxels of the grid levels that received gradients since the last optimiser step (whole levels where no mask is installed), the
 * gradients of the trainable decoders and the 4 loss floats; after the caller's all-reduce (sum) over that buffer nsk_grad_unpack
 * writes the sums back into the slab for nsk_adam_step.  Levels the stage did not touch are not sent at all.  The marked-voxel lists
 * are rebuilt only when a mask changes (ascending voxel order, identical on every rank). */
int nsk_grad_pack(nsk_ctx* ctx, float** d_ptr, size_t* n_floats);
int nsk_grad_unpack(nsk_ctx* ctx);
/* A caller-owned device vector that travels with the exchange: nsk_grad_pack appends its n_floats (a multiple of 4, 16-byte aligned) behind
 * the loss floats, nsk_grad_unpack writes the sums back into it.  The C++ Mapper registers [8 floats per window frame: the bundle-adjustment
 * pose gradients of nsk_pose_step_multi(step = 0) | loss | kept-ray count | 6 spare] so that a sharded BA iteration still needs exactly
 * one all-reduce (SURVEY.md 8e lists the 7 (window - 1) pose floats as part of the slab).  n_floats = 0 removes it. */
int nsk_grad_extra(nsk_ctx* ctx, float* d_buf, size_t n_floats);
/* nsk_grad_pack + ncclAllReduce(sum, fp32) on the context's stream + nsk_grad_unpack; comm is an ncclComm_t (RCCL). */
int nsk_allreduce_grads(nsk_ctx* ctx, void* nccl_comm);

/* ---- scene mesh (config/nice_slam.yaml `meshing:` level_set, resolution; the reference ships no mesher) ---------------- */
/* Occupancy (channel 3 of nsk_eval_points' raw, with its "100 outside the bound" rule, src/Renderer.cpp:26-36) at the nodes of a
 * lattice: node (i, j, k) is the point origin_a + i_a * step_a per axis -- the product rounded, then the sum rounded, no FMA, so that
 * float32 numpy `origin + arange(n).astype(float32) * step` gives the same bits -- and its value goes to d_volume[(k * ny + j) * nx + i]
 * (x fastest, device memory, nx * ny * nz floats).  Stages 0..2; stage 3 gives the fine stage's occupancy.  Any node count: the lattice
 * is walked in slabs of max(2^21, the current workspace's samples) nodes (nsk_set_tuning "lattice_slab" n sets the slab to n nodes,
 * 0 = automatic), each slab below the 2^26 samples of a launch: a small kernel writes the slab's points (12 B / node), the decoders'
 * forward launches of nsk_eval_points run on them, a finish kernel writes the scalars.  Values equal nsk_eval_points' bit for bit. */
int nsk_eval_lattice(nsk_ctx* ctx, int stage, const float h_origin[3], const float h_step[3], int nx, int ny, int nz, float* d_volume);
/* The same at the nodes a validity mask keeps (d_valid: one byte per node on the device, laid out as d_volume; any non-zero byte counts as
 * set, as in nsk_lattice_seen and nsk_mesh_extract).  A set node receives exactly the bits nsk_eval_lattice writes there (the "100 outside
 * the bound" rule included; stage 3 gives the fine stage's occupancy); every other node receives the bits of `fill`, whatever they are
 * (NaN payloads, -0.0).  Every node of d_volume is written.  nsk_mesh_extract with the same d_valid never uses the volume at an unset node
 * (a cell is processed only when its eight corners are valid), so its mesh is the same bytes as from the dense volume, at the decoding
 * cost of the set nodes alone.  The set nodes are counted per 256-node workgroup, the counts scanned (the multi-launch scan of
 * nsk_mesh_extract: no atomics) and ranked into an ascending list of 32-bit node indices (4 B per set node; the unset nodes are filled in
 * that pass); the slabs of nsk_eval_lattice (same size rule and "lattice_slab" key, applied to the list) then run over the list: a
 * points kernel reads idx[m], the decoders' forward launches run, a finish kernel scatters to d_volume[idx[m]].  The count comes to the
 * host between the two passes: the call's one synchronisation.  With no set node no decoder is launched.  n_evaluated (may be NULL)
 * receives the number of set nodes.  At most 2^28 nodes per call (32-bit counts).  Not while a graph is being captured. */
int nsk_eval_lattice_masked(nsk_ctx* ctx, int stage, const float h_origin[3], const float h_step[3], int nx, int ny, int nz,
                            const uint8_t* d_valid, float fill, float* d_volume, long long* n_evaluated);

/* Marching cubes on the device over a volume laid out as above (at least 2 nodes per axis, at most 2^28 nodes; steps > 0).
 *   - a node is INSIDE when value > level (occupancy grows into the solid);
 *   - a cell is processed when its 8 corners are finite and (d_valid given: one byte per node, device) valid; other cells emit nothing;
 *   - indexed, welded mesh: every lattice edge belongs to its lower node (three per node: +x, +y, +z).  An edge of a processed cell whose
 *     ends lie on different sides owns exactly one vertex at p0 + t (p1 - p0), t = (level - v0) / (v1 - v0), p0 / p1 the end nodes' points
 *     formed as above and every operation rounded on its own (fp32, no FMA);
 *   - deterministic: vertex index = rank of (node index * 3 + axis) among those edges; triangles ordered by cell index, then by the order
 *     of nsk_mesh_table; compaction by prefix sums (multi-launch scans: no atomic append, no workgroup waits on another), so two runs give
 *     the same bytes;
 *   - triangles are wound so that their normal (v1 - v0) x (v2 - v0) points from the inside to the outside (towards free space).
 * Synchronises: the counts go to the host.  The mesh stays in context-owned device buffers until the next extract: nsk_mesh_buffers gives
 * them ([n_vertices][3] floats, [n_triangles][3] int32; NULL when empty), nsk_mesh_download copies them to the host (either may be NULL).
 * Device memory besides the caller's volume: 13 B per node (edge map 12, cell case 1) + 8 B per 256 nodes of scan scratch (+ its upper
 * levels, 1/256 of that each) + 12 B per vertex + 12 B per triangle.  An allocation that fails returns an error that names the byte
 * count; the context stays usable. */
int nsk_mesh_extract(nsk_ctx* ctx, const float* d_volume, const uint8_t* d_valid, int nx, int ny, int nz, const float h_origin[3],
                     const float h_step[3], float level, int* n_vertices, int* n_triangles);
int nsk_mesh_buffers(nsk_ctx* ctx, float** d_vertices, int32_t** d_triangles);
int nsk_mesh_download(nsk_ctx* ctx, float* h_vertices, int32_t* h_triangles);
/* The triangle list of one of the 256 corner-sign cases; needs no device.  Returns the number of triangles (at most 5; < 0 on error) and
 * writes three edge numbers per triangle to h_edges (may be NULL to ask for the count; capacity in entries).
 *   corner c of a cell has the offsets (x, y, z) = (c & 1, (c >> 1) & 1, c >> 2); bit c of case_index is set when corner c is inside;
 *   edge e = 4 * axis + idx runs along axis (0 x, 1 y, 2 z) from the corner whose other two offsets, in axis order, are (idx & 1, idx >> 1):
 *   edges 0..3 along x from (0, y, z), idx = y + 2 z; 4..7 along y from (x, 0, z), idx = x + 2 z; 8..11 along z from (x, y, 0), idx = x + 2 y.
 * The table is derived when first used: the segments a case leaves on a cube face depend on that face's four corner signs alone (two
 * inside corners on a face's diagonal are always cut off one by one), which makes neighbouring cells agree on every shared face. */
int nsk_mesh_table(int case_index, int8_t* h_edges, int capacity);

/* The nodes of a lattice (origin, step, nx, ny, nz and the node points as in nsk_eval_lattice; at most 2^28 nodes) that at least one of K
 * keyframes saw: d_valid[(k * ny + j) * nx + i] = 1, else 0 -- the d_valid of nsk_mesh_extract.  accumulate != 0 ORs the old byte in, so a
 * long keyframe list can be streamed through in batches of a few depth images; K = 0 with accumulate = 0 clears the mask.  This is a union
 * of depth-truncated view frusta, per node: tighter than the convex hull of a TSDF fusion that upstream's get_mesh takes, which
 * nsk_points_hull / nsk_lattice_in_hull give.
 * d_depth [K][H][W] floats on the device; h_w2c [K][16] row-major world-to-camera on the host (the caller inverts its c2w, so that rounding
 * is the caller's); the camera looks along -z, as in nsk_frustum_mask and nsk_rays_from_camera.  Keyframe k sees the node p when, every
 * operation an fp32 operation of its own (no FMA):
 *   c_a = ((w[4a] p0 + w[4a+1] p1) + w[4a+2] p2) + w[4a+3], a = 0..2;   d = -c_2 > 0;
 *   u = cx + (fx c_0) / d,  v = cy - (fy c_1) / d;   i = floor(u + 0.5), j = floor(v + 0.5)   (the nearest pixel);
 *   edge <= i < W - edge and edge <= j < H - edge, decided on the floats (a NaN fails; an edge that leaves no pixel is valid: nothing is seen);
 *   D = d_depth[k][j][i] is finite and > 0 (a pixel without a measurement sees nothing);   d <= D + trunc.
 * One thread per node loops over the keyframes (matrices and intrinsics ride in the kernel arguments, 32 keyframes per launch, longer
 * lists in several launches); a wave leaves the loop once all its nodes are seen.  n_seen (may be NULL) receives the number of set bytes
 * after the call: asking for it is the call's only synchronisation.  Not while a graph is being captured. */
int nsk_lattice_seen(nsk_ctx* ctx, const float h_origin[3], const float h_step[3], int nx, int ny, int nz, int K, const float* d_depth,
                     int H, int W, float fx, float fy, float cx, float cy, const float* h_w2c, int edge, float trunc, int accumulate,
                     uint8_t* d_valid, long long* n_seen);

/* Connected components of the mesh of the last nsk_mesh_extract, filtered in place (an error when there is none; an empty mesh is none:
 * n_components = 0).
 *   - vertices joined by a triangle are connected (the mesh is welded: shared vertex index).  Union-find on the device: roots are hooked
 *     below smaller indices by compare-and-swap, paths are halved, a flatten pass ends it, so a component's label is its smallest vertex
 *     index whatever order the atomics ran in;
 *   - triangle area 0.5 |(v1 - v0) x (v2 - v0)| in fp32, summed per component in fp64 (atomic adds: order-dependent in the last bits only);
 *   - largest_only = 0: components with area > min_area stay (upstream's remove_small_geometry_threshold, in the units the caller passes);
 *     largest_only != 0: the component with the largest area stays, ties to the smaller label (get_largest_components); min_area is not read;
 *   - compaction by the multi-launch scans of nsk_mesh_extract: kept vertices and triangles keep their relative order, triangles are
 *     re-indexed, vertices without a triangle are dropped; two runs give the same bytes.
 * Afterwards nsk_mesh_buffers / nsk_mesh_download describe the filtered mesh (NULL and 0 when nothing stays).  n_components counts the
 * components before the filter, n_kept those that stay.  Synchronises once.  Device memory: 14 B per vertex of scratch, 4 B per vertex and
 * per triangle of scan scratch, and a second vertex and triangle buffer (12 B each) the result is compacted into; an allocation that
 * fails names its byte count and leaves context and mesh as they were. */
int nsk_mesh_filter(nsk_ctx* ctx, float min_area, int largest_only, int* n_vertices, int* n_triangles, int* n_components, int* n_kept);

/* ---- whole frames: render a view of the map, compare it with the input frame (upstream Renderer.render_img and the visualiser) ---- */
/* A VIEW is the pixel set i = W0 + stride * col, j = H0 + stride * row of an H x W image, col < Wv = ceil((W1 - W0) / stride),
 * row < Hv = ceil((H1 - H0) / stride); the window [H0,H1) x [W0,W1) lies inside the image and stride >= 1 (at most 2^30 view pixels).
 * View pixel n = row * Wv + col (row-major: upstream's get_rays(...).reshape(-1, 3) order); pix_i is the column and pix_j the row, as
 * everywhere else here.  The pose is on the device: 12 floats c2w, or with pose_is_cam7 the 7-vector (as in nsk_frame_rays).
 *
 * nsk_image_rays: the rays (d_rays_o, d_rays_d [n][3]) and the ground-truth depth (d_gt_depth [n], read from d_depth_img [H][W]; both NULL
 * or both given) of view pixels [first, first + n), in one launch and without pixel-index arrays.  The arithmetic is that of
 * nsk_rays_from_pixels (c2w) / nsk_rays_from_camera (7-vector) and nsk_gather_pixels on the explicit index lists: the results are
 * bit-identical.  mode as in nsk_rays_from_pixels.  The pose matrix is formed once per workgroup. */
int nsk_image_rays(nsk_ctx* ctx, int first, int n, int H0, int H1, int W0, int W1, int stride, int H, int W, float fx, float fy, float cx,
                   float cy, const float* d_pose, int pose_is_cam7, int mode, const float* d_depth_img, float* d_rays_o, float* d_rays_d,
                   float* d_gt_depth);
/* nsk_render_image: the view rendered into d_rgb [Hv][Wv][3], d_depth [Hv][Wv], d_var [Hv][Wv] (device).  The view is walked in chunks of
 * chunk_rays pixels (the last one ragged); per chunk one nsk_image_rays launch into context-owned buffers, then the launches of
 * nsk_render_forward on those rays, the compositing writing straight into the images at the chunk's offset.
 *   d_depth_img NULL: no ground truth (N_surface = 0, near = 0.01, as nsk_render_forward with d_gt_depth NULL); gt_depth_max is not read;
 *   gt_depth_max < 0: every chunk is a batch of its own with its own device-computed max(gt_depth) (src/Renderer.cpp:76,93) -- upstream's
 *       render_img.  The bytes are those of nsk_render_forward called on that chunk's rays, so THE FRAME DEPENDS ON chunk_rays, as it does
 *       upstream (far = 1.2 max(gt) of the chunk feeds the sample depths of every ray of the chunk, and of the rays without a measurement);
 *   gt_depth_max >= 0: that value for every chunk; the frame does not depend on the chunking.
 * chunk_rays * S (S = n_samples (+ n_surface)) must stay below the 2^26 samples of a launch; a larger value is rejected with the largest
 * allowed one.  Asynchronous on the context's stream, no host synchronisation (unless a buffer has to grow).  Not capturable: the call
 * grows the workspace to chunk_rays rays (a reallocation makes recorded graphs stale, as for any larger batch).
 * Other context state: a render shows every ray, so an installed ray mask (nsk_set_ray_mask) is ignored; so is a depth-max batch
 * (nsk_set_depth_max_batch): it describes another batch, an image chunk's maximum is its own.  A batch registered with nsk_map_prepare
 * stays registered: the next nsk_map_step gives the loss and the outputs it gives without the render in between, bit for bit (if the
 * render had to grow the workspace the batch is sampled at its own step, with the same results). */
int nsk_render_image(nsk_ctx* ctx, int stage, int H0, int H1, int W0, int W1, int stride, int H, int W, float fx, float fy, float cx,
                     float cy, const float* d_pose, int pose_is_cam7, int mode, const float* d_depth_img, float gt_depth_max,
                     int chunk_rays, float* d_rgb, float* d_depth, float* d_var);
/* nsk_image_metrics: residuals of a rendered frame (d_rgb [Hv][Wv][3], d_depth [Hv][Wv]) against the input frame (d_gt_depth, d_gt_color:
 * same shapes, either may be NULL) and their sums, on the device.
 *   d_res_depth [Hv][Wv] (or NULL) = gt > 0 ? |gt - d| : 0 (the visualiser's rule: no measurement, no residual);
 *   d_res_color [Hv][Wv][3] (or NULL) = |gt_c - c|.  A residual image needs its ground truth.
 * Each difference is one fp32 operation; it is widened to double (squared, for the colour) and summed in fp64.  A pixel whose rendered
 * depth or colour is not finite is left out of every sum and counted; so is a term that is not finite through the ground truth.
 *   h_out[0] pixels;  [1] pixels in the depth sum (gt > 0);  [2] sum |gt - d| over them;  [3] colour components in the colour sum;
 *   [4] sum (gt_c - c)^2 over them;  [5] pixels with a non-finite rendered value;  [6], [7] zero.
 * Depth L1 = [2] / [1], PSNR = -10 log10([4] / [3]).  Without d_gt_depth [1] = [2] = 0, without d_gt_color [3] = [4] = 0.
 * No floating-point atomics: lanes add their pixels in index order, waves meet by shuffles, every workgroup writes one row of partial
 * sums and a second, single-workgroup launch adds the rows in index order -- two runs give the same bytes.  Reading h_out is the call's
 * one synchronisation. */
int nsk_image_metrics(nsk_ctx* ctx, int Hv, int Wv, const float* d_rgb, const float* d_depth, const float* d_gt_depth,
                      const float* d_gt_color, float* d_res_depth, float* d_res_color, double h_out[8]);
/* nsk_image_ssim: structural similarity of two images d_a, d_b ([Hv][Wv][C] float32, channel-interleaved as d_rgb is; C = 1..4, a depth
 * image is C = 1), on the device: SSIM (Wang et al. 2004) and, with levels > 1, MS-SSIM, with the conventions of the pytorch_msssim package.
 *   Window: win odd, 3..15; g_k = exp(-(k - win/2)^2 / (2 sigma^2)) divided by the sum of the g_k taken in index order, formed on the host
 *     in double.  Padding is "valid": the map has Hm = Hv - win + 1 rows and Wm = Wv - win + 1 columns.
 *   Every pixel is widened to double once; everything after that is fp64, every multiply and add an operation of its own (no FMA).
 *   Five images are filtered, x, y, x x, y y, x y (each product formed per pixel), along W first, then along H, the taps in increasing index
 *     order: acc = g_0 v_0, then acc = acc + g_k v_k.
 *   Per window, with C1 = (k1 L)^2, C2 = (k2 L)^2, L = data_range:  sx = F(xx) - mx mx, sy = F(yy) - my my, sxy = F(xy) - mx my,
 *     cs = (2 sxy + C2) / ((sx + sy) + C2),  ssim = ((2 (mx my) + C1) / ((mx mx + my my) + C1)) cs.  ssim(x, x) is 1.0 exactly.
 *   Sums, per level and channel: the sum of ssim, the sum of cs and the count of the windows where both are finite; a window with a
 *     non-finite value is left out of both sums and counted as left out (as nsk_image_metrics does).  The association is that of the row
 *     reductions (256 threads, at most 1024 rows), the element the window index i Wm + j, the columns 3 c + {0 ssim, 1 cs, 2 count}.  No
 *     floating-point atomics: two runs give the same bytes.
 *   MS-SSIM: level l + 1 is the 2 x 2 average of level l with p = size mod 2 of zero padding per axis: pixel (i, j) =
 *     ((v(2i-p_h, 2j-p_w) + v(2i-p_h, 2j-p_w+1)) + (v(2i-p_h+1, 2j-p_w) + v(2i-p_h+1, 2j-p_w+1))) 0.25, a source pixel outside the image
 *     counting as 0; its size is (size + 2 p) / 2.  Level images stay in fp64.  The per-channel value of a level is its mean cs, of the last
 *     level its mean ssim; the result is the mean over channels of prod_l max(value_l, 0)^w_l, combined on the host in double.  h_weights
 *     ([levels] doubles, host) may be NULL only for levels = 1, or for levels = 5: the standard 0.0448, 0.2856, 0.3001, 0.2363, 0.1333.
 *     Every level must be at least win on both sides, else the call fails and names the smallest side that would do
 *     ((win - 1) 2^(levels - 1) + 1: 161 for the defaults).
 *   d_map [Hm][Wm][C] (or NULL): the level-0 ssim of every window, rounded to float32.
 *   h_out[0] the result: SSIM when levels = 1, else MS-SSIM;  [1] the level-0 SSIM, the mean over channels of the per-channel means;
 *     [2] windows counted over all levels and channels;  [3] windows left out;  [4] levels;  [5] Hm;  [6] Wm;  [7] 0.
 *   h_levels [levels][C][4] (host, or NULL): the sum of ssim, the sum of cs, the count, the value used for that level.
 * A channel-level without a finite window makes [0] NaN; that is not an error.  Not capturable (the workspace of the windows' values and of
 * the pooled levels grows to the largest call).  No other context state is read or written: a batch registered with nsk_map_prepare stays
 * registered.  Reading h_out is the call's one synchronisation. */
int nsk_image_ssim(nsk_ctx* ctx, int Hv, int Wv, int C, const float* d_a, const float* d_b, int win, double sigma, double data_range,
                   double k1, double k2, int levels, const double* h_weights, float* d_map, double h_out[8], double* h_levels);

/* ---- reconstruction metrics: accuracy, completion, completion ratio (upstream src/tools/eval_recon.py) ----------------------- */
/* nsk_mesh_sample: n area-weighted surface samples of a triangle mesh (d_vertices [n_vertices][3] float32, d_triangles [n_triangles][3]).
 *   Area: A_t = 0.5 |(b - a) x (c - a)|, formed in double from the float32 vertices.  A triangle whose area is not finite or not positive,
 *     or that has an index outside [0, n_vertices), has area 0: it is counted in *h_degenerate and never chosen.
 *   Cumulative area: the inclusive fp64 scan of A_t in triangle order (lanes by shuffles, waves, workgroups and runs of workgroups each in
 *     index order: one fixed association, two calls give the same bytes).  *h_area = its last entry.
 *   Sample s: u_k = (hash_u32(seed, s, k) >> 8) 2^-24 for k = 0, 1, 2 (the counter hash of nsk_sample_pixels);
 *     triangle = the first t with cum[t] > (double)u_0 cum[last], by binary search;
 *     r = sqrt(u_1) correctly rounded in fp32, w_a = 1 - r, w_b = r (1 - u_2), w_c = r u_2, p = (w_a a + w_b b) + w_c c per component,
 *     every product and sum an fp32 operation of its own.
 *   d_points [n][3]; d_tri [n] (or NULL) the chosen triangles.  n = 0 is valid.  n_triangles = 0 or a total area of 0 is an error.
 * Synchronises once (the total area and the count come back to the host before the samples are drawn). */
int nsk_mesh_sample(nsk_ctx* ctx, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles,
                    unsigned long long seed, int n, float* d_points, int32_t* d_tri, double* h_area, int* h_degenerate);
/* nsk_cloud_nearest: for every query point the distance to the nearest target point and (d_index, or NULL) that target.
 *   d_dist[q] = sqrt(min_t d2(q, t)), d2 = (dx dx + dy dy) + dz dz with dx = q_x - t_x (y, z alike), each operation rounded on its own in
 *   fp32, the square root correctly rounded; d_index[q] = the LOWEST t that attains the minimum of d2.  These are the bits of a brute-force
 *   evaluation over all targets; the grid below only decides which targets are looked at.
 *   A target with a non-finite component is left out and counted in *h_target_skipped (or NULL).  A query with a non-finite component gets
 *   NaN and -1.  Without a finite target every distance is +inf and every index -1.  n_target = 0 is an error; n_query = 0 is valid.
 * Search: a uniform grid of cubic cells over the box of the finite targets (device reduction -> cells and histogram -> exclusive scan ->
 * placement with the original indices), about one cell per target and never more than 2^22; an axis shorter than the cell edge has one
 * cell.  Memory O(n_target + n_query + cells), owned by the context and reused.  A query walks shells of cells of growing Chebyshev radius
 * around its own (unclamped) cell and stops when its best d2 is strictly below fl(m m), m = the smallest fp32 distance from the query to
 * a plane of the searched block that still has cells behind it, or when the block covers the grid.  The grid's planes are fp32 numbers
 * and a target's cell is defined by comparisons with them, so the bound holds for d2 as evaluated, not only in real arithmetic.
 * Synchronises once (the box and the skipped count come back to the host; the grid is sized from them). */
int nsk_cloud_nearest(nsk_ctx* ctx, const float* d_query, int n_query, const float* d_target, int n_target, float* d_dist,
                      int32_t* d_index, int* h_target_skipped);
/* nsk_cloud_stats: h_out[0] the sum of the finite distances, each widened to double;  [1] their number;  [2] the number of finite
 * distances with d < threshold (strict);  [3] the largest finite distance (0 without one).  No floating-point atomics: lanes add in index
 * order, waves meet by shuffles, one row per workgroup, a single-workgroup launch adds the rows in index order -- two runs give the same
 * bytes.  Reading h_out is the call's one synchronisation.  n = 0 gives zeros. */
int nsk_cloud_stats(nsk_ctx* ctx, const float* d_dist, int n, float threshold, double h_out[4]);

/* ---- reconstruction metrics against the surface itself: point-to-triangle distances, normal agreement -------------------------- */
/* nsk_mesh_nearest: for every query point [n_query][3] the distance to the nearest point of the mesh (d_dist), the triangle that holds it
 * (d_tri, or NULL) and that point (d_point [n_query][3], or NULL).  The results are the bits of a brute-force evaluation over all
 * triangles; the search structure only decides which triangles are looked at.  Every operation below is an fp32 operation of its own
 * (no FMA contraction).
 *   Which triangles take part.  The triangles to which nsk_mesh_sample gives a positive area: a triangle is left out and counted in
 *     *h_skipped (or NULL) when an index is outside [0, n_vertices), a vertex is non-finite, or the fp64 area is not finite or not positive.
 *   Box.  lo and hi are the componentwise min and max of the triangle's three fp32 vertices a, b, c.
 *   Plane candidate.  e0 = b - a, e1 = c - a, n = e0 x e1 with each component fl(fl(xy) - fl(zw));  nn = (n.x n.x + n.y n.y) + n.z n.z;
 *     s = ((q - a) . n) / nn (a dot product is (x x' + y y') + z z');  p = q - s n.  The candidate counts when all four of these hold:
 *     nn > 0;  ((e0 x (p - a)) . n) >= 0;  (((c - b) x (p - b)) . n) >= 0;  (((a - c) x (p - c)) . n) >= 0.
 *   Edge candidates, in the order ab, bc, ca.  For an edge (u, v): e = v - u, w = q - u, t = clamp((w . e) / (e . e), 0, 1) with t = 0 unless
 *     e . e > 0, p = u + t e.
 *   Clamp.  Every candidate point is clamped componentwise to [lo, hi] (p < lo ? lo : p > hi ? hi : p).  The clamp is exact, and it is
 *     what makes the stopping bound below hold for the value as evaluated.
 *   Distance.  d2 = (dx dx + dy dy) + dz dz with dx = q_x - p_x, exactly as nsk_cloud_nearest forms it.
 *   Choice.  The triangle's d2 is the smallest candidate's; ties go plane, ab, bc, ca.  Across triangles the lowest triangle index wins
 *     among equal d2.  d_dist = the correctly rounded square root of that d2; d_point = the clamped candidate point that gave it.
 *   Conventions, as in nsk_cloud_nearest.  A query with a non-finite component gets NaN / -1 / NaN.  Without a participating triangle
 *     every query gets +inf / -1 / NaN (so does a query for which no candidate of any triangle has a comparable d2, which needs
 *     coordinates whose squares overflow).  n_triangles = 0 is an error that leaves the context usable; n_query = 0 is valid.
 * Search: a uniform grid with the planes and the cell rule of nsk_cloud_nearest over the box of the participating triangles' vertices.
 * A triangle is registered in every cell its [lo, hi] overlaps (count -> exclusive scan -> place); the cell edge stays above 8 ulp of the
 * largest coordinate, there are at most 2^22 cells, and the edge grows by 1.25 until the references fit their cap.  A triangle whose box
 * covers more than 64 cells goes to a wide list that every query tests before its walk.  A query walks the shells of nsk_cloud_nearest and
 * stops on the same rule, best d2 < fl(m m) strictly: a triangle that is registered in no cell of the searched block has its whole
 * [lo_a, hi_a] beyond one of the block's planes on some axis a, the clamped candidate point lies inside [lo_a, hi_a], so |fl(q_a - p_a)|
 * >= m and d2 as evaluated >= fl(m m).  nsk_set_tuning "surface_cells_x4" (cells aimed at per participating triangle, in quarters;
 * default 16) and "surface_query_mode" (bit 0 reserved; + 2 queries always in input order, + 4 always in cell order; 0: in cell order
 * from 2^19 queries on) change no byte of the result.  Memory O(n_triangles + references + cells + n_query), owned by the context and
 * reused.  Not capturable.  Synchronises (the box, the skipped count and the reference count come back to the host). */
int nsk_mesh_nearest(nsk_ctx* ctx, const float* d_query, int n_query, const float* d_vertices, int n_vertices, const int32_t* d_triangles,
                     int n_triangles, float* d_dist, int32_t* d_tri, float* d_point, int* h_skipped);
/* nsk_normal_stats: the agreement of the normals of n triangle pairs; pair i is triangle d_ia[i] of mesh A (d_va [nva][3], d_ta [nta][3])
 * and triangle d_ib[i] of mesh B.
 *   Normal: n = (b - a) x (c - a), formed in double from the float32 vertices, each operation on its own (a component is xy - zw of two
 *     rounded products).  cos_i = |n_A . n_B| / (|n_A| |n_B|), the dot products as (x x' + y y') + z z', |n| = sqrt(n . n).
 *   A pair is skipped when a triangle index is negative or out of range, a vertex index is out of range, or a length is not finite or not
 *     positive.
 *   h_out[0] the sum of cos_i;  [1] the pairs counted;  [2] the pairs skipped.  The sum is the row reduction of nsk_cloud_stats: two runs
 *     give the same bytes.  n = 0 gives zeros.  Reading h_out is the call's one synchronisation.  Not capturable. */
int nsk_normal_stats(nsk_ctx* ctx, int n, const float* d_va, int nva, const int32_t* d_ta, int nta, const int32_t* d_ia,
                     const float* d_vb, int nvb, const int32_t* d_tb, int ntb, const int32_t* d_ib, double h_out[3]);

/* ---- alignment: point-to-point ICP of the reconstruction onto the ground truth (upstream src/tools/eval_recon.py, align=True: Open3D's
 * registration_icp with threshold 0.1 m, identity start, 30 iterations, relative fitness / RMSE 1e-6) ------------------------------ */
/* The rule.
 *   Transformed source point.  Source S [n_s][3] and target T [n_t][3] are float32 on the device.  The current transform M is a 4x4 of
 *     doubles on the host, row-major, last row 0 0 0 1 (the last row is not read).  The point is formed in double from the float32 source
 *     point: s'_a = ((M[a][0] x + M[a][1] y) + M[a][2] z) + M[a][3], every product and sum its own operation (no FMA), and rounded once to
 *     float32.  A source point with a component that is not finite is its own s', unchanged.  It is always the ORIGINAL source that is
 *     transformed, by the accumulated M -- never a transformed copy again -- so rounding does not pile up over iterations.
 *   Correspondence.  The nearest finite target and its distance d exactly as nsk_cloud_nearest defines them for the query s': the same
 *     bits, the lowest index on ties.  The pair counts when s' is finite and d <= threshold (inclusive, on the fp32 distance).
 *   Pair sums.  17 doubles over the counting pairs: [0] the count; [1] sum d d, the fp32 d widened to double and squared there;
 *     [2..4] sum s'; [5..7] sum t; [8..16] sum s'_a t_b, row-major, the float32 values widened and the products in double.
 *     No floating-point atomics.  Pairs are added by SOURCE INDEX whatever order the queries ran in, in the association of
 *     nsk_cloud_stats: a lane adds its sources in index order, lanes meet by shuffles, waves in wave order, one row per workgroup, a
 *     single-workgroup launch adds the rows in index order.  Two runs, and every cloud_query_mode / cloud_cells_x4, give the same bytes.
 *   Rigid solve (host, double, no scaling: Umeyama / Kabsch; csrc/nsk_rigid.h).  n = [0], mu_s = [2..4] / n, mu_t = [5..7] / n,
 *     C = sum s' t^T / n - mu_s mu_t^T.  C = U diag(sigma) V^T by a cyclic one-sided Jacobi, sigma descending.
 *     R = V diag(1, 1, det(V U^T)) U^T, which maps s' onto t;  trans = mu_t - R mu_s;  the update is [R trans; 0 0 0 1].
 *     rank = the number of sigma above 1e-12 of the largest (a C that is all rounding of its own formation, every sigma below 1e-14 of
 *     the largest |sum s'_a t_b| / n, has rank 0).  Rank >= 2 determines R.  Rank <= 1 still returns a proper rotation
 *     (R^T R = I, det +1, finite) and is reported as `degenerate`.  A count of 0 returns the identity.
 *   The loop (Open3D's, in its order).  1. evaluate the pairs under M_0 (the init, default identity): fitness = count / n_s,
 *     rmse = sqrt([1] / count) (0 without a pair).  2. solve for the update U from the sums.  3. M <- U M, a 4x4 product in double,
 *     every product and sum on its own, k ascending.  4. evaluate again.  5. stop when both |fitness - previous| < rel_fitness and
 *     |rmse - previous| < rel_rmse (converged), or after max_iter updates.  max_iter = 0 is the evaluation alone.  A count of 0 at any
 *     evaluation stops the loop (not converged) and returns the M that was evaluated.
 *
 * nsk_cloud_pair_sums: one evaluation.  h_M NULL: the identity.  d_dist [n_source] / d_index [n_source] (either may be NULL) receive the
 *   correspondences by source index: NaN / -1 where s' is not finite, +inf / -1 without a finite target.  *h_target_skipped (or NULL) =
 *   targets with a non-finite component.  n_source = 0 is valid (zeros).  n_target = 0 and a negative threshold are errors that leave
 *   the context usable.  Synchronises twice: the grid's box, the sums.
 * nsk_rigid_from_sums: the rigid solve alone.  Host only: no context, no device.  h_U [16] row-major, *h_rank (or NULL) as above.
 *   A sum that is not finite is an error.
 * nsk_cloud_icp: the loop.  The targets' grid is built once; every evaluation queries it with the source transformed on load (no
 *   transformed copy of the source is stored) and costs one synchronisation (the sums).  h_init NULL: the identity.  h_M [16] receives
 *   the accumulated transform.  h_info: [0] updates applied; [1] fitness and [2] inlier rmse of the last evaluation (of h_M);
 *   [3] its correspondences; [4] 1 converged, 0 stopped at max_iter or without a pair; [5] targets skipped; [6] sources whose s' is not
 *   finite; [7] 1 when any solve had rank <= 1.  n_source = 0 is valid and gives the init.  n_target = 0, a negative threshold or a
 *   negative max_iter are errors that leave the context usable.
 * nsk_cloud_transform: d_out[p] = the transformed point of d_in[p] by the rule above, n points; d_out == d_in is allowed; a point with a
 *   non-finite component passes through unchanged.  h_M NULL: the identity.  Asynchronous.
 * None of the four may be called while a graph is being captured (nsk_rigid_from_sums aside). */
int nsk_cloud_pair_sums(nsk_ctx* ctx, const float* d_source, int n_source, const float* d_target, int n_target, const double* h_M,
                        float threshold, double* h_sums, float* d_dist, int32_t* d_index, int* h_target_skipped);
int nsk_rigid_from_sums(const double* h_sums, double* h_U, int* h_rank);
int nsk_cloud_icp(nsk_ctx* ctx, const float* d_source, int n_source, const float* d_target, int n_target, float threshold, int max_iter,
                  double rel_fitness, double rel_rmse, const double* h_init, double* h_M, double* h_info);
int nsk_cloud_transform(nsk_ctx* ctx, const double* h_M, const float* d_in, int n, float* d_out);

/* ---- reconstruction depth L1: depth views of a mesh (upstream src/tools/eval_recon.py calc_2d_metric) -------------------------- */
/* nsk_mesh_depth: depth images of a triangle mesh (d_vertices [n_vertices][3] float32, d_triangles [n_triangles][3] int32, device) from
 * V views: h_w2c [V][16] row-major world-to-camera on the host, the camera looking along -z, as in nsk_lattice_seen.  d_depth [V][H][W]
 * float32 on the device receives the depth along -z of the nearest surface, 0 where nothing is hit (the background value of upstream's
 * renderer, and what nsk_image_metrics reads as "no measurement").  H W <= 2^24, so pixel indices are exact in fp32.  n_triangles = 0 is
 * valid and gives zeros; V = 0 is valid.  Every operation below is an fp32 operation of its own (no FMA).
 *   Camera space, vertex p, a = 0..2:  c_a = ((w[4a] p0 + w[4a+1] p1) + w[4a+2] p2) + w[4a+3];   d = -c_2.
 *   Left out: a triangle with an index outside [0, n_vertices) is left out of every view and counted once in *h_skipped (may be NULL);
 *     a triangle with a camera-space component that is not finite in a view is left out of that view.
 *   Pixel (column i, row j): the ray through the camera centre is (x, y, -1), x = (i - cx) / fx, y = -((j - cy) / fy).
 *   Edge values, with n(p, q) = p x q, n_x = (p_y q_z) - (p_z q_y), n_y = (p_z q_x) - (p_x q_z), n_z = (p_x q_y) - (p_y q_x):
 *     E(p, q) = (x n_x + y n_y) - n_z;   U = E(b, c), V = E(c, a), W = E(a, b) for the camera-space vertices a, b, c.
 *     The pixel is inside when U >= 0, V >= 0 and W >= 0, or U <= 0, V <= 0 and W <= 0: both faces are drawn.  Two triangles that share
 *     an edge evaluate its value as exact negatives of each other, so a welded surface has no cracks and needs no fill convention: a
 *     pixel on the edge is taken by both and the minimum decides.
 *   Depth, from the plane through a (not from the edge values, which lose distance / size of their digits):
 *     e1 = b - a, e2 = c - a, n = e1 x e2 (as above);   t = ((a_x n_x + a_y n_y) + a_z n_z) / ((x n_x + y n_y) - n_z).
 *     The hit counts when t is finite and t > 0; t is the depth along -z.
 *   The pixel box is part of the rule, not an acceleration: only its pixels are tested.
 *     all three d <= 0: the triangle is behind the camera and has no pixel;
 *     all three d > 0: u_k = cx + (fx c_0) / d, v_k = cy - (fy c_1) / d as in nsk_lattice_seen; if all six are finite and below 2^20 in
 *       magnitude the box is the columns floor(min u) - 1 .. floor(max u) + 2 and the rows floor(min v) - 1 .. floor(max v) + 2, clamped
 *       to the image (an empty box has no pixel);
 *     every other case (a triangle across the camera plane, a projection out of range): the whole image.  Such a triangle is drawn
 *       correctly by the rule as it stands; there is no clipping step.
 *   Result per pixel and view: the minimum t over the triangles that hit it; its bits do not depend on the order of execution.
 * One thread per triangle loads its vertices once and loops over the views of a launch (32 views' matrices ride in the kernel arguments;
 * longer lists go in several launches).  The image itself is the depth buffer: the uint32 bits of t, +inf at first, lowered by an atomic
 * minimum (behind a plain load that skips it when the stored value is already smaller); a finish pass turns +inf into 0.  A (view,
 * triangle) pair whose box has more than raster_inline_max pixels goes to a context-owned queue (one atomic cursor, raster_queue_cap
 * entries of 24 B) that a second kernel walks with a wave per entry, 64 pixels at a time; when the queue is full the thread walks the box
 * itself.  nsk_set_tuning "raster_inline_max", "raster_queue_cap", "raster_load_first" (0: the bare atomic) are test and sweep aids: every
 * setting gives the same bytes.  Asynchronous on the context's stream; asking for *h_skipped is the call's only synchronisation.  An
 * allocation that fails names its byte count and leaves the context usable.  Not while a graph is being captured. */
int nsk_mesh_depth(nsk_ctx* ctx, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles, int V,
                   const float* h_w2c, int H, int W, float fx, float fy, float cx, float cy, float* d_depth, int* h_skipped);
/* nsk_depth_pair_stats: per-view sums over two depth stacks d_a, d_b [V][n_pix] (device) -> h_out [V][4] doubles:
 *   [0] the sum of |a - b| over all pixels, each difference one fp32 operation widened to double (upstream's np.abs(gt - ours).mean()
 *       numerator: the background zeros are part of it);   [1] the number of pixels with a > 0 and b > 0;
 *   [2] the sum of |a - b| over the pixels of [1];   [3] the number of pixels with a > 0.
 * A term that is not finite is left out of its sums.  No floating-point atomics: lanes add in index order, waves meet by shuffles, one
 * row per workgroup (at most 64 per view, a function of n_pix alone), a second launch adds each view's rows in index order -- two runs
 * give the same bytes.  All views go in one call; reading h_out is its one synchronisation.  n_pix <= 2^24, V <= 2^20; V = 0 is valid. */
int nsk_depth_pair_stats(nsk_ctx* ctx, const float* d_a, const float* d_b, int V, int n_pix, double* h_out);
/* nsk_depth_views: the V random views inside a mesh's box that Depth L1 is taken over, as h_w2c [V][16] for nsk_mesh_depth.
 *   The box: the minimum and maximum of the vertices with finite coordinates (the reduction of nsk_cloud_nearest), written to
 *   h_box = {lo x y z, hi x y z}.  With d_vertices NULL the box is read from h_box instead, and the call needs neither context nor device.
 *   View k, every operation a double operation of its own (no FMA), lo / hi widened from float32:
 *     u_m = (hash_u32(seed, k, m) >> 8) 2^-24, m = 0..5 (the counter hash of nsk_sample_pixels);   ext = hi - lo, ctr = 0.5 (lo + hi);
 *     origin_a = ctr_a + (u_a - 0.5) (shrink ext_a): uniform in the box scaled by shrink about its centre;
 *     target_a = lo_a + u_{3+a} ext_a: uniform in the box;   f = target - origin, then f = f / sqrt((f_0 f_0 + f_1 f_1) + f_2 f_2);
 *     upstream's viewmatrix with up = (0, 0, -1):  s = up x f = (f_1, -f_0, 0) / sqrt(f_1 f_1 + f_0 f_0);   v = f x s, each component
 *     (f_y s_z) - (f_z s_y) and so on, then v = v / sqrt((v_0 v_0 + v_1 v_1) + v_2 v_2);
 *     upstream's camera looks along +z with y down, this project's along -z with y up: camera-to-world has the columns s, -v, -f, origin;
 *     inverted as a rigid motion: row a of world-to-camera is r_a = s, -v, -f and its fourth entry -((r_a0 o_0 + r_a1 o_1) + r_a2 o_2);
 *     each of the twelve rounded once to float32; the last row is 0 0 0 1.
 *   A view whose direction is parallel to up, or whose target is its origin, has NaN entries: nsk_mesh_depth then draws nothing for it. */
int nsk_depth_views(nsk_ctx* ctx, const float* d_vertices, int n_vertices, float h_box[6], unsigned long long seed, double shrink, int V,
                    float* h_w2c);
/* nsk_depth_views_range: views first .. first + V - 1 of the stream nsk_depth_views draws from the box h_box (lo x y z, hi x y z), as h_w2c
 * [V][16]: view first + k reads u_m = (hash_u32(seed, first + k, m) >> 8) 2^-24 and is formed as stated above.  Host only: no context, no
 * device.  nsk_depth_views is this with first = 0 (after it has found the box).  first >= 0 and first + V <= 2^32 (the hash's counter is
 * 32 bits wide); V = 0 is valid. */
int nsk_depth_views_range(const float h_box[6], unsigned long long seed, double shrink, long long first, int V, float* h_w2c);

/* ---- culling a mesh to what a trajectory saw; depth views clear of the unseen (upstream src/tools/cull_mesh.py, and the unseen points that
 * eval_recon.py's calc_2d_metric rejects views with) ---------------------------------------------------------------------------------- */
/* nsk_points_seen: the points of a list (d_points [n][3] float32, device) that at least one of K frames saw: d_seen[p] = 1, else 0 (device,
 * one byte per point).  d_depth [K][H][W] floats on the device or NULL; h_w2c [K][16] row-major world-to-camera on the host; the camera
 * looks along -z.  Frame k sees the point p by the rule of nsk_lattice_seen, word for word -- every operation an fp32 operation of its own
 * (no FMA):
 *   c_a = ((w[4a] p0 + w[4a+1] p1) + w[4a+2] p2) + w[4a+3], a = 0..2;   d = -c_2 > 0;
 *   u = cx + (fx c_0) / d,  v = cy - (fy c_1) / d;   i = floor(u + 0.5), j = floor(v + 0.5)   (the nearest pixel);
 *   edge <= i < W - edge and edge <= j < H - edge, decided on the floats (a NaN fails; an edge that leaves no pixel is valid: nothing is seen);
 *   D = d_depth[k][j][i] is finite and > 0 (a pixel without a measurement sees nothing);   d <= D + eps   (eps takes the place of trunc).
 * zero_sees != 0 is for depth that was rendered from the mesh itself (nsk_mesh_depth): a pixel with D == 0 (nothing hit, so nothing in
 * the way) is read as FLT_MAX; NaN and +-inf still see nothing.  d_depth == NULL is the frustum alone: every pixel is read as FLT_MAX.
 * A point with a component that is not finite is never seen.  accumulate != 0 ORs the old byte in, as in nsk_lattice_seen, so a long
 * trajectory can be streamed through in batches of a few depth images; K = 0 with accumulate = 0 clears the mask.  n = 0 is valid;
 * n <= 2^31 - 1.  One thread per point loops over the frames (at most 32 frames' matrices ride in the kernel arguments; longer lists go in
 * several launches); a wave leaves the loop once all its points are seen.  n_seen (may be NULL) receives the number of set bytes after the
 * call: asking for it is the call's only synchronisation.  Not while a graph is being captured. */
int nsk_points_seen(nsk_ctx* ctx, const float* d_points, int n, int K, const float* d_depth, int H, int W, float fx, float fy, float cx,
                    float cy, const float* h_w2c, int edge, float eps, int zero_sees, int accumulate, uint8_t* d_seen, long long* n_seen);
/* nsk_mesh_select: the sub-mesh of a mesh the caller owns (d_vertices [n_vertices][3] float32, d_triangles [n_triangles][3] int32, device)
 * that a per-vertex mask selects (d_seen [n_vertices] bytes, any non-zero byte counts as set): upstream's face_mask = mask[faces].all(axis=1)
 * followed by remove_unreferenced_vertices.
 *   A triangle with an index outside [0, n_vertices) belongs to neither part and is counted in *h_skipped (may be NULL).
 *   part = 0: the triangles whose three vertices are all seen.  part = 1: every other valid triangle (the unseen complement).
 *   Kept triangles keep their relative order.  A vertex stays when a kept triangle names it; kept vertices keep their relative order.
 *   Triangles are re-indexed.  d_vertex_src[o] (or NULL) is the input index of output vertex o.
 * The output buffers (d_out_vertices [n_vertices][3], d_out_triangles [n_triangles][3], d_vertex_src [n_vertices]) are the caller's, sized
 * for the input (the output cannot be larger), and must not alias the input.  Compaction by the multi-launch scans of nsk_mesh_extract:
 * no atomic append, so two runs give the same bytes.  An empty result gives zero counts and no error; n_vertices = 0 or n_triangles = 0
 * is valid.  At most (2^31 - 1) / 3 vertices and triangles.  Synchronises once, for the counts.  Device memory: 4 B per vertex and per
 * triangle of scan scratch (+ its upper levels); an allocation that fails names its byte count and leaves the context usable.  Not while
 * a graph is being captured. */
int nsk_mesh_select(nsk_ctx* ctx, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles, const uint8_t* d_seen,
                    int part, float* d_out_vertices, int32_t* d_out_triangles, int32_t* d_vertex_src, int* out_vertices, int* out_triangles,
                    int* h_skipped);
/* nsk_points_view_counts: h_count[k] = the number of the points (d_points [n][3], device) that view k (h_w2c [V][16], host) has in its
 * image by the frustum rule of nsk_points_seen (camera space, d > 0, the nearest pixel inside the edge bounds; a point with a component
 * that is not finite is never counted).  No depth: a hidden point still counts, as upstream's check_proj does.  n <= 2^31 - 1, so the
 * 32-bit device counters cannot wrap.  One thread per point loops over the launch's 32 views; per view a ballot and a population count,
 * and one integer atomic add per wave with a non-zero count: integer addition gives the same result whatever the order.  V = 0 and n = 0
 * are valid.  Reading h_count is the call's one synchronisation.  Not while a graph is being captured. */
int nsk_points_view_counts(nsk_ctx* ctx, const float* d_points, int n, int V, const float* h_w2c, int H, int W, float fx, float fy, float cx,
                           float cy, int edge, long long* h_count);

/* ---- depth frames fused into a truncated signed distance volume on a lattice (the first half of upstream's get_bound_from_frames, whose
 * Open3D ScalableTSDFVolume is sparse and on the host; here the volume is dense, on the device, and meshed by nsk_mesh_extract) -------- */
/* nsk_tsdf_integrate: K depth frames at known poses integrated into d_tsdf / d_weight (device, nx * ny * nz floats each).  Node points,
 * layout ([(k * ny + j) * nx + i]), camera convention (h_w2c [K][16] row-major world-to-camera on the host, the camera looks along -z),
 * `edge` and the at most 2^28 nodes are as in nsk_lattice_seen.  Every operation below is an fp32 operation of its own (no FMA).
 * Frame k SEES the node p exactly when nsk_lattice_seen says so with the same edge and trunc:
 *   c_a = ((w[4a] p0 + w[4a+1] p1) + w[4a+2] p2) + w[4a+3], a = 0..2;   d = -c_2 > 0;
 *   u = cx + (fx c_0) / d,  v = cy - (fy c_1) / d;   i = floor(u + 0.5), j = floor(v + 0.5)   (the nearest pixel);
 *   edge <= i < W - edge and edge <= j < H - edge, decided on the floats (a NaN fails; an edge that leaves no pixel is valid: nothing is seen);
 *   D = d_depth[k][j][i] is finite and > 0 (a pixel without a measurement sees nothing);   d <= D + trunc.
 * So weight > 0 after a call from a cleared state is, byte for byte, the mask nsk_lattice_seen gives.  A frame that sees the node updates
 * it; the frames are applied in ascending k; each of these is one rounding:
 *   sdf = D - d;
 *   t = min(1, sdf / trunc)   (the occlusion test already gives t >= -1 up to rounding: there is no clamp below);
 *   T <- ((W * T) + t) / (W + 1);
 *   W <- min(W + 1, max_weight).
 * A frame that does not see the node leaves both values untouched.  accumulate == 0 starts every node from T = 0, W = 0 whatever the
 * buffers held (NaN included: the old values are not read, no 0 * T_old is formed); K = 0 then clears the buffers.  accumulate != 0
 * continues from the buffers: a trajectory streamed in batches of any size gives the bytes of one call over all frames.
 * Errors (< 0, a message in nsk_last_error, the context stays usable): trunc not finite or <= 0; max_weight < 1 or > 2^24 (beyond it
 * W + 1 no longer counts); more than 2^28 nodes; H or W outside 1 .. 2^24; intrinsics that are not finite; edge < 0; while a graph is
 * being captured.  n_observed (may be NULL) receives the number of nodes with W > 0 after the call: asking for it is the call's only
 * synchronisation.
 * One thread per node, x fastest, loops over the frames (matrices and intrinsics ride in the kernel arguments, 32 frames per launch,
 * longer lists in several launches); T and W stay in registers over a launch's frames and are stored once.  Every frame counts, so
 * no wave leaves the loop early; no atomics but the one integer add per wave of the count. */
int nsk_tsdf_integrate(nsk_ctx* ctx, const float h_origin[3], const float h_step[3], int nx, int ny, int nz, int K, const float* d_depth,
                       int H, int W, float fx, float fy, float cx, float cy, const float* h_w2c, int edge, float trunc, float max_weight,
                       int accumulate, float* d_tsdf, float* d_weight, long long* n_observed);
/* nsk_tsdf_volume: the fused values as a volume for nsk_mesh_extract (n nodes; all pointers device).  Where d_weight >= min_weight:
 * d_volume = -T (the sign bit flipped, so +0.0 gives -0.0: nsk_mesh_extract's "inside when value > level" then puts the solid behind the
 * surface) and d_valid = 1.  Elsewhere (a NaN weight included) d_volume is the quiet NaN 0x7fc00000 and d_valid = 0.  d_valid may be
 * NULL: nsk_mesh_extract skips cells with a corner that is not finite anyway.  nsk_mesh_extract at level 0 then gives a welded mesh,
 * wound towards free space, with the same bytes in two runs.  n_valid (may be NULL) receives the number of valid nodes; the call is
 * asynchronous on the context's stream unless it is asked for.  n = 0 is valid.  Not while a graph is being captured. */
int nsk_tsdf_volume(nsk_ctx* ctx, long long n, const float* d_tsdf, const float* d_weight, float min_weight, float* d_volume,
                    uint8_t* d_valid, long long* n_valid);

/* ---- vertex normals of an indexed mesh; vertex colours from short rays along them (upstream's meshing.color_mesh_extraction_method
 * render_ray_along_normal: mesh.compute_vertex_normals(), then a ray of 0.1 m per vertex through render_batch_ray, stage color) ------ */
/* ---- the convex hull of a point cloud, and the lattice nodes inside the scaled hull (the second half of upstream's
 * get_bound_from_frames: the hull of the fusion's vertices and the camera centres, scaled by meshing.clean_mesh_bound_scale; Mesher.get_mesh
 * evaluates the map only inside it) ------------------------------------------------------------------------------------------------------ */
/* nsk_points_hull: the hull of d_points [n][3] float32 (device) followed by h_extra [n_extra][3] (host: the camera centres); indices run
 * over the concatenation, n + n_extra <= 2^31 - 1; either part may be empty.  Every decision is an integer comparison, so two runs, a
 * fresh context and tests/hull_checks.py give the same bytes however many points are coplanar or collinear:
 *   1. a point with a non-finite coordinate is left out and counted;
 *   2. lo_a / hi_a: the finite points' minimum / maximum per axis, widened to double; E = max_a(hi_a - lo_a) (E == 0: no hull);
 *      s = (2^20 - 1) / E;  q_a = (int64) rint((double(p_a) - lo_a) * s), every operation an fp64 operation of its own, rint to even;
 *   3. det(a, b, c, p) = ((q_b - q_a) x (q_c - q_a)) . (q_p - q_a) in int64 (differences < 2^20, cross components < 2^41, the dot product
 *      < 3 * 2^61: no overflow); p is OUTSIDE the face (a, b, c) when det > 0, strictly;
 *   4. i0: the lexicographically smallest (q_x, q_y, q_z, index); i1: the largest squared distance from i0; i2: the largest
 *      max(|c_x|, |c_y|, |c_z|) of c = (q_i1 - q_i0) x (q_p - q_i0); i3: the largest |det(i0, i1, i2, p)|; every tie to the smallest index.
 *      A maximum of 0 means a point, a line or a plane: no hull, and info carries the rank (0, 1, 2).  If det(i0, i1, i2, i3) > 0, i1 and i2
 *      are swapped.  Faces 0..3 are (i0, i1, i2), (i0, i3, i1), (i1, i3, i2), (i2, i3, i0);
 *   5. every other finite point belongs to the lowest-numbered face it is outside of; a point outside no face is interior for good;
 *   6. until no live face has an outside point: F = the lowest-numbered live face with one; the apex = F's outside point with the largest
 *      det, ties to the smallest index; the visible faces = all live faces with det(face, apex) > 0; a horizon edge = a directed edge
 *      (u, v) of a visible face whose twin (v, u) belongs to a live face that is not visible; the new faces (u, v, apex) are created in
 *      ascending (visible face number, edge slot), the slots of (a, b, c) being (a, b), (b, c), (c, a), and take the next face numbers
 *      (never reused); the visible faces die; the points of their outside sets, but the apex, go to the lowest-numbered NEW face they are
 *      outside of, or become interior;
 *   7. the faces: the live faces in ascending number, as index triples wound so that outside is det > 0; the vertices: the ascending list
 *      of the indices the faces name.  (A tie can elect a point in the interior of a flat face, and it then stays a vertex: harmless for
 *      an inside test, and part of the rule.)
 * The quantum E / (2^20 - 1) is about 8 um for an 8 m room: 16 fp32 ulps at that magnitude, far below any lattice step.
 * h_info: [0] finite points, [1] points left out, [2] rank (3: there is a hull; 0 also without a finite point), [3] vertices, [4] faces,
 * [5] insertions, [6] the quantum as the bits of a double (0 without one), [7] re-compactions of the list of outside points.  The call
 * succeeds without a hull ([3] = [4] = 0).
 * What grows with n runs on the device: the bounds, the quantisation to int32 triples, the four selection passes, and per insertion one
 * launch over the compacted list of the points still outside, which re-homes the points whose face died (a point decides that itself:
 * the apex sees its face) and combines each new face's count and largest det (64-bit integer maxima, then a minimum of the index among the
 * points that reach it: no result depends on the order of the atomics) in LDS before at most one global update per workgroup and face.
 * The list is re-compacted (the multi-launch scan of nsk_mesh_extract) when less than half of it is still outside.  The face table
 * (csrc/nsk_hull_plan.h: a few thousand faces) lives on the host: per insertion one upload of the new faces' planes, one download of their
 * counts and apexes -- one synchronisation per hull vertex.  Device memory: 16 B per point, + 4 B per point outside at the first
 * re-compaction, + 40 B per face ever made.  A failing allocation names its byte count; the context stays usable.  Not while a graph is
 * being captured.  The hull stays in the context until the next nsk_points_hull or nsk_hull_upload. */
int nsk_points_hull(nsk_ctx* ctx, const float* d_points, int n, const float* h_extra, int n_extra, long long h_info[8]);
/* the last hull: h_vertices [info[3]] ascending indices, h_faces [info[4]][3]; either may be NULL; nothing is written without a hull */
int nsk_hull_download(nsk_ctx* ctx, int32_t* h_vertices, int32_t* h_faces);
/* a caller's own convex mesh as the bound: h_xyz [n_vertices][3] finite coordinates, h_faces [n_faces][3] vertex numbers, wound so that
 * (B - A) x (C - A) points outwards; at least 4 and at most 2^24 of each.  Convexity and closedness are the caller's business. */
int nsk_hull_upload(nsk_ctx* ctx, const float* h_xyz, int n_vertices, const int32_t* h_faces, int n_faces);
/* nsk_lattice_in_hull: d_valid[(k * ny + j) * nx + i] = 1 for the lattice nodes (origin, step, nx, ny, nz, node points and the at most 2^28
 * nodes as in nsk_lattice_seen) inside the last hull scaled about its centre, else 0 -- the d_valid of nsk_mesh_extract and
 * nsk_eval_lattice_masked.  All of it fp64, every operation rounded on its own (no FMA):
 *   the hull vertices' own fp32 coordinates (not the quantised ones) widened; c = their sum in ascending index order, left to right, divided
 *   by their number;  V' = c + scale * (V - c);  per face u = B' - A', v = C' - A', n = u x v (each product and each difference rounded);
 *   the node P formed in fp32 as nsk_eval_lattice forms it, then widened;  w = P - A';  s = (w_x n_x + w_y n_y) + w_z n_z.
 * A node is inside when it lies in the box of the V' (lo_a <= P_a <= hi_a) and no face has s > 0.  accumulate != 0 ORs the old byte in.
 * Without a hull every node is outside.  One thread per node loops over the faces; the planes are computed once per call, on the host; a
 * node outside the box never enters the loop, and a wave leaves it when all its nodes are outside.  n_inside (may be NULL) receives the
 * number of set bytes after the call.  scale > 0 and finite.  Not while a graph is being captured. */
int nsk_lattice_in_hull(nsk_ctx* ctx, const float h_origin[3], const float h_step[3], int nx, int ny, int nz, double scale,
                        int accumulate, uint8_t* d_valid, long long* n_inside);

/* ---- a mesh made smaller: uniform vertex clustering (Rossignac-Borrel).  All vertices in one cell of a uniform grid collapse to one
 * representative, triangles are re-indexed, collapsed and duplicate triangles and unreferenced vertices go ------------------------------ */
/* nsk_mesh_simplify: d_vertices [n_vertices][3] float32, d_triangles [n_triangles][3] int32 (device, the caller's) -> d_out_vertices
 * [out_vertices][3], d_out_triangles [out_triangles][3] and, unless NULL, d_vertex_map [n_vertices]: buffers of the caller, on the device,
 * sized for the input, not aliasing it (as in nsk_mesh_select).  At most (2^31 - 1) / 3 vertices and triangles; empty inputs and empty
 * results are valid.  Every decision is made on integers, so two runs, a fresh context and tests/simplify_checks.py give the same bytes:
 *   1. cell is finite and > 0, else an error.  A vertex with a non-finite coordinate is left out and counted; a triangle with an index
 *      outside [0, n_vertices), or naming a left-out vertex, is dropped and counted (invalid);
 *   2. lo_a / hi_a: the finite vertices' minimum / maximum per axis, widened to double;  g_a = (double(p_a) - lo_a) / double(cell);
 *      c_a = (int64) floor(g_a);  n_a = c_a(hi_a) + 1: every operation an fp64 operation of its own, no contraction.  The cell index is
 *      (c_z n_y + c_y) n_x + c_x.  More than 2^28 cells is an error that names the count; so is an axis of more than 2^21 - 1 cells
 *      (h_info[7] packs 21 bits per axis).  The context stays usable after either;
 *   3. the representative of a cell is a fixed-point mean, so that no floating-point atomic decides a bit:
 *      q_a = (int64) rint((g_a - c_a) * 2^20), ties to even; per cell the member count and the three sums of q_a over ALL its finite
 *      vertices (referenced by a triangle or not) are accumulated with integer atomics -- with count < 2^31 every sum is < 2^51;
 *      m_a = double(sum_a) / double(count);  the position is float(lo_a + (double(c_a) + m_a / 2^20) * double(cell)), each operation fp64,
 *      then one rounding to float;
 *   4. a triangle's corners map to their cells.  It is COLLAPSED (dropped, counted) when two corners share a cell.  Unless flags & 1 it is
 *      a DUPLICATE (dropped, counted) when a valid, not collapsed triangle with a lower input index has the same corner cells in the same
 *      cyclic order: the triples are compared after rotating the smallest cell to the front.  The mirrored triple (a, c, b) is NOT a
 *      duplicate: the two sides of a thin wall stay.  Kept triangles keep their relative order and their own corner order.  (With
 *      flags & 1 the output of a closed oriented mesh still has every directed edge as often as its reverse: identifying vertices commutes
 *      with the boundary.  Removing a duplicate can break that balance.)
 *   5. the output vertices are the cells a kept triangle names, in ascending cell index; the triangles are re-indexed;
 *      d_vertex_map[i] = the output vertex of input vertex i, or -1 (left out, or its cell is named by no kept triangle);
 *   6. h_info: [0] finite vertices, [1] vertices left out, [2] triangles dropped as invalid, [3] collapsed, [4] duplicates, [5] occupied
 *      cells, [6] cells, [7] n_x | n_y << 21 | n_z << 42.  Without a finite vertex there is no grid: [5] = [6] = [7] = 0, every triangle
 *      is invalid, every map entry -1.
 * Passes (csrc/nsk_simplify.h): the bounds (the first pass of nsk_points_hull), the vertices' cells and a 4-byte occupancy flag per cell,
 * the multi-launch scan of nsk_mesh_extract over the flags, so that count and sums (28 B) and the cell index (4 B) exist per OCCUPIED cell
 * only, the integer accumulation (a run of equal cells inside a wave is summed by shuffles and adds once per word), the triangles'
 * corner cells, duplicate detection without a sort (every surviving triangle is registered under its smallest corner by count -> scan ->
 * placement through an integer cursor; a triangle is a duplicate iff its list holds an equal rotated triple with a lower input index,
 * whatever order the cursor gave: one thread searches a list of up to nsk_mesh_simplify_list_threshold() triangles, a workgroup a
 * longer one; a list of k triangles costs k^2 comparisons), the collapsed count derived from the others, flags -> scans ->
 * compaction without an atomic append.  Device memory: 4 B per vertex, 4 B per cell, 40 B per occupied cell, 20 B per triangle (+ the
 * scans' levels, 1 / 255 of the flags).  Three synchronisations: the bounds size the flags, the occupied count sizes the sums, the last
 * fetches the counts.  A failing allocation names its byte count; the context stays usable.  Not while a graph is being captured. */
int nsk_mesh_simplify(nsk_ctx* ctx, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles, float cell, int flags,
                      float* d_out_vertices, int32_t* d_out_triangles, int32_t* d_vertex_map, int* out_vertices, int* out_triangles,
                      long long h_info[8]);
/* the longest smallest-corner list one thread searches (a first choice, not tuned) */
int nsk_mesh_simplify_list_threshold(void);

/* nsk_mesh_vertex_normals: the area-weighted unit normal of every vertex of a mesh (d_vertices [n_vertices][3] float32, d_triangles
 * [n_triangles][3] int32) into d_normals [n_vertices][3].  With the winding of nsk_mesh_extract the normals point to free space.  Every
 * operation below is an fp32 operation of its own (no FMA contraction).
 *   Triangle normal.  e0 = b - a, e1 = c - a, n_t = e0 x e1 with each component fl(fl(xy) - fl(zw)): the plane candidate's normal of
 *     nsk_mesh_nearest.  It is not normalised, so the sum below weighs a triangle by its area, as upstream's does.
 *   Which triangles take part.  A triangle is left out and counted in h_info[0] when an index is outside [0, n_vertices) or n_t has a
 *     component that is not finite.  A triangle that names a vertex twice takes part; its n_t is exactly zero.
 *   Sum.  For vertex v, acc starts at +0 and receives n_t once for every (triangle, corner) that names v, in ascending triangle index,
 *     then ascending corner: acc = fl(acc + n_t) per component.  The order is part of the contract, because an fp32 sum depends on it.
 *   Normalise.  nn = (x x + y y) + z z of acc;  L = the correctly rounded square root of nn;  n = acc / L per component.
 *   Vertices without a normal.  When nn is not finite or not > 0 the vertex receives (+0, +0, +0) and is counted in h_info[1]: an isolated
 *     vertex, a vertex all of whose triangles have no area, a sum that cancels, overflows or underflows.
 *   h_info (4 ints on the host, or NULL): [0] triangles left out;  [1] vertices without a normal;  [2] the largest number of namings of one
 *     vertex by triangles that take part;  [3] 0.
 * n_triangles = 0 is valid (every normal is zero); n_vertices = 0 is valid (every triangle is left out).  At most 2^30 corners
 * (3 n_triangles) and (2^31 - 1) / 3 vertices.  How: face normals are formed once and the vertices' namings counted; the counts are
 * scanned by the multi-launch scan of nsk_mesh_extract; every corner is placed into its vertex's segment of one list through an integer
 * cursor; every segment is sorted by corner number (up to 32 corners by the vertex's own thread, longer ones by a workgroup each); one
 * thread per vertex then sums over its segment in that order.  No floating-point atomic: two runs, and a run in a fresh process, give the
 * same bytes.  Device memory, owned by the context and reused: 24 B per triangle (face normals, the corner list) and 4 B per vertex (+ the
 * scan's upper levels); an allocation that fails names its byte count and leaves the context usable.  Reading h_info is the call's only
 * synchronisation: without it the call is asynchronous on the context's stream.  Not while a graph is being captured. */
int nsk_mesh_vertex_normals(nsk_ctx* ctx, const float* d_vertices, int n_vertices, const int32_t* d_triangles, int n_triangles,
                            float* d_normals, int h_info[4]);
/* nsk_normal_rays: for each of n vertices the ray that looks at the surface from `length` out along the normal (d_rays_o [n][3],
 * d_rays_d [n][3], d_gt_depth [n], d_has_ray [n] bytes or NULL).  `length` must be finite and > 0.
 *   A vertex whose normal is not zero, with every component of vertex and normal finite:  o = fl(v + fl(length n)) per component,  d = -n,
 *     gt_depth = length,  has_ray = 1.
 *   Every other vertex:  o = v (its bits),  d = (0, 0, -1),  gt_depth = length,  has_ray = 0: a ray that renders, whose result is not used.
 * n = 0 is valid.  Asynchronous on the context's stream. */
int nsk_normal_rays(nsk_ctx* ctx, int n, const float* d_vertices, const float* d_normals, float length, float* d_rays_o, float* d_rays_d,
                    float* d_gt_depth, uint8_t* d_has_ray);
/* nsk_mesh_vertex_colors: the colour of every vertex into d_rgb [n_vertices][3], not clamped.
 *   With d_normals: a vertex with has_ray (nsk_normal_rays with `length`) receives, bit for bit, the rgb that nsk_render_forward gives its
 *     ray at stage NSK_COLOR with d_gt_depth = length and gt_depth_max = length, under the context's current render options (so every
 *     ray carries n_samples + n_surface samples, the surface samples around `length`, i.e. around the vertex).  gt_depth_max is given
 *     and not taken from the batch, so neither the chunking nor the rays of the other vertices change a byte.  Every other vertex
 *     receives channels 0..2 of nsk_eval_points at stage NSK_COLOR at the vertex itself, and *h_fallback (or NULL) counts them.
 *   With d_normals NULL every vertex takes the point query (*h_fallback = n_vertices): upstream's direct_point_query.
 * The vertices are walked in chunks of chunk_rays rays (0: 25 600, the default of nsk_render_image; at most (2^26 - 1) / samples per ray),
 * point queries in chunks of as many samples; the chunk size changes no byte.  `length` must be finite and > 0 (it is not read without
 * normals, and still checked).  n_vertices = 0 is valid.  Reading h_fallback is the call's only synchronisation.  Not while a graph is
 * being captured. */
int nsk_mesh_vertex_colors(nsk_ctx* ctx, const float* d_vertices, int n_vertices, const float* d_normals, float length, int chunk_rays,
                           float* d_rgb, int* h_fallback);

/* ---- raw frames prepared on the device (upstream NICE-SLAM's dataset layer, src/utils/datasets.py __getitem__: cv2.undistort, cv2.resize
 * to the depth size, F.interpolate to cam.crop_size, cam.crop_edge cut off, the intrinsics moved along) --------------------------------- */
#define NSK_FRAME_U8 0      /* colour [n][H][W][3] bytes */
#define NSK_FRAME_U16 1     /* depth [n][H][W] 16-bit */
#define NSK_FRAME_F32 2     /* either, float32 */
typedef struct nsk_frame_opts {
    float fx, fy, cx, cy;            /* for the depth size Hd x Wd (the cam block's meaning) */
    int n_dist;                      /* 0 (no undistortion), 4, 5 or 8 coefficients */
    float dist[8];                   /* OpenCV's order k1 k2 p1 p2 [k3 [k4 k5 k6]]; those beyond n_dist are not read (they are zeros in the rule) */
    int crop_H, crop_W;              /* cam.crop_size; both 0 = off */
    int crop_edge;                   /* cam.crop_edge */
    float png_depth_scale, scale;    /* depth = (float(v) / png_depth_scale) * scale */
    int swap_rb;                     /* exchange channels 0 and 2 of the colour output */
} nsk_frame_opts;
/* The rule.  Every operation is an fp32 operation of its own (no FMA contraction), every stage's result a rounded fp32 value; a stage that
 * is off is skipped, not run with neutral parameters.  tests/frame_checks.py restates it one numpy operation per operation.
 *   S0 conversion.  uint8 colour: float(v) / 255.0f, a correctly rounded division; float32 colour passes.  Depth, both types:
 *     (float(v) / png_depth_scale) * scale.
 *   S1 undistort (colour only; on when n_dist > 0; needs Hc == Hd and Wc == Wd).  OpenCV's undistort with newCameraMatrix = K.  For the
 *     destination pixel (u, v):  x = (u - cx) / fx,  y = (v - cy) / fy,  xx = x x, yy = y y, xy = x y, r2 = xx + yy, r4 = r2 r2, r6 = r4 r2,
 *     rad = (((1 + k1 r2) + k2 r4) + k3 r6) / (((1 + k4 r2) + k5 r4) + k6 r6),
 *     xd = (x rad + (2 p1) xy) + p2 (r2 + 2 xx),   yd = (y rad + p1 (r2 + 2 yy)) + (2 p2) xy,   us = fx xd + cx,   vs = fy yd + cy.
 *     Taps at i0 = floor(us), i0 + 1 (likewise j0 from vs) with l1 = us - float(i0), l0 = 1 - l1; a tap outside the image has the value 0
 *     (OpenCV's constant border); when !(us > -1 && us < Wc && vs > -1 && vs < Hc) the pixel is 0, which also catches NaN.  Zero
 *     coefficients with n_dist > 0 still run the arithmetic.
 *   S2 colour to the depth size (on when the sizes differ): cv2.resize INTER_LINEAR = F.interpolate(bilinear, align_corners=False).  Per
 *     axis  s = float(in) / float(out),  r = max((float(o) + 0.5f) s - 0.5f, 0),  i0 = min(int(r), in - 1),  i1 = min(i0 + 1, in - 1),
 *     l1 = r - float(i0),  l0 = 1 - l1.
 *   S3 crop_size (on when crop_H, crop_W > 0).  Colour: F.interpolate(bilinear, align_corners=True): s = float(in - 1) / float(out - 1)
 *     (0 when out == 1), r = float(o) s, taps as in S2.  Depth: F.interpolate(nearest): src = min(int(floorf(float(o) (float(in) /
 *     float(out)))), in - 1); depth is never interpolated.
 *   Every bilinear value:  top = lx0 v00 + lx1 v01,  bot = lx0 v10 + lx1 v11,  out = ly0 top + ly1 bot, each product and sum rounded.
 *   S4 crop_edge: e pixels off every side.
 *   Intrinsics (fp32, on the host): with crop_size sx = float(crop_W) / float(Wd), sy = float(crop_H) / float(Hd), fx *= sx, cx *= sx,
 *     fy *= sy, cy *= sy; with crop_edge cx -= e, cy -= e.
 * nsk_frame_plan: validates the options for a colour size Hc x Wc and a depth size Hd x Wd and returns the output size and the intrinsics
 * [fx fy cx cy].  It takes no context and works without a GPU.  Errors (< 0, nsk_last_error names the option): a size < 1; n_dist not 0,
 * 4, 5 or 8; crop_edge < 0; exactly one of crop_H, crop_W positive, or one negative; undistortion with Hc != Hd or Wc != Wd; 2 crop_edge
 * >= a side of the image it is cut from. */
int nsk_frame_plan(const nsk_frame_opts* opts, int Hc, int Wc, int Hd, int Wd, int* H_out, int* W_out, float intr_out[4]);
/* nsk_frame_prepare: n raw frames (d_color_raw [n][Hc][Wc][3] of color_type NSK_FRAME_U8 / _F32, d_depth_raw [n][Hd][Wd] of depth_type
 * NSK_FRAME_U16 / _F32) -> d_color_out [n][H'][W'][3] and d_depth_out [n][H'][W'] float32, the layouts nsk_prepare_rays,
 * nsk_tsdf_integrate and nsk_points_seen take.  Either pair (raw and out) may be NULL to prepare only the other; the sizes of the absent
 * image still decide the stages.  One launch; a thread per output pixel evaluates the stages that are on by recursion over taps (at most
 * 16 raw taps per channel), so no intermediate image exists and the bytes are the rule's.
 * *h_n_border (or NULL): the number of output colour pixels, over all frames, that read at least one S1 tap outside the image through
 * whatever stages follow (a tap of weight 0 counts, a pixel S1 sets to 0 counts); 0 without S1 or without colour.  Reading it is the
 * call's only synchronisation.  n = 0 is valid.  Errors: those of nsk_frame_plan; a type the image does not have; n < 0, n > 65535 or
 * n H' W' >= 2^31; they leave the outputs untouched.  Not while a graph is being captured. */
int nsk_frame_prepare(nsk_ctx* ctx, const nsk_frame_opts* opts, int n, const void* d_color_raw, int color_type, int Hc, int Wc,
                      const void* d_depth_raw, int depth_type, int Hd, int Wd, float* d_color_out, float* d_depth_out, int* h_n_border);

/* ---- introspection for benchmarks ------------------------------------------------------------------------ */
/* algorithmic bytes / flops of the last render or step call (SURVEY.md section 8d accounting) */
int nsk_last_call_stats(nsk_ctx* ctx, double* alg_bytes, double* alg_flops, int* samples);
/* per-kernel timing with HIP events recorded on the context's stream around every launch between
 * nsk_profile_begin and nsk_profile_end; _end synchronises and writes "name launches total_ms\n" lines. */
int nsk_profile_begin(nsk_ctx* ctx);
int nsk_profile_end(nsk_ctx* ctx, char* buf, size_t buf_bytes);

/* ---- test aids (tests/test_gpu_relu.py, tools/relu_flips.py; never on the product path) ------------------------- */
/* A ReLU's derivative jumps at zero, so what a gradient test can demand depends on which side of every kink the forward stood.
 * nsk_debug_relu_bits: the "input > 0" bits the forward of the last nsk_map_step / nsk_track_step / nsk_render_backward saved for decoder
 * `which` (1 middle, 2 fine, 3 colour; reference src/models/MLP.cpp:92,98 torch::relu), by SAMPLE (ray * S + s): h_bits[M][5][32] bytes.
 * nsk_debug_preact: the ReLU inputs themselves ([M][5][32] floats, device), recomputed over the same samples by the forward body of the
 * current matmul mode (N, rays = those of the last step). */
int nsk_debug_relu_bits(nsk_ctx* ctx, int which, int M, uint8_t* h_bits);
/* nsk_debug_fetch: a per-sample array of the last step's workspace, to the host: what = 0..2 the occupancy output of decoder 0..2 [M] (their sum is
 * the sigma whose relu the compositing takes, include/torchlib/utils.h:160), 3 the colour decoder's output [M][4], 4 d loss / d raw [M][4], 5 z [M],
 * 6 the 10 x median threshold the last nsk_track_step with handle_dynamic applied (one float). */
int nsk_debug_fetch(nsk_ctx* ctx, int what, int M, float* h_out);
int nsk_debug_preact(nsk_ctx* ctx, int which, int N, const float* d_rays_o, const float* d_rays_d, float* d_preact);
/* nsk_debug_live_tiles: the dead-tile skip (nsk_set_mask) of the last step's backward, after a synchronise.  h_counts[0..2]: the 16-sample tiles the
 * frozen role of the middle / fine / colour level ran (-1: the level had no frozen role; every tile where nothing was skipped), h_counts[3]: 1 if
 * a role was skipping; h_counts[4..6]: the workgroups the launch gave the role of each level (frozen or trainable; 0: none, or one launch per
 * decoder), h_counts[7]: the tiles of the batch -- h_counts has 8 entries.  h_perm [M] (may be NULL): the sample in each tile slot; h_bytes [M] (may be NULL): the slots' liveness bytes -- bit 0
 * middle, 1 fine, 2 colour: the sample's cell at that level has a marked corner voxel (7 everywhere when the step wrote none). */
int nsk_debug_live_tiles(nsk_ctx* ctx, int M, int* h_counts, int32_t* h_perm, uint8_t* h_bytes);
/* nsk_debug_last_split: how the last forward decoder launch (dir 0) or the last backward (dir 1) of the context divided its workgroups, after a
 * synchronise.  Recorded on the host where the launch's role ranges are filled; launches nothing.  h_out has NSK_SPLIT_INTS entries:
 *   [0]      the form, one of NSK_SPLIT_* below (0: no such launch yet, or the backward had no gradient to compute)
 *   [1]      n, the roles of the launch (separate launches: the decoders launched one after the other)
 *   [2..4]   which[r]: the decoder of role r (0 coarse .. 3 colour); the merged middle + fine role of NSK_SPLIT_FWD_MERGED reports 1
 *   [5..7]   train[r]: 1 if role r is the trainable body (forward: 0)
 *   [8..10]  the workgroups of role r (single decoder / separate launches: the grid of each launch)
 *   [11]     the workgroups of the prepared batch's cell-sort scan riding behind the roles (nsk_map_prepare)
 *   [12]     1 if a workgroup behind those summed the per-ray losses (the Tracker's launch: its last workgroup did)
 *   [13]     the 16-sample tiles of the batch
 *   [14]     the workgroups of the launch, riders included
 *   [15]     1 if the last workgroup found the Tracker's median threshold (NSK_SPLIT_BWD_TRACK) */
#define NSK_SPLIT_INTS 16
#define NSK_SPLIT_FWD_SINGLE 1       /* one decoder: k_decode_fwd */
#define NSK_SPLIT_FWD_MULTI 2        /* a role per decoder, fp32 MFMA */
#define NSK_SPLIT_FWD_MULTI_SPLIT 3  /* a role per decoder, split-precision operands (matmul modes 1 and 2) */
#define NSK_SPLIT_FWD_MERGED 4       /* middle + fine as one role (+ colour) */
#define NSK_SPLIT_BWD_SEPARATE 1     /* one launch per decoder */
#define NSK_SPLIT_BWD_MULTI 2        /* k_decode_bwd_multi */
#define NSK_SPLIT_BWD_MULTI_FULL 3   /* k_decode_bwd_multi_full (nsk_set_backward_mode 0) */
#define NSK_SPLIT_BWD_FROZEN 4       /* k_decode_bwd_frozen */
#define NSK_SPLIT_BWD_TRACK 5        /* k_decode_bwd_track */
int nsk_debug_last_split(nsk_ctx* ctx, int dir, int* h_out);
/* nsk_debug_decoder_images: one of the derived copies of decoder `which`'s parameters that the MFMA kernels read, copied to the host after a
 * synchronise (tests/test_gpu_adam.py: an optimiser step rewrites them through inverse index tables, an upload builds them through the forward
 * tables, and the two must agree byte for byte).  what = 0 the fp32 forward fragment image, 1 the fp32 backward image, 2 the forward image in
 * 16-bit pieces (2 fp16 under matmul mode 2, 3 bf16 otherwise) followed by its fp32 tail, 3 the fp16 backward image followed by its fp32 tail
 * (built lazily: a stale one is rebuilt first, as the next backward that reads it would).  Returns the image's size in bytes (0: the coarse
 * decoder has no image in pieces), -1 on failure; h_out = NULL only asks for the size, otherwise capacity (bytes) must hold the image.
 * Changes nothing a step reads. */
int nsk_debug_decoder_images(nsk_ctx* ctx, int which, int what, void* h_out, size_t capacity);
/* nsk_decoder_image_table: the index table an upload builds image `what` (numbered as above) of decoder `which` through; needs no context and
 * no device.  pieces = 2 or 3 is the piece count of image 2 (the table itself does not depend on it, the image's size and layout do; ignored
 * for the other images).  Returns the number of entries (0 for images 2 and 3 of the coarse decoder, which has none), -1 on a bad argument;
 * copies the entries when h_idx is not NULL and capacity (entries) suffices, h_idx = NULL only asks for the count.
 *   How an image follows from its table idx and the packed parameters P (nsk_decoder_download):
 *   - entry t holds parameter idx[t], or zero where idx[t] = -1;
 *   - images 0 and 1 are plain: float t of the image is entry t;
 *   - images 2 and 3 keep np 16-bit pieces per entry (image 2: pieces; image 3: always 2): with fg = t / 512, lane = (t / 8) % 64, j = t % 8,
 *     piece p of entry t is unsigned short ((fg * np + p) * 64 + lane) * 8 + j of the image;
 *   - the pieces of a value x (store_pieces of csrc/nsk_bf16.h), every conversion rounding to nearest even:
 *       np = 2: h = fp16(x), l = fp16((x - float(h)) * 2048), differences and products in fp32;
 *       np = 3: h = bf16(x), m = bf16(x - float(h)), l = bf16((x - float(h)) - float(m));
 *     fp16 results below the smallest normal are kept as subnormals, not flushed;
 *   - the fragments' entries * np unsigned shorts are followed by an fp32 tail: the image's last tail_n floats equal the last tail_n floats of
 *     the fp32 sibling, image what - 2 (tail_n = 740 for image 2: biases, output weight and bias, embedding matrix; 416 for image 3: output
 *     weight, embedding matrix). */
int nsk_decoder_image_table(int which, int what, int pieces, int32_t* h_idx, size_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* NSK_H */
