/*
 * egr_raytracer.h -- C ABI of the MI355X-native differentiable Gaussian ray tracer (libegr_hip.so).
 *
 * Drop-in boundary for the hot path of graphdeco-inria/editable-gaussian-reflections:
 * editable_gauss_refl/cuda (OptiX/CUDA). The reference exposes this path as TorchScript custom classes
 * (TORCH_LIBRARY(raytracer, m), cuda/csrc/raytracer.cpp:208-218); every entry point below replaces one
 * method of that `Raytracer` class and takes exactly the raw device pointers its `reify()` structs hold.
 * No torch types cross this boundary. The thin TORCH_LIBRARY shim that re-exports these functions under
 * the reference's class names lives in editable-gaussian-reflections_amd/csrc/torch_binding.cpp; the
 * reference-side binding is shown in INTEGRATION.md.
 *
 * All pointers are DEVICE pointers (HIP, gfx950) unless stated otherwise. All arithmetic is fp32.
 * Functions return 0 on success, non-zero on failure; egr_last_error() gives the message. Nothing here
 * synchronises the stream unless documented. Not thread-safe per context (the reference is not either:
 * train.py:214-215 serialises callers with a lock).
 *
 * Paths in comments are relative to /root/reference/editable_gauss_refl/cuda/csrc/.
 */
#ifndef EGR_RAYTRACER_H
#define EGR_RAYTRACER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGR_MAX_BOUNCES 2                       /* flags.h:4  */
#define EGR_NUM_STEPS (EGR_MAX_BOUNCES + 1)
#define EGR_MAX_ALPHA 0.9999f                   /* flags.h:7  */
#define EGR_ROUGHNESS_DOWNWEIGHT_GRAD 1         /* flags.h:11 */
#define EGR_ROUGHNESS_DOWNWEIGHT_GRAD_POWER 3.0f /* flags.h:12 */
#define EGR_MAX_COMPOSITED_PER_RAY (16 * 99)    /* BUFFER_SIZE * MAX_ITERATIONS, flags.h:15-16 */
#define EGR_PPLL_NULL_PTR (2u << 29)            /* core/per_pixel_linked_list.h:4 */

typedef struct egr_context egr_context; /* replaces struct Raytracer (raytracer.cpp:24-79) */

/* core/gaussians.h:3-25 -- raw (pre-activation) parameters, row-major [count, k], and their gradients */
typedef struct egr_gaussians {
    uint32_t count;
    const float *rgb;       /* [N,3] relu            */
    const float *normal;    /* [N,3] identity        */
    const float *f0;        /* [N,3] clip01          */
    const float *roughness; /* [N,1] clip01          */
    const float *opacity;   /* [N,1] sigmoid         */
    const float *scale;     /* [N,3] exp             */
    const float *mean;      /* [N,3] identity        */
    const float *rotation;  /* [N,4] normalise (r,x,y,z) */
    float *dL_drgb, *dL_dnormal, *dL_df0, *dL_droughness, *dL_dopacity, *dL_dscale, *dL_dmean, *dL_drotation;
    float *total_weight;    /* [N,1] */
} egr_gaussians;

/* core/config.h:5-26 -- device-resident scalars, read by pointer inside the kernels (Python mutates them in place) */
typedef struct egr_config {
    const float *exp_power, *alpha_threshold, *transmittance_threshold;
    const uint8_t *accumulate_samples, *jitter_primary_rays; /* torch bool */
    const int32_t *num_bounces;
    const float *global_scale_factor;
    const float *loss_weight_diffuse, *loss_weight_specular, *loss_weight_depth, *loss_weight_normal, *loss_weight_f0,
        *loss_weight_roughness;
    const float *eps_forward_normalization, *eps_scale_grad, *eps_ray_surface_offset, *eps_min_roughness;
    const float *reflection_invalid_normal_threshold, *backfacing_invalid_normal_threshold, *backfacing_max_dist;
} egr_config;

/* core/camera.h:8-15 */
typedef struct egr_camera {
    const float *origin;               /* [3]   */
    const float *vertical_fov_radians; /* [1]   */
    const float *rotation_c2w;         /* [3,3] */
    const float *rotation_w2c;         /* [3,3] = c2w^T (camera.h:67) */
    const float *znear, *zfar;         /* [1]   */
} egr_camera;

/* core/framebuffer.h:72-102 -- outputs [3,H,W,c] indexed pixel_id + H*W*step (:132), final/denoised [1,H,W,3] */
typedef struct egr_framebuffer {
    float *output_rgb, *output_depth, *output_normal, *output_f0, *output_roughness, *output_transmittance,
        *output_total_transmittance, *output_ray_origin, *output_ray_direction, *output_final, *output_denoised;
    float *accumulated_rgb, *accumulated_transmittance, *accumulated_total_transmittance, *accumulated_depth,
        *accumulated_normal, *accumulated_f0, *accumulated_roughness;
    int32_t *accumulated_sample_count; /* [1] */
    const float *target_diffuse, *target_specular, *target_depth, *target_normal, *target_f0, *target_roughness;
} egr_framebuffer;

/* core/metadata.h:3-7 */
typedef struct egr_metadata {
    uint8_t *grads_enabled;    /* [1] torch bool, written by egr_raytrace from its argument (metadata.h:29) */
    int32_t *total_num_calls;  /* [1] incremented by egr_raytrace before the launch (metadata.h:30)        */
    int32_t *random_seeds;     /* [H,W,1] final per-pixel RNG state (shaders.cu:172)                        */
} egr_metadata;

/* core/stats.h:3-6 */
typedef struct egr_stats {
    int32_t *num_accumulated_per_pixel; /* [H,W] composited hits of the LAST executed step (forward_pass.cu:140) */
    int32_t *num_traversed_per_pixel;   /* [H,W] intersection-program invocations, all steps (forward_pass.cu:46) with egr_set_exact_stats;
                                         * by default the subset of them whose response point lies inside the gaussian's ellipsoid (see there) */
} egr_stats;

/* Whole-launch work counters (not in the reference; used for the roofline's algorithmic bytes). */
typedef struct egr_counters {
    uint64_t rays[EGR_NUM_STEPS];        /* rays traced per bounce step (a ray = one pixel x step)            */
    uint64_t candidates[EGR_NUM_STEPS];  /* candidates per step: those inside their ellipsoid (default), or Hc = cube overlaps with exact stats */
    uint64_t composited[EGR_NUM_STEPS];  /* composited hits per step (Kc)                                     */
    uint64_t lifetime_rays;              /* rays of ALL launches since egr_create / egr_reset_lifetime_counters */
    uint32_t lifetime_launches;
    uint32_t status;                     /* EGR_STATUS_* bit mask of the last launch                          */
    uint32_t bvh_depth;
    uint32_t bucket_records;             /* 64-B gradient records (16-lane atomic adds) the backward chain sent to the gradient rows in this launch */
    uint64_t device_bytes;               /* device memory this context holds right now (scratch, arena, ray state, tree, records);
                                          * the caller's tensors (parameters, gradients, framebuffer) are not included          */
    uint32_t arena_blocks_used, arena_blocks_cap; /* composited-hit arena (backward capacity): 9-KB blocks the last grad launch took (waves take them in runs of 8:
                                                   * up to 7 per resident wave are taken and not written; the count runs on past the capacity when the arena
                                                   * overflows: used > cap then) / holds */
    uint32_t ext_blocks_used, ext_blocks_cap;     /* candidate-list extension blocks (forward capacity) the last launch took / holds         */
    uint64_t accepted[EGR_NUM_STEPS];    /* accepted candidates per step = entries the reference inserts into its forward list
                                          * (shaders.cu:74; its counter runs on over the three steps, so their SUM must stay below
                                          * ppll_forward_size upstream - there is no check there)                               */
} egr_counters;

#define EGR_STATUS_OK 0u
/* Both overflows are defined states (nothing is written out of bounds, the next launch starts clean; tests/test_hip_overflow.py): */
#define EGR_STATUS_CANDIDATE_OVERFLOW 1u /* a ray met more candidates than the forward capacity allows: the candidates that found neither room in the ray's
                                          * own run nor an extension block are dropped from its list; rays whose list fits their own run are bit-exact */
#define EGR_STATUS_HIT_ARENA_OVERFLOW 2u /* composited-hit arena (backward capacity) exhausted: an 8x8 tile's bounce step that needed a block and got none is
                                          * not recorded at all; the forward results stay exact, the gradients are exactly those of the recorded (tile, step)s */

/* Raytracer::Raytracer(width, height, num_gaussians, ppll_forward_size, ppll_backward_size) (raytracer.cpp:45-79).
 * The two sizes are entry counts of the reference's per-pixel linked lists (36 B per entry,
 * per_pixel_linked_list.h:6-16); this implementation spends the same byte budgets on its candidate scratch and
 * its composited-hit arena. device = HIP device ordinal the buffers live on. */
int egr_create(egr_context **ctx, int device, int width, int height, int64_t ppll_forward_size, int64_t ppll_backward_size);
void egr_destroy(egr_context *ctx);

/* params_on_host.{camera,config,framebuffer,metadata,stats} = holder->reify() (raytracer.cpp:61-68) */
int egr_bind(egr_context *ctx, const egr_camera *camera, const egr_config *config, const egr_framebuffer *framebuffer,
             const egr_metadata *metadata, const egr_stats *stats);

/* Raytracer::resize re-reify + upload of Params.gaussians (raytracer.cpp:112-120) */
int egr_set_gaussians(egr_context *ctx, const egr_gaussians *gaussians);

/* Raytracer::rebuild_bvh (raytracer.cpp:102-110; optix/bvh_wrapper.h:24-30,118-157): instance transforms from
 * the current parameters + full LBVH build. Synchronises the stream (the reference's build also does). */
int egr_rebuild_bvh(egr_context *ctx, void *hip_stream); /* fails for count >= 2^26 (67M): record indices are packed into 26 bits */

/* Raytracer::update_bvh (raytracer.cpp:100; optix/bvh_wrapper.h:32-59): re-snapshot instance transforms and
 * refit the existing tree. Asynchronous; reads alpha_threshold/exp_power/global_scale_factor on the device
 * (the reference does three blocking .item() reads, bvh_wrapper.h:38-40). */
int egr_update_bvh(egr_context *ctx, void *hip_stream);
/* The same with flags. EGR_UPDATE_FUSE_LIVE: the pass over the cloud that snapshots the transforms also writes the LIVE per-gaussian
 * records (activated appearance, opacity, sigma: what the reference's read_* helpers fetch inside the launch, utils/helpers.cu:10-33),
 * and the NEXT egr_raytrace does not repeat that pass. The caller promises that the parameter tensors and the config scalars the live
 * records depend on (alpha_threshold, exp_power) are not written between this call and that egr_raytrace (the reference's caller, gaussian_raytracer.py:139-142, calls the two back to back); every later launch
 * reads the live parameters again as usual. One pass of ~130 B per gaussian less per training iteration. */
#define EGR_UPDATE_FUSE_LIVE 1u
int egr_update_bvh_ex(egr_context *ctx, unsigned flags, void *hip_stream);
/* Export and refit in one pass (an additive symbol of library version 0.8): egr_update_bvh_ex(flags) for a caller whose current parameter values are in tensors
 * of its OWN. The pass over the cloud reads the eight parameter pointers of `src` (count rows of the bound gaussians, fp32, contiguous, device memory, rotation
 * 16-byte aligned; nothing else of `src` is read), stores what it read to the bound parameter tensors - they then hold what eight copies from `src` would leave,
 * bit for bit - and snapshots the transforms from the same values. A pointer of `src` that equals the bound one is not stored. `flags` as for egr_update_bvh_ex.
 * With a count of 0 the pointers are not read and may be NULL. A NULL src or parameter pointer, a misaligned rotation and an unknown flag return non-zero with an egr_last_error message before anything is launched. */
int egr_update_bvh_from(egr_context *ctx, const egr_gaussians *src, unsigned flags, void *hip_stream);

/* Raytracer::raytrace (raytracer.cpp:81-94): metadata update, stats reset, one launch of the whole
 * forward (+ backward when grads_enabled) path = __raygen__rg (shaders.cu:77-173), then
 * accumulated_sample_count += 1 when accumulate_samples. grads_enabled is what
 * torch::autograd::GradMode::is_enabled() returned in the caller (metadata.h:29). Asynchronous. */
int egr_raytrace(egr_context *ctx, int grads_enabled, void *hip_stream);
/* Gather and import in one pass (an additive symbol of library version 0.8): egr_raytrace(grads_enabled = 1) for a caller that adds the bound gradient tensors
 * to gradient tensors of its own after every launch. Only the eight dL_d* pointers of `dst` are read (count rows each, fp32, contiguous, device memory). The
 * launch's last kernel leaves in the bound tensors what egr_raytrace leaves there and adds every value it leaves - the ACCUMULATED one, also of gaussians the
 * launch did not hit - to dst's: the result of `dst.dL_dX += bound.dL_dX` for the eight tensors after the launch, bit for bit. total_weight is not imported.
 * With a count of 0 the pointers are not read and may be NULL. Refused (non-zero, egr_last_error, nothing launched): a NULL dst or dL_d* pointer, a dL_d* pointer that is the bound one, and a context with
 * egr_set_grad_overwrite on (a partition reduces its per-launch buffer before anything is imported). */
int egr_raytrace_import(egr_context *ctx, const egr_gaussians *dst, void *hip_stream);
/* Targets read in place (an additive symbol of library version 0.8): egr_raytrace with, optionally, the import of egr_raytrace_import (dst as there; NULL: no
 * import) and, optionally, the six target images of the view read where the caller keeps them (targets; NULL: the launch reads framebuffer.target_* like
 * egr_raytrace). `targets` is an array of six DEVICE pointers in the order of egr_set_targets_chw - diffuse, specular, depth, normal, roughness, f0 - each a
 * contiguous channel-major fp32 image [C][H][W] of the context's size with C = 3, 3, 1, 3, 1, 3; a NULL entry = the target is absent and reads zero (what
 * egr_set_targets_chw writes for it). The array itself is read during the call; the images must stay valid and unmodified until the launch has completed on
 * its stream. Such a launch neither reads nor writes framebuffer.target_* and launches nothing for the targets: it leaves what egr_set_targets_chw with the
 * same six pointers followed by egr_raytrace(1) / egr_raytrace_import leaves, except in framebuffer.target_*. A context of a partition reads the pixels of
 * its own tiles only. Refused (non-zero, egr_last_error, nothing launched): targets or dst with grads_enabled == 0, and what egr_raytrace_import refuses in dst. */
int egr_raytrace_targets(egr_context *ctx, int grads_enabled, const egr_gaussians *dst, const float *const *targets, void *hip_stream);

/* Camera upload (replaces the caller's ten tiny tensor kernels of renderer/gaussian_raytracer.py:94-100, which stay valid): rotation_c2w_dataset =
 * the dataset's camera-to-world rotation `viewpoint_camera.R` (row-major 3x3 fp32), camera_center = `viewpoint_camera.camera_center` (3 fp32), both DEVICE
 * pointers. ONE launch writes the bound camera struct: rotation_c2w = -R with column 0 negated back (the reference's Blender convention), its transpose,
 * the origin, and the three scalars. Asynchronous on the stream. */
int egr_set_camera_from_dataset(egr_context *ctx, const float *rotation_c2w_dataset, const float *camera_center, float vertical_fov_radians, float znear,
                                float zfar, void *hip_stream);
/* The same with flags: EGR_CAMERA_ROTATION_ON_HOST / EGR_CAMERA_CENTER_ON_HOST say that the pointer is HOST memory (a dataset keeps R as a numpy array). Such
 * values are read before the call returns and travel to the ONE launch by value: no upload, no wait for the stream, and the caller's array is free again at
 * once. The bound camera struct holds the same bits as after the device-pointer call. Unknown flags are refused (non-zero, egr_last_error). */
#define EGR_CAMERA_ROTATION_ON_HOST 1u
#define EGR_CAMERA_CENTER_ON_HOST 2u
int egr_set_camera_from_dataset_ex(egr_context *ctx, const float *rotation_c2w_dataset, const float *camera_center, float vertical_fov_radians, float znear,
                                   float zfar, unsigned flags, void *hip_stream);

/* Target upload (replaces the caller's six `framebuffer.target_*.copy_(image.moveaxis(0, -1))` of renderer/gaussian_raytracer.py:109-137, which
 * stay valid): device pointers to channel-major fp32 images ([3][H][W] diffuse, specular, normal, f0; [1][H][W] depth, roughness), NULL = the
 * target is absent and reads zero (the reference zeroes the buffer). ONE launch writes the framebuffer's pixel-major target buffers for the pixels
 * of THIS context's partition only - the only target pixels its launches read; the target_* buffers OUTSIDE the partition's tiles keep whatever they held
 * (undefined for a caller that reads them; a context that is switched to another partition or to the whole image uploads its targets again). Asynchronous on the stream. */
int egr_set_targets_chw(egr_context *ctx, const float *diffuse, const float *specular, const float *depth, const float *normal, const float *roughness,
                        const float *f0, void *hip_stream);

/* Raytracer::denoise (raytracer.cpp:96; optix/denoiser_wrapper.h:42-105: HDR image output_final + normal guide output_normal
 * -> output_denoised). The OptiX AI denoiser is a closed network; the stand-in is an edge-avoiding a-trous wavelet filter with
 * the same inputs and output (csrc/denoise.hip; parity with OptiX is unpinned). Env EGR_DENOISE=0 at creation: plain copy. */
int egr_denoise(egr_context *ctx, void *hip_stream);
/* Batched denoise on caller buffers (not in the reference; an additive symbol of library version 0.8, egr_version() is unchanged): the filter of
 * egr_denoise - five a-trous passes with holes 1 to 16, the same weights - on V images of the context's size, all views of a pass in ONE launch (5 launches
 * for V views). View v reads final + v * H*W*3 and the guide normal + v * normal_view_stride (in floats: 3*H*W*3 for egr_view_batch.normal, whose step 0 is
 * the guide; H*W*3 for a packed [V][H][W][3] array) and writes denoised + v * H*W*3. Per pixel the arithmetic is that of egr_denoise, so a view's result is
 * bit-equal to egr_denoise on a framebuffer that holds the same final / normal. The framebuffer is not touched (output_denoised included). Honours the
 * context's denoise mode (env EGR_DENOISE=0 at creation: plain copy). The ping-pong memory (one image per view) is the context's own: grown on demand, freed
 * with the context, counted in egr_counters.device_bytes. Refused BEFORE any HIP call, with an egr_last_error message: num_views == 0 (or > 65535), a NULL
 * pointer, final or normal overlapping denoised (the filter runs out of place), a stride smaller than one image. Asynchronous on the stream. */
int egr_denoise_views(egr_context *ctx, uint32_t num_views, const float *final /* [V][H][W][3] */,
                      const float *normal /* view v's guide = normal + v * normal_view_stride, [H][W][3] */,
                      size_t normal_view_stride /* in floats; 3*H*W*3 for render_views' normal buffer: the guide is step 0 */,
                      float *denoised /* [V][H][W][3] */, void *hip_stream);

/* Multi-GPU image partition (not in the reference): this context only traces the 16x16-pixel macro tiles it owns;
 * default rank 0 of 1 = whole image. Ownership: the macro tiles (index m = my * ceil(width / 16) + mx) are sorted along a Z-curve over
 * (mx, my); the tile at position i of that order belongs to rank (i + i / world_size) % world_size - every run of world_size
 * consecutive positions (a compact 2-D block of the image) holds each rank once, rotated by the block index. Hosts that need the map
 * (image gathers, pixel masks) ask egr_tile_owner instead of re-implementing it. */
int egr_set_partition(egr_context *ctx, int rank, int world_size);
/* The rank that owns macro tile `tile_index` (= my * ceil(width / 16) + mx) of a width x height image cut `world_size` ways; -1 for
 * arguments out of range. Pure host function (no context, no device). */
int egr_tile_owner(int width, int height, int world_size, int tile_index);

/* Per-launch gradient buffers (not in the reference; the multi-GPU exchange step). The reference's launch ADDS to the
 * gradient tensors (atomicAdd, backward_pass.cu:210-220) and so does this library by default. With enable != 0 the dL_d* / total_weight
 * pointers of egr_set_gaussians are taken as a PER-LAUNCH buffer: the first grad launch after the caller has consumed the buffer
 * (egr_grad_delta_consumed; also right after this call) STORES its sums there (rows no ray touched read 0), so the caller can all-reduce
 * the buffer over the ranks and add it to its persistent gradients without clearing it in between (one write pass over [22N] instead of
 * a read-modify-write, and no memset per iteration). A grad launch that finds the buffer NOT consumed yet - two launches before one
 * fold: multi-view accumulation, a caller that raised between launch and fold - ADDS to it like the default path, so no launch's
 * gradients or total_weight are ever dropped. */
int egr_set_grad_overwrite(egr_context *ctx, int enable);
/* The caller has folded the per-launch buffer into its persistent gradients (after the all-reduce): the next grad launch stores again.
 * REQUIRED after every fold (changed in library version 0.6: until then every launch stored): a host that all-reduces the buffer in place and
 * never calls this has every later launch ADD to the already rank-summed values, and the next reduce sums those again. */
int egr_grad_delta_consumed(egr_context *ctx);

/* Exact statistics (not in the reference). By default the tree bounds each Gaussian's ELLIPSOID and the walk only has to find the
 * instances whose response point can be accepted, so stats.num_traversed_per_pixel and egr_counters.candidates count the candidates
 * whose response point lies INSIDE the ellipsoid (|u|^2 <= 1, shaders.cu:48) on the ray's segment - accepted ones plus the back-face /
 * behind-the-origin rejections among them: a property of ray and gaussian, whatever the walk, and pixel by pixel a SUBSET of the reference's
 * intersection-program invocations (every instance whose cube the segment overlaps, shaders.cu:33; about half of them on surfel
 * clouds); every other output is unaffected.
 * With enable != 0 the next egr_update_bvh / egr_rebuild_bvh bounds the instance CUBES (what OptiX's TLAS holds) and every launch
 * counts exactly the instances whose unit cube the ray segment overlaps: the reference's number, at a slower walk. egr_raytrace
 * fails if the flag changed since the last refit. Used by tests and by bench.py to measure Hc. */
int egr_set_exact_stats(egr_context *ctx, int enable);

/* Kept for existing callers (library version 0.7 removed strands: every launch runs all of this context's tiles on the caller's
 * stream). Accepts only 1 and returns 0 for it; returns 1 for any other value. */
int egr_set_strands(egr_context *ctx, int strands);

/* Task shape (not in the reference): pixels one wave traces together. 64 = 8x8 (default), 32 = 8x4, 16 = 4x4; 0 = automatic (64, or
 * 32 for a rank of a partition with fewer than two 8x8 tiles per resident wave when team help is off). Also settable at creation with env
 * EGR_RAYS_PER_TASK. The ORDER of exactly tied hits of a bounce ray depends on the shape (deviation (a)); parity tests
 * that trace single macro tiles through egr_set_partition pin the shape of the run they compare with. Returns 1 for other values. */
int egr_set_rays_per_task(egr_context *ctx, int rays_per_task);

/* Team help (not in the reference): the forward chain's workgroups are teams of waves with a shared LDS; with help on, a wave that has no tile
 * left (or waits for its own helpers) walks (ray, node) pairs that a team mate with a long pair stack puts on offer - several waves on one heavy
 * tile: the tail of every launch, and most of the launch of a rank of a multi-GPU partition. Help changes the ORDER in which a ray's candidates
 * enter its list, never the set; that order reaches an output only where two candidates of a ray have EXACTLY the same distance (the depth
 * selection orders by (t, list index); the total transmittance is an fp64 product rounded once): without exact ties the images of a run with
 * help equal those of a run without bit for bit (tests/test_hip_parity.py), with them the tied hits may composite in another order from run to
 * run (deviation (a); upstream the order of tied hits is its PPLL's insertion order, which is timing too). 1 = on (default since
 * round 5: whole image -6 % / -3 % forward chain), 0 = off (launches reproducible bit for bit), -1 = on only for a rank of a partition with fewer than
 * two 8x8 tiles per wave slot; also env EGR_TEAM_HELP (0 / 1) at creation. Returns 1 for other values. (1 also selects the backward chain's team build, which an under-filled rank of a partition gets in any
 * case: its waves without tiles take batches of their team mates' bounce hits - gradients are atomic adds, no result depends on it.) */
int egr_set_team_help(egr_context *ctx, int on);

/* Batched no-grad render (not in the reference): V views x S samples per view in as few launches as the ray state allows.
 * A batch is V views times S samples per view; frame f = v * S + s is sample s of view v. For each view v the outputs equal, bit for bit
 * when team help is off, what this library leaves for: reset the accumulators, then S times (camera of view v, egr_raytrace with
 * grads_enabled = 0 and accumulate_samples = (S > 1)), then read the framebuffer outputs. In detail:
 *   - seeds: metadata.total_num_calls advances by V * S; frame f draws its seeds from (value before the batch) + f + 1, as the f-th of the
 *     sequential launches would, so a launch after the batch sees the same counter as after V * S single launches;
 *   - accumulation: a view's samples are added into fp32 running sums in sample order and divided by S (k_finish's accumulation); for S == 1
 *     the value is written undivided (a non-accumulating launch);
 *   - config: the config scalars are read on the device as in any launch; accumulate_samples is ignored (S decides);
 *   - outputs: the caller's per-view buffers below (NULL: not written). The framebuffer's output_*, accumulated_* and accumulated_sample_count
 *     are NOT touched by a batch;
 *   - stats.* and metadata.random_seeds hold what the LAST frame's sequential launch would leave; metadata.grads_enabled is set to 0;
 *   - egr_counters: rays / candidates / composited / accepted are sums over the batch's frames, status is ORed over them, lifetime_launches
 *     grows by V * S;
 *   - the BVH gates (stale tree, changed exact-stats flag), the partition (a rank traces its own tiles of every frame; other pixels of the
 *     outputs are left untouched), the debug pixel mask, team help and the exact-statistics build behave as for egr_raytrace.
 * The camera arrays use the dataset convention of egr_set_camera_from_dataset, one entry per view. */
typedef struct egr_view_batch {
    uint32_t num_views;               /* V >= 1 */
    uint32_t samples_per_view;        /* S >= 1 */
    const float *rotation_c2w_dataset; /* [V][3][3] device pointer: the dataset's camera-to-world rotations (viewpoint_camera.R) */
    const float *camera_center;       /* [V][3] device pointer */
    const float *vertical_fov_radians; /* [V] device pointer */
    float znear;
    float zfar;
    float *final;                     /* [V][H][W][3] required */
    float *rgb;                       /* [V][3][H][W][3] per bounce step, or NULL */
    float *depth;                     /* [V][3][H][W][1] or NULL */
    float *normal;                    /* [V][3][H][W][3] or NULL */
    float *f0;                        /* [V][3][H][W][3] or NULL */
    float *roughness;                 /* [V][3][H][W][1] or NULL */
} egr_view_batch;
/* Asynchronous on the stream. A batch runs in chunks of min(V * S, batch frames) frames (egr_set_batch_frames); the ray state of a chunk
 * (444 B per pixel and frame) is allocated by the first call and counted in egr_counters.device_bytes from then on. Wrong arguments (V == 0,
 * S == 0, a NULL final or a NULL camera array) return non-zero with an egr_last_error message and write nothing. */
int egr_render_views(egr_context *ctx, const egr_view_batch *batch, void *hip_stream);
/* Frames per launch of egr_render_views and egr_train_views (default 8; env EGR_BATCH_FRAMES at creation). Returns 1 for values < 1. */
int egr_set_batch_frames(egr_context *ctx, int frames);

/* Multi-view training launch (not in the reference; an additive symbol of library version 0.8, egr_version() is unchanged): the gradients of V views,
 * one sample each, in as few launches as the ray state allows. After the call the context is in the state V sequential egr_raytrace(grads_enabled = 1)
 * calls leave, where call v has camera v and targets v bound. In detail:
 *   - gradients: the dL_d* tensors and total_weight gain the sum over the views (equal up to the order of the float atomic adds). With
 *     egr_set_grad_overwrite the whole batch is ONE grad launch: the first after egr_grad_delta_consumed stores, any later one adds;
 *   - seeds: metadata.total_num_calls advances by V; view v draws its seeds from (value before the call) + v + 1, as in egr_render_views;
 *   - stats.* and metadata.random_seeds hold what the LAST view's launch would leave (bit for bit when team help is off); grads_enabled is set to 1;
 *   - egr_counters: rays / candidates / composited / accepted / bucket_records are sums over the views, status is ORed over them,
 *     lifetime_launches grows by V; arena_blocks_used is what the last chunk took of the batch arena (see below);
 *   - NOT touched: the framebuffer (outputs - a grad launch writes none, shaders.cu:155-169 -, accumulators, accumulated_sample_count: accumulate_samples
 *     is ignored as in egr_render_views - and the target buffers) and the bound camera;
 *   - the BVH gates (stale tree, changed exact-stats flag), the partition (a rank traces its own tiles of every view), the debug pixel mask, team help
 *     (both chains' team builds are chosen as for egr_raytrace) and the exact-statistics build behave as for egr_raytrace;
 *   - debug exports: a batch traces into buffers of its own, so egr_debug_get_step_hits and egr_debug_get_hit_sequence_hash keep describing the
 *     last egr_raytrace with grads_enabled.
 * Targets are channel-major like egr_set_targets_chw's, one image per view; NULL = the target is absent and reads zero (the reference zeroes the buffer).
 * The camera arrays use the dataset convention of egr_set_camera_from_dataset. */
typedef struct egr_train_batch {
    uint32_t num_views;               /* V >= 1 */
    const float *rotation_c2w_dataset; /* [V][3][3] device pointer: the dataset's camera-to-world rotations (viewpoint_camera.R) */
    const float *camera_center;       /* [V][3] device pointer */
    const float *vertical_fov_radians; /* [V] device pointer */
    float znear;
    float zfar;
    const float *target_diffuse;      /* [V][3][H][W] or NULL */
    const float *target_specular;     /* [V][3][H][W] or NULL */
    const float *target_depth;        /* [V][1][H][W] or NULL */
    const float *target_normal;       /* [V][3][H][W] or NULL */
    const float *target_roughness;    /* [V][1][H][W] or NULL */
    const float *target_f0;           /* [V][3][H][W] or NULL */
} egr_train_batch;
/* Asynchronous on the stream. Runs in chunks of min(V, batch frames) views (egr_set_batch_frames). The first call allocates, counted in
 * egr_counters.device_bytes from then on: the ray state of a chunk (shared with egr_render_views: 444 B per pixel and frame), a composited-hit arena of
 * (batch frames) x the single-launch arena (so a view whose hits fit one egr_raytrace also fits inside a chunk; an overflow is still flagged,
 * EGR_STATUS_HIT_ARENA_OVERFLOW, never silent) and 80 B per 8x8 tile and frame of per-task tables. Wrong arguments (V == 0, a NULL camera array), a stale
 * tree and the exact-stats gate return non-zero with an egr_last_error message and write nothing. */
int egr_train_views(egr_context *ctx, const egr_train_batch *batch, void *hip_stream);
/* The same with the import of egr_raytrace_import in the batch's one gather (dst as there; NULL: egr_train_views). */
int egr_train_views_import(egr_context *ctx, const egr_train_batch *batch, const egr_gaussians *dst, void *hip_stream);

/* Synchronises the stream and returns the work counters / status of the most recent egr_raytrace.
 * ABI: egr_counters only ever GROWS AT ITS END (version string of egr_version() bumps with it). egr_get_counters writes
 * sizeof(egr_counters) of THIS header; a host compiled against an older header passes its own sizeof to egr_get_counters_ex, which
 * writes min(out_bytes, sizeof(egr_counters)) bytes - never more than the caller's struct holds. */
int egr_get_counters(egr_context *ctx, egr_counters *out, void *hip_stream);
int egr_get_counters_ex(egr_context *ctx, void *out, size_t out_bytes, void *hip_stream);
int egr_reset_lifetime_counters(egr_context *ctx, void *hip_stream);

/* Wall-clock of the last egr_raytrace / egr_update_bvh on the GPU (HIP events recorded on the launch stream
 * when timing is enabled). Returns milliseconds, <0 if not available. Synchronises on the end event. */
int egr_enable_timing(egr_context *ctx, int enable);
float egr_last_raytrace_ms(egr_context *ctx);
float egr_last_update_bvh_ms(egr_context *ctx);
/* duration of the individual kernels of the last egr_raytrace, in launch order; returns count written */
int egr_last_kernel_ms(egr_context *ctx, float *ms, const char **names, int max_entries);

/* Copies the snapshot instance records for parity tests: M[N*12], W[N*12] (3x4 row-major), aabb[N*6]
 * (lo xyz, hi xyz; invisible instances have lo > hi). Host pointers; synchronises. */
int egr_debug_get_instances(egr_context *ctx, float *M, float *W, float *aabb, void *hip_stream);
/* Debug: the 64-B backward record of every gaussian, by gaussian id, on the host: out[n][4][4] = rows 0-2 (row of M as of the last update / rebuild, exp(scale_a)
 * as of the last grad launch or update), row 3 the raw quaternion (likewise). n = the count the tree was last built for (egr_debug_get_bvh_state: info[3]).
 * Synchronises the stream. */
int egr_debug_get_backward_records(egr_context *ctx, float *out, void *hip_stream);
/* Composited hits per pixel and bounce step of the last egr_raytrace with grads_enabled (what backward_pass.cu:38-45 calls
 * num_hits[step]; the reference keeps it in registers, stats.num_accumulated_per_pixel only shows the last step): host_out =
 * int32 [EGR_NUM_STEPS][H*W], host pointer; pixels outside this context's partition read 0. Parity tests use it to LIST the
 * pixels whose bounce rays met a different number of hits than the CPU oracle's. Synchronises. */
int egr_debug_get_step_hits(egr_context *ctx, int32_t *host_out, void *hip_stream);
/* The ORDERED sequence of gaussians every pixel composited on every step of the last egr_raytrace with grads_enabled, as a hash: host_out = uint64
 * [EGR_NUM_STEPS][H*W] (host pointer), sum_i (id_i + 1) B^i mod 2^64 over the composite index i (front to back), B = 0x9E3779B97F4A7C15; 0 = no hit, and for
 * pixels outside this context's partition. The CPU oracle reports the same number (oracle/egr_oracle.cpp: Outputs::hit_sequence_hash): a pixel composited the
 * same hits in the same order on both sides iff the hashes agree - the definition of a "clean" pixel in the at-size gradient check. Synchronises. */
int egr_debug_get_hit_sequence_hash(egr_context *ctx, uint64_t *host_out, void *hip_stream);
/* Pixel mask for parity tests: device_mask = uint8 [H*W] in DEVICE memory (caller-owned, must outlive the launches that use it), or NULL
 * to clear. A pixel whose mask byte is 0 is treated like a pixel outside the image by every kernel of a launch: no ray, no outputs written,
 * no statistics, no gradient contribution. The CPU oracle has the same hook (orc_set_pixel_mask), so both sides can trace exactly the pixels
 * whose per-step hit counts agree (tests/test_hip_configs.py: the at-size gradient check). Takes effect at the next egr_raytrace. */
int egr_debug_set_pixel_mask(egr_context *ctx, const uint8_t *device_mask);
/* Unit-test hook: the division and square root of the hot per-candidate / per-hit arithmetic (csrc/egr_device.hpp: the compiler's IEEE correction steps without
 * its range scaling). quot[i] = a[i] / b[i], root[i] = sqrt(a[i]) as THOSE functions compute them; device pointers, n elements each. ACCEPTED DOMAIN: the results
 * are the correctly rounded ones whenever 2^-100 <= |b| <= 2^100, |a / b| is a normal number or 0, and a is 0 or a normal number >= 2^-100 for the root
 * (tests/test_hip_parity.py holds them to `/` and sqrtf bit for bit over that domain); outside it - b = 0, b = inf, a = inf, denormal radicands - they return NaN
 * or a result that is off in the last bits where IEEE gives inf / 0 / a denormal: a degenerate gaussian (all-zero quaternion, |W d| out of range) then drops out of
 * a ray's list through the NaN comparisons instead of contributing an inf. Asynchronous on the stream. Context-free (CONTEXT-FREE FUNCTIONS below), but
 * without an error string: a test hook, it reports through its return value alone. */
int egr_debug_lean_arith(int device, const float *a, const float *b, float *quot, float *root, uint32_t n, void *hip_stream);
/* BVH self-check: every leaf box equals its instance box, every internal box is the union of its children,
 * every visible instance is reachable exactly once. Returns 0 if consistent. Host-side; synchronises. */
int egr_debug_check_bvh(egr_context *ctx, void *hip_stream);
/* State of the tree for tests of the refit (read-only; an additive symbol of library version 0.8, egr_version() is unchanged): frame = origin xyz and
 * scale xyz (cells per world unit) of the 16-bit quantisation frame the last rebuild fixed; info = {out_of_frame flag (1: some box of the last refit left the
 * frame and carries the -inf / +inf sentinel cells, so the walks run their sentinel decode), wide nodes, depth of the wide tree, gaussian count the tree was
 * built for}. Host pointers; synchronises. */
int egr_debug_get_bvh_state(egr_context *ctx, float frame[6], uint32_t info[4], void *hip_stream);
/* The tree the last rebuild produced (and the last refit re-boxed), stage by stage, for tests that restate the builder on the CPU (read-only; an additive
 * symbol like the one above). One stream synchronisation, then device-to-host copies only: no kernel runs. Every pointer is a host pointer and may be
 * NULL (that array is skipped). With n = info[3], nw = info[1] and depth = info[2] of egr_debug_get_bvh_state:
 *   keys        uint64 [n]         the 63-bit Morton keys in sorted order (x bit highest of each triple, 21 bits per axis)
 *   gid_of_pos  uint32 [n]         gaussian id at every sorted position (the sort's values); pos_of_gid uint32 [n] is its inverse
 *   left, right int32  [n - 1]     children of the binary (Karras) node i; ids: internal i -> i, leaf at sorted position j -> (n - 1) + j
 *   dp          float  [n - 1][16] the collapse's row of binary node i, raw: 0-2 box lo xyz, 3-5 box hi xyz, 6-12 T(i, 1..7); 13-15 unused, never written
 *   wnodes      uint32 [nw][8][4]  the wide nodes: per slot lo.x | lo.y << 16, lo.z | hi.x << 16, hi.y | hi.z << 16 (16-bit cells of the build frame),
 *                                  link (EGR_LEAF_FLAG | sorted position, child node index, or EGR_EMPTY_SLOT)
 *   bsph        float  [n][4]      bounding spheres in record order (sorted position): centre xyz, squared radius (< 0: unusable gaussian)
 *   level_start uint32 [depth + 1] wide nodes of level L are level_start[L] .. level_start[L + 1] - 1 (root = level 0)
 * left, right and dp are empty for n <= 1 (a single gaussian hangs under a root that no binary node stands for); for n = 0 everything but
 * level_start = {0} is empty. The unsorted keys are not kept: the collapse reuses their buffer. */
int egr_debug_get_tree(egr_context *ctx, uint64_t *keys, uint32_t *gid_of_pos, uint32_t *pos_of_gid, int32_t *left, int32_t *right, float *dp,
                       uint32_t *wnodes, float *bsph, uint32_t *level_start, void *hip_stream);

const char *egr_last_error(egr_context *ctx);
const char *egr_version(void);

/* ---- CONTEXT-FREE FUNCTIONS: everything below (and egr_debug_lean_arith above) takes `int device, ..., void *hip_stream` and no egr_context. They share:
 *   device      the HIP device of EVERY device pointer of the call and of hip_stream. It need not be the calling thread's current device, and the thread's
 *               current device is the same after the call as before it, on success and on failure. (The egr_context functions keep the same promise for
 *               their context's device.)
 *   validation  arguments are checked BEFORE any HIP call: a refused call has touched neither the device nor the runtime, and runs on a machine without a GPU.
 *               Where a call must be out of place, a NULL or empty range touches nothing.
 *   errors      a non-zero return; the module's egr_<module>_last_error() then holds "libegr_hip: <function>: <why>" - the text of the failed check or the
 *               HIP error string - per module (a failure in one never shows in another's) and per thread. The pointer is valid until the thread's next
 *               failure in that module.
 *   launches    asynchronous on hip_stream unless the function says that it synchronises. */

/* ---- `simple_knn._C.distCUDA2` (editable_gauss_refl/scene/gaussian_model.py:17, called at :197-201 and
 * :246-250 to initialise the scales). out[i] = mean of the squared distances from point i to its 3 nearest OTHER points
 * (exact; duplicates count with distance 0). points_xyz = [n][3] fp32, out = [n] fp32, both device pointers. Synchronises the
 * stream before returning (it frees its temporaries). Returns 0 on success; egr_knn_last_error() describes a failure. */
int egr_knn_mean_dist2(int device, const float *points_xyz, uint32_t n, float *out_mean_dist2, void *hip_stream);
const char *egr_knn_last_error(void);

/* ---- the host step around every raytrace as ONE launch - gradient import
 * (renderer/gaussian_raytracer.py:50-58), scale decay (train.py:224-226), torch.optim.Adam(eps=1e-15) over the 8 parameter
 * groups (scene/gaussian_model.py:296-338), clamps (train.py:251-254), both zero_grads (train.py:248-249) and the parameter
 * export of the next iteration (gaussian_raytracer.py:36-48). All pointers are device pointers to [n][width] fp32 arrays. */
#define EGR_MAX_PARAM_GROUPS 8
typedef struct egr_param_group {
    float *param;       /* model parameter, updated in place                                              */
    float *grad;        /* model gradient: read, then zeroed (NULL: none)                                   */
    float *rt_param;    /* raytracer-side tensor refreshed with the new value (export; NULL: skip)          */
    float *rt_grad;     /* raytracer-side gradient dL_d*: added to the gradient, then zeroed (NULL: skip)   */
    float *exp_avg;     /* Adam first moment  (NULL together with exp_avg_sq: no optimizer update)          */
    float *exp_avg_sq;  /* Adam second moment                                                               */
    uint32_t width;     /* floats per gaussian                                                               */
    float lr;           /* this iteration's learning rate of the group                                      */
    float clamp_min, clamp_max; /* applied after the update (-INFINITY / +INFINITY: none)                    */
    float log_decay;    /* != 1: param = log(exp(param) * log_decay) before the update (scale decay)        */
    uint32_t step;      /* this group's own 1-based Adam step count; 0: use the `step` argument             */
} egr_param_group;
/* `step` is Adam's 1-based step count of THIS update (torch keeps one per parameter tensor: a group whose state was re-created
 * - gaussian_model.py replace_tensor_to_optimizer - passes its own count in egr_param_group.step). Asynchronous on the stream. Returns 0 on success.
 * A parameter that is or becomes NaN stays NaN in every group: the clamp propagates it like torch's clamp_ (it is neither clamp_min nor -INFINITY afterwards). */
int egr_fused_adam_step(int device, const egr_param_group *groups, int num_groups, uint32_t n, uint32_t step, double beta1, double beta2,
                        double eps, void *hip_stream);
const char *egr_fused_step_last_error(void);

/* ---- Fused prune (not in the reference as one call; additive symbols of library version 0.8, egr_version() is unchanged): what train.py:238-245,
 * scene/scene.py:88-105 (select_points_to_prune_near_cameras) and scene/gaussian_model.py:478-531 (prune_points / _prune_optimizer) do with one
 * nonzero + index pair per tensor, as a SELECT - criteria + stable scan - and ONE out-of-place GATHER over all arrays (csrc/prune.hip).
 *
 * egr_prune_select: row i of n is REMOVED if any of up to three optional criteria holds -
 *   weight        total_weight[i] / divisor < min_weight, evaluated in that form: IEEE fp32 division, strict `<` - a row whose quotient EQUALS
 *                 min_weight is kept, and so are NaN and +inf (-inf goes). total_weight == NULL skips the criterion.
 *   near a camera sqrt(dx^2 + dy^2 + dz^2) < cam_znear[c] in fp32 for ANY of num_cams cameras (d = points[i] - cam_centers[c]; strict: znear 0 removes
 *                 nothing, a point AT a centre goes when znear > 0). points = [n][3], cam_centers = [num_cams][3], cam_znear = [num_cams]; any number
 *                 of cameras (staged through LDS in chunks). points == NULL or num_cams == 0 skips the criterion.
 *   caller's mask remove_mask[i] != 0 (uint8 [n]). NULL skips it.
 * Outputs (device): src_index[0 .. count) = the KEPT row numbers in ASCENDING order - this order is what makes a gather equal to `tensor[keep]` - the rest
 * of src_index [n] is not written; count [1] = their number. workspace: EGR_PRUNE_WORKSPACE_BYTES(n) bytes of device memory, 8-byte aligned, owned by the
 * caller (the library allocates nothing) and free for reuse once the stream has passed the call.
 * Three launches, asynchronous on the stream; the stream order between them is the only dependency between workgroups (no workgroup ever waits for
 * another), and the result depends on nothing but the inputs: ranks that hold the same all-reduced total_weight select the same rows.
 * ONE synchronisation belongs to a prune, and it is the caller's: reading `count` back before sizing the gather's outputs.
 * Arguments are validated BEFORE any HIP call (NULL src_index / count, n > 2^26 - the tree's own limit -, cameras without their arrays, a missing or
 * misaligned workspace): returns non-zero, egr_prune_last_error() says why. n == 0 returns 0 and touches nothing: there are no rows, `count` is 0 by
 * definition and is not written.
 *
 * egr_prune_gather: dst[r * width + c] = src[src_index[r] * width + c] for r < count, for each of 1..EGR_MAX_PRUNE_ARRAYS table entries in one launch.
 * Elements are 4-byte words moved as bits (fp32 and int32 alike; NaN payloads survive). n = rows of every src (count <= n <= 2^26). OUT OF PLACE ONLY:
 * a dst range [count][width] that touches any src range [n][width] (src == dst included) or another dst is refused - stable compaction in place is not
 * safe in parallel. Also refused before any HIP call: a NULL table / src / dst / src_index, width 0, more than EGR_MAX_PRUNE_ARRAYS entries.
 * count == 0 returns 0 and launches nothing. Asynchronous on the stream. */
#define EGR_MAX_PRUNE_ARRAYS 32
#define EGR_PRUNE_ROWS_PER_WG 1024u /* rows one workgroup of the select covers: 16 wave ballots (8 bytes each) + 1 count (4 bytes) of workspace */
#define EGR_PRUNE_WORKSPACE_BYTES(n) ((((size_t)(n) + EGR_PRUNE_ROWS_PER_WG - 1) / EGR_PRUNE_ROWS_PER_WG) * (16 * 8 + 4))
typedef struct egr_prune_array {
    const void *src; /* [n][width] 4-byte elements                  */
    void *dst;       /* [count][width], must not overlap any src    */
    uint32_t width;  /* elements per row, >= 1                      */
} egr_prune_array;
int egr_prune_select(int device, uint32_t n, const float *total_weight, float divisor, float min_weight, const float *points,
                     const float *cam_centers, const float *cam_znear, uint32_t num_cams, const uint8_t *remove_mask, uint32_t *src_index,
                     uint32_t *count, void *workspace, void *hip_stream);
int egr_prune_gather(int device, const egr_prune_array *arrays, int num_arrays, uint32_t n, const uint32_t *src_index, uint32_t count,
                     void *hip_stream);
const char *egr_prune_last_error(void);

/* ---- Growing the cloud (not in the reference as one call; additive symbols of library version 0.8, egr_version() is unchanged): what
 * scene/gaussian_model.py:233-283 (add_farfield_points) does with torch.randn from the device generator and one torch.cat per tensor
 * (cat_tensors_to_optimizer, gaussian_model.py:533-585), as ONE launch that writes the candidates and ONE out-of-place APPEND over all arrays
 * (csrc/grow.hip). Context-free like egr_prune_*: the library allocates nothing, every call is asynchronous on the stream, and arguments are validated
 * BEFORE any HIP call (non-zero return, egr_grow_last_error() says why). The camera filter between the two calls is egr_prune_select +
 * egr_prune_gather on the candidates.
 *
 * egr_grow_sample: out_points [n][3] fp32; row r is candidate i = first + r and depends on (seed, i, radius, clamp) only - not on n, on the launch
 * shape, on earlier calls or on the device: ranks that pass the same arguments hold the same points, and a call may be split at any row.
 *   generator   Philox4x32-10 as published (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten
 *               rounds, counter words (i & 0xffffffff, i >> 32, 0, 0), key (seed & 0xffffffff, seed >> 32); it gives four words x0..x3.
 *   uniforms    u_k = ((x_k >> 9) + 0.5) * 2^-23: 24 significant bits, exact in fp32 and fp64, never 0 or 1.
 *   normals     Box-Muller in fp64, each rounded to fp32 once: z0 = sqrt(-2 ln u0) cos(2 pi u1), z1 = sqrt(-2 ln u0) sin(2 pi u1),
 *               z2 = sqrt(-2 ln u2) cos(2 pi u3)  (|z| < 5.7 on this grid).
 *   point       (x, y, z) = clamp(fp32(z_k), -clamp, +clamp) * radius in fp32. The reference: clamp 3, radius = cameras_extent * scene_extent_init_radius.
 * Refused: a NULL out_points, n > 2^26, first + n overflowing 64 bits, a non-finite or negative radius or clamp. n == 0 returns 0 and launches nothing.
 *
 * egr_grow_append: for each of 1..EGR_MAX_PRUNE_ARRAYS table entries, in one launch, dst [n + m][width] takes in rows < n the words of src [n][width]
 * and in rows >= n, by tail_kind, the words of tail [m][width] (EGR_GROW_TAIL_ROWS) or the word fill_bits (EGR_GROW_TAIL_FILL; tail is ignored).
 * Elements are 4-byte words moved as bits (fp32 and int32 alike; NaN payloads and -0.0 survive). OUT OF PLACE ONLY: a dst range [n + m][width] that
 * touches any src range, any tail range (src == dst included) or another dst is refused. Also refused: a NULL table or dst, src == NULL with n > 0,
 * tail == NULL with EGR_GROW_TAIL_ROWS and m > 0, width 0, an unknown tail_kind, more than EGR_MAX_PRUNE_ARRAYS entries, n + m > 2^26 (the tree's
 * limit). n == 0 is legal (the tail alone), m == 0 is legal (a copy); n + m == 0 returns 0 and launches nothing. */
#define EGR_GROW_TAIL_ROWS 0u /* rows >= n come from `tail`    */
#define EGR_GROW_TAIL_FILL 1u /* rows >= n are `fill_bits`     */
typedef struct egr_grow_array {
    const void *src;    /* [n][width] 4-byte elements; may be NULL when n == 0              */
    void *dst;          /* [n + m][width], must not overlap any src, tail or other dst      */
    const void *tail;   /* [m][width] (EGR_GROW_TAIL_ROWS); ignored for EGR_GROW_TAIL_FILL  */
    uint32_t width;     /* elements per row, >= 1                                           */
    uint32_t tail_kind; /* EGR_GROW_TAIL_ROWS or EGR_GROW_TAIL_FILL                         */
    uint32_t fill_bits; /* the word of every new element (EGR_GROW_TAIL_FILL)               */
} egr_grow_array;
int egr_grow_sample(int device, uint64_t first, uint32_t n, uint64_t seed, float radius, float clamp, float *out_points, void *hip_stream);
int egr_grow_append(int device, const egr_grow_array *arrays, int num_arrays, uint32_t n, uint32_t m, void *hip_stream);
const char *egr_grow_last_error(void);

/* ---- Scene editing (additive symbols of library version 0.8, egr_version() is unchanged): the reference's EditableGaussianModel
 * (scene/editable_gaussian_model.py: make_editable's selections and the seven getter overrides) as a SELECT that writes one bitmask per row and ONE
 * pass that applies every object's edit and writes the tracer's eight native arrays - edit and export in one launch (csrc/edit.hip).
 *
 * egr_edit_select: mask[i] bit k = row i belongs to objects[k], k < num_objects <= EGR_MAX_EDIT_OBJECTS, evaluated on the UNEDITED raw parameters:
 *   shape      box: box_min <= p <= box_max on all three axes, BOTH ENDS INCLUSIVE, exact fp32 comparisons. EGR_EDIT_SEL_CYLINDER: the ellipse inscribed
 *              in the box's xy extent - ((x - cx) / hx)^2 + ((y - cy) / hy)^2 <= 1 with c = 0.5 (min + max), h = 0.5 (max - min) in fp32 - and
 *              box_min.z <= z <= box_max.z. EGR_EDIT_SEL_EVERYTHING: every row, whatever else the object says.
 *   ranges     EGR_EDIT_SEL_RANGE_F0 / _ROUGHNESS / _DIFFUSE: the mean over the channels of the RAW parameter ((a + b + c) / 3 in fp32; one channel: the
 *              value itself) lies in [range_lo[j], range_hi[j]], both ends inclusive (j = 0 f0, 1 roughness, 2 diffuse). With EGR_EDIT_SEL_ZRANGE a row
 *              inside the sub-box [sub_min, box_max] (inclusive) is exempt from every range test. The reference also lists "metalness", an attribute its
 *              model does not have: there is no such range here.
 *   exclude    bit j set: rows inside the SHAPE (box or cylinder, not the ranges) of objects[j] are taken out.
 * `objects` is HOST memory (it travels as a kernel argument: no upload); xyz [n][3]; f0 [n][3], roughness [n][1], diffuse [n][3] may be NULL unless an
 * object has the matching range flag. One launch, asynchronous on the stream.
 *
 * egr_edit_apply: one pass over the n rows. Reads the eight raw arrays of `src` and `mask`, applies records[k] for every set bit k in ascending k -
 * EACH ON THE RESULT OF THE ONE BEFORE - and writes the eight arrays of `dst`. `records` is DEVICE memory ([num_records] egr_edit_record, staged in LDS).
 * A row whose mask has no bit below num_records set, and every group of a record whose flag is clear, is copied BIT FOR BIT (NaN payloads, -0, denormals).
 * Everything that depends on the edit alone is precomputed by the caller (editing.py does it in fp64): the kernel contains no trigonometry.
 *   EGR_EDIT_ROUGHNESS  r = clamp(roughness_mult * (base + roughness_shift), 0, 1), base = roughness_base with EGR_EDIT_ROUGHNESS_OVERRIDE, else r
 *                       (the caller stores override^2 and |shift|: the reference's copysign(shift, shift^2))
 *   EGR_EDIT_DIFFUSE / EGR_EDIT_F0 (egr_edit_colour): x = lerp(x, override_rgb, override_w) in torch's two-branch form; RGB -> HSV by the hexcone
 *                       formula (v = max, s = (max - min) / (max + 1e-8), sector of the FIRST channel that attains the max, achromatic hue 0, hue in
 *                       radians in [0, 2 pi)); h = (h + hue) mod 2 pi >= 0; s = clamp(s_mult * (s + s_shift), 0, 1); v = max(v_mult * (v + v_shift), 0);
 *                       HSV -> RGB by the six-sector table
 *   EGR_EDIT_TRANSFORM  p += translate; p = (p - centre) * scale + centre; p = R (p - centre) + centre; normal = R normal; scale_raw += log_scale;
 *                       rotation = q (x) (rotation / |rotation|), a Hamilton product in (w, x, y, z). R is row-major.
 *   EGR_EDIT_REMOVED    opacity = -1e8 (what the reference's destructive remove_object leaves; here the raw opacity is untouched)
 * IN PLACE OR DISJOINT: dst->X may be the very pointer src->X (the work is row-local) or must not touch it; any other overlap - a dst range with another
 * array's src, with another dst, with the mask or the records - is refused. One launch, asynchronous on the stream, no host synchronisation.
 *
 * Both validate BEFORE any HIP call (a NULL output or required input, more than EGR_MAX_EDIT_OBJECTS objects / records, n > 2^26 - the tree's own limit -,
 * a range flag without its array, partial overlap): non-zero is returned, egr_edit_last_error() says why, nothing was touched. n == 0 returns 0. */
#define EGR_MAX_EDIT_OBJECTS 32
#define EGR_EDIT_SEL_CYLINDER 1u
#define EGR_EDIT_SEL_EVERYTHING 2u
#define EGR_EDIT_SEL_RANGE_F0 4u
#define EGR_EDIT_SEL_RANGE_ROUGHNESS 8u
#define EGR_EDIT_SEL_RANGE_DIFFUSE 16u
#define EGR_EDIT_SEL_ZRANGE 32u
#define EGR_EDIT_ROUGHNESS 1u
#define EGR_EDIT_DIFFUSE 2u
#define EGR_EDIT_F0 4u
#define EGR_EDIT_TRANSFORM 8u
#define EGR_EDIT_REMOVED 16u
#define EGR_EDIT_ROUGHNESS_OVERRIDE 32u
typedef struct egr_edit_object {
    float box_min[3];
    float box_max[3];
    float sub_min[3];   /* EGR_EDIT_SEL_ZRANGE: lower corner of the exempt sub-box, box_min + (box_max - box_min) * zrange */
    float range_lo[3];  /* f0, roughness, diffuse */
    float range_hi[3];
    uint32_t flags;     /* EGR_EDIT_SEL_*                                       */
    uint32_t exclude;   /* bit j: subtract the shape of objects[j]              */
} egr_edit_object;
typedef struct egr_edit_colour {
    float override_rgb[3];
    float override_w;
    float hue;          /* pi * hue_shift, radians */
    float s_shift;
    float s_mult;
    float v_shift;
    float v_mult;
} egr_edit_colour;
typedef struct egr_edit_record {
    uint32_t flags;          /* EGR_EDIT_*: which groups are active          */
    float roughness_base;    /* override^2                                   */
    float roughness_shift;   /* |shift|                                      */
    float roughness_mult;
    egr_edit_colour diffuse;
    egr_edit_colour f0;
    float translate[3];
    float centre[3];         /* box centre + translate                       */
    float scale;             /* > 0                                          */
    float log_scale;         /* log(scale)                                   */
    float R[9];              /* Rodrigues' rotation, row-major               */
    float q[4];              /* the same rotation as a quaternion (w, x, y, z) */
} egr_edit_record;
typedef struct egr_edit_arrays { /* the export order of gaussian_raytracer.py:41-50 */
    float *scale;     /* [n][3] raw (log) */
    float *rotation;  /* [n][4] */
    float *mean;      /* [n][3] */
    float *opacity;   /* [n][1] raw */
    float *rgb;       /* [n][3] */
    float *normal;    /* [n][3] */
    float *roughness; /* [n][1] */
    float *f0;        /* [n][3] */
} egr_edit_arrays;
int egr_edit_select(int device, uint32_t n, const float *xyz, const float *f0, const float *roughness, const float *diffuse,
                    const egr_edit_object *objects, uint32_t num_objects, uint32_t *mask, void *hip_stream);
int egr_edit_apply(int device, uint32_t n, const egr_edit_arrays *src, const egr_edit_arrays *dst, const uint32_t *mask,
                   const egr_edit_record *records, uint32_t num_records, void *hip_stream);
const char *egr_edit_last_error(void);

/* ---- Per-object coverage of one view (an additive symbol of library version 0.8, egr_version() is unchanged): what the reference's viewer computes when
 * selection mode is entered (gaussian_viewer.py:292-321) - one image per object, each from a full render with the object's 0/1 indicator as the diffuse
 * colour - as ONE primary pass (trace.hip: k_forward_objects).
 *
 * Take the camera of the query and the primary ray the NEXT launch would trace at a pixel: seeds from metadata.total_num_calls + 1, jitter as the config
 * says, everything else from the context's current native tensors and tree. The ray's composited hits in order are i = 0 .. n-1 with weights
 * w_i = T - next_T (forward_pass.cu:108-109). For the j-th requested selection bit b = bits[j]:
 *     c    = sum in hit order, fp32, of w_i over the hits whose row has bit b set in row_bits   (plain adds, starting at +0)
 *     mask = c + rem * (c * inv_norm)      rem = T - full_T, inv_norm = 1 / max(1 - T, eps_forward_normalization): R4 of the primary step, unfused
 * which is, bit for bit, every channel of output_rgb[0] after egr_raytrace(grads_enabled = 0) on this context with accumulate_samples off and a model whose
 * rgb is (1, 1, 1) on the rows of the object and (0, 0, 0) elsewhere (relu keeps 0 and 1; fma(1, w, c) = c + w, fma(0, w, c) = c).
 *   masks  [K][H][W] fp32, K = num_bits, in the order of `bits`
 *   hit    [H][W] or NULL: bit j set iff masks[j] != 0 at the pixel (j is the OUTPUT index, not the selection bit; a NaN counts as non-zero)
 *   top    [H][W] or NULL: the output index with the largest mask under a strict `>` - ties go to the lowest index, a NaN never wins; -1 where hit == 0
 * The call is a QUERY: framebuffer outputs and accumulators, stats.*, metadata (random_seeds, total_num_calls, grads_enabled), gradients, total_weight, the
 * config and the hit arena of the last grad launch stay exactly as they were. No bounce is traced whatever num_bounces says. The per-launch egr_counters and
 * egr_last_kernel_ms describe this launch afterwards (lifetime_launches does not grow); a candidate-list overflow is reported in egr_counters.status as by
 * egr_render_views. The BVH gates, the partition (a rank traces its own tiles; other pixels are left untouched) and the debug pixel mask behave as for
 * egr_render_views. Single-wave workgroups always: team help is ignored. A context in exact-statistics mode (egr_set_exact_stats) is refused: only the
 * product tree has this kernel.
 * Validation BEFORE any HIP call: a NULL query, row_bits, bits, masks or camera array, num_bits == 0 or > EGR_MAX_EDIT_OBJECTS, a bit >= 32 or given twice,
 * an exact-statistics context: non-zero is returned, egr_last_error says why, nothing was touched. Asynchronous on the stream. */
typedef struct egr_object_mask_query {
    const float *rotation_c2w_dataset; /* [3][3] device pointer: the dataset's camera-to-world rotation, as egr_view_batch */
    const float *camera_center;        /* [3] device pointer */
    const float *vertical_fov_radians; /* [1] device pointer */
    float znear;
    float zfar;
    const uint32_t *row_bits;          /* device, [count the tree was built for]: membership word per gaussian id (egr_edit_select's mask) */
    const uint8_t *bits;               /* HOST, [num_bits]: distinct selection bits < 32, the output order */
    uint32_t num_bits;                 /* K, 1 .. EGR_MAX_EDIT_OBJECTS */
    float *masks;                      /* [K][H][W] required */
    uint32_t *hit;                     /* [H][W] or NULL */
    int32_t *top;                      /* [H][W] or NULL */
} egr_object_mask_query;
int egr_object_masks(egr_context *ctx, const egr_object_mask_query *q, void *hip_stream);

/* ---- Fused evaluation metrics (not in the reference as one call; additive symbols of library version 0.8, egr_version() is unchanged): what train.py:103-134
 * (training_report) and render.py:216-228 followed by metrics.py do per test view with six tone-mapping chains and three reductions, for V views in TWO
 * launches (csrc/eval.hip). Context-free like egr_prune_* and egr_edit_*.
 *
 * Three passes per view, prediction against ground truth, as the reference defines them:
 *   0 final     final [V][H][W][3] (the denoised or the plain final image)       against target_final    (original_image)
 *   1 diffuse   rgb[v][0], rgb = [V][3][H][W][3] per-step radiance               against target_diffuse  (diffuse_image)
 *   2 specular  rgb[v][1] + rgb[v][2] (one fp32 add: rgb[1:].sum(0))             against target_specular (specular_image)
 * The targets are channel-major [V][3][H][W]; a pass whose target is NULL is skipped and its results are NaN (rgb may be NULL when both of its passes are).
 * Both sides go through D(x) = clamp(tonemap(x), 0, 1) with the filmic tonemap of utils/tonemapping.py:1-5: nan_to_num(posinf = 999999999.9) - NaN becomes 0,
 * -inf the most negative float -, x (6.2 x + 0.5) / (x (6.2 x + 1.7) + 0.06), ** 1.3; every operation rounded to fp32 on its own, as torch evaluates it.
 * NaN propagates as in torch: NaN -> 0, +inf -> 1, but -inf, 3e38 (inf / inf) and every negative input (a negative quotient under the power) -> NaN, and the
 * clamp keeps a NaN.
 * Outputs (device):
 *   sse     [V][3 passes][3 channels] fp64: the sum over the pixels of ((double)D(pred) - (double)D(gt))^2. A NaN pixel makes its (view, pass, channel) sum NaN
 *           and no other.
 *   psnr    [V][3 passes][2] fp64, from sse on the device: [0] = the reference's number, psnr(a, b).mean() of utils/image_utils.py:19-21 on CHW images - a
 *           per-CHANNEL mse, 20 log10(1 / sqrt(mse_c)), then the mean over the three channels (its view(img.shape[0], -1) quirk kept; +inf for mse 0);
 *           [1] = 10 log10(1 / mse) over all three channels (torchmetrics' PeakSignalNoiseRatio(data_range = 1) of metrics.py) - on the unquantised floats,
 *           where metrics.py measures images after a PNG round trip.
 *   display [V][3 passes][2][3][H][W] fp32 or NULL: D(pred) and D(gt), channel-major - what save_image / format_image receive. A skipped pass is not written.
 * k_eval_partial (grid: EGR_EVAL_BLOCKS x V workgroups of 256 threads) keeps 9 fp64 sums per thread, reduces them over the wave and the workgroup and stores
 * one partial per workgroup in `workspace`; k_eval_finish (one workgroup per view) adds the partials in a fixed order. No float atomics, no workgroup waits
 * for another: the result depends on the inputs alone and is the same bit for bit on every run and rank.
 * workspace: EGR_EVAL_WORKSPACE_BYTES(V, H, W) bytes of device memory, 8-byte aligned, owned by the caller, free for reuse once the stream has passed the call.
 * Refused BEFORE any HIP call (non-zero, egr_eval_last_error() says why): V == 0 (or > 65535), H or W == 0, a NULL final / sse / psnr / workspace, a misaligned
 * workspace, a diffuse or specular target without rgb, an output that overlaps an input or another output. Asynchronous on the stream. */
#define EGR_EVAL_PIXELS_PER_WG 2048u /* pixels one workgroup of k_eval_partial covers: one partial (9 fp64 sums) of workspace */
#define EGR_EVAL_BLOCKS(H, W) (((size_t)(H) * (size_t)(W) + EGR_EVAL_PIXELS_PER_WG - 1) / EGR_EVAL_PIXELS_PER_WG)
#define EGR_EVAL_WORKSPACE_BYTES(V, H, W) ((size_t)(V) * EGR_EVAL_BLOCKS(H, W) * (9 * 8))
int egr_eval_metrics(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *target_final,
                     const float *target_diffuse, const float *target_specular, double *sse, double *psnr, float *display, void *workspace,
                     void *hip_stream);
const char *egr_eval_last_error(void);

/* ---- Fused SSIM (additive symbols of library version 0.8, egr_version() is unchanged): the structural similarity of utils/loss_utils.py:39-70 (ssim) for the
 * same three passes of V views in TWO launches (csrc/ssim.hip), in fp64. Context-free; errors are reported through egr_eval_last_error().
 *
 * Definition. p and g are display images: D(pred) and D(gt) with the D of egr_eval_metrics - the same device function, bit for bit - for egr_eval_ssim, and the
 * caller's images as they are for egr_ssim_images.
 *   window    w[k] = e[k] / sum(e), e[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10: computed and normalised on the host in fp64, applied separably (rows, then
 *             columns).
 *   padding   zero, "same" (loss_utils.py:51-60): a tap outside the image contributes nothing and is never read.
 *   moments   per pixel and channel, in fp64: mu1 = W*p, mu2 = W*g, s1 = W*(p p) - mu1^2, s2 = W*(g g) - mu2^2, s12 = W*(p g) - mu1 mu2.
 *   map       ((2 mu1 mu2 + C1) (2 s12 + C2)) / ((mu1^2 + mu2^2 + C1) (s1 + s2 + C2)), C1 = 1e-4, C2 = 9e-4. NaN propagates by plain arithmetic: the display
 *             clamp keeps a NaN, so a NaN pixel poisons its 11 x 11 neighbourhood and the means, as upstream.
 *   [0] full      the mean of the map over all 3 H W values: the reference's ssim(pred[None], gt[None]).
 *   [1] interior  the mean over the 3 (H - 10) (W - 10) values whose window lies wholly inside the image; NaN when H < 11 or W < 11. This is the region that
 *                 torchmetrics' StructuralSimilarityIndexMeasure averages (reflect pad, then crop the pad off); agreement with torchmetrics itself is UNPINNED
 *                 (it is not available where this library is tested).
 * Deviations from loss_utils.ssim, deliberate: the arithmetic is fp64 throughout (upstream: fp32, whose variance terms - a cancellation divided by C2 - are noise
 * in the fourth digit on flat regions), and the window is exactly separable and sums to 1 (upstream's 2-D window is an fp32 outer product of fp32 weights whose
 * sum is off by about 1e-8, which alone moves the result by 2.6e-6 on flat regions).
 * Outputs (device, fp64), both flavours from the same map:
 *   egr_eval_ssim     ssim_sum [V][3 passes][3 channels][2]: the sums of the map over all pixels and over the interior; ssim [V][3 passes][2]: the two means over
 *                     the three channels. A pass whose target is NULL (or that lacks rgb) is skipped and reports NaN, as in egr_eval_metrics.
 *   egr_ssim_images   pred, gt [V][3][H][W] channel-major fp32, one pass: ssim_sum [V][3 channels][2], ssim [V][2].
 * k_ssim_partial (grid: EGR_SSIM_BLOCKS x V workgroups of 256 threads) owns one EGR_SSIM_TILE^2 output tile: the tile and a 5-pixel halo of both sides in LDS,
 * the row pass and the column pass of the five moments in fp64, two sums per pass and channel reduced over the wave and the workgroup, one partial (18 fp64 sums)
 * per tile in `workspace`; k_ssim_finish (one workgroup per view) adds the partials in a fixed order. No float atomics, no workgroup waits for another: the
 * result depends on the inputs alone and is the same bit for bit on every run.
 * workspace: EGR_SSIM_WORKSPACE_BYTES(V, H, W) bytes of device memory, 8-byte aligned, owned by the caller, free for reuse once the stream has passed the call.
 * Refused BEFORE any HIP call (non-zero, egr_eval_last_error() says why): V == 0 (or > 65535), H or W == 0, a NULL final / pred / gt / ssim_sum / ssim /
 * workspace, a misaligned workspace, a diffuse or specular target without rgb, an output that overlaps an input or another output. Asynchronous on the stream. */
#define EGR_SSIM_TILE 32u /* output pixels per tile edge of k_ssim_partial: one partial (18 fp64 sums) of workspace per tile */
#define EGR_SSIM_BLOCKS(H, W) ((((size_t)(H) + EGR_SSIM_TILE - 1) / EGR_SSIM_TILE) * (((size_t)(W) + EGR_SSIM_TILE - 1) / EGR_SSIM_TILE))
#define EGR_SSIM_WORKSPACE_BYTES(V, H, W) ((size_t)(V) * EGR_SSIM_BLOCKS(H, W) * (18 * 8))
int egr_eval_ssim(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *target_final,
                  const float *target_diffuse, const float *target_specular, double *ssim_sum, double *ssim, void *workspace, void *hip_stream);
int egr_ssim_images(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *pred, const float *gt, double *ssim_sum, double *ssim,
                    void *workspace, void *hip_stream);

/* ---- Evaluation frames and exact 8-bit metrics (additive symbols of library version 0.8, egr_version() is unchanged): the fourteen images render.py:218-292
 * writes per test view - seven kinds, prediction and ground truth - as bytes ready for a PNG encoder, and the PSNR metrics.py measures on those bytes, for V views
 * in at most THREE launches (csrc/frames.hip). Context-free; errors are reported through egr_eval_last_error(). Every pointer of the arguments may be NULL
 * except frames, sse8, psnr8 and workspace.
 *
 * Seven kinds in fixed order; bit k of `kinds` selects kind k. Both sides of a kind go through the same value map before quantisation:
 *   0 render     final [V][H][W][3]                          against targets[0] (original)   D(x): the tone curve and clamp of egr_eval_metrics - the same device
 *   1 diffuse    rgb[v][0], rgb = [V][3][H][W][3]            against targets[1]              function, bit for bit
 *   2 specular   rgb[v][1] + rgb[v][2] (one fp32 add)        against targets[2]              D(x)
 *   3 depth      depth[v][0], depth = [V][3][H][W][1]        against targets[3], one channel EGR_FRAMES_DEPTH_MAX: x / hi (render.py:250-255);
 *                                                                                            EGR_FRAMES_DEPTH_MINMAX: (x - lo) / (hi - lo) (train.py:152).
 *                lo, hi = the minimum and maximum of THAT view's target depth (a NaN takes both ends, as torch's amin / amax); one correctly rounded division
 *   4 normal     normal[v][0], [V][3][H][W][3]               against targets[4]              x / 2 + 0.5: two fp32 roundings, no contraction
 *   5 roughness  roughness[v][0], [V][3][H][W][1]            against targets[5], one channel identity
 *   6 f0         f0[v][0], [V][3][H][W][3]                   against targets[6]              identity
 * The predictions are pixel-major, as egr_render_views writes them; the targets are channel-major fp32 [V][C][H][W]. One-channel kinds are replicated to three
 * channels (save_image / make_grid, repeat(3, 1, 1)).
 * The byte of a mapped value x, every fp32 operation rounded on its own:
 *   EGR_FRAMES_ROUND_SAVE    x * 255, + 0.5, clamp to [0, 255], truncate: torchvision's save_image. torchvision is not available where this library is tested:
 *                            the rule is stated here as a DEFINITION and is not pinned by a fixture.
 *   EGR_FRAMES_ROUND_TRUNC   clamp to [0, 1], * 255, truncate: format_image of render.py:303.
 *   NaN gives byte 0 - torch leaves that conversion unspecified, so this is a definition of this library -, +inf gives 255 and -inf gives 0.
 * Outputs (device):
 *   frames       uint8, interleaved RGB. EGR_FRAMES_SEPARATE: [V][7][2 sides][H][W][3], side 0 the prediction, side 1 the ground truth. EGR_FRAMES_SIDE_BY_SIDE:
 *                [V][7][H][2W][3], prediction left and ground truth right (the vs_target images of training_report, the cat(dim = 2) of the videos).
 *   sse8         [V][7][3] int64: the exact sum over the pixels of (pred_byte - gt_byte)^2 per channel. Integers: no summation order, no rounding.
 *   psnr8        [V][7][2] fp64, from sse8 on the device with mse = sse8 / (255^2 n): [0] the reference's per-channel-then-mean flavour, [1] 10 log10(1 / mse) over
 *                all three channels = PeakSignalNoiseRatio(data_range = 1) on to_tensor bytes, what metrics.py measures. An mse of 0 gives +inf.
 *   depth_range  [V][2] fp32 or NULL: (lo, hi), written when depth is selected and its target given.
 * Which slots are written: those of the selected kinds only. A selected kind writes its prediction side when its prediction is given and its ground-truth side
 * when its target is given; both sides of depth need targets[3], without it the depth kind writes no frame. A selected kind that lacks either side reports
 * sse8 = -1 and psnr8 = NaN. Slots of unselected kinds, and sides that are not written, keep what they hold.
 * k_frames_range (only when depth is written) stores one (min, max) per workgroup, k_frames_write (EGR_FRAMES_BLOCKS x V workgroups of 256 threads, one lane per
 * four consecutive pixels: 16-byte loads, 12 bytes stored per frame when H * W % 4 == 0 - side by side: and W % 4 == 0 -, element-wise accesses with the same
 * results otherwise) stores one partial of 21 integer sums per workgroup, k_frames_finish (one workgroup per view) adds them. No atomics, no memset.
 * workspace: EGR_FRAMES_WORKSPACE_BYTES(V, H, W) bytes of device memory, 8-byte aligned, owned by the caller, free for reuse once the stream has passed the call.
 * Refused BEFORE any HIP call (non-zero, egr_eval_last_error() says why): V == 0 (or > 65535), H or W == 0, an empty or unknown kinds / rounding / depth_mode /
 * layout, diffuse or specular selected with its target but without rgb, a NULL frames / sse8 / psnr8 / workspace, a misaligned workspace, an output that overlaps
 * an input or another output. Asynchronous on the stream. */
#define EGR_FRAMES_KINDS 7
#define EGR_FRAMES_ALL_KINDS 0x7Fu
#define EGR_FRAMES_ROUND_SAVE 0u
#define EGR_FRAMES_ROUND_TRUNC 1u
#define EGR_FRAMES_DEPTH_MAX 0u
#define EGR_FRAMES_DEPTH_MINMAX 1u
#define EGR_FRAMES_SEPARATE 0u
#define EGR_FRAMES_SIDE_BY_SIDE 1u
#define EGR_FRAMES_PIXELS_PER_WG 4096u /* pixels one workgroup of k_frames_write covers: one partial (21 uint32 sums) of workspace */
#define EGR_FRAMES_RANGE_BLOCKS 64u    /* depth-range partials (two uint32 keys each) per view */
#define EGR_FRAMES_BLOCKS(H, W) (((size_t)(H) * (size_t)(W) + EGR_FRAMES_PIXELS_PER_WG - 1) / EGR_FRAMES_PIXELS_PER_WG)
/* (rounded up to a multiple of 8: the partials are 84 bytes each) */
#define EGR_FRAMES_WORKSPACE_BYTES(V, H, W) ((((size_t)(V) * (EGR_FRAMES_RANGE_BLOCKS * 8 + EGR_FRAMES_BLOCKS(H, W) * (21 * 4))) + 7) & ~(size_t)7)
typedef struct egr_frames_args {
    uint32_t num_views, height, width;
    uint32_t kinds;      /* bit k selects kind k; EGR_FRAMES_ALL_KINDS */
    uint32_t rounding;   /* EGR_FRAMES_ROUND_* */
    uint32_t depth_mode; /* EGR_FRAMES_DEPTH_* */
    uint32_t layout;     /* EGR_FRAMES_SEPARATE or EGR_FRAMES_SIDE_BY_SIDE */
    uint32_t reserved;   /* 0 */
    const float *final, *rgb, *depth, *normal, *roughness, *f0; /* predictions, pixel-major */
    const float *targets[EGR_FRAMES_KINDS];                     /* channel-major, in kind order */
    uint8_t *frames;
    int64_t *sse8;
    double *psnr8;
    float *depth_range;
    void *workspace;
} egr_frames_args;
int egr_eval_frames(int device, const egr_frames_args *args, void *hip_stream);

/* ---- The dense-init cloud (additive symbols of library version 0.8, egr_version() is unchanged): what prepare_initial_ply.py:52-104 does on the CPU with every
 * pixel of every view in memory - unproject by the depth image, snap to a voxel of 1 / voxel_scale, average the diffuse colours per voxel, keep the voxels
 * seen by at least min_count pixels - as a streamed scatter-reduce into a hash table the caller owns (csrc/initcloud.hip). Context-free like egr_prune_*.
 *
 * The table is three device buffers: keys int64 [cap] (-1 = empty), acc int64 [cap][4] (count and three colour sums), status int64 [EGR_VOXEL_STATUS_WORDS].
 * cap is a power of two in EGR_VOXEL_MIN_CAPACITY..EGR_VOXEL_MAX_CAPACITY. The caller initialises it: keys to -1 (all bits set), acc and status to 0.
 *   key      (x + 2^20) << 42 | (y + 2^20) << 21 | (z + 2^20) for the signed voxel coordinate (x, y, z): non-negative, and its integer order is the
 *            lexicographic order of the signed triples, the order of torch.unique(dim=0).
 *   sums     FIXED POINT: every colour component is quantised once, q = llrint((double)c * 2^32), and added as an int64. Integer addition is associative:
 *            the content of the table depends on the SET of pixels alone - not on the order of the views, the chunking, the capacity, growth or timing. No
 *            float atomics. The mean is (float)((double)sum / ((double)count * 2^32)). The sums stay inside int64 while count * colour_max < 2^31.
 *   status   [0] occupied slots, [1] pixels added, [2] pixels dropped, [3] pixels (rehash: of records) that found no slot, and written by egr_voxel_extract:
 *            [4] the largest count of the table, [5] the number of rows that extraction selected. [6], [7] are reserved.
 *
 * egr_voxel_accumulate: V views of H x W pixels in one launch. Per view, computed by the caller in fp64: c2w [V][9] row-major = -R with column 0 negated
 * again, origin [V][3] = -R T, view_size [V] = tan(FovY / 2) - there is no trigonometry on the device. Per pixel (y, x), in fp64 with every operation rounded
 * on its own (utils/depth_utils.py:28-63): u = (x + 0.5) / W, v = (y + 0.5) / H, cam = ((W / H) view_size (2u - 1), view_size (1 - 2v), -1),
 * dir = cam c2w^T / |cam c2w^T|, pos = origin + dir * depth, coord = int32(rint(pos * voxel_scale)) - round half to even, as torch.round. depth is fp32
 * [V][H][W]. The colour is fp32 [V][H][W][3] as it is (`colour`), or uint8 [V][H][W][3] (`colour_u8`) looked up in the caller's 256-entry fp32
 * `colour_table` (untonemap(i / 255), prepare_initial_ply.py:72-73): exactly one of the two. positions_out (fp64 [V][H][W][3], NULL in production) receives pos.
 * A pixel is DROPPED and counted in status[2] when its depth, position or colour is not finite, a coordinate is outside [-2^20, 2^20) voxels, or a colour
 * component exceeds colour_max in magnitude (the reference would cast an undefined integer or average a NaN). Pixels of depth 0 are kept, as upstream.
 * Pixels that share a voxel within a workgroup's 16 x 16 tile are combined in LDS first; the global table then sees one 64-bit compare-and-swap on the key and
 * four 64-bit integer adds per distinct voxel of the tile. Probing is open addressing from a 64-bit mix of the key, BOUNDED by cap: a pixel that finds no slot
 * is counted in status[3] and otherwise ignored - the kernel never writes outside the table and never spins, whatever the caller does. A caller that keeps
 * occupied + pixels of the call <= cap / 2 never sees one. One launch, asynchronous on the stream.
 *
 * egr_voxel_rehash: inserts every occupied slot of the table (src_keys, src_acc, src_cap) into the table (keys, acc, cap) through the same claim-and-add;
 * adds the slots it claims to status[0] (the caller zeroes status[0] first when it reuses the old status). Out of place. One launch, asynchronous.
 *
 * egr_voxel_extract: the slots with count >= min_count are compacted into (key, slot) pairs (wave-aggregated append), sorted by key with
 * rocprim::radix_sort_pairs - the slot order depends on timing, the sorted order on the inputs alone - and written in one pass as n rows:
 *   coords int32 [n][3], points fp32 [n][3] = (float)coord / (float)voxel_scale (an IEEE fp32 division, as coords.float() / voxel_scale upstream),
 *   colors fp32 [n][3], counts int32 [n] (saturated at 2^31 - 1).
 * The outputs have room for max_rows rows (<= cap; the occupied slots are always enough). SYNCHRONISES the stream once, to read n and the largest count:
 * host_rows_and_largest[0] = n, [1] = the largest count (host memory). n > max_rows is an error and writes no row. The table is not modified.
 * workspace: egr_voxel_extract_workspace_bytes(device, max_rows) bytes of device memory, 16-byte aligned, owned by the caller: EGR_VOXEL_PAIR_BYTES(max_rows)
 * for the pairs plus what the sort asks for (the query makes HIP calls; it returns 0 on failure).
 *
 * The three validate BEFORE any HIP call (non-zero, egr_voxel_last_error() says why, nothing was touched): a NULL or misaligned table, a required pointer
 * that is NULL, cap not a power of two or out of range, V, H or W == 0, both or neither of colour and colour_u8, colour_u8 without its table, voxel_scale
 * <= 0 or not finite, colour_max outside (0, 2^30], max_rows == 0 or > cap, a short workspace, an output that overlaps an input or another output. */
#define EGR_VOXEL_STATUS_WORDS 8
#define EGR_VOXEL_MIN_CAPACITY 1024ull
#define EGR_VOXEL_MAX_CAPACITY (1ull << 31)
#define EGR_VOXEL_COORD_HALF_RANGE (1 << 20) /* coordinates are in [-2^20, 2^20) voxels: +-2621 m at the default voxel_scale of 400 */
#define EGR_VOXEL_PAIR_BYTES(max_rows) ((((size_t)(max_rows) * 24) + 15) & ~(size_t)15) /* two (int64 key, uint32 slot) arrays: unsorted and sorted */
int egr_voxel_accumulate(int device, int64_t *keys, int64_t *acc, int64_t *status, uint64_t cap, uint32_t num_views, uint32_t height, uint32_t width,
                         const double *c2w, const double *origin, const double *view_size, const float *depth, const float *colour, const uint8_t *colour_u8,
                         const float *colour_table, double voxel_scale, double colour_max, double *positions_out, void *hip_stream);
int egr_voxel_rehash(int device, int64_t *keys, int64_t *acc, int64_t *status, uint64_t cap, const int64_t *src_keys, const int64_t *src_acc, uint64_t src_cap,
                     void *hip_stream);
size_t egr_voxel_extract_workspace_bytes(int device, uint64_t max_rows);
int egr_voxel_extract(int device, const int64_t *keys, const int64_t *acc, int64_t *status, uint64_t cap, uint32_t min_count, double voxel_scale,
                      uint64_t max_rows, int32_t *coords, float *points, float *colors, int32_t *counts, uint64_t *host_rows_and_largest, void *workspace,
                      size_t workspace_bytes, void *hip_stream);
const char *egr_voxel_last_error(void);

/* ---- The training views, resident in fp16 (additive symbols of library version 0.8, egr_version() is unchanged): what scene/cameras.py:59-82
 * (Camera.__init__: the 8-bit conversions and seven .half() images per view), dataset/blender_dataset.py:112-129 (_resize_image_tensor) and
 * scene/scene.py:107-121 (autoadjust_zplanes: depth min / max per view) do per image with torch, as ONE launch per chunk of views into a store the caller
 * owns, and ONE launch that turns a batch of stored views into the fp32 arrays the batch calls read (csrc/viewset.hip). Context-free like egr_grow_*: the
 * library allocates nothing, every call is asynchronous on the stream, and arguments are validated BEFORE any HIP call (non-zero return,
 * egr_viewset_last_error() says why, nothing was touched).
 *
 * The kinds, in this order everywhere: 0 render, 1 diffuse, 2 specular, 3 depth, 4 normal, 5 roughness, 6 f0. The store holds, per kind, fp16 planes
 * [num_slots][C][height][width] (channel-major, as Camera holds them) with C = 3, except C = 1 for depth and roughness; a row of depth_range
 * [num_slots][2] fp32 per slot; and, for egr_viewset_gather, the camera rows R [num_slots][9], centers [num_slots][3], fovy [num_slots] in fp32.
 *
 * egr_viewset_ingest: views first_slot .. first_slot + num_views of the store from sources[kind].data [num_views][src_height][src_width][channels]
 * (pixel-major, the dataset's layout) of uint8 (EGR_VIEWSET_U8) or fp32 (EGR_VIEWSET_F32). A kind whose data is NULL is ABSENT: its planes are not
 * written (a store that started as zeros keeps zeros there). channels is 3 for the colour kinds and 1 or 3 for depth and roughness, which take CHANNEL 0
 * of a 3-channel source.
 *   resize     when src_height != height: torch's adaptive average ("area"). The caller's sizes must satisfy width == (uint32_t)((double)height *
 *              ((double)src_width / (double)src_height)) (_resize_image_tensor's output size in Python floats); with src_height == height, src_width ==
 *              width. Window i of an axis covers floor(i * src / dst) up to but excluding ceil((i + 1) * src / dst).
 *   fp32       the fp32 sum of the window in row-major order starting from +0, ONE correctly rounded IEEE division by the element count, then
 *              round-to-nearest-even to half: above 65504 (from 65520) is inf, NaN stays NaN, -0 and subnormals as IEEE rounds them. Without resize: the
 *              value itself, rounded to half.
 *   uint8      the integer sum of the window floor-divided by the count (= .float() -> area -> .byte() upstream), then sources[kind].table[byte]: 256 halfs
 *              in device memory that the caller computed (Camera.__init__'s expressions; there is no pow on the device). uint8 depth is refused, as upstream.
 *              A uint8 source is read as the ALIGNED 32-bit words that contain its bytes: up to 3 bytes past its end inside the last word are read and ignored.
 *   range      depth_range[slot] = (min, max) of the STORED half depth plane as fp32 when depth is present (else the row is not written). The call first
 *              sets the rows to (+inf, -inf); the ingest launch reduces order-preserving integer keys (bits ^ (sign ? ~0 : 1 << 31): -0 < +0) per wave and
 *              per workgroup, and each workgroup then makes one integer atomic per end on the fp32 bit pattern itself (signed min / unsigned max by the
 *              sign bit), so min and max do not depend on arrival order and need no decoding pass. Any NaN in the plane gives (NaN, NaN), as torch's
 *              amin / amax: a NaN is the extreme pattern of its end (0xFFC00000 / 0x7FC00000) and wins against every number in any order.
 * Refused: a NULL table of sources or depth_range, num_views, a size == 0 or > 65535, a window of more than 2^24 elements, the size rule above, first_slot +
 * num_views > num_slots, every kind absent, channels other than 1 or 3 (or 1 for a colour kind), an unknown dtype, uint8 depth, a uint8 source
 * without its table, an fp32 source WITH a table, present data without planes, an fp32 source that is not 4-byte aligned, planes that are not 2-byte
 * aligned, an output (the written planes, the written depth_range rows) that overlaps an input (data, table) or another output.
 *
 * egr_viewset_gather: for v < num_views, out->targets[kind][v] (fp32 [num_views][C][height][width], NULL = not wanted) = (float)planes[kind][indices[v]] -
 * exactly float(half) - and out->R / centers / fovy [v] = the store's rows indices[v] (each NULL = not wanted). `indices` is a HOST array read during the
 * call: it travels in the kernel arguments, EGR_VIEWSET_MAX_GATHER per launch (more views make more launches); no upload, no synchronisation. Repeats and any
 * order are allowed. Refused: a NULL store, out or indices, num_views == 0, height or width == 0, an index >= num_filled, num_filled > num_slots, a wanted
 * kind without planes, a wanted camera row without its store array, nothing wanted, an output that is not 4-byte aligned, an output that overlaps the store
 * or another output. */
#define EGR_VIEWSET_KINDS 7
#define EGR_VIEWSET_DEPTH 3 /* the kind whose min / max is reduced */
#define EGR_VIEWSET_U8 0u
#define EGR_VIEWSET_F32 1u
#define EGR_VIEWSET_MAX_GATHER 64 /* view indices per launch */
typedef struct egr_viewset_source {
    const void *data;  /* [num_views][src_height][src_width][channels]; NULL = the kind is absent  */
    const void *table; /* 256 halfs, device memory: required for uint8, must be NULL for fp32     */
    void *planes;      /* the store's fp16 [num_slots][C][height][width] of this kind            */
    uint32_t channels; /* 1 or 3                                                                */
    uint32_t dtype;    /* EGR_VIEWSET_U8 or EGR_VIEWSET_F32                                      */
} egr_viewset_source;
typedef struct egr_viewset_store {
    const void *planes[EGR_VIEWSET_KINDS]; /* fp16 [num_slots][C][height][width]; NULL where no kind is wanted */
    const float *R;                        /* [num_slots][9]  */
    const float *centers;                  /* [num_slots][3]  */
    const float *fovy;                     /* [num_slots]     */
    uint32_t num_slots;
    uint32_t num_filled; /* indices must be below this */
    uint32_t height;
    uint32_t width;
} egr_viewset_store;
typedef struct egr_viewset_batch {
    float *targets[EGR_VIEWSET_KINDS]; /* fp32 [num_views][C][height][width]; NULL = not wanted */
    float *R;                          /* [num_views][9]; NULL = not wanted */
    float *centers;                    /* [num_views][3] */
    float *fovy;                       /* [num_views]    */
} egr_viewset_batch;
int egr_viewset_ingest(int device, const egr_viewset_source *sources, uint32_t num_views, uint32_t src_height, uint32_t src_width, uint32_t height,
                       uint32_t width, uint32_t first_slot, uint32_t num_slots, float *depth_range, void *hip_stream);
int egr_viewset_gather(int device, const egr_viewset_store *store, const uint32_t *indices, uint32_t num_views, const egr_viewset_batch *out,
                       void *hip_stream);
const char *egr_viewset_last_error(void);

/* ---- prior views (additive symbols of library version 0.8, egr_version() is unchanged): what dataset/blender_prior_dataset.py:94-126 and
 * dataset/colmap_prior_dataset.py:124-146 do per view on the CPU before a network-predicted G-buffer can be trained on - the sparse SfM depth map
 * (utils/depth_utils.py:101-182), the robust affine fit of the predicted depth to it (ransac_linear_fit, :208-278), depth -> distance along the pixel's ray
 * (:66-98), camera normals -> world (:7-16) and f0 from metalness - for a chunk of V views sharing height x width, in three calls (csrc/priors.hip;
 * tests/priors_restatement.py is the same arithmetic in numpy). Context-free: the library allocates nothing, every call is asynchronous on the stream, and
 * arguments are validated BEFORE any HIP call (non-zero return, egr_prior_last_error() says why, nothing was touched). Arrays marked HOST are read during the
 * call by the validation; the array of the same name with _dev is the caller's device copy of the same values, which the kernels read (they clamp what they read
 * from it to the validated sizes, so a copy that differs gives wrong numbers, never an access outside the arrays).
 *
 * cams [V][EGR_PRIOR_CAM_FLOATS] fp32, device: per view the 3x4 world-to-camera matrix (row-major: rows of [R^T | T] of the record), then fx, fy, cx, cy - the
 * Python-float expressions W / (2 tan(fovx / 2)), H / (2 tan(fovy / 2)), W / 2, H / 2 rounded to fp32 on the host - then the record's R (3x3 row-major), which
 * takes camera normals to the world.
 *
 * egr_prior_pairs (steps 1 and 2):
 *   project   every point p of view v (points[offsets[v] .. offsets[v + 1]], world space): c = ((m0 x + m1 y) + m2 z) + m3 per row in fp32; kept if c.z > 0;
 *             u = rint(c.x * fx / c.z + cx), v = rint(c.y * fy / c.z + cy) with every product, quotient and sum rounded once (no contraction) and halves
 *             rounded to even, as torch.round; kept if 0 <= u < width and 0 <= v < height (-0.5 is column 0, width - 0.5 is outside). The kept c.z goes into
 *             sparse [V][height][width], which the call first fills with +inf, by a 32-bit atomic minimum on the bit pattern: the NEAREST point of a pixel
 *             wins, whatever the order of the points (upstream's unstable argsort keeps an arbitrary one). +inf stays where no point fell: +inf = EMPTY.
 *   pairs     per view, the pixels that hold a point in ROW-MAJOR order (the order of upstream's boolean-mask indexing): pairs_x[v][i] = depth[v][pixel]
 *             [channel 0] (the predicted depth), pairs_y[v][i] = sparse[v][pixel], count[v] pairs. A pair whose x is not finite is DROPPED and counted in
 *             dropped[v] (upstream would poison its lstsq). One workgroup and one scan per view: no global counter, the order is exact.
 * Refused: NULL args or a NULL cams, offsets, offsets_dev, depth or output, points NULL with offsets[V] > 0, num_views, height or width outside 1..65535,
 * depth_channels other than 1 or 3, offsets[0] != 0 or offsets that do not ascend, an output that overlaps an input or another output.
 *
 * egr_prior_fit (steps 3 and 4), on pair lists pairs_x / pairs_y [V][pair_stride] of which view v uses the first views[v][0]:
 *   views     HOST [V][4] uint32: count, sample_size S, top_k, 0. Upstream's S = min(max(2, ceil(0.1 N)), 50) and top_k = max(1, ceil(0.1 N)) are Python-float
 *             expressions and stay with the caller. A view with count < 2 cannot be fitted: it gets a = 1, b = 0, best_iteration = -1, best_error = NaN.
 *   samples   HOST [V][num_iters][sample_stride] int32: row (v, it) holds the S pair indices of hypothesis `it` (upstream: random.sample(range(N), S)).
 *   hypotheses (method EGR_PRIOR_RANSAC; grid num_iters x V, one workgroup each) y = w x + b through the S sampled pairs in fp64 by centred normal
 *             equations, summed in sample order: w = Sxy / Sxx, b = my - w mx; with Sxx == 0 the minimum-norm solution (w, b) = my (mx, 1) / (mx^2 + 1), as
 *             lstsq gives for a rank-deficient system. w, b are rounded to fp32. Residuals r_i = |y_i - (w x_i + b)| in fp32 with separate roundings,
 *             recomputed in every pass, never stored. threshold = the top_k-th smallest r, by a 4-pass 8-bit radix select on the bit patterns (monotone for
 *             |.|, +inf and NaN above every number) with a 256-bin histogram in LDS. error = the fp64 sum of r^2 over the top_k smallest = sum over r <
 *             threshold in a fixed order, without atomics, + (top_k - count_less) threshold^2: ties at the threshold do not change it.
 *             hyp_error[v][it] = error; hyp_model[v][it] = (w, b, threshold, the bits of top_k - count_less).
 *   select    (one workgroup per view) best = the smallest error, the lowest iteration among equals (upstream's strict <); a NaN error never wins against a
 *             number. Inliers = every pair with r < threshold plus the FIRST top_k - count_less pairs with r == threshold in pair order (the tie rule: a
 *             definition of this library). (a, b) = the fp64 fit to the inliers, with the same rule for Sxx == 0, rounded to fp32 into ab[v]. best_iteration
 *             [v], best_error[v]; inliers[v][i] (uint8, i < count, NULL = not wanted).
 *   EGR_PRIOR_LSTSQ (upstream's commented-out linear_least_squares_1d) skips the hypotheses: every pair is an inlier, best_iteration = -1, best_error = NaN;
 *             samples, samples_dev, hyp_error and hyp_model are not read or written, num_iters and sample_stride are ignored.
 * Refused: NULL args, pairs, views, views_dev, ab, best_iteration or best_error; for EGR_PRIOR_RANSAC NULL samples, samples_dev, hyp_error or hyp_model,
 * num_iters outside 1..65535, sample_stride outside 1..EGR_PRIOR_MAX_SAMPLE; num_views outside 1..65535, pair_stride outside 1..65535^2, an unknown method, a
 * count above pair_stride, for a view with count >= 2 a sample_size outside 2..min(count, sample_stride) or a top_k outside 1..count, a sample index < 0 or >=
 * its view's count, an output that overlaps an input or another output.
 *
 * egr_prior_finish (step 5), one streaming pass, out of place: per pixel (row v, column u) of view i with a, b = ab[i] read from DEVICE memory (no read-back
 * after the fit):
 *   distance  Z = depth[channel 0] * a + b; X = (u - cx) * Z / fx; Y = (v - cy) * Z / fy; distance = sqrtf((X X + Y Y) + Z Z): fp32, every operation rounded once.
 *   normals   n = -n; n = n / sqrtf((nx nx + ny ny) + nz nz); out = R n (rows of R, ((r0 nx + r1 ny) + r2 nz)). A zero normal gives NaN, as upstream.
 *   f0        0.04f * (1 - m) + m, three times (metalness NULL: f0 is not written and may be NULL).
 * distance [V][H][W][1], normal_out [V][H][W][3], f0 [V][H][W][3]: fp32, pixel-major, the dataset's layout. Refused: NULL args, cams, ab, depth, normal,
 * distance or normal_out, metalness without f0, sizes outside 1..65535, depth_channels other than 1 or 3, an output that overlaps an input or another output. */
#define EGR_PRIOR_CAM_FLOATS 25
#define EGR_PRIOR_RANSAC 0u
#define EGR_PRIOR_LSTSQ 1u
#define EGR_PRIOR_MAX_SAMPLE 1024 /* pair indices per hypothesis */
typedef struct egr_prior_pairs_args {
    uint32_t num_views;
    uint32_t height;
    uint32_t width;
    uint32_t depth_channels;     /* 1 or 3: channel 0 is read                                  */
    const float *cams;           /* device [V][EGR_PRIOR_CAM_FLOATS]                            */
    const float *points;         /* device [offsets[V]][3], world space                         */
    const uint32_t *offsets;     /* HOST [V + 1], ascending from 0                              */
    const uint32_t *offsets_dev; /* device copy of offsets                                      */
    const float *depth;          /* device [V][H][W][depth_channels], the predicted depth       */
    float *sparse;               /* out, device [V][H][W]: nearest point depth, +inf = empty    */
    float *pairs_x;              /* out, device [V][H * W]                                      */
    float *pairs_y;              /* out, device [V][H * W]                                      */
    uint32_t *count;             /* out, device [V]                                             */
    uint32_t *dropped;           /* out, device [V]                                             */
} egr_prior_pairs_args;
typedef struct egr_prior_fit_args {
    uint32_t num_views;
    uint32_t pair_stride;   /* elements between the pair lists of two views (H * W after egr_prior_pairs) */
    uint32_t num_iters;
    uint32_t sample_stride; /* columns of the sample table                                     */
    uint32_t method;        /* EGR_PRIOR_RANSAC or EGR_PRIOR_LSTSQ                             */
    uint32_t reserved;
    const float *pairs_x;        /* device [V][pair_stride]                                     */
    const float *pairs_y;        /* device [V][pair_stride]                                     */
    const uint32_t *views;       /* HOST [V][4]: count, sample_size, top_k, 0                   */
    const uint32_t *views_dev;   /* device copy of views                                        */
    const int32_t *samples;      /* HOST [V][num_iters][sample_stride]                          */
    const int32_t *samples_dev;  /* device copy of samples                                      */
    double *hyp_error;           /* out, device [V][num_iters]                                  */
    float *hyp_model;            /* out, device [V][num_iters][4]: w, b, threshold, ties taken  */
    float *ab;                   /* out, device [V][2]                                          */
    int32_t *best_iteration;     /* out, device [V]                                             */
    double *best_error;          /* out, device [V]                                             */
    uint8_t *inliers;            /* out, device [V][pair_stride]; NULL = not wanted             */
} egr_prior_fit_args;
typedef struct egr_prior_finish_args {
    uint32_t num_views;
    uint32_t height;
    uint32_t width;
    uint32_t depth_channels; /* 1 or 3: channel 0 is read                                       */
    const float *cams;       /* device [V][EGR_PRIOR_CAM_FLOATS]                                */
    const float *ab;         /* device [V][2]                                                   */
    const float *depth;      /* device [V][H][W][depth_channels]                                */
    const float *normal;     /* device [V][H][W][3], camera space                               */
    const float *metalness;  /* device [V][H][W]; NULL = no f0                                  */
    float *distance;         /* out, device [V][H][W][1]                                        */
    float *normal_out;       /* out, device [V][H][W][3], world space                           */
    float *f0;               /* out, device [V][H][W][3]                                        */
} egr_prior_finish_args;
int egr_prior_pairs(int device, const egr_prior_pairs_args *args, void *hip_stream);
int egr_prior_fit(int device, const egr_prior_fit_args *args, void *hip_stream);
int egr_prior_finish(int device, const egr_prior_finish_args *args, void *hip_stream);
const char *egr_prior_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* EGR_RAYTRACER_H */
