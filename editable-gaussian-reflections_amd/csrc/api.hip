// extern "C" surface of libegr_hip.so (see include/egr_raytracer.h). Host-only code; the kernels live in
// bvh.hip and trace.hip. The product fails loudly: every HIP error becomes a non-zero return + message.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <algorithm>

#include "egr_internal.hpp"
#include "egr_diag.hpp"
#include "egr_device.hpp" // egr_div_rn / egr_sqrt_rn: the debug kernel below runs exactly the functions the hot kernels use

void egr_copy_final_to_denoised(egr_context *c, hipStream_t s);
void egr_denoise_atrous(egr_context *c, hipStream_t s); // denoise.hip
void egr_denoise_views_atrous(egr_context *c, uint32_t num_views, const float *final, const float *normal, size_t normal_view_stride, float *denoised, hipStream_t s); // denoise.hip
void egr_export_step_hits(egr_context *c, int32_t *host_out, hipStream_t s); // trace.hip
void egr_export_hit_hash(egr_context *c, uint64_t *host_out, hipStream_t s); // trace.hip
void egr_upload_targets(egr_context *c, const float *const chw[6], hipStream_t s); // trace.hip
void egr_set_camera_launch(egr_context *c, const float *R, const float *centre, float fov, float znear, float zfar, hipStream_t s); // trace.hip
void egr_set_camera_values_launch(egr_context *c, const float *R, bool R_on_host, const float *centre, bool centre_on_host, float fov, float znear, float zfar, hipStream_t s); // trace.hip

void egr_stamp_begin(egr_context *c, const char *name, hipStream_t s) {
    if (!c->timing) return;
    if (c->stamps_used == c->stamps.size()) {
        KernelStamp k{name, nullptr, nullptr};
        EGR_HIP(hipEventCreate(&k.start));
        EGR_HIP(hipEventCreate(&k.stop));
        c->stamps.push_back(k);
    }
    c->stamps[c->stamps_used].name = name;
    EGR_HIP(hipEventRecord(c->stamps[c->stamps_used].start, s));
}
void egr_stamp_end(egr_context *c, hipStream_t s) {
    if (!c->timing) return;
    EGR_HIP(hipEventRecord(c->stamps[c->stamps_used].stop, s));
    c->stamps_used++;
}

namespace {
template <class F> int guarded(egr_context *c, F &&f) {
    try {
        EgrDeviceScope scope(c->device); // the caller's device is back on every way out, a throwing f() included
        f();
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) throw EgrCheck{e, "kernel launch"};
        return 0;
    } catch (const EgrCheck &e) {
        char buf[512];
        snprintf(buf, sizeof buf, "libegr_hip: %s failed: %s", e.what, hipGetErrorString(e.e));
        c->last_error = buf;
        return 1;
    } catch (const std::exception &e) {
        c->last_error = std::string("libegr_hip: ") + e.what();
        return 1;
    }
}
int require_ready(egr_context *c, bool need_bvh) {
    if (!c->bound || !c->have_gaussians) {
        c->last_error = "libegr_hip: egr_bind / egr_set_gaussians must be called first";
        return 1;
    }
    if (need_bvh && (!c->bvh_valid || c->n_built != c->g.count)) {
        c->last_error = "libegr_hip: BVH is missing or was built for a different gaussian count; call egr_rebuild_bvh";
        return 1;
    }
    return 0;
}

// A traced call (egr_raytrace, egr_render_views, egr_train_views) from the readiness checks on: `launch(stream)` runs between the two events
// egr_last_raytrace_ms reads, with the per-kernel stamps counted from zero.
template <class F> int traced(egr_context *c, void *stream, F &&launch) {
    if (require_ready(c, true)) return 1;
    if (c->exact_stats != c->boxes_are_cubes) {
        c->last_error = "libegr_hip: egr_set_exact_stats changed since the tree was last refitted; call egr_update_bvh or egr_rebuild_bvh first";
        return 1;
    }
    return guarded(c, [&] {
        hipStream_t s = (hipStream_t)stream;
        c->stamps_used = 0;
        if (c->timing) EGR_HIP(hipEventRecord(c->ev_rt0, s));
        launch(s);
        if (c->timing) EGR_HIP(hipEventRecord(c->ev_rt1, s)), c->have_rt = true;
    });
}
} // namespace

extern "C" {

#ifdef EGR_VARIANT_NAME // a variant build (build.py) carries its name after the product's string
#define EGR_VERSION_SUFFIX " variant " EGR_VARIANT_NAME
#else
#define EGR_VERSION_SUFFIX ""
#endif
const char *egr_version(void) { return "egr-hip 0.8 (gfx950)" EGR_VERSION_SUFFIX; } // 0.8: egr_render_views, egr_set_batch_frames, and (additive, same version) egr_train_views; 0.7: strands removed, egr_set_strands accepts only 1; 0.6: egr_grad_delta_consumed (round 5); 0.4: egr_counters grew (round 3), egr_get_counters_ex, egr_set_rays_per_task; 0.5: egr_set_team_help

int egr_create(egr_context **out, int device, int width, int height, int64_t ppll_forward_size, int64_t ppll_backward_size) {
    if (!out || width <= 0 || height <= 0) return 1;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "libegr_hip: no HIP device available (this library has no CPU fallback)\n");
        return 2;
    }
    egr_context *c = new egr_context();
    c->device = device, c->width = width, c->height = height;
    c->fwd_capacity = ppll_forward_size > 0 ? ppll_forward_size : 1, c->bwd_capacity = ppll_backward_size > 0 ? ppll_backward_size : 1;
    if (const char *e = getenv("EGR_DENOISE")) c->denoise_mode = atoi(e);
    if (const char *e = getenv("EGR_TEAM_HELP")) c->team_help = atoi(e) != 0 ? 1 : 0;
    if (const char *e = getenv("EGR_BATCH_FRAMES")) c->batch_frames = (uint32_t)std::max(1, atoi(e));
    int rc = guarded(c, [&] {
        egr_trace_alloc(c);
        EGR_HIP(hipEventCreate(&c->ev_rt0)), EGR_HIP(hipEventCreate(&c->ev_rt1));
        EGR_HIP(hipEventCreate(&c->ev_ub0)), EGR_HIP(hipEventCreate(&c->ev_ub1));
    });
    if (rc) {
        fprintf(stderr, "%s\n", c->last_error.c_str());
        delete c;
        return rc;
    }
    *out = c;
    return 0;
}

void egr_destroy(egr_context *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    egr_trace_free(c);
    egr_bvh_free(c);
    egr_dev_free(c, c->denoise_views_tmp);
    for (auto &k : c->stamps) (void)hipEventDestroy(k.start), (void)hipEventDestroy(k.stop);
    if (c->ev_rt0) (void)hipEventDestroy(c->ev_rt0), (void)hipEventDestroy(c->ev_rt1), (void)hipEventDestroy(c->ev_ub0), (void)hipEventDestroy(c->ev_ub1);
    delete c;
}

int egr_bind(egr_context *c, const egr_camera *camera, const egr_config *config, const egr_framebuffer *framebuffer,
             const egr_metadata *metadata, const egr_stats *stats) {
    if (!c || !camera || !config || !framebuffer || !metadata || !stats) return 1;
    c->cam = *camera, c->cfg = *config, c->fb = *framebuffer, c->meta = *metadata, c->stats = *stats;
    c->bound = true;
    c->live_fresh = false; // other config scalars: the live records of a fused update are not trusted across a re-bind
    return 0;
}

int egr_set_gaussians(egr_context *c, const egr_gaussians *g) {
    if (!c || !g) return 1;
    c->g = *g;
    c->have_gaussians = true;
    c->live_fresh = false;
    return guarded(c, [&] { egr_bvh_reserve(c, g->count); });
}

int egr_set_partition(egr_context *c, int rank, int world) {
    if (!c || world < 1 || rank < 0 || rank >= world) return 1;
    c->rank = rank, c->world = world;
    return guarded(c, [&] { egr_build_task_order(c); }); // cached per (rank, world): flipping between two partitions costs nothing
}

int egr_set_grad_overwrite(egr_context *c, int enable) {
    if (!c) return 1;
    c->grad_overwrite = enable != 0;
    c->delta_pending = false;
    return 0;
}

int egr_grad_delta_consumed(egr_context *c) {
    if (!c) return 1;
    c->delta_pending = false;
    return 0;
}

int egr_set_exact_stats(egr_context *c, int enable) {
    if (!c) return 1;
    c->live_fresh = false;
    c->exact_stats = enable != 0; // the boxes change at the next egr_update_bvh / egr_rebuild_bvh; egr_raytrace checks that they did
    return 0;
}

int egr_set_rays_per_task(egr_context *c, int rays_per_task) {
    if (!c || !(rays_per_task == 0 || rays_per_task == 16 || rays_per_task == 32 || rays_per_task == 64)) return 1;
    c->rays_per_task = rays_per_task;
    return 0;
}

int egr_set_team_help(egr_context *c, int on) {
    if (!c || !(on == 0 || on == 1 || on == -1)) return 1;
    c->team_help = on;
    return 0;
}

int egr_set_strands(egr_context *c, int strands) { return c && strands == 1 ? 0 : 1; }

int egr_rebuild_bvh(egr_context *c, void *stream) {
    if (!c || require_ready(c, false)) return 1;
    return guarded(c, [&] { egr_bvh_rebuild(c, (hipStream_t)stream); });
}

int egr_update_bvh_ex(egr_context *c, unsigned flags, void *stream) {
    if (!c) return 1;
    c->live_fresh = false; // set again by a refit that wrote the live records (egr_bvh_refit), and only if it got that far
    if (require_ready(c, true)) return 1;
    if (flags & ~(unsigned)EGR_UPDATE_FUSE_LIVE) {
        c->last_error = "libegr_hip: egr_update_bvh_ex: unknown flag";
        return 1;
    }
    return guarded(c, [&] {
        hipStream_t s = (hipStream_t)stream;
        if (c->timing) EGR_HIP(hipEventRecord(c->ev_ub0, s));
        egr_bvh_refit(c, s, (flags & EGR_UPDATE_FUSE_LIVE) != 0);
        if (c->timing) EGR_HIP(hipEventRecord(c->ev_ub1, s)), c->have_ub = true;
    });
}
int egr_update_bvh(egr_context *c, void *stream) { return egr_update_bvh_ex(c, 0u, stream); }

int egr_update_bvh_from(egr_context *c, const egr_gaussians *src, unsigned flags, void *stream) {
    if (!c) return 1;
    c->live_fresh = false;
    // ---- validation: before any HIP call
    // (an empty cloud has nothing to read: its tensors have no storage, and their pointers may be NULL)
    if (!src || (c->g.count != 0 && (!src->scale || !src->rotation || !src->mean || !src->opacity || !src->rgb || !src->normal || !src->roughness || !src->f0))) {
        c->last_error = "libegr_hip: egr_update_bvh_from: src and its eight parameter pointers must be non-NULL";
        return 1;
    }
    if (reinterpret_cast<uintptr_t>(src->rotation) & 15u) {
        c->last_error = "libegr_hip: egr_update_bvh_from: src->rotation must be 16-byte aligned";
        return 1;
    }
    if (flags & ~(unsigned)EGR_UPDATE_FUSE_LIVE) {
        c->last_error = "libegr_hip: egr_update_bvh_from: unknown flag";
        return 1;
    }
    if (require_ready(c, true)) return 1;
    const EgrParamSource from{src->scale, src->rotation, src->mean, src->opacity, src->rgb, src->normal, src->roughness, src->f0};
    return guarded(c, [&] {
        hipStream_t s = (hipStream_t)stream;
        if (c->timing) EGR_HIP(hipEventRecord(c->ev_ub0, s));
        egr_bvh_refit(c, s, (flags & EGR_UPDATE_FUSE_LIVE) != 0, &from);
        if (c->timing) EGR_HIP(hipEventRecord(c->ev_ub1, s)), c->have_ub = true;
    });
}

int egr_raytrace(egr_context *c, int grads_enabled, void *stream) {
    if (!c) return 1;
    // The live records of an egr_update_bvh_ex(EGR_UPDATE_FUSE_LIVE) are honoured by the raytrace that is the NEXT call on this context
    // and by nothing else: the flag is consumed here, before anything can fail, so a launch that is refused (stale tree, exact-stats
    // gate) or any other call in between (egr_bind, egr_set_gaussians, egr_set_exact_stats, rebuild, another update) leaves the next
    // launch reading the live tensors itself.
    const bool live_fresh = c->live_fresh;
    c->live_fresh = false;
    return traced(c, stream, [&](hipStream_t s) { egr_trace_launch(c, grads_enabled != 0, live_fresh, s); });
}

// The caller's gradient tensors of an importing grad launch, validated before any HIP call: all eight non-NULL, none the holder's own (the sum would be
// added to itself), and no per-launch buffer (its launches store, and a partition reduces between gather and import).
static int import_target(egr_context *c, const char *who, const egr_gaussians *dst, EgrGradImport &imp) {
    auto refuse = [&](const char *what) {
        c->last_error = std::string("libegr_hip: ") + who + ": " + what;
        return 1;
    };
    const bool empty = c->g.count == 0; // (nothing to add to: the pointers are not read and may be NULL)
    if (!dst || (!empty && (!dst->dL_drgb || !dst->dL_dnormal || !dst->dL_df0 || !dst->dL_droughness || !dst->dL_dopacity || !dst->dL_dscale || !dst->dL_dmean || !dst->dL_drotation)))
        return refuse("dst and its eight dL_d* pointers must be non-NULL");
    if (c->grad_overwrite) return refuse("the context writes a per-launch gradient buffer (egr_set_grad_overwrite): import after the reduction instead");
    const egr_gaussians &h = c->g;
    if (!empty && (dst->dL_drgb == h.dL_drgb || dst->dL_dnormal == h.dL_dnormal || dst->dL_df0 == h.dL_df0 || dst->dL_droughness == h.dL_droughness || dst->dL_dopacity == h.dL_dopacity ||
        dst->dL_dscale == h.dL_dscale || dst->dL_dmean == h.dL_dmean || dst->dL_drotation == h.dL_drotation))
        return refuse("dst must not be the bound gradient tensors themselves");
    imp = EgrGradImport{dst->dL_drgb, dst->dL_dnormal, dst->dL_df0, dst->dL_droughness, dst->dL_dopacity, dst->dL_dscale, dst->dL_dmean, dst->dL_drotation};
    return 0;
}

int egr_raytrace_import(egr_context *c, const egr_gaussians *dst, void *stream) {
    if (!c) return 1;
    const bool live_fresh = c->live_fresh; // (consumed as by egr_raytrace)
    c->live_fresh = false;
    EgrGradImport imp{};
    if (import_target(c, "egr_raytrace_import", dst, imp)) return 1;
    return traced(c, stream, [&](hipStream_t s) { egr_trace_launch(c, true, live_fresh, s, &imp); });
}

// A launch with its optional extras: the import of egr_raytrace_import (dst) and the six target images read in place (targets). Both need a grad launch.
int egr_raytrace_targets(egr_context *c, int grads_enabled, const egr_gaussians *dst, const float *const *targets, void *stream) {
    if (!c) return 1;
    const bool live_fresh = c->live_fresh; // (consumed as by egr_raytrace)
    c->live_fresh = false;
    if (!grads_enabled && targets) {
        c->last_error = "libegr_hip: egr_raytrace_targets: targets need a grad launch (a no-grad launch reads no target)";
        return 1;
    }
    if (!grads_enabled && dst) {
        c->last_error = "libegr_hip: egr_raytrace_targets: dst needs a grad launch (a no-grad launch has no gradients to import)";
        return 1;
    }
    EgrGradImport imp{};
    if (dst && import_target(c, "egr_raytrace_targets", dst, imp)) return 1;
    EgrTargetPlanes planes{};
    if (targets)
        for (int k = 0; k < 6; k++) planes.chw[k] = targets[k];
    return traced(c, stream, [&](hipStream_t s) { egr_trace_launch(c, grads_enabled != 0, live_fresh, s, dst ? &imp : nullptr, targets ? &planes : nullptr); });
}

int egr_render_views(egr_context *c, const egr_view_batch *b, void *stream) {
    if (!c) return 1;
    const bool live_fresh = c->live_fresh; // (consumed as by egr_raytrace: the batch's first chunk may use the live records of a fused update)
    c->live_fresh = false;
    if (!b || b->num_views == 0 || b->samples_per_view == 0 || !b->final || !b->rotation_c2w_dataset || !b->camera_center || !b->vertical_fov_radians) {
        c->last_error = "libegr_hip: egr_render_views: num_views and samples_per_view must be >= 1, final and the three camera arrays non-NULL";
        return 1;
    }
    if ((uint64_t)b->num_views * b->samples_per_view > 0x7FFFFFFFull) {
        c->last_error = "libegr_hip: egr_render_views: num_views x samples_per_view must stay below 2^31";
        return 1;
    }
    return traced(c, stream, [&](hipStream_t s) { egr_render_views_launch(c, b, live_fresh, s); });
}

int egr_train_views(egr_context *c, const egr_train_batch *b, void *stream) { return egr_train_views_import(c, b, nullptr, stream); }

int egr_train_views_import(egr_context *c, const egr_train_batch *b, const egr_gaussians *dst, void *stream) {
    if (!c) return 1;
    const bool live_fresh = c->live_fresh; // (consumed as by egr_raytrace)
    c->live_fresh = false;
    EgrGradImport imp{};
    if (dst && import_target(c, "egr_train_views_import", dst, imp)) return 1;
    if (!b || b->num_views == 0 || !b->rotation_c2w_dataset || !b->camera_center || !b->vertical_fov_radians) {
        c->last_error = "libegr_hip: egr_train_views: num_views must be >= 1 and the three camera arrays non-NULL";
        return 1;
    }
    if (b->num_views > 0x7FFFFFFFu) {
        c->last_error = "libegr_hip: egr_train_views: num_views must stay below 2^31";
        return 1;
    }
    return traced(c, stream, [&](hipStream_t s) { egr_train_views_launch(c, b, live_fresh, s, dst ? &imp : nullptr); });
}

int egr_object_masks(egr_context *c, const egr_object_mask_query *q, void *stream) {
    if (!c) return 1;
    auto refuse = [&](const char *what) { // (before any HIP call: nothing was touched, a fused update's live records stay valid for the next launch)
        c->last_error = std::string("libegr_hip: egr_object_masks: ") + what;
        return 1;
    };
    if (!q) return refuse("the query must be non-NULL");
    if (!q->rotation_c2w_dataset || !q->camera_center || !q->vertical_fov_radians) return refuse("the three camera arrays must be non-NULL");
    if (!q->row_bits || !q->bits || !q->masks) return refuse("row_bits, bits and masks must be non-NULL");
    if (q->num_bits == 0 || q->num_bits > EGR_MAX_EDIT_OBJECTS) return refuse("num_bits must be 1 .. EGR_MAX_EDIT_OBJECTS (32)");
    uint32_t seen = 0u;
    for (uint32_t j = 0; j < q->num_bits; j++) {
        if (q->bits[j] >= 32) return refuse("a selection bit must be < 32");
        if ((seen >> q->bits[j]) & 1u) return refuse("a selection bit was given twice");
        seen |= 1u << q->bits[j];
    }
    if (c->exact_stats || c->boxes_are_cubes) return refuse("the context is in exact-statistics mode (egr_set_exact_stats): per-object coverage exists for the product tree only");
    const bool live_fresh = c->live_fresh; // (consumed as by egr_raytrace)
    c->live_fresh = false;
    return traced(c, stream, [&](hipStream_t s) { egr_object_masks_launch(c, q, live_fresh, s); });
}

int egr_set_batch_frames(egr_context *c, int frames) {
    if (!c || frames < 1) return 1;
    c->batch_frames = (uint32_t)frames;
    return 0;
}

int egr_set_camera_from_dataset(egr_context *c, const float *rotation_c2w_dataset, const float *camera_center, float vertical_fov_radians, float znear, float zfar, void *stream) {
    if (!c || !c->bound || !rotation_c2w_dataset || !camera_center) return 1;
    return guarded(c, [&] { egr_set_camera_launch(c, rotation_c2w_dataset, camera_center, vertical_fov_radians, znear, zfar, (hipStream_t)stream); });
}

int egr_set_camera_from_dataset_ex(egr_context *c, const float *rotation_c2w_dataset, const float *camera_center, float vertical_fov_radians, float znear, float zfar, unsigned flags,
                                   void *stream) {
    if (!c || !c->bound || !rotation_c2w_dataset || !camera_center) return 1;
    if (flags & ~(EGR_CAMERA_ROTATION_ON_HOST | EGR_CAMERA_CENTER_ON_HOST)) {
        c->last_error = "libegr_hip: egr_set_camera_from_dataset_ex: unknown flag";
        return 1;
    }
    if (flags == 0u) return egr_set_camera_from_dataset(c, rotation_c2w_dataset, camera_center, vertical_fov_radians, znear, zfar, stream);
    return guarded(c, [&] {
        egr_set_camera_values_launch(c, rotation_c2w_dataset, (flags & EGR_CAMERA_ROTATION_ON_HOST) != 0u, camera_center, (flags & EGR_CAMERA_CENTER_ON_HOST) != 0u, vertical_fov_radians, znear,
                                     zfar, (hipStream_t)stream);
    });
}

int egr_set_targets_chw(egr_context *c, const float *diffuse, const float *specular, const float *depth, const float *normal, const float *roughness, const float *f0, void *stream) {
    if (!c || !c->bound) return 1;
    const float *chw[6] = {diffuse, specular, depth, normal, roughness, f0};
    return guarded(c, [&] { egr_upload_targets(c, chw, (hipStream_t)stream); });
}

int egr_denoise(egr_context *c, void *stream) {
    if (!c || require_ready(c, false)) return 1;
    return guarded(c, [&] {
        if (c->denoise_mode == 0) egr_copy_final_to_denoised(c, (hipStream_t)stream); // EGR_DENOISE=0: plain copy
        else egr_denoise_atrous(c, (hipStream_t)stream);
    });
}

int egr_denoise_views(egr_context *c, uint32_t num_views, const float *final, const float *normal, size_t normal_view_stride, float *denoised, void *stream) {
    if (!c) return 1;
    // ---- validation: before any HIP call
    const size_t n = (size_t)c->width * c->height * 3;
    auto refuse = [&](const char *what) {
        c->last_error = std::string("libegr_hip: egr_denoise_views: ") + what;
        return 1;
    };
    if (num_views == 0 || num_views > 65535u) return refuse("num_views must be in 1..65535");
    if (!final || !normal || !denoised) return refuse("final, normal and denoised must be non-NULL");
    if (normal_view_stride < n) return refuse("normal_view_stride is smaller than one image (H * W * 3 floats)");
    const uintptr_t f0 = (uintptr_t)final, d0 = (uintptr_t)denoised, g0 = (uintptr_t)normal;
    const size_t bytes = (size_t)num_views * n * sizeof(float), gbytes = ((size_t)(num_views - 1) * normal_view_stride + n) * sizeof(float);
    if (f0 < d0 + bytes && d0 < f0 + bytes) return refuse("final and denoised overlap: the filter runs out of place");
    if (g0 < d0 + bytes && d0 < g0 + gbytes) return refuse("normal and denoised overlap: every pass reads the guide");
    return guarded(c, [&] {
        hipStream_t s = (hipStream_t)stream;
        if (c->denoise_mode == 0) EGR_HIP(hipMemcpyAsync(denoised, final, bytes, hipMemcpyDeviceToDevice, s)); // EGR_DENOISE=0: plain copy
        else egr_denoise_views_atrous(c, num_views, final, normal, normal_view_stride, denoised, s);
    });
}

int egr_get_counters(egr_context *c, egr_counters *out, void *stream) { return egr_get_counters_ex(c, out, sizeof(egr_counters), stream); }

int egr_get_counters_ex(egr_context *c, void *out_raw, size_t out_bytes, void *stream) {
    if (!c || !out_raw) return 1;
    egr_counters full{}, *out = &full; // filled completely, then the caller gets as much of it as its struct holds
    const int rc = guarded(c, [&] {
        // the control block only crosses PCIe when somebody asks for it (nothing does inside a training iteration)
        EGR_HIP(hipMemcpyAsync(c->control_host, c->control, CW_COUNT * sizeof(uint32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
        EGR_HIP(hipStreamSynchronize((hipStream_t)stream));
        const uint32_t *w = c->control_host;
        auto u64 = [&](int i) { return (uint64_t)w[i] | ((uint64_t)w[i + 1] << 32); };
        for (int s = 0; s < EGR_NSTEPS; s++)
            out->rays[s] = u64(CW_RAYS + 2 * s), out->candidates[s] = u64(CW_CAND + 2 * s), out->composited[s] = u64(CW_COMP + 2 * s), out->accepted[s] = u64(CW_ACCEPTED + 2 * s);
        out->lifetime_rays = u64(CW_LIFE_RAYS);
        out->lifetime_launches = w[CW_LIFE_LAUNCHES];
        out->status = w[CW_STATUS];
        out->bvh_depth = c->max_depth;
        out->bucket_records = w[CW_BUCKET_RECORDS];
        out->device_bytes = (uint64_t)c->device_bytes;
        out->arena_blocks_used = w[CW_HIT_BUMP], out->arena_blocks_cap = c->hit_blocks_cap;
        out->ext_blocks_used = w[CW_EXT_BUMP], out->ext_blocks_cap = c->ext_blocks_cap;
        if (getenv("EGR_DEBUG_EXT")) fprintf(stderr, "[egr] extension blocks used %u of %u, cand_cap %u\n", w[CW_EXT_BUMP], c->ext_blocks_cap, c->cand_cap);
        if (getenv("EGR_PRINT_TRAVERSAL_STATS")) egr_diag_print(w); // (egr_diag.hpp; all zero unless this is an EGR_TRAVERSAL_STATS build)
    });
    if (rc == 0) memcpy(out_raw, &full, out_bytes < sizeof(full) ? out_bytes : sizeof(full));
    return rc;
}

int egr_reset_lifetime_counters(egr_context *c, void *stream) {
    if (!c) return 1;
    return guarded(c, [&] { EGR_HIP(hipMemsetAsync(c->control + CW_LIFE_RAYS, 0, 4 * sizeof(uint32_t), (hipStream_t)stream)); });
}

int egr_enable_timing(egr_context *c, int enable) {
    if (!c) return 1;
    c->timing = enable != 0;
    c->have_rt = c->have_ub = false;
    c->stamps_used = 0;
    return 0;
}
float egr_last_raytrace_ms(egr_context *c) {
    if (!c || !c->have_rt) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(c->ev_rt1) != hipSuccess || hipEventElapsedTime(&ms, c->ev_rt0, c->ev_rt1) != hipSuccess) return -1.0f;
    return ms;
}
float egr_last_update_bvh_ms(egr_context *c) {
    if (!c || !c->have_ub) return -1.0f;
    float ms = -1.0f;
    if (hipEventSynchronize(c->ev_ub1) != hipSuccess || hipEventElapsedTime(&ms, c->ev_ub0, c->ev_ub1) != hipSuccess) return -1.0f;
    return ms;
}
int egr_last_kernel_ms(egr_context *c, float *ms, const char **names, int max_entries) {
    if (!c) return 0;
    int n = 0;
    for (size_t i = 0; i < c->stamps_used && n < max_entries; i++) {
        float t = -1.0f;
        if (hipEventSynchronize(c->stamps[i].stop) != hipSuccess) break;
        if (hipEventElapsedTime(&t, c->stamps[i].start, c->stamps[i].stop) != hipSuccess) break;
        ms[n] = t;
        if (names) names[n] = c->stamps[i].name;
        n++;
    }
    return n;
}

int egr_debug_get_instances(egr_context *c, float *M, float *W, float *aabb, void *stream) {
    if (!c) return 1;
    return guarded(c, [&] {
        EGR_HIP(hipStreamSynchronize((hipStream_t)stream));
        size_t n = c->n_built;
        std::vector<uint32_t> pos(n);
        std::vector<float> tmp(n * 16);
        EGR_HIP(hipMemcpy(pos.data(), c->pos_of_gid, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        auto unpermute = [&](const float4 *src, float *dst, size_t stride) { // test records live at sorted positions; report them per gaussian id
            EGR_HIP(hipMemcpy(tmp.data(), src, n * stride * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) memcpy(dst + 12 * i, tmp.data() + stride * (size_t)pos[i], 12 * sizeof(float));
        };
        if (M) { // backward records (kept by id) hold (M row, exp(scale)); the reported 3x4 transform carries the mean in column 3
            EGR_HIP(hipMemcpy(tmp.data(), c->inst_m, n * 16 * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++) memcpy(M + 12 * i, tmp.data() + 16 * i, 12 * sizeof(float));
            std::vector<float> mean(3 * n);
            EGR_HIP(hipMemcpy(mean.data(), c->g.mean, 3 * n * sizeof(float), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; i++)
                for (int a = 0; a < 3; a++) M[12 * i + 4 * a + 3] = mean[3 * i + a];
        }
        if (W) unpermute(c->inst_w, W, 16);
        if (aabb) EGR_HIP(hipMemcpy(aabb, c->aabb, n * 6 * sizeof(float), hipMemcpyDeviceToHost));
    });
}

int egr_debug_get_backward_records(egr_context *c, float *host_out, void *stream) {
    if (!c || !host_out) return 1;
    return guarded(c, [&] {
        EGR_HIP(hipStreamSynchronize((hipStream_t)stream));
        if (c->n_built) EGR_HIP(hipMemcpy(host_out, c->inst_m, (size_t)c->n_built * 16 * sizeof(float), hipMemcpyDeviceToHost)); // (kept by id: no permutation)
    });
}

int egr_debug_set_pixel_mask(egr_context *c, const uint8_t *device_mask) {
    if (!c) return 1;
    c->pixel_mask = device_mask;
    return 0;
}

int egr_debug_get_step_hits(egr_context *c, int32_t *host_out, void *stream) {
    if (!c || !host_out || require_ready(c, false)) return 1;
    return guarded(c, [&] { egr_export_step_hits(c, host_out, (hipStream_t)stream); });
}

int egr_debug_get_hit_sequence_hash(egr_context *c, uint64_t *host_out, void *stream) {
    if (!c || !host_out || require_ready(c, false)) return 1;
    return guarded(c, [&] { egr_export_hit_hash(c, host_out, (hipStream_t)stream); });
}

// Unit test hook for the division / square root of the hot arithmetic (egr_device.hpp): quot[i] = egr_div_rn(a[i], b[i], egr_rcp_refined(b[i])), root[i] = egr_sqrt_rn(a[i]).
__global__ void k_debug_lean_arith(const float *__restrict__ a, const float *__restrict__ b, float *__restrict__ quot, float *__restrict__ root, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    quot[i] = egr_div_rn(a[i], b[i], egr_rcp_refined(b[i]));
    root[i] = egr_sqrt_rn(a[i]);
}
int egr_debug_lean_arith(int device, const float *a, const float *b, float *quot, float *root, uint32_t n, void *stream) {
    if (!a || !b || !quot || !root) return 1;
    std::string unused; // (a test hook: it reports through its return value alone)
    return egr_on_device(device, unused, "egr_debug_lean_arith", [&] {
        if (n) egr_launch(k_debug_lean_arith, dim3((n + 255u) / 256u), dim3(256), (hipStream_t)stream, a, b, quot, root, n);
    });
}

int egr_debug_check_bvh(egr_context *c, void *stream) {
    if (!c) return 1;
    int bad = 0;
    int rc = guarded(c, [&] {
        std::string msg;
        bad = egr_bvh_check(c, (hipStream_t)stream, msg);
        if (bad) c->last_error = "libegr_hip: BVH check failed: " + msg;
    });
    return rc ? rc : bad;
}

int egr_debug_get_bvh_state(egr_context *c, float frame[6], uint32_t info[4], void *stream) {
    if (!c || !frame || !info) return 1;
    return guarded(c, [&] {
        EGR_HIP(hipStreamSynchronize((hipStream_t)stream));
        uint32_t flag = 0;
        if (c->out_of_frame) EGR_HIP(hipMemcpy(&flag, c->out_of_frame, sizeof(uint32_t), hipMemcpyDeviceToHost));
        const BvhFrame fr = c->frame;
        frame[0] = fr.ox, frame[1] = fr.oy, frame[2] = fr.oz, frame[3] = fr.sx, frame[4] = fr.sy, frame[5] = fr.sz;
        info[0] = flag, info[1] = c->num_wide, info[2] = c->max_depth, info[3] = c->n_built;
    });
}

int egr_debug_get_tree(egr_context *c, uint64_t *keys, uint32_t *gid_of_pos, uint32_t *pos_of_gid, int32_t *left, int32_t *right, float *dp,
                       uint32_t *wnodes, float *bsph, uint32_t *level_start, void *stream) {
    if (!c) return 1;
    return guarded(c, [&] {
        EGR_HIP(hipStreamSynchronize((hipStream_t)stream));
        const size_t n = c->n_built, nb = n > 1 ? n - 1 : 0, nw = c->num_wide; // (binary nodes exist from two leaves on)
        auto fetch = [&](void *dst, const void *src, size_t bytes) {
            if (dst && bytes) EGR_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        };
        fetch(keys, c->keys_out, n * sizeof(uint64_t));
        fetch(gid_of_pos, c->vals_out, n * sizeof(uint32_t));
        fetch(pos_of_gid, c->pos_of_gid, n * sizeof(uint32_t));
        fetch(left, c->k_left, nb * sizeof(int32_t));
        fetch(right, c->k_right, nb * sizeof(int32_t));
        fetch(dp, c->k_dp, nb * EGR_DP_STRIDE * sizeof(float));
        fetch(wnodes, c->wnodes, nw * EGR_WIDTH * sizeof(uint4));
        fetch(bsph, c->bsph, n * sizeof(float4));
        if (level_start) std::copy(c->level_start.begin(), c->level_start.end(), level_start);
    });
}

const char *egr_last_error(egr_context *c) { return c ? c->last_error.c_str() : "libegr_hip: null context"; }

} // extern "C"
