// libraytracer.so -- TORCH_LIBRARY(raytracer, m) shim over the C ABI of libegr_hip.so.
//
// Registers the same eight TorchScript custom classes, with the same names, constructor signature, methods and
// read-only tensor attributes (names, shapes, dtypes, defaults) as the reference's
// editable_gauss_refl/cuda/csrc/raytracer.cpp:122-218 and core/*.h holders, so
//     torch.classes.load_library(".../libraytracer.so"); torch.classes.raytracer.Raytracer(W, H, N, fwd, bwd)
// works unchanged (editable_gauss_refl/__init__.py:15-27). This file only owns tensors and forwards raw device
// pointers; all arithmetic is in the HIP library. There is no CPU fallback: construction fails without a GPU.
//
// "torch::kCUDA" below is PyTorch's device name for HIP devices on ROCm builds, not a compatibility layer.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/custom_class.h>
#include <torch/library.h>
#include <torch/torch.h>

#include <string>
#include <tuple>
#include <vector>

#include "../../include/egr_raytracer.h"

using at::Tensor;

namespace {
inline at::TensorOptions F32() { return torch::dtype(torch::kFloat32).device(torch::kCUDA); }
inline at::TensorOptions I32() { return torch::dtype(torch::kInt32).device(torch::kCUDA); }
inline at::TensorOptions B8() { return torch::dtype(torch::kBool).device(torch::kCUDA); }
inline void *current_stream() { return (void *)c10::hip::getCurrentHIPStream().stream(); }
template <class T> T *ptr(const Tensor &t) { return reinterpret_cast<T *>(t.data_ptr()); }
} // namespace

// core/camera.h:43-77
struct CameraDataHolder : torch::CustomClassHolder {
    Tensor origin = torch::zeros({3}, F32());
    Tensor vertical_fov_radians = torch::zeros({1}, F32());
    Tensor rotation_c2w = torch::zeros({3, 3}, F32());
    Tensor rotation_w2c = torch::zeros({3, 3}, F32());
    Tensor znear = torch::zeros({1}, F32());
    Tensor zfar = torch::zeros({1}, F32());
    egr_camera reify() {
        return egr_camera{ptr<float>(origin), ptr<float>(vertical_fov_radians), ptr<float>(rotation_c2w), ptr<float>(rotation_w2c),
                          ptr<float>(znear), ptr<float>(zfar)};
    }
    void set_pose(const Tensor &c2w_origin, const Tensor &c2w_rotation) { // camera.h:62-68
        TORCH_CHECK(c2w_rotation.sizes() == torch::IntArrayRef({3, 3}), "c2w_rotation must be 3x3");
        TORCH_CHECK(c2w_origin.sizes() == torch::IntArrayRef({3}), "c2w_origin must be 3");
        rotation_c2w.copy_(c2w_rotation);
        origin.copy_(c2w_origin);
        rotation_w2c.copy_(c2w_rotation.transpose(0, 1));
    }
    static void bind(torch::Library &m) {
        m.class_<CameraDataHolder>("CameraDataHolder")
            .def("set_pose", &CameraDataHolder::set_pose)
            .def_readonly("vertical_fov_radians", &CameraDataHolder::vertical_fov_radians)
            .def_readonly("znear", &CameraDataHolder::znear)
            .def_readonly("zfar", &CameraDataHolder::zfar);
    }
};

// core/config.h:31-101 (defaults :32-51)
struct ConfigDataHolder : torch::CustomClassHolder {
    Tensor exp_power = torch::tensor({3.0f}, F32());
    Tensor alpha_threshold = torch::tensor({0.005f}, F32());
    Tensor transmittance_threshold = torch::tensor({0.01f}, F32());
    Tensor accumulate_samples = torch::zeros({1}, B8());
    Tensor jitter_primary_rays = torch::ones({1}, B8());
    Tensor num_bounces = torch::full({1}, 2, I32());
    Tensor global_scale_factor = torch::ones({1}, F32());
    Tensor loss_weight_diffuse = torch::ones({1}, F32());
    Tensor loss_weight_specular = torch::ones({1}, F32());
    Tensor loss_weight_depth = torch::ones({1}, F32());
    Tensor loss_weight_normal = torch::ones({1}, F32());
    Tensor loss_weight_f0 = torch::ones({1}, F32());
    Tensor loss_weight_roughness = torch::ones({1}, F32());
    Tensor eps_forward_normalization = torch::tensor({1e-12f}, F32());
    Tensor eps_scale_grad = torch::tensor({1e-12f}, F32());
    Tensor eps_ray_surface_offset = torch::tensor({0.01f}, F32());
    Tensor eps_min_roughness = torch::tensor({0.01f}, F32());
    Tensor reflection_invalid_normal_threshold = torch::tensor({0.7f}, F32());
    Tensor backfacing_invalid_normal_threshold = torch::tensor({0.9f}, F32());
    Tensor backfacing_max_dist = torch::tensor({0.1f}, F32());
    egr_config reify() {
        egr_config c;
        c.exp_power = ptr<float>(exp_power), c.alpha_threshold = ptr<float>(alpha_threshold);
        c.transmittance_threshold = ptr<float>(transmittance_threshold);
        c.accumulate_samples = ptr<uint8_t>(accumulate_samples), c.jitter_primary_rays = ptr<uint8_t>(jitter_primary_rays);
        c.num_bounces = ptr<int32_t>(num_bounces), c.global_scale_factor = ptr<float>(global_scale_factor);
        c.loss_weight_diffuse = ptr<float>(loss_weight_diffuse), c.loss_weight_specular = ptr<float>(loss_weight_specular);
        c.loss_weight_depth = ptr<float>(loss_weight_depth), c.loss_weight_normal = ptr<float>(loss_weight_normal);
        c.loss_weight_f0 = ptr<float>(loss_weight_f0), c.loss_weight_roughness = ptr<float>(loss_weight_roughness);
        c.eps_forward_normalization = ptr<float>(eps_forward_normalization), c.eps_scale_grad = ptr<float>(eps_scale_grad);
        c.eps_ray_surface_offset = ptr<float>(eps_ray_surface_offset), c.eps_min_roughness = ptr<float>(eps_min_roughness);
        c.reflection_invalid_normal_threshold = ptr<float>(reflection_invalid_normal_threshold);
        c.backfacing_invalid_normal_threshold = ptr<float>(backfacing_invalid_normal_threshold);
        c.backfacing_max_dist = ptr<float>(backfacing_max_dist);
        return c;
    }
    static void bind(torch::Library &m) {
        m.class_<ConfigDataHolder>("ConfigDataHolder")
            .def_readonly("exp_power", &ConfigDataHolder::exp_power)
            .def_readonly("alpha_threshold", &ConfigDataHolder::alpha_threshold)
            .def_readonly("transmittance_threshold", &ConfigDataHolder::transmittance_threshold)
            .def_readonly("accumulate_samples", &ConfigDataHolder::accumulate_samples)
            .def_readonly("jitter_primary_rays", &ConfigDataHolder::jitter_primary_rays)
            .def_readonly("num_bounces", &ConfigDataHolder::num_bounces)
            .def_readonly("global_scale_factor", &ConfigDataHolder::global_scale_factor)
            .def_readonly("loss_weight_diffuse", &ConfigDataHolder::loss_weight_diffuse)
            .def_readonly("loss_weight_specular", &ConfigDataHolder::loss_weight_specular)
            .def_readonly("loss_weight_depth", &ConfigDataHolder::loss_weight_depth)
            .def_readonly("loss_weight_normal", &ConfigDataHolder::loss_weight_normal)
            .def_readonly("loss_weight_f0", &ConfigDataHolder::loss_weight_f0)
            .def_readonly("loss_weight_roughness", &ConfigDataHolder::loss_weight_roughness)
            .def_readonly("eps_forward_normalization", &ConfigDataHolder::eps_forward_normalization)
            .def_readonly("eps_scale_grad", &ConfigDataHolder::eps_scale_grad)
            .def_readonly("eps_ray_surface_offset", &ConfigDataHolder::eps_ray_surface_offset)
            .def_readonly("eps_min_roughness", &ConfigDataHolder::eps_min_roughness)
            .def_readonly("reflection_invalid_normal_threshold", &ConfigDataHolder::reflection_invalid_normal_threshold)
            .def_readonly("backfacing_invalid_normal_threshold", &ConfigDataHolder::backfacing_invalid_normal_threshold)
            .def_readonly("backfacing_max_dist", &ConfigDataHolder::backfacing_max_dist);
    }
};

// core/framebuffer.h:159-288
struct FramebufferDataHolder : torch::CustomClassHolder {
    Tensor output_rgb, output_depth, output_normal, output_f0, output_roughness, output_transmittance, output_total_transmittance,
        output_ray_origin, output_ray_direction, output_final, output_denoised;
    Tensor accumulated_rgb, accumulated_transmittance, accumulated_total_transmittance, accumulated_depth, accumulated_normal,
        accumulated_f0, accumulated_roughness, accumulated_sample_count;
    Tensor target_diffuse, target_specular, target_depth, target_normal, target_f0, target_roughness;
    FramebufferDataHolder(int64_t w, int64_t h) {
        const int64_t S = EGR_NUM_STEPS;
        auto z = [&](int64_t lead, int64_t c) { return torch::zeros({lead, h, w, c}, F32()); };
        output_rgb = z(S, 3), output_depth = z(S, 1), output_normal = z(S, 3), output_f0 = z(S, 3), output_roughness = z(S, 1);
        output_transmittance = z(S, 1), output_total_transmittance = z(S, 1), output_ray_origin = z(S, 3), output_ray_direction = z(S, 3);
        output_final = z(1, 3), output_denoised = z(1, 3);
        accumulated_rgb = z(S, 3), accumulated_transmittance = z(S, 1), accumulated_total_transmittance = z(S, 1);
        accumulated_depth = z(S, 1), accumulated_normal = z(S, 3), accumulated_f0 = z(S, 3), accumulated_roughness = z(S, 1);
        accumulated_sample_count = torch::zeros({1}, I32());
        auto t = [&](int64_t c) { return torch::zeros({h, w, c}, F32()); };
        target_diffuse = t(3), target_specular = t(3), target_depth = t(1), target_normal = t(3), target_f0 = t(3), target_roughness = t(1);
    }
    egr_framebuffer reify() {
        egr_framebuffer f;
        f.output_rgb = ptr<float>(output_rgb), f.output_depth = ptr<float>(output_depth), f.output_normal = ptr<float>(output_normal);
        f.output_f0 = ptr<float>(output_f0), f.output_roughness = ptr<float>(output_roughness);
        f.output_transmittance = ptr<float>(output_transmittance), f.output_total_transmittance = ptr<float>(output_total_transmittance);
        f.output_ray_origin = ptr<float>(output_ray_origin), f.output_ray_direction = ptr<float>(output_ray_direction);
        f.output_final = ptr<float>(output_final), f.output_denoised = ptr<float>(output_denoised);
        f.accumulated_rgb = ptr<float>(accumulated_rgb), f.accumulated_transmittance = ptr<float>(accumulated_transmittance);
        f.accumulated_total_transmittance = ptr<float>(accumulated_total_transmittance), f.accumulated_depth = ptr<float>(accumulated_depth);
        f.accumulated_normal = ptr<float>(accumulated_normal), f.accumulated_f0 = ptr<float>(accumulated_f0);
        f.accumulated_roughness = ptr<float>(accumulated_roughness), f.accumulated_sample_count = ptr<int32_t>(accumulated_sample_count);
        f.target_diffuse = ptr<float>(target_diffuse), f.target_specular = ptr<float>(target_specular), f.target_depth = ptr<float>(target_depth);
        f.target_normal = ptr<float>(target_normal), f.target_f0 = ptr<float>(target_f0), f.target_roughness = ptr<float>(target_roughness);
        return f;
    }
    void reset_accumulators() { // framebuffer.h:249-258
        accumulated_rgb.zero_(), accumulated_transmittance.zero_(), accumulated_total_transmittance.zero_(), accumulated_depth.zero_();
        accumulated_normal.zero_(), accumulated_f0.zero_(), accumulated_roughness.zero_(), accumulated_sample_count.zero_();
    }
    static void bind(torch::Library &m) {
        m.class_<FramebufferDataHolder>("Framebuffer")
            .def_readonly("output_rgb", &FramebufferDataHolder::output_rgb)
            .def_readonly("output_depth", &FramebufferDataHolder::output_depth)
            .def_readonly("output_normal", &FramebufferDataHolder::output_normal)
            .def_readonly("output_f0", &FramebufferDataHolder::output_f0)
            .def_readonly("output_roughness", &FramebufferDataHolder::output_roughness)
            .def_readonly("output_transmittance", &FramebufferDataHolder::output_transmittance)
            .def_readonly("output_total_transmittance", &FramebufferDataHolder::output_total_transmittance)
            .def_readonly("output_ray_origin", &FramebufferDataHolder::output_ray_origin)
            .def_readonly("output_ray_direction", &FramebufferDataHolder::output_ray_direction)
            .def_readonly("output_final", &FramebufferDataHolder::output_final)
            .def_readonly("output_denoised", &FramebufferDataHolder::output_denoised)
            .def_readonly("accumulated_rgb", &FramebufferDataHolder::accumulated_rgb)
            .def_readonly("accumulated_transmittance", &FramebufferDataHolder::accumulated_transmittance)
            .def_readonly("accumulated_total_transmittance", &FramebufferDataHolder::accumulated_total_transmittance)
            .def_readonly("accumulated_depth", &FramebufferDataHolder::accumulated_depth)
            .def_readonly("accumulated_normal", &FramebufferDataHolder::accumulated_normal)
            .def_readonly("accumulated_f0", &FramebufferDataHolder::accumulated_f0)
            .def_readonly("accumulated_roughness", &FramebufferDataHolder::accumulated_roughness)
            .def_readonly("accumulated_sample_count", &FramebufferDataHolder::accumulated_sample_count)
            .def_readonly("target_diffuse", &FramebufferDataHolder::target_diffuse)
            .def_readonly("target_specular", &FramebufferDataHolder::target_specular)
            .def_readonly("target_depth", &FramebufferDataHolder::target_depth)
            .def_readonly("target_normal", &FramebufferDataHolder::target_normal)
            .def_readonly("target_f0", &FramebufferDataHolder::target_f0)
            .def_readonly("target_roughness", &FramebufferDataHolder::target_roughness);
    }
};

// core/gaussians.h:30-135. The nine gradient tensors are windows into ONE contiguous buffer (grad_flat, 22 floats
// per Gaussian, tensor-major) so that multi-GPU training needs a single all-reduce; each keeps the reference's
// shape and is installed as .grad of its parameter (gaussians.h:54-61).
struct GaussianDataHolder : torch::CustomClassHolder {
    int64_t count = 1;
    Tensor rgb = torch::zeros({1, 3}, F32()), normal = torch::zeros({1, 3}, F32()), f0 = torch::zeros({1, 3}, F32());
    Tensor roughness = torch::zeros({1, 1}, F32()), opacity = torch::zeros({1, 1}, F32()), scale = torch::zeros({1, 3}, F32());
    Tensor mean = torch::zeros({1, 3}, F32()), rotation = torch::zeros({1, 4}, F32());
    Tensor grad_flat = torch::zeros({22}, F32());
    Tensor dL_drgb = torch::empty({0}, F32()), dL_dnormal = torch::empty({0}, F32()), dL_df0 = torch::empty({0}, F32());
    Tensor dL_droughness = torch::empty({0}, F32()), dL_dopacity = torch::empty({0}, F32()), dL_dscale = torch::empty({0}, F32());
    Tensor dL_dmean = torch::empty({0}, F32()), dL_drotation = torch::empty({0}, F32()), total_weight = torch::empty({0}, F32());

    void point_grads() {
        int64_t off = 0;
        auto win = [&](Tensor &t, int64_t c) {
            t.set_(grad_flat.storage(), off, {count, c}, {c, 1}); // same TensorImpl, new window
            off += count * c;
        };
        win(dL_drgb, 3), win(dL_dnormal, 3), win(dL_df0, 3), win(dL_droughness, 1), win(dL_dopacity, 1);
        win(dL_dscale, 3), win(dL_dmean, 3), win(dL_drotation, 4), win(total_weight, 1);
    }
    GaussianDataHolder() {
        torch::NoGradGuard no_grad;
        point_grads();
        rgb.mutable_grad() = dL_drgb, normal.mutable_grad() = dL_dnormal, f0.mutable_grad() = dL_df0;
        roughness.mutable_grad() = dL_droughness, opacity.mutable_grad() = dL_dopacity, scale.mutable_grad() = dL_dscale;
        mean.mutable_grad() = dL_dmean, rotation.mutable_grad() = dL_drotation;
    }
    // Multi-GPU (not in the reference): with `use_delta` a grad launch STORES its gradients and weights in a [22N] buffer of its own
    // (grad_delta; egr_set_grad_overwrite: rows no ray touched read 0, nobody has to clear it) instead of adding them to the persistent
    // one, so the caller can all-reduce exactly one launch's contribution and then fold it in (renderer.py: all_reduce_grads) - summing
    // the persistent buffer would multiply whatever it already holds (total_weight across a pruning interval, accumulated gradients)
    // by the world size on every iteration.
    Tensor grad_delta = torch::empty({0}, F32());
    bool use_delta = false;
    void set_use_delta(bool on) {
        use_delta = on;
        grad_delta = on ? torch::zeros({22 * count}, F32()) : torch::empty({0}, F32());
    }
    void resize(int64_t n) { // gaussians.h:64-86: resize_ keeps the first min(old, n) rows of every tensor; grown gradient memory is zeroed here
        torch::NoGradGuard no_grad;
        const int64_t keep = std::min(count, n);
        Tensor old_rows[9] = {dL_drgb.narrow(0, 0, keep).clone(), dL_dnormal.narrow(0, 0, keep).clone(), dL_df0.narrow(0, 0, keep).clone(),
                              dL_droughness.narrow(0, 0, keep).clone(), dL_dopacity.narrow(0, 0, keep).clone(), dL_dscale.narrow(0, 0, keep).clone(),
                              dL_dmean.narrow(0, 0, keep).clone(), dL_drotation.narrow(0, 0, keep).clone(), total_weight.narrow(0, 0, keep).clone()};
        count = n;
        rgb.resize_({n, 3}), normal.resize_({n, 3}), f0.resize_({n, 3}), roughness.resize_({n, 1}), opacity.resize_({n, 1});
        scale.resize_({n, 3}), mean.resize_({n, 3}), rotation.resize_({n, 4});
        grad_flat = torch::zeros({22 * n}, F32());
        point_grads();
        Tensor *win[9] = {&dL_drgb, &dL_dnormal, &dL_df0, &dL_droughness, &dL_dopacity, &dL_dscale, &dL_dmean, &dL_drotation, &total_weight};
        for (int k = 0; k < 9 && keep > 0; k++) win[k]->narrow(0, 0, keep).copy_(old_rows[k]);
        if (use_delta) grad_delta = torch::zeros({22 * n}, F32());
    }
    egr_gaussians reify() {
        egr_gaussians g;
        g.count = (uint32_t)count;
        g.rgb = ptr<float>(rgb), g.normal = ptr<float>(normal), g.f0 = ptr<float>(f0), g.roughness = ptr<float>(roughness);
        g.opacity = ptr<float>(opacity), g.scale = ptr<float>(scale), g.mean = ptr<float>(mean), g.rotation = ptr<float>(rotation);
        float *base = use_delta ? ptr<float>(grad_delta) : ptr<float>(grad_flat); // same tensor-major layout as point_grads()
        const size_t n = (size_t)count;
        g.dL_drgb = base, g.dL_dnormal = base + 3 * n, g.dL_df0 = base + 6 * n, g.dL_droughness = base + 9 * n, g.dL_dopacity = base + 10 * n;
        g.dL_dscale = base + 11 * n, g.dL_dmean = base + 14 * n, g.dL_drotation = base + 17 * n, g.total_weight = base + 21 * n;
        return g;
    }
    static void bind(torch::Library &m) {
        m.class_<GaussianDataHolder>("GaussianDataHolder")
            .def_readonly("rgb", &GaussianDataHolder::rgb)
            .def_readonly("normal", &GaussianDataHolder::normal)
            .def_readonly("f0", &GaussianDataHolder::f0)
            .def_readonly("roughness", &GaussianDataHolder::roughness)
            .def_readonly("opacity", &GaussianDataHolder::opacity)
            .def_readonly("scale", &GaussianDataHolder::scale)
            .def_readonly("mean", &GaussianDataHolder::mean)
            .def_readonly("rotation", &GaussianDataHolder::rotation)
            .def_readonly("dL_drgb", &GaussianDataHolder::dL_drgb)
            .def_readonly("dL_dnormal", &GaussianDataHolder::dL_dnormal)
            .def_readonly("dL_df0", &GaussianDataHolder::dL_df0)
            .def_readonly("dL_droughness", &GaussianDataHolder::dL_droughness)
            .def_readonly("dL_dopacity", &GaussianDataHolder::dL_dopacity)
            .def_readonly("dL_dscale", &GaussianDataHolder::dL_dscale)
            .def_readonly("dL_dmean", &GaussianDataHolder::dL_dmean)
            .def_readonly("dL_drotation", &GaussianDataHolder::dL_drotation)
            .def_readonly("total_weight", &GaussianDataHolder::total_weight)
            .def_readonly("grad_flat", &GaussianDataHolder::grad_flat)    // addition: [22N] view of all of the above
            .def_readonly("grad_delta", &GaussianDataHolder::grad_delta); // addition: per-launch gradient buffer (empty unless use_grad_delta): stored by the first grad launch after grad_delta_consumed(), added to by further ones
    }
};

// core/metadata.h:12-39
struct MetaDataHolder : torch::CustomClassHolder {
    Tensor grads_enabled = torch::ones({1}, B8());
    Tensor total_num_calls = torch::zeros({1}, I32());
    Tensor random_seeds;
    MetaDataHolder(int64_t w, int64_t h) { random_seeds = torch::randint(0, 1000000000, {h, w, 1}, I32()); }
    egr_metadata reify() { return egr_metadata{ptr<uint8_t>(grads_enabled), ptr<int32_t>(total_num_calls), ptr<int32_t>(random_seeds)}; }
    static void bind(torch::Library &m) {
        m.class_<MetaDataHolder>("MetaDataHolder")
            .def_readonly("grads_enabled", &MetaDataHolder::grads_enabled)
            .def_readonly("total_num_calls", &MetaDataHolder::total_num_calls)
            .def_readonly("random_seeds", &MetaDataHolder::random_seeds);
    }
};

// core/stats.h:11-37
struct StatsDataHolder : torch::CustomClassHolder {
    Tensor num_accumulated_per_pixel, num_traversed_per_pixel;
    StatsDataHolder(int64_t w, int64_t h) {
        num_accumulated_per_pixel = torch::zeros({h, w}, I32());
        num_traversed_per_pixel = torch::zeros({h, w}, I32());
    }
    egr_stats reify() { return egr_stats{ptr<int32_t>(num_accumulated_per_pixel), ptr<int32_t>(num_traversed_per_pixel)}; }
    static void bind(torch::Library &m) {
        m.class_<StatsDataHolder>("StatsDataHolder")
            .def_readonly("num_accumulated_per_pixel", &StatsDataHolder::num_accumulated_per_pixel)
            .def_readonly("num_traversed_per_pixel", &StatsDataHolder::num_traversed_per_pixel);
    }
};

// core/per_pixel_linked_list.h:80-136. The HIP path has no global linked list; the class is kept (no Python
// caller reads its entries) with one-entry stubs so attribute access and NULL_PTR() keep working. `size` is
// remembered because it sizes the candidate scratch / hit arena instead.
struct PPLLDataHolder : torch::CustomClassHolder {
    int64_t requested_size;
    Tensor head_per_pixel, total_hits = torch::zeros({1}, I32()) - 1, gaussian_ids, distances, gaussvals, alphas, local_hits, transmittances,
                           previous_entries;
    PPLLDataHolder(int64_t w, int64_t h, int64_t size) : requested_size(size) {
        head_per_pixel = torch::full({h, w}, (int64_t)(int32_t)EGR_PPLL_NULL_PTR, I32());
        gaussian_ids = torch::zeros({1}, I32()), distances = torch::zeros({1}, F32()), gaussvals = torch::zeros({1}, F32());
        alphas = torch::zeros({1}, F32()), local_hits = torch::zeros({1, 3}, F32()), transmittances = torch::zeros({1}, F32());
        previous_entries = torch::zeros({1}, I32());
    }
    static void bind(torch::Library &m) {
        m.class_<PPLLDataHolder>("PPLLDataHolder")
            .def_readonly("head_per_pixel", &PPLLDataHolder::head_per_pixel)
            .def_readonly("total_hits", &PPLLDataHolder::total_hits)
            .def_readonly("gaussian_ids", &PPLLDataHolder::gaussian_ids)
            .def_readonly("distances", &PPLLDataHolder::distances)
            .def_readonly("alphas", &PPLLDataHolder::alphas)
            .def_readonly("transmittances", &PPLLDataHolder::transmittances)
            .def_readonly("local_hits", &PPLLDataHolder::local_hits)
            .def_readonly("gaussvals", &PPLLDataHolder::gaussvals)
            .def_readonly("previous_entries", &PPLLDataHolder::previous_entries)
            .def_static("NULL_PTR", []() { return (int64_t)EGR_PPLL_NULL_PTR; });
    }
};

// raytracer.cpp:24-205
struct Raytracer : torch::CustomClassHolder {
    int64_t width, height;
    c10::intrusive_ptr<CameraDataHolder> camera_data;
    c10::intrusive_ptr<ConfigDataHolder> config_data;
    c10::intrusive_ptr<FramebufferDataHolder> framebuffer_data;
    c10::intrusive_ptr<GaussianDataHolder> gaussian_data;
    c10::intrusive_ptr<MetaDataHolder> meta_data;
    c10::intrusive_ptr<StatsDataHolder> stats_data;
    c10::intrusive_ptr<PPLLDataHolder> ppll_forward_data, ppll_backward_data;
    egr_context *ctx = nullptr;
    Tensor pixel_mask; // debug_set_pixel_mask: the mask the context points at
    // raytrace(targets=...) read its images in place and left framebuffer.target_* BEHIND them. The images are remembered (referenced, not copied) until the next
    // set_targets_chw, or until a grad raytrace() WITHOUT targets - a launch that reads framebuffer.target_* - uploads them first: the upload the in-place launch
    // skipped is made only for a caller that goes on to need it (the reference's caller leaves its targets in the framebuffer, and a bare raytrace() after it reads them)
    Tensor behind_targets[6];
    bool framebuffer_targets_behind = false;
    void forget_behind_targets() {
        for (auto &t : behind_targets) t = Tensor();
        framebuffer_targets_behind = false;
    }
    void upload_behind_targets() {
        if (!framebuffer_targets_behind) return;
        const float *p[6];
        for (int k = 0; k < 6; k++) p[k] = behind_targets[k].defined() ? behind_targets[k].data_ptr<float>() : nullptr;
        check(egr_set_targets_chw(ctx, p[0], p[1], p[2], p[3], p[4], p[5], current_stream()), "raytrace");
        forget_behind_targets();
    }

    void check(int rc, const char *what) {
        if (rc != 0) throw std::runtime_error(std::string(what) + ": " + (ctx ? egr_last_error(ctx) : "no context"));
    }

    Raytracer(int64_t width_, int64_t height_, int64_t num_gaussians, int64_t forward_ppl_size, int64_t backward_ppl_size)
        : width(width_), height(height_), camera_data(c10::make_intrusive<CameraDataHolder>()),
          config_data(c10::make_intrusive<ConfigDataHolder>()),
          framebuffer_data(c10::make_intrusive<FramebufferDataHolder>(width_, height_)),
          gaussian_data(c10::make_intrusive<GaussianDataHolder>()), meta_data(c10::make_intrusive<MetaDataHolder>(width_, height_)),
          stats_data(c10::make_intrusive<StatsDataHolder>(width_, height_)),
          ppll_forward_data(c10::make_intrusive<PPLLDataHolder>(width_, height_, forward_ppl_size)),
          ppll_backward_data(c10::make_intrusive<PPLLDataHolder>(width_, height_, backward_ppl_size)) {
        if (num_gaussians > 0) gaussian_data->resize(num_gaussians);
        int device = (int)camera_data->origin.get_device();
        int rc = egr_create(&ctx, device, (int)width, (int)height, forward_ppl_size, backward_ppl_size);
        if (rc != 0) throw std::runtime_error("raytracer: egr_create failed (no usable HIP device? there is no CPU fallback)");
        egr_camera cam = camera_data->reify();
        egr_config cfg = config_data->reify();
        egr_framebuffer fb = framebuffer_data->reify();
        egr_metadata md = meta_data->reify();
        egr_stats st = stats_data->reify();
        check(egr_bind(ctx, &cam, &cfg, &fb, &md, &st), "egr_bind");
        egr_gaussians g = gaussian_data->reify();
        check(egr_set_gaussians(ctx, &g), "egr_set_gaussians");
        // upstream builds the TLAS over `count` (zero-initialised) instances in the constructor (bvh_wrapper.h:17-22)
        check(egr_rebuild_bvh(ctx, current_stream()), "egr_rebuild_bvh");
    }
    ~Raytracer() override {
        if (ctx) egr_destroy(ctx);
    }

    // The caller's eight tensors of a fused export / import, in the export order of gaussian_raytracer.py:41-50 (scale, rotation, mean, opacity, rgb, normal,
    // roughness, f0): each a contiguous fp32 tensor on the tracer's device with the shape of the holder's. Checked before anything is launched.
    void check_like_holder(const char *who, const std::vector<Tensor> &t) {
        const Tensor *like[8] = {&gaussian_data->scale, &gaussian_data->rotation, &gaussian_data->mean, &gaussian_data->opacity, &gaussian_data->rgb, &gaussian_data->normal,
                                 &gaussian_data->roughness, &gaussian_data->f0};
        static const char *const names[8] = {"scale", "rotation", "mean", "opacity", "rgb", "normal", "roughness", "f0"};
        TORCH_CHECK(t.size() == 8, who, ": eight tensors expected (scale, rotation, mean, opacity, rgb, normal, roughness, f0), got ", t.size());
        for (int k = 0; k < 8; k++)
            TORCH_CHECK(t[k].defined() && t[k].device() == like[k]->device() && t[k].scalar_type() == torch::kFloat32 && t[k].is_contiguous() && t[k].sizes() == like[k]->sizes(), who,
                        ": '", names[k], "' must be a contiguous fp32 tensor ", like[k]->sizes(), " on the tracer's device");
    }
    // import_into (addition; grad mode only): the caller's eight gradient tensors, in the order of update_bvh_from's parameters. The launch's gather adds what it
    // leaves in the holder's gradients to them - `t.grad += holder.grad` for the eight, bit for bit, without the extra pass (egr_raytrace_import).
    // targets (addition; grad mode only): the view's six target images in set_targets_chw's order (diffuse, specular, depth, normal, roughness, f0), each None
    // (absent = zeros) or a contiguous fp32 [C,H,W] tensor on the tracer's device. The launch reads them where they are - no upload, framebuffer.target_* is
    // neither read nor written (egr_raytrace_targets). The caller keeps them alive and unmodified until the launch has completed on the current stream.
    void raytrace(c10::optional<std::vector<Tensor>> import_into, c10::optional<std::vector<c10::optional<Tensor>>> targets) { // raytracer.cpp:81-94
        const bool grads = torch::autograd::GradMode::is_enabled();
        if (grads && !targets.has_value()) upload_behind_targets(); // this launch reads framebuffer.target_*
        if (!import_into.has_value() && !targets.has_value()) {
            check(egr_raytrace(ctx, grads ? 1 : 0, current_stream()), "raytrace");
            return;
        }
        TORCH_CHECK(grads || !import_into.has_value(), "raytrace: import_into needs grad mode (a no-grad launch has no gradients to import)");
        TORCH_CHECK(grads || !targets.has_value(), "raytrace: targets need grad mode (a no-grad launch reads no target)");
        egr_gaussians dst{};
        if (import_into.has_value()) dst = import_target("raytrace", *import_into);
        const float *planes[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        if (targets.has_value()) {
            TORCH_CHECK(targets->size() == 6, "raytrace: six targets expected (diffuse, specular, depth, normal, roughness, f0; None = absent), got ", targets->size());
            const auto dev = framebuffer_data->output_rgb.device();
            for (int k = 0; k < 6; k++) {
                if (!(*targets)[k].has_value() || !(*targets)[k]->defined()) continue;
                const Tensor &t = *(*targets)[k];
                const std::vector<int64_t> want{TARGETS[k].channels, height, width};
                TORCH_CHECK(t.device() == dev && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.sizes() == torch::IntArrayRef(want), "raytrace: target '", TARGETS[k].name,
                            "' must be a contiguous fp32 tensor ", torch::IntArrayRef(want), " (channel-major) on the tracer's device, got ", t.sizes(), " ", t.scalar_type(), " on ", t.device());
                planes[k] = t.data_ptr<float>();
            }
        }
        check(egr_raytrace_targets(ctx, 1, import_into.has_value() ? &dst : nullptr, targets.has_value() ? planes : nullptr, current_stream()), "raytrace");
        if (targets.has_value()) {
            for (int k = 0; k < 6; k++) behind_targets[k] = (*targets)[k].has_value() ? *(*targets)[k] : Tensor();
            framebuffer_targets_behind = true;
        }
    }
    egr_gaussians import_target(const char *who, const std::vector<Tensor> &t) {
        check_like_holder(who, t);
        egr_gaussians dst{};
        dst.count = (uint32_t)gaussian_data->count;
        dst.dL_dscale = ptr<float>(t[0]), dst.dL_drotation = ptr<float>(t[1]), dst.dL_dmean = ptr<float>(t[2]), dst.dL_dopacity = ptr<float>(t[3]);
        dst.dL_drgb = ptr<float>(t[4]), dst.dL_dnormal = ptr<float>(t[5]), dst.dL_droughness = ptr<float>(t[6]), dst.dL_df0 = ptr<float>(t[7]);
        return dst;
    }
    void denoise() { check(egr_denoise(ctx, current_stream()), "denoise"); }
    void reset_accumulators() { framebuffer_data->reset_accumulators(); }
    // fuse_live (addition; default = the reference's update_bvh()): the pass also writes the live per-gaussian records and the NEXT raytrace()
    // skips its own pass over the cloud - for callers that run update_bvh() and raytrace() back to back (egr_update_bvh_ex)
    void update_bvh(bool fuse_live) { check(egr_update_bvh_ex(ctx, fuse_live ? EGR_UPDATE_FUSE_LIVE : 0u, current_stream()), "update_bvh"); }
    // export + update_bvh(fuse_live) in one pass over the cloud (egr_update_bvh_from): the eight tensors hold the caller's current parameter values; the
    // holder's tensors then hold them too, as after the eight copy_ calls of gaussian_raytracer.py:41-50
    void update_bvh_from(Tensor scale, Tensor rotation, Tensor mean, Tensor opacity, Tensor rgb, Tensor normal, Tensor roughness, Tensor f0, bool fuse_live) {
        const std::vector<Tensor> t{scale, rotation, mean, opacity, rgb, normal, roughness, f0};
        check_like_holder("update_bvh_from", t);
        TORCH_CHECK((reinterpret_cast<uintptr_t>(rotation.data_ptr()) & 15u) == 0, "update_bvh_from: 'rotation' must be 16-byte aligned");
        egr_gaussians src{};
        src.count = (uint32_t)gaussian_data->count;
        src.scale = ptr<float>(scale), src.rotation = ptr<float>(rotation), src.mean = ptr<float>(mean), src.opacity = ptr<float>(opacity);
        src.rgb = ptr<float>(rgb), src.normal = ptr<float>(normal), src.roughness = ptr<float>(roughness), src.f0 = ptr<float>(f0);
        check(egr_update_bvh_from(ctx, &src, fuse_live ? EGR_UPDATE_FUSE_LIVE : 0u, current_stream()), "update_bvh_from");
    }
    void rebuild_bvh() { check(egr_rebuild_bvh(ctx, current_stream()), "rebuild_bvh"); }
    void resize(int64_t n) { // raytracer.cpp:112-120
        gaussian_data->resize(n);
        egr_gaussians g = gaussian_data->reify();
        check(egr_set_gaussians(ctx, &g), "resize");
    }
    // ---- additions (not in the reference) ----
    void set_partition(int64_t rank, int64_t world) { check(egr_set_partition(ctx, (int)rank, (int)world), "set_partition"); }
    void use_grad_delta(bool on) { // see GaussianDataHolder::grad_delta
        gaussian_data->set_use_delta(on);
        egr_gaussians g = gaussian_data->reify();
        check(egr_set_gaussians(ctx, &g), "use_grad_delta");
        check(egr_set_grad_overwrite(ctx, on ? 1 : 0), "use_grad_delta"); // the first grad launch after grad_delta_consumed() STORES its sums in grad_delta (nobody clears it), further ones add
    }
    void grad_delta_consumed() { check(egr_grad_delta_consumed(ctx), "grad_delta_consumed"); } // the caller folded grad_delta into grad_flat: the next grad launch stores again
    // exact statistics: num_traversed_per_pixel / the candidate counters become the reference's intersection-program invocation
    // count (cube boxes, slower). Takes effect with the next update_bvh() / rebuild_bvh(); raytrace() refuses to run in between.
    void set_exact_stats(bool on) { check(egr_set_exact_stats(ctx, on ? 1 : 0), "set_exact_stats"); }
    // debug: trace only the pixels with mask != 0 ([H*W] or [H, W] uint8 CUDA tensor; an empty tensor clears the mask). The tensor is kept alive here.
    void debug_set_pixel_mask(Tensor mask) {
        if (mask.numel() == 0) {
            pixel_mask = Tensor();
            check(egr_debug_set_pixel_mask(ctx, nullptr), "debug_set_pixel_mask");
            return;
        }
        TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == torch::kUInt8 && mask.numel() == width * height, "debug_set_pixel_mask: uint8 CUDA tensor with H*W elements expected");
        pixel_mask = mask.contiguous();
        check(egr_debug_set_pixel_mask(ctx, pixel_mask.data_ptr<uint8_t>()), "debug_set_pixel_mask");
    }
    // pose + scalars of a view in one launch (egr_set_camera_from_dataset): R = the dataset's c2w rotation [3,3], centre = camera_center [3], fp32 CUDA tensors
    void set_camera(Tensor R, Tensor centre, double fov, double znear, double zfar) {
        // (the reference's copy_ calls - gaussian_raytracer.py:98-100 - take tensors of any device: a CPU tensor is moved to this tracer's device first)
        TORCH_CHECK(R.dim() == 2 && R.size(0) == 3 && R.size(1) == 3 && centre.numel() == 3, "set_camera: tensors [3,3] and [3] expected");
        const auto dev = framebuffer_data->output_rgb.device();
        Tensor r = R.to(dev, torch::kFloat32).contiguous(), cc = centre.to(dev, torch::kFloat32).contiguous();
        check(egr_set_camera_from_dataset(ctx, r.data_ptr<float>(), cc.data_ptr<float>(), (float)fov, (float)znear, (float)zfar, current_stream()), "set_camera");
    }
    static constexpr struct { const char *name; int64_t channels; } TARGETS[6] = {{"diffuse", 3}, {"specular", 3}, {"depth", 1}, {"normal", 3}, {"roughness", 1}, {"f0", 3}}; // (the order of the C ABI's six target pointers)
    // the six target images of a training view, channel-major ([C,H,W] contiguous fp32 CUDA tensors; an undefined / empty tensor = absent = zeros), written into
    // the framebuffer's pixel-major target buffers for this context's own tiles in one launch (egr_set_targets_chw)
    void set_targets_chw(c10::optional<Tensor> diffuse, c10::optional<Tensor> specular, c10::optional<Tensor> depth, c10::optional<Tensor> normal, c10::optional<Tensor> roughness,
                         c10::optional<Tensor> f0) {
        const c10::optional<Tensor> *in[6] = {&diffuse, &specular, &depth, &normal, &roughness, &f0};
        Tensor keep[6];
        const float *p[6];
        for (int b = 0; b < 6; b++) {
            p[b] = nullptr;
            if (!in[b]->has_value() || (*in[b])->numel() == 0) continue;
            // (the reference's `buf.copy_(val.moveaxis(0, -1))` raises on any other shape and accepts any device: same here - a [H,W,C] tensor must not be read as [C,H,W])
            const Tensor &t = **in[b];
            TORCH_CHECK(t.dim() == 3 && t.size(0) == TARGETS[b].channels && t.size(1) == height && t.size(2) == width, "set_targets_chw: target ", b, " must be a [", TARGETS[b].channels, ",", height, ",", width, "] tensor (channel-major), got ", t.sizes());
            keep[b] = t.to(framebuffer_data->output_rgb.device(), torch::kFloat32).contiguous();
            p[b] = keep[b].data_ptr<float>();
        }
        check(egr_set_targets_chw(ctx, p[0], p[1], p[2], p[3], p[4], p[5], current_stream()), "set_targets_chw");
        forget_behind_targets(); // the framebuffer's targets are what the caller says again
    }
    // batched no-grad render (egr_render_views): R [V,3,3] (dataset c2w rotations), centers [V,3], fovy [V] (any device, moved like set_camera's),
    // `outputs` = names among final / rgb / depth / normal / f0 / roughness. render_views allocates them (zeros) in the framebuffer's HWC layout with a
    // leading V - final [V,H,W,3], the others [V,3,H,W,c] - and returns them in the order asked; render_views_into writes the caller's tensors instead.
    static int64_t view_output_channels(const std::string &name) {
        if (name == "final" || name == "rgb" || name == "normal" || name == "f0") return 3;
        if (name == "depth" || name == "roughness") return 1;
        return 0;
    }
    // The three camera tensors of a batch, validated (`who` = the caller's name in the messages): (R, centers, fovy) as contiguous fp32 tensors on the tracer's device, and V.
    std::tuple<Tensor, Tensor, Tensor, int64_t> batch_cameras(const char *who, const Tensor &R, const Tensor &centers, const Tensor &fovy) {
        TORCH_CHECK(R.dim() == 3 && R.size(1) == 3 && R.size(2) == 3, who, ": R must be [V,3,3], got ", R.sizes());
        const int64_t V = R.size(0);
        TORCH_CHECK(centers.dim() == 2 && centers.size(0) == V && centers.size(1) == 3, who, ": centers must be [V,3] = [", V, ",3], got ", centers.sizes());
        TORCH_CHECK(fovy.dim() == 1 && fovy.size(0) == V, who, ": fovy must be [V] = [", V, "], got ", fovy.sizes());
        const auto dev = framebuffer_data->output_rgb.device();
        return {R.to(dev, torch::kFloat32).contiguous(), centers.to(dev, torch::kFloat32).contiguous(), fovy.to(dev, torch::kFloat32).contiguous(), V};
    }
    std::vector<Tensor> render_views(Tensor R, Tensor centers, Tensor fovy, double znear, double zfar, int64_t samples_per_view, std::vector<std::string> outputs) {
        const auto opts = framebuffer_data->output_rgb.options();
        const int64_t V = R.dim() == 3 ? R.size(0) : 0;
        std::vector<Tensor> bufs;
        for (const auto &name : outputs) {
            const int64_t ch = view_output_channels(name);
            TORCH_CHECK(ch != 0, "render_views: unknown output '", name, "' (final, rgb, depth, normal, f0, roughness)");
            bufs.push_back(name == "final" ? torch::zeros({V, height, width, 3}, opts) : torch::zeros({V, EGR_NUM_STEPS, height, width, ch}, opts));
        }
        render_views_into(R, centers, fovy, znear, zfar, samples_per_view, outputs, bufs);
        return bufs;
    }
    void render_views_into(Tensor R, Tensor centers, Tensor fovy, double znear, double zfar, int64_t samples_per_view, std::vector<std::string> outputs,
                           std::vector<Tensor> buffers) {
        const auto [r, cc, fv, V] = batch_cameras("render_views", R, centers, fovy);
        TORCH_CHECK(samples_per_view >= 0 && samples_per_view <= 0x7FFFFFFF, "render_views: samples_per_view out of range");
        TORCH_CHECK(outputs.size() == buffers.size(), "render_views_into: one buffer per output name expected");
        const auto dev = framebuffer_data->output_rgb.device();
        egr_view_batch b{};
        b.num_views = (uint32_t)V, b.samples_per_view = (uint32_t)samples_per_view;
        b.rotation_c2w_dataset = r.data_ptr<float>(), b.camera_center = cc.data_ptr<float>(), b.vertical_fov_radians = fv.data_ptr<float>();
        b.znear = (float)znear, b.zfar = (float)zfar;
        for (size_t i = 0; i < outputs.size(); i++) {
            const std::string &name = outputs[i];
            const int64_t ch = view_output_channels(name);
            TORCH_CHECK(ch != 0, "render_views: unknown output '", name, "' (final, rgb, depth, normal, f0, roughness)");
            const Tensor &t = buffers[i];
            const std::vector<int64_t> want = name == "final" ? std::vector<int64_t>{V, height, width, 3} : std::vector<int64_t>{V, EGR_NUM_STEPS, height, width, ch};
            TORCH_CHECK(t.device() == dev && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.sizes() == torch::IntArrayRef(want), "render_views: output '", name,
                        "' must be a contiguous fp32 tensor ", torch::IntArrayRef(want), " on the tracer's device, got ", t.sizes());
            float **slot = name == "final" ? &b.final : name == "rgb" ? &b.rgb : name == "depth" ? &b.depth : name == "normal" ? &b.normal : name == "f0" ? &b.f0 : &b.roughness;
            TORCH_CHECK(*slot == nullptr, "render_views: output '", name, "' requested twice");
            *slot = t.data_ptr<float>();
        }
        check(egr_render_views(ctx, &b, current_stream()), "render_views");
    }
    // per-object coverage of one view (egr_object_masks): R [3,3], center [3] (any device, moved and converted like render_views'), row_bits int32 [N] on the
    // tracer's device (editing.EditableGaussians.selection_mask), bits = the requested selection bits in output order. Returns (masks [K,H,W] fp32,
    // hit int32 [H,W] - bit j = masks[j] != 0, output index 31 is the sign bit -, top int32 [H,W]). A query: nothing else of the tracer changes.
    std::tuple<Tensor, Tensor, Tensor> object_masks(Tensor R, Tensor center, double fovy, double znear, double zfar, Tensor row_bits, std::vector<int64_t> bits) {
        TORCH_CHECK(R.dim() == 2 && R.size(0) == 3 && R.size(1) == 3 && center.numel() == 3, "object_masks: R [3,3] and center [3] expected");
        const auto dev = framebuffer_data->output_rgb.device();
        TORCH_CHECK(row_bits.device() == dev && row_bits.scalar_type() == torch::kInt32 && row_bits.dim() == 1 && row_bits.is_contiguous() &&
                        row_bits.size(0) == gaussian_data->mean.size(0),
                    "object_masks: row_bits must be a contiguous int32 tensor [", gaussian_data->mean.size(0), "] on the tracer's device, got ", row_bits.sizes(), " ", row_bits.scalar_type(), " on ", row_bits.device());
        TORCH_CHECK(!bits.empty() && bits.size() <= EGR_MAX_EDIT_OBJECTS, "object_masks: 1 .. ", EGR_MAX_EDIT_OBJECTS, " bits expected, got ", bits.size());
        uint8_t b8[EGR_MAX_EDIT_OBJECTS];
        for (size_t j = 0; j < bits.size(); j++) {
            TORCH_CHECK(bits[j] >= 0 && bits[j] < 256, "object_masks: bit ", bits[j], " out of range");
            b8[j] = (uint8_t)bits[j];
        }
        const auto [r, cc, fv, V] = batch_cameras("object_masks", R.unsqueeze(0), center.reshape({1, 3}), torch::full({1}, fovy, torch::dtype(torch::kFloat32)));
        (void)V;
        const auto fopts = framebuffer_data->output_rgb.options();
        Tensor masks = torch::zeros({(int64_t)bits.size(), height, width}, fopts);
        Tensor hit = torch::zeros({height, width}, fopts.dtype(torch::kInt32)), top = torch::full({height, width}, -1, fopts.dtype(torch::kInt32));
        egr_object_mask_query q{};
        q.rotation_c2w_dataset = r.data_ptr<float>(), q.camera_center = cc.data_ptr<float>(), q.vertical_fov_radians = fv.data_ptr<float>();
        q.znear = (float)znear, q.zfar = (float)zfar;
        q.row_bits = reinterpret_cast<const uint32_t *>(row_bits.data_ptr<int32_t>());
        q.bits = b8, q.num_bits = (uint32_t)bits.size();
        q.masks = masks.data_ptr<float>(), q.hit = reinterpret_cast<uint32_t *>(hit.data_ptr<int32_t>()), q.top = top.data_ptr<int32_t>();
        check(egr_object_masks(ctx, &q, current_stream()), "object_masks");
        return {masks, hit, top};
    }
    // multi-view training launch (egr_train_views): R [V,3,3], centers [V,3], fovy [V] as for render_views; the six targets are channel-major [V,C,H,W]
    // fp32 tensors on the tracer's device (C = 3, depth / roughness 1; None or an empty tensor = absent = zeros). Adds the gradients of the V views to
    // the gradient tensors (or the per-launch buffer: one grad launch for the whole batch) as V sequential raytrace() calls with grad mode on would.
    void train_views(Tensor R, Tensor centers, Tensor fovy, double znear, double zfar, c10::optional<Tensor> diffuse, c10::optional<Tensor> specular,
                     c10::optional<Tensor> depth, c10::optional<Tensor> normal, c10::optional<Tensor> roughness, c10::optional<Tensor> f0) {
        train_views_import(R, centers, fovy, znear, zfar, diffuse, specular, depth, normal, roughness, f0, c10::nullopt);
    }
    // ... with raytrace()'s import_into: the batch's one gather also adds to the caller's eight gradient tensors (egr_train_views_import)
    void train_views_import(Tensor R, Tensor centers, Tensor fovy, double znear, double zfar, c10::optional<Tensor> diffuse, c10::optional<Tensor> specular,
                            c10::optional<Tensor> depth, c10::optional<Tensor> normal, c10::optional<Tensor> roughness, c10::optional<Tensor> f0,
                            c10::optional<std::vector<Tensor>> import_into) {
        const auto [r, cc, fv, V] = batch_cameras("train_views", R, centers, fovy);
        const auto dev = framebuffer_data->output_rgb.device();
        egr_train_batch b{};
        b.num_views = (uint32_t)V;
        b.rotation_c2w_dataset = r.data_ptr<float>(), b.camera_center = cc.data_ptr<float>(), b.vertical_fov_radians = fv.data_ptr<float>();
        b.znear = (float)znear, b.zfar = (float)zfar;
        const c10::optional<Tensor> *in[6] = {&diffuse, &specular, &depth, &normal, &roughness, &f0};
        const float **slot[6] = {&b.target_diffuse, &b.target_specular, &b.target_depth, &b.target_normal, &b.target_roughness, &b.target_f0};
        for (int k = 0; k < 6; k++) {
            if (!in[k]->has_value() || !(*in[k])->defined() || (*in[k])->numel() == 0) continue;
            const Tensor &t = **in[k];
            const std::vector<int64_t> want{V, TARGETS[k].channels, height, width};
            TORCH_CHECK(t.device() == dev && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.sizes() == torch::IntArrayRef(want), "train_views: target '", TARGETS[k].name,
                        "' must be a contiguous fp32 tensor ", torch::IntArrayRef(want), " (channel-major) on the tracer's device, got ", t.sizes(), " ", t.scalar_type(), " on ", t.device());
            *slot[k] = t.data_ptr<float>();
        }
        if (import_into.has_value()) {
            const egr_gaussians dst = import_target("train_views", *import_into);
            check(egr_train_views_import(ctx, &b, &dst, current_stream()), "train_views");
        } else {
            check(egr_train_views(ctx, &b, current_stream()), "train_views");
        }
    }
    // batched denoise (egr_denoise_views): final [V,H,W,3] and its guide normal - render_views' [V,3,H,W,3] buffer (step 0 is the guide) or a packed [V,H,W,3] -
    // as contiguous fp32 tensors on the tracer's device. Returns a new [V,H,W,3] tensor; each view is bit-equal to denoise() on a framebuffer that holds the same
    // final / normal. The framebuffer is not touched.
    Tensor denoise_views(Tensor final, Tensor normal) {
        const auto dev = framebuffer_data->output_rgb.device();
        TORCH_CHECK(final.dim() == 4 && final.size(1) == height && final.size(2) == width && final.size(3) == 3, "denoise_views: final must be [V,", height, ",", width, ",3], got ", final.sizes());
        const int64_t V = final.size(0);
        const bool steps = normal.dim() == 5;
        const std::vector<int64_t> want = steps ? std::vector<int64_t>{V, EGR_NUM_STEPS, height, width, 3} : std::vector<int64_t>{V, height, width, 3};
        TORCH_CHECK(normal.sizes() == torch::IntArrayRef(want), "denoise_views: normal must be [V,3,H,W,3] or [V,H,W,3] with V = ", V, ", got ", normal.sizes());
        for (const Tensor *t : {&final, &normal})
            TORCH_CHECK(t->device() == dev && t->scalar_type() == torch::kFloat32 && t->is_contiguous(), "denoise_views: contiguous fp32 tensors on the tracer's device expected");
        Tensor out = torch::empty_like(final);
        if (V == 0) return out;
        check(egr_denoise_views(ctx, (uint32_t)V, final.data_ptr<float>(), normal.data_ptr<float>(), (size_t)((steps ? EGR_NUM_STEPS : 1) * height * width * 3), out.data_ptr<float>(),
                                current_stream()),
              "denoise_views");
        return out;
    }
    void set_batch_frames(int64_t n) { TORCH_CHECK(n >= 1 && n <= 0x7FFFFFFF && egr_set_batch_frames(ctx, (int)n) == 0, "set_batch_frames: a frame count >= 1 expected"); }
    void set_rays_per_task(int64_t n) { TORCH_CHECK(egr_set_rays_per_task(ctx, (int)n) == 0, "set_rays_per_task: 0 (automatic), 16, 32 or 64 expected"); }
    void set_team_help(bool on) { TORCH_CHECK(egr_set_team_help(ctx, on ? 1 : 0) == 0, "set_team_help failed"); }
    void set_team_help_auto() { TORCH_CHECK(egr_set_team_help(ctx, -1) == 0, "set_team_help_auto failed"); } // on for under-filled ranks of a partition only (egr_set_team_help(-1))
    void set_strands(int64_t n) { TORCH_CHECK(egr_set_strands(ctx, (int)n) == 0, "set_strands: only 1 is accepted (strands were removed; every launch runs on the caller's stream)"); }
    std::vector<int64_t> get_counters() { // synchronises
        egr_counters c{};
        check(egr_get_counters(ctx, &c, current_stream()), "get_counters");
        // [rays0..2, candidates0..2, composited0..2, lifetime_rays, lifetime_launches, status, bvh_depth, bucket_records, device_bytes, arena_blocks_used, arena_blocks_cap,
        //  ext_blocks_used, ext_blocks_cap, accepted0..2]
        return {(int64_t)c.rays[0], (int64_t)c.rays[1], (int64_t)c.rays[2], (int64_t)c.candidates[0], (int64_t)c.candidates[1],
                (int64_t)c.candidates[2], (int64_t)c.composited[0], (int64_t)c.composited[1], (int64_t)c.composited[2],
                (int64_t)c.lifetime_rays, (int64_t)c.lifetime_launches, (int64_t)c.status, (int64_t)c.bvh_depth, (int64_t)c.bucket_records,
                (int64_t)c.device_bytes, (int64_t)c.arena_blocks_used, (int64_t)c.arena_blocks_cap, (int64_t)c.ext_blocks_used, (int64_t)c.ext_blocks_cap,
                (int64_t)c.accepted[0], (int64_t)c.accepted[1], (int64_t)c.accepted[2]};
    }
    void reset_lifetime_counters() { check(egr_reset_lifetime_counters(ctx, current_stream()), "reset_lifetime_counters"); }
    void enable_timing(bool on) { egr_enable_timing(ctx, on ? 1 : 0); }
    double last_raytrace_ms() { return egr_last_raytrace_ms(ctx); }
    double last_update_bvh_ms() { return egr_last_update_bvh_ms(ctx); }
    std::vector<std::tuple<std::string, double>> last_kernel_ms() {
        float ms[32];
        const char *names[32];
        int n = egr_last_kernel_ms(ctx, ms, names, 32);
        std::vector<std::tuple<std::string, double>> out;
        for (int i = 0; i < n; i++) out.emplace_back(std::string(names[i]), (double)ms[i]);
        return out;
    }
    Tensor debug_step_hits() { // [3,H,W] int32 on the host: composited hits per bounce step of the last grad launch
        Tensor t = torch::zeros({EGR_NUM_STEPS, height, width}, torch::kInt32);
        check(egr_debug_get_step_hits(ctx, t.data_ptr<int32_t>(), current_stream()), "debug_step_hits");
        return t;
    }
    Tensor debug_hit_sequence_hash() { // [3,H,W] int64 (the bits of the uint64 hashes) on the host: ordered composited gaussian ids per pixel and step of the last grad launch
        Tensor t = torch::zeros({EGR_NUM_STEPS, height, width}, torch::kInt64);
        check(egr_debug_get_hit_sequence_hash(ctx, reinterpret_cast<uint64_t *>(t.data_ptr<int64_t>()), current_stream()), "debug_hit_sequence_hash");
        return t;
    }
    int64_t check_bvh() { return egr_debug_check_bvh(ctx, current_stream()); }
    std::string last_error() { return egr_last_error(ctx); }
    std::vector<Tensor> debug_instances() {
        int64_t n = gaussian_data->count;
        Tensor M = torch::zeros({n, 3, 4}, torch::kFloat32), W = torch::zeros({n, 3, 4}, torch::kFloat32), A = torch::zeros({n, 6}, torch::kFloat32);
        check(egr_debug_get_instances(ctx, M.data_ptr<float>(), W.data_ptr<float>(), A.data_ptr<float>(), current_stream()), "debug_instances");
        return {M, W, A};
    }
    Tensor debug_backward_records() { // [n,4,4] float32 on the host, by gaussian id (egr_debug_get_backward_records)
        float frame[6];
        uint32_t info[4] = {0u, 0u, 0u, 0u}; // (info[3]: the count the tree was built for - the rows the library copies, whatever the holder was resized to since)
        check(egr_debug_get_bvh_state(ctx, frame, info, current_stream()), "debug_backward_records");
        Tensor t = torch::zeros({(int64_t)info[3], 4, 4}, torch::kFloat32);
        check(egr_debug_get_backward_records(ctx, t.data_ptr<float>(), current_stream()), "debug_backward_records");
        return t;
    }
    std::tuple<Tensor, Tensor> debug_bvh_state() { // (float32[6]: the build frame's origin xyz and cells per world unit xyz; int64[4]: out_of_frame flag, wide nodes, depth, n built) on the host
        Tensor f = torch::zeros({6}, torch::kFloat32), i = torch::zeros({4}, torch::kInt64);
        uint32_t info[4] = {0u, 0u, 0u, 0u};
        check(egr_debug_get_bvh_state(ctx, f.data_ptr<float>(), info, current_stream()), "debug_bvh_state");
        for (int k = 0; k < 4; k++) i.data_ptr<int64_t>()[k] = (int64_t)info[k];
        return {f, i};
    }
    // The built tree on the host (egr_debug_get_tree), in this order: keys int64 [n] (the bits of the uint64 keys), gid_of_pos int32 [n], pos_of_gid int32 [n],
    // left int32 [n-1], right int32 [n-1], dp float32 [n-1,16], wnodes int32 [nw,8,4] (the bits of the uint32 words), bsph float32 [n,4], level_start int32 [depth+1]
    std::vector<Tensor> debug_tree() {
        float frame[6];
        uint32_t info[4] = {0u, 0u, 0u, 0u};
        check(egr_debug_get_bvh_state(ctx, frame, info, current_stream()), "debug_tree");
        const int64_t n = info[3], nb = n > 1 ? n - 1 : 0, nw = info[1], levels = (int64_t)info[2] + 1;
        Tensor keys = torch::zeros({n}, torch::kInt64), gop = torch::zeros({n}, torch::kInt32), pog = torch::zeros({n}, torch::kInt32);
        Tensor left = torch::zeros({nb}, torch::kInt32), right = torch::zeros({nb}, torch::kInt32), dp = torch::zeros({nb, 16}, torch::kFloat32);
        Tensor wn = torch::zeros({nw, 8, 4}, torch::kInt32), bs = torch::zeros({n, 4}, torch::kFloat32), ls = torch::zeros({levels}, torch::kInt32);
        auto u32 = [](Tensor &t) { return reinterpret_cast<uint32_t *>(t.data_ptr<int32_t>()); };
        check(egr_debug_get_tree(ctx, reinterpret_cast<uint64_t *>(keys.data_ptr<int64_t>()), u32(gop), u32(pog), left.data_ptr<int32_t>(), right.data_ptr<int32_t>(),
                                 dp.data_ptr<float>(), u32(wn), bs.data_ptr<float>(), u32(ls), current_stream()),
              "debug_tree");
        return {keys, gop, pog, left, right, dp, wn, bs, ls};
    }

    static void bind(torch::Library &m) {
        using Self = c10::intrusive_ptr<Raytracer>;
        m.class_<Raytracer>("Raytracer")
            .def(torch::init<int64_t, int64_t, int64_t, int64_t, int64_t>())
            .def("raytrace", &Raytracer::raytrace, "", {torch::arg("import_into") = c10::IValue(), torch::arg("targets") = c10::IValue()})
            .def("denoise", &Raytracer::denoise)
            .def("reset_accumulators", &Raytracer::reset_accumulators)
            .def("update_bvh", &Raytracer::update_bvh, "", {torch::arg("fuse_live") = false})
            .def("update_bvh_from", &Raytracer::update_bvh_from)
            .def("rebuild_bvh", &Raytracer::rebuild_bvh)
            .def("resize", &Raytracer::resize)
            .def("get_camera", [](const Self &self) { return self->camera_data; })
            .def("get_config", [](const Self &self) { return self->config_data; })
            .def("get_framebuffer", [](const Self &self) { return self->framebuffer_data; })
            .def("get_gaussians", [](const Self &self) { return self->gaussian_data; })
            .def("get_metadata", [](const Self &self) { return self->meta_data; })
            .def("get_stats", [](const Self &self) { return self->stats_data; })
            .def("get_ppll_forward_data", [](const Self &self) { return self->ppll_forward_data; })
            .def("get_ppll_backward_data", [](const Self &self) { return self->ppll_backward_data; })
            .def_static("MAX_BOUNCES", []() { return (int64_t)EGR_MAX_BOUNCES; })
            .def_static("MAX_ALPHA", []() { return (double)EGR_MAX_ALPHA; })
            .def_static("ROUGHNESS_DOWNWEIGHT_GRAD", []() { return (bool)EGR_ROUGHNESS_DOWNWEIGHT_GRAD; })
            .def_static("ROUGHNESS_DOWNWEIGHT_GRAD_POWER", []() { return (double)EGR_ROUGHNESS_DOWNWEIGHT_GRAD_POWER; })
            .def("describe_output_buffers", // raytracer.cpp:151-167
                 [](const Self &) {
                     std::vector<std::tuple<std::string, int64_t>> t = {
                         {"output_rgb", 3}, {"output_depth", 1}, {"output_normal", 3}, {"output_f0", 3}, {"output_roughness", 1},
                         {"output_transmittance", 1}, {"output_total_transmittance", 1}, {"output_brdf", 3}, {"output_ray_origin", 3},
                         {"output_ray_direction", 3}, {"output_final", 3}};
                     return t;
                 })
            .def("describe_accumulation_buffers", // :168-180
                 [](const Self &) {
                     std::vector<std::tuple<std::string, int64_t>> t = {
                         {"accumulated_rgb", 3}, {"accumulated_transmittance", 1}, {"accumulated_total_transmittance", 1},
                         {"accumulated_depth", 1}, {"accumulated_normal", 3}, {"accumulated_f0", 3}, {"accumulated_roughness", 1}};
                     return t;
                 })
            .def("describe_target_buffers", // :181-190
                 [](const Self &) {
                     std::vector<std::tuple<std::string, int64_t>> t = {
                         {"target_depth", 1}, {"target_normal", 3}, {"target_f0", 3}, {"target_roughness", 1}};
                     return t;
                 })
            .def("describe_gaussian_attributes", // :193-204
                 [](const Self &) {
                     std::vector<std::tuple<std::string, int64_t>> t = {
                         {"gaussian_rgb", 3}, {"gaussian_normal", 3}, {"gaussian_f0", 3}, {"gaussian_roughness", 1},
                         {"gaussian_opacity", 1}, {"gaussian_scale", 3}, {"gaussian_mean", 3}, {"gaussian_rotation", 4}};
                     return t;
                 })
            // additions for multi-GPU tile partitioning, measurement and tests
            .def("set_partition", &Raytracer::set_partition)
            .def("use_grad_delta", &Raytracer::use_grad_delta)
            .def("grad_delta_consumed", &Raytracer::grad_delta_consumed)
            .def("debug_set_pixel_mask", &Raytracer::debug_set_pixel_mask)
            .def("set_targets_chw", &Raytracer::set_targets_chw)
            .def("set_camera", &Raytracer::set_camera)
            .def("render_views", &Raytracer::render_views)
            .def("render_views_into", &Raytracer::render_views_into)
            .def("object_masks", &Raytracer::object_masks)
            .def("train_views", &Raytracer::train_views)
            .def("train_views_import", &Raytracer::train_views_import)
            .def("denoise_views", &Raytracer::denoise_views)
            .def("set_batch_frames", &Raytracer::set_batch_frames)
            .def("set_exact_stats", &Raytracer::set_exact_stats)
            .def("set_strands", &Raytracer::set_strands)
            .def("set_team_help", &Raytracer::set_team_help)
            .def("set_team_help_auto", &Raytracer::set_team_help_auto)
            .def("set_rays_per_task", &Raytracer::set_rays_per_task)
            .def("get_counters", &Raytracer::get_counters)
            .def("reset_lifetime_counters", &Raytracer::reset_lifetime_counters)
            .def("enable_timing", &Raytracer::enable_timing)
            .def("last_raytrace_ms", &Raytracer::last_raytrace_ms)
            .def("last_update_bvh_ms", &Raytracer::last_update_bvh_ms)
            .def("last_kernel_ms", &Raytracer::last_kernel_ms)
            .def("check_bvh", &Raytracer::check_bvh)
            .def("last_error", &Raytracer::last_error)
            .def("debug_instances", &Raytracer::debug_instances)
            .def("debug_backward_records", &Raytracer::debug_backward_records)
            .def("debug_bvh_state", &Raytracer::debug_bvh_state)
            .def("debug_tree", &Raytracer::debug_tree)
            .def("debug_step_hits", &Raytracer::debug_step_hits)
            .def("debug_hit_sequence_hash", &Raytracer::debug_hit_sequence_hash);
    }
};

// simple_knn._C.distCUDA2 (gaussian_model.py:17): float CUDA(HIP) tensor [N,3] -> [N] mean squared distance to the 3 nearest
// neighbours. Registered as torch.ops.simple_knn.distCUDA2; the package's simple_knn.py re-exports it under the reference's name.
static torch::Tensor dist_hip2(const torch::Tensor &points) {
    TORCH_CHECK(points.is_cuda(), "distCUDA2: points must live on the GPU (there is no CPU path)");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "distCUDA2: expected an [N,3] tensor");
    auto p = points.to(torch::kFloat32).contiguous();
    auto out = torch::zeros({p.size(0)}, p.options());
    const int rc = egr_knn_mean_dist2(p.get_device(), p.data_ptr<float>(), (uint32_t)p.size(0), out.data_ptr<float>(), current_stream());
    TORCH_CHECK(rc == 0, egr_knn_last_error());
    return out;
}
// One launch for import + scale decay + Adam + clamps + zero_grad + export (csrc/step.hip). Tensor lists are parallel, one
// entry per parameter group; an undefined / empty tensor means "absent" for grads, rt_params, rt_grads and the Adam moments.
static void fused_adam_step(std::vector<torch::Tensor> params, std::vector<torch::Tensor> grads, std::vector<torch::Tensor> rt_params,
                            std::vector<torch::Tensor> rt_grads, std::vector<torch::Tensor> exp_avg, std::vector<torch::Tensor> exp_avg_sq,
                            std::vector<double> lrs, std::vector<double> clamp_min, std::vector<double> clamp_max, std::vector<double> log_decay,
                            int64_t step, double beta1, double beta2, double eps, std::vector<int64_t> group_steps) {
    const size_t G = params.size();
    TORCH_CHECK(G >= 1 && G <= EGR_MAX_PARAM_GROUPS, "fused_adam_step: 1..8 parameter groups");
    TORCH_CHECK(grads.size() == G && rt_params.size() == G && rt_grads.size() == G && exp_avg.size() == G && exp_avg_sq.size() == G && lrs.size() == G &&
                    clamp_min.size() == G && clamp_max.size() == G && log_decay.size() == G,
                "fused_adam_step: all lists need one entry per group");
    TORCH_CHECK(group_steps.empty() || group_steps.size() == G, "fused_adam_step: group_steps must be empty (every group uses `step`) or hold one count per group");
    egr_param_group g[EGR_MAX_PARAM_GROUPS];
    const int64_t n = params[0].size(0);
    auto ptr = [&](const torch::Tensor &t, const torch::Tensor &like, const char *what) -> float * {
        if (!t.defined() || t.numel() == 0) return nullptr;
        TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.numel() == like.numel(), "fused_adam_step: ", what,
                    " must be a contiguous float GPU tensor of the parameter's size");
        return t.data_ptr<float>();
    };
    for (size_t k = 0; k < G; k++) {
        TORCH_CHECK(params[k].is_cuda() && params[k].scalar_type() == torch::kFloat32 && params[k].is_contiguous() && params[k].size(0) == n,
                    "fused_adam_step: parameters must be contiguous float GPU tensors with the same leading size");
        g[k].param = params[k].data_ptr<float>();
        g[k].grad = ptr(grads[k], params[k], "grad"), g[k].rt_param = ptr(rt_params[k], params[k], "rt_param");
        g[k].rt_grad = ptr(rt_grads[k], params[k], "rt_grad");
        g[k].exp_avg = ptr(exp_avg[k], params[k], "exp_avg"), g[k].exp_avg_sq = ptr(exp_avg_sq[k], params[k], "exp_avg_sq");
        g[k].width = n ? (uint32_t)(params[k].numel() / n) : 1u;
        g[k].lr = (float)lrs[k], g[k].clamp_min = (float)clamp_min[k], g[k].clamp_max = (float)clamp_max[k], g[k].log_decay = (float)log_decay[k];
        g[k].step = group_steps.size() == G ? (uint32_t)group_steps[k] : 0u;
    }
    const int rc = egr_fused_adam_step(params[0].get_device(), g, (int)G, (uint32_t)n, (uint32_t)step, beta1, beta2, eps, current_stream());
    TORCH_CHECK(rc == 0, egr_fused_step_last_error());
}

// Fused prune, part 1 (egr_prune_select, csrc/prune.hip): which rows survive. Every criterion is optional (None = skipped) but at least one of
// total_weight [N] / [N,1], points [N,3], remove_mask [N] (uint8 or bool) must be given - it fixes N. Returns (src_index int32 [N]: the first `count`
// entries are the kept rows, ascending; count int32 [1]) on the device, asynchronously: reading `count` is the caller's one synchronisation.
static std::tuple<Tensor, Tensor> prune_select(const c10::optional<Tensor> &total_weight, double divisor, double min_weight, const c10::optional<Tensor> &points,
                                               const c10::optional<Tensor> &cam_centers, const c10::optional<Tensor> &cam_znear, const c10::optional<Tensor> &remove_mask) {
    auto given = [](const c10::optional<Tensor> &t) { return t.has_value() && t->defined(); };
    int64_t n = -1;
    c10::Device dev(torch::kCUDA);
    auto rows = [&](const Tensor &t, const char *what) {
        TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.dim() >= 1, "prune_select: ", what, " must be a contiguous GPU tensor");
        TORCH_CHECK(n < 0 || (t.size(0) == n && t.device() == dev), "prune_select: ", what, " has ", t.size(0), " rows on ", t.device(), ", expected ", n, " on ", dev);
        n = t.size(0), dev = t.device();
    };
    const float *tw = nullptr, *pts = nullptr, *cc = nullptr, *cz = nullptr;
    const uint8_t *mask = nullptr;
    int64_t num_cams = 0;
    if (given(total_weight)) {
        rows(*total_weight, "total_weight");
        TORCH_CHECK(total_weight->scalar_type() == torch::kFloat32 && total_weight->numel() == n, "prune_select: total_weight must be fp32 [N] or [N,1]");
        tw = total_weight->data_ptr<float>();
    }
    if (given(points)) {
        rows(*points, "points");
        TORCH_CHECK(points->scalar_type() == torch::kFloat32 && points->dim() == 2 && points->size(1) == 3, "prune_select: points must be fp32 [N,3]");
        pts = points->data_ptr<float>();
    }
    if (given(remove_mask)) {
        rows(*remove_mask, "remove_mask");
        TORCH_CHECK((remove_mask->scalar_type() == torch::kUInt8 || remove_mask->scalar_type() == torch::kBool) && remove_mask->numel() == n, "prune_select: remove_mask must be uint8 or bool [N]");
        mask = reinterpret_cast<const uint8_t *>(remove_mask->data_ptr());
    }
    TORCH_CHECK(n >= 0, "prune_select: one of total_weight, points, remove_mask is required (it fixes the number of rows)");
    TORCH_CHECK(given(cam_centers) == given(cam_znear), "prune_select: cam_centers and cam_znear go together");
    if (given(cam_centers)) {
        TORCH_CHECK(pts != nullptr, "prune_select: the camera criterion needs points");
        num_cams = cam_znear->numel();
        TORCH_CHECK(cam_centers->is_cuda() && cam_centers->device() == dev && cam_centers->scalar_type() == torch::kFloat32 && cam_centers->is_contiguous() && cam_centers->dim() == 2 &&
                        cam_centers->size(0) == num_cams && cam_centers->size(1) == 3,
                    "prune_select: cam_centers must be a contiguous fp32 [C,3] tensor on the points' device");
        TORCH_CHECK(cam_znear->is_cuda() && cam_znear->device() == dev && cam_znear->scalar_type() == torch::kFloat32 && cam_znear->is_contiguous() && cam_znear->dim() == 1,
                    "prune_select: cam_znear must be a contiguous fp32 [C] tensor on the points' device");
        cc = cam_centers->data_ptr<float>(), cz = cam_znear->data_ptr<float>();
    }
    TORCH_CHECK(n <= (int64_t)0xFFFFFFFFll, "prune_select: too many rows");
    const auto i32 = torch::dtype(torch::kInt32).device(dev);
    Tensor src_index = torch::empty({n}, i32), count = torch::zeros({1}, i32);
    if (n == 0) return {src_index, count}; // (no rows: count 0, nothing to launch)
    Tensor workspace = torch::empty({(int64_t)(EGR_PRUNE_WORKSPACE_BYTES(n) + 7) / 8}, torch::dtype(torch::kInt64).device(dev)); // (freed stream-ordered by the caching allocator)
    const int rc = egr_prune_select(dev.index(), (uint32_t)n, tw, (float)divisor, (float)min_weight, pts, cc, cz, (uint32_t)num_cams, mask,
                                    reinterpret_cast<uint32_t *>(src_index.data_ptr<int32_t>()), reinterpret_cast<uint32_t *>(count.data_ptr<int32_t>()),
                                    workspace.data_ptr(), current_stream());
    TORCH_CHECK(rc == 0, egr_prune_last_error());
    return {src_index, count};
}
// Fused prune, part 2 (egr_prune_gather): out[k] = src[k][src_index[:count]] for every tensor of `src` - contiguous GPU tensors of 4-byte elements (fp32,
// int32) with the same leading size - as one launch per EGR_MAX_PRUNE_ARRAYS tensors over the same index list. The outputs are new tensors of the source's
// dtype and trailing shape with `count` rows.
static std::vector<Tensor> prune_gather(std::vector<Tensor> src, const Tensor &src_index, int64_t count) {
    TORCH_CHECK(src_index.is_cuda() && src_index.scalar_type() == torch::kInt32 && src_index.is_contiguous() && src_index.dim() == 1, "prune_gather: src_index must be the int32 list of prune_select");
    TORCH_CHECK(count >= 0 && count <= src_index.numel(), "prune_gather: count must be in 0..", src_index.numel());
    std::vector<Tensor> out;
    if (src.empty()) return out;
    const int64_t n = src[0].dim() >= 1 ? src[0].size(0) : -1;
    TORCH_CHECK(n == src_index.numel(), "prune_gather: the tensors need the ", src_index.numel(), " rows the index list was selected from");
    std::vector<egr_prune_array> table;
    for (const Tensor &t : src) {
        TORCH_CHECK(t.is_cuda() && t.device() == src_index.device() && t.is_contiguous() && t.element_size() == 4 && t.dim() >= 1 && t.size(0) == n,
                    "prune_gather: contiguous GPU tensors of 4-byte elements with the same leading size are required");
        auto shape = t.sizes().vec();
        shape[0] = count;
        out.push_back(torch::empty(shape, t.options()));
        const int64_t width = n ? t.numel() / n : 1;
        if (width == 0) continue; // (a [N,0] tensor has no elements to move)
        table.push_back(egr_prune_array{t.data_ptr(), out.back().data_ptr(), (uint32_t)width});
    }
    if (n == 0 || count == 0) return out; // (empty tensors have no storage to hand to the library)
    for (size_t k0 = 0; k0 < table.size(); k0 += EGR_MAX_PRUNE_ARRAYS) {
        const int rc = egr_prune_gather(src_index.get_device(), table.data() + k0, (int)std::min<size_t>(EGR_MAX_PRUNE_ARRAYS, table.size() - k0), (uint32_t)n,
                                        reinterpret_cast<const uint32_t *>(src_index.data_ptr<int32_t>()), (uint32_t)count, current_stream());
        TORCH_CHECK(rc == 0, egr_prune_last_error());
    }
    return out;
}

// Growing the cloud, part 1 (egr_grow_sample, csrc/grow.hip): candidates first .. first + n of the far-field cloud as a new fp32 [n,3] tensor on `device`, on
// the current stream. `first` and `seed` are unsigned 64-bit values carried in the schema's int (their bits: 2^63 + 5 is passed as -2^63 + 5).
static Tensor grow_sample(int64_t first, int64_t n, int64_t seed, double radius, double clamp, c10::Device device) {
    TORCH_CHECK(device.is_cuda(), "grow_sample: device must be a GPU (there is no CPU path), got ", device);
    TORCH_CHECK(n >= 0 && n <= ((int64_t)1 << 26), "grow_sample: n must be in 0..2^26 (the limit of the tree), got ", n);
    const c10::Device dev(torch::kCUDA, device.has_index() ? device.index() : c10::hip::current_device());
    const c10::DeviceGuard guard(dev); // the output and current_stream() belong to `device`, which need not be the current one
    Tensor out = torch::empty({n, 3}, torch::dtype(torch::kFloat32).device(dev));
    if (n == 0) return out; // (an empty tensor has no storage to hand to the library)
    const int rc = egr_grow_sample(dev.index(), (uint64_t)first, (uint32_t)n, (uint64_t)seed, (float)radius, (float)clamp, out.data_ptr<float>(), current_stream());
    TORCH_CHECK(rc == 0, egr_grow_last_error());
    return out;
}
// Growing the cloud, part 2 (egr_grow_append): out[k] = cat(src[k], new rows) for every tensor of `src` - contiguous GPU tensors of 4-byte elements with the
// same leading size n - as one launch per EGR_MAX_PRUNE_ARRAYS tensors. The m new rows of entry k are tail[k] (same dtype and trailing shape, m rows) or,
// where tail[k] is None, the word fill_bits[k] in every element (an fp32's or int32's bits, -2^31 .. 2^32 - 1). The outputs are new tensors.
static std::vector<Tensor> grow_append(std::vector<Tensor> src, const c10::List<c10::optional<Tensor>> &tail, std::vector<int64_t> fill_bits, int64_t m) {
    TORCH_CHECK(tail.size() == src.size() && fill_bits.size() == src.size(), "grow_append: src, tail and fill_bits must have one entry per tensor (", src.size(), ", ",
                tail.size(), ", ", fill_bits.size(), ")");
    std::vector<Tensor> out;
    if (src.empty()) return out;
    const int64_t n = src[0].dim() >= 1 ? src[0].size(0) : -1;
    TORCH_CHECK(n >= 0, "grow_append: tensors with a leading (row) dimension are required");
    TORCH_CHECK(m >= 0 && n + m <= ((int64_t)1 << 26), "grow_append: m must be >= 0 and n + m <= 2^26 rows (the limit of the tree), got n = ", n, ", m = ", m);
    const c10::Device dev = src[0].device();
    const c10::DeviceGuard guard(dev);
    std::vector<egr_grow_array> table;
    for (size_t k = 0; k < src.size(); k++) {
        const Tensor &t = src[k];
        TORCH_CHECK(t.is_cuda() && t.device() == dev && t.is_contiguous() && t.element_size() == 4 && t.dim() >= 1 && t.size(0) == n,
                    "grow_append: contiguous GPU tensors of 4-byte elements with the same leading size are required (src[", k, "])");
        TORCH_CHECK(fill_bits[k] >= -((int64_t)1 << 31) && fill_bits[k] < ((int64_t)1 << 32), "grow_append: fill_bits[", k, "] is not a 32-bit word");
        auto shape = t.sizes().vec();
        int64_t width = 1;
        for (size_t d = 1; d < shape.size(); d++) width *= shape[d];
        shape[0] = n + m;
        egr_grow_array e{n ? t.data_ptr() : nullptr, nullptr, nullptr, (uint32_t)width, EGR_GROW_TAIL_FILL, (uint32_t)(uint64_t)fill_bits[k]};
        const c10::optional<Tensor> add = tail.get(k);
        if (add.has_value() && add->defined()) {
            auto want = shape;
            want[0] = m;
            TORCH_CHECK(add->is_cuda() && add->device() == dev && add->is_contiguous() && add->scalar_type() == t.scalar_type() && add->sizes().vec() == want,
                        "grow_append: tail[", k, "] must be a contiguous ", t.scalar_type(), " tensor ", c10::IntArrayRef(want), " on ", dev, ", got ", add->scalar_type(), " ",
                        add->sizes(), " on ", add->device());
            e.tail = m ? add->data_ptr() : nullptr, e.tail_kind = EGR_GROW_TAIL_ROWS;
        }
        out.push_back(torch::empty(shape, t.options()));
        if (width == 0) continue; // (a [N,0] tensor has no elements to move)
        e.dst = out.back().data_ptr();
        table.push_back(e);
    }
    if (n + m == 0) return out; // (empty tensors have no storage to hand to the library)
    for (size_t k0 = 0; k0 < table.size(); k0 += EGR_MAX_PRUNE_ARRAYS) {
        const int rc = egr_grow_append(dev.index(), table.data() + k0, (int)std::min<size_t>(EGR_MAX_PRUNE_ARRAYS, table.size() - k0), (uint32_t)n, (uint32_t)m, current_stream());
        TORCH_CHECK(rc == 0, egr_grow_last_error());
    }
    return out;
}

// Scene editing, part 1 (egr_edit_select, csrc/edit.hip): the membership mask of up to 32 objects. `objects`: a CPU int32 tensor [K, 17] holding K
// egr_edit_object records as bits (editing.py packs them); xyz fp32 [N,3] on the GPU; f0 [N,3], roughness [N,1], diffuse [N,3] only where an object has
// that property range. Returns int32 [N] (bit k = row belongs to object k) on the current stream, no host synchronisation.
static Tensor edit_select(const Tensor &xyz, const c10::optional<Tensor> &f0, const c10::optional<Tensor> &roughness, const c10::optional<Tensor> &diffuse, const Tensor &objects) {
    TORCH_CHECK(xyz.is_cuda() && xyz.scalar_type() == torch::kFloat32 && xyz.is_contiguous() && xyz.dim() == 2 && xyz.size(1) == 3, "edit_select: xyz must be a contiguous fp32 [N,3] GPU tensor");
    const int64_t n = xyz.size(0);
    TORCH_CHECK(n <= (int64_t)1 << 26, "edit_select: n exceeds 2^26 rows (the limit of the tree)");
    TORCH_CHECK(!objects.is_cuda() && objects.scalar_type() == torch::kInt32 && objects.is_contiguous() && objects.dim() == 2 &&
                    objects.size(1) == (int64_t)(sizeof(egr_edit_object) / 4),
                "edit_select: objects must be a contiguous CPU int32 [K,", sizeof(egr_edit_object) / 4, "] tensor (egr_edit_object records)");
    TORCH_CHECK(objects.size(0) <= EGR_MAX_EDIT_OBJECTS, "edit_select: at most ", EGR_MAX_EDIT_OBJECTS, " objects");
    auto ptr = [&](const c10::optional<Tensor> &t, int64_t width, const char *what) -> const float * {
        if (!t.has_value() || !t->defined()) return nullptr;
        TORCH_CHECK(t->is_cuda() && t->device() == xyz.device() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->numel() == n * width,
                    "edit_select: ", what, " must be a contiguous fp32 [N,", width, "] tensor on xyz's device");
        return t->data_ptr<float>();
    };
    const float *pf0 = ptr(f0, 3, "f0"), *pr = ptr(roughness, 1, "roughness"), *pd = ptr(diffuse, 3, "diffuse");
    Tensor mask = torch::empty({n}, torch::dtype(torch::kInt32).device(xyz.device()));
    if (n == 0) return mask; // (no rows: nothing to launch)
    const int rc = egr_edit_select(xyz.get_device(), (uint32_t)n, xyz.data_ptr<float>(), pf0, pr, pd, reinterpret_cast<const egr_edit_object *>(objects.data_ptr<int32_t>()),
                                   (uint32_t)objects.size(0), reinterpret_cast<uint32_t *>(mask.data_ptr<int32_t>()), current_stream());
    TORCH_CHECK(rc == 0, egr_edit_last_error());
    return mask;
}
// Scene editing, part 2 (egr_edit_apply): edit and export in one launch. `src` / `dst`: eight contiguous fp32 GPU tensors each, in the export order
// scale [N,3], rotation [N,4], mean [N,3], opacity [N,1], rgb [N,3], normal [N,3], roughness [N,1], f0 [N,3]; dst[k] may be src[k] itself. `mask`: the int32 [N]
// tensor of edit_select; `records`: a GPU int32 tensor [K, 43] holding K egr_edit_record records as bits. Current stream, no host synchronisation.
static void edit_apply(std::vector<Tensor> src, std::vector<Tensor> dst, const Tensor &mask, const Tensor &records) {
    static const int64_t width[8] = {3, 4, 3, 1, 3, 3, 1, 3};
    TORCH_CHECK(src.size() == 8 && dst.size() == 8, "edit_apply: src and dst are eight tensors each (scale, rotation, mean, opacity, rgb, normal, roughness, f0)");
    TORCH_CHECK(src[0].dim() >= 1, "edit_apply: tensors with rows are required");
    const int64_t n = src[0].size(0);
    TORCH_CHECK(n <= (int64_t)1 << 26, "edit_apply: n exceeds 2^26 rows (the limit of the tree)");
    const auto dev = src[0].device();
    egr_edit_arrays s{}, d{};
    float **sp = &s.scale, **dp = &d.scale;
    for (int k = 0; k < 8; k++) {
        for (const Tensor *t : {&src[k], &dst[k]})
            TORCH_CHECK(t->is_cuda() && t->device() == dev && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->dim() >= 1 && t->size(0) == n && t->numel() == n * width[k],
                        "edit_apply: tensor ", k, " must be a contiguous fp32 [N,", width[k], "] GPU tensor");
        sp[k] = src[k].data_ptr<float>(), dp[k] = dst[k].data_ptr<float>();
    }
    TORCH_CHECK(records.is_cuda() && records.device() == dev && records.scalar_type() == torch::kInt32 && records.is_contiguous() && records.dim() == 2 &&
                    records.size(1) == (int64_t)(sizeof(egr_edit_record) / 4) && records.size(0) <= EGR_MAX_EDIT_OBJECTS,
                "edit_apply: records must be a contiguous GPU int32 [K <= 32,", sizeof(egr_edit_record) / 4, "] tensor (egr_edit_record records)");
    TORCH_CHECK(mask.is_cuda() && mask.device() == dev && mask.scalar_type() == torch::kInt32 && mask.is_contiguous() && mask.dim() == 1 && mask.size(0) == n,
                "edit_apply: mask must be the int32 [N] tensor of edit_select");
    if (n == 0) return; // (empty tensors have no storage to hand to the library)
    const int rc = egr_edit_apply(dev.index(), (uint32_t)n, &s, &d, reinterpret_cast<const uint32_t *>(mask.data_ptr<int32_t>()),
                                  records.size(0) ? reinterpret_cast<const egr_edit_record *>(records.data_ptr<int32_t>()) : nullptr, (uint32_t)records.size(0), current_stream());
    TORCH_CHECK(rc == 0, egr_edit_last_error());
}

// Fused evaluation metrics (egr_eval_metrics, csrc/eval.hip): final [V,H,W,3], rgb [V,3,H,W,3] (None when both of its targets are) and the channel-major targets
// [V,3,H,W] (None: the pass is skipped and reports NaN) as contiguous fp32 GPU tensors. Returns (sse fp64 [V,3,3], psnr fp64 [V,3,2], display fp32 [V,3,2,3,H,W] -
// or an empty tensor without want_display; a skipped pass reads NaN there) on the device, two launches on the current stream, no host synchronisation.
static std::tuple<Tensor, Tensor, Tensor> eval_metrics(const Tensor &final, const c10::optional<Tensor> &rgb, const c10::optional<Tensor> &target_final,
                                                       const c10::optional<Tensor> &target_diffuse, const c10::optional<Tensor> &target_specular, bool want_display) {
    TORCH_CHECK(final.is_cuda() && final.scalar_type() == torch::kFloat32 && final.is_contiguous() && final.dim() == 4 && final.size(3) == 3, "eval_metrics: final must be a contiguous fp32 [V,H,W,3] GPU tensor");
    const int64_t V = final.size(0), H = final.size(1), W = final.size(2);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && H <= 0x7FFFFFFF && W <= 0x7FFFFFFF, "eval_metrics: at least one view and one pixel are required");
    const auto dev = final.device();
    const c10::DeviceGuard guard(dev); // the outputs, the workspace and current_stream() belong to final's device, which need not be the current one
    auto ptr = [&](const c10::optional<Tensor> &t, std::vector<int64_t> want, const char *what) -> const float * {
        if (!t.has_value() || !t->defined()) return nullptr;
        TORCH_CHECK(t->is_cuda() && t->device() == dev && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->sizes() == torch::IntArrayRef(want), "eval_metrics: ", what,
                    " must be a contiguous fp32 tensor ", torch::IntArrayRef(want), " on final's device, got ", t->sizes());
        return t->data_ptr<float>();
    };
    const float *prgb = ptr(rgb, {V, EGR_NUM_STEPS, H, W, 3}, "rgb");
    const float *tf = ptr(target_final, {V, 3, H, W}, "target_final"), *td = ptr(target_diffuse, {V, 3, H, W}, "target_diffuse"), *ts = ptr(target_specular, {V, 3, H, W}, "target_specular");
    const auto f64 = torch::dtype(torch::kFloat64).device(dev);
    Tensor sse = torch::empty({V, 3, 3}, f64), psnr = torch::empty({V, 3, 2}, f64);
    Tensor display = torch::empty({0}, final.options());
    if (want_display) display = (tf && td && ts) ? torch::empty({V, 3, 2, 3, H, W}, final.options()) : torch::full({V, 3, 2, 3, H, W}, NAN, final.options());
    Tensor workspace = torch::empty({(int64_t)(EGR_EVAL_WORKSPACE_BYTES(V, H, W) / 8)}, f64); // (freed stream-ordered by the caching allocator)
    const int rc = egr_eval_metrics(dev.index(), (uint32_t)V, (uint32_t)H, (uint32_t)W, final.data_ptr<float>(), prgb, tf, td, ts, sse.data_ptr<double>(), psnr.data_ptr<double>(),
                                    want_display ? display.data_ptr<float>() : nullptr, workspace.data_ptr(), current_stream());
    TORCH_CHECK(rc == 0, egr_eval_last_error());
    return {sse, psnr, display};
}

// Fused SSIM (egr_eval_ssim, csrc/ssim.hip) on the tensors of eval_metrics, with its checks. Returns (ssim_sum fp64 [V,3,3,2]: the sums of the SSIM map per pass and
// channel over all pixels and over the interior, ssim fp64 [V,3,2]: the two means per pass; a skipped pass reads NaN) on the device, two launches on the current
// stream, no host synchronisation.
static std::tuple<Tensor, Tensor> eval_ssim(const Tensor &final, const c10::optional<Tensor> &rgb, const c10::optional<Tensor> &target_final,
                                            const c10::optional<Tensor> &target_diffuse, const c10::optional<Tensor> &target_specular) {
    TORCH_CHECK(final.is_cuda() && final.scalar_type() == torch::kFloat32 && final.is_contiguous() && final.dim() == 4 && final.size(3) == 3, "eval_ssim: final must be a contiguous fp32 [V,H,W,3] GPU tensor");
    const int64_t V = final.size(0), H = final.size(1), W = final.size(2);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && H <= 0x7FFFFFFF && W <= 0x7FFFFFFF, "eval_ssim: at least one view and one pixel are required");
    const auto dev = final.device();
    const c10::DeviceGuard guard(dev); // the outputs, the workspace and current_stream() belong to final's device, which need not be the current one
    auto ptr = [&](const c10::optional<Tensor> &t, std::vector<int64_t> want, const char *what) -> const float * {
        if (!t.has_value() || !t->defined()) return nullptr;
        TORCH_CHECK(t->is_cuda() && t->device() == dev && t->scalar_type() == torch::kFloat32 && t->is_contiguous() && t->sizes() == torch::IntArrayRef(want), "eval_ssim: ", what,
                    " must be a contiguous fp32 tensor ", torch::IntArrayRef(want), " on final's device, got ", t->sizes());
        return t->data_ptr<float>();
    };
    const float *prgb = ptr(rgb, {V, EGR_NUM_STEPS, H, W, 3}, "rgb");
    const float *tf = ptr(target_final, {V, 3, H, W}, "target_final"), *td = ptr(target_diffuse, {V, 3, H, W}, "target_diffuse"), *ts = ptr(target_specular, {V, 3, H, W}, "target_specular");
    const auto f64 = torch::dtype(torch::kFloat64).device(dev);
    Tensor sum = torch::empty({V, 3, 3, 2}, f64), mean = torch::empty({V, 3, 2}, f64);
    Tensor workspace = torch::empty({(int64_t)(EGR_SSIM_WORKSPACE_BYTES(V, H, W) / 8)}, f64); // (freed stream-ordered by the caching allocator)
    const int rc = egr_eval_ssim(dev.index(), (uint32_t)V, (uint32_t)H, (uint32_t)W, final.data_ptr<float>(), prgb, tf, td, ts, sum.data_ptr<double>(), mean.data_ptr<double>(),
                                 workspace.data_ptr(), current_stream());
    TORCH_CHECK(rc == 0, egr_eval_last_error());
    return {sum, mean};
}

// The same kernel on display images the caller already has (egr_ssim_images): pred, gt contiguous fp32 [V,3,H,W] on one GPU, used as they are. Returns
// (ssim_sum fp64 [V,3,2], ssim fp64 [V,2]) on the device.
static std::tuple<Tensor, Tensor> ssim_images(const Tensor &pred, const Tensor &gt) {
    TORCH_CHECK(pred.is_cuda() && pred.scalar_type() == torch::kFloat32 && pred.is_contiguous() && pred.dim() == 4 && pred.size(1) == 3, "ssim_images: pred must be a contiguous fp32 [V,3,H,W] GPU tensor");
    TORCH_CHECK(gt.is_cuda() && gt.device() == pred.device() && gt.scalar_type() == torch::kFloat32 && gt.is_contiguous() && gt.sizes() == pred.sizes(),
                "ssim_images: gt must be a contiguous fp32 tensor ", pred.sizes(), " on pred's device, got ", gt.sizes());
    const int64_t V = pred.size(0), H = pred.size(2), W = pred.size(3);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && H <= 0x7FFFFFFF && W <= 0x7FFFFFFF, "ssim_images: at least one view and one pixel are required");
    const auto dev = pred.device();
    const c10::DeviceGuard guard(dev);
    const auto f64 = torch::dtype(torch::kFloat64).device(dev);
    Tensor sum = torch::empty({V, 3, 2}, f64), mean = torch::empty({V, 2}, f64);
    Tensor workspace = torch::empty({(int64_t)(EGR_SSIM_WORKSPACE_BYTES(V, H, W) / 8)}, f64);
    const int rc = egr_ssim_images(dev.index(), (uint32_t)V, (uint32_t)H, (uint32_t)W, pred.data_ptr<float>(), gt.data_ptr<float>(), sum.data_ptr<double>(), mean.data_ptr<double>(),
                                   workspace.data_ptr(), current_stream());
    TORCH_CHECK(rc == 0, egr_eval_last_error());
    return {sum, mean};
}

// Evaluation frames (egr_eval_frames, csrc/frames.hip): the predictions as render_views hands them out - final [V,H,W,3], rgb / normal / f0 [V,3,H,W,3], depth /
// roughness [V,3,H,W,1] - and the channel-major targets [V,3,H,W] ([V,1,H,W] for depth and roughness), every one optional, contiguous fp32 on one GPU. `kinds` is the
// bitmask of the header, `rounding` and `depth_mode` its constants. Returns (frames uint8 [V,7,2,H,W,3] or, side by side, [V,7,H,2W,3]; sse8 int64 [V,7,3]; psnr8 fp64
// [V,7,2]; depth_range fp32 [V,2]) on the device, allocated with empty: slots the call does not write are unspecified. At most three launches on the current stream, no
// host synchronisation.
static std::tuple<Tensor, Tensor, Tensor, Tensor> eval_frames(const c10::optional<Tensor> &final, const c10::optional<Tensor> &rgb, const c10::optional<Tensor> &depth,
                                                              const c10::optional<Tensor> &normal, const c10::optional<Tensor> &roughness, const c10::optional<Tensor> &f0,
                                                              const c10::optional<Tensor> &t_final, const c10::optional<Tensor> &t_diffuse, const c10::optional<Tensor> &t_specular,
                                                              const c10::optional<Tensor> &t_depth, const c10::optional<Tensor> &t_normal, const c10::optional<Tensor> &t_roughness,
                                                              const c10::optional<Tensor> &t_f0, int64_t kinds, int64_t rounding, int64_t depth_mode, bool side_by_side) {
    struct In { const c10::optional<Tensor> *t; const char *name; bool pixel_major; int64_t channels; };
    const In in[13] = {{&final, "final", true, 3}, {&rgb, "rgb", true, 3}, {&depth, "depth", true, 1}, {&normal, "normal", true, 3}, {&roughness, "roughness", true, 1}, {&f0, "f0", true, 3},
                       {&t_final, "t_final", false, 3}, {&t_diffuse, "t_diffuse", false, 3}, {&t_specular, "t_specular", false, 3}, {&t_depth, "t_depth", false, 1},
                       {&t_normal, "t_normal", false, 3}, {&t_roughness, "t_roughness", false, 1}, {&t_f0, "t_f0", false, 3}};
    const Tensor *first = nullptr;
    int64_t V = 0, H = 0, W = 0;
    for (int i = 0; i < 13 && !first; i++) {
        if (!in[i].t->has_value() || !(*in[i].t)->defined()) continue;
        first = &**in[i].t;
        const int64_t want_dim = i == 0 || !in[i].pixel_major ? 4 : 5;
        TORCH_CHECK(first->dim() == want_dim, "eval_frames: ", in[i].name, " must have ", want_dim, " dimensions, got ", first->sizes());
        V = first->size(0), H = first->size(want_dim - (in[i].pixel_major ? 3 : 2)), W = first->size(want_dim - (in[i].pixel_major ? 2 : 1));
    }
    TORCH_CHECK(first && first->is_cuda(), "eval_frames: at least one GPU tensor is required");
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && H <= 0x7FFFFFFF && W <= 0x7FFFFFFF, "eval_frames: at least one view and one pixel are required");
    TORCH_CHECK(kinds >= 0 && kinds <= 0xFFFFFFFFll && rounding >= 0 && rounding <= 0xFFFFFFFFll && depth_mode >= 0 && depth_mode <= 0xFFFFFFFFll, "eval_frames: kinds, rounding and depth_mode are the header's unsigned constants");
    const auto dev = first->device();
    const c10::DeviceGuard guard(dev); // the outputs, the workspace and current_stream() belong to the inputs' device, which need not be the current one
    const float *p[13];
    for (int i = 0; i < 13; i++) {
        p[i] = nullptr;
        if (!in[i].t->has_value() || !(*in[i].t)->defined()) continue;
        const Tensor &t = **in[i].t;
        const std::vector<int64_t> want = i == 0 ? std::vector<int64_t>{V, H, W, 3} : in[i].pixel_major ? std::vector<int64_t>{V, EGR_NUM_STEPS, H, W, in[i].channels} : std::vector<int64_t>{V, in[i].channels, H, W};
        TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.sizes() == torch::IntArrayRef(want), "eval_frames: ", in[i].name,
                    " must be a contiguous fp32 tensor ", torch::IntArrayRef(want), " on one GPU, got ", t.sizes());
        p[i] = t.data_ptr<float>();
    }
    const auto opt = [&](torch::ScalarType ty) { return torch::dtype(ty).device(dev); };
    Tensor frames = side_by_side ? torch::empty({V, EGR_FRAMES_KINDS, H, 2 * W, 3}, opt(torch::kUInt8)) : torch::empty({V, EGR_FRAMES_KINDS, 2, H, W, 3}, opt(torch::kUInt8));
    Tensor sse8 = torch::empty({V, EGR_FRAMES_KINDS, 3}, opt(torch::kInt64)), psnr8 = torch::empty({V, EGR_FRAMES_KINDS, 2}, opt(torch::kFloat64));
    Tensor range = torch::empty({V, 2}, opt(torch::kFloat32));
    Tensor workspace = torch::empty({(int64_t)((EGR_FRAMES_WORKSPACE_BYTES(V, H, W) + 7) / 8)}, opt(torch::kFloat64)); // (whole doubles that hold every byte; freed stream-ordered by the caching allocator)
    egr_frames_args a{};
    a.num_views = (uint32_t)V, a.height = (uint32_t)H, a.width = (uint32_t)W;
    a.kinds = (uint32_t)kinds, a.rounding = (uint32_t)rounding, a.depth_mode = (uint32_t)depth_mode, a.layout = side_by_side ? EGR_FRAMES_SIDE_BY_SIDE : EGR_FRAMES_SEPARATE;
    a.final = p[0], a.rgb = p[1], a.depth = p[2], a.normal = p[3], a.roughness = p[4], a.f0 = p[5];
    for (int k = 0; k < EGR_FRAMES_KINDS; k++) a.targets[k] = p[6 + k];
    a.frames = frames.data_ptr<uint8_t>(), a.sse8 = sse8.data_ptr<int64_t>(), a.psnr8 = psnr8.data_ptr<double>(), a.depth_range = range.data_ptr<float>();
    a.workspace = workspace.data_ptr();
    const int rc = egr_eval_frames(dev.index(), &a, current_stream());
    TORCH_CHECK(rc == 0, egr_eval_last_error());
    return {frames, sse8, psnr8, range};
}

// The dense-init cloud (egr_voxel_*, csrc/initcloud.hip). The table is three caller-owned GPU tensors: keys int64 [cap] (filled with -1), acc int64 [cap,4] and
// status int64 [8] (zeroed). voxel_accumulate adds V views in one launch: c2w fp64 [V,3,3], origin fp64 [V,3], view_size fp64 [V] (the caller's host fp64 camera
// set-up, uploaded), depth fp32 [V,H,W], colour fp32 or uint8 [V,H,W,3] (uint8 with the 256-entry fp32 table), positions_out fp64 [V,H,W,3] or None.
// Current stream, no host synchronisation.
static void voxel_table_check(const char *fn, const Tensor &keys, const Tensor &acc, const Tensor &status) {
    TORCH_CHECK(keys.is_cuda() && keys.scalar_type() == torch::kInt64 && keys.is_contiguous() && keys.dim() == 1, fn, ": keys must be a contiguous int64 [cap] GPU tensor");
    TORCH_CHECK(acc.is_cuda() && acc.device() == keys.device() && acc.scalar_type() == torch::kInt64 && acc.is_contiguous() && acc.dim() == 2 && acc.size(0) == keys.size(0) && acc.size(1) == 4,
                fn, ": acc must be a contiguous int64 [cap,4] tensor on the device of keys");
    TORCH_CHECK(status.is_cuda() && status.device() == keys.device() && status.scalar_type() == torch::kInt64 && status.is_contiguous() && status.numel() == EGR_VOXEL_STATUS_WORDS,
                fn, ": status must be a contiguous int64 [", EGR_VOXEL_STATUS_WORDS, "] tensor on the device of keys");
}
static void voxel_accumulate(const Tensor &keys, const Tensor &acc, const Tensor &status, const Tensor &c2w, const Tensor &origin, const Tensor &view_size, const Tensor &depth,
                             const Tensor &colour, const c10::optional<Tensor> &colour_table, double voxel_scale, double colour_max, const c10::optional<Tensor> &positions_out) {
    voxel_table_check("voxel_accumulate", keys, acc, status);
    const auto dev = keys.device();
    const c10::DeviceGuard guard(dev);
    TORCH_CHECK(depth.is_cuda() && depth.device() == dev && depth.scalar_type() == torch::kFloat32 && depth.is_contiguous() && depth.dim() == 3, "voxel_accumulate: depth must be a contiguous fp32 [V,H,W] tensor on the table's device");
    const int64_t V = depth.size(0), H = depth.size(1), W = depth.size(2);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && V <= 65535 && H <= (1 << 20) && W <= (1 << 20), "voxel_accumulate: at least one view and one pixel are required");
    auto f64 = [&](const Tensor &t, std::vector<int64_t> want, const char *what) -> const double * {
        TORCH_CHECK(t.is_cuda() && t.device() == dev && t.scalar_type() == torch::kFloat64 && t.is_contiguous() && t.sizes() == torch::IntArrayRef(want), "voxel_accumulate: ", what,
                    " must be a contiguous fp64 tensor ", torch::IntArrayRef(want), " on the table's device, got ", t.sizes());
        return t.data_ptr<double>();
    };
    const double *pc2w = f64(c2w, {V, 3, 3}, "c2w"), *porigin = f64(origin, {V, 3}, "origin"), *pview = f64(view_size, {V}, "view_size");
    const bool u8 = colour.scalar_type() == torch::kUInt8;
    TORCH_CHECK(colour.is_cuda() && colour.device() == dev && (u8 || colour.scalar_type() == torch::kFloat32) && colour.is_contiguous() && colour.sizes() == torch::IntArrayRef({V, H, W, 3}),
                "voxel_accumulate: colour must be a contiguous fp32 or uint8 [V,H,W,3] tensor on the table's device");
    const float *table = nullptr;
    if (u8) {
        TORCH_CHECK(colour_table.has_value() && colour_table->defined() && colour_table->is_cuda() && colour_table->device() == dev && colour_table->scalar_type() == torch::kFloat32 &&
                        colour_table->is_contiguous() && colour_table->numel() == 256,
                    "voxel_accumulate: uint8 colours need colour_table, a contiguous fp32 [256] tensor on the table's device");
        table = colour_table->data_ptr<float>();
    }
    double *pos = nullptr;
    if (positions_out.has_value() && positions_out->defined()) pos = const_cast<double *>(f64(*positions_out, {V, H, W, 3}, "positions_out"));
    const int rc = egr_voxel_accumulate(dev.index(), keys.data_ptr<int64_t>(), acc.data_ptr<int64_t>(), status.data_ptr<int64_t>(), (uint64_t)keys.size(0), (uint32_t)V, (uint32_t)H,
                                        (uint32_t)W, pc2w, porigin, pview, depth.data_ptr<float>(), u8 ? nullptr : colour.data_ptr<float>(), u8 ? colour.data_ptr<uint8_t>() : nullptr,
                                        table, voxel_scale, colour_max, pos, current_stream());
    TORCH_CHECK(rc == 0, egr_voxel_last_error());
}
// Growth: every occupied slot of (src_keys, src_acc) is inserted into the initialised table (keys, acc); the slots it claims are added to status[0].
static void voxel_rehash(const Tensor &keys, const Tensor &acc, const Tensor &status, const Tensor &src_keys, const Tensor &src_acc) {
    voxel_table_check("voxel_rehash", keys, acc, status);
    voxel_table_check("voxel_rehash", src_keys, src_acc, status);
    TORCH_CHECK(src_keys.device() == keys.device(), "voxel_rehash: both tables must be on one device");
    const c10::DeviceGuard guard(keys.device());
    const int rc = egr_voxel_rehash(keys.device().index(), keys.data_ptr<int64_t>(), acc.data_ptr<int64_t>(), status.data_ptr<int64_t>(), (uint64_t)keys.size(0), src_keys.data_ptr<int64_t>(),
                                    src_acc.data_ptr<int64_t>(), (uint64_t)src_keys.size(0), current_stream());
    TORCH_CHECK(rc == 0, egr_voxel_last_error());
}
// The voxels with count >= min_count in the order of torch.unique(dim=0): (coords int32 [n,3], points fp32 [n,3], colors fp32 [n,3], counts int32 [n], the largest
// count of the table). max_rows bounds n (the table's occupied slots always do). ONE host synchronisation: the read-back of n.
static std::tuple<Tensor, Tensor, Tensor, Tensor, int64_t> voxel_extract(const Tensor &keys, const Tensor &acc, const Tensor &status, int64_t min_count, double voxel_scale, int64_t max_rows) {
    voxel_table_check("voxel_extract", keys, acc, status);
    TORCH_CHECK(min_count >= 0 && min_count <= 0xFFFFFFFFll, "voxel_extract: min_count must be in 0..2^32-1");
    TORCH_CHECK(max_rows >= 1 && max_rows <= keys.size(0), "voxel_extract: max_rows must be in 1..cap");
    const auto dev = keys.device();
    const c10::DeviceGuard guard(dev);
    const auto i32 = torch::dtype(torch::kInt32).device(dev), f32 = torch::dtype(torch::kFloat32).device(dev);
    Tensor coords = torch::empty({max_rows, 3}, i32), points = torch::empty({max_rows, 3}, f32), colors = torch::empty({max_rows, 3}, f32), counts = torch::empty({max_rows}, i32);
    const size_t bytes = egr_voxel_extract_workspace_bytes(dev.index(), (uint64_t)max_rows);
    TORCH_CHECK(bytes != 0, egr_voxel_last_error());
    Tensor workspace = torch::empty({(int64_t)((bytes + 15) / 16) * 2}, torch::dtype(torch::kInt64).device(dev)); // (the caching allocator aligns to 512 bytes)
    uint64_t host[2] = {0, 0};
    const int rc = egr_voxel_extract(dev.index(), keys.data_ptr<int64_t>(), acc.data_ptr<int64_t>(), status.data_ptr<int64_t>(), (uint64_t)keys.size(0), (uint32_t)min_count, voxel_scale,
                                     (uint64_t)max_rows, coords.data_ptr<int32_t>(), points.data_ptr<float>(), colors.data_ptr<float>(), counts.data_ptr<int32_t>(), host,
                                     workspace.data_ptr(), (size_t)workspace.numel() * 8, current_stream());
    TORCH_CHECK(rc == 0, egr_voxel_last_error());
    const int64_t n = (int64_t)host[0];
    return {coords.narrow(0, 0, n), points.narrow(0, 0, n), colors.narrow(0, 0, n), counts.narrow(0, 0, n), (int64_t)host[1]};
}

// The training views in fp16, part 1 (egr_viewset_ingest, csrc/viewset.hip): the views of one chunk into slots first_slot .. first_slot + V of the store, in one
// launch on the current stream. sources[kind]: a contiguous uint8 or fp32 [V,Hs,Ws,Cs] GPU tensor or None (absent); tables[kind]: the contiguous half [256] GPU
// table of a uint8 source, None for fp32; planes[kind]: the store's contiguous half [slots,C,H,W]; depth_range: contiguous fp32 [slots,2]. One entry per kind each.
static void viewset_ingest(const c10::List<c10::optional<Tensor>> &sources, const c10::List<c10::optional<Tensor>> &tables, std::vector<Tensor> planes, const Tensor &depth_range,
                           int64_t first_slot) {
    TORCH_CHECK(sources.size() == EGR_VIEWSET_KINDS && tables.size() == EGR_VIEWSET_KINDS && planes.size() == EGR_VIEWSET_KINDS,
                "viewset_ingest: sources, tables and planes must have one entry per kind (", EGR_VIEWSET_KINDS, ")");
    TORCH_CHECK(depth_range.is_cuda() && depth_range.scalar_type() == torch::kFloat32 && depth_range.is_contiguous() && depth_range.dim() == 2 && depth_range.size(1) == 2,
                "viewset_ingest: depth_range must be a contiguous fp32 [slots,2] GPU tensor");
    const c10::Device dev = depth_range.device();
    const c10::DeviceGuard guard(dev);
    const int64_t slots = depth_range.size(0);
    TORCH_CHECK(first_slot >= 0 && first_slot <= slots, "viewset_ingest: first_slot must be in 0..slots, got ", first_slot);
    egr_viewset_source table[EGR_VIEWSET_KINDS] = {};
    int64_t V = -1, Hs = 0, Ws = 0, H = -1, W = -1;
    for (size_t k = 0; k < EGR_VIEWSET_KINDS; k++) {
        const Tensor &p = planes[k];
        const int64_t C = (k == EGR_VIEWSET_DEPTH || k == 5) ? 1 : 3;
        TORCH_CHECK(p.is_cuda() && p.device() == dev && p.scalar_type() == torch::kFloat16 && p.is_contiguous() && p.dim() == 4 && p.size(0) == slots && p.size(1) == C,
                    "viewset_ingest: planes[", k, "] must be a contiguous half [", slots, ",", C, ",H,W] tensor on the store's device, got ", p.sizes());
        if (H < 0) H = p.size(2), W = p.size(3);
        TORCH_CHECK(p.size(2) == H && p.size(3) == W, "viewset_ingest: the planes of every kind must share one image size");
        const c10::optional<Tensor> s = sources.get(k), t = tables.get(k);
        const bool has_table = t.has_value() && t->defined();
        if (has_table) {
            TORCH_CHECK(t->is_cuda() && t->device() == dev && t->scalar_type() == torch::kFloat16 && t->is_contiguous() && t->numel() == 256,
                        "viewset_ingest: tables[", k, "] must be a contiguous half [256] tensor on the store's device");
            table[k].table = t->data_ptr();
        }
        if (!(s.has_value() && s->defined())) {
            table[k].table = nullptr; // (the table of an absent kind is ignored)
            continue;
        }
        TORCH_CHECK(s->is_cuda() && s->device() == dev && s->is_contiguous() && s->dim() == 4 && (s->scalar_type() == torch::kUInt8 || s->scalar_type() == torch::kFloat32),
                    "viewset_ingest: sources[", k, "] must be a contiguous uint8 or fp32 [V,Hs,Ws,Cs] tensor on the store's device");
        if (V < 0) V = s->size(0), Hs = s->size(1), Ws = s->size(2);
        TORCH_CHECK(s->size(0) == V && s->size(1) == Hs && s->size(2) == Ws, "viewset_ingest: the sources of one call must share [V,Hs,Ws] (sources[", k, "] is ", s->sizes(), ")");
        table[k].data = s->data_ptr(), table[k].planes = p.data_ptr(), table[k].channels = (uint32_t)s->size(3);
        table[k].dtype = s->scalar_type() == torch::kUInt8 ? EGR_VIEWSET_U8 : EGR_VIEWSET_F32;
    }
    TORCH_CHECK(V >= 1, "viewset_ingest: at least one kind with at least one view is required");
    TORCH_CHECK(Hs > 0 && Ws > 0 && H > 0 && W > 0 && std::max(std::max(V, Hs), std::max(std::max(Ws, H), W)) <= 65535, "viewset_ingest: V and the image sizes must be in 1..65535");
    const int rc = egr_viewset_ingest(dev.index(), table, (uint32_t)V, (uint32_t)Hs, (uint32_t)Ws, (uint32_t)H, (uint32_t)W, (uint32_t)first_slot, (uint32_t)slots,
                                      depth_range.data_ptr<float>(), current_stream());
    TORCH_CHECK(rc == 0, egr_viewset_last_error());
}
// The training views in fp16, part 2 (egr_viewset_gather): rows v < len(indices) of the fp32 outputs = the stored views indices[v], exactly float(half), and their
// camera rows, in one launch per 64 indices on the current stream - `indices` are host integers: no upload, no synchronisation. planes[kind]: the store's half
// [slots,C,H,W]; R [slots,3,3], centers [slots,3], fovy [slots]: its camera table; out[kind]: a contiguous fp32 [>= V,C,H,W] tensor or None (not wanted);
// out_R / out_centers / out_fovy: contiguous fp32 with >= V rows. Only the first V rows of an output are written.
static void viewset_gather(std::vector<Tensor> planes, const Tensor &R, const Tensor &centers, const Tensor &fovy, int64_t num_filled, std::vector<int64_t> indices,
                           const c10::List<c10::optional<Tensor>> &out, const Tensor &out_R, const Tensor &out_centers, const Tensor &out_fovy) {
    TORCH_CHECK(planes.size() == EGR_VIEWSET_KINDS && out.size() == EGR_VIEWSET_KINDS, "viewset_gather: planes and out must have one entry per kind (", EGR_VIEWSET_KINDS, ")");
    const int64_t V = (int64_t)indices.size();
    TORCH_CHECK(V >= 1, "viewset_gather: at least one index is required");
    TORCH_CHECK(fovy.is_cuda() && fovy.dim() == 1, "viewset_gather: fovy must be an fp32 [slots] GPU tensor");
    const c10::Device dev = fovy.device();
    const c10::DeviceGuard guard(dev);
    const int64_t slots = fovy.size(0);
    TORCH_CHECK(num_filled >= 0 && num_filled <= slots, "viewset_gather: num_filled must be in 0..slots");
    auto f32 = [&](const Tensor &t, std::vector<int64_t> tail, int64_t rows, bool exact, const char *what) {
        bool ok = t.is_cuda() && t.device() == dev && t.scalar_type() == torch::kFloat32 && t.is_contiguous() && t.dim() == (int64_t)tail.size() + 1 &&
                  (exact ? t.size(0) == rows : t.size(0) >= rows);
        for (size_t d = 0; ok && d < tail.size(); d++) ok = t.size((int64_t)d + 1) == tail[d];
        TORCH_CHECK(ok, "viewset_gather: ", what, " must be a contiguous fp32 tensor with ", exact ? "" : "at least ", rows, " rows of ", c10::IntArrayRef(tail), " on the store's device, got ",
                    t.sizes());
        return t.data_ptr<float>();
    };
    egr_viewset_store store = {};
    egr_viewset_batch batch = {};
    store.R = f32(R, {3, 3}, slots, true, "R"), store.centers = f32(centers, {3}, slots, true, "centers"), store.fovy = f32(fovy, {}, slots, true, "fovy");
    batch.R = f32(out_R, {3, 3}, V, false, "out_R"), batch.centers = f32(out_centers, {3}, V, false, "out_centers"), batch.fovy = f32(out_fovy, {}, V, false, "out_fovy");
    int64_t H = -1, W = -1;
    for (size_t k = 0; k < EGR_VIEWSET_KINDS; k++) {
        const Tensor &p = planes[k];
        const int64_t C = (k == EGR_VIEWSET_DEPTH || k == 5) ? 1 : 3;
        TORCH_CHECK(p.is_cuda() && p.device() == dev && p.scalar_type() == torch::kFloat16 && p.is_contiguous() && p.dim() == 4 && p.size(0) == slots && p.size(1) == C,
                    "viewset_gather: planes[", k, "] must be a contiguous half [", slots, ",", C, ",H,W] tensor on the store's device, got ", p.sizes());
        if (H < 0) H = p.size(2), W = p.size(3);
        TORCH_CHECK(p.size(2) == H && p.size(3) == W, "viewset_gather: the planes of every kind must share one image size");
        store.planes[k] = p.data_ptr();
        const c10::optional<Tensor> o = out.get(k);
        if (o.has_value() && o->defined()) batch.targets[k] = f32(*o, {C, H, W}, V, false, "out[kind]");
    }
    TORCH_CHECK(H > 0 && W > 0 && H <= 65535 && W <= 65535 && slots <= 0xFFFFFFFFll, "viewset_gather: image sizes must be in 1..65535");
    store.num_slots = (uint32_t)slots, store.num_filled = (uint32_t)num_filled, store.height = (uint32_t)H, store.width = (uint32_t)W;
    std::vector<uint32_t> idx((size_t)V);
    for (int64_t v = 0; v < V; v++) {
        TORCH_CHECK(indices[(size_t)v] >= 0 && indices[(size_t)v] < num_filled, "viewset_gather: index ", indices[(size_t)v], " is out of range: ", num_filled, " slots are filled");
        idx[(size_t)v] = (uint32_t)indices[(size_t)v];
    }
    const int rc = egr_viewset_gather(dev.index(), &store, idx.data(), (uint32_t)V, &batch, current_stream());
    TORCH_CHECK(rc == 0, egr_viewset_last_error());
}

// unit-test hook (egr_debug_lean_arith): (a / b, sqrt(a)) as the hot kernels' division and square root compute them
static std::tuple<torch::Tensor, torch::Tensor> debug_lean_arith(const torch::Tensor &a, const torch::Tensor &b) {
    TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.numel() == b.numel(), "debug_lean_arith: two GPU tensors of one size expected");
    auto x = a.to(torch::kFloat32).contiguous(), y = b.to(torch::kFloat32).contiguous();
    auto q = torch::zeros_like(x), r = torch::zeros_like(x);
    TORCH_CHECK(egr_debug_lean_arith(x.get_device(), x.data_ptr<float>(), y.data_ptr<float>(), q.data_ptr<float>(), r.data_ptr<float>(), (uint32_t)x.numel(), current_stream()) == 0, "debug_lean_arith failed");
    return {q, r};
}

TORCH_LIBRARY(simple_knn, m) { m.def("distCUDA2(Tensor points) -> Tensor", &dist_hip2); }
TORCH_LIBRARY(egr, m) {
    m.def("fused_adam_step(Tensor[] params, Tensor[] grads, Tensor[] rt_params, Tensor[] rt_grads, Tensor[] exp_avg, Tensor[] exp_avg_sq, float[] lrs, "
          "float[] clamp_min, float[] clamp_max, float[] log_decay, int step, float beta1, float beta2, float eps, int[] group_steps=[]) -> ()",
          &fused_adam_step);
    m.def("debug_lean_arith(Tensor a, Tensor b) -> (Tensor, Tensor)", &debug_lean_arith);
    m.def("prune_select(Tensor? total_weight, float divisor, float min_weight, Tensor? points, Tensor? cam_centers, Tensor? cam_znear, Tensor? remove_mask) -> "
          "(Tensor src_index, Tensor count)",
          &prune_select);
    m.def("prune_gather(Tensor[] src, Tensor src_index, int count) -> Tensor[]", &prune_gather);
    m.def("grow_sample(int first, int n, int seed, float radius, float clamp, Device device) -> Tensor", &grow_sample);
    m.def("grow_append(Tensor[] src, Tensor?[] tail, int[] fill_bits, int m) -> Tensor[]", &grow_append);
    m.def("edit_select(Tensor xyz, Tensor? f0, Tensor? roughness, Tensor? diffuse, Tensor objects) -> Tensor", &edit_select);
    m.def("edit_apply(Tensor[] src, Tensor[] dst, Tensor mask, Tensor records) -> ()", &edit_apply);
    m.def("eval_metrics(Tensor final, Tensor? rgb, Tensor? target_final, Tensor? target_diffuse, Tensor? target_specular, bool want_display=False) -> "
          "(Tensor sse, Tensor psnr, Tensor display)",
          &eval_metrics);
    m.def("eval_ssim(Tensor final, Tensor? rgb, Tensor? target_final, Tensor? target_diffuse, Tensor? target_specular) -> (Tensor ssim_sum, Tensor ssim)", &eval_ssim);
    m.def("ssim_images(Tensor pred, Tensor gt) -> (Tensor ssim_sum, Tensor ssim)", &ssim_images);
    m.def("eval_frames(Tensor? final, Tensor? rgb, Tensor? depth, Tensor? normal, Tensor? roughness, Tensor? f0, Tensor? t_final, Tensor? t_diffuse, Tensor? t_specular, "
          "Tensor? t_depth, Tensor? t_normal, Tensor? t_roughness, Tensor? t_f0, int kinds, int rounding, int depth_mode, bool side_by_side) -> "
          "(Tensor frames, Tensor sse8, Tensor psnr8, Tensor depth_range)",
          &eval_frames);
    m.def("voxel_accumulate(Tensor keys, Tensor acc, Tensor status, Tensor c2w, Tensor origin, Tensor view_size, Tensor depth, Tensor colour, Tensor? colour_table, "
          "float voxel_scale, float colour_max, Tensor? positions_out=None) -> ()",
          &voxel_accumulate);
    m.def("voxel_rehash(Tensor keys, Tensor acc, Tensor status, Tensor src_keys, Tensor src_acc) -> ()", &voxel_rehash);
    m.def("voxel_extract(Tensor keys, Tensor acc, Tensor status, int min_count, float voxel_scale, int max_rows) -> "
          "(Tensor coords, Tensor points, Tensor colors, Tensor counts, int largest_count)",
          &voxel_extract);
    m.def("viewset_ingest(Tensor?[] sources, Tensor?[] tables, Tensor[] planes, Tensor depth_range, int first_slot) -> ()", &viewset_ingest);
    m.def("viewset_gather(Tensor[] planes, Tensor R, Tensor centers, Tensor fovy, int num_filled, int[] indices, Tensor?[] out, Tensor out_R, Tensor out_centers, "
          "Tensor out_fovy) -> ()",
          &viewset_gather);
}

TORCH_LIBRARY(raytracer, m) {
    CameraDataHolder::bind(m);
    ConfigDataHolder::bind(m);
    FramebufferDataHolder::bind(m);
    GaussianDataHolder::bind(m);
    MetaDataHolder::bind(m);
    PPLLDataHolder::bind(m);
    StatsDataHolder::bind(m);
    Raytracer::bind(m);
}
