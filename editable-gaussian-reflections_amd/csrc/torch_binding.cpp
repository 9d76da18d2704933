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

// ---- The argument checks of both halves of this file: the Raytracer's methods and the context-free ops
bool given(const c10::optional<Tensor> &t) { return t.has_value() && t->defined(); }
// (a Tensor[] cannot hold None: there an undefined or empty tensor is an absent entry)
c10::optional<Tensor> unless_empty(const Tensor &t) { return t.defined() && t.numel() ? c10::optional<Tensor>(t) : c10::nullopt; }

// What a tensor argument must measure: a full shape (-1: any size in that dimension), at least so many rows of a trailing shape, or a number of elements in any shape.
struct Shape {
    std::vector<int64_t> dims;
    int64_t min_rows = 0, numel = -1;
    Shape(std::initializer_list<int64_t> d) : dims(d) {}
    Shape(std::vector<int64_t> d) : dims(std::move(d)) {}
    static Shape at_least(int64_t rows, std::vector<int64_t> trailing) {
        trailing.insert(trailing.begin(), -1);
        Shape s(std::move(trailing));
        s.min_rows = rows;
        return s;
    }
    static Shape elements(int64_t n) {
        Shape s(std::vector<int64_t>{});
        s.numel = n;
        return s;
    }
    bool fits(const Tensor &t) const {
        if (numel >= 0) return t.numel() == numel;
        if (t.dim() != (int64_t)dims.size() || (min_rows > 0 && t.size(0) < min_rows)) return false;
        for (size_t d = 0; d < dims.size(); d++)
            if (dims[d] >= 0 && t.size((int64_t)d) != dims[d]) return false;
        return true;
    }
    std::string text() const {
        if (numel >= 0) return "of " + std::to_string(numel) + " elements";
        std::string s = "[";
        for (size_t d = 0; d < dims.size(); d++)
            s += (d ? ", " : "") + (dims[d] >= 0 ? std::to_string(dims[d]) : d == 0 && min_rows > 0 ? ">= " + std::to_string(min_rows) : std::string("*"));
        return s + "]";
    }
};

// THE argument check: a tensor of T's dtype, contiguous, on `dev`, of the wanted shape -> its data pointer. An absent one (None, or undefined) -> NULL if it is
// optional, an error if it is required. Errors carry the op's and the argument's name.
template <class T> T *tensor_arg(const char *op, const std::string &name, const c10::optional<Tensor> &t, c10::Device dev, const Shape &want, bool required = true) {
    if (!given(t)) {
        TORCH_CHECK(!required, op, ": ", name, " is required");
        return nullptr;
    }
    constexpr c10::ScalarType dtype = c10::CppTypeToScalarType<T>::value;
    TORCH_CHECK(t->is_cuda() && t->device() == dev && t->scalar_type() == dtype && t->is_contiguous() && want.fits(*t), op, ": ", name, " must be a contiguous ", dtype, " tensor ",
                want.text(), " on ", dev, ", got ", t->scalar_type(), " ", t->sizes(), t->is_contiguous() ? "" : " (not contiguous)", " on ", t->device());
    return t->data_ptr<T>();
}
// An entry of the tensor lists of prune_gather and grow_append: n rows of 4-byte elements of any dtype, moved as bits.
void *words_arg(const char *op, const char *list, size_t k, const Tensor &t, c10::Device dev, int64_t n) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == dev && t.is_contiguous() && t.element_size() == 4 && t.dim() >= 1 && t.size(0) == n, op, ": ", list, "[", k,
                "] must be a contiguous tensor of 4-byte elements with ", n, " rows on ", dev, " (contiguous GPU tensors of 4-byte elements with the same leading size are required)");
    return t.data_ptr();
}
// The device of an op: that of the tensor that leads its arguments.
c10::Device gpu_of(const char *op, const char *name, const Tensor &t) {
    TORCH_CHECK(t.defined() && t.is_cuda(), op, ": ", name, " must be a GPU tensor (there is no CPU path)");
    return t.device();
}
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

    // THE table of the eight parameters, in the export order of gaussian_raytracer.py:41-50 (the order of update_bvh_from's and import_into's tensors): name, width,
    // where the gradient's window starts in the flat buffer (floats per Gaussian; the buffer is tensor-major in the holder's order, total_weight last at 21), the
    // holder's parameter and gradient tensors and the same two in egr_gaussians.
    struct Param { const char *name; int64_t width, grad_offset; Tensor GaussianDataHolder::*value, GaussianDataHolder::*grad; const float *egr_gaussians::*raw_value; float *egr_gaussians::*raw_grad; };
    static const Param PARAMS[8];
    static std::string param_names() {
        std::string s;
        for (const Param &p : PARAMS) s += (s.empty() ? "" : ", ") + std::string(p.name);
        return s;
    }

    void point_grads() {
        auto win = [&](Tensor &t, int64_t offset, int64_t c) { t.set_(grad_flat.storage(), offset * count, {count, c}, {c, 1}); }; // same TensorImpl, new window
        for (const Param &p : PARAMS) win(this->*p.grad, p.grad_offset, p.width);
        win(total_weight, 21, 1);
    }
    GaussianDataHolder() {
        torch::NoGradGuard no_grad;
        point_grads();
        for (const Param &p : PARAMS) (this->*p.value).mutable_grad() = this->*p.grad;
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
        std::vector<Tensor *> win{&total_weight};
        for (const Param &p : PARAMS) win.push_back(&(this->*p.grad));
        std::vector<Tensor> old_rows;
        for (Tensor *w : win) old_rows.push_back(w->narrow(0, 0, keep).clone());
        count = n;
        for (const Param &p : PARAMS) (this->*p.value).resize_({n, p.width});
        grad_flat = torch::zeros({22 * n}, F32());
        point_grads();
        for (size_t k = 0; k < win.size() && keep > 0; k++) win[k]->narrow(0, 0, keep).copy_(old_rows[k]);
        if (use_delta) grad_delta = torch::zeros({22 * n}, F32());
    }
    egr_gaussians reify() {
        egr_gaussians g;
        g.count = (uint32_t)count;
        float *base = use_delta ? ptr<float>(grad_delta) : ptr<float>(grad_flat); // same tensor-major layout as point_grads()
        for (const Param &p : PARAMS) g.*p.raw_value = ptr<float>(this->*p.value), g.*p.raw_grad = base + p.grad_offset * count;
        g.total_weight = base + 21 * count;
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

const GaussianDataHolder::Param GaussianDataHolder::PARAMS[8] = {
    {"scale", 3, 11, &GaussianDataHolder::scale, &GaussianDataHolder::dL_dscale, &egr_gaussians::scale, &egr_gaussians::dL_dscale},
    {"rotation", 4, 17, &GaussianDataHolder::rotation, &GaussianDataHolder::dL_drotation, &egr_gaussians::rotation, &egr_gaussians::dL_drotation},
    {"mean", 3, 14, &GaussianDataHolder::mean, &GaussianDataHolder::dL_dmean, &egr_gaussians::mean, &egr_gaussians::dL_dmean},
    {"opacity", 1, 10, &GaussianDataHolder::opacity, &GaussianDataHolder::dL_dopacity, &egr_gaussians::opacity, &egr_gaussians::dL_dopacity},
    {"rgb", 3, 0, &GaussianDataHolder::rgb, &GaussianDataHolder::dL_drgb, &egr_gaussians::rgb, &egr_gaussians::dL_drgb},
    {"normal", 3, 3, &GaussianDataHolder::normal, &GaussianDataHolder::dL_dnormal, &egr_gaussians::normal, &egr_gaussians::dL_dnormal},
    {"roughness", 1, 9, &GaussianDataHolder::roughness, &GaussianDataHolder::dL_droughness, &egr_gaussians::roughness, &egr_gaussians::dL_droughness},
    {"f0", 3, 6, &GaussianDataHolder::f0, &GaussianDataHolder::dL_df0, &egr_gaussians::f0, &egr_gaussians::dL_df0},
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
    // The device of the holders' tensors and of the context: the one current at construction. A method may be called with any device current: each one that reads
    // current_stream(), allocates a tensor or hands the library a stream takes a c10::DeviceGuard for `device` first.
    const c10::Device device;
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
          ppll_backward_data(c10::make_intrusive<PPLLDataHolder>(width_, height_, backward_ppl_size)), device(camera_data->origin.device()) {
        if (num_gaussians > 0) gaussian_data->resize(num_gaussians);
        int rc = egr_create(&ctx, (int)device.index(), (int)width, (int)height, forward_ppl_size, backward_ppl_size);
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

    // The caller's eight tensors of a fused export (update_bvh_from: parameter values) or import (import_into: gradients), in the order of GaussianDataHolder::PARAMS: each a
    // contiguous fp32 tensor on the tracer's device with the shape of the holder's. Checked before anything is launched; returns them as the library takes them.
    egr_gaussians like_holder(const char *who, const std::vector<Tensor> &t, bool gradients) {
        TORCH_CHECK(t.size() == 8, who, ": eight tensors expected (", GaussianDataHolder::param_names(), "), got ", t.size());
        egr_gaussians g{};
        g.count = (uint32_t)gaussian_data->count;
        for (int k = 0; k < 8; k++) {
            const auto &p = GaussianDataHolder::PARAMS[k];
            float *data = tensor_arg<float>(who, std::string("'") + p.name + "'", t[k], device, Shape(((*gaussian_data).*p.value).sizes().vec()));
            if (gradients) g.*p.raw_grad = data;
            else g.*p.raw_value = data;
        }
        return g;
    }
    // import_into (addition; grad mode only): the caller's eight gradient tensors, in the order of update_bvh_from's parameters. The launch's gather adds what it
    // leaves in the holder's gradients to them - `t.grad += holder.grad` for the eight, bit for bit, without the extra pass (egr_raytrace_import).
    // targets (addition; grad mode only): the view's six target images in set_targets_chw's order (diffuse, specular, depth, normal, roughness, f0), each None
    // (absent = zeros) or a contiguous fp32 [C,H,W] tensor on the tracer's device. The launch reads them where they are - no upload, framebuffer.target_* is
    // neither read nor written (egr_raytrace_targets). The caller keeps them alive and unmodified until the launch has completed on the current stream.
    void raytrace(c10::optional<std::vector<Tensor>> import_into, c10::optional<std::vector<c10::optional<Tensor>>> targets) { // raytracer.cpp:81-94
        const c10::DeviceGuard guard(device);
        const bool grads = torch::autograd::GradMode::is_enabled();
        if (grads && !targets.has_value()) upload_behind_targets(); // this launch reads framebuffer.target_*
        if (!import_into.has_value() && !targets.has_value()) {
            check(egr_raytrace(ctx, grads ? 1 : 0, current_stream()), "raytrace");
            return;
        }
        TORCH_CHECK(grads || !import_into.has_value(), "raytrace: import_into needs grad mode (a no-grad launch has no gradients to import)");
        TORCH_CHECK(grads || !targets.has_value(), "raytrace: targets need grad mode (a no-grad launch reads no target)");
        egr_gaussians dst{};
        if (import_into.has_value()) dst = like_holder("raytrace", *import_into, true);
        const float *planes[6];
        if (targets.has_value()) six_targets("raytrace", *targets, {}, false, nullptr, planes);
        check(egr_raytrace_targets(ctx, 1, import_into.has_value() ? &dst : nullptr, targets.has_value() ? planes : nullptr, current_stream()), "raytrace");
        if (targets.has_value()) {
            for (int k = 0; k < 6; k++) behind_targets[k] = (*targets)[k].has_value() ? *(*targets)[k] : Tensor();
            framebuffer_targets_behind = true;
        }
    }
    void denoise() { const c10::DeviceGuard guard(device); check(egr_denoise(ctx, current_stream()), "denoise"); }
    void reset_accumulators() { framebuffer_data->reset_accumulators(); }
    // fuse_live (addition; default = the reference's update_bvh()): the pass also writes the live per-gaussian records and the NEXT raytrace()
    // skips its own pass over the cloud - for callers that run update_bvh() and raytrace() back to back (egr_update_bvh_ex)
    void update_bvh(bool fuse_live) { const c10::DeviceGuard guard(device); check(egr_update_bvh_ex(ctx, fuse_live ? EGR_UPDATE_FUSE_LIVE : 0u, current_stream()), "update_bvh"); }
    // export + update_bvh(fuse_live) in one pass over the cloud (egr_update_bvh_from): the eight tensors hold the caller's current parameter values; the
    // holder's tensors then hold them too, as after the eight copy_ calls of gaussian_raytracer.py:41-50
    void update_bvh_from(Tensor scale, Tensor rotation, Tensor mean, Tensor opacity, Tensor rgb, Tensor normal, Tensor roughness, Tensor f0, bool fuse_live) {
        const c10::DeviceGuard guard(device);
        const egr_gaussians src = like_holder("update_bvh_from", {scale, rotation, mean, opacity, rgb, normal, roughness, f0}, false);
        TORCH_CHECK((reinterpret_cast<uintptr_t>(rotation.data_ptr()) & 15u) == 0, "update_bvh_from: 'rotation' must be 16-byte aligned");
        check(egr_update_bvh_from(ctx, &src, fuse_live ? EGR_UPDATE_FUSE_LIVE : 0u, current_stream()), "update_bvh_from");
    }
    void rebuild_bvh() { const c10::DeviceGuard guard(device); check(egr_rebuild_bvh(ctx, current_stream()), "rebuild_bvh"); }
    void resize(int64_t n) { // raytracer.cpp:112-120
        const c10::DeviceGuard guard(device);
        gaussian_data->resize(n);
        egr_gaussians g = gaussian_data->reify();
        check(egr_set_gaussians(ctx, &g), "resize");
    }
    // ---- additions (not in the reference) ----
    void set_partition(int64_t rank, int64_t world) { check(egr_set_partition(ctx, (int)rank, (int)world), "set_partition"); }
    void use_grad_delta(bool on) { // see GaussianDataHolder::grad_delta
        const c10::DeviceGuard guard(device);
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
        // (the reference's copy_ calls - gaussian_raytracer.py:98-100 - take tensors of any device. A tensor of another GPU is moved to this tracer's device; a CPU
        // tensor - a dataset's numpy pose - is converted on the host and its values go to the launch BY VALUE: the upload of a pageable tensor would wait for
        // the stream, once per training iteration)
        TORCH_CHECK(R.dim() == 2 && R.size(0) == 3 && R.size(1) == 3 && centre.numel() == 3, "set_camera: tensors [3,3] and [3] expected");
        const c10::DeviceGuard guard(device);
        const auto here = [&](const Tensor &t) { return t.is_cpu() ? t.to(torch::kFloat32).contiguous() : t.to(device, torch::kFloat32).contiguous(); };
        Tensor r = here(R), cc = here(centre);
        const unsigned flags = (r.is_cpu() ? EGR_CAMERA_ROTATION_ON_HOST : 0u) | (cc.is_cpu() ? EGR_CAMERA_CENTER_ON_HOST : 0u);
        check(egr_set_camera_from_dataset_ex(ctx, r.data_ptr<float>(), cc.data_ptr<float>(), (float)fov, (float)znear, (float)zfar, flags, current_stream()), "set_camera");
    }
    static constexpr struct { const char *name; int64_t channels; } TARGETS[6] = {{"diffuse", 3}, {"specular", 3}, {"depth", 1}, {"normal", 3}, {"roughness", 1}, {"f0", 3}}; // (the order of the C ABI's six target pointers)
    // THE walk over the six optional targets of a launch (`in`, in TARGETS' order): out[k] = the data of a contiguous fp32 [lead..., C, H, W] tensor on the tracer's device, or
    // NULL for an absent one (None or undefined; with `empty_is_absent` an empty tensor too). With `converted` (set_targets_chw) only the shape is the caller's business: the
    // tensor is moved to the tracer's device as fp32 and kept alive there.
    void six_targets(const char *op, const std::vector<c10::optional<Tensor>> &in, const std::vector<int64_t> &lead, bool empty_is_absent, Tensor *converted, const float *out[6]) {
        TORCH_CHECK(in.size() == 6, op, ": six targets expected (diffuse, specular, depth, normal, roughness, f0; None = absent), got ", in.size());
        for (int k = 0; k < 6; k++) {
            out[k] = nullptr;
            if (!given(in[k]) || (empty_is_absent && in[k]->numel() == 0)) continue;
            std::vector<int64_t> dims = lead;
            dims.insert(dims.end(), {TARGETS[k].channels, height, width});
            const Shape want(std::move(dims));
            const std::string name = std::string("target '") + TARGETS[k].name + "' (channel-major)";
            if (converted) { // (the reference's `buf.copy_(val.moveaxis(0, -1))` raises on any other shape and accepts any device: same here - a [H,W,C] tensor must not be read as [C,H,W])
                TORCH_CHECK(want.fits(*in[k]), op, ": ", name, " must be a tensor ", want.text(), ", got ", in[k]->sizes());
                converted[k] = in[k]->to(device, torch::kFloat32).contiguous();
            }
            out[k] = tensor_arg<float>(op, name, converted ? converted[k] : *in[k], device, want);
        }
    }
    // the six target images of a training view, channel-major ([C,H,W] tensors of any device and float dtype; an undefined / empty tensor = absent = zeros), written into
    // the framebuffer's pixel-major target buffers for this context's own tiles in one launch (egr_set_targets_chw)
    void set_targets_chw(c10::optional<Tensor> diffuse, c10::optional<Tensor> specular, c10::optional<Tensor> depth, c10::optional<Tensor> normal, c10::optional<Tensor> roughness,
                         c10::optional<Tensor> f0) {
        const c10::DeviceGuard guard(device);
        Tensor keep[6];
        const float *p[6];
        six_targets("set_targets_chw", {diffuse, specular, depth, normal, roughness, f0}, {}, true, keep, p);
        check(egr_set_targets_chw(ctx, p[0], p[1], p[2], p[3], p[4], p[5], current_stream()), "set_targets_chw");
        forget_behind_targets(); // the framebuffer's targets are what the caller says again
    }
    // batched no-grad render (egr_render_views): R [V,3,3] (dataset c2w rotations), centers [V,3], fovy [V] (any device, moved like set_camera's),
    // `outputs` = names among VIEW_OUTPUTS. render_views allocates them (zeros) in the framebuffer's HWC layout with a leading V - final [V,H,W,3], the
    // others [V,3,H,W,c] - and returns them in the order asked; render_views_into writes the caller's tensors instead.
    struct ViewOutput { const char *name; int64_t channels; float *egr_view_batch::*slot; };
    static constexpr ViewOutput VIEW_OUTPUTS[6] = {{"final", 3, &egr_view_batch::final},   {"rgb", 3, &egr_view_batch::rgb}, {"depth", 1, &egr_view_batch::depth},
                                                   {"normal", 3, &egr_view_batch::normal}, {"f0", 3, &egr_view_batch::f0},   {"roughness", 1, &egr_view_batch::roughness}};
    // (the table's entry of a name, and the shape of its buffer for V views: only the final image has no bounce steps)
    std::pair<const ViewOutput *, std::vector<int64_t>> view_output(const std::string &name, int64_t V) const {
        for (const ViewOutput &o : VIEW_OUTPUTS)
            if (name == o.name) return {&o, o.slot == &egr_view_batch::final ? std::vector<int64_t>{V, height, width, o.channels} : std::vector<int64_t>{V, EGR_NUM_STEPS, height, width, o.channels}};
        TORCH_CHECK(false, "render_views: unknown output '", name, "' (final, rgb, depth, normal, f0, roughness)");
    }
    // The three camera tensors of a batch, validated (`who` = the caller's name in the messages): (R, centers, fovy) as contiguous fp32 tensors on the tracer's device, and V.
    std::tuple<Tensor, Tensor, Tensor, int64_t> batch_cameras(const char *who, const Tensor &R, const Tensor &centers, const Tensor &fovy) {
        TORCH_CHECK(R.dim() == 3 && R.size(1) == 3 && R.size(2) == 3, who, ": R must be [V,3,3], got ", R.sizes());
        const int64_t V = R.size(0);
        TORCH_CHECK(Shape({V, 3}).fits(centers), who, ": centers must be [V,3] = ", Shape({V, 3}).text(), ", got ", centers.sizes());
        TORCH_CHECK(Shape({V}).fits(fovy), who, ": fovy must be [V] = ", Shape({V}).text(), ", got ", fovy.sizes());
        return {R.to(device, torch::kFloat32).contiguous(), centers.to(device, torch::kFloat32).contiguous(), fovy.to(device, torch::kFloat32).contiguous(), V};
    }
    std::vector<Tensor> render_views(Tensor R, Tensor centers, Tensor fovy, double znear, double zfar, int64_t samples_per_view, std::vector<std::string> outputs) {
        const c10::DeviceGuard guard(device);
        const int64_t V = R.dim() == 3 ? R.size(0) : 0;
        std::vector<Tensor> bufs;
        for (const auto &name : outputs) bufs.push_back(torch::zeros(view_output(name, V).second, framebuffer_data->output_rgb.options()));
        render_views_into(R, centers, fovy, znear, zfar, samples_per_view, outputs, bufs);
        return bufs;
    }
    void render_views_into(Tensor R, Tensor centers, Tensor fovy, double znear, double zfar, int64_t samples_per_view, std::vector<std::string> outputs,
                           std::vector<Tensor> buffers) {
        const c10::DeviceGuard guard(device);
        const auto [r, cc, fv, V] = batch_cameras("render_views", R, centers, fovy);
        TORCH_CHECK(samples_per_view >= 0 && samples_per_view <= 0x7FFFFFFF, "render_views: samples_per_view out of range");
        TORCH_CHECK(outputs.size() == buffers.size(), "render_views_into: one buffer per output name expected");
        egr_view_batch b{};
        b.num_views = (uint32_t)V, b.samples_per_view = (uint32_t)samples_per_view;
        b.rotation_c2w_dataset = r.data_ptr<float>(), b.camera_center = cc.data_ptr<float>(), b.vertical_fov_radians = fv.data_ptr<float>();
        b.znear = (float)znear, b.zfar = (float)zfar;
        for (size_t i = 0; i < outputs.size(); i++) {
            const auto [o, shape] = view_output(outputs[i], V);
            float *data = tensor_arg<float>("render_views", "output '" + outputs[i] + "'", buffers[i], device, Shape(shape));
            TORCH_CHECK(b.*o->slot == nullptr, "render_views: output '", outputs[i], "' requested twice");
            b.*o->slot = data;
        }
        check(egr_render_views(ctx, &b, current_stream()), "render_views");
    }
    // per-object coverage of one view (egr_object_masks): R [3,3], center [3] (any device, moved and converted like render_views'), row_bits int32 [N] on the
    // tracer's device (editing.EditableGaussians.selection_mask), bits = the requested selection bits in output order. Returns (masks [K,H,W] fp32,
    // hit int32 [H,W] - bit j = masks[j] != 0, output index 31 is the sign bit -, top int32 [H,W]). A query: nothing else of the tracer changes.
    std::tuple<Tensor, Tensor, Tensor> object_masks(Tensor R, Tensor center, double fovy, double znear, double zfar, Tensor row_bits, std::vector<int64_t> bits) {
        const c10::DeviceGuard guard(device);
        TORCH_CHECK(R.dim() == 2 && R.size(0) == 3 && R.size(1) == 3 && center.numel() == 3, "object_masks: R [3,3] and center [3] expected");
        egr_object_mask_query q{};
        q.row_bits = reinterpret_cast<const uint32_t *>(tensor_arg<int32_t>("object_masks", "row_bits", row_bits, device, {gaussian_data->mean.size(0)}));
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
        q.rotation_c2w_dataset = r.data_ptr<float>(), q.camera_center = cc.data_ptr<float>(), q.vertical_fov_radians = fv.data_ptr<float>();
        q.znear = (float)znear, q.zfar = (float)zfar;
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
        const c10::DeviceGuard guard(device);
        const auto [r, cc, fv, V] = batch_cameras("train_views", R, centers, fovy);
        egr_train_batch b{};
        b.num_views = (uint32_t)V;
        b.rotation_c2w_dataset = r.data_ptr<float>(), b.camera_center = cc.data_ptr<float>(), b.vertical_fov_radians = fv.data_ptr<float>();
        b.znear = (float)znear, b.zfar = (float)zfar;
        const float *p[6];
        six_targets("train_views", {diffuse, specular, depth, normal, roughness, f0}, {V}, true, nullptr, p);
        b.target_diffuse = p[0], b.target_specular = p[1], b.target_depth = p[2], b.target_normal = p[3], b.target_roughness = p[4], b.target_f0 = p[5];
        if (import_into.has_value()) {
            const egr_gaussians dst = like_holder("train_views", *import_into, true);
            check(egr_train_views_import(ctx, &b, &dst, current_stream()), "train_views");
        } else {
            check(egr_train_views(ctx, &b, current_stream()), "train_views");
        }
    }
    // batched denoise (egr_denoise_views): final [V,H,W,3] and its guide normal - render_views' [V,3,H,W,3] buffer (step 0 is the guide) or a packed [V,H,W,3] -
    // as contiguous fp32 tensors on the tracer's device. Returns a new [V,H,W,3] tensor; each view is bit-equal to denoise() on a framebuffer that holds the same
    // final / normal. The framebuffer is not touched.
    Tensor denoise_views(Tensor final, Tensor normal) {
        const c10::DeviceGuard guard(device);
        const float *image = tensor_arg<float>("denoise_views", "final", final, device, {-1, height, width, 3});
        const int64_t V = final.size(0);
        const bool steps = normal.dim() == 5; // ([V,3,H,W,3], or the packed [V,H,W,3])
        const float *guide = tensor_arg<float>("denoise_views", "normal", normal, device, steps ? Shape{V, EGR_NUM_STEPS, height, width, 3} : Shape{V, height, width, 3});
        Tensor out = torch::empty_like(final);
        if (V == 0) return out;
        check(egr_denoise_views(ctx, (uint32_t)V, image, guide, (size_t)((steps ? EGR_NUM_STEPS : 1) * height * width * 3), out.data_ptr<float>(), current_stream()), "denoise_views");
        return out;
    }
    void set_batch_frames(int64_t n) { TORCH_CHECK(n >= 1 && n <= 0x7FFFFFFF && egr_set_batch_frames(ctx, (int)n) == 0, "set_batch_frames: a frame count >= 1 expected"); }
    void set_rays_per_task(int64_t n) { TORCH_CHECK(egr_set_rays_per_task(ctx, (int)n) == 0, "set_rays_per_task: 0 (automatic), 16, 32 or 64 expected"); }
    void set_team_help(bool on) { TORCH_CHECK(egr_set_team_help(ctx, on ? 1 : 0) == 0, "set_team_help failed"); }
    void set_team_help_auto() { TORCH_CHECK(egr_set_team_help(ctx, -1) == 0, "set_team_help_auto failed"); } // on for under-filled ranks of a partition only (egr_set_team_help(-1))
    void set_strands(int64_t n) { TORCH_CHECK(egr_set_strands(ctx, (int)n) == 0, "set_strands: only 1 is accepted (strands were removed; every launch runs on the caller's stream)"); }
    std::vector<int64_t> get_counters() { // synchronises
        const c10::DeviceGuard guard(device);
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
    void reset_lifetime_counters() { const c10::DeviceGuard guard(device); check(egr_reset_lifetime_counters(ctx, current_stream()), "reset_lifetime_counters"); }
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
        const c10::DeviceGuard guard(device);
        Tensor t = torch::zeros({EGR_NUM_STEPS, height, width}, torch::kInt32);
        check(egr_debug_get_step_hits(ctx, t.data_ptr<int32_t>(), current_stream()), "debug_step_hits");
        return t;
    }
    Tensor debug_hit_sequence_hash() { // [3,H,W] int64 (the bits of the uint64 hashes) on the host: ordered composited gaussian ids per pixel and step of the last grad launch
        const c10::DeviceGuard guard(device);
        Tensor t = torch::zeros({EGR_NUM_STEPS, height, width}, torch::kInt64);
        check(egr_debug_get_hit_sequence_hash(ctx, reinterpret_cast<uint64_t *>(t.data_ptr<int64_t>()), current_stream()), "debug_hit_sequence_hash");
        return t;
    }
    int64_t check_bvh() { const c10::DeviceGuard guard(device); return egr_debug_check_bvh(ctx, current_stream()); }
    std::string last_error() { return egr_last_error(ctx); }
    std::vector<Tensor> debug_instances() {
        const c10::DeviceGuard guard(device);
        int64_t n = gaussian_data->count;
        Tensor M = torch::zeros({n, 3, 4}, torch::kFloat32), W = torch::zeros({n, 3, 4}, torch::kFloat32), A = torch::zeros({n, 6}, torch::kFloat32);
        check(egr_debug_get_instances(ctx, M.data_ptr<float>(), W.data_ptr<float>(), A.data_ptr<float>(), current_stream()), "debug_instances");
        return {M, W, A};
    }
    Tensor debug_backward_records() { // [n,4,4] float32 on the host, by gaussian id (egr_debug_get_backward_records)
        const c10::DeviceGuard guard(device);
        float frame[6];
        uint32_t info[4] = {0u, 0u, 0u, 0u}; // (info[3]: the count the tree was built for - the rows the library copies, whatever the holder was resized to since)
        check(egr_debug_get_bvh_state(ctx, frame, info, current_stream()), "debug_backward_records");
        Tensor t = torch::zeros({(int64_t)info[3], 4, 4}, torch::kFloat32);
        check(egr_debug_get_backward_records(ctx, t.data_ptr<float>(), current_stream()), "debug_backward_records");
        return t;
    }
    std::tuple<Tensor, Tensor> debug_bvh_state() { // (float32[6]: the build frame's origin xyz and cells per world unit xyz; int64[4]: out_of_frame flag, wide nodes, depth, n built) on the host
        const c10::DeviceGuard guard(device);
        Tensor f = torch::zeros({6}, torch::kFloat32), i = torch::zeros({4}, torch::kInt64);
        uint32_t info[4] = {0u, 0u, 0u, 0u};
        check(egr_debug_get_bvh_state(ctx, f.data_ptr<float>(), info, current_stream()), "debug_bvh_state");
        for (int k = 0; k < 4; k++) i.data_ptr<int64_t>()[k] = (int64_t)info[k];
        return {f, i};
    }
    // The built tree on the host (egr_debug_get_tree), in this order: keys int64 [n] (the bits of the uint64 keys), gid_of_pos int32 [n], pos_of_gid int32 [n],
    // left int32 [n-1], right int32 [n-1], dp float32 [n-1,16], wnodes int32 [nw,8,4] (the bits of the uint32 words), bsph float32 [n,4], level_start int32 [depth+1]
    std::vector<Tensor> debug_tree() {
        const c10::DeviceGuard guard(device);
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

// ---- The context-free ops (torch.ops.egr.*, torch.ops.simple_knn.distCUDA2): tensors in, one library call each. Every op checks its tensor arguments through
// tensor_arg (words_arg for the lists of 4-byte rows) and takes a c10::DeviceGuard for the tensors' device BEFORE it allocates an output or reads
// current_stream(): the tensors need not live on the current device, and the library is handed the stream of the device it is told to run on.

// simple_knn._C.distCUDA2 (gaussian_model.py:17): float CUDA(HIP) tensor [N,3] -> [N] mean squared distance to the 3 nearest
// neighbours. Registered as torch.ops.simple_knn.distCUDA2; the package's simple_knn.py re-exports it under the reference's name.
static Tensor dist_hip2(const Tensor &points) {
    TORCH_CHECK(points.is_cuda(), "distCUDA2: points must live on the GPU (there is no CPU path)");
    TORCH_CHECK(points.dim() == 2 && points.size(1) == 3, "distCUDA2: expected an [N,3] tensor");
    const c10::DeviceGuard guard(points.device());
    auto p = points.to(torch::kFloat32).contiguous();
    auto out = torch::zeros({p.size(0)}, p.options());
    const int rc = egr_knn_mean_dist2(p.get_device(), p.data_ptr<float>(), (uint32_t)p.size(0), out.data_ptr<float>(), current_stream());
    TORCH_CHECK(rc == 0, egr_knn_last_error());
    return out;
}
// One launch for import + scale decay + Adam + clamps + zero_grad + export (csrc/step.hip). Tensor lists are parallel, one
// entry per parameter group; an undefined / empty tensor means "absent" for grads, rt_params, rt_grads and the Adam moments.
static void fused_adam_step(std::vector<Tensor> params, std::vector<Tensor> grads, std::vector<Tensor> rt_params, std::vector<Tensor> rt_grads, std::vector<Tensor> exp_avg,
                            std::vector<Tensor> exp_avg_sq, std::vector<double> lrs, std::vector<double> clamp_min, std::vector<double> clamp_max, std::vector<double> log_decay,
                            int64_t step, double beta1, double beta2, double eps, std::vector<int64_t> group_steps) {
    const char *op = "fused_adam_step";
    const size_t G = params.size();
    TORCH_CHECK(G >= 1 && G <= EGR_MAX_PARAM_GROUPS, "fused_adam_step: 1..8 parameter groups");
    TORCH_CHECK(grads.size() == G && rt_params.size() == G && rt_grads.size() == G && exp_avg.size() == G && exp_avg_sq.size() == G && lrs.size() == G &&
                    clamp_min.size() == G && clamp_max.size() == G && log_decay.size() == G,
                "fused_adam_step: all lists need one entry per group");
    TORCH_CHECK(group_steps.empty() || group_steps.size() == G, "fused_adam_step: group_steps must be empty (every group uses `step`) or hold one count per group");
    const c10::Device dev = gpu_of(op, "params[0]", params[0]);
    const c10::DeviceGuard guard(dev);
    TORCH_CHECK(params[0].dim() >= 1, "fused_adam_step: parameters must be contiguous float GPU tensors with the same leading size");
    const int64_t n = params[0].size(0);
    egr_param_group g[EGR_MAX_PARAM_GROUPS];
    for (size_t k = 0; k < G; k++) {
        const std::string at = "[" + std::to_string(k) + "]";
        const Shape size = Shape::elements(params[k].defined() ? params[k].numel() : 0); // (of the parameter: every other tensor of the group has it)
        g[k].param = tensor_arg<float>(op, "params" + at, params[k], dev, size);
        TORCH_CHECK(params[k].dim() >= 1 && params[k].size(0) == n, "fused_adam_step: parameters must be contiguous float GPU tensors with the same leading size");
        g[k].grad = tensor_arg<float>(op, "grads" + at, unless_empty(grads[k]), dev, size, false);
        g[k].rt_param = tensor_arg<float>(op, "rt_params" + at, unless_empty(rt_params[k]), dev, size, false);
        g[k].rt_grad = tensor_arg<float>(op, "rt_grads" + at, unless_empty(rt_grads[k]), dev, size, false);
        g[k].exp_avg = tensor_arg<float>(op, "exp_avg" + at, unless_empty(exp_avg[k]), dev, size, false);
        g[k].exp_avg_sq = tensor_arg<float>(op, "exp_avg_sq" + at, unless_empty(exp_avg_sq[k]), dev, size, false);
        g[k].width = n ? (uint32_t)(params[k].numel() / n) : 1u;
        g[k].lr = (float)lrs[k], g[k].clamp_min = (float)clamp_min[k], g[k].clamp_max = (float)clamp_max[k], g[k].log_decay = (float)log_decay[k];
        g[k].step = group_steps.size() == G ? (uint32_t)group_steps[k] : 0u;
    }
    const int rc = egr_fused_adam_step(dev.index(), g, (int)G, (uint32_t)n, (uint32_t)step, beta1, beta2, eps, current_stream());
    TORCH_CHECK(rc == 0, egr_fused_step_last_error());
}

// Fused prune, part 1 (egr_prune_select, csrc/prune.hip): which rows survive. Every criterion is optional (None = skipped) but at least one of
// total_weight [N] / [N,1], points [N,3], remove_mask [N] (uint8 or bool) must be given - it fixes N. Returns (src_index int32 [N]: the first `count`
// entries are the kept rows, ascending; count int32 [1]) on the device, asynchronously: reading `count` is the caller's one synchronisation.
static std::tuple<Tensor, Tensor> prune_select(const c10::optional<Tensor> &total_weight, double divisor, double min_weight, const c10::optional<Tensor> &points,
                                               const c10::optional<Tensor> &cam_centers, const c10::optional<Tensor> &cam_znear, const c10::optional<Tensor> &remove_mask) {
    const char *op = "prune_select";
    const Tensor *first = given(total_weight) ? &*total_weight : given(points) ? &*points : given(remove_mask) ? &*remove_mask : nullptr;
    TORCH_CHECK(first, "prune_select: one of total_weight, points, remove_mask is required (it fixes the number of rows)");
    const c10::Device dev = gpu_of(op, "the first criterion", *first);
    const c10::DeviceGuard guard(dev);
    TORCH_CHECK(first->dim() >= 1, "prune_select: the criteria are tensors with one row per gaussian");
    const int64_t n = first->size(0);
    TORCH_CHECK(n <= (int64_t)0xFFFFFFFFll, "prune_select: too many rows");
    const float *tw = tensor_arg<float>(op, "total_weight ([N] or [N,1])", total_weight, dev, Shape::elements(n), false);
    const float *pts = tensor_arg<float>(op, "points", points, dev, {n, 3}, false);
    const bool as_bool = given(remove_mask) && remove_mask->scalar_type() == torch::kBool; // (a bool is a byte that is 0 or 1)
    const uint8_t *mask = tensor_arg<uint8_t>(op, "remove_mask (uint8 or bool)", as_bool ? c10::optional<Tensor>(remove_mask->view(torch::kUInt8)) : remove_mask, dev, Shape::elements(n), false);
    TORCH_CHECK(given(cam_centers) == given(cam_znear), "prune_select: cam_centers and cam_znear go together");
    TORCH_CHECK(!given(cam_centers) || given(points), "prune_select: the camera criterion needs points");
    const int64_t num_cams = given(cam_znear) ? cam_znear->numel() : 0;
    const float *cc = tensor_arg<float>(op, "cam_centers", cam_centers, dev, {num_cams, 3}, false), *cz = tensor_arg<float>(op, "cam_znear", cam_znear, dev, {num_cams}, false);
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
    const char *op = "prune_gather";
    const c10::Device dev = gpu_of(op, "src_index", src_index);
    const c10::DeviceGuard guard(dev);
    const int64_t n = src_index.numel(); // (the tensors need the rows the index list was selected from)
    const uint32_t *index = reinterpret_cast<const uint32_t *>(tensor_arg<int32_t>(op, "src_index (the list of prune_select)", src_index, dev, {n}));
    TORCH_CHECK(count >= 0 && count <= n, "prune_gather: count must be in 0..", n);
    std::vector<Tensor> out;
    std::vector<egr_prune_array> table;
    for (size_t k = 0; k < src.size(); k++) {
        const Tensor &t = src[k];
        const void *rows = words_arg(op, "src", k, t, dev, n);
        auto shape = t.sizes().vec();
        shape[0] = count;
        out.push_back(torch::empty(shape, t.options()));
        const int64_t width = n ? t.numel() / n : 1;
        if (width == 0) continue; // (a [N,0] tensor has no elements to move)
        table.push_back(egr_prune_array{rows, out.back().data_ptr(), (uint32_t)width});
    }
    if (n == 0 || count == 0) return out; // (empty tensors have no storage to hand to the library)
    for (size_t k0 = 0; k0 < table.size(); k0 += EGR_MAX_PRUNE_ARRAYS) {
        const int rc = egr_prune_gather(dev.index(), table.data() + k0, (int)std::min<size_t>(EGR_MAX_PRUNE_ARRAYS, table.size() - k0), (uint32_t)n, index, (uint32_t)count, current_stream());
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
    const c10::DeviceGuard guard(dev);
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
    const char *op = "grow_append";
    TORCH_CHECK(tail.size() == src.size() && fill_bits.size() == src.size(), "grow_append: src, tail and fill_bits must have one entry per tensor (", src.size(), ", ",
                tail.size(), ", ", fill_bits.size(), ")");
    std::vector<Tensor> out;
    if (src.empty()) return out;
    const int64_t n = src[0].dim() >= 1 ? src[0].size(0) : -1;
    TORCH_CHECK(n >= 0, "grow_append: tensors with a leading (row) dimension are required");
    TORCH_CHECK(m >= 0 && n + m <= ((int64_t)1 << 26), "grow_append: m must be >= 0 and n + m <= 2^26 rows (the limit of the tree), got n = ", n, ", m = ", m);
    const c10::Device dev = gpu_of(op, "src[0]", src[0]);
    const c10::DeviceGuard guard(dev);
    std::vector<egr_grow_array> table;
    for (size_t k = 0; k < src.size(); k++) {
        const Tensor &t = src[k];
        const void *rows = words_arg(op, "src", k, t, dev, n);
        TORCH_CHECK(fill_bits[k] >= -((int64_t)1 << 31) && fill_bits[k] < ((int64_t)1 << 32), "grow_append: fill_bits[", k, "] is not a 32-bit word");
        auto shape = t.sizes().vec();
        int64_t width = 1;
        for (size_t d = 1; d < shape.size(); d++) width *= shape[d];
        shape[0] = n + m;
        egr_grow_array e{n ? rows : nullptr, nullptr, nullptr, (uint32_t)width, EGR_GROW_TAIL_FILL, (uint32_t)(uint64_t)fill_bits[k]};
        const c10::optional<Tensor> add = tail.get(k);
        if (given(add)) {
            const void *new_rows = words_arg(op, "tail", k, *add, dev, m);
            TORCH_CHECK(add->scalar_type() == t.scalar_type() && add->sizes().slice(1) == t.sizes().slice(1), "grow_append: tail[", k, "] must have the dtype and the trailing shape of src[", k,
                        "] (", t.scalar_type(), " ", t.sizes().slice(1), "), got ", add->scalar_type(), " ", add->sizes().slice(1));
            e.tail = m ? new_rows : nullptr, e.tail_kind = EGR_GROW_TAIL_ROWS;
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
    const char *op = "edit_select";
    const c10::Device dev = gpu_of(op, "xyz", xyz);
    const c10::DeviceGuard guard(dev);
    const float *pxyz = tensor_arg<float>(op, "xyz", xyz, dev, {-1, 3});
    const int64_t n = xyz.size(0);
    TORCH_CHECK(n <= (int64_t)1 << 26, "edit_select: n exceeds 2^26 rows (the limit of the tree)");
    TORCH_CHECK(!objects.is_cuda() && objects.scalar_type() == torch::kInt32 && objects.is_contiguous() && objects.dim() == 2 &&
                    objects.size(1) == (int64_t)(sizeof(egr_edit_object) / 4),
                "edit_select: objects must be a contiguous CPU int32 [K,", sizeof(egr_edit_object) / 4, "] tensor (egr_edit_object records)");
    TORCH_CHECK(objects.size(0) <= EGR_MAX_EDIT_OBJECTS, "edit_select: at most ", EGR_MAX_EDIT_OBJECTS, " objects");
    const float *pf0 = tensor_arg<float>(op, "f0 ([N,3])", f0, dev, Shape::elements(n * 3), false), *pr = tensor_arg<float>(op, "roughness ([N,1])", roughness, dev, Shape::elements(n), false);
    const float *pd = tensor_arg<float>(op, "diffuse ([N,3])", diffuse, dev, Shape::elements(n * 3), false);
    Tensor mask = torch::empty({n}, torch::dtype(torch::kInt32).device(dev));
    if (n == 0) return mask; // (no rows: nothing to launch)
    const int rc = egr_edit_select(dev.index(), (uint32_t)n, pxyz, pf0, pr, pd, reinterpret_cast<const egr_edit_object *>(objects.data_ptr<int32_t>()), (uint32_t)objects.size(0),
                                   reinterpret_cast<uint32_t *>(mask.data_ptr<int32_t>()), current_stream());
    TORCH_CHECK(rc == 0, egr_edit_last_error());
    return mask;
}
// Scene editing, part 2 (egr_edit_apply): edit and export in one launch. `src` / `dst`: eight contiguous fp32 GPU tensors each, in the export order
// scale [N,3], rotation [N,4], mean [N,3], opacity [N,1], rgb [N,3], normal [N,3], roughness [N,1], f0 [N,3]; dst[k] may be src[k] itself. `mask`: the int32 [N]
// tensor of edit_select; `records`: a GPU int32 tensor [K, 43] holding K egr_edit_record records as bits. Current stream, no host synchronisation.
static void edit_apply(std::vector<Tensor> src, std::vector<Tensor> dst, const Tensor &mask, const Tensor &records) {
    const char *op = "edit_apply";
    static const int64_t width[8] = {3, 4, 3, 1, 3, 3, 1, 3};
    TORCH_CHECK(src.size() == 8 && dst.size() == 8, "edit_apply: src and dst are eight tensors each (scale, rotation, mean, opacity, rgb, normal, roughness, f0)");
    const c10::Device dev = gpu_of(op, "src[0]", src[0]);
    const c10::DeviceGuard guard(dev);
    TORCH_CHECK(src[0].dim() >= 1, "edit_apply: tensors with rows are required");
    const int64_t n = src[0].size(0);
    TORCH_CHECK(n <= (int64_t)1 << 26, "edit_apply: n exceeds 2^26 rows (the limit of the tree)");
    egr_edit_arrays s{}, d{};
    float **sp = &s.scale, **dp = &d.scale;
    for (int k = 0; k < 8; k++) {
        const std::string at = "[" + std::to_string(k) + "] ([N," + std::to_string(width[k]) + "])";
        sp[k] = tensor_arg<float>(op, "src" + at, src[k], dev, Shape::elements(n * width[k])), dp[k] = tensor_arg<float>(op, "dst" + at, dst[k], dev, Shape::elements(n * width[k]));
        TORCH_CHECK(src[k].dim() >= 1 && src[k].size(0) == n && dst[k].dim() >= 1 && dst[k].size(0) == n, "edit_apply: tensor ", k, " must be a contiguous fp32 [N,", width[k], "] GPU tensor");
    }
    const int32_t *rec = tensor_arg<int32_t>(op, "records (K <= 32 egr_edit_record records)", records, dev, {-1, (int64_t)(sizeof(egr_edit_record) / 4)});
    const int64_t K = records.size(0);
    TORCH_CHECK(K <= EGR_MAX_EDIT_OBJECTS, "edit_apply: at most ", EGR_MAX_EDIT_OBJECTS, " records");
    const int32_t *bits = tensor_arg<int32_t>(op, "mask (the tensor of edit_select)", mask, dev, {n});
    if (n == 0) return; // (empty tensors have no storage to hand to the library)
    const int rc = egr_edit_apply(dev.index(), (uint32_t)n, &s, &d, reinterpret_cast<const uint32_t *>(bits), K ? reinterpret_cast<const egr_edit_record *>(rec) : nullptr, (uint32_t)K, current_stream());
    TORCH_CHECK(rc == 0, egr_edit_last_error());
}

// What eval_metrics and eval_ssim take: final [V,H,W,3], rgb [V,3,H,W,3] (None when both of its targets are) and the channel-major targets [V,3,H,W] (None: the pass
// is skipped and reports NaN) as contiguous fp32 tensors on one GPU. The checks of both ops, the sizes they derive and the pointers they pass on.
struct EvalInputs {
    c10::Device dev;
    int64_t V, H, W;
    const float *final, *rgb, *target_final, *target_diffuse, *target_specular;
};
static EvalInputs eval_inputs(const char *op, const Tensor &final, const c10::optional<Tensor> &rgb, const c10::optional<Tensor> &target_final,
                              const c10::optional<Tensor> &target_diffuse, const c10::optional<Tensor> &target_specular) {
    EvalInputs a{gpu_of(op, "final", final), 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};
    a.final = tensor_arg<float>(op, "final ([V,H,W,3])", final, a.dev, {-1, -1, -1, 3});
    a.V = final.size(0), a.H = final.size(1), a.W = final.size(2);
    TORCH_CHECK(a.V >= 1 && a.H >= 1 && a.W >= 1 && a.H <= 0x7FFFFFFF && a.W <= 0x7FFFFFFF, op, ": at least one view and one pixel are required");
    a.rgb = tensor_arg<float>(op, "rgb", rgb, a.dev, {a.V, EGR_NUM_STEPS, a.H, a.W, 3}, false);
    a.target_final = tensor_arg<float>(op, "target_final", target_final, a.dev, {a.V, 3, a.H, a.W}, false);
    a.target_diffuse = tensor_arg<float>(op, "target_diffuse", target_diffuse, a.dev, {a.V, 3, a.H, a.W}, false);
    a.target_specular = tensor_arg<float>(op, "target_specular", target_specular, a.dev, {a.V, 3, a.H, a.W}, false);
    return a;
}

// Fused evaluation metrics (egr_eval_metrics, csrc/eval.hip) on the tensors of eval_inputs. Returns (sse fp64 [V,3,3], psnr fp64 [V,3,2], display fp32 [V,3,2,3,H,W] -
// or an empty tensor without want_display; a skipped pass reads NaN there) on the device, two launches on the current stream, no host synchronisation.
static std::tuple<Tensor, Tensor, Tensor> eval_metrics(const Tensor &final, const c10::optional<Tensor> &rgb, const c10::optional<Tensor> &target_final,
                                                       const c10::optional<Tensor> &target_diffuse, const c10::optional<Tensor> &target_specular, bool want_display) {
    const EvalInputs a = eval_inputs("eval_metrics", final, rgb, target_final, target_diffuse, target_specular);
    const c10::DeviceGuard guard(a.dev);
    const int64_t V = a.V, H = a.H, W = a.W;
    const auto f64 = torch::dtype(torch::kFloat64).device(a.dev);
    Tensor sse = torch::empty({V, 3, 3}, f64), psnr = torch::empty({V, 3, 2}, f64);
    Tensor display = torch::empty({0}, final.options());
    if (want_display)
        display = (a.target_final && a.target_diffuse && a.target_specular) ? torch::empty({V, 3, 2, 3, H, W}, final.options()) : torch::full({V, 3, 2, 3, H, W}, NAN, final.options());
    Tensor workspace = torch::empty({(int64_t)(EGR_EVAL_WORKSPACE_BYTES(V, H, W) / 8)}, f64); // (freed stream-ordered by the caching allocator)
    const int rc = egr_eval_metrics(a.dev.index(), (uint32_t)V, (uint32_t)H, (uint32_t)W, a.final, a.rgb, a.target_final, a.target_diffuse, a.target_specular, sse.data_ptr<double>(),
                                    psnr.data_ptr<double>(), want_display ? display.data_ptr<float>() : nullptr, workspace.data_ptr(), current_stream());
    TORCH_CHECK(rc == 0, egr_eval_last_error());
    return {sse, psnr, display};
}

// Fused SSIM (egr_eval_ssim, csrc/ssim.hip) on the tensors of eval_inputs. Returns (ssim_sum fp64 [V,3,3,2]: the sums of the SSIM map per pass and channel over all
// pixels and over the interior, ssim fp64 [V,3,2]: the two means per pass; a skipped pass reads NaN) on the device, two launches on the current stream, no host
// synchronisation.
static std::tuple<Tensor, Tensor> eval_ssim(const Tensor &final, const c10::optional<Tensor> &rgb, const c10::optional<Tensor> &target_final,
                                            const c10::optional<Tensor> &target_diffuse, const c10::optional<Tensor> &target_specular) {
    const EvalInputs a = eval_inputs("eval_ssim", final, rgb, target_final, target_diffuse, target_specular);
    const c10::DeviceGuard guard(a.dev);
    const auto f64 = torch::dtype(torch::kFloat64).device(a.dev);
    Tensor sum = torch::empty({a.V, 3, 3, 2}, f64), mean = torch::empty({a.V, 3, 2}, f64);
    Tensor workspace = torch::empty({(int64_t)(EGR_SSIM_WORKSPACE_BYTES(a.V, a.H, a.W) / 8)}, f64); // (freed stream-ordered by the caching allocator)
    const int rc = egr_eval_ssim(a.dev.index(), (uint32_t)a.V, (uint32_t)a.H, (uint32_t)a.W, a.final, a.rgb, a.target_final, a.target_diffuse, a.target_specular, sum.data_ptr<double>(),
                                 mean.data_ptr<double>(), workspace.data_ptr(), current_stream());
    TORCH_CHECK(rc == 0, egr_eval_last_error());
    return {sum, mean};
}

// The same kernel on display images the caller already has (egr_ssim_images): pred, gt contiguous fp32 [V,3,H,W] on one GPU, used as they are. Returns
// (ssim_sum fp64 [V,3,2], ssim fp64 [V,2]) on the device.
static std::tuple<Tensor, Tensor> ssim_images(const Tensor &pred, const Tensor &gt) {
    const char *op = "ssim_images";
    const c10::Device dev = gpu_of(op, "pred", pred);
    const c10::DeviceGuard guard(dev);
    const float *p = tensor_arg<float>(op, "pred ([V,3,H,W])", pred, dev, {-1, 3, -1, -1});
    const int64_t V = pred.size(0), H = pred.size(2), W = pred.size(3);
    const float *g = tensor_arg<float>(op, "gt", gt, dev, {V, 3, H, W});
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && H <= 0x7FFFFFFF && W <= 0x7FFFFFFF, "ssim_images: at least one view and one pixel are required");
    const auto f64 = torch::dtype(torch::kFloat64).device(dev);
    Tensor sum = torch::empty({V, 3, 2}, f64), mean = torch::empty({V, 2}, f64);
    Tensor workspace = torch::empty({(int64_t)(EGR_SSIM_WORKSPACE_BYTES(V, H, W) / 8)}, f64);
    const int rc = egr_ssim_images(dev.index(), (uint32_t)V, (uint32_t)H, (uint32_t)W, p, g, sum.data_ptr<double>(), mean.data_ptr<double>(), workspace.data_ptr(), current_stream());
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
    const char *op = "eval_frames";
    struct In { const c10::optional<Tensor> *t; const char *name; bool pixel_major; int64_t channels; };
    const In in[13] = {{&final, "final", true, 3}, {&rgb, "rgb", true, 3}, {&depth, "depth", true, 1}, {&normal, "normal", true, 3}, {&roughness, "roughness", true, 1}, {&f0, "f0", true, 3},
                       {&t_final, "t_final", false, 3}, {&t_diffuse, "t_diffuse", false, 3}, {&t_specular, "t_specular", false, 3}, {&t_depth, "t_depth", false, 1},
                       {&t_normal, "t_normal", false, 3}, {&t_roughness, "t_roughness", false, 1}, {&t_f0, "t_f0", false, 3}};
    const Tensor *first = nullptr;
    int64_t V = 0, H = 0, W = 0;
    for (int i = 0; i < 13 && !first; i++) {
        if (!given(*in[i].t)) continue;
        first = &**in[i].t;
        const int64_t want_dim = i == 0 || !in[i].pixel_major ? 4 : 5;
        TORCH_CHECK(first->dim() == want_dim, "eval_frames: ", in[i].name, " must have ", want_dim, " dimensions, got ", first->sizes());
        V = first->size(0), H = first->size(want_dim - (in[i].pixel_major ? 3 : 2)), W = first->size(want_dim - (in[i].pixel_major ? 2 : 1));
    }
    TORCH_CHECK(first && first->is_cuda(), "eval_frames: at least one GPU tensor is required");
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && H <= 0x7FFFFFFF && W <= 0x7FFFFFFF, "eval_frames: at least one view and one pixel are required");
    TORCH_CHECK(kinds >= 0 && kinds <= 0xFFFFFFFFll && rounding >= 0 && rounding <= 0xFFFFFFFFll && depth_mode >= 0 && depth_mode <= 0xFFFFFFFFll, "eval_frames: kinds, rounding and depth_mode are the header's unsigned constants");
    const c10::Device dev = first->device();
    const c10::DeviceGuard guard(dev);
    const float *p[13];
    for (int i = 0; i < 13; i++)
        p[i] = tensor_arg<float>(op, in[i].name, *in[i].t, dev, i == 0 ? Shape{V, H, W, 3} : in[i].pixel_major ? Shape{V, EGR_NUM_STEPS, H, W, in[i].channels} : Shape{V, in[i].channels, H, W}, false);
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
struct VoxelTable {
    c10::Device dev;
    int64_t *keys, *acc, *status;
    uint64_t cap;
};
static VoxelTable voxel_table(const char *op, const Tensor &keys, const Tensor &acc, const Tensor &status) {
    TORCH_CHECK(keys.defined() && keys.is_cuda(), op, ": keys must be a contiguous int64 [cap] GPU tensor"); // (a CPU tensor is refused, not dereferenced)
    VoxelTable t{keys.device(), nullptr, nullptr, nullptr, 0};
    t.keys = tensor_arg<int64_t>(op, "keys ([cap])", keys, t.dev, {-1});
    t.cap = (uint64_t)keys.size(0);
    t.acc = tensor_arg<int64_t>(op, "acc", acc, t.dev, {keys.size(0), 4});
    t.status = tensor_arg<int64_t>(op, "status", status, t.dev, Shape::elements(EGR_VOXEL_STATUS_WORDS));
    return t;
}
static void voxel_accumulate(const Tensor &keys, const Tensor &acc, const Tensor &status, const Tensor &c2w, const Tensor &origin, const Tensor &view_size, const Tensor &depth,
                             const Tensor &colour, const c10::optional<Tensor> &colour_table, double voxel_scale, double colour_max, const c10::optional<Tensor> &positions_out) {
    const char *op = "voxel_accumulate";
    const VoxelTable T = voxel_table(op, keys, acc, status);
    const c10::Device dev = T.dev;
    const c10::DeviceGuard guard(dev);
    const float *pdepth = tensor_arg<float>(op, "depth ([V,H,W])", depth, dev, {-1, -1, -1});
    const int64_t V = depth.size(0), H = depth.size(1), W = depth.size(2);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && V <= 65535 && H <= (1 << 20) && W <= (1 << 20), "voxel_accumulate: at least one view and one pixel are required");
    const double *pc2w = tensor_arg<double>(op, "c2w", c2w, dev, {V, 3, 3}), *porigin = tensor_arg<double>(op, "origin", origin, dev, {V, 3}), *pview = tensor_arg<double>(op, "view_size", view_size, dev, {V});
    const bool u8 = colour.defined() && colour.scalar_type() == torch::kUInt8;
    const uint8_t *colour8 = u8 ? tensor_arg<uint8_t>(op, "colour", colour, dev, {V, H, W, 3}) : nullptr;
    const float *colour32 = u8 ? nullptr : tensor_arg<float>(op, "colour (fp32 or uint8)", colour, dev, {V, H, W, 3});
    const float *table = u8 ? tensor_arg<float>(op, "colour_table (uint8 colours need it)", colour_table, dev, Shape::elements(256)) : nullptr;
    double *pos = tensor_arg<double>(op, "positions_out", positions_out, dev, {V, H, W, 3}, false);
    const int rc = egr_voxel_accumulate(dev.index(), T.keys, T.acc, T.status, T.cap, (uint32_t)V, (uint32_t)H, (uint32_t)W, pc2w, porigin, pview, pdepth, colour32, colour8, table, voxel_scale,
                                        colour_max, pos, current_stream());
    TORCH_CHECK(rc == 0, egr_voxel_last_error());
}
// Growth: every occupied slot of (src_keys, src_acc) is inserted into the initialised table (keys, acc); the slots it claims are added to status[0].
static void voxel_rehash(const Tensor &keys, const Tensor &acc, const Tensor &status, const Tensor &src_keys, const Tensor &src_acc) {
    const VoxelTable T = voxel_table("voxel_rehash", keys, acc, status), S = voxel_table("voxel_rehash", src_keys, src_acc, status);
    TORCH_CHECK(S.dev == T.dev, "voxel_rehash: both tables must be on one device");
    const c10::DeviceGuard guard(T.dev);
    const int rc = egr_voxel_rehash(T.dev.index(), T.keys, T.acc, T.status, T.cap, S.keys, S.acc, S.cap, current_stream());
    TORCH_CHECK(rc == 0, egr_voxel_last_error());
}
// The voxels with count >= min_count in the order of torch.unique(dim=0): (coords int32 [n,3], points fp32 [n,3], colors fp32 [n,3], counts int32 [n], the largest
// count of the table). max_rows bounds n (the table's occupied slots always do). ONE host synchronisation: the read-back of n.
static std::tuple<Tensor, Tensor, Tensor, Tensor, int64_t> voxel_extract(const Tensor &keys, const Tensor &acc, const Tensor &status, int64_t min_count, double voxel_scale, int64_t max_rows) {
    const VoxelTable T = voxel_table("voxel_extract", keys, acc, status);
    TORCH_CHECK(min_count >= 0 && min_count <= 0xFFFFFFFFll, "voxel_extract: min_count must be in 0..2^32-1");
    TORCH_CHECK(max_rows >= 1 && max_rows <= (int64_t)T.cap, "voxel_extract: max_rows must be in 1..cap");
    const c10::Device dev = T.dev;
    const c10::DeviceGuard guard(dev);
    const auto i32 = torch::dtype(torch::kInt32).device(dev), f32 = torch::dtype(torch::kFloat32).device(dev);
    Tensor coords = torch::empty({max_rows, 3}, i32), points = torch::empty({max_rows, 3}, f32), colors = torch::empty({max_rows, 3}, f32), counts = torch::empty({max_rows}, i32);
    const size_t bytes = egr_voxel_extract_workspace_bytes(dev.index(), (uint64_t)max_rows);
    TORCH_CHECK(bytes != 0, egr_voxel_last_error());
    Tensor workspace = torch::empty({(int64_t)((bytes + 15) / 16) * 2}, torch::dtype(torch::kInt64).device(dev)); // (the caching allocator aligns to 512 bytes)
    uint64_t host[2] = {0, 0};
    const int rc = egr_voxel_extract(dev.index(), T.keys, T.acc, T.status, T.cap, (uint32_t)min_count, voxel_scale, (uint64_t)max_rows, coords.data_ptr<int32_t>(), points.data_ptr<float>(),
                                     colors.data_ptr<float>(), counts.data_ptr<int32_t>(), host, workspace.data_ptr(), (size_t)workspace.numel() * 8, current_stream());
    TORCH_CHECK(rc == 0, egr_voxel_last_error());
    const int64_t n = (int64_t)host[0];
    return {coords.narrow(0, 0, n), points.narrow(0, 0, n), colors.narrow(0, 0, n), counts.narrow(0, 0, n), (int64_t)host[1]};
}

// The training views in fp16, part 1 (egr_viewset_ingest, csrc/viewset.hip): the views of one chunk into slots first_slot .. first_slot + V of the store, in one
// launch on the current stream. sources[kind]: a contiguous uint8 or fp32 [V,Hs,Ws,Cs] GPU tensor or None (absent); tables[kind]: the contiguous half [256] GPU
// table of a uint8 source, None for fp32; planes[kind]: the store's contiguous half [slots,C,H,W]; depth_range: contiguous fp32 [slots,2]. One entry per kind each.
static void viewset_ingest(const c10::List<c10::optional<Tensor>> &sources, const c10::List<c10::optional<Tensor>> &tables, std::vector<Tensor> planes, const Tensor &depth_range,
                           int64_t first_slot) {
    const char *op = "viewset_ingest";
    TORCH_CHECK(sources.size() == EGR_VIEWSET_KINDS && tables.size() == EGR_VIEWSET_KINDS && planes.size() == EGR_VIEWSET_KINDS,
                "viewset_ingest: sources, tables and planes must have one entry per kind (", EGR_VIEWSET_KINDS, ")");
    const c10::Device dev = gpu_of(op, "depth_range", depth_range);
    const c10::DeviceGuard guard(dev);
    float *range = tensor_arg<float>(op, "depth_range ([slots,2])", depth_range, dev, {-1, 2});
    const int64_t slots = depth_range.size(0);
    TORCH_CHECK(first_slot >= 0 && first_slot <= slots, "viewset_ingest: first_slot must be in 0..slots, got ", first_slot);
    egr_viewset_source table[EGR_VIEWSET_KINDS] = {};
    int64_t V = -1, Hs = -1, Ws = -1, H = -1, W = -1; // (-1: any, until the first tensor that has it fixes it for the rest)
    for (size_t k = 0; k < EGR_VIEWSET_KINDS; k++) {
        const std::string at = "[" + std::to_string(k) + "]";
        const int64_t C = (k == EGR_VIEWSET_DEPTH || k == 5) ? 1 : 3;
        void *store = tensor_arg<at::Half>(op, "planes" + at + " (the planes of every kind share one image size)", planes[k], dev, {slots, C, H, W});
        H = planes[k].size(2), W = planes[k].size(3);
        const c10::optional<Tensor> s = sources.get(k);
        const void *lookup = tensor_arg<at::Half>(op, "tables" + at, tables.get(k), dev, Shape::elements(256), false);
        if (!given(s)) continue; // (the table of an absent kind is ignored)
        const bool u8 = s->scalar_type() == torch::kUInt8;
        const std::string name = "sources" + at + " (uint8 or fp32; the sources of one call share [V,Hs,Ws])";
        table[k].data = u8 ? (const void *)tensor_arg<uint8_t>(op, name, s, dev, {V, Hs, Ws, -1}) : (const void *)tensor_arg<float>(op, name, s, dev, {V, Hs, Ws, -1});
        V = s->size(0), Hs = s->size(1), Ws = s->size(2);
        table[k].table = lookup, table[k].planes = store, table[k].channels = (uint32_t)s->size(3);
        table[k].dtype = u8 ? EGR_VIEWSET_U8 : EGR_VIEWSET_F32;
    }
    TORCH_CHECK(V >= 1, "viewset_ingest: at least one kind with at least one view is required");
    TORCH_CHECK(Hs > 0 && Ws > 0 && H > 0 && W > 0 && std::max(std::max(V, Hs), std::max(std::max(Ws, H), W)) <= 65535, "viewset_ingest: V and the image sizes must be in 1..65535");
    const int rc = egr_viewset_ingest(dev.index(), table, (uint32_t)V, (uint32_t)Hs, (uint32_t)Ws, (uint32_t)H, (uint32_t)W, (uint32_t)first_slot, (uint32_t)slots, range, current_stream());
    TORCH_CHECK(rc == 0, egr_viewset_last_error());
}
// The training views in fp16, part 2 (egr_viewset_gather): rows v < len(indices) of the fp32 outputs = the stored views indices[v], exactly float(half), and their
// camera rows, in one launch per 64 indices on the current stream - `indices` are host integers: no upload, no synchronisation. planes[kind]: the store's half
// [slots,C,H,W]; R [slots,3,3], centers [slots,3], fovy [slots]: its camera table; out[kind]: a contiguous fp32 [>= V,C,H,W] tensor or None (not wanted);
// out_R / out_centers / out_fovy: contiguous fp32 with >= V rows. Only the first V rows of an output are written.
static void viewset_gather(std::vector<Tensor> planes, const Tensor &R, const Tensor &centers, const Tensor &fovy, int64_t num_filled, std::vector<int64_t> indices,
                           const c10::List<c10::optional<Tensor>> &out, const Tensor &out_R, const Tensor &out_centers, const Tensor &out_fovy) {
    const char *op = "viewset_gather";
    TORCH_CHECK(planes.size() == EGR_VIEWSET_KINDS && out.size() == EGR_VIEWSET_KINDS, "viewset_gather: planes and out must have one entry per kind (", EGR_VIEWSET_KINDS, ")");
    const int64_t V = (int64_t)indices.size();
    TORCH_CHECK(V >= 1, "viewset_gather: at least one index is required");
    const c10::Device dev = gpu_of(op, "fovy", fovy);
    const c10::DeviceGuard guard(dev);
    egr_viewset_store store = {};
    egr_viewset_batch batch = {};
    store.fovy = tensor_arg<float>(op, "fovy ([slots])", fovy, dev, {-1});
    const int64_t slots = fovy.size(0);
    TORCH_CHECK(num_filled >= 0 && num_filled <= slots, "viewset_gather: num_filled must be in 0..slots");
    store.R = tensor_arg<float>(op, "R", R, dev, {slots, 3, 3}), store.centers = tensor_arg<float>(op, "centers", centers, dev, {slots, 3});
    batch.R = tensor_arg<float>(op, "out_R", out_R, dev, Shape::at_least(V, {3, 3})), batch.centers = tensor_arg<float>(op, "out_centers", out_centers, dev, Shape::at_least(V, {3}));
    batch.fovy = tensor_arg<float>(op, "out_fovy", out_fovy, dev, Shape::at_least(V, {}));
    int64_t H = -1, W = -1; // (-1: any, until the first kind fixes it for the rest)
    for (size_t k = 0; k < EGR_VIEWSET_KINDS; k++) {
        const std::string at = "[" + std::to_string(k) + "]";
        const int64_t C = (k == EGR_VIEWSET_DEPTH || k == 5) ? 1 : 3;
        store.planes[k] = tensor_arg<at::Half>(op, "planes" + at + " (the planes of every kind share one image size)", planes[k], dev, {slots, C, H, W});
        H = planes[k].size(2), W = planes[k].size(3);
        batch.targets[k] = tensor_arg<float>(op, "out" + at, out.get(k), dev, Shape::at_least(V, {C, H, W}), false);
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

// Prior views, part 1 (egr_prior_pairs, csrc/priors.hip): the sparse depth maps of V views and their (predicted, sparse) pairs in row-major order. cams: fp32
// [V,25] (priors.py: camera_rows); points: fp32 [M,3], the views' world-space points one after the other; offsets: V + 1 host integers ascending from 0 to M;
// depth: fp32 [V,H,W,1|3]. Returns sparse fp32 [V,H,W] (+inf = empty), pairs_x / pairs_y fp32 [V,H*W], count / dropped int32 [V]. Current stream; the offsets are
// uploaded, nothing is read back.
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> prior_pairs(const Tensor &cams, const Tensor &points, std::vector<int64_t> offsets, const Tensor &depth) {
    const char *op = "prior_pairs";
    const c10::Device dev = gpu_of(op, "depth", depth);
    const c10::DeviceGuard guard(dev);
    egr_prior_pairs_args a = {};
    a.depth = tensor_arg<float>(op, "depth ([V,H,W,1|3])", depth, dev, {-1, -1, -1, -1});
    const int64_t V = depth.size(0), H = depth.size(1), W = depth.size(2);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && std::max(V, std::max(H, W)) <= 65535, "prior_pairs: V and the image sizes must be in 1..65535");
    a.cams = tensor_arg<float>(op, "cams", cams, dev, {V, EGR_PRIOR_CAM_FLOATS});
    a.points = tensor_arg<float>(op, "points ([M,3])", points, dev, {-1, 3});
    TORCH_CHECK((int64_t)offsets.size() == V + 1, "prior_pairs: offsets must have V + 1 = ", V + 1, " entries, got ", offsets.size());
    std::vector<int32_t> host(offsets.size());
    for (size_t i = 0; i < offsets.size(); i++) {
        TORCH_CHECK(offsets[i] >= 0 && offsets[i] <= points.size(0), "prior_pairs: offsets[", i, "] = ", offsets[i], " is outside the ", points.size(0), " points");
        host[i] = (int32_t)(uint32_t)offsets[i];
    }
    TORCH_CHECK(points.size(0) <= 0xFFFFFFFFll && offsets.back() == points.size(0), "prior_pairs: offsets must end at the number of points");
    const Tensor offsets_dev = torch::from_blob(host.data(), {V + 1}, torch::kInt32).to(dev);
    const auto f32 = torch::dtype(torch::kFloat32).device(dev), i32 = torch::dtype(torch::kInt32).device(dev);
    Tensor sparse = torch::empty({V, H, W}, f32), pairs_x = torch::empty({V, H * W}, f32), pairs_y = torch::empty({V, H * W}, f32), count = torch::empty({V}, i32), dropped = torch::empty({V}, i32);
    a.num_views = (uint32_t)V, a.height = (uint32_t)H, a.width = (uint32_t)W, a.depth_channels = (uint32_t)depth.size(3);
    a.offsets = (const uint32_t *)host.data(), a.offsets_dev = (const uint32_t *)offsets_dev.data_ptr<int32_t>();
    a.sparse = sparse.data_ptr<float>(), a.pairs_x = pairs_x.data_ptr<float>(), a.pairs_y = pairs_y.data_ptr<float>();
    a.count = (uint32_t *)count.data_ptr<int32_t>(), a.dropped = (uint32_t *)dropped.data_ptr<int32_t>();
    const int rc = egr_prior_pairs(dev.index(), &a, current_stream());
    TORCH_CHECK(rc == 0, egr_prior_last_error());
    return {sparse, pairs_x, pairs_y, count, dropped};
}
// Prior views, part 2 (egr_prior_fit): y = a x + b per view over the first counts[v] pairs of pairs_x / pairs_y [V,stride]. method 0 (RANSAC): samples is a CPU
// int32 [V,num_iters,S] table of pair indices (row (v, it) uses its first sample_sizes[v]); top_ks[v] residuals score and refit. method 1: the least-squares fit
// of all pairs (samples None). Returns ab fp32 [V,2], best_iteration int32 [V], best_error fp64 [V], hyp_error fp64 [V,num_iters], hyp_model fp32 [V,num_iters,4]
// (w, b, threshold, bits of the ties taken) and the inlier mask uint8 [V,stride] (zeros beyond a view's count; [V,0] unless want_mask). Current stream; the
// table and the sizes are uploaded, nothing is read back.
static std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> prior_fit(const Tensor &pairs_x, const Tensor &pairs_y, std::vector<int64_t> counts, std::vector<int64_t> sample_sizes,
                                                                            std::vector<int64_t> top_ks, const c10::optional<Tensor> &samples, int64_t method, bool want_mask) {
    const char *op = "prior_fit";
    const c10::Device dev = gpu_of(op, "pairs_x", pairs_x);
    const c10::DeviceGuard guard(dev);
    egr_prior_fit_args a = {};
    a.pairs_x = tensor_arg<float>(op, "pairs_x ([V,stride])", pairs_x, dev, {-1, -1});
    const int64_t V = pairs_x.size(0), stride = pairs_x.size(1);
    a.pairs_y = tensor_arg<float>(op, "pairs_y", pairs_y, dev, {V, stride});
    TORCH_CHECK(V >= 1 && V <= 65535 && stride >= 1 && stride <= 65535ll * 65535ll, "prior_fit: V must be in 1..65535 and the stride in 1..65535^2");
    TORCH_CHECK(method == EGR_PRIOR_RANSAC || method == EGR_PRIOR_LSTSQ, "prior_fit: method must be 0 (RANSAC) or 1 (least squares), got ", method);
    TORCH_CHECK((int64_t)counts.size() == V && (int64_t)sample_sizes.size() == V && (int64_t)top_ks.size() == V, "prior_fit: counts, sample_sizes and top_ks must have one entry per view (", V, ")");
    std::vector<int32_t> views((size_t)V * 4, 0);
    for (int64_t v = 0; v < V; v++) {
        const int64_t e[3] = {counts[(size_t)v], sample_sizes[(size_t)v], top_ks[(size_t)v]};
        for (int j = 0; j < 3; j++) {
            TORCH_CHECK(e[j] >= 0 && e[j] <= 0xFFFFFFFFll, "prior_fit: view ", v, ": counts, sample_sizes and top_ks must be in 0..2^32-1");
            views[(size_t)v * 4 + j] = (int32_t)(uint32_t)e[j];
        }
    }
    int64_t iters = 0, S = 0;
    Tensor samples_dev;
    if (method == EGR_PRIOR_RANSAC) {
        TORCH_CHECK(given(samples) && samples->device().is_cpu() && samples->scalar_type() == torch::kInt32 && samples->is_contiguous() && samples->dim() == 3 && samples->size(0) == V,
                    "prior_fit: samples must be a contiguous CPU int32 tensor [V,num_iters,S] (the table is checked on the host, where it was made)");
        iters = samples->size(1), S = samples->size(2);
        TORCH_CHECK(iters >= 1 && iters <= 65535 && S >= 1 && S <= EGR_PRIOR_MAX_SAMPLE, "prior_fit: num_iters must be in 1..65535 and the table's width in 1..", EGR_PRIOR_MAX_SAMPLE);
        samples_dev = samples->to(dev);
        a.samples = samples->data_ptr<int32_t>(), a.samples_dev = samples_dev.data_ptr<int32_t>();
    }
    const Tensor views_dev = torch::from_blob(views.data(), {V, 4}, torch::kInt32).to(dev);
    const auto f32 = torch::dtype(torch::kFloat32).device(dev), f64 = torch::dtype(torch::kFloat64).device(dev), i32 = torch::dtype(torch::kInt32).device(dev);
    Tensor ab = torch::empty({V, 2}, f32), best_iteration = torch::empty({V}, i32), best_error = torch::empty({V}, f64), hyp_error = torch::empty({V, iters}, f64),
           hyp_model = torch::empty({V, iters, 4}, f32), inliers = torch::zeros({V, want_mask ? stride : 0}, torch::dtype(torch::kUInt8).device(dev));
    a.num_views = (uint32_t)V, a.pair_stride = (uint32_t)stride, a.num_iters = (uint32_t)iters, a.sample_stride = (uint32_t)S, a.method = (uint32_t)method;
    a.views = (const uint32_t *)views.data(), a.views_dev = (const uint32_t *)views_dev.data_ptr<int32_t>();
    a.hyp_error = iters ? hyp_error.data_ptr<double>() : nullptr, a.hyp_model = iters ? hyp_model.data_ptr<float>() : nullptr;
    a.ab = ab.data_ptr<float>(), a.best_iteration = best_iteration.data_ptr<int32_t>(), a.best_error = best_error.data_ptr<double>();
    a.inliers = want_mask ? inliers.data_ptr<uint8_t>() : nullptr;
    const int rc = egr_prior_fit(dev.index(), &a, current_stream());
    TORCH_CHECK(rc == 0, egr_prior_last_error());
    return {ab, best_iteration, best_error, hyp_error, hyp_model, inliers};
}
// Prior views, part 3 (egr_prior_finish): one pass over V views - the distance image of depth * a + b with (a, b) = ab[v] read on the device, the world normals
// and f0 from metalness. depth fp32 [V,H,W,1|3], normal fp32 [V,H,W,3] (camera space), metalness fp32 [V,H,W] or [V,H,W,1] or None. Returns distance [V,H,W,1],
// normals [V,H,W,3], f0 [V,H,W,3] ([0] without metalness): new tensors, the dataset's pixel-major layout. Current stream, no synchronisation.
static std::tuple<Tensor, Tensor, Tensor> prior_finish(const Tensor &cams, const Tensor &ab, const Tensor &depth, const Tensor &normal, const c10::optional<Tensor> &metalness) {
    const char *op = "prior_finish";
    const c10::Device dev = gpu_of(op, "depth", depth);
    const c10::DeviceGuard guard(dev);
    egr_prior_finish_args a = {};
    a.depth = tensor_arg<float>(op, "depth ([V,H,W,1|3])", depth, dev, {-1, -1, -1, -1});
    const int64_t V = depth.size(0), H = depth.size(1), W = depth.size(2);
    TORCH_CHECK(V >= 1 && H >= 1 && W >= 1 && std::max(V, std::max(H, W)) <= 65535, "prior_finish: V and the image sizes must be in 1..65535");
    a.cams = tensor_arg<float>(op, "cams", cams, dev, {V, EGR_PRIOR_CAM_FLOATS}), a.ab = tensor_arg<float>(op, "ab", ab, dev, {V, 2});
    a.normal = tensor_arg<float>(op, "normal", normal, dev, {V, H, W, 3});
    a.metalness = tensor_arg<float>(op, "metalness ([V,H,W] or [V,H,W,1])", metalness, dev, Shape::elements(V * H * W), false);
    const auto f32 = torch::dtype(torch::kFloat32).device(dev);
    Tensor distance = torch::empty({V, H, W, 1}, f32), world = torch::empty({V, H, W, 3}, f32), f0 = a.metalness ? torch::empty({V, H, W, 3}, f32) : torch::empty({0}, f32);
    a.num_views = (uint32_t)V, a.height = (uint32_t)H, a.width = (uint32_t)W, a.depth_channels = (uint32_t)depth.size(3);
    a.distance = distance.data_ptr<float>(), a.normal_out = world.data_ptr<float>(), a.f0 = a.metalness ? f0.data_ptr<float>() : nullptr;
    const int rc = egr_prior_finish(dev.index(), &a, current_stream());
    TORCH_CHECK(rc == 0, egr_prior_last_error());
    return {distance, world, f0};
}

// unit-test hook (egr_debug_lean_arith): (a / b, sqrt(a)) as the hot kernels' division and square root compute them
static std::tuple<Tensor, Tensor> debug_lean_arith(const Tensor &a, const Tensor &b) {
    TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.device() == b.device() && a.numel() == b.numel(), "debug_lean_arith: two tensors of one size on one GPU expected");
    const c10::DeviceGuard guard(a.device());
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
    m.def("prior_pairs(Tensor cams, Tensor points, int[] offsets, Tensor depth) -> (Tensor sparse, Tensor pairs_x, Tensor pairs_y, Tensor count, Tensor dropped)", &prior_pairs);
    m.def("prior_fit(Tensor pairs_x, Tensor pairs_y, int[] counts, int[] sample_sizes, int[] top_ks, Tensor? samples, int method=0, bool want_mask=False) -> "
          "(Tensor ab, Tensor best_iteration, Tensor best_error, Tensor hyp_error, Tensor hyp_model, Tensor inliers)",
          &prior_fit);
    m.def("prior_finish(Tensor cams, Tensor ab, Tensor depth, Tensor normal, Tensor? metalness) -> (Tensor distance, Tensor normal_world, Tensor f0)", &prior_finish);
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
