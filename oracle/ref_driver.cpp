// =====================================================================================
// oracle/ref_driver.cpp  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.
//
// Runs the reference's own shader code on the CPU. This file is ours; at build time it
// #includes the reference's shaders.cu (raygen + intersection programs, forward and
// backward pass, utils/, core/) from the reference directory, and the part of its
// optix/bvh_wrapper.cu that comes before the host launcher (the recipe in oracle/Makefile
// writes that part to oracle/_ref/, untracked). The stand-in headers of oracle/ref_shim/
// make that code plain C++. Nothing of the reference is restated here: this file supplies
// what OptiX and raytracer.cpp supply around the programs -
//   * buffers and the Params struct,
//   * the instance inverse transform,
//   * optixTraverse as brute force over the instances,
//   * the launch sequence of Raytracer::raytrace().
// Single-threaded; the shim's atomicAdd is a plain add.
//
// COMPILER: the reference writes make_float2(rnd(seed), rnd(seed)) (bounce sample, camera
// jitter). C++ leaves the evaluation order of function arguments open: clang++ goes left to
// right - what nvcc's device code does, and what the oracle and the HIP kernels assume -,
// g++ right to left (the two draws swap). The recipe therefore fixes ROCm's clang++, and
// tests/test_oracle_vs_reference.py pins the order in the built library.
// =====================================================================================
#include <optix.h>

#include <cstdlib>
#include <vector>

uint3 threadIdx = {0, 0, 0}, blockIdx = {0, 0, 0}, blockDim = {1, 1, 1};
EgrShimRay egr_shim_ray;

#include "shaders.cu"          // the reference's, from EGR_REFERENCE_DIR
#include "bvh_wrapper_head.inc" // the reference's create_transform_matrix + _populateBVH, from oracle/_ref/

namespace {

struct ConfigStore { // the device tensors behind core/config.h's pointers
    float exp_power = 3.0f, alpha_threshold = 0.005f, transmittance_threshold = 0.01f;
    bool accumulate_samples = false, jitter_primary_rays = true;
    int num_bounces = 2;
    float global_scale_factor = 1.0f;
    float loss_weight_diffuse = 1, loss_weight_specular = 1, loss_weight_depth = 1, loss_weight_normal = 1, loss_weight_f0 = 1, loss_weight_roughness = 1;
    float eps_forward_normalization = 1e-12f, eps_scale_grad = 1e-12f, eps_ray_surface_offset = 0.01f, eps_min_roughness = 0.01f;
    float reflection_invalid_normal_threshold = 0.7f, backfacing_invalid_normal_threshold = 0.9f, backfacing_max_dist = 0.1f;
};

struct List { // storage of one PerPixelLinkedList; entries are malloc'ed and never touched before they are written
    std::vector<uint32_t> head;
    uint32_t total_hits = 0;
    size_t capacity = 0;
    uint32_t *gaussian_ids = nullptr, *previous_entries = nullptr;
    float *distances = nullptr, *alphas = nullptr, *transmittances = nullptr, *gaussvals = nullptr;
    float3 *local_hits = nullptr;
    void release() {
        std::free(gaussian_ids), std::free(previous_entries), std::free(distances), std::free(alphas), std::free(transmittances), std::free(gaussvals), std::free(local_hits);
        gaussian_ids = previous_entries = nullptr, distances = alphas = transmittances = gaussvals = nullptr, local_hits = nullptr, capacity = 0;
    }
    bool reserve(size_t n) {
        if (n <= capacity) return true;
        release();
        gaussian_ids = (uint32_t *)std::malloc(n * sizeof(uint32_t)), previous_entries = (uint32_t *)std::malloc(n * sizeof(uint32_t));
        distances = (float *)std::malloc(n * sizeof(float)), alphas = (float *)std::malloc(n * sizeof(float));
        transmittances = (float *)std::malloc(n * sizeof(float)), gaussvals = (float *)std::malloc(n * sizeof(float));
        local_hits = (float3 *)std::malloc(n * sizeof(float3));
        if (!(gaussian_ids && previous_entries && distances && alphas && transmittances && gaussvals && local_hits)) return release(), false;
        capacity = n;
        return true;
    }
    PerPixelLinkedList view() {
        PerPixelLinkedList l;
        l.head_per_pixel = head.data(), l.total_hits = &total_hits, l.gaussian_ids = gaussian_ids, l.distances = distances, l.alphas = alphas;
        l.transmittances = transmittances, l.local_hits = local_hits, l.gaussvals = gaussvals, l.previous_entries = previous_entries;
        return l;
    }
};

struct Ref {
    int W, H;
    size_t P;
    ConfigStore cfg;
    // camera
    float3 origin = {0, 0, 0};
    float3 c2w[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, w2c[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    float fov = 1.0f, znear = 0.01f, zfar = 999.9f;
    // framebuffer
    std::vector<float> out_rgb, out_depth, out_normal, out_f0, out_roughness, out_T, out_Ttot, out_ro, out_rd, out_final, out_denoised;
    std::vector<float> acc_rgb, acc_T, acc_Ttot, acc_depth, acc_normal, acc_f0, acc_roughness;
    int accumulated_sample_count = 0;
    std::vector<float> tg_diffuse, tg_specular, tg_depth, tg_normal, tg_f0, tg_roughness;
    // gaussians (live raw parameters) and their gradients
    uint32_t n = 0;
    std::vector<float> rgb, normal, f0, roughness, opacity, scale, mean, rotation;
    std::vector<float> d_rgb, d_normal, d_f0, d_roughness, d_opacity, d_scale, d_mean, d_rotation, total_weight;
    // metadata, stats
    bool grads_enabled = false;
    uint32_t total_num_calls = 0;
    std::vector<uint32_t> random_seeds;
    std::vector<int> num_accumulated, num_traversed;
    List fwd, bwd;
    // what update_bvh leaves behind: the reference kernel's instance records and their inverses
    std::vector<OptixInstance> instances;
    std::vector<float4> inverse; // [n][3]
    bool reverse_traversal = false;

    Ref(int w, int h) : W(w), H(h), P((size_t)w * h) {
        auto z = [&](std::vector<float> &v, size_t c) { v.assign(P * c, 0.0f); };
        z(out_rgb, 9), z(out_depth, 3), z(out_normal, 9), z(out_f0, 9), z(out_roughness, 3), z(out_T, 3), z(out_Ttot, 3), z(out_ro, 9), z(out_rd, 9);
        z(out_final, 3), z(out_denoised, 3);
        z(tg_diffuse, 3), z(tg_specular, 3), z(tg_depth, 1), z(tg_normal, 3), z(tg_f0, 3), z(tg_roughness, 1);
        reset_accumulators();
        random_seeds.assign(P, 0u), num_accumulated.assign(P, 0), num_traversed.assign(P, 0);
        fwd.head.assign(P, PerPixelLinkedList::NULL_PTR), bwd.head.assign(P, PerPixelLinkedList::NULL_PTR);
    }
    ~Ref() { fwd.release(), bwd.release(); }

    void reset_accumulators() { // FramebufferDataHolder::reset_accumulators
        auto z = [&](std::vector<float> &v, size_t c) { v.assign(P * c, 0.0f); };
        z(acc_rgb, 9), z(acc_T, 3), z(acc_Ttot, 3), z(acc_depth, 3), z(acc_normal, 9), z(acc_f0, 9), z(acc_roughness, 3);
        accumulated_sample_count = 0;
    }

    Gaussians gaussians() {
        Gaussians g;
        g.count = n;
        g.rgb = (const float3 *)rgb.data(), g.normal = (const float3 *)normal.data(), g.f0 = (const float3 *)f0.data();
        g.roughness = roughness.data(), g.opacity = opacity.data(), g.scale = (const float3 *)scale.data();
        g.mean = (const float3 *)mean.data(), g.rotation = (const float4 *)rotation.data();
        g.dL_drgb = (float3 *)d_rgb.data(), g.dL_dnormal = (float3 *)d_normal.data(), g.dL_df0 = (float3 *)d_f0.data();
        g.dL_droughness = d_roughness.data(), g.dL_dopacity = d_opacity.data(), g.dL_dscale = (float3 *)d_scale.data();
        g.dL_dmean = (float3 *)d_mean.data(), g.dL_drotation = (float4 *)d_rotation.data(), g.total_weight = total_weight.data();
        return g;
    }

    Params make_params() {
        Params p;
        p.image_width = (uint32_t)W, p.image_height = (uint32_t)H;
        p.camera.origin = &origin, p.camera.vertical_fov_radians = &fov, p.camera.rotation_c2w = c2w, p.camera.rotation_w2c = w2c;
        p.camera.znear = &znear, p.camera.zfar = &zfar;
        Config &c = p.config;
        c.exp_power = &cfg.exp_power, c.alpha_threshold = &cfg.alpha_threshold, c.transmittance_threshold = &cfg.transmittance_threshold;
        c.accumulate_samples = &cfg.accumulate_samples, c.jitter_primary_rays = &cfg.jitter_primary_rays, c.num_bounces = &cfg.num_bounces;
        c.global_scale_factor = &cfg.global_scale_factor;
        c.loss_weight_diffuse = &cfg.loss_weight_diffuse, c.loss_weight_specular = &cfg.loss_weight_specular, c.loss_weight_depth = &cfg.loss_weight_depth;
        c.loss_weight_normal = &cfg.loss_weight_normal, c.loss_weight_f0 = &cfg.loss_weight_f0, c.loss_weight_roughness = &cfg.loss_weight_roughness;
        c.eps_forward_normalization = &cfg.eps_forward_normalization, c.eps_scale_grad = &cfg.eps_scale_grad;
        c.eps_ray_surface_offset = &cfg.eps_ray_surface_offset, c.eps_min_roughness = &cfg.eps_min_roughness;
        c.reflection_invalid_normal_threshold = &cfg.reflection_invalid_normal_threshold;
        c.backfacing_invalid_normal_threshold = &cfg.backfacing_invalid_normal_threshold, c.backfacing_max_dist = &cfg.backfacing_max_dist;
        Framebuffer &f = p.framebuffer;
        f.output_rgb = (float3 *)out_rgb.data(), f.output_depth = out_depth.data(), f.output_normal = (float3 *)out_normal.data();
        f.output_f0 = (float3 *)out_f0.data(), f.output_roughness = out_roughness.data(), f.output_transmittance = out_T.data();
        f.output_total_transmittance = out_Ttot.data(), f.output_ray_origin = (float3 *)out_ro.data(), f.output_ray_direction = (float3 *)out_rd.data();
        f.output_final = (float3 *)out_final.data(), f.output_denoised = (float3 *)out_denoised.data();
        f.accumulated_rgb = (float3 *)acc_rgb.data(), f.accumulated_transmittance = acc_T.data(), f.accumulated_total_transmittance = acc_Ttot.data();
        f.accumulated_depth = acc_depth.data(), f.accumulated_normal = (float3 *)acc_normal.data(), f.accumulated_f0 = (float3 *)acc_f0.data();
        f.accumulated_roughness = acc_roughness.data(), f.accumulated_sample_count = &accumulated_sample_count;
        f.target_diffuse = (const float3 *)tg_diffuse.data(), f.target_specular = (const float3 *)tg_specular.data(), f.target_depth = tg_depth.data();
        f.target_normal = (const float3 *)tg_normal.data(), f.target_f0 = (const float3 *)tg_f0.data(), f.target_roughness = tg_roughness.data();
        f.num_pixels = (uint32_t)P;
        p.gaussians = gaussians();
        p.metadata.grads_enabled = &grads_enabled, p.metadata.total_num_calls = &total_num_calls, p.metadata.random_seeds = random_seeds.data();
        p.stats.num_accumulated_per_pixel = num_accumulated.data(), p.stats.num_traversed_per_pixel = num_traversed.data();
        p.ppll_forward = fwd.view(), p.ppll_backward = bwd.view();
        p.bvh_handle = 1;
        return p;
    }

    // BVHWrapper::update: the reference's instance kernel, its body called once per index, then the inverses.
    void update_bvh() {
        instances.assign(n, OptixInstance{});
        inverse.assign((size_t)n * 3, float4{0, 0, 0, 0});
        blockDim = {1, 1, 1}, threadIdx = {0, 0, 0};
        for (uint32_t i = 0; i < n; i++) {
            blockIdx = {i, 0, 0};
            _populateBVH(instances.data(), 1, (int)n, gaussians(), cfg.alpha_threshold, cfg.exp_power, cfg.global_scale_factor);
        }
        blockIdx = {0, 0, 0};
        // OptiX keeps the world-to-object transform of every instance and does not specify how it computes it. Here: the inverse of the 3x4 in fp64
        // (cofactors), rounded to fp32 - the correctly rounded answer, which any sound method is within a few ulps of.
        for (uint32_t i = 0; i < n; i++) {
            if (!instances[i].visibilityMask) continue; // (never traversed, never composited: its inverse is never read)
            const float *m = instances[i].transform;
            const double a[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}}, t[3] = {m[3], m[7], m[11]};
            double c[3][3];
            for (int r = 0; r < 3; r++)
                for (int q = 0; q < 3; q++) c[r][q] = a[(q + 1) % 3][(r + 1) % 3] * a[(q + 2) % 3][(r + 2) % 3] - a[(q + 1) % 3][(r + 2) % 3] * a[(q + 2) % 3][(r + 1) % 3];
            const double det = a[0][0] * c[0][0] + a[0][1] * c[1][0] + a[0][2] * c[2][0];
            for (int r = 0; r < 3; r++) {
                const double x = c[r][0] / det, y = c[r][1] / det, z = c[r][2] / det;
                inverse[(size_t)i * 3 + r] = {(float)x, (float)y, (float)z, (float)-(x * t[0] + y * t[1] + z * t[2])};
            }
        }
    }

    // Raytracer::raytrace() (raytracer.cpp:81-94)
    int launch(bool grads) {
        grads_enabled = grads, total_num_calls += 1; // MetaDataHolder::update
        std::fill(num_accumulated.begin(), num_accumulated.end(), 0), std::fill(num_traversed.begin(), num_traversed.end(), 0); // StatsDataHolder::reset
        for (List *l : {&fwd, &bwd}) l->total_hits = 0, std::fill(l->head.begin(), l->head.end(), PerPixelLinkedList::NULL_PTR); // PPLLDataHolder::reset
        // capacities for the whole launch (the lists' counters run on from pixel to pixel and from step to step, as upstream): every visible instance
        // on every step of every pixel; the backward list takes the composited hits, at most MAX_ITERATIONS * BUFFER_SIZE per step
        size_t visible = 0;
        for (const OptixInstance &I : instances) visible += I.visibilityMask ? 1 : 0;
        const size_t steps = MAX_BOUNCES + 1;
        if (!fwd.reserve(P * steps * visible + 1)) return 1;
        if (!bwd.reserve(grads ? P * steps * std::min(visible, (size_t)MAX_ITERATIONS * BUFFER_SIZE) + 1 : 1)) return 1;
        params = make_params();
        current = this;
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++) {
                egr_shim_ray.launch_index = {(unsigned)x, (unsigned)y, 0}, egr_shim_ray.launch_dimensions = {(unsigned)W, (unsigned)H, 1};
                __raygen__rg();
            }
        current = nullptr;
        if (cfg.accumulate_samples) accumulated_sample_count += 1;
        return 0;
    }
    static Ref *current;
};
Ref *Ref::current = nullptr;

inline float3 xform_point(const float4 *w, float3 p) {
    return {w[0].x * p.x + w[0].y * p.y + w[0].z * p.z + w[0].w, w[1].x * p.x + w[1].y * p.y + w[1].z * p.z + w[1].w, w[2].x * p.x + w[2].y * p.y + w[2].z * p.z + w[2].w};
}
inline float3 xform_vector(const float4 *w, float3 v) {
    return {w[0].x * v.x + w[0].y * v.y + w[0].z * v.z, w[1].x * v.x + w[1].y * v.y + w[1].z * v.z, w[2].x * v.x + w[2].y * v.y + w[2].z * v.z};
}

// the segment [tmin, tmax] of the object-space ray against the unit cube [-1, 1]^3: the one AABB of the reference's BLAS
bool segment_overlaps_unit_cube(float3 o, float3 d, float tmin, float tmax) {
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    float t0 = tmin, t1 = tmax;
    for (int a = 0; a < 3; a++) {
        if (dd[a] != 0.0f) {
            float ta = (-1.0f - oo[a]) / dd[a], tb = (1.0f - oo[a]) / dd[a];
            if (ta > tb) std::swap(ta, tb);
            t0 = std::max(t0, ta), t1 = std::min(t1, tb);
        } else if (oo[a] < -1.0f || oo[a] > 1.0f) {
            return false;
        }
    }
    return t0 <= t1;
}

} // namespace

// ------------------------------------------------------------------------------------- what OptiX supplies to the programs
OptixTraversableHandle optixGetInstanceTraversableFromIAS(OptixTraversableHandle, unsigned int instance_index) { return (OptixTraversableHandle)instance_index + 1; }
const float4 *optixGetInstanceTransformFromHandle(OptixTraversableHandle h) { return reinterpret_cast<const float4 *>(Ref::current->instances[h - 1].transform); }
const float4 *optixGetInstanceInverseTransformFromHandle(OptixTraversableHandle h) { return &Ref::current->inverse[(size_t)(h - 1) * 3]; }

// Brute force: every instance whose visibility mask meets the ray's, in index order (or in reverse: the order in which an acceleration structure
// reports candidates is unspecified, and the tie tests show with this switch which outputs depend on it). The intersection program runs for every
// instance whose box the segment overlaps. A ray with a non-finite component is invalid for OptiX; it reports nothing here (the driver's choice,
// not the reference's: its programs never see such a ray).
void optixTraverse(OptixTraversableHandle, float3 ray_origin, float3 ray_direction, float tmin, float tmax, float, OptixVisibilityMask visibility_mask,
                   unsigned int, unsigned int, unsigned int, unsigned int, unsigned int &p0, unsigned int &p1, unsigned int &p2, unsigned int &p3,
                   unsigned int &p4, unsigned int &p5, unsigned int &p6, unsigned int &p7) {
    Ref *r = Ref::current;
    unsigned int *p[8] = {&p0, &p1, &p2, &p3, &p4, &p5, &p6, &p7};
    if (!(std::isfinite(ray_origin.x + ray_origin.y + ray_origin.z) && std::isfinite(ray_direction.x + ray_direction.y + ray_direction.z))) return;
    for (int k = 0; k < 8; k++) egr_shim_ray.payload[k] = *p[k];
    const uint32_t n = (uint32_t)r->instances.size();
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t i = r->reverse_traversal ? n - 1 - k : k;
        if (!(r->instances[i].visibilityMask & visibility_mask)) continue;
        const float4 *w = &r->inverse[(size_t)i * 3];
        const float3 lo = xform_point(w, ray_origin), ld = xform_vector(w, ray_direction);
        if (!segment_overlaps_unit_cube(lo, ld, tmin, tmax)) continue;
        egr_shim_ray.object_origin = lo, egr_shim_ray.object_direction = ld, egr_shim_ray.instance_index = i;
        __intersection__gaussian();
    }
    for (int k = 0; k < 8; k++) *p[k] = egr_shim_ray.payload[k];
}

// ------------------------------------------------------------------------------------- C interface (oracle/reference.py)
extern "C" {

void *ref_create(int width, int height) { return new Ref(width, height); }
void ref_destroy(void *h) { delete (Ref *)h; }

// 20 doubles in the order of core/config.h
void ref_set_config(void *h, const double *c) {
    ConfigStore &s = ((Ref *)h)->cfg;
    s.exp_power = (float)c[0], s.alpha_threshold = (float)c[1], s.transmittance_threshold = (float)c[2];
    s.accumulate_samples = c[3] != 0, s.jitter_primary_rays = c[4] != 0, s.num_bounces = (int)c[5];
    s.global_scale_factor = (float)c[6];
    s.loss_weight_diffuse = (float)c[7], s.loss_weight_specular = (float)c[8], s.loss_weight_depth = (float)c[9];
    s.loss_weight_normal = (float)c[10], s.loss_weight_f0 = (float)c[11], s.loss_weight_roughness = (float)c[12];
    s.eps_forward_normalization = (float)c[13], s.eps_scale_grad = (float)c[14], s.eps_ray_surface_offset = (float)c[15];
    s.eps_min_roughness = (float)c[16], s.reflection_invalid_normal_threshold = (float)c[17];
    s.backfacing_invalid_normal_threshold = (float)c[18], s.backfacing_max_dist = (float)c[19];
}

// CameraDataHolder::set_pose: rotation_w2c is the transpose of rotation_c2w
void ref_set_camera(void *h, const float *origin, const float *c2w, float fov, float znear, float zfar) {
    Ref *r = (Ref *)h;
    r->origin = {origin[0], origin[1], origin[2]};
    for (int a = 0; a < 3; a++) r->c2w[a] = {c2w[3 * a], c2w[3 * a + 1], c2w[3 * a + 2]}, r->w2c[a] = {c2w[a], c2w[3 + a], c2w[6 + a]};
    r->fov = fov, r->znear = znear, r->zfar = zfar;
}

// the eight copy_ of the caller's parameter export; a new count resizes (and zeroes) the gradient tensors
void ref_set_gaussians(void *h, int n, const float *rgb, const float *normal, const float *f0, const float *roughness, const float *opacity,
                       const float *scale, const float *mean, const float *rotation) {
    Ref *r = (Ref *)h;
    const size_t N = (size_t)n;
    const bool resized = r->n != (uint32_t)n;
    r->n = (uint32_t)n;
    r->rgb.assign(rgb, rgb + 3 * N), r->normal.assign(normal, normal + 3 * N), r->f0.assign(f0, f0 + 3 * N), r->roughness.assign(roughness, roughness + N);
    r->opacity.assign(opacity, opacity + N), r->scale.assign(scale, scale + 3 * N), r->mean.assign(mean, mean + 3 * N), r->rotation.assign(rotation, rotation + 4 * N);
    if (resized) {
        r->d_rgb.assign(3 * N, 0.0f), r->d_normal.assign(3 * N, 0.0f), r->d_f0.assign(3 * N, 0.0f), r->d_roughness.assign(N, 0.0f), r->d_opacity.assign(N, 0.0f);
        r->d_scale.assign(3 * N, 0.0f), r->d_mean.assign(3 * N, 0.0f), r->d_rotation.assign(4 * N, 0.0f), r->total_weight.assign(N, 0.0f);
    }
}

void ref_set_targets(void *h, const float *diffuse, const float *specular, const float *depth, const float *normal, const float *f0, const float *roughness) {
    Ref *r = (Ref *)h;
    auto cp = [&](std::vector<float> &dst, const float *src) {
        if (src) dst.assign(src, src + dst.size());
        else std::fill(dst.begin(), dst.end(), 0.0f);
    };
    cp(r->tg_diffuse, diffuse), cp(r->tg_specular, specular), cp(r->tg_depth, depth), cp(r->tg_normal, normal), cp(r->tg_f0, f0), cp(r->tg_roughness, roughness);
}

void ref_update_bvh(void *h) { ((Ref *)h)->update_bvh(); }
void ref_reset_accumulators(void *h) { ((Ref *)h)->reset_accumulators(); }
void ref_set_reverse_traversal(void *h, int reverse) { ((Ref *)h)->reverse_traversal = reverse != 0; }
uint32_t ref_get_total_num_calls(void *h) { return ((Ref *)h)->total_num_calls; }
void ref_set_total_num_calls(void *h, uint32_t v) { ((Ref *)h)->total_num_calls = v; }
int ref_get_accumulated_sample_count(void *h) { return ((Ref *)h)->accumulated_sample_count; }

// the nine gradient tensors, side by side in the order of core/gaussians.h: read (dst) or written (src); null = zero them
void ref_gradients(void *h, int write, float **ptrs) {
    Ref *r = (Ref *)h;
    std::vector<float> *v[9] = {&r->d_rgb, &r->d_normal, &r->d_f0, &r->d_roughness, &r->d_opacity, &r->d_scale, &r->d_mean, &r->d_rotation, &r->total_weight};
    for (int k = 0; k < 9; k++) {
        if (!ptrs) std::fill(v[k]->begin(), v[k]->end(), 0.0f);
        else if (write) std::copy(ptrs[k], ptrs[k] + v[k]->size(), v[k]->begin());
        else std::copy(v[k]->begin(), v[k]->end(), ptrs[k]);
    }
}

// one launch; returns 0, or 1 when the lists could not be allocated
int ref_raytrace(void *h, int grads_enabled) { return ((Ref *)h)->launch(grads_enabled != 0); }

// framebuffer, metadata and stats as the launch left them: outs = the ten output tensors in the order of core/framebuffer.h (denoised left out)
void ref_read_outputs(void *h, float **outs, uint32_t *random_seeds, int *num_traversed, int *num_accumulated) {
    Ref *r = (Ref *)h;
    const std::vector<float> *v[10] = {&r->out_rgb, &r->out_depth, &r->out_normal, &r->out_f0, &r->out_roughness, &r->out_T, &r->out_Ttot, &r->out_ro, &r->out_rd, &r->out_final};
    for (int k = 0; k < 10; k++) std::copy(v[k]->begin(), v[k]->end(), outs[k]);
    std::copy(r->random_seeds.begin(), r->random_seeds.end(), random_seeds);
    std::copy(r->num_traversed.begin(), r->num_traversed.end(), num_traversed);
    std::copy(r->num_accumulated.begin(), r->num_accumulated.end(), num_accumulated);
}

// instance records of the last update_bvh: M[n][12] (the reference kernel's), Wm[n][12] (the driver's inverse; zeros where invisible), visible[n]
void ref_get_instances(void *h, float *M, float *Wm, int *visible) {
    Ref *r = (Ref *)h;
    for (size_t i = 0; i < r->instances.size(); i++) {
        std::copy(r->instances[i].transform, r->instances[i].transform + 12, M + 12 * i);
        std::memcpy(Wm + 12 * i, &r->inverse[3 * i], 12 * sizeof(float));
        visible[i] = (int)r->instances[i].visibilityMask;
    }
}

// ------------------------------------------------------------------------------------- the reference's small functions, one call per element
uint32_t ref_tea4(uint32_t a, uint32_t b) { return tea<4>(a, b); }
uint32_t ref_lcg(uint32_t *state) { return lcg(*state); }
float ref_rnd(uint32_t *state) { return rnd(*state); }

// Camera::compute_primary_ray_direction for pixel (ix, iy) of a width x height launch; *seed advances when jitter is on
void ref_primary_ray_direction(const float *c2w, float fov, int jitter, int ix, int iy, int width, int height, uint32_t *seed, float *dir) {
    float3 w2c[3];
    for (int a = 0; a < 3; a++) w2c[a] = {c2w[a], c2w[3 + a], c2w[6 + a]};
    Camera cam{};
    cam.vertical_fov_radians = &fov, cam.rotation_w2c = w2c;
    float3 d = cam.compute_primary_ray_direction(jitter != 0, make_uint3(ix, iy, 0), make_uint3(width, height, 1), *seed);
    dir[0] = d.x, dir[1] = d.y, dir[2] = d.z;
}

void ref_sample_cook_torrance(int count, const float *N, const float *V, const float *roughness, const float *u, float *L) {
    for (int i = 0; i < count; i++) {
        float3 l = sample_cook_torrance(make_float3(N[3 * i], N[3 * i + 1], N[3 * i + 2]), make_float3(V[3 * i], V[3 * i + 1], V[3 * i + 2]), roughness[i], make_float2(u[2 * i], u[2 * i + 1]));
        L[3 * i] = l.x, L[3 * i + 1] = l.y, L[3 * i + 2] = l.z;
    }
}
void ref_cook_torrance_weight(int count, const float *N, const float *V, const float *L, const float *roughness, const float *f0, float *w) {
    for (int i = 0; i < count; i++) {
        float3 r = cook_torrance_weight(make_float3(N[3 * i], N[3 * i + 1], N[3 * i + 2]), make_float3(V[3 * i], V[3 * i + 1], V[3 * i + 2]),
                                        make_float3(L[3 * i], L[3 * i + 1], L[3 * i + 2]), roughness[i], make_float3(f0[3 * i], f0[3 * i + 1], f0[3 * i + 2]));
        w[3 * i] = r.x, w[3 * i + 1] = r.y, w[3 * i + 2] = r.z;
    }
}
void ref_compute_scaling_factor(int count, const float *opacity, const float *alpha_threshold, const float *exp_power, float *out) {
    for (int i = 0; i < count; i++) out[i] = compute_scaling_factor(opacity[i], alpha_threshold[i], exp_power[i]);
}
void ref_eval_gaussian(int count, const float *local_hit, const float *exp_power, float *out) {
    for (int i = 0; i < count; i++) out[i] = eval_gaussian(make_float3(local_hit[3 * i], local_hit[3 * i + 1], local_hit[3 * i + 2]), exp_power[i]);
}
// which: 0 sigmoid, 1 relu, 2 clipped relu, 3 exp
void ref_activation(int which, int count, const float *x, float *y) {
    for (int i = 0; i < count; i++) y[i] = which == 0 ? sigmoid_act(x[i]) : which == 1 ? relu_act(x[i]) : which == 2 ? clipped_relu_act(x[i]) : exp_act(x[i]);
}
void ref_activation_backward(int which, int count, const float *dL_dy, const float *y, float *dL_dx) {
    for (int i = 0; i < count; i++)
        dL_dx[i] = which == 0 ? backward_sigmoid_act(dL_dy[i], y[i]) : which == 1 ? backward_relu_act(dL_dy[i], y[i])
                   : which == 2 ? backward_clipped_relu_act(dL_dy[i], y[i]) : backward_exp_act(dL_dy[i], y[i]);
}
void ref_normalize_act(int count, const float *x, float *y) {
    for (int i = 0; i < count; i++) {
        float4 r = normalize_act(make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]));
        y[4 * i] = r.x, y[4 * i + 1] = r.y, y[4 * i + 2] = r.z, y[4 * i + 3] = r.w;
    }
}
void ref_backward_normalize_act(int count, const float *dL_dy, const float *x, float *dL_dx) {
    for (int i = 0; i < count; i++) {
        float4 xi = make_float4(x[4 * i], x[4 * i + 1], x[4 * i + 2], x[4 * i + 3]);
        float4 r = backward_normalize_act(make_float4(dL_dy[4 * i], dL_dy[4 * i + 1], dL_dy[4 * i + 2], dL_dy[4 * i + 3]), xi, normalize_act(xi));
        dL_dx[4 * i] = r.x, dL_dx[4 * i + 1] = r.y, dL_dx[4 * i + 2] = r.z, dL_dx[4 * i + 3] = r.w;
    }
}

} // extern "C"
