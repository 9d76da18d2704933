// SPDX-License-Identifier: MIT
// Scene editing (include/egr_raytracer.h: egr_edit_select / egr_edit_apply): what the reference's EditableGaussianModel does on every dirty frame with
//   make_editable          scene/editable_gaussian_model.py:16-77    (one boolean mask per object: box / cylinder, property ranges, exclusions)
//   seven getter overrides scene/editable_gaussian_model.py:103-279  (a clone + a loop over the objects with torch.where / boolean index assignments each)
//   the eight export copies renderer/gaussian_raytracer.py:41-50
// - as a SELECT (one 32-bit membership mask per row) and ONE pass that reads the eight raw arrays, applies every object's edit in order and writes the
// tracer's eight native arrays.
//
// MI355X mapping: one lane per row, 256 threads per workgroup. The pass is row-local and memory bound (88 B in, 84 B out per row): neighbouring lanes read
// neighbouring 12- and 16-byte rows. The edit records (172 B each, at most 32) are staged in LDS once per workgroup; the loop over the objects is
// wave-uniform and a lane applies edit k iff bit k of its mask is set. Everything that depends on the edit alone (rotation matrix, quaternion, log(scale),
// pi * hue_shift, override^2, the object centre) arrives precomputed: there is no trigonometry here.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

namespace {

constexpr uint32_t EDIT_THREADS = 256;
constexpr uint32_t EDIT_MAX_ROWS = 1u << 26; // the tree's own limit
constexpr uint32_t EDIT_RECORD_WORDS = sizeof(egr_edit_record) / 4;
constexpr uint32_t EDIT_SEL_RANGES = EGR_EDIT_SEL_RANGE_F0 | EGR_EDIT_SEL_RANGE_ROUGHNESS | EGR_EDIT_SEL_RANGE_DIFFUSE;
constexpr float EDIT_TWO_PI = 6.283185307179586f, EDIT_SECTOR = 1.0471975511965976f; // 2 pi, pi / 3
static_assert(sizeof(egr_edit_object) == 68 && sizeof(egr_edit_colour) == 36 && sizeof(egr_edit_record) == 172 && sizeof(egr_edit_arrays) == 64, "ABI layout (c_abi.py mirrors it)");

struct SelectArgs {
    const float *xyz, *f0, *roughness, *diffuse;
    uint32_t *mask;
    uint32_t n, num_objects;
    egr_edit_object obj[EGR_MAX_EDIT_OBJECTS]; // 2176 B of kernel arguments: no upload, no device buffer
};

__device__ inline bool in_box(float x, float y, float z, const float *lo, const float *hi) {
    return x >= lo[0] && x <= hi[0] && y >= lo[1] && y <= hi[1] && z >= lo[2] && z <= hi[2];
}

__global__ void __launch_bounds__(EDIT_THREADS) k_edit_select(SelectArgs a) {
    const uint32_t row = blockIdx.x * EDIT_THREADS + threadIdx.x;
    if (row >= a.n) return;
    const float x = a.xyz[(size_t)row * 3], y = a.xyz[(size_t)row * 3 + 1], z = a.xyz[(size_t)row * 3 + 2];
    float mean[3] = {0.0f, 0.0f, 0.0f}; // f0, roughness, diffuse (a NULL array is never asked for: validated on the host)
    if (a.f0) mean[0] = (a.f0[(size_t)row * 3] + a.f0[(size_t)row * 3 + 1] + a.f0[(size_t)row * 3 + 2]) / 3.0f;
    if (a.roughness) mean[1] = a.roughness[row];
    if (a.diffuse) mean[2] = (a.diffuse[(size_t)row * 3] + a.diffuse[(size_t)row * 3 + 1] + a.diffuse[(size_t)row * 3 + 2]) / 3.0f;
    uint32_t shape = 0;
    for (uint32_t k = 0; k < a.num_objects; k++) { // (uniform: the objects are kernel arguments)
        const egr_edit_object &o = a.obj[k];
        bool in;
        if (o.flags & EGR_EDIT_SEL_EVERYTHING) {
            in = true;
        } else if (o.flags & EGR_EDIT_SEL_CYLINDER) {
            const float cx = 0.5f * (o.box_min[0] + o.box_max[0]), cy = 0.5f * (o.box_min[1] + o.box_max[1]);
            const float hx = 0.5f * (o.box_max[0] - o.box_min[0]), hy = 0.5f * (o.box_max[1] - o.box_min[1]);
            const float nx = (x - cx) / hx, ny = (y - cy) / hy;
            in = nx * nx + ny * ny <= 1.0f && z >= o.box_min[2] && z <= o.box_max[2];
        } else {
            in = in_box(x, y, z, o.box_min, o.box_max);
        }
        shape |= (in ? 1u : 0u) << k;
    }
    uint32_t m = 0;
    for (uint32_t k = 0; k < a.num_objects; k++) {
        const egr_edit_object &o = a.obj[k];
        bool sel = (shape >> k) & 1u;
        if (!(o.flags & EGR_EDIT_SEL_EVERYTHING)) {
            if (o.flags & EDIT_SEL_RANGES) {
                const bool exempt = (o.flags & EGR_EDIT_SEL_ZRANGE) && in_box(x, y, z, o.sub_min, o.box_max);
                if (!exempt) {
#pragma unroll
                    for (uint32_t j = 0; j < 3; j++)
                        if (o.flags & (EGR_EDIT_SEL_RANGE_F0 << j)) sel = sel && mean[j] >= o.range_lo[j] && mean[j] <= o.range_hi[j];
                }
            }
            if (shape & o.exclude) sel = false;
        }
        m |= (sel ? 1u : 0u) << k;
    }
    a.mask[row] = m;
}

struct ApplyArgs {
    egr_edit_arrays src, dst;
    const uint32_t *mask;
    const egr_edit_record *records;
    uint32_t n, num_records;
};

__device__ inline float edit_lerp(float a, float b, float w) { // torch.lerp's two branches
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * (1.0f - w);
}

__device__ inline void edit_colour(float &r, float &g, float &b, const egr_edit_colour &c) {
    r = edit_lerp(r, c.override_rgb[0], c.override_w), g = edit_lerp(g, c.override_rgb[1], c.override_w), b = edit_lerp(b, c.override_rgb[2], c.override_w);
    const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
    const float d = mx - mn;
    float s = d / (mx + 1e-8f), v = mx, h = 0.0f; // achromatic: hue 0
    if (d != 0.0f) {
        float h6 = r == mx ? (g - b) / d : (g == mx ? 2.0f + (b - r) / d : 4.0f + (r - g) / d); // the first channel that attains the max
        if (h6 < 0.0f) h6 += 6.0f;
        h = h6 * EDIT_SECTOR;
    }
    h += c.hue;
    h -= EDIT_TWO_PI * floorf(h / EDIT_TWO_PI);
    if (h < 0.0f) h += EDIT_TWO_PI;
    if (h >= EDIT_TWO_PI) h -= EDIT_TWO_PI;
    s = fminf(fmaxf(c.s_mult * (s + c.s_shift), 0.0f), 1.0f);
    v = fmaxf(c.v_mult * (v + c.v_shift), 0.0f);
    const float h6 = h / EDIT_SECTOR, fl = floorf(h6), f = h6 - fl;
    int hi = (int)fl;
    if (hi >= 6) hi -= 6; // h / (pi / 3) may round up to 6
    const float p = v * (1.0f - s), q = v * (1.0f - f * s), t = v * (1.0f - (1.0f - f) * s);
    switch (hi) {
    case 0: r = v, g = t, b = p; break;
    case 1: r = q, g = v, b = p; break;
    case 2: r = p, g = v, b = t; break;
    case 3: r = p, g = q, b = v; break;
    case 4: r = t, g = p, b = v; break;
    default: r = v, g = p, b = q; break;
    }
}

__device__ inline void edit_rotate(float &x, float &y, float &z, const float *R) {
    const float a = R[0] * x + R[1] * y + R[2] * z, b = R[3] * x + R[4] * y + R[5] * z, c = R[6] * x + R[7] * y + R[8] * z;
    x = a, y = b, z = c;
}

// dst may be src (row-local: a lane has read its whole row before it writes it), so no pointer here is __restrict__
__global__ void __launch_bounds__(EDIT_THREADS) k_edit_apply(ApplyArgs a) {
    __shared__ egr_edit_record s_rec[EGR_MAX_EDIT_OBJECTS]; // 5.4 KB
    {
        uint32_t *s = (uint32_t *)s_rec;
        const uint32_t *g = (const uint32_t *)a.records;
        for (uint32_t i = threadIdx.x; i < a.num_records * EDIT_RECORD_WORDS; i += EDIT_THREADS) s[i] = g[i]; // num_records <= 32: validated on the host
    }
    __syncthreads();
    const uint32_t row = blockIdx.x * EDIT_THREADS + threadIdx.x;
    if (row >= a.n) return; // (after the only barrier)
    const size_t r3 = (size_t)row * 3, r4 = (size_t)row * 4;
    float sx = a.src.scale[r3], sy = a.src.scale[r3 + 1], sz = a.src.scale[r3 + 2];
    float qw = a.src.rotation[r4], qx = a.src.rotation[r4 + 1], qy = a.src.rotation[r4 + 2], qz = a.src.rotation[r4 + 3];
    float px = a.src.mean[r3], py = a.src.mean[r3 + 1], pz = a.src.mean[r3 + 2];
    float opacity = a.src.opacity[row];
    float cr = a.src.rgb[r3], cg = a.src.rgb[r3 + 1], cb = a.src.rgb[r3 + 2];
    float nx = a.src.normal[r3], ny = a.src.normal[r3 + 1], nz = a.src.normal[r3 + 2];
    float rough = a.src.roughness[row];
    float fr = a.src.f0[r3], fg = a.src.f0[r3 + 1], fb = a.src.f0[r3 + 2];
    uint32_t m = a.num_records ? a.mask[row] : 0u;
    if (a.num_records < 32u) m &= (1u << a.num_records) - 1u;
    for (uint32_t k = 0; k < a.num_records; k++) { // wave-uniform trip count; in object order, each edit on the result of the one before
        if (!((m >> k) & 1u)) continue;
        const egr_edit_record &e = s_rec[k];
        const uint32_t flags = e.flags;
        if (flags & EGR_EDIT_ROUGHNESS) {
            const float base = (flags & EGR_EDIT_ROUGHNESS_OVERRIDE) ? e.roughness_base : rough;
            rough = fminf(fmaxf(e.roughness_mult * (base + e.roughness_shift), 0.0f), 1.0f);
        }
        if (flags & EGR_EDIT_DIFFUSE) edit_colour(cr, cg, cb, e.diffuse);
        if (flags & EGR_EDIT_F0) edit_colour(fr, fg, fb, e.f0);
        if (flags & EGR_EDIT_TRANSFORM) {
            px += e.translate[0], py += e.translate[1], pz += e.translate[2];
            px = (px - e.centre[0]) * e.scale + e.centre[0], py = (py - e.centre[1]) * e.scale + e.centre[1], pz = (pz - e.centre[2]) * e.scale + e.centre[2];
            float dx = px - e.centre[0], dy = py - e.centre[1], dz = pz - e.centre[2];
            edit_rotate(dx, dy, dz, e.R);
            px = dx + e.centre[0], py = dy + e.centre[1], pz = dz + e.centre[2];
            edit_rotate(nx, ny, nz, e.R);
            sx += e.log_scale, sy += e.log_scale, sz += e.log_scale;
            const float len = sqrtf(qw * qw + qx * qx + qy * qy + qz * qz);
            const float w = qw / len, x = qx / len, y = qy / len, z = qz / len;
            qw = e.q[0] * w - e.q[1] * x - e.q[2] * y - e.q[3] * z;
            qx = e.q[0] * x + e.q[1] * w + e.q[2] * z - e.q[3] * y;
            qy = e.q[0] * y - e.q[1] * z + e.q[2] * w + e.q[3] * x;
            qz = e.q[0] * z + e.q[1] * y - e.q[2] * x + e.q[3] * w;
        }
        if (flags & EGR_EDIT_REMOVED) opacity = -1e8f;
    }
    a.dst.scale[r3] = sx, a.dst.scale[r3 + 1] = sy, a.dst.scale[r3 + 2] = sz;
    a.dst.rotation[r4] = qw, a.dst.rotation[r4 + 1] = qx, a.dst.rotation[r4 + 2] = qy, a.dst.rotation[r4 + 3] = qz;
    a.dst.mean[r3] = px, a.dst.mean[r3 + 1] = py, a.dst.mean[r3 + 2] = pz;
    a.dst.opacity[row] = opacity;
    a.dst.rgb[r3] = cr, a.dst.rgb[r3 + 1] = cg, a.dst.rgb[r3 + 2] = cb;
    a.dst.normal[r3] = nx, a.dst.normal[r3 + 1] = ny, a.dst.normal[r3 + 2] = nz;
    a.dst.roughness[row] = rough;
    a.dst.f0[r3] = fr, a.dst.f0[r3 + 1] = fg, a.dst.f0[r3 + 2] = fb;
}

thread_local std::string g_edit_error;

constexpr int EDIT_ARRAYS = 8;
constexpr uint32_t EDIT_WIDTH[EDIT_ARRAYS] = {3, 4, 3, 1, 3, 3, 1, 3}; // egr_edit_arrays, in field order

} // namespace

extern "C" const char *egr_edit_last_error(void) { return g_edit_error.c_str(); }

extern "C" int egr_edit_select(int device, uint32_t n, const float *xyz, const float *f0, const float *roughness, const float *diffuse,
                               const egr_edit_object *objects, uint32_t num_objects, uint32_t *mask, void *hip_stream) {
    const char *fn = "egr_edit_select";
    // ---- validation: before any HIP call
    if (!mask) return egr_fail(g_edit_error, fn, "mask is a required output");
    if (num_objects > EGR_MAX_EDIT_OBJECTS) return egr_fail(g_edit_error, fn, "more than EGR_MAX_EDIT_OBJECTS (32) objects");
    if (num_objects != 0 && !objects) return egr_fail(g_edit_error, fn, "num_objects > 0 needs objects");
    if (n > EDIT_MAX_ROWS) return egr_fail(g_edit_error, fn, "n exceeds 2^26 rows (the limit of the tree)");
    if (n != 0 && !xyz) return egr_fail(g_edit_error, fn, "xyz is required");
    SelectArgs a{};
    for (uint32_t k = 0; k < num_objects; k++) {
        const uint32_t f = objects[k].flags;
        if (((f & EGR_EDIT_SEL_RANGE_F0) && !f0) || ((f & EGR_EDIT_SEL_RANGE_ROUGHNESS) && !roughness) || ((f & EGR_EDIT_SEL_RANGE_DIFFUSE) && !diffuse))
            return egr_fail(g_edit_error, fn, "an object has a property range whose array is NULL");
        if (num_objects < 32u && (objects[k].exclude >> num_objects)) return egr_fail(g_edit_error, fn, "an object excludes an object that does not exist");
        a.obj[k] = objects[k];
    }
    if (n == 0) return 0;
    const EgrRange out = {mask, (uint64_t)n * 4}, in[4] = {{xyz, (uint64_t)n * 12}, {f0, (uint64_t)n * 12}, {roughness, (uint64_t)n * 4}, {diffuse, (uint64_t)n * 12}};
    if (egr_find_clash(&out, 1, in, 4)) return egr_fail(g_edit_error, fn, "mask overlaps an input");
    a.xyz = xyz, a.f0 = f0, a.roughness = roughness, a.diffuse = diffuse, a.mask = mask, a.n = n, a.num_objects = num_objects;
    return egr_on_device(device, g_edit_error, fn, [&] { egr_launch(k_edit_select, dim3((n + EDIT_THREADS - 1) / EDIT_THREADS), dim3(EDIT_THREADS), (hipStream_t)hip_stream, a); });
}

extern "C" int egr_edit_apply(int device, uint32_t n, const egr_edit_arrays *src, const egr_edit_arrays *dst, const uint32_t *mask,
                              const egr_edit_record *records, uint32_t num_records, void *hip_stream) {
    const char *fn = "egr_edit_apply";
    // ---- validation: before any HIP call
    if (!src || !dst) return egr_fail(g_edit_error, fn, "src and dst are required");
    if (num_records > EGR_MAX_EDIT_OBJECTS) return egr_fail(g_edit_error, fn, "more than EGR_MAX_EDIT_OBJECTS (32) records");
    if (n > EDIT_MAX_ROWS) return egr_fail(g_edit_error, fn, "n exceeds 2^26 rows (the limit of the tree)");
    if (num_records != 0 && (!mask || !records)) return egr_fail(g_edit_error, fn, "num_records > 0 needs mask and records");
    float *const *s = &src->scale, *const *d = &dst->scale; // eight float * fields in a row (static_assert above: 64 bytes)
    for (int k = 0; k < EDIT_ARRAYS; k++)
        if (!s[k] || !d[k]) return egr_fail(g_edit_error, fn, "a NULL array in src or dst");
    if (n == 0) return 0;
    // in place is allowed here (dst[k] == src[k] exactly), so the pairs are walked by hand: egr_find_clash knows out-of-place launches only
    const EgrRange m = {num_records ? mask : nullptr, (uint64_t)n * 4}, r = {records, (uint64_t)num_records * sizeof(egr_edit_record)};
    for (int k = 0; k < EDIT_ARRAYS; k++) {
        const EgrRange dk = {d[k], (uint64_t)n * EDIT_WIDTH[k] * 4};
        for (int j = 0; j < EDIT_ARRAYS; j++) {
            const uint64_t jbytes = (uint64_t)n * EDIT_WIDTH[j] * 4;
            if (!(j == k && s[j] == d[k]) && egr_overlap(dk, EgrRange{s[j], jbytes}))
                return egr_fail(g_edit_error, fn, "partial overlap: a dst array must be its own src array or touch no src array");
            if (j != k && egr_overlap(dk, EgrRange{d[j], jbytes})) return egr_fail(g_edit_error, fn, "partial overlap: two dst arrays overlap");
        }
        if (egr_overlap(dk, m) || egr_overlap(dk, r)) return egr_fail(g_edit_error, fn, "partial overlap: a dst array overlaps the mask or the records");
    }
    ApplyArgs a{};
    a.src = *src, a.dst = *dst, a.mask = mask, a.records = records, a.n = n, a.num_records = num_records;
    return egr_on_device(device, g_edit_error, fn, [&] { egr_launch(k_edit_apply, dim3((n + EDIT_THREADS - 1) / EDIT_THREADS), dim3(EDIT_THREADS), (hipStream_t)hip_stream, a); });
}
