// SPDX-License-Identifier: MIT
// distCUDA2 replacement: for every point the MEAN of the squared distances to its 3 nearest neighbours.
//
// The reference calls `simple_knn._C.distCUDA2(points)` (editable_gauss_refl/scene/gaussian_model.py:17,197-201,246-250) to
// initialise the Gaussian scales. simple-knn is an un-vendored submodule (graphdeco-inria/simple-knn, empty directory in the
// reference tree), so this file restates its published algorithm rather than any source: Morton-sort the points, cut the
// sorted sequence into boxes of 1024 points with their bounds, seed the 3 best distances of a point from its 3 + 3 neighbours
// in Morton order, then visit every box whose distance to the point is below the current 3rd-best and scan it. The result is
// the EXACT 3-NN mean (the box test only prunes), which is what tests/test_knn.py checks against brute force.
//
// MI355X mapping: one lane per (Morton-sorted) point, so the 64 points of a wave are spatial neighbours and prune / scan the
// same boxes; box bounds are wave-uniform (scalar loads), box scans read consecutive float4s (coalesced broadcast).
#include <hip/hip_runtime.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

namespace {

constexpr int KNN_BOX = 1024; // points per box (simple-knn's BOX_SIZE)
constexpr int BS = 256;

__device__ __forceinline__ uint32_t ordered(float f) {
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) {
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    return __uint_as_float(u);
}

__global__ void __launch_bounds__(BS) k_knn_bounds(uint32_t n, const float *__restrict__ p, uint32_t *__restrict__ b) {
    __shared__ uint32_t s[6];
    if (threadIdx.x < 3) s[threadIdx.x] = 0xFFFFFFFFu, s[3 + threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t i = blockIdx.x * BS + threadIdx.x; i < n; i += gridDim.x * BS)
        for (int a = 0; a < 3; a++) {
            const float v = p[3 * (size_t)i + a];
            if (v == v) atomicMin(&s[a], ordered(v)), atomicMax(&s[3 + a], ordered(v));
        }
    __syncthreads();
    if (threadIdx.x < 3) atomicMin(&b[threadIdx.x], s[threadIdx.x]), atomicMax(&b[3 + threadIdx.x], s[3 + threadIdx.x]);
}

__device__ __forceinline__ uint64_t spread21(uint32_t v) {
    uint64_t x = v & 0x1FFFFFu;
    x = (x | (x << 32)) & 0x1F00000000FFFFull;
    x = (x | (x << 16)) & 0x1F0000FF0000FFull;
    x = (x | (x << 8)) & 0x100F00F00F00F00Full;
    x = (x | (x << 4)) & 0x10C30C30C30C30C3ull;
    x = (x | (x << 2)) & 0x1249249249249249ull;
    return x;
}
__global__ void __launch_bounds__(BS) k_knn_codes(uint32_t n, const float *__restrict__ p, const uint32_t *__restrict__ b, uint64_t *__restrict__ keys,
                                                  uint32_t *__restrict__ vals) {
    const uint32_t i = blockIdx.x * BS + threadIdx.x;
    if (i >= n) return;
    uint64_t key = 0;
    for (int a = 0; a < 3; a++) {
        const float lo = unordered(b[a]), hi = unordered(b[3 + a]);
        const float v = p[3 * (size_t)i + a];
        const float u = (v == v && hi > lo) ? (v - lo) / (hi - lo) : 0.0f;
        const uint32_t q = (uint32_t)fminf(fmaxf(u * 2097152.0f, 0.0f), 2097151.0f);
        key |= spread21(q) << (2 - a);
    }
    keys[i] = key;
    vals[i] = i;
}
__global__ void __launch_bounds__(BS) k_knn_gather(uint32_t n, const float *__restrict__ p, const uint32_t *__restrict__ order, float4 *__restrict__ sp) {
    const uint32_t i = blockIdx.x * BS + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = order[i];
    sp[i] = make_float4(p[3 * (size_t)g], p[3 * (size_t)g + 1], p[3 * (size_t)g + 2], __uint_as_float(g));
}
// one workgroup per box of KNN_BOX consecutive sorted points
__global__ void __launch_bounds__(BS) k_knn_boxes(uint32_t n, const float4 *__restrict__ sp, float *__restrict__ boxes) {
    __shared__ float lo[3][BS], hi[3][BS];
    const uint32_t beg = blockIdx.x * KNN_BOX, end = min(n, beg + KNN_BOX);
    float l[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, h[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (uint32_t i = beg + threadIdx.x; i < end; i += BS) {
        const float4 q = sp[i];
        l[0] = fminf(l[0], q.x), l[1] = fminf(l[1], q.y), l[2] = fminf(l[2], q.z);
        h[0] = fmaxf(h[0], q.x), h[1] = fmaxf(h[1], q.y), h[2] = fmaxf(h[2], q.z);
    }
    for (int a = 0; a < 3; a++) lo[a][threadIdx.x] = l[a], hi[a][threadIdx.x] = h[a];
    __syncthreads();
    for (int s = BS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int a = 0; a < 3; a++) {
                lo[a][threadIdx.x] = fminf(lo[a][threadIdx.x], lo[a][threadIdx.x + s]);
                hi[a][threadIdx.x] = fmaxf(hi[a][threadIdx.x], hi[a][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 3) boxes[6 * (size_t)blockIdx.x + threadIdx.x] = lo[threadIdx.x][0], boxes[6 * (size_t)blockIdx.x + 3 + threadIdx.x] = hi[threadIdx.x][0];
}

__device__ __forceinline__ void keep3(float d, float best[3]) { // best[0] <= best[1] <= best[2]
    if (d < best[2]) {
        best[2] = d;
        if (best[2] < best[1]) { const float t = best[1]; best[1] = best[2], best[2] = t; }
        if (best[1] < best[0]) { const float t = best[0]; best[0] = best[1], best[1] = t; }
    }
}
__device__ __forceinline__ float dist2(const float4 &a, const float4 &b) {
    const float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return dx * dx + dy * dy + dz * dz;
}
__global__ void __launch_bounds__(64) k_knn_search(uint32_t n, uint32_t nboxes, const float4 *__restrict__ sp, const float *__restrict__ boxes,
                                                   float *__restrict__ out) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const float4 me = live ? sp[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    float best[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
    if (live)
        for (int d = -3; d <= 3; d++) { // seed from the neighbours in Morton order
            const int64_t j = (int64_t)i + d;
            if (d == 0 || j < 0 || j >= (int64_t)n) continue;
            keep3(dist2(me, sp[j]), best);
        }
    // the seed only yields a rejection radius (an upper bound of the 3rd-nearest distance); the boxes then rebuild the best three
    // from scratch, otherwise the Morton neighbours would be counted twice
    const float reject = best[2];
    best[0] = best[1] = best[2] = FLT_MAX;
    for (uint32_t b = 0; b < nboxes; b++) { // wave-uniform loop: box bounds come through the scalar cache
        const float *bx = boxes + 6 * (size_t)b;
        const float ex = fmaxf(fmaxf(bx[0] - me.x, me.x - bx[3]), 0.0f), ey = fmaxf(fmaxf(bx[1] - me.y, me.y - bx[4]), 0.0f),
                    ez = fmaxf(fmaxf(bx[2] - me.z, me.z - bx[5]), 0.0f);
        const float bd = ex * ex + ey * ey + ez * ez;
        const bool want = live && bd <= reject && bd <= best[2];
        if (__ballot(want) == 0ull) continue;
        const uint32_t beg = b * KNN_BOX, end = min(n, beg + KNN_BOX);
        if (want)
            for (uint32_t j = beg; j < end; j++) {
                if (j == i) continue;
                keep3(dist2(me, sp[j]), best);
            }
    }
    if (live) {
        // n <= 3: fewer than 3 neighbours exist - average the ones that do (simple-knn assumes n >= 4)
        float sum = 0.0f;
        int cnt = 0;
        for (int k = 0; k < 3; k++)
            if (best[k] < FLT_MAX) sum += best[k], cnt++;
        out[__float_as_uint(me.w)] = cnt ? sum / (float)cnt : 0.0f;
    }
}

thread_local std::string g_knn_error;

struct DeviceTemp { // a hipMalloc that ends with its block
    void *p = nullptr;
    ~DeviceTemp() {
        if (p) (void)hipFree(p);
    }
};

} // namespace

extern "C" const char *egr_knn_last_error(void) { return g_knn_error.c_str(); }

extern "C" int egr_knn_mean_dist2(int device, const float *points_xyz, uint32_t n, float *out_mean_dist2, void *hip_stream) {
    const char *fn = "egr_knn_mean_dist2";
    // ---- validation: before any HIP call
    if (n == 0) return 0;
    if (!points_xyz || !out_mean_dist2) return egr_fail(g_knn_error, fn, "null pointer: invalid argument");
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_knn_error, fn, [&] {
        DeviceTemp tmp, sort_tmp; // freed on every way out
        const uint32_t nboxes = (n + KNN_BOX - 1) / KNN_BOX;
        // one allocation: bounds[8] | keys_in | keys_out | vals_in | vals_out | sorted float4 | boxes
        auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_b = 0, o_ki = al(32), o_ko = o_ki + al(8 * (size_t)n), o_vi = o_ko + al(8 * (size_t)n), o_vo = o_vi + al(4 * (size_t)n),
                     o_sp = o_vo + al(4 * (size_t)n), o_bx = o_sp + al(16 * (size_t)n), total = o_bx + al(24 * (size_t)nboxes);
        EGR_HIP(hipMalloc(&tmp.p, total));
        char *base = (char *)tmp.p;
        uint32_t *bounds = (uint32_t *)(base + o_b);
        uint64_t *ki = (uint64_t *)(base + o_ki), *ko = (uint64_t *)(base + o_ko);
        uint32_t *vi = (uint32_t *)(base + o_vi), *vo = (uint32_t *)(base + o_vo);
        float4 *sp = (float4 *)(base + o_sp);
        float *boxes = (float *)(base + o_bx);
        const uint32_t init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
        EGR_HIP(hipMemcpyAsync(bounds, init, sizeof(init), hipMemcpyHostToDevice, s));
        const uint32_t blocks = (n + BS - 1) / BS;
        egr_launch(k_knn_bounds, dim3(std::min(blocks, 2048u)), dim3(BS), s, n, points_xyz, bounds);
        egr_launch(k_knn_codes, dim3(blocks), dim3(BS), s, n, points_xyz, bounds, ki, vi);
        size_t bytes = 0;
        EGR_HIP(rocprim::radix_sort_pairs(nullptr, bytes, ki, ko, vi, vo, (size_t)n, 0, 63, s));
        EGR_HIP(hipMalloc(&sort_tmp.p, std::max<size_t>(bytes, 16)));
        EGR_HIP(rocprim::radix_sort_pairs(sort_tmp.p, bytes, ki, ko, vi, vo, (size_t)n, 0, 63, s));
        egr_launch(k_knn_gather, dim3(blocks), dim3(BS), s, n, points_xyz, vo, sp);
        egr_launch(k_knn_boxes, dim3(nboxes), dim3(BS), s, n, sp, boxes);
        egr_launch(k_knn_search, dim3((n + 63) / 64), dim3(64), s, n, nboxes, sp, boxes, out_mean_dist2);
        EGR_HIP(hipStreamSynchronize(s)); // the temporaries are freed on the way out
    });
}
