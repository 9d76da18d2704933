// SPDX-License-Identifier: MIT
// Fused prune (include/egr_raytracer.h: egr_prune_select / egr_prune_gather): what the reference does at every pruning interval with
// boolean indexing -
//   the weight test      train.py:238-245                                   (total_weight / interval < min_weight)
//   the camera spheres   scene/scene.py:88-105                              (|p - T| < znear, one kernel chain per training camera)
//   the compaction       scene/gaussian_model.py:478-531 prune_points        (8 parameters + 16 Adam moments, one nonzero + index pair each)
// - as a SELECT (criteria + stable scan -> ascending list of surviving rows + their count) and ONE out-of-place GATHER over all arrays.
//
// Select is three launches in stream order, and the stream order is the ONLY dependency between workgroups (no look-back, no flags, no tickets:
// nothing ever waits for another workgroup):
//   k_prune_flag     one workgroup per EGR_PRUNE_ROWS_PER_WG rows: evaluates the criteria, stores the 64-bit keep ballot of every wave segment and
//                    the workgroup's kept-row count
//   k_prune_scan     ONE workgroup: exclusive scan of the workgroup counts in passes of PRUNE_SCAN_THREADS counts with a running carry; writes `count`
//   k_prune_scatter  one workgroup per EGR_PRUNE_ROWS_PER_WG rows: rank of a kept row = workgroup offset + kept rows of the earlier segments + mbcnt
//                    of the ballot below its lane; writes the row number there (ascending by construction: the result is `tensor[keep]`)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

namespace {

constexpr uint32_t PRUNE_THREADS = 256;                                      // 4 waves
constexpr uint32_t PRUNE_ROWS_PER_THREAD = EGR_PRUNE_ROWS_PER_WG / PRUNE_THREADS; // 4: a wave covers 64 CONSECUTIVE rows per iteration (one ballot = one segment)
constexpr uint32_t PRUNE_SEGMENTS = EGR_PRUNE_ROWS_PER_WG / 64;              // 16 ballots per workgroup
constexpr uint32_t PRUNE_CAM_CHUNK = 256;                                    // cameras staged in LDS at a time (4 KB)
constexpr uint32_t PRUNE_SCAN_THREADS = 1024;                                // workgroup counts per pass of k_prune_scan
constexpr uint32_t PRUNE_MAX_ROWS = 1u << 26;                                // the tree's own limit
static_assert(EGR_PRUNE_ROWS_PER_WG == 1024 && PRUNE_ROWS_PER_THREAD * PRUNE_THREADS == EGR_PRUNE_ROWS_PER_WG, "EGR_PRUNE_WORKSPACE_BYTES assumes 16 ballots + 1 count per 1024 rows");

struct SelectArgs {
    const float *total_weight; // [n] or NULL
    const float *points;       // [n][3] or NULL
    const float *cam_centers;  // [num_cams][3]
    const float *cam_znear;    // [num_cams]
    const uint8_t *remove_mask; // [n] or NULL
    uint64_t *ballots;         // [num_wg * PRUNE_SEGMENTS] keep ballots
    uint32_t *wg_counts;       // [num_wg] kept rows per workgroup; after k_prune_scan: their exclusive prefix
    uint32_t *src_index;       // [n]
    uint32_t *count;           // [1]
    float divisor, min_weight;
    uint32_t n, num_cams, num_wg;
};

__global__ void __launch_bounds__(PRUNE_THREADS) k_prune_flag(SelectArgs a) {
    __shared__ float4 s_cam[PRUNE_CAM_CHUNK];
    __shared__ uint32_t s_wave_kept[PRUNE_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t base = blockIdx.x * EGR_PRUNE_ROWS_PER_WG;
    bool remove[PRUNE_ROWS_PER_THREAD];
    float px[PRUNE_ROWS_PER_THREAD], py[PRUNE_ROWS_PER_THREAD], pz[PRUNE_ROWS_PER_THREAD];
    const bool cams = a.points != nullptr && a.num_cams != 0;
#pragma unroll
    for (uint32_t it = 0; it < PRUNE_ROWS_PER_THREAD; it++) {
        const uint32_t row = base + it * PRUNE_THREADS + tid;
        const bool in = row < a.n;
        bool r = false;
        if (in && a.total_weight) r = __fdiv_rn(a.total_weight[row], a.divisor) < a.min_weight; // IEEE division, strict: NaN and +inf are kept
        if (in && a.remove_mask) r = r || a.remove_mask[row] != 0;
        remove[it] = r;
        px[it] = py[it] = pz[it] = 0.0f;
        if (in && cams) px[it] = a.points[(size_t)row * 3], py[it] = a.points[(size_t)row * 3 + 1], pz[it] = a.points[(size_t)row * 3 + 2];
    }
    if (cams) {
        for (uint32_t c0 = 0; c0 < a.num_cams; c0 += PRUNE_CAM_CHUNK) { // (uniform trip count: every thread reaches both barriers)
            const uint32_t chunk = min(PRUNE_CAM_CHUNK, a.num_cams - c0);
            __syncthreads();
            if (tid < chunk) s_cam[tid] = make_float4(a.cam_centers[(size_t)(c0 + tid) * 3], a.cam_centers[(size_t)(c0 + tid) * 3 + 1], a.cam_centers[(size_t)(c0 + tid) * 3 + 2], a.cam_znear[c0 + tid]);
            __syncthreads();
            for (uint32_t c = 0; c < chunk; c++) {
                const float4 cam = s_cam[c];
#pragma unroll
                for (uint32_t it = 0; it < PRUNE_ROWS_PER_THREAD; it++) {
                    const float dx = px[it] - cam.x, dy = py[it] - cam.y, dz = pz[it] - cam.z;
                    remove[it] = remove[it] || __fsqrt_rn(dx * dx + dy * dy + dz * dz) < cam.w; // strict: znear 0 removes nothing, a point AT the centre goes when znear > 0
                }
            }
        }
    }
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t it = 0; it < PRUNE_ROWS_PER_THREAD; it++) {
        const uint32_t row = base + it * PRUNE_THREADS + tid;
        const uint64_t ballot = __ballot(row < a.n && !remove[it]);
        if (lane == 0) a.ballots[(size_t)blockIdx.x * PRUNE_SEGMENTS + it * (PRUNE_THREADS / 64) + wave] = ballot;
        kept += (uint32_t)__popcll(ballot); // wave-uniform
    }
    if (lane == 0) s_wave_kept[wave] = kept;
    __syncthreads();
    if (tid == 0) a.wg_counts[blockIdx.x] = s_wave_kept[0] + s_wave_kept[1] + s_wave_kept[2] + s_wave_kept[3];
}

// ONE workgroup. Pass p scans counts [p * 1024, (p + 1) * 1024) in place (exclusive, plus the carry of the earlier passes).
__global__ void __launch_bounds__(PRUNE_SCAN_THREADS) k_prune_scan(SelectArgs a) {
    __shared__ uint32_t s_wave_sum[PRUNE_SCAN_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t p0 = 0; p0 < a.num_wg; p0 += PRUNE_SCAN_THREADS) { // (uniform trip count)
        const uint32_t i = p0 + tid;
        const uint32_t v = i < a.num_wg ? a.wg_counts[i] : 0u;
        uint32_t incl = v; // inclusive scan within the wave
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        __syncthreads(); // the previous pass has read s_wave_sum
        if (lane == 63) s_wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < PRUNE_SCAN_THREADS / 64; w++) {
            const uint32_t s = s_wave_sum[w];
            before += w < wave ? s : 0u;
            total += s;
        }
        if (i < a.num_wg) a.wg_counts[i] = carry + before + incl - v;
        carry += total;
    }
    if (tid == 0) a.count[0] = carry;
}

__global__ void __launch_bounds__(PRUNE_THREADS) k_prune_scatter(SelectArgs a) {
    __shared__ uint32_t s_seg_kept[PRUNE_SEGMENTS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t *ballots = a.ballots + (size_t)blockIdx.x * PRUNE_SEGMENTS;
    if (tid < PRUNE_SEGMENTS) s_seg_kept[tid] = (uint32_t)__popcll(ballots[tid]);
    __syncthreads();
    const uint32_t wg_offset = a.wg_counts[blockIdx.x];
#pragma unroll
    for (uint32_t it = 0; it < PRUNE_ROWS_PER_THREAD; it++) {
        const uint32_t seg = it * (PRUNE_THREADS / 64) + wave;
        uint32_t before = 0;
#pragma unroll
        for (uint32_t s = 0; s < PRUNE_SEGMENTS; s++) before += s < seg ? s_seg_kept[s] : 0u;
        const uint64_t ballot = ballots[seg];
        if ((ballot >> lane) & 1ull) { // (only rows < n are ever set)
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u));
            a.src_index[wg_offset + before + rank] = blockIdx.x * EGR_PRUNE_ROWS_PER_WG + seg * 64u + lane; // < count <= n
        }
    }
}

struct GatherArgs {
    egr_prune_array t[EGR_MAX_PRUNE_ARRAYS];
    const uint32_t *src_index;
    uint32_t count;
};

__global__ void __launch_bounds__(256) k_prune_gather(GatherArgs a) {
    const egr_prune_array &T = a.t[blockIdx.y];
    const uint32_t *src = (const uint32_t *)T.src;
    uint32_t *dst = (uint32_t *)T.dst;
    const size_t total = (size_t)a.count * T.width;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / T.width, c = i - r * T.width;
        dst[i] = src[(size_t)a.src_index[r] * T.width + c]; // 4-byte words moved as bits
    }
}

thread_local std::string g_prune_error;

} // namespace

extern "C" const char *egr_prune_last_error(void) { return g_prune_error.c_str(); }

extern "C" int egr_prune_select(int device, uint32_t n, const float *total_weight, float divisor, float min_weight, const float *points,
                                const float *cam_centers, const float *cam_znear, uint32_t num_cams, const uint8_t *remove_mask, uint32_t *src_index,
                                uint32_t *count, void *workspace, void *hip_stream) {
    const char *fn = "egr_prune_select";
    // ---- validation: before any HIP call
    if (!src_index || !count) return egr_fail(g_prune_error, fn, "src_index and count are required outputs");
    if (n > PRUNE_MAX_ROWS) return egr_fail(g_prune_error, fn, "n exceeds 2^26 rows (the limit of the tree)");
    if (points && num_cams != 0 && (!cam_centers || !cam_znear)) return egr_fail(g_prune_error, fn, "num_cams > 0 needs cam_centers and cam_znear");
    if (n == 0) return 0;
    if (!workspace || ((uintptr_t)workspace & 7u)) return egr_fail(g_prune_error, fn, "an 8-byte aligned workspace of EGR_PRUNE_WORKSPACE_BYTES(n) is required");
    SelectArgs a{};
    a.num_wg = (n + EGR_PRUNE_ROWS_PER_WG - 1) / EGR_PRUNE_ROWS_PER_WG;
    a.total_weight = total_weight, a.points = points, a.cam_centers = cam_centers, a.cam_znear = cam_znear, a.remove_mask = remove_mask;
    a.ballots = (uint64_t *)workspace, a.wg_counts = (uint32_t *)(a.ballots + (size_t)a.num_wg * PRUNE_SEGMENTS);
    a.src_index = src_index, a.count = count;
    a.divisor = divisor, a.min_weight = min_weight;
    a.n = n, a.num_cams = points ? num_cams : 0u;
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_prune_error, fn, [&] {
        egr_launch(k_prune_flag, dim3(a.num_wg), dim3(PRUNE_THREADS), s, a);
        egr_launch(k_prune_scan, dim3(1), dim3(PRUNE_SCAN_THREADS), s, a);
        egr_launch(k_prune_scatter, dim3(a.num_wg), dim3(PRUNE_THREADS), s, a);
    });
}

extern "C" int egr_prune_gather(int device, const egr_prune_array *arrays, int num_arrays, uint32_t n, const uint32_t *src_index, uint32_t count,
                                void *hip_stream) {
    const char *fn = "egr_prune_gather";
    // ---- validation: before any HIP call
    if (!arrays || num_arrays < 1 || num_arrays > EGR_MAX_PRUNE_ARRAYS) return egr_fail(g_prune_error, fn, "1..EGR_MAX_PRUNE_ARRAYS table entries are required");
    if (!src_index) return egr_fail(g_prune_error, fn, "src_index is required");
    if (n > PRUNE_MAX_ROWS || count > n) return egr_fail(g_prune_error, fn, "count <= n <= 2^26 rows is required");
    GatherArgs a{};
    uint32_t wmax = 1;
    for (int k = 0; k < num_arrays; k++) {
        if (!arrays[k].src || !arrays[k].dst || arrays[k].width == 0) return egr_fail(g_prune_error, fn, "table entry without src / dst, or with width 0");
        a.t[k] = arrays[k];
        wmax = std::max(wmax, arrays[k].width);
    }
    // out of place only: a parallel gather must never write what another thread still reads (no dst may touch any src or another dst)
    // (an empty table still counts with its first row: count == 0 or n == 0 does not excuse src == dst)
    EgrRange dst[EGR_MAX_PRUNE_ARRAYS], src[EGR_MAX_PRUNE_ARRAYS];
    for (int k = 0; k < num_arrays; k++) {
        dst[k] = EgrRange{arrays[k].dst, (uint64_t)std::max(count, 1u) * arrays[k].width * 4};
        src[k] = EgrRange{arrays[k].src, (uint64_t)std::max(n, 1u) * arrays[k].width * 4};
    }
    if (const EgrClash clash = egr_find_clash(dst, num_arrays, src, num_arrays))
        return egr_fail(g_prune_error, fn, clash.kind == EGR_CLASH_INPUT ? "dst overlaps a src (src == dst or overlapping ranges): the gather runs out of place" : "two dst ranges overlap");
    if (count == 0) return 0;
    a.src_index = src_index, a.count = count;
    const size_t total = (size_t)count * wmax;
    const uint32_t bx = (uint32_t)std::min<size_t>((total + 255) / 256, 65535u * 16u);
    return egr_on_device(device, g_prune_error, fn, [&] { egr_launch(k_prune_gather, dim3(bx, (uint32_t)num_arrays), dim3(256), (hipStream_t)hip_stream, a); });
}
