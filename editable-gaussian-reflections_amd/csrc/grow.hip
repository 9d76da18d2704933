// SPDX-License-Identifier: MIT
// Growing the cloud (include/egr_raytracer.h: egr_grow_sample / egr_grow_append): what the reference does when the bounces are switched on -
//   the candidates   scene/gaussian_model.py:233-236 add_farfield_points     (torch.randn(75_000, 3).clamp(-3, 3) * extent, from the device generator)
//   the append       scene/gaussian_model.py:533-585 cat_tensors_to_optimizer (8 parameters + 16 Adam moments + per-row extras, one cat each)
// - as ONE launch that writes candidates which are a function of (seed, index) alone, and ONE out-of-place launch over all arrays, the mirror image of
// k_prune_gather. The camera filter between the two is egr_prune_select + egr_prune_gather on the candidates: there is one predicate in the library.
//
// The generator is Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), restated from the paper: candidate i
// takes the counter (i_lo, i_hi, 0, 0) under the key (seed_lo, seed_hi); its four words give four uniforms on the 2^-23 grid (never 0 or 1), and two
// Box-Muller pairs evaluated in fp64 give the three normals, each rounded to fp32 once. No state, no launch-shape dependence, no library whose transform
// could change under us: tests/grow_restatement.py is the same arithmetic in numpy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

namespace {

constexpr uint32_t GROW_THREADS = 256;
constexpr uint64_t GROW_MAX_ROWS = 1ull << 26; // the tree's own limit
constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t x[4]) {
#pragma unroll
    for (int round = 0; round < 10; round++) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
        k0 += PHILOX_W0, k1 += PHILOX_W1; // (the bump after the tenth round is never used)
    }
    x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

// 24 significant bits: exact in fp32 and fp64, in (0, 1)
__device__ __forceinline__ double grid_uniform(uint32_t x) { return ((double)(x >> 9) + 0.5) * (1.0 / 8388608.0); }

__global__ void __launch_bounds__(GROW_THREADS) k_grow_sample(uint64_t first, uint32_t n, uint64_t seed, float radius, float clamp, float *out) {
    const uint32_t r = blockIdx.x * GROW_THREADS + threadIdx.x;
    if (r >= n) return;
    const uint64_t i = first + r; // (first + n does not wrap: checked on the host)
    uint32_t x[4];
    philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), 0u, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    const double two_pi = 6.283185307179586; // fp64(2 pi)
    const double r0 = sqrt(-2.0 * log(grid_uniform(x[0]))), t0 = two_pi * grid_uniform(x[1]);
    const double r1 = sqrt(-2.0 * log(grid_uniform(x[2]))), t1 = two_pi * grid_uniform(x[3]);
    const float z[3] = {(float)(r0 * cos(t0)), (float)(r0 * sin(t0)), (float)(r1 * cos(t1))}; // one rounding each
#pragma unroll
    for (int k = 0; k < 3; k++) out[(size_t)r * 3 + k] = fminf(fmaxf(z[k], -clamp), clamp) * radius;
}

struct AppendArgs {
    egr_grow_array t[EGR_MAX_PRUNE_ARRAYS];
    uint32_t n, m;
};

// A streaming copy. The old rows - 93 % of the words at the reference's size - go as 16 bytes per lane where src and dst are both 16-byte aligned (they share
// their word offsets, so one test covers every vector; a torch allocation always is); the up to three words left of them, the tail - whose seam n * width falls
// anywhere - and every entry that is not aligned go as one word per lane. tools/ubench/copy_width.hip measured the two widths on this copy's size: 5.96 against
// 3.68 TB/s.
__global__ void __launch_bounds__(GROW_THREADS) k_grow_append(AppendArgs a) {
    const egr_grow_array &T = a.t[blockIdx.y];
    const uint32_t *src = (const uint32_t *)T.src, *tail = (const uint32_t *)T.tail;
    uint32_t *dst = (uint32_t *)T.dst;
    const size_t head = (size_t)a.n * T.width, total = head + (size_t)a.m * T.width;
    const size_t first = (size_t)blockIdx.x * GROW_THREADS + threadIdx.x, stride = (size_t)gridDim.x * GROW_THREADS;
    const size_t vectors = (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0 ? head / 4 : 0; // (4 * vectors <= head: inside both arrays)
    for (size_t i = first; i < vectors; i += stride) ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
    const bool rows = T.tail_kind == EGR_GROW_TAIL_ROWS;
    for (size_t i = vectors * 4 + first; i < total; i += stride) dst[i] = i < head ? src[i] : rows ? tail[i - head] : T.fill_bits; // 4-byte words moved as bits
}

thread_local std::string g_grow_error;

} // namespace

extern "C" const char *egr_grow_last_error(void) { return g_grow_error.c_str(); }

extern "C" int egr_grow_sample(int device, uint64_t first, uint32_t n, uint64_t seed, float radius, float clamp, float *out_points, void *hip_stream) {
    const char *fn = "egr_grow_sample";
    // ---- validation: before any HIP call
    if (!out_points) return egr_fail(g_grow_error, fn, "out_points is a required output");
    if (n > GROW_MAX_ROWS) return egr_fail(g_grow_error, fn, "n exceeds 2^26 rows (the limit of the tree)");
    if (first > UINT64_MAX - n) return egr_fail(g_grow_error, fn, "first + n overflows 64 bits");
    if (!std::isfinite(radius) || radius < 0.0f) return egr_fail(g_grow_error, fn, "radius must be finite and not negative");
    if (!std::isfinite(clamp) || clamp < 0.0f) return egr_fail(g_grow_error, fn, "clamp must be finite and not negative");
    if (n == 0) return 0;
    return egr_on_device(device, g_grow_error, fn, [&] {
        egr_launch(k_grow_sample, dim3((n + GROW_THREADS - 1) / GROW_THREADS), dim3(GROW_THREADS), (hipStream_t)hip_stream, first, n, seed, radius, clamp, out_points);
    });
}

extern "C" int egr_grow_append(int device, const egr_grow_array *arrays, int num_arrays, uint32_t n, uint32_t m, void *hip_stream) {
    const char *fn = "egr_grow_append";
    // ---- validation: before any HIP call
    if (!arrays || num_arrays < 1 || num_arrays > EGR_MAX_PRUNE_ARRAYS) return egr_fail(g_grow_error, fn, "1..EGR_MAX_PRUNE_ARRAYS table entries are required");
    if ((uint64_t)n + m > GROW_MAX_ROWS) return egr_fail(g_grow_error, fn, "n + m exceeds 2^26 rows (the limit of the tree)");
    AppendArgs a{};
    uint32_t wmax = 1;
    for (int k = 0; k < num_arrays; k++) {
        const egr_grow_array &T = arrays[k];
        if (!T.dst || T.width == 0) return egr_fail(g_grow_error, fn, "table entry without dst, or with width 0");
        if (T.tail_kind != EGR_GROW_TAIL_ROWS && T.tail_kind != EGR_GROW_TAIL_FILL) return egr_fail(g_grow_error, fn, "unknown tail_kind (EGR_GROW_TAIL_ROWS or EGR_GROW_TAIL_FILL)");
        if (!T.src && n > 0) return egr_fail(g_grow_error, fn, "table entry without src although n > 0");
        if (T.tail_kind == EGR_GROW_TAIL_ROWS && !T.tail && m > 0) return egr_fail(g_grow_error, fn, "EGR_GROW_TAIL_ROWS entry without tail although m > 0");
        a.t[k] = T;
        wmax = std::max(wmax, T.width);
    }
    // out of place only: no dst may touch anything the launch reads, or another dst
    EgrRange dst[EGR_MAX_PRUNE_ARRAYS], in[2 * EGR_MAX_PRUNE_ARRAYS]; // in: every src, then every tail (a fill has none)
    for (int k = 0; k < num_arrays; k++) {
        const egr_grow_array &T = arrays[k];
        dst[k] = EgrRange{T.dst, ((uint64_t)n + m) * T.width * 4};
        in[k] = EgrRange{T.src, (uint64_t)n * T.width * 4};
        in[num_arrays + k] = EgrRange{T.tail_kind == EGR_GROW_TAIL_ROWS ? T.tail : nullptr, (uint64_t)m * T.width * 4};
    }
    if (const EgrClash clash = egr_find_clash(dst, num_arrays, in, 2 * num_arrays))
        return egr_fail(g_grow_error, fn, clash.kind == EGR_CLASH_OUTPUT ? "two dst ranges overlap"
                                          : clash.other < num_arrays     ? "dst overlaps a src (src == dst or overlapping ranges): the append runs out of place"
                                                                         : "dst overlaps a tail: the append runs out of place");
    if ((uint64_t)n + m == 0) return 0;
    a.n = n, a.m = m;
    const size_t total = ((size_t)n + m) * wmax; // words of the widest entry: one thread per 16 bytes of it, the loops stride over the rest
    const uint32_t bx = (uint32_t)std::min<size_t>((total / 4 + GROW_THREADS) / GROW_THREADS, 65535u * 16u);
    return egr_on_device(device, g_grow_error, fn, [&] { egr_launch(k_grow_append, dim3(bx, (uint32_t)num_arrays), dim3(GROW_THREADS), (hipStream_t)hip_stream, a); });
}
