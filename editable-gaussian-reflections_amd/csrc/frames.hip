// SPDX-License-Identifier: MIT
// Evaluation frames (include/egr_raytracer.h: egr_eval_frames): what the reference does with a test view after the render and before metrics.py -
//   the fourteen images  render.py:218-292   seven passes, prediction and ground truth: tone curve or affine map, then torchvision's save_image
//   the byte rule        save_image: x * 255 + 0.5, clamp, truncate;   render.py:303 format_image: clamp, * 255, truncate
//   the 8-bit PSNR       metrics.py: PeakSignalNoiseRatio(data_range = 1) on the bytes read back from the PNGs
// - fourteen full-image torch chains per view - as at most THREE launches for V views:
//   k_frames_range    grid (range blocks, V), only when depth is selected: every workgroup strides over its view's target depth and stores ONE (min key, max key)
//   k_frames_write    grid (EGR_FRAMES_BLOCKS, V): one lane per FOUR consecutive pixels and four such quads per thread. Per kind it loads 48 (12) contiguous bytes of
//                     the pixel-major prediction and 16 bytes per target plane, maps, quantises, stores 12 bytes per frame and keeps the squared byte differences as
//                     32-bit integers; the workgroup stores ONE partial: [V][blocks][21] uint32.
//   k_frames_finish   ONE workgroup per view: adds the partials as 64-bit integers, writes sse8 and both PSNR flavours.
// The sums are integers: no summation order, no rounding. No atomics, no memset, and no workgroup waits for another (the stream order between the launches is
// the only dependency, as in eval.hip). Every fp32 operation of a map or of the byte rule is rounded on its own.
//
// Traffic per pixel and view with all kinds: 80 B of predictions + 68 B of targets read, 42 B written.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_eval_shared.hpp"

namespace {

constexpr uint32_t FR_THREADS = 256;                                                  // 4 waves
constexpr uint32_t FR_QUAD = 4;                                                       // consecutive pixels per lane and step
constexpr uint32_t FR_STEPS = EGR_FRAMES_PIXELS_PER_WG / (FR_THREADS * FR_QUAD);      // quads per thread
constexpr uint32_t FR_SUMS = EGR_FRAMES_KINDS * 3;                                    // 7 kinds x 3 channels
constexpr uint32_t FR_MAX_VIEWS = 65535;
constexpr uint32_t FR_DEPTH = 3;
constexpr uint32_t FR_KEY_NAN_MIN = 0u, FR_KEY_NAN_MAX = 0xFFFFFFFFu;                 // a NaN wins at both ends
static_assert(EGR_FRAMES_PIXELS_PER_WG % (FR_THREADS * FR_QUAD) == 0, "a workgroup covers whole steps of its 256 quads");
// a workgroup's sum of squared byte differences fits 32 bits
static_assert((uint64_t)EGR_FRAMES_PIXELS_PER_WG * 255 * 255 < (1ull << 32), "the partial sums are 32-bit integers");
static_assert(EGR_FRAMES_RANGE_BLOCKS <= 64, "one wave reads a view's range partials");

__host__ __device__ constexpr uint32_t kind_channels(uint32_t kind) { return kind == FR_DEPTH || kind == 5 ? 1u : 3u; }

struct FramesArgs {
    const float *pred[EGR_FRAMES_KINDS];   // the prediction of each kind at view 0 (specular: rgb[0][1]; its second term lies one step further) or NULL
    uint64_t pred_stride[EGR_FRAMES_KINDS]; // floats from view to view
    const float *target[EGR_FRAMES_KINDS]; // [V][C][HW] or NULL
    uint8_t *frames;
    int64_t *sse8;                         // [V][7][3]
    double *psnr8;                         // [V][7][2]
    float *depth_range;                    // [V][2] or NULL
    uint32_t *range_partial;               // workspace: [V][EGR_FRAMES_RANGE_BLOCKS][2] keys
    uint32_t *partial;                     // workspace: [V][blocks][21]
    uint64_t hw;
    uint32_t H, W, blocks, range_blocks;
    uint32_t kinds;                        // the kinds to write (depth without its target is not among them)
    uint32_t report;                       // the kinds whose sse8 / psnr8 slots are written: the caller's selection
    uint32_t rounding, depth_mode, layout;
};

// order-preserving key of an fp32 bit pattern (-0 < +0), and back (csrc/viewset.hip has the same pair)
__device__ __forceinline__ uint32_t order_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// four consecutive floats at src into a 16-byte aligned local; lanes of the tail read only what exists
__device__ __forceinline__ void load4(const float *src, uint32_t valid, float x[4]) {
    if (valid == FR_QUAD && ((uintptr_t)src & 15u) == 0) {
        *(float4 *)x = *(const float4 *)src;
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) x[j] = j < valid ? src[j] : 0.0f;
    }
}

// four pixel-major pixels of three floats at src: 48 contiguous bytes
__device__ __forceinline__ void load12(const float *src, uint32_t valid, float x[12]) {
    if (valid == FR_QUAD && ((uintptr_t)src & 15u) == 0) {
#pragma unroll
        for (uint32_t j = 0; j < 3; j++) *(float4 *)(x + 4 * j) = ((const float4 *)src)[j];
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 12; j++) x[j] = j < 3 * valid ? src[j] : 0.0f;
    }
}

// the byte of a mapped value. NaN gives 0 (a definition: torch leaves the conversion unspecified), +inf 255, -inf 0.
__device__ __forceinline__ uint32_t quantise(float x, uint32_t rounding) {
#pragma clang fp contract(off)
    float y;
    if (rounding == EGR_FRAMES_ROUND_SAVE) { // save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)
        y = x * 255.0f;
        y = y + 0.5f;
        y = y < 0.0f ? 0.0f : y;
        y = y > 255.0f ? 255.0f : y;
    } else { // format_image: (image.clamp(0, 1) * 255).to(uint8)
        y = x < 0.0f ? 0.0f : x;
        y = y > 1.0f ? 1.0f : y;
        y = y * 255.0f;
    }
    return y != y ? 0u : (uint32_t)y; // (y is in [0, 255]: the conversion truncates)
}

struct DepthMap {
    float lo, hi, span; // span = hi - lo
};

// the value map of a kind, both sides alike
template <uint32_t KIND>
__device__ __forceinline__ float map_value(float x, const DepthMap &d, uint32_t depth_mode) {
#pragma clang fp contract(off)
    if (KIND <= 2) return tone_display(x);
    if (KIND == FR_DEPTH) return depth_mode == EGR_FRAMES_DEPTH_MAX ? __fdiv_rn(x, d.hi) : __fdiv_rn(x - d.lo, d.span);
    if (KIND == 4) {
        const float h = x / 2.0f; // (exact or correctly rounded, as the division is)
        return h + 0.5f;
    }
    return x;
}

// Where a quad lies: its first pixel, the number of its pixels that exist, and - side by side only - the row and column of the first pixel
struct Quad {
    uint64_t p0;
    uint32_t valid, y0, x0;
};

// Stores the 12 bytes of four pixels (b[k][c]) of one frame side. Separate: `frame` is the side's [HW][3]. Side by side: `frame` is the pair's [H][2W][3] and the
// side's first column is side * W. A whole quad that lies in one row and starts on a 4-byte boundary goes out as three word stores; every other one byte by byte.
__device__ __forceinline__ void store_quad(uint8_t *frame, const FramesArgs &a, const Quad &q, uint32_t side, const uint32_t b[4][3]) {
    const bool sbs = a.layout == EGR_FRAMES_SIDE_BY_SIDE;
    if (q.valid == FR_QUAD && (!sbs || (a.W & 3u) == 0)) { // (W % 4 == 0 and p0 % 4 == 0: the quad does not leave row y0)
        uint8_t *dst = frame + (sbs ? ((uint64_t)q.y0 * 2 * a.W + q.x0 + (uint64_t)side * a.W) * 3 : q.p0 * 3);
        if (((uintptr_t)dst & 3u) == 0) {
            uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
            for (uint32_t i = 0; i < 12; i++) w[i >> 2] |= b[i / 3][i % 3] << ((i & 3u) * 8);
#pragma unroll
            for (uint32_t j = 0; j < 3; j++) ((uint32_t *)dst)[j] = w[j];
            return;
        }
    }
    uint32_t y = q.y0, x = q.x0;
#pragma unroll
    for (uint32_t k = 0; k < FR_QUAD; k++) {
        if (k >= q.valid) break;
        uint64_t at = (q.p0 + k) * 3;
        if (sbs) {
            if (x >= a.W) x = 0, y++; // (pixel p0 + k exists, so y < H)
            at = ((uint64_t)y * 2 * a.W + x + (uint64_t)side * a.W) * 3;
            x++;
        }
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) frame[at + c] = (uint8_t)b[k][c];
    }
}

// One kind of one quad: both sides loaded, mapped, quantised and stored; the squared byte differences added to acc[0..C) when both sides exist.
template <uint32_t KIND>
__device__ __forceinline__ void do_kind(const FramesArgs &a, uint32_t v, const Quad &q, const DepthMap &dm, uint32_t acc[3]) {
    const uint64_t p0 = q.p0;
    const uint32_t valid = q.valid;
    constexpr uint32_t C = kind_channels(KIND);
    const uint64_t hw = a.hw;
    const bool has_pred = a.pred[KIND] != nullptr, has_gt = a.target[KIND] != nullptr; // (uniform over the launch; depth without its target is not selected)
    uint8_t *slot = a.frames + ((size_t)v * EGR_FRAMES_KINDS + KIND) * 2 * hw * 3; // [2 sides][HW][3] or [H][2W][3]
    const bool sbs = a.layout == EGR_FRAMES_SIDE_BY_SIDE;
    uint32_t pb[4][3], gb[4][3];
    if (has_pred) {
        const float *src = a.pred[KIND] + (size_t)v * a.pred_stride[KIND] + p0 * C;
        alignas(16) float x[4 * C];
        if constexpr (C == 3) load12(src, valid, x);
        else load4(src, valid, x);
        if constexpr (KIND == 2) { // rgb[1] + rgb[2]: one fp32 add
            alignas(16) float x2[12];
            load12(src + hw * 3, valid, x2);
#pragma unroll
            for (uint32_t j = 0; j < 12; j++) x[j] = x[j] + x2[j];
        }
#pragma unroll
        for (uint32_t k = 0; k < FR_QUAD; k++)
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) pb[k][c] = c < C ? quantise(map_value<KIND>(x[k * C + c], dm, a.depth_mode), a.rounding) : pb[k][0];
        store_quad(slot, a, q, 0, pb);
    }
    if (has_gt) {
        const float *src = a.target[KIND] + (size_t)v * C * hw + p0;
#pragma unroll
        for (uint32_t c = 0; c < C; c++) {
            alignas(16) float t[4];
            load4(src + (size_t)c * hw, valid, t);
#pragma unroll
            for (uint32_t k = 0; k < FR_QUAD; k++) gb[k][c] = quantise(map_value<KIND>(t[k], dm, a.depth_mode), a.rounding);
        }
        if (C == 1) {
#pragma unroll
            for (uint32_t k = 0; k < FR_QUAD; k++) gb[k][1] = gb[k][2] = gb[k][0];
        }
        store_quad(sbs ? slot : slot + hw * 3, a, q, 1, gb);
    }
    if (has_pred && has_gt) {
#pragma unroll
        for (uint32_t k = 0; k < FR_QUAD; k++) {
            if (k >= valid) break;
#pragma unroll
            for (uint32_t c = 0; c < C; c++) {
                const int32_t d = (int32_t)pb[k][c] - (int32_t)gb[k][c];
                acc[c] += (uint32_t)(d * d);
            }
        }
    }
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// The range of each view's target depth: one (min key, max key) per workgroup; a NaN takes both ends.
__global__ void __launch_bounds__(FR_THREADS) k_frames_range(FramesArgs a) {
    __shared__ uint32_t s_min[FR_THREADS / 64], s_max[FR_THREADS / 64];
    const uint32_t tid = threadIdx.x, v = blockIdx.y;
    const uint64_t hw = a.hw;
    const float *depth = a.target[FR_DEPTH] + (size_t)v * hw;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u; // (nothing seen)
    for (uint64_t p0 = ((uint64_t)blockIdx.x * FR_THREADS + tid) * FR_QUAD; p0 < hw; p0 += (uint64_t)gridDim.x * FR_THREADS * FR_QUAD) { // p0 < hw: valid >= 1
        const uint32_t valid = hw - p0 < FR_QUAD ? (uint32_t)(hw - p0) : FR_QUAD;
        alignas(16) float t[4];
        load4(depth + p0, valid, t);
#pragma unroll
        for (uint32_t k = 0; k < FR_QUAD; k++) {
            if (k >= valid) break;
            const bool nan = t[k] != t[k];
            const uint32_t key = order_key(__float_as_uint(t[k]));
            const uint32_t lo = nan ? FR_KEY_NAN_MIN : key, hi = nan ? FR_KEY_NAN_MAX : key;
            kmin = lo < kmin ? lo : kmin, kmax = hi > kmax ? hi : kmax;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t omin = __shfl_xor(kmin, off, 64), omax = __shfl_xor(kmax, off, 64);
        kmin = omin < kmin ? omin : kmin, kmax = omax > kmax ? omax : kmax;
    }
    if ((tid & 63u) == 0) s_min[tid >> 6] = kmin, s_max[tid >> 6] = kmax;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (uint32_t w = 1; w < FR_THREADS / 64; w++) kmin = s_min[w] < kmin ? s_min[w] : kmin, kmax = s_max[w] > kmax ? s_max[w] : kmax;
        uint32_t *out = a.range_partial + ((size_t)v * EGR_FRAMES_RANGE_BLOCKS + blockIdx.x) * 2;
        out[0] = kmin, out[1] = kmax;
    }
}

__global__ void __launch_bounds__(FR_THREADS) k_frames_write(FramesArgs a) {
    __shared__ uint32_t s_wave[FR_THREADS / 64][FR_SUMS];
    __shared__ float s_range[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, v = blockIdx.y;
    const uint64_t hw = a.hw;
    const uint32_t kinds = a.kinds;
    DepthMap dm{0.0f, 0.0f, 0.0f};
    if (kinds & (1u << FR_DEPTH)) { // (uniform) the first wave folds the view's range partials: every workgroup the same values in the same order
        if (wave == 0) {
            uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
            if (lane < a.range_blocks) {
                const uint32_t *in = a.range_partial + ((size_t)v * EGR_FRAMES_RANGE_BLOCKS + lane) * 2;
                kmin = in[0], kmax = in[1];
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t omin = __shfl_xor(kmin, off, 64), omax = __shfl_xor(kmax, off, 64);
                kmin = omin < kmin ? omin : kmin, kmax = omax > kmax ? omax : kmax;
            }
            if (lane == 0) {
                const bool nan = kmin == FR_KEY_NAN_MIN; // (a view has at least one pixel, so the keys of a number were seen otherwise)
                const float lo = nan ? __uint_as_float(0x7FC00000u) : __uint_as_float(key_bits(kmin)), hi = nan ? __uint_as_float(0x7FC00000u) : __uint_as_float(key_bits(kmax));
                s_range[0] = lo, s_range[1] = hi;
                if (blockIdx.x == 0 && a.depth_range) a.depth_range[(size_t)v * 2] = lo, a.depth_range[(size_t)v * 2 + 1] = hi;
            }
        }
        __syncthreads();
        dm.lo = s_range[0], dm.hi = s_range[1];
        {
#pragma clang fp contract(off)
            dm.span = dm.hi - dm.lo;
        }
    }
    uint32_t acc[EGR_FRAMES_KINDS][3];
#pragma unroll
    for (uint32_t k = 0; k < EGR_FRAMES_KINDS; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0u;
    for (uint32_t step = 0; step < FR_STEPS; step++) {
        const uint64_t p0 = ((uint64_t)blockIdx.x * (EGR_FRAMES_PIXELS_PER_WG / FR_QUAD) + (uint64_t)step * FR_THREADS + tid) * FR_QUAD;
        if (p0 >= hw) break; // every read and write below is of pixels p0 .. p0 + valid - 1 < hw
        Quad q{p0, hw - p0 < FR_QUAD ? (uint32_t)(hw - p0) : FR_QUAD, 0u, 0u};
        if (a.layout == EGR_FRAMES_SIDE_BY_SIDE) q.y0 = (uint32_t)(p0 / a.W), q.x0 = (uint32_t)(p0 - (uint64_t)q.y0 * a.W);
        if (kinds & 1u) do_kind<0>(a, v, q, dm, acc[0]);
        if (kinds & 2u) do_kind<1>(a, v, q, dm, acc[1]);
        if (kinds & 4u) do_kind<2>(a, v, q, dm, acc[2]);
        if (kinds & 8u) do_kind<3>(a, v, q, dm, acc[3]);
        if (kinds & 16u) do_kind<4>(a, v, q, dm, acc[4]);
        if (kinds & 32u) do_kind<5>(a, v, q, dm, acc[5]);
        if (kinds & 64u) do_kind<6>(a, v, q, dm, acc[6]);
    }
#pragma unroll
    for (uint32_t k = 0; k < EGR_FRAMES_KINDS; k++)
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            const uint32_t s = wave_sum_u32(acc[k][c < kind_channels(k) ? c : 0]); // (a one-channel kind: the same sum three times, folded by the compiler)
            if (lane == 0) s_wave[wave][k * 3 + c] = s;
        }
    __syncthreads();
    if (tid < FR_SUMS) a.partial[((size_t)v * a.blocks + blockIdx.x) * FR_SUMS + tid] = s_wave[0][tid] + s_wave[1][tid] + s_wave[2][tid] + s_wave[3][tid];
}

// ONE workgroup per view: integer sums of the partials, then the two PSNR flavours in fp64.
__global__ void __launch_bounds__(FR_THREADS) k_frames_finish(FramesArgs a) {
    __shared__ unsigned long long s_wave[FR_THREADS / 64][FR_SUMS];
    __shared__ unsigned long long s_sse[FR_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, v = blockIdx.x;
    const uint32_t *partial = a.partial + (size_t)v * a.blocks * FR_SUMS;
    unsigned long long acc[FR_SUMS];
#pragma unroll
    for (uint32_t k = 0; k < FR_SUMS; k++) acc[k] = 0ull;
    for (uint32_t b = tid; b < a.blocks; b += FR_THREADS) {
#pragma unroll
        for (uint32_t k = 0; k < FR_SUMS; k++) acc[k] += partial[(size_t)b * FR_SUMS + k];
    }
#pragma unroll
    for (uint32_t k = 0; k < FR_SUMS; k++) {
        unsigned long long s = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
        if (lane == 0) s_wave[wave][k] = s;
    }
    __syncthreads();
    if (tid < FR_SUMS) {
        const uint32_t kind = tid / 3;
        const bool scored = a.pred[kind] != nullptr && a.target[kind] != nullptr;
        const unsigned long long s = s_wave[0][tid] + s_wave[1][tid] + s_wave[2][tid] + s_wave[3][tid];
        s_sse[tid] = s;
        if (a.report & (1u << kind)) a.sse8[(size_t)v * FR_SUMS + tid] = scored ? (int64_t)s : -1; // a kind that lacks a side reports -1
    }
    __syncthreads();
    if (tid < EGR_FRAMES_KINDS && (a.report & (1u << tid))) { // one thread per kind
        const bool scored = a.pred[tid] != nullptr && a.target[tid] != nullptr;
        double per_channel = (double)NAN, global = (double)NAN;
        if (scored) {
            const double n = 65025.0 * (double)a.hw; // 255^2 n: mse = sse8 / (255^2 n) is the mse of the bytes / 255
            const unsigned long long s0 = s_sse[tid * 3], s1 = s_sse[tid * 3 + 1], s2 = s_sse[tid * 3 + 2];
            // the two flavours of egr_eval_metrics, on the bytes; mse 0 gives +inf
            per_channel = (20.0 * log10(1.0 / sqrt((double)s0 / n)) + 20.0 * log10(1.0 / sqrt((double)s1 / n)) + 20.0 * log10(1.0 / sqrt((double)s2 / n))) / 3.0;
            global = 10.0 * log10(1.0 / ((double)(s0 + s1 + s2) / (3.0 * n)));
        }
        a.psnr8[((size_t)v * EGR_FRAMES_KINDS + tid) * 2] = per_channel;
        a.psnr8[((size_t)v * EGR_FRAMES_KINDS + tid) * 2 + 1] = global;
    }
}

const char *const KIND_NAMES[EGR_FRAMES_KINDS] = {"render", "diffuse", "specular", "depth", "normal", "roughness", "f0"};

} // namespace

extern "C" int egr_eval_frames(int device, const egr_frames_args *args, void *hip_stream) {
    const char *fn = "egr_eval_frames";
    auto fail = [&](const std::string &what) { return egr_fail(g_eval_error, fn, what); };
    // ---- validation: before any HIP call
    if (!args) return fail("args is required");
    const egr_frames_args &g = *args;
    if (g.num_views == 0 || g.num_views > FR_MAX_VIEWS) return fail("num_views must be in 1..65535");
    if (g.height == 0 || g.width == 0) return fail("height and width must be >= 1");
    if (g.kinds == 0) return fail("kinds is empty: select at least one of the seven kinds");
    if (g.kinds & ~EGR_FRAMES_ALL_KINDS) return fail("kinds has unknown bits (bit k selects kind k, k < 7)");
    if (g.rounding != EGR_FRAMES_ROUND_SAVE && g.rounding != EGR_FRAMES_ROUND_TRUNC) return fail("unknown rounding (EGR_FRAMES_ROUND_SAVE or EGR_FRAMES_ROUND_TRUNC)");
    if (g.depth_mode != EGR_FRAMES_DEPTH_MAX && g.depth_mode != EGR_FRAMES_DEPTH_MINMAX) return fail("unknown depth_mode (EGR_FRAMES_DEPTH_MAX or EGR_FRAMES_DEPTH_MINMAX)");
    if (g.layout != EGR_FRAMES_SEPARATE && g.layout != EGR_FRAMES_SIDE_BY_SIDE) return fail("unknown layout (EGR_FRAMES_SEPARATE or EGR_FRAMES_SIDE_BY_SIDE)");
    if (!g.rgb && (((g.kinds & 2u) && g.targets[1]) || ((g.kinds & 4u) && g.targets[2]))) return fail("the diffuse and specular kinds need rgb");
    if (!g.frames || !g.sse8 || !g.psnr8) return fail("frames, sse8 and psnr8 are required outputs");
    if (!g.workspace || ((uintptr_t)g.workspace & 7u)) return fail("an 8-byte aligned workspace of EGR_FRAMES_WORKSPACE_BYTES(num_views, height, width) is required");
    if (((uintptr_t)g.sse8 & 7u) || ((uintptr_t)g.psnr8 & 7u) || ((uintptr_t)g.depth_range & 3u)) return fail("misaligned sse8, psnr8 or depth_range");
    const uint64_t hw = (uint64_t)g.height * g.width;
    const size_t blocks = EGR_FRAMES_BLOCKS(g.height, g.width);
    if (blocks > 0x7FFFFFFFull) return fail("the image is too large");
    const size_t V = g.num_views, plane = (size_t)hw * sizeof(float);
    const char *const in_name[13] = {"final", "rgb", "depth", "normal", "roughness", "f0", "target render", "target diffuse", "target specular", "target depth", "target normal",
                                     "target roughness", "target f0"};
    const EgrRange in[13] = {{g.final, V * 3 * plane}, {g.rgb, V * 9 * plane}, {g.depth, V * 3 * plane}, {g.normal, V * 9 * plane}, {g.roughness, V * 3 * plane},
                             {g.f0, V * 9 * plane}, {g.targets[0], V * 3 * plane}, {g.targets[1], V * 3 * plane}, {g.targets[2], V * 3 * plane}, {g.targets[3], V * plane},
                             {g.targets[4], V * 3 * plane}, {g.targets[5], V * plane}, {g.targets[6], V * 3 * plane}};
    const char *const out_name[5] = {"frames", "sse8", "psnr8", "depth_range", "workspace"};
    const EgrRange out[5] = {{g.frames, V * EGR_FRAMES_KINDS * 2 * (size_t)hw * 3}, {g.sse8, V * FR_SUMS * 8}, {g.psnr8, V * EGR_FRAMES_KINDS * 2 * 8}, {g.depth_range, V * 2 * 4},
                             {g.workspace, EGR_FRAMES_WORKSPACE_BYTES(g.num_views, g.height, g.width)}};
    for (int i = 0; i < 13; i++)
        if ((uintptr_t)in[i].p & 3u) return fail(std::string(in_name[i]) + " is not 4-byte aligned");
    if (const EgrClash clash = egr_find_clash(out, 5, in, 13))
        return fail(clash.kind == EGR_CLASH_INPUT ? std::string("an output (") + out_name[clash.out] + ") overlaps an input (" + in_name[clash.other] + ")"
                                                  : std::string("two outputs (") + out_name[clash.out] + ", " + out_name[clash.other] + ") overlap");
    FramesArgs a{};
    const float *pred[EGR_FRAMES_KINDS] = {g.final, g.rgb, g.rgb ? g.rgb + (size_t)hw * 3 : nullptr, g.depth, g.normal, g.roughness, g.f0};
    const uint64_t steps = EGR_NUM_STEPS;
    const uint64_t stride[EGR_FRAMES_KINDS] = {hw * 3, steps * hw * 3, steps * hw * 3, steps * hw, steps * hw * 3, steps * hw, steps * hw * 3};
    a.kinds = a.report = g.kinds;
    if (!g.targets[FR_DEPTH]) a.kinds &= ~(1u << FR_DEPTH); // both sides of depth are scaled by the target's range: without it the kind is skipped
    for (uint32_t k = 0; k < EGR_FRAMES_KINDS; k++) a.pred[k] = pred[k], a.pred_stride[k] = stride[k], a.target[k] = g.targets[k];
    a.frames = g.frames, a.sse8 = g.sse8, a.psnr8 = g.psnr8, a.depth_range = g.depth_range;
    a.range_partial = (uint32_t *)g.workspace;
    a.partial = a.range_partial + V * EGR_FRAMES_RANGE_BLOCKS * 2;
    a.hw = hw, a.H = g.height, a.W = g.width, a.blocks = (uint32_t)blocks;
    const uint64_t range_blocks = (hw + FR_THREADS * FR_QUAD - 1) / (FR_THREADS * FR_QUAD);
    a.range_blocks = (uint32_t)(range_blocks < EGR_FRAMES_RANGE_BLOCKS ? range_blocks : EGR_FRAMES_RANGE_BLOCKS);
    a.rounding = g.rounding, a.depth_mode = g.depth_mode, a.layout = g.layout;
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_eval_error, fn, [&] {
        if (a.kinds & (1u << FR_DEPTH)) egr_launch(k_frames_range, dim3(a.range_blocks, g.num_views), dim3(FR_THREADS), s, a);
        if (a.kinds) egr_launch(k_frames_write, dim3(a.blocks, g.num_views), dim3(FR_THREADS), s, a); // (depth alone without its target: nothing to write, -1 and NaN to report)
        egr_launch(k_frames_finish, dim3(g.num_views), dim3(FR_THREADS), s, a);
    });
}
