// SPDX-License-Identifier: MIT
// Fused evaluation metrics (include/egr_raytracer.h: egr_eval_metrics): what the reference does per test view after the render -
//   the passes       train.py:103-109 / render.py:216-228     final | rgb[0] | rgb[1:].sum(0) against original | diffuse | specular image
//   the tone curve   utils/tonemapping.py:1-5 + .clamp(0, 1)   nan_to_num(posinf = 999999999.9), the filmic rational, ** 1.3
//   the metric       utils/image_utils.py:19-21 psnr().mean()  per-channel mse -> 20 log10(1 / sqrt(mse)) -> mean over the channels
// - six full-image torch chains, three reductions and their copies per view - as TWO launches for V views:
//   k_eval_partial   grid (blocks per view, V): every workgroup strides over its view's pixels, keeps 9 fp64 sums (3 passes x 3 channels) per thread, reduces them
//                    over the wave and then over the four waves through LDS, and stores ONE partial: [V][blocks][9]. Optionally writes the display images.
//   k_eval_finish    ONE workgroup per view: sums the partials in a fixed order, writes sse [V][3][3] and both PSNR flavours [V][3][2].
// No float atomics and no workgroup waits for another (the stream order between the two launches is the only dependency, as in prune.hip): the result depends on
// the inputs alone, bit for bit on every run.
//
// Traffic per pixel and view: final 12 B + rgb 36 B + three targets 36 B = 84 B read; + 72 B written with `display`.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_eval_shared.hpp"

namespace {

constexpr uint32_t EVAL_THREADS = 256; // 4 waves
constexpr uint32_t EVAL_SUMS = 9;      // 3 passes x 3 channels
constexpr uint32_t EVAL_MAX_VIEWS = 65535;
static_assert(EGR_EVAL_PIXELS_PER_WG % EVAL_THREADS == 0, "a workgroup covers whole strides of its 256 threads");

struct EvalArgs {
    const float *final;          // [V][HW][3]
    const float *rgb;            // [V][3][HW][3] or NULL (then passes 1 and 2 are absent)
    const float *target[3];      // [V][3][HW] each or NULL: final, diffuse, specular
    double *partial;             // [V][blocks][9]
    double *sse;                 // [V][3][3]
    double *psnr;                // [V][3][2]
    float *display;              // [V][3][2][3][HW] or NULL
    uint64_t hw;                 // pixels per view
    uint32_t blocks;             // workgroups per view
};

struct F3 {
    float x, y, z;
};

// D(x) = clamp(tonemap(x), 0, 1) and the wave's fixed summation tree: egr_eval_shared.hpp (csrc/ssim.hip uses the same two)

__global__ void __launch_bounds__(EVAL_THREADS) k_eval_partial(EvalArgs a) {
    __shared__ double s_wave[EVAL_THREADS / 64][EVAL_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, v = blockIdx.y;
    const uint64_t hw = a.hw;
    const F3 *final = (const F3 *)a.final + (size_t)v * hw;
    const F3 *rgb = a.rgb ? (const F3 *)a.rgb + (size_t)v * 3 * hw : nullptr;
    const bool on[3] = {a.target[0] != nullptr, a.target[1] != nullptr && rgb != nullptr, a.target[2] != nullptr && rgb != nullptr};
    double acc[EVAL_SUMS];
#pragma unroll
    for (uint32_t k = 0; k < EVAL_SUMS; k++) acc[k] = 0.0;
    for (uint64_t p = (uint64_t)blockIdx.x * EVAL_THREADS + tid; p < hw; p += (uint64_t)gridDim.x * EVAL_THREADS) { // p < hw: every read and write below is in range
#pragma unroll
        for (uint32_t pass = 0; pass < 3; pass++) {
            if (!on[pass]) continue; // (uniform over the launch)
            F3 pr;
            if (pass == 0) pr = final[p];
            else if (pass == 1) pr = rgb[p];
            else {
                const F3 s1 = rgb[hw + p], s2 = rgb[2 * hw + p];
                pr = F3{s1.x + s2.x, s1.y + s2.y, s1.z + s2.z}; // rgb[1:].sum(0): one fp32 add
            }
            const float *t = a.target[pass] + (size_t)v * 3 * hw + p;
            const float dp[3] = {tone_display(pr.x), tone_display(pr.y), tone_display(pr.z)};
            const float dg[3] = {tone_display(t[0]), tone_display(t[hw]), tone_display(t[2 * hw])};
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) {
                const double d = (double)dp[c] - (double)dg[c];
                acc[pass * 3 + c] += d * d;
            }
            if (a.display) {
                float *out = a.display + (((size_t)v * 3 + pass) * 2) * 3 * hw + p;
#pragma unroll
                for (uint32_t c = 0; c < 3; c++) out[c * hw] = dp[c], out[(3 + c) * hw] = dg[c];
            }
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < EVAL_SUMS; k++) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) s_wave[wave][k] = s;
    }
    __syncthreads();
    if (tid < EVAL_SUMS) a.partial[((size_t)v * a.blocks + blockIdx.x) * EVAL_SUMS + tid] = ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid];
}

// ONE workgroup per view. Thread t adds the partials of blocks t, t + 256, ... in ascending order, then the fixed tree of wave_sum and the four waves in order.
__global__ void __launch_bounds__(EVAL_THREADS) k_eval_finish(EvalArgs a) {
    __shared__ double s_wave[EVAL_THREADS / 64][EVAL_SUMS];
    __shared__ double s_sse[EVAL_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, v = blockIdx.x;
    const double *partial = a.partial + (size_t)v * a.blocks * EVAL_SUMS;
    double acc[EVAL_SUMS];
#pragma unroll
    for (uint32_t k = 0; k < EVAL_SUMS; k++) acc[k] = 0.0;
    for (uint32_t b = tid; b < a.blocks; b += EVAL_THREADS) {
#pragma unroll
        for (uint32_t k = 0; k < EVAL_SUMS; k++) acc[k] += partial[(size_t)b * EVAL_SUMS + k];
    }
#pragma unroll
    for (uint32_t k = 0; k < EVAL_SUMS; k++) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) s_wave[wave][k] = s;
    }
    __syncthreads();
    const bool on[3] = {a.target[0] != nullptr, a.target[1] != nullptr && a.rgb != nullptr, a.target[2] != nullptr && a.rgb != nullptr};
    if (tid < EVAL_SUMS) {
        const double s = on[tid / 3] ? ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid] : (double)NAN; // an absent pass reports NaN
        s_sse[tid] = s;
        a.sse[(size_t)v * EVAL_SUMS + tid] = s;
    }
    __syncthreads();
    if (tid < 3) { // one thread per pass
        const double n = (double)a.hw;
        const double s0 = s_sse[tid * 3], s1 = s_sse[tid * 3 + 1], s2 = s_sse[tid * 3 + 2];
        // image_utils.py:19-21 on a CHW image, then .mean(): 20 log10(1 / sqrt(mse_c)) per CHANNEL (the view(img.shape[0], -1) quirk), averaged; mse 0 gives +inf
        const double per_channel = (20.0 * log10(1.0 / sqrt(s0 / n)) + 20.0 * log10(1.0 / sqrt(s1 / n)) + 20.0 * log10(1.0 / sqrt(s2 / n))) / 3.0;
        const double global = 10.0 * log10(1.0 / (((s0 + s1) + s2) / (3.0 * n))); // PeakSignalNoiseRatio(data_range = 1) over all three channels
        a.psnr[((size_t)v * 3 + tid) * 2] = per_channel;
        a.psnr[((size_t)v * 3 + tid) * 2 + 1] = global;
    }
}

} // namespace

thread_local std::string g_eval_error; // (egr_eval_shared.hpp: shared with ssim.hip and frames.hip)

extern "C" const char *egr_eval_last_error(void) { return g_eval_error.c_str(); }

extern "C" int egr_eval_metrics(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *target_final,
                                const float *target_diffuse, const float *target_specular, double *sse, double *psnr, float *display, void *workspace,
                                void *hip_stream) {
    const char *fn = "egr_eval_metrics";
    auto fail = [&](const std::string &what) { return egr_fail(g_eval_error, fn, what); };
    // ---- validation: before any HIP call
    if (num_views == 0 || num_views > EVAL_MAX_VIEWS) return fail("num_views must be in 1..65535");
    if (height == 0 || width == 0) return fail("height and width must be >= 1");
    if (!final) return fail("final is required");
    if (!sse || !psnr) return fail("sse and psnr are required outputs");
    if (!rgb && (target_diffuse || target_specular)) return fail("the diffuse and specular passes need rgb");
    if (!workspace || ((uintptr_t)workspace & 7u)) return fail("an 8-byte aligned workspace of EGR_EVAL_WORKSPACE_BYTES(num_views, height, width) is required");
    const uint64_t hw = (uint64_t)height * width;
    const size_t blocks = EGR_EVAL_BLOCKS(height, width);
    if (blocks > 0x7FFFFFFFull) return fail("the image is too large");
    const size_t image = (size_t)num_views * hw * 3 * sizeof(float);
    const EgrRange in[5] = {{final, image}, {rgb, 3 * image}, {target_final, image}, {target_diffuse, image}, {target_specular, image}};
    const EgrRange out[4] = {{sse, (uint64_t)num_views * 9 * 8}, {psnr, (uint64_t)num_views * 6 * 8}, {display, 6 * image}, {workspace, EGR_EVAL_WORKSPACE_BYTES(num_views, height, width)}};
    if (const EgrClash clash = egr_find_clash(out, 4, in, 5))
        return fail(clash.kind == EGR_CLASH_INPUT ? "an output (sse, psnr, display, workspace) overlaps an input" : "two outputs (sse, psnr, display, workspace) overlap");
    EvalArgs a{};
    a.final = final, a.rgb = rgb, a.target[0] = target_final, a.target[1] = target_diffuse, a.target[2] = target_specular;
    a.partial = (double *)workspace, a.sse = sse, a.psnr = psnr, a.display = display;
    a.hw = hw, a.blocks = (uint32_t)blocks;
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_eval_error, fn, [&] {
        egr_launch(k_eval_partial, dim3(a.blocks, num_views), dim3(EVAL_THREADS), s, a);
        egr_launch(k_eval_finish, dim3(num_views), dim3(EVAL_THREADS), s, a);
    });
}
