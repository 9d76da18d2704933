// SPDX-License-Identifier: MIT
// Fused SSIM (include/egr_raytracer.h: egr_eval_ssim, egr_ssim_images): what utils/loss_utils.py:39-70 (ssim) does per pair of display images with five depthwise
// 11 x 11 convolutions in fp32 - on top of the six tone-mapping chains of the evaluation path - as TWO launches for V views, in fp64:
//   k_ssim_partial   grid (tiles per view, V): a workgroup of 256 threads owns one 32 x 32 output tile and loops over the passes that are present and the 3 channels.
//                    Per (pass, channel): load the tile + a 5-pixel halo of both sides (42 x 42, tone_display once per loaded value, an out-of-image tap is an exact
//                    zero and is never read) into LDS as fp32; the row pass of the five moments W*p, W*g, W*pp, W*gg, W*pg into LDS as fp64; the column pass from
//                    LDS, four vertically adjacent outputs per thread; the map in fp64; two sums (all pixels of the tile inside the image, the interior subset)
//                    over the wave's fixed tree. ONE partial of 18 sums per tile: [V][tiles][3 passes][3 channels][2].
//   k_ssim_finish    ONE workgroup per view: sums the partials in ascending tile order, writes the sums and the two means per pass.
// No float atomics and no workgroup waits for another (the stream order between the two launches is the only dependency, as in eval.hip): the result depends on
// the inputs alone, bit for bit on every run.
//
// LDS per workgroup: 2 x 42 x 42 x 4 B (the halos) + 5 x 42 x 32 x 8 B (the row results) + 576 B = 68.4 KB: two workgroups per CU (160 KB).
// Banking (64 banks of 4 B): in every LDS access of the row and the column pass the 32 lanes of a lane group address consecutive elements of one row - fp32 halo
// reads, fp64 row-result stores and loads alike - so none of them conflicts and no padding is needed.
// Work per 1080p view (2040 tiles x 9 pass-channels): 42 x 32 x 55 + 32 x 32 x 55 = 130 k fp64 multiply-adds per tile and channel, 2.4 G in all; the halo
// tone-maps 42 x 42 / (32 x 32) = 1.7 x the pixels. Traffic: 84 B per pixel and view from memory once (the halo's second reads come from the caches).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_eval_shared.hpp"

namespace {

constexpr uint32_t SSIM_THREADS = 256;                  // 4 waves
constexpr int TILE = EGR_SSIM_TILE;                     // output pixels per tile edge
constexpr int TAPS = 11, REACH = TAPS / 2;              // the window and its half width
constexpr int HALO = TILE + 2 * REACH;                  // 42
constexpr uint32_t SSIM_SUMS = 18;                      // 3 passes x 3 channels x {all pixels, interior}
constexpr uint32_t SSIM_MAX_VIEWS = 65535;
constexpr int ROWS_PER_THREAD = TILE * TILE / SSIM_THREADS; // 4 vertically adjacent outputs per thread in the column pass
static_assert(TILE == 32 && ROWS_PER_THREAD == 4, "the thread mappings below are written for a 32 x 32 tile and 256 threads");
constexpr double C1 = 1e-4, C2 = 9e-4;                  // (0.01)^2 and (0.03)^2 for a data range of 1

struct SsimArgs {
    const float *final;     // [V][H][W][3], or the images loader's pred [V][3][H][W]
    const float *rgb;       // [V][3][H][W][3] or NULL
    const float *target[3]; // [V][3][H][W] each or NULL; [0] is the images loader's gt
    double *partial;        // [V][tiles][18]
    double *sum;            // [V][passes][3][2]
    double *mean;           // [V][passes][2]
    double w[TAPS];         // the normalised window, computed on the host in fp64
    uint32_t height, width;
    uint32_t tiles_x, tiles; // tiles per row of tiles and per view
    uint32_t passes;        // 3, or 1 with the images loader
};

// One value of each side at pixel (y, x) of channel c. IMAGES: the two [V][3][H][W] images as they are. Otherwise the raw render and targets through the tone curve.
template <bool IMAGES>
__device__ __forceinline__ void load_pair(const SsimArgs &a, uint32_t v, uint32_t pass, uint32_t c, uint32_t y, uint32_t x, float &p, float &g) {
    const size_t hw = (size_t)a.height * a.width, pix = (size_t)y * a.width + x; // y < height and x < width: every read below is in range
    if (IMAGES) {
        p = a.final[((size_t)v * 3 + c) * hw + pix];
        g = a.target[0][((size_t)v * 3 + c) * hw + pix];
        return;
    }
    float raw;
    if (pass == 0) raw = a.final[((size_t)v * hw + pix) * 3 + c];
    else if (pass == 1) raw = a.rgb[((size_t)v * 3 * hw + pix) * 3 + c];
    else raw = a.rgb[(((size_t)v * 3 + 1) * hw + pix) * 3 + c] + a.rgb[(((size_t)v * 3 + 2) * hw + pix) * 3 + c]; // rgb[1:].sum(0): one fp32 add
    p = tone_display(raw);
    g = tone_display(a.target[pass][((size_t)v * 3 + c) * hw + pix]);
}

template <bool IMAGES>
__global__ void __launch_bounds__(SSIM_THREADS) k_ssim_partial(SsimArgs a) {
    __shared__ float s_p[HALO][HALO], s_g[HALO][HALO];
    __shared__ double s_row[5][HALO][TILE]; // the row pass of mu1, mu2, pp, gg, pg at halo row r and tile column x
    __shared__ double s_wave[SSIM_THREADS / 64][SSIM_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, v = blockIdx.y;
    const int y0 = (int)(blockIdx.x / a.tiles_x) * TILE, x0 = (int)(blockIdx.x % a.tiles_x) * TILE; // the tile's first output pixel
    const int H = (int)a.height, W = (int)a.width;
    const bool on[3] = {a.target[0] != nullptr, !IMAGES && a.target[1] != nullptr && a.rgb != nullptr, !IMAGES && a.target[2] != nullptr && a.rgb != nullptr};
    if (tid < SSIM_SUMS) {
#pragma unroll
        for (uint32_t k = 0; k < SSIM_THREADS / 64; k++) s_wave[k][tid] = 0.0; // (an absent pass stores zeros; k_ssim_finish reports NaN for it)
    }
    const int cx = (int)(tid & 31u), cy = (int)(tid >> 5) * ROWS_PER_THREAD; // column pass: this thread's column and first row inside the tile
    for (uint32_t pass = 0; pass < 3; pass++) {
        if (!on[pass]) continue; // (uniform over the launch)
        for (uint32_t c = 0; c < 3; c++) {
            __syncthreads(); // the previous round's column pass has read s_row; s_wave's zeros are in place
            for (int i = (int)tid; i < HALO * HALO; i += (int)SSIM_THREADS) {
                const int hy = i / HALO, hx = i - hy * HALO, y = y0 + hy - REACH, x = x0 + hx - REACH;
                float p = 0.0f, g = 0.0f; // zero padding: a tap outside the image adds an exact zero to every moment
                if (y >= 0 && y < H && x >= 0 && x < W) load_pair<IMAGES>(a, v, pass, c, (uint32_t)y, (uint32_t)x, p, g);
                s_p[hy][hx] = p, s_g[hy][hx] = g;
            }
            __syncthreads();
            for (int i = (int)tid; i < HALO * TILE; i += (int)SSIM_THREADS) { // row pass: halo row r, tile column x
                const int r = i >> 5, x = i & 31;
                double m1 = 0.0, m2 = 0.0, pp = 0.0, gg = 0.0, pg = 0.0;
#pragma unroll
                for (int k = 0; k < TAPS; k++) {
                    const double p = (double)s_p[r][x + k], g = (double)s_g[r][x + k], w = a.w[k];
                    m1 += w * p, m2 += w * g, pp += w * (p * p), gg += w * (g * g), pg += w * (p * g);
                }
                s_row[0][r][x] = m1, s_row[1][r][x] = m2, s_row[2][r][x] = pp, s_row[3][r][x] = gg, s_row[4][r][x] = pg;
            }
            __syncthreads();
            double m[ROWS_PER_THREAD][5]; // column pass: outputs (cy + j, cx), j = 0..3, from halo rows cy .. cy + 13
#pragma unroll
            for (int j = 0; j < ROWS_PER_THREAD; j++)
#pragma unroll
                for (int q = 0; q < 5; q++) m[j][q] = 0.0;
#pragma unroll
            for (int r = 0; r < TAPS + ROWS_PER_THREAD - 1; r++) {
                double t[5];
#pragma unroll
                for (int q = 0; q < 5; q++) t[q] = s_row[q][cy + r][cx];
#pragma unroll
                for (int j = 0; j < ROWS_PER_THREAD; j++) {
                    if (r - j < 0 || r - j >= TAPS) continue; // (resolved at compile time) output j takes taps k = r - j in ascending order
#pragma unroll
                    for (int q = 0; q < 5; q++) m[j][q] += a.w[r - j] * t[q];
                }
            }
            double all = 0.0, interior = 0.0;
#pragma unroll
            for (int j = 0; j < ROWS_PER_THREAD; j++) {
                const int y = y0 + cy + j, x = x0 + cx;
                const double mu1 = m[j][0], mu2 = m[j][1];
                const double s1 = m[j][2] - mu1 * mu1, s2 = m[j][3] - mu2 * mu2, s12 = m[j][4] - mu1 * mu2;
                const double value = ((2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2));
                if (y < H && x < W) {
                    all += value;
                    if (y >= REACH && y + REACH < H && x >= REACH && x + REACH < W) interior += value; // the whole window lies inside the image
                }
            }
            all = wave_sum(all), interior = wave_sum(interior);
            if (lane == 0) s_wave[wave][(pass * 3 + c) * 2] = all, s_wave[wave][(pass * 3 + c) * 2 + 1] = interior;
        }
    }
    __syncthreads();
    if (tid < SSIM_SUMS) a.partial[((size_t)v * a.tiles + blockIdx.x) * SSIM_SUMS + tid] = ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid];
}

// ONE workgroup per view. Thread t adds the partials of tiles t, t + 256, ... in ascending order, then the fixed tree of wave_sum and the four waves in order.
__global__ void __launch_bounds__(SSIM_THREADS) k_ssim_finish(SsimArgs a) {
    __shared__ double s_wave[SSIM_THREADS / 64][SSIM_SUMS];
    __shared__ double s_sum[SSIM_SUMS];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, v = blockIdx.x;
    const double *partial = a.partial + (size_t)v * a.tiles * SSIM_SUMS;
    double acc[SSIM_SUMS];
#pragma unroll
    for (uint32_t k = 0; k < SSIM_SUMS; k++) acc[k] = 0.0;
    for (uint32_t b = tid; b < a.tiles; b += SSIM_THREADS) {
#pragma unroll
        for (uint32_t k = 0; k < SSIM_SUMS; k++) acc[k] += partial[(size_t)b * SSIM_SUMS + k];
    }
#pragma unroll
    for (uint32_t k = 0; k < SSIM_SUMS; k++) {
        const double s = wave_sum(acc[k]);
        if (lane == 0) s_wave[wave][k] = s;
    }
    __syncthreads();
    const bool on[3] = {a.target[0] != nullptr, a.passes == 3 && a.target[1] != nullptr && a.rgb != nullptr, a.passes == 3 && a.target[2] != nullptr && a.rgb != nullptr};
    const uint32_t sums = a.passes * 6;
    if (tid < sums) {
        const double s = on[tid / 6] ? ((s_wave[0][tid] + s_wave[1][tid]) + s_wave[2][tid]) + s_wave[3][tid] : (double)NAN; // an absent pass reports NaN
        s_sum[tid] = s;
        a.sum[(size_t)v * sums + tid] = s;
    }
    __syncthreads();
    if (tid < a.passes * 2) { // one thread per (pass, flavour)
        const uint32_t pass = tid >> 1, f = tid & 1u;
        const double s = (s_sum[pass * 6 + f] + s_sum[pass * 6 + 2 + f]) + s_sum[pass * 6 + 4 + f]; // the three channels in order
        const bool has_interior = a.height >= (uint32_t)TAPS && a.width >= (uint32_t)TAPS;
        const double n = f == 0 ? 3.0 * (double)a.height * (double)a.width : 3.0 * ((double)a.height - 10.0) * ((double)a.width - 10.0);
        a.mean[((size_t)v * a.passes + pass) * 2 + f] = (f == 1 && !has_interior) ? (double)NAN : s / n;
    }
}

// The checks both entry points share, before any HIP call; then the two launches.
int run(const char *fn, bool images, int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *const target[3],
        double *ssim_sum, double *ssim, void *workspace, void *hip_stream) {
    auto fail = [&](const std::string &what) { return egr_fail(g_eval_error, fn, what); };
    if (num_views == 0 || num_views > SSIM_MAX_VIEWS) return fail("num_views must be in 1..65535");
    if (height == 0 || width == 0) return fail("height and width must be >= 1");
    if (images) {
        if (!final || !target[0]) return fail("pred and gt are required");
    } else if (!final) return fail("final is required");
    if (!ssim_sum || !ssim) return fail("ssim_sum and ssim are required outputs");
    if (!rgb && (target[1] || target[2])) return fail("the diffuse and specular passes need rgb");
    if (!workspace || ((uintptr_t)workspace & 7u)) return fail("an 8-byte aligned workspace of EGR_SSIM_WORKSPACE_BYTES(num_views, height, width) is required");
    const size_t tiles_x = ((size_t)width + TILE - 1) / TILE, tiles = EGR_SSIM_BLOCKS(height, width);
    if (tiles > 0x7FFFFFFFull) return fail("the image is too large");
    const size_t image = (size_t)num_views * height * width * 3 * sizeof(float), passes = images ? 1 : 3;
    const EgrRange in[5] = {{final, image}, {rgb, 3 * image}, {target[0], image}, {target[1], image}, {target[2], image}};
    const EgrRange out[3] = {{ssim_sum, (uint64_t)num_views * passes * 6 * 8}, {ssim, (uint64_t)num_views * passes * 2 * 8}, {workspace, EGR_SSIM_WORKSPACE_BYTES(num_views, height, width)}};
    if (const EgrClash clash = egr_find_clash(out, 3, in, 5))
        return fail(clash.kind == EGR_CLASH_INPUT ? "an output (ssim_sum, ssim, workspace) overlaps an input" : "two outputs (ssim_sum, ssim, workspace) overlap");
    SsimArgs a{};
    a.final = final, a.rgb = rgb, a.target[0] = target[0], a.target[1] = target[1], a.target[2] = target[2];
    a.partial = (double *)workspace, a.sum = ssim_sum, a.mean = ssim;
    a.height = height, a.width = width, a.tiles_x = (uint32_t)tiles_x, a.tiles = (uint32_t)tiles, a.passes = (uint32_t)passes;
    double e[TAPS], total = 0.0; // w[k] = e[k] / sum(e), e[k] = exp(-(k - 5)^2 / (2 * 1.5^2)): fp64, exactly separable, summed in ascending order
    for (int k = 0; k < TAPS; k++) total += e[k] = std::exp(-(double)((k - REACH) * (k - REACH)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < TAPS; k++) a.w[k] = e[k] / total;
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_eval_error, fn, [&] {
        egr_launch(images ? k_ssim_partial<true> : k_ssim_partial<false>, dim3(a.tiles, num_views), dim3(SSIM_THREADS), s, a);
        egr_launch(k_ssim_finish, dim3(num_views), dim3(SSIM_THREADS), s, a);
    });
}

} // namespace

extern "C" int egr_eval_ssim(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *target_final,
                             const float *target_diffuse, const float *target_specular, double *ssim_sum, double *ssim, void *workspace, void *hip_stream) {
    const float *const target[3] = {target_final, target_diffuse, target_specular};
    return run("egr_eval_ssim", false, device, num_views, height, width, final, rgb, target, ssim_sum, ssim, workspace, hip_stream);
}

extern "C" int egr_ssim_images(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *pred, const float *gt, double *ssim_sum, double *ssim,
                               void *workspace, void *hip_stream) {
    const float *const target[3] = {gt, nullptr, nullptr};
    return run("egr_ssim_images", true, device, num_views, height, width, pred, nullptr, target, ssim_sum, ssim, workspace, hip_stream);
}
