// SPDX-License-Identifier: MIT
// Prior views (include/egr_raytracer.h: egr_prior_pairs / egr_prior_fit / egr_prior_finish): what the reference's prior datasets do per view on the CPU before a
// network-predicted G-buffer can be trained on -
//   the sparse depth  utils/depth_utils.py:101-182 transform_points, project_pointcloud_to_depth_map
//   the fit           utils/depth_utils.py:208-278 ransac_linear_fit   (100 x [lstsq, residuals, topk, SSE], then a refit)
//   the distance      utils/depth_utils.py:66-98   transform_depth_to_position_image + norm
//   the normals, f0   utils/depth_utils.py:7-16, dataset/blender_prior_dataset.py:126
// - for a chunk of V views in six launches and no host synchronisation of their own: a fill, k_prior_project (one lane per point, an atomic minimum per kept
// point), k_prior_pairs (one workgroup and one scan per view: a stable compaction in row-major order), k_prior_hypotheses (one workgroup per hypothesis and view:
// an fp64 fit, a 4-pass radix select of the top_k-th residual, an fp64 error), k_prior_select (one workgroup per view: the best hypothesis, its inliers by the tie
// rule, the fp64 refit) and k_prior_finish (one lane per pixel). Every fp32 product, quotient and sum below is rounded on its own, as torch evaluates them:
// the whole file is compiled without contraction. tests/priors_restatement.py is the same arithmetic in numpy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t PR_THREADS = 256; // project, hypotheses, select, finish; = the bins of a radix pass
constexpr uint32_t PR_WAVES = PR_THREADS / 64;
constexpr uint32_t PR_SCAN_THREADS = 1024; // pairs: one workgroup per view
constexpr uint32_t PR_SCAN_WAVES = PR_SCAN_THREADS / 64;
constexpr uint32_t PR_MAX_SIDE = 65535;
constexpr uint32_t PR_INF = 0x7F800000u;
constexpr uint32_t PR_CAM = EGR_PRIOR_CAM_FLOATS, PR_FX = 12, PR_R = 16; // a row of cams: w2c [12], fx fy cx cy, R [9]

__device__ __forceinline__ bool finite_bits(uint32_t bits) { return (bits & PR_INF) != PR_INF; }

// ---- step 1: the nearest point per pixel
__global__ void __launch_bounds__(PR_THREADS) k_prior_project(const float *cams, const float *points, const uint32_t *offsets, uint32_t total, float *sparse, uint32_t H, uint32_t W) {
    const uint32_t v = blockIdx.y;
    uint32_t last = offsets[v + 1], first = offsets[v];
    last = last < total ? last : total, first = first < last ? first : last; // (inside the points whatever the device copy holds)
    const uint64_t i = (uint64_t)first + (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (i >= last) return;
    const float *m = cams + (size_t)v * PR_CAM;
    const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
    const float cx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const float cy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const float cz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    if (!(cz > 0.0f) || !finite_bits(__float_as_uint(cz))) return; // behind the camera, NaN; +inf = empty
    const float u = rintf(cx * m[PR_FX] / cz + m[PR_FX + 2]), r = rintf(cy * m[PR_FX + 1] / cz + m[PR_FX + 3]); // halves to even, as torch.round
    if (!(u >= 0.0f && u < (float)W && r >= 0.0f && r < (float)H)) return;                                      // (-0 is column 0; a NaN is outside)
    atomicMin((unsigned int *)sparse + ((size_t)v * H + (uint32_t)r) * W + (uint32_t)u, __float_as_uint(cz));   // positive floats order as their patterns
}

// ---- step 2: the pairs of a view in row-major order. Wave w owns the w-th run of pixels: it counts its pairs, the 16 counts are scanned, it writes its pairs
// from its base with a ballot per 64 pixels. A wave takes four rows of 64 pixels per step, so that four loads of the map - and, under a point, of the predicted
// depth - are in flight per lane: one workgroup per view is bound by the latency of its loads. The map is read twice (it stays in L2).
constexpr uint32_t PR_ROWS = 4;

// rows j < PR_ROWS of 64 pixels from q: whether lane's pixel of row j holds a point, and its pair (keep: the prediction is finite)
__device__ __forceinline__ void load_rows(const float *sp, const float *dp, uint32_t C, uint64_t q, uint64_t end, uint32_t lane, bool point[PR_ROWS], bool keep[PR_ROWS], float x[PR_ROWS],
                                          float y[PR_ROWS]) {
    uint32_t bits[PR_ROWS];
#pragma unroll
    for (uint32_t j = 0; j < PR_ROWS; j++) {
        const uint64_t p = q + j * 64 + lane;
        bits[j] = p < end ? __float_as_uint(sp[p]) : PR_INF;
    }
#pragma unroll
    for (uint32_t j = 0; j < PR_ROWS; j++) {
        point[j] = bits[j] < PR_INF;
        x[j] = point[j] ? dp[(q + j * 64 + lane) * C] : 0.0f;
    }
#pragma unroll
    for (uint32_t j = 0; j < PR_ROWS; j++) y[j] = __uint_as_float(bits[j]), keep[j] = point[j] && finite_bits(__float_as_uint(x[j]));
}

__global__ void __launch_bounds__(PR_SCAN_THREADS) k_prior_pairs(const float *depth, uint32_t C, const float *sparse, float *pairs_x, float *pairs_y, uint32_t *count, uint32_t *dropped, uint64_t HW) {
    __shared__ uint32_t wave_count[PR_SCAN_WAVES], wave_drop[PR_SCAN_WAVES];
    const uint32_t v = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const float *sp = sparse + (size_t)v * HW, *dp = depth + (size_t)v * HW * C;
    const uint64_t run = ((HW + PR_SCAN_THREADS - 1) / PR_SCAN_THREADS) * 64; // pixels per wave: a multiple of 64
    const uint64_t p0 = (uint64_t)wave * run < HW ? (uint64_t)wave * run : HW, p1 = p0 + run < HW ? p0 + run : HW;
    bool point[PR_ROWS], keep[PR_ROWS];
    float x[PR_ROWS], y[PR_ROWS];
    uint32_t n = 0, d = 0;
    for (uint64_t q = p0; q < p1; q += PR_ROWS * 64) { // (uniform over the wave)
        load_rows(sp, dp, C, q, p1, lane, point, keep, x, y);
#pragma unroll
        for (uint32_t j = 0; j < PR_ROWS; j++) n += keep[j] ? 1u : 0u, d += point[j] && !keep[j] ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64), d += __shfl_xor(d, off, 64);
    if (lane == 0) wave_count[wave] = n, wave_drop[wave] = d;
    __syncthreads();
    uint32_t base = 0, all = 0, drops = 0;
#pragma unroll
    for (uint32_t w = 0; w < PR_SCAN_WAVES; w++) base += w < wave ? wave_count[w] : 0u, all += wave_count[w], drops += wave_drop[w];
    if (threadIdx.x == 0) count[v] = all, dropped[v] = drops;
    float *ox = pairs_x + (size_t)v * HW, *oy = pairs_y + (size_t)v * HW;
    for (uint64_t q = p0; q < p1; q += PR_ROWS * 64) {
        load_rows(sp, dp, C, q, p1, lane, point, keep, x, y);
#pragma unroll
        for (uint32_t j = 0; j < PR_ROWS; j++) { // row after row, lane after lane: the pixel order
            const uint64_t mask = __ballot(keep[j]);
            if (keep[j]) {
                const uint32_t at = base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)); // (< all <= HW)
                ox[at] = x[j], oy[at] = y[j];
            }
            base += (uint32_t)__popcll(mask);
        }
    }
}

// ---- steps 3 and 4
struct FitArgs {
    const float *pairs_x, *pairs_y;
    const uint32_t *views;
    const int32_t *samples;
    double *hyp_error;
    float *hyp_model;
    float *ab;
    int32_t *best_iteration;
    double *best_error;
    uint8_t *inliers;
    uint32_t pair_stride, num_iters, sample_stride, method;
};

// what a view may use of its row, whatever the device copy of `views` holds: n <= pair_stride pairs, S <= sample_stride indices, 1 <= k <= n
__device__ __forceinline__ void view_sizes(const FitArgs &a, uint32_t v, uint32_t &n, uint32_t &S, uint32_t &k) {
    const uint32_t *e = a.views + (size_t)v * 4;
    n = e[0] < a.pair_stride ? e[0] : a.pair_stride;
    S = e[1] < a.sample_stride ? e[1] : a.sample_stride;
    S = S < (uint32_t)EGR_PRIOR_MAX_SAMPLE ? S : (uint32_t)EGR_PRIOR_MAX_SAMPLE;
    k = e[2] < n ? e[2] : n;
    k = k ? k : 1u;
}

// y = w x + b from the means and the centred sums; without spread in x the minimum-norm solution of [x 1] (w b)^T = y, as lstsq
__device__ __forceinline__ void line_of(double mx, double my, double sxx, double sxy, float &w, float &b) {
    double wd, bd;
    if (sxx == 0.0) {
        const double c = my / (mx * mx + 1.0);
        wd = c * mx, bd = c;
    } else {
        wd = sxy / sxx, bd = my - wd * mx;
    }
    w = (float)wd, b = (float)bd;
}

__device__ __forceinline__ uint32_t residual_bits(float x, float y, float w, float b) { return __float_as_uint(fabsf(y - (w * x + b))); }

// the sum of one double per lane over the workgroup, in a fixed order; every lane gets it. `red`: PR_THREADS doubles
__device__ __forceinline__ double block_sum(double value, double *red) {
    const uint32_t t = threadIdx.x;
    __syncthreads(); // (the previous use of red is over)
    red[t] = value;
    __syncthreads();
    for (uint32_t half = PR_THREADS / 2; half > 0; half >>= 1) {
        if (t < half) red[t] += red[t + half];
        __syncthreads();
    }
    return red[0];
}

__global__ void __launch_bounds__(PR_THREADS) k_prior_hypotheses(FitArgs a) {
    __shared__ float sx[EGR_PRIOR_MAX_SAMPLE], sy[EGR_PRIOR_MAX_SAMPLE];
    __shared__ uint32_t hist[PR_THREADS], scan[PR_THREADS];
    __shared__ double red[PR_THREADS];
    __shared__ float s_w, s_b;
    __shared__ uint32_t s_digit, s_k;
    const uint32_t it = blockIdx.x, v = blockIdx.y, t = threadIdx.x;
    uint32_t n, S, k;
    view_sizes(a, v, n, S, k);
    if (n < 2 || S < 2) return; // (uniform over the workgroup) the view cannot be fitted: k_prior_select says so
    const float *x = a.pairs_x + (size_t)v * a.pair_stride, *y = a.pairs_y + (size_t)v * a.pair_stride;
    const int32_t *row = a.samples + ((size_t)v * a.num_iters + it) * a.sample_stride;
    for (uint32_t i = t; i < S; i += PR_THREADS) {
        uint32_t j = (uint32_t)row[i];
        j = j < n ? j : n - 1; // (validated on the host; inside the row whatever the device copy holds)
        sx[i] = x[j], sy[i] = y[j];
    }
    __syncthreads();
    if (t == 0) { // S <= 1024 terms from LDS, in sample order
        double mx = 0.0, my = 0.0, sxx = 0.0, sxy = 0.0;
        for (uint32_t i = 0; i < S; i++) mx += (double)sx[i], my += (double)sy[i];
        mx /= (double)S, my /= (double)S;
        for (uint32_t i = 0; i < S; i++) {
            const double dx = (double)sx[i] - mx;
            sxx += dx * dx, sxy += dx * ((double)sy[i] - my);
        }
        float w, b;
        line_of(mx, my, sxx, sxy, w, b);
        s_w = w, s_b = b;
    }
    __syncthreads();
    const float w = s_w, b = s_b;
    // the k-th smallest residual: 8 bits of its pattern per pass, from the top
    uint32_t prefix = 0, rank = k; // the pattern's digits so far; the rank among the residuals that share them
    for (uint32_t pass = 0; pass < 4; pass++) {
        const uint32_t shift = 24 - 8 * pass;
        hist[t] = 0;
        __syncthreads();
        for (uint32_t i = t; i < n; i += PR_THREADS) {
            const uint32_t bits = residual_bits(x[i], y[i], w, b);
            if ((uint32_t)((uint64_t)bits >> (shift + 8)) == prefix) atomicAdd(&hist[(bits >> shift) & 255u], 1u);
        }
        __syncthreads();
        const uint32_t own = hist[t];
        scan[t] = own;
        __syncthreads();
        for (uint32_t off = 1; off < PR_THREADS; off <<= 1) { // inclusive scan of the 256 bins
            const uint32_t add = t >= off ? scan[t - off] : 0u;
            __syncthreads();
            scan[t] += add;
            __syncthreads();
        }
        const uint32_t incl = scan[t], excl = incl - own;
        if (own && excl < rank && rank <= incl) s_digit = t, s_k = rank - excl; // exactly one bin holds the rank (1 <= rank <= the residuals counted)
        __syncthreads();
        prefix = (prefix << 8) | s_digit, rank = s_k;
        __syncthreads();
    }
    // prefix = the threshold's pattern; rank = how many of the residuals equal to it belong to the k smallest
    double sse = 0.0;
    for (uint32_t i = t; i < n; i += PR_THREADS) {
        const uint32_t bits = residual_bits(x[i], y[i], w, b);
        if (bits < prefix) {
            const double r = (double)__uint_as_float(bits);
            sse += r * r;
        }
    }
    sse = block_sum(sse, red);
    if (t == 0) {
        const double thr = (double)__uint_as_float(prefix);
        const size_t h = (size_t)v * a.num_iters + it;
        a.hyp_error[h] = sse + (double)rank * (thr * thr);
        float *model = a.hyp_model + h * 4;
        model[0] = w, model[1] = b, model[2] = __uint_as_float(prefix), model[3] = __uint_as_float(rank);
    }
}

__global__ void __launch_bounds__(PR_THREADS) k_prior_select(FitArgs a) {
    __shared__ double red[PR_THREADS];
    __shared__ uint32_t red_it[PR_THREADS];
    __shared__ uint32_t wave_ties[2][PR_WAVES];
    const uint32_t v = blockIdx.x, t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    uint32_t n, S, k;
    view_sizes(a, v, n, S, k);
    const bool ransac = a.method == EGR_PRIOR_RANSAC;
    if (n < 2 || (ransac && S < 2)) { // (uniform) fewer than 2 pairs: the identity, and no iteration
        if (t == 0) a.ab[2 * v] = 1.0f, a.ab[2 * v + 1] = 0.0f, a.best_iteration[v] = -1, a.best_error[v] = __longlong_as_double(0x7FF8000000000000ll);
        return;
    }
    const float *x = a.pairs_x + (size_t)v * a.pair_stride, *y = a.pairs_y + (size_t)v * a.pair_stride;
    float w = 0.0f, b = 0.0f;
    uint32_t thr = 0, take = 0;
    int32_t best = -1;
    double best_error = __longlong_as_double(0x7FF8000000000000ll);
    if (ransac) {
        // the smallest error, the lowest iteration among equals; a NaN counts as +inf
        const double *err = a.hyp_error + (size_t)v * a.num_iters;
        double e = INFINITY;
        uint32_t at = 0xFFFFFFFFu;
        for (uint32_t i = t; i < a.num_iters; i += PR_THREADS) {
            double c = err[i];
            c = c == c ? c : INFINITY;
            if (c < e || (c == e && i < at)) e = c, at = i;
        }
        red[t] = e, red_it[t] = at;
        __syncthreads();
        for (uint32_t half = PR_THREADS / 2; half > 0; half >>= 1) {
            if (t < half && (red[t + half] < red[t] || (red[t + half] == red[t] && red_it[t + half] < red_it[t]))) red[t] = red[t + half], red_it[t] = red_it[t + half];
            __syncthreads();
        }
        best = (int32_t)red_it[0]; // (< num_iters: iteration 0 ties with the initial +inf and wins by its index)
        best_error = err[best];
        const float *model = a.hyp_model + ((size_t)v * a.num_iters + (uint32_t)best) * 4;
        w = model[0], b = model[1], thr = __float_as_uint(model[2]), take = __float_as_uint(model[3]);
    }
    // two passes over the pairs in order: the means of the inliers (and the mask), then the centred sums
    double mx = 0.0, my = 0.0, sxx = 0.0, sxy = 0.0;
    for (uint32_t pass = 0; pass < 2; pass++) {
        double s0 = 0.0, s1 = 0.0, members = 0.0;
        uint32_t ties_before = 0, flip = 0; // ties in the chunks so far (uniform)
        for (uint32_t first = 0; first < n; first += PR_THREADS, flip ^= 1u) {
            const uint32_t i = first + t;
            bool inlier = i < n, tie = false;
            if (ransac) {
                const uint32_t bits = i < n ? residual_bits(x[i], y[i], w, b) : 0xFFFFFFFFu;
                inlier = i < n && bits < thr, tie = i < n && bits == thr;
                const uint64_t mask = __ballot(tie);
                if (lane == 0) wave_ties[flip][wave] = (uint32_t)__popcll(mask);
                __syncthreads(); // (two buffers: a wave may be one chunk ahead of the slowest reader, never two)
                uint32_t before = ties_before + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), chunk = 0;
#pragma unroll
                for (uint32_t q = 0; q < PR_WAVES; q++) before += q < wave ? wave_ties[flip][q] : 0u, chunk += wave_ties[flip][q];
                if (tie && before < take) inlier = true; // the tie rule: the first `take` pairs at the threshold, in pair order
                ties_before += chunk;
            }
            if (i < n) {
                if (pass == 0 && a.inliers) a.inliers[(size_t)v * a.pair_stride + i] = inlier ? 1 : 0;
                if (inlier) {
                    const double xd = (double)x[i], yd = (double)y[i];
                    if (pass == 0) s0 += xd, s1 += yd, members += 1.0;
                    else s0 += (xd - mx) * (xd - mx), s1 += (xd - mx) * (yd - my);
                }
            }
        }
        s0 = block_sum(s0, red), s1 = block_sum(s1, red);
        if (pass == 0) {
            members = block_sum(members, red); // (exact: integers below 2^32)
            mx = s0 / members, my = s1 / members;
        } else {
            sxx = s0, sxy = s1;
        }
    }
    if (t == 0) {
        float fa, fb;
        line_of(mx, my, sxx, sxy, fa, fb);
        a.ab[2 * v] = fa, a.ab[2 * v + 1] = fb, a.best_iteration[v] = best, a.best_error[v] = best_error;
    }
}

// ---- step 5: distance, world normals, f0
__global__ void __launch_bounds__(PR_THREADS) k_prior_finish(egr_prior_finish_args a) {
    const uint32_t v = blockIdx.y;
    const uint64_t HW = (uint64_t)a.height * a.width, p = (uint64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (p >= HW) return;
    const float *m = a.cams + (size_t)v * PR_CAM, *R = m + PR_R;
    const float fx = m[PR_FX], fy = m[PR_FX + 1], cx = m[PR_FX + 2], cy = m[PR_FX + 3];
    const float sa = a.ab[2 * v], sb = a.ab[2 * v + 1];
    const uint32_t row = (uint32_t)(p / a.width), col = (uint32_t)(p - (uint64_t)row * a.width);
    const size_t px = (size_t)v * HW + p;
    const float Z = a.depth[px * a.depth_channels] * sa + sb;
    const float X = ((float)col - cx) * Z / fx, Y = ((float)row - cy) * Z / fy;
    a.distance[px] = sqrtf((X * X + Y * Y) + Z * Z);
    float nx = -a.normal[3 * px], ny = -a.normal[3 * px + 1], nz = -a.normal[3 * px + 2];
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    nx = nx / len, ny = ny / len, nz = nz / len; // (a zero normal: 0 / 0 = NaN, as upstream)
#pragma unroll
    for (uint32_t r = 0; r < 3; r++) a.normal_out[3 * px + r] = (R[3 * r] * nx + R[3 * r + 1] * ny) + R[3 * r + 2] * nz;
    if (a.metalness) {
        const float metal = a.metalness[px], f0 = 0.04f * (1.0f - metal) + metal;
        a.f0[3 * px] = f0, a.f0[3 * px + 1] = f0, a.f0[3 * px + 2] = f0;
    }
}

thread_local std::string g_prior_error;

bool bad_side(uint32_t s) { return s == 0 || s > PR_MAX_SIDE; }
bool misaligned(const void *p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }
const char *clash_text(const EgrClash &c) { return c.kind == EGR_CLASH_INPUT ? "an output overlaps an input" : "two outputs overlap"; }

} // namespace

extern "C" const char *egr_prior_last_error(void) { return g_prior_error.c_str(); }

extern "C" int egr_prior_pairs(int device, const egr_prior_pairs_args *args, void *hip_stream) {
    const char *fn = "egr_prior_pairs";
    // ---- validation: before any HIP call
    if (!args) return egr_fail(g_prior_error, fn, "args is required");
    const egr_prior_pairs_args a = *args;
    if (!a.cams || !a.offsets || !a.offsets_dev || !a.depth) return egr_fail(g_prior_error, fn, "cams, offsets, offsets_dev and depth are required");
    if (!a.sparse || !a.pairs_x || !a.pairs_y || !a.count || !a.dropped) return egr_fail(g_prior_error, fn, "sparse, pairs_x, pairs_y, count and dropped are required outputs");
    if (bad_side(a.num_views)) return egr_fail(g_prior_error, fn, "num_views must be in 1..65535 per call");
    if (bad_side(a.height) || bad_side(a.width)) return egr_fail(g_prior_error, fn, "image sizes must be in 1..65535");
    if (a.depth_channels != 1 && a.depth_channels != 3) return egr_fail(g_prior_error, fn, "depth_channels must be 1 or 3");
    if (a.offsets[0] != 0) return egr_fail(g_prior_error, fn, "offsets must start at 0");
    uint32_t most = 0;
    for (uint32_t v = 0; v < a.num_views; v++) {
        if (a.offsets[v + 1] < a.offsets[v]) return egr_fail(g_prior_error, fn, "offsets do not ascend at view " + std::to_string(v));
        const uint32_t m = a.offsets[v + 1] - a.offsets[v];
        most = m > most ? m : most;
    }
    const uint32_t total = a.offsets[a.num_views];
    if (total && !a.points) return egr_fail(g_prior_error, fn, "points is required: the offsets count " + std::to_string(total));
    for (const void *p : {(const void *)a.cams, (const void *)a.points, (const void *)a.offsets_dev, (const void *)a.depth, (const void *)a.sparse, (const void *)a.pairs_x,
                          (const void *)a.pairs_y, (const void *)a.count, (const void *)a.dropped})
        if (misaligned(p, 4)) return egr_fail(g_prior_error, fn, "a misaligned array: all hold 4-byte elements");
    const uint64_t V = a.num_views, HW = (uint64_t)a.height * a.width;
    const EgrRange in[4] = {{a.cams, V * PR_CAM * 4}, {a.points, (uint64_t)total * 12}, {a.offsets_dev, (V + 1) * 4}, {a.depth, V * HW * a.depth_channels * 4}};
    const EgrRange out[5] = {{a.sparse, V * HW * 4}, {a.pairs_x, V * HW * 4}, {a.pairs_y, V * HW * 4}, {a.count, V * 4}, {a.dropped, V * 4}};
    if (const EgrClash clash = egr_find_clash(out, 5, in, 4)) return egr_fail(g_prior_error, fn, clash_text(clash));
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_prior_error, fn, [&] {
        EGR_HIP(hipMemsetD32Async((hipDeviceptr_t)a.sparse, (int)PR_INF, (size_t)(V * HW), s));
        if (most) egr_launch(k_prior_project, dim3((most + PR_THREADS - 1) / PR_THREADS, a.num_views), dim3(PR_THREADS), s, a.cams, a.points, a.offsets_dev, total, a.sparse, a.height, a.width);
        egr_launch(k_prior_pairs, dim3(a.num_views), dim3(PR_SCAN_THREADS), s, a.depth, a.depth_channels, (const float *)a.sparse, a.pairs_x, a.pairs_y, a.count, a.dropped, HW);
    });
}

extern "C" int egr_prior_fit(int device, const egr_prior_fit_args *args, void *hip_stream) {
    const char *fn = "egr_prior_fit";
    // ---- validation: before any HIP call
    if (!args) return egr_fail(g_prior_error, fn, "args is required");
    const egr_prior_fit_args a = *args;
    if (!a.pairs_x || !a.pairs_y || !a.views || !a.views_dev) return egr_fail(g_prior_error, fn, "pairs_x, pairs_y, views and views_dev are required");
    if (!a.ab || !a.best_iteration || !a.best_error) return egr_fail(g_prior_error, fn, "ab, best_iteration and best_error are required outputs");
    if (a.method != EGR_PRIOR_RANSAC && a.method != EGR_PRIOR_LSTSQ) return egr_fail(g_prior_error, fn, "unknown method (EGR_PRIOR_RANSAC or EGR_PRIOR_LSTSQ)");
    const bool ransac = a.method == EGR_PRIOR_RANSAC;
    if (bad_side(a.num_views)) return egr_fail(g_prior_error, fn, "num_views must be in 1..65535 per call");
    if (a.pair_stride == 0 || a.pair_stride > PR_MAX_SIDE * PR_MAX_SIDE) return egr_fail(g_prior_error, fn, "pair_stride must be in 1..65535^2");
    if (ransac) {
        if (!a.samples || !a.samples_dev) return egr_fail(g_prior_error, fn, "samples and samples_dev are required");
        if (!a.hyp_error || !a.hyp_model) return egr_fail(g_prior_error, fn, "hyp_error and hyp_model are required outputs");
        if (bad_side(a.num_iters)) return egr_fail(g_prior_error, fn, "num_iters must be in 1..65535");
        if (a.sample_stride == 0 || a.sample_stride > EGR_PRIOR_MAX_SAMPLE) return egr_fail(g_prior_error, fn, "sample_stride must be in 1.." + std::to_string(EGR_PRIOR_MAX_SAMPLE));
    }
    for (uint32_t v = 0; v < a.num_views; v++) {
        const uint32_t n = a.views[4 * v], S = a.views[4 * v + 1], k = a.views[4 * v + 2];
        const std::string view = "view " + std::to_string(v) + ": ";
        if (n > a.pair_stride) return egr_fail(g_prior_error, fn, view + "count " + std::to_string(n) + " exceeds pair_stride");
        if (n < 2) continue; // not fitted: the identity
        if (!ransac) continue;
        if (S < 2 || S > n || S > a.sample_stride) return egr_fail(g_prior_error, fn, view + "sample_size " + std::to_string(S) + " must be in 2..min(count, sample_stride)");
        if (k < 1 || k > n) return egr_fail(g_prior_error, fn, view + "top_k " + std::to_string(k) + " must be in 1..count");
        for (uint32_t it = 0; it < a.num_iters; it++) {
            const int32_t *row = a.samples + ((size_t)v * a.num_iters + it) * a.sample_stride;
            for (uint32_t i = 0; i < S; i++)
                if (row[i] < 0 || (uint32_t)row[i] >= n)
                    return egr_fail(g_prior_error, fn, view + "sample index " + std::to_string(row[i]) + " (iteration " + std::to_string(it) + ") is out of range: the view has " + std::to_string(n) + " pairs");
        }
    }
    for (const void *p : {(const void *)a.pairs_x, (const void *)a.pairs_y, (const void *)a.views_dev, (const void *)a.samples_dev, (const void *)a.hyp_model, (const void *)a.ab,
                          (const void *)a.best_iteration})
        if (misaligned(p, 4)) return egr_fail(g_prior_error, fn, "a misaligned array of 4-byte elements");
    if (misaligned(a.hyp_error, 8) || misaligned(a.best_error, 8)) return egr_fail(g_prior_error, fn, "a misaligned array of doubles");
    const uint64_t V = a.num_views, rows = ransac ? V * a.num_iters : 0;
    const EgrRange in[4] = {{a.pairs_x, V * a.pair_stride * 4}, {a.pairs_y, V * a.pair_stride * 4}, {a.views_dev, V * 16}, {a.samples_dev, rows * a.sample_stride * 4}};
    const EgrRange out[6] = {{a.hyp_error, rows * 8}, {a.hyp_model, rows * 16}, {a.ab, V * 8}, {a.best_iteration, V * 4}, {a.best_error, V * 8}, {a.inliers, V * a.pair_stride}};
    if (const EgrClash clash = egr_find_clash(out, 6, in, 4)) return egr_fail(g_prior_error, fn, clash_text(clash));
    const FitArgs f{a.pairs_x, a.pairs_y, a.views_dev, a.samples_dev, a.hyp_error, a.hyp_model, a.ab, a.best_iteration, a.best_error, a.inliers, a.pair_stride, ransac ? a.num_iters : 0u,
                    ransac ? a.sample_stride : 0u, a.method};
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_prior_error, fn, [&] {
        if (ransac) egr_launch(k_prior_hypotheses, dim3(a.num_iters, a.num_views), dim3(PR_THREADS), s, f);
        egr_launch(k_prior_select, dim3(a.num_views), dim3(PR_THREADS), s, f);
    });
}

extern "C" int egr_prior_finish(int device, const egr_prior_finish_args *args, void *hip_stream) {
    const char *fn = "egr_prior_finish";
    // ---- validation: before any HIP call
    if (!args) return egr_fail(g_prior_error, fn, "args is required");
    const egr_prior_finish_args a = *args;
    if (!a.cams || !a.ab || !a.depth || !a.normal) return egr_fail(g_prior_error, fn, "cams, ab, depth and normal are required");
    if (!a.distance || !a.normal_out) return egr_fail(g_prior_error, fn, "distance and normal_out are required outputs");
    if (a.metalness && !a.f0) return egr_fail(g_prior_error, fn, "f0 is a required output when metalness is given");
    if (bad_side(a.num_views)) return egr_fail(g_prior_error, fn, "num_views must be in 1..65535 per call");
    if (bad_side(a.height) || bad_side(a.width)) return egr_fail(g_prior_error, fn, "image sizes must be in 1..65535");
    if (a.depth_channels != 1 && a.depth_channels != 3) return egr_fail(g_prior_error, fn, "depth_channels must be 1 or 3");
    for (const void *p : {(const void *)a.cams, (const void *)a.ab, (const void *)a.depth, (const void *)a.normal, (const void *)a.metalness, (const void *)a.distance, (const void *)a.normal_out,
                          (const void *)a.f0})
        if (misaligned(p, 4)) return egr_fail(g_prior_error, fn, "a misaligned array: all hold fp32");
    const uint64_t V = a.num_views, HW = (uint64_t)a.height * a.width;
    const EgrRange in[5] = {{a.cams, V * PR_CAM * 4}, {a.ab, V * 8}, {a.depth, V * HW * a.depth_channels * 4}, {a.normal, V * HW * 12}, {a.metalness, V * HW * 4}};
    const EgrRange out[3] = {{a.distance, V * HW * 4}, {a.normal_out, V * HW * 12}, {a.metalness ? a.f0 : nullptr, V * HW * 12}};
    if (const EgrClash clash = egr_find_clash(out, 3, in, 5)) return egr_fail(g_prior_error, fn, clash_text(clash));
    return egr_on_device(device, g_prior_error, fn, [&] {
        egr_launch(k_prior_finish, dim3((uint32_t)((HW + PR_THREADS - 1) / PR_THREADS), a.num_views), dim3(PR_THREADS), (hipStream_t)hip_stream, a);
    });
}
