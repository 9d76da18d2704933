// SPDX-License-Identifier: MIT
// The training views, resident in fp16 (include/egr_raytracer.h: egr_viewset_ingest / egr_viewset_gather): what the reference's Scene / Camera layer does
// per image with torch -
//   the resize       dataset/blender_dataset.py:112-129 _resize_image_tensor   (interpolate(mode="area"), .byte() for 8-bit images)
//   the conversions  scene/cameras.py:59-82 Camera.__init__                    (untonemap(x.half() / 255), x.half() / 255 * 2 - 1, x.half() / 255, seven .half())
//   the depth range  scene/scene.py:107-121 autoadjust_zplanes                 (depth_image.amin() / .amax() per view)
// - as ONE launch per chunk of views that reads the dataset's pixel-major sources once and writes the store's channel-major half planes once, and ONE launch
// per batch that widens the stored views of a batch into the fp32 arrays egr_train_views reads in place. Both are streams: no pow on the device (8-bit values
// go through a 256-entry half table the caller made), 8-bit pixels are fetched as the aligned 32-bit words that hold them, halfs move four or eight at a time.
// tests/viewset_restatement.py is the same arithmetic in numpy.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

namespace {

constexpr uint32_t VS_THREADS = 256;
constexpr uint32_t VS_WAVES = VS_THREADS / 64;
constexpr uint32_t VS_QUAD = 4;          // ingest: consecutive output pixels per lane (one 8-byte store per channel)
constexpr uint32_t VS_OCT = 8;           // gather: halfs per lane (one 16-byte load, two 16-byte stores)
constexpr uint32_t VS_MAX_SIDE = 65535;  // of a source or stored image
constexpr uint64_t VS_MAX_WINDOW = 1ull << 24; // elements of one averaging window: the count is exact in fp32 and 255 * count fits 32 bits
constexpr uint32_t VS_NAN_MIN = 0xFFC00000u, VS_NAN_MAX = 0x7FC00000u; // a NaN as the extreme pattern of each end of the range
constexpr uint32_t VS_POS_INF = 0x7F800000u, VS_NEG_INF = 0xFF800000u;

__host__ __device__ constexpr uint32_t kind_channels(uint32_t kind) { return kind == EGR_VIEWSET_DEPTH || kind == 5 ? 1u : 3u; }

struct IngestArgs {
    egr_viewset_source s[EGR_VIEWSET_KINDS];
    uint32_t V, Hs, Ws, H, W, first_slot;
    float *range;
};

// order-preserving key of an fp32 bit pattern (-0 < +0), and back
__device__ __forceinline__ uint32_t order_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// min / max of fp32 bit patterns with integer atomics on the pattern itself: non-negative patterns order as signed integers, negative ones in reverse as unsigned
// ones, and every negative pattern is above every non-negative one as unsigned. The result does not depend on the order of arrival.
__device__ __forceinline__ void atomic_min_bits(float *p, uint32_t bits) {
    if (bits >> 31) atomicMax((unsigned int *)p, bits);
    else atomicMin((int *)p, (int)bits);
}
__device__ __forceinline__ void atomic_max_bits(float *p, uint32_t bits) {
    if (bits >> 31) atomicMin((unsigned int *)p, bits);
    else atomicMax((int *)p, (int)bits);
}

__global__ void __launch_bounds__(64) k_viewset_range_init(float *range, uint32_t first_slot, uint32_t V) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= 2 * V) return;
    ((uint32_t *)range)[(size_t)first_slot * 2 + i] = (i & 1) ? VS_NEG_INF : VS_POS_INF;
}

// The 32-bit words that hold `count` (<= 3) realigned words of bytes starting at address `at`: words wholly at or past `end` are not loaded (they hold no pixel)
__device__ __forceinline__ void load_realigned(uintptr_t at, uintptr_t end, uint32_t count, uint32_t r[3]) {
    const uintptr_t a = at & ~(uintptr_t)3;
    const uint32_t shift = (uint32_t)(at & 3) * 8;
    uint32_t w[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) w[j] = (j < count + (shift ? 1u : 0u) && a + 4 * j < end) ? *(const uint32_t *)(a + 4 * j) : 0u;
#pragma unroll
    for (uint32_t j = 0; j < 3; j++) r[j] = __builtin_amdgcn_alignbit(w[j + 1], w[j], shift); // (w[j+1] : w[j]) >> shift
}

__global__ void __launch_bounds__(VS_THREADS) k_viewset_ingest(IngestArgs a) {
    __shared__ uint16_t table[256];
    __shared__ uint32_t wave_min[VS_WAVES], wave_max[VS_WAVES], wave_nan[VS_WAVES];
    const uint32_t kind = blockIdx.y, v = blockIdx.z;
    const egr_viewset_source &S = a.s[kind];
    if (!S.data) return; // absent: the planes keep what they hold (uniform over the workgroup)
    const bool u8 = S.dtype == EGR_VIEWSET_U8;
    if (u8) {
        table[threadIdx.x] = ((const uint16_t *)S.table)[threadIdx.x];
        __syncthreads();
    }
    const uint32_t Cs = S.channels, Co = kind_channels(kind);
    const size_t HW = (size_t)a.H * a.W, HWs = (size_t)a.Hs * a.Ws;
    // The 4 pixels of a lane. Without resize they are consecutive (p0 + k): one lane reads 12 consecutive bytes or floats and writes 4 consecutive halfs per channel.
    // A resized fp32 source deals the wave's 256 pixels round-robin (p0 + 64 k): in every step the 64 lanes walk 64 ADJACENT windows, so a wave's loads fall on
    // neighbouring source pixels, and its stores are 64 consecutive halfs (measured at 1080 -> 768, 8 views: 1.04 ms against 2.05 ms with consecutive pixels per
    // lane). A resized 8-bit source is bound by the byte walk, not by its loads, and keeps the consecutive pixels and the 8-byte stores (0.82 against 1.00 ms).
    const bool resize = a.Hs != a.H, dealt = resize && !u8;
    const size_t stride = dealt ? 64 : 1;
    const size_t p0 = dealt ? ((size_t)blockIdx.x * VS_THREADS + (threadIdx.x & ~63u)) * VS_QUAD + (threadIdx.x & 63u) : ((size_t)blockIdx.x * VS_THREADS + threadIdx.x) * VS_QUAD;
    const uint32_t valid = p0 >= HW ? 0u : (uint32_t)((HW - p0 + stride - 1) / stride < VS_QUAD ? (HW - p0 + stride - 1) / stride : VS_QUAD); // (p0 + k * stride < HW for k < valid)
    uint16_t h[VS_QUAD][3] = {};
    if (valid) {
        if (!resize && u8) {
            // 4 pixels = 12 (or 4) consecutive bytes = the 3 (or 1) words that hold them, realigned
            const uintptr_t base = (uintptr_t)S.data, end = base + (size_t)a.V * HWs * Cs;
            uint32_t r[3];
            load_realigned(base + ((size_t)v * HWs + p0) * Cs, end, Cs == 3 ? 3u : 1u, r);
#pragma unroll
            for (uint32_t k = 0; k < VS_QUAD; k++)
#pragma unroll
                for (uint32_t c = 0; c < 3; c++) {
                    const uint32_t i = Cs == 3 ? 3 * k + c : k; // byte of the 12 (or 4)
                    h[k][c] = table[(r[i >> 2] >> ((i & 3) * 8)) & 0xFFu];
                }
        } else if (!resize) {
            const float *src = (const float *)S.data + ((size_t)v * HWs + p0) * Cs;
            if (Cs == 3) {
                float x[12];
                if (valid == VS_QUAD && ((uintptr_t)src & 15u) == 0) {
#pragma unroll
                    for (uint32_t j = 0; j < 3; j++) *(float4 *)(x + 4 * j) = ((const float4 *)src)[j];
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 12; j++) x[j] = j < 3 * valid ? src[j] : 0.0f;
                }
#pragma unroll
                for (uint32_t k = 0; k < VS_QUAD; k++)
#pragma unroll
                    for (uint32_t c = 0; c < 3; c++) h[k][c] = __half_as_ushort(__float2half_rn(x[3 * k + c]));
            } else {
                float x[4];
                if (valid == VS_QUAD && ((uintptr_t)src & 15u) == 0) {
                    *(float4 *)x = *(const float4 *)src;
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < 4; j++) x[j] = j < valid ? src[j] : 0.0f;
                }
#pragma unroll
                for (uint32_t k = 0; k < VS_QUAD; k++) h[k][0] = __half_as_ushort(__float2half_rn(x[k]));
            }
        } else {
            // torch's adaptive average: window i of an axis is [floor(i * src / dst), ceil((i + 1) * src / dst))
#pragma unroll
            for (uint32_t k = 0; k < VS_QUAD; k++) {
                if (k >= valid) break;
                // 32-bit arithmetic throughout: every side is <= 65535, so a pixel index and (i + 1) * src + dst - 1 stay below 2^32
                const uint32_t p = (uint32_t)p0 + k * (uint32_t)stride;
                const uint32_t y = p / a.W, x = p - y * a.W;
                const uint32_t r0 = (y * a.Hs) / a.H, r1 = ((y + 1) * a.Hs + a.H - 1) / a.H;
                const uint32_t c0 = (x * a.Ws) / a.W, c1 = ((x + 1) * a.Ws + a.W - 1) / a.W;
                const uint32_t count = (r1 - r0) * (c1 - c0);
                if (u8) {
                    uint32_t sum[3] = {0u, 0u, 0u}; // integer sums: the order of the terms does not matter
                    for (uint32_t r = r0; r < r1; r++) {
                        // the row of the window is (c1 - c0) * Cs consecutive bytes, taken from the aligned words that hold them
                        uintptr_t at = (uintptr_t)S.data + (((size_t)v * a.Hs + r) * a.Ws + c0) * Cs;
                        const uint32_t n = (c1 - c0) * Cs;
                        uint32_t left = 4 - (uint32_t)(at & 3), ch = 0;
                        at &= ~(uintptr_t)3;
                        uint32_t word = *(const uint32_t *)at >> ((4 - left) * 8);
                        for (uint32_t i = 0; i < n; i++) {
                            if (left == 0) {
                                at += 4;
                                word = *(const uint32_t *)at; // (it holds byte i of the row: inside the array)
                                left = 4;
                            }
                            const uint32_t byte = word & 0xFFu;
                            word >>= 8, left--;
                            sum[0] += ch == 0 ? byte : 0u, sum[1] += ch == 1 ? byte : 0u, sum[2] += ch == 2 ? byte : 0u;
                            ch = ch + 1 == Cs ? 0u : ch + 1;
                        }
                    }
#pragma unroll
                    for (uint32_t c = 0; c < 3; c++) h[k][c] = table[(sum[c] / count) & 0xFFu]; // floor: .float() -> area -> .byte()
                } else {
                    float sum[3] = {0.0f, 0.0f, 0.0f}; // row-major order, from +0
                    const uint32_t used = Co < Cs ? Co : Cs;
                    for (uint32_t r = r0; r < r1; r++) {
                        const float *row = (const float *)S.data + (((size_t)v * a.Hs + r) * a.Ws) * Cs;
                        for (uint32_t c = c0; c < c1; c++)
#pragma unroll
                            for (uint32_t ch = 0; ch < 3; ch++)
                                if (ch < used) sum[ch] += row[(size_t)c * Cs + ch];
                    }
#pragma unroll
                    for (uint32_t c = 0; c < 3; c++) h[k][c] = __half_as_ushort(__float2half_rn(sum[c] / (float)count)); // ONE correctly rounded division
                }
            }
        }
        // channel-major planes: per channel, 4 consecutive halfs as one 8-byte store where the address allows it (dealt pixels: one half per lane and step)
        uint16_t *dst = (uint16_t *)S.planes + (size_t)(a.first_slot + v) * Co * HW + p0;
#pragma unroll
        for (uint32_t c = 0; c < 3; c++) {
            if (c >= Co) break;
            uint16_t *d = dst + (size_t)c * HW;
            if (!dealt && valid == VS_QUAD && ((uintptr_t)d & 7u) == 0) {
                *(uint2 *)d = make_uint2((uint32_t)h[0][c] | ((uint32_t)h[1][c] << 16), (uint32_t)h[2][c] | ((uint32_t)h[3][c] << 16));
            } else {
#pragma unroll
                for (uint32_t k = 0; k < VS_QUAD; k++)
                    if (k < valid) d[k * stride] = h[k][c];
            }
        }
    }
    if (kind != EGR_VIEWSET_DEPTH) return; // (uniform over the workgroup)
    // the range of the STORED halfs: keys per lane, per wave, per workgroup, then one atomic per end
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u, nan = 0u;
#pragma unroll
    for (uint32_t k = 0; k < VS_QUAD; k++)
        if (k < valid) {
            const float f = __half2float(__ushort_as_half(h[k][0]));
            if (f != f) nan = 1u;
            else {
                const uint32_t key = order_key(__float_as_uint(f));
                kmin = key < kmin ? key : kmin, kmax = key > kmax ? key : kmax;
            }
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t omin = __shfl_xor(kmin, off, 64), omax = __shfl_xor(kmax, off, 64), onan = __shfl_xor(nan, off, 64);
        kmin = omin < kmin ? omin : kmin, kmax = omax > kmax ? omax : kmax, nan |= onan;
    }
    const uint32_t wave = threadIdx.x / 64;
    if ((threadIdx.x & 63u) == 0) wave_min[wave] = kmin, wave_max[wave] = kmax, wave_nan[wave] = nan;
    __syncthreads();
    if (threadIdx.x != 0) return;
#pragma unroll
    for (uint32_t w = 1; w < VS_WAVES; w++) {
        kmin = wave_min[w] < kmin ? wave_min[w] : kmin, kmax = wave_max[w] > kmax ? wave_max[w] : kmax, nan |= wave_nan[w];
    }
    float *range = a.range + (size_t)(a.first_slot + v) * 2;
    if (nan) {
        atomicMax((unsigned int *)range, VS_NAN_MIN); // above every number's pattern as unsigned, below every non-negative one as signed: it stays
        atomicMax((int *)(range + 1), (int)VS_NAN_MAX);
    } else if (kmin <= kmax) { // (a workgroup without a pixel contributes nothing)
        atomic_min_bits(range, key_bits(kmin));
        atomic_max_bits(range + 1, key_bits(kmax));
    }
}

struct GatherArgs {
    const uint16_t *planes[EGR_VIEWSET_KINDS];
    float *out[EGR_VIEWSET_KINDS];
    const float *R, *centers, *fovy;
    float *out_R, *out_centers, *out_fovy;
    uint32_t idx[EGR_VIEWSET_MAX_GATHER];
    uint32_t V, first; // views of this launch; their first row in the outputs
    uint64_t HW;
};

__global__ void __launch_bounds__(VS_THREADS) k_viewset_gather(GatherArgs a) {
    const uint32_t kind = blockIdx.y, v = blockIdx.z;
    const uint32_t slot = a.idx[v];
    const size_t row = (size_t)a.first + v;
    if (blockIdx.x == 0 && kind == 0) { // the camera rows of the view: 13 words
        const uint32_t t = threadIdx.x;
        if (t < 9 && a.out_R) a.out_R[row * 9 + t] = a.R[(size_t)slot * 9 + t];
        if (t >= 9 && t < 12 && a.out_centers) a.out_centers[row * 3 + (t - 9)] = a.centers[(size_t)slot * 3 + (t - 9)];
        if (t == 12 && a.out_fovy) a.out_fovy[row] = a.fovy[slot];
    }
    if (!a.out[kind]) return;
    const size_t n = (size_t)kind_channels(kind) * a.HW;
    const size_t i = ((size_t)blockIdx.x * VS_THREADS + threadIdx.x) * VS_OCT;
    if (i >= n) return;
    const uint16_t *src = a.planes[kind] + (size_t)slot * n + i;
    float *dst = a.out[kind] + row * n + i;
    if (n - i >= VS_OCT && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
        const uint4 q = *(const uint4 *)src;
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
        float f[8];
#pragma unroll
        for (uint32_t j = 0; j < 4; j++) {
            f[2 * j] = __half2float(__ushort_as_half((uint16_t)(w[j] & 0xFFFFu))); // exact
            f[2 * j + 1] = __half2float(__ushort_as_half((uint16_t)(w[j] >> 16)));
        }
        ((float4 *)dst)[0] = make_float4(f[0], f[1], f[2], f[3]);
        ((float4 *)dst)[1] = make_float4(f[4], f[5], f[6], f[7]);
    } else {
        const uint32_t m = (uint32_t)(n - i < VS_OCT ? n - i : VS_OCT);
        for (uint32_t j = 0; j < m; j++) dst[j] = __half2float(__ushort_as_half(src[j]));
    }
}

thread_local std::string g_viewset_error;

const char *const KIND_NAMES[EGR_VIEWSET_KINDS] = {"render", "diffuse", "specular", "depth", "normal", "roughness", "f0"};

} // namespace

extern "C" const char *egr_viewset_last_error(void) { return g_viewset_error.c_str(); }

extern "C" int egr_viewset_ingest(int device, const egr_viewset_source *sources, uint32_t num_views, uint32_t src_height, uint32_t src_width, uint32_t height,
                                  uint32_t width, uint32_t first_slot, uint32_t num_slots, float *depth_range, void *hip_stream) {
    const char *fn = "egr_viewset_ingest";
    // ---- validation: before any HIP call
    if (!sources) return egr_fail(g_viewset_error, fn, "the table of sources is required");
    if (!depth_range) return egr_fail(g_viewset_error, fn, "depth_range is a required output");
    if (num_views == 0 || num_views > VS_MAX_SIDE) return egr_fail(g_viewset_error, fn, "num_views must be in 1..65535 per call");
    if (src_height == 0 || src_width == 0 || height == 0 || width == 0 || src_height > VS_MAX_SIDE || src_width > VS_MAX_SIDE || height > VS_MAX_SIDE || width > VS_MAX_SIDE)
        return egr_fail(g_viewset_error, fn, "image sizes must be in 1..65535");
    if (src_height != height) {
        const uint32_t want = (uint32_t)((double)height * ((double)src_width / (double)src_height)); // _resize_image_tensor's int(resolution * aspect_ratio)
        if (width != want) return egr_fail(g_viewset_error, fn, "size mismatch: a resized source must give the store's width, int(height * (src_width / src_height)) = " + std::to_string(want));
        const uint64_t wh = (src_height + height - 1) / height + 1, ww = (src_width + width - 1) / width + 1;
        if (wh * ww > VS_MAX_WINDOW) return egr_fail(g_viewset_error, fn, "an averaging window of more than 2^24 elements");
    } else if (src_width != width) {
        return egr_fail(g_viewset_error, fn, "size mismatch: a source of the store's height must have the store's width");
    }
    if ((uint64_t)first_slot + num_views > num_slots) return egr_fail(g_viewset_error, fn, "first_slot + num_views exceeds num_slots");
    IngestArgs a{};
    EgrRange in[2 * EGR_VIEWSET_KINDS], out[EGR_VIEWSET_KINDS + 1];
    int nin = 0, nout = 0;
    const size_t HW = (size_t)height * width, HWs = (size_t)src_height * src_width;
    for (uint32_t k = 0; k < EGR_VIEWSET_KINDS; k++) {
        const egr_viewset_source &S = sources[k];
        if (!S.data) continue;
        const std::string name = KIND_NAMES[k];
        if (S.channels != 1 && S.channels != 3) return egr_fail(g_viewset_error, fn, name + ": channels must be 1 or 3");
        if (S.channels == 1 && kind_channels(k) == 3) return egr_fail(g_viewset_error, fn, name + ": a colour kind needs 3 channels");
        if (S.dtype != EGR_VIEWSET_U8 && S.dtype != EGR_VIEWSET_F32) return egr_fail(g_viewset_error, fn, name + ": unknown dtype (EGR_VIEWSET_U8 or EGR_VIEWSET_F32)");
        if (S.dtype == EGR_VIEWSET_U8 && k == EGR_VIEWSET_DEPTH) return egr_fail(g_viewset_error, fn, "uint8 depth is refused (the reference asserts the same)");
        if (S.dtype == EGR_VIEWSET_U8 && !S.table) return egr_fail(g_viewset_error, fn, name + ": a uint8 source needs its table of 256 halfs");
        if (S.dtype == EGR_VIEWSET_F32 && S.table) return egr_fail(g_viewset_error, fn, name + ": a table was given for an fp32 source");
        if (!S.planes) return egr_fail(g_viewset_error, fn, name + ": present data without planes");
        if (S.dtype == EGR_VIEWSET_F32 && ((uintptr_t)S.data & 3u)) return egr_fail(g_viewset_error, fn, name + ": an fp32 source must be 4-byte aligned");
        if (((uintptr_t)S.planes & 1u) || (S.table && ((uintptr_t)S.table & 1u))) return egr_fail(g_viewset_error, fn, name + ": planes and table must be 2-byte aligned");
        in[nin++] = EgrRange{S.data, (size_t)num_views * HWs * S.channels * (S.dtype == EGR_VIEWSET_U8 ? 1 : 4)};
        if (S.table) in[nin++] = EgrRange{S.table, 512};
        out[nout++] = EgrRange{(const uint16_t *)S.planes + (size_t)first_slot * kind_channels(k) * HW, (size_t)num_views * kind_channels(k) * HW * 2};
        a.s[k] = S;
    }
    if (nout == 0) return egr_fail(g_viewset_error, fn, "every kind is absent");
    out[nout++] = EgrRange{depth_range + (size_t)first_slot * 2, (size_t)num_views * 8};
    if (const EgrClash clash = egr_find_clash(out, nout, in, nin))
        return egr_fail(g_viewset_error, fn, clash.kind == EGR_CLASH_INPUT ? "an output (planes or depth_range rows) overlaps an input (data or table)" : "two outputs overlap");
    a.V = num_views, a.Hs = src_height, a.Ws = src_width, a.H = height, a.W = width, a.first_slot = first_slot, a.range = depth_range;
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_viewset_error, fn, [&] {
        if (a.s[EGR_VIEWSET_DEPTH].data) egr_launch(k_viewset_range_init, dim3((2 * num_views + 63) / 64), dim3(64), s, depth_range, first_slot, num_views);
        const size_t quads = (HW + VS_QUAD - 1) / VS_QUAD;
        egr_launch(k_viewset_ingest, dim3((uint32_t)((quads + VS_THREADS - 1) / VS_THREADS), EGR_VIEWSET_KINDS, num_views), dim3(VS_THREADS), s, a);
    });
}

extern "C" int egr_viewset_gather(int device, const egr_viewset_store *store, const uint32_t *indices, uint32_t num_views, const egr_viewset_batch *out,
                                  void *hip_stream) {
    const char *fn = "egr_viewset_gather";
    // ---- validation: before any HIP call
    if (!store || !out || !indices) return egr_fail(g_viewset_error, fn, "store, indices and out are required");
    if (num_views == 0) return egr_fail(g_viewset_error, fn, "num_views is 0");
    if (store->height == 0 || store->width == 0 || store->height > VS_MAX_SIDE || store->width > VS_MAX_SIDE) return egr_fail(g_viewset_error, fn, "image sizes must be in 1..65535");
    if (store->num_filled > store->num_slots) return egr_fail(g_viewset_error, fn, "num_filled exceeds num_slots");
    for (uint32_t v = 0; v < num_views; v++)
        if (indices[v] >= store->num_filled) return egr_fail(g_viewset_error, fn, "index " + std::to_string(indices[v]) + " (entry " + std::to_string(v) + ") is out of range: " + std::to_string(store->num_filled) + " slots are filled");
    const size_t HW = (size_t)store->height * store->width;
    EgrRange in[EGR_VIEWSET_KINDS + 3], o[EGR_VIEWSET_KINDS + 3];
    int nin = 0, nout = 0;
    uint32_t cmax = 0;
    for (uint32_t k = 0; k < EGR_VIEWSET_KINDS; k++) {
        if (!out->targets[k]) continue;
        if (!store->planes[k]) return egr_fail(g_viewset_error, fn, std::string(KIND_NAMES[k]) + ": wanted, but the store has no planes of it");
        if (((uintptr_t)out->targets[k] & 3u) || ((uintptr_t)store->planes[k] & 1u)) return egr_fail(g_viewset_error, fn, std::string(KIND_NAMES[k]) + ": misaligned planes or output");
        in[nin++] = EgrRange{store->planes[k], (size_t)store->num_slots * kind_channels(k) * HW * 2};
        o[nout++] = EgrRange{out->targets[k], (size_t)num_views * kind_channels(k) * HW * 4};
        cmax = cmax > kind_channels(k) ? cmax : kind_channels(k);
    }
    const struct { float *dst; const float *src; uint32_t width; const char *name; } rows[3] = {{out->R, store->R, 9, "R"}, {out->centers, store->centers, 3, "centers"}, {out->fovy, store->fovy, 1, "fovy"}};
    for (const auto &r : rows) {
        if (!r.dst) continue;
        if (!r.src) return egr_fail(g_viewset_error, fn, std::string(r.name) + ": wanted, but the store has no such array");
        if (((uintptr_t)r.dst & 3u) || ((uintptr_t)r.src & 3u)) return egr_fail(g_viewset_error, fn, std::string(r.name) + ": misaligned array");
        in[nin++] = EgrRange{r.src, (size_t)store->num_slots * r.width * 4};
        o[nout++] = EgrRange{r.dst, (size_t)num_views * r.width * 4};
    }
    if (nout == 0) return egr_fail(g_viewset_error, fn, "nothing is wanted: every output is NULL");
    if (const EgrClash clash = egr_find_clash(o, nout, in, nin))
        return egr_fail(g_viewset_error, fn, clash.kind == EGR_CLASH_INPUT ? "an output overlaps the store (an input)" : "two outputs overlap");
    return egr_on_device(device, g_viewset_error, fn, [&] {
        for (uint32_t v0 = 0; v0 < num_views; v0 += EGR_VIEWSET_MAX_GATHER) {
            GatherArgs a{};
            for (uint32_t k = 0; k < EGR_VIEWSET_KINDS; k++) a.planes[k] = (const uint16_t *)store->planes[k], a.out[k] = out->targets[k];
            a.R = store->R, a.centers = store->centers, a.fovy = store->fovy, a.out_R = out->R, a.out_centers = out->centers, a.out_fovy = out->fovy;
            a.V = num_views - v0 < EGR_VIEWSET_MAX_GATHER ? num_views - v0 : EGR_VIEWSET_MAX_GATHER, a.first = v0, a.HW = HW;
            for (uint32_t v = 0; v < a.V; v++) a.idx[v] = indices[v0 + v];
            const size_t octs = cmax ? ((size_t)cmax * HW + VS_OCT - 1) / VS_OCT : 1;
            egr_launch(k_viewset_gather, dim3((uint32_t)((octs + VS_THREADS - 1) / VS_THREADS), EGR_VIEWSET_KINDS, a.V), dim3(VS_THREADS), (hipStream_t)hip_stream, a);
        }
    });
}
