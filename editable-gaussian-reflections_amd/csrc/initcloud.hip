// SPDX-License-Identifier: MIT
// The dense-init cloud (include/egr_raytracer.h: egr_voxel_accumulate / egr_voxel_rehash / egr_voxel_extract): what the reference's prepare_initial_ply.py does
// on the CPU with every pixel of every training view in memory -
//   the unprojection   prepare_initial_ply.py:57-69 + utils/depth_utils.py:28-63   pos = origin + normalised(cam @ c2w^T) * depth, in fp64
//   the voxel grid     prepare_initial_ply.py:83-86                                (pos * voxel_scale).round().int(), torch.unique(dim=0, inverse, counts)
//   the average        prepare_initial_ply.py:89-93                                index_add_ of the colours, / counts
//   the selection      prepare_initial_ply.py:98-104                               counts >= 2, coords.float() / voxel_scale
// - as a streamed scatter-reduce into an open-addressing hash table that the caller owns. Memory is that of the table, not of the pixels.
//
//   k_voxel_accumulate  grid (W / 16, H / 16, V), one pixel per thread. The 256 pixels of a 16 x 16 tile are first combined in an LDS table of 512 slots
//                       (64-bit LDS compare-and-swap on the key, four 64-bit LDS adds); then every occupied LDS slot goes to the global table once:
//                       64-bit compare-and-swap on the key, four 64-bit integer adds on its record. Probing is bounded by the capacity on both levels.
//   k_voxel_rehash      one thread per slot of the old table, the same claim-and-add into the new one.
//   k_voxel_compact     slots with count >= min_count -> (key, slot) pairs through a wave-aggregated append (the waves of a workgroup meet in LDS: one global
//                       atomic per 2048 slots); the largest count of the table.
//   rocprim::radix_sort_pairs on the packed keys: the slot order depends on timing, the sorted order on the inputs alone.
//   k_voxel_write       coords, points, colours and counts of the sorted pairs in one pass.
// The colour sums are 2^-32 fixed point in int64: integer addition is associative, so the table's CONTENT is a function of the set of pixels - whatever the
// order of the views, the chunking, the capacity, the growth or the timing. No float atomics anywhere.
#include <hip/hip_runtime.h>
#include <string.h>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/egr_raytracer.h"
#include "egr_host.hpp"

namespace {

typedef unsigned long long ull;
constexpr ull VOXEL_EMPTY = ~0ull;                 // int64 -1: no key has the top bit set
constexpr uint32_t VOXEL_THREADS = 256;            // 4 waves
constexpr uint32_t VOXEL_TILE = 16;                // a workgroup's image tile is 16 x 16 pixels
constexpr uint32_t VOXEL_LDS_SLOTS = 512;          // twice the pixels of a tile: an LDS insert always finds a slot
constexpr uint32_t VOXEL_COMPACT_ITEMS = 8;        // slots per thread and pass of the compaction
constexpr uint32_t VOXEL_COMPACT_CHUNK = VOXEL_COMPACT_ITEMS * VOXEL_THREADS; // 2048 slots per workgroup and pass
constexpr double VOXEL_FIX = 4294967296.0;         // 2^32: one colour unit in the fixed-point sums
constexpr int64_t VOXEL_HALF = (int64_t)EGR_VOXEL_COORD_HALF_RANGE;
static_assert(VOXEL_TILE * VOXEL_TILE == VOXEL_THREADS && VOXEL_LDS_SLOTS == 2 * VOXEL_THREADS, "one pixel per thread, two LDS slots per thread");
static_assert(EGR_VOXEL_COORD_HALF_RANGE == (1 << 20), "the key packs three 21-bit fields");

struct AccArgs {
    ull *keys;                 // [cap]
    ull *acc;                  // [cap][4]: count, three colour sums (two's complement)
    ull *status;               // [EGR_VOXEL_STATUS_WORDS]
    uint64_t cap;
    const double *c2w;         // [V][9] row-major
    const double *origin;      // [V][3]
    const double *view_size;   // [V]
    const float *depth;        // [V][H][W]
    const float *colour;       // [V][H][W][3] or NULL
    const uint8_t *colour_u8;  // [V][H][W][3] or NULL
    const float *table;        // [256] with colour_u8
    double *positions_out;     // [V][H][W][3] or NULL
    double voxel_scale, colour_max;
    uint32_t V, H, W;
};

__device__ __forceinline__ uint64_t mix64(uint64_t x) { // the finaliser of splitmix64
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

// Claim-and-add into the global table. At most `cap` probes, every slot index is masked by cap - 1 (cap is a power of two): never outside the table, never
// endless. Returns false when every slot holds another key. `claimed`: this call took an empty slot.
__device__ __forceinline__ bool voxel_insert(ull *keys, ull *acc, uint64_t cap, ull key, ull count, ull s0, ull s1, ull s2, bool &claimed) {
    const uint64_t mask = cap - 1;
    uint64_t slot = mix64(key) & mask;
    for (uint64_t probe = 0; probe < cap; probe++, slot = (slot + 1) & mask) {
        ull cur = __hip_atomic_load(&keys[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // (a key never changes once set: a stale EMPTY only costs the swap below)
        if (cur == VOXEL_EMPTY) {
            cur = atomicCAS(&keys[slot], VOXEL_EMPTY, key);
            if (cur == VOXEL_EMPTY) claimed = true, cur = key;
        }
        if (cur == key) {
            ull *r = acc + slot * 4;
            atomicAdd(r, count), atomicAdd(r + 1, s0), atomicAdd(r + 2, s1), atomicAdd(r + 3, s2);
            return true;
        }
    }
    return false;
}

__device__ __forceinline__ bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e308; } // false for NaN and +-inf

__global__ void __launch_bounds__(VOXEL_THREADS) k_voxel_accumulate(AccArgs a) {
#pragma clang fp contract(off) // every product and sum rounded on its own, as numpy and torch evaluate them
    __shared__ ull s_keys[VOXEL_LDS_SLOTS];
    __shared__ ull s_acc[VOXEL_LDS_SLOTS][4];
    __shared__ uint32_t s_stat[4]; // claimed slots, pixels added, pixels dropped, pixels that found no slot
    const uint32_t tid = threadIdx.x, v = blockIdx.z;
    const uint32_t x = blockIdx.x * VOXEL_TILE + (tid & (VOXEL_TILE - 1)), y = blockIdx.y * VOXEL_TILE + tid / VOXEL_TILE;
    for (uint32_t s = tid; s < VOXEL_LDS_SLOTS; s += VOXEL_THREADS) {
        s_keys[s] = VOXEL_EMPTY;
        s_acc[s][0] = s_acc[s][1] = s_acc[s][2] = s_acc[s][3] = 0;
    }
    if (tid < 4) s_stat[tid] = 0;
    __syncthreads();
    if (x < a.W && y < a.H) { // every read and write below is of pixel (v, y, x) < (V, H, W)
        const uint64_t pixel = ((uint64_t)v * a.H + y) * a.W + x;
        const double *R = a.c2w + (size_t)v * 9, *O = a.origin + (size_t)v * 3;
        const double view_size = a.view_size[v], aspect = (double)a.W / (double)a.H;
        const double pu = ((double)x + 0.5) / (double)a.W, pv = ((double)y + 0.5) / (double)a.H;
        const double cx = (aspect * view_size) * (2.0 * pu - 1.0), cy = view_size * (1.0 - 2.0 * pv), cz = -1.0;
        double dx = cx * R[0] + cy * R[1] + cz * R[2], dy = cx * R[3] + cy * R[4] + cz * R[5], dz = cx * R[6] + cy * R[7] + cz * R[8]; // cam @ c2w^T
        const double norm = sqrt(dx * dx + dy * dy + dz * dz);
        dx = dx / norm, dy = dy / norm, dz = dz / norm;
        const double depth = (double)a.depth[pixel];
        const double px = O[0] + dx * depth, py = O[1] + dy * depth, pz = O[2] + dz * depth;
        if (a.positions_out) {
            double *o = a.positions_out + pixel * 3;
            o[0] = px, o[1] = py, o[2] = pz;
        }
        float c[3];
        if (a.colour) {
            c[0] = a.colour[pixel * 3], c[1] = a.colour[pixel * 3 + 1], c[2] = a.colour[pixel * 3 + 2];
        } else {
            c[0] = a.table[a.colour_u8[pixel * 3]], c[1] = a.table[a.colour_u8[pixel * 3 + 1]], c[2] = a.table[a.colour_u8[pixel * 3 + 2]];
        }
        const double rx = rint(px * a.voxel_scale), ry = rint(py * a.voxel_scale), rz = rint(pz * a.voxel_scale); // round half to even, as torch.round
        const double lo = -(double)VOXEL_HALF, hi = (double)VOXEL_HALF;
        bool ok = finite_d(depth) && rx >= lo && rx < hi && ry >= lo && ry < hi && rz >= lo && rz < hi; // (a NaN fails every comparison)
#pragma unroll
        for (int k = 0; k < 3; k++) ok = ok && fabs((double)c[k]) <= a.colour_max;                      // (and so does a NaN colour)
        if (!ok) {
            atomicAdd(&s_stat[2], 1u);
        } else {
            atomicAdd(&s_stat[1], 1u);
            const ull key = ((ull)((int64_t)rx + VOXEL_HALF) << 42) | ((ull)((int64_t)ry + VOXEL_HALF) << 21) | (ull)((int64_t)rz + VOXEL_HALF);
            const ull q0 = (ull)llrint((double)c[0] * VOXEL_FIX), q1 = (ull)llrint((double)c[1] * VOXEL_FIX), q2 = (ull)llrint((double)c[2] * VOXEL_FIX);
            uint32_t slot = (uint32_t)mix64(key) & (VOXEL_LDS_SLOTS - 1);
            for (uint32_t probe = 0; probe < VOXEL_LDS_SLOTS; probe++, slot = (slot + 1) & (VOXEL_LDS_SLOTS - 1)) { // at most 256 keys in 512 slots: always ends in a hit
                const ull cur = atomicCAS(&s_keys[slot], VOXEL_EMPTY, key);
                if (cur == VOXEL_EMPTY || cur == key) {
                    atomicAdd(&s_acc[slot][0], 1ull), atomicAdd(&s_acc[slot][1], q0), atomicAdd(&s_acc[slot][2], q1), atomicAdd(&s_acc[slot][3], q2);
                    break;
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t s = tid; s < VOXEL_LDS_SLOTS; s += VOXEL_THREADS) { // one global claim-and-add per distinct key of the tile
        const ull key = s_keys[s];
        if (key == VOXEL_EMPTY) continue;
        bool claimed = false;
        if (!voxel_insert(a.keys, a.acc, a.cap, key, s_acc[s][0], s_acc[s][1], s_acc[s][2], s_acc[s][3], claimed)) atomicAdd(&s_stat[3], (uint32_t)s_acc[s][0]);
        if (claimed) atomicAdd(&s_stat[0], 1u);
    }
    __syncthreads();
    if (tid < 4 && s_stat[tid] != 0) atomicAdd(&a.status[tid], (ull)s_stat[tid]);
}

struct RehashArgs {
    ull *keys, *acc, *status;
    uint64_t cap;
    const ull *src_keys, *src_acc;
    uint64_t src_cap;
};

__global__ void __launch_bounds__(VOXEL_THREADS) k_voxel_rehash(RehashArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * VOXEL_THREADS + threadIdx.x; // the grid covers src_cap exactly (a multiple of 256)
    bool claimed = false, lost = false;
    ull count = 0;
    if (i < a.src_cap) {
        const ull key = a.src_keys[i];
        if (key != VOXEL_EMPTY) {
            const ull *r = a.src_acc + i * 4;
            count = r[0];
            lost = !voxel_insert(a.keys, a.acc, a.cap, key, count, r[1], r[2], r[3], claimed);
        }
    }
    const uint64_t ballot = __ballot(claimed);
    if ((threadIdx.x & 63u) == 0 && ballot) atomicAdd(&a.status[0], (ull)__popcll(ballot));
    if (lost) atomicAdd(&a.status[3], count); // (never, unless the caller made the new table too small)
}

struct ExtractArgs {
    const ull *keys, *acc;
    ull *status;
    uint64_t cap, max_rows, n;
    ull *pair_keys[2];      // [max_rows] each: unsorted, sorted
    uint32_t *pair_slots[2];
    int32_t *coords;        // [n][3]
    float *points, *colors; // [n][3]
    int32_t *counts;        // [n]
    uint32_t min_count;
    float voxel_scale;
};

// A workgroup takes VOXEL_COMPACT_CHUNK consecutive slots per pass and appends its kept rows with ONE global atomic: the waves meet in LDS first. (One atomic per
// wave and 64 slots - 524 288 returning atomics on one address for 2^25 slots - made this launch 6.4 ms, most of the extraction; same-address atomics serialise.)
__global__ void __launch_bounds__(VOXEL_THREADS) k_voxel_compact(ExtractArgs a) {
    __shared__ uint32_t s_kept;
    __shared__ ull s_first;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    ull largest = 0;
    if (tid == 0) s_first = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * VOXEL_COMPACT_CHUNK; base < a.cap; base += (uint64_t)gridDim.x * VOXEL_COMPACT_CHUNK) { // (uniform per workgroup)
        if (tid == 0) s_kept = 0;
        __syncthreads();
        ull key[VOXEL_COMPACT_ITEMS];
        uint64_t ballot[VOXEL_COMPACT_ITEMS];
        uint32_t wave_kept = 0;
#pragma unroll
        for (uint32_t k = 0; k < VOXEL_COMPACT_ITEMS; k++) {
            const uint64_t i = base + (uint64_t)k * VOXEL_THREADS + tid;
            const bool in = i < a.cap; // (uniform per wave: cap is a multiple of 256)
            key[k] = in ? a.keys[i] : VOXEL_EMPTY;
            const ull count = key[k] != VOXEL_EMPTY ? a.acc[i * 4] : 0ull;
            largest = count > largest ? count : largest;
            ballot[k] = __ballot(key[k] != VOXEL_EMPTY && count >= a.min_count);
            wave_kept += (uint32_t)__popcll(ballot[k]);
        }
        uint32_t wave_first = 0;
        if (lane == 0 && wave_kept) wave_first = atomicAdd(&s_kept, wave_kept);
        wave_first = __shfl(wave_first, 0, 64);
        __syncthreads();
        if (tid == 0 && s_kept) s_first = atomicAdd(&a.status[5], (ull)s_kept); // one append per workgroup and pass
        __syncthreads();
        ull row = s_first + wave_first;
#pragma unroll
        for (uint32_t k = 0; k < VOXEL_COMPACT_ITEMS; k++) {
            if ((ballot[k] >> lane) & 1ull) { // (only slots < cap are ever set)
                const ull r = row + (ull)__popcll(ballot[k] & ((1ull << lane) - 1ull));
                if (r < a.max_rows) a.pair_keys[0][r] = key[k], a.pair_slots[0][r] = (uint32_t)(base + (uint64_t)k * VOXEL_THREADS + tid); // rows beyond max_rows are counted, not written
            }
            row += (ull)__popcll(ballot[k]);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const ull other = __shfl_down(largest, d, 64);
        largest = other > largest ? other : largest;
    }
    if ((threadIdx.x & 63u) == 0 && largest) atomicMax(&a.status[4], largest);
}

__global__ void __launch_bounds__(VOXEL_THREADS) k_voxel_write(ExtractArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * VOXEL_THREADS + threadIdx.x;
    if (i >= a.n) return;
    const ull key = a.pair_keys[1][i];
    const ull *r = a.acc + (uint64_t)a.pair_slots[1][i] * 4; // a slot index the compaction wrote: < cap
    const int32_t c[3] = {(int32_t)((int64_t)(key >> 42) - VOXEL_HALF), (int32_t)((int64_t)((key >> 21) & 0x1FFFFFull) - VOXEL_HALF), (int32_t)((int64_t)(key & 0x1FFFFFull) - VOXEL_HALF)};
    const ull count = r[0];
    const double denom = (double)count * VOXEL_FIX;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.coords[i * 3 + k] = c[k];
        a.points[i * 3 + k] = __fdiv_rn((float)c[k], a.voxel_scale);           // an IEEE fp32 division, as coords.float() / voxel_scale
        a.colors[i * 3 + k] = (float)((double)(int64_t)r[1 + k] / denom);
    }
    a.counts[i] = count > 0x7FFFFFFFull ? 0x7FFFFFFF : (int32_t)count;
}

thread_local std::string g_voxel_error;

bool bad_cap(uint64_t cap) { return cap < EGR_VOXEL_MIN_CAPACITY || cap > EGR_VOXEL_MAX_CAPACITY || (cap & (cap - 1)) != 0; }
bool misaligned(const void *p) { return ((uintptr_t)p & 7u) != 0; }
const char *CAP_TEXT = "the capacity must be a power of two in EGR_VOXEL_MIN_CAPACITY..EGR_VOXEL_MAX_CAPACITY";

uint64_t pair_bytes(uint64_t max_rows) { return EGR_VOXEL_PAIR_BYTES(max_rows); }

} // namespace

extern "C" const char *egr_voxel_last_error(void) { return g_voxel_error.c_str(); }

extern "C" int egr_voxel_accumulate(int device, int64_t *keys, int64_t *acc, int64_t *status, uint64_t cap, uint32_t num_views, uint32_t height, uint32_t width,
                                    const double *c2w, const double *origin, const double *view_size, const float *depth, const float *colour,
                                    const uint8_t *colour_u8, const float *colour_table, double voxel_scale, double colour_max, double *positions_out,
                                    void *hip_stream) {
    const char *fn = "egr_voxel_accumulate";
    // ---- validation: before any HIP call
    if (!keys || !acc || !status) return egr_fail(g_voxel_error, fn, "keys, acc and status are required");
    if (misaligned(keys) || misaligned(acc) || misaligned(status) || misaligned(c2w) || misaligned(origin) || misaligned(view_size) || misaligned(positions_out))
        return egr_fail(g_voxel_error, fn, "the table and the fp64 arrays must be 8-byte aligned");
    if (bad_cap(cap)) return egr_fail(g_voxel_error, fn, CAP_TEXT);
    if (num_views == 0 || num_views > 65535u) return egr_fail(g_voxel_error, fn, "num_views must be in 1..65535");
    if (height == 0 || width == 0 || height > (1u << 20) || width > (1u << 20)) return egr_fail(g_voxel_error, fn, "height and width must be in 1..2^20");
    if (!c2w || !origin || !view_size || !depth) return egr_fail(g_voxel_error, fn, "c2w, origin, view_size and depth are required");
    if ((colour != nullptr) == (colour_u8 != nullptr)) return egr_fail(g_voxel_error, fn, "exactly one of colour (fp32) and colour_u8 is required");
    if (colour_u8 && !colour_table) return egr_fail(g_voxel_error, fn, "colour_u8 needs the 256-entry colour_table");
    if (!(voxel_scale > 0.0) || !std::isfinite(voxel_scale)) return egr_fail(g_voxel_error, fn, "voxel_scale must be positive and finite");
    if (!(colour_max > 0.0) || !(colour_max <= 1073741824.0)) return egr_fail(g_voxel_error, fn, "colour_max must be in (0, 2^30]");
    const uint64_t pixels = (uint64_t)num_views * height * width;
    if (pixels >= (1ull << 40)) return egr_fail(g_voxel_error, fn, "more than 2^40 pixels in one call");
    const EgrRange out[4] = {{keys, cap * 8}, {acc, cap * 32}, {status, EGR_VOXEL_STATUS_WORDS * 8}, {positions_out, pixels * 24}};
    const EgrRange in[7] = {{c2w, (uint64_t)num_views * 72}, {origin, (uint64_t)num_views * 24}, {view_size, (uint64_t)num_views * 8}, {depth, pixels * 4},
                         {colour, pixels * 12}, {colour_u8, pixels * 3}, {colour_table, colour_u8 ? 1024u : 0u}};
    if (egr_find_clash(out, 4, in, 7)) return egr_fail(g_voxel_error, fn, "the table, status or positions_out overlaps an input or another output");
    AccArgs a{};
    a.keys = (ull *)keys, a.acc = (ull *)acc, a.status = (ull *)status, a.cap = cap;
    a.c2w = c2w, a.origin = origin, a.view_size = view_size, a.depth = depth, a.colour = colour, a.colour_u8 = colour_u8, a.table = colour_table;
    a.positions_out = positions_out, a.voxel_scale = voxel_scale, a.colour_max = colour_max;
    a.V = num_views, a.H = height, a.W = width;
    const dim3 grid((width + VOXEL_TILE - 1) / VOXEL_TILE, (height + VOXEL_TILE - 1) / VOXEL_TILE, num_views); // <= 65536 x 65536 x 65535
    return egr_on_device(device, g_voxel_error, fn, [&] { egr_launch(k_voxel_accumulate, grid, dim3(VOXEL_THREADS), (hipStream_t)hip_stream, a); });
}

extern "C" int egr_voxel_rehash(int device, int64_t *keys, int64_t *acc, int64_t *status, uint64_t cap, const int64_t *src_keys, const int64_t *src_acc,
                                uint64_t src_cap, void *hip_stream) {
    const char *fn = "egr_voxel_rehash";
    // ---- validation: before any HIP call
    if (!keys || !acc || !status || !src_keys || !src_acc) return egr_fail(g_voxel_error, fn, "keys, acc, status, src_keys and src_acc are required");
    if (misaligned(keys) || misaligned(acc) || misaligned(status) || misaligned(src_keys) || misaligned(src_acc)) return egr_fail(g_voxel_error, fn, "the tables must be 8-byte aligned");
    if (bad_cap(cap) || bad_cap(src_cap)) return egr_fail(g_voxel_error, fn, CAP_TEXT);
    const EgrRange out[3] = {{keys, cap * 8}, {acc, cap * 32}, {status, EGR_VOXEL_STATUS_WORDS * 8}};
    const EgrRange in[2] = {{src_keys, src_cap * 8}, {src_acc, src_cap * 32}};
    if (egr_find_clash(out, 3, in, 2)) return egr_fail(g_voxel_error, fn, "the new table or status overlaps the old table or another output: a rehash runs out of place");
    RehashArgs a{(ull *)keys, (ull *)acc, (ull *)status, cap, (const ull *)src_keys, (const ull *)src_acc, src_cap};
    return egr_on_device(device, g_voxel_error, fn, [&] { egr_launch(k_voxel_rehash, dim3((uint32_t)(src_cap / VOXEL_THREADS)), dim3(VOXEL_THREADS), (hipStream_t)hip_stream, a); });
}

extern "C" size_t egr_voxel_extract_workspace_bytes(int device, uint64_t max_rows) {
    const char *fn = "egr_voxel_extract_workspace_bytes";
    if (max_rows == 0 || max_rows > EGR_VOXEL_MAX_CAPACITY) {
        egr_fail(g_voxel_error, fn, "max_rows must be in 1..EGR_VOXEL_MAX_CAPACITY");
        return 0; // (a size, not a status: 0 is the failure)
    }
    size_t bytes = 0;
    const int rc = egr_on_device(device, g_voxel_error, fn, [&] {
        EGR_HIP(rocprim::radix_sort_pairs(nullptr, bytes, (ull *)nullptr, (ull *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)max_rows, 0, 63, 0));
    });
    return rc ? 0 : (size_t)pair_bytes(max_rows) + ((bytes + 15) & ~(size_t)15) + 16;
}

extern "C" int egr_voxel_extract(int device, const int64_t *keys, const int64_t *acc, int64_t *status, uint64_t cap, uint32_t min_count, double voxel_scale,
                                 uint64_t max_rows, int32_t *coords, float *points, float *colors, int32_t *counts, uint64_t *host_rows_and_largest,
                                 void *workspace, size_t workspace_bytes, void *hip_stream) {
    const char *fn = "egr_voxel_extract";
    // ---- validation: before any HIP call
    if (!keys || !acc || !status) return egr_fail(g_voxel_error, fn, "keys, acc and status are required");
    if (misaligned(keys) || misaligned(acc) || misaligned(status)) return egr_fail(g_voxel_error, fn, "the table must be 8-byte aligned");
    if (bad_cap(cap)) return egr_fail(g_voxel_error, fn, CAP_TEXT);
    if (!(voxel_scale > 0.0) || !std::isfinite(voxel_scale)) return egr_fail(g_voxel_error, fn, "voxel_scale must be positive and finite");
    if (max_rows == 0 || max_rows > cap) return egr_fail(g_voxel_error, fn, "max_rows must be in 1..cap");
    if (!coords || !points || !colors || !counts || !host_rows_and_largest) return egr_fail(g_voxel_error, fn, "coords, points, colors, counts and host_rows_and_largest are required outputs");
    if (!workspace || ((uintptr_t)workspace & 15u)) return egr_fail(g_voxel_error, fn, "a 16-byte aligned workspace of egr_voxel_extract_workspace_bytes(device, max_rows) is required");
    if (workspace_bytes < pair_bytes(max_rows) + 16) return egr_fail(g_voxel_error, fn, "the workspace is smaller than egr_voxel_extract_workspace_bytes(device, max_rows)");
    const EgrRange out[6] = {{status, EGR_VOXEL_STATUS_WORDS * 8}, {coords, max_rows * 12}, {points, max_rows * 12}, {colors, max_rows * 12}, {counts, max_rows * 4},
                             {workspace, workspace_bytes}};
    const EgrRange in[2] = {{keys, cap * 8}, {acc, cap * 32}};
    if (egr_find_clash(out, 6, in, 2)) return egr_fail(g_voxel_error, fn, "an output (status, coords, points, colors, counts, workspace) overlaps the table or another output");
    ExtractArgs a{};
    a.keys = (const ull *)keys, a.acc = (const ull *)acc, a.status = (ull *)status, a.cap = cap, a.max_rows = max_rows;
    uint8_t *w = (uint8_t *)workspace;
    a.pair_keys[0] = (ull *)w, a.pair_keys[1] = (ull *)(w + max_rows * 8);
    a.pair_slots[0] = (uint32_t *)(w + max_rows * 16), a.pair_slots[1] = (uint32_t *)(w + max_rows * 20);
    void *sort_tmp = w + pair_bytes(max_rows);
    const size_t sort_room = workspace_bytes - (size_t)pair_bytes(max_rows);
    a.coords = coords, a.points = points, a.colors = colors, a.counts = counts;
    a.min_count = min_count, a.voxel_scale = (float)voxel_scale;
    hipStream_t s = (hipStream_t)hip_stream;
    return egr_on_device(device, g_voxel_error, fn, [&]() -> int {
        EGR_HIP(hipMemsetAsync(status + 4, 0, 16, s)); // the largest count and the number of rows of THIS extraction
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((cap + VOXEL_COMPACT_CHUNK - 1) / VOXEL_COMPACT_CHUNK, 256u * 8u);
        egr_launch(k_voxel_compact, dim3(blocks), dim3(VOXEL_THREADS), s, a);
        uint64_t host[2] = {0, 0}; // largest count, rows
        EGR_HIP(hipMemcpyAsync(host, status + 4, 16, hipMemcpyDeviceToHost, s));
        EGR_HIP(hipStreamSynchronize(s)); // the one read-back: the number of rows sizes the sort and the last launch
        host_rows_and_largest[0] = host[1], host_rows_and_largest[1] = host[0];
        if (host[1] > max_rows) return egr_fail(g_voxel_error, fn, "more rows than max_rows: nothing was written");
        a.n = host[1];
        if (a.n == 0) return 0;
        // only the n selected pairs are sorted; the workspace was sized for max_rows >= n, and a shortfall is refused, never overrun
        size_t need = 0;
        EGR_HIP(rocprim::radix_sort_pairs(nullptr, need, a.pair_keys[0], a.pair_keys[1], a.pair_slots[0], a.pair_slots[1], (size_t)a.n, 0, 63, s));
        if (need > sort_room) return egr_fail(g_voxel_error, fn, "the workspace is smaller than egr_voxel_extract_workspace_bytes(device, max_rows)");
        EGR_HIP(rocprim::radix_sort_pairs(sort_tmp, need, a.pair_keys[0], a.pair_keys[1], a.pair_slots[0], a.pair_slots[1], (size_t)a.n, 0, 63, s));
        egr_launch(k_voxel_write, dim3((uint32_t)((a.n + VOXEL_THREADS - 1) / VOXEL_THREADS)), dim3(VOXEL_THREADS), s, a);
        return 0;
    });
}
