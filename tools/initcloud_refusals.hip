// SPDX-License-Identifier: MIT
// The host side of csrc/initcloud.hip - argument validation, overlap arithmetic, workspace layout sizes - under the host sanitizers. It calls ONLY refusals: every
// call returns before the first HIP call, so this runs on a machine without a GPU. A stand-alone program (not loaded into Python, not part of the GPU suite):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/initcloud_refusals.hip editable-gaussian-reflections_amd/csrc/initcloud.hip -o initcloud_refusals && ./initcloud_refusals
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../include/egr_raytracer.h"

static int failures = 0;
static void refused(int rc, const char *needle, const char *what) {
    const char *msg = egr_voxel_last_error();
    if (rc == 0 || !strstr(msg, needle)) {
        printf("NOT REFUSED as expected: %s (rc %d, message '%s')\n", what, rc, msg);
        failures++;
    }
}

int main() {
    // fake device pointers, far apart and 16-byte aligned; they are never dereferenced
    auto P = [](uint64_t k) { return (void *)(uintptr_t)(0x10000000ull * k); };
    int64_t *keys = (int64_t *)P(1), *acc = (int64_t *)P(2), *status = (int64_t *)P(3);
    const double *c2w = (const double *)P(4), *origin = (const double *)P(5), *view = (const double *)P(6);
    const float *depth = (const float *)P(7), *colour = (const float *)P(8), *table = (const float *)P(9);
    const uint8_t *u8 = (const uint8_t *)P(10);
    const uint64_t cap = 4096;
    auto accumulate = [&](int64_t *k, int64_t *a, int64_t *s, uint64_t c, uint32_t V, uint32_t H, uint32_t W, const float *d, const float *col, const uint8_t *b, const float *t,
                          double scale, double cmax, double *pos) { return egr_voxel_accumulate(0, k, a, s, c, V, H, W, c2w, origin, view, d, col, b, t, scale, cmax, pos, nullptr); };
    refused(accumulate(nullptr, acc, status, cap, 2, 19, 37, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "required", "NULL keys");
    refused(accumulate((int64_t *)((uintptr_t)keys + 4), acc, status, cap, 2, 19, 37, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "aligned", "misaligned keys");
    const uint64_t caps[] = {0, 1, 1023, 3000, 1ull << 32, ~0ull, (1ull << 63)};
    for (uint64_t c : caps) refused(accumulate(keys, acc, status, c, 2, 19, 37, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "power of two", "bad capacity");
    refused(accumulate(keys, acc, status, cap, 0, 19, 37, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "num_views", "no views");
    refused(accumulate(keys, acc, status, cap, 2, 0, 37, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "height and width", "no rows");
    refused(accumulate(keys, acc, status, cap, 2, 0xFFFFFFFFu, 0xFFFFFFFFu, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "height and width", "huge image");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, nullptr, colour, nullptr, nullptr, 400, 32768, nullptr), "required", "NULL depth");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, depth, nullptr, nullptr, nullptr, 400, 32768, nullptr), "exactly one", "no colour");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, depth, colour, u8, table, 400, 32768, nullptr), "exactly one", "two colours");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, depth, nullptr, u8, nullptr, 400, 32768, nullptr), "colour_table", "bytes without a table");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, depth, colour, nullptr, nullptr, 0, 32768, nullptr), "voxel_scale", "zero scale");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, depth, colour, nullptr, nullptr, 400, 1e300, nullptr), "colour_max", "huge colour_max");
    refused(accumulate(keys, (int64_t *)((uintptr_t)keys + cap * 8 - 8), status, cap, 2, 19, 37, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "overlaps", "acc in keys");
    refused(accumulate(keys, acc, status, cap, 65535, 1u << 20, 1u << 20, depth, colour, nullptr, nullptr, 400, 32768, nullptr), "2^40", "too many pixels");
    refused(accumulate(keys, acc, status, 1ull << 31, 60000, 1u << 10, 1u << 10, depth, colour, nullptr, nullptr, 400, 32768, (double *)P(11)), "overlaps", "the largest sizes overlap");
    refused(accumulate(keys, acc, status, cap, 2, 19, 37, depth, colour, nullptr, nullptr, 400, 32768, (double *)((uintptr_t)status - 8)), "overlaps", "positions_out ends in status");

    const int64_t *src_keys = (const int64_t *)P(12), *src_acc = (const int64_t *)P(13);
    refused(egr_voxel_rehash(0, keys, acc, status, 2 * cap, nullptr, src_acc, cap, nullptr), "required", "NULL source");
    refused(egr_voxel_rehash(0, keys, acc, status, 2 * cap + 2, src_keys, src_acc, cap, nullptr), "power of two", "bad new capacity");
    refused(egr_voxel_rehash(0, keys, acc, status, 2 * cap, keys, src_acc, cap, nullptr), "out of place", "in place");
    refused(egr_voxel_rehash(0, keys, acc, status, 1ull << 31, src_keys, src_acc, 1ull << 31, nullptr), "out of place", "the largest tables overlap");

    int32_t *coords = (int32_t *)P(20), *counts = (int32_t *)P(23);
    float *points = (float *)P(21), *colors = (float *)P(22);
    uint64_t host[2] = {7, 7};
    void *ws = P(30);
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, 0, coords, points, colors, counts, host, ws, 1 << 20, nullptr), "max_rows", "no rows");
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, cap + 1, coords, points, colors, counts, host, ws, 1 << 20, nullptr), "max_rows", "more rows than slots");
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, 100, coords, points, colors, counts, nullptr, ws, 1 << 20, nullptr), "required outputs", "NULL host result");
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, 100, coords, points, colors, counts, host, nullptr, 1 << 20, nullptr), "workspace", "NULL workspace");
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, 100, coords, points, colors, counts, host, ws, EGR_VOXEL_PAIR_BYTES(100), nullptr), "smaller than", "short workspace");
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, 100, coords, points, colors, counts, host, ws, 0, nullptr), "smaller than", "empty workspace");
    refused(egr_voxel_extract(0, keys, acc, status, cap, 2, 400, 100, coords, (float *)((uintptr_t)coords + 1196), colors, counts, host, ws, 1 << 20, nullptr), "overlaps", "points in coords");
    refused(egr_voxel_extract(0, keys, acc, status, 1ull << 31, 2, 400, 1ull << 31, coords, points, colors, counts, host, ws, ~(size_t)0 >> 1, nullptr), "overlaps", "the largest sizes overlap");
    if (host[0] != 7 || host[1] != 7) printf("a refusal wrote its host result\n"), failures++;
    if (egr_voxel_extract_workspace_bytes(0, 0) != 0) printf("workspace query for no rows\n"), failures++;
    if (EGR_VOXEL_PAIR_BYTES(1) != 32 || EGR_VOXEL_PAIR_BYTES(1ull << 31) != 24ull << 31) printf("EGR_VOXEL_PAIR_BYTES\n"), failures++;
    printf(failures ? "FAILED: %d\n" : "initcloud refusals: all refused, sanitizers silent (%d failures)\n", failures);
    return failures ? 1 : 0;
}
