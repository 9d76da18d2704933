// Micro-benchmark: a streaming out-of-place copy of the size csrc/grow.hip's append moves at the reference's size (1M + 75k rows of 8 parameters and 16
// moments: 63 words a row, 271 MB read + 271 MB written), as a grid-stride loop with
//   mode 0: one 4-byte word per lane and iteration   (k_grow_append: no alignment beyond the element's, the seam between old rows and tail anywhere)
//   mode 1: one 16-byte vector per lane and iteration (needs 16-byte aligned src and dst and a seam on a 16-byte boundary)
//   mode 2: hipMemcpyAsync device to device          (the runtime's own copy, for scale)
// Each mode: 3 warm-up runs, then the median of 9 timed with events. Build: hipcc --offload-arch=gfx950 -O3 tools/ubench/copy_width.hip -o tools/ubench/copy_width
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
__global__ void __launch_bounds__(256) k_words(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
__global__ void __launch_bounds__(256) k_vec4(const uint4 *__restrict__ src, uint4 *__restrict__ dst, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) dst[i] = src[i];
}
#define CHECK(x)                                                                     \
    do {                                                                             \
        hipError_t e_ = (x);                                                         \
        if (e_ != hipSuccess) {                                                      \
            printf("%s: %s\n", #x, hipGetErrorString(e_));                           \
            return 1;                                                                \
        }                                                                            \
    } while (0)
int main() {
    const size_t words = (size_t)1075000 * 63 / 4 * 4; // a multiple of 4: the same bytes in every mode
    uint32_t *src, *dst;
    CHECK(hipMalloc(&src, words * 4));
    CHECK(hipMalloc(&dst, words * 4));
    CHECK(hipMemset(src, 1, words * 4));
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    const uint32_t cap = 65535u * 16u; // the append's own grid limit
    for (int mode = 0; mode < 3; mode++) {
        float ms[12];
        for (int rep = 0; rep < 12; rep++) {
            CHECK(hipEventRecord(a));
            if (mode == 0) hipLaunchKernelGGL(k_words, dim3((uint32_t)std::min<size_t>((words + 255) / 256, cap)), dim3(256), 0, 0, src, dst, words);
            if (mode == 1) hipLaunchKernelGGL(k_vec4, dim3((uint32_t)std::min<size_t>((words / 4 + 255) / 256, cap)), dim3(256), 0, 0, (const uint4 *)src, (uint4 *)dst, words / 4);
            if (mode == 2) CHECK(hipMemcpyAsync(dst, src, words * 4, hipMemcpyDeviceToDevice, 0));
            CHECK(hipGetLastError());
            CHECK(hipEventRecord(b));
            CHECK(hipEventSynchronize(b));
            CHECK(hipEventElapsedTime(&ms[rep], a, b));
        }
        std::sort(ms + 3, ms + 12);
        printf("mode %d: median %.3f ms (min %.3f, max %.3f) for %.1f MB read + %.1f MB written = %.2f TB/s\n", mode, ms[7], ms[3], ms[11], words * 4 / 1e6, words * 4 / 1e6,
               2.0 * words * 4 / ms[7] / 1e9);
    }
    return 0;
}
