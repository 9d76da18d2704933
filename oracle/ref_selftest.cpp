// oracle/ref_selftest.cpp  --  TEST INFRASTRUCTURE.
// A stand-alone program around oracle/ref_driver.cpp for sanitizer runs of the driver and of the reference code it includes (`make -C oracle
// ref_selftest`: built with -fsanitize=address,undefined and run on the CPU). A seeded random scene, some instances invisible, threshold 0 so that
// every hit is composited: image and grad launches in both visiting orders with accumulation on, then a smaller model (the lists shrink, the
// gradient tensors are resized), then the instance records. It checks nothing but that the lists' counters stay inside what the driver reserved;
// the sanitizers do the rest. Comparisons with the oracle live in tests/test_oracle_vs_reference.py.
#include "ref_driver.cpp"
#include <cstdio>
#include <random>
int main() {
    const int W = 24, H = 16, N = 600;
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> rgb(3 * N), nrm(3 * N), f0(3 * N), rough(N), opa(N), scale(3 * N), mean(3 * N), rot(4 * N);
    for (int i = 0; i < N; i++) {
        for (int c = 0; c < 3; c++) rgb[3 * i + c] = u(rng), f0[3 * i + c] = u(rng), scale[3 * i + c] = std::log(0.1f + 0.3f * u(rng));
        nrm[3 * i] = -1, nrm[3 * i + 1] = 0.1f * u(rng), nrm[3 * i + 2] = 0.1f * u(rng);
        rough[i] = 0.05f + 0.3f * u(rng), opa[i] = i % 7 == 0 ? -8.0f : 4 * u(rng) - 1;
        mean[3 * i] = 1.5f + 2.5f * u(rng), mean[3 * i + 1] = 2 * u(rng) - 1, mean[3 * i + 2] = 2 * u(rng) - 1;
        for (int c = 0; c < 4; c++) rot[4 * i + c] = u(rng) - 0.5f;
    }
    void *h = ref_create(W, H);
    const float origin[3] = {0, 0, 0}, c2w[9] = {0, 0, -1, -1, 0, 0, 0, 1, 0};
    ref_set_camera(h, origin, c2w, 0.69f, 0.01f, 999.9f);
    double cfg[20] = {3, 0.005, 0.0, 1, 1, 2, 1, 5, 3, 2.5, 2.5, 1, 1, 1e-12, 1e-12, 0.01, 0.01, 0.2, 0.9, 0.1};
    ref_set_config(h, cfg);
    ref_set_gaussians(h, N, rgb.data(), nrm.data(), f0.data(), rough.data(), opa.data(), scale.data(), mean.data(), rot.data());
    ref_update_bvh(h);
    for (int rev = 0; rev < 2; rev++) {
        ref_set_reverse_traversal(h, rev);
        if (ref_raytrace(h, 0) || ref_raytrace(h, 1)) return 2;
    }
    ref_reset_accumulators(h);
    ref_set_gaussians(h, N / 2, rgb.data(), nrm.data(), f0.data(), rough.data(), opa.data(), scale.data(), mean.data(), rot.data());
    ref_update_bvh(h);
    if (ref_raytrace(h, 1)) return 2;
    std::vector<float> M(12 * N), Wm(12 * N); std::vector<int> vis(N);
    ref_get_instances(h, M.data(), Wm.data(), vis.data());
    Ref *r = (Ref *)h;
    std::printf("launches %u, last launch: %u forward entries of %zu reserved, %u backward entries of %zu reserved\n", ref_get_total_num_calls(h), r->fwd.total_hits,
                r->fwd.capacity, r->bwd.total_hits, r->bwd.capacity);
    if (r->fwd.total_hits > r->fwd.capacity || r->bwd.total_hits > r->bwd.capacity) return 3;
    ref_destroy(h);
    return 0;
}
