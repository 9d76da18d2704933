// SPDX-License-Identifier: MIT
// The host path of a context-free entry point (`int egr_x(int device, ..., void *hip_stream)`, no egr_context): the next fused op starts here.
//
//   thread_local std::string g_x_error;                                             // one per module: egr_x_last_error() speaks for its own functions only
//   extern "C" int egr_x(int device, ..., void *hip_stream) {
//       if (!out) return egr_fail(g_x_error, "egr_x", "out is a required output");  // validation: BEFORE any HIP call, hipGetDevice included
//       if (egr_find_clash(outs, num_outs, ins, num_ins)) return egr_fail(...);     // one overlap rule: a NULL or empty range touches nothing
//       return egr_on_device(device, g_x_error, "egr_x", [&] {                      // entered only after the last validation failure
//           egr_launch(k_x, grid, block, (hipStream_t)hip_stream, args);            // in order; the first HIP error ends the body, its string is the message
//       });
//   }
//
// Host-only: nothing here is device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <utility>

// ---- HIP errors travel as exceptions inside the library and end at its C boundary (egr_on_device below, guarded() in api.hip)
struct EgrCheck {
    hipError_t e;
    const char *what;
};
inline void egr_hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) throw EgrCheck{e, what};
}
#define EGR_HIP(expr) egr_hip_check((expr), #expr)

// ---- ranges of device memory, and the one overlap rule
struct EgrRange {
    const void *p;
    uint64_t bytes;
};
inline bool egr_overlap(const EgrRange &a, const EgrRange &b) { // a NULL or empty range touches nothing
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a.bytes != 0 && b.bytes != 0 && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}
// What an out-of-place launch must not have: an output that touches an input (EGR_CLASH_INPUT: out[out] with in[other]) or another output
// (EGR_CLASH_OUTPUT: out[out] with out[other], out < other). The first clash in the order of the outputs; converts to false when there is none.
enum EgrClashKind { EGR_CLASH_NONE = 0, EGR_CLASH_INPUT, EGR_CLASH_OUTPUT };
struct EgrClash {
    EgrClashKind kind;
    int out, other;
    explicit operator bool() const { return kind != EGR_CLASH_NONE; }
};
inline EgrClash egr_find_clash(const EgrRange *out, int num_out, const EgrRange *in, int num_in) {
    for (int o = 0; o < num_out; o++) {
        for (int i = 0; i < num_in; i++)
            if (egr_overlap(out[o], in[i])) return EgrClash{EGR_CLASH_INPUT, o, i};
        for (int q = o + 1; q < num_out; q++)
            if (egr_overlap(out[o], out[q])) return EgrClash{EGR_CLASH_OUTPUT, o, q};
    }
    return EgrClash{EGR_CLASH_NONE, -1, -1};
}

// ---- failure: "libegr_hip: <function>: <what>" into the module's thread_local string; returns 1
inline int egr_fail(std::string &error, const char *function, const std::string &what) {
    error = std::string("libegr_hip: ") + function + ": " + what;
    return 1;
}

// ---- the device: the calling thread runs on `device` while the scope lives and is back on its own device afterwards, whichever way the scope is left
class EgrDeviceScope {
    int prev_ = 0, device_;

  public:
    explicit EgrDeviceScope(int device) : device_(device) {
        EGR_HIP(hipGetDevice(&prev_));
        if (prev_ != device_) EGR_HIP(hipSetDevice(device_)); // (a throwing constructor has no destructor to run: nothing was switched)
    }
    ~EgrDeviceScope() {
        if (prev_ != device_) (void)hipSetDevice(prev_);
    }
    EgrDeviceScope(const EgrDeviceScope &) = delete;
    EgrDeviceScope &operator=(const EgrDeviceScope &) = delete;
};

// One kernel launch and its check.
template <class... P, class... A> void egr_launch(void (*kernel)(P...), dim3 grid, dim3 block, hipStream_t s, A &&...args) {
    hipLaunchKernelGGL(kernel, grid, block, 0, s, std::forward<A>(args)...);
    EGR_HIP(hipGetLastError());
}

// Runs `body` on `device`: launches through egr_launch, other HIP calls through EGR_HIP. Returns what the body returns (0 for a body without a result),
// or, after the first HIP error, egr_fail with that error's string.
template <class F> int egr_on_device(int device, std::string &error, const char *function, F &&body) {
    try {
        EgrDeviceScope scope(device);
        if constexpr (std::is_void_v<decltype(body())>) {
            body();
            return 0;
        } else {
            return body();
        }
    } catch (const EgrCheck &e) {
        return egr_fail(error, function, hipGetErrorString(e.e));
    }
}
