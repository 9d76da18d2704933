// SPDX-License-Identifier: MIT
// What the evaluation kernels share (csrc/eval.hip: PSNR, csrc/ssim.hip: SSIM): ONE tone curve, ONE reduction tree and ONE error string, so that the two
// metrics of a view are computed on the same display values and egr_eval_last_error() speaks for both.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "egr_host.hpp"

// D(x) = clamp(tonemap(x), 0, 1), operation by operation as torch evaluates it in fp32 (every product and sum rounded on its own: no fused multiply-add).
// NaN propagates: a negative quotient gives NaN from the power, +-huge inputs give inf / inf, and the clamp is written with comparisons, which keep a NaN
// (fminf / fmaxf would drop it).
__device__ __forceinline__ float tone_display(float x) {
#pragma clang fp contract(off)
    if (x != x) x = 0.0f;                                         // nan_to_num: NaN -> 0
    else if (x == INFINITY) x = 999999999.9f;                     //             +inf -> posinf
    else if (x == -INFINITY) x = -3.402823466e+38f;               //             -inf -> the most negative float (then inf / inf = NaN below)
    const float num = x * (6.2f * x + 0.5f);
    const float den = x * (6.2f * x + 1.7f) + 0.06f;
    float y = powf(__fdiv_rn(num, den), 1.3f);
    y = y < 0.0f ? 0.0f : y;
    y = y > 1.0f ? 1.0f : y;
    return y;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v; // lane 0 holds the sum (a fixed tree: the same order on every run)
}

// What egr_eval_last_error() returns: the one string eval.hip (which defines it), ssim.hip and frames.hip hand to egr_fail / egr_on_device.
extern thread_local std::string g_eval_error;
