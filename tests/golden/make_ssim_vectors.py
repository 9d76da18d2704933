"""Generates tests/golden/ssim_vectors.npz by IMPORTING the reference's pure-torch metric editable_gauss_refl/utils/loss_utils.py:39-70 (ssim: an 11 x 11
Gaussian window, zero "same" padding, five depthwise convolutions, the map, its mean). Run in the build container only (needs /root/reference); the .npz it
writes is data (inputs + expected outputs), committed next to it.

    python tests/golden/make_ssim_vectors.py

Per case: the two fp32 images a, b [3,H,W]; `ssim64` = the reference's ssim(a[None], b[None]) evaluated on fp64 tensors and `ssim64_channels` [3] =
ssim(a[:, None], b[:, None], size_average=False) on fp64 tensors - what the tests compare with -; `ssim32`, the same call on the fp32 tensors, for the record.
It also prints the distance of tests/ssim_restatement.py from ssim64 per case (tests/test_ssim_host.py derives its bound from the worst of them) and the
reference's own fp32-to-fp64 distance."""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ssim_restatement as sr  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_loss_utils", "/root/reference/editable_gauss_refl/utils/loss_utils.py")
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

rng = np.random.default_rng(11)


def noisy(shape, eps):
    a = rng.random(shape)
    return a, np.clip(a + eps * rng.standard_normal(shape), 0, 1)


ramp = np.broadcast_to(np.linspace(0, 1, 48)[None, None, :] * np.linspace(0.2, 1, 40)[None, :, None], (3, 40, 48)) * np.array([1.0, 0.8, 0.6])[:, None, None]
binary = (rng.random((3, 24, 31)) < 0.5).astype(np.float64)
cases = {
    "random_1x1": noisy((3, 1, 1), 0.1),      # no interior; every tap but one is padding
    "random_5x7": noisy((3, 5, 7), 0.1),      # no interior in either axis
    "random_12x10": noisy((3, 12, 10), 0.1),  # an interior in one axis only: none
    "random_11x11": noisy((3, 11, 11), 0.1),  # exactly one interior pixel
    "random_16x24": noisy((3, 16, 24), 0.05),
    "random_37x53": noisy((3, 37, 53), 0.1),  # several tiles, ragged edges, halos across tile borders
    "random_45x70": noisy((3, 45, 70), 0.02),
    "flat_050_075": (np.full((3, 40, 40), 0.5), np.full((3, 40, 40), 0.75)),  # the variance terms are pure cancellation
    "flat_identical": (np.full((3, 40, 40), 0.3), np.full((3, 40, 40), 0.3)),
    "zeros": (np.zeros((3, 20, 33)), np.zeros((3, 20, 33))),
    "ones_vs_zeros": (np.ones((3, 20, 33)), np.zeros((3, 20, 33))),
    "ramp_noise": (ramp, np.clip(ramp + 1e-3 * rng.standard_normal(ramp.shape), 0, 1)),
    "binary_complement": (binary, 1.0 - binary),  # negative SSIM
}
out, worst, worst32 = {}, 0.0, 0.0
for name, (a, b) in cases.items():
    a, b = a.astype(np.float32), b.astype(np.float32)
    ta, tb = torch.tensor(a), torch.tensor(b)
    s64 = float(ref.ssim(ta.double()[None], tb.double()[None]))
    c64 = ref.ssim(ta.double()[:, None], tb.double()[:, None], size_average=False).numpy()
    s32 = float(ref.ssim(ta[None], tb[None]))
    out[name + "_a"], out[name + "_b"] = a, b
    out[name + "_ssim64"], out[name + "_ssim64_channels"], out[name + "_ssim32"] = np.float64(s64), c64.astype(np.float64), np.float32(s32)
    m = sr.ssim_map(a, b)
    d = max(abs(float(sr.means(m)[0]) - s64), float(np.abs(m.mean((-2, -1)) - c64).max()))
    worst, worst32 = max(worst, d), max(worst32, abs(s32 - s64))
    print(f"{name:18s} ssim64 {s64:+.9f}  restatement - ssim64 {d:.2e}  reference fp32 - fp64 {abs(s32 - s64):.2e}  interior {float(sr.means(m)[1]):+.9f}")
print(f"worst restatement distance {worst:.2e}; worst reference fp32-to-fp64 distance {worst32:.2e}")
np.savez_compressed(os.path.join(HERE, "ssim_vectors.npz"), **out)
print("wrote", len(cases), "cases,", os.path.getsize(os.path.join(HERE, "ssim_vectors.npz")), "bytes")
