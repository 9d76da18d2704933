"""Generates tests/golden/tonemap_vectors.npz by IMPORTING the reference's pure-torch helpers by path - editable_gauss_refl/utils/tonemapping.py (tonemap,
untonemap) and editable_gauss_refl/utils/image_utils.py (psnr) - and running them on the CPU. Needs a checkout of the reference; the .npz it writes is data
(inputs + expected outputs), committed next to it.

    python tests/golden/make_tonemap_vectors.py <root of the reference checkout>
"""
import importlib.util
import os
import sys

import numpy as np
import torch


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


root = sys.argv[1] if len(sys.argv) > 1 else os.environ["EGR_REFERENCE_ROOT"]
tm = load(root, "editable_gauss_refl/utils/tonemapping.py", "ref_tonemapping")
iu = load(root, "editable_gauss_refl/utils/image_utils.py", "ref_image_utils")

rng = np.random.default_rng(11)
out = {}
# edge values: NaN -> 0, +inf -> 1, -inf / 3e38 / negatives -> NaN, -0.0 -> 0
edge = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-8, 0.18, 1.0, 50.0, 1e9, 3e38, -1e-30, -0.01], np.float32)
sweep = np.concatenate([edge, np.exp(rng.uniform(np.log(1e-6), np.log(1e4), 243)).astype(np.float32)])
out["x"] = sweep
out["tonemap"] = tm.tonemap(torch.tensor(sweep)).numpy()
y = np.concatenate([np.array([0.0, 1e-6, 0.5, 0.999, 1.0], np.float32), rng.random(123).astype(np.float32)])
out["y"] = y
out["untonemap"] = tm.untonemap(torch.tensor(y)).numpy()
# an HDR image [3, 19, 37] with a noisy twin at roughly 30 dB after the tone curve
for i, (scale, noise) in enumerate(((3.0, 0.2),)):
    a = (scale * rng.random((3, 19, 37)) ** 2).astype(np.float32)
    b = np.abs(a * (1.0 + noise * rng.standard_normal(a.shape)) + 0.01 * noise * rng.standard_normal(a.shape)).astype(np.float32)
    ta, tb = tm.tonemap(torch.tensor(a)).clamp(0, 1), tm.tonemap(torch.tensor(b)).clamp(0, 1)
    out[f"img{i}_a"], out[f"img{i}_b"] = a, b
    out[f"img{i}_psnr"] = iu.psnr(ta, tb).numpy()  # [3, 1]: one number per channel; callers take .mean()
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "tonemap_vectors.npz"), **out)
print({k: v.ravel().tolist() for k, v in out.items() if k.endswith("psnr")}, out["tonemap"][:13])
