"""Generates tests/golden/camera_u8_tables.npz by IMPORTING the reference's editable_gauss_refl/utils/tonemapping.py (untonemap) by path and evaluating, on the
CPU in half, the three 8-bit conversions of the reference's Camera.__init__ (editable_gauss_refl/scene/cameras.py:59-70) on every byte value. Needs a checkout
of the reference; the .npz it writes is data (three 256-entry tables as uint16 bit patterns of the halfs, and the torch version that made them), committed
next to it.

    python tests/golden/make_camera_tables.py <root of the reference checkout>
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

b = torch.arange(256, dtype=torch.uint8)
bits = lambda t: t.numpy().view(np.uint16).copy()
out = {"untonemap": bits(tm.untonemap(b.half() / 255.0)),  # image / diffuse_image / specular_image (there on the GPU; here the CPU defines it)
       "normal": bits(b.half() / 255.0 * 2.0 - 1.0),  # normal_image
       "unit": bits(b.half() / 255.0),  # roughness_image / f0_image
       "torch_version": np.array(torch.__version__)}
for k in ("untonemap", "normal", "unit"):
    assert out[k].dtype == np.uint16 and out[k].shape == (256,)
np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "camera_u8_tables.npz"), **out)
print({k: out[k][[0, 1, 127, 254, 255]].tolist() for k in ("untonemap", "normal", "unit")}, torch.__version__)
