"""Generates tests/golden/scene_2k_64_reference.npz: the scene, camera and targets of scene_2k_64.npz (the same g_*, cam_*, tg_* arrays) with ref_*
arrays written by the REFERENCE's own shader code run on the CPU (oracle/reference.py, needs oracle/_ref/libegr_reference.so) instead of by the
oracle: the same launches as make_golden_scene.py - a no-grad launch (total_num_calls = 1), then a grad launch (2). Machines without the reference's
sources, the GPU machines among them, check the kernels and the oracle against this file. Data only: what the reference's code computed, none of
its text.

    python tests/golden/make_reference_scene.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
IMAGES = ("output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance", "output_total_transmittance", "output_final")
GRADS = ("dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation", "total_weight")


def main():
    z = np.load(os.path.join(HERE, "scene_2k_64.npz"))
    W, H = int(z["W"]), int(z["H"])
    out = {k: z[k] for k in z.files if not k.startswith("ref_")}
    g = {k[2:]: z[k] for k in z.files if k.startswith("g_")}
    tg = {k[3:]: z[k] for k in z.files if k.startswith("tg_")}
    r = reference.Reference(W, H)
    r.set_camera(z["cam_origin"], z["cam_c2w"], z["cam_fov"])
    r.set_config(jitter_primary_rays=1, num_bounces=2, loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_depth=2.5, loss_weight_normal=2.5,
                 loss_weight_f0=1.0, loss_weight_roughness=1.0)  # synthetic.TRAIN_LOSS_WEIGHTS, as make_golden_scene.py
    r.set_gaussians(g)
    r.update_bvh()
    ref = r.raytrace(False)
    for k in IMAGES:
        out["ref_" + k] = ref[k]
    for k in ("num_traversed", "num_accumulated", "random_seeds"):
        out["ref_" + k] = ref[k]
    refg = r.raytrace(True, targets=tg)
    for k in GRADS:
        out["ref_" + k] = refg[k]
    p = os.path.join(HERE, "scene_2k_64_reference.npz")
    np.savez_compressed(p, **out)
    print("wrote", p, os.path.getsize(p), "bytes; scene_2k_64.npz:", os.path.getsize(os.path.join(HERE, "scene_2k_64.npz")))


if __name__ == "__main__":
    main()
