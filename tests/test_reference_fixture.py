"""The CPU oracle against tests/golden/scene_2k_64_reference.npz: outputs that the reference's own shader code wrote for the golden 2k scene when it
was run on the CPU (tests/golden/make_reference_scene.py). Needs no reference sources: every machine checks the oracle against the reference's
numbers with this, under the comparison rule of tests/ref_compare.py."""
import os

import numpy as np

import ref_compare as rc

GOLD = os.path.join(os.path.dirname(__file__), "golden")
IMAGES = [k for k in rc.OUT_KEYS if k not in ("output_ray_origin", "output_ray_direction")]  # (what the fixture holds)


def test_oracle_reproduces_the_reference_fixture(orc):
    z = np.load(os.path.join(GOLD, "scene_2k_64_reference.npz"))
    W, H = int(z["W"]), int(z["H"])
    g = {k[2:]: z[k] for k in z.files if k.startswith("g_")}
    tg = {k[3:]: z[k] for k in z.files if k.startswith("tg_")}
    fix = {k[4:]: z[k] for k in z.files if k.startswith("ref_")}
    sides = [orc.Oracle(W, H, use_bvh=False, inverse_from_transform=True), orc.Oracle(W, H, double=True)]  # (candidates in index order and the transforms' inverse as the fixture's writer met and formed them)
    for o in sides:
        o.set_camera(z["cam_origin"], z["cam_c2w"], z["cam_fov"])
        o.set_config(jitter_primary_rays=1, num_bounces=2, loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_depth=2.5, loss_weight_normal=2.5,
                     loss_weight_f0=1.0, loss_weight_roughness=1.0)
        o.set_gaussians(g)
        o.update_bvh()

    def launch(grads):
        return [o.raytrace(grads, targets=tg) for o in sides]

    a, b = launch(False)  # total_num_calls = 1, as the fixture's
    rc.assert_integers(fix, a, "reference_fixture")
    res = rc.three_way(fix, a, b, IMAGES)
    for s in range(3):
        keys = IMAGES[:-1]
        per = rc.three_way({k: fix[k][s:s + 1] for k in keys}, {k: a[k][s:s + 1] for k in keys}, {k: b[k][s:s + 1] for k in keys}, keys)
        res.update({f"{k}[{s}]": v for k, v in per.items()})
    ag, bg = launch(True)  # 2
    resg = rc.three_way({k: fix[k][None, None] for k in rc.GRAD_KEYS}, {k: ag[k][None, None] for k in rc.GRAD_KEYS}, {k: bg[k][None, None] for k in rc.GRAD_KEYS}, rc.GRAD_KEYS)
    listing = rc.could_be_left_out(a)
    rc.report("reference_fixture", images_worst_ratio=f"{rc.worst_ratio(res):.2f}", grads_worst_ratio=f"{rc.worst_ratio(resg):.2f}", pixels_the_oracle_flags=len(listing))
    # the fixture holds whole-image results, so no pixel can be taken out of it: the integers (assert_integers above) and the rule hold with every pixel in
    assert not rc.failing(res), (rc.failing(res), listing)
    assert not rc.failing(resg), (rc.failing(resg), listing)
