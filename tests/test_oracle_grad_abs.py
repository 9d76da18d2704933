"""The oracle's per-component sums of absolute contributions (raytrace(..., abs_sums=True) -> out["grad_abs"]) and the one-loss-term-at-a-time
isolation that tests/test_hip_gradient_terms.py builds on: both are CPU-only properties of the oracle itself."""
import numpy as np
import pytest

GRAD = ["dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation", "total_weight"]
TERMS = ["diffuse", "depth", "normal", "f0", "roughness", "specular"]
WEIGHTS = dict(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0)


def _scene_oracle(orc, syn, double, W=40, H=30, n=1500, **cfg):
    g = syn.make_scene(n, "trained", seed=21)
    cam = syn.default_camera()
    o = orc.Oracle(W, H, double=double)
    o.set_camera(cam["origin"], cam["c2w"], cam["fov"])
    o.set_gaussians(g)
    o.set_config(jitter_primary_rays=0, num_bounces=2, **{**WEIGHTS, **cfg})
    o.update_bvh()
    return o, syn.make_targets(W, H)


@pytest.mark.parametrize("double", [False, True], ids=["fp32", "fp64"])
def test_grad_abs_bounds_every_component(orc, syn, double):
    o, tg = _scene_oracle(orc, syn, double)
    ref = o.raytrace(True, targets=tg, abs_sums=True)
    assert (ref["effective_steps"] > 1).mean() > 0.3  # bounce steps contribute too
    ab = ref["grad_abs"]
    assert sorted(ab) == sorted(GRAD)
    for k in GRAD:
        assert ab[k].shape == ref[k].shape, k
        assert np.abs(ref[k]).max() > 0, k
        # (the two sums are flushed from the threads' tables in possibly different orders: round-off of one fp64 sum is allowed)
        assert np.all(ab[k] >= np.abs(ref[k]) - 1e-12 * ab[k]), k
        assert np.all(ref[k][ab[k] == 0] == 0), k  # no contribution, no gradient
    # cancellation is real: on many components the plain sum is far below the sum of magnitudes
    ratio = np.abs(ref["dL_dmean"]) / np.maximum(ab["dL_dmean"], 1e-300)
    assert (ratio[ab["dL_dmean"] > 0] < 0.5).mean() > 0.05
    np.testing.assert_allclose(ab["total_weight"], ref["total_weight"], rtol=1e-12, atol=0)  # every weight is >= 0


def test_grad_abs_is_off_by_default(orc, syn):
    o, tg = _scene_oracle(orc, syn, False, W=8, H=6, n=300)
    assert "grad_abs" not in o.raytrace(True, targets=tg)
    assert "grad_abs" not in o.raytrace(False, abs_sums=True)


def test_grad_abs_of_a_single_hit_is_the_gradients_magnitude(orc, syn):
    """One gaussian, one pixel, no bounces: every component has exactly one contribution, so Σ|c| = |Σ c| bit for bit."""
    o = orc.Oracle(1, 1, double=True, use_bvh=False)
    cam = syn.plus_x_camera(fov=0.5)
    o.set_camera(cam["origin"].astype(np.float64), cam["c2w"].astype(np.float64), 0.5)
    o.set_config(jitter_primary_rays=0, num_bounces=0, **WEIGHTS)
    g = dict(rgb=np.array([[0.5, 0.3, 0.7]]), normal=np.array([[-1.0, 0.2, 0.1]]), f0=np.array([[0.3, 0.4, 0.5]]), roughness=np.array([[0.5]]),
             opacity=np.array([[0.4]]), scale=np.log(np.array([[0.3, 0.25, 0.35]])), mean=np.array([[2.0, 0.03, -0.02]]),
             rotation=np.array([[0.9, 0.1, -0.2, 0.3]]))
    o.set_gaussians(g)
    o.update_bvh()
    tg = dict(diffuse=np.full((1, 1, 3), 0.9), specular=np.zeros((1, 1, 3)), depth=np.full((1, 1, 1), 3.0), normal=np.zeros((1, 1, 3)),
              f0=np.full((1, 1, 3), 0.9), roughness=np.full((1, 1, 1), 0.1))
    ref = o.raytrace(True, targets=tg, abs_sums=True)
    assert ref["num_accumulated"][0, 0] == 1
    for k in GRAD:
        assert np.abs(ref[k]).min() > 0, k  # every component is live (one hit feeds them all)
        np.testing.assert_array_equal(ref["grad_abs"][k], np.abs(ref[k]), err_msg=k)


def test_per_term_gradients_sum_to_the_all_terms_gradient(orc, syn):
    """The isolation method of the per-term GPU tests: with the other five loss weights at 0, each run is one term's share of the gradient;
    the forward does not depend on the weights, so the six shares add up to the all-terms gradient up to fp64 round-off of the sums."""
    o, tg = _scene_oracle(orc, syn, True)
    full = o.raytrace(True, targets=tg, abs_sums=True)
    total = {k: np.zeros_like(full[k]) for k in GRAD}
    scale = {k: np.zeros_like(full[k]) for k in GRAD}
    for term in TERMS:
        o.set_config(**{w: (v if w == "loss_weight_" + term else 0.0) for w, v in WEIGHTS.items()})
        o.total_num_calls = 0
        part = o.raytrace(True, targets=tg, abs_sums=True)
        for k in GRAD[:-1]:
            total[k] += part[k]
            scale[k] += part["grad_abs"][k]
        np.testing.assert_allclose(part["total_weight"], full["total_weight"], rtol=1e-12, atol=0)  # (the forward, hence every weight, is the same launch)
        assert np.abs(part["dL_dopacity"]).max() > 0, term  # every term feeds opacity
    o.set_config(**WEIGHTS)
    for k in GRAD[:-1]:
        assert np.all(np.abs(total[k] - full[k]) <= 1e-12 * scale[k] + 1e-300), (k, float(np.abs(total[k] - full[k]).max()))
        assert np.all(scale[k] >= full["grad_abs"][k] * (1 - 1e-12)), k  # |w1 c1 + w2 c2| <= w1|c1| + w2|c2| per hit
