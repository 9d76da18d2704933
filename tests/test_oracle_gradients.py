"""fp64 finite-difference validation of the oracle's analytic backward.

The reference's backward (backward_pass.cu:80-220) is the exact gradient of the in-kernel L1 loss when
(i) no ray is truncated (transmittance_threshold = 0), (ii) loss_weight_depth = 0 (d depth / d geometry is not
propagated), (iii) no candidate straddles a clip boundary within the FD step, (iv) num_bounces = 0 IN THIS FILE: the bounce steps, where
the backward additionally holds every bounce ray, throughput and down-weight constant, are differentiated in test_oracle_bounce_gradients.py
(with those held at their base values: Oracle.set_frozen_chain)."""
import numpy as np
import pytest


def _setup(orc, syn, n=14, W=5, H=4, seed=0, **cfg):
    g = syn.random_blob_scene(n, seed=seed, extent=0.35, depth_range=(1.5, 3.0), scale_range=(0.12, 0.3), dtype=np.float64)
    cam = syn.plus_x_camera(fov=0.5)
    o = orc.Oracle(W, H, double=True, use_bvh=False)
    o.set_camera(cam["origin"].astype(np.float64), cam["c2w"].astype(np.float64), 0.5)
    base = dict(jitter_primary_rays=0, num_bounces=0, transmittance_threshold=0.0, loss_weight_depth=0.0,
                loss_weight_diffuse=5.0, loss_weight_normal=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0)
    base.update(cfg)
    o.set_config(**base)
    rng = np.random.default_rng(seed + 100)
    tg = dict(diffuse=rng.uniform(0, 1, (H, W, 3)), specular=rng.uniform(0, 1, (H, W, 3)), depth=rng.uniform(1, 3, (H, W, 1)),
              normal=rng.uniform(-1, 1, (H, W, 3)), f0=rng.uniform(0, 1, (H, W, 3)), roughness=rng.uniform(0, 1, (H, W, 1)))
    return o, g, tg


def _loss(orc, o, g, tg):
    o.set_gaussians(g)
    o.update_bvh()
    out = o.raytrace(False)
    return orc.l1_loss(out, tg, o.config, 0)


@pytest.mark.parametrize("seed", [0, 1])
def test_backward_matches_central_differences(orc, syn, seed):
    o, g, tg = _setup(orc, syn, seed=seed)
    o.set_gaussians(g)
    o.update_bvh()
    an = o.raytrace(True, targets=tg)
    assert an["num_accumulated"].sum() > 40  # the test must actually exercise hits
    names = {"rgb": "dL_drgb", "normal": "dL_dnormal", "f0": "dL_df0", "roughness": "dL_droughness", "opacity": "dL_dopacity",
             "mean": "dL_dmean", "scale": "dL_dscale", "rotation": "dL_drotation"}
    eps = 1e-6
    for k, gk in names.items():
        fd = np.zeros_like(g[k])
        it = np.nditer(g[k], flags=["multi_index"])
        for _ in it:
            idx = it.multi_index
            gp = {a: b.copy() for a, b in g.items()}
            gm = {a: b.copy() for a, b in g.items()}
            gp[k][idx] += eps
            gm[k][idx] -= eps
            fd[idx] = (_loss(orc, o, gp, tg) - _loss(orc, o, gm, tg)) / (2 * eps)
        scale = np.abs(fd).max() + 1e-12
        err = np.abs(fd - an[gk]).max() / scale
        assert err < 2e-5, (k, err, scale)


def test_depth_weight_breaks_geometry_gradients_only(orc, syn):
    """With loss_weight_depth != 0 appearance/opacity still match FD; mean/scale/rotation do not, because the
    reference does not back-propagate d t / d geometry (backward_pass.cu:127-128,141). Documents, not fixes."""
    o, g, tg = _setup(orc, syn, seed=0, loss_weight_depth=2.5)
    o.set_gaussians(g)
    o.update_bvh()
    an = o.raytrace(True, targets=tg)
    eps = 1e-6

    def fd_of(k, idx):
        gp = {a: b.copy() for a, b in g.items()}
        gm = {a: b.copy() for a, b in g.items()}
        gp[k][idx] += eps
        gm[k][idx] -= eps
        return (_loss(orc, o, gp, tg) - _loss(orc, o, gm, tg)) / (2 * eps)

    i = int(np.argmax(np.abs(an["dL_dopacity"][:, 0])))
    assert abs(fd_of("opacity", (i, 0)) - an["dL_dopacity"][i, 0]) < 1e-5 * (1 + abs(an["dL_dopacity"][i, 0]))
    assert abs(fd_of("rgb", (i, 1)) - an["dL_drgb"][i, 1]) < 1e-5 * (1 + abs(an["dL_drgb"][i, 1]))
    dm = max(abs(fd_of("mean", (i, a)) - an["dL_dmean"][i, a]) for a in range(3))
    assert dm > 1e-3


def test_sign_of_zero_residual_is_plus_one(orc, syn):
    """misc.cu:59-63 copysignf(1, 0) = +1: a pixel whose output equals its target still pushes gradients."""
    o, g, tg = _setup(orc, syn, n=1, W=1, H=1)
    g = dict(rgb=np.array([[0.5, 0.5, 0.5]]), normal=np.array([[-1.0, 0, 0]]), f0=np.full((1, 3), 0.04), roughness=np.array([[0.5]]),
             opacity=np.array([[0.0]]), scale=np.full((1, 3), np.log(0.3)), mean=np.array([[2.0, 0, 0]]), rotation=np.array([[1.0, 0, 0, 0]]))
    o.set_gaussians(g)
    o.update_bvh()
    out = o.raytrace(False)
    tg = dict(diffuse=out["output_rgb"][0].copy(), normal=out["output_normal"][0].copy(), f0=out["output_f0"][0].copy(),
              roughness=out["output_roughness"][0].copy(), depth=out["output_depth"][0].copy(), specular=np.zeros((1, 1, 3)))
    an = o.raytrace(True, targets=tg)
    a = float(np.float32(0.9999)) * 0.5
    np.testing.assert_allclose(an["dL_drgb"][0], np.full(3, float(np.float32(1 / 3)) * 5.0 * a), rtol=1e-7)
    np.testing.assert_allclose(an["total_weight"][0, 0], a, rtol=1e-7)


def test_grad_accumulates_onto_existing_buffers(orc, syn):
    o, g, tg = _setup(orc, syn, seed=1)
    o.set_gaussians(g)
    o.update_bvh()
    a = o.raytrace(True, targets=tg)
    o.total_num_calls = 0
    b = o.raytrace(True, targets=tg, grads_into={k: v.copy() for k, v in a.items() if k.startswith("dL_") or k == "total_weight"})
    np.testing.assert_allclose(b["dL_dmean"], 2 * a["dL_dmean"], rtol=1e-12)
