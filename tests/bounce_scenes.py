"""Scenes whose bounce steps carry real work at transmittance_threshold = 0, shared by the finite-difference tests of the oracle's bounce-step
backward (test_oracle_bounce_gradients.py, fp64, a few pixels) and the HIP tests on the same scenes at size (test_hip_bounce_fd.py, fp32).
A plain module: no fixtures, nothing is collected from here."""
import numpy as np

GRAD_OF = {"rgb": "dL_drgb", "normal": "dL_dnormal", "f0": "dL_df0", "roughness": "dL_droughness", "opacity": "dL_dopacity",
           "mean": "dL_dmean", "scale": "dL_dscale", "rotation": "dL_drotation"}
# the finite-difference tests' configuration: no ray is truncated, d depth / d geometry is not propagated upstream (test_oracle_gradients.py (i), (ii))
FD_CONFIG = dict(transmittance_threshold=0.0, loss_weight_depth=0.0, loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5,
                 loss_weight_f0=1.0, loss_weight_roughness=1.0)


def room_scene(n, seed=0, radius=(2.0, 2.4), scale=(0.3, 0.6), dtype=np.float64):
    """n blobs on a thick shell around the origin, normals facing in: a ray from the inside meets the shell wherever it goes, so a camera at the
    origin sees a closed room and every bounce ray crosses the room and composites the far wall. Opacity logits 1..4 (sigmoid 0.73..0.98: the
    accumulated normal stays above the reflection threshold), roughness 0.05..0.4, f0 0.3..0.9 (both strictly inside the clip range), rgb > 0,
    anisotropic scales and NON-unit quaternions (the backward of the normalisation is live)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    mean = d * rng.uniform(radius[0], radius[1], (n, 1))
    nrm = -d + rng.normal(scale=0.08, size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    q = rng.normal(size=(n, 4))
    q *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    g = dict(rgb=rng.uniform(0.1, 0.9, (n, 3)), normal=nrm, f0=rng.uniform(0.3, 0.9, (n, 3)), roughness=rng.uniform(0.05, 0.4, (n, 1)),
             opacity=rng.uniform(1.0, 4.0, (n, 1)), scale=np.log(rng.uniform(scale[0], scale[1], (n, 3))), mean=mean, rotation=q)
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in g.items()}


def mirror_scene(seed=0, n_mirror=24, n_far=10, dtype=np.float64):
    """(g, far_rows): a near-opaque mirror cluster in front of a +x camera at the origin, facing it, and `far_rows`: blobs BEHIND the camera that no
    primary ray can meet (x < 0) and that the rays reflected by the mirror composite. A change of a far row leaves step 0, hence every bounce ray,
    throughput and down-weight, exactly as it was: the true loss is differentiated with the rays frozen by construction, no hook involved."""
    rng = np.random.default_rng(seed)
    m, f = n_mirror, n_far
    mean = np.concatenate([np.stack([rng.uniform(1.9, 2.1, m), rng.uniform(-0.45, 0.45, m), rng.uniform(-0.4, 0.4, m)], 1),
                           np.stack([rng.uniform(-3.0, -1.5, f), rng.uniform(-0.8, 0.8, f), rng.uniform(-0.8, 0.8, f)], 1)])
    nrm = np.concatenate([np.array([[-1.0, 0.0, 0.0]]) + rng.normal(scale=0.03, size=(m, 3)), np.array([[1.0, 0.0, 0.0]]) + rng.normal(scale=0.2, size=(f, 3))])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    n = m + f
    q = rng.normal(size=(n, 4))
    q *= rng.uniform(0.5, 2.0, (n, 1)) / np.linalg.norm(q, axis=1, keepdims=True)
    g = dict(rgb=rng.uniform(0.1, 0.9, (n, 3)), normal=nrm, f0=rng.uniform(0.3, 0.9, (n, 3)),
             roughness=np.concatenate([rng.uniform(0.03, 0.12, (m, 1)), rng.uniform(0.05, 0.4, (f, 1))]),
             opacity=np.concatenate([rng.uniform(3.0, 5.0, (m, 1)), rng.uniform(-0.5, 2.5, (f, 1))]),
             scale=np.log(np.concatenate([rng.uniform(0.25, 0.4, (m, 3)), rng.uniform(0.3, 0.7, (f, 3))])), mean=mean, rotation=q)
    return {k: np.ascontiguousarray(v.astype(dtype)) for k, v in g.items()}, np.arange(m, n)


def camera(fov=0.5):
    """Origin, looking along +x, z up (synthetic.plus_x_camera in fp64)."""
    c2w = np.array([[0.0, 0.0, -1.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return dict(origin=np.zeros(3), c2w=c2w, fov=float(fov))


def targets_away_from(out, num_bounces, seed=0, gap=(0.05, 0.5), dtype=np.float64):
    """Targets at a random distance in `gap`, on a random side, of every output of the launch `out`: no residual changes sign within a
    finite-difference step, nor between two implementations that agree to 1e-3. The specular target sits off sum_{j>=1} output_rgb[j]."""
    rng = np.random.default_rng(seed + 1000)

    def off(x):
        return (x + rng.choice([-1.0, 1.0], x.shape) * rng.uniform(gap[0], gap[1], x.shape)).astype(dtype)

    return dict(diffuse=off(out["output_rgb"][0]), specular=off(out["output_rgb"][1:num_bounces + 1].sum(axis=0)), depth=off(out["output_depth"][0]),
                normal=off(out["output_normal"][0]), f0=off(out["output_f0"][0]), roughness=off(out["output_roughness"][0]))


def make_oracle(orc, g, cam, W, H, double=True, use_bvh=False, **cfg):
    o = orc.Oracle(W, H, double=double, use_bvh=use_bvh)
    o.set_camera(cam["origin"], cam["c2w"], cam["fov"])
    o.set_config(**cfg)
    o.set_gaussians(g)
    o.update_bvh()
    return o


def launch(o, g=None, grads=False, targets=None, K=1, **kw):
    """One launch with total_num_calls = K (the jitter and GGX seeds are functions of it: every launch of a finite difference traces the same samples)."""
    if g is not None:
        o.set_gaussians(g)
        o.update_bvh()
    o.total_num_calls = K - 1
    return o.raytrace(grads, targets=targets, **kw)
