"""Generates tests/golden/prior_vectors.npz by IMPORTING the reference's editable_gauss_refl/utils/depth_utils.py by path and running its functions on the CPU:

  * pair lists with N in {21, 64, 257, 1000, 5000} (a line with 30 % outliers): the random.sample tables that random.seed(s) gives ransac_linear_fit, and the
    (a, b) and inlier mask it returns under that seed;
  * one whole view of 24 x 40 pixels with about 300 points through the chain of dataset/blender_prior_dataset.py:94-126: world normals, sparse depth map, fit,
    distance, f0.

The reference alone is a fair yardstick only where its accidents cannot show, so this script ASSERTS, and searches seeds until they hold:
  * no two points of the view share a pixel (the reference keeps an arbitrary one), and every projected coordinate is at least 0.05 from a rounding boundary;
  * the second-best hypothesis error is at least 1.01 x the best (the reference sums its errors in fp32);
  * the best hypothesis' top_k-th and (top_k + 1)-th smallest residuals differ by more than 1e-4 relative (the reference's topk picks among equals as it likes).
It stores tol_a (relative) and tol_b (absolute): 4 x the largest difference, over these cases, between the reference's fp32 lstsq result and the fp64
least-squares fit on the reference's own inlier set - the fp32 QR noise a correct implementation may differ by.

Needs a checkout of the reference; the .npz it writes is data, committed next to it.

    python tests/golden/make_prior_vectors.py <root of the reference checkout>
"""
import importlib.util
import math
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import priors_restatement as pr  # noqa: E402  (ours: the hypothesis errors behind the conditions)


def load(root, rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


root = sys.argv[1] if len(sys.argv) > 1 else os.environ["EGR_REFERENCE_ROOT"]
du = load(root, "editable_gauss_refl/utils/depth_utils.py", "ref_depth_utils")
SIZES = (21, 64, 257, 1000, 5000)
NUM_ITERS = 100


def sizes_of(n):
    return min(max(2, math.ceil(n * 0.1)), 50), max(1, math.ceil(n * 0.1))


def tables_of(n, seed):
    random.seed(seed)  # the draws ransac_linear_fit makes after the same call
    s, _ = sizes_of(n)
    return np.array([random.sample(range(n), s) for _ in range(NUM_ITERS)], np.int32)


def fair(x, y, table, top_k):
    """The conditions under which the reference's choice of hypothesis and of inliers is no accident; (ok, error ratio, residual gap)."""
    models = [pr.hypothesis(x, y, row.astype(np.int64), top_k) for row in table]
    errors = np.array([m[4] for m in models])
    order = np.argsort(errors, kind="stable")
    ratio = errors[order[1]] / errors[order[0]]
    w, b = models[order[0]][:2]
    r = np.sort(pr.residuals(x, y, w, b).astype(np.float64))
    gap = (r[top_k] - r[top_k - 1]) / r[top_k] if top_k < len(r) else 1.0
    return ratio >= 1.01 and gap > 1e-4, float(ratio), float(gap)


def reference_fit(x, y, seed):
    """(a, b, mask, best iteration) of the reference. It does not return the iteration it kept: torch.topk is watched while it runs, its values are the negated
    residuals each iteration scores, and the reference's own fp32 sum of their squares with its strict < names the iteration."""
    seen, real = [], torch.topk

    def watched(*args, **kwargs):
        result = real(*args, **kwargs)
        seen.append(result[0].clone())
        return result

    random.seed(seed)
    torch.topk = watched
    try:
        (a, b), mask = du.ransac_linear_fit(torch.from_numpy(x), torch.from_numpy(y))
    finally:
        torch.topk = real
    assert len(seen) == NUM_ITERS
    best, best_error = None, None
    for it, values in enumerate(seen):
        error = values.pow(2).sum()
        if best_error is None or error < best_error:
            best, best_error = it, error
    return np.float32(a.item()), np.float32(b.item()), mask.numpy().copy(), best


def qr_noise(x, y, a, b, mask):
    """|reference fp32 result - fp64 least squares on the reference's inlier set|: (relative in a, absolute in b)."""
    A = np.stack([x[mask].astype(np.float64), np.ones(int(mask.sum()))], axis=1)
    (a64, b64), *_ = np.linalg.lstsq(A, y[mask].astype(np.float64), rcond=None)
    return abs(float(a) - a64) / abs(a64), abs(float(b) - b64)


def fitted_case(x, y, name):
    n = len(x)
    _, top_k = sizes_of(n)
    for seed in range(1000):
        table = tables_of(n, seed)
        ok, ratio, gap = fair(x, y, table, top_k)
        if ok:
            break
    else:
        raise AssertionError(name + ": no seed gives a fair case")
    a, b, mask, best = reference_fit(x, y, seed)
    assert mask.sum() == top_k
    noise = qr_noise(x, y, a, b, mask)
    print(f"{name}: N {n} seed {seed} iteration {best} a {a:.6f} b {b:.6f} error ratio {ratio:.3f} residual gap {gap:.2e} fp32 noise {noise[0]:.2e} {noise[1]:.2e}")
    return dict(seed=np.int64(seed), table=table, a=a, b=b, mask=mask, best_iteration=np.int64(best)), noise


out, noises = {}, []
for n in SIZES:
    g = np.random.default_rng(1000 + n)
    x = g.uniform(0.5, 5.0, n).astype(np.float32)
    y = (1.7 * x + 0.4 + g.normal(0.0, 0.01, n)).astype(np.float32)
    bad = g.random(n) < 0.3
    y[bad] += g.uniform(-3.0, 3.0, int(bad.sum())).astype(np.float32)
    case, noise = fitted_case(x, y, f"pairs_{n}")
    noises.append(noise)
    out.update({f"pairs_{n}_x": x, f"pairs_{n}_y": y, **{f"pairs_{n}_{k}": v for k, v in case.items()}})

# ---- one whole view: ~300 points, each in a pixel of its own, at least 0.05 from the pixel's edges
H, W, M = 24, 40, 300
g = np.random.default_rng(7)
fovx = 1.1
fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
q, _ = np.linalg.qr(g.normal(size=(3, 3)))
c2w_rot = q * np.sign(np.linalg.det(q))  # a proper rotation
centre = g.normal(size=3)
w2c = np.eye(4)
w2c[:3, :3] = c2w_rot.T
w2c[:3, 3] = -c2w_rot.T @ centre
R, T = np.transpose(w2c[:3, :3]).copy(), w2c[:3, 3].copy()  # as the readers store them
fx, fy, cx, cy = W / (2 * math.tan(fovx / 2)), H / (2 * math.tan(fovy / 2)), W / 2, H / 2
pix = g.choice(H * W, M, replace=False)
pu, pv = (pix % W) + g.uniform(-0.44, 0.44, M), (pix // W) + g.uniform(-0.44, 0.44, M)
pz = g.uniform(1.5, 6.0, M)
cam = np.stack([(pu - cx) * pz / fx, (pv - cy) * pz / fy, pz], axis=1)
points = ((cam - w2c[:3, 3]) @ c2w_rot.T).astype(np.float32)  # world = R_c2w (cam - t)
depth = g.uniform(0.3, 3.0, (H, W, 1)).astype(np.float32)  # the prediction: (z - 0.25) / 2.1 under the points, 30 % of them off
pred = (pz - 0.25) / 2.1 + g.normal(0.0, 0.004, M)
off = g.random(M) < 0.3
pred[off] += g.uniform(-1.0, 1.0, int(off.sum()))
depth.reshape(-1)[pix] = pred.astype(np.float32)
normal = g.normal(size=(H, W, 3)).astype(np.float32)
metal = g.random((H, W, 1)).astype(np.float32)

R_t, w2c_t = torch.tensor(R, dtype=torch.float32), torch.tensor(w2c, dtype=torch.float32)
cam_t = du.transform_points(torch.from_numpy(points), w2c_t)
# the conditions on the projection, on the reference's own camera-space points
uf = (cam_t[:, 0] * fx / cam_t[:, 2] + cx).numpy().astype(np.float64)
vf = (cam_t[:, 1] * fy / cam_t[:, 2] + cy).numpy().astype(np.float64)
for c in (uf, vf):
    assert (np.abs(c - np.floor(c) - 0.5) >= 0.05).all(), "a projected coordinate is within 0.05 of a rounding boundary"
assert len(set(zip(np.rint(uf).astype(int).tolist(), np.rint(vf).astype(int).tolist()))) == M, "two points share a pixel"
assert (np.rint(vf) * W + np.rint(uf) == pix).all()
sparse = du.project_pointcloud_to_depth_map(cam_t, fovx, fovy, (H, W))
valid = sparse != 0
assert int(valid.sum()) == M
depth_t = torch.from_numpy(depth)
x, y = depth_t[:, :, 0][valid].float().numpy().copy(), sparse[valid].numpy().copy()
case, noise = fitted_case(x, y, "view")
noises.append(noise)
a_t, b_t = torch.tensor(case["a"]), torch.tensor(case["b"])
fitted = depth_t * a_t + b_t
position = du.transform_depth_to_position_image(fitted.squeeze(-1), fovx, fovy)
distance = torch.norm(position, dim=-1, keepdim=True)
world = du.transform_normals_to_world(torch.from_numpy(normal), R_t)
metal_t = torch.from_numpy(metal)
f0 = (0.04 * (1.0 - metal_t) + metal_t).repeat(1, 1, 3)
out.update(view_R=R, view_T=T, view_fovx=np.float64(fovx), view_fovy=np.float64(fovy), view_points=points, view_depth=depth, view_normal=normal, view_metalness=metal,
           view_sparse=sparse.numpy(), view_x=x, view_y=y, view_distance=distance.numpy(), view_normal_world=world.numpy(), view_f0=f0.numpy(),
           **{f"view_{k}": v for k, v in case.items()})

worst_a, worst_b = max(n[0] for n in noises), max(n[1] for n in noises)
out.update(tol_a=np.float64(4 * worst_a), tol_b=np.float64(4 * worst_b), sizes=np.array(SIZES), num_iters=np.int64(NUM_ITERS), torch_version=np.array(torch.__version__))
print(f"fp32 QR noise before the factor: a {worst_a:.2e} (relative), b {worst_b:.2e} (absolute)")
path = os.path.join(HERE, "prior_vectors.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
