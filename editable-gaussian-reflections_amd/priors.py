"""Prior views: network-predicted G-buffers made trainable on the GPU (csrc/priors.hip) - what the reference's prior datasets do per view on the CPU in their
__getitem__ (dataset/blender_prior_dataset.py:94-126, dataset/colmap_prior_dataset.py:124-146 with utils/depth_utils.py):

  1. the camera-space normals are flipped, normalised and rotated into the world,
  2. the predicted, affine-ambiguous depth is aligned to the SfM points the view sees: a sparse depth map of the points, a RANSAC fit y = a x + b over the pixels
     that hold a point, depth * a + b,
  3. that depth becomes the distance along the pixel's ray,
  4. f0 = 0.04 (1 - metalness) + metalness, three times.

`prepare_prior_views` does this for `views_per_call` views at a time in six launches and ONE read-back (the pair counts, which size the sample tables), and
returns records `dataset.ViewSet.add` takes as they are. The hypotheses are upstream's own: the sample table of a view is drawn on the host by
random.Random(seed + view index).sample(range(N), S), the call upstream makes, so seeding like upstream fits upstream's lines.

Definitions of this package where upstream's result is an accident of its implementation:
  * NEAREST POINT. Where several points fall into one pixel the nearest one wins. Upstream means to ("sort by pixel index and depth") but sorts by pixel only, with
    an unstable argsort, and keeps an arbitrary one. Here the map depends on the set of points, not on their order.
  * TIE RULE. The inliers of the best hypothesis are the pairs with a residual below the top_k-th smallest, plus the first pairs IN PAIR ORDER (row-major pixel
    order) among those equal to it, until top_k are taken. Upstream's topk picks among equals as its implementation happens to.
  * DROPPED PAIRS. A pixel under a point whose predicted depth is not finite is left out of the fit and counted (depth_fit.dropped). Upstream would feed it to
    lstsq and get NaN for the whole view.

Out of scope: image and COLMAP model readers (PIL's decoders and pycolmap are no dependencies: the caller brings decoded arrays and the points each view sees);
resizing before the fit - prepare the views at the size you train at, since ViewSet.add's resize would average distances after the fit where upstream resizes
first; a device-side sampler that would spare the count read-back; writing halfs straight into the ViewSet planes.
"""
import math
import random
from types import SimpleNamespace

import numpy as np
import torch

from . import load_library

CAM_FLOATS = 25  # EGR_PRIOR_CAM_FLOATS: w2c [3,4], fx, fy, cx, cy, R [3,3]
MAX_SAMPLE = 1024  # EGR_PRIOR_MAX_SAMPLE
METHODS = {"ransac": 0, "lstsq": 1}


def fit_sizes(num_pairs, sample_fraction=0.1, max_sample_size=50, best_fraction=0.1):
    """(sample size S, top_k) of ransac_linear_fit for N pairs (depth_utils.py:232-234), in Python floats as upstream: (0, 0) below 2 pairs."""
    if num_pairs < 2:
        return 0, 0
    return min(max(2, math.ceil(num_pairs * sample_fraction)), max_sample_size), max(1, math.ceil(num_pairs * best_fraction))


def sample_table(num_pairs, num_iters=100, sample_fraction=0.1, max_sample_size=50, seed=0):
    """The hypotheses of one pair list: int32 [num_iters, S], row i = the i-th random.sample(range(N), S) of random.Random(seed) - what upstream's loop draws
    after random.seed(seed)."""
    S, _ = fit_sizes(num_pairs, sample_fraction, max_sample_size)
    if S < 2:
        raise ValueError(f"sample_table: {num_pairs} pairs cannot be sampled (at least 2 are required)")
    if S > num_pairs:
        raise ValueError(f"sample_table: a sample of {S} from {num_pairs} pairs")
    rng = random.Random(seed)
    return np.array([rng.sample(range(num_pairs), S) for _ in range(num_iters)], dtype=np.int32).reshape(num_iters, S)


def intrinsics(fovx, fovy, height, width):
    """(fx, fy, cx, cy) of depth_utils.py:145-150, in Python floats."""
    return width / (2 * math.tan(fovx / 2)), height / (2 * math.tan(fovy / 2)), width / 2, height / 2


def camera_rows(cam_infos, height, width):
    """fp32 [V, 25] rows of include/egr_raytracer.h's `cams`: the world-to-camera matrix [R^T | T] (3 x 4, row-major), fx, fy, cx, cy rounded from Python floats,
    and the record's R (camera to world, which rotates the normals)."""
    rows = np.zeros((len(cam_infos), CAM_FLOATS), np.float32)
    for v, info in enumerate(cam_infos):
        R = np.asarray(info.R, np.float64).reshape(3, 3)
        w2c = np.concatenate([R.T, np.asarray(info.T, np.float64).reshape(3, 1)], axis=1)
        fovy = float(info.FovY if hasattr(info, "FovY") else info.FoVy)
        fovx = float(info.FovX if hasattr(info, "FovX") else info.FoVx)
        rows[v, :12] = w2c.astype(np.float32).reshape(12)
        rows[v, 12:16] = np.array(intrinsics(fovx, fovy, height, width), np.float64).astype(np.float32)
        rows[v, 16:] = R.astype(np.float32).reshape(9)
    return rows


def _f32(x, device):
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    return t.to(device=device, dtype=torch.float32)


@torch.no_grad()
def project_points(points_cam, fovx, fovy, image_size, device="cuda"):
    """project_pointcloud_to_depth_map (depth_utils.py:132-182) with the nearest-point rule: fp32 [H,W] on the device, the depth of the nearest CAMERA-space point
    per pixel, 0 = empty."""
    load_library()
    H, W = int(image_size[0]), int(image_size[1])
    dev = torch.device(device)
    pts = _f32(points_cam, dev).reshape(-1, 3).contiguous()
    row = np.zeros((1, CAM_FLOATS), np.float32)
    row[0, [0, 5, 10]] = 1.0  # points already in camera space: the identity
    row[0, 12:16] = np.array(intrinsics(float(fovx), float(fovy), H, W), np.float64).astype(np.float32)
    sparse = torch.ops.egr.prior_pairs(torch.from_numpy(row).to(dev), pts, [0, pts.shape[0]], torch.zeros((1, H, W, 1), dtype=torch.float32, device=dev))[0][0]
    return torch.where(torch.isinf(sparse), torch.zeros_like(sparse), sparse)


@torch.no_grad()
def ransac_linear_fit(x, y, samples=None, seed=0, num_iters=100, sample_fraction=0.1, max_sample_size=50, best_fraction=0.1, method="ransac", details=False, device="cuda"):
    """ransac_linear_fit (depth_utils.py:208-278) for one pair list: ((a, b), inlier mask) with a, b 0-dim fp32 tensors and the mask a bool [N] tensor on the
    device; nothing is read back. `samples`: an int [num_iters, S] table of pair indices (default: sample_table(N, ..., seed)). method "lstsq" fits all pairs.
    details=True adds a SimpleNamespace(best_iteration, best_error, hyp_error, hyp_model, top_k) of device tensors as third result."""
    load_library()
    if method not in METHODS:
        raise ValueError(f"ransac_linear_fit: method must be one of {sorted(METHODS)}, got {method!r}")
    dev = torch.device(device)
    x, y = _f32(x, dev).reshape(1, -1).contiguous(), _f32(y, dev).reshape(1, -1).contiguous()
    N = x.shape[1]
    if y.shape[1] != N:
        raise ValueError("ransac_linear_fit: x and y must have one length")
    if N < 2:
        raise ValueError(f"ransac_linear_fit: {N} pairs cannot be fitted (at least 2 are required)")
    S, top_k = fit_sizes(N, sample_fraction, max_sample_size, best_fraction)
    table = None
    if method == "ransac":
        table = sample_table(N, num_iters, sample_fraction, max_sample_size, seed) if samples is None else np.asarray(samples)
        if table.ndim != 2 or table.shape[0] < 1 or not 2 <= table.shape[1] <= min(N, MAX_SAMPLE):
            raise ValueError(f"ransac_linear_fit: samples must be [num_iters, S] with 2 <= S <= min(N, {MAX_SAMPLE}), got {table.shape}")
        if table.min() < 0 or table.max() >= N:
            raise ValueError(f"ransac_linear_fit: a sample index outside 0..{N - 1}")
        S = table.shape[1]
        table = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int32)).reshape(1, -1, S)
    ab, best_it, best_err, hyp_error, hyp_model, mask = torch.ops.egr.prior_fit(x, y, [N], [S], [top_k], table, METHODS[method], True)
    result = ((ab[0, 0], ab[0, 1]), mask[0].bool())
    if details:
        return result + (SimpleNamespace(best_iteration=best_it[0], best_error=best_err[0], hyp_error=hyp_error[0], hyp_model=hyp_model[0], top_k=top_k),)
    return result


def _image(img, dev, what, channels):
    t = _f32(img, dev)
    if t.dim() == 2:
        t = t.unsqueeze(-1)
    if t.dim() != 3 or t.shape[2] not in channels:
        raise ValueError(f"prepare_prior_views: {what} must be [H,W] or [H,W,C] with C in {channels}, got {tuple(t.shape)}")
    return t


def _record(info, **changes):
    fields = info._asdict() if hasattr(info, "_asdict") else dict(vars(info))
    fields.update(changes)
    return SimpleNamespace(**fields)


@torch.no_grad()
def prepare_prior_views(cam_infos, points, views_per_call=8, seed=0, method="ransac", on_too_few="raise", num_iters=100, sample_fraction=0.1, max_sample_size=50,
                        best_fraction=0.1, device="cuda"):
    """The records of `cam_infos` made trainable: per record (R, T, FovY, FovX, depth_image [H,W(,1|3)] predicted camera z of which channel 0 is read, normal_image
    [H,W,3] in camera space and already * 2 - 1, metalness_image [H,W(,1)] or None; any other attribute is passed through untouched) a SimpleNamespace with the same
    attributes and depth_image = the DISTANCE image [H,W,1], normal_image = the world normals [H,W,3], f0_image [H,W,3] (with metalness): fp32 tensors on the
    device, and depth_fit = SimpleNamespace(a, b, best_iteration, best_error: 0-dim device tensors; num_pairs, top_k, dropped, fitted: host values).
    `points[v]`: the world-space SfM points view v sees, [M_v,3] (M_v may be 0). View i draws its hypotheses from random.Random(seed + i).
    A view with fewer than 2 pairs cannot be fitted: on_too_few="raise" raises a ValueError that names it, "identity" keeps its depth (a = 1, b = 0, fitted False).
    Consecutive records that share the image size go `views_per_call` at a time: six launches and one read-back per chunk."""
    load_library()
    cam_infos, points = list(cam_infos), list(points)
    if len(points) != len(cam_infos):
        raise ValueError(f"prepare_prior_views: {len(cam_infos)} records, {len(points)} point lists")
    if method not in METHODS:
        raise ValueError(f"prepare_prior_views: method must be one of {sorted(METHODS)}, got {method!r}")
    if on_too_few not in ("raise", "identity"):
        raise ValueError(f"prepare_prior_views: on_too_few must be 'raise' or 'identity', got {on_too_few!r}")
    if views_per_call < 1:
        raise ValueError("prepare_prior_views: views_per_call must be positive")
    dev = torch.device(device)
    out, chunk, chunk_sig = [], [], None

    def flush():
        if chunk:
            out.extend(_prepare_chunk(chunk, dev, seed, method, on_too_few, num_iters, sample_fraction, max_sample_size, best_fraction))
            chunk.clear()

    for i, (info, pts) in enumerate(zip(cam_infos, points)):
        depth = _image(info.depth_image, dev, "depth_image", (1, 3))
        normal = _image(info.normal_image, dev, "normal_image", (3,))
        metal = getattr(info, "metalness_image", None)
        metal = None if metal is None else _image(metal, dev, "metalness_image", (1,))
        if normal.shape[:2] != depth.shape[:2] or (metal is not None and metal.shape[:2] != depth.shape[:2]):
            raise ValueError(f"prepare_prior_views: view {i}: depth, normal and metalness images must share one size")
        sig = (tuple(depth.shape), metal is not None)
        if chunk and (sig != chunk_sig or len(chunk) == views_per_call):
            flush()
        chunk_sig = sig
        chunk.append((i, info, _f32(pts, dev).reshape(-1, 3), depth, normal, metal))
    flush()
    return out


def _prepare_chunk(chunk, dev, seed, method, on_too_few, num_iters, sample_fraction, max_sample_size, best_fraction):
    V = len(chunk)
    H, W = chunk[0][3].shape[:2]
    infos = [c[1] for c in chunk]
    cams = torch.from_numpy(camera_rows(infos, H, W)).to(dev)
    offsets = [0]
    for c in chunk:
        offsets.append(offsets[-1] + c[2].shape[0])
    pts = torch.cat([c[2] for c in chunk]).contiguous()
    depth = torch.stack([c[3] for c in chunk]).contiguous()
    normal = torch.stack([c[4] for c in chunk]).contiguous()
    metal = torch.stack([c[5] for c in chunk]).contiguous() if chunk[0][5] is not None else None
    _, pairs_x, pairs_y, count, dropped = torch.ops.egr.prior_pairs(cams, pts, offsets, depth)
    counts, drops = torch.stack([count, dropped]).cpu().tolist()  # THE read-back of the chunk: the sample sizes and the tables depend on the counts
    for (i, *_), n, d in zip(chunk, counts, drops):
        if n < 2 and on_too_few == "raise":
            raise ValueError(f"prepare_prior_views: view {i} has {n} (predicted, sparse) depth pairs ({d} dropped as not finite): at least 2 are required for the fit")
    sizes = [fit_sizes(n, sample_fraction, max_sample_size, best_fraction) for n in counts]
    table = None
    if method == "ransac":
        width = max(max(s for s, _ in sizes), 1)
        host = np.zeros((V, num_iters, width), np.int32)
        for v, ((i, *_), n, (s, _)) in enumerate(zip(chunk, counts, sizes)):
            if s:
                host[v, :, :s] = sample_table(n, num_iters, sample_fraction, max_sample_size, seed + i)
        table = torch.from_numpy(host)
    ab, best_it, best_err, _, _, _ = torch.ops.egr.prior_fit(pairs_x, pairs_y, counts, [s for s, _ in sizes], [k for _, k in sizes], table, METHODS[method], False)
    distance, world, f0 = torch.ops.egr.prior_finish(cams, ab, depth, normal, metal)
    recs = []
    for v, (i, info, *_) in enumerate(chunk):
        fit = SimpleNamespace(a=ab[v, 0], b=ab[v, 1], num_pairs=counts[v], top_k=sizes[v][1], best_iteration=best_it[v], best_error=best_err[v], dropped=drops[v], fitted=counts[v] >= 2)
        changes = dict(depth_image=distance[v], normal_image=world[v], depth_fit=fit)
        if metal is not None:
            changes["f0_image"] = f0[v]
        recs.append(_record(info, **changes))
    return recs
