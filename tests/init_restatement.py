"""The tests' own statement of the dense-init cloud (include/egr_raytracer.h: egr_voxel_*; initialization.py), in fp64 numpy and in the project's words - not the
code under test and not the reference's program text:

  per view      c2w = -R with column 0 negated again, origin = -R @ T, view_size = tan(FovY / 2)
  per pixel     u = (x + 0.5) / W, v = (y + 0.5) / H, cam = ((W / H) view_size (2u - 1), view_size (1 - 2v), -1), dir = cam c2w^T / |cam c2w^T|,
                pos = origin + dir * depth, coord = rint(pos * voxel_scale) (round half to even)
  dropped       depth, position or colour not finite; a coordinate outside [-2^20, 2^20); a colour component above colour_max in magnitude
  per voxel     count, the mean colour in fp64 (np.add.at into fp64 sums), kept if count >= min_count
  order         ascending packed key (x + 2^20) << 42 | (y + 2^20) << 21 | (z + 2^20) = np.unique of the int64 keys
  points        float32(coord) / float32(voxel_scale)

Cameras are objects with R, T, FovY, depth_image [H,W] or [H,W,1] and diffuse_image [H,W,3] (numpy)."""
import math
from types import SimpleNamespace

import numpy as np

HALF = 1 << 20


def pack(coords):
    c = np.asarray(coords, np.int64) + HALF
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


def unpack(keys):
    k = np.asarray(keys, np.int64)
    return (np.stack([k >> 42, (k >> 21) & (2 * HALF - 1), k & (2 * HALF - 1)], -1) - HALF).astype(np.int32)


def setup(cam):
    R, T = np.asarray(cam.R, np.float64), np.asarray(cam.T, np.float64)
    c2w = -R.copy()
    c2w[:, 0] = -c2w[:, 0]
    return c2w, -R @ T, math.tan(float(cam.FovY) * 0.5)


def directions(c2w, view_size, H, W):
    """Unit primary ray directions [H,W,3] in fp64, every operation rounded on its own."""
    u = (np.arange(W, dtype=np.float64) + 0.5) / float(W)
    v = (np.arange(H, dtype=np.float64) + 0.5) / float(H)
    cx = np.broadcast_to(((W / float(H)) * view_size * (2.0 * u - 1.0))[None, :], (H, W))
    cy = np.broadcast_to((view_size * (1.0 - 2.0 * v))[:, None], (H, W))
    d = np.stack([cx * c2w[i, 0] + cy * c2w[i, 1] + (-1.0) * c2w[i, 2] for i in range(3)], -1)
    return d / np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])[..., None]


def positions(cam):
    c2w, origin, view_size = setup(cam)
    depth = np.asarray(cam.depth_image, np.float32)
    H, W = depth.shape[:2]
    return origin + directions(c2w, view_size, H, W) * depth.reshape(H, W, 1).astype(np.float64)


def colours_of(cam, table=None):
    c = np.asarray(cam.diffuse_image)
    return (np.asarray(table, np.float32)[c] if c.dtype == np.uint8 else c.astype(np.float32)).reshape(-1, 3)


def pixels(cameras, voxel_scale, colour_max=32768.0, table=None):
    """Every pixel of every view: (scaled positions fp64 [P,3], colours fp32 [P,3], keep mask [P])."""
    scaled = np.concatenate([positions(c).reshape(-1, 3) for c in cameras]) * float(voxel_scale)
    colour = np.concatenate([colours_of(c, table) for c in cameras])
    depth = np.concatenate([np.asarray(c.depth_image, np.float32).reshape(-1) for c in cameras])
    with np.errstate(invalid="ignore"):
        r = np.rint(scaled)
        keep = np.isfinite(depth) & np.all((r >= -HALF) & (r < HALF), axis=1) & np.all(np.abs(colour.astype(np.float64)) <= colour_max, axis=1)
    return scaled, colour, keep


def half_integer_margin(scaled, keep):
    """The smallest distance of a kept scaled coordinate from a half-integer: the integer results are only defined beyond the arithmetic's own error."""
    s = scaled[keep]
    return float(np.abs(np.abs(s - np.floor(s)) - 0.5).min()) if s.size else 0.5


def cloud(cameras, voxel_scale=400.0, min_count=2, colour_max=32768.0, table=None):
    scaled, colour, keep = pixels(cameras, voxel_scale, colour_max, table)
    keys_all = pack(np.rint(scaled[keep]).astype(np.int64))
    keys, inverse, counts = np.unique(keys_all, return_inverse=True, return_counts=True)
    sums = np.zeros((keys.shape[0], 3), np.float64)
    np.add.at(sums, inverse, colour[keep].astype(np.float64))
    mean = sums / counts[:, None]
    sel = counts >= min_count
    coords = unpack(keys[sel])
    return SimpleNamespace(coords=coords, keys=keys[sel], points=coords.astype(np.float32) / np.float32(voxel_scale), colors=mean[sel], counts=counts[sel].astype(np.int32),
                           dropped=int(np.count_nonzero(~keep)), num_pixels=int(np.count_nonzero(keep)), largest=int(counts.max()) if counts.size else 0,
                           voxels=int(keys.shape[0]), margin=half_integer_margin(scaled, keep), inverse=inverse, all_counts=counts, kept_colours=colour[keep], selected=sel)


def colour_bound(mean64):
    """|colour - mean| allowed: half an fp32 ulp of the value (one rounding) plus 2^-32 (the quantisation step of the fixed-point sums)."""
    return 0.5 * np.spacing(np.abs(mean64).astype(np.float32)).astype(np.float64) + 2.0**-32
