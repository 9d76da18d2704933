"""From a dataset's views to the first training iteration: the reference's dense initial cloud and the raw parameters made from it.

`dense_init_cloud` is what prepare_initial_ply.py:52-104 computes on the CPU with every pixel of every view in memory: each pixel is unprojected along its
primary ray by the depth image, snapped to a voxel of `1 / voxel_scale`, the diffuse colours are averaged per voxel and the voxels seen by fewer than
`min_count` pixels are dropped. Here the views are STREAMED, `views_per_call` at a time, into a hash table of voxels on the GPU (csrc/initcloud.hip: one launch
per chunk), and the table is sorted and written out once. `VoxelAccumulator` is the same in two steps, for callers that load their views one by one.

`gaussians_from_cloud` is GaussianModel.create_from_pcd (scene/gaussian_model.py:182-230): the eight raw parameter tensors of the cloud, under the names
`synthetic.make_scene` uses, with the isotropic scales from `distCUDA2`.

Deviations from the reference (also in include/egr_raytracer.h and DESIGN.md 8f-7):
  * A pixel is dropped, and counted in `dropped`, when its depth, position or colour is not finite, when a coordinate falls outside [-2^20, 2^20) voxels
    (+-2621 m at the default scale) or when a colour component exceeds `colour_max` in magnitude. Upstream would cast an undefined integer or average a NaN.
  * Colours are the correctly rounded mean of the 2^-32-quantised values (int64 sums: the result does not depend on the order of the views, the chunking, the
    table's capacity or timing); upstream's are a sequential fp32 sum divided by the count. Points, coordinates, counts, the kept set and its order are identical.
  * Views are streamed: memory is that of the table (40 bytes per slot, at least twice the voxels plus the pixels of one chunk), upstream holds every pixel.
  * Pixels of depth 0 are KEPT, as upstream keeps them: they all fall into the camera's own voxel. Mask them (depth = NaN drops a pixel) if that is unwanted.

Not here: the far-field points (add_farfield_points), the dataset's image readers and a command-line script."""
import math
import warnings
from types import SimpleNamespace

import numpy as np
import torch

from . import load_library
from .c_abi import EGR_VOXEL_MIN_CAPACITY, EGR_VOXEL_STATUS_WORDS
from .evaluation import untonemap

DROPPED_WARN_SHARE = 0.01  # extract warns when at least this share of the pixels was dropped


def camera_setup(R, T, FovY):
    """The host fp64 set-up of one view, as prepare_initial_ply.py:58-67 makes it from a CameraInfo: (c2w [3,3] = -R with column 0 negated again, origin [3] =
    -R @ T, view_size = tan(FovY / 2)). There is no trigonometry on the device."""
    R = np.asarray(R.detach().cpu().numpy() if hasattr(R, "detach") else R, np.float64)
    T = np.asarray(T.detach().cpu().numpy() if hasattr(T, "detach") else T, np.float64)
    c2w = R * np.array([1.0, -1.0, -1.0])  # columns 1 and 2 change sign, column 0 is negated twice: exact
    return c2w, -R @ T, math.tan(float(FovY) * 0.5)


def _image(x, device):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).to(device)


class VoxelAccumulator:
    """A growing hash table of voxels on `device`: `add` streams views into it, `extract` sorts it out. The table is three plain tensors (`keys` int64 [cap],
    `acc` int64 [cap,4], `status` int64 [8]); `growths` counts how often it was rebuilt at a larger capacity."""

    def __init__(self, voxel_scale=400.0, colour_max=32768.0, device="cuda", initial_capacity=1 << 22):
        load_library()
        if not voxel_scale > 0:
            raise ValueError("VoxelAccumulator: voxel_scale must be positive")
        if initial_capacity < EGR_VOXEL_MIN_CAPACITY or initial_capacity & (initial_capacity - 1):
            raise ValueError(f"VoxelAccumulator: initial_capacity must be a power of two >= {EGR_VOXEL_MIN_CAPACITY}")
        self.voxel_scale, self.colour_max, self.device = float(voxel_scale), float(colour_max), torch.device(device)
        self.status = torch.zeros(EGR_VOXEL_STATUS_WORDS, dtype=torch.int64, device=self.device)
        self.keys, self.acc = self._table(initial_capacity)
        self.growths, self._table_u8 = 0, None

    def _table(self, cap):
        return torch.full((cap,), -1, dtype=torch.int64, device=self.device), torch.zeros((cap, 4), dtype=torch.int64, device=self.device)

    @property
    def capacity(self):
        return self.keys.shape[0]

    def _reserve(self, pixels):
        """occupied + pixels <= capacity / 2 before every launch: no pixel can fail to find a slot. One read-back of `occupied`."""
        occupied = int(self.status[0].item())
        need = 2 * (occupied + pixels)
        if need <= self.capacity:
            return
        cap = 2 * self.capacity
        while cap < need:
            cap *= 2
        if occupied == 0:  # nothing to keep: the empty table is freed before its successor is allocated, and comes back if that fails
            old_cap = self.capacity
            self.keys = self.acc = None
            try:
                self.keys, self.acc = self._table(cap)
            except BaseException:
                self.keys, self.acc = self._table(old_cap)
                raise
        else:  # the accumulator keeps its table until the larger one is allocated AND filled
            keys, acc = self._table(cap)
            status = self.status.clone()
            status[0].zero_()  # the rehash counts the slots it claims
            torch.ops.egr.voxel_rehash(keys, acc, status, self.keys, self.acc)
            self.keys, self.acc, self.status = keys, acc, status
        self.growths += 1

    def stage(self, group):
        """The arguments of one accumulate launch for `group` (cameras of one size and colour type), on the device: (c2w fp64 [V,3,3], origin fp64 [V,3],
        view_size fp64 [V], depth fp32 [V,H,W], colour fp32 or uint8 [V,H,W,3], the 256-entry table for uint8 colours or None)."""
        setups = [camera_setup(c.R, c.T, c.FovY) for c in group]
        host = np.concatenate([np.stack([s[0] for s in setups]).reshape(-1), np.stack([s[1] for s in setups]).reshape(-1), np.array([s[2] for s in setups])])
        dev, V = torch.from_numpy(host).to(self.device), len(group)  # one upload: [V,3,3], [V,3], [V]
        depth = torch.stack([_image(c.depth_image, self.device).to(torch.float32).reshape(c.depth_image.shape[0], c.depth_image.shape[1]) for c in group]).contiguous()
        colour = torch.stack([_image(c.diffuse_image, self.device) for c in group])
        table = None
        if colour.dtype == torch.uint8:
            if self._table_u8 is None:  # prepare_initial_ply.py:72-73 for the 256 values a byte can take
                self._table_u8 = untonemap(torch.arange(256, device=self.device).float() / 255.0).contiguous()
            table = self._table_u8
        else:
            colour = colour.to(torch.float32)
        H, W = depth.shape[1:]
        if tuple(colour.shape) != (V, H, W, 3):
            raise ValueError(f"VoxelAccumulator.add: diffuse_image must be [{H},{W},3] like the depth image, got {tuple(colour.shape[1:])}")
        return dev[: 9 * V].view(V, 3, 3), dev[9 * V : 12 * V].view(V, 3), dev[12 * V :], depth, colour.contiguous(), table

    def launch(self, staged):
        """One accumulate launch of what `stage` returned, into the table as it is (no growth: `add` reserves room first)."""
        c2w, origin, view_size, depth, colour, table = staged
        torch.ops.egr.voxel_accumulate(self.keys, self.acc, self.status, c2w, origin, view_size, depth, colour, table, self.voxel_scale, self.colour_max, None)

    def _launch(self, group):
        staged = self.stage(group)
        self._reserve(staged[3].numel())
        self.launch(staged)

    @torch.no_grad()
    def add(self, cameras, views_per_call=8):
        """Adds every pixel of `cameras`: objects with `R` [3,3], `T` [3], `FovY`, `depth_image` ([H,W] or [H,W,1]) and `diffuse_image` ([H,W,3], float or uint8)
        as numpy arrays or torch tensors on the host or the device - the fields of the reference's CameraInfo. Up to `views_per_call` consecutive cameras of equal
        size and colour type go into one launch. uint8 colours are un-tonemapped through a 256-entry table; mind that untonemap(255 / 255) is about 1.9e5, above
        the default `colour_max`: such pixels are dropped unless `colour_max` is raised."""
        if views_per_call < 1:
            raise ValueError("VoxelAccumulator.add: views_per_call must be >= 1")
        group, kind = [], None
        for c in cameras:
            k = (tuple(c.depth_image.shape[:2]), str(c.diffuse_image.dtype).endswith("uint8"))
            if group and (k != kind or len(group) == views_per_call):
                self._launch(group)
                group = []
            group.append(c)
            kind = k
        if group:
            self._launch(group)
        return self

    @torch.no_grad()
    def extract(self, min_count=2):
        """The voxels seen by at least `min_count` pixels, in the order of torch.unique(dim=0) (lexicographic on the signed coordinates), as a namespace of device
        tensors `points` fp32 [n,3], `colors` fp32 [n,3], `counts` int32 [n], `coords` int32 [n,3], and the integers `dropped` and `num_pixels` (pixels that
        reached a voxel). The table is left as it is: more views can be added and extracted again."""
        occupied, added, dropped, without_slot = (int(x) for x in self.status[:4].tolist())
        if without_slot:
            raise RuntimeError(f"VoxelAccumulator: {without_slot} pixels found no slot in the table (the table was filled outside add)")
        if dropped and dropped >= DROPPED_WARN_SHARE * (dropped + added):
            warnings.warn(f"VoxelAccumulator: {dropped} of {dropped + added} pixels were dropped (non-finite, out of range, or a colour above colour_max = {self.colour_max}; "
                          "untonemap of a saturated uint8 component is about 1.9e5: pass a larger colour_max for 8-bit images with saturated pixels)", RuntimeWarning, stacklevel=2)
        if occupied == 0:
            e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=self.device)
            return SimpleNamespace(points=e(0, 3), colors=e(0, 3), counts=e(0, dtype=torch.int32), coords=e(0, 3, dtype=torch.int32), dropped=dropped, num_pixels=added)
        coords, points, colors, counts, largest = torch.ops.egr.voxel_extract(self.keys, self.acc, self.status, int(min_count), self.voxel_scale, occupied)
        if largest * self.colour_max >= 2**31:
            raise RuntimeError(f"VoxelAccumulator: a voxel holds {largest} pixels; with colour_max = {self.colour_max} its colour sum may have left int64. "
                               "Pass a smaller colour_max, for instance the configuration's clamp_max")
        return SimpleNamespace(points=points, colors=colors, counts=counts, coords=coords, dropped=dropped, num_pixels=added)


def dense_init_cloud(cameras, voxel_scale=400.0, min_count=2, colour_max=32768.0, device="cuda", views_per_call=8, initial_capacity=1 << 22):
    """prepare_initial_ply.py's dense cloud of `cameras` (see VoxelAccumulator.add for their fields) in one call. Returns the namespace of
    VoxelAccumulator.extract; `formats.save_init_cloud(path, cloud.points.cpu(), cloud.colors.cpu())` writes the reference's point_cloud_dense.ply."""
    return VoxelAccumulator(voxel_scale, colour_max, device, initial_capacity).add(cameras, views_per_call).extract(min_count)


@torch.no_grad()
def gaussians_from_cloud(points, colors, normals=None, init_scale=1.0, init_opa=0.1, init_roughness=0.1, init_f0=0.04, clamp_max=None):
    """GaussianModel.create_from_pcd (scene/gaussian_model.py:182-230): the eight RAW parameter tensors of a cloud, fp32 on the device of `points` (a GPU:
    distCUDA2 has no CPU path), under the names of synthetic.make_scene - mean, rgb (the diffuse colour, clamped to [0, clamp_max] when that is set), normal
    (zeros when none are given, as dataset_readers.py:127-131 passes them), f0, roughness, opacity = log(p / (1 - p)), scale =
    log(sqrt(clamp_min(distCUDA2(points), 1e-7)) * init_scale) three times, rotation = (1, 0, 0, 0)."""
    from .simple_knn import distCUDA2

    mean = torch.as_tensor(points).to(torch.float32).contiguous()
    if not mean.is_cuda:
        raise ValueError("gaussians_from_cloud: points must live on the GPU (distCUDA2 has no CPU path)")
    n, dev = mean.shape[0], mean.device
    on_device = lambda x: torch.as_tensor(x).to(dev, torch.float32).clone()
    constant = lambda value, width: torch.full((n, width), float(value), dtype=torch.float32, device=dev)
    rgb = on_device(colors)
    if clamp_max is not None:
        rgb.clamp_(min=0.0, max=clamp_max)
    spacing = distCUDA2(mean).clamp(min=1e-7).sqrt()  # the distance to the three nearest neighbours, floored as upstream floors the squared one
    p = constant(init_opa, 1)
    rotation = constant(0.0, 4)
    rotation[:, 0] = 1.0  # (filled on the device: a host list would be one more synchronising copy)
    return dict(rgb=rgb, normal=constant(0.0, 3) if normals is None else on_device(normals), f0=constant(init_f0, 3), roughness=constant(init_roughness, 1),
                opacity=(p / (1.0 - p)).log(), scale=(spacing * init_scale).log().unsqueeze(1).expand(n, 3).contiguous(), mean=mean,
                rotation=rotation)
