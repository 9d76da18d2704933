"""The training views, resident on the GPU in fp16: the reference's Scene / Camera layer (scene/cameras.py:22-152, scene/scene.py:107-121,
dataset/blender_dataset.py:107-129) as a store that is built once and read by one launch per step (csrc/viewset.hip).

`ViewSet.add` takes the dataset's per-view records as upstream's readers make them (R, T, FovY and up to seven pixel-major images of uint8 or float) and
does, per chunk of views and in ONE launch, what upstream does per image with torch: the area resize to the store's size, the 8-bit conversions of
Camera.__init__, the rounding to half of all seven images, the move to channel-major and the depth minimum / maximum behind autoadjust_zplanes.
`ViewSet.train` turns a batch of view indices into the fp32 arrays the multi-view launch reads in place with ONE gather launch - no per-camera `.to()`,
no `torch.stack`, no host-to-device copy - and then runs the tail of `renderer.train_views`. `ViewSet.camera(i)` is a duck-typed `Camera`, so `render`,
`render_views`, `evaluate_views` and `selection_masks` take a view of the set as they take any camera.

Deviations from the reference, all deliberate:
  * depth / roughness with three channels store CHANNEL 0. That is what cameras.py:71-74 means to do; upstream tests `shape[-1]` after the move to
    channel-major, where it is the width, so its slice never fires and it keeps three planes.
  * the 8-bit conversion tables are DEFINED by the reference's expressions evaluated in half on the CPU (tests/golden/camera_u8_tables.npz pins them); upstream
    evaluates them in half on its GPU, whose pow may round differently. Parity with that is not pinned.
  * a saturated byte (255) of render / diffuse / specular is +inf, as in upstream's images: in half, 1 - y + eps is 1.01e-6 and the quotient overflows. The L1
    sign gradient and tonemap's nan_to_num cope with it.
  * the backward chain still reads fp32 targets: `train` widens the batch into staging buffers kept across steps instead of reading the halfs in the chain.
"""
import random

import numpy as np
import torch

from . import load_library
from .evaluation import untonemap
from .renderer import TRAIN_TARGETS, train_stacked_views

KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")  # the order of every per-kind list (include/egr_raytracer.h)
KIND_CHANNELS = (3, 3, 3, 1, 3, 1, 3)
# the attribute of a dataset record (CameraInfo) and of a Camera per kind
INFO_ATTRS = ("image", "diffuse_image", "specular_image", "depth_image", "normal_image", "roughness_image", "f0_image")
CAMERA_ATTRS = ("original_image", "diffuse_image", "specular_image", "depth_image", "normal_image", "roughness_image", "f0_image")
DEPTH = KINDS.index("depth")
MAX_GATHER = 64  # indices per gather launch (EGR_VIEWSET_MAX_GATHER)


def u8_tables():
    """The three 256-entry half tables of Camera.__init__ (cameras.py:59-70), by the reference's op sequence in half on the CPU: "untonemap" for render / diffuse /
    specular (entry 255 is +inf), "normal" = b / 255 * 2 - 1, "unit" = b / 255 for roughness / f0. CPU half tensors."""
    b = torch.arange(256)
    return {"untonemap": untonemap(b.half() / 255.0), "normal": b.half() / 255.0 * 2.0 - 1.0, "unit": b.half() / 255.0}


TABLE_OF_KIND = ("untonemap", "untonemap", "untonemap", None, "normal", "unit", "unit")  # (uint8 depth is refused, as upstream asserts)


def resized_size(src_height, src_width, height):
    """_resize_image_tensor's output size (blender_dataset.py:112-124) in Python floats: (height, int(height * (src_width / src_height)))."""
    return height, int(height * (src_width / src_height))


class _Sampler:
    """Upstream's viewpoint stack (train.py:218-220): pop(randint(0, len - 1)) without replacement, refilled when empty - also in the middle of a batch."""

    def __init__(self, num_views, seed, views_per_step):
        if num_views < 1 or views_per_step < 1:
            raise ValueError("sampler: an empty view set, or views_per_step < 1")
        self.n, self.rng, self.per_step, self.stack = num_views, random.Random(seed), int(views_per_step), []

    def __iter__(self):
        return self

    def __next__(self):
        batch = []
        for _ in range(self.per_step):
            if not self.stack:
                self.stack = list(range(self.n))
            batch.append(self.stack.pop(self.rng.randint(0, len(self.stack) - 1)))
        return batch


class ViewCamera:
    """One view of a `ViewSet` with the attributes of upstream's `Camera` that this package reads: R (numpy fp32, the dataset's), T, FoVy, camera_center (fp32 on
    the device), znear / zfar (0-dim device tensors, autoadjust_zplanes), image_height / image_width and the seven images as fp32 [C,H,W] device tensors made
    from the stored halfs on every access, like upstream's properties. A kind that no view of the set has is None."""

    def __init__(self, views, index):
        self._views, self.uid = views, index
        self.R, self.T, self.FoVy = views._host_R[index], views._host_T[index], float(views._host_fovy[index])
        self.camera_center = views.centers[index]
        self.image_height, self.image_width = views.height, views.width

    znear = property(lambda s: s._views.znear[s.uid])
    zfar = property(lambda s: s._views.zfar[s.uid])

    def _image(self, kind):
        return self._views.planes[kind][self.uid].float() if self._views.present[kind] else None


for _k, _attr in enumerate(CAMERA_ATTRS):
    setattr(ViewCamera, _attr, property(lambda s, _k=_k: s._image(_k)))


class ViewSet:
    def __init__(self, height, width, num_views, device="cuda", znear_scaledown=0.8, zfar_scaleup=1.5):
        """Room for `num_views` views of `height` x `width` pixels: 17 half planes per view (7 kinds), zeros until a view brings the kind."""
        if height < 1 or width < 1 or num_views < 1:
            raise ValueError("ViewSet: height, width and num_views must be positive")
        load_library()
        self.height, self.width, self.capacity, self.device = int(height), int(width), int(num_views), torch.device(device)
        self.znear_scaledown, self.zfar_scaleup = float(znear_scaledown), float(zfar_scaleup)
        dev = self.device
        self.planes = [torch.zeros((self.capacity, c, self.height, self.width), dtype=torch.float16, device=dev) for c in KIND_CHANNELS]
        self.depth_range = torch.zeros((self.capacity, 2), dtype=torch.float32, device=dev)
        self._R = torch.zeros((self.capacity, 3, 3), dtype=torch.float32, device=dev)
        self._centers = torch.zeros((self.capacity, 3), dtype=torch.float32, device=dev)
        self._fovy = torch.zeros((self.capacity,), dtype=torch.float32, device=dev)
        self._host_R = np.zeros((self.capacity, 3, 3), np.float32)
        self._host_T = np.zeros((self.capacity, 3), np.float32)
        self._host_fovy = np.zeros((self.capacity,), np.float64)
        self._host_centers = np.zeros((self.capacity, 3), np.float64)
        self.present = [False] * len(KINDS)  # whether any view brought the kind
        self.tables_cpu = u8_tables()
        self._tables = {k: t.to(dev) for k, t in self.tables_cpu.items()}
        self._staging, self._staged_rows = None, 0
        self.n = 0

    def __len__(self):
        return self.n

    # ---- the camera table and what autoadjust_zplanes / getNerfppNorm derive
    R = property(lambda s: s._R[: s.n])
    centers = property(lambda s: s._centers[: s.n])
    fovy = property(lambda s: s._fovy[: s.n])
    znear = property(lambda s: s.depth_range[: s.n, 0] * s.znear_scaledown)  # fp32 products, as camera.depth_image.amin() * cfg.znear_scaledown
    zfar = property(lambda s: s.depth_range[: s.n, 1] * s.zfar_scaleup)

    @property
    def max_zfar(self):
        """scene.py:121: the largest zfar of the views, a Python float (synchronises)."""
        if self.n == 0:
            raise ValueError("max_zfar of an empty ViewSet")
        return self.zfar.max().item()

    @property
    def cameras_extent(self):
        """getNerfppNorm's radius (scene/dataset_readers.py:41-62): 1.1 x the largest distance of a camera centre from the mean centre, on the host in fp64."""
        if self.n == 0:
            raise ValueError("cameras_extent of an empty ViewSet")
        c = self._host_centers[: self.n]
        return float(1.1 * np.linalg.norm(c - c.mean(axis=0, keepdims=True), axis=1).max())

    # ---- ingest
    @staticmethod
    def _source(img):
        """A record's image as the ingest takes it: a CPU or device tensor [Hs,Ws,Cs] of uint8 or fp32 (fp16 / fp64 are widened / narrowed to fp32 here)."""
        t = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img))
        if t.dim() == 2:
            t = t.unsqueeze(-1)
        if t.dim() != 3:
            raise ValueError(f"ViewSet.add: an image must be [H,W] or [H,W,C], got {tuple(t.shape)}")
        if t.dtype != torch.uint8:
            if not t.dtype.is_floating_point:
                raise ValueError(f"ViewSet.add: images must be uint8 or floating point, got {t.dtype}")
            t = t.to(torch.float32)
        return t

    def _signature(self, info):
        """(images per kind, (Hs, Ws, per kind (dtype, channels) or None)) of one record; raises where its images disagree on the size or cannot be taken."""
        imgs, sig, size = [], [], None
        for k, attr in enumerate(INFO_ATTRS):
            img = getattr(info, attr, None)
            if img is None:
                imgs.append(None), sig.append(None)
                continue
            t = self._source(img)
            if t.dtype == torch.uint8 and k == DEPTH:
                raise ValueError("ViewSet.add: uint8 depth is refused (the reference asserts the same)")
            if t.shape[2] not in (1, 3) or (t.shape[2] == 1 and KIND_CHANNELS[k] == 3):
                raise ValueError(f"ViewSet.add: {attr} has {t.shape[2]} channels")
            if size is None:
                size = (int(t.shape[0]), int(t.shape[1]))
            elif size != (int(t.shape[0]), int(t.shape[1])):
                raise ValueError(f"ViewSet.add: the images of one view have mixed sizes ({size} and {tuple(t.shape[:2])}): one launch reads one source size")
            imgs.append(t), sig.append((t.dtype, int(t.shape[2])))
        if size is None:
            raise ValueError("ViewSet.add: a view without any image")
        gives = size if size[0] == self.height else resized_size(size[0], size[1], self.height)  # (a source of the store's height is not resized)
        if gives != (self.height, self.width):
            raise ValueError(f"ViewSet.add: a {size[0]} x {size[1]} source gives {gives[0]} x {gives[1]}, the store is {self.height} x {self.width}")
        return imgs, (size, tuple(sig))

    @torch.no_grad()
    def add(self, cam_infos, views_per_call=8):
        """Appends the views of `cam_infos`: records with R, T, FovY (or FoVy) and image / diffuse_image / specular_image / depth_image / normal_image /
        roughness_image / f0_image in the dataset's pixel-major layout (uint8, fp32, or fp16 widened here); a missing or None image leaves that kind's planes zero.
        Consecutive records that share source size, dtypes and channel counts go `views_per_call` at a time: one upload per kind and one launch per chunk."""
        cam_infos = list(cam_infos)
        if self.n + len(cam_infos) > self.capacity:
            raise ValueError(f"ViewSet.add: {len(cam_infos)} more views do not fit: {self.n} of {self.capacity} slots are filled")
        if views_per_call < 1:
            raise ValueError("ViewSet.add: views_per_call must be positive")
        chunk, chunk_sig = [], None
        for info in cam_infos:
            imgs, sig = self._signature(info)
            if chunk and (sig != chunk_sig or len(chunk) == views_per_call):
                self._ingest(chunk)
                chunk = []
            chunk_sig = sig
            chunk.append((info, imgs))
        if chunk:
            self._ingest(chunk)

    def _ingest(self, chunk):
        dev, first, V = self.device, self.n, len(chunk)
        sources, tables = [], []
        for k in range(len(KINDS)):
            if chunk[0][1][k] is None:
                sources.append(None), tables.append(None)
                continue
            sources.append(torch.stack([imgs[k] for _, imgs in chunk]).to(dev).contiguous())  # (stacked where the images are: one upload per kind)
            tables.append(self._tables[TABLE_OF_KIND[k]] if sources[-1].dtype == torch.uint8 else None)
        self._write_cameras(first, [info for info, _ in chunk])
        torch.ops.egr.viewset_ingest(sources, tables, self.planes, self.depth_range, first)
        for k, s in enumerate(sources):
            self.present[k] = self.present[k] or s is not None
        self.n = first + V

    def _write_cameras(self, first, infos):
        """The camera rows of the slots first .. first + len(infos): the host copies, and one upload per array into the device table."""
        dev, V = self.device, len(infos)
        for v, info in enumerate(infos):
            R = np.asarray(info.R, np.float64).reshape(3, 3)
            T = np.asarray(info.T, np.float64).reshape(3)
            self._host_R[first + v], self._host_T[first + v] = R.astype(np.float32), T.astype(np.float32)
            self._host_centers[first + v] = -R @ T  # camera_from_RT: the translation of the inverse world-to-view matrix, in fp64
            self._host_fovy[first + v] = float(info.FovY if hasattr(info, "FovY") else info.FoVy)
        rows = slice(first, first + V)
        self._R[rows] = torch.from_numpy(self._host_R[rows]).to(dev)
        self._centers[rows] = torch.from_numpy(self._host_centers[rows].astype(np.float32)).to(dev)
        self._fovy[rows] = torch.from_numpy(self._host_fovy[rows].astype(np.float32)).to(dev)

    # ---- reading
    def camera(self, i):
        if not 0 <= int(i) < self.n:
            raise IndexError(f"ViewSet.camera: view {i} of {self.n}")
        return ViewCamera(self, int(i))

    def cameras(self):
        return [self.camera(i) for i in range(self.n)]

    def sampler(self, seed, views_per_step=1):
        """An endless iterator of index lists of length `views_per_step` in upstream's order of draws (train.py:218-220) from random.Random(seed)."""
        return _Sampler(self.n, seed, views_per_step)

    def _check_indices(self, idx):
        idx = [int(i) for i in idx]
        if not idx:
            raise ValueError("ViewSet: an empty batch of view indices")
        for i in idx:
            if not 0 <= i < self.n:
                raise IndexError(f"ViewSet: view index {i} is out of range: {self.n} views are filled")
        return idx

    @torch.no_grad()
    def gather(self, idx, kinds=KINDS, out=None):
        """The views `idx` (host integers: any order, repeats allowed) as fp32: dict with kind -> [V,C,H,W] for every kind of `kinds`, and "R" [V,3,3], "centers" [V,3],
        "fovy" [V] - exactly the stored halfs and camera rows, written by one launch per 64 indices. `out`: a dict of buffers with at least V rows to write into
        (as `train` keeps), else new tensors."""
        idx = self._check_indices(idx)
        V, dev = len(idx), self.device
        unknown = set(kinds) - set(KINDS)
        if unknown:
            raise ValueError(f"unknown kinds {sorted(unknown)}; expected some of {KINDS}")
        if out is None:
            out = {k: torch.empty((V, KIND_CHANNELS[KINDS.index(k)], self.height, self.width), dtype=torch.float32, device=dev) for k in kinds}
            out.update(R=torch.empty((V, 3, 3), dtype=torch.float32, device=dev), centers=torch.empty((V, 3), dtype=torch.float32, device=dev),
                       fovy=torch.empty((V,), dtype=torch.float32, device=dev))
        torch.ops.egr.viewset_gather(self.planes, self._R, self._centers, self._fovy, self.n, idx, [out[k] if k in kinds else None for k in KINDS], out["R"], out["centers"],
                                     out["fovy"])
        return {k: t[:V] for k, t in out.items() if k in kinds or k in ("R", "centers", "fovy")}

    def train(self, idx, raytracer, znear=0.01, zfar=999.9):
        """A V-view training step on the views `idx`: leaves what `renderer.train_views([self.camera(i) for i in idx], raytracer)` leaves. ONE gather launch widens the
        batch into staging buffers that live across steps (grown when a larger batch comes), then the tail of `train_views` runs on them in place."""
        if self.n == 0:
            raise ValueError("ViewSet.train: the set is empty")
        idx = self._check_indices(idx)
        if (raytracer.image_height, raytracer.image_width) != (self.height, self.width):
            raise ValueError(f"ViewSet.train: the tracer renders {raytracer.image_height} x {raytracer.image_width}, the views are {self.height} x {self.width}")
        V, dev = len(idx), self.device
        kinds = [k for k, _, _ in TRAIN_TARGETS if self.present[KINDS.index(k)]]  # (a kind no view has: None, the library reads zeros - as train_views passes it)
        if self._staging is None or self._staged_rows < V or set(kinds) - set(self._staging):
            self._staging = {k: torch.empty((V, KIND_CHANNELS[KINDS.index(k)], self.height, self.width), dtype=torch.float32, device=dev) for k in kinds}
            self._staging.update(R=torch.empty((V, 3, 3), dtype=torch.float32, device=dev), centers=torch.empty((V, 3), dtype=torch.float32, device=dev),
                                 fovy=torch.empty((V,), dtype=torch.float32, device=dev))
            self._staged_rows = V
        got = self.gather(idx, kinds, self._staging)
        train_stacked_views(raytracer, got["R"], got["centers"], got["fovy"], [got.get(k) for k, _, _ in TRAIN_TARGETS], znear, zfar)
