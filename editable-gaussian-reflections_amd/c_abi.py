"""ctypes view of include/egr_raytracer.h for hosts WITHOUT torch: the structs mirror the header field for
field, every argument is a raw device pointer or an integer. `RawRaytracer` runs the sequence of the reference's `Raytracer`
constructor and methods (cuda/csrc/raytracer.cpp:45-120) on buffers the caller owns - any allocator that yields HIP device
pointers will do (tests/test_c_abi_direct.py uses torch tensors purely as that allocator and checks the result bit for bit against
the TORCH_LIBRARY shim)."""
import ctypes as C
import os

from . import HIP_LIB_PATH

_F, _U8, _I32 = C.c_void_p, C.c_void_p, C.c_void_p  # all fields are device pointers; the aliases only document the element type


def _struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": fields})


GAUSSIAN_PARAMS = ("rgb", "normal", "f0", "roughness", "opacity", "scale", "mean", "rotation")
GAUSSIAN_GRADS = ("dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation", "total_weight")
CONFIG_FIELDS = ("exp_power", "alpha_threshold", "transmittance_threshold", "accumulate_samples", "jitter_primary_rays", "num_bounces", "global_scale_factor",
                 "loss_weight_diffuse", "loss_weight_specular", "loss_weight_depth", "loss_weight_normal", "loss_weight_f0", "loss_weight_roughness",
                 "eps_forward_normalization", "eps_scale_grad", "eps_ray_surface_offset", "eps_min_roughness", "reflection_invalid_normal_threshold",
                 "backfacing_invalid_normal_threshold", "backfacing_max_dist")
CAMERA_FIELDS = ("origin", "vertical_fov_radians", "rotation_c2w", "rotation_w2c", "znear", "zfar")
FRAMEBUFFER_FIELDS = ("output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance", "output_total_transmittance",
                      "output_ray_origin", "output_ray_direction", "output_final", "output_denoised", "accumulated_rgb", "accumulated_transmittance",
                      "accumulated_total_transmittance", "accumulated_depth", "accumulated_normal", "accumulated_f0", "accumulated_roughness",
                      "accumulated_sample_count", "target_diffuse", "target_specular", "target_depth", "target_normal", "target_f0", "target_roughness")
METADATA_FIELDS = ("grads_enabled", "total_num_calls", "random_seeds")
STATS_FIELDS = ("num_accumulated_per_pixel", "num_traversed_per_pixel")

egr_gaussians = _struct("egr_gaussians", [("count", C.c_uint32)] + [(k, _F) for k in GAUSSIAN_PARAMS + GAUSSIAN_GRADS])
egr_config = _struct("egr_config", [(k, _F) for k in CONFIG_FIELDS])
egr_camera = _struct("egr_camera", [(k, _F) for k in CAMERA_FIELDS])
egr_framebuffer = _struct("egr_framebuffer", [(k, _F) for k in FRAMEBUFFER_FIELDS])
egr_metadata = _struct("egr_metadata", [(k, _F) for k in METADATA_FIELDS])
egr_stats = _struct("egr_stats", [(k, _F) for k in STATS_FIELDS])
egr_counters = _struct("egr_counters", [("rays", C.c_uint64 * 3), ("candidates", C.c_uint64 * 3), ("composited", C.c_uint64 * 3), ("lifetime_rays", C.c_uint64),
                                        ("lifetime_launches", C.c_uint32), ("status", C.c_uint32), ("bvh_depth", C.c_uint32), ("bucket_records", C.c_uint32),
                                        ("device_bytes", C.c_uint64), ("arena_blocks_used", C.c_uint32), ("arena_blocks_cap", C.c_uint32),
                                        ("ext_blocks_used", C.c_uint32), ("ext_blocks_cap", C.c_uint32), ("accepted", C.c_uint64 * 3)])
VIEW_BATCH_OUTPUTS = ("final", "rgb", "depth", "normal", "f0", "roughness")
egr_view_batch = _struct("egr_view_batch", [("num_views", C.c_uint32), ("samples_per_view", C.c_uint32), ("rotation_c2w_dataset", _F), ("camera_center", _F),
                                            ("vertical_fov_radians", _F), ("znear", C.c_float), ("zfar", C.c_float)] + [(k, _F) for k in VIEW_BATCH_OUTPUTS])
TRAIN_BATCH_TARGETS = ("target_diffuse", "target_specular", "target_depth", "target_normal", "target_roughness", "target_f0")
egr_train_batch = _struct("egr_train_batch", [("num_views", C.c_uint32), ("rotation_c2w_dataset", _F), ("camera_center", _F), ("vertical_fov_radians", _F),
                                              ("znear", C.c_float), ("zfar", C.c_float)] + [(k, _F) for k in TRAIN_BATCH_TARGETS])
# per-object coverage of one view (egr_object_masks): the camera of ONE view as egr_view_batch gives it, the membership words, the requested bits (host), outputs
egr_object_mask_query = _struct("egr_object_mask_query", [("rotation_c2w_dataset", _F), ("camera_center", _F), ("vertical_fov_radians", _F), ("znear", C.c_float),
                                                          ("zfar", C.c_float), ("row_bits", C.c_void_p), ("bits", C.POINTER(C.c_uint8)), ("num_bits", C.c_uint32),
                                                          ("masks", _F), ("hit", C.c_void_p), ("top", C.c_void_p)])
EGR_CAMERA_ROTATION_ON_HOST, EGR_CAMERA_CENTER_ON_HOST = 1, 2  # egr_set_camera_from_dataset_ex: that pointer is host memory, read before the call returns
EGR_MAX_PRUNE_ARRAYS = 32
EGR_PRUNE_ROWS_PER_WG = 1024
egr_prune_array = _struct("egr_prune_array", [("src", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_uint32)])
# growing the cloud (csrc/grow.hip): one table entry of egr_grow_append - rows >= n come from `tail` (ROWS) or are the word `fill_bits` (FILL)
EGR_GROW_TAIL_ROWS, EGR_GROW_TAIL_FILL = 0, 1
egr_grow_array = _struct("egr_grow_array", [("src", C.c_void_p), ("dst", C.c_void_p), ("tail", C.c_void_p), ("width", C.c_uint32), ("tail_kind", C.c_uint32),
                                            ("fill_bits", C.c_uint32)])

# scene editing (csrc/edit.hip): selection objects (host), edit records (device) and the two tables of eight arrays
EGR_MAX_EDIT_OBJECTS = 32
EGR_EDIT_SEL_CYLINDER, EGR_EDIT_SEL_EVERYTHING, EGR_EDIT_SEL_RANGE_F0, EGR_EDIT_SEL_RANGE_ROUGHNESS, EGR_EDIT_SEL_RANGE_DIFFUSE, EGR_EDIT_SEL_ZRANGE = 1, 2, 4, 8, 16, 32
EGR_EDIT_ROUGHNESS, EGR_EDIT_DIFFUSE, EGR_EDIT_F0, EGR_EDIT_TRANSFORM, EGR_EDIT_REMOVED, EGR_EDIT_ROUGHNESS_OVERRIDE = 1, 2, 4, 8, 16, 32
_F3 = C.c_float * 3
egr_edit_object = _struct("egr_edit_object", [("box_min", _F3), ("box_max", _F3), ("sub_min", _F3), ("range_lo", _F3), ("range_hi", _F3), ("flags", C.c_uint32),
                                              ("exclude", C.c_uint32)])
egr_edit_colour = _struct("egr_edit_colour", [("override_rgb", _F3), ("override_w", C.c_float), ("hue", C.c_float), ("s_shift", C.c_float), ("s_mult", C.c_float),
                                              ("v_shift", C.c_float), ("v_mult", C.c_float)])
egr_edit_record = _struct("egr_edit_record", [("flags", C.c_uint32), ("roughness_base", C.c_float), ("roughness_shift", C.c_float), ("roughness_mult", C.c_float),
                                              ("diffuse", egr_edit_colour), ("f0", egr_edit_colour), ("translate", _F3), ("centre", _F3), ("scale", C.c_float),
                                              ("log_scale", C.c_float), ("R", C.c_float * 9), ("q", C.c_float * 4)])
EDIT_ARRAYS = ("scale", "rotation", "mean", "opacity", "rgb", "normal", "roughness", "f0")  # the export order of gaussian_raytracer.py:41-50
EDIT_ARRAY_WIDTHS = (3, 4, 3, 1, 3, 3, 1, 3)
egr_edit_arrays = _struct("egr_edit_arrays", [(k, C.c_void_p) for k in EDIT_ARRAYS])


def prune_workspace_bytes(n):
    """EGR_PRUNE_WORKSPACE_BYTES(n) of the header: 16 wave ballots (8 bytes) + 1 count (4 bytes) per EGR_PRUNE_ROWS_PER_WG rows."""
    return ((n + EGR_PRUNE_ROWS_PER_WG - 1) // EGR_PRUNE_ROWS_PER_WG) * (16 * 8 + 4)


EGR_EVAL_PIXELS_PER_WG = 2048


def eval_workspace_bytes(num_views, height, width):
    """EGR_EVAL_WORKSPACE_BYTES(V, H, W) of the header: one partial of 9 fp64 sums per workgroup of EGR_EVAL_PIXELS_PER_WG pixels and view."""
    return num_views * ((height * width + EGR_EVAL_PIXELS_PER_WG - 1) // EGR_EVAL_PIXELS_PER_WG) * (9 * 8)


def _check(rc, last_error):
    """A context-free call's status: non-zero raises the message of its module's egr_<x>_last_error (per module and per thread)."""
    if rc != 0:
        raise RuntimeError(last_error().decode())


def eval_metrics(num_views, height, width, final, rgb, target_final, target_diffuse, target_specular, sse, psnr, workspace, display=None, device=0, stream=0):
    """egr_eval_metrics on integer device addresses (include/egr_raytracer.h has the shapes; None = NULL). `workspace`: eval_workspace_bytes() bytes, 8-byte aligned."""
    L = lib()
    _check(L.egr_eval_metrics(device, num_views, height, width, final, rgb, target_final, target_diffuse, target_specular, sse, psnr, display, workspace, C.c_void_p(stream)), L.egr_eval_last_error)


EGR_SSIM_TILE = 32


def ssim_workspace_bytes(num_views, height, width):
    """EGR_SSIM_WORKSPACE_BYTES(V, H, W) of the header: one partial of 18 fp64 sums per EGR_SSIM_TILE x EGR_SSIM_TILE tile and view."""
    return num_views * ((height + EGR_SSIM_TILE - 1) // EGR_SSIM_TILE) * ((width + EGR_SSIM_TILE - 1) // EGR_SSIM_TILE) * (18 * 8)


def eval_ssim(num_views, height, width, final, rgb, target_final, target_diffuse, target_specular, ssim_sum, ssim, workspace, device=0, stream=0):
    """egr_eval_ssim on integer device addresses (include/egr_raytracer.h has the shapes; None = NULL). `workspace`: ssim_workspace_bytes() bytes, 8-byte aligned."""
    L = lib()
    _check(L.egr_eval_ssim(device, num_views, height, width, final, rgb, target_final, target_diffuse, target_specular, ssim_sum, ssim, workspace, C.c_void_p(stream)), L.egr_eval_last_error)


def ssim_images(num_views, height, width, pred, gt, ssim_sum, ssim, workspace, device=0, stream=0):
    """egr_ssim_images on integer device addresses: pred, gt [V][3][H][W] display images. `workspace`: ssim_workspace_bytes() bytes, 8-byte aligned."""
    L = lib()
    _check(L.egr_ssim_images(device, num_views, height, width, pred, gt, ssim_sum, ssim, workspace, C.c_void_p(stream)), L.egr_eval_last_error)


# evaluation frames (csrc/frames.hip): seven kinds in fixed order, prediction and ground truth as bytes, exact 8-bit metrics
EGR_FRAMES_KINDS, EGR_FRAMES_ALL_KINDS = 7, 0x7F
EGR_FRAMES_ROUND_SAVE, EGR_FRAMES_ROUND_TRUNC = 0, 1
EGR_FRAMES_DEPTH_MAX, EGR_FRAMES_DEPTH_MINMAX = 0, 1
EGR_FRAMES_SEPARATE, EGR_FRAMES_SIDE_BY_SIDE = 0, 1
EGR_FRAMES_PIXELS_PER_WG, EGR_FRAMES_RANGE_BLOCKS = 4096, 64
FRAMES_KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")  # bit k of `kinds`, the order of every per-kind array
FRAMES_PREDICTIONS = ("final", "rgb", "depth", "normal", "roughness", "f0")
egr_frames_args = _struct("egr_frames_args", [(k, C.c_uint32) for k in ("num_views", "height", "width", "kinds", "rounding", "depth_mode", "layout", "reserved")]
                          + [(k, _F) for k in FRAMES_PREDICTIONS] + [("targets", C.c_void_p * EGR_FRAMES_KINDS), ("frames", _U8), ("sse8", C.c_void_p), ("psnr8", C.c_void_p),
                                                                     ("depth_range", _F), ("workspace", C.c_void_p)])


def frames_workspace_bytes(num_views, height, width):
    """EGR_FRAMES_WORKSPACE_BYTES(V, H, W) of the header: per view EGR_FRAMES_RANGE_BLOCKS pairs of uint32 keys and one partial of 21 uint32 sums per workgroup of
    EGR_FRAMES_PIXELS_PER_WG pixels, rounded up to a multiple of 8."""
    return (num_views * (EGR_FRAMES_RANGE_BLOCKS * 8 + ((height * width + EGR_FRAMES_PIXELS_PER_WG - 1) // EGR_FRAMES_PIXELS_PER_WG) * (21 * 4)) + 7) & ~7


def eval_frames(num_views, height, width, frames, sse8, psnr8, workspace, predictions=None, targets=None, kinds=EGR_FRAMES_ALL_KINDS, rounding=EGR_FRAMES_ROUND_SAVE,
                depth_mode=EGR_FRAMES_DEPTH_MAX, layout=EGR_FRAMES_SEPARATE, depth_range=None, device=0, stream=0):
    """egr_eval_frames on integer device addresses (include/egr_raytracer.h has the shapes; None = NULL). `predictions`: dict name of FRAMES_PREDICTIONS -> address;
    `targets`: dict kind name of FRAMES_KINDS -> address. `workspace`: frames_workspace_bytes() bytes, 8-byte aligned."""
    L = lib()
    predictions, targets = predictions or {}, targets or {}
    unknown = (set(predictions) - set(FRAMES_PREDICTIONS)) | (set(targets) - set(FRAMES_KINDS))
    if unknown:
        raise ValueError(f"unknown names {sorted(unknown)}; expected predictions of {FRAMES_PREDICTIONS} and targets of {FRAMES_KINDS}")
    a = egr_frames_args(num_views=num_views, height=height, width=width, kinds=kinds, rounding=rounding, depth_mode=depth_mode, layout=layout, frames=frames, sse8=sse8,
                        psnr8=psnr8, depth_range=depth_range, workspace=workspace, **{k: predictions.get(k) for k in FRAMES_PREDICTIONS})
    for k, name in enumerate(FRAMES_KINDS):
        a.targets[k] = targets.get(name)
    _check(L.egr_eval_frames(device, C.byref(a), C.c_void_p(stream)), L.egr_eval_last_error)


# the dense-init cloud (csrc/initcloud.hip): a hash table of voxels in three caller-owned device buffers
EGR_VOXEL_STATUS_WORDS = 8
EGR_VOXEL_MIN_CAPACITY, EGR_VOXEL_MAX_CAPACITY = 1024, 1 << 31
EGR_VOXEL_COORD_HALF_RANGE = 1 << 20
VOXEL_STATUS = ("occupied", "pixels_added", "pixels_dropped", "pixels_without_slot", "largest_count", "rows")  # status[0..5]


def voxel_pair_bytes(max_rows):
    """EGR_VOXEL_PAIR_BYTES(max_rows) of the header: two (int64 key, uint32 slot) arrays, rounded up to 16 bytes."""
    return (max_rows * 24 + 15) & ~15


def voxel_pack_keys(coords):
    """The table's key of signed voxel coordinates [..., 3] (numpy or anything np.asarray takes): (x + 2^20) << 42 | (y + 2^20) << 21 | (z + 2^20), int64. Its
    integer order is the lexicographic order of the signed triples. Coordinates outside [-2^20, 2^20) raise."""
    import numpy as np

    c = np.asarray(coords).astype(np.int64)
    if c.shape[-1] != 3 or (c.size and (c.min() < -EGR_VOXEL_COORD_HALF_RANGE or c.max() >= EGR_VOXEL_COORD_HALF_RANGE)):
        raise ValueError("voxel_pack_keys: [..., 3] coordinates in [-2^20, 2^20) are required")
    b = c + EGR_VOXEL_COORD_HALF_RANGE
    return (b[..., 0] << 42) | (b[..., 1] << 21) | b[..., 2]


def voxel_unpack_keys(keys):
    """The inverse of voxel_pack_keys: int64 [...] -> int32 [..., 3]."""
    import numpy as np

    k = np.asarray(keys).astype(np.int64)
    return (np.stack([k >> 42, (k >> 21) & 0x1FFFFF, k & 0x1FFFFF], axis=-1) - EGR_VOXEL_COORD_HALF_RANGE).astype(np.int32)


def voxel_accumulate(keys, acc, status, cap, num_views, height, width, c2w, origin, view_size, depth, colour=None, colour_u8=None, colour_table=None, voxel_scale=400.0,
                     colour_max=32768.0, positions_out=None, device=0, stream=0):
    """egr_voxel_accumulate on integer device addresses (include/egr_raytracer.h has the shapes; None = NULL)."""
    L = lib()
    _check(L.egr_voxel_accumulate(device, keys, acc, status, cap, num_views, height, width, c2w, origin, view_size, depth, colour, colour_u8, colour_table, voxel_scale, colour_max,
                                  positions_out, C.c_void_p(stream)), L.egr_voxel_last_error)


def voxel_rehash(keys, acc, status, cap, src_keys, src_acc, src_cap, device=0, stream=0):
    """egr_voxel_rehash on integer device addresses."""
    L = lib()
    _check(L.egr_voxel_rehash(device, keys, acc, status, cap, src_keys, src_acc, src_cap, C.c_void_p(stream)), L.egr_voxel_last_error)


def voxel_extract(keys, acc, status, cap, min_count, voxel_scale, max_rows, coords, points, colors, counts, workspace, workspace_bytes, device=0, stream=0):
    """egr_voxel_extract on integer device addresses; `workspace`: egr_voxel_extract_workspace_bytes(device, max_rows) bytes, 16-byte aligned. Synchronises the stream once.
    Returns (n, largest count)."""
    L = lib()
    host = (C.c_uint64 * 2)()
    _check(L.egr_voxel_extract(device, keys, acc, status, cap, min_count, voxel_scale, max_rows, coords, points, colors, counts, host, workspace, workspace_bytes, C.c_void_p(stream)), L.egr_voxel_last_error)
    return int(host[0]), int(host[1])


# the training views in fp16 (csrc/viewset.hip): one source per kind for egr_viewset_ingest; the store and the outputs of a batch for egr_viewset_gather
EGR_VIEWSET_KINDS, EGR_VIEWSET_DEPTH, EGR_VIEWSET_MAX_GATHER = 7, 3, 64
EGR_VIEWSET_U8, EGR_VIEWSET_F32 = 0, 1
VIEWSET_KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")  # the order of every per-kind array
VIEWSET_CHANNELS = (3, 3, 3, 1, 3, 1, 3)
egr_viewset_source = _struct("egr_viewset_source", [("data", C.c_void_p), ("table", C.c_void_p), ("planes", C.c_void_p), ("channels", C.c_uint32), ("dtype", C.c_uint32)])
egr_viewset_store = _struct("egr_viewset_store", [("planes", C.c_void_p * EGR_VIEWSET_KINDS), ("R", _F), ("centers", _F), ("fovy", _F), ("num_slots", C.c_uint32),
                                                  ("num_filled", C.c_uint32), ("height", C.c_uint32), ("width", C.c_uint32)])
egr_viewset_batch = _struct("egr_viewset_batch", [("targets", C.c_void_p * EGR_VIEWSET_KINDS), ("R", _F), ("centers", _F), ("fovy", _F)])


def viewset_ingest(sources, num_views, src_height, src_width, height, width, first_slot, num_slots, depth_range, device=0, stream=0):
    """egr_viewset_ingest on integer device addresses. `sources`: dict kind name -> (data, table or None, planes, channels, dtype); kinds left out are absent."""
    L = lib()
    unknown = set(sources) - set(VIEWSET_KINDS)
    if unknown:
        raise ValueError(f"unknown kinds {sorted(unknown)}; expected some of {VIEWSET_KINDS}")
    table = (egr_viewset_source * EGR_VIEWSET_KINDS)()
    for k, name in enumerate(VIEWSET_KINDS):
        if name in sources:
            data, tab, planes, channels, dtype = sources[name]
            table[k] = egr_viewset_source(data=data, table=tab, planes=planes, channels=channels, dtype=dtype)
    _check(L.egr_viewset_ingest(device, table, num_views, src_height, src_width, height, width, first_slot, num_slots, depth_range, C.c_void_p(stream)), L.egr_viewset_last_error)


def viewset_gather(planes, R, centers, fovy, num_slots, num_filled, height, width, indices, targets, out_R=None, out_centers=None, out_fovy=None, device=0, stream=0):
    """egr_viewset_gather on integer device addresses. `planes`, `targets`: dicts kind name -> address (kinds left out: none / not wanted); `indices`: host integers."""
    L = lib()
    store = egr_viewset_store(R=R, centers=centers, fovy=fovy, num_slots=num_slots, num_filled=num_filled, height=height, width=width)
    batch = egr_viewset_batch(R=out_R, centers=out_centers, fovy=out_fovy)
    for k, name in enumerate(VIEWSET_KINDS):
        store.planes[k], batch.targets[k] = planes.get(name), targets.get(name)
    idx = (C.c_uint32 * max(len(indices), 1))(*[int(i) for i in indices])
    _check(L.egr_viewset_gather(device, C.byref(store), idx, len(indices), C.byref(batch), C.c_void_p(stream)), L.egr_viewset_last_error)


# prior views (csrc/priors.hip): the arguments of egr_prior_pairs, egr_prior_fit and egr_prior_finish, field for field
EGR_PRIOR_CAM_FLOATS, EGR_PRIOR_MAX_SAMPLE = 25, 1024
EGR_PRIOR_RANSAC, EGR_PRIOR_LSTSQ = 0, 1
_U32P, _I32P = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)  # HOST arrays, read during the call
egr_prior_pairs_args = _struct("egr_prior_pairs_args", [(k, C.c_uint32) for k in ("num_views", "height", "width", "depth_channels")] + [
    ("cams", _F), ("points", _F), ("offsets", _U32P), ("offsets_dev", C.c_void_p), ("depth", _F), ("sparse", _F), ("pairs_x", _F), ("pairs_y", _F), ("count", C.c_void_p),
    ("dropped", C.c_void_p)])
egr_prior_fit_args = _struct("egr_prior_fit_args", [(k, C.c_uint32) for k in ("num_views", "pair_stride", "num_iters", "sample_stride", "method", "reserved")] + [
    ("pairs_x", _F), ("pairs_y", _F), ("views", _U32P), ("views_dev", C.c_void_p), ("samples", _I32P), ("samples_dev", C.c_void_p), ("hyp_error", C.c_void_p), ("hyp_model", _F),
    ("ab", _F), ("best_iteration", C.c_void_p), ("best_error", C.c_void_p), ("inliers", _U8)])
egr_prior_finish_args = _struct("egr_prior_finish_args", [(k, C.c_uint32) for k in ("num_views", "height", "width", "depth_channels")] + [
    ("cams", _F), ("ab", _F), ("depth", _F), ("normal", _F), ("metalness", _F), ("distance", _F), ("normal_out", _F), ("f0", _F)])


def _host_array(ctype, values):
    """A host array of `ctype` for a HOST argument, or NULL for None."""
    if values is None:
        return None
    values = [int(x) for x in values]
    return (ctype * max(len(values), 1))(*values)


def prior_pairs(num_views, height, width, cams, points, offsets, offsets_dev, depth, sparse, pairs_x, pairs_y, count, dropped, depth_channels=1, device=0, stream=0):
    """egr_prior_pairs on integer device addresses (include/egr_raytracer.h has the shapes; None = NULL). `offsets`: the V + 1 host integers; `offsets_dev`: the
    address of their device copy (uint32)."""
    L = lib()
    a = egr_prior_pairs_args(num_views=num_views, height=height, width=width, depth_channels=depth_channels, cams=cams, points=points, offsets=_host_array(C.c_uint32, offsets),
                             offsets_dev=offsets_dev, depth=depth, sparse=sparse, pairs_x=pairs_x, pairs_y=pairs_y, count=count, dropped=dropped)
    _check(L.egr_prior_pairs(device, C.byref(a), C.c_void_p(stream)), L.egr_prior_last_error)


def prior_fit(num_views, pair_stride, pairs_x, pairs_y, views, views_dev, ab, best_iteration, best_error, samples=None, samples_dev=None, num_iters=0, sample_stride=0,
              hyp_error=None, hyp_model=None, inliers=None, method=EGR_PRIOR_RANSAC, device=0, stream=0):
    """egr_prior_fit on integer device addresses. `views`: the flat host integers [V][4] (count, sample_size, top_k, 0); `samples`: the flat host integers
    [V][num_iters][sample_stride]; `views_dev`, `samples_dev`: the addresses of their device copies."""
    L = lib()
    a = egr_prior_fit_args(num_views=num_views, pair_stride=pair_stride, num_iters=num_iters, sample_stride=sample_stride, method=method, pairs_x=pairs_x, pairs_y=pairs_y,
                           views=_host_array(C.c_uint32, views), views_dev=views_dev, samples=_host_array(C.c_int32, samples), samples_dev=samples_dev, hyp_error=hyp_error,
                           hyp_model=hyp_model, ab=ab, best_iteration=best_iteration, best_error=best_error, inliers=inliers)
    _check(L.egr_prior_fit(device, C.byref(a), C.c_void_p(stream)), L.egr_prior_last_error)


def prior_finish(num_views, height, width, cams, ab, depth, normal, distance, normal_out, metalness=None, f0=None, depth_channels=1, device=0, stream=0):
    """egr_prior_finish on integer device addresses (None = NULL)."""
    L = lib()
    a = egr_prior_finish_args(num_views=num_views, height=height, width=width, depth_channels=depth_channels, cams=cams, ab=ab, depth=depth, normal=normal, metalness=metalness,
                              distance=distance, normal_out=normal_out, f0=f0)
    _check(L.egr_prior_finish(device, C.byref(a), C.c_void_p(stream)), L.egr_prior_last_error)


_lib = None


def lib(path=None):
    """dlopen libegr_hip.so and declare the prototypes of include/egr_raytracer.h."""
    global _lib
    if _lib is None:
        path = path or HIP_LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: build it first (there is no CPU fallback)")
        L = C.CDLL(path)
        P = C.c_void_p
        L.egr_create.argtypes = [C.POINTER(P), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64]
        L.egr_destroy.argtypes = [P]
        L.egr_destroy.restype = None
        L.egr_bind.argtypes = [P, C.POINTER(egr_camera), C.POINTER(egr_config), C.POINTER(egr_framebuffer), C.POINTER(egr_metadata), C.POINTER(egr_stats)]
        L.egr_set_gaussians.argtypes = [P, C.POINTER(egr_gaussians)]
        for name in ("egr_rebuild_bvh", "egr_update_bvh", "egr_denoise", "egr_reset_lifetime_counters", "egr_debug_check_bvh"):
            getattr(L, name).argtypes = [P, P]
        L.egr_raytrace.argtypes = [P, C.c_int, P]
        L.egr_update_bvh_ex.argtypes = [P, C.c_uint, P]
        L.egr_update_bvh_from.argtypes = [P, C.POINTER(egr_gaussians), C.c_uint, P]  # ctx, src (its eight parameter pointers), flags, stream
        L.egr_raytrace_import.argtypes = [P, C.POINTER(egr_gaussians), P]  # ctx, dst (its eight dL_d* pointers), stream
        L.egr_raytrace_targets.argtypes = [P, C.c_int, C.POINTER(egr_gaussians), C.POINTER(P * 6), P]  # ctx, grads_enabled, dst or NULL, six target images or NULL, stream
        L.egr_debug_get_backward_records.argtypes = [P, P, P]  # ctx, host out [n][4][4] floats, stream
        L.egr_set_partition.argtypes = [P, C.c_int, C.c_int]
        L.egr_set_exact_stats.argtypes = [P, C.c_int]
        L.egr_set_grad_overwrite.argtypes = [P, C.c_int]
        L.egr_grad_delta_consumed.argtypes = [P]
        L.egr_debug_set_pixel_mask.argtypes = [P, P]
        L.egr_set_targets_chw.argtypes = [P, P, P, P, P, P, P, P]
        L.egr_set_camera_from_dataset.argtypes = [P, P, P, C.c_float, C.c_float, C.c_float, P]
        L.egr_set_camera_from_dataset_ex.argtypes = [P, P, P, C.c_float, C.c_float, C.c_float, C.c_uint, P]  # ... flags (EGR_CAMERA_*_ON_HOST: that pointer is host memory), stream
        L.egr_tile_owner.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.egr_tile_owner.restype = C.c_int
        L.egr_set_strands.argtypes = [P, C.c_int]
        L.egr_set_rays_per_task.argtypes = [P, C.c_int]
        L.egr_set_team_help.argtypes = [P, C.c_int]
        L.egr_render_views.argtypes = [P, C.POINTER(egr_view_batch), P]
        L.egr_set_batch_frames.argtypes = [P, C.c_int]
        L.egr_object_masks.argtypes = [P, C.POINTER(egr_object_mask_query), P]
        L.egr_train_views.argtypes = [P, C.POINTER(egr_train_batch), P]
        L.egr_train_views_import.argtypes = [P, C.POINTER(egr_train_batch), C.POINTER(egr_gaussians), P]
        L.egr_get_counters.argtypes = [P, C.POINTER(egr_counters), P]
        L.egr_get_counters_ex.argtypes = [P, P, C.c_size_t, P]
        # fused prune (csrc/prune.hip): device, n, total_weight, divisor, min_weight, points, cam_centers, cam_znear, num_cams, remove_mask, src_index, count, workspace, stream
        L.egr_prune_select.argtypes = [C.c_int, C.c_uint32, P, C.c_float, C.c_float, P, P, P, C.c_uint32, P, P, P, P, P]
        L.egr_prune_gather.argtypes = [C.c_int, C.POINTER(egr_prune_array), C.c_int, C.c_uint32, P, C.c_uint32, P]  # device, table, entries, n, src_index, count, stream
        L.egr_prune_last_error.argtypes = []
        L.egr_prune_last_error.restype = C.c_char_p
        # growing the cloud (csrc/grow.hip). sample: device, first, n, seed, radius, clamp, out_points, stream; append: device, table, entries, n, m, stream
        L.egr_grow_sample.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_uint64, C.c_float, C.c_float, P, P]
        L.egr_grow_append.argtypes = [C.c_int, C.POINTER(egr_grow_array), C.c_int, C.c_uint32, C.c_uint32, P]
        L.egr_grow_last_error.argtypes = []
        L.egr_grow_last_error.restype = C.c_char_p
        # scene editing (csrc/edit.hip): device, n, xyz, f0, roughness, diffuse, objects (host), num_objects, mask, stream
        L.egr_edit_select.argtypes = [C.c_int, C.c_uint32, P, P, P, P, C.POINTER(egr_edit_object), C.c_uint32, P, P]
        L.egr_edit_apply.argtypes = [C.c_int, C.c_uint32, C.POINTER(egr_edit_arrays), C.POINTER(egr_edit_arrays), P, P, C.c_uint32, P]  # device, n, src, dst, mask, records (device), num_records, stream
        L.egr_edit_last_error.argtypes = []
        L.egr_edit_last_error.restype = C.c_char_p
        L.egr_denoise_views.argtypes = [P, C.c_uint32, P, P, C.c_size_t, P, P]  # ctx, num_views, final, normal, normal_view_stride (floats), denoised, stream
        # fused evaluation metrics (csrc/eval.hip): device, V, H, W, final, rgb, target_final, target_diffuse, target_specular, sse, psnr, display, workspace, stream
        L.egr_eval_metrics.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P, P, P, P, P, P, P]
        L.egr_eval_last_error.argtypes = []
        L.egr_eval_last_error.restype = C.c_char_p
        # fused SSIM (csrc/ssim.hip): device, V, H, W, final, rgb, target_final, target_diffuse, target_specular, ssim_sum, ssim, workspace, stream
        L.egr_eval_ssim.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P, P, P, P, P, P]
        L.egr_ssim_images.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P, P, P]  # device, V, H, W, pred, gt, ssim_sum, ssim, workspace, stream
        L.egr_eval_frames.argtypes = [C.c_int, C.POINTER(egr_frames_args), P]  # evaluation frames (csrc/frames.hip): device, args, stream
        # the dense-init cloud (csrc/initcloud.hip). accumulate: device, keys, acc, status, cap, V, H, W, c2w, origin, view_size, depth, colour, colour_u8, colour_table,
        # voxel_scale, colour_max, positions_out, stream
        L.egr_voxel_accumulate.argtypes = [C.c_int, P, P, P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, P, P, P, P, P, P, P, C.c_double, C.c_double, P, P]
        L.egr_voxel_rehash.argtypes = [C.c_int, P, P, P, C.c_uint64, P, P, C.c_uint64, P]  # device, keys, acc, status, cap, src_keys, src_acc, src_cap, stream
        L.egr_voxel_extract_workspace_bytes.argtypes = [C.c_int, C.c_uint64]
        L.egr_voxel_extract_workspace_bytes.restype = C.c_size_t
        # extract: device, keys, acc, status, cap, min_count, voxel_scale, max_rows, coords, points, colors, counts, host_rows_and_largest, workspace, workspace_bytes, stream
        L.egr_voxel_extract.argtypes = [C.c_int, P, P, P, C.c_uint64, C.c_uint32, C.c_double, C.c_uint64, P, P, P, P, C.POINTER(C.c_uint64 * 2), P, C.c_size_t, P]
        L.egr_voxel_last_error.argtypes = []
        L.egr_voxel_last_error.restype = C.c_char_p
        # the training views in fp16 (csrc/viewset.hip). ingest: device, sources [7], V, Hs, Ws, H, W, first_slot, num_slots, depth_range, stream;
        # gather: device, store, indices (host), V, out, stream
        L.egr_viewset_ingest.argtypes = [C.c_int, C.POINTER(egr_viewset_source), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P, P]
        L.egr_viewset_gather.argtypes = [C.c_int, C.POINTER(egr_viewset_store), C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(egr_viewset_batch), P]
        L.egr_viewset_last_error.argtypes = []
        L.egr_viewset_last_error.restype = C.c_char_p
        # prior views (csrc/priors.hip): device, args, stream each
        L.egr_prior_pairs.argtypes = [C.c_int, C.POINTER(egr_prior_pairs_args), P]
        L.egr_prior_fit.argtypes = [C.c_int, C.POINTER(egr_prior_fit_args), P]
        L.egr_prior_finish.argtypes = [C.c_int, C.POINTER(egr_prior_finish_args), P]
        L.egr_prior_last_error.argtypes = []
        L.egr_prior_last_error.restype = C.c_char_p
        L.egr_last_error.argtypes = [P]
        L.egr_last_error.restype = C.c_char_p
        L.egr_version.restype = C.c_char_p
        _lib = L
    return _lib


class RawRaytracer:
    """The reference's `Raytracer` life cycle on caller-owned device buffers.

    `pointers`: dict name -> integer device address for every field of the six structs above (see the *_FIELDS tuples);
    `count`: number of gaussians; `stream`: a hipStream_t as an integer (0 = the NULL stream)."""

    def __init__(self, width, height, count, pointers, ppll_forward_size=180_000_000, ppll_backward_size=120_000_000, device=0, stream=0):
        self.L = lib()
        self.stream = C.c_void_p(stream)
        self.ctx = C.c_void_p()
        if self.L.egr_create(C.byref(self.ctx), device, width, height, ppll_forward_size, ppll_backward_size) != 0:  # raytracer.cpp:45-60
            raise RuntimeError("egr_create failed: no usable HIP device (there is no CPU fallback)")
        fill = lambda st, names: st(**{k: pointers[k] for k in names})
        self.cam, self.cfg = fill(egr_camera, CAMERA_FIELDS), fill(egr_config, CONFIG_FIELDS)
        self.fb, self.meta, self.stats = fill(egr_framebuffer, FRAMEBUFFER_FIELDS), fill(egr_metadata, METADATA_FIELDS), fill(egr_stats, STATS_FIELDS)
        self._check(self.L.egr_bind(self.ctx, C.byref(self.cam), C.byref(self.cfg), C.byref(self.fb), C.byref(self.meta), C.byref(self.stats)))  # :61-68
        self.set_gaussians(count, pointers)
        self.rebuild_bvh()  # :76-78

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.egr_last_error(self.ctx).decode())  # C++ exceptions upstream -> RuntimeError in Python

    def set_gaussians(self, count, pointers):  # Raytracer::resize (:112-120): the holder re-reifies, the struct is uploaded again
        self.g = egr_gaussians(count=count, **{k: pointers[k] for k in GAUSSIAN_PARAMS + GAUSSIAN_GRADS})
        self._check(self.L.egr_set_gaussians(self.ctx, C.byref(self.g)))

    def rebuild_bvh(self):  # :102-110
        self._check(self.L.egr_rebuild_bvh(self.ctx, self.stream))

    def update_bvh(self, fuse_live=False):  # :100 (fuse_live: egr_update_bvh_ex with EGR_UPDATE_FUSE_LIVE)
        if fuse_live:
            self._check(self.L.egr_update_bvh_ex(self.ctx, 1, self.stream))
        else:
            self._check(self.L.egr_update_bvh(self.ctx, self.stream))

    def update_bvh_from(self, pointers, fuse_live=False):
        """egr_update_bvh_from: export and refit in one pass. `pointers`: dict with the integer device addresses of the caller's eight parameter
        arrays (GAUSSIAN_PARAMS); the bound arrays then hold their values."""
        src = egr_gaussians(count=self.g.count, **{k: pointers[k] for k in GAUSSIAN_PARAMS})
        self._check(self.L.egr_update_bvh_from(self.ctx, C.byref(src), 1 if fuse_live else 0, self.stream))

    def raytrace(self, grads_enabled):  # :81-94
        self._check(self.L.egr_raytrace(self.ctx, 1 if grads_enabled else 0, self.stream))

    def raytrace_import(self, pointers):
        """egr_raytrace_import: a grad launch whose gather also adds the bound gradient arrays to the caller's. `pointers`: dict with the integer
        device addresses of the caller's eight gradient arrays (GAUSSIAN_GRADS without total_weight)."""
        dst = egr_gaussians(count=self.g.count, **{k: pointers[k] for k in GAUSSIAN_GRADS[:8]})
        self._check(self.L.egr_raytrace_import(self.ctx, C.byref(dst), self.stream))

    def raytrace_targets(self, grads_enabled=True, import_into=None, targets=None):
        """egr_raytrace_targets: a launch that reads its target images where the caller keeps them. `import_into`: as raytrace_import's `pointers`, or
        None; `targets`: six integer device addresses of contiguous fp32 [C,H,W] images in the order of TRAIN_BATCH_TARGETS (None / 0 = absent = zeros), or None for the
        framebuffer's target buffers. The images must stay valid and unmodified until the launch has completed."""
        dst = None if import_into is None else C.byref(egr_gaussians(count=self.g.count, **{k: import_into[k] for k in GAUSSIAN_GRADS[:8]}))
        planes = None if targets is None else C.byref((C.c_void_p * 6)(*[t or None for t in targets]))
        self._check(self.L.egr_raytrace_targets(self.ctx, 1 if grads_enabled else 0, dst, planes, self.stream))

    def render_views(self, num_views, samples_per_view, rotation_c2w_dataset, camera_center, vertical_fov_radians, znear=0.01, zfar=999.9, **outputs):
        """egr_render_views: the camera arrays and `outputs` (final= required; rgb=, depth=, normal=, f0=, roughness= optional) are integer
        device addresses of the caller's buffers (include/egr_raytracer.h: egr_view_batch has their shapes)."""
        unknown = set(outputs) - set(VIEW_BATCH_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}; expected some of {VIEW_BATCH_OUTPUTS}")
        b = egr_view_batch(num_views=num_views, samples_per_view=samples_per_view, rotation_c2w_dataset=rotation_c2w_dataset, camera_center=camera_center,
                           vertical_fov_radians=vertical_fov_radians, znear=znear, zfar=zfar, **{k: outputs.get(k) for k in VIEW_BATCH_OUTPUTS})
        self._check(self.L.egr_render_views(self.ctx, C.byref(b), self.stream))

    def train_views(self, num_views, rotation_c2w_dataset, camera_center, vertical_fov_radians, znear=0.01, zfar=999.9, **targets):
        """egr_train_views: the camera arrays and `targets` (target_diffuse=, target_specular=, target_depth=, target_normal=, target_roughness=,
        target_f0=; each optional, absent = zeros) are integer device addresses of the caller's buffers (include/egr_raytracer.h: egr_train_batch
        has their shapes)."""
        unknown = set(targets) - set(TRAIN_BATCH_TARGETS)
        if unknown:
            raise ValueError(f"unknown targets {sorted(unknown)}; expected some of {TRAIN_BATCH_TARGETS}")
        b = egr_train_batch(num_views=num_views, rotation_c2w_dataset=rotation_c2w_dataset, camera_center=camera_center, vertical_fov_radians=vertical_fov_radians,
                            znear=znear, zfar=zfar, **{k: targets.get(k) for k in TRAIN_BATCH_TARGETS})
        self._check(self.L.egr_train_views(self.ctx, C.byref(b), self.stream))

    def object_masks(self, rotation_c2w_dataset, camera_center, vertical_fov_radians, row_bits, bits, masks, hit=None, top=None, znear=0.01, zfar=999.9):
        """egr_object_masks: per-object coverage of one view. The camera arrays, `row_bits` (uint32 [count]), `masks` (fp32 [K][H][W]) and the optional `hit`
        (uint32 [H][W]) / `top` (int32 [H][W]) are integer device addresses; `bits`: the K requested selection bits (host integers) in output order."""
        bits = [int(b) for b in bits]
        if any(b < 0 or b > 255 for b in bits):
            raise ValueError(f"selection bits must fit a byte, got {bits}")
        b8 = (C.c_uint8 * max(len(bits), 1))(*bits)
        q = egr_object_mask_query(rotation_c2w_dataset=rotation_c2w_dataset, camera_center=camera_center, vertical_fov_radians=vertical_fov_radians, znear=znear, zfar=zfar,
                                  row_bits=row_bits, bits=C.cast(b8, C.POINTER(C.c_uint8)), num_bits=len(bits), masks=masks, hit=hit, top=top)
        self._check(self.L.egr_object_masks(self.ctx, C.byref(q), self.stream))

    def set_batch_frames(self, frames):
        self._check(self.L.egr_set_batch_frames(self.ctx, frames))

    def denoise(self):  # :96
        self._check(self.L.egr_denoise(self.ctx, self.stream))

    def denoise_views(self, num_views, final, normal, normal_view_stride, denoised):
        """egr_denoise_views: integer device addresses of final [V][H][W][3], the guide (view v at normal + v * normal_view_stride floats) and the output."""
        self._check(self.L.egr_denoise_views(self.ctx, num_views, final, normal, normal_view_stride, denoised, self.stream))

    def counters(self):  # synchronises the stream; the sized call: the library never writes more than THIS mirror of the struct holds
        c = egr_counters()
        self._check(self.L.egr_get_counters_ex(self.ctx, C.byref(c), C.sizeof(c), self.stream))
        return c

    def close(self):
        if self.ctx:
            self.L.egr_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
