"""Scene editing: the reference's EditableGaussianModel (scene/editable_gaussian_model.py) and the `Edit` state of its viewer
(gaussian_viewer.py:38-68) on the fused kernels of csrc/edit.hip.

`EditableGaussians(pc, bounding_boxes)` wraps a model that holds the raw parameters (`GaussianParams`, or the reference's `GaussianModel`), selects the
objects of `bounding_boxes` ONCE (one launch: a 32-bit membership mask per row) and keeps one `Edit` per object. A `GaussianRaytracer` built on it
exports through `export_edited`: one small upload of the packed edit records (only when they changed) and ONE launch that reads the raw parameters, applies
every object's edit in order and writes the tracer's native tensors - edit and export in one pass. `render_edited` is the viewer's frame.

Deviations from the reference, all deliberate (DESIGN.md "Scene editing" has the reasons):
  * a group of an edit (roughness / diffuse / f0 / transform) whose fields are at their defaults is SKIPPED, so a default `Edit` leaves every row bit for bit;
    the reference pushes every selected row through an HSV round trip and every row through log(exp(s))
  * scale_raw += log(scale) instead of log(exp(s) * scale); rotation = q_R (x) q / |q| (Hamilton product) instead of the matrix round trip: equal up to the
    quaternion's sign, which the tracer's normalisation does not see
  * `removed` is a flag of the edit (exported opacity -1e8, the value the reference's destructive remove_object leaves): clearing it undoes the removal
  * the "metalness" property range of make_editable names an attribute the reference's model does not have: it is refused here
  * duplicate_object gives the copy its own deep-copied box; the reference's viewer aliases the source's box and shifts both
  * at most 32 objects (one bit each)
  * selection_masks (the viewer's selection mode, gaussian_viewer.py:292-321) is ONE primary pass for all objects instead of one full render per object:
    one launch and one seed (the reference gives each object its own launch and jitter and advances total_num_calls by K; here the counter stays);
    no mean(dim=0) over the three equal channels ((x + x + x) / 3 is not always x in fp32); colour edits do not reach the mask (upstream the indicator goes
    through the object's diffuse edit, so a diffuse_override tints every object's mask and breaks the pick) while geometry edits (transform, scale,
    removed) act through the tracer's exported state; no bounce is traced (rgb[0] does not depend on them)
The HSV conventions are kornia's as the reference calls it (hexcone, hue in radians); kornia itself is not a dependency, so parity with it is unpinned."""
import copy
import ctypes as C
import math
import os
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from . import c_abi, load_library
from .renderer import render

MAX_OBJECTS = c_abi.EGR_MAX_EDIT_OBJECTS
# the export order of gaussian_raytracer.py:41-50: raw attribute of the model, field of the native holder
EXPORT = (("_scaling", "scale"), ("_rotation", "rotation"), ("_xyz", "mean"), ("_opacity", "opacity"), ("_diffuse", "rgb"), ("_normal", "normal"),
          ("_roughness", "roughness"), ("_f0", "f0"))
EXTRA_ROW_ATTRS = ("_round_counter",)  # per-row tensors of the reference's GaussianModel that duplicate_object extends along with the eight parameters
RANGE_PROPS = (("f0", c_abi.EGR_EDIT_SEL_RANGE_F0), ("roughness", c_abi.EGR_EDIT_SEL_RANGE_ROUGHNESS), ("diffuse", c_abi.EGR_EDIT_SEL_RANGE_DIFFUSE))


@dataclass(eq=True)
class Edit:
    """gaussian_viewer.py:38-68, field for field (a viewer state maps onto it one to one), plus `removed`."""
    roughness_shift: float = 0.0
    roughness_mult: float = 1.0

    diffuse_override: tuple = (0.5, 0.5, 0.5, 0.0)
    diffuse_hue_shift: float = 0.0
    diffuse_saturation_shift: float = 0.0
    diffuse_saturation_mult: float = 1.0
    diffuse_value_shift: float = 0.0
    diffuse_value_mult: float = 1.0

    use_roughness_override: bool = False
    roughness_override: float = 0.0

    specular_override: tuple = (0.5, 0.5, 0.5, 0.0)
    specular_hue_shift: float = 0.0
    specular_saturation_shift: float = 0.0
    specular_saturation_mult: float = 1.0
    specular_value_shift: float = 0.0
    specular_value_mult: float = 1.0

    translate_x: float = 0.0
    translate_y: float = 0.0
    translate_z: float = 0.0

    scale: float = 1.0

    rotate_x: float = 0.0
    rotate_y: float = 0.0
    rotate_z: float = 0.0

    removed: bool = False


def rotation_from_axis_angle_degrees(rx, ry, rz):
    """(R [3,3], q [4] as (w, x, y, z)) in fp64 of Rodrigues' rotation for the ONE axis-angle vector deg2rad(rx, ry, rz) - not Euler angles."""
    v = np.deg2rad(np.array([rx, ry, rz], np.float64))
    theta = float(np.linalg.norm(v))
    if theta == 0.0:
        return np.eye(3), np.array([1.0, 0.0, 0.0, 0.0])
    k = v / theta
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    R = np.eye(3) + math.sin(theta) * K + (1.0 - math.cos(theta)) * (K @ K)
    return R, np.concatenate([[math.cos(0.5 * theta)], math.sin(0.5 * theta) * k])


def _colour_active(override, hue, s_shift, s_mult, v_shift, v_mult):
    return bool(override[3] != 0.0 or hue != 0.0 or s_shift != 0.0 or s_mult != 1.0 or v_shift != 0.0 or v_mult != 1.0)


def edit_groups(edit):
    """Which of the four groups of `edit` are off their defaults (a group at its defaults is skipped: the identity, bit for bit)."""
    return dict(
        roughness=bool(edit.use_roughness_override or edit.roughness_shift != 0.0 or edit.roughness_mult != 1.0),
        diffuse=_colour_active(edit.diffuse_override, edit.diffuse_hue_shift, edit.diffuse_saturation_shift, edit.diffuse_saturation_mult, edit.diffuse_value_shift,
                               edit.diffuse_value_mult),
        f0=_colour_active(edit.specular_override, edit.specular_hue_shift, edit.specular_saturation_shift, edit.specular_saturation_mult, edit.specular_value_shift,
                          edit.specular_value_mult),
        transform=bool(edit.translate_x != 0.0 or edit.translate_y != 0.0 or edit.translate_z != 0.0 or edit.scale != 1.0 or edit.rotate_x != 0.0 or
                       edit.rotate_y != 0.0 or edit.rotate_z != 0.0))


def edit_constants(edit, box):
    """Everything of an edit that does not depend on the row, in fp64: dict(groups, roughness_base, roughness_shift, hue_diffuse, hue_f0, translate, centre,
    scale, log_scale, R, q). `box`: the object's bounding box (its centre is the pivot of scale and rotation)."""
    if not edit.scale > 0.0:
        raise ValueError(f"Edit.scale must be positive, got {edit.scale}")
    t = np.array([edit.translate_x, edit.translate_y, edit.translate_z], np.float64)
    centre = 0.5 * (np.asarray(box["min"], np.float64) + np.asarray(box["max"], np.float64)) + t
    R, q = rotation_from_axis_angle_degrees(edit.rotate_x, edit.rotate_y, edit.rotate_z)
    return dict(groups=edit_groups(edit), roughness_base=float(edit.roughness_override) ** 2, roughness_shift=abs(float(edit.roughness_shift)),
                hue_diffuse=math.pi * edit.diffuse_hue_shift, hue_f0=math.pi * edit.specular_hue_shift, translate=t, centre=centre, scale=float(edit.scale),
                log_scale=math.log(edit.scale), R=R, q=q)


def pack_record(edit, box):
    """The egr_edit_record of one edit (include/egr_raytracer.h)."""
    k = edit_constants(edit, box)
    g = k["groups"]
    flags = ((c_abi.EGR_EDIT_ROUGHNESS if g["roughness"] else 0) | (c_abi.EGR_EDIT_DIFFUSE if g["diffuse"] else 0) | (c_abi.EGR_EDIT_F0 if g["f0"] else 0) |
             (c_abi.EGR_EDIT_TRANSFORM if g["transform"] else 0) | (c_abi.EGR_EDIT_REMOVED if edit.removed else 0) |
             (c_abi.EGR_EDIT_ROUGHNESS_OVERRIDE if edit.use_roughness_override else 0))
    F3 = C.c_float * 3

    def colour(override, hue, s_shift, s_mult, v_shift, v_mult):
        return c_abi.egr_edit_colour(override_rgb=F3(*override[:3]), override_w=override[3], hue=hue, s_shift=s_shift, s_mult=s_mult, v_shift=v_shift, v_mult=v_mult)

    return c_abi.egr_edit_record(
        flags=flags, roughness_base=k["roughness_base"], roughness_shift=k["roughness_shift"], roughness_mult=edit.roughness_mult,
        diffuse=colour(edit.diffuse_override, k["hue_diffuse"], edit.diffuse_saturation_shift, edit.diffuse_saturation_mult, edit.diffuse_value_shift, edit.diffuse_value_mult),
        f0=colour(edit.specular_override, k["hue_f0"], edit.specular_saturation_shift, edit.specular_saturation_mult, edit.specular_value_shift, edit.specular_value_mult),
        translate=F3(*k["translate"]), centre=F3(*k["centre"]), scale=k["scale"], log_scale=k["log_scale"], R=(C.c_float * 9)(*k["R"].reshape(-1)),
        q=(C.c_float * 4)(*k["q"]))


def pack_object(name, box, names):
    """The egr_edit_object of one entry of bounding_boxes.json: keys min, max, cyl, f0 / roughness / diffuse ([lo, hi]), zrange, exclude (names)."""
    unknown = set(box) - {"min", "max", "cyl", "f0", "roughness", "diffuse", "zrange", "exclude"}
    if unknown:
        raise ValueError(f"bounding box of {name!r}: unknown keys {sorted(unknown)} (the reference's 'metalness' range names an attribute its model does not have)")
    lo, hi = np.asarray(box["min"], np.float32), np.asarray(box["max"], np.float32)
    flags, exclude = 0, 0
    if name == "everything":
        flags |= c_abi.EGR_EDIT_SEL_EVERYTHING
    if "cyl" in box:
        flags |= c_abi.EGR_EDIT_SEL_CYLINDER
    rlo, rhi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    for j, (prop, bit) in enumerate(RANGE_PROPS):
        if prop in box:
            flags |= bit
            rlo[j], rhi[j] = box[prop][0], box[prop][1]
    sub = lo
    if "zrange" in box:
        flags |= c_abi.EGR_EDIT_SEL_ZRANGE
        sub = lo + (hi - lo) * np.asarray(box["zrange"], np.float32)  # fp32, as the reference's tensors compute it
    for other in box.get("exclude", ()):
        exclude |= 1 << names.index(other)
    F3 = C.c_float * 3
    return c_abi.egr_edit_object(box_min=F3(*lo), box_max=F3(*hi), sub_min=F3(*sub), range_lo=F3(*rlo), range_hi=F3(*rhi), flags=flags, exclude=exclude)


def _as_int32(structs, words):
    """A [K, words] int32 CPU tensor holding the bits of K ctypes structs."""
    raw = b"".join(bytes(s) for s in structs)
    return torch.from_numpy(np.frombuffer(raw, np.int32).reshape(len(structs), words).copy())


def _bit_value(k):
    """1 << k as an int32 value (bit 31 is the sign bit: torch has no uint32 arithmetic)."""
    return (1 << k) - (1 << 32) if k == 31 else 1 << k


def _launch_apply(src, dst, mask, records):
    """The one launch of an export (and of the getters' temporaries)."""
    load_library()
    torch.ops.egr.edit_apply(src, dst, mask, records)


class EditableGaussians:
    """A model with per-object edits (see the module docstring). `pc`: the wrapped model; `bounding_boxes`: name -> box, as bounding_boxes.json; the key
    "everything" selects every row. `selection_mask`: a precomputed int32 [N] mask (bit k = k-th key), e.g. a saved one - skips the select launch."""

    def __init__(self, pc, bounding_boxes, selection_mask=None):
        if len(bounding_boxes) > MAX_OBJECTS:
            raise ValueError(f"at most {MAX_OBJECTS} objects (one selection bit each), got {len(bounding_boxes)}")
        self.pc = pc
        self.bounding_boxes = copy.deepcopy(dict(bounding_boxes))
        self.names = list(self.bounding_boxes)
        self.bits = {name: k for k, name in enumerate(self.names)}
        self.edits = {name: Edit() for name in self.names}
        self.created_objects = list(self.names)
        if selection_mask is None:
            load_library()
            objects = [pack_object(name, self.bounding_boxes[name], self.names) for name in self.names]
            need = lambda prop: getattr(pc, "_" + prop).detach() if any(prop in b for b in self.bounding_boxes.values()) else None
            selection_mask = torch.ops.egr.edit_select(pc._xyz.detach(), need("f0"), need("roughness"), need("diffuse"),
                                                       _as_int32(objects, C.sizeof(c_abi.egr_edit_object) // 4) if objects else torch.zeros((0, 17), dtype=torch.int32))
        self.selection_mask = selection_mask
        self.is_dirty = True
        self._packed = {}  # name -> (edit, box, record bytes): what the device records were packed from
        self._records, self._records_version = None, 0  # the packed records on the device; the version counts their uploads
        self._exported_version = None  # the version of the last export (dirty_check compares with it)
        self._last_scaling_modifier = 1.0
        self._edited, self._edited_key = None, None  # the getters' temporaries

    def __getattr__(self, name):  # the raw attributes (_xyz, ...), parameters(), cfg and whatever else the wrapped model has
        if name == "pc":
            raise AttributeError(name)
        return getattr(self.pc, name)

    @property
    def selections(self):
        """The selections as they are held: `mask` (int32 [N], bit k = the row belongs to object k) and `bits` (name -> k)."""
        return SimpleNamespace(mask=self.selection_mask, bits=self.bits)

    def selection(self, name):
        """bool [N]: the rows of object `name`."""
        return ((self.selection_mask >> self.bits[name]) & 1).bool()

    def _stale(self, name):
        c = self._packed.get(name)
        return c is None or c[0] != self.edits[name] or c[1] != self.bounding_boxes[name]

    def dirty_check(self, scaling_modifier=1.0):
        """is_dirty = an edit or a bounding box (the pivot of scale and rotation) differs from the last exported one, nothing was exported yet, or
        `scaling_modifier` (the viewer's global scale, which the caller pushes into the tracer's config) differs from the one the last check saw."""
        modifier_changed = scaling_modifier != self._last_scaling_modifier
        self._last_scaling_modifier = scaling_modifier
        self.is_dirty = (modifier_changed or self._exported_version is None or self._exported_version != self._records_version or
                         any(self._stale(name) for name in self.names))
        return self.is_dirty

    def _device_records(self, device):
        """(the packed records on `device`, their version): an object is packed again only when its edit or its box changed, and any change uploads anew."""
        changed = self._records is None or self._records.device != device
        for name in self.names:
            if self._stale(name):
                edit, box = copy.deepcopy(self.edits[name]), copy.deepcopy(self.bounding_boxes[name])
                self._packed[name] = (edit, box, bytes(pack_record(edit, box)))
                changed = True
        if changed:
            words = C.sizeof(c_abi.egr_edit_record) // 4
            raw = np.frombuffer(b"".join(self._packed[name][2] for name in self.names), np.int32).reshape(len(self.names), words)
            self._records = torch.from_numpy(raw.copy()).to(device)  # the one small upload
            self._records_version += 1
        return self._records, self._records_version

    def _raw(self):
        return [getattr(self.pc, attr).detach() for attr, _ in EXPORT]

    @torch.no_grad()
    def export_edited(self, native_gaussians):
        """Edit and export in one launch: the raw parameters -> the eight native tensors of `native_gaussians` (GaussianRaytracer._export_param_values)."""
        src = self._raw()
        records = self._device_records(src[0].device)[0]
        _launch_apply(src, [getattr(native_gaussians, field) for _, field in EXPORT], self.selection_mask, records)
        self._exported_version = self._records_version

    @torch.no_grad()
    def edited(self):
        """dict raw attribute name -> edited tensor (temporaries written by the same kernel; cached until the edits or the parameters change)."""
        src = self._raw()
        records, version = self._device_records(src[0].device)
        key = (version, tuple((t.data_ptr(), t._version) for t in src), self.selection_mask.data_ptr())
        if self._edited_key != key:
            dst = [torch.empty_like(t) for t in src]
            _launch_apply(src, dst, self.selection_mask, records)
            self._edited, self._edited_key = {attr: t for (attr, _), t in zip(EXPORT, dst)}, key
        return self._edited

    # the getters the reference's EditableGaussianModel overrides
    _get_scaling = property(lambda s: s.edited()["_scaling"])
    _get_rotation = property(lambda s: s.edited()["_rotation"])
    get_scaling = property(lambda s: torch.exp(s.edited()["_scaling"]))
    get_xyz = property(lambda s: s.edited()["_xyz"])
    get_diffuse = property(lambda s: s.edited()["_diffuse"])
    get_normal = property(lambda s: s.edited()["_normal"])
    get_roughness = property(lambda s: s.edited()["_roughness"])
    get_f0 = property(lambda s: s.edited()["_f0"])
    get_opacity_raw = property(lambda s: s.edited()["_opacity"])

    def _check_new_object(self, name):
        if name not in self.bits:
            raise KeyError(name)
        if len(self.names) >= MAX_OBJECTS:
            raise ValueError(f"at most {MAX_OBJECTS} objects: {name + '_copy'!r} would be object {len(self.names) + 1}")
        if name + "_copy" in self.bits:
            raise ValueError(f"{name + '_copy'!r} exists already")

    @torch.no_grad()
    def append_object(self, name, rows, offset):
        """The bookkeeping half of duplicate_object (no launch): `rows` = the eight raw tensors of object `name`'s rows (in EXPORT order) are appended with
        xyz + offset + translate; the new rows belong to `<name>_copy` ONLY (the reference's "Everything" never matches its own "everything" key, so
        not even that one gains them); the copy gets a default Edit and the source's box shifted by offset + translate. Of the wrapped model's other per-row
        tensors only those named in EXTRA_ROW_ATTRS (the reference's `_round_counter`) are extended with the source's rows; optimizer state is not (a model
        that is being edited is not being trained)."""
        self._check_new_object(name)
        edit, new = self.edits[name], name + "_copy"
        delta = [edit.translate_x, edit.translate_y, edit.translate_z]
        count = rows[0].shape[0]
        for (attr, _), add in zip(EXPORT, rows):
            old = getattr(self.pc, attr)
            if attr == "_xyz":
                add = add + offset + torch.tensor(delta, dtype=add.dtype, device=add.device)
            t = torch.cat((old.detach(), add), dim=0).contiguous()
            if old.grad is not None:
                t.grad = torch.zeros_like(t)
            setattr(self.pc, attr, t)
        source_rows = self.selection(name)
        for attr in EXTRA_ROW_ATTRS:  # further per-row tensors of the wrapped model (the reference's _round_counter)
            t = getattr(self.pc, attr, None)
            if torch.is_tensor(t) and t.dim() >= 1 and t.shape[0] == source_rows.shape[0]:
                setattr(self.pc, attr, torch.cat((t, t[source_rows.to(t.device)].clone()), dim=0))
        bit = len(self.names)
        self.selection_mask = torch.cat((self.selection_mask, torch.full((count,), _bit_value(bit), dtype=torch.int32, device=self.selection_mask.device)))
        box = copy.deepcopy(self.bounding_boxes[name])
        for end in ("min", "max"):
            box[end] = [float(box[end][i]) + offset + delta[i] for i in range(3)]
        self.names.append(new)
        self.bits[new] = bit
        self.bounding_boxes[new] = box
        self.edits[new] = Edit()
        self.created_objects.append(new)
        self._exported_version, self._records = None, None  # another object list: uploaded and exported anew
        return count

    @torch.no_grad()
    def duplicate_object(self, name, offset):
        """scene/editable_gaussian_model.py:284-322 + gaussian_viewer.py:244-252: appends a copy of object `name`'s rows as `<name>_copy`. The rows are
        gathered with the fused prune's kernels (one read-back: their count). The caller then calls raytracer.rebuild_bvh(). Returns the number of new rows."""
        self._check_new_object(name)
        src_index, count = torch.ops.egr.prune_select(None, 1.0, 0.0, None, None, None, ~self.selection(name))
        rows = torch.ops.egr.prune_gather(self._raw(), src_index, int(count.item()))
        return self.append_object(name, rows, offset)


def render_edited(camera, raytracer, **kw):
    """One frame of the viewer loop (gaussian_viewer.py:290-341): dirty_check(), then render with force_update_bvh = is_dirty."""
    pc = raytracer.pc
    pc.dirty_check()
    return render(camera, raytracer, force_update_bvh=pc.is_dirty, **kw)


@torch.no_grad()
def selection_masks(camera, raytracer, names=None, znear=0.01, zfar=999.9):
    """The viewer's selection mode (gaussian_viewer.py:292-321) in one call: per-object coverage of `camera`'s view. dirty_check(); if dirty, the edits are
    exported and the tree refitted exactly as `render_edited` would, without a render; then ONE launch (Raytracer.object_masks) composites the primary step once
    and splits every hit's weight over the objects its row belongs to. `names`: the objects asked for, in output order (default: every object but the key
    "everything", in `pc.names` order; copies made by duplicate_object are covered through their own bit).

    Returns SimpleNamespace(names, masks [K,H,W] fp32, hit int32 [H,W], top int32 [H,W]) on the device. masks[j] is, bit for bit, every channel of
    `render(...).rgb[0]` on this tracer with object names[j]'s 0/1 indicator as the diffuse colour and the same seed; hit has bit j set where masks[j] != 0
    (output index 31 is the sign bit); top is the index of the largest mask (ties: the lowest index), -1 where no object covers the pixel. A query: the
    framebuffer, the statistics, random_seeds, total_num_calls, the gradients and the config stay as they were; the next render draws the seed this call
    used. A partitioned tracer traces the whole image on the calling rank, as `render_views` does. See the module docstring for the deviations."""
    pc = raytracer.pc
    names = [n for n in pc.names if n != "everything"] if names is None else list(names)
    bits = [pc.bits[n] for n in names]
    pc.dirty_check()
    if pc.is_dirty:
        raytracer._export_and_update_bvh()
    m = raytracer.cuda_module
    R = torch.from_numpy(camera.R).float() if isinstance(camera.R, np.ndarray) else camera.R
    row_bits = pc.selection_mask.to(m.get_framebuffer().output_rgb.device, torch.int32).contiguous()
    raytracer._set_full_image(True)
    try:
        masks, hit, top = m.object_masks(R, torch.as_tensor(camera.camera_center), float(camera.FoVy), float(os.getenv("ZNEAR", znear)), float(os.getenv("ZFAR", zfar)),
                                         row_bits, bits)
    finally:
        raytracer._set_full_image(False)
    return SimpleNamespace(names=names, masks=masks, hit=hit, top=top)


def pick(result, x, y, rule="last"):
    """The object under pixel (x, y) of a `selection_masks` result, or None where no object covers it: one pixel read back. x and y are clamped to the image,
    as the viewer clamps the cursor. rule="last" is the reference's (gaussian_viewer.py:728-745: the last name in order whose mask is non-zero wins - the
    highest set bit of `hit`); rule="top" returns the object with the largest coverage."""
    if rule not in ("last", "top"):
        raise ValueError(f"rule must be 'last' or 'top', got {rule!r}")
    H, W = result.hit.shape[-2:]
    x, y = min(max(int(x), 0), W - 1), min(max(int(y), 0), H - 1)
    if rule == "top":
        j = int(result.top[y, x])
        return result.names[j] if j >= 0 else None
    h = int(result.hit[y, x]) & 0xFFFFFFFF  # (int32: output index 31 is the sign bit)
    return result.names[h.bit_length() - 1] if h else None
