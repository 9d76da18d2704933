"""CPU checks of the scene-editing ABI (include/egr_raytracer.h: egr_edit_select, egr_edit_apply, egr_edit_last_error and their four structs): the header text, the
ctypes mirrors, the exported symbols, the two torch ops, the argument validation - which runs before any HIP call, so all of this needs no device -, the packing of
the edit records against fp64 formulas, and the host-side bookkeeping of editing.EditableGaussians (dirty_check, the 32-object limit, duplicate_object's names and
bits on CPU tensors)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import edit_restatement as er

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
WIDTHS = (3, 4, 3, 1, 3, 3, 1, 3)


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


@pytest.fixture(scope="module")
def ed():
    return importlib.import_module(PKG + ".editing")


def error(L):
    return L.egr_edit_last_error().decode()


def header_struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return [re.sub(r"\[.*\]", "", d.strip().split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]


def test_header_declares_the_functions_structs_and_constants(cabi):
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int egr_edit_select(int device, uint32_t n, const float *xyz, const float *f0, const float *roughness, const float *diffuse, "
            "const egr_edit_object *objects, uint32_t num_objects, uint32_t *mask, void *hip_stream);") in hdr
    assert ("int egr_edit_apply(int device, uint32_t n, const egr_edit_arrays *src, const egr_edit_arrays *dst, const uint32_t *mask, "
            "const egr_edit_record *records, uint32_t num_records, void *hip_stream);") in hdr
    assert "const char *egr_edit_last_error(void);" in hdr
    assert "#define EGR_MAX_EDIT_OBJECTS 32" in hdr and cabi.EGR_MAX_EDIT_OBJECTS == 32
    for name in ("EGR_EDIT_SEL_CYLINDER", "EGR_EDIT_SEL_EVERYTHING", "EGR_EDIT_SEL_RANGE_F0", "EGR_EDIT_SEL_RANGE_ROUGHNESS", "EGR_EDIT_SEL_RANGE_DIFFUSE",
                 "EGR_EDIT_SEL_ZRANGE", "EGR_EDIT_ROUGHNESS", "EGR_EDIT_DIFFUSE", "EGR_EDIT_F0", "EGR_EDIT_TRANSFORM", "EGR_EDIT_REMOVED", "EGR_EDIT_ROUGHNESS_OVERRIDE"):
        assert "#define %s %du" % (name, getattr(cabi, name)) in hdr, name
    for name in ("egr_edit_object", "egr_edit_colour", "egr_edit_record", "egr_edit_arrays"):
        assert header_struct_fields(hdr, name) == [f[0] for f in getattr(cabi, name)._fields_], name
    assert [f[0] for f in cabi.egr_edit_arrays._fields_] == list(cabi.EDIT_ARRAYS) == ["scale", "rotation", "mean", "opacity", "rgb", "normal", "roughness", "f0"]
    assert cabi.EDIT_ARRAY_WIDTHS == WIDTHS
    # the contract is written down: inclusive ends, the order of the edits, bit-exact copies, the aliasing rule, the missing attribute
    for word in ("BOTH ENDS INCLUSIVE", "EACH ON THE RESULT OF THE ONE BEFORE", "BIT FOR BIT", "IN PLACE OR DISJOINT", "metalness", "no trigonometry"):
        assert word in hdr, word


def test_struct_sizes_and_offsets(cabi):
    assert C.sizeof(cabi.egr_edit_object) == 68 and C.sizeof(cabi.egr_edit_colour) == 36 and C.sizeof(cabi.egr_edit_record) == 172 and C.sizeof(cabi.egr_edit_arrays) == 64
    o, r = cabi.egr_edit_object, cabi.egr_edit_record
    assert [getattr(o, f).offset for f in ("box_min", "box_max", "sub_min", "range_lo", "range_hi", "flags", "exclude")] == [0, 12, 24, 36, 48, 60, 64]
    assert [getattr(r, f).offset for f in ("flags", "roughness_base", "roughness_shift", "roughness_mult", "diffuse", "f0", "translate", "centre", "scale", "log_scale",
                                           "R", "q")] == [0, 4, 8, 12, 16, 52, 88, 100, 112, 116, 120, 156]


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_edit_select.argtypes) == 10 and len(L.egr_edit_apply.argtypes) == 8
    assert L.egr_edit_last_error.restype is C.c_char_p
    assert L.egr_version().decode()  # additive symbols: the library still answers as before


def test_torch_ops_exist_with_their_schemas():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.edit_select.default._schema) == "egr::edit_select(Tensor xyz, Tensor? f0, Tensor? roughness, Tensor? diffuse, Tensor objects) -> Tensor"
    assert str(torch.ops.egr.edit_apply.default._schema) == "egr::edit_apply(Tensor[] src, Tensor[] dst, Tensor mask, Tensor records) -> ()"
    with pytest.raises(RuntimeError):  # CPU tensors are refused by the shim (there is no CPU path)
        torch.ops.egr.edit_select(torch.zeros(4, 3), None, None, None, torch.zeros((0, 17), dtype=torch.int32))


class Host:
    """Host arrays that stand in for device memory: a call that fails validation never touches them, and that is checked."""

    def __init__(self, n=16):
        self.n = n
        self.src = [np.full((n, w), 1.5 + k, np.float32) for k, w in enumerate(WIDTHS)]
        self.dst = [np.full((n, w), -7.0 - k, np.float32) for k, w in enumerate(WIDTHS)]
        self.mask = np.full(n, 0x5A5A5A5A, np.uint32)
        self.records = np.zeros(32 * 43, np.uint32)
        self.copies = [a.copy() for a in self.src + self.dst + [self.mask, self.records]]

    def untouched(self):
        return all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(self.src + self.dst + [self.mask, self.records], self.copies))

    def table(self, cabi, arrays, **replace):
        ptr = {k: a.ctypes.data for k, a in zip(cabi.EDIT_ARRAYS, arrays)}
        ptr.update(replace)
        return cabi.egr_edit_arrays(**ptr)


def test_select_validation(L, cabi):
    h = Host()
    xyz, mask = h.src[2].ctypes.data, h.mask.ctypes.data
    objs = (cabi.egr_edit_object * 33)()
    assert L.egr_edit_select(0, h.n, xyz, None, None, None, objs, 1, None, None) != 0 and "mask" in error(L)
    assert L.egr_edit_select(0, h.n, xyz, None, None, None, objs, 33, mask, None) != 0 and "EGR_MAX_EDIT_OBJECTS" in error(L)
    assert L.egr_edit_select(0, h.n, xyz, None, None, None, None, 1, mask, None) != 0 and "objects" in error(L)
    assert L.egr_edit_select(0, (1 << 26) + 1, xyz, None, None, None, objs, 1, mask, None) != 0 and "2^26" in error(L)
    assert L.egr_edit_select(0, h.n, None, None, None, None, objs, 1, mask, None) != 0 and "xyz" in error(L)
    for flag in (cabi.EGR_EDIT_SEL_RANGE_F0, cabi.EGR_EDIT_SEL_RANGE_ROUGHNESS, cabi.EGR_EDIT_SEL_RANGE_DIFFUSE):
        objs[1].flags = flag
        assert L.egr_edit_select(0, h.n, xyz, None, None, None, objs, 2, mask, None) != 0 and "range" in error(L)
    objs[1].flags = 0
    objs[0].exclude = 1 << 2
    assert L.egr_edit_select(0, h.n, xyz, None, None, None, objs, 2, mask, None) != 0 and "does not exist" in error(L)
    objs[0].exclude = 0
    assert L.egr_edit_select(0, h.n, xyz, None, None, None, objs, 2, xyz + 4, None) != 0 and "overlaps" in error(L)
    assert h.untouched()
    assert L.egr_edit_select(0, 0, None, None, None, None, objs, 2, mask, None) == 0  # no rows: success, nothing launched (no device here to launch on)
    assert h.untouched()


def test_apply_validation(L, cabi):
    h = Host()
    n, mask, rec = h.n, h.mask.ctypes.data, h.records.ctypes.data
    src, dst = h.table(cabi, h.src), h.table(cabi, h.dst)
    apply = lambda s, d, n=n, mask=mask, rec=rec, k=2: L.egr_edit_apply(0, n, s, d, mask, rec, k, None)
    assert apply(None, dst) != 0 and apply(src, None) != 0 and "src and dst" in error(L)
    assert apply(src, dst, k=33) != 0 and "EGR_MAX_EDIT_OBJECTS" in error(L)
    assert apply(src, dst, n=(1 << 26) + 1) != 0 and "2^26" in error(L)
    assert apply(src, dst, mask=None) != 0 and "mask and records" in error(L)
    assert apply(src, dst, rec=None) != 0 and "mask and records" in error(L)
    for name in cabi.EDIT_ARRAYS:  # every NULL output and input
        assert apply(src, h.table(cabi, h.dst, **{name: None})) != 0 and "NULL" in error(L), name
        assert apply(h.table(cabi, h.src, **{name: None}), dst) != 0 and "NULL" in error(L), name
    # partial overlap: a dst shifted by one word into its own src, a dst on another array's src, two dst on each other, a dst on the mask / the records
    a = {k: x.ctypes.data for k, x in zip(cabi.EDIT_ARRAYS, h.src)}
    assert apply(src, h.table(cabi, h.dst, mean=a["mean"] + 4)) != 0 and "partial overlap" in error(L)
    assert apply(src, h.table(cabi, h.dst, mean=a["mean"] + n * 12 - 4)) != 0 and "partial overlap" in error(L)  # starts in the last word
    assert apply(src, h.table(cabi, h.dst, mean=a["rgb"])) != 0 and "partial overlap" in error(L)  # whole, but ANOTHER array's src
    assert apply(src, h.table(cabi, h.dst, rgb=h.dst[5].ctypes.data)) != 0 and "two dst" in error(L)
    assert apply(src, h.table(cabi, h.dst, opacity=mask)) != 0 and "mask or the records" in error(L)
    assert apply(src, h.table(cabi, h.dst, roughness=rec + 8)) != 0 and "mask or the records" in error(L)
    assert h.untouched()
    # no rows: success, nothing launched - in place (dst IS src) and disjoint alike
    assert apply(src, src, n=0) == 0 and apply(src, dst, n=0) == 0 and apply(src, dst, n=0, k=0, mask=None, rec=None) == 0
    assert h.untouched()


BOX = dict(min=[-1.0, 0.25, 2.0], max=[3.0, 1.25, 2.5])


def test_record_packing_against_fp64_formulas(ed, cabi):
    e = ed.Edit(roughness_shift=-0.2, roughness_mult=1.5, use_roughness_override=True, roughness_override=0.3, diffuse_override=(0.1, 0.2, 0.3, 0.4),
                diffuse_hue_shift=0.7, diffuse_saturation_shift=0.05, diffuse_saturation_mult=1.1, diffuse_value_shift=-0.03, diffuse_value_mult=0.9,
                specular_hue_shift=-1.3, translate_x=0.5, translate_y=-0.25, translate_z=0.125, scale=1.7, rotate_x=20.0, rotate_y=-35.0, rotate_z=50.0)
    r = ed.pack_record(e, BOX)
    f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)
    assert r.flags == cabi.EGR_EDIT_ROUGHNESS | cabi.EGR_EDIT_DIFFUSE | cabi.EGR_EDIT_F0 | cabi.EGR_EDIT_TRANSFORM | cabi.EGR_EDIT_ROUGHNESS_OVERRIDE
    assert r.roughness_base == f32(0.3 ** 2) and r.roughness_shift == f32(0.2) and r.roughness_mult == f32(1.5)  # override^2, |shift|
    assert list(r.diffuse.override_rgb) == list(f32([0.1, 0.2, 0.3])) and r.diffuse.override_w == f32(0.4)
    assert r.diffuse.hue == f32(math.pi * 0.7) and r.f0.hue == f32(-math.pi * 1.3)
    assert (r.diffuse.s_shift, r.diffuse.s_mult, r.diffuse.v_shift, r.diffuse.v_mult) == tuple(f32([0.05, 1.1, -0.03, 0.9]))
    assert (r.f0.override_w, r.f0.s_shift, r.f0.s_mult, r.f0.v_shift, r.f0.v_mult) == (0.0, 0.0, 1.0, 0.0, 1.0)
    assert list(r.translate) == [0.5, -0.25, 0.125] and list(r.centre) == list(f32([1.0 + 0.5, 0.75 - 0.25, 2.25 + 0.125]))  # box centre + translate
    assert r.scale == f32(1.7) and r.log_scale == f32(math.log(1.7))
    R64, q64 = er.rotation_constants(20.0, -35.0, 50.0)  # the quaternion route, against editing.py's Rodrigues formula
    assert np.abs(np.array(list(r.R), np.float64) - R64.reshape(-1)).max() <= 2.0 ** -24 and np.abs(np.array(list(r.q), np.float64) - q64).max() <= 2.0 ** -24
    # one axis-angle vector, not Euler angles: |v| is the angle, v / |v| the axis; and R is a rotation
    v = np.deg2rad([20.0, -35.0, 50.0])
    R, q = ed.rotation_from_axis_angle_degrees(20.0, -35.0, 50.0)
    assert np.allclose(R @ v, v, atol=1e-15) and np.isclose(np.trace(R), 1 + 2 * math.cos(np.linalg.norm(v)), atol=1e-15)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and np.isclose(np.linalg.det(R), 1.0) and np.isclose(q @ q, 1.0)
    assert np.array_equal(ed.rotation_from_axis_angle_degrees(0, 0, 0)[0], np.eye(3))
    # a default edit: no group active, the identity in every field; `removed` alone sets only its flag
    d = ed.pack_record(ed.Edit(), BOX)
    assert d.flags == 0 and list(d.R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(d.q) == [1, 0, 0, 0] and d.log_scale == 0.0 and d.scale == 1.0
    assert ed.pack_record(ed.Edit(removed=True), BOX).flags == cabi.EGR_EDIT_REMOVED
    # each group switches on alone
    for kw, flag in ((dict(roughness_mult=0.5), cabi.EGR_EDIT_ROUGHNESS), (dict(diffuse_value_shift=0.1), cabi.EGR_EDIT_DIFFUSE),
                     (dict(specular_override=(0.5, 0.5, 0.5, 0.2)), cabi.EGR_EDIT_F0), (dict(rotate_y=1.0), cabi.EGR_EDIT_TRANSFORM), (dict(scale=2.0), cabi.EGR_EDIT_TRANSFORM)):
        assert ed.pack_record(ed.Edit(**kw), BOX).flags == flag, kw
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ed.pack_record(ed.Edit(scale=bad), BOX)


def test_edit_fields_follow_the_viewer(ed):
    names = [f.name for f in ed.Edit.__dataclass_fields__.values()]
    assert names == ["roughness_shift", "roughness_mult", "diffuse_override", "diffuse_hue_shift", "diffuse_saturation_shift", "diffuse_saturation_mult", "diffuse_value_shift",
                     "diffuse_value_mult", "use_roughness_override", "roughness_override", "specular_override", "specular_hue_shift", "specular_saturation_shift",
                     "specular_saturation_mult", "specular_value_shift", "specular_value_mult", "translate_x", "translate_y", "translate_z", "scale", "rotate_x", "rotate_y",
                     "rotate_z", "removed"]
    e = ed.Edit()
    assert (e.diffuse_override, e.specular_override, e.scale, e.roughness_mult, e.removed) == ((0.5, 0.5, 0.5, 0.0), (0.5, 0.5, 0.5, 0.0), 1.0, 1.0, False)


def test_object_packing(ed, cabi):
    names = ["a", "b", "everything"]
    o = ed.pack_object("a", dict(min=[0, 0, 0], max=[1, 2, 4], cyl=True, roughness=[0.1, 0.3], f0=[0.5, 1.0], zrange=0.5, exclude=["b"]), names)
    assert o.flags == cabi.EGR_EDIT_SEL_CYLINDER | cabi.EGR_EDIT_SEL_RANGE_F0 | cabi.EGR_EDIT_SEL_RANGE_ROUGHNESS | cabi.EGR_EDIT_SEL_ZRANGE and o.exclude == 2
    assert list(o.sub_min) == [0.5, 1.0, 2.0] and list(o.range_lo) == [0.5, np.float32(0.1), 0.0] and list(o.range_hi) == [1.0, np.float32(0.3), 0.0]
    assert ed.pack_object("everything", dict(min=[0, 0, 0], max=[1, 1, 1]), names).flags == cabi.EGR_EDIT_SEL_EVERYTHING
    with pytest.raises(ValueError, match="metalness"):
        ed.pack_object("a", dict(min=[0, 0, 0], max=[1, 1, 1], metalness=[0, 1]), names)


def cpu_model(n=10, seed=0):
    ren = importlib.import_module(PKG + ".renderer")
    syn = importlib.import_module(PKG + ".synthetic")
    return ren.GaussianParams(syn.random_blob_scene(n, seed=seed), device="cpu")


def boxes(k):
    return {"obj%d" % i: dict(min=[0.0, 0.0, 0.0], max=[1.0 + i, 1.0, 1.0]) for i in range(k)}


def test_dirty_check_and_the_one_upload(ed, monkeypatch):
    launches = []
    monkeypatch.setattr(ed, "_launch_apply", lambda src, dst, mask, records: launches.append(records))
    pc = cpu_model()
    e = ed.EditableGaussians(pc, boxes(2), selection_mask=torch.tensor([1, 2, 3, 0, 1, 1, 2, 2, 3, 0], dtype=torch.int32))
    assert e.is_dirty and e.dirty_check() is True and e.dirty_check() is True  # nothing exported yet: dirty however often it is asked
    native = type("G", (), {f: None for _, f in ed.EXPORT})()
    e.export_edited(native)
    assert e.dirty_check() is False and not e.is_dirty
    e.edits["obj1"].roughness_mult = 0.5
    assert e.dirty_check() is True
    e.export_edited(native)
    assert e.dirty_check() is False
    e.export_edited(native)  # unchanged edits: the packed records are not uploaded again
    assert launches[2] is launches[1] and launches[1] is not launches[0] and launches[0].shape == (2, 43) and launches[0].dtype == torch.int32
    e.edits["obj1"].roughness_mult = 1.0  # back to the first state: differs from the last EXPORTED one
    assert e.dirty_check() is True
    e.export_edited(native)
    e.edits["obj0"] = ed.Edit()  # an equal edit object is not a change
    assert e.dirty_check() is False
    e.edits["obj0"].removed = True
    assert e.dirty_check() is True
    e.export_edited(native)
    # the viewer's global scale: dirty once per change of the value, not on every frame that passes a value other than 1
    assert e.dirty_check(1.5) is True and e.dirty_check(1.5) is False and e.dirty_check(1.5) is False and e.dirty_check(1.0) is True and e.dirty_check() is False
    # a bounding box is the pivot of scale and rotation: moving it is a change like an edit, and its object is packed again
    n_launches = len(launches)
    e.bounding_boxes["obj1"]["max"] = [4.0, 1.0, 1.0]
    assert e.dirty_check() is True
    e.export_edited(native)
    assert e.dirty_check() is False and launches[-1] is not launches[n_launches - 1]
    assert launches[-1][1].tolist() == ed._as_int32([ed.pack_record(e.edits["obj1"], e.bounding_boxes["obj1"])], 43)[0].tolist()
    # the getters' temporaries after a change are an upload that was not exported: still dirty
    e.edits["obj1"].scale = 2.0
    e.edited()
    assert e.dirty_check() is True
    # forwarding: raw attributes, parameters(), cfg
    assert e._xyz is pc._xyz and e.cfg is pc.cfg and all(a is b for a, b in zip(e.parameters(), pc.parameters()))
    assert e.selections.mask is e.selection_mask and e.selections.bits == {"obj0": 0, "obj1": 1}
    assert e.selection("obj0").tolist() == [True, False, True, False, True, True, False, False, True, False]
    assert e.selection("obj1").tolist() == [False, True, True, False, False, False, True, True, True, False]


def test_the_32_object_limit(ed):
    pc = cpu_model()
    with pytest.raises(ValueError, match="32"):
        ed.EditableGaussians(pc, boxes(33), selection_mask=torch.zeros(10, dtype=torch.int32))
    e = ed.EditableGaussians(pc, boxes(32), selection_mask=torch.full((10,), -1, dtype=torch.int32))
    assert e.selection("obj31").all() and e.selection("obj0").all()  # bit 31 is the sign bit of the int32 mask
    before = [getattr(pc, a) for a, _ in ed.EXPORT]
    mask, names = e.selection_mask, list(e.names)
    for call in (lambda: e.duplicate_object("obj3", 0.08), lambda: e.append_object("obj3", [getattr(pc, a)[:2] for a, _ in ed.EXPORT], 0.08)):
        with pytest.raises(ValueError, match="32"):  # a 33rd object: refused before anything is touched (and before any launch: there is no device here)
            call()
    assert all(getattr(pc, a) is t for (a, _), t in zip(ed.EXPORT, before)) and e.selection_mask is mask and e.names == names and "obj3_copy" not in e.edits


def test_duplicate_bookkeeping_on_cpu_tensors(ed):
    pc = cpu_model(n=10, seed=2)
    bb = boxes(2)
    bb["everything"] = dict(min=[-9.0, -9.0, -9.0], max=[9.0, 9.0, 9.0])
    base_mask = torch.tensor([1, 2, 3, 0, 1, 1, 2, 2, 3, 0], dtype=torch.int32) | 4
    e = ed.EditableGaussians(pc, bb, selection_mask=base_mask.clone())
    e.edits["obj1"].translate_y = 0.5
    e.edits["obj1"].roughness_mult = 0.5
    old = {a: getattr(pc, a).clone() for a, _ in ed.EXPORT}
    sel = e.selection("obj1")
    pc._round_counter = torch.arange(10, dtype=torch.int32)  # the reference's model carries this per-row tensor: it grows with the parameters
    count = e.append_object("obj1", [getattr(pc, a)[sel] for a, _ in ed.EXPORT], 0.08)
    assert pc._round_counter.tolist() == list(range(10)) + [1, 2, 6, 7, 8]
    assert count == 5 and e.names == ["obj0", "obj1", "everything", "obj1_copy"] and e.bits["obj1_copy"] == 3 and e.created_objects[-1] == "obj1_copy"
    for a, _ in ed.EXPORT:
        add = old[a][sel]
        if a == "_xyz":
            add = add + 0.08 + torch.tensor([0.0, 0.5, 0.0])
        want = torch.cat((old[a], add))
        got = getattr(pc, a)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and got.grad is not None and got.grad.shape == got.shape and not got.grad.any(), a
    # the new rows belong to the copy ONLY (not to the source, and - as upstream, whose "Everything" never matches its "everything" key - not to `everything`)
    assert torch.equal(e.selection_mask[:10], base_mask) and e.selection_mask[10:].tolist() == [8] * 5
    assert e.selection("obj1_copy").tolist() == [False] * 10 + [True] * 5 and not e.selection("everything")[10:].any() and not e.selection("obj1")[10:].any()
    assert e.edits["obj1_copy"] == ed.Edit() and e.edits["obj1"].roughness_mult == 0.5
    copy_box = e.bounding_boxes["obj1_copy"]  # its own box, shifted by offset + translate; the source's stays
    assert copy_box["min"] == pytest.approx([0.08, 0.58, 0.08], abs=1e-12) and copy_box["max"] == pytest.approx([2.08, 1.58, 1.08], abs=1e-12) and e.bounding_boxes["obj1"] == bb["obj1"]
    assert e.dirty_check() is True
    with pytest.raises(ValueError, match="exists"):
        e.append_object("obj1", [getattr(pc, a)[:1] for a, _ in ed.EXPORT], 0.08)
    with pytest.raises(KeyError):
        e.append_object("nothing", [], 0.08)
