"""CPU checks of the per-object coverage ABI (include/egr_raytracer.h: egr_object_mask_query, egr_object_masks): the header text, the ctypes mirror's layout, the
exported symbol and its prototype, the shim method, the refusals that need no GPU, the unchanged library version - and editing.pick on hand-made results."""
import ctypes as C
import importlib
import os
import re
from types import SimpleNamespace

import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")


def header_fields(struct):
    hdr = open(HEADER).read()
    body = re.search(r"typedef struct " + struct + r" \{(.*?)\} " + struct + ";", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[.*?\]", "", part.strip().split()[-1].lstrip("*")) for decl in body.split(";") if decl.strip() for part in decl.split(",")]


def test_header_states_the_contract():
    hdr = open(HEADER).read()
    assert re.search(r"\bint egr_object_masks\(egr_context \*ctx, const egr_object_mask_query \*q, void \*hip_stream\);", hdr)
    text = " ".join(hdr.split())
    for phrase in ("sum in hit order, fp32", "c + rem * (c * inv_norm)", "total_num_calls + 1", "ties go to the lowest index", "a NaN never wins", "-1 where hit == 0",
                   "exact-statistics", "egr_version() is unchanged", "BEFORE any HIP call"):
        assert phrase in text, phrase


def test_query_mirror_matches_the_header():
    cabi = importlib.import_module(PKG + ".c_abi")
    q = cabi.egr_object_mask_query
    want = ["rotation_c2w_dataset", "camera_center", "vertical_fov_radians", "znear", "zfar", "row_bits", "bits", "num_bits", "masks", "hit", "top"]
    assert [f[0] for f in q._fields_] == header_fields("egr_object_mask_query") == want
    # the C layout on LP64: three pointers, two floats, two pointers, one uint32 + padding, three pointers
    offsets = {name: getattr(q, name).offset for name in want}
    assert offsets == dict(rotation_c2w_dataset=0, camera_center=8, vertical_fov_radians=16, znear=24, zfar=28, row_bits=32, bits=40, num_bits=48, masks=56, hit=64, top=72)
    assert C.sizeof(q) == 80
    assert getattr(q, "num_bits").size == 4 and getattr(q, "znear").size == 4
    assert cabi.EGR_MAX_EDIT_OBJECTS == 32 and re.search(r"#define EGR_MAX_EDIT_OBJECTS 32\b", open(HEADER).read())


def test_entry_point_is_exported_and_declared():
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    assert hasattr(L, "egr_object_masks")
    assert L.egr_object_masks.argtypes == [C.c_void_p, C.POINTER(cabi.egr_object_mask_query), C.c_void_p]
    assert L.egr_object_masks.restype is C.c_int
    assert callable(getattr(cabi.RawRaytracer, "object_masks"))


def test_null_context_is_refused_not_dereferenced():
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    bits = (C.c_uint8 * 1)(0)
    q = cabi.egr_object_mask_query(row_bits=8, bits=C.cast(bits, C.POINTER(C.c_uint8)), num_bits=1, masks=8)  # (never read: the context comes first)
    assert L.egr_object_masks(None, C.byref(q), None) != 0
    assert L.egr_object_masks(None, None, None) != 0


def test_shim_method_exists():
    pkg = importlib.import_module(PKG)
    pkg.load_library()
    methods = {s.name: str(s) for s in torch._C._jit_get_custom_class_schemas()}
    assert methods.get("object_masks") == ("object_masks(__torch__.torch.classes.raytracer.Raytracer _0, Tensor _1, Tensor _2, float _3, float _4, float _5, Tensor _6, int[] _7) -> "
                                           "((Tensor, Tensor, Tensor) _0)"), methods.get("object_masks")
    ed = importlib.import_module(PKG + ".editing")
    assert callable(ed.selection_masks) and callable(ed.pick)


def test_library_version_is_unchanged():
    cabi = importlib.import_module(PKG + ".c_abi")
    assert cabi.lib().egr_version() == b"egr-hip 0.8 (gfx950)"


# ---------------------------------------------------------------- editing.pick

def hand_made(K=32, H=3, W=4):
    """hit / top / names as selection_masks returns them, on the CPU. Pixel (x, y): (0,0) nobody; (1,0) objects 0 and 2, the largest coverage is 0's; (2,0) object 31
    alone (the sign bit of an int32 hit); (3,0) objects 31 and 5, the largest is 5's; (0,2) object 1; (3,2) object 7."""
    names = ["obj%d" % j for j in range(K)]
    hit = torch.zeros((H, W), dtype=torch.int32)
    top = torch.full((H, W), -1, dtype=torch.int32)
    hit[0, 1], top[0, 1] = 0b101, 0
    hit[0, 2], top[0, 2] = -(1 << 31), 31
    hit[0, 3], top[0, 3] = -(1 << 31) + (1 << 5), 5
    hit[2, 0], top[2, 0] = 0b10, 1
    hit[2, 3], top[2, 3] = 1 << 7, 7
    return SimpleNamespace(names=names, masks=None, hit=hit, top=top)


def test_pick_both_rules():
    ed = importlib.import_module(PKG + ".editing")
    r = hand_made()
    assert ed.pick(r, 1, 0) == "obj2" and ed.pick(r, 1, 0, rule="last") == "obj2"  # the reference's rule: the last name whose mask is non-zero
    assert ed.pick(r, 1, 0, rule="top") == "obj0"
    assert ed.pick(r, 0, 2) == "obj1" and ed.pick(r, 0, 2, rule="top") == "obj1"
    with pytest.raises(ValueError):
        ed.pick(r, 0, 0, rule="first")


def test_pick_uncovered_pixel_is_none():
    ed = importlib.import_module(PKG + ".editing")
    r = hand_made()
    assert ed.pick(r, 0, 0) is None and ed.pick(r, 0, 0, rule="top") is None
    assert ed.pick(r, 2, 1) is None and ed.pick(r, 2, 1, rule="top") is None


def test_pick_output_index_31_is_the_sign_bit():
    ed = importlib.import_module(PKG + ".editing")
    r = hand_made()
    assert int(r.hit[0, 2]) < 0
    assert ed.pick(r, 2, 0) == "obj31" and ed.pick(r, 2, 0, rule="top") == "obj31"
    assert ed.pick(r, 3, 0) == "obj31" and ed.pick(r, 3, 0, rule="top") == "obj5"


def test_pick_clamps_to_the_image():
    ed = importlib.import_module(PKG + ".editing")
    r = hand_made()
    assert ed.pick(r, 99, 99) == "obj7" and ed.pick(r, 4, 3, rule="top") == "obj7"  # -> (3, 2)
    assert ed.pick(r, -5, 7) == "obj1" and ed.pick(r, -1, 2.9) == "obj1"  # -> (0, 2)
    assert ed.pick(r, -3, -3) is None  # -> (0, 0)
    assert ed.pick(r, 2.7, -1) == "obj31"  # -> (2, 0)


def test_pick_with_a_subset_of_names():
    ed = importlib.import_module(PKG + ".editing")
    r = hand_made(K=3)
    r.names = ["c", "a", "b"]  # the caller's order: output index, not selection bit
    assert ed.pick(r, 1, 0) == "b" and ed.pick(r, 1, 0, rule="top") == "c" and ed.pick(r, 0, 2) == "a"
