"""CPU checks of the view-store ABI (include/egr_raytracer.h: egr_viewset_ingest, egr_viewset_gather, egr_viewset_last_error and their three structs): the
header text against the ctypes mirror, the exported symbols, the two torch ops, and every refusal - validation runs before any HIP call, so none of this needs a
device."""
import ctypes as C
import importlib
import os
import re

import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
# non-NULL "device pointers", far apart: a call that fails validation never touches them
DATA, TABLE, PLANES, RANGE, OUT, CAMS = 0x10000000, 0x20000000, 0x30000000, 0x50000000, 0x60000000, 0x70000000


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def error(L):
    return L.egr_viewset_last_error().decode()


def struct_fields(hdr, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return [re.sub(r"\[.*\]", "", d.strip().split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]


def test_header_declares_the_functions_and_the_structs(cabi):
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int egr_viewset_ingest(int device, const egr_viewset_source *sources, uint32_t num_views, uint32_t src_height, uint32_t src_width, uint32_t height, "
            "uint32_t width, uint32_t first_slot, uint32_t num_slots, float *depth_range, void *hip_stream);") in hdr
    assert ("int egr_viewset_gather(int device, const egr_viewset_store *store, const uint32_t *indices, uint32_t num_views, const egr_viewset_batch *out, "
            "void *hip_stream);") in hdr
    assert "const char *egr_viewset_last_error(void);" in hdr
    for name, value in (("EGR_VIEWSET_KINDS", "%d" % cabi.EGR_VIEWSET_KINDS), ("EGR_VIEWSET_DEPTH", "%d" % cabi.EGR_VIEWSET_DEPTH), ("EGR_VIEWSET_U8", "%du" % cabi.EGR_VIEWSET_U8),
                        ("EGR_VIEWSET_F32", "%du" % cabi.EGR_VIEWSET_F32), ("EGR_VIEWSET_MAX_GATHER", "%d" % cabi.EGR_VIEWSET_MAX_GATHER)):
        assert "#define %s %s " % (name, value) in hdr, name
    assert (cabi.EGR_VIEWSET_KINDS, cabi.EGR_VIEWSET_DEPTH, cabi.EGR_VIEWSET_U8, cabi.EGR_VIEWSET_F32, cabi.EGR_VIEWSET_MAX_GATHER) == (7, 3, 0, 1, 64)
    assert cabi.VIEWSET_KINDS == ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0") and cabi.VIEWSET_KINDS[cabi.EGR_VIEWSET_DEPTH] == "depth"
    assert "0 render, 1 diffuse, 2 specular, 3 depth, 4 normal, 5 roughness, 6 f0" in hdr
    assert struct_fields(hdr, "egr_viewset_source") == [f[0] for f in cabi.egr_viewset_source._fields_] == ["data", "table", "planes", "channels", "dtype"]
    assert [f[1] for f in cabi.egr_viewset_source._fields_] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32] and C.sizeof(cabi.egr_viewset_source) == 32
    assert struct_fields(hdr, "egr_viewset_store") == [f[0] for f in cabi.egr_viewset_store._fields_] == ["planes", "R", "centers", "fovy", "num_slots", "num_filled", "height", "width"]
    assert C.sizeof(cabi.egr_viewset_store) == 7 * 8 + 3 * 8 + 4 * 4
    assert struct_fields(hdr, "egr_viewset_batch") == [f[0] for f in cabi.egr_viewset_batch._fields_] == ["targets", "R", "centers", "fovy"]
    assert C.sizeof(cabi.egr_viewset_batch) == 7 * 8 + 3 * 8
    # the contract is written down
    for word in ("BEFORE any HIP call", "CHANNEL 0", "row-major order starting from +0", "ONE correctly rounded IEEE division", "floor-divided", "uint8 depth is refused",
                 "floor(i * src / dst) up to but excluding ceil((i + 1) * src / dst)", "((double)src_width / (double)src_height)",
                 "(+inf, -inf)", "do not depend on arrival order", "(NaN, NaN)", "exactly float(half)", "HOST array", "no upload, no synchronisation", "Repeats and any"):
        assert word in hdr, word


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_viewset_ingest.argtypes) == 11 and len(L.egr_viewset_gather.argtypes) == 6
    assert L.egr_viewset_last_error.restype is C.c_char_p
    assert L.egr_version() == b"egr-hip 0.8 (gfx950)"  # additive symbols: the library still answers as before


def test_torch_ops_exist_with_their_schemas():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.viewset_ingest.default._schema) == ("egr::viewset_ingest(Tensor?[] sources, Tensor?[] tables, Tensor[] planes, Tensor depth_range, int first_slot) -> ()")
    assert str(torch.ops.egr.viewset_gather.default._schema) == ("egr::viewset_gather(Tensor[] planes, Tensor R, Tensor centers, Tensor fovy, int num_filled, int[] indices, "
                                                                 "Tensor?[] out, Tensor out_R, Tensor out_centers, Tensor out_fovy) -> ()")
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path
        torch.ops.egr.viewset_ingest([None] * 7, [None] * 7, [torch.zeros((1, c, 2, 2), dtype=torch.float16) for c in (3, 3, 3, 1, 3, 1, 3)], torch.zeros((1, 2)), 0)


F32, U8 = 1, 0


def ingest(L, cabi, kinds=None, V=2, Hs=4, Ws=6, H=4, W=6, first=0, slots=4, rng=RANGE, table=True):
    """kinds: {kind index: (data, table, planes, channels, dtype)}; default: an fp32 3-channel diffuse and a 1-channel depth."""
    if kinds is None:
        kinds = {1: (DATA, None, PLANES, 3, F32), 3: (DATA + 0x1000000, None, PLANES + 0x1000000, 1, F32)}
    t = (cabi.egr_viewset_source * 7)()
    for k, e in kinds.items():
        t[k] = cabi.egr_viewset_source(data=e[0], table=e[1], planes=e[2], channels=e[3], dtype=e[4])
    return L.egr_viewset_ingest(0, t if table else None, V, Hs, Ws, H, W, first, slots, rng, None)


def test_ingest_refusals(L, cabi):
    named = lambda what: "egr_viewset_ingest" in error(L) and what in error(L)
    one = lambda k, *e: {k: e}
    assert ingest(L, cabi, one(3, DATA, TABLE, PLANES, 1, U8)) != 0 and named("uint8 depth")
    assert ingest(L, cabi, one(1, DATA, None, PLANES, 3, U8)) != 0 and named("needs its table")  # a table missing
    assert ingest(L, cabi, one(1, DATA, TABLE, PLANES, 3, F32)) != 0 and named("table was given for an fp32")  # ... or given for fp32
    assert ingest(L, cabi, Ws=7) != 0 and named("size mismatch")  # the store's height, another width
    assert ingest(L, cabi, Hs=45, Ws=80, H=32, W=57) != 0 and named("size mismatch") and "56" in error(L)  # int(32 * (80 / 45)) = 56
    assert ingest(L, cabi, Hs=8, Ws=12, H=4, W=5) != 0 and named("size mismatch")
    assert ingest(L, cabi, V=0) != 0 and named("num_views")
    assert ingest(L, cabi, V=65536, slots=70000) != 0 and named("num_views")
    for ch in (0, 2, 4):
        assert ingest(L, cabi, one(5, DATA, None, PLANES, ch, F32)) != 0 and named("channels must be 1 or 3"), ch
    assert ingest(L, cabi, one(1, DATA, None, PLANES, 1, F32)) != 0 and named("colour kind needs 3 channels")
    assert ingest(L, cabi, one(1, DATA, None, PLANES, 3, 2)) != 0 and named("unknown dtype")
    assert ingest(L, cabi, one(1, DATA, None, None, 3, F32)) != 0 and named("without planes")
    assert ingest(L, cabi, one(1, DATA + 2, None, PLANES, 3, F32)) != 0 and named("4-byte aligned")
    assert ingest(L, cabi, one(1, DATA, None, PLANES + 1, 3, F32)) != 0 and named("2-byte aligned")
    assert ingest(L, cabi, {}) != 0 and named("every kind is absent")
    assert ingest(L, cabi, table=False) != 0 and named("sources")
    assert ingest(L, cabi, rng=None) != 0 and named("depth_range")
    assert ingest(L, cabi, first=3) != 0 and named("exceeds num_slots")  # slots 3, 4 of 4
    assert ingest(L, cabi, first=(1 << 32) - 1) != 0 and named("exceeds num_slots")  # (the sum does not wrap)
    for bad in (dict(H=0, Hs=0), dict(W=0, Ws=0), dict(Hs=65536, H=65536), dict(Ws=65536, W=65536)):
        assert ingest(L, cabi, **bad) != 0 and named("1..65535"), bad
    assert ingest(L, cabi, one(1, DATA, None, PLANES, 3, F32), V=1, Hs=65535, Ws=65535, H=1, W=1) != 0 and named("2^24")
    # an output overlapping an input, or another output: 2 views of 4 x 6 x 3 fp32 are 576 bytes of data and 288 bytes of planes
    assert ingest(L, cabi, one(1, DATA, None, DATA, 3, F32)) != 0 and named("overlaps an input")  # planes == data
    assert ingest(L, cabi, one(1, DATA, None, DATA + 576 - 2, 3, F32)) != 0 and named("overlaps an input")  # planes start in the last bytes of data
    assert ingest(L, cabi, one(1, DATA, None, DATA - 288 + 2, 3, F32)) != 0 and named("overlaps an input")  # ... end in its first
    assert ingest(L, cabi, one(4, DATA, TABLE, TABLE + 510, 3, U8)) != 0 and named("overlaps an input")  # planes in the table's last half
    assert ingest(L, cabi, one(1, DATA, None, PLANES, 3, F32), rng=DATA + 8) != 0 and named("overlaps an input")  # the range rows in the data
    assert ingest(L, cabi, one(1, DATA, None, PLANES, 3, F32), rng=PLANES + 286) != 0 and named("two outputs")  # the range rows in the written planes
    assert ingest(L, cabi, {1: (DATA, None, PLANES, 3, F32), 2: (DATA + 0x1000, None, PLANES + 2, 3, F32)}) != 0 and named("two outputs")
    # only the WRITTEN slots count: the planes of slot 0 may hold the data that goes into slots 2, 3
    assert ingest(L, cabi, one(1, PLANES, None, PLANES, 3, F32), first=2) != 0 and named("overlaps")  # 576 bytes from PLANES reach slots 2.. (144 bytes each)


def gather(L, cabi, idx=(0, 1), filled=3, slots=4, H=4, W=6, planes=None, targets=None, cams=(CAMS, CAMS + 0x1000, CAMS + 0x2000), outs=(OUT + 0x100000, OUT + 0x101000, OUT + 0x102000),
           store=True, out=True, indices=True):
    s = cabi.egr_viewset_store(R=cams[0], centers=cams[1], fovy=cams[2], num_slots=slots, num_filled=filled, height=H, width=W)
    b = cabi.egr_viewset_batch(R=outs[0], centers=outs[1], fovy=outs[2])
    for k, p in ({1: PLANES} if planes is None else planes).items():
        s.planes[k] = p
    for k, p in ({1: OUT} if targets is None else targets).items():
        b.targets[k] = p
    arr = (C.c_uint32 * max(len(idx), 1))(*idx)
    return L.egr_viewset_gather(0, C.byref(s) if store else None, arr if indices else None, len(idx), C.byref(b) if out else None, None)


def test_gather_refusals(L, cabi):
    named = lambda what: "egr_viewset_gather" in error(L) and what in error(L)
    assert gather(L, cabi, idx=(0, 3)) != 0 and named("out of range") and "index 3" in error(L)  # 3 slots are filled
    assert gather(L, cabi, idx=(2, 0, 0xFFFFFFFF)) != 0 and named("out of range")
    assert gather(L, cabi, idx=(0,), filled=0) != 0 and named("out of range")  # an empty store
    assert gather(L, cabi, idx=()) != 0 and named("num_views is 0")
    assert gather(L, cabi, filled=5) != 0 and named("num_filled exceeds")
    assert gather(L, cabi, store=False) != 0 and named("required") and gather(L, cabi, out=False) != 0 and named("required") and gather(L, cabi, indices=False) != 0 and named("required")
    assert gather(L, cabi, H=0) != 0 and named("1..65535") and gather(L, cabi, W=65536) != 0 and named("1..65535")
    assert gather(L, cabi, targets={2: OUT}) != 0 and named("specular") and "no planes" in error(L)  # wanted, but the store has none
    assert gather(L, cabi, cams=(None, CAMS, CAMS + 0x1000)) != 0 and named("R: wanted")
    assert gather(L, cabi, targets={}, outs=(None, None, None)) != 0 and named("nothing is wanted")
    assert gather(L, cabi, targets={1: OUT + 2}) != 0 and named("misaligned")
    # an output overlapping the store: 4 slots of 3 x 4 x 6 halfs are 576 bytes, 2 gathered views are 576 bytes of fp32
    assert gather(L, cabi, targets={1: PLANES}) != 0 and named("overlaps the store")
    assert gather(L, cabi, targets={1: PLANES + 572}) != 0 and named("overlaps the store")
    assert gather(L, cabi, targets={1: PLANES - 572}) != 0 and named("overlaps the store")
    assert gather(L, cabi, outs=(CAMS + 0x1000 + 44, OUT + 0x101000, OUT + 0x102000)) != 0 and named("overlaps the store")  # out R over the last centre row
    assert gather(L, cabi, planes={1: PLANES, 4: PLANES + 0x100000}, targets={1: OUT, 4: OUT + 572}) != 0 and named("two outputs")
    assert gather(L, cabi, outs=(OUT + 0x100000, OUT + 0x100000 + 68, OUT + 0x102000)) != 0 and named("two outputs")  # centers in the last row of R
