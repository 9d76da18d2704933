"""CPU checks of the dense-init cloud's ABI (include/egr_raytracer.h: egr_voxel_accumulate, egr_voxel_rehash, egr_voxel_extract, egr_voxel_last_error): the header
text, the exported symbols, the ctypes mirror, the torch ops' schemas and every refusal of the argument validation - which runs before any HIP call, so fake
pointers do and no device is needed -, the key packing helper against a lexicographic sort, and the host fp64 camera set-up against the reference's own R_blender
(tests/golden/reference_cameras.npz)."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "egr_raytracer.h")
# fake "device pointers", far apart, 16-byte aligned
KEYS, ACC, STATUS, C2W, ORG, VIEW, DEPTH, COL, TAB, POS, SRCK, SRCA, OUT, WS = (0x10000000 * k for k in range(1, 15))
CAP = 4096


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def error(L):
    return L.egr_voxel_last_error().decode()


def test_header_declares_the_functions_and_states_the_contract():
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    assert ("int egr_voxel_accumulate(int device, int64_t *keys, int64_t *acc, int64_t *status, uint64_t cap, uint32_t num_views, uint32_t height, uint32_t width, "
            "const double *c2w, const double *origin, const double *view_size, const float *depth, const float *colour, const uint8_t *colour_u8, "
            "const float *colour_table, double voxel_scale, double colour_max, double *positions_out, void *hip_stream);") in hdr
    assert ("int egr_voxel_rehash(int device, int64_t *keys, int64_t *acc, int64_t *status, uint64_t cap, const int64_t *src_keys, const int64_t *src_acc, "
            "uint64_t src_cap, void *hip_stream);") in hdr
    assert ("int egr_voxel_extract(int device, const int64_t *keys, const int64_t *acc, int64_t *status, uint64_t cap, uint32_t min_count, double voxel_scale, "
            "uint64_t max_rows, int32_t *coords, float *points, float *colors, int32_t *counts, uint64_t *host_rows_and_largest, void *workspace, "
            "size_t workspace_bytes, void *hip_stream);") in hdr
    assert "size_t egr_voxel_extract_workspace_bytes(int device, uint64_t max_rows);" in hdr
    assert "const char *egr_voxel_last_error(void);" in hdr
    text = open(HEADER).read()
    for word in ("FIXED POINT", "BOUNDED by cap", "round half to even", "an IEEE fp32 division", "DROPPED", "depth 0 are kept", "BEFORE any HIP call", "No float atomics",
                 "SYNCHRONISES the stream once"):
        assert word in text, word
    assert 'return "egr-hip 0.8 (gfx950)"' in open(os.path.join(ROOT, PKG, "csrc", "api.hip")).read()  # additive symbols: the version stays


def test_constants_mirror_the_header(cabi):
    text = open(HEADER).read()
    assert "#define EGR_VOXEL_STATUS_WORDS %d\n" % cabi.EGR_VOXEL_STATUS_WORDS in text
    assert "#define EGR_VOXEL_MIN_CAPACITY %dull" % cabi.EGR_VOXEL_MIN_CAPACITY in text
    assert "#define EGR_VOXEL_MAX_CAPACITY (1ull << 31)" in text and cabi.EGR_VOXEL_MAX_CAPACITY == 1 << 31
    assert "#define EGR_VOXEL_COORD_HALF_RANGE (1 << 20)" in text and cabi.EGR_VOXEL_COORD_HALF_RANGE == 1 << 20
    assert "#define EGR_VOXEL_PAIR_BYTES(max_rows) ((((size_t)(max_rows) * 24) + 15) & ~(size_t)15)" in text
    assert [cabi.voxel_pair_bytes(n) for n in (1, 2, 3, 1000)] == [32, 48, 80, 24000]
    assert len(cabi.VOXEL_STATUS) <= cabi.EGR_VOXEL_STATUS_WORDS


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_voxel_accumulate.argtypes) == 19 and len(L.egr_voxel_rehash.argtypes) == 9 and len(L.egr_voxel_extract.argtypes) == 16
    assert L.egr_voxel_extract_workspace_bytes.restype is C.c_size_t and L.egr_voxel_last_error.restype is C.c_char_p
    assert L.egr_version().decode().startswith("egr-hip 0.8 ")


def test_torch_ops_exist():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.voxel_accumulate.default._schema) == (
        "egr::voxel_accumulate(Tensor keys, Tensor acc, Tensor status, Tensor c2w, Tensor origin, Tensor view_size, Tensor depth, Tensor colour, Tensor? colour_table, "
        "float voxel_scale, float colour_max, Tensor? positions_out=None) -> ()")
    assert str(torch.ops.egr.voxel_rehash.default._schema) == "egr::voxel_rehash(Tensor keys, Tensor acc, Tensor status, Tensor src_keys, Tensor src_acc) -> ()"
    assert str(torch.ops.egr.voxel_extract.default._schema) == (
        "egr::voxel_extract(Tensor keys, Tensor acc, Tensor status, int min_count, float voxel_scale, int max_rows) -> "
        "(Tensor coords, Tensor points, Tensor colors, Tensor counts, int largest_count)")
    k, a, s = torch.full((1024,), -1, dtype=torch.int64), torch.zeros((1024, 4), dtype=torch.int64), torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="keys must be a contiguous int64"):  # a CPU tensor is refused, not dereferenced
        torch.ops.egr.voxel_extract(k, a, s, 2, 400.0, 16)
    init = importlib.import_module(PKG + ".initialization")
    for name in ("VoxelAccumulator", "dense_init_cloud", "gaussians_from_cloud", "camera_setup"):
        assert hasattr(init, name), name


def accumulate(L, keys=KEYS, acc=ACC, status=STATUS, cap=CAP, V=2, H=19, W=37, c2w=C2W, origin=ORG, view=VIEW, depth=DEPTH, colour=COL, u8=None, table=None, scale=400.0,
               cmax=32768.0, pos=None):
    return L.egr_voxel_accumulate(0, keys, acc, status, cap, V, H, W, c2w, origin, view, depth, colour, u8, table, scale, cmax, pos, None)


def test_accumulate_validation(L):
    for kw in (dict(keys=None), dict(acc=None), dict(status=None)):
        assert accumulate(L, **kw) != 0 and "keys, acc and status are required" in error(L)
    assert accumulate(L, keys=KEYS + 4) != 0 and "8-byte aligned" in error(L)
    assert accumulate(L, c2w=C2W + 4) != 0 and "8-byte aligned" in error(L)
    for cap in (0, 512, 3000, 4097, 1 << 32):
        assert accumulate(L, cap=cap) != 0 and "power of two" in error(L), cap
    assert accumulate(L, V=0) != 0 and "num_views" in error(L)
    assert accumulate(L, V=65536) != 0 and "num_views" in error(L)
    assert accumulate(L, H=0) != 0 and "height and width" in error(L)
    assert accumulate(L, W=0) != 0 and "height and width" in error(L)
    assert accumulate(L, H=(1 << 20) + 1) != 0 and "height and width" in error(L)
    assert accumulate(L, W=(1 << 20) + 1) != 0 and "height and width" in error(L)
    assert accumulate(L, V=65535, H=1 << 20, W=1 << 20) != 0 and "2^40" in error(L)  # 2^40 or more pixels in one call
    assert accumulate(L, pos=POS + 4) != 0 and "8-byte aligned" in error(L)  # a misaligned positions_out
    for kw in (dict(c2w=None), dict(origin=None), dict(view=None), dict(depth=None)):
        assert accumulate(L, **kw) != 0 and "c2w, origin, view_size and depth are required" in error(L)
    assert accumulate(L, colour=None) != 0 and "exactly one of colour" in error(L)
    assert accumulate(L, u8=COL + 0x1000000, table=TAB) != 0 and "exactly one of colour" in error(L)
    assert accumulate(L, colour=None, u8=COL) != 0 and "colour_table" in error(L)
    for scale in (0.0, -400.0, float("nan"), float("inf")):
        assert accumulate(L, scale=scale) != 0 and "voxel_scale" in error(L), scale
    for cmax in (0.0, -1.0, float("nan"), 2.0**31):
        assert accumulate(L, cmax=cmax) != 0 and "colour_max" in error(L), cmax
    pixels = 2 * 19 * 37
    assert accumulate(L, acc=KEYS + CAP * 8 - 8) != 0 and "overlaps" in error(L)  # acc starts in the last key
    assert accumulate(L, status=ACC + CAP * 32 - 8) != 0 and "overlaps" in error(L)
    assert accumulate(L, depth=KEYS + 64) != 0 and "overlaps" in error(L)  # an input inside the table
    assert accumulate(L, pos=COL + pixels * 12 - 8) != 0 and "overlaps" in error(L)  # positions_out starts in the last colour
    assert accumulate(L, pos=STATUS - pixels * 24 + 8) != 0 and "overlaps" in error(L)  # ... or ends in status
    assert accumulate(L, colour=None, u8=COL, table=ACC + 1024) != 0 and "overlaps" in error(L)


def rehash(L, keys=KEYS, acc=ACC, status=STATUS, cap=2 * CAP, src_keys=SRCK, src_acc=SRCA, src_cap=CAP):
    return L.egr_voxel_rehash(0, keys, acc, status, cap, src_keys, src_acc, src_cap, None)


def test_rehash_validation(L):
    for kw in (dict(keys=None), dict(acc=None), dict(status=None), dict(src_keys=None), dict(src_acc=None)):
        assert rehash(L, **kw) != 0 and "are required" in error(L)
    assert rehash(L, src_acc=SRCA + 2) != 0 and "8-byte aligned" in error(L)
    assert rehash(L, cap=1000) != 0 and "power of two" in error(L)
    assert rehash(L, src_cap=0) != 0 and "power of two" in error(L)
    assert rehash(L, src_keys=KEYS) != 0 and "out of place" in error(L)  # in place
    assert rehash(L, src_acc=ACC + 2 * CAP * 32 - 32) != 0 and "out of place" in error(L)
    assert rehash(L, status=SRCK + 8) != 0 and "out of place" in error(L)


def extract(L, keys=KEYS, acc=ACC, status=STATUS, cap=CAP, min_count=2, scale=400.0, max_rows=100, coords=OUT, points=OUT + 0x100000, colors=OUT + 0x200000, counts=OUT + 0x300000,
            host=True, ws=WS, ws_bytes=1 << 20):
    h = (C.c_uint64 * 2)()
    return L.egr_voxel_extract(0, keys, acc, status, cap, min_count, scale, max_rows, coords, points, colors, counts, h if host else None, ws, ws_bytes, None)


def test_extract_validation(L, cabi):
    for kw in (dict(keys=None), dict(acc=None), dict(status=None)):
        assert extract(L, **kw) != 0 and "keys, acc and status are required" in error(L)
    assert extract(L, status=STATUS + 4) != 0 and "8-byte aligned" in error(L)
    assert extract(L, cap=CAP + 1) != 0 and "power of two" in error(L)
    assert extract(L, scale=0.0) != 0 and "voxel_scale" in error(L)
    assert extract(L, max_rows=0) != 0 and "max_rows" in error(L)
    assert extract(L, max_rows=CAP + 1) != 0 and "max_rows" in error(L)
    for kw in (dict(coords=None), dict(points=None), dict(colors=None), dict(counts=None), dict(host=False)):
        assert extract(L, **kw) != 0 and "required outputs" in error(L)
    assert extract(L, ws=None) != 0 and "workspace" in error(L)
    assert extract(L, ws=WS + 8) != 0 and "workspace" in error(L)  # misaligned
    assert extract(L, ws_bytes=cabi.voxel_pair_bytes(100)) != 0 and "smaller than" in error(L)  # room for the pairs but not for the sort
    assert extract(L, points=OUT + 100 * 12 - 4) != 0 and "overlaps" in error(L)  # points starts in the last coordinate
    assert extract(L, counts=KEYS + 8) != 0 and "overlaps" in error(L)  # an output inside the table
    assert extract(L, ws=ACC + 1024) != 0 and "overlaps" in error(L)
    assert extract(L, ws=OUT + 0x300000 - 0x100000 + 16, ws_bytes=1 << 20) != 0 and "overlaps" in error(L)  # the workspace ends in counts
    assert L.egr_voxel_extract_workspace_bytes(0, 0) == 0 and "max_rows" in error(L)


def test_key_packing_orders_like_a_lexicographic_sort(cabi):
    rng = np.random.default_rng(7)
    H = cabi.EGR_VOXEL_COORD_HALF_RANGE
    edges = np.array([[a, b, c] for a in (-H, -1, 0, H - 1) for b in (-H, -1, 0, H - 1) for c in (-H, -1, 0, 1, H - 1)])
    coords = np.concatenate([rng.integers(-H, H, (4000, 3)), rng.integers(-3, 3, (4000, 3)), edges]).astype(np.int64)
    keys = cabi.voxel_pack_keys(coords)
    assert keys.dtype == np.int64 and keys.min() >= 0
    assert np.array_equal(cabi.voxel_unpack_keys(keys), coords.astype(np.int32))
    lexicographic = np.lexsort((coords[:, 2], coords[:, 1], coords[:, 0]))  # x first, then y, then z, all signed
    by_key = np.argsort(keys, kind="stable")
    assert np.array_equal(coords[by_key], coords[lexicographic])
    unique_rows = torch.unique(torch.from_numpy(coords), dim=0).numpy()  # the order the output has to have
    assert np.array_equal(cabi.voxel_unpack_keys(np.unique(keys)), unique_rows.astype(np.int32))
    for bad in ([H, 0, 0], [0, -H - 1, 0]):
        with pytest.raises(ValueError):
            cabi.voxel_pack_keys(np.array([bad]))


def test_host_camera_setup_reproduces_the_reference_vectors():
    init = importlib.import_module(PKG + ".initialization")
    z = np.load(os.path.join(ROOT, "tests", "golden", "reference_cameras.npz"))
    for i in range(int(z["num_cases"])):
        R, T, fovy = z[f"c{i}_R"], z[f"c{i}_T"], float(z[f"c{i}_FoVy"])
        c2w, origin, view_size = init.camera_setup(R, T, fovy)
        assert c2w.dtype == np.float64 and np.array_equal(c2w, z[f"c{i}_R_blender"])  # bit for bit: two negations
        assert np.array_equal(origin, -R @ T) and np.abs(origin - z[f"c{i}_camera_center"]).max() < 1e-5
        assert view_size == math.tan(fovy * 0.5)
        c2, o2, v2 = init.camera_setup(torch.from_numpy(R), torch.from_numpy(T), torch.tensor(fovy, dtype=torch.float64))  # torch inputs, the same numbers
        assert np.array_equal(c2, c2w) and np.array_equal(o2, origin) and v2 == view_size
