"""CPU checks of the fused-prune ABI (include/egr_raytracer.h: egr_prune_select, egr_prune_gather, egr_prune_last_error, egr_prune_array): the header text, the
ctypes mirror, the exported symbols, the two torch ops, and the argument validation - which runs before any HIP call, so all of this needs no device."""
import ctypes as C
import importlib
import os
import re

import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
FAKE = 0x10000  # a non-NULL "device pointer": a call that fails validation never touches it (8-byte aligned, and far from FAKE2)
FAKE2 = 0x90000000


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def error(L):
    return L.egr_prune_last_error().decode()


def test_header_declares_the_functions_and_the_struct(cabi):
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    assert ("int egr_prune_select(int device, uint32_t n, const float *total_weight, float divisor, float min_weight, const float *points, const float *cam_centers, "
            "const float *cam_znear, uint32_t num_cams, const uint8_t *remove_mask, uint32_t *src_index, uint32_t *count, void *workspace, void *hip_stream);") in hdr
    assert "int egr_prune_gather(int device, const egr_prune_array *arrays, int num_arrays, uint32_t n, const uint32_t *src_index, uint32_t count, void *hip_stream);" in hdr
    assert "const char *egr_prune_last_error(void);" in hdr
    assert "#define EGR_MAX_PRUNE_ARRAYS 32" in hdr and cabi.EGR_MAX_PRUNE_ARRAYS == 32
    assert "#define EGR_PRUNE_ROWS_PER_WG %du" % cabi.EGR_PRUNE_ROWS_PER_WG in hdr
    body = re.search(r"typedef struct egr_prune_array \{(.*?)\} egr_prune_array;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in cabi.egr_prune_array._fields_] == ["src", "dst", "width"]
    assert [f[1] for f in cabi.egr_prune_array._fields_] == [C.c_void_p, C.c_void_p, C.c_uint32]
    # the contract is written down: strictness, ordering, the one synchronisation, no overlap
    for word in ("strict", "ASCENDING", "ONE synchronisation", "OUT OF PLACE"):
        assert word in hdr, word


def test_workspace_size_mirror(cabi):
    # 16 ballots of 8 bytes + one 4-byte count per EGR_PRUNE_ROWS_PER_WG rows (the header's macro)
    R = cabi.EGR_PRUNE_ROWS_PER_WG
    assert [cabi.prune_workspace_bytes(n) for n in (0, 1, R, R + 1, 3 * R + 17)] == [0, 132, 132, 264, 528]
    assert re.search(r"#define EGR_PRUNE_WORKSPACE_BYTES\(n\) \(\(\(\(size_t\)\(n\) \+ EGR_PRUNE_ROWS_PER_WG - 1\) / EGR_PRUNE_ROWS_PER_WG\) \* \(16 \* 8 \+ 4\)\)", open(HEADER).read())


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_prune_select.argtypes) == 14 and len(L.egr_prune_gather.argtypes) == 7
    assert L.egr_prune_last_error.restype is C.c_char_p
    assert L.egr_version().decode()  # additive symbols: the library still answers as before


def test_torch_ops_exist_with_their_schemas():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.prune_select.default._schema) == (
        "egr::prune_select(Tensor? total_weight, float divisor, float min_weight, Tensor? points, Tensor? cam_centers, Tensor? cam_znear, Tensor? remove_mask) -> "
        "(Tensor src_index, Tensor count)")
    assert str(torch.ops.egr.prune_gather.default._schema) == "egr::prune_gather(Tensor[] src, Tensor src_index, int count) -> Tensor[]"


def select(L, n, src_index=FAKE, count=FAKE + 64, workspace=FAKE2, points=None, cams=0):
    return L.egr_prune_select(0, n, None, 1.0, 0.0, points, None, None, cams, FAKE + 128, src_index, count, workspace, None)


def test_select_validation(L):
    for kw in (dict(src_index=None), dict(count=None)):
        assert select(L, 16, **kw) != 0
        assert "src_index and count" in error(L)
    assert select(L, (1 << 26) + 1) != 0 and "2^26" in error(L)
    assert select(L, 16, workspace=None) != 0 and "workspace" in error(L)
    assert select(L, 16, workspace=FAKE2 + 4) != 0 and "workspace" in error(L)  # misaligned
    assert select(L, 16, points=FAKE + 256, cams=3) != 0 and "cam_centers" in error(L)  # cameras announced, arrays missing
    assert select(L, 0) == 0  # no rows: success, nothing launched (no device here to launch on)
    assert select(L, 0, workspace=None) == 0


def gather(L, cabi, entries, n=16, count=8, src_index=FAKE2):
    table = (cabi.egr_prune_array * max(len(entries), 1))(*[cabi.egr_prune_array(src=s, dst=d, width=w) for s, d, w in entries])
    return L.egr_prune_gather(0, table, len(entries), n, src_index, count, None)


def test_gather_validation(L, cabi):
    A, B = 0x100000, 0x200000
    assert gather(L, cabi, [(A, B, 0)]) != 0 and "width 0" in error(L)
    assert gather(L, cabi, [(A + 0x1000 * k, B + 0x1000 * k, 1) for k in range(33)]) != 0 and "EGR_MAX_PRUNE_ARRAYS" in error(L)
    assert gather(L, cabi, []) != 0 and error(L)
    assert L.egr_prune_gather(0, None, 1, 16, FAKE2, 8, None) != 0 and error(L)
    assert gather(L, cabi, [(A, A, 3)]) != 0 and "out of place" in error(L)  # src == dst
    assert gather(L, cabi, [(A, A + 16 * 3 * 4 - 4, 3)]) != 0 and "out of place" in error(L)  # dst starts in the last word of src
    assert gather(L, cabi, [(A, B, 3), (A + 0x1000, A, 1)]) != 0 and "out of place" in error(L)  # dst of one entry over the src of another
    assert gather(L, cabi, [(A, B, 3), (A + 0x1000, B + 4, 1)]) != 0 and "two dst" in error(L)
    assert gather(L, cabi, [(None, B, 3)]) != 0 and gather(L, cabi, [(A, None, 3)]) != 0
    assert gather(L, cabi, [(A, B, 3)], src_index=None) != 0 and "src_index" in error(L)
    assert gather(L, cabi, [(A, B, 3)], n=8, count=9) != 0 and "count <= n" in error(L)
    assert gather(L, cabi, [(A, B, 3)], n=(1 << 26) + 1) != 0
    assert gather(L, cabi, [(A, B, 3)], count=0) == 0  # nothing to move: success, nothing launched
    assert gather(L, cabi, [(A, A + 16 * 3 * 4, 3)], count=0) == 0  # adjacent ranges do not overlap
