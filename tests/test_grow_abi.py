"""CPU checks of the cloud-growing ABI (include/egr_raytracer.h: egr_grow_sample, egr_grow_append, egr_grow_last_error, egr_grow_array): the generator's
restatement against the published Philox4x32-10 known-answer vectors, the header text, the ctypes mirror, the exported symbols, the two torch ops, and the
argument validation - which runs before any HIP call, so all of this needs no device."""
import ctypes as C
import importlib
import math
import os
import re

import numpy as np
import pytest

import grow_restatement as gr

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
A, B, T = 0x100000, 0x90000000, 0x50000000  # non-NULL "device pointers", far apart: a call that fails validation never touches them


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def error(L):
    return L.egr_grow_last_error().decode()


# Random123's kat_vectors for philox4x32 with 10 rounds: counter, key, result
KAT = (((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)))


def test_restated_philox_reproduces_the_known_answer_vectors():
    for counter, key, want in KAT:
        got = gr.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
        assert tuple(int(x) for x in got) == want, (counter, key, [hex(int(x)) for x in got])
    # all three at once (the restatement is vectorised), and the counter / key layout of a candidate: (i_lo, i_hi, 0, 0) under (seed_lo, seed_hi)
    got = gr.philox4x32_10(np.array([k[0] for k in KAT], np.uint64), np.array([k[1] for k in KAT], np.uint64))
    assert got.tolist() == [list(k[2]) for k in KAT]
    i, seed = (5 << 32) | 7, (9 << 32) | 11
    assert gr.words(i, 1, seed).tolist() == gr.philox4x32_10(np.array([[7, 5, 0, 0]], np.uint64), np.array([11, 9], np.uint64)).tolist()
    assert gr.words(0, 1, 0)[0].tolist() == list(KAT[0][2])


def test_restated_uniforms_and_normals():
    w = gr.words(0, 4097, 750)
    u = ((w >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert u.min() > 0.0 and u.max() < 1.0 and np.array_equal(u.astype(np.float32).astype(np.float64), u)  # 24 significant bits: exact in fp32
    z = gr.normals(0, 4097, 750)
    assert abs(float(z.mean())) < 0.05 and abs(float(z.std()) - 1.0) < 0.05  # 12291 standard normals
    assert float(np.abs(z).max()) < math.sqrt(-2.0 * math.log(2.0 ** -24)) + 1e-6  # the grid's largest radius (5.77)
    c = gr.candidates(0, 4097, 750, 2.5)
    assert c.dtype == np.float32 and int((np.abs(z) > 3.0).sum()) == 27 and int((np.abs(c) == 7.5).sum()) == 27 and float(np.abs(c).max()) == 7.5


def test_header_declares_the_functions_and_the_struct(cabi):
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    assert "int egr_grow_sample(int device, uint64_t first, uint32_t n, uint64_t seed, float radius, float clamp, float *out_points, void *hip_stream);" in hdr
    assert "int egr_grow_append(int device, const egr_grow_array *arrays, int num_arrays, uint32_t n, uint32_t m, void *hip_stream);" in hdr
    assert "const char *egr_grow_last_error(void);" in hdr
    assert "#define EGR_GROW_TAIL_ROWS %du" % cabi.EGR_GROW_TAIL_ROWS in hdr and "#define EGR_GROW_TAIL_FILL %du" % cabi.EGR_GROW_TAIL_FILL in hdr
    assert (cabi.EGR_GROW_TAIL_ROWS, cabi.EGR_GROW_TAIL_FILL) == (0, 1)
    body = re.search(r"typedef struct egr_grow_array \{(.*?)\} egr_grow_array;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    fields = [d.strip().split()[-1].lstrip("*") for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in cabi.egr_grow_array._fields_] == ["src", "dst", "tail", "width", "tail_kind", "fill_bits"]
    assert [f[1] for f in cabi.egr_grow_array._fields_] == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    assert C.sizeof(cabi.egr_grow_array) == 40
    # the contract is written down: what a candidate depends on, the generator's constants, the uniform grid, no overlap, moved as bits
    for word in ("depends on (seed, i", "Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(i & 0xffffffff, i >> 32, 0, 0)", "((x_k >> 9) + 0.5) * 2^-23",
                 "Box-Muller in fp64", "OUT OF PLACE", "moved as bits", "BEFORE any HIP call", "n + m == 0 returns 0 and launches nothing"):
        assert word in hdr, word


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_grow_sample.argtypes) == 8 and len(L.egr_grow_append.argtypes) == 6
    assert L.egr_grow_sample.argtypes[1] is C.c_uint64 and L.egr_grow_sample.argtypes[3] is C.c_uint64
    assert L.egr_grow_last_error.restype is C.c_char_p
    assert L.egr_version() == b"egr-hip 0.8 (gfx950)"  # additive symbols: the library still answers as before


def test_torch_ops_exist_with_their_schemas():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.grow_sample.default._schema) == "egr::grow_sample(int first, int n, int seed, float radius, float clamp, Device device) -> Tensor"
    assert str(torch.ops.egr.grow_append.default._schema) == "egr::grow_append(Tensor[] src, Tensor?[] tail, int[] fill_bits, int m) -> Tensor[]"


def sample(L, first=0, n=16, seed=1, radius=1.0, clamp=3.0, out=A):
    return L.egr_grow_sample(0, first, n, seed, radius, clamp, out, None)


def test_sample_validation(L):
    assert sample(L, out=None) != 0 and "egr_grow_sample" in error(L) and "out_points" in error(L)
    assert sample(L, n=(1 << 26) + 1) != 0 and "egr_grow_sample" in error(L) and "2^26" in error(L)
    assert sample(L, first=(1 << 64) - 1, n=2) != 0 and "egr_grow_sample" in error(L) and "overflows" in error(L)
    assert sample(L, first=(1 << 64) - 16, n=17) != 0 and "overflows" in error(L)
    for bad in (math.nan, math.inf, -math.inf, -1.0):
        assert sample(L, radius=bad) != 0 and "egr_grow_sample" in error(L) and "radius" in error(L), bad
        assert sample(L, clamp=bad) != 0 and "egr_grow_sample" in error(L) and "clamp" in error(L), bad
    assert sample(L, n=0) == 0  # no rows: success, nothing launched (no device here to launch on)
    assert sample(L, n=0, first=(1 << 64) - 1) == 0
    assert sample(L, n=0, out=None) != 0  # (the output stays required)


def append(L, cabi, entries, n=16, m=8):
    """entries: (src, dst, tail, width[, kind[, fill_bits]])"""
    rows = [cabi.egr_grow_array(src=e[0], dst=e[1], tail=e[2], width=e[3], tail_kind=e[4] if len(e) > 4 else (cabi.EGR_GROW_TAIL_ROWS if e[2] else cabi.EGR_GROW_TAIL_FILL),
                                fill_bits=e[5] if len(e) > 5 else 0) for e in entries]
    table = (cabi.egr_grow_array * max(len(rows), 1))(*rows)
    return L.egr_grow_append(0, table, len(rows), n, m, None)


def test_append_validation(L, cabi):
    named = lambda what: "egr_grow_append" in error(L) and what in error(L)
    assert append(L, cabi, [(A, A, T, 3)]) != 0 and named("out of place")  # src == dst
    assert append(L, cabi, [(A, A + 16 * 3 * 4 - 4, T, 3)]) != 0 and named("out of place")  # dst starts in the last word of src
    assert append(L, cabi, [(A, B, T, 3), (A + 0x1000, A, T + 0x1000, 1)]) != 0 and named("out of place")  # dst of one entry over the src of another
    assert append(L, cabi, [(A, T, T, 3)]) != 0 and named("overlaps a tail")  # dst == its own tail
    assert append(L, cabi, [(A, T - 24 * 3 * 4 + 4, T, 3)]) != 0 and named("overlaps a tail")  # dst ends in the first word of the tail
    assert append(L, cabi, [(A, B, T, 3), (A + 0x1000, T + 4, T + 0x1000, 1)]) != 0 and named("overlaps a tail")  # ... of another entry's tail
    assert append(L, cabi, [(A, B, T, 3), (A + 0x1000, B + 4, T + 0x1000, 1)]) != 0 and named("two dst")
    assert append(L, cabi, [(A, B, T, 3), (A + 0x1000, B + 24 * 3 * 4 - 4, None, 1)]) != 0 and named("two dst")  # the second starts in the last word of the first
    assert append(L, cabi, [(A + 0x1000 * k, B + 0x1000 * k, None, 1) for k in range(33)]) != 0 and named("EGR_MAX_PRUNE_ARRAYS")
    assert append(L, cabi, []) != 0 and named("EGR_MAX_PRUNE_ARRAYS")
    assert L.egr_grow_append(0, None, 1, 16, 8, None) != 0 and named("table")
    assert append(L, cabi, [(A, B, T, 0)]) != 0 and named("width 0")
    assert append(L, cabi, [(A, B, T, 3, 2)]) != 0 and named("tail_kind")
    assert append(L, cabi, [(A, None, T, 3)]) != 0 and named("dst")
    assert append(L, cabi, [(None, B, T, 3)]) != 0 and named("src")
    assert append(L, cabi, [(A, B, None, 3, cabi.EGR_GROW_TAIL_ROWS)]) != 0 and named("tail")
    assert append(L, cabi, [(A, B, T, 3)], n=1 << 26, m=1) != 0 and named("2^26")
    assert append(L, cabi, [(A, B, T, 3)], n=1, m=1 << 26) != 0 and named("2^26")
    assert append(L, cabi, [(A, B, T, 3)], n=(1 << 32) - 1, m=(1 << 32) - 1) != 0 and named("2^26")  # (the sum does not wrap)
    # n + m == 0: success, nothing launched (no device here to launch on) - with or without the pointers an empty array has
    assert append(L, cabi, [(A, B, T, 3)], n=0, m=0) == 0
    assert append(L, cabi, [(None, B, None, 3, cabi.EGR_GROW_TAIL_ROWS)], n=0, m=0) == 0
    assert append(L, cabi, [(A, A, A, 3)], n=0, m=0) == 0  # (empty ranges touch nothing)
    assert append(L, cabi, [(A, B, T, 0)], n=0, m=0) != 0  # (the table is still checked)
