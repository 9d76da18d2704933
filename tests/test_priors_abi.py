"""CPU checks of the prior-view ABI (include/egr_raytracer.h: egr_prior_pairs, egr_prior_fit, egr_prior_finish, egr_prior_last_error and their three argument
structs): the header text against the ctypes mirror, the exported symbols, the three torch ops, and every refusal - validation runs before any HIP call, so none
of this needs a device."""
import ctypes as C
import importlib
import os
import re

import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
# non-NULL "device pointers", far apart: a call that fails validation never touches them
CAMS, POINTS, OFFS, DEPTH, SPARSE, PX, PY, COUNT, DROPPED = (0x10000000 * k for k in range(1, 10))
VIEWS, SAMPLES, HERR, HMODEL, AB, BEST_IT, BEST_ERR, MASK = (0xA0000000 + 0x1000000 * k for k in range(8))
NORMAL, METAL, DIST, NOUT, F0 = (0xB0000000 + 0x1000000 * k for k in range(5))


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def error(L):
    return L.egr_prior_last_error().decode()


def struct_fields(hdr, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body)
    return [re.sub(r"\[.*\]", "", d.strip().split()[-1].lstrip("*")) for d in body.split(";") if d.strip()]


def test_header_declares_the_functions_and_the_structs(cabi):
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    for proto in ("int egr_prior_pairs(int device, const egr_prior_pairs_args *args, void *hip_stream);", "int egr_prior_fit(int device, const egr_prior_fit_args *args, void *hip_stream);",
                  "int egr_prior_finish(int device, const egr_prior_finish_args *args, void *hip_stream);", "const char *egr_prior_last_error(void);"):
        assert proto in hdr, proto
    assert hdr.index("CONTEXT-FREE FUNCTIONS") < hdr.index("int egr_prior_pairs(")
    for name, value in (("EGR_PRIOR_CAM_FLOATS", "%d" % cabi.EGR_PRIOR_CAM_FLOATS), ("EGR_PRIOR_RANSAC", "%du" % cabi.EGR_PRIOR_RANSAC), ("EGR_PRIOR_LSTSQ", "%du" % cabi.EGR_PRIOR_LSTSQ),
                        ("EGR_PRIOR_MAX_SAMPLE", "%d" % cabi.EGR_PRIOR_MAX_SAMPLE)):
        assert "#define %s %s " % (name, value) in hdr, name
    assert (cabi.EGR_PRIOR_CAM_FLOATS, cabi.EGR_PRIOR_RANSAC, cabi.EGR_PRIOR_LSTSQ, cabi.EGR_PRIOR_MAX_SAMPLE) == (25, 0, 1, 1024)
    pairs, fit, finish = cabi.egr_prior_pairs_args, cabi.egr_prior_fit_args, cabi.egr_prior_finish_args
    assert struct_fields(hdr, "egr_prior_pairs_args") == [f[0] for f in pairs._fields_] == [
        "num_views", "height", "width", "depth_channels", "cams", "points", "offsets", "offsets_dev", "depth", "sparse", "pairs_x", "pairs_y", "count", "dropped"]
    assert C.sizeof(pairs) == 4 * 4 + 10 * 8
    assert struct_fields(hdr, "egr_prior_fit_args") == [f[0] for f in fit._fields_] == [
        "num_views", "pair_stride", "num_iters", "sample_stride", "method", "reserved", "pairs_x", "pairs_y", "views", "views_dev", "samples", "samples_dev", "hyp_error", "hyp_model", "ab",
        "best_iteration", "best_error", "inliers"]
    assert C.sizeof(fit) == 6 * 4 + 12 * 8
    assert struct_fields(hdr, "egr_prior_finish_args") == [f[0] for f in finish._fields_] == [
        "num_views", "height", "width", "depth_channels", "cams", "ab", "depth", "normal", "metalness", "distance", "normal_out", "f0"]
    assert C.sizeof(finish) == 4 * 4 + 8 * 8
    for st in (pairs, fit, finish):
        assert all(f[1] is C.c_uint32 for f in st._fields_ if f[0] in ("num_views", "height", "width", "depth_channels", "pair_stride", "num_iters", "sample_stride", "method", "reserved"))
    # the contract is written down
    for word in ("BEFORE any HIP call", "rounded to even, as torch.round", "NEAREST point", "+inf = EMPTY", "ROW-MAJOR order", "is DROPPED", "no global counter", "in fp64 by centred normal",
                 "in sample order", "minimum-norm solution", "4-pass 8-bit radix select", "in a fixed order, without atomics", "ties at the threshold do not change it",
                 "the lowest iteration among equals", "in pair order (the tie rule", "read from DEVICE memory", "A zero normal gives NaN", "0.04f * (1 - m) + m",
                 "a = 1, b = 0, best_iteration = -1", "offsets that do not ascend", "a sample index < 0 or >="):
        assert word in hdr, word


def test_symbols_resolve_with_prototypes(L):
    for name in ("egr_prior_pairs", "egr_prior_fit", "egr_prior_finish"):
        assert len(getattr(L, name).argtypes) == 3, name
    assert L.egr_prior_last_error.restype is C.c_char_p
    assert L.egr_version() == b"egr-hip 0.8 (gfx950)"  # additive symbols: the library still answers as before


def test_torch_ops_exist_with_their_schemas():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.prior_pairs.default._schema) == ("egr::prior_pairs(Tensor cams, Tensor points, int[] offsets, Tensor depth) -> (Tensor sparse, Tensor pairs_x, Tensor pairs_y, "
                                                             "Tensor count, Tensor dropped)")
    assert str(torch.ops.egr.prior_fit.default._schema) == ("egr::prior_fit(Tensor pairs_x, Tensor pairs_y, int[] counts, int[] sample_sizes, int[] top_ks, Tensor? samples, int method=0, "
                                                           "bool want_mask=False) -> (Tensor ab, Tensor best_iteration, Tensor best_error, Tensor hyp_error, Tensor hyp_model, Tensor inliers)")
    assert str(torch.ops.egr.prior_finish.default._schema) == ("egr::prior_finish(Tensor cams, Tensor ab, Tensor depth, Tensor normal, Tensor? metalness) -> (Tensor distance, "
                                                              "Tensor normal_world, Tensor f0)")
    with pytest.raises(RuntimeError, match="GPU tensor"):  # no CPU path
        torch.ops.egr.prior_pairs(torch.zeros((1, 25)), torch.zeros((0, 3)), [0, 0], torch.zeros((1, 2, 2, 1)))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.egr.prior_fit(torch.zeros((1, 4)), torch.zeros((1, 4)), [4], [2], [1], torch.zeros((1, 1, 2), dtype=torch.int32), 0, False)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        torch.ops.egr.prior_finish(torch.zeros((1, 25)), torch.zeros((1, 2)), torch.zeros((1, 2, 2, 1)), torch.zeros((1, 2, 2, 3)), None)


def pairs(L, cabi, args=True, offsets=(0, 3, 3), **over):
    """2 views of 4 x 6 with 3 + 0 points; `over` replaces fields."""
    off = None if offsets is None else (C.c_uint32 * len(offsets))(*offsets)
    a = dict(num_views=2, height=4, width=6, depth_channels=1, cams=CAMS, points=POINTS, offsets=off, offsets_dev=OFFS, depth=DEPTH, sparse=SPARSE, pairs_x=PX, pairs_y=PY, count=COUNT,
             dropped=DROPPED)
    a.update(over)
    return L.egr_prior_pairs(0, C.byref(cabi.egr_prior_pairs_args(**a)) if args else None, None)


def test_pairs_refusals(L, cabi):
    named = lambda what: "libegr_hip: egr_prior_pairs: " in error(L) and what in error(L)
    assert pairs(L, cabi, args=False) != 0 and named("args")
    for field in ("cams", "offsets", "offsets_dev", "depth"):
        assert pairs(L, cabi, **{field: None}) != 0 and named("required"), field
    for field in ("sparse", "pairs_x", "pairs_y", "count", "dropped"):
        assert pairs(L, cabi, **{field: None}) != 0 and named("required outputs"), field
    assert pairs(L, cabi, points=None) != 0 and named("points is required")
    for bad in (dict(num_views=0), dict(num_views=65536)):
        assert pairs(L, cabi, offsets=(0,) * 65537, **bad) != 0 and named("num_views"), bad
    for bad in (dict(height=0), dict(width=0), dict(height=65536), dict(width=65536)):
        assert pairs(L, cabi, **bad) != 0 and named("1..65535"), bad
    for ch in (0, 2, 4):
        assert pairs(L, cabi, depth_channels=ch) != 0 and named("depth_channels"), ch
    assert pairs(L, cabi, offsets=(0, 3, 2)) != 0 and named("do not ascend") and "view 1" in error(L)
    assert pairs(L, cabi, offsets=(1, 3, 3)) != 0 and named("start at 0")
    assert pairs(L, cabi, depth=DEPTH + 2) != 0 and named("misaligned")
    # an output overlapping an input or another output: 2 views of 4 x 6 are 192 bytes per fp32 image array, the cameras 200, the points 36
    assert pairs(L, cabi, sparse=DEPTH + 188) != 0 and named("overlaps an input")
    assert pairs(L, cabi, pairs_x=CAMS + 196) != 0 and named("overlaps an input")
    assert pairs(L, cabi, count=POINTS + 32) != 0 and named("overlaps an input")
    assert pairs(L, cabi, dropped=OFFS + 8) != 0 and named("overlaps an input")
    assert pairs(L, cabi, pairs_y=PX + 188) != 0 and named("two outputs")
    assert pairs(L, cabi, dropped=COUNT + 4) != 0 and named("two outputs")


def fit(L, cabi, args=True, views=(8, 2, 1, 0, 8, 2, 1, 0), samples=(0, 7, 1, 2, 3, 4) * 2, **over):
    """2 views with 8 pairs of a stride of 24, 3 iterations of 2 samples; `over` replaces fields."""
    vw = None if views is None else (C.c_uint32 * len(views))(*views)
    sm = None if samples is None else (C.c_int32 * len(samples))(*samples)
    a = dict(num_views=2, pair_stride=24, num_iters=3, sample_stride=2, method=0, pairs_x=PX, pairs_y=PY, views=vw, views_dev=VIEWS, samples=sm, samples_dev=SAMPLES, hyp_error=HERR,
             hyp_model=HMODEL, ab=AB, best_iteration=BEST_IT, best_error=BEST_ERR, inliers=MASK)
    a.update(over)
    return L.egr_prior_fit(0, C.byref(cabi.egr_prior_fit_args(**a)) if args else None, None)


def test_fit_refusals(L, cabi):
    named = lambda what: "libegr_hip: egr_prior_fit: " in error(L) and what in error(L)
    assert fit(L, cabi, args=False) != 0 and named("args")
    for field in ("pairs_x", "pairs_y", "views", "views_dev"):
        assert fit(L, cabi, **{field: None}) != 0 and named("required"), field
    for field in ("ab", "best_iteration", "best_error"):
        assert fit(L, cabi, **{field: None}) != 0 and named("required outputs"), field
    for field in ("samples", "samples_dev"):
        assert fit(L, cabi, **{field: None}) != 0 and named("samples and samples_dev"), field
    for field in ("hyp_error", "hyp_model"):
        assert fit(L, cabi, **{field: None}) != 0 and named("hyp_error and hyp_model"), field
    assert fit(L, cabi, method=2) != 0 and named("unknown method")
    for bad in (dict(num_views=0), dict(num_views=65536)):
        assert fit(L, cabi, **bad) != 0 and named("num_views"), bad
    assert fit(L, cabi, pair_stride=0) != 0 and named("pair_stride") and fit(L, cabi, pair_stride=65535 * 65535 + 1) != 0 and named("pair_stride")
    for bad in (dict(num_iters=0), dict(num_iters=65536)):
        assert fit(L, cabi, **bad) != 0 and named("num_iters"), bad
    for bad in (dict(sample_stride=0), dict(sample_stride=1025)):
        assert fit(L, cabi, **bad) != 0 and named("sample_stride"), bad
    assert fit(L, cabi, views=(25, 2, 1, 0, 8, 2, 1, 0)) != 0 and named("exceeds pair_stride") and "view 0" in error(L)
    for s in (1, 3, 9):  # below 2, above the table's width, above the count
        assert fit(L, cabi, views=(8, 2, 1, 0, 8, s, 1, 0), sample_stride=2 if s < 9 else 16, samples=(0,) * 96) != 0 and named("sample_size") and "view 1" in error(L), s
    for k in (0, 9):
        assert fit(L, cabi, views=(8, 2, k, 0, 8, 2, 1, 0)) != 0 and named("top_k"), k
    assert fit(L, cabi, samples=(0, 7, 1, 2, 3, 8) + (0, 1) * 3) != 0 and named("sample index 8") and "iteration 2" in error(L) and "view 0" in error(L)
    assert fit(L, cabi, samples=(0, 1) * 5 + (-1, 0)) != 0 and named("sample index -1") and "view 1" in error(L)
    assert fit(L, cabi, ab=AB + 2) != 0 and named("misaligned") and fit(L, cabi, best_error=BEST_ERR + 4) != 0 and named("doubles")
    # overlaps: the pair lists are 192 bytes each, the device views 32, the table 48, hyp_error 48, hyp_model 96, ab 16, best_iteration 8, best_error 16, the mask 48
    assert fit(L, cabi, ab=PX + 188) != 0 and named("overlaps an input")
    assert fit(L, cabi, inliers=PY - 44) != 0 and named("overlaps an input")
    assert fit(L, cabi, hyp_model=SAMPLES + 44) != 0 and named("overlaps an input")
    assert fit(L, cabi, best_iteration=VIEWS + 28) != 0 and named("overlaps an input")
    assert fit(L, cabi, best_error=HERR + 40) != 0 and named("two outputs")
    assert fit(L, cabi, inliers=AB + 12) != 0 and named("two outputs")
    # least squares reads no table: its rows are not looked at, and the ranges of the hypotheses are empty there (the overlap below is of the mask)
    assert fit(L, cabi, method=1, samples=(99,) * 12, hyp_model=SAMPLES, inliers=PX + 188) != 0 and named("overlaps an input")


def finish(L, cabi, args=True, **over):
    a = dict(num_views=2, height=4, width=6, depth_channels=1, cams=CAMS, ab=AB, depth=DEPTH, normal=NORMAL, metalness=METAL, distance=DIST, normal_out=NOUT, f0=F0)
    a.update(over)
    return L.egr_prior_finish(0, C.byref(cabi.egr_prior_finish_args(**a)) if args else None, None)


def test_finish_refusals(L, cabi):
    named = lambda what: "libegr_hip: egr_prior_finish: " in error(L) and what in error(L)
    assert finish(L, cabi, args=False) != 0 and named("args")
    for field in ("cams", "ab", "depth", "normal"):
        assert finish(L, cabi, **{field: None}) != 0 and named("required"), field
    for field in ("distance", "normal_out"):
        assert finish(L, cabi, **{field: None}) != 0 and named("required outputs"), field
    assert finish(L, cabi, f0=None) != 0 and named("f0 is a required output")
    for bad in (dict(num_views=0), dict(num_views=65536)):
        assert finish(L, cabi, **bad) != 0 and named("num_views"), bad
    for bad in (dict(height=0), dict(width=0), dict(height=65536), dict(width=65536)):
        assert finish(L, cabi, **bad) != 0 and named("1..65535"), bad
    assert finish(L, cabi, depth_channels=2) != 0 and named("depth_channels")
    assert finish(L, cabi, normal=NORMAL + 1) != 0 and named("misaligned")
    # overlaps: 2 views of 4 x 6 are 192 bytes per channel
    assert finish(L, cabi, distance=DEPTH) != 0 and named("overlaps an input")  # in place is refused
    assert finish(L, cabi, normal_out=NORMAL + 572) != 0 and named("overlaps an input")
    assert finish(L, cabi, f0=METAL - 572) != 0 and named("overlaps an input")
    assert finish(L, cabi, distance=AB + 12) != 0 and named("overlaps an input")
    assert finish(L, cabi, f0=NOUT + 572) != 0 and named("two outputs")
    assert finish(L, cabi, depth_channels=3, distance=DEPTH + 572) != 0 and named("overlaps an input")  # three channels are three times the bytes


def test_last_error_speaks_for_its_module_only(L, cabi):
    assert finish(L, cabi, depth_channels=2) != 0
    mine = error(L)
    assert "egr_prior_finish" in mine
    assert L.egr_viewset_gather(0, None, None, 0, None, None) != 0  # another module fails ...
    assert "egr_viewset_gather" in L.egr_viewset_last_error().decode() and error(L) == mine  # ... and says so in its own string only
    assert pairs(L, cabi, depth_channels=2) != 0 and "egr_prior_pairs" in error(L) and "egr_viewset_gather" in L.egr_viewset_last_error().decode()
