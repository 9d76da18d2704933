"""CPU checks of the launch entry that reads its targets in place (include/egr_raytracer.h: egr_raytrace_targets): the header text, the exported symbol,
the ctypes mirror, the torch schema, and what is refused before any HIP call."""
import ctypes as C
import importlib
import os
import re

import pytest

pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "egr_raytracer.h")
PROTOTYPE = r"\bint egr_raytrace_targets\(egr_context \*ctx, int grads_enabled, const egr_gaussians \*dst, const float \*const \*targets, void \*hip_stream\);"


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


def test_declared_and_exported(cabi):
    hdr = open(HEADER).read()
    assert re.search(PROTOTYPE, hdr)
    comment = hdr[:re.search(PROTOTYPE, hdr).start()].rsplit("/*", 1)[1]  # the contract in front of the prototype
    for words in ("diffuse, specular, depth, normal, roughness, f0", "C = 3, 3, 1, 3, 1, 3", "NULL entry", "valid and unmodified until the launch has completed",
                  "neither reads nor writes framebuffer.target_*", "grads_enabled == 0"):
        assert words in comment, words
    assert hasattr(cabi.lib(), "egr_raytrace_targets")  # dlsym


def test_the_ctypes_mirror(cabi):
    L = cabi.lib()
    assert L.egr_raytrace_targets.argtypes == [C.c_void_p, C.c_int, C.POINTER(cabi.egr_gaussians), C.POINTER(C.c_void_p * 6), C.c_void_p]
    assert callable(cabi.RawRaytracer.raytrace_targets)
    assert cabi.TRAIN_BATCH_TARGETS == ("target_diffuse", "target_specular", "target_depth", "target_normal", "target_roughness", "target_f0")  # the order of the six


def test_the_version_string_stays(cabi):
    assert cabi.lib().egr_version() == b"egr-hip 0.8 (gfx950)"  # an additive symbol


def test_a_null_context_is_refused_before_any_hip_call(cabi):
    """No context can exist on a machine without a GPU: the call must come back non-zero (not crash, not reach the HIP runtime), and egr_last_error has
    words for it. The refusals that need a context run on a live one in tests/test_hip_targets_in_place_c_abi.py."""
    L = cabi.lib()
    g = cabi.egr_gaussians(count=1)
    six = (C.c_void_p * 6)()
    for grads in (0, 1):
        assert L.egr_raytrace_targets(None, grads, None, None, None) != 0
        assert L.egr_raytrace_targets(None, grads, C.byref(g), C.byref(six), None) != 0
    assert b"null context" in L.egr_last_error(None)


def test_the_torch_binding_takes_both_optional_arguments():
    src = open(os.path.join(ROOT, PKG, "csrc", "torch_binding.cpp")).read()
    assert 'torch::arg("import_into") = c10::IValue(), torch::arg("targets") = c10::IValue()' in src  # raytrace(import_into=None, targets=None)
    assert "egr_raytrace_targets(ctx, 1," in src


def test_what_the_renderer_hands_to_the_launch():
    """GaussianRaytracer._targets_in_place: the images as the native checks take them, or None for the upload path."""
    import torch

    ren = importlib.import_module(PKG + ".renderer")
    rt = ren.GaussianRaytracer.__new__(ren.GaussianRaytracer)  # (no tracer without a GPU: the method reads the image size only)
    rt.image_width, rt.image_height = 5, 3
    dev = torch.device("cpu")
    good = [torch.zeros(c, 3, 5) for c in ren.GaussianRaytracer.TARGET_CHANNELS]
    assert ren.GaussianRaytracer.TARGET_CHANNELS == (3, 3, 1, 3, 1, 3)
    assert rt._targets_in_place(good, dev) == good
    assert rt._targets_in_place([None] * 6, dev) == [None] * 6
    assert rt._targets_in_place([good[0], None, good[2], None, None, good[5]], dev) is not None
    for k, bad in ((0, torch.zeros(3, 5, 3).moveaxis(-1, 0)), (2, torch.zeros(1, 3, 5, dtype=torch.float64)), (3, torch.zeros(3, 5, 3)), (4, torch.zeros(0)), (5, torch.zeros(3, 3, 6)[:, :, :5]),
                   (1, torch.zeros(3, 3, 5, device="meta"))):
        assert rt._targets_in_place(good[:k] + [bad] + good[k + 1:], dev) is None, k
