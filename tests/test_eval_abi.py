"""CPU checks of the evaluation ABI (include/egr_raytracer.h: egr_denoise_views, egr_eval_metrics, egr_eval_last_error, EGR_EVAL_WORKSPACE_BYTES): the header text,
the ctypes mirror, the exported symbols, the torch op and the shim method, and the argument validation of egr_eval_metrics - which runs before any HIP call, so all
of this needs no device. egr_denoise_views takes a context, which only exists on a GPU: here a NULL context is refused; its other refusals (V = 0, NULL final,
overlap, short stride) run on a real context with the same fake pointers in tests/test_hip_eval.py."""
import ctypes as C
import importlib
import os
import re

import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
A, B, T, S, P, D, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x40001000, 0x50000000, 0x70000000  # fake "device pointers", far apart, 8-byte aligned


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def error(L):
    return L.egr_eval_last_error().decode()


def test_header_declares_the_functions_and_states_the_contract():
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S))
    assert ("int egr_denoise_views(egr_context *ctx, uint32_t num_views, const float *final , const float *normal , size_t normal_view_stride , float *denoised , "
            "void *hip_stream);") in hdr
    assert ("int egr_eval_metrics(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *target_final, "
            "const float *target_diffuse, const float *target_specular, double *sse, double *psnr, float *display, void *workspace, void *hip_stream);") in hdr
    assert "const char *egr_eval_last_error(void);" in hdr
    text = open(HEADER).read()
    for word in ("bit-equal to egr_denoise", "fixed order", "NaN propagates", "BEFORE any HIP call", "PNG round trip"):
        assert word in text, word
    assert 'return "egr-hip 0.8 (gfx950)"' in open(os.path.join(os.path.dirname(HEADER), "..", PKG, "csrc", "api.hip")).read()  # additive symbols: the version stays


def test_workspace_size_mirror(cabi):
    # one partial of 9 fp64 sums per EGR_EVAL_PIXELS_PER_WG pixels and view
    G = cabi.EGR_EVAL_PIXELS_PER_WG
    text = open(HEADER).read()
    assert "#define EGR_EVAL_PIXELS_PER_WG %du" % G in text
    assert "#define EGR_EVAL_BLOCKS(H, W) (((size_t)(H) * (size_t)(W) + EGR_EVAL_PIXELS_PER_WG - 1) / EGR_EVAL_PIXELS_PER_WG)" in text
    assert "#define EGR_EVAL_WORKSPACE_BYTES(V, H, W) ((size_t)(V) * EGR_EVAL_BLOCKS(H, W) * (9 * 8))" in text
    assert [cabi.eval_workspace_bytes(*a) for a in ((1, 1, 1), (3, 1, G), (1, 1, G + 1), (8, 1080, 1920), (2, 19, 37))] == [72, 216, 144, 8 * 1013 * 72, 144]


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_eval_metrics.argtypes) == 14 and len(L.egr_denoise_views.argtypes) == 7
    assert L.egr_eval_last_error.restype is C.c_char_p
    assert L.egr_version().decode().startswith("egr-hip 0.8 ")
    assert L.egr_denoise_views(None, 1, A, B, 1 << 20, D, None) != 0  # a NULL context is refused, not dereferenced


def test_torch_op_and_method_exist():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.eval_metrics.default._schema) == (
        "egr::eval_metrics(Tensor final, Tensor? rgb, Tensor? target_final, Tensor? target_diffuse, Tensor? target_specular, bool want_display=False) -> "
        "(Tensor sse, Tensor psnr, Tensor display)")
    methods = {s.name: str(s) for s in torch._C._jit_get_custom_class_schemas()}
    assert methods.get("denoise_views") == "denoise_views(__torch__.torch.classes.raytracer.Raytracer _0, Tensor _1, Tensor _2) -> Tensor _0"
    assert hasattr(importlib.import_module(PKG + ".c_abi").RawRaytracer, "denoise_views")


def metrics(L, V=2, H=19, W=37, final=A, rgb=B, tf=T, td=T + 0x1000000, ts=T + 0x2000000, sse=S, psnr=P, display=None, workspace=WS):
    return L.egr_eval_metrics(0, V, H, W, final, rgb, tf, td, ts, sse, psnr, display, workspace, None)


def test_eval_metrics_validation(L):
    assert metrics(L, V=0) != 0 and "num_views" in error(L)
    assert metrics(L, V=65536) != 0 and "num_views" in error(L)
    assert metrics(L, H=0) != 0 and "height" in error(L)
    assert metrics(L, final=None) != 0 and "final is required" in error(L)
    assert metrics(L, sse=None) != 0 and metrics(L, psnr=None) != 0 and "required outputs" in error(L)
    assert metrics(L, workspace=None) != 0 and "workspace" in error(L)
    assert metrics(L, workspace=WS + 4) != 0 and "workspace" in error(L)  # misaligned
    assert metrics(L, rgb=None) != 0 and "need rgb" in error(L)  # a diffuse / specular target without the per-step radiance
    image = 2 * 19 * 37 * 3 * 4
    assert metrics(L, display=A + image - 4) != 0 and "overlaps an input" in error(L)  # display starts in the last word of final
    assert metrics(L, workspace=B + 8) != 0 and "overlaps an input" in error(L)
    assert metrics(L, sse=T) != 0 and "overlaps an input" in error(L)
    assert metrics(L, psnr=S + 8) != 0 and "two outputs" in error(L)
    assert metrics(L, display=WS - 8) != 0 and "two outputs" in error(L)
