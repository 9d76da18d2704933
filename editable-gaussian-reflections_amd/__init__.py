"""MI355X-native drop-in for the hot path of graphdeco-inria/editable-gaussian-reflections.

Mirrors editable_gauss_refl/__init__.py:15-27: `make_raytracer(...)` loads `libraytracer.so` with
`torch.classes.load_library` and returns `torch.classes.raytracer.Raytracer(...)`. The library is the
TORCH_LIBRARY shim over the HIP C ABI (include/egr_raytracer.h); there is no CPU fallback and no second
backend: if the native libraries are missing or no GPU is present this fails loudly.
"""
import os

from .build import lib_paths, variant_dir, variant_name

# The build-time settings that select a variant build (build.py: VARIANT_SETTINGS) select the same library here; none set: the product in build/.
VARIANT = variant_name(os.environ)
BUILD_DIR = variant_dir(os.environ)
HIP_LIB_PATH, GAUSS_TRACER_PATH = lib_paths(os.environ)
LOADED = False


def load_library():
    global LOADED
    if not LOADED:
        import torch

        if VARIANT and not (os.path.exists(GAUSS_TRACER_PATH) and os.path.exists(HIP_LIB_PATH)):  # selected but not built: never the product in its place
            raise RuntimeError(
                f"variant build '{VARIANT}' is selected by the environment but not built: expected {GAUSS_TRACER_PATH} and {HIP_LIB_PATH}; "
                "run `tools/build_variant.sh` with the same settings")
        if not (os.path.exists(GAUSS_TRACER_PATH) and os.path.exists(HIP_LIB_PATH)):
            raise RuntimeError(
                f"native libraries not built: expected {GAUSS_TRACER_PATH} and {HIP_LIB_PATH}; "
                "run `python -c 'import __graft_entry__ as g; g.build()'` (there is no Python/CPU fallback)")
        torch.classes.load_library(GAUSS_TRACER_PATH)
        LOADED = True


def make_raytracer(image_width: int, image_height: int, num_gaussians: int, ppll_forward_size: int = 180_000_000,
                   ppll_backward_size: int = 120_000_000):
    """Same signature and defaults as the reference's make_raytracer (editable_gauss_refl/__init__.py:15-27)."""
    import torch

    load_library()
    return torch.classes.raytracer.Raytracer(image_width, image_height, num_gaussians, ppll_forward_size, ppll_backward_size)
