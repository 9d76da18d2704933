"""CPU checks of the SSIM addition (include/egr_raytracer.h: egr_eval_ssim, egr_ssim_images): the numpy fp64 restatement of the definition
(tests/ssim_restatement.py) against tests/golden/ssim_vectors.npz - the reference's own ssim evaluated on fp64 tensors (make_ssim_vectors.py) -, its interior
flavour against an independent "valid" convolution, and the ABI: the header text, the ctypes mirror, the exported symbols, the torch ops and the argument
validation, which runs before any HIP call, so none of this needs a device.

The bound against the reference, 1e-5 absolute: the restatement differs from the reference's fp64 evaluation by at most 1.2e-7 on every case but the flat
0.5 / 0.75 pair, where it is 2.6e-6 - upstream's 2-D window, an fp32 outer product of fp32 weights, does not sum to 1 (off by about 1e-8), and on a flat region
the variance terms are that error divided by C2. 1e-5 is 4 x the worst case (the generator prints the distances; the reference's own fp32 result is 1.9e-4 away
from its fp64 evaluation on that pair)."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import ssim_restatement as sr  # noqa: E402

PKG = "editable-gaussian-reflections_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "egr_raytracer.h")
BOUND = 1e-5
CASES = ("random_1x1", "random_5x7", "random_12x10", "random_11x11", "random_16x24", "random_37x53", "random_45x70", "flat_050_075", "flat_identical", "zeros",
         "ones_vs_zeros", "ramp_noise", "binary_complement")
A, B, T, S, P, WS = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x40001000, 0x70000000  # fake "device pointers", far apart, 8-byte aligned


@pytest.fixture(scope="module")
def vec():
    v = dict(np.load(os.path.join(ROOT, "tests", "golden", "ssim_vectors.npz")))
    assert sorted(k[:-2] for k in v if k.endswith("_a")) == sorted(CASES)
    return v


@pytest.mark.parametrize("name", CASES)
def test_restatement_against_the_reference_in_fp64(vec, name):
    a, b = vec[name + "_a"], vec[name + "_b"]
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and a.shape[0] == 3
    m = sr.ssim_map(a, b)
    full = float(sr.means(m)[0])
    per_channel = sr.sums(m)[:, 0] / (a.shape[1] * a.shape[2])
    d = max(abs(full - float(vec[name + "_ssim64"])), float(np.abs(per_channel - vec[name + "_ssim64_channels"]).max()))
    print(f"{name}: restatement - reference fp64 {d:.2e}; reference fp32 - fp64 {abs(float(vec[name + '_ssim32']) - float(vec[name + '_ssim64'])):.2e}")
    assert d <= BOUND, (name, d)
    assert abs(full - per_channel.mean()) < 1e-15


def test_the_fixture_holds_the_hard_cases(vec):
    assert float(vec["binary_complement_ssim64"]) < -0.5 and float(vec["flat_identical_ssim64"]) == 1.0 and float(vec["zeros_ssim64"]) == 1.0
    assert 0.0 < float(vec["ones_vs_zeros_ssim64"]) < 1e-3
    # the flat pair is where fp32 fails: the reference's own fp32 result is further from its fp64 evaluation than the bound of this file
    assert abs(float(vec["flat_050_075_ssim32"]) - float(vec["flat_050_075_ssim64"])) > 10 * BOUND
    assert abs(sr.WINDOW.sum() - 1.0) < 1e-15 and np.array_equal(sr.WINDOW, sr.WINDOW[::-1])


def valid_mean(p, g):
    """The mean of the SSIM map over the pixels whose window lies inside the image, from a "valid" 2-D convolution with the 121-tap window: no padding involved."""
    p, g = p.astype(np.float64), g.astype(np.float64)
    H, W = p.shape[-2:]
    w2 = np.outer(sr.WINDOW, sr.WINDOW)
    conv = lambda a: sum(w2[i, j] * a[:, i : i + H - 10, j : j + W - 10] for i in range(11) for j in range(11))
    mu1, mu2 = conv(p), conv(g)
    s1, s2, s12 = conv(p * p) - mu1**2, conv(g * g) - mu2**2, conv(p * g) - mu1 * mu2
    return float((((2 * mu1 * mu2 + sr.C1) * (2 * s12 + sr.C2)) / ((mu1**2 + mu2**2 + sr.C1) * (s1 + s2 + sr.C2))).mean())


@pytest.mark.parametrize("name", CASES)
def test_interior_flavour_is_the_valid_convolution(vec, name):
    a, b = vec[name + "_a"], vec[name + "_b"]
    interior = float(sr.means(sr.ssim_map(a, b))[1])
    if min(a.shape[1:]) < 11:
        assert np.isnan(interior)
        return
    want = valid_mean(a, b)
    # both are fp64 evaluations of the same 121 products per moment in another order: the bound of the GPU test (22 roundings of values in [0, 1], amplified by 1 / C2)
    assert abs(interior - want) <= 1e-9, (name, interior, want)
    if name == "random_11x11":  # one interior pixel per channel
        assert abs(interior - float(sr.ssim_map(a, b)[:, 5, 5].mean())) < 1e-15


def test_nan_poisons_its_neighbourhood_only():
    rng = np.random.default_rng(3)
    a, b = rng.random((3, 30, 30)), rng.random((3, 30, 30))
    a[1, 20, 7] = np.nan
    m = sr.ssim_map(a, b)
    want = np.zeros((3, 30, 30), bool)
    want[1, 15:26, 2:13] = True
    assert np.array_equal(np.isnan(m), want)
    assert np.isnan(sr.means(m)).all() and np.isnan(sr.sums(m)[1]).all() and np.isfinite(sr.sums(m)[[0, 2]]).all()


# ---- the ABI


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
    assert ("int egr_eval_ssim(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *final, const float *rgb, const float *target_final, "
            "const float *target_diffuse, const float *target_specular, double *ssim_sum, double *ssim, void *workspace, void *hip_stream);") in hdr
    assert ("int egr_ssim_images(int device, uint32_t num_views, uint32_t height, uint32_t width, const float *pred, const float *gt, double *ssim_sum, double *ssim, "
            "void *workspace, void *hip_stream);") in hdr
    text = open(HEADER).read()
    for word in ("e[k] = exp(-(k - 5)^2 / (2 * 1.5^2))", "never read", "C1 = 1e-4, C2 = 9e-4", "interior", "NaN when H < 11 or W < 11", "UNPINNED", "fp64 throughout",
                 "exactly separable", "No float atomics", "BEFORE any HIP call", "egr_eval_last_error()"):
        assert word in text, word
    assert 'return "egr-hip 0.8 (gfx950)"' in open(os.path.join(ROOT, PKG, "csrc", "api.hip")).read()  # additive symbols: the version stays


def test_workspace_size_mirror(cabi):
    text = open(HEADER).read()
    assert "#define EGR_SSIM_TILE %du" % cabi.EGR_SSIM_TILE in text
    assert "#define EGR_SSIM_BLOCKS(H, W) ((((size_t)(H) + EGR_SSIM_TILE - 1) / EGR_SSIM_TILE) * (((size_t)(W) + EGR_SSIM_TILE - 1) / EGR_SSIM_TILE))" in text
    assert "#define EGR_SSIM_WORKSPACE_BYTES(V, H, W) ((size_t)(V) * EGR_SSIM_BLOCKS(H, W) * (18 * 8))" in text
    assert [cabi.ssim_workspace_bytes(*a) for a in ((1, 1, 1), (3, 32, 32), (1, 33, 32), (8, 1080, 1920), (2, 37, 53))] == [144, 432, 288, 8 * 34 * 60 * 144, 2 * 4 * 144]


def test_symbols_resolve_with_prototypes(L):
    assert len(L.egr_eval_ssim.argtypes) == 13 and len(L.egr_ssim_images.argtypes) == 10
    assert L.egr_eval_last_error.restype is C.c_char_p
    assert L.egr_version().decode().startswith("egr-hip 0.8 ")


def test_torch_ops_exist():
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.eval_ssim.default._schema) == (
        "egr::eval_ssim(Tensor final, Tensor? rgb, Tensor? target_final, Tensor? target_diffuse, Tensor? target_specular) -> (Tensor ssim_sum, Tensor ssim)")
    assert str(torch.ops.egr.ssim_images.default._schema) == "egr::ssim_images(Tensor pred, Tensor gt) -> (Tensor ssim_sum, Tensor ssim)"
    ev = importlib.import_module(PKG + ".evaluation")
    with pytest.raises(ValueError, match="GPU tensors"):
        ev.ssim(torch.zeros(3, 12, 12), torch.zeros(3, 12, 12))  # no second arithmetic for the CPU


def eval_ssim(L, V=2, H=19, W=37, final=A, rgb=B, tf=T, td=T + 0x1000000, ts=T + 0x2000000, ssum=S, ssim=P, workspace=WS):
    return L.egr_eval_ssim(0, V, H, W, final, rgb, tf, td, ts, ssum, ssim, workspace, None)


def ssim_images(L, V=2, H=19, W=37, pred=A, gt=B, ssum=S, ssim=P, workspace=WS):
    return L.egr_ssim_images(0, V, H, W, pred, gt, ssum, ssim, workspace, None)


def test_eval_ssim_validation(L):
    assert eval_ssim(L, V=0) != 0 and "egr_eval_ssim: num_views" in error(L)
    assert eval_ssim(L, V=65536) != 0 and "num_views" in error(L)
    assert eval_ssim(L, H=0) != 0 and "height" in error(L)
    assert eval_ssim(L, W=0) != 0 and "width" in error(L)
    assert eval_ssim(L, final=None) != 0 and "final is required" in error(L)
    assert eval_ssim(L, ssum=None) != 0 and eval_ssim(L, ssim=None) != 0 and "required outputs" in error(L)
    assert eval_ssim(L, workspace=None) != 0 and "workspace" in error(L)
    assert eval_ssim(L, workspace=WS + 4) != 0 and "workspace" in error(L)  # misaligned
    assert eval_ssim(L, rgb=None) != 0 and "need rgb" in error(L)  # a diffuse / specular target without the per-step radiance
    image = 2 * 19 * 37 * 3 * 4
    assert eval_ssim(L, workspace=A + image - 8) != 0 and "overlaps an input" in error(L)  # the workspace starts in the last words of final
    assert eval_ssim(L, workspace=B + 8) != 0 and "overlaps an input" in error(L)
    assert eval_ssim(L, ssum=T) != 0 and "overlaps an input" in error(L)
    assert eval_ssim(L, ssim=T + 0x2000000 + image - 8) != 0 and "overlaps an input" in error(L)  # the last word of target_specular
    assert eval_ssim(L, ssim=S + 2 * 18 * 8 - 8) != 0 and "two outputs" in error(L)  # ssim starts in the last word of ssim_sum
    assert eval_ssim(L, ssum=WS + 8) != 0 and "two outputs" in error(L)


def test_ssim_images_validation(L):
    assert ssim_images(L, V=0) != 0 and "egr_ssim_images: num_views" in error(L)
    assert ssim_images(L, V=65536) != 0 and "num_views" in error(L)
    assert ssim_images(L, H=0) != 0 and ssim_images(L, W=0) != 0 and "height and width" in error(L)
    assert ssim_images(L, pred=None) != 0 and "pred and gt are required" in error(L)
    assert ssim_images(L, gt=None) != 0 and "pred and gt are required" in error(L)
    assert ssim_images(L, ssum=None) != 0 and ssim_images(L, ssim=None) != 0 and "required outputs" in error(L)
    assert ssim_images(L, workspace=None) != 0 and ssim_images(L, workspace=WS + 4) != 0 and "workspace" in error(L)
    image = 2 * 19 * 37 * 3 * 4
    assert ssim_images(L, ssum=B + image - 8) != 0 and "overlaps an input" in error(L)  # the last word of gt
    assert ssim_images(L, workspace=A) != 0 and "overlaps an input" in error(L)
    assert ssim_images(L, ssim=S + 2 * 6 * 8 - 8) != 0 and "two outputs" in error(L)  # one pass: ssim_sum is [V][3][2], ssim starts in its last word
