"""the denoiser stand-in (csrc/denoise.hip, an edge-avoiding a-trous wavelet filter on output_final guided by
output_normal) against a plain PyTorch fp32 implementation of the same filter. Parity with the OptiX AI denoiser is unpinned."""
import importlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"


def atrous_reference(img, normal, sigma_c=0.6, sigma_n=0.3):
    """img, normal: [H,W,3] float32 GPU tensors. Same 5 passes / 25 taps / weights as k_atrous, written with torch ops."""
    h = torch.tensor([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=torch.float32, device=img.device)
    H, W, _ = img.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=img.device), torch.arange(W, device=img.device), indexing="ij")
    cur = img
    for p in range(5):
        hole = 1 << p
        acc = torch.zeros_like(cur)
        wsum = torch.zeros(H, W, 1, device=img.device)
        for j in range(-2, 3):
            for i in range(-2, 3):
                yy, xx = ys + j * hole, xs + i * hole
                ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).unsqueeze(-1).float()
                yc, xc = yy.clamp(0, H - 1), xx.clamp(0, W - 1)
                tap, ntap = cur[yc, xc], normal[yc, xc]
                wc = torch.exp(-((tap - cur) ** 2).sum(-1, keepdim=True) / sigma_c ** 2)
                wn = torch.exp(-((ntap - normal) ** 2).sum(-1, keepdim=True) / sigma_n ** 2)
                w = h[i + 2] * h[j + 2] * wc * wn * ok
                acc += w * tap
                wsum += w
        cur = acc / wsum
        sigma_c *= 0.5
    return cur


@pytest.fixture(scope="module")
def rt():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    ren = importlib.import_module(PKG + ".renderer")
    syn = importlib.import_module(PKG + ".synthetic")
    pc = ren.GaussianParams(syn.make_scene(3000, "trained", seed=2))
    return ren, syn, ren.GaussianRaytracer(pc, 160, 96)


def test_matches_torch_reference_on_a_render(rt):
    ren, syn, r = rt
    cam = syn.default_camera()
    camera = ren.camera_from_c2w(cam["origin"], cam["c2w"], cam["fov"])
    with torch.no_grad():
        r(camera, denoise=True)
    fb = r.cuda_module.get_framebuffer()
    assert fb.output_denoised.shape == fb.output_final.shape
    H, W = r.image_height, r.image_width
    final, out = fb.output_final.reshape(H, W, 3), fb.output_denoised.reshape(H, W, 3)
    ref = atrous_reference(final.clone(), fb.output_normal[0].clone())
    assert float((out - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max()))
    assert float((out - final).abs().max()) > 1e-4  # it is not the old copy


def test_properties_constant_noise_and_edges(rt):
    ren, syn, r = rt
    m = r.cuda_module
    fb = m.get_framebuffer()
    H, W = r.image_height, r.image_width
    final_view, den_view = fb.output_final.reshape(H, W, 3), fb.output_denoised.reshape(H, W, 3)
    g = torch.Generator(device="cuda").manual_seed(0)
    # constant image + constant normals -> unchanged
    fb.output_final.fill_(0.37)
    fb.output_normal.zero_()
    fb.output_normal[0, :, :, 2] = 1.0
    m.denoise()
    assert float((den_view - 0.37).abs().max()) < 1e-6
    # flat region with noise: variance drops a lot; a normal discontinuity in the middle keeps the two halves apart
    base = torch.zeros(H, W, 3, device="cuda")
    base[:, W // 2:] = 1.0
    noisy = base + 0.05 * torch.randn(H, W, 3, device="cuda", generator=g)
    final_view.copy_(noisy)
    fb.output_normal[0, :, W // 2:, 2] = 0.0
    fb.output_normal[0, :, W // 2:, 0] = 1.0
    m.denoise()
    out = den_view
    left, right = out[:, : W // 2], out[:, W // 2:]
    assert float(left.std()) < 0.012 and float(right.std()) < 0.012  # 0.05 -> ~0.005
    assert abs(float(left.mean())) < 0.01 and abs(float(right.mean()) - 1.0) < 0.01  # no bleeding across the edge
    ref = atrous_reference(noisy, fb.output_normal[0].clone())
    assert float((out - ref).abs().max()) < 2e-5


# ---- k_atrous through denoise_views and denoise() against the fp64 numpy restatement (tests/aux_restatement.py: atrous64, out-of-range taps skipped by slicing) ----
# Inputs are built on the CPU in fp64 from a fixed seed, rounded to fp32 and uploaded; the restatement reads the rounded values. The bar is the project's own,
# max |out - ref| < 2e-5 max(1, max |ref|): the fp32 torch restatement stays below 1.5 % of it on these inputs, the rest is room for __expf.
import functools  # noqa: E402

import aux_restatement as ar  # noqa: E402
from hip_common import ren, report, tracer  # noqa: E402,F401

SIZES = [(1, 1), (7, 70), (33, 9), (37, 19), (65, 33), (160, 96)]  # one pixel; narrower / lower than one 32 x 8 block and than the reach; ragged; block multiples
NV = 3


def _unit_normals(rng, V, H, W):
    n = rng.normal(size=(V, H, W, 3))
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


@functools.lru_cache(maxsize=None)
def case(W, H, kind="plain"):
    """(final fp32 [V,H,W,3], normal fp32, atrous64 of them) - computed once, shared, never written to."""
    rng = np.random.default_rng(1000 * W + H)
    if kind == "step" or (kind == "plain" and (W, H) == (65, 33)):  # the noisy step with a normal edge of test_properties_constant_noise_and_edges
        final = np.zeros((NV, H, W, 3))
        final[:, :, W // 2:] = 1.0
        final += 0.05 * rng.normal(size=final.shape)
        normal = np.zeros_like(final)
        normal[:, :, : W // 2, 2] = 1.0
        normal[:, :, W // 2:, 0] = 1.0
    elif kind == "hdr":
        final = 100.0 * rng.random((NV, H, W, 3)) ** 2
        final[1, H // 3, W // 3] = 1e4
        normal = _unit_normals(rng, NV, H, W)
    elif kind == "constant":
        final = np.full((NV, H, W, 3), 0.37)
        normal = np.zeros_like(final)
        normal[..., 2] = 1.0
    else:
        final = 2.0 * rng.random((NV, H, W, 3)) ** 2
        normal = _unit_normals(rng, NV, H, W)
    final, normal = final.astype(np.float32), normal.astype(np.float32)
    ref = ar.atrous64(final.astype(np.float64), normal.astype(np.float64))
    for a in (final, normal, ref):
        a.setflags(write=False)
    return final, normal, ref


@pytest.fixture(scope="module")
def tracers(ren, syn):
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = tracer(ren, syn, W=W, H=H, N=300)
        return made[(W, H)]

    return get


def denoise_views(r, final, normal):
    return r.cuda_module.denoise_views(torch.from_numpy(np.array(final)).cuda(), torch.from_numpy(np.array(normal)).cuda()).cpu().numpy()


def ratio_to_bar(out, ref):
    return float(np.abs(out - ref).max()) / (2e-5 * max(1.0, float(np.abs(ref).max())))


@pytest.mark.parametrize("W,H", SIZES)
def test_views_match_fp64_restatement(tracers, W, H):
    final, normal, ref = case(W, H)
    r = tracers(W, H)
    out = denoise_views(r, final, normal)
    assert out.shape == (NV, H, W, 3) and np.isfinite(out).all()
    q = ratio_to_bar(out, ref)
    report(f"denoise_{W}x{H}", ratio_to_bar=f"{q:.4f}", max_ref=f"{np.abs(ref).max():.3f}")
    assert q < 1.0
    if W * H > 1:
        assert float(np.abs(out - final).max()) > 1e-3  # it filters
    # view 0 through the framebuffer's own denoise(): the same kernel with strides 0, bit for bit
    m = r.cuda_module
    fb = m.get_framebuffer()
    fb.output_final.copy_(torch.from_numpy(np.array(final[0])).cuda().reshape(fb.output_final.shape))
    fb.output_normal[0].copy_(torch.from_numpy(np.array(normal[0])).cuda())
    m.denoise()
    assert np.array_equal(fb.output_denoised.reshape(H, W, 3).cpu().numpy(), out[0])


def test_hdr_values_stay_finite_and_within_the_bar(tracers):
    W, H = 160, 96
    final, normal, ref = case(W, H, "hdr")
    assert float(final.max()) == 1e4
    out = denoise_views(tracers(W, H), final, normal)
    assert np.isfinite(out).all()
    q = ratio_to_bar(out, ref)
    report("denoise_hdr_160x96", ratio_to_bar=f"{q:.4f}", max_ref=f"{np.abs(ref).max():.1f}")
    assert q < 1.0


@pytest.mark.parametrize("W,H,x,y", [(160, 96, 80, 48), (37, 19, 0, 0), (37, 19, 36, 18)])
def test_one_nan_pixel_reaches_exactly_the_pixels_that_read_it(tracers, W, H, x, y):
    """One NaN in view 1. The NaN mask of the output is atrous64's, to the pixel at every border: the hole sequence, the pass count and the skipped taps - which the
    numeric bar cannot see for the far taps, whose weight is (1/16)^5. Every other pixel, and the other views, are bit-equal to the run without the NaN."""
    final, normal, _ = case(W, H)
    r = tracers(W, H)
    clean = denoise_views(r, final, normal)
    marked = np.array(final)
    marked[1, y, x, 1] = np.nan
    out = denoise_views(r, marked, normal)
    want = np.isnan(ar.atrous64(marked[1:2].astype(np.float64), normal[1:2].astype(np.float64)))[0]
    assert np.array_equal(want.any(-1), want.all(-1)) and want[y, x].all()
    if (W, H) == (160, 96):  # 2 * (1 + 2 + 4 + 8 + 16) = 62 either side, clipped by the image
        box = np.zeros((H, W), bool)
        box[:, x - 62:x + 63] = True
        assert np.array_equal(want[..., 0], box)
    got = np.isnan(out)
    assert not got[0].any() and not got[2].any()
    assert np.array_equal(got[1], want), (int(got[1].sum()), int(want.sum()))
    keep = ~got
    assert np.array_equal(out[keep].view(np.uint32), clean[keep].view(np.uint32))


def test_constant_image_is_unchanged_at_a_ragged_size(tracers):
    final, normal, ref = case(37, 19, "constant")
    out = denoise_views(tracers(37, 19), final, normal)
    assert float(np.abs(out - 0.37).max()) < 1e-6 and float(np.abs(ref - np.float32(0.37)).max()) < 1e-15
