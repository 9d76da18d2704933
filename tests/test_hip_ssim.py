"""SSIM on the GPU (csrc/ssim.hip; torch.ops.egr.ssim_images / eval_ssim, evaluation.evaluate_views(ssim=True), evaluation.ssim) against the numpy fp64
restatement of the definition (tests/ssim_restatement.py) and the reference's own fp64 values (tests/golden/ssim_vectors.npz).

The bound against the restatement, 1e-9 absolute on the means, is derived: each moment is at most 22 fp64 roundings of values in [0, 1], about 2.5e-15; the
worst amplification is 1 / C2 = 1.1e3; that gives about 1e-11 per map value, and the bound is 100 x that. A sum over n values is held to n x the bound. Against
the reference's fp64 values the bound is that of tests/test_ssim_host.py (1e-5: upstream's window does not sum to 1).
eval_ssim is compared with the restatement applied to the display images that eval_metrics returns for the same inputs: both kernels share one tone curve, and no
powf is compared across devices.
Measured on an MI355X (REPORT lines): the means are within 3.4e-16 of the restatement on every fixture case but the flat 0.5 / 0.75 pair (2.6e-13),
eval_ssim within 2.2e-16; the distance from the reference's fp64 values is the restatement's own (at most 1.2e-7, 2.6e-6 on the flat pair)."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import eval_restatement as er  # noqa: E402
import ssim_restatement as sr  # noqa: E402
from hip_common import cam_obj, ren, report, tracer, views  # noqa: E402,F401
from test_ssim_host import BOUND as REFERENCE_BOUND, CASES  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-9


@pytest.fixture(scope="module")
def ev(ren):
    mod = importlib.import_module(PKG + ".evaluation")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def vec():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "ssim_vectors.npz")))


def close(got, want, bound):
    """NaN in the same places, and the rest within `bound` (a scalar or an array); returns the largest distance."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), (got, want)
    d = np.nan_to_num(np.abs(got - want), nan=0.0)
    assert bool((d <= bound).all()), (float(d.max()), got, want)
    return float(d.max(initial=0.0))


def sum_bound(shape_hw, leading):
    """The bound of a sum: BOUND per value, for the [all pixels, interior] pair of an H x W image."""
    H, W = shape_hw
    return np.broadcast_to(np.array([H * W, max((H - 10) * (W - 10), 1)], np.float64) * BOUND, leading + (2,))


def images_op(a, b):
    s, m = torch.ops.egr.ssim_images(torch.as_tensor(a).cuda().contiguous(), torch.as_tensor(b).cuda().contiguous())
    return s, m


@pytest.mark.parametrize("name", CASES)
def test_ssim_images_on_the_fixture(ev, vec, name):
    a, b = vec[name + "_a"], vec[name + "_b"]
    H, W = a.shape[1:]
    s, m = images_op(a[None], b[None])
    assert s.shape == (1, 3, 2) and m.shape == (1, 2) and s.dtype == m.dtype == torch.float64
    want = sr.ssim_map(a, b)
    d_mean = close(m[0].cpu().numpy(), sr.means(want), BOUND)
    d_sum = close(s[0].cpu().numpy(), sr.sums(want), sum_bound((H, W), (3,)))
    d_ref = max(abs(float(m[0, 0]) - float(vec[name + "_ssim64"])), float(np.abs(s[0, :, 0].cpu().numpy() / (H * W) - vec[name + "_ssim64_channels"]).max()))
    report("ssim_images_" + name, mean_err=f"{d_mean:.2e}", sum_err=f"{d_sum:.2e}", distance_from_reference_fp64=f"{d_ref:.2e}", full=f"{float(m[0, 0]):.9f}",
           interior=f"{float(m[0, 1]):.9f}")
    assert d_ref <= REFERENCE_BOUND
    assert bool(torch.isnan(m[0, 1])) == (min(H, W) < 11)


def test_batched_views_are_bit_equal_to_single_calls(ev, vec):
    g = torch.Generator(device="cuda").manual_seed(21)
    rnd = lambda: torch.rand(3, 3, 37, 53, device="cuda", generator=g)
    stacks = [(np.stack([vec[n + "_a"] for n in names]), np.stack([vec[n + "_b"] for n in names])) for names in (("flat_050_075", "flat_identical"), ("zeros", "ones_vs_zeros"))]
    p = rnd()
    stacks.append((p.cpu().numpy(), (p + 0.1 * (rnd() - 0.5)).clamp(0, 1).cpu().numpy()))  # three different images at 37 x 53: several tiles per view
    for a, b in stacks:
        s, m = images_op(a, b)
        s2, m2 = images_op(a, b)
        assert torch.equal(s, s2) and torch.equal(m.nan_to_num(-2.0), m2.nan_to_num(-2.0))  # a second run: bit for bit
        close(m.cpu().numpy(), sr.means(sr.ssim_map(a, b)), BOUND)
        for v in range(a.shape[0]):
            s1, m1 = images_op(a[v : v + 1], b[v : v + 1])
            assert torch.equal(s1[0], s[v]) and torch.equal(m1[0].nan_to_num(-2.0), m[v].nan_to_num(-2.0)), v  # a view does not depend on its neighbours
    assert len({float(x) for x in m[:, 0]}) == 3


def raw_inputs(V, H, W, seed):
    """HDR predictions and noisy targets (as tests/test_hip_eval.py makes them); view 1 holds an exact 0, a NaN (display 0), a +inf (display 1) and a negative target
    (display NaN)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
    final = (3 * rnd(V, H, W, 3) ** 2).contiguous()
    rgb = (2 * rnd(V, 3, H, W, 3) ** 2).contiguous()
    noisy = lambda t: (t * (1 + 0.17 * torch.randn(t.shape, device="cuda", generator=g))).abs().contiguous()
    targets = [noisy(p) for p in er.predictions(final, rgb)]
    final[1, 3, 4, 0], final[1, 7, 30, 1], final[1, H - 1, W - 1, 2], final[1, 20, 20, :] = float("nan"), float("inf"), 0.0, 0.0
    targets[1][1, 1, 9, 11] = -0.01
    assert float(final[0].max()) > 1.0
    return final, rgb, targets


def restate_display(disp):
    """[V,3,2,3,H,W] display images of eval_metrics -> (sums [V,3,3,2], means [V,3,2]) by the restatement."""
    d = disp.cpu().numpy()
    m = sr.ssim_map(d[:, :, 0], d[:, :, 1])
    return sr.sums(m), sr.means(m)


@pytest.mark.parametrize("H,W", [(37, 53), (45, 70)])
def test_eval_ssim_against_the_restatement_of_the_display_images(ev, H, W):
    V = 2
    final, rgb, targets = raw_inputs(V, H, W, seed=300 + H)
    _, _, disp = torch.ops.egr.eval_metrics(final, rgb, *targets, True)
    assert int(torch.isnan(disp[0]).sum()) == 0 and int(torch.isnan(disp[1]).sum()) == 1 and bool(torch.isnan(disp[1, 1, 1, 1, 9, 11]))
    assert float(disp[1, 0, 0, 0, 3, 4]) == 0.0 and float(disp[1, 0, 0, 1, 7, 30]) == 1.0
    s, m = torch.ops.egr.eval_ssim(final, rgb, *targets)
    assert s.shape == (V, 3, 3, 2) and m.shape == (V, 3, 2) and s.dtype == m.dtype == torch.float64
    want_s, want_m = restate_display(disp)
    d_mean = close(m.cpu().numpy(), want_m, BOUND)
    d_sum = close(s.cpu().numpy(), want_s, sum_bound((H, W), (V, 3, 3)))
    # the NaN pixel (view 1, diffuse target, channel 1) poisons the two sums of its channel and the means of its pass, and nothing else
    want_nan = torch.zeros(V, 3, 3, 2, dtype=torch.bool)
    want_nan[1, 1, 1] = True
    assert torch.equal(torch.isnan(s).cpu(), want_nan) and torch.equal(torch.isnan(m).cpu(), want_nan.any(2))
    report(f"eval_ssim_{H}x{W}", mean_err=f"{d_mean:.2e}", sum_err=f"{d_sum:.2e}", full=[f"{float(x):.6f}" for x in m[0, :, 0]], interior=[f"{float(x):.6f}" for x in m[0, :, 1]])
    s2, m2 = torch.ops.egr.eval_ssim(final, rgb, *targets)
    same = lambda x, y: torch.equal(x.nan_to_num(-2.0), y.nan_to_num(-2.0))
    assert same(s, s2) and same(m, m2)  # bit for bit on every run
    # absent passes report NaN; the others do not change by a bit
    s_f, m_f = torch.ops.egr.eval_ssim(final, None, targets[0], None, None)
    assert same(s_f[:, 0], s[:, 0]) and same(m_f[:, 0], m[:, 0]) and bool(torch.isnan(s_f[:, 1:]).all()) and bool(torch.isnan(m_f[:, 1:]).all())
    s_n, m_n = torch.ops.egr.eval_ssim(final, rgb, targets[0], targets[1], None)
    assert same(s_n[:, :2], s[:, :2]) and same(m_n[:, :2], m[:, :2]) and bool(torch.isnan(s_n[:, 2]).all()) and bool(torch.isnan(m_n[:, 2]).all())
    # the plain-image loader on the display images: the same numbers as the raw loader, bit for bit (one kernel, two loaders)
    s_i, m_i = torch.ops.egr.ssim_images(disp[:, 0, 0].contiguous(), disp[:, 0, 1].contiguous())
    assert same(s_i, s[:, 0]) and same(m_i, m[:, 0])


def test_evaluate_views_with_ssim(ren, ev, syn):
    W, H, V, S, base = 48, 40, 3, 2, 20  # neither dimension a multiple of the 32 x 32 tile
    torch.manual_seed(7)
    rt = tracer(ren, syn, W=W, H=H, N=2000, seed=7)
    m = rt.cuda_module
    tg = syn.make_targets(W, H)
    cams = [cam_obj(ren, c, tg) for c in views(syn, V)]
    for i, c in enumerate(cams):
        c.diffuse_image = (c.diffuse_image * (1.0 + 0.1 * i)).contiguous()
        c.original_image = (c.diffuse_image + c.specular_image).contiguous()
    for denoise in (True, False):
        m.get_metadata().total_num_calls.fill_(base)
        plain = ev.evaluate_views(cams, rt, spp=S, denoise=denoise, views_per_call=2)
        assert int(m.get_metadata().total_num_calls) == base + V * S
        assert plain.ssim is None and plain.ssim_interior is None and plain.ssim_channels is None and plain.mean_ssim is None
        m.get_metadata().total_num_calls.fill_(base)
        res = ev.evaluate_views(cams, rt, spp=S, denoise=denoise, views_per_call=2, keep_images=True, ssim=True)
        assert int(m.get_metadata().total_num_calls) == base + V * S  # total_num_calls advances equally
        for name in ev.PASSES:
            assert torch.equal(res.psnr[name], plain.psnr[name]) and torch.equal(res.psnr_global[name], plain.psnr_global[name]) and torch.equal(res.sse[name], plain.sse[name])
            assert res.ssim[name].shape == res.ssim_interior[name].shape == (V,) and res.ssim_channels[name].shape == (V, 3) and res.ssim[name].dtype == torch.float64
            assert not res.ssim[name].is_cuda and res.mean_ssim[name] == float(res.ssim[name].mean())
            for v in range(V):
                mp = sr.ssim_map(getattr(res.images[v], name).cpu().numpy(), getattr(res.images[v], name + "_gt").cpu().numpy())
                full, interior = sr.means(mp)
                d = max(close(res.ssim[name][v].numpy(), full, BOUND), close(res.ssim_interior[name][v].numpy(), interior, BOUND),
                        close(res.ssim_channels[name][v].numpy(), sr.sums(mp)[:, 0] / (H * W), BOUND))
                report(f"evaluate_views_ssim_denoise{int(denoise)}_v{v}_{name}", ssim=f"{float(full):.6f}", interior=f"{float(interior):.6f}", err=f"{d:.2e}")
                assert -1.0 <= float(full) <= 1.0 and np.isfinite(interior)
        if denoise:
            denoised = res
    assert not torch.equal(denoised.ssim["final"], res.ssim["final"]) and torch.equal(denoised.ssim["diffuse"], res.ssim["diffuse"])  # the denoiser touches `final` alone
    # one chunk for all views gives the same numbers as chunks of two
    m.get_metadata().total_num_calls.fill_(base)
    res8 = ev.evaluate_views(cams, rt, spp=S, denoise=False, views_per_call=8, ssim=True)
    for name in ev.PASSES:
        assert torch.equal(res8.ssim[name], res.ssim[name]) and torch.equal(res8.ssim_interior[name], res.ssim_interior[name]) and torch.equal(res8.ssim_channels[name], res.ssim_channels[name])
    # a camera without one of the images: that pass is NaN for the whole call
    del cams[1].specular_image
    m.get_metadata().total_num_calls.fill_(base)
    res4 = ev.evaluate_views(cams, rt, spp=S, denoise=False, ssim=True)
    assert bool(torch.isnan(res4.ssim["specular"]).all()) and np.isnan(res4.mean_ssim["specular"]) and torch.equal(res4.ssim["final"], res.ssim["final"])
    empty = ev.evaluate_views([], rt, ssim=True)
    assert empty.ssim["final"].shape == (0,) and empty.ssim_channels["final"].shape == (0, 3) and np.isnan(empty.mean_ssim["final"])


def test_evaluation_ssim_on_images(ev, vec):
    a, b = torch.tensor(vec["random_37x53_a"]).cuda(), torch.tensor(vec["random_37x53_b"]).cuda()
    want = sr.means(sr.ssim_map(vec["random_37x53_a"], vec["random_37x53_b"]))
    full, interior = ev.ssim(a, b)
    assert full.is_cuda and full.dtype == torch.float64 and full.shape == interior.shape == ()
    close([float(full), float(interior)], want, BOUND)
    assert abs(float(full) - float(vec["random_37x53_ssim64"])) <= REFERENCE_BOUND
    full2, interior2 = ev.ssim(torch.stack([a, b]), torch.stack([b, b]))
    assert full2.shape == interior2.shape == (2,) and float(full2[0]) == float(full) and float(interior2[0]) == float(interior) and abs(float(full2[1]) - 1.0) < 1e-12
    with pytest.raises(ValueError, match="GPU tensors"):
        ev.ssim(a.cpu(), b.cpu())
    with pytest.raises(ValueError, match="must both be"):
        ev.ssim(a, b[:, :-1])


def test_raw_pointers_through_the_c_abi(ev, vec):
    cabi = importlib.import_module(PKG + ".c_abi")
    V, H, W = 2, 37, 53
    final, rgb, targets = raw_inputs(V, H, W, seed=9)
    s, m = torch.ops.egr.eval_ssim(final, rgb, *targets)
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device="cuda")
    s_r, m_r = f64(V, 3, 3, 2), f64(V, 3, 2)
    assert cabi.ssim_workspace_bytes(V, H, W) == V * 4 * 144
    ws = f64(cabi.ssim_workspace_bytes(V, H, W) // 8)
    dev, stream = torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream
    cabi.eval_ssim(V, H, W, final.data_ptr(), rgb.data_ptr(), targets[0].data_ptr(), targets[1].data_ptr(), targets[2].data_ptr(), s_r.data_ptr(), m_r.data_ptr(), ws.data_ptr(),
                   device=dev, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(s_r.nan_to_num(-2.0), s.nan_to_num(-2.0)) and torch.equal(m_r.nan_to_num(-2.0), m.nan_to_num(-2.0))
    a, b = torch.tensor(vec["random_45x70_a"]).cuda()[None].contiguous(), torch.tensor(vec["random_45x70_b"]).cuda()[None].contiguous()
    s_i, m_i = torch.ops.egr.ssim_images(a, b)
    s_q, m_q = f64(1, 3, 2), f64(1, 2)
    ws = f64(cabi.ssim_workspace_bytes(1, 45, 70) // 8)
    cabi.ssim_images(1, 45, 70, a.data_ptr(), b.data_ptr(), s_q.data_ptr(), m_q.data_ptr(), ws.data_ptr(), device=dev, stream=stream)
    torch.cuda.synchronize()
    assert torch.equal(s_q, s_i) and torch.equal(m_q, m_i)
    with pytest.raises(RuntimeError, match="workspace"):
        cabi.ssim_images(1, 45, 70, a.data_ptr(), b.data_ptr(), s_q.data_ptr(), m_q.data_ptr(), None)
