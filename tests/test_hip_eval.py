"""Evaluation on the GPU: the batched denoise (egr_denoise_views / Raytracer.denoise_views) bit for bit against denoise(), the fused metrics
(csrc/eval.hip; torch.ops.egr.eval_metrics) against the stock-torch restatement of tests/eval_restatement.py, and evaluation.evaluate_views against the loop it
replaces. Team help is off (conftest.py), so launches are reproducible bit for bit.

Bars, by the suite's convention (test_hip_edit.py), are MEASURED in the same run from the fp32 torch restatement on the device, both sides against the fp64 restatement:
  display   max-abs err(kernel) <= 4 * err(fp32 restatement) + 4 * 2^-23 (values lie in [0, 1]); NaN positions identical
  sse       against the fp64 sum over the kernel's own display: relative n * 2^-53 * 4, n = pixels (the fp64 summation order is the only freedom)
  psnr      err(kernel) <= 4 * err(fp32 restatement) + 4 * 2^-23 * 4.35 dB (a relative mse error of 4 ulps)
Measured on an MI355X: DESIGN.md 8f-6 has the table."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import eval_restatement as er  # noqa: E402
from hip_common import cam_obj, ren, report, tracer, views  # noqa: E402,F401

pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -23
DW, DH, DV = 37, 19, 3  # the denoise tests' image: both dimensions below the 2 x 16 reach of the last pass, neither a multiple of the 32 x 8 block


@pytest.fixture(scope="module")
def ev(ren):
    mod = importlib.import_module(PKG + ".evaluation")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def small(ren, syn):
    """A 37 x 19 tracer, random final / normal for three views, and what denoise() makes of each view through the framebuffer."""
    rt = tracer(ren, syn, W=DW, H=DH, N=300)
    m = rt.cuda_module
    fb = m.get_framebuffer()
    g = torch.Generator(device="cuda").manual_seed(1)
    final = (2 * torch.rand(DV, DH, DW, 3, device="cuda", generator=g) ** 2).contiguous()
    normal = torch.nn.functional.normalize(torch.randn(DV, 3, DH, DW, 3, device="cuda", generator=g), dim=-1).contiguous()
    ref = []
    for v in range(DV):
        fb.output_final.copy_(final[v][None])
        fb.output_normal.copy_(normal[v])
        m.denoise()
        ref.append(fb.output_denoised[0].clone())
    return rt, final, normal, torch.stack(ref)


def test_denoise_views_is_bit_equal_to_denoise(small):
    rt, final, normal, ref = small
    m = rt.cuda_module
    fb = m.get_framebuffer()
    held = fb.output_denoised.clone()
    bytes_before = m.get_counters()[14]
    out = m.denoise_views(final, normal)
    assert out.shape == (DV, DH, DW, 3) and torch.equal(out, ref), int((out != ref).sum())
    assert float((out - final).abs().max()) > 1e-3  # it filters
    assert torch.equal(m.denoise_views(final, normal[:, 0].contiguous()), ref)  # the packed guide
    assert torch.equal(m.denoise_views(final[1:2].contiguous(), normal[1:2].contiguous())[0], ref[1])  # a view does not depend on its neighbours
    assert torch.equal(fb.output_denoised, held)  # the framebuffer is not touched
    assert m.get_counters()[14] == bytes_before + DV * DH * DW * 3 * 4  # one temporary per view, counted, grown once
    with pytest.raises(RuntimeError, match="normal must be"):
        m.denoise_views(final, normal[:2].contiguous())


def test_denoise_views_copies_under_EGR_DENOISE_0(ren):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "eval_denoise_copy_worker.py")], cwd=ROOT, env=dict(os.environ, EGR_DENOISE="0"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert info == {"copy": True, "shape": [DV, DH, DW, 3]}, info


def make_inputs(V, H, W, seed):
    """HDR predictions and targets that are a noisy copy of them (20-40 dB after the tone curve)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
    final = (3 * rnd(V, H, W, 3) ** 2).contiguous()
    rgb = (2 * rnd(V, 3, H, W, 3) ** 2).contiguous()
    noisy = lambda t: (t * (1 + 0.17 * torch.randn(t.shape, device="cuda", generator=g))).abs().contiguous()
    targets = [noisy(p) for p in er.predictions(final, rgb)]
    return final, rgb, targets


def own_sse(disp):
    return ((disp[:, :, 0].double() - disp[:, :, 1].double()) ** 2).flatten(-2).sum(-1)  # [V,3,3]


def check_against_restatement(name, final, rgb, targets, sse, psnr, disp):
    """The three bars of the module docstring; returns the measured figures. NaN entries must be NaN on both sides and are left out of the maxima."""
    V, H, W, _ = final.shape
    d32, _, p32 = er.metrics(final, rgb, targets, torch.float32)
    d64, _, p64 = er.metrics(final, rgb, targets, torch.float64)
    assert torch.equal(torch.isnan(disp), torch.isnan(d64)) and torch.equal(torch.isnan(d32), torch.isnan(d64)), name
    err = lambda a: float((a.double() - d64).abs().nan_to_num(0.0).max())
    e_k, e_r = err(disp), err(d32)
    own = own_sse(disp)
    assert torch.equal(torch.isnan(sse), torch.isnan(own)), (name, sse, own)
    rel = float(((sse - own).abs() / own.clamp_min(1e-300)).nan_to_num(0.0).max())
    assert torch.equal(torch.isnan(psnr), torch.isnan(p64)), (name, psnr, p64)
    fin = torch.isfinite(p64)
    assert torch.equal(psnr[~fin & ~torch.isnan(p64)], p64[~fin & ~torch.isnan(p64)])  # +inf stays +inf
    perr = lambda a: float((a.double() - p64)[fin].abs().max()) if bool(fin.any()) else 0.0
    p_k, p_r = perr(psnr), perr(p32)
    report(name, display_err_kernel=f"{e_k:.2e}", display_err_fp32_torch=f"{e_r:.2e}", sse_rel_vs_own_display=f"{rel:.2e}", psnr_err_kernel_dB=f"{p_k:.2e}",
           psnr_err_fp32_torch_dB=f"{p_r:.2e}", psnr_range=(f"{float(p64[fin].min()):.1f}..{float(p64[fin].max()):.1f}" if bool(fin.any()) else "-"))
    assert e_k <= 4 * e_r + 4 * ULP, (name, e_k, e_r)
    assert rel <= H * W * 2.0 ** -53 * 4, (name, rel)
    assert p_k <= 4 * p_r + 4 * ULP * 4.35, (name, p_k, p_r)
    return p64


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (19, 37), (96, 160)])
def test_eval_metrics_against_the_restatement(ev, H, W, V):
    final, rgb, targets = make_inputs(V, H, W, seed=100 + H + V)
    sse, psnr, disp = torch.ops.egr.eval_metrics(final, rgb, *targets, True)
    assert sse.shape == (V, 3, 3) and psnr.shape == (V, 3, 2) and disp.shape == (V, 3, 2, 3, H, W) and sse.dtype == psnr.dtype == torch.float64
    p64 = check_against_restatement(f"eval_metrics_{H}x{W}_V{V}", final, rgb, targets, sse, psnr, disp)
    assert bool(torch.isfinite(psnr).all()) and (H * W == 1 or (15.0 < float(p64.min()) and float(p64.max()) < 45.0))
    sse2, psnr2, none = torch.ops.egr.eval_metrics(final, rgb, *targets, False)  # the same inputs again, without the display images
    assert torch.equal(sse2, sse) and torch.equal(psnr2, psnr) and none.numel() == 0


def test_edge_values_through_the_op(ev):
    H, W = 19, 37
    final, rgb, targets = make_inputs(1, H, W, seed=5)
    final[0, 3, 4, 0], final[0, 7, 30, 1], final[0, 18, 36, 2] = float("nan"), float("inf"), 3e38
    targets[1][0, 1, 9, 11] = -0.01
    sse, psnr, disp = torch.ops.egr.eval_metrics(final, rgb, *targets, True)
    d32 = er.metrics(final, rgb, targets, torch.float32)[0]
    assert float(disp[0, 0, 0, 0, 3, 4]) == 0.0 and float(disp[0, 0, 0, 1, 7, 30]) == 1.0  # NaN -> 0, +inf -> 1
    assert bool(torch.isnan(disp[0, 0, 0, 2, 18, 36])) and bool(torch.isnan(disp[0, 1, 1, 1, 9, 11])) and int(torch.isnan(disp).sum()) == 2  # 3e38, -0.01 -> NaN; no others
    assert torch.equal(torch.isnan(disp), torch.isnan(d32))  # (the values: check_against_restatement below)
    # exactly the (pass, channel) sums that hold a NaN pixel are NaN
    want_nan = torch.zeros(1, 3, 3, dtype=torch.bool, device="cuda")
    want_nan[0, 0, 2] = want_nan[0, 1, 1] = True
    assert torch.equal(torch.isnan(sse), want_nan), sse
    assert bool(torch.isnan(psnr[0, :2]).all()) and bool(torch.isfinite(psnr[0, 2]).all())
    check_against_restatement("eval_metrics_edge_values", final, rgb, targets, sse, psnr, disp)
    # a NULL target: that pass reports NaN, the others are unaffected
    sse_n, psnr_n, disp_n = torch.ops.egr.eval_metrics(final, rgb, targets[0], targets[1], None, True)
    assert bool(torch.isnan(sse_n[0, 2]).all()) and bool(torch.isnan(psnr_n[0, 2]).all()) and bool(torch.isnan(disp_n[0, 2]).all())
    assert torch.equal(sse_n[0, :2].nan_to_num(-1.0), sse[0, :2].nan_to_num(-1.0)) and torch.equal(disp_n[0, :2].nan_to_num(-1.0), disp[0, :2].nan_to_num(-1.0))
    sse_f, psnr_f, _ = torch.ops.egr.eval_metrics(final, None, targets[0], None, None, False)  # final alone needs no rgb
    assert torch.equal(sse_f[0, 0].nan_to_num(-1.0), sse[0, 0].nan_to_num(-1.0)) and bool(torch.isnan(psnr_f[0, 1:]).all())
    # identical prediction and target: mse 0, +inf in both flavours
    clean, rgb2, _ = make_inputs(1, H, W, seed=6)
    same = [p.clone() for p in er.predictions(clean, rgb2)]
    sse_s, psnr_s, _ = torch.ops.egr.eval_metrics(clean, rgb2, *same, False)
    assert float(sse_s.abs().max()) == 0.0 and bool((psnr_s == float("inf")).all())


def sequential_evaluation(ren, ev, rt, cams, spp, base, denoise=True):
    """The loop evaluate_views replaces (train.py:103-134 / render.py:195-228) on the single-frame API: per camera reset_accumulators, spp renders with
    accumulate_samples, denoise(), torch tonemap / clamp / psnr. Returns per view the images it compared and its three PSNRs (fp32 .mean().double())."""
    m = rt.cuda_module
    fb = m.get_framebuffer()
    m.get_metadata().total_num_calls.fill_(base)
    m.get_config().accumulate_samples.fill_(True)
    out = []
    try:
        for c in cams:
            m.reset_accumulators()
            with torch.no_grad():
                for _ in range(spp):
                    package = ren.render(c, rt, targets_available=False)
                if denoise:
                    m.denoise()
                    package.final = fb.output_denoised.clone().moveaxis(-1, 1)
            preds = [package.final[0], package.rgb[0], package.rgb[1:].sum(dim=0)]
            gts = [c.original_image, c.diffuse_image, c.specular_image]
            out.append(dict(preds=preds, plain_final=fb.output_final.clone().moveaxis(-1, 1)[0],
                            psnr=[ev.psnr(ev.display(p), ev.display(t)).mean().double() for p, t in zip(preds, gts)]))
    finally:
        m.get_config().accumulate_samples.fill_(False)
    return out


def test_evaluate_views_equals_the_loop_it_replaces(ren, ev, syn):
    W, H, V, S, base = 160, 96, 3, 4, 20
    torch.manual_seed(7)  # (random_seeds of a new tracer: the same jitter on every run)
    rt = tracer(ren, syn, W=W, H=H, N=2000, seed=7)  # the 2k room
    m = rt.cuda_module
    m.get_config().jitter_primary_rays.fill_(True)
    tg = syn.make_targets(W, H)
    cams = [cam_obj(ren, c, tg) for c in views(syn, V)]
    for i, c in enumerate(cams):  # every view its own ground truth; original = diffuse + specular
        c.diffuse_image = (c.diffuse_image * (1.0 + 0.1 * i)).contiguous()
        c.original_image = (c.diffuse_image + c.specular_image).contiguous()
    loop = sequential_evaluation(ren, ev, rt, cams, S, base)
    fb = m.get_framebuffer()
    held = {k: getattr(fb, k).clone() for k in ("output_final", "output_denoised", "output_rgb", "accumulated_rgb", "accumulated_sample_count")}
    m.get_metadata().total_num_calls.fill_(base)
    res = ev.evaluate_views(cams, rt, spp=S, denoise=True, views_per_call=8, keep_images=True)
    assert int(m.get_metadata().total_num_calls) == base + V * S == 32
    for k, t in held.items():
        assert torch.equal(getattr(fb, k), t), k  # the framebuffer is not touched
    assert sorted(res.psnr) == sorted(res.psnr_global) == sorted(res.mean) == ["diffuse", "final", "specular"] and len(res.images) == V
    for v in range(V):
        for k, name in enumerate(ev.PASSES):
            pred, gt = loop[v]["preds"][k].contiguous(), getattr(cams[v], ev.PASS_TARGETS[k])
            for got, src in ((getattr(res.images[v], name), pred), (getattr(res.images[v], name + "_gt"), gt)):
                d64, d32 = er.display(src, torch.float64), er.display(src, torch.float32)
                e_k, e_r = float((got.double() - d64).abs().max()), float((d32.double() - d64).abs().max())
                assert got.shape == (3, H, W) and e_k <= 4 * e_r + 4 * ULP, (v, name, e_k, e_r)
            pair = (pred.movedim(0, -1)[None].contiguous(), None, [gt[None], None, None])  # (pass 0 of the restatement on this pair)
            p64, p32 = er.metrics(*pair, torch.float64)[2][0, 0].cpu(), er.metrics(*pair, torch.float32)[2][0, 0].cpu()
            assert abs(float(loop[v]["psnr"][k]) - float(p32[0])) < 1e-4  # the loop's own number is the fp32 restatement's
            p_r, p_r_global = abs(float(p32[0]) - float(p64[0])), abs(float(p32[1]) - float(p64[1]))
            p_k = abs(float(res.psnr[name][v]) - float(p64[0]))
            report(f"evaluate_views_v{v}_{name}", psnr=f"{float(res.psnr[name][v]):.3f}", psnr_global=f"{float(res.psnr_global[name][v]):.3f}", loop=f"{float(loop[v]['psnr'][k]):.3f}",
                   err_kernel_dB=f"{p_k:.2e}", err_loop_fp32_dB=f"{p_r:.2e}")
            assert p_k <= 4 * p_r + 4 * ULP * 4.35, (v, name, p_k, p_r)
            assert abs(float(res.psnr_global[name][v]) - float(p64[1])) <= 4 * p_r_global + 4 * ULP * 4.35
            assert 5.0 < float(res.psnr[name][v]) < 60.0
    for name in ev.PASSES:
        assert res.psnr[name].dtype == torch.float64 and not res.psnr[name].is_cuda and res.mean[name] == float(res.psnr[name].mean())
    # a chunk boundary inside V = 3 changes nothing
    m.get_metadata().total_num_calls.fill_(base)
    res2 = ev.evaluate_views(cams, rt, spp=S, denoise=True, views_per_call=2)
    assert res2.images is None and int(m.get_metadata().total_num_calls) == base + V * S
    for name in ev.PASSES:
        assert torch.equal(res2.psnr[name], res.psnr[name]) and torch.equal(res2.psnr_global[name], res.psnr_global[name]) and torch.equal(res2.sse[name], res.sse[name])
    # denoise = False scores the plain final image
    m.get_metadata().total_num_calls.fill_(base)
    res3 = ev.evaluate_views(cams, rt, spp=S, denoise=False, keep_images=True)
    for v in range(V):
        src = loop[v]["plain_final"].contiguous()
        d64, d32 = er.display(src, torch.float64), er.display(src, torch.float32)
        e_k, e_r = float((res3.images[v].final.double() - d64).abs().max()), float((d32.double() - d64).abs().max())
        assert e_k <= 4 * e_r + 4 * ULP, (v, e_k, e_r)
        assert not torch.equal(res3.images[v].final, res.images[v].final) and torch.equal(res3.images[v].diffuse, res.images[v].diffuse)
    assert torch.equal(res3.psnr["diffuse"], res.psnr["diffuse"]) and not torch.equal(res3.psnr["final"], res.psnr["final"])
    # a camera without one of the images: that pass is absent for the whole call
    del cams[1].specular_image
    m.get_metadata().total_num_calls.fill_(base)
    res4 = ev.evaluate_views(cams, rt, spp=S, denoise=True)
    assert bool(torch.isnan(res4.psnr["specular"]).all()) and torch.equal(res4.psnr["final"], res.psnr["final"]) and torch.equal(res4.psnr["diffuse"], res.psnr["diffuse"])


def test_raw_pointers_through_the_c_abi(small, ev):
    """egr_denoise_views and egr_eval_metrics on raw device addresses through c_abi.py (torch is nothing but the allocator): the results of the shim bit for bit,
    and egr_denoise_views' refusals - on a real context, with fake pointers that a refused call never touches."""
    cabi = importlib.import_module(PKG + ".c_abi")
    rt, final, normal, ref = small
    L = cabi.lib()
    ctx = C.c_void_p()
    assert L.egr_create(C.byref(ctx), torch.cuda.current_device(), DW, DH, 1000, 1000) == 0
    try:
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        n = DH * DW * 3
        A, B, D = 0x10000000, 0x20000000, 0x30000000
        err = lambda: L.egr_last_error(ctx).decode()
        assert L.egr_denoise_views(ctx, 0, A, B, n, D, stream) != 0 and "num_views" in err()
        assert L.egr_denoise_views(ctx, 2, None, B, n, D, stream) != 0 and "non-NULL" in err()
        assert L.egr_denoise_views(ctx, 2, A, None, n, D, stream) != 0 and L.egr_denoise_views(ctx, 2, A, B, n, None, stream) != 0
        assert L.egr_denoise_views(ctx, 2, A, B, n, A + 2 * n * 4 - 4, stream) != 0 and "final and denoised overlap" in err()  # denoised starts in final's last word
        assert L.egr_denoise_views(ctx, 2, A, B, n, A, stream) != 0 and "overlap" in err()
        assert L.egr_denoise_views(ctx, 2, A, B, n - 1, D, stream) != 0 and "stride" in err()
        assert L.egr_denoise_views(ctx, 2, A, B, 3 * n, B + 4 * n * 4 - 4, stream) != 0 and "normal and denoised overlap" in err()
        out = torch.empty_like(final)
        assert L.egr_denoise_views(ctx, DV, final.data_ptr(), normal.data_ptr(), 3 * n, out.data_ptr(), stream) == 0, err()
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    finally:
        L.egr_destroy(ctx)
    H, W, V = 19, 37, 3
    fin, rgb, targets = make_inputs(V, H, W, seed=9)
    sse, psnr, disp = torch.ops.egr.eval_metrics(fin, rgb, *targets, True)
    f64 = lambda *s: torch.empty(*s, dtype=torch.float64, device="cuda")
    sse_r, psnr_r, disp_r = f64(V, 3, 3), f64(V, 3, 2), torch.empty_like(disp)
    assert cabi.eval_workspace_bytes(V, H, W) == V * 1 * 72
    ws = torch.empty(cabi.eval_workspace_bytes(V, H, W) // 8, dtype=torch.float64, device="cuda")
    cabi.eval_metrics(V, H, W, fin.data_ptr(), rgb.data_ptr(), targets[0].data_ptr(), targets[1].data_ptr(), targets[2].data_ptr(), sse_r.data_ptr(), psnr_r.data_ptr(),
                      ws.data_ptr(), display=disp_r.data_ptr(), device=torch.cuda.current_device(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert torch.equal(sse_r, sse) and torch.equal(psnr_r, psnr) and torch.equal(disp_r, disp)
    with pytest.raises(RuntimeError, match="workspace"):
        cabi.eval_metrics(V, H, W, fin.data_ptr(), rgb.data_ptr(), None, None, None, sse_r.data_ptr(), psnr_r.data_ptr(), None)
