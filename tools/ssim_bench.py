"""The fused SSIM (csrc/ssim.hip) against the stock-torch sequence it replaces, at 1920x1080 with V = 8 views:
  1. the launch pair alone (torch.ops.egr.eval_ssim on random final / rgb / targets), ms per view and the model's rates (0.17 GB read, 2.4 G fp64 multiply-adds per view);
  2. the torch sequence on the same device: display() of both sides of the three passes, then the reference's five depthwise 11 x 11 conv2d per pass in fp32
     (utils/loss_utils.py:50-65 restated with torch ops), per view, as the reference's loop would run it - and the number of launches it makes;
  3. evaluation.evaluate_views with and without ssim=True on the 100k cloud (BASELINE config B), spp 1.
Every figure is the median of --reps runs after a warm-up, timed with device events on the current stream; the candidates take turns.
Usage: python tools/ssim_bench.py [--reps 9] [--views 8] [--no-scene]"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
syn = importlib.import_module("editable-gaussian-reflections_amd.synthetic")
ren = importlib.import_module("editable-gaussian-reflections_amd.renderer")
ev = importlib.import_module("editable-gaussian-reflections_amd.evaluation")

W, H = 1920, 1080


def window(device):
    g = torch.tensor([np.exp(-((x - 5) ** 2) / (2 * 1.5**2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).expand(3, 1, 11, 11).contiguous().to(device)


def torch_ssim(a, b, win):
    """loss_utils._ssim on [1,3,H,W] fp32 images."""
    conv = lambda x: F.conv2d(x, win, padding=5, groups=3)
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1.pow(2), conv(b * b) - mu2.pow(2), conv(a * b) - mu1 * mu2
    return (((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1.pow(2) + mu2.pow(2) + 1e-4) * (s1 + s2 + 9e-4))).mean()


def torch_sequence(final, rgb, targets, win):
    """Per view and pass: display() of prediction and target, the reference's ssim. The numbers stay on the device."""
    rows = []
    for v in range(final.shape[0]):
        preds = (final[v].movedim(-1, 0), rgb[v, 0].movedim(-1, 0), rgb[v, 1:].sum(0).movedim(-1, 0))
        rows.append(torch.stack([torch_ssim(ev.display(p)[None], ev.display(t[v])[None], win) for p, t in zip(preds, targets)]))
    return torch.stack(rows)


def timed(fns, reps):
    """Median ms of each function between two device events, the functions taking turns, after one warm-up each."""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            fn()
            stop.record()
            torch.cuda.synchronize()
            ts[i].append(start.elapsed_time(stop))
    return [float(np.median(t)) for t in ts], [(float(np.min(t)), float(np.max(t))) for t in ts]


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=9)
    p.add_argument("--views", type=int, default=8)
    p.add_argument("--no-scene", action="store_true", help="skip part 3 (evaluate_views on the 100k cloud)")
    a = p.parse_args()
    assert torch.cuda.is_available(), "ssim_bench.py needs a GPU"
    V = a.views
    ev.load_library()
    g = torch.Generator(device="cuda").manual_seed(0)
    final = (2 * torch.rand(V, H, W, 3, device="cuda", generator=g) ** 2).contiguous()
    rgb = (torch.rand(V, 3, H, W, 3, device="cuda", generator=g) ** 2).contiguous()
    tg = [(2 * torch.rand(V, 3, H, W, device="cuda", generator=g) ** 2).contiguous() for _ in range(3)]
    win = window("cuda")
    fused = lambda: torch.ops.egr.eval_ssim(final, rgb, *tg)
    stock = lambda: torch_sequence(final, rgb, tg, win)
    worst = float((fused()[1][:, :, 0] - stock().double()).abs().max())
    (t_fused, t_stock), ((lo_f, hi_f), (lo_s, hi_s)) = timed([fused, stock], a.reps)
    n_fused, n_stock = launches(fused), launches(stock)
    per_view = t_fused / V
    print(f"eval_ssim alone V={V} {W}x{H}: {t_fused:.3f} ms [{lo_f:.3f} .. {hi_f:.3f}] = {per_view:.3f} ms/view, {n_fused} launches; model per view: "
          f"{H * W * 84 / 1e9:.3f} GB read = {H * W * 84 / (per_view * 1e-3) / 1e9:.0f} GB/s, 2.4 G fp64 multiply-adds = {2.4e9 * 2 / (per_view * 1e-3) / 1e12:.1f} TFLOP/s", flush=True)
    print(f"torch sequence (6 display chains + 15 conv2d per view, fp32): {t_stock:.3f} ms [{lo_s:.3f} .. {hi_s:.3f}] = {t_stock / V:.3f} ms/view, {n_stock / V:.1f} launches/view | "
          f"{t_stock / t_fused:.2f}x | max |fused fp64 - torch fp32| {worst:.1e}", flush=True)
    if a.no_scene:
        return
    import eval_bench  # the bench cameras with ground truth

    rt = ren.GaussianRaytracer(ren.GaussianParams(syn.make_scene(100_000, "init", seed=0)), W, H, ppll_forward_size=400_000_000, ppll_backward_size=1_000_000)
    rt.cuda_module.set_batch_frames(8)
    cams = eval_bench.cameras(V)
    without = lambda: ev.evaluate_views(cams, rt, spp=1, denoise=True, views_per_call=V)
    with_ssim = lambda: ev.evaluate_views(cams, rt, spp=1, denoise=True, views_per_call=V, ssim=True)
    (t_without, t_with), _ = timed([without, with_ssim], a.reps)
    res = with_ssim()
    print(f"evaluate_views B (100k) V={V} spp=1: {t_without / V:.3f} ms/view without ssim, {t_with / V:.3f} ms/view with it (+{(t_with - t_without) / V:.3f}); {launches(without) / V:.1f} / "
          f"{launches(with_ssim) / V:.1f} launches/view; SSIM final {res.mean_ssim['final']:.4f} diffuse {res.mean_ssim['diffuse']:.4f} specular {res.mean_ssim['specular']:.4f}", flush=True)


if __name__ == "__main__":
    main()
