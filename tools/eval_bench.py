"""evaluation.evaluate_views against the sequential evaluation loop it replaces (per camera: reset_accumulators, spp renders, denoise(), torch tonemap / clamp /
psnr of the three passes on the device, one host read-back after the last view) at 1920x1080, V = 8 cameras, on the synthetic scenes of BASELINE configs B (100k) and C trained-like (1M), for
spp = 1 (training_report's case) and spp = 16 (render.py's). The two paths are checked equal first, then timed interleaved in one process (median of --reps, every
timed region between device synchronisations). Prints ms per view for both paths, the share of it that is rendering, launches per view (torch's profiler, in a
pass of its own) and, for the fused metrics alone, GB/s over their 84 B per pixel and view.
Usage: python tools/eval_bench.py [--reps 5] [--configs B,C-trained] [--spp 1,16] [--views 8]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
syn = importlib.import_module("editable-gaussian-reflections_amd.synthetic")
ren = importlib.import_module("editable-gaussian-reflections_amd.renderer")
ev = importlib.import_module("editable-gaussian-reflections_amd.evaluation")

CONFIGS = {"B": (100_000, "init"), "C-trained": (1_000_000, "trained")}
W, H = 1920, 1080


def cameras(n):
    """The bench camera, then moved and turned a little, each with ground-truth images of its own."""
    base = syn.default_camera()
    tg = syn.make_targets(W, H)
    chw = lambda a: torch.tensor(a).cuda().moveaxis(-1, 0).contiguous()
    out = []
    for i in range(n):
        eye = base["origin"].astype(np.float64) + np.array([0.06 * i, -0.04 * i, 0.02 * i])
        c2w = syn.look_at(eye, (1.2 - 0.05 * i, 0.5 + 0.03 * i, -0.9)).astype(np.float32)
        d, s = chw(tg["diffuse"]) * (1.0 + 0.05 * i), chw(tg["specular"])
        out.append(ren.camera_from_c2w(eye.astype(np.float32), c2w, base["fov"], diffuse_image=d, specular_image=s, original_image=d + s))
    return out


def sequential(rt, cams, S, metrics=True):
    """The loop evaluate_views replaces, on the single-frame API. The per-pass PSNRs stay on the device (train.py:131-133 keeps running sums as tensors) and are read
    back once after the last view. Returns the [V,3] PSNRs on the host."""
    m = rt.cuda_module
    fb = m.get_framebuffer()
    m.get_config().accumulate_samples.fill_(S > 1)
    rows = []
    with torch.no_grad():
        for c in cams:
            m.reset_accumulators()
            for _ in range(S):
                package = ren.render(c, rt, targets_available=False)
            m.denoise()
            if not metrics:
                continue
            package.final = fb.output_denoised.clone().detach().moveaxis(-1, 1)
            preds = (package.final[0], package.rgb[0], package.rgb[1:].sum(dim=0))
            gts = (c.original_image, c.diffuse_image, c.specular_image)
            rows.append(torch.stack([ev.psnr(ev.display(p), ev.display(t)).mean().double() for p, t in zip(preds, gts)]))
    m.get_config().accumulate_samples.fill_(False)
    return torch.stack(rows).cpu() if rows else torch.zeros((0, 3), dtype=torch.float64)  # the one read-back


def fused(rt, cams, S):
    res = ev.evaluate_views(cams, rt, spp=S, denoise=True, views_per_call=len(cams))
    return torch.stack([res.psnr[k] for k in ev.PASSES], dim=1)


def render_only(rt, cams, S):
    ren.render_views_raw(cams, rt, spp=S, outputs=("final", "rgb", "normal"))


def interleaved(fns, reps):
    """Median ms of each function, the functions taking turns."""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e3)
    return [float(np.median(t)) for t in ts]


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def metrics_alone(V, reps):
    g = torch.Generator(device="cuda").manual_seed(0)
    final = torch.rand(V, H, W, 3, device="cuda", generator=g)
    rgb = torch.rand(V, 3, H, W, 3, device="cuda", generator=g)
    tg = [torch.rand(V, 3, H, W, device="cuda", generator=g) for _ in range(3)]
    out = {}
    for label, disp in (("no display, 84 B/px", False), ("with display, 156 B/px", True)):
        fn = lambda: torch.ops.egr.eval_metrics(final, rgb, *tg, disp)
        fn()
        ms = interleaved([fn], max(reps, 9))[0]
        out[label] = (ms, V * H * W * (156 if disp else 84) / (ms * 1e-3) / 1e9)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--configs", default="B,C-trained")
    p.add_argument("--spp", default="1,16")
    p.add_argument("--views", type=int, default=8)
    a = p.parse_args()
    assert torch.cuda.is_available(), "eval_bench.py needs a GPU"
    V = a.views
    ev.load_library()
    for label, (ms, gbs) in metrics_alone(V, a.reps).items():
        print(f"eval_metrics alone V={V} {W}x{H} ({label}): {ms:.3f} ms = {ms / V:.3f} ms/view, {gbs:.0f} GB/s (float4 copy: 6290 GB/s)", flush=True)
    for cfg in a.configs.split(","):
        N, variant = CONFIGS[cfg]
        rt = ren.GaussianRaytracer(ren.GaussianParams(syn.make_scene(N, variant, seed=0)), W, H, ppll_forward_size=400_000_000, ppll_backward_size=1_000_000)
        m = rt.cuda_module
        m.set_batch_frames(8)
        cams = cameras(V)
        for S in [int(s) for s in a.spp.split(",")]:
            base = int(m.get_metadata().total_num_calls)
            seq = sequential(rt, cams, S)  # (also the warm-up)
            m.get_metadata().total_num_calls.fill_(base)
            fus = fused(rt, cams, S)
            worst = float((seq - fus).abs().max())
            assert worst < 1e-3, (cfg, S, seq, fus)  # team help is on here: exact depth ties may composite in another order; the loop's PSNR is fp32
            t_seq, t_fus, t_render, t_seq_render = interleaved([lambda: sequential(rt, cams, S), lambda: fused(rt, cams, S), lambda: render_only(rt, cams, S),
                                                                lambda: sequential(rt, cams, S, metrics=False)], a.reps)
            n_seq, n_fus = launches(lambda: sequential(rt, cams, S)), launches(lambda: fused(rt, cams, S))
            print(f"{cfg:9s} V={V} spp={S:2d} sequential {t_seq / V:8.3f} ms/view (render+denoise {t_seq_render / V:8.3f}, {n_seq / V:6.1f} launches/view) | evaluate_views "
                  f"{t_fus / V:8.3f} ms/view (render {t_render / V:8.3f} = {100 * t_render / t_fus:4.1f} %, {n_fus / V:6.1f} launches/view) | {t_seq / t_fus:.2f}x | "
                  f"PSNR final {float(fus[:, 0].mean()):.2f} dB, max |loop - fused| {worst:.1e} dB", flush=True)
        del rt, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
