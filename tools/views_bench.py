"""Batched (renderer.render_views / egr_render_views) against sequential no-grad rendering at 1920x1080 on the synthetic scenes of BASELINE
configs B (100k dense-init) and C (1M, dense-init and trained-like), for two workloads: V=8 views x S=1 sample (measure_fps.py's shape) and
V=1 view x S=16 samples (render.py's accumulated samples). Prints Mrays/s (rays of all bounce steps, from the launch counters), ms per frame,
the ratio, and the per-kernel times (egr_last_kernel_ms) of one run of each path.
Usage: python tools/views_bench.py [--reps 5] [--configs B,C-init,C-trained] [--batch-frames 8]"""
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

CONFIGS = {"B": (100_000, "init"), "C-init": (1_000_000, "init"), "C-trained": (1_000_000, "trained")}
W, H = 1920, 1080


def cameras(n):
    """The bench camera, then moved and turned a little (an orbit segment of a test set)."""
    base = syn.default_camera()
    out = []
    for i in range(n):
        eye = base["origin"].astype(np.float64) + np.array([0.06 * i, -0.04 * i, 0.02 * i])
        c2w = syn.look_at(eye, (1.2 - 0.05 * i, 0.5 + 0.03 * i, -0.9)).astype(np.float32)
        out.append(ren.camera_from_c2w(eye.astype(np.float32), c2w, base["fov"]))
    return out


def sequential(rt, cams, S):
    m = rt.cuda_module
    m.get_config().accumulate_samples.fill_(S > 1)
    with torch.no_grad():
        for c in cams:
            m.reset_accumulators()
            for _ in range(S):
                ren.render(c, rt, targets_available=False)
    m.get_config().accumulate_samples.fill_(False)


def batched(rt, cams, S):
    ren.render_views(cams, rt, spp=S)


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def kernel_ms(m):
    acc = {}
    for name, ms in m.last_kernel_ms():
        acc[name] = acc.get(name, 0.0) + ms
    return {k: round(v, 3) for k, v in acc.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--configs", default="B,C-init,C-trained")
    p.add_argument("--batch-frames", type=int, default=8)
    a = p.parse_args()
    assert torch.cuda.is_available(), "views_bench.py needs a GPU"
    for cfg in a.configs.split(","):
        N, variant = CONFIGS[cfg]
        rt = ren.GaussianRaytracer(ren.GaussianParams(syn.make_scene(N, variant, seed=0)), W, H, ppll_forward_size=400_000_000, ppll_backward_size=1_000_000)
        m = rt.cuda_module
        m.set_batch_frames(a.batch_frames)
        for V, S in ((8, 1), (1, 16)):
            cams = cameras(V)
            frames = V * S
            res = {}
            for label, fn in (("sequential", lambda: sequential(rt, cams, S)), ("batched", lambda: batched(rt, cams, S))):
                fn()  # warm-up (the first batch call allocates the ray state of its chunk)
                m.reset_lifetime_counters()
                fn()
                torch.cuda.synchronize()
                c = m.get_counters()
                rays = int(c[9])  # lifetime rays: every step of every frame of the run
                assert c[10] == frames and c[11] == 0, (label, c[10], c[11])
                ms = timed(fn, a.reps)
                m.enable_timing(True)
                fn()
                torch.cuda.synchronize()
                kms = kernel_ms(m)  # sequential: the last launch; batched: the whole batch
                m.enable_timing(False)
                res[label] = (ms, rays)
                print(f"{cfg:9s} V={V} S={S:2d} {label:10s} {ms / frames:7.3f} ms/frame  {rays / (ms * 1e-3) / 1e6:7.1f} Mrays/s  kernels {kms}", flush=True)
            ratio = res["sequential"][0] / res["batched"][0]
            print(f"{cfg:9s} V={V} S={S:2d} batched / sequential speed: {ratio:.3f}x", flush=True)
        del rt, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
