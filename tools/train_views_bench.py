"""Multi-view training (renderer.train_views / egr_train_views) against sequential grad launches at 1920x1080 on the synthetic scenes of BASELINE
config C (1M, dense-init and trained-like): V x (update_bvh + grad raytrace) one camera at a time, against ONE train_views call for the V cameras
(which refits once: every view shares the parameters). Runs of the two paths are interleaved; each row is the median of --reps runs. Prints ms per
view, Mrays/s (rays of all bounce steps, from the launch counters), forward and backward chain ms per view (egr_last_kernel_ms of one extra run;
sequential: the last launch's), and the speed ratio.
Usage: python tools/train_views_bench.py [--reps 5] [--configs C-init,C-trained] [--views 1,4,8] [--batch-frames 8]"""
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

CONFIGS = {"C-init": (1_000_000, "init"), "C-trained": (1_000_000, "trained")}
W, H = 1920, 1080


def cameras(n, targets):
    """The bench camera, then moved and turned a little (views of a training set), each with the six target images (CHW)."""
    base = syn.default_camera()
    out = []
    for i in range(n):
        eye = base["origin"].astype(np.float64) + np.array([0.06 * i, -0.04 * i, 0.02 * i])
        c2w = syn.look_at(eye, (1.2 - 0.05 * i, 0.5 + 0.03 * i, -0.9)).astype(np.float32)
        out.append(ren.camera_from_c2w(eye.astype(np.float32), c2w, base["fov"], **targets))
    return out


def sequential(rt, cams):
    for c in cams:  # the reference's loop: render() with grad mode on = export, targets, update_bvh, grad raytrace, import
        ren.render(c, rt)


def batched(rt, cams):
    ren.train_views(cams, rt)


def kernel_ms(m):
    acc = {}
    for name, ms in m.last_kernel_ms():
        acc[name] = acc.get(name, 0.0) + ms
    return acc


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--configs", default="C-init,C-trained")
    p.add_argument("--views", default="1,4,8")
    p.add_argument("--batch-frames", type=int, default=8)
    a = p.parse_args()
    assert torch.cuda.is_available(), "train_views_bench.py needs a GPU"
    tg = {k + "_image": torch.tensor(v).cuda().moveaxis(-1, 0).contiguous() for k, v in syn.make_targets(W, H).items()}
    for cfg in a.configs.split(","):
        N, variant = CONFIGS[cfg]
        rt = ren.GaussianRaytracer(ren.GaussianParams(syn.make_scene(N, variant, seed=0)), W, H, ppll_forward_size=400_000_000, ppll_backward_size=300_000_000)
        m = rt.cuda_module
        m.set_batch_frames(a.batch_frames)
        for V in (int(x) for x in a.views.split(",")):
            cams = cameras(V, tg)
            paths = (("sequential", lambda: sequential(rt, cams)), ("train_views", lambda: batched(rt, cams)))
            rays, chains = {}, {}
            for label, fn in paths:
                rt.zero_grad()
                fn()  # warm-up (the first batch call allocates the ray state and arena of its chunk)
                m.reset_lifetime_counters()
                fn()
                torch.cuda.synchronize()
                c = m.get_counters()
                rays[label] = int(c[9])  # lifetime rays: every step of every view of the run
                assert c[10] == V and c[11] == 0, (label, c[10], c[11])
                m.enable_timing(True)
                fn()
                torch.cuda.synchronize()
                k = kernel_ms(m)  # sequential: the last launch (x V below); train_views: the whole call
                m.enable_timing(False)
                scale = 1.0 if label == "sequential" else 1.0 / V
                chains[label] = (k.get("forward_chain", 0.0) * scale, k.get("backward_chain", 0.0) * scale)
            ts = {label: [] for label, _ in paths}
            for _ in range(a.reps):  # interleaved: drifts of clock and temperature hit both paths alike
                for label, fn in paths:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts[label].append(time.perf_counter() - t0)
            ms = {label: float(np.median(v)) * 1e3 for label, v in ts.items()}
            for label, _ in paths:
                print(f"{cfg:9s} V={V} {label:11s} {ms[label] / V:7.3f} ms/view  {rays[label] / (ms[label] * 1e-3) / 1e6:7.1f} Mrays/s  "
                      f"forward chain {chains[label][0]:6.3f} ms/view  backward chain {chains[label][1]:6.3f} ms/view", flush=True)
            print(f"{cfg:9s} V={V} train_views / sequential speed per view: {ms['sequential'] / ms['train_views']:.3f}x", flush=True)
        del rt, m
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
