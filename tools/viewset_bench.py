"""The view store at full size (dataset.ViewSet, csrc/viewset.hip) against the stock torch sequences it replaces. Three measurements, each the median of --reps
timed samples bracketed by device synchronisations, the two sides of a comparison alternating in one process:

  ingest   8 views of 1080 x 1920 sources into a store of 768 x 1365 (resized) and of 1080 x 1920 (as they are), 8-bit sources (depth fp32) and fp32 sources, all
           seven kinds, sources already on the device: torch.ops.egr.viewset_ingest against the same work as stock torch ops on the same device - per image
           interpolate(mode="area") (and .byte()), the expressions of Camera.__init__, moveaxis, .half(), and depth amin / amax. GB/s is over the bytes the
           algorithm must move: every source byte read once, every half written once.
  gather   V = 4 and 8 views of 1080 x 1920 into fp32 batch arrays (six training kinds + camera rows): ViewSet.gather into kept buffers against the stacking
           renderer.train_views does today on cameras that hold fp32 device images (six torch.stack, 2V + 1 small uploads).
  step     one V = 8 training call on a 1M cloud at 1080 x 1920, per view: ViewSet.train against renderer.train_views on cameras with fp32 device images and on
           cameras with fp16 CPU images (upstream's default, IMAGE_HOLDING_DEVICE=cpu).

Device launches of one call are counted with torch's profiler where it works. Writes runs/<tag>/viewset_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/viewset_bench.py [--reps 7] [--views 8] [--parts ingest,gather,step] [--variants trained,init] [--n 1000000] [--tag viewset_bench]"""
import argparse
import importlib
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "editable-gaussian-reflections_amd"
syn = importlib.import_module(PKG + ".synthetic")
ren = importlib.import_module(PKG + ".renderer")
ds = importlib.import_module(PKG + ".dataset")
ev = importlib.import_module(PKG + ".evaluation")


def median_ms(fns, reps, inner=1, warm=2):
    """{label: (median, min, max) ms per call} of the callables `fns`, alternating; every sample is `inner` calls between two device synchronisations."""
    ts = {k: [] for k in fns}
    for rep in range(reps + warm):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            if rep >= warm:
                ts[k].append((time.perf_counter() - t0) * 1e3 / inner)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def launches(fn):
    try:
        from torch.profiler import ProfilerActivity, profile

        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:  # (a torch without a working device profiler: the times stand)
        return repr(e)


def torch_ingest(sources, H, W, resize):
    """What Scene / Camera do per image, on the device: the list of seven half [V,C,H,W] stacks and the depth range [V,2]."""
    out, rng = [], None
    for k, src in enumerate(sources):
        planes = []
        for img in src:  # per view, as the dataset reader and Camera.__init__ see one image at a time
            if resize:
                x = img.permute(2, 0, 1)[None]
                u8 = x.dtype == torch.uint8
                x = torch.nn.functional.interpolate(x.float() if u8 else x, (H, W), mode="area")
                img = (x.byte() if u8 else x)[0].permute(1, 2, 0)
            x = img.moveaxis(-1, 0)
            if x.dtype == torch.uint8:
                if k <= 2:
                    x = ev.untonemap(x.half() / 255.0)
                elif k == 4:
                    x = x.half() / 255.0 * 2.0 - 1.0
                else:
                    x = x.half() / 255.0
            if k in (3, 5):
                x = x[:1]
            planes.append(x.half())
        stack = torch.stack(planes)
        if k == 3:
            rng = torch.stack([stack.float().amin(dim=(1, 2, 3)), stack.float().amax(dim=(1, 2, 3))], dim=1)
        out.append(stack)
    return out, rng


def bench_ingest(a, result):
    V, Hs, Ws = a.views, 1080, 1920
    gen = torch.Generator(device="cuda").manual_seed(0)
    for dtype in ("u8", "f32"):
        sources = []
        for k, c in enumerate(ds.KIND_CHANNELS):
            if dtype == "u8" and k != ds.DEPTH:
                sources.append(torch.randint(0, 255, (V, Hs, Ws, c), dtype=torch.uint8, device="cuda", generator=gen))  # (255 would be inf: kept out of the timing's data)
            else:
                sources.append(torch.rand((V, Hs, Ws, c), device="cuda", generator=gen) * 4.0 + 0.5)
        for resize in (True, False):
            H, W = ds.resized_size(Hs, Ws, 768) if resize else (Hs, Ws)
            vs = ds.ViewSet(H, W, V)
            tables = [vs._tables[ds.TABLE_OF_KIND[k]] if s.dtype == torch.uint8 else None for k, s in enumerate(sources)]
            fused = lambda: torch.ops.egr.viewset_ingest(sources, tables, vs.planes, vs.depth_range, 0)
            stock = lambda: torch_ingest(sources, H, W, resize)
            key = f"ingest_{dtype}_{'resized_768x1365' if resize else 'plain_1080x1920'}"
            # the same values first (the u8 table is defined on the CPU: the device's half pow may differ in the last bit, so only fp32 is compared bit for bit)
            fused()
            ref, rng = stock()
            torch.cuda.synchronize()
            if dtype == "f32":
                worst = max(int((p.view(torch.int16).int() - r.view(torch.int16).int()).abs().max()) for p, r in zip(vs.planes, ref))
                result[key + "_max_half_steps_vs_torch"] = worst
                result[key + "_range_equal"] = bool(torch.equal(vs.depth_range, rng))
            moved = sum(s.numel() * s.element_size() for s in sources) + sum(V * c * H * W * 2 for c in ds.KIND_CHANNELS)
            t = median_ms({"fused": fused, "torch": stock}, a.reps, inner=5)
            for side in ("fused", "torch"):
                result[f"{key}_{side}_ms"], result[f"{key}_{side}_ms_min_max"] = t[side][0], list(t[side][1:])
                result[f"{key}_{side}_GB_per_s"] = moved / t[side][0] / 1e6
            result[key + "_bytes_moved"] = moved
            result[key + "_torch_over_fused"] = t["torch"][0] / t["fused"][0]
            result[key + "_launches_fused"], result[key + "_launches_torch"] = launches(fused), launches(stock)
            del vs, ref
            torch.cuda.empty_cache()


def make_views(V, H, W, seed=0):
    """V dataset records at the tracer's size with fp32 targets (the synthetic scene's own, shifted per view), and their poses."""
    hc_views = []
    base = syn.default_camera()
    tg = syn.make_targets(W, H)
    for i in range(V):
        eye = base["origin"].astype(np.float64) + np.array([0.06 * i, -0.04 * i, 0.02 * i])
        c2w = syn.look_at(eye, (1.2 - 0.05 * i, 0.5 + 0.03 * i, -0.9)).astype(np.float64)
        R = c2w.copy()
        R[:, 0] = -R[:, 0]
        R = -R
        images = {k + "_image": (v + np.float32(0.03 * i)).astype(np.float32) for k, v in tg.items()}
        hc_views.append(SimpleNamespace(R=R, T=-R.T @ eye, FovY=float(base["fov"]), **images))
    return hc_views


class CpuHalfCamera:
    """A camera as upstream holds it by default (scene/cameras.py:56-146): half images on the CPU, widened and uploaded at every access."""

    def __init__(self, pose, halfs):
        self.__dict__.update(vars(pose))
        self._halfs = halfs

    def __getattr__(self, name):  # (only reached for what is not in __dict__)
        halfs = self.__dict__.get("_halfs", {})
        if name in halfs:
            return halfs[name].float().cuda()
        raise AttributeError(name)


def bench_gather_and_step(a, result, parts):
    W, H, V = 1920, 1080, a.views
    infos = make_views(V, H, W)
    vs = ds.ViewSet(H, W, V)
    vs.add(infos, views_per_call=4)
    torch.cuda.synchronize()
    # today's callers: cameras that hold fp32 device images, and upstream's default - fp16 images on the CPU, widened and uploaded at every access
    dev_cams = [ren.camera_from_RT(i.R, i.T, i.FovY, **{attr: getattr(vs.camera(v), attr) for attr in ds.CAMERA_ATTRS[1:]}) for v, i in enumerate(infos)]
    cpu_cams = []
    for v, i in enumerate(infos):
        halfs = {attr: vs.planes[k + 1][v].cpu() for k, attr in enumerate(ds.CAMERA_ATTRS[1:])}
        cpu_cams.append(CpuHalfCamera(ren.camera_from_RT(i.R, i.T, i.FovY), halfs))

    def stack_today(cams):
        R, centers, fovy = ren._stack_cameras(cams, "cuda")
        return [torch.stack([getattr(c, attr) for c in cams]).contiguous() for _, attr, _ in ren.TRAIN_TARGETS], R, centers, fovy

    if "gather" in parts:
        for n in sorted({4, V}):
            idx = list(range(n))
            kinds = [k for k, _, _ in ren.TRAIN_TARGETS]
            out = vs.gather(idx, kinds)  # buffers kept across calls, as train keeps them
            fns = {"fused": lambda: vs.gather(idx, kinds, out), "torch": lambda: stack_today(dev_cams[:n])}
            for k, t in zip(kinds, stack_today(dev_cams[:n])[0]):
                assert torch.equal(out[k], t), k
            t = median_ms(fns, a.reps, inner=5)
            moved = n * 13 * H * W * (2 + 4)  # 13 channels: halfs read, floats written
            for side in ("fused", "torch"):
                result[f"gather_V{n}_{side}_ms"], result[f"gather_V{n}_{side}_ms_min_max"] = t[side][0], list(t[side][1:])
            result[f"gather_V{n}_fused_GB_per_s"] = moved / t["fused"][0] / 1e6
            result[f"gather_V{n}_torch_GB_per_s_of_its_own_bytes"] = n * 13 * H * W * 8 / t["torch"][0] / 1e6  # the stack reads and writes fp32
            result[f"gather_V{n}_torch_over_fused"] = t["torch"][0] / t["fused"][0]
            result[f"gather_V{n}_launches_fused"], result[f"gather_V{n}_launches_torch"] = launches(fns["fused"]), launches(fns["torch"])
    if "step" in parts:
        for variant in a.variants.split(","):
            pc = ren.GaussianParams(syn.make_scene(a.n, variant, seed=0))
            rt = ren.GaussianRaytracer(pc, W, H, ppll_forward_size=400_000_000, ppll_backward_size=300_000_000)
            idx = list(range(V))
            fns = {"viewset_train": lambda: vs.train(idx, rt), "train_views_fp32_device_images": lambda: ren.train_views(dev_cams, rt),
                   "train_views_fp16_cpu_images": lambda: ren.train_views(cpu_cams, rt)}
            t = median_ms(fns, a.reps, inner=1, warm=3)
            for k, (med, lo, hi) in t.items():
                result[f"step_{variant}_{k}_ms_per_view"], result[f"step_{variant}_{k}_ms_per_view_min_max"] = med / V, [lo / V, hi / V]
            result[f"step_{variant}_status"] = int(rt.cuda_module.get_counters()[11])
            del rt, pc
            torch.cuda.empty_cache()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--views", type=int, default=8)
    p.add_argument("--parts", default="ingest,gather,step")
    p.add_argument("--variants", default="trained,init")
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--tag", default="viewset_bench")
    a = p.parse_args()
    assert torch.cuda.is_available(), "viewset_bench.py needs a GPU"
    assert a.reps >= 7, "medians of at least 7 repetitions"
    parts = a.parts.split(",")
    result = dict(views=a.views, reps=a.reps, n=a.n, device=torch.cuda.get_device_name(0))
    out_dir = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out_dir, exist_ok=True)

    def write():
        with open(os.path.join(out_dir, "viewset_bench.json"), "w") as f:
            json.dump(result, f, indent=1)

    with torch.no_grad():
        if "ingest" in parts:
            bench_ingest(a, result)
            write()
    if "gather" in parts or "step" in parts:
        bench_gather_and_step(a, result, parts)
    write()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
