"""The fused frames of an evaluation (torch.ops.egr.eval_frames, csrc/frames.hip) against the stock-torch sequence they replace, at 1920x1080, V = 8 views, all
seven kinds, inputs on the device (a working set of 3 GB: far past the Infinity Cache). The stock sequence is what render.py:218-292 does per view up to the
file write: fourteen display or affine chains (tonemap + clamp, x / amax, x / 2 + 0.5), save_image's mul(255).add_(0.5).clamp_(0, 255), permute, .to(uint8) - the
bytes stay on the device on both sides, so the comparison is of launch sets alone. The bytes that differ between the two are counted first, then both are timed
alternating in one process (medians of --reps, every timed region between device synchronisations).
Prints: ms and launches of both sides, GB/s of the fused kernel over its 190 B per pixel and view (80 B predictions + 68 B targets read, 42 B written), the
download a host needs per view as bytes against floats, and the host PNG encode time of one 1080p frame per filter and level (formats.write_png, one thread).
Writes runs/<tag>/frames_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/frames_bench.py [--reps 7] [--views 8] [--tag frames_bench]"""
import argparse
import importlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ev = importlib.import_module("editable-gaussian-reflections_amd.evaluation")
fm = importlib.import_module("editable-gaussian-reflections_amd.formats")
W, H = 1920, 1080
BYTES_PER_PIXEL = 80 + 68 + 42


def inputs(V):
    """Smooth images with a little noise: what a render looks like to a PNG encoder (pure noise would not compress at all)."""
    g = torch.Generator(device="cuda").manual_seed(0)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H, device="cuda"), torch.linspace(0, 1, W, device="cuda"), indexing="ij")
    base = torch.stack([0.5 + 0.4 * torch.sin(9 * xx + 3 * yy), 0.5 + 0.4 * torch.cos(5 * yy - 2 * xx), 0.3 + 0.6 * xx * yy], -1)  # [H,W,3] in [0.1, 0.9]
    noise = lambda *s: 0.02 * torch.randn(*s, device="cuda", generator=g)
    pm3 = lambda: (base[None, None] * (1 + noise(V, 3, H, W, 3))).contiguous()
    pm1 = lambda: (base[None, None, ..., :1] * (1 + noise(V, 3, H, W, 1))).contiguous()
    cm3 = lambda: (base.movedim(-1, 0)[None] * (1 + noise(V, 3, H, W))).contiguous()
    cm1 = lambda: (base.movedim(-1, 0)[None, :1] * (1 + noise(V, 1, H, W))).contiguous()
    pred = dict(final=(2 * base[None] * (1 + noise(V, H, W, 3))).contiguous(), rgb=pm3(), depth=(1 + 3 * pm1()).contiguous(), normal=(2 * pm3() - 1).contiguous(), roughness=pm1(),
                f0=pm3())
    target = dict(render=2 * cm3(), diffuse=cm3(), specular=2 * cm3(), depth=(1 + 3 * cm1()).contiguous(), normal=(2 * cm3() - 1).contiguous(), roughness=cm1(), f0=cm3())
    return pred, target


def stock(pred, target):
    """render.py:218-292 up to the file write, per view, in stock torch. Returns per view the fourteen uint8 [H,W,3] images in the order of `ev.KINDS`, prediction first."""
    to_bytes = lambda x: (x.expand(3, -1, -1) if x.shape[0] == 1 else x).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8)  # make_grid, save_image
    chw = lambda x: x.movedim(-1, 0)
    out = []
    for v in range(pred["final"].shape[0]):
        hi = target["depth"][v].amax()
        pairs = [(ev.display(chw(pred["final"][v])), ev.display(target["render"][v])), (ev.display(chw(pred["rgb"][v, 0])), ev.display(target["diffuse"][v])),
                 (ev.display(chw(pred["rgb"][v, 1:].sum(dim=0))), ev.display(target["specular"][v])), (chw(pred["depth"][v, 0]) / hi, target["depth"][v] / hi),
                 (chw(pred["normal"][v, 0]) / 2 + 0.5, target["normal"][v] / 2 + 0.5), (chw(pred["roughness"][v, 0]), target["roughness"][v]),
                 (chw(pred["f0"][v, 0]), target["f0"][v])]
        out.append([to_bytes(x) for pair in pairs for x in pair])
    return out


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


def encode_times(frame, reps=3):
    """Host ms and file bytes of formats.write_png on one [H,W,3] frame, per filter and level, one thread."""
    out = {}
    for filt in ("none", "sub", "up"):
        for level in (1, 6):
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                n = fm.write_png(io.BytesIO(), frame, level=level, filter=filt)
                ts.append((time.perf_counter() - t0) * 1e3)
            out[f"{filt}/{level}"] = dict(ms=float(np.median(ts)), bytes=n)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--views", type=int, default=8)
    p.add_argument("--tag", default="frames_bench")
    a = p.parse_args()
    assert torch.cuda.is_available(), "frames_bench.py needs a GPU"
    ev.load_library()
    V = a.views
    pred, target = inputs(V)
    fused = lambda **kw: ev.frames(**pred, targets=target, **kw)
    got = fused()
    ref = stock(pred, target)
    torch.cuda.synchronize()
    # a sanity count, not a test (tests/test_hip_frames.py pins every byte: the plain kinds to CPU torch, the tone-mapped kinds to eval_metrics' display): the tone
    # curve's powf may differ from torch's pow in the last place, which moves a byte only at a threshold
    differ = {}
    for k, kind in enumerate(ev.KINDS):
        for s, side in enumerate(("pred", "gt")):
            n = sum(int((got.frames[v, k, s] != ref[v][2 * k + s]).sum()) for v in range(V))
            differ[f"{kind}/{side}"] = n
    tone_total = sum(n for key, n in differ.items() if key.split("/")[0] in ev.KINDS[:3])
    plain_total = sum(differ.values()) - tone_total
    print(f"bytes that differ from stock torch on the device: plain kinds {plain_total} of {8 * V * H * W * 3}, tone-mapped kinds {tone_total} of {6 * V * H * W * 3} "
          f"(torch's pow against powf)", flush=True)
    del ref
    t_fused, t_stock, t_sbs = interleaved([fused, lambda: stock(pred, target), lambda: fused(layout="side_by_side")], a.reps)
    t_part = {name: interleaved([lambda: ev.frames(**pred, targets=target, kinds=kinds)], a.reps)[0] for name, kinds in (("tone-mapped", ev.KINDS[:3]), ("plain", ev.KINDS[3:]))}
    n_fused, n_stock = launches(fused), launches(lambda: stock(pred, target))
    gbs = lambda ms: V * H * W * BYTES_PER_PIXEL / (ms * 1e-3) / 1e9
    print(f"V={V} {W}x{H}, all seven kinds, {V * H * W * BYTES_PER_PIXEL / 1e9:.2f} GB per call", flush=True)
    print(f"  eval_frames separate     {t_fused:8.3f} ms  {n_fused:4d} launches  {gbs(t_fused):6.0f} GB/s over 190 B per pixel and view", flush=True)
    print(f"  eval_frames side by side {t_sbs:8.3f} ms                {gbs(t_sbs):6.0f} GB/s", flush=True)
    print(f"  stock torch              {t_stock:8.3f} ms  {n_stock:4d} launches  = {n_stock / V:.0f} per view;  {t_stock / t_fused:.2f}x", flush=True)
    print(f"  eval_frames, the three tone-mapped kinds alone {t_part['tone-mapped']:.3f} ms ({V * H * W * (84 + 18) / t_part['tone-mapped'] / 1e6:.0f} GB/s over 102 B), "
          f"the four plain kinds alone {t_part['plain']:.3f} ms ({V * H * W * (64 + 24) / t_part['plain'] / 1e6:.0f} GB/s over 88 B)", flush=True)
    per_view_bytes, per_view_floats = 14 * H * W * 3, 14 * H * W * 3 * 4
    print(f"  download per view: {per_view_bytes / 1e6:.1f} MB of bytes against {per_view_floats / 1e6:.1f} MB of floats", flush=True)
    enc = encode_times(got.frames[0, 0, 0].cpu().numpy())
    for key, r in enc.items():
        print(f"  write_png 1080p render frame, filter/level {key:7s}: {r['ms']:7.1f} ms, {r['bytes'] / 1e6:.2f} MB", flush=True)
    out_dir = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "frames_bench.json"), "w") as f:
        json.dump(dict(views=V, width=W, height=H, reps=a.reps, ms=dict(fused=t_fused, fused_side_by_side=t_sbs, stock=t_stock, fused_tone_mapped=t_part["tone-mapped"], fused_plain=t_part["plain"]),
                       launches=dict(fused=n_fused, stock=n_stock), GBps=dict(fused=gbs(t_fused), fused_side_by_side=gbs(t_sbs)), bytes_that_differ=differ,
                       download_per_view=dict(bytes=per_view_bytes, floats=per_view_floats), write_png=enc, device=torch.cuda.get_device_name(0)), f, indent=1)
    print("wrote", os.path.join(out_dir, "frames_bench.json"))


if __name__ == "__main__":
    main()
