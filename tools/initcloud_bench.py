"""initialization.dense_init_cloud against the stock-torch sequence it replaces, on the same device and inputs: fp64 unprojection of every pixel of every view,
torch.unique(dim=0, return_inverse, return_counts) of the rounded coordinates, index_add_ of the colours, divide, mask - what the reference's prepare_initial_ply.py
does on the CPU, stated here in the project's own formulation (include/egr_raytracer.h). The scene is the synthetic room of synthetic.py seen by V cameras at
1920x1080 (synthetic.room_poses); depth is analytic (ray against the room's box and spheres), the colour a fixed pattern, both made on the device. The two paths are
checked equal first (coordinates, counts and points bit for bit), then timed alternating in one process (median of --reps, host clock, every timed region between
device synchronisations). Reports ms, peak device memory above the inputs (torch.cuda.max_memory_allocated), kernel launches (torch's profiler, in a pass of its
own), voxels and table growths. For the fused path also `fused_add_only` (host clock: table set-up + stacking + upload + accumulate launches, without the
extraction) and, when all views fit one chunk, `accumulate_launch_ms`: the device time of the accumulate launch alone, between two events. Kernel times proper come
from running this tool under `rocprofv3 --kernel-trace --stats`.
Writes runs/<tag>/initcloud_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/initcloud_bench.py [--views 8,64] [--reps 5] [--fused-only] [--tag initcloud]"""
import argparse
import importlib
import json
import math
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
syn = importlib.import_module("editable-gaussian-reflections_amd.synthetic")
init = importlib.import_module("editable-gaussian-reflections_amd.initialization")
W, H = 1920, 1080
SCALE = 400.0


def pixel_centres(n):
    return (torch.arange(n, device="cuda", dtype=torch.float64) + 0.5) / n


def unit_rays(c2w, view_size):
    """Unit primary ray directions [H,W,3] in fp64 on the device, in the formulation of include/egr_raytracer.h (and tests/init_restatement.py): the camera-space
    point ((W / H) view_size (2u - 1), view_size (1 - 2v), -1) through c2w, component by component, divided by its length."""
    cx = ((W / H) * view_size * (2.0 * pixel_centres(W) - 1.0))[None, :]
    cy = (view_size * (1.0 - 2.0 * pixel_centres(H)))[:, None]
    d = torch.stack([cx * c2w[i, 0] + cy * c2w[i, 1] - c2w[i, 2] for i in range(3)], dim=-1)
    return d / (d[..., 0] ** 2 + d[..., 1] ** 2 + d[..., 2] ** 2).sqrt()[..., None]


def room_depth(eye, d):
    """synthetic.room_depth on the device."""
    half = torch.tensor(syn.ROOM_HALF, device="cuda", dtype=torch.float64)
    inf = torch.full_like(d, float("inf"))
    t = torch.where(d > 0, (half - eye) / d, torch.where(d < 0, (-half - eye) / d, inf)).amin(dim=-1)
    for c, r in syn.SPHERES:
        oc = eye - torch.tensor(c, device="cuda", dtype=torch.float64)
        b = (d * oc).sum(-1)
        disc = b * b - ((oc * oc).sum() - r * r)
        near = -b - torch.sqrt(disc.clamp_min(0.0))
        t = torch.where((disc > 0) & (near > 0), torch.minimum(t, near), t)
    return t


def views(V):
    """V CameraInfo-like objects whose images live on the device."""
    out = []
    for eye, c2w, fov in syn.room_poses(V):
        R, T = syn.dataset_pose(eye, c2w)
        d = unit_rays(torch.from_numpy(c2w).cuda(), math.tan(fov * 0.5))
        e = torch.from_numpy(eye).cuda()
        depth = room_depth(e, d)
        hit = e + d * depth[..., None]
        checker = (torch.floor(hit * 2.0 + 1e-6).sum(-1).long() & 1).double()
        colour = ((0.2 + 0.6 * checker)[..., None] * torch.tensor([1.0, 0.9, 0.8], device="cuda", dtype=torch.float64) + 0.1 * (d * 0.5 + 0.5)).float().contiguous()
        out.append(SimpleNamespace(R=R, T=T, FovY=fov, depth_image=depth.float()[..., None].contiguous(), diffuse_image=colour))
    return out


def torch_sequence(cams):
    """The dense cloud with stock torch operations on the device, holding every pixel at once: fp64 unprojection, torch.unique(dim=0) of the rounded coordinates,
    index_add_ of the colours, divide, mask."""
    position, colour = [], []
    for c in cams:
        c2w, origin, view_size = init.camera_setup(c.R, c.T, c.FovY)
        rays = unit_rays(torch.from_numpy(c2w).cuda(), view_size)
        position.append((torch.from_numpy(origin).cuda() + rays * c.depth_image.double()).view(-1, 3))
        colour.append(c.diffuse_image.view(-1, 3))
    position, colour = torch.cat(position), torch.cat(colour)
    voxel = torch.round(position * SCALE).to(torch.int32)
    coords, member, count = torch.unique(voxel, dim=0, return_inverse=True, return_counts=True)
    total = torch.zeros((coords.shape[0], 3), dtype=torch.float32, device="cuda").index_add_(0, member, colour)
    keep = count >= 2
    coords, count = coords[keep], count[keep]
    # an IEEE division: with a Python float as the divisor torch multiplies by the reciprocal on the device, which rounds half of the points differently
    points = coords.to(torch.float32) / torch.tensor(SCALE, dtype=torch.float32, device="cuda")
    return SimpleNamespace(coords=coords, points=points, colors=total[keep] / count[:, None], counts=count)


def accumulate_launch_ms(cams, capacity, reps):
    """Device time of the ONE accumulate launch of all views, between two events on the stream; the table (re-initialised before every repetition) and the stacked
    inputs are prepared outside the timed region."""
    acc = init.VoxelAccumulator(voxel_scale=SCALE, initial_capacity=capacity)
    staged = acc.stage(cams)
    ms = []
    for _ in range(reps + 1):  # (the first one warms up)
        acc.keys.fill_(-1), acc.acc.zero_(), acc.status.zero_()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        acc.launch(staged)
        end.record()
        torch.cuda.synchronize()
        ms.append(start.elapsed_time(end))
    assert int(acc.status[3]) == 0
    return ms[1:]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def launches(fn):
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", default="8,64")
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--fused-only", action="store_true")
    p.add_argument("--tag", default="initcloud")
    a = p.parse_args()
    assert torch.cuda.is_available(), "initcloud_bench.py needs a GPU"
    init.load_library()
    pkg = importlib.import_module("editable-gaussian-reflections_amd")
    result = {"variant": pkg.VARIANT, "width": W, "height": H, "voxel_scale": SCALE}
    out = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out, exist_ok=True)
    for V in [int(v) for v in a.views.split(",")]:
        cams = views(V)
        state = {}

        def fused():
            acc = init.VoxelAccumulator(voxel_scale=SCALE)
            acc.add(cams)
            state["acc"] = acc
            return acc.extract()

        def add_only():  # host clock: allocating and filling the table at its final capacity, stacking the views, the upload, the read-back of `occupied`, the launches
            init.VoxelAccumulator(voxel_scale=SCALE, initial_capacity=state["acc"].capacity).add(cams)

        got = fused()  # (also the warm-up)
        acc = state["acc"]
        row = {"pixels": V * H * W, "voxels": int(acc.status[0]), "kept": int(got.counts.shape[0]), "largest_count": int(acc.status[4]), "growths": acc.growths, "capacity": acc.capacity,
               "pixels_without_slot": int(acc.status[3])}
        legs = [("fused", fused), ("fused_add_only", add_only)]
        if not a.fused_only:
            ref = torch_sequence(cams)
            same = ref.coords.shape == got.coords.shape and torch.equal(ref.coords, got.coords) and torch.equal(ref.counts.int(), got.counts) and torch.equal(ref.points, got.points)
            if not same:  # say what differs: torch's fp64 device arithmetic (a BLAS product, its own norm) may round a coordinate next to a half-integer the other way
                pack = lambda c: ((c[:, 0].long() + (1 << 20)) << 42) | ((c[:, 1].long() + (1 << 20)) << 21) | (c[:, 2].long() + (1 << 20))
                kr, kg = pack(ref.coords), pack(got.coords)
                row["rows_torch"], row["rows_fused"] = int(kr.shape[0]), int(kg.shape[0])
                row["rows_only_in_torch"], row["rows_only_in_fused"] = int((~torch.isin(kr, kg)).sum()), int((~torch.isin(kg, kr)).sum())
                row["torch_rows_sorted_by_key"] = bool((kr[1:] > kr[:-1]).all())
                if kr.shape == kg.shape and torch.equal(kr, kg):
                    row["counts_differing"] = int((ref.counts.int() != got.counts).sum())
                    row["points_differing"] = int((ref.points != got.points).any(dim=1).sum())
                print("the two paths disagree:", json.dumps(row), flush=True)
                assert row["rows_only_in_torch"] + row["rows_only_in_fused"] <= 8 and row["torch_rows_sorted_by_key"], "the two paths disagree by more than a few boundary voxels"
            row["paths_identical"] = bool(same)
            if same:
                row["max_colour_difference"] = float((ref.colors - got.colors).abs().max())
            del ref
            legs.append(("torch", lambda: torch_sequence(cams)))
        del got
        ts = {label: [] for label, _ in legs}
        for _ in range(a.reps):  # alternating: drifts of clock and temperature hit all paths alike
            for label, fn in legs:
                ts[label].append(timed(fn)[0])
        for label, fn in legs:
            row[f"{label}_ms"] = float(np.median(ts[label]))
            row[f"{label}_ms_min_max"] = [float(min(ts[label])), float(max(ts[label]))]
        state.clear()
        del acc
        for label, fn in legs:
            if label != "fused_add_only":
                row[f"{label}_peak_bytes"] = peak(fn)
        state.clear()
        if V <= 8:  # one chunk: all views in one launch
            launch = accumulate_launch_ms(cams, row["capacity"], max(a.reps, 5))
            row["accumulate_launch_ms"], row["accumulate_launch_ms_min_max"] = float(np.median(launch)), [float(min(launch)), float(max(launch))]
            row["accumulate_launch_pixels_per_s"] = V * H * W / (row["accumulate_launch_ms"] * 1e-3)
        if not a.fused_only:
            row["torch_over_fused"] = row["torch_ms"] / row["fused_ms"]
        result[f"V{V}"] = row
        with open(os.path.join(out, "initcloud_bench.json"), "w") as f:  # the timings are on disk before the profiler starts
            json.dump(result, f, indent=1)
        for label, fn in legs:
            if label != "fused_add_only":
                row[f"{label}_launches"] = launches(fn)
        state.clear()
        with open(os.path.join(out, "initcloud_bench.json"), "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps({f"V{V}": row}), flush=True)
        del cams
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
