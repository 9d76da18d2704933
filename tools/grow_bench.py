"""The growth step at full size: trainer.FusedTrainStep.add_farfield_points (csrc/grow.hip: one sample launch, the prune kernels as the camera filter, one append
launch, one read-back) against the stock sequence it replaces - torch.randn(...).clamp(-3, 3) * radius, one `(points - T).norm(dim=1) < znear` chain per camera as
scene.select_points_to_prune_near_cameras runs it, boolean indexing, distCUDA2 and the constant tensors of gaussian_model.py:233-283, one torch.cat for each of the
8 parameters and 16 moments, rebuild_bvh - on a 1M dense-init cloud with 75,000 candidates and 200 cameras. Both paths run in one process, alternating, from the
same restored state; every timed region is bracketed by device synchronisations; each figure is the median of --reps runs. Measured with and without the rebuild
(resize + export + full tree build, common to both paths). The append alone (torch.ops.egr.grow_append over the 24 arrays against 24 torch.cat) is timed as well.
The host synchronisations of one run of each path are counted with torch's sync debug mode, the device launches (kernels and copies) with torch's profiler.
Writes runs/<tag>/grow_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/grow_bench.py [--reps 7] [--n 1000000] [--candidates 75000] [--cameras 200] [--tag grow_bench]"""
import argparse
import importlib
import json
import os
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
syn = importlib.import_module("editable-gaussian-reflections_amd.synthetic")
ren = importlib.import_module("editable-gaussian-reflections_amd.renderer")
tr = importlib.import_module("editable-gaussian-reflections_amd.trainer")
knn = importlib.import_module("editable-gaussian-reflections_amd.simple_knn")

LRS = dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)
RADIUS, ZNEAR, SEED = 3.0, 0.5, 750


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--candidates", type=int, default=75_000)
    p.add_argument("--cameras", type=int, default=200)
    p.add_argument("--tag", default="grow_bench")
    a = p.parse_args()
    assert torch.cuda.is_available(), "grow_bench.py needs a GPU"
    assert a.reps >= 7, "medians of at least 7 repetitions"
    N, K, C = a.n, a.candidates, a.cameras
    pc = ren.GaussianParams(syn.make_scene(N, "init", seed=0))
    rt = ren.GaussianRaytracer(pc, 64, 64)
    step = tr.FusedTrainStep(pc, rt, LRS)
    gen = torch.Generator(device="cuda").manual_seed(0)
    names = [n for n, _, _ in tr.GROUPS]
    attrs = [at for _, at, _ in tr.GROUPS]
    # the state every run starts from: parameters, moments with content, cameras spread like the candidates
    master = {at: getattr(pc, at).clone() for at in attrs}
    moments = {n: (torch.randn(step.exp_avg[n].shape, device="cuda", generator=gen), torch.rand(step.exp_avg[n].shape, device="cuda", generator=gen)) for n in names}
    centers = (torch.randn((C, 3), device="cuda", generator=gen) * (0.5 * RADIUS)).contiguous()
    znear = torch.full((C,), ZNEAR, device="cuda")
    znear_host = znear.tolist()  # (upstream's camera.znear is a host number per camera)
    rebuild = ren.GaussianRaytracer.rebuild_bvh

    def restore():
        for at in attrs:
            t = master[at].clone()
            t.grad = torch.zeros_like(t)
            setattr(pc, at, t)
        for n in names:
            step.exp_avg[n], step.exp_avg_sq[n] = moments[n][0].clone(), moments[n][1].clone()
        rebuild(rt)
        torch.cuda.synchronize()

    def fused(with_rebuild):
        rt.rebuild_bvh = (lambda: rebuild(rt)) if with_rebuild else (lambda: None)  # (without: the call's own part - sample, filter, read-back, initial values, append, install)
        try:
            return step.add_farfield_points(K, RADIUS, SEED, cam_centers=centers, cam_znear=znear)[0]
        finally:
            del rt.rebuild_bvh

    def torch_sequence(with_rebuild):
        xyz = torch.randn(K, 3, device="cuda").clamp(-3, 3) * RADIUS  # gaussian_model.py:236
        mask = torch.zeros(K, dtype=torch.bool, device="cuda")
        for c in range(C):  # scene.py:94-103
            mask |= (xyz - centers[c]).norm(dim=1) < znear_host[c]
        xyz = xyz[~mask]
        k = xyz.shape[0]
        dist2 = torch.clamp_min(knn.distCUDA2(xyz), 0.0000001)
        rotation = torch.zeros((k, 4), device="cuda")
        rotation[:, 0] = 1
        opacity = 0.1 * torch.ones((k, 1), dtype=torch.float, device="cuda")
        new = dict(_xyz=xyz, _scaling=torch.log(torch.sqrt(dist2) * 0.1)[..., None].repeat(1, 3), _rotation=rotation, _opacity=torch.log(opacity / (1 - opacity)),
                   _diffuse=torch.ones_like(xyz) * 0.2, _normal=torch.zeros_like(xyz), _f0=torch.ones_like(xyz) * 0.04, _roughness=torch.zeros_like(xyz)[:, :1])
        for at in attrs:  # GaussianParams.append_points on device tensors: cat_tensors_to_optimizer's parameter half
            t = torch.cat([getattr(pc, at), new[at]], 0)
            t.grad = torch.zeros_like(t)
            setattr(pc, at, t)
        step.extend(k)  # ... and its moment half: 16 more torch.cat
        if with_rebuild:
            rt.rebuild_bvh()
        return k

    paths = (("fused", fused), ("torch", torch_sequence))
    result = dict(n=N, candidates=K, cameras=C, reps=a.reps, device=torch.cuda.get_device_name(0))
    for label, fn in paths:  # the host synchronisations of one run (torch warns at every synchronising call in this mode)
        restore()
        fn(True)  # warm-up of every shape
        restore()
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                result["added_" + label] = fn(True)
            result["host_syncs_" + label] = sum("synchroniz" in str(x.message).lower() for x in w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert pc._xyz.shape[0] == N + result["added_" + label] == rt.cuda_module.get_gaussians().mean.shape[0]
    result["removed_share_fused"] = 1.0 - result["added_fused"] / K
    for with_rebuild in (True, False):
        ts = {label: [] for label, _ in paths}
        for _ in range(a.reps):  # alternating: drifts of clock and temperature hit both paths alike
            for label, fn in paths:
                restore()
                t0 = time.perf_counter()
                fn(with_rebuild)
                torch.cuda.synchronize()
                ts[label].append((time.perf_counter() - t0) * 1e3)
        key = "with_rebuild" if with_rebuild else "without_rebuild"
        for label, _ in paths:
            result[f"{label}_ms_{key}"] = float(np.median(ts[label]))
            result[f"{label}_ms_{key}_min_max"] = [float(min(ts[label])), float(max(ts[label]))]
        result[f"torch_over_fused_{key}"] = result[f"torch_ms_{key}"] / result[f"fused_ms_{key}"]

    # the append alone: the 24 arrays of the model, K new rows each (all candidates), one launch against 24 torch.cat
    restore()
    src = [getattr(pc, at) for at in attrs] + [step.exp_avg[n] for n in names] + [step.exp_avg_sq[n] for n in names]
    rows = [torch.randn((K,) + tuple(t.shape[1:]), device="cuda", generator=gen) for t in src[:8]]
    zeros = [torch.zeros((K,) + tuple(t.shape[1:]), device="cuda") for t in src[8:]]
    appends = (("append_one_launch", lambda: torch.ops.egr.grow_append(src, rows + [None] * 16, [0] * 24, K)),
               ("append_24_cat", lambda: [torch.cat([t, r], 0) for t, r in zip(src, rows + zeros)]))
    ts = {label: [] for label, _ in appends}
    for rep in range(a.reps + 2):
        for label, fn in appends:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if rep >= 2:  # (two warm-up rounds: the allocator has the blocks)
                ts[label].append((time.perf_counter() - t0) * 1e3)
            del out
    moved = 2 * sum(t.numel() + K * (t.numel() // N) for t in src) * 4
    for label, _ in appends:
        result[label + "_ms"] = float(np.median(ts[label]))
        result[label + "_ms_min_max"] = [float(min(ts[label])), float(max(ts[label]))]
        result[label + "_TB_per_s"] = moved / result[label + "_ms"] / 1e9
    result["append_bytes_read_plus_written"] = moved

    out_dir = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out_dir, exist_ok=True)

    def write():
        with open(os.path.join(out_dir, "grow_bench.json"), "w") as f:
            json.dump(result, f, indent=1)

    write()
    # device launches of one run of each path (kernels and memory operations the profiler records on the device), rebuild included
    try:
        from torch.profiler import ProfilerActivity, profile

        for label, fn in paths:
            restore()
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                fn(True)
                torch.cuda.synchronize()
            result["device_launches_" + label] = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as e:  # (a torch without a working device profiler: the times above stand)
        result["device_launches_error"] = repr(e)
    write()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
