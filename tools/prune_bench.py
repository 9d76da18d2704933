"""The pruning step at full size: trainer.FusedTrainStep.prune_and_rebuild (csrc/prune.hip: select + one gather, one read-back) against the torch sequence it
replaces - the caller's mask arithmetic (total_weight / interval < min_weight, then one `(points - T).norm(dim=1) < znear` chain per camera as
scene.select_points_to_prune_near_cameras runs it), GaussianParams.prune_points (8 tensors), FusedTrainStep.prune (16 moments), the zeroing and rebuild_bvh -
on a 1M dense-init cloud with 200 cameras and about 10 % of the rows removed. Both paths run in one process, alternating, from the same restored state; every
timed region is bracketed by device synchronisations; each figure is the median of --reps runs. Measured with and without the rebuild (resize + export + full
tree build, common to both paths). The host synchronisations of one run of each path are counted with torch's sync debug mode.
Writes runs/<tag>/prune_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/prune_bench.py [--reps 11] [--n 1000000] [--cameras 200] [--tag prune_bench]"""
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

LRS = dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)
INTERVAL, MIN_WEIGHT = 125, 0.07


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=11)
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--cameras", type=int, default=200)
    p.add_argument("--tag", default="prune_bench")
    a = p.parse_args()
    assert torch.cuda.is_available(), "prune_bench.py needs a GPU"
    assert a.reps >= 10, "medians of at least 10 repetitions"
    N, C = a.n, a.cameras
    pc = ren.GaussianParams(syn.make_scene(N, "init", seed=0))
    rt = ren.GaussianRaytracer(pc, 64, 64)
    step = tr.FusedTrainStep(pc, rt, LRS)
    gen = torch.Generator(device="cuda").manual_seed(0)
    names = [n for n, _, _ in tr.GROUPS]
    attrs = [at for _, at, _ in tr.GROUPS]
    # the state every run starts from: parameters, moments with content, a total_weight of which ~7 % lies under the threshold, cameras at gaussians of the cloud
    master = {at: getattr(pc, at).clone() for at in attrs}
    moments = {n: (torch.randn(step.exp_avg[n].shape, device="cuda", generator=gen), torch.rand(step.exp_avg[n].shape, device="cuda", generator=gen)) for n in names}
    weight = torch.rand((N, 1), device="cuda", generator=gen) * INTERVAL
    weight[(weight / INTERVAL - MIN_WEIGHT).abs() < 1e-5] = 0.0  # (torch may multiply by a rounded 1 / interval where the kernel divides: no row within an ulp of the threshold)
    centers = (pc._xyz[torch.randint(0, N, (C,), device="cuda", generator=gen)] + 0.01).contiguous()
    znear = torch.full((C,), 0.07, device="cuda")  # ~3 % of the cloud inside the 200 spheres
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
        rt.cuda_module.get_gaussians().total_weight.copy_(weight)
        torch.cuda.synchronize()

    def fused(with_rebuild):
        rt.rebuild_bvh = (lambda: rebuild(rt)) if with_rebuild else (lambda: None)  # (without: the call's own part - select, read-back, gather, install, zeroing)
        try:
            return step.prune_and_rebuild(min_weight=MIN_WEIGHT, interval=INTERVAL, cam_centers=centers, cam_znear=znear)[0]
        finally:
            del rt.rebuild_bvh

    def torch_sequence(with_rebuild):
        g = rt.cuda_module.get_gaussians()
        mask = (g.total_weight / INTERVAL < MIN_WEIGHT).reshape(-1)  # train.py:240
        points = pc._xyz
        for c in range(C):  # scene.py:94-103
            mask |= (points - centers[c]).norm(dim=1) < znear_host[c]
        pc.prune_points(mask)
        step.prune(~mask)
        g.total_weight.zero_()
        if with_rebuild:
            rt.rebuild_bvh()
        return pc._xyz.shape[0]

    paths = (("fused", fused), ("torch", torch_sequence))
    result = dict(n=N, cameras=C, reps=a.reps, device=torch.cuda.get_device_name(0))
    # same result, and the host synchronisations of one run (torch warns at every synchronising call in this mode)
    kept, state = {}, {}
    for label, fn in paths:
        restore()
        fn(True)  # warm-up of every shape
        restore()
        try:
            torch.cuda.set_sync_debug_mode("warn")
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                kept[label] = fn(True)
            result["host_syncs_" + label] = sum("synchroniz" in str(x.message).lower() for x in w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        state[label] = [getattr(pc, at).clone() for at in attrs] + [step.exp_avg[n].clone() for n in names] + [step.exp_avg_sq[n].clone() for n in names]
    assert kept["fused"] == kept["torch"] and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(state["fused"], state["torch"])), "the two paths differ"
    result["kept"], result["removed_share"] = kept["fused"], 1.0 - kept["fused"] / N
    del state
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
    out = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "prune_bench.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
