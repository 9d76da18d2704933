"""Per-object coverage (editing.selection_masks / egr_object_masks) at 1920x1080 on the 1M dense-init and trained-like clouds with K = 4 and K = 16 box objects
(a grid of boxes over the room; rows_in_objects reports how many gaussians they hold). Three times per case, medians over --reps after a warm-up, host clock around a device synchronise:

  call    the one call: selection_masks (no export, no refit: nothing is dirty), plus one `pick` read-back
  loop    the reference's selection-mode loop (gaussian_viewer.py:292-321) restated with this project's `render`: per object the indicator into _diffuse,
          render(force_update_bvh=True), rgb[0].mean(dim=0), then _diffuse restored; plus the hover's K read-backs (mask[i, j] of every object)
  floor   one render_views frame of the same camera with num_bounces = 0: what a primary pass that composites the appearance costs

Next to the times: tracer launches (the library's lifetime launch counter), chain kernels per run (egr_last_kernel_ms entries) and host synchronisations (read-backs;
neither path needs one to produce its device tensors). --floor-only times the floor alone (a checkout without the feature, e.g. the parent commit).
Writes runs/<tag>/masks_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/masks_bench.py [--reps 7] [--configs C-init,C-trained] [--ks 4,16] (any K <= 32; 32 shows what the [K][64] sums in LDS cost in resident waves) [--tag masks_bench] [--floor-only | --call-only]"""
import argparse
import importlib
import json
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


def grid_boxes(K):
    """K boxes that tile the room: a kx x ky grid of columns over x and y (4: 2 x 2, 16: 4 x 4, 32: 4 x 8)."""
    kx = max(d for d in range(1, int(K ** 0.5) + 1) if K % d == 0)
    ky = K // kx
    lo, hi = -syn.ROOM_HALF * 1.01, syn.ROOM_HALF * 1.01
    xs, ys = np.linspace(lo[0], hi[0], kx + 1), np.linspace(lo[1], hi[1], ky + 1)
    eps = 1e-6  # (box ends are inclusive: the upper faces are pulled in so that no row is in two boxes)
    return {"box%d_%d" % (i, j): dict(min=[float(xs[i]), float(ys[j]), float(lo[2])], max=[float(xs[i + 1] - eps), float(ys[j + 1] - eps), float(hi[2])])
            for i in range(kx) for j in range(ky)}


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=round(float(np.median(ts)), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3), reps=reps)


def counted(m, fn):
    """(tracer launches, kernel stamps by name) of one run of fn."""
    m.reset_lifetime_counters()
    torch.cuda.synchronize()
    before = int(m.get_counters()[10])
    m.enable_timing(True)
    fn()
    torch.cuda.synchronize()
    acc = {}
    for name, ms in m.last_kernel_ms():  # (the LAST traced call's stamps: the one call, or the loop's last render)
        acc[name] = round(acc.get(name, 0.0) + ms, 3)
    m.enable_timing(False)
    return int(m.get_counters()[10]) - before, acc


def floor_frame(g, cam, reps):
    """The floor: a primary-only frame (num_bounces = 0) through render_views on a plain model."""
    rt = ren.GaussianRaytracer(ren.GaussianParams(g), W, H, ppll_forward_size=400_000_000, ppll_backward_size=1_000_000)
    m = rt.cuda_module
    m.get_config().num_bounces.fill_(0)
    floor_fn = lambda: ren.render_views([cam], rt, spp=1, outputs=("final", "rgb"))
    floor_fn(), floor_fn()
    floor = timed(floor_fn, reps)
    launches, kms = counted(m, floor_fn)
    del rt, m
    torch.cuda.empty_cache()
    return dict(what="floor_render_views_num_bounces_0", tracer_launches=launches, kernels_ms=kms, **floor)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--configs", default="C-init,C-trained")
    p.add_argument("--ks", default="4,16")
    p.add_argument("--tag", default="masks_bench")
    p.add_argument("--floor-only", action="store_true")
    p.add_argument("--call-only", action="store_true", help="the one call alone (a sweep over builds: EGR_EXTRA_FLAGS selects the variant)")
    a = p.parse_args()
    assert torch.cuda.is_available(), "masks_bench.py needs a GPU"
    ed = None if a.floor_only else importlib.import_module("editable-gaussian-reflections_amd.editing")
    base = syn.default_camera()
    cam = ren.camera_from_c2w(base["origin"], base["c2w"], base["fov"])
    results = []
    for cfg in a.configs.split(","):
        N, variant = CONFIGS[cfg]
        g = syn.make_scene(N, variant, seed=0)
        if not a.call_only:
            row = dict(config=cfg, n=N, **floor_frame(g, cam, a.reps))
            print(json.dumps(row), flush=True)
            results.append(row)
        if a.floor_only:
            continue
        for K in [int(k) for k in a.ks.split(",")]:
            e = ed.EditableGaussians(ren.GaussianParams(g), grid_boxes(K))
            sizes = [int(e.selection(nm).sum()) for nm in e.names]
            assert min(sizes) > 0, sizes  # (a row on a shared face may sit in two boxes or, by fp32 rounding of the pulled-in face, in none: rows_in_objects says)
            rt = ren.GaussianRaytracer(e, W, H, ppll_forward_size=400_000_000, ppll_backward_size=1_000_000)
            m = rt.cuda_module
            state = {}

            def call():
                state["res"] = ed.selection_masks(cam, rt)

            def call_pick():
                return ed.pick(state["res"], W // 2, H // 2)  # one read-back

            def loop():
                keep = e._diffuse.clone()
                masks = []
                with torch.no_grad():
                    for nm in e.names:
                        e._diffuse.copy_(e.selection(nm).to(torch.float32)[:, None].expand(-1, 3))
                        masks.append(ren.render(cam, rt, targets_available=False, force_update_bvh=True).rgb[0].mean(dim=0))
                    e._diffuse.copy_(keep)
                state["loop"] = masks

            def loop_pick():
                picked = None
                for nm, mk in zip(e.names, state["loop"]):  # gaussian_viewer.py:728-745: mask[i, j] of every object, the last non-zero one wins
                    if float(mk[H // 2, W // 2]) != 0.0:  # K read-backs
                        picked = nm
                return picked

            for label, fn, pick_fn, syncs in (("call", call, call_pick, 1), ("loop", loop, loop_pick, K))[: 1 if a.call_only else 2]:
                fn(), fn()  # warm-up (the first call allocates; the loop's first render uploads nothing new afterwards)
                t = timed(fn, a.reps)
                launches, kms = counted(m, fn)
                if label == "call":  # (a query counts no frame in the lifetime counters: its one chain launch is the forward_objects stamp)
                    assert launches == 0 and "forward_objects" in kms, (launches, kms)
                    launches = 1
                tp = timed(pick_fn, a.reps)
                status = int(m.get_counters()[11])
                row = dict(config=cfg, n=N, K=K, what=label, tracer_launches=launches, host_syncs_to_pick=syncs, rows_in_objects=sum(sizes), pick_median_ms=tp["median_ms"], last_launch_kernels_ms=kms,
                           status=status, picked=pick_fn(), **t)
                print(json.dumps(row), flush=True)
                results.append(row)
            # (the loop's masks differ from the call's by their seeds - one launch number each - and by mean(dim=0); with jitter off and the seed pinned they are the
            # bits tests/test_hip_object_masks.py compares)
            del rt, m, e
            torch.cuda.empty_cache()
    out = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "masks_bench.json"), "w") as f:
        json.dump(dict(width=W, height=H, results=results), f, indent=1)
    print("wrote", os.path.join(out, "masks_bench.json"))


if __name__ == "__main__":
    main()
