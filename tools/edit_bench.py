"""An edited frame's host step at full size: editing.EditableGaussians (csrc/edit.hip: one select launch when the objects are made, one edit-and-export launch
per frame) against the torch sequence it replaces - the fp32 restatement of the reference's make_editable and seven getter overrides
(tests/edit_restatement.py) followed by the eight export copies - on the 1M dense-init cloud with four objects: the three spheres of the synthetic room and
`everything`, each with all four groups of its edit active.
What is timed, each under its own name:
  select       the selection of the objects (once per object list)
  dirty_frame  one edit field changes before EVERY call (a slider moving), then export_edited: packing of the changed record, upload, launch; the torch side
               takes the same change and recomputes its getters and copies (as the reference does on a dirty frame)
  clean_frame  export_edited with unchanged edits (what every frame's export costs when nothing moved): bookkeeping and launch, no packing, no upload
  launch_only  torch.ops.egr.edit_apply alone, rotating over --sets sets of source and destination arrays (172 MB each at 1M rows) so that the sets together
               exceed the 256 MB Infinity Cache: its bytes/s over the 172 B per row the algorithm needs (88 read, 84 written) is an HBM figure
Both paths run in one process, alternating; every timed window is bracketed by device events and holds --inner calls of the fused path or --inner-torch calls of
the torch path; 5 warm-ups; each figure is the median of --reps windows, per call. Kernel launches of one call: torch's profiler, in a pass of its own after
the timing.
Writes runs/<tag>/edit_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/edit_bench.py [--reps 20] [--inner 200] [--inner-torch 10] [--sets 4] [--n 1000000] [--tag edit_bench]"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
syn = importlib.import_module("editable-gaussian-reflections_amd.synthetic")
ren = importlib.import_module("editable-gaussian-reflections_amd.renderer")
ed = importlib.import_module("editable-gaussian-reflections_amd.editing")
import edit_restatement as er  # noqa: E402

BYTES_PER_ROW = 88 + 84


def all_groups(k):
    return ed.Edit(roughness_shift=0.05 + 0.01 * k, roughness_mult=0.9, diffuse_override=(0.7, 0.3, 0.2, 0.25), diffuse_hue_shift=0.2 + 0.1 * k, diffuse_saturation_shift=0.04,
                   diffuse_saturation_mult=1.15, diffuse_value_shift=0.03, diffuse_value_mult=0.9, specular_override=(0.2, 0.6, 0.9, 0.3), specular_hue_shift=-0.3 - 0.1 * k,
                   specular_saturation_shift=0.02, specular_saturation_mult=0.85, specular_value_shift=-0.02, specular_value_mult=1.1, translate_x=0.05 * (k + 1),
                   translate_y=-0.05, translate_z=0.1, scale=1.0 + 0.05 * (k + 1), rotate_x=10.0 * (k + 1), rotate_y=-20.0, rotate_z=35.0)


def count_kernels(fn):
    """Kernel launches of one call of `fn`."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--inner", type=int, default=200)
    p.add_argument("--inner-torch", type=int, default=10)
    p.add_argument("--sets", type=int, default=4)
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--tag", default="edit_bench")
    a = p.parse_args()
    assert torch.cuda.is_available(), "edit_bench.py needs a GPU"
    assert a.reps >= 20, "medians of at least 20 alternating repetitions"
    N = a.n
    pc = ren.GaussianParams(syn.make_scene(N, "init", seed=0))
    boxes = {"sphere%d" % k: dict(min=[c[i] - r - 0.01 for i in range(3)], max=[c[i] + r + 0.01 for i in range(3)]) for k, (c, r) in enumerate(syn.SPHERES)}
    boxes["everything"] = dict(min=(-syn.ROOM_HALF).tolist(), max=syn.ROOM_HALF.tolist())
    names = list(boxes)
    e = ed.EditableGaussians(pc, boxes)
    for k, name in enumerate(names):
        e.edits[name] = all_groups(k)
    native = {field: torch.empty_like(getattr(pc, attr)) for attr, field in ed.EXPORT}  # stands in for the tracer's eight native tensors
    native_ns = type("Native", (), native)()
    params32 = er.as_params(pc, torch.float32, "cuda")
    objects = ed._as_int32([ed.pack_object(name, boxes[name], names) for name in names], 17)

    def fused_select():
        return torch.ops.egr.edit_select(pc._xyz, None, None, None, objects)

    slider = [0]

    def move_slider():  # one field of one edit changes: the frame is dirty
        slider[0] ^= 1
        e.edits["sphere0"].diffuse_hue_shift = 0.2 + 0.05 * slider[0]

    def fused_dirty():
        move_slider()
        e.export_edited(native_ns)

    def fused_clean():
        e.export_edited(native_ns)

    rotation = [0]

    def fused_launch():  # the launch alone, on the next of the rotating sets
        rotation[0] = (rotation[0] + 1) % len(sets)
        torch.ops.egr.edit_apply(sets[rotation[0]][0], sets[rotation[0]][1], e.selection_mask, records)

    def torch_select():
        return er.select(params32, boxes)

    selections = torch_select()

    def torch_dirty():
        move_slider()
        torch_apply()

    def torch_apply():
        out = er.edited(params32, selections, names, e.edits, boxes)
        torch._foreach_copy_([native[field] for _, field in ed.EXPORT], [out[attr] for attr, _ in ed.EXPORT])  # the eight export copies

    # the two paths compute the same thing: selections bit for bit, arrays to fp32 rounding of each array's largest entry
    assert torch.equal(fused_select(), er.mask_bits(selections, names)), "the selections differ"
    fused_clean()
    got = {attr: native[field].clone() for attr, field in ed.EXPORT}
    torch_apply()
    worst = {}
    for attr, field in ed.EXPORT:
        x, y = got[attr].double(), native[field].double()
        if attr == "_rotation":
            x, y = er.rotation_matrices(x), er.rotation_matrices(y)
        worst[attr] = float((x - y).abs().max() / y.abs().max())
    assert max(worst.values()) < 1e-4, worst
    result = dict(n=N, objects=len(names), reps=a.reps, inner=a.inner, inner_torch=a.inner_torch, sets=a.sets, device=torch.cuda.get_device_name(0), selected={k: int(v.sum()) for k, v in selections.items()},
                  fused_vs_torch_max_rel_diff=worst)

    records = e._device_records(pc._xyz.device)[0]
    sets = [([t.clone() for t in e._raw()], [torch.empty_like(t) for t in e._raw()]) for _ in range(a.sets)]
    result["launch_only_working_set_bytes"] = BYTES_PER_ROW * N * a.sets

    def window(fn, inner):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(inner):
            fn()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) / inner

    paths = {"select": (("fused", fused_select, a.inner), ("torch", torch_select, a.inner_torch)),
             "dirty_frame": (("fused", fused_dirty, a.inner), ("torch", torch_dirty, a.inner_torch)),
             "clean_frame": (("fused", fused_clean, a.inner),), "launch_only": (("fused", fused_launch, a.inner),)}
    for part, legs in paths.items():
        for _, fn, _ in legs:
            for _ in range(5):  # warm-ups of every shape
                fn()
        torch.cuda.synchronize()
        ts = {label: [] for label, _, _ in legs}
        for _ in range(a.reps):  # alternating: drifts of clock and temperature hit both paths alike
            for label, fn, inner in legs:
                ts[label].append(window(fn, inner))
        for label, _, _ in legs:
            result[f"{label}_{part}_ms"] = float(np.median(ts[label]))
            result[f"{label}_{part}_ms_min_max"] = [float(min(ts[label])), float(max(ts[label]))]
        if len(legs) == 2:
            result[f"torch_over_fused_{part}"] = result[f"torch_{part}_ms"] / result[f"fused_{part}_ms"]
    result["fused_launch_only_bytes_per_s"] = BYTES_PER_ROW * N / (result["fused_launch_only_ms"] * 1e-3)
    result["torch_dirty_frame_bytes_per_s_algorithmic"] = BYTES_PER_ROW * N / (result["torch_dirty_frame_ms"] * 1e-3)
    out = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out, exist_ok=True)
    for with_launches in (False, True):  # the timings are on disk before the profiler starts
        if with_launches:
            for part, legs in paths.items():  # launches: a pass of its own, after the timing
                for label, fn, _ in legs:
                    result[f"{label}_{part}_launches"] = count_kernels(fn)
        with open(os.path.join(out, "edit_bench.json"), "w") as f:
            json.dump(result, f, indent=1)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
