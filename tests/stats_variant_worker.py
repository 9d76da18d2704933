"""tests/test_hip_stats_variant.py: one no-grad and one grad launch of hip_common.tracer's default scene (64x48, N = 3000, `trained`; 2 bounces, jitter off,
team help off) on whatever build the environment selects. The test calls `run()` in-process for the product and runs this file as a fresh child process
with EGR_TRAVERSAL_STATS=1 for the `stats` variant (two TORCH_LIBRARY(raytracer) shims cannot share a process): the child saves the arrays to argv[1]
and prints one JSON line {"version", "variant", "npz"}; the diagnostics it printed after each launch ([egr stats ...], stderr) follow a "=== <launch>" line."""
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "editable-gaussian-reflections_amd"
W, H = 64, 48


def run():
    """{launch: {name: array}} for launch in ("nograd", "grad"): the ten output buffers, both statistics images, random_seeds, the counters, the gradients."""
    import hip_common as hc

    syn, ren = importlib.import_module(PKG + ".synthetic"), importlib.import_module(PKG + ".renderer")
    torch.manual_seed(7)  # (random_seeds of a new tracer)
    rt = hc.tracer(ren, syn, W, H, bwd=8_000_000, team_help=False)
    m = rt.cuda_module
    m.get_config().jitter_primary_rays.fill_(False)
    m.get_config().num_bounces.fill_(2)
    cam = syn.default_camera()
    camera = hc.cam_obj(ren, cam, hc.generic_targets(syn, W, H))
    out = {}
    for launch in ("nograd", "grad"):
        m.get_metadata().total_num_calls.fill_(4)
        if launch == "grad":
            hc.run_grad(ren, rt, camera)
        else:
            with torch.no_grad():
                rt(camera)
        torch.cuda.synchronize()
        os.write(2, ("=== %s\n" % launch).encode())
        d = dict(hc.hip_outputs(rt), **hc.hip_grads(rt))
        d["counters"] = np.asarray(m.get_counters(), np.int64)  # (under EGR_PRINT_TRAVERSAL_STATS this prints the diagnostics of the launch)
        d["num_traversed_per_pixel"] = m.get_stats().num_traversed_per_pixel.cpu().numpy()
        d["num_accumulated_per_pixel"] = m.get_stats().num_accumulated_per_pixel.cpu().numpy()
        d["random_seeds"] = m.get_metadata().random_seeds.cpu().numpy()
        out[launch] = d
    return out


if __name__ == "__main__":
    os.environ["EGR_PRINT_TRAVERSAL_STATS"] = "1"
    res = run()
    np.savez(sys.argv[1], **{launch + "/" + k: v for launch, d in res.items() for k, v in d.items()})
    pkg, cabi = importlib.import_module(PKG), importlib.import_module(PKG + ".c_abi")
    print(json.dumps({"version": cabi.lib().egr_version().decode(), "variant": pkg.VARIANT, "npz": sys.argv[1]}), flush=True)
