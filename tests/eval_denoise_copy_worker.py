"""tests/test_hip_eval.py: run as a fresh child process with EGR_DENOISE=0 (read when a context is created). A 37 x 19 tracer's denoise_views on random images
must then be a plain copy; prints one JSON line {"copy": bool, "shape": [...]}."""
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
PKG = "editable-gaussian-reflections_amd"

if __name__ == "__main__":
    import hip_common as hc

    syn, ren = importlib.import_module(PKG + ".synthetic"), importlib.import_module(PKG + ".renderer")
    rt = hc.tracer(ren, syn, W=37, H=19, N=300)
    g = torch.Generator(device="cuda").manual_seed(3)
    final = torch.rand(3, 19, 37, 3, device="cuda", generator=g) * 2
    normal = torch.randn(3, 3, 19, 37, 3, device="cuda", generator=g)
    out = rt.cuda_module.denoise_views(final, normal)
    torch.cuda.synchronize()
    print(json.dumps({"copy": bool(torch.equal(out, final)) and out.data_ptr() != final.data_ptr(), "shape": list(out.shape)}), flush=True)
