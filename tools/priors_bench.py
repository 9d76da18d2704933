"""priors.prepare_prior_views against the same work as a sequence of stock torch ops on the same device and inputs: per view the point transform and projection
with the nearest-point rule (scatter_reduce amin), the pairs by boolean-mask indexing, 100 hypotheses (a closed-form fit through the sampled pairs, a residual
pass, a topk and a sum of squares each, with upstream's `error < best_error` test on the host), the refit, and the distance / normal / f0 images - written from
the description in include/egr_raytracer.h, not from upstream's text. A chunk is 8 views of 768 x 1365 with 5,000 and 20,000 points each; the images and points
are on the device before the clock starts. Both paths are checked against each other first ((a, b) of every view), then timed alternating in one process: medians
of --reps, host clock, every timed region between device synchronisations. The sequence upstream actually runs is on the CPU: the same torch sequence is timed
on this machine's host for ONE view and labelled as such.

Reports per point count: ms per chunk for both paths, kernel launches and per-kernel device time of the fused path (torch's profiler, in a pass of its own; from it
the share of k_prior_hypotheses, step 3), and the synchronising torch calls of each path (torch.cuda.set_sync_debug_mode("warn"), counted in a pass of its own):
for the fused path these are its uploads (camera rows, offsets, sample tables, sizes) and its ONE read-back, the pair counts.
Writes runs/<tag>/priors_bench.json (EGR_RUNS_DIR moves runs/).
Usage: python tools/priors_bench.py [--points 5000,20000] [--views 8] [--reps 7] [--size 768x1365] [--tag priors]"""
import argparse
import importlib
import json
import math
import os
import sys
import time
import warnings
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
priors = importlib.import_module("editable-gaussian-reflections_amd.priors")


def make_views(V, H, W, M, seed, dev):
    """V records with device images and their world-space points: M points per view at random pixels (collisions happen), the prediction (z - 0.25) / 2.1 under them
    with noise, 30 % of it off."""
    g = np.random.default_rng(seed)
    infos, points = [], []
    for _ in range(V):
        q, _ = np.linalg.qr(g.normal(size=(3, 3)))
        c2w = q * np.sign(np.linalg.det(q))
        w2c_R, w2c_t = c2w.T, -c2w.T @ g.normal(size=3)
        fovx = 1.0
        fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
        fx, fy, cx, cy = priors.intrinsics(fovx, fovy, H, W)
        pu, pv, pz = g.uniform(0, W - 1, M), g.uniform(0, H - 1, M), g.uniform(1.5, 6.0, M)
        cam = np.stack([(pu - cx) * pz / fx, (pv - cy) * pz / fy, pz], axis=1)
        world = ((cam - w2c_t) @ c2w.T).astype(np.float32)
        depth = g.uniform(0.3, 3.0, (H, W)).astype(np.float32)
        pred = (pz - 0.25) / 2.1 + g.normal(0, 0.004, M)
        off = g.random(M) < 0.3
        pred[off] += g.uniform(-1, 1, int(off.sum()))
        depth[np.rint(pv).astype(int), np.rint(pu).astype(int)] = pred.astype(np.float32)
        infos.append(SimpleNamespace(R=w2c_R.T.copy(), T=w2c_t.copy(), FovX=fovx, FovY=fovy, depth_image=torch.from_numpy(depth[:, :, None]).to(dev),
                                     normal_image=torch.from_numpy(g.normal(size=(H, W, 3)).astype(np.float32)).to(dev),
                                     metalness_image=torch.from_numpy(g.random((H, W, 1)).astype(np.float32)).to(dev)))
        points.append(torch.from_numpy(world).to(dev))
    return infos, points


def torch_view(info, pts, seed):
    """One view by stock torch ops on the device of its tensors; returns (a, b, distance, normals, f0)."""
    dev = pts.device
    depth0 = info.depth_image[:, :, 0]
    H, W = depth0.shape
    row = torch.from_numpy(priors.camera_rows([info], H, W)[0]).to(dev)
    w2c, (fx, fy, cx, cy), R = row[:12].reshape(3, 4), row[12:16], row[16:].reshape(3, 3)
    cam = pts @ w2c[:, :3].T + w2c[:, 3]
    x, y, z = cam.unbind(1)
    u, v = (x * fx / z + cx).round(), (y * fy / z + cy).round()
    keep = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    lin = (v * W + u)[keep].long()
    sparse = torch.full((H * W,), float("inf"), device=dev).scatter_reduce(0, lin, z[keep], "amin")
    valid = torch.isfinite(sparse) & torch.isfinite(depth0.reshape(-1))
    xs, ys = depth0.reshape(-1)[valid], sparse[valid]
    N = xs.shape[0]
    _, top_k = priors.fit_sizes(N)
    table = torch.from_numpy(priors.sample_table(N, seed=seed)).to(dev).long()

    def line(sx, sy):
        sx, sy = sx.double(), sy.double()
        mx, my = sx.mean(), sy.mean()
        w = ((sx - mx) * (sy - my)).sum() / ((sx - mx) ** 2).sum()
        return w.float(), (my - w * mx).float()

    best_error, best_idx = None, None
    for it in range(table.shape[0]):
        w, b = line(xs[table[it]], ys[table[it]])
        r = (ys - (w * xs + b)).abs()
        values, idx = torch.topk(r, top_k, largest=False)
        error = values.double().pow(2).sum()
        if best_error is None or error < best_error:  # upstream's test: the host waits for the device here
            best_error, best_idx = error, idx
    a, b = line(xs[best_idx], ys[best_idx])
    Z = depth0 * a + b
    uu, vv = torch.arange(W, device=dev).float()[None, :], torch.arange(H, device=dev).float()[:, None]
    X, Y = (uu - cx) * Z / fx, (vv - cy) * Z / fy
    distance = torch.sqrt(X * X + Y * Y + Z * Z)[:, :, None]
    n = -info.normal_image
    n = n / torch.sqrt((n * n).sum(-1, keepdim=True))
    m = info.metalness_image
    return a, b, distance, n @ R.T, (0.04 * (1.0 - m) + m).repeat(1, 1, 3)


def torch_chunk(infos, points, seed=0):
    return [torch_view(info, pts, seed + i) for i, (info, pts) in enumerate(zip(infos, points))]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def profiled(fn):
    """(kernel launches, {kernel name: device ms}) of one call."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
    per = {}
    for e in kernels:
        per[e.name] = per.get(e.name, 0.0) + e.device_time_total * 1e-3
    return len(kernels), per


def sync_calls(fn):
    """The synchronising torch calls of one call of fn, as torch's sync debug mode reports them."""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return sum(1 for w in seen if "synchroniz" in str(w.message).lower())


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--points", default="5000,20000")
    p.add_argument("--views", type=int, default=8)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--size", default="768x1365")
    p.add_argument("--tag", default="priors")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("priors_bench needs a GPU: nothing here is a measurement without one")
    H, W = (int(s) for s in a.size.split("x"))
    out = os.path.join(os.environ.get("EGR_RUNS_DIR", os.path.join(ROOT, "runs")), a.tag)
    os.makedirs(out, exist_ok=True)
    result = {"views": a.views, "height": H, "width": W, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    for M in (int(m) for m in a.points.split(",")):
        infos, points = make_views(a.views, H, W, M, 100 + M, "cuda")
        fused = lambda: priors.prepare_prior_views(infos, points, views_per_call=a.views)
        stock = lambda: torch_chunk(infos, points)
        recs, refs = fused(), stock()  # warm-up of every shape, and the check
        worst = max(max(abs(float(r.depth_fit.a) - float(t[0])) / abs(float(t[0])), abs(float(r.depth_fit.b) - float(t[1]))) for r, t in zip(recs, refs))
        if not worst < 1e-4:
            raise SystemExit(f"the two paths disagree: (a, b) differ by {worst:.3e}")
        ts = {"fused": [], "torch": []}
        for _ in range(a.reps):
            for label, fn in (("fused", fused), ("torch", stock)):
                ts[label].append(timed(fn)[0])
        row = {"points_per_view": M, "pairs_per_view": [r.depth_fit.num_pairs for r in recs], "ab_worst_difference": worst}
        for label in ts:
            row[f"{label}_ms_per_chunk"] = float(np.median(ts[label]))
            row[f"{label}_ms_min_max"] = [float(min(ts[label])), float(max(ts[label]))]
        row["torch_over_fused"] = row["torch_ms_per_chunk"] / row["fused_ms_per_chunk"]
        cpu_info = SimpleNamespace(**{k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in vars(infos[0]).items()})
        cpu_pts = points[0].cpu()
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            torch_view(cpu_info, cpu_pts, 0)
            cpu.append((time.perf_counter() - t0) * 1e3)
        row["torch_on_host_cpu_ms_per_VIEW"] = float(np.median(cpu))
        result[f"M{M}"] = row
        with open(os.path.join(out, "priors_bench.json"), "w") as f:  # the timings are on disk before the profiler starts
            json.dump(result, f, indent=1)
        row["fused_launches"], per = profiled(fused)
        row["fused_kernel_ms"] = per
        total = sum(per.values())
        row["hypotheses_share_of_kernel_time"] = sum(t for k, t in per.items() if "k_prior_hypotheses" in k) / total if total else None
        row["torch_launches"], _ = profiled(stock)
        row["fused_sync_calls"], row["torch_sync_calls"] = sync_calls(fused), sync_calls(stock)
        row["fused_readbacks"] = 1  # the pair counts of the chunk: priors._prepare_chunk
        with open(os.path.join(out, "priors_bench.json"), "w") as f:
            json.dump(result, f, indent=1)
        print(json.dumps(row), flush=True)
        del infos, points, recs, refs


if __name__ == "__main__":
    main()
