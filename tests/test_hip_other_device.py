"""Calls on tensors of a device that is NOT the current one (csrc/torch_binding.cpp takes a DeviceGuard for the tensors' device in every context-free op, and
for the tracer's device in every Raytracer method that reads the current stream, allocates or launches).

The context-free ops (include/egr_raytracer.h: CONTEXT-FREE FUNCTIONS): with device 0 current and the tensors on device 1, one op per family gives outputs
on device 1 that equal, bit for bit, the same call made with device 1 current, and leaves device 0 current. The sizes are the smallest that cross a wave (65 rows).

The Raytracer: a tracer built on device 1 runs its entry points once with device 1 current and, on a twin with the same seeds, with device 0 current: every
result is on device 1, device 0 stays current, the no-grad results are bit-equal and the gradients agree as two grad launches do (stream_order.GRAD_TOL).
32x16 pixels (two macro tiles), 300 gaussians (more than a wave), team help off (conftest.py). Both tests need two GPUs."""
import ctypes as C
import importlib

import numpy as np
import pytest

import stream_order as so
from hip_common import GRAD_KEYS, OUT_KEYS, cam_obj, generic_targets, ren, tracer, views  # noqa: F401 (fixture)

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
N, M = 65, 3


def families(dev):
    """name -> a call that returns the op's outputs as a list of tensors. Every input is on `dev`, from one seed."""
    ed = importlib.import_module(PKG + ".editing")
    ed.load_library()
    cabi = importlib.import_module(PKG + ".c_abi")
    ops = torch.ops.egr
    rng = np.random.default_rng(65)
    f32 = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dev)
    weight, points, rows, ids = f32(N).abs(), f32(N, 3), f32(N, 4), torch.arange(N, dtype=torch.int32).to(dev)
    cam_centers, cam_znear = f32(2, 3), torch.tensor([0.5, 0.25]).to(dev)
    tail = f32(M, 4)
    objects = ed._as_int32([ed.pack_object("box", {"min": [-0.5, -0.5, -0.5], "max": [0.5, 0.5, 0.5]}, ["box"])], C.sizeof(cabi.egr_edit_object) // 4)
    V, H, W = 1, 7, 9
    final, rgb, target = f32(V, H, W, 3).abs(), f32(V, 3, H, W, 3).abs(), f32(V, 3, H, W).abs()

    def prune():
        src_index, count = ops.prune_select(weight, 1.0, 0.5, points, cam_centers, cam_znear, None)
        k = int(count.item())
        assert 0 < k < N  # both criteria bite, and rows survive
        return [src_index[:k], count] + ops.prune_gather([rows, ids], src_index, k)

    def adam():
        param, grad, rt_param, rt_grad, m, v = f32(N, 3), f32(N, 3), torch.zeros(N, 3, device=dev), f32(N, 3), f32(N, 3), f32(N, 3).abs()
        ops.fused_adam_step([param], [grad], [rt_param], [rt_grad], [m], [v], [1e-2], [-1.0], [1.0], [1.0], 3, 0.9, 0.999, 1e-15)
        return [param, grad, rt_param, rt_grad, m, v]

    return {"prune_select + prune_gather": prune,
            "grow_append": lambda: ops.grow_append([rows, ids], [tail, None], [0, 7], M),
            "edit_select": lambda: [ops.edit_select(points, None, None, None, objects)],
            "fused_adam_step": adam,
            "distCUDA2": lambda: [torch.ops.simple_knn.distCUDA2(points)],
            "eval_metrics": lambda: list(ops.eval_metrics(final, rgb, target, target, None, True))}


@pytest.mark.gpu
def test_ops_run_on_their_tensors_device_and_leave_the_current_one():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    dev = torch.device("cuda", 1)
    with torch.cuda.device(1):
        want = {name: [t.cpu() for t in call()] for name, call in families(dev).items()}  # device 1 current: the ordinary case
        torch.cuda.synchronize()
    torch.cuda.set_device(0)
    for name, call in families(dev).items():
        got = call()
        assert torch.cuda.current_device() == 0, name
        assert len(got) == len(want[name])
        for k, (g, w) in enumerate(zip(got, want[name])):
            assert g.device == dev, (name, k, g.device)
            g = g.cpu()
            assert g.dtype == w.dtype and g.shape == w.shape, (name, k)
            assert np.array_equal(g.numpy().view(np.uint8), w.numpy().view(np.uint8)), (name, k)  # bit for bit (NaN included)
        assert torch.cuda.current_device() == 0, name


W, H, NG, V, K = 32, 16, 300, 2, 4
TARGET_ORDER = ("diffuse", "specular", "depth", "normal", "roughness", "f0")  # the order of set_targets_chw / raytrace(targets=...) / train_views
VIEW_OUTPUTS = ["final", "rgb", "depth", "normal", "f0", "roughness"]


def tracer_sequence(ren, syn, rt, dev, seeds=None):
    """The tracer's entry points in the order of a session, every device input on `dev`, whatever device is current. Asserts after every call that the current
    device is still the one it was and that every tensor handed back is on `dev`. Returns (no-grad results, gradients) as host arrays and the seeds used."""
    current = torch.cuda.current_device()
    m = rt.cuda_module
    fb, g, md = m.get_framebuffer(), m.get_gaussians(), m.get_metadata()
    if seeds is not None:
        md.random_seeds.copy_(seeds)
    exact, grads = {}, {}

    def keep(into, prefix, tensors):
        assert torch.cuda.current_device() == current, prefix
        for k, t in tensors.items():
            assert t.device == dev, (prefix, k, t.device)
            into[prefix + k] = t.clone()

    on = lambda a, dtype=torch.float32: torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(dev)
    cams = [cam_obj(ren, c) for c in views(syn, V)]
    Rs, centers = torch.stack([on(c.R.cpu()) for c in cams]).contiguous(), torch.stack([on(c.camera_center.cpu()) for c in cams]).contiguous()
    fovy = on([c.FoVy for c in cams])
    tg = generic_targets(syn, W, H)
    images = [on(tg[k]).moveaxis(-1, 0).contiguous() for k in TARGET_ORDER]
    stacks = [torch.stack([t, 0.5 * t]).contiguous() for t in images]
    row_bits = on(np.arange(NG) % 4, torch.int32)

    def fresh_grads():
        rt.zero_grad()
        g.total_weight.zero_()
        md.total_num_calls.fill_(K - 1)
        m.update_bvh(True)

    with torch.no_grad():
        rt._export_param_values()
        m.set_camera(Rs[0], centers[0], float(cams[0].FoVy), 0.01, 999.9)
        keep(exact, "set_camera.", {})
        m.set_targets_chw(*images)
        keep(exact, "set_targets_chw.", {"target_" + k: getattr(fb, "target_" + k) for k in TARGET_ORDER})
        md.total_num_calls.fill_(K - 1)
        m.update_bvh(True)
        keep(exact, "update_bvh.", {})
        m.raytrace()
        keep(exact, "raytrace.", {k: getattr(fb, k) for k in OUT_KEYS})
        m.denoise()
        keep(exact, "denoise.", {"output_denoised": fb.output_denoised})
        bufs = dict(zip(VIEW_OUTPUTS, m.render_views(Rs, centers, fovy, 0.01, 999.9, 1, VIEW_OUTPUTS)))
        keep(exact, "render_views.", bufs)
        keep(exact, "denoise_views.", {"denoised": m.denoise_views(bufs["final"], bufs["normal"])})
        keep(exact, "object_masks.", dict(zip(("masks", "hit", "top"), m.object_masks(Rs[0], centers[0], float(cams[0].FoVy), 0.01, 999.9, row_bits, [0, 1]))))
    fresh_grads()
    with torch.enable_grad():
        m.raytrace(None, images)
    keep(grads, "raytrace_targets.", {k: getattr(g, k) for k in GRAD_KEYS})
    fresh_grads()
    m.train_views(Rs, centers, fovy, 0.01, 999.9, *stacks)
    keep(grads, "train_views.", {k: getattr(g, k) for k in GRAD_KEYS})
    counters = m.get_counters()  # (synchronises)
    assert torch.cuda.current_device() == current and counters[11] == 0, counters
    exact["counters.rays"] = torch.tensor(counters[0:3])
    return so.to_host(exact), so.to_host(grads), md.random_seeds.clone()


def assert_same_session(got, want):
    for k in want[0]:
        assert np.array_equal(got[0][k].view(np.uint8), want[0][k].view(np.uint8)), k  # bit for bit
    assert float(np.abs(want[0]["raytrace.output_rgb"]).max()) > 0 and float(np.abs(want[0]["render_views.final"]).max()) > 0
    so.assert_same("tracer session", got[1], want[1], so.GRAD_TOL)


@pytest.mark.gpu
def test_a_tracer_runs_on_its_own_device_whatever_device_is_current(ren, syn):
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    dev = torch.device("cuda", 1)
    with torch.cuda.device(1):
        a, b = (tracer(ren, syn, W=W, H=H, N=NG, bwd=8_000_000) for _ in range(2))
        assert a.device == dev and b.device == dev
        want = tracer_sequence(ren, syn, a, dev)  # device 1 current: the ordinary case
        torch.cuda.synchronize()
    torch.cuda.set_device(0)
    got = tracer_sequence(ren, syn, b, dev, seeds=want[2])
    assert_same_session(got, want)
    # the Python callers build their tensors on the tracer's device: cameras and images of device 0 (camera_from_c2w's default) are moved
    tg = generic_targets(syn, W, H)
    cams = [cam_obj(ren, c, tg) for c in views(syn, V)]
    assert cams[0].R.device.index == 0 and cams[0].diffuse_image.device.index == 0
    b.zero_grad()
    ren.train_views(cams, b)
    assert torch.cuda.current_device() == 0
    grad = b.cuda_module.get_gaussians().dL_dmean
    assert grad.device == dev and float(grad.abs().max()) > 0
    shots = ren.render_views(cams, b)
    assert torch.cuda.current_device() == 0 and len(shots) == V
    for shot in shots:
        for k in ("final", "rgb", "depth", "normal", "roughness", "f0"):
            assert getattr(shot, k).device == dev, k
        assert float(shot.final.abs().max()) > 0
