"""The context-free ops on tensors of a device that is NOT the current one (include/egr_raytracer.h: CONTEXT-FREE FUNCTIONS; csrc/torch_binding.cpp takes a
DeviceGuard for the tensors' device in every op): with device 0 current and the tensors on device 1, one op per family gives outputs on device 1 that equal,
bit for bit, the same call made with device 1 current, and leaves device 0 current. Needs two GPUs; the sizes are the smallest that cross a wave (65 rows)."""
import ctypes as C
import importlib

import numpy as np
import pytest

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
