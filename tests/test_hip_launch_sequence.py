"""The per-kernel stamps of a launch (egr_last_kernel_ms / Raytracer.last_kernel_ms): their names and their order for the four kinds of call. bench.py,
tools/views_bench.py, tools/train_views_bench.py and tools/launch_times.py key their per-kernel figures on exactly these."""
import pytest

from hip_common import cam_obj, generic_targets, ren, tracer, views  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H, V = 64, 48, 3  # three views in chunks of two frames: one full and one short chunk


@pytest.fixture(scope="module")
def timed(ren, syn):
    """(tracer with timing on, the cameras of V views with targets): 3000 gaussians of the trained-like scene, two bounces (the default)."""
    rt = tracer(ren, syn, W, H, bwd=8_000_000)
    rt.cuda_module.enable_timing(True)
    rt.cuda_module.set_batch_frames(2)
    tg = generic_targets(syn, W, H)
    return rt, [cam_obj(ren, c, tg) for c in views(syn, V)]


def stamp_names(rt):
    torch.cuda.synchronize()
    return [name for name, _ in rt.cuda_module.last_kernel_ms()]


def test_no_grad_render(ren, timed):
    rt, cams = timed
    with torch.no_grad():
        ren.render(cams[0], rt, targets_available=False)
    assert stamp_names(rt) == ["prologue+live", "forward_chain", "write_outputs"]


def test_grad_render(ren, timed):
    rt, cams = timed
    rt.zero_grad()
    ren.render(cams[0], rt)
    assert stamp_names(rt) == ["prologue+live", "forward_chain", "backward_chain", "backward_grad_gather"]


def test_render_views(ren, timed):
    rt, cams = timed
    ren.render_views(cams, rt, spp=1)
    assert stamp_names(rt) == ["prologue+live"] + ["forward_chain", "write_outputs"] * 2


def test_train_views(ren, timed):
    rt, cams = timed
    rt.zero_grad()
    ren.train_views(cams, rt)
    assert stamp_names(rt) == ["prologue+live"] + ["forward_chain", "backward_chain"] * 2 + ["backward_grad_gather"]
