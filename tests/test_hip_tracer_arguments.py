"""The argument rules of the Raytracer's methods (csrc/torch_binding.cpp: every strict tensor argument goes through tensor_arg, as the context-free ops' do).

Strict arguments - the eight tensors of update_bvh_from and of import_into, the six targets of raytrace and train_views_import, the buffers of
render_views_into, final / normal of denoise_views, row_bits of object_masks - are refused one at a time with each of four faults: fp64, a view that is not
contiguous, one dimension one too long, a CPU tensor. A refusal is a RuntimeError that names the method and the argument, comes before any launch and leaves
the tracer as it was: afterwards a no-grad launch is bit-equal to the same launch of a twin that never saw a refused call. The converting entries keep
converting: set_camera takes CPU fp64 tensors and set_targets_chw CPU fp32 ones, with the results of the GPU fp32 call.

32x16 pixels (two macro tiles of whole 8x8 tiles) and 300 gaussians (more than a wave); team help is off (conftest.py)."""
import numpy as np
import pytest

from fused_io_common import HOLDER_PARAMS, PARAM_ATTRS, bits, grads_of
from hip_common import OUT_KEYS, cam_obj, ren, torch, tracer, views  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

W, H, N, V, K = 32, 16, 300, 2, 4
TARGETS = (("diffuse", 3), ("specular", 3), ("depth", 1), ("normal", 3), ("roughness", 1), ("f0", 3))  # the order of set_targets_chw, raytrace(targets=) and train_views
VIEW_OUTPUTS = (("final", (V, H, W, 3)), ("rgb", (V, 3, H, W, 3)), ("depth", (V, 3, H, W, 1)), ("normal", (V, 3, H, W, 3)), ("f0", (V, 3, H, W, 3)), ("roughness", (V, 3, H, W, 1)))
FAULTS = {"fp64": lambda t: t.double(),
          "not_contiguous": lambda t: torch.stack([t, t], dim=-1)[..., 0],  # the same shape with every stride doubled
          "one_wrong_dimension": lambda t: torch.cat([t, t[..., :1]], dim=-1).contiguous(),
          "cpu": lambda t: t.cpu()}


def twins(ren, syn):
    """Two tracers on the same scene with the same seeds, camera bound and tree refitted; the model's .grad tensors exist (import_into adds to them)."""
    pair = []
    for _ in range(2):
        rt = tracer(ren, syn, W=W, H=H, N=N, bwd=8_000_000)
        for attr in PARAM_ATTRS:
            p = getattr(rt.pc, attr)
            p.grad = torch.zeros_like(p)
        pair.append(rt)
    a, b = pair
    b.cuda_module.get_metadata().random_seeds.copy_(a.cuda_module.get_metadata().random_seeds)
    cam = cam_obj(ren, syn.default_camera())
    for rt in pair:
        with torch.no_grad():
            rt._export_param_values()
            rt.cuda_module.set_camera(cam.R, cam.camera_center, float(cam.FoVy), 0.01, 999.9)
            rt.cuda_module.update_bvh(True)
    return a, b


def state_of(m):
    """Everything a no-grad launch writes, and the target buffers, as bits on the host."""
    fb, st, md = m.get_framebuffer(), m.get_stats(), m.get_metadata()
    out = {k: bits(getattr(fb, k)) for k in OUT_KEYS}
    out.update({"target_" + k: bits(getattr(fb, "target_" + k)) for k, _ in TARGETS})
    out.update(num_accumulated=st.num_accumulated_per_pixel.cpu(), num_traversed=st.num_traversed_per_pixel.cpu(), random_seeds=md.random_seeds.cpu(),
               total_num_calls=md.total_num_calls.cpu())
    return out


def launch_no_grad(m):
    m.get_metadata().total_num_calls.fill_(K - 1)
    with torch.no_grad():
        m.raytrace()
    torch.cuda.synchronize()
    assert m.get_counters()[11] == 0
    return state_of(m)


def refusals(ren, syn, rt):
    """(method, argument as the message names it, call(bad tensor)) for every strict tensor argument, with valid values in every other place."""
    m, g = rt.cuda_module, rt.cuda_module.get_gaussians()
    rng = np.random.default_rng(32)
    f32 = lambda *shape: torch.from_numpy(rng.random(shape, dtype=np.float32)).cuda()
    values = [getattr(g, k).clone() for k in HOLDER_PARAMS]
    grads = grads_of(rt.pc)
    images, stacks = [f32(c, H, W) for _, c in TARGETS], [f32(V, c, H, W) for _, c in TARGETS]
    cams = [cam_obj(ren, c) for c in views(syn, V)]
    R, centers = torch.stack([c.R for c in cams]).contiguous(), torch.stack([c.camera_center for c in cams]).contiguous()
    fovy = torch.tensor([c.FoVy for c in cams], dtype=torch.float32).cuda()
    buffers = [torch.zeros(shape, device="cuda") for _, shape in VIEW_OUTPUTS]
    final, normal = f32(V, H, W, 3), f32(V, 3, H, W, 3)
    row_bits = torch.ones(N, dtype=torch.int32, device="cuda")
    swap = lambda seq, k, bad: list(seq[:k]) + [bad] + list(seq[k + 1:])

    def grad_mode(call):
        def run(bad):
            with torch.enable_grad():
                call(bad)
        return run

    out = []
    for k, name in enumerate(HOLDER_PARAMS):
        out.append(("update_bvh_from", f"'{name}'", values[k], lambda bad, k=k: m.update_bvh_from(*swap(values, k, bad), True)))
        out.append(("raytrace", f"'{name}'", grads[k], grad_mode(lambda bad, k=k: m.raytrace(swap(grads, k, bad), None))))
        out.append(("train_views", f"'{name}'", grads[k], lambda bad, k=k: m.train_views_import(R, centers, fovy, 0.01, 999.9, *stacks, swap(grads, k, bad))))
    for k, (name, _) in enumerate(TARGETS):
        out.append(("raytrace", f"target '{name}'", images[k], grad_mode(lambda bad, k=k: m.raytrace(None, swap(images, k, bad)))))
        out.append(("train_views", f"target '{name}'", stacks[k], lambda bad, k=k: m.train_views_import(R, centers, fovy, 0.01, 999.9, *swap(stacks, k, bad), None)))
    for k, (name, _) in enumerate(VIEW_OUTPUTS):
        out.append(("render_views", f"output '{name}'", buffers[k],
                    lambda bad, k=k: m.render_views_into(R, centers, fovy, 0.01, 999.9, 1, [n for n, _ in VIEW_OUTPUTS], swap(buffers, k, bad))))
    out.append(("denoise_views", "final", final, lambda bad: m.denoise_views(bad, normal)))
    out.append(("denoise_views", "normal", normal, lambda bad: m.denoise_views(final, bad)))
    out.append(("denoise_views", "normal", normal[:, 0].contiguous(), lambda bad: m.denoise_views(final, bad)))  # the packed guide
    out.append(("object_masks", "row_bits", row_bits, lambda bad: m.object_masks(cams[0].R, cams[0].camera_center, float(cams[0].FoVy), 0.01, 999.9, bad, [0, 1])))
    return out


def test_every_strict_argument_is_refused_by_name_before_any_launch(ren, syn):
    a, b = twins(ren, syn)
    m = a.cuda_module
    before = state_of(m)
    held = [t.clone() for t in grads_of(a.pc)] + [getattr(m.get_gaussians(), k).clone() for k in HOLDER_PARAMS]
    tried = 0
    for method, argument, good, call in refusals(ren, syn, a):
        for fault, spoil in FAULTS.items():
            with pytest.raises(RuntimeError) as err:
                call(spoil(good))
            text = str(err.value)
            assert text.startswith(method + ": ") and argument in text.split(" must be ")[0] and " must be " in text, (method, argument, fault, text)
            tried += 1
    assert tried == (3 * 8 + 2 * 6 + 6 + 3 + 1) * len(FAULTS)
    torch.cuda.synchronize()
    after = state_of(m)
    for k in before:  # nothing was launched and nothing was written
        assert torch.equal(before[k], after[k]), k
    for t, t0 in zip(grads_of(a.pc) + [getattr(m.get_gaussians(), k) for k in HOLDER_PARAMS], held):
        assert torch.equal(bits(t), bits(t0))
    got, want = launch_no_grad(m), launch_no_grad(b.cuda_module)  # the twin never saw a refused call
    assert float(want["output_rgb"].view(torch.float32).abs().max()) > 0
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_the_converting_entries_still_convert(ren, syn):
    a, b = twins(ren, syn)
    cam = cam_obj(ren, views(syn, 2)[1])  # another pose than the bound one
    tg = syn.make_targets(W, H)
    images = [torch.tensor(tg[k]).moveaxis(-1, 0).contiguous() for k, _ in TARGETS]  # CPU fp32 [C,H,W]
    with torch.no_grad():
        a.cuda_module.set_camera(cam.R.cpu().double(), cam.camera_center.cpu().double(), float(cam.FoVy), 0.01, 999.9)
        a.cuda_module.set_targets_chw(*images)
        b.cuda_module.set_camera(cam.R, cam.camera_center, float(cam.FoVy), 0.01, 999.9)
        b.cuda_module.set_targets_chw(*[t.cuda() for t in images])
    for m in (a.cuda_module, b.cuda_module):
        m.update_bvh(True)
    got, want = launch_no_grad(a.cuda_module), launch_no_grad(b.cuda_module)
    assert float(want["target_diffuse"].view(torch.float32).abs().max()) > 0 and float(want["output_rgb"].view(torch.float32).abs().max()) > 0
    for k in want:
        assert torch.equal(got[k], want[k]), k
    with pytest.raises(RuntimeError) as err:  # ... and only the shape is refused: a pixel-major image must not be read as channel-major
        a.cuda_module.set_targets_chw(images[0].moveaxis(0, -1).contiguous(), None, None, None, None, None)
    assert "set_targets_chw" in str(err.value) and "target 'diffuse'" in str(err.value)
