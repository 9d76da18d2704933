"""Shared by the tests of the fused export / refit and gather / import passes (test_hip_fused_refit.py, test_hip_fused_import.py): one small cloud in
shuffled order with the three rows no ray can hit, tracers on it, a parameter drift, and bit-level comparisons that treat NaN as a value."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

W, H, N = 64, 48, 3001  # (N is no multiple of the 256-thread block; more than one block)
NAN_ROW, TRANSPARENT_ROW, COLLAPSED_ROW = 7, 19, 33
PARAM_ATTRS = ("_scaling", "_rotation", "_xyz", "_opacity", "_diffuse", "_normal", "_roughness", "_f0")  # the export order
HOLDER_PARAMS = ("scale", "rotation", "mean", "opacity", "rgb", "normal", "roughness", "f0")  # the same order, by the holder's names


def cloud(syn, n=N, seed=11):
    """n gaussians of the synthetic room in an order of their own (sorted position != id), among them a NaN mean, an opacity of -1e8 and a scale whose
    exponential underflows to 0: rows no ray can hit, which every pass still has to carry."""
    g = syn.make_scene(max(n, 64), "trained", seed=seed)
    perm = np.random.default_rng(seed).permutation(max(n, 64))[:n]
    g = {k: np.ascontiguousarray(v[perm]) for k, v in g.items()}
    if n > COLLAPSED_ROW:
        g["mean"][NAN_ROW, 1] = np.nan
        g["opacity"][TRANSPARENT_ROW] = -1e8
        g["scale"][COLLAPSED_ROW] = -200.0  # expf(-200) == 0
    return g


def tracer(ren, g, **kw):
    kw.setdefault("team_help", False)
    return ren.GaussianRaytracer(ren.GaussianParams(g), W, H, ppll_forward_size=8_000_000, ppll_backward_size=8_000_000, **kw)


def drift(pc, seed=3, amount=0.02):
    """The same small change of every parameter on every model it is applied to (generated on the host)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name in PARAM_ATTRS:
            p = getattr(pc, name)
            p.add_((amount * torch.randn(p.shape, generator=gen)).to(p.device))


def sources(pc):
    """What `_export_param_values` copies from, in the export order."""
    return [pc._get_scaling, pc._get_rotation, pc.get_xyz, pc._opacity, pc.get_diffuse, pc.get_normal, pc.get_roughness, pc.get_f0]


def grads_of(pc):
    return [getattr(pc, name).grad for name in PARAM_ATTRS]


def bits(t):
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    """Bit equality (a NaN equals the same NaN; -0 differs from +0)."""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool(torch.equal(a, b))


def bind_view(ren, syn, rt, targets=True):
    """Camera and targets of the room's default view, as `GaussianRaytracer.__call__` binds them. Returns the camera object."""
    cam = syn.default_camera()
    images = {k + "_image": torch.tensor(v).cuda().moveaxis(-1, 0).contiguous() for k, v in syn.make_targets(W, H).items()} if targets else {}
    camera = ren.camera_from_c2w(cam["origin"], cam["c2w"], cam["fov"], **images)
    m = rt.cuda_module
    with torch.no_grad():
        m.set_camera(camera.R, camera.camera_center, float(camera.FoVy), 0.01, 999.9)
        m.set_targets_chw(*[images.get(k + "_image") for k in ("diffuse", "specular", "depth", "normal", "roughness", "f0")])
    return camera
