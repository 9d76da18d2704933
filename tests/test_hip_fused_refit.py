"""Export and refit in one pass (egr_update_bvh_from; Raytracer.update_bvh_from) against the two calls it replaces, and the backward record, which is
kept by gaussian id. Everything here is bit for bit: the fused pass runs the same expressions on the same values."""
import pytest

from fused_io_common import COLLAPSED_ROW, HOLDER_PARAMS, NAN_ROW, TRANSPARENT_ROW, bind_view, bits, cloud, drift, same_bits, sources, torch, tracer
from hip_common import OUT_KEYS, ren  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def holder_params(m):
    g = m.get_gaussians()
    return [getattr(g, k) for k in HOLDER_PARAMS]


def assert_exp_of(w, raw_scale):
    """w = expf(raw_scale) as the device evaluates it: within 2 ulps of the correctly rounded value (the library function's documented 1 ulp and the
    rounding of the fp64 reference itself); an underflowing exponential is exactly 0."""
    want = torch.exp(raw_scale.detach().cpu().double())
    err = (w.double() - want).abs()
    assert bool((err <= 2.0 * 2.0 ** -23 * want + 1e-45).all()), float((err / want.clamp_min(1e-300)).max())


def refit_pair(ren, syn, n, fuse_live=True):
    """Two tracers on the same cloud after the same drift: `a` exports and refits in two calls, `b` in one."""
    g = cloud(syn, n)
    a, b = tracer(ren, g), tracer(ren, g)
    for rt in (a, b):
        drift(rt.pc)
        bind_view(ren, syn, rt, targets=False)
    a._export_param_values()
    a.cuda_module.update_bvh(fuse_live)
    b.cuda_module.update_bvh_from(*sources(b.pc), fuse_live)
    return a, b


def assert_same_state(a, b):
    ma, mb = a.cuda_module, b.cuda_module
    for name, src, held in zip(HOLDER_PARAMS, sources(b.pc), holder_params(mb)):
        assert same_bits(held, src), name  # the holder holds the sources ...
    for name, x, y in zip(HOLDER_PARAMS, holder_params(ma), holder_params(mb)):
        assert same_bits(x, y), name  # ... which is what the eight copies leave
    for name, x, y in zip(("M", "W", "aabb"), ma.debug_instances(), mb.debug_instances()):
        assert same_bits(x, y), name
    assert same_bits(ma.debug_backward_records(), mb.debug_backward_records())
    assert ma.check_bvh() == 0 and mb.check_bvh() == 0, (ma.last_error(), mb.last_error())
    with torch.no_grad():
        ma.raytrace()
        mb.raytrace()
    fa, fb = ma.get_framebuffer(), mb.get_framebuffer()
    for k in OUT_KEYS:
        assert same_bits(getattr(fa, k), getattr(fb, k)), k
    for k in ("num_accumulated_per_pixel", "num_traversed_per_pixel"):
        assert torch.equal(getattr(ma.get_stats(), k), getattr(mb.get_stats(), k)), k
    assert torch.equal(ma.get_metadata().random_seeds, mb.get_metadata().random_seeds)


@pytest.mark.parametrize("fuse_live", [True, False], ids=["fuse_live", "plain"])
def test_one_pass_leaves_what_export_and_update_leave(ren, syn, fuse_live):
    a, b = refit_pair(ren, syn, 3001, fuse_live)
    assert_same_state(a, b)
    held = holder_params(b.cuda_module)
    assert bool(torch.isnan(held[2][NAN_ROW, 1])) and float(held[3][TRANSPARENT_ROW]) < -9e7 and float(held[0][COLLAPSED_ROW].max()) < -150  # the three rows went through
    assert int(b.cuda_module.get_stats().num_accumulated_per_pixel.max()) > 0  # (something was hit)


def test_a_single_gaussian(ren, syn):
    assert_same_state(*refit_pair(ren, syn, 1))


def test_the_holder_as_its_own_source(ren, syn):
    g = cloud(syn)
    a, b = tracer(ren, g), tracer(ren, g)
    for rt in (a, b):
        drift(rt.pc)
        bind_view(ren, syn, rt, targets=False)
        rt._export_param_values()
    a.cuda_module.update_bvh(True)
    before = [t.clone() for t in holder_params(b.cuda_module)]
    b.cuda_module.update_bvh_from(*holder_params(b.cuda_module), True)
    for name, x, y in zip(HOLDER_PARAMS, before, holder_params(b.cuda_module)):
        assert same_bits(x, y), name
    assert_same_state(a, b)


def test_the_renderer_takes_the_one_pass_and_falls_back(ren, syn):
    g = cloud(syn)
    a, b = tracer(ren, g), tracer(ren, g)
    for rt in (a, b):
        drift(rt.pc)
    camera = bind_view(ren, syn, a)
    bind_view(ren, syn, b)
    a._export_param_values()
    a.cuda_module.update_bvh(True)
    calls = []
    b._export_param_values = lambda: calls.append("export")  # (the instance's own: a fused call never gets here)
    with torch.no_grad():
        a.cuda_module.raytrace()
        b(camera, force_update_bvh=True)
    assert calls == []
    for k in OUT_KEYS:
        assert same_bits(getattr(a.cuda_module.get_framebuffer(), k), getattr(b.cuda_module.get_framebuffer(), k)), k
    for rt in (a, b):  # a training call (grad mode, nothing forced) refits from the model's current values too
        drift(rt.pc, seed=4)
    a._export_param_values()
    a.cuda_module.update_bvh(True)
    with torch.enable_grad():
        b(camera)
    assert calls == []
    for name, x, y in zip(("M", "W", "aabb"), a.cuda_module.debug_instances(), b.cuda_module.debug_instances()):
        assert same_bits(x, y), name
    for name, x, y in zip(HOLDER_PARAMS, holder_params(a.cuda_module), holder_params(b.cuda_module)):
        assert same_bits(x, y), name
    del b._export_param_values
    b.pc._xyz = b.pc._xyz.t().contiguous().t()  # a getter the native checks refuse (same values, other strides): the two calls
    exported = []
    plain = b._export_param_values
    b._export_param_values = lambda: (exported.append(1), plain())
    with torch.no_grad():
        b(camera, force_update_bvh=True)
    assert exported == [1]
    assert not b.pc._xyz.is_contiguous() and same_bits(b.cuda_module.get_gaussians().mean, b.pc._xyz.contiguous())


def test_refused_arguments_raise_before_any_launch(ren, syn):
    rt = tracer(ren, cloud(syn))
    m = rt.cuda_module
    drift(rt.pc)
    good = sources(rt.pc)
    before = [t.clone() for t in holder_params(m)]
    records = m.debug_backward_records()
    bad = {"shape": lambda t: t[:-1].contiguous(), "dtype": lambda t: t.double(), "device": lambda t: t.cpu(), "strides": lambda t: t.t().contiguous().t()}
    for what, spoil in bad.items():
        for k in (0, 1, 2, 7):  # scale, rotation, mean, f0
            args = list(good)
            args[k] = spoil(args[k])
            assert what != "strides" or (args[k].shape == good[k].shape and not args[k].is_contiguous())
            with pytest.raises(RuntimeError, match="update_bvh_from"):
                m.update_bvh_from(*args, True)
    with pytest.raises(RuntimeError, match="16-byte"):
        m.update_bvh_from(good[0], torch.zeros(4 * 3001 + 1, device="cuda")[1:].view(3001, 4), *good[2:], True)
    torch.cuda.synchronize()
    for name, x, y in zip(HOLDER_PARAMS, before, holder_params(m)):
        assert same_bits(x, y), name  # nothing was exported ...
    assert same_bits(records, m.debug_backward_records())  # ... and nothing refitted
    m.update_bvh_from(*good, True)  # the tracer is as usable as before
    assert m.check_bvh() == 0


def test_backward_record_is_kept_by_id_and_its_live_part_follows_the_parameters(ren, syn):
    """Scale and rotation change WITHOUT a refit, then a grad launch: rows 0-2 keep the snapshot's M, their fourth components are exp of the current scale
    and row 3 is the current raw quaternion - each at the gaussian's id, whatever its sorted position."""
    rt = tracer(ren, cloud(syn))
    m = rt.cuda_module
    bind_view(ren, syn, rt)
    rt._export_param_values()
    m.update_bvh(False)  # (plain: the launch below must read the live parameters itself)
    snapshot = m.debug_instances()[0]  # [n,3,4] by id; column 3 carries the mean there
    rec0 = m.debug_backward_records()
    assert same_bits(rec0[:, :3, :3], snapshot[:, :, :3])
    assert_exp_of(rec0[:, :3, 3], rt.pc._scaling)
    assert same_bits(rec0[:, 3], rt.pc._rotation)
    with torch.no_grad():
        rt.pc._scaling.add_(0.05)
        rt.pc._rotation.mul_(1.5).add_(0.01)
    rt._export_param_values()
    with torch.enable_grad():
        m.raytrace()
    rec = m.debug_backward_records()
    assert same_bits(rec[:, :3, :3], snapshot[:, :, :3])  # the snapshot stays
    assert not torch.equal(bits(rec[:, :3, 3]), bits(rec0[:, :3, 3]))
    assert_exp_of(rec[:, :3, 3], rt.pc._scaling)
    assert float(rec[COLLAPSED_ROW, :3, 3].abs().max()) == 0.0
    assert same_bits(rec[:, 3], rt.pc._rotation)


def test_an_empty_cloud_has_nothing_to_export_or_import(ren, syn):
    """n = 0: the model's tensors have no storage (NULL pointers), which both fused entries accept - nothing is read."""
    rt = tracer(ren, {k: v[:0] for k, v in cloud(syn, 64).items()})
    m = rt.cuda_module
    camera = bind_view(ren, syn, rt)
    assert m.get_gaussians().mean.shape[0] == 0
    with torch.enable_grad():
        rt(camera)
    with torch.no_grad():
        rt(camera, force_update_bvh=True)
    c = m.get_counters()
    assert c[11] == 0 and c[0] == 64 * 48
    assert float(m.get_framebuffer().output_final.abs().max()) == 0.0
    assert not bool(m.get_stats().num_accumulated_per_pixel.any()) and not bool(m.get_stats().num_traversed_per_pixel.any())
