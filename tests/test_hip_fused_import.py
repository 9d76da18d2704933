"""Gather and import in one pass (egr_raytrace_import, egr_train_views_import; Raytracer.raytrace(import_into=...)) against the launch followed by the
multi-tensor add it replaces, and the per-pixel statistics of launches that no longer clear them first.

What is exact: the import itself. The kernel adds to the caller's tensor the very value it has just stored in the holder's, so after ANY launch
caller_after == caller_before + holder_after, bit for bit - the sum `_foreach_add_(caller, holder)` computes from the same two numbers. Two LAUNCHES of a
grad pass differ by the order of their float atomics (tests/test_hip_parity.py: "the atomics' order is the only freedom"), fused or not: on this cloud
(3001 gaussians, 64x48, two bounces) two tracers that both run launch + add differ in 3910-4240 of the 63021 holder gradient elements, a fused against an
unfused one in 4170-4420 (the REPORT line prints both). So two tracers are held to the suite's bar for two launches, 1e-5 of a tensor's largest
magnitude, and the fused arithmetic to bit equality on the launch that ran it."""
import numpy as np
import pytest

from fused_io_common import H, HOLDER_PARAMS, N, PARAM_ATTRS, W, bind_view, bits, cloud, grads_of, same_bits, torch, tracer
from hip_common import cam_obj, make_pair, mismatch_list, ren, report, views  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu


def holder_grads(m):
    g = m.get_gaussians()
    return [getattr(g, k).grad for k in HOLDER_PARAMS]


def prefill_grads(pc, seed=21):
    """The model's .grad tensors start from values of their own (an import ADDS)."""
    gen = torch.Generator().manual_seed(seed)
    for name in PARAM_ATTRS:
        p = getattr(pc, name)
        p.grad = torch.randn(p.shape, generator=gen).to(p.device)


def ready(ren, syn, n=N, **kw):
    rt = tracer(ren, cloud(syn, n), **kw)
    prefill_grads(rt.pc)
    bind_view(ren, syn, rt)
    rt._export_param_values()
    return rt


def launch(rt, fused):
    """One grad launch and the import of its gradients. Returns what the identity needs: the caller's gradients before, the holder's after."""
    m = rt.cuda_module
    m.update_bvh(True)
    before = [t.clone() for t in grads_of(rt.pc)]
    with torch.enable_grad():
        if fused:
            m.raytrace(grads_of(rt.pc))
        else:
            m.raytrace()
            rt._import_param_gradients()
    torch.cuda.synchronize()
    return before, [t.clone() for t in holder_grads(m)]


def assert_import_identity(rt, before, held):
    for name, b, h, now in zip(PARAM_ATTRS, before, held, grads_of(rt.pc)):
        assert same_bits(now, b + h), name


def differing(xs, ys):
    return sum(int((bits(x) != bits(y)).sum()) for x, y in zip(xs, ys))


def assert_same_up_to_the_order_of_atomics(xs, ys, names):
    """The suite's bar for two grad launches of the same rays (tests/test_hip_parity.py, tests/test_c_abi_direct.py): 1e-5 of the tensor's largest
    magnitude. NaN stays NaN at the same places."""
    for name, x, y in zip(names, xs, ys):
        x, y = x.detach().cpu().double(), y.detach().cpu().double()
        assert torch.equal(torch.isnan(x), torch.isnan(y)), name
        x, y = torch.nan_to_num(x), torch.nan_to_num(y)
        assert float((x - y).abs().max()) <= 1e-5 * max(float(y.abs().max()), 1e-30), name


# n = 3001: the holder's gradient tensors start 3n, 6n, ... floats into one buffer, so all but the first are off 16-byte alignment and the import adds them
# float by float. n = 3004 (a multiple of 4, not of the 256-thread block): all eight are aligned, as at the benchmark's 1 M - float4 lines for the eleven
# whole blocks of every tensor, floats for the last, partial one.
@pytest.mark.parametrize("n", [N, 3004])
def test_fused_import_is_the_launch_followed_by_the_add(ren, syn, n):
    a, b, c = ready(ren, syn, n), ready(ren, syn, n), ready(ren, syn, n)  # a, c: launch + add; b: one pass
    if n == 3004:
        hg = b.cuda_module.get_gaussians()
        assert all(getattr(hg, k).grad.data_ptr() % 16 == 0 for k in HOLDER_PARAMS) and all(t.data_ptr() % 16 == 0 for t in grads_of(b.pc))
    for second in (False, True):  # the second launch follows without zero_grad: the holder's accumulated value is imported again, as by the add
        ra, rb, rc = launch(a, False), launch(b, True), launch(c, False)
        assert_import_identity(a, *ra)
        assert_import_identity(b, *rb)  # exact: the fused arithmetic
        untouched = [(h == 0).all(dim=1) if not second else None for h in rb[1]]
        report("fused_import", second_launch=second, holder_elements_differing_fused_vs_unfused=differing(ra[1], rb[1]),
               holder_elements_differing_unfused_vs_unfused=differing(ra[1], rc[1]), caller_elements_differing_fused_vs_unfused=differing(grads_of(a.pc), grads_of(b.pc)))
        assert_same_up_to_the_order_of_atomics(rb[1], ra[1], HOLDER_PARAMS)
        assert_same_up_to_the_order_of_atomics(grads_of(b.pc), grads_of(a.pc), PARAM_ATTRS)
        if not second:  # rows the launch did not reach (holder gradient still zero): the caller keeps its value, bit for bit, on both paths
            for name, rows, before, now_a, now_b in zip(PARAM_ATTRS, untouched, rb[0], grads_of(a.pc), grads_of(b.pc)):
                assert int(rows.sum()) > 0 and same_bits(now_b[rows], before[rows]) and same_bits(now_a[rows], before[rows]), name
        wa, wb = a.cuda_module.get_gaussians().total_weight, b.cuda_module.get_gaussians().total_weight
        assert_same_up_to_the_order_of_atomics([wb], [wa], ["total_weight"])
        assert float(wb.sum()) > 0
    assert int(a.cuda_module.get_metadata().total_num_calls) == int(b.cuda_module.get_metadata().total_num_calls) == 2


def test_the_renderer_imports_in_the_launch(ren, syn):
    a, b = ready(ren, syn), ready(ren, syn)
    camera = bind_view(ren, syn, a)
    a.import_grads = False  # a: the launch, then the add by hand
    before = [t.clone() for t in grads_of(b.pc)]
    added = []
    plain = b._import_param_gradients
    b._import_param_gradients = lambda: (added.append(1), plain())
    with torch.enable_grad():
        a(camera, **{k: getattr(camera, k.replace("target_", "") + "_image") for k in ("target_diffuse", "target_specular", "target_depth", "target_normal", "target_roughness", "target_f0")})
        b(camera, **{k: getattr(camera, k.replace("target_", "") + "_image") for k in ("target_diffuse", "target_specular", "target_depth", "target_normal", "target_roughness", "target_f0")})
    a._import_param_gradients()
    torch.cuda.synchronize()
    assert added == []  # the launch did it
    assert_import_identity(b, before, holder_grads(b.cuda_module))
    assert_same_up_to_the_order_of_atomics(grads_of(b.pc), grads_of(a.pc), PARAM_ATTRS)


def test_a_partitioned_tracer_never_imports_in_the_launch(ren, syn):
    rt = ready(ren, syn, rank=0, world_size=2)  # set_partition(0, 2), use_grad_delta(True)
    m = rt.cuda_module
    assert m.get_gaussians().grad_delta.numel() == 22 * N
    assert rt._import_target() is None
    before = [t.clone() for t in grads_of(rt.pc)]
    m.update_bvh(True)
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match="per-launch"):
            m.raytrace(grads_of(rt.pc))
    torch.cuda.synchronize()
    for name, x, y in zip(PARAM_ATTRS, before, grads_of(rt.pc)):
        assert same_bits(x, y), name
    assert int(m.get_metadata().total_num_calls) == 0  # refused before anything ran


def test_refused_import_targets(ren, syn):
    rt = ready(ren, syn)
    m = rt.cuda_module
    good = grads_of(rt.pc)
    m.update_bvh(True)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="grad mode"):
            m.raytrace(good)
    with torch.enable_grad():
        for spoil in (lambda t: t[:-1].contiguous(), lambda t: t.double(), lambda t: t.cpu(), lambda t: t.t().contiguous().t()):
            args = list(good)
            args[2] = spoil(args[2])
            with pytest.raises(RuntimeError, match="raytrace"):
                m.raytrace(args)
        with pytest.raises(RuntimeError, match="eight tensors"):
            m.raytrace(good[:7])
        with pytest.raises(RuntimeError, match="bound gradient tensors"):
            m.raytrace(holder_grads(m))
    assert int(m.get_metadata().total_num_calls) == 0


def test_train_views_imports_in_its_one_gather(ren, syn):
    tg = syn.make_targets(W, H)
    cams = [cam_obj(ren, c, tg) for c in views(syn, 2)]
    a, b = ready(ren, syn), ready(ren, syn)
    a.import_grads = False
    before = [t.clone() for t in grads_of(b.pc)]
    ren.train_views(cams, a)
    a._import_param_gradients()
    ren.train_views(cams, b)
    torch.cuda.synchronize()
    assert_import_identity(b, before, holder_grads(b.cuda_module))
    assert_same_up_to_the_order_of_atomics(grads_of(b.pc), grads_of(a.pc), PARAM_ATTRS)
    assert_same_up_to_the_order_of_atomics(holder_grads(b.cuda_module), holder_grads(a.cuda_module), HOLDER_PARAMS)
    assert int(a.cuda_module.get_metadata().total_num_calls) == int(b.cuda_module.get_metadata().total_num_calls) == 2
    assert float(b.cuda_module.get_gaussians().total_weight.sum()) > 0


# ---- per-pixel statistics: a whole-image launch without a mask stores every pixel and clears nothing first; every other launch clears as before

def stats_of(m):
    st = m.get_stats()
    torch.cuda.synchronize()
    return st.num_accumulated_per_pixel.cpu().numpy().copy(), st.num_traversed_per_pixel.cpu().numpy().copy()


def test_statistics_whole_image_partition_mask_and_no_stale_counts(ren, orc, syn, pkg):
    import importlib

    par = importlib.import_module(pkg.__name__ + ".parallel")
    g = cloud(syn)
    cam = syn.default_camera()
    rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(num_bounces=2), team_help=False)
    m = rt.cuda_module
    camera = cam_obj(ren, cam)
    m.set_exact_stats(True)  # (num_traversed is then the oracle's number: egr_set_exact_stats)

    def render(k=0):
        m.get_metadata().total_num_calls.fill_(k)
        with torch.no_grad():
            rt(camera, force_update_bvh=True)
        return stats_of(m)

    def launch_only(k=0):
        m.get_metadata().total_num_calls.fill_(k)
        with torch.no_grad():
            m.raytrace()
        return stats_of(m)

    acc, trav = render()
    o.total_num_calls = 0
    ref = o.raytrace(False)
    bad_a, n_a = mismatch_list(acc, ref["num_accumulated"])
    bad_t, n_t = mismatch_list(trav, ref["num_traversed"])
    report("stats_vs_oracle", accumulated_mismatches=n_a, traversed_mismatches=n_t, of=W * H, first=bad_a[:4] + bad_t[:4])
    # bounce rays differ by ulps between the two implementations, so the counts of the bounce steps agree statistically: the bars of
    # test_exact_stats_mode_counts_reference_invocations (tests/test_hip_parity.py) for a launch with bounces
    assert n_t <= 0.02 * W * H and n_a <= 0.02 * W * H, (n_t, n_a)
    assert abs(int(trav.sum()) - int(ref["num_traversed"].sum())) <= 2e-3 * int(ref["num_traversed"].sum())
    assert int(acc.max()) > 0 and int(trav.max()) > 0
    # the same launch on the clearing path (a mask of ones: every pixel traced, both images cleared first) - bit for bit
    m.debug_set_pixel_mask(torch.ones(H * W, dtype=torch.uint8, device="cuda"))
    try:
        acc1, trav1 = launch_only()
    finally:
        m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
    assert np.array_equal(acc, acc1) and np.array_equal(trav, trav1)
    # a rank of two: its own pixels as in the whole image, foreign tiles 0 (the images held the whole launch's counts a moment ago)
    own = par.owner_map(W, H, 2) == 1
    m.set_partition(1, 2)
    try:
        acc2, trav2 = launch_only()
    finally:
        m.set_partition(0, 1)
    assert 0 < int(own.sum()) < W * H
    assert not acc2[~own].any() and not trav2[~own].any()
    assert np.array_equal(acc2[own], acc[own]) and np.array_equal(trav2[own], trav[own])
    # a pixel mask: masked pixels 0
    acc, trav = launch_only()  # (whole image again: every count is back)
    keep = np.random.default_rng(5).random((H, W)) < 0.5
    m.debug_set_pixel_mask(torch.from_numpy(keep.astype(np.uint8)).cuda())
    try:
        acc3, trav3 = launch_only()
    finally:
        m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
    assert not acc3[~keep].any() and not trav3[~keep].any()
    assert np.array_equal(acc3[keep], acc[keep]) and np.array_equal(trav3[keep], trav[keep])
    # after a launch with more hits per pixel, one with fewer: half of the cloud turns transparent. Every pixel holds this launch's count, not the last
    # one's - the same launch on the clearing path (a mask of ones) says which that is, bit for bit
    with torch.no_grad():
        rt.pc._opacity[::2] = -1e8
    acc5, trav5 = render()
    report("stats_fewer_hits", pixels_with_fewer_composited=int((acc5 < acc).sum()), pixels_with_fewer_candidates=int((trav5 < trav).sum()), pixels_still_hit=int((acc5 > 0).sum()), of=W * H)
    assert int((acc5 < acc).sum()) > 0 and int((trav5 < trav).sum()) > W * H // 8 and int((acc5 > 0).sum()) > W * H // 4 and int(trav5.sum()) < int(trav.sum())
    m.debug_set_pixel_mask(torch.ones(H * W, dtype=torch.uint8, device="cuda"))
    try:
        acc6, trav6 = launch_only()
    finally:
        m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
    assert np.array_equal(acc5, acc6) and np.array_equal(trav5, trav6)
    # ... and a cloud nothing can hit: no count of the earlier launch is left, although nothing was cleared
    acc, trav = launch_only()
    assert int((acc > 0).sum()) > W * H // 2
    with torch.no_grad():
        rt.pc._opacity.fill_(-1e8)
    acc4, trav4 = render()
    assert not acc4.any() and not trav4.any()
