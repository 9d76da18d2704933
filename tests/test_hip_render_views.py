"""Batched no-grad render (egr_render_views / Raytracer.render_views / renderer.render_views): V views x S samples in as few launches as the
ray state allows, held against what the single-frame path gives for the same frames (include/egr_raytracer.h: egr_view_batch)."""
import importlib

import numpy as np
import pytest

from hip_common import BOTH_HELP_MODES, cam_obj, make_pair, psnr, ren, report, tracer, views  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PKG = "editable-gaussian-reflections_amd"
FIELDS = ("final", "rgb", "depth", "normal", "roughness", "f0")


def sequential(ren, rt, cams, S, base):
    """The contract's reference: per view reset_accumulators() + S no-grad launches with accumulate_samples = (S > 1)."""
    m = rt.cuda_module
    m.get_metadata().total_num_calls.fill_(base)
    m.get_config().accumulate_samples.fill_(S > 1)
    out = []
    try:
        for c in cams:
            m.reset_accumulators()
            with torch.no_grad():
                for _ in range(S):
                    r = ren.render(c, rt, targets_available=False)
            out.append({k: getattr(r, k) for k in FIELDS})
    finally:
        m.get_config().accumulate_samples.fill_(False)
    torch.cuda.synchronize()
    return out


def batched(ren, rt, cams, S, base):
    rt.cuda_module.get_metadata().total_num_calls.fill_(base)
    vs = ren.render_views(cams, rt, spp=S)
    torch.cuda.synchronize()
    return [{k: getattr(v, k) for k in FIELDS} for v in vs]


def assert_views_equal(a, b, what):
    for v, (x, y) in enumerate(zip(a, b)):
        for k in FIELDS:
            assert x[k].shape == y[k].shape, (what, v, k, x[k].shape, y[k].shape)
            assert torch.equal(x[k], y[k]), (what, v, k, int((x[k] != y[k]).sum()))


@pytest.mark.parametrize("jitter", [False, True], ids=["jitter_off", "jitter_on"])
def test_multi_view_equals_sequential_renders(ren, syn, jitter):
    rt = tracer(ren, syn)
    m = rt.cuda_module
    m.get_config().num_bounces.fill_(2)
    m.get_config().jitter_primary_rays.fill_(jitter)
    cams = [cam_obj(ren, c) for c in views(syn, 3)]
    seq = sequential(ren, rt, cams, 1, 40)
    bat = batched(ren, rt, cams, 1, 40)
    assert_views_equal(bat, seq, "V=3 S=1")
    assert bat[0]["final"].shape == (1, 3, 48, 64) and bat[0]["rgb"].shape == (3, 3, 48, 64) and bat[0]["depth"].shape == (3, 1, 48, 64)
    assert not torch.equal(bat[0]["final"], bat[1]["final"]) and float(bat[2]["final"].abs().sum()) > 0  # three different images
    assert int(m.get_counters()[11]) == 0


def test_multi_sample_equals_accumulated_launches(ren, syn):
    rt = tracer(ren, syn)
    rt.cuda_module.get_config().jitter_primary_rays.fill_(True)
    cams = [cam_obj(ren, c) for c in views(syn, 2)]
    seq = sequential(ren, rt, cams, 8, 7)
    bat = batched(ren, rt, cams, 8, 7)
    assert_views_equal(bat, seq, "V=2 S=8")
    one = batched(ren, rt, cams[:1], 1, 7)  # the average of 8 jittered samples is not one sample
    assert not torch.equal(one[0]["final"], bat[0]["final"])


def test_chunk_boundaries_inside_views_change_nothing(ren, syn):
    rt = tracer(ren, syn)
    m = rt.cuda_module
    m.get_config().jitter_primary_rays.fill_(True)
    cams = [cam_obj(ren, c) for c in views(syn, 3)]
    m.set_batch_frames(3)  # 15 frames in chunks of 3: every view spans a chunk boundary
    small = batched(ren, rt, cams, 5, 100)
    m.set_batch_frames(16)
    whole = batched(ren, rt, cams, 5, 100)
    assert_views_equal(small, whole, "chunks of 3 vs one chunk")
    assert_views_equal(small, sequential(ren, rt, cams, 5, 100), "chunks of 3 vs sequential")


def test_side_effects_match_the_sequential_launches(ren, syn):
    rt = tracer(ren, syn)
    m = rt.cuda_module
    m.get_config().jitter_primary_rays.fill_(True)
    cams = [cam_obj(ren, c) for c in views(syn, 2)]
    probe = cam_obj(ren, views(syn, 4)[3])
    V, S, base = 2, 3, 11
    fb, md, st = m.get_framebuffer(), m.get_metadata(), m.get_stats()
    names = list(ren.GaussianRaytracer.OUTPUT_BUFFERS) + ["output_denoised", "accumulated_rgb", "accumulated_transmittance", "accumulated_total_transmittance",
                                                          "accumulated_depth", "accumulated_normal", "accumulated_f0", "accumulated_roughness", "accumulated_sample_count"]
    with torch.no_grad():  # framebuffer content a batch must leave alone (including accumulators mid-sequence)
        m.get_config().accumulate_samples.fill_(True)
        ren.render(probe, rt, targets_available=False)
        m.get_config().accumulate_samples.fill_(False)
    before = {n: getattr(fb, n).clone() for n in names}
    bat = batched(ren, rt, cams, S, base)
    for n in names:
        assert torch.equal(getattr(fb, n), before[n]), n
    assert int(md.total_num_calls) == base + V * S and not bool(md.grads_enabled)
    seeds_b, acc_b, trav_b = md.random_seeds.clone(), st.num_accumulated_per_pixel.clone(), st.num_traversed_per_pixel.clone()
    c = m.get_counters()
    with torch.no_grad():
        after_batch = ren.render(probe, rt, targets_available=False).final
    seq = sequential(ren, rt, cams, S, base)
    assert_views_equal(bat, seq, "V=2 S=3")
    assert torch.equal(md.random_seeds, seeds_b) and torch.equal(st.num_accumulated_per_pixel, acc_b) and torch.equal(st.num_traversed_per_pixel, trav_b)
    assert int(st.num_traversed_per_pixel.sum()) > 0
    # counters: sums over the batch's frames (every frame traces all W*H primary rays)
    assert c[0] == V * S * 64 * 48 and c[11] == 0
    with torch.no_grad():
        after_seq = ren.render(probe, rt, targets_available=False).final
    assert torch.equal(after_batch, after_seq)  # the next launch sees the same total_num_calls


@BOTH_HELP_MODES
def test_batch_view_against_the_oracle(ren, orc, syn, team_help):
    rng = np.random.default_rng(3)
    W, H = 72, 40
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    cam = dict(origin=rng.uniform(-1.0, 1.0, 3).astype(np.float32), c2w=q.astype(np.float32), fov=np.float32(rng.uniform(0.3, 1.4)), znear=np.float32(0.01), zfar=np.float32(999.9))
    g = syn.make_scene(3000, "trained", seed=51)
    rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(jitter_primary_rays=0, num_bounces=1), team_help=team_help)
    other = syn.default_camera()
    rt.cuda_module.get_metadata().total_num_calls.fill_(20)
    vs = ren.render_views([cam_obj(ren, other), cam_obj(ren, cam)], rt)  # view 1 = frame 1: the seeds of total_num_calls 22
    o.total_num_calls = 21
    ref = o.raytrace(False)
    out = dict(output_rgb=vs[1].rgb.moveaxis(1, -1), output_final=vs[1].final.moveaxis(1, -1), output_depth=vs[1].depth.moveaxis(1, -1),
               output_normal=vs[1].normal.moveaxis(1, -1))
    out = {k: v.cpu().numpy() for k, v in out.items()}
    lv = {k: round(psnr(out[k], ref[k]), 1) for k in out}
    report(f"render_views_oracle_help_{int(team_help)}", **lv)
    assert min(lv.values()) > 70, lv
    assert psnr(out["output_rgb"][0], ref["output_rgb"][0]) > 110


def test_team_help_on_stays_within_the_tie_bar(ren, syn):
    rt = tracer(ren, syn, W=192, H=128, N=20000, seed=8, team_help=True)
    rt.cuda_module.get_config().jitter_primary_rays.fill_(True)
    cams = [cam_obj(ren, c) for c in views(syn, 3)]
    seq = sequential(ren, rt, cams, 2, 3)
    bat = batched(ren, rt, cams, 2, 3)
    for v in range(3):
        diff = float((bat[v]["final"] != seq[v]["final"]).any(1).float().mean())
        assert diff < 2e-3, (v, diff)
        assert psnr(bat[v]["final"].cpu().numpy(), seq[v]["final"].cpu().numpy()) > 60


def test_partition_traces_own_tiles_only(ren, syn):
    par = importlib.import_module(PKG + ".parallel")
    W, H = 96, 64
    rt = tracer(ren, syn, W=W, H=H, rank=0, world_size=2)
    m = rt.cuda_module
    m.set_rays_per_task(64)  # (the task shape of the whole-image launch: exact ties composite in the same order)
    cams = [cam_obj(ren, c) for c in views(syn, 2)]
    m.get_metadata().total_num_calls.fill_(5)
    whole = ren.render_views(cams, rt)  # a partitioned tracer renders the whole image on the calling rank
    R = torch.stack([c.R for c in cams]).float()
    centers = torch.stack([c.camera_center for c in cams])
    fovy = torch.tensor([c.FoVy for c in cams], dtype=torch.float32)
    sentinel = -7.25
    bufs = [torch.full((2, H, W, 3), sentinel, device="cuda"), torch.full((2, 3, H, W, 1), sentinel, device="cuda")]
    m.get_metadata().total_num_calls.fill_(5)
    m.render_views_into(R, centers, fovy, 0.01, 999.9, 1, ["final", "depth"], bufs)  # rank 0 of 2
    torch.cuda.synchronize()
    own = torch.from_numpy(np.kron(par.tile_owner(W, H, 2), np.ones((16, 16), np.int64))[:H, :W] == 0).cuda()
    for v in range(2):
        fin, dep = bufs[0][v], bufs[1][v]
        assert bool((fin[~own] == sentinel).all()) and bool((dep[:, ~own] == sentinel).all())
        assert torch.equal(fin[own], whole[v].final[0].moveaxis(0, -1)[own])
        assert torch.equal(dep[:, own], whole[v].depth.moveaxis(1, -1)[:, own])
    assert int(m.get_metadata().total_num_calls) == 7


def test_exact_stats_and_argument_errors(ren, syn):
    rt = tracer(ren, syn)
    m = rt.cuda_module
    cams = [cam_obj(ren, c) for c in views(syn, 2)]
    default = batched(ren, rt, cams, 2, 9)
    m.set_exact_stats(True)
    with pytest.raises(RuntimeError):  # the tree was not refitted with cube boxes yet
        ren.render_views(cams, rt)
    m.update_bvh()
    exact = batched(ren, rt, cams, 2, 9)
    assert_views_equal(exact, default, "exact-stats build")
    m.set_exact_stats(False)
    m.update_bvh()
    R = torch.stack([c.R for c in cams]).float()
    centers = torch.stack([c.camera_center for c in cams])
    fovy = torch.tensor([c.FoVy for c in cams], dtype=torch.float32)
    fin, rgb = torch.full((2, 48, 64, 3), 3.5, device="cuda"), torch.full((2, 3, 48, 64, 3), 3.5, device="cuda")
    m.get_metadata().total_num_calls.fill_(9)
    bad = [(R, centers, fovy, 0, ["final", "rgb"], [fin, rgb]),  # S == 0
           (R, centers, fovy, 1, ["rgb"], [rgb]),  # no final
           (R, centers[:1], fovy, 1, ["final"], [fin]),  # shape
           (R[:0], centers[:0], fovy[:0], 1, ["final"], [fin[:0]])]  # V == 0
    for r_, c_, f_, s_, names, bufs in bad:
        with pytest.raises(RuntimeError):
            m.render_views_into(r_, c_, f_, 0.01, 999.9, s_, names, bufs)
    with pytest.raises(RuntimeError):
        m.render_views(R, centers, fovy, 0.01, 999.9, 1, ["final", "brdf"])
    with pytest.raises(RuntimeError):
        m.set_batch_frames(0)
    torch.cuda.synchronize()
    assert bool((fin == 3.5).all()) and bool((rgb == 3.5).all()) and int(m.get_metadata().total_num_calls) == 9
