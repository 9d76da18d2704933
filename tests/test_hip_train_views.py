"""Multi-view training launch (egr_train_views / Raytracer.train_views / renderer.train_views): the gradients of V views in one call, held against V
sequential grad launches into a zeroed gradient buffer and against the fp32 oracle (include/egr_raytracer.h: egr_train_batch). Gradient bars are per
tensor, relative to that tensor's max |grad|."""
import functools

import numpy as np
import pytest

import hip_common
from hip_common import BOTH_HELP_MODES, GRAD_KEYS, cam_obj, generic_targets, hip_grads, make_pair, ren, report, views  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TARGET_KEYS = ("diffuse", "specular", "depth", "normal", "roughness", "f0")
tracer = functools.partial(hip_common.tracer, bwd=8_000_000)  # (grad launches: the hit arena of a training configuration)


def view_targets(syn, W, H, n):
    """Distinct, non-zero targets per view."""
    out = []
    for i in range(n):
        tg = generic_targets(syn, W, H)
        out.append({k: (v + np.float32(0.07 * i)).astype(np.float32) for k, v in tg.items()})
    return out


def zero_native(rt):
    rt.zero_grad()
    rt.cuda_module.get_gaussians().total_weight.zero_()


def sequential(ren, rt, cams, base):
    """The contract's reference: V grad launches into a zeroed gradient buffer. Returns the native gradients and the summed work counters."""
    m = rt.cuda_module
    zero_native(rt)
    m.get_metadata().total_num_calls.fill_(base)
    work = np.zeros(9, np.int64)
    status = 0
    for c in cams:
        ren.render(c, rt)
        c_ = m.get_counters()
        work += np.array(c_[:9], np.int64)
        status |= int(c_[11])
    torch.cuda.synchronize()
    return hip_grads(rt), work, status


def batched(ren, rt, cams, base):
    m = rt.cuda_module
    zero_native(rt)
    m.get_metadata().total_num_calls.fill_(base)
    ren.train_views(cams, rt)
    c_ = m.get_counters()
    torch.cuda.synchronize()
    return hip_grads(rt), np.array(c_[:9], np.int64), int(c_[11])


def rel_errs(a, b):
    out = {}
    for k in GRAD_KEYS:
        scale = float(np.abs(b[k]).max())
        assert scale > 0, k
        out[k] = float(np.abs(a[k] - b[k]).max()) / scale
    return out


def assert_grads_close(a, b, what, bar=1e-5):
    e = rel_errs(a, b)
    report(what, worst=f"{max(e.values()):.1e}")
    assert max(e.values()) < bar, (what, e)


@pytest.mark.parametrize("bounces", [0, 2])
@pytest.mark.parametrize("jitter", [False, True], ids=["jitter_off", "jitter_on"])
def test_multi_view_equals_sequential(ren, syn, jitter, bounces):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    m = rt.cuda_module
    m.get_config().num_bounces.fill_(bounces)
    m.get_config().jitter_primary_rays.fill_(jitter)
    tgs = view_targets(syn, W, H, 3)
    cams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 3), tgs)]
    seq, work_s, st_s = sequential(ren, rt, cams, 40)
    bat, work_b, st_b = batched(ren, rt, cams, 40)
    assert_grads_close(bat, seq, f"train_views_vs_sequential_j{int(jitter)}_b{bounces}")
    assert st_s == 0 and st_b == 0
    assert np.array_equal(work_b, work_s), (work_b, work_s)  # rays, candidates, composited per step
    assert work_b[0] == 3 * W * H and (bounces == 0 or work_b[1] > 0)
    one, _, _ = batched(ren, rt, cams[:1], 40)  # three views are not one
    assert not np.allclose(one["dL_dmean"], bat["dL_dmean"])


def test_chunking_changes_nothing(ren, syn):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    m = rt.cuda_module
    tgs = view_targets(syn, W, H, 5)
    cams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 5, 0.08), tgs)]
    m.set_batch_frames(2)  # chunks of 2, 2, 1
    small, work_s, st_s = batched(ren, rt, cams, 3)
    m.set_batch_frames(8)
    whole, work_w, st_w = batched(ren, rt, cams, 3)
    assert_grads_close(small, whole, "train_views_chunks_of_2_vs_8")
    assert np.array_equal(work_s, work_w) and st_s == 0 and st_w == 0


def test_side_effects_match_the_sequential_launches(ren, syn):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    m = rt.cuda_module
    tgs = view_targets(syn, W, H, 3)
    cams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 3), tgs)]
    probe = cam_obj(ren, views(syn, 4)[3], generic_targets(syn, W, H))
    fb, md, st, cam = m.get_framebuffer(), m.get_metadata(), m.get_stats(), m.get_camera()
    ren.render(probe, rt)  # binds the probe's camera
    md.total_num_calls.fill_(90)
    with torch.no_grad():
        m.raytrace()  # an image of the bound camera (its pose is not readable: the batch must leave it as it is)
    final_before = fb.output_final.clone()
    ren.render(probe, rt)  # a single grad launch: what the debug exports describe
    hits0, hash0 = m.debug_step_hits().clone(), m.debug_hit_sequence_hash().clone()
    assert int(hits0.sum()) > 0
    sentinel = 7.25
    outs = list(ren.GaussianRaytracer.OUTPUT_BUFFERS) + ["output_denoised", "accumulated_rgb", "accumulated_depth"]
    tnames = ["target_" + k for k in TARGET_KEYS]
    for n in outs + tnames:
        getattr(fb, n).fill_(sentinel)
    cam_before = {n: getattr(cam, n).clone() for n in ("vertical_fov_radians", "znear", "zfar")}
    acc_count = fb.accumulated_sample_count.clone()
    V, base = 3, 11
    md.total_num_calls.fill_(base)
    md.grads_enabled.fill_(False)
    ren.train_views(cams, rt)
    torch.cuda.synchronize()
    assert int(md.total_num_calls) == base + V and bool(md.grads_enabled)
    for n in outs + tnames:
        assert bool((getattr(fb, n) == sentinel).all()), n
    assert torch.equal(fb.accumulated_sample_count, acc_count)
    for n, t in cam_before.items():
        assert torch.equal(getattr(cam, n), t), n
    # the batch traced into buffers of its own: the debug exports still describe the single launch above
    assert torch.equal(m.debug_step_hits(), hits0) and torch.equal(m.debug_hit_sequence_hash(), hash0)
    seeds_b, acc_b, trav_b = md.random_seeds.clone(), st.num_accumulated_per_pixel.clone(), st.num_traversed_per_pixel.clone()
    c = m.get_counters()
    assert c[10] >= V and c[11] == 0
    md.total_num_calls.fill_(90)
    with torch.no_grad():
        m.raytrace()
    assert torch.equal(fb.output_final, final_before)  # the bound camera is the probe's still
    md.total_num_calls.fill_(base)
    for cm in cams:
        ren.render(cm, rt)
    torch.cuda.synchronize()
    assert int(md.total_num_calls) == base + V
    assert torch.equal(md.random_seeds, seeds_b) and torch.equal(st.num_accumulated_per_pixel, acc_b) and torch.equal(st.num_traversed_per_pixel, trav_b)
    assert int(st.num_traversed_per_pixel.sum()) > 0


@BOTH_HELP_MODES
def test_batch_gradients_against_the_oracle(ren, orc, syn, team_help):
    W, H = 80, 48
    g = syn.make_scene(3000, "trained", seed=21)
    cams = views(syn, 2, 0.03)
    tgs = [syn.make_targets(W, H), generic_targets(syn, W, H)]
    rt, o = make_pair(ren, orc, g, cams[0], W, H, cfg=dict(jitter_primary_rays=0), team_help=team_help)
    base = 30
    ref = {k: 0.0 for k in GRAD_KEYS}
    for v, (c, tg) in enumerate(zip(cams, tgs)):
        o.set_camera(c["origin"], c["c2w"], c["fov"], c["znear"], c["zfar"])
        o.total_num_calls = base + v
        r = o.raytrace(True, targets=tg)
        for k in GRAD_KEYS:
            ref[k] = ref[k] + r[k]
    bat, _, status = batched(ren, rt, [cam_obj(ren, c, t) for c, t in zip(cams, tgs)], base)
    e = rel_errs(bat, ref)
    report(f"train_views_oracle_help_{int(team_help)}", worst=f"{max(e.values()):.1e}")
    assert max(e.values()) < 1e-3, e
    assert status == 0


def test_at_size_equals_sequential(ren, syn):
    """1920x1080, 1M dense-init: 32-bit index and stride errors only show at real task counts."""
    W, H = 1920, 1080
    rt = tracer(ren, syn, W, H, N=1_000_000, seed=0, variant="init", fwd=400_000_000, bwd=300_000_000)
    tg = {k: torch.tensor(v).cuda().moveaxis(-1, 0).contiguous() for k, v in generic_targets(syn, W, H).items()}
    cams = []
    for i, c in enumerate(views(syn, 3, 0.06)):
        cams.append(cam_obj(ren, c))
        for k, t in tg.items():
            setattr(cams[-1], k + "_image", (t + 0.05 * i).contiguous())
    seq, work_s, st_s = sequential(ren, rt, cams, 5)
    bat, work_b, st_b = batched(ren, rt, cams, 5)
    assert_grads_close(bat, seq, "train_views_at_size")
    assert np.array_equal(work_b, work_s) and st_s == 0 and st_b == 0


def test_partition_ranks_sum_to_the_whole_batch(ren, syn):
    W, H = 96, 64
    tgs = view_targets(syn, W, H, 3)
    cams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 3), tgs)]
    whole = tracer(ren, syn, W, H)
    ref, _, _ = batched(ren, whole, cams, 8)
    ranks = [tracer(ren, syn, W, H, rank=r, world_size=2) for r in range(2)]
    deltas = []
    for rt in ranks:
        m = rt.cuda_module
        m.set_rays_per_task(64)  # (the whole-image task shape: exact ties composite in the same order)
        g = m.get_gaussians()
        m.grad_delta_consumed()
        g.grad_delta.fill_(3.5)  # a stale buffer: the first batch after a fold STORES
        rt._export_param_values()
        m.update_bvh(True)
        m.get_metadata().total_num_calls.fill_(8)
        R = torch.stack([c.R for c in cams]).float()
        centers = torch.stack([c.camera_center for c in cams])
        fovy = torch.tensor([c.FoVy for c in cams], dtype=torch.float32)
        t = [torch.stack([getattr(c, k + "_image") for c in cams]).contiguous() for k in TARGET_KEYS]
        m.train_views(R, centers, fovy, 0.01, 999.9, *t)
        first = g.grad_delta.clone()
        m.get_metadata().total_num_calls.fill_(8)
        m.train_views(R, centers, fovy, 0.01, 999.9, *t)  # no fold in between: ADDS
        torch.cuda.synchronize()
        assert int(m.get_counters()[11]) == 0
        second = g.grad_delta.clone()
        err = float((second - 2 * first).abs().max()) / float(first.abs().max())
        assert err < 1e-5, err
        deltas.append(first)
    n = ranks[0].cuda_module.get_gaussians().mean.shape[0]
    summed = (deltas[0] + deltas[1]).cpu().numpy()
    off = {"dL_drgb": (0, 3), "dL_dnormal": (3, 3), "dL_df0": (6, 3), "dL_droughness": (9, 1), "dL_dopacity": (10, 1), "dL_dscale": (11, 3), "dL_dmean": (14, 3),
           "dL_drotation": (17, 4), "total_weight": (21, 1)}
    got = {k: summed[o * n : (o + c) * n].reshape(n, c) for k, (o, c) in off.items()}
    assert_grads_close(got, ref, "train_views_partition_2")


def test_errors_write_nothing_and_arena_capacity(ren, syn):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    m = rt.cuda_module
    cams = [cam_obj(ren, c) for c in views(syn, 2)]
    R = torch.stack([c.R for c in cams]).float()
    centers = torch.stack([c.camera_center for c in cams])
    fovy = torch.tensor([c.FoVy for c in cams], dtype=torch.float32)
    g = m.get_gaussians()
    g.grad_flat.fill_(2.5)
    m.get_metadata().total_num_calls.fill_(17)
    ok = torch.zeros((2, 3, H, W), device="cuda")
    bad = [dict(R=R[:0], centers=centers[:0], fovy=fovy[:0], t=None),  # V == 0
           dict(R=R, centers=centers[:1], fovy=fovy, t=None),  # camera shape
           dict(R=R, centers=centers, fovy=fovy, t=torch.zeros((2, 3, H, W + 1), device="cuda")),  # target shape
           dict(R=R, centers=centers, fovy=fovy, t=ok.double())]  # target dtype
    for b in bad:
        with pytest.raises(RuntimeError):
            m.train_views(b["R"], b["centers"], b["fovy"], 0.01, 999.9, b["t"], None, None, None, None, None)
    m.set_exact_stats(True)
    with pytest.raises(RuntimeError):  # the tree was not refitted with cube boxes yet
        m.train_views(R, centers, fovy, 0.01, 999.9, ok, None, None, None, None, None)
    torch.cuda.synchronize()
    assert bool((g.grad_flat == 2.5).all()) and int(m.get_metadata().total_num_calls) == 17
    m.set_exact_stats(False)
    m.update_bvh()
    m.train_views(R, centers, fovy, 0.01, 999.9, ok, None, None, None, None, None)
    torch.cuda.synchronize()
    assert int(m.get_metadata().total_num_calls) == 19 and int(m.get_counters()[11]) == 0
    # capacity: a tiny backward arena overflows in a batch exactly when a single launch of the same frame does
    for bwd, expect in ((1_000, 2), (8_000_000, 0)):
        small = tracer(ren, syn, W, H, bwd=bwd)
        sm = small.cuda_module
        ren.render(cams[0], small)
        single = int(sm.get_counters()[11]) & 2
        ren.train_views([cams[0], cams[0]], small)
        batch = int(sm.get_counters()[11]) & 2
        assert single == expect and batch == expect, (bwd, single, batch)


def test_python_level_equals_render_per_camera(ren, syn):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    rt.cuda_module.get_config().jitter_primary_rays.fill_(True)
    tgs = view_targets(syn, W, H, 3)
    cams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 3), tgs)]
    pc = rt.pc
    for p in pc.parameters():
        p.grad.zero_()
    rt.cuda_module.get_metadata().total_num_calls.fill_(50)
    for c in cams:
        rt.zero_grad()
        ren.render(c, rt)
    seq = [p.grad.clone() for p in pc.parameters()]
    for p in pc.parameters():
        p.grad.zero_()
    rt.zero_grad()
    rt.cuda_module.get_metadata().total_num_calls.fill_(50)
    ren.train_views(cams, rt)
    torch.cuda.synchronize()
    for p, s in zip(pc.parameters(), seq):
        scale = float(s.abs().max())
        assert scale > 0
        assert float((p.grad - s).abs().max()) / scale < 1e-5
