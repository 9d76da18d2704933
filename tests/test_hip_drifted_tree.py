"""The refitted tree after Gaussians drifted out of the build frame (tests/drift_scenes.py). Training refits the BVH every iteration and rebuilds it
only at pruning intervals; a box that leaves the quantisation frame of the last rebuild is stored with sentinel cells, the device flag out_of_frame
is raised, and every forward launch runs other code: pair_walk<SENT = true> with qslab_hit, the frustum walk's `keep |= sentinel` term, no
beyond-far shortcut (csrc/trace.hip, csrc/forward_task.inc, csrc/bvh.hip).

The strongest check needs no tolerance: a tree that was only refitted and a tree rebuilt on the same parameters differ in the walk, not in what a
ray meets - same candidate set, hence the same per-pixel statistics, counters, composited sequences and bit-identical images (the argument of
test_team_help_changes_the_list_order_only). Pixels where the oracle sees two consecutive hits within 4 ulps (num_depth_ties; the order of an exact
tie follows the list order, which a rebuild changes) are listed and held to the swapped-pair bound instead. The drifted tree is held against the
oracle as well, gradients included. test_drift_scenes.py holds the inputs to what these tests need from them, without a GPU.

Every test builds on the base scene (the constructor fixes the frame), copies the drifted parameters in and refits with one launch
(force_update_bvh); the real frame and flag come from Raytracer.debug_bvh_state (egr_debug_get_bvh_state)."""
import numpy as np
import pytest

import drift_scenes as ds
from hip_common import (BOTH_HELP_MODES, GRAD_KEYS, OUT_KEYS, cam_obj, generic_targets, grads_vs_oracle_listing_flipped_pixels, hip_grads, hip_outputs, make_pair,  # noqa: F401
                        mismatch_list, psnr, ren, report, views)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

W, H = ds.W, ds.H
PARAMS = (("_xyz", "mean"), ("_opacity", "opacity"), ("_scaling", "scale"), ("_rotation", "rotation"), ("_diffuse", "rgb"), ("_normal", "normal"),
          ("_roughness", "roughness"), ("_f0", "f0"))
INTEGERS = ("trav", "acc", "hits", "seq")  # both per-pixel statistics, composited hits per step, hash of the ordered composited ids per step


def load(rt, g):
    with torch.no_grad():
        for attr, key in PARAMS:
            getattr(rt.pc, attr).copy_(torch.from_numpy(g[key]).cuda())


def refit(ren, rt, cam, **zz):
    with torch.no_grad():
        rt(cam_obj(ren, cam), force_update_bvh=True, **zz)  # exports the parameters, update_bvh: a refit in the frame of the last rebuild
    torch.cuda.synchronize()


def bvh_state(rt):
    frame, info = rt.cuda_module.debug_bvh_state()
    return frame.numpy().copy(), [int(x) for x in info]


def assert_tree(rt, flag, sides_expected=()):
    """The assertions of every test: a consistent tree, no overflow, the flag, and the flag's reason restated from the boxes and the real frame."""
    m = rt.cuda_module
    assert m.check_bvh() == 0, m.last_error()
    assert int(m.get_counters()[11]) == 0
    frame, info = bvh_state(rt)
    assert info[0] == flag and info[1] >= 1 and info[2] >= 1 and info[3] == ds.N, info
    mask, sides = ds.out_of_frame_mask(m.debug_instances()[2].numpy(), frame)
    assert bool(mask.any()) == bool(flag), (flag, sides)
    for side in ds.SIDES:
        assert (sides[side] > 0) == (side in sides_expected), (side, sides, sorted(sides_expected))
    return frame, sides


def drifted_pair(ren, orc, base, drifted, cam, cfg, exact_stats=False, zz=None, **kw):
    """(tracer, oracle): the tree built on `base`, the parameters of `drifted` refitted into it; the oracle holds `drifted`."""
    rt, o = make_pair(ren, orc, base, cam, W, H, cfg=cfg, **kw)
    assert_tree(rt, 0)
    if exact_stats:
        rt.cuda_module.set_exact_stats(True)
    load(rt, drifted)
    o.set_gaussians(drifted)
    o.update_bvh()
    refit(ren, rt, cam, **(zz or {}))
    return rt, o


def launch_images(rt, camera, **zz):
    m = rt.cuda_module
    m.get_metadata().total_num_calls.zero_()
    with torch.no_grad():
        rt(camera, **zz)
    torch.cuda.synchronize()
    st, c = m.get_stats(), m.get_counters()
    assert int(c[11]) == 0
    return dict(out=hip_outputs(rt), trav=st.num_traversed_per_pixel.cpu().numpy().copy(), acc=st.num_accumulated_per_pixel.cpu().numpy().copy(),
                counters=[int(x) for x in c[:9]])


def launch_grads(ren, rt, camera, **zz):
    m = rt.cuda_module
    m.get_metadata().total_num_calls.zero_()
    rt.zero_grad()
    m.get_gaussians().total_weight.zero_()
    ren.render(camera, rt, **zz)
    torch.cuda.synchronize()
    assert int(m.get_counters()[11]) == 0
    return dict(grads=hip_grads(rt), hits=m.debug_step_hits().numpy().copy(), seq=m.debug_hit_sequence_hash().numpy().copy())


def both_launches(ren, rt, cam, tg, **zz):
    """One no-grad and one grad launch of the same rays (total_num_calls zeroed before each)."""
    return dict(launch_images(rt, cam_obj(ren, cam), **zz), **launch_grads(ren, rt, cam_obj(ren, cam, tg), **zz))


def oracle_images(o):
    o.total_num_calls = 0
    return o.raytrace(False)


def oracle_near_ties(o, tg, name):
    """[H,W] mask of the pixels with two consecutive hits within 4 ulps (oracle, grad launch of the same rays): at most 8, listed."""
    o.total_num_calls = 0
    flagged = o.raytrace(True, targets=tg)["num_depth_ties"] > 0
    ys, xs = np.nonzero(flagged)
    report(name + "_near_tie_pixels", count=int(flagged.sum()), pixels=[(int(x), int(y)) for y, x in zip(ys, xs)])
    assert int(flagged.sum()) <= 8, (name, int(flagged.sum()))
    return flagged


def assert_same_walk(a, b, flagged, name, integers=INTEGERS, grad_bar=1e-4):
    """Two launch pairs (both_launches) of the same rays through two walks of the same scene: counters and the per-pixel integers equal at every
    pixel; every output bit-equal at every pixel outside `flagged` and within 2e-4 (the swapped-pair bound of test_forward_strict_parity_primary) on
    it; gradients within 1e-4 of each tensor's maximum (same set, other order of the atomics)."""
    assert a["counters"] == b["counters"], (name, a["counters"], b["counters"])
    assert a["counters"][0] == W * H
    for k in integers:
        bad, n = mismatch_list(a[k], b[k])
        assert n == 0, (name, k, n, bad)
    worst_flagged = 0.0
    for k in OUT_KEYS:
        x, y = a["out"][k], b["out"][k]
        differs = np.any(x.view(np.uint32) != y.view(np.uint32), axis=(0, -1))  # [H,W]
        wrong = differs & ~flagged
        ys, xs = np.nonzero(wrong)
        assert not wrong.any(), (name, k, int(wrong.sum()), [(int(x_), int(y_)) for y_, x_ in zip(ys[:8], xs[:8])])
        if flagged.any():
            d = float(np.abs(x - y).max(axis=(0, -1))[flagged].max())
            worst_flagged = max(worst_flagged, d)
            assert d <= 2e-4, (name, k, d)
    errs = {}
    for k in GRAD_KEYS:
        errs[k] = float(np.abs(a["grads"][k] - b["grads"][k]).max() / max(float(np.abs(b["grads"][k]).max()), 1e-30))
    report(name, worst_grad=f"{max(errs.values()):.1e}", worst_output_difference_on_near_tie_pixels=f"{worst_flagged:.1e}")
    assert float(np.abs(b["grads"]["dL_dmean"]).max()) > 0
    assert max(errs.values()) < grad_bar, (name, errs)


def refit_then_rebuild(ren, rt, o, cam, tg, sides, name, zz=None):
    """The launches on the refitted tree, rebuild_bvh(), the same launches; returns both."""
    zz = zz or {}
    flagged = oracle_near_ties(o, tg, name)
    a = both_launches(ren, rt, cam, tg, **zz)
    frame_a, _ = assert_tree(rt, 1, sides)  # (the grad launch refitted once more: same frame, same flag)
    rt.cuda_module.rebuild_bvh()
    frame_b, _ = assert_tree(rt, 0)
    assert not np.array_equal(frame_a, frame_b)
    b = both_launches(ren, rt, cam, tg, **zz)
    assert_tree(rt, 0)
    assert_same_walk(a, b, flagged, name)
    return a, b, flagged


# ------------------------------------------------------------------------------------------------ refit equals rebuild
@pytest.mark.parametrize("rays_per_task", [64, 16])
@pytest.mark.parametrize("kind,seed", [("dilate", 1), ("two_walls", 1), ("growth", 1), ("far_wall", 8)])
def test_refit_equals_rebuild(ren, orc, syn, monkeypatch, kind, seed, rays_per_task):
    """8x8 tasks: step 0 is the frustum walk, steps 1 and 2 the pair walk; 4x4 tasks: every step is the pair walk. Jitter on, two bounces, help off."""
    monkeypatch.setenv("EGR_RAYS_PER_TASK", str(rays_per_task))
    g = ds.base_scene(syn, seed)
    cam, tg = syn.default_camera(), generic_targets(syn, W, H)
    rt, o = drifted_pair(ren, orc, g, ds.drift(syn, g, kind), cam, dict(jitter_primary_rays=1, num_bounces=2), team_help=False)
    assert_tree(rt, 1, ds.EXPECTED_SIDES[kind])
    a, _, _ = refit_then_rebuild(ren, rt, o, cam, tg, ds.EXPECTED_SIDES[kind], f"refit_vs_rebuild_{kind}_{rays_per_task}")
    assert a["counters"][1] > 0 and a["counters"][2] > 0  # the bounce steps ran


@pytest.mark.parametrize("axis,sign", ds.WALLS)
def test_each_sentinel_kind_alone_in_the_frustum_walk(ren, orc, syn, monkeypatch, axis, sign):
    """One wall moved out by 1.0, seen at an angle: exactly one of the six sentinel terms of frustum_hit keeps these boxes."""
    monkeypatch.setenv("EGR_RAYS_PER_TASK", "64")
    g = ds.base_scene(syn, 9)
    cam, tg = ds.oblique_camera(syn, axis, sign), generic_targets(syn, W, H)
    side = {ds.wall_side(axis, sign)}
    rt, o = drifted_pair(ren, orc, g, ds.wall(syn, g, axis, sign), cam, dict(jitter_primary_rays=0, num_bounces=0), team_help=False)
    assert_tree(rt, 1, side)
    name = "sentinel_" + ds.wall_side(axis, sign)
    a, _, _ = refit_then_rebuild(ren, rt, o, cam, tg, side, name)
    ref = oracle_images(o)
    bad, n_acc = mismatch_list(a["acc"], ref["num_accumulated"])
    levels = {k: round(psnr(a["out"][k], ref[k]), 1) for k in ("output_rgb", "output_depth", "output_total_transmittance")}
    report(name + "_vs_oracle", acc_mismatch=n_acc, first=bad, **levels)
    assert n_acc <= 1, bad
    for k, v in levels.items():
        assert v > 90, (k, v)


# ------------------------------------------------------------------------------------------------ against the oracle
@BOTH_HELP_MODES
@pytest.mark.parametrize("kind", ["dilate", "growth"])
def test_drifted_tree_against_the_oracle_with_gradients(ren, orc, syn, kind, team_help):
    g = ds.base_scene(syn, 9)
    cam, tg = syn.default_camera(), generic_targets(syn, W, H)
    rt, o = drifted_pair(ren, orc, g, ds.drift(syn, g, kind), cam, dict(jitter_primary_rays=0, num_bounces=2), team_help=team_help)
    assert_tree(rt, 1, ds.EXPECTED_SIDES[kind])
    img, ref = launch_images(rt, cam_obj(ren, cam)), oracle_images(o)
    levels = {k: round(psnr(img["out"][k], ref[k]), 1) for k in OUT_KEYS}
    name = f"drifted_{kind}_{'help_on' if team_help else 'help_off'}"
    report(name + "_forward", **levels)
    for k, v in levels.items():
        assert v >= 50, (k, v)
    grads_vs_oracle_listing_flipped_pixels(ren, rt, o, cam_obj(ren, cam, tg), tg, W, H, name + "_grads")
    assert_tree(rt, 1, ds.EXPECTED_SIDES[kind])


def test_near_and_far_segments_on_a_drifted_tree(ren, orc, syn):
    """znear 1.5, zfar 4.0: candidates in front of near and beyond far still enter T_total (quirk Q1) - here most of them left the frame."""
    g = ds.base_scene(syn, 9)
    cam = dict(syn.default_camera(), znear=np.float32(1.5), zfar=np.float32(4.0))
    zz, tg = dict(znear=1.5, zfar=4.0), generic_targets(syn, W, H)
    rt, o = drifted_pair(ren, orc, g, ds.drift(syn, g, "dilate"), cam, dict(jitter_primary_rays=0, num_bounces=1), zz=zz, team_help=False)
    assert_tree(rt, 1, ds.ALL_SIDES)
    ref = oracle_images(o)
    q1 = float((ref["output_total_transmittance"][0] < ref["output_transmittance"][0] - 1e-4).mean())
    assert q1 >= 0.5, q1
    a, _, _ = refit_then_rebuild(ren, rt, o, cam, tg, ds.ALL_SIDES, "near_far_dilate", zz=zz)
    levels = {k: round(psnr(a["out"][k], ref[k]), 1) for k in ("output_rgb", "output_total_transmittance", "output_transmittance", "output_depth")}
    report("near_far_dilate_vs_oracle", q1_share=round(q1, 3), **levels)
    for k, v in levels.items():
        assert v > 55, (k, v)


def test_far_plane_between_the_frame_and_the_drifted_wall(ren, orc, syn):
    """The beyond-far shortcut (forward_task.inc: beyond_far_empty) skips segment 2 (t > far) when no corner of the FRAME is farther than the far
    plane - valid only while every box lies inside the frame. Here the frame ends 6 units from the camera, the far plane lies at 30 and the +x wall,
    12 times as far and as large, straddles it: the candidates beyond far whose cubes reach back over the plane (quirk Q1) all left the frame, so the
    shortcut taken on this tree would drop them. Precondition from the oracle: hiding the Gaussians beyond the plane changes T_total of step 0 on at
    least 5 % of the pixels (measured 12 %; 5 % is the smallest share test_drift_scenes.py accepts for an input)."""
    zfar = 30.0
    g = ds.base_scene(syn, 8)
    d = ds.drift(syn, g, "far_wall")
    cam = dict(syn.default_camera(), zfar=np.float32(zfar))
    zz, tg, cfg = dict(zfar=zfar), generic_targets(syn, W, H), dict(jitter_primary_rays=0, num_bounces=1)
    sides = ds.EXPECTED_SIDES["far_wall"]
    rt, o = drifted_pair(ren, orc, g, d, cam, cfg, zz=zz, team_help=False)
    frame, _ = assert_tree(rt, 1, sides)
    corners = np.array([[frame[a] + (-2.0, 65534.0)[(c >> a) & 1] / frame[3 + a] for a in range(3)] for c in range(8)])
    assert float(np.linalg.norm(corners - cam["origin"], axis=1).max()) < 0.9 * zfar  # the shortcut's condition holds for the primary rays
    ref = oracle_images(o)
    beyond = np.linalg.norm(d["mean"].astype(np.float64) - cam["origin"], axis=1) > zfar
    _, o_hidden = make_pair(ren, orc, ds.hidden(d, beyond), cam, W, H, cfg=cfg)
    share = float((np.abs(ref["output_total_transmittance"][0] - oracle_images(o_hidden)["output_total_transmittance"][0]) > 1e-4).mean())
    assert share >= 0.05, share
    a, _, _ = refit_then_rebuild(ren, rt, o, cam, tg, sides, "far_plane_far_wall", zz=zz)
    levels = {k: round(psnr(a["out"][k], ref[k]), 1) for k in ("output_rgb", "output_total_transmittance", "output_transmittance", "output_depth")}
    report("far_plane_far_wall_vs_oracle", share_of_pixels_fed_from_beyond_far=round(share, 3), **levels)
    for k, v in levels.items():
        assert v > 55, (k, v)


# ------------------------------------------------------------------------------------------------ the other launch paths
def test_team_help_on_a_drifted_tree(ren, orc, syn):
    """test_team_help_changes_the_list_order_only on a refitted tree: the helpers always run pair_walk<true, ...>, whose sentinel decode the flag
    now needs. (off, on, on): counters and both statistics equal, images bit-equal, gradients within 1e-4."""
    g = ds.base_scene(syn, 1)
    cam, tg = syn.default_camera(), generic_targets(syn, W, H)
    sides = ds.EXPECTED_SIDES["two_walls"]
    rt, o = drifted_pair(ren, orc, g, ds.drift(syn, g, "two_walls"), cam, dict(jitter_primary_rays=1, num_bounces=2), team_help=False)
    assert_tree(rt, 1, sides)
    flagged = oracle_near_ties(o, tg, "team_help_two_walls")
    m = rt.cuda_module
    runs = []
    for help_on in (False, True, True):
        m.set_team_help(help_on)
        runs.append(both_launches(ren, rt, cam, tg))
        assert_tree(rt, 1, sides)
    m.set_team_help(False)
    for i in (1, 2):
        assert_same_walk(runs[i], runs[0], flagged, f"team_help_two_walls_run{i}", integers=("trav", "acc"))
    # help on and off could be wrong together (one decode serves both): the rebuilt tree, walked without help, is the third witness
    m.rebuild_bvh()
    assert_tree(rt, 0)
    rebuilt = both_launches(ren, rt, cam, tg)
    for i in (1, 2):
        assert_same_walk(runs[i], rebuilt, flagged, f"team_help_two_walls_run{i}_vs_rebuild", integers=("trav", "acc"))


def test_exact_statistics_on_a_drifted_tree(ren, orc, syn):
    """set_exact_stats(True), then the refit: the tree bounds the instance CUBES, which cross the frame's border too; num_traversed_per_pixel is the
    reference's invocation count (bars of test_exact_stats_mode_counts_reference_invocations, primary step)."""
    g = ds.base_scene(syn, 9)
    cam = syn.default_camera()
    rt, o = drifted_pair(ren, orc, g, ds.drift(syn, g, "growth"), cam, dict(jitter_primary_rays=0, num_bounces=0), exact_stats=True, team_help=False)
    assert_tree(rt, 1, ds.ALL_SIDES)
    img, ref = launch_images(rt, cam_obj(ren, cam)), oracle_images(o)
    bad, nbad = mismatch_list(img["trav"], ref["num_traversed"])
    report("exact_stats_growth", mismatching_pixels=nbad, first=bad, hc_exact=int(img["trav"].sum()), hc_oracle=int(ref["num_traversed"].sum()))
    assert nbad <= 2, bad
    assert abs(int(img["trav"].sum()) - int(ref["num_traversed"].sum())) <= 2
    assert_tree(rt, 1, ds.ALL_SIDES)


def test_batch_paths_on_a_drifted_tree(ren, orc, syn):
    """render_views and train_views by the existing batch tests' criteria, on a tree whose flag is set."""
    import test_hip_render_views as rv
    import test_hip_train_views as tv

    g = ds.base_scene(syn, 1)
    cam = syn.default_camera()
    rt, _ = drifted_pair(ren, orc, g, ds.drift(syn, g, "dilate"), cam, dict(jitter_primary_rays=1, num_bounces=2), team_help=False)
    assert_tree(rt, 1, ds.ALL_SIDES)
    cams = [cam_obj(ren, c) for c in views(syn, 3)]
    seq = rv.sequential(ren, rt, cams, 2, 40)
    bat = rv.batched(ren, rt, cams, 2, 40)
    rv.assert_views_equal(bat, seq, "drifted V=3 S=2")
    assert float(bat[2]["final"].abs().sum()) > 0 and not torch.equal(bat[0]["final"], bat[1]["final"])
    assert_tree(rt, 1, ds.ALL_SIDES)
    tcams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 3), tv.view_targets(syn, W, H, 3))]
    gs, work_s, st_s = tv.sequential(ren, rt, tcams, 40)
    gb, work_b, st_b = tv.batched(ren, rt, tcams, 40)
    tv.assert_grads_close(gb, gs, "drifted_train_views_vs_sequential")
    assert st_s == 0 and st_b == 0 and np.array_equal(work_b, work_s), (work_b, work_s)
    assert work_b[0] == 3 * W * H and work_b[1] > 0
    assert_tree(rt, 1, ds.ALL_SIDES)


# ------------------------------------------------------------------------------------------------ the flag
def test_life_of_the_out_of_frame_flag(ren, orc, syn):
    g = ds.base_scene(syn, 1)
    d = ds.drift(syn, g, "dilate")
    cam = syn.default_camera()
    camera = cam_obj(ren, cam)
    rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(jitter_primary_rays=1, num_bounces=2), team_help=False)
    frame0, _ = assert_tree(rt, 0)  # 1. built: flag 0
    img_a = launch_images(rt, camera)
    load(rt, d)  # 2. drifted and refitted: flag 1
    refit(ren, rt, cam)
    frame1, _ = assert_tree(rt, 1, ds.ALL_SIDES)
    assert np.array_equal(frame0, frame1)
    img_refit = launch_images(rt, camera)
    load(rt, g)  # 3. back and refitted: the flag clears, the tree is the built one
    refit(ren, rt, cam)
    frame2, _ = assert_tree(rt, 0)
    assert np.array_equal(frame0, frame2)
    img_back = launch_images(rt, camera)
    for k in OUT_KEYS:
        assert np.array_equal(img_back["out"][k].view(np.uint32), img_a["out"][k].view(np.uint32)), k
    assert img_back["counters"] == img_a["counters"] and np.array_equal(img_back["trav"], img_a["trav"]) and np.array_equal(img_back["acc"], img_a["acc"])
    load(rt, d)  # 4. drifted again and REBUILT: flag 0 in a new frame, the images of step 2
    rt._export_param_values()
    rt.cuda_module.rebuild_bvh()
    frame3, _ = assert_tree(rt, 0)
    assert not np.array_equal(frame0, frame3)
    img_rebuilt = launch_images(rt, camera)
    o.set_gaussians(d)
    o.update_bvh()
    flagged = oracle_near_ties(o, generic_targets(syn, W, H), "flag_life_dilate")
    for k in OUT_KEYS:
        differs = np.any(img_rebuilt["out"][k].view(np.uint32) != img_refit["out"][k].view(np.uint32), axis=(0, -1))
        assert not (differs & ~flagged).any(), (k, int((differs & ~flagged).sum()))
    assert img_rebuilt["counters"] == img_refit["counters"] and np.array_equal(img_rebuilt["trav"], img_refit["trav"])
    assert psnr(img_refit["out"]["output_rgb"][0], img_a["out"]["output_rgb"][0]) < 40  # the two states really differ


def test_many_refits_between_two_rebuilds(ren, orc, syn):
    """Twenty small increments of every mean and scale, refitted after each one: the stand-in for a training interval."""
    g = ds.base_scene(syn, 1)
    cam, tg = syn.default_camera(), generic_targets(syn, W, H)
    rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(jitter_primary_rays=1, num_bounces=2), team_help=False)
    assert_tree(rt, 0)
    m = rt.cuda_module
    states = ds.walk(g, 20, np.random.default_rng(1))
    for i, s in enumerate(states, 1):
        load(rt, s)
        refit(ren, rt, cam)
        if i % 5 == 0:
            assert m.check_bvh() == 0, (i, m.last_error())
            assert int(m.get_counters()[11]) == 0
    frame, info = bvh_state(rt)
    mask, sides = ds.out_of_frame_mask(m.debug_instances()[2].numpy(), frame)
    report("many_refits", out_of_frame_boxes=int(mask.sum()), sides=sides)
    assert info[0] == 1 and mask.any()
    o.set_gaussians(states[-1])
    o.update_bvh()
    refit_then_rebuild(ren, rt, o, cam, tg, {k for k, v in sides.items() if v > 0}, "many_refits_vs_rebuild")
