"""The inputs of test_hip_drifted_tree.py, held to what that file needs from them with the CPU oracle alone (no GPU): every drift produces the
sentinel kinds it is meant to (and no others), the Gaussians that left the build frame carry a large share of the image (a walk that drops them
cannot pass an image comparison), and the rays have next to no near-ties (so "same candidate set" means "same image", bit for bit).
These are conditions on the inputs, not measurements of a kernel."""
import numpy as np
import pytest

import drift_scenes as ds

LOSS_WEIGHTS = dict(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0)
# (kind, seed, jitter) as test_hip_drifted_tree.py uses them; tie-free pairs are the ones whose gradients are held against the oracle
KIND_CASES = [("dilate", 1, 1), ("two_walls", 1, 1), ("growth", 1, 1), ("far_wall", 8, 1), ("dilate", 9, 0), ("growth", 9, 0)]
TIE_FREE = {("dilate", 9, 0), ("growth", 9, 0)}
WALL_SEED = 9


def oracle_for(orc, g, cam, **cfg):
    o = orc.Oracle(ds.W, ds.H)
    o.set_camera(cam["origin"], cam["c2w"], cam["fov"], cam.get("znear", 0.01), cam.get("zfar", 999.9))
    o.set_config(**dict(LOSS_WEIGHTS, **cfg))
    o.set_gaussians(g)
    o.update_bvh()
    return o


def study(orc, syn, base, drifted, cam, **cfg):
    """(sentinel sides' counts, image of the drifted scene, image without the Gaussians that left the frame, near-tie pixels)."""
    frame = ds.frame_restated(ds.ellipsoid_boxes(oracle_for(orc, base, cam)))
    o = oracle_for(orc, drifted, cam, **cfg)
    mask, sides = ds.out_of_frame_mask(ds.ellipsoid_boxes(o), frame)
    o.total_num_calls = 0
    img = o.raytrace(False)
    o.total_num_calls = 0
    ties = int((o.raytrace(True, targets=syn.make_targets(ds.W, ds.H))["num_depth_ties"] > 0).sum())
    oh = oracle_for(orc, ds.hidden(drifted, mask), cam, **cfg)
    oh.total_num_calls = 0
    return sides, img, oh.raytrace(False), ties


def assert_sides(sides, expected, what):
    for side in ds.SIDES:
        if side in expected:
            assert sides[side] >= 100, (what, side, sides)
        else:
            assert sides[side] == 0, (what, side, sides)


def test_base_scene_lies_inside_its_own_frame(orc, syn):
    for seed in (1, 8, 9):
        boxes = ds.ellipsoid_boxes(oracle_for(orc, ds.base_scene(syn, seed), syn.default_camera()))
        mask, sides = ds.out_of_frame_mask(boxes, ds.frame_restated(boxes))
        assert not mask.any() and sum(sides.values()) == 0, (seed, sides)


@pytest.mark.parametrize("kind,seed,jitter", KIND_CASES)
def test_drift_kinds_leave_the_frame_visibly_and_without_ties(orc, syn, kind, seed, jitter):
    g = ds.base_scene(syn, seed)
    sides, img, img_hidden, ties = study(orc, syn, g, ds.drift(syn, g, kind), syn.default_camera(), jitter_primary_rays=jitter, num_bounces=2)
    shares = [ds.changed_share(img, img_hidden, s) for s in range(3)]
    print(f"REPORT drift_inputs_{kind}_s{seed}_j{jitter}: sides={sides}, changed_share={[round(s, 3) for s in shares]}, near_tie_pixels={ties}")
    assert_sides(sides, ds.EXPECTED_SIDES[kind], (kind, seed))
    assert shares[0] >= 0.20 and shares[1] >= 0.20, (kind, seed, shares)
    assert ties <= 8, (kind, seed, ties)
    if (kind, seed, jitter) in TIE_FREE:
        assert ties == 0, (kind, seed, ties)


@pytest.mark.parametrize("axis,sign", ds.WALLS)
def test_single_walls_give_one_sentinel_kind_seen_obliquely(orc, syn, axis, sign):
    g = ds.base_scene(syn, WALL_SEED)
    cam = ds.oblique_camera(syn, axis, sign)
    sides, img, img_hidden, ties = study(orc, syn, g, ds.wall(syn, g, axis, sign), cam, jitter_primary_rays=0, num_bounces=0)
    share = ds.changed_share(img, img_hidden, 0)
    print(f"REPORT drift_inputs_wall_{ds.wall_side(axis, sign)}: sides={sides}, changed_share={share:.3f}, near_tie_pixels={ties}")
    assert_sides(sides, {ds.wall_side(axis, sign)}, (axis, sign))
    assert share >= 0.05, (axis, sign, share)
    assert ties <= 8, (axis, sign, ties)
    # never head-on: the central ray meets the wall's plane at an angle
    fwd = -np.asarray(cam["c2w"], np.float64)[:, 2]
    assert abs(fwd[axis]) < 0.85, (axis, sign, fwd)


def test_near_far_case_carries_q1_through_out_of_frame_candidates(orc, syn):
    """dilate with znear 1.5 / zfar 4.0: on most pixels candidates in front of near or beyond far enter T_total only (quirk Q1)."""
    g = ds.base_scene(syn, 9)
    cam = dict(syn.default_camera(), znear=np.float32(1.5), zfar=np.float32(4.0))
    sides, img, _, ties = study(orc, syn, g, ds.drift(syn, g, "dilate"), cam, jitter_primary_rays=0, num_bounces=1)
    q1 = float((img["output_total_transmittance"][0] < img["output_transmittance"][0] - 1e-4).mean())
    print(f"REPORT drift_inputs_near_far: q1_share={q1:.3f}, near_tie_pixels={ties}")
    assert_sides(sides, ds.ALL_SIDES, "near_far")
    assert q1 >= 0.5 and ties <= 8, (q1, ties)


def test_far_plane_case_is_fed_from_beyond_the_far_plane(orc, syn):
    """far_wall with zfar 30: the frame of the base scene ends within 6 units of the camera, the drifted wall straddles the far plane, and
    hiding the Gaussians beyond the plane changes T_total of step 0 (they are candidates by quirk Q1 alone) on at least 5 % of the pixels."""
    zfar = 30.0
    g = ds.base_scene(syn, 8)
    d = ds.drift(syn, g, "far_wall")
    cam = dict(syn.default_camera(), zfar=np.float32(zfar))
    sides, img, _, ties = study(orc, syn, g, d, cam, jitter_primary_rays=0, num_bounces=1)
    frame = ds.frame_restated(ds.ellipsoid_boxes(oracle_for(orc, g, cam)))
    corners = np.array([[frame[a] + (-2.0, 65534.0)[(c >> a) & 1] / frame[3 + a] for a in range(3)] for c in range(8)])
    reach = float(np.linalg.norm(corners - cam["origin"], axis=1).max())
    beyond = np.linalg.norm(d["mean"].astype(np.float64) - cam["origin"], axis=1) > zfar
    oh = oracle_for(orc, ds.hidden(d, beyond), cam, jitter_primary_rays=0, num_bounces=1)
    oh.total_num_calls = 0
    share = float((np.abs(img["output_total_transmittance"][0] - oh.raytrace(False)["output_total_transmittance"][0]) > 1e-4).mean())
    print(f"REPORT drift_inputs_far_plane: farthest_frame_corner={reach:.2f}, beyond={int(beyond.sum())}, T_total_share={share:.3f}, near_tie_pixels={ties}")
    assert_sides(sides, ds.EXPECTED_SIDES["far_wall"], "far_plane")
    assert reach < 0.9 * zfar and share >= 0.05 and ties <= 8, (reach, share, ties)


def test_walk_reaches_the_frame_border_within_twenty_steps(orc, syn):
    g = ds.base_scene(syn, 1)
    states = ds.walk(g, 20, np.random.default_rng(1))
    assert len(states) == 20 and not np.array_equal(states[0]["mean"], states[1]["mean"])
    sides, _, _, ties = study(orc, syn, g, states[-1], syn.default_camera(), jitter_primary_rays=1, num_bounces=2)
    print(f"REPORT drift_inputs_walk20: sides={sides}, near_tie_pixels={ties}")
    assert sum(sides.values()) >= 20 and ties <= 8, (sides, ties)


def test_mask_and_frame_rules_on_hand_made_boxes():
    """out_of_frame_mask / frame_restated against numbers worked out by hand: unit cube frame, one box per case."""
    boxes = np.array([[0, 0, 0, 1, 1, 1], [0.2, 0.2, 0.2, 0.4, 0.4, 0.4]], np.float32)
    frame = ds.frame_restated(boxes)
    np.testing.assert_allclose(frame[:3], -0.05, rtol=1e-6)
    np.testing.assert_allclose(frame[3:], 65530.0 / 1.1, rtol=1e-6)
    probe = np.array([[0.2, 0.2, 0.2, 0.4, 0.4, 0.4],       # inside
                      [-0.06, 0.2, 0.2, 0.4, 0.4, 0.4],     # lo x below the origin
                      [0.2, 0.2, 0.2, 0.4, 1.06, 0.4],      # hi y beyond cell 65533
                      [0.2, 0.2, -1.0, 0.4, 0.4, 2.0],      # both z sides
                      [5.0, 5.0, 5.0, -5.0, -5.0, -5.0]],   # not usable: never counted
                     np.float32)
    mask, sides = ds.out_of_frame_mask(probe, frame)
    assert mask.tolist() == [False, True, True, True, False]
    assert sides == dict(lo_x=1, lo_y=0, lo_z=1, hi_x=0, hi_y=1, hi_z=1)
