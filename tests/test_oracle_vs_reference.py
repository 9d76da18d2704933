"""The CPU oracle (oracle/egr_oracle.cpp, a restatement) against the reference's own shader code compiled for the CPU (oracle/ref_driver.cpp ->
oracle/_ref/libegr_reference.so, oracle/reference.py). Every HIP parity test trusts the oracle; this module is what the oracle answers to.

Each case feeds the same calls to three sides - the reference build, the fp32 oracle, the fp64 oracle - and applies tests/ref_compare.py: integers
exact at every pixel of every case, floats per tensor max|ref - o64| <= 8 max|o32 - o64| + 1e-6 max|o64| (and, for the images, per step as well: step 0 does not inherit the
slack that the bounce steps' amplified rounding gives the whole tensor). Both oracles run brute force (use_bvh=False), so all sides meet the
candidates of a ray in index order, the order the reference build's optixTraverse visits them in. Measured levels: oracle/REFERENCE_PARITY.md.

CPU only; at most 32 x 24 pixels and 2000 Gaussians per case. Skips as a whole where the reference library was not built (no reference sources)."""
import math

import numpy as np
import pytest

import bounce_scenes as bs
import ref_compare as rc
from oracle import reference as R

if not R.available():
    pytest.skip("oracle/_ref/libegr_reference.so is not built (the reference's sources were not there when build() ran)", allow_module_level=True)

MAX_ALPHA = 0.9999
GENERIC = dict(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0)


def logit(p):
    return math.log(p / (1 - p))


class Trio:
    """Reference build, fp32 oracle, fp64 oracle on one scene / camera / config; every call goes to all three."""

    def __init__(self, orc, g, cam, W, H, cfg=None, reverse_traversal=False, inverse_from_transform=True):
        self.W, self.H = W, H
        self.ref, self.o32, self.o64 = R.Reference(W, H, reverse_traversal=reverse_traversal), orc.Oracle(W, H, use_bvh=False, inverse_from_transform=inverse_from_transform), orc.Oracle(W, H, double=True, use_bvh=False)
        self.sides = (self.ref, self.o32, self.o64)
        f32 = lambda x: np.asarray(x, np.float32)  # noqa: E731  (the fp64 oracle gets the fp32 inputs the other two get)
        for o in self.sides:
            o.set_camera(f32(cam["origin"]), f32(cam["c2w"]), f32(cam["fov"]), f32(cam.get("znear", 0.01)), f32(cam.get("zfar", 999.9)))
            o.set_config(**(cfg or {}))
        self.set_gaussians(g)
        self.call("update_bvh")

    def call(self, name, *a, **kw):
        for o in self.sides:
            getattr(o, name)(*a, **kw)

    def set_gaussians(self, g):
        self.call("set_gaussians", {k: np.ascontiguousarray(v, np.float32) for k, v in g.items()})

    def launch(self, grads=False, targets=None, K=None):
        outs = []
        if targets is not None:
            targets = {k: np.ascontiguousarray(v, np.float32) for k, v in targets.items()}
        for o in self.sides:
            if K is not None:
                o.total_num_calls = K - 1
            outs.append(o.raytrace(grads, targets=targets))
        assert self.ref.total_num_calls == self.o32.total_num_calls == self.o64.total_num_calls
        return outs

    @staticmethod
    def _compare(outs, grads):
        ref, a, b = outs
        res = rc.three_way(ref, a, b, rc.GRAD_KEYS if grads else rc.OUT_KEYS)
        if not grads:  # ... and step by step
            keys = rc.OUT_KEYS[:-1]
            for s in range(3):
                per = rc.three_way({k: ref[k][s:s + 1] for k in keys}, {k: a[k][s:s + 1] for k in keys}, {k: b[k][s:s + 1] for k in keys}, keys)
                res.update({f"{k}[{s}]": v for k, v in per.items()})
        return res

    def check(self, name, grads=False, targets=None, K=None):
        """One launch on all sides at total_num_calls = K (None: the next one): the three integer outputs equal at every pixel, the floats under the
        comparison rule with every pixel in. No case leaves a pixel out; a failure lists the pixels the rule would allow to. Returns the three results."""
        outs = self.launch(grads, targets, K=K)
        ref, a, _ = outs
        rc.assert_integers(ref, a, name)
        res = self._compare(outs, grads)
        direct = max(float(np.nanmax(np.abs(np.asarray(ref[k], np.float64) - a[k].reshape(ref[k].shape))) / max(float(np.nanmax(np.abs(a[k]))), 1e-30)) for k in (rc.GRAD_KEYS if grads else rc.OUT_KEYS))
        rc.report(name + ("_grad" if grads else ""), worst_ratio=f"{rc.worst_ratio(res):.2f}", ref_vs_o32_rel=f"{direct:.1e}")
        assert not rc.failing(res), (name, rc.failing(res), "pixels the oracle flags:", rc.could_be_left_out(a))
        return outs

    def check_both(self, name, targets, K=5):
        out = self.check(name, False, K=K)
        self.check(name, True, targets, K=K)
        return out


def generic_targets(syn, W, H):
    """syn.make_targets with roughness / f0 moved off the scene's own wall values (as hip_common.generic_targets)."""
    tg = syn.make_targets(W, H)
    tg["roughness"] = tg["roughness"] + np.float32(0.23)
    tg["f0"] = tg["f0"] + np.float32(0.17)
    return tg


# ------------------------------------------------------------------------------------------------ 1. synthetic scenes
@pytest.mark.parametrize("jitter", [0, 1], ids=["jitter_off", "jitter_on"])
@pytest.mark.parametrize("bounces", [0, 1, 2])
@pytest.mark.parametrize("variant,n,size", [("trained", 400, (24, 16)), ("trained", 2000, (32, 24)), ("init", 400, (24, 16))])
def test_synthetic_scenes(orc, syn, variant, n, size, bounces, jitter):
    """Training loss weights, a no-grad and a grad launch."""
    W, H = size
    g = syn.make_scene(n, variant, seed=4)
    t = Trio(orc, g, syn.default_camera(), W, H, dict(jitter_primary_rays=jitter, num_bounces=bounces, **syn.TRAIN_LOSS_WEIGHTS))
    out = t.check_both(f"synthetic_{variant}_{n}_b{bounces}_j{jitter}", syn.make_targets(W, H), K=7)
    if variant == "trained" and bounces:
        assert np.any(out[0]["output_ray_direction"][bounces - 1] != 0)  # the chain did reach the last step somewhere


# ------------------------------------------------------------------------------------------------ 2. quirk scenes
def one_gaussian(s=0.3, o_act=0.1, b=0.2, t=3.0, raw_opacity=None):
    """test_oracle_known_answers._one_gaussian's scene: isotropic, scale s, at distance t on the +x axis, offset sideways by b."""
    return dict(rgb=np.array([[0.3, 0.6, 0.9]]), normal=np.array([[-1.0, 0, 0]]), f0=np.array([[0.04, 0.05, 0.06]]), roughness=np.array([[0.25]]),
                opacity=np.array([[logit(o_act) if raw_opacity is None else raw_opacity]]), scale=np.full((1, 3), math.log(s)), mean=np.array([[t, b, 0.0]]),
                rotation=np.array([[1.0, 0, 0, 0]]))


ONE_TARGETS = dict(diffuse=np.full((1, 1, 3), 0.5), specular=np.full((1, 1, 3), 0.1), depth=np.full((1, 1, 1), 2.0), normal=np.zeros((1, 1, 3)),
                   f0=np.full((1, 1, 3), 0.3), roughness=np.full((1, 1, 1), 0.6))
PRIMARY = dict(jitter_primary_rays=0, num_bounces=0)


def test_near_plane_q1(orc, syn):
    """Response point in front of znear, box reaching past it: counted in T_total, not composited."""
    cam = dict(syn.plus_x_camera(), znear=0.2)
    out = Trio(orc, one_gaussian(s=0.2, o_act=0.5, b=0.0, t=0.05), cam, 1, 1, PRIMARY).check_both("near_plane_q1", ONE_TARGETS)[0]
    assert out["num_accumulated"][0, 0] == 0 and out["num_traversed"][0, 0] == 1 and out["output_transmittance"][0, 0, 0, 0] == 1.0
    np.testing.assert_allclose(out["output_total_transmittance"][0, 0, 0, 0], 1 - MAX_ALPHA * 0.5, rtol=1e-6)


def test_near_and_far_plane_cut(orc, syn):
    """znear 1.5 / zfar 3.0 through the room (test_near_plane_cut_and_far_plane): candidates before the near plane and behind the far plane."""
    W, H = 32, 24
    cam = dict(syn.default_camera(), znear=np.float32(1.5), zfar=np.float32(3.0))
    t = Trio(orc, syn.make_scene(2000, "trained", seed=6), cam, W, H, dict(jitter_primary_rays=0, num_bounces=1, **GENERIC))
    out = t.check_both("near_far_cut", generic_targets(syn, W, H))[0]
    assert np.any(out["output_total_transmittance"][0] < out["output_transmittance"][0] - 1e-3)


def colinear(n, t, opacity, scale, seed=3):
    rng = np.random.default_rng(seed)
    return dict(rgb=rng.uniform(0.1, 0.9, (n, 3)), normal=np.tile(np.array([-1.0, 0, 0]), (n, 1)), f0=np.full((n, 3), 0.04), roughness=np.full((n, 1), 0.3),
                opacity=np.full((n, 1), logit(opacity)), scale=np.full((n, 3), math.log(scale)), mean=np.stack([t, np.zeros(n), np.zeros(n)], 1),
                rotation=np.tile(np.array([1.0, 0, 0, 0]), (n, 1)))


def test_more_than_sixteen_hits_in_batches(orc, syn):
    """40 co-linear Gaussians in shuffled order: three selection rounds of 16."""
    g = colinear(40, np.random.default_rng(3).permutation(40) * 0.1 + 1.0, 0.05, 0.02)
    out = Trio(orc, g, syn.plus_x_camera(), 1, 1, dict(transmittance_threshold=0.0, **PRIMARY)).check_both("forty_colinear", ONE_TARGETS)[0]
    assert out["num_accumulated"][0, 0] == 40


def test_composite_cap_of_99_batches_of_16(orc, syn):
    """A 1 x 1 image and 1600 coaxial Gaussians: 1584 are composited, the last 16 only count in T_total."""
    g = colinear(1600, 2.0 + 0.01 * np.arange(1600), 0.01, 1.5, seed=0)
    out = Trio(orc, g, syn.plus_x_camera(), 1, 1, dict(transmittance_threshold=0.0, **PRIMARY)).check_both("cap_1584", ONE_TARGETS)[0]
    assert out["num_accumulated"][0, 0] == 1584 and out["num_traversed"][0, 0] == 1600
    assert out["output_total_transmittance"][0, 0, 0, 0] < out["output_transmittance"][0, 0, 0, 0]


@pytest.mark.parametrize("reverse", [False, True], ids=["index_order", "reverse_order"])
def test_q3_tie_drop_at_batch_boundaries(orc, syn, reverse):
    """20 bit-identical copies of every Gaussian (test_q3_tie_drop_at_16_hit_batch_boundaries_matches_oracle, at 100 x 20 Gaussians): the strict `>` of
    the batch fill drops the 4 copies that tie with the 16th composited hit. How many are dropped does not depend on the order in which the
    candidates are met - every image and both counts agree with the oracle in either visiting order -; WHICH copies are dropped does: per-copy
    gradients follow the list order, their sums over the copies of a Gaussian do not."""
    W, H, n = 32, 24, 100
    g = syn.make_scene(n, "init", seed=13)
    g20 = {k: np.concatenate([v] * 20, 0) for k, v in g.items()}
    cfg = dict(transmittance_threshold=0.0, **PRIMARY, **GENERIC)
    tg = generic_targets(syn, W, H)
    t = Trio(orc, g20, syn.default_camera(), W, H, cfg, reverse_traversal=reverse)
    out = t.check("q3_ties_" + ("reverse" if reverse else "index"), K=5)
    na = out[0]["num_accumulated"]
    assert int(na.max()) >= 32 and np.all(na % 16 == 0), int(na.max())
    assert bool((out[0]["output_total_transmittance"][0] < 0.9 * out[0]["output_transmittance"][0]).any())  # the dropped copies still count in T_total
    if not reverse:
        t.check("q3_ties_index", True, tg, K=5)
    else:
        ref, a, b = t.launch(True, tg, K=5)
        fold = lambda x: {k: x[k].reshape(20, n, -1).sum(0)[None, None] for k in rc.GRAD_KEYS}  # noqa: E731  ([1,1,n,C]: three_way's tensor layout)
        res = rc.three_way(fold(ref), fold(a), fold(b), rc.GRAD_KEYS)
        assert not rc.failing(res), rc.failing(res)
        w = ref["total_weight"].reshape(20, n)
        # the list is walked newest entry first and the fill keeps the first 16 of a tie: the copies met FIRST are the ones dropped
        assert np.any((w[19] == 0) & (w[0] > 0)) and not np.any((w[0] == 0) & (w[19] > 0))  # visited last to first
        wa = a["total_weight"].reshape(20, n)
        assert np.any((wa[0] == 0) & (wa[19] > 0)) and not np.any((wa[19] == 0) & (wa[0] > 0))  # (the oracle met them first to last)


@pytest.mark.parametrize("reverse", [False, True], ids=["index_order", "reverse_order"])
def test_exact_depth_ties_inside_a_batch(orc, syn, reverse):
    """Two bit-identical copies of every Gaussian (test_exact_depth_ties_inside_a_batch_are_all_composited, at 2 x 1000): pairs never straddle a batch
    boundary, both copies are composited once, in either visiting order."""
    W, H = 32, 24
    g = syn.make_scene(1000, "init", seed=13)
    g2 = {k: np.concatenate([v, v], 0) for k, v in g.items()}
    t = Trio(orc, g2, syn.default_camera(), W, H, dict(jitter_primary_rays=0, num_bounces=2, **GENERIC), reverse_traversal=reverse)
    out = t.check("pair_ties_" + ("reverse" if reverse else "index"), K=5)[0]
    assert int(out["num_accumulated"].max()) > 16
    assert np.all(out["output_total_transmittance"] <= out["output_transmittance"] + 4e-6)


def test_opacity_at_or_below_alpha_threshold(orc, syn):
    """sigmoid(raw) around alpha_threshold, fp32 neighbour by neighbour: invisible at and below it, the faintest visible Gaussian just above."""
    raw0 = np.float32(logit(0.005))
    seen = []
    for k in range(-4, 5):
        raw = raw0
        for _ in range(abs(k)):
            raw = np.nextafter(raw, np.float32(np.inf if k > 0 else -np.inf))
        out = Trio(orc, one_gaussian(b=0.0, raw_opacity=float(raw)), syn.plus_x_camera(), 1, 1, PRIMARY).check_both(f"alpha_threshold_{k:+d}ulp", ONE_TARGETS)[0]
        seen.append(int(out["num_traversed"][0, 0]))
    assert seen[0] == 0 and seen[-1] == 1 and sorted(seen) == seen, seen
    out = Trio(orc, one_gaussian(b=0.0, o_act=0.004), syn.plus_x_camera(), 1, 1, PRIMARY).check("opacity_below_threshold")[0]
    assert out["num_traversed"][0, 0] == 0 and out["output_transmittance"][0, 0, 0, 0] == 1.0


def test_gaussian_behind_the_camera(orc, syn):
    """Centre behind the origin, box around it: the program runs (counted) and rejects."""
    out = Trio(orc, one_gaussian(s=0.3, o_act=0.5, b=0.0, t=-0.2), syn.plus_x_camera(), 1, 1, PRIMARY).check_both("behind_camera", ONE_TARGETS)[0]
    assert out["num_traversed"][0, 0] == 1 and out["output_transmittance"][0, 0, 0, 0] == 1.0


def test_downward_normals_nan_rays(orc, syn):
    """Normals exactly (0, 0, -1): the sampled direction is NaN, fmaxf zeroes the throughput, the NaN ray meets nothing. Same NaN positions
    (three_way asserts them), finite images."""
    W, H = 32, 24
    g = syn.make_scene(1500, "trained", seed=2)
    g["normal"][:] = np.array([0, 0, -1.0], np.float32)
    t = Trio(orc, g, syn.default_camera(), W, H, dict(jitter_primary_rays=0, **GENERIC))
    out = t.check_both("nan_rays", generic_targets(syn, W, H))[0]
    assert np.isnan(out["output_ray_direction"][0]).any() and not np.isnan(out["output_final"]).any()
    assert np.all(out["output_rgb"][1][np.isnan(out["output_ray_direction"][0]).any(-1)] == 0)


def test_transmittance_threshold_stop(orc, syn):
    """Two co-linear Gaussians, threshold above T after the first (test_truncated_pair_tail_renormalisation): the second only counts in T_total."""
    g = colinear(2, np.array([2.0, 3.0]), 0.5, 0.2)
    g["opacity"][1] = logit(0.7)
    out = Trio(orc, g, syn.plus_x_camera(), 1, 1, dict(transmittance_threshold=0.6, **PRIMARY)).check_both("threshold_stop", ONE_TARGETS)[0]
    assert out["num_accumulated"][0, 0] == 1 and out["num_traversed"][0, 0] == 2


def test_num_bounces_five_is_clamped(orc, syn):
    W, H = 24, 16
    g = syn.make_scene(400, "trained", seed=4)
    outs = [Trio(orc, g, syn.default_camera(), W, H, dict(jitter_primary_rays=0, num_bounces=nb, **GENERIC)).check_both(f"num_bounces_{nb}", generic_targets(syn, W, H))[0] for nb in (5, 2)]
    for k in rc.OUT_KEYS:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k


def test_backface_rejection_of_bounce_rays(orc, syn):
    """bounce_scenes.mirror_scene with the far blobs turned away from the mirror: the reflected rays meet them from behind, 3.5 to 5 units after
    they leave the mirror. backfacing_max_dist below all of these hits, between them, and above all of them."""
    W, H = 24, 16
    g, far = bs.mirror_scene(seed=0, dtype=np.float32)
    g["normal"][far] = -g["normal"][far]
    cam = bs.camera()
    cfg = dict(jitter_primary_rays=0, num_bounces=1, **bs.FD_CONFIG)
    base = Trio(orc, g, cam, W, H, cfg).launch()[1]
    tg = bs.targets_away_from(base, 1, dtype=np.float32)
    lit = {}
    for max_dist in (0.1, 4.25, 10.0):
        out = Trio(orc, g, cam, W, H, dict(cfg, backfacing_max_dist=max_dist)).check_both(f"backface_{max_dist}", tg)[0]
        lit[max_dist] = float((1.0 - out["output_total_transmittance"][1].astype(np.float64)).sum())
    assert lit[0.1] > 1.05 * lit[4.25] > 1.05 * 1.05 * lit[10.0], lit  # the threshold really sits below, between and above the hits


# ------------------------------------------------------------------------------------------------ 3. config scalars
@pytest.mark.parametrize("cfg", [dict(global_scale_factor=2.0), dict(exp_power=2.0), dict(global_scale_factor=0.5, exp_power=4.0, alpha_threshold=0.02)],
                         ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_scale_factor_and_exp_power(orc, syn, cfg):
    """The three configs of test_non_default_scale_factor_and_exp_power."""
    W, H = 32, 24
    t = Trio(orc, syn.make_scene(2000, "trained", seed=31), syn.default_camera(), W, H, dict(jitter_primary_rays=0, **GENERIC, **cfg))
    t.check_both("cfg_" + "_".join(f"{k}{v}" for k, v in cfg.items()), generic_targets(syn, W, H))


@pytest.mark.parametrize("cfg", [
    dict(num_bounces=1), dict(reflection_invalid_normal_threshold=0.2), dict(reflection_invalid_normal_threshold=0.99),
    dict(backfacing_max_dist=1.0, backfacing_invalid_normal_threshold=0.5), dict(eps_ray_surface_offset=0.05), dict(eps_min_roughness=0.3),
    dict(alpha_threshold=0.05), dict(transmittance_threshold=0.2), dict(transmittance_threshold=0.0), dict(eps_forward_normalization=1e-2),
    dict(eps_scale_grad=1e-3), dict(loss_weight_depth=0.0, loss_weight_specular=0.01), dict(loss_weight_diffuse=0.0, loss_weight_normal=0.0, loss_weight_f0=0.0, loss_weight_roughness=0.0),
], ids=lambda c: ",".join(f"{k}={v}" for k, v in c.items()))
def test_every_config_scalar(orc, syn, cfg):
    """The scalars of test_every_config_scalar_is_read_on_the_device, one change at a time (num_bounces=5: test_num_bounces_five_is_clamped)."""
    W, H = 32, 24
    c = dict(jitter_primary_rays=0, **GENERIC)
    c.update(cfg)
    t = Trio(orc, syn.make_scene(2000, "trained", seed=41), syn.default_camera(), W, H, c)
    t.check_both("cfg_scalar_" + ",".join(f"{k}={v}" for k, v in cfg.items()), generic_targets(syn, W, H))


# ------------------------------------------------------------------------------------------------ 4. sequences
def test_accumulating_launches_and_reset(orc, syn):
    """accumulate_samples with jitter: three image launches (a running mean of three jitter patterns), then a grad launch - it adds nothing to the
    sums, yet raytracer.cpp counts it, so the image launch after it divides by one more than it summed -, reset_accumulators, and one more."""
    W, H = 24, 16
    t = Trio(orc, syn.make_scene(1500, "trained", seed=4), syn.default_camera(), W, H, dict(accumulate_samples=1, num_bounces=2, **GENERIC))
    tg = generic_targets(syn, W, H)
    firsts = []
    for k in range(3):
        out = t.check(f"accumulate_{k}")[0]
        firsts.append(out["output_rgb"].copy())
        assert t.ref.accumulated_sample_count == k + 1
        np.testing.assert_allclose(out["output_final"][0], out["output_rgb"].sum(0), atol=1e-5)
    assert np.abs(firsts[1] - firsts[0]).max() > 1e-3
    t.check("accumulate_grad_launch", True, tg)
    assert t.ref.accumulated_sample_count == 4
    out = t.check("accumulate_after_grad_launch")[0]  # four samples summed, divided by five
    assert t.ref.accumulated_sample_count == 5
    t.call("reset_accumulators")
    assert t.ref.accumulated_sample_count == 0
    t.check("accumulate_after_reset")
    assert t.ref.total_num_calls == 6


def test_seeds_over_consecutive_launches(orc, syn):
    """seed = tea4(pixel, total_num_calls), advanced by the draws the pixel's chain makes: image and grad launches in a row, the counter never set."""
    W, H = 24, 16
    t = Trio(orc, syn.make_scene(400, "trained", seed=4), syn.default_camera(), W, H, dict(jitter_primary_rays=1, num_bounces=2, **GENERIC))
    seen = []
    for k, grads in enumerate([False, False, True, False]):
        ref, a, _ = t.launch(grads, generic_targets(syn, W, H))
        rc.assert_integers(ref, a, f"seeds_launch_{k}")
        assert t.ref.total_num_calls == k + 1
        seen.append(ref["random_seeds"].copy())
    assert all(np.any(seen[i] != seen[i + 1]) for i in range(3))


@pytest.mark.parametrize("bounces", [0, 2])
def test_parameters_changed_without_update_bvh(orc, syn, bounces):
    """test_update_bvh_snapshot_semantics: moved and recoloured Gaussians without update_bvh are traversed where they were, with their new colour
    (images and, with live scale / rotation, gradients: test_grad_launch_without_refit_reads_scale_and_rotation_live); after update_bvh, where they are."""
    W, H = 32, 24
    g = syn.make_scene(2000, "trained", seed=9)
    t = Trio(orc, g, syn.default_camera(), W, H, dict(jitter_primary_rays=0, num_bounces=bounces, **GENERIC))
    tg = generic_targets(syn, W, H)
    before = t.check("snapshot_before", K=3)[0]
    rng = np.random.default_rng(3)
    g2 = {k: v.copy() for k, v in g.items()}
    g2["mean"] += 0.3
    g2["rgb"] = 1.0 - g2["rgb"]
    g2["scale"] += rng.uniform(-0.3, 0.3, g2["scale"].shape).astype(np.float32)
    g2["rotation"] += rng.normal(0, 0.3, g2["rotation"].shape).astype(np.float32)
    t.set_gaussians(g2)
    stale = t.check_both("snapshot_stale", tg, K=3)
    assert np.array_equal(stale[0]["output_depth"][0], before["output_depth"][0]) and np.abs(stale[0]["output_rgb"][0] - before["output_rgb"][0]).max() > 0.05
    t.call("update_bvh")
    fresh = t.check_both("snapshot_fresh", tg, K=3)
    assert np.abs(fresh[0]["output_depth"][0] - before["output_depth"][0]).max() > 0.05


# ------------------------------------------------------------------------------------------------ 5. instance records
def test_instance_records(orc, syn):
    """Oracle.instances() against the reference kernel's transforms and visibility mask, and against the driver's fp64 inverse of them."""
    n = 500
    g = syn.random_blob_scene(n, seed=5)
    g["opacity"][::7] = -8.0  # sigmoid < alpha_threshold
    raw0 = np.float32(logit(0.005))
    for k in range(9):  # at the threshold, fp32 neighbour by neighbour
        raw = raw0
        for _ in range(abs(k - 4)):
            raw = np.nextafter(raw, np.float32(np.inf if k > 4 else -np.inf))
        g["opacity"][1 + 7 * k] = raw
    g["scale"][3] = -200.0  # exp underflows: size 0 on every axis -> invisible
    g["scale"][10, 1] = -200.0  # ... on one axis: still visible
    g["rotation"] *= np.random.default_rng(1).uniform(0.01, 100.0, (n, 1)).astype(np.float32)  # far from unit length
    for gsf in (1.0, 1.7):
        same = Trio(orc, g, syn.plus_x_camera(), 8, 8, dict(global_scale_factor=gsf))  # the oracle inverting the 3x4 like the driver: the same bits
        assert np.array_equal(same.ref.instances()[0], same.o32.instances()[0].astype(np.float32))
        vis = same.ref.instances()[2] != 0
        assert np.array_equal(same.ref.instances()[1][vis], same.o32.instances()[1].astype(np.float32)[vis], equal_nan=True)  # (NaN: the row with a zero size)
        t = Trio(orc, g, syn.plus_x_camera(), 8, 8, dict(global_scale_factor=gsf), inverse_from_transform=False)  # the oracle's own (analytic) inverse
        Mr, Wr, vr = t.ref.instances()
        M32, W32, _, v32 = t.o32.instances()
        M64, W64, _, _ = t.o64.instances()
        assert np.array_equal(vr != 0, v32 != 0)
        v = vr != 0
        assert not v[3] and v[10] and not v[0] and 0 < int(v[1:1 + 7 * 9:7].sum()) < 9
        as4 = lambda x: np.asarray(x)[None, None]  # noqa: E731
        res = rc.three_way({"M": as4(Mr)}, {"M": as4(M32)}, {"M": as4(M64)}, ["M"])
        ok = v & (np.arange(n) != 10)  # (a zero size has no inverse)
        res.update(rc.three_way({"W": as4(Wr[ok])}, {"W": as4(W32[ok])}, {"W": as4(W64[ok])}, ["W"]))
        # row by row, so that a large transform does not hide a small one
        for i in np.flatnonzero(ok):
            row = rc.three_way({"M": as4(Mr[i]), "W": as4(Wr[i])}, {"M": as4(M32[i]), "W": as4(W32[i])}, {"M": as4(M64[i]), "W": as4(W64[i])}, ["M", "W"])
            assert not rc.failing(row), (i, rc.failing(row))
        rc.report(f"instances_gsf{gsf}", worst_ratio=f"{rc.worst_ratio(res):.2f}")
        assert not rc.failing(res), rc.failing(res)


# ------------------------------------------------------------------------------------------------ 6. room scene
def test_room_scene_with_gradients(orc, syn):
    """bounce_scenes.room_scene: every bounce ray crosses the room and composites the far wall over several 16-hit batches."""
    W, H = 24, 16
    g = bs.room_scene(1500, seed=2, dtype=np.float32)
    cfg = dict(jitter_primary_rays=0, num_bounces=2, **bs.FD_CONFIG)
    t = Trio(orc, g, bs.camera(), W, H, cfg)
    out = t.check("room", K=5)
    assert int(out[1]["num_composited_per_step"][1:].max()) > 32 and np.mean(out[1]["effective_steps"] == 3) > 0.3
    t.check("room", True, bs.targets_away_from(out[1], 2, dtype=np.float32), K=5)


# ------------------------------------------------------------------------------------------------ 7. unit functions
N_UNIT = 10000


def _unit(name, ref, o32, o64):
    res = rc.three_way({name: np.asarray(ref)[None, None]}, {name: np.asarray(o32)[None, None]}, {name: np.asarray(o64)[None, None]}, [name])
    rc.report("unit_" + name, ratio=f"{res[name][4]:.2f}", ref_vs_o64=f"{res[name][1]:.2e}", o32_vs_o64=f"{res[name][2]:.2e}",
              ref_vs_o32=f"{float(np.nanmax(np.abs(np.asarray(ref, np.float64) - np.asarray(o32, np.float64)))):.2e}")
    assert not rc.failing(res), rc.failing(res)


def test_tea4_and_lcg_are_exact(orc):
    rng = np.random.default_rng(0)
    for a, b in np.concatenate([rng.integers(0, 2 ** 32, (N_UNIT, 2), dtype=np.uint64), [[0, 0], [2 ** 32 - 1, 2 ** 32 - 1], [767, 1]]]):
        assert R.tea4(int(a), int(b)) == orc.tea4(int(a), int(b))
    for seed in (0, 1, 0xFFFFFFFF, 123456789):
        assert R.lcg_sequence(seed, N_UNIT // 4) == orc.lcg_sequence(seed, N_UNIT // 4)
    vals, _ = R.rnd_sequence(42, 1000)
    ints, _ = R.lcg_sequence(42, 1000)
    assert vals == [np.float32(i) / np.float32(2 ** 24) for i in ints] and 0.0 <= min(vals) and max(vals) < 1.0


def test_argument_evaluation_order_pin(orc):
    """make_float2(rnd(seed) - 0.5f, rnd(seed) - 0.5f): the jitter's x offset is the FIRST draw in the built library (a compiler that evaluates
    arguments right to left would swap the two), and make_float2(rnd(seed), rnd(seed)) of the bounce sample follows the same rule: phi from the
    first draw, checked through a launch below."""
    W, H, fov = 8, 6, 0.8
    c2w = np.eye(3, dtype=np.float32)
    for (ix, iy, calls) in [(3, 2, 7), (0, 0, 1), (7, 5, 1000)]:
        seed = R.tea4(iy * W + ix, calls)
        d, after = R.primary_ray_direction(c2w, fov, True, ix, iy, W, H, seed)
        (u0, u1), st = R.rnd_sequence(seed, 2)
        assert after == st
        view = math.tan(fov / 2)
        x_first = W / H * view * (2 * (ix + (u0 - 0.5) + 0.5) / W - 1)
        y_second = view * (1 - 2 * (iy + (u1 - 0.5) + 0.5) / H)
        v = np.array([x_first, y_second, -1.0])
        assert np.abs(d - v / np.linalg.norm(v)).max() < 1e-6, (ix, iy)
        x_swapped = W / H * view * (2 * (ix + (u1 - 0.5) + 0.5) / W - 1)
        assert abs(x_swapped - x_first) > 1e-3  # (the two orders are told apart at these pixels)
        o = orc.Oracle(W, H)
        o.set_camera(np.zeros(3), c2w, fov)
        assert np.abs(o.primary_rays(jitter=True, total_num_calls=calls)[iy, ix] - d).max() < 1e-6


def test_bounce_sample_draw_order_in_a_launch(orc, syn):
    """One opaque mirror Gaussian, 1 x 1 image: the ray that leaves step 0 is sample_cook_torrance(N, V, roughness, (first draw, second draw))."""
    g = one_gaussian(s=0.5, o_act=0.99, b=0.0, t=2.0)
    g["roughness"][:] = 0.6
    g["f0"][:] = 0.5
    t = Trio(orc, g, syn.plus_x_camera(), 1, 1, dict(jitter_primary_rays=0, num_bounces=1))
    ref = t.check("bounce_draw_order", K=3)[0]
    (u0, u1), _ = R.rnd_sequence(R.tea4(0, 3), 2)
    n = ref["output_normal"][0, 0, 0].astype(np.float64)
    assert np.linalg.norm(n) > 0.7
    N, V, rough = n / np.linalg.norm(n), np.array([-1.0, 0, 0]), float(ref["output_roughness"][0, 0, 0, 0])
    d = ref["output_ray_direction"][0, 0, 0]
    first_then_second = R.sample_cook_torrance(N, V, rough, [u0, u1])[0]
    swapped = R.sample_cook_torrance(N, V, rough, [u1, u0])[0]
    assert np.abs(d - first_then_second).max() < 1e-5 and np.abs(d - swapped).max() > 1e-2, (d, first_then_second, swapped)


def _brdf_inputs(rng, n):
    """Unit normals and view vectors on the normal's side; edges: roughness at eps_min_roughness, grazing V, f0 of 0 and 1."""
    N = rng.normal(size=(n, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    N[:50] = [0.0, 0.0, 1.0]  # the other tangent frame (N.z >= 0.999)
    V = rng.normal(size=(n, 3))
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    V = np.where((V * N).sum(1, keepdims=True) < 0, V - 2 * N * (V * N).sum(1, keepdims=True), V)
    graze = slice(50, 250)  # grazing: N.V of 1e-4 .. 1e-2
    T = np.cross(N[graze], rng.normal(size=(200, 3)))
    T /= np.linalg.norm(T, axis=1, keepdims=True)
    c = 10.0 ** rng.uniform(-4, -2, (200, 1))
    V[graze] = np.sqrt(1 - c * c) * T + c * N[graze]
    rough = rng.uniform(0.01, 1.0, n)
    rough[250:450] = 0.01  # eps_min_roughness
    f0 = rng.uniform(0.0, 1.0, (n, 3))
    f0[450:500], f0[500:550] = 0.0, 1.0
    u = rng.uniform(0.0, 1.0, (n, 2))
    u[550:560, 1], u[560:570, 0] = 0.0, 0.0
    f = lambda x: np.ascontiguousarray(x, np.float32)  # noqa: E731
    return f(N), f(V), f(rough), f(f0), f(u)


def test_brdf_sample_and_weight(orc):
    N, V, rough, f0, u = _brdf_inputs(np.random.default_rng(11), N_UNIT)
    L = R.sample_cook_torrance(N, V, rough, u)
    _unit("sample_cook_torrance", L, orc.unit("sample_cook_torrance", N, V, rough, u), orc.unit("sample_cook_torrance", N, V, rough, u, double=True))
    assert np.isfinite(L).all()
    w = R.cook_torrance_weight(N, V, L, rough, f0)
    assert np.all(w[450:500] == 0)  # f0 == 0
    # per element as well: a weight is a ratio of small numbers at grazing angles, and a large one must not hide the others
    w32, w64 = orc.unit("cook_torrance_weight", N, V, L, rough, f0), orc.unit("cook_torrance_weight", N, V, L, rough, f0, double=True)
    _unit("cook_torrance_weight", w, w32, w64)
    quiet = np.abs(w64).max(1) < 10.0
    assert quiet.mean() > 0.9
    _unit("cook_torrance_weight_below_10", w[quiet], w32[quiet], w64[quiet])
    # the NaN direction of a downward normal, and what the weight makes of it
    Ln = R.sample_cook_torrance([[0, 0, -1.0]], [[0, 0.6, -0.8]], [0.2], [[0.3, 0.3]])
    assert np.all(np.isnan(Ln)) and np.all(R.cook_torrance_weight([[0, 0, -1.0]], [[0, 0.6, -0.8]], Ln, [0.2], [[0.04, 0.04, 0.04]]) == 0)


def test_scaling_factor_and_eval_gaussian(orc):
    rng = np.random.default_rng(12)
    thr = np.float32(0.005)
    op = rng.uniform(0.0, 1.0, N_UNIT).astype(np.float32)
    op[:4] = [thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0)), 1.0]
    at = np.full(N_UNIT, thr, np.float32)
    at[N_UNIT // 2:] = rng.uniform(0.001, 0.1, N_UNIT - N_UNIT // 2)
    p = rng.choice(np.array([1.0, 2.0, 3.0, 4.0], np.float32), N_UNIT)
    s = R.compute_scaling_factor(op, at, p)
    assert s[0] == 0 and s[2] == 0 and s[1] > 0
    assert np.array_equal(s == 0, op <= at)
    _unit("compute_scaling_factor", s, orc.unit("compute_scaling_factor", op, at, p), orc.unit("compute_scaling_factor", op, at, p, double=True))
    x = (rng.normal(size=(N_UNIT, 3)) * rng.uniform(0.0, 1.6, (N_UNIT, 1))).astype(np.float32)
    x[0] = 0.0
    _unit("eval_gaussian", R.eval_gaussian(x, p), orc.unit("eval_gaussian", x, p), orc.unit("eval_gaussian", x, p, double=True))


def test_activations_and_their_backward(orc):
    rng = np.random.default_rng(13)
    x = rng.normal(scale=3.0, size=N_UNIT).astype(np.float32)
    x[:8] = [0.0, -0.0, 1.0, np.nextafter(np.float32(1), np.float32(2)), np.nextafter(np.float32(0), np.float32(-1)), -200.0, 20.0, -88.0]  # (no larger argument: exp(88) would be the tensor's scale and hide everything else)
    gr = rng.normal(size=N_UNIT).astype(np.float32)
    for name in ("sigmoid", "relu", "clipped_relu", "exp"):
        y = R.activation(name, x)
        _unit(name, y, orc.unit("activation", x, which=name), orc.unit("activation", x, which=name, double=True))
        # the backward functions take the ACTIVATED value (and 0 and 1 are inside the clipped relu's pass band)
        _unit(name + "_backward", R.activation_backward(name, gr, y), orc.unit("activation_backward", gr, y, which=name), orc.unit("activation_backward", gr, y, which=name, double=True))
    assert np.array_equal(R.activation_backward("clipped_relu", np.ones(4, np.float32), np.array([0.0, 1.0, -1e-6, 1.000001], np.float32)), [1, 1, 0, 0])
    q = (rng.normal(size=(N_UNIT, 4)) * 10.0 ** rng.uniform(-2, 2, (N_UNIT, 1))).astype(np.float32)
    dq = rng.normal(size=(N_UNIT, 4)).astype(np.float32)
    _unit("normalize_act", R.normalize_act(q), orc.unit("normalize_act", q), orc.unit("normalize_act", q, double=True))
    # (gradients of quaternions of length 0.01 .. 100 span four decades: held to the rule decade by decade)
    ln = np.linalg.norm(q, axis=1)
    for lo in (0.0, 0.1, 1.0, 10.0):
        sel = (ln >= lo) & (ln < (lo * 10 if lo else 0.1))
        _unit(f"backward_normalize_act_len_from_{lo}", R.backward_normalize_act(dq[sel], q[sel]), orc.unit("backward_normalize_act", dq[sel], q[sel]), orc.unit("backward_normalize_act", dq[sel], q[sel], double=True))
