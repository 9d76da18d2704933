"""Bounce hits sum the local matrix Q like primary hits do, and the scale / rotation chain runs once per gaussian on the sum (k_grad_gather): the HIP
backward against the fp32 and the fp64 oracle on a scene where that chain has something to get wrong.

The stock synthetic cloud is near-isotropic with unit quaternions: its rotation gradients nearly cancel and the quaternion normalisation is the
identity. Here every axis of every gaussian is scaled by U(0.5, 2) and every raw quaternion multiplied by U(0.5, 2). At 96 x 64 with the reference's
defaults (jitter on, two bounces) 12 008 gaussians are hit by bounce rays only - their scale and rotation gradients come from bounce hits alone - and
3 123 by both kinds of ray (fp64 oracle); 6144 / 6004 / 4708 rays are live on the three steps.
  * the bars of test_hip_gradient_terms.py (1e-3 of each tensor's maximum, per-component kappa, no further from the fp64 oracle than C_FP32 times the
    fp32 oracle is) for the specular term alone and for all terms, in both help modes, the last one also on the scale / rotation rows of the gaussians
    only bounce rays hit; once more with eps_scale_grad = 1e-3, where the chain's denominators are not exp(scale) * sigma;
  * a bounce hit is still ONE gradient record;
  * a two-view training launch equals the sum of the two single launches.
The oracles' pass over all pixels is computed once per configuration and shared by the help modes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from hip_common import (BOTH_HELP_MODES, GRAD_KEYS, LOSS_WEIGHTS, OUT_KEYS, SequenceMatched, cam_obj, generic_targets, hip_grads, make_pair,  # noqa: F401
                        per_component_ratio, ren, report, set_config_everywhere, views)
from test_hip_gradient_terms import C_FP32, KAPPA_BOUNCE, ZERO, _rel, _weights
from test_hip_train_views import assert_grads_close, batched, sequential, view_targets

W, H, N = 96, 64, 20000
K = 1  # total_num_calls of every launch (jitter seeds): the launch the counts in this file's comments were taken on
# Cap on the pixels taken out in pass 1: the pixels the two ORACLES trace differently (SequenceMatched.masks' criterion applied to the fp32 against the fp64
# oracle - HIP has no say in it) times HEAD_ROOM. Measured: the oracles differ on 1321 of 6144 pixels (531 of them in their ordered hit sequence, the
# others in total transmittance or an output: the fp64 oracle's bounce rays leave from points 1e-3 away), cap 1651, HIP against both 1324 in both help modes.
HEAD_ROOM = 1.25
# Gradient records (get_counters()[13]) of the all-terms launch with help off, as the commit before bounce hits summed Q sent them: one per bounce hit,
# two per flushed table slot or primary hit without a slot. The primary step's share does not depend on what a bounce hit sends.
PARENT_RECORDS, PARENT_BOUNCE_HITS = 135561, 106427  # (29 134 = 2 x 14 567 flushed slots and primary hits without a slot)

_S = {}
_ORACLE_PASS1 = {}


def perturbed_scene(syn):
    g = syn.make_scene(N, "trained", seed=0)
    rng = np.random.default_rng(1)
    g["scale"] = (g["scale"] + np.log(rng.uniform(0.5, 2.0, (N, 3)))).astype(np.float32)
    g["rotation"] = (g["rotation"] * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32)
    return g


def _scene(ren, orc, syn, team_help):
    """(rt, o32, o64, targets, camera): one tracer per help mode, one pair of oracles for the module."""
    if "g" not in _S:
        _S["g"], _S["cam"] = perturbed_scene(syn), syn.default_camera()
        tg = generic_targets(syn, W, H)
        tg["normal"] = tg["normal"] + np.float32([0.11, -0.07, 0.05])
        tg["depth"] = tg["depth"] + np.float32(0.37)
        _S["tg"] = tg
    g, cam = _S["g"], _S["cam"]
    if ("rt", team_help) not in _S:
        rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(jitter_primary_rays=1, num_bounces=2), team_help=team_help)
        _S[("rt", team_help)] = rt
        if "o32" not in _S:
            o64 = orc.Oracle(W, H, double=True)
            o64.set_camera(cam["origin"], cam["c2w"], cam["fov"])
            o64.set_gaussians(g)
            o64.set_config(**o.config)
            o64.update_bvh()
            _S["o32"], _S["o64"] = o, o64
    return _S[("rt", team_help)], _S["o32"], _S["o64"], dict(_S["tg"]), cam


class SharedOracles(SequenceMatched):
    """SequenceMatched whose oracle results for the unmasked pass are computed once per configuration `key` and shared (read only)."""

    def __init__(self, *a, key, **kw):
        super().__init__(*a, **kw)
        self.key = key

    def _oracle(self, oo, mask, images, abs_sums):
        if mask is not None:
            return super()._oracle(oo, mask, images, abs_sums)
        k = (oo.double, self.key)
        if k not in _ORACLE_PASS1:
            _ORACLE_PASS1[k] = super()._oracle(oo, mask, images, abs_sums)
        return _ORACLE_PASS1[k]


def _oracles_differ(p1):
    """Pixels the fp32 and the fp64 oracle do not trace alike, by the criterion of SequenceMatched.masks: the cap's only input."""
    alike = np.all(p1["seq_32"] == p1["seq_64"], axis=0)
    alike &= np.all(np.abs(p1["img_32"]["output_total_transmittance"] - p1["img_64"]["output_total_transmittance"]) <= 2e-5, axis=(0, -1))
    for key in OUT_KEYS:
        if key not in ("output_ray_origin", "output_ray_direction"):
            alike &= ~np.any(np.abs(p1["img_32"][key] - p1["img_64"][key]) > 1e-3, axis=(0, -1))
    return int(alike.size - np.count_nonzero(alike))


def _hit_kinds(o64, tg, mask):
    """(bounce_only, both) [N] masks from the fp64 oracle: total_weight takes the weight of every hit whatever the loss, so a no-bounce launch tells
    the gaussians primary rays hit, and a gaussian whose total_weight grows with the bounces is hit by bounce rays."""
    tw = {}
    o64.set_pixel_mask(mask)
    try:
        for nb in (0, 2):
            o64.set_config(num_bounces=nb)
            o64.total_num_calls = K - 1
            tw[nb] = o64.raytrace(True, targets=tg)["total_weight"][:, 0]
    finally:
        o64.set_pixel_mask(None)
        o64.set_config(num_bounces=2)
    primary = tw[0] > 0
    return (tw[2] > 0) & ~primary, primary & (tw[2] > tw[0] * (1.0 + 1e-12))


def _rows_ratio(x, ref, abs_, rows, floor=1e-7):
    """per_component_ratio over the dL_dscale / dL_drotation rows `rows` only."""
    worst = 0.0
    for k in ("dL_dscale", "dL_drotation"):
        excess = (np.abs(np.asarray(x[k], np.float64) - ref[k]) - floor * float(np.abs(ref[k]).max()))[rows]
        fed = abs_[k][rows] > 0
        if np.any(excess[~fed] > 0):
            return float("inf")
        if np.any(fed):
            worst = max(worst, float((np.maximum(excess[fed], 0.0) / abs_[k][rows][fed]).max()))
    return worst


def _check(ren, orc, syn, term, team_help, eps):
    rt, o, o64, tg, cam = _scene(ren, orc, syn, team_help)
    name = f"bounce_q_{term}_eps{eps:g}[help={int(team_help)}]"
    set_config_everywhere(rt, (o, o64), num_bounces=2, eps_scale_grad=eps, **_weights(term))
    try:
        sm = SharedOracles(ren, rt, o, o64, cam_obj(ren, cam, tg), tg, K=K, key=(term, eps))
        p1 = sm.trace(None)
        same, clean = SequenceMatched.masks(p1)
        unclean, cap = int(clean.size - np.count_nonzero(clean)), int(HEAD_ROOM * _oracles_differ(p1))
        if "kinds" not in _S:  # the test's subject, on the oracle side: gaussians only bounce rays hit, and gaussians both kinds of ray hit
            _S["kinds"] = _hit_kinds(o64, tg, None)
        report(name + "_pass1", pixels=int(clean.size), not_clean=unclean, oracles_differ=_oracles_differ(p1), cap=cap,
               bounce_only_gaussians=int(_S["kinds"][0].sum()), gaussians_hit_by_both=int(_S["kinds"][1].sum()))
        assert _S["kinds"][0].sum() > 0 and _S["kinds"][1].sum() > 0
        assert unclean <= cap, (name, unclean, cap)
        p2 = sm.trace(clean)
        bounce_only, _ = _hit_kinds(o64, tg, clean)
        assert bounce_only.sum() > 0
    finally:
        set_config_everywhere(rt, (o, o64), num_bounces=2, eps_scale_grad=1e-12, **LOSS_WEIGHTS)
    for k in ZERO[term]:
        for side in ("grad_h", "grad_32", "grad_64"):
            assert float(np.abs(p1[side][k]).max()) == 0.0, (name, side, k)
    live = [k for k in GRAD_KEYS if k not in ZERO[term]]
    for k in live:
        assert np.abs(p2["grad_64"][k]).max() > 0, (name, k)
    err_clean = _rel(p2["grad_h"], p2["grad_32"], live)
    r_h = per_component_ratio(p2["grad_h"], p2["grad_32"], p2["abs32"])
    r_h64 = per_component_ratio(p2["grad_h"], p2["grad_64"], p2["abs64"])
    r_3264 = per_component_ratio(p2["grad_32"], p2["grad_64"], p2["abs64"])
    b_h64 = _rows_ratio(p2["grad_h"], p2["grad_64"], p2["abs64"], bounce_only)
    b_3264 = _rows_ratio(p2["grad_32"], p2["grad_64"], p2["abs64"], bounce_only)
    report(name, clean_pixels=int(clean.sum()), err_clean_pixels={k: f"{v:.1e}" for k, v in err_clean.items()}, kappa_hip_vs_fp32=f"{r_h:.2e}",
           kappa_hip_vs_fp64=f"{r_h64:.2e}", kappa_fp32_oracle_vs_fp64=f"{r_3264:.2e}", hip_over_fp32=f"{r_h64 / max(r_3264, 1e-30):.3f}",
           bounce_only_rows=int(bounce_only.sum()), scale_rot_bounce_only_hip_vs_fp64=f"{b_h64:.2e}", scale_rot_bounce_only_fp32_oracle_vs_fp64=f"{b_3264:.2e}")
    # measured (both help modes alike): worst tensor 6.1e-5 (dL_drgb), dL_dscale 5.4e-6 ... 2.3e-5, dL_drotation 1.2e-5 ... 1.6e-5; kappa against the fp32
    # oracle 1.33e-2 (specular) / 9.7e-3 (all); HIP / fp32 oracle against the fp64 oracle 0.996 over all rows and on the bounce-only scale / rotation rows
    assert max(err_clean.values()) < 1e-3, (name, err_clean)
    assert r_h <= KAPPA_BOUNCE, (name, r_h)
    assert r_h64 <= C_FP32 * r_3264, (name, r_h64, r_3264)
    assert b_h64 <= C_FP32 * b_3264, (name, b_h64, b_3264)


@BOTH_HELP_MODES
@pytest.mark.parametrize("term", ["specular", "all"])
def test_bounce_hits_sum_q(ren, orc, syn, term, team_help):
    _check(ren, orc, syn, term, team_help, 1e-12)


@BOTH_HELP_MODES
def test_bounce_hits_sum_q_with_eps_scale_grad(ren, orc, syn, team_help):
    """eps_scale_grad = 1e-3: the chain divides by exp(scale) * sigma + eps, which only k_grad_gather knows about now."""
    _check(ren, orc, syn, "all", team_help, 1e-3)


def test_a_bounce_hit_is_one_record(ren, orc, syn):
    rt, o, o64, tg, cam = _scene(ren, orc, syn, False)
    m = rt.cuda_module
    rt.zero_grad()
    m.get_metadata().total_num_calls.fill_(K - 1)
    ren.render(cam_obj(ren, cam, tg), rt)
    torch.cuda.synchronize()
    records = int(m.get_counters()[13])
    bounce_hits = int(m.debug_step_hits().numpy()[1:].sum())
    report("bounce_q_records", records=records, bounce_hits=bounce_hits, parent_records=PARENT_RECORDS, parent_bounce_hits=PARENT_BOUNCE_HITS)
    assert bounce_hits > 0
    assert records == bounce_hits + (PARENT_RECORDS - PARENT_BOUNCE_HITS), (records, bounce_hits)


def test_two_views_equal_the_sum_of_single_launches(ren, orc, syn):
    rt, o, o64, tg, cam = _scene(ren, orc, syn, False)
    m = rt.cuda_module
    tgs = view_targets(syn, W, H, 2)
    cams = [cam_obj(ren, c, t) for c, t in zip(views(syn, 2), tgs)]
    seq, work_s, st_s = sequential(ren, rt, cams, 40)
    bat, work_b, st_b = batched(ren, rt, cams, 40)
    assert st_s == 0 and st_b == 0 and np.array_equal(work_b, work_s) and work_b[1] > 0
    assert_grads_close(bat, seq, "bounce_q_train_views_vs_sequential")
