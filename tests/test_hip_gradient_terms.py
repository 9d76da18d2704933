"""Gradients per loss term, per bounce step and per gaussian: the HIP backward against the fp32 and the fp64 oracle where the suite's
whole-tensor bar (max-abs error < 1e-3 of the tensor's max-abs) cannot see it.

That bar is set by the primary step: the specular term alone is 6-24 % of the all-terms maximum, the second bounce step alone 1-3 %, and in a
third of the rows every component is below 1e-3 of its tensor's maximum - a bounce-step backward off by several per cent, or a gaussian whose
gradient has the wrong sign, passes it. Here
  * each loss term runs alone (the other five weights 0): tensors the term cannot feed are exactly 0 (backward_pass.cu:80-132), the 1e-3 bar is
    taken against THIS run's maximum, and on the pixels all three sides trace alike (hip_common.SequenceMatched) every component of every gaussian
    is held to |hip - o32| <= KAPPA * grad_abs32 + 1e-7 * max|o32| (grad_abs: the oracle's sum of |contribution| per component, a scale no
    cancellation shrinks) and HIP may be no further from the fp64 oracle than C_FP32 times the fp32 oracle is;
  * the second bounce step alone is the difference of a two- and a one-bounce launch with the specular target pinned far below every output;
  * the same bars hold when an image is traced as the eight ranks of a partition (help across waves does most of the backward there);
  * the forward outputs of those pixels are held per pixel and step, where PSNR would average a few bad pixels away.
Measured values are in the comments next to each bar and in the REPORT lines."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from hip_common import (BOTH_HELP_MODES, GRAD_KEYS, LOSS_WEIGHTS, SequenceMatched, cam_obj, generic_targets, make_pair, per_component_ratio, ren,  # noqa: F401
                        report, set_config_everywhere)

TERMS = ["diffuse", "depth", "normal", "f0", "roughness", "specular"]
# the gradient tensors a term cannot feed (backward_pass.cu:80-132 as egr_oracle.cpp backward_pass encodes it): dL_dnormal / df0 / droughness only
# see their own primary-step term (d_normal = dL_normal * weight, ...; bounce steps write none of them); dL_drgb sees the diffuse term on the
# primary step and the specular term on the bounce steps; depth feeds dL/dalpha only. Opacity, scale, mean, rotation (and total_weight) are fed by all.
ZERO = {"diffuse": ("dL_dnormal", "dL_df0", "dL_droughness"), "depth": ("dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness"),
        "normal": ("dL_drgb", "dL_df0", "dL_droughness"), "f0": ("dL_drgb", "dL_dnormal", "dL_droughness"),
        "roughness": ("dL_drgb", "dL_dnormal", "dL_df0"), "specular": ("dL_dnormal", "dL_df0", "dL_droughness"), "all": ()}

# per-component bar on clean pixels, |hip - o32| <= KAPPA * grad_abs32 + 1e-7 * max|o32|, against the fp32 oracle: the fp64 oracle's bounce rays leave
# from points up to 1e-3 away (GGX sampling amplifies the last bits of the accumulated normal), so on the bounce steps the fp32 oracle is as far from
# it as HIP is (kappa vs o64: 0.2-0.85 for both). Primary-step terms: measured 1.0e-5 ... 2.4e-5 (both help modes). Terms fed by the bounce steps
# (specular, all, the second step alone): measured 1.1e-3 (eight ranks, all), 1.2e-3 (trained), 2.3e-3 (eight ranks, specular), 2.9e-3 (step 2,
# trained), 6.2e-3 (init), 7.7e-3 (step 2, init); every one of them ALSO holds the 1e-3-of-max bar on the same pixels.
KAPPA_PRIMARY = 1e-4
KAPPA_BOUNCE = 1.5e-2
# HIP's worst per-component ratio against the fp64 oracle over the fp32 oracle's: measured 0.46-0.95 (primary terms), 1.000-1.001 (bounce terms)
C_FP32 = 1.05
MAX_UNCLEAN = {"trained": 1000, "init": 1320, "trained128": 3350, "fwd": 330}  # pixels not clean in pass 1; measured 946 / 3840, 1250 / 3072, 3179 / 12288,
# 301 / 6144 with another sequence or T_total (fwd). Most of them are clean against HIP and the fp32 oracle: the fp64 oracle's bounce rays leave from
# points 1e-3 away (GGX sampling amplifies the last bits of the accumulated normal), and the long-chain cloud composites other sequences at fp64
# per-step max-abs of every output vs the fp32 oracle on same-sequence pixels (jitter on, two bounces; measured in both help modes, in the comment)
FWD_BARS = {"output_rgb": (1e-5, 1e-4, 2e-4),                 # 3.0e-6, 2.1e-5, 4.9e-5
            "output_depth": (1e-5, 1e-4, 2e-3),               # 3.6e-6, 3.1e-5, 9.2e-4
            "output_normal": (1e-5, 2e-4, 1e-3),              # 4.4e-6, 4.5e-5, 3.8e-4
            "output_f0": (1e-5, 1e-4, 1e-3),                  # 2.4e-6, 2.1e-5, 3.0e-4
            "output_roughness": (1e-6, 1e-5, 1e-4),           # 2.2e-7, 2.0e-6, 2.8e-5
            "output_transmittance": (1e-6, 2e-5, 2e-4),       # 1.4e-7, 5.2e-6, 5.8e-5
            "output_total_transmittance": (1e-7, 1e-5, 1e-5), # 2.3e-8, 1.8e-6, 1.6e-6
            "output_final": (2e-4,)}                          # 5.0e-5


def _weights(term):
    if term == "all":
        return dict(LOSS_WEIGHTS)
    return {k: (v if k == "loss_weight_" + term else 0.0) for k, v in LOSS_WEIGHTS.items()}


_SCENES = {}


def _scene(ren, orc, syn, name, W, H, team_help, bounces=2, jitter=0):
    """(rt, o32, o64, targets, camera object) of one scene, built once per module and help mode."""
    key = (name, W, H, team_help, jitter)
    if key not in _SCENES:
        cam = syn.default_camera()
        if name.startswith("trained"):
            g = syn.make_scene(3000, "trained", seed=21)
        elif name == "init":  # the long-chain scene of test_backward_parity_long_bounce_chains
            g = syn.make_scene(4000, "init", seed=13)
            g["opacity"] = np.full_like(g["opacity"], np.log(0.35 / 0.65)).astype(np.float32)
        else:  # "fwd": the scene of test_forward_parity_with_bounces_and_jitter
            g = syn.make_scene(4000, "trained", seed=12)
        tg = generic_targets(syn, W, H)  # (targets moved off the walls' own values: sign(output - target) must not hang on the last bit)
        tg["normal"] = tg["normal"] + np.float32([0.11, -0.07, 0.05])
        tg["depth"] = tg["depth"] + np.float32(0.37)
        rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(jitter_primary_rays=jitter, num_bounces=bounces), team_help=team_help)
        o64 = orc.Oracle(W, H, double=True)
        o64.set_camera(cam["origin"], cam["c2w"], cam["fov"])
        o64.set_gaussians(g)
        o64.set_config(**o.config)
        o64.update_bvh()
        _SCENES[key] = (rt, o, o64, tg, cam)
    rt, o, o64, tg, cam = _SCENES[key]
    return rt, o, o64, dict(tg), cam


def _rel(x, ref, keys, scale=None):
    scale = ref if scale is None else scale
    return {k: float(np.abs(np.asarray(x[k], np.float64) - ref[k]).max() / np.abs(scale[k]).max()) for k in keys}


def _check_term(ren, syn, rt, o, o64, tg, cam, term, name, parts=((0, 1),), max_unclean=60):
    set_config_everywhere(rt, (o, o64), num_bounces=2, **_weights(term))
    sm = SequenceMatched(ren, rt, o, o64, cam_obj(ren, cam, tg), tg, parts=parts)
    p1, p2, clean = sm.run(max_unclean, name)
    # (a) what the term cannot feed is exactly zero, on HIP as on both oracles
    for k in ZERO[term]:
        for side in ("grad_h", "grad_32", "grad_64"):
            assert float(np.abs(p1[side][k]).max()) == 0.0, (name, side, k)
    live = [k for k in GRAD_KEYS if k not in ZERO[term]]
    for k in live:
        assert np.abs(p2["grad_64"][k]).max() > 0, (name, k)
    # (b) the suite's bar against this run's own maximum: all pixels and clean pixels
    err_all = _rel(p1["grad_h"], p1["grad_32"], live)
    err_clean = _rel(p2["grad_h"], p2["grad_32"], live)
    # (c) per component on clean pixels against the fp32 oracle (the same rays: the fp64 oracle's bounce rays leave from points up to 1e-3 away, and
    # the fp32 oracle is as far from it as HIP is), and per component no further from the fp64 oracle than the fp32 oracle is
    r_h = per_component_ratio(p2["grad_h"], p2["grad_32"], p2["abs32"])
    r_h64 = per_component_ratio(p2["grad_h"], p2["grad_64"], p2["abs64"])
    r_3264 = per_component_ratio(p2["grad_32"], p2["grad_64"], p2["abs64"])
    fmt = lambda d: {k: f"{v:.1e}" for k, v in d.items()}
    report(name, clean_pixels=int(clean.sum()), err_all_pixels=fmt(err_all), err_clean_pixels=fmt(err_clean), kappa_hip_vs_fp32=f"{r_h:.2e}",
           kappa_hip_vs_fp64=f"{r_h64:.2e}", kappa_fp32_oracle_vs_fp64=f"{r_3264:.2e}", hip_over_fp32=f"{r_h64 / max(r_3264, 1e-30):.3f}")
    assert max(err_all.values()) < 1e-3, (name, err_all)
    assert max(err_clean.values()) < 1e-3, (name, err_clean)
    assert r_h <= (KAPPA_PRIMARY if term in TERMS[:5] else KAPPA_BOUNCE), (name, r_h)
    assert r_h64 <= C_FP32 * r_3264, (name, r_h64, r_3264)
    return p1, p2, clean


@BOTH_HELP_MODES
@pytest.mark.parametrize("scene,term", [("trained", t) for t in TERMS] + [("init", "specular")])
def test_one_loss_term_at_a_time(ren, orc, syn, scene, term, team_help):
    W, H = (80, 48) if scene == "trained" else (64, 48)
    rt, o, o64, tg, cam = _scene(ren, orc, syn, scene, W, H, team_help)
    _check_term(ren, syn, rt, o, o64, tg, cam, term, f"gradient_terms_{scene}_{term}[help={int(team_help)}]", max_unclean=MAX_UNCLEAN[scene])


@BOTH_HELP_MODES
@pytest.mark.parametrize("scene", ["trained", "init"])
def test_second_bounce_step_alone(ren, orc, syn, scene, team_help):
    """Specular term only, target -10 (every residual of a bounce step has sign +1, whatever the number of bounces): the one- and the two-bounce
    launch share steps 0 and 1 exactly, so (2 bounces - 1 bounce) is what step 2 contributes - on HIP and on both oracles."""
    W, H = (80, 48) if scene == "trained" else (64, 48)
    rt, o, o64, tg, cam = _scene(ren, orc, syn, scene, W, H, team_help)
    tg["specular"] = np.full_like(tg["specular"], -10.0)
    name = f"second_bounce_step_{scene}[help={int(team_help)}]"
    runs, cleans = {}, []
    for nb in (2, 1):
        set_config_everywhere(rt, (o, o64), num_bounces=nb, **_weights("specular"))
        sm = SequenceMatched(ren, rt, o, o64, cam_obj(ren, cam, tg), tg)
        p1 = sm.trace(None)
        cleans.append(SequenceMatched.masks(p1)[1])
        runs[nb] = sm
    clean = cleans[0] & cleans[1]
    unclean = int(clean.size - clean.sum())
    report(name + "_pass1", not_clean=unclean)
    assert unclean <= MAX_UNCLEAN[scene], unclean
    p = {}
    for nb in (2, 1):
        set_config_everywhere(rt, (o, o64), num_bounces=nb)
        p[nb] = runs[nb].trace(clean)
    set_config_everywhere(rt, (o, o64), num_bounces=2)
    keys = ["dL_drgb", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation"]  # (normal / f0 / roughness: zero; total_weight: not a gradient)
    d = {side: {k: np.asarray(p[2][side][k], np.float64) - p[1][side][k] for k in GRAD_KEYS} for side in ("grad_h", "grad_32", "grad_64")}
    abs_sum = {k: p[2]["abs64"][k] + p[1]["abs64"][k] for k in GRAD_KEYS}
    share = {k: float(np.abs(d["grad_64"][k]).max() / np.abs(p[2]["grad_64"][k]).max()) for k in keys}
    for k in keys:
        assert np.abs(d["grad_64"][k]).max() > 0, k
    abs32 = {k: p[2]["abs32"][k] + p[1]["abs32"][k] for k in GRAD_KEYS}
    err = _rel(d["grad_h"], d["grad_32"], keys)
    err64 = _rel(d["grad_h"], d["grad_64"], keys)
    err3264 = _rel(d["grad_32"], d["grad_64"], keys)
    r_h = per_component_ratio(d["grad_h"], d["grad_32"], abs32)
    r_h64 = per_component_ratio(d["grad_h"], d["grad_64"], abs_sum)
    r_3264 = per_component_ratio(d["grad_32"], d["grad_64"], abs_sum)
    fmt = lambda x: {k: f"{v:.1e}" for k, v in x.items()}
    report(name, clean_pixels=int(clean.sum()), step2_share_of_specular_max=fmt(share), err_vs_own_max=fmt(err), err_vs_fp64=fmt(err64),
           fp32_oracle_err_vs_fp64=fmt(err3264), kappa_hip_vs_fp32=f"{r_h:.2e}", kappa_hip_vs_fp64=f"{r_h64:.2e}", kappa_fp32_oracle_vs_fp64=f"{r_3264:.2e}")
    assert max(err.values()) < 1e-3, err
    assert r_h <= KAPPA_BOUNCE, r_h
    assert r_h64 <= C_FP32 * r_3264, (r_h64, r_3264)
    for k in keys:
        assert err64[k] <= C_FP32 * err3264[k] + 1e-6, (k, err64[k], err3264[k])

@pytest.mark.parametrize("term", ["specular", "all"])
def test_under_filled_teams_eight_ranks_summed(ren, orc, syn, term):
    """Help on, the image traced as the eight ranks of a partition (set_partition(r, 8)), images tiled and gradients summed: every rank's launch is
    under-filled, and the bounce batches that waves without tiles take over through the ticket (k_backward_chain<4>) do most of the backward."""
    W, H = 128, 96
    rt, o, o64, tg, cam = _scene(ren, orc, syn, "trained128", W, H, True)
    _check_term(ren, syn, rt, o, o64, tg, cam, term, f"gradient_terms_eight_ranks_{term}", parts=[(r, 8) for r in range(8)],
                max_unclean=MAX_UNCLEAN["trained128"])


@BOTH_HELP_MODES
def test_forward_per_pixel(ren, orc, syn, team_help):
    """Every forward output, every step, per pixel, on the pixels whose rays composite the same sequences on all sides (reference defaults: jitter on,
    two bounces): a handful of pixel values off by 1e-2 would hide under the 50-70 dB PSNR bars of the bounce steps."""
    W, H = 96, 64
    rt, o, o64, tg, cam = _scene(ren, orc, syn, "fwd", W, H, team_help, jitter=1)
    set_config_everywhere(rt, (o, o64), num_bounces=2, **LOSS_WEIGHTS)
    sm = SequenceMatched(ren, rt, o, o64, cam_obj(ren, cam, tg), tg)
    p1 = sm.trace(None)
    same, clean = SequenceMatched.masks(p1)
    name = f"forward_per_pixel[help={int(team_help)}]"
    levels = {}
    for key in ("output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance", "output_total_transmittance", "output_final"):
        for s in range(p1["img_h"][key].shape[0]):
            dif = np.abs(p1["img_h"][key][s] - p1["img_32"][key][s]).max(axis=-1)
            levels[f"{key}[{s}]"] = float(dif[same].max())
    report(name, same_sequence_pixels=int(same.sum()), clean_pixels=int(clean.sum()), max_abs={k: f"{v:.1e}" for k, v in levels.items()})
    assert int(same.size - same.sum()) <= MAX_UNCLEAN["fwd"]
    assert (p1["ref32"]["effective_steps"] > 2).mean() > 0.3  # the second bounce is really exercised
    for key, bars in FWD_BARS.items():
        for st, bar in enumerate(bars):
            assert levels[f"{key}[{st}]"] <= bar, (key, st, levels[f"{key}[{st}]"], bar)
