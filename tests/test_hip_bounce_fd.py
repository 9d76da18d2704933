"""The HIP backward on the bounce steps of never-truncated rays, against the gradient that finite differences have proven.

test_oracle_bounce_gradients.py holds the fp64 oracle's bounce-step backward to central differences of the frozen-chain loss on the room scene of
bounce_scenes.py at transmittance_threshold = 0, loss_weight_depth = 0. Here the same scene function, as fp32 parameters and at a size where the
chains have work (1000 blobs, 48x32 pixels: bounce rays composite up to ~90 hits, six of the 16-hit batches), runs through the HIP kernels with
two bounces, jitter off and on, in both help modes. In the `fd_weights` runs the fp64 side of every comparison below IS that proven gradient
(same scene function, same configuration, the oracle's Real = double instantiation); the `all_weights` runs add the depth term, whose geometry
gradient upstream does not propagate (test_oracle_gradients.py) and which therefore only the oracle defines.

No other GPU test launches a gradient with bounces and transmittance_threshold = 0: rays that are never truncated build the longest bounce-step
lists (extension blocks, the 99-batch cap). The bars are test_hip_gradient_terms.py's, unchanged: 1e-3 of the tensor's maximum on all pixels and
on clean pixels, KAPPA_BOUNCE per component against the fp32 oracle, and HIP no further from the fp64 oracle than C_FP32 times the fp32 oracle is."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import bounce_scenes as bs
from hip_common import (BOTH_HELP_MODES, GRAD_KEYS, LOSS_WEIGHTS, SequenceMatched, cam_obj, make_pair, per_component_ratio, ren, report,  # noqa: F401
                        set_config_everywhere)
from test_hip_gradient_terms import C_FP32, KAPPA_BOUNCE

W, H, N, SEED, FOV = 48, 32, 1000, 0, 0.9
WEIGHTS = {"fd_weights": {k: v for k, v in bs.FD_CONFIG.items() if k.startswith("loss_weight_")},  # LOSS_WEIGHTS with loss_weight_depth = 0
           "all_weights": dict(LOSS_WEIGHTS)}
# Pixels that are not clean: a CONDITION of the comparison, not a measurement of the kernels. Measured on the CPU with SequenceMatched.masks' logic on
# the two oracles alone (fp32 against fp64: other sequence, T_total 2e-5 apart or an output 1e-3 apart), of 1536 pixels: jitter off 10, jitter on 7,
# second step (two- and one-bounce launches, jitter off) 10. The cap is 10 % above that count, rounded up; HIP has no allowance of its own.
UNCLEAN_FP32_VS_FP64 = {"jitter0": 10, "jitter1": 7, "step2": 10}
MAX_UNCLEAN = {k: math.ceil(1.1 * v) for k, v in UNCLEAN_FP32_VS_FP64.items()}

_SIDES = {}


def cpu_sides(orc, jitter, num_bounces=2):
    """(gaussians, camera, fp32 oracle settings) shared with the CPU measurement of UNCLEAN_FP32_VS_FP64: scene, camera and configuration of the runs."""
    g = bs.room_scene(N, seed=SEED, dtype=np.float32)
    c = bs.camera(FOV)
    cam = dict(origin=c["origin"].astype(np.float32), c2w=c["c2w"].astype(np.float32), fov=np.float32(c["fov"]))
    cfg = dict(num_bounces=num_bounces, jitter_primary_rays=jitter, transmittance_threshold=0.0)
    return g, cam, cfg


def fp64_oracle(orc, g, cam, config):
    o64 = orc.Oracle(W, H, double=True)
    o64.set_camera(cam["origin"], cam["c2w"], cam["fov"])
    o64.set_gaussians(g)
    o64.set_config(**config)
    o64.update_bvh()
    return o64


def _sides(ren, orc, jitter, team_help):
    """(rt, o32, o64, targets, camera) of the room scene, built once per jitter and help mode."""
    key = (jitter, team_help)
    if key not in _SIDES:
        g, cam, cfg = cpu_sides(orc, jitter)
        rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(cfg, **WEIGHTS["fd_weights"]), team_help=team_help)
        o64 = fp64_oracle(orc, g, cam, o.config)
        tg = bs.targets_away_from(bs.launch(o64, K=5), 2, seed=SEED, dtype=np.float32)  # (K = 5: SequenceMatched's launches)
        _SIDES[key] = (rt, o, o64, tg, cam)
    rt, o, o64, tg, cam = _SIDES[key]
    return rt, o, o64, dict(tg), cam


def _rel(x, ref, keys):
    return {k: float(np.abs(np.asarray(x[k], np.float64) - ref[k]).max() / np.abs(ref[k]).max()) for k in keys}


@BOTH_HELP_MODES
@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("weights", ["fd_weights", "all_weights"])
def test_room_scene_two_bounces_never_truncated(ren, orc, weights, jitter, team_help):
    """fd_weights: the fp64 side is the gradient test_oracle_bounce_gradients.py has proven against finite differences on this scene function and
    configuration (transmittance_threshold = 0, loss_weight_depth = 0). NOT YET MEASURED on an MI355X: the levels are printed in the REPORT lines
    (pytest -s) and belong next to the bars below once a run has produced them."""
    rt, o, o64, tg, cam = _sides(ren, orc, jitter, team_help)
    set_config_everywhere(rt, (o, o64), num_bounces=2, **WEIGHTS[weights])
    name = f"bounce_fd_hip_{weights}[jitter={jitter},help={int(team_help)}]"
    sm = SequenceMatched(ren, rt, o, o64, cam_obj(ren, cam, tg), tg)
    p1, p2, clean = sm.run(MAX_UNCLEAN[f"jitter{jitter}"], name)
    assert rt.cuda_module.get_counters()[11] == 0  # no capacity overflow (also asserted after every launch inside SequenceMatched)
    steps, hits = p1["ref32"]["effective_steps"], p1["ref32"]["num_composited_per_step"]
    assert np.mean(steps == 3) >= 0.5  # at least half of the pixels run every step
    assert np.mean(hits[1:][:, steps == 3] > 16) >= 0.5 and hits[1:].max() > 64  # most bounce lists cross the 16-hit batches, some several times
    live = list(GRAD_KEYS)
    for k in live:
        assert np.abs(p2["grad_64"][k]).max() > 0, (name, k)
    err_all = _rel(p1["grad_h"], p1["grad_32"], live)
    err_clean = _rel(p2["grad_h"], p2["grad_32"], live)
    r_h = per_component_ratio(p2["grad_h"], p2["grad_32"], p2["abs32"])
    r_h64 = per_component_ratio(p2["grad_h"], p2["grad_64"], p2["abs64"])
    r_3264 = per_component_ratio(p2["grad_32"], p2["grad_64"], p2["abs64"])
    fmt = lambda d: {k: f"{v:.1e}" for k, v in d.items()}
    report(name, clean_pixels=int(clean.sum()), max_hits_of_a_bounce_ray=int(hits[1:].max()), err_all_pixels=fmt(err_all), err_clean_pixels=fmt(err_clean),
           kappa_hip_vs_fp32=f"{r_h:.2e}", kappa_hip_vs_fp64=f"{r_h64:.2e}", kappa_fp32_oracle_vs_fp64=f"{r_3264:.2e}",
           hip_over_fp32=f"{r_h64 / max(r_3264, 1e-30):.3f}")
    assert max(err_all.values()) < 1e-3, (name, err_all)
    assert max(err_clean.values()) < 1e-3, (name, err_clean)
    assert r_h <= KAPPA_BOUNCE, (name, r_h)
    assert r_h64 <= C_FP32 * r_3264, (name, r_h64, r_3264)


@BOTH_HELP_MODES
def test_second_bounce_step_alone_never_truncated(ren, orc, team_help):
    """test_hip_gradient_terms.test_second_bounce_step_alone at transmittance_threshold = 0: specular term only, target -10 (every residual of a
    bounce step has sign +1, whatever the number of bounces), so the one- and the two-bounce launch share steps 0 and 1 exactly and their
    difference is what step 2 contributes - on HIP and on both oracles."""
    rt, o, o64, tg, cam = _sides(ren, orc, 0, team_help)
    tg["specular"] = np.full_like(tg["specular"], -10.0)
    spec_only = {k: (v if k == "loss_weight_specular" else 0.0) for k, v in LOSS_WEIGHTS.items()}
    name = f"bounce_fd_hip_second_step[help={int(team_help)}]"
    runs, cleans = {}, []
    for nb in (2, 1):
        set_config_everywhere(rt, (o, o64), num_bounces=nb, **spec_only)
        sm = SequenceMatched(ren, rt, o, o64, cam_obj(ren, cam, tg), tg)
        p1 = sm.trace(None)
        cleans.append(SequenceMatched.masks(p1)[1])
        runs[nb] = sm
    clean = cleans[0] & cleans[1]
    unclean = int(clean.size - clean.sum())
    report(name + "_pass1", not_clean=unclean, cap=MAX_UNCLEAN["step2"])
    assert unclean <= MAX_UNCLEAN["step2"], unclean
    p = {}
    for nb in (2, 1):
        set_config_everywhere(rt, (o, o64), num_bounces=nb)
        p[nb] = runs[nb].trace(clean)
    set_config_everywhere(rt, (o, o64), num_bounces=2)
    assert rt.cuda_module.get_counters()[11] == 0
    keys = ["dL_drgb", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation"]  # (normal / f0 / roughness: zero; total_weight: not a gradient)
    d = {side: {k: np.asarray(p[2][side][k], np.float64) - p[1][side][k] for k in GRAD_KEYS} for side in ("grad_h", "grad_32", "grad_64")}
    abs64 = {k: p[2]["abs64"][k] + p[1]["abs64"][k] for k in GRAD_KEYS}
    abs32 = {k: p[2]["abs32"][k] + p[1]["abs32"][k] for k in GRAD_KEYS}
    for k in keys:
        assert np.abs(d["grad_64"][k]).max() > 0, k
    share = {k: float(np.abs(d["grad_64"][k]).max() / np.abs(p[2]["grad_64"][k]).max()) for k in keys}
    err = _rel(d["grad_h"], d["grad_32"], keys)
    err64 = _rel(d["grad_h"], d["grad_64"], keys)
    err3264 = _rel(d["grad_32"], d["grad_64"], keys)
    r_h = per_component_ratio(d["grad_h"], d["grad_32"], abs32)
    r_h64 = per_component_ratio(d["grad_h"], d["grad_64"], abs64)
    r_3264 = per_component_ratio(d["grad_32"], d["grad_64"], abs64)
    fmt = lambda x: {k: f"{v:.1e}" for k, v in x.items()}
    report(name, clean_pixels=int(clean.sum()), step2_share_of_specular_max=fmt(share), err_vs_own_max=fmt(err), err_vs_fp64=fmt(err64),
           fp32_oracle_err_vs_fp64=fmt(err3264), kappa_hip_vs_fp32=f"{r_h:.2e}", kappa_hip_vs_fp64=f"{r_h64:.2e}", kappa_fp32_oracle_vs_fp64=f"{r_3264:.2e}")
    assert max(err.values()) < 1e-3, err
    assert r_h <= KAPPA_BOUNCE, r_h
    assert r_h64 <= C_FP32 * r_3264, (r_h64, r_3264)
    for k in keys:
        assert err64[k] <= C_FP32 * err3264[k] + 1e-6, (k, err64[k], err3264[k])
