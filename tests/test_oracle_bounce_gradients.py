"""fp64 finite-difference validation of the oracle's analytic backward ON THE BOUNCE STEPS (condition (iv) of test_oracle_gradients.py lifted).

Every HIP gradient test holds the kernels to the oracle; the oracle and the kernels were written from one reading of the reference's backward
(backward_pass.cu:80-220), so a misreading shared by both passes all of them. Here the oracle's bounce-step backward - the specular term,
throughput[step-1], the (1 - roughness[step-1])^3 down-weighting, one gaussian fed from several steps, the scale / rotation chain - is held to
central differences of a loss, which no reading of the backward enters.

The reference's backward treats every bounce ray, throughput and down-weight as a constant. It is therefore the exact gradient of
    L = l1_loss(step 0) + sum_{j>=1} w_spec/3 * D_j * sum_c s_c * output_rgb[j]_c      (oracle.frozen_chain_loss)
with the chain of a base launch held fixed (Oracle.set_frozen_chain: after each step the next ray, the throughput and the continue / break decision
come from the base launch, while every step's outputs are computed from the perturbed parameters), under (i) transmittance_threshold = 0,
(ii) loss_weight_depth = 0, (iii) no candidate straddling a clip boundary within the step. The bar is test_oracle_gradients.py's: err < 2e-5 of
max|fd| per tensor, over ALL rows of all eight tensors. test_mirror_scene_without_the_hook keeps the hook itself honest: there the rays of the
differentiated rows are frozen by the scene's construction and the loss itself, |spec - target| and all, is differentiated.

Two places where the analytic backward is NOT the derivative of that loss, on purpose (upstream's own formulas), are asserted as such at the end."""
import numpy as np
import pytest

import bounce_scenes as bs

EPS = 1e-6  # test_oracle_gradients.py's step
BAR = 2e-5  # test_oracle_gradients.py's bar, of max|fd| per tensor. Measured here (REPORT lines), worst tensor of each test: room scene 7.6e-8 (one
#             bounce, two bounces, jitter off; opacity), 4.5e-8 / 5.1e-8 (jitter on), every other tensor 2.9e-8 ... 3.2e-8, roughness 1.1e-9 ... 1.3e-9;
#             specular term alone 3.0e-8; exp_power 2: 3.2e-8; mirror scene without the hook 6.6e-8 (opacity; others 2.5e-8 ... 3.3e-8);
#             global_scale_factor 0.7: 6.1e-8, rotation * 0.7: 4.1e-8. (The floor of 3e-8 is the reference's float literal 1.0f / 3.0f in the
#             analytic backward against 1 / 3 in the loss.)
W, H = 5, 4
ROOM_N, ROOM_SEED = 250, 0


def report(name, **kv):
    print("REPORT " + name + ": " + ", ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


@pytest.fixture(autouse=True)
def one_thread(orc):
    """A launch here is 20 pixels, one block of the oracle's parallel loop: a thread team only spins. Restored for the tests that follow."""
    before = orc.lib().orc_max_threads()
    orc.lib().orc_set_threads(1)
    yield
    orc.lib().orc_set_threads(before)


def true_loss(orc, out, tg, cfg):
    """One bounce, nothing held constant and nothing linearised: l1_loss(step 0) + w_spec/3 * (1 - output_roughness[0])^3 * |output_rgb[1] -
    target_specular|, every factor taken from the launch `out` itself (the down-weighting is part of the loss whose gradient backward_pass.cu:11-13,
    :80-108 hard-codes; it multiplies the residual's sign there)."""
    assert int(cfg["num_bounces"]) == 1
    D = (1.0 - out["output_roughness"][0]) ** 3
    return orc.l1_loss(out, tg, cfg, 1) + cfg["loss_weight_specular"] / 3.0 * float((D * np.abs(out["output_rgb"][1] - tg["specular"])).sum())


def central_differences(o, g, loss, rows=None, keys=None):
    """{parameter: d loss / d parameter by central differences}, every component of the given rows (None: all). loss(out) -> float."""
    fd = {}
    for k in keys or bs.GRAD_OF:
        fd[k] = np.zeros_like(g[k])
        for i in (range(g[k].shape[0]) if rows is None else rows):
            for c in range(g[k].shape[1]):
                v = []
                for sgn in (+1.0, -1.0):
                    gp = dict(g)
                    gp[k] = g[k].copy()
                    gp[k][i, c] += sgn * EPS
                    v.append(loss(bs.launch(o, gp)))
                fd[k][i, c] = (v[0] - v[1]) / (2 * EPS)
    o.set_gaussians(g)
    o.update_bvh()
    return fd


def errors(fd, an, rows=None, factor=None):
    """per tensor: max |fd - analytic| over the rows, in units of max|fd| (test_oracle_gradients.py's measure)."""
    sl = slice(None) if rows is None else rows
    return {k: float(np.abs(fd[k][sl] - an[bs.GRAD_OF[k]][sl] * (factor or {}).get(k, 1.0)).max() / (np.abs(fd[k][sl]).max() + 1e-12)) for k in fd}


def room(orc, num_bounces, jitter, weights=None, n=ROOM_N, seed=ROOM_SEED, **cfg):
    """(oracle, gaussians, targets, base launch with gradients) of the room scene; the frozen chain of the base launch is NOT yet set."""
    g = bs.room_scene(n, seed=seed)
    c = dict(bs.FD_CONFIG, num_bounces=num_bounces, jitter_primary_rays=jitter)
    c.update(weights or {})
    c.update(cfg)
    o = bs.make_oracle(orc, g, bs.camera(0.5), W, H, **c)
    tg = bs.targets_away_from(bs.launch(o), num_bounces, seed=seed)
    base = bs.launch(o, grads=True, targets=tg)
    assert base["decision_margin"].min() > 100 * EPS  # (iii): no candidate within reach of a clip boundary, no pixel at the reflection threshold
    return o, g, tg, base


def assert_exercises_the_bounce_steps(orc, o, tg, base, num_bounces):
    """What the room scene is for, asserted before anything is differentiated."""
    steps = base["effective_steps"]
    assert np.mean(steps == num_bounces + 1) >= 0.5, steps  # at least half of the pixels run every step
    hits = base["num_composited_per_step"]
    assert hits[1:num_bounces + 1].max() > 16, hits.reshape(3, -1).max(axis=1)  # a bounce ray crosses the 16-hit batches of forward_pass.cu:55-87
    tw = {num_bounces: base["total_weight"][:, 0]}
    for nb in range(num_bounces):
        o.set_config(num_bounces=nb)
        tw[nb] = bs.launch(o, grads=True, targets=tg)["total_weight"][:, 0]
    o.set_config(num_bounces=num_bounces)
    per_step = np.stack([tw[0]] + [tw[nb] - tw[nb - 1] for nb in range(1, num_bounces + 1)])  # [steps, N]: weight a gaussian collects on each step
    fed_by = (per_step > 1e-6).sum(axis=0)
    assert fed_by.max() >= 2 and (fed_by >= 2).sum() >= 10, fed_by  # one gradient row summed from several steps
    return dict(all_steps=f"{int((steps == num_bounces + 1).sum())}/{steps.size}", hits_per_step=hits.reshape(3, -1).sum(axis=1).tolist(),
                max_hits_of_a_ray=hits.reshape(3, -1).max(axis=1).tolist(), gaussians_fed_by_two_steps=int((fed_by >= 2).sum()),
                by_three=int((fed_by >= 3).sum()))


def check_frozen_fd(orc, name, o, g, tg, base, factor=None):
    o.set_frozen_chain(orc.Oracle.frozen_chain_from(base))
    fd = central_differences(o, g, lambda out: orc.frozen_chain_loss(out, tg, o.config, base))
    err = errors(fd, base, factor=factor)
    report(name, **{k: f"{v:.1e}" for k, v in err.items()})
    for k, gk in bs.GRAD_OF.items():
        assert np.abs(fd[k]).max() > 0 or np.abs(base[gk]).max() == 0, k
        assert err[k] < BAR, (name, k, err)
    return fd, err


@pytest.mark.parametrize("double", [True, False], ids=["fp64", "fp32"])
@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("num_bounces", [1, 2])
def test_frozen_chain_of_the_base_launch_reproduces_it_exactly(orc, num_bounces, jitter, double):
    """The hook changes nothing but where the next ray comes from: with the table of a free launch, every output and every gradient of that launch
    comes out bit for bit - in both instantiations."""
    g = bs.room_scene(ROOM_N, seed=ROOM_SEED)
    o = bs.make_oracle(orc, g, bs.camera(0.5), W, H, double=double, **dict(bs.FD_CONFIG, num_bounces=num_bounces, jitter_primary_rays=jitter))
    tg = bs.targets_away_from(bs.launch(o), num_bounces)
    free = bs.launch(o, grads=True, targets=tg, abs_sums=True)
    assert np.any(free["effective_steps"] == num_bounces + 1) and np.any(free["effective_steps"] < num_bounces + 1)  # both decisions are replayed
    o.set_frozen_chain(orc.Oracle.frozen_chain_from(free))
    frozen = bs.launch(o, grads=True, targets=tg, abs_sums=True)
    o.set_frozen_chain(None)
    again = bs.launch(o, grads=True, targets=tg, abs_sums=True)
    assert set(frozen) == set(free)
    for other in (frozen, again):
        for k in free:
            if k == "grad_abs":
                for kk in free[k]:
                    assert np.array_equal(free[k][kk], other[k][kk]), kk
            else:
                assert np.array_equal(free[k], other[k]), k
    assert np.abs(free["dL_drgb"]).max() > 0 and free["output_throughput"][0].min() < 1.0


@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("num_bounces", [1, 2])
def test_room_backward_matches_frozen_chain_differences(orc, num_bounces, jitter):
    o, g, tg, base = room(orc, num_bounces, jitter)
    report(f"bounce_fd_room_scene[bounces={num_bounces},jitter={jitter}]", **assert_exercises_the_bounce_steps(orc, o, tg, base, num_bounces))
    check_frozen_fd(orc, f"bounce_fd_room[bounces={num_bounces},jitter={jitter}]", o, g, tg, base)


def test_specular_term_alone(orc):
    """The other five weights 0: nothing of the primary step's loss covers for the bounce steps, and dL_dnormal / df0 / droughness, which only the
    primary step's own terms feed (backward_pass.cu:80-132), are exactly zero - as are their finite differences under the frozen chain."""
    off = {k: 0.0 for k in bs.FD_CONFIG if k.startswith("loss_weight_") and k != "loss_weight_specular"}
    o, g, tg, base = room(orc, 2, 0, weights=off)
    fd, _ = check_frozen_fd(orc, "bounce_fd_room_specular_alone", o, g, tg, base)
    for k in ("normal", "f0", "roughness"):
        assert np.abs(base[bs.GRAD_OF[k]]).max() == 0.0 and np.abs(fd[k]).max() == 0.0, k
    for k in ("rgb", "opacity", "mean", "scale", "rotation"):
        assert np.abs(base[bs.GRAD_OF[k]]).max() > 0, k


def test_other_kernel_shape(orc):
    """exp_power = 2, alpha_threshold = 0.02 at global_scale_factor = 1: the d gaussval / d |x|^2 power and the clip radius in the geometry chain."""
    o, g, tg, base = room(orc, 2, 0, exp_power=2.0, alpha_threshold=0.02)
    assert np.mean(base["effective_steps"] == 3) >= 0.5 and base["num_composited_per_step"][1:].max() > 16
    check_frozen_fd(orc, "bounce_fd_room_exp_power_2", o, g, tg, base)


def test_mirror_scene_without_the_hook(orc):
    """Cross-check that never sets the hook: the bounce rays of a near-opaque mirror in front of the camera composite blobs BEHIND the camera, which
    no primary ray meets. Perturbing such a row leaves step 0 - hence every bounce ray, throughput, down-weight - untouched, so the loss itself
    (true_loss: |spec - target|, not its linearisation) is differentiated with the chain frozen by construction."""
    g, far = bs.mirror_scene()
    cfg = dict(bs.FD_CONFIG, num_bounces=1, jitter_primary_rays=0)
    o = bs.make_oracle(orc, g, bs.camera(0.25), W, H, **cfg)
    tg = bs.targets_away_from(bs.launch(o), 1)
    o.set_config(num_bounces=0)
    assert np.all(bs.launch(o, grads=True, targets=tg)["total_weight"][far] == 0.0)  # the primary rays cannot see the differentiated rows
    o.set_config(num_bounces=1)
    base = bs.launch(o, grads=True, targets=tg)
    assert base["decision_margin"].min() > 100 * EPS
    assert np.all(base["effective_steps"] == 2) and np.count_nonzero(base["total_weight"][far, 0] > 1e-3) >= far.size // 2
    keys = ["rgb", "opacity", "mean", "scale", "rotation"]  # (bounce steps feed no normal / f0 / roughness gradient: asserted zero below)
    fd = central_differences(o, g, lambda out: true_loss(orc, out, tg, o.config), rows=far)
    err = errors(fd, base, rows=far)
    report("bounce_fd_mirror_scene_no_hook", **{k: f"{v:.1e}" for k, v in err.items()})
    for k in keys:
        assert np.abs(fd[k][far]).max() > 0, k
        assert err[k] < BAR, (k, err)
    for k in ("normal", "f0", "roughness"):  # what a bounce step composites of them reaches no loss term: exactly zero, both ways
        assert np.abs(fd[k][far]).max() == 0.0 and np.abs(base[bs.GRAD_OF[k]][far]).max() == 0.0, k


def test_rotation_gradient_misses_global_scale_factor(orc):
    """Documents, not fixes: upstream's rotation line multiplies dL/dM by the RAW scale (backward_pass.cu:185-187), while M carries
    scale * scaling_factor * global_scale_factor and the scaling_factor alone is applied before (:161-167). With global_scale_factor != 1 the
    analytic dL_drotation is therefore fd / global_scale_factor - 0.3 / 0.7 = 0.43 of max|fd| off - and dL_drotation * global_scale_factor holds
    the bar; every other tensor holds it as it is."""
    gsf = 0.7
    o, g, tg, base = room(orc, 2, 0, global_scale_factor=gsf, exp_power=2.0, alpha_threshold=0.02, n=400)
    assert np.mean(base["effective_steps"] == 3) >= 0.5 and base["num_composited_per_step"][1:].sum() > 100
    fd, _ = check_frozen_fd(orc, "bounce_fd_room_global_scale_0.7_rotation_times_0.7", o, g, tg, base, factor={"rotation": gsf})
    raw = errors({"rotation": fd["rotation"]}, base)["rotation"]
    report("bounce_fd_room_global_scale_0.7_rotation_as_it_is", rotation=f"{raw:.3f}")
    assert abs(raw - (1.0 - gsf) / gsf) < 1e-3 * (1.0 - gsf) / gsf, raw


def test_no_gradient_flows_through_the_throughput(orc):
    """Documents, not fixes: hook off and the loss itself (true_loss), the mirror's own f0 and roughness move the throughput and the down-weight
    of everything its bounce rays see, and the analytic backward knows nothing of it (the reference treats both as constants): dL_df0 of the
    mirror rows is far from the finite differences - which is why the bounce steps can only be pinned with the chain frozen."""
    g, far = bs.mirror_scene()
    mirror = np.arange(far[0])
    cfg = dict(bs.FD_CONFIG, num_bounces=1, jitter_primary_rays=0)
    o = bs.make_oracle(orc, g, bs.camera(0.25), W, H, **cfg)
    tg = bs.targets_away_from(bs.launch(o), 1)
    base = bs.launch(o, grads=True, targets=tg)
    fd = central_differences(o, g, lambda out: true_loss(orc, out, tg, o.config), rows=mirror, keys=["f0", "roughness"])
    err = errors(fd, base, rows=mirror)
    report("bounce_fd_mirror_scene_unfrozen", **{k: f"{v:.2f}" for k, v in err.items()})
    assert err["f0"] > 0.1 and err["roughness"] > 0.1, err  # measured 0.53 and 1.01 of max|fd|: four orders of magnitude above BAR
    # ... and with the chain frozen the same rows hold the bar
    o.set_frozen_chain(orc.Oracle.frozen_chain_from(base))
    fz = central_differences(o, g, lambda out: orc.frozen_chain_loss(out, tg, o.config, base), rows=mirror, keys=["f0", "roughness"])
    o.set_frozen_chain(None)
    efz = errors(fz, base, rows=mirror)
    report("bounce_fd_mirror_scene_frozen", **{k: f"{v:.1e}" for k, v in efz.items()})
    assert max(efz.values()) < BAR, efz
