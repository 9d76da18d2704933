"""What a launch that runs out of one of the tracer's two fixed capacities still guarantees (include/egr_raytracer.h: EGR_STATUS_*).

A. The composited-hit arena (ppll_backward_size). A wave takes arena blocks while it composites; a (task, step) - one 8x8 tile on one bounce step - that
   needs a block the arena no longer has stops recording: the backward skips it, the forward's results are those of a launch that fits. So an overflowing
   grad launch leaves EXACTLY the gradient of its recorded (task, step)s, and the next launch starts clean. Which (task, step)s are recorded is a race on
   the bump counter: every test reads the recorded set from the launch it checks (debug_step_hits = the S_NHITS the backward reads) and restates the
   launch on a tracer whose arena fits, with debug_set_pixel_mask on the recorded tiles.
B. Waves take arena blocks in runs of 8: what a launch takes is at most what it writes + 7 per wave, and a capacity of that + 8 fits.
C. The candidate scratch (ppll_forward_size): 64-entry runs per ray, longer lists continue in one extension block per ray while the pool lasts. A ray
   whose list fits its own run is untouched by its neighbours' overflow; the others lose candidates (flagged), never write out of bounds.

Tasks are pinned to 8x8 pixels (set_rays_per_task(64)) wherever a test reasons about tiles; no budget is below the floors the library enforces."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from hip_common import (BOTH_HELP_MODES, GRAD_KEYS, LOSS_WEIGHTS, OUT_KEYS, cam_obj, generic_targets, hip_grads, hip_outputs, make_pair, ren, report,  # noqa: F401
                        run_grad, set_config_everywhere, tracer, views)

W, H = 96, 64
TY, TX = H // 8, W // 8
TASKS = TY * TX                   # 96 tasks of 8x8 pixels
WAVES = -(-TASKS // 16) * 16      # the forward chain's wave slots for an image this small: whole teams of 16 (egr_trace_alloc: num_slots)
ENTRIES_PER_BLOCK = 256           # one arena block = 9 rows x 64 lanes x 16 B = 9216 B = 256 entries of ppll_backward_size (36 B each)
FLOOR_BWD = 1000                  # -> the 64-block floor
BIG_BWD = 50_000_000
K = 7                             # total_num_calls of every compared launch (jitter and bounce sampling draw from it)
SCENE = dict(N=4000, variant="init", seed=13)  # opacity 0.1: 2-8 blocks per tile on the primary step, ~450 (no bounces) / ~670 (two bounces) per launch


def _tiles(a):
    """[..., H, W] -> [..., TY, TX, 64]: the pixels of every 8x8 task."""
    a = np.asarray(a)
    lead = a.shape[:-2]
    return a.reshape(lead + (TY, 8, TX, 8)).swapaxes(-3, -2).reshape(lead + (TY, TX, 64))


def _pixels(task_mask):
    """[TY, TX] bool -> [H, W] bool."""
    return np.repeat(np.repeat(np.asarray(task_mask, bool), 8, axis=0), 8, axis=1)


def _bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _mk(ren, syn, bwd, team_help=False, fwd=8_000_000):
    rt = tracer(ren, syn, W, H, fwd=fwd, bwd=bwd, team_help=team_help, **SCENE)
    rt.cuda_module.set_rays_per_task(64)
    return rt


_BIG = {}


def _big(ren, syn, team_help=False):
    """The tracer whose arena fits, one per help mode for the module (every test sets the config scalars it relies on)."""
    if team_help not in _BIG:
        _BIG[team_help] = _mk(ren, syn, BIG_BWD, team_help)
    return _BIG[team_help]


def _configure(tracers, oracles=(), **cfg):
    full = dict(LOSS_WEIGHTS, num_bounces=2, jitter_primary_rays=1)
    full.update(cfg)
    for rt in tracers:
        set_config_everywhere(rt, oracles, **full)


def _grad_launch(ren, rt, camera, mask=None):
    """One grad launch into zeroed gradients at total_num_calls = K; `mask` [H,W]: the pixels traced. The debug exports are read from an unmasked
    launch only (they describe the pixels the export kernel sees)."""
    m = rt.cuda_module
    if mask is not None:
        m.debug_set_pixel_mask(torch.from_numpy(np.ascontiguousarray(mask, dtype=np.uint8)).cuda())
    try:
        m.get_metadata().total_num_calls.fill_(K - 1)
        run_grad(ren, rt, camera)
    finally:
        if mask is not None:
            m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
    out = dict(c=[int(x) for x in m.get_counters()], grads=hip_grads(rt))
    if mask is None:
        st, md = m.get_stats(), m.get_metadata()
        out.update(hits=m.debug_step_hits().numpy().copy(), seq=m.debug_hit_sequence_hash().numpy().copy(),
                   acc=st.num_accumulated_per_pixel.cpu().numpy(), trav=st.num_traversed_per_pixel.cpu().numpy(), seeds=md.random_seeds.cpu().numpy())
    return out


def _image_launch(rt, camera):
    m = rt.cuda_module
    m.get_metadata().total_num_calls.fill_(K - 1)
    with torch.no_grad():
        rt(camera)
    torch.cuda.synchronize()
    return int(m.get_counters()[11]), hip_outputs(rt)


def _recorded_sets(small, big):
    """All-or-nothing per (task, step), from the hit counts the backward reads. Returns (has, rec), both [3, TY, TX]: the (task, step)s that composite
    anything in the launch that fits, and those the overflowing launch recorded (a (task, step) without hits needs no block: recorded)."""
    hs, hb = small["hits"], big["hits"]
    per_pixel = (hs == hb) | (hs == 0)
    assert per_pixel.all(), ("a pixel's recorded hit count is neither the full one nor 0", np.argwhere(~per_pixel)[:8].tolist())
    ts, tb = _tiles(hs), _tiles(hb)
    has = tb.max(-1) > 0
    rec, dropped = (ts == tb).all(-1), (ts == 0).all(-1)
    assert (rec | dropped).all(), ("a (task, step) recorded in part", np.argwhere(~(rec | dropped))[:8].tolist())
    return has, rec


def _check_chains(small, big, has, rec):
    """The arena chains the backward walks: the launch that fits' sequence on a recorded (task, step), nothing on a dropped one."""
    ss, sb = _tiles(small["seq"]), _tiles(big["seq"])
    r, d = has & rec, has & ~rec
    assert np.array_equal(ss[r], sb[r]), "a recorded (task, step) walks another hit sequence"
    assert not ss[d].any(), "a dropped (task, step) still has an arena chain"


def _check_forward_untouched(small, big):
    for key in ("acc", "trav", "seeds"):
        assert _bit_equal(small[key], big[key]), key
    assert small["c"][0:3] == big["c"][0:3] and small["c"][6:9] == big["c"][6:9], (small["c"][:9], big["c"][:9])


def _rel(a, b, scale=None):
    """Per tensor: max |a - b| over the max-abs of `scale` (default b). A tensor that is zero in both is 0."""
    out = {}
    for k in GRAD_KEYS:
        s = float(np.abs(b[k] if scale is None else scale[k]).max())
        d = float(np.abs(np.asarray(a[k], np.float64) - b[k]).max())
        assert s > 0 or d == 0, (k, d)
        out[k] = d / s if s > 0 else 0.0
    return out


def _fmt(d):
    return {k: f"{v:.1e}" for k, v in d.items()}


# ------------------------------------------------------------------------------------------------ A: the hit arena
def test_a1_recorded_or_dropped_per_task_and_step_forward_untouched(ren, syn):
    """Reference defaults (jitter, two bounces), the 64-block floor against an arena that fits. Only what the header states is asserted about the
    counters: the floor launch takes more blocks than it holds (arena_blocks_used counts every block taken from the bump counter)."""
    cam = syn.default_camera()
    camera = cam_obj(ren, cam, generic_targets(syn, W, H))
    small, big = _mk(ren, syn, FLOOR_BWD), _big(ren, syn)
    _configure((small, big))
    ls, lb = _grad_launch(ren, small, camera), _grad_launch(ren, big, camera)
    assert lb["c"][11] == 0 and ls["c"][11] & 2, (lb["c"][11], ls["c"][11])
    assert ls["c"][16] == 64 and lb["c"][15] >= 300, (ls["c"][16], lb["c"][15])  # the floor; the scene needs several hundred blocks
    has, rec = _recorded_sets(ls, lb)
    n_rec, n_drop = int((has & rec).sum()), int((has & ~rec).sum())
    report("overflow_a1", task_steps_with_hits=int(has.sum()), recorded=n_rec, dropped=n_drop, blocks_taken=ls["c"][15], blocks_cap=ls["c"][16], blocks_needed=lb["c"][15])
    assert n_rec > 0 and n_drop > 0, (n_rec, n_drop)
    _check_chains(ls, lb, has, rec)
    _check_forward_untouched(ls, lb)


@BOTH_HELP_MODES
def test_a2_gradients_are_those_of_the_recorded_tasks(ren, orc, syn, team_help):
    """No bounces, jitter on: the overflowing launch against the launch that fits and against the oracle, both restricted to the recorded tiles R (tiles
    without any hit are in R: they feed nothing on either side). Bars: float-atomic order (1e-5 of the tensor's max-abs) against the masked launch, the
    project's 1e-3 against the masked oracle; and the UNMASKED launch must be further than 1e-3 away, or the mask would prove nothing."""
    cam = syn.default_camera()
    tg = generic_targets(syn, W, H)
    camera = cam_obj(ren, cam, tg)
    small, o = make_pair(ren, orc, syn.make_scene(SCENE["N"], SCENE["variant"], seed=SCENE["seed"]), cam, W, H, bwd=FLOOR_BWD, team_help=team_help)
    small.cuda_module.set_rays_per_task(64)
    big = _big(ren, syn, team_help)
    _configure((small, big), (o,), num_bounces=0)
    ls, lb = _grad_launch(ren, small, camera), _grad_launch(ren, big, camera)
    assert lb["c"][11] == 0 and ls["c"][11] & 2
    has, rec = _recorded_sets(ls, lb)
    assert (has[0] & rec[0]).any() and (has[0] & ~rec[0]).any()
    R = _pixels(rec[0])
    masked = _grad_launch(ren, big, camera, mask=R)
    assert masked["c"][11] == 0 and masked["c"][0] == int(R.sum())
    o.set_pixel_mask(R)
    try:
        o.total_num_calls = K - 1
        ref = o.raytrace(True, targets=tg)
    finally:
        o.set_pixel_mask(None)
    e_masked, e_oracle, e_unmasked = _rel(ls["grads"], masked["grads"]), _rel(ls["grads"], ref), _rel(ls["grads"], lb["grads"])
    report(f"overflow_a2[help={int(team_help)}]", recorded_tiles=int((has[0] & rec[0]).sum()), dropped_tiles=int((has[0] & ~rec[0]).sum()),
           vs_masked_launch=f"{max(e_masked.values()):.1e}", vs_masked_oracle=f"{max(e_oracle.values()):.1e}", vs_unmasked_launch=f"{max(e_unmasked.values()):.1e}")
    assert max(e_masked.values()) < 1e-5, _fmt(e_masked)
    assert max(e_oracle.values()) < 1e-3, _fmt(e_oracle)
    assert max(e_unmasked.values()) > 1e-3, _fmt(e_unmasked)


# A3's arena: 512 blocks. The two-bounce launch writes ~670 blocks (the oracle's hit counts: 451 + 204 + 13 on the three steps) and its 96 waves take their
# first run of 8 early in the primary step, so 64 waves get a run inside the arena and 32 do not: tiles are dropped. The 44 tiles that need at most 5
# blocks on all steps together reach compositing first; 64 runs are more than those, so at least 20 go to tiles that need 7-17 blocks, of which at most
# 10 need no more than the 8 of their run - the others record the primary step from their run and ask for a second run on a bounce step, when the bump
# counter is long past 512. (The 64-block floor gives 8 runs to the first 8 tiles that composite, mostly the lightest: too few to count on a mixed tile.)
# Measured: 64 / 7 / 0 (task, step)s recorded and 32 / 42 / 5 dropped on the three steps, 13-14 mixed tiles.
A3_BWD = 512 * ENTRIES_PER_BLOCK


@BOTH_HELP_MODES
def test_a3_two_bounces_steps_recorded_independently(ren, syn, team_help):
    """Two bounces: a tile may be recorded on one step and dropped on another. The backward treats the steps of a tile independently, so with A_s the
    tiles recorded on step s the overflowing launch equals sum_s [G(A_s, s bounces) - G(A_s, s - 1 bounces)], G(., -1) = 0, G(A, n) = the launch that fits
    with n bounces on the tiles A. The specular target is -10 (the only loss term the bounce steps feed: its residual's sign is +1 whatever the number of
    bounces, as in test_second_bounce_step_alone), the other terms keep their weights. Bar per tensor: 1e-5 (float-atomic order) of the sum of the six
    launches' max-abs."""
    cam = syn.default_camera()
    tg = generic_targets(syn, W, H)
    tg["specular"] = np.full_like(tg["specular"], -10.0)
    camera = cam_obj(ren, cam, tg)
    small, big = _mk(ren, syn, A3_BWD, team_help), _big(ren, syn, team_help)
    _configure((small, big))
    ls, lb = _grad_launch(ren, small, camera), _grad_launch(ren, big, camera)
    assert lb["c"][11] == 0 and ls["c"][11] & 2, (ls["c"][11], ls["c"][15], ls["c"][16])
    has, rec = _recorded_sets(ls, lb)
    ok, lost = has & rec, has & ~rec
    mixed = (ok[0] & (lost[1] | lost[2])) | (lost[0] & (ok[1] | ok[2]))
    assert mixed.any(), "no tile recorded on the primary step and dropped on a bounce step (or the reverse)"
    terms, scale = [], {k: float(np.abs(ls["grads"][k]).max()) for k in GRAD_KEYS}
    for s, nb, sign in ((0, 0, 1.0), (1, 1, 1.0), (1, 0, -1.0), (2, 2, 1.0), (2, 1, -1.0)):
        _configure((big,), num_bounces=nb)
        run = _grad_launch(ren, big, camera, mask=_pixels(rec[s]))
        assert run["c"][11] == 0
        terms.append((sign, run["grads"]))
        for k in GRAD_KEYS:
            scale[k] += float(np.abs(run["grads"][k]).max())
    _configure((big,))
    ratio = {}
    for k in GRAD_KEYS:
        expected = sum(sign * np.asarray(gr[k], np.float64) for sign, gr in terms)
        ratio[k] = float(np.abs(ls["grads"][k] - expected).max()) / (1e-5 * scale[k])
    unmasked = _rel(ls["grads"], lb["grads"])
    report(f"overflow_a3[help={int(team_help)}]", mixed_tiles=int(mixed.sum()), recorded=ok.sum(axis=(1, 2)).tolist(), dropped=lost.sum(axis=(1, 2)).tolist(),
           worst_over_bar=f"{max(ratio.values()):.1e}", over_bar=_fmt(ratio), vs_unmasked_launch=f"{max(unmasked.values()):.1e}")
    assert max(ratio.values()) < 1.0, _fmt(ratio)


def test_a4_the_launches_after_an_overflow_are_clean(ren, syn):
    cam = syn.default_camera()
    camera = cam_obj(ren, cam, generic_targets(syn, W, H))
    small, big = _mk(ren, syn, FLOOR_BWD), _big(ren, syn)
    _configure((small, big))
    lb = _grad_launch(ren, big, camera)
    st_b, img_b = _image_launch(big, camera)
    assert lb["c"][11] == 0 and st_b == 0
    first = _grad_launch(ren, small, camera)
    assert first["c"][11] & 2
    # a no-grad render: nothing left of the overflow, every output buffer is the fitting tracer's
    st_s, img_s = _image_launch(small, camera)
    assert st_s == 0
    for k in OUT_KEYS:
        assert _bit_equal(img_s[k], img_b[k]), k
    # a second overflowing grad launch (the bump counters and the chain heads start again): all of A1 once more
    second = _grad_launch(ren, small, camera)
    assert second["c"][11] & 2 and second["c"][16] == 64
    has, rec = _recorded_sets(second, lb)
    assert (has & rec).any() and (has & ~rec).any()
    _check_chains(second, lb, has, rec)
    _check_forward_untouched(second, lb)
    # another cloud size and back (resize + rebuild), then a no-grad render
    m = small.cuda_module
    m.resize(SCENE["N"] // 2)
    m.rebuild_bvh()
    small.rebuild_bvh()  # back to the model's size: resize, export, rebuild
    assert m.get_gaussians().mean.shape[0] == SCENE["N"]
    st_s, img_s = _image_launch(small, camera)
    assert st_s == 0
    for k in OUT_KEYS:
        assert _bit_equal(img_s[k], img_b[k]), k


def _train(ren, rt, cams, base):
    m = rt.cuda_module
    rt.zero_grad()
    m.get_gaussians().total_weight.zero_()
    m.get_metadata().total_num_calls.fill_(base)
    ren.train_views(cams, rt)
    status = int(m.get_counters()[11])
    torch.cuda.synchronize()
    return hip_grads(rt), status


def test_a5_batch_overflow_is_flagged_and_never_adds(ren, orc, syn):
    """train_views of three views in chunks of 2 + 1 on a floor arena. The debug exports describe the last egr_raytrace, not the batch (no
    export of k_forward_batch_grads' tables exists), so the recorded set of a batch cannot be read back and A2's exact form is out of reach. What can be
    held: with the diffuse term alone and a target far below every output, every residual is +1 and every hit's contribution to dL_drgb and total_weight
    is non-negative, so a subset of the hits can only give less. The oracle says per component whether all contributions share one sign (|sum| = sum of
    |contribution|): all of dL_drgb and total_weight do, 70-90 % of opacity / scale / mean / rotation do; the components that mix signs are left out (a
    partial sum of those may exceed the whole)."""
    V, base = 3, 20
    poses = views(syn, V)
    target = {"diffuse": np.full((H, W, 3), -10.0, np.float32)}
    cams = [cam_obj(ren, c, target) for c in poses]
    weights = {k: (v if k == "loss_weight_diffuse" else 0.0) for k, v in LOSS_WEIGHTS.items()}
    o = orc.Oracle(W, H)
    o.set_gaussians(syn.make_scene(SCENE["N"], SCENE["variant"], seed=SCENE["seed"]))
    o.set_config(num_bounces=2, jitter_primary_rays=1, **weights)
    o.update_bvh()
    total = {k: 0.0 for k in GRAD_KEYS}
    total_abs = {k: 0.0 for k in GRAD_KEYS}
    for v, c in enumerate(poses):
        o.set_camera(c["origin"], c["c2w"], c["fov"], c["znear"], c["zfar"])
        o.total_num_calls = base + v
        r = o.raytrace(True, targets=target, abs_sums=True)
        for k in GRAD_KEYS:
            total[k] = total[k] + r[k]
            total_abs[k] = total_abs[k] + r["grad_abs"][k]
    one_sign = {k: np.abs(total[k]) >= total_abs[k] * (1.0 - 1e-9) for k in GRAD_KEYS}
    assert one_sign["dL_drgb"].all() and one_sign["total_weight"].all() and total_abs["dL_drgb"].max() > 0
    assert np.all(total["dL_drgb"] >= 0) and np.all(total["total_weight"] >= 0)

    def mk(bwd):
        rt = _mk(ren, syn, bwd)
        rt.cuda_module.set_batch_frames(2)
        _configure((rt,), **weights)
        return rt

    big, small = mk(8_000_000), mk(FLOOR_BWD)
    g_big, st_big = _train(ren, big, cams, base)
    assert st_big == 0
    assert max(_rel(g_big, total).values()) < 1e-3  # (the batch that fits is the oracle's sum over the views)
    g_small, st_small = _train(ren, small, cams, base)
    assert st_small & 2, st_small
    checked = {}
    for k in GRAD_KEYS:
        assert np.isfinite(g_small[k]).all(), k
        tol = 1e-5 * float(np.abs(g_big[k]).max())
        sel = one_sign[k]
        assert np.all(np.abs(g_small[k])[sel] <= np.abs(g_big[k])[sel] + tol), k
        checked[k] = f"{sel.mean():.2f}"
    assert np.all(g_small["total_weight"] >= 0) and np.all(g_small["dL_drgb"] >= -1e-5 * float(np.abs(g_big["dL_drgb"]).max()))
    lost = 1.0 - float(g_small["total_weight"].sum()) / float(g_big["total_weight"].sum())
    assert lost > 1e-3  # the batch really dropped tiles
    report("overflow_a5", share_of_components_with_one_sign=checked, share_of_total_weight_dropped=f"{lost:.3f}")
    after, st_after = _train(ren, mk(8_000_000), cams, base)  # a tracer created after the overflow
    assert st_after == 0 and max(_rel(after, g_big).values()) < 1e-5


# ------------------------------------------------------------------------------------------------ B: runs of 8 blocks
def _blocks_written(hits):
    """forward_task.inc, the compositing loop: a batch of 8 hits per lane per iteration; the loop goes on while ANY lane of the tile still has a successor
    (`__ballot(running)`), and every iteration that does takes exactly one block in front of its batch; a lane that is running composites at least the
    first hit of the batch. So a (task, step) writes ceil(max over its pixels of the composited hits / 8) blocks - exactly, not a bound (the 1584-hit cap
    is a multiple of 8)."""
    return int(np.ceil(_tiles(hits).max(-1) / 8.0).sum())


def test_b1_blocks_taken_stay_within_seven_per_wave_of_the_blocks_written(ren, syn):
    cam = syn.default_camera()
    camera = cam_obj(ren, cam, generic_targets(syn, W, H))
    big = _big(ren, syn)
    _configure((big,))
    lb = _grad_launch(ren, big, camera)
    assert lb["c"][11] == 0
    written, used = _blocks_written(lb["hits"]), lb["c"][15]
    bound = written + 7 * WAVES
    report("overflow_b1", used=used, written=written, bound=bound, waves=WAVES)
    assert written >= 300
    assert written <= used <= bound and used % 8 == 0, (written, used, bound)  # (every written block was taken; runs of 8)


def test_b2_a_capacity_of_written_plus_waste_plus_eight_fits(ren, syn):
    cam = syn.default_camera()
    camera = cam_obj(ren, cam, generic_targets(syn, W, H))
    big = _big(ren, syn)
    _configure((big,))
    lb = _grad_launch(ren, big, camera)
    cap = _blocks_written(lb["hits"]) + 7 * WAVES + 8
    tight = _mk(ren, syn, ENTRIES_PER_BLOCK * cap)
    _configure((tight,))
    lt = _grad_launch(ren, tight, camera)
    assert lt["c"][16] == cap, (lt["c"][16], cap)
    assert lt["c"][11] == 0, (lt["c"][11], lt["c"][15], cap)
    e = _rel(lt["grads"], lb["grads"])
    report("overflow_b2", cap=cap, used=lt["c"][15], worst=f"{max(e.values()):.1e}")
    assert max(e.values()) < 1e-5, _fmt(e)
    assert np.array_equal(lt["hits"], lb["hits"])


# ------------------------------------------------------------------------------------------------ C: the candidate scratch
# 3000 blobs in front of the +x camera, moved 0.9 to one side so that part of the image is sparse: on the CPU oracle's counts (cube overlaps, never fewer than
# the candidates this build counts) 41 % of the pixels meet at most 64 candidates and 3637 meet more (up to 349) - thousands of rays ask for one of the 64
# extension blocks. transmittance_threshold = 0: no ray stops early, so a ray composites exactly the list it kept and dropping candidates can only remove hits
# (with a threshold, a ray that lost candidates in front keeps more light and may go on to hits the full list never reaches).
C_CFG = dict(jitter_primary_rays=0, num_bounces=0, transmittance_threshold=0.0)
C_FWD_SMALL = 1000  # -> 64-entry runs (the floor) and the 64-block extension floor


def _blob_scene(syn):
    g = syn.random_blob_scene(3000, seed=7)
    g["mean"][:, 1] += np.float32(0.9)
    return g


def _c_tracer(ren, g, fwd):
    rt = ren.GaussianRaytracer(ren.GaussianParams(g), W, H, ppll_forward_size=fwd, ppll_backward_size=BIG_BWD, team_help=False)
    rt.cuda_module.set_rays_per_task(64)
    set_config_everywhere(rt, (), **C_CFG)
    return rt


def _stat(t):
    return t.cpu().numpy().reshape(H, W)


@pytest.fixture(scope="module")
def cand(ren, syn):
    """The pair of C1-C3 after one no-grad launch each: (small, large, camera, results)."""
    g = _blob_scene(syn)
    cam = syn.plus_x_camera()
    camera = cam_obj(ren, cam, generic_targets(syn, W, H))
    res = {}
    rts = {}
    for name, fwd in (("small", C_FWD_SMALL), ("large", 50_000_000)):
        rt = _c_tracer(ren, g, fwd)
        status, img = _image_launch(rt, camera)
        st = rt.cuda_module.get_stats()
        res[name] = dict(status=status, img=img, c=[int(x) for x in rt.cuda_module.get_counters()], acc=_stat(st.num_accumulated_per_pixel).copy(),
                         trav=_stat(st.num_traversed_per_pixel).copy())
        rts[name] = rt
    assert res["large"]["status"] == 0 and res["small"]["status"] == 1, (res["large"]["status"], res["small"]["status"])
    assert res["small"]["c"][18] == 64 and res["small"]["c"][17] >= res["small"]["c"][18]  # the pool is exhausted
    # A ray's list holds its ACCEPTED candidates. The default statistic num_traversed_per_pixel counts the candidates inside their ellipsoid, accepted or
    # not (forward_task.inc: `traversed++` in front of the acceptance test), so it bounds the list length from above; the exact-statistics build counts
    # cube overlaps, a looser bound. The count of the LARGE tracer, whose lists are whole: <= 64 = the list fits the ray's own run.
    short = res["large"]["trav"] <= 64
    report("overflow_c", short_pixels=int(short.sum()), long_pixels=int((~short).sum()), longest=int(res["large"]["trav"].max()),
           ext_blocks_taken=res["small"]["c"][17], ext_blocks_cap=res["small"]["c"][18])
    assert short.mean() >= 0.25 and (~short).any(), short.mean()
    return rts["small"], rts["large"], camera, res, short


def test_c1_pixels_whose_list_fits_its_run_are_bit_equal(cand):
    _, _, _, res, short = cand
    for k in OUT_KEYS:
        a, b = res["small"]["img"][k], res["large"]["img"][k]
        assert _bit_equal(a[:, short], b[:, short]), k
    assert np.array_equal(res["small"]["acc"][short], res["large"]["acc"][short])
    assert (res["small"]["acc"][~short] != res["large"]["acc"][~short]).any()  # the overflow did drop candidates the rays would have composited


def test_c2_overflowed_pixels_stay_sane(cand):
    _, _, _, res, short = cand
    long_ = ~short
    for k in OUT_KEYS:
        assert np.isfinite(res["small"]["img"][k][:, long_]).all(), k
    for k in ("output_transmittance", "output_total_transmittance"):
        t = res["small"]["img"][k][:, long_]
        assert t.min() >= 0.0 and t.max() <= 1.0, (k, float(t.min()), float(t.max()))
    assert np.all(res["small"]["acc"][long_] <= res["large"]["acc"][long_])


def test_c3_gradients_under_candidate_overflow_and_a_small_cloud_after_it(ren, syn, cand):
    small, _, camera, _, _ = cand
    m = small.cuda_module
    m.get_metadata().total_num_calls.fill_(K - 1)
    run_grad(ren, small, camera)
    assert int(m.get_counters()[11]) == 1  # candidates dropped; the arena fits
    assert bool(torch.isfinite(m.get_gaussians().grad_flat).all())
    g2 = syn.random_blob_scene(300, seed=3, scale_range=(0.03, 0.08))  # at most 12 candidates per ray on the oracle: no list leaves its run
    small.pc = ren.GaussianParams(g2)
    small.rebuild_bvh()
    fresh = _c_tracer(ren, g2, C_FWD_SMALL)
    st_s, img_s = _image_launch(small, camera)
    st_f, img_f = _image_launch(fresh, camera)
    assert st_s == 0 and st_f == 0
    assert np.abs(img_f["output_rgb"]).max() > 0
    for k in OUT_KEYS:
        assert _bit_equal(img_s[k], img_f[k]), k
