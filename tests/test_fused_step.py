"""the fused host step (csrc/step.hip, trainer.py) against the reference's own sequence of torch calls."""
import ast
import importlib
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _expon_lr():
    # trainer.py loads the native library on import (GPU product); the schedule itself is pure numpy: load it without that
    src = open(os.path.join(ROOT, PKG, "trainer.py")).read()
    tree = ast.parse(src)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "expon_lr")
    ns = {"np": np, "math": math}
    exec(compile(ast.Module([fn], []), "trainer.expon_lr", "exec"), ns)
    return ns["expon_lr"]


def test_lr_schedule_matches_reference_vectors():
    """tests/golden/expon_lr.npz was produced by the reference's get_expon_lr_func (make_expon_lr_vectors.py)."""
    f = _expon_lr()
    z = np.load(os.path.join(GOLD, "expon_lr.npz"))
    for k, c in enumerate(z["cases"]):
        kw = eval(str(c))
        got = np.array([f(int(s), **kw) for s in z["steps"]])
        np.testing.assert_allclose(got, z[f"lr{k}"], rtol=1e-12, atol=0)


LRS = dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)


def reference_sequence(pc, rtg, opt, scale_decay):
    """train.py:224-254 + gaussian_raytracer.py:41-62 with stock torch calls."""
    with torch.no_grad():
        pc._xyz.grad.add_(rtg.mean.grad), pc._opacity.grad.add_(rtg.opacity.grad), pc._scaling.grad.add_(rtg.scale.grad)
        pc._rotation.grad.add_(rtg.rotation.grad), pc._diffuse.grad.add_(rtg.rgb.grad), pc._normal.grad.add_(rtg.normal.grad)
        pc._roughness.grad.add_(rtg.roughness.grad), pc._f0.grad.add_(rtg.f0.grad)
        if scale_decay < 1.0:
            pc._scaling.copy_(torch.log(torch.exp(pc._scaling) * scale_decay))
        opt.step()
        opt.zero_grad(set_to_none=False)
        for t in (rtg.rgb, rtg.opacity, rtg.scale, rtg.rotation, rtg.mean, rtg.normal, rtg.roughness, rtg.f0):
            t.grad.zero_()
        pc._diffuse.data.clamp_(min=0.0), pc._roughness.data.clamp_(min=0.0, max=1.0), pc._f0.data.clamp_(min=0.0, max=1.0)
        rtg.scale.copy_(pc._scaling), rtg.rotation.copy_(pc._rotation), rtg.mean.copy_(pc._xyz), rtg.opacity.copy_(pc._opacity)
        rtg.rgb.copy_(pc._diffuse), rtg.normal.copy_(pc._normal), rtg.roughness.copy_(pc._roughness), rtg.f0.copy_(pc._f0)


@pytest.mark.gpu
@pytest.mark.parametrize("scale_decay", [1.0, 0.999])
def test_fused_step_matches_torch_adam(scale_decay):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    ren = importlib.import_module(PKG + ".renderer")
    syn = importlib.import_module(PKG + ".synthetic")
    tr = importlib.import_module(PKG + ".trainer")
    N = 20000
    g = syn.make_scene(N, "trained", seed=4)
    pcs, rts = [], []
    for _ in range(2):
        pc = ren.GaussianParams(g)
        pcs.append(pc), rts.append(ren.GaussianRaytracer(pc, 32, 32))
    (pa, pb), (ra, rb) = pcs, rts
    groups = [{"params": [getattr(pb, attr)], "lr": LRS[name], "name": name} for name, attr, _ in tr.GROUPS]
    opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15, betas=(0.9, 0.999))
    fused = tr.FusedTrainStep(pa, ra, LRS, scale_decay=scale_decay)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for it in range(6):
        for _, attr, rtname in tr.GROUPS:  # same synthetic gradients on both sides: raytracer gradients + a model-side part
            shape = getattr(pa, attr).shape
            d_rt = torch.randn(shape, device="cuda", generator=gen) * 10.0 ** float(torch.randint(-6, 1, (1,)).item())
            d_model = torch.randn(shape, device="cuda", generator=gen) * 1e-3 * (it % 2)
            for pc, rt in ((pa, ra), (pb, rb)):
                getattr(rt.cuda_module.get_gaussians(), rtname).grad.copy_(d_rt)
                getattr(pc, attr).grad.copy_(d_model)
        fused.step()
        reference_sequence(pb, rb.cuda_module.get_gaussians(), opt, scale_decay)
        ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()
        for name, attr, rtname in tr.GROUPS:
            a, b = getattr(pa, attr), getattr(pb, attr)
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (it, name, float((a - b).abs().max()))
            assert torch.equal(getattr(ga, rtname), a), (it, name)  # export
            assert float(getattr(ga, rtname).grad.abs().max()) == 0.0 and float(a.grad.abs().max()) == 0.0  # both zero_grads
            st = opt.state[b]
            for mine, ref in ((fused.exp_avg[name], st["exp_avg"]), (fused.exp_avg_sq[name], st["exp_avg_sq"])):
                # fp32 round-off only (the lerp cancels: compare against the tensor's scale, not element by element)
                assert float((mine - ref).abs().max()) <= 1e-6 * float(ref.abs().max()) + 1e-30, (it, name)
    assert float(pa._diffuse.min()) >= 0.0 and float(pa._roughness.max()) <= 1.0 and float(pa._f0.min()) >= 0.0


@pytest.mark.gpu
def test_reset_state_keeps_the_step_count_like_replace_tensor_to_optimizer():
    """scene/gaussian_model.py:464-476 zeroes exp_avg / exp_avg_sq of one group and re-attaches the SAME state dict, so torch's
    per-tensor `step` - the bias correction - carries on. The fused step must do the same: after 5 steps and a reset of "opacity"
    the next update equals torch.optim.Adam's on a state whose moments were zeroed in place."""
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    ren = importlib.import_module(PKG + ".renderer")
    syn = importlib.import_module(PKG + ".synthetic")
    tr = importlib.import_module(PKG + ".trainer")
    N = 4000
    g = syn.make_scene(N, "trained", seed=6)
    pa, pb = ren.GaussianParams(g), ren.GaussianParams(g)
    ra, rb = ren.GaussianRaytracer(pa, 32, 32), ren.GaussianRaytracer(pb, 32, 32)
    opt = torch.optim.Adam([{"params": [getattr(pb, attr)], "lr": LRS[name], "name": name} for name, attr, _ in tr.GROUPS], lr=0.0, eps=1e-15)
    fused = tr.FusedTrainStep(pa, ra, LRS)
    gen = torch.Generator(device="cuda").manual_seed(7)
    for it in range(8):
        if it == 5:  # opacity reset (train.py resets opacities every opacity_reset_interval): new values, zero moments, same step count
            new_opa = torch.full_like(pa._opacity, -2.0)
            pa._opacity.copy_(new_opa), pb._opacity.data.copy_(new_opa)
            fused.reset_state("opacity")
            st = opt.state[pb._opacity]
            st["exp_avg"].zero_(), st["exp_avg_sq"].zero_()  # what replace_tensor_to_optimizer leaves behind (`step` untouched)
            assert int(st["step"]) == 5
        for _, attr, rtname in tr.GROUPS:
            d = torch.randn(getattr(pa, attr).shape, device="cuda", generator=gen) * 1e-2
            for pc, rt in ((pa, ra), (pb, rb)):
                getattr(rt.cuda_module.get_gaussians(), rtname).grad.copy_(d)
        before = pa._opacity.clone()
        fused.step()
        reference_sequence(pb, rb.cuda_module.get_gaussians(), opt, 1.0)
        for name, attr, _ in tr.GROUPS:
            a, b = getattr(pa, attr), getattr(pb, attr)
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (it, name, float((a - b).abs().max()))
        if it == 5:  # the first update after the reset is (1-b1)/sqrt(1-b2) * sqrt(1-b2^6)/(1-b1^6) ~ 0.52 lr, not lr (a restarted count)
            ratio = float(((pa._opacity - before).abs() / LRS["opacity"]).median())
            want = (1 - 0.9) / (1 - 0.9 ** 6) / math.sqrt((1 - 0.999) / (1 - 0.999 ** 6))
            assert abs(ratio - want) < 1e-3 * want, (ratio, want)


@pytest.mark.gpu
def test_fused_step_full_size_timing():
    ren = importlib.import_module(PKG + ".renderer")
    syn = importlib.import_module(PKG + ".synthetic")
    tr = importlib.import_module(PKG + ".trainer")
    import time
    N = 1_000_000
    g = syn.make_scene(N, "trained", seed=0)
    pc = ren.GaussianParams(g)
    rt = ren.GaussianRaytracer(pc, 64, 64)
    fused = tr.FusedTrainStep(pc, rt, LRS, scale_decay=0.9999)
    opt = torch.optim.Adam([{"params": [getattr(pc, attr)], "lr": LRS[name]} for name, attr, _ in tr.GROUPS], lr=0.0, eps=1e-15)
    rtg = rt.cuda_module.get_gaussians()

    def timed(f, reps=20):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    t_fused = timed(fused.step)
    t_torch = timed(lambda: reference_sequence(pc, rtg, opt, 0.9999))
    print(f"host step at N=1M: fused {t_fused:.3f} ms vs stock torch sequence {t_torch:.3f} ms")
    assert t_fused < t_torch
    with pytest.raises(RuntimeError):
        torch.ops.egr.fused_adam_step([pc._xyz], [pc._xyz.grad], [], [], [], [], [1.0], [-math.inf], [math.inf], [1.0], 1, 0.9, 0.999, 1e-15)
    with pytest.raises(RuntimeError):  # a per-group step list of the wrong length is rejected, not silently ignored
        torch.ops.egr.fused_adam_step([pc._xyz], [pc._xyz.grad], [pc._xyz], [pc._xyz.grad], [pc._xyz], [pc._xyz], [1.0], [-math.inf], [math.inf], [1.0], 1, 0.9,
                                      0.999, 1e-15, [1, 2])


# ---- torch.ops.egr.fused_adam_step called directly on hand-made tensors, one step at a time against the fp64 restatement (tests/aux_restatement.py) ----
#
# Every step hands the kernel's OWN previous fp32 p, m, v and the fp32 gradient to the restatement: nothing free-runs (free-running fp32 against fp64 loses the
# update to cancellation in m within a dozen steps). Bars, from the kernel's operation count with eps32 = 2^-24 (division and square root 2.5 ulp each; w1, beta2,
# w2, step_size and bc2_sqrt are rounded to float):
#   m          |m_hip - m64| <= 4 eps32 max(|m_prev|, |g|)
#   v          |v_hip - v64| <= 8 eps32 v64
#   parameter  |p_hip - (p_prev - u64)| <= eps32 max(|p_prev|, |p_hip|) + 16 eps32 |u64|,  u64 = the fp64 update from the KERNEL's new m and v
#   decay      |p_hip - log(exp(p) float(d))| <= 8 eps32 max(1, |p|)  (a group with decay AND moments gets the sum of the last two: the decayed value is p_prev)
import aux_restatement as ar  # noqa: E402
from hip_common import report  # noqa: E402

EPS32 = 2.0 ** -24
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-15
INF = math.inf
WIDTHS = dict(xyz=3, normal=3, roughness=1, f0=3, f_dc=3, opacity=1, scaling=3, rotation=4)
NAMES = tuple(WIDTHS)  # trainer.GROUPS' order
CLAMPS = {"f_dc": (0.0, INF), "roughness": (0.0, 1.0), "f0": (0.0, 1.0)}


@pytest.fixture(scope="module")
def op():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    importlib.import_module(PKG).load_library()
    return torch.ops.egr.fused_adam_step


class Grp:
    """One parameter group on the GPU. grad / rt / moments False: that tensor is passed EMPTY, the binding's "absent". The export target starts as 777."""

    def __init__(self, p, lr, lo=-INF, hi=INF, decay=1.0, grad=True, rt_param=True, rt_grad=True, moments=True, m=None, v=None):
        p = np.ascontiguousarray(p, np.float32)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
        none = lambda: torch.empty(0, device="cuda")
        self.p0, self.p, self.lr, self.lo, self.hi, self.decay = p.copy(), up(p), lr, lo, hi, decay
        self.g = torch.zeros_like(self.p) if grad else none()
        self.rg = torch.zeros_like(self.p) if rt_grad else none()
        self.rp = torch.full_like(self.p, 777.0) if rt_param else none()
        self.m = (up(m) if m is not None else torch.zeros_like(self.p)) if moments else none()
        self.v = (up(v) if v is not None else torch.zeros_like(self.p)) if moments else none()

    def host(self):
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("p", "g", "rg", "rp", "m", "v")}


def launch(op, groups, step, group_steps=()):
    op([x.p for x in groups], [x.g for x in groups], [x.rp for x in groups], [x.rg for x in groups], [x.m for x in groups], [x.v for x in groups],
       [x.lr for x in groups], [x.lo for x in groups], [x.hi for x in groups], [x.decay for x in groups], step, B1, B2, ADAM_EPS, list(group_steps))
    torch.cuda.synchronize()


def units(err, unit):
    """max err / unit; where the unit is 0 the error has to be 0 (inf otherwise)."""
    err, unit = np.asarray(err, np.float64).ravel(), np.asarray(unit, np.float64).ravel()
    if np.any(err[unit == 0] != 0):
        return math.inf
    return float((err[unit > 0] / unit[unit > 0]).max()) if np.any(unit > 0) else 0.0


def check_one_step(x, before, t, worst):
    """Group x after one launch against the restatement of that one step from `before` (x.host() taken just before the launch)."""
    after = x.host()
    g32 = before["g"] + before["rg"] if before["g"].size and before["rg"].size else (before["g"] if before["g"].size else before["rg"])  # the kernel's one fp32 add
    assert g32.dtype == np.float32
    m64, v64 = ar.adam_moments64(before["m"], before["v"], g32, B1, B2)
    worst["m"] = max(worst["m"], units(np.abs(after["m"] - m64), EPS32 * np.maximum(np.abs(before["m"]), np.abs(g32))))
    worst["v"] = max(worst["v"], units(np.abs(after["v"] - v64), EPS32 * v64))
    p_prev = before["p"].astype(np.float64)
    slack = EPS32 * np.maximum(np.abs(p_prev), np.abs(after["p"]))
    if x.decay != 1.0:
        slack = slack + 8 * EPS32 * np.maximum(1.0, np.abs(p_prev))
        p_prev = ar.scale_decay64(p_prev, np.float32(x.decay))
    u64 = ar.adam_update64(after["m"], after["v"], x.lr, t, B1, B2, ADAM_EPS)
    want = np.clip(p_prev - u64, x.lo, x.hi)  # (a clamp moves two numbers no further apart)
    worst["update"] = max(worst["update"], units(np.maximum(np.abs(after["p"] - want) - slack, 0.0), EPS32 * np.abs(u64)))
    assert not after["rp"].size or np.array_equal(after["rp"], after["p"])  # export, bit for bit
    assert not after["g"].any() and not after["rg"].any()  # both zero_grads
    if x.lo > -INF or x.hi < INF:
        assert after["p"].min() >= x.lo and after["p"].max() <= x.hi


def trainer_like_groups(rng, n, names=NAMES, decay=0.999):
    out = []
    for name in names:
        w = WIDTHS[name]
        p = rng.random((n, w)) if name in CLAMPS else rng.normal(size=(n, w)) * (3.0 if name == "xyz" else 1.0)
        lo, hi = CLAMPS.get(name, (-INF, INF))
        out.append(Grp(p, LRS[name], lo, hi, decay if name == "scaling" else 1.0))
    return out


def feed(rng, groups, it):
    """g = randn * 10^k, k from -6..0 per group and step, on the raytracer side; a model-side part on odd steps; steps 0 and 3: every 7th element exactly 0."""
    for x in groups:
        shape = tuple(x.p.shape)
        rg = rng.normal(size=shape) * 10.0 ** int(rng.integers(-6, 1))
        g = rng.normal(size=shape) * 1e-3 * (it % 2)
        if it in (0, 3):
            rg.reshape(-1)[::7] = 0.0
            g.reshape(-1)[::7] = 0.0
        for t, a in ((x.rg, rg), (x.g, g)):
            if t.numel():
                t.copy_(torch.from_numpy(a.astype(np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
def test_direct_one_step_against_fp64_restatement(op, n):
    """Measured on an MI355X (REPORT lines): DESIGN.md section 8 has the table."""
    rng = np.random.default_rng(n)
    groups = trainer_like_groups(rng, n)
    worst = dict(m=0.0, v=0.0, update=0.0)
    for it in range(6):
        feed(rng, groups, it)
        before = [x.host() for x in groups]
        launch(op, groups, it + 1)
        for x, b in zip(groups, before):
            check_one_step(x, b, it + 1, worst)
    report(f"fused_step_one_step_n{n}", m_units=f"{worst['m']:.2f}", v_units=f"{worst['v']:.2f}", update_units=f"{worst['update']:.2f}", bars="4 / 8 / 16")
    assert worst["m"] <= 4.0 and worst["v"] <= 8.0 and worst["update"] <= 16.0, worst


def _zero_start(rng, n, w, t):
    """p = 0, so the new parameter IS minus the update; moments of a run in progress unless t = 1."""
    m = rng.normal(size=(n, w)) * 1e-3 if t > 1 else None
    v = rng.random((n, w)) * 1e-5 + 1e-9 if t > 1 else None
    return Grp(np.zeros((n, w)), 1.6e-4, m=m, v=v)


def _update_units(x, before, t):
    after = x.host()
    assert after["m"].all()  # every element moves
    u64 = ar.adam_update64(after["m"], after["v"], x.lr, t, B1, B2, ADAM_EPS)
    assert not before["p"].any()
    return units(np.abs(after["p"] + u64), EPS32 * np.abs(u64))


@pytest.mark.gpu
def test_update_from_zero_parameters_holds_the_bias_correction_to_16_ulp(op):
    """|p_new + u64| <= 16 eps32 |u64| at t = 1, 7, 1000 through `step`, then three groups with their own counts through `group_steps` (`step` is then unused).
    A 1 % error of either bias correction, 1 - beta^t evaluated in float (1.3e-5 at t = 1000) or a neighbouring t cannot pass."""
    rng = np.random.default_rng(3)
    got = {}
    for t in (1, 7, 1000):
        x = _zero_start(rng, 257, 3, t)
        feed(rng, [x], 1)
        before = x.host()
        launch(op, [x], t)
        got[f"t{t}"] = _update_units(x, before, t)
    counts = (1000, 1, 7)
    groups = [_zero_start(rng, 255, w, t) for w, t in zip((4, 1, 3), counts)]
    feed(rng, groups, 1)
    before = [x.host() for x in groups]
    launch(op, groups, 3, counts)
    for x, b, t in zip(groups, before, counts):
        got[f"group_steps_t{t}"] = _update_units(x, b, t)
    report("fused_step_update_from_zero", **{k: f"{v:.2f}" for k, v in got.items()}, bar=16)
    assert max(got.values()) <= 16.0, got


@pytest.mark.gpu
@pytest.mark.parametrize("G", [1, 3, 8])
def test_group_shapes_and_side_effects(op, G):
    """G groups of different widths in one launch, each with another set of tensors absent; tensors of groups that are not passed stay as they are."""
    rng = np.random.default_rng(10 + G)
    n = 257
    all8 = trainer_like_groups(rng, n)
    all8[1] = Grp(rng.normal(size=(n, 3)), 1e-3, rt_param=False, rt_grad=False)  # no raytracer side at all
    all8[2] = Grp(rng.random((n, 1)) * 1.4 - 0.2, 2e-3, 0.0, 1.0, moments=False)  # no moments: decay and clamp only
    all8[5] = Grp(rng.normal(size=(n, 1)), 2.5e-2, grad=False)  # only the raytracer's gradient
    pick = {1: [5], 3: [2, 1, 7], 8: list(range(8))}[G]
    groups, others = [all8[k] for k in pick], [all8[k] for k in range(8) if k not in pick]
    feed(rng, all8, 1)
    before, untouched = [x.host() for x in groups], [x.host() for x in others]
    launch(op, groups, 4)
    worst = dict(m=0.0, v=0.0, update=0.0)
    for x, b in zip(groups, before):
        a = x.host()
        if a["m"].size:
            check_one_step(x, b, 4, worst)
        else:  # decay (none here) and clamp only; gradients still imported and zeroed, value exported
            assert np.array_equal(a["p"], np.clip(b["p"], x.lo, x.hi)) and np.any(a["p"] != b["p"])
            assert np.array_equal(a["rp"], a["p"]) and not a["g"].any() and not a["rg"].any() and b["rg"].any()
            assert a["m"].size == 0 and a["v"].size == 0
    assert worst["m"] <= 4.0 and worst["v"] <= 8.0 and worst["update"] <= 16.0, worst
    for x, b in zip(others, untouched):
        a = x.host()
        assert all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [0.999, 0.9])
def test_scale_decay_alone(op, d):
    grid = np.concatenate([np.linspace(-80.0, 80.0, 999), [0.0]]).astype(np.float32)
    x = Grp(grid[:, None], 0.0, decay=d, moments=False)
    launch(op, [x], 1)
    got = x.host()["p"][:, 0]
    worst = units(np.abs(got - ar.scale_decay64(grid, np.float32(d))), EPS32 * np.maximum(1.0, np.abs(grid)))
    report(f"fused_step_scale_decay_{d}", units=f"{worst:.2f}", bar=8)
    assert worst <= 8.0
    # beyond the normal range of fp32 exp only the class is held: finite, -inf or +inf, as numpy's fp32 evaluation of the same expression
    far = np.array([-110.0, -100.0, -90.0, 88.0, 89.0], np.float32)
    with np.errstate(all="ignore"):
        want = np.log(np.exp(far) * np.float32(d))
    assert want.dtype == np.float32
    y = Grp(far[:, None], 0.0, decay=d, moments=False)
    launch(op, [y], 1)
    got = y.host()["p"][:, 0]
    cls = lambda a: np.where(np.isnan(a), 3, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 1, 0)))
    assert np.array_equal(cls(got), cls(want)), (got, want)
    assert list(cls(want)) == [1, 0, 0, 0, 2]  # exp(-110) is below the smallest denormal, exp(89) above the largest float


@pytest.mark.gpu
def test_no_decay_leaves_the_parameter_bit_unchanged(op):
    vals = np.concatenate([np.linspace(-80.0, 80.0, 255), [0.0, -110.0, 89.0, 1e-40, INF, -INF]]).astype(np.float32)
    x = Grp(vals[:, None], 0.0, decay=1.0, moments=False)
    launch(op, [x], 1)
    assert np.array_equal(x.host()["p"][:, 0].view(np.uint32), vals.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("moments", [False, True], ids=["clamp_only", "adam_lr0"])
def test_clamp_edges_are_bit_exact(op, moments):
    """lr = 0 (with moments: p - 0 * (0 / eps)): at, just inside and just outside [0, 1] and [0, inf)."""
    f = np.float32
    up, down = (lambda a: np.nextafter(f(a), f(INF))), (lambda a: np.nextafter(f(a), f(-INF)))
    v01 = np.array([down(0), 0.0, up(0), 0.5, down(1), 1.0, up(1), -1.0, 2.0, -3e38, 3e38, -INF, INF], np.float32)
    v0i = np.array([down(0), 0.0, up(0), -1e-38, 1e-38, -1.0, 3e38, INF, -INF], np.float32)
    a, b = Grp(v01[:, None], 0.0, 0.0, 1.0, moments=moments), Grp(np.resize(v0i, len(v01))[:, None], 0.0, 0.0, INF, moments=moments)
    launch(op, [a, b], 1)
    for x, vals, lo, hi in ((a, v01, 0.0, 1.0), (b, np.resize(v0i, len(v01)), 0.0, INF)):
        got = x.host()["p"][:, 0]
        assert np.array_equal(got.view(np.uint32), np.clip(vals, f(lo), f(hi)).view(np.uint32)), (got, vals)
    z = Grp(np.array([[-0.0]], np.float32), 0.0, 0.0, 1.0, moments=moments)  # either zero is a correct clamp of -0
    launch(op, [z], 1)
    assert float(z.host()["p"][0, 0]) == 0.0


def _classes(a):
    return np.where(np.isnan(a), 3, np.where(np.isposinf(a), 2, np.where(np.isneginf(a), 1, 0)))


def _same_class_and_value(mine, ref, what):
    """Equal as class everywhere; finite values within 8 eps32 relative (both sides are fp32 evaluations of the same few operations: they may contract or order them
    differently) or 2^-126 absolute (below the normal range either side may flush)."""
    assert np.array_equal(_classes(mine), _classes(ref)), (what, mine.ravel()[:8], ref.ravel()[:8])
    fin = np.isfinite(ref)
    np.testing.assert_allclose(mine[fin], ref[fin], rtol=8 * EPS32, atol=2.0 ** -126, err_msg=str(what))


@pytest.mark.gpu
def test_non_finite_values_follow_stock_torch(op):
    """Rows 0..5 of every group: a NaN parameter; a NaN, +inf, -inf gradient element; a zero gradient on zero moments; a gradient of 1e-40. Two steps against
    torch.optim.Adam + the three clamp_ calls on the same fp32 inputs. NaN stays NaN in all eight groups: fmaxf / fminf alone made it clamp_min, or -inf."""
    rng = np.random.default_rng(8)
    n = 12
    mine, ref = [], []
    for name in NAMES:
        p = (0.25 + 0.5 * rng.random((n, WIDTHS[name]))).astype(np.float32)  # away from 0 and from the clamps: the update is a small part of the value
        p[0, 0] = np.nan
        lo, hi = CLAMPS.get(name, (-INF, INF))
        mine.append(Grp(p, LRS[name], lo, hi))
        ref.append(torch.nn.Parameter(torch.from_numpy(p.copy()).cuda()))
    opt = torch.optim.Adam([{"params": [q], "lr": LRS[name]} for q, name in zip(ref, NAMES)], lr=0.0, eps=ADAM_EPS, betas=(B1, B2), foreach=False)
    special = [0.01, np.nan, INF, -INF, 0.0, 1e-40]
    first = [(rng.normal(size=tuple(x.p.shape)) * 1e-2).astype(np.float32) for x in mine]
    for it in range(2):
        for x, q, g1 in zip(mine, ref, first):
            g = g1 * np.float32(1.0 if it == 0 else 0.5)  # (half the first one: m grows from 0.1 g to 0.14 g, no cancellation that would need a wider bar)
            g[:6, 0] = special if it == 0 else [0.005, 0.01, 0.01, 0.01, 0.01, 0.5e-40]
            x.rg.copy_(torch.from_numpy(g))
            q.grad = torch.from_numpy(g.copy()).cuda()
        launch(op, mine, it + 1)
        with torch.no_grad():
            opt.step()
            ref[NAMES.index("f_dc")].clamp_(min=0.0), ref[NAMES.index("roughness")].clamp_(min=0.0, max=1.0), ref[NAMES.index("f0")].clamp_(min=0.0, max=1.0)
        for x, q, name in zip(mine, ref, NAMES):
            a = x.host()
            assert np.isnan(a["p"][0, 0]), (it, name, a["p"][0, 0])  # the NaN parameter
            assert np.isnan(a["p"][1:4, 0]).all(), (it, name, a["p"][1:4, 0])  # NaN gradient; inf / inf
            assert np.array_equal(a["rp"].view(np.uint32), a["p"].view(np.uint32)) and not a["rg"].any()
            st = opt.state[q]
            _same_class_and_value(a["p"], q.detach().cpu().numpy(), (it, name, "p"))
            _same_class_and_value(a["m"], st["exp_avg"].cpu().numpy(), (it, name, "m"))
            _same_class_and_value(a["v"], st["exp_avg_sq"].cpu().numpy(), (it, name, "v"))
            if it == 0:
                assert a["p"][4, 0] == x.p0[4, 0] and a["m"][4, 0] == 0.0 and a["v"][4, 0] == 0.0  # 0 / eps = 0: it stays
