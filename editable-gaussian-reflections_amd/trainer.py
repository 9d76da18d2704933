"""Host step of one training iteration as ONE HIP launch.

Mirrors what the reference does around `render()` in train.py:217-254 with ~60 small torch kernels:
gradient import (renderer/gaussian_raytracer.py:53-62), scale decay (train.py:224-226), `gaussians.optimizer.step()` =
torch.optim.Adam(eps=1e-15, betas=(beta_1, beta_2)) over the eight parameter groups of scene/gaussian_model.py:296-338,
`zero_grad` of the model and of the raytracer (train.py:248-249), the three clamps (train.py:251-254) and the parameter
export the next `GaussianRaytracer.__call__` would do (gaussian_raytracer.py:41-50). `expon_lr` restates
utils/general_utils.py:31-60 (pinned by tests/golden/expon_lr.npz, generated from the reference's own function).
"""
import importlib
import math

import torch

importlib.import_module(__package__).load_library()

# (optimizer group name, model attribute, raytracer tensor) in the order of gaussian_model.py:296-326
GROUPS = (("xyz", "_xyz", "mean"), ("normal", "_normal", "normal"), ("roughness", "_roughness", "roughness"), ("f0", "_f0", "f0"),
          ("f_dc", "_diffuse", "rgb"), ("opacity", "_opacity", "opacity"), ("scaling", "_scaling", "scale"), ("rotation", "_rotation", "rotation"))
CLAMPS = {"f_dc": (0.0, math.inf), "roughness": (0.0, 1.0), "f0": (0.0, 1.0)}  # train.py:251-254


def expon_lr(step, lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1000000):
    """The xyz learning-rate schedule (behaviour of utils/general_utils.py:31-60, pinned by tests/golden/expon_lr.npz):
    geometric interpolation lr_init -> lr_final over max_steps, times a warm-up factor that eases from lr_delay_mult to 1
    along a quarter sine over the first lr_delay_steps. A negative step or two zero rates switch the group off."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    frac = min(max(step / max_steps, 0.0), 1.0)
    rate = lr_init * (lr_final / lr_init) ** frac  # = exp((1 - frac) ln lr_init + frac ln lr_final)
    if lr_delay_steps > 0:
        ease = math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0.0), 1.0))
        rate *= lr_delay_mult + (1.0 - lr_delay_mult) * ease
    return float(rate)


def _camera_spheres(cam_centers, cam_znear, device):
    """(centers [C,3], znear [C]) as contiguous fp32 tensors on `device` for torch.ops.egr.prune_select, or (None, None) without cameras. `cam_znear`
    may be one number for all cameras."""
    if cam_centers is None:
        return None, None
    centers = torch.as_tensor(cam_centers, dtype=torch.float32, device=device).reshape(-1, 3).contiguous()
    znear = torch.as_tensor(cam_znear, dtype=torch.float32, device=device).reshape(-1)
    if znear.numel() == 1 and centers.shape[0] != 1:
        znear = znear.expand(centers.shape[0])
    return centers, znear.contiguous()


@torch.no_grad()
def filter_points_near_cameras(points, cam_centers, cam_znear):
    """The far-field candidate filter of add_farfield_points (`points[~scene.select_points_to_prune_near_cameras(points)]`): the rows of `points`
    [N,3] (fp32, GPU) outside every camera's znear sphere, in their old order - one select, one read-back, one gather."""
    points = points.contiguous()
    centers, znear = _camera_spheres(cam_centers, cam_znear, points.device)
    src_index, count = torch.ops.egr.prune_select(None, 1.0, 0.0, points, centers, znear, None)
    return torch.ops.egr.prune_gather([points], src_index, int(count.item()))[0]


class FusedTrainStep:
    """`step()` = import + scale decay + Adam + clamps + both zero_grads + export, one kernel over all eight groups.

    pc: model with the reference's raw parameter attributes (each with a `.grad`); raytracer: renderer.GaussianRaytracer;
    lrs: {group name: learning rate}; xyz_schedule: kwargs of `expon_lr` (the reference only schedules xyz,
    gaussian_model.py:349-355)."""

    def __init__(self, pc, raytracer, lrs, beta1=0.9, beta2=0.999, eps=1e-15, scale_decay=1.0, xyz_schedule=None):
        self.pc, self.rt = pc, raytracer
        self.lrs = {name: float(lrs.get(name, 0.0)) for name, _, _ in GROUPS}
        self.beta1, self.beta2, self.eps, self.scale_decay = beta1, beta2, eps, scale_decay
        self.xyz_schedule = xyz_schedule
        self.steps = 0
        self.exp_avg = {name: torch.zeros_like(getattr(pc, attr)) for name, attr, _ in GROUPS}
        self.exp_avg_sq = {name: torch.zeros_like(getattr(pc, attr)) for name, attr, _ in GROUPS}
        # the fused kernel adds the raytracer-side gradients itself: GaussianRaytracer.__call__ must not import them as well
        # (it would count them twice: g = model_grad + 2 * rt_grad)
        raytracer.import_grads = False

    # ---- optimizer surgery, mirroring scene/gaussian_model.py (the moments follow the parameters through topology changes)
    @torch.no_grad()
    def prune(self, keep_mask):
        """gaussian_model.py `_prune_optimizer`: keep the rows of both moments where `keep_mask` is True. The caller prunes the
        parameters themselves (`pc.prune_points(~keep_mask)`) and calls raytracer.rebuild_bvh().
        train.py:238-249 prunes BETWEEN render() and optimizer.step(): upstream the raytracer gradients of that iteration were
        already added to the old parameters' `.grad`, which prune_points replaces by zeros, so the step that follows sees a zero
        gradient. Here the import happens inside the fused step, so the iteration's raytracer gradients are dropped now
        (resize() would otherwise keep their first rows, misaligned with the pruned model).
        `prune_and_rebuild` is this whole sequence - criteria, parameters, moments, zeroing, rebuild - as one call that cannot go out of step."""
        for name in self.exp_avg:
            self.exp_avg[name] = self.exp_avg[name][keep_mask].contiguous()
            self.exp_avg_sq[name] = self.exp_avg_sq[name][keep_mask].contiguous()
        self.rt.zero_grad()

    @torch.no_grad()
    def prune_and_rebuild(self, min_weight=0.0, interval=1, cam_centers=None, cam_znear=None, remove_mask=None, extra=()):
        """The pruning step of train.py:238-249 as ONE call (csrc/prune.hip): select + compact + resize + rebuild with one host read-back.
        A row is removed if `total_weight / interval < min_weight` (the native total_weight; IEEE fp32 division, strict `<`: NaN and +inf stay), or
        if it lies inside a camera's znear sphere (`|xyz - cam_centers[c]| < cam_znear[c]` for any c: scene.select_points_to_prune_near_cameras;
        cam_centers [C,3], cam_znear [C] or one number), or if `remove_mask` (bool / uint8 [N]) marks it. With `train_views` pass interval * V.
        `extra`: further per-row tensors of the caller's model (4-byte elements, e.g. upstream's `_round_counter`); they come back compacted.
        Leaves bit for bit what `pc.prune_points(mask); self.prune(~mask); total_weight.zero_(); rt.rebuild_bvh()` leaves for the same mask: kept rows
        in their old order in the 8 parameters (fresh zero `.grad`) and the 16 moments, the iteration's raytracer gradients dropped, total_weight
        restarted, the tree rebuilt. The result depends on the inputs alone, so the ranks of a partition - which all hold the same all-reduced
        total_weight - keep identical clouds. Returns (n_kept, [compacted extra tensors]); raises ValueError, before anything is touched, if no row
        would survive."""
        pc, g = self.pc, self.rt.cuda_module.get_gaussians()
        xyz = pc._xyz
        centers, znear = _camera_spheres(cam_centers, cam_znear, xyz.device)
        if remove_mask is not None:
            remove_mask = torch.as_tensor(remove_mask, device=xyz.device).contiguous()
        src_index, count = torch.ops.egr.prune_select(g.total_weight, float(interval), float(min_weight), xyz, centers, znear, remove_mask)
        n_kept = int(count.item())  # the one synchronisation
        if n_kept == 0:
            raise ValueError("prune_and_rebuild: no gaussian would survive (nothing was changed)")
        attrs = [attr for _, attr, _ in GROUPS]
        names = [name for name, _, _ in GROUPS]
        extra = list(extra)
        out = torch.ops.egr.prune_gather([getattr(pc, a) for a in attrs] + [self.exp_avg[n] for n in names] + [self.exp_avg_sq[n] for n in names] + extra,
                                         src_index, n_kept)
        for k, attr in enumerate(attrs):
            out[k].grad = torch.zeros_like(out[k])
            setattr(pc, attr, out[k])
        for k, name in enumerate(names):
            self.exp_avg[name], self.exp_avg_sq[name] = out[8 + k], out[16 + k]
        self.rt.rebuild_bvh()  # resize + export + full build
        self.rt.cuda_module.get_gaussians().grad_flat.zero_()  # resize kept the first rows of the old gradients and weights: the gradients in flight are dropped, total_weight restarts
        return n_kept, out[24:]

    @torch.no_grad()
    def extend(self, n_new):
        """gaussian_model.py `cat_tensors_to_optimizer` (add_farfield_points): new rows start with zero moments."""
        for name in self.exp_avg:
            z = self.exp_avg[name].new_zeros((n_new,) + tuple(self.exp_avg[name].shape[1:]))
            self.exp_avg[name] = torch.cat([self.exp_avg[name], z], 0)
            self.exp_avg_sq[name] = torch.cat([self.exp_avg_sq[name], z.clone()], 0)

    @torch.no_grad()
    def reset_state(self, name):
        """gaussian_model.py:464-476 `replace_tensor_to_optimizer`: the group's parameter was replaced, both moments restart at zero.
        The stored state object - and with it torch's `step` count, hence the bias correction - is re-attached unchanged, so the
        first update after a reset is lr * m_hat / sqrt(v_hat) with the OLD step count (about 3.16 lr sign(g) late in training,
        not lr sign(g))."""
        attr = {n: a for n, a, _ in GROUPS}[name]
        self.exp_avg[name] = torch.zeros_like(getattr(self.pc, attr))
        self.exp_avg_sq[name] = torch.zeros_like(getattr(self.pc, attr))

    def update_learning_rate(self, iteration):  # gaussian_model.py:349-355
        if self.xyz_schedule is not None:
            self.lrs["xyz"] = expon_lr(iteration, **self.xyz_schedule)
        return self.lrs["xyz"]

    @torch.no_grad()
    def step(self):
        g = self.rt.cuda_module.get_gaussians()
        self.steps += 1  # one count for all groups: none of the reference's optimizer surgery touches torch's per-tensor `step`
        params = [getattr(self.pc, attr) for _, attr, _ in GROUPS]
        grads = [getattr(self.pc, attr).grad for _, attr, _ in GROUPS]
        rt_params = [getattr(g, rt) for _, _, rt in GROUPS]
        rt_grads = [getattr(g, rt).grad for _, _, rt in GROUPS]
        torch.ops.egr.fused_adam_step(
            params, grads, rt_params, rt_grads, [self.exp_avg[n] for n, _, _ in GROUPS], [self.exp_avg_sq[n] for n, _, _ in GROUPS],
            [self.lrs[n] for n, _, _ in GROUPS], [CLAMPS.get(n, (-math.inf, math.inf))[0] for n, _, _ in GROUPS],
            [CLAMPS.get(n, (-math.inf, math.inf))[1] for n, _, _ in GROUPS], [self.scale_decay if n == "scaling" else 1.0 for n, _, _ in GROUPS],
            self.steps, self.beta1, self.beta2, self.eps)
