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

import numpy as np
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


def farfield_candidates(n, seed, radius, clamp=3.0, first=0, device="cuda"):
    """Candidates first .. first + n of the far-field cloud (csrc/grow.hip: egr_grow_sample) as a new fp32 [n,3] tensor: `randn().clamp(-clamp, clamp) * radius`
    of gaussian_model.py:236 with a generator of our own - Philox4x32-10 keyed by `seed`, counter = the candidate's index, Box-Muller in fp64 (the header has
    the definition, tests/grow_restatement.py restates it). Row r depends on (seed, first + r, radius, clamp) alone: not on n, the device, torch's version or
    anything run before, so every rank of a partition draws the same points and a call can be split at any row. `seed` and `first` are unsigned 64-bit
    integers (taken modulo 2^64)."""
    as_i64 = lambda v: ((int(v) % (1 << 64)) ^ (1 << 63)) - (1 << 63)  # the op's schema carries the 64 bits in a signed int
    return torch.ops.egr.grow_sample(as_i64(first), int(n), as_i64(seed), float(radius), float(clamp), torch.device(device))


def _word_bits(value, dtype):
    """The 32-bit word of `value` as an element of a 4-byte `dtype` (egr_grow_append's fill_bits)."""
    if dtype == torch.float32:
        return int(np.array(value, np.float32).view(np.uint32))
    if dtype == torch.int32:
        return int(np.array(value, np.int64).astype(np.int32).view(np.uint32))
    raise ValueError(f"per-row extras must be float32 or int32 tensors, got {dtype}")


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
    def grow_and_rebuild(self, new, extra=()):
        """The growth step of train.py:259-260 (`add_farfield_points` from the new rows on, + `rebuild_bvh`) as ONE call (csrc/grow.hip): one out-of-place
        append launch writes the 8 parameters (old rows + new rows), the 16 moments (old rows + zeros) and the caller's per-row extras (old rows + fill),
        then the tree is rebuilt. `new`: the dict GaussianParams.append_points takes (mean, opacity, scale, rotation, rgb, normal, roughness, f0: GPU or CPU
        tensors or arrays with m rows each). `extra`: (tensor, fill_value) pairs - further per-row tensors of the caller's model with 4-byte elements, e.g.
        upstream's `_round_counter` with 0; they come back extended.
        Leaves bit for bit what `pc.append_points(new); self.extend(m); rt.rebuild_bvh()` leave: every parameter a new tensor with a fresh zero `.grad`,
        `steps` unchanged, and in the native holder the old rows' gradients and total_weight with their bits, the new rows' at zero (upstream adds the points
        mid-interval without clearing total_weight). No host read-back. Returns (n_total, [extended extras]).
        Raises ValueError, before anything is touched, for m == 0, for row counts that disagree, and for a model with `export_edited`
        (editing.EditableGaussians keeps per-row selection masks that growth would leave stale: `duplicate_object` is the way to grow an edited scene)."""
        pc = self.pc
        if hasattr(pc, "export_edited"):
            raise ValueError("grow_and_rebuild: an editing model keeps per-row selection masks that new rows would leave stale (use duplicate_object); nothing was changed")
        dev, n = pc._xyz.device, pc._xyz.shape[0]
        src, tail, fill, m = [], [], [], None
        for _, attr, key in GROUPS:  # (the third name of a group is the key of `new`)
            old = getattr(pc, attr)
            if key not in new:
                raise ValueError(f"grow_and_rebuild: new['{key}'] is missing (nothing was changed)")
            v = new[key]
            add = v.detach().to(dev, torch.float32) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v), dtype=torch.float32, device=dev)
            width = old.shape[1]
            if add.numel() % width != 0 or (m is not None and add.numel() // width != m):
                raise ValueError(f"grow_and_rebuild: new['{key}'] has {add.numel()} elements, expected {m if m is not None else 'a multiple of'} x {width} (nothing was changed)")
            m = add.numel() // width
            src.append(old), tail.append(add.reshape(m, width).contiguous()), fill.append(0)
        if m == 0:
            raise ValueError("grow_and_rebuild: no rows to add (nothing was changed)")
        for moments in (self.exp_avg, self.exp_avg_sq):
            for name, _, _ in GROUPS:
                src.append(moments[name]), tail.append(None), fill.append(0)
        for t, value in extra:
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dim() >= 1 and t.shape[0] == n and t.element_size() == 4):
                raise ValueError(f"grow_and_rebuild: per-row extras must be GPU tensors of 4-byte elements with {n} rows (nothing was changed)")
            src.append(t.contiguous()), tail.append(None), fill.append(_word_bits(value, t.dtype))
        out = torch.ops.egr.grow_append(src, tail, fill, m)
        for k, (_, attr, _) in enumerate(GROUPS):
            out[k].grad = torch.zeros_like(out[k])
            setattr(pc, attr, out[k])
        for k, (name, _, _) in enumerate(GROUPS):
            self.exp_avg[name], self.exp_avg_sq[name] = out[8 + k], out[16 + k]
        self.rt.rebuild_bvh()  # resize (keeps the old rows' gradients and weights, zeroes the new ones) + export + full build
        return n + m, out[24:]

    @torch.no_grad()
    def add_farfield_points(self, num_points, radius, seed, cam_centers=None, cam_znear=None, clamp=3.0, init_scale=0.1, init_opa=0.1, init_diffuse=0.2, init_f0=0.04,
                            init_roughness=0.0, normals=0.0, extra=()):
        """gaussian_model.py:233-283 `add_farfield_points(scene)` + `raytracer.rebuild_bvh()` (train.py:259-260) as one call: `num_points` candidates
        (`farfield_candidates(num_points, seed, radius, clamp)`; upstream: 75_000, radius = scene.cameras_extent * cfg.scene_extent_init_radius), those inside a
        camera's znear sphere dropped (`filter_points_near_cameras`: the one read-back, the survivor count), the eight raw tensors from
        `initialization.gaussians_from_cloud` - so scales and opacity carry the bits initialisation gives -, then `grow_and_rebuild`. The defaults are config.py:43-50
        (init_scale_farfield, init_opa_farfield, init_diffuse_farfield, f0 0.04, roughness 0, normal 0). `extra` as in `grow_and_rebuild`.
        Returns (n_added, [extended extras]). The result depends on the arguments alone: ranks that make the same call keep identical clouds.
        Deviations from upstream: the points come from our generator, not torch.randn's stream (same distribution); the ADD_BOOK_INIT_PTS demo switch is not
        built (pass such rows to `grow_and_rebuild`); `num_bounces` is switched by the caller, as train.py:257 does."""
        from .initialization import gaussians_from_cloud

        if hasattr(self.pc, "export_edited"):  # (before the sampling: nothing is launched for a model that cannot grow)
            raise ValueError("add_farfield_points: an editing model cannot grow (see grow_and_rebuild); nothing was changed")
        points = farfield_candidates(num_points, seed, radius, clamp, device=self.pc._xyz.device)
        if cam_centers is not None:
            points = filter_points_near_cameras(points, cam_centers, cam_znear)
        k = points.shape[0]
        if k == 0:
            raise ValueError("add_farfield_points: no candidate lies outside the cameras' znear spheres (nothing was changed)")
        constant = lambda value: torch.full((k, 3), float(value), dtype=torch.float32, device=points.device)
        new = gaussians_from_cloud(points, constant(init_diffuse), normals=constant(normals), init_scale=init_scale, init_opa=init_opa, init_roughness=init_roughness,
                                   init_f0=init_f0)
        n_total, extras = self.grow_and_rebuild(new, extra)
        return k, extras

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
