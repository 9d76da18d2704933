"""Host-side mirror of the reference's L3 caller:
editable_gauss_refl/renderer/gaussian_raytracer.py:10-151 (`GaussianRaytracer`) and
editable_gauss_refl/renderer/gaussian_renderer.py:21-92 (`render`).

Same call sequence, attribute names and tensor conventions, so a reference `GaussianModel` / `Camera` can be
passed unchanged: pose conversion R_blender = -R with column 0 re-negated, set_pose(camera_center, R_blender),
fov = FoVy, ZNEAR/ZFAR env overrides, export order, targets CHW -> HWC, zero targets when absent, update_bvh iff
grad mode or forced, raytrace, optional denoise, gradient import by add_.

Additions for the MI355X build: `rank` / `world_size` (image-tile partition), `all_reduce_grads()` which sums
THIS launch's [22N] gradient contribution over ranks with ONE RCCL all-reduce (`parallel.all_reduce_launch_delta`) and folds it
into the persistent gradient buffer, and `gather_outputs()` which completes the images of a partitioned no-grad render on every
rank with one all-gather (`parallel.ImageGather`).
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import make_raytracer
from .parallel import ImageGather, all_reduce_launch_delta


class GaussianParams:
    """Minimal stand-in for the parts of scene/gaussian_model.py:31 the tracer reads (raw, pre-activation tensors
    with the reference's attribute names). `cfg` carries the nine values pushed into the native config."""

    def __init__(self, g, device="cuda", cfg=None):
        # numpy arrays, or tensors on any device (initialization.gaussians_from_cloud): copied, never aliased
        t = lambda a: (a.detach().to(device, torch.float32).clone() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a), dtype=torch.float32, device=device)).contiguous()
        self._xyz, self._opacity, self._scaling, self._rotation = t(g["mean"]), t(g["opacity"]), t(g["scale"]), t(g["rotation"])
        self._diffuse, self._normal, self._roughness, self._f0 = t(g["rgb"]), t(g["normal"]), t(g["roughness"]), t(g["f0"])
        for p in self.parameters():
            p.grad = torch.zeros_like(p)
        self.cfg = cfg or SimpleNamespace(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5,
                                          loss_weight_f0=1.0, loss_weight_roughness=1.0, transmittance_threshold=0.01, alpha_threshold=0.005,
                                          exp_power=3)

    def parameters(self):
        return [self._xyz, self._opacity, self._scaling, self._rotation, self._diffuse, self._normal, self._roughness, self._f0]

    _NAMES = ("_xyz", "_opacity", "_scaling", "_rotation", "_diffuse", "_normal", "_roughness", "_f0")

    @torch.no_grad()
    def prune_points(self, mask):
        """scene/gaussian_model.py:493-531 `prune_points(mask)`: rows with mask == True are REMOVED; every parameter is re-created
        from the kept rows with a fresh zero `.grad` (the gradient of the iteration in flight is dropped, like upstream)."""
        keep = ~mask
        for name in self._NAMES:
            t = getattr(self, name)[keep].contiguous()
            t.grad = torch.zeros_like(t)
            setattr(self, name, t)

    @torch.no_grad()
    def append_points(self, new):
        """scene/gaussian_model.py:533-585 `cat_tensors_to_optimizer` + `densification_postfix` (add_farfield_points): rows are
        appended to every parameter, gradients restart at zero. `new`: dict with the reference's raw attribute names
        (mean, opacity, scale, rotation, rgb, normal, roughness, f0)."""
        src = dict(_xyz="mean", _opacity="opacity", _scaling="scale", _rotation="rotation", _diffuse="rgb", _normal="normal", _roughness="roughness", _f0="f0")
        for name in self._NAMES:
            old = getattr(self, name)
            add = torch.as_tensor(np.asarray(new[src[name]]), dtype=torch.float32, device=old.device).reshape(-1, old.shape[1])
            t = torch.cat([old, add], 0).contiguous()
            t.grad = torch.zeros_like(t)
            setattr(self, name, t)

    # getters read by _export_param_values (gaussian_raytracer.py:41-50); editing.EditableGaussians overrides these
    get_scaling = property(lambda s: torch.exp(s._scaling))
    _get_scaling = property(lambda s: s._scaling)
    _get_rotation = property(lambda s: s._rotation)
    get_xyz = property(lambda s: s._xyz)
    get_diffuse = property(lambda s: s._diffuse)
    get_normal = property(lambda s: s._normal)
    get_roughness = property(lambda s: s._roughness)
    get_f0 = property(lambda s: s._f0)


class GaussianRaytracer:
    OUTPUT_BUFFERS = ("output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance",
                      "output_total_transmittance", "output_ray_origin", "output_ray_direction", "output_final")

    EVAL_MODES = ("gather", "full_image")

    def __init__(self, pc, image_width: int, image_height: int, ppll_forward_size=None, ppll_backward_size=None, rank=0, world_size=1,
                 gather_buffers=None, team_help=None, eval_mode="gather", group=None):
        """`eval_mode` (partitioned tracers only; also a per-call argument): what a no-grad render does.
        "gather": every rank traces its own tiles and the images are completed with ONE all-gather - a COLLECTIVE: every rank of
        `group` must make the call (needs a process group whose size equals `world_size`; without one the rank traces the whole image).
        "full_image": this rank traces the whole image itself, no collective - for the usual `if rank == 0: evaluate()` pattern.
        `group`: the process group of the partition's ranks (None = the default group); used by the gradient all-reduce and the gather."""
        assert eval_mode in self.EVAL_MODES, eval_mode
        self.eval_mode, self.group = eval_mode, group
        self.image_width, self.image_height = image_width, image_height
        # partitioned evaluation renders: which framebuffer outputs `gather_outputs` completes on every rank (default: all ten) and
        # whether every no-grad call does it (False: the caller gathers when it needs the images, e.g. once after the 128 accumulated
        # samples of render.py:195-204 - the accumulators of a rank's own pixels live on that rank)
        self.gather_buffers = tuple(gather_buffers) if gather_buffers is not None else self.OUTPUT_BUFFERS
        self.gather_each_render = True
        self._image_gather = None
        kw = {}
        if ppll_forward_size is not None:
            kw["ppll_forward_size"] = int(ppll_forward_size)
        if ppll_backward_size is not None:
            kw["ppll_backward_size"] = int(ppll_backward_size)
        n = pc.get_scaling.shape[0]
        self.cuda_module = make_raytracer(image_width, image_height, n, **kw)
        self.device = self.cuda_module.get_framebuffer().output_rgb.device  # the tracer's: it may be called with any device current
        if self.cuda_module.get_gaussians().mean.shape[0] != n:  # n == 0: the native holder starts with count = 1 (core/gaussians.h:31)
            self.cuda_module.resize(n)
        self.rank, self.world_size = rank, world_size
        self.import_grads = True  # False: a fused host step (trainer.FusedTrainStep) imports the raytracer gradients itself
        if team_help is not None:  # several waves on one heavy tile (egr_set_team_help; library default: on). Only the order of EXACT depth ties of bounce rays depends on it
            self.cuda_module.set_team_help(bool(team_help))
        if world_size > 1:
            self.cuda_module.set_partition(rank, world_size)
            self.cuda_module.use_grad_delta(True)  # grad launches write a per-launch buffer (the first after a fold stores, further ones add): see all_reduce_grads
        config = self.cuda_module.get_config()  # gaussian_raytracer.py:16-25
        config.loss_weight_diffuse.fill_(pc.cfg.loss_weight_diffuse)
        config.loss_weight_specular.fill_(pc.cfg.loss_weight_specular)
        config.loss_weight_normal.fill_(pc.cfg.loss_weight_normal)
        config.loss_weight_depth.fill_(pc.cfg.loss_weight_depth)
        config.loss_weight_f0.fill_(pc.cfg.loss_weight_f0)
        config.loss_weight_roughness.fill_(pc.cfg.loss_weight_roughness)
        config.transmittance_threshold.fill_(pc.cfg.transmittance_threshold)
        config.alpha_threshold.fill_(pc.cfg.alpha_threshold)
        config.exp_power.fill_(pc.cfg.exp_power)
        self.pc = pc
        self._export_param_values()
        self.cuda_module.rebuild_bvh()

    @torch.no_grad()
    def rebuild_bvh(self):  # gaussian_raytracer.py:33-38
        self.cuda_module.resize(self.pc._xyz.shape[0])
        self._export_param_values()
        self.cuda_module.rebuild_bvh()

    @torch.no_grad()
    def _export_param_values(self):  # gaussian_raytracer.py:41-50 (same order)
        g = self.cuda_module.get_gaussians()
        if hasattr(self.pc, "export_edited"):  # editing.EditableGaussians: edit and export in one launch (csrc/edit.hip)
            self.pc.export_edited(g)
            return
        # the eight copy_ calls upstream, as one multi-tensor launch (same order, same semantics)
        torch._foreach_copy_([g.scale, g.rotation, g.mean, g.opacity, g.rgb, g.normal, g.roughness, g.f0],
                             [self.pc._get_scaling, self.pc._get_rotation, self.pc.get_xyz, self.pc._opacity, self.pc.get_diffuse, self.pc.get_normal,
                              self.pc.get_roughness, self.pc.get_f0])

    @staticmethod
    def _like_holder(tensors, holders, aligned=()):
        """The native checks of update_bvh_from / raytrace(import_into=...): contiguous fp32 tensors on the holder's device with the holder's shapes."""
        ok = lambda t, h: isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == h.device and t.shape == h.shape and t.is_contiguous()
        return all(ok(t, h) for t, h in zip(tensors, holders)) and all(tensors[k].data_ptr() % 16 == 0 for k in aligned)

    @torch.no_grad()
    def _export_and_update_bvh(self):
        """`_export_param_values()` + `update_bvh(True)`: one native pass that reads the model's tensors, leaves their values in the holder's and refits
        (update_bvh_from). An editing model exports through its own launch, and tensors the native checks would refuse take the two calls."""
        m = self.cuda_module
        if not hasattr(self.pc, "export_edited"):
            g = m.get_gaussians()
            src = [self.pc._get_scaling, self.pc._get_rotation, self.pc.get_xyz, self.pc._opacity, self.pc.get_diffuse, self.pc.get_normal, self.pc.get_roughness, self.pc.get_f0]
            if self._like_holder(src, [g.scale, g.rotation, g.mean, g.opacity, g.rgb, g.normal, g.roughness, g.f0], aligned=(1,)):
                m.update_bvh_from(*src, True)
                return
        self._export_param_values()
        m.update_bvh(True)

    def _import_target(self):
        """The model's eight .grad tensors when the grad launch itself can add to them (raytrace(import_into=...)), else None: the caller imports. A tracer
        with a per-launch buffer (a partition) reduces between the launch and the import, so it never fuses."""
        g = self.cuda_module.get_gaussians()
        if not self.import_grads or g.grad_delta.numel() != 0:
            return None
        dst = [p.grad for p in (self.pc._scaling, self.pc._rotation, self.pc._xyz, self.pc._opacity, self.pc._diffuse, self.pc._normal, self.pc._roughness, self.pc._f0)]
        return dst if self._like_holder(dst, [g.scale, g.rotation, g.mean, g.opacity, g.rgb, g.normal, g.roughness, g.f0]) else None

    TARGET_CHANNELS = (3, 3, 1, 3, 1, 3)  # diffuse, specular, depth, normal, roughness, f0 (the order of set_targets_chw)

    def _targets_in_place(self, images, device):
        """The six target images as raytrace(targets=...) takes them - None (absent) or a contiguous fp32 [C,H,W] tensor on the tracer's device - or None
        when one of them is anything else (a CPU tensor, a view, another dtype, an empty tensor): the caller uploads through set_targets_chw then."""
        ok = lambda t, c: t is None or (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.is_contiguous()
                                        and tuple(t.shape) == (c, self.image_height, self.image_width))
        return list(images) if all(ok(t, c) for t, c in zip(images, self.TARGET_CHANNELS)) else None

    @torch.no_grad()
    def _import_param_gradients(self):  # gaussian_raytracer.py:53-62
        g = self.cuda_module.get_gaussians()
        # the eight add_ calls upstream, as one multi-tensor launch
        torch._foreach_add_([self.pc._xyz.grad, self.pc._opacity.grad, self.pc._scaling.grad, self.pc._rotation.grad, self.pc._diffuse.grad,
                             self.pc._normal.grad, self.pc._roughness.grad, self.pc._f0.grad],
                            [g.mean.grad, g.opacity.grad, g.scale.grad, g.rotation.grad, g.rgb.grad, g.normal.grad, g.roughness.grad, g.f0.grad])

    def zero_grad(self):  # gaussian_raytracer.py:64-73 (one fill of the flat buffer == the eight zero_() upstream + total_weight kept)
        g = self.cuda_module.get_gaussians()
        n = g.mean.shape[0]
        g.grad_flat[: 21 * n].zero_()  # the eight gradient tensors are the first 21N floats of the flat buffer; total_weight is the tail

    @torch.no_grad()
    def all_reduce_grads(self):
        """Multi-GPU exchange step: the grad launches since the last fold left this rank's gradients + weights in the
        per-launch buffer `grad_delta` ([22N], 88 MB at N=1M; the first launch after a fold stores, further ones add, nobody clears it);
        ONE all-reduce sums it over the ranks, then it is added to the persistent `grad_flat` (whose total_weight tail lives across a
        whole pruning interval) and the library is told that the buffer is consumed. A collective: every rank of the group calls it.
        No-op when the tracer is not partitioned."""
        g = self.cuda_module.get_gaussians()
        if g.grad_delta.numel():
            all_reduce_launch_delta(g.grad_flat, g.grad_delta, self.group, cuda_module=self.cuda_module)  # (reduce + fold + "consumed" in one call: they must not be separated)

    def _partitioned_eval(self, eval_mode=None):
        """Evaluation (no-grad) renders of a partitioned tracer in "gather" mode: with a process group of the partition's size every rank
        traces its own tiles and the images are all-gathered (`gather_outputs`). In "full_image" mode, or without such a group (a single
        process driving one "rank" of a partition, as tools and tests do), the rank traces the whole image itself."""
        import torch.distributed as dist

        if (eval_mode or self.eval_mode) != "gather":
            return False
        return self.world_size > 1 and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) == self.world_size

    def _set_full_image(self, full):
        """Whole-image no-grad render on a partitioned tracer (no process group, see _partitioned_eval). The library caches the tile
        order of every partition it has seen, so the flip is a pointer swap: no device sync, no upload."""
        if self.world_size > 1:
            self.cuda_module.set_partition(0 if full else self.rank, 1 if full else self.world_size)

    @torch.no_grad()
    def gather_outputs(self, names=None):
        """Completes the framebuffer outputs `names` (default: self.gather_buffers) of the last partitioned no-grad render on every rank:
        one all-gather of each rank's own pixels, bit-identical to a whole-image render. The per-pixel statistics and
        random_seeds stay per rank. A collective over `self.group`. No-op for an unpartitioned tracer and for one in "full_image" mode."""
        if not self._partitioned_eval():
            return
        fb = self.cuda_module.get_framebuffer()
        if self._image_gather is None:
            self._image_gather = ImageGather(self.image_width, self.image_height, self.rank, self.world_size, fb.output_rgb.device)
        self._image_gather.gather([getattr(fb, n) for n in (names or self.gather_buffers)], self.group)

    @staticmethod
    def blender_rotation(R):
        """gaussian_raytracer.py:95-97: R_c2w_blender = -R; R_c2w_blender[:, 0] *= -1."""
        Rb = -R
        Rb[:, 0] = -Rb[:, 0]
        return Rb

    def __call__(self, viewpoint_camera, target=None, target_diffuse=None, target_specular=None, target_depth=None, target_normal=None,
                 target_roughness=None, target_f0=None, force_update_bvh=False, denoise=False, znear=0.01, zfar=999.9, eval_mode=None):
        assert eval_mode is None or eval_mode in self.EVAL_MODES, eval_mode
        grads = torch.is_grad_enabled()
        refit = grads or force_update_bvh  # (then the export below is part of the refit's pass)
        with torch.no_grad():
            # (a numpy or CPU pose stays on the host: set_camera hands its twelve floats to the launch by value, where an upload would wait for the stream)
            R = torch.from_numpy(viewpoint_camera.R) if isinstance(viewpoint_camera.R, np.ndarray) else viewpoint_camera.R
            # gaussian_raytracer.py:94-100 (R_c2w_blender = blender_rotation(R); znear / zfar / fov fill_; set_pose(camera_center, R_c2w_blender)) as ONE launch
            self.cuda_module.set_camera(R, viewpoint_camera.camera_center, float(viewpoint_camera.FoVy), float(os.getenv("ZNEAR", znear)), float(os.getenv("ZFAR", zfar)))
            if not refit:
                self._export_param_values()
            framebuffer = self.cuda_module.get_framebuffer()
            # A grad launch reads the six images where they are (raytrace(targets=...): no copy, framebuffer.target_* untouched) when each is absent or a
            # tensor the native checks take. Otherwise, and for a no-grad render:
            # CHW -> HWC into framebuffer.target_*, zeros when absent (gaussian_raytracer.py:109-137: six copy_ / zero_ calls) - as ONE launch over the
            # pixels of this rank's own tiles (egr_set_targets_chw; the kernel waits for nothing: a temporary's memory is stream-ordered)
            targets = self._targets_in_place([target_diffuse, target_specular, target_depth, target_normal, target_roughness, target_f0], framebuffer.output_rgb.device) if grads else None
            if targets is None:
                self.cuda_module.set_targets_chw(target_diffuse, target_specular, target_depth, target_normal, target_roughness, target_f0)
        if refit:
            # raytrace() follows with the same parameter values: one pass over the cloud exports them, writes the snapshot AND the live records
            self._export_and_update_bvh()
        gathered = not grads and self._partitioned_eval(eval_mode)  # (a collective follows: every rank of the group makes this call - or pass eval_mode="full_image")
        if not grads and not gathered:
            self._set_full_image(True)
        import_into = self._import_target() if grads else None  # (the launch's gather adds to the model's .grad itself)
        try:
            self.cuda_module.raytrace(import_into, targets)  # (`targets` holds the images until the launch is enqueued; their memory is stream-ordered)
        finally:  # a raytrace that raises (stale BVH, exact-stats gate) must not leave a training rank tracing the whole image
            if not grads and not gathered:
                self._set_full_image(False)
        if gathered and (self.gather_each_render or denoise):
            self.gather_outputs()  # every rank now holds the whole image (the denoiser needs it)
        if denoise:
            self.cuda_module.denoise()
        if grads:
            self.all_reduce_grads()
            if self.import_grads and import_into is None:
                self._import_param_gradients()
        return {"render": framebuffer.output_rgb.clone()}


def render(camera, raytracer: GaussianRaytracer, targets_available=True, force_update_bvh=False, denoise=False, znear=0.01, zfar=999.9, eval_mode=None):
    """gaussian_renderer.py:21-92: returns CHW clones rgb[3,3,H,W], final[1,3,H,W], depth/normal/roughness/f0."""
    do_backprop = torch.is_grad_enabled()
    names = ("original_image", "diffuse_image", "specular_image", "normal_image", "f0_image", "roughness_image", "depth_image")
    tg = {n: (getattr(camera, n, None) if targets_available else None) for n in names}
    with torch.set_grad_enabled(do_backprop):
        raytracer(camera, target=tg["original_image"], target_diffuse=tg["diffuse_image"], target_specular=tg["specular_image"],
                  target_depth=tg["depth_image"], target_normal=tg["normal_image"], target_roughness=tg["roughness_image"],
                  target_f0=tg["f0_image"], force_update_bvh=force_update_bvh, denoise=denoise, znear=znear, zfar=zfar, eval_mode=eval_mode)
    fb = raytracer.cuda_module.get_framebuffer()
    cl = lambda t: t.clone().detach().moveaxis(-1, 1)
    return SimpleNamespace(rgb=cl(fb.output_rgb), final=cl(fb.output_denoised) if denoise else cl(fb.output_final), depth=cl(fb.output_depth),
                           normal=cl(fb.output_normal), roughness=cl(fb.output_roughness), f0=cl(fb.output_f0), target=tg["original_image"],
                           target_diffuse=tg["diffuse_image"], target_specular=tg["specular_image"], target_depth=tg["depth_image"],
                           target_normal=tg["normal_image"], target_roughness=tg["roughness_image"], target_f0=tg["f0_image"])


VIEW_OUTPUTS = ("final", "rgb", "depth", "normal", "roughness", "f0")


def _stack_cameras(cameras, device):
    """The cameras of a batch as the tensors the batch launches take, on `device`: R [V,3,3] (dataset c2w rotations), centers [V,3], fovy [V]."""
    as_t = lambda x: torch.from_numpy(np.asarray(x)).float() if isinstance(x, np.ndarray) else torch.as_tensor(x).float()
    R = torch.stack([as_t(c.R).to(device) for c in cameras]) if cameras else torch.zeros((0, 3, 3), device=device)
    centers = torch.stack([as_t(c.camera_center).to(device) for c in cameras]) if cameras else torch.zeros((0, 3), device=device)
    fovy = torch.tensor([float(c.FoVy) for c in cameras], dtype=torch.float32, device=device)
    return R, centers, fovy


def render_views_raw(cameras, raytracer: GaussianRaytracer, spp=1, outputs=VIEW_OUTPUTS, force_update_bvh=False, znear=0.01, zfar=999.9):
    """The launch of `render_views`, returning the batch buffers themselves: dict name -> tensor in the framebuffer's layout with a leading V (final
    [V,H,W,3], the others [V,3,H,W,c]); "final" is always among them. `evaluation.evaluate_views` feeds them to the batched denoise and the fused metrics."""
    cameras = list(cameras)
    outputs = tuple(outputs)
    if "final" not in outputs:
        outputs = ("final",) + outputs  # (the library always writes it)
    m = raytracer.cuda_module
    with torch.no_grad():
        R, centers, fovy = _stack_cameras(cameras, raytracer.device)
        raytracer._export_param_values()
        if force_update_bvh:
            m.update_bvh(True)
        raytracer._set_full_image(True)
        try:
            bufs = m.render_views(R, centers, fovy, float(os.getenv("ZNEAR", znear)), float(os.getenv("ZFAR", zfar)), int(spp), list(outputs))
        finally:
            raytracer._set_full_image(False)
    return dict(zip(outputs, bufs))


def render_views(cameras, raytracer: GaussianRaytracer, spp=1, outputs=VIEW_OUTPUTS, force_update_bvh=False, znear=0.01, zfar=999.9):
    """Batched no-grad render (egr_render_views): every camera of `cameras` with `spp` accumulated samples, in as few launches as the ray
    state allows. View v equals reset_accumulators() + spp x (`render` of cameras[v] with accumulate_samples = spp > 1) bit for bit when team
    help is off; the framebuffer is not touched, total_num_calls advances by len(cameras) * spp. Returns one SimpleNamespace per view with the
    CHW fields of `render` (rgb [3,3,H,W], final [1,3,H,W], depth / roughness [3,1,H,W], normal / f0 [3,3,H,W]); fields not in `outputs`
    are None. Parameters are exported (and the tree refitted with `force_update_bvh`) as by `GaussianRaytracer.__call__`. A partitioned
    tracer renders the whole image on the calling rank (eval_mode="full_image")."""
    cameras = list(cameras)
    got = render_views_raw(cameras, raytracer, spp, outputs, force_update_bvh, znear, zfar)
    views = []
    for v in range(len(cameras)):
        f = lambda k: got[k][v].moveaxis(-1, 1) if k in got else None
        views.append(SimpleNamespace(final=got["final"][v : v + 1].moveaxis(-1, 1), rgb=f("rgb"), depth=f("depth"), normal=f("normal"), roughness=f("roughness"),
                                     f0=f("f0")))
    return views


TRAIN_TARGETS = (("diffuse", "diffuse_image", 3), ("specular", "specular_image", 3), ("depth", "depth_image", 1), ("normal", "normal_image", 3),
                 ("roughness", "roughness_image", 1), ("f0", "f0_image", 3))


def train_views(cameras, raytracer: GaussianRaytracer, targets_available=True, znear=0.01, zfar=999.9):
    """Multi-view training launch (egr_train_views): the grad branch of `GaussianRaytracer.__call__` for every camera of `cameras` at once. The
    parameters are exported and the tree refitted ONCE (all views share them), one launch adds the gradients of all views, then the gradient
    exchange of a partitioned tracer (`all_reduce_grads`) and the import into the parameters' .grad (when `import_grads`) run once. The targets come
    from each camera's *_image attributes as `render` takes them (CHW; absent, or targets_available=False: zeros). Leaves in the gradients what
    `render(cam)` with grad mode on leaves summed over the cameras, and advances total_num_calls by len(cameras); writes no images. NOTE: the
    gradient is the SUM over the views and total_weight grows by all of them (a V-view training step)."""
    cameras = list(cameras)
    W, H = raytracer.image_width, raytracer.image_height
    with torch.no_grad():
        R, centers, fovy = _stack_cameras(cameras, raytracer.device)
        targets = []
        for _, attr, ch in TRAIN_TARGETS:
            imgs = [getattr(c, attr, None) if targets_available else None for c in cameras]
            if all(t is None for t in imgs):
                targets.append(None)  # absent for every view: the library reads zeros
                continue
            zeros = torch.zeros((ch, H, W), dtype=torch.float32, device=raytracer.device)
            targets.append(torch.stack([zeros if t is None else torch.as_tensor(t).to(raytracer.device, torch.float32) for t in imgs]).contiguous())
    train_stacked_views(raytracer, R, centers, fovy, targets, znear, zfar)


def train_stacked_views(raytracer: GaussianRaytracer, R, centers, fovy, targets, znear=0.01, zfar=999.9):
    """What `train_views` does once the batch is stacked (dataset.ViewSet.train comes here straight from its gather): R [V,3,3], centers [V,3], fovy [V] and the
    six `targets` in the order of TRAIN_TARGETS - fp32 [V,C,H,W] on the tracer's device, or None (zeros) - are read in place by the launch."""
    with torch.no_grad():
        raytracer._export_and_update_bvh()  # the launch follows with the same parameter values (fused live records)
        import_into = raytracer._import_target()
        raytracer.cuda_module.train_views_import(R, centers, fovy, float(os.getenv("ZNEAR", znear)), float(os.getenv("ZFAR", zfar)), *targets, import_into)
    raytracer.all_reduce_grads()
    if raytracer.import_grads and import_into is None:
        raytracer._import_param_gradients()


def camera_from_RT(R, T, FoVy, device="cuda", **images):
    """What scene/cameras.py:22-152 holds for a view, from the dataset's (R, T, FovY) (dataset/blender_dataset.py:62-75: R is the
    camera-to-world rotation in COLMAP axes - "stored transposed" -, T the world-to-camera translation): `R` unchanged, `FoVy`, and
    `camera_center` = the translation of the inverse world-to-view matrix (Camera.update via getWorld2View2) = -R T. Pinned by
    tests/golden/reference_cameras.npz, generated by running the reference's Camera class."""
    R = np.asarray(R, np.float64)
    centre = -R @ np.asarray(T, np.float64)
    cam = SimpleNamespace(R=R.astype(np.float32), T=np.asarray(T, np.float32), FoVy=float(FoVy),
                          camera_center=torch.as_tensor(centre.astype(np.float32), device=device))
    for k, v in images.items():
        setattr(cam, k, v)
    return cam


def camera_from_c2w(origin, c2w_blender, fov, **images):
    """Builds a duck-typed reference `Camera` (scene/cameras.py:22) whose .R reproduces `c2w_blender` after the
    caller-side conversion above (R = blender rotation with the inverse flip applied)."""
    Rb = torch.as_tensor(np.asarray(c2w_blender), dtype=torch.float32).clone()
    R = Rb.clone()
    R[:, 0] = -R[:, 0]
    R = -R
    cam = SimpleNamespace(R=R.cuda(), FoVy=float(fov), camera_center=torch.as_tensor(np.asarray(origin), dtype=torch.float32).cuda())
    for k, v in images.items():
        setattr(cam, k, v)
    return cam
