"""Evaluation in one call: what the reference does for every test camera in train.py:74-169 (`training_report`) and
render.py:195-228 followed by metrics.py - reset the accumulators, render `spp` times, `denoise()`, tonemap prediction and ground truth, clamp,
PSNR of the final, diffuse and specular passes - for V cameras with one batched render (`renderer.render_views_raw`), one batched denoise
(`Raytracer.denoise_views`: 5 launches for V views) and one fused metrics launch pair (`torch.ops.egr.eval_metrics`, csrc/eval.hip) per chunk of
`views_per_call` cameras, and ONE host read-back at the end. With `ssim=True` every chunk makes one more launch pair (`torch.ops.egr.eval_ssim`,
csrc/ssim.hip) on the same tensors: the SSIM of utils/loss_utils.py:39-70 on the same display values, in fp64.

The module also holds the reference's image helpers as plain torch functions, for callers that have images but no cameras: `tonemap` / `untonemap`
(utils/tonemapping.py), `psnr` (utils/image_utils.py) and `display` = tonemap + clamp, the form every image takes before it is compared or saved.
tests/golden/tonemap_vectors.npz and psnr_vectors.npz pin them to the reference's own functions. `ssim` is the fused kernel on display images (GPU only).

SSIM deviates from loss_utils.ssim in two places, deliberately (include/egr_raytracer.h has the definition, DESIGN.md 8f-6 the figures): the arithmetic is fp64
throughout where upstream's is fp32, and the 11-tap Gaussian window is exactly separable and sums to 1 where upstream's 2-D window is an fp32 outer product of
fp32 weights whose sum is off by about 1e-8. The "interior" flavour averages the pixels whose window lies inside the image, the region torchmetrics'
StructuralSimilarityIndexMeasure averages; agreement with torchmetrics itself is unpinned.

`export_views` is the other half of render.py:195-292 and metrics.py: per chunk one more launch set (`torch.ops.egr.eval_frames`, csrc/frames.hip)
turns the seven kinds of a view - render, diffuse, specular, depth, normal, roughness, f0; prediction and ground truth - into bytes on the device and measures the
PSNR of those bytes with integer sums (exact: no summation order, no rounding); one asynchronous copy per chunk brings the bytes to the host, where `formats.write_png`
encodes them on a thread pool while the next chunk renders. `quantise` is the byte rule as plain torch, `frames` the typed wrapper of the op.

Not here: video writing and format_image's bilinear resize to even sizes, LPIPS, SSIM on the bytes (feed `frames / 255` to `ssim`), reading a
ViewSet's fp16 planes in place (targets are fp32, as `camera(i)` hands them out), the per-step all_rays previews, a user-supplied depth scale for views without
target depth, the image file readers of the datasets, and splitting the camera list over ranks (pass `cameras[rank::world]`). The "save" byte rule restates
torchvision's save_image, which is not available where this package is tested: it is a definition here, not pinned by a fixture."""
import json
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import torch

from . import load_library
from .formats import write_png
from .renderer import render_views_raw

PASSES = ("final", "diffuse", "specular")
PASS_TARGETS = ("original_image", "diffuse_image", "specular_image")  # the camera attribute that holds the ground truth of each pass
KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")  # the frames of a view, in the order of include/egr_raytracer.h (bit k of `kinds`)
KIND_TARGETS = PASS_TARGETS + ("depth_image", "normal_image", "roughness_image", "f0_image")
KIND_CHANNELS = (3, 3, 3, 1, 3, 1, 3)
KIND_OUTPUTS = ("final", "rgb", "rgb", "depth", "normal", "roughness", "f0")  # the render output each kind's prediction comes from
ROUNDINGS = {"save": 0, "trunc": 1}  # EGR_FRAMES_ROUND_*
DEPTH_MODES = {"max": 0, "minmax": 1}  # EGR_FRAMES_DEPTH_*
LAYOUTS = {"separate": False, "side_by_side": True}
ENCODE_WORKERS = 8  # PNG encoders at once (zlib releases the GIL); not sized by the CPU count


def tonemap(x, gamma=1.3):
    """The reference's filmic tonemap. NaN -> 0 and +inf -> 1, but -inf, 3e38 (inf / inf) and every negative input (a negative quotient under the power) -> NaN."""
    x = torch.nan_to_num(x, posinf=999999999.9)
    a = 6.2 * x
    return ((x * (a + 0.5)) / (x * (a + 1.7) + 0.06)) ** gamma


def untonemap(y, gamma=1.3, eps=1e-6):
    """The reference's inverse of `tonemap` (its fitted closed form; exact only up to that fit)."""
    r = y ** (1 / gamma)
    root = (r**2 - 0.1512 * r + 0.1783) ** 0.5
    return (0.1371 * r + 0.09549 * root - 0.04032) / (1 - r + eps)


def display(x, gamma=1.3):
    """tonemap + clamp to [0, 1]: what the reference compares and saves. torch.clamp keeps a NaN."""
    return tonemap(x, gamma).clamp(0, 1)


def psnr(img1, img2):
    """The reference's psnr: both images clamped to [0, 1], one mse per entry of the LEADING axis (a CHW image gives three numbers, one per channel: callers
    take .mean()), 20 log10(1 / sqrt(mse)); +inf for identical images. Returns [img1.shape[0], 1]."""
    err = (img1.clamp(0, 1) - img2.clamp(0, 1)) ** 2
    mse = err.reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def ssim(pred, gt):
    """SSIM of display images on the GPU through the fused kernel (`torch.ops.egr.ssim_images`): `pred`, `gt` are [3,H,W] or [V,3,H,W] tensors on one GPU, taken as
    they are (fp32, no tone curve, no clamp). Returns (full, interior), fp64 device tensors of shape [] or [V]: the mean of the SSIM map over all pixels - the
    reference's ssim(pred[None], gt[None]) - and over the pixels whose 11 x 11 window lies inside the image (NaN when H < 11 or W < 11). No host synchronisation.
    There is no CPU arithmetic: CPU tensors raise."""
    load_library()
    if not (pred.is_cuda and gt.is_cuda):
        raise ValueError("ssim: pred and gt must be GPU tensors (the metric is computed by the HIP kernel; there is no CPU path)")
    if pred.dim() not in (3, 4) or pred.shape != gt.shape:
        raise ValueError(f"ssim: pred and gt must both be [3,H,W] or [V,3,H,W], got {tuple(pred.shape)} and {tuple(gt.shape)}")
    batched = pred.dim() == 4
    a, b = (t.to(torch.float32).reshape((-1,) + tuple(t.shape[-3:])).contiguous() for t in (pred, gt))
    _, mean = torch.ops.egr.ssim_images(a, b)
    return (mean[:, 0], mean[:, 1]) if batched else (mean[0, 0], mean[0, 1])


def _stack_targets(cameras, attr, present, H, W, device, channels=3, who="evaluate_views"):
    if not present:
        return None
    imgs = [torch.as_tensor(getattr(c, attr)).to(device, torch.float32) for c in cameras]
    if channels == 1:  # depth_image is [H,W] upstream and [1,H,W] in the framebuffer's layout
        imgs = [t.reshape(1, H, W) if t.numel() == H * W else t for t in imgs]
    for t in imgs:
        if tuple(t.shape) != (channels, H, W):
            raise ValueError(f"{who}: {attr} must be a [{channels},{H},{W}] image (channel-major), got {tuple(t.shape)}")
    return torch.stack(imgs).contiguous()


def _all_have(cameras, attr):
    return bool(cameras) and all(getattr(c, attr, None) is not None for c in cameras)


def _scored_chunks(cameras, raytracer, spp, denoise, znear, zfar, views_per_call, outputs, keep_images, ssim):
    """The chunk loop of `evaluate_views` and `export_views`: per chunk of `views_per_call` cameras ONE batched render of `outputs`, the batched denoise, the
    stacked targets of the three passes and the fused metrics (and SSIM). Yields (first view, cameras of the chunk, render buffers, final, the three targets,
    the chunk's row of numbers [v,3,5(+5)] on the device, the display tensor)."""
    m = raytracer.cuda_module
    H, W = raytracer.image_height, raytracer.image_width
    present = [_all_have(cameras, attr) for attr in PASS_TARGETS]
    for v0 in range(0, len(cameras), views_per_call):
        chunk = cameras[v0 : v0 + views_per_call]
        got = render_views_raw(chunk, raytracer, spp=spp, outputs=outputs, znear=znear, zfar=zfar)
        final = m.denoise_views(got["final"], got["normal"]) if denoise else got["final"]
        targets = [_stack_targets(chunk, attr, on, H, W, got["final"].device) for attr, on in zip(PASS_TARGETS, present)]
        sse, ps, disp = torch.ops.egr.eval_metrics(final, got.get("rgb"), targets[0], targets[1], targets[2], keep_images)
        row = [ps, sse]
        if ssim:
            ssum, smean = torch.ops.egr.eval_ssim(final, got.get("rgb"), targets[0], targets[1], targets[2])
            row += [smean, ssum[..., 0] / float(H * W)]  # [v,3,2] both means and [v,3,3] the per-channel means of the full flavour
        yield v0, chunk, got, final, targets, torch.cat(row, dim=2), disp  # (the row stays on the device)


def _metrics_namespace(table, ssim, num_views, images):
    """The return value of `evaluate_views` from the host table [V,3,5(+5)]."""
    per = lambda col: {name: table[:, k, col].clone() for k, name in enumerate(PASSES)}
    res = SimpleNamespace(psnr=per(0), psnr_global=per(1), sse={name: table[:, k, 2:5].clone() for k, name in enumerate(PASSES)}, images=images)
    res.mean = {name: (float(res.psnr[name].mean()) if num_views else float("nan")) for name in PASSES}
    res.ssim = per(5) if ssim else None
    res.ssim_interior = per(6) if ssim else None
    res.ssim_channels = {name: table[:, k, 7:10].clone() for k, name in enumerate(PASSES)} if ssim else None
    res.mean_ssim = {name: (float(res.ssim[name].mean()) if num_views else float("nan")) for name in PASSES} if ssim else None
    return res


@torch.no_grad()
def evaluate_views(cameras, raytracer, spp=128, denoise=True, znear=0.01, zfar=999.9, views_per_call=8, keep_images=False, ssim=False):
    """Renders, denoises and scores every camera of `cameras`. Per chunk of `views_per_call` cameras: one batched render of final / rgb / normal with
    `spp` accumulated samples per view, the batched denoise of `final` guided by the primary normals (when `denoise`), and one fused launch pair that
    tonemaps, clamps and compares the three passes with the cameras' `original_image` / `diffuse_image` / `specular_image` ([3,H,W]; a pass for which any
    camera lacks its image is absent for the whole call: NaN). The metrics of all chunks stay on the device and are read back ONCE. Returns a namespace:

      psnr          {"final": [V], "diffuse": [V], "specular": [V]} fp64 host tensors: the reference's psnr(pred, gt).mean() (per-channel mse)
      psnr_global   the same keys: 10 log10(1 / mse) over all three channels (torchmetrics' PeakSignalNoiseRatio(data_range=1)), on unquantised floats
      sse           the same keys: [V,3] fp64 sums of squared display differences per channel
      mean          {"final": float, ...}: the mean of `psnr` over the views = training_report's psnr_test / diffuse_psnr_test / specular_psnr_test
      ssim          ssim=True: the same keys, [V] fp64: the mean of the SSIM map over all pixels and channels = the reference's ssim(pred[None], gt[None]), in fp64
      ssim_interior the same keys, [V]: the mean over the pixels whose 11 x 11 window lies inside the image (NaN below 11 x 11)
      ssim_channels the same keys, [V,3]: the per-channel means of `ssim`
      mean_ssim     {"final": float, ...}: the mean of `ssim` over the views. All four are None without `ssim`, and the call makes no SSIM launch
      images        keep_images: per view a SimpleNamespace(final, diffuse, specular, final_gt, diffuse_gt, specular_gt) of [3,H,W] display tensors on the
                    device (None for an absent pass); else None

    As with `render_views`: total_num_calls advances by len(cameras) * spp, the framebuffer is not touched (output_denoised included), and a partitioned
    tracer evaluates whole images on the calling rank. `export_views` adds the frames, the 8-bit metrics and the PNG files."""
    load_library()
    cameras = list(cameras)
    if views_per_call < 1:
        raise ValueError("evaluate_views: views_per_call must be >= 1")
    present = [_all_have(cameras, attr) for attr in PASS_TARGETS]
    need_rgb = present[1] or present[2]
    outputs = ("final",) + (("rgb",) if need_rgb else ()) + (("normal",) if denoise else ())
    numbers, images = [], [] if keep_images else None
    for _, chunk, _, _, _, row, disp in _scored_chunks(cameras, raytracer, spp, denoise, znear, zfar, views_per_call, outputs, keep_images, ssim):
        numbers.append(row)
        if keep_images:
            for v in range(len(chunk)):
                side = lambda k, s: disp[v, k, s] if present[k] else None
                images.append(SimpleNamespace(**{name: side(k, 0) for k, name in enumerate(PASSES)}, **{name + "_gt": side(k, 1) for k, name in enumerate(PASSES)}))
    table = torch.cat(numbers).cpu() if numbers else torch.zeros((0, 3, 10 if ssim else 5), dtype=torch.float64)  # the one read-back
    return _metrics_namespace(table, ssim, len(cameras), images)


def quantise(x, rule="save"):
    """The byte of every value of `x` (any float tensor, CPU or GPU; computed in fp32), as csrc/frames.hip defines it:
      "save"   x * 255, + 0.5, clamp to [0, 255], truncate: torchvision's save_image (0.5 -> 128)
      "trunc"  clamp to [0, 1], * 255, truncate: format_image of render.py:303 (0.5 -> 127)
    NaN gives 0 (torch leaves that conversion unspecified: a definition of this package), +inf 255, -inf 0. Returns a uint8 tensor of x's shape."""
    if rule not in ROUNDINGS:
        raise ValueError(f"quantise: rule must be one of {sorted(ROUNDINGS)}, got {rule!r}")
    x = torch.as_tensor(x).to(torch.float32)
    y = x.mul(255).add(0.5).clamp(0, 255) if rule == "save" else x.clamp(0, 1).mul(255)
    return torch.where(torch.isnan(y), torch.zeros_like(y), y).to(torch.uint8)


def _kind_mask(kinds, who):
    kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
    unknown = [k for k in kinds if k not in KINDS]
    if unknown or not kinds:
        raise ValueError(f"{who}: kinds must be some of {KINDS}, got {kinds}")
    return sum(1 << KINDS.index(k) for k in set(kinds))


def frames(final=None, rgb=None, depth=None, normal=None, roughness=None, f0=None, targets=None, kinds=KINDS, rounding="save", depth_mode="max", layout="separate"):
    """The frames of V views through the fused kernel (`torch.ops.egr.eval_frames`, csrc/frames.hip; GPU only, no CPU arithmetic). The predictions are the buffers of
    `render_views_raw` (final [V,H,W,3], rgb / normal / f0 [V,3,H,W,3], depth / roughness [V,3,H,W,1]); `targets` maps kind names of `KINDS` to channel-major
    [V,C,H,W] tensors (C = 1 for depth and roughness). Everything is optional: a selected kind writes the sides it has. Returns a namespace of device tensors:
      frames       uint8 [V,7,2,H,W,3] (side 0 prediction, 1 ground truth) or, layout="side_by_side", [V,7,H,2W,3]; slots that were not written are unspecified
      sse8         int64 [V,7,3]: the exact sums of squared byte differences per channel; -1 for a selected kind that lacks a side
      psnr8        fp64 [V,7,2]: [0] per-channel-then-mean, [1] over all three channels (metrics.py's number); NaN for a kind that lacks a side
      depth_range  fp32 [V,2]: amin and amax of each view's target depth (when depth is selected and has its target)
    No host synchronisation."""
    load_library()
    targets = dict(targets or {})
    unknown = set(targets) - set(KINDS)
    if unknown:
        raise ValueError(f"frames: unknown target kinds {sorted(unknown)}; expected some of {KINDS}")
    if rounding not in ROUNDINGS or depth_mode not in DEPTH_MODES or layout not in LAYOUTS:
        raise ValueError(f"frames: rounding of {sorted(ROUNDINGS)}, depth_mode of {sorted(DEPTH_MODES)} and layout of {sorted(LAYOUTS)} are required, got {rounding!r}, {depth_mode!r}, {layout!r}")
    out = torch.ops.egr.eval_frames(final, rgb, depth, normal, roughness, f0, *[targets.get(k) for k in KINDS], _kind_mask(kinds, "frames"), ROUNDINGS[rounding],
                                    DEPTH_MODES[depth_mode], LAYOUTS[layout])
    return SimpleNamespace(frames=out[0], sse8=out[1], psnr8=out[2], depth_range=out[3])


def frame_paths(out_dir, index, kind, layout="separate"):
    """The files of one view and kind, as render.py:51-64, 231-292 names them: {"pred": <out_dir>/<kind>/00012_<kind>.png, "gt": <out_dir>/<kind>_gt/...}, or for
    side-by-side frames {"vs": <out_dir>/<kind>_vs/...}."""
    name = "{0:05d}_{1}.png".format(index, kind)
    if LAYOUTS[layout]:
        return {"vs": os.path.join(out_dir, kind + "_vs", name)}
    return {"pred": os.path.join(out_dir, kind, name), "gt": os.path.join(out_dir, kind + "_gt", name)}


@torch.no_grad()
def export_views(cameras, raytracer, out_dir=None, spp=128, denoise=True, kinds=KINDS, layout="separate", depth_mode="max", ssim=False, views_per_call=8, png_level=6,
                 znear=0.01, zfar=999.9, rounding="save", png_filter="up"):
    """render.py's "regular" mode followed by metrics.py: renders, denoises and scores every camera as `evaluate_views` does - the same chunk loop - and turns the
    selected `kinds` of every view into 8-bit frames, prediction and ground truth (the cameras' original / diffuse / specular / depth / normal / roughness / f0
    `_image`; a kind for which any camera lacks its image has no ground truth for the whole call, and depth without it is skipped: both of its sides are scaled by
    the target's range). Per chunk of `views_per_call` cameras: ONE batched render with the outputs the kinds need, the batched denoise, the fused metrics (and
    SSIM), the fused frames (`frames`), and ONE asynchronous copy of the bytes into one of two pinned host buffers; the PNGs of a chunk are encoded on a pool of
    `ENCODE_WORKERS` threads while the next chunk renders. The host waits on the device once per chunk, for that copy, and reads the number tables back once at the
    end; before a pinned buffer is filled again it also waits for the encoder threads of the chunk before last that still read it (a wait on threads, not on the device,
    and over when encoding keeps up with rendering). The copy and the pinned buffers hold the kinds that are written, both sides of each: 2 x views_per_call x kinds x
    6 H W bytes of pinned memory (1080p, 8 views, all seven kinds: 2 x 697 MB; lower `views_per_call` or select fewer kinds to shrink it), and a kind without ground
    truth still copies its unwritten side.

    With `out_dir` the files are <out_dir>/<kind>/{i:05d}_<kind>.png and <out_dir>/<kind>_gt/{i:05d}_<kind>.png (layout="side_by_side": one file per kind that has
    both sides under <out_dir>/<kind>_vs/), and <out_dir>/metrics.json holds {"<kind>": {"psnr": x}} for every selected kind that has both sides: the mean over the
    views of `psnr8_global`, rounded to 2 places - metrics.py's number, measured on the bytes of the files. That is a superset of upstream's keys (metrics.py writes
    render, diffuse and specular; depth, normal, roughness and f0 are added here when selected). With out_dir=None nothing is written.

    Returns `evaluate_views`' namespace (images = None) and
      psnr8, psnr8_global   {kind: [V] fp64}: the per-channel-then-mean and the all-channel PSNR of the bytes (NaN for a kind that lacks a side); selected kinds
      sse8                  {kind: [V,3] int64}: the exact sums of squared byte differences (-1 for a kind that lacks a side)
      depth_range           [V,2] fp32 (amin, amax of each target depth), or None when depth was not written
      files                 per view {kind: {"pred": path, "gt": path}} (or {"vs": path}) of the files written; {} entries without out_dir
      frames                out_dir=None: per view {kind: {"pred": uint8 [H,W,3], "gt": ...}} (or {"vs": [H,2W,3]}) host arrays of the sides that exist; else None
    Framebuffer, accumulators and statistics are left as `evaluate_views` leaves them; total_num_calls advances by len(cameras) * spp."""
    load_library()
    cameras = list(cameras)
    if views_per_call < 1:
        raise ValueError("export_views: views_per_call must be >= 1")
    if layout not in LAYOUTS or depth_mode not in DEPTH_MODES or rounding not in ROUNDINGS:
        raise ValueError(f"export_views: layout of {sorted(LAYOUTS)}, depth_mode of {sorted(DEPTH_MODES)} and rounding of {sorted(ROUNDINGS)} are required")
    mask = _kind_mask(kinds, "export_views")
    selected = [k for k in range(len(KINDS)) if mask >> k & 1]
    H, W = raytracer.image_height, raytracer.image_width
    has_gt = [_all_have(cameras, attr) for attr in KIND_TARGETS]
    written = [k for k in selected if k != 3 or has_gt[3]]  # the kinds that have a prediction side
    sbs = LAYOUTS[layout]
    sides = lambda k: (["vs"] if has_gt[k] else []) if sbs else ["pred"] + (["gt"] if has_gt[k] else [])
    need = {KIND_OUTPUTS[k] for k in written} | ({"rgb"} if has_gt[1] or has_gt[2] else set()) | ({"normal"} if denoise else set())
    outputs = ("final",) + tuple(o for o in ("rgb", "depth", "normal", "roughness", "f0") if o in need)
    copied = [k for k in written if sides(k)]  # the kinds whose bytes travel to the host, in the order of the pinned buffers
    slot = {k: i for i, k in enumerate(copied)}
    rows = min(views_per_call, len(cameras))
    shape = (rows, len(copied), H, 2 * W, 3) if sbs else (rows, len(copied), 2, H, W, 3)
    pinned = [torch.empty(shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)] if cameras and copied else []
    pick = None  # the copied kinds as a device index, made with the first chunk
    jobs = [[], []]  # the encoders (or copies) that still read each pinned buffer
    tables, files, host_frames = [], [{} for _ in cameras], ([{} for _ in cameras] if out_dir is None else None)
    if out_dir is not None:
        for k in written:
            for side in sides(k):
                os.makedirs(os.path.dirname(frame_paths(out_dir, 0, KINDS[k], layout)[side]), exist_ok=True)

    def take(buf, v, k, side):
        return buf[v, slot[k]] if sbs else buf[v, slot[k], 0 if side == "pred" else 1]

    def hand_over(pool, which, v0, n, done):
        """The copy of a chunk has been enqueued: wait for it (the chunk's one host wait) and give its frames to the encoders."""
        done.synchronize()
        buf = pinned[which].numpy()
        for v in range(n):
            for k in copied:
                for side in sides(k):
                    if out_dir is None:
                        host_frames[v0 + v].setdefault(KINDS[k], {})[side] = take(buf, v, k, side).copy()
                    else:
                        path = frame_paths(out_dir, v0 + v, KINDS[k], layout)[side]
                        files[v0 + v].setdefault(KINDS[k], {})[side] = path
                        jobs[which].append(pool.submit(write_png, path, take(buf, v, k, side), png_level, png_filter))

    with ThreadPoolExecutor(ENCODE_WORKERS) as pool:
        waiting = None
        for i, (v0, chunk, got, final, targets, row, _) in enumerate(_scored_chunks(cameras, raytracer, spp, denoise, znear, zfar, views_per_call, outputs, False, ssim)):
            device = final.device
            more = [_stack_targets(chunk, KIND_TARGETS[k], k in selected and has_gt[k], H, W, device, KIND_CHANNELS[k], "export_views") for k in range(3, 7)]
            gts = [t if k in selected else None for k, t in enumerate(targets)] + more
            preds = {name: (final if name == "final" else got.get(name)) for name in ("final", "rgb", "depth", "normal", "roughness", "f0")}
            preds = {name: (t if any(KIND_OUTPUTS[k] == name for k in written) else None) for name, t in preds.items()}
            fr, sse8, psnr8, rng = torch.ops.egr.eval_frames(preds["final"], preds["rgb"], preds["depth"], preds["normal"], preds["roughness"], preds["f0"], *gts, mask,
                                                             ROUNDINGS[rounding], DEPTH_MODES[depth_mode], sbs)
            n = len(chunk)
            # one int64 table per chunk: the fp64 numbers, the 8-bit PSNRs, the integer sums and the depth range as their bit patterns, read back once at the end
            tables.append(torch.cat([row.reshape(n, -1).view(torch.int64), psnr8.reshape(n, -1).view(torch.int64), sse8.reshape(n, -1), rng.view(torch.int64)], dim=1))
            if not copied:  # (side by side without any ground truth: no file, no frame to hand out)
                continue
            which = i & 1
            for j in jobs[which]:  # the encoders of the chunk before last must have let go of this buffer (a wait on threads; none when encoding keeps up)
                j.result()
            jobs[which] = []
            if len(copied) < len(KINDS) and pick is None:
                pick = torch.tensor(copied, dtype=torch.int64, device=device)
            pinned[which][:n].copy_(fr if pick is None else fr.index_select(1, pick), non_blocking=True)  # the ONE copy of the chunk: the kinds that are written
            done = torch.cuda.Event()
            done.record()
            if waiting is not None:
                hand_over(pool, *waiting)  # chunk i - 1 is encoded while chunk i renders
            waiting = (which, v0, n, done)
        if waiting is not None:
            hand_over(pool, *waiting)
        for j in jobs[0] + jobs[1]:
            j.result()
    V, cols = len(cameras), 3 * (10 if ssim else 5)
    table = torch.cat(tables).cpu() if tables else torch.zeros((0, cols + 14 + 21 + 1), dtype=torch.int64)  # the one read-back
    res = _metrics_namespace(table[:, :cols].view(torch.float64).reshape(V, 3, cols // 3), ssim, V, None)
    psnr8 = table[:, cols : cols + 14].view(torch.float64).reshape(V, 7, 2)
    sse8 = table[:, cols + 14 : cols + 35].reshape(V, 7, 3)
    res.psnr8 = {KINDS[k]: psnr8[:, k, 0].clone() for k in selected}
    res.psnr8_global = {KINDS[k]: psnr8[:, k, 1].clone() for k in selected}
    res.sse8 = {KINDS[k]: sse8[:, k].clone() for k in selected}
    res.depth_range = table[:, cols + 35 :].contiguous().view(torch.float32).reshape(V, 2).clone() if 3 in written else None
    res.files, res.frames = files, host_frames
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        scored = {KINDS[k]: {"psnr": round(float(res.psnr8_global[KINDS[k]].mean()), 2)} for k in written if has_gt[k] and V}
        with open(os.path.join(out_dir, "metrics.json"), "w") as f:
            json.dump(scored, f, indent=True)
    return res
