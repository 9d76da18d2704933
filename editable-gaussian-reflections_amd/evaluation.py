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

Not here: PNG / video writing, LPIPS, metrics on 8-bit quantised images (`psnr_global` is computed on the unquantised
floats; metrics.py measures PNG round trips), the depth / normal / roughness / f0 preview images, and splitting the camera list over ranks (pass
`cameras[rank::world]`)."""
from types import SimpleNamespace

import torch

from . import load_library
from .renderer import render_views_raw

PASSES = ("final", "diffuse", "specular")
PASS_TARGETS = ("original_image", "diffuse_image", "specular_image")  # the camera attribute that holds the ground truth of each pass


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


def _stack_targets(cameras, attr, present, H, W, device):
    if not present:
        return None
    imgs = [torch.as_tensor(getattr(c, attr)).to(device, torch.float32) for c in cameras]
    for t in imgs:
        if tuple(t.shape) != (3, H, W):
            raise ValueError(f"evaluate_views: {attr} must be a [3,{H},{W}] image (channel-major), got {tuple(t.shape)}")
    return torch.stack(imgs).contiguous()


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
    tracer evaluates whole images on the calling rank."""
    load_library()
    cameras = list(cameras)
    if views_per_call < 1:
        raise ValueError("evaluate_views: views_per_call must be >= 1")
    m = raytracer.cuda_module
    H, W = raytracer.image_height, raytracer.image_width
    present = [bool(cameras) and all(getattr(c, attr, None) is not None for c in cameras) for attr in PASS_TARGETS]
    need_rgb = present[1] or present[2]
    outputs = ("final",) + (("rgb",) if need_rgb else ()) + (("normal",) if denoise else ())
    numbers, images = [], [] if keep_images else None
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
        numbers.append(torch.cat(row, dim=2))  # [v,3,2+3(+2+3)], stays on the device
        if keep_images:
            for v in range(len(chunk)):
                side = lambda k, s: disp[v, k, s] if present[k] else None
                images.append(SimpleNamespace(**{name: side(k, 0) for k, name in enumerate(PASSES)}, **{name + "_gt": side(k, 1) for k, name in enumerate(PASSES)}))
    table = torch.cat(numbers).cpu() if numbers else torch.zeros((0, 3, 10 if ssim else 5), dtype=torch.float64)  # the one read-back
    per = lambda col: {name: table[:, k, col].clone() for k, name in enumerate(PASSES)}
    res = SimpleNamespace(psnr=per(0), psnr_global=per(1), sse={name: table[:, k, 2:5].clone() for k, name in enumerate(PASSES)}, images=images)
    res.mean = {name: (float(res.psnr[name].mean()) if len(cameras) else float("nan")) for name in PASSES}
    res.ssim = per(5) if ssim else None
    res.ssim_interior = per(6) if ssim else None
    res.ssim_channels = {name: table[:, k, 7:10].clone() for k, name in enumerate(PASSES)} if ssim else None
    res.mean_ssim = {name: (float(res.ssim[name].mean()) if len(cameras) else float("nan")) for name in PASSES} if ssim else None
    return res
