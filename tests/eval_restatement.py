"""Stock-torch restatement of the fused evaluation metrics (csrc/eval.hip; include/egr_raytracer.h: egr_eval_metrics), in fp32 or fp64 and on any device: the three
passes, the tone curve D(x) = clamp(tonemap(x), 0, 1), the per-channel sums of squared differences and both PSNR flavours. tests/test_eval_host.py holds it to
tests/golden/tonemap_vectors.npz (the reference's own functions); tests/test_hip_eval.py holds the kernels to it.

WHICH pixels are NaN is part of the definition and is decided in fp32, the precision the reference evaluates in: 3e38 overflows there (inf / inf) and does not in
fp64. The fp64 restatement therefore computes its values in fp64 and takes the NaN positions from the fp32 evaluation."""
import torch

POSINF = 999999999.9
PASSES = ("final", "diffuse", "specular")


def tone(x, gamma=1.3):
    x = torch.nan_to_num(x, posinf=POSINF)
    s = 6.2 * x
    num, den = x * (s + 0.5), x * (s + 1.7) + 0.06
    return (num / den) ** gamma


def display(x, dtype=torch.float32):
    """D(x) in `dtype`; x is fp32 data."""
    d32 = tone(x.float()).clamp(0, 1)
    if dtype == torch.float32:
        return d32
    d = tone(x.to(dtype)).clamp(0, 1)
    return torch.where(torch.isnan(d32), torch.full_like(d, float("nan")), torch.where(torch.isnan(d), d32.to(dtype), d))


def predictions(final, rgb):
    """The three predictions, channel-major [V,3,H,W] fp32: final [V,H,W,3]; rgb [V,3,H,W,3] -> rgb[:, 0] and rgb[:, 1] + rgb[:, 2] (one fp32 add)."""
    chw = lambda t: t.movedim(-1, 1).contiguous()  # (contiguous: the same elementwise loops as on any other image)
    return [chw(final), chw(rgb[:, 0]) if rgb is not None else None, chw(rgb[:, 1] + rgb[:, 2]) if rgb is not None else None]


def metrics(final, rgb, targets, dtype=torch.float32):
    """targets: three [V,3,H,W] tensors or None. Returns (display [V,3,2,3,H,W] in dtype, sse [V,3,3] in dtype, psnr [V,3,2] in dtype); an absent pass is NaN. In
    fp32 the PSNR is computed as the reference computes it (fp32 mean, sqrt, log10); [..., 1] is 10 log10(1 / mse) over all three channels."""
    V, H, W, _ = final.shape
    dev = final.device
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=dtype, device=dev)
    disp, sse, psnr = nan(V, 3, 2, 3, H, W), nan(V, 3, 3), nan(V, 3, 2)
    for k, (pred, gt) in enumerate(zip(predictions(final, rgb), targets)):
        if pred is None or gt is None:
            continue
        dp, dg = display(pred, dtype), display(gt, dtype)
        disp[:, k, 0], disp[:, k, 1] = dp, dg
        err = (dp - dg) ** 2
        sse[:, k] = err.reshape(V, 3, -1).sum(-1)
        mse_c = err.reshape(V, 3, -1).mean(-1)
        psnr[:, k, 0] = (20 * torch.log10(1.0 / torch.sqrt(mse_c))).mean(-1)
        psnr[:, k, 1] = 10 * torch.log10(1.0 / err.reshape(V, -1).mean(-1))
    return disp, sse, psnr
