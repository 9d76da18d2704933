"""The SSIM definition of include/egr_raytracer.h (egr_eval_ssim) restated in numpy fp64, for tests/test_ssim_host.py and tests/test_hip_ssim.py: the normalised
11-tap Gaussian window applied separably (rows, then columns) with zero "same" padding, the five moments, the map. Both flavours and the per-channel sums come
from the map this returns."""
import numpy as np

C1, C2 = 1e-4, 9e-4
E = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5**2))
WINDOW = E / E.sum()


def blur(a):
    """W * a for a [..., H, W] fp64 array: zero padding, rows first."""
    H, W = a.shape[-2:]
    pad = np.zeros(a.shape[:-2] + (H + 10, W + 10))
    pad[..., 5 : H + 5, 5 : W + 5] = a
    rows = sum(WINDOW[k] * pad[..., :, k : k + W] for k in range(11))
    return sum(WINDOW[k] * rows[..., k : k + H, :] for k in range(11))


def ssim_map(p, g):
    """The SSIM map of two [..., H, W] images (any leading axes: channels, views), in fp64. NaN propagates by plain arithmetic."""
    p, g = np.asarray(p, np.float64), np.asarray(g, np.float64)
    with np.errstate(invalid="ignore"):
        mu1, mu2 = blur(p), blur(g)
        s1, s2, s12 = blur(p * p) - mu1 * mu1, blur(g * g) - mu2 * mu2, blur(p * g) - mu1 * mu2
        return ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))


def sums(m):
    """[..., C, H, W] map -> [..., C, 2]: the sum over all pixels and over the interior (the pixels whose window lies inside the image; 0 without one)."""
    return np.stack([m.sum((-2, -1)), m[..., 5:-5, 5:-5].sum((-2, -1))], -1)


def means(m):
    """[..., 3, H, W] map -> [..., 2]: "full" and "interior" (NaN when H < 11 or W < 11)."""
    H, W = m.shape[-2:]
    s = sums(m).sum(-2)
    return np.stack([s[..., 0] / (3 * H * W), s[..., 1] / (3 * (H - 10) * (W - 10)) if H >= 11 and W >= 11 else np.full(s.shape[:-1], np.nan)], -1)
