"""numpy restatement of csrc/viewset.hip (include/egr_raytracer.h: egr_viewset_ingest / egr_viewset_gather): the averaging windows, the order of the fp32 sum,
the one division, the rounding to half, the 8-bit tables, the channel pick, the depth range with NaN, and the gather. Slow and plain on purpose: loops over
windows, numpy fp32 scalars for every operation that rounds."""
import numpy as np

KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")
KIND_CHANNELS = (3, 3, 3, 1, 3, 1, 3)
TABLE_OF_KIND = ("untonemap", "untonemap", "untonemap", None, "normal", "unit", "unit")


def windows(src, dst):
    """[(start, end)] of torch's adaptive average along one axis: floor(i * src / dst) up to but excluding ceil((i + 1) * src / dst)."""
    return [((i * src) // dst, ((i + 1) * src + dst - 1) // dst) for i in range(dst)]


def resized_size(src_height, src_width, height):
    return height, int(height * (src_width / src_height))


def area_u8(img, H, W):
    """uint8 [Hs,Ws,C] -> uint8 [H,W,C]: the integer sum of the window, floor-divided by its element count."""
    Hs, Ws, C = img.shape
    out = np.zeros((H, W, C), np.uint8)
    wide = img.astype(np.int64)
    for y, (r0, r1) in enumerate(windows(Hs, H)):
        for x, (c0, c1) in enumerate(windows(Ws, W)):
            out[y, x] = wide[r0:r1, c0:c1].reshape(-1, C).sum(axis=0) // ((r1 - r0) * (c1 - c0))
    return out


def area_f32(img, H, W):
    """fp32 [Hs,Ws,C] -> fp32 [H,W,C]: per channel the fp32 sum of the window in row-major order starting from +0, then ONE fp32 division by the count."""
    Hs, Ws, C = img.shape
    out = np.zeros((H, W, C), np.float32)
    with np.errstate(all="ignore"):
        for y, (r0, r1) in enumerate(windows(Hs, H)):
            for x, (c0, c1) in enumerate(windows(Ws, W)):
                s = np.zeros(C, np.float32)
                for r in range(r0, r1):
                    for c in range(c0, c1):
                        s = (s + img[r, c]).astype(np.float32)  # one rounding per term and channel
                out[y, x] = s / np.float32((r1 - r0) * (c1 - c0))
    return out


def to_half(x):
    """fp32 -> half, round to nearest even: above 65504 (from 65520) inf, NaN stays NaN, -0 and subnormals as IEEE rounds them."""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float32).astype(np.float16)


def ingest_kind(kind, img, H, W, tables=None):
    """One source image [Hs,Ws,Cs] (uint8 or fp32) of kind index `kind` -> the stored half plane [C,H,W]. `tables`: name -> 256 halfs."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    Hs, Ws, Cs = img.shape
    Co = KIND_CHANNELS[kind]
    assert Cs in (1, 3) and not (Cs == 1 and Co == 3)
    assert (H, W) == ((Hs, Ws) if Hs == H else resized_size(Hs, Ws, H)), "size mismatch"
    img = img[..., :Co]  # depth / roughness: channel 0 of a 3-channel source
    if img.dtype == np.uint8:
        assert TABLE_OF_KIND[kind] is not None, "uint8 depth is refused"
        q = img if Hs == H else area_u8(img, H, W)
        plane = np.asarray(tables[TABLE_OF_KIND[kind]], np.float16)[q]
    else:
        assert img.dtype == np.float32
        plane = to_half(img if Hs == H else area_f32(img, H, W))
    return np.ascontiguousarray(np.moveaxis(plane, -1, 0))


def depth_range(plane):
    """(min, max) of a stored half depth plane as fp32; any NaN gives (NaN, NaN)."""
    f = np.asarray(plane, np.float16).astype(np.float32)
    if np.isnan(f).any():
        return np.array([np.nan, np.nan], np.float32)
    return np.array([f.min(), f.max()], np.float32)


def gather(planes, idx):
    """planes half [n,C,H,W] -> fp32 [V,C,H,W]: exactly float(half) of the views idx."""
    return np.asarray(planes, np.float16)[np.asarray(idx, np.int64)].astype(np.float32)
