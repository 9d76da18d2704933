"""A numpy restatement of csrc/priors.hip (include/egr_raytracer.h: egr_prior_pairs / egr_prior_fit / egr_prior_finish), step by step. Where the device
computes in fp32 with one rounding per operation (the projection, the residuals, f0) this does the same in numpy fp32, so those results are comparable bit for
bit; the fits, the errors and the finish are fp64.

    sparse               = project(row, points_world, H, W)        [H,W] fp32, +inf = empty
    x, y, pixels, drops  = pairs(sparse, depth0)
    fit                  = ransac(x, y, table, top_k)              dict(a, b, mask, best_iteration, best_error, errors, models)
    fit                  = lstsq(x, y)
    distance, world, f0  = finish(row, a, b, depth0, normal, metalness)

`row` is one fp32 [25] row of the library's `cams` (priors.camera_rows)."""
import numpy as np

F = np.float32


def project(row, points, H, W):
    row = np.asarray(row, F)
    p = np.asarray(points, F).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    m = row[:12]
    with np.errstate(all="ignore"):
        cx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3]  # fp32 arrays and fp32 scalars: every product and sum is rounded to fp32
        cy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7]
        cz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11]
        u = np.rint(cx * row[12] / cz + row[14])  # halves to even
        v = np.rint(cy * row[13] / cz + row[15])
    assert cx.dtype == F and u.dtype == F
    keep = (cz > 0) & np.isfinite(cz) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    sparse = np.full((H, W), np.inf, F)
    np.minimum.at(sparse, (v[keep].astype(np.int64), u[keep].astype(np.int64)), cz[keep])  # the nearest point of a pixel
    return sparse


def pairs(sparse, depth0):
    """(x, y, flat pixel index per pair, dropped): the pixels under a point in row-major order; a pair whose predicted depth is not finite is dropped."""
    sparse, depth0 = np.asarray(sparse, F), np.asarray(depth0, F)
    pix = np.flatnonzero(np.isfinite(sparse).reshape(-1))
    x, y = depth0.reshape(-1)[pix], sparse.reshape(-1)[pix]
    ok = np.isfinite(x)
    return x[ok], y[ok], pix[ok], int((~ok).sum())


def line_of(mx, my, sxx, sxy):
    """(w, b) in fp32 from fp64 means and centred sums; without spread in x the minimum-norm solution, as lstsq."""
    if sxx == 0.0:
        c = my / (mx * mx + 1.0)
        return F(c * mx), F(c)
    w = sxy / sxx
    return F(w), F(my - w * mx)


def fit_in_order(xs, ys):
    """The hypothesis fit: fp64 sums term by term in sample order (Python floats are IEEE doubles: the same operations as the device's)."""
    xs, ys = [float(v) for v in xs], [float(v) for v in ys]
    mx = my = 0.0
    for a, b in zip(xs, ys):
        mx += a
        my += b
    mx /= float(len(xs))
    my /= float(len(xs))
    sxx = sxy = 0.0
    for a, b in zip(xs, ys):
        dx = a - mx
        sxx += dx * dx
        sxy += dx * (b - my)
    return line_of(mx, my, sxx, sxy)


def fit64(x, y):
    """The refit: fp64 centred normal equations on a set of pairs (numpy's summation order; the device's differs in the last bits of fp64)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mx, my = x.mean(), y.mean()
    return line_of(mx, my, ((x - mx) ** 2).sum(), ((x - mx) * (y - my)).sum())


def residuals(x, y, w, b):
    with np.errstate(all="ignore"):
        r = np.abs(np.asarray(y, F) - (F(w) * np.asarray(x, F) + F(b)))
    assert r.dtype == F
    return r


def hypothesis(x, y, idx, top_k):
    """(w, b, threshold, ties taken, error) of one hypothesis: the fit through the sampled pairs, the top_k-th smallest residual, the fp64 sum of the top_k
    smallest squared residuals."""
    w, b = fit_in_order(np.asarray(x, F)[idx], np.asarray(y, F)[idx])
    r = residuals(x, y, w, b)
    bits = r.view(np.uint32)  # monotone for non-negative floats; +inf and NaN above every number
    thr_bits = np.partition(bits, top_k - 1)[top_k - 1]
    less = bits < thr_bits
    take = top_k - int(less.sum())
    thr = float(np.array([thr_bits], np.uint32).view(F)[0])
    with np.errstate(all="ignore"):
        error = float((r[less].astype(np.float64) ** 2).sum()) + take * (thr * thr)
    return w, b, thr_bits, take, error


def inliers_of(x, y, w, b, thr_bits, take):
    bits = residuals(x, y, w, b).view(np.uint32)
    mask = bits < thr_bits
    mask[np.flatnonzero(bits == thr_bits)[:take]] = True  # the tie rule: the first pairs at the threshold, in pair order
    return mask


def ransac(x, y, table, top_k):
    x, y = np.asarray(x, F), np.asarray(y, F)
    models = [hypothesis(x, y, np.asarray(row, np.int64), top_k) for row in np.asarray(table)]
    errors = np.array([m[4] for m in models], np.float64)
    best = int(np.argmin(np.where(np.isnan(errors), np.inf, errors)))  # the lowest iteration among equals
    w, b, thr_bits, take, _ = models[best]
    mask = inliers_of(x, y, w, b, thr_bits, take)
    a, c = fit64(x[mask], y[mask])
    return dict(a=a, b=c, mask=mask, best_iteration=best, best_error=errors[best], errors=errors, models=models)


def lstsq(x, y):
    a, b = fit64(x, y)
    return dict(a=a, b=b, mask=np.ones(len(x), bool), best_iteration=-1)


def finish(row, a, b, depth0, normal, metalness=None):
    """(distance [H,W], world normals [H,W,3]) in fp64 from fp32 inputs, and f0 [H,W,3] by the fp32 expression (None without metalness)."""
    row = np.asarray(row, F).astype(np.float64)
    d = np.asarray(depth0, F).astype(np.float64)
    H, W = d.shape
    fx, fy, cx, cy = row[12:16]
    Z = d * float(a) + float(b)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    X, Y = (u - cx) * Z / fx, (v - cy) * Z / fy
    distance = np.sqrt(X * X + Y * Y + Z * Z)
    n = -np.asarray(normal, F).astype(np.float64)
    with np.errstate(all="ignore"):
        n = n / np.sqrt((n * n).sum(-1, keepdims=True))
    world = np.einsum("ij,...j->...i", row[16:25].reshape(3, 3), n)
    f0 = None
    if metalness is not None:
        m = np.asarray(metalness, F).reshape(H, W)
        f0 = F(0.04) * (F(1.0) - m) + m
        assert f0.dtype == F
        f0 = np.repeat(f0[:, :, None], 3, axis=2)
    return distance, world, f0
