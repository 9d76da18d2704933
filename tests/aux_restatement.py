"""TEST INFRASTRUCTURE ONLY: plain fp64 numpy restatements of two support kernels, in the project's words - not the code under test.

  csrc/step.hip     torch's single-tensor Adam (non-capturable, no amsgrad, no weight decay), one step:
                      m' = m + (1 - beta1) (g - m)                       lerp_
                      v' = beta2 v + (1 - beta2) g g                     mul_ + addcmul_
                      update = lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
                    and the scale decay p' = log(exp(p) d)
  csrc/denoise.hip  the edge-avoiding a-trous filter: 5 passes over [V,H,W,3], 25 taps per pass at holes 1, 2, 4, 8, 16, B3 weights 1/16 1/4 3/8 1/4 1/16 per axis
                    times exp(-|colour difference|^2 / sigma_c^2) exp(-|normal difference|^2 / sigma_n^2), normalised by the weight sum; sigma_c halves after every pass.
                    A tap outside the image is SKIPPED (array slices; never a product with 0), so a non-finite pixel reaches exactly the pixels that read it.

tests/test_aux_restatements.py holds these to torch.optim.Adam in float64 and to tests/test_denoise.py's torch restatement; the GPU tests hold the kernels to them.
(distCUDA2's checker stays oracle/knn.py:dist2_bruteforce.)"""
import numpy as np

B3 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def adam_moments64(m, v, g, beta1, beta2):
    m, v, g = (np.asarray(a, np.float64) for a in (m, v, g))
    return m + (1.0 - beta1) * (g - m), v * beta2 + (1.0 - beta2) * g * g


def adam_update64(m, v, lr, t, beta1, beta2, eps):
    """What one step subtracts from the parameter, given the NEW moments and the 1-based step count t."""
    m, v = np.asarray(m, np.float64), np.asarray(v, np.float64)
    step_size = float(lr) / (1.0 - float(beta1) ** int(t))
    bc2_sqrt = np.sqrt(1.0 - float(beta2) ** int(t))
    return step_size * (m / (np.sqrt(v) / bc2_sqrt + float(eps)))


def scale_decay64(p, d):
    return np.log(np.exp(np.asarray(p, np.float64)) * np.float64(d))


def atrous64(img, normal, sigma_c=0.6, sigma_n=0.3, passes=5):
    cur = np.array(img, np.float64)
    nrm = np.asarray(normal, np.float64)
    assert cur.ndim == 4 and cur.shape[-1] == 3 and nrm.shape == cur.shape
    V, H, W, _ = cur.shape
    for p in range(passes):
        hole = 1 << p
        acc = np.zeros_like(cur)
        wsum = np.zeros((V, H, W, 1))
        for j in range(-2, 3):
            dy = j * hole
            y0, y1 = max(0, -dy), min(H, H - dy)  # the centre rows whose tap row y + dy lies inside the image
            if y0 >= y1:
                continue
            for i in range(-2, 3):
                dx = i * hole
                x0, x1 = max(0, -dx), min(W, W - dx)
                if x0 >= x1:
                    continue
                c, t = (slice(None), slice(y0, y1), slice(x0, x1)), (slice(None), slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                with np.errstate(invalid="ignore", over="ignore", under="ignore"):
                    wc = np.exp(-((cur[t] - cur[c]) ** 2).sum(-1, keepdims=True) / sigma_c ** 2)
                    wn = np.exp(-((nrm[t] - nrm[c]) ** 2).sum(-1, keepdims=True) / sigma_n ** 2)
                    w = B3[i + 2] * B3[j + 2] * wc * wn
                    acc[c] += w * cur[t]
                    wsum[c] += w
        with np.errstate(invalid="ignore"):
            cur = acc / wsum  # (the centre tap always contributes 9/64)
        sigma_c *= 0.5
    return cur
