"""The far-field candidate generator of csrc/grow.hip (include/egr_raytracer.h: egr_grow_sample) restated in numpy, from its definition: Philox4x32-10 in
uint64 arithmetic, the 24-bit uniforms, Box-Muller in fp64 rounded to fp32 once, the clamp and the multiply in fp32. Not a test module: test_grow_abi.py pins
its Philox to the published known-answer vectors, test_hip_grow.py holds the kernel to it."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (32-bit words held in uint64) -> [..., 4] uint64 words below 2^32."""
    c = [np.asarray(counter, np.uint64)[..., k] & MASK for k in range(4)]
    k0, k1 = (np.asarray(key, np.uint64)[..., k] & MASK for k in range(2))
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]  # 32 x 32 -> 64 bits: no wrap
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(np.broadcast_arrays(*c), axis=-1)


def words(first, n, seed):
    """The four Philox words of candidates first .. first + n under `seed` (Python ints, taken modulo 2^64): [n, 4] uint64."""
    i = (np.uint64(first % (1 << 64)) + np.arange(n, dtype=np.uint64))  # (first + n < 2^64 is the caller's business, as in the library)
    counter = np.stack([i & MASK, i >> S32, np.zeros(n, np.uint64), np.zeros(n, np.uint64)], axis=-1)
    seed = seed % (1 << 64)
    return philox4x32_10(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def normals(first, n, seed):
    """[n, 3] fp32: the three Box-Muller normals of every candidate, evaluated in fp64 and rounded once."""
    u = ((words(first, n, seed) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    t0, t1 = (2.0 * np.pi) * u[:, 1], (2.0 * np.pi) * u[:, 3]
    return np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1)], axis=-1).astype(np.float32)


def candidates(first, n, seed, radius, clamp=3.0):
    """[n, 3] fp32: clamp(normal, -clamp, +clamp) * radius in fp32."""
    z = normals(first, n, seed)
    return (np.clip(z, np.float32(-clamp), np.float32(clamp)) * np.float32(radius)).astype(np.float32)
