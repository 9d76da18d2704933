"""The fp64 restatements of tests/aux_restatement.py against independent statements of the same operations, on the CPU: torch.optim.Adam on float64 tensors, a first
step computed by hand, tests/test_denoise.py's torch restatement run in float64, and the reach of one NaN pixel through the five a-trous passes."""
import numpy as np
import pytest

import aux_restatement as ar

torch = pytest.importorskip("torch")


def test_adam_restatement_matches_torch_float64_over_8_steps():
    rng = np.random.default_rng(0)
    lr, b1, b2, eps = 2.5e-2, 0.9, 0.999, 1e-15
    p0 = rng.normal(size=(257, 3))
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([{"params": [p], "lr": lr}], lr=0.0, eps=eps, betas=(b1, b2))
    mine, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t in range(1, 9):
        g = rng.normal(size=p0.shape) * 10.0 ** rng.integers(-6, 1)
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        m, v = ar.adam_moments64(m, v, g, b1, b2)
        mine = mine - ar.adam_update64(m, v, lr, t, b1, b2, eps)
        st = opt.state[p]
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(mine, p.detach().numpy(), rtol=1e-12, atol=0)


def test_adam_first_step_by_hand():
    """t = 1, g = 1, zero moments: m = 1 - beta1, v = 1 - beta2, both bias corrections cancel them: the update is lr * 1 / (1 + eps)."""
    lr, b1, b2, eps = 1.6e-4, 0.9, 0.999, 1e-3  # (an eps that shows)
    m, v = ar.adam_moments64(0.0, 0.0, 1.0, b1, b2)
    assert abs(float(m) - 0.1) < 1e-16 and abs(float(v) - 0.001) < 1e-18
    u = float(ar.adam_update64(m, v, lr, 1, b1, b2, eps))
    assert abs(u - lr / (1.0 + eps)) <= 1e-15 * lr
    # t = 2 after g = 1 twice: m = 0.19, v = 0.001999, m_hat = v_hat = 1 again (1 - 0.999^2 cancels three digits of the fp64 sixteen)
    m, v = ar.adam_moments64(m, v, 1.0, b1, b2)
    assert abs(float(ar.adam_update64(m, v, lr, 2, b1, b2, 0.0)) - lr) <= 1e-12 * lr
    assert float(ar.scale_decay64(0.0, 0.5)) == np.log(0.5) and abs(float(ar.scale_decay64(-3.0, 0.999)) - (-3.0 + np.log(0.999))) < 1e-15


def _inputs(rng, V, H, W):
    img = 2 * rng.random((V, H, W, 3)) ** 2
    n = rng.normal(size=(V, H, W, 3))
    return img, n / np.linalg.norm(n, axis=-1, keepdims=True)


@pytest.mark.parametrize("W,H", [(37, 19), (7, 70)])
def test_atrous64_matches_the_torch_restatement_in_float64(W, H):
    from test_denoise import atrous_reference

    img, nrm = _inputs(np.random.default_rng(W), 2, H, W)
    out = ar.atrous64(img, nrm)
    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = np.stack([atrous_reference(torch.tensor(img[v]), torch.tensor(nrm[v])).numpy() for v in range(2)])
    finally:
        torch.set_default_dtype(before)
    assert ref.dtype == np.float64
    assert float(np.abs(out - ref).max()) < 1e-12
    assert float(np.abs(out - img).max()) > 1e-3  # it filters


def test_atrous64_keeps_a_constant_image():
    img = np.full((1, 19, 37, 3), 0.37)
    nrm = np.zeros_like(img)
    nrm[..., 2] = 1.0
    assert float(np.abs(ar.atrous64(img, nrm) - 0.37).max()) < 1e-15


def _reach(H, W, y, x):
    """Which pixels read pixel (y, x) through the five ordered passes, as a boolean dilation that keeps every step of a path inside the image."""
    m = np.zeros((H, W), bool)
    m[y, x] = True
    for p in range(5):
        hole, nxt = 1 << p, np.zeros_like(m)
        for yy, xx in zip(*np.nonzero(m)):
            for j in range(-2, 3):
                for i in range(-2, 3):
                    cy, cx = yy - j * hole, xx - i * hole  # the centre whose tap (j, i) is (yy, xx)
                    if 0 <= cy < H and 0 <= cx < W:
                        nxt[cy, cx] = True
        m = nxt
    return m


def test_atrous64_nan_reach_is_the_125_square():
    W, H = 160, 140
    img, nrm = _inputs(np.random.default_rng(5), 1, H, W)
    img[0, 70, 80, 1] = np.nan
    mask = np.isnan(ar.atrous64(img, nrm)).any(-1)[0]
    want = np.zeros((H, W), bool)
    want[70 - 62:70 + 63, 80 - 62:80 + 63] = True  # 2 * (1 + 2 + 4 + 8 + 16) = 62 either side
    assert int(want.sum()) == 125 * 125 and np.array_equal(mask, want)
    assert np.array_equal(mask, _reach(H, W, 70, 80))


def test_atrous64_nan_reach_from_a_corner():
    """37 x 19, NaN at (0, 0): every path of in-image steps counts and no other. Recorded once: after the passes with holes 1, 2, 4 the reach is rows / columns 0..14,
    hole 8 adds 8 and 16 to them (all 19 rows, columns 0..30), hole 16 the columns 31..36 - here the clipped square IS the whole image; with four passes it is not."""
    W, H = 37, 19
    img, nrm = _inputs(np.random.default_rng(6), 1, H, W)
    img[0, 0, 0, :] = np.nan
    mask = np.isnan(ar.atrous64(img, nrm)).any(-1)[0]
    assert np.array_equal(mask, _reach(H, W, 0, 0))
    assert int(mask.sum()) == W * H
    four = np.isnan(ar.atrous64(img, nrm, passes=4)).any(-1)[0]
    want4 = np.zeros((H, W), bool)
    want4[:, :31] = True
    assert np.array_equal(four, want4) and int(four.sum()) == 19 * 31
