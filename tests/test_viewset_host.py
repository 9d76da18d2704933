"""CPU checks of the view store's host side (dataset.py) and of the numpy restatement of its kernels (viewset_restatement.py): the 8-bit tables against the
reference's functions (tests/golden/camera_u8_tables.npz), the restated resize against torch's area interpolation, the sampler, and what is derived from the
camera table. No device is needed: nothing here launches."""
import importlib
import os
import random
from types import SimpleNamespace

import numpy as np
import pytest

import viewset_restatement as vr

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESIZES = ((45, 80, 32), (27, 48, 20), (54, 96, 24), (33, 50, 32))  # (Hs, Ws, H); W follows from _resize_image_tensor's rule
MORE_RESIZES = ((40, 64, 16), (23, 37, 23))


@pytest.fixture(scope="module")
def ds():
    return importlib.import_module(PKG + ".dataset")


def torch_area(x, H, W):
    """_resize_image_tensor's interpolate on an [Hs,Ws,C] fp32 tensor -> [H,W,C]."""
    return torch.nn.functional.interpolate(x.permute(2, 0, 1)[None], (H, W), mode="area")[0].permute(1, 2, 0)


def test_tables_equal_the_fixture_bit_for_bit(ds):
    gold = np.load(os.path.join(GOLD, "camera_u8_tables.npz"))
    tables = ds.u8_tables()
    assert set(tables) == {"untonemap", "normal", "unit"}
    for name, t in tables.items():
        assert t.dtype == torch.float16 and tuple(t.shape) == (256,) and not t.is_cuda
        got = t.numpy().view(np.uint16)
        assert np.array_equal(got, gold[name]), (name, np.flatnonzero(got != gold[name])[:8])
        assert not bool(torch.isnan(t).any()), name
    u = tables["untonemap"]
    assert float(u[255]) == float("inf") and bool(torch.isfinite(u[:255]).all())  # a saturated byte: 1 - y + eps is 1.01e-6 in half and the quotient overflows
    assert float(tables["normal"][0]) == -1.0 and float(tables["normal"][255]) == 1.0 and float(tables["unit"][255]) == 1.0
    assert ds.TABLE_OF_KIND == vr.TABLE_OF_KIND and ds.KINDS == vr.KINDS and ds.KIND_CHANNELS == vr.KIND_CHANNELS


def test_windows_are_torchs_adaptive_windows():
    assert vr.windows(45, 32)[:4] == [(0, 2), (1, 3), (2, 5), (4, 6)] and vr.windows(45, 32)[-1] == (43, 45)
    assert vr.windows(7, 7) == [(i, i + 1) for i in range(7)]
    for src, dst in ((1080, 768), (45, 32), (33, 32), (50, 48), (5, 1)):
        w = vr.windows(src, dst)
        assert w[0][0] == 0 and w[-1][1] == src and all(a < b for a, b in w) and all(w[i + 1][0] <= w[i][1] for i in range(dst - 1))


def test_window_sizes_of_the_gpu_cases():
    """What the shapes of test_hip_viewset.py exercise. 45 x 80 -> 32 x 56 has the windows of 1080 -> 768 (2 and 3). 33 x 50 -> 32 x 48 has windows of 2 only - a
    window of 1 needs both of its ends on the source grid, so a source that is not smaller than the output by a whole factor never has one -; 24 x 36 -> 32 x 48
    (an enlargement, which the same rule covers) has windows of 1 and 2."""
    sizes = lambda src, dst: {b - a for a, b in vr.windows(src, dst)}
    assert vr.resized_size(45, 80, 32) == (32, 56) and sizes(45, 32) == {2, 3} and sizes(80, 56) == {2, 3} and sizes(1080, 768) == {2, 3}
    assert vr.resized_size(33, 50, 32) == (32, 48) and sizes(33, 32) == {2} and sizes(50, 48) == {2}
    assert vr.resized_size(24, 36, 32) == (32, 48) and sizes(24, 32) == {1, 2} and sizes(36, 48) == {1, 2}
    assert vr.resized_size(90, 160, 64) == (64, 113)


@pytest.mark.parametrize("Hs,Ws,H", RESIZES)
def test_restated_uint8_resize_equals_torch_exactly(Hs, Ws, H):
    W = vr.resized_size(Hs, Ws, H)[1]
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 256, (Hs, Ws, 3), generator=g, dtype=torch.uint8)
    want = torch_area(x.float(), H, W).byte().numpy()  # _resize_image_tensor: .float() -> area -> .byte()
    got = vr.area_u8(x.numpy(), H, W)
    assert got.shape == want.shape == (H, W, 3)
    assert int((got != want).sum()) == 0


def half_steps(a, b):
    """Distance of two finite half arrays in units of the half grid (0 = equal, 1 = neighbours)."""
    key = lambda h: np.where(h.view(np.int16) < 0, -(h.view(np.int16).astype(np.int32) & 0x7FFF), h.view(np.int16).astype(np.int32))
    return np.abs(key(a) - key(b))


def test_restated_fp32_resize_against_torch():
    g = torch.Generator().manual_seed(3)
    total = unequal = 0
    for Hs, Ws, H in RESIZES + MORE_RESIZES:
        W = vr.resized_size(Hs, Ws, H)[1]
        x = torch.randint(0, 256, (Hs, Ws, 3), generator=g).float() / 64.0  # multiples of 1/64 in [0, 4): window sums are exact in fp32
        want = torch_area(x, H, W).half().numpy()
        got = vr.to_half(vr.area_f32(x.numpy(), H, W))
        assert got.shape == want.shape == (H, W, 3)
        steps = half_steps(got, want)
        assert int(steps.max()) <= 1, (Hs, Ws, H, int(steps.max()))  # every element within one half ulp
        total += steps.size
        unequal += int((steps != 0).sum())
    print(f"REPORT viewset_fp32_resize: unequal={unequal} of {total}")
    assert total == 18861
    assert unequal <= total // 1000  # at most 0.1 %


def test_restated_fp32_mean_is_within_its_error_bound():
    """A sum of n terms plus one division: the fp32 value before the half rounding is within n * 2^-24 relative of the fp64 mean (positive inputs)."""
    rng = np.random.default_rng(5)
    for Hs, Ws, H in RESIZES:
        W = vr.resized_size(Hs, Ws, H)[1]
        x = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (Hs, Ws, 3))).astype(np.float32)
        got = vr.area_f32(x, H, W).astype(np.float64)
        for y, (r0, r1) in enumerate(vr.windows(Hs, H)):
            for xx, (c0, c1) in enumerate(vr.windows(Ws, W)):
                n = (r1 - r0) * (c1 - c0)
                mean = x[r0:r1, c0:c1].astype(np.float64).reshape(-1, 3).mean(axis=0)
                assert np.all(np.abs(got[y, xx] - mean) <= n * 2.0 ** -24 * mean), (Hs, Ws, H, y, xx)


def test_restated_conversions_channel_pick_and_range(ds):
    tables = {k: t.numpy() for k, t in ds.u8_tables().items()}
    rng = np.random.default_rng(2)
    u8 = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    for kind, name in ((0, "untonemap"), (4, "normal"), (6, "unit")):
        plane = vr.ingest_kind(kind, u8, 5, 7, tables)
        assert plane.dtype == np.float16 and plane.shape == (3, 5, 7)
        assert np.array_equal(plane.view(np.uint16), np.moveaxis(tables[name][u8], -1, 0).view(np.uint16))
    rough = vr.ingest_kind(5, u8, 5, 7, tables)  # three channels in: channel 0 is stored
    assert rough.shape == (1, 5, 7) and np.array_equal(rough[0].view(np.uint16), tables["unit"][u8[..., 0]].view(np.uint16))
    with pytest.raises(AssertionError):
        vr.ingest_kind(3, u8, 5, 7, tables)  # uint8 depth
    f = np.array([[np.nan, np.inf, -np.inf, 65504.0, 65519.0, 65520.0, 1e-8, -0.0, 3e-8, 6e-6]], np.float32)[..., None]
    h = vr.ingest_kind(3, f, 1, 10)[0, 0]
    assert np.isnan(h[0]) and h[1] == np.inf and h[2] == -np.inf and h[3] == 65504 and h[4] == 65504 and h[5] == np.inf and h[6] == 0 and np.signbit(h[7]) and h[7] == 0
    assert h[8] == np.float16(2.0 ** -24) and h[9] == np.float16(6e-6)  # subnormals of half
    assert np.isnan(vr.depth_range(h)).all()
    r = vr.depth_range(np.array([[2.5, 2.5], [2.5, 2.5]], np.float16))
    assert r.dtype == np.float32 and r.tolist() == [2.5, 2.5]
    planes = rng.standard_normal((4, 1, 2, 3)).astype(np.float16)
    got = vr.gather(planes, [3, 3, 0])
    assert got.dtype == np.float32 and np.array_equal(got, planes[[3, 3, 0]].astype(np.float32))


def test_sampler_draws_upstreams_stack(ds):
    vs = SimpleNamespace(n=7)
    s = ds.ViewSet.sampler(vs, seed=11, views_per_step=3)
    draws = [next(s) for _ in range(14)]  # 42 indices = 6 epochs of 7, refilled in the middle of a batch (7 is no multiple of 3)
    flat = [i for b in draws for i in b]
    assert all(len(b) == 3 for b in draws)
    for e in range(6):
        assert sorted(flat[7 * e : 7 * e + 7]) == list(range(7)), e  # every epoch is a permutation
    assert len({tuple(flat[7 * e : 7 * e + 7]) for e in range(6)}) > 1
    # upstream's loop (train.py:218-220) with the same generator
    rng, stack, want = random.Random(11), [], []
    for _ in range(42):
        if not stack:
            stack = list(range(7))
        want.append(stack.pop(rng.randint(0, len(stack) - 1)))
    assert flat == want
    again = ds.ViewSet.sampler(vs, seed=11, views_per_step=3)
    assert [next(again) for _ in range(14)] == draws  # reproducible from the seed
    other = ds.ViewSet.sampler(vs, seed=12, views_per_step=3)
    assert [next(other) for _ in range(14)] != draws
    with pytest.raises(ValueError):
        ds.ViewSet.sampler(SimpleNamespace(n=0), seed=1)


def test_camera_table_and_what_is_derived_from_it(ds):
    """The host side needs no device: a store on the CPU takes the camera rows; the depth ranges (the ingest's output) are set by hand."""
    rng = np.random.default_rng(9)
    n = 5
    infos = []
    for i in range(n):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        infos.append(SimpleNamespace(R=q, T=rng.standard_normal(3) * 3.0, FovY=0.6 + 0.01 * i))
    vs = ds.ViewSet(4, 6, n + 2, device="cpu", znear_scaledown=0.8, zfar_scaleup=1.5)
    assert len(vs) == 0
    with pytest.raises(ValueError):
        vs.train([0], None)  # an empty set
    with pytest.raises(ValueError):
        vs.cameras_extent
    vs._write_cameras(0, infos)
    rng_depth = np.array([[0.5 + i, 3.0 + 2 * i] for i in range(n)], np.float32)
    vs.depth_range[:n] = torch.from_numpy(rng_depth)
    vs.n = n
    centres = np.stack([-np.asarray(c.R, np.float64) @ np.asarray(c.T, np.float64) for c in infos])
    assert tuple(vs.R.shape) == (n, 3, 3) and tuple(vs.centers.shape) == (n, 3) and tuple(vs.fovy.shape) == (n,)
    assert vs.R.dtype == vs.centers.dtype == vs.fovy.dtype == torch.float32
    assert np.array_equal(vs.centers.numpy(), centres.astype(np.float32))  # -R T in fp64, then fp32 (camera_from_RT)
    assert np.array_equal(vs.R.numpy(), np.stack([c.R for c in infos]).astype(np.float32))
    assert np.array_equal(vs.fovy.numpy(), np.array([c.FovY for c in infos], np.float32))
    want = 1.1 * np.linalg.norm(centres - centres.mean(axis=0, keepdims=True), axis=1).max()
    assert vs.cameras_extent == pytest.approx(want, rel=1e-15)
    assert np.array_equal(vs.znear.numpy(), rng_depth[:, 0] * np.float32(0.8)) and np.array_equal(vs.zfar.numpy(), rng_depth[:, 1] * np.float32(1.5))  # fp32 products
    assert vs.max_zfar == float((rng_depth[:, 1] * np.float32(1.5)).max())
    cam = vs.camera(2)
    ren = importlib.import_module(PKG + ".renderer")
    ref = ren.camera_from_RT(infos[2].R, infos[2].T, infos[2].FovY, device="cpu")
    assert np.array_equal(cam.R, ref.R) and cam.FoVy == ref.FoVy and torch.equal(cam.camera_center, ref.camera_center) and np.array_equal(cam.T, ref.T)
    assert float(cam.znear) == float(vs.znear[2]) and float(cam.zfar) == float(vs.zfar[2])
    assert cam.original_image is None and cam.depth_image is None  # no view has brought a kind yet
    with pytest.raises(IndexError):
        vs.camera(n)
    with pytest.raises(ValueError):
        vs.add([infos[0]] * 3)  # beyond num_views
    # what add refuses before it launches anything
    img = lambda h, w, c=3, dt=np.float32: np.zeros((h, w, c), dt)
    with pytest.raises(ValueError, match="uint8 depth"):
        vs.add([SimpleNamespace(R=infos[0].R, T=infos[0].T, FovY=0.6, depth_image=img(4, 6, 1, np.uint8))])
    with pytest.raises(ValueError, match="mixed sizes"):
        vs.add([SimpleNamespace(R=infos[0].R, T=infos[0].T, FovY=0.6, image=img(4, 6), depth_image=img(8, 12, 1))])
    with pytest.raises(ValueError, match="the store is"):
        vs.add([SimpleNamespace(R=infos[0].R, T=infos[0].T, FovY=0.6, image=img(4, 7))])
    with pytest.raises(ValueError, match="the store is"):
        vs.add([SimpleNamespace(R=infos[0].R, T=infos[0].T, FovY=0.6, image=img(8, 15))])  # resized: 4 x int(4 * (15 / 8)) = 4 x 7
    assert ds.resized_size(8, 13, 4) == (4, 6) and ds.resized_size(1080, 1920, 768) == (768, 1365)
    # what the wrapper hands to the launch: uint8 as it is, every float type as fp32, [H,W] as [H,W,1]
    assert ds.ViewSet._source(np.zeros((4, 6, 3), np.uint8)).dtype == torch.uint8
    for dt in (np.float16, np.float32, np.float64):
        t = ds.ViewSet._source(np.full((4, 6), 0.1, dt))
        assert t.dtype == torch.float32 and tuple(t.shape) == (4, 6, 1) and float(t[0, 0, 0]) == float(np.float32(dt(0.1)))
    assert ds.ViewSet._source(torch.zeros((4, 6, 1), dtype=torch.float16)).dtype == torch.float32
    with pytest.raises(ValueError):
        ds.ViewSet._source(np.zeros((4, 6, 3), np.int32))
    assert len(vs) == n  # nothing was added
