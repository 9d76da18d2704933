"""The dense-init cloud on the GPU (csrc/initcloud.hip, initialization.py) against the fp64 numpy restatement of tests/init_restatement.py and the
reference's own ray directions (tests/golden/reference_cameras.npz: c*_dirs is its run of compute_primary_ray_directions).

Inputs: the six cameras of reference_cameras.npz (33 x 17 up to 96 x 54: non-square, no multiple of the 16 x 16 tile, several workgroups). The depth makes a ray end
on the plane y = -0.5 where it meets it within MAX_T, and at MISS_DEPTH otherwise; voxel_scale 20 (and 8), so that a voxel holds from 1 to a few hundred pixels.

Bars. The kernel's fp64 positions may differ from numpy's by a few ulp (about 1e-13 after the scaling), so every test first asserts ON ITS OWN INPUT that no scaled
coordinate lies within 1e-9 of a half-integer; under that condition coords, counts, n, the order and points are exact: bit-equal, no share left out. A colour may
differ from the fp64 mean by half an fp32 ulp of the value (one rounding) plus 2^-32 (the quantisation step of the fixed-point sums): init_restatement.colour_bound."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import init_restatement as ir  # noqa: E402
from hip_common import ren, report  # noqa: E402,F401
from types import SimpleNamespace  # noqa: E402

pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cameras.npz")

PLANE_Y, MAX_T, MISS_DEPTH = -0.5, 6.0, 2.0
MARGIN = 1e-9


@pytest.fixture(scope="module")
def init(ren):
    mod = importlib.import_module(PKG + ".initialization")
    mod.load_library()
    return mod


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def cams(golden):
    """The six reference cameras as CameraInfo-like objects (numpy, on the host): plane-or-constant depth [H,W,1] fp32 and a fixed random fp32 colour image."""
    rng = np.random.default_rng(11)
    out = []
    for i in range(int(golden["num_cases"])):
        R, T, dirs = golden[f"c{i}_R"], golden[f"c{i}_T"], golden[f"c{i}_dirs"]
        W, H = (int(x) for x in golden[f"c{i}_wh"])
        origin = -R @ T
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (PLANE_Y - origin[1]) / dirs[..., 1]
        depth = np.where(np.isfinite(t) & (t > 0) & (t < MAX_T), t, MISS_DEPTH).astype(np.float32)
        assert depth.shape == (H, W)
        out.append(SimpleNamespace(R=R, T=T, FovY=float(golden[f"c{i}_FoVy"]), depth_image=depth[..., None], diffuse_image=rng.random((H, W, 3), dtype=np.float32)))
    return out


@pytest.fixture(scope="module")
def ref20(cams):
    """The restatement at scale 20, computed once and left unchanged."""
    r = ir.cloud(cams, voxel_scale=20.0, min_count=2)
    report("init_cloud_scale20", pixels=r.num_pixels, voxels=r.voxels, kept=len(r.counts), largest=r.largest, half_integer_margin=f"{r.margin:.2e}")
    assert r.margin > MARGIN
    return r


@pytest.fixture(scope="module")
def got20(init, cams):
    return init.dense_init_cloud(cams, voxel_scale=20.0)


def assert_integer_results(got, ref):
    assert got.coords.dtype == torch.int32 and got.counts.dtype == torch.int32 and got.points.dtype == torch.float32 and got.colors.dtype == torch.float32
    assert tuple(got.coords.shape) == tuple(ref.coords.shape), (tuple(got.coords.shape), ref.coords.shape)
    assert np.array_equal(got.coords.cpu().numpy(), ref.coords)  # the set AND the order
    assert np.array_equal(got.counts.cpu().numpy(), ref.counts)
    assert np.array_equal(got.points.cpu().numpy().view(np.uint32), ref.points.view(np.uint32))
    assert got.dropped == ref.dropped and got.num_pixels == ref.num_pixels


def colour_error(got, ref):
    err = np.abs(got.colors.cpu().numpy().astype(np.float64) - ref.colors)
    return err, ir.colour_bound(ref.colors)


def same(a, b):
    return all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("coords", "points", "colors", "counts")) and a.dropped == b.dropped and a.num_pixels == b.num_pixels


def test_rays_equal_the_references_own_directions(init, golden):
    """positions_out with depth 1 and origin 0 = the unit ray directions: against c*_dirs within 1e-15 absolute (about eight fp64 roundings of 1.1e-16)."""
    worst = 0.0
    for i in range(int(golden["num_cases"])):
        W, H = (int(x) for x in golden[f"c{i}_wh"])
        c2w, _, view_size = init.camera_setup(golden[f"c{i}_R"], golden[f"c{i}_T"], float(golden[f"c{i}_FoVy"]))
        keys, acc = torch.full((16384,), -1, dtype=torch.int64, device="cuda"), torch.zeros((16384, 4), dtype=torch.int64, device="cuda")
        status = torch.zeros(8, dtype=torch.int64, device="cuda")
        pos = torch.full((1, H, W, 3), float("nan"), dtype=torch.float64, device="cuda")
        f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
        torch.ops.egr.voxel_accumulate(keys, acc, status, f64(c2w)[None], torch.zeros((1, 3), dtype=torch.float64, device="cuda"), f64([view_size]),
                                       torch.ones((1, H, W), device="cuda"), torch.zeros((1, H, W, 3), device="cuda"), None, 20.0, 32768.0, pos)
        err = float(np.abs(pos[0].cpu().numpy() - golden[f"c{i}_dirs"]).max())
        worst = max(worst, err)
        assert err <= 1e-15, (i, err)
        assert status.tolist()[1:4] == [H * W, 0, 0]
    report("init_cloud_rays", worst_abs_err=f"{worst:.2e}")


def test_integer_results_are_bit_equal_to_the_restatement(got20, ref20):
    assert len(ref20.counts) > 1000 and ref20.largest > 20 and int((ref20.all_counts == 1).sum()) > 1000  # the input exercises single, small and crowded voxels
    assert_integer_results(got20, ref20)
    keys = ir.pack(got20.coords.cpu().numpy())
    assert np.all(np.diff(keys) > 0)


def test_colours_are_the_correctly_rounded_mean(got20, ref20):
    err, bound = colour_error(got20, ref20)
    report("init_cloud_colours", worst_err=f"{err.max():.2e}", worst_over_bound=f"{(err / bound).max():.3f}")
    assert np.all(err <= bound), float((err / bound).max())
    # the reference's flow - fp32 index_add_ in pixel order, divided by the counts - restated with torch on the CPU: it must be no closer to the fp64 mean at the worst element
    accum = torch.zeros((ref20.voxels, 3), dtype=torch.float32)
    accum.index_add_(0, torch.from_numpy(ref20.inverse), torch.from_numpy(ref20.kept_colours))
    upstream = (accum / torch.from_numpy(ref20.all_counts).unsqueeze(1)).numpy()[ref20.selected]
    upstream_err = float(np.abs(upstream.astype(np.float64) - ref20.colors).max())
    report("init_cloud_colours_vs_upstream_flow", ours=f"{err.max():.2e}", upstream_fp32_flow=f"{upstream_err:.2e}")
    assert err.max() <= upstream_err


def test_order_of_views_chunking_and_growth_change_nothing(init, cams, got20):
    one_by_one = init.VoxelAccumulator(voxel_scale=20.0)
    for c in reversed(cams):
        one_by_one.add([c], views_per_call=1)
    assert same(one_by_one.extract(), got20)
    small = init.VoxelAccumulator(voxel_scale=20.0, initial_capacity=1024)
    small.add(cams)
    assert small.growths >= 3 and small.capacity >= 16384, (small.growths, small.capacity)
    assert same(small.extract(), got20)
    assert same(small.extract(), got20)  # extraction leaves the table as it is
    assert int(small.status[3]) == 0 and int(small.status[0]) == int(one_by_one.status[0])


def test_views_of_one_size_go_into_one_launch(init, cams):
    """Three poses with one image size: one launch of three views = three launches of one = the restatement."""
    H, W = cams[2].depth_image.shape[:2]
    rng = np.random.default_rng(5)
    group = [SimpleNamespace(R=c.R, T=c.T, FovY=c.FovY, depth_image=(1.0 + rng.random((H, W), dtype=np.float32)), diffuse_image=rng.random((H, W, 3), dtype=np.float32)) for c in cams[1:4]]
    ref = ir.cloud(group, voxel_scale=8.0, min_count=2)
    assert ref.margin > MARGIN
    batched = init.dense_init_cloud(group, voxel_scale=8.0, views_per_call=8)
    assert_integer_results(batched, ref)
    err, bound = colour_error(batched, ref)
    assert np.all(err <= bound)
    assert same(init.dense_init_cloud(group, voxel_scale=8.0, views_per_call=1), batched)
    assert same(init.dense_init_cloud(group, voxel_scale=8.0, views_per_call=2), batched)


@pytest.mark.parametrize("min_count", [1, 2, 100000])
def test_min_count(init, cams, min_count):
    ref = ir.cloud(cams, voxel_scale=8.0, min_count=min_count)
    assert ref.margin > MARGIN and ref.largest < 100000
    got = init.dense_init_cloud(cams, voxel_scale=8.0, min_count=min_count)
    assert_integer_results(got, ref)
    if min_count == 100000:
        assert got.points.shape == (0, 3) and got.colors.shape == (0, 3) and got.counts.shape == (0,)
    else:
        err, bound = colour_error(got, ref)
        assert np.all(err <= bound)
        assert len(ref.counts) == (ref.voxels if min_count == 1 else int((ref.all_counts >= 2).sum()))


def test_depth_zero_everywhere_is_one_voxel_at_the_camera(init, cams):
    c = cams[5]
    H, W = c.depth_image.shape[:2]
    zero = SimpleNamespace(R=c.R, T=c.T, FovY=c.FovY, depth_image=np.zeros((H, W), np.float32), diffuse_image=c.diffuse_image)
    got = init.dense_init_cloud([zero], voxel_scale=20.0)
    origin = -c.R @ c.T
    assert np.abs(np.abs(origin * 20.0 - np.floor(origin * 20.0)) - 0.5).min() > MARGIN
    assert got.coords.cpu().numpy().tolist() == [np.rint(origin * 20.0).astype(int).tolist()]
    assert got.counts.tolist() == [H * W] and got.num_pixels == H * W and got.dropped == 0
    mean = c.diffuse_image.reshape(-1, 3).astype(np.float64).mean(0)
    assert np.all(np.abs(got.colors.cpu().numpy()[0] - mean) <= ir.colour_bound(mean) + H * W * 2.0**-53)  # (+ numpy's own fp64 summation error)


def test_uint8_colours_go_through_the_table(init, cams):
    rng = np.random.default_rng(3)
    u8 = [SimpleNamespace(R=c.R, T=c.T, FovY=c.FovY, depth_image=c.depth_image, diffuse_image=rng.integers(0, 250, c.diffuse_image.shape, dtype=np.uint8)) for c in cams]
    ev = importlib.import_module(PKG + ".evaluation")
    table = ev.untonemap(torch.arange(256, device="cuda").float() / 255.0)
    assert float(table[:250].abs().max()) < 32768.0  # every colour of this input is below colour_max
    fed = [SimpleNamespace(R=c.R, T=c.T, FovY=c.FovY, depth_image=c.depth_image, diffuse_image=table[torch.from_numpy(c.diffuse_image).cuda().long()]) for c in u8]  # device tensors
    a, b = init.dense_init_cloud(u8, voxel_scale=20.0), init.dense_init_cloud(fed, voxel_scale=20.0)
    assert a.dropped == 0 and len(a.counts) > 1000 and same(a, b)
    ref = ir.cloud(u8, voxel_scale=20.0, table=table.cpu().numpy())
    assert_integer_results(a, ref)
    assert np.all(colour_error(a, ref)[0] <= colour_error(a, ref)[1])


def test_dropped_pixels_are_counted_and_change_nothing_else(init, cams, ref20):
    bad = [SimpleNamespace(R=c.R, T=c.T, FovY=c.FovY, depth_image=c.depth_image.copy(), diffuse_image=c.diffuse_image.copy()) for c in cams]
    bad[0].depth_image[3, 5] = np.nan
    bad[0].depth_image[4, 6] = np.inf
    bad[1].depth_image[0, 0] = -np.inf
    bad[2].diffuse_image[7, 9, 1] = np.nan
    bad[3].diffuse_image[1, 2, 0] = 40000.0  # above colour_max
    bad[3].diffuse_image[1, 3, 2] = -40000.0
    bad[4].diffuse_image[2, 2, 2] = np.inf
    bad[5].depth_image[10, 11] = 3.0e5  # 6e6 voxels away at scale 20: beyond 2^20
    bad[5].depth_image[53, 95] = 3.0e38  # the scaled coordinate overflows nothing in fp64, and is out of range
    ref = ir.cloud(bad, voxel_scale=20.0)
    assert ref.dropped == 9 and ref.margin > MARGIN and ref.num_pixels == ref20.num_pixels - 9
    got = init.dense_init_cloud(bad, voxel_scale=20.0)
    assert got.dropped == 9
    assert_integer_results(got, ref)
    err, bound = colour_error(got, ref)
    assert np.all(err <= bound) and np.all(np.isfinite(got.colors.cpu().numpy()))
    with pytest.raises(RuntimeError, match="smaller colour_max"):  # 2^31 / 77 < 1e8: the largest voxel could have left int64
        init.dense_init_cloud(cams, voxel_scale=20.0, colour_max=1.0e8)


def test_a_visible_share_of_dropped_pixels_warns(init, cams):
    """Saturated uint8 pixels un-tonemap to about 1.9e5, above the default colour_max: they are dropped, and extract says so; a colour_max that holds them is silent."""
    import warnings

    c = cams[4]
    img = np.full(c.diffuse_image.shape, 128, np.uint8)
    img[:4] = 255  # 4 of 17 rows saturated
    view = SimpleNamespace(R=c.R, T=c.T, FovY=c.FovY, depth_image=c.depth_image, diffuse_image=img)
    with pytest.warns(RuntimeWarning, match="colour_max"):
        got = init.dense_init_cloud([view], voxel_scale=20.0)
    assert got.dropped == 4 * img.shape[1] and got.num_pixels == (img.shape[0] - 4) * img.shape[1]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        kept = init.dense_init_cloud([view], voxel_scale=20.0, colour_max=1.0e6)
    assert kept.dropped == 0 and kept.num_pixels == img.shape[0] * img.shape[1] and float(kept.colors.max()) > 1.0e5


def test_gaussians_from_cloud_and_a_tracer_built_from_it(init, ren, got20):
    from importlib import import_module

    knn = import_module(PKG + ".simple_knn")
    g = init.gaussians_from_cloud(got20.points, got20.colors * 3.0 - 1.0, init_scale=0.7, clamp_max=1.5)
    n = got20.points.shape[0]
    # the same statement in the test's own words, on the device with the project's distCUDA2: every operation is one rounding, so the bits must agree
    floor = torch.tensor(1e-7, device="cuda")
    spacing = torch.maximum(knn.distCUDA2(got20.points), floor).sqrt()
    column = lambda value, width: torch.full((n, width), value, dtype=torch.float32, device="cuda")
    shifted = got20.colors * 3.0 - 1.0
    p = column(0.1, 1)
    want = dict(mean=got20.points, rgb=torch.minimum(torch.maximum(shifted, column(0.0, 3)), column(1.5, 3)), normal=column(0.0, 3), f0=column(0.04, 3), roughness=column(0.1, 1),
                opacity=(p / (1.0 - p)).log(), scale=torch.stack([(spacing * 0.7).log()] * 3, dim=1), rotation=torch.cat([column(1.0, 1), column(0.0, 3)], dim=1))
    assert sorted(g) == sorted(want)
    for k in want:
        assert g[k].dtype == torch.float32 and g[k].shape == want[k].shape and torch.equal(g[k], want[k]), k
    assert float(g["rgb"].min()) == 0.0 and float(g["rgb"].max()) == 1.5
    unclamped = init.gaussians_from_cloud(got20.points, got20.colors * 3.0 - 1.0, normals=torch.ones((n, 3)))
    assert float(unclamped["rgb"].min()) < 0.0 and torch.equal(unclamped["normal"], torch.ones((n, 3), device="cuda"))
    W, H = 64, 48
    rt = ren.GaussianRaytracer(ren.GaussianParams(init.gaussians_from_cloud(got20.points, got20.colors)), W, H, ppll_forward_size=8_000_000, ppll_backward_size=1_000_000)
    m = rt.cuda_module
    assert m.check_bvh() == 0, m.last_error()
    m.get_config().jitter_primary_rays.fill_(False)
    syn = import_module(PKG + ".synthetic")
    eye = np.array([0.3, 1.0, 0.4])
    camera = ren.camera_from_c2w(eye.astype(np.float32), syn.look_at(eye, (0.0, -0.5, 0.0)).astype(np.float32), 0.9)  # above the plane, looking down at it
    with torch.no_grad():
        out = ren.render(camera, rt, targets_available=False)
    torch.cuda.synchronize()
    assert m.get_counters()[11] == 0, "capacity overflow"
    assert bool(torch.isfinite(out.rgb).all())

def test_file_round_trip(init, got20, tmp_path):
    fmt = importlib.import_module(PKG + ".formats")
    path = str(tmp_path / "point_cloud_dense.ply")
    fmt.save_init_cloud(path, got20.points.cpu().numpy(), got20.colors.cpu().numpy())
    points, colors = fmt.read_init_cloud(path)[:2]
    p32, c32 = got20.points.cpu().numpy(), got20.colors.cpu().numpy()
    assert points.shape == p32.shape and len(points) > 1000
    # the ASCII format stores repr(float(x)) of every fp32 value: text that reads back as the same number
    assert np.array_equal(np.asarray(points, np.float32), p32) and np.array_equal(np.asarray(colors, np.float32), c32)
    lines = open(path).read().split("\n")
    first = lines[lines.index("end_header") + 1].split()
    assert lines[1] == "format ascii 1.0" and first == [repr(float(x)) for x in list(p32[0]) + list(c32[0])]

def test_two_full_size_views_from_the_minimum_capacity(init, syn):
    """2 views of 1920 x 1080 of the analytic room in one launch, default scale, the table grown from 1024 slots."""
    views = syn.room_camera_infos(2, 1920, 1080)
    ref = ir.cloud(views, voxel_scale=400.0, min_count=2)
    report("init_cloud_1080p", pixels=ref.num_pixels, voxels=ref.voxels, kept=len(ref.counts), largest=ref.largest, half_integer_margin=f"{ref.margin:.2e}")
    assert ref.margin > MARGIN
    acc = init.VoxelAccumulator(initial_capacity=1024)
    acc.add(views)
    got = acc.extract()
    assert acc.growths == 1 and acc.capacity == 1 << 23 and int(acc.status[3]) == 0  # no pixel without a slot
    assert int(acc.status[0]) == ref.voxels and int(acc.status[4]) == ref.largest and int(acc.status[5]) == len(ref.counts)
    assert_integer_results(got, ref)
    assert np.array_equal(ir.pack(got.coords.cpu().numpy()), ref.keys)
    err, bound = colour_error(got, ref)
    assert np.all(err <= bound), float((err / bound).max())
