"""The fused prune on the GPU (csrc/prune.hip; torch.ops.egr.prune_select / prune_gather; trainer.FusedTrainStep.prune_and_rebuild, trainer.filter_points_near_cameras)
against stock torch: boolean indexing, `tensor / scalar < threshold`, a restatement of scene.select_points_to_prune_near_cameras, and today's four-call pruning
sequence. Every comparison is exact (index lists, masks, bit patterns)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import hip_common as hc
from hip_common import ren  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"

# the implementation's shape (csrc/prune.hip): a workgroup of the select covers ROWS_PER_WG rows, and the ONE workgroup that scans the per-workgroup counts takes
# SCAN_COUNTS_PER_PASS of them per pass - so one pass covers ROWS_PER_WG * SCAN_COUNTS_PER_PASS rows and one row more needs a second pass with a carry
ROWS_PER_WG = 1024  # EGR_PRUNE_ROWS_PER_WG
SCAN_COUNTS_PER_PASS = 1024  # PRUNE_SCAN_THREADS
CAM_CHUNK = 256  # PRUNE_CAM_CHUNK: cameras staged in LDS at a time
SELECT_N = [1, 63, 64, 65, 255, 256, 257, ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1, 3 * ROWS_PER_WG + 17, ROWS_PER_WG * SCAN_COUNTS_PER_PASS + 1]


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    cabi = importlib.import_module(PKG + ".c_abi")
    assert cabi.EGR_PRUNE_ROWS_PER_WG == ROWS_PER_WG
    return importlib.import_module(PKG + ".trainer")


def select_mask(remove):
    src_index, count = torch.ops.egr.prune_select(None, 1.0, 0.0, None, None, None, remove)
    return src_index, int(count.item())


def runs(n, length, wave_offset):
    """`length` removed rows starting `wave_offset` into every fourth wave segment, and centred on every workgroup boundary."""
    rows = torch.arange(n, device="cuda")
    first = ROWS_PER_WG - length // 2
    return ((rows >= wave_offset) & ((rows - wave_offset) % 256 < length)) | ((rows >= first) & ((rows - first) % ROWS_PER_WG < length))


def patterns(n):
    rows = torch.arange(n, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(1000 + n % 997)
    yield "keep_all", torch.zeros(n, dtype=torch.bool, device="cuda")
    yield "keep_row_0", rows != 0
    yield "keep_last_row", rows != n - 1
    yield "alternate", rows % 2 == 1
    yield "random_half", torch.rand(n, device="cuda", generator=gen) < 0.5
    yield "random_keep_2_percent", torch.rand(n, device="cuda", generator=gen) >= 0.02
    yield "runs_of_64", runs(n, 64, 32)  # rows 32..95 of a 256-row stretch: across a wave boundary
    yield "runs_of_100", runs(n, 100, 30)  # rows 30..129: across two
    yield "keep_none", torch.ones(n, dtype=torch.bool, device="cuda")


@pytest.mark.parametrize("n", SELECT_N)
def test_select_equals_nonzero(tr, n):
    payload = torch.arange(n, dtype=torch.int32, device="cuda") * 3 + 1
    for name, remove in patterns(n):
        want = torch.nonzero(~remove).flatten()
        for mask in (remove, remove.to(torch.uint8) * 255 if name == "alternate" else remove.to(torch.uint8)):  # bool and uint8 (any non-zero value removes)
            src_index, count = select_mask(mask)
            assert src_index.dtype == torch.int32 and src_index.shape == (n,)
            assert count == want.numel(), (name, n, count, want.numel())
            assert torch.equal(src_index[:count].long(), want), (name, n)
        if name == "keep_none":
            assert count == 0
        got = torch.ops.egr.prune_gather([payload], src_index, count)[0]  # one width-1 array
        assert got.dtype == torch.int32 and torch.equal(got, payload[~remove]), (name, n)


SPECIAL_BITS = (0x7FC00001, 0x7FA5A5A5, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x3F800000, 0x00000000)


def special_rows(width):
    """[12, width] fp32 rows whose bits a float move could lose: NaNs with payloads (quiet and signalling patterns), +/-inf, -0.0, denormals."""
    bits = np.array(SPECIAL_BITS, np.uint32).view(np.int32)
    return torch.from_numpy(np.repeat(bits[:, None], width, axis=1)).cuda().view(torch.float32)


def test_gather_equals_boolean_indexing_bit_for_bit(tr):
    n = 3 * ROWS_PER_WG + 17
    gen = torch.Generator(device="cuda").manual_seed(5)
    remove = torch.rand(n, device="cuda", generator=gen) < 0.5
    remove[:12] = torch.tensor([0, 1, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.bool, device="cuda")
    keep = ~remove
    src_index, count = select_mask(remove)
    tensors = []
    for width in (1, 3, 4):
        t = torch.randn((n, width), device="cuda", generator=gen)
        t[:12] = special_rows(width)
        t[n - 12 :] = special_rows(width)
        tensors.append(t)
    tensors.append(torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 2), device="cuda", generator=gen, dtype=torch.int32))
    tensors.append(torch.randn(n, device="cuda", generator=gen))  # 1-D: keeps its shape
    out = torch.ops.egr.prune_gather(tensors, src_index, count)
    assert len(out) == len(tensors)
    for t, o in zip(tensors, out):
        want = t[keep]
        assert o.dtype == t.dtype and o.shape == want.shape and o.is_contiguous()
        assert torch.equal(o.view(torch.int32), want.view(torch.int32))
    # 33 arrays: one more than a table of the C ABI holds (the shim splits the list over the same index list)
    many = [torch.randn((n, 1 + k % 4), device="cuda", generator=gen) for k in range(33)]
    out = torch.ops.egr.prune_gather(many, src_index, count)
    assert len(out) == 33
    for t, o in zip(many, out):
        assert torch.equal(o.view(torch.int32), t[keep].view(torch.int32))
    # what the shim refuses
    with pytest.raises(RuntimeError):
        torch.ops.egr.prune_gather([tensors[0][: n - 1]], src_index, count)  # other leading size
    with pytest.raises(RuntimeError):
        torch.ops.egr.prune_gather([tensors[0].double()], src_index, count)  # 8-byte elements
    with pytest.raises(RuntimeError):
        torch.ops.egr.prune_gather([tensors[1][:, :2]], src_index, count)  # not contiguous
    with pytest.raises(RuntimeError):
        torch.ops.egr.prune_gather([tensors[0]], src_index, n + 1)


def test_overlapping_src_and_dst_are_refused(tr):
    """The torch op allocates its outputs, so an overlap can only be asked for through the C ABI: refused with an error before anything is launched."""
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    n = 300
    src_index, count = select_mask(torch.arange(n, device="cuda") % 3 == 0)
    buf = torch.arange(2 * n * 3, dtype=torch.float32, device="cuda")
    before = buf.clone()
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dst_offset in (0, 4, (n * 3 - 1) * 4):  # src == dst, shifted by one word, dst starting in the last word of src
        table = (cabi.egr_prune_array * 1)(cabi.egr_prune_array(src=buf.data_ptr(), dst=buf.data_ptr() + dst_offset, width=3))
        assert L.egr_prune_gather(buf.get_device(), table, 1, n, src_index.data_ptr(), count, stream) != 0
        assert b"out of place" in L.egr_prune_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # the adjacent range is fine, and equals the torch op
    table = (cabi.egr_prune_array * 1)(cabi.egr_prune_array(src=buf.data_ptr(), dst=buf.data_ptr() + n * 3 * 4, width=3))
    assert L.egr_prune_gather(buf.get_device(), table, 1, n, src_index.data_ptr(), count, stream) == 0, L.egr_prune_last_error()
    torch.cuda.synchronize()
    want = torch.ops.egr.prune_gather([before[: n * 3].reshape(n, 3)], src_index, count)[0]
    assert torch.equal(buf[n * 3 : n * 3 + count * 3].reshape(count, 3), want) and torch.equal(buf[: n * 3], before[: n * 3])


def test_weight_criterion_equals_torch_division(tr):
    """`total_weight / divisor < min_weight` against torch's own expression on the same device. The kernel divides in IEEE fp32; torch's `tensor / python_scalar`
    may multiply by a rounded reciprocal, so the two may differ within 1 ulp of the threshold: the weights are CONSTRUCTED at least 6 ulp of min_weight away from
    it (checked below in fp64: more than 4 ulp for every row, none left out), apart from special rows that are exact in both forms."""
    divisor = 125.0  # 1/125 is inexact
    mw = np.float32(0.37)
    ulp = float(np.spacing(mw))
    n = 2 * ROWS_PER_WG + 77
    rng = np.random.default_rng(3)
    steps = np.concatenate([rng.integers(6, 64, n // 2), np.exp(rng.uniform(np.log(64), np.log(2 ** 22), n - n // 2)).astype(np.int64)])  # ulps off the threshold: 6 .. 4M
    quotient = np.float64(mw) + np.where(rng.random(n) < 0.5, -1.0, 1.0) * steps * ulp
    tw = (quotient * divisor).astype(np.float32)  # (rounding tw to fp32 moves tw / divisor by at most half an ulp of the quotient)
    distance = np.abs(tw.astype(np.float64) / divisor - np.float64(mw))
    assert np.all(distance > 4 * ulp) and np.count_nonzero(distance < 16 * ulp) > 100  # nothing left out; and the threshold's neighbourhood is populated
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np.float32)
    tw_all = torch.from_numpy(np.concatenate([tw, specials])).cuda()
    src_index, count = torch.ops.egr.prune_select(tw_all, divisor, float(mw), None, None, None, None)
    count = int(count)
    remove_torch = tw_all / divisor < float(mw)
    assert remove_torch[n:].tolist() == [False, False, True, True, True]  # NaN and +inf are kept, -inf goes (0 < 0.37 goes as well)
    assert count == int((~remove_torch).sum()) and torch.equal(src_index[:count].long(), torch.nonzero(~remove_torch).flatten())
    got_remove = torch.ones(n + 5, dtype=torch.bool, device="cuda")
    got_remove[src_index[:count].long()] = False
    assert torch.equal(got_remove, remove_torch)
    # [N,1], as the native total_weight is shaped
    s2, c2 = torch.ops.egr.prune_select(tw_all[:, None], divisor, float(mw), None, None, None, None)
    assert int(c2) == count and torch.equal(s2[:count], src_index[:count])
    # strict `<`: with divisor 128 both forms are exact, and the row whose quotient EQUALS min_weight is kept (its lower neighbour goes, its upper one stays)
    edge = torch.tensor([128.0 * float(mw), np.nextafter(np.float32(128.0 * float(mw)), np.float32(0)), np.nextafter(np.float32(128.0 * float(mw)), np.float32(100))],
                        dtype=torch.float32, device="cuda")
    assert float(edge[0]) / 128.0 == float(mw)
    s3, c3 = torch.ops.egr.prune_select(edge, 128.0, float(mw), None, None, None, None)
    assert int(c3) == 2 and s3[:2].tolist() == [0, 2]
    assert (edge / 128.0 < float(mw)).tolist() == [False, True, False]
    # min_weight 0: a weight of exactly 0 (either sign) is kept; NaN and +inf kept, negatives and -inf go
    zero = torch.tensor([0.0, -0.0, 1e-30, -1e-30, -np.inf, np.nan, np.inf], dtype=torch.float32, device="cuda")
    s4, c4 = torch.ops.egr.prune_select(zero, divisor, 0.0, None, None, None, None)
    assert s4[: int(c4)].tolist() == [0, 1, 2, 5, 6]
    assert (zero / divisor < 0.0).tolist() == [False, False, False, True, True, False, False]


def near_cameras_torch(points, centers, znear):
    """scene/scene.py:88-105 select_points_to_prune_near_cameras with stock torch calls, one camera at a time."""
    prune = torch.zeros(points.shape[0], dtype=torch.bool, device=points.device)
    for c in range(centers.shape[0]):
        prune |= (points - centers[c]).norm(dim=1) < znear[c]
    return prune


def camera_scene(n, num_cams, seed):
    """(points [n,3], centers [C,3], znear [C]) fp32 arrays: every point sits at a chosen radius - 0.2..0.9 (inside) or 1.1..3 (outside) of its home camera's
    znear - along a random direction from that camera; one camera has znear 0 (removes nothing), point 0 sits exactly AT camera 0's centre (znear > 0: removed) and
    point 1 exactly at the znear-0 camera's. Checked in fp64 on the fp32 values: no | |p - T| - znear | is below 1e-5 * znear, for ANY camera."""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(-1.0, 1.0, (num_cams, 3)).astype(np.float32)
    znear = rng.uniform(0.05, 0.3, num_cams).astype(np.float32)
    zero_cam = None
    if num_cams >= 2:
        zero_cam = num_cams - 2
        znear[zero_cam] = 0.0
    if num_cams == 0:
        return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32), centers, znear
    c64 = centers.astype(np.float64)

    def place(k):  # k points: home camera, radius and direction drawn anew
        home = rng.integers(0, num_cams, k)
        radius = np.where(rng.random(k) < 0.4, rng.uniform(0.2, 0.9, k), rng.uniform(1.1, 3.0, k)) * np.maximum(znear[home], 0.05)
        direction = rng.normal(size=(k, 3))
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        return (c64[home] + radius[:, None] * direction).astype(np.float32)

    def in_band(pts, rel):  # [k] bool: within rel * znear of the surface of ANY camera's sphere
        dist = np.linalg.norm(pts.astype(np.float64)[:, None, :] - c64[None, :, :], axis=2)
        return np.any(np.abs(dist - znear[None, :]) < rel * znear[None, :], axis=1)

    points = place(n)
    for _ in range(20):  # a point that lands near the sphere of a camera other than its home is placed again (a few per 100k pairs)
        bad = in_band(points, 1e-4)
        if not bad.any():
            break
        points[bad] = place(int(bad.sum()))
    points[0] = centers[0]
    if zero_cam is not None:
        points[1] = centers[zero_cam]
    assert not in_band(points, 1e-5).any()
    return points, centers, znear


@pytest.mark.parametrize("num_cams", [0, 1, 7, CAM_CHUNK + 1])
def test_camera_criterion_equals_select_points_to_prune_near_cameras(tr, num_cams):
    n = 2 * ROWS_PER_WG + 100
    p, c, z = camera_scene(n, num_cams, seed=20 + num_cams)
    points, centers, znear = torch.from_numpy(p).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(z).cuda()
    want = near_cameras_torch(points, centers, znear)
    if num_cams:
        assert bool(want[0])  # the point AT camera 0's centre
        assert 0.1 * n < int(want.sum()) < 0.9 * n
    if num_cams >= 2:
        assert not bool(((points - centers[num_cams - 2]).norm(dim=1) < znear[num_cams - 2]).any())  # znear 0 removes nothing, not even the point at its centre
    src_index, count = torch.ops.egr.prune_select(None, 1.0, 0.0, points, centers, znear, None)
    assert int(count) == int((~want).sum()) and torch.equal(src_index[: int(count)].long(), torch.nonzero(~want).flatten())
    kept = tr.filter_points_near_cameras(points, centers, znear)
    assert torch.equal(kept.view(torch.int32), points[~want].view(torch.int32))
    if num_cams == 7:  # plain Python inputs, one znear for all cameras
        kept = tr.filter_points_near_cameras(points, c.tolist(), 0.0)
        assert torch.equal(kept, points)


def test_three_criteria_give_their_union_in_stable_order(tr):
    n = 2 * ROWS_PER_WG + 100
    p, c, z = camera_scene(n, 7, seed=31)
    points, centers, znear = torch.from_numpy(p).cuda(), torch.from_numpy(c).cuda(), torch.from_numpy(z).cuda()
    gen = torch.Generator(device="cuda").manual_seed(8)
    tw = torch.where(torch.rand(n, device="cuda", generator=gen) < 0.3, 1.0, 3.0)  # / 2 = 0.5 or 1.5 against 1.0: exact in every form
    mask = torch.rand(n, device="cuda", generator=gen) < 0.2
    parts = [tw / 2.0 < 1.0, near_cameras_torch(points, centers, znear), mask]
    union = parts[0] | parts[1] | parts[2]
    assert all(int((q & ~(parts[(k + 1) % 3] | parts[(k + 2) % 3])).sum()) > 0 for k, q in enumerate(parts))  # each criterion removes rows no other does
    src_index, count = torch.ops.egr.prune_select(tw, 2.0, 1.0, points, centers, znear, mask)
    assert int(count) == int((~union).sum()) and torch.equal(src_index[: int(count)].long(), torch.nonzero(~union).flatten())


LRS = dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)
EYES = ((-1.7, -1.2, 0.4), (1.6, -1.3, 0.2), (0.0, 1.5, -0.5))  # three views of the synthetic room, so that most gaussians collect weight
LOOKS = ((1.2, 0.5, -0.9), (-1.5, 1.0, -0.5), (0.3, -1.8, 0.6))


def same_sums(a, b):
    """Two [22N] buffers of atomically summed gradients and weights of the same launches: equal to 1e-4 of the largest entry of each of the nine tensors (ten times
    the 1e-5 the project records between two launches)."""
    n = a.numel() // 22
    lo = 0
    for width in (3, 3, 3, 1, 1, 3, 3, 4, 1):
        x, y = a[lo * n : (lo + width) * n], b[lo * n : (lo + width) * n]
        assert float((x - y).abs().max()) <= 1e-4 * float(x.abs().max()), (lo, float((x - y).abs().max()), float(x.abs().max()))
        lo += width


def test_prune_and_rebuild_equals_todays_sequence(tr, ren, syn):
    N, W, H, interval = 20000, 32, 32, 3
    g = syn.make_scene(N, "trained", seed=4)
    tg = syn.make_targets(W, H)
    fov = syn.default_camera()["fov"]
    cameras = [hc.cam_obj(ren, dict(origin=np.array(e, np.float32), c2w=syn.look_at(np.array(e, np.float64), l).astype(np.float32), fov=fov), tg) for e, l in zip(EYES, LOOKS)]
    sides = []
    for _ in range(2):
        pc = ren.GaussianParams(g)
        rt = ren.GaussianRaytracer(pc, W, H, team_help=False)
        rt.cuda_module.get_config().jitter_primary_rays.fill_(False)
        sides.append((pc, rt, tr.FusedTrainStep(pc, rt, LRS)))
    for pc, rt, step in sides:  # total_weight and the moments are real
        for cam in cameras:
            ren.render(cam, rt)
            step.step()
    (pa, ra, sa), (pb, rb, sb) = sides
    ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()
    attrs = [attr for _, attr, _ in tr.GROUPS]
    assert float(ga.total_weight.max()) > 0.0
    # Images of two launches are bit-equal with team help off, but gradients and total_weight are sums of float atomic adds whose order is not (DESIGN section 6
    # records 1e-5 ... 1e-6 of a tensor's maximum between launches): the two sides agree to that level, and side B then takes side A's state bit for bit, so that
    # everything after this line compares the two PRUNING paths and nothing else.
    same_sums(ga.grad_flat, gb.grad_flat)
    gb.grad_flat.copy_(ga.grad_flat)
    for name, attr, _ in tr.GROUPS:
        getattr(pb, attr).copy_(getattr(pa, attr))
        sb.exp_avg[name].copy_(sa.exp_avg[name]), sb.exp_avg_sq[name].copy_(sa.exp_avg_sq[name])
    assert sa.steps == sb.steps == 3

    # the threshold: midway between two adjacent sorted values of tw / interval more than 8 ulp apart, searching outward from the median
    q = np.sort((ga.total_weight.cpu().numpy().reshape(-1) / np.float32(interval)).astype(np.float32))
    mid, min_weight = N // 2, None
    for k in range(100):
        j = mid + (k + 1) // 2 * (1 if k % 2 else -1)
        if q[j + 1] - q[j] > 8 * np.spacing(q[j + 1]):
            min_weight = float(np.float32(0.5 * (np.float64(q[j]) + np.float64(q[j + 1]))))
            break
    assert min_weight is not None and q[j] < min_weight < q[j + 1], "no gap of 8 ulp within 100 positions of the median"
    # one camera sphere, around a gaussian of the cloud; no gaussian within 1e-5 * znear of its surface (fp64 on the CPU)
    xyz = pa._xyz.cpu().numpy().astype(np.float64)
    centre, znear = (xyz[123] + 0.01).astype(np.float32), np.float32(0.35)
    dist = np.linalg.norm(xyz - centre.astype(np.float64), axis=1)
    assert not np.any(np.abs(dist - float(znear)) < 1e-5 * float(znear)) and 10 < np.count_nonzero(dist < znear) < N // 4
    extra = torch.arange(N, dtype=torch.int32, device="cuda") * 7 - 3

    # keep none: ValueError, and nothing was touched
    objects = [getattr(pa, a) for a in attrs] + [sa.exp_avg[n] for n, _, _ in tr.GROUPS] + [sa.exp_avg_sq[n] for n, _, _ in tr.GROUPS]
    copies = [t.clone() for t in objects] + [ga.grad_flat.clone()]
    with pytest.raises(ValueError):
        sa.prune_and_rebuild(min_weight=min_weight, interval=interval, remove_mask=torch.ones(N, dtype=torch.bool, device="cuda"))
    now = [getattr(pa, a) for a in attrs] + [sa.exp_avg[n] for n, _, _ in tr.GROUPS] + [sa.exp_avg_sq[n] for n, _, _ in tr.GROUPS]
    assert all(x is y for x, y in zip(objects, now)) and all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(now + [ga.grad_flat], copies))
    assert ra.cuda_module.get_gaussians().mean.shape[0] == N

    # side A: the one call
    n_kept, (extra_a,) = sa.prune_and_rebuild(min_weight=min_weight, interval=interval, cam_centers=torch.from_numpy(centre)[None].cuda(), cam_znear=[float(znear)], extra=[extra])
    # side B: today's sequence, with the mask written out by the caller
    mask = (gb.total_weight.reshape(-1) / interval < min_weight) | ((pb._xyz - torch.from_numpy(centre).cuda()).norm(dim=1) < float(znear))
    assert 0.25 * N <= int(mask.sum()) <= 0.75 * N
    pb.prune_points(mask)
    sb.prune(~mask)
    gb.total_weight.zero_()
    rb.rebuild_bvh()
    extra_b = extra[~mask]

    assert n_kept == N - int(mask.sum())
    ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()

    def same_state():
        for name, attr, _ in tr.GROUPS:
            assert torch.equal(getattr(pa, attr).view(torch.int32), getattr(pb, attr).view(torch.int32)), attr
            assert torch.equal(sa.exp_avg[name].view(torch.int32), sb.exp_avg[name].view(torch.int32)), name
            assert torch.equal(sa.exp_avg_sq[name].view(torch.int32), sb.exp_avg_sq[name].view(torch.int32)), name

    same_state()
    assert float(sa.exp_avg["xyz"].abs().max()) > 0.0  # (the moments are real)
    assert extra_a.dtype == torch.int32 and torch.equal(extra_a, extra_b)
    for attr in attrs:
        p = getattr(pa, attr)
        assert p.shape[0] == n_kept and p.grad is not None and p.grad.shape == p.shape and float(p.grad.abs().max()) == 0.0
    for gs in (ga, gb):
        assert gs.grad_flat.numel() == 22 * n_kept and float(gs.grad_flat.abs().max()) == 0.0  # native gradients and total_weight
    assert ga.mean.shape[0] == n_kept and torch.equal(ga.mean, pa._xyz)
    assert ra.cuda_module.check_bvh() == 0, ra.cuda_module.last_error()
    assert ra.cuda_module.get_counters()[11] == 0

    # one more iteration and an image: the two sides stay bit-equal. The grad launches of the two sides sum their float atomics in their own order (see above), so
    # side B's step takes side A's sums - after they are shown to agree; the step itself and the image that follows are reproducible (team help off).
    for pc, rt, step in sides:
        ren.render(cameras[0], rt)
    ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()
    assert float(ga.grad_flat[: 21 * n_kept].abs().max()) > 0.0
    same_sums(ga.grad_flat, gb.grad_flat)
    gb.grad_flat.copy_(ga.grad_flat)
    finals = []
    for pc, rt, step in sides:
        step.step()
        with torch.no_grad():
            ren.render(cameras[1], rt, targets_available=False)
        finals.append(rt.cuda_module.get_framebuffer().output_final.clone())
    same_state()
    assert torch.equal(finals[0].view(torch.int32), finals[1].view(torch.int32)) and float(finals[0].abs().max()) > 0.0
    assert ra.cuda_module.get_counters()[11] == 0
