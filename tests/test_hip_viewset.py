"""The view store on the GPU (csrc/viewset.hip; torch.ops.egr.viewset_ingest / viewset_gather; dataset.ViewSet): the ingest bit for bit against the numpy
restatement (viewset_restatement.py) - planes and depth ranges -, the gather bit for bit against the stored halfs, and ViewSet.train against
renderer.train_views on the set's own cameras from the same state."""
import functools
import importlib
from types import SimpleNamespace

import numpy as np
import pytest

import hip_common
import viewset_restatement as vr
from hip_common import GRAD_KEYS, generic_targets, hip_grads, ren, views  # noqa: F401
from test_hip_train_views import assert_grads_close, view_targets, zero_native

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
ATTRS = ("image", "diffuse_image", "specular_image", "depth_image", "normal_image", "roughness_image", "f0_image")
tracer = functools.partial(hip_common.tracer, bwd=8_000_000)


@pytest.fixture(scope="module")
def ds():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    return importlib.import_module(PKG + ".dataset")


def pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return dict(R=q, T=rng.standard_normal(3) * 2.0, FovY=float(rng.uniform(0.5, 0.9)))


def image(rng, Hs, Ws, channels, dtype):
    if dtype == "u8":
        return rng.integers(0, 256, (Hs, Ws, channels), dtype=np.uint8)
    return np.exp(rng.uniform(np.log(1e-3), np.log(30.0), (Hs, Ws, channels))).astype(np.float32) * rng.choice(np.float32([1.0, -1.0]), (Hs, Ws, channels), p=[0.8, 0.2])


def make_infos(rng, V, Hs, Ws, spec):
    """spec: kind index -> (channels, "u8" | "f32"); kinds left out are missing."""
    return [SimpleNamespace(**pose(rng), **{ATTRS[k]: image(rng, Hs, Ws, c, dt) for k, (c, dt) in spec.items()}) for _ in range(V)]


def same_range(got, want):
    return np.array_equal(np.asarray(got, np.float32), np.asarray(want, np.float32), equal_nan=True)


def half_bits(h):
    """The bit patterns of a half array with every NaN as one pattern: which NaN an invalid operation gives (inf - inf) differs between processors."""
    bits = np.ascontiguousarray(h).view(np.uint16).copy()
    bits[np.isnan(h)] = 0x7E00
    return bits


def check_store(ds, vs, infos, first=0):
    """Planes, depth ranges and camera rows of the slots first.. against the restatement."""
    tables = {k: t.numpy() for k, t in ds.u8_tables().items()}
    planes = [p.cpu().numpy() for p in vs.planes]
    ranges = vs.depth_range.cpu().numpy()
    for v, info in enumerate(infos):
        for k, attr in enumerate(ATTRS):
            img = getattr(info, attr, None)
            got = planes[k][first + v]
            want = np.zeros_like(got) if img is None else vr.ingest_kind(k, img, vs.height, vs.width, tables)
            assert got.shape == want.shape, (v, attr)
            bad = np.flatnonzero(half_bits(got) != half_bits(want))
            assert bad.size == 0, (v, attr, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
            if k == vr.KINDS.index("depth") and img is not None:
                assert same_range(ranges[first + v], vr.depth_range(want)), (v, ranges[first + v], vr.depth_range(want))
                t = vs.planes[k][first + v].float()
                assert same_range(ranges[first + v], [float(t.amin()), float(t.amax())])  # ... which is torch's amin / amax of the stored plane
        assert np.array_equal(vs.R[first + v].cpu().numpy(), np.asarray(info.R, np.float32))
        assert np.array_equal(vs.centers[first + v].cpu().numpy(), (-np.asarray(info.R, np.float64) @ np.asarray(info.T, np.float64)).astype(np.float32))
        assert float(vs.fovy[first + v]) == float(np.float32(info.FovY))


ALL_U8 = {0: (3, "u8"), 1: (3, "u8"), 2: (3, "u8"), 3: (1, "f32"), 4: (3, "u8"), 5: (1, "u8"), 6: (3, "u8")}  # (uint8 depth does not exist)
ALL_F32 = {0: (3, "f32"), 1: (3, "f32"), 2: (3, "f32"), 3: (3, "f32"), 4: (3, "f32"), 5: (3, "f32"), 6: (3, "f32")}  # three-channel depth / roughness: channel 0
MIXED = {1: (3, "u8"), 3: (3, "f32"), 4: (3, "f32"), 5: (3, "u8"), 6: (3, "u8")}  # render and specular are missing
CASES = [("resize_45x80_u8", 45, 80, 32, ALL_U8, 3, 8), ("resize_45x80_f32", 45, 80, 32, ALL_F32, 1, 8), ("resize_33x50_mixed_chunks_of_2", 33, 50, 32, MIXED, 5, 2),
         ("resize_33x50_f32", 33, 50, 32, {**ALL_F32, 3: (1, "f32"), 5: (1, "f32")}, 3, 8), ("plain_19x37_u8", 19, 37, 19, ALL_U8, 3, 8),
         ("plain_19x37_f32_chunks_of_2", 19, 37, 19, ALL_F32, 5, 2), ("plain_19x37_mixed", 19, 37, 19, MIXED, 1, 8), ("plain_1x1_u8", 1, 1, 1, ALL_U8, 3, 8),
         ("plain_1x1_f32", 1, 1, 1, ALL_F32, 1, 8), ("plain_16x24_u8_chunks_of_2", 16, 24, 16, ALL_U8, 5, 2), ("plain_16x24_f32", 16, 24, 16, ALL_F32, 3, 8),
         ("plain_64x72_two_workgroups_u8", 64, 72, 64, {**ALL_U8, 5: (3, "u8")}, 3, 8), ("resize_90x160_two_workgroups_f32", 90, 160, 64, ALL_F32, 1, 8),
         ("enlarge_24x36_u8", 24, 36, 32, ALL_U8, 3, 8), ("enlarge_24x36_f32", 24, 36, 32, ALL_F32, 1, 8)]  # windows of 1 and 2 (test_viewset_host.py has the window sizes of every case)


@pytest.mark.parametrize("name,Hs,Ws,H,spec,V,per_call", CASES, ids=[c[0] for c in CASES])
def test_ingest_equals_the_restatement(ds, name, Hs, Ws, H, spec, V, per_call):
    rng = np.random.default_rng(len(name) * 131 + Hs)
    W = Ws if Hs == H else vr.resized_size(Hs, Ws, H)[1]
    infos = make_infos(rng, V, Hs, Ws, spec)
    vs = ds.ViewSet(H, W, V + 1)
    vs.add(infos, views_per_call=per_call)
    torch.cuda.synchronize()
    assert len(vs) == V and vs.present == [k in spec for k in range(7)]
    check_store(ds, vs, infos)
    for p in vs.planes:  # the slot nobody filled
        assert not bool(p[V].any())
    assert vs.depth_range[V].tolist() == [0.0, 0.0]
    assert same_range(vs.znear.cpu().numpy(), vs.depth_range[:V, 0].cpu().numpy() * np.float32(0.8))
    assert same_range(vs.zfar.cpu().numpy(), vs.depth_range[:V, 1].cpu().numpy() * np.float32(1.5))


def special_image(Hs, Ws, channels, rng):
    x = image(rng, Hs, Ws, channels, "f32")
    flat = x.reshape(-1)
    vals = np.float32([np.nan, np.inf, -np.inf, 65504.0, 65519.9, 65520.0, 1e-8, -0.0, 3e-8, 6e-6, -65520.0, 70000.0])
    pos = rng.choice(flat.size, vals.size, replace=False)
    flat[pos] = vals
    return x


@pytest.mark.parametrize("Hs,Ws,H", [(19, 37, 19), (16, 24, 16), (33, 50, 32)], ids=["plain_odd", "plain_vector", "resized"])
def test_fp32_special_values_and_the_range(ds, Hs, Ws, H):
    """NaN, +-inf, 65504, 65520 (-> inf), 1e-8 (-> 0), -0 and half subnormals in every kind. View 0's depth has them all (range NaN), view 1's depth has exactly one
    NaN (range NaN), view 2's is finite with both signs, view 3's has one value everywhere (minimum == maximum)."""
    rng = np.random.default_rng(77 + Hs)
    W = Ws if Hs == H else vr.resized_size(Hs, Ws, H)[1]
    infos = []
    for v in range(4):
        kw = {ATTRS[k]: special_image(Hs, Ws, 3, rng) for k in (0, 1, 2, 4, 6)}
        kw[ATTRS[5]] = special_image(Hs, Ws, 1, rng)
        if v == 0:
            depth = special_image(Hs, Ws, 1, rng)
        elif v == 1:
            depth = np.abs(image(rng, Hs, Ws, 1, "f32"))
            depth[Hs // 2, Ws // 3, 0] = np.nan
        elif v == 2:
            depth = image(rng, Hs, Ws, 1, "f32")
        else:
            depth = np.full((Hs, Ws, 1), 2.7182817, np.float32)
        infos.append(SimpleNamespace(**pose(rng), depth_image=depth, **kw))
    vs = ds.ViewSet(H, W, 4)
    vs.add(infos, views_per_call=3)
    torch.cuda.synchronize()
    check_store(ds, vs, infos)
    r = vs.depth_range.cpu().numpy()
    assert np.isnan(r[0]).all() and np.isnan(r[1]).all() and np.isfinite(r[2]).all() and r[2, 0] < 0 < r[2, 1]
    assert r[3, 0] == r[3, 1] == np.float32(np.float16(2.7182817))
    assert np.isnan(vs.znear.cpu().numpy()[:2]).all() and np.isnan(vs.max_zfar)  # as torch's max


@pytest.fixture(scope="module")
def filled(ds):
    """One store for the read-side tests: 9 views of 19 x 37 (odd pixel count: no plane is 16-byte aligned) and 9 of 16 x 24, every kind present."""
    out = {}
    for name, (H, W) in (("odd", (19, 37)), ("vector", (16, 24))):
        rng = np.random.default_rng(H)
        infos = make_infos(rng, 9, H, W, {**ALL_F32, 0: (3, "u8"), 5: (1, "f32")})
        vs = ds.ViewSet(H, W, 10)
        vs.add(infos, views_per_call=4)
        out[name] = vs
    torch.cuda.synchronize()
    return out


GATHERS = [("one", [4], None), ("eight_repeats_descending", [8, 7, 7, 5, 3, 3, 1, 0], None), ("subset", [2, 0, 6], ("depth", "normal", "render")),
           ("only_depth", [1], ("depth",)), ("two_launches_65", [(7 * i + 3) % 9 for i in range(65)], ("diffuse", "roughness"))]


@pytest.mark.parametrize("which", ["odd", "vector"])
@pytest.mark.parametrize("name,idx,kinds", GATHERS, ids=[g[0] for g in GATHERS])
def test_gather_equals_the_stored_halfs(ds, filled, which, name, idx, kinds):
    vs = filled[which]
    got = vs.gather(idx) if kinds is None else vs.gather(idx, kinds)
    torch.cuda.synchronize()
    want_kinds = ds.KINDS if kinds is None else kinds
    assert set(got) == set(want_kinds) | {"R", "centers", "fovy"}
    sel = torch.tensor(idx, device="cuda")
    for k in want_kinds:
        plane = vs.planes[ds.KINDS.index(k)]
        assert got[k].dtype == torch.float32 and tuple(got[k].shape) == (len(idx),) + tuple(plane.shape[1:]) and got[k].is_contiguous()
        assert torch.equal(got[k].view(torch.int32), plane[sel].float().view(torch.int32)), k
        assert np.array_equal(got[k].cpu().numpy(), vr.gather(plane.cpu().numpy(), idx))
    assert torch.equal(got["R"], vs.R[sel]) and torch.equal(got["centers"], vs.centers[sel]) and torch.equal(got["fovy"], vs.fovy[sel])


def test_gather_refuses_bad_indices_and_leaves_its_buffers_alone(ds, filled):
    vs = filled["odd"]
    for bad in ([9], [0, -1], [], [3, 10]):  # 9 views are filled, the store has 10 slots
        with pytest.raises((IndexError, ValueError)):
            vs.gather(bad)
    with pytest.raises(RuntimeError, match="out of range"):  # the op checks again, before the launch
        torch.ops.egr.viewset_gather(vs.planes, vs._R, vs._centers, vs._fovy, 9, [9], [None] * 7, torch.empty((1, 3, 3), device="cuda"), torch.empty((1, 3), device="cuda"),
                                     torch.empty((1,), device="cuda"))
    # a larger buffer: only the first V rows are written
    out = {"depth": torch.full((4, 1, 19, 37), 7.25, device="cuda"), "R": torch.full((4, 3, 3), 7.25, device="cuda"), "centers": torch.full((4, 3), 7.25, device="cuda"),
           "fovy": torch.full((4,), 7.25, device="cuda")}
    got = vs.gather([5, 2], ("depth",), out)
    torch.cuda.synchronize()
    assert tuple(got["depth"].shape) == (2, 1, 19, 37) and torch.equal(got["depth"], vs.planes[3][[5, 2]].float())
    for t in out.values():
        assert bool((t[2:] == 7.25).all())


def test_camera_images_equal_the_gather(ds, filled):
    vs = filled["vector"]
    cam = vs.camera(6)
    got = vs.gather([6])
    for k, attr in zip(ds.KINDS, ds.CAMERA_ATTRS):
        img = getattr(cam, attr)
        assert img.dtype == torch.float32 and img.is_cuda and torch.equal(img.view(torch.int32), got[k][0].view(torch.int32)), attr
    assert torch.equal(cam.camera_center, got["centers"][0]) and np.array_equal(cam.R, got["R"][0].cpu().numpy()) and np.float32(cam.FoVy) == got["fovy"][0].item()
    assert float(cam.znear) == float(vs.znear[6]) and float(cam.zfar) == float(vs.zfar[6]) and (cam.image_height, cam.image_width) == (16, 24)


def dataset_pose(cam):
    """(R, T) of the dataset's convention for a synthetic camera (origin, blender c2w): renderer.camera_from_c2w's R, and T with -R T = origin."""
    R = np.asarray(cam["c2w"], np.float64).copy()
    R[:, 0] = -R[:, 0]
    R = -R
    return R, -R.T @ np.asarray(cam["origin"], np.float64)


def test_train_equals_train_views_on_the_sets_cameras(ds, ren, syn):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    m = rt.cuda_module
    m.get_config().jitter_primary_rays.fill_(True)
    tgs = view_targets(syn, W, H, 4)
    infos = []
    for c, tg in zip(views(syn, 4), tgs):
        R, T = dataset_pose(c)
        infos.append(SimpleNamespace(R=R, T=T, FovY=float(c["fov"]), **{k + "_image": v for k, v in tg.items()}))
    vs = ds.ViewSet(H, W, 4)
    vs.add(infos, views_per_call=3)
    assert vs.present == [False, True, True, True, True, True, True]
    idx = [2, 0, 3]
    cams = [vs.camera(i) for i in idx]
    pc = rt.pc
    fb, md, st = m.get_framebuffer(), m.get_metadata(), m.get_stats()
    raw = [p.clone() for p in pc.parameters()]
    sentinel = 7.25
    fb_names = list(ren.GaussianRaytracer.OUTPUT_BUFFERS) + ["output_denoised"] + ["target_" + k for k in ("diffuse", "specular", "depth", "normal", "roughness", "f0")]

    def run(call):
        zero_native(rt)
        for p in pc.parameters():
            p.grad.zero_()
        for n in fb_names:
            getattr(fb, n).fill_(sentinel)
        md.total_num_calls.fill_(23)
        call()
        torch.cuda.synchronize()
        for n in fb_names:
            assert bool((getattr(fb, n) == sentinel).all()), n  # the framebuffer is untouched
        for p, r in zip(pc.parameters(), raw):
            assert torch.equal(p, r)  # ... and so are the model's raw parameters
        assert int(m.get_counters()[11]) == 0
        return dict(native=hip_grads(rt), model=[p.grad.clone() for p in pc.parameters()], calls=int(md.total_num_calls), seeds=md.random_seeds.clone(),
                    acc=st.num_accumulated_per_pixel.clone(), trav=st.num_traversed_per_pixel.clone())

    want = run(lambda: ren.train_views(cams, rt))
    got = run(lambda: vs.train(idx, rt))
    again = run(lambda: vs.train(idx, rt))  # the staging buffers of the first call are reused
    for g in (got, again):
        assert g["calls"] == want["calls"] == 23 + 3
        assert torch.equal(g["seeds"], want["seeds"]) and torch.equal(g["acc"], want["acc"]) and torch.equal(g["trav"], want["trav"])
        assert_grads_close(g["native"], want["native"], "viewset_train_vs_train_views")  # gradients and total_weight: float atomics in another order
        for a, b in zip(g["model"], want["model"]):
            scale = float(b.abs().max())
            assert scale > 0 and float((a - b).abs().max()) / scale < 1e-5
    assert int(want["trav"].sum()) > 0
    one = run(lambda: vs.train([2], rt))  # three views are not one
    assert not np.allclose(one["native"]["dL_dmean"], want["native"]["dL_dmean"])
    # what train refuses
    with pytest.raises(ValueError):
        ds.ViewSet(H, W, 2).train([0], rt)  # an empty set
    with pytest.raises(IndexError):
        vs.train([4], rt)
    with pytest.raises(ValueError):
        vs.train([], rt)
    other = ds.ViewSet(H, W + 2, 1)
    other.add([SimpleNamespace(R=infos[0].R, T=infos[0].T, FovY=0.7, depth_image=np.ones((H, W + 2, 1), np.float32))])
    with pytest.raises(ValueError, match="the tracer renders"):
        other.train([0], rt)


def test_views_of_the_set_render_and_evaluate_like_any_camera(ds, ren, syn):
    W, H = 64, 48
    rt = tracer(ren, syn, W, H)
    ev = importlib.import_module(PKG + ".evaluation")
    tgs = view_targets(syn, W, H, 2)
    infos = []
    for c, tg in zip(views(syn, 2), tgs):
        R, T = dataset_pose(c)
        infos.append(SimpleNamespace(R=R, T=T, FovY=float(c["fov"]), image=(tg["diffuse"] + tg["specular"]).astype(np.float32), **{k + "_image": v for k, v in tg.items()}))
    vs = ds.ViewSet(H, W, 2)
    vs.add(infos)
    cams = vs.cameras()
    with torch.no_grad():
        single = ren.render(cams[1], rt)
        batch = ren.render_views(cams, rt, outputs=("final", "depth"))
    assert tuple(single.final.shape) == (1, 3, H, W) and torch.equal(single.target_depth, vs.planes[3][1].float()) and bool(torch.isfinite(batch[1].final).all())
    md = rt.cuda_module.get_metadata()
    plain = [ren.camera_from_RT(i.R, i.T, i.FovY, **{a: getattr(c, a) for a in ds.CAMERA_ATTRS}) for i, c in zip(infos, cams)]
    scores = []
    for side in (cams, plain):
        md.total_num_calls.fill_(5)
        scores.append(ev.evaluate_views(side, rt, spp=2, denoise=False))
    for name in ("final", "diffuse", "specular"):
        assert bool(torch.isfinite(scores[0].psnr[name]).all()) and torch.equal(scores[0].psnr[name], scores[1].psnr[name]), name


def test_prune_and_rebuild_takes_the_sets_tensors(ds, ren, syn):
    tr = importlib.import_module(PKG + ".trainer")
    N, W, H = 20000, 32, 32
    g = syn.make_scene(N, "trained", seed=4)
    pc = ren.GaussianParams(g)
    rt = ren.GaussianRaytracer(pc, W, H, team_help=False)
    step = tr.FusedTrainStep(pc, rt, dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3))
    xyz = pc._xyz.cpu().numpy().astype(np.float64)
    rng = np.random.default_rng(6)
    infos = []
    for row, near in ((123, 0.5), (4567, 0.4)):  # a camera next to a gaussian of the cloud; depth minimum near / 0.8, so znear = near up to rounding
        depth = rng.uniform(near / 0.8, 5.0, (H, W, 1)).astype(np.float32)
        depth[3, 5, 0] = near / 0.8
        infos.append(SimpleNamespace(R=np.eye(3), T=-(xyz[row] + 0.01), FovY=0.7, depth_image=depth))
    vs = ds.ViewSet(H, W, 3)
    vs.add(infos)
    centers, znear = vs.centers, vs.znear
    assert centers.is_cuda and znear.is_cuda and tuple(centers.shape) == (2, 3) and tuple(znear.shape) == (2,)
    c64, z64 = centers.cpu().numpy().astype(np.float64), znear.cpu().numpy().astype(np.float64)
    dist = np.linalg.norm(xyz[:, None, :] - c64[None], axis=2)
    assert not np.any(np.abs(dist - z64[None]) < 1e-5 * z64[None])  # no gaussian on a sphere's surface
    inside = np.any(dist < z64[None], axis=1)
    assert 10 < int(inside.sum()) < N // 2
    n_kept, _ = step.prune_and_rebuild(min_weight=0.0, interval=1, cam_centers=vs.centers, cam_znear=vs.znear)
    assert n_kept == N - int(inside.sum()) and pc._xyz.shape[0] == n_kept
    assert np.array_equal(pc._xyz.cpu().numpy(), xyz[~inside].astype(np.float32))  # the kept rows, in order
