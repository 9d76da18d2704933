"""Every entry point behind a busy stream and on a side stream ("Stream order"; INTEGRATION.md section 3: "Launches go to the current
PyTorch HIP stream", "No internal HIP streams", "nothing synchronises per iteration").

Every other GPU test calls the library on the idle default stream and synchronises before it looks. Here each case runs three times more: behind a stall on
the default stream (b), behind a stall on a side stream with the default stream idle (c) and - the context cases - dealt call by call over two side streams
(d). tests/stream_order.py has the method: stale state A, a stall, the fresh state B copied in stream order, the calls, clones of the outputs, and only then
a host wait; the result must be the plain run of B. Calls that INTEGRATION.md promises not to synchronise must return with the stall still pending; host
objects they were given are overwritten while it is."""
import ctypes as C
import importlib
import math

import numpy as np
import pytest

import hip_common
import stream_order as so
from hip_common import GRAD_KEYS, OUT_KEYS, generic_targets, ren, views  # noqa: F401 (fixture)
from stream_order import ASYNC, EITHER, SYNC, Case, DeviceInputs, run_case

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PKG = "editable-gaussian-reflections_amd"
N = 3000
TARGET_ORDER = ("diffuse", "specular", "depth", "normal", "roughness", "f0")  # the order of set_targets_chw / raytrace(targets=...) / train_views
TARGET_ATTRS = ("diffuse_image", "specular_image", "depth_image", "normal_image", "roughness_image", "f0_image")
GRAD_TOL = so.GRAD_TOL
CALLS = {"A": 3, "B": 7}  # total_num_calls before the first launch: other seeds for the stale and the fresh run
NV = 3


def cuda(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


def scene_tensors(syn, n, seed):
    g = syn.make_scene(n, "trained", seed=seed)
    return {k: cuda(g[k]).reshape(n, -1) for k in ("mean", "opacity", "scale", "rotation", "rgb", "normal", "roughness", "f0")}


PC_ATTRS = dict(mean="_xyz", opacity="_opacity", scale="_scaling", rotation="_rotation", rgb="_diffuse", normal="_normal", roughness="_roughness", f0="_f0")


class Ctx:
    """One tracer and the A / B values of everything its calls read: the model's eight parameter tensors (scenes of seeds 5 and 6), NV cameras each (R, centre as
    device tensors and as host arrays, fov as a host number) and six target images per camera."""

    def __init__(self, ren, syn, W, H, n=N):
        self.ren, self.W, self.H, self.n = ren, W, H, n
        self.rt = hip_common.tracer(ren, syn, W=W, H=H, N=n, seed=5, bwd=8_000_000)
        self.m, self.pc = self.rt.cuda_module, self.rt.pc
        self.m.set_batch_frames(2)  # batches of NV = 3 views cross a chunk boundary
        a, b = scene_tensors(syn, n, 5), scene_tensors(syn, n, 6)
        self.params = {"A": a, "B": b}
        cams = views(syn, 2 * NV)
        self.cams = {"A": cams[:NV], "B": cams[NV:]}
        self.dev_cams, self.targets = {}, {}
        rng = np.random.default_rng(17)
        for which in "AB":
            objs = [ren.camera_from_c2w(c["origin"], c["c2w"], c["fov"]) for c in self.cams[which]]
            self.dev_cams[which] = dict(R=torch.stack([o.R for o in objs]).contiguous(), centers=torch.stack([o.camera_center for o in objs]).contiguous(),
                                        fovy=torch.tensor([o.FoVy for o in objs], dtype=torch.float32).cuda())
            tg = generic_targets(syn, W, H)
            self.targets[which] = [torch.stack([cuda(tg[k] + 0.2 * rng.standard_normal(tg[k].shape).astype(np.float32)).moveaxis(-1, 0) for _ in range(NV)]).contiguous()
                                   for k in TARGET_ORDER]  # six [NV,C,H,W]
        # the buffers the calls are handed (persistent: `load` copies A or B into them, device to device)
        self.R, self.centers, self.fovy = (self.dev_cams["A"][k].clone() for k in ("R", "centers", "fovy"))
        self.images = [t.clone() for t in self.targets["A"]]
        self.hwc = [t[0].moveaxis(0, -1).contiguous() for t in self.images]  # view 0's targets pixel-major: their channel-major VIEWS are not contiguous
        torch.cuda.synchronize()

    def load(self, which, calls=None):
        for k, attr in PC_ATTRS.items():
            getattr(self.pc, attr).copy_(self.params[which][k])
        self.R.copy_(self.dev_cams[which]["R"]), self.centers.copy_(self.dev_cams[which]["centers"]), self.fovy.copy_(self.dev_cams[which]["fovy"])
        for t, src in zip(self.images, self.targets[which]):
            t.copy_(src)
        for t, src in zip(self.hwc, self.targets[which]):
            t.copy_(src[0].moveaxis(0, -1))
        self.m.get_metadata().total_num_calls.fill_((CALLS[which] if calls is None else calls) - 1)
        self.fov = float(self.cams[which][0]["fov"])

    def zero_grads(self):
        self.rt.zero_grad()
        self.m.get_gaussians().total_weight.zero_()
        for p in self.pc.parameters():
            p.grad.zero_()

    def export(self):
        with torch.no_grad():
            self.rt._export_param_values()

    def src8(self):
        pc = self.pc
        return [pc._get_scaling, pc._get_rotation, pc.get_xyz, pc._opacity, pc.get_diffuse, pc.get_normal, pc.get_roughness, pc.get_f0]

    def image_outputs(self):
        fb, st, md = self.m.get_framebuffer(), self.m.get_stats(), self.m.get_metadata()
        out = {k: getattr(fb, k).clone() for k in OUT_KEYS}
        out.update(num_accumulated=st.num_accumulated_per_pixel.clone(), num_traversed=st.num_traversed_per_pixel.clone(), random_seeds=md.random_seeds.clone())
        return out

    def grad_outputs(self, model=False):
        g = self.m.get_gaussians()
        out = {k: getattr(g, k).clone() for k in GRAD_KEYS}
        if model:
            out.update({"model" + attr: getattr(self.pc, attr).grad.clone() for attr in PC_ATTRS.values()})
        return out

    def raytrace(self, grads=False, *args):
        with torch.set_grad_enabled(grads):
            self.m.raytrace(*args)


@pytest.fixture(scope="module")
def ctx(ren, syn):
    return Ctx(ren, syn, 64, 48)


@pytest.fixture(scope="module")
def ctx_ragged(ren, syn):
    return Ctx(ren, syn, 42, 26)  # ragged 8x8 tiles, 1092 pixels


@pytest.fixture(scope="module")
def lib(ren):
    importlib.import_module(PKG).load_library()
    return torch.ops.egr


def pytest_generate_tests(metafunc):
    """(b) and (c) for every case; (d), two side streams, for the cases of the raytracer context (the raw C context is created on ONE stream handle)."""
    if "mode" in metafunc.fixturenames:
        context = {"ctx", "ctx_ragged"} & set(metafunc.fixturenames) or metafunc.function.__name__ in ("test_first_batch_calls_of_a_context", "test_rebuild_with_more_gaussians", "test_prune_grow_and_rebuild")
        metafunc.parametrize("mode", so.MODES if context else so.MODES[:2])


# ---------------------------------------------------------------------------------------------------------------- the context: camera, refit, no-grad launch
REFITS = ("update_bvh", "update_bvh_fuse_live", "update_bvh_from")


def refit_steps(c, how):
    m = c.m
    if how == "update_bvh_from":
        return [lambda: m.update_bvh_from(*c.src8(), True)]
    return [c.export, lambda: m.update_bvh(how == "update_bvh_fuse_live")]


@pytest.mark.parametrize("how", REFITS)
def test_set_camera_from_tensors_refit_and_render(ctx, how, mode):
    """set_camera from device tensors, the three refits and a no-grad raytrace: ten output buffers, both statistics images and random_seeds, bit for bit."""
    c = ctx
    steps = [lambda: c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9)] + refit_steps(c, how) + [lambda: c.raytrace(False)]
    run_case(Case(name="camera_tensors_" + how, kind=ASYNC, load=c.load, steps=lambda: steps, outputs=c.image_outputs), mode)


def test_ragged_image_refit_and_render(ctx_ragged, mode):
    c = ctx_ragged
    steps = [lambda: c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9), lambda: c.m.update_bvh_from(*c.src8(), True), lambda: c.raytrace(False)]
    run_case(Case(name="camera_tensors_42x26", kind=ASYNC, load=c.load, steps=lambda: steps, outputs=c.image_outputs), mode)


class HostCamera:
    """A camera as a dataset hands it over: R a numpy array, camera_center a CPU tensor over a numpy array - host memory the call must have read before it
    returns (it is overwritten with the stale camera right after)."""

    def __init__(self, c):
        self.host = {}
        for which in "AB":  # (made beforehand: nothing here may wait for the device once the stall is enqueued)
            self.host[which] = (c.dev_cams[which]["R"][0].cpu().numpy().copy(), c.dev_cams[which]["centers"][0].cpu().numpy().copy(), float(c.cams[which][0]["fov"]))

    def make(self, which):
        R, centre, fov = self.host[which]
        self.R, self.centre = R.copy(), centre.copy()
        return type("Camera", (), dict(R=self.R, camera_center=torch.from_numpy(self.centre), FoVy=fov))()

    def scribble(self):
        self.R[...] = self.host["A"][0]
        self.centre[...] = 0.0


def test_set_camera_from_numpy_through_the_renderer(ctx, mode):
    """GaussianRaytracer.__call__ with a host camera (numpy R, CPU camera_center), force_update_bvh. The pose travels to set_camera's launch by value: the call
    returns with the stall pending (an upload of the pageable arrays would wait for the stream, once per training iteration - it did, before this test), and
    the host arrays are overwritten while it still is."""
    c, hc, cam = ctx, HostCamera(ctx), {}

    def load(which):
        c.load(which)
        cam["camera"] = hc.make(which)

    def call():
        with torch.no_grad():
            c.rt(cam["camera"], force_update_bvh=True)

    run_case(Case(name="camera_numpy_renderer", kind=ASYNC, load=load, steps=lambda: [call], outputs=c.image_outputs, scribble=hc.scribble), mode)


def test_set_camera_from_cpu_tensors(ctx, mode):
    """Raytracer.set_camera with CPU tensors (read on the host, handed to the launch by value), then the fused refit and the launch."""
    c, hc, cam = ctx, HostCamera(ctx), {}

    def load(which):
        c.load(which)
        cam["camera"] = hc.make(which)

    steps = [lambda: c.m.set_camera(torch.from_numpy(hc.R), cam["camera"].camera_center, cam["camera"].FoVy, 0.01, 999.9), lambda: c.m.update_bvh_from(*c.src8(), True),
             lambda: c.raytrace(False)]
    run_case(Case(name="camera_cpu_tensors", kind=ASYNC, load=load, steps=lambda: steps, outputs=c.image_outputs, scribble=hc.scribble), mode)


def test_host_pose_leaves_the_bits_of_the_device_pose(ctx):
    """set_camera from device tensors, from host tensors, and mixed as upstream's Camera holds them (R a numpy array, camera_center on the GPU): the camera's
    three scalars and the frame traced from the bound pose (the pose itself is not readable: the rays' origins and directions are) hold the same bits; fp64
    host values are rounded as the device conversion rounds them."""
    c = ctx
    cam, fb = c.m.get_camera(), c.m.get_framebuffer()
    scalars, images = ("vertical_fov_radians", "znear", "zfar"), ("output_ray_origin", "output_ray_direction", "output_depth", "output_final")
    c.load("B")
    c.m.update_bvh_from(*c.src8(), True)
    R, centre = c.dev_cams["B"]["R"][1].clone(), c.dev_cams["B"]["centers"][1].clone()
    R64 = R.double().cpu() * (1.0 + 2.0 ** -30)  # (not representable in fp32)
    snapshots = []
    for r, cc in ((R, centre), (R.cpu(), centre.cpu()), (R.cpu(), centre), (R, centre.cpu()), (R64.cuda(), centre), (R64, centre.double().cpu()), (c.dev_cams["A"]["R"][0], centre)):
        for f in scalars:
            getattr(cam, f).fill_(7.25)
        c.m.get_metadata().total_num_calls.fill_(4)
        c.m.set_camera(r, cc, 0.77, 0.02, 555.5)
        c.raytrace(False)
        torch.cuda.synchronize()
        snapshots.append({**{f: getattr(cam, f).cpu().numpy().copy() for f in scalars}, **{f: getattr(fb, f).cpu().numpy().copy() for f in images}})
    assert snapshots[0]["vertical_fov_radians"][0] == np.float32(0.77) and snapshots[0]["zfar"][0] == np.float32(555.5)
    assert snapshots[6]["output_ray_direction"].tobytes() != snapshots[0]["output_ray_direction"].tobytes()  # (another pose is another frame)
    for k, base in ((1, 0), (2, 0), (3, 0), (5, 4)):
        for f in scalars + images:
            assert snapshots[k][f].tobytes() == snapshots[base][f].tobytes(), (k, f)


# ---------------------------------------------------------------------------------------------------------------- the context: grad launches
def device_camera(c, images):
    cam = type("Camera", (), {})()
    cam.R, cam.camera_center = c.R[0], c.centers[0]  # (views of the persistent buffers: they hold whatever `load` copied last)
    for attr, t in zip(TARGET_ATTRS, images):
        setattr(cam, attr, t)
    return cam


@pytest.mark.parametrize("form", ["uploaded_targets", "targets_in_place", "import_into"])
def test_grad_launch_through_the_renderer(ctx, form, mode):
    """ren.render in grad mode behind the stall, zero_grad inside the stream. uploaded: the targets are non-contiguous views, so the renderer takes
    set_targets_chw; in place: raytrace(targets=...), and the images are overwritten in stream order behind the launch (a legal write); import_into: the
    launch's gather also adds to the model's .grad tensors. Nine native gradient tensors (and the model's eight) within 1e-5 of each tensor's maximum."""
    c = ctx
    uploaded = form == "uploaded_targets"
    images = [t.moveaxis(-1, 0) for t in c.hwc] if uploaded else [t[0] for t in c.images]
    assert all(t.is_contiguous() for t in images) != uploaded  # (one image the launch cannot read in place sends all six through set_targets_chw)
    cam = device_camera(c, images)

    def load(which):
        c.load(which)
        cam.FoVy = c.fov
        c.zero_grads()

    def call():
        c.rt.import_grads = form == "import_into"
        try:
            c.ren.render(cam, c.rt)
        finally:
            c.rt.import_grads = True

    def scribble():
        for t in (c.hwc if uploaded else c.images):
            t.zero_()

    run_case(Case(name="grad_" + form, kind=ASYNC, tol=GRAD_TOL, load=load, steps=lambda: [call], outputs=lambda: c.grad_outputs(form == "import_into"), scribble=scribble), mode)


# ---------------------------------------------------------------------------------------------------------------- the context: batches, denoise, masks
VIEW_OUTPUTS = ("final", "rgb", "depth", "normal", "roughness", "f0")


def test_render_views(ctx, mode):
    """NV = 3 views x 2 samples in chunks of 2 frames (a chunk boundary inside a view), after the first call of the context: bit for bit."""
    c, got = ctx, {}

    def call():
        with torch.no_grad():
            got["bufs"] = c.m.render_views(c.R, c.centers, c.fovy, 0.01, 999.9, 2, list(VIEW_OUTPUTS))

    steps = [c.export, lambda: c.m.update_bvh(True), call]
    run_case(Case(name="render_views", kind=ASYNC, load=c.load, steps=lambda: steps, outputs=lambda: {k: t.clone() for k, t in zip(VIEW_OUTPUTS, got["bufs"])}), mode)


@pytest.mark.parametrize("imported", [False, True], ids=["native_gradients", "import_into"])
def test_train_views(ctx, imported, mode):
    """renderer.train_stacked_views (what train_views and ViewSet.train end in) on NV = 3 views in chunks of 2, targets read in place and overwritten behind it."""
    c = ctx

    def load(which):
        c.load(which)
        c.zero_grads()

    def call():
        c.rt.import_grads = imported
        try:
            c.ren.train_stacked_views(c.rt, c.R, c.centers, c.fovy, list(c.images))
        finally:
            c.rt.import_grads = True

    def scribble():
        for t in c.images:
            t.zero_()

    run_case(Case(name="train_views_" + ("import" if imported else "native"), kind=ASYNC, tol=GRAD_TOL, load=load, steps=lambda: [call], outputs=lambda: c.grad_outputs(imported),
                  scribble=scribble), mode)


@pytest.fixture(scope="module")
def denoise_inputs(ctx):
    """Random final images and unit normals of NV views, A and B."""
    H, W = ctx.H, ctx.W
    vals = {}
    for which, seed in (("A", 1), ("B", 2)):
        g = torch.Generator(device="cuda").manual_seed(seed)
        vals[which] = dict(final=(2 * torch.rand(NV, H, W, 3, device="cuda", generator=g) ** 2).contiguous(),
                           normal=torch.nn.functional.normalize(torch.randn(NV, 3, H, W, 3, device="cuda", generator=g), dim=-1).contiguous())
    return DeviceInputs(vals["A"], vals["B"])


def test_denoise(ctx, denoise_inputs, mode):
    """denoise() of the framebuffer's output_final guided by output_normal (both written in stream order behind the stall)."""
    c, d = ctx, denoise_inputs
    fb = c.m.get_framebuffer()

    def load(which):
        d.load(which)
        fb.output_final.copy_(d["final"][:1]), fb.output_normal.copy_(d["normal"][0])

    run_case(Case(name="denoise", kind=ASYNC, load=load, steps=lambda: [c.m.denoise], outputs=lambda: dict(denoised=fb.output_denoised.clone())), mode)


def test_denoise_views(ctx, denoise_inputs, mode):
    c, d, got = ctx, denoise_inputs, {}

    def call():
        got["out"] = c.m.denoise_views(d["final"], d["normal"])

    def scribble():  # (legal: behind the launch in stream order)
        d["final"].zero_()

    run_case(Case(name="denoise_views", kind=EITHER, load=d.load, steps=lambda: [call], outputs=lambda: dict(denoised=got["out"].clone()), scribble=scribble), mode)


def test_object_masks(ctx, mode):
    """Per-object coverage of one view: the membership words are a device input, the requested bits a host list (overwritten after the call). The binding uploads
    the field of view with a pageable copy: synchronising by design."""
    c, got = ctx, {}
    rng = np.random.default_rng(3)
    rows = DeviceInputs(dict(bits=cuda(rng.integers(0, 8, c.n), torch.int32)), dict(bits=cuda(rng.integers(0, 8, c.n), torch.int32)))
    bits = []

    def load(which):
        c.load(which)
        rows.load(which)
        bits[:] = [0, 1, 2] if which == "A" else [2, 0, 1]

    def call():
        with torch.no_grad():
            got["out"] = c.m.object_masks(c.R[0], c.centers[0], c.fov, 0.01, 999.9, rows["bits"], bits)

    def scribble():
        bits[:] = [0, 0, 0]
        rows["bits"].zero_()

    steps = [c.export, lambda: c.m.update_bvh(True), call]
    run_case(Case(name="object_masks", kind=SYNC, load=load, steps=lambda: steps, outputs=lambda: dict(zip(("masks", "hit", "top"), (t.clone() for t in got["out"]))),
                  scribble=scribble), mode)


# ---------------------------------------------------------------------------------------------------------------- the context: growth behind a stall
def fresh_pair(ren, syn, W=64, H=48):
    """Two contexts built alike: one for the plain runs, one whose FIRST call of a kind happens behind the stall."""
    return Ctx(ren, syn, W, H), Ctx(ren, syn, W, H)


def run_first_call(name, plain, stalled, steps_of, outputs_of, mode, tol=None, prepare=None, stale_steps_of=None):
    """A growth path (free and reallocate with work in flight) runs once per context, so the plain run of B and the stalled run of B use two contexts built alike.
    The stale state is what the construction left (scene A); such calls synchronise by design: the stall must be pending at entry. The stale answer the fresh one
    must be far from comes from the plain context: `stale_steps_of` before its first call (a render of the cloud before it grows), else the same steps once more
    with A afterwards."""
    name = f"{name}[{mode}]"
    dflt = [torch.cuda.default_stream()]

    def plain_run(which, steps):
        plain.load(which)
        if prepare:
            prepare(plain)
        so.run_steps(steps, dflt)
        out = outputs_of(plain)
        torch.cuda.synchronize()
        return so.to_host(out)

    torch.cuda.synchronize()
    stale = plain_run("A", stale_steps_of(plain)) if stale_steps_of else None
    want = plain_run("B", steps_of(plain))
    if stale is None:
        stale = plain_run("A", steps_of(plain))
    so.assert_far_apart(name, stale, want, tol)
    streams = so.streams_of(mode)
    ev = so.enqueue_stall(50.0, streams[0])
    with torch.cuda.stream(streams[0]):
        stalled.load("B")
        if prepare:
            prepare(stalled)
    assert not ev.query(), f"{name}: not exercised - the stall had drained before the call"
    last = so.run_steps(steps_of(stalled), streams, after=streams[0])
    with torch.cuda.stream(last):
        out = outputs_of(stalled)
    last.synchronize()
    torch.cuda.synchronize()
    so.assert_same(name, so.to_host(out), want, tol)


def test_first_batch_calls_of_a_context(ren, syn, mode):
    """The first render_views and the first train_views of a context allocate the batch buffers behind a device-wide wait: with a stall in flight, and off the
    default stream, the launches that follow must still see the inputs enqueued before them."""
    plain, stalled = fresh_pair(ren, syn)
    got = {}

    def steps_of(c):
        def render():
            with torch.no_grad():
                got[id(c)] = c.m.render_views(c.R, c.centers, c.fovy, 0.01, 999.9, 2, list(VIEW_OUTPUTS))
        return [c.export, lambda: c.m.update_bvh(True), render, lambda: c.ren.train_stacked_views(c.rt, c.R, c.centers, c.fovy, list(c.images))]

    def outputs_of(c):
        out = {k: t.clone() for k, t in zip(VIEW_OUTPUTS, got[id(c)])}
        out.update(c.grad_outputs(True))
        return out

    # (one tolerance for the case: the images of two launches are bit-equal, and 1e-5 of the maximum hides no stale scene - the gap to it is asserted)
    run_first_call("first_batch_calls", plain, stalled, steps_of, outputs_of, mode, tol=GRAD_TOL, prepare=lambda c: c.zero_grads())


def test_rebuild_with_more_gaussians(ren, syn, mode):
    """pc.__init__(scene of 3500) + rebuild_bvh(): resize, reserve, free and reallocate with work in flight, then a render of the new cloud."""
    plain, stalled = fresh_pair(ren, syn)
    bigger = syn.make_scene(3500, "trained", seed=6)

    def steps_of(c):
        def grow():
            c.pc.__init__(bigger)
            c.rt.rebuild_bvh()
        return [lambda: c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9), grow, lambda: c.raytrace(False)]

    before = lambda c: [lambda: c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9), lambda: c.raytrace(False)]  # the cloud of 3000, as built
    run_first_call("rebuild_3500", plain, stalled, steps_of, lambda c: c.image_outputs(), mode, stale_steps_of=before)
    assert stalled.m.get_gaussians().mean.shape[0] == 3500 and stalled.m.check_bvh() == 0


def test_partition_cycle_drops_the_task_order_cache(ctx, mode):
    """More than eight (rank, world) pairs: the ninth drops the cached task order tables behind a device-wide wait. Every rank's launch writes its own tiles; the
    framebuffer after each is kept."""
    c = ctx
    pairs = [(r, w) for w in (2, 3, 4, 5) for r in range(w)][:11]
    kept = []

    def load(which):
        c.load(which)
        for k in OUT_KEYS:
            getattr(c.m.get_framebuffer(), k).zero_()
        del kept[:]

    def launch(r, w):
        def step():
            c.m.set_partition(r, w)
            c.raytrace(False)
            kept.append(c.m.get_framebuffer().output_final.clone())
        return step

    steps = [lambda: c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9), lambda: c.m.update_bvh_from(*c.src8(), True)] + [launch(r, w) for r, w in pairs]
    try:
        run_case(Case(name="partition_cycle", kind=SYNC, load=load, steps=lambda: steps, outputs=lambda: {f"final_{i}": t for i, t in enumerate(kept)}), mode)
    finally:
        c.m.set_partition(0, 1)


def test_timing_on_a_side_stream(ctx):
    """enable_timing(True): the context's events are recorded on the caller's stream, whichever it is."""
    c = ctx
    s = so.side_streams()[0]
    torch.cuda.synchronize()
    c.m.enable_timing(True)
    try:
        with torch.cuda.stream(s):
            c.load("B")
            c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9)
            c.m.update_bvh_from(*c.src8(), True)
            c.raytrace(False)
        s.synchronize()
        ms, kernels = c.m.last_raytrace_ms(), c.m.last_kernel_ms()
        refit = c.m.last_update_bvh_ms()
    finally:
        c.m.enable_timing(False)
    print(f"REPORT stream_order_timing: raytrace_ms={ms:.4f} update_bvh_ms={refit:.4f} kernels={kernels}", flush=True)
    assert math.isfinite(ms) and ms > 0 and math.isfinite(refit) and refit > 0
    assert kernels and all(math.isfinite(t) and t > 0 for _, t in kernels), kernels


# ---------------------------------------------------------------------------------------------------------------- the C ABI through ctypes
def test_c_abi_context_on_the_callers_stream(ren, syn, mode):
    """c_abi.RawRaytracer (no torch shim) with stream = the stalled stream's handle: egr_update_bvh + egr_raytrace read the caller's buffers in stream order."""
    cabi = importlib.import_module(PKG + ".c_abi")
    W, H = 64, 48
    s = so.streams_of(mode)[0]
    cam = syn.default_camera()
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    T = {k: v.clone() for k, v in scene_tensors(syn, N, 5).items()}
    for k, w in (("dL_drgb", 3), ("dL_dnormal", 3), ("dL_df0", 3), ("dL_droughness", 1), ("dL_dopacity", 1), ("dL_dscale", 3), ("dL_dmean", 3), ("dL_drotation", 4), ("total_weight", 1)):
        T[k] = f32(N, w)
    defaults = dict(exp_power=3.0, alpha_threshold=0.005, transmittance_threshold=0.01, global_scale_factor=1.0, loss_weight_diffuse=5.0, loss_weight_specular=3.0,
                    loss_weight_depth=2.5, loss_weight_normal=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0, eps_forward_normalization=1e-12, eps_scale_grad=1e-12,
                    eps_ray_surface_offset=0.01, eps_min_roughness=0.01, reflection_invalid_normal_threshold=0.7, backfacing_invalid_normal_threshold=0.9, backfacing_max_dist=0.1)
    for k, v in defaults.items():
        T[k] = torch.tensor([v], dtype=torch.float32, device="cuda")
    T["accumulate_samples"], T["jitter_primary_rays"] = torch.zeros(1, dtype=torch.bool, device="cuda"), torch.ones(1, dtype=torch.bool, device="cuda")
    T["num_bounces"] = torch.full((1,), 2, dtype=torch.int32, device="cuda")
    c2w = cuda(cam["c2w"])
    T["origin"], T["rotation_c2w"], T["rotation_w2c"] = cuda(cam["origin"]), c2w.contiguous(), c2w.t().contiguous()
    T["vertical_fov_radians"], T["znear"], T["zfar"] = cuda([float(cam["fov"])]), cuda([0.01]), cuda([999.9])
    for k, w in (("output_rgb", 3), ("output_depth", 1), ("output_normal", 3), ("output_f0", 3), ("output_roughness", 1), ("output_transmittance", 1), ("output_total_transmittance", 1),
                 ("output_ray_origin", 3), ("output_ray_direction", 3), ("accumulated_rgb", 3), ("accumulated_transmittance", 1), ("accumulated_total_transmittance", 1),
                 ("accumulated_depth", 1), ("accumulated_normal", 3), ("accumulated_f0", 3), ("accumulated_roughness", 1)):
        T[k] = f32(3, H, W, w)
    T["output_final"], T["output_denoised"] = f32(1, H, W, 3), f32(1, H, W, 3)
    T["accumulated_sample_count"] = torch.zeros(1, dtype=torch.int32, device="cuda")
    for k, w in (("diffuse", 3), ("specular", 3), ("depth", 1), ("normal", 3), ("f0", 3), ("roughness", 1)):
        T["target_" + k] = f32(H, W, w)
    T["grads_enabled"], T["total_num_calls"] = torch.ones(1, dtype=torch.bool, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    T["random_seeds"] = torch.zeros(H, W, 1, dtype=torch.int32, device="cuda")
    T["num_accumulated_per_pixel"], T["num_traversed_per_pixel"] = torch.zeros(H, W, dtype=torch.int32, device="cuda"), torch.zeros(H, W, dtype=torch.int32, device="cuda")
    params = {"A": scene_tensors(syn, N, 5), "B": scene_tensors(syn, N, 6)}
    torch.cuda.synchronize()
    raw = cabi.RawRaytracer(W, H, N, {k: v.data_ptr() for k, v in T.items()}, ppll_forward_size=8_000_000, ppll_backward_size=8_000_000, device=torch.cuda.current_device(),
                            stream=s.cuda_stream)
    try:
        def load(which):
            for k, v in params[which].items():
                T[k].copy_(v)
            T["total_num_calls"].fill_(CALLS[which] - 1)

        keys = OUT_KEYS + ["random_seeds", "num_accumulated_per_pixel", "num_traversed_per_pixel"]
        plain = {}
        for which in ("B", "A"):  # (the raw context's stream is fixed: the plain runs use it idle)
            with torch.cuda.stream(s):
                load(which)
                raw.update_bvh(fuse_live=True)
                raw.raytrace(False)
                plain[which] = {k: T[k].clone() for k in keys}
            torch.cuda.synchronize()
            plain[which] = so.to_host(plain[which])
        so.assert_far_apart(f"c_abi_context[{mode}]", plain["A"], plain["B"], None)
        ev = so.enqueue_stall(30.0, s)
        with torch.cuda.stream(s):
            load("B")
            raw.update_bvh(fuse_live=True)
            raw.raytrace(False)
            pending = not ev.query()
            out = {k: T[k].clone() for k in keys}
        s.synchronize()
        assert pending, f"c_abi_context[{mode}]: not exercised - the stall was no longer pending when egr_raytrace returned"
        so.assert_same(f"c_abi_context[{mode}]", so.to_host(out), plain["B"], None)
    finally:
        torch.cuda.synchronize()
        raw.close()


def test_c_abi_prune_gather_table_is_read_before_the_call_returns(ren, mode):
    """egr_prune_gather through ctypes on the stalled stream: the table of (src, dst, width) entries is a host array, overwritten right after the call."""
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    n, count = 3 * 1024 + 17, 2049
    rng = np.random.default_rng(11)
    index = lambda: np.concatenate([np.sort(rng.permutation(n)[:count]), np.zeros(n - count, np.int64)])  # prune_select's list: n entries, the first `count` are the kept rows
    make = lambda: dict(a=cuda(rng.standard_normal((n, 3))), b=cuda(rng.integers(-9, 9, (n, 1)), torch.int32), index=cuda(index(), torch.int32))
    d = DeviceInputs(make(), make())
    out = dict(a=torch.zeros(count, 3, device="cuda"), b=torch.zeros(count, 1, dtype=torch.int32, device="cuda"))
    table = (cabi.egr_prune_array * 2)()

    def load(which):
        d.load(which)
        table[0] = cabi.egr_prune_array(src=d["a"].data_ptr(), dst=out["a"].data_ptr(), width=3)
        table[1] = cabi.egr_prune_array(src=d["b"].data_ptr(), dst=out["b"].data_ptr(), width=1)

    def call():
        rc = L.egr_prune_gather(torch.cuda.current_device(), table, 2, n, d["index"].data_ptr(), count, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, L.egr_prune_last_error()

    def scribble():
        C.memset(table, 0, C.sizeof(table))
        d["a"].zero_()

    run_case(Case(name="c_abi_prune_gather", kind=ASYNC, load=load, steps=lambda: [call], outputs=lambda: {k: t.clone() for k, t in out.items()}, scribble=scribble), mode)


# ---------------------------------------------------------------------------------------------------------------- context-free ops
def test_knn(ren, mode):
    knn = importlib.import_module(PKG + ".simple_knn")
    rng = np.random.default_rng(5)
    d = DeviceInputs(dict(p=cuda(rng.standard_normal((1025, 3)))), dict(p=cuda(rng.standard_normal((1025, 3)) * 2.0)))
    got = {}
    run_case(Case(name="distCUDA2", kind=SYNC, load=d.load, steps=lambda: [lambda: got.update(out=knn.distCUDA2(d["p"]))], outputs=lambda: dict(dist2=got["out"].clone())), mode)


def test_fused_adam_step(lib, mode):
    """G = 3 groups of n = 257 rows (widths 3, 1, 4). The learning rates, clamps and decays are host lists: overwritten while the stall is pending."""
    n, widths = 257, (3, 1, 4)
    rng = np.random.default_rng(257)

    def make():
        out = {}
        for g, w in enumerate(widths):
            out.update({f"p{g}": cuda(rng.standard_normal((n, w))), f"g{g}": cuda(rng.standard_normal((n, w)) * 1e-3), f"rp{g}": cuda(np.full((n, w), 777.0)),
                        f"rg{g}": cuda(rng.standard_normal((n, w)) * 1e-2), f"m{g}": cuda(rng.standard_normal((n, w)) * 1e-3), f"v{g}": cuda(rng.random((n, w)) * 1e-5 + 1e-9)})
        return out

    d = DeviceInputs(make(), make())
    host = {}

    def load(which):
        d.load(which)
        k = 1.0 if which == "A" else 2.0
        host.update(lrs=[1e-3 * k, 2e-3 * k, 5e-3 * k], lo=[-math.inf, 0.0, -math.inf], hi=[math.inf, 1.0, math.inf], decay=[1.0, 1.0, 0.999], steps=[], step=3 if which == "A" else 5)

    def call():
        col = lambda name: [d[f"{name}{g}"] for g in range(3)]
        lib.fused_adam_step(col("p"), col("g"), col("rp"), col("rg"), col("m"), col("v"), host["lrs"], host["lo"], host["hi"], host["decay"], host["step"], 0.9, 0.999, 1e-15,
                            host["steps"])

    def scribble():
        for k in ("lrs", "lo", "hi", "decay"):
            host[k][:] = [0.0] * 3

    run_case(Case(name="fused_adam_step", kind=ASYNC, load=load, steps=lambda: [call], outputs=lambda: {k: t.clone() for k, t in d.buf.items()}, scribble=scribble), mode)


def test_prune_select_and_gather(lib, mode):
    """All three criteria on 3 * 1024 + 17 rows and seven cameras; the survivor count is read back (the op's one synchronisation), so the sizes depend on the data."""
    n = 3 * 1024 + 17
    rng = np.random.default_rng(21)

    def make(keep):
        return dict(tw=cuda(rng.random(n) * 2.0 * keep), pts=cuda(rng.standard_normal((n, 3)) * 2.0), cc=cuda(rng.standard_normal((7, 3))), cz=cuda(rng.random(7) * 0.5 + 0.1),
                    mask=cuda(rng.random(n) < 0.1, torch.uint8), a=cuda(rng.standard_normal((n, 4))), b=cuda(rng.integers(-99, 99, (n, 1)), torch.int32))

    d = DeviceInputs(make(1.0), make(0.7))
    got = {}

    def call():
        index, count = lib.prune_select(d["tw"], 2.0, 0.25, d["pts"], d["cc"], d["cz"], d["mask"])
        k = int(count.item())
        got.update(count=count, index=index[:k], rows=lib.prune_gather([d["a"], d["b"]], index, k))

    outputs = lambda: dict(count=got["count"].clone(), index=got["index"].clone(), a=got["rows"][0].clone(), b=got["rows"][1].clone())
    run_case(Case(name="prune_select_gather", kind=SYNC, sizes_differ=True, load=d.load, steps=lambda: [call], outputs=outputs), mode)


def test_grow_sample_and_append(lib, mode):
    """Far-field candidates (seed and first index are host numbers) appended to two arrays, one with a tail of rows and one with a fill word."""
    n, m = 1025, 1023
    rng = np.random.default_rng(31)
    make = lambda: dict(a=cuda(rng.standard_normal((n, 3))), b=cuda(rng.integers(-99, 99, (n, 1)), torch.int32))
    d = DeviceInputs(make(), make())
    host, got = {}, {}

    def load(which):
        d.load(which)
        host.update(seed=750 if which == "A" else 751, fill=[0, 5 if which == "A" else 9])

    def call():
        tail = lib.grow_sample(0, m, host["seed"], 2.5, 3.0, torch.device("cuda"))
        got.update(tail=tail, out=lib.grow_append([d["a"], d["b"]], [tail, None], host["fill"], m))

    def scribble():
        host["fill"][:] = [0, 0]
        d["a"].zero_()

    outputs = lambda: dict(tail=got["tail"].clone(), a=got["out"][0].clone(), b=got["out"][1].clone())
    run_case(Case(name="grow_sample_append", kind=EITHER, load=load, steps=lambda: [call], outputs=outputs, scribble=scribble), mode)


def test_edit_select_and_apply(lib, mode):
    """Selection objects are a CPU tensor (a kernel argument: overwritten after the call), edit records live on the device."""
    ed = importlib.import_module(PKG + ".editing")
    cabi = importlib.import_module(PKG + ".c_abi")
    n = 3 * 1024 + 17
    rng = np.random.default_rng(41)
    boxes = {"A": {"left": dict(min=[-3.0, -3.0, -3.0], max=[0.0, 3.0, 3.0]), "everything": dict(min=[-9.0] * 3, max=[9.0] * 3)},
             "B": {"left": dict(min=[-0.5, -3.0, -3.0], max=[3.0, 3.0, 0.5]), "everything": dict(min=[-9.0] * 3, max=[9.0] * 3)}}
    edits = {"A": ed.Edit(translate_x=0.5, roughness_mult=0.5, diffuse_hue_shift=0.2), "B": ed.Edit(translate_y=-0.25, scale=1.5, rotate_z=30.0, specular_value_mult=0.5, diffuse_hue_shift=-0.4)}
    widths = dict(zip(cabi.EDIT_ARRAYS, cabi.EDIT_ARRAY_WIDTHS))

    def records(which):
        recs = [ed.pack_record(edits[which], boxes[which]["left"]), ed.pack_record(ed.Edit(roughness_shift=0.1 if which == "A" else 0.3), boxes[which]["everything"])]
        return ed._as_int32(recs, C.sizeof(cabi.egr_edit_record) // 4).cuda()

    def make(which):
        out = {k: cuda(rng.random((n, w)) if k in ("rgb", "roughness", "f0") else rng.standard_normal((n, w))) for k, w in widths.items()}
        out["records"] = records(which)
        return out

    d = DeviceInputs(make("A"), make("B"))
    dst = {k: torch.zeros(n, w, device="cuda") for k, w in widths.items()}
    host, got = {}, {}

    def load(which):
        d.load(which)
        names = list(boxes[which])
        host["objects"] = ed._as_int32([ed.pack_object(name, boxes[which][name], names) for name in names], C.sizeof(cabi.egr_edit_object) // 4)

    def call():
        got["mask"] = lib.edit_select(d["mean"], None, None, None, host["objects"])
        lib.edit_apply([d[k] for k in cabi.EDIT_ARRAYS], [dst[k] for k in cabi.EDIT_ARRAYS], got["mask"], d["records"])

    def scribble():
        host["objects"].zero_()
        d["records"].zero_()

    outputs = lambda: dict(mask=got["mask"].clone(), **{k: t.clone() for k, t in dst.items()})
    run_case(Case(name="edit_select_apply", kind=ASYNC, load=load, steps=lambda: [call], outputs=outputs, scribble=scribble), mode)


@pytest.fixture(scope="module")
def eval_inputs(ren):
    """Predictions and targets of NV views of 19 x 37 pixels (no plane is 16-byte aligned), A and B."""
    V, H, W = NV, 19, 37
    vals = {}
    for which, seed in (("A", 3), ("B", 4)):
        g = torch.Generator(device="cuda").manual_seed(seed)
        rnd = lambda *s: torch.rand(*s, device="cuda", generator=g)
        vals[which] = dict(final=(3 * rnd(V, H, W, 3) ** 2).contiguous(), rgb=(2 * rnd(V, 3, H, W, 3) ** 2).contiguous(), t_final=(3 * rnd(V, 3, H, W) ** 2).contiguous(),
                           t_diffuse=(2 * rnd(V, 3, H, W) ** 2).contiguous(), t_specular=(2 * rnd(V, 3, H, W) ** 2).contiguous())
    return DeviceInputs(vals["A"], vals["B"])


def test_eval_metrics(lib, eval_inputs, mode):
    d, got = eval_inputs, {}

    def call():
        got["out"] = lib.eval_metrics(d["final"], d["rgb"], d["t_final"], d["t_diffuse"], d["t_specular"], True)

    run_case(Case(name="eval_metrics", kind=ASYNC, load=d.load, steps=lambda: [call], outputs=lambda: dict(zip(("sse", "psnr", "display"), (t.clone() for t in got["out"]))),
                  scribble=lambda: d["final"].zero_()), mode)


def test_eval_ssim_and_ssim_images(lib, eval_inputs, mode):
    d, got = eval_inputs, {}

    def call():
        got["a"] = lib.eval_ssim(d["final"], d["rgb"], d["t_final"], d["t_diffuse"], d["t_specular"])
        got["b"] = lib.ssim_images(d["t_final"], d["t_diffuse"])

    outputs = lambda: dict(sum=got["a"][0].clone(), mean=got["a"][1].clone(), images_sum=got["b"][0].clone(), images_mean=got["b"][1].clone())
    run_case(Case(name="eval_ssim_ssim_images", kind=EITHER, load=d.load, steps=lambda: [call], outputs=outputs, scribble=lambda: d["t_final"].zero_()), mode)


def test_eval_frames(ren, eval_inputs, mode):
    """evaluation.frames: the 8-bit frames of three kinds, the exact integer sums and the 8-bit PSNRs."""
    ev = importlib.import_module(PKG + ".evaluation")
    ev.load_library()
    d, got = eval_inputs, {}

    def call():
        got["out"] = ev.frames(final=d["final"], rgb=d["rgb"], targets=dict(render=d["t_final"], diffuse=d["t_diffuse"], specular=d["t_specular"]), kinds=("render", "diffuse", "specular"))

    def outputs():  # (the slots of the kinds that were not selected are unspecified: render, diffuse and specular are kinds 0..2)
        out = got["out"]
        return dict(frames=out.frames[:, :3].clone(), sse8=out.sse8[:, :3].clone(), psnr8=out.psnr8[:, :3].clone())

    run_case(Case(name="eval_frames", kind=EITHER, load=d.load, steps=lambda: [call], outputs=outputs, scribble=lambda: d["rgb"].zero_()), mode)


def test_viewset_gather_and_train(ren, syn, ctx, mode):
    """ViewSet.train: one gather launch (the view indices are a host list, overwritten after the call) into staging buffers, then the batch launch in place."""
    ds = importlib.import_module(PKG + ".dataset")
    c = ctx
    from types import SimpleNamespace

    tg = generic_targets(syn, c.W, c.H)
    rng = np.random.default_rng(9)
    infos = []
    for cam in views(syn, 4):
        R = np.asarray(cam["c2w"], np.float64).copy()
        R[:, 0] = -R[:, 0]
        R = -R
        infos.append(SimpleNamespace(R=R, T=-R.T @ np.asarray(cam["origin"], np.float64), FovY=float(cam["fov"]),
                                     **{k + "_image": (v + 0.2 * rng.standard_normal(v.shape)).astype(np.float32) for k, v in tg.items()}))
    vs = ds.ViewSet(c.H, c.W, 4)
    vs.add(infos, views_per_call=3)
    torch.cuda.synchronize()
    idx = []

    def load(which):
        c.load(which)
        c.zero_grads()
        idx[:] = [2, 0, 3] if which == "A" else [1, 3, 0]

    def call():
        c.rt.import_grads = False
        try:
            vs.train(idx, c.rt)
        finally:
            c.rt.import_grads = True

    def scribble():
        idx[:] = [0, 0, 0]

    run_case(Case(name="viewset_train", kind=ASYNC, tol=GRAD_TOL, load=load, steps=lambda: [call], outputs=lambda: c.grad_outputs(False), scribble=scribble), mode)


def test_evaluate_and_export_views(ren, syn, ctx, mode):
    """evaluation.export_views(out_dir=None, views_per_call=1) over three cameras: three chunks, so both pinned buffers are filled twice between the stream, an event
    and the host copies. It waits for every chunk's copy (synchronising by design); what it returns must be the fresh scene's."""
    ev = importlib.import_module(PKG + ".evaluation")
    c, got = ctx, {}
    cams = []
    for v in range(NV):
        cam = type("Camera", (), {})()
        cam.R, cam.camera_center = c.R[v], c.centers[v]
        cam.original_image, cam.diffuse_image, cam.specular_image = c.images[0][v], c.images[0][v], c.images[1][v]
        cams.append(cam)

    def load(which):
        c.load(which)
        for v, cam in enumerate(cams):
            cam.FoVy = float(c.cams[which][v]["fov"])

    def call():
        got["res"] = ev.export_views(cams, c.rt, out_dir=None, spp=1, denoise=True, kinds=("render", "diffuse", "specular"), views_per_call=1)
        got["plain"] = ev.evaluate_views(cams, c.rt, spp=1, denoise=True, views_per_call=2)

    def outputs():
        res, out = got["res"], {}
        for v in range(NV):
            for kind, sides in sorted(res.frames[v].items()):
                for side, a in sorted(sides.items()):
                    out[f"frame{v}_{kind}_{side}"] = torch.from_numpy(a)
        for kind in ("render", "diffuse", "specular"):
            out["sse8_" + kind] = res.sse8[kind]
        for name in ("final", "diffuse", "specular"):
            out["psnr_" + name], out["evaluate_psnr_" + name] = res.psnr[name], got["plain"].psnr[name]
        return out

    run_case(Case(name="export_views", kind=SYNC, load=load, steps=lambda: [call], outputs=outputs), mode)


def test_voxel_accumulate_rehash_extract(lib, mode):
    """The dense-init cloud: two views of 19 x 37 pixels into a table of the smallest capacity, the table rehashed into one of twice the size, the voxels seen by
    at least two pixels extracted (coarse voxels, so that many pixels share one). Integer atomics: bit for bit; the row count depends on the data and
    voxel_extract reads it back."""
    cabi = importlib.import_module(PKG + ".c_abi")
    V, H, W, scale = 2, 19, 37, 6.0
    cap = max(cabi.EGR_VOXEL_MIN_CAPACITY, 4096)
    rng = np.random.default_rng(51)

    def make(spread):
        q = [np.linalg.qr(rng.standard_normal((3, 3)))[0] for _ in range(V)]
        return dict(c2w=cuda(np.stack(q), torch.float64), origin=cuda(rng.standard_normal((V, 3)) * 0.3, torch.float64), view=cuda(np.tan(rng.uniform(0.3, 0.45, V)), torch.float64),
                    depth=cuda(1.0 + spread * rng.random((V, H, W))), colour=cuda(rng.random((V, H, W, 3))))

    d = DeviceInputs(make(2.0), make(0.5))
    keys, acc, status = torch.empty(cap, dtype=torch.int64, device="cuda"), torch.empty(cap, 4, dtype=torch.int64, device="cuda"), torch.empty(cabi.EGR_VOXEL_STATUS_WORDS, dtype=torch.int64, device="cuda")
    keys2, acc2, status2 = torch.empty(2 * cap, dtype=torch.int64, device="cuda"), torch.empty(2 * cap, 4, dtype=torch.int64, device="cuda"), torch.empty_like(status)
    got = {}

    def load(which):
        d.load(which)
        keys.fill_(-1), acc.zero_(), status.zero_(), keys2.fill_(-1), acc2.zero_()

    def accumulate():
        lib.voxel_accumulate(keys, acc, status, d["c2w"], d["origin"], d["view"], d["depth"], d["colour"], None, scale, 32768.0, None)

    def rehash():
        status2.copy_(status)
        status2[0].zero_()  # the rehash counts the slots it claims
        lib.voxel_rehash(keys2, acc2, status2, keys, acc)

    def extract():
        got["out"] = lib.voxel_extract(keys2, acc2, status2, 2, scale, V * H * W)

    def outputs():
        coords, points, colors, counts, largest = got["out"]
        return dict(coords=coords.clone(), points=points.clone(), colors=colors.clone(), counts=counts.clone(), status=status2.clone(), largest=torch.tensor([largest]))

    run_case(Case(name="voxel_accumulate_rehash_extract", kind=SYNC, sizes_differ=True, load=load, steps=lambda: [accumulate, rehash, extract], outputs=outputs), mode)


def test_prepare_prior_views(ren, mode):
    """priors.prepare_prior_views (prior_pairs, prior_fit, prior_finish and the read-back between them) on the fixture's view: every input is host memory, uploaded
    by the call - synchronising by design; on a side stream the uploads, the three launches and the read-back must still be one stream-ordered chain."""
    from test_priors_host import GOLD
    from types import SimpleNamespace

    priors = importlib.import_module(PKG + ".priors")
    importlib.import_module(PKG).load_library()
    gold = dict(np.load(GOLD))
    host, got = {}, {}

    def load(which):
        k = 1.0 if which == "A" else 1.25
        host["info"] = SimpleNamespace(R=gold["view_R"].copy(), T=gold["view_T"].copy(), FovX=float(gold["view_fovx"]), FovY=float(gold["view_fovy"]),
                                       depth_image=(gold["view_depth"] * np.float32(k)).astype(np.float32), normal_image=gold["view_normal"].copy(),
                                       metalness_image=(gold["view_metalness"] * np.float32(2.0 - k)).astype(np.float32))
        host["points"] = gold["view_points"].copy() if which == "A" else gold["view_points"][:150].copy()
        host["seed"] = 3 if which == "A" else 4

    def call():
        got["rec"] = priors.prepare_prior_views([host["info"]], [host["points"]], seed=host["seed"])[0]

    def scribble():
        host["info"].depth_image[...] = 1.0
        host["points"][...] = 0.0

    def outputs():
        rec = got["rec"]
        fit = rec.depth_fit
        return dict(distance=rec.depth_image.clone(), normal=rec.normal_image.clone(), f0=rec.f0_image.clone(), a=torch.as_tensor(fit.a).clone().reshape(1), b=torch.as_tensor(fit.b).clone().reshape(1),
                    best_error=torch.as_tensor(fit.best_error).clone().reshape(1), pairs=torch.zeros(int(fit.num_pairs), dtype=torch.int8))

    run_case(Case(name="prepare_prior_views", kind=SYNC, sizes_differ=True, load=load, steps=lambda: [call], outputs=outputs, scribble=scribble), mode)


def test_prune_grow_and_rebuild(ren, syn, mode):
    """trainer.FusedTrainStep.prune_and_rebuild (camera spheres and a mask: one read-back, one gather, resize, rebuild) and add_farfield_points (sample, filter,
    append, rebuild) behind a stall, then a render of the new cloud. The row counts depend on the data; every reserve, free and reallocation happens with work
    in flight and, in modes (c) and (d), off the default stream. Three contexts built alike: the stale answer, the plain run and the stalled run."""
    tr = importlib.import_module(PKG + ".trainer")
    lrs = dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)
    stale, plain, stalled = (Ctx(ren, syn, 64, 48) for _ in range(3))
    rng = np.random.default_rng(61)
    masks = {"A": cuda(rng.random(N) < 0.05, torch.uint8), "B": cuda(rng.random(N) < 0.3, torch.uint8)}
    state = {}
    for c in (stale, plain, stalled):
        state[id(c)] = dict(step=tr.FusedTrainStep(c.pc, c.rt, lrs), mask=masks["A"].clone())
    torch.cuda.synchronize()

    def prepare(which):
        def run(c):
            s = state[id(c)]
            s["mask"].copy_(masks[which])
            s["seed"], s["znear"] = (750, 0.9) if which == "A" else (751, 1.2)
        return run

    def steps_of(c):
        s = state[id(c)]

        def prune():
            s["kept"], _ = s["step"].prune_and_rebuild(min_weight=0.0, interval=1, cam_centers=c.centers, cam_znear=s["znear"], remove_mask=s["mask"])

        def grow():
            s["added"], _ = s["step"].add_farfield_points(500, radius=3.0, seed=s["seed"], cam_centers=c.centers, cam_znear=s["znear"])

        return [prune, grow, lambda: c.m.set_camera(c.R[0], c.centers[0], c.fov, 0.01, 999.9), lambda: c.raytrace(False)]

    def outputs_of(c):
        out = c.image_outputs()
        out.update({attr: getattr(c.pc, attr).clone() for attr in PC_ATTRS.values()})
        out["exp_avg_xyz"] = state[id(c)]["step"].exp_avg["xyz"].clone()
        return out

    dflt = [torch.cuda.default_stream()]
    answers = {}
    for which, c in (("A", stale), ("B", plain)):
        c.load(which)
        prepare(which)(c)
        so.run_steps(steps_of(c), dflt)
        out = outputs_of(c)
        torch.cuda.synchronize()
        answers[which] = so.to_host(out)
    name = f"prune_grow_rebuild[{mode}]"
    so.assert_far_apart(name, answers["A"], answers["B"], None, sizes_differ=True)
    streams = so.streams_of(mode)
    ev = so.enqueue_stall(50.0, streams[0])
    with torch.cuda.stream(streams[0]):
        stalled.load("B")
        prepare("B")(stalled)
    assert not ev.query(), f"{name}: not exercised - the stall had drained before the call"
    last = so.run_steps(steps_of(stalled), streams, after=streams[0])
    with torch.cuda.stream(last):
        out = outputs_of(stalled)
    last.synchronize()
    torch.cuda.synchronize()
    so.assert_same(name, so.to_host(out), answers["B"], None)
    assert state[id(stalled)]["kept"] == state[id(plain)]["kept"] != state[id(stale)]["kept"] and stalled.m.check_bvh() == 0


def test_counters_and_debug_exports(ctx, mode):
    """get_counters and every debug_* export after a grad launch: each waits for the caller's stream and then copies through the NULL stream (synchronising by
    design). Behind a stall on a side stream the wait must be on THAT stream, or the copies read the stale launch's state."""
    c, got = ctx, {}
    cam = device_camera(c, [t[0] for t in c.images])

    def load(which):
        c.load(which)
        cam.FoVy = c.fov
        c.zero_grads()

    def launch():
        c.rt.import_grads = False
        try:
            c.ren.render(cam, c.rt)
        finally:
            c.rt.import_grads = True

    def exports():
        m = c.m
        counters = m.get_counters()  # rays, candidates, composited per step; status, tree depth; accepted per step (the lifetime counters and the byte and block counts go on counting)
        got.update(counters=torch.tensor(counters[:9] + counters[11:13] + counters[19:22]), step_hits=m.debug_step_hits(), hash=m.debug_hit_sequence_hash(), check=torch.tensor([m.check_bvh()]),
                   records=m.debug_backward_records())
        got.update({f"instances{i}": t for i, t in enumerate(m.debug_instances())})
        got.update({f"bvh_state{i}": t for i, t in enumerate(m.debug_bvh_state())})
        got.update({f"tree{i}": t for i, t in enumerate(m.debug_tree()) if i not in (5,)})  # (5: the collapse's rows carry three unused floats)

    run_case(Case(name="counters_and_debug_exports", kind=SYNC, load=load, steps=lambda: [launch, exports], outputs=lambda: dict(got)), mode)


def test_export_edited_through_the_renderer(ren, syn, mode):
    """editing.EditableGaussians behind the renderer: the edit records are packed on the host and uploaded when they changed (a pageable copy: synchronising),
    export_edited launches edit_apply from the raw parameters into the native tensors, the refit and a no-grad launch follow."""
    ed = importlib.import_module(PKG + ".editing")
    c = Ctx(ren, syn, 64, 48)
    eg = ed.EditableGaussians(c.pc, {"left": dict(min=[-3.0, -3.0, -3.0], max=[0.0, 3.0, 3.0]), "everything": dict(min=[-9.0] * 3, max=[9.0] * 3)})
    c.rt.pc = eg
    cam = device_camera(c, [None] * 6)
    torch.cuda.synchronize()

    def load(which):
        c.load(which)
        cam.FoVy = c.fov
        eg.edits["left"] = ed.Edit(translate_x=0.5, diffuse_hue_shift=0.2) if which == "A" else ed.Edit(translate_y=-0.25, scale=1.4, rotate_z=30.0, specular_value_mult=0.5)

    def call():
        with torch.no_grad():
            ed.render_edited(cam, c.rt, targets_available=False)

    run_case(Case(name="export_edited", kind=SYNC, load=load, steps=lambda: [call], outputs=c.image_outputs), mode)


def test_viewset_ingest_and_gather(ren, mode):
    """ViewSet.add (the images are host arrays: uploaded, then ONE ingest launch per chunk - here 2 + 1 views, resized 33 x 50 -> 32 x 48) and a gather of the
    stored halfs; the view indices of the gather are a host list."""
    ds = importlib.import_module(PKG + ".dataset")
    from types import SimpleNamespace

    attrs = ("image", "diffuse_image", "specular_image", "depth_image", "normal_image", "roughness_image", "f0_image")
    chans = (3, 3, 3, 1, 3, 1, 3)
    rng = np.random.default_rng(71)

    def infos():
        out = []
        for _ in range(3):
            q, _r = np.linalg.qr(rng.standard_normal((3, 3)))
            imgs = {a: (rng.integers(0, 256, (33, 50, ch), dtype=np.uint8) if a in ("image", "diffuse_image") else np.exp(rng.uniform(-3.0, 2.0, (33, 50, ch))).astype(np.float32))
                    for a, ch in zip(attrs, chans)}
            out.append(SimpleNamespace(R=q, T=rng.standard_normal(3) * 2.0, FovY=float(rng.uniform(0.5, 0.9)), **imgs))
        return out

    host, got, idx = {"A": infos(), "B": infos()}, {}, []

    def load(which):
        got["infos"] = host[which]
        idx[:] = [2, 0, 1, 1] if which == "A" else [1, 2, 2, 0]

    def call():
        vs = ds.ViewSet(32, 48, 3)
        vs.add(got["infos"], views_per_call=2)
        got["vs"], got["batch"] = vs, vs.gather(idx)

    def scribble():
        idx[:] = [0, 0, 0, 0]

    def outputs():
        vs = got["vs"]
        out = {f"plane{k}": p.clone() for k, p in enumerate(vs.planes)}
        out.update(depth_range=vs.depth_range.clone(), **{"gather_" + k: t.clone() for k, t in got["batch"].items()})
        return out

    run_case(Case(name="viewset_ingest_gather", kind=SYNC, load=load, steps=lambda: [call], outputs=outputs, scribble=scribble), mode)
