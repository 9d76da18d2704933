"""Grad launches that read the caller's target images where they are (Raytracer.raytrace(targets=...), egr_raytrace_targets) against the upload into the
framebuffer's pixel-major buffers followed by the plain launch.

One tracer, one launch index (total_num_calls: the same rays), three launches: (i) set_targets_chw + raytrace; (ii) the framebuffer's targets overwritten
with zeros, then a launch with the real targets in place; (iii) zeros in both places. The rays do not depend on the targets, so step hits, hit-sequence
hashes and statistics of (i) and (ii) are bit-equal; the gradients are two launches' - equal within 1e-5 of each tensor's maximum, the suite's bar for
float atomics in another order - and far from (iii)'s, which shows that (ii) read the caller's images and not the framebuffer's zeros.

Sizes: 40x24 (whole 8x8 tiles), 42x26 (ragged tiles), 41x23 (943 pixels, no multiple of 4: the flat upload cannot take it), and 40x24 as rank 1 of 2."""
import numpy as np
import pytest

from hip_common import GRAD_KEYS, cam_obj, hip_grads, ren, report, torch, tracer  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu

ORDER = ("diffuse", "specular", "depth", "normal", "roughness", "f0")  # the order of set_targets_chw and of raytrace(targets=...)
K = 4  # the launch index of every launch here
CASES = {"40x24": (40, 24, None), "42x26_ragged": (42, 26, None), "41x23_odd_pixel_count": (41, 23, None), "40x24_rank_1_of_2": (40, 24, (1, 2))}


def images_of(syn, W, H, seed=6):
    """Six channel-major images, contiguous fp32 on the GPU: the synthetic targets plus noise (no pixel equals a rendered value or a neighbour)."""
    rng = np.random.default_rng(seed)
    tg = syn.make_targets(W, H)
    return [torch.tensor(tg[k] + 0.2 * rng.standard_normal(tg[k].shape).astype(np.float32)).cuda().moveaxis(-1, 0).contiguous() for k in ORDER]


def prepared(ren, syn, W, H, part=None):
    rt = tracer(ren, syn, W=W, H=H, bwd=8_000_000, team_help=False)
    m = rt.cuda_module
    camera = cam_obj(ren, syn.default_camera())
    with torch.no_grad():
        rt._export_param_values()
        m.set_camera(camera.R, camera.camera_center, float(camera.FoVy), 0.01, 999.9)
    if part:
        m.set_partition(*part)
    return rt, m, camera


def launch(rt, m, uploaded, in_place):
    """One grad launch at launch index K. `uploaded`: six images (or None) for set_targets_chw; `in_place`: None, or six for raytrace(targets=...)."""
    rt.zero_grad()
    m.get_gaussians().total_weight.zero_()
    m.get_metadata().total_num_calls.fill_(K - 1)
    m.update_bvh(True)
    m.set_targets_chw(*uploaded)
    with torch.enable_grad():
        if in_place is None:
            m.raytrace()
        else:
            m.raytrace(None, in_place)
    torch.cuda.synchronize()
    c = m.get_counters()
    assert c[11] == 0
    st = m.get_stats()
    return dict(grads=hip_grads(rt), hits=m.debug_step_hits().numpy(), seq=m.debug_hit_sequence_hash().numpy(), rays=tuple(c[0:3]),
                acc=st.num_accumulated_per_pixel.cpu().numpy(), trav=st.num_traversed_per_pixel.cpu().numpy())


def fb_targets(m):
    fb = m.get_framebuffer()
    return [getattr(fb, "target_" + k).clone() for k in ORDER]


def assert_same_rays(a, b):
    for k in ("hits", "seq", "acc", "trav"):
        assert np.array_equal(a[k], b[k]), k
    assert a["rays"] == b["rays"]


def grad_distance(a, b):
    """max |a - b| over max |b|, per gradient tensor."""
    return {k: float(np.abs(a["grads"][k].astype(np.float64) - b["grads"][k]).max() / np.abs(b["grads"][k]).max()) for k in GRAD_KEYS}


@pytest.mark.parametrize("case", sorted(CASES))
def test_in_place_launch_equals_upload_and_launch(ren, syn, case):
    W, H, part = CASES[case]
    rt, m, _ = prepared(ren, syn, W, H, part)
    imgs = images_of(syn, W, H)
    kept = [t.clone() for t in imgs]
    none6 = [None] * 6
    classic = launch(rt, m, imgs, None)  # (i)
    in_place = launch(rt, m, none6, imgs)  # (ii)
    fb_after = fb_targets(m)
    zeros = launch(rt, m, none6, none6)  # (iii)
    assert classic["rays"][0] > 0 and classic["hits"].sum() > 0 and all(np.abs(classic["grads"][k]).max() > 0 for k in GRAD_KEYS)
    if part is None:
        assert classic["rays"][0] == W * H
    assert_same_rays(classic, in_place)
    assert_same_rays(classic, zeros)
    d = grad_distance(in_place, classic)
    far = grad_distance(in_place, zeros)
    report("targets_in_place_" + case, **{k: f"{v:.1e}" for k, v in d.items()}, dL_drgb_vs_zero_targets=f"{far['dL_drgb']:.1e}")
    for k, v in d.items():
        assert v <= 1e-5, (case, k, v)
    assert far["dL_drgb"] > 1e-2, far
    for k, t in zip(ORDER, fb_after):  # the framebuffer's targets are still the zeros of (ii): the launch wrote nothing there
        assert not bool(t.any()), k
    for k, t, t0 in zip(ORDER, imgs, kept):  # ... and the caller's images are as they were
        assert torch.equal(t, t0), k


def test_absent_targets_read_zero_like_the_upload(ren, syn):
    W, H = 42, 26
    rt, m, _ = prepared(ren, syn, W, H)
    imgs = images_of(syn, W, H)
    some = [imgs[0], None, imgs[2], None, None, imgs[5]]
    classic = launch(rt, m, some, None)
    in_place = launch(rt, m, [None] * 6, some)
    assert_same_rays(classic, in_place)
    for k, v in grad_distance(in_place, classic).items():
        assert v <= 1e-5, (k, v)
    other = launch(rt, m, [None] * 6, [None, imgs[1], None, imgs[3], imgs[4], None])  # the complement: another loss
    assert grad_distance(other, classic)["dL_drgb"] > 1e-2


def test_the_binding_refuses_what_it_cannot_read_in_place(ren, syn):
    W, H = 40, 24
    rt, m, _ = prepared(ren, syn, W, H)
    imgs = images_of(syn, W, H)
    before = int(m.get_metadata().total_num_calls)
    m.update_bvh(True)
    with torch.enable_grad():
        for k, bad, words in ((0, imgs[0].cpu(), r"raytrace: target 'diffuse' .* on cuda:\d+, got .* on cpu"), (3, imgs[3].double(), "raytrace: target 'normal' .* contiguous Float tensor .*, got Double"),
                              (5, imgs[5].moveaxis(0, -1).contiguous().moveaxis(-1, 0), r"raytrace: target 'f0' .* contiguous Float tensor .*\(not contiguous\)"),
                              (2, imgs[0], "channel-major"), (4, imgs[4][:, :, : W - 1].contiguous(), "channel-major")):
            with pytest.raises(RuntimeError, match=words):
                m.raytrace(None, imgs[:k] + [bad] + imgs[k + 1:])
        with pytest.raises(RuntimeError, match="six targets expected"):
            m.raytrace(None, imgs[:5])
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="targets need grad mode"):
            m.raytrace(None, imgs)
    torch.cuda.synchronize()
    assert int(m.get_metadata().total_num_calls) == before  # nothing was launched


def test_a_bare_grad_launch_after_an_in_place_one_finds_the_targets_in_the_framebuffer(ren, syn):
    """The reference's caller leaves its targets in framebuffer.target_*, and raytrace() without arguments reads them there. After raytrace(targets=...) the
    buffers are behind the images; the binding remembers the images and uploads them in front of the next grad raytrace() that has none of its own."""
    W, H = 42, 26
    rt, m, _ = prepared(ren, syn, W, H)
    imgs = images_of(syn, W, H)
    hwc = [t.moveaxis(0, -1).contiguous() for t in imgs]
    none6 = [None] * 6
    classic = launch(rt, m, imgs, None)
    launch(rt, m, none6, imgs)  # in place: the framebuffer holds zeros
    assert all(not bool(t.any()) for t in fb_targets(m))
    rt.zero_grad()
    m.get_gaussians().total_weight.zero_()
    m.get_metadata().total_num_calls.fill_(K - 1)
    with torch.no_grad():
        m.raytrace()  # (a no-grad launch reads no target: nothing is uploaded for it)
    assert all(not bool(t.any()) for t in fb_targets(m))
    m.get_metadata().total_num_calls.fill_(K - 1)
    with torch.enable_grad():
        m.raytrace()
    torch.cuda.synchronize()
    for k, t, want in zip(ORDER, fb_targets(m), hwc):
        assert torch.equal(t, want), k
    for k, v in grad_distance(dict(grads=hip_grads(rt)), classic).items():
        assert v <= 1e-5, (k, v)
    # ... once: set_targets_chw (here: zeros) is the caller's word again, and a bare launch reads that
    after_zeros = launch(rt, m, none6, None)
    assert all(not bool(t.any()) for t in fb_targets(m))
    assert grad_distance(after_zeros, classic)["dL_drgb"] > 1e-2


@pytest.mark.parametrize("part", [None, (1, 2)], ids=["whole_image", "rank_1_of_2"])
def test_the_renderer_reads_cuda_targets_in_place_and_uploads_the_others(ren, syn, part):
    """GaussianRaytracer.__call__ in grad mode: contiguous CUDA images go to the launch (the framebuffer's targets keep what they held), a CPU or a
    non-contiguous image takes set_targets_chw (the framebuffer then holds the images) - with the same gradients."""
    W, H = 42, 26
    rt, m, camera = prepared(ren, syn, W, H, part)
    imgs = images_of(syn, W, H)
    names = ("target_diffuse", "target_specular", "target_depth", "target_normal", "target_roughness", "target_f0")
    hwc = [t.moveaxis(0, -1).contiguous() for t in imgs]

    def call(images):
        rt.zero_grad()
        m.get_gaussians().total_weight.zero_()
        m.set_targets_chw(*[None] * 6)
        m.get_metadata().total_num_calls.fill_(K - 1)
        with torch.enable_grad():
            rt(camera, **dict(zip(names, images)))
        torch.cuda.synchronize()
        assert m.get_counters()[11] == 0
        return dict(grads=hip_grads(rt)), fb_targets(m)

    in_place, fb = call(imgs)
    assert all(not bool(t.any()) for t in fb)  # no upload: still the zeros
    results = {}
    for name, images in (("cpu_target", [imgs[0].cpu()] + imgs[1:]), ("non_contiguous_target", imgs[:3] + [hwc[3].moveaxis(-1, 0)] + imgs[4:])):
        results[name], fb = call(images)
        if part is None:  # (a rank uploads the pixels of its own tiles only)
            for k, t, want in zip(ORDER, fb, hwc):
                assert torch.equal(t, want), (name, k)
        else:
            assert all(bool(t.any()) for t in fb), name
    for name, r in results.items():
        for k, v in grad_distance(in_place, r).items():
            assert v <= 1e-5, (name, k, v)
